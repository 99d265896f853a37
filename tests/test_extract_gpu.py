"""Adapter extraction on the MI355X: sdlt_delta_matmul (ops.delta_matmul / ops.DeltaPlan) element-wise against the fp64 product under the
fp32 summation bound, bitwise repeatable, one launch per product for the SDXL layer set; exact recovery, truncation quality and `energy`
with the yardsticks of tests/extract_ref.py; the round trip train -> merge -> extract -> render loader through the command line, and the
real topologies' merged adapters recovered and run."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import extract_ref as XR
from tests.test_merge_cpu import SHAPES

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PAIRS = [(BF, BF), (F16, F16), (F32, F32), (BF, F32), (F16, BF), (F32, F16)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def _rt():
    import sd_lora_trainer_amd.unet as M
    return M.Runtime("cuda:0", 1)


def _pair(N, K, seed, d0, d1):
    g = torch.Generator().manual_seed(seed)
    W0 = (torch.randn(N, K, generator=g) * 0.02).to(d0)
    W1 = (W0.float() + torch.randn(N, K, generator=g) * 0.004).to(d1)
    return W0, W1


@pytest.mark.parametrize("L", [16, 80, 272])
def test_kernel_meets_fp32_bound(ops, L):
    """Linear, conv (K = 9 Cin), ragged and stacked q|k|v row slices, every dtype pairing, both orientations in ONE launch; every element
    within gamma_R sum |D| |X| of the fp64 product (gamma_{R+1} where the fp32 difference rounds: tests/extract_ref.py), the
    element-load path (ragged K, unaligned views) included; a second launch gives the same bits; rowsq = the rows' sums of squares."""
    host, items = [], []
    g = torch.Generator().manual_seed(L)
    cases = [(N, K, *_pair(N, K, 100 * L + i, *PAIRS[i % 6]), f"{N}x{K}") for i, (N, K) in enumerate(SHAPES)]
    N, K = 320, 320
    st0 = torch.cat([_pair(N, K, 7 + m, BF, BF)[0] for m in range(3)], 0)
    st1 = (st0.float() + torch.randn(3 * N, K, generator=g) * 0.004).to(F16)
    d0, d1 = st0.cuda(), st1.cuda()
    dev_of = {}
    for m in range(3):
        cases.append((N, K, st0[m * N:(m + 1) * N], st1[m * N:(m + 1) * N], f"stacked member {m}"))
        dev_of[len(cases) - 1] = (d0[m * N:(m + 1) * N], d1[m * N:(m + 1) * N])
    # the element-load path: K not a multiple of 8, a column-offset view (base not 16-byte aligned) and an odd row stride
    cases.append((100, 77, *_pair(100, 77, 900 + L, BF, BF), "100x77"))
    cases.append((100, 77, *_pair(100, 77, 901 + L, F32, F16), "100x77"))
    for j, (d0_, d1_, c0, ld) in enumerate([(BF, BF, 3, 96), (F16, F32, 1, 96), (BF, BF, 0, 81), (F32, F32, 0, 83)]):
        N, K = 72, 80
        b0, b1 = _pair(N, ld, 910 + 10 * j + L, d0_, d1_)
        g0, g1 = b0.cuda(), b1.cuda()
        cases.append((N, K, b0[:, c0:c0 + K], b1[:, c0:c0 + K], f"72x80 view at column {c0} of ld {ld}"))
        dev_of[len(cases) - 1] = (g0[:, c0:c0 + K], g1[:, c0:c0 + K])
    for i, (N, K, W0, W1, what) in enumerate(cases):
        w0d, w1d = dev_of.get(i, (None, None))
        w0d = W0.cuda() if w0d is None else w0d
        w1d = W1.cuda() if w1d is None else w1d
        for tr in (False, True):
            X = torch.randn(N if tr else K, L, generator=g)
            Y = torch.full((K if tr else N, L), float("nan"), device="cuda")
            rs = None if tr else torch.full((N,), float("nan"), device="cuda")
            items.append(dict(W0=w0d, W1=w1d, X=X.cuda(), Y=Y, transposed=tr, rowsq=rs))
            host.append((W0, W1, X, tr, Y, rs, f"L={L} {what} {W0.dtype}/{W1.dtype} {'T' if tr else 'N'}"))
    keep = ops.delta_matmul(items)
    torch.cuda.synchronize()
    first = [it["Y"].clone() for it in items]
    for it in items:
        it["Y"].fill_(float("nan"))
    keep2 = ops.delta_matmul(items)
    torch.cuda.synchronize()
    del keep, keep2
    for (W0, W1, X, tr, Y, rs, what), y1 in zip(host, first):
        assert torch.equal(Y, y1), f"{what}: two runs differ"
        ref, b = XR.product_bound(W0, W1, X, tr)
        err = (Y.double().cpu() - ref).abs()
        n, worst = int((~(err <= b)).sum()), float((err / b.clamp(min=1e-300)).max())
        print(f"{what}: worst err/bound {worst:.3g}")
        assert n == 0, f"{what}: {n} elements outside the bound (worst err/bound {worst:.3g})"
        if rs is not None:
            D = (W1.double() - W0.double())
            ss = (D * D).sum(1)
            assert bool(((rs.double().cpu() - ss).abs() <= XR.gamma(D.shape[1] + 3) * ss).all()), f"{what}: rowsq"


def test_sdxl_extraction_is_one_launch_per_product(ops, monkeypatch):
    from sd_lora_trainer_amd import extract as X
    from sd_lora_trainer_amd import topology
    cfg = topology.CONFIGS["sdxl"]
    shapes = topology.param_shapes(cfg)
    targets = topology.lora_targets(cfg)
    assert len(targets) == 577
    g = torch.Generator(device="cuda").manual_seed(0)
    base = {n + ".weight": (torch.randn(shapes[n + ".weight"], generator=g, device="cuda") * 0.02).to(BF) for n in targets}
    tuned = {k: (v.float() + 0.002 * torch.randn(v.shape, generator=g, device="cuda")).to(BF) for k, v in base.items()}
    lib = ops._lib.load()
    calls, real = [], lib.sdlt_delta_matmul

    def wrapped(*a):
        calls.append(a[4])
        return real(*a)
    monkeypatch.setattr(lib, "sdlt_delta_matmul", wrapped)
    q = 1
    ex = X.extract_adapters(base, tuned, 16, power_iters=q, runtime=_rt(), targets=targets)
    torch.cuda.synchronize()
    assert calls == [32] * (2 * q + 2), f"sdlt_delta_matmul calls for {len(targets)} layers: {calls}"
    assert len(ex.lora) == 577 and all(torch.isfinite(a).all() and torch.isfinite(b).all() for a, b in list(ex.lora.values())[:8])
    assert abs(ex.coverage - 1.0) <= 1e-12 and 0.0 < ex.residuals()["overall"] < 1.0


@pytest.mark.parametrize("rank", [4, 16, 64, 128])
def test_exact_recovery_gpu(ops, rank):
    from sd_lora_trainer_amd import extract as X
    from tests.test_extract_cpu import merged_case, shapes2d
    rt = _rt()
    base, tuned, lora = merged_case(rt, rank, seed=10 * rank)
    names = list(lora)
    ex = X.extract_adapters(base, tuned, rank, seed=5, runtime=rt, targets=names)
    L = X.padded_columns(rank, 16)
    om = XR.omegas_by_name(names, shapes2d(base, names), L, 5)
    XR.check_recovery(ex, base, tuned, lora, rank, L, om, 2, f"gpu r={rank}")
    assert abs(ex.coverage - 1.0) <= 1e-12


def test_truncation_quality_gpu(ops):
    """(b): the HIP path's residual, same Omega, exceeds the fp64 restatement's by no more than the fp32 bound (figures printed)."""
    from sd_lora_trainer_amd import extract as X
    from tests.test_extract_cpu import DECAY, Q_T, RANK_T, _spectrum_case, shapes2d
    base, tuned, sig = _spectrum_case()
    names = list(sig)
    L = X.padded_columns(RANK_T, 16)
    om = XR.omegas_by_name(names, shapes2d(base, names), L, 0)
    ex = X.extract_adapters(base, tuned, RANK_T, power_iters=Q_T, seed=0, runtime=_rt(), targets=names)
    for n in names:
        D = XR.delta64(XR.view2d(base[n + ".weight"]), XR.view2d(tuned[n + ".weight"]))
        A, B, _ = XR.extract_ref(D, om[n], RANK_T, Q_T)
        res_ref = float((D - B @ A).norm())
        opt = float((sig[n][RANK_T:] ** 2).sum().sqrt())
        A2, B2 = ex.lora[n]
        res = float((D - XR.product2d(A2, B2)).norm())
        allow = res_ref + XR.fp32_bound(D, L, XR.view2d(A2), XR.view2d(B2))
        print(f"truncation r={RANK_T} p={L - RANK_T} q={Q_T} decay={DECAY} {n}: HIP {res:.6e}  restatement {res_ref:.6e}  optimal {opt:.6e}  allowance {allow:.6e}")
        assert res <= allow


def test_energy_gpu(ops):
    from sd_lora_trainer_amd import extract as X
    from tests.test_extract_cpu import RANK_T, _spectrum_case
    base, tuned, sig = _spectrum_case()
    ex = X.extract_adapters(base, tuned, RANK_T, energy=0.9, seed=0, runtime=_rt(), targets=list(sig))
    for n, s in sig.items():
        s2 = s ** 2
        expect = int((torch.cumsum(s2, 0) < 0.9 * s2.sum()).sum()) + 1
        assert ex.layers[n]["kept"] == expect
        A, B = ex.lora[n]
        assert not XR.view2d(A)[expect:].any() and not XR.view2d(B)[:, expect:].any() and XR.view2d(A)[expect - 1].any()


def _inputs(cfg, h, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, h, h, generator=g)
    ctx = torch.randn(1, 77, cfg["cross_dim"], generator=g)
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    pooled = torch.randn(1, P, generator=g) if P else None
    tid = torch.tensor([[8. * h, 8. * h, 0, 0, 8. * h, 8. * h]]) if P else None
    emb = (torch.randn(1, 77, cfg["cross_dim"], generator=g), torch.randn(1, 77, cfg["cross_dim"], generator=g),
           torch.randn(1, P, generator=g) if P else None, torch.randn(1, P, generator=g) if P else None)
    return x, ctx, pooled, tid, emb, torch.randn(1, 4, h, h, generator=g)


def _compare(version, base, original, extracted, rank, h=32):
    """The engine with the EXTRACTED adapters against the original checkpoint's prediction and 8-step CFG render, taken - as
    tests/test_merge_gpu.py takes them for the merged model - from the fp32 oracle with the ORIGINAL adapters, under that file's bars.
    Engine against engine sits at the bf16 path's noise floor (any re-rounding of the same product B A into the bf16 adapter operands moves
    an sd15 render to cos 0.9994 against itself), so it would measure two realisations of that noise and not the extraction."""
    import sd_lora_trainer_amd.unet as M
    from oracle import sampler_ref as SR
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import sampler as SM
    from sd_lora_trainer_amd import topology
    from tests.test_step_gpu import _cos_rel
    cfg, ocfg = topology.CONFIGS[version], U.CONFIGS[version]
    x, ctx, pooled, tid, emb, noise = _inputs(cfg, h, 5)
    add = {"text_embeds": pooled, "time_ids": tid} if pooled is not None else None
    with torch.no_grad():
        ref = U.unet_forward(ocfg, base, x, torch.tensor([500]), ctx, add, lora=original, lora_scale=1.0)
        lat_o = SR.sample_latents(ocfg, base, original, 1.0, emb, noise, 8, guidance_scale=8.0)
    rt1 = M.Runtime("cuda:0", 1)
    unet1 = M.UNet(rt1, cfg, base, lora_rank=rank)
    unet1.arena.load(extracted)
    pred = XR.predict(unet1, rt1, cfg, x, 500, ctx, pooled, tid, h)
    del unet1
    rt = M.Runtime("cuda:0", 2)
    unet = M.UNet(rt, cfg, base, lora_rank=rank)
    unet.arena.load(extracted)
    lat = SM.LatentSampler(rt, unet).sample(tuple(e.cuda() if e is not None else None for e in emb), h, h, steps=8, guidance_scale=8.0,
                                            latents=noise.cuda()).cpu()
    del unet
    torch.cuda.empty_cache()
    e = float((pred - ref).abs().max()) / float(ref.abs().max())
    cos, rel = _cos_rel(lat, lat_o)
    print(f"{version} r={rank}: extracted adapters against the oracle with the original ones: prediction {e:.3g}, render cos {cos} rel {rel}")
    assert torch.isfinite(pred).all() and torch.isfinite(lat).all()
    assert e <= 4e-2, f"prediction error {e}"
    assert cos >= 0.9995 and rel <= 4e-2, (cos, rel)


@pytest.mark.parametrize("version,rank", [("sd15", 16), ("sdxl", 16), ("sdxl", 128)])
def test_real_topology_round_trip(ops, tmp_path, monkeypatch, version, rank):
    """The real topologies through the tools: a 4-step train() job, merge.merge on its checkpoint, extract.extract at the trained rank with
    the job's checkpoint carried over, render.load_for_inference on the written directory; coverage 1 (below 1 once a feed-forward weight moves
    too); the adapters read back from the written file predict and render like the trained ones (_compare)."""
    import gc
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import checkpoint as ckpt
    from sd_lora_trainer_amd import extract as X
    from safetensors.torch import load_file, save_file
    from sd_lora_trainer_amd import merge as MG
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import topology
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_render_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    targets = topology.lora_targets(topology.CONFIGS[version])
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="job", seed=1, resolution=256, train_batch_size=1, max_train_steps=4,
                         checkpointing_steps=1000, lora_rank=rank, n_sample_imgs=0, output_dir=str(tmp_path / "job"), unet_lr=3e-3,
                         pretrained_model={"path": f"synthetic:{version}", "tokenizer_path": tok_dir, "tokenizer_2_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    ckdir = os.path.abspath(ckdir)
    gc.collect()
    torch.cuda.empty_cache()
    rt = M.Runtime("cuda:0", 1)
    models = T.Models(config, rt, build=False)
    # the base model as a bf16 file (and exactly those values for the oracle); merged and extracted in fp32: a mixed bf16 / fp32 pair per layer
    sd = {k: v.detach().to("cpu", BF) for k, v in models.unet_state().items()}
    del models
    base_path = str(tmp_path / "base.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, base_path)
    sd = {k: v.float() for k, v in sd.items()}
    merged_dir, out = str(tmp_path / "merged"), str(tmp_path / "extracted")
    MG.merge(base_path, ckdir, merged_dir, dtype="fp32", runtime=rt)
    files, line = X.extract(base_path, merged_dir, rank, out, checkpoint_dir=ckdir, runtime=rt, weight_type="fp32")
    line = json.loads(json.dumps(line))
    print(f"{version} r={rank}: {line}")
    assert line["rank"] == rank and abs(line["coverage"] - 1.0) <= 1e-9 and line["residual"]["overall"] <= 1e-3, line
    gc.collect()
    torch.cuda.empty_cache()
    ld = R.load_for_inference(out)
    assert ld.stack.unet.arena.rank == rank and len(ld.stack.unet.arena.entries) == len(targets)
    del ld
    gc.collect()
    torch.cuda.empty_cache()
    # a synthetic full fine-tune: the merged model with a feed-forward weight moved as well
    tuned = load_file(os.path.join(merged_dir, "diffusion_pytorch_model.safetensors"))
    ff = next(k for k in sd if ".ff.net." in k and k.endswith(".weight"))
    tuned[ff] = tuned[ff] + 0.01 * torch.randn(tuned[ff].shape, generator=torch.Generator().manual_seed(1))
    cov = X.extract_adapters(sd, tuned, rank, power_iters=0, runtime=rt).coverage
    assert 0.0 < cov < 1.0 - 1e-6, cov
    del tuned
    find = lambda d: next(os.path.join(d, f) for f in os.listdir(d) if f.endswith("_lora.safetensors"))  # noqa: E731
    _compare(version, sd, ckpt.load_lora(find(ckdir), targets), ckpt.load_lora(find(out), targets), rank)


def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_cli_round_trip_gpu(tmp_path, monkeypatch, version):
    """4-step train() -> merge CLI -> extract CLI at the trained rank -> render.load_for_inference; prediction and render against the
    trained checkpoint's adapters; then the resize CLI."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safetensors.torch import save_file
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import checkpoint as ckpt
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import topology
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_render_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    res = 256 if version == "tinyxl" else 128
    rank = 16
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="job", seed=1, resolution=res, train_batch_size=1, max_train_steps=4,
                         checkpointing_steps=1000, lora_rank=rank, n_sample_imgs=0, output_dir=str(tmp_path / "job"), unet_lr=3e-3,
                         pretrained_model={"path": f"synthetic:{version}", "tokenizer_path": tok_dir, "tokenizer_2_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    ckdir = os.path.abspath(ckdir)
    models = T.Models(config, M.Runtime(config.device, 1))
    base = {k: v.detach().float().cpu().contiguous() for k, v in models.unet_state().items()}
    del models
    base_path = str(tmp_path / "base.safetensors")
    save_file(base, base_path)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def cli(mod, *args):
        r = subprocess.run([sys.executable, "-m", f"sd_lora_trainer_amd.{mod}", *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    cli("merge", "--unet", base_path, "--checkpoint", ckdir, "--out", str(tmp_path / "merged"), "--dtype", "fp32")
    out = str(tmp_path / "extracted")
    line = json.loads(cli("extract", "--base", base_path, "--tuned", str(tmp_path / "merged"), "--rank", str(rank), "--out", out, "--checkpoint", ckdir,
                          "--dtype", "fp32").strip().splitlines()[-1])
    print(line)
    assert line["rank"] == rank and abs(line["coverage"] - 1.0) <= 1e-9 and line["residual"]["overall"] <= 1e-3, line
    ld = R.load_for_inference(out)
    assert ld.stack.unet.arena.rank == rank
    del ld
    targets = topology.lora_targets(topology.CONFIGS[version])
    find = lambda d: next(os.path.join(d, f) for f in os.listdir(d) if f.endswith("_lora.safetensors"))  # noqa: E731
    _compare(version, base, ckpt.load_lora(find(ckdir), targets), ckpt.load_lora(find(out), targets), rank)
    out2 = str(tmp_path / "resized")
    line = json.loads(cli("extract", "--resize", ckdir, "--rank", "4", "--out", out2).strip().splitlines()[-1])
    assert line["rank"] == 4 and 0.0 <= line["residual"]["overall"] < 1.0, line
    assert R.load_for_inference(out2).stack.unet.arena.rank == 4
