"""Adapter merge on the MI355X: sdlt_lora_merge (ops.MergePlan) against an fp64 CPU merge under the fp32 summation bound of
tests/test_merge_cpu.py, one launch per arena (two with DoRA), no effect on training state or on a captured step, the merged UNet's
prediction / render against the fp32 oracle WITH adapters, and the CLI round trip through training jobs."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U
from tests.test_merge_cpu import SHAPES, bound, case

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def _check(out, W, A, B, s, mag, out_dtype, what):
    ref, b = bound(W, A, B, s, mag, out_dtype)
    err = (out.double().cpu() - ref).abs()
    n, worst = int((err > b).sum()), float((err / b).max())
    print(f"{what}: worst err/bound {worst:.3g}")
    assert n == 0, f"{what}: {n} elements outside the bound (worst err/bound {worst:.3g})"


@pytest.mark.parametrize("r,dora", [(4, False), (16, False), (64, False), (128, False), (256, False), (16, True), (64, True)])
@pytest.mark.parametrize("out_dtype", [BF, F16, F32])
def test_kernel_meets_fp32_bound(ops, r, dora, out_dtype):
    """Linear, conv (K = 9 Cin) and stacked q|k|v row slices in ONE plan, base weights in bf16 / fp16 / fp32."""
    s = 0.75
    host, layers = [], []
    wdt = [BF, F16, F32]
    for i, (N, K) in enumerate(SHAPES):
        W, A, B, mag = case(N, K, r, seed=1000 * r + i, w_dtype=wdt[i % 3], dora=dora)
        out = torch.full((N, K), float("nan"), dtype=out_dtype, device="cuda")
        host.append((W, A, B, mag, out, f"{N}x{K}"))
        layers.append(dict(W=W.cuda(), A=A.cuda(), B=B.cuda(), out=out, s=s, mag=mag.cuda() if mag is not None else None))
    # stacked to_q|to_k|to_v: the members' weights and outputs are row slices of one [3 N, K] tensor
    N, K = 320, 320
    Wst = torch.cat([case(N, K, r, seed=7 + g, w_dtype=BF)[0] for g in range(3)], 0)
    Wd, Od = Wst.cuda(), torch.full((3 * N, K), float("nan"), dtype=out_dtype, device="cuda")
    for g in range(3):
        _, A, B, mag = case(N, K, r, seed=70 + g, dora=dora)
        W = Wst[g * N:(g + 1) * N]
        host.append((W, A, B, mag, Od[g * N:(g + 1) * N], f"stacked member {g}"))
        layers.append(dict(W=Wd[g * N:(g + 1) * N], A=A.cuda(), B=B.cuda(), out=Od[g * N:(g + 1) * N], s=s, mag=mag.cuda() if mag is not None else None))
    plan = ops.MergePlan(layers, out_dtype, torch.device("cuda"))
    plan.run()
    torch.cuda.synchronize()
    for W, A, B, mag, out, what in host:
        _check(out, W, A, B, s, mag, out_dtype, f"r={r} dora={dora} {out_dtype} {what} W {W.dtype}")


def _count_calls(monkeypatch, lib):
    calls = []
    real = lib.sdlt_lora_merge

    def wrapped(*a):
        calls.append(a[5])
        return real(*a)
    monkeypatch.setattr(lib, "sdlt_lora_merge", wrapped)
    return calls


@pytest.mark.parametrize("dora,expect", [(False, 1), (True, 2)])
def test_sdxl_arena_merges_in_one_launch(ops, monkeypatch, dora, expect):
    from sd_lora_trainer_amd import merge as MG
    from sd_lora_trainer_amd import topology
    import sd_lora_trainer_amd.unet as M
    cfg = topology.CONFIGS["sdxl"]
    shapes = topology.param_shapes(cfg)
    targets = topology.lora_targets(cfg)
    assert len(targets) == 577
    g = torch.Generator(device="cuda").manual_seed(0)
    base = {n + ".weight": (torch.randn(shapes[n + ".weight"], generator=g, device="cuda") * 0.02).to(BF) for n in targets}
    rt = M.Runtime("cuda:0", 1)
    arena = MG.build_arena(rt, [(n, base[n + ".weight"]) for n in targets], 16, 1.0, dora)
    arena.params.normal_(0.0, 0.05, generator=g)
    calls = _count_calls(monkeypatch, ops._lib.load())
    m = arena.merged(base, dtype=BF)
    torch.cuda.synchronize()
    assert len(calls) == expect, f"sdlt_lora_merge calls for {len(targets)} layers: {calls}"
    assert len(m) == 577 and all(torch.isfinite(v).all() for v in list(m.values())[:8])


def test_merge_leaves_training_state_and_captured_step_alone(ops):
    import sd_lora_trainer_amd.step as S
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import topology
    from tests.test_step_gpu import _inputs
    version, B, h, rank = "tinyxl", 1, 16, 16
    cfg = U.CONFIGS[version]
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    latent, noise, mask, t, ctx, pooled, tid, add = _inputs(cfg, B, h)
    rt = M.Runtime("cuda:0", B)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    ts = S.TrainStep(rt, unet, latent_hw=(h, h), snr_gamma=5.0)
    dv = lambda x: x.cuda() if x is not None else None  # noqa: E731
    ts.set_batch(dv(latent), dv(noise), dv(t), dv(mask), dv(ctx), dv(pooled), dv(tid))
    ts.capture(warmup=1)
    ts.run(0.0)                       # lr 0: the parameters stay, so every replay computes the same gradients
    torch.cuda.synchronize()
    g0 = unet.arena.grads.clone()
    a = unet.arena
    st = [a.params, a.m, a.v] + [e[k] for e in a.entries for k in ("A_s", "B_s", "Bt_s", "At_s", "Ab_s") if k in e]
    before = [x.clone() for x in st]
    m = a.merged(sd, scale=0.75)
    torch.cuda.synchronize()
    assert len(m) == len(a.entries)
    for x, y in zip(before, st):
        assert torch.equal(x, y), "merged() changed training state"
    assert a.scale == a.alpha_scale
    ts.run(0.0)
    torch.cuda.synchronize()
    assert torch.equal(unet.arena.grads, g0), "a replay after the merge computed different gradients"


def _predict(unet, rt, cfg, x, t, ctx, pooled, tid, h):
    import sd_lora_trainer_amd.unet as M
    dev = rt.device
    x64 = rt.zeros(h * h, 64)
    x64[:, :4] = x.permute(0, 2, 3, 1).reshape(h * h, 4).to(dev, x64.dtype)
    cb = rt.zeros(M.CTX_PAD, cfg["cross_dim"])
    cb[:77] = ctx[0].to(dev, cb.dtype)
    pb = pooled.to(dev, rt.act) if pooled is not None else None
    tb = tid.reshape(-1).to(dev, F32) if tid is not None else None
    with torch.no_grad():
        eps = unet.forward(x64, torch.tensor([float(t)], device=dev), cb, pb, tb, B=1, H=h, W=h)
    torch.cuda.synchronize()
    return eps.float().view(1, h, h, 4).permute(0, 3, 1, 2).cpu()


def _sd_and_lora(version, rank, dora, s):
    from tests.test_real_topology_gpu import _unet_state
    cfg = U.CONFIGS[version]
    sd = U.init_unet_state(cfg, seed=0) if version.startswith("tiny") else _unet_state(version)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    if dora:
        lora = U.init_dora_magnitudes(cfg, sd, lora, lora_scale=s, jitter=0.1, seed=2)
    return cfg, sd, lora


@pytest.mark.parametrize("rank,dora", [(16, False), (128, False), (16, True)])
@pytest.mark.parametrize("lora_scale", [1.0, 0.75])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl", "sd15", "sdxl"])
def test_merged_unet_matches_oracle_with_adapters(ops, version, lora_scale, rank, dora):
    """UNet(merged_sd) without adapters and the adapter path on the same inputs, both against oracle.unet_forward(..., lora, lora_scale) in fp32
    (32 x 32 latent), with the prediction bar of tests/test_wide_rank_gpu.py::_step."""
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import topology
    h = 32
    cfg, sd, lora = _sd_and_lora(version, rank, dora, lora_scale)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, h, h, generator=g)
    t = 500
    ctx = torch.randn(1, 77, cfg["cross_dim"], generator=g)
    pooled = tid = add = None
    if cfg["addition"]:
        pooled = torch.randn(1, cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"], generator=g)
        tid = torch.tensor([[8. * h, 8. * h, 0, 0, 8. * h, 8. * h]])
        add = {"text_embeds": pooled, "time_ids": tid}
    with torch.no_grad():
        ref = U.unet_forward(cfg, sd, x, torch.tensor([t]), ctx, add, lora=lora, lora_scale=lora_scale)
    rt = M.Runtime("cuda:0", 1)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank, use_dora=dora)
    unet.arena.load(lora)
    merged = unet.arena.merged(sd, scale=lora_scale, dtype=BF)
    msd = dict(sd)
    msd.update({k: v.float().cpu() for k, v in merged.items()})
    del merged
    unet.arena.set_scale(unet.arena.alpha_scale * lora_scale)          # the adapter path at the render scale (its own instance)
    p_ad = _predict(unet, rt, cfg, x, t, ctx, pooled, tid, h)
    del unet
    rt2 = M.Runtime("cuda:0", 1)
    plain = M.UNet(rt2, topology.CONFIGS[version], msd)
    p_m = _predict(plain, rt2, cfg, x, t, ctx, pooled, tid, h)
    del plain
    scale = float(ref.abs().max())
    e_m, e_ad = float((p_m - ref).abs().max()) / scale, float((p_ad - ref).abs().max()) / scale
    print(f"{version} s={lora_scale} r={rank} dora={dora}: merged {e_m:.3g}, adapters {e_ad:.3g}")
    assert torch.isfinite(p_m).all() and torch.isfinite(p_ad).all()
    assert e_m <= 4e-2, f"merged UNet prediction error {e_m}"
    assert e_ad <= 4e-2, f"adapter path prediction error {e_ad}"
    torch.cuda.empty_cache()


def test_merged_render_matches_oracle_sampler():
    """tinyxl, 8 trailing Euler steps at CFG 8: the merged UNet without adapters against the oracle sampler WITH adapters (lora_scale 0.75),
    tests/test_e2e_image_gpu.py's latent bars."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import sampler_ref as SR
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import sampler as SM
    from sd_lora_trainer_amd import topology
    from tests.test_step_gpu import _cos_rel
    version, h, rank, s = "tinyxl", 32, 16, 0.75
    cfg, sd, lora = _sd_and_lora(version, rank, False, s)
    g = torch.Generator().manual_seed(9)
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"]
    emb = (torch.randn(1, 77, cfg["cross_dim"], generator=g), torch.randn(1, 77, cfg["cross_dim"], generator=g),
           torch.randn(1, P, generator=g), torch.randn(1, P, generator=g))
    noise = torch.randn(1, 4, h, h, generator=g)
    lat_o = SR.sample_latents(cfg, sd, lora, s, emb, noise, 8, guidance_scale=8.0)
    rt = M.Runtime("cuda:0", 2)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    msd = dict(sd)
    msd.update({k: v.float().cpu() for k, v in unet.arena.merged(sd, scale=s).items()})
    rt2 = M.Runtime("cuda:0", 2)
    smp = SM.LatentSampler(rt2, M.UNet(rt2, topology.CONFIGS[version], msd))
    lat = smp.sample(tuple(e.cuda() for e in emb), h, h, steps=8, guidance_scale=8.0, latents=noise.cuda()).cpu()
    assert torch.isfinite(lat).all()
    cos, rel = _cos_rel(lat, lat_o)
    print(f"merged render vs oracle sampler with adapters: cos {cos} rel {rel}")
    assert cos >= 0.9995 and rel <= 4e-2, (cos, rel)


def _run(gen):
    progress = []
    try:
        while True:
            progress.append(next(gen))
    except StopIteration as e:
        return progress, e.value


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_cli_round_trip_gpu(tmp_path, monkeypatch, version):
    """4-step train() job (use_dora, text-encoder adapters) -> base weights written from train.Models -> the CLI -> the output as
    pretrained_model of a fresh job that trains a finite step."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import subprocess
    import sys
    from safetensors.torch import save_file
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    monkeypatch.chdir(tmp_path)
    res = 256 if version == "tinyxl" else 128          # (tinyxl: 64 tokens at the coarsest hooked level, the smallest the token-attention GEMMs take)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model={"path": f"synthetic:{version}"}, seed=1,
                         resolution=res, train_batch_size=1, max_train_steps=4, use_dora=True, text_encoder_lora_optimizer="adamw",
                         checkpointing_steps=1000, n_sample_imgs=0)
    _, (config, out_dir) = _run(T.train(cfg))
    out_dir = os.path.abspath(out_dir)
    models = T.Models(config, M.Runtime(config.device, 1))
    paths = {"unet": str(tmp_path / "base_unet.safetensors")}
    save_file({k: v.detach().cpu().contiguous() for k, v in models.unet_state().items()}, paths["unet"])
    for i in range(len(models.kinds)):
        paths[f"te{i}"] = str(tmp_path / f"base_te{i}.safetensors")
        save_file({k: v.detach().cpu().contiguous() for k, v in models.clip_state(i).items()}, paths[f"te{i}"])
    del models
    xl = version == "tinyxl"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "sd_lora_trainer_amd.merge", "--unet", paths["unet"], "--checkpoint", out_dir, "--out", str(tmp_path / "merged"),
           "--dtype", "bf16", "--text-encoder", paths["te0"]] + (["--text-encoder-2", paths["te1"]] if xl else [])
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    mdir = tmp_path / "merged"
    from safetensors.torch import load_file
    out, base = load_file(str(mdir / "diffusion_pytorch_model.safetensors")), load_file(paths["unet"])
    assert set(out) == set(base) and all(out[k].dtype == BF and out[k].shape == base[k].shape for k in out)
    pm = {"path": str(mdir / "diffusion_pytorch_model.safetensors"), "text_encoder_path": str(mdir / "text_encoder" / "model.safetensors")}
    if xl:
        pm["text_encoder_2_path"] = str(mdir / "text_encoder_2" / "model.safetensors")
    cfg2 = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model=pm, seed=2, resolution=res, train_batch_size=1,
                          max_train_steps=1, checkpointing_steps=1000, n_sample_imgs=0, output_dir=str(tmp_path / "job2"))
    cfg2.sd_model_version = version
    progress, (_, out2) = _run(T.train(cfg2))
    assert progress[-1] == 1.0
    ta = json.load(open(os.path.join(out2, "training_args.json")))
    assert all(np.isfinite(ta["training_attributes"]["losses"]["tot_loss"]))
