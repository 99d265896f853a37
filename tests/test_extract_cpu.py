"""Adapter extraction and resizing (sd_lora_trainer_amd.extract) on CPU: sdlt_delta_matmul replaced by the torch emulation of
tests/extract_ref.py (injected through the runtime's op table), judged against the fp64 restatement there.  The kernel itself and the real
topologies are checked on the GPU by tests/test_extract_gpu.py with the same yardsticks."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file, save_file

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import checkpoint as ckpt
from sd_lora_trainer_amd import extract as X
from sd_lora_trainer_amd import merge as MG
from sd_lora_trainer_amd import topology
from tests import extract_ref as XR

F32 = torch.float32


def _rt(ops=None, B=1):
    return unet_mod.Runtime("cpu", B, act_dtype=F32, ops=ops or XR.emu_ops_with_delta())


def merged_case(rt, rank, seed, dtype=F32):
    """base, seeded adapters of `rank`, tuned = arena.merged(base, dtype)."""
    base = XR.case_base(seed)
    lora = XR.case_lora(rank, seed + 1)
    arena = MG.build_arena(rt, [(n, base[n + ".weight"]) for n in lora], rank, 1.0, False)
    arena.load(lora)
    tuned = {k: v.detach().cpu().contiguous() for k, v in arena.merged(base, dtype=dtype).items()}
    return base, tuned, lora


def shapes2d(base, names):
    return [tuple(XR.view2d(base[n + ".weight"]).shape) for n in names]


@pytest.mark.parametrize("rank", [4, 16, 64, 128])
def test_exact_recovery(rank):
    rt = _rt()
    base, tuned, lora = merged_case(rt, rank, seed=10 * rank)
    names = list(lora)
    XR.EmuDeltaPlan.launches.clear()
    ex = X.extract_adapters(base, tuned, rank, seed=5, runtime=rt, targets=names)
    assert XR.EmuDeltaPlan.launches == ["forward", "transposed", "forward", "transposed", "forward", "transposed"], "2 q + 2 products for the whole model"
    L = X.padded_columns(rank, 16)
    om = XR.omegas_by_name(names, shapes2d(base, names), L, 5)
    XR.check_recovery(ex, base, tuned, lora, rank, L, om, 2, f"cpu r={rank}")
    assert abs(ex.coverage - 1.0) <= 1e-12
    for n in names:
        assert ex.lora[n][0].shape == lora[n][0].shape and ex.lora[n][1].shape == lora[n][1].shape
        assert ex.layers[n]["kept"] == rank and ex.layers[n]["residual"] <= 1e-3


DECAY, RANK_T, Q_T = 0.8, 16, 2


def _spectrum_case():
    base = XR.case_base(3)
    tuned, sig = {}, {}
    for i, (k, w) in enumerate(base.items()):
        w2 = XR.view2d(w)
        D, s = XR.spectrum_delta(w2.shape[0], w2.shape[1], DECAY, seed=40 + i)
        t2 = (w2.double() + D).float()
        tuned[k] = t2.view(w.shape[0], 3, 3, w.shape[1]).permute(0, 3, 1, 2).contiguous() if w.dim() == 4 else t2
        sig[k[: -len(".weight")]] = s
    return base, tuned, sig


def test_truncation_quality():
    """(a) the restatement's spectral residual within the Halko-Martinsson-Tropp power-scheme bound for r = 16, p = 16, q = 2 on a 0.8^i
    spectrum; (b) the emulated fp32 pipeline's Frobenius residual within the restatement's plus the fp32 bound, against the optimal one."""
    rt = _rt()
    base, tuned, sig = _spectrum_case()
    names = list(sig)
    L = X.padded_columns(RANK_T, 16)
    om = XR.omegas_by_name(names, shapes2d(base, names), L, 0)
    ex = X.extract_adapters(base, tuned, RANK_T, power_iters=Q_T, seed=0, runtime=rt, targets=names)
    for n in names:
        D = XR.delta64(XR.view2d(base[n + ".weight"]), XR.view2d(tuned[n + ".weight"]))
        A, B, _ = XR.extract_ref(D, om[n], RANK_T, Q_T)
        spec = float(torch.linalg.matrix_norm(D - B @ A, ord=2))
        hmt = XR.hmt_bound(sig[n], RANK_T, L - RANK_T, Q_T)
        res_ref = float((D - B @ A).norm())
        opt = float((sig[n][RANK_T:] ** 2).sum().sqrt())
        A2, B2 = ex.lora[n]
        res = float((D - XR.product2d(A2, B2)).norm())
        allow = res_ref + XR.fp32_bound(D, L, XR.view2d(A2), XR.view2d(B2))
        print(f"{n}: spectral {spec:.4e} (sigma_r+1 {float(sig[n][RANK_T]):.4e}, HMT {hmt:.4e}); Frobenius: fp32 {res:.6e}, restatement {res_ref:.6e}, optimal {opt:.6e}")
        assert spec <= hmt
        assert res <= allow
        assert res_ref >= opt * (1 - 1e-6)          # Eckart-Young: nothing beats the optimum (up to the fp32 rounding of the tuned weights)
        assert abs(ex.layers[n]["residual"] * ex.layers[n]["delta_norm"] - res) <= 1e-3 * res


def test_energy_keeps_the_smallest_count():
    rt = _rt()
    base, tuned, sig = _spectrum_case()
    names = list(sig)
    f = 0.9
    ex = X.extract_adapters(base, tuned, RANK_T, energy=f, seed=0, runtime=rt, targets=names)
    for n in names:
        s2 = sig[n] ** 2
        expect = int((torch.cumsum(s2, 0) < f * s2.sum()).sum()) + 1
        assert 1 < expect < RANK_T
        assert ex.layers[n]["kept"] == expect, (n, ex.layers[n]["kept"], expect)
        A, B = ex.lora[n]
        assert not XR.view2d(A)[expect:].any() and not XR.view2d(B)[:, expect:].any()
        assert XR.view2d(A)[expect - 1].any() and XR.view2d(B)[:, expect - 1].any()
        assert not ex.layers[n]["sigma"][expect:].any()


def test_energy_zeros_reach_the_file(tmp_path):
    rt = _rt()
    base, tuned, sig = _spectrum_case()
    names = list(sig)
    ex = X.extract_adapters(base, tuned, RANK_T, energy=0.9, seed=0, runtime=rt, targets=names)
    files = X.write_checkpoint(str(tmp_path / "e"), rt, ex.lora, RANK_T, "tiny15")
    sd = load_file(files["lora"])
    for n in names:
        k = ckpt.kohya_key(n)
        c = ex.layers[n]["kept"]
        assert sd[k + ".lora_down.weight"].shape[0] == RANK_T and int(sd[k + ".alpha"]) == RANK_T
        assert not sd[k + ".lora_down.weight"][c:].any() and not sd[k + ".lora_up.weight"][:, c:].any()
        assert sd[k + ".lora_down.weight"][:c].any()


def _kohya(lora, dtype=F32):
    return ckpt.lora_to_kohya(lora, dtype=dtype)


def test_resize():
    lora = XR.case_lora(128, 7)
    s = 0.5
    sd = _kohya(lora)
    rz = X.resize_adapters(sd, 16, scale=s)
    same = X.resize_adapters(sd, 128, scale=s)
    for n, (A, B) in lora.items():
        k = ckpt.kohya_key(n)
        D = s * (B.flatten(1).double() @ A.flatten(1).double())
        U, S, Vt = torch.linalg.svd(D, full_matrices=False)
        best = (U[:, :16] * S[:16]) @ Vt[:16]
        A2, B2 = rz.lora[k]
        assert A2.shape == (16,) + tuple(A.shape[1:]) and B2.shape == (B.shape[0], 16) + tuple(B.shape[2:])
        P = B2.flatten(1).double() @ A2.flatten(1).double()
        # fp64 route (condition: the gap sigma_16 - sigma_17 is of the order of sigma_16) + the factors' fp32 rounding
        tol = 2 * XR.U32 * float((B2.flatten(1).double().abs() @ A2.flatten(1).double().abs()).norm()) + 1e-12 * float(D.norm())
        assert float((P - best).norm()) <= tol, (n, float((P - best).norm()), tol)
        assert torch.allclose(rz.layers[k]["sigma"], S[:16], rtol=1e-10, atol=0)
        A3, B3 = same.lora[k]
        P3 = B3.flatten(1).double() @ A3.flatten(1).double()
        tol3 = 2 * XR.U32 * float((B3.flatten(1).double().abs() @ A3.flatten(1).double().abs()).norm()) + 1e-12 * float(D.norm())
        assert float((P3 - D).norm()) <= tol3, n
    with pytest.raises(ValueError):
        X.resize_adapters(dict(sd, **{ckpt.kohya_key("a.to_q") + ".dora_scale": torch.ones(320)}), 16)


def test_rank_limits():
    assert X.padded_columns(4, 16) == 32 and X.padded_columns(64, 16) == 80 and X.padded_columns(256, 16) == 272
    with pytest.raises(ValueError):
        X.padded_columns(257, 16)


def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_round_trip_through_the_tools(tmp_path, monkeypatch, capsys, version):
    """train -> merge -> extract at the trained rank: the loader takes the result, its UNet prediction and an 8-step render match the
    original checkpoint's (the bars of tests/test_merge_gpu.py), coverage 1; below 1 when a feed-forward weight moved too; both CLI modes."""
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import sampler as SM
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_render_cpu import _tokenizer_dir, emu_render
    from tests.test_step_gpu import _cos_rel
    monkeypatch.chdir(tmp_path)
    ops = XR.emu_ops_with_delta(emu_render)
    mk = lambda B=1: unet_mod.Runtime("cpu", B, act_dtype=F32, ops=ops)  # noqa: E731
    tok_dir, _ = _tokenizer_dir(tmp_path)
    rank = 4
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="job", seed=1, resolution=128, train_batch_size=1, max_train_steps=3,
                         checkpointing_steps=1000, lora_rank=rank, n_sample_imgs=0, output_dir=str(tmp_path / "job"), unet_lr=3e-3,
                         pretrained_model={"path": f"synthetic:{version}", "tokenizer_path": tok_dir, "tokenizer_2_path": tok_dir})
    config, ckdir = _run(T.train(cfg, runtime=mk()))
    models = T.Models(config, mk())
    base = {k: v.detach().float().contiguous() for k, v in models.unet_state().items()}
    base_path = str(tmp_path / "base.safetensors")
    save_file(base, base_path)
    files = MG.merge(base_path, ckdir, str(tmp_path / "merged"), dtype="fp32", runtime=mk())
    out = str(tmp_path / "extracted")
    X.main(["--base", base_path, "--tuned", str(tmp_path / "merged"), "--rank", str(rank), "--out", out, "--checkpoint", ckdir, "--dtype", "fp32"], runtime=mk())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["rank"] == rank and abs(line["coverage"] - 1.0) <= 1e-9 and line["residual"]["overall"] <= 1e-3, line
    ld = R.load_for_inference(out, runtime=mk())
    assert ld.stack.unet.arena.rank == rank
    assert os.path.exists(os.path.join(out, "special_params.json")) and any(f.endswith("_embeddings.safetensors") for f in os.listdir(out))
    # the two adapter files on the same base: prediction and render
    tcfg = topology.CONFIGS[version]
    targets = topology.lora_targets(tcfg)
    find = lambda d: next(os.path.join(d, f) for f in os.listdir(d) if f.endswith("_lora.safetensors"))  # noqa: E731
    loras = [ckpt.load_lora(find(d), targets) for d in (ckdir, out)]
    h = 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, h, h, generator=g)
    ctx = torch.randn(1, 77, tcfg["cross_dim"], generator=g)
    pooled = tid = None
    P = 0
    if tcfg["addition"]:
        P = tcfg["proj_class_in"] - 6 * tcfg["addition_time_embed_dim"]
        pooled = torch.randn(1, P, generator=g)
        tid = torch.tensor([[8. * h, 8. * h, 0, 0, 8. * h, 8. * h]])
    emb = (torch.randn(1, 77, tcfg["cross_dim"], generator=g), torch.randn(1, 77, tcfg["cross_dim"], generator=g),
           torch.randn(1, P, generator=g) if P else None, torch.randn(1, P, generator=g) if P else None)
    noise = torch.randn(1, 4, h, h, generator=g)
    preds, lats = [], []
    for lora in loras:
        rt = mk()
        unet = unet_mod.UNet(rt, tcfg, base, lora_rank=rank)
        unet.arena.load(lora)
        preds.append(XR.predict(unet, rt, tcfg, x, 500, ctx, pooled, tid, h))
        rt2 = mk(2)
        unet2 = unet_mod.UNet(rt2, tcfg, base, lora_rank=rank)
        unet2.arena.load(lora)
        lats.append(SM.LatentSampler(rt2, unet2).sample(emb, h, h, steps=8, guidance_scale=8.0, latents=noise.clone()).cpu())
    e = float((preds[1] - preds[0]).abs().max()) / float(preds[0].abs().max())
    cos, rel = _cos_rel(lats[1], lats[0])
    print(f"{version}: prediction {e:.3g}, render cos {cos} rel {rel}")
    assert e <= 4e-2 and cos >= 0.9995 and rel <= 4e-2
    # a synthetic full fine-tune: the merged model with a feed-forward weight moved as well
    tuned = load_file(files["unet"])
    ff = next(k for k in tuned if ".ff.net." in k and k.endswith(".weight"))
    tuned[ff] = tuned[ff] + 0.01 * torch.randn(tuned[ff].shape, generator=g)
    ex = X.extract_adapters(base, tuned, rank, runtime=mk())
    assert 0.0 < ex.coverage < 1.0 - 1e-6, ex.coverage
    # resize mode
    out2 = str(tmp_path / "resized")
    X.main(["--resize", ckdir, "--rank", "2", "--out", out2], runtime=mk())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["rank"] == 2 and 0.0 <= line["residual"]["overall"] < 1.0
    assert R.load_for_inference(out2, runtime=mk()).stack.unet.arena.rank == 2
