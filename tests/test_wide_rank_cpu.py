"""LoRA ranks 65..256 (the wide adapter path, DESIGN "Wide LoRA ranks") on CPU through the fp32 op emulation: rank padding and shadows of the
arena, the refusals, one step + trajectory against the fp32 oracle, the job driver with wide UNet and text-encoder adapters, and the same
rank-16 adapters through the fused and the forced wide path."""
import json
import os
import types

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import unet_ref as U
from sd_lora_trainer_amd import topology
from tests import emu_ops


def _gemm_grouped_x2(X, W, out, *, X2=None, W2=None, x2_group_n=0, **kw):
    """Restatement of the grouped second segment (sdlt_gemm_params.x2_group_n), which tests/emu_ops.gemm does not know: output column
    group g reads X2 columns [g K2, (g+1) K2) - i.e. a plain second segment against the block-diagonal expansion of W2."""
    if x2_group_n:
        N, K2 = W2.shape
        G = N // x2_group_n
        assert X2.shape[1] == G * K2
        W2d = torch.zeros(N, G * K2, dtype=W2.dtype, device=W2.device)
        for g in range(G):
            W2d[g * x2_group_n:(g + 1) * x2_group_n, g * K2:(g + 1) * K2] = W2[g * x2_group_n:(g + 1) * x2_group_n]
        W2 = W2d
    return emu_ops.gemm(X, W, out, X2=X2, W2=W2, **kw)


# the emulation plus the one op option it lacks
emu_wide = types.ModuleType("emu_wide")
emu_wide.__dict__.update({k: v for k, v in vars(emu_ops).items() if not k.startswith("__")})
emu_wide.gemm = _gemm_grouped_x2


@pytest.mark.parametrize("rank,rp", [(65, 128), (96, 128), (128, 128), (200, 256), (256, 256)])
def test_arena_rank_padding_and_shadows(rank, rp):
    cfg = topology.CONFIGS["tiny15"]
    sd = U.init_unet_state(U.CONFIGS["tiny15"], seed=0)
    rt = unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_wide)
    unet = unet_mod.UNet(rt, cfg, sd, lora_rank=rank)
    ar = unet.arena
    assert ar.Rp == rp and ar.wide and ar.Wu == rp
    lora = U.init_lora(U.CONFIGS["tiny15"], rank, seed=1, b_std=0.05)
    ar.load(lora)
    n_conv = 0
    for e in ar.entries:
        N, K = e["N"], e["K"]
        A, B = e["A"], e["B"]
        assert tuple(A.shape) == (rank, K) and tuple(B.shape) == (N, rank)
        assert tuple(e["A_s"].shape) == (rp, K) and tuple(e["B_s"].shape) == (N, rp) and tuple(e["Bt_s"].shape) == (rp, N)
        assert torch.equal(e["A_s"][:rank], A.to(e["A_s"].dtype)) and not e["A_s"][rank:].any()
        assert torch.equal(e["B_s"][:, :rank], B.to(e["B_s"].dtype)) and not e["B_s"][:, rank:].any()
        assert torch.equal(e["Bt_s"][:rank], B.t().to(e["Bt_s"].dtype)) and not e["Bt_s"][rank:].any()
        if e["conv_cin"] is None:
            assert tuple(e["At_s"].shape) == (K, rp)
            assert torch.equal(e["At_s"][:, :rank], A.t().to(e["At_s"].dtype)) and not e["At_s"][:, rank:].any()
        else:
            n_conv += 1
            cin = e["conv_cin"]
            Ab = e["Ab_s"].view(cin, 9, rp)
            assert tuple(e["Ab_s"].shape) == (cin, 9 * rp)
            assert torch.equal(Ab[:, :, :rank], A.view(rank, 9, cin).permute(2, 1, 0).to(Ab.dtype)) and not Ab[:, :, rank:].any()
    assert n_conv > 0
    # the real rank leaves the engine (peft / kohya layouts)
    out = ar.export()
    name = next(e["name"] for e in ar.entries if e["conv_cin"] is not None)
    assert out[name][0].shape[0] == rank and out[name][1].shape[1] == rank


def test_rank_limits():
    rt = unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_wide)
    with pytest.raises(ValueError):
        unet_mod.LoraArena(rt, 257)
    with pytest.raises(NotImplementedError):
        unet_mod.LoraArena(rt, 128, dora=True)
    assert not unet_mod.LoraArena(rt, 64).wide and unet_mod.LoraArena(rt, 64).Rp == 64
    assert not unet_mod.LoraArena(rt, 64, dora=True).wide


@pytest.mark.parametrize("rank", [128, 96])
@pytest.mark.parametrize("version,B,kinds", [("tiny15", 2, ["tiny_l"]), ("tinyxl", 1, ["tiny_l", "tiny_g"])])
def test_wide_step_against_oracle_cpu(version, B, kinds, rank):
    pytest.importorskip("transformers")
    from tests.test_real_topology_gpu import TOL_FP32, TOL_FP32_FAITHFUL, _bf16_exact, run_step_and_trajectory
    sd = _bf16_exact(U.init_unet_state(U.CONFIGS[version], seed=0))
    traj = run_step_and_trajectory(version, B, 32 if U.CONFIGS[version]["addition"] else 16, sd, kinds, device="cpu", ops=emu_wide,
                                   act_dtype=torch.float32, tol=TOL_FP32, tol_faithful=TOL_FP32_FAITHFUL, rank=rank, n_steps=3)
    assert len(traj) == 3


def test_train_driver_wide_ranks(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from safetensors.torch import load_file
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model={"path": "synthetic:tiny15"}, seed=1, resolution=128,
                         train_batch_size=1, max_train_steps=3, lora_rank=128, text_encoder_lora_optimizer="adamw", text_encoder_lora_rank=96,
                         checkpointing_steps=1000)
    gen = T.train(cfg, runtime=unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_wide))
    progress = []
    try:
        while True:
            progress.append(next(gen))
    except StopIteration as e:
        config, out_dir = e.value
    assert progress[-1] == 1.0
    ta = json.load(open(os.path.join(out_dir, "training_args.json")))
    assert all(np.isfinite(ta["training_attributes"]["losses"]["tot_loss"]))
    sd = load_file(next(os.path.join(out_dir, f) for f in os.listdir(out_dir) if f.endswith("_lora.safetensors")))
    unet_keys = [k[: -len(".lora_down.weight")] for k in sd if k.startswith("lora_unet") and k.endswith(".lora_down.weight")]
    te_keys = [k[: -len(".lora_down.weight")] for k in sd if k.startswith("lora_te") and k.endswith(".lora_down.weight")]
    assert unet_keys and te_keys
    for k, r in [(k, 128) for k in unet_keys] + [(k, 96) for k in te_keys]:
        down, up = sd[k + ".lora_down.weight"], sd[k + ".lora_up.weight"]
        assert down.shape[0] == r and up.shape[1] == r, (k, down.shape, up.shape)
        assert int(sd[k + ".alpha"]) == r


def _one_pass(version, rank, wide_min, monkeypatch):
    """loss and adapter gradients of one forward / backward at fp32 through the emulation, with SDLT_LORA_WIDE_MIN = wide_min"""
    import sd_lora_trainer_amd.step as S
    from oracle import loss_ref as L
    monkeypatch.setattr(unet_mod, "LORA_WIDE_MIN", wide_min)
    cfg = U.CONFIGS[version]
    B, h = 2, 16
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    g = torch.Generator().manual_seed(3)
    latent = torch.randn(B, 4, h, h, generator=g) * cfg["scaling_factor"]
    noise = torch.randn(B, 4, h, h, generator=g)
    mask = torch.ones(B, 4, h, h)
    t = torch.tensor([500, 20])
    ctx = torch.randn(B, 77, cfg["cross_dim"], generator=g)
    rt = unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=emu_wide)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    ts = S.TrainStep(rt, unet, latent_hw=(h, h))
    ts.set_batch(latent, noise, t, mask, ctx)
    ts.forward_backward()
    assert unet.arena.wide == (wide_min <= 16)
    return float(ts.loss), unet.arena.export("grads")


def test_forced_wide_matches_fused_path(monkeypatch):
    """Same rank-16 adapters through the fused in-tile kernels' contract and through the wide decomposition (SDLT_LORA_WIDE_MIN=16)."""
    loss0, g0 = _one_pass("tiny15", 16, 128, monkeypatch)
    loss1, g1 = _one_pass("tiny15", 16, 16, monkeypatch)
    assert abs(loss0 - loss1) <= 1e-5 * abs(loss0)
    for k in g0:
        for a, b in zip(g0[k], g1[k]):
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-6 * float(a.abs().max()) + 1e-12), k
