"""LoRA ranks 65..256 on the MI355X (the wide adapter path, DESIGN "Wide LoRA ranks"): the new product forms of sdlt_gemm_bf16 (a convolution
followed by a plain second K segment, the grouped second segment) and sdlt_lora_grad_wide against their restatements, then whole steps against
the fp32 oracle, the forced wide path against the fused one, and a job that writes a loadable checkpoint."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U
from tests import emu_ops as E
from tests.test_kernels_gpu import close, dev, rnd
from tests.test_wide_rank_cpu import _gemm_grouped_x2

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


# ResnetBlock conv2 geometries of the tiny and the 64 x 64 latents (Cin = Cout), padded ranks 128 / 256
@pytest.mark.parametrize("B,H,C,Rp", [(1, 16, 128, 128), (2, 16, 64, 256), (1, 64, 320, 128), (2, 32, 640, 128)])
@pytest.mark.parametrize("splitk", [0, 1, 3])
def test_conv_then_second_segment(ops, B, H, C, Rp, splitk):
    g = torch.Generator().manual_seed(B * 1000 + H + C + Rp + splitk)
    M = B * H * H
    X = rnd(M, C, g=g)
    Wm = rnd(C, 9 * C, g=g, scale=1 / math.sqrt(9 * C))
    T = rnd(M, Rp, g=g, scale=0.5)
    Bu = rnd(C, Rp, g=g, scale=1 / math.sqrt(Rp))
    bias = torch.randn(C, generator=g)
    rowb = rnd(B, C, g=g)
    R = rnd(M, C, g=g)
    ref = E.gemm(X, Wm, torch.empty(M, C, dtype=BF), conv=E.ConvGeom(B, H, H, C, H, H), X2=T, W2=Bu, bias=bias, rowbias=rowb,
                 rows_per_batch=H * H, residual=R)
    Xd, Wd, Td, Bd, bd, rbd, Rd = dev(X, Wm, T, Bu, bias, rowb, R)
    out = ops.gemm(Xd, Wd, torch.empty(M, C, dtype=BF, device="cuda"), conv=ops.ConvGeom(B, H, H, C, H, H), X2=Td, W2=Bd, bias=bd,
                   rowbias=rbd, rows_per_batch=H * H, residual=Rd, splitk=splitk)
    close(out, ref, what=f"conv + second segment B={B} H={H} C={C} Rp={Rp} splitk={splitk}")
    # the T launch of the wide forward: a mode-1 product with N = Rp and alpha = s
    A = rnd(Rp, 9 * C, g=g, scale=0.05)
    Tref = E.gemm(X, A, torch.empty(M, Rp, dtype=BF), conv=E.ConvGeom(B, H, H, C, H, H), alpha=0.75)
    Tg = ops.gemm(Xd, A.cuda(), torch.empty(M, Rp, dtype=BF, device="cuda"), conv=ops.ConvGeom(B, H, H, C, H, H), alpha=0.75, splitk=splitk)
    close(Tg, Tref, what="conv T launch")


@pytest.mark.parametrize("M,N,K,G,Rp,ct", [(256, 320, 320, 3, 128, False), (128, 64, 128, 3, 256, False), (160, 640, 768, 2, 192, True), (1024, 1280, 1280, 3, 128, False)])
def test_grouped_second_segment(ops, M, N, K, G, Rp, ct):
    g = torch.Generator().manual_seed(M + N + G + Rp)
    X = rnd(M, K, g=g)
    Wm = rnd(G * N, K, g=g, scale=1 / math.sqrt(K))
    T = rnd(M, G * Rp, g=g, scale=0.5)
    Bu = rnd(G * N, Rp, g=g, scale=1 / math.sqrt(Rp))
    bias = torch.randn(G * N, generator=g)
    Ctr = torch.zeros(G * N, M, dtype=BF) if ct else None
    ref = _gemm_grouped_x2(X, Wm, torch.empty(M, G * N, dtype=BF), X2=T, W2=Bu, x2_group_n=N, bias=bias, Ct=Ctr)
    Xd, Wd, Td, Bd, bd = dev(X, Wm, T, Bu, bias)
    Ctd = torch.zeros(G * N, M, dtype=BF, device="cuda") if ct else None
    out = ops.gemm(Xd, Wd, torch.empty(M, G * N, dtype=BF, device="cuda"), X2=Td, W2=Bd, x2_group_n=N, bias=bd, Ct=Ctd)
    close(out, ref, what=f"grouped second segment {M}x{G}*{N}x{K} Rp={Rp}")
    if ct:
        close(Ctd, Ctr, what="grouped second segment Ct")


@pytest.mark.parametrize("Rp,R", [(128, 100), (192, 100), (256, 100), (256, 256)])
def test_lora_grad_wide(ops, Rp, R):
    g = torch.Generator().manual_seed(Rp + R)
    # (M, Cw, rank_major, conv): plain and im2col problems, MFMA-able ones and one that takes the VALU kernel
    specs = [(520, 320, True, None), (333, 128, False, None), (2 * 8 * 8, 9 * 64, True, (2, 8, 8, 64)), (4 * 4, 9 * 128, False, (1, 4, 4, 128))]
    odd = [(2 * 4 * 4, 9 * 32, True, (2, 4, 4, 32)), (100, 36, False, None)]
    for specs_, expect in ((specs, 1), (odd, 0)):
        for accumulate in (0, 1):
            probs_c, probs_g, bufs = [], [], []
            for (M, Cw, rank_major, conv) in specs_:
                Q = torch.zeros(M, Rp, dtype=BF)
                Q[:, :R] = rnd(M, R, g=g)
                Q[:, R:] = rnd(M, Rp - R, g=g)      # padded columns hold garbage: must not reach any output
                if conv is None:
                    P, cc, cg = rnd(M, Cw, g=g), None, None
                else:
                    B, H, W, Cin = conv
                    P = rnd(B * H * W, Cin, g=g)
                    cc, cg = E.ConvGeom(B, H, W, Cin, H, W), ops.ConvGeom(B, H, W, Cin, H, W)
                init = torch.randn(Cw * R, generator=g)
                probs_c.append(dict(P=P, Q=Q, out=init.clone(), M=M, Cw=Cw, R=R, rank_major=rank_major, conv=cc))
                buf = torch.full((Cw * R + 256,), 7.0, dtype=F32, device="cuda")    # tail sentinel: nothing past the real rank's block is written
                buf[: Cw * R] = init.cuda()
                bufs.append(buf)
                probs_g.append(dict(P=P.cuda(), Q=Q.cuda(), out=buf[: Cw * R], M=M, Cw=Cw, R=R, rank_major=rank_major, conv=cg))
            pc = E.LoraGradPlan(probs_c, Rp, "cpu")
            pc.set_accumulate(accumulate)
            pc.run()
            plan = ops.LoraGradPlan(probs_g, Rp, torch.device("cuda"))
            assert plan.mfma == expect
            plan.set_accumulate(accumulate)
            plan.run()
            torch.cuda.synchronize()
            for a, b_, buf in zip(probs_c, probs_g, bufs):
                close(b_["out"], a["out"], tol=2e-3, what=f"wide lora grad Rp={Rp} R={R} M={a['M']} Cw={a['Cw']} acc={accumulate}")
                assert bool((buf[a["Cw"] * R:] == 7.0).all()), "write past the real rank"


def _step(version, B, rank, graph=True):
    """One step of the HIP path against the fp32 oracle (the bars of tests/test_step_gpu.py::test_step_matches_fp32_oracle)."""
    import sd_lora_trainer_amd.step as S
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import topology
    from tests.test_step_gpu import _cos_rel, _flat, _inputs, _oracle
    cfg, h = U.CONFIGS[version], 16
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    latent, noise, mask, t, ctx, pooled, tid, add = _inputs(cfg, B, h)
    rt = M.Runtime("cuda:0", B)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    ts = S.TrainStep(rt, unet, latent_hw=(h, h), snr_gamma=5.0, l1_penalty=0.03, weight_decay=0.004)
    dv = lambda x: x.cuda() if x is not None else None  # noqa: E731
    ts.set_batch(dv(latent), dv(noise), dv(t), dv(mask), dv(ctx), dv(pooled), dv(tid))
    pred = ts.forward_backward().float().cpu().reshape(B, h, h, 4).permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    assert torch.isfinite(pred).all()
    if not graph:
        return unet, ts
    pred_o, loss_o, grads_o, gctx_o = _oracle(cfg, sd, lora, latent, noise, t, mask, ctx, add, 5.0)
    err = float((pred - pred_o).abs().max()) / float(pred_o.abs().max())
    assert err <= 4e-2, f"prediction error {err}"
    assert abs(float(ts.loss) - loss_o) <= 2e-2 * abs(loss_o), (float(ts.loss), loss_o)
    cos, rel = _cos_rel(_flat(unet.arena.export("grads")), _flat(grads_o))
    assert cos >= 0.99 and rel <= 8e-2, f"LoRA grads cos {cos} rel {rel}"
    gctx = ts.dctx.float().cpu().view(B, M.CTX_PAD, -1)
    cos, rel = _cos_rel(gctx[:, :77], gctx_o)
    assert cos >= 0.99 and rel <= 8e-2, f"dctx cos {cos} rel {rel}"
    g_eager = unet.arena.grads.clone()
    ts.capture(warmup=1)
    unet.arena.grads.zero_()
    ts.run(1e-3)
    torch.cuda.synchronize()
    cos, rel = _cos_rel(unet.arena.grads, g_eager)
    assert cos >= 0.999999 and rel <= 1e-6, f"graph replay vs eager gradients: cos {cos} rel {rel}"
    losses = []
    for _ in range(5):
        ts.run(1e-3)
        losses.append(ts.total_loss())
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0], f"loss did not go down over 5 replayed steps on a fixed batch: {losses}"
    return unet, ts


@pytest.mark.parametrize("version,B,rank", [("tiny15", 2, 128), ("tinyxl", 1, 128), ("tiny15", 1, 96), ("tinyxl", 2, 96)])
def test_wide_step_matches_fp32_oracle(version, B, rank):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    unet, _ = _step(version, B, rank)
    assert unet.arena.wide and unet.arena.Rp == 128


def test_forced_wide_rank64_matches_fused(monkeypatch):
    """SDLT_LORA_WIDE_MIN=64: the same rank-64 adapters through the wide decomposition give the fused kernels' gradients."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sd_lora_trainer_amd.unet as M
    from tests.test_step_gpu import _cos_rel
    unet0, ts0 = _step("tinyxl", 2, 64, graph=False)
    assert not unet0.arena.wide
    g0, l0 = unet0.arena.grads.clone(), float(ts0.loss)
    monkeypatch.setattr(M, "LORA_WIDE_MIN", 64)
    unet1, ts1 = _step("tinyxl", 2, 64, graph=False)
    assert unet1.arena.wide
    cos, rel = _cos_rel(unet1.arena.grads, g0)
    # two bf16 evaluation orders of the same step (T rounded once per tile vs once per launch, different K walks) through ~40 bf16 layers:
    # measured cos 0.99966 / rel 2.6e-2 on tinyxl - both paths meet the fp32-oracle bars on their own (test_wide_step_matches_fp32_oracle,
    # tests/test_step_gpu.py)
    assert cos >= 0.999, f"wide vs fused rank-64 gradients: cos {cos} rel {rel}"
    assert abs(float(ts1.loss) - l0) <= 1e-3 * abs(l0)


@pytest.mark.parametrize("version,B,h,n_steps", [("sd15", 4, 32, 2), ("sdxl", 1, 32, 1)])
def test_wide_real_topology(version, B, h, n_steps):
    from tests.test_real_topology_gpu import _case_step_and_trajectory
    _case_step_and_trajectory(version, B, h=h, n_steps=n_steps, rank=128)


def test_wide_job_writes_loadable_checkpoint(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    monkeypatch.chdir(tmp_path)
    from sd_lora_trainer_amd import topology
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.checkpoint import load_lora
    from sd_lora_trainer_amd.config import TrainingConfig
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model={"path": "synthetic:tiny15"}, seed=1, resolution=128,
                         train_batch_size=1, max_train_steps=4, lora_rank=128, text_encoder_lora_optimizer="adamw", text_encoder_lora_rank=128,
                         checkpointing_steps=1000)
    gen = T.train(cfg)
    progress = []
    try:
        while True:
            progress.append(next(gen))
    except StopIteration as e:
        config, out_dir = e.value
    assert progress[-1] == 1.0
    ta = json.load(open(os.path.join(out_dir, "training_args.json")))
    assert all(np.isfinite(ta["training_attributes"]["losses"]["tot_loss"]))
    path = next(os.path.join(out_dir, f) for f in os.listdir(out_dir) if f.endswith("_lora.safetensors"))
    lo = load_lora(path, topology.lora_targets(topology.CONFIGS["tiny15"]))
    assert lo and all(A.shape[0] == 128 and B.shape[1] == 128 and torch.isfinite(A).all() and torch.isfinite(B).all() for A, B in lo.values())
