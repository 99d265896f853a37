"""sdlt_attn_nag_fwd (cross-attention with normalized attention guidance, csrc/attn_nag.hip) against its formula in float64 from the bf16-rounded inputs, at
the attention forward test's bar times the blend's amplification; and UNet.set_attention_nag against the plain forward."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
STD = (5.0, 2.5, 0.5)


def _ref64(q, k, v, neg, B, H, Nq, Nk, Nkp, d, scale, s, tau, alpha):
    """-> O, max(|z+|, |z-|), the clip factors c [rows] of the guided rows - all float64"""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    def attend(b, m):
        z = torch.zeros(Nq, H * d, dtype=torch.float64)
        for h in range(H):
            cols, rows = slice(h * d, (h + 1) * d), slice(m * Nkp, m * Nkp + Nk)
            z[:, cols] = torch.softmax(scale * q[b * Nq:(b + 1) * Nq, cols] @ k[rows, cols].T, dim=-1) @ v[rows, cols]
        return z
    out, big, cs = torch.zeros(B * Nq, H * d, dtype=torch.float64), 0.0, []
    for b in range(B):
        zp = attend(b, b)
        o, big = zp, max(big, float(zp.abs().max()))
        if 0 <= neg[b] < B and alpha != 0 and s != 1:
            zn = attend(b, neg[b])
            e = s * zp - (s - 1) * zn
            n, ne = zp.abs().sum(1), e.abs().sum(1)
            c = torch.where(ne <= tau * n, torch.ones_like(n), tau * n / ne)
            o, big = (1 - alpha) * zp + alpha * c[:, None] * e, max(big, float(zn.abs().max()))
            cs.append(c)
        out[b * Nq:(b + 1) * Nq] = o
    return out, big, torch.cat(cs) if cs else torch.ones(0, dtype=torch.float64)


@pytest.mark.parametrize("B,H,Nq,Nk,Nkp,d,neg,sta,sharp,strided,table", [
    (1, 1, 1, 1, 8, 64, [0], STD, 1, False, False),                  # minimum of every extent; the negative is the own row: c = 1
    (2, 2, 17, 77, 128, 64, [-1, 0], STD, 1, False, False),          # fewer heads than waves, one row past a tile, the pair layout
    (2, 2, 17, 77, 128, 64, [-1, 0], (5.0, 1e9, 1.0), 1, False, False),
    (2, 2, 17, 77, 128, 64, [-1, 0], (3.0, 1.0, 0.25), 1, False, False),
    (2, 5, 16, 77, 128, 64, [-1, 0], STD, 1, False, False),          # uneven heads over four waves
    (2, 20, 33, 77, 128, 64, [-1, 0], STD, 1, False, False),         # deepest register case, SDXL
    (2, 8, 16, 80, 80, 160, [-1, 0], STD, 1, False, False),          # widest heads
    (2, 8, 16, 80, 80, 160, [-1, 0], (5.0, 1e9, 1.0), 1, False, False),
    (2, 8, 16, 80, 80, 160, [-1, 0], (3.0, 1.0, 0.25), 1, False, False),
    (2, 8, 130, 77, 128, 40, [-1, 0], STD, 1, False, False),         # pad columns
    (3, 2, 24, 77, 128, 64, [1, 1, 7], STD, 1, False, False),        # negative = another row, own row, out of range treated as -1
    (2, 2, 40, 77, 128, 64, [-1, 0], STD, 1, True, False),           # K and V as column slices of one [rows, 2 C] buffer
    (2, 2, 24, 77, 128, 64, [-1, 0], STD, 4, False, False),          # sharp logits
    (2, 3, 24, 128, 128, 80, [-1, 0], STD, 1, False, True),          # a 3-row table, ctr at 1
])
def test_attn_nag_matches_fp64(B, H, Nq, Nk, Nkp, d, neg, sta, sharp, strided, table):
    # key rows [Nk, Nkp) hold 1e4 (K) / -1e4 (V); sharp: scale sharp / sqrt(d); table: rows 0 and 2 have alpha 0, ctr points at row 1
    from sd_lora_trainer_amd import ops
    g, C, scale, (s, tau, alpha) = torch.Generator().manual_seed(1000 * Nq + 10 * Nk + d + H), H * d, sharp / math.sqrt(d), sta
    q = torch.randn(B * Nq, C, generator=g).to(BF16).cuda()
    kv = torch.randn(B * Nkp, 2 * C, generator=g).to(BF16).view(B, Nkp, 2 * C)
    kv[:, Nk:, :C], kv[:, Nk:, C:] = 1e4, -1e4
    kv = kv.view(B * Nkp, 2 * C).cuda()
    k, v = (kv[:, :C], kv[:, C:]) if strided else (kv[:, :C].contiguous(), kv[:, C:].contiguous())
    tab = torch.tensor([[s, tau, 0.0, 0.0], [s, tau, alpha, 0.0], [s, tau, 0.0, 0.0]] if table else [[s, tau, alpha, 0.0]]).cuda()
    ctr = torch.tensor([1, 0], dtype=torch.int32).cuda() if table else None
    ref, big, c = _ref64(q, k, v, neg, B, H, Nq, Nk, Nkp, d, scale, s, tau, alpha)
    assert torch.isfinite(ref).all() and big > 0.1
    # the reference itself must exercise what the case is for
    own = all(m == b or not 0 <= m < B for b, m in enumerate(neg))
    if own:
        assert bool((c == 1).all())
    elif tau == 2.5:
        assert bool((c < 1).any()), "no clipped row in the reference"
    elif tau == 1e9:
        assert bool((c == 1).all())
    outs = []
    for _ in range(2):
        buf = torch.full((B * Nq + 8, C), 7.0, dtype=BF16, device="cuda")
        ops.attn_nag_fwd(q, k, v, buf[:B * Nq], torch.tensor(neg, dtype=torch.int32).cuda(), tab, B=B, H=H, Nq=Nq, Nk=Nk, Nkp=Nkp, d=d, scale=scale, ctr=ctr)
        torch.cuda.synchronize()
        assert bool((buf[B * Nq:] == 7.0).all()), "rows beyond B Nq were written"
        outs.append(buf[:B * Nq].clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    # O = a z+ - b z- with a + b <= (1 - alpha) + alpha (2 s - 1): the attention forward test's 1.5e-2 times that factor
    err, bar = float((outs[0].double().cpu() - ref).abs().max()), 1.5e-2 * ((1 - alpha) + alpha * (2 * s - 1)) * big + 1e-6
    print(f"attn_nag {(B, H, Nq, Nk, Nkp, d)} neg={neg} {sta}: max err {err:.3e} (bar {bar:.3e}), clipped rows {int((c < 1).sum())} / {c.numel()}")
    assert err <= bar


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_nag_identities(version):
    from oracle import unet_ref as U
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import topology
    from tests.test_attn_couple_gpu import _cmp
    B, h, w, cfg, g = 2, 8, 12, U.CONFIGS[version], torch.Generator().manual_seed(11)
    x, tf = torch.randn(B, 4, h, w, generator=g), torch.tensor([500.0, 200.0]).cuda()
    ctx = torch.randn(3, 77, cfg["cross_dim"], generator=g)
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    rt = M.Runtime("cuda:0", B)
    extra = (torch.randn(B, P, generator=g).to(rt.act).cuda(), torch.tensor([64., 96, 0, 0, 64, 96]).repeat(B).cuda()) if P else ()
    unet = M.UNet(rt, topology.CONFIGS[version], U.init_unet_state(cfg, seed=0), lora_rank=4)
    unet.arena.load(U.init_lora(cfg, 4, seed=1, b_std=0.05))
    x64 = torch.nn.functional.pad(x.permute(0, 2, 3, 1).reshape(-1, 4), (0, 60)).to(rt.act).cuda()
    def run(c):      # c [B, 77, D] -> ctx rows [B CTX_PAD, D]
        rows = torch.zeros(B, M.CTX_PAD, c.shape[-1], dtype=rt.act, device="cuda")
        rows[:, :77] = c.to(rt.act)
        return unet.forward(x64, tf, rows.view(-1, c.shape[-1]), *extra, B=B, H=h, W=w, train=False).clone()
    tab, i32, half = torch.tensor([[5.0, 2.5, 0.5, 0.0]]).cuda(), dict(dtype=torch.int32, device="cuda"), x64.shape[0] // 2
    plain, plain11 = run(ctx[[0, 1]]), run(ctx[[1, 1]])
    unet.set_attention_nag(dict(neg_row=torch.tensor([-1, -1], **i32), tab=tab, ctr=None))
    off = run(ctx[[0, 1]])
    _cmp(off, plain, "(a) every neg_row -1: plain attention from the other kernel")
    unet.set_attention_nag(dict(neg_row=torch.tensor([-1, 0], **i32), tab=tab, ctr=None))      # the sampler's (negative, positive) pair
    _cmp(run(ctx[[1, 1]]), plain11, "(b) the same context on both rows of the pair: e = z+, c = 1")
    got = run(ctx[[0, 1]])
    assert torch.equal(got[:half], off[:half]), "the negative row changed"
    assert torch.isfinite(got).all() and not torch.equal(got[half:], off[half:]), "a different negative context left the positive row unchanged"
    unet.set_attention_nag(None)
    assert torch.equal(run(ctx[[0, 1]]), plain)      # off again: the plain launches, the same bits


def test_render_cli_nag(tmp_path, monkeypatch):
    # a one-step tinyxl job, four steps: the replayed graph and the eager loop write the same bytes (the counter walks the table in both); --nag changes the
    # picture; --nag 5 --nag-alpha 0 is the plain picture from the other kernel
    import numpy as np
    from PIL import Image
    from sd_lora_trainer_amd import ops, render as R, train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_hires_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="nag job", seed=3, resolution=256, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    calls, real = [], ops.attn_nag_fwd
    monkeypatch.setattr(ops, "attn_nag_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--negative-prompt", "a red barn", "--size", "64", "96", "--steps", "4", "--seed", "11"]
    pics = {}
    for out, extra in (("graph", ["--nag"]), ("eager", ["--nag", "--eager"]), ("plain", []), ("alpha0", ["--nag", "5", "--nag-alpha", "0"])):
        del calls[:]
        R.main(common + ["--out", str(tmp_path / out)] + extra)
        files = list((tmp_path / out).glob("img_00_seed11_scale*.jpg"))
        assert len(files) == 1 and bool(calls) == (out != "plain")
        pics[out] = (open(files[0], "rb").read(), np.asarray(Image.open(files[0]), dtype=np.float64))
    assert pics["graph"][0] == pics["eager"][0]
    assert pics["graph"][0] != pics["plain"][0]
    # alpha 0 runs every cross-attention as plain attention from the OTHER kernel: the same picture up to what another bf16 kernel changes, seen through two
    # JPEG files.  No neighbouring test has a closeness bar for two JPEGs, so it is built from two that exist: the max-error bar of a UNet output from another
    # kernel (tests/test_attn_couple_gpu._cmp: 5e-2 of the range, here 255 levels) plus the quality-95 round trip of each file, taken as 6 levels per file.
    diff, bar = float(np.abs(pics["alpha0"][1] - pics["plain"][1]).max()), 5e-2 * 255 + 2 * 6
    print(f"--nag 5 --nag-alpha 0 against the plain picture: max pixel difference {diff:g} of 255 (bar {bar:g}); --nag against plain: "
          f"{float(np.abs(pics['graph'][1] - pics['plain'][1]).max()):g}")
    assert diff <= bar
