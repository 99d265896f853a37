"""sdlt_attn_couple_fwd (region-coupled cross-attention, csrc/attn_couple.hip) against its formula in float64 from the bf16-rounded inputs, at the attention
forward test's bar (tests/test_kernels_gpu.py, tests/test_attn_wide_gpu.py), and UNet.set_attention_couple against the plain forward."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _weights(case, R, Nq, g):
    if case == "hard":      # contiguous query ranges, no multiple of 16; region 5 owns exactly query 63, the last of tile 0; regions 6 and 7 own nothing
        own = torch.tensor([0] * 37 + [1] * 26 + [5] + [2] * 37 + [3] * 49 + [4] * 50)
        return (torch.arange(R)[:, None] == own[None, :]).float()
    wt = torch.ones(R, Nq) if case == "ones" else torch.rand(R, Nq, generator=g) + 0.05
    return wt / wt.sum(0, keepdim=True) if case == "norm" else wt


def _ref64(q, k, v, wt, rc, B, H, Nq, Nk, Nkp, d, R, scale):
    q, k, v, wt = q.double().cpu(), k.double().cpu(), v.double().cpu(), wt.double().cpu()
    out = torch.zeros(B * Nq, H * d, dtype=torch.float64)
    for b, hd in ((b, hd) for b in range(B) for hd in range(H)):
        cols, qs = slice(hd * d, (hd + 1) * d), slice(b * Nq, (b + 1) * Nq)
        for r in range(rc[b]):
            rows = slice((b * R + r) * Nkp, (b * R + r) * Nkp + Nk)
            out[qs, cols] += wt[r][:, None] * (torch.softmax(scale * q[qs, cols] @ k[rows, cols].T, dim=-1) @ v[rows, cols])
    return out


@pytest.mark.parametrize("B,H,Nq,Nk,Nkp,d,R,wcase,rcount,sharp,strided", [
    (1, 1, 1, 1, 8, 64, 1, "rand", None, 1, False), (1, 2, 16, 77, 128, 64, 1, "ones", None, 1, False), (2, 2, 72, 77, 128, 64, 3, "norm", [1, 3], 1, False),
    (1, 1, 130, 80, 80, 40, 2, "rand", None, 1, False), (1, 1, 64, 17, 24, 160, 4, "rand", None, 4, False), (1, 1, 200, 128, 128, 80, 8, "hard", None, 1, False),
    (1, 3, 24, 77, 128, 32, 16, "rand", None, 1, False), (1, 2, 96, 77, 128, 64, 2, "rand", None, 1, True)])
def test_attn_couple_matches_fp64(B, H, Nq, Nk, Nkp, d, R, wcase, rcount, sharp, strided):
    # key rows [Nk, Nkp) hold 1e4 (K) / -1e4 (V), regions >= rcount[b] NaN; sharp: scale sharp / sqrt(d); strided: K, V are column slices of one [rows, 2 C] buffer
    from sd_lora_trainer_amd import ops
    g, C, scale, rc = torch.Generator().manual_seed(1000 * Nq + 10 * Nk + d + R), H * d, sharp / math.sqrt(d), rcount or [R] * B
    q = torch.randn(B * Nq, C, generator=g).to(BF16).cuda()
    kv = torch.randn(B * R * Nkp, 2 * C, generator=g).to(BF16).view(B, R, Nkp, 2 * C)
    kv[:, :, Nk:, :C], kv[:, :, Nk:, C:] = 1e4, -1e4
    for b in range(B):
        kv[b, rc[b]:] = float("nan")
    kv = kv.view(B * R * Nkp, 2 * C).cuda()
    k, v = (kv[:, :C], kv[:, C:]) if strided else (kv[:, :C].contiguous(), kv[:, C:].contiguous())
    wt = _weights(wcase, R, Nq, g).cuda()
    ref = _ref64(q, k, v, wt, rc, B, H, Nq, Nk, Nkp, d, R, scale)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0.1
    outs = []
    for _ in range(2):
        buf = torch.full((B * Nq + 8, C), 7.0, dtype=BF16, device="cuda")
        ops.attn_couple_fwd(q, k, v, buf[:B * Nq], wt, B=B, H=H, Nq=Nq, Nk=Nk, Nkp=Nkp, R=R, d=d, scale=scale,
                            rcount=torch.tensor(rcount, dtype=torch.int32, device="cuda") if rcount else None)
        torch.cuda.synchronize()
        assert bool((buf[B * Nq:] == 7.0).all()), "rows beyond B Nq were written"
        outs.append(buf[:B * Nq].clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    err, bar = float((outs[0].double().cpu() - ref).abs().max()), 1.5e-2 * float(ref.abs().max()) + 1e-6
    print(f"attn_couple {(B, H, Nq, Nk, Nkp, d, R)} {wcase}: max err {err:.3e} (bar {bar:.3e})")
    assert err <= bar


def _cmp(a, b, what, cos_below=None):      # tests/test_attn_wide_gpu.py's bars, or a cap on the cosine alone
    err, a, b = float((a.float() - b.float()).abs().max()) / float(b.float().abs().max()), a.float().cpu().reshape(-1).double(), b.float().cpu().reshape(-1).double()
    cos = float(a @ b / (a.norm() * b.norm()))
    assert cos < cos_below if cos_below else (err <= 5e-2 and cos >= 0.995), (what, err, cos)


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_couple_identities(version):
    from oracle import unet_ref as U
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import ops, topology
    B, h, w, R, cfg, g = 2, 8, 12, 3, U.CONFIGS[version], torch.Generator().manual_seed(11)      # innermost token grid 2 x 3
    x, tf = torch.randn(B, 4, h, w, generator=g), torch.tensor([500.0, 200.0]).cuda()
    # unscaled contexts: the ORACLE's plain forwards of prompts 0 and 1 at these seeds have cos 0.911 (tiny15) / 0.913 (tinyxl): the reference alone meets the cap of (b)
    ctx = torch.randn(B, R, 77, cfg["cross_dim"], generator=g)
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    rt = M.Runtime("cuda:0", B)
    extra = (torch.randn(B, P, generator=g).to(rt.act).cuda(), torch.tensor([64., 96, 0, 0, 64, 96]).repeat(B).cuda()) if P else ()
    unet = M.UNet(rt, topology.CONFIGS[version], U.init_unet_state(cfg, seed=0), lora_rank=4)
    unet.arena.load(U.init_lora(cfg, 4, seed=1, b_std=0.05))
    x64 = torch.nn.functional.pad(x.permute(0, 2, 3, 1).reshape(-1, 4), (0, 60)).to(rt.act).cuda()
    def run(c):      # c [B, S, 77, D] -> ctx rows [B S CTX_PAD, D]
        rows = torch.zeros(B, c.shape[1], M.CTX_PAD, c.shape[-1], dtype=rt.act, device="cuda")
        rows[:, :, :77] = c.to(rt.act)
        return unet.forward(x64, tf, rows.view(-1, c.shape[-1]), *extra, B=B, H=h, W=w, train=False).clone()
    plain0, plain1 = run(ctx[:, :1]), run(ctx[:, 1:2])
    levels = sorted({l for _, l in unet._attn_levels()})
    wn = torch.rand(R, h, w, generator=g) + 0.05
    tabs = {N: t.cuda() for N, t in ops.couple_weights(wn / wn.sum(0, keepdim=True), levels).items()}
    unet.set_attention_couple(dict(R=R, weights=tabs, rcount=torch.full((B,), R, dtype=torch.int32, device="cuda")))
    _cmp(run(ctx[:, :1].expand(B, R, 77, -1)), plain0, "(a) the same context in every slot, random weights: the plain forward in another summation")
    for N, t in ops.couple_weights(torch.eye(R)[1].view(R, 1, 1).expand(R, h, w).contiguous(), levels).items():
        tabs[N].copy_(t)
    got = run(ctx)
    _cmp(got, plain1, "(b) hard weights give region 1 the whole picture (the tables are the caller's device buffers: rewritten in place)")
    _cmp(got, plain0, "a kernel that ignores the weights would equal region 0's forward", cos_below=0.99)
    unet.set_attention_couple(None)
    assert torch.equal(run(ctx[:, :1]), plain0)      # off again: the plain launches, the same bits


def test_sampler_couple_paths(monkeypatch):
    # graph == fused == torch loop bit for bit; one capture serves another mask set (device tables, rewritten per call); no region_gather; the setting does not stick
    from sd_lora_trainer_amd import ops
    from tests.test_region_gpu import H, PATHS, W, _cuda, _inputs, _regions, _setup, hard_masks      # (its own helpers and those it borrows)
    cfg, sd, lora, smp = _setup("tiny15")      # a runtime of batch 2 n: one UNet pass
    monkeypatch.setattr(ops, "region_gather", lambda *a, **k: pytest.fail("region_gather launched in couple mode"))
    embeds, noise, _ = _inputs(cfg, 5, H, W, 1)
    em, rg = _cuda(embeds)[0], _regions(cfg, mode="couple")
    run = lambda path, **kw: smp.sample(em, H, W, steps=4, guidance_scale=8.0, guidance_rescale=0.5, latents=noise.cuda(), **PATHS[path], **kw).cpu()  # noqa: E731
    plain, fused = run("fused"), run("fused", regions=rg)
    assert torch.isfinite(fused).all() and not torch.equal(fused, plain)
    assert torch.equal(run("graph", regions=rg), fused) and torch.equal(run("torch", regions=rg), fused)
    other = _regions(cfg, masks=hard_masks(), mode="couple")
    n_graphs = len(smp._guided_graphs)
    o = run("graph", regions=other)
    assert torch.equal(o, run("fused", regions=other)) and not torch.equal(o, fused) and len(smp._guided_graphs) == n_graphs
    assert torch.equal(run("graph", regions=rg), fused)      # ... and back: the replayed capture reads the rewritten tables
    assert torch.equal(run("fused"), plain) and smp.unet._couple is None
    # plain graph -> couple graph -> plain graph -> couple graph on one sampler: both captures replay after the switch (their k | v buffers are keyed by row count)
    for _ in range(2):
        assert torch.equal(run("graph"), plain) and torch.equal(run("graph", regions=rg), fused)
    assert len(smp._guided_graphs) == n_graphs + 1


def test_render_cli_region_mode_couple(tmp_path, monkeypatch):
    # a one-step tinyxl job, four steps, the graph path and the eager loop: every cross-attention of every iteration Python issues is the coupled launch
    import json
    from PIL import Image
    from sd_lora_trainer_amd import ops, render as R, train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_hires_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="couple job", seed=3, resolution=256, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    calls, real = [], ops.attn_couple_fwd
    monkeypatch.setattr(ops, "attn_couple_fwd", lambda *a, **k: (calls.append(k["R"]), real(*a, **k))[1])
    monkeypatch.setattr(ops, "region_gather", lambda *a, **k: pytest.fail("region_gather launched in couple mode"))
    common = ["--checkpoint", ckdir, "--prompt", "a photo of a field", "--size", "64", "96", "--steps", "4", "--seed", "11",
              "--region", "0,0,0.5,1", "a photo of <concept>", "--region", "0.5,0,1,1", "a red barn", "--region-mode", "couple"]
    n_cross = len(R.load_for_inference(ckdir).stack.unet.cross_attns)
    for out, extra, iterations in (("graph", [], None), ("eager", ["--eager"], 4)):
        del calls[:]
        R.main(common + ["--out", str(tmp_path / out)] + extra)
        pics = list((tmp_path / out).glob("img_00_seed11_scale*.jpg"))
        assert len(pics) == 1 and Image.open(pics[0]).size == (64, 96)
        meta = json.load(open(tmp_path / out / "prompts.json"))
        assert meta["region_mode"] == "couple" and meta["region_bootstrap"] == 0.0 and len(meta["regions"]) == 2
        assert calls and set(calls) == {3} and len(calls) % n_cross == 0 and (iterations is None or len(calls) == n_cross * iterations), (len(calls), n_cross)
    assert open(next((tmp_path / "graph").glob("img_00*.jpg")), "rb").read() == open(next((tmp_path / "eager").glob("img_00*.jpg")), "rb").read()
