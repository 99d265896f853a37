"""Key / value token downsampling on the MI355X: the sdlt_token_pool kernel against the fp32 restatement (tests/kvpool_ref.py) at the tolerance of the
LayerNorm forward test, its pad rows and its determinism; a self-attention block with pooled keys and values against the torch restatement at the
tolerance of the attention forward test; LatentSampler.sample(kv_downsample=) on tinyxl - off is free, graph == eager, repeatable, and as close to its
plain run as the CPU restatement is to its own; and a two-pass render whose second pass alone carries the setting."""
import functools
import json
import math
import os

import pytest
import torch

from tests import kvpool_ref as KR
from tests.test_img2img_gpu import _cuda, _inputs, _run, _setup
from tests.test_kernels_gpu import close, dev, rnd
from tests.test_sampler_gpu import TOL_COS          # the sampler's bar against the fp32 oracle loop: how far a device trajectory may turn from its fp32 twin

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = -7.25
# (B, H, W, C, f, extra leading dimension): each the smallest shape with its reason
SHAPES = {
    "odd-5x7": (2, 5, 7, 320, 2, 0),            # odd in both axes: partial windows on both edges, two images, 12 keys padded to 16
    "exact-8x12": (1, 8, 12, 640, 4, 0),        # exact division, non-square; 6 keys padded to 8; 80 chunks: the second chunk of 16 lanes
    "wide-6x6": (2, 6, 6, 1280, 3, 0),          # the widest rows (three chunks per lane, the third on 32 lanes), an odd factor, 4 keys padded to 8
    "strip-9x4": (1, 9, 4, 640, 4, 0),          # the last output row is a window of one row by four columns
    "strided-5x7": (2, 5, 7, 320, 2, 64),       # a view with ldx = 384 > C
}
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> x bf16 [B H W, ld] on the CPU (columns past C hold a sentinel), gamma, beta, {mode: fp32 reference [B Nkp, C]}.  Computed once and shared."""
    B, H, W, C, f, pad = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.full((B * H * W, C + pad), 100.0, dtype=BF)
    x[:, :C] = (torch.randn(B * H * W, C, generator=g) * 1.5 + 0.3 + torch.randn(B * H * W, 1, generator=g)).to(BF)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    want = {m: KR.token_pool_ref(x[:, :C], B=B, H=H, W=W, gamma=gamma, beta=beta, eps=EPS, f=f, mode=m) for m in KR.MODES}
    return x, gamma, beta, want


def _pool(name, mode):
    from sd_lora_trainer_amd import ops
    B, H, W, C, f, _ = SHAPES[name]
    x, gamma, beta, _ = _case(name)
    Nkp = ops.token_pool_rows(H, W, f)[3]
    xd, gd, bd = dev(x, gamma, beta)
    buf = torch.full((B * Nkp + 3, C), SENT, dtype=BF, device="cuda")          # three rows of tail: nothing is written past y
    y = ops.token_pool(xd[:, :C], buf[: B * Nkp], B=B, H=H, W=W, gamma=gd, beta=bd, eps=EPS, f=f, mode=mode)
    torch.cuda.synchronize()
    assert bool((buf[B * Nkp:] == SENT).all()) and torch.equal(xd.cpu(), x)
    return y.cpu()


@pytest.mark.parametrize("mode", KR.MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_token_pool_kernel(name, mode):
    """Against the fp32 restatement with `close` at its default tolerance (1.5e-2 of the reference's max-abs), as test_layernorm_fwd_bwd holds
    sdlt_layernorm_fwd: both sides round fp32 LayerNorm values to bf16 once.  Pad rows are zero exactly; a second run gives the same bits."""
    B, H, W, C, f, _ = SHAPES[name]
    _, _, Nk, Nkp = KR.token_pool_rows(H, W, f)
    got, want = _pool(name, mode), _case(name)[3][mode]
    err = float((got.float() - want).abs().max())
    print(f"{name} {mode}: max err {err:.4g} of scale {float(want.abs().max()):.4g}")
    close(got, want, what=f"token_pool {name} {mode}")
    assert bool((got.view(B, Nkp, C)[:, Nk:] == 0).all()) and Nkp > Nk
    assert torch.equal(_pool(name, mode), got)


def test_token_pool_factor_one_is_the_layernorm_launch():
    """f = 1: the rows sdlt_layernorm_fwd writes, bit for bit, in either mode (0 + x and x / 1 are exact) - what the plain path's keys are made from."""
    from sd_lora_trainer_amd import ops
    B, H, W, C, _, _ = SHAPES["odd-5x7"]
    x, gamma, beta, _ = _case("odd-5x7")
    xd, gd, bd = dev(x[:, :C].contiguous(), gamma, beta)
    M = B * H * W
    Nkp = ops.token_pool_rows(H, W, 1)[3]
    ln = ops.layernorm_fwd(xd, torch.empty(M, C, dtype=BF, device="cuda"), torch.zeros(2 * M, device="cuda"), gamma=gd, beta=bd, eps=EPS).cpu()
    for mode in KR.MODES:
        y = ops.token_pool(xd, torch.empty(B * Nkp, C, dtype=BF, device="cuda"), B=B, H=H, W=W, gamma=gd, beta=bd, eps=EPS, f=1, mode=mode).cpu()
        assert torch.equal(y.view(B, Nkp, C)[:, : H * W].reshape(M, C), ln), mode


def test_token_pool_errors_launch_nothing():
    from sd_lora_trainer_amd import _lib, ops
    B, H, W, C = 2, 5, 7, 320
    x, g = torch.zeros(B * H * W, C, dtype=BF, device="cuda"), torch.ones(C, device="cuda")
    y = torch.full((B * 16, C), SENT, dtype=BF, device="cuda")
    kw = dict(B=B, H=H, W=W, gamma=g, beta=g, eps=EPS, f=2, mode="area")
    for bad in (dict(f=6), dict(f=0), dict(mode="cubic"), dict(gamma=g.to(BF)), dict(B=3)):
        with pytest.raises(AssertionError):
            ops.token_pool(x, y, **dict(kw, **bad))
    for args in ((x.float(), y), (x, y[:-8]), (x, y[:, :312]), (x[1:], y)):
        with pytest.raises(AssertionError):
            ops.token_pool(*args, **kw)
    with pytest.raises(_lib.KernelLibraryError, match="overlaps"):
        big = torch.zeros(B * H * W + B * 16, C, dtype=BF, device="cuda")
        ops.token_pool(big[: B * H * W], big[B * H * W - 8: B * H * W + B * 16 - 8], **kw)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


# ---- the attention block ----------------------------------------------------------------------------------------------------------------------
def _block(C, heads, fold, B, seed):
    """One self-attention of `heads` heads with rank-16 adapters on q / k / v / out at adapter scale 0.7 behind its LayerNorm, built as
    TransformerBlock builds attn1 (fold: the LayerNorm folded into the stacked projection, as the 1280-wide blocks have it) -> (norm, attn, the weights)."""
    import sd_lora_trainer_amd.unet as M
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(BF).float()  # noqa: E731
    sd = {"n.weight": 1 + 0.1 * torch.randn(C, generator=g), "n.bias": 0.1 * torch.randn(C, generator=g), "a.to_out.0.bias": 0.1 * torch.randn(C, generator=g)}
    names = dict(q="a.to_q", k="a.to_k", v="a.to_v", out="a.to_out.0")
    for n in names.values():
        sd[n + ".weight"] = bf(torch.randn(C, C, generator=g) * C ** -0.5)
    lora = {n: (bf(torch.randn(16, C, generator=g) * C ** -0.5), bf(torch.randn(C, 16, generator=g) * 0.25)) for n in names.values()}
    rt = M.Runtime("cuda:0", B)
    arena = M.LoraArena(rt, 16)
    norm = M.LayerNorm(rt, "n", sd)
    attn = M.Attention(rt, "a", sd, arena, heads, cross=False, hooked=False)
    attn.norm = norm
    if fold:
        attn.stack.fold_ln(norm, [sd[names[p] + ".weight"] for p in "qkv"])
    arena.finalize()
    arena.load(lora)
    arena.set_scale(0.7)
    ref = dict(gamma=sd["n.weight"], beta=sd["n.bias"], eps=norm.eps, weights={p: sd[n + ".weight"] for p, n in names.items()},
               adapters={p: lora[n] for p, n in names.items()}, scale=0.7, bias_out=sd["a.to_out.0.bias"])
    return norm, attn, ref


@pytest.mark.parametrize("C,heads,fold", [(640, 10, False), (320, 8, False), (1280, 20, True)], ids=["640x10", "sd15-320x8", "folded-1280x20"])
def test_attention_block_with_pooled_keys(C, heads, fold):
    """B = 2, 16 x 24 tokens, f = 2 and f = 4, both modes (the 40-wide heads of SD1.5 and the folded 1280-wide block: f = 2 nearest, once) against
    kvpool_ref.attention_block: softmax(q k_pool^T / sqrt(d)) v_pool, to_out, the residual.  Tolerance: test_attention_fwd_bwd compares O with
    `close(O, O_ref)` at the helper's default, 1.5e-2 of the reference's max-abs; the same here on the block's output.  The plain path of the same
    module (f = 1) is held to the same bar first, so the reference is known to describe this module."""
    B, H, W = 2, 16, 24
    N = H * W
    norm, attn, ref = _block(C, heads, fold, B, seed=C + heads)
    g = torch.Generator().manual_seed(7)
    x = (rnd(B * N, C, g=g, scale=1.5) + 0.3)
    xd = x.cuda()

    def run():
        return attn.forward(norm.forward(xd), None, B, N, residual=xd, grid=(H, W)).float().cpu()

    plain = run()
    close(plain, KR.attention_block(x, B=B, H=H, W=W, heads=heads, f=1, mode="nearest", **ref), what="plain block")
    q_plain = attn.to_q._b["y"].clone()
    cases = [(2, "nearest"), (2, "area"), (4, "nearest"), (4, "area")] if (C, fold) == (640, False) else [(2, "nearest")]
    for f, mode in cases:
        attn._kv = (f, KR.MODES.index(mode))
        got = run()
        want = KR.attention_block(x, B=B, H=H, W=W, heads=heads, f=f, mode=mode, **ref)
        err, moved = float((got - want).abs().max()), float((got - plain).abs().max())
        print(f"C={C} f={f} {mode}: max err {err:.4g} of scale {float(want.abs().max()):.4g}; the option moves the output by {moved:.4g}")
        close(got, want, what=f"pooled block C={C} f={f} {mode}")
        assert moved > 0 and torch.equal(run(), got)
        # q: the same operands (the stack's rows of to_q, folded or not) in a product of its own instead of the first third of the stacked one; held
        # to the bar test_kernels_gpu.py holds one GEMM kernel to against another (1e-2), since tile and K-split choices follow the output's width
        print(f"    q bit-equal to the stacked product's: {torch.equal(attn._b['q_ds'], q_plain)}")
        close(attn._b["q_ds"], q_plain, tol=1e-2, what="q of the pooled path vs the stacked product")
    attn._kv = None
    assert torch.equal(run(), plain)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------------
def _cos(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return float(a @ b / (a.norm() * b.norm()))


def test_sampler_on_tinyxl():
    """16 x 16 latent (the largest self-attention grid is 8 x 8: 64 queries, 16 pooled keys), 3 Euler steps.  (1,) is the run without the option, bit
    for bit, on the graph path and the eager one.  (2,): graph == eager and a second call == the first, bit for bit; the result differs from the plain
    run, is finite, and is as close to it as the CPU restatement (the same sampler on the fp32 emulated op table, tests/kvpool_ref.emu_kv, with the same
    weights) is to ITS plain run: each device trajectory may turn from its fp32 twin by the angle of tests/test_sampler_gpu.py's bar, arccos(TOL_COS), so
    the device pair's angle is at most the restatement pair's plus twice that.  A mis-wired pool (wrong rows, no normalisation) fails this."""
    import sd_lora_trainer_amd.unet as unet_mod
    from sd_lora_trainer_amd import sampler as SM
    from sd_lora_trainer_amd import topology
    h = w = 16
    cfg, sd, lora, smp = _setup("tinyxl")
    embeds, noise, _ = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    kw = dict(steps=3, guidance_scale=8.0, latents=noise.cuda())
    plain_g, plain_e = smp.sample(em, h, w, graph=True, **kw).cpu(), smp.sample(em, h, w, fused=True, **kw).cpu()
    assert torch.equal(smp.sample(em, h, w, graph=True, kv_downsample=(1,), **kw).cpu(), plain_g)
    assert torch.equal(smp.sample(em, h, w, fused=True, kv_downsample=(1,), **kw).cpu(), plain_e) and len(smp._graphs) == 1
    rows = {}
    for mode in KR.MODES:
        graph = smp.sample(em, h, w, graph=True, kv_downsample=(2,), kv_downsample_mode=mode, **kw).cpu()
        assert torch.isfinite(graph).all()
        assert torch.equal(smp.sample(em, h, w, fused=True, kv_downsample=(2,), kv_downsample_mode=mode, **kw).cpu(), graph)
        assert torch.equal(smp.sample(em, h, w, graph=True, kv_downsample=(2,), kv_downsample_mode=mode, **kw).cpu(), graph)
        assert not torch.equal(graph, plain_g)
        rows[mode] = graph
    assert not torch.equal(rows["nearest"], rows["area"]) and len(smp._graphs) == 3            # a capture per setting, never a stale replay
    assert torch.equal(smp.sample(em, h, w, graph=True, **kw).cpu(), plain_g) and smp.unet._kv_ds is None
    # the restatement: the same model in fp32 on the emulated table
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=KR.emu_kv)
    unet = unet_mod.UNet(rt, topology.CONFIGS["tinyxl"], sd, lora_rank=8)
    unet.arena.load(lora)
    ref = SM.LatentSampler(rt, unet)
    ref.set_lora_scale(0.75)
    kw_ref = dict(steps=3, guidance_scale=8.0, latents=noise)
    ref_plain = ref.sample(embeds[0], h, w, **kw_ref)
    turn = 2 * math.acos(TOL_COS)
    for mode in KR.MODES:
        ref_ds = ref.sample(embeds[0], h, w, kv_downsample=(2,), kv_downsample_mode=mode, **kw_ref)
        c_ref, c_dev = _cos(ref_ds, ref_plain), _cos(rows[mode], plain_g)
        bar = math.cos(min(math.pi, math.acos(min(1.0, c_ref)) + turn))
        print(f"tinyxl (2,) {mode}: cos(device, device plain) {c_dev:.6f}; restatement {c_ref:.6f}; bar {bar:.6f}; device vs restatement {_cos(rows[mode], ref_ds):.6f}")
        assert c_dev >= bar, (mode, c_dev, c_ref, bar)


# ---- render -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    root = tmp_path_factory.mktemp("kv_job")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        tok_dir, _ = _tokenizer_dir(root)
        cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="kv job", seed=3, resolution=256, train_batch_size=1,     # (tinyxl trains from 256 px up: its smallest hooked grid must hold 64 tokens)
                             max_train_steps=1, checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(root / "job"),
                             pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
        _, ckdir = _run(T.train(cfg))
    finally:
        os.chdir(cwd)
    return ckdir


def test_render_hires_second_pass_alone(ckpt_dir, tmp_path, monkeypatch):
    """render.main --hires-scale 2 --kv-downsample 2 on tinyxl writes its pictures; the sample() calls show that the first pass ran without the setting
    and the second with it (the UNet's own state after each call says the same); prompts.json records it."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import sampler as SM
    log = []
    real = SM.LatentSampler.sample

    def spy(self, embeds, h, w, **kw):
        out = real(self, embeds, h, w, **kw)
        log.append((h, w, kw.get("kv_downsample"), self.unet._kv_ds))
        return out

    monkeypatch.setattr(SM.LatentSampler, "sample", spy)
    out = tmp_path / "kv"
    res = R.main(["--checkpoint", ckpt_dir, "--out", str(out), "--prompt", "a photo of <concept>", "--size", "64", "64", "--steps", "4", "--seed", "11",
                  "--hires-scale", "2", "--kv-downsample", "2"])
    (paths,) = res.values()
    assert len(paths) == 1 and Image.open(paths[0]).size == (128, 128)
    assert len(log) == 2 and log[0][2:] == (None, None) and log[1][2:] == ((2,), ((2,), "nearest")) and log[1][0] == 2 * log[0][0]
    assert json.load(open(out / "prompts.json"))["kv_downsample"] == dict(factors=[2], mode="nearest", passes="hires")
