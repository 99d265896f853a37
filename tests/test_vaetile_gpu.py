"""Tiled VAE decode / encode on the MI355X: sdlt_tile_blend against its fp32 restatement (tests/vaetile_ref.py: blend32), bit for bit, and against the fp64
composition; its refusals; decode_tiled / encode_moments_tiled against the composition of single-tile passes made by hand; the decoder's buffers; and
`python -m sd_lora_trainer_amd.render --vae-tile` end to end on a tiny15 job."""
import json
import os

import pytest
import torch

from tests import vaetile_ref as TR
from tests.test_hires_gpu import NAME, _main, ckpt_dir  # noqa: F401  (fixture: a one-step tiny15 job; the CLI helper of the hires tests)
from tests.test_vaetile_cpu import buffer_shapes

pytestmark = pytest.mark.gpu

SENT = -7.25
TILE_SHAPES = [(5, 7), (16, 64), (64, 40), (1, 1)]
ROWS = [(3, 4), (8, 8), (1, 1), (3, 3)]          # (C, ld): the decoder's rows, the encoder's, a single plane, and rows that are not 16-byte aligned


def _axis(t, n):
    """n tiles of extent t on one axis with an ODD step between neighbours -> (length, starts, fp32 weight tables)."""
    if n == 1:
        return t, [0], [torch.ones(t)]
    if t == 1:                                   # no overlap is possible: n samples side by side
        return n, list(range(n)), [torch.ones(1) for _ in range(n)]
    O = t // 3
    if (t - O) % 2 == 0:
        O = O + 1 if 2 * (O + 1) <= t else O - 1
    L = n * (t - O) + O
    starts = TR.tile_starts(L, t, O)
    assert starts == [k * (t - O) for k in range(n)] and (t - O) % 2 == 1
    return L, starts, TR.weights32(L, t, O, 1)


def _values(th, tw, ld, gen):
    v = torch.randn(th, tw, ld, generator=gen)
    r = torch.rand(th, tw, ld, generator=gen)
    v = torch.where(r < 0.08, torch.full_like(v, 1e30) * v.sign(), v)                     # large and small magnitudes beside ordinary ones: the order of
    v = torch.where(r > 0.92, torch.full_like(v, 1e-30) * v.sign(), v)                    # the three roundings shows
    return v


def _run_layouts(layouts, C, ld, H, W, tail=64):
    """layouts: [(tiles [th, tw, ld] row-major, ys, xs, wys, wxs)] -> (ops.tile_blend's picture on the CPU, the sentinel tail behind it)."""
    from sd_lora_trainer_amd import ops
    flat = torch.full((C * H * W + tail,), SENT, device="cuda")
    out = flat[: C * H * W].view(C, H, W)
    out.zero_()
    for tiles, ys, xs, wys, wxs in layouts:
        for i, y in enumerate(ys):
            for j, x in enumerate(xs):
                t = tiles[i * len(xs) + j]
                ops.tile_blend(t.reshape(-1, ld).cuda(), out, wys[i].cuda(), wxs[j].cuda(), y, x, C)
    torch.cuda.synchronize()
    return out.cpu(), flat[C * H * W:].cpu()


@pytest.mark.parametrize("C,ld", ROWS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_blend_exact(shape, C, ld):
    """A 3 x 1 layout from the origin and a 2 x 2 layout flush with the far corner, accumulated into one picture: offsets 0, odd offsets, the last sample."""
    th, tw = shape
    gen = torch.Generator().manual_seed(th * 1000 + tw * 10 + ld)
    H3, ys3, wys3 = _axis(th, 3)
    W3, xs3, wxs3 = _axis(tw, 1)
    H2, ys2, wys2 = _axis(th, 2)
    W2, xs2, wxs2 = _axis(tw, 2)
    H, W = max(H3, H2), max(W3, W2)
    ys2, xs2 = [y + H - H2 for y in ys2], [x + W - W2 for x in xs2]
    assert ys3[0] == xs3[0] == 0 and ys2[-1] + th == H and xs2[-1] + tw == W
    if th > 1:
        assert any(v % 2 for v in ys3 + ys2)
    layouts = [([_values(th, tw, ld, gen) for _ in range(3)], ys3, xs3, wys3, wxs3), ([_values(th, tw, ld, gen) for _ in range(4)], ys2, xs2, wys2, wxs2)]
    got, tail = _run_layouts(layouts, C, ld, H, W)
    ref = torch.zeros(C, H, W)
    ref64, scale = torch.zeros(C, H, W, dtype=torch.float64), torch.zeros(C, H, W, dtype=torch.float64)
    for lay in layouts:
        TR.blend32(*lay, C, H, W, out=ref)
        ref64 += TR.blend(*lay, C, H, W)
        scale += TR.blend(*lay, C, H, W, absolute=True)
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref), (shape, C, ld, int((got != ref).sum()), float((got - ref).abs().max()))
    assert bool((tail == SENT).all())
    err = (got.double() - ref64).abs()
    print(f"tile {th}x{tw} C={C} ld={ld}: max error / bound = {float((err / (4 * 2.0 ** -23 * scale).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= 4 * 2.0 ** -23 * scale).all())                                     # at most 4 terms of 3 roundings each


def test_tile_blend_unaligned_base():
    """Rows of 4 floats that start 4 bytes off a 16-byte boundary take the scalar path: the same bits."""
    from sd_lora_trainer_amd import ops
    th, tw, C, ld = 6, 9, 3, 4
    gen = torch.Generator().manual_seed(4)
    v = _values(th, tw, ld, gen)
    wy, wx = torch.rand(th, generator=gen) + 0.01, torch.rand(tw, generator=gen) + 0.01
    buf = torch.zeros(th * tw * ld + 1, device="cuda")
    buf[1:] = v.reshape(-1).cuda()
    tile = buf[1:].view(th * tw, ld)
    assert tile.data_ptr() % 16 == 4
    out = torch.zeros(C, th + 2, tw + 3, device="cuda")
    ops.tile_blend(tile, out, wy.cuda(), wx.cuda(), 2, 3, C)
    assert torch.equal(out.cpu(), TR.blend32([v], [2], [3], [wy], [wx], C, th + 2, tw + 3))


@pytest.mark.parametrize("c", [0.3, 1.75])
def test_constant_in_constant_out(c):
    """3 x 3 tiles with unequal overlaps (19 -> starts 0, 6, 11; 17 -> 0, 5, 9 at tile 8, overlap 2), every tile the constant c: the weights of the up to four
    tiles at a sample sum to 1, so the picture is c within 2 ulp."""
    T, O, g, C, ld = 8, 2, 2, 3, 4
    H, W = 19, 17
    sy, sx = TR.tile_starts(H, T, O), TR.tile_starts(W, T, O)
    assert sy == [0, 6, 11] and sx == [0, 5, 9]
    lay = ([torch.full((g * T, g * T, ld), c) for _ in range(9)], [g * s for s in sy], [g * s for s in sx], TR.weights32(H, T, O, g), TR.weights32(W, T, O, g))
    got, tail = _run_layouts([lay], C, ld, g * H, g * W)
    ulp = float(torch.nextafter(torch.tensor(c), torch.tensor(float("inf"))) - torch.tensor(c))
    print(f"c = {c}: max |out - c| = {float((got - c).abs().max()) / ulp:.2f} ulp")
    assert torch.equal(got, TR.blend32(*lay, C, g * H, g * W))
    assert float((got.double() - float(torch.tensor(c))).abs().max()) <= 2 * ulp and bool((tail == SENT).all())


def test_tile_blend_errors_launch_nothing():
    from sd_lora_trainer_amd import _lib, ops
    from tests.test_vaetile_cpu import lib_tile_blend
    lib = _lib.load()
    th, tw, H, W = 5, 7, 10, 11
    tile = torch.randn(th * tw, 4, device="cuda")
    wide = torch.randn(th * tw, 20, device="cuda")
    wy, wx = torch.rand(th, device="cuda"), torch.rand(tw, device="cuda")
    out = torch.full((16, H, W), SENT, device="cuda")
    ok = dict(tile=tile.data_ptr(), ld=4, th=th, tw=tw, C=3, wy=wy.data_ptr(), wx=wx.data_ptr(), out=out.data_ptr(), H=H, W=W, y0=5, x0=4)
    for change in (dict(tile=None), dict(out=None), dict(wy=None), dict(wx=None),                                                 # a null pointer
                   dict(th=0), dict(tw=0), dict(th=-5), dict(tw=-7), dict(C=0), dict(C=-1), dict(H=0), dict(W=0), dict(H=-10),     # a non-positive extent
                   dict(C=4, ld=3), dict(C=8, ld=4),                                                                              # C > ld
                   dict(C=17, ld=20, tile=wide.data_ptr()),                                                                       # C above the kernel's 16
                   dict(y0=6), dict(x0=5), dict(y0=-1), dict(x0=-1), dict(th=6), dict(tw=8), dict(H=9), dict(W=10)):             # outside H x W
        rc = lib_tile_blend(lib, **dict(ok, **change))
        msg = lib.sdlt_last_error()
        assert rc < 0 and b"sdlt_tile_blend" in msg, (change, rc, msg)
    for bad in (lambda: ops.tile_blend(tile, out[:3], wy, wx, 6, 4, 3), lambda: ops.tile_blend(tile, out[:3], wy, wx, 5, 4, 5),
                lambda: ops.tile_blend(tile.double(), out[:3], wy, wx, 5, 4, 3), lambda: ops.tile_blend(tile, out[:3], wy[:4], wx, 5, 4, 3),
                lambda: ops.tile_blend(tile, out[:3, :, :10], wy, wx, 0, 0, 3)):
        with pytest.raises(AssertionError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- decode_tiled / encode_moments_tiled ------------------------------------------------------------------------------------------------------------
_STATES = {}


def _vae(kind):
    """(cfg, state dict (bf16-rounded, shared), f, make decoder, make encoder)."""
    from oracle import vae_ref as V
    from sd_lora_trainer_amd import vae
    import sd_lora_trainer_amd.unet as M
    cfg = V.CONFIGS[kind]
    if kind not in _STATES:
        _STATES[kind] = {k: v.to(torch.bfloat16).float() for k, v in V.init_state(cfg, seed=0).items()}
    sd = _STATES[kind]
    f = 2 ** (len(cfg["block_out_channels"]) - 1)
    return cfg, sd, f, (lambda: vae.VaeDecoder(M.Runtime("cuda:0", 1), sd)), (lambda: vae.VaeEncoder(M.Runtime("cuda:0", 1), sd))


def test_single_tile_is_the_plain_pass():
    cfg, sd, f, new_dec, new_enc = _vae("tiny")
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(new_dec().decode_tiled(z, tile=8, overlap=2), new_dec().decode(z))
    img = torch.tanh(torch.randn(1, 3, 8 * f, 8 * f, generator=torch.Generator().manual_seed(2))).cuda()
    assert torch.equal(new_enc().encode_moments_tiled(img, tile=8, overlap=2), new_enc().encode_moments(img))


@pytest.mark.parametrize("kind,h,w,T,O", [("tiny", 20, 12, 8, 2), ("tiny", 8, 24, 8, 2), ("sd", 40, 32, 32, 8)])
def test_tiled_passes_are_the_composition_of_their_tiles(kind, h, w, T, O):
    cfg, sd, f, new_dec, new_enc = _vae(kind)
    gen = torch.Generator().manual_seed(h * 100 + w)
    z = torch.randn(1, 4, h, w, generator=gen).cuda()
    ys, xs = TR.tile_starts(h, T, O), TR.tile_starts(w, T, O)
    eh, ew = min(h, T), min(w, T)
    assert len(ys) * len(xs) > 1
    dec = new_dec()
    got = dec.decode_tiled(z, tile=T, overlap=O)
    assert got.shape == (1, 3, f * h, f * w) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    one = dec if kind == "sd" else new_dec()              # (the real topology's 84 M parameters are packed once per pass: its tiles are decoded again by the same plan)
    tiles = [TR.nhwc(one.decode(z[:, :, y:y + eh, x:x + ew])).cpu() for y in ys for x in xs]
    ref = TR.blend32(tiles, [f * y for y in ys], [f * x for x in xs], TR.weights32(h, T, O, f), TR.weights32(w, T, O, f), 3, f * h, f * w)
    assert torch.equal(got[0].cpu(), ref), (int((got[0].cpu() != ref).sum()), float((got[0].cpu() - ref).abs().max()))
    del one, got, dec
    img = torch.tanh(torch.randn(1, 3, f * h, f * w, generator=gen)).cuda()
    enc = new_enc()
    mom = enc.encode_moments_tiled(img, tile=T, overlap=O)
    assert mom.shape == (1, 8, h, w) and bool(torch.isfinite(mom).all())
    one = enc if kind == "sd" else new_enc()
    tiles = [one.moment_rows(img[:, :, f * y:f * (y + eh), f * x:f * (x + ew)])[0].reshape(eh, ew, 8).cpu() for y in ys for x in xs]
    ref = TR.blend32(tiles, ys, xs, TR.weights32(h, T, O, 1), TR.weights32(w, T, O, 1), 8, h, w)
    assert torch.equal(mom, one.quant(ref[None].cuda()))


def test_decoder_buffers_are_those_of_one_tile():
    cfg, sd, f, new_dec, new_enc = _vae("tiny")
    gen = torch.Generator().manual_seed(7)
    tiled, plain = new_dec(), new_dec()
    tiled.decode_tiled(torch.randn(1, 4, 20, 12, generator=gen).cuda(), tile=8, overlap=2)
    plain.decode(torch.randn(1, 4, 8, 8, generator=gen).cuda())
    a, b = buffer_shapes(tiled), buffer_shapes(plain)
    assert a == b and len(a) > 10
    full = f * 20 * f * 12
    assert not any(full in shape or 20 * 12 in shape for shape, _ in a.values())         # none has the picture's pixel or latent count for a dimension
    et, ep = new_enc(), new_enc()
    et.encode_moments_tiled(torch.zeros(1, 3, 20 * f, 12 * f, device="cuda"), tile=8, overlap=2)
    ep.encode_moments(torch.zeros(1, 3, 8 * f, 8 * f, device="cuda"))
    assert buffer_shapes(et) == buffer_shapes(ep)


# ---- render --vae-tile ----------------------------------------------------------------------------------------------------------------------------
TILE = ("--vae-tile", "8", "--vae-tile-overlap", "2")


def test_render_vae_tile_cli(ckpt_dir, tmp_path, monkeypatch):  # noqa: F811
    """A hires render (64 px -> 96 px: toy latents 16 x 16 -> 24 x 24) with 8 x 8 tiles: the picture's size, prompts.json, the decoder built once while the UNet
    is rebuilt once, and every decode at the tile's shape."""
    from PIL import Image
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd import vae as V
    builds, decoders, shapes = [], [], []
    real_build, real_init, real_rows = T.RenderStack.build_sampler, V.VaeDecoder.__init__, V.VaeDecoder.decode_rows
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n: (builds.append(n), real_build(self, n))[1])
    monkeypatch.setattr(V.VaeDecoder, "__init__", lambda self, *a, **k: (decoders.append(1), real_init(self, *a, **k))[1])
    monkeypatch.setattr(V.VaeDecoder, "decode_rows", lambda self, z: (shapes.append(tuple(z.shape)), real_rows(self, z))[1])
    tiled = _main(ckpt_dir, tmp_path / "tiled", "--hires-scale", "1.5", *TILE)
    assert Image.open(tmp_path / "tiled" / NAME).size == (96, 96)
    meta = json.load(open(tmp_path / "tiled" / "prompts.json"))
    assert meta["vae_tile"] == dict(tile=8, overlap=2) and meta["hires"]["size"] == [96, 96]
    assert builds == [1, 1] and decoders == [1]
    assert shapes == [(1, 4, 8, 8)] * len(TR.tile_starts(24, 8, 2)) ** 2 and len(shapes) == 16
    del builds[:], decoders[:], shapes[:]
    plain = _main(ckpt_dir, tmp_path / "plain", "--hires-scale", "1.5")
    assert "vae_tile" not in json.load(open(tmp_path / "plain" / "prompts.json"))
    assert builds == [1, 1] and decoders == [1, 1] and shapes == [(1, 4, 24, 24)]         # the untiled render rebuilds the decoder with the UNet, as before
    assert plain != tiled                                                                # GroupNorm statistics per tile: not the same picture


def test_render_pixel_upscaler_runs_tiled(ckpt_dir, tmp_path, monkeypatch):  # noqa: F811
    from PIL import Image
    from sd_lora_trainer_amd import ops
    calls = []
    real = ops.tile_blend
    monkeypatch.setattr(ops, "tile_blend", lambda tile, out, wy, wx, y0, x0, C: (calls.append((C, tuple(out.shape), wy.numel(), wx.numel())), real(tile, out, wy, wx, y0, x0, C))[1])
    _main(ckpt_dir, tmp_path / "pixel", "--hires-scale", "1.5", "--hires-upscaler", "pixel", *TILE)
    assert Image.open(tmp_path / "pixel" / NAME).size == (96, 96)
    # the first pass's 16 x 16 latents decoded in 3 x 3 tiles, the enlarged picture encoded in 4 x 4 pixel tiles, the final 24 x 24 latents decoded in 4 x 4
    assert calls == [(3, (3, 64, 64), 32, 32)] * 9 + [(8, (8, 24, 24), 8, 8)] * 16 + [(3, (3, 96, 96), 32, 32)] * 16
    assert json.load(open(tmp_path / "pixel" / "prompts.json"))["vae_tile"] == dict(tile=8, overlap=2)


def test_render_without_vae_tile_is_unchanged(ckpt_dir, tmp_path):  # noqa: F811
    """Without the flag the files are those of the loop render() has always run: sample, VaeDecoder.decode, JPEG - and VaeEncoder.encode_moments for an init picture."""
    import numpy as np
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import vae as V
    W = H = 64
    init = str(tmp_path / "init.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).save(init)
    plain = _main(ckpt_dir, tmp_path / "plain")
    img = _main(ckpt_dir, tmp_path / "img", "--init-image", init)
    assert sorted(json.load(open(tmp_path / "plain" / "prompts.json"))) == ["guidance_scale", "lora_scales", "prompts", "seed", "size", "steps"]
    ld = R.load_for_inference(ckpt_dir)
    stack, cfg = ld.stack, ld.models.cfg
    stack.sampler.set_lora_scale(0.85)
    emb = stack.conditioning("a photo of <concept>", 0.85, None, None)[0]
    f = 2 ** (len(stack.decoder.ups) - 1)
    h, w = H // f, W // f
    x0, _ = R.encode_init(ld, init, None, (W, H), (h, w))
    for want, kw in ((plain, {}), (img, dict(init_latents=x0, strength=0.6))):
        noise = torch.randn(1, 4, h, w, generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
        lat = stack.sampler.sample(emb, h, w, steps=6, guidance_scale=8.0, size=(H, W), latents=noise, graph=True, fused=True, n_images=1, **kw)
        dec = V.postprocess(stack.decoder.decode(lat / cfg["scaling_factor"]))[0].permute(1, 2, 0)
        path = str(tmp_path / "manual.jpg")
        Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(path, format="JPEG", quality=95)
        assert open(path, "rb").read() == want
    # an init picture encoded in tiles: another file, and the setting recorded
    tiled = _main(ckpt_dir, tmp_path / "timg", "--init-image", init, *TILE)
    assert tiled != img and json.load(open(tmp_path / "timg" / "prompts.json"))["vae_tile"] == dict(tile=8, overlap=2)
