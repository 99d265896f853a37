"""Tiled VAE decode / encode without a GPU: the tile geometry and the normalised feather weights of vae.py against their independent restatement
(tests/vaetile_ref.py), the refusals, decode_tiled / encode_moments_tiled on the emulated op table against the composition made by hand, the entry
point's argument checks, and render()'s `vae_tile` / the CLI's --vae-tile."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import vae_ref as V
from sd_lora_trainer_amd import vae
from tests import emu_ops
from tests import vaetile_ref as TR
from tests.test_guidance_cpu import _FakeLoaded
from tests.test_hires_cpu import emu_hires
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)

GEOMETRIES = [(8, 2), (8, 0), (8, 4), (64, 16), (5, 1)]


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,O", GEOMETRIES)
def test_tile_starts(T, O):
    for L in range(1, 201):
        s = vae.tile_starts(L, T, O)
        assert s == TR.tile_starts(L, T, O), (L, T, O)
        E = min(L, T)
        assert s[0] == 0 and s[-1] + E == L
        assert (len(s) == 1) == (L <= T)
        assert all(b > a for a, b in zip(s, s[1:]))
        assert all(a + E - b >= O for a, b in zip(s, s[1:])), (L, T, O, s)               # neighbours overlap by at least O (and so leave no gap)


@pytest.mark.parametrize("g", [1, 8])
@pytest.mark.parametrize("T,O", GEOMETRIES)
def test_tile_weights(T, O, g):
    for L in list(range(1, 40)) + [63, 64, 65, 100, 127, 128, 129, 200]:
        ref = TR.tile_weights(L, T, O, g)
        got = vae.tile_weights(L, T, O, g)
        s = TR.tile_starts(L, T, O)
        E = g * min(L, T)
        total = np.zeros(g * L)
        assert len(got) == len(ref) == len(s)
        for k, (r, w) in enumerate(zip(ref, got)):
            r = np.asarray(r, dtype=np.float64)
            assert r.shape == (E,) and bool((r > 0).all()) and bool((r <= 1).all())
            total[g * s[k]: g * s[k] + E] += r
            assert w.dtype == torch.float32 and w.device.type == "cpu" and np.array_equal(w.numpy(), r.astype(np.float32)), (L, T, O, g, k)
            assert bool((w > 0).all())
        assert float(np.abs(total - 1.0).max()) <= 1e-12, (L, T, O, g)


def test_weights_shape_of_the_feather():
    """First and last tile keep weight 1 to the picture's edge; in a two-tile overlap the pair crosses at one half; overlap 0 is a hard seam."""
    w = TR.tile_weights(14, 8, 2, 1)                       # starts 0, 6: overlap exactly 2
    assert TR.tile_starts(14, 8, 2) == [0, 6]
    assert w[0][:6] == [1.0] * 6 and w[1][2:] == [1.0] * 6
    assert w[0][6] == pytest.approx(0.75) and w[0][7] == pytest.approx(0.25) and w[1][0] == pytest.approx(0.25) and w[1][1] == pytest.approx(0.75)
    for row in TR.tile_weights(16, 8, 0, 1):
        assert row == [1.0] * 8


@pytest.mark.parametrize("T,O", [(8, 5), (1, 0), (0, 0), (8, -1), (64, 33)])
def test_bad_geometry(T, O):
    with pytest.raises(ValueError, match="tile"):
        vae.tile_starts(20, T, O)
    with pytest.raises(ValueError, match="tile"):
        vae.tile_weights(20, T, O, 8)


# ---- the reference composition itself -----------------------------------------------------------------------------------------------------------
def _layout(H, W, T, O, g, C, ld, seed):
    """Random tiles of a g-times-upsampled H x W latent grid -> (tiles [th, tw, ld], ys, xs, wys, wxs)."""
    ys, xs = [g * s for s in TR.tile_starts(H, T, O)], [g * s for s in TR.tile_starts(W, T, O)]
    wys, wxs = TR.weights32(H, T, O, g), TR.weights32(W, T, O, g)
    gen = torch.Generator().manual_seed(seed)
    tiles = [torch.randn(g * min(H, T), g * min(W, T), ld, generator=gen) for _ in range(len(ys) * len(xs))]
    return tiles, ys, xs, wys, wxs


def test_blend32_against_blend_and_constant():
    H, W, T, O, g, C = 20, 13, 8, 2, 2, 3
    tiles, ys, xs, wys, wxs = _layout(H, W, T, O, g, C, 4, 0)
    a32 = TR.blend32(tiles, ys, xs, wys, wxs, C, g * H, g * W)
    a64 = TR.blend(tiles, ys, xs, wys, wxs, C, g * H, g * W)
    bound = 4 * 2.0 ** -23 * TR.blend(tiles, ys, xs, wys, wxs, C, g * H, g * W, absolute=True)
    assert bool(((a32.double() - a64).abs() <= bound).all())
    const = [torch.full_like(t, 1.75) for t in tiles]
    c32 = TR.blend32(const, ys, xs, wys, wxs, C, g * H, g * W)
    assert float((c32 - 1.75).abs().max()) <= 2 * 2.0 ** -23                              # 2 ulp of 1.75: the weights sum to 1 at every sample, corners included


# ---- decode_tiled / encode_moments_tiled on the emulated table ------------------------------------------------------------------------------------
def _tile_blend(tile, out, wy, wx, y0, x0, C):
    th, tw = wy.numel(), wx.numel()
    assert tile.dtype == out.dtype == wy.dtype == wx.dtype == torch.float32 and tuple(tile.shape[:1]) == (th * tw,) and out.shape[0] == C <= tile.shape[1]
    TR.blend32([tile.reshape(th, tw, -1)], [y0], [x0], [wy], [wx], C, out.shape[1], out.shape[2], out=out)
    return out


emu_tile = types.ModuleType("emu_tile")
emu_tile.__dict__.update({k: v for k, v in vars(emu_hires).items() if not k.startswith("__")})
emu_tile.tile_blend = _tile_blend


def _vae(ops, kind="tiny"):
    cfg = V.CONFIGS[kind]
    sd = V.init_state(cfg, seed=0)
    rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=ops)  # noqa: E731
    return cfg, vae.VaeDecoder(rt(), sd), vae.VaeEncoder(rt(), sd), (lambda: vae.VaeDecoder(rt(), sd)), (lambda: vae.VaeEncoder(rt(), sd))


def _modules(v):
    if isinstance(v, unet_mod._Module):
        yield v
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from _modules(x)


def buffer_shapes(mod, seen=None):
    """{module name:key: (shape, dtype)} of every persistent buffer of a plan (unet._Module.buf), through its sub-modules."""
    seen = {} if seen is None else seen
    for key, t in mod._b.items():
        seen[f"{mod.name}:{key}"] = (tuple(t.shape), t.dtype)
    for v in vars(mod).values():
        for m in _modules(v):
            buffer_shapes(m, seen)
    return seen


@pytest.mark.parametrize("h,w,T,O", [(20, 12, 8, 2), (8, 24, 8, 2), (9, 9, 8, 4)])
def test_tiled_passes_on_the_emulated_table(h, w, T, O):
    cfg, dec, enc, new_dec, new_enc = _vae(emu_tile)
    f = 2 ** (len(cfg["block_out_channels"]) - 1)
    gen = torch.Generator().manual_seed(h * 100 + w)
    z = torch.randn(2, 4, h, w, generator=gen)
    ys, xs = TR.tile_starts(h, T, O), TR.tile_starts(w, T, O)
    eh, ew = min(h, T), min(w, T)
    got = dec.decode_tiled(z, tile=T, overlap=O)
    assert got.shape == (2, 3, f * h, f * w) and got.dtype == torch.float32
    one = new_dec()
    for b in range(2):
        tiles = [TR.nhwc(one.decode(z[b:b + 1, :, y:y + eh, x:x + ew])) for y in ys for x in xs]
        ref = TR.blend32(tiles, [f * y for y in ys], [f * x for x in xs], TR.weights32(h, T, O, f), TR.weights32(w, T, O, f), 3, f * h, f * w)
        assert torch.equal(got[b], ref)
    assert buffer_shapes(dec) == buffer_shapes(one)                                     # one tile-shaped buffer set, none keyed by the picture
    img = torch.tanh(torch.randn(2, 3, f * h, f * w, generator=gen))
    mom = enc.encode_moments_tiled(img, tile=T, overlap=O)
    assert mom.shape == (2, 8, h, w)
    one = new_enc()
    for b in range(2):
        tiles = [one.moment_rows(img[b:b + 1, :, f * y:f * (y + eh), f * x:f * (x + ew)])[0].reshape(eh, ew, 8).clone() for y in ys for x in xs]
        ref = TR.blend32(tiles, ys, xs, TR.weights32(h, T, O, 1), TR.weights32(w, T, O, 1), 8, h, w)
        assert torch.equal(mom[b], one.quant(ref[None])[0])
        # quant_conv is linear and the weights sum to 1: applying it per tile gives the same moments up to rounding
        per_tile = [TR.nhwc(one.encode_moments(img[b:b + 1, :, f * y:f * (y + eh), f * x:f * (x + ew)])) for y in ys for x in xs]
        lin = TR.blend(per_tile, ys, xs, TR.weights32(h, T, O, 1), TR.weights32(w, T, O, 1), 8, h, w)
        torch.testing.assert_close(mom[b].double(), lin, rtol=1e-4, atol=1e-5 * float(lin.abs().max()))
    assert buffer_shapes(enc) == buffer_shapes(one)


def test_single_tile_is_the_plain_pass():
    cfg, dec, enc, new_dec, new_enc = _vae(emu_ops)                                      # (no tile_blend needed: nothing is blended)
    z = torch.randn(1, 4, 8, 6, generator=torch.Generator().manual_seed(2))
    assert torch.equal(dec.decode_tiled(z, tile=8, overlap=2), new_dec().decode(z))
    img = torch.tanh(torch.randn(1, 3, 32, 24, generator=torch.Generator().manual_seed(3)))
    assert torch.equal(enc.encode_moments_tiled(img, tile=8, overlap=2), new_enc().encode_moments(img))


def test_tiling_needs_the_kernel():
    cfg, dec, enc, _, _ = _vae(emu_ops)
    with pytest.raises(NotImplementedError, match="tile_blend"):
        dec.decode_tiled(torch.zeros(1, 4, 12, 8), tile=8, overlap=2)
    with pytest.raises(NotImplementedError, match="sdlt_tile_blend"):
        enc.encode_moments_tiled(torch.zeros(1, 3, 32, 48), tile=8, overlap=2)
    with pytest.raises(ValueError, match="overlap"):
        dec.decode_tiled(torch.zeros(1, 4, 12, 8), tile=8, overlap=5)
    with pytest.raises(ValueError, match="multiple of 4"):
        enc.encode_moments_tiled(torch.zeros(1, 3, 34, 48), tile=8, overlap=2)


# ---- the entry point's checks (nothing is launched: no GPU here) ------------------------------------------------------------------------------------
REFUSALS = ((dict(tile=None), -1, b"null"), (dict(out=None), -1, b"null"), (dict(wy=None), -1, b"null"), (dict(wx=None), -1, b"null"),
            (dict(th=0), -1, b"th=0"), (dict(tw=-3), -1, b"tw=-3"), (dict(C=0), -1, b"C=0"), (dict(H=0), -1, b"H=0"), (dict(W=-1), -1, b"W=-1"),
            (dict(C=17, ld=20), -1, b"C=17"), (dict(C=4, ld=3), -1, b"ld=3"), (dict(y0=6), -1, b"outside"), (dict(x0=5), -1, b"outside"),
            (dict(y0=-1), -1, b"outside"), (dict(x0=-1), -1, b"outside"), (dict(th=11), -1, b"outside"), (dict(tw=2 ** 31 - 1, x0=4), -1, b"outside"),
            (dict(tile=0x10002), -2, b"aligned"), (dict(out=0x20001), -2, b"aligned"), (dict(out=0x10000), -1, b"overlaps"),
            (dict(out=0x10000 + 4 * (5 * 7 * 4 - 1)), -1, b"overlaps"), (dict(tile=0x20000 + 4 * (3 * 10 * 11 - 1)), -1, b"overlaps"))


def lib_tile_blend(lib, **kw):
    a = dict(dict(tile=0x10000, ld=4, th=5, tw=7, C=3, wy=0x30000, wx=0x40000, out=0x20000, H=10, W=11, y0=5, x0=4), **kw)
    return lib.sdlt_tile_blend(a["tile"], a["ld"], a["th"], a["tw"], a["C"], a["wy"], a["wx"], a["out"], a["H"], a["W"], a["y0"], a["x0"], None)


def test_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_tile_blend" in _lib.SYMBOLS
    for change, code, word in REFUSALS:
        assert lib_tile_blend(lib, **change) == code, change
        msg = lib.sdlt_last_error()
        assert b"sdlt_tile_blend" in msg and word in msg, (change, msg)


# ---- render() and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    for bad in ((32, 20), 1, (8, -1), (0, 0), "64", (64,), (64.0, 16), True):
        with pytest.raises(ValueError, match="tile"):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), vae_tile=bad)
    assert not os.path.exists(tmp_path / "o")
    assert R.vae_tile_args(None) is None and R.vae_tile_args(64) == (64, 16) and R.vae_tile_args((8, 2)) == (8, 2) and R.vae_tile_args([32, 0]) == (32, 0)


def test_cli_arguments(tmp_path, capsys):
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--vae-tile", "32", "--vae-tile-overlap", "20"], "overlap"), (["--vae-tile-overlap", "8"], "needs --vae-tile"),
                       (["--vae-tile", "1", "--vae-tile-overlap", "0"], "tile"), (["--vae-tile", "8"], "overlap"), (["--vae-tile", "8.5"], "--vae-tile"),
                       (["--vae-tile", "64", "--vae-tile-overlap", "-1"], "overlap")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)                                                          # (the checkpoint does not exist: refused before anything is loaded)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert "vae_tile" not in seen                                                     # without the flag render() is called as before
        R.main(base + ["--vae-tile"])
        assert seen["vae_tile"] == (64, 16)
        R.main(base + ["--vae-tile", "--prompt", "a house"])
        assert seen["vae_tile"] == (64, 16)
        R.main(base + ["--vae-tile", "32"])
        assert seen["vae_tile"] == (32, 16)
        R.main(base + ["--vae-tile", "48", "--vae-tile-overlap", "24"])
        assert seen["vae_tile"] == (48, 24)


def test_render_tiled_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    """--vae-tile on a hires render with the pixel upscaler: tiled decodes and encodes at ONE tile shape, the decoder built once (the hires pass rebuilds the
    UNet alone), prompts.json carries the setting only when it is set, and an op table without the kernel is refused."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    config, ckdir = job
    builds, decoders, dshapes, eshapes = [], [], [], []
    real_build, real_init = T.RenderStack.build_sampler, vae.VaeDecoder.__init__
    real_rows, real_mrows = vae.VaeDecoder.decode_rows, vae.VaeEncoder.moment_rows
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n: (builds.append(n), real_build(self, n))[1])
    monkeypatch.setattr(vae.VaeDecoder, "__init__", lambda self, *a, **k: (decoders.append(1), real_init(self, *a, **k))[1])
    monkeypatch.setattr(vae.VaeDecoder, "decode_rows", lambda self, z: (dshapes.append(tuple(z.shape[2:])), real_rows(self, z))[1])
    monkeypatch.setattr(vae.VaeEncoder, "moment_rows", lambda self, x: (eshapes.append(tuple(x.shape[2:])), real_mrows(self, x))[1])
    rt = lambda ops=emu_tile: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=ops)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", "32", "32", "--steps", "2", "--seed", "5"]
    hires = ["--hires-size", "48", "64", "--hires-strength", "0.5", "--hires-upscaler", "pixel"]
    R.main(common + ["--out", str(tmp_path / "plain")], runtime=rt())
    meta = json.load(open(tmp_path / "plain" / "prompts.json"))
    assert "vae_tile" not in meta and (builds, decoders, dshapes) == ([1], [1], [(8, 8)])
    del builds[:], decoders[:], dshapes[:]
    R.main(common + hires + ["--out", str(tmp_path / "tiled"), "--vae-tile", "8", "--vae-tile-overlap", "2"], runtime=rt())
    meta = json.load(open(tmp_path / "tiled" / "prompts.json"))
    assert meta["vae_tile"] == dict(tile=8, overlap=2) and meta["hires"]["size"] == [48, 64]
    assert builds == [1, 1] and decoders == [1]                                           # the UNet's one rebuild; the decoder is the load's
    # first pass 8 x 8 (one tile: the plain decode), enlarged and encoded in 3 x 2 pixel tiles of 32 px, the final 16 x 12 latent decoded in 3 x 2 tiles
    nt = len(TR.tile_starts(16, 8, 2)) * len(TR.tile_starts(12, 8, 2))
    assert nt == 6 and dshapes == [(8, 8)] + [(8, 8)] * nt and eshapes == [(32, 32)] * nt
    name = next(f for f in sorted(os.listdir(tmp_path / "tiled")) if f.startswith("img_00"))
    assert Image.open(tmp_path / "tiled" / name).size == (48, 64)
    with pytest.raises(NotImplementedError, match="tile_blend"):
        R.main(common + ["--out", str(tmp_path / "none"), "--vae-tile", "8", "--vae-tile-overlap", "2"], runtime=rt(emu_hires))
    assert not os.path.exists(tmp_path / "none")
