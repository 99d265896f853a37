"""The hires pass without a GPU: the NumPy restatement of sdlt_resize_planes (tests/hires_ref.py) against torch.nn.functional.interpolate, its
identity and constant-image properties, sampler.hires_plan / upscale_latents, render()'s refusals, the CLI, the entry point's argument checks, and a
two-pass render on the emulated op table (tests/img2img_ref.emu_img plus the restated resize)."""
import ctypes as C
import json
import os
import types
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import emu_ops
from tests import hires_ref as HR
from tests import img2img_ref as IR
from tests.test_guidance_cpu import _FakeLoaded
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)

# (h, w) -> (H, W): odd sizes, differing scales per axis, a 2 x 2 and a 1 x 1 source, one downscale
CASES = [((5, 7), (9, 11)), ((8, 12), (12, 20)), ((33, 47), (83, 101)), ((2, 2), (7, 5)), ((1, 1), (4, 4)), ((16, 16), (10, 6))]
TORCH_MODE = {0: "nearest-exact", 1: "bilinear", 2: "bicubic"}
# max |got - ref| / max |ref| of hires_ref.resize against F.interpolate in fp64 over CASES x planes (4, 3), measured on the CPU with the seeds below:
# bilinear 3.42e-6, bicubic 4.29e-6 (both at (33, 47) -> (83, 101): the fp32 coordinate near 47 carries 47 * 2^-24 = 2.8e-6 into the fraction).
# The bar is four times the measured value and never above 1e-5: 1e-5 for both.
MEASURED = {1: 3.42e-6, 2: 4.29e-6}
BAR = {m: min(4 * v, 1e-5) for m, v in MEASURED.items()}


def _data(planes, h, w):
    return torch.randn(2, planes, h, w, generator=torch.Generator().manual_seed(h * 100 + w + planes))


def test_shapes_have_no_near_ties():
    """No (d + 0.5) in / out lies within 1e-3 of an integer without BEING that integer.  Where it is one (8 -> 12, 2 -> 7, 2 -> 5, 16 -> 10,
    16 -> 6 of the list: a nearest-exact index that the contract takes in integer arithmetic), the yardstick's fp32 scale in / out is rounded up, so
    its floor((d + 0.5) * scale) cannot fall below that integer either."""
    exact = set()
    for (h, w), (H, W) in CASES:
        for i, o in ((h, H), (w, W)):
            for d in range(o):
                v = Fraction(2 * d + 1, 2) * Fraction(i, o)
                dist = abs(v - round(v))
                assert dist == 0 or dist > Fraction(1, 1000), (i, o, d, float(v))
                if dist == 0:
                    exact.add((i, o))
    for i, o in exact:
        assert Fraction(float(np.float32(i) / np.float32(o))) >= Fraction(i, o), (i, o)


@pytest.mark.parametrize("planes", [4, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_restatement_against_interpolate(case, planes):
    (h, w), (H, W) = case
    x = _data(planes, h, w)
    got = HR.resize(x, H, W, 0)
    assert got.dtype == torch.float32 and torch.equal(got, F.interpolate(x, size=(H, W), mode="nearest-exact"))
    for m in (1, 2):
        got = HR.resize(x, H, W, m)
        ref = F.interpolate(x.double(), size=(H, W), mode=TORCH_MODE[m], align_corners=False)
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print(f"{TORCH_MODE[m]} {case} planes {planes}: {err:.3e}")
        assert err <= BAR[m], (TORCH_MODE[m], case, err)
    assert torch.equal(HR.resize(x, H, W, "bicubic"), HR.resize(x, H, W, 2))           # the modes by name
    assert np.array_equal(HR.resize(x.numpy(), H, W, 1), HR.resize(x, H, W, 1).numpy())


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_identity_and_constant(mode):
    x = torch.randn(3, 4, 9, 13, generator=torch.Generator().manual_seed(1))
    assert torch.equal(HR.resize(x, 9, 13, mode), x)                                    # identity: bit for bit
    rows = x.reshape(3 * 4 * 9, 1, 13)                                                  # identity on one axis: that axis adds no rounding
    assert torch.equal(HR.resize(x, 9, 20, mode), HR.resize(rows, 1, 20, mode).reshape(3, 4, 9, 20))
    assert torch.equal(HR.resize(x.transpose(2, 3).contiguous(), 20, 9, mode), HR.resize(x, 9, 20, mode).transpose(2, 3))
    for cval in (1.0, 0.1, -3.7, 1e-3, 12345.678, 0.18215, 1.9999999, 1.0000001):
        for (h, w), (H, W) in CASES:
            c = np.full((3, h, w), cval, dtype=np.float32)
            out = HR.resize(c, H, W, mode)
            ulps = float(np.abs(out.astype(np.float64) - np.float64(c[0, 0, 0])).max() / np.spacing(np.abs(c[0, 0, 0])))
            assert ulps <= 4, (mode, cval, (h, w), (H, W), ulps)


def test_hires_plan():
    assert SM.hires_plan((1024, 1024), scale=1.5) == (1536, 1536)
    assert SM.hires_plan((64, 64), scale=1.5) == (96, 96)
    assert SM.hires_plan((512, 768), scale=1.3) == (664, 1000)                          # 665.6 -> 83 * 8, 998.4 -> 125 * 8
    assert SM.hires_plan((64, 32), scale=1.1) == (72, 32)                               # one axis may stay
    assert SM.hires_plan((64, 64), target=(96, 64)) == (96, 64)
    assert SM.hires_plan((64, 64), scale=2, f=16) == (128, 128)
    for kw in (dict(), dict(scale=1.5, target=(96, 96)), dict(target=(100, 96)), dict(target=(64, 64)), dict(target=(56, 96)), dict(scale=1.0),
               dict(scale=0.5), dict(scale=1.01), dict(scale=-2.0), dict(scale="big")):
        with pytest.raises(ValueError):
            SM.hires_plan((64, 64), **kw)


def test_upscale_latents_needs_the_kernel():
    with pytest.raises(NotImplementedError, match="resize_planes"):
        SM.upscale_latents(emu_ops, torch.zeros(1, 4, 8, 8), 12, 12, "bilinear")
    with pytest.raises(ValueError, match="resample"):
        SM.upscale_latents(emu_ops, torch.zeros(1, 4, 8, 8), 12, 12, "lanczos")


def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    for kw, msg in ((dict(hires=dict(scale=1.5), init_image="x.png", mask_image="m.png"), "mask_image"),
                    (dict(hires=dict(scale=1.5, strength=0.0)), "strength"), (dict(hires=dict(scale=1.5, strength=1.5)), "strength"),
                    (dict(hires=dict(scale=1.5, strength=0.1), steps=6), "leaves no step"), (dict(hires=dict(scale=1.5, strength=0.1, steps=9)), "leaves no step"),
                    (dict(hires=dict(scale=1.5, size=(96, 96))), "either a scale or a target"), (dict(hires=dict()), "either a scale or a target"),
                    (dict(hires=dict(size=(100, 96))), "multiple of 8"), (dict(hires=dict(size=(64, 64))), "larger on one"),
                    (dict(hires=dict(scale=1.5, upscaler="esrgan")), "upscaler"), (dict(hires=dict(scale=1.5, resample="lanczos")), "resample"),
                    (dict(hires=dict(scale=1.5, factor=2)), "unknown key")):
        with pytest.raises(ValueError, match=msg):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), **kw)          # (_FakeLoaded has nothing to build with)
    assert not os.path.exists(tmp_path / "o")
    assert R.hires_args(dict(scale=1.5), (64, 64), 6) == dict(size=(96, 96), base_size=(64, 64), strength=0.6, steps=6, upscaler="latent", resample="bilinear")
    assert R.hires_args(dict(size=(128, 64), upscaler="pixel", steps=10, strength=0.3), (64, 64), 6)["resample"] == "bicubic"


def test_cli_arguments(tmp_path, capsys):
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--hires-scale", "1.5", "--hires-size", "96", "96"], "exclude each other"), (["--hires-strength", "0.5"], "need --hires-scale"),
                       (["--hires-upscaler", "pixel"], "need --hires-scale"), (["--hires-scale", "1.5", "--hires-strength", "0"], "--hires-strength"),
                       (["--hires-scale", "1.5", "--hires-upscaler", "esrgan"], "--hires-upscaler"), (["--hires-size", "96"], "--hires-size"),
                       (["--hires-scale", "1.5", "--hires-resample", "lanczos"], "--hires-resample"), (["--hires-scale", "1.5", "--hires-steps", "0"], "--hires-steps"),
                       (["--hires-scale", "1.5", "--init-image", "a.png", "--mask", "m.png"], "--mask")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert "hires" not in seen                                                           # without the flags render() is called as before
        R.main(base + ["--hires-scale", "1.5"])
        assert seen["hires"] == dict(scale=1.5)
        R.main(base + ["--hires-size", "96", "128", "--hires-strength", "0.4", "--hires-steps", "12", "--hires-upscaler", "pixel", "--hires-resample", "nearest"])
        assert seen["hires"] == dict(size=[96, 128], strength=0.4, steps=12, upscaler="pixel", resample="nearest")


def test_entry_point_validation():
    """Bad arguments: a negative code, the entry point's name in the message, nothing launched (no GPU here)."""
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_resize_planes" in _lib.SYMBOLS and C.sizeof(_lib.ResizeParams) == 48
    assert lib.sdlt_resize_planes(None, None) == -1 and b"sdlt_resize_planes" in lib.sdlt_last_error()
    ok = dict(in_=0x10000, out=0x20000, planes=12, planes_per_image=4, h=5, w=7, H=9, W=11, mode=1)
    SHAPE, ALIGN, UNSUPPORTED = -1, -2, -4
    for change, code, word in ((dict(in_=None), SHAPE, b"null"), (dict(out=None), SHAPE, b"null"), (dict(planes=0), SHAPE, b"planes=0"),
                               (dict(planes=-4), SHAPE, b"planes=-4"), (dict(planes_per_image=0), SHAPE, b"planes_per_image=0"),
                               (dict(planes=10), SHAPE, b"planes=10 planes_per_image=4"), (dict(h=0), SHAPE, b"h=0 w=7 H=9 W=11"),
                               (dict(w=-1), SHAPE, b"w=-1"), (dict(H=0), SHAPE, b"H=0"), (dict(W=0), SHAPE, b"W=0"), (dict(W=16385), SHAPE, b"W=16385"),
                               (dict(mode=3), UNSUPPORTED, b"mode=3"), (dict(mode=-1), UNSUPPORTED, b"mode=-1"),
                               (dict(planes=4 * 16, planes_per_image=1, H=16384, W=16384), SHAPE, b"output pixels"),
                               (dict(in_=0x10002), ALIGN, b"aligned"), (dict(out=0x20001), ALIGN, b"aligned"),
                               (dict(out=0x10000), SHAPE, b"aliases"), (dict(out=0x10000 + 4 * (12 * 35 - 1)), SHAPE, b"aliases"),
                               (dict(in_=0x20000 + 4 * (12 * 99 - 1)), SHAPE, b"aliases"), (dict(out=0x10000, H=5, W=7), SHAPE, b"aliases")):
        p = _lib.ResizeParams(**dict(ok, **change))
        assert lib.sdlt_resize_planes(C.byref(p), None) == code, change
        msg = lib.sdlt_last_error()
        assert b"sdlt_resize_planes" in msg and word in msg, (change, msg)


# ---- render() on the emulated op table -------------------------------------------------------------------------------------------------------
def _resize_planes(src, out, mode):
    out.copy_(HR.resize(src, out.shape[2], out.shape[3], mode))
    return out


emu_hires = types.ModuleType("emu_hires")
emu_hires.__dict__.update({k: v for k, v in vars(IR.emu_img).items() if not k.startswith("__")})
emu_hires.resize_planes = _resize_planes


def test_render_two_passes_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    config, ckdir = job
    builds = []
    real = T.RenderStack.build_sampler
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n: (builds.append(n), real(self, n))[1])
    rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_hires)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--prompt", "a house", "--lora-scale", "0.5", "--lora-scale", "0.9",
              "--size", "32", "32", "--steps", "3", "--seed", "5"]
    plain, hires = str(tmp_path / "plain"), str(tmp_path / "hires")
    R.main(common + ["--out", plain], runtime=rt())
    assert builds == [1]                                                                    # the load alone
    meta = json.load(open(os.path.join(plain, "prompts.json")))
    assert sorted(meta) == ["guidance_scale", "lora_scales", "prompts", "seed", "size", "steps"]         # the keys of a render without hires: as before
    R.main(common + ["--out", hires, "--hires-size", "48", "64", "--hires-strength", "0.7", "--hires-steps", "4"], runtime=rt())
    assert builds == [1, 1, 1]                                                              # load, and ONE rebuild for two prompts x two scales
    meta2 = json.load(open(os.path.join(hires, "prompts.json")))
    assert sorted(set(meta2) - set(meta)) == ["hires"] and meta2["size"] == [32, 32] and meta2["steps"] == 3
    assert meta2["hires"] == dict(size=[48, 64], base_size=[32, 32], strength=0.7, steps=4, upscaler="latent", resample="bilinear")
    names = sorted(f for f in os.listdir(plain) if f.endswith(".jpg"))
    assert names == sorted(f for f in os.listdir(hires) if f.endswith(".jpg")) and len(names) == 6       # the file names do not change
    for f in names:
        if not f.startswith("grid"):
            assert Image.open(os.path.join(plain, f)).size == (32, 32) and Image.open(os.path.join(hires, f)).size == (48, 64), f
    # an op table without the kernel: refused, no torch fallback
    with pytest.raises(NotImplementedError, match="resize_planes"):
        R.main(common + ["--out", str(tmp_path / "none"), "--hires-scale", "1.5"], runtime=unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=IR.emu_img))
