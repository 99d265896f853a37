"""FreeU without a GPU: the closed form of the skip filter (seven weighted sums) against the torch.fft form in fp64, the properties of the two
backbone scales, the tiny UNets on the emulated op table against the fp32 oracle with FreeU (tests/freeu_ref.py), sample()'s and render()'s argument
checks, the refusals (no kernel in the op table, backward), the CLI, the metadata, and a two-pass hires render that keeps the setting."""
import ctypes as C
import json
import os
import types

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import unet_ref as U
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd import topology
from sd_lora_trainer_amd.unet import CTX_PAD
from tests import freeu_ref as FR
from tests import img2img_ref as IR
from tests.test_guidance_cpu import _FakeLoaded
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)

SIZES = [(2, 2), (3, 5), (8, 8), (6, 16)]
FREEU = dict(b1=1.3, b2=1.4, s1=0.9, s2=0.2)


def _plane(H, W, C=6, B=2, seed=0):
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    return torch.randn(B, C, H, W, generator=g, dtype=torch.float64) + torch.rand(B, 1, H, W, generator=g, dtype=torch.float64) * 2 - 1


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_closed_form_is_the_fft_form(hw, version):
    """fp64: the seven-sum form equals fftn -> fftshift -> mask -> ifftn(.).real to 1e-12 of max |x|, for s below and above 1; and the whole op
    (either backbone version, which the filter does not touch) agrees whichever form filters the skip."""
    H, W = hw
    x = _plane(H, W)
    for s in (0.2, 0.9, 1.7):
        err = float((FR.closed_form(x, s) - FR.fourier_filter(x, s)).abs().max() / x.abs().max())
        print(f"{H}x{W} s={s}: {err:.3e}")
        assert err <= 1e-12, (hw, s, err)
    h = _plane(H, W, C=8, seed=1)
    a, b = FR.freeu_nchw(h, x, 1.4, 0.2, version), FR.freeu_nchw(h, x, 1.4, 0.2, version, filt=FR.closed_form)
    assert torch.equal(a[0], b[0]) and float((a[1] - b[1]).abs().max()) <= 1e-12 * float(x.abs().max())
    assert float((a[1] - x).abs().max()) > 1e-3                              # the filter does something


def test_size_one_is_refused():
    with pytest.raises(ValueError, match="empty"):
        FR.fourier_filter(torch.zeros(1, 1, 1, 4, dtype=torch.float64), 0.5)


@pytest.mark.parametrize("version", [1, 2])
def test_neutral_and_half_channels(version):
    h, sk = _plane(5, 6, C=8), _plane(5, 6, C=4, seed=2)
    ho, so = FR.freeu_nchw(h, sk, 1.0, 1.0, version)
    assert torch.equal(ho, h) and float((so - sk).abs().max()) <= 1e-14 * float(sk.abs().max())
    assert torch.equal(FR.closed_form(sk, 1.0), sk)
    ho, _ = FR.freeu_nchw(h, sk, 1.4, 0.2, version)
    assert torch.equal(ho[:, 4:], h[:, 4:]) and not torch.equal(ho[:, :4], h[:, :4])      # only the first half of the backbone changes
    if version == 2:                                                           # the factor runs from 1 (at the image's lowest mean) to b (at its highest)
        f = (ho[:, :4] / h[:, :4])
        assert abs(float(f.min()) - 1.0) <= 1e-12 and abs(float(f.max()) - 1.4) <= 1e-12
        flat = torch.full((1, 8, 3, 3), 0.5, dtype=torch.float64)             # hi == lo: n = 0, the library's choice
        assert torch.equal(FR.backbone(flat, 1.4, 2), flat)
    # the op on rows: neutral parameters return the bits
    hr, sr = torch.randn(2 * 30, 8), torch.randn(2 * 30, 4)
    o1, o2 = FR.freeu(hr, sr, torch.empty_like(hr), torch.empty_like(sr), None, None, B=2, H=5, W=6, b=1.0, s=1.0, version=version)
    assert torch.equal(o1, hr) and torch.equal(o2, sr)


def test_backbone_widths():
    assert FR.backbone_widths(U.CONFIGS["sdxl"]) == {"up_blocks.0.resnets.0": 1280, "up_blocks.0.resnets.1": 1280, "up_blocks.0.resnets.2": 1280,
                                                    "up_blocks.1.resnets.0": 1280, "up_blocks.1.resnets.1": 640, "up_blocks.1.resnets.2": 640}
    assert FR.backbone_widths(U.CONFIGS["tiny15"]) == {"up_blocks.0.resnets.0": 128, "up_blocks.0.resnets.1": 128,
                                                      "up_blocks.1.resnets.0": 128, "up_blocks.1.resnets.1": 128}


# ---- the UNet on the emulated op table ------------------------------------------------------------------------------------------------------
def _forward_case(version, h=8, B=2, rank=4):
    cfg = U.CONFIGS[version]
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, h, h, generator=g)
    t = torch.tensor([10, 900][:B])
    ctx = torch.randn(B, 77, cfg["cross_dim"], generator=g)
    pooled = tid = add = None
    if cfg["addition"]:
        pooled = torch.randn(B, cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"], generator=g)
        tid = torch.tensor([[1024., 1024, 0, 0, 128, 128]] * B)
        add = {"text_embeds": pooled, "time_ids": tid}
    rt = unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=FR.emu_freeu)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)

    def run():
        x64 = rt.zeros(B * h * h, 64)
        x64[:, :4] = x.permute(0, 2, 3, 1).reshape(B * h * h, 4)
        cb = rt.zeros(B * CTX_PAD, cfg["cross_dim"])
        cb.view(B, CTX_PAD, -1)[:, :77] = ctx
        out = unet.forward(x64, t.float(), cb, pooled, None if tid is None else tid.flatten(), B=B, H=h, W=h)
        return out.reshape(B, h, h, 4).permute(0, 3, 1, 2).clone()

    oracle = lambda fz: FR.unet_forward_freeu(cfg, sd, x, t, ctx, add, lora, freeu=fz)  # noqa: E731
    return unet, run, oracle


@pytest.mark.parametrize("fver", [1, 2])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_with_freeu_matches_the_oracle(version, fver):
    """The tolerance of tests/test_engine_cpu.py's forward parity (rtol 1e-3, atol 1e-4) at an 8 x 8 latent: up_blocks.0 runs at 2 x 2, up_blocks.1 at 4 x 4."""
    unet, run, oracle = _forward_case(version)
    plain = run()
    torch.testing.assert_close(plain, oracle(None), rtol=1e-3, atol=1e-4)
    fz = dict(FREEU, version=fver)
    unet.set_freeu(fz)
    got = run()
    torch.testing.assert_close(got, oracle(fz), rtol=1e-3, atol=1e-4)
    assert float((got - plain).abs().max()) > 1e-2                            # FreeU moves the prediction far beyond the tolerance
    unet.set_freeu(dict(b1=1, b2=1, s1=1, s2=1, version=fver))
    assert torch.equal(run(), plain)                                          # neutral: the same bits
    unet.set_freeu(None)
    assert torch.equal(run(), plain)


def test_set_freeu_refusals():
    unet, run, _ = _forward_case("tiny15")
    for bad in (dict(b1=1.2, b2=1.4, s1=0.9), dict(FREEU, version=3), dict(FREEU, b1=0.0), dict(FREEU, s2=float("nan")), dict(FREEU, gain=2.0)):
        with pytest.raises((ValueError, KeyError), match="freeu|b1|s2"):
            unet.set_freeu(bad)
    unet.set_freeu(FREEU)
    with pytest.raises(RuntimeError, match="freeu"):                           # inference only
        unet.backward(None, None)
    unet.set_freeu(None)
    # an op table without the kernel: refused by name, no torch fallback
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=IR.emu_img)
    plain = unet_mod.UNet(rt, topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)
    with pytest.raises(NotImplementedError, match="freeu"):
        plain.set_freeu(FREEU)
    smp = SM.LatentSampler(rt, plain)
    e = (torch.zeros(1, 77, 64), torch.zeros(1, 77, 64))
    with pytest.raises(NotImplementedError, match="freeu"):
        smp.sample(e, 8, 8, steps=1, freeu=(1.3, 1.4, 0.9, 0.2))
    # a latent too small for the filter: up_blocks.0 of a 4 x 4 latent runs at 1 x 1
    unet4, run4, _ = _forward_case("tiny15", h=4)
    unet4.set_freeu(FREEU)
    with pytest.raises(ValueError, match="freeu"):
        run4()


def test_sample_arguments():
    assert SM.freeu_args(None) is None
    assert SM.freeu_args((1.3, 1.4, 0.9, 0.2)) == dict(FREEU, version=1) == SM.freeu_args([1.3, 1.4, 0.9, 0.2])
    assert SM.freeu_args(dict(FREEU, version=2)) == dict(FREEU, version=2)
    for bad in ((1.3, 1.4, 0.9), (1.3, 1.4, 0.9, 0.2, 1.0), (1.3, 1.4, 0.9, -0.2), (1.3, 1.4, 0.0, 0.2), (1.3, float("inf"), 0.9, 0.2),
                (1.3, float("nan"), 0.9, 0.2), ("a", 1, 1, 1), (True, 1, 1, 1), 1.3, dict(FREEU, version=0), dict(FREEU, version=3), dict(FREEU, version=True),
                dict(b1=1.3, b2=1.4, s1=0.9), dict(FREEU, s3=1.0)):
        with pytest.raises(ValueError, match="freeu"):
            SM.freeu_args(bad)
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=FR.emu_freeu)
    unet = unet_mod.UNet(rt, topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)
    smp = SM.LatentSampler(rt, unet)
    e = (torch.zeros(1, 77, 64), torch.zeros(1, 77, 64))
    with pytest.raises(ValueError, match="freeu"):
        smp.sample(e, 8, 8, steps=1, freeu=(1.3, 1.4, 0.9))


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths_agree_and_follow_the_oracle(version):
    """Torch loop and fused loop on the emulated table, 3 steps at 8 x 8: the same launches, so the same latents; neutral FreeU is no FreeU, bit for
    bit; a real setting moves the latents and follows the oracle loop with FreeU closer than it follows the plain one."""
    cfg = U.CONFIGS[version]
    sd, lora = U.init_unet_state(cfg, seed=0), U.init_lora(cfg, 4, seed=1, b_std=0.05)
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    embeds = (mk(1, 77, cfg["cross_dim"]), mk(1, 77, cfg["cross_dim"])) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None))
    noise = mk(1, 4, 8, 8)
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=FR.emu_freeu)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=4)
    unet.arena.load(lora)
    smp = SM.LatentSampler(rt, unet)
    kw = dict(steps=3, guidance_scale=8.0, latents=noise)
    plain = smp.sample(embeds, 8, 8, **kw)
    assert torch.equal(smp.sample(embeds, 8, 8, freeu=(1, 1, 1, 1), **kw), plain)
    fz = (1.3, 1.4, 0.9, 0.2)
    loop = smp.sample(embeds, 8, 8, freeu=fz, **kw)
    fused = smp.sample(embeds, 8, 8, freeu=fz, fused=True, **kw)
    assert float((loop - fused).abs().max()) <= 1e-4 * float(loop.abs().max())
    assert torch.equal(smp.sample(embeds, 8, 8, **kw), plain) and unet._freeu is None          # freeu=None afterwards: the setting does not stick
    ref, ref_plain = FR.sample_latents_freeu(cfg, sd, lora, 1.0, embeds, noise, 3, freeu=fz), FR.sample_latents_freeu(cfg, sd, lora, 1.0, embeds, noise, 3, freeu=None)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    print(f"{version}: freeu vs oracle+freeu {rel(loop, ref):.3e}; plain vs oracle {rel(plain, ref_plain):.3e}; freeu vs plain {rel(loop, plain):.3e}")
    assert rel(loop, ref) <= 1e-3 and rel(plain, ref_plain) <= 1e-3 and rel(loop, plain) > 1e-2


# ---- render() and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    for bad in ((1.3, 1.4, 0.9), (1.3, 1.4, 0.9, -1.0), dict(FREEU, version=4)):
        with pytest.raises(ValueError, match="freeu"):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), freeu=bad)
    assert not os.path.exists(tmp_path / "o")


def test_cli_arguments(tmp_path, capsys):
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--freeu", "1.3", "1.4", "0.9"], "--freeu"), (["--freeu-v2"], "--freeu-v2 needs --freeu"), (["--freeu", "1.3", "1.4", "0.9", "0"], "positive"),
                       (["--freeu", "1.3", "1.4", "0.9", "-0.2"], "positive"), (["--freeu", "1.3", "nan", "0.9", "0.2"], "positive"), (["--freeu", "a", "b", "c", "d"], "--freeu")):
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
        assert "freeu" not in seen                                              # without the flag render() is called as before
        R.main(base + ["--freeu", "1.3", "1.4", "0.9", "0.2"])
        assert seen["freeu"] == dict(FREEU, version=1)
        R.main(base + ["--freeu", "1.5", "1.6", "0.9", "0.2", "--freeu-v2"])
        assert seen["freeu"] == dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, version=2)


def test_render_metadata_and_hires_keep_the_setting(job, tmp_path):  # noqa: F811
    """prompts.json records the setting; both passes of a hires render run the op (first pass 8 x 8 latent: 2 x 2 and 4 x 4 planes; second pass
    12 x 12: 3 x 3 and 6 x 6), on the UNet that render() rebuilds between them."""
    from sd_lora_trainer_amd import render as R
    from tests.test_hires_cpu import _resize_planes
    config, ckdir = job
    calls = []

    def spy(h, skip, h_out, skip_out, tabs, ws, **kw):
        calls.append((kw["H"], kw["W"], kw["b"], kw["s"], kw["version"]))
        return FR.freeu(h, skip, h_out, skip_out, tabs, ws, **kw)

    table = types.ModuleType("emu_freeu_hires")
    table.__dict__.update({k: v for k, v in vars(FR.emu_freeu).items() if not k.startswith("__")})
    table.resize_planes, table.freeu = _resize_planes, spy
    rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", "32", "32", "--steps", "2", "--seed", "5"]
    R.main(common + ["--out", str(tmp_path / "plain")], runtime=rt())
    assert not calls and "freeu" not in json.load(open(tmp_path / "plain" / "prompts.json"))
    R.main(common + ["--out", str(tmp_path / "fu"), "--freeu", "1.3", "1.4", "0.9", "0.2", "--freeu-v2"], runtime=rt())
    assert json.load(open(tmp_path / "fu" / "prompts.json"))["freeu"] == dict(FREEU, version=2)
    assert {c[:2] for c in calls} == {(2, 2), (4, 4)} and len(calls) == 2 * 4             # 2 steps x (2 + 2 resnets)
    assert {c[2:] for c in calls} == {(1.3, 0.9, 2), (1.4, 0.2, 2)}
    name = next(f for f in sorted(os.listdir(tmp_path / "plain")) if f.startswith("img_00"))
    assert open(tmp_path / "fu" / name, "rb").read() != open(tmp_path / "plain" / name, "rb").read()
    calls.clear()
    R.main(common + ["--out", str(tmp_path / "hi"), "--freeu", "1.3", "1.4", "0.9", "0.2", "--hires-size", "48", "48", "--hires-strength", "0.5"], runtime=rt())
    meta = json.load(open(tmp_path / "hi" / "prompts.json"))
    assert meta["freeu"] == dict(FREEU, version=1) and meta["hires"]["size"] == [48, 48]
    assert {c[:2] for c in calls} == {(2, 2), (4, 4), (3, 3), (6, 6)}                     # the second pass, on the rebuilt UNet, has it too
    assert [c[:2] for c in calls].index((3, 3)) == 2 * 4                                  # ... after the whole first pass


def test_entry_point_validation():
    """Contract violations: a negative code, the entry point's name in the message, nothing launched (no GPU here)."""
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_freeu" in _lib.SYMBOLS and "sdlt_freeu_ws_floats" in _lib.SYMBOLS
    assert lib.sdlt_freeu_ws_floats(2, 8, 8, 128, 64) == 2 * 2 * 7 * 64 + 2 * 64 + 2 * 2 * 2          # 64 rows: two chunks of 32
    assert lib.sdlt_freeu_ws_floats(2, 2, 2, 8, 8) == 2 * 1 * 7 * 8 + 2 * 4 + 2 * 1 * 2
    assert lib.sdlt_freeu_ws_floats(1, 64, 64, 64, 72) == 16 * 7 * 72 + 4096 + 16 * 2
    assert lib.sdlt_freeu_ws_floats(1, 1, 8, 64, 64) == -1 and b"sdlt_freeu" in lib.sdlt_last_error()
    ok = dict(h=0x100000, ld_h=16, skip=0x200000, ld_s=24, h_out=0x300000, ld_ho=16, skip_out=0x400000, ld_so=24, B=2, H=3, W=5, C1=16, C2=24,
              b=1.4, s=0.2, version=1, ty=0x500000, tx=0x500100, ws=0x600000, ws_floats=1 << 20)
    order = ("h", "ld_h", "skip", "ld_s", "h_out", "ld_ho", "skip_out", "ld_so", "B", "H", "W", "C1", "C2", "b", "s", "version", "ty", "tx", "ws", "ws_floats")
    SHAPE, ALIGN, UNSUPPORTED = -1, -2, -4
    for change, code, word in ((dict(h=None), SHAPE, b"null"), (dict(skip_out=None), SHAPE, b"null"), (dict(ty=None), SHAPE, b"null"), (dict(ws=None), SHAPE, b"null"),
                               (dict(B=0), SHAPE, b"B=0"), (dict(H=1), SHAPE, b"H=1"), (dict(W=1), SHAPE, b"W=1"), (dict(W=0), SHAPE, b"W=0"),
                               (dict(C1=12, ld_h=16), SHAPE, b"C1=12"), (dict(C1=7), SHAPE, b"C1=7"), (dict(C2=20), SHAPE, b"C2=20"), (dict(C2=0), SHAPE, b"C2=0"),
                               (dict(ld_h=8), SHAPE, b"leading"), (dict(ld_so=16), SHAPE, b"leading"),
                               (dict(version=0), UNSUPPORTED, b"version=0"), (dict(version=3), UNSUPPORTED, b"version=3"),
                               (dict(h=0x100008), ALIGN, b"aligned"), (dict(skip_out=0x400002), ALIGN, b"aligned"), (dict(ld_s=28), ALIGN, b"aligned"),
                               (dict(ws=0x600002), ALIGN, b"aligned"), (dict(tx=0x500101), ALIGN, b"aligned"),
                               (dict(h_out=0x100000), SHAPE, b"overlaps"), (dict(skip_out=0x200000), SHAPE, b"overlaps"), (dict(h_out=0x200000), SHAPE, b"overlaps"),
                               (dict(skip_out=0x300000), SHAPE, b"overlaps"), (dict(h_out=0x100000 + 2 * (29 * 16 + 8)), SHAPE, b"overlaps"),
                               (dict(ws_floats=100), SHAPE, b"workspace")):
        a = dict(ok, **change)
        assert lib.sdlt_freeu(*[a[k] for k in order], None) == code, change
        msg = lib.sdlt_last_error()
        assert b"sdlt_freeu" in msg and word in msg, (change, msg)
