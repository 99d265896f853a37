"""Differential diffusion without a GPU: sampler.hold_map and ops.blur_taps against known answers, LatentSampler.sample(change_map=) on the torch loop
(and the fused path on the emulated op table of tests/diffdiff_ref.py) - the exact invariants, the refusals - the command line, and a render whose
change map is all black."""
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd.config import TrainingConfig
from tests import blur_ref as BR
from tests import diffdiff_ref as DR
from tests import img2img_ref as IR
from tests.test_driver_cpu import _run, _tokenizer_dir
from tests.test_img2img_cpu import EMB, _Stub, _case


# ---- the hold map ------------------------------------------------------------------------------------------------------------------------
def test_hold_map_known_answers():
    c = torch.tensor([0.0, 0.01, 0.5, 0.9, 1.0])
    got = SM.hold_map(c, 10)
    assert got.dtype == torch.float32 and got.tolist() == [11.0, 10.0, 5.0, 1.0, 0.0]
    assert np.array_equal(DR.hold_rule(c.numpy(), 10), got.double().numpy())
    assert SM.hold_map(torch.tensor([[0.0, 1e-30, 1.0]]), 1).tolist() == [[2.0, 1.0, 0.0]]            # c > 0 always runs the last step free
    assert SM.hold_map(torch.tensor([0.3, 0.7, 0.25]), 10).tolist() == [7.0, 3.0, 8.0]                # i / k whichever way fp32 rounded c; 7.5 -> 8


@pytest.mark.parametrize("k", [1, 6, 15, 1000])
def test_hold_map_monotone_and_bounded(k):
    c = torch.cat([torch.linspace(0, 1, 4097), torch.rand(1000, generator=torch.Generator().manual_seed(k))]).sort().values
    hold = SM.hold_map(c, k)
    assert bool((hold[1:] <= hold[:-1]).all())                                                         # non-increasing in c
    assert bool((hold == hold.round()).all()) and float(hold.min()) == 0.0 and float(hold.max()) == k + 1
    assert bool((hold[c > 0] <= k).all()) and bool((hold[c == 0] == k + 1).all()) and bool((hold[c == 1] == 0).all())
    assert np.array_equal(DR.hold_rule(c.numpy(), k), hold.double().numpy())


def test_hold_map_refusals():
    for bad in ([0.5, 1.5], [-0.1, 0.5], [0.5, float("nan")], [float("inf")], [-float("inf"), 0.0]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            SM.hold_map(torch.tensor(bad), 10)
    with pytest.raises(ValueError, match="fp32"):
        SM.hold_map(torch.tensor([0.5], dtype=torch.float64), 10)
    for bad_k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="step count"):
            SM.hold_map(torch.tensor([0.5]), bad_k)


# ---- the taps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.3, 0.5, 1.5, 2.0, 8.0, 21.0, 21.5, 100.0])
def test_blur_taps(sigma):
    taps = ops.blur_taps(sigma)
    R = min(int(np.ceil(3.0 * sigma)), 64)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (2 * R + 1,) and R <= 64
    assert torch.equal(taps, taps.flip(0)) and float(taps[R]) == float(taps.max()) and float(taps.min()) > 0.0
    # each weight is rounded once, by at most half an ulp of a value below 1 (2^-25): 2 R + 1 of them around an fp64 sum of 1
    assert abs(float(taps.double().sum()) - 1.0) <= (2 * R + 1) * 2.0 ** -25
    R64, w64 = BR.taps64(sigma)
    assert R64 == R and np.array_equal(w64.astype(np.float32), taps.numpy())


def test_blur_taps_refusals():
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="sigma"):
            ops.blur_taps(bad)


def test_blur_map_host_cases():
    m = torch.rand(1, 1, 5, 7, generator=torch.Generator().manual_seed(0))
    assert SM.blur_map(object(), m, 0.0) is m                                                          # sigma 0: no launch, whatever the op table
    with pytest.raises(NotImplementedError, match="blur_planes"):
        SM.blur_map(IR.emu_img, m, 1.0)
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="mask_blur"):
            SM.blur_map(DR.emu_dd, m, bad)
    out = SM.blur_map(DR.emu_dd, m, 2.0)
    assert out.shape == m.shape and float(out.min()) >= 0.0 and float(out.max()) <= 1.0 and not torch.equal(out, m)
    one = SM.blur_map(DR.emu_dd, torch.ones(1, 1, 5, 7), 8.0)                                          # the radius beyond the extent; rounded weights: clamped
    assert float(one.max()) <= 1.0 and float((one - 1).abs().max()) < 1e-5


# ---- LatentSampler.sample(change_map=) ----------------------------------------------------------------------------------------------------
def _sampler(h, w, table=None, pred="epsilon"):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=DR.emu_dd if table is None else table)
    stub = _Stub(1, h, w, 7)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m", "euler_a"])
@pytest.mark.parametrize("hw", [(8, 8), (8, 12)])
def test_exact_invariants(hw, sampler, fused):
    h, w = hw
    noise, x0, _ = _case(h, w, 1)

    def run(steps=6, **kw):
        smp, _ = _sampler(h, w)
        return smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=fused, sampler=sampler, seeds=[5], init_latents=x0, **kw)

    ones, zeros = torch.ones(1, 1, h, w), torch.zeros(1, 1, h, w)
    for strength in (0.5, 1.0):
        assert torch.equal(run(strength=strength, change_map=zeros), x0), strength                      # everything kept: the init latents, bit for bit
    free = run(strength=0.5)
    assert torch.equal(run(strength=0.5, change_map=ones), free) and not torch.equal(free, x0)            # ones: the maskless img2img call's bits
    two = ones.clone()
    two[..., : w // 2] = 0
    out = run(strength=0.5, change_map=two)
    assert torch.equal(out[..., : w // 2], x0[..., : w // 2]) and not torch.equal(out[..., w // 2:], x0[..., w // 2:])
    ramp = torch.linspace(0, 1, h * w).view(1, 1, h, w)
    out = run(strength=0.5, change_map=ramp)
    assert torch.isfinite(out).all() and torch.equal(out[0, :, 0, 0], x0[0, :, 0, 0]) and not torch.equal(out, free) and not torch.equal(out, x0)


def test_torch_loop_and_fused_against_reference_loop():
    h, w, steps, strength, g = 8, 12, 10, 0.6, 8.0
    noise, x0, _ = _case(h, w)
    ramp = torch.linspace(0, 1, h * w).view(1, 1, h, w)
    ref_stub = _Stub(1, h, w, 7)
    ref = DR.sample_loop(ref_stub.model, noise, steps, init_latents=x0, strength=strength, change_map=ramp, guidance_scale=g)
    for fused in (False, True):
        smp, stub = _sampler(h, w)
        got = smp.sample(EMB, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=fused, init_latents=x0, strength=strength, change_map=ramp)
        assert stub.calls == ref_stub.calls == 6
        # the bar of tests/test_img2img_cpu.py (rounding only: the select adds no operation to a released pixel and a held one is k in both)
        assert float((got - ref).abs().max()) <= 2.0 ** -14 * max(float(ref.abs().max()), float((x0.abs() + 3.4 * noise.abs()).max())), fused


def test_argument_errors():
    h, w = 8, 8
    noise, x0, mask = _case(h, w)
    smp, stub = _sampler(h, w)
    cm = torch.full((1, 1, h, w), 0.5)
    kw = dict(steps=10, latents=noise)
    with pytest.raises(ValueError, match="init_latents"):
        smp.sample(EMB, h, w, change_map=cm, **kw)
    with pytest.raises(ValueError, match="exclude"):
        smp.sample(EMB, h, w, init_latents=x0, strength=0.5, mask=mask, change_map=cm, **kw)
    for bad in (cm * 3, cm - 1, cm * float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            smp.sample(EMB, h, w, init_latents=x0, strength=0.5, change_map=bad, **kw)
    for bad in (torch.ones(1, 4, h, w), torch.ones(1, 1, h, w + 1), torch.ones(h, w)):
        with pytest.raises(ValueError, match="change_map"):
            smp.sample(EMB, h, w, init_latents=x0, strength=0.5, change_map=bad, **kw)
    # an op table without the kernel: the fused path refuses, naming it, before the UNet runs; the torch loop works
    smp2, stub2 = _sampler(h, w, table=IR.emu_img)
    for path in (dict(fused=True), dict(graph=True)):
        with pytest.raises(NotImplementedError, match="sampler_step_dd"):
            smp2.sample(EMB, h, w, init_latents=x0, strength=0.5, change_map=cm, **path, **kw)
    assert stub.calls == stub2.calls == 0
    assert smp2.sample(EMB, h, w, init_latents=x0, strength=0.5, change_map=cm, **kw).shape == (1, 4, h, w)


def test_latent_change_map():
    from PIL import Image
    from sd_lora_trainer_amd import dataset as D
    arr = np.zeros((32, 48), dtype=np.uint8)
    arr[:, 24:] = 255
    arr[:8, :8] = 128
    m = D.latent_change_map(Image.fromarray(arr), (48, 32), (4, 6))
    assert tuple(m.shape) == (1, 1, 4, 6) and m.dtype == torch.float32
    assert float(m[0, 0, 0, 0]) == float(np.float32(128) / np.float32(255)) and bool((m[0, 0, 1:, :3] == 0).all()) and bool((m[0, 0, :, 3:] == 1).all())
    assert bool((D.latent_change_map(Image.fromarray(np.full((20, 30, 3), 255, dtype=np.uint8)), (48, 32), (4, 6)) == 1).all())
    assert bool((D.latent_change_map(Image.fromarray(np.zeros((20, 30), dtype=np.uint8)), (48, 32), (4, 6)) == 0).all())


# ---- the command line and render() -------------------------------------------------------------------------------------------------------
def test_cli_argument_errors(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    init = ["--init-image", "i.png"]
    for extra, msg in ((["--change-map", "m.png"], "--init-image"), (["--mask-blur", "2"], "--init-image"),
                       (init + ["--change-map", "m.png", "--mask", "k.png"], "exclude"), (init + ["--mask-blur", "2"], "--change-map or --mask"),
                       (init + ["--change-map", "m.png", "--mask-blur", "-1"], "--mask-blur"), (init + ["--change-map", "m.png", "--mask-blur", "nan"], "--mask-blur"),
                       (init + ["--change-map", "m.png", "--hires-scale", "2"], "--change-map")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra


def _mk_rt(B=1, table=None):
    return unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=DR.emu_dd if table is None else table)


def test_render_with_change_map(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd import vae as V
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="cpu job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=4, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    _, (config, ckdir) = _run(T.train(cfg, runtime=_mk_rt()))
    ld = R.load_for_inference(ckdir, runtime=_mk_rt())
    f = 2 ** (len(ld.stack.decoder.ups) - 1)
    W, H = 12 * f, 8 * f
    rng = np.random.default_rng(0)
    init, black, white, half = (str(tmp_path / f"{k}.png") for k in ("init", "black", "white", "half"))
    Image.fromarray(rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)).save(init)
    Image.fromarray(np.zeros((50, 70), dtype=np.uint8)).save(black)
    Image.fromarray(np.full((50, 70, 3), 255, dtype=np.uint8)).save(white)
    hv = np.zeros((H, W), dtype=np.uint8)
    hv[:, W // 2:] = 255
    Image.fromarray(hv).save(half)
    # refusals of render(), before anything is built
    for kw, msg in ((dict(change_map_image=black), "init_image"), (dict(mask_blur=1.0, init_image=init), "mask_blur"),
                    (dict(init_image=init, change_map_image=black, mask_image=black), "exclude"),
                    (dict(init_image=init, change_map_image=black, hires=dict(scale=2.0)), "hires"),
                    (dict(init_image=init, change_map_image=black, mask_blur=-1.0), "mask_blur")):
        with pytest.raises(ValueError, match=msg):
            R.render(ld, ["a house"], str(tmp_path / "e"), size=(W, H), steps=4, **kw)
    ld_plain = R.load_for_inference(ckdir, runtime=_mk_rt(table=IR.emu_img))                              # an op table without the blur kernel
    with pytest.raises(NotImplementedError, match="blur_planes"):
        R.render(ld_plain, ["a house"], str(tmp_path / "e"), size=(W, H), steps=4, init_image=init, change_map_image=black, mask_blur=1.0)
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", str(W), str(H), "--steps", "4", "--seed", "5", "--init-image", init]
    outs = {}
    for tag, extra in (("keep", ["--change-map", black]), ("img", []), ("white", ["--change-map", white]), ("half", ["--change-map", half]),
                       ("soft", ["--change-map", half, "--mask-blur", "1.5"]), ("mask", ["--mask", half]), ("mask0", ["--mask", half, "--mask-blur", "0"]),
                       ("masksoft", ["--mask", half, "--mask-blur", "1.5"])):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(common + extra + ["--out", outs[tag]], runtime=_mk_rt())
    name = "img_00_seed5_scale0.85.jpg"
    px = {k: np.asarray(Image.open(os.path.join(d, name))) for k, d in outs.items()}
    # everything kept: the picture is decode(encode(image)), byte for byte
    x0, _ = R.encode_init(ld, init, None, (W, H), (H // f, W // f))
    dec = V.postprocess(ld.stack.decoder.decode(x0 / ld.models.cfg["scaling_factor"]))[0].permute(1, 2, 0)
    Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(tmp_path / "roundtrip.jpg", format="JPEG", quality=95)
    assert open(os.path.join(outs["keep"], name), "rb").read() == open(tmp_path / "roundtrip.jpg", "rb").read()
    assert np.array_equal(px["white"], px["img"]) and not np.array_equal(px["img"], px["keep"])          # a white map is the plain img2img render
    assert not np.array_equal(px["half"], px["img"]) and not np.array_equal(px["half"], px["keep"]) and not np.array_equal(px["soft"], px["half"])
    assert np.array_equal(px["mask0"], px["mask"]) and not np.array_equal(px["masksoft"], px["mask"])    # --mask-blur 0 launches nothing; a blurred mask blends
    meta = {k: json.load(open(os.path.join(d, "prompts.json"))) for k, d in outs.items()}
    assert meta["soft"]["change_map"] == dict(file=half, mask_blur=1.5) and meta["keep"]["change_map"] == dict(file=black, mask_blur=0.0)
    assert "change_map" not in meta["img"] and "change_map" not in meta["mask"] and "mask_blur" not in meta["mask"] and "mask_blur" not in meta["img"]
    assert meta["masksoft"]["mask_blur"] == 1.5 and meta["masksoft"]["masked"] is True and "change_map" not in meta["masksoft"]


# ---- the entry points refuse bad arguments before they launch anything (no GPU involved) -------------------------------------------------
def test_entry_point_validation():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_sampler_step_dd" in _lib.SYMBOLS and C.sizeof(_lib.SamplerDdParams) == 128
    assert lib.sdlt_sampler_step_dd(None, None) == -1 and b"sdlt_sampler_step_dd" in lib.sdlt_last_error()
    ok = dict(eps=0x1000, x=0x2000, x0=0x3000, noise=0x4000, dprev=0x5000, xin=0x6000, ld_xin=64, timesteps=0x7000, table=0x8000, ctr=0x9000,
              n=1, hw=35, table_rows=5, init=0, seeds=0xA000, hold=0xB000, form=2)
    SHAPE, ALIGN, UNSUPPORTED = -1, -2, -4
    for change, code in ((dict(n=0), SHAPE), (dict(hw=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE), (dict(table_rows=2), SHAPE),       # what its siblings refuse
                         (dict(x=None), SHAPE), (dict(xin=None), SHAPE), (dict(timesteps=None), SHAPE), (dict(table=None), SHAPE), (dict(ctr=None), SHAPE),
                         (dict(eps=None), SHAPE), (dict(x0=None), SHAPE), (dict(noise=None), SHAPE), (dict(dprev=None), SHAPE), (dict(seeds=None), SHAPE),
                         (dict(form=1, dprev=None), SHAPE), (dict(init=1, x0=None), SHAPE), (dict(init=1, noise=None), SHAPE),
                         (dict(x0=0x2000), SHAPE), (dict(noise=0x2000), SHAPE), (dict(init=1, noise=0x2000), SHAPE), (dict(dprev=0x2000), SHAPE),
                         (dict(dprev=0x3000), SHAPE), (dict(dprev=0x4000), SHAPE),
                         (dict(ld_xin=2), ALIGN), (dict(ld_xin=66), ALIGN), (dict(xin=0x6004), ALIGN), (dict(eps=0x1008), ALIGN), (dict(x=0x2002), ALIGN),
                         (dict(x0=0x3002), ALIGN), (dict(noise=0x4001), ALIGN), (dict(dprev=0x5002), ALIGN), (dict(seeds=0xA002), ALIGN),
                         (dict(hold=None), SHAPE), (dict(form=0, hold=None), SHAPE),                                                            # its own
                         (dict(hold=0x2000), SHAPE), (dict(hold=0x5000), SHAPE), (dict(form=1, hold=0x5000), SHAPE), (dict(form=0, hold=0x2000), SHAPE),
                         (dict(hold=0xB002), ALIGN), (dict(form=3), UNSUPPORTED), (dict(form=-1), UNSUPPORTED)):
        p = _lib.SamplerDdParams(**dict(ok, **change))
        assert lib.sdlt_sampler_step_dd(C.byref(p), None) == code, change
        assert b"sdlt_sampler_step_dd" in lib.sdlt_last_error(), change


def test_blur_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    ok = dict(src=0x10000, out=0x20000, scratch=0x30000, C=1, H=5, W=7, taps=0x40000, R=2, clamp01=0)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(src=None), SHAPE), (dict(out=None), SHAPE), (dict(scratch=None), SHAPE), (dict(taps=None), SHAPE),
                         (dict(C=0), SHAPE), (dict(H=0), SHAPE), (dict(W=-1), SHAPE), (dict(H=16385), SHAPE), (dict(W=16385), SHAPE), (dict(C=65536), SHAPE),
                         (dict(R=65), SHAPE), (dict(R=-1), SHAPE),
                         (dict(scratch=0x10000), SHAPE), (dict(scratch=0x20000), SHAPE), (dict(scratch=0x10000 + 4 * 34), SHAPE), (dict(scratch=0x20000 - 4), SHAPE),
                         (dict(src=0x10002), ALIGN), (dict(out=0x20001), ALIGN), (dict(scratch=0x30002), ALIGN), (dict(taps=0x40003), ALIGN)):
        a = dict(ok, **change)
        rc = lib.sdlt_blur_planes(a["src"], a["out"], a["scratch"], a["C"], a["H"], a["W"], a["taps"], a["R"], a["clamp01"], None)
        assert rc == code, change
        assert b"sdlt_blur_planes" in lib.sdlt_last_error(), change
