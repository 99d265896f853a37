"""Sampling from an init image without a GPU: the schedule offset and the step table against hand-computed cases, LatentSampler.sample(init_latents=,
strength=, mask=) - the torch loop and, on the emulated op table with the restated kernels (tests/img2img_ref.py), the fused path - against the
plain-torch reference loop, the exact invariants of the mask, and the argument errors of the sampler, render() and the command line."""
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import unet_ref as U
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd import topology
from sd_lora_trainer_amd.config import TrainingConfig
from tests import img2img_ref as IR
from tests.test_driver_cpu import _run, _tokenizer_dir


# ---- schedule and table ---------------------------------------------------------------------------------------------------------------
def test_schedule_offset_hand_computed():
    assert SM.img2img_steps(25, 0.6) == (15, 10)
    assert SM.img2img_steps(25, 1.0) == (25, 0)
    assert SM.img2img_steps(30, 0.5) == (15, 15) and SM.img2img_steps(4, 0.3) == (1, 3)
    for bad in (0.03, 0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(ValueError):
            SM.img2img_steps(25, bad)
    full = SM.EulerDiscrete().set_timesteps(25)
    ts_full, sig_full = full.timesteps.copy(), full.sigmas.copy()
    s = SM.EulerDiscrete().set_timesteps(25, start=10)
    # trailing spacing, 25 steps: 999, 959, ... (40 apart): entry 10 is timestep 599, the last one 39
    assert len(s.timesteps) == 15 and len(s.sigmas) == 16 and s.timesteps[0] == 599.0 and s.timesteps[-1] == 39.0 and s.sigmas[-1] == 0.0
    assert np.array_equal(s.timesteps, ts_full[10:]) and np.array_equal(s.sigmas, sig_full[10:])
    assert float(s.sigmas[0]) == float(np.float32(np.float64(s.sigmas_all[599])))
    again = SM.EulerDiscrete().set_timesteps(25)                     # the plain call is what it was
    assert np.array_equal(again.timesteps, ts_full) and np.array_equal(again.sigmas, sig_full) and again.init_noise_sigma == float(sig_full.max())
    k, start, ts, sig = IR.schedule(25, 0.6)
    assert (k, start) == (15, 10) and list(ts) == [int(t) for t in s.timesteps]
    torch.testing.assert_close(torch.tensor(sig, dtype=torch.float32), torch.tensor(s.sigmas), rtol=1e-6, atol=0)


def test_step_table_img_rows():
    s = SM.EulerDiscrete(prediction_type="v_prediction").set_timesteps(25, start=10)
    tab = SM.step_table_img(s, 7.5)
    assert tab.shape == (17, 4) and tab.dtype == torch.float32
    sig0 = np.float64(s.sigmas[0])
    assert tab[0].tolist() == [7.5, float(s.sigmas[0]), float(np.float32(1 / np.sqrt(sig0 ** 2 + 1))), 599.0]      # column 1: the FIRST USED sigma
    assert float(tab[0, 1]) < 14.0                                                                           # not init_noise_sigma of the full schedule
    assert tab[1].tolist() == [15.0, 1.0, 0.0, 0.0]
    assert tab[2].tolist()[:2] == [float(s.sigmas[0]), float(s.sigmas[1])] and float(tab[2, 3]) == 559.0
    assert tab[16].tolist() == [float(s.sigmas[14]), 0.0, 1.0, 599.0]                                        # the last row steps to sigma 0 and wraps the timestep
    # strength 1: the table of txt2img except for nothing - the first used sigma IS init_noise_sigma
    s1 = SM.EulerDiscrete().set_timesteps(6, start=0)
    assert torch.equal(SM.step_table_img(s1, 8.0), SM.step_table(SM.EulerDiscrete().set_timesteps(6), 8.0))


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
class _Stub:
    """A UNet stand-in whose prediction depends on its input, the timestep and the call: eps = E[call] + tanh(xin) / 4 + t / 4000."""

    def __init__(self, n, h, w, seed, calls=12):
        self.cfg, self.arena = dict(cross_dim=8, addition=False), None
        g = torch.Generator().manual_seed(seed)
        self.E = [torch.randn(2 * n, 4, h, w, generator=g) for _ in range(calls)]
        self.calls = 0

    def model(self, xin, t):
        self.calls += 1
        return self.E[self.calls - 1] + torch.tanh(xin) / 4 + t / 4000.0

    def forward(self, x, t, ctx, pooled, tid, *, B, H, W):
        xin = x[:, :4].float().view(B, H, W, 4).permute(0, 3, 1, 2)
        assert torch.equal(xin[0::2], xin[1::2]) and bool((t == t[0]).all())          # both rows of a pair hold the same model input
        return self.model(xin, float(t[0])).permute(0, 2, 3, 1).reshape(B * H * W, 4).contiguous()


EMB = (torch.zeros(1, 77, 8), torch.zeros(1, 77, 8), None, None)


def _case(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    noise, x0 = torch.randn(1, 4, h, w, generator=g), 0.8 * torch.randn(1, 4, h, w, generator=g)
    mask = (torch.rand(1, 1, h, w, generator=g) * 3).floor() / 2                     # 0, 0.5 and 1
    return noise, x0, mask


def _stub_sampler(h, w, pred="epsilon", seed=7):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=IR.emu_img)
    stub = _Stub(1, h, w, seed)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_paths_against_reference_loop_stub(pred, masked, fused):
    h, w, steps, strength, g = 8, 12, 10, 0.6, 8.0
    noise, x0, mask = _case(h, w)
    mask = mask if masked else None
    smp, stub = _stub_sampler(h, w, pred)
    got = smp.sample(EMB, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=fused, init_latents=x0, strength=strength, mask=mask)
    ref_stub = _Stub(1, h, w, 7)
    ref = IR.sample_loop(ref_stub.model, noise, steps, init_latents=x0, strength=strength, mask=mask, guidance_scale=g, prediction_type=pred)
    assert stub.calls == ref_stub.calls == 6
    # Both are fp32 throughout and differ in rounding only: <= 15 operations per step on the update (tests/test_render_gpu.py counts them), and a model input
    # that differs by ~2 ulp (x / sqrt(..) against x * (1 / sqrt(..))), which guidance 8 passes on with a factor <= (1 + 2 * 8) / 4 * |dt| < 9 per step (|dt| < 2
    # from sigma 3.4 down).  6 steps x (15 + 2 * 9) ulp ~ 200 ulp of the largest magnitude on the path; the bar is 2^-14 of it (1024 ulp).
    assert float((got - ref).abs().max()) <= 2.0 ** -14 * max(float(ref.abs().max()), float((x0.abs() + 3.4 * noise.abs()).max()))
    assert not torch.equal(got, x0)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_torch_loop_matches_reference_loop_unet(pred):
    """The torch loop with the real (tiny) UNet on the emulated op table against the fp32 oracle UNet: the bar of tests/test_sampler_cpu.py."""
    version, h, w, rank, steps, scale, strength = "tiny15", 8, 12, 4, 5, 0.75, 0.6
    cfg = U.CONFIGS[version]
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    g = torch.Generator().manual_seed(5)
    embeds = (torch.randn(1, 77, cfg["cross_dim"], generator=g), torch.randn(1, 77, cfg["cross_dim"], generator=g), None, None)
    noise, x0, mask = _case(h, w, 3)
    ref = IR.sample_latents(cfg, sd, lora, scale, embeds, noise, steps, init_latents=x0, strength=strength, mask=mask, prediction_type=pred)
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=IR.emu_img)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    smp = SM.LatentSampler(rt, unet, prediction_type=pred)
    smp.set_lora_scale(scale)
    got = smp.sample(embeds, h, w, steps=steps, latents=noise, init_latents=x0, strength=strength, mask=mask)
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(got[keep], x0[keep]) and torch.equal(ref[keep], x0[keep])


# ---- exact invariants (the GPU suite repeats them on the kernels) -------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("hw", [(8, 8), (8, 12)])
def test_exact_invariants(hw, fused):
    h, w = hw
    steps = 6
    noise, x0, _ = _case(h, w, 1)

    def run(**kw):
        smp, _ = _stub_sampler(h, w)
        return smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=fused, **kw)

    plain = run()
    assert torch.equal(run(init_latents=x0, strength=1.0), plain)                                       # (a) strength 1 without a mask is txt2img from the noise
    ones, zeros = torch.ones(1, 1, h, w), torch.zeros(1, 1, h, w)
    assert torch.equal(run(init_latents=x0, strength=1.0, mask=ones), plain)
    free = run(init_latents=x0, strength=0.5)
    assert not torch.equal(free, plain) and not torch.equal(free, x0)
    assert torch.equal(run(init_latents=x0, strength=0.5, mask=ones), free)                             # (b) a mask of ones is no mask
    assert torch.equal(run(init_latents=x0, strength=0.5, mask=zeros), x0)                              # (c) a mask of zeros returns the init latents
    assert torch.equal(run(init_latents=x0, strength=1.0, mask=zeros), x0)
    half = ones.clone()
    half[..., : w // 2] = 0
    out = run(init_latents=x0, strength=0.5, mask=half)
    assert torch.equal(out[..., : w // 2], x0[..., : w // 2])                                           # (d) the kept half is the init latents
    assert not torch.equal(out[..., w // 2:], x0[..., w // 2:])
    assert torch.equal(run(), plain)


def test_argument_errors():
    h, w = 8, 8
    noise, x0, mask = _case(h, w)
    smp, _ = _stub_sampler(h, w)
    kw = dict(steps=10, latents=noise)
    with pytest.raises(ValueError, match="init_latents"):
        smp.sample(EMB, h, w, mask=mask, **kw)
    with pytest.raises(ValueError, match="init_latents"):
        smp.sample(EMB, h, w, strength=0.5, **kw)
    for bad in (0.0, 1.5, 0.03):
        with pytest.raises(ValueError, match="strength"):
            smp.sample(EMB, h, w, init_latents=x0, strength=bad, **kw)
    for bad in (mask * 2, mask - 0.5, mask * float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            smp.sample(EMB, h, w, init_latents=x0, strength=0.5, mask=bad, **kw)
    with pytest.raises(ValueError, match="mask"):
        smp.sample(EMB, h, w, init_latents=x0, strength=0.5, mask=torch.ones(1, 4, h, w), **kw)
    with pytest.raises(ValueError, match="init_latents"):
        smp.sample(EMB, h, w, init_latents=x0[..., :4], strength=0.5, **kw)
    # an op table with the txt2img kernel only: the fused path refuses instead of falling back
    from tests.test_render_cpu import emu_render
    smp2 = SM.LatentSampler(unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=emu_render), _Stub(1, h, w, 7))
    with pytest.raises(NotImplementedError, match="sampler_step_img"):
        smp2.sample(EMB, h, w, init_latents=x0, strength=0.5, fused=True, **kw)
    assert smp2.sample(EMB, h, w, init_latents=x0, strength=0.5, **kw).shape == (1, 4, h, w)


def test_cli_argument_errors(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--mask", "m.png"], "--init-image"), (["--strength", "0.5"], "--init-image"),
                       (["--init-image", "i.png", "--strength", "0"], "--strength"), (["--init-image", "i.png", "--strength", "1.2"], "--strength")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err


# ---- render() ----------------------------------------------------------------------------------------------------------------------------
def _mk_rt(B=1):
    return unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=IR.emu_img)


def test_render_from_init_image(tmp_path, monkeypatch):
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
    init = tmp_path / "init.png"
    Image.fromarray(rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)).save(init)                      # another size: resized to --size
    black, white = tmp_path / "black.png", tmp_path / "white.png"
    Image.fromarray(np.zeros((50, 70), dtype=np.uint8)).save(black)
    Image.fromarray(np.full((50, 70, 3), 255, dtype=np.uint8)).save(white)
    with pytest.raises(ValueError, match="init_image"):
        R.render(ld, ["a house"], str(tmp_path / "e1"), size=(W, H), steps=4, mask_image=str(black))
    with pytest.raises(ValueError, match="strength"):
        R.render(ld, ["a house"], str(tmp_path / "e2"), size=(W, H), steps=4, init_image=str(init), strength=0.1)
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", str(W), str(H), "--steps", "4", "--seed", "5", "--init-image", str(init)]
    outs = {}
    for tag, extra in (("keep", ["--mask", str(black)]), ("img", []), ("white", ["--mask", str(white)]), ("s1", ["--strength", "1.0"]), ("s1w", ["--strength", "1.0", "--mask", str(white)])):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(common + extra + ["--out", outs[tag]], runtime=_mk_rt())
    name = "img_00_seed5_scale0.85.jpg"
    px = {k: np.asarray(Image.open(os.path.join(d, name))) for k, d in outs.items()}
    assert px["keep"].shape == (H, W, 3)
    # everything kept: the picture is decode(encode(image)), bit for bit
    x0, _ = R.encode_init(ld, str(init), None, (W, H), (H // f, W // f))
    dec = V.postprocess(ld.stack.decoder.decode(x0 / ld.models.cfg["scaling_factor"]))[0].permute(1, 2, 0)
    Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(tmp_path / "roundtrip.jpg", format="JPEG", quality=95)
    assert np.array_equal(px["keep"], np.asarray(Image.open(tmp_path / "roundtrip.jpg")))
    assert not np.array_equal(px["img"], px["keep"]) and np.array_equal(px["white"], px["img"])          # a white mask regenerates everything
    # strength 1 without a mask (or with a white one) is the plain render from the same seed
    R.main([a for a in common if a not in ("--init-image", str(init))] + ["--out", str(tmp_path / "out_plain")], runtime=_mk_rt())
    plain = np.asarray(Image.open(os.path.join(str(tmp_path / "out_plain"), name)))
    assert np.array_equal(px["s1"], plain) and np.array_equal(px["s1w"], plain) and not np.array_equal(px["img"], plain)


# ---- the entry point refuses bad arguments before it launches anything (no GPU involved) -------------------------------------------
def test_entry_point_validation():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert lib.sdlt_sampler_step_img(None, None) == -1 and b"sdlt_sampler_step_img" in lib.sdlt_last_error()
    ok = dict(eps=0x1000, x=0x2000, x0=0x3000, noise=0x4000, mask=0x5000, xin=0x6000, ld_xin=64, timesteps=0x7000, table=0x8000, ctr=0x9000,
              n=1, hw=35, table_rows=5, init=0)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(n=0), SHAPE), (dict(hw=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE), (dict(table_rows=2), SHAPE),
                         (dict(x=None), SHAPE), (dict(xin=None), SHAPE), (dict(timesteps=None), SHAPE), (dict(table=None), SHAPE), (dict(ctr=None), SHAPE),
                         (dict(eps=None), SHAPE), (dict(x0=None), SHAPE), (dict(noise=None), SHAPE),                # a step with a mask reads both
                         (dict(init=1, x0=None, mask=None), SHAPE), (dict(init=1, noise=None), SHAPE),
                         (dict(x0=0x2000), SHAPE), (dict(init=1, noise=0x2000), SHAPE),                             # may not alias x
                         (dict(ld_xin=2), ALIGN), (dict(ld_xin=66), ALIGN), (dict(xin=0x6004), ALIGN), (dict(eps=0x1008), ALIGN),
                         (dict(x=0x2002), ALIGN), (dict(mask=0x5001), ALIGN), (dict(x0=0x3002), ALIGN), (dict(noise=0x4001), ALIGN)):
        p = _lib.SamplerImgParams(**dict(ok, **change))
        assert lib.sdlt_sampler_step_img(C.byref(p), None) == code, change
        assert b"sdlt_sampler_step_img" in lib.sdlt_last_error()
