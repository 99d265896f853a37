"""Guidance rescale, guidance interval, a per-step guidance scale and the negative prompt without a GPU: the restated rescale (tests/guidance_ref.py),
sampler.guidance_table, LatentSampler.sample(guidance_scale=[...], guidance_rescale=, guidance_interval=) - torch loop and fused path on the emulated
op table - the argument errors, the command line and the negative prompt's way to the encoder."""
import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import guidance_ref as GR
from tests import sde_ref as SR
from tests.test_multistep_cpu import CASES, EMB, _case, _Stub

FAMILIES = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")


# ---- the rescale ---------------------------------------------------------------------------------------------------------------------------
def test_rescale_against_direct_restatement():
    g = torch.Generator().manual_seed(0)
    ep, en = torch.randn(3, 4, 5, 7, generator=g, dtype=torch.float64) * 1.3 + 0.2, torch.randn(3, 4, 5, 7, generator=g, dtype=torch.float64)
    ec = en + 7.5 * (ep - en)
    N = 4 * 5 * 7
    for phi in (0.0, 0.3, 0.7, 1.0):
        got = GR.rescale(ep, ec, phi)
        assert got.dtype == torch.float64
        for j in range(3):                                                       # per image, the sums written out: divisor N - 1, about the mean
            sp = float((((ep[j] - ep[j].sum() / N) ** 2).sum() / (N - 1)) ** 0.5)
            sc = float((((ec[j] - ec[j].sum() / N) ** 2).sum() / (N - 1)) ** 0.5)
            want = phi * (ec[j] * (sp / sc)) + (1 - phi) * ec[j]
            assert float((got[j] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        if phi == 0.0:
            assert torch.equal(got, ec)
        if phi == 1.0:
            for j in range(3):
                assert abs(float(got[j].std()) / float(ep[j].std()) - 1.0) <= 1e-12
    # the contract on CPU tensors is that function with its statistics in fp64 and the rest in fp32
    eps = torch.randn(2 * 3 * 35, 4, generator=g)
    gtab = torch.tensor([[1.0, 0, 0, 0], [7.5, 0.7, 0, 0]])
    want = eps.clone().view(3, 2, 35, 4).double()
    want = GR.rescale(want[:, 1], want[:, 0] + 7.5 * (want[:, 1] - want[:, 0]), float(np.float32(0.7)))
    got = GR.guidance(eps, gtab, torch.zeros(2, dtype=torch.int32), 3).view(3, 2, 35, 4)
    assert torch.equal(got[:, 0], got[:, 1]) and float((got[:, 0].double() - want).abs().max()) <= 8 * 2.0 ** -24 * float(want.abs().max())


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
@pytest.mark.parametrize("n,start", [(10, 0), (10, 4), (25, 10), (1, 0)])
def test_guidance_table(n, start, sigkind):
    s = SM.EulerDiscrete().set_timesteps(n, start, sigkind)
    k = n - start
    sig = s.sigmas[:k].astype(np.float64)
    tab = SM.guidance_table(s, 7.5)
    assert tab.shape == (1 + k, 4) and tab.dtype == torch.float32 and tab[0].tolist() == [float(k), 0.0, 0.0, 0.0]
    assert tab[1:, 0].tolist() == [7.5] * k and bool((tab[1:, 1:] == 0).all())
    seq = [1.0 + 0.5 * i for i in range(k)]                                      # (its first entry is 1: no rescale on that row)
    tab = SM.guidance_table(s, seq, 0.7)
    assert tab[1:, 0].tolist() == seq and tab[1:, 1].tolist() == [0.0] + [float(np.float32(0.7))] * (k - 1) and bool((tab[:, 2:] == 0).all())
    if k >= 3:
        lo, hi = float(sig[-1]), float(sig[1])                                   # (lo, hi]: sigma_1 is inside, the last sigma is outside, sigma_0 is above
        for gs in (7.5, seq):
            tab = SM.guidance_table(s, gs, 0.7, (lo, hi))
            want = GR.schedule_g(sig, gs, (lo, hi))
            inside = [bool(lo < v <= hi) for v in sig]
            assert inside[0] is False and inside[1] is True and inside[-1] is False and any(inside)
            assert tab[1:, 0].tolist() == want and all((w == 1.0) or i for w, i in zip(want, inside))
            assert [float(v) == 1.0 for v in tab[1:, 0]] == [(not i) or gi == 1.0 for i, gi in zip(inside, seq if gs is seq else [7.5] * k)]
            assert tab[1:, 1].tolist() == [0.0 if w == 1.0 else float(np.float32(0.7)) for w in want]
    every = SM.guidance_table(s, 7.5, 0.3, (0.0, 1e9))                           # an interval that holds every sigma
    assert torch.equal(every, SM.guidance_table(s, 7.5, 0.3))
    assert SM.guidance_in_use(7.5) is False and SM.guidance_in_use(8) is False
    assert SM.guidance_in_use([7.5]) and SM.guidance_in_use(7.5, 0.1) and SM.guidance_in_use(7.5, 0.0, (0.0, 1.0))


# ---- LatentSampler on the emulated op table ------------------------------------------------------------------------------------------------
def _stub_sampler(h, w, pred="epsilon", seed=7, ops=GR.emu_guidance):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=ops)
    stub = _Stub(h, w, seed)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


def _kw(family, case, x0, mask):
    kw = dict(CASES[case])
    img = dict(init_latents=x0, strength=kw["strength"], mask=mask if kw.get("masked") else None) if kw else {}
    return dict(img, sampler=family, **(dict(seeds=[0x1234567ABCDEF]) if family in SM.SDE_KINDS else {})), (6 if kw else 10)


@pytest.mark.parametrize("case", ["txt2img", "masked"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("family", FAMILIES)
def test_torch_loop_equals_fused(family, pred, case):
    h, w, steps = 8, 12, 10
    noise, x0, mask = _case(h, w)
    kw, k = _kw(family, case, x0, mask)
    sig = SM.EulerDiscrete().set_timesteps(steps, steps - k).sigmas
    interval = (float(sig[-2]), float(sig[1]))                                   # guidance off at the first and the last step that runs
    out = {}
    for fused in (False, True):
        smp, stub = _stub_sampler(h, w, pred)
        out[fused] = smp.sample(EMB, h, w, steps=steps, guidance_scale=7.5, guidance_rescale=0.7, guidance_interval=interval, latents=noise.clone(),
                                fused=fused, **kw)
        assert stub.calls == k and out[fused].dtype == torch.float32 and bool(torch.isfinite(out[fused]).all())
    assert torch.equal(out[False], out[True])                                    # bit for bit
    if case == "masked":
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(out[True][keep], x0[keep])
    # every control changes the result, and for the deterministic families the fp64 loop with the published rescale is rounding away.  The bar is
    # tests/test_sde_cpu.py's for these shapes: the multistep path's worst-case rounding bound stays below 2^-8 max|x|, and the blend adds three
    # operations on a value of the prediction's size
    smp, stub = _stub_sampler(h, w, pred)
    run = lambda **k2: (setattr(stub, "calls", 0), smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=True, **dict(kw, **k2)))[1]  # noqa: E731
    plain = run(guidance_scale=7.5)
    assert not torch.equal(run(guidance_scale=7.5, guidance_rescale=0.7), plain) and not torch.equal(run(guidance_scale=7.5, guidance_interval=interval), plain)
    assert not torch.equal(run(guidance_scale=7.5, guidance_rescale=0.7), out[True])
    if family in ("euler", "dpmpp_2m"):
        img = {k2: v for k2, v in kw.items() if k2 in ("init_latents", "strength", "mask")}
        ref = GR.sample_loop(_Stub(h, w, 7).model, noise, steps, sampler=family, guidance_scale=7.5, guidance_rescale=float(np.float32(0.7)),
                             guidance_interval=interval, prediction_type=pred, **img)
        mx = float((x0.abs() + 14.7 * noise.abs()).max())
        err = float((out[True].double() - ref).abs().max())
        print(family, pred, case, err, mx)
        assert err <= 2.0 ** -8 * mx


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_constant_schedule_through_the_pre_pass_is_the_scalar_path(family, fused):
    """g constant and phi = 0 passed as a sequence: the pre-pass writes e_c into both rows, the step launch returns it - the final latents are the
    scalar path's (the fused one: the torch loop of the deterministic samplers rounds differently without the pre-pass, as before).  And an interval
    that holds every sigma is no interval."""
    h, w, steps = 8, 12, 10
    noise, x0, mask = _case(h, w, 3)
    for case in ("txt2img", "masked"):
        kw, k = _kw(family, case, x0, mask)
        smp, stub = _stub_sampler(h, w)
        run = lambda f=fused, **k2: (setattr(stub, "calls", 0), smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=f, **dict(kw, **k2)))[1]  # noqa: E731
        scalar = run(f=True, guidance_scale=7.5)
        assert torch.equal(run(guidance_scale=[7.5] * k), scalar), (family, case)
        assert torch.equal(run(guidance_scale=7.5, guidance_interval=(0.0, 1e9)), scalar), (family, case)
        resc = run(guidance_scale=7.5, guidance_rescale=0.5)
        assert torch.equal(run(guidance_scale=7.5, guidance_rescale=0.5, guidance_interval=(0.0, 1e9)), resc) and not torch.equal(resc, scalar)
        assert torch.equal(run(f=True, guidance_scale=7.5), scalar)              # and the default call after guided ones is what it was
        with pytest.raises(ValueError, match="guidance_scale"):
            run(guidance_scale=[7.5] * (k + 1))


def test_defaults_launch_nothing_new():
    """A scalar guidance scale without rescale and interval needs no guidance op and builds no new state."""
    h, w = 8, 8
    noise, _, _ = _case(h, w, 2)
    for fused in (False, True):
        rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=SR.emu_sde)
        smp = SM.LatentSampler(rt, _Stub(h, w, 7))
        assert not hasattr(rt.ops, "guidance")
        out = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, guidance_scale=7.5, guidance_rescale=0.0, guidance_interval=None)
        assert out.shape == (1, 4, h, w) and smp._guided_graphs == {} and (smp._fused is None or "gtab" not in smp._fused)
        for kw in (dict(guidance_rescale=0.5), dict(guidance_interval=(1.0, 5.0)), dict(guidance_scale=[7.5] * 6)):
            with pytest.raises(NotImplementedError, match="guidance"):
                smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, **kw)


def test_argument_errors():
    h, w = 8, 8
    noise, x0, _ = _case(h, w)
    smp, stub = _stub_sampler(h, w)
    for fused in (False, True):
        for family in FAMILIES:
            base = dict(steps=4, latents=noise, fused=fused, sampler=family)
            for phi in (-0.1, 1.5, float("nan")):
                with pytest.raises(ValueError, match="guidance_rescale"):
                    smp.sample(EMB, h, w, guidance_rescale=phi, **base)
            for seq in ([7.5] * 3, [7.5] * 5, []):
                with pytest.raises(ValueError, match="guidance_scale"):
                    smp.sample(EMB, h, w, guidance_scale=seq, **base)
            for iv in ((2.0, 2.0), (3.0, 1.0)):
                with pytest.raises(ValueError, match="guidance_interval"):
                    smp.sample(EMB, h, w, guidance_interval=iv, **base)
        with pytest.raises(ValueError, match="guidance_scale"):                   # img2img: one value per step that RUNS (int(5 * 0.6) = 3)
            smp.sample(EMB, h, w, steps=5, latents=noise, fused=fused, guidance_scale=[7.5] * 5, init_latents=x0, strength=0.6)
        stub.calls = 0
        assert smp.sample(EMB, h, w, steps=5, latents=noise, fused=fused, guidance_scale=[7.5] * 3, init_latents=x0, strength=0.6).shape == (1, 4, h, w)
        stub.calls = 0


def test_cli_arguments(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--guidance-rescale", "1.5"], "--guidance-rescale"), (["--guidance-rescale", "-0.1"], "--guidance-rescale"),
                       (["--guidance-rescale", "much"], "--guidance-rescale"), (["--guidance-interval", "3", "1"], "--guidance-interval"),
                       (["--guidance-interval", "2", "2"], "--guidance-interval"), (["--guidance-interval", "2"], "--guidance-interval"),
                       (["--negative-prompt"], "--negative-prompt")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_load(checkpoint, pm, device=None, runtime=None):
        return "loaded"

    def fake_render(loaded, prompts, out, **kw):
        seen.update(kw)
        return {}

    import unittest.mock as mock
    with mock.patch.object(R, "load_for_inference", fake_load), mock.patch.object(R, "render", fake_render):
        R.main(base + ["--guidance-rescale", "0.7", "--guidance-interval", "0.5", "5.5", "--negative-prompt", "blurry, low quality"])
        assert seen["guidance_rescale"] == 0.7 and tuple(seen["guidance_interval"]) == (0.5, 5.5) and seen["negative_prompt"] == "blurry, low quality"
        R.main(base)
        assert seen["guidance_rescale"] == 0.0 and seen["guidance_interval"] is None and seen["negative_prompt"] is None
    # render() itself refuses them before it builds anything
    for kw, msg in ((dict(guidance_rescale=2.0), "guidance_rescale"), (dict(guidance_interval=(3.0, 1.0)), "guidance_interval")):
        with pytest.raises(ValueError, match=msg):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), **kw)


class _FakeLoaded:
    class _C:
        training_attributes, concept_mode, seed, prompt_modifier, sample_imgs_lora_scale, validation_img_size = None, "object", 0, None, 0.8, 64

    class _S:
        decoder = object()
        rt = type("rt", (), dict(device=torch.device("cpu")))()

    class _M:
        cfg = dict(addition=False, scaling_factor=0.18215)

    config, stack, models = _C(), _S(), _M()


# ---- the negative prompt -------------------------------------------------------------------------------------------------------------------
def test_negative_prompt_reaches_the_encoder():
    from sd_lora_trainer_amd import prompts as P
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    stack = T.RenderStack.__new__(T.RenderStack)
    stack.config = TrainingConfig(lora_training_urls="synthetic:1", concept_mode="object", name="np job", _make_dirs=False)
    calls = []

    def encode(prompt, negative):
        calls.append((prompt, negative))
        return (torch.zeros(1, 77, 8), torch.zeros(1, 77, 8))

    stack.encode = encode
    stack.conditioning("a photo of <concept>", 0.8)
    assert len(calls) == 2 and all(neg == P.NEGATIVE_PROMPT for _, neg in calls)
    del calls[:]
    stack.conditioning("a photo of <concept>", 0.8, None, None)
    assert len(calls) == 2 and all(neg == P.NEGATIVE_PROMPT for _, neg in calls)
    del calls[:]
    stack.conditioning("a photo of <concept>", 0.8, negative_prompt="blurry,  low quality ")
    assert len(calls) == 2 and all(neg == "blurry,  low quality " for _, neg in calls) and calls[0][0] != calls[1][0]
    del calls[:]
    stack.conditioning("a photo of <concept>", 0.8, negative_prompt="")          # an empty negative prompt is the caller's own, not the default
    assert [neg for _, neg in calls] == ["", ""]


# ---- the entry point refuses bad arguments before it launches anything (no GPU involved) -----------------------------------------------
def test_entry_point_validation():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_guidance" in _lib.SYMBOLS and _lib.struct_sizes()[-1] == ("GuidanceParams", 40) and lib.sdlt_struct_size(25) == 40
    assert lib.sdlt_guidance(None, None) == -1 and b"sdlt_guidance" in lib.sdlt_last_error()
    ok = dict(eps=0x1000, gtab=0x2000, ctr=0x3000, n=1, hw=35, gtab_rows=5)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(eps=None), SHAPE), (dict(gtab=None), SHAPE), (dict(ctr=None), SHAPE), (dict(n=0), SHAPE), (dict(n=-1), SHAPE), (dict(hw=0), SHAPE),
                         (dict(hw=-3), SHAPE), (dict(gtab_rows=1), SHAPE), (dict(gtab_rows=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE),
                         (dict(eps=0x1008), ALIGN), (dict(eps=0x1004), ALIGN), (dict(gtab=0x2002), ALIGN), (dict(ctr=0x3001), ALIGN)):
        p = _lib.GuidanceParams(**dict(ok, **change))
        assert lib.sdlt_guidance(C.byref(p), None) == code, change
        assert b"sdlt_guidance" in lib.sdlt_last_error()
