"""DPM-Solver++ (2M) and Karras noise levels without a GPU: the convergence order of sampler.DpmSolverPP2M on an analytic denoiser, the schedules, the
step table's coefficients, LatentSampler.sample(sampler="dpmpp_2m") - the torch loop and, on the emulated op table with the restated kernels
(tests/multistep_ref.py), the fused path - against the fp64 reference loop, the exact invariant of an all-zero mask, and the argument errors."""
import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import multistep_ref as MR

U24 = 2.0 ** -24


# ---- convergence order ------------------------------------------------------------------------------------------------------------------
C2 = 0.64                      # data N(0, 0.8^2 I): the exact denoiser is D(x, sigma) = x C2 / (C2 + sigma^2), e = (x - D) / sigma = x sigma / (C2 + sigma^2)


def _final_error(cls, N):
    """|x_N - exact| at the last sigma of a grid uniform in log sigma from 14.6146 to 0.03, everything in fp64."""
    sig = np.exp(np.linspace(np.log(14.6146), np.log(0.03), N + 1))
    sched = cls().set_sigmas(sig)
    assert sched.sigmas.dtype == np.float64
    x = torch.tensor([(C2 + sig[0] ** 2) ** 0.5], dtype=torch.float64)
    start = float(x)
    for i in range(N):
        e = x * sig[i] / (C2 + sig[i] ** 2)
        x = sched.step(e, i, x)
    assert x.dtype == torch.float64
    exact = start * ((C2 + sig[-1] ** 2) / (C2 + sig[0] ** 2)) ** 0.5
    return abs(float(x) - exact)


def test_convergence_order():
    Ns = (10, 20, 40, 80)
    err_e = [_final_error(SM.EulerDiscrete, N) for N in Ns]
    err_m = [_final_error(SM.DpmSolverPP2M, N) for N in Ns]
    ord_e = [float(np.log2(err_e[i] / err_e[i + 1])) for i in range(3)]
    ord_m = [float(np.log2(err_m[i] / err_m[i + 1])) for i in range(3)]
    print("euler", err_e, ord_e)
    print("2m", err_m, ord_m)
    assert all(o > 1.5 for o in ord_m), ord_m                  # second order (theory: 2)
    assert all(o < 1.25 for o in ord_e), ord_e                 # first order (theory: 1)
    assert all(m < e for m, e in zip(err_m, err_e))


# ---- schedules ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [SM.EulerDiscrete, SM.DpmSolverPP2M])
@pytest.mark.parametrize("n,start", [(25, 0), (25, 10), (6, 0), (1, 0)])
def test_trailing_schedule_is_eulers(cls, n, start):
    ref = SM.EulerDiscrete().set_timesteps(n, start) if start else SM.EulerDiscrete().set_timesteps(n)
    s = cls().set_timesteps(n, start, sigmas="trailing")
    assert s.sigmas.dtype == np.float32 and s.timesteps.dtype == np.float32
    assert np.array_equal(s.sigmas, ref.sigmas) and np.array_equal(s.timesteps, ref.timesteps) and s.init_noise_sigma == ref.init_noise_sigma
    # and those are the known answers of tests/test_sampler_cpu.py: trailing spacing, sigma_max of the scaled-linear schedule
    _, _, ts, sig = MR.schedule(n, (n - start) / n if start else 1.0)
    assert np.array_equal(s.timesteps, ts.astype(np.float32)) and np.array_equal(s.sigmas, sig.astype(np.float32))


@pytest.mark.parametrize("cls", [SM.EulerDiscrete, SM.DpmSolverPP2M])
@pytest.mark.parametrize("n", [2, 6, 25, 50])
def test_karras_schedule(cls, n):
    s = cls().set_timesteps(n, sigmas="karras")
    sig, ts = s.sigmas, s.timesteps
    assert sig.dtype == np.float32 and ts.dtype == np.float32 and len(sig) == n + 1 and len(ts) == n
    assert bool((np.diff(sig.astype(np.float64)) < 0).all()) and sig[-1] == 0.0
    assert sig[0] == np.float32(s.sigmas_all[999]) and sig[-2] == np.float32(s.sigmas_all[0])
    assert s.init_noise_sigma == float(sig[0])
    assert bool((np.diff(ts.astype(np.float64)) < 0).all()) and ts[0] <= 999.0 and ts[-1] >= 0.0
    assert ts[0] == 999.0 and ts[-1] == 0.0
    # eq. 5 of Karras et al. and the fractional timesteps, restated (fp64 -> fp32: half an ulp each way plus the power's few fp64 ulps)
    _, _, rts, rsig = MR.schedule(n, 1.0, "karras")
    np.testing.assert_allclose(sig.astype(np.float64), rsig, rtol=2 * U24, atol=0)
    np.testing.assert_allclose(ts.astype(np.float64), rts, rtol=0, atol=999 * 2 * U24 + 1e-6)
    # from the middle of the schedule (img2img): the tail of the full one
    k = SM.EulerDiscrete().set_timesteps(n, n // 2, "karras")
    assert np.array_equal(k.sigmas, sig[n // 2:]) and np.array_equal(k.timesteps, ts[n // 2:])


def test_unknown_schedule_kind():
    with pytest.raises(ValueError, match="sigmas"):
        SM.EulerDiscrete().set_timesteps(5, sigmas="exponential")


# ---- table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trailing", "karras"])
@pytest.mark.parametrize("n,start", [(25, 0), (25, 10), (6, 3), (1, 0)])
def test_step_table_ms(kind, n, start):
    s = SM.DpmSolverPP2M(prediction_type="v_prediction").set_timesteps(n, start, kind)
    tab = SM.step_table_ms(s, 7.5)
    k = n - start
    assert tab.shape == (2 + k, 8) and tab.dtype == torch.float32
    base = SM.step_table_img(SM.EulerDiscrete(prediction_type="v_prediction").set_timesteps(n, start, kind), 7.5)
    assert torch.equal(tab[:, :4], base) and float(tab[0, 1]) == float(s.sigmas[0])               # header rows and columns 0..3: step_table_img's
    assert bool((tab[:2, 4:] == 0).all()) and bool((tab[:, 7] == 0).all())
    co = s.coeffs
    assert co.dtype == np.float64 and co.shape == (k, 3)
    np.testing.assert_allclose(co.sum(1), 1.0, rtol=0, atol=8 * 2.0 ** -53 * np.abs(co).sum(1).max())   # a + b + c = 1: a constant denoiser is a fixed point
    assert torch.equal(tab[2:, 4:7], torch.from_numpy(co.astype(np.float32)))                      # rounded once
    assert float(tab[2, 6]) == 0.0 and co[0, 2] == 0.0                                             # the first step that runs (of an img2img table too)
    assert s.sigmas[-1] == 0.0 and float(tab[2 + k - 1, 6]) == 0.0 and co[-1, 2] == 0.0            # the step to sigma = 0
    assert co[-1].tolist() == [0.0, 1.0, 0.0]
    if k > 2:
        assert bool((co[1:-1, 2] < 0).all()) and bool((tab[3:-1, 6] != 0).all())                   # second order in between
    np.testing.assert_allclose(co, MR.coefficients(s.sigmas), rtol=1e-12, atol=1e-14)              # the paper's exp / expm1 form


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
LIP = 1.0 / 32                 # |d eps / d xin| of the stub


class _Stub:
    """A UNet stand-in whose prediction depends on its input, the timestep and the call: eps = E[call] + tanh(xin) / 32 + t / 4000, in the dtype of its input."""

    def __init__(self, h, w, seed, calls=12):
        self.cfg, self.arena = dict(cross_dim=8, addition=False), None
        g = torch.Generator().manual_seed(seed)
        self.E = [torch.randn(2, 4, h, w, generator=g) for _ in range(calls)]
        self.calls = 0

    def model(self, xin, t):
        self.calls += 1
        return self.E[self.calls - 1].to(xin.dtype) + torch.tanh(xin) * LIP + t / 4000.0

    def forward(self, x, t, ctx, pooled, tid, *, B, H, W):
        xin = x[:, :4].float().view(B, H, W, 4).permute(0, 3, 1, 2)
        assert torch.equal(xin[0::2], xin[1::2]) and bool((t == t[0]).all())
        return self.model(xin, float(t[0])).permute(0, 2, 3, 1).reshape(B * H * W, 4).contiguous()


EMB = (torch.zeros(1, 77, 8), torch.zeros(1, 77, 8), None, None)
CASES = dict(txt2img=dict(), img2img=dict(strength=0.6), masked=dict(strength=0.6, masked=True))


def _case(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    noise, x0 = torch.randn(1, 4, h, w, generator=g), 0.8 * torch.randn(1, 4, h, w, generator=g)
    mask = (torch.rand(1, 1, h, w, generator=g) * 3).floor() / 2                     # 0, 0.5 and 1
    return noise, x0, mask


def _stub_sampler(h, w, pred="epsilon", seed=7):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=MR.emu_ms)
    stub = _Stub(h, w, seed)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


def _rounding_bound(steps, strength, kind, pred, g, mx, me):
    """How far an fp32 evaluation of the multistep loop can drift from the fp64 one, as a running worst case in the maximum norm (u = 2^-24; mx, me: the
    largest |x| and |model output| on the fp64 path).  Per step, with err the error carried in x and errp the one in the previous D:
      model input   x / sqrt(..) or x * (1 / sqrt(..)): 3 roundings                       ei   = inv (err + 3 u mx)
      model         Lipschitz LIP in its input, ~6 fp32 operations                         em   = LIP ei + 6 u me
      guidance      e = en + g (ep - en): 3 operations, |e| <= (1 + 2 g) me               ee   = (1 + 2 g) em + 3 u (1 + 2 g) me
      D             epsilon: x - s e (2 operations + the rounding of s)                    ed   = err + s ee + 3 u (mx + s (1 + 2 g) me)
                    v: e c1 + x / q, |c1| < 1 (3 operations + 4 for c1, q)                 ed   = ee + err / q + 7 u ((1 + 2 g) me + mx / q)
      update        a x + b D + c D_prev: 5 operations + 3 coefficient roundings           err' = |a| err + |b| ed + |c| errp + 8 u (|a| mx + (|b| + |c|) md)
      mask          k + m (x - k), k = x0 + noise s: 4 operations on magnitudes <= 2 mx    err' += 6 u 2 mx."""
    _, _, _, sig = MR.schedule(steps, strength, kind)
    sig = sig.astype(np.float32).astype(np.float64)
    co = MR.coefficients(sig)
    G = 1 + 2 * g
    md = mx + sig[0] * G * me
    err, errp = 2 * U24 * mx, 0.0
    for i in range(len(sig) - 1):
        s = sig[i]
        inv = 1 / np.sqrt(s * s + 1)
        ei = inv * (err + 3 * U24 * mx)
        em = LIP * ei + 6 * U24 * me
        ee = G * em + 3 * U24 * G * me
        if pred == "epsilon":
            ed = err + s * ee + 3 * U24 * (mx + s * G * me)
        else:
            q = s * s + 1
            ed = ee + err / q + 7 * U24 * (G * me + mx / q)
        a, b, c = np.abs(co[i])
        err, errp = a * err + b * ed + c * errp + 8 * U24 * (a * mx + (b + c) * md) + 12 * U24 * mx, ed
    return err


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", ["trailing", "karras"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_paths_against_fp64_reference_loop(pred, kind, case, fused):
    h, w, steps, g = 8, 12, 10, 8.0
    noise, x0, mask = _case(h, w)
    kw = dict(CASES[case])
    img = dict(init_latents=x0, strength=kw["strength"], mask=mask if kw.get("masked") else None) if kw else {}
    smp, stub = _stub_sampler(h, w, pred)
    got = smp.sample(EMB, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=fused, sampler="dpmpp_2m", sigmas=kind, **img)
    ref_stub = _Stub(h, w, 7)
    xs = []

    def model(xin, t):
        out = ref_stub.model(xin, t)
        xs.append((float(xin.abs().max()), float(out.abs().max())))
        return out

    ref = MR.sample_loop(model, noise, steps, sigmas=kind, guidance_scale=g, prediction_type=pred, **img)
    assert ref.dtype == torch.float64 and stub.calls == ref_stub.calls == (6 if kw else 10)
    mx = max(float(ref.abs().max()), float((x0.abs() + 14.7 * noise.abs()).max()))                 # |x| never exceeds its noised start on this path
    me = max(o for _, o in xs)
    bound = _rounding_bound(steps, kw.get("strength", 1.0), kind, pred, g, mx, me)
    err = float((got.double() - ref).abs().max())
    print(f"{pred} {kind} {case} fused={fused}: err {err:.3e} bound {bound:.3e} max|x| {float(ref.abs().max()):.3f}")
    assert bound < 2.0 ** -8 * mx                                                                  # a worst case, yet well below the scale of the latents
    assert err <= bound
    assert got.dtype == torch.float32 and not torch.equal(got, x0)
    # the solver is not Euler on the same levels: the two differ by far more than rounding
    eul = MR.sample_loop(_Stub(h, w, 7).model, noise, steps, sampler="euler", sigmas=kind, guidance_scale=g, prediction_type=pred, **img)
    assert float((eul - ref).abs().max()) > 10 * bound


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["trailing", "karras"])
def test_zero_mask_returns_init_latents(kind, fused):
    h, w = 8, 12
    noise, x0, _ = _case(h, w, 1)
    for strength in (0.5, 1.0):
        smp, _ = _stub_sampler(h, w)
        out = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, sampler="dpmpp_2m", sigmas=kind, init_latents=x0, strength=strength,
                         mask=torch.zeros(1, 1, h, w))
        assert torch.equal(out, x0), (kind, fused, strength)


def test_fused_equals_torch_loop_inputs_and_euler_untouched():
    """The default call is what it was whether or not a multistep call came before it on the same sampler, and Euler on Karras levels runs on the Euler kernels."""
    h, w = 8, 8
    noise, x0, mask = _case(h, w, 2)
    for fused in (False, True):
        smp, _ = _stub_sampler(h, w)
        plain = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused)
        smp.unet.calls = 0
        ms = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, sampler="dpmpp_2m")
        smp.unet.calls = 0
        assert torch.equal(smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused), plain) and not torch.equal(ms, plain)
        smp.unet.calls = 0
        assert torch.equal(smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, sampler="euler", sigmas="trailing"), plain)
        smp.unet.calls = 0
        ek = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, sigmas="karras")
        ref = MR.sample_loop(_Stub(h, w, 7).model, noise, 6, sampler="euler", sigmas="karras")
        assert not torch.equal(ek, plain) and float((ek.double() - ref).abs().max()) <= 2.0 ** -14 * 14.7 * float(noise.abs().max())


def test_argument_errors():
    h, w = 8, 8
    noise, x0, mask = _case(h, w)
    smp, _ = _stub_sampler(h, w)
    for fused in (False, True):
        with pytest.raises(ValueError, match="sampler"):
            smp.sample(EMB, h, w, steps=4, latents=noise, fused=fused, sampler="nope")
        with pytest.raises(ValueError, match="sigmas"):
            smp.sample(EMB, h, w, steps=4, latents=noise, fused=fused, sigmas="nope")
    # an op table without the multistep kernel: the fused path refuses instead of falling back; the torch loop runs
    from tests.img2img_ref import emu_img
    smp2 = SM.LatentSampler(unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=emu_img), _Stub(h, w, 7))
    with pytest.raises(NotImplementedError, match="sampler_step_ms"):
        smp2.sample(EMB, h, w, steps=4, latents=noise, fused=True, sampler="dpmpp_2m")
    assert smp2.sample(EMB, h, w, steps=4, latents=noise, sampler="dpmpp_2m").shape == (1, 4, h, w)


def test_cli_argument_errors(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--sampler", "heun"], "--sampler"), (["--sigmas", "exponential"], "--sigmas")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err


# ---- the entry point refuses bad arguments before it launches anything (no GPU involved) -------------------------------------------
def test_entry_point_validation():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert lib.sdlt_sampler_step_ms(None, None) == -1 and b"sdlt_sampler_step_ms" in lib.sdlt_last_error()
    ok = dict(eps=0x1000, x=0x2000, x0=0x3000, noise=0x4000, mask=0x5000, dprev=0xa000, xin=0x6000, ld_xin=64, timesteps=0x7000, table=0x8000, ctr=0x9000,
              n=1, hw=35, table_rows=5, init=0)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(n=0), SHAPE), (dict(hw=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE), (dict(table_rows=2), SHAPE),
                         (dict(x=None), SHAPE), (dict(xin=None), SHAPE), (dict(timesteps=None), SHAPE), (dict(table=None), SHAPE), (dict(ctr=None), SHAPE),
                         (dict(eps=None), SHAPE), (dict(dprev=None), SHAPE), (dict(x0=None), SHAPE), (dict(noise=None), SHAPE),   # a step with a mask reads both
                         (dict(init=1, noise=None), SHAPE),
                         (dict(x0=0x2000), SHAPE), (dict(init=1, noise=0x2000), SHAPE), (dict(dprev=0x2000), SHAPE), (dict(dprev=0x3000), SHAPE),
                         (dict(ld_xin=2), ALIGN), (dict(ld_xin=66), ALIGN), (dict(xin=0x6004), ALIGN), (dict(eps=0x1008), ALIGN),
                         (dict(x=0x2002), ALIGN), (dict(mask=0x5001), ALIGN), (dict(x0=0x3002), ALIGN), (dict(noise=0x4001), ALIGN), (dict(dprev=0xa002), ALIGN)):
        p = _lib.SamplerMsParams(**dict(ok, **change))
        assert lib.sdlt_sampler_step_ms(C.byref(p), None) == code, change
        assert b"sdlt_sampler_step_ms" in lib.sdlt_last_error()
