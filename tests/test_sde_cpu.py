"""The stochastic samplers (Euler ancestral, DPM-Solver++ (2M) SDE) without a GPU: the Philox generator and the noise it defines, sampler.sde_coefficients
against the published loops of tests/sde_ref.py, the eta = 0 limits, the table, the variance the samplers reach on Gaussian data, and
LatentSampler.sample(sampler="euler_a" | "dpmpp_2m_sde") - torch loop and fused path on the emulated op table with the restated kernels - and the
argument errors."""
import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import multistep_ref as MR
from tests import sde_ref as SR
from tests.test_multistep_cpu import CASES, EMB, _case, _Stub

KINDS = ("euler_a", "dpmpp_2m_sde")
CLS = dict(euler_a=SM.EulerAncestral, dpmpp_2m_sde=SM.DpmSolverPP2MSDE)


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, want):
    """Random123's known-answer vectors for philox4x32-10."""
    assert " ".join(f"{int(v):08x}" for v in SR.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("seed,step", [(1234, 3), (0, 0), (2 ** 32 - 1, 999)])
def test_noise_moments(seed, step):
    """2^20 normals of one (seed, step): mean and standard deviation within 5 standard errors (measured: <= 0.55 and <= 1.23), all finite - the
    uniforms never reach 0 or 1 - and |z| below sqrt(-2 ln 2^-24) = 5.77."""
    z = SR.noise(seed, step, 2 ** 18).reshape(-1)
    N = z.size
    m, s = abs(z.mean()) * N ** 0.5, abs(z.std() - 1.0) * (2 * N) ** 0.5
    print(seed, step, m, s, abs(z).max())
    assert N == 2 ** 20 and np.isfinite(z).all() and abs(z).max() < 5.77
    assert m <= 5.0 and s <= 5.0
    # another step, another seed and the high seed word each give other numbers; the four channels of a pixel are four different numbers
    a = SR.noise(seed, step, 64)
    assert not np.array_equal(a, SR.noise(seed, step + 1, 64)) and not np.array_equal(a, SR.noise(seed + 1, step, 64))
    assert not np.array_equal(a, SR.noise(seed + 2 ** 32, step, 64)) and len(np.unique(a)) == a.size
    assert np.array_equal(a, SR.noise(seed, step, 128)[:, :64])                 # a pixel's noise does not depend on the image's size


def test_seed_words():
    w = SM.seed_words([0, 1, 2 ** 32, 2 ** 64 - 1, -1, 0x0123456789ABCDEF], 6)
    assert w.dtype == torch.int32 and tuple(w.shape) == (6, 2)
    assert SR._seeds_of(w) == [0, 1, 2 ** 32, 2 ** 64 - 1, 2 ** 64 - 1, 0x0123456789ABCDEF]
    for bad in ([1], [1, 2, 3], [1.0, 2]):
        with pytest.raises(ValueError, match="seeds"):
            SM.seed_words(bad, 2)
    g = SM.seed_words(None, 3, torch.Generator().manual_seed(5))
    assert tuple(g.shape) == (3, 2) and torch.equal(g, SM.seed_words(None, 3, torch.Generator().manual_seed(5))) and len(set(SR._seeds_of(g))) == 3


# ---- coefficients ------------------------------------------------------------------------------------------------------------------------
C2 = 0.64


def _denoiser(x, s):
    """The exact denoiser of N(0, 0.8^2 I) data plus a bounded nonlinear part: the trajectory is not a product of scalars."""
    return x * (C2 / (C2 + s * s)) + 0.1 * torch.tanh(x)


@pytest.mark.parametrize("steps", [1, 2, 7])
@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_coefficients_against_published_loops(kind, eta, sigkind, steps):
    """x_{i+1} = a x + b D_i + c D_{i-1} + d z (the scheduler class on sde_coefficients) against k-diffusion's loops as published, both in fp64 on
    the same grid and noise: they differ by fp64 algebra only."""
    sig = SM.EulerDiscrete().set_timesteps(steps, 0, sigkind).sigmas.astype(np.float64)
    assert len(sig) == steps + 1 and sig[-1] == 0.0
    g = torch.Generator().manual_seed(steps)
    x0 = torch.randn(64, generator=g, dtype=torch.float64) * float(sig[0])
    zs = [torch.randn(64, generator=g, dtype=torch.float64) for _ in range(steps)]
    for grid in (sig, sig[:-1]) if steps > 1 else (sig,):                       # to sigma = 0, and stopping at the last positive level
        sched = CLS[kind](eta=eta).set_sigmas(grid)
        assert sched.sigmas.dtype == np.float64 and sched.coeffs.dtype == np.float64 and sched.coeffs.shape == (len(grid) - 1, 4)
        x, peak = x0, float(x0.abs().max())
        for i in range(len(grid) - 1):
            s = float(grid[i])
            x = sched.step((x - _denoiser(x, s)) / s, i, x, zs[i])
            peak = max(peak, float(x.abs().max()))
        ref = SR.published_loop(kind, lambda x, i: _denoiser(x, float(grid[i])), x0, grid, eta, zs)
        assert x.dtype == ref.dtype == torch.float64
        err = float((x - ref).abs().max())
        print(kind, eta, sigkind, steps, len(grid), err / peak)
        assert err <= 1e-12 * peak
        if eta == 1.0 and len(grid) > 2:                                        # and the noise matters: without it the end point is elsewhere
            ref0 = SR.published_loop(kind, lambda x, i: _denoiser(x, float(grid[i])), x0, grid, eta, [torch.zeros_like(z) for z in zs])
            assert float((ref - ref0).abs().max()) > 1e-3


@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
@pytest.mark.parametrize("n,start", [(25, 0), (7, 3), (2, 0), (1, 0)])
def test_eta_zero_is_the_deterministic_sampler(sigkind, n, start):
    sig = SM.EulerDiscrete().set_timesteps(n, start, sigkind).sigmas
    for grid in (sig, sig.astype(np.float64)):
        co = SM.sde_coefficients(grid, "dpmpp_2m_sde", 0.0)
        assert co.dtype == np.float64 and np.array_equal(co[:, :3], SM.ms_coefficients(grid)) and np.array_equal(co[:, 3], np.zeros(len(grid) - 1))
        s64 = np.asarray(grid, dtype=np.float64)
        a = s64[1:] / s64[:-1]
        assert np.array_equal(SM.sde_coefficients(grid, "euler_a", 0.0), np.stack([a, 1.0 - a, np.zeros_like(a), np.zeros_like(a)], 1))
    # the classes carry eta to their coefficients
    assert np.array_equal(SM.DpmSolverPP2MSDE(eta=0.0).set_timesteps(n, start, sigkind).coeffs[:, :3], SM.DpmSolverPP2M().set_timesteps(n, start, sigkind).coeffs)


def test_coefficient_argument_errors():
    sig = [3.0, 1.0, 0.0]
    for eta in (-1e-9, -1.0, float("nan")):
        for kind in KINDS:
            with pytest.raises(ValueError, match="eta"):
                SM.sde_coefficients(sig, kind, eta)
    with pytest.raises(ValueError, match="kind"):
        SM.sde_coefficients(sig, "heun", 1.0)
    assert SM.SAMPLERS == ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")
    for kind in KINDS:                                                           # the default is eta = 1
        assert np.array_equal(SM.sde_coefficients(sig, kind), SM.sde_coefficients(sig, kind, 1.0)) and CLS[kind]().eta == 1.0


# ---- table and classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
@pytest.mark.parametrize("n,start", [(25, 0), (25, 10), (6, 3), (1, 0)])
def test_step_table_sde(kind, sigkind, n, start):
    s = CLS[kind](prediction_type="v_prediction", eta=0.7).set_timesteps(n, start, sigkind)
    tab = SM.step_table_sde(s, 7.5)
    k = n - start
    assert tab.shape == (2 + k, 8) and tab.dtype == torch.float32
    ref = SM.EulerDiscrete(prediction_type="v_prediction").set_timesteps(n, start, sigkind)
    assert np.array_equal(s.sigmas, ref.sigmas) and np.array_equal(s.timesteps, ref.timesteps) and s.init_noise_sigma == ref.init_noise_sigma
    assert torch.equal(tab[:, :4], SM.step_table_img(ref, 7.5)) and bool((tab[:2, 4:] == 0).all())          # step_table_ms's layout, column 7 = d
    co = s.coeffs
    assert co.dtype == np.float64 and co.shape == (k, 4)
    assert torch.equal(tab[2:, 4:8], torch.from_numpy(co.astype(np.float32)))                               # rounded once
    assert co[0, 2] == 0.0 and float(tab[2, 6]) == 0.0                                                      # first order on the first step that runs
    assert co[-1].tolist() == [0.0, 1.0, 0.0, 0.0] and tab[2 + k - 1, 4:].tolist() == [0.0, 1.0, 0.0, 0.0]   # the step to sigma = 0: x = D, no noise
    if k > 1:
        assert bool((co[:-1, 3] > 0).all()) and bool((tab[2:-1, 7] > 0).all()) and bool((co[:-1, 0] > 0).all())
    if k > 2:
        second = kind == "dpmpp_2m_sde"
        assert bool((co[1:-1, 2] < 0).all()) == second and bool((co[1:-1, 2] == 0).all()) != second
    if kind == "euler_a":
        np.testing.assert_allclose(co[:, 0] + co[:, 1], 1.0, rtol=0, atol=2.0 ** -52)                       # a constant denoiser is a fixed point of the mean
    # the variance an exact-noise state keeps: from sigma^2 I at a constant D the ancestral step lands on sigma_next^2 I, (a sigma)^2 + d^2 = sigma_next^2
    if kind == "euler_a":
        sig = s.sigmas.astype(np.float64)
        np.testing.assert_allclose((co[:, 0] * sig[:-1]) ** 2 + co[:, 3] ** 2, sig[1:] ** 2, rtol=1e-12, atol=0)


# ---- Gaussian data: the variance the sampler reaches --------------------------------------------------------------------------------------
def _final_variance(kind, N, eta=1.0, s_min=0.002, s_max=14.6146):
    """Data N(0, C2): the exact denoiser is linear, D = kappa(sigma) x, kappa = C2 / (C2 + sigma^2), so x stays Gaussian and its variance follows
    x_{i+1} = (a + b kappa_i) x_i + c kappa_{i-1} x_{i-1} + d z exactly: a recursion on the covariance of (x_i, x_{i-1}), started from the exact
    marginal C2 + sigma_0^2.  The grid is uniform in log sigma down to s_min = 0.002, then the step to 0, whose own bias (x = kappa x: about s_min^2 =
    4e-6) lies far below the discretisation error at every N used here."""
    sig = np.concatenate([np.exp(np.linspace(np.log(s_max), np.log(s_min), N)), [0.0]])
    co = SM.sde_coefficients(sig, kind, eta)
    kap = C2 / (C2 + sig ** 2)
    v11, v12, v22, kprev = C2 + sig[0] ** 2, 0.0, 0.0, 0.0
    for i in range(N):
        a, b, c, d = co[i]
        p, q = a + b * kap[i], c * kprev
        v11, v12, v22 = p * p * v11 + 2 * p * q * v12 + q * q * v22 + d * d, p * v11 + q * v12, v11
        kprev = kap[i]
    return v11


@pytest.mark.parametrize("kind", KINDS)
def test_variance_on_gaussian_data_converges(kind):
    err = [abs(_final_variance(kind, N) - C2) for N in (20, 40, 80, 160)]
    print(kind, err)
    assert all(b < a for a, b in zip(err, err[1:])), err                         # strictly smaller at each doubling; no rate asserted
    assert err[-1] < 0.1 * C2
    # without the noise (eta = 0) the same recursion is the deterministic sampler's: it converges to the same variance
    det = [abs(_final_variance(kind, N, eta=0.0) - C2) for N in (20, 160)]
    assert det[1] < det[0]


# ---- LatentSampler on the emulated op table -----------------------------------------------------------------------------------------------
def _stub_sampler(h, w, pred="epsilon", seed=7, ops=SR.emu_sde):
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=ops)
    stub = _Stub(h, w, seed)
    return SM.LatentSampler(rt, stub, prediction_type=pred), stub


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("kind", KINDS)
def test_torch_loop_equals_fused(kind, pred, sigkind, case):
    h, w, steps, g, seed = 8, 12, 10, 8.0, 0x1234567ABCDEF
    noise, x0, mask = _case(h, w)
    kw = dict(CASES[case])
    img = dict(init_latents=x0, strength=kw["strength"], mask=mask if kw.get("masked") else None) if kw else {}
    out = {}
    for fused in (False, True):
        smp, stub = _stub_sampler(h, w, pred)
        out[fused] = smp.sample(EMB, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=fused, sampler=kind, sigmas=sigkind, seeds=[seed], **img)
        assert stub.calls == (6 if kw else 10) and out[fused].dtype == torch.float32 and bool(torch.isfinite(out[fused]).all())
    assert torch.equal(out[False], out[True])                                    # bit for bit
    if kw.get("masked"):
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(out[True][keep], x0[keep]) and not torch.equal(out[True][~keep], x0[~keep])
    # the published loop in fp64 on the same noise (the emulated kernel's z is the fp64 reference rounded to fp32): fp32 rounding apart.  The bar:
    # the multistep path's worst-case rounding bound on these shapes stays below 2^-8 max|x| (tests/test_multistep_cpu.py); one more term does not
    # change its order, and a wrong coefficient or a noise term on the wrong side of the mask blend is wrong by far more
    k = 6 if kw else 10
    zs = [torch.from_numpy(SR.noise(seed, i, h * w)).view(1, 4, h, w) for i in range(k)]
    ref = SR.sample_loop(_Stub(h, w, 7).model, noise, steps, zs, sampler=kind, sigmas=sigkind, guidance_scale=g, prediction_type=pred, **img)
    mx = float((x0.abs() + 14.7 * noise.abs()).max())
    err = float((out[True].double() - ref).abs().max())
    print(kind, pred, sigkind, case, err, mx)
    assert err <= 2.0 ** -8 * mx
    # another seed, and eta, change the result; the same seed repeats it
    smp, _ = _stub_sampler(h, w, pred)
    run = lambda **k2: (setattr(smp.unet, "calls", 0), smp.sample(EMB, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=True, sampler=kind,  # noqa: E731
                                                                  sigmas=sigkind, **img, **k2))[1]
    assert torch.equal(run(seeds=[seed]), out[True]) and not torch.equal(run(seeds=[seed + 1]), out[True]) and not torch.equal(run(seeds=[seed], eta=0.5), out[True])


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sigkind", ["trailing", "karras"])
def test_eta_zero_equals_dpmpp_2m(sigkind, case):
    """eta = 0: the multistep table with d = 0, so the fused path gives sdlt_sampler_step_ms's bits, and Euler ancestral is Euler's update."""
    h, w = 8, 12
    noise, x0, mask = _case(h, w, 3)
    kw = dict(CASES[case])
    img = dict(init_latents=x0, strength=kw["strength"], mask=mask if kw.get("masked") else None) if kw else {}
    smp, stub = _stub_sampler(h, w)
    run = lambda **k2: (setattr(stub, "calls", 0), smp.sample(EMB, h, w, steps=10, latents=noise.clone(), fused=True, sigmas=sigkind, **img, **k2))[1]  # noqa: E731
    ms = run(sampler="dpmpp_2m")
    assert torch.equal(run(sampler="dpmpp_2m_sde", eta=0.0, seeds=[1]), ms) and torch.equal(run(sampler="dpmpp_2m_sde", eta=0.0, seeds=[2]), ms)
    assert not torch.equal(run(sampler="dpmpp_2m_sde", eta=1.0, seeds=[1]), ms)
    stub.calls = 0
    loop = smp.sample(EMB, h, w, steps=10, latents=noise.clone(), sigmas=sigkind, sampler="dpmpp_2m_sde", eta=0.0, seeds=[1], **img)
    assert torch.equal(loop, ms)
    eul = MR.sample_loop(_Stub(h, w, 7).model, noise, 10, sampler="euler", sigmas=sigkind, **img)
    ea = run(sampler="euler_a", eta=0.0, seeds=[1])
    assert float((ea.double() - eul).abs().max()) <= 2.0 ** -14 * 14.7 * float(noise.abs().max())          # the bar tests/test_multistep_cpu.py holds Euler on Karras levels to


def test_seeds_from_the_generator_and_defaults_untouched():
    h, w = 8, 8
    noise, x0, mask = _case(h, w, 2)
    for fused in (False, True):
        smp, stub = _stub_sampler(h, w)
        plain = smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused)
        outs = []
        for seed in (11, 11, 12):                                                # seeds=None: drawn from the generator
            stub.calls = 0
            outs.append(smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused, sampler="euler_a", generator=torch.Generator().manual_seed(seed)))
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
        stub.calls = 0
        assert torch.equal(smp.sample(EMB, h, w, steps=6, latents=noise.clone(), fused=fused), plain)       # the default call is what it was


def test_argument_errors():
    h, w = 8, 8
    noise, x0, mask = _case(h, w)
    smp, _ = _stub_sampler(h, w)
    for fused in (False, True):
        with pytest.raises(ValueError, match="sampler"):
            smp.sample(EMB, h, w, steps=4, latents=noise, fused=fused, sampler="dpmpp_sde")
        for kind in KINDS:
            with pytest.raises(ValueError, match="eta"):
                smp.sample(EMB, h, w, steps=4, latents=noise, fused=fused, sampler=kind, eta=-0.5)
            with pytest.raises(ValueError, match="seeds"):
                smp.sample(EMB, h, w, steps=4, latents=noise, fused=fused, sampler=kind, seeds=[1, 2])
    # an op table without the kernel: the fused path refuses instead of falling back, and so does the torch loop - its noise is the kernel's
    smp2, _ = _stub_sampler(h, w, ops=MR.emu_ms)
    for kind in KINDS:
        with pytest.raises(NotImplementedError, match="sampler_step_sde"):
            smp2.sample(EMB, h, w, steps=4, latents=noise, fused=True, sampler=kind)
        with pytest.raises(NotImplementedError, match="sampler_step_sde"):
            smp2.sample(EMB, h, w, steps=4, latents=noise, sampler=kind)
    assert smp2.sample(EMB, h, w, steps=4, latents=noise, fused=True, sampler="dpmpp_2m").shape == (1, 4, h, w)


def test_cli_argument_errors(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--eta", "0.5"], "--eta"), (["--sampler", "dpmpp_2m", "--eta", "1"], "--eta"), (["--sampler", "euler", "--eta", "0"], "--eta"),
                       (["--sampler", "euler_a", "--eta", "-0.1"], "--eta"), (["--sampler", "dpmpp_2m_sde", "--eta", "much"], "--eta"),
                       (["--sampler", "dpmpp_sde"], "--sampler")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    for extra in (["--sampler", "euler_a"], ["--sampler", "dpmpp_2m_sde", "--eta", "0.5", "--sigmas", "karras"]):   # accepted: fails later, on the checkpoint
        with pytest.raises(Exception) as e:
            R.main(base + extra)
        assert not isinstance(e.value, SystemExit), extra


# ---- the entry points refuse bad arguments before they launch anything (no GPU involved) ------------------------------------------------
def test_entry_point_validation():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.SamplerSdeParams) == C.sizeof(_lib.SamplerMsParams) + 8
    assert lib.sdlt_sampler_step_sde(None, None) == -1 and b"sdlt_sampler_step_sde" in lib.sdlt_last_error()
    ok = dict(eps=0x1000, x=0x2000, x0=0x3000, noise=0x4000, mask=0x5000, dprev=0xa000, xin=0x6000, ld_xin=64, timesteps=0x7000, table=0x8000, ctr=0x9000,
              n=1, hw=35, table_rows=5, init=0, seeds=0xb000)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(seeds=None), SHAPE), (dict(seeds=None, mask=None, x0=None, noise=None), SHAPE), (dict(seeds=0xb002), ALIGN), (dict(seeds=0xb001), ALIGN),
                         (dict(n=0), SHAPE), (dict(hw=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE), (dict(table_rows=2), SHAPE),
                         (dict(x=None), SHAPE), (dict(xin=None), SHAPE), (dict(timesteps=None), SHAPE), (dict(table=None), SHAPE), (dict(ctr=None), SHAPE),
                         (dict(eps=None), SHAPE), (dict(dprev=None), SHAPE), (dict(x0=None), SHAPE), (dict(noise=None), SHAPE),
                         (dict(init=1, noise=None), SHAPE),
                         (dict(x0=0x2000), SHAPE), (dict(init=1, noise=0x2000), SHAPE), (dict(dprev=0x2000), SHAPE), (dict(dprev=0x3000), SHAPE),
                         (dict(ld_xin=2), ALIGN), (dict(ld_xin=66), ALIGN), (dict(xin=0x6004), ALIGN), (dict(eps=0x1008), ALIGN),
                         (dict(x=0x2002), ALIGN), (dict(mask=0x5001), ALIGN), (dict(x0=0x3002), ALIGN), (dict(noise=0x4001), ALIGN), (dict(dprev=0xa002), ALIGN)):
        p = _lib.SamplerSdeParams(**dict(ok, **change))
        assert lib.sdlt_sampler_step_sde(C.byref(p), None) == code, change
        assert b"sdlt_sampler_step_sde" in lib.sdlt_last_error()
    for args, code in (((None, 0, 1, 35, 0x2000), SHAPE), ((0x1000, 0, 1, 35, None), SHAPE), ((0x1000, 0, 0, 35, 0x2000), SHAPE), ((0x1000, 0, 1, 0, 0x2000), SHAPE),
                       ((0x1000, -1, 1, 35, 0x2000), SHAPE), ((0x1000, 0, 1 << 15, 1 << 14, 0x2000), SHAPE), ((0x1002, 0, 1, 35, 0x2000), ALIGN),
                       ((0x1000, 0, 1, 35, 0x2001), ALIGN)):
        assert lib.sdlt_sampler_noise(*args, None) == code, args
        assert b"sdlt_sampler_noise" in lib.sdlt_last_error()
