"""Adaptive projected guidance without a GPU: sampler.apg_table, the contract (tests/apg_ref.guidance_apg) against the published function
in fp64, the identities that define the three controls, the running average and its restart at step row 0, LatentSampler.sample(apg=) on the emulated op
table - torch loop == fused with every sampler family, mask, regions and windows; the launch list without it; two trajectories in a row - the entry
point's refusals, the command line, and render() end to end on the synthetic stack."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import apg_ref as AR
from tests import guidance_ref as GR
from tests import region_ref as RR
from tests import tilediff_ref as TD
from tests.test_hires_cpu import _resize_planes
from tests.test_multistep_cpu import CASES, EMB, _case, _Stub
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)
from tests.test_region_cpu import _regions
from tests.test_sampler_sequence_cpu import recording
from tests.test_tilediff_cpu import _embeds, _unet

FAMILIES = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")
APG = (0.0, 15.0, -0.5)
emu_window = AR.with_apg(TD.emu_table(GR.emu_guidance), "emu_apg_window")
emu_window.resize_planes = _resize_planes
emu_region = AR.with_apg(RR.emu_table(GR.emu_guidance), "emu_apg_region")


def _sched(k):
    return SM.EulerDiscrete().set_timesteps(k)


def _pair(n, hw, seed, spread=0.12):
    """eps fp32 [2n hw, 4]: a negative prediction and a positive one close to it, as a UNet's two rows are."""
    g = torch.Generator().manual_seed(seed)
    en = torch.randn(n, 1, hw, 4, generator=g) * 1.1 + 0.05
    return torch.cat([en, en + spread * torch.randn(n, 1, hw, 4, generator=g)], 1).reshape(2 * n * hw, 4).contiguous()


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def test_apg_table_known_answers():
    s = _sched(4)
    tab = SM.apg_table(s, (0.25, 15, -0.5))
    assert tab.dtype == torch.float32 and tab.tolist() == [[4.0, 0, 0, 0]] + [[0.25, 15.0, -0.5, 0.0]] * 4
    assert torch.equal(SM.apg_table(s, [0.25, 15.0, -0.5], 4), tab) and torch.equal(SM.apg_table(None, (0.25, 15, -0.5), 4), tab)
    rows = [(0.0, 15.0, -0.5), (0.5, 0.0, 0.0), (1.0, 2.5, 0.75)]
    tab = SM.apg_table(s, rows, 3)                                               # one tuple per step that runs (img2img: fewer than the schedule's)
    assert tab.tolist() == [[3.0, 0, 0, 0]] + [list(r) + [0.0] for r in rows]
    assert SM.apg_table(s, (1, 0, 0), 1).tolist() == [[1.0, 0, 0, 0], [1.0, 0.0, 0.0, 0.0]]
    assert float(SM.apg_table(s, (0.3, 0.1, -0.9))[1, 0]) == float(np.float32(0.3))


@pytest.mark.parametrize("bad,msg", [((-0.1, 15, -0.5), "eta"), ((1.5, 15, -0.5), "eta"), ((float("nan"), 15, 0), "eta"), ((0, -1.0, 0), "norm_threshold"),
                                     ((0, float("inf"), 0), "norm_threshold"), ((0, float("nan"), 0), "norm_threshold"), ((0, 15, 1.0), "momentum"),
                                     ((0, 15, -1.0), "momentum"), ((0, 15, 1.5), "momentum"), ((0, 15, float("nan")), "momentum"),
                                     ((0, 15), "three numbers"), (0.5, "three numbers"), ("apg", "three numbers"), ((0, 15, True), "three numbers"),
                                     ([(0, 15, -0.5)] * 3, "three numbers"), ([(0, 15, -0.5)] * 5, "three numbers"), ([(0, 15, -0.5)] * 3 + [(0, 15)], "three numbers"),
                                     ([(0, 15, -0.5)] * 3 + [(2.0, 15, 0)], "eta")])
def test_apg_table_refusals(bad, msg):
    with pytest.raises(ValueError, match=msg):
        SM.apg_table(_sched(4), bad)


# ---- the contract against the published function ---------------------------------------------------------------------------------------------
def _tabs(g, phi, apg, k=3):
    gtab, atab = torch.zeros(1 + k, 4), torch.zeros(1 + k, 4)
    gtab[0, 0] = atab[0, 0] = k
    gtab[1:, 0], gtab[1:, 1] = g, phi
    atab[1:, :3] = torch.tensor(apg)
    return gtab, atab


@pytest.mark.parametrize("apg", [(0.0, 0.0, 0.0), (0.3, 2.5, 0.0), (0.0, 15.0, -0.5), (1.0, 0.0, 0.4)])
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_contract_is_the_published_function(apg, phi):
    """Three steps in a row, fresh eps each, one running average: the contract (fp32, its sums in fp64) against normalized_guidance + MomentumBuffer
    + rescale_noise_cfg in fp64 on the same inputs.  The bar: the contract rounds at most 12 times per value (two for the running average per step, six
    from d to e_c, four in the blend), each rounding at most 2^-24 of an intermediate no larger than 2 max|e| + ..., and the rounded scalars c, a, r
    add 2^-24 each: 32 * 2^-24 max|e| holds all of it."""
    n, hw, g = 3, 35, 7.5
    gtab, atab = _tabs(g, phi, apg)
    a32 = tuple(float(v) for v in atab[1, :3])
    mom, m64 = torch.full((n * hw, 4), float("nan")), None
    for row in range(3):
        eps = _pair(n, hw, 100 + row, spread=0.12 if apg[1] != 2.5 else 0.4)
        e64 = eps.view(n, 2, hw, 4).double()
        want, m_new = AR.published(e64[:, 1], e64[:, 0], g, a32[0], a32[1], a32[2], m64)
        if phi:
            want = GR.rescale(e64[:, 1], want, float(np.float32(phi)))
        m64 = m_new if a32[2] != 0.0 else None
        got = AR.guidance_apg(eps.clone(), gtab, atab, mom, torch.tensor([row, 0], dtype=torch.int32), n).view(n, 2, hw, 4)
        assert got.dtype == torch.float32 and torch.equal(got[:, 0], got[:, 1]) and bool(torch.isfinite(got).all())
        assert float((got[:, 0].double() - want).abs().max()) <= 32 * 2.0 ** -24 * float(want.abs().max()), row
        if a32[2] != 0.0:
            assert float((mom.view(n, hw, 4).double() - m64).abs().max()) <= 8 * 2.0 ** -24 * float(m64.abs().max())
        else:
            assert bool(torch.isnan(mom).all())                                  # beta == 0: the buffer is not touched
    if apg[1] == 2.5:                                                            # (and the clip was active in that case)
        assert float(AR.scalars(*(lambda v: (v[:, 1] - v[:, 0], v[:, 1]))(eps.view(n, 2, -1)), 2.5)[0].max()) < 1.0


def test_identities_in_fp64():
    g64 = torch.Generator().manual_seed(3)
    ep = torch.randn(3, 4, 5, 7, generator=g64, dtype=torch.float64) * 1.3 + 0.2
    en = ep + 0.3 * torch.randn(3, 4, 5, 7, generator=g64, dtype=torch.float64)
    dot = lambda a, b: (a * b).sum(dim=(1, 2, 3))  # noqa: E731
    # (1, 0, 0) is classifier-free guidance
    out, _ = AR.published(ep, en, 7.5, 1.0, 0.0, 0.0)
    cfg = en + 7.5 * (ep - en)
    assert float((out - cfg).abs().max()) <= 1e-13 * float(cfg.abs().max())
    # eta = 0: the update is orthogonal to e_pos
    out, _ = AR.published(ep, en, 7.5, 0.0, 0.0, 0.0)
    upd = out - ep
    assert float((dot(upd, ep).abs() / (dot(upd, upd).sqrt() * dot(ep, ep).sqrt())).max()) <= 1e-13 and float(dot(upd, upd).min()) > 0.1
    # and eta interpolates the parallel part: out(eta) - out(0) = eta (out(1) - out(0))
    half, _ = AR.published(ep, en, 7.5, 0.5, 0.0, 0.0)
    assert float((half - out - 0.5 * (cfg - out)).abs().max()) <= 1e-13 * float(cfg.abs().max())
    # tau bounds the update's norm: |out - e_pos| <= (g - 1) tau at eta <= 1, with equality of |d| = tau where the clip is active
    norm = dot(ep - en, ep - en).sqrt()
    tau = float(norm.sort().values[1])                                           # active for one image, on the edge for one, idle for one
    out, _ = AR.published(ep, en, 7.5, 1.0, tau, 0.0)
    un = dot(out - ep, out - ep).sqrt() / 6.5
    assert float((un - torch.minimum(norm, torch.tensor(tau, dtype=torch.float64))).abs().max()) <= 1e-12 * tau
    assert int((norm > tau).sum()) == 1 and float(un.max()) <= tau * (1 + 1e-12)
    for eta in (0.0, 0.4):
        out, _ = AR.published(ep, en, 7.5, eta, tau, 0.0)
        assert float(dot(out - ep, out - ep).sqrt().max()) <= 6.5 * tau * (1 + 1e-12)
    # the contract has them too (fp32): neutral values are CFG within rounding, not bit for bit
    eps = _pair(3, 35, 5)
    gtab, atab = _tabs(7.5, 0.0, (1.0, 0.0, 0.0))
    ctr = torch.zeros(2, dtype=torch.int32)
    a = AR.guidance_apg(eps.clone(), gtab, atab, None, ctr, 3)
    b = GR.guidance(eps.clone(), gtab, ctr, 3)
    assert float((a - b).abs().max()) <= 8 * 2.0 ** -24 * float(b.abs().max()) and not torch.equal(a, b)


def test_momentum_over_four_steps_and_the_restart():
    n, hw, g, beta = 2, 35, 7.5, -0.5
    gtab, atab = _tabs(g, 0.0, (1.0, 0.0, beta), k=4)
    es = [_pair(n, hw, 40 + i) for i in range(4)]
    ds = [(e.view(n, 2, -1)[:, 1] - e.view(n, 2, -1)[:, 0]) for e in es]
    hand = [ds[0] + beta * torch.zeros_like(ds[0])]
    for i in range(1, 4):
        hand.append(ds[i] + beta * hand[-1])                                     # fp32, the contract's two roundings per step
    outs = {}
    for fill in ("nan", "0", "3"):                                               # whatever the buffer holds before row 0
        mom = torch.full((n * hw, 4), float(fill))
        outs[fill] = []
        for i in range(4):
            e = AR.guidance_apg(es[i].clone(), gtab, atab, mom, torch.tensor([i, 9], dtype=torch.int32), n)
            assert torch.equal(mom.view(n, -1), hand[i]), i
            outs[fill].append(e)
    for fill in ("0", "3"):
        assert all(torch.equal(a, b) for a, b in zip(outs[fill], outs["nan"]))
    # the fp64 recursion: m_3 = d_3 - d_2 / 2 + d_1 / 4 - d_0 / 8
    m3 = ds[3].double() - ds[2].double() / 2 + ds[1].double() / 4 - ds[0].double() / 8
    assert float((hand[3].double() - m3).abs().max()) <= 4 * 2.0 ** -24 * float(m3.abs().max())
    # a g = 1 row in the middle passes e_pos through and leaves the buffer alone
    gtab[2, 0] = 1.0
    mom = torch.full((n * hw, 4), float("nan"))
    AR.guidance_apg(es[0].clone(), gtab, atab, mom, torch.tensor([0, 0], dtype=torch.int32), n)
    held = mom.clone()
    e = AR.guidance_apg(es[1].clone(), gtab, atab, mom, torch.tensor([1, 0], dtype=torch.int32), n).view(n, 2, -1)
    assert torch.equal(mom, held) and torch.equal(e[:, 0], es[1].view(n, 2, -1)[:, 1]) and torch.equal(e[:, 1], e[:, 0])


# ---- LatentSampler on the emulated op table ------------------------------------------------------------------------------------------------
def _stub_sampler(h, w, pred="epsilon", seed=7, ops=AR.emu_apg):
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
    controls = dict(guidance_scale=7.5, guidance_rescale=0.7, guidance_interval=(float(sig[-2]), float(sig[1])), apg=(0.0, 3.0, -0.5))
    out = {}
    for fused in (False, True):
        smp, stub = _stub_sampler(h, w, pred)
        out[fused] = smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=fused, **controls, **kw)
        assert stub.calls == k and out[fused].dtype == torch.float32 and bool(torch.isfinite(out[fused]).all())
        assert tuple(smp._fused["shapes"][(h, w)]["mom"].shape) == (h * w, 4) and tuple(smp._fused["atab"].shape) == tuple(smp._fused["gtab"].shape)
    assert torch.equal(out[False], out[True])                                    # bit for bit
    if case == "masked":
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(out[True][keep], x0[keep])
    # apg alone counts as guidance in use, every control changes the result, and the deterministic families follow the fp64 loop with the published
    # function.  The bar is tests/test_guidance_cpu.py's for these shapes (the multistep path's rounding bound stays below 2^-8 max|x|)
    smp, stub = _stub_sampler(h, w, pred)
    run = lambda **k2: (setattr(stub, "calls", 0), smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=True, **dict(kw, **k2)))[1]  # noqa: E731
    plain, alone = run(guidance_scale=7.5), run(guidance_scale=7.5, apg=(0.0, 3.0, -0.5))
    assert not torch.equal(alone, plain) and not torch.equal(alone, out[True])
    assert len({tuple(run(guidance_scale=7.5, apg=a).flatten().tolist()) for a in ((0.0, 3.0, -0.5), (0.5, 3.0, -0.5), (0.0, 1.0, -0.5), (0.0, 3.0, 0.0))}) == 4
    per_step = run(guidance_scale=7.5, apg=[(0.0, 3.0, -0.5)] * k)
    assert torch.equal(per_step, alone)
    if family in ("euler", "dpmpp_2m"):
        img = {k2: v for k2, v in kw.items() if k2 in ("init_latents", "strength", "mask")}
        a32 = tuple(float(np.float32(v)) for v in controls["apg"])
        ref = AR.sample_loop(_Stub(h, w, 7).model, noise, steps, sampler=family, apg=a32, guidance_scale=7.5, guidance_rescale=float(np.float32(0.7)),
                             guidance_interval=controls["guidance_interval"], prediction_type=pred, **img)
        mx = float((x0.abs() + 14.7 * noise.abs()).max())
        err = float((out[True].double() - ref).abs().max())
        print(family, pred, case, err, mx)
        assert err <= 2.0 ** -8 * mx


def _tiny(table, B):
    cfg, sd, lora, rt, unet = _unet("tiny15", B, table)
    smp = SM.LatentSampler(rt, unet, n_images=1)
    smp.set_lora_scale(0.75)
    return cfg, smp, _embeds(cfg, 5, 1)[0]


def test_with_windows_and_with_regions():
    """Guidance runs on the fused full-size prediction: the running average has the whole latent's size, and the torch loop gives the fused path's bits."""
    h, w, steps = 12, 20, 3
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(9))
    plan = SM.tile_plan(h, w, (8, 2))
    cfg, smp, em = _tiny(emu_window, 2 * plan.ty * plan.tx)
    run = lambda **kw: smp.sample(em, h, w, steps=steps, latents=noise.clone(), tile=(8, 2), **kw)  # noqa: E731
    a = run(fused=True, apg=APG, sampler="dpmpp_2m")
    assert torch.equal(a, run(apg=APG, sampler="dpmpp_2m")) and not torch.equal(a, run(fused=True, sampler="dpmpp_2m")) and bool(torch.isfinite(a).all())
    (sh,) = smp._fused["shapes"].values()
    assert tuple(sh["mom"].shape) == (h * w, 4) and tuple(sh["win"]["eps_full"].shape) == (2 * h * w, 4)
    cfg, smp, em = _tiny(emu_region, 2 * 3)
    rg = _regions(cfg)
    run = lambda **kw: smp.sample(em, h, w, steps=steps, latents=noise.clone(), regions=rg, seeds=[31], **kw)  # noqa: E731
    a = run(fused=True, apg=APG, guidance_rescale=0.5)
    assert torch.equal(a, run(apg=APG, guidance_rescale=0.5)) and not torch.equal(a, run(fused=True, guidance_rescale=0.5)) and bool(torch.isfinite(a).all())
    (sh,) = smp._fused["shapes"].values()
    assert tuple(sh["mom"].shape) == (h * w, 4)


@pytest.mark.parametrize("fused", [False, True])
def test_none_is_the_launch_list_as_before_and_a_missing_kernel_is_an_error(fused):
    h, w = 8, 8
    noise, _, _ = _case(h, w, 2)
    assert not hasattr(GR.emu_guidance, "guidance_apg")
    logs, outs = [], []
    for extra in ({}, dict(apg=None)):
        for kw in (dict(guidance_scale=7.5), dict(guidance_scale=7.5, guidance_rescale=0.5)):
            seen = []
            smp, _ = _stub_sampler(h, w, ops=recording(GR.emu_guidance, seen))
            outs.append(smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, **kw, **extra))
            logs.append(list(seen))
            assert smp._apg_graphs == {} and "atab" not in smp._fused and all("mom" not in sh for sh in smp._fused["shapes"].values())
    assert logs[0] == logs[2] and logs[1] == logs[3] and torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert "guidance" not in logs[0] and logs[1].count("guidance") == 4
    smp, stub = _stub_sampler(h, w, ops=GR.emu_guidance)
    with pytest.raises(NotImplementedError, match="sdlt_guidance_apg"):
        smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, apg=APG)
    assert stub.calls == 0 and smp._fused is None                                # refused before anything is built
    # with the op: one guidance_apg per step where guidance would be, and no guidance launch
    seen = []
    smp, _ = _stub_sampler(h, w, ops=recording(AR.emu_apg, seen))
    smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, guidance_rescale=0.5, apg=APG)
    assert [("guidance_apg" if nm == "guidance" else nm) for nm in logs[1]] == seen and seen.count("guidance_apg") == 4
    for bad in ((2.0, 15, 0), (0, -1, 0), (0, 15, 1), [(0, 15, 0)] * 3):
        with pytest.raises(ValueError, match="apg"):
            smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, apg=bad)


@pytest.mark.parametrize("fused", [False, True])
def test_second_trajectory_restarts_the_running_average(fused):
    """Two sample() calls in a row on one sampler: the second gives the bits a fresh sampler's first call gives, though the buffer still holds the
    first trajectory's average - and a poisoned buffer changes nothing either."""
    h, w = 8, 12
    noise, _, _ = _case(h, w, 4)

    def call(smp, stub, sampler):
        stub.calls = 0
        return smp.sample(EMB, h, w, steps=5, latents=noise.clone(), fused=fused, sampler=sampler, apg=(0.0, 3.0, -0.5), **(dict(seeds=[3]) if sampler in SM.SDE_KINDS else {}))

    for sampler in ("euler", "dpmpp_2m_sde"):
        smp, stub = _stub_sampler(h, w)
        first = call(smp, stub, sampler)
        mom = smp._fused["shapes"][(h, w)]["mom"]
        assert bool(torch.isfinite(mom).all()) and float(mom.abs().max()) > 0
        assert torch.equal(call(smp, stub, sampler), first)
        mom.fill_(float("nan"))
        assert torch.equal(call(smp, stub, sampler), first) and bool(torch.isfinite(mom).all())
        fresh, stub2 = _stub_sampler(h, w)
        assert torch.equal(call(fresh, stub2, sampler), first)


# ---- the entry point refuses bad arguments before it launches anything (no GPU involved) -----------------------------------------------
def test_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_guidance_apg" in _lib.SYMBOLS and C.sizeof(_lib.GuidanceApgParams) == 56
    assert lib.sdlt_guidance_apg(None, None) == -1 and b"sdlt_guidance_apg" in lib.sdlt_last_error()
    hw = 35
    ok = dict(eps=0x10000, gtab=0x2000, atab=0x4000, mom=0x20000, ctr=0x3000, n=2, hw=hw, gtab_rows=5)
    SHAPE, ALIGN = -1, -2
    img = 2 * hw * 16                                                            # bytes of mom; eps is twice that
    for change, code in ((dict(eps=None), SHAPE), (dict(gtab=None), SHAPE), (dict(atab=None), SHAPE), (dict(ctr=None), SHAPE), (dict(n=0), SHAPE), (dict(n=-1), SHAPE),
                         (dict(hw=0), SHAPE), (dict(hw=-3), SHAPE), (dict(gtab_rows=1), SHAPE), (dict(gtab_rows=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE),
                         (dict(eps=0x10008), ALIGN), (dict(eps=0x10004), ALIGN), (dict(mom=0x20008), ALIGN), (dict(mom=0x20004), ALIGN), (dict(gtab=0x2002), ALIGN),
                         (dict(atab=0x4002), ALIGN), (dict(ctr=0x3001), ALIGN),
                         (dict(mom=0x10000), SHAPE), (dict(mom=0x10000 + 2 * img - 16), SHAPE), (dict(mom=0x10000 - img + 16), SHAPE), (dict(mom=0x10000 + img), SHAPE)):
        p = _lib.GuidanceApgParams(**dict(ok, **change))
        assert lib.sdlt_guidance_apg(C.byref(p), None) == code, change
        assert b"sdlt_guidance_apg" in lib.sdlt_last_error()


# ---- the command line and render() -------------------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--apg-eta", "0.5"], "need --apg"), (["--apg-norm-threshold", "10"], "need --apg"), (["--apg-momentum", "-0.25"], "need --apg"),
                       (["--apg", "--apg-eta", "1.5"], "eta"), (["--apg", "--apg-eta", "-0.5"], "eta"), (["--apg", "--apg-norm-threshold", "-1"], "norm_threshold"),
                       (["--apg", "--apg-momentum", "1"], "momentum"), (["--apg", "--apg-momentum", "-1.5"], "momentum"), (["--apg", "--apg-eta", "much"], "--apg-eta"),
                       (["--apg", "--apg-eta"], "--apg-eta")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    import unittest.mock as mock
    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert "apg" not in seen                                                 # without the flag: the call as before
        R.main(base + ["--apg"])
        assert seen["apg"] == (0.0, 15.0, -0.5) == R.APG_DEFAULT
        R.main(base + ["--apg", "--apg-eta", "0.25", "--apg-momentum", "0"])
        assert seen["apg"] == (0.25, 15.0, 0.0)
        R.main(base + ["--apg", "--apg-norm-threshold", "7.5", "--guidance-rescale", "0.5"])
        assert seen["apg"] == (0.0, 7.5, -0.5) and seen["guidance_rescale"] == 0.5
    assert R.apg_args(None) is None and R.apg_args(False) is None and R.apg_args(True) == R.APG_DEFAULT
    assert R.apg_args([1, 2, 0]) == (1.0, 2.0, 0.0) and R.apg_args(dict(momentum=-0.25)) == (0.0, 15.0, -0.25)
    for bad, msg in (((0, 15), "apg takes"), (dict(beta=1), "unknown"), ((2, 15, 0), "eta"), ("on", "apg takes"), (1.0, "apg takes")):
        with pytest.raises(ValueError, match=msg):
            R.apg_args(bad)


def test_render_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    """--apg end to end on the synthetic stack: the files, prompts.json, a picture that differs from the plain one, both passes of a hires render, with
    --tile-diffusion, and an op table without the launch."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    config, ckdir = job
    calls = []
    real_sample = SM.LatentSampler.sample
    monkeypatch.setattr(SM.LatentSampler, "sample", lambda self, em, h, w, **kw: (calls.append((h, w, kw.get("apg"), kw.get("tile"))), real_sample(self, em, h, w, **kw))[1])
    rt = lambda table=emu_window: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--steps", "3", "--seed", "5", "--size", "32", "32"]
    plain, apg = tmp_path / "plain", tmp_path / "apg"
    R.main(common + ["--out", str(plain)], runtime=rt())
    R.main(common + ["--apg", "--apg-norm-threshold", "2", "--out", str(apg)], runtime=rt())
    assert calls == [(8, 8, None, None), (8, 8, (0.0, 2.0, -0.5), None)]
    name = next(f for f in sorted(os.listdir(apg)) if f.startswith("img_00"))
    assert sorted(os.listdir(apg)) == sorted(os.listdir(plain)) and Image.open(apg / name).size == (32, 32)
    assert open(plain / name, "rb").read() != open(apg / name, "rb").read()
    assert np.isfinite(np.asarray(Image.open(apg / name), dtype=np.float64)).all()
    meta = json.load(open(apg / "prompts.json"))
    assert meta["apg"] == dict(eta=0.0, norm_threshold=2.0, momentum=-0.5) and "apg" not in json.load(open(plain / "prompts.json"))
    # render() takes True, the three numbers or a dict; hires: both passes carry it; with windows in the second
    del calls[:]
    ld = R.load_for_inference(ckdir, runtime=rt())
    R.render(ld, ["a house"], str(tmp_path / "h"), size=(32, 32), steps=2, apg=dict(norm_threshold=2.0), hires=dict(size=(80, 48), strength=0.5), tile_diffusion=(8, 2),
             sampler="dpmpp_2m", guidance_rescale=0.5)
    assert calls == [(8, 8, (0.0, 2.0, -0.5), None), (12, 20, (0.0, 2.0, -0.5), (8, 2))]
    assert json.load(open(tmp_path / "h" / "prompts.json"))["apg"]["norm_threshold"] == 2.0
    R.render(ld, ["a house"], str(tmp_path / "t"), size=(32, 32), steps=2, apg=True)
    assert json.load(open(tmp_path / "t" / "prompts.json"))["apg"] == dict(eta=0.0, norm_threshold=15.0, momentum=-0.5)
    # refused before anything is built: bad values, and an op table without the kernel
    with pytest.raises(ValueError, match="momentum"):
        R.render(ld, ["a house"], str(tmp_path / "none"), size=(32, 32), steps=2, apg=(0, 15, 1.0))
    with pytest.raises(NotImplementedError, match="sdlt_guidance_apg"):
        R.main(common + ["--apg", "--out", str(tmp_path / "none")], runtime=rt(TD.emu_table(GR.emu_guidance)))
    assert not os.path.exists(tmp_path / "none")
