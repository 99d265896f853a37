"""Dynamic thresholding without a GPU: sampler.dyn_table, the contract (tests/dynthresh_ref.contract) against the same mathematics in fp64
with torch.quantile, the identities that define the three controls, LatentSampler.sample(dynthresh=) on the emulated op table - torch loop == fused with
every sampler family, mask, regions and windows; the launch list without it - the entry point's refusals, the refusals with apg and rescale, the command
line, and render() end to end on the synthetic stack."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from tests import apg_ref as AR
from tests import dynthresh_ref as DR
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
DYN = (3.0, 0.97, 1.0)
emu_window = DR.with_dyn(TD.emu_table(GR.emu_guidance), "emu_dyn_window")
emu_window.resize_planes = _resize_planes
emu_region = DR.with_dyn(RR.emu_table(GR.emu_guidance), "emu_dyn_region")


def _sched(k):
    return SM.EulerDiscrete().set_timesteps(k)


def _pair(n, hw, seed, spread=0.12, mean=0.05):
    """eps fp32 [2n hw, 4]: a negative prediction and a positive one close to it, as a UNet's two rows are."""
    g = torch.Generator().manual_seed(seed)
    en = torch.randn(n, 1, hw, 4, generator=g) * 1.1 + mean
    return torch.cat([en, en + spread * torch.randn(n, 1, hw, 4, generator=g)], 1).reshape(2 * n * hw, 4).contiguous()


def _tabs(g, dyn, k=3):
    gtab, dtab = torch.zeros(1 + k, 4), torch.zeros(1 + k, 4)
    gtab[0, 0] = dtab[0, 0] = k
    gtab[1:, 0] = g
    dtab[1:, :3] = torch.tensor(dyn)
    return gtab, dtab


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def test_dyn_table_known_answers():
    s = _sched(4)
    tab = SM.dyn_table(s, (7, 0.75, 0.5))
    assert tab.dtype == torch.float32 and tab.tolist() == [[4.0, 0, 0, 0]] + [[7.0, 0.75, 0.5, 0.0]] * 4
    assert torch.equal(SM.dyn_table(s, [7.0, 0.75, 0.5], 4), tab) and torch.equal(SM.dyn_table(None, (7, 0.75, 0.5), 4), tab)
    rows = [(7.0, 0.75, 1.0), (1.0, 1.0, 0.0), (5.5, 0.5, 0.25)]
    tab = SM.dyn_table(s, rows, 3)                                               # one tuple per step that runs (img2img: fewer than the schedule's)
    assert tab.tolist() == [[3.0, 0, 0, 0]] + [list(r) + [0.0] for r in rows]
    assert SM.dyn_table(s, (1, 1, 0), 1).tolist() == [[1.0, 0, 0, 0], [1.0, 1.0, 0.0, 0.0]]
    assert float(SM.dyn_table(s, (7, 0.999, 1))[1, 1]) == float(np.float32(0.999))


@pytest.mark.parametrize("bad,msg", [((0.5, 0.99, 1), "mimic"), ((float("inf"), 0.99, 1), "mimic"), ((float("nan"), 0.99, 1), "mimic"), ((-7, 0.99, 1), "mimic"),
                                     ((7, 0.0, 1), "percentile"), ((7, -0.1, 1), "percentile"), ((7, 1.5, 1), "percentile"), ((7, float("nan"), 1), "percentile"),
                                     ((7, 0.99, -0.1), "interpolate"), ((7, 0.99, 1.5), "interpolate"), ((7, 0.99, float("nan")), "interpolate"),
                                     ((7, 0.99), "three numbers"), (7.0, "three numbers"), ("dyn", "three numbers"), ((7, 0.99, True), "three numbers"),
                                     ([(7, 0.99, 1)] * 3, "three numbers"), ([(7, 0.99, 1)] * 5, "three numbers"), ([(7, 0.99, 1)] * 3 + [(7, 0.99)], "three numbers"),
                                     ([(7, 0.99, 1)] * 3 + [(0.0, 0.99, 1)], "mimic")])
def test_dyn_table_refusals(bad, msg):
    with pytest.raises(ValueError, match=msg):
        SM.dyn_table(_sched(4), bad)


# ---- the contract against the same mathematics in fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [1, 2, 35, 351, 4097])
@pytest.mark.parametrize("dyn", [(7.0, 0.999, 1.0), (3.0, 0.5, 1.0), (5.0, 1.0, 0.25), (2.0, 0.01, 0.6), (4.0, 0.9, 1.0)])
def test_contract_is_the_published_mathematics(dyn, hw):
    """The quantile is the derivable part: Q lies between the two exact order statistics, and within |v_hi - v_lo| hw 2^-23 + 2^-23 |v_hi| of
    torch.quantile in fp64 on the contract's own fp32 deviations (fp32 `pos` against torch's own position - at most (hw - 1) 2^-24 q apart, times the
    gap - plus the interpolation's roundings).  Where the fp32 position rounds onto or across an integer that torch's fp64 position has not reached
    (q = 0.9f at hw = 351: 315.0 against 314.9999917), the two interpolate in neighbouring brackets; Q is continuous and piecewise linear in the position,
    so the same formula holds with v_lo, v_hi spanning both brackets - which is what is asserted; where the brackets agree it is the formula as it stands.
    The prediction: every value passes at most 12 roundings of intermediates no larger than 2 max|e_g|, and a
    threshold off by dS moves a value by at most A dS / S (|clamp| <= S): 32 * 2^-24 max|e_g| + 2 dQ holds all of it (A <= S)."""
    n, g = 3, 12.0
    gtab, dtab = _tabs(g, dyn)
    mimic, q, psi = (float(v) for v in dtab[1, :3])
    eps = _pair(n, hw, 100 + hw)
    e = eps.view(n, 2, hw, 4)
    p = DR.parts(e[:, 0].numpy(), e[:, 1].numpy(), np.float32(g), np.float32(mimic), np.float32(q))
    srt = np.sort(np.abs(p["cg"]), axis=1)
    lo, hi, w = DR.ranks(q, hw)
    assert 0 <= lo <= hi <= hw - 1 and hi - lo <= 1 and 0.0 <= float(w) < 1.0
    assert np.array_equal(p["v_lo"][:, 0], srt[:, lo]) and np.array_equal(p["v_hi"][:, 0], srt[:, hi])
    assert bool((p["Q"] >= p["v_lo"]).all()) and bool((p["Q"] <= p["v_hi"]).all())
    tq = torch.quantile(torch.from_numpy(np.abs(p["cg"])).double(), q, dim=1, keepdim=True).numpy()
    lo64 = min(int(np.floor(q * (hw - 1))), hw - 1)                             # torch's own bracket: q (the fp32 value) times hw - 1 in fp64
    v_lo, v_hi = srt[:, min(lo, lo64)][:, None].astype(np.float64), srt[:, max(hi, min(lo64 + 1, hw - 1))][:, None].astype(np.float64)
    assert abs(lo64 - lo) <= 1
    bound = np.abs(v_hi - v_lo) * hw * 2.0 ** -23 + 2.0 ** -23 * np.abs(v_hi)
    assert bool((np.abs(p["Q"] - tq) <= bound).all()), float((np.abs(p["Q"] - tq) - bound).max())
    got = DR.contract(eps.clone(), gtab, dtab, torch.tensor([1, 0], dtype=torch.int32), n).view(n, 2, hw, 4)
    assert got.dtype == torch.float32 and torch.equal(got[:, 0], got[:, 1]) and bool(torch.isfinite(got).all())
    e64 = e.double().permute(0, 1, 3, 2)                                         # [n, 2, 4, hw]: channels second, as the loop's NCHW
    want = DR.published(e64[:, 1], e64[:, 0], g, mimic, q, psi).permute(0, 2, 1)
    tol = 32 * 2.0 ** -24 * float(np.abs(p["eg"]).max()) + 2 * float(bound.max())
    assert float((got[:, 0].double() - want).abs().max()) <= tol


def test_identities():
    n, hw, g = 3, 351, 12.0
    eps = _pair(n, hw, 7)
    e = eps.view(n, 2, hw, 4)
    ctr = torch.tensor([0, 0], dtype=torch.int32)
    eg = (e[:, 0] + np.float32(g) * (e[:, 1] - e[:, 0]))
    # mimic == g with q = 1: A = Q = S = max |c_g|, the clamp is idle and (c_g / S) S + mu_g is e_g to within a few ulps of S (or of e_g where larger)
    out = DR.contract(eps.clone(), *_tabs(g, (g, 1.0, 1.0)), ctr, n).view(n, 2, hw, 4)[:, 0]
    p = DR.parts(e[:, 0].numpy(), e[:, 1].numpy(), np.float32(g), np.float32(g), np.float32(1.0))
    assert np.array_equal(p["A"], p["Q"]) and np.array_equal(p["A"], p["S"])
    assert float((out - eg).abs().max()) <= 4 * 2.0 ** -23 * max(float(p["S"].max()), float(eg.abs().max())) and not torch.equal(out, eg)
    # a g == 1 row returns e_pos bit for bit
    out = DR.contract(eps.clone(), *_tabs(1.0, (7.0, 0.99, 1.0)), ctr, n).view(n, 2, hw, 4)
    assert torch.equal(out[:, 0], e[:, 1]) and torch.equal(out[:, 1], e[:, 1])
    # psi = 0 returns e_g bit for bit
    out = DR.contract(eps.clone(), *_tabs(g, (3.0, 0.99, 0.0)), ctr, n).view(n, 2, hw, 4)[:, 0]
    assert torch.equal(out, eg)
    # psi = 1: no value of a channel is further from the guided mean than A (the division by S gives at most 1, the product at most A; the last sum
    # rounds once: half an ulp of e)
    for dyn in ((3.0, 0.99, 1.0), (7.0, 0.5, 1.0), (2.0, 1.0, 1.0)):
        out = DR.contract(eps.clone(), *_tabs(g, dyn), ctr, n).view(n, 2, hw, 4)[:, 0]
        p = DR.parts(e[:, 0].numpy(), e[:, 1].numpy(), np.float32(g), np.float32(dyn[0]), np.float32(dyn[1]))
        dev = np.abs(out.numpy().astype(np.float64) - p["mu_g"]).max(1, keepdims=True)
        assert bool((dev <= p["A"] + 2.0 ** -24 * np.abs(out.numpy()).max()).all()) and not torch.equal(out, eg)
        assert bool((np.abs(p["cg"]).max(1, keepdims=True) > p["A"]).all())              # (every channel's range was in fact reduced)
    # interpolate blends: psi = 0.5 lies halfway
    a = DR.contract(eps.clone(), *_tabs(g, (3.0, 0.99, 1.0)), ctr, n).view(n, 2, hw, 4)[:, 0]
    h = DR.contract(eps.clone(), *_tabs(g, (3.0, 0.99, 0.5)), ctr, n).view(n, 2, hw, 4)[:, 0]
    assert float((h - (0.5 * a + 0.5 * eg)).abs().max()) <= 4 * 2.0 ** -24 * float(eg.abs().max())
    # a constant channel: S == 0 there, e = e_g, finite
    flat = eps.clone().view(n, 2, hw, 4)
    flat[:, :, :, 2] = 0.25
    out = DR.contract(flat.reshape(-1, 4).contiguous(), *_tabs(g, (3.0, 0.99, 1.0)), ctr, n).view(n, 2, hw, 4)[:, 0]
    assert bool(torch.isfinite(out).all()) and bool((out[:, :, 2] == 0.25).all())


# ---- LatentSampler on the emulated op table ------------------------------------------------------------------------------------------------
def _stub_sampler(h, w, pred="epsilon", seed=7, ops=DR.emu_dyn):
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
    controls = dict(guidance_scale=12.0, guidance_interval=(float(sig[-2]), float(sig[1])), dynthresh=DYN)
    out = {}
    for fused in (False, True):
        smp, stub = _stub_sampler(h, w, pred)
        out[fused] = smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=fused, **controls, **kw)
        assert stub.calls == k and out[fused].dtype == torch.float32 and bool(torch.isfinite(out[fused]).all())
        assert tuple(smp._fused["dtab"].shape) == tuple(smp._fused["gtab"].shape) and smp._fused["dtab"][1, :3].tolist() == [float(np.float32(v)) for v in DYN]
    assert torch.equal(out[False], out[True])                                    # bit for bit
    if case == "masked":
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(out[True][keep], x0[keep])
    # dynthresh alone counts as guidance in use, every control changes the result, per-step tuples and per-step scales work
    smp, stub = _stub_sampler(h, w, pred)
    run = lambda **k2: (setattr(stub, "calls", 0), smp.sample(EMB, h, w, steps=steps, latents=noise.clone(), fused=True, **dict(kw, **k2)))[1]  # noqa: E731
    plain, alone = run(guidance_scale=12.0), run(guidance_scale=12.0, dynthresh=DYN)
    assert not torch.equal(alone, plain) and not torch.equal(alone, out[True])
    assert len({tuple(run(guidance_scale=12.0, dynthresh=d).flatten().tolist()) for d in (DYN, (5.0, 0.97, 1.0), (3.0, 0.5, 1.0), (3.0, 0.97, 0.5))}) == 4
    assert torch.equal(run(guidance_scale=12.0, dynthresh=[DYN] * k), alone)
    assert torch.equal(run(guidance_scale=[12.0] * k, dynthresh=DYN), alone)
    assert torch.equal(run(guidance_scale=12.0, dynthresh=(3.0, 0.97, 0.0)), run(guidance_scale=[12.0] * k))      # psi = 0 is the plain pre-pass's e_g, bit for bit
    if family in ("euler", "dpmpp_2m"):
        # the deterministic families follow the fp64 loop.  The bar is tests/test_guidance_cpu.py's for these shapes (2^-8 max|x|)
        img = {k2: v for k2, v in kw.items() if k2 in ("init_latents", "strength", "mask")}
        d32 = tuple(float(np.float32(v)) for v in DYN)
        ref = DR.sample_loop(_Stub(h, w, 7).model, noise, steps, sampler=family, dyn=d32, guidance_scale=12.0, guidance_interval=controls["guidance_interval"],
                             prediction_type=pred, **img)
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
    """The launch runs on the fused full-size prediction, and the torch loop gives the fused path's bits."""
    h, w, steps = 12, 20, 3
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(9))
    plan = SM.tile_plan(h, w, (8, 2))
    cfg, smp, em = _tiny(emu_window, 2 * plan.ty * plan.tx)
    run = lambda **kw: smp.sample(em, h, w, steps=steps, latents=noise.clone(), tile=(8, 2), guidance_scale=12.0, **kw)  # noqa: E731
    a = run(fused=True, dynthresh=DYN, sampler="dpmpp_2m")
    assert torch.equal(a, run(dynthresh=DYN, sampler="dpmpp_2m")) and not torch.equal(a, run(fused=True, sampler="dpmpp_2m")) and bool(torch.isfinite(a).all())
    (sh,) = smp._fused["shapes"].values()
    assert tuple(sh["win"]["eps_full"].shape) == (2 * h * w, 4)
    cfg, smp, em = _tiny(emu_region, 2 * 3)
    rg = _regions(cfg)
    run = lambda **kw: smp.sample(em, h, w, steps=steps, latents=noise.clone(), regions=rg, seeds=[31], guidance_scale=12.0, **kw)  # noqa: E731
    a = run(fused=True, dynthresh=DYN)
    assert torch.equal(a, run(dynthresh=DYN)) and not torch.equal(a, run(fused=True)) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("fused", [False, True])
def test_none_is_the_launch_list_as_before_and_a_missing_kernel_is_an_error(fused):
    h, w = 8, 8
    noise, _, _ = _case(h, w, 2)
    assert not hasattr(AR.emu_apg, "guidance_dyn")
    logs, outs = [], []
    for extra in ({}, dict(dynthresh=None)):
        for kw in (dict(guidance_scale=7.5), dict(guidance_scale=7.5, guidance_rescale=0.5), dict(guidance_scale=7.5, apg=(0.0, 3.0, -0.5))):
            seen = []
            smp, _ = _stub_sampler(h, w, ops=recording(AR.emu_apg, seen))
            outs.append(smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, **kw, **extra))
            logs.append(list(seen))
            assert smp._dyn_graphs == {} and "dtab" not in smp._fused
    assert logs[:3] == logs[3:] and all(torch.equal(a, b) for a, b in zip(outs[:3], outs[3:]))
    assert "guidance" not in logs[0] and logs[1].count("guidance") == 4 and logs[2].count("guidance_apg") == 4
    assert not any("guidance_dyn" in lg for lg in logs)
    smp, stub = _stub_sampler(h, w, ops=AR.emu_apg)
    with pytest.raises(NotImplementedError, match="sdlt_guidance_dyn"):
        smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=DYN)
    assert stub.calls == 0 and smp._fused is None                                # refused before anything is built
    # with the op: one guidance_dyn per step where guidance would be, and no guidance launch
    seen = []
    smp, _ = _stub_sampler(h, w, ops=recording(DR.emu_dyn, seen))
    smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=DYN)
    assert [("guidance_dyn" if nm == "guidance" else nm) for nm in logs[1]] == seen and seen.count("guidance_dyn") == 4
    for bad in ((0.5, 0.99, 1), (7, 0, 1), (7, 0.99, 2), [(7, 0.99, 1)] * 3):
        with pytest.raises(ValueError, match="dynthresh"):
            smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=bad)


@pytest.mark.parametrize("fused", [False, True])
def test_not_with_apg_and_not_with_rescale(fused):
    h, w = 8, 8
    noise, _, _ = _case(h, w, 2)
    table = AR.with_apg(DR.emu_dyn, "emu_dyn_apg")
    smp, stub = _stub_sampler(h, w, ops=table)
    with pytest.raises(ValueError, match="dynthresh.*apg"):
        smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=DYN, apg=(0.0, 15.0, -0.5))
    with pytest.raises(ValueError, match="dynthresh.*guidance_rescale"):
        smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=DYN, guidance_rescale=0.7)
    assert stub.calls == 0 and smp._fused is None
    assert bool(torch.isfinite(smp.sample(EMB, h, w, steps=4, latents=noise.clone(), fused=fused, dynthresh=DYN, guidance_rescale=0.0)).all())


def test_trajectory_has_a_defaulted_dyn_field():
    assert SM.Trajectory._fields[-1] == "dyn" and SM.Trajectory._field_defaults["dyn"] is None and SM.Trajectory._field_defaults["apg"] is None


# ---- the entry point refuses bad arguments before it launches anything (no GPU involved) -----------------------------------------------
def test_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_guidance_dyn" in _lib.SYMBOLS and C.sizeof(_lib.GuidanceDynParams) == 48
    assert lib.sdlt_guidance_dyn(None, None) == -1 and b"sdlt_guidance_dyn" in lib.sdlt_last_error()
    ok = dict(eps=0x10000, gtab=0x2000, dtab=0x4000, ctr=0x3000, n=2, hw=35, gtab_rows=5)
    SHAPE, ALIGN = -1, -2
    for change, code in ((dict(eps=None), SHAPE), (dict(gtab=None), SHAPE), (dict(dtab=None), SHAPE), (dict(ctr=None), SHAPE), (dict(n=0), SHAPE), (dict(n=-1), SHAPE),
                         (dict(hw=0), SHAPE), (dict(hw=-3), SHAPE), (dict(gtab_rows=1), SHAPE), (dict(gtab_rows=0), SHAPE), (dict(n=1 << 15, hw=1 << 14), SHAPE),
                         (dict(n=1, hw=(1 << 24) + 1), SHAPE), (dict(eps=0x10008), ALIGN), (dict(eps=0x10004), ALIGN), (dict(gtab=0x2002), ALIGN),
                         (dict(dtab=0x4002), ALIGN), (dict(dtab=0x4001), ALIGN), (dict(ctr=0x3001), ALIGN)):
        p = _lib.GuidanceDynParams(**dict(ok, **change))
        assert lib.sdlt_guidance_dyn(C.byref(p), None) == code, change
        assert b"sdlt_guidance_dyn" in lib.sdlt_last_error()


# ---- the command line and render() -------------------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--dynthresh-percentile", "0.9"], "need --dynthresh"), (["--dynthresh-interpolate", "0.5"], "need --dynthresh"),
                       (["--dynthresh", "0.5"], "mimic"), (["--dynthresh", "--dynthresh-percentile", "0"], "percentile"),
                       (["--dynthresh", "--dynthresh-percentile", "1.5"], "percentile"), (["--dynthresh", "--dynthresh-interpolate", "-1"], "interpolate"),
                       (["--dynthresh", "much"], "--dynthresh"), (["--dynthresh", "--dynthresh-percentile"], "--dynthresh-percentile"),
                       (["--dynthresh", "--apg"], "--apg"), (["--dynthresh", "--guidance-rescale", "0.7"], "--guidance-rescale")):
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
        assert "dynthresh" not in seen                                           # without the flag: the call as before
        R.main(base + ["--dynthresh"])
        assert seen["dynthresh"] == (7.0, 0.999, 1.0) == R.DYN_DEFAULT
        R.main(base + ["--dynthresh", "5", "--dynthresh-interpolate", "0.5"])
        assert seen["dynthresh"] == (5.0, 0.999, 0.5)
        R.main(base + ["--guidance", "14", "--dynthresh", "--dynthresh-percentile", "0.95"])
        assert seen["dynthresh"] == (7.0, 0.95, 1.0) and seen["guidance_scale"] == 14.0
    assert R.dynthresh_args(None) is None and R.dynthresh_args(False) is None and R.dynthresh_args(True) == R.DYN_DEFAULT
    assert R.dynthresh_args([5, 1, 0]) == (5.0, 1.0, 0.0) and R.dynthresh_args(dict(percentile=0.9)) == (7.0, 0.9, 1.0)
    for bad, msg in (((7, 0.99), "dynthresh takes"), (dict(q=1), "unknown"), ((0.5, 0.99, 1), "mimic"), ("on", "dynthresh takes"), (7.0, "dynthresh takes")):
        with pytest.raises(ValueError, match=msg):
            R.dynthresh_args(bad)


def test_render_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    """--dynthresh end to end on the synthetic stack: the files, prompts.json, a picture that differs from the plain one, both passes of a hires render,
    with --tile-diffusion, the refusals, and an op table without the launch."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    config, ckdir = job
    calls = []
    real_sample = SM.LatentSampler.sample
    monkeypatch.setattr(SM.LatentSampler, "sample", lambda self, em, h, w, **kw: (calls.append((h, w, kw.get("dynthresh"), kw.get("tile"))), real_sample(self, em, h, w, **kw))[1])
    rt = lambda table=emu_window: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--steps", "3", "--seed", "5", "--size", "32", "32", "--guidance", "14"]
    plain, dyn = tmp_path / "plain", tmp_path / "dyn"
    R.main(common + ["--out", str(plain)], runtime=rt())
    R.main(common + ["--dynthresh", "3", "--dynthresh-percentile", "0.9", "--out", str(dyn)], runtime=rt())
    assert calls == [(8, 8, None, None), (8, 8, (3.0, 0.9, 1.0), None)]
    name = next(f for f in sorted(os.listdir(dyn)) if f.startswith("img_00"))
    assert sorted(os.listdir(dyn)) == sorted(os.listdir(plain)) and Image.open(dyn / name).size == (32, 32)
    assert open(plain / name, "rb").read() != open(dyn / name, "rb").read()
    assert np.isfinite(np.asarray(Image.open(dyn / name), dtype=np.float64)).all()
    meta = json.load(open(dyn / "prompts.json"))
    assert meta["dynthresh"] == dict(mimic=3.0, percentile=0.9, interpolate=1.0) and "dynthresh" not in json.load(open(plain / "prompts.json"))
    # render() takes True, the three numbers or a dict; hires: both passes carry it; with windows in the second
    del calls[:]
    ld = R.load_for_inference(ckdir, runtime=rt())
    R.render(ld, ["a house"], str(tmp_path / "h"), size=(32, 32), steps=2, guidance_scale=14.0, dynthresh=dict(mimic=3.0), hires=dict(size=(80, 48), strength=0.5),
             tile_diffusion=(8, 2), sampler="dpmpp_2m")
    assert calls == [(8, 8, (3.0, 0.999, 1.0), None), (12, 20, (3.0, 0.999, 1.0), (8, 2))]
    assert json.load(open(tmp_path / "h" / "prompts.json"))["dynthresh"]["mimic"] == 3.0
    R.render(ld, ["a house"], str(tmp_path / "t"), size=(32, 32), steps=2, dynthresh=True)
    assert json.load(open(tmp_path / "t" / "prompts.json"))["dynthresh"] == dict(mimic=7.0, percentile=0.999, interpolate=1.0)
    # refused before anything is built: bad values, the alternatives, and an op table without the kernel
    with pytest.raises(ValueError, match="percentile"):
        R.render(ld, ["a house"], str(tmp_path / "none"), size=(32, 32), steps=2, dynthresh=(7, 0.0, 1.0))
    with pytest.raises(ValueError, match="dynthresh.*apg"):
        R.render(ld, ["a house"], str(tmp_path / "none"), size=(32, 32), steps=2, dynthresh=True, apg=True)
    with pytest.raises(ValueError, match="dynthresh.*guidance_rescale"):
        R.render(ld, ["a house"], str(tmp_path / "none"), size=(32, 32), steps=2, dynthresh=True, guidance_rescale=0.5)
    with pytest.raises(NotImplementedError, match="sdlt_guidance_dyn"):
        R.main(common + ["--dynthresh", "--out", str(tmp_path / "none")], runtime=rt(TD.emu_table(GR.emu_guidance)))
    assert not os.path.exists(tmp_path / "none")
