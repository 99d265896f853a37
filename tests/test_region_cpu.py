"""Regional prompts without a GPU: the region plan against its restatement (tests/region_ref.py) and known answers, blend32's rounding
bound, the identity that lets the prediction be fused before the step (fp64), the sampler on an emulated op table - paths, reference trajectory,
R = 1, two images, bootstrap - the refusals, the entry points' argument checks, render() on the emulated table, and the CLI."""
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops
from sd_lora_trainer_amd import sampler as SM
from tests import blur_ref as BR
from tests import diffdiff_ref as DR
from tests import guidance_ref as GR
from tests import region_ref as RR
from tests.test_hires_cpu import _resize_planes
from tests.test_img2img_cpu import EMB, _Stub
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)
from tests.test_tilediff_cpu import _embeds, _unet

emu_plain = GR.emu_guidance                                   # every sampler family and the guidance pre-pass, no region launches
emu_region = RR.emu_table(emu_plain)
emu_region.resize_planes = _resize_planes
emu_region.sampler_step_dd = DR.sampler_step_dd               # (the launch with a hold map: a change map with regions)
emu_region.blur_planes, emu_region.blur_taps = BR.blur_planes, ops.blur_taps      # (--region-feather)

H, W = 12, 20


def soft_masks(h=H, w=W):
    """Two soft foreground masks that overlap each other and leave some pixels to the background alone."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    a = torch.sigmoid((w * 0.45 - xs) * 0.9) * torch.sigmoid((ys - 1.5) * 2.0)
    b = torch.sigmoid((xs - w * 0.4) * 0.7) * torch.sigmoid((h - 2.5 - ys) * 2.0)
    return torch.stack([a, b]).clamp_(0.0, 1.0)


def hard_masks(h=H, w=W):
    m = torch.zeros(2, h, w)
    m[0, 2:9, 1:8] = 1.0
    m[1, 4:11, 11:19] = 1.0
    return m


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def test_plan_known_answers():
    # two disjoint boxes: every pixel belongs to one region entirely
    t = SM.region_plan(H, W, hard_masks())
    assert t.R == 3 and t.wn.dtype == torch.float32 and tuple(t.wn.shape) == (3, H, W)
    assert torch.equal(t.wn[1], hard_masks()[0]) and torch.equal(t.wn[2], hard_masks()[1]) and torch.equal(t.wn[0], 1.0 - hard_masks().sum(0))
    # two overlapping soft masks at one pixel: fg 0.75 and 0.5, background clamp(1 - 1.25) = 0 -> (0, 0.6, 0.4)
    m = torch.zeros(2, 1, 2)
    m[:, 0, 0] = torch.tensor([0.75, 0.5])
    m[:, 0, 1] = torch.tensor([0.25, 0.25])                                           # background 0.5 -> (0.5, 0.25, 0.25)
    t = SM.region_plan(1, 2, m)
    assert t.wn[:, 0, 0].tolist() == [0.0, np.float32(0.6), np.float32(0.4)] and t.wn[:, 0, 1].tolist() == [0.5, 0.25, 0.25]
    assert t.wraw[:, 0, 0].tolist() == [0.0, 0.75, 0.5]
    # full coverage by foregrounds: the background has no weight anywhere; base > 0 gives it some everywhere
    t = SM.region_plan(2, 2, torch.ones(1, 2, 2))
    assert torch.equal(t.wn[0], torch.zeros(2, 2)) and torch.equal(t.wn[1], torch.ones(2, 2))
    t = SM.region_plan(2, 2, torch.ones(1, 2, 2), base=0.25)
    assert torch.equal(t.wn[0], torch.full((2, 2), 0.2)) and torch.equal(t.wn[1], torch.full((2, 2), 0.8)) and float(t.wraw[0, 0, 0]) == 0.25
    # no foreground: the background alone
    t = SM.region_plan(3, 4, None)
    assert t.R == 1 and torch.equal(t.wn, torch.ones(1, 3, 4))


@pytest.mark.parametrize("base", [0.0, 0.3])
def test_plan_is_the_restatement_and_sums_to_one(base):
    for masks in (soft_masks(), hard_masks(), torch.rand(7, 5, 9, generator=torch.Generator().manual_seed(1))):
        h, w = masks.shape[1:]
        t = SM.region_plan(h, w, masks, base)
        wn, wraw, R = RR.tables(h, w, masks, base)
        assert t.R == R and torch.equal(t.wn, wn) and torch.equal(t.wraw, wraw)
        assert float((t.wn.double().sum(0) - 1.0).abs().max()) <= 2.0 ** -23
        t2 = ops.region_tables(h, w, masks, base)
        assert torch.equal(t2.wn, t.wn) and torch.equal(t2.wraw, t.wraw)


@pytest.mark.parametrize("masks,base,msg", [(torch.full((1, H, W), 1.5), 0.0, r"\[0, 1\]"), (torch.full((1, H, W), -0.1), 0.0, r"\[0, 1\]"),
                                            (torch.full((1, H, W), float("nan")), 0.0, r"\[0, 1\]"), (torch.zeros(1, H, W + 1), 0.0, "expected"),
                                            (torch.zeros(H, W), 0.0, "expected"), (torch.zeros(8, H, W), 0.0, "at most 8"),
                                            (torch.zeros(1, H, W), -0.5, "base"), (torch.zeros(1, H, W), float("inf"), "base")])
def test_bad_plans(masks, base, msg):
    with pytest.raises(ValueError, match=msg):
        SM.region_plan(H, W, masks, base)


# ---- blend32 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R", [(1, 1), (1, 3), (2, 8)])
def test_blend32_of_one_field_returns_it(n, R):
    """R copies of one field fuse back to it within (R + 2) 2^-24 max|v|: one rounding per weight, one per product, R - 1 adds."""
    gen = torch.Generator().manual_seed(R)
    masks = torch.rand(R - 1, H, W, generator=gen) * 0.6
    t = SM.region_plan(H, W, masks)
    field = torch.randn(n, 1, 2, H, W, 4, generator=gen)
    back = RR.blend32(field.expand(n, R, 2, H, W, 4).reshape(-1, 4).contiguous(), t.wn, n, R, H, W)
    err = float((back.double() - field.reshape(-1, 4).double()).abs().max())
    bound = (R + 2) * 2.0 ** -24 * float(field.abs().max())
    print(f"n = {n}, R = {R}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_blend32_with_hard_masks_selects_the_owner():
    n, R = 2, 3
    t = SM.region_plan(H, W, hard_masks())
    eps = torch.randn(n, R, 2, H, W, 4, generator=torch.Generator().manual_seed(5))
    out = RR.blend32(eps.reshape(-1, 4), t.wn, n, R, H, W).view(n, 2, H, W, 4)
    owner = t.wn.argmax(0)
    for r in range(R):
        sel = owner == r
        assert bool(sel.any()) and torch.equal(out[:, :, sel], eps[:, r][:, :, sel])


def test_emulated_launches_are_the_contract():
    n, R = 2, 3
    gen = torch.Generator().manual_seed(3)
    tabs = ops.region_tables(H, W, soft_masks())
    x_full, tf = torch.randn(2 * n * H * W, 64, generator=gen).to(torch.bfloat16), torch.arange(2 * n, dtype=torch.float32) + 100.0
    x_r, tf_r = torch.zeros(2 * n * R * H * W, 64, dtype=torch.bfloat16), torch.zeros(2 * n * R)
    RR.emu_region_gather(tabs, x_full, x_r, tf, tf_r, n=n, H=H, W=W)
    rx, rt = RR.gather_ref(x_full, tf, n, R, H, W)
    assert torch.equal(x_r.view(torch.int16), rx.view(torch.int16)) and torch.equal(tf_r, rt)
    assert torch.equal(x_r.view(n, R, 2, H * W, 64)[:, 2].view(torch.int16), x_full.view(n, 2, H * W, 64).view(torch.int16))      # every region: the image's rows
    eps = torch.randn(2 * n * R * H * W, 4, generator=gen)
    out = RR.emu_region_blend(tabs, eps, torch.full((2 * n * H * W, 4), float("nan")), n=n, H=H, W=W)
    assert torch.equal(out, RR.blend32(eps, tabs.wn, n, R, H, W))
    # the noise: seed, step, region and pixel - and never the stochastic samplers' draw
    from tests import sde_ref as SR
    a = RR.noise(77, 2, 1, 40)
    assert not np.array_equal(a, RR.noise(77, 2, 2, 40)) and not np.array_equal(a, RR.noise(77, 3, 1, 40)) and not np.array_equal(a, RR.noise(78, 2, 1, 40))
    assert not np.array_equal(RR.noise(77, 2, 0, 40), SR.noise(77, 2, 40)) and np.array_equal(a[:, :30], RR.noise(77, 2, 1, 30))


# ---- the identity: fuse the predictions, then step == step every region, then fuse -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_fuse_then_step_is_step_then_fuse(kind, pred):
    R = 3
    cls = SM.EulerDiscrete if kind == "euler" else SM.DpmSolverPP2M
    sig = np.array([14.6, 6.1, 2.2, 0.7, 0.0], dtype=np.float64)
    full, regs = cls(prediction_type=pred).set_sigmas(sig), cls(prediction_type=pred).set_sigmas(sig)
    gen = torch.Generator().manual_seed(11)
    wn = torch.tensor(RR.weights64(H, W, soft_masks())[0], dtype=torch.float64)
    xa = xb = torch.randn(2 * H * W, 4, generator=gen, dtype=torch.float64) * sig[0]
    for i in range(len(sig) - 1):
        eps = torch.randn(2 * R * H * W, 4, generator=gen, dtype=torch.float64)     # every region predicts something else
        xa = full.step(RR.blend64(eps, wn, 1, R, H, W), i, xa)                     # this project: one prediction for the whole latent, one step
        xr = xb.view(1, 1, 2, H * W, 4).expand(1, R, 2, H * W, 4).reshape(-1, 4)   # the paper: every region stepped from the fused latent, then fused
        xb = RR.blend64(regs.step(eps, i, xr), wn, 1, R, H, W)
        assert float((xa - xb).abs().max()) <= 1e-12, (i, float((xa - xb).abs().max()))


# ---- the sampler on the emulated table ------------------------------------------------------------------------------------------------------------
def _regions(cfg, n=1, masks=None, seed=21, **kw):
    masks = soft_masks() if masks is None else masks
    em = _embeds(cfg, seed, n * masks.shape[0])
    per = [em[j * masks.shape[0]:(j + 1) * masks.shape[0]] for j in range(n)]
    return dict(masks=masks, embeds=per[0] if n == 1 else per, **kw)


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths_and_reference_on_the_emulated_table(version):
    steps, R = 4, 3
    cfg, sd, lora, rt, unet = _unet(version, 2 * R, emu_region)
    smp = SM.LatentSampler(rt, unet, n_images=1)
    assert (smp.n, smp.tiles) == (1, R)
    smp.set_lora_scale(0.75)
    em = _embeds(cfg, 5, 1)[0]
    gen = torch.Generator().manual_seed(9)
    noise, x0 = torch.randn(1, 4, H, W, generator=gen), 0.8 * torch.randn(1, 4, H, W, generator=gen)
    mask = (torch.rand(1, 1, H, W, generator=gen) * 3).floor() / 2
    bg = torch.randn(1, R, 4, generator=gen) * 0.3
    for boot in (0, 2):
        rg = _regions(cfg, bootstrap=boot, bg=bg)
        run = lambda **kw: smp.sample(em, H, W, steps=steps, latents=noise.clone(), regions=rg, seeds=[31], **kw)  # noqa: E731
        fused = run(fused=True)
        ref = RR.sample_latents(cfg, sd, lora, 0.75, em, rg["embeds"], rg["masks"], noise, steps, bootstrap=boot, bg=bg[0], seed=31)
        a, b = fused.reshape(-1).double(), ref.reshape(-1).double()
        cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
        print(f"{version} bootstrap={boot}: cos {cos:.6f} rel {rel:.4f}")
        assert cos >= 0.999 and rel <= 0.06                                              # DESIGN 4.21's bars
        # the torch loop with the guidance pre-pass in use takes the step in the kernel's order: the fused path's bits
        kw = dict(guidance_rescale=0.5)
        assert torch.equal(run(**kw), run(fused=True, **kw))
        for sampler_ in ("dpmpp_2m", "euler_a"):
            a = run(fused=True, sampler=sampler_, **kw)
            assert torch.isfinite(a).all() and torch.equal(a, run(sampler=sampler_, **kw))
    # a mask at full size: the kept pixels are the init latents exactly; a change map alike
    out = run(fused=True, init_latents=x0, strength=0.5, mask=mask)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(out[keep], x0[keep]) and torch.isfinite(out).all()
    cmap = torch.linspace(0, 1, H * W).view(1, 1, H, W)
    assert torch.equal(run(fused=True, init_latents=x0, strength=0.5, change_map=cmap, **kw), run(init_latents=x0, strength=0.5, change_map=cmap, **kw))
    # another mask set with the same region count: the same persistent buffers
    assert len(smp._fused["shapes"]) == 1
    other = smp.sample(em, H, W, steps=2, latents=noise.clone(), regions=_regions(cfg, masks=hard_masks()), fused=True)
    assert len(smp._fused["shapes"]) == 1 and torch.isfinite(other).all()
    # the conditioning layout: row 2 r + 1 carries region r's positive context, every even row the call's negative one
    from sd_lora_trainer_amd.unet import CTX_PAD
    cv = smp.ctx.view(1, R, 2, CTX_PAD, -1)
    for r in range(R):
        c_r = em[0] if r == 0 else rg["embeds"][r - 1][0]
        assert torch.equal(cv[0, r, 1, :77], c_r[0].to(cv.dtype)) and torch.equal(cv[0, r, 0, :77], em[1][0].to(cv.dtype)), r


def test_no_foreground_is_the_plain_path():
    """R = 1: the same launch list, bits and capture key as without the keyword - on a table without the region launches."""
    calls = []
    import types
    table = types.ModuleType("emu_logged")
    for k, v in vars(emu_plain).items():
        if not k.startswith("__"):
            setattr(table, k, (lambda f, k_: (lambda *a, **kw: (calls.append(k_), f(*a, **kw))[1]))(v, k) if callable(v) and not isinstance(v, type) else v)
    cfg, sd, lora, rt, unet = _unet("tiny15", 2, table)
    smp = SM.LatentSampler(rt, unet)
    em = _embeds(cfg, 5, 1)[0]
    noise = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    none = dict(masks=torch.zeros(0, 8, 8), embeds=[])
    for kw in (dict(), dict(fused=True), dict(fused=True, sampler="euler_a", seeds=[3])):
        del calls[:]
        a = smp.sample(em, 8, 8, steps=3, latents=noise.clone(), **kw)
        plain_calls = list(calls)
        del calls[:]
        assert torch.equal(smp.sample(em, 8, 8, steps=3, latents=noise.clone(), regions=none, **kw), a) and calls == plain_calls
    assert list(smp._fused["shapes"]) == [(8, 8)]                                         # the plain shape's state: no region buffers, the plain capture key
    assert "reg" not in smp._fused["shapes"][(8, 8)]


def test_two_images_are_sampled_as_each_alone():
    n, R = 2, 3
    outs = {}
    for k in (1, n):
        cfg, sd, lora, rt, unet = _unet("tinyxl", 2 * k * R, emu_region)
        smp = SM.LatentSampler(rt, unet, n_images=k)
        ems = _embeds(cfg, 5, n)
        rg = _regions(cfg, n, bootstrap=1)
        noise = torch.randn(n, 4, H, W, generator=torch.Generator().manual_seed(2))
        if k == 1:
            outs[k] = torch.cat([smp.sample(ems[j], H, W, steps=3, latents=noise[j:j + 1].clone(), fused=True, seeds=[50 + j],
                                            regions=dict(rg, embeds=rg["embeds"][j])) for j in range(n)])
        else:
            outs[k] = smp.sample(ems, H, W, steps=3, latents=noise.clone(), fused=True, n_images=n, seeds=[50, 51], regions=rg)
    # a CPU matrix product's bits may follow the batch it runs in: fp32 sums of up to ~10^3 terms in another order differ by about sqrt(K) 2^-24 = 2e-6
    # of the operands' scale per product; a few products deep and three steps long, 1e-5 of the latents' scale (the random tinyxl weights give ~10^2)
    scale = float(outs[1].abs().max())
    err = float((outs[1] - outs[n]).abs().max())
    print(f"alone vs together: max |difference| {err:.3e}, scale {scale:.3e}")
    assert err <= 1e-5 * scale
    assert not torch.equal(outs[n][0], outs[n][1])


def test_bootstrap_replaces_the_model_input_outside_the_masks_only(monkeypatch):
    steps, R = 4, 3
    cfg, sd, lora, rt, unet = _unet("tiny15", 2 * R, emu_region)
    smp = SM.LatentSampler(rt, unet, n_images=1)
    em = _embeds(cfg, 5, 1)[0]
    noise = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(9))
    seen = []
    real = emu_region.region_gather

    def spy(tabs, x_full, x_regions, *a, **kw):
        out = real(tabs, x_full, x_regions, *a, **kw)
        diff = (x_regions.view(R, 2, H, W, -1) != x_full.view(1, 2, H, W, -1)).float()
        seen.append((diff[..., :4].amax(-1), float(diff[..., 4:].max()), tabs.wraw.clone()))
        return out

    monkeypatch.setattr(emu_region, "region_gather", spy)
    # bootstrap = 0: no noise is drawn, and neither the seeds nor bg reach the model input - NaN backgrounds leave every bit alone
    RR.READS["noise"] = 0
    rg0 = _regions(cfg, bootstrap=0)
    poisoned = dict(rg0, bg=None)
    a = smp.sample(em, H, W, steps=steps, latents=noise.clone(), regions=poisoned, fused=True)
    assert RR.READS["noise"] == 0 and len(seen) == steps and all(float(d.max()) == 0.0 and rest == 0.0 for d, rest, _ in seen)
    smp._fused["shapes"][(H, W, "region", R)]["reg"]["bg"].fill_(float("nan"))
    monkeypatch.setattr(SM.LatentSampler, "_region_state", lambda self, sh, h, w, reg: sh["reg"])      # (keep the poison: the tables are those of the call above)
    assert torch.equal(smp.sample(em, H, W, steps=steps, latents=noise.clone(), regions=poisoned, fused=True), a)
    monkeypatch.undo()
    monkeypatch.setattr(emu_region, "region_gather", spy)
    # bootstrap = 2 of 4: rows r >= 1 differ from x_full exactly on wraw < 0.5 at steps 0 and 1, nowhere at steps 2 and 3; row 0 never; columns 4.. never
    for path in (dict(fused=True), dict()):
        del seen[:]
        b = smp.sample(em, H, W, steps=steps, latents=noise.clone(), regions=_regions(cfg, bootstrap=2, bg=torch.full((1, R, 4), 0.25)), seeds=[8], **path)
        assert len(seen) == steps and RR.READS["noise"] > 0 and not torch.equal(a, b)
        for i, (d, rest, wraw) in enumerate(seen):
            assert rest == 0.0 and float(d[0].max()) == 0.0, i
            for r in (1, 2):
                want = (wraw[r] < 0.5).float().expand(2, H, W) if i < 2 else torch.zeros(2, H, W)
                assert torch.equal(d[r], want), (i, r)                                    # (a bf16 draw equal to the row's own value has probability ~ 0: none here)
    # a bootstrap longer than the trajectory is cut to it
    del seen[:]
    smp.sample(em, H, W, steps=2, latents=noise.clone(), regions=_regions(cfg, bootstrap=50), seeds=[8], fused=True)
    assert len(seen) == 2 and all(float(d[1].max()) == 1.0 for d, _, _ in seen)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_refusals():
    stub = _Stub(1, H, W, 7)
    smp = SM.LatentSampler(unet_mod.Runtime("cpu", 6, act_dtype=torch.float32, ops=emu_region), stub, n_images=1)
    noise = torch.zeros(1, 4, H, W)
    rg = dict(masks=soft_masks(), embeds=[EMB, EMB])
    call = lambda **kw: smp.sample(EMB, H, W, steps=2, latents=noise, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="tile"):
        call(regions=rg, tile=(8, 2))
    with pytest.raises(ValueError, match="heatmap"):
        call(regions=rg, heatmap=dict(cols=[[1]]))
    with pytest.raises(ValueError, match="3 window"):                              # the runtime was built for three regions: a plain call and another count
        call()
    with pytest.raises(ValueError, match="the call needs 2"):
        call(regions=dict(masks=soft_masks()[:1], embeds=[EMB]), fused=True)
    for bad, msg in ((dict(rg, embeds=[EMB]), "per foreground region"), (dict(rg, masks=soft_masks() * 2), r"\[0, 1\]"), (dict(rg, base=-1.0), "base"),
                     (dict(rg, bootstrap=-1), "bootstrap"), (dict(rg, bootstrap=0.5), "bootstrap"), (dict(rg, bg=torch.zeros(1, 2, 4)), "bg"),
                     (dict(rg, feather=2), "unknown"), (dict(masks=soft_masks()), "embeds"), (dict(rg, masks=torch.zeros(8, H, W), embeds=[EMB] * 8), "at most 8")):
        with pytest.raises(ValueError, match=msg):
            call(regions=bad)
    assert stub.calls == 0
    bare = SM.LatentSampler(unet_mod.Runtime("cpu", 6, act_dtype=torch.float32, ops=emu_plain), stub, n_images=1)
    for kw in (dict(), dict(fused=True)):
        with pytest.raises(NotImplementedError, match="sdlt_region_blend"):        # no torch fallback
            bare.sample(EMB, H, W, steps=2, latents=noise, regions=rg, **kw)
    assert stub.calls == 0


# ---- the entry points' checks (nothing is launched: no GPU here) ----------------------------------------------------------------------------------
def lib_region(lib, which, **kw):
    """sdlt_region_gather / sdlt_region_blend on made-up addresses, one argument changed: n = 1, R = 3, a 10 x 11 grid."""
    import ctypes
    from sd_lora_trainer_amd import _lib
    a = dict(dict(wn=0x1000, wraw=0x2000, bg=0x3000, rtab=0x4000, ctr=0x7000, seeds=0x8000, n=1, R=3, H=10, W=11,
                  x_full=0x100000, x_regions=0x200000, ld=64, tf_full=0x5000, tf_regions=0x6000, eps_regions=0x300000, eps_full=0x400000), **kw)
    p = None
    if not a.get("null_block"):
        p = _lib.RegionParams(**{k: a[k] for k in ("wn", "wraw", "bg", "rtab", "ctr", "seeds", "n", "R", "H", "W")})
    ref = None if p is None else ctypes.byref(p)
    if which == "gather":
        return lib.sdlt_region_gather(ref, a["x_full"], a["x_regions"], a["ld"], a["tf_full"], a["tf_regions"], None)
    return lib.sdlt_region_blend(ref, a["eps_regions"], a["eps_full"], None)


SHARED_REFUSALS = [dict(null_block=True), dict(n=0), dict(R=0), dict(H=0), dict(W=-1), dict(R=17), dict(H=16385), dict(W=16385), dict(n=32768),
                   dict(n=32767, R=16, H=16384, W=16384)]
GATHER_REFUSALS = [dict(x_full=None), dict(x_regions=None), dict(tf_full=None), dict(tf_regions=None), dict(ld=0), dict(ld=60), dict(ld=-8), dict(ld=4104),
                   dict(ld=1 << 20), dict(x_full=0x100008), dict(x_regions=0x200004), dict(tf_full=0x5002), dict(tf_regions=0x6001),
                   dict(x_regions=0x100000), dict(x_regions=0x100000 + 2 * 110 * 128 - 16), dict(x_full=0x200000 + 6 * 110 * 128 - 16),
                   dict(wraw=None), dict(bg=None), dict(rtab=None), dict(ctr=None), dict(seeds=None), dict(wraw=None, bg=None, rtab=None, ctr=None),
                   dict(wraw=0x2002), dict(bg=0x3001), dict(rtab=0x4002), dict(ctr=0x7001), dict(seeds=0x8003)]
BLEND_REFUSALS = [dict(wn=None), dict(eps_regions=None), dict(eps_full=None), dict(eps_regions=0x300008), dict(eps_full=0x400004), dict(wn=0x1001),
                  dict(eps_full=0x300000), dict(eps_full=0x300000 + 6 * 110 * 16 - 16), dict(eps_regions=0x400000 + 2 * 110 * 16 - 16)]


def check_refusals():
    """Every refusal returns a negative code, names the entry point and launches nothing (the addresses are made up: a launch would fault).  Also called
    by the GPU file."""
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert all(f"sdlt_region_{k}" in _lib.SYMBOLS for k in ("gather", "blend", "noise"))
    for which, own in (("gather", GATHER_REFUSALS), ("blend", BLEND_REFUSALS)):
        for change in SHARED_REFUSALS + own:
            assert lib_region(lib, which, **change) < 0, (which, change)
            assert f"sdlt_region_{which}".encode() in lib.sdlt_last_error(), (which, change, lib.sdlt_last_error())
    # gather does not read the weights, blend not the bootstrap's tables: null is fine there, so the first refusal they meet is the next one in line
    assert lib_region(lib, "gather", wn=None, x_full=None) == -1 and b"null pointer" in lib.sdlt_last_error()
    assert lib_region(lib, "blend", wraw=None, seeds=None, eps_full=None) == -1 and b"null pointer" in lib.sdlt_last_error()
    for args, code in (((None, 0, 1, 1, 4, 0x1000), -1), ((0x1000, 0, 1, 1, 4, None), -1), ((0x1000, -1, 1, 1, 4, 0x2000), -1), ((0x1000, 0, -1, 1, 4, 0x2000), -1),
                       ((0x1000, 0, 1, 0, 4, 0x2000), -1), ((0x1000, 0, 1, 1, 0, 0x2000), -1), ((0x1000, 0, 1, 1 << 20, 1 << 20, 0x2000), -1),
                       ((0x1002, 0, 1, 1, 4, 0x2000), -2), ((0x1000, 0, 1, 1, 4, 0x2001), -2)):
        assert lib.sdlt_region_noise(*args, None) == code, args
        assert b"sdlt_region_noise" in lib.sdlt_last_error()


def test_entry_point_validation():
    check_refusals()


def test_wrappers_check_shapes():
    tabs = ops.region_tables(H, W, soft_masks())
    with pytest.raises(AssertionError):
        ops.region_blend(tabs, torch.zeros(10, 4), torch.zeros(10, 4), n=1, H=H, W=W)      # CPU tensors: refused before the library is asked
    with pytest.raises(AssertionError):
        ops.region_gather(tabs, torch.zeros(10, 64), torch.zeros(30, 64), torch.zeros(2), torch.zeros(6), n=1, H=H, W=W)
    with pytest.raises(AssertionError):
        ops.region_noise(torch.zeros(1, 2, dtype=torch.int32), 0, 1, torch.zeros(1, 4, 2, 2))


# ---- render() and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path, capsys):
    import types
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    box = ["--region", "0,0,0.5,1", "a barn"]
    for extra, msg in ((["--region-feather", "2"], "need --region"), (["--region-base", "0.5"], "need --region"), (["--region-bootstrap", "0.1"], "need --region"),
                       (box + ["--tile-diffusion", "8"], "--tile-diffusion"), (box + ["--heatmap"], "--heatmap"), (box + ["--hires-scale", "2"], "--hires"),
                       (box + ["--hires-size", "64", "64"], "--hires"), (box + ["--hires-strength", "0.5"], "--hires"),
                       (["--region", "0.5,0,0.2,1", "a barn"], "box"), (["--region", "0,0,1.5,1", "a barn"], "box"), (["--region", "0,0,1,1", " "], "prompt"),
                       (["--region", str(tmp_path / "no.png"), "a barn"], "neither a box"), (["--region", "0,0,1", "a barn"], "neither a box"),
                       (box + ["--region-feather", "-1"], "region_feather"), (box + ["--region-base", "-0.5"], "region_base"),
                       (box + ["--region-bootstrap", "1.5"], "region_bootstrap"), (box * 8, "1 .. 7"), (["--region", "0,0,1,1"], "expected 2 arguments")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)                                                          # (the checkpoint does not exist: refused before anything is loaded)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    loaded = types.SimpleNamespace(config=types.SimpleNamespace(resolution=1024))
    png = tmp_path / "m.png"
    png.write_bytes(b"")
    with mock.patch.object(R, "load_for_inference", lambda *a, **k: loaded), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert not any(k.startswith("region") for k in seen)                              # without the flag render() is called as before
        R.main(base + box + ["--region", str(png), "a photo of <concept>"])
        assert seen["regions"] == [((0.0, 0.0, 0.5, 1.0), "a barn"), (str(png), "a photo of <concept>")] and "region_feather" not in seen
        R.main(base + box + ["--region-feather", "1.5", "--region-base", "0.25", "--region-bootstrap", "0"])
        assert (seen["region_feather"], seen["region_base"], seen["region_bootstrap"]) == (1.5, 0.25, 0.0)


def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    from tests.test_guidance_cpu import _FakeLoaded
    box = [((0.0, 0.0, 0.5, 1.0), "a barn")]
    for kw, msg in ((dict(region_feather=1.0), "need regions"), (dict(region_base=0.1), "need regions"), (dict(region_bootstrap=0.1), "need regions"),
                    (dict(regions=[]), "1 .. 7"), (dict(regions=box * 8), "1 .. 7"), (dict(regions=[((0.5, 0, 0.5, 1), "a")]), "box"), (dict(regions=[("m.png",)]), "prompt"),
                    (dict(regions=box, region_feather=-1.0), "region_feather"), (dict(regions=box, region_base=float("nan")), "region_base"),
                    (dict(regions=box, region_bootstrap=2), "region_bootstrap"), (dict(regions=box, tile_diffusion=(8, 2)), "tile_diffusion"),
                    (dict(regions=box, heatmap=[]), "heatmap"), (dict(regions=box, hires=dict(scale=2.0)), "hires")):
        with pytest.raises(ValueError, match=msg):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), **kw)
    assert not os.path.exists(tmp_path / "o")


def test_render_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    """--region end to end: pictures, prompts.json, the UNet built for batch 2 R and kept for another mask set, the conditioning route of a region's
    prompt, an op table without the launches - and a region that covers nothing, which gives the picture of the render without it."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    config, ckdir = job
    builds, calls, lats = [], [], []
    real_build, real_sample = T.RenderStack.build_sampler, SM.LatentSampler.sample
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n, **kw: (builds.append((n, kw.get("tiles", 1))), real_build(self, n, **kw))[1])

    def spy(self, em, h, w, **kw):
        calls.append((h, w, self.rt.B, kw.get("regions"), kw.get("seeds")))
        lats.append(real_sample(self, em, h, w, **kw))
        return lats[-1]

    monkeypatch.setattr(SM.LatentSampler, "sample", spy)
    rt = lambda table=emu_region: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of a field", "--steps", "4", "--seed", "5", "--size", "80", "48"]      # a 12 x 20 latent of the tiny VAE
    mask_png = str(tmp_path / "mask.png")
    arr = np.zeros((48, 80), dtype=np.uint8)
    arr[24:, :40] = 255
    Image.fromarray(arr).save(mask_png)
    out = tmp_path / "regions"
    R.main(common + ["--region", "0.5,0,1,1", "a photo of <concept>", "--region", mask_png, "a red barn", "--region-base", "0.1", "--out", str(out)], runtime=rt())
    meta = json.load(open(out / "prompts.json"))
    assert meta["regions"] == [dict(prompt="a photo of <concept>", box=[0.5, 0.0, 1.0, 1.0]), dict(prompt="a red barn", mask=mask_png)]
    assert (meta["region_base"], meta["region_bootstrap"], meta["region_feather"]) == (0.1, 0.2, 0.0) and meta["size"] == [80, 48]
    assert builds == [(1, 1), (1, 3)] and len(calls) == 1
    h, w, B, rg, seeds = calls[0]
    assert (h, w, B) == (12, 20, 6) and seeds == [5] and rg["bootstrap"] == 1 and rg["base"] == 0.1 and tuple(rg["bg"].shape) == (1, 3, 4)      # round(0.2 * 4) = 1
    want = torch.zeros(2, 12, 20)
    want[0, :, 10:] = 1.0
    want[1, 6:, :10] = 1.0
    assert torch.equal(rg["masks"], want) and len(rg["embeds"]) == 2 and bool(torch.isfinite(rg["bg"]).all()) and float(rg["bg"].abs().max()) > 0
    name = next(f for f in sorted(os.listdir(out)) if f.startswith("img_00"))
    assert Image.open(out / name).size == (80, 48)
    assert np.isfinite(np.asarray(Image.open(out / name), dtype=np.float64)).all()
    plain = tmp_path / "plain"
    del lats[:]
    R.main(common + ["--out", str(plain)], runtime=rt())
    assert not any(k.startswith("region") for k in json.load(open(plain / "prompts.json")))      # without the flag: the keys as before
    assert open(plain / name, "rb").read() != open(out / name, "rb").read()
    lat_plain = lats[-1]
    # a region that covers nothing (an all-black mask, bootstrap 0): its weight is 0 everywhere and the background's 1, so every fused prediction is
    # 1 * v + 0 * v' = v up to blend32's bound (R + 2) 2^-24 max|v|; one Euler step from sigma_0 multiplies it by sigma_0
    black = str(tmp_path / "black.png")
    Image.fromarray(np.zeros((48, 80), dtype=np.uint8)).save(black)
    one = ["--checkpoint", ckdir, "--prompt", "a photo of a field", "--steps", "1", "--seed", "5", "--size", "80", "48"]
    del lats[:]
    R.main(one + ["--out", str(tmp_path / "p1")], runtime=rt())
    R.main(one + ["--region", black, "a red barn", "--region-bootstrap", "0", "--out", str(tmp_path / "r1")], runtime=rt())
    sig0 = float(SM.EulerDiscrete().set_timesteps(1).sigmas[0])
    eps_max = float(lats[0].abs().max()) / sig0 + 6.0                      # x_1 = x_0 - sigma_0 eps with x_0 = sigma_0 noise: |eps| <= |x_1| / sigma_0 + |noise|, |noise| < 6
    err = float((lats[0] - lats[1]).abs().max())
    print(f"a region that covers nothing: max |difference| {err:.3e}, bound {(2 + 2) * 2.0 ** -24 * eps_max * sig0:.3e}")
    assert err <= (2 + 2) * 2.0 ** -24 * eps_max * sig0
    # one loaded checkpoint, two mask sets and bootstrap shares: the UNet and its sampler are built once
    ld = R.load_for_inference(ckdir, runtime=rt())
    del builds[:], calls[:]
    R.render(ld, ["a house"], str(tmp_path / "a"), size=(80, 48), steps=2, regions=[((0.0, 0.0, 0.5, 1.0), "a tree"), ((0.5, 0.0, 1.0, 1.0), "a barn")], region_feather=1.0)
    first = ld.stack.sampler
    R.render(ld, ["a house"], str(tmp_path / "b"), size=(80, 48), steps=2, regions=[((0.2, 0.2, 0.6, 0.9), "a tree"), (mask_png, "a barn")], region_bootstrap=0.0)
    assert ld.stack.sampler is first and builds == [(1, 3)] and ld.shape == (1, 12, 20, "region", 3)
    feathered = calls[0][3]["masks"]
    assert 0.0 < float(feathered[0, 5, 9]) < 1.0 and calls[1][3]["bootstrap"] == 0 and calls[1][3]["bg"] is None
    # a region's prompt takes the main prompt's route: the trigger substitution and blend_conditions
    c_main = ld.stack.conditioning("a photo of <concept>", 0.8)[0]
    del calls[:]
    R.render(ld, ["a house"], str(tmp_path / "c"), size=(80, 48), steps=1, lora_scales=[0.8], regions=[((0.0, 0.0, 0.5, 1.0), "a photo of <concept>"), (mask_png, "a barn")])
    assert torch.equal(calls[0][3]["embeds"][0][0], c_main[0]) and not torch.equal(calls[0][3]["embeds"][1][0], c_main[0])
    # an op table without the launches: refused, nothing written
    with pytest.raises(NotImplementedError, match="sdlt_region_blend"):
        R.main(common + ["--region", "0,0,0.5,1", "a barn", "--out", str(tmp_path / "none")], runtime=rt(emu_plain))
    assert not os.path.exists(tmp_path / "none")
