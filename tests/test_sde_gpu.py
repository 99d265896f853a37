"""The stochastic samplers on the MI355X: sdlt_sampler_noise against the fp64 Philox / Box-Muller reference, sdlt_sampler_step_sde against its contract
evaluated in torch (bit for bit) and against sdlt_sampler_step_ms where it adds no noise, LatentSampler.sample(sampler="euler_a" | "dpmpp_2m_sde") -
graph == fused == torch loop, seeds, batch independence, the published loops of tests/sde_ref.py driven by the oracle UNet - and
`python -m sd_lora_trainer_amd.render --sampler euler_a | dpmpp_2m_sde` end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import sde_ref as SR
from tests.test_multistep_gpu import _cuda, _figures, _inputs, _run, _setup
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars tests/test_multistep_gpu.py holds dpmpp_2m to against its reference loop

pytestmark = pytest.mark.gpu

SENT = 3.25
KINDS = ("euler_a", "dpmpp_2m_sde")
SEEDS3 = [1234, 2 ** 63 + 5, 0xFFFFFFFF00000001]
# |z_gpu - z_fp64| over the launches of test_sampler_noise, measured on the MI355X: 3.545e-7; the uniforms are exact, so only logf, sqrtf,
# sincospif and the final product differ.  The bar is four times that, and may never exceed 1e-4
NOISE_TOL = 4 * 3.545e-7
assert NOISE_TOL <= 1e-4


def _words(seeds):
    from sd_lora_trainer_amd import sampler as SM
    return SM.seed_words(seeds, len(seeds)).cuda()


# ---- the noise -------------------------------------------------------------------------------------------------------------------------
def test_sampler_noise():
    from sd_lora_trainer_amd import ops
    n, h, w = 3, 9, 13                                                           # 351 threads: two workgroups, both image boundaries inside the first
    words = _words(SEEDS3)
    worst, outs = 0.0, {}
    for step in (0, 3, 4, 999):
        z = ops.sampler_noise(words, step, torch.full((n, 4, h, w), float("nan"), device="cuda")).cpu()
        ref = np.stack([SR.noise(s, step, h * w).reshape(4, h, w) for s in SEEDS3])
        assert bool(torch.isfinite(z).all())
        worst = max(worst, float(np.abs(z.double().numpy() - ref).max()))
        outs[step] = z
    print(f"sdlt_sampler_noise: max |z - fp64 reference| = {worst:.3e} (bar {NOISE_TOL:.3e})")
    assert worst <= NOISE_TOL
    assert not torch.equal(outs[3], outs[4]) and not torch.equal(outs[0], outs[3])                           # step i and step i + 1 differ
    # image 1 of the launch is the n = 1 launch with image 1's seed: not the batch, not the place in it
    alone = ops.sampler_noise(_words(SEEDS3[1:2]), 3, torch.zeros(1, 4, h, w, device="cuda")).cpu()
    assert torch.equal(alone[0], outs[3][1]) and not torch.equal(outs[3][0], outs[3][1]) and not torch.equal(outs[3][2], outs[3][1])


# ---- the step kernel -------------------------------------------------------------------------------------------------------------------
def _trajectory_state(n, h, w, ld, dev):
    return dict(x=torch.full((n, 4, h, w), float("nan"), device=dev), dprev=torch.full((n, 4, h, w), float("nan"), device=dev),
                xin=torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16, device=dev), tf=torch.full((2 * n,), -1.0, device=dev),
                ctr=torch.tensor([2, 0], dtype=torch.int32, device=dev))


@pytest.mark.parametrize("kind,pred,case,shape", [(k, p, c, (3, 9, 13)) for k in KINDS for p in ("epsilon", "v_prediction") for c in ("txt2img", "x0", "random")]
                         + [("dpmpp_2m_sde", "epsilon", "random", (1, 19, 27))])     # 351 pixels; 513 = 2 * 256 + 1: a third workgroup of one thread
def test_sampler_step_sde_kernel_exact(kind, pred, case, shape):
    """init (without / with x0), a first-order row, rows with c != 0 (dpmpp_2m_sde), the last row (d = 0), with and without a mask: x, dprev, both rows
    of every pair of the model input, timesteps and counter against the restated kernel fed sdlt_sampler_noise's z, bit for bit."""
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w = shape
    g, ld, k = 7.5, 64, 4
    steps, start = (k, 0) if case == "txt2img" else (7, 3)
    cls = dict(euler_a=SM.EulerAncestral, dpmpp_2m_sde=SM.DpmSolverPP2MSDE)[kind]
    tab = SM.step_table_sde(cls(prediction_type=pred, eta=1.0).set_timesteps(steps, start, "karras" if kind == "dpmpp_2m_sde" else "trailing"), g)
    assert tab.shape == (2 + k, 8) and float(tab[2 + k - 1, 1]) == 0.0
    assert [float(c) != 0.0 for c in tab[2:, 6]] == ([False, True, True, False] if kind == "dpmpp_2m_sde" else [False] * 4)
    assert [float(d) != 0.0 for d in tab[2:, 7]] == [True, True, True, False]
    table = torch.zeros(40, 8)
    table[: tab.shape[0]] = tab
    gen = torch.Generator().manual_seed(1000 * n + h)
    x0, noise = 0.8 * torch.randn(n, 4, h, w, generator=gen), torch.randn(n, 4, h, w, generator=gen)
    mask = torch.rand(n, 1, h, w, generator=gen) if case == "random" else None
    if case == "txt2img":
        x0 = None
    if mask is not None:
        mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
        mask[-1, 0, -1, -2:] = 0.0
    eps = [torch.randn(2 * n * h * w, 4, generator=gen) for _ in range(k)]
    seeds = SEEDS3[:n]
    dev = "cuda"
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    st = _trajectory_state(n, h, w, ld, dev)
    x, dprev, xin, tf, ctr = st["x"], st["dprev"], st["xin"], st["tf"], st["ctr"]
    table_d, x0_d, noise_d, mask_d, words = d(table), d(x0), d(noise), d(mask), _words(seeds)
    rx, rd = torch.zeros(n, 4, h, w), torch.full((n, 4, h, w), float("nan"))
    rxin, rtf, rctr = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16), torch.zeros(2 * n), torch.tensor([2, 0], dtype=torch.int32)

    def compare(what, with_d=True):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), rx), (what, int((x.cpu() != rx).sum()))
        if with_d:
            assert torch.equal(dprev.cpu(), rd), (what, int((dprev.cpu() != rd).sum()))
        assert torch.equal(xin.cpu().view(torch.int16), rxin.view(torch.int16)), what
        assert torch.equal(tf.cpu(), rtf) and ctr.cpu().tolist() == rctr.tolist(), (what, tf.cpu(), ctr.cpu())

    ops.sampler_step_sde(None, x, xin, tf, table_d, ctr, dprev=dprev, seeds=words, x0=x0_d, noise=noise_d, mask=mask_d, init=True)
    SR.sampler_step_sde(None, rx, rxin, rtf, table, rctr, dprev=rd, seeds=words.cpu(), x0=x0, noise=noise, mask=mask, init=True)
    assert rctr.tolist() == [0, 0] and float(rtf[0]) == float(tab[0, 3])
    compare("init", with_d=False)
    assert bool(torch.isnan(dprev).all())
    x_init, first, zbuf = x.clone(), [], torch.zeros(n, 4, h, w, device=dev)
    for i in range(k):
        z = ops.sampler_noise(words, i, zbuf).cpu() if float(tab[2 + i, 7]) != 0.0 else None
        before = x.clone()
        ops.sampler_step_sde(eps[i].to(dev), x, xin, tf, table_d, ctr, dprev=dprev, seeds=words, x0=x0_d, noise=noise_d, mask=mask_d)
        SR.sampler_step_sde(eps[i], rx, rxin, rtf, table, rctr, dprev=rd, seeds=words.cpu(), x0=x0, noise=noise, mask=mask, z=z)
        assert rctr.tolist() == [(i + 1) % k, 0] and float(rtf[0]) == float(tab[2 + i, 3])
        compare(i)
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(dprev).all()), i
        first.append((x.clone(), dprev.clone(), xin.clone(), tf.clone()))
        if z is not None:                                                        # and the noise is in there: the same step from the same state without it
            y, yd, yc = before.cpu(), rd.clone(), torch.tensor([i, 0], dtype=torch.int32)
            SR.sampler_step_sde(eps[i], y, rxin.clone(), rtf.clone(), table, yc, dprev=yd, seeds=words.cpu(), x0=x0, noise=noise, mask=mask, z=torch.zeros_like(z))
            assert not torch.equal(y, rx)
    assert ctr.cpu().tolist() == [0, 0] and torch.equal(tf.cpu(), torch.full((2 * n,), float(tab[0, 3])))
    if mask is not None:
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) >= 12 and torch.equal(x.cpu()[keep], x0[keep])                     # the kept region: re-injected after the noise
    # a second trajectory on the wrapped counter, same seeds: the same bits at every step; then other seeds: other bits from the first step on
    for other in (False, True):
        x.copy_(x_init)
        if other:
            words.copy_(_words([s + 1 for s in seeds]))
        for i in range(k):
            ops.sampler_step_sde(eps[i].to(dev), x, xin, tf, table_d, ctr, dprev=dprev, seeds=words, x0=x0_d, noise=noise_d, mask=mask_d)
            torch.cuda.synchronize()
            fx, fd, fxin, ftf = first[i]
            assert torch.equal(x, fx) != other and torch.equal(tf, ftf), (other, i)
            assert other or (torch.equal(dprev, fd) and torch.equal(xin.view(torch.int16), fxin.view(torch.int16))), i
            assert ctr.cpu().tolist() == [(i + 1) % k, 0]
    assert bool((xin[:, 4:] == SENT).all())


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_no_noise_rows_are_the_multistep_kernel(pred):
    """A table whose d column is zero (step_table_ms's own): every output equals sdlt_sampler_step_ms's on the same inputs, bit for bit; and a step
    launch without seeds, or with misaligned ones, is refused before anything is launched."""
    from sd_lora_trainer_amd import _lib, ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w, ld, k = 3, 9, 13, 64, 4
    tab = SM.step_table_ms(SM.DpmSolverPP2M(prediction_type=pred).set_timesteps(7, 3, "karras"), 7.5)
    assert bool((tab[:, 7] == 0).all()) and [float(c) != 0.0 for c in tab[2:, 6]] == [False, True, True, False]
    table = torch.zeros(40, 8)
    table[: tab.shape[0]] = tab
    gen = torch.Generator().manual_seed(9)
    dev = "cuda"
    x0, noise, mask = (t.to(dev) for t in (0.8 * torch.randn(n, 4, h, w, generator=gen), torch.randn(n, 4, h, w, generator=gen), torch.rand(n, 1, h, w, generator=gen)))
    eps = [torch.randn(2 * n * h * w, 4, generator=gen).to(dev) for _ in range(k)]
    table_d, words = table.to(dev), _words(SEEDS3)
    a, b = _trajectory_state(n, h, w, ld, dev), _trajectory_state(n, h, w, ld, dev)
    kw = lambda s: dict(dprev=s["dprev"], x0=x0, noise=noise, mask=mask)  # noqa: E731
    ops.sampler_step_ms(None, a["x"], a["xin"], a["tf"], table_d, a["ctr"], init=True, **kw(a))
    ops.sampler_step_sde(None, b["x"], b["xin"], b["tf"], table_d, b["ctr"], seeds=words, init=True, **kw(b))
    for i in range(k):
        ops.sampler_step_ms(eps[i], a["x"], a["xin"], a["tf"], table_d, a["ctr"], **kw(a))
        ops.sampler_step_sde(eps[i], b["x"], b["xin"], b["tf"], table_d, b["ctr"], seeds=words, **kw(b))
        torch.cuda.synchronize()
        for key in ("x", "dprev", "tf", "ctr"):
            assert torch.equal(a[key], b[key]), (i, key)
        assert torch.equal(a["xin"].view(torch.int16), b["xin"].view(torch.int16)) and bool(torch.isfinite(b["x"]).all()), i
    lib = _lib.load()
    ptr = lambda t: t.data_ptr()  # noqa: E731
    base = dict(eps=ptr(eps[0]), x=ptr(b["x"]), x0=ptr(x0), noise=ptr(noise), mask=ptr(mask), dprev=ptr(b["dprev"]), xin=ptr(b["xin"]), ld_xin=ld,
                timesteps=ptr(b["tf"]), table=ptr(table_d), ctr=ptr(b["ctr"]), n=n, hw=h * w, table_rows=40, init=0)
    keep = b["x"].clone()
    for seeds, code in ((None, -1), (ptr(words) + 2, -2), (ptr(words) + 1, -2)):                  # SDLT_ERR_SHAPE, SDLT_ERR_ALIGN
        p = _lib.SamplerSdeParams(seeds=seeds, **base)
        assert lib.sdlt_sampler_step_sde(C.byref(p), None) == code and b"sdlt_sampler_step_sde" in lib.sdlt_last_error()
    torch.cuda.synchronize()
    assert torch.equal(b["x"], keep)


def test_four_entry_points_share_counter_init_and_tail():
    """ONE counter and ONE timestep buffer, stepped by the four entry points in turn, a whole trajectory each (tables of the same step count, the same
    noise, eps and init operands): every trajectory leaves the counter at [0, 0] and the table's wrap-around timestep for the next one.  The Euler
    entry equals sdlt_sampler_step_img without a mask and without skipped steps, the multistep entry equals the stochastic one on a table whose d
    column is zero, bit for bit: init and the ticket tail serve every form alike."""
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w, ld, k, g = 3, 24, 40, 64, 3, 7.5                                   # 2880 pixels: 12 workgroups, both image boundaries inside one
    dev = "cuda"
    euler, ms = SM.EulerDiscrete().set_timesteps(k, 0), SM.DpmSolverPP2M().set_timesteps(k, 0, "trailing")
    tab4, tab4i, tab8 = (t.to(dev) for t in (SM.step_table(euler, g), SM.step_table_img(euler, g), SM.step_table_ms(ms, g)))
    assert bool((tab8[:, 7] == 0).all()) and float(tab8[3, 6]) != 0.0 and torch.equal(tab4[:, 3], tab8[:, 3])
    wrap = float(tab4[2 + k - 1, 3])
    assert wrap == float(tab4[0, 3])
    gen = torch.Generator().manual_seed(24)
    noise, zero = torch.randn(n, 4, h, w, generator=gen).to(dev), torch.zeros(n, 4, h, w, device=dev)
    eps = [torch.randn(2 * n * h * w, 4, generator=gen).to(dev) for _ in range(k)]
    words = _words(SEEDS3)
    ctr, tf = torch.tensor([2, 0], dtype=torch.int32, device=dev), torch.full((2 * n,), -1.0, device=dev)
    runs = dict(euler=(ops.sampler_step, tab4, lambda s, init: dict(noise=noise) if init else {}),
                img=(ops.sampler_step_img, tab4i, lambda s, init: dict(x0=zero, noise=noise, init=init)),
                ms=(ops.sampler_step_ms, tab8, lambda s, init: dict(dprev=s["dprev"], x0=zero, noise=noise, init=init)),
                sde=(ops.sampler_step_sde, tab8, lambda s, init: dict(dprev=s["dprev"], seeds=words, x0=zero, noise=noise, init=init)))
    out = {}
    for name, (op, table, kw) in runs.items():
        s = _trajectory_state(n, h, w, ld, dev)
        op(None, s["x"], s["xin"], tf, table, ctr, **kw(s, True))
        for i in range(k):
            torch.cuda.synchronize()
            assert ctr.cpu().tolist() == [i, 0], (name, i)
            op(eps[i], s["x"], s["xin"], tf, table, ctr, **kw(s, False))
        torch.cuda.synchronize()
        assert ctr.cpu().tolist() == [0, 0] and torch.equal(tf.cpu(), torch.full((2 * n,), wrap)), name
        assert bool(torch.isfinite(s["x"]).all()) and bool((s["xin"][:, 4:] == SENT).all()), name
        out[name] = s
    for a, b in (("euler", "img"), ("ms", "sde")):
        assert torch.equal(out[a]["x"], out[b]["x"]) and torch.equal(out[a]["xin"].view(torch.int16), out[b]["xin"].view(torch.int16)), (a, b)
    assert torch.equal(out["ms"]["dprev"], out["sde"]["dprev"]) and not torch.equal(out["euler"]["x"], out["ms"]["x"])


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
H, W, STEPS = 8, 12, 5
COMBOS = [(kind, sig, case) for kind in KINDS for sig in ("trailing", "karras") for case in ("txt2img", "masked")]


def _half_mask(n=1):
    m = torch.ones(n, 1, H, W)
    m[..., : W // 2] = 0
    return m


def test_graph_fused_and_batch_independence():
    """n = 2 images together: graph == fused bit for bit; the same seeds on the same captured graph repeat the bits (the counter wrapped to row 0);
    another seed changes them; image 0 does not see image 1's seed."""
    cfg, sd, lora, smp = _setup("tinyxl", n=2)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 2)
    em = _cuda(embeds)
    half = _half_mask()

    def run(path, kind, sig, case, seeds, **kw):
        img = dict(init_latents=x0.cuda(), strength=0.8, mask=half.cuda()) if case == "masked" else {}
        return smp.sample(em, H, W, steps=STEPS, guidance_scale=8.0, latents=noise.cuda(), n_images=2, sampler=kind, sigmas=sig, seeds=seeds,
                          **{path: True}, **img, **kw).cpu()

    for kind, sig, case in COMBOS:
        gr = run("graph", kind, sig, case, [7, 8])
        assert bool(torch.isfinite(gr).all()) and torch.equal(gr, run("fused", kind, sig, case, [7, 8])), (kind, sig, case)
        assert torch.equal(run("graph", kind, sig, case, [7, 8]), gr), (kind, sig, case)                    # same seeds, same capture: same bits
        other = run("graph", kind, sig, case, [7, 9])
        assert torch.equal(other[0], gr[0]) and not torch.equal(other[1], gr[1]), (kind, sig, case)          # image 0 does not depend on image 1's seed
        assert not torch.equal(run("graph", kind, sig, case, [6, 8])[0], gr[0])
        assert not torch.equal(run("graph", kind, sig, case, [7, 8], eta=0.5), gr)
        if case == "masked":
            assert torch.equal(gr[..., : W // 2], x0.expand(2, -1, -1, -1)[..., : W // 2]) and not torch.equal(gr[..., W // 2:], x0.expand(2, -1, -1, -1)[..., W // 2:])
    # both samplers, both schedules, eta and the step count live in the table: one capture without a mask, one with; the other dicts are untouched
    assert len(smp._sde_graphs) == 2 and len(smp._ms_graphs) == 0 and len(smp._graphs) == 0 and len(smp._img_graphs) == 0
    ms = smp.sample(em, H, W, steps=STEPS, guidance_scale=8.0, latents=noise.cuda(), n_images=2, sampler="dpmpp_2m", graph=True).cpu()
    assert torch.equal(run("graph", "dpmpp_2m_sde", "trailing", "txt2img", [7, 8], eta=0.0), ms) and len(smp._ms_graphs) == 1 and len(smp._sde_graphs) == 2


def test_torch_loop_equals_fused_equals_graph():
    cfg, sd, lora, smp = _setup("tinyxl", n=1)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    em = _cuda(embeds)[0]
    half = _half_mask()
    for kind, sig, case in COMBOS:
        img = dict(init_latents=x0.cuda(), strength=0.8, mask=half.cuda()) if case == "masked" else {}
        out = [smp.sample(em, H, W, steps=STEPS, guidance_scale=8.0, latents=noise.cuda(), sampler=kind, sigmas=sig, seeds=[21], **path, **img).cpu()
               for path in ({}, dict(fused=True), dict(graph=True))]
        assert bool(torch.isfinite(out[0]).all()) and torch.equal(out[0], out[1]) and torch.equal(out[1], out[2]), (kind, sig, case)
        if case == "masked":
            assert torch.equal(out[0][..., : W // 2], x0[..., : W // 2])


@pytest.mark.parametrize("version,kind,sig,case", [("tinyxl", "euler_a", "trailing", "txt2img"), ("tinyxl", "dpmpp_2m_sde", "karras", "txt2img"),
                                                   ("tinyxl", "dpmpp_2m_sde", "karras", "masked"), ("tiny15", "euler_a", "trailing", "masked")])
def test_fused_against_published_loop(version, kind, sig, case):
    """The fused path against k-diffusion's loop as published (tests/sde_ref.py) in fp32, driven by the oracle UNet and fed the kernel's own noise, at
    the bars tests/test_multistep_gpu.py holds dpmpp_2m to.  Measured on the MI355X (cos / rel-L2), in the order of the cases: 0.999296 / 0.0376, 0.999360 / 0.0359,
    0.999425 / 0.0340, 0.999520 / 0.0310."""
    from sd_lora_trainer_amd import ops
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    seed, img, dimg, mask = 33, {}, {}, None
    if case == "masked":
        mask = (torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(2)) * 3).floor() / 2          # 0, 0.5 and 1
        img = dict(init_latents=x0, strength=1.0, mask=mask)
        dimg = dict(init_latents=x0.cuda(), strength=1.0, mask=mask.cuda())
    zs = [ops.sampler_noise(_words([seed]), i, torch.zeros(1, 4, H, W, device="cuda")).cpu() for i in range(STEPS)]
    ref = SR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, STEPS, zs, sampler=kind, sigmas=sig, **img)
    got = smp.sample(_cuda(embeds)[0], H, W, steps=STEPS, guidance_scale=8.0, latents=noise.cuda(), fused=True, sampler=kind, sigmas=sig, seeds=[seed], **dimg).cpu()
    assert bool(torch.isfinite(got).all())
    cos, rel = _figures(got, ref)
    print(f"{version} {kind} {sig} {case}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, kind, sig, case, cos, rel)
    if mask is not None:
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(got[keep], x0[keep])
    # the noise is what the reference was given: the published loop without it ends further away than the one with it
    ref0 = SR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, STEPS, [torch.zeros_like(z) for z in zs], sampler=kind, sigmas=sig, **img)
    rel0 = _figures(got, ref0)[1]
    print(f"    against the same loop without the noise: rel {rel0:.4f}")
    assert rel0 > rel


# ---- render --sampler euler_a / dpmpp_2m_sde -------------------------------------------------------------------------------------------
def test_render_cli_stochastic(tmp_path, monkeypatch):
    import json
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="sde job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    Wp, Hp = 96, 64
    base = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--prompt", "a drawing of <concept>", "--size", str(Wp), str(Hp), "--steps", "6"]
    ea = ["--sampler", "euler_a", "--eta", "1"]
    runs = dict(ea=ea + ["--seed", "11"], ea_again=ea + ["--seed", "11"], ea_batch=ea + ["--seed", "11", "--images-per-batch", "2"],
                ea_seed=ea + ["--seed", "12"], ea_eta=["--sampler", "euler_a", "--eta", "0.5", "--seed", "11"], euler=["--seed", "11"],
                sde=["--sampler", "dpmpp_2m_sde", "--sigmas", "karras", "--seed", "11"])
    outs = {}
    for tag, extra in runs.items():
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(base + extra + ["--out", outs[tag]])
    names = lambda s: [f"img_00_seed{s}_scale0.85.jpg", f"img_01_seed{s + 1}_scale0.85.jpg"]  # noqa: E731
    for tag in outs:
        want = names(12 if tag == "ea_seed" else 11)
        assert sorted(f for f in os.listdir(outs[tag]) if f.endswith(".jpg")) == sorted(want + ["grid_scale0.85.jpg"]), tag
        assert Image.open(os.path.join(outs[tag], want[0])).size == (Wp, Hp)
    raw = {tag: [open(os.path.join(d, f), "rb").read() for f in names(12 if tag == "ea_seed" else 11)] for tag, d in outs.items()}
    assert raw["ea"] == raw["ea_again"]                                         # the same --seed: byte-identical files
    for a, b in (("ea", "ea_seed"), ("ea", "ea_eta"), ("ea", "euler"), ("sde", "euler"), ("sde", "ea")):
        assert raw[a][0] != raw[b][0] and raw[a][1] != raw[b][1], (a, b)
    meta = json.load(open(os.path.join(outs["ea"], "prompts.json")))
    assert meta["sampler"] == "euler_a" and meta["eta"] == 1.0 and "eta" not in json.load(open(os.path.join(outs["euler"], "prompts.json")))
    assert json.load(open(os.path.join(outs["sde"], "prompts.json")))["eta"] == 1.0
