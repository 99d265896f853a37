"""Differential diffusion on the MI355X: the sdlt_sampler_step_dd kernel against its contract evaluated in torch on the CPU (tests/diffdiff_ref.py) and
against its sibling entries, bit for bit; LatentSampler.sample(change_map=) on the torch loop, the fused loop and the replayed graph; the fused path
against the fp32 reference loop; and `python -m sd_lora_trainer_amd.render --change-map --mask-blur` end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import diffdiff_ref as DR
from tests.test_img2img_gpu import _cuda, _inputs, _run, _setup
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop

pytestmark = pytest.mark.gpu

SENT = 3.25


def _table(form, pred, steps, start, g):
    from sd_lora_trainer_amd import sampler as SM
    if form == 0:
        return SM.step_table_img(SM.EulerDiscrete(prediction_type=pred).set_timesteps(steps, start), g)
    if form == 1:
        return SM.step_table_ms(SM.DpmSolverPP2M(prediction_type=pred).set_timesteps(steps, start), g)
    return SM.step_table_sde(SM.DpmSolverPP2MSDE(prediction_type=pred, eta=1.0).set_timesteps(steps, start), g)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 24, 40)])       # 35 pixels: a partial block; 3 x 960: 12 blocks, the last-block ticket, j = idx / hw across images
def test_sampler_step_dd_kernel_exact(shape, form, pred):
    """k = 4 step rows: row 0 (i = 0; first order, d != 0), rows 1, 2 (second order, d != 0), row 3 (the last: sigma_next = 0, first order, d = 0).  The hold
    map holds every value 0 .. k + 1 scattered over the pixels, so at each row i the set {0, 1, i, i + 1, i + 2, k, k + 1} is present."""
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w = shape
    steps, strength, g, ld = 5, 0.8, 7.5, 64
    k, start = SM.img2img_steps(steps, strength)
    assert (k, start) == (4, 1)
    tab = _table(form, pred, steps, start, g)
    W = tab.shape[1]
    assert W == (4 if form == 0 else 8) and float(tab[2 + k - 1, 1]) == 0.0
    if form >= 1:
        assert float(tab[2, 6]) == 0.0 and float(tab[3, 6]) != 0.0 and float(tab[4, 6]) != 0.0 and float(tab[5, 6]) == 0.0
    if form == 2:
        assert float(tab[2, 7]) != 0.0 and float(tab[4, 7]) != 0.0 and float(tab[5, 7]) == 0.0
    table = torch.zeros(40, W)
    table[: tab.shape[0]] = tab
    gen = torch.Generator().manual_seed(1000 * n + h + form)
    x0, noise = 0.8 * torch.randn(n, 4, h, w, generator=gen), torch.randn(n, 4, h, w, generator=gen)
    hold = (torch.randperm(n * h * w, generator=gen) % (k + 2)).float().view(n, 1, h, w)
    zero_hold = torch.zeros(n, 1, h, w)
    seeds = SM.seed_words([7 + 2 ** 40 * j for j in range(n)], n)
    dev = "cuda"
    # device state, poisoned: init overwrites x, resets a counter left anywhere; dprev may hold anything before the first step
    x = torch.full((n, 4, h, w), float("nan"), device=dev)
    dprev = torch.full((n, 4, h, w), float("nan"), device=dev)
    xin = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16, device=dev)
    tf = torch.full((2 * n,), -1.0, device=dev)
    ctr = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    table_d, x0_d, noise_d, hold_d, zero_d, seeds_d = table.to(dev), x0.to(dev), noise.to(dev), hold.to(dev), zero_hold.to(dev), seeds.to(dev)
    extra_d = dict(dprev=dprev) if form >= 1 else {}
    if form == 2:
        extra_d["seeds"] = seeds_d
    # the contract, on the CPU
    rx, rdprev = torch.zeros(n, 4, h, w), torch.zeros(n, 4, h, w)
    rxin, rtf, rctr = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16), torch.zeros(2 * n), torch.tensor([2, 0], dtype=torch.int32)
    extra_r = dict(dprev=rdprev) if form >= 1 else {}
    if form == 2:
        extra_r["seeds"] = seeds

    def sibling(eps, sx, sxin, stf, sctr, sdprev, init=False):
        """The form's existing entry, maskless, on copies of the device state."""
        if form == 0:
            return ops.sampler_step_img(eps, sx, sxin, stf, table_d, sctr, x0=x0_d, noise=noise_d, init=init)
        if form == 1:
            return ops.sampler_step_ms(eps, sx, sxin, stf, table_d, sctr, dprev=sdprev, x0=x0_d, noise=noise_d, init=init)
        return ops.sampler_step_sde(eps, sx, sxin, stf, table_d, sctr, dprev=sdprev, seeds=seeds_d, x0=x0_d, noise=noise_d, init=init)

    def compare(what):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), rx), (what, int((x.cpu() != rx).sum()))
        assert torch.equal(xin.cpu().view(torch.int16), rxin.view(torch.int16)), what            # both rows of every pair, columns 4.. untouched
        assert torch.equal(tf.cpu(), rtf) and ctr.cpu().tolist() == rctr.tolist(), (what, tf.cpu(), ctr.cpu())
        if form >= 1 and what != "init":
            assert torch.equal(dprev.cpu(), rdprev), what

    ops.sampler_step_dd(None, x, xin, tf, table_d, ctr, x0=x0_d, noise=noise_d, hold=hold_d, form=form, init=True, **extra_d)
    DR.sampler_step_dd(None, rx, rxin, rtf, table, rctr, x0=x0, noise=noise, hold=hold, form=form, init=True, **extra_r)
    assert rctr.tolist() == [0, 0] and float(rtf[0]) == float(tab[0, 3]) and torch.equal(rx, x0 + noise * tab[0, 1])
    compare("init")
    for i in range(k):
        eps = torch.randn(2 * n * h * w, 4, generator=gen)
        eps_d = eps.to(dev)
        # copies of the state before the step: the sibling entry, and this entry with hold = 0 everywhere
        sib = [t.clone() for t in (x, xin, tf, ctr, dprev)]
        sibling(eps_d, *sib)
        nohold = [t.clone() for t in (x, xin, tf, ctr, dprev)]
        ops.sampler_step_dd(eps_d, nohold[0], nohold[1], nohold[2], table_d, nohold[3], x0=x0_d, noise=noise_d, hold=zero_d, form=form,
                            **dict(extra_d, **(dict(dprev=nohold[4]) if form >= 1 else {})))
        for a, b in zip(sib, nohold):                                                           # hold = 0: the maskless entry's bits, every output
            assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b) or \
                (a is sib[4] and form == 0), i
        z = None
        if form == 2 and float(tab[2 + i, 7]) != 0.0:
            z = ops.sampler_noise(seeds_d, i, torch.empty(n, 4, h, w, device=dev)).cpu()
        ops.sampler_step_dd(eps_d, x, xin, tf, table_d, ctr, x0=x0_d, noise=noise_d, hold=hold_d, form=form, **extra_d)
        DR.sampler_step_dd(eps, rx, rxin, rtf, table, rctr, x0=x0, noise=noise, hold=hold, form=form, z=z, **extra_r)
        assert rctr.tolist() == [(i + 1) % k, 0] and float(rtf[0]) == float(tab[2 + i, 3])
        compare(i)
        # a pixel is x0 + noise * sigma_next bit for bit iff i + 1 < hold; every other pixel has the sibling entry's bits
        kk = x0 + noise * tab[2 + i, 1]
        held = (hold > i + 1).expand_as(x0)
        got, free = x.cpu(), sib[0].cpu()
        assert 0 < int(held.sum()) < held.numel()
        assert torch.equal(got[held], kk[held]) and torch.equal(got[~held], free[~held]) and not bool((free[~held] == kk[~held]).all())
        assert torch.equal(tf.cpu(), sib[2].cpu()) and torch.equal(ctr.cpu(), sib[3].cpu())       # timesteps and counter as the sibling gives
        if form >= 1:
            assert torch.equal(dprev.cpu(), sib[4].cpu())                                         # the history is written as today, held pixels included
    assert ctr.cpu().tolist() == [0, 0]
    keep = (hold == k + 1).expand_as(x0)
    assert int(keep.sum()) > 0 and torch.equal(x.cpu()[keep], x0[keep])                           # hold > steps: held after the last step, the init latents exactly
    assert bool((xin[:, 4:] == SENT).all())


def test_refusals():
    from tests.test_diffdiff_cpu import test_entry_point_validation
    test_entry_point_validation()


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
PATHS = dict(torch={}, fused=dict(fused=True), graph=dict(graph=True))


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde"])
@pytest.mark.parametrize("hw", [(8, 8), (8, 12)])
def test_sampler_invariants(hw, sampler):
    h, w = hw
    cfg, sd, lora, smp = _setup("tiny15")
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]

    def run(path, steps=6, strength=0.5, **kw):
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        return smp.sample(em, h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), sampler=sampler, seeds=[9], init_latents=x0.cuda(), strength=strength,
                          **PATHS[path], **kw).cpu()

    ones, zeros = torch.ones(1, 1, h, w), torch.zeros(1, 1, h, w)
    two = ones.clone()
    two[..., : w // 2] = 0
    ramp = torch.linspace(0, 1, h * w).view(1, 1, h, w)
    out = {}
    for p in PATHS:
        free = run(p)                                                                                      # the maskless img2img call
        assert torch.isfinite(free).all() and not torch.equal(free, x0)
        assert torch.equal(run(p, change_map=zeros), x0), p                                                # (a) everything kept: the init latents, bit for bit
        assert torch.equal(run(p, change_map=zeros, strength=1.0), x0), p
        assert torch.equal(run(p, change_map=ones), free), p                                               # (b) ones: the maskless call's bits
        o = run(p, change_map=two)
        assert torch.equal(o[..., : w // 2], x0[..., : w // 2]), p                                         # (c) the zero region is the init latents
        assert torch.isfinite(o).all() and not torch.equal(o[..., w // 2:], x0[..., w // 2:])
        out[p] = run(p, change_map=ramp)
        assert torch.isfinite(out[p]).all() and not torch.equal(out[p], free) and not torch.equal(out[p], x0)
    assert torch.equal(out["graph"], out["fused"])                                                         # (d) graph == fused, bit for bit
    assert len(smp._dd_graphs) == 1
    for strength, steps, cm in ((0.8, 6, two), (0.5, 10, ramp.flip(3)), (1.0, 4, ramp)):                   # (e) another map, strength, step count: the same capture
        a, b = (run(p, steps=steps, strength=strength, change_map=cm) for p in ("graph", "fused"))
        assert torch.equal(a, b), (strength, steps)
    assert len(smp._dd_graphs) == 1


def test_other_captures_are_left_alone():
    h, w = 8, 12
    cfg, sd, lora, smp = _setup("tinyxl")
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    half = torch.ones(1, 1, h, w)
    half[..., : w // 2] = 0
    run = lambda **kw: smp.sample(em, h, w, steps=6, guidance_scale=8.0, latents=noise.cuda(), graph=True, **kw).cpu()  # noqa: E731
    img = dict(init_latents=x0.cuda(), strength=0.5)
    before = run(), run(**img), run(mask=half.cuda(), **img)
    counts = len(smp._graphs), len(smp._img_graphs)
    dd = run(change_map=half.cuda(), **img)
    assert torch.equal(dd[..., : w // 2], x0[..., : w // 2]) and not torch.equal(dd, before[2])             # a select is not the blend
    after = run(), run(**img), run(mask=half.cuda(), **img)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert (len(smp._graphs), len(smp._img_graphs)) == counts == (1, 2) and len(smp._dd_graphs) == 1


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_fused_against_reference_loop(version):
    h = w = 16
    steps, strength = 10, 0.6                                                                              # 6 steps run, as in tests/test_img2img_gpu.py
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    ramp = torch.linspace(0, 1, h * w).view(1, 1, h, w)
    ref = DR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, init_latents=x0, strength=strength, change_map=ramp)
    got = smp.sample(_cuda(embeds)[0], h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), fused=True, init_latents=x0.cuda(), strength=strength,
                     change_map=ramp.cuda()).cpu()
    assert torch.isfinite(got).all()
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"{version} change map: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, cos, rel)
    assert torch.equal(got[0, :, 0, 0], x0[0, :, 0, 0])


# ---- render --change-map ---------------------------------------------------------------------------------------------------------------
def test_render_with_change_map(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="dd job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    W, H = 96, 64
    rng = np.random.default_rng(0)
    init, half = str(tmp_path / "init.png"), str(tmp_path / "half.png")
    Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(init)
    hv = np.zeros((H, W), dtype=np.uint8)
    hv[:, W // 2:] = 255
    Image.fromarray(hv).save(half)
    name = "img_00_seed11_scale0.85.jpg"
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", str(W), str(H), "--steps", "6", "--seed", "11", "--init-image", init,
              "--strength", "0.5"]
    outs = {}
    for tag, extra in (("soft", ["--change-map", half, "--mask-blur", "1.5"]), ("eager", ["--change-map", half, "--mask-blur", "1.5", "--eager"]),
                       ("hard", ["--change-map", half]), ("img", [])):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(common + extra + ["--out", outs[tag]])
    raw = {k: open(os.path.join(d, name), "rb").read() for k, d in outs.items()}
    assert Image.open(os.path.join(outs["soft"], name)).size == (W, H) and os.path.exists(os.path.join(outs["soft"], "grid_scale0.85.jpg"))
    assert raw["soft"] == raw["eager"] and raw["soft"] != raw["hard"] and raw["hard"] != raw["img"]       # the graph and the eager loop agree
    meta = {k: json.load(open(os.path.join(d, "prompts.json"))) for k, d in outs.items()}
    assert meta["soft"]["change_map"] == dict(file=half, mask_blur=1.5) and meta["hard"]["change_map"] == dict(file=half, mask_blur=0.0)
    assert "change_map" not in meta["img"]
