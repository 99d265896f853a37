"""Heat maps on the MI355X: sdlt_heatmap_accum and sdlt_heatmap_overlay against the fp64 restatement (tests/heatmap_ref.py) under per-element bounds derived
from the kernels, then LatentSampler.sample(heatmap=) on a tiny topology: latents untouched bit for bit, graph == fused bit for bit, one capture for other
columns and weights, the torch loop beside them.

The accumulation's bound, per element: |kernel - fp64| <= C_ACCUM 2^-24 M, with M the magnitude operator of heatmap_ref (the products the kernel forms:
|a_1| + sum |w_k| (|a_k| + |a_1|) per axis, times |scale|, summed over resolutions and calls).  C_ACCUM counts the fp32 roundings on the longest path of one
source value to the output (csrc/heatmap.hip, resample.h's combine<4>): horizontal sum - difference, product, three additions = 5; vertical sum 5; the
sum over 3 resolutions 2 (P = 1: none over positions); scale = weight x (1 / layers): 2; scale x total 1; heat + increment, and the first call's value passes
the second call's addition too: 2.  That is 17; one more covers the second-order terms.  The grids of the test are in power-of-two ratios (as the levels of
every UNet are), so coordinates, fractions and tap weights are exact in fp32 and add nothing.
M is deliberately the kernel's form, not sum |w_k a_k| with w_1 = 1 - w_0 - w_2 - w_3: the kernel sums about the centre tap (differences first, so that a
constant plane comes out exactly), and a rounding of w_k (a_k - a_1) is relative to |w_k| (|a_k| + |a_1|), which sum |w_k a_k| does not bound where a_1
dominates.  M is at most (1 + 2 sum_{k != 1} |w_k|) / |w_1| of the plain form per axis - about 1.4 at t = 0.25, 3 at t = 0.5.
The normalised maps: range = hi - lo, v - lo, the division: 3 roundings, C_NORM = 4 with the second-order terms, relative to |v - lo| / range <= 1 - and
the subtraction's own cancellation makes the absolute error 2^-24 (|v| + |lo|) / range, which the bound carries."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import heatmap_ref as HR
from tests.test_heatmap_cpu import synthetic
from tests.test_img2img_gpu import _cuda, _inputs, _setup

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
C_ACCUM = 18
C_NORM = 4
WEIGHTS = (0.25, 0.75)


@functools.lru_cache(maxsize=None)
def _accum_case(grid):
    """-> entries (CPU), cols, the fp64 maps and magnitudes after two calls with WEIGHTS.  n = 2 with guidance rows: the positive block starts at row 2."""
    from sd_lora_trainer_amd import sampler as SM
    entries, cols = synthetic()
    gh, gw = SM.heat_grid(entries, grid)
    want, mag = np.zeros((2, 3, gh, gw)), None
    for step in (0, 1):
        want, mag = HR.accum_ref(entries, cols.numpy(), step, np.float32(WEIGHTS), want, mag, row_off=2)
    return entries, cols, want, mag


@pytest.mark.parametrize("grid", ["max", "min"])
def test_accum_kernel(grid):
    from sd_lora_trainer_amd import ops
    entries, cols, want, mag = _accum_case(grid)
    dev = [(s.cuda(), h, w, L) for s, h, w, L in entries]
    heat = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
    ctr, wts = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.tensor(WEIGHTS, device="cuda")
    for step in (0, 1):                                                     # the weight comes through the device counter
        ctr[0] = step
        ops.heatmap_accum(dev, cols.cuda(), ctr, wts, heat, row_off=2)
    got = heat.cpu().double().numpy()
    err, bound = np.abs(got - want), C_ACCUM * U24 * mag
    print(f"grid {grid}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, max |map| {float(np.abs(want).max()):.3f}")
    assert (err <= bound).all()
    assert not got[0, 2].any() and not got[1, 1].any() and np.abs(got[0, 0]).max() > 0                # absent tokens stay zero


def test_same_grid_is_the_source_exactly():
    from sd_lora_trainer_amd import ops
    entries, cols = synthetic()
    s, h, w, _ = entries[0]
    heat = torch.zeros(2, 3, h, w, device="cuda")
    ops.heatmap_accum([(s.cuda(), h, w, 1)], cols.cuda(), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(1, device="cuda"), heat, row_off=2)
    planes = s.view(4, h, w, -1)
    assert torch.equal(heat[0, 0].cpu(), planes[2, :, :, 1]) and torch.equal(heat[0, 1].cpu(), planes[2, :, :, 76]) and torch.equal(heat[1, 2].cpu(), planes[3, :, :, 1])


def test_overlay_kernel():
    from sd_lora_trainer_amd import ops
    g = torch.Generator().manual_seed(1)
    heat = torch.randn(2, 3, 4, 6, generator=g)
    heat[1] = 2.5                                                           # a constant image: no division by zero
    cols = torch.tensor([[[3, -1], [-1, -1], [5, 6]], [[1, -1], [2, -1], [-1, -1]]], dtype=torch.int32)      # absent maps in both images
    image = torch.rand(2, 3, 20, 28, generator=g)
    lut = ops.heatmap_colour_table()
    alpha = float(np.float32(0.6))
    norm, out = ops.heatmap_overlay(heat.cuda(), cols.cuda(), image.cuda(), lut.cuda(), alpha=alpha)
    want_norm, want_out, _ = HR.overlay_ref(heat.numpy(), cols.numpy(), image.numpy(), lut.numpy(), alpha)
    norm, out = norm.cpu().double().numpy(), out.cpu().numpy()
    lo, hi = float(heat[0, [0, 2]].min()), float(heat[0, [0, 2]].max())
    bound = C_NORM * U24 * (np.abs(heat.double().numpy()) + abs(lo)) / (hi - lo)
    assert (np.abs(norm - want_norm) <= bound).all() and np.isfinite(norm).all()
    assert not norm[1].any() and not norm[0, 1].any() and norm[0].max() == 1.0 and norm[0, [0, 2]].min() == 0.0
    diff = np.abs(out.astype(np.int32) - want_out.astype(np.int32))
    print(f"overlay: {int((diff > 0).sum())} of {diff.size} levels differ, by at most {int(diff.max())}")
    assert diff.max() <= 1
    plain = (image * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert (out[0, 1] == plain[0]).all() and (out[1, 2] == plain[1]).all()


def test_errors_launch_nothing():
    import ctypes as C
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert lib.sdlt_heatmap_accum(C.byref(_lib.HeatAccumParams()), None) == -1 and b"sdlt_heatmap_accum" in lib.sdlt_last_error()
    assert lib.sdlt_heatmap_overlay(C.byref(_lib.HeatOverlayParams()), None) == -1 and b"sdlt_heatmap_overlay" in lib.sdlt_last_error()


@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
def test_sampler_with_heatmap(sampler):
    """tiny15 at 8 x 12 with guidance, 3 steps: the latents with heatmap= are the bits without, before and after; graph == fused bit for bit, maps included; a
    second graph call with other columns and weights reuses the capture; with the guidance pre-pass on, the torch loop gives the fused path's latents and maps bit for bit."""
    h, w = 8, 12
    cfg, sd, lora, smp = _setup("tiny15")
    embeds, noise, _ = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    kw = dict(steps=3, guidance_scale=8.0, latents=noise.cuda(), sampler=sampler)
    hm = dict(cols=[[[1, 2], [76, -1], [-1, -1]]])
    before = smp.sample(em, h, w, fused=True, **kw).cpu()
    lat_f, heat_f = smp.sample(em, h, w, fused=True, heatmap=hm, **kw)
    after = smp.sample(em, h, w, fused=True, **kw).cpu()
    assert torch.equal(lat_f.cpu(), before) and torch.equal(after, before)
    assert tuple(heat_f.shape) == (1, 3, h, w) and bool(torch.isfinite(heat_f).all()) and float(heat_f[0, 0].abs().max()) > 0 and not bool(heat_f[0, 2].any())
    plain_g = smp.sample(em, h, w, graph=True, **kw).cpu()
    lat_g, heat_g = smp.sample(em, h, w, graph=True, heatmap=hm, **kw)
    assert torch.equal(lat_g.cpu(), before) and torch.equal(plain_g, before) and torch.equal(heat_g, heat_f)
    graphs = smp._ms_graphs if sampler == "dpmpp_2m" else smp._graphs
    assert len(graphs) == 2                                                  # without and with the accumulation
    other = dict(cols=[[[5, -1], [1, 2], [76, -1]]], weights=[0.0, 0.5, 0.5])
    lat_o, heat_o = smp.sample(em, h, w, graph=True, heatmap=other, **kw)
    assert len(graphs) == 2 and torch.equal(lat_o.cpu(), before)             # the same capture: columns and weights are device memory
    assert torch.equal(heat_o, smp.sample(em, h, w, fused=True, heatmap=other, **kw)[1]) and not torch.equal(heat_o[0, 1], heat_g[0, 0])
    assert torch.equal(smp.sample(em, h, w, graph=True, heatmap=hm, **kw)[1], heat_g)
    _, heat_min = smp.sample(em, h, w, graph=True, heatmap=dict(hm, grid="min"), **kw)
    assert tuple(heat_min.shape) == (1, 3, h // 2, w // 2) and len(graphs) == 3
    # the torch loop issues the same launches; with the guidance pre-pass its update is taken in the step kernel's order (sampler.py), so latents and
    # maps are the fused path's bits by contract
    gk = dict(kw, guidance_rescale=0.5)
    lat_l, heat_l = smp.sample(em, h, w, heatmap=other, **gk)
    lat_r, heat_r = smp.sample(em, h, w, fused=True, heatmap=other, **gk)
    assert torch.equal(lat_l, lat_r) and torch.equal(heat_l, heat_r) and not torch.equal(heat_r, heat_o)


def test_two_images_each_read_their_own_rows_and_columns():
    """n = 2 (UNet batch 4, rows uc0 c0 uc1 c1: the positive blocks are 1 and 3) with different prompts, noise and columns per image, graph path.  Each image's
    maps against its own single-image run: the two runs' GEMMs have another M and may tile differently, and their activations are rounded to bf16 (2^-8), so
    the maps are held to a relative L2 of 2 x 2^-8, not to equality; the OTHER image's single run must be far away (a wrong stride or cols row shows there)."""
    h, w = 8, 12
    cfg, sd, lora, smp2 = _setup("tiny15", n=2)
    _, _, _, smp1 = _setup("tiny15")
    embeds, noise, _ = _inputs(cfg, 7, h, w, 2)
    ems = _cuda(embeds)
    cols = [[[1, 2], [40, -1]], [[5, -1], [-1, -1]]]
    kw = dict(steps=3, guidance_scale=8.0)
    lat2, heat2 = smp2.sample(ems, h, w, graph=True, n_images=2, latents=noise.cuda(), heatmap=dict(cols=cols), **kw)
    assert torch.equal(lat2, smp2.sample(ems, h, w, graph=True, n_images=2, latents=noise.cuda(), **kw))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    singles = [smp1.sample(ems[j], h, w, graph=True, latents=noise[j:j + 1].cuda(), heatmap=dict(cols=[cols[j]]), **kw)[1] for j in range(2)]
    crossed = smp1.sample(ems[0], h, w, graph=True, latents=noise[:1].cuda(), heatmap=dict(cols=[cols[1]]), **kw)[1]
    own = [rel(heat2[j:j + 1], singles[j]) for j in range(2)]
    far = rel(heat2[1:2, :1], crossed[:, :1])
    print(f"two images: each against its single-image run, rel {own[0]:.3e} {own[1]:.3e}; image 1 against image 0's rows with its columns {far:.3f}")
    assert max(own) <= 2 * 2.0 ** -8 and far > 0.1 and not bool(heat2[1, 1].any())


def test_accumulated_map_against_the_per_layer_maps():
    """The new launch on the model's own score sums.  With keep_daam_maps every hooked layer also leaves its own S (one more product per layer; the forward's
    results do not move).  Two steps with weights (0, 1): the first adds 0 x total, the map is the second forward's.  Reducing the kept per-layer maps in fp64
    must give it within the accumulation's bound plus the fp32 order in which UNet._daam_forward sums a resolution's L_r layer maps: L_r - 1 additions, each
    rounding relative to at most sum_l |S_l| - so the bound is (C_ACCUM + max_r L_r - 1) 2^-24 M with M taken on sum_l |S_l|."""
    h, w = 8, 12
    cfg, sd, lora, smp = _setup("tinyxl")
    embeds, noise, _ = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    cols = [[[1, 2], [76, -1], [-1, -1]]]
    rt = smp.rt
    rt.keep_daam_maps = True
    try:
        _, heat = smp.sample(em, h, w, fused=True, steps=2, guidance_scale=8.0, latents=noise.cuda(), heatmap=dict(cols=cols, weights=[0.0, 1.0]))
        kept = [S.clone() for _, S in rt.daam]
    finally:
        rt.keep_daam_maps = False
    sums, mags = HR.layer_entries(kept, h, w)
    assert sum(e[3] for e in sums) == len(kept) > 2
    want, _ = HR.accum_ref(sums, np.array(cols), 1, [0.0, 1.0], np.zeros(tuple(heat.shape)), row_off=1, row_stride=2)
    _, mag = HR.accum_ref(mags, np.array(cols), 1, [0.0, 1.0], np.zeros(tuple(heat.shape)), row_off=1, row_stride=2)
    c = C_ACCUM + max(e[3] for e in sums) - 1
    err = np.abs(heat.cpu().double().numpy() - want)
    print(f"per-layer maps: {len(kept)} layers, {[e[3] for e in sums]} per resolution, c = {c}; worst error / bound {float((err / np.maximum(c * U24 * mag, 1e-300)).max()):.3f}")
    assert (err <= c * U24 * mag).all() and np.abs(want[0, 0]).max() > 0 and not want[0, 2].any()


def _metric(got, ref):
    a, b = torch.as_tensor(got).reshape(-1).double(), torch.as_tensor(ref).reshape(-1).double()
    return float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


E2E_COLS = [[[1, 2], [40, -1]]]
# Measured on the MI355X, fused path against sample_maps_ref (tiny topologies, 8 x 12 latent, 3 steps, guidance 8): (cos, rel-L2) of the maps.  The latents of
# the same runs lie at tiny15 0.999469 / 0.0326, tinyxl 0.999300 / 0.0375 - the scores pass through the same bf16 Q and K.  The bars give each measured value
# the margin DESIGN 4.21's latent bars (cos >= 0.999, rel-L2 <= 0.06) have to their own measured values, taken where it is tightest: 0.06 / 0.0363 = 1.65 on
# rel-L2 and 0.001 / 0.000647 = 1.55 on 1 - cos (tinyxl, 3 steps: 0.999353 / 0.0363).
E2E_MEASURED = {("tiny15", "max"): (0.999454, 0.0332), ("tiny15", "min"): (0.999464, 0.0328), ("tinyxl", "max"): (0.999605, 0.0297), ("tinyxl", "min"): (0.999652, 0.0287)}
E2E_BARS = {k: (1.0 - 1.55 * (1.0 - c), 1.65 * r) for k, (c, r) in E2E_MEASURED.items()}


def e2e_metrics(version, grid):
    h, w, steps = 8, 12, 3
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, _ = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    lat, heat = smp.sample(em, h, w, fused=True, steps=steps, guidance_scale=8.0, latents=noise.cuda(), heatmap=dict(cols=E2E_COLS, grid=grid))
    ref_lat, ref = HR.sample_maps_ref(cfg, sd, lora, 0.75, embeds[0], noise, steps, E2E_COLS, grid)
    return _metric(heat.cpu(), ref), _metric(lat.cpu(), ref_lat)


@pytest.mark.parametrize("grid", ["max", "min"])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_maps_against_the_fp32_restatement(version, grid):
    (cos, rel), (lcos, lrel) = e2e_metrics(version, grid)
    bar_cos, bar_rel = E2E_BARS[version, grid]
    print(f"{version} grid {grid}: maps cos {cos:.6f} rel {rel:.4f} (bars {bar_cos:.6f} / {bar_rel:.4f}); latents cos {lcos:.6f} rel {lrel:.4f}")
    assert cos >= bar_cos and rel <= bar_rel


def test_render_writes_the_maps_on_the_device(tmp_path, monkeypatch):
    """render() end to end with the HIP kernels on a job trained here: two prompts as one batch of two images, trigger tokens and a word; the files, their
    shapes, one scale per picture; the hires case maps the second pass's coarsest grid."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_render_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="heat job", seed=3, resolution=128, train_batch_size=1, max_train_steps=2,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    W, H = 128, 64
    base = ["--checkpoint", ckdir, "--prompt", "a photo of <concept> a", "--prompt", "a <concept>", "--size", str(W), str(H), "--steps", "3", "--seed", "11",
            "--images-per-batch", "2"]
    R.main(base + ["--out", str(tmp_path / "plain")])
    R.main(base + ["--out", str(tmp_path / "hm"), "--heatmap", "a"])
    f = 8 * W // np.load(next(str(tmp_path / "hm" / n) for n in sorted(os.listdir(tmp_path / "hm")) if n.endswith("_heat.npy"))).shape[2] // 8
    for i in range(2):
        stem = next(n for n in sorted(os.listdir(tmp_path / "hm")) if n.startswith(f"img_{i:02d}") and "_heat" not in n)[: -len(".jpg")]
        assert open(tmp_path / "hm" / (stem + ".jpg"), "rb").read() == open(tmp_path / "plain" / (stem + ".jpg"), "rb").read()      # the picture did not move
        maps = np.load(tmp_path / "hm" / (stem + "_heat.npy"))
        assert maps.shape == (2, H // f, W // f) and maps.dtype == np.float32 and maps.min() == 0.0 and maps.max() == 1.0 and maps[0].any() and maps[1].any()
        for tag in ("trigger", "a"):
            im = Image.open(tmp_path / "hm" / f"{stem}_heat_{tag}.jpg")
            assert im.size == (W, H) and np.abs(np.asarray(im).astype(int) - np.asarray(Image.open(tmp_path / "hm" / (stem + ".jpg"))).astype(int)).max() > 8
    first = [np.load(tmp_path / "hm" / n) for n in sorted(os.listdir(tmp_path / "hm")) if n.endswith("_heat.npy")]
    assert not np.array_equal(first[0], first[1])                               # each image its own rows and columns
    R.main(base + ["--out", str(tmp_path / "hi"), "--heatmap", "--heatmap-grid", "min", "--hires-size", "192", "96", "--hires-strength", "0.5"])
    maps = np.load(next(str(tmp_path / "hi" / n) for n in sorted(os.listdir(tmp_path / "hi")) if n.endswith("_heat.npy")))
    assert maps.shape == (1, 96 // f // 2, 192 // f // 2)                       # the second pass's latent, one level down (the first pass's would be half of it)
