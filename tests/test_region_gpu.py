"""Regional prompts on the MI355X: sdlt_region_gather / sdlt_region_blend against their contracts in torch (tests/region_ref.py), bit for
bit; sdlt_region_noise against the fp64 Philox / Box-Muller reference; LatentSampler.sample(regions=) on the torch loop, the fused loop and the replayed
graph; the fused path against the reference trajectory (the fp32 oracle UNet on every region's rows, fused in fp64); and
`python -m sd_lora_trainer_amd.render --region` end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import region_ref as RR
from tests.test_img2img_gpu import _cuda, _inputs, _run
from tests.test_region_cpu import H, W, hard_masks, soft_masks
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop
from tests.test_sde_gpu import NOISE_TOL, SEEDS3, _words     # the bar of the transcendental step of the noise
from tests.test_tilediff_gpu import PATHS, _setup

pytestmark = pytest.mark.gpu

SENT = 3.25
# the smallest shapes that cross a wave's 64-x boundary, leave a ragged last y block, put R at its cap and have n > 1
SHAPES = [(1, 1, 5, 7), (1, 2, 12, 20), (2, 3, 9, 65), (1, 5, 4, 130), (1, 16, 3, 3)]


def _masks(R, h, w, gen):
    m = torch.rand(max(R - 1, 0), h, w, generator=gen)
    return ((m * (m > 0.3)) * (0.9 / max(R - 1, 1) + 0.3)).clamp_(0.0, 1.0)      # soft, overlapping, on both sides of 0.5, some pixels background only


def _rtab(rows):
    from sd_lora_trainer_amd import ops
    tab = torch.zeros(ops.REGION_TABLE_ROWS, 2)
    tab[:, 0] = -1.0
    for i, s in rows.items():
        tab[i, 0], tab[i, 1] = s, float(np.float32(1.0 / np.sqrt(np.float64(np.float32(s)) ** 2 + 1.0)))
    return tab


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [64, 8])
@pytest.mark.parametrize("n,R,H_,W_", SHAPES)
def test_region_kernels_exact(n, R, H_, W_, ld):
    from sd_lora_trainer_amd import ops
    dev = "cuda"
    gen = torch.Generator().manual_seed(1000 * H_ + W_ + R)
    tabs_c = ops.region_tables(H_, W_, _masks(R, H_, W_, gen), base=0.1)
    tabs = tabs_c._replace(wn=tabs_c.wn.to(dev), wraw=tabs_c.wraw.to(dev))
    B = 2 * n * R
    x_full = torch.randn(2 * n * H_ * W_, ld, generator=gen).to(torch.bfloat16)         # every column carries data: whole rows travel
    tf = torch.arange(2 * n, dtype=torch.float32) * 7.0 + 3.0
    x_full_d, tf_d = x_full.to(dev), tf.to(dev)
    seeds = _words((SEEDS3 * 2)[:n])
    bg = torch.randn(n, R, 4, generator=gen) * 0.5
    rtab = _rtab({0: 14.6, 5: 3.25, 999: 0.5})
    boot = lambda i: dict(bg=bg.to(dev), rtab=rtab.to(dev), ctr=torch.tensor([i, 7], dtype=torch.int32, device=dev), seeds=seeds)  # noqa: E731
    # no bootstrap pointers; a mid-table row that bootstraps; a row with sigma < 0; the last row; a counter outside the table (clamped to row 999)
    for case, i in (("copy", None), ("mid", 5), ("off", 6), ("last", 999), ("past", 5000)):
        x_r = torch.full((B * H_ * W_, ld), SENT, dtype=torch.bfloat16, device=dev)
        tf_r = torch.full((B,), -1.0, device=dev)
        bt = None if i is None else boot(i)
        ops.region_gather(tabs, x_full_d, x_r, tf_d, tf_r, n=n, H=H_, W=W_, boot=bt)
        ref_boot = None
        if i is not None:
            row = min(i, 999)
            z = torch.zeros(n, R, 4, H_, W_)
            for r in range(1, R):                                                           # the launch's own z: the kernel's noise through the same device function
                z[:, r] = ops.region_noise(seeds, row, r, torch.full((n, 4, H_, W_), float("nan"), device=dev)).cpu()
            ref_boot = dict(wraw=tabs_c.wraw, bg=bg, sigma=rtab[row, 0], inv=rtab[row, 1], z=z)
            assert bt["ctr"].tolist() == [i, 7]                                             # a gather launch does not write the counter
        rx, rtf = RR.gather_ref(x_full, tf, n, R, H_, W_, ref_boot)
        torch.cuda.synchronize()
        got = x_r.cpu()
        assert torch.equal(got.view(torch.int16), rx.view(torch.int16)), (case, int((got.view(torch.int16) != rx.view(torch.int16)).sum()))
        assert torch.equal(tf_r.cpu(), rtf), case
        plain = RR.gather_ref(x_full, tf, n, R, H_, W_)[0]
        changed = not torch.equal(got.view(torch.int16), plain.view(torch.int16))
        assert changed == (case in ("mid", "last", "past") and R > 1 and bool((tabs_c.wraw[1:] < 0.5).any())), case
    assert torch.equal(x_full_d.cpu().view(torch.int16), x_full.view(torch.int16))      # the source is left alone
    eps = torch.randn(B * H_ * W_, 4, generator=gen)
    eps_full = torch.full((2 * n * H_ * W_, 4), float("nan"), device=dev)
    ops.region_blend(tabs, eps.to(dev), eps_full, n=n, H=H_, W=W_)
    ref = RR.blend32(eps, tabs_c.wn, n, R, H_, W_)
    torch.cuda.synchronize()
    got = eps_full.cpu()
    assert torch.isfinite(got).all()                                                    # every row written: no NaN of the poison is left
    assert torch.equal(got, ref), int((got != ref).sum())
    again = torch.full_like(eps_full, float("nan"))
    ops.region_blend(tabs, eps.to(dev), again, n=n, H=H_, W=W_)
    assert torch.equal(again.cpu(), got)                                                # repeats bit for bit


def test_region_noise():
    from sd_lora_trainer_amd import ops
    n, h, w = 3, 9, 13                                                           # 351 threads: two workgroups, both image boundaries inside the first
    words = _words(SEEDS3)
    worst, outs = 0.0, {}
    for step, region in ((0, 1), (3, 1), (3, 2), (999, 15)):
        z = ops.region_noise(words, step, region, torch.full((n, 4, h, w), float("nan"), device="cuda")).cpu()
        ref = np.stack([RR.noise(s, step, region, h * w).reshape(4, h, w) for s in SEEDS3])
        assert bool(torch.isfinite(z).all())
        worst = max(worst, float(np.abs(z.double().numpy() - ref).max()))
        outs[(step, region)] = z
    print(f"sdlt_region_noise: max |z - fp64 reference| = {worst:.3e} (bar {NOISE_TOL:.3e})")
    assert worst <= NOISE_TOL
    assert not torch.equal(outs[(3, 1)], outs[(3, 2)]) and not torch.equal(outs[(0, 1)], outs[(3, 1)])      # region and step both key the draw
    # never the stochastic samplers' draw for the same seed, step and pixel - region 0 included
    sde = ops.sampler_noise(words, 3, torch.zeros(n, 4, h, w, device="cuda")).cpu()
    for region in (0, 1):
        z = ops.region_noise(words, 3, region, torch.zeros(n, 4, h, w, device="cuda")).cpu()
        assert int((z == sde).sum()) <= 1, region                                # (1404 values: bit-different, up to one chance meeting of two fp32 normals)
    alone = ops.region_noise(_words(SEEDS3[1:2]), 3, 1, torch.zeros(1, 4, h, w, device="cuda")).cpu()
    assert torch.equal(alone[0], outs[(3, 1)][1])                                                           # the image's seed, not its place in the batch


def test_refusals_launch_nothing():
    from tests.test_region_cpu import check_refusals
    check_refusals()            # (made-up addresses: a launch would fault)
    torch.cuda.synchronize()


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
R3 = 3


def _regions(cfg, n=1, masks=None, seed=21, **kw):
    masks = soft_masks() if masks is None else masks
    em = _cuda(_inputs(cfg, seed, H, W, n * masks.shape[0])[0])
    per = [em[j * masks.shape[0]:(j + 1) * masks.shape[0]] for j in range(n)]
    return dict(masks=masks, embeds=per[0] if n == 1 else per, **kw)


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_no_foreground_is_the_plain_path(version):
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, _ = _inputs(cfg, 5, 8, 8, 1)
    em = _cuda(embeds)[0]
    none = dict(masks=torch.zeros(0, 8, 8), embeds=[])
    for p, kw in PATHS.items():
        a = smp.sample(em, 8, 8, steps=4, latents=noise.cuda(), regions=none, **kw).cpu()
        assert torch.equal(a, smp.sample(em, 8, 8, steps=4, latents=noise.cuda(), **kw).cpu()), p
    assert len(smp._graphs) == 1                                                          # the same capture: `regions` adds nothing to the key of a plain pass


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths(version):
    cfg, sd, lora, smp = _setup(version, tiles=R3)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    em = _cuda(embeds)[0]
    bg = torch.randn(1, R3, 4, generator=torch.Generator().manual_seed(4)) * 0.3
    rg = _regions(cfg, bootstrap=2, bg=bg)

    def run(path, steps=6, regions=rg, **kw):
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        return smp.sample(em, H, W, steps=steps, guidance_scale=8.0, latents=noise.cuda(), regions=regions, seeds=[9], **PATHS[path], **kw).cpu()

    fused = run("fused")
    assert torch.isfinite(fused).all() and torch.equal(run("graph"), fused)                                # graph == fused, bit for bit
    assert len(smp._graphs) == 1
    # one capture serves another mask set and another bootstrap length: masks, weights, backgrounds and the bootstrap table are device memory
    for other in (_regions(cfg, masks=hard_masks(), bootstrap=2, bg=bg), dict(rg, bootstrap=0), dict(rg, bootstrap=4)):
        o = run("graph", regions=other)
        assert torch.equal(o, run("fused", regions=other)) and len(smp._graphs) == 1 and not torch.equal(o, fused)
    resc = dict(guidance_rescale=0.5)                                                                      # the pre-pass in use: the torch loop steps in the kernel's order
    for s_kw in (dict(), dict(sampler="dpmpp_2m"), dict(sampler="euler_a")):
        a = run("fused", **resc, **s_kw)
        assert torch.isfinite(a).all()
        assert torch.equal(run("torch", **resc, **s_kw), a), s_kw
        assert torch.equal(run("graph", **resc, **s_kw), a), s_kw
    mask = torch.ones(1, 1, H, W)
    mask[..., : W // 2] = 0
    a = run("fused", init_latents=x0, strength=0.5, mask=mask, **resc)
    assert torch.equal(run("torch", init_latents=x0, strength=0.5, mask=mask, **resc), a) and torch.equal(run("graph", init_latents=x0, strength=0.5, mask=mask, **resc), a)
    assert torch.equal(a[..., : W // 2], x0[..., : W // 2]) and not torch.equal(a[..., W // 2:], x0[..., W // 2:])
    cmap = torch.linspace(0, 1, H * W).view(1, 1, H, W)
    cmap[..., :3] = 0
    b = run("fused", init_latents=x0, strength=0.5, change_map=cmap, **resc)
    assert torch.equal(run("torch", init_latents=x0, strength=0.5, change_map=cmap, **resc), b) and torch.equal(run("graph", init_latents=x0, strength=0.5, change_map=cmap, **resc), b)
    assert torch.equal(b[..., :3], x0[..., :3]) and torch.isfinite(b).all() and not torch.equal(b, a)
    with pytest.raises(ValueError, match="heatmap"):
        run("fused", heatmap=dict(cols=[[1]]))
    with pytest.raises(ValueError, match="tile"):
        run("fused", tile=(8, 2))


def test_two_images_together():
    n = 2
    cfg, sd, lora, smp = _setup("tinyxl", n=n, tiles=R3)
    assert (smp.n, smp.tiles, smp.rt.B) == (2, R3, 12)
    embeds, noise, _ = _inputs(cfg, 7, H, W, n)
    em = _cuda(embeds)
    rg = _regions(cfg, n, bootstrap=2)
    outs = [smp.sample(em, H, W, steps=4, latents=noise.cuda(), n_images=n, regions=rg, seeds=[50, 51], **kw).cpu() for kw in (dict(fused=True), dict(graph=True))]
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    assert not torch.equal(outs[0][0], outs[0][1])                                                         # each image has its own noise and prompts
    # the conditioning layout, bit for bit: UNet batch row 2 (R j + r) + s carries image j's negative (s = 0) | region r's positive (s = 1) rows
    from sd_lora_trainer_amd.unet import CTX_PAD
    cv, pv = smp.ctx.view(n, R3, 2, CTX_PAD, -1), smp.pooled.view(n, R3, 2, -1)
    for j in range(n):
        _, uc, _, puc = em[j]
        for r in range(R3):
            c, _, pc, _ = em[j] if r == 0 else rg["embeds"][j][r - 1]
            assert torch.equal(cv[j, r, 0, :77], uc[0].to(cv.dtype)) and torch.equal(cv[j, r, 1, :77], c[0].to(cv.dtype)), (j, r)
            assert torch.equal(pv[j, r, 0], puc[0].to(pv.dtype)) and torch.equal(pv[j, r, 1], pc[0].to(pv.dtype)), (j, r)
    one = _setup("tinyxl", n=1, tiles=R3)[3]
    for j in range(n):                         # and is the image it would be alone (to bf16 rounding: a product's route, hence its bits, may follow the batch)
        alone = one.sample(em[j], H, W, steps=4, latents=noise[j:j + 1].cuda(), regions=dict(rg, embeds=rg["embeds"][j]), seeds=[50 + j], fused=True).cpu()
        rel = float((alone - outs[0][j:j + 1]).norm() / alone.norm())
        print(f"image {j}: alone vs together rel {rel:.5f}")
        assert rel <= TOL_REL, (j, rel)


@pytest.mark.parametrize("boot", [0, 2])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_fused_against_reference_trajectory(version, sampler, boot):
    """The fused path against tests/region_ref.py's trajectory at tests/test_sampler_gpu.py's bars."""
    steps, strength = 10, 0.6                                                                              # 6 steps run, as in tests/test_sampler_gpu.py
    cfg, sd, lora, smp = _setup(version, tiles=R3)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    bg = torch.randn(1, R3, 4, generator=torch.Generator().manual_seed(4)) * 0.3
    reg_embeds = _inputs(cfg, 21, H, W, R3 - 1)[0]
    ref = RR.sample_latents(cfg, sd, lora, 0.75, embeds[0], reg_embeds, soft_masks(), noise, steps, bootstrap=boot, bg=bg[0], seed=31, sampler=sampler,
                            init_latents=x0, strength=strength)
    got = smp.sample(_cuda(embeds)[0], H, W, steps=steps, guidance_scale=8.0, latents=noise.cuda(), fused=True, sampler=sampler, init_latents=x0.cuda(),
                     strength=strength, seeds=[31], regions=dict(masks=soft_masks(), embeds=_cuda(reg_embeds), bootstrap=boot, bg=bg)).cpu()
    assert torch.isfinite(got).all()
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"{version} {sampler} bootstrap={boot}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, sampler, boot, cos, rel)


# ---- render --region -------------------------------------------------------------------------------------------------------------------
def test_render_regions(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="region job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    ld = R.load_for_inference(ckdir)
    f = 2 ** (len(ld.stack.decoder.ups) - 1)
    size = (f * W, f * H)
    name = "img_00_seed11_scale0.85.jpg"
    mask_png = str(tmp_path / "mask.png")
    arr = np.zeros((size[1], size[0]), dtype=np.uint8)
    arr[size[1] // 2:, : size[0] // 2] = 255
    Image.fromarray(arr).save(mask_png)
    common = ["--checkpoint", ckdir, "--prompt", "a photo of a field", "--steps", "4", "--seed", "11", "--size", str(size[0]), str(size[1])]
    rg = ["--region", "0.5,0,1,1", "a photo of <concept>", "--region", mask_png, "a red barn", "--region-feather", "1.0", "--region-base", "0.1"]
    out = str(tmp_path / "regions")
    R.main(common + rg + ["--out", out])
    meta = json.load(open(os.path.join(out, "prompts.json")))
    assert meta["regions"] == [dict(prompt="a photo of <concept>", box=[0.5, 0.0, 1.0, 1.0]), dict(prompt="a red barn", mask=mask_png)]
    assert meta["region_base"] == 0.1 and meta["region_bootstrap"] == 0.2 and meta["region_feather"] == 1.0
    assert sorted(os.listdir(out)) == sorted([name, "grid_scale0.85.jpg", "prompts.json"])
    img = np.asarray(Image.open(os.path.join(out, name)))
    assert img.shape == (size[1], size[0], 3) and img.std() > 0
    plain = str(tmp_path / "plain")
    R.main(common + ["--out", plain])
    assert "regions" not in json.load(open(os.path.join(plain, "prompts.json")))
    assert open(os.path.join(plain, name), "rb").read() != open(os.path.join(out, name), "rb").read()
    # one loaded checkpoint: the graph and the eager loop agree; another mask set and bootstrap share keeps the UNet, its sampler and the capture
    regions = [((0.5, 0.0, 1.0, 1.0), "a photo of <concept>"), (mask_png, "a red barn")]
    outs = {}
    for tag, kw in (("graph", {}), ("eager", dict(graph=False))):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.render(ld, ["a photo of a field"], outs[tag], size=size, steps=4, seed=11, regions=regions, region_feather=1.0, region_base=0.1, **kw)
    raw = {k: open(os.path.join(d, name), "rb").read() for k, d in outs.items()}
    assert raw["graph"] == raw["eager"] == open(os.path.join(out, name), "rb").read()
    smp = ld.stack.sampler
    assert (smp.n, smp.tiles) == (1, 3) and len(smp._graphs) == 1
    R.render(ld, ["a photo of a field"], str(tmp_path / "other"), size=size, steps=4, seed=11, regions=[((0.0, 0.0, 0.4, 1.0), "a tree"), ((0.6, 0.0, 1.0, 0.5), "a cloud")],
             region_bootstrap=0.5)
    assert ld.stack.sampler is smp and len(smp._graphs) == 1
    assert open(os.path.join(tmp_path, "other", name), "rb").read() != raw["graph"]
