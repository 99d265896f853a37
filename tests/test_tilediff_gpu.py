"""Tiled diffusion on the MI355X: sdlt_window_gather / sdlt_window_blend against their contracts in torch (tests/tilediff_ref.py), bit for
bit; LatentSampler.sample(tile=) on the torch loop, the fused loop and the replayed graph; the fused path against the reference trajectory (the fp32
oracle UNet on every window, fused in fp64); and `python -m sd_lora_trainer_amd.render --tile-diffusion` end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import tilediff_ref as TD
from tests.test_img2img_gpu import _cuda, _inputs, _run
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop

pytestmark = pytest.mark.gpu

SENT = 3.25
TILE = (8, 2)            # 12 x 20 -> 2 x 3 windows of 8 x 8: the tiny topologies halve the grid twice, so a window is a multiple of 4
H, W = 12, 20


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H_,W_,T,O", [(1, 5, 7, 4, 1),           # a partial wave, odd extents
                                         (2, 13, 24, 8, 4),         # three windows over samples 5..7 of the y axis; j and s across images
                                         (1, 6, 20, 8, 2),          # one window on the y axis, th = H < T
                                         (1, 70, 150, 64, 16)])     # more than one workgroup per window row, row offsets past a wave
def test_window_kernels_exact(n, H_, W_, T, O):
    from sd_lora_trainer_amd import ops
    dev, ld = "cuda", 64
    tabs = ops.window_tables(H_, W_, T, O, device=dev)
    g = TD.geometry(H_, W_, T, O)
    assert (tabs.th, tabs.tw, tabs.ty, tabs.tx) == (g.th, g.tw, g.ty, g.tx)
    B = 2 * n * g.ty * g.tx
    gen = torch.Generator().manual_seed(1000 * H_ + W_)
    x_full = torch.randn(2 * n * H_ * W_, ld, generator=gen).to(torch.bfloat16)         # every column carries data: whole rows travel
    tf = torch.arange(2 * n, dtype=torch.float32) * 7.0 + 3.0
    x_tiles = torch.full((B * g.th * g.tw, ld), SENT, dtype=torch.bfloat16, device=dev)
    tf_tiles = torch.full((B,), -1.0, device=dev)
    x_full_d = x_full.to(dev)
    ops.window_gather(tabs, x_full_d, x_tiles, tf.to(dev), tf_tiles, n=n, H=H_, W=W_)
    rx, rtf = TD.gather(x_full, tf, n, H_, W_, T, O)
    torch.cuda.synchronize()
    assert torch.equal(x_tiles.cpu().view(torch.int16), rx.view(torch.int16))           # columns 4.. of the copied rows included
    assert torch.equal(tf_tiles.cpu(), rtf)
    assert torch.equal(x_full_d.cpu().view(torch.int16), x_full.view(torch.int16))      # the source is left alone
    eps = torch.randn(B * g.th * g.tw, 4, generator=gen)
    eps_full = torch.full((2 * n * H_ * W_, 4), float("nan"), device=dev)
    ops.window_blend(tabs, eps.to(dev), eps_full, n=n, H=H_, W=W_)
    ref = TD.blend32(eps, n, H_, W_, T, O)
    torch.cuda.synchronize()
    got = eps_full.cpu()
    assert torch.isfinite(got).all()                                                    # every row written: no NaN of the poison is left
    assert torch.equal(got, ref), int((got != ref).sum())
    again = torch.full_like(eps_full, float("nan"))
    ops.window_blend(tabs, eps.to(dev), again, n=n, H=H_, W=W_)
    assert torch.equal(again.cpu(), got)                                                # repeats bit for bit


def test_refusals_launch_nothing():
    from tests.test_tilediff_cpu import check_refusals
    check_refusals()            # (made-up addresses: a launch would fault)
    torch.cuda.synchronize()


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
def _setup(version, n=1, tiles=1, rank=8):
    """tests/test_img2img_gpu.py's _setup on a runtime of batch 2 n tiles."""
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import sampler, topology
    import sd_lora_trainer_amd.unet as M
    cfg = U.CONFIGS[version]
    sd = {k: v.to(torch.bfloat16).float() for k, v in U.init_unet_state(cfg, seed=0).items()}
    lora = {k: (a.to(torch.bfloat16).float(), b.to(torch.bfloat16).float()) for k, (a, b) in U.init_lora(cfg, rank, seed=1, b_std=0.05).items()}
    rt = M.Runtime("cuda:0", 2 * n * tiles)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    smp = sampler.LatentSampler(rt, unet, **({} if tiles == 1 else dict(n_images=n)))
    smp.set_lora_scale(0.75)
    return cfg, sd, lora, smp


PATHS = dict(torch={}, fused=dict(fused=True), graph=dict(graph=True))


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_single_window_is_the_plain_path(version):
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, _ = _inputs(cfg, 5, 8, 8, 1)
    em = _cuda(embeds)[0]
    for p, kw in PATHS.items():
        a = smp.sample(em, 8, 8, steps=4, latents=noise.cuda(), tile=TILE, **kw).cpu()
        assert torch.equal(a, smp.sample(em, 8, 8, steps=4, latents=noise.cuda(), **kw).cpu()), p
    assert len(smp._graphs) == 1                                                          # the same capture: `tile` adds nothing to the key of a plain pass


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths(version):
    from sd_lora_trainer_amd import sampler as SM
    plan = SM.tile_plan(H, W, TILE)
    assert (plan.ty, plan.tx, plan.th, plan.tw) == (2, 3, 8, 8)
    cfg, sd, lora, smp = _setup(version, tiles=6)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    em = _cuda(embeds)[0]

    def run(path, steps=6, tile=TILE, **kw):
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        return smp.sample(em, H, W, steps=steps, guidance_scale=8.0, latents=noise.cuda(), tile=tile, **PATHS[path], **kw).cpu()

    fused = run("fused")
    assert torch.isfinite(fused).all() and torch.equal(run("graph"), fused)                                # graph == fused, bit for bit
    assert len(smp._graphs) == 1
    other = run("graph", tile=(8, 1))                                                                      # another overlap, the same window counts: the same capture
    assert torch.equal(other, run("fused", tile=(8, 1))) and len(smp._graphs) == 1 and not torch.equal(other, fused)
    resc = dict(guidance_rescale=0.5)                                                                      # the pre-pass in use: the torch loop steps in the kernel's order
    for s_kw in (dict(), dict(sampler="dpmpp_2m"), dict(sampler="euler_a", seeds=[9])):
        a = run("fused", **resc, **s_kw)
        assert torch.isfinite(a).all()
        assert torch.equal(run("torch", **resc, **s_kw), a), s_kw
        assert torch.equal(run("graph", **resc, **s_kw), a), s_kw
    mask = torch.ones(1, 1, H, W)
    mask[..., : W // 2] = 0
    a = run("fused", init_latents=x0, strength=0.5, mask=mask)
    assert torch.equal(run("graph", init_latents=x0, strength=0.5, mask=mask), a)
    assert torch.equal(a[..., : W // 2], x0[..., : W // 2]) and not torch.equal(a[..., W // 2:], x0[..., W // 2:])      # the kept half crosses window seams
    cmap = torch.linspace(0, 1, H * W).view(1, 1, H, W)
    cmap[..., :3] = 0
    b = run("fused", init_latents=x0, strength=0.5, change_map=cmap)
    assert torch.equal(run("graph", init_latents=x0, strength=0.5, change_map=cmap), b)
    assert torch.equal(b[..., :3], x0[..., :3]) and torch.isfinite(b).all() and not torch.equal(b, a)
    with pytest.raises(ValueError, match="heatmap"):
        run("fused", heatmap=dict(cols=[[1]]))
    # freeu and kv_downsample act inside the UNet, per window (last: they change the UNet's setting)
    for o_kw in (dict(freeu=(1.3, 1.4, 0.9, 0.2)),) + ((dict(kv_downsample=(2,)),) if version == "tiny15" else ()):      # (tiny15: an 8 x 8 self-attention grid per window)
        c = run("fused", **o_kw)
        assert torch.isfinite(c).all() and not torch.equal(c, fused) and torch.equal(run("graph", **o_kw), c), o_kw


def test_two_images_together():
    n = 2
    cfg, sd, lora, smp = _setup("tinyxl", n=n, tiles=6)
    assert (smp.n, smp.tiles, smp.rt.B) == (2, 6, 24)
    embeds, noise, _ = _inputs(cfg, 7, H, W, n)
    em = _cuda(embeds)
    outs = [smp.sample(em, H, W, steps=4, latents=noise.cuda(), n_images=n, tile=TILE, **kw).cpu() for kw in (dict(fused=True), dict(graph=True))]
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    assert not torch.equal(outs[0][0], outs[0][1])                                                         # each image has its own noise and prompt
    # the conditioning layout, bit for bit: UNet batch row 2 (6 j + t) + s carries image j's negative (s = 0) | positive (s = 1) rows on every window t
    from sd_lora_trainer_amd.unet import CTX_PAD
    cv, pv, tv = smp.ctx.view(n, 6, 2, CTX_PAD, -1), smp.pooled.view(n, 6, 2, -1), smp._fused["tid"].view(n, 6, 2, 6)
    for j in range(n):
        c, uc, pc, puc = em[j]
        for t in range(6):
            assert torch.equal(cv[j, t, 0, :77], uc[0].to(cv.dtype)) and torch.equal(cv[j, t, 1, :77], c[0].to(cv.dtype)), (j, t)
            assert torch.equal(pv[j, t, 0], puc[0].to(pv.dtype)) and torch.equal(pv[j, t, 1], pc[0].to(pv.dtype)), (j, t)
    assert not torch.equal(cv[0, 0, 1], cv[1, 0, 1]) and bool((tv == tv[0, 0, 0]).all()) and tv[0, 0, 0].tolist() == [8.0 * H, 8.0 * W, 0.0, 0.0, 8.0 * H, 8.0 * W]
    one = _setup("tinyxl", n=1, tiles=6)[3]
    for j in range(n):                         # and is the image it would be alone (to bf16 rounding: a product's route, hence its bits, may follow the batch)
        alone = one.sample(em[j], H, W, steps=4, latents=noise[j:j + 1].cuda(), tile=TILE, fused=True).cpu()
        rel = float((alone - outs[0][j:j + 1]).norm() / alone.norm())
        print(f"image {j}: alone vs together rel {rel:.5f}")
        assert rel <= TOL_REL, (j, rel)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_fused_against_reference_trajectory(version, sampler, masked):
    """Measured on the MI355X (profiles/tile_diffusion_render_bench.txt): tiny15 cos 0.99973 .. 0.99979, rel 0.021 .. 0.023; tinyxl cos 0.99941 .. 0.99963,
    rel 0.027 .. 0.035."""
    steps, strength = 10, 0.6                                                                              # 6 steps run, as in tests/test_sampler_gpu.py
    cfg, sd, lora, smp = _setup(version, tiles=6)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    mask = None
    if masked:
        mask = (torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(2)) * 3).floor() / 2        # 0, 0.5 and 1
    ref = TD.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, TILE, sampler=sampler, init_latents=x0, strength=strength, mask=mask)
    got = smp.sample(_cuda(embeds)[0], H, W, steps=steps, guidance_scale=8.0, latents=noise.cuda(), fused=True, tile=TILE, sampler=sampler,
                     init_latents=x0.cuda(), strength=strength, mask=None if mask is None else mask.cuda()).cpu()
    assert torch.isfinite(got).all()
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"{version} {sampler} masked={masked}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, sampler, masked, cos, rel)
    if masked:
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(got[keep], x0[keep])


# ---- render --tile-diffusion -----------------------------------------------------------------------------------------------------------
def test_render_tile_diffusion(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="tile job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    ld = R.load_for_inference(ckdir)
    f = 2 ** (len(ld.stack.decoder.ups) - 1)
    px = lambda h, w: (f * w, f * h)  # noqa: E731
    name = "img_00_seed11_scale0.85.jpg"
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--steps", "4", "--seed", "11"]
    td = ["--tile-diffusion", "8", "--tile-diffusion-overlap", "2"]
    size = [str(v) for v in px(H, W)]
    # the command line: a 12 x 20 latent in 2 x 3 windows
    out = str(tmp_path / "tiled")
    R.main(common + td + ["--size"] + size + ["--out", out])
    meta = json.load(open(os.path.join(out, "prompts.json")))
    assert meta["tile_diffusion"] == dict(tile=8, overlap=2, tiles=[2, 3]) and meta["size"] == list(px(H, W))
    assert sorted(os.listdir(out)) == sorted([name, "grid_scale0.85.jpg", "prompts.json"])
    img = np.asarray(Image.open(os.path.join(out, name)))
    assert img.shape == (f * H, f * W, 3) and img.std() > 0
    plain = str(tmp_path / "plain")
    R.main(common + ["--size"] + size + ["--out", plain])
    assert "tile_diffusion" not in json.load(open(os.path.join(plain, "prompts.json")))
    assert open(os.path.join(plain, name), "rb").read() != open(os.path.join(out, name), "rb").read()
    # one loaded checkpoint: the graph and the eager loop agree; another picture size with the same window counts keeps the UNet and its sampler, and a
    # picture size seen before replays its capture - whatever the overlap
    outs = {}
    for tag, kw in (("graph", {}), ("eager", dict(graph=False))):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.render(ld, ["a photo of <concept>"], outs[tag], size=px(H, W), steps=4, seed=11, tile_diffusion=TILE, **kw)
    raw = {k: open(os.path.join(d, name), "rb").read() for k, d in outs.items()}
    assert raw["graph"] == raw["eager"] == open(os.path.join(out, name), "rb").read()
    smp = ld.stack.sampler
    assert (smp.n, smp.tiles) == (1, 6) and ld.shape == (1, 8, 8, 2, 3) and len(smp._graphs) == 1
    R.render(ld, ["a photo of <concept>"], str(tmp_path / "other"), size=px(H - 1, W - 1), steps=4, seed=11, tile_diffusion=TILE)
    assert ld.stack.sampler is smp and len(smp._graphs) == 2                               # the full shape is part of the key: the step launches run at it
    assert Image.open(os.path.join(tmp_path, "other", name)).size == px(H - 1, W - 1)
    R.render(ld, ["a photo of <concept>"], str(tmp_path / "again"), size=px(H, W), steps=4, seed=11, tile_diffusion=(8, 1))
    assert ld.stack.sampler is smp and len(smp._graphs) == 2
    assert open(os.path.join(tmp_path, "again", name), "rb").read() != raw["graph"]
    # hires: the first pass at the window's size is plain, the second is tiled
    seen = []
    from sd_lora_trainer_amd import sampler as SM
    real = SM.LatentSampler.sample
    monkeypatch.setattr(SM.LatentSampler, "sample", lambda self, em, h, w, **kw: (seen.append((h, w, kw.get("tile"), self.rt.B)), real(self, em, h, w, **kw))[1])
    hires = str(tmp_path / "hires")
    R.main(common + td + ["--size"] + [str(v) for v in px(8, 8)] + ["--hires-size"] + size + ["--hires-strength", "0.5", "--out", hires])
    assert seen == [(8, 8, None, 2), (H, W, TILE, 12)]
    meta = json.load(open(os.path.join(hires, "prompts.json")))
    assert meta["tile_diffusion"]["tiles"] == [2, 3] and meta["hires"]["size"] == list(px(H, W))
    assert Image.open(os.path.join(hires, name)).size == px(H, W)
