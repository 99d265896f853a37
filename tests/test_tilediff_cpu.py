"""Tiled diffusion without a GPU: the window plan and tables against their restatement (tests/tilediff_ref.py), the weights' sum, blend32's
rounding bound, the identity that lets the prediction be fused before the step (fp64), the refusals, the entry points' argument checks, the sampler and
render() on an emulated op table, and the CLI."""
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd import topology
from tests import guidance_ref as GR
from tests import tilediff_ref as TD
from tests.test_hires_cpu import _resize_planes
from tests.test_img2img_cpu import EMB, _Stub
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)

GEOMETRY = [(1, 5, 7, 4, 1), (2, 13, 24, 8, 4), (1, 6, 20, 8, 2), (1, 70, 150, 64, 16)]      # (n, H, W, T, O): the GPU file's cases

emu_plain = GR.emu_guidance                                   # every sampler family and the guidance pre-pass, no window launches
emu_window = TD.emu_table(emu_plain)
emu_window.resize_planes = _resize_planes


# ---- plan and tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,T,O", GEOMETRY)
def test_plan_and_tables(n, H, W, T, O):
    g = TD.geometry(H, W, T, O)
    plan = SM.tile_plan(H, W, (T, O))
    assert tuple(plan) == (T, O, g.th, g.tw, g.ty, g.tx)
    tabs, ref = ops.window_tables(H, W, T, O), TD.tables(H, W, T, O)
    assert (tabs.th, tabs.tw, tabs.ty, tabs.tx) == ref[4:]
    for a, b in zip(tabs[:4], ref[:4]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert g.ys[0] == 0 and g.ys[-1] + g.th == H and g.xs[0] == 0 and g.xs[-1] + g.tw == W      # no window reaches outside the grid
    # the products of the windows that cover a sample sum to 1
    total = torch.zeros(H, W, dtype=torch.float64)
    for iy, y0 in enumerate(g.ys):
        for ix, x0 in enumerate(g.xs):
            total[y0:y0 + g.th, x0:x0 + g.tw] += tabs.wy[iy].double()[:, None] * tabs.wx[ix].double()[None, :]
    assert float((total - 1.0).abs().max()) <= 2.0 ** -23


def test_known_plans():
    assert TD.geometry(13, 24, 8, 4).ys == [0, 3, 5] and TD.coverage(13, 24, 8, 4) >= 3        # samples 5..7 of the y axis lie in three windows
    assert tuple(SM.tile_plan(12, 20, (8, 2))) == (8, 2, 8, 8, 2, 3)
    assert tuple(SM.tile_plan(6, 20, 8)) == (8, 2, 6, 8, 1, 3)                                # one window on the y axis, th = H < T; O defaults to T // 4
    assert tuple(SM.tile_plan(128, 512, 128)) == (128, 32, 128, 128, 1, 5)                    # an SDXL 4096 x 1024 px panorama
    for h, w, tile in ((8, 8, 8), (8, 8, (8, 2)), (5, 7, 16), (16, 16, None), (64, 3, (64, 32))):
        assert SM.tile_plan(h, w, tile) is None, (h, w, tile)                                  # a pass that fits one window is the plain path


@pytest.mark.parametrize("bad", [(8, 5), 1, (8, -1), (0, 0), "64", (64,), (64.0, 16), True, (8, 2, 1)])
def test_bad_plans(bad):
    with pytest.raises(ValueError, match="window"):
        SM.tile_plan(32, 32, bad)


def test_too_many_windows():
    with pytest.raises(ValueError, match="at most 64"):
        SM.tile_plan(8, 2000, (8, 0))


# ---- blend32 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,T,O", GEOMETRY)
def test_blend32_of_one_field_returns_it(n, H, W, T, O):
    """Windows cut from one field fuse back to it: the weights sum to 1 up to one rounding per weight, and blend32 rounds once per product, per multiply
    and per add - (k + 3) 2^-24 max|v| with k the largest number of windows over a sample."""
    gen = torch.Generator().manual_seed(H * 1000 + W)
    field = torch.randn(2 * n * H * W, 4, generator=gen)
    tiles, _ = TD.gather(field, torch.zeros(2 * n), n, H, W, T, O)
    k = TD.coverage(H, W, T, O)
    back = TD.blend32(tiles, n, H, W, T, O)
    err = float((back.double() - field.double()).abs().max())
    bound = (k + 3) * 2.0 ** -24 * float(field.abs().max())
    print(f"({n}, {H}, {W}, {T}, {O}): k = {k}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # and against the fp64 fusion with the same tables
    ref = TD.blend64(tiles, n, H, W, T, O, rounded_weights=True)
    assert float((back.double() - ref).abs().max()) <= (k + 2) * 2.0 ** -24 * float(field.abs().max())


def test_emulated_launches_are_the_contract():
    n, H, W, T, O = 2, 13, 24, 8, 4
    gen = torch.Generator().manual_seed(3)
    tabs = ops.window_tables(H, W, T, O)
    B = 2 * n * tabs.ty * tabs.tx
    x_full, tf = torch.randn(2 * n * H * W, 64, generator=gen).to(torch.bfloat16), torch.arange(2 * n, dtype=torch.float32) + 100.0
    x_tiles, tf_tiles = torch.zeros(B * tabs.th * tabs.tw, 64, dtype=torch.bfloat16), torch.zeros(B)
    TD.emu_window_gather(tabs, x_full, x_tiles, tf, tf_tiles, n=n, H=H, W=W)
    rx, rt = TD.gather(x_full, tf, n, H, W, T, O)
    assert torch.equal(x_tiles.view(torch.int16), rx.view(torch.int16)) and torch.equal(tf_tiles, rt)
    eps = torch.randn(B * tabs.th * tabs.tw, 4, generator=gen)
    out = TD.emu_window_blend(tabs, eps, torch.full((2 * n * H * W, 4), float("nan")), n=n, H=H, W=W)
    assert torch.equal(out, TD.blend32(eps, n, H, W, T, O))


# ---- the identity: fuse the predictions, then step == step every window, then fuse -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["euler", "dpmpp_2m"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_fuse_then_step_is_step_then_fuse(kind, pred):
    H, W, T, O = 13, 24, 8, 4
    cls = SM.EulerDiscrete if kind == "euler" else SM.DpmSolverPP2M
    sig = np.array([14.6, 6.1, 2.2, 0.7, 0.0], dtype=np.float64)
    full, wins = cls(prediction_type=pred).set_sigmas(sig), cls(prediction_type=pred).set_sigmas(sig)
    gen = torch.Generator().manual_seed(11)
    g = TD.geometry(H, W, T, O)
    rows = 2 * g.ty * g.tx * g.th * g.tw
    xa = xb = torch.randn(2 * H * W, 4, generator=gen, dtype=torch.float64) * sig[0]
    tf = torch.zeros(2, dtype=torch.float64)
    for i in range(len(sig) - 1):
        eps = torch.randn(rows, 4, generator=gen, dtype=torch.float64)             # every window predicts something else
        xa = full.step(TD.blend64(eps, 1, H, W, T, O), i, xa)                      # this project: one prediction for the whole latent, one step
        xw, _ = TD.gather(xb, tf, 1, H, W, T, O)                                   # the paper: every window stepped from the fused latent, then averaged
        xb = TD.blend64(wins.step(eps, i, xw), 1, H, W, T, O)
        assert float((xa - xb).abs().max()) <= 1e-12, (i, float((xa - xb).abs().max()))


# ---- the sampler on the emulated table ------------------------------------------------------------------------------------------------------------
def _unet(version, B, table, rank=4):
    from oracle import unet_ref as U
    cfg = U.CONFIGS[version]
    sd = U.init_unet_state(cfg, seed=0)
    lora = U.init_lora(cfg, rank, seed=1, b_std=0.05)
    rt = unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=table)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    return cfg, sd, lora, rt, unet


def _embeds(cfg, seed, n):
    g = torch.Generator().manual_seed(seed)
    D = cfg["cross_dim"]
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return [(mk(1, 77, D), mk(1, 77, D)) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None)) for _ in range(n)]


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths_and_reference_on_the_emulated_table(version):
    h, w, tile, steps = 12, 20, (8, 2), 4
    plan = SM.tile_plan(h, w, tile)
    cfg, sd, lora, rt, unet = _unet(version, 2 * plan.ty * plan.tx, emu_window)
    smp = SM.LatentSampler(rt, unet, n_images=1)
    assert (smp.n, smp.tiles) == (1, 6)
    smp.set_lora_scale(0.75)
    em = _embeds(cfg, 5, 1)[0]
    gen = torch.Generator().manual_seed(9)
    noise, x0 = torch.randn(1, 4, h, w, generator=gen), 0.8 * torch.randn(1, 4, h, w, generator=gen)
    mask = (torch.rand(1, 1, h, w, generator=gen) * 3).floor() / 2
    run = lambda **kw: smp.sample(em, h, w, steps=steps, latents=noise.clone(), tile=tile, **kw)  # noqa: E731
    fused = run(fused=True)
    ref = TD.sample_latents(cfg, sd, lora, 0.75, em, noise, steps, tile)
    torch.testing.assert_close(fused, ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    # the torch loop with the guidance pre-pass in use takes the step in the kernel's order: the fused path's bits
    kw = dict(guidance_rescale=0.5)
    assert torch.equal(run(**kw), run(fused=True, **kw))
    for sampler_ in ("dpmpp_2m", "euler_a"):
        a = run(fused=True, sampler=sampler_, seeds=[4], **kw)
        assert torch.isfinite(a).all() and torch.equal(a, run(sampler=sampler_, seeds=[4], **kw))
    # a mask at full size: the kept pixels are the init latents exactly
    out = run(fused=True, init_latents=x0, strength=0.5, mask=mask)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(out[keep], x0[keep]) and torch.isfinite(out).all()
    ref = TD.sample_latents(cfg, sd, lora, 0.75, em, noise, steps, tile, init_latents=x0, strength=0.5, mask=mask)
    torch.testing.assert_close(out, ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    # another overlap with the same window counts: the same persistent buffers
    assert SM.tile_plan(h, w, (8, 1))[2:] == plan[2:]
    assert len(smp._fused["shapes"]) == 1
    smp.sample(em, h, w, steps=2, latents=noise.clone(), tile=(8, 1), fused=True)
    assert len(smp._fused["shapes"]) == 1


def test_freeu_and_kv_downsample_act_per_window():
    """Both live inside the UNet: with windows they run at the window's grid, and their factor checks see that grid."""
    from tests import freeu_ref as FR
    from tests import kvpool_ref as KR
    table = TD.emu_table(emu_window, "emu_window_opts")
    table.freeu, table.freeu_tables, table.freeu_ws_floats = FR.freeu, FR.freeu_tables, FR.freeu_ws_floats
    table.token_pool, table.token_pool_rows = KR.token_pool, KR.token_pool_rows
    h, w, tile = 12, 20, (8, 2)
    cfg, sd, lora, rt, unet = _unet("tiny15", 12, table)
    smp = SM.LatentSampler(rt, unet, n_images=1)
    em = _embeds(cfg, 5, 1)[0]
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(9))
    run = lambda **kw: smp.sample(em, h, w, steps=2, latents=noise.clone(), tile=tile, **kw)  # noqa: E731
    plain = run(fused=True)
    for kw in (dict(freeu=(1.3, 1.4, 0.9, 0.2)), dict(kv_downsample=(2,)), dict(kv_downsample=(2,), kv_downsample_mode="area", freeu=(1.3, 1.4, 0.9, 0.2))):
        a = run(fused=True, **kw)
        assert torch.isfinite(a).all() and not torch.equal(a, plain), kw
        assert torch.equal(run(guidance_rescale=0.5, **kw), run(fused=True, guidance_rescale=0.5, **kw)), kw      # the torch loop too
        smp.sample(em, h, w, steps=1, latents=noise.clone(), tile=tile, fused=True, kv_downsample=())               # (off again for the next case)
    assert torch.equal(run(fused=True), plain)                                                                     # and both off: the plain bits
    with pytest.raises(ValueError, match="does not fit the 8 x 8"):                                              # the window's grid, not the 12 x 20 latent's
        run(fused=True, kv_downsample=(16,))


def test_single_window_is_the_plain_path():
    cfg, sd, lora, rt, unet = _unet("tiny15", 2, emu_plain)                       # (no window launch needed: nothing is cut)
    smp = SM.LatentSampler(rt, unet)
    em = _embeds(cfg, 5, 1)[0]
    noise = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    for kw in (dict(), dict(fused=True)):
        assert torch.equal(smp.sample(em, 8, 8, steps=3, latents=noise.clone(), tile=(8, 2), **kw), smp.sample(em, 8, 8, steps=3, latents=noise.clone(), **kw))


def test_two_images_are_sampled_as_each_alone():
    h, w, tile, n = 12, 20, (8, 2), 2
    outs = {}
    for k in (1, n):
        cfg, sd, lora, rt, unet = _unet("tinyxl", 2 * k * 6, emu_window)
        smp = SM.LatentSampler(rt, unet, n_images=k)
        ems = _embeds(cfg, 5, n)
        noise = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(2))
        if k == 1:
            outs[k] = torch.cat([smp.sample(ems[j], h, w, steps=3, latents=noise[j:j + 1].clone(), tile=tile, fused=True) for j in range(n)])
        else:
            outs[k] = smp.sample(ems, h, w, steps=3, latents=noise.clone(), tile=tile, fused=True, n_images=n)
    torch.testing.assert_close(outs[1], outs[n], rtol=1e-4, atol=1e-4)               # (a CPU matrix product's bits may follow the batch it runs in)
    assert not torch.equal(outs[n][0], outs[n][1])


def test_refusals():
    h, w = 12, 20
    stub = _Stub(1, h, w, 7)
    stub.cfg = dict(stub.cfg, block_out_channels=(64, 128, 128))
    smp = SM.LatentSampler(unet_mod.Runtime("cpu", 12, act_dtype=torch.float32, ops=emu_window), stub, n_images=1)
    noise = torch.zeros(1, 4, h, w)
    with pytest.raises(ValueError, match="heatmap"):
        smp.sample(EMB, h, w, steps=2, latents=noise, tile=(8, 2), heatmap=dict(cols=[[1]]))
    with pytest.raises(ValueError, match="overlap"):
        smp.sample(EMB, h, w, steps=2, latents=noise, tile=(8, 5))
    with pytest.raises(ValueError, match="multiple of 4"):
        smp.sample(EMB, h, w, steps=2, latents=noise, tile=(6, 1))                 # a 6 x 6 window: the tiny UNets halve the grid twice
    with pytest.raises(ValueError, match="6 window"):                              # the runtime was built for 2 x 3 windows: a plain call and another plan
        smp.sample(EMB, 8, 8, steps=2, latents=torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="the call needs 12"):
        smp.sample(EMB, 16, 24, steps=2, latents=torch.zeros(1, 4, 16, 24), tile=(8, 2), fused=True)
    assert stub.calls == 0
    bare = SM.LatentSampler(unet_mod.Runtime("cpu", 12, act_dtype=torch.float32, ops=emu_plain), stub, n_images=1)
    for kw in (dict(), dict(fused=True)):
        with pytest.raises(NotImplementedError, match="sdlt_window_blend"):        # no torch fallback
            bare.sample(EMB, h, w, steps=2, latents=noise, tile=(8, 2), **kw)
    assert stub.calls == 0


# ---- the entry points' checks (nothing is launched: no GPU here) ----------------------------------------------------------------------------------
def lib_window(lib, which, **kw):
    """sdlt_window_gather / sdlt_window_blend on made-up addresses, one argument changed: n = 1, a 10 x 11 grid, 2 x 2 windows of 6 x 7."""
    from sd_lora_trainer_amd import _lib
    a = dict(dict(ys=0x1000, xs=0x2000, wy=0x3000, wx=0x4000, n=1, H=10, W=11, th=6, tw=7, ty=2, tx=2,
                  x_full=0x100000, x_tiles=0x200000, ld=64, tf_full=0x5000, tf_tiles=0x6000, eps_tiles=0x300000, eps_full=0x400000), **kw)
    p = None
    if not a.get("null_block"):
        p = _lib.WindowParams(**{k: a[k] for k in ("ys", "xs", "wy", "wx", "n", "H", "W", "th", "tw", "ty", "tx")})
    ref = None if p is None else __import__("ctypes").byref(p)
    if which == "gather":
        return lib.sdlt_window_gather(ref, a["x_full"], a["x_tiles"], a["ld"], a["tf_full"], a["tf_tiles"], None)
    return lib.sdlt_window_blend(ref, a["eps_tiles"], a["eps_full"], None)


SHARED_REFUSALS = [dict(null_block=True), dict(ys=None), dict(xs=None), dict(n=0), dict(H=0), dict(W=-1), dict(th=0), dict(tw=-2), dict(ty=0), dict(tx=0),
                   dict(ty=65), dict(tx=65), dict(H=16385), dict(W=16385), dict(n=32768),
                   dict(n=32767, H=16384, W=16384, th=16384, tw=16384, ty=64, tx=64), dict(th=11), dict(tw=12), dict(ys=0x1002), dict(xs=0x2001)]
GATHER_REFUSALS = [dict(x_full=None), dict(x_tiles=None), dict(tf_full=None), dict(tf_tiles=None), dict(ld=0), dict(ld=60), dict(ld=-8), dict(ld=4104), dict(ld=1 << 20), dict(x_full=0x100008),
                   dict(x_tiles=0x200004), dict(tf_full=0x5002), dict(x_tiles=0x100000), dict(x_tiles=0x100000 + 2 * 10 * 11 * 128 - 16),
                   dict(x_full=0x200000 + 8 * 42 * 128 - 16)]
BLEND_REFUSALS = [dict(wy=None), dict(wx=None), dict(eps_tiles=None), dict(eps_full=None), dict(eps_tiles=0x300008), dict(eps_full=0x400004), dict(wy=0x3001),
                  dict(eps_full=0x300000), dict(eps_full=0x300000 + 8 * 42 * 16 - 16), dict(eps_tiles=0x400000 + 2 * 110 * 16 - 16)]


def check_refusals():
    """Every refusal returns a negative code, names the entry point and launches nothing (the addresses are made up: a launch would fault).  Also called
    by the GPU file."""
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_window_gather" in _lib.SYMBOLS and "sdlt_window_blend" in _lib.SYMBOLS
    for which, own in (("gather", GATHER_REFUSALS), ("blend", BLEND_REFUSALS)):
        for change in SHARED_REFUSALS + own:
            assert lib_window(lib, which, **change) < 0, (which, change)
            assert f"sdlt_window_{which}".encode() in lib.sdlt_last_error(), (which, change, lib.sdlt_last_error())
    # gather does not read the weights: null is fine there, so the first refusal it meets is the next one in line
    assert lib_window(lib, "gather", wy=None, wx=None, x_full=None) == -1 and b"null pointer" in lib.sdlt_last_error()


def test_entry_point_validation():
    check_refusals()


def test_wrappers_check_shapes():
    tabs = ops.window_tables(12, 20, 8, 2)
    with pytest.raises(AssertionError):
        ops.window_blend(tabs, torch.zeros(10, 4), torch.zeros(10, 4), n=1, H=12, W=20)      # CPU tensors: refused before the library is asked


# ---- render() and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path, capsys):
    import types
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--tile-diffusion-overlap", "8"], "needs --tile-diffusion"), (["--tile-diffusion", "8.5"], "--tile-diffusion"),
                       (["--tile-diffusion", "0"], "window"), (["--tile-diffusion", "1"], "window"), (["--tile-diffusion", "-8"], "window"),
                       (["--tile-diffusion", "8", "--tile-diffusion-overlap", "5"], "overlap"), (["--tile-diffusion", "8", "--tile-diffusion-overlap", "-1"], "overlap"),
                       (["--tile-diffusion", "64", "--heatmap"], "--heatmap")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)                                                          # (the checkpoint does not exist: refused before anything is loaded)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    loaded = types.SimpleNamespace(config=types.SimpleNamespace(resolution=1024))
    with mock.patch.object(R, "load_for_inference", lambda *a, **k: loaded), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert "tile_diffusion" not in seen                                               # without the flag render() is called as before
        R.main(base + ["--tile-diffusion"])
        assert seen["tile_diffusion"] == (128, 32)                                        # the job's resolution // 8, overlap T // 4
        R.main(base + ["--tile-diffusion", "--prompt", "a house"])
        assert seen["tile_diffusion"] == (128, 32)
        R.main(base + ["--tile-diffusion", "96"])
        assert seen["tile_diffusion"] == (96, 24)
        R.main(base + ["--tile-diffusion", "64", "--tile-diffusion-overlap", "32"])
        assert seen["tile_diffusion"] == (64, 32)


def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    assert hasattr(R.encode_image, "__wrapped__") and not hasattr(R.tile_diffusion_default, "__wrapped__")      # the VAE encode runs without autograd, as before
    from tests.test_guidance_cpu import _FakeLoaded
    for bad in ((32, 20), 1, (8, -1), "64", (64.0, 16)):
        with pytest.raises(ValueError, match="window"):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), tile_diffusion=bad)
    assert not os.path.exists(tmp_path / "o")


def test_render_on_the_emulated_table(job, tmp_path, monkeypatch):  # noqa: F811
    """--tile-diffusion end to end: a picture larger than one window, prompts.json, the instances kept at another picture size with the same window
    counts, a hires render whose first pass is plain and whose second is tiled, and an op table without the launches."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    config, ckdir = job
    builds, tiles = [], []
    real_build, real_sample = T.RenderStack.build_sampler, SM.LatentSampler.sample
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n, **kw: (builds.append((n, kw.get("tiles", 1))), real_build(self, n, **kw))[1])
    monkeypatch.setattr(SM.LatentSampler, "sample", lambda self, em, h, w, **kw: (tiles.append((h, w, kw.get("tile"), self.rt.B)), real_sample(self, em, h, w, **kw))[1])
    rt = lambda table=emu_window: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--steps", "2", "--seed", "5"]
    td = ["--tile-diffusion", "8", "--tile-diffusion-overlap", "2"]
    # 80 x 48 px = a 12 x 20 latent of the tiny VAE (factor 4): 2 x 3 windows of 8 x 8
    out = tmp_path / "tiled"
    R.main(common + td + ["--size", "80", "48", "--out", str(out)], runtime=rt())
    meta = json.load(open(out / "prompts.json"))
    assert meta["tile_diffusion"] == dict(tile=8, overlap=2, tiles=[2, 3]) and meta["size"] == [80, 48]
    assert builds == [(1, 1), (1, 6)] and tiles == [(12, 20, (8, 2), 12)]
    name = next(f for f in sorted(os.listdir(out)) if f.startswith("img_00"))
    assert Image.open(out / name).size == (80, 48)
    assert np.isfinite(np.asarray(Image.open(out / name), dtype=np.float64)).all()
    plain = tmp_path / "plain"
    R.main(common + ["--size", "80", "48", "--out", str(plain)], runtime=rt())
    assert "tile_diffusion" not in json.load(open(plain / "prompts.json"))                      # without the flag: the keys as before
    assert open(plain / name, "rb").read() != open(out / name, "rb").read()
    # one loaded checkpoint, two picture sizes with the same window counts: the UNet and its sampler are built once
    ld = R.load_for_inference(ckdir, runtime=rt())
    del builds[:], tiles[:]
    R.render(ld, ["a house"], str(tmp_path / "a"), size=(80, 48), steps=2, tile_diffusion=(8, 2))
    first = ld.stack.sampler
    R.render(ld, ["a house"], str(tmp_path / "b"), size=(76, 44), steps=2, tile_diffusion=(8, 2))    # an 11 x 19 latent: 2 x 3 windows again
    assert ld.stack.sampler is first and builds == [(1, 6)] and [t[:2] for t in tiles] == [(12, 20), (11, 19)]
    assert ld.shape == (1, 8, 8, 2, 3)
    # hires: the first pass at 32 x 32 px fits one window and stays plain, the second at 80 x 48 px is tiled
    del builds[:], tiles[:]
    hires = tmp_path / "hires"
    R.main(common + td + ["--size", "32", "32", "--hires-size", "80", "48", "--hires-strength", "0.5", "--out", str(hires)], runtime=rt())
    assert builds == [(1, 1), (1, 6)] and tiles == [(8, 8, None, 2), (12, 20, (8, 2), 12)]
    meta = json.load(open(hires / "prompts.json"))
    assert meta["tile_diffusion"]["tiles"] == [2, 3] and meta["hires"]["size"] == [80, 48]
    assert Image.open(hires / name).size == (80, 48)
    # a window the UNet's downsampling does not accept, and an op table without the launches: refused, nothing written
    with pytest.raises(ValueError, match="multiple of 4"):
        R.main(common + ["--tile-diffusion", "6", "--size", "80", "48", "--out", str(tmp_path / "none")], runtime=rt())
    with pytest.raises(NotImplementedError, match="sdlt_window_blend"):
        R.main(common + td + ["--size", "80", "48", "--out", str(tmp_path / "none")], runtime=rt(emu_plain))
    assert not os.path.exists(tmp_path / "none")
