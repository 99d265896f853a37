"""Heat maps without a GPU: the fp64 restatement against torch's own resampling, the emulated ops against it, the token-position lookup, the colour table,
sample(heatmap=) on the emulated op table (all paths, latents untouched), render()'s files and the CLI's argument errors."""
import json
import os

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import unet_ref as U
from sd_lora_trainer_amd import ops as OPS
from sd_lora_trainer_amd import render as R
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd import topology
from sd_lora_trainer_amd.tokenizer import ClipBpeTokenizer
from tests import freeu_ref as FR
from tests import heatmap_ref as HR
from tests.test_driver_cpu import _tokenizer_dir
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)


def test_reference_resampling_is_torchs():
    bicubic, bilinear = HR.self_check()
    print(f"fp64 axis matrices vs F.interpolate: bicubic {bicubic:.2e}, bilinear {bilinear:.2e}")
    assert bicubic <= 1e-12 and bilinear <= 1e-12


def test_magnitude_operator_dominates_the_weights():
    for n_in, n_out in ((8, 12), (2, 8), (12, 3), (5, 5)):
        W, M = HR.cubic_axis(n_in, n_out)
        assert (M >= np.abs(W) - 1e-15).all() and np.allclose(W.sum(1), 1.0, atol=1e-14)


def synthetic(seed=0, n=2, grids=((8, 12), (4, 6), (2, 3)), layers=(3, 2, 1)):
    g = torch.Generator().manual_seed(seed)
    entries = [(torch.randn(2 * n * h * w, unet_mod.CTX_PAD, generator=g) * 3.0, h, w, L) for (h, w), L in zip(grids, layers)]
    cols = torch.tensor([[[1], [76], [-1]], [[76], [-1], [1]]], dtype=torch.int32)
    return entries, cols


@pytest.mark.parametrize("grid", ["max", "min"])
def test_emulated_accum_is_the_reference_and_reads_the_right_rows(grid):
    entries, cols = synthetic()
    gh, gw = SM.heat_grid(entries, grid)
    heat = torch.zeros(2, 3, gh, gw)
    weights = torch.tensor([0.25, 0.75])
    for step in (0, 1):
        HR.heatmap_accum(entries, cols, torch.tensor([step, 0], dtype=torch.int32), weights, heat, row_off=2)
    # by hand: weights sum to 1, so the map is the layer mean of the resampled columns of row block n + i
    want = torch.zeros(2, 3, gh, gw, dtype=torch.float64)
    for s, h, w, _ in entries:
        planes = s.double().view(4, h, w, -1)
        for i in range(2):
            for t in range(3):
                c = int(cols[i, t, 0])
                if c >= 0:
                    p = planes[2 + i, :, :, c][None, None]
                    want[i, t] += (p if (h, w) == (gh, gw) else torch.nn.functional.interpolate(p, size=(gh, gw), mode="bicubic", align_corners=False))[0, 0] / 6.0
    assert float((heat.double() - want).abs().max()) <= 1e-5
    assert float(heat[0, 2].abs().max()) == 0.0 and float(heat[1, 1].abs().max()) == 0.0          # absent tokens stay zero


def test_emulated_overlay_scale_absent_and_constant():
    g = torch.Generator().manual_seed(1)
    heat = torch.randn(2, 3, 4, 6, generator=g)
    heat[1] = 2.5                                                           # image 1: a constant map - no division by zero
    cols = torch.tensor([[[3, -1], [-1, -1], [5, 6]], [[1, -1], [2, -1], [-1, -1]]], dtype=torch.int32)
    image = torch.rand(2, 3, 16, 24, generator=g)
    lut = OPS.heatmap_colour_table()
    norm, out = HR.heatmap_overlay(heat, cols, image, lut, alpha=0.6)
    assert tuple(out.shape) == (2, 3, 16, 24, 3) and out.dtype == torch.uint8
    present = torch.stack([norm[0, 0], norm[0, 2]])
    assert float(present.min()) == 0.0 and float(present.max()) == 1.0      # ONE scale over the image's present maps
    assert float(norm[0, 1].abs().max()) == 0.0 and float(norm[1].abs().max()) == 0.0 and bool(torch.isfinite(norm).all())
    plain = (image * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(out[0, 1], plain[0]) and torch.equal(out[1, 2], plain[1])          # an absent token: the untouched picture
    assert not torch.equal(out[0, 0], plain[0])


def test_colour_table():
    lut = OPS.heatmap_colour_table()
    assert tuple(lut.shape) == (256, 3) and lut.dtype == torch.uint8
    assert lut[0].tolist() == [0, 0, 0] and lut[255].tolist() == [255, 255, 255] and lut[85].tolist() == [255, 0, 0] and lut[170].tolist() == [255, 255, 0]
    lum = lut.double() @ torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)
    assert bool((lum[1:] > lum[:-1]).all())                                  # strictly rising luminance
    assert bool((lut[1:].int() >= lut[:-1].int()).all())                     # no channel ever falls


# ---- token positions ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def toks(tmp_path):
    d, _ = _tokenizer_dir(tmp_path)
    a, b = ClipBpeTokenizer.from_files(d), ClipBpeTokenizer.from_files(d)     # SDXL's pair: one vocabulary, another pad token
    for t in (a, b):
        t.add_tokens(["<s0>", "<s1>"])
    return a, b


def test_positions_of_triggers_and_words(toks):
    trig = ["<s0>", "<s1>"]
    n_a = len(toks[0].tokenize_ids("a"))
    names, cols = R.heat_positions(toks, "<s0><s1> a", [], trig)
    assert names == ["trigger"] and cols == [[1, 2] + [-1] * (R.HEAT_P - 2)]                      # at the front: right after bos
    names, cols = R.heat_positions(toks, "a <s0><s1> a", ["a"], trig)
    assert names == ["trigger", "a"] and cols[0][:3] == [1 + n_a, 2 + n_a, -1]                   # in the middle
    assert cols[1][: 2 * n_a] == list(range(1, 1 + n_a)) + list(range(3 + n_a, 3 + 2 * n_a))     # both occurrences of the word
    word = next(w for w in ("photograph", "beach", "zzqx", "abcdefgh") if len(toks[0].tokenize_ids(w)) > 1)
    k = len(toks[0].tokenize_ids(word))
    _, cols = R.heat_positions(toks, f"<s0> {word}", [word], trig)
    assert cols[1][: k + 1] == list(range(2, 2 + k)) + [-1]                                      # a word of several BPE pieces: all of them
    with pytest.warns(UserWarning, match="not in the prompt"):
        _, cols = R.heat_positions(toks, "<s0><s1> a", [word], trig)
    assert cols[1] == [-1] * R.HEAT_P                                                            # an absent word
    # the 77-token cut: the row keeps 75 ids - a trigger at id 74 is position 75, the next one is gone
    filler = " ".join(["a"] * 80)
    n_f = len(toks[0].tokenize_ids("a"))
    assert n_f == 1, "the toy vocabulary holds 'a' as one piece"
    _, cols = R.heat_positions(toks, " ".join(["a"] * 74) + " <s0><s1>", [], trig)
    assert cols == [[75] + [-1] * (R.HEAT_P - 1)]
    with pytest.warns(UserWarning, match="not in the prompt"):
        _, cols = R.heat_positions(toks, filler + " <s0><s1>", [], trig)
    assert cols == [[-1] * R.HEAT_P]
    _, one = R.heat_positions(toks[:1], "a <s0><s1> a", ["a"], trig)
    _, two = R.heat_positions(toks, "a <s0><s1> a", ["a"], trig)
    assert one == two                                                                            # SDXL's two tokenizers agree


def test_heatmap_args():
    assert SM.heatmap_args(None, 1) is None
    hm = SM.heatmap_args(dict(cols=[[1, 2]]), 1, 4)
    assert tuple(hm["cols"].shape) == (1, 2, 1) and hm["cols"].dtype == torch.int32 and hm["grid"] == "max" and hm["weights"].tolist() == [0.25] * 4
    for bad in (dict(cols=[[1]], grid="mid"), dict(cols=[[77]]), dict(cols=[[-2]]), dict(cols=[1]), dict(cols=[[1.0]]), dict(grid="max"), dict(cols=[[1]], what=1),
                dict(cols=[[1], [2]])):
        with pytest.raises(ValueError, match="heatmap"):
            SM.heatmap_args(bad, 1, 4)
    with pytest.raises(ValueError, match="weights"):
        SM.heatmap_args(dict(cols=[[1]], weights=[1.0]), 1, 4)


# ---- the sampler on the emulated op table ------------------------------------------------------------------------------------------------------
def _sampler(version, ops):
    cfg = U.CONFIGS[version]
    sd, lora = U.init_unet_state(cfg, seed=0), U.init_lora(cfg, 4, seed=1, b_std=0.05)
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    embeds = (mk(1, 77, cfg["cross_dim"]), mk(1, 77, cfg["cross_dim"])) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None))
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=ops)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=4)
    unet.arena.load(lora)
    return SM.LatentSampler(rt, unet), embeds, mk(1, 4, 8, 12)


def test_op_table_without_the_kernel_refuses():
    smp, embeds, noise = _sampler("tiny15", FR.emu_freeu)
    with pytest.raises(NotImplementedError, match="heatmap_accum"):
        smp.sample(embeds, 8, 12, steps=1, latents=noise, heatmap=dict(cols=[[1]]))


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sample_with_heatmap_leaves_the_latents_and_is_the_mean_of_the_score_sums(version):
    """3 steps at 8 x 12: latents with heatmap= are the bits without; torch loop and fused loop give the same maps; the maps are the reference applied to the
    score sums the forwards left (recorded by a spy), weights 1 / 3 by default and as given."""
    seen = []

    def spy(entries, cols, ctr, weights, heat, **kw):
        seen.append(([(s.clone(), h, w, L) for s, h, w, L in entries], int(ctr[0]), kw))
        return HR.heatmap_accum(entries, cols, ctr, weights, heat, **kw)

    table = HR.with_heat(FR.emu_freeu, "emu_heat_spy")
    table.heatmap_accum = spy
    smp, embeds, noise = _sampler(version, table)
    kw = dict(steps=3, guidance_scale=8.0, latents=noise)
    plain = smp.sample(embeds, 8, 12, **kw)
    cols = [[[1, 2], [76, -1], [-1, -1]]]
    lat, heat = smp.sample(embeds, 8, 12, heatmap=dict(cols=cols, grid="min"), **kw)
    assert torch.equal(lat, plain)
    assert [s[1] for s in seen] == [0, 1, 2] and all(s[2] == dict(row_off=1, row_stride=2) for s in seen)
    gh, gw = seen[0][0][-1][1:3]
    assert tuple(heat.shape) == (1, 3, gh, gw) and (gh, gw) == min((e[1], e[2]) for e in seen[0][0])
    want = np.zeros((1, 3, gh, gw))
    for entries, step, _ in seen:
        want, _ = HR.accum_ref(entries, np.array(cols), step, [1 / 3] * 3, want, row_off=1, row_stride=2)
    assert float(np.abs(heat.double().numpy() - want).max()) <= 1e-5 * float(np.abs(want).max()) and float(heat[0, 2].abs().max()) == 0.0
    assert float(heat[0, 0].abs().max()) > 0.0
    seen.clear()
    lat_f, heat_f = smp.sample(embeds, 8, 12, heatmap=dict(cols=cols, grid="min"), fused=True, **kw)
    assert float((lat_f - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    assert float((heat_f - heat).abs().max()) <= 1e-4 * float(heat.abs().max()) and [s[1] for s in seen] == [0, 1, 2]
    lat_w, heat_w = smp.sample(embeds, 8, 12, heatmap=dict(cols=cols, weights=[0.0, 0.0, 1.0]), fused=True, **kw)
    fine = seen[-1][0][0][1:3]                                                                     # grid "max": the finest hooked resolution
    last = HR.accum_ref(seen[-1][0], np.array(cols), 0, [1.0], np.zeros((1, 3) + fine), row_off=1, row_stride=2)[0]
    assert tuple(heat_w.shape) == (1, 3) + fine and fine == max((e[1], e[2]) for e in seen[-1][0]) and torch.equal(lat_w, lat_f)
    assert float(np.abs(heat_w.double().numpy() - last).max()) <= 1e-4 * float(np.abs(last).max())
    assert torch.equal(smp.sample(embeds, 8, 12, **kw), plain)                                     # and a plain call afterwards is the plain call


# ---- render() and the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_arguments(tmp_path, capsys):
    import unittest.mock as mock
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--heatmap-grid", "min"], "--heatmap-grid needs --heatmap"), (["--heatmap", "--heatmap-grid", "mid"], "--heatmap-grid"),
                       (["--heatmap", " "], "non-empty")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert "heatmap" not in seen and "heatmap_grid" not in seen                 # without the flag render() is called as before
        R.main(base + ["--heatmap"])
        assert seen["heatmap"] == [] and seen["heatmap_grid"] == "max"
        R.main(base + ["--heatmap", "beach", "sand", "--heatmap-grid", "min"])
        assert seen["heatmap"] == ["beach", "sand"] and seen["heatmap_grid"] == "min"


def test_render_writes_the_maps(job, tmp_path):  # noqa: F811
    """The files beside each picture, their shapes, the metadata; a hires render maps the second pass's grid; a checkpoint without trigger tokens and no word is
    an error that says so."""
    from PIL import Image
    from tests.test_hires_cpu import _resize_planes
    config, ckdir = job
    table = HR.with_heat(FR.emu_freeu, "emu_heat_hires")
    table.resize_planes = _resize_planes
    rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept> a", "--size", "32", "32", "--steps", "2", "--seed", "5"]
    R.main(common + ["--out", str(tmp_path / "plain")], runtime=rt())
    with pytest.warns(UserWarning, match="not in the prompt"):
        R.main(common + ["--out", str(tmp_path / "hm"), "--heatmap", "a", "zzqx"], runtime=rt())
    files = sorted(os.listdir(tmp_path / "hm"))
    pic = next(f for f in files if f.startswith("img_00") and "_heat" not in f)
    stem = pic[: -len(".jpg")]
    assert {stem + "_heat_trigger.jpg", stem + "_heat_a.jpg", stem + "_heat_zzqx.jpg", stem + "_heat.npy"} <= set(files)
    assert open(tmp_path / "hm" / pic, "rb").read() == open(tmp_path / "plain" / pic, "rb").read()      # the picture itself did not move
    maps = np.load(tmp_path / "hm" / (stem + "_heat.npy"))
    assert maps.shape == (3, 8, 8) and maps.dtype == np.float32 and maps.min() == 0.0 and maps.max() == 1.0 and not maps[2].any()
    assert Image.open(tmp_path / "hm" / (stem + "_heat_a.jpg")).size == (32, 32)
    assert open(tmp_path / "hm" / (stem + "_heat_zzqx.jpg"), "rb").read() == open(tmp_path / "hm" / pic, "rb").read()      # an absent word: the plain picture
    meta = json.load(open(tmp_path / "hm" / "prompts.json"))["heatmap"]
    assert meta["maps"] == ["trigger", "a", "zzqx"] and meta["grid"] == "max" and meta["positions"][0][2] == [-1] * R.HEAT_P
    R.main(common + ["--out", str(tmp_path / "hi"), "--heatmap", "--heatmap-grid", "min", "--hires-size", "48", "48", "--hires-strength", "0.5"], runtime=rt())
    maps = np.load(tmp_path / "hi" / (stem + "_heat.npy"))
    assert maps.shape == (1, 6, 6)                                          # the second pass: a 12 x 12 latent, its coarsest hooked grid (the first pass would give 4 x 4)
    loaded = R.load_for_inference(ckdir, runtime=rt())
    loaded.config.disable_ti = True
    with pytest.raises(ValueError, match="no trigger tokens"):
        R.render(loaded, ["a"], str(tmp_path / "none"), size=(32, 32), steps=1, heatmap=[])
