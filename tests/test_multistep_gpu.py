"""DPM-Solver++ (2M) on the MI355X: the sdlt_sampler_step_ms kernel against its contract evaluated in torch (bit for bit), the invariants of
LatentSampler.sample(sampler="dpmpp_2m", sigmas=) on the fused loop and the replayed graph, the fused path against the fp32 reference loop
(tests/multistep_ref.py) driven by the oracle UNet, and `python -m sd_lora_trainer_amd.render --sampler dpmpp_2m --sigmas karras` end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import multistep_ref as MR
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop

pytestmark = pytest.mark.gpu

SENT = 3.25


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["txt2img", "x0", "random", "zeros"])         # no x0 / x0 without a mask / x0 and a random mask / x0 and a mask of zeros
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape,kind", [((1, 5, 7), "trailing"), ((3, 24, 40), "karras")])   # 35 pixels: a partial block; 2880: 12 blocks, the ticket, j = idx / hw
def test_sampler_step_ms_kernel_exact(shape, kind, pred, case):
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w = shape
    g, ld, k = 7.5, 64, 4
    steps, start = (k, 0) if case == "txt2img" else (7, 3)                     # img2img: strength 0.6 of 7 steps
    if start:
        assert SM.img2img_steps(steps, 0.6) == (k, start)
    tab = SM.step_table_ms(SM.DpmSolverPP2M(prediction_type=pred).set_timesteps(steps, start, kind), g)
    assert tab.shape == (2 + k, 8) and float(tab[2 + k - 1, 1]) == 0.0 and float(tab[0, 1]) == float(tab[2, 0])
    assert [float(c) != 0.0 for c in tab[2:, 6]] == [False, True, True, False]                 # first order, second, second, first (sigma -> 0)
    table = torch.zeros(40, 8)
    table[: tab.shape[0]] = tab
    gen = torch.Generator().manual_seed(1000 * n + h)
    x0, noise = 0.8 * torch.randn(n, 4, h, w, generator=gen), torch.randn(n, 4, h, w, generator=gen)
    mask = dict(txt2img=None, x0=None, random=torch.rand(n, 1, h, w, generator=gen), zeros=torch.zeros(n, 1, h, w))[case]
    if case == "txt2img":
        x0 = None
    if case == "random":
        mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    eps = [torch.randn(2 * n * h * w, 4, generator=gen) for _ in range(k)]
    dev = "cuda"
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    # device state, poisoned: the init entry overwrites x, resets a counter left anywhere and touches columns 0..3 only; dprev is NaN until a step writes it
    x = torch.full((n, 4, h, w), float("nan"), device=dev)
    dprev = torch.full((n, 4, h, w), float("nan"), device=dev)
    xin = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16, device=dev)
    tf = torch.full((2 * n,), -1.0, device=dev)
    ctr = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    table_d, x0_d, noise_d, mask_d = d(table), d(x0), d(noise), d(mask)
    # the contract, on the CPU
    rx, rd = torch.zeros(n, 4, h, w), torch.full((n, 4, h, w), float("nan"))
    rxin, rtf, rctr = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16), torch.zeros(2 * n), torch.tensor([2, 0], dtype=torch.int32)

    def compare(what, with_d=True):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), rx), (what, int((x.cpu() != rx).sum()))
        if with_d:
            assert torch.equal(dprev.cpu(), rd), (what, int((dprev.cpu() != rd).sum()))
        assert torch.equal(xin.cpu().view(torch.int16), rxin.view(torch.int16)), what            # both rows of every pair, columns 4.. untouched
        assert torch.equal(tf.cpu(), rtf) and ctr.cpu().tolist() == rctr.tolist(), (what, tf.cpu(), ctr.cpu())

    ops.sampler_step_ms(None, x, xin, tf, table_d, ctr, dprev=dprev, x0=x0_d, noise=noise_d, mask=mask_d, init=True)
    MR.sampler_step_ms(None, rx, rxin, rtf, table, rctr, dprev=rd, x0=x0, noise=noise, mask=mask, init=True)
    assert rctr.tolist() == [0, 0] and float(rtf[0]) == float(tab[0, 3])
    compare("init", with_d=False)
    assert bool(torch.isnan(dprev).all())                                                         # the init entry leaves the history alone
    x_init, first = x.clone(), []
    for i in range(k):
        ops.sampler_step_ms(eps[i].to(dev), x, xin, tf, table_d, ctr, dprev=dprev, x0=x0_d, noise=noise_d, mask=mask_d)
        MR.sampler_step_ms(eps[i], rx, rxin, rtf, table, rctr, dprev=rd, x0=x0, noise=noise, mask=mask)
        assert rctr.tolist() == [(i + 1) % k, 0] and float(rtf[0]) == float(tab[2 + i, 3])
        compare(i)
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(dprev).all()), i             # the NaN history was not read by the first-order row
        first.append((x.clone(), dprev.clone(), xin.clone(), tf.clone()))
    assert ctr.cpu().tolist() == [0, 0] and torch.equal(tf.cpu(), torch.full((2 * n,), float(tab[0, 3])))     # back at the start after k steps
    if case == "zeros":
        assert torch.equal(x.cpu(), x0)                                                           # everything kept: the init latents exactly
    if case == "random":
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(x.cpu()[keep], x0[keep])
    # a second trajectory straight after, on the counter the last step wrapped to 0 (no init launch): row 0 is first order again, so the history the
    # first trajectory left is not read, and every step gives the bits it gave before
    x.copy_(x_init)
    for i in range(k):
        ops.sampler_step_ms(eps[i].to(dev), x, xin, tf, table_d, ctr, dprev=dprev, x0=x0_d, noise=noise_d, mask=mask_d)
        torch.cuda.synchronize()
        fx, fd, fxin, ftf = first[i]
        assert torch.equal(x, fx) and torch.equal(dprev, fd) and torch.equal(xin.view(torch.int16), fxin.view(torch.int16)) and torch.equal(tf, ftf), i
        assert ctr.cpu().tolist() == [(i + 1) % k, 0]
    assert bool((xin[:, 4:] == SENT).all())


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
def _setup(version, n=1, rank=8):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import sampler, topology
    import sd_lora_trainer_amd.unet as M
    cfg = U.CONFIGS[version]
    sd = {k: v.to(torch.bfloat16).float() for k, v in U.init_unet_state(cfg, seed=0).items()}
    lora = {k: (a.to(torch.bfloat16).float(), b.to(torch.bfloat16).float()) for k, (a, b) in U.init_lora(cfg, rank, seed=1, b_std=0.05).items()}
    rt = M.Runtime("cuda:0", 2 * n)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    smp = sampler.LatentSampler(rt, unet)
    smp.set_lora_scale(0.75)
    return cfg, sd, lora, smp


def _inputs(cfg, seed, h, w, n):
    g = torch.Generator().manual_seed(seed)
    D = cfg["cross_dim"]
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    embeds = [(mk(1, 77, D), mk(1, 77, D)) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None)) for _ in range(n)]
    return embeds, mk(n, 4, h, w), 0.8 * mk(1, 4, h, w)


def _cuda(embeds):
    return [tuple(None if e is None else e.cuda() for e in em) for em in embeds]


@pytest.mark.parametrize("version", ["tinyxl", "tiny15"])
def test_sampler_invariants(version):
    h = w = 16
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    PATHS = dict(fused=dict(fused=True), graph=dict(graph=True))

    def run(path, steps=6, **kw):
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        return smp.sample(em, h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), **PATHS[path], **kw).cpu()

    MS = dict(sampler="dpmpp_2m")
    zeros, half = torch.zeros(1, 1, h, w), torch.ones(1, 1, h, w)
    half[..., : w // 2] = 0
    euler = run("graph")                                                                                   # a Euler capture first
    assert len(smp._graphs) == 1 and len(smp._img_graphs) == 0 and len(smp._ms_graphs) == 0
    out = {}
    for p in PATHS:
        out[p] = run(p, **MS)
        out[p + "_img"] = run(p, init_latents=x0, strength=0.5, **MS)
        out[p + "_half"] = run(p, init_latents=x0, strength=0.5, mask=half, **MS)
        assert all(torch.isfinite(out[p + t]).all() for t in ("", "_img", "_half"))
        assert not torch.equal(out[p], euler) and not torch.equal(out[p + "_img"], out[p]) and not torch.equal(out[p + "_img"], x0)
        assert torch.equal(out[p + "_half"][..., : w // 2], x0[..., : w // 2]) and not torch.equal(out[p + "_half"][..., w // 2:], x0[..., w // 2:])
        assert torch.equal(run(p, init_latents=x0, strength=0.5, mask=zeros, **MS), x0), p                 # a mask of zeros returns the init latents
        assert torch.equal(run(p, init_latents=x0, strength=1.0, **MS), out[p]), p                         # strength 1 without a mask: txt2img from the noise
    for t in ("", "_img", "_half"):
        assert torch.equal(out["graph" + t], out["fused" + t]), t                                          # graph == fused, bit for bit
    # without a mask txt2img and img2img issue the same launch (one capture); with a mask the pointers differ (a second one); Euler's dicts are untouched
    assert len(smp._ms_graphs) == 2 and len(smp._graphs) == 1 and len(smp._img_graphs) == 0
    for strength, steps, kind in ((0.8, 6, "karras"), (0.5, 10, "trailing"), (1.0, 4, "karras")):          # other steps, strength and sigmas: the same captures
        for m in (None, half):
            a, b = (run(p, steps=steps, init_latents=x0, strength=strength, mask=m, sigmas=kind, **MS) for p in ("graph", "fused"))
            assert torch.equal(a, b) and torch.isfinite(a).all(), (strength, steps, kind, m is None)
    assert len(smp._ms_graphs) == 2
    assert torch.equal(run("graph"), euler) and len(smp._graphs) == 1                                      # the Euler graph after: identical latents, no new capture
    # Euler on Karras sigmas: the Euler kernels with another table - the same capture again
    ek = run("graph", sigmas="karras")
    assert torch.equal(ek, run("fused", sigmas="karras")) and not torch.equal(ek, euler) and len(smp._graphs) == 1 and len(smp._ms_graphs) == 2


def _figures(got, ref):
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    return float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


@pytest.mark.parametrize("version,case,kind", [("tinyxl", "txt2img", "trailing"), ("tinyxl", "txt2img", "karras"), ("tinyxl", "masked", "karras"),
                                               ("tiny15", "img2img", "trailing")])
def test_fused_against_reference_loop(version, case, kind):
    """Measured on the MI355X (rel-L2 of the multistep path | of the Euler path on the same inputs): see DESIGN 4.24."""
    h = w = 16
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    steps, img, dimg = 6, {}, {}
    if case != "txt2img":
        steps = 10                                                                                         # strength 0.6: 6 steps run, as in tests/test_sampler_gpu.py
        mask = (torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(2)) * 3).floor() / 2 if case == "masked" else None   # 0, 0.5 and 1
        img = dict(init_latents=x0, strength=0.6, mask=mask)
        dimg = dict(init_latents=x0.cuda(), strength=0.6, mask=None if mask is None else mask.cuda())
    for name in ("euler", "dpmpp_2m"):                                                                     # Euler first: the yardstick of the same session and inputs
        ref = MR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, sampler=name, sigmas=kind, **img)
        got = smp.sample(_cuda(embeds)[0], h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), fused=True, sampler=name, sigmas=kind, **dimg).cpu()
        assert torch.isfinite(got).all()
        cos, rel = _figures(got, ref)
        print(f"{version} {case} {kind} {name}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, case, kind, cos, rel)
    if case == "masked":
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(got[keep], x0[keep])


# ---- render --sampler dpmpp_2m --sigmas karras -----------------------------------------------------------------------------------------
def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


def test_render_cli_multistep(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd import vae as V
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="ms job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    W, H = 96, 64
    base = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", str(W), str(H), "--steps", "6", "--seed", "11"]
    ms = ["--sampler", "dpmpp_2m", "--sigmas", "karras"]
    name = "img_00_seed11_scale0.85.jpg"
    outs = {}
    for tag, extra in (("ms", ms), ("ms_eager", ms + ["--eager"]), ("euler", []), ("ms_trailing", ms[:2])):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(base + extra + ["--out", outs[tag]])
    assert sorted(f for f in os.listdir(outs["ms"]) if f.endswith(".jpg")) == sorted([name, "grid_scale0.85.jpg"])
    assert Image.open(os.path.join(outs["ms"], name)).size == (W, H)
    raw = {k: open(os.path.join(d, name), "rb").read() for k, d in outs.items()}
    assert raw["ms"] == raw["ms_eager"] and raw["ms"] != raw["euler"] and raw["ms"] != raw["ms_trailing"] and raw["ms_trailing"] != raw["euler"]
    meta = json.load(open(os.path.join(outs["ms"], "prompts.json")))
    assert meta["sampler"] == "dpmpp_2m" and meta["sigmas"] == "karras" and "sampler" not in json.load(open(os.path.join(outs["euler"], "prompts.json")))
    # from a picture, everything kept: the file is decode(encode(picture)), byte for byte, as for Euler
    rng = np.random.default_rng(0)
    init, black = str(tmp_path / "init.png"), str(tmp_path / "black.png")
    Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(init)
    Image.fromarray(np.zeros((H, W), dtype=np.uint8)).save(black)
    out_keep = str(tmp_path / "out_keep")
    R.main(base + ms + ["--out", out_keep, "--init-image", init, "--strength", "0.5", "--mask", black])
    ld = R.load_for_inference(ckdir)
    f = 2 ** (len(ld.stack.decoder.ups) - 1)
    x0, _ = R.encode_init(ld, init, None, (W, H), (H // f, W // f))
    dec = V.postprocess(ld.stack.decoder.decode(x0 / ld.models.cfg["scaling_factor"]))[0].permute(1, 2, 0)
    rt_path = str(tmp_path / "roundtrip.jpg")
    Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(rt_path, format="JPEG", quality=95)
    assert open(os.path.join(out_keep, name), "rb").read() == open(rt_path, "rb").read()
    # without the mask the picture changes
    out_img = str(tmp_path / "out_img")
    R.render(ld, ["a photo of <concept>"], out_img, size=(W, H), steps=6, seed=11, init_image=init, sampler="dpmpp_2m", sigmas="karras")
    assert open(os.path.join(out_img, name), "rb").read() != open(rt_path, "rb").read()
