"""Sampling from an init image on the MI355X: the sdlt_sampler_step_img kernel against its contract evaluated in torch (bit for bit), the invariants of
LatentSampler.sample(init_latents=, strength=, mask=) on the torch loop, the fused loop and the replayed graph, the fused path against the fp32
reference loop (tests/img2img_ref.py), and `python -m sd_lora_trainer_amd.render --init-image` end to end."""
import os

import numpy as np
import pytest
import torch

from tests import img2img_ref as IR
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop

pytestmark = pytest.mark.gpu

SENT = 3.25


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", ["none", "random", "ones", "zeros"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 24, 40)])       # 35 pixels: a partial block; 2880: 12 blocks, the last-block ticket, j = idx / hw across images
def test_sampler_step_img_kernel_exact(shape, pred, mask_kind):
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    n, h, w = shape
    steps, strength, g, ld = 5, 0.6, 7.5, 64
    k, start = SM.img2img_steps(steps, strength)
    assert (k, start) == (3, 2)
    tab = SM.step_table_img(SM.EulerDiscrete(prediction_type=pred).set_timesteps(steps, start), g)
    assert float(tab[2 + k - 1, 1]) == 0.0 and float(tab[0, 1]) == float(tab[2, 0])
    table = torch.zeros(40, 4)
    table[: tab.shape[0]] = tab
    gen = torch.Generator().manual_seed(1000 * n + h)
    x0, noise = 0.8 * torch.randn(n, 4, h, w, generator=gen), torch.randn(n, 4, h, w, generator=gen)
    mask = dict(none=None, random=torch.rand(n, 1, h, w, generator=gen), ones=torch.ones(n, 1, h, w), zeros=torch.zeros(n, 1, h, w))[mask_kind]
    if mask_kind == "random":
        mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    dev = "cuda"
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    # device state, poisoned: the init entry overwrites x, resets a counter left anywhere and touches columns 0..3 only
    x = torch.full((n, 4, h, w), float("nan"), device=dev)
    xin = torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16, device=dev)
    tf = torch.full((2 * n,), -1.0, device=dev)
    ctr = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    table_d, x0_d, noise_d, mask_d = d(table), d(x0), d(noise), d(mask)
    # the contract, on the CPU
    rx, rxin, rtf, rctr = torch.zeros(n, 4, h, w), torch.full((2 * n * h * w, ld), SENT, dtype=torch.bfloat16), torch.zeros(2 * n), torch.tensor([2, 0], dtype=torch.int32)

    def compare(what):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), rx), (what, int((x.cpu() != rx).sum()))
        assert torch.equal(xin.cpu().view(torch.int16), rxin.view(torch.int16)), what            # both rows of every pair, columns 4.. untouched
        assert torch.equal(tf.cpu(), rtf) and ctr.cpu().tolist() == rctr.tolist(), (what, tf.cpu(), ctr.cpu())

    ops.sampler_step_img(None, x, xin, tf, table_d, ctr, x0=x0_d, noise=noise_d, mask=mask_d, init=True)
    IR.sampler_step_img(None, rx, rxin, rtf, table, rctr, x0=x0, noise=noise, mask=mask, init=True)
    assert rctr.tolist() == [0, 0] and float(rtf[0]) == float(tab[0, 3])
    compare("init")
    for i in range(k):
        eps = torch.randn(2 * n * h * w, 4, generator=gen)
        ops.sampler_step_img(eps.to(dev), x, xin, tf, table_d, ctr, x0=x0_d, noise=noise_d, mask=mask_d)
        IR.sampler_step_img(eps, rx, rxin, rtf, table, rctr, x0=x0, noise=noise, mask=mask)
        assert rctr.tolist() == [(i + 1) % k, 0] and float(rtf[0]) == float(tab[2 + i, 3])
        compare(i)
    assert ctr.cpu().tolist() == [0, 0] and torch.equal(tf.cpu(), torch.full((2 * n,), float(tab[0, 3])))     # back at the start after k steps
    if mask_kind == "zeros":
        assert torch.equal(x.cpu(), x0)                                                                       # everything kept: the init latents exactly
    if mask_kind == "random":
        keep = (mask == 0).expand_as(x0)
        assert int(keep.sum()) > 0 and torch.equal(x.cpu()[keep], x0[keep])
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


@pytest.mark.parametrize("hw", [(8, 8), (8, 12)])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_invariants(version, hw):
    h, w = hw
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    PATHS = dict(torch={}, fused=dict(fused=True), graph=dict(graph=True))

    def run(path, steps=6, **kw):
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
        return smp.sample(em, h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), **PATHS[path], **kw).cpu()

    ones, zeros = torch.ones(1, 1, h, w), torch.zeros(1, 1, h, w)
    half = ones.clone()
    half[..., : w // 2] = 0
    plain = {p: run(p) for p in PATHS}
    assert len(smp._graphs) == 1 and len(smp._img_graphs) == 0
    img = {}
    for p in PATHS:
        assert torch.isfinite(plain[p]).all()
        assert torch.equal(run(p, init_latents=x0, strength=1.0), plain[p]), p                              # (a) strength 1 without a mask: txt2img from the noise
        img[p] = run(p, init_latents=x0, strength=0.5)
        assert torch.isfinite(img[p]).all() and not torch.equal(img[p], plain[p]) and not torch.equal(img[p], x0)
        assert torch.equal(run(p, init_latents=x0, strength=0.5, mask=ones), img[p]), p                    # (b) a mask of ones is no mask
        assert torch.equal(run(p, init_latents=x0, strength=0.5, mask=zeros), x0), p                       # (c) a mask of zeros returns the init latents
        out = run(p, init_latents=x0, strength=0.5, mask=half)
        assert torch.equal(out[..., : w // 2], x0[..., : w // 2]), p                                       # (d) the kept half is the init latents
        assert torch.isfinite(out).all() and not torch.equal(out[..., w // 2:], x0[..., w // 2:])
        img[p + "_half"] = out
    assert torch.equal(img["graph"], img["fused"]) and torch.equal(img["graph_half"], img["fused_half"])   # (e) graph == fused, bit for bit
    assert len(smp._img_graphs) == 2 and len(smp._graphs) == 1                                             # without / with the mask pointer; txt2img's capture is alone in its dict
    for strength, steps in ((0.8, 6), (0.5, 10), (1.0, 4)):                                                # (f) another strength / step count: the same captures
        for m in (None, half):
            if m is None and strength == 1.0:
                continue
            a, b = (run(p, steps=steps, init_latents=x0, strength=strength, mask=m) for p in ("graph", "fused"))
            assert torch.equal(a, b), (strength, steps, m is None)
    assert len(smp._img_graphs) == 2
    assert torch.equal(run("graph"), plain["graph"]) and len(smp._graphs) == 1                             # (g) txt2img's graph before and after: no collision


def test_two_images_share_init_and_mask():
    h, w, n = 8, 12, 2
    cfg, sd, lora, smp = _setup("tinyxl", n=n)
    embeds, noise, x0 = _inputs(cfg, 7, h, w, n)
    em = _cuda(embeds)
    mask = torch.ones(1, 1, h, w)
    mask[:, :, : h // 2] = 0
    outs = [smp.sample(em, h, w, steps=6, latents=noise.cuda(), n_images=n, init_latents=x0.cuda(), strength=0.5, mask=mask.cuda(), **kw).cpu()
            for kw in (dict(fused=True), dict(graph=True))]
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    for j in range(n):
        assert torch.equal(outs[0][j, :, : h // 2], x0[0, :, : h // 2])
    assert not torch.equal(outs[0][0, :, h // 2:], outs[0][1, :, h // 2:])                                 # each image has its own noise and prompt


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_fused_against_reference_loop(version, masked):
    h = w = 16
    steps, strength = 10, 0.6                                                                              # 6 steps run, as in tests/test_sampler_gpu.py
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    mask = None
    if masked:
        mask = (torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(2)) * 3).floor() / 2        # 0, 0.5 and 1
    ref = IR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, init_latents=x0, strength=strength, mask=mask)
    got = smp.sample(_cuda(embeds)[0], h, w, steps=steps, guidance_scale=8.0, latents=noise.cuda(), fused=True, init_latents=x0.cuda(), strength=strength,
                     mask=None if mask is None else mask.cuda()).cpu()
    assert torch.isfinite(got).all()
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"{version} masked={masked}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, masked, cos, rel)
    if masked:
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(got[keep], x0[keep])


# ---- render --init-image ---------------------------------------------------------------------------------------------------------------
def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


def test_render_from_init_image(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd import vae as V
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="img job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    W, H = 96, 64
    rng = np.random.default_rng(0)
    init, black = str(tmp_path / "init.png"), str(tmp_path / "black.png")
    Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(init)
    Image.fromarray(np.zeros((H, W), dtype=np.uint8)).save(black)
    name = "img_00_seed11_scale0.85.jpg"
    # the command line, everything kept: the picture is decode(encode(image)), bit for bit
    out_keep = str(tmp_path / "out_keep")
    R.main(["--checkpoint", ckdir, "--out", out_keep, "--prompt", "a photo of <concept>", "--size", str(W), str(H), "--steps", "6", "--seed", "11",
            "--init-image", init, "--strength", "0.5", "--mask", black])
    keep = Image.open(os.path.join(out_keep, name))
    assert keep.size == (W, H)
    ld = R.load_for_inference(ckdir)
    f = 2 ** (len(ld.stack.decoder.ups) - 1)
    x0, _ = R.encode_init(ld, init, None, (W, H), (H // f, W // f))
    dec = V.postprocess(ld.stack.decoder.decode(x0 / ld.models.cfg["scaling_factor"]))[0].permute(1, 2, 0)
    rt_path = str(tmp_path / "roundtrip.jpg")
    Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(rt_path, format="JPEG", quality=95)
    assert open(os.path.join(out_keep, name), "rb").read() == open(rt_path, "rb").read()
    # without the mask the picture changes; the graph and the eager loop agree; the default strength is 0.6
    outs = {}
    for tag, kw in (("graph", {}), ("eager", dict(graph=False)), ("s06", dict(strength=0.6)), ("s03", dict(strength=0.3))):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.render(ld, ["a photo of <concept>"], outs[tag], size=(W, H), steps=6, seed=11, init_image=init, **kw)
    raw = {k: open(os.path.join(d, name), "rb").read() for k, d in outs.items()}
    assert raw["graph"] == raw["eager"] == raw["s06"] and raw["graph"] != raw["s03"]
    assert Image.open(os.path.join(outs["graph"], name)).size == (W, H)
    assert not np.array_equal(np.asarray(Image.open(os.path.join(outs["graph"], name))), np.asarray(keep))
