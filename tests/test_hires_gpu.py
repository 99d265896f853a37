"""The hires pass on the MI355X: sdlt_resize_planes against its contract in NumPy float32 (tests/hires_ref.py), bit for bit; its bounds and argument
checks; the second pass = img2img at a new shape against the fp32 reference loop at the bars of tests/test_sampler_gpu.py; and
`python -m sd_lora_trainer_amd.render --hires-*` end to end on a tiny15 job."""
import json
import os

import numpy as np
import pytest
import torch

from tests import hires_ref as HR
from tests.test_hires_cpu import CASES
from tests.test_img2img_gpu import _cuda, _inputs, _run, _setup
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars test_img2img_gpu holds the same launch to

pytestmark = pytest.mark.gpu

SENT = -7.25
# CASES: (2, 2) -> (7, 5) has 35 output pixels per image (less than a wave); (33, 47) -> (83, 101) has 8383 (33 workgroups, a partial last one, a
# width that is no multiple of 64); (8, 12) -> (12, 20) and (16, 16) -> (10, 6) scale the axes differently; plus identity on one axis only, and on both
SHAPES = CASES + [((5, 7), (5, 11)), ((6, 9), (13, 9)), ((9, 13), (9, 13))]


def _resize(x, H, W, mode, tail=64):
    """ops.resize_planes into a sentinel-filled buffer with a tail -> (out on the CPU, the tail)."""
    from sd_lora_trainer_amd import ops
    n, c = x.shape[:2]
    flat = torch.full((n * c * H * W + tail,), SENT, device="cuda")
    out = ops.resize_planes(x.cuda().contiguous(), flat[: n * c * H * W].view(n, c, H, W), mode)
    torch.cuda.synchronize()
    return out.cpu(), flat[n * c * H * W:].cpu()


@pytest.mark.parametrize("planes", [4, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_resize_kernel_exact(shape, mode, planes):
    (h, w), (H, W) = shape
    x = torch.randn(3, planes, h, w, generator=torch.Generator().manual_seed(h * 100 + w + planes))
    got, tail = _resize(x, H, W, mode)
    ref = HR.resize(x, H, W, mode)
    assert torch.equal(got, ref), (shape, mode, int((got != ref).sum()), float((got - ref).abs().max()))
    assert bool((tail == SENT).all()) and not bool((got == SENT).any())
    if (h, w) == (H, W):
        assert torch.equal(got, x)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resize_kernel_extreme_values(mode):
    """+-3e38 and denormals: finite exactly where the contract's result is, and the same bits there."""
    (h, w), (H, W) = (8, 12), (12, 20)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 4, h, w, generator=g)
    x[0] = torch.where(torch.rand(4, h, w, generator=g) < 0.5, 3e38, -3e38)             # neighbours of opposite sign at the edge of the range
    x[1] = 3e38                                                                         # a constant at the edge of the range
    x[2] = x[2] * 1e-42                                                                 # denormals
    got, tail = _resize(x, H, W, mode)
    ref = HR.resize(x, H, W, mode)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(got[fin], ref[fin]) and bool((tail == SENT).all())
    assert bool(fin[1:].all())                                                          # the constant and the denormals stay finite in every mode
    if mode != 2:
        assert bool(fin.all())                                                          # convex weights: no overflow
    assert bool((got[2].abs() <= 1e-41).all()) and bool((got[2] != 0).any())


def test_resize_errors_launch_nothing():
    from sd_lora_trainer_amd import _lib, ops
    x = torch.randn(2, 4, 5, 7, device="cuda")
    out = torch.full((2, 4, 9, 11), SENT, device="cuda")
    for bad_out, mode in ((out, 3), (out, -1), (x, 1), (x.view(-1)[7:7 + 2 * 4 * 5 * 6].view(2, 4, 5, 6), 1)):
        with pytest.raises(_lib.KernelLibraryError, match="sdlt_resize_planes"):
            ops.resize_planes(x, bad_out, mode)
    with pytest.raises(AssertionError):
        ops.resize_planes(x, out[:1], 1)
    with pytest.raises(AssertionError):
        ops.resize_planes(x.double(), out, 1)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- the second pass is img2img at a new shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,hw,hw2", [("tiny15", (8, 8), (12, 12)), ("tinyxl", (8, 8), (12, 12)), ("tinyxl", (8, 12), (12, 20))])
def test_second_pass_against_reference_loop(version, hw, hw2):
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    (h, w), (H, W) = hw, hw2
    steps, strength = 10, 0.6
    cfg, sd, lora, smp1 = _setup(version)
    _, _, _, smp2 = _setup(version)                                                     # the same weights, buffers of its own for the large shape
    embeds, noise1, _ = _inputs(cfg, 5, h, w, 1)
    noise2 = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(6))
    em = _cuda(embeds)[0]
    first = smp1.sample(em, h, w, steps=6, guidance_scale=8.0, latents=noise1.cuda(), fused=True, size=(8 * h, 8 * w))
    x0 = SM.upscale_latents(ops, first, H, W, "bilinear")
    assert torch.equal(x0.cpu(), HR.resize(first.cpu(), H, W, 1))
    kw = dict(steps=steps, guidance_scale=8.0, latents=noise2.cuda(), init_latents=x0, strength=strength, size=(8 * H, 8 * W))
    got = smp2.sample(em, H, W, fused=True, **kw).cpu()
    ref = HR.second_pass(cfg, sd, lora, 0.75, embeds[0], first, noise2, steps, H=H, W=W, mode=1, strength=strength, size=(8 * H, 8 * W))
    assert torch.isfinite(got).all()
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"{version} {hw} -> {hw2}: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (version, cos, rel)
    assert torch.equal(smp2.sample(em, H, W, graph=True, **kw).cpu(), got)                # graph == fused, bit for bit
    assert len(smp2._img_graphs) == 1 and not (smp2._graphs or smp2._ms_graphs or smp2._sde_graphs or smp2._guided_graphs)


# ---- render --hires-* -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    root = tmp_path_factory.mktemp("hires_job")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        tok_dir, _ = _tokenizer_dir(root)
        cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="hires job", seed=3, resolution=128, train_batch_size=1,
                             max_train_steps=1, checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(root / "job"),
                             pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
        _, ckdir = _run(T.train(cfg))
    finally:
        os.chdir(cwd)
    return ckdir


NAME = "img_00_seed11_scale0.85.jpg"


def _main(ckdir, out, *extra):
    from sd_lora_trainer_amd import render as R
    R.main(["--checkpoint", ckdir, "--out", str(out), "--prompt", "a photo of <concept>", "--size", "64", "64", "--steps", "6", "--seed", "11", *extra])
    return open(os.path.join(str(out), NAME), "rb").read()


def test_render_hires_cli(ckpt_dir, tmp_path):
    from PIL import Image
    raw = _main(ckpt_dir, tmp_path / "graph", "--hires-scale", "1.5")
    assert Image.open(tmp_path / "graph" / NAME).size == (96, 96)
    meta = json.load(open(tmp_path / "graph" / "prompts.json"))
    assert meta["size"] == [64, 64] and meta["hires"] == dict(size=[96, 96], base_size=[64, 64], strength=0.6, steps=6, upscaler="latent", resample="bilinear")
    assert _main(ckpt_dir, tmp_path / "eager", "--hires-scale", "1.5", "--eager") == raw                       # graph == eager, byte for byte
    assert _main(ckpt_dir, tmp_path / "s06", "--hires-size", "96", "96", "--hires-strength", "0.6") == raw     # the default strength, the size given
    assert _main(ckpt_dir, tmp_path / "s03", "--hires-scale", "1.5", "--hires-strength", "0.3") != raw


def test_render_hires_pixel_upscaler(ckpt_dir, tmp_path):
    from PIL import Image
    latent = _main(ckpt_dir, tmp_path / "latent", "--hires-scale", "1.5")
    pixel = _main(ckpt_dir, tmp_path / "pixel", "--hires-scale", "1.5", "--hires-upscaler", "pixel")
    assert Image.open(tmp_path / "pixel" / NAME).size == (96, 96) and pixel != latent
    assert json.load(open(tmp_path / "pixel" / "prompts.json"))["hires"]["resample"] == "bicubic"


def test_render_hires_rebuilds_once(ckpt_dir, tmp_path, monkeypatch):
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    builds = []
    real = T.RenderStack.build_sampler
    monkeypatch.setattr(T.RenderStack, "build_sampler", lambda self, n: (builds.append(n), real(self, n))[1])
    R.main(["--checkpoint", ckpt_dir, "--out", str(tmp_path / "o"), "--prompt", "a photo of <concept>", "--prompt", "a house", "--lora-scale", "0.5",
            "--lora-scale", "0.9", "--size", "64", "64", "--steps", "4", "--seed", "11", "--hires-scale", "1.5"])
    assert builds == [1, 1]                                                              # the load, and one rebuild for 2 prompts x 2 scales
    jpgs = sorted(f for f in os.listdir(tmp_path / "o") if f.startswith("img_"))
    assert jpgs == sorted(f"img_{i:02d}_seed{11 + i}_scale{s}.jpg" for i in range(2) for s in ("0.50", "0.90"))


def test_render_hires_stochastic_repeats(ckpt_dir, tmp_path):
    a = _main(ckpt_dir, tmp_path / "a", "--hires-scale", "1.5", "--sampler", "euler_a")
    b = _main(ckpt_dir, tmp_path / "b", "--hires-scale", "1.5", "--sampler", "euler_a")
    c = _main(ckpt_dir, tmp_path / "c", "--hires-scale", "1.5")
    assert a == b and a != c


def test_render_without_hires_is_unchanged(ckpt_dir, tmp_path):
    """Without the hires flags the file is that of the loop render() has always run: the noise of seed + i, one sample() call, decode, JPEG."""
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import vae as V
    W = H = 64
    init = str(tmp_path / "init.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).save(init)
    plain = _main(ckpt_dir, tmp_path / "plain")
    img = _main(ckpt_dir, tmp_path / "img", "--init-image", init)
    assert sorted(json.load(open(tmp_path / "plain" / "prompts.json"))) == ["guidance_scale", "lora_scales", "prompts", "seed", "size", "steps"]
    ld = R.load_for_inference(ckpt_dir)
    stack, cfg = ld.stack, ld.models.cfg
    stack.sampler.set_lora_scale(0.85)
    emb = stack.conditioning("a photo of <concept>", 0.85, None, None)[0]
    f = 2 ** (len(stack.decoder.ups) - 1)                                                # the VAE's factor (4 for the tiny one)
    h, w = H // f, W // f
    x0, _ = R.encode_init(ld, init, None, (W, H), (h, w))
    for want, kw in ((plain, {}), (img, dict(init_latents=x0, strength=0.6))):
        noise = torch.randn(1, 4, h, w, generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
        lat = stack.sampler.sample(emb, h, w, steps=6, guidance_scale=8.0, size=(H, W), latents=noise, graph=True, fused=True, n_images=1, **kw)
        dec = V.postprocess(stack.decoder.decode(lat / cfg["scaling_factor"]))[0].permute(1, 2, 0)
        path = str(tmp_path / "manual.jpg")
        Image.fromarray((dec.float().cpu().numpy() * 255).round().astype("uint8")).save(path, format="JPEG", quality=95)
        assert open(path, "rb").read() == want
