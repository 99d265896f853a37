"""Rendering from a checkpoint on the MI355X: the fused guidance + Euler + repack kernel (sdlt_sampler_step) against an fp64 restatement, the
graph-replayed sampler against the eager loop with the same kernel (bit for bit) and against the fp32 oracle loop, the adapter scale a capture
bakes, and the round trip train() -> checkpoint directory -> `python -m sd_lora_trainer_amd.render`."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_COS, TOL_REL = 0.999, 0.06          # the bars of tests/test_sampler_gpu.py (profiles/r04_parity_report_sampler.json)
U24 = 2.0 ** -24


def _table(steps, guidance, pred):
    from sd_lora_trainer_amd import sampler as SM
    s = SM.EulerDiscrete(prediction_type=pred).set_timesteps(steps)
    return s, SM.step_table(s, guidance)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("hw", [(16, 16), (24, 32), (128, 128)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_sampler_step_kernel_fp64(n, hw, pred):
    from sd_lora_trainer_amd import ops
    h, w = hw
    steps, g = 6, 7.5
    sched, tab = _table(steps, g, pred)
    assert float(tab[2 + steps - 1, 1]) == 0.0            # the last row steps to sigma = 0
    dev = "cuda"
    gen = torch.Generator().manual_seed(n * 1000 + h)
    noise = torch.randn(n, 4, h, w, generator=gen)
    table = torch.zeros(40, 4)
    table[: tab.shape[0]] = tab
    table_d = table.to(dev)
    x = torch.zeros(n, 4, h, w, device=dev)
    SENT = 3.25
    xin = torch.full((2 * n * h * w, 64), SENT, dtype=torch.bfloat16, device=dev)
    tf = torch.full((2 * n,), -1.0, device=dev)
    ctr = torch.tensor([5, 0], dtype=torch.int32, device=dev)      # the init entry resets a counter left anywhere
    t64 = tab.double()

    def check_xin(x_now, inv32, x_exact, inv64):
        got = xin[:, :4].float().cpu().view(n, 2, h, w, 4)
        assert torch.equal(got[:, 0], got[:, 1])                    # both rows of the pair
        got = got[:, 0].permute(0, 3, 1, 2)
        own = (x_now * inv32).to(torch.bfloat16).float()            # round-to-nearest-even of the kernel's own fp32 x times the table factor
        ex = (x_exact * inv64)
        one_ulp = torch.ldexp(torch.ones_like(ex), torch.frexp(ex)[1] - 8)                               # |v| = m 2^e, m in [0.5, 1): a bf16 ulp (8-bit significand) is 2^(e - 8)
        ok = (got == own) | ((got.double() - ex).abs() <= one_ulp)
        assert bool(ok.all()), int((~ok).sum())
        assert bool((xin[:, 4:] == SENT).all())                     # columns 4..63 are never touched

    # ---- init entry
    ops.sampler_step(None, x, xin, tf, table_d, ctr, noise=noise.to(dev))
    torch.cuda.synchronize()
    x_ex = noise.double() * t64[0, 1]
    # k = 1 fp32 operation on the path (noise * init_noise_sigma)
    assert bool(((x.cpu().double() - x_ex).abs() <= 1 * U24 * x_ex.abs()).all())
    check_xin(x.cpu(), tab[0, 2], x_ex, t64[0, 2])
    assert torch.equal(tf.cpu(), torch.full((2 * n,), float(tab[0, 3]))) and ctr.cpu().tolist() == [0, 0]
    # ---- every row of the table, each from the kernel's own previous x
    for i in range(steps):
        eps = torch.randn(2 * n * h * w, 4, generator=gen)
        x_prev = x.cpu().double()
        ops.sampler_step(eps.to(dev), x, xin, tf, table_d, ctr)
        torch.cuda.synchronize()
        e4 = eps.double().view(n, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        en, ep = e4[:, 0], e4[:, 1]
        s, sn, inv_n, t_n = (t64[2 + i, c] for c in range(4))
        e = en + g * (ep - en)
        E = en.abs() + abs(g) * (ep.abs() + en.abs())
        dt = sn - s
        if pred == "epsilon":
            x_ex = x_prev + e * dt
            # k = 6: ep - en, g *, en +, sigma_next - sigma, d * dt, x +
            k, S = 6, x_prev.abs() + E * abs(dt)
        else:
            q = s * s + 1
            x0 = e * (-s / q ** 0.5) + x_prev / q
            x_ex = x_prev + (x_prev - x0) / s * dt
            # k = 15: the 3 of e; s * s, + 1, sqrt, -s / (4) for the coefficient of e; e * c1, x / q, + (3) for x0; x - x0, / s (2); sigma_next - sigma, d * dt, x + (3)
            k, S = 15, x_prev.abs() + abs(dt / s) * (x_prev.abs() + E * abs(s / q ** 0.5) + x_prev.abs() / q)
        err = (x.cpu().double() - x_ex).abs()
        assert bool((err <= k * U24 * S).all()), (i, float((err / (U24 * S)).max()))
        check_xin(x.cpu(), tab[2 + i, 2], x_ex, inv_n)
        assert torch.equal(tf.cpu(), torch.full((2 * n,), float(t_n)))
        assert ctr.cpu().tolist() == [(i + 1) % steps, 0]           # wraps to 0 after the last step


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 24, 40)])
def test_sampler_step_init_noise_aliases_x(shape):
    """sdlt_sampler_step's init entry may be given x itself as `noise` (include/sdlt_kernels.h): every thread reads its pixel before it writes it.
    x, the model input, the timesteps and the counter equal the call with a buffer of its own, bit for bit."""
    from sd_lora_trainer_amd import ops
    n, h, w = shape
    dev = "cuda"
    _, tab = _table(6, 7.5, "epsilon")
    table = tab.to(dev)
    noise = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(h))
    out = []
    for aliased in (False, True):
        x = noise.to(dev) if aliased else torch.zeros(n, 4, h, w, device=dev)
        xin = torch.full((2 * n * h * w, 64), 3.25, dtype=torch.bfloat16, device=dev)
        tf = torch.full((2 * n,), -1.0, device=dev)
        ctr = torch.tensor([5, 0], dtype=torch.int32, device=dev)
        ops.sampler_step(None, x, xin, tf, table, ctr, noise=x if aliased else noise.to(dev))
        torch.cuda.synchronize()
        out.append((x.cpu(), xin[:, :4].cpu(), tf.cpu(), ctr.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0], noise) and out[0][3].tolist() == [0, 0]


def _setup(version, rank=None, dora=False, n=1, h=None):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import sampler, topology
    import sd_lora_trainer_amd.unet as M
    real = not version.startswith("tiny")
    cfg = U.CONFIGS[version]
    rank = rank or (16 if real else 8)
    if real:
        from tests.test_real_topology_gpu import _unet_state
        sd = _unet_state(version)
    else:
        sd = {k: v.to(torch.bfloat16).float() for k, v in U.init_unet_state(cfg, seed=0).items()}
    lora = {k: (a.to(torch.bfloat16).float(), b.to(torch.bfloat16).float()) for k, (a, b) in U.init_lora(cfg, rank, seed=1, b_std=0.05).items()}
    if dora:
        lora = {k: tuple(t.to(torch.bfloat16).float() for t in v) for k, v in U.init_dora_magnitudes(cfg, sd, lora, jitter=0.1, seed=2).items()}
    rt = M.Runtime("cuda:0", 2 * n)
    unet = M.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank, use_dora=dora)
    unet.arena.load(lora)
    return cfg, sd, lora, sampler.LatentSampler(rt, unet)


def _embeds(cfg, seed, h, w, n):
    g = torch.Generator().manual_seed(seed)
    D = cfg["cross_dim"]
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    embeds = [(mk(1, 77, D), mk(1, 77, D)) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None)) for _ in range(n)]
    noise = mk(n, 4, h, w)
    return embeds, noise


def _cuda(embeds):
    return [tuple(None if e is None else e.cuda() for e in em) for em in embeds]


def _sample(smp, embeds, noise, h, w, n, **kw):
    em = _cuda(embeds)
    return smp.sample(em if n > 1 else em[0], h, w, steps=6, guidance_scale=8.0, latents=noise.cuda(), n_images=n, **kw).cpu()


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_graph_equals_eager_with_kernel(version, n):
    cfg, sd, lora, smp = _setup(version, n=n)
    smp.set_lora_scale(0.75)
    embeds, noise = _embeds(cfg, 5, 16, 16, n)
    eager = _sample(smp, embeds, noise, 16, 16, n, fused=True)
    graph = _sample(smp, embeds, noise, 16, 16, n, graph=True)
    assert torch.isfinite(eager).all() and torch.equal(graph, eager)
    assert torch.equal(_sample(smp, embeds, noise, 16, 16, n, graph=True), graph)      # replayed again: the same latents
    em = _cuda(embeds)
    a, b = (smp.sample(em if n > 1 else em[0], 16, 16, steps=3, generator=torch.Generator(device="cuda").manual_seed(3), graph=True, n_images=n) for _ in range(2))
    assert torch.equal(a, b)                                                           # same seed twice
    assert len(smp._graphs) == 1                                                       # one capture served 6 and 3 steps, both guidance scales


def _against_oracle(version, *, h, w, n=1, dora=False, size=None, scale=0.75):
    from oracle import sampler_ref as SR
    cfg, sd, lora, smp = _setup(version, dora=dora, n=n)
    smp.set_lora_scale(scale)
    embeds, noise = _embeds(cfg, 5, h, w, n)
    em = _cuda(embeds)
    got = smp.sample(em if n > 1 else em[0], h, w, steps=6, guidance_scale=8.0, latents=noise.cuda(), size=size, graph=True, n_images=n).cpu()
    assert torch.isfinite(got).all()
    for j in range(n):                                                                 # each image against its own oracle run
        if dora:
            ref = _oracle_dora(cfg, sd, lora, scale, embeds[j], noise[j:j + 1], 6, size)
        else:
            ref = SR.sample_latents(cfg, sd, lora, scale, embeds[j], noise[j:j + 1], 6, guidance_scale=8.0, size=size)
        a, b = got[j].reshape(-1).double(), ref.reshape(-1).double()
        cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
        print(f"{version} h{h} w{w} n{n} dora={dora} image {j}: cos {cos:.6f} rel {rel:.4f}")
        assert cos >= TOL_COS and rel <= TOL_REL, (version, j, cos, rel)


def _oracle_dora(cfg, sd, lora, scale, embeds, noise, steps, size):
    """oracle.sampler_ref.sample_latents' loop with DoRA adapters: the render scale is the adapter scale of unet_forward (it enters the weight norm)."""
    from oracle import sampler_ref as SR
    from oracle import unet_ref as U
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    timesteps, sigmas = SR.euler_trailing(steps)
    x = noise.float() * float(sigmas.max())
    h, w = x.shape[-2:]
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    with torch.no_grad():
        for i, t in enumerate(timesteps):
            xin = torch.cat([x, x], 0) / float((sigmas[i] ** 2 + 1) ** 0.5)
            eps = U.unet_forward(cfg, sd, xin, torch.tensor([int(t)] * 2), torch.cat([uc, c], 0), add, lora=lora, lora_scale=scale)
            x = x + (eps[0:1] + 8.0 * (eps[1:2] - eps[0:1])) * float(sigmas[i + 1] - sigmas[i])
    return x


@pytest.mark.parametrize("version", ["tiny15", "tinyxl", "sd15", "sdxl"])
def test_graph_sampler_against_oracle(version):
    h = 16 if version.startswith("tiny") else 32
    _against_oracle(version, h=h, w=h)


def test_graph_sampler_non_square():
    _against_oracle("tinyxl", h=24, w=32, size=(192, 256))


def test_graph_sampler_two_images():
    _against_oracle("tinyxl", h=16, w=16, n=2)


def test_graph_sampler_dora():
    _against_oracle("tinyxl", h=16, w=16, dora=True)


def test_no_stale_scale():
    cfg, sd, lora, smp = _setup("tinyxl")
    embeds, noise = _embeds(cfg, 5, 16, 16, 1)
    smp.set_lora_scale(0.75)
    g75 = _sample(smp, embeds, noise, 16, 16, 1, graph=True)
    smp.set_lora_scale(0.4)
    g40 = _sample(smp, embeds, noise, 16, 16, 1, graph=True)
    e40 = _sample(smp, embeds, noise, 16, 16, 1, fused=True)
    assert torch.equal(g40, e40) and not torch.equal(g40, g75)
    smp.set_lora_scale(0.75)
    assert torch.equal(_sample(smp, embeds, noise, 16, 16, 1, graph=True), g75) and len(smp._graphs) == 2


def _run(gen):
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


@pytest.mark.parametrize("version,dora", [("tiny15", False), ("tinyxl", True)])
def test_round_trip_through_a_job(tmp_path, monkeypatch, version, dora):
    from PIL import Image
    from safetensors.torch import load_file
    from sd_lora_trainer_amd import checkpoint as ckpt
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    kw = dict(use_dora=True) if dora else dict(text_encoder_lora_optimizer="adamw", text_encoder_lora_rank=4, text_encoder_lora_lr=1e-3, txt_encoders_lr_warmup_steps=0)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="rt job", seed=3, resolution=256 if version == "tinyxl" else 128, train_batch_size=1,
                         max_train_steps=4, checkpointing_steps=1000, lora_rank=8, unet_lr=2e-3, ti_lr=1e-3, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": f"synthetic:{version}", "tokenizer_path": tok_dir}, **kw)
    config, ckdir = _run(T.train(cfg))
    # ---- what the loader holds is what the files hold
    ld = R.load_for_inference(ckdir)
    sd = load_file(next(os.path.join(ckdir, f) for f in os.listdir(ckdir) if f.endswith("_lora.safetensors")))
    exp = ld.stack.unet.arena.export()
    assert len(exp) > 10
    for name, (A, B, *m) in exp.items():
        k = ckpt.kohya_key(name)
        assert torch.equal(A.cpu().float().reshape(-1), sd[k + ".lora_down.weight"].float().reshape(-1)), name
        assert torch.equal(B.cpu().float().reshape(-1), sd[k + ".lora_up.weight"].float().reshape(-1)), name
        assert bool(m) == dora
        if dora:
            assert torch.equal(m[0].cpu().float().reshape(-1), sd[k + ".dora_scale"].float().reshape(-1)), name
    if not dora:
        assert ld.stack.te_arena is not None and any(k.startswith("lora_te1_") for k in sd)
        for name, (A, B, *m) in ld.stack.te_arena.export().items():
            k = ckpt.kohya_text_key(name)
            assert torch.equal(A.cpu().float(), sd[k + ".lora_down.weight"].float()) and torch.equal(B.cpu().float(), sd[k + ".lora_up.weight"].float()), name
    rows = ckpt.load_embeddings(next(os.path.join(ckdir, f) for f in os.listdir(ckdir) if f.endswith("_embeddings.safetensors")))
    assert len(rows) == len(ld.stack.encoders)
    for enc, r in zip(ld.stack.encoders, rows):
        assert torch.equal(enc.table[enc.V - 3:].cpu().float(), r.float())
    del ld
    # ---- the CLI: two prompts, two scales, a non-square size
    W, H = (128, 64)
    base = ["--checkpoint", ckdir, "--prompt", "a photo of <concept> on a beach", "--prompt", "a drawing of a house", "--lora-scale", "0.5", "--lora-scale", "0.9",
            "--size", str(W), str(H), "--steps", "4", "--seed", "11"]
    outs = {}
    for tag, extra in (("a", []), ("b", []), ("eager", ["--eager"])):
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(base + ["--out", outs[tag]] + extra)
    names = sorted(f for f in os.listdir(outs["a"]) if f.endswith(".jpg"))
    assert names == sorted([f"img_{i:02d}_seed{11 + i}_scale{s}.jpg" for i in range(2) for s in ("0.50", "0.90")] + ["grid_scale0.50.jpg", "grid_scale0.90.jpg"])
    for f in names:
        im = Image.open(os.path.join(outs["a"], f))
        assert im.size == ((2 * W, H) if f.startswith("grid") else (W, H)), (f, im.size)
        raw = open(os.path.join(outs["a"], f), "rb").read()
        assert raw == open(os.path.join(outs["b"], f), "rb").read(), f                  # two invocations: identical files
        assert raw == open(os.path.join(outs["eager"], f), "rb").read(), f              # eager with the fused kernel == graph
    a50, a90 = (np.asarray(Image.open(os.path.join(outs["a"], f"img_00_seed11_scale{s}.jpg"))).astype(np.int32) for s in ("0.50", "0.90"))
    assert np.abs(a50 - a90).max() > 0                                                  # the two scales give different images
    assert json.load(open(os.path.join(outs["a"], "prompts.json")))["lora_scales"] == [0.5, 0.9]
