"""Rendering from a checkpoint without a GPU: the step table + a torch restatement of sdlt_sampler_step reproduce LatentSampler.sample's present
loop, the loader and the CLI round-trip a job of train() on the emulated op table, and load_for_inference names what a directory lacks."""
import json
import os
import types

import numpy as np
import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd.config import TrainingConfig
from tests import emu_ops
from tests.test_driver_cpu import _run, _tokenizer_dir

U24 = 2.0 ** -24


def _sampler_step(eps, x, xin, timesteps, table, ctr, *, noise=None):
    """torch restatement of sdlt_sampler_step (include/sdlt_kernels.h), fp32, one rounding per operation, in the kernel's order."""
    n, _, h, w = x.shape
    steps = int(table[1, 0])
    if noise is not None:
        x.copy_(noise * table[0, 1])
        inv, tn, nxt = table[0, 2], table[0, 3], 0
    else:
        i = int(ctr[0])
        g, (s, sn, inv, tn) = table[0, 0], table[2 + i]
        e4 = eps.view(n, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        e = e4[:, 0] + g * (e4[:, 1] - e4[:, 0])
        if float(table[1, 1]) != 0.0:
            q = s * s + 1
            e = (x - (e * (-s / torch.sqrt(q)) + x / q)) / s
        x.copy_(x + e * (sn - s))
        nxt = (i + 1) % steps
    v = (x * inv).permute(0, 2, 3, 1).reshape(n, 1, h * w, 4).expand(n, 2, h * w, 4).reshape(2 * n * h * w, 4)
    xin[:, :4] = v.to(xin.dtype)
    timesteps[: 2 * n] = tn
    ctr[0], ctr[1] = nxt, 0
    return x


emu_render = types.ModuleType("emu_render")
emu_render.__dict__.update({k: v for k, v in vars(emu_ops).items() if not k.startswith("__")})
emu_render.sampler_step = _sampler_step


class _StubUNet:
    """forward() returns a fixed noise prediction per call (independent of its input), and keeps the model inputs it was given."""

    def __init__(self, n, h, w, seed):
        self.cfg, self.arena = dict(cross_dim=8, addition=False), None
        g = torch.Generator().manual_seed(seed)
        self.eps = [torch.randn(2 * n * h * w, 4, generator=g) for _ in range(8)]
        self.calls, self.inputs, self.ts = 0, [], []

    def forward(self, x, t, ctx, pooled, tid, *, B, H, W):
        self.inputs.append(x[:, :4].clone())
        self.ts.append(t.clone())
        self.calls += 1
        return self.eps[self.calls - 1]


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_table_and_restated_kernel_reproduce_sample(pred):
    h, w, steps, g = 8, 12, 6, 8.0
    emb = (torch.randn(1, 77, 8), torch.randn(1, 77, 8), None, None)
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(1))
    outs = []
    for fused in (False, True):
        rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=emu_render)
        stub = _StubUNet(1, h, w, 7)
        smp = SM.LatentSampler(rt, stub, prediction_type=pred)
        outs.append((smp.sample(emb, h, w, steps=steps, guidance_scale=g, latents=noise.clone(), fused=fused), stub))
    (xa, sa), (xb, sb) = outs
    assert sa.calls == sb.calls == steps
    # fp64 trajectory with the same predictions: per step, either implementation is within k 2^-24 S of the exact update of its own input (k fp32 operations on
    # the path, S the sum of the absolute values of the terms - tests/test_render_gpu.py counts them: 6 / 15); an error carried in x is passed on with a factor
    # 1 (epsilon) or 1 + (sigma_next - sigma) sigma / (sigma^2 + 1) in (0, 1) (v prediction), so after n steps the two differ by at most the sum of both bounds
    sig = SM.EulerDiscrete(prediction_type=pred).set_timesteps(steps).sigmas.astype(np.float64)
    x = noise.double() * sig.max()
    bound = 2 * 1 * U24 * x.abs()
    for i in range(steps):
        # the model inputs: x / sqrt(sigma^2 + 1) (today's loop: the divisor rounded to fp32, one division) against x * (1 / sqrt(..) rounded to fp32): k = 2 each
        a, b = (s_.inputs[i][: h * w].view(h, w, 4).permute(2, 0, 1).double() for s_ in (sa, sb))
        inv = 1.0 / np.sqrt(sig[i] ** 2 + 1)
        assert bool(((a - b).abs() <= (bound + 2 * 2 * U24 * x.abs()) * inv * (1 + 4 * U24)).all()), i
        assert torch.equal(sa.ts[i], sb.ts[i])
        e4 = sa.eps[i].double().view(1, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        en, ep = e4[:, 0], e4[:, 1]
        e, E = en + g * (ep - en), en.abs() + g * (ep.abs() + en.abs())
        s, dt = sig[i], sig[i + 1] - sig[i]
        if pred == "epsilon":
            k, S = 6, x.abs() + E * abs(dt)
            x = x + e * dt
        else:
            q = s * s + 1
            k, S = 15, x.abs() + abs(dt / s) * (x.abs() + E * s / q ** 0.5 + x.abs() / q)
            x = x + (x - (e * (-s / q ** 0.5) + x / q)) / s * dt
        bound = bound + 2 * k * U24 * (S + bound)
    assert bool(((xa.double() - xb.double()).abs() <= bound).all())
    assert bool(((xa.double() - x).abs() <= bound).all()) and bool(((xb.double() - x).abs() <= bound).all())
    assert not torch.equal(xa, noise)


def test_default_sample_needs_no_new_op():
    """Op tables without sampler_step (tests/emu_ops.py) keep the torch loop; the fused path refuses instead of falling back."""
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=emu_ops)
    smp = SM.LatentSampler(rt, _StubUNet(1, 8, 8, 3))
    emb = (torch.randn(1, 77, 8), torch.randn(1, 77, 8), None, None)
    assert smp.sample(emb, 8, 8, steps=3).shape == (1, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="sampler_step"):
        smp.sample(emb, 8, 8, steps=3, fused=True)


def test_step_table_layout():
    s = SM.EulerDiscrete().set_timesteps(25)
    tab = SM.step_table(s, 8.0)
    assert tab.shape == (27, 4) and tab.dtype == torch.float32
    assert tab[0].tolist() == [8.0, float(np.float32(s.init_noise_sigma)), float(np.float32(1 / np.sqrt(np.float64(s.sigmas[0]) ** 2 + 1))), 999.0]
    assert tab[1].tolist() == [25.0, 0.0, 0.0, 0.0] and float(tab[26, 1]) == 0.0 and float(tab[26, 2]) == 1.0
    assert tab[2:, 3].tolist() == s.timesteps[1:].tolist() + [999.0]
    assert SM.step_table(SM.EulerDiscrete(prediction_type="v_prediction").set_timesteps(4), 1.0)[1].tolist() == [4.0, 1.0, 0.0, 0.0]


def _mk_rt(B=1):
    return unet_mod.Runtime("cpu", B, act_dtype=torch.float32, ops=emu_render)


@pytest.fixture
def job(tmp_path, monkeypatch):
    from sd_lora_trainer_amd import train as T
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="cpu job", seed=3, resolution=128, train_batch_size=1, max_train_steps=2,
                         checkpointing_steps=1000, lora_rank=4, n_sample_imgs=0, output_dir=str(tmp_path / "job"), text_encoder_lora_optimizer="adamw",
                         text_encoder_lora_rank=4, pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    _, (config, ckdir) = _run(T.train(cfg, runtime=_mk_rt()))
    return config, ckdir


def test_loader_and_cli_round_trip(job, tmp_path):
    from PIL import Image
    from safetensors.torch import load_file
    from sd_lora_trainer_amd import checkpoint as ckpt
    from sd_lora_trainer_amd import render as R
    config, ckdir = job
    ld = R.load_for_inference(ckdir, runtime=_mk_rt())
    sd = load_file(next(os.path.join(ckdir, f) for f in os.listdir(ckdir) if f.endswith("_lora.safetensors")))
    for arena, key in ((ld.stack.unet.arena, ckpt.kohya_key), (ld.stack.te_arena, ckpt.kohya_text_key)):
        exp = arena.export()
        assert exp
        for name, (A, B, *_) in exp.items():
            assert torch.equal(A.float().reshape(-1), sd[key(name) + ".lora_down.weight"].float().reshape(-1)), name
            assert torch.equal(B.float().reshape(-1), sd[key(name) + ".lora_up.weight"].float().reshape(-1)), name
    rows = ckpt.load_embeddings(next(os.path.join(ckdir, f) for f in os.listdir(ckdir) if f.endswith("_embeddings.safetensors")))
    for enc, r in zip(ld.stack.encoders, rows):
        assert torch.equal(enc.table[enc.V - config.n_tokens:].float(), r.float())
    outs = []
    for tag in ("a", "b"):
        outs.append(str(tmp_path / f"out_{tag}"))
        R.main(["--checkpoint", ckdir, "--out", outs[-1], "--prompt", "a photo of <concept>", "--prompt", "a house", "--lora-scale", "0.5", "--lora-scale", "0.9",
                "--size", "64", "32", "--steps", "2", "--seed", "5"], runtime=_mk_rt())
    names = sorted(f for f in os.listdir(outs[0]) if f.endswith(".jpg"))
    assert names == sorted([f"img_{i:02d}_seed{5 + i}_scale{s}.jpg" for i in range(2) for s in ("0.50", "0.90")] + ["grid_scale0.50.jpg", "grid_scale0.90.jpg"])
    for f in names:
        assert Image.open(os.path.join(outs[0], f)).size == ((128, 32) if f.startswith("grid") else (64, 32))
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
    assert json.load(open(os.path.join(outs[0], "prompts.json")))["prompts"] == ["a photo of <concept>", "a house"]
    # validation prompts of the job's concept mode when none are given
    res = R.render(ld, None, str(tmp_path / "out_val"), size=(32, 32), steps=1, n_validation=2)
    assert [len(v) for v in res.values()] == [2]


def test_loader_errors_name_what_is_missing(job, tmp_path):
    import shutil
    from safetensors.torch import save_file
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import topology
    from sd_lora_trainer_amd.train import _random_state
    config, ckdir = job
    d = str(tmp_path / "no_args")
    shutil.copytree(ckdir, d)
    os.remove(os.path.join(d, "training_args.json"))
    with pytest.raises(FileNotFoundError, match="training_args.json"):
        R.load_for_inference(d, runtime=_mk_rt())
    d = str(tmp_path / "no_adapter")
    shutil.copytree(ckdir, d)
    os.remove(next(os.path.join(d, f) for f in os.listdir(d) if f.endswith("_lora.safetensors")))
    with pytest.raises(FileNotFoundError, match=r"_lora\.safetensors"):
        R.load_for_inference(d, runtime=_mk_rt())
    d = str(tmp_path / "no_key")
    shutil.copytree(ckdir, d)
    args = json.load(open(os.path.join(d, "training_args.json")))
    del args["n_tokens"]
    json.dump(args, open(os.path.join(d, "training_args.json"), "w"))
    with pytest.raises(KeyError, match="n_tokens"):
        R.load_for_inference(d, runtime=_mk_rt())
    # text-encoder adapters in the file, a real UNet file as the base model, no text-encoder weights
    unet_file = str(tmp_path / "unet.safetensors")
    save_file({k: v.contiguous() for k, v in _random_state(topology.param_shapes(topology.CONFIGS["tiny15"]), "cpu", seed=0).items()}, unet_file)
    with pytest.raises(ValueError, match=r"text_encoder_path.*text-encoder adapters"):
        R.load_for_inference(ckdir, pretrained_model={"path": unet_file, "tokenizer_path": config.pretrained_model["tokenizer_path"]}, runtime=_mk_rt())
