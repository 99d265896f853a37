"""Adapter merge (LoraArena.merged / checkpoint.save_merged / python -m sd_lora_trainer_amd.merge) on CPU, with sdlt_lora_merge replaced by
the torch emulation below (injected through the runtime's op table like tests/emu_ops.py); the kernel itself is checked on the GPU by
tests/test_merge_gpu.py against the same fp64 reference and bound."""
import json
import os
import types

import pytest
import torch
from safetensors.torch import load_file

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import topology
from tests import emu_ops

MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
EMIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}


class EmuMergePlan:
    """torch emulation of ops.MergePlan: fp32 merged values, DoRA row factor from them, one rounding to the output dtype."""
    runs = 0

    def __init__(self, layers, out_dtype, device):
        self.layers, self.out_dtype = layers, out_dtype

    def run(self):
        EmuMergePlan.runs += 1
        for L in self.layers:
            v = L["W"].float() + float(L["s"]) * (L["B"].float() @ L["A"].float())
            if L.get("mag") is not None:
                v = (L["mag"].float() / v.norm(dim=1)).view(-1, 1) * v
            L["out"].copy_(v.to(self.out_dtype))


def emu_ops_with_merge():
    ns = types.SimpleNamespace(**{k: getattr(emu_ops, k) for k in dir(emu_ops) if not k.startswith("__")})
    ns.MergePlan = EmuMergePlan
    return ns


def ulp(x, dtype):
    """ulp of the fp64 values x in `dtype` (subnormal range included)."""
    _, e = torch.frexp(x.double())
    e = torch.clamp(e - 1, min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - MANT[dtype])


def ref64(W, A, B, s, mag=None):
    """fp64 merge -> (ref, row factor c (ones for LoRA), sum_r |B||A|)."""
    W, A, B = W.double(), A.double(), B.double()
    v = W + s * (B @ A)
    c = torch.ones(W.shape[0], 1, dtype=torch.float64) if mag is None else (mag.double().view(-1) / v.norm(dim=1)).view(-1, 1)
    return c * v, c, B.abs() @ A.abs()


def bound(W, A, B, s, mag, out_dtype):
    """|out - ref64| <= 1/2 ulp(ref64) + (r+2) 2^-24 |c| (|W| + |s| sum_r |B||A|) + (K+2) 2^-24 |ref64| [DoRA]: the fp32 summation bound of the issue."""
    r, K = A.shape
    ref, c, bafs = ref64(W, A, B, s, mag)
    u = 2.0 ** -24
    b = 0.5 * ulp(ref, out_dtype) + (r + 2) * u * c.abs() * (W.double().abs() + abs(s) * bafs)
    if mag is not None:
        b = b + (K + 2) * u * ref.abs()
    return ref, b


def case(N, K, r, seed, w_dtype=torch.float32, dora=False):
    """Gaussian W (std 0.02), A as init_lora (N(0, 1/r^2)), B std 0.05 (init_lora(b_std=0.05)); DoRA: jittered magnitudes."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(w_dtype)
    A = torch.randn(r, K, generator=g) / r
    B = torch.randn(N, r, generator=g) * 0.05
    mag = None
    if dora:
        v = W.double() + B.double() @ A.double()
        mag = (v.norm(dim=1) * (1.0 + 0.1 * torch.randn(N, generator=g, dtype=torch.float64))).float()
    return W, A, B, mag


def violations(out, W, A, B, s, mag, out_dtype):
    ref, b = bound(W, A, B, s, mag, out_dtype)
    err = (out.double().cpu() - ref).abs()
    return int((err > b).sum()), float((err / b).max())


# shapes of the kernel cases (tests/test_merge_gpu.py): tiny / real linears, a ragged one, 3x3 convs (K = 9 Cin)
SHAPES = [(64, 64), (320, 320), (640, 2048), (100, 72), (64, 576), (320, 2880)]


@pytest.mark.parametrize("r,dora", [(4, False), (16, False), (64, False), (128, False), (256, False), (16, True), (64, True)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_plain_fp32_merge_meets_the_bound(r, dora, out_dtype):
    """The inputs are fit for the bound: a plain fp32 torch merge (fp32 products and sums, one rounding) stays within it everywhere, and for an
    fp32 output a merge that rounds A and B to bf16 does not."""
    for i, (N, K) in enumerate(SHAPES):
        W, A, B, mag = case(N, K, r, seed=100 * r + i, dora=dora)
        s = 0.75
        v = W.float() + s * (B @ A)
        if dora:
            v = (mag / v.norm(dim=1)).view(-1, 1) * v
        n, worst = violations(v.to(out_dtype), W, A, B, s, mag, out_dtype)
        print(f"fp32 merge N={N} K={K} r={r} dora={dora} {out_dtype}: worst err/bound {worst:.3g}")
        assert n == 0, f"a plain fp32 merge misses the bound at {n} elements (worst err/bound {worst})"
        if out_dtype == torch.float32 and not dora:
            vb = W.float() + s * (B.bfloat16().float() @ A.bfloat16().float())
            assert violations(vb, W, A, B, s, mag, out_dtype)[0] > 0, "a bf16-rounded adapter passes the bound: it does not discriminate"


def _arena(version, rank, dora, ops, sd):
    rt = unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=ops)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank, use_dora=dora)
    g = torch.Generator().manual_seed(rank)
    for e in unet.arena.entries:
        e["A"].copy_(torch.randn(e["A"].shape, generator=g) / rank)
        e["B"].copy_(torch.randn(e["B"].shape, generator=g) * 0.05)
        if dora:
            e["M"].mul_(1.0 + 0.1 * torch.randn(e["M"].shape, generator=g))
    unet.arena.refresh_shadows()
    return unet


def _state(arena):
    st = [arena.params, arena.grads, arena.m, arena.v] + ([arena.dscale] if arena.dora else [])
    for e in arena.entries:
        st += [e[k] for k in ("A_s", "B_s", "Bt_s", "At_s", "Ab_s") if k in e]
    return [t.clone() for t in st], arena.scale


@pytest.mark.parametrize("version,rank,dora", [("tiny15", 16, False), ("tinyxl", 128, False), ("tinyxl", 16, True)])
def test_arena_merged_values_and_no_side_effects(version, rank, dora):
    from oracle import unet_ref as U
    sd = U.init_unet_state(U.CONFIGS[version], seed=0)
    unet = _arena(version, rank, dora, emu_ops_with_merge(), sd)
    arena = unet.arena
    before, scale = _state(arena)
    EmuMergePlan.runs = 0
    for s_render in (1.0, 0.75):
        m = arena.merged(sd, scale=s_render, dtype=torch.float32)
        assert set(m) == {e["name"] + ".weight" for e in arena.entries}
        lo = arena.export()
        for e in arena.entries:
            key = e["name"] + ".weight"
            A, B, *mg = lo[e["name"]]
            w = sd[key]
            assert tuple(m[key].shape) == tuple(w.shape) and m[key].dtype == torch.float32
            ref = w.double() + s_render * (B.flatten(1).double() @ A.flatten(1).double()).reshape(w.shape)
            if mg:
                ref = (mg[0].double().reshape(-1) / ref.flatten(1).norm(dim=1)).view(-1, *([1] * (w.dim() - 1))) * ref
            err = float((m[key].double() - ref).abs().max())
            assert err <= 1e-5 * float(ref.abs().max()), (key, err)
    assert EmuMergePlan.runs == 2, "one merge plan run per merged() call"
    after, scale2 = _state(arena)
    assert scale2 == scale
    for a, b in zip(before, after):
        assert torch.equal(a, b), "merged() changed training state"


def test_save_merged_writes_the_base_key_set(tmp_path):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import checkpoint as ckpt
    sd = U.init_unet_state(U.CONFIGS["tiny15"], seed=0)
    unet = _arena("tiny15", 8, False, emu_ops_with_merge(), sd)
    adapted = {e["name"] + ".weight" for e in unet.arena.entries}
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        d = tmp_path / str(dtype).split(".")[-1]
        files = ckpt.save_merged(str(d), sd, unet.arena, "tiny15", dtype=dtype)
        out = load_file(files["unet"])
        assert set(out) == set(sd)
        for k, v in sd.items():
            assert tuple(out[k].shape) == tuple(v.shape) and out[k].dtype == dtype, k
            if k not in adapted:
                assert torch.equal(out[k], v.to(dtype)), f"{k}: not the base value cast to {dtype}"
        assert sum(not torch.equal(out[k], sd[k].to(dtype)) for k in adapted) == len(adapted)
        cfgj = json.load(open(d / "config.json"))
        assert cfgj == json.loads(json.dumps(topology.diffusers_unet_config(topology.CONFIGS["tiny15"]), sort_keys=True))
        # ... and loads as a plain UNet without adapters
        rt = unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_ops)
        plain = unet_mod.UNet(rt, topology.CONFIGS["tiny15"], {k: v.float() for k, v in out.items()})
        assert plain.arena is None


def _run(gen):
    progress = []
    try:
        while True:
            progress.append(next(gen))
    except StopIteration as e:
        return progress, e.value


@pytest.mark.parametrize("version,dora", [("tiny15", False), ("tinyxl", True)])
def test_cli_round_trip_through_a_training_job(tmp_path, monkeypatch, version, dora):
    """train() (text-encoder adapters on) -> the CLI on its checkpoint -> the output as pretrained_model of a fresh job that trains a finite step."""
    import numpy as np
    from safetensors.torch import save_file
    from sd_lora_trainer_amd import merge as MG
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    monkeypatch.chdir(tmp_path)
    ops = emu_ops_with_merge()
    mk_rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=ops)  # noqa: E731
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model={"path": f"synthetic:{version}"}, seed=1,
                         resolution=128, train_batch_size=1, max_train_steps=2, text_encoder_lora_optimizer="adamw", use_dora=dora,
                         lora_rank=8, text_encoder_lora_rank=4, lora_alpha_multiplier=0.5, checkpointing_steps=1000, n_sample_imgs=0)
    _, (config, out_dir) = _run(T.train(cfg, runtime=mk_rt()))
    models = T.Models(config, mk_rt())
    paths = {"unet": str(tmp_path / "base_unet.safetensors")}
    save_file({k: v.contiguous() for k, v in models.unet_state().items()}, paths["unet"])
    for i in range(len(models.kinds)):
        paths[f"te{i}"] = str(tmp_path / f"base_te{i}.safetensors")
        save_file({k: v.contiguous() for k, v in models.clip_state(i).items()}, paths[f"te{i}"])
    xl = len(models.kinds) == 2
    files = MG.merge(paths["unet"], out_dir, str(tmp_path / "merged"), lora_scale=1.0, dtype="fp32", text_encoder=paths["te0"],
                     text_encoder_2=paths.get("te1"), runtime=mk_rt())
    assert os.path.exists(files["unet"]) and os.path.exists(files["text_encoder"]) and (os.path.exists(files["text_encoder_2"]) if xl else True)
    assert os.path.exists(tmp_path / "merged" / "special_params.json")
    assert any(f.endswith("_embeddings.safetensors") for f in os.listdir(tmp_path / "merged"))
    # the merged weights against the adapters of the checkpoint (fp64)
    acfg = json.load(open(os.path.join(out_dir, "adapter_config.json")))
    s = acfg["lora_alpha"] / acfg["r"]
    base, merged = load_file(paths["unet"]), load_file(files["unet"])
    lora_file = next(os.path.join(out_dir, f) for f in os.listdir(out_dir) if f.endswith("_lora.safetensors"))
    lora = MG.ckpt.load_lora(lora_file, topology.lora_targets(topology.CONFIGS[version]))
    for name, (A, B, *mg) in lora.items():
        w = base[name + ".weight"].double()
        ref = w + s * (B.flatten(1).double() @ A.flatten(1).double()).reshape(w.shape)
        if mg:
            ref = (mg[0].double().reshape(-1) / ref.flatten(1).norm(dim=1)).view(-1, *([1] * (w.dim() - 1))) * ref
        assert float((merged[name + ".weight"].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-7, name
    te_base, te_m = load_file(paths["te0"]), load_file(files["text_encoder"])
    assert set(te_m) == set(te_base)
    assert any(not torch.equal(te_m[k], te_base[k]) for k in te_m if "self_attn" in k and k.endswith(".weight"))
    # fresh job on the merged model
    pm = {"path": files["unet"], "text_encoder_path": files["text_encoder"]}
    if xl:
        pm["text_encoder_2_path"] = files["text_encoder_2"]
    cfg2 = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", pretrained_model=pm, seed=2, resolution=128, train_batch_size=1,
                          max_train_steps=1, checkpointing_steps=1000, n_sample_imgs=0, output_dir=str(tmp_path / "job2"))
    cfg2.sd_model_version = version           # (the toy topologies are not told apart from the real ones by their key names)
    progress, (config2, out2) = _run(T.train(cfg2, runtime=mk_rt()))
    assert progress[-1] == 1.0
    ta = json.load(open(os.path.join(out2, "training_args.json")))
    assert all(np.isfinite(ta["training_attributes"]["losses"]["tot_loss"]))


def test_detect_version():
    from sd_lora_trainer_amd import merge as MG
    for v in ("tiny15", "tinyxl"):
        sd = {k: torch.empty(s, device="meta") for k, s in topology.param_shapes(topology.CONFIGS[v]).items()}
        assert MG.detect_version(sd) == v
