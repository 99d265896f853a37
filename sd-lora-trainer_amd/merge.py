"""Merge a trained checkpoint's adapters into the base weights: a standalone UNet (and text encoders) instead of base + adapter file - what
the reference's inference script does with `pipe.fuse_lora()` (scripts/test_inference.py:53) and kohya's merge_lora.

    python -m sd_lora_trainer_amd.merge --unet BASE.safetensors --checkpoint CKPT_DIR --out DIR [--lora-scale X] [--dtype bf16|fp16|fp32]
                                        [--text-encoder F] [--text-encoder-2 F]

CKPT_DIR is what train() / checkpoint.save_checkpoint wrote: the kohya adapter file (`*_lora.safetensors`, with `.dora_scale` for DoRA),
adapter_config.json, the embeddings and special_params.json.  The kohya file stores alpha = r whatever the multiplier was, so lora_alpha / r
comes from adapter_config.json.  The adapters are loaded into a unet.LoraArena and merged on the GPU (ops.MergePlan -> sdlt_lora_merge);
the output directory is checkpoint.save_merged's.
"""
import argparse
import json
import os

import torch
from safetensors.torch import load_file

from . import checkpoint as ckpt
from . import topology


def detect_version(sd):
    """The topology whose parameter names and shapes are exactly those of the state dict sd."""
    for v, cfg in topology.CONFIGS.items():
        shapes = topology.param_shapes(cfg)
        if len(shapes) == len(sd) and all(k in sd and tuple(sd[k].shape) == tuple(s) for k, s in shapes.items()):
            return v
    raise ValueError("the UNet state dict matches none of the known topologies (" + ", ".join(topology.CONFIGS) + ")")


def build_arena(rt, modules, rank, alpha_multiplier, dora):
    """A LoraArena holding the given modules' adapters: modules = [(name, base weight)], the weight giving [N, K] (3x3 conv: [Cout, Cin, 3, 3]).
    DoRA entries carry the bf16 forward operand the arena's magnitude initialisation reads (the loaded magnitudes replace it)."""
    from . import unet as M
    arena = M.LoraArena(rt, rank, alpha_multiplier, problems=[], dora=dora)
    for name, w in modules:
        if w.dim() == 4 and w.shape[-1] == 3:
            N, cin = w.shape[0], w.shape[1]
            wop = w.permute(0, 2, 3, 1).reshape(N, 9 * cin) if dora else None
            arena.add(name, N, 9 * cin, conv_cin=cin, W=None if wop is None else wop.to(rt.device, torch.bfloat16).contiguous())
        else:
            N, K = w.shape[0], w.numel() // w.shape[0]
            arena.add(name, N, K, W=w.reshape(N, K).to(rt.device, torch.bfloat16).contiguous() if dora else None)
    arena.finalize()
    return arena


def _load_text_lora(lora_sd, te_sd, prefix):
    """prefixed module name -> (A, B[, magnitude]) of every text-encoder module the kohya file adapts (lora_te1_ / lora_te2_ keys)."""
    mods = {}
    for k, w in te_sd.items():
        if not k.endswith(".weight") or w.dim() != 2:
            continue
        name = prefix + k[: -len(".weight")]
        base = ckpt.kohya_text_key(name)
        if base + ".lora_down.weight" in lora_sd:
            mods[name] = ((lora_sd[base + ".lora_down.weight"].float(), lora_sd[base + ".lora_up.weight"].float())
                          + ((lora_sd[base + ".dora_scale"].float(),) if base + ".dora_scale" in lora_sd else ()))
    return mods


def merge(unet_path, checkpoint_dir, out_dir, *, lora_scale=1.0, dtype="bf16", text_encoder=None, text_encoder_2=None, runtime=None):
    """-> the files checkpoint.save_merged wrote.  runtime: a unet.Runtime to merge on (default: cuda:0)."""
    from . import unet as M
    rt = runtime or M.Runtime("cuda:0", 1)
    base = load_file(unet_path) if unet_path.endswith(".safetensors") else torch.load(unet_path, map_location="cpu")
    version = detect_version(base)
    lora_file = next((os.path.join(checkpoint_dir, f) for f in sorted(os.listdir(checkpoint_dir)) if f.endswith("_lora.safetensors")), None)
    if lora_file is None:
        raise FileNotFoundError(f"{checkpoint_dir}: no *_lora.safetensors adapter file")
    with open(os.path.join(checkpoint_dir, "adapter_config.json")) as f:
        acfg = json.load(f)
    mult = float(acfg["lora_alpha"]) / float(acfg["r"])          # the kohya file's alpha is r whatever the multiplier was
    dora = bool(acfg.get("use_dora", False))
    lora_sd = load_file(lora_file)
    targets = topology.lora_targets(topology.CONFIGS[version])
    lora = ckpt.load_lora(lora_file, targets)
    rank = next(iter(lora.values()))[0].shape[0]
    arena = build_arena(rt, [(n, base[n + ".weight"]) for n in targets], rank, mult, dora)
    arena.load(lora)
    te_paths = [p for p in (text_encoder, text_encoder_2) if p]
    text_arena, te_sds = None, None
    if any(k.startswith("lora_te") for k in lora_sd):
        if not te_paths:
            raise ValueError("the checkpoint holds text-encoder adapters: pass --text-encoder (and --text-encoder-2 for SDXL)")
        te_sds = [load_file(p) if p.endswith(".safetensors") else torch.load(p, map_location="cpu") for p in te_paths]
        te_lora = {}
        for pre, sd in zip(ckpt.TEXT_PREFIXES, te_sds):
            te_lora.update(_load_text_lora(lora_sd, sd, pre))
        te_rank = next(iter(te_lora.values()))[0].shape[0]
        view = {}
        for pre, sd in zip(ckpt.TEXT_PREFIXES, te_sds):
            view.update({pre + k: v for k, v in sd.items()})
        text_arena = build_arena(rt, [(n, view[n + ".weight"]) for n in te_lora], te_rank, mult, dora)
        text_arena.load(te_lora)
    return ckpt.save_merged(out_dir, base, arena, version, scale=lora_scale, text_arena=text_arena, te_base_sds=te_sds, dtype=ckpt.DTYPES[dtype],
                            checkpoint_dir=checkpoint_dir)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m sd_lora_trainer_amd.merge", description=__doc__.split("\n\n")[0])
    ap.add_argument("--unet", required=True, help="base UNet weights (.safetensors, diffusers names)")
    ap.add_argument("--checkpoint", required=True, help="checkpoint directory written by train()")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--lora-scale", type=float, default=1.0, help="adapter weight (sample_imgs_lora_scale semantics), default 1.0")
    ap.add_argument("--dtype", choices=sorted(ckpt.DTYPES), default="bf16")
    ap.add_argument("--text-encoder", default=None, help="base text encoder (Hugging Face state dict) - needed when the checkpoint adapts it")
    ap.add_argument("--text-encoder-2", default=None, help="SDXL's second text encoder")
    a = ap.parse_args(argv)
    files = merge(a.unet, a.checkpoint, a.out, lora_scale=a.lora_scale, dtype=a.dtype, text_encoder=a.text_encoder, text_encoder_2=a.text_encoder_2)
    for k, v in files.items():
        print(f"{k}: {v}")
    return files


if __name__ == "__main__":
    main()
