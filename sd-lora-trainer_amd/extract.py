"""Adapters from weight differences - the inverse of `merge`: a tuned model (a full fine-tune, or a merged checkpoint) minus its base becomes
the kohya LoRA file every consumer of this project reads, and a wide adapter becomes its best narrow one (kohya's extract_lora_from_models
and resize_lora next to merge_lora).

    python -m sd_lora_trainer_amd.extract --base BASE.safetensors --tuned TUNED.safetensors|DIR --rank R --out DIR
                                          [--energy F] [--oversample P] [--power-iters Q] [--seed S] [--dtype bf16|fp16|fp32]
                                          [--text-encoder F --tuned-text-encoder F [--text-encoder-2 F --tuned-text-encoder-2 F]] [--checkpoint CKPT_DIR]
    python -m sd_lora_trainer_amd.extract --resize CKPT_DIR --rank R --out DIR [--energy F] [--dtype ...]

Extraction is a randomized subspace iteration (Halko, Martinsson, Tropp 2011, algorithms 4.4 + 5.1) over ALL adapted layers at once: with
D = W1 - W0 of a layer ([N, K]; 3x3 conv: tap-major [Cout, 9 Cin]) and L = rank + oversample columns (rounded up to a multiple of 16),
    Y = D Omega, Q = orth(Y) ;  q times:  Z = D^T Q, Q' = orth(Z), Y = D Q', Q = orth(Y) ;  C = D^T Q ;  D ~ Q C^T = U S V^T
and B = U_r S_r^(1/2), A = S_r^(1/2) V_r^T (lora_alpha = r: scale 1).  Every product with D is ONE sdlt_delta_matmul launch for the whole
model (ops.DeltaPlan: the difference is formed in fp32 registers, f32-input MFMA) - 2 q + 2 launches; the orthonormalisations (Householder
QR) and the L-sized factorisation run in fp64 through torch.linalg, batched over the layers of one shape.  Nothing synchronises per layer.
The text encoders' q/k/v/out projections are added when tuned text-encoder files are given.

A LoRA file holds the targeted layers only (to_q / to_k / to_v / to_out.0 / conv2).  What a full fine-tune moved elsewhere (feed-forward,
conv1, norms, biases) cannot be represented in it: `coverage` is the share of sum ||W1 - W0||_F^2 over all UNet tensors that lies in the
targeted layers - 1 for a merged LoRA, below 1 for a full fine-tune - and the command prints it.

Resizing needs no large product: D = s B A is given in factors, so QR of B and of A^T, the SVD of the r x r core and truncation, all fp64.
"""
import argparse
import json
import os
import shutil

import torch
from safetensors.torch import load_file

from . import checkpoint as ckpt
from . import topology
from .merge import detect_version

F32, F64 = torch.float32, torch.float64
TEXT_SUFFIXES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj")


def padded_columns(rank, oversample):
    """Columns of the range finder: rank + oversample rounded up to the kernel's multiple of 16."""
    L = -(-(rank + oversample) // 16) * 16
    if rank < 1 or L > 272:
        raise ValueError(f"rank {rank} + oversample {oversample}: the range finder takes up to 272 columns")
    return L


def weight_view(w, device):
    """The [N, K] operand of a layer's weight as LoraArena.merged() views it (3x3 conv: tap-major [Cout, 9 Cin]); bf16 / fp16 / fp32 kept."""
    w = w.to(device)
    if w.dim() == 4 and w.shape[-1] == 3:
        w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    else:
        w = w.reshape(w.shape[0], -1)
    if w.dtype not in (torch.bfloat16, torch.float16, F32):
        w = w.float()
    return w.contiguous()


def shape_groups(shapes):
    """[(N, K)] per layer -> [((N, K), [layer indices])] in order of first appearance: the batches of the torch.linalg steps."""
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(tuple(s), []).append(i)
    return list(groups.items())


def draw_omega(shapes, L, seed):
    """The test matrices: one seeded CPU generator, a [G, K, L] normal draw per shape group in shape_groups() order (the same numbers on
    every device)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(len(idx), K, L, generator=g, dtype=F32) for (N, K), idx in shape_groups(shapes)]


def _orth(P):
    """In place: the columns of every [rows, L] panel of P [G, rows, L] replaced by an orthonormal basis of their span (Householder QR in
    fp64 - it also serves rank-deficient panels, which an exactly low-rank difference produces); panels with rows < L keep `rows` columns."""
    Q = torch.linalg.qr(P.to(F64), mode="reduced")[0]
    if Q.shape[2] < P.shape[2]:
        P.zero_()
    P[:, :, : Q.shape[2]].copy_(Q)


def kept_count(s2, total, rank, energy):
    """Per layer: the smallest count <= rank whose sigma^2 sum reaches energy * total (rank where it is not reached, or energy is None).
    s2 [G, >= rank] descending, total [G]."""
    full = torch.full(s2.shape[:1], rank, dtype=torch.int64, device=s2.device)
    if energy is None:
        return full
    reach = torch.cumsum(s2[:, :rank], 1) >= (float(energy) * total).unsqueeze(1)
    first = torch.where(reach.any(1), reach.to(torch.int64).argmax(1) + 1, full)
    return first.clamp(max=rank)


def _factors(U, S, Vt, rank, keep):
    """B = U_r S_r^(1/2), A = S_r^(1/2) V_r^T in fp32 with the components past `keep` (per layer) exactly zero."""
    r = min(rank, S.shape[1])
    mask = (torch.arange(r, device=S.device).unsqueeze(0) < keep.unsqueeze(1)).to(F64)
    rs = S[:, :r].clamp(min=0).sqrt() * mask
    B = torch.zeros(U.shape[0], U.shape[1], rank, dtype=F32, device=U.device)
    A = torch.zeros(U.shape[0], rank, Vt.shape[2], dtype=F32, device=U.device)
    B[:, :, :r] = (U[:, :, :r] * rs.unsqueeze(1)).to(F32)
    A[:, :r] = (rs.unsqueeze(2) * Vt[:, :r]).to(F32)
    return A, B


class Extracted:
    """What extract_adapters / resize_adapters return.  lora: module -> (A, B) in peft layout (LoraArena.load); layers: module ->
    dict(sigma: the kept singular values (fp64, zeroed components are 0), kept, delta_norm = ||D||_F, residual = ||D - B A||_F / ||D||_F
    (from the singular values: sqrt(||D||_F^2 - sum sigma^2))); coverage: see the module docstring (None when not computed)."""

    def __init__(self, rank, lora, layers, coverage):
        self.rank, self.lora, self.layers, self.coverage = rank, lora, layers, coverage

    def residuals(self):
        """{layer class: relative residual, ..., "overall": ...}: sqrt(sum ||D - B A||_F^2 / sum ||D||_F^2) over the layers of a class
        (the module name's last component; text-encoder modules under "te.<name>")."""
        num, den = {}, {}
        for name, l in self.layers.items():
            cls = name.rsplit(".", 1)[-1] if not name.startswith("text_encoder") else "te." + name.rsplit(".", 1)[-1]
            if cls == "0":
                cls = "to_out.0"
            for c in (cls, "overall"):
                num[c] = num.get(c, 0.0) + (l["residual"] * l["delta_norm"]) ** 2
                den[c] = den.get(c, 0.0) + l["delta_norm"] ** 2
        return {c: (num[c] / den[c]) ** 0.5 if den[c] > 0 else 0.0 for c in num}


def _peft_layout(A, B, w):
    """[r, K], [N, r] of the [N, K] view -> peft layout of the weight w (conv: A [r, Cin, 3, 3], B [Cout, r, 1, 1])."""
    if w.dim() == 4 and w.shape[-1] == 3:
        r = A.shape[0]
        return A.reshape(r, 3, 3, w.shape[1]).permute(0, 3, 1, 2).contiguous(), B.reshape(B.shape[0], r, 1, 1)
    return A, B


def extract_adapters(base_sd, tuned_sd, rank, *, oversample=16, power_iters=2, energy=None, seed=0, runtime=None, targets=None):
    """-> Extracted.  base_sd / tuned_sd: state dicts with the same keys (UNet: diffusers names; text encoders: under "text_encoder." /
    "text_encoder_2." prefixes); targets: module names (default: the LoRA targets of the topology base_sd matches).  runtime: a
    unet.Runtime whose device and op table (ops.DeltaPlan) the products use (default: cuda:0 with the HIP kernels)."""
    from . import unet as M
    rt = runtime or M.Runtime("cuda:0", 1)
    dev = rt.device
    if targets is None:
        targets = topology.lora_targets(topology.CONFIGS[detect_version(base_sd)])
    L = padded_columns(rank, oversample)
    W0 = [weight_view(base_sd[n + ".weight"], dev) for n in targets]
    W1 = [weight_view(tuned_sd[n + ".weight"], dev) for n in targets]
    shapes = [tuple(w.shape) for w in W0]
    for n, a, b in zip(targets, W0, W1):
        if a.shape != b.shape:
            raise ValueError(f"{n}.weight: base {tuple(a.shape)} and tuned {tuple(b.shape)} differ")
    groups = shape_groups(shapes)
    # per shape group: the K-side and the N-side panels of all its layers and the rows' sums of squares of D
    Pk = [om.to(dev) for om in draw_omega(shapes, L, seed)]
    Pn = [torch.zeros(len(idx), N, L, dtype=F32, device=dev) for (N, K), idx in groups]
    rowsq = [torch.zeros(len(idx), N, dtype=F32, device=dev) for (N, K), idx in groups]
    layers = [None] * len(targets)
    for g, (_, idx) in enumerate(groups):
        for j, i in enumerate(idx):
            layers[i] = dict(W0=W0[i], W1=W1[i], Pk=Pk[g][j], Pn=Pn[g][j], rowsq=rowsq[g][j])
    plan = rt.ops.DeltaPlan(layers, L, dev)

    def orth(panels):
        for P in panels:
            _orth(P)

    plan.forward()                      # Y = D Omega
    orth(Pn)
    for _ in range(power_iters):
        plan.transposed()               # Z = D^T Q
        orth(Pk)
        plan.forward()                  # Y = D Q'
        orth(Pn)
    plan.transposed()                   # C = D^T Q  ([K, L]);  D ~ Q C^T
    lora, info = {}, {}
    per_group = []
    for g, ((N, K), idx) in enumerate(groups):
        # C = Qc R (thin QR), R = Ur S Vr^T  =>  Q C^T = (Q Vr) S (Qc Ur)^T
        Qc, R = torch.linalg.qr(Pk[g].to(F64), mode="reduced")
        Ur, S, Vrt = torch.linalg.svd(R, full_matrices=False)
        U = Pn[g].to(F64)[:, :, : Vrt.shape[2]] @ Vrt.transpose(1, 2)
        Vt = (Qc @ Ur).transpose(1, 2)
        total = rowsq[g].to(F64).sum(1)
        keep = kept_count(S * S, total, rank, energy)
        A, B = _factors(U, S, Vt, rank, keep)
        r = min(rank, S.shape[1])
        sig = torch.zeros(len(idx), rank, dtype=F64, device=dev)
        sig[:, :r] = S[:, :r] * (torch.arange(r, device=dev).unsqueeze(0) < keep.unsqueeze(1))
        per_group.append((A, B, sig, keep, total))
    # coverage: squared differences of every tensor outside the targets, against the targeted layers' (one host read at the end)
    tkeys = {n + ".weight" for n in targets}
    inside = torch.stack([t.sum() for *_, t in per_group]).sum()
    outside = torch.zeros((), dtype=F64, device=dev)
    for k, v in base_sd.items():
        if k not in tkeys and k in tuned_sd and torch.is_floating_point(v):
            outside += (tuned_sd[k].to(dev, F32).double() - v.to(dev, F32).double()).pow(2).sum()
    cov = torch.where(inside + outside > 0, inside / (inside + outside), torch.ones_like(inside))
    host = [(A.cpu(), B.cpu(), sig.cpu(), keep.cpu(), total.cpu()) for A, B, sig, keep, total in per_group]
    coverage = float(cov)
    for (A, B, sig, keep, total), (_, idx) in zip(host, groups):
        for j, i in enumerate(idx):
            name = targets[i]
            lora[name] = _peft_layout(A[j], B[j], base_sd[name + ".weight"])
            t = float(total[j])
            res2 = max(t - float((sig[j] ** 2).sum()), 0.0)
            info[name] = dict(sigma=sig[j], kept=int(keep[j]), delta_norm=t ** 0.5, residual=(res2 / t) ** 0.5 if t > 0 else 0.0)
    return Extracted(rank, {n: lora[n] for n in targets}, {n: info[n] for n in targets}, coverage)


def split_lora_sd(lora_sd):
    """kohya state dict -> {kohya base key: (down, up)}; raises ValueError for DoRA files."""
    if any(k.endswith(".dora_scale") for k in lora_sd):
        raise ValueError("a DoRA checkpoint (.dora_scale keys) cannot be resized: the magnitude vector belongs to the full-rank direction "
                         "W + s B A and does not survive a truncation of B A")
    return {k[: -len(".lora_down.weight")]: (lora_sd[k], lora_sd[k[: -len(".lora_down.weight")] + ".lora_up.weight"])
            for k in lora_sd if k.endswith(".lora_down.weight")}


def resize_adapters(lora_sd, rank, energy=None, scale=1.0, device="cpu"):
    """-> Extracted with lora keyed by the kohya base keys of lora_sd (a kohya state dict: lora_down [r, K(, 3, 3)] / lora_up [N, r(, 1, 1)]):
    the best rank-`rank` approximation of D = scale * up * down per module, exactly: QR of up and of down^T, SVD of the r x r core, fp64.
    scale: lora_alpha / r of the file's adapter_config.json (the kohya `.alpha` this project writes is r whatever the multiplier was).
    The result's own scale is 1.  Conv factors keep the file's layout (down's (ci, ky, kx) column order)."""
    mods = split_lora_sd(lora_sd)
    names = list(mods)
    downs = [mods[n][0].to(device, F64).flatten(1) for n in names]
    ups = [mods[n][1].to(device, F64).flatten(1) for n in names]
    out, info = {}, {}
    for (N, K, r0), idx in shape_groups([(u.shape[0], d.shape[1], d.shape[0]) for u, d in zip(ups, downs)]):
        Bm = torch.stack([ups[i] for i in idx]) * float(scale)               # [G, N, r0]
        Am = torch.stack([downs[i] for i in idx])                            # [G, r0, K]
        Qb, Rb = torch.linalg.qr(Bm, mode="reduced")
        Qa, Ra = torch.linalg.qr(Am.transpose(1, 2), mode="reduced")
        Uc, S, Vct = torch.linalg.svd(Rb @ Ra.transpose(1, 2), full_matrices=False)
        U, Vt = Qb @ Uc, (Qa @ Vct.transpose(1, 2)).transpose(1, 2)
        total = (S * S).sum(1)
        keep = kept_count(S * S, total, min(rank, S.shape[1]), energy)
        A, B = _factors(U, S, Vt, rank, keep)
        for j, i in enumerate(idx):
            n = names[i]
            down, up = mods[n]
            out[n] = (A[j].reshape(rank, *down.shape[1:]).cpu(), B[j].reshape(up.shape[0], rank, *up.shape[2:]).cpu())
            r = min(rank, S.shape[1])
            sig = torch.zeros(rank, dtype=F64)
            sig[:r] = (S[j, :r] * (torch.arange(r, device=S.device) < keep[j])).cpu()
            t = float(total[j])
            info[n] = dict(sigma=sig, kept=int(keep[j]), delta_norm=t ** 0.5,
                           residual=(max(t - float((sig ** 2).sum()), 0.0) / t) ** 0.5 if t > 0 else 0.0)
    return Extracted(rank, out, info, None)


# ---------------------------------------------------------------------------------------- writing

class _Args:
    """training_args.json as far as render.load_for_inference reads it: concept_mode, n_tokens, is_lora, lora_rank, lora_alpha_multiplier,
    use_dora, pretrained_model (+ name, seed, sd_model_version, weight_type, disable_ti, text_encoder_lora_rank, lora_training_urls) - the
    job's own file from checkpoint_dir with the adapter fields replaced when there is one.  Stands in for the TrainingConfig that
    checkpoint.save_checkpoint asks for its tensor dtype (weight_type) and has write the file."""

    def __init__(self, checkpoint_dir, rank, te_rank, version, base_path, has_embeddings, weight_type):
        src = os.path.join(checkpoint_dir, "training_args.json") if checkpoint_dir else None
        if src and os.path.exists(src):
            with open(src) as f:
                data = json.load(f)
        else:
            data = {"lora_training_urls": "extracted", "concept_mode": "object", "name": "extracted", "seed": 0, "n_tokens": 3,
                    "pretrained_model": {"path": base_path, "version": version}, "sd_model_version": version if version in ("sdxl", "sd15") else None}
        data.update(is_lora=True, lora_rank=int(rank), lora_alpha_multiplier=1.0, use_dora=False, weight_type=weight_type)
        if te_rank is not None:
            data["text_encoder_lora_rank"] = int(te_rank)
        if not has_embeddings:
            data["disable_ti"] = True
        self.data, self.weight_type = data, weight_type

    def save_as_json(self, path):
        with open(path, "w") as f:
            json.dump(self.data, f, indent=4)


def arena_of(rt, lora, rank):
    """A LoraArena (LoRA, scale 1) holding the adapters lora: module -> (A, B) in peft layout; the layer shapes come from the factors
    ([N, K] from B's rows and A's columns; A [r, Cin, 3, 3]: a 3x3 conv)."""
    from . import unet as M
    arena = M.LoraArena(rt, rank, 1.0, problems=[], dora=False)
    for name, (A, B) in lora.items():
        if A.dim() == 4:
            arena.add(name, B.shape[0], 9 * A.shape[1], conv_cin=A.shape[1])
        else:
            arena.add(name, B.shape[0], A.shape[1])
    arena.finalize()
    arena.load(lora)
    return arena


def write_checkpoint(out_dir, rt, unet_lora, rank, version, *, text_lora=None, checkpoint_dir=None, name="extracted", base_path=None,
                     weight_type="bf16"):
    """The factors through a LoraArena and checkpoint.save_checkpoint (kohya keys, adapter_config.json), the embeddings and
    special_params.json copied from checkpoint_dir, and training_args.json (_Args); tensors leave in weight_type like a training job's.
    unet_lora / text_lora: module -> (A, B) in peft layout (text modules under their "text_encoder." / "text_encoder_2." names)."""
    arena = arena_of(rt, unet_lora, rank)
    text_arena = arena_of(rt, text_lora, next(iter(text_lora.values()))[0].shape[0]) if text_lora else None
    token_dict, copied = {}, []
    if checkpoint_dir:
        for f in sorted(os.listdir(checkpoint_dir)):
            if f.endswith("_embeddings.safetensors"):
                copied.append(f)
            elif f == "special_params.json":
                with open(os.path.join(checkpoint_dir, f)) as fh:
                    token_dict = json.load(fh)
        prev = next((f for f in sorted(os.listdir(checkpoint_dir)) if f.endswith("_lora.safetensors")), None)
        if prev is not None and name == "extracted":
            name = prev[: -len(f"_{version}_lora.safetensors")] if prev.endswith(f"_{version}_lora.safetensors") else name
    args = _Args(checkpoint_dir, rank, None if text_arena is None else text_arena.rank, version, base_path, bool(copied), weight_type)
    files = ckpt.save_checkpoint(out_dir, 0, arena, None, token_dict, name, version, config=args, text_arena=text_arena)
    for f in copied:
        shutil.copy(os.path.join(checkpoint_dir, f), os.path.join(out_dir, f))
        files[f] = os.path.join(out_dir, f)
    return files


def _load_sd(path):
    if os.path.isdir(path):
        path = os.path.join(path, "diffusion_pytorch_model.safetensors")
    return load_file(path) if path.endswith(".safetensors") else torch.load(path, map_location="cpu")


def text_targets(sd, prefix):
    return [prefix + k[: -len(".weight")] for k, w in sd.items() if k.endswith(".weight") and w.dim() == 2 and k[: -len(".weight")].endswith(TEXT_SUFFIXES)]


def _summary(ex, te=None):
    res = ex.residuals()
    if te is not None:
        res.update({k: v for k, v in te.residuals().items() if k != "overall"})
        res["text_overall"] = te.residuals()["overall"]
    return {"rank": ex.rank, "coverage": ex.coverage, "residual": res}


def extract(base_path, tuned_path, rank, out_dir, *, energy=None, oversample=16, power_iters=2, seed=0, text_encoders=(), tuned_text_encoders=(),
            checkpoint_dir=None, runtime=None, weight_type="bf16"):
    """The CLI's extraction mode -> (files, summary)."""
    from . import unet as M
    rt = runtime or M.Runtime("cuda:0", 1)
    base, tuned = _load_sd(base_path), _load_sd(tuned_path)
    version = detect_version(base)
    kw = dict(oversample=oversample, power_iters=power_iters, energy=energy, seed=seed, runtime=rt)
    ex = extract_adapters(base, tuned, rank, **kw)
    te = te_view = None
    if tuned_text_encoders:
        if len(text_encoders) != len(tuned_text_encoders):
            raise ValueError("every --tuned-text-encoder needs its base --text-encoder")
        te_view, tuned_view, tt = {}, {}, []
        for pre, b, t in zip(ckpt.TEXT_PREFIXES, text_encoders, tuned_text_encoders):
            bs, ts = _load_sd(b), _load_sd(t)
            te_view.update({pre + k: v for k, v in bs.items()})
            tuned_view.update({pre + k: v for k, v in ts.items()})
            tt += text_targets(bs, pre)
        te = extract_adapters(te_view, tuned_view, rank, targets=tt, **kw)
    files = write_checkpoint(out_dir, rt, ex.lora, rank, version, text_lora=te.lora if te else None, checkpoint_dir=checkpoint_dir,
                             base_path=base_path, weight_type=weight_type)
    return files, _summary(ex, te)


def resize(checkpoint_dir, rank, out_dir, *, energy=None, runtime=None, weight_type="bf16"):
    """The CLI's resize mode -> (files, summary): every module of CKPT_DIR's adapter file (UNet and text encoders) at the new rank."""
    from . import unet as M
    rt = runtime or M.Runtime("cuda:0", 1)
    lora_file = next((os.path.join(checkpoint_dir, f) for f in sorted(os.listdir(checkpoint_dir)) if f.endswith("_lora.safetensors")), None)
    if lora_file is None:
        raise FileNotFoundError(f"{checkpoint_dir}: no *_lora.safetensors adapter file")
    with open(os.path.join(checkpoint_dir, "adapter_config.json")) as f:
        acfg = json.load(f)
    lora_sd = load_file(lora_file)
    rz = resize_adapters(lora_sd, rank, energy, scale=float(acfg["lora_alpha"]) / float(acfg["r"]), device=rt.device)
    with open(os.path.join(checkpoint_dir, "training_args.json")) as f:
        ta = json.load(f)
    version = ta.get("sd_model_version") or (ta.get("pretrained_model") or {}).get("version")
    version = next((v for v in topology.CONFIGS if os.path.basename(lora_file).endswith(f"_{v}_lora.safetensors")), version)
    targets = topology.lora_targets(topology.CONFIGS[version])
    by_key = {ckpt.kohya_key(m): m for m in targets}
    unet_lora = {by_key[k]: v for k, v in rz.lora.items() if k in by_key}
    # text modules: "lora_te1_<path with _>" -> "text_encoder.<path with _>", which checkpoint.kohya_text_key maps back to the same key
    text_lora = {("text_encoder_2." if k.startswith("lora_te2_") else "text_encoder.") + k[len("lora_te1_"):]: v
                 for k, v in rz.lora.items() if k.startswith("lora_te")}
    files = write_checkpoint(out_dir, rt, unet_lora, rank, version, text_lora=text_lora or None, checkpoint_dir=checkpoint_dir, weight_type=weight_type)
    named = Extracted(rank, {}, {by_key.get(k, k): v for k, v in rz.layers.items()}, None)
    s = _summary(named)
    s["coverage"] = 1.0
    return files, s


def main(argv=None, runtime=None):
    ap = argparse.ArgumentParser(prog="python -m sd_lora_trainer_amd.extract", description=__doc__.split("\n\n")[0])
    ap.add_argument("--base", help="base UNet weights (.safetensors, diffusers names)")
    ap.add_argument("--tuned", help="tuned UNet weights: a .safetensors file or a directory with diffusion_pytorch_model.safetensors")
    ap.add_argument("--resize", metavar="CKPT_DIR", help="resize the adapters of this checkpoint directory instead of extracting")
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--out", required=True, help="output checkpoint directory")
    ap.add_argument("--energy", type=float, default=None, help="per layer, zero the components past this fraction of the squared singular values")
    ap.add_argument("--oversample", type=int, default=16)
    ap.add_argument("--power-iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--text-encoder", default=None, help="base text encoder (Hugging Face state dict)")
    ap.add_argument("--tuned-text-encoder", default=None)
    ap.add_argument("--text-encoder-2", default=None, help="SDXL's second text encoder")
    ap.add_argument("--tuned-text-encoder-2", default=None)
    ap.add_argument("--checkpoint", default=None, help="checkpoint directory whose embeddings, special_params.json and training_args.json are carried over")
    ap.add_argument("--dtype", choices=sorted(ckpt.DTYPES), default="bf16", help="dtype of the adapter file (a training job's weight_type)")
    a = ap.parse_args(argv)
    if a.resize:
        files, summary = resize(a.resize, a.rank, a.out, energy=a.energy, weight_type=a.dtype, runtime=runtime)
    else:
        if not (a.base and a.tuned):
            ap.error("--base and --tuned are required (or --resize CKPT_DIR)")
        files, summary = extract(a.base, a.tuned, a.rank, a.out, energy=a.energy, oversample=a.oversample, power_iters=a.power_iters, seed=a.seed,
                                 text_encoders=[p for p in (a.text_encoder, a.text_encoder_2) if p],
                                 tuned_text_encoders=[p for p in (a.tuned_text_encoder, a.tuned_text_encoder_2) if p], checkpoint_dir=a.checkpoint,
                                 weight_type=a.dtype, runtime=runtime)
    print(json.dumps(summary))
    return files, summary


if __name__ == "__main__":
    main()
