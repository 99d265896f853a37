"""Bit record of the optimizer kernels: four steps on fixed seeds through whichever library SDLT_KERNEL_LIB selects, one SHA-256 per output tensor.  Two builds compute the
same bits when their outputs are the same text.  usage: SDLT_KERNEL_LIB=<lib> python tools/optim_bits.py > profiles/<name>.txt ; diff"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sd_lora_trainer_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
gen = torch.Generator().manual_seed(12)


def hyper(step, l1c=0.0):
    h = torch.zeros(16, dtype=F32)
    h[:9] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** step, 1 - 0.999 ** step, l1c, 1.0])
    return h.to(dev)


def grad(n, step):
    x = torch.randn(n, generator=gen) * 1e-3 * (1 + step % 3)
    x[torch.rand(n, generator=gen) < 2e-3] *= 1e4
    return x.to(dev)


def show(tag, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        print(f"{tag:28s} {k:7s} {hashlib.sha256(t.contiguous().view(U8).cpu().numpy().tobytes()).hexdigest()}")


def tiles(rows, cols, off, kind):
    n = rows * cols
    p, g = torch.zeros(off + n + 63, dtype=F32, device=dev), torch.zeros(off + n + 63, dtype=F32, device=dev)
    p[off: off + n] = (torch.randn(n, generator=gen) * 0.05).to(dev)
    W, Wt = torch.zeros(rows, (cols + 7) // 8 * 8, dtype=BF16, device=dev), torch.zeros(cols, (rows + 7) // 8 * 8, dtype=BF16, device=dev)
    plan = ops.ShadowPlan([(off, rows, cols, cols, W, Wt)], dev)
    nb, tag = plan.n_blocks, f"{kind} {rows}x{cols}@{off}"
    if kind == "adamw8":
        m, v, absmax, tables = torch.zeros(4096 * nb, dtype=U8, device=dev), torch.zeros(4096 * nb, dtype=U8, device=dev), torch.zeros(4 * nb, dtype=F32, device=dev), ops.q8_tables(dev)
    else:
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 5):
        g[off: off + n] = grad(n, step)
        if kind == "adamw8":
            plan.adamw8(p, g, m, v, absmax, tables, hyper(step))
            show(f"{tag} step{step}", p=p, m8=m, v8=v, absmax=absmax, W=W, Wt=Wt)
        else:
            plan.adamw(p, g, m, v, hyper(step))
            show(f"{tag} step{step}", p=p, m=m, v=v, W=W, Wt=Wt)
    if kind == "adamw":
        W.zero_(), Wt.zero_()
        plan.run(p)
        show(f"refresh {rows}x{cols}@{off}", W=W, Wt=Wt)


def flat(n, kind, shift=0, l1=False):
    p, g = torch.zeros(n + shift, dtype=F32, device=dev)[shift:], torch.zeros(n + shift, dtype=F32, device=dev)[shift:]
    p.copy_((torch.randn(n, generator=gen) * 0.05).to(dev))
    if kind == "adamw8_flat":
        m, v, absmax, tables = torch.zeros(n, dtype=U8, device=dev), torch.zeros(n, dtype=U8, device=dev), torch.zeros(2 * ((n + 2047) // 2048), dtype=F32, device=dev), ops.q8_tables(dev)
    else:
        m, v, l1_sum = torch.zeros(n + shift, dtype=F32, device=dev)[shift:], torch.zeros(n + shift, dtype=F32, device=dev)[shift:], torch.zeros(1, dtype=F32, device=dev)
    for step in range(1, 5):
        g.copy_(grad(n, step))
        if kind == "adamw8_flat":
            ops.adamw8_flat(p, g, m, v, absmax, tables, hyper(step))
            show(f"{kind} n={n} step{step}", p=p, m8=m, v8=v, absmax=absmax)
        else:          # (the L1 sum itself is an atomic sum over workgroups: not a bit record)
            ops.adamw_fused(p, g, m, v, hyper(step, 1e-6 if l1 else 0.0), l1_sum if l1 else None)
            show(f"{kind} n={n}+{shift} l1={int(l1)} step{step}", p=p, m=m, v=v)


for rows, cols, off in ((96, 64, 128), (96, 64, 129), (100, 77, 128), (64, 128, 128)):
    tiles(rows, cols, off, "adamw8")
for rows, cols in ((70, 192), (200, 130)):
    tiles(rows, cols, 128, "adamw")
for shift in (0, 1):
    for l1 in (False, True):
        flat(4099, "adamw_fused", shift, l1)
for n in (6144, 28):
    flat(n, "adamw8_flat")
