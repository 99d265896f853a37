"""Times sdlt_attn_nag_fwd against sdlt_attn_fwd on the same rows at SDXL's two cross-attention shapes (B = 2, 77 keys in 128-row pads, d = 64):
neg_row all -1 (the same work as the plain kernel) and the sampler's pair layout [-1, 0] (the positive row attends to both key sets).  Device events
around alternating blocks of launches; prints one line per shape.  Then one replayed SDXL iteration at 1024 px, 30-step graph samples, with and without
nag, alternated.  Needs a GPU."""
import math
import os
import statistics
import sys

import torch

from sd_lora_trainer_amd import ops

BF16, REPS, BLOCK = torch.bfloat16, 20, 50


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / BLOCK


def main():
    g = torch.Generator().manual_seed(0)
    for N, H in ((4096, 10), (1024, 20)):
        B, d, Nk, Nkp = 2, 64, 77, 128
        C = H * d
        q, k, v = (torch.randn(r, C, generator=g).to(BF16).cuda() for r in (B * N, B * Nkp, B * Nkp))
        O, L = torch.empty(B * N, C, dtype=BF16, device="cuda"), torch.empty(B * H * N, dtype=torch.float32, device="cuda")
        tab = torch.tensor([[5.0, 2.5, 0.5, 0.0]]).cuda()
        off, pair = (torch.tensor(r, dtype=torch.int32).cuda() for r in ([-1, -1], [-1, 0]))
        kw = dict(B=B, H=H, Nk=Nk, Nkp=Nkp, d=d, scale=1 / math.sqrt(d))
        runs = {"attn_fwd": lambda: ops.attn_fwd(q, k, v, None, O, L, Nq=N, Nqp=N, **kw),
                "nag off": lambda: ops.attn_nag_fwd(q, k, v, O, off, tab, Nq=N, **kw),
                "nag pair": lambda: ops.attn_nag_fwd(q, k, v, O, pair, tab, Nq=N, **kw)}
        for fn in runs.values():      # warm-up: code objects, the LDS attribute
            timed(fn)
        t = {name: [] for name in runs}
        for _ in range(REPS):         # alternating blocks
            for name, fn in runs.items():
                t[name].append(timed(fn))
        med = {name: statistics.median(ts) for name, ts in t.items()}
        print(f"N={N} H={H} d={d} B={B}: " + "  ".join(f"{name} {med[name]:.1f} us (min {min(t[name]):.1f}, max {max(t[name]):.1f})" for name in runs) +
              f"  ratios off {med['nag off'] / med['attn_fwd']:.2f} x, pair {med['nag pair'] / med['attn_fwd']:.2f} x", flush=True)


def iteration_times(h=128, steps=30, repeats=3, rank=16):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import render_bench as RB
    cfg, smp = RB.build("sdxl", 1, rank)
    em = RB.embeds(cfg, 1)
    noise = torch.randn(1, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    run = lambda **kw: smp.sample(em, h, h, steps=steps, latents=noise, graph=True, n_images=1, **kw)  # noqa: E731
    variants = {"plain": run, "nag (5, 2.5, 0.5)": lambda: run(nag=True), "nag, end above every sigma (all rows plain)": lambda: run(nag=dict(end=1e4))}
    times = {k: [] for k in variants}
    for r in range(repeats + 1):      # round 0: warm-up (buffers, packed weights, the captures)
        for k, fn in variants.items():
            t = RB.timed(fn) * 1e3 / steps
            if r:
                times[k].append(t)
    print(f"sdxl topology, {h} x {h} latent ({8 * h} px), 1 picture (batch 2), rank {rank}, {steps}-step graph samples; wall ms per iteration: median (min .. max) of {repeats} rounds, alternated")
    base = statistics.median(times["plain"])
    for k, t in times.items():
        print(f"{k:<46} {statistics.median(t):>9.3f} {min(t):>9.3f} {max(t):>9.3f}   {statistics.median(t) / base:.3f} x plain", flush=True)


if __name__ == "__main__":
    main()
    if "--kernel-only" not in sys.argv:
        iteration_times()
