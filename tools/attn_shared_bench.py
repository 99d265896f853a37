"""What style-aligned batches (shared self-attention) cost, in ONE session with the variants alternating:
(i) the kernels on SDXL's two self-attention shapes at 1024 px (N = 4096 x 10 heads, N = 1024 x 20 heads, d = 64) with B = 4 rows in groups of G = 2:
    (a) sdlt_attn_fwd at N keys (the plain launch, the yardstick: the shared kernel does 1.5 x its score work at G = 2), (b) what the parent would need: torch
    AdaIN of q and k (statistics and affine) + `cat` of K and V to [own; reference] + sdlt_attn_fwd at Nk = 2 N, (c) sdlt_adain_affine + sdlt_attn_shared_fwd;
    q, k, v are column views of one [M, 3 C] buffer as in the UNet - device events around `launches` back-to-back calls, median (min .. max) of `repeats`
    rounds after a warm-up;
(ii) one replayed SDXL iteration (random weights, rank-16 adapters, --latent 128 = 1024 px, two pictures a batch) without and with style_align - wall ms per
    iteration of `steps`-step graph samples, median (min .. max) of `repeats` rounds after a warm-up.

    python tools/attn_shared_bench.py [--out profiles/style_align_render_bench.txt] [--repeats 3] [--latent 128] [--steps 4] [--kernel-only]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16, F32 = torch.bfloat16, torch.float32


def kernel_times(launches, repeats):
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    B, G, d = 4, 2, 64
    lines = [f"# (i) device-event us per call, B = {B}, G = {G}, d = {d}, {launches} calls back to back: median (min .. max) of {repeats} rounds, alternated",
             f"{'N':>5} {'H':>3} {'variant':<58} {'us / call':>11} {'min':>10} {'max':>10}"]
    for N, H in ((4096, 10), (1024, 20)):
        C, M = H * d, B * N
        qkv = torch.randn(M, 3 * C, device="cuda", generator=g).to(BF16)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        O, L = torch.zeros(M, C, dtype=BF16, device="cuda"), torch.zeros(B * H * N, dtype=F32, device="cuda")
        A, S = torch.zeros(B, 2 * C, device="cuda"), torch.zeros(B, 2 * C, device="cuda")
        ws = torch.zeros(ops.adain_ws_floats(B, N, 2 * C), device="cuda")
        ref = torch.arange(B, device="cuda") // G * G
        qa, kk, vv = torch.zeros(M, C, dtype=BF16, device="cuda"), torch.zeros(B, 2 * N, C, dtype=BF16, device="cuda"), torch.zeros(B, 2 * N, C, dtype=BF16, device="cuda")

        def adain(t):      # torch AdaIN towards the group's first image
            x = t.float().view(B, N, C)
            mean, std = x.mean(1, keepdim=True), (x.var(1, keepdim=True) + 1e-5).sqrt()
            return ((x - mean) / std * std[ref] + mean[ref]).to(BF16)

        def parent():
            qa.copy_(adain(q).view(M, C))
            torch.cat([adain(k), k.view(B, N, C)[ref]], 1, out=kk)
            torch.cat([v.view(B, N, C), v.view(B, N, C)[ref]], 1, out=vv)
            ops.attn_fwd(qa, kk.view(-1, C), vv.view(-1, C), None, O, L, B=B, H=H, Nq=N, Nk=2 * N, Nqp=N, Nkp=2 * N, d=d, scale=0.125)

        def shared():
            ops.adain_affine(qkv[:, :2 * C], A, S, B=B, N=N, G=G, ws=ws)
            ops.attn_shared_fwd(q, k, v, O, B=B, H=H, N=N, d=d, G=G, scale=0.125, tables=(A[:, :C], S[:, :C], A[:, C:], S[:, C:]))
        kinds = {"(a) sdlt_attn_fwd, N keys (no sharing)": lambda: ops.attn_fwd(q, k, v, None, O, L, B=B, H=H, Nq=N, Nk=N, Nqp=N, Nkp=N, d=d, scale=0.125),
                 "(b) torch AdaIN + cat + sdlt_attn_fwd, 2 N keys": parent,
                 "(c) sdlt_adain_affine + sdlt_attn_shared_fwd": shared,
                 "    sdlt_adain_affine alone (both launches)": lambda: ops.adain_affine(qkv[:, :2 * C], A, S, B=B, N=N, G=G, ws=ws),
                 "    sdlt_attn_shared_fwd alone, no tables": lambda: ops.attn_shared_fwd(q, k, v, O, B=B, H=H, N=N, d=d, G=G, scale=0.125)}
        times = {k_: [] for k_ in kinds}
        for r in range(repeats + 1):                        # round 0: warm-up
            for k_, fn in kinds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[k_].append(e0.elapsed_time(e1) * 1e3 / launches)
        for name, ts in times.items():
            lines.append(f"{N:>5} {H:>3} {name:<58} {statistics.median(ts):>11.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
    return lines


def iteration_times(version, h, steps, repeats, rank=16):
    import render_bench as RB
    cfg, smp = RB.build(version, 2, rank)
    em = RB.embeds(cfg, 2)
    noise = torch.randn(2, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    run = lambda **kw: smp.sample(em, h, h, steps=steps, latents=noise, graph=True, n_images=2, **kw)  # noqa: E731
    variants = {"plain": run, "style_align (weight 1, adain qk)": lambda: run(style_align=True), "style_align, no adain": lambda: run(style_align=dict(adain=False))}
    times = {k: [] for k in variants}
    for r in range(repeats + 1):                            # round 0: warm-up (buffers, packed weights, the captures)
        for k, fn in variants.items():
            t = RB.timed(fn) * 1e3 / steps
            if r:
                times[k].append(t)
    lines = [f"# (ii) {version} topology, {h} x {h} latent ({8 * h} px), 2 pictures (batch 4), rank {rank}, {steps}-step graph samples; wall ms per iteration: "
             f"median (min .. max) of {repeats} rounds, alternated",
             f"{'variant':<36} {'ms / iteration':>16} {'min':>9} {'max':>9} {'/ plain':>9}"]
    base = statistics.median(times["plain"])
    for k, t in times.items():
        lines.append(f"{k:<36} {statistics.median(t):>16.3f} {min(t):>9.3f} {max(t):>9.3f} {statistics.median(t) / base:>9.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}"] + kernel_times(a.launches, a.repeats)
    if not a.kernel_only:
        lines += iteration_times(a.version, a.latent, a.steps, a.repeats)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
