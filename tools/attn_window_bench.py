"""What tiled self-attention (HyperTile) costs and saves, in ONE session with the variants alternating:
(i) the kernel at B = 2, H = 10, d = 64 on 64 x 64 and 128 x 128 token grids (SDXL's largest self-attention at 1024 and 2048 px) with 1 x 1, 2 x 2 and 4 x 4 tiles:
    (a) sdlt_attn_fwd on the whole grid (the parent's launch: no tiles, the yardstick), (b) torch index gather of q, k, v into tile-major rows + sdlt_attn_fwd
    with the tiles as batch + index scatter of O (what the parent could do), (c) sdlt_attn_window_fwd; q, k, v are column views of one [M, 3 C] buffer as in the
    UNet - device events around `launches` back-to-back launches, median (min .. max) of `repeats` rounds after a warm-up;
(ii) one replayed SDXL iteration (random weights, rank-16 adapters, --latent 256 = 2048 px, the shape of a hires pass) without and with hypertile (--tile latent
    cells, --depth) - wall ms per iteration of `steps`-step graph samples, median (min .. max) of `repeats` rounds after a warm-up.

    python tools/attn_window_bench.py [--out profiles/hypertile_render_bench.txt] [--repeats 3] [--latent 256] [--tile 32] [--depth 0] [--steps 4] [--kernel-only]
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
    lines = [f"# (i) device-event us per call, B = 2, H = 10, d = 64, {launches} calls back to back: median (min .. max) of {repeats} rounds, alternated",
             f"{'grid':>9} {'tiles':>6} {'variant':<44} {'us / call':>11} {'min':>10} {'max':>10}"]
    B, H, d = 2, 10, 64
    C = H * d
    for side in (64, 128):
        N, M = side * side, B * side * side
        qkv = torch.randn(M, 3 * C, device="cuda", generator=g).to(BF16)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        O, L = torch.zeros(M, C, dtype=BF16, device="cuda"), torch.zeros(B * H * N, dtype=F32, device="cuda")
        kinds = {(1, "(a) sdlt_attn_fwd, whole grid"): lambda: ops.attn_fwd(q, k, v, None, O, L, B=B, H=H, Nq=N, Nk=N, Nqp=N, Nkp=N, d=d, scale=0.125)}
        for t in (1, 2, 4):
            n, T = N // (t * t), B * t * t
            idx = torch.arange(M, device="cuda").view(B, t, side // t, t, side // t).permute(0, 1, 3, 2, 4).reshape(-1)      # tile-major row order
            gq, gk, gv, gO = (torch.zeros(M, C, dtype=BF16, device="cuda") for _ in range(4))

            def gathered(idx=idx, gq=gq, gk=gk, gv=gv, gO=gO, n=n, T=T):
                torch.index_select(q, 0, idx, out=gq), torch.index_select(k, 0, idx, out=gk), torch.index_select(v, 0, idx, out=gv)
                ops.attn_fwd(gq, gk, gv, None, gO, L, B=T, H=H, Nq=n, Nk=n, Nqp=n, Nkp=n, d=d, scale=0.125)
                O.index_copy_(0, idx, gO)
            if t > 1:
                kinds[(t, "(b) gather + sdlt_attn_fwd (tiles as batch) + scatter")] = gathered
            kinds[(t, "(c) sdlt_attn_window_fwd")] = lambda t=t: ops.attn_window_fwd(q, k, v, O, B=B, H=H, grid=(side, side), tiles=(t, t), d=d, scale=0.125)
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
        for (t, name), ts in times.items():
            lines.append(f"{side:>4} x {side:<4} {t:>2} x {t:<2} {name:<44} {statistics.median(ts):>11.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
    return lines


def iteration_times(version, h, tile, depth, steps, repeats, rank=16):
    import render_bench as RB
    cfg, smp = RB.build(version, 1, rank)
    em = RB.embeds(cfg, 1)
    noise = torch.randn(1, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    variants = {"plain": lambda: smp.sample(em[0], h, h, steps=steps, latents=noise, graph=True),
                f"hypertile tile={tile} depth={depth}": lambda: smp.sample(em[0], h, h, steps=steps, latents=noise, graph=True, hypertile=dict(tile=tile, depth=depth))}
    times = {k: [] for k in variants}
    for r in range(repeats + 1):                            # round 0: warm-up (buffers, packed weights, the captures)
        for k, fn in variants.items():
            t = RB.timed(fn) * 1e3 / steps
            if r:
                times[k].append(t)
    from sd_lora_trainer_amd.sampler import hypertile_plan
    plan = hypertile_plan(h, h, {lv for _, lv in smp.unet._attn_levels()}, tile, depth)
    lines = [f"# (ii) {version} topology, {h} x {h} latent ({8 * h} px), batch 2, rank {rank}, {steps}-step graph samples, tiles {plan}; wall ms per iteration: "
             f"median (min .. max) of {repeats} rounds, alternated",
             f"{'variant':<28} {'ms / iteration':>16} {'min':>9} {'max':>9} {'/ plain':>9}"]
    base = statistics.median(times["plain"])
    for k, t in times.items():
        lines.append(f"{k:<28} {statistics.median(t):>16.3f} {min(t):>9.3f} {max(t):>9.3f} {statistics.median(t) / base:>9.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, default=256)
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}"] + kernel_times(a.launches, a.repeats)
    if not a.kernel_only:
        lines += iteration_times(a.version, a.latent, a.tile, a.depth, a.steps, a.repeats)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
