"""What self-attention guidance (SAG) costs, in ONE session with the variants alternating:
(i) per call at B = 2 (n = 1 image, the negative row) on the mid-block shapes - 32 x 32 tokens x 1280 channels (H = 20, d = 64: SDXL at 1024 px) and 8 x 8 x 1280
    (H = 8, d = 160: SD1.5 at 512 px): sdlt_attn_fwd on the same operands (the launch that leaves q, k and L: the yardstick), sdlt_attn_colmass (its two launches),
    sdlt_sag_degrade and one sdlt_sag_apply phase on the latent of that picture - `launches` calls captured into one graph, device events around `replays`
    replays of it, median (min .. max) of `repeats` rounds after a warm-up;
(ii) one replayed SDXL iteration (random weights, rank-16 adapters) at the given latent sizes, plain and with sag - wall ms per iteration of `steps`-step graph
    samples, median (min .. max) of `repeats` rounds after a warm-up.

    python tools/sag_bench.py [--out profiles/sag_render_bench.txt] [--repeats 3] [--latent 128] [--steps 4] [--kernel-only]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def kernel_times(launches, replays, repeats):
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    lines = [f"# (i) device-event us per call, B = 2, n = 1, {replays} replays of a graph of {launches} calls: median (min .. max) of {repeats} rounds, alternated",
             f"{'grid x C, d':>20} {'launch':<40} {'us / call':>11} {'min':>10} {'max':>10}"]
    B = 2
    for side, C, d, lat in ((32, 1280, 64, 128), (8, 1280, 160, 64)):
        H, N = C // d, side * side
        qkv = torch.randn(B * N, 3 * C, device="cuda", generator=g).to(BF16)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        O, L = torch.zeros(B * N, C, dtype=BF16, device="cuda"), torch.zeros(B * H * N, dtype=F32, device="cuda")
        mass, ws = torch.zeros(1, N, dtype=F32, device="cuda"), torch.zeros(H * N, dtype=F32, device="cuda")
        x, eps = torch.randn(1, 4, lat, lat, device="cuda", generator=g), torch.randn(2 * lat * lat, 4, device="cuda", generator=g)
        t, x64 = torch.randn(lat * lat, 4, device="cuda", generator=g), torch.zeros(lat * lat, 64, dtype=BF16, device="cuda")
        stab, ctr, taps = torch.tensor([[1.0, 0, 0, 0], [3.0, 0.5, 1.0, 0]], device="cuda"), torch.zeros(2, dtype=I32, device="cuda"), ops.blur_taps(2.0, 4).cuda()
        kinds = {"sdlt_attn_fwd (leaves q, k, L)": lambda: ops.attn_fwd(q, k, v, None, O, L, B=B, H=H, Nq=N, Nk=N, Nqp=N, Nkp=N, d=d, scale=d ** -0.5),
                 "sdlt_attn_colmass (both launches)": lambda: ops.attn_colmass(q, k, L, mass, B=B, H=H, N=N, d=d, scale=d ** -0.5, n=1, row_off=0, row_stride=2, ws=ws),
                 f"sdlt_sag_degrade, {lat} x {lat} latent": lambda: ops.sag_degrade(x, eps, mass, taps, stab, ctr, x64, grid=(side, side)),
                 f"sdlt_sag_apply phase 0, {lat} x {lat}": lambda: ops.sag_apply(eps, t, stab, ctr, 1, 0)}
        times, graphs = {k_: [] for k_ in kinds}, {}
        for k_, fn in kinds.items():                        # one eager call each (attn_fwd leaves the L colmass reads), then the capture
            fn()
            torch.cuda.synchronize()
            graphs[k_] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k_]):
                for _ in range(launches):
                    fn()
        for rnd in range(repeats + 1):                      # round 0: warm-up
            for k_, gr in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(replays):
                    gr.replay()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[k_].append(e0.elapsed_time(e1) * 1e3 / (launches * replays))
        for name, ts in times.items():
            lines.append(f"{side:>4} x {side:<3} x {C:<4} {d:>4} {name:<40} {statistics.median(ts):>11.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
        # the least the hardware could take for colmass: 2 N^2 d H flops per image on the bf16 MFMAs (MI355X_MICROARCH.md has the peak)
        lines.append(f"{side:>4} x {side:<3} x {C:<4} {d:>4} {'colmass: GFLOP per call (2 N^2 H d)':<40} {2.0 * N * N * H * d / 1e9:>11.3f}")
    return lines


def iteration_times(version, h, steps, repeats, rank=16):
    import render_bench as RB
    cfg, smp = RB.build(version, 1, rank)
    em = RB.embeds(cfg, 1)
    noise = torch.randn(1, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    variants = {"plain": {}, "sag (0.5, 2.0, 1.0)": dict(sag=True)}
    times = {k: [] for k in variants}
    for rnd in range(repeats + 1):                          # round 0: warm-up (buffers, packed weights, the plan clone, the captures)
        for k, kw in variants.items():
            t = RB.timed(lambda: smp.sample(em[0], h, h, steps=steps, latents=noise, graph=True, **kw)) * 1e3 / steps
            if rnd:
                times[k].append(t)
    lines = [f"# (ii) {version} topology, {h} x {h} latent ({8 * h} px), batch 2 (sag: the second forward at batch 1), rank {rank}, {steps}-step graph samples; "
             f"wall ms per iteration: median (min .. max) of {repeats} rounds, alternated",
             f"{'variant':<28} {'ms / iteration':>16} {'min':>9} {'max':>9} {'/ plain':>9}"]
    base = statistics.median(times["plain"])
    for k, t in times.items():
        lines.append(f"{k:<28} {statistics.median(t):>16.3f} {min(t):>9.3f} {max(t):>9.3f} {statistics.median(t) / base:>9.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, nargs="+", default=[128])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}"] + kernel_times(a.launches, a.replays, a.repeats)
    if not a.kernel_only:
        for h in a.latent:
            lines += iteration_times(a.version, h, a.steps, a.repeats)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
