"""What token merging (ToMe) costs and saves, in ONE session with the variants alternating:
(i) per call at B = 2 on 64 x 64 tokens x 640 channels (H = 10) and 32 x 32 x 1280 (H = 20), ratio 0.5: sdlt_attn_fwd on the full grid (the plain launch: the
    yardstick), the four token-merging launches each alone and sdlt_attn_fwd on the N / 2 merged rows - `launches` calls captured into one graph, device events
    around `replays` replays of it (the host enqueues one graph, not every launch, so the 10 us launches are not timed at the rate Python can issue them),
    median (min .. max) of `repeats` rounds after a warm-up;
(ii) one replayed SDXL iteration (random weights, rank-16 adapters) at the given latent sizes: plain, token merging on the largest grid, and on both grids -
    wall ms per iteration of `steps`-step graph samples, median (min .. max) of `repeats` rounds after a warm-up.

    python tools/tome_bench.py [--out profiles/tome_render_bench.txt] [--repeats 3] [--latent 128 256] [--steps 4] [--kernel-only]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def kernel_times(launches, replays, repeats, ratio=0.5):
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    lines = [f"# (i) device-event us per call, B = 2, d = 64, ratio {ratio}, mode random, {replays} replays of a graph of {launches} calls: median (min .. max) of {repeats} rounds, alternated",
             f"{'grid x C':>16} {'launch':<44} {'us / call':>11} {'min':>10} {'max':>10}"]
    B, d = 2, 64
    for side, C in ((64, 640), (32, 1280)):
        H, N, grid = C // d, side * side, (side, side)
        r = ops.tome_rows(N, ratio)
        Np, Nd, Ns = N - r, N // 4, N - N // 4
        qkv = torch.randn(B * N, 3 * C, device="cuda", generator=g).to(BF16)
        y, res = torch.randn(B * N, C, device="cuda", generator=g).to(BF16), torch.randn(B * N, C, device="cuda", generator=g).to(BF16)
        O, L, out = torch.zeros(B * N, C, dtype=BF16, device="cuda"), torch.zeros(B * H * N, dtype=F32, device="cuda"), torch.zeros(B * N, C, dtype=BF16, device="cuda")
        z = lambda n, dt=I32: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        dst, nmax, nidx, tmap, kept, offs, lst, ctr = z(Nd), z(B * Ns, F32), z(B * Ns), z(B * N), z(B * Np), z(B * (Nd + 1)), z(B * r), z(2)
        ym, a = torch.zeros(B * Np, C, dtype=BF16, device="cuda"), torch.randn(B * Np, C, device="cuda", generator=g).to(BF16)
        full = lambda n: ops.attn_fwd(qkv[:B * n, :C], qkv[:B * n, C:2 * C], qkv[:B * n, 2 * C:], None, O[:B * n], L[:B * H * n], B=B, H=H, Nq=n, Nk=n, Nqp=n, Nkp=n, d=d, scale=0.125)  # noqa: E731
        kinds = {"sdlt_attn_fwd, full grid (plain)": lambda: full(N),
                 "sdlt_tome_match": lambda: ops.tome_match(y, dst, nmax, nidx, B=B, grid=grid, mode="random", seed=1, ctr=ctr, layer=0),
                 "sdlt_tome_plan": lambda: ops.tome_plan(nmax, nidx, dst, tmap, kept, offs, lst, B=B, grid=grid, r=r),
                 "sdlt_tome_merge": lambda: ops.tome_merge(y, dst, kept, offs, lst, ym, B=B, grid=grid, r=r),
                 "sdlt_tome_unmerge": lambda: ops.tome_unmerge(res, a, tmap, out, B=B, N=N, Np=Np),
                 f"sdlt_attn_fwd, {Np} merged rows": lambda: full(Np)}
        times, graphs = {k_: [] for k_ in kinds}, {}
        for k_, fn in kinds.items():                        # one eager call each (it also leaves valid tables for the launches that read them), then the capture
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
            lines.append(f"{side:>4} x {side:<3} x {C:<4} {name:<44} {statistics.median(ts):>11.1f} {min(ts):>10.1f} {max(ts):>10.1f}")
        med = {k_: statistics.median(t) for k_, t in times.items()}
        tome = sum(v for k_, v in med.items() if "plain" not in k_)
        lines.append(f"{side:>4} x {side:<3} x {C:<4} {'sum of the five token-merging launches / plain':<44} {tome / med['sdlt_attn_fwd, full grid (plain)']:>11.3f}")
    return lines


def iteration_times(version, h, steps, repeats, ratio=0.5, rank=16):
    import render_bench as RB
    cfg, smp = RB.build(version, 1, rank)
    em = RB.embeds(cfg, 1)
    noise = torch.randn(1, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    variants = {"plain": {}, f"tome {ratio}": dict(token_merge=dict(ratio=ratio)), f"tome {ratio} depth 1": dict(token_merge=dict(ratio=ratio, depth=1))}
    times = {k: [] for k in variants}
    for rnd in range(repeats + 1):                          # round 0: warm-up (buffers, packed weights, the captures)
        for k, kw in variants.items():
            t = RB.timed(lambda: smp.sample(em[0], h, h, steps=steps, latents=noise, graph=True, **kw)) * 1e3 / steps
            if rnd:
                times[k].append(t)
    lines = [f"# (ii) {version} topology, {h} x {h} latent ({8 * h} px), batch 2, rank {rank}, {steps}-step graph samples, mode random; wall ms per iteration: "
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
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, nargs="+", default=[128, 256])
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
