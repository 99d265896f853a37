"""What attention couple costs, in ONE session with the variants alternating:
(i) the kernel: sdlt_attn_couple_fwd at R = 1 against sdlt_attn_fwd on SDXL's two cross-attention shapes (N = 4096 with 10 heads, N = 1024 with 20 heads; d = 64,
    77 keys in 128 rows, batch 2), and at R = 3 with box masks as three vertical bands ("cols": a 64-query tile is a run of a token ROW and crosses all
    three, so no region is skipped), as three horizontal bands ("rows": a tile lies in one band, or two at a boundary, and skips the others) and with soft masks
    (every region has weight everywhere) - device events around `launches` back-to-back launches, median (min .. max) of `repeats` rounds after a warm-up;
(ii) one replayed SDXL iteration (random weights, rank-16 adapters, --latent 128 = 1024 px): plain at batch 2, couple at R = 3 (batch 2), fuse at R = 3 (batch 6) -
    wall ms per iteration of `steps`-step graph samples, median (min .. max) of `repeats` rounds after a warm-up.

    python tools/attn_couple_bench.py [--out profiles/attention_couple_render_bench.txt] [--repeats 3] [--latent 128] [--steps 10] [--kernel-only]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16, F32 = torch.bfloat16, torch.float32


def masks3(side, soft, rows=False):
    """Normalised weights fp32 [3, side * side]: three bands - vertical, or horizontal with `rows` - hard (box) or blended by wide sigmoids (soft: every region
    non-zero everywhere)."""
    x = torch.arange(side, dtype=F32)[None, :].expand(side, side) / side
    x = x.t() if rows else x
    if soft:
        raw = torch.stack([torch.sigmoid((1 / 3 - x) * 6) + 0.05, torch.exp(-((x - 0.5) * 3) ** 2) + 0.05, torch.sigmoid((x - 2 / 3) * 6) + 0.05])
    else:
        raw = torch.stack([(x < 1 / 3).float(), ((x >= 1 / 3) & (x < 2 / 3)).float(), (x >= 2 / 3).float()])
    return (raw / raw.sum(0, keepdim=True)).reshape(3, side * side).contiguous().cuda()


def kernel_times(launches, repeats):
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    lines = [f"# (i) device-event us per launch, B = 2, d = 64, Nk = 77 (Nkp = 128), {launches} launches back to back: median (min .. max) of {repeats} rounds, alternated",
             f"{'N':>5} {'H':>3} {'variant':<36} {'us / launch':>12} {'min':>9} {'max':>9}"]
    for N, H in ((4096, 10), (1024, 20)):
        B, d, Nk, Nkp, C, side = 2, 64, 77, 128, H * 64, int(math.isqrt(N))
        mk = lambda rows: torch.randn(rows, C, device="cuda", generator=g).to(BF16)  # noqa: E731
        q, O, L = mk(B * N), torch.zeros(B * N, C, dtype=BF16, device="cuda"), torch.zeros(B * H * N, dtype=F32, device="cuda")
        k1, v1, k3, v3 = mk(B * Nkp), mk(B * Nkp), mk(B * 3 * Nkp), mk(B * 3 * Nkp)
        one, box, rowbox, soft = torch.ones(1, N, device="cuda"), masks3(side, False), masks3(side, False, rows=True), masks3(side, True)
        kw = dict(B=B, H=H, Nk=Nk, Nkp=Nkp, d=d, scale=0.125)
        kinds = {"sdlt_attn_fwd": lambda: ops.attn_fwd(q, k1, v1, None, O, L, Nq=N, Nqp=N, **kw),
                 "sdlt_attn_couple_fwd R = 1": lambda: ops.attn_couple_fwd(q, k1, v1, O, one, Nq=N, R=1, **kw),
                 "sdlt_attn_couple_fwd R = 3, box cols": lambda: ops.attn_couple_fwd(q, k3, v3, O, box, Nq=N, R=3, **kw),
                 "sdlt_attn_couple_fwd R = 3, box rows": lambda: ops.attn_couple_fwd(q, k3, v3, O, rowbox, Nq=N, R=3, **kw),
                 "sdlt_attn_couple_fwd R = 3, soft": lambda: ops.attn_couple_fwd(q, k3, v3, O, soft, Nq=N, R=3, **kw)}
        times = {k: [] for k in kinds}
        for r in range(repeats + 1):                        # round 0: warm-up
            for k, fn in kinds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
        for k, t in times.items():
            lines.append(f"{N:>5} {H:>3} {k:<36} {statistics.median(t):>12.2f} {min(t):>9.2f} {max(t):>9.2f}")
    return lines


def iteration_times(version, h, steps, repeats, rank=16):
    import render_bench as RB
    cfg, smp2 = RB.build(version, 1, rank)                  # batch 2: plain and couple
    _, smp6 = build6(version, rank)                         # batch 2 R = 6: fuse; the same seeds, so the same weights and adapters
    em = RB.embeds(cfg, 3)
    noise = torch.randn(1, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    x = torch.arange(h, dtype=F32)[None, :].expand(h, h) / h
    fg = torch.stack([((x >= 1 / 3) & (x < 2 / 3)).float(), (x >= 2 / 3).float()])      # two foreground boxes; the main prompt keeps the left third
    rg = lambda mode: dict(masks=fg, embeds=em[1:], mode=mode)  # noqa: E731
    variants = {"plain, batch 2": lambda: smp2.sample(em[0], h, h, steps=steps, latents=noise, graph=True),
                "couple R = 3, batch 2": lambda: smp2.sample(em[0], h, h, steps=steps, latents=noise, graph=True, regions=rg("couple")),
                "fuse R = 3, batch 6": lambda: smp6.sample(em[0], h, h, steps=steps, latents=noise, graph=True, regions=rg("fuse"), seeds=[1])}
    times = {k: [] for k in variants}
    for r in range(repeats + 1):                            # round 0: warm-up (buffers, packed weights, the captures)
        for k, fn in variants.items():
            t = RB.timed(fn) * 1e3 / steps
            if r:
                times[k].append(t)
    lines = [f"# (ii) {version} topology, {h} x {h} latent, rank {rank}, {steps}-step graph samples; wall ms per iteration: median (min .. max) of {repeats} rounds, alternated",
             f"{'variant':<28} {'ms / iteration':>16} {'min':>9} {'max':>9} {'/ plain':>9}"]
    base = statistics.median(times["plain, batch 2"])
    for k, t in times.items():
        lines.append(f"{k:<28} {statistics.median(t):>16.3f} {min(t):>9.3f} {max(t):>9.3f} {statistics.median(t) / base:>9.3f}")
    return lines


def build6(version, rank):
    """render_bench.build on a runtime of batch 2 R = 6 with one image: the fuse mode's sampler."""
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import sampler, topology
    from sd_lora_trainer_amd.train import _random_state
    cfg = topology.CONFIGS[version]
    rt = M.Runtime("cuda:0", 6)
    unet = M.UNet(rt, cfg, _random_state(topology.param_shapes(cfg), "cuda:0", seed=0), lora_rank=rank)
    g = torch.Generator(device="cuda").manual_seed(1)
    for e in unet.arena.entries:
        e["A"].copy_(torch.randn(e["A"].shape, generator=g, device="cuda") / rank)
        e["B"].copy_(torch.randn(e["B"].shape, generator=g, device="cuda") * 0.02)
    unet.arena.refresh_shadows()
    smp = sampler.LatentSampler(rt, unet, n_images=1)
    smp.set_lora_scale(0.75)
    return cfg, smp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
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
