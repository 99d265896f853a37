"""What extracting SDXL's adapted layer set (577 layers, bf16) costs, two ways in ONE session, alternated so that clocks and neighbours hit
both alike: (a) extract.extract_adapters - 2 q + 2 sdlt_delta_matmul launches for the whole model plus the batched fp64 torch.linalg steps;
(b) the per-layer loop a torch user would write: D = W1 - W0 materialised in fp32, torch.svd_lowrank(D, q = rank + oversample, niter = q).
Synthetic weights: tuned = base + a seeded perturbation with a geometrically decaying spectrum (U diag(0.05 * 0.9^i) V^T over 64 components).
Also the kernel alone: the forward and the transposed launch at the run's column count, 10 back-to-back launches between two stream events
per round, with the bytes a launch must read and its flops.

    python tools/extract_bench.py [--out FILE] [--rounds 3] [--ranks 16 128] [--power-iters 2]

Prints one table: wall seconds per extraction (median over the rounds, min .. max) and the launch times in milliseconds.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launch_ms(fn, reps=10, rounds=5):
    """Milliseconds per launch: `reps` back-to-back launches between two stream events, per round."""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def model_pair(targets, shapes, comps=64):
    g = torch.Generator(device="cuda").manual_seed(0)
    base, tuned = {}, {}
    sig = 0.05 * 0.9 ** torch.arange(comps, device="cuda", dtype=torch.float32)
    for n in targets:
        s = shapes[n + ".weight"]
        N, K = s[0], int(torch.tensor(s[1:]).prod())
        w = torch.randn(N, K, generator=g, device="cuda") * 0.02
        U = torch.linalg.qr(torch.randn(N, comps, generator=g, device="cuda"))[0]
        V = torch.linalg.qr(torch.randn(K, comps, generator=g, device="cuda"))[0]
        base[n + ".weight"] = w.to(torch.bfloat16).view(s)
        tuned[n + ".weight"] = (w + (U * sig) @ V.t()).to(torch.bfloat16).view(s)
    return base, tuned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--power-iters", type=int, default=2)
    a = ap.parse_args()
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import extract as X
    from sd_lora_trainer_amd import ops, topology
    cfg = topology.CONFIGS["sdxl"]
    shapes, targets = topology.param_shapes(cfg), topology.lora_targets(cfg)
    base, tuned = model_pair(targets, shapes)
    rt = M.Runtime("cuda:0", 1)
    elems = sum(v.numel() for v in base.values())
    lines = [f"SDXL adapted layers: {len(targets)}, {elems / 1e9:.3f} G weights, {4 * elems / 1e9:.2f} GB read per product (bf16 base + tuned); "
             f"power iterations {a.power_iters}, rounds {a.rounds}", ""]
    for rank in a.ranks:
        L = X.padded_columns(rank, 16)

        def ours():
            X.extract_adapters(base, tuned, rank, power_iters=a.power_iters, runtime=rt, targets=targets)

        def loop():
            for n in targets:
                D = X.weight_view(tuned[n + ".weight"], "cuda").float() - X.weight_view(base[n + ".weight"], "cuda").float()
                U, S, V = torch.svd_lowrank(D, q=min(L, *D.shape), niter=a.power_iters)
                rs = S[:rank].sqrt()
                _ = (U[:, :rank] * rs, rs.unsqueeze(1) * V[:, :rank].t())
        ours(), loop()                                   # warm-up: allocator, solver handles, code objects
        t_ours, t_loop = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours))
            t_loop.append(timed(loop))
        # the kernel alone
        W0 = [X.weight_view(base[n + ".weight"], "cuda") for n in targets]
        W1 = [X.weight_view(tuned[n + ".weight"], "cuda") for n in targets]
        layers = [dict(W0=w0, W1=w1, Pk=torch.randn(w0.shape[1], L, device="cuda"), Pn=torch.zeros(w0.shape[0], L, device="cuda")) for w0, w1 in zip(W0, W1)]
        plan = ops.DeltaPlan(layers, L, torch.device("cuda"))
        plan.forward(), plan.transposed()
        k_f, k_t = launch_ms(plan.forward), launch_ms(plan.transposed)
        del plan, layers
        flops = 2.0 * elems * L
        fmt = lambda t: f"{statistics.median(t):8.3f} s ({min(t):.3f} .. {max(t):.3f})"  # noqa: E731
        lines += [f"rank {rank} (L = {L})",
                  f"  extract_adapters (batched, sdlt_delta_matmul) {fmt(t_ours)}",
                  f"  per-layer torch.svd_lowrank loop              {fmt(t_loop)}"]
        for name, t in (("forward   ", k_f), ("transposed", k_t)):
            m = statistics.median(t) * 1e-3
            lines.append(f"  one {name} launch  {m * 1e3:8.2f} ms ({min(t):.2f} .. {max(t):.2f})   {4 * elems / m / 1e12:.2f} TB/s of weights, {flops / m / 1e12:.1f} TFLOP/s")
        lines.append("")
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
