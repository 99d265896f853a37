"""The VAE's mid-block attention alone (one head, d = 512, B = 1): the one-pass kernel (ops.attn_wide_fwd) against the dense sequence it replaces (the V^T
side output aside: score GEMM into fp32 [N, N], torch.softmax + cast into bf16 [N, N], second GEMM), alternating in one process, by device events.
python tools/attn_wide_probe.py [N ...]   (default 4096 16384)"""
import math
import sys

import torch

sys.path.insert(0, ".")
from sd_lora_trainer_amd import ops      # noqa: E402

d = 512
for N in [int(v) for v in sys.argv[1:]] or [4096, 16384]:
    g = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(N, d, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    vt = v.t().contiguous()
    S, P = torch.empty(N, N, dtype=torch.float32, device="cuda"), torch.empty(N, N, dtype=torch.bfloat16, device="cuda")
    Of, Od = torch.empty(N, d, dtype=torch.bfloat16, device="cuda"), torch.empty(N, d, dtype=torch.bfloat16, device="cuda")
    scale = 1.0 / math.sqrt(d)

    def flash():
        ops.attn_wide_fwd(q, k, v, Of, B=1, Nq=N, Nk=N, scale=scale)

    def dense():
        ops.gemm(q, k, S, alpha=scale)
        P.copy_(torch.softmax(S, dim=-1))
        ops.gemm(P, vt, Od)

    def timed(fn, reps=5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for fn in (flash, dense, flash, dense):      # warm-up
        fn()
    torch.cuda.synchronize()
    res = {"flash": [], "dense": []}
    for _ in range(3):                           # three alternating repeats: the spread
        res["flash"].append(timed(flash))
        res["dense"].append(timed(dense))
    diff = float((Of.float() - Od.float()).abs().max())
    for name, ms in res.items():
        print(f"N={N} {name}: {min(ms):.3f} ms (repeats {' '.join(f'{m:.3f}' for m in ms)}), {4.0 * N * N * d / (min(ms) * 1e-3) / 1e12:.1f} TFLOP/s of 4 N^2 d")
    print(f"N={N} max |flash - dense| = {diff:.3e}")
    del S, P
    torch.cuda.empty_cache()
