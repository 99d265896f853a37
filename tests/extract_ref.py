"""fp64 restatement of the adapter extraction (sd_lora_trainer_amd.extract), the torch emulation of ops.DeltaPlan for the CPU tests, and the
bounds the extraction tests apply.  Written from the algorithm (Halko, Martinsson, Tropp 2011: algorithm 4.4, the randomized subspace
iteration, followed by algorithm 5.1, the SVD through the small factor), one layer at a time, everything in fp64.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u), Higham 2002 section 3.1):
 * a product Y = D X of the kernel: |Y - Y64| <= gamma_R |D| |X| element-wise, R the reduction length (R products and sums in any order),
   for a bf16 / bf16 or fp16 / fp16 pair, whose fp32 difference is exact; gamma_{R+1} for fp32 and mixed pairs, whose difference rounds once.
 * the extracted product P = B'A' of the fp32 pipeline against the fp64 restatement on the same D and Omega, in the Frobenius norm, to
   first order in u:  with Q = orth(D Q' + E), |E| <= gamma_{K+1} |D| |Q'|, and Q' an orthonormal basis that holds D's dominant row
   space, the part of that space's image that Q misses is at most ||E||_F <= gamma_{K+1} sqrt(L) ||D||_F (every column of |Q'| has norm 1);
   C = D^T Q + E_C with ||E_C||_F <= gamma_{N+1} sqrt(L) ||D||_F and Q C^T carries it unamplified (||Q||_2 = 1); Q enters the kernel
   rounded to fp32: 2 u sqrt(L) ||D||_F; and the fp32 rounding of the two factors: 2 u || |B'| |A'| ||_F.  Sum:
       fp32_bound = (gamma_{K+1} + gamma_{N+1} + 2 u) sqrt(L) ||D||_F + 2 u || |B'| |A'| ||_F
 * Halko-Martinsson-Tropp corollary 10.10 (power scheme, expected spectral error of the (k + p)-column basis) with theorem 9.3 (truncation
   to rank k adds sigma_{k+1}):
       E ||D - P_k||_2 <= sigma_{k+1} + [(1 + sqrt(k / (p - 1))) sigma_{k+1}^(2q+1) + e sqrt(k + p) / p (sum_{j>k} sigma_j^(2(2q+1)))^(1/2)]^(1/(2q+1))
"""
import math
import types

import torch

from tests import emu_ops

U32 = 2.0 ** -24
F64 = torch.float64


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def delta64(W0, W1):
    """What the kernel multiplies with, exactly: the fp32 difference of the two operands (exact for bf16 / fp16 pairs), as fp64."""
    return (W1.float() - W0.float()).double()


def product_bound(W0, W1, X, transposed):
    """-> (fp64 product of the exact difference, element-wise bound gamma_R |D| |X|; gamma_{R+1} where the fp32 difference rounds)."""
    exact = W0.dtype == W1.dtype and W0.dtype in (torch.bfloat16, torch.float16)
    D = W1.double() - W0.double()
    if transposed:
        D = D.t()
    R = D.shape[1]
    return D @ X.double(), gamma(R if exact else R + 1) * (D.abs() @ X.double().abs())


def orth64(Y):
    return torch.linalg.qr(Y, mode="reduced")[0]


def extract_ref(D, omega, rank, power_iters):
    """One layer in fp64: D [N, K], omega [K, L] -> (A [rank, K], B [N, rank], sigma [min(L, N, K)])."""
    D, omega = D.to(F64), omega.to(F64)
    Q = orth64(D @ omega)
    for _ in range(power_iters):
        Qp = orth64(D.t() @ Q)
        Q = orth64(D @ Qp)
    C = D.t() @ Q                       # [K, L'];  D ~ Q C^T
    Uc, S, Vct = torch.linalg.svd(C.t(), full_matrices=False)
    U = Q @ Uc
    r = min(rank, S.numel())
    rs = S[:r].sqrt()
    B = torch.zeros(D.shape[0], rank, dtype=F64)
    A = torch.zeros(rank, D.shape[1], dtype=F64)
    B[:, :r] = U[:, :r] * rs
    A[:r] = rs.unsqueeze(1) * Vct[:r]
    return A, B, S


def fp32_bound(D, L, A, B):
    """Frobenius-norm allowance of the fp32 pipeline over the restatement (module docstring)."""
    N, K = D.shape
    return (gamma(K + 1) + gamma(N + 1) + 2 * U32) * math.sqrt(L) * float(D.norm()) + 2 * U32 * float((B.double().abs() @ A.double().abs()).norm())


def hmt_bound(sigma, k, p, q):
    """Expected spectral-norm error of the rank-k truncation of the power scheme's approximation (module docstring); sigma: the full spectrum."""
    s = sigma.double()
    e = 2 * q + 1
    tail = float((s[k:] ** (2 * e)).sum().sqrt())
    inner = (1 + math.sqrt(k / (p - 1))) * float(s[k]) ** e + math.e * math.sqrt(k + p) / p * tail
    return float(s[k]) + inner ** (1.0 / e)


def spectrum_delta(N, K, decay, seed, scale=0.05):
    """-> (D fp64 [N, K] = U diag(sigma) V^T with sigma_i = scale * decay^i and seeded orthonormal U, V; sigma)."""
    g = torch.Generator().manual_seed(seed)
    n = min(N, K)
    U = orth64(torch.randn(N, n, generator=g, dtype=F64))
    V = orth64(torch.randn(K, n, generator=g, dtype=F64))
    sigma = scale * decay ** torch.arange(n, dtype=F64)
    return (U * sigma) @ V.t(), sigma


class EmuDeltaPlan:
    """torch emulation of ops.DeltaPlan: the fp32 difference times the fp32 panel, one fp32 matmul per layer."""
    launches = []

    def __init__(self, layers, L, device):
        self.layers, self.L = layers, L

    def forward(self):
        EmuDeltaPlan.launches.append("forward")
        for l in self.layers:
            D = l["W1"].float() - l["W0"].float()
            l["Pn"].copy_(D @ l["Pk"])
            if l.get("rowsq") is not None:
                l["rowsq"].copy_((D * D).sum(1))

    def transposed(self):
        EmuDeltaPlan.launches.append("transposed")
        for l in self.layers:
            l["Pk"].copy_((l["W1"].float() - l["W0"].float()).t() @ l["Pn"])


def emu_ops_with_delta(base=None):
    """The emulated op table plus MergePlan (tests/test_merge_cpu.py) and DeltaPlan."""
    from tests.test_merge_cpu import EmuMergePlan
    src = base if base is not None else emu_ops
    ns = types.SimpleNamespace(**{k: getattr(src, k) for k in dir(src) if not k.startswith("__")})
    ns.MergePlan = EmuMergePlan
    ns.DeltaPlan = EmuDeltaPlan
    return ns


# layers of the synthetic extraction cases: name -> weight shape (two linears, a ragged one, a 3x3 conv)
CASE_SHAPES = {"a.to_q": (320, 320), "a.to_k": (320, 320), "b.to_out.0": (200, 456), "c.conv2": (256, 32, 3, 3)}


def case_base(seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return {n + ".weight": (torch.randn(s, generator=g) * 0.02).to(dtype) for n, s in CASE_SHAPES.items()}


def case_lora(rank, seed):
    """Seeded adapters in peft layout: A ~ N(0, 1 / r^2)... scaled so that B A is of the order of a trained update (std 0.05 rows)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, s in CASE_SHAPES.items():
        if len(s) == 4:
            out[n] = (torch.randn(rank, s[1], 3, 3, generator=g) / rank, torch.randn(s[0], rank, 1, 1, generator=g) * 0.05)
        else:
            out[n] = (torch.randn(rank, s[1], generator=g) / rank, torch.randn(s[0], rank, generator=g) * 0.05)
    return out


def view2d(w):
    """[N, K] view of a weight / a peft factor, tap-major for 3x3 convs (the arena's layout)."""
    if w.dim() == 4 and w.shape[-1] == 3:
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return w.reshape(w.shape[0], -1)


def product2d(A, B):
    """B A of a peft-layout pair as fp64 [N, K] in the arena's layout."""
    return view2d(B).double() @ view2d(A).double()


def check_recovery(ex, base, tuned, lora, rank, L, omegas_by_name, power_iters, what):
    """Check 2: per layer, ||B'A' - BA||_F <= (the restatement's deviation on the same fp32 difference and Omega) + fp32_bound."""
    worst = 0.0
    for n, (A, B) in lora.items():
        D = delta64(view2d(base[n + ".weight"]), view2d(tuned[n + ".weight"]))
        BA = product2d(A, B)
        Ar, Br, _ = extract_ref(D, omegas_by_name[n], rank, power_iters)
        dev_ref = float((Br @ Ar - BA).norm())
        A2, B2 = ex.lora[n]
        dev = float((product2d(A2, B2) - BA).norm())
        allow = dev_ref + fp32_bound(D, L, view2d(A2), view2d(B2))
        print(f"{what} {n}: deviation {dev:.3e}, restatement {dev_ref:.3e}, allowance {allow:.3e}, ||BA|| {float(BA.norm()):.3e}")
        assert dev <= allow, f"{what} {n}: ||B'A' - BA||_F = {dev:.3e} > {allow:.3e} (restatement {dev_ref:.3e})"
        worst = max(worst, dev / allow)
    return worst


def omegas_by_name(names, shapes2d, L, seed):
    from sd_lora_trainer_amd import extract as X
    om = X.draw_omega(shapes2d, L, seed)
    out = {}
    for g, (_, idx) in enumerate(X.shape_groups(shapes2d)):
        for j, i in enumerate(idx):
            out[names[i]] = om[g][j]
    return out


def predict(unet, rt, cfg, x, t, ctx, pooled, tid, h):
    """One UNet prediction [1, 4, h, h] (fp32, CPU) on either device - tests/test_merge_gpu.py's _predict without the CUDA-only synchronize."""
    import sd_lora_trainer_amd.unet as M
    dev = rt.device
    x64 = rt.zeros(h * h, 64)
    x64[:, :4] = x.permute(0, 2, 3, 1).reshape(h * h, 4).to(dev, x64.dtype)
    cb = rt.zeros(M.CTX_PAD, cfg["cross_dim"])
    cb[:77] = ctx[0].to(dev, cb.dtype)
    pb = pooled.to(dev, rt.act) if pooled is not None else None
    tb = tid.reshape(-1).to(dev, torch.float32) if tid is not None else None
    with torch.no_grad():
        eps = unet.forward(x64, torch.tensor([float(t)], device=dev), cb, pb, tb, B=1, H=h, W=h)
    return eps.float().view(1, h, h, 4).permute(0, 3, 1, 2).cpu()
