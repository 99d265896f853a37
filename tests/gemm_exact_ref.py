"""Exact-arithmetic reference of the linear products (sdlt_gemm_bf16 mode 0, every option of it that is linear), of the adapter gradients
(sdlt_lora_grad_grouped / _wide) and of the weight-gradient chain, with the small-integer operands that make them exact.  Plain torch in fp64
on the CPU; imports nothing from the project (tests/conv_exact_ref.py supplies `rounded`, the operand ranges and the 3 x 3 gather).

The contract restated (ops.gemm docstring, include/sdlt_kernels.h):

  out = alpha * col_scale[n] * (X W^T + X2 W2^T + Tb Bup^T) + bias[n] + rowbias[m // rows_per_batch, n] + residual[m, n]      (+ out, `accumulate`, fp32)

  * Tb = bf16(s * X Adown^T), which is also T_out.
  * lora_group_n = w:  output column n uses adapter group g = n // w: Adown rows [g Rp, (g+1) Rp), T_out columns [g Rp, (g+1) Rp); Bup [N, Rp].
  * lora_group_k = C:  group g reads X columns [g C, (g+1) C) against the same columns of Adown [Rp, K]: T_out [M, G Rp]; Bup [N, G Rp].
  * x2_group_n = w:    output column n reads X2 columns [g K2, (g+1) K2), g = n // w; W2 [N, K2].
  * Ct[n][m] = bf16(out[m][n]).

Adapter gradients:  out[c][r]  or (rank_major)  out[r][c]  (+)=  sum_m P[m][c] Q[m][r],  r < R;  conv form: P's rows gathered by the forward 3 x 3
geometry (k = tap * Cin + ci), taken from conv_exact_ref.conv9 by convolving with the identity.

With X, X2 in {-2..2}, W / W2 / Bup in {-1, 0, 1}, at most three +-1 per Adown row (per K group where K is grouped), s = 0.5, alpha in {0.5, 2},
col_scale in {0.5, 1, 2} and small-integer bias / row bias / residual / previous contents, every partial sum is a multiple of 0.25 far below 2^24:
an fp32 result does not depend on the summation order, tile, K split or ring depth and equals the fp64 one bit for bit (alpha = 0.5 goes with
integer products, alpha = 2 with the adapter's halves: tests/test_gemm_exact_cpu.py asserts the grid).
"""
import functools

import torch

from tests.conv_exact_ref import BF, F32, F64, K2, LORA_SCALE, Geom, conv9, rounded  # noqa: F401  (re-exported)

N_PLAIN = 200
MS = (105, 280)                       # ragged against the 64-, 128- and 256-row tiles
KS = (64, 192, 576)                   # one, three and nine K steps
PADS = (16, 32, 64)
NB = 3                                # row-bias rows (rows_per_batch = ceil(M / 3)); problems of a batched launch
GROUP_W = {1: 128, 2: 128, 3: 64, 8: 160}     # the smallest lora_group_n / x2_group_n a tile takes


# ---------------------------------------------------------------------------------------------------------------- the product
def gemm_ref(X, W, *, X2=None, W2=None, x2_group_n=0, lora=None, lora_group_n=0, lora_group_k=0, col_scale=None, bias=None, rowbias=None,
             rows_per_batch=0, residual=None, alpha=1.0):
    """-> (fp64 result [M, N] before the output rounding and before `accumulate`, T_out bf16 or None).  lora = (Adown, Bup, scale)."""
    x, w = X.to(F64), W.to(F64)
    M, N = x.shape[0], w.shape[0]
    acc = x @ w.t()
    if X2 is not None:
        x2, w2 = X2.to(F64), W2.to(F64)
        k2 = w2.shape[1]
        if x2_group_n:
            for g in range(N // x2_group_n):
                cols = slice(g * x2_group_n, (g + 1) * x2_group_n)
                acc[:, cols] += x2[:, g * k2:(g + 1) * k2] @ w2[cols].t()
        else:
            acc = acc + x2 @ w2.t()
    T_out = None
    if lora is not None:
        Adown, Bup, scale = lora[:3]
        a, bu = Adown.to(F64), Bup.to(F64)
        if lora_group_k:
            C = lora_group_k
            T = torch.cat([x[:, g * C:(g + 1) * C] @ a[:, g * C:(g + 1) * C].t() for g in range(x.shape[1] // C)], 1)
        else:
            T = x @ a.t()
        T_out = (T * scale).to(F32).to(BF)                               # the contract rounds s*T to bf16 here
        t = T_out.to(F64)
        if lora_group_n:
            Rp = bu.shape[1]
            for g in range(N // lora_group_n):
                cols = slice(g * lora_group_n, (g + 1) * lora_group_n)
                acc[:, cols] += t[:, g * Rp:(g + 1) * Rp] @ bu[cols].t()
        else:
            acc = acc + t @ bu.t()
    acc = acc * alpha
    if col_scale is not None:
        acc = acc * col_scale.to(F64)[None, :]
    if bias is not None:
        acc = acc + bias.to(F64)[None, :]
    if rowbias is not None:
        acc = acc + rowbias.to(F64)[torch.arange(M) // rows_per_batch]
    if residual is not None:
        acc = acc + residual.to(F64)
    return acc, T_out


# ---------------------------------------------------------------------------------------------------------------- operands
def _ints(g, lo, hi, *shape, dtype=BF):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def _sparse_rows(g, rows, K, C):
    """[rows, K] with three +-1 per row inside every group of C columns (C = K: three per row): |X A^T| <= 6 per group."""
    A = torch.zeros(rows, K, dtype=BF)
    for k0 in range(0, K, C):
        cols = k0 + torch.randint(0, C, (rows, 3), generator=g)
        A[torch.arange(rows)[:, None], cols] = (torch.randint(0, 2, (rows, 3), generator=g) * 2 - 1).to(BF)
    return A


@functools.lru_cache(maxsize=None)
def operands(M, N, K, idx=0, gk=0):
    """Everything a case can use, from one seeded generator.  Adown has 3 x 64 rows (three groups of rank pad 64; smaller pads and fewer groups use the
    first rows), Bup 4 x 64 columns; gk > 0: Adown's entries are placed per K group of gk columns.  idx: the problem of a batched launch."""
    g = torch.Generator().manual_seed(7000 + 131 * M + 17 * N + K + 7919 * idx + 3 * gk)
    d = dict(M=M, N=N, K=K, rows_per_batch=-(-M // NB))
    d["X"] = _ints(g, -2, 2, M, K)
    d["W"] = _ints(g, -1, 1, N, K)
    d["bias"] = _ints(g, -4, 4, N, dtype=F32)
    d["rowbias"] = _ints(g, -3, 3, NB, N)
    d["residual"] = _ints(g, -8, 8, M, N)
    d["start"] = _ints(g, -16, 16, M, N, dtype=F32)                      # what an fp32 output holds before an `accumulate` launch
    d["Adown"] = _sparse_rows(g, 3 * 64, K, gk or K)
    d["Bup"] = _ints(g, -1, 1, N, 4 * 64)
    d["col_scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    d["X2"] = _ints(g, -2, 2, M, 3 * K2)
    d["W2"] = _ints(g, -1, 1, N, K2)
    return d


def _variants():
    full = dict(bias=1, rowbias=1, residual=1)
    v = {"plain": dict(), "bias": dict(bias=1), "full": dict(alpha=0.5, **full), "seg2": dict(seg2=1), "lora16full": dict(pad=16, cs=1, alpha=2.0, **full)}
    for p in PADS:
        v[f"lora{p}"] = dict(pad=p)
        v[f"lora{p}cs"] = dict(pad=p, cs=1, alpha=2.0)
        for w in (64, 128, 160):
            v[f"gn{p}w{w}"] = dict(pad=p, gn=w, bias=1)
        for c in (64, 192):
            v[f"gk{p}c{c}"] = dict(pad=p, gk=c, residual=1)
        v[f"gkb{p}c64"] = dict(pad=p, gk=64)                          # batched launches: the residual is launch-wide, so none
    for w in (64, 128):
        v[f"x2g{w}"] = dict(seg2=1, x2g=w)
    return v


VARIANTS = _variants()


def variant_gk(variant):
    return VARIANTS[variant].get("gk", 0)


def variant_kwargs(d, v, T_out=None, four=True):
    """gemm() keyword arguments of a variant from an operand set (CPU tensors, or the same dict moved to a device)."""
    kw = {}
    pad = v.get("pad", 0)
    if pad:
        if v.get("gk"):
            G = d["K"] // v["gk"]
            A, Bu, kw["lora_group_k"] = d["Adown"][:pad], d["Bup"][:, :G * pad], v["gk"]
        elif v.get("gn"):
            G = d["N"] // v["gn"]
            A, Bu, kw["lora_group_n"] = d["Adown"][:G * pad], d["Bup"][:, :pad], v["gn"]
        else:
            A, Bu = d["Adown"][:pad], d["Bup"][:, :pad]
        kw["lora"] = (A, Bu, LORA_SCALE) + ((T_out,) if four else ())
    if v.get("cs"):
        kw["col_scale"] = d["col_scale"]
    if v.get("alpha"):
        kw["alpha"] = v["alpha"]
    if v.get("bias"):
        kw["bias"] = d["bias"]
    if v.get("rowbias"):
        kw["rowbias"], kw["rows_per_batch"] = d["rowbias"], d["rows_per_batch"]
    if v.get("residual"):
        kw["residual"] = d["residual"]
    if v.get("seg2"):
        G2 = d["N"] // v["x2g"] if v.get("x2g") else 1
        kw["X2"], kw["W2"] = d["X2"][:, :G2 * K2], d["W2"]
        if v.get("x2g"):
            kw["x2_group_n"] = v["x2g"]
    return kw


def t_width(d, v):
    """Columns of T_out: the rank pad times the number of adapter groups."""
    pad = v.get("pad", 0)
    return pad * (d["K"] // v["gk"] if v.get("gk") else (d["N"] // v["gn"] if v.get("gn") else 1))


@functools.lru_cache(maxsize=None)
def reference(M, N, K, variant, idx=0):
    """(fp64 result, T_out) of a case; computed once, shared by every test that needs it, never modified."""
    d = operands(M, N, K, idx, variant_gk(variant))
    return gemm_ref(d["X"], d["W"], **variant_kwargs(d, VARIANTS[variant], four=False))


# the cases of tests/test_gemm_exact_gpu.py, (M, N, K, variant, idx): the GPU file runs nothing that is not listed here, the CPU file checks them all
MK = [(M, K) for M in MS for K in KS]
PLAIN_CASES = [(M, N_PLAIN, K, v, 0) for (M, K) in MK for v in ("plain", "full")] + [(1, N_PLAIN, 192, v, 0) for v in ("plain", "full")]
ADAPTER_CASES = ([(M, N_PLAIN, K, f"lora{p}{cs}", 0) for M in MS for K in (192, 576) for p in PADS for cs in ("", "cs")]
                 + [(M, N_PLAIN, 192, "lora16full", 0) for M in MS])
GROUP_N_CASES = [(M, G * w, 192, f"gn{p}w{w}", 0) for M in MS for G in (2, 3) for w in (64, 128, 160) for p in PADS if not (w == 160 and p > 16)]
GROUP_K_CASES = ([(M, N_PLAIN, G * 64, f"gk{p}c64", 0) for M in MS for G in (2, 3, 4) for p in PADS]
                 + [(M, N_PLAIN, 576, "gk16c192", 0) for M in MS])
BATCH_CASES = ([(105, N_PLAIN, 192, "bias", i) for i in range(NB)]
               + [(105, 2 * w, 192, f"gn{p}w{w}", i) for w in (64, 128) for p in PADS for i in range(NB)]
               + [(105, N_PLAIN, 128, f"gkb{p}c64", i) for p in PADS for i in range(NB)])
SEG2_CASES = [(M, N_PLAIN, 192, "seg2", 0) for M in MS] + [(M, G * w, 192, f"x2g{w}", 0) for M in MS for G in (2, 3) for w in (64, 128)]
ALL_CASES = tuple(dict.fromkeys(PLAIN_CASES + ADAPTER_CASES + GROUP_N_CASES + GROUP_K_CASES + BATCH_CASES + SEG2_CASES))


# ---------------------------------------------------------------------------------------------------------------- adapter gradients
GRAD_MS = (1, 31, 33, 97, 280)        # fewer 32-token chunks than waves, a partial last chunk, uneven chunks per wave
GRAD_CWS = (64, 200)                  # the last 64-column block of 200 is partial
GRAD_CW_VALU = 36                     # Cw % 8 != 0: the whole plan takes the VALU kernel
WIDE_RPS = (128, 192, 256)
CONV_MAPS = ((5, 7), (10, 14))        # B = 2: image borders inside a 32-token chunk
CONV_CINS = (64, 192, 32)             # Cin = 32: column blocks straddle taps -> VALU kernel


@functools.lru_cache(maxsize=None)
def grad_P(M, Cw):
    return _ints(torch.Generator().manual_seed(9000 + 31 * M + Cw), -2, 2, M, Cw)


@functools.lru_cache(maxsize=None)
def grad_Q(M, Rp, salt=0):
    return _ints(torch.Generator().manual_seed(9500 + 37 * M + Rp + 1009 * salt), -2, 2, M, Rp)


def grad_ref(Pm, Q, R, rank_major):
    """fp64 [Cw, R] or (rank_major) [R, Cw] of sum_m P[m][c] Q[m][r], r < R; Pm = P, or its 3 x 3 gather (conv_cols)."""
    out = Pm.to(F64).t() @ Q.to(F64)[:, :R]
    return out.t().contiguous() if rank_major else out


def conv_geom(B, H, W, Cin, stride):
    return Geom(B, H, W, Cin, (H - 1) // stride + 1, (W - 1) // stride + 1, stride=stride)


def conv_cols(X, g):
    """fp64 [M, 9 Cin] im2col of the NHWC activation X (k = tap * Cin + ci): conv9's own gather, read out by convolving with the identity."""
    return conv9(X, torch.eye(9 * g.Cin, dtype=F64), g)


@functools.lru_cache(maxsize=None)
def conv_problem(H, W, Cin, stride):
    """(geometry, P [B H W, Cin], fp64 gathered columns [M, 9 Cin]) of a conv-form gradient problem, B = 2."""
    g = conv_geom(2, H, W, Cin, stride)
    X = _ints(torch.Generator().manual_seed(9900 + 101 * H + W + Cin + stride), -2, 2, 2 * H * W, Cin)
    return g, X, conv_cols(X, g)


# ---------------------------------------------------------------------------------------------------------------- weight-gradient chain
@functools.lru_cache(maxsize=None)
def wgrad_operands(M, conv):
    """x [M, 136] (conv: the NHWC activation [M, 64] of three 5 x 7 maps, M = 105, or two 10 x 14 maps, M = 280), dy [M, 72]; fp64 dW = dy^T x (conv: dy^T im2col(x))."""
    g = torch.Generator().manual_seed(9990 + M + conv)
    N = 72
    dy = _ints(g, -2, 2, M, N)
    if conv:
        H, W = {105: (5, 7), 280: (10, 14)}[M]
        B = M // (H * W)
        geom = Geom(B, H, W, 64, H, W)
        x = _ints(g, -2, 2, M, 64)
        cols = conv_cols(x, geom)
    else:
        geom, x = None, _ints(g, -2, 2, M, 136)
        cols = x.to(F64)
    return dict(x=x, dy=dy, geom=geom, cols=cols, dW=dy.to(F64).t() @ cols)
