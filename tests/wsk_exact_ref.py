"""Exact-arithmetic reference of the wave-split-K product (sdlt_wsk_gemm / _p / _rowdot / _parts, csrc/wsk.hip) and of the row-strip product of the
text encoders (sdlt_strip_gemm / _pair, csrc/strip.hip): the case lists, the small-integer operands and the fp64 references.  Plain torch on the CPU;
imports nothing from the project (tests/gemm_exact_ref.py supplies `rounded`, `gemm_ref` and the operand generators).

The contracts restated (include/sdlt_kernels.h):

  wave-split-K   v  = col_scale[n] * (X W^T + Tb Bup^T) + bias[n]                 Tb = bf16(s * X Adown^T) = T_out (per K group with lora_group_k)
                 Y0 = rounded(v)                                                  "the layer's own output BEFORE the residual"
                 Y  = rounded(v + R)                                              "(= that value in fp32 + R)"; with dotD R is the attention output O, "NOT added to Y"
                 D[(b H + h) Nq + q] = sum over head h's 64 columns of bf16(Y)[m, n] O[m, n],   m = b Nq + q, H = N / 64
                 ln_parts[m, tn, 0]  = sum of bf16(Y)[m, 80 tn .. 80 tn + 79]
  row strip      Y[b Tp + t] = X[b Tp + t] W^T + bias + R[b Tp + t]   for t < T;  slab s of P = the fp32 product over the K columns [s K / S, (s + 1) K / S)

Operands follow tests/gemm_exact_ref.py: X, O in {-2..2}, W / Bup in {-1, 0, 1}, three +-1 per Adown row (per K group where K is grouped), s = 0.5,
col_scale in {0.5, 1, 2}, small-integer bias / residual.  Every partial sum - a wave's quarter of K, a K group, a strip split, a head's or a tile's
row sum of the rounded output - is then a multiple of 0.25 far below 2^24 (tests/test_wsk_exact_cpu.py asserts it), so an fp32 result depends on
no wave split, ring depth, stagger, strip width, split count or atomic order and equals the fp64 one bit for bit."""
import functools

import torch

from tests.gemm_exact_ref import BF, F32, F64, LORA_SCALE, _ints, _sparse_rows, gemm_ref, rounded  # noqa: F401  (re-exported)

NW = 4                                # waves of a workgroup, in both kernels: wave w walks the 64-column steps w, w + 4, ... of its K range
TILE_M, TILE_N, HEAD = 64, 80, 64     # the wave-split-K output tile; a head of the row-dot side output

# ================================================================================================================ wave-split-K
WSK_MS = (64, 128, 192, 448)          # one row tile (1D XCD map), two (2D map), odd row-tile counts
WSK_NS = (640, 1280)
WSK_KS = (256, 768, 1024, 2304)       # 1 / 3 / 4 / 9 K steps per wave: one step, the packed ring's depth, a refill on both rings, a wrapping tile rotation
WSK_REDUCED = ((64, 640, 256), (128, 640, 1024), (192, 1280, 768), (448, 640, 2304))
# (M, N, K, lora_group_k): G = 2 with the seam between waves' steps, G = 2 with the seam on a wave seam, G = 3 with seams inside waves, G = 2 over 4 steps per wave
WSK_GROUPED = ((64, 640, 256, 128), (192, 1280, 768, 384), (192, 1280, 768, 256), (128, 640, 1024, 512))

# form -> options.  pad: the adapter's padded rank; T: T_out is requested; cs: col_scale; y0: the second output; dot: the row-dot side output with
# Nq = 64 or M; parts: ln_parts; pf: the next-weight prefetch hint.  What the flat entry points cannot say (cs, y0, pad 32, pf) runs through sdlt_wsk_gemm_p only.
WSK_FORMS = {
    "plain": dict(),
    "bias": dict(bias=1),
    "biasR": dict(bias=1, R=1),
    "parts": dict(bias=1, R=1, parts=1),
    "dot64": dict(bias=1, dot=64),
    "dotM": dict(dot="M"),
    "lora": dict(pad=16),
    "loraT": dict(pad=16, T=1, bias=1, R=1),
    "loracs": dict(pad=16, T=1, cs=1, bias=1),
    "loray0": dict(pad=16, T=1, cs=1, bias=1, y0=1),
    "loray0R": dict(pad=16, cs=1, bias=1, y0=1, R=1),
    "loradot64": dict(pad=16, T=1, dot=64),
    "loradotM": dict(pad=16, T=1, bias=1, dot="M"),
    "loraparts": dict(pad=16, T=1, R=1, parts=1),
    "lorapf": dict(pad=16, T=1, bias=1, R=1, pf=1),
    "rp32": dict(pad=32, T=1, bias=1, R=1),
    "rp32y0": dict(pad=32, T=1, cs=1, bias=1, y0=1, R=1),
    "rp32dot": dict(pad=32, dot=64),
    "gk": dict(pad=16, T=1, R=1),
    "gkbias": dict(pad=16, T=1, bias=1),
}
WSK_PLAIN_CASES = tuple((M, N, K, "plain", 0) for M in WSK_MS for N in WSK_NS for K in WSK_KS)
WSK_EPILOGUE_CASES = tuple((M, N, K, f, 0) for (M, N, K) in WSK_REDUCED for f in ("bias", "biasR", "parts"))
WSK_ADAPTER_CASES = tuple((M, N, K, f, 0) for (M, N, K) in WSK_REDUCED for f in ("lora", "loraT", "loracs", "loray0", "loray0R", "loraparts"))
WSK_ROWDOT_CASES = tuple(dict.fromkeys((M, N, K, f + ("64" if M == 64 else nq), 0) for (M, N, K) in WSK_REDUCED for f in ("dot", "loradot") for nq in ("64", "M")))
WSK_RP32_CASES = tuple((M, N, K, f, 0) for (M, N, K) in WSK_REDUCED for f in ("rp32", "rp32y0", "rp32dot"))
WSK_GROUP_K_CASES = tuple((M, N, K, f, gk) for (M, N, K, gk) in WSK_GROUPED for f in ("gk", "gkbias"))
WSK_PREFETCH_CASES = tuple((M, N, K, "lorapf", 0) for (M, N, K) in WSK_REDUCED)
ALL_WSK_CASES = tuple(dict.fromkeys(WSK_PLAIN_CASES + WSK_EPILOGUE_CASES + WSK_ADAPTER_CASES + WSK_ROWDOT_CASES + WSK_RP32_CASES + WSK_GROUP_K_CASES
                                    + WSK_PREFETCH_CASES))


@functools.lru_cache(maxsize=None)
def wsk_operands(M, N, K, gk=0):
    """Everything a wave-split-K case can use, from one seeded generator.  Adown has 32 rows (rank pad 32; pad 16 uses the first 16), Bup 48 columns
    (three K groups of 16); gk > 0: Adown's entries are placed per K group of gk columns."""
    g = torch.Generator().manual_seed(8100 + 131 * M + 17 * N + K + 3 * gk)
    d = dict(M=M, N=N, K=K)
    d["X"] = _ints(g, -2, 2, M, K)
    d["W"] = _ints(g, -1, 1, N, K)
    d["bias"] = _ints(g, -4, 4, N, dtype=F32)
    d["residual"] = _ints(g, -8, 8, M, N)
    d["O"] = _ints(g, -2, 2, M, N)
    d["Adown"] = _sparse_rows(g, 32, K, gk or K)
    d["Bup"] = _ints(g, -1, 1, N, 48)
    d["col_scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    return d


def wsk_nq(M, v):
    """Rows per batch element of the row-dot side output (0: none)."""
    return 0 if not v.get("dot") else (M if v["dot"] == "M" else int(v["dot"]))


def wsk_t_width(K, v, gk):
    return v.get("pad", 0) * (K // gk if gk else 1)


def wsk_adapter(d, v, gk):
    """(Adown, Bup) of a form from an operand set (CPU tensors or the same dict on a device), or None."""
    pad = v.get("pad", 0)
    return (d["Adown"][:pad], d["Bup"][:, :wsk_t_width(d["K"], v, gk)]) if pad else None


def rowdot_ref(Yb, O, Nq):
    """D[(b H + h) Nq + q] of the ROUNDED output Yb (fp64 values of the bf16 result) and O, both [M, N]."""
    M, N = Yb.shape
    return (Yb * O.to(F64)).reshape(M // Nq, Nq, N // HEAD, HEAD).sum(-1).permute(0, 2, 1).reshape(-1)


def parts_ref(Yb):
    """ln_parts[..., 0]: the sum of the ROUNDED output over each 80-column tile, [M, N / 80]."""
    M, N = Yb.shape
    return Yb.reshape(M, N // TILE_N, TILE_N).sum(-1)


@functools.lru_cache(maxsize=None)
def wsk_reference(M, N, K, form, gk=0):
    """dict(Y, T, Y0, D, parts): fp64 before the output rounding (T: bf16), None where the form has no such output.  Computed once, never modified."""
    d, v = wsk_operands(M, N, K, gk), WSK_FORMS[form]
    ad = wsk_adapter(d, v, gk)
    v0, T = gemm_ref(d["X"], d["W"], lora=(ad + (LORA_SCALE,)) if ad else None, lora_group_k=gk, col_scale=d["col_scale"] if v.get("cs") else None,
                     bias=d["bias"] if v.get("bias") else None)
    Y = v0 + d["residual"].to(F64) if v.get("R") else v0        # sdlt_kernels.h: "Y0 ... written next to Y (= that value in fp32 + R)"
    Yb = rounded(Y, BF).to(F64)
    Nq = wsk_nq(M, v)
    return dict(Y=Y, T=T if v.get("T") else None, Y0=v0 if v.get("y0") else None, D=rowdot_ref(Yb, d["O"], Nq) if Nq else None,
                parts=parts_ref(Yb) if v.get("parts") else None)


def wave_columns(K, w, k_lo=0):
    """The K columns wave w of a workgroup walks in [k_lo, k_lo + K): the 64-column steps w, w + 4, ..."""
    k = torch.arange(K)
    return k_lo + k[(k // 64) % NW == w]


# ================================================================================================================ row strip
STRIP_TS = (1, 16, 17, 77, 80)
STRIP_TPS = (80, 96)
STRIP_BS = (1, 3)
STRIP_KS = (256, 768, 2304)           # 1 / 3 / 9 K steps per wave; 9 > two ring turns: the weight touches ahead of the ring run
STRIP_NS = (16, 48, 2304, 2320)       # 2304: the 32-column kernel; 2320 >= the width threshold but no multiple of 32: 16-column strips
STRIP_N_PAIR = 2368                   # a second width that takes the 32-column kernel (the partner of 2304 in a paired launch)
STRIP_ROWS = 80                       # operands are made for 80 rows per batch element; a case uses the first T
STRIP_REDUCED = ((1, 1, 80, 16, 256), (3, 17, 96, 48, 768), (3, 77, 80, 2304, 2304), (1, 80, 96, 2320, 768), (3, 16, 80, 2304, 768), (1, 77, 96, 48, 2304))
STRIP_FORMS = {"plain": dict(), "bias": dict(bias=1), "biasR": dict(bias=1, R=1), "split2": dict(bias=1, R=1, split=2), "split3": dict(split=3),
               "split9": dict(bias=1, split=9), "slab1": dict(slabs=1), "slab3": dict(slabs=3)}
# (B, T, Tp, N, K, form)
STRIP_PLAIN_CASES = tuple((B, T, Tp, N, K, "plain") for N in STRIP_NS for K in STRIP_KS for B in STRIP_BS for T in STRIP_TS for Tp in STRIP_TPS)
STRIP_EPILOGUE_CASES = tuple((B, T, Tp, N, K, f) for (B, T, Tp, N, K) in STRIP_REDUCED for f in ("bias", "biasR"))
STRIP_SPLIT_CASES = (tuple((B, T, Tp, N, 768, f) for N in STRIP_NS for (B, T, Tp) in ((1, 17, 80), (3, 77, 96)) for f in ("split2", "split3"))
                     + tuple((B, T, Tp, N, 2304, "split9") for N in STRIP_NS for (B, T, Tp) in ((1, 80, 96), (3, 16, 80))))
STRIP_SLAB_CASES = tuple((B, T, Tp, N, K, f) for N in STRIP_NS for (B, T, Tp, K) in ((1, 17, 80, 768), (3, 77, 96, 2304), (3, 1, 80, 768)) for f in ("slab1", "slab3"))
# paired launches: two problems that differ in N, K, B and T; 16- with 16-column strips, 32- with 32-column strips, and two partial outputs
STRIP_PAIRS = (((1, 17, 80, 16, 256, "biasR"), (3, 77, 96, 48, 768, "plain")),
               ((3, 16, 80, 2304, 768, "bias"), (1, 77, 96, STRIP_N_PAIR, 256, "biasR")),
               ((1, 80, 96, 48, 768, "slab3"), (3, 1, 80, 16, 256, "slab1")))
STRIP_PAIR_CASES = tuple(c for pair in STRIP_PAIRS for c in pair)
ALL_STRIP_CASES = tuple(dict.fromkeys(STRIP_PLAIN_CASES + STRIP_EPILOGUE_CASES + STRIP_SPLIT_CASES + STRIP_SLAB_CASES + STRIP_PAIR_CASES))


@functools.lru_cache(maxsize=None)
def strip_X(B, K):
    return _ints(torch.Generator().manual_seed(8500 + 7 * B + K), -2, 2, B, STRIP_ROWS, K)


@functools.lru_cache(maxsize=None)
def strip_W(N, K):
    return _ints(torch.Generator().manual_seed(8600 + 13 * N + K), -1, 1, N, K)


@functools.lru_cache(maxsize=None)
def strip_bias(N):
    return _ints(torch.Generator().manual_seed(8700 + N), -4, 4, N, dtype=F32)


@functools.lru_cache(maxsize=None)
def strip_R(B, N):
    return _ints(torch.Generator().manual_seed(8800 + 7 * B + N), -8, 8, B, STRIP_ROWS, N)


def split_ranges(K, S):
    """[k_lo, k_hi) of each of S splits: the K / 256 steps of 256 columns dealt out as evenly as they go, the first splits taking one more
    (sdlt_kernels.h asks for K % (256 S) == 0 where slabs are read; the host check admits any S <= K / 256 for the in-kernel split)."""
    steps, out, lo = K // 256, [], 0
    for s in range(S):
        n = steps // S + (1 if s < steps % S else 0)
        out.append((lo * 256, (lo + n) * 256))
        lo += n
    assert lo == steps and all(hi > lo_ for lo_, hi in out)
    return out


@functools.lru_cache(maxsize=None)
def strip_full(B, N, K, form):
    """(fp64 [B, 80, N] result of all 80 rows, fp64 [S, B, 80, N] slabs or None); a case reads the first T rows.  Computed once, never modified."""
    v = STRIP_FORMS[form]
    x, w = strip_X(B, K).to(F64), strip_W(N, K).to(F64)
    if v.get("slabs"):
        S = v["slabs"]
        assert K % (256 * S) == 0
        return None, torch.stack([x[..., lo:hi] @ w[:, lo:hi].t() for lo, hi in split_ranges(K, S)])
    acc = x @ w.t()
    if v.get("bias"):
        acc = acc + strip_bias(N).to(F64)
    if v.get("R"):
        acc = acc + strip_R(B, N).to(F64)
    return acc, None


def strip_reference(B, T, Tp, N, K, form):
    """(fp64 [B, T, N] or None, fp64 slabs [S, B, T, N] or None) of a case: views of strip_full's tensors."""
    acc, slabs = strip_full(B, N, K, form)
    return (acc[:, :T] if acc is not None else None), (slabs[:, :, :T] if slabs is not None else None)


def strip_layout(valid, Tp, pad):
    """[..., B, T, N] -> [..., B Tp, N] as the kernel's buffers hold it, the rows t >= T filled with `pad`."""
    *lead, B, T, N = valid.shape
    out = torch.full((*lead, B, Tp, N), pad, dtype=valid.dtype, device=valid.device)
    out[..., :T, :] = valid
    return out.reshape(*lead, B * Tp, N)
