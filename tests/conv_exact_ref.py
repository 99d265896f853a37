"""Exact-arithmetic reference of the implicit-GEMM 3 x 3 convolution (sdlt_gemm_bf16 mode 1 / MODE 2, sdlt_wsk_conv) and the small-integer
operands that make it exact.  Plain torch on the CPU; imports nothing from the project.

The contract restated (csrc/gemm.hip header, ops.gemm docstring): X is an NHWC activation [B*Hin*Win, Cin], W is [N, 9*Cin] with
k = tap*Cin + ci, tap = 3*dy + dx, padding 1.  Output pixel (oh, ow) of image b reads, for tap (dy, dx) with offset (oy, ox) = (dy-1, dx-1)
- or (1-dy, 1-dx) when flip = 1 -

  * stride s, input upsampled nearest by ups:   X[b, (oh*s + oy) // ups, (ow*s + ox) // ups]   if 0 <= oh*s + oy < Hin*ups (same in x)
  * transposed stride 2 (tr = 1, with flip):     X[b, (oh + oy) / 2, (ow + ox) / 2]            if oh + oy >= 0, even, < 2*Hin (same in x)

and zero otherwise.  Epilogue:  col_scale[n] * alpha * (conv + X2 . W2^T + Tb . Bup^T) + bias[n] + rowbias[m // rows_per_batch, n] + residual[m, n]
with Tb = bf16(s * conv(X, Adown)), which is also T_out.

With X in {-2..2}, W / Bup / W2 in {-1, 0, 1}, at most three +-1 per Adown row, s = 0.5, col_scale in {0.5, 1, 2} and small-integer bias /
row bias / residual, every partial sum is an integer (or a multiple of 0.25) far below 2^24: an fp32 result does not depend on the summation
order, tile, K split or ring depth and equals the fp64 one bit for bit; a bf16 result is the one RNE rounding of that exact value.
"""
import functools

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
LORA_SCALE = 0.5
N_TILED, N_WSK, K2 = 200, 640, 128


class Geom:
    """Same fields as ops.ConvGeom / emu_ops.ConvGeom (conv_ref takes any of the three)."""
    __slots__ = ("B", "Hin", "Win", "Cin", "Hout", "Wout", "stride", "ups", "flip", "tr")

    def __init__(self, B, Hin, Win, Cin, Hout, Wout, stride=1, ups=1, flip=0, tr=0):
        self.B, self.Hin, self.Win, self.Cin, self.Hout, self.Wout = B, Hin, Win, Cin, Hout, Wout
        self.stride, self.ups, self.flip, self.tr = stride, ups, flip, tr

    @property
    def M(self):
        return self.B * self.Hout * self.Wout

    def as_kwargs(self):
        return {k: getattr(self, k) for k in self.__slots__}


# name -> (B, Hin, Win, kind).  M = 280 / 135 / 280 / 280 / 540 / 105: ragged against the 64-, 128- and 256-row tiles, image boundaries inside tiles
GEOMS = {
    "s1": (2, 10, 14, "s1"),
    "s2": (3, 10, 18, "s2"),
    "ups": (2, 5, 7, "ups"),
    "flip": (2, 10, 14, "flip"),
    "tr": (3, 5, 9, "tr"),
    "small": (3, 5, 7, "s1"),
}
CINS = (64, 192)
# sdlt_wsk_conv: the smallest maps its host check takes (B*H*W % 64 == 0); 48-row images put image boundaries inside the 64-row tiles
WSK_MAPS = ((1, 8, 8), (2, 4, 8), (4, 4, 12))
WSK_CINS = (64, 192, 320)


def make_geom(kind, B, Hin, Win, Cin):
    if kind == "s1":
        return Geom(B, Hin, Win, Cin, Hin, Win)
    if kind == "s2":
        assert Hin % 2 == 0 and Win % 2 == 0
        return Geom(B, Hin, Win, Cin, Hin // 2, Win // 2, stride=2)
    if kind == "ups":
        return Geom(B, Hin, Win, Cin, 2 * Hin, 2 * Win, ups=2)
    if kind == "flip":
        return Geom(B, Hin, Win, Cin, Hin, Win, flip=1)
    if kind == "tr":
        return Geom(B, Hin, Win, Cin, 2 * Hin, 2 * Win, flip=1, tr=1)
    raise ValueError(kind)


def tiled_geom(name, Cin):
    B, Hin, Win, kind = GEOMS[name]
    return make_geom(kind, B, Hin, Win, Cin)


def _axis(n_out, n_in, off, g):
    """Source index along one axis for every output index, and whether the tap lies inside the (upsampled) image."""
    o = torch.arange(n_out)
    if g.tr:
        p = o + off
        ok = (p >= 0) & (p % 2 == 0) & (p < 2 * n_in)
        src = torch.div(p, 2, rounding_mode="floor")
    else:
        p = o * g.stride + off
        ok = (p >= 0) & (p < n_in * g.ups)
        src = torch.div(p, g.ups, rounding_mode="floor")
    return src.clamp(0, n_in - 1), ok


def conv9(X, Wm, g):
    """fp64 [B*Hout*Wout, N]: nine shifted, masked adds, one per tap."""
    N = Wm.shape[0]
    assert tuple(X.shape) == (g.B * g.Hin * g.Win, g.Cin) and Wm.shape[1] == 9 * g.Cin
    x = X.to(F64).reshape(g.B, g.Hin, g.Win, g.Cin)
    w = Wm.to(F64).reshape(N, 9, g.Cin)
    out = torch.zeros(g.B, g.Hout, g.Wout, N, dtype=F64)
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        oy, ox = (1 - dy, 1 - dx) if g.flip else (dy - 1, dx - 1)
        hi, oky = _axis(g.Hout, g.Hin, oy, g)
        wi, okx = _axis(g.Wout, g.Win, ox, g)
        patch = x[:, hi][:, :, wi]                                       # [B, Hout, Wout, Cin]
        mask = (oky[:, None] & okx[None, :]).to(F64)[None, :, :, None]
        out += (patch * mask) @ w[:, tap].t()
    return out.reshape(g.M, N)


def conv_ref(X, Wm, g, *, X2=None, W2=None, lora=None, col_scale=None, bias=None, rowbias=None, rows_per_batch=0, residual=None, alpha=1.0):
    """-> (fp64 result [M, N] before the output rounding, T_out bf16 [M, Rp] or None).  lora = (Adown [Rp, 9 Cin], Bup [N, Rp], scale)."""
    acc = conv9(X, Wm, g)
    if X2 is not None:
        acc = acc + X2.to(F64) @ W2.to(F64).t()
    T_out = None
    if lora is not None:
        Adown, Bup, scale = lora[:3]
        T_out = (conv9(X, Adown, g) * scale).to(F32).to(BF)             # the contract rounds s*T to bf16 here
        acc = acc + T_out.to(F64) @ Bup.to(F64).t()
    acc = acc * alpha
    if col_scale is not None:
        acc = acc * col_scale.to(F64)[None, :]
    if bias is not None:
        acc = acc + bias.to(F64)[None, :]
    if rowbias is not None:
        acc = acc + rowbias.to(F64)[torch.arange(acc.shape[0]) // rows_per_batch]
    if residual is not None:
        acc = acc + residual.to(F64)
    return acc, T_out


def rounded(acc, dtype):
    """The exact fp64 value in the output's format: nothing to round for fp32 (asserted), one RNE rounding for bf16."""
    f = acc.to(F32)
    assert torch.equal(f.to(F64), acc), "the operands do not keep the result exact in fp32"
    return f if dtype == F32 else f.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- operands
def _ints(g, lo, hi, *shape, dtype=BF):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def make_operands(geom, N, seed):
    """Everything a case can use, from one seeded generator.  Adown / Bup are cut for rank pad 64; pads 16 / 32 use the first rows / columns."""
    g = torch.Generator().manual_seed(seed)
    K = 9 * geom.Cin
    M = geom.M
    d = dict(geom=geom, N=N)
    d["X"] = _ints(g, -2, 2, geom.B * geom.Hin * geom.Win, geom.Cin)
    d["W"] = _ints(g, -1, 1, N, K)
    d["bias"] = _ints(g, -4, 4, N, dtype=F32)
    d["rowbias"] = _ints(g, -3, 3, geom.B, N)
    d["residual"] = _ints(g, -8, 8, M, N)
    A = torch.zeros(64, K, dtype=BF)
    cols = torch.randint(0, K, (64, 3), generator=g)
    A[torch.arange(64)[:, None], cols] = (torch.randint(0, 2, (64, 3), generator=g) * 2 - 1).to(BF)      # <= three +-1 per row: |T| <= 6
    d["Adown"] = A
    d["Bup"] = _ints(g, -1, 1, N, 64)
    d["col_scale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    d["X2"] = _ints(g, -2, 2, M, K2)
    d["W2"] = _ints(g, -1, 1, N, K2)
    return d


@functools.lru_cache(maxsize=None)
def tiled_operands(name, Cin):
    return make_operands(tiled_geom(name, Cin), N_TILED, 1000 + 17 * sorted(GEOMS).index(name) + Cin)


@functools.lru_cache(maxsize=None)
def wsk_operands(B, H, W, Cin, flip):
    return make_operands(Geom(B, H, W, Cin, H, W, flip=flip), N_WSK, 5000 + 97 * B + 13 * H + W + Cin + flip)


# the epilogue variants of the tiled kernel's tests.  name -> which operands take part
VARIANTS = {
    "plain": dict(),
    "full": dict(bias=1, rowbias=1, residual=1),
    "lora16": dict(pad=16), "lora32": dict(pad=32), "lora64": dict(pad=64),
    "lora16cs": dict(pad=16, cs=1), "lora32cs": dict(pad=32, cs=1), "lora64cs": dict(pad=64, cs=1),
    "lora16full": dict(pad=16, cs=1, bias=1, rowbias=1, residual=1),
    "seg2": dict(seg2=1),
}
WSK_VARIANTS = {
    "plain": dict(), "extras": dict(bias=1, rowbias=1, residual=1), "lora16": dict(pad=16), "lora16extras": dict(pad=16, bias=1, rowbias=1, residual=1),
}


def variant_kwargs(d, v, T_out=None, four=True):
    """gemm() keyword arguments of a variant from an operand set (CPU tensors, or the same dict moved to a device)."""
    kw = {}
    if v.get("pad"):
        Rp = v["pad"]
        kw["lora"] = (d["Adown"][:Rp], d["Bup"][:, :Rp], LORA_SCALE) + ((T_out,) if four else ())
    if v.get("cs"):
        kw["col_scale"] = d["col_scale"]
    if v.get("bias"):
        kw["bias"] = d["bias"]
    if v.get("rowbias"):
        kw["rowbias"], kw["rows_per_batch"] = d["rowbias"], d["geom"].Hout * d["geom"].Wout
    if v.get("residual"):
        kw["residual"] = d["residual"]
    if v.get("seg2"):
        kw["X2"], kw["W2"] = d["X2"], d["W2"]
    return kw


def _reference(d, v):
    return conv_ref(d["X"], d["W"], d["geom"], **variant_kwargs(d, v, four=False))


@functools.lru_cache(maxsize=None)
def tiled_reference(name, Cin, variant):
    """(fp64 result, T_out) of a tiled-kernel case; computed once, shared by every test that needs it, never modified."""
    return _reference(tiled_operands(name, Cin), VARIANTS[variant])


@functools.lru_cache(maxsize=None)
def wsk_reference(B, H, W, Cin, flip, variant):
    return _reference(wsk_operands(B, H, W, Cin, flip), WSK_VARIANTS[variant])
