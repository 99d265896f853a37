"""The tiled VAE passes restated independently of vae.py: the tile geometry and the normalised feather weights in plain loops, exact
rationals and fp64; `blend`, the composition of a picture from its tiles in fp64; and `blend32`, the same composition in torch fp32 in the operation
order of sdlt_tile_blend (t = wy wx, u = t v, out = out + u: one rounding each), which the kernel has to match bit for bit."""
from fractions import Fraction

import numpy as np
import torch


def tile_starts(L, T, O):
    if T < 2 or O < 0 or 2 * O > T:
        raise ValueError((T, O))
    if L <= T:
        return [0]
    n = 2
    while O + n * (T - O) < L:               # the fewest tiles that cover L with overlaps of at least O: n T - (n - 1) O >= L
        n += 1
    out = []
    for k in range(n):
        x = Fraction(k * (L - T), n - 1) + Fraction(1, 2)
        out.append(x.numerator // x.denominator)            # floor(k (L - T) / (n - 1) + 1 / 2)
    return out


def extent(L, T):
    return min(L, T)


def raw_weight(k, n, p, E, R):
    w = 1.0
    if R > 0 and k > 0:
        w = min(w, (p + 0.5) / R)
    if R > 0 and k < n - 1:
        w = min(w, (E - p - 0.5) / R)
    return w


def tile_weights(L, T, O, g):
    """-> one list of E python floats (fp64) per tile."""
    starts = tile_starts(L, T, O)
    n, E, R = len(starts), g * extent(L, T), g * O
    out = []
    for k in range(n):
        row = []
        for p in range(E):
            x = g * starts[k] + p                             # the sample on the whole axis
            total = 0.0
            for j in range(n):
                q = x - g * starts[j]
                if 0 <= q < E:
                    total += raw_weight(j, n, q, E, R)
            row.append(raw_weight(k, n, p, E, R) / total)
        out.append(row)
    return out


def weights32(L, T, O, g):
    """The tables as the kernel gets them: fp64, rounded once -> list of fp32 tensors."""
    return [torch.from_numpy(np.asarray(r, dtype=np.float64).astype(np.float32)) for r in tile_weights(L, T, O, g)]


def _tiles(tiles, ys, xs):
    assert len(tiles) == len(ys) * len(xs), (len(tiles), len(ys), len(xs))
    return [(tiles[i * len(xs) + j], i, j) for i in range(len(ys)) for j in range(len(xs))]      # row-major


def blend(tiles, ys, xs, wys, wxs, C, H, W, absolute=False):
    """tiles: row-major list of [th, tw, >= C] tensors (NHWC); ys, xs: the tiles' starts on the output grid; wys, wxs: their 1-D weight tables (the
    fp32 tables the kernel reads, taken to fp64 exactly) -> [C, H, W] fp64 = sum of wy wx v; absolute: sum of |wy wx v| (the scale of the rounding bound)."""
    out = torch.zeros(C, H, W, dtype=torch.float64)
    for t, i, j in _tiles(tiles, ys, xs):
        wy, wx = wys[i].double(), wxs[j].double()
        th, tw = wy.numel(), wx.numel()
        u = (wy[:, None] * wx[None, :])[:, :, None] * t[:, :, :C].double().reshape(th, tw, C)
        out[:, ys[i]:ys[i] + th, xs[j]:xs[j] + tw] += (u.abs() if absolute else u).permute(2, 0, 1)
    return out


def blend32(tiles, ys, xs, wys, wxs, C, H, W, out=None):
    """The same in fp32, in the kernel's order: per tile (row-major) t = wy * wx, u = t * v, out = out + u, each rounded once (torch's CPU fp32 multiply
    and add are separate operations: nothing is contracted).  out: accumulate into this [C, H, W] fp32 tensor instead of zeros."""
    out = torch.zeros(C, H, W, dtype=torch.float32) if out is None else out
    for t, i, j in _tiles(tiles, ys, xs):
        wy, wx = wys[i].float().cpu(), wxs[j].float().cpu()
        th, tw = wy.numel(), wx.numel()
        tt = wy[:, None] * wx[None, :]
        u = tt[:, :, None] * t[:, :, :C].float().cpu().reshape(th, tw, C)
        view = out[:, ys[i]:ys[i] + th, xs[j]:xs[j] + tw]
        view.copy_(view + u.permute(2, 0, 1))
    return out


def nhwc(chw):
    """[1, C, H, W] or [C, H, W] (what decode / encode return for one tile) -> [H, W, C]."""
    chw = chw[0] if chw.dim() == 4 else chw
    return chw.permute(1, 2, 0).contiguous()
