"""Self-attention guidance in fp64 torch: the three formulas of include/sdlt_kernels.h (sdlt_attn_colmass, sdlt_sag_degrade, sdlt_sag_apply), nothing else."""
import torch
import torch.nn.functional as F


def colmass(Q, K, L, *, B, H, N, d, scale, rows, dtype=torch.float64):
    """mass [len(rows), N] = (1 / H) sum_h sum_q exp(scale Q_h[q] . K_h[k] - L[b, h, q]) for the batch rows b in `rows`; Q, K [B N, >= H d], L [B, H, N]."""
    q = Q.to(dtype)[:, :H * d].reshape(B, N, H, d)[rows].permute(0, 2, 1, 3)
    k = K.to(dtype)[:, :H * d].reshape(B, N, H, d)[rows].permute(0, 2, 1, 3)
    p = torch.exp(scale * (q @ k.transpose(-1, -2)) - L.to(dtype).reshape(B, H, N)[rows][..., None])
    return p.sum(2).sum(1) / H


def degrade(x, eps, mass, taps, row, grid):
    """out fp64 [n h w, 4] before the bf16 rounding; x [n, 4, h, w], eps [2 n h w, 4], mass [n, hm wm], taps [9], row = (sigma, scale, threshold, 0)."""
    n, _, h, w = x.shape
    (hm, wm), sigma, thr = grid, float(row[0]), float(row[2])
    e = eps.double().reshape(n, 2, h, w, 4)[:, 0].permute(0, 3, 1, 2)
    x0 = x.double() - sigma * e
    t = taps.double()
    pad = F.pad(x0, (4, 4, 4, 4), mode="reflect")
    blur = F.conv2d(F.conv2d(pad.reshape(n * 4, 1, h + 8, w + 8), t.reshape(1, 1, 1, 9)), t.reshape(1, 1, 9, 1)).reshape(n, 4, h, w)
    ys, xs = torch.arange(h) * hm // h, torch.arange(w) * wm // w
    mask = (mass.reshape(n, hm, wm)[:, ys][:, :, xs] > thr)[:, None]
    out = (torch.where(mask, blur, x0) + sigma * e) / (sigma * sigma + 1.0) ** 0.5
    return out.permute(0, 2, 3, 1).reshape(n * h * w, 4)


def apply(eps, t, scale, n, phase):
    """phase 0 -> t' = scale (e_neg - t); phase 1 -> eps with t added to both row blocks of every image (fp64)."""
    e = eps.double().reshape(n, 2, -1, 4)
    if phase == 0:
        return scale * (e[:, 0] - t.double().reshape(n, -1, 4)).reshape(-1, 4)
    return (e + t.double().reshape(n, 1, -1, 4)).reshape(-1, 4)
