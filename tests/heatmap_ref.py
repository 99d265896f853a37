"""fp64 restatement of the two heat-map launches (include/sdlt_kernels.h: sdlt_heatmap_accum, sdlt_heatmap_overlay) - the oracle of tests/test_heatmap_cpu.py
and tests/test_heatmap_gpu.py - and `emu_heat`, tests/freeu_ref.emu_freeu plus torch forms of ops.heatmap_accum / ops.heatmap_overlay, so the CPU tests
run the host path.

Resampling is written as one matrix per axis.  `cubic_axis(n_in, n_out)` returns the weights of F.interpolate(mode="bicubic", align_corners=False)
(Keys, A = -0.75, border taps clamped; `self_check` holds it to torch in fp64) and, beside them, the MAGNITUDE operator of the kernel's form of the same
sum, a_1 + sum_{k != 1} w_k (a_k - a_1): the products that form are 1 a_1, w_k a_k and w_k a_1, so |a_1| + sum |w_k| (|a_k| + |a_1|) bounds every intermediate
value.  Applied to |source| along both axes, scaled and summed like the values, it is the `sum |tap weight x source value|` of the per-element error bound."""
import math
import types

import numpy as np
import torch

from tests import freeu_ref as FR

A = -0.75


def cubic_axis(n_in, n_out):
    """-> (W, M) fp64 [n_out, n_in]: weights and magnitude operator of one axis; identity for n_in == n_out (the kernel reads the source there)."""
    W, M = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    if n_in == n_out:
        return np.eye(n_in), np.eye(n_in)
    s = n_in / n_out
    for d in range(n_out):
        c = (d + 0.5) * s - 0.5
        i = math.floor(c)
        t = c - i
        u = 1.0 - t
        w = {0: A * t * u * u, 2: t * (1.0 + u * (1.0 - 1.25 * u)), 3: A * u * t * t}
        idx = [max(0, min(i - 1 + k, n_in - 1)) for k in range(4)]
        W[d, idx[1]] += 1.0 - sum(w.values())
        M[d, idx[1]] += 1.0
        for k, wk in w.items():
            W[d, idx[k]] += wk
            M[d, idx[k]] += abs(wk)
            M[d, idx[1]] += abs(wk)
    return W, M


def linear_axis(n_in, n_out):
    """Bilinear weights of one axis, fp64 [n_out, n_in] (F.interpolate(mode="bilinear", align_corners=False))."""
    W = np.zeros((n_out, n_in))
    s = n_in / n_out
    for d in range(n_out):
        c = max((d + 0.5) * s - 0.5, 0.0)
        i0 = min(math.floor(c), n_in - 1)
        t = c - i0
        W[d, i0] += 1.0 - t
        W[d, min(i0 + 1, n_in - 1)] += t
    return W


def self_check(sizes=((8, 12, 5, 7), (4, 6, 8, 12), (2, 3, 8, 12), (8, 12, 2, 3), (5, 7, 16, 9)), seed=0):
    """The axis matrices against torch's own resampling in fp64 on random planes -> the largest absolute differences (bicubic, bilinear)."""
    g = torch.Generator().manual_seed(seed)
    worst = [0.0, 0.0]
    for h, w, H, W in sizes:
        x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
        for j, (axis, mode) in enumerate(((lambda a, b: cubic_axis(a, b)[0], "bicubic"), (linear_axis, "bilinear"))):
            Wy, Wx = torch.from_numpy(axis(h, H)), torch.from_numpy(axis(w, W))
            mine = torch.einsum("yh,nchw,xw->ncyx", Wy, x, Wx)
            ref = torch.nn.functional.interpolate(x, size=(H, W), mode=mode, align_corners=False)
            worst[j] = max(worst[j], float((mine - ref).abs().max()))
    return tuple(worst)


def present(cols):
    """cols int [n, T, P] -> bool [n, T]: the map has a position."""
    return (np.asarray(cols) >= 0).any(-1)


def accum_ref(entries, cols, step, weights, heat, mag=None, *, row_off, row_stride=1, grid=None):
    """One sdlt_heatmap_accum call in fp64 -> (heat + increment, mag + magnitude of the increment).  entries: [(sums [B h w, ld], h, w, layers)] (any float
    dtype: read as fp64); cols int [n, T, P]; step: the counter's value; weights: the fp32 table; heat fp64 [n, T, gh, gw]."""
    heat = np.array(heat, dtype=np.float64)
    mag = np.zeros_like(heat) if mag is None else np.array(mag, dtype=np.float64)
    n, T, gh, gw = heat.shape
    cols = np.asarray(cols)
    wts = np.asarray(weights, dtype=np.float64)
    scale = wts[max(0, min(int(step), len(wts) - 1))] / float(sum(e[3] for e in entries))
    for s, h, w, _ in entries:
        s = np.asarray(s.detach().cpu().double() if torch.is_tensor(s) else s, dtype=np.float64)
        (Wy, My), (Wx, Mx) = cubic_axis(h, gh), cubic_axis(w, gw)
        planes = s.reshape(-1, h, w, s.shape[1])
        for i in range(n):
            blk = planes[row_off + i * row_stride]
            for t in range(T):
                for c in cols[i, t]:
                    if c >= 0:
                        heat[i, t] += scale * (Wy @ blk[:, :, c] @ Wx.T)
                        mag[i, t] += abs(scale) * (My @ np.abs(blk[:, :, c]) @ Mx.T)
    return heat, mag


def overlay_ref(heat, cols, image, lut, alpha):
    """sdlt_heatmap_overlay in fp64 from the fp32 maps -> (norm fp64 [n, T, gh, gw], out uint8 [n, T, H, W, 3], the unrounded levels fp64)."""
    heat = np.asarray(heat, dtype=np.float64)
    image, lut = np.asarray(image, dtype=np.float64), np.asarray(lut, dtype=np.float64)
    n, T, gh, gw = heat.shape
    H, W = image.shape[2:]
    here = present(cols)
    norm = np.zeros_like(heat)
    levels = np.zeros((n, T, H, W, 3))
    Wy, Wx = linear_axis(gh, H), linear_axis(gw, W)
    for i in range(n):
        pic = 255.0 * image[i].transpose(1, 2, 0)
        if here[i].any():
            lo, hi = heat[i, here[i]].min(), heat[i, here[i]].max()
            if hi - lo > 0:
                norm[i, here[i]] = (heat[i, here[i]] - lo) / (hi - lo)
        for t in range(T):
            if not here[i, t]:
                levels[i, t] = pic
                continue
            q = 255.0 * np.clip(Wy @ norm[i, t] @ Wx.T, 0.0, 1.0)
            k = np.minimum(np.floor(q).astype(np.int64), 254)
            f = (q - k)[..., None]
            colour = lut[k] + f * (lut[k + 1] - lut[k])
            levels[i, t] = (1.0 - alpha) * pic + alpha * colour
    return norm, np.clip(np.rint(levels), 0, 255).astype(np.uint8), levels


# ---- the whole trajectory in fp32 torch, with per-layer score maps
def sample_maps_ref(cfg, sd, lora, lora_scale, embeds, noise, steps, cols, grid="max", guidance_scale=8.0, size=None):
    """The fp32 reference loop of tests/img2img_ref.py (txt2img: zero init latents at strength 1) driven by the oracle UNet, which returns every hooked layer's
    score map [2, N, 77] -> (latents, maps fp64 [1, T, gh, gw]): per step the positive row's maps summed per resolution in fp64, through accum_ref with
    weight 1 / steps."""
    from oracle import unet_ref as U
    from tests import img2img_ref as IR
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    h, w = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    lora_s = None if lora is None else {k: (A_, B_ * lora_scale) for k, (A_, B_) in lora.items()}
    per_step = []

    def model(xin, t):
        out, daam = U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2), ctx, add, lora=lora_s, return_daam=True)
        per_step.append(layer_entries([m for _, m in daam], h, w)[0])
        return out

    with torch.no_grad():
        lat = IR.sample_loop(model, noise, steps, init_latents=torch.zeros_like(noise), strength=1.0, guidance_scale=guidance_scale)
    gh, gw = per_step[0][0][1:3] if grid == "max" else per_step[0][-1][1:3]
    maps = np.zeros((1, len(cols[0]), gh, gw))
    for i, entries in enumerate(per_step):
        maps, _ = accum_ref(entries, np.asarray(cols), i, [1.0 / steps] * steps, maps, row_off=1, row_stride=2)
    return lat, maps


def layer_entries(layer_maps, h, w):
    """Per-layer score maps [B, N, >= 77] of one forward at latent h x w -> (entries of their fp64 sums, entries of the sums of their magnitudes), finest
    resolution first, each [(fp64 [B N, columns], h_r, w_r, layers)]."""
    groups = {}
    for m in layer_maps:
        groups.setdefault(m.shape[1], []).append(m.detach().cpu().double())
    sums, mags = [], []
    for N in sorted(groups, reverse=True):
        k = next(k for k in range(16) if (h >> k) * (w >> k) == N)
        ms = groups[N]
        sums.append((sum(ms).reshape(-1, ms[0].shape[-1]), h >> k, w >> k, len(ms)))
        mags.append((sum(m.abs() for m in ms).reshape(-1, ms[0].shape[-1]), h >> k, w >> k, len(ms)))
    return sums, mags


# ---- the CPU op table
def heatmap_accum(entries, cols, ctr, weights, heat, *, row_off, row_stride=1):
    out, _ = accum_ref(entries, cols.numpy(), int(ctr[0]), weights.numpy(), heat.double().numpy(), row_off=row_off, row_stride=row_stride)
    heat.copy_(torch.from_numpy(out).to(heat.dtype))
    return heat


def heatmap_overlay(heat, cols, image, lut, *, alpha=0.6):
    norm, out, _ = overlay_ref(heat.numpy(), cols.numpy(), image.numpy(), lut.numpy(), float(np.float32(alpha)))
    return torch.from_numpy(norm).to(heat.dtype), torch.from_numpy(out)


def with_heat(table, name):
    mod = types.ModuleType(name)
    mod.__dict__.update({k: v for k, v in vars(table).items() if not k.startswith("__")})
    mod.heatmap_accum, mod.heatmap_overlay = heatmap_accum, heatmap_overlay
    return mod


emu_heat = with_heat(FR.emu_freeu, "emu_heat")
