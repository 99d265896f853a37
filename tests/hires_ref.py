"""NumPy float32 restatement of sdlt_resize_planes (include/sdlt_kernels.h) and the two-pass hires reference built on it.

`resize(x, H, W, mode)` evaluates the header's contract - PyTorch's align_corners=False conventions, every operation rounded once to float32 in the
order the header writes down: the scale as one division, the coordinate, the fraction, the weights, the horizontal sums (taps left to right), then the
vertical sum (rows top to bottom).  The GPU tests compare bits with it; tests/test_hires_cpu.py holds it to torch.nn.functional.interpolate.

`second_pass` is the hires second pass as the issue defines it: tests/img2img_ref.sample_latents (the fp32 reference loop of img2img) started from the
resized first-pass latents at the large shape.
"""
import numpy as np
import torch

from tests import img2img_ref as IR

MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
f32 = np.float32


def _keys_outer(t, u):
    m = f32(-0.75) * t
    m = m * u
    return m * u


def _keys_inner(t, u):
    m = f32(1.25) * u
    m = f32(1.0) - m
    m = m * u
    m = m + f32(1.0)
    return m * t


def _combine(a, w):
    """One axis' sum of the header: a = the taps' values (2 or 4 arrays), w = their weights (broadcastable)."""
    if len(a) == 2:
        return w[0] * a[0] + w[1] * a[1]
    v = a[1] + w[0] * (a[0] - a[1])
    v = v + w[2] * (a[2] - a[1])
    return v + w[3] * (a[3] - a[1])


def axis(n_in, n_out, mode):
    """-> (idx int64 [T, n_out], wt float32 [T, n_out]) of one axis: T = 1, 2, 4 taps for modes 0, 1, 2."""
    d = np.arange(n_out, dtype=np.int64)
    if mode == 0:
        idx = np.minimum(((2 * d + 1) * n_in) // (2 * n_out), n_in - 1)
        return idx[None], np.ones((1, n_out), dtype=f32)
    s = f32(n_in) / f32(n_out)
    c = d.astype(f32) + f32(0.5)
    c = c * s
    c = c - f32(0.5)
    assert c.dtype == f32
    if mode == 1:
        c = np.maximum(c, f32(0.0))
        i0 = np.minimum(c.astype(np.int64), n_in - 1)
        t = c - i0.astype(f32)
        return np.stack([i0, np.minimum(i0 + 1, n_in - 1)]), np.stack([f32(1.0) - t, t])
    if mode == 2:
        fl = np.floor(c)
        i = fl.astype(np.int64)
        t = c - fl
        u = f32(1.0) - t
        idx = np.stack([np.clip(i - 1 + k, 0, n_in - 1) for k in range(4)])
        wt = np.stack([_keys_outer(t, u), np.ones_like(t), _keys_inner(t, u), _keys_outer(u, t)])      # (w_1 is not read)
        assert wt.dtype == f32
        return idx, wt
    raise ValueError(f"mode must be 0, 1 or 2, got {mode!r}")


def resize(x, H, W, mode):
    """x [..., h, w] float32 (torch CPU tensor or array) -> [..., H, W] float32 of the same kind.  mode: 0 | 1 | 2 or its name (MODES)."""
    mode = MODES.get(mode, mode)
    is_t = torch.is_tensor(x)
    a = x.detach().cpu().numpy() if is_t else np.asarray(x)
    assert a.dtype == f32
    h, w = a.shape[-2:]
    ix, wx = axis(w, W, mode)
    iy, wy = axis(h, H, mode)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == 0:
            out = a[..., iy[0][:, None], ix[0][None, :]]
        else:
            hs = []
            for r in range(len(iy)):
                rows = a[..., iy[r], :]                                   # [..., H, w]
                hs.append(_combine([rows[..., ix[k]] for k in range(len(ix))], wx))
            out = _combine(hs, [wy[r][:, None] for r in range(len(iy))])
    out = np.ascontiguousarray(out, dtype=f32)
    assert out.shape[-2:] == (H, W)
    return torch.from_numpy(out) if is_t else out


def second_pass(cfg, sd, lora, lora_scale, embeds, first, noise2, steps, *, H, W, mode, strength, size=None, guidance_scale=8.0):
    """The second pass of a hires render on the fp32 reference: img2img from resize(first [1, 4, h, w]) at [1, 4, H, W] with the noise `noise2`."""
    x0 = resize(first.float().cpu(), H, W, mode)
    return IR.sample_latents(cfg, sd, lora, lora_scale, embeds, noise2, steps, init_latents=x0, strength=strength, guidance_scale=guidance_scale, size=size)
