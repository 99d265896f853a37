"""sdlt_blur_planes restated in torch fp32 on the CPU, for tests/test_blur_gpu.py and the emulated op table of the CPU tests: a separable Gaussian
with replicated edges, rows then columns, each output the sum over the taps from -R to +R IN THAT ORDER, started from the first product, one multiply
and one add per tap, each rounded once (full-tensor operands: every operation is one IEEE fp32 operation per element).  The taps come from
ops.blur_taps; `taps64` restates them in NumPy for the test of that function."""
import numpy as np
import torch


def taps64(sigma):
    """-> (R, float64 [2 R + 1]): the normalised weights before the one rounding to fp32."""
    R = min(int(np.ceil(3.0 * sigma)), 64)
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * sigma * sigma))
    return R, w / w.sum()


def _pass(v, taps, axis):
    R, n = taps.numel() // 2, v.shape[axis]
    idx, acc = torch.arange(n), None
    for t in range(-R, R + 1):
        pr = v.index_select(axis, (idx + t).clamp(0, n - 1)) * float(taps[t + R])      # (a Python float that is an fp32 value: one fp32 multiply)
        acc = pr if acc is None else acc + pr
    return acc


def blur_planes(src, out, scratch, taps, clamp01=False):
    """ops.blur_planes on CPU tensors [.., h, w]: scratch = the row pass, out = the column pass (clamped to [0, 1] with clamp01)."""
    assert src.dtype == taps.dtype == torch.float32 and not src.is_cuda and src.shape == out.shape == scratch.shape
    scratch.copy_(_pass(src, taps, src.dim() - 1))
    res = _pass(scratch, taps, src.dim() - 2)
    out.copy_(res.clamp(0.0, 1.0) if clamp01 else res)
    return out
