"""Key / value token downsampling restated in torch, fp32 on the CPU: the contract of sdlt_token_pool (include/sdlt_kernels.h) with explicit windows, its
emulation for the CPU op table (tests/emu_ops.py stays as it is: `emu_kv` is a copy of tests/img2img_ref.emu_img with the new op and the restated
resize of the hires pass), and a self-attention block with pooled keys and values - softmax(q k_pool^T / sqrt(d)) v_pool, to_out, the residual."""
import math
import types

import torch
import torch.nn.functional as F

from tests import hires_ref as HR
from tests import img2img_ref as IR

MODES = ("nearest", "area")
BF = torch.bfloat16


def token_pool_rows(H, W, f):
    """(Ho, Wo, Nk, Nkp): ceil division, Nk = Ho Wo, Nkp = Nk rounded up to 8 (the attention forward's rule for the keys' rows per image)."""
    Ho, Wo = -(-H // f), -(-W // f)
    return Ho, Wo, Ho * Wo, (Ho * Wo + 7) // 8 * 8


def layernorm_rows(x, gamma, beta, eps):
    xf = x.float()
    mean = xf.mean(1, keepdim=True)
    var = ((xf - mean) ** 2).mean(1, keepdim=True)
    return (xf - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float()


def token_pool_ref(x, *, B, H, W, gamma, beta, eps, f, mode):
    """fp32 [B Nkp, C]: window by window; the pad rows are zero."""
    mode = MODES[mode] if isinstance(mode, int) else mode
    assert mode in MODES and 1 <= f <= min(H, W) and x.shape[0] == B * H * W
    C = x.shape[1]
    ln = layernorm_rows(x, gamma, beta, eps).view(B, H, W, C)
    Ho, Wo, Nk, Nkp = token_pool_rows(H, W, f)
    out = torch.zeros(B, Nkp, C)
    for oy in range(Ho):
        for ox in range(Wo):
            if mode == "nearest":
                out[:, oy * Wo + ox] = ln[:, oy * f, ox * f]
            else:
                win = ln[:, oy * f: min(H, oy * f + f), ox * f: min(W, ox * f + f)].reshape(B, -1, C)
                acc = torch.zeros(B, C)
                for r in range(win.shape[1]):          # (r, c) order, as the kernel adds them
                    acc = acc + win[:, r]
                out[:, oy * Wo + ox] = acc / win.shape[1]
    return out.view(B * Nkp, C)


def token_pool_torch(x, *, B, H, W, gamma, beta, eps, f, mode):
    """The same through torch's own operators (valid rows only, fp32 [B, Nk, C]): F.layer_norm -> NHWC view -> [::f, ::f] or avg_pool2d."""
    C = x.shape[1]
    ln = F.layer_norm(x.float(), (C,), gamma.float(), beta.float(), eps).view(B, H, W, C)
    if mode in ("nearest", 0):
        return ln[:, ::f, ::f].reshape(B, -1, C)
    return F.avg_pool2d(ln.permute(0, 3, 1, 2), f, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1).reshape(B, -1, C)


def token_pool(x, y, *, B, H, W, gamma, beta, eps, f, mode):
    """ops.token_pool on the emulated table: the same argument checks, y written in its own dtype."""
    mode = MODES.index(mode) if mode in MODES else mode
    assert mode in (0, 1) and B >= 1 and 1 <= f <= min(H, W)
    Nkp = token_pool_rows(H, W, f)[3]
    assert x.shape[0] == B * H * W and tuple(y.shape) == (B * Nkp, x.shape[1]) and gamma.numel() == x.shape[1] == beta.numel()
    y.copy_(token_pool_ref(x, B=B, H=H, W=W, gamma=gamma, beta=beta, eps=eps, f=f, mode=mode).to(y.dtype))
    return y


def _resize_planes(src, out, mode):
    out.copy_(HR.resize(src, out.shape[2], out.shape[3], mode))
    return out


emu_kv = types.ModuleType("emu_kv")
emu_kv.__dict__.update({k: v for k, v in vars(IR.emu_img).items() if not k.startswith("__")})
emu_kv.token_pool, emu_kv.token_pool_rows, emu_kv.resize_planes = token_pool, token_pool_rows, _resize_planes


def attention_block(x, *, B, H, W, heads, f, mode, gamma, beta, eps, weights, adapters, scale, bias_out, act=BF):
    """residual + to_out(softmax(q k^T / sqrt(d)) v) of a self-attention block: q from every token of LayerNorm(x), k and v from the pooled tokens
    (f == 1: from every token).  weights: dict q, k, v, out -> [C, C]; adapters: the same keys -> (A [r, C], B [C, r]), y += scale (x A^T) B^T.
    fp32 arithmetic; the tensors the device keeps in `act` - the pooled rows, q, k, v, the attention output - are rounded to it where it stores them."""
    C = x.shape[1]
    d = C // heads
    rd = lambda t: t.to(act).float()  # noqa: E731

    def lin(t, name):
        A, Bm = adapters[name]
        return t @ weights[name].float().t() + scale * ((t @ A.float().t()) @ Bm.float().t())

    ln = layernorm_rows(x, gamma, beta, eps)
    if f == 1:
        pooled, Nk = rd(ln).view(B, H * W, C), H * W
    else:
        _, _, Nk, Nkp = token_pool_rows(H, W, f)
        pooled = rd(token_pool_ref(x, B=B, H=H, W=W, gamma=gamma, beta=beta, eps=eps, f=f, mode=mode)).view(B, Nkp, C)[:, :Nk]
    q = rd(lin(rd(ln), "q")).view(B, H * W, heads, d).permute(0, 2, 1, 3)
    k = rd(lin(pooled, "k")).view(B, Nk, heads, d).permute(0, 2, 1, 3)
    v = rd(lin(pooled, "v")).view(B, Nk, heads, d).permute(0, 2, 1, 3)
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1) @ v
    o = rd(o.permute(0, 2, 1, 3).reshape(B * H * W, C))
    return lin(o, "out") + bias_out.float() + x.float()
