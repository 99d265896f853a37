"""DPM-Solver++ (2M) with trailing or Karras noise levels, restated for the tests of sampler.DpmSolverPP2M, sampler.step_table_ms,
LatentSampler.sample(sampler=, sigmas=) and the sdlt_sampler_step_ms kernel.  Written from the papers, not from the package:

 * Lu et al. 2022, DPM-Solver++, algorithm 2 (multistep, second order), data prediction, in the variance-exploding form the sampler uses (alpha = 1,
   lambda = -log sigma):  x_{i+1} = (sigma_{i+1} / sigma_i) x - (exp(-h) - 1) D',  D' = (1 + 1 / (2 r)) D_i - (1 / (2 r)) D_{i-1},  h = lambda_{i+1} -
   lambda_i,  r = h_{i-1} / h;  D' = D_i on the first step that runs and on a step to sigma = 0;
 * Karras et al. 2022, eq. 5 with rho = 7, between the sigmas of training timesteps 999 and 0; the model is called at the fractional timestep at which
   log sigma_t, linear between integer timesteps, takes the level's value;
 * img2img and the mask as tests/img2img_ref.py: the last k = min(int(steps * strength), steps) levels, x = x0 + noise * sigma_start, and after every
   step k = x0 + noise * sigma_next, x = k + m (x - k).

`sample_loop` runs in the dtype asked for (float64: the reference of the CPU tests; float32: the loop the GPU path is compared with, driven by the
oracle UNet).  `sampler_step_ms` is the kernel's contract evaluated by torch on the CPU, fp32, one rounding per operation, in the order
include/sdlt_kernels.h writes them (IEEE division and square root): the GPU tests compare bits with it, and `emu_ms` (tests/emu_ops.py plus the three
sampler kernels) lets the CPU tests run the fused path.
"""
import math
import types

import numpy as np
import torch

from oracle import loss_ref as L
from oracle import unet_ref as U
from tests import img2img_ref as IR

RHO = 7.0


def sigmas_all(T=1000):
    acp = L.ddpm_alphas_cumprod(T).double().numpy()
    return ((1 - acp) / acp) ** 0.5


def schedule(steps, strength=1.0, sigmas="trailing", T=1000):
    """-> (k, start, timesteps float64 [k], sigmas float64 [k + 1] with the final 0)."""
    k = min(int(steps * strength), steps)
    if not (0.0 < strength <= 1.0) or k < 1:
        raise ValueError((steps, strength))
    sa = sigmas_all(T)
    if sigmas == "trailing":
        ts = np.round(np.arange(T, 0, -T / steps)) - 1
        sig = np.interp(ts, np.arange(T), sa)
    else:
        assert sigmas == "karras"
        lo, hi = sa[0] ** (1 / RHO), sa[T - 1] ** (1 / RHO)
        sig = np.array([(hi + (i / max(steps - 1, 1)) * (lo - hi)) ** RHO for i in range(steps)])
        ts = np.zeros(steps)
        for j, s in enumerate(sig):                                           # fractional timestep: log sigma linear between integer timesteps
            t = int(np.clip(np.searchsorted(sa, s, side="right") - 1, 0, T - 2))
            w = (math.log(s) - math.log(sa[t])) / (math.log(sa[t + 1]) - math.log(sa[t]))
            ts[j] = t + min(max(w, 0.0), 1.0)
    start = steps - k
    return k, start, ts[start:], np.concatenate([sig[start:], [0.0]])


def coefficients(sig):
    """(a, b, c) per step with x_{i+1} = a x + b D_i + c D_{i-1}, from the paper's form: a = exp(-h), b = -(exp(-h) - 1)(1 + 1 / (2 r)), c = (exp(-h) - 1) / (2 r)."""
    sig = np.asarray(sig, dtype=np.float64)
    out, h_prev = [], None
    for i in range(len(sig) - 1):
        if sig[i + 1] == 0.0:
            out.append((0.0, 1.0, 0.0))                                       # h = infinity: exp(-h) = 0, first order
            h_prev = None
            continue
        h = math.log(sig[i]) - math.log(sig[i + 1])
        phi = -math.expm1(-h)
        if h_prev is None:
            out.append((math.exp(-h), phi, 0.0))
        else:
            r = h_prev / h
            out.append((math.exp(-h), phi * (1 + 1 / (2 * r)), -phi / (2 * r)))
        h_prev = h
    return np.array(out)


def denoised(e, x, s, prediction_type):
    if prediction_type == "epsilon":
        return x - e * s
    return e * (-s / (s * s + 1) ** 0.5) + x / (s * s + 1)


def sample_loop(model, noise, steps, *, sampler="dpmpp_2m", sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0,
                prediction_type="epsilon", dtype=torch.float64):
    """model(xin [2, 4, h, w] (negative | positive rows), t float) -> [2, 4, h, w].  noise, init_latents [1, 4, h, w]; mask [1, 1, h, w] | None.
    The noise levels are the fp32 roundings of the schedule (what the package stores); everything after that is `dtype`."""
    k, start, ts, sig = schedule(steps, strength, sigmas)
    sig = sig.astype(np.float32).astype(np.float64)
    co = coefficients(sig)
    noise = noise.to(dtype)
    x0 = None if init_latents is None else init_latents.to(dtype)
    x = noise * float(sig[0]) if x0 is None else x0 + noise * float(sig[0])
    dprev = None
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((s * s + 1) ** 0.5), float(np.float32(t)))
        e = out[0:1] + guidance_scale * (out[1:2] - out[0:1])
        if sampler == "euler":
            d = e if prediction_type == "epsilon" else (x - denoised(e, x, s, prediction_type)) / s
            x = x + d * (sn - s)
        else:
            D = denoised(e, x, s, prediction_type)
            a, b, c = (float(v) for v in co[i])
            x = a * x + b * D + (c * dprev if c != 0.0 else 0.0)
            dprev = D
        if mask is not None:
            kk = x0 + noise * sn
            x = kk + mask.to(dtype) * (x - kk)
    return x


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, *, sampler="dpmpp_2m", sigmas="trailing", init_latents=None, strength=1.0, mask=None,
                   guidance_scale=8.0, size=None, prediction_type="epsilon"):
    """The fp32 reference loop driven by the fp32 oracle UNet (oracle.sampler_ref.sample_latents' conventions, adapters weighted by lora_scale)."""
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    h, w = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    with torch.no_grad():
        return sample_loop(lambda xin, t: U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2, dtype=torch.float32), ctx, add, lora=lora_s), noise, steps,
                           sampler=sampler, sigmas=sigmas, init_latents=init_latents, strength=strength, mask=mask, guidance_scale=guidance_scale,
                           prediction_type=prediction_type, dtype=torch.float32)


# ---- the kernel's contract on the CPU -----------------------------------------------------------------------------------------------------
def sampler_step_ms(eps, x, xin, timesteps, table, ctr, *, dprev, x0=None, noise=None, mask=None, init=False):
    """sdlt_sampler_step_ms on CPU tensors (x, dprev fp32 [n, 4, h, w] in place; table fp32 [rows, 8]; ctr int32 [2])."""
    assert x.dtype == table.dtype == dprev.dtype == torch.float32 and not x.is_cuda and table.shape[1] == 8
    n, _, h, w = x.shape
    steps = max(1, min(int(table[1, 0]), table.shape[0] - 2))
    if init:
        v = noise * table[0, 1]
        x.copy_(v if x0 is None else x0 + v)
        inv, tn, nxt = table[0, 2], table[0, 3], 0
    else:
        i = max(0, min(int(ctr[0]), steps - 1))
        g, (s, sn, inv, tn, a, b, c, _) = table[0, 0], table[2 + i]
        e4 = eps.view(n, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        e = e4[:, 0] + g * (e4[:, 1] - e4[:, 0])
        if float(table[1, 1]) != 0.0:
            # torch divides a CPU tensor by a one-element operand as a product with its reciprocal (two roundings): the scalar quotient is
            # taken in numpy's float32 and the element-wise divisor is a full tensor, so that every division is IEEE's
            s32 = np.float32(float(s))
            q = s32 * s32 + np.float32(1.0)
            c1 = -s32 / np.sqrt(q)
            assert q.dtype == c1.dtype == np.float32
            D = e * float(c1) + x / torch.full_like(x, float(q))
        else:
            D = x - s * e
        xn = a * x + b * D
        if float(c) != 0.0:
            xn = xn + c * dprev
        if mask is not None:
            k = x0 + noise * sn
            xn = k + mask * (xn - k)
        x.copy_(xn)
        dprev.copy_(D)
        nxt = 0 if i + 1 >= steps else i + 1
    IR._repack(x, inv, xin, timesteps, tn, n, h, w)
    ctr[0], ctr[1] = nxt, 0
    return x


emu_ms = types.ModuleType("emu_ms")
emu_ms.__dict__.update({k: v for k, v in vars(IR.emu_img).items() if not k.startswith("__")})
emu_ms.sampler_step_ms = sampler_step_ms
