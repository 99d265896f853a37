"""Plain-torch fp32 restatement of sampling from an init image (img2img) and of masked inpainting, for the tests of sampler.LatentSampler.sample(
init_latents=, strength=, mask=) and of the sdlt_sampler_step_img kernel.  Written from the algorithm:

 * schedule: diffusers' img2img rule (StableDiffusionImg2ImgPipeline.get_timesteps): k = min(int(steps * strength), steps), the trajectory is the
   LAST k entries of the `steps`-entry Euler-trailing schedule;
 * init: x = x0 + noise * sigma of the first kept entry (EulerDiscreteScheduler.add_noise);
 * per step: the Euler update, then - with a mask (1 regenerate, 0 keep) - the known region put back, noised to the sigma the step arrived at with
   the SAME noise: k = x0 + noise * sigma_next, x = k + m (x - k).  After the last step sigma_next = 0: kept pixels are x0 exactly.

`sampler_step_img` is the kernel's contract evaluated in torch on the CPU, fp32, one rounding per operation, in the order include/sdlt_kernels.h
writes them (IEEE division and square root): the GPU tests compare bits with it, and `emu_img` (tests/emu_ops.py plus the two sampler kernels)
lets the CPU tests run the fused path.
"""
import types

import numpy as np
import torch

from oracle import loss_ref as L
from oracle import unet_ref as U
from tests import emu_ops


def schedule(steps, strength, T=1000):
    """-> (k, start, timesteps int64 [k], sigmas float64 [k + 1] with the final 0)."""
    k = min(int(steps * strength), steps)
    if not (0.0 < strength <= 1.0) or k < 1:
        raise ValueError((steps, strength))
    acp = L.ddpm_alphas_cumprod(T).double().numpy()
    sig_all = ((1 - acp) / acp) ** 0.5
    ts = np.round(np.arange(T, 0, -T / steps)).astype(np.int64) - 1          # "trailing"
    sig = np.interp(ts, np.arange(T), sig_all)
    start = steps - k
    return k, start, ts[start:], np.concatenate([sig[start:], [0.0]])


def sample_loop(model, noise, steps, *, init_latents, strength, mask=None, guidance_scale=8.0, prediction_type="epsilon"):
    """model(xin [2, 4, h, w] (negative | positive rows), t int) -> [2, 4, h, w].  noise, init_latents [1, 4, h, w]; mask [1, 1, h, w] | None."""
    k, start, ts, sig = schedule(steps, strength)
    sig = sig.astype(np.float32)
    x0, noise = init_latents.float(), noise.float()
    x = x0 + noise * float(sig[0])
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((np.float64(sig[i]) ** 2 + 1) ** 0.5), int(t))
        e = out[0:1] + guidance_scale * (out[1:2] - out[0:1])
        if prediction_type == "epsilon":
            d = e
        else:
            d = (x - (e * (-s / (s * s + 1) ** 0.5) + x / (s * s + 1))) / s
        x = x + d * (sn - s)
        if mask is not None:
            kk = x0 + noise * sn
            x = kk + mask.float() * (x - kk)
    return x


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, *, init_latents, strength, mask=None, guidance_scale=8.0, size=None,
                   prediction_type="epsilon"):
    """oracle.sampler_ref.sample_latents' conventions (fp32 oracle UNet, adapters weighted by lora_scale), from init latents."""
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    h, w = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    with torch.no_grad():
        return sample_loop(lambda xin, t: U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2), ctx, add, lora=lora_s), noise, steps,
                           init_latents=init_latents, strength=strength, mask=mask, guidance_scale=guidance_scale, prediction_type=prediction_type)


# ---- the kernels' contract on the CPU -----------------------------------------------------------------------------------------------------
def _repack(x, inv, xin, timesteps, tn, n, h, w):
    v = (x * inv).permute(0, 2, 3, 1).reshape(n, 1, h * w, 4).expand(n, 2, h * w, 4).reshape(2 * n * h * w, 4)
    xin[:, :4] = v.to(xin.dtype)
    timesteps[: 2 * n] = tn


def sampler_step_img(eps, x, xin, timesteps, table, ctr, *, x0, noise, mask=None, init=False):
    """sdlt_sampler_step_img on CPU tensors (x fp32 [n, 4, h, w] in place; table fp32 [rows, 4]; ctr int32 [2])."""
    assert x.dtype == table.dtype == x0.dtype == noise.dtype == torch.float32 and not x.is_cuda
    n, _, h, w = x.shape
    steps = max(1, min(int(table[1, 0]), table.shape[0] - 2))
    if init:
        x.copy_(x0 + noise * table[0, 1])
        inv, tn, nxt = table[0, 2], table[0, 3], 0
    else:
        i = max(0, min(int(ctr[0]), steps - 1))
        g, (s, sn, inv, tn) = table[0, 0], table[2 + i]
        e4 = eps.view(n, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        d = e4[:, 0] + g * (e4[:, 1] - e4[:, 0])
        if float(table[1, 1]) != 0.0:
            # torch divides a CPU tensor by a one-element operand as a product with its reciprocal (two roundings): the scalar quotient is
            # taken in numpy's float32 and the element-wise divisors are full tensors, so that every division is IEEE's
            s32 = np.float32(float(s))
            q = s32 * s32 + np.float32(1.0)
            c1 = -s32 / np.sqrt(q)
            assert q.dtype == c1.dtype == np.float32
            d = (x - (d * float(c1) + x / torch.full_like(x, float(q)))) / torch.full_like(x, float(s32))
        xn = x + d * (sn - s)
        if mask is not None:
            k = x0 + noise * sn
            xn = k + mask * (xn - k)
        x.copy_(xn)
        nxt = 0 if i + 1 >= steps else i + 1
    _repack(x, inv, xin, timesteps, tn, n, h, w)
    ctr[0], ctr[1] = nxt, 0
    return x


def sampler_step(eps, x, xin, timesteps, table, ctr, *, noise=None):
    """sdlt_sampler_step on CPU tensors (the txt2img launch: a captured txt2img iteration must not be disturbed by an img2img one)."""
    n, _, h, w = x.shape
    if noise is not None:
        x.copy_(noise * table[0, 1])
        _repack(x, table[0, 2], xin, timesteps, table[0, 3], n, h, w)
        ctr[0], ctr[1] = 0, 0
        return x
    return sampler_step_img(eps, x, xin, timesteps, table, ctr, x0=x, noise=x)


emu_img = types.ModuleType("emu_img")
emu_img.__dict__.update({k: v for k, v in vars(emu_ops).items() if not k.startswith("__")})
emu_img.sampler_step = sampler_step
emu_img.sampler_step_img = sampler_step_img
