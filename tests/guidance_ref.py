"""Guidance rescale, guidance interval and a per-step guidance scale, restated for the tests of sampler.guidance_table, LatentSampler.sample(
guidance_scale=[...], guidance_rescale=, guidance_interval=) and the sdlt_guidance kernel.  Written from the papers, not from the package:

 * `rescale`: Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4, in the form diffusers publishes it as
   rescale_noise_cfg: std over everything but the batch axis (torch's default: unbiased), e_c * (std_pos / std_c), blended with weight phi;
 * `schedule_g`: Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval": the guidance scale inside (sigma_lo, sigma_hi], 1 outside;
 * `sample_loop`: tests/multistep_ref.sample_loop (Euler and DPM-Solver++ (2M)) with those two in its guidance line, in the dtype asked for.
`guidance` is the kernel's contract on CPU tensors: the two standard deviations in fp64 (rounded once to fp32), every other operation in fp32, one
rounding each, in the order include/sdlt_kernels.h writes them.  The GPU tests hold the kernel - whose statistics are fp32 sums - to it within a
measured bound; `emu_guidance` adds it to the emulated op table.
"""
import types

import numpy as np
import torch

from oracle import unet_ref as U
from tests import multistep_ref as MR
from tests import sde_ref as SR


def rescale(e_pos, e_c, phi):
    """rescale_noise_cfg(noise_cfg=e_c, noise_pred_text=e_pos, guidance_rescale=phi) on [n, ...] tensors, in their dtype."""
    dims = list(range(1, e_pos.dim()))
    std_pos = e_pos.std(dim=dims, keepdim=True)
    std_c = e_c.std(dim=dims, keepdim=True)
    rescaled = e_c * (std_pos / std_c)
    return phi * rescaled + (1 - phi) * e_c


def schedule_g(sig, g, interval):
    """sig [k] (the sigma of each step that runs), g: a number or k numbers -> list of k: g_i inside (lo, hi], 1 outside."""
    gs = [float(g)] * len(sig) if isinstance(g, (int, float)) else [float(v) for v in g]
    assert len(gs) == len(sig)
    if interval is not None:
        lo, hi = interval
        gs = [gi if lo < float(s) <= hi else 1.0 for gi, s in zip(gs, sig)]
    return gs


def guide(e_neg, e_pos, g, phi):
    """One step's prediction as the pipelines form it: g = 1 is the positive prediction alone (no guidance), otherwise CFG and - phi > 0 - its rescale."""
    if g == 1.0:
        return e_pos
    e_c = e_neg + g * (e_pos - e_neg)
    return rescale(e_pos, e_c, phi) if phi > 0.0 else e_c


def sample_loop(model, noise, steps, *, sampler="euler", sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0,
                guidance_rescale=0.0, guidance_interval=None, prediction_type="epsilon", dtype=torch.float64):
    """tests/multistep_ref.sample_loop with `guide` as its guidance line.  model(xin [2, 4, h, w], t) -> [2, 4, h, w]."""
    k, start, ts, sig = MR.schedule(steps, strength, sigmas)
    sig = sig.astype(np.float32).astype(np.float64)
    co = MR.coefficients(sig)
    gs = schedule_g(sig[:k], guidance_scale, guidance_interval)
    noise = noise.to(dtype)
    x0 = None if init_latents is None else init_latents.to(dtype)
    x = noise * float(sig[0]) if x0 is None else x0 + noise * float(sig[0])
    dprev = None
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((s * s + 1) ** 0.5), float(np.float32(t)))
        e = guide(out[0:1], out[1:2], gs[i], guidance_rescale)
        if sampler == "euler":
            d = e if prediction_type == "epsilon" else (x - MR.denoised(e, x, s, prediction_type)) / s
            x = x + d * (sn - s)
        else:
            D = MR.denoised(e, x, s, prediction_type)
            a, b, c = (float(v) for v in co[i])
            x = a * x + b * D + (c * dprev if c != 0.0 else 0.0)
            dprev = D
        if mask is not None:
            kk = x0 + noise * sn
            x = kk + mask.to(dtype) * (x - kk)
    return x


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, *, size=None, **kw):
    """The fp32 reference loop driven by the fp32 oracle UNet (tests/multistep_ref.sample_latents' conventions)."""
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
                           dtype=torch.float32, **kw)


# ---- the kernel's contract on the CPU -----------------------------------------------------------------------------------------------------
def guidance(eps, gtab, ctr, n):
    """sdlt_guidance on CPU tensors: eps fp32 [2n hw, 4] in place, gtab fp32 [rows, 4], ctr int32 (read only)."""
    assert eps.dtype == gtab.dtype == torch.float32 and not eps.is_cuda and eps.shape[1] == 4 and eps.shape[0] % (2 * n) == 0
    k = max(1, min(int(gtab[0, 0]), gtab.shape[0] - 1))
    i = max(0, min(int(ctr[0]), k - 1))
    g, phi = gtab[1 + i, 0], gtab[1 + i, 1]
    e = eps.view(n, 2, -1)
    en, ep = e[:, 0], e[:, 1]
    if float(g) == 1.0 and float(phi) == 0.0:
        out = ep.clone()
    else:
        out = en + g * (ep - en)
        if float(phi) != 0.0:
            ec = out
            s_pos = ep.double().std(dim=1).numpy().astype(np.float32)             # unbiased, about the mean, in fp64; rounded once
            s_c = ec.double().std(dim=1).numpy().astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(s_c == 0, np.float32(1.0), s_pos / s_c)              # (numpy's fp32 quotient: IEEE division)
            assert r.dtype == np.float32
            out = phi * (ec * torch.from_numpy(r)[:, None]) + (1 - phi) * ec
    assert out.dtype == torch.float32
    e[:, 0] = out
    e[:, 1] = out
    return eps


emu_guidance = types.ModuleType("emu_guidance")
emu_guidance.__dict__.update({k: v for k, v in vars(SR.emu_sde).items() if not k.startswith("__")})
emu_guidance.guidance = guidance
