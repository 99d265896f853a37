"""Adaptive projected guidance (Sadat et al. 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales") restated for the tests of
sampler.apg_table, LatentSampler.sample(apg=) and the sdlt_guidance_apg kernel.  Written from the published function, not from the package:

 * `published`: diffusers' normalized_guidance with its MomentumBuffer, on [n, ...] tensors in their dtype (the tests call it in fp64): the running
   average diff + momentum * previous, the norm clip diff * min(1, threshold / ||diff||), the projection on the normalised positive prediction,
   pred_cond + (g - 1) (orthogonal + eta parallel);
 * `guide`: one step's prediction as a pipeline forms it - g = 1 the positive prediction alone, otherwise `published` and, phi > 0, the rescale of
   tests/guidance_ref.py;
 * `sample_loop` / `sample_latents`: tests/guidance_ref.sample_loop's trajectory with `guide` as its guidance line (the oracle UNet drives it).
`guidance_apg` is the kernel's contract on CPU tensors: the three sums and the two standard deviations in fp64 (each rounded once to fp32), every other
operation in fp32, one rounding each, in the order include/sdlt_kernels.h writes them.  The GPU tests hold the kernel - whose sums are fp32 in a fixed
order - to it within a measured bound; `emu_apg` adds it to the emulated op table, `with_apg` to any other.
"""
import types

import numpy as np
import torch

from oracle import unet_ref as U
from tests import guidance_ref as GR
from tests import multistep_ref as MR


def published(e_pos, e_neg, g, eta, tau, beta, m_prev=None):
    """normalized_guidance(pred_cond=e_pos, pred_uncond=e_neg, guidance_scale=g, momentum_buffer, eta, norm_threshold=tau) -> (prediction, running
    average).  m_prev None: a fresh MomentumBuffer (its running average starts at 0).  beta == 0: no buffer."""
    dims = list(range(1, e_pos.dim()))
    diff = e_pos - e_neg
    if beta != 0.0:
        diff = diff + beta * (torch.zeros_like(diff) if m_prev is None else m_prev)      # MomentumBuffer.update
    m = diff
    if tau > 0.0:
        norm = (diff * diff).sum(dim=dims, keepdim=True).sqrt()
        diff = diff * torch.minimum(torch.ones_like(norm), tau / norm)
    v1 = e_pos / (e_pos * e_pos).sum(dim=dims, keepdim=True).sqrt().clamp_min(1e-12)     # torch.nn.functional.normalize
    par = (diff * v1).sum(dim=dims, keepdim=True) * v1
    orth = diff - par
    return e_pos + (g - 1.0) * (orth + eta * par), m


def guide(e_neg, e_pos, g, phi, apg, m_prev):
    """-> (prediction, running average).  apg = (eta, tau, beta).  A step with g = 1 passes e_pos through and leaves the running average alone."""
    if g == 1.0:
        return e_pos, m_prev
    eta, tau, beta = apg
    e_c, m = published(e_pos, e_neg, g, eta, tau, beta, m_prev)
    return (GR.rescale(e_pos, e_c, phi) if phi > 0.0 else e_c), (m if beta != 0.0 else m_prev)


def sample_loop(model, noise, steps, *, apg, sampler="euler", sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0,
                guidance_rescale=0.0, guidance_interval=None, prediction_type="epsilon", dtype=torch.float64):
    """tests/guidance_ref.sample_loop with `guide` above as its guidance line.  apg: (eta, tau, beta), the fp32 values the table holds."""
    k, start, ts, sig = MR.schedule(steps, strength, sigmas)
    sig = sig.astype(np.float32).astype(np.float64)
    co = MR.coefficients(sig)
    gs = GR.schedule_g(sig[:k], guidance_scale, guidance_interval)
    noise = noise.to(dtype)
    x0 = None if init_latents is None else init_latents.to(dtype)
    x = noise * float(sig[0]) if x0 is None else x0 + noise * float(sig[0])
    dprev = m = None
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((s * s + 1) ** 0.5), float(np.float32(t)))
        e, m = guide(out[0:1], out[1:2], gs[i], guidance_rescale, apg, m)
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
    """The fp32 reference loop driven by the fp32 oracle UNet (tests/guidance_ref.sample_latents' conventions)."""
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
def scalars(d, ep, tau):
    """(c, a) of the contract per image, fp32 numpy [n]: the three sums in fp64 from the fp32 values, each rounded once; the rest in fp32."""
    f = lambda t: t.numpy().astype(np.float32)  # noqa: E731
    s_dd, s_dp, s_pp = f((d.double() * d.double()).sum(1)), f((d.double() * ep.double()).sum(1)), f((ep.double() * ep.double()).sum(1))
    tau = np.float32(tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where((tau > 0) & (s_dd != 0), np.minimum(np.float32(1.0), tau / np.sqrt(s_dd)), np.float32(1.0)).astype(np.float32)
        a = np.where(s_pp == 0, np.float32(0.0), (c * s_dp) / s_pp).astype(np.float32)
    return c, a


def guidance_apg(eps, gtab, atab, mom, ctr, n):
    """sdlt_guidance_apg on CPU tensors: eps fp32 [2n hw, 4] and mom fp32 [n hw, 4] (or None) in place, gtab / atab fp32 [rows, 4], ctr int32 (read only)."""
    assert eps.dtype == gtab.dtype == atab.dtype == torch.float32 and not eps.is_cuda and eps.shape[1] == 4 and eps.shape[0] % (2 * n) == 0
    assert tuple(atab.shape) == tuple(gtab.shape) and (mom is None or (mom.dtype == torch.float32 and tuple(mom.shape) == (eps.shape[0] // 2, 4)))
    k = max(1, min(int(gtab[0, 0]), gtab.shape[0] - 1))
    i = max(0, min(int(ctr[0]), k - 1))
    g, phi = gtab[1 + i, 0], gtab[1 + i, 1]
    eta, tau, beta = atab[1 + i, 0], atab[1 + i, 1], atab[1 + i, 2]
    e = eps.view(n, 2, -1)
    en, ep = e[:, 0], e[:, 1]
    if float(g) == 1.0:
        out = ep.clone()
    else:
        d = ep - en
        if float(beta) != 0.0 and mom is not None:
            mv = mom.view(n, -1)
            d = d + beta * (torch.zeros_like(d) if i == 0 else mv)                # (row 0 does not read the buffer)
            mv.copy_(d)
        c, a = (torch.from_numpy(v)[:, None] for v in scalars(d, ep, float(tau)))
        d = c * d
        par = a * ep
        orth = d - par
        out = ep + (g - 1.0) * (orth + eta * par)
        if float(phi) != 0.0:
            ec = out
            s_pos = ep.double().std(dim=1).numpy().astype(np.float32)             # unbiased, about the mean, in fp64; rounded once
            s_c = ec.double().std(dim=1).numpy().astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(s_c == 0, np.float32(1.0), s_pos / s_c)
            assert r.dtype == np.float32
            out = phi * (ec * torch.from_numpy(r)[:, None]) + (1 - phi) * ec
    assert out.dtype == torch.float32
    e[:, 0] = out
    e[:, 1] = out
    return eps


def with_apg(table, name):
    """`table` (an emulated op table) plus the emulated guidance_apg."""
    m = types.ModuleType(name)
    m.__dict__.update({k: v for k, v in vars(table).items() if not k.startswith("__")})
    m.guidance_apg = guidance_apg
    return m


emu_apg = with_apg(GR.emu_guidance, "emu_apg")
