"""Dynamic thresholding (the "Dynamic Thresholding (CFG scale fix)" extension of A1111 / ComfyUI / SwarmUI in its default mode - per channel, "AD"
variability, "MEAN" start point - a latent-space form of Imagen's dynamic thresholding) restated for the tests of sampler.dyn_table,
LatentSampler.sample(dynthresh=) and the sdlt_guidance_dyn kernel.  Written from the contract of include/sdlt_kernels.h, not from the package:

 * `published`: the mathematics in the tensors' dtype (the tests call it in fp64) on [n, C, ...] tensors, with torch.quantile as the quantile;
 * `guide`: one step's prediction - g = 1 the positive prediction alone, otherwise `published`;
 * `sample_loop` / `sample_latents`: tests/guidance_ref.sample_loop's trajectory with `guide` as its guidance line (the oracle UNet drives it).
`contract` is the kernel's contract on CPU tensors in fp32 numpy: the two means' sums in fp64 (each rounded once to fp32), every other operation in fp32,
one rounding each, in the header's order; the two order statistics from a full sort.  `parts` gives its per-channel scalars.  The GPU tests hold the
kernel to it - bit for bit where every fp32 sum is exact, within a measured bound elsewhere; `emu_dyn` adds it to the emulated op table, `with_dyn` to
any other.
"""
import types

import numpy as np
import torch

from oracle import unet_ref as U
from tests import guidance_ref as GR
from tests import multistep_ref as MR

F = np.float32


def published(e_pos, e_neg, g, mimic, q, psi):
    """[n, C, ...] -> [n, C, ...]: per image and channel over everything else.  g, mimic, q, psi: Python floats (the fp32 values the tables hold)."""
    shape = e_pos.shape
    ep, en = e_pos.flatten(2), e_neg.flatten(2)
    d = ep - en
    eg, em = en + g * d, en + mimic * d
    mu_g, mu_m = eg.mean(2, keepdim=True), em.mean(2, keepdim=True)
    cg, cm = eg - mu_g, em - mu_m
    A = cm.abs().amax(2, keepdim=True)
    Q = torch.quantile(cg.abs(), q, dim=2, keepdim=True)
    S = torch.maximum(A, Q)
    safe = torch.where(S == 0, torch.ones_like(S), S)
    ed = torch.where(S == 0, eg, torch.minimum(torch.maximum(cg, -S), S) / safe * A + mu_g)
    return (psi * ed + (1.0 - psi) * eg).reshape(shape)


def guide(e_neg, e_pos, g, dyn):
    """A step with g = 1 passes e_pos through.  dyn = (mimic, q, psi)."""
    return e_pos if g == 1.0 else published(e_pos, e_neg, g, *dyn)


def sample_loop(model, noise, steps, *, dyn, sampler="euler", sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0,
                guidance_interval=None, prediction_type="epsilon", dtype=torch.float64):
    """tests/guidance_ref.sample_loop with `guide` above as its guidance line.  dyn: (mimic, q, psi), the fp32 values the table holds; None: plain guidance."""
    k, start, ts, sig = MR.schedule(steps, strength, sigmas)
    sig = sig.astype(np.float32).astype(np.float64)
    co = MR.coefficients(sig)
    gs = GR.schedule_g(sig[:k], guidance_scale, guidance_interval)
    noise = noise.to(dtype)
    x0 = None if init_latents is None else init_latents.to(dtype)
    x = noise * float(sig[0]) if x0 is None else x0 + noise * float(sig[0])
    dprev = None
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((s * s + 1) ** 0.5), float(np.float32(t)))
        e = GR.guide(out[0:1], out[1:2], gs[i], 0.0) if dyn is None else guide(out[0:1], out[1:2], gs[i], dyn)
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


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, *, size=None, dtype=torch.float64, **kw):
    """The reference loop driven by the oracle UNet (tests/guidance_ref.sample_latents' conventions).  The oracle UNet is an fp32 restatement: it takes
    the model input rounded to fp32 and its prediction enters the loop - the guidance line with its quantile, the step - in `dtype`."""
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    h, w = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    with torch.no_grad():
        return sample_loop(lambda xin, t: U.unet_forward(cfg, sd, xin.float(), torch.tensor([t] * 2, dtype=torch.float32), ctx, add, lora=lora_s).to(dtype),
                           noise, steps, dtype=dtype, **kw)


# ---- the kernel's contract on the CPU -----------------------------------------------------------------------------------------------------
def ranks(q, hw):
    """(lo, hi, w) of the contract: pos = q (float)(hw - 1) in fp32."""
    pos = F(q) * F(hw - 1)
    lo = min(int(np.floor(pos)), hw - 1)
    hi = min(lo + 1, hw - 1)
    return lo, hi, F(pos - F(lo))


def parts(en, ep, g, mimic, q):
    """en, ep fp32 numpy [n, hw, 4]; g, mimic, q fp32 scalars -> dict of e_g, c_g [n, hw, 4] and mu_g, A, v_lo, v_hi, Q, S [n, 1, 4], all fp32."""
    hw = en.shape[1]
    d = ep - en
    eg, em = en + g * d, en + mimic * d
    mean = lambda v: (v.astype(np.float64).sum(1, keepdims=True).astype(F) / F(hw)).astype(F)  # noqa: E731  (the sum in fp64, rounded once; the quotient in fp32)
    mu_g, mu_m = mean(eg), mean(em)
    cg, cm = eg - mu_g, em - mu_m
    A = np.abs(cm).max(1, keepdims=True)
    lo, hi, w = ranks(q, hw)
    srt = np.sort(np.abs(cg), axis=1)
    v_lo, v_hi = srt[:, lo:lo + 1], srt[:, hi:hi + 1]
    Q = v_lo + w * (v_hi - v_lo)
    out = dict(eg=eg, cg=cg, mu_g=mu_g, A=A, v_lo=v_lo, v_hi=v_hi, Q=Q, S=np.maximum(A, Q))
    assert all(v.dtype == F for v in out.values())
    return out


def contract(eps, gtab, dtab, ctr, n):
    """sdlt_guidance_dyn on CPU tensors: eps fp32 [2n hw, 4] in place, gtab / dtab fp32 [rows, 4], ctr int32 (read only)."""
    assert eps.dtype == gtab.dtype == dtab.dtype == torch.float32 and not eps.is_cuda and eps.shape[1] == 4 and eps.shape[0] % (2 * n) == 0
    assert tuple(dtab.shape) == tuple(gtab.shape) and eps.is_contiguous()
    k = max(1, min(int(gtab[0, 0]), gtab.shape[0] - 1))
    i = max(0, min(int(ctr[0]), k - 1))
    g = F(gtab[1 + i, 0])
    mimic, q, psi = (F(v) for v in dtab[1 + i, :3])
    e = eps.view(n, 2, -1, 4).numpy()                                            # (shares eps's memory)
    en, ep = e[:, 0].copy(), e[:, 1].copy()
    if g == 1.0:
        out = ep
    else:
        p = parts(en, ep, g, mimic, q)
        S, A, cg, eg = p["S"], p["A"], p["cg"], p["eg"]
        with np.errstate(divide="ignore", invalid="ignore"):
            ed = ((np.minimum(np.maximum(cg, -S), S) / S) * A) + p["mu_g"]
        ed = np.where(S == 0, eg, ed)
        out = ed if psi == 1.0 else psi * ed + (F(1.0) - psi) * eg
    assert out.dtype == F
    e[:, 0] = out
    e[:, 1] = out
    return eps


def with_dyn(table, name):
    """`table` (an emulated op table) plus the emulated guidance_dyn."""
    m = types.ModuleType(name)
    m.__dict__.update({k: v for k, v in vars(table).items() if not k.startswith("__")})
    m.guidance_dyn = contract
    return m


emu_dyn = with_dyn(GR.emu_guidance, "emu_dyn")
