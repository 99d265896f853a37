"""Differential diffusion (Levin & Fried 2023, "Giving Each Pixel Its Strength") restated for the tests of sampler.hold_map,
LatentSampler.sample(change_map=) and the sdlt_sampler_step_dd kernel.  Written from the algorithm:

 * `hold_rule`: the paper keeps a pixel before step i iff (1 - c) > i / k; for a select AFTER step row i (0-based, arriving at sigma_{i+1}) that is
   "held iff i + 1 < hold" with hold = ceil((1 - c) k), in NumPy fp64 from the fp32 map.  A product within k 2^-24 above an integer counts as the integer
   (an fp32 c is a real number known to 2^-25), and c == 0 is kept for good (hold = k + 1: after the last step sigma = 0 and the pixel is x0).
 * `sample_loop` / `sample_latents`: the fp32 Euler img2img loop of tests/img2img_ref.py with the select in place of the blend.
 * `sampler_step_dd`: the kernel's contract on CPU tensors - the form's own maskless step (tests/img2img_ref.py, multistep_ref.py, sde_ref.py: fp32,
   one rounding per operation, full-tensor divisors), then k = x0 + noise * sigma_next (one multiply, one add) SELECTED where (float)(i + 1) < hold, and
   the repack of what was selected.  `emu_dd` adds it, and tests/blur_ref.py's blur, to the emulated op table.
"""
import types

import numpy as np
import torch

from oracle import unet_ref as U
from tests import blur_ref as BR
from tests import img2img_ref as IR
from tests import multistep_ref as MR
from tests import sde_ref as SR


def hold_rule(c, k):
    """c: fp32 array in [0, 1] -> float64 array of the same shape."""
    c = np.asarray(c)
    assert c.dtype == np.float32
    c64 = c.astype(np.float64)
    return np.where(c64 == 0.0, float(k + 1), np.maximum(np.ceil((1.0 - c64) * k - k * 2.0 ** -24), 0.0))


def sample_loop(model, noise, steps, *, init_latents, strength, change_map, guidance_scale=8.0, prediction_type="epsilon"):
    """tests/img2img_ref.sample_loop with a change map [1, 1, h, w] instead of a mask."""
    k, start, ts, sig = IR.schedule(steps, strength)
    sig = sig.astype(np.float32)
    x0, noise = init_latents.float(), noise.float()
    hold = torch.from_numpy(hold_rule(change_map.numpy(), k))
    x = x0 + noise * float(sig[0])
    for i, t in enumerate(ts):
        s, sn = float(sig[i]), float(sig[i + 1])
        out = model(torch.cat([x, x], 0) / float((np.float64(sig[i]) ** 2 + 1) ** 0.5), int(t))
        e = out[0:1] + guidance_scale * (out[1:2] - out[0:1])
        d = e if prediction_type == "epsilon" else (x - (e * (-s / (s * s + 1) ** 0.5) + x / (s * s + 1))) / s
        x = x + d * (sn - s)
        x = torch.where(hold > i + 1, x0 + noise * sn, x)
    return x


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, *, init_latents, strength, change_map, guidance_scale=8.0, size=None,
                   prediction_type="epsilon"):
    """tests/img2img_ref.sample_latents' conventions (fp32 oracle UNet, adapters weighted by lora_scale)."""
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
                           init_latents=init_latents, strength=strength, change_map=change_map, guidance_scale=guidance_scale,
                           prediction_type=prediction_type)


# ---- the kernel's contract on the CPU -----------------------------------------------------------------------------------------------------
def sibling_step(form, eps, x, xin, timesteps, table, ctr, *, x0, noise, dprev=None, seeds=None, init=False, z=None):
    """The maskless step (or the init from x0) of the entry whose update `form` names, on CPU tensors."""
    if form == 0:
        return IR.sampler_step_img(eps, x, xin, timesteps, table, ctr, x0=x0, noise=noise, init=init)
    if form == 1:
        return MR.sampler_step_ms(eps, x, xin, timesteps, table, ctr, dprev=dprev, x0=x0, noise=noise, init=init)
    return SR.sampler_step_sde(eps, x, xin, timesteps, table, ctr, dprev=dprev, seeds=seeds, x0=x0, noise=noise, init=init, z=z)


def sampler_step_dd(eps, x, xin, timesteps, table, ctr, *, x0, noise, hold, form, dprev=None, seeds=None, init=False, z=None):
    """sdlt_sampler_step_dd on CPU tensors (x, dprev fp32 [n, 4, h, w] in place; hold fp32 [n, 1, h, w]; ctr int32 [2])."""
    assert form in (0, 1, 2) and table.shape[1] == (4 if form == 0 else 8) and x0 is not None and noise is not None
    n, _, h, w = x.shape
    if init:
        return sibling_step(form, None, x, xin, timesteps, table, ctr, x0=x0, noise=noise, dprev=dprev, seeds=seeds, init=True)
    assert hold.dtype == torch.float32 and tuple(hold.shape) == (n, 1, h, w)
    steps = max(1, min(int(table[1, 0]), table.shape[0] - 2))
    i = max(0, min(int(ctr[0]), steps - 1))                  # read before the step advances the counter
    sn, inv, tn = table[2 + i, 1], table[2 + i, 2], table[2 + i, 3]
    sibling_step(form, eps, x, xin, timesteps, table, ctr, x0=x0, noise=noise, dprev=dprev, seeds=seeds, z=z)
    k = x0 + noise * sn
    x.copy_(torch.where(hold > float(i + 1), k, x))
    IR._repack(x, inv, xin, timesteps, tn, n, h, w)
    return x


def _blur_taps(sigma):
    from sd_lora_trainer_amd import ops
    return ops.blur_taps(sigma)


emu_dd = types.ModuleType("emu_dd")
emu_dd.__dict__.update({k: v for k, v in vars(SR.emu_sde).items() if not k.startswith("__")})
emu_dd.sampler_step_dd = sampler_step_dd
emu_dd.blur_planes = BR.blur_planes
emu_dd.blur_taps = _blur_taps
