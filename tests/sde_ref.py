"""The stochastic samplers - Euler ancestral and DPM-Solver++ (2M) SDE - restated for the tests of sampler.sde_coefficients, sampler.EulerAncestral /
DpmSolverPP2MSDE, sampler.step_table_sde, LatentSampler.sample(sampler="euler_a" | "dpmpp_2m_sde") and the sdlt_sampler_step_sde / sdlt_sampler_noise
kernels.  Written from the published algorithms, not from the package:

 * `ancestral_step` / `dpmpp_2m_sde_step`: the loops of k-diffusion's sample_euler_ancestral and sample_dpmpp_2m_sde (midpoint, s_noise = 1) in the form
   they are published in - sigma_up / sigma_down and the derivative d = (x - D) / sigma; t = -ln sigma, h, expm1 - step by step with the caller's z.
   They never form the package's (a, b, c, d).
 * `philox4x32_10` (Salmon et al. 2011; known answers of Random123 in tests/test_sde_cpu.py) and `noise`: the per-pixel noise the kernel defines,
   key = the image's (seed_lo, seed_hi), counter = (pixel, step row, 0, 0x53444531), u = ((word >> 9) + 0.5) 2^-23, Box-Muller - in fp64 from the
   exact u's.
 * `sampler_step_sde` / `sampler_noise`: the kernels' contract on CPU tensors, fp32, one rounding per operation, in the order include/sdlt_kernels.h
   writes them, as tests/multistep_ref.py restates sdlt_sampler_step_ms; `emu_sde` adds them to the emulated op table.
Schedules, img2img and the mask are tests/multistep_ref.py's.
"""
import math
import types

import numpy as np
import torch

from oracle import unet_ref as U
from tests import img2img_ref as IR
from tests import multistep_ref as MR


# ---- the published loops ------------------------------------------------------------------------------------------------------------------
def ancestral_step(x, D, s, sn, eta, z):
    """One iteration of sample_euler_ancestral: get_ancestral_step, the Euler step to sigma_down, then noise of sigma_up."""
    up = min(sn, eta * (sn ** 2 * (s ** 2 - sn ** 2) / s ** 2) ** 0.5)
    down = (sn ** 2 - up ** 2) ** 0.5
    d = (x - D) / s
    x = x + d * (down - s)
    if sn > 0:
        x = x + z * up
    return x


def dpmpp_2m_sde_step(x, D, s, sn, eta, z, state):
    """One iteration of sample_dpmpp_2m_sde, solver_type "midpoint"; state = dict(old=previous denoised | None, h_last)."""
    if sn == 0:
        x = D
    else:
        t, t_next = -math.log(s), -math.log(sn)
        h = t_next - t
        eta_h = eta * h
        x = sn / s * math.exp(-eta_h) * x + (-math.expm1(-h - eta_h)) * D
        if state.get("old") is not None:
            r = state["h_last"] / h
            x = x + 0.5 * (-math.expm1(-h - eta_h)) * (1 / r) * (D - state["old"])
        if eta:
            x = x + z * (sn * (-math.expm1(-2 * eta_h)) ** 0.5)
        state["h_last"] = h
    state["old"] = D
    return x


def published_loop(kind, denoise, x, sig, eta, zs, after=None):
    """x_0 -> x_k over the grid sig [k + 1] (floats); denoise(x, i) -> D_i; zs[i]: the noise of step i; after(x, i): the mask blend, if any."""
    state = {}
    for i in range(len(sig) - 1):
        s, sn = float(sig[i]), float(sig[i + 1])
        D = denoise(x, i)
        x = ancestral_step(x, D, s, sn, eta, zs[i]) if kind == "euler_a" else dpmpp_2m_sde_step(x, D, s, sn, eta, zs[i], state)
        if after is not None:
            x = after(x, i)
    return x


def sample_loop(model, noise, steps, zs, *, sampler, eta=1.0, sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0,
                prediction_type="epsilon", dtype=torch.float64):
    """tests/multistep_ref.sample_loop for the stochastic samplers: model(xin [2, 4, h, w], t) -> [2, 4, h, w]; zs: one [1, 4, h, w] per step that runs."""
    k, start, ts, sig = MR.schedule(steps, strength, sigmas)
    sig = sig.astype(np.float32).astype(np.float64)
    noise = noise.to(dtype)
    x0 = None if init_latents is None else init_latents.to(dtype)
    x = noise * float(sig[0]) if x0 is None else x0 + noise * float(sig[0])

    def denoise(x, i):
        s = float(sig[i])
        out = model(torch.cat([x, x], 0) / float((s * s + 1) ** 0.5), float(np.float32(ts[i])))
        return MR.denoised(out[0:1] + guidance_scale * (out[1:2] - out[0:1]), x, s, prediction_type)

    def blend(x, i):
        kk = x0 + noise * float(sig[i + 1])
        return kk + mask.to(dtype) * (x - kk)

    return published_loop(sampler, denoise, x, sig, eta, [z.to(dtype) for z in zs], blend if mask is not None else None)


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, zs, *, sampler, eta=1.0, sigmas="trailing", init_latents=None, strength=1.0,
                   mask=None, guidance_scale=8.0, size=None):
    """The fp32 published loop driven by the fp32 oracle UNet (tests/multistep_ref.sample_latents' conventions)."""
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    h, w = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        H, W = size if size is not None else (8 * h, 8 * w)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(H), float(W), 0.0, 0.0, float(H), float(W)]] * 2)}
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    with torch.no_grad():
        return sample_loop(lambda xin, t: U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2, dtype=torch.float32), ctx, add, lora=lora_s), noise, steps, zs,
                           sampler=sampler, eta=eta, sigmas=sigmas, init_latents=init_latents, strength=strength, mask=mask,
                           guidance_scale=guidance_scale, dtype=torch.float32)


# ---- the noise ----------------------------------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG = 0x53444531
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 values or arrays (broadcast together), key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in ctr])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                    # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def seed_key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def noise(seed, step, hw):
    """-> float64 [4, hw]: the four channel normals of every pixel of one image at step row `step`, from the exact uniforms."""
    w = philox4x32_10((np.arange(hw, dtype=np.uint64), step, 0, TAG), seed_key(seed))
    u = [((v >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for v in w]
    out = np.empty((4, hw), dtype=np.float64)
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(u[2 * h]))
        out[2 * h], out[2 * h + 1] = r * np.cos(2.0 * np.pi * u[2 * h + 1]), r * np.sin(2.0 * np.pi * u[2 * h + 1])
    return out


def _seeds_of(words):
    """int32 [n, 2] tensor of (lo, hi) words -> n Python ints."""
    w = words.cpu().numpy().view(np.uint32).astype(np.uint64)
    return [int(lo) | (int(hi) << 32) for lo, hi in w]


# ---- the kernels' contract on the CPU -----------------------------------------------------------------------------------------------------
def sampler_noise(seeds, step, out):
    """sdlt_sampler_noise on CPU tensors: the fp64 reference rounded to fp32 (the device evaluates log, sqrt, sin and cos in fp32: a few ulps apart)."""
    n, _, h, w = out.shape
    for j, seed in enumerate(_seeds_of(seeds)):
        out[j] = torch.from_numpy(noise(seed, int(step), h * w).astype(np.float32)).view(4, h, w)
    return out


def sampler_step_sde(eps, x, xin, timesteps, table, ctr, *, dprev, seeds, x0=None, noise=None, mask=None, init=False, z=None):
    """sdlt_sampler_step_sde on CPU tensors (x, dprev fp32 [n, 4, h, w] in place; table fp32 [rows, 8]; ctr int32 [2]).  z: the noise of this step
    (the GPU tests pass sdlt_sampler_noise's); None: sampler_noise's.  A row with d = 0 reads neither."""
    assert x.dtype == table.dtype == dprev.dtype == torch.float32 and not x.is_cuda and table.shape[1] == 8
    n, _, h, w = x.shape
    steps = max(1, min(int(table[1, 0]), table.shape[0] - 2))
    if init:
        v = noise * table[0, 1]
        x.copy_(v if x0 is None else x0 + v)
        inv, tn, nxt = table[0, 2], table[0, 3], 0
    else:
        i = max(0, min(int(ctr[0]), steps - 1))
        g, (s, sn, inv, tn, a, b, c, d) = table[0, 0], table[2 + i]
        e4 = eps.view(n, 2, h, w, 4).permute(0, 1, 4, 2, 3)
        e = e4[:, 0] + g * (e4[:, 1] - e4[:, 0])
        if float(table[1, 1]) != 0.0:
            s32 = np.float32(float(s))                                            # (IEEE divisions: see tests/multistep_ref.sampler_step_ms)
            q = s32 * s32 + np.float32(1.0)
            c1 = -s32 / np.sqrt(q)
            assert q.dtype == c1.dtype == np.float32
            D = e * float(c1) + x / torch.full_like(x, float(q))
        else:
            D = x - s * e
        xn = a * x + b * D
        if float(c) != 0.0:
            xn = xn + c * dprev
        if float(d) != 0.0:
            if z is None:
                z = sampler_noise(seeds, i, torch.empty_like(x))
            xn = xn + d * z
        if mask is not None:
            k = x0 + noise * sn
            xn = k + mask * (xn - k)
        x.copy_(xn)
        dprev.copy_(D)
        nxt = 0 if i + 1 >= steps else i + 1
    IR._repack(x, inv, xin, timesteps, tn, n, h, w)
    ctr[0], ctr[1] = nxt, 0
    return x


emu_sde = types.ModuleType("emu_sde")
emu_sde.__dict__.update({k: v for k, v in vars(MR.emu_ms).items() if not k.startswith("__")})
emu_sde.sampler_step_sde = sampler_step_sde
emu_sde.sampler_noise = sampler_noise
