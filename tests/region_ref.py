"""Regional prompts (MultiDiffusion section 4.2) restated in torch on the CPU, independently of ops.py / sampler.py: the normalised weights
by plain loops in fp64; `gather_ref` and `blend32`, the contracts of sdlt_region_gather / sdlt_region_blend, which the kernels match bit for bit;
`blend64`, the same fusion in fp64 with unrounded weights; the bootstrap noise from tests/sde_ref.py's Philox; the launches as entries of an emulated
op table; and a reference trajectory - the fp32 oracle UNet on every region's rows, the predictions fused in fp64, the step taken by
tests/multistep_ref.py's loop on the whole latent.

Layouts: full-size rows ((2 j + s) H + y) W + x (image j, s = 0 negative | 1 positive); region batch row b = 2 (j R + r) + s, pixel row (b H + y) W + x.
Region 0 is the background."""
import numpy as np
import torch

from tests import sde_ref as SR

TAG = 0x52474E31            # counter word 3 of the bootstrap noise; the stochastic samplers' is sde_ref.TAG
TABLE_ROWS = 1000           # rows of the bootstrap table
assert TAG != SR.TAG


# ---- weights ----------------------------------------------------------------------------------------------------------------------------------
def weights64(h, w, masks, base=0.0):
    """masks [R - 1][h][w] numbers in [0, 1] -> (wn, raw), lists [R][h][w] of Python floats (fp64): raw[0] = clamp(1 - sum fg, 0, 1) + base, raw[r] the
    masks, wn = raw / its sum over r.  Plain loops."""
    m = [[[float(v) for v in row] for row in plane] for plane in (masks.tolist() if torch.is_tensor(masks) else masks)]
    R = len(m) + 1
    raw = [[[0.0] * w for _ in range(h)] for _ in range(R)]
    wn = [[[0.0] * w for _ in range(h)] for _ in range(R)]
    for y in range(h):
        for x in range(w):
            fg = 0.0
            for r in range(1, R):
                raw[r][y][x] = m[r - 1][y][x]
                fg += m[r - 1][y][x]
            raw[0][y][x] = min(max(1.0 - fg, 0.0), 1.0) + base
            total = 0.0
            for r in range(R):
                total += raw[r][y][x]
            assert total > 0.0
            for r in range(R):
                wn[r][y][x] = raw[r][y][x] / total
    return wn, raw


def tables(h, w, masks, base=0.0):
    """What ops.region_tables returns, from weights64: (wn fp32 [R, h, w], wraw fp32 [R, h, w], R)."""
    wn, raw = weights64(h, w, masks, base)
    return torch.tensor(wn, dtype=torch.float64).to(torch.float32), torch.tensor(raw, dtype=torch.float64).to(torch.float32), len(wn)


# ---- the noise --------------------------------------------------------------------------------------------------------------------------------
def noise(seed, step, region, hw):
    """-> float64 [4, hw]: the four channel normals of every pixel of one image at step row `step` for region `region`, from the exact uniforms
    (tests/sde_ref.noise with the counter (pixel, step, region, TAG))."""
    wd = SR.philox4x32_10((np.arange(hw, dtype=np.uint64), step, region, TAG), SR.seed_key(seed))
    u = [((v >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for v in wd]
    out = np.empty((4, hw), dtype=np.float64)
    for k in range(2):
        r = np.sqrt(-2.0 * np.log(u[2 * k]))
        out[2 * k], out[2 * k + 1] = r * np.cos(2.0 * np.pi * u[2 * k + 1]), r * np.sin(2.0 * np.pi * u[2 * k + 1])
    return out


def region_noise(seeds, step, region, out):
    """sdlt_region_noise on CPU tensors: the fp64 reference rounded to fp32 (the device evaluates log, sqrt, sin and cos in fp32: a few ulps apart)."""
    n, _, h, w = out.shape
    for j, seed in enumerate(SR._seeds_of(seeds)):
        out[j] = torch.from_numpy(noise(seed, int(step), int(region), h * w).astype(np.float32)).view(4, h, w)
    return out


# ---- the two launches' contracts ---------------------------------------------------------------------------------------------------------------
def gather_ref(x_full, tf_full, n, R, H, W, boot=None):
    """x_full bf16 [2n H W, ld], tf_full [2n] -> (x_regions [2n R H W, ld], tf_regions [2n R]): whole rows, every column.  boot: None, or dict(wraw fp32
    [R, H, W], bg fp32 [n, R, 4], sigma, inv (fp32 scalars of the step's row; sigma < 0: no bootstrap), z fp32 [n, R, 4, H, W] (z[:, r]: the launch's
    noise for region r)): columns 0 .. 3 of the rows of a region r >= 1 where wraw[r] < 0.5 are bf16((bg + sigma z) inv) - three fp32 operations."""
    ld = x_full.shape[1]
    xf = x_full.reshape(2 * n, H, W, ld)
    xr = torch.empty(2 * n * R, H, W, ld, dtype=x_full.dtype)
    tf = torch.empty(2 * n * R, dtype=tf_full.dtype)
    for j in range(n):
        for r in range(R):
            for s in range(2):
                b = 2 * (j * R + r) + s
                xr[b] = xf[2 * j + s]
                tf[b] = tf_full[2 * j + s]
                if boot is not None and r >= 1 and float(boot["sigma"]) >= 0.0:
                    sigma, inv = torch.tensor(float(boot["sigma"]), dtype=torch.float32), torch.tensor(float(boot["inv"]), dtype=torch.float32)
                    z = boot["z"][j, r].permute(1, 2, 0)                                   # [H, W, 4]
                    t = sigma * z
                    u = boot["bg"][j, r].view(1, 1, 4) + t
                    v = (u * inv).to(x_full.dtype)
                    assert t.dtype == u.dtype == torch.float32
                    out = boot["wraw"][r] < 0.5
                    xr[b][..., :4][out] = v[out]
    return xr.reshape(-1, ld), tf


def _blend(eps_regions, wn, n, R, H, W, dtype):
    e = eps_regions.to(dtype).reshape(n, R, 2, H, W, 4)
    acc = torch.zeros(n, 2, H, W, 4, dtype=dtype)
    for r in range(R):                                  # r ascending: a pixel's terms arrive in the kernel's order
        u = wn[r].to(dtype).view(1, 1, H, W, 1) * e[:, r]
        acc = acc + u
    return acc.reshape(-1, 4)


def blend32(eps_regions, wn, n, R, H, W):
    """sdlt_region_blend's contract: eps_regions fp32 [2n R H W, 4], wn fp32 [R, H, W] -> fp32 [2n H W, 4]; per term u = w * v, acc = acc + u from +0.0,
    one fp32 rounding each (torch's CPU multiply and add are separate operations), r ascending."""
    assert eps_regions.dtype == torch.float32 and wn.dtype == torch.float32
    return _blend(eps_regions, wn, n, R, H, W, torch.float32)


def blend64(eps_regions, wn, n, R, H, W):
    """The fusion in fp64; wn: any dtype (fp64 unrounded weights, or the fp32 tables taken to fp64 exactly)."""
    return _blend(eps_regions, wn, n, R, H, W, torch.float64)


# ---- the launches as entries of an emulated op table (CPU tensors) ----------------------------------------------------------------------------------
READS = dict(noise=0)          # how often the emulated gather asked for noise (a bootstrap step of a foreground region)


def emu_region_gather(tabs, x_full, x_regions, tf_full, tf_regions, *, n, H, W, boot=None):
    b = None
    if boot is not None:
        i = max(0, min(int(boot["ctr"][0]), TABLE_ROWS - 1))
        sigma, inv = boot["rtab"][i]
        b = dict(wraw=tabs.wraw, sigma=sigma, inv=inv)
        if float(sigma) >= 0.0:                         # (uniform over the launch: without bootstrap neither seeds nor bg are read)
            z = torch.zeros(n, tabs.R, 4, H, W)
            for r in range(1, tabs.R):
                READS["noise"] += 1
                region_noise(boot["seeds"], i, r, z[:, r])
            b.update(bg=boot["bg"], z=z)
    xr, tf = gather_ref(x_full, tf_full[: 2 * n], n, tabs.R, H, W, b)
    x_regions.copy_(xr)
    tf_regions[: 2 * n * tabs.R] = tf
    return x_regions


def emu_region_blend(tabs, eps_regions, eps_full, *, n, H, W):
    eps_full.copy_(blend32(eps_regions, tabs.wn, n, tabs.R, H, W))
    return eps_full


def emu_table(base, name="emu_region"):
    """An op table = `base` (a module of emulated ops) plus the region launches; region_tables is the package's own (pure torch)."""
    import types
    from sd_lora_trainer_amd import ops
    m = types.ModuleType(name)
    m.__dict__.update({k: v for k, v in vars(base).items() if not k.startswith("__")})
    m.region_tables, m.region_gather, m.region_blend, m.region_noise = ops.region_tables, emu_region_gather, emu_region_blend, region_noise
    return m


# ---- the reference trajectory ---------------------------------------------------------------------------------------------------------------
def regional_model(models, wn, H, W, boot=None):
    """models[r](xin [2, 4, H, W], t) -> [2, 4, H, W], the UNet with region r's conditioning -> the same signature: every region's prediction, fused
    in fp64 with the weights wn [R, H, W].  boot: None, or dict(wraw, bg [R, 4], sig (the sigmas of the steps that run), k (steps that bootstrap),
    seed): call i < k gives region r >= 1 the background noised to sigma_i outside its mask, from the emulated noise."""
    R, calls = len(models), [0]

    def run(xin, t):
        i = calls[0]
        calls[0] += 1
        rows = torch.empty(2 * R, H, W, 4, dtype=torch.float64)
        for r in range(R):
            xr = xin
            if boot is not None and r >= 1 and i < boot["k"]:
                s = float(boot["sig"][i])
                z = torch.from_numpy(noise(boot["seed"], i, r, H * W)).view(4, H, W).to(xin.dtype)
                v = (boot["bg"][r].view(4, 1, 1).to(xin.dtype) + s * z) / float((s * s + 1.0) ** 0.5)
                xr = torch.where((boot["wraw"][r] < 0.5).view(1, 1, H, W), v[None], xin)
            out = models[r](xr.contiguous(), t)
            rows[2 * r], rows[2 * r + 1] = out[0].permute(1, 2, 0).double(), out[1].permute(1, 2, 0).double()
        full = blend64(rows.reshape(-1, 4), wn, 1, R, H, W)
        return full.reshape(2, H, W, 4).permute(0, 3, 1, 2).to(xin.dtype)
    return run


def sample_latents(cfg, sd, lora, lora_scale, embeds, region_embeds, masks, noise_, steps, *, base=0.0, bootstrap=0, bg=None, seed=0, sampler="euler",
                   sigmas="trailing", init_latents=None, strength=1.0, mask=None, guidance_scale=8.0, size=None, prediction_type="epsilon"):
    """tests/multistep_ref.py's fp32 reference loop with the fp32 oracle UNet run once per region: region r >= 1 takes region_embeds[r - 1]'s positive
    conditioning, every region the main negative one; SDXL's size conditioning is the whole picture's."""
    from oracle import unet_ref as U
    from tests import multistep_ref as MR
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    H, W = noise_.shape[-2:]
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    models = []
    for e in [embeds] + list(region_embeds):
        cr, _, pcr, _ = (tuple(e) + (None, None))[:4]
        ctx = torch.cat([uc, cr], 0)
        add = None
        if cfg["addition"]:
            PH, PW = size if size is not None else (8 * H, 8 * W)
            add = {"text_embeds": torch.cat([puc, pcr], 0), "time_ids": torch.tensor([[float(PH), float(PW), 0.0, 0.0, float(PH), float(PW)]] * 2)}
        models.append(lambda xin, t, ctx=ctx, add=add: U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2, dtype=torch.float32), ctx, add, lora=lora_s))
    wn, raw = weights64(H, W, masks, base)
    wn = torch.tensor(wn, dtype=torch.float64)
    boot = None
    if bootstrap:
        k, _, _, sig = MR.schedule(steps, strength, sigmas)
        boot = dict(wraw=torch.tensor(raw, dtype=torch.float64).to(torch.float32), bg=torch.zeros(len(models), 4) if bg is None else bg, k=min(bootstrap, k),
                    sig=sig.astype(np.float32).astype(np.float64), seed=seed)
    with torch.no_grad():
        return MR.sample_loop(regional_model(models, wn, H, W, boot), noise_, steps, sampler=sampler, sigmas=sigmas, init_latents=init_latents,
                              strength=strength, mask=mask, guidance_scale=guidance_scale, prediction_type=prediction_type, dtype=torch.float32)
