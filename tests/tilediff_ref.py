"""Tiled diffusion (MultiDiffusion) restated in torch on the CPU, independently of ops.py / sampler.py: the window geometry and weights from
tests/vaetile_ref.py's plain loops; `gather` and `blend32`, the contracts of sdlt_window_gather / sdlt_window_blend, which the kernels match bit for
bit; `blend64`, the same fusion in fp64 with unrounded weights; the two launches as entries of an emulated op table; and a reference trajectory - the
fp32 oracle UNet on every window, the predictions fused in fp64, the step taken by tests/multistep_ref.py's loop on the whole latent.

Layouts: full-size rows ((2 j + s) H + y) W + x (image j, s = 0 negative | 1 positive); tile batch row b = 2 (j ty tx + iy tx + ix) + s, pixel row
(b th + p) tw + q."""
import collections

import torch

from tests import vaetile_ref as TR

Geometry = collections.namedtuple("Geometry", "ys xs th tw ty tx")


def geometry(H, W, T, O):
    ys, xs = TR.tile_starts(H, T, O), TR.tile_starts(W, T, O)
    return Geometry(ys, xs, TR.extent(H, T), TR.extent(W, T), len(ys), len(xs))


def coverage(H, W, T, O):
    """The largest number of windows that cover one sample."""
    g = geometry(H, W, T, O)
    cy = max(sum(1 for s in g.ys if s <= y < s + g.th) for y in range(H))
    cx = max(sum(1 for s in g.xs if s <= x < s + g.tw) for x in range(W))
    return cy * cx


def tables(H, W, T, O):
    """What ops.window_tables returns, built from vaetile_ref: (ys int32 [ty], xs int32 [tx], wy fp32 [ty, th], wx fp32 [tx, tw], th, tw, ty, tx)."""
    g = geometry(H, W, T, O)
    return (torch.tensor(g.ys, dtype=torch.int32), torch.tensor(g.xs, dtype=torch.int32), torch.stack(TR.weights32(H, T, O, 1)),
            torch.stack(TR.weights32(W, T, O, 1)), g.th, g.tw, g.ty, g.tx)


def _windows(n, g):
    """(b, j, s, iy, ix) of every row of the tile batch, in order."""
    return [(2 * (j * g.ty * g.tx + iy * g.tx + ix) + s, j, s, iy, ix) for j in range(n) for iy in range(g.ty) for ix in range(g.tx) for s in range(2)]


def gather(x_full, tf_full, n, H, W, T, O):
    """x_full [2n H W, ld], tf_full [2n] -> (x_tiles [2n ty tx th tw, ld], tf_tiles [2n ty tx]): whole rows, every column."""
    g = geometry(H, W, T, O)
    ld = x_full.shape[1]
    xf = x_full.reshape(2 * n, H, W, ld)
    xt = torch.empty(2 * n * g.ty * g.tx, g.th, g.tw, ld, dtype=x_full.dtype)
    tf = torch.empty(2 * n * g.ty * g.tx, dtype=tf_full.dtype)
    for b, j, s, iy, ix in _windows(n, g):
        xt[b] = xf[2 * j + s, g.ys[iy]:g.ys[iy] + g.th, g.xs[ix]:g.xs[ix] + g.tw]
        tf[b] = tf_full[2 * j + s]
    return xt.reshape(-1, ld), tf


def _blend(eps_tiles, n, H, W, g, wys, wxs, dtype):
    et = eps_tiles.to(dtype).reshape(2 * n * g.ty * g.tx, g.th, g.tw, 4)
    out = torch.zeros(2 * n, H, W, 4, dtype=dtype)
    for b, j, s, iy, ix in _windows(n, g):          # per (j, s): iy ascending, then ix ascending - a sample's terms arrive in the kernel's order
        t = wys[iy].to(dtype)[:, None] * wxs[ix].to(dtype)[None, :]
        u = t[:, :, None] * et[b]
        view = out[2 * j + s, g.ys[iy]:g.ys[iy] + g.th, g.xs[ix]:g.xs[ix] + g.tw]
        view.copy_(view + u)
    return out.reshape(-1, 4)


def blend32(eps_tiles, n, H, W, T, O):
    """sdlt_window_blend's contract: eps_tiles fp32 [2n ty tx th tw, 4] -> fp32 [2n H W, 4]; per term t = wy * wx, u = t * v, acc = acc + u from +0.0, one
    fp32 rounding each (torch's CPU multiply and add are separate operations), the covering windows iy ascending then ix ascending."""
    assert eps_tiles.dtype == torch.float32
    return _blend(eps_tiles, n, H, W, geometry(H, W, T, O), TR.weights32(H, T, O, 1), TR.weights32(W, T, O, 1), torch.float32)


def blend64(eps_tiles, n, H, W, T, O, rounded_weights=False):
    """The fusion in fp64, with the unrounded normalised weights (rounded_weights: with the fp32 tables, taken to fp64 exactly)."""
    if rounded_weights:
        wys, wxs = TR.weights32(H, T, O, 1), TR.weights32(W, T, O, 1)
    else:
        wys, wxs = ([torch.tensor(r, dtype=torch.float64) for r in TR.tile_weights(L, T, O, 1)] for L in (H, W))
    return _blend(eps_tiles, n, H, W, geometry(H, W, T, O), wys, wxs, torch.float64)


# ---- the two launches as entries of an emulated op table (CPU tensors) ------------------------------------------------------------------------------
def _plan_of(tabs, H, W):
    """(T, O)-free restatement from the tables themselves: the emulated launches read starts and weights as the kernels do."""
    return Geometry(tabs.ys.tolist(), tabs.xs.tolist(), tabs.th, tabs.tw, tabs.ty, tabs.tx)


def emu_window_gather(tabs, x_full, x_tiles, tf_full, tf_tiles, *, n, H, W):
    g = _plan_of(tabs, H, W)
    xf, xt = x_full.view(2 * n, H, W, -1), x_tiles.view(2 * n * g.ty * g.tx, g.th, g.tw, -1)
    for b, j, s, iy, ix in _windows(n, g):
        xt[b].copy_(xf[2 * j + s, g.ys[iy]:g.ys[iy] + g.th, g.xs[ix]:g.xs[ix] + g.tw])
        tf_tiles[b] = tf_full[2 * j + s]
    return x_tiles


def emu_window_blend(tabs, eps_tiles, eps_full, *, n, H, W):
    g = _plan_of(tabs, H, W)
    eps_full.copy_(_blend(eps_tiles, n, H, W, g, list(tabs.wy), list(tabs.wx), torch.float32))
    return eps_full


def emu_table(base, name="emu_window"):
    """An op table = `base` (a module of emulated ops) plus the window launches; window_tables is the package's own (pure torch)."""
    import types
    from sd_lora_trainer_amd import ops
    m = types.ModuleType(name)
    m.__dict__.update({k: v for k, v in vars(base).items() if not k.startswith("__")})
    m.window_tables, m.window_gather, m.window_blend = ops.window_tables, emu_window_gather, emu_window_blend
    return m


# ---- the reference trajectory ---------------------------------------------------------------------------------------------------------------
def windowed_model(model, H, W, T, O):
    """model(xin [2, 4, th, tw], t) -> [2, 4, th, tw], the UNet on one window -> the same signature on the whole [2, 4, H, W] latent: every window's
    prediction, fused in fp64 with the unrounded weights."""
    g = geometry(H, W, T, O)

    def run(xin, t):
        tiles = torch.empty(2 * g.ty * g.tx, g.th, g.tw, 4, dtype=torch.float64)
        for b, j, s, iy, ix in _windows(1, g):
            if s == 0:                                  # one forward per window: both rows of the pair
                out = model(xin[:, :, g.ys[iy]:g.ys[iy] + g.th, g.xs[ix]:g.xs[ix] + g.tw].contiguous(), t)
                tiles[b], tiles[b + 1] = out[0].permute(1, 2, 0).double(), out[1].permute(1, 2, 0).double()
        full = blend64(tiles.reshape(-1, 4), 1, H, W, T, O)
        return full.reshape(2, H, W, 4).permute(0, 3, 1, 2).to(xin.dtype)
    return run


def sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, tile, *, sampler="euler", sigmas="trailing", init_latents=None, strength=1.0, mask=None,
                   guidance_scale=8.0, size=None, prediction_type="epsilon"):
    """tests/multistep_ref.py's fp32 reference loop with the fp32 oracle UNet run on every window of `tile` = (T, O); the conditioning of every window
    is the image's, SDXL's size conditioning the whole picture's."""
    from oracle import unet_ref as U
    from tests import multistep_ref as MR
    c, uc, pc, puc = (tuple(embeds) + (None, None))[:4]
    H, W = noise.shape[-2:]
    ctx = torch.cat([uc, c], 0)
    add = None
    if cfg["addition"]:
        PH, PW = size if size is not None else (8 * H, 8 * W)
        add = {"text_embeds": torch.cat([puc, pc], 0), "time_ids": torch.tensor([[float(PH), float(PW), 0.0, 0.0, float(PH), float(PW)]] * 2)}
    lora_s = None if lora is None else {k: (A, B * lora_scale) for k, (A, B) in lora.items()}
    one = lambda xin, t: U.unet_forward(cfg, sd, xin, torch.tensor([t] * 2, dtype=torch.float32), ctx, add, lora=lora_s)  # noqa: E731
    with torch.no_grad():
        return MR.sample_loop(windowed_model(one, H, W, *tile), noise, steps, sampler=sampler, sigmas=sigmas, init_latents=init_latents, strength=strength,
                              mask=mask, guidance_scale=guidance_scale, prediction_type=prediction_type, dtype=torch.float32)
