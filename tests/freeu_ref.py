"""FreeU (Si et al., CVPR 2024) restated in torch and fp64 for the tests of sdlt_freeu, UNet.set_freeu, LatentSampler.sample(freeu=) and render(freeu=).
Written from the published method (the authors' Fourier_filter / diffusers' apply_freeu), not from the package:

 * skip filter: `fourier_filter` is the published fftn -> fftshift -> mask[crow - 1 : crow + 1, ccol - 1 : ccol + 1] = s -> ifftshift -> ifftn(.).real
   (threshold 1) on NCHW, through torch.fft.  `closed_form` is the header's seven-sum form of the same four bins; tests/test_freeu_cpu.py holds the one
   to the other, so the kernel is checked against the FFT definition and not against itself;
 * backbone scale: version 1 multiplies the first half of the channels by b; version 2 by (b - 1) n + 1 with n the per-image min-max-normalised channel
   mean (n = 0 where max == min: the library's stated choice);
 * placement: diffusers' rule - every resnet of up_blocks.0 takes (b1, s1), every resnet of up_blocks.1 (b2, s2), right before it reads cat(h, skip).

`emu_freeu` is tests/img2img_ref.emu_img plus a torch `freeu`, so the CPU tests run the host path; `unet_forward_freeu` / `sample_latents_freeu` are the
fp32 oracle UNet and the oracle sampler loop with oracle.unet_ref._resnet wrapped for those two blocks (oracle/ itself is not edited)."""
import contextlib
import math
import types

import torch

from oracle import sampler_ref as SR
from oracle import unet_ref as U
from tests import img2img_ref as IR


def as_dict(freeu):
    if isinstance(freeu, dict):
        return dict(freeu, version=freeu.get("version", 1))
    b1, b2, s1, s2 = freeu
    return dict(b1=b1, b2=b2, s1=s1, s2=s2, version=1)


def fourier_filter(x, s):
    """x [..., H, W] -> the published filter (threshold 1), in the dtype of x (use float64)."""
    H, W = x.shape[-2:]
    if H < 2 or W < 2:
        raise ValueError("the published mask slice is empty on an axis of size 1")
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[crow - 1: crow + 1, ccol - 1: ccol + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(X * mask, dim=(-2, -1)), dim=(-2, -1)).real


def closed_form(x, s):
    """The header's form: skip + (s - 1) L, L from S0 and the six cos / sin weighted sums of each plane."""
    H, W = x.shape[-2:]
    ty = (2 * math.pi / H) * torch.arange(H, dtype=x.dtype)[:, None]
    tx = (2 * math.pi / W) * torch.arange(W, dtype=x.dtype)[None, :]
    one = torch.ones(H, W, dtype=x.dtype)
    basis = [one, torch.cos(ty) * one, torch.sin(ty) * one, torch.cos(tx) * one, torch.sin(tx) * one, torch.cos(ty + tx), torch.sin(ty + tx)]
    L = sum((x * w).sum((-2, -1), keepdim=True) * w for w in basis) / (H * W)
    return x + (s - 1) * L


def backbone(h, b, version):
    """h [B, C, H, W] -> the first C // 2 channels scaled."""
    C = h.shape[1]
    out = h.clone()
    if version == 1:
        out[:, : C // 2] = h[:, : C // 2] * b
        return out
    m = h.mean(1, keepdim=True)
    lo, hi = m.amin((-2, -1), keepdim=True), m.amax((-2, -1), keepdim=True)
    n = torch.where(hi > lo, (m - lo) / torch.where(hi > lo, hi - lo, torch.ones_like(hi)), torch.zeros_like(m))
    out[:, : C // 2] = h[:, : C // 2] * ((b - 1) * n + 1)
    return out


def freeu_nchw(h, skip, b, s, version, filt=fourier_filter):
    """(h [B, C1, H, W], skip [B, C2, H, W]) -> their FreeU forms, fp64."""
    return backbone(h.double(), b, version), filt(skip.double(), s)


def freeu_rows(h, skip, B, H, W, b, s, version):
    """The kernel's layout: h [B H W, C1], skip [B H W, C2] (any float dtype) -> fp64 rows of the same shapes."""
    nchw = lambda t: t.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)  # noqa: E731
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1)  # noqa: E731
    ho, so = freeu_nchw(nchw(h), nchw(skip), b, s, version)
    return rows(ho), rows(so)


# ---- the op on CPU tensors ------------------------------------------------------------------------------------------------------------------
def freeu_tables(H, W, device):
    return torch.zeros(2 * H + 2 * W, device=device)          # (the torch op takes its angles from torch.fft)


def freeu_ws_floats(B, H, W, C1, C2):
    return 1


def freeu(h, skip, h_out, skip_out, tabs, ws, *, B, H, W, b, s, version=1):
    """ops.freeu on CPU tensors.  Neutral parameters copy, as the kernel does."""
    assert h.shape == h_out.shape and skip.shape == skip_out.shape and h.shape[0] == skip.shape[0] == B * H * W and h.shape[1] % 2 == 0
    assert h_out.data_ptr() not in (h.data_ptr(), skip.data_ptr()) and skip_out.data_ptr() not in (h.data_ptr(), skip.data_ptr())
    ho, so = freeu_rows(h, skip, B, H, W, b, s, version)
    h_out.copy_(h if b == 1 else ho.to(h.dtype))
    skip_out.copy_(skip if s == 1 else so.to(skip.dtype))
    return h_out, skip_out


emu_freeu = types.ModuleType("emu_freeu")
emu_freeu.__dict__.update({k: v for k, v in vars(IR.emu_img).items() if not k.startswith("__")})
emu_freeu.freeu, emu_freeu.freeu_tables, emu_freeu.freeu_ws_floats = freeu, freeu_tables, freeu_ws_floats


# ---- the oracle UNet with FreeU ---------------------------------------------------------------------------------------------------------
def backbone_widths(cfg):
    """resnet name -> channels of h in cat(h, skip) for the resnets of up_blocks.0 and up_blocks.1 (the wiring of diffusers' UNet2DConditionModel)."""
    rev = list(reversed(cfg["block_out_channels"]))
    out = {}
    for i in (0, 1):
        prev = rev[max(i - 1, 0)]
        for j in range(cfg["layers_per_block"] + 1):
            out[f"up_blocks.{i}.resnets.{j}"] = prev if j == 0 else rev[i]
    return out


@contextlib.contextmanager
def oracle_freeu(cfg, freeu):
    """Inside: oracle.unet_ref.unet_forward applies FreeU in front of the resnets of up_blocks.0 / .1 (freeu None: nothing changes)."""
    if freeu is None:
        yield
        return
    fz, widths, real = as_dict(freeu), backbone_widths(cfg), U._resnet

    def resnet(c, n, x, temb):
        if n in widths:
            i, C1 = int(n.split(".")[1]), widths[n]
            assert 0 < C1 < x.shape[1]
            ho, so = freeu_nchw(x[:, :C1], x[:, C1:], fz[f"b{i + 1}"], fz[f"s{i + 1}"], fz["version"])
            x = torch.cat([ho, so], 1).to(x.dtype)
        return real(c, n, x, temb)

    U._resnet = resnet
    try:
        yield
    finally:
        U._resnet = real


def unet_forward_freeu(cfg, sd, sample, timesteps, ctx, added_cond=None, lora=None, *, freeu):
    with oracle_freeu(cfg, freeu), torch.no_grad():
        return U.unet_forward(cfg, sd, sample, timesteps, ctx, added_cond, lora=lora)


def sample_latents_freeu(cfg, sd, lora, lora_scale, embeds, noise, steps, *, freeu, guidance_scale=8.0, size=None):
    """oracle.sampler_ref.sample_latents with FreeU in every forward."""
    with oracle_freeu(cfg, freeu):
        return SR.sample_latents(cfg, sd, lora, lora_scale, embeds, noise, steps, guidance_scale=guidance_scale, size=size)
