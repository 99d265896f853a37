"""The launch sequence of LatentSampler.sample() is pinned: every call the sampler makes on its op table - the setup's, the init launch and each iteration's
forward stage and step launch - is recorded by name on an emulated table and compared with a literal list, for every step family (sampler.FAMILIES), with
and without the guidance pre-pass and the mask, with heat maps and with windows, on the fused path and in the torch loop.  The UNet is a stand-in that calls
no op, so a list holds the sampler's own launches only.  The lists were recorded from the commit before the sampler's two drivers were given one setup and
one forward stage; a driver that reorders, drops or adds a launch fails here without a GPU."""
import types

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd.unet import CTX_PAD
from tests import diffdiff_ref as DR
from tests import guidance_ref as GR
from tests import heatmap_ref as HR
from tests import tilediff_ref as TD
from tests.test_img2img_cpu import EMB, _Stub, _case

H, W, STEPS = 8, 12, 4

_full = HR.with_heat(TD.emu_table(GR.emu_guidance), "emu_sequence")      # every step family but dd, the pre-pass, the windows, the heat maps
_full.sampler_step_dd = DR.sampler_step_dd


def recording(table, seen):
    """`table` with every function wrapped to append its name to `seen` first (constants and classes as they are: hasattr answers alike)."""
    mod = types.ModuleType(table.__name__ + "_recorded")
    for name, v in vars(table).items():
        if isinstance(v, types.FunctionType):
            v = (lambda f, nm: lambda *a, **k: (seen.append(nm), f(*a, **k))[1])(v, name)
        if not name.startswith("__"):
            setattr(mod, name, v)
    return mod


class _HeatStub(_Stub):
    """_Stub that leaves score sums at one resolution behind, as the UNet's hooked cross-attentions do."""

    def forward(self, x, t, ctx, pooled, tid, *, B, H, W):
        g = torch.Generator().manual_seed(self.calls)
        self.rt.daam_sums = {H * W: [torch.randn(B * H * W, CTX_PAD, generator=g), 1, False]}
        return super().forward(x, t, ctx, pooled, tid, B=B, H=H, W=W)


def _family_kw(family, masked):
    """sample()'s keywords that select `family`; masked: with init latents and a mask."""
    noise, x0, mask = _case(H, W)
    img = dict(init_latents=x0, strength=0.75)
    dd = dict(img, change_map=torch.linspace(0, 1, H * W).view(1, 1, H, W))
    kw = dict(euler={}, img=img, multistep=dict(sampler="dpmpp_2m"), sde=dict(sampler="euler_a", seeds=[5]), dd_euler=dd,
              dd_ms=dict(dd, sampler="dpmpp_2m"), dd_sde=dict(dd, sampler="dpmpp_2m_sde", seeds=[5]))[family]
    if masked:
        kw = dict(kw, **img, mask=mask)
    return dict(kw, latents=noise.clone())


CASES = [(f, guided, masked) for f in SM.FAMILIES for guided in (False, True) for masked in ((False, True) if f in ("img", "multistep", "sde") else (False,))]


def run(fused, family="euler", guided=False, masked=False, heat=False, tile=None):
    """-> the names of the op calls of one sample() of STEPS steps (3 of them run from init latents), in order."""
    seen = []
    plan = SM.tile_plan(H, W, tile)
    tiles = 1 if plan is None else plan.ty * plan.tx
    rt = unet_mod.Runtime("cpu", 2 * tiles, act_dtype=torch.float32, ops=recording(_full, seen))
    stub = (_HeatStub if heat else _Stub)(tiles, H if plan is None else plan.th, W if plan is None else plan.tw, 7)
    stub.rt, stub.cfg = rt, dict(stub.cfg, block_out_channels=(64, 128, 128))
    smp = SM.LatentSampler(rt, stub, n_images=1)
    kw = _family_kw(family, masked)
    if guided:
        kw.update(guidance_rescale=0.5)
    if heat:
        kw.update(heatmap=dict(cols=[[[1, 2], [76, -1]]]))
    if tile is not None:
        kw.update(tile=tile)
    out = smp.sample(EMB, H, W, steps=STEPS, fused=fused, **kw)
    assert torch.isfinite(out[0] if heat else out).all()
    assert SM.step_family(kw.get("sampler", "euler"), None if "init_latents" not in kw else True, "change_map" in kw) == family
    return seen


def _id(family, guided, masked):
    return family + ("-guided" if guided else "") + ("-masked" if masked else "")


# ---- recorded from the parent commit: {case: the whole call's op names} -----------------------------------------------------------------------
FUSED = {"euler": ["sampler_step", "sampler_step", "sampler_step", "sampler_step", "sampler_step"],
 "euler-guided": ["sampler_step", "guidance", "sampler_step", "guidance", "sampler_step", "guidance", "sampler_step", "guidance", "sampler_step"],
 "img": ["sampler_step_img", "sampler_step_img", "sampler_step_img", "sampler_step_img"],
 "img-masked": ["sampler_step_img", "sampler_step_img", "sampler_step_img", "sampler_step_img"],
 "img-guided": ["sampler_step_img", "guidance", "sampler_step_img", "guidance", "sampler_step_img", "guidance", "sampler_step_img"],
 "img-guided-masked": ["sampler_step_img", "guidance", "sampler_step_img", "guidance", "sampler_step_img", "guidance", "sampler_step_img"],
 "multistep": ["sampler_step_ms", "sampler_step_ms", "sampler_step_ms", "sampler_step_ms", "sampler_step_ms"],
 "multistep-masked": ["sampler_step_ms", "sampler_step_ms", "sampler_step_ms", "sampler_step_ms"],
 "multistep-guided": ["sampler_step_ms", "guidance", "sampler_step_ms", "guidance", "sampler_step_ms", "guidance", "sampler_step_ms", "guidance",
                      "sampler_step_ms"],
 "multistep-guided-masked": ["sampler_step_ms", "guidance", "sampler_step_ms", "guidance", "sampler_step_ms", "guidance", "sampler_step_ms"],
 "sde": ["sampler_step_sde", "sampler_step_sde", "sampler_step_sde", "sampler_step_sde", "sampler_step_sde"],
 "sde-masked": ["sampler_step_sde", "sampler_step_sde", "sampler_step_sde", "sampler_step_sde"],
 "sde-guided": ["sampler_step_sde", "guidance", "sampler_step_sde", "guidance", "sampler_step_sde", "guidance", "sampler_step_sde", "guidance",
                "sampler_step_sde"],
 "sde-guided-masked": ["sampler_step_sde", "guidance", "sampler_step_sde", "guidance", "sampler_step_sde", "guidance", "sampler_step_sde"],
 "dd_euler": ["sampler_step_dd", "sampler_step_dd", "sampler_step_dd", "sampler_step_dd"],
 "dd_euler-guided": ["sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd"],
 "dd_ms": ["sampler_step_dd", "sampler_step_dd", "sampler_step_dd", "sampler_step_dd"],
 "dd_ms-guided": ["sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd"],
 "dd_sde": ["sampler_step_dd", "sampler_step_dd", "sampler_step_dd", "sampler_step_dd"],
 "dd_sde-guided": ["sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd", "guidance", "sampler_step_dd"]}
TORCH = {"euler": [],
 "euler-guided": ["guidance", "guidance", "guidance", "guidance"],
 "img": [],
 "img-masked": [],
 "img-guided": ["guidance", "guidance", "guidance"],
 "img-guided-masked": ["guidance", "guidance", "guidance"],
 "multistep": [],
 "multistep-masked": [],
 "multistep-guided": ["guidance", "guidance", "guidance", "guidance"],
 "multistep-guided-masked": ["guidance", "guidance", "guidance"],
 "sde": ["sampler_noise", "sampler_noise", "sampler_noise"],
 "sde-masked": ["sampler_noise", "sampler_noise"],
 "sde-guided": ["guidance", "sampler_noise", "guidance", "sampler_noise", "guidance", "sampler_noise", "guidance"],
 "sde-guided-masked": ["guidance", "sampler_noise", "guidance", "sampler_noise", "guidance"],
 "dd_euler": [],
 "dd_euler-guided": ["guidance", "guidance", "guidance"],
 "dd_ms": [],
 "dd_ms-guided": ["guidance", "guidance", "guidance"],
 "dd_sde": ["sampler_noise", "sampler_noise"],
 "dd_sde-guided": ["guidance", "sampler_noise", "guidance", "sampler_noise", "guidance"]}
EXTRA = {("heat", True): ["sampler_step", "heatmap_accum", "sampler_step", "heatmap_accum", "sampler_step", "heatmap_accum", "sampler_step", "heatmap_accum",
                  "sampler_step"],
 ("heat", False): ["heatmap_accum", "heatmap_accum", "heatmap_accum", "heatmap_accum"],
 ("heat-guided", True): ["sampler_step", "heatmap_accum", "guidance", "sampler_step", "heatmap_accum", "guidance", "sampler_step", "heatmap_accum",
                         "guidance", "sampler_step", "heatmap_accum", "guidance", "sampler_step"],
 ("heat-guided", False): ["heatmap_accum", "guidance", "heatmap_accum", "guidance", "heatmap_accum", "guidance", "heatmap_accum", "guidance"],
 ("tile", True): ["window_tables", "sampler_step", "window_gather", "window_blend", "sampler_step", "window_gather", "window_blend", "sampler_step",
                  "window_gather", "window_blend", "sampler_step", "window_gather", "window_blend", "sampler_step"],
 ("tile", False): ["window_tables", "window_gather", "window_blend", "window_gather", "window_blend", "window_gather", "window_blend",
                   "window_gather", "window_blend"],
 ("tile-guided-sde", True): ["window_tables", "sampler_step_sde", "window_gather", "window_blend", "guidance", "sampler_step_sde", "window_gather",
                             "window_blend", "guidance", "sampler_step_sde", "window_gather", "window_blend", "guidance", "sampler_step_sde",
                             "window_gather", "window_blend", "guidance", "sampler_step_sde"],
 ("tile-guided-sde", False): ["window_tables", "window_gather", "window_blend", "guidance", "sampler_noise", "window_gather", "window_blend",
                              "guidance", "sampler_noise", "window_gather", "window_blend", "guidance", "sampler_noise", "window_gather",
                              "window_blend", "guidance"]}


@pytest.mark.parametrize("family,guided,masked", CASES, ids=[_id(*c) for c in CASES])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_family_sequence(fused, family, guided, masked):
    assert run(fused, family, guided, masked) == (FUSED if fused else TORCH)[_id(family, guided, masked)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("what,kw", [("heat", dict(heat=True)), ("heat-guided", dict(heat=True, guided=True)), ("tile", dict(tile=(8, 2))),
                                     ("tile-guided-sde", dict(tile=(8, 2), guided=True, family="sde"))])
def test_heat_and_tile_sequence(what, kw, fused):
    assert run(fused, **kw) == EXTRA[what, fused]


def test_every_family_is_covered():
    assert {c[0] for c in CASES} == set(SM.FAMILIES) and len(CASES) == 20
