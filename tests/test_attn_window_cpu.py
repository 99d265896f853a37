"""Tiled self-attention ("HyperTile") without a device: sampler.hypertile_plan's known answers and the refusals of the wrapper, of UNet.set_hypertile, of
sample, render and the CLI, and of the entry point."""
import ctypes as C

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops, sampler as SM


def test_hypertile_plan_known_answers():
    assert SM.hypertile_plan(17, 13, (0, 1), 4, 0) == ()                                   # prime sides stay whole: all plain
    assert SM.hypertile_plan(17, 34, (0, 1), 4, 0) == ((1, 2),)
    assert SM.hypertile_plan(128, 96, (1, 2), 32, 1) == ((4, 3), (4, 3))                   # SDXL's levels: 64 x 48 tokens in 16 x 16 tiles, 32 x 24 in 8 x 8
    assert SM.hypertile_plan(128, 96, (0, 1, 2, 3), 32, 0) == ((4, 3),)
    assert SM.hypertile_plan(128, 96, (1, 2), 48, 1) == ((2, 2), (2, 2))                   # 64 / 2 = 32 >= 24, 64 / 4 = 16 < 24
    assert SM.hypertile_plan(64, 64, (1, 2), 16, 9) == ((4, 4), (4, 4))                    # depth beyond the grids
    assert SM.hypertile_plan(64, 64, (1, 2), 64, 1) == ()                                  # one tile on every level


ARGS = dict(Q=0x10000, ldq=384, K=0x10100, ldk=384, V=0x10200, ldv=384, O=0x400000, ldo=128, B=2, H=2, Hg=12, Wg=20, ty=2, tx=2, d=64, scale=0.125)
REFUSALS = [(dict(Q=None), -1), (dict(K=None), -1), (dict(V=None), -1), (dict(O=None), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(Hg=0), -1), (dict(Wg=0), -1),
            (dict(ty=0), -1), (dict(tx=0), -1), (dict(d=0), -1), (dict(ty=5), -1), (dict(tx=3), -1), (dict(ldo=120), -1), (dict(ldk=64), -1), (dict(O=0x10000 + 768 * 10), -1),
            (dict(O=0x10300), -1), (dict(Hg=2 ** 16, Wg=2 ** 15), -1), (dict(B=2 ** 12, Hg=2 ** 10, Wg=2 ** 10), -1), (dict(ldq=388), -2), (dict(ldo=132), -2),
            (dict(Q=0x10008), -2), (dict(O=0x400002), -2), (dict(d=36), -4), (dict(d=104, ldq=640, ldk=640, ldv=640, ldo=208), -4)]


def test_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert lib.sdlt_attn_window_fwd(None, None) == -1 and b"sdlt_attn_window_fwd" in lib.sdlt_last_error()
    for change, code in REFUSALS:
        p = _lib.AttnWindowParams()
        for k, v in {**ARGS, **change}.items():
            setattr(p, k, v)
        assert lib.sdlt_attn_window_fwd(C.byref(p), None) == code and b"sdlt_attn_window_fwd" in lib.sdlt_last_error(), (change, lib.sdlt_last_error())


@pytest.mark.parametrize("what", ["cpu tensors", "bad grid", "tiles do not divide", "wide head", "no kernel", "bad pairs", "too many pairs", "grid not divided", "kv clash",
                                  "kv clash reversed", "forward grid", "training forward", "backward", "sampler dict", "sampler no kernel", "render px", "render depth alone",
                                  "render pass", "cli px", "cli depth alone", "cli pass hires"])
def test_refusals(what, tmp_path, capsys):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import render as R, topology
    from tests import kvpool_ref as KR
    z, kw = torch.zeros(64, 64, dtype=torch.bfloat16), dict(B=1, H=1, grid=(8, 8), tiles=(2, 2), d=64, scale=1.0)
    wrapper = {"cpu tensors": {}, "bad grid": dict(grid=(8, 0)), "tiles do not divide": dict(tiles=(3, 2)), "wide head": dict(d=104)}
    if what in wrapper:
        with pytest.raises(ValueError, match="attn_window_fwd"):
            ops.attn_window_fwd(z, z, z, z.clone(), **{**kw, **wrapper[what]})
        return
    if what.startswith("render"):
        a, msg = {"render px": ((100,), "multiple of 8"), "render depth alone": ((None, 1), "need hypertile"), "render pass": ((256, 0, "hires"), "has none")}[what]
        with pytest.raises(ValueError, match=msg):
            R.hypertile_args(*a)
        assert R.hypertile_args(True, hires=True) == dict(tile_px=256, tile=32, depth=0, passes="hires") and R.hypertile_args(64)["passes"] == "all"
        return
    if what.startswith("cli"):
        extra, msg = {"cli px": (["--hypertile", "100"], "multiple of 8"), "cli depth alone": (["--hypertile-depth", "1"], "need hypertile"),
                      "cli pass hires": (["--hypertile", "--hypertile-pass", "hires"], "has none")}[what]
        with pytest.raises(SystemExit) as e:
            R.main(["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")] + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
        return
    table = KR.emu_kv if "no kernel" in what else type("T", (), {**vars(KR.emu_kv), "attn_window_fwd": lambda *a, **k: pytest.fail("launched")})
    unet = unet_mod.UNet(unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=table), topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)
    if what.startswith("sampler"):
        from tests.test_tilediff_cpu import _embeds
        smp, em = SM.LatentSampler(unet.rt, unet), _embeds(U.CONFIGS["tiny15"], 5, 1)[0]
        exc, hp, msg = {"sampler dict": (ValueError, dict(tiles=4), "hypertile takes"), "sampler no kernel": (NotImplementedError, dict(tile=4), "sdlt_attn_window_fwd")}[what]
        with pytest.raises(exc, match=msg):
            smp.sample(em, 8, 8, steps=2, hypertile=hp)
        return
    if what in ("no kernel", "bad pairs", "too many pairs", "grid not divided", "kv clash"):
        if what == "kv clash":
            unet.set_kv_downsample((1, 2))
        exc, msg, args = {"no kernel": (NotImplementedError, "sdlt_attn_window_fwd", (((2, 2),),)), "bad pairs": (ValueError, "pairs of integers", ((2, (2, 0)),)),
                          "too many pairs": (ValueError, "4 pairs", (((2, 2),) * 4,)), "grid not divided": (ValueError, "token grid of down_blocks.1.attentions.0", (((2, 2), (4, 1)), (12, 8))),
                          "kv clash": (ValueError, "kv_downsample factor 2", (((2, 2), (2, 2)),))}[what]
        with pytest.raises(exc, match=msg):
            unet.set_hypertile(*args)
        assert unet._ht is None
        return
    assert sorted(unet.set_hypertile(((2, 2), (1, 1)))) == ["down_blocks.0.attentions.0", "up_blocks.2.attentions.0", "up_blocks.2.attentions.1"] and unet._ht == ((2, 2),)
    if what == "kv clash reversed":
        with pytest.raises(ValueError, match="set_hypertile"):
            unet.set_kv_downsample((2,))
        assert unet.set_kv_downsample((1, 2)) and unet.set_hypertile(None) == {} and unet._ht is None
        return
    if what == "backward":
        with pytest.raises(NotImplementedError, match="hypertile"):
            unet.backward(None, None)
        return
    hw = 9 if what == "forward grid" else 8      # (a 9 x 9 grid is not cut by 2 x 2)
    exc, msg = (ValueError, "do not divide the token grid .* of down_blocks.0.attentions.0") if what == "forward grid" else (NotImplementedError, "hypertile is an inference option")
    with pytest.raises(exc, match=msg):
        unet.forward(torch.zeros(2 * hw * hw, 64), torch.zeros(2), torch.zeros(2 * unet_mod.CTX_PAD, unet.cfg["cross_dim"]), B=2, H=hw, W=hw, train=what == "training forward")
