"""Attention couple without a device: ops.couple_weights' known answers and the refusals of the wrapper, of UNet.set_attention_couple and of the entry point."""
import ctypes as C

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops


def test_couple_weights_known_answers():
    wn = torch.zeros(2, 4, 6)
    wn[0, :, :3], wn[1, :, 3:] = 1.0, 1.0      # a hard left / right split
    t = ops.couple_weights(wn, [0, 1, 2])
    assert sorted(t) == [1, 6, 24] and torch.equal(t[24], wn.reshape(2, 24)) and torch.equal(t[1], torch.tensor([[0.75], [0.25]]))
    assert torch.equal(t[6].view(2, 2, 3)[0], torch.tensor([[1, 0.5, 0], [1, 0.5, 0]])) and torch.equal(t[6][1], 1 - t[6][0])
    w3 = torch.softmax(torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(0)), 0)
    t = ops.couple_weights(w3, [1, 0])
    blk = w3.double()[:, :4, :6].reshape(3, 2, 2, 3, 2).mean(dim=(2, 4))      # 2 x 3 tokens: the odd last row and column have no token
    assert torch.equal(t[35], w3.reshape(3, 35)) and torch.equal(t[6], (blk / blk.sum(0)).float().reshape(3, 6))
    assert all(float((tab.double().sum(0) - 1).abs().max()) <= 2.0 ** -23 for tab in t.values())


ARGS = dict(Q=0x10000, ldq=128, K=0x20000, ldk=128, V=0x30000, ldv=128, O=0x40000, ldo=128, Wt=0x50000, rcount=0x60000, B=2, H=2, Nq=72, Nk=77, Nkp=128, R=3, d=64, scale=0.125)
REFUSALS = [dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(Wt=None), dict(B=0), dict(H=0), dict(Nq=0), dict(Nk=0), dict(R=0), dict(d=0),
            dict(R=17), dict(Nk=129, Nkp=136), dict(Nkp=72), dict(Nk=70, Nkp=76), dict(d=36), dict(d=168, ldq=336, ldk=336, ldv=336, ldo=336),
            dict(ldq=132), dict(ldo=120), dict(ldk=64), dict(Q=0x10008), dict(O=0x40002), dict(Wt=0x50002), dict(rcount=0x60001),
            dict(O=0x10000 + 2 * 128 * 10), dict(O=0x20000), dict(O=0x50000), dict(Nq=2 ** 31 - 10), dict(B=2 ** 20, H=2 ** 12)]


def test_entry_point_validation():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert lib.sdlt_attn_couple_fwd(None, None) == -1 and b"sdlt_attn_couple_fwd" in lib.sdlt_last_error()
    for change in REFUSALS:
        p = _lib.AttnCoupleParams()
        for k, v in {**ARGS, **change}.items():
            setattr(p, k, v)
        assert lib.sdlt_attn_couple_fwd(C.byref(p), None) < 0 and b"sdlt_attn_couple_fwd" in lib.sdlt_last_error(), (change, lib.sdlt_last_error())


@pytest.mark.parametrize("what", ["cpu tensors", "bad extent", "too many keys", "wide head", "no kernel", "bad state", "too many regions", "training forward", "missing table", "ctx rows",
                                  "score maps", "sampler bootstrap", "sampler mode", "sampler batch", "render bootstrap", "render mode alone", "cli mode alone", "cli bootstrap"])
def test_refusals(what, tmp_path, capsys):
    if what.startswith(("sampler", "render", "cli")):
        return _section4(what, tmp_path, capsys)
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import topology
    from tests import kvpool_ref as KR
    z, kw = torch.zeros(8, 64, dtype=torch.bfloat16), dict(B=1, H=1, Nq=8, Nk=8, Nkp=8, R=1, d=64, scale=1.0)
    wrapper = {"cpu tensors": {}, "bad extent": dict(Nq=0), "too many keys": dict(Nk=136, Nkp=136), "wide head": dict(d=168)}
    if what in wrapper:
        with pytest.raises(ValueError, match="attn_couple_fwd"):
            ops.attn_couple_fwd(z, z, z, z.clone(), torch.ones(1, 8), **{**kw, **wrapper[what]})
        return
    table = KR.emu_kv if what == "no kernel" else type("T", (), {**vars(KR.emu_kv), "attn_couple_fwd": lambda *a, **k: pytest.fail("launched")})
    unet = unet_mod.UNet(unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=table), topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)
    state = dict(R=2, weights={}, rcount=torch.tensor([2, 2], dtype=torch.int32))
    if what in ("no kernel", "bad state", "too many regions"):
        exc, msg = (NotImplementedError, "sdlt_attn_couple_fwd") if what == "no kernel" else (ValueError, "attention couple")
        with pytest.raises(exc, match=msg):
            unet.set_attention_couple({"no kernel": state, "bad state": dict(R=2, weights={}), "too many regions": dict(state, R=17)}[what])
        return
    if what == "score maps":      # hooked score side outputs (the heat maps' per-layer maps) see one key set per row
        unet.rt.keep_daam_maps = True
        with pytest.raises(ValueError, match="keep_daam_maps"):
            unet.set_attention_couple(state)
        return
    unet.set_attention_couple(state)
    ctx = torch.zeros(2 * (1 if what == "ctx rows" else 2) * unet_mod.CTX_PAD, unet.cfg["cross_dim"])
    exc, msg = {"training forward": (NotImplementedError, "attention couple"), "ctx rows": (ValueError, "ctx has"), "missing table": (ValueError, "no weight table for the 64 tokens")}[what]
    with pytest.raises(exc, match=msg):
        unet.forward(torch.zeros(2 * 64, 64), torch.zeros(2), ctx, B=2, H=8, W=8, train=what == "training forward")


def _section4(what, tmp_path, capsys):
    from sd_lora_trainer_amd import render as R, sampler as SM
    from tests.test_region_cpu import H, W, emu_region, hard_masks
    from tests.test_tilediff_cpu import _embeds, _unet
    box = [((0.0, 0.0, 0.5, 1.0), "a barn")]
    if what.startswith("sampler"):
        tiles = 3 if what == "sampler batch" else 1      # (a runtime of batch 2 n R: the fuse mode's)
        cfg, _, _, rt, unet = _unet("tiny15", 2 * tiles, type("T", (), {**vars(emu_region), "attn_couple_fwd": lambda *a, **k: pytest.fail("launched")}))
        smp = SM.LatentSampler(rt, unet, **({} if tiles == 1 else dict(n_images=1)))
        em = _embeds(cfg, 5, 3)
        rg = dict(masks=hard_masks(), embeds=em[1:], mode="couple")
        kw, msg = {"sampler bootstrap": (dict(regions=dict(rg, bootstrap=2)), "bootstrap must be 0"), "sampler mode": (dict(regions=dict(rg, mode="mix")), "mode must be one of"),
                   "sampler batch": (dict(regions=rg), r"holds 3 window\(s\) per image")}[what]
        with pytest.raises(ValueError, match=msg):
            smp.sample(em[0], H, W, steps=2, **kw)
    elif what.startswith("render"):
        kw, msg = {"render bootstrap": (dict(regions=box, region_mode="couple", region_bootstrap=0.2), "region_bootstrap must be 0"), "render mode alone": (dict(regions=None, region_mode="couple"), "need regions")}[what]
        with pytest.raises(ValueError, match=msg):
            R.region_args(kw.pop("regions"), **kw)
        assert R.region_args(box, region_mode="couple")["bootstrap"] == 0.0 and R.region_args(box)["bootstrap"] == R.REGION_BOOTSTRAP
    else:
        extra, msg = {"cli mode alone": (["--region-mode", "couple"], "need --region"), "cli bootstrap": (["--region", "0,0,0.5,1", "a barn", "--region-mode", "couple", "--region-bootstrap", "0.2"], "region_bootstrap must be 0")}[what]
        with pytest.raises(SystemExit) as e:
            R.main(["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")] + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
