"""Style-aligned batches without a device: the refusals of the two entry points, of the wrappers, of UNet.set_shared_attention, of sample, render and the CLI,
and render's batch plan."""
import ctypes as C

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops, render as R, sampler as SM

ATTN = dict(Q=0x10000, ldq=384, K=0x10100, ldk=384, V=0x10200, ldv=384, O=0x400000, ldo=128, Aq=0x800000, Sq=0x800400, Ak=0x800200, Sk=0x800600, ldt=256,
            B=4, H=2, N=80, d=64, G=2, gs=1, scale=0.125, shift=0.5)
ATTN_REFUSALS = [(dict(Q=None), -1), (dict(K=None), -1), (dict(V=None), -1), (dict(O=None), -1), (dict(Sk=None), -1), (dict(B=0), -1), (dict(H=0), -1), (dict(N=0), -1),
                 (dict(d=0), -1), (dict(G=0), -1), (dict(gs=0), -1), (dict(G=3), -1), (dict(gs=4), -1), (dict(shift=float("inf")), -1), (dict(shift=float("nan")), -1),
                 (dict(scale=0.0), -1), (dict(ldo=120), -1), (dict(ldk=64), -1), (dict(ldt=64), -1), (dict(O=0x10300), -1), (dict(B=2 ** 16, N=2 ** 15), -1),
                 (dict(ldq=388), -2), (dict(ldt=258), -2), (dict(Q=0x10008), -2), (dict(Ak=0x800204), -2), (dict(d=36), -4),
                 (dict(d=168, ldq=1024, ldk=1024, ldv=1024, ldo=336, ldt=336), -4)]
ADAIN = dict(X=0x10000, ld=384, A=0x400000, S=0x500000, ws=0x600000, B=4, N=80, C2=256, G=2, gs=1)
ADAIN_REFUSALS = [(dict(X=None), -1), (dict(A=None), -1), (dict(S=None), -1), (dict(ws=None), -1), (dict(B=0), -1), (dict(N=1), -1), (dict(C2=0), -1), (dict(G=3), -1),
                  (dict(gs=0), -1), (dict(ld=128), -1), (dict(C2=260), -2), (dict(ld=388), -2), (dict(X=0x10008), -2), (dict(A=0x400002), -2)]


@pytest.mark.parametrize("entry,cls,args,refusals", [("sdlt_attn_shared_fwd", "AttnSharedParams", ATTN, ATTN_REFUSALS), ("sdlt_adain_affine", "AdainAffineParams", ADAIN, ADAIN_REFUSALS)])
def test_entry_point_validation(entry, cls, args, refusals):
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, entry)
    assert fn(None, None) == -1 and entry.encode() in lib.sdlt_last_error()
    for change, code in refusals:
        p = getattr(_lib, cls)()
        for k, v in {**args, **change}.items():
            setattr(p, k, v)
        assert fn(C.byref(p), None) == code and entry.encode() in lib.sdlt_last_error(), (change, lib.sdlt_last_error())


def _unet(table_extra):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import topology
    from tests import kvpool_ref as KR
    table = type("T", (), {**vars(KR.emu_kv), **table_extra})
    return unet_mod.UNet(unet_mod.Runtime("cpu", 4, act_dtype=torch.float32, ops=table), topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)


LAUNCHED = dict(attn_shared_fwd=lambda *a, **k: pytest.fail("launched"), adain_affine=lambda *a, **k: pytest.fail("launched"))
STATE = dict(group=2, shift=0.0, adain=True)


@pytest.mark.parametrize("what", ["wrapper cpu tensors", "wrapper groups", "wrapper shift", "wrapper head", "adain one token", "adain groups", "no kernel", "bad keys", "bad group",
                                  "bad shift", "kv clash", "hypertile clash", "tome clash", "probe clash", "kv clash reversed", "batch not divided", "training forward",
                                  "backward", "sampler one image", "sampler weight", "sampler sag", "sampler tile", "sampler hypertile", "sampler torch loop",
                                  "sampler no kernel", "render one per batch", "render weight", "render adain alone", "render adain", "cli one per batch", "cli sag"])
def test_refusals(what, tmp_path, capsys):
    z, kw = torch.zeros(64, 64, dtype=torch.bfloat16), dict(B=2, H=1, N=32, d=64, G=2, scale=1.0)
    wrapper = {"wrapper cpu tensors": {}, "wrapper groups": dict(G=3), "wrapper shift": dict(shift=float("nan")), "wrapper head": dict(d=168)}
    if what in wrapper:
        with pytest.raises(ValueError, match="attn_shared_fwd"):
            ops.attn_shared_fwd(z, z, z, z.clone(), **{**kw, **wrapper[what]})
        return
    if what.startswith("adain"):
        with pytest.raises(ValueError, match="adain_affine"):
            ops.adain_affine(z, torch.zeros(2, 64), torch.zeros(2, 64), **dict(dict(B=2, N=32, G=2), **(dict(B=64, N=1) if what == "adain one token" else dict(G=3))))
        return
    if what.startswith("render"):
        a, msg = {"render one per batch": ((True, None, None, 1), "at least 2"), "render weight": ((0.0,), "finite and > 0"),
                  "render adain alone": ((None, None, "qk"), "need style_align"), "render adain": ((True, None, "v"), "one of")}[what]
        with pytest.raises(ValueError, match=msg):
            R.style_align_args(*a)
        assert R.style_align_args(True, images_per_batch=2) == dict(weight=1.0, adain="qk") and R.style_align_args(0.5, None, "none") == dict(weight=0.5, adain="none")
        return
    if what.startswith("cli"):
        extra, msg = {"cli one per batch": (["--style-align"], "at least 2"), "cli sag": (["--style-align", "--images-per-batch", "2", "--sag"], "--sag")}[what]
        with pytest.raises(SystemExit) as e:
            R.main(["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")] + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
        return
    unet = _unet({} if "no kernel" in what else LAUNCHED)
    if what.startswith("sampler"):
        from oracle import unet_ref as U
        from tests.test_tilediff_cpu import _embeds
        smp, em = SM.LatentSampler(unet.rt, unet), _embeds(U.CONFIGS["tiny15"], 5, 2)
        exc, kws, msg = {"sampler one image": (ValueError, dict(n_images=1), "at least 2"), "sampler weight": (ValueError, dict(style_align=dict(weight=0.0)), "weight"),
                         "sampler sag": (ValueError, dict(sag=True), "does not combine with sag"), "sampler tile": (ValueError, dict(tile=4), "does not combine with tile"),
                         "sampler hypertile": (ValueError, dict(hypertile=dict(tile=4)), "does not combine with hypertile"),
                         "sampler torch loop": (ValueError, dict(fused=False), "fused=True or graph=True"),
                         "sampler no kernel": (NotImplementedError, {}, "sdlt_attn_shared_fwd")}[what]
        with pytest.raises(exc, match=msg):
            smp.sample(**{**dict(embeds=em, h=8, w=8, steps=2, n_images=2, fused=True, style_align=True), **kws})
        assert smp._fused is None and unet._share is None      # refused before the UNet is touched
        return
    if what in ("no kernel", "bad keys", "bad group", "bad shift", "kv clash", "hypertile clash", "tome clash", "probe clash"):
        if what == "kv clash":
            unet.set_kv_downsample((1, 2))
        if what == "probe clash":
            unet.set_attention_probe(True)
        if what in ("hypertile clash", "tome clash"):
            unet.rt.ops = type("T", (unet.rt.ops,), dict(attn_window_fwd=None, tome_match=1, tome_plan=1, tome_merge=1, tome_unmerge=1))
            unet._ht = ((2, 2),) if what == "hypertile clash" else None
            unet._tome = ((0.5,), "fixed", 0) if what == "tome clash" else None
        exc, msg, state = {"no kernel": (NotImplementedError, "sdlt_attn_shared_fwd", STATE), "bad keys": (ValueError, "takes dict", dict(group=2, shift=0.0)),
                           "bad group": (ValueError, "group=0", dict(STATE, group=0)), "bad shift": (ValueError, "shift=", dict(STATE, shift=float("inf"))),
                           "kv clash": (ValueError, "kv_downsample is set", STATE), "hypertile clash": (ValueError, "hypertile is set", STATE),
                           "tome clash": (ValueError, "token_merge is set", STATE), "probe clash": (ValueError, "attention probe is set", STATE)}[what]
        with pytest.raises(exc, match=msg):
            unet.set_shared_attention(state)
        assert unet._share is None
        return
    names = unet.set_shared_attention(STATE)
    assert len(names) >= 3 and all(n.endswith("attn1") for n in names) and unet._share == dict(STATE, stride=1)
    if what == "kv clash reversed":
        with pytest.raises(ValueError, match="set_shared_attention"):
            unet.set_kv_downsample((2,))
        assert unet.set_shared_attention(None) == {} and unet._share is None and unet.set_kv_downsample((2,))
        return
    if what == "backward":
        with pytest.raises(NotImplementedError, match="shared attention"):
            unet.backward(None, None)
        return
    B = 3 if what == "batch not divided" else 4
    exc, msg = (ValueError, "do not divide the batch of 3 rows") if what == "batch not divided" else (NotImplementedError, "shared attention is an inference option")
    with pytest.raises(exc, match=msg):
        unet.forward(torch.zeros(B * 64, 64), torch.zeros(B), torch.zeros(B * unet_mod.CTX_PAD, unet.cfg["cross_dim"]), B=B, H=8, W=8, train=what == "training forward")


@pytest.mark.parametrize("n_prompts,n", [(1, 2), (2, 2), (5, 2), (7, 3), (4, 4), (9, 4)])
def test_render_batch_plan(n_prompts, n):
    plan = R.batch_plan(n_prompts, n, True)
    assert all(len(idx) == n and idx[0] == 0 and all(0 <= i < n_prompts for i in idx) for idx, _ in plan)      # prompt 0 leads every batch
    assert sorted(idx[j] for idx, keep in plan for j in keep) == list(range(n_prompts))                          # every picture is saved once
    assert all(0 not in keep for _, keep in plan[1:])                                                            # picture 0 from the first batch only
    assert R.batch_plan(n_prompts, n) == [([min(s + j, n_prompts - 1) for j in range(n)], list(range(min(n, n_prompts - s)))) for s in range(0, n_prompts, n)]
