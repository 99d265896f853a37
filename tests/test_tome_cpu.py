"""Token merging without a device: the r rule, the fixed-mode destinations against a worked example, and the refusals of the entry points, of
UNet.set_token_merge, of sample, render and the CLI."""
import ctypes as C

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from sd_lora_trainer_amd import ops, sampler as SM


# fixed mode on a 4 x 6 grid, by hand: token rows 0 and 2 hold the cells' top-left corners, at columns 0, 2, 4 (tests/test_tome_gpu.py holds dst_tok to it)
FIXED_4X6 = [0, 2, 4, 12, 14, 16]


def test_r_rule():
    # 60 tokens: floor(30) = 30 leaves 30 rows, lowered to 28 (32 rows); 256 and 1024: half; 0.75: N_src where N / 4 is a multiple of 8, else lowered
    assert [ops.tome_rows(N, 0.5) for N in (60, 256, 1024)] == [28, 128, 512]
    assert [ops.tome_rows(N, 0.75) for N in (60, 256, 1024)] == [44, 192, 768]
    assert ops.tome_rows(16, 0.1) <= 0 and ops.tome_rows(64, 0.0) == 0 and ops.tome_rows(12, 0.3) <= 0      # r <= 0: the plain path


MATCH = dict(y=0x10000, ld=72, ctr=0x90000, dst_tok=0x100000, node_max=0x200000, node_idx=0x300000, seed=1, B=2, Hg=6, Wg=10, C=64, mode=1, layer=0)
PLAN = dict(node_max=0x10000, node_idx=0x20000, dst_tok=0x30000, map=0x40000, kept_tok=0x50000, offsets=0x60000, list=0x70000, B=2, Hg=6, Wg=10, r=28)
MERGE = dict(y=0x10000, ld=72, dst_tok=0x90000, kept_tok=0xa0000, offsets=0xb0000, list=0xc0000, ym=0x100000, ldm=64, B=2, Hg=6, Wg=10, C=64, r=28)
UNMERGE = dict(residual=0x10000, ldr=64, a=0x100000, lda=64, map=0x200000, out=0x300000, ldo=64, B=2, N=60, Np=32, C=64)
REFUSALS = [("match", MATCH, [(dict(y=None), -1), (dict(ctr=None), -1), (dict(node_idx=None), -1), (dict(B=0), -1), (dict(Hg=5), -1), (dict(Wg=7), -1), (dict(ld=56), -1),
                              (dict(Hg=256, Wg=256), -1), (dict(node_max=0x10010), -1), (dict(ld=76), -2), (dict(C=60), -2), (dict(y=0x10008), -2), (dict(mode=2), -4)]),
            ("plan", PLAN, [(dict(map=None), -1), (dict(list=None), -1), (dict(Hg=7), -1), (dict(r=-4), -1), (dict(r=46), -1), (dict(r=30), -1), (dict(map=0x10000), -1),
                            (dict(kept_tok=0x40010), -1), (dict(offsets=0x60002), -2)]),
            ("merge", MERGE, [(dict(ym=None), -1), (dict(Wg=9), -1), (dict(r=30), -1), (dict(ldm=56), -1), (dict(ym=0x10040), -1), (dict(C=0), -1), (dict(ldm=68), -2),
                              (dict(ym=0x100008), -2)]),
            ("unmerge", UNMERGE, [(dict(a=None), -1), (dict(N=0), -1), (dict(Np=61), -1), (dict(lda=56), -1), (dict(out=0x10040), -1), (dict(B=2 ** 20, N=2 ** 12), -1),
                                  (dict(ldo=68), -2), (dict(map=0x200002), -2)])]


@pytest.mark.parametrize("name,base,cases", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_point_validation(name, base, cases):
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    fn, cls = getattr(lib, "sdlt_tome_" + name), getattr(_lib, f"Tome{name.capitalize()}Params")
    assert fn(None, None) == -1 and b"sdlt_tome_" + name.encode() in lib.sdlt_last_error()
    for change, code in cases:
        p = cls()
        for k, v in {**base, **change}.items():
            setattr(p, k, v)
        assert fn(C.byref(p), None) == code and b"sdlt_tome_" + name.encode() in lib.sdlt_last_error(), (change, lib.sdlt_last_error())


def test_render_args():
    from sd_lora_trainer_amd import render as R
    for a, msg in (((0.9,), "0.75"), ((None, 1), "need tome"), ((0.5, 0, None, "hires"), "has none")):
        with pytest.raises(ValueError, match=msg):
            R.tome_args(*a)
    assert R.tome_args(True, hires=True) == dict(ratio=0.5, depth=0, mode="random", passes="hires") and R.tome_args(0.25)["passes"] == "all"


@pytest.mark.parametrize("extra,msg", [(["--tome", "0.9"], "0.75"), (["--tome-mode", "fixed"], "need tome"), (["--tome", "--tome-pass", "hires"], "has none"),
                                       (["--tome", "--hypertile"], "does not combine with --hypertile"),
                                       (["--tome", "--tome-depth", "1", "--kv-downsample", "1", "2", "--kv-downsample-pass", "all"], "same token grid")])
def test_cli_refusals(extra, msg, tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    with pytest.raises(SystemExit) as e:
        R.main(["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")] + extra)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def _unet(kernels):      # a CPU tiny15 UNet on the emulated op table, with or without token-merging entries (which fail the test when launched)
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import topology
    from tests import kvpool_ref as KR
    launched = lambda *a, **k: pytest.fail("launched")  # noqa: E731
    table = type("T", (), {**vars(KR.emu_kv), **{n: launched for n in ("tome_match", "tome_plan", "tome_merge", "tome_unmerge")}}) if kernels else KR.emu_kv
    return unet_mod.UNet(unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=table), topology.CONFIGS["tiny15"], U.init_unet_state(U.CONFIGS["tiny15"], seed=0), lora_rank=4)


@pytest.mark.parametrize("kernels,exc,msg,args,kw", [
    (False, NotImplementedError, "sdlt_tome_match", ((0.5,),), {}), (True, ValueError, r"ratios in \[0, 0.75\]", ((0.8,),), {}),
    (True, ValueError, "mode must be one of", ((0.5,),), dict(mode="nearest")), (True, ValueError, "4 ratios", ((0.5,) * 4,), {}),
    (True, ValueError, "token grid of down_blocks.1.attentions.0 is odd", ((0.5, 0.5),), dict(latent=(12, 6))),
    (True, ValueError, "kv_downsample factor 2", ((0.5, 0.5),), dict(kv=(1, 2)))])
def test_set_token_merge_refusals(kernels, exc, msg, args, kw):
    unet = _unet(kernels)
    if "kv" in kw:
        unet.set_kv_downsample(kw.pop("kv"))
    with pytest.raises(exc, match=msg):
        unet.set_token_merge(*args, **kw)
    assert unet._tome is None


@pytest.mark.parametrize("kernels,exc,tm,msg", [(True, ValueError, dict(ratios=0.5), "token_merge takes"), (False, NotImplementedError, dict(ratio=0.5), "sdlt_tome_match")])
def test_sampler_refusals(kernels, exc, tm, msg):
    from oracle import unet_ref as U
    from tests.test_tilediff_cpu import _embeds
    unet = _unet(kernels)
    with pytest.raises(exc, match=msg):
        SM.LatentSampler(unet.rt, unet).sample(_embeds(U.CONFIGS["tiny15"], 5, 1)[0], 8, 8, steps=2, token_merge=tm)


@pytest.mark.parametrize("ratio,hw,train,exc,msg", [(0.5, 9, False, ValueError, "down_blocks.0.attentions.0.*needs an even token grid"), (0.1, 8, False, None, None),
                                                    (0.5, 8, True, NotImplementedError, "token_merge is an inference option"), (0.5, 8, None, NotImplementedError, "token_merge")])
def test_forward_refusals(ratio, hw, train, exc, msg):
    # train None: the backward; ratio 0.1 of 64 or 16 tokens merges nothing: every layer stays plain and nothing is launched
    unet = _unet(True)
    assert sorted(unet.set_token_merge((ratio, 0.0))) == ["down_blocks.0.attentions.0", "up_blocks.2.attentions.0", "up_blocks.2.attentions.1"] and unet._tome == ((ratio,), "random", 0)
    fwd = lambda: unet.forward(torch.zeros(2 * hw * hw, 64), torch.zeros(2), torch.zeros(2 * unet_mod.CTX_PAD, unet.cfg["cross_dim"]), B=2, H=hw, W=hw, train=train)  # noqa: E731
    if exc is None:
        assert fwd().shape[0] == 2 * hw * hw
        return
    with pytest.raises(exc, match=msg):
        unet.backward(None, None) if train is None else fwd()
