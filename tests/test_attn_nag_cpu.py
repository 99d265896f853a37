"""sdlt_attn_nag_fwd's entry-point validation (no launch: every case is refused before one), its ctypes mirror, and the UNet setter's refusals."""
import ctypes as C
import re
from pathlib import Path

import pytest

from sd_lora_trainer_amd import _lib

BUF = (C.c_char * 4096)()
BASE = (C.addressof(BUF) + 15) & ~15


def _block(**kw):
    p = _lib.AttnNagParams()
    p.Q, p.K, p.V, p.O, p.neg_row, p.tab, p.ctr = BASE, BASE, BASE, BASE + 2048, BASE, BASE, None
    p.ldq = p.ldk = p.ldv = p.ldo = 64
    p.B, p.H, p.Nq, p.Nk, p.Nkp, p.d, p.tab_rows, p.scale = 1, 1, 1, 1, 8, 64, 1, 0.125
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("change,code", [
    (dict(Q=None), -1), (dict(O=None), -1), (dict(neg_row=None), -1), (dict(tab=None), -1), (dict(B=0), -1), (dict(Nq=0), -1), (dict(Nk=0), -1), (dict(d=0), -1),
    (dict(tab_rows=0), -1), (dict(H=21, ldq=21 * 64, ldk=21 * 64, ldv=21 * 64, ldo=21 * 64), -1), (dict(Nk=129, Nkp=136), -1), (dict(Nk=9), -1), (dict(ldq=56), -1),
    (dict(d=168, ldq=168, ldk=168, ldv=168, ldo=168), -1), (dict(d=12), -1), (dict(H=9, d=160, ldq=1440, ldk=1440, ldv=1440, ldo=1440), -1), (dict(O=BASE), -1),
    (dict(B=1 << 30, Nq=4), -1), (dict(Nkp=12, Nk=9), -2), (dict(ldo=68), -2), (dict(K=BASE + 8), -2), (dict(tab=BASE + 2), -2), (dict(ctr=BASE + 1), -2)])
def test_entry_refuses_before_any_launch(change, code):
    lib = _lib.load()
    assert lib.sdlt_attn_nag_fwd(C.byref(_block(**change)), None) == code
    assert b"sdlt_attn_nag_fwd" in lib.sdlt_last_error()


def test_null_block_and_mirror_size():
    assert _lib.load().sdlt_attn_nag_fwd(None, None) == -1
    text = (Path(__file__).resolve().parents[1] / "include" / "sdlt_kernels.h").read_text()
    assert C.sizeof(_lib.AttnNagParams) == int(re.search(r"\} sdlt_attn_nag_params;\s*/\* (\d+) bytes", text).group(1)) == 120
    assert "sdlt_attn_nag_fwd" in _lib.SYMBOLS and "AttnNagParams" not in [n for n, _ in _lib.struct_sizes()]


def test_unet_setter_refusals():
    import types
    from sd_lora_trainer_amd import unet as M
    u = M.UNet.__new__(M.UNet)
    u.cross_attns, u._nag = [types.SimpleNamespace(_nag=None)], None
    u.rt = types.SimpleNamespace(ops=types.SimpleNamespace())      # an op table without the kernel
    with pytest.raises(NotImplementedError, match="sdlt_attn_nag_fwd"):
        u.set_attention_nag(dict(neg_row=0, tab=0, ctr=None))
    with pytest.raises(ValueError, match="neg_row=, tab=, ctr="):
        u.set_attention_nag(dict(neg_row=0))
    u.rt.ops.attn_nag_fwd = lambda *a, **k: None
    u.set_attention_nag(dict(neg_row=1, tab=2, ctr=None))
    assert u.cross_attns[0]._nag == dict(neg_row=1, tab=2, ctr=None) == u._nag
    u.set_attention_nag(None)
    assert u.cross_attns[0]._nag is None and u._nag is None


def test_nag_table_and_rows():
    import torch
    from sd_lora_trainer_amd import sampler as SM
    tab = SM.nag_table([14.6, 3.0, 1.0, 0.5], 5.0, 2.5, 0.5, 1.0)      # guided while sigma > end: rows 2 and 3 are plain (alpha 0); no header row
    assert tab.dtype == torch.float32 and tab.tolist() == [[5.0, 2.5, 0.5, 0.0], [5.0, 2.5, 0.5, 0.0], [5.0, 2.5, 0.0, 0.0], [5.0, 2.5, 0.0, 0.0]]
    assert SM.nag_table([14.6, 0.03], 3.0, 1.0, 0.25, 0.0)[:, 2].tolist() == [0.25, 0.25]      # end 0: every step
    assert SM.nag_rows(3).dtype == torch.int32 and SM.nag_rows(3).tolist() == [-1, 0, -1, 2, -1, 4]      # (negative j, positive j) pairs
    assert SM.nag_args(True) == SM.NAG_DEFAULT == (5.0, 2.5, 0.5, 0.0) and SM.nag_args(None) is None and SM.nag_args(3) == (3.0, 2.5, 0.5, 0.0)
    for bad in (dict(scale=0.5), dict(tau=0.0), dict(alpha=1.5), dict(end=-1.0), dict(beta=1), "on"):
        with pytest.raises(ValueError, match="nag"):
            SM.nag_args(bad)


@pytest.mark.parametrize("kws,exc,msg", [
    (dict(regions=dict(mode="fuse")), ValueError, "nag does not combine with regions"), (dict(regions=dict(mode="couple")), ValueError, "nag does not combine with regions"),
    (dict(tile=4), ValueError, "nag does not combine with tile"), (dict(nag=dict(tau=-1.0)), ValueError, "tau > 0"), (dict(no_kernel=True), NotImplementedError, "sdlt_attn_nag_fwd")])
def test_sampler_refusals(kws, exc, msg):
    from oracle import unet_ref as U
    from sd_lora_trainer_amd import sampler as SM
    from tests.test_style_align_cpu import _unet
    from tests.test_tilediff_cpu import _embeds
    kws = dict(kws)
    unet = _unet({} if kws.pop("no_kernel", False) else dict(attn_nag_fwd=lambda *a, **k: pytest.fail("launched")))
    smp = SM.LatentSampler(unet.rt, unet)
    with pytest.raises(exc, match=msg):
        smp.sample(**{**dict(embeds=_embeds(U.CONFIGS["tiny15"], 5, 2), h=8, w=8, steps=2, n_images=2, fused=True, nag=True), **kws})
    assert smp._fused is None and unet._nag is None      # refused before the UNet is touched


def test_render_and_cli_arguments(tmp_path, capsys):
    from sd_lora_trainer_amd import render as R
    assert R.nag_args(True) == (5.0, 2.5, 0.5, 0.0) and R.nag_args(3.0, alpha=0.0, end=1.5) == (3.0, 2.5, 0.0, 1.5) and R.nag_args(None) is None
    with pytest.raises(ValueError, match="need nag"):
        R.nag_args(None, tau=2.0)
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--nag", "--region", "0,0,1,1", "a barn"], "--nag does not combine with --region"), (["--nag", "--tile-diffusion"], "--nag does not combine with --tile-diffusion"),
                       (["--nag-alpha", "0.3"], "need nag"), (["--nag", "0.5"], "scale >= 1")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
