"""sdlt_attn_wide_fwd's refusals (host checks only: nothing is launched, no GPU here) and the `attention=` / `vae_attention=` settings' own checks."""
import ctypes as C
import types

import pytest
import torch

from tests import emu_ops
from tests.test_guidance_cpu import _FakeLoaded
from tests.test_vaetile_cpu import _vae


@pytest.mark.parametrize("change,word", [(dict(d=256), b"d=256"), (dict(ldk=516), b"ld % 8"), (dict(V=None), b"null"), (dict(Nk=0), b"Nk=0")])
def test_entry_point_refuses(change, word):
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    q, k, v = (torch.zeros(8, 512, dtype=torch.bfloat16) for _ in range(3))
    out = torch.full((8, 512), 3.0, dtype=torch.bfloat16)
    p = _lib.AttnWideParams()
    p.Q, p.K, p.V, p.O = (C.c_void_p(t.data_ptr()) for t in (q, k, v, out))
    p.ldq = p.ldk = p.ldv = p.ldo = 512
    p.B, p.Nq, p.Nk, p.d, p.scale = 1, 8, 8, 512, 0.04
    for name, val in change.items():
        setattr(p, name, val)
    assert lib.sdlt_attn_wide_fwd(C.byref(p), None) != 0
    msg = lib.sdlt_last_error()
    assert b"sdlt_attn_wide_fwd" in msg and word in msg, msg
    assert bool((out == 3.0).all())


def test_settings_are_checked_before_anything_is_built(tmp_path):
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import unet as M
    from sd_lora_trainer_amd import vae
    from oracle import vae_ref as V
    with pytest.raises(ValueError, match="nope"):
        R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), vae_attention="nope")
    assert not (tmp_path / "o").exists()
    rt = M.Runtime("cpu", 1, act_dtype=torch.float32, ops=emu_ops)
    with pytest.raises(ValueError, match="nope"):
        vae.VaeDecoder(rt, {}, attention="nope")
    with pytest.raises(NotImplementedError, match="sdlt_attn_wide_fwd"):      # the emulated op table has no such kernel, and there is no torch fallback
        vae.VaeEncoder(rt, {}, attention="flash")
    assert _vae(emu_ops)[1].mid.attn.attention == "dense"                     # the default
    sd = V.init_state(dict(V.CONFIGS["tiny"], block_out_channels=(32, 64)), seed=0)
    have = types.SimpleNamespace(**dict(vars(emu_ops), attn_wide_fwd=None))
    with pytest.raises(ValueError, match="64 wide"):                           # a mid width the kernel is not built for
        vae.VaeDecoder(M.Runtime("cpu", 1, act_dtype=torch.float32, ops=have), sd, attention="flash")
