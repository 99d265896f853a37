"""Which attention kernel a call runs, pinned without a GPU: sdlt_attn_route is the host-side plan of sdlt_attn_fwd / sdlt_attn_bwd
(attn_plan_fwd / attn_plan_bwd in csrc/attn.hip) and launches nothing.  The parity tests compare numbers only, so a threshold edit that
moves a shape onto another kernel passes them; this file is what notices.  Cases: ATTN_CASES of test_kernels_gpu.py, in list order."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from sd_lora_trainer_amd import _lib
from tests.test_kernels_gpu import ATTN_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4      # csrc/common.h
POINTERS = ("Q", "K", "V", "O", "L", "dO", "D", "dQ", "dK", "dV", "dK32", "dV32")
LDS = ("ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv", "ld32")


def params(c, **over):
    """The parameter block test_attention_fwd_bwd builds for case c (256-byte-aligned made-up addresses: nothing dereferences them)."""
    p = _lib.AttnParams()
    for i, name in enumerate(POINTERS):
        setattr(p, name, 0x100000 + 256 * i)
    for name in LDS:
        setattr(p, name, c["H"] * c["d"])
    p.B, p.H, p.Nq, p.Nk, p.Nkp, p.d = c["B"], c["H"], c["Nq"], c["Nk"], c["Nkp"], c["d"]
    p.Nqp = (c["Nq"] + 7) // 8 * 8
    p.scale, p.qsplit, p.causal = c["d"] ** -0.5, c["qsplit"], int(c["causal"])
    p.accumulate_dq = p.accumulate_dk = int(bool(c.get("accumulate")))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def route(c, backward, **over):
    """Decoded route of case c (a dict), or the negative error code."""
    code = _lib.load().sdlt_attn_route(ctypes.byref(params(c, **over)), backward)
    return code if code < 0 else _lib.attn_route_decode(code)


def all_routes():
    return [[route(c, 0), route(c, 1)] for c in ATTN_CASES]


def R(name, dp=64, ks=1, dv48=False, five=False, prep=False, splitsum=False):
    return dict(route=name, dp=dp, ks=ks, dv48=dv48, five=five, prep=prep, splitsum=splitsum)


SELF32 = (R("FWD32", ks=2), R("BWD_BOTH32", ks=2, prep=True))
DEFAULT = [
    SELF32,
    (R("FWD16"), R("BWD_CROSS_ROLES", five=True, splitsum=True)),
    (R("FWD16"), R("BWD_BOTH16", prep=True)),
    (R("FWD16", dp=96), R("BWD_CROSS", dp=96, five=True, splitsum=True)),
    (R("FWD16", dv48=True), R("BWD_CROSS_ROLES", splitsum=True)),
    (R("FWD16"), R("BWD_CROSS_ROLES", five=True, splitsum=True)),
    (R("FWD16_KS2", ks=2), R("BWD_BOTH16", prep=True)),
    (R("FWD16", dp=160), R("BWD_BOTH16", dp=160, prep=True)),
    (R("FWD16", dp=96), R("BWD_BOTH16", dp=96, prep=True)),
    (R("FWD16"), R("BWD_BOTH16", prep=True)),
    SELF32,
    (R("FWD32", ks=1), R("BWD_BOTH32", ks=1, prep=True)),
    SELF32,
    SELF32,
    SELF32,
    (R("FWD16", dp=160), R("BWD_SPLIT", dp=160, splitsum=True)),
    (R("FWD16", dv48=True), R("BWD_SPLIT", dv48=True)),
]


def test_default_switches_route_every_case():
    switches = sorted(k for k in os.environ if k.startswith(("SDLT_ATTN", "SDLT_XATTN")))      # (the table below is the one of the defaults)
    assert len(DEFAULT) == len(ATTN_CASES)
    got = all_routes()
    for i, (c, g, want) in enumerate(zip(ATTN_CASES, got, DEFAULT)):
        assert tuple(g) == want, f"case {i + 1} {c} (switches set in the environment: {switches})"
    assert {r["route"] for g in got for r in g} == set(_lib.ATTN_ROUTES), "a route no case reaches"


def test_threshold_edges():
    c1, c2 = ATTN_CASES[0], ATTN_CASES[1]
    # 16-byte epilogue stores of the 32-row kernels: a misaligned output keeps the call on the 16-row kernels
    assert route(c1, 0, O=0x100008) == R("FWD16_KS2", ks=2)
    assert route(c1, 1, dK=0x100008) == R("BWD_BOTH16", prep=True)
    assert route(c1, 1, d_ready=1) == R("BWD_BOTH32", ks=2)
    assert route(c2, 1, defer_splitsum=1) == R("BWD_CROSS_ROLES", five=True)
    # the 32-row backward stores the rows of its key tiles only: pad keys behind whole tiles keep the backward on the 16-row kernel (which zeroes their dK / dV rows)
    x = dict(B=1, H=2, Nq=192, Nk=64, Nkp=72, d=64, causal=False, qsplit=1)
    assert route(x, 0) == R("FWD32", ks=1) and route(x, 1) == R("BWD_BOTH16", prep=True)
    # five 16-key blocks: 64 < Nk <= 80
    for Nk, five in ((64, False), (65, True), (80, True), (81, False)):
        x = dict(B=1, H=2, Nq=128, Nk=Nk, Nkp=128, d=64, causal=False, qsplit=2)
        assert route(x, 1) == R("BWD_CROSS_ROLES", five=five, splitsum=True), Nk
    # one backward launch up to (ceil(Nq / 64) + ceil(Nk / 64)) * H * B = 2048 workgroups, dQ and dK / dV launches beyond
    assert route(dict(B=8, H=8, Nq=1024, Nk=1024, Nkp=1024, d=64, causal=False, qsplit=1), 1) == R("BWD_BOTH32", ks=2, prep=True)      # 32 * 64 = 2048
    assert route(dict(B=1, H=683, Nq=128, Nk=64, Nkp=64, d=64, causal=False, qsplit=1), 1) == R("BWD_SPLIT")                             # 3 * 683 = 2049
    # the forward's key split up to 512 workgroups
    assert route(dict(B=1, H=8, Nq=4096, Nk=256, Nkp=256, d=40, causal=False, qsplit=1), 0) == R("FWD16_KS2", ks=2)                      # 64 * 8 = 512
    assert route(dict(B=1, H=19, Nq=1728, Nk=256, Nkp=256, d=40, causal=False, qsplit=1), 0) == R("FWD16", dv48=True)                    # 27 * 19 = 513


@pytest.mark.parametrize("over,code,entry", [(dict(accumulate_dq=1), ERR_UNSUPPORTED, 1), (dict(accumulate_dk=1), ERR_UNSUPPORTED, 1),
                                             (dict(d=168), ERR_SHAPE, 0), (dict(d=168), ERR_SHAPE, 1), (dict(ldq=4), ERR_ALIGN, 0), (dict(ldq=4), ERR_ALIGN, 1)])
def test_refusals_are_those_of_the_launch_entry(over, code, entry):
    assert route(ATTN_CASES[0], entry, **over) == code
    assert (b"sdlt_attn_bwd" if entry else b"sdlt_attn_fwd") in _lib.load().sdlt_last_error()


def _child(env):
    """all_routes() of a fresh interpreter under `env` (the switches are read once per process); the child never touches a GPU."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.test_attn_route_cpu"], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_fallback_switches():
    got = _child(dict(SDLT_ATTN_R32="0", SDLT_ATTN_KS="1", SDLT_ATTN_DV48="0", SDLT_XATTN_ROLES="0", SDLT_XATTN_FIVE="0"))
    assert len(got) == len(ATTN_CASES)
    for g in got:
        for r in g:
            assert r["route"] not in ("FWD32", "FWD16_KS2", "BWD_BOTH32", "BWD_CROSS_ROLES") and not r["dv48"] and not r["five"], r
    assert got[0] == [R("FWD16"), R("BWD_BOTH16", prep=True)]
    assert got[1][1] == R("BWD_CROSS", splitsum=True)


def test_wave_group_switches():
    got = _child(dict(SDLT_ATTN32_KS_FWD="4", SDLT_ATTN32_KS_BWD="1"))
    assert got[13] == [R("FWD32", ks=4), R("BWD_BOTH32", ks=1, prep=True)]


if __name__ == "__main__":
    print(json.dumps(all_routes()))
