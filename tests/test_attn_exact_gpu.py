"""Bit-exact parity of the attention kernels (MI355X): sdlt_attn_fwd / sdlt_attn_bwd on every route of attn_plan_fwd / attn_plan_bwd and
sdlt_attn_splitsum_batch, against the fp64 reference of tests/attn_exact_ref.py on operands whose softmax rows tie exactly (1, 2, 4 or 8 winners, every
loser past the fp32 underflow; tests/test_attn_exact_cpu.py proves that every rounding a kernel performs then lands on the exact value).  O, dQ, dK, dV
and the fp32 slabs dK32 / dV32 compare with torch.equal - no tolerance; only L = logsumexp has one, derived from its five roundings (R.l_bound).
scale = 0.125 for every head width.  Every operand is a production-shaped view: Q | K | V column slices of one [rows, 3 C + 16] buffer, dQ | dK | dV likewise,
O and dO slices of wider buffers; everything around an input is NaN (stray reads), pad rows inside it hold finite bait (pad keys carry a class code that
would beat every winner and V = 96; pad queries a class code and dO = 2; O pad rows 5), outputs are NaN-filled views of sentinel-filled buffers with a
64-row tile of slack behind them (stray writes).  Before every launch sdlt_attn_route is asked about the very block that is launched, and under the default
switches its answer must be the route the case names; under SDLT_ATTN_* / SDLT_XATTN_* switches (test_fallback_kernel_paths_in_a_subprocess) the planner's
answer is taken as it comes and the same bits are required of the fallback kernels.

Route / variant                                   case (tests/attn_exact_ref.py CASES)                     tests
  FWD32 ks 2 / BWD_BOTH32 ks 2                      self32_ks2  B2 H2 256 x 256 d64                          test_forward_backward, test_d_ready
  FWD32 ks 1 / BWD_BOTH32 ks 1                      self32_ks1  192 x 64 d64                                 test_forward_backward, test_d_ready
  FWD32 / BWD_BOTH16: pad keys behind whole tiles   self32_pad_keys  192 x 64 (Nkp 72) d64                   test_forward_backward, test_d_ready
  FWD16_KS2 / BWD_BOTH16 by misalignment            self32_misaligned  the same, outputs 8 bytes off         test_forward_backward, test_d_ready
  FWD16_KS2 / BWD_BOTH16, d40 in 64 columns         ks2_d40  B1 H8 250 x 257 (264) d40                       test_forward_backward, test_d_ready
  FWD16 dp 64, four key tiles, the last of one key  self16_more_keys  100 x 193 (200) d64                    test_forward_backward, test_d_ready
  FWD16 / BWD_BOTH16 dp 96                          dp96  100 x 129 (136) d80                                test_forward_backward, test_d_ready
  FWD16 / BWD_BOTH16 dp 160 (single LDS buffer)     dp160  130 x 130 (136) d160                              test_forward_backward, test_d_ready
  BWD_CROSS_ROLES five, Nkp 80, qsplit 2            cross_five_80  200 x 77                                  test_forward_backward, test_cross_accumulate, test_deferred_splitsum
  BWD_CROSS_ROLES five, Nkp 128, qsplit 4           cross_five_128  B2 H3 300 x 77 (an empty last split)     the same three
  BWD_CROSS_ROLES, 64 keys                          cross_64_keys  136 x 64, qsplit 3                        the same three
  FWD16 dv48 / BWD_CROSS_ROLES at d40               cross_dv48  68 x 40 d40, qsplit 2                        the same three
  BWD_CROSS dp 96 five                              cross_dp96  B2 H3 200 x 77 (128) d80, qsplit 3           the same three
  BWD_SPLIT with slabs, dp 160                      split_slabs  B2 H2 316 x 77 (128) d160, qsplit 4         test_forward_backward (slabs compared, pad rows zero)
  BWD_SPLIT by workgroup count, d64 (FWD32 ks 1)    split_grid_d64  H683 128 x 64                            test_forward_backward
  BWD_SPLIT dv48 by workgroup count                 split_grid_d40  B5 H205 60 x 64 d40                      test_forward_backward
  causal (the CLIP shape)                           causal  B2 H2 77 x 77 (80) d64                           test_forward_backward, test_d_ready
  sdlt_attn_splitsum_batch                          every cross case in one launch, acc0 on two, strided    test_deferred_splitsum
  zero_D (forward clears D)                         self32_ks2 (kernel epilogue), ks2_d40 (memset)           test_forward_zeroes_d
Refused, and so not here: accumulate_dq / accumulate_dk off the cross routes (tests/test_attn_route_cpu.py pins the error).  Not reachable by a shape:
dp 128 (no model has such heads; attn_dp maps d 104 .. 128 there - dp160 and dp96 run the same templates), BWD_CROSS_ROLES<96> (never planned), ks 4
(SDLT_ATTN32_KS_* only: the fallback child runs this file under it).  Out of scope: near-ties and random logits (test_attention_fwd_bwd), the paired
launches, the DAAM side output.  To add a shape: add a case to attn_exact_ref.CASES (the CPU file then checks its operands and its route).
"""
import ctypes
import functools
import os

import pytest
import torch

from tests import attn_exact_ref as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SENT = -24576.0            # exact in bf16; no result of these operands comes near it
NAMES = [c["name"] for c in R.CASES]
SWITCHED = sorted(k for k in os.environ if k.startswith(("SDLT_ATTN", "SDLT_XATTN")))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


# ------------------------------------------------------------------------------------------------ frames
def _view(bufs, name, tensor):
    buf, r0, c0, rows, cols = R.frames(name)[1][tensor]
    b = bufs[buf]
    return b[0, c0:c0 + cols] if tensor in ("L", "D") else b[r0:r0 + rows, c0:c0 + cols]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The input buffers of a case on the device (NaN around the operands, bait in their pad rows), built once and never written."""
    c, op = R.BY_NAME[name], R.operands(name)
    spec, _ = R.frames(name)
    host = {b: torch.full((rows, width), NAN, dtype=dt) for b, (rows, width, dt) in spec.items() if b.startswith("in_")}
    for nm in ("Q", "K", "V", "dO"):
        _view(host, name, nm).copy_(op[nm])
    bufs = {b: t.cuda() for b, t in host.items()}
    for b in bufs.values():
        assert b.data_ptr() % 256 == 0
    return bufs


@functools.lru_cache(maxsize=None)
def _want(name, what, dtype, plus=None):
    """The reference in the output's format, on the device: computed once, never written.  plus: the previous contents an accumulating launch adds to."""
    acc = R.reference(name)[what]
    if plus:
        acc = acc + R.operands(name)[plus].to(F64)
    return R.rounded(acc, dtype).cuda()


@functools.lru_cache(maxsize=None)
def _rows(name, Np, N):
    return R.row_mask(R.BY_NAME[name], Np, N).cuda()


def _outputs(name):
    """Fresh output buffers: the sentinel everywhere, NaN in the views."""
    spec, t = R.frames(name)
    bufs = {b: torch.full((rows, width), SENT, dtype=dt, device="cuda") for b, (rows, width, dt) in spec.items() if b.startswith("out_")}
    for nm, (buf, *_rest) in t.items():
        if buf in bufs:
            _view(bufs, name, nm).fill_(NAN)
    return bufs


def _frames_intact(name, bufs, what):
    """Everything outside the output views still holds the sentinel."""
    _, t = R.frames(name)
    for b, buf in bufs.items():
        keep = torch.ones_like(buf, dtype=torch.bool)
        for nm, (bb, r0, c0, rows, cols) in t.items():
            if bb == b:
                keep[r0:r0 + rows, c0:c0 + cols] = False
        assert bool((buf[keep] == SENT).all()), f"{what}: wrote outside the views of {b}"


def _same(got, want, what, c, Np, rows=None):
    """torch.equal, or: how many elements differ, the first one decoded to (batch, row, head, column), and the rows affected.  rows: the row mask compared."""
    if rows is not None:
        assert bool(got.isfinite().all()), f"{what}: a pad row is not finite"
        got, want = got * rows, want * rows
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    r0, c0 = idx[0].tolist()
    where = sorted(set((idx[:, 0] % Np).tolist()))
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at (batch {r0 // Np}, row {r0 % Np}, head {c0 // c['d']}, column {c0 % c['d']}): "
                         f"got {float(got[r0, c0])}, want {float(want[r0, c0])}; rows {where[:12]}{'...' if len(where) > 12 else ''} of {Np}")


# ------------------------------------------------------------------------------------------------ launches
def _launch(ops, name, views, backward, **flags):
    """Build the block (R.fill_block: the fields ops.attn_fwd / ops.attn_bwd set), ask the planner about this very block, launch it.  Returns the route."""
    c = R.BY_NAME[name]
    for nm, v in views.items():
        assert v.stride(-1) == 1 and (v.dim() == 1 or v.stride(0) == R.address(name, nm)[1]), nm
    p = R.fill_block(ops._lib.AttnParams(), name, lambda nm: views[nm].data_ptr(), backward, **flags)
    code = ops._lib.load().sdlt_attn_route(ctypes.byref(p), int(backward))
    assert code >= 0, ops._lib.load().sdlt_last_error()
    got = ops._lib.attn_route_decode(code)
    if not SWITCHED:
        want = dict(c["bwd"] if backward else c["fwd"])
        if flags.get("d_ready"):
            want["prep"] = False
        if flags.get("defer_splitsum"):
            want["splitsum"] = False
        assert got == want, f"{name}: the planner sends this block to {got}, the case is meant for {want}"
    ops._issue("attn_bwd" if backward else "attn_fwd", p)
    return got


def _views(name, ins, outs):
    _, t = R.frames(name)
    return {nm: _view(outs if t[nm][0].startswith("out_") else ins, name, nm) for nm in t}


@functools.lru_cache(maxsize=None)
def _forward(ops, name):
    """The forward of a case, checked; returns (input buffers with O_in filled in: the exact O with bait in the pad rows, L on the device).  Run once per case."""
    c = R.BY_NAME[name]
    ins, outs = _inputs(name), _outputs(name)
    v = _views(name, ins, outs)
    _launch(ops, name, v, False)
    q_rows = _rows(name, c["Nqp"], c["Nq"])
    _same(v["O"], _want(name, "O", BF), f"{name} O", c, c["Nqp"], q_rows)      # pad rows of O: finite, unspecified
    L_ref = R.reference(name)["L"].cuda()
    err = (v["L"].double() - L_ref).abs()
    assert bool((err <= R.l_bound(L_ref)).all()), f"{name} L: off by {float(err.max())} (allowed {float(R.l_bound(L_ref).min())}) at {int(err.argmax())}"
    assert bool(v["D"].isnan().all()), "a forward without D wrote it"
    _frames_intact(name, outs, f"{name} forward")
    o_in = torch.where(q_rows, v["O"], torch.full_like(v["O"], R.O_PAD))
    v["O_in"].copy_(o_in)
    return ins, v["L"].clone()


def _backward(ops, name, *, start=None, **flags):
    """One backward launch into fresh frames; returns (views, buffers, route).  start: dict of previous contents (accumulating launches)."""
    ins, L = _forward(ops, name)
    outs = _outputs(name)
    v = _views(name, ins, outs)
    v["L"].copy_(L)
    for nm, t in (start or {}).items():
        v[nm].copy_(t)
    if flags.get("d_ready"):
        v["D"].copy_(R.reference(name)["D"].to(F32))
    route = _launch(ops, name, v, True, **flags)
    return v, outs, route


def _check_backward(name, v, outs, route, what, *, dq_plus=None, dk_plus=None, deferred=False):
    c = R.BY_NAME[name]
    Nqp, Nkp = c["Nqp"], c["Nkp"]
    _same(v["dQ"], _want(name, "dQ", BF, dq_plus), f"{what} dQ", c, Nqp, _rows(name, Nqp, c["Nq"]))      # pad rows of dQ: finite, unspecified
    if not deferred:
        _same(v["dK"], _want(name, "dK", BF, dk_plus), f"{what} dK", c, Nkp)                             # pad rows: zeros (or what they held)
        _same(v["dV"], _want(name, "dV", BF), f"{what} dV", c, Nkp)
    else:
        assert bool(v["dK"].isnan().all() & v["dV"].isnan().all()), f"{what}: a deferred slab sum wrote dK / dV"
    D_ref = R.reference(name)["D"].to(F32).cuda()
    assert torch.equal(v["D"], D_ref) or route["route"] in ("BWD_CROSS", "BWD_CROSS_ROLES"), f"{what}: D"      # (the single-pass kernels keep D in LDS)
    if c["qsplit"] > 1:
        # the slabs themselves: their sum over the splits is the exact fp32 dK / dV; pad-key rows are zeros (BWD_SPLIT) or untouched (cross routes)
        rows = c["B"] * Nkp
        live = _rows(name, Nkp, c["Nk"])
        for nm in ("dK32", "dV32"):
            slab = v[nm].reshape(c["qsplit"], rows, -1)
            pad = slab[:, ~live[:, 0]]
            assert bool(pad.isnan().all() if route["route"] != "BWD_SPLIT" else (pad == 0).all()), f"{what} {nm}: pad rows"
            total = torch.where(live, slab, torch.zeros_like(slab)).sum(0)
            _same(total, _want(name, nm[:2], F32), f"{what} {nm} summed", c, Nkp)
    _frames_intact(name, outs, what)


# ------------------------------------------------------------------------------------------------ 1. every route: forward + backward
@pytest.mark.parametrize("name", NAMES)
def test_forward_backward(ops, name):
    v, outs, route = _backward(ops, name)
    _check_backward(name, v, outs, route, f"{name} {route['route']}")


# ------------------------------------------------------------------------------------------------ 2. d_ready, zero_D
@pytest.mark.parametrize("name", R.SELF)
def test_d_ready(ops, name):
    """D supplied from the reference, no pre-pass launch: the same bits; and the pre-pass run's D is that D."""
    v0, _, _ = _backward(ops, name)
    v, outs, route = _backward(ops, name, d_ready=True)
    assert not route["prep"]
    _check_backward(name, v, outs, route, f"{name} d_ready")
    for nm in ("dQ", "dK", "dV"):
        assert torch.equal(v[nm].nan_to_num(7.0), v0[nm].nan_to_num(7.0)), nm
    assert torch.equal(v0["D"], v["D"])


@pytest.mark.parametrize("name", ["self32_ks2", "ks2_d40"])
def test_forward_zeroes_d(ops, name):
    c = R.BY_NAME[name]
    ins, outs = _inputs(name), _outputs(name)
    v = _views(name, ins, outs)
    _launch(ops, name, v, False, zero_D=True)
    assert float(v["D"].abs().max()) == 0.0
    _same(v["O"], _want(name, "O", BF), f"{name} O with zero_D", c, c["Nqp"], _rows(name, c["Nqp"], c["Nq"]))
    _frames_intact(name, outs, f"{name} forward with zero_D")


# ------------------------------------------------------------------------------------------------ 3. cross routes: accumulate, deferred slab sum
@pytest.mark.parametrize("name", R.CROSS)
def test_cross_accumulate(ops, name):
    """dQ and dK already hold small integers: bf16(previous + exact), one rounding; dV is overwritten; pad rows of dK keep what they held."""
    op = R.operands(name)
    v, outs, route = _backward(ops, name, start=dict(dQ=op["dQ0"].cuda(), dK=op["dK0"].cuda()), accumulate=True)
    _check_backward(name, v, outs, route, f"{name} accumulate", dq_plus="dQ0", dk_plus="dK0")


def test_deferred_splitsum(ops):
    """defer_splitsum leaves the slabs; one SplitsumPlan launch then sums the slabs of all cross cases, dK / dV strided views, every other item with acc0."""
    runs = []
    for i, name in enumerate(R.CROSS):
        op = R.operands(name)
        v, outs, route = _backward(ops, name, defer_splitsum=True)
        _check_backward(name, v, outs, route, f"{name} deferred", deferred=True)
        if i % 2:
            v["dK"].copy_(op["dK0"].cuda())
        runs.append((name, v, outs, bool(i % 2)))
    c = R.BY_NAME
    items = [dict(dK32=v["dK32"], dV32=v["dV32"], dK=v["dK"], dV=v["dV"], nsplit=c[n]["qsplit"], B=c[n]["B"], Nk=c[n]["Nk"], Nkp=c[n]["Nkp"], acc0=acc)
             for n, v, _, acc in runs]
    ops.SplitsumPlan(items, torch.device("cuda")).run()
    for name, v, outs, acc in runs:
        _same(v["dK"], _want(name, "dK", BF, "dK0" if acc else None), f"{name} slab sum dK (acc0 {acc})", c[name], c[name]["Nkp"])
        _same(v["dV"], _want(name, "dV", BF), f"{name} slab sum dV", c[name], c[name]["Nkp"])
        _frames_intact(name, outs, f"{name} slab sum")


# ------------------------------------------------------------------------------------------------ 4. the block is the one the public entries build
def test_block_is_the_one_of_the_public_entries(ops, monkeypatch):
    """ops.attn_fwd / ops.attn_bwd on the same views leave the same parameter block as R.fill_block (compared byte for byte, nothing launched)."""
    name = "cross_five_128"
    c = R.BY_NAME[name]
    v = _views(name, _inputs(name), _outputs(name))
    seen = []
    monkeypatch.setattr(ops, "_issue", lambda kind, p, keep=None: seen.append(bytes(p)))
    kw = dict(B=c["B"], H=c["H"], Nq=c["Nq"], Nk=c["Nk"], Nqp=c["Nqp"], Nkp=c["Nkp"], d=c["d"], scale=R.SCALE, causal=c["causal"])
    ops.attn_fwd(v["Q"], v["K"], v["V"], None, v["O"], v["L"], **kw)
    ops.attn_bwd(v["Q"], v["K"], v["V"], None, None, v["O_in"], v["L"], v["dO"], None, v["D"], v["dQ"], v["dK"], v["dV"], **kw, qsplit=c["qsplit"],
                 dK32=v["dK32"], dV32=v["dV32"], accumulate_dq=True, accumulate_dk=True)
    ptr = lambda nm: v[nm].data_ptr()      # noqa: E731
    assert seen[0] == bytes(R.fill_block(ops._lib.AttnParams(), name, ptr, False))
    assert seen[1] == bytes(R.fill_block(ops._lib.AttnParams(), name, ptr, True, accumulate=True))
