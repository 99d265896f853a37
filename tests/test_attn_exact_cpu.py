"""What makes tests/test_attn_exact_gpu.py exact, proved without a GPU for every case of tests/attn_exact_ref.py: the winners of every softmax row tie,
the losers underflow, every rounding a kernel performs (P and dS to bf16, the fp32 sums) lands on the exact value, the results are not trivially zero,
the project's own emulator (the oracle of test_attention_fwd_bwd) gives the same bits, and the planner sends every case to the route its name says."""
import ctypes
import os

import pytest
import torch

from sd_lora_trainer_amd import _lib
from tests import attn_exact_ref as R
from tests import emu_ops as E

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAMES = [c["name"] for c in R.CASES]
SWITCHED = sorted(k for k in os.environ if k.startswith(("SDLT_ATTN", "SDLT_XATTN")))


def _bf16_heals(x):
    """x is a bf16 number, and stays the nearest one after a relative error of 2^-12 in either direction (the kernels' exp2 / L are that good and better)."""
    ok = torch.equal(x.to(F32).to(BF).to(F64), x)
    for s in (1 + 2.0 ** -12, 1 - 2.0 ** -12):
        ok = ok and torch.equal((x * s).to(F32).to(BF).to(F64), x)
    return ok


def _parts(name):
    c, op, ref = R.BY_NAME[name], R.operands(name), R.reference(name)
    B, H, Nq, Nk, d = c["B"], c["H"], c["Nq"], c["Nk"], c["d"]
    h = lambda t, Np, N: R._heads(t, B, Np, H, d)[:, :, :N]      # noqa: E731
    return c, op, ref, h(op["Q"], c["Nqp"], Nq), h(op["K"], c["Nkp"], Nk), h(op["V"], c["Nkp"], Nk), h(op["dO"], c["Nqp"], Nq)


@pytest.mark.parametrize("name", NAMES)
def test_ties_gap_and_p(name):
    c, op, ref, q, k, v, do = _parts(name)
    S, P = ref["S"], ref["P"]
    top = S.max(-1, keepdim=True).values
    win = S == top
    t = win.sum(-1)
    assert set(t.flatten().tolist()) == {1, 2, 4, 8}, "every tie count in every case, and no other"
    best_loser = S.masked_fill(win, float("-inf")).max(-1).values
    assert float(((top.squeeze(-1) - best_loser) * R.LOG2E).min()) >= 150, "a loser closer than 150 octaves"
    assert float((top * R.LOG2E).abs().max()) < 256
    assert len(set(S[S > float("-inf")].flatten().tolist())) >= 4, "winners and at least three loser levels"
    assert torch.equal(P[win], (1.0 / t.to(F64))[..., None].expand_as(P)[win]), "fp64 softmax is not exactly 1 / t on the winners"
    assert float(P[~win].max()) < 2.0 ** -150, "a loser that does not underflow in fp32"
    if c["causal"]:
        assert bool((P.triu(1) == 0).all())
    # placement: some row finds its winners only in the last 64-key tile, some only in the first, some in even and odd tiles at once
    if c["Nk"] > 64:
        tile = torch.arange(c["Nk"]) // 64
        last, first = int(tile.max()), 0
        in_tile = torch.stack([(win & (tile == i)).any(-1) for i in range(last + 1)], -1)      # [B, H, Nq, tiles]
        only = lambda i: bool((in_tile[..., i] & (in_tile.sum(-1) == 1)).any())      # noqa: E731
        assert only(last) and only(first)
        if not c["causal"] and last >= 1:
            assert bool((in_tile[..., 0::2].any(-1) & in_tile[..., 1::2].any(-1)).any())


@pytest.mark.parametrize("name", NAMES)
def test_every_rounding_heals_and_every_sum_is_exact(name):
    c, op, ref, q, k, v, do = _parts(name)
    P = ref["P"].to(F32).to(F64)                     # the losers' 2^-178 gone: what a kernel holds
    B, H, Nq, d = c["B"], c["H"], c["Nq"], c["d"]
    O = R._heads(R.rounded(ref["O"], F32), B, c["Nqp"], H, d)[:, :, :Nq]
    dS = ref["dS"].to(F32).to(F64)
    assert float((dS - ref["dS"]).abs().max()) < 2.0 ** -140
    for what, x in (("P", P), ("O", O), ("dS / scale", dS), ("dS", dS * R.SCALE)):
        assert _bf16_heals(x), f"{what} is not a bf16 number that survives a 2^-12 error"
    assert float(dS.abs().max()) <= 8
    # every term of every fp32 sum is a multiple of 2^-9, and the sum of the terms' magnitudes stays below 2^15: 24 bits hold any partial sum in any order
    unit = 2.0 ** -9
    for x in (P, O, dS * R.SCALE, q, k, v, do):
        assert torch.equal((x / unit).round() * unit, x)
    kt, a = k.abs().transpose(-1, -2), dS.abs()
    sums = dict(s=q.abs() @ kt, o=P @ v.abs(), dp=do.abs() @ v.abs().transpose(-1, -2), D=(do * O).abs().sum(-1), dq=a @ k.abs() + 3,
                dk=a.transpose(-1, -2) @ q.abs() + 3, dv=P.transpose(-1, -2) @ do.abs())
    for what, x in sums.items():
        assert float(x.max()) < 2.0 ** 15, what
    # the outputs themselves are fp32 numbers (R.rounded asserts it), also after the accumulating launches' addition
    for nm in ("O", "dQ", "dK", "dV"):
        R.rounded(ref[nm], F32)


@pytest.mark.parametrize("name", NAMES)
def test_results_are_not_trivial(name):
    c, op, ref, q, k, v, do = _parts(name)
    B, H, d = c["B"], c["H"], c["d"]
    live = {nm: R._heads(R.rounded(ref[nm], F32), B, Np, H, d)[:, :, :N] for nm, Np, N in
            (("O", c["Nqp"], c["Nq"]), ("dQ", c["Nqp"], c["Nq"]), ("dK", c["Nkp"], c["Nk"]), ("dV", c["Nkp"], c["Nk"]))}
    assert float((live["dQ"] != 0).double().mean()) >= 0.10
    assert float((live["dV"] != 0).double().mean()) >= 0.25
    for nm, x in live.items():
        assert bool((x != 0).any(2).all()), f"{nm}: a column of a head that is zero in every row"
    # every key of a class of two or more has a gradient; a key of no class has none
    for b in range(B):
        for h in range(H):
            members, _ = op["classes"][(b * H + h) % R.NPATTERN]
            in_class = sorted(j for m in members for j in m)
            for m in members:
                if len(m) >= 2:
                    assert bool((live["dK"][b, h, m] != 0).any(-1).all()), (b, h, m)
            rest = [j for j in range(c["Nk"]) if j not in in_class]
            assert rest and not bool(live["dK"][b, h, rest].any()) and not bool(live["dV"][b, h, rest].any())
    for nm, Np, N in (("dK", c["Nkp"], c["Nk"]), ("dV", c["Nkp"], c["Nk"])):
        assert not bool(ref[nm][~R.row_mask(c, Np, N).expand_as(ref[nm])].any())


@pytest.mark.parametrize("name", NAMES)
def test_emulator_gives_the_exact_result(name):
    c, op, ref = R.BY_NAME[name], R.operands(name), R.reference(name)
    kw = dict(B=c["B"], H=c["H"], Nq=c["Nq"], Nk=c["Nk"], Nqp=c["Nqp"], Nkp=c["Nkp"], d=c["d"], scale=R.SCALE, causal=c["causal"])
    O, L = torch.full_like(op["Q"], float("nan")), torch.zeros(c["B"] * c["H"] * c["Nq"])
    E.attn_fwd(op["Q"], op["K"], op["V"], None, O, L, **kw)
    rows = R.row_mask(c, c["Nqp"], c["Nq"])
    want_O = R.rounded(ref["O"], BF)
    assert torch.equal(O * rows, want_O * rows)
    assert bool(((L.double() - ref["L"]).abs() <= R.l_bound(ref["L"])).all())
    dQ, dK, dV = (torch.full_like(t, float("nan")) for t in (op["Q"], op["K"], op["V"]))
    E.attn_bwd(op["Q"], op["K"], op["V"], None, None, O, L, op["dO"], None, None, dQ, dK, dV, **kw)
    assert torch.equal(dQ * rows, R.rounded(ref["dQ"], BF) * rows)
    assert torch.equal(dK, R.rounded(ref["dK"], BF)) and torch.equal(dV, R.rounded(ref["dV"], BF)), "pad rows of dK / dV are zeros"
    if name in R.CROSS:
        dQ, dK = op["dQ0"].clone(), op["dK0"].clone()
        E.attn_bwd(op["Q"], op["K"], op["V"], None, None, O, L, op["dO"], None, None, dQ, dK, dV, **kw, accumulate_dq=True, accumulate_dk=True)
        assert torch.equal(dQ * rows, R.rounded(op["dQ0"].double() + ref["dQ"], BF) * rows)
        assert torch.equal(dK, R.rounded(op["dK0"].double() + ref["dK"], BF))


# ---------------------------------------------------------------------------------------------------------------- routes
def block(name, backward, **flags):
    """The parameter block the GPU file launches for a case (R.fill_block), on made-up buffers at 256-byte-aligned addresses: nothing dereferences them."""
    bufs, _ = R.frames(name)
    base = {b: 0x10000000 * (i + 1) for i, b in enumerate(sorted(bufs))}
    return R.fill_block(_lib.AttnParams(), name, lambda nm: R.address(name, nm, base[R.frames(name)[1][nm][0]])[0], backward, **flags)


def route(name, backward, **flags):
    code = _lib.load().sdlt_attn_route(ctypes.byref(block(name, backward, **flags)), backward)
    return code if code < 0 else _lib.attn_route_decode(code)


def test_every_case_takes_the_route_it_names():
    """(The table is the one of the default switches: SWITCHED names what the environment sets.)"""
    reached = set()
    for c in R.CASES:
        f, b = route(c["name"], 0), route(c["name"], 1)
        assert f == c["fwd"] and b == c["bwd"], (c["name"], f, b, SWITCHED)
        reached |= {f["route"], b["route"]}
    assert reached == set(_lib.ATTN_ROUTES), "a route no exact case reaches"


def test_variant_flags_keep_the_route():
    for name in R.SELF:
        assert route(name, 1, d_ready=True) == dict(R.BY_NAME[name]["bwd"], prep=False), name
    for name in R.CROSS:
        assert route(name, 1, accumulate=True) == R.BY_NAME[name]["bwd"], name
        assert route(name, 1, defer_splitsum=True) == dict(R.BY_NAME[name]["bwd"], splitsum=False), name
    assert route("self32_ks2", 0, zero_D=True) == R.BY_NAME["self32_ks2"]["fwd"]


def test_frames_keep_the_alignment_the_kernels_need():
    for c in R.CASES:
        for nm in R.frames(c["name"])[1]:
            off, ld = R.address(c["name"], nm)
            out16 = nm in ("O", "dQ", "dK", "dV")
            assert off % (8 if out16 and c["ocol"] == 4 else 16) == 0 and (off % 16 == 8) == (out16 and c["ocol"] == 4), (c["name"], nm)
            assert ld % 8 == 0 or nm in ("L", "D", "dK32", "dV32")
