"""The exact-arithmetic reference of the wave-split-K and row-strip products (tests/wsk_exact_ref.py) checked without a GPU, on every case the GPU
file (tests/test_wsk_exact_gpu.py) uses: (a) every operand is a bf16 value, (b) the grid that makes torch.equal legitimate - every fp64 partial sum
(a wave's quarter of K, a K group, a strip split, a head's and a tile's row sum of the rounded output) is a multiple of 0.25 below 2^24, and so is the
sum of the terms' magnitudes, which covers every other order -, (c) the output rounding is idempotent, (d) equality with a second formulation written
with einsum and plain loops on the smallest case of every form, (e) every case the GPU file runs is in the reference's lists, (f) the GPU file's
table names every launch_wsk<...> / launch_strip<...> instantiation of the two dispatch ladders (csrc/wsk.hip, csrc/strip.hip), read as text."""
import os
import re

import pytest
import torch

from tests import test_wsk_exact_gpu as G
from tests import wsk_exact_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sd-lora-trainer_amd", "csrc")
LIMIT = float(2 ** 24)


def on_grid(t, what, step=0.25):
    t = t.to(F64)
    assert torch.equal(t / step, torch.round(t / step)), f"{what}: not a multiple of {step}"
    assert float(t.abs().max()) < LIMIT, f"{what}: {float(t.abs().max())} >= 2^24"


def is_bf16(t, what):
    assert t.dtype in (BF, F32) and torch.equal(t.to(BF).to(F64), t.to(F64)), f"{what}: not exactly representable in bf16"


def idempotent(acc, dtype, what):
    once = R.rounded(acc, dtype)
    assert torch.equal(R.rounded(once.to(F64), dtype), once), f"{what}: rounding twice differs from rounding once"
    return once


# ================================================================================================================ wave-split-K
def test_wsk_operand_ranges():
    for (M, N, K, gk) in [(448, 640, 2304, 0), (192, 1280, 768, 256), (64, 640, 256, 128)]:
        d = R.wsk_operands(M, N, K, gk)
        for k in ("X", "O"):
            assert set(d[k].float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        for k in ("W", "Bup"):
            assert set(d[k].float().unique().tolist()) <= {-1.0, 0.0, 1.0}
        per_group = (d["Adown"] != 0).reshape(32, -1, gk or K).sum(2)
        assert int(per_group.max()) <= 3 and int(per_group.min()) >= 1 and set(d["Adown"].float().unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set(d["col_scale"].unique().tolist()) <= {0.5, 1.0, 2.0} and R.LORA_SCALE == 0.5
        for k in ("bias", "residual"):
            assert torch.equal(d[k].float(), torch.round(d[k].float()))


@pytest.mark.parametrize("case", R.ALL_WSK_CASES, ids=str)
def test_wsk_cases_exact(case):
    M, N, K, form, gk = case
    assert M % 64 == 0 and N % 640 == 0 and K % 256 == 0 and (not gk or (K % gk == 0 and gk % 64 == 0 and K // gk in (2, 3)))
    d, v, ref = R.wsk_operands(M, N, K, gk), R.WSK_FORMS[form], R.wsk_reference(*case)
    for k in ("X", "W", "O", "residual", "Adown", "Bup", "bias", "col_scale"):
        is_bf16(d[k], k)                                                                              # (a)
    x, w = d["X"].to(F64), d["W"].to(F64)
    on_grid(x.abs() @ w.abs().t(), "sum of |x w|", 1.0)                                               # (b) any order of the K sum
    total = torch.zeros(M, N, dtype=F64)
    for wv in range(R.NW):                                                                            # the four waves' partial tiles, added in wave order
        cols = R.wave_columns(K, wv)
        part = x[:, cols] @ w[:, cols].t()
        on_grid(part, f"wave {wv}'s quarter of K", 1.0)
        total = total + part
        on_grid(total, f"partial tiles of waves 0..{wv}", 1.0)
    assert torch.equal(total, x @ w.t())
    ad = R.wsk_adapter(d, v, gk)
    if ad:
        a, bu = ad[0].to(F64), ad[1].to(F64)
        pad, C = v["pad"], gk or K
        for g in range(K // C):
            for wv in range(R.NW):
                cols = R.wave_columns(K, wv)
                cols = cols[(cols >= g * C) & (cols < (g + 1) * C)]
                on_grid(x[:, cols] @ a[:, cols].t(), f"wave {wv}'s share of K group {g} of T", 1.0)
            Tg = x[:, g * C:(g + 1) * C] @ a[:, g * C:(g + 1) * C].t()
            assert float(Tg.abs().max()) <= 6.0                                                      # three +-1 against |x| <= 2: s T is a multiple of 0.5, |s T| <= 3
            on_grid((R.LORA_SCALE * Tg) @ bu[:, g * pad:(g + 1) * pad].t(), f"up-projection of K group {g}", 0.5)
        on_grid((R.LORA_SCALE * 6.0) * bu.abs().sum(1), "sum of |Tb bup|", 0.5)
    if ref["T"] is not None:
        assert tuple(ref["T"].shape) == (M, R.wsk_t_width(K, v, gk)) and ref["T"].dtype == BF
        on_grid(ref["T"], "T_out", 0.5)
        assert float(ref["T"].to(F64).abs().max()) <= 3.0
    assert (ref["T"] is not None) == bool(v.get("T")) and (ref["Y0"] is not None) == bool(v.get("y0"))
    assert (ref["D"] is not None) == bool(v.get("dot")) and (ref["parts"] is not None) == bool(v.get("parts"))
    on_grid(ref["Y"], "Y before rounding")
    Yb = idempotent(ref["Y"], BF, "Y").to(F64)                                                        # (c)
    if ref["Y0"] is not None:
        on_grid(ref["Y0"], "Y0 before rounding")
        idempotent(ref["Y0"], BF, "Y0")
        assert torch.equal(ref["Y"], ref["Y0"] + (d["residual"].to(F64) if v.get("R") else 0.0))
    if ref["D"] is not None:
        Nq, H = R.wsk_nq(M, v), N // R.HEAD
        assert M % Nq == 0 and tuple(ref["D"].shape) == (M * H,)
        on_grid(ref["D"], "D")
        prod = Yb * d["O"].to(F64)
        on_grid(prod.abs().reshape(M, H, R.HEAD).sum(-1), "sum of |y o| over a head")                  # any order, either tile's contribution
        blocks = prod.reshape(M, N // 16, 16).sum(-1)                                                   # a head's share of a tile is whole 16-column units
        on_grid(blocks, "16-column unit of y o")
        assert any((h * 64) // 80 != (h * 64 + 63) // 80 for h in range(H)), "no head straddles two tiles"
        idempotent(ref["D"], F32, "D")
    if ref["parts"] is not None:
        assert tuple(ref["parts"].shape) == (M, N // R.TILE_N)
        on_grid(ref["parts"], "row sum over an 80-column tile")
        on_grid(Yb.abs().reshape(M, N // R.TILE_N, R.TILE_N).sum(-1), "sum of |y| over an 80-column tile")
        idempotent(ref["parts"], F32, "ln_parts[..., 0]")


def _wsk_naive(case):
    """The same contract with einsum and plain loops over K groups, heads and tiles."""
    M, N, K, form, gk = case
    d, v = R.wsk_operands(M, N, K, gk), R.WSK_FORMS[form]
    x = d["X"].to(F64)
    acc = torch.einsum("mk,nk->mn", x, d["W"].to(F64))
    T = None
    pad = v.get("pad", 0)
    if pad:
        C = gk or K
        G = K // C
        T = torch.empty(M, pad * G, dtype=BF)
        for g in range(G):
            t = torch.einsum("mk,rk->mr", x[:, g * C:(g + 1) * C], d["Adown"][:pad, g * C:(g + 1) * C].to(F64))
            T[:, g * pad:(g + 1) * pad] = (0.5 * t).to(F32).to(BF)
            acc += torch.einsum("mr,nr->mn", T[:, g * pad:(g + 1) * pad].to(F64), d["Bup"][:, g * pad:(g + 1) * pad].to(F64))
    if v.get("cs"):
        acc = torch.einsum("mn,n->mn", acc, d["col_scale"].to(F64))
    if v.get("bias"):
        acc = acc + d["bias"].to(F64)[None, :]
    Y0 = acc.clone()
    if v.get("R"):
        acc = acc + d["residual"].to(F64)
    Yb = acc.to(F32).to(BF).to(F64)
    D = parts = None
    Nq = R.wsk_nq(M, v)
    if Nq:
        H, o = N // 64, d["O"].to(F64)
        D = torch.zeros(M * H, dtype=F64)
        for b in range(M // Nq):
            for h in range(H):
                for q in range(Nq):
                    m = b * Nq + q
                    D[(b * H + h) * Nq + q] = float((Yb[m, 64 * h:64 * h + 64] * o[m, 64 * h:64 * h + 64]).sum())
    if v.get("parts"):
        parts = torch.stack([Yb[:, 80 * t:80 * t + 80].sum(1) for t in range(N // 80)], 1)
    return dict(Y=acc, T=T if v.get("T") else None, Y0=Y0 if v.get("y0") else None, D=D, parts=parts)


SMALLEST_WSK = [c for c in R.ALL_WSK_CASES if c[:3] == (64, 640, 256)] + [(192, 1280, 768, "gk", 256), (128, 640, 1024, "dotM", 0), (128, 640, 1024, "loradotM", 0)]
# (every form; G = 2 and G = 3; Nq = M differs from Nq = 64 from M = 128 on)


@pytest.mark.parametrize("case", SMALLEST_WSK, ids=str)
def test_wsk_reference_against_naive(case):
    ref, naive = R.wsk_reference(*case), _wsk_naive(case)
    for k in ("Y", "T", "Y0", "D", "parts"):
        assert (ref[k] is None) == (naive[k] is None), k
        if ref[k] is not None:
            assert torch.equal(ref[k], naive[k]), f"{case}: {k} differs between gemm_ref and the naive formulation"


def test_wsk_every_form_has_a_smallest_case():
    forms = {c[3] for c in SMALLEST_WSK}
    assert forms == set(R.WSK_FORMS), set(R.WSK_FORMS) - forms
    assert {c[3] for c in R.ALL_WSK_CASES} == set(R.WSK_FORMS)


def test_wsk_case_lists_cover_the_mechanisms():
    assert len(R.WSK_PLAIN_CASES) == len(R.WSK_MS) * len(R.WSK_NS) * len(R.WSK_KS) == 32
    assert {(M // 64) % 2 for M in R.WSK_MS} == {0, 1} and 64 in R.WSK_MS                      # one row tile, even and odd row-tile counts
    assert {K // 256 for K in R.WSK_KS} == {1, 3, 4, 9}                                          # steps per wave: 1, the packed ring's 3, 4 > both rings, 9
    assert set(R.WSK_REDUCED) <= {c[:3] for c in R.WSK_PLAIN_CASES}
    assert {(K // gk, gk) for (_, _, K, gk) in R.WSK_GROUPED} == {(2, 128), (2, 384), (3, 256), (2, 512)}
    assert {R.wsk_nq(c[0], R.WSK_FORMS[c[3]]) == c[0] for c in R.WSK_ROWDOT_CASES} == {True, False}


# ================================================================================================================ row strip
STRIP_PRODUCTS = tuple(dict.fromkeys((B, N, K, f) for (B, T, Tp, N, K, f) in R.ALL_STRIP_CASES))


@pytest.mark.parametrize("B,N,K,form", STRIP_PRODUCTS)
def test_strip_products_exact(B, N, K, form):
    assert K % 256 == 0 and N % 16 == 0
    v = R.STRIP_FORMS[form]
    X, W = R.strip_X(B, K), R.strip_W(N, K)
    is_bf16(X, "X"), is_bf16(W, "W"), is_bf16(R.strip_bias(N), "bias"), is_bf16(R.strip_R(B, N), "R")
    assert set(X.float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(W.float().unique().tolist()) <= {-1.0, 0.0, 1.0}
    x, w = X.to(F64), W.to(F64)
    on_grid(x.abs() @ w.abs().t(), "sum of |x w|", 1.0)
    S = v.get("split", 0) or v.get("slabs", 0) or 1
    assert S <= K // 256
    total = torch.zeros(B, R.STRIP_ROWS, N, dtype=F64)
    for s, (lo, hi) in enumerate(R.split_ranges(K, S)):
        split = torch.zeros_like(total)
        for wv in range(R.NW):
            cols = R.wave_columns(hi - lo, wv, lo)
            part = x[..., cols] @ w[:, cols].t()
            on_grid(part, f"split {s}, wave {wv}", 1.0)
            split = split + part
        on_grid(split, f"split {s}", 1.0)
        total = total + split
        on_grid(total, f"splits 0..{s}", 1.0)
    assert torch.equal(total, x @ w.t())
    acc, slabs = R.strip_full(B, N, K, form)
    if slabs is not None:
        assert acc is None and tuple(slabs.shape) == (S, B, R.STRIP_ROWS, N) and torch.equal(slabs.sum(0), total)
        on_grid(slabs, "slabs", 1.0)
        idempotent(slabs, F32, "P")
    else:
        on_grid(acc, "Y before rounding", 1.0)
        idempotent(acc, BF, "Y")


@pytest.mark.parametrize("case", [c for c in R.ALL_STRIP_CASES if c[3] == 16 and c[:3] in ((1, 17, 80), (3, 1, 80), (1, 1, 80))], ids=str)
def test_strip_reference_against_naive(case):
    B, T, Tp, N, K, form = case
    v = R.STRIP_FORMS[form]
    x, w = R.strip_X(B, K)[:, :T].to(F64), R.strip_W(N, K).to(F64)
    acc, slabs = R.strip_reference(*case)
    if v.get("slabs"):
        S = v["slabs"]
        for s in range(S):
            ks = slice(s * K // S, (s + 1) * K // S)
            assert torch.equal(slabs[s], torch.einsum("btk,nk->btn", x[..., ks], w[:, ks])), f"{case}: slab {s}"
        assert tuple(slabs.shape) == (S, B, T, N)
        return
    naive = torch.einsum("btk,nk->btn", x, w)
    if v.get("bias"):
        naive = naive + R.strip_bias(N).to(F64)[None, None, :]
    if v.get("R"):
        naive = naive + R.strip_R(B, N)[:, :T].to(F64)
    assert torch.equal(acc, naive)
    laid = R.strip_layout(acc, Tp, 5.0).reshape(B, Tp, N)
    assert torch.equal(laid[:, :T], acc) and bool((laid[:, T:] == 5.0).all())


def test_strip_every_form_has_a_smallest_case():
    small = {c[5] for c in R.ALL_STRIP_CASES if c[3] == 16 and c[:3] in ((1, 17, 80), (3, 1, 80), (1, 1, 80))}
    assert small >= {"plain", "bias", "biasR", "split2", "split3", "slab1", "slab3"} and {c[5] for c in R.ALL_STRIP_CASES} == set(R.STRIP_FORMS)


def test_strip_case_lists_cover_the_mechanisms():
    assert len(R.STRIP_PLAIN_CASES) == 5 * 2 * 2 * 3 * 4
    for (B, T, Tp, N, K, f) in R.ALL_STRIP_CASES:
        assert 1 <= T <= 80 <= Tp and K % 256 == 0 and N % 16 == 0
        S = R.STRIP_FORMS[f].get("slabs", 0)
        assert not S or K % (256 * S) == 0
    assert {c[5] for c in R.STRIP_SPLIT_CASES} == {"split2", "split3", "split9"} and {c[4] for c in R.STRIP_SPLIT_CASES if c[5] == "split9"} == {2304}
    for a, b in R.STRIP_PAIRS:                                   # a pair's problems differ in N, K, B and T
        assert all(a[i] != b[i] for i in (0, 1, 3, 4))
    widths = [{N >= 2304 and N % 32 == 0 for N in (a[3], b[3])} for a, b in R.STRIP_PAIRS]
    assert {True} in widths and {False} in widths and all(len(s) == 1 for s in widths)


# ================================================================================================================ the GPU file
def test_gpu_file_runs_listed_cases_only():
    wsk, strip = set(R.ALL_WSK_CASES), set(R.ALL_STRIP_CASES)
    assert {(M, N, K, "plain", 0) for (M, N, K) in G.PLAIN_SHAPES} <= wsk
    for name in ("EPILOGUE_CASES", "ADAPTER_CASES", "ROWDOT_CASES", "RP32_CASES", "GROUP_K_CASES", "PREFETCH_CASES"):
        assert getattr(G, name) and set(getattr(G, name)) <= wsk, name
    assert {(B, T, Tp, N, K, "plain") for (N, K) in G.STRIP_NK for B in R.STRIP_BS for T in R.STRIP_TS for Tp in R.STRIP_TPS} <= strip
    for name in ("STRIP_EPILOGUE_CASES", "STRIP_SPLIT_CASES", "STRIP_SLAB_CASES"):
        assert getattr(G, name) and set(getattr(G, name)) <= strip, name
    assert {c for pair in G.STRIP_PAIRS for c in pair} <= strip
    names = {n for n in dir(G) if n.endswith(("_CASES", "_SHAPES", "_PAIRS", "_NK"))}
    assert names == {"PLAIN_SHAPES", "EPILOGUE_CASES", "ADAPTER_CASES", "ROWDOT_CASES", "RP32_CASES", "GROUP_K_CASES", "PREFETCH_CASES", "STRIP_NK",
                     "STRIP_EPILOGUE_CASES", "STRIP_SPLIT_CASES", "STRIP_SLAB_CASES", "STRIP_PAIRS"}, "a new case list of the GPU file: check it here"


def instantiations(csrc):
    """The launch_wsk<...> / launch_strip<...> / launch_strip_pair<...> instantiations the dispatch code of csrc/wsk.hip and csrc/strip.hip names, as text."""
    norm = lambda s: re.sub(r"\s*,\s*", ", ", s.strip())      # noqa: E731
    wsk = open(os.path.join(csrc, "wsk.hip")).read()
    ladder = wsk[wsk.index("static int wsk_dispatch("):]
    ladder = ladder[:ladder.index("\n}\n")]
    found = [f"launch_wsk<{norm(a)}>" for a in re.findall(r"launch_wsk<([^<>]*)>\s*\(", ladder)]
    assert len(found) == len(re.findall(r"launch_wsk<[^<>]*>\s*\(", wsk)), "a launch_wsk<...> call outside wsk_dispatch"
    strip = open(os.path.join(csrc, "strip.hip")).read()
    found += [f"{name}<{norm(a)}>" for name, a in re.findall(r"(launch_strip(?:_pair)?)<([^<>]*)>\s*\(", strip)]
    return found


def test_route_table():
    found = instantiations(CSRC)
    assert len(found) == len(set(found)), found
    assert set(found) == set(G.ROUTES), f"not in ROUTES: {sorted(set(found) - set(G.ROUTES))}; no longer in the dispatch code: {sorted(set(G.ROUTES) - set(found))}"
    for inst, tests in G.ROUTES.items():
        assert inst in G.__doc__ or inst.split("<")[0] in G.__doc__
        if tests[0] is None:                                    # out of scope here: the test that keeps it must exist
            path, name = tests[1].split("::")
            assert re.search(rf"^def {name}\(", open(os.path.join(ROOT, path)).read(), re.M), tests[1]
        else:
            for name in tests:
                assert callable(getattr(G, name, None)) and name.startswith("test_"), f"{inst}: {name} is not a test of tests/test_wsk_exact_gpu.py"
                assert name in G.__doc__, f"{name} is missing from the docstring's table"
