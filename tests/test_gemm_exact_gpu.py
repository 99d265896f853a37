"""Bit-exact parity of the linear products and the adapter gradients (MI355X): sdlt_gemm_bf16 mode 0 on every tile id, rank pad, ring depth, K split,
adapter grouping, batched launch and second-segment form, sdlt_lora_grad_grouped / _wide on both kernel families, and the weight-gradient chain,
against the fp64 reference of tests/gemm_exact_ref.py on small-integer operands.  Every partial sum is a multiple of 0.25 far below 2^24
(tests/test_gemm_exact_cpu.py asserts it), so no result depends on summation order, tile, split or ring depth: every comparison here is torch.equal,
there is no tolerance.  Outputs are NaN-filled views of larger sentinel-filled buffers with room for a whole 256 x 256 tile beyond them (stray
writes); X, X2, P and Q are views of wider buffers whose other columns and rows hold NaN (stray reads).  Every product runs a forced tile - or has
an fp32 output, a second segment or adapter groups - so ops.gemm takes the tiled kernel, never the wave-split-K route.
The nonlinear epilogues of mode 0 (GEGLU forward / backward, activation side output / backward: EPI 1..4, and the folded LayerNorm: LN 1 / 2)
cannot be exact and are out of scope; tests/test_kernels_gpu.py keeps them under a tolerance.

Linear instantiations gemm_kernel<MI, NI, WN, MODE 0, R16, NS, KG, BT, WM> that gemm_plan reaches in mode 0 (csrc/gemm.hip, rows of GEMM_FAMILIES), R16 = rank pad / 16:
  plain family, requested ring depth 2 and 4, KG 0, BT 0
    R16 0:          tiles 1..8                      test_plain (both rings); second segment K2 / x2_group_n are runtime options of the same
                                                    kernels: test_second_segment_every_tile, test_second_segment_grouped
    R16 1:          tiles 1..8                      test_adapter_every_instantiation; lora_group_n is a runtime option: test_group_n
    R16 2, 4:       tiles 1..6 except (6, R16 4)    test_adapter_every_instantiation, test_group_n (tiles 1..3)
    refused:        tiles 7 / 8 with R16 2 / 4 ("tile id"), tile 6 with R16 4 ("does not fit the 160 KB LDS"), tile ids outside 1..8: test_rejected
    refused:        lora_group_n / x2_group_n no multiple of a forced tile's width: test_group_n_rejected, test_second_segment_grouped_rejected;
                    tile 0 moves to tile 3 instead: test_group_n_planner_moves_to_tile_3, test_second_segment_grouped (tile 0)
  lora_group_k, KG 4, BT 0, NS 4
    R16 1, 2, 4:    tiles 1..3                      test_group_k (unsplit, one split per group, and any other split count = unsplit)
    refused:        every other tile ("lora_group_k needs mode 0 and tile 1..3"): test_group_k_rejected
  batch, BT 1, NS 4
    R16 0, KG 0:    tiles 1..3                      test_batched[none]
    R16 1, 2, 4, KG 0: tiles 1..3                   test_batched[gn]
    R16 1, 2, 4, KG 4: tiles 1..3                   test_batched[gk]
    refused:        every other tile ("batched launch needs mode 0 and tile 1..3"): test_batched_rejected
Adapter gradients: lora_grad_mfma_kernel<16 / 32 / 64> and lora_grad_valu_kernel<16 / 32 / 64>: test_grad_linear, test_grad_conv, test_grad_accumulate_and_order;
<64, WIDE> of both at padded ranks 128 / 192 / 256: test_grad_wide.
To add a tile id: add it to TILES / TILE_COLS; to add a shape or a variant: add it to the case lists of gemm_exact_ref (the CPU file checks them all).
"""
import functools

import pytest
import torch

from tests import gemm_exact_ref as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
SENT = -24576.0            # exact in bf16; no result of these operands comes near it
TILES = (1, 2, 3, 4, 5, 6, 7, 8)
TILE_COLS = {1: 128, 2: 128, 3: 64, 4: 128, 5: 128, 6: 256, 7: 160, 8: 160}
SEAM_TILES = (1, 2, 3, 7, 8)
SEAM_SPLITS = (2, 3, 5)                                # K = 576: nine K steps
ADAPTER_OK = [(t, p) for t in TILES for p in R.PADS if not (t in (7, 8) and p > 16) and not (t == 6 and p == 64)]
REJECTED = [(7, 32, "tile id"), (7, 64, "tile id"), (8, 32, "tile id"), (8, 64, "tile id"), (6, 64, "does not fit the 160 KB LDS")]
GROUP_N_OK = [(t, p) for t in (1, 2, 3, 8) for p in R.PADS if not (t == 8 and p > 16)]
N0 = R.N_PLAIN


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def _poisoned(X):
    """X as a view of a wider and taller buffer; everything else in it is NaN: a read outside the operand's rows or columns poisons the result.
    (18 rows behind it: one token too many of a conv-form gradient gathers up to a map row and a pixel beyond the last image.)"""
    wide = torch.full((X.shape[0] + 20, X.shape[1] + 16), NAN, dtype=X.dtype)
    wide[2:2 + X.shape[0], 8:8 + X.shape[1]] = X
    return wide.cuda()[2:2 + X.shape[0], 8:8 + X.shape[1]]


@functools.lru_cache(maxsize=None)
def _dev(M, N, K, idx, gk):
    d = R.operands(M, N, K, idx, gk)
    out = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items() if k not in ("X", "X2")}
    out["X"], out["X2"] = _poisoned(d["X"]), _poisoned(d["X2"])
    return out


def _case_dev(case):
    M, N, K, variant, idx = case
    assert case in R.ALL_CASES, f"{case} is not among the cases tests/test_gemm_exact_cpu.py checks"
    return _dev(M, N, K, idx, R.variant_gk(variant)), R.VARIANTS[variant]


@functools.lru_cache(maxsize=None)
def _want(case, dtype, times=0):
    """The reference in the output's format, on the device: computed once, never written.  times > 0: that many accumulating launches onto `start`."""
    M, N, K, variant, idx = case
    acc, T = R.reference(M, N, K, variant, idx)
    if times:
        acc = R.operands(M, N, K, idx, R.variant_gk(variant))["start"].to(F64) + times * acc
    return R.rounded(acc, dtype).cuda(), (T.cuda() if T is not None else None)


def _framed(M, N, dtype):
    """[M, N] view, NaN-filled, of a sentinel-filled buffer with room for whole 256 x 256 tiles beyond it (a missing mask must not leave the allocation)."""
    rows = (M + 255) // 256 * 256 + 256
    big = torch.full((rows, (N + 255) // 256 * 256 + 264), SENT, dtype=dtype, device="cuda")
    big[:M, :N] = NAN
    return big, big[:M, :N]


def _frame_intact(big, M, N):
    return bool((big[M:] == SENT).all() & (big[:M, N:] == SENT).all())


def _same(got, want, what):
    if torch.equal(got, want):
        return
    got, want = got.reshape(got.shape[0], -1), want.reshape(got.shape[0], -1)
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    r0, c0 = idx[0].tolist()
    rows = sorted(set(idx[:, 0].tolist()))
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at ({r0}, {c0}): got {float(got[r0, c0])}, want {float(want[r0, c0])}; "
                         f"rows {rows[:8]}{'...' if len(rows) > 8 else ''}")


def _outputs(d, v, dtype, with_ct):
    """The framed outputs of one problem: (C, T_out, Ct), each (buffer, view) or None."""
    M, N, tw = d["M"], d["N"], R.t_width(d, v)
    return _framed(M, N, dtype), (_framed(M, tw, BF) if tw else None), (_framed(N, M, BF) if with_ct else None)


def _check(d, v, outs, want, Twant, what):
    (big, out), Tf, Ctf = outs
    M, N = d["M"], d["N"]
    _same(out, want, what)
    assert _frame_intact(big, M, N), f"{what}: wrote outside the [M, N] output"
    if Tf is not None:
        _same(Tf[1], Twant, what + " T_out")
        assert _frame_intact(Tf[0], M, Twant.shape[1]), f"{what}: wrote outside T_out"
    if Ctf is not None:
        _same(Ctf[1], want.to(BF).t(), what + " Ct")
        assert _frame_intact(Ctf[0], N, M), f"{what}: wrote outside Ct"


def _run(ops, case, dtype, *, tile, stages=0, splitk=1, times=1, with_ct=False, accumulate=False, **over):
    """One case on the tiled kernel (forced tile / ring depth / split), `times` launches into the same split-K workspace; checks the output, T_out, Ct and
    their frames and returns the output view.  accumulate: the launches add onto the operand set's `start`, in the same fp32 buffer."""
    d, v = _case_dev(case)
    want, Twant = _want(case, dtype, times if accumulate else 0)
    outs = None
    for rep in range(times):
        if outs is None or not accumulate:
            outs = _outputs(d, v, dtype, with_ct)
            if accumulate:
                outs[0][1].copy_(d["start"])
        kw = R.variant_kwargs(d, v, outs[1][1] if outs[1] else None)
        kw.update(over)
        if with_ct:
            kw["Ct"] = outs[2][1]
        ops.gemm(d["X"], d["W"], outs[0][1], tile=tile, stages=stages, splitk=splitk, accumulate=accumulate, **kw)
        what = f"{case} {dtype} tile {tile} stages {stages} splitk {splitk} launch {rep}"
        if not accumulate or rep == times - 1:
            _check(d, v, outs, want, Twant, what)
    return outs[0][1]


def _refused(ops, case, why, *, tile, stages=0, splitk=1):
    """The library's error, and nothing written - never another tile in silence."""
    d, v = _case_dev(case)
    outs = _outputs(d, v, BF, False)
    with pytest.raises(ops._lib.KernelLibraryError, match=why):
        ops.gemm(d["X"], d["W"], outs[0][1], tile=tile, stages=stages, splitk=splitk, **R.variant_kwargs(d, v, outs[1][1] if outs[1] else None))
    torch.cuda.synchronize()
    for f, (r, c) in zip(outs[:2], ((d["M"], d["N"]), (d["M"], R.t_width(d, v)))):
        if f is not None:
            assert bool(f[1].isnan().all()) and _frame_intact(f[0], r, c), f"{case} tile {tile}: refused, yet something was written"


# ------------------------------------------------------------------------------------------------ 1. plain: every tile, both rings, both formats
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,K", R.MK)
def test_plain(ops, M, K, tile, stages):
    """Without an epilogue, and with all of it: alpha, bias, row bias, residual, Ct."""
    for dtype in (F32, BF):
        _run(ops, (M, N0, K, "plain", 0), dtype, tile=tile, stages=stages)
        _run(ops, (M, N0, K, "full", 0), dtype, tile=tile, stages=stages, with_ct=True)


@pytest.mark.parametrize("tile", TILES)
def test_plain_one_row(ops, tile):
    for dtype in (F32, BF):
        _run(ops, (1, N0, 192, "full", 0), dtype, tile=tile, with_ct=True)
    _run(ops, (1, N0, 192, "plain", 0), F32, tile=tile, splitk=3, times=2)


@pytest.mark.parametrize("tile", TILES)
def test_plain_accumulate(ops, tile):
    """fp32 output += result: two launches give the start value plus twice the product (with the epilogue: twice all of it), unsplit and split."""
    _run(ops, (105, N0, 192, "full", 0), F32, tile=tile, times=2, accumulate=True)
    _run(ops, (280, N0, 576, "plain", 0), F32, tile=tile, stages=2, splitk=3, times=2, accumulate=True)


# ------------------------------------------------------------------------------------------------ 2. split seams
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("splitk", SEAM_SPLITS)
@pytest.mark.parametrize("tile", SEAM_TILES)
@pytest.mark.parametrize("M", R.MS)
def test_split_seams(ops, M, tile, splitk, stages):
    """Twice into the same workspace (the arrival counters re-arm), onto NaN: the bits of the unsplit launch."""
    for dtype in (F32, BF):
        one = _run(ops, (M, N0, 576, "plain", 0), dtype, tile=tile, stages=stages)
        split = _run(ops, (M, N0, 576, "plain", 0), dtype, tile=tile, stages=stages, splitk=splitk, times=2)
        assert torch.equal(split, one)


# ------------------------------------------------------------------------------------------------ 3. fused adapter
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile,pad", ADAPTER_OK)
def test_adapter_every_instantiation(ops, tile, pad, stages):
    for dtype in (F32, BF):
        _run(ops, (105, N0, 192, f"lora{pad}", 0), dtype, tile=tile, stages=stages)


@pytest.mark.parametrize("K,splitk", [(192, 1), (576, 1), (576, 3)])
@pytest.mark.parametrize("cs", ["", "cs"])
@pytest.mark.parametrize("tile,pad", [(t, p) for t in (1, 2, 3) for p in R.PADS] + [(7, 16), (8, 16)])
@pytest.mark.parametrize("M", R.MS)
def test_adapter(ops, M, tile, pad, cs, K, splitk):
    """Output and T_out with rank pads 16 / 32 / 64, with and without col_scale (and alpha = 2), unsplit and split."""
    for dtype in (F32, BF):
        _run(ops, (M, N0, K, f"lora{pad}{cs}", 0), dtype, tile=tile, splitk=splitk, times=2 if splitk > 1 else 1)


@pytest.mark.parametrize("tile", [1, 3, 8])
@pytest.mark.parametrize("M", R.MS)
def test_adapter_full_epilogue(ops, M, tile):
    for dtype in (F32, BF):
        _run(ops, (M, N0, 192, "lora16full", 0), dtype, tile=tile, splitk=3, times=2, with_ct=True)


@pytest.mark.parametrize("tile,pad,why", REJECTED)
def test_rejected(ops, tile, pad, why):
    for stages in (0, 2):
        _refused(ops, (105, N0, 192, f"lora{pad}", 0), why, tile=tile, stages=stages)


def test_rejected_tile_id(ops):
    _refused(ops, (105, N0, 192, "plain", 0), "tile id", tile=9)
    _refused(ops, (105, N0, 192, "lora16", 0), "tile id", tile=9)


# ------------------------------------------------------------------------------------------------ 4. lora_group_n
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("tile,pad", GROUP_N_OK)
def test_group_n(ops, tile, pad, G, splitk):
    """One adapter per group of output columns, the smallest group width the tile takes: T_out [M, G Rp], each group's columns against its own Adown rows."""
    w = R.GROUP_W[tile]
    for M, dtype in ((105, BF), (280, F32), (280, BF)):
        _run(ops, (M, G * w, 192, f"gn{pad}w{w}", 0), dtype, tile=tile, splitk=splitk, times=2 if splitk > 1 else 1)


@pytest.mark.parametrize("pad", R.PADS)
def test_group_n_planner_moves_to_tile_3(ops, pad):
    """tile = 0 with 64-wide groups: whatever the shape heuristics pick, the planner ends on the 64 x 64 tile - result exact, nothing refused."""
    for M in R.MS:
        for G in (2, 3):
            _run(ops, (M, G * 64, 192, f"gn{pad}w64", 0), BF, tile=0, splitk=0)


@pytest.mark.parametrize("tile,w", [(1, 64), (2, 64), (8, 64), (8, 128), (4, 64), (6, 128), (7, 128)])
def test_group_n_rejected(ops, tile, w):
    _refused(ops, (105, 2 * w, 192, f"gn16w{w}", 0), f"lora_group_n={w} is not a multiple", tile=tile)


# ------------------------------------------------------------------------------------------------ 5. lora_group_k
@pytest.mark.parametrize("G", [2, 3, 4])
@pytest.mark.parametrize("pad", R.PADS)
@pytest.mark.parametrize("tile", [1, 2, 3])
def test_group_k(ops, tile, pad, G):
    """One adapter per group of K columns, with residual.  The host check (gemm_plan, `splitk = p.splitk == G ... ? G : 1`) has two sides: splitk = G is
    one split per group, every other forced count (1, G + 1) runs unsplit - each must give the same bits, twice into the same workspace."""
    for M, dtype in ((105, BF), (280, F32)):
        case = (M, N0, G * 64, f"gk{pad}c64", 0)
        one = _run(ops, case, dtype, tile=tile, splitk=1)
        for splitk in (G, G + 1):
            assert torch.equal(_run(ops, case, dtype, tile=tile, splitk=splitk, times=2), one)


@pytest.mark.parametrize("tile", [1, 2, 3])
def test_group_k_wide_groups(ops, tile):
    """Three groups of 192 columns: three K steps per group, the T flush between them."""
    for M, dtype in ((105, F32), (280, BF)):
        for splitk in (1, 3):
            _run(ops, (M, N0, 576, "gk16c192", 0), dtype, tile=tile, splitk=splitk, times=2 if splitk > 1 else 1)


@pytest.mark.parametrize("tile", [4, 5, 6, 7, 8])
def test_group_k_rejected(ops, tile):
    _refused(ops, (105, N0, 128, "gk16c64", 0), "lora_group_k needs mode 0 and tile 1..3", tile=tile)


# ------------------------------------------------------------------------------------------------ 6. batched
def _batch_cases(kind, tile, pad):
    if kind == "none":
        return [(105, N0, 192, "bias", i) for i in range(R.NB)]
    if kind == "gn":
        w = R.GROUP_W[tile]
        return [(105, 2 * w, 192, f"gn{pad}w{w}", i) for i in range(R.NB)]
    return [(105, N0, 128, f"gkb{pad}c64", i) for i in range(R.NB)]


def _run_batch(ops, cases, dtype, tile, with_ct):
    devs = [_case_dev(c) for c in cases]
    v = devs[0][1]
    outs = [_outputs(d, v, dtype, with_ct) for d, _ in devs]
    items = []
    for (d, _), o in zip(devs, outs):
        kw = R.variant_kwargs(d, v, o[1][1] if o[1] else None)
        it = dict(X=d["X"], W=d["W"], C=o[0][1], bias=kw.get("bias"), Ct=o[2][1] if with_ct else None)
        if "lora" in kw:
            it["Adown"], it["Bup"], _s, it["T_out"] = kw["lora"]
        items.append({k: t for k, t in it.items() if t is not None})
    d0 = devs[0][0]
    kw0 = R.variant_kwargs(d0, v, outs[0][1][1] if outs[0][1] else None)
    if with_ct:
        kw0["Ct"] = outs[0][2][1]
    return devs, v, outs, lambda: ops.gemm(d0["X"], d0["W"], outs[0][0][1], tile=tile, batch=ops.GemmBatch(items, d0["X"].device), **kw0)


@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("kind,pad", [("none", 0)] + [(k, p) for k in ("gn", "gk") for p in R.PADS])
def test_batched(ops, kind, pad, tile):
    """Three problems in one launch, each with its own operand set (a swapped pointer shows) and its own framed C / T_out / Ct."""
    cases = _batch_cases(kind, tile, pad)
    for dtype in (BF, F32):
        devs, v, outs, launch = _run_batch(ops, cases, dtype, tile, with_ct=kind != "gk")
        launch()
        for case, (d, _), o in zip(cases, devs, outs):
            want, Twant = _want(case, dtype)
            _check(d, v, o, want, Twant, f"batched {case} {dtype} tile {tile}")


@pytest.mark.parametrize("kind,pad", [("none", 0), ("gn", 16), ("gk", 16)])
def test_batched_rejected(ops, kind, pad):
    cases = _batch_cases(kind, 1, pad)
    devs, v, outs, launch = _run_batch(ops, cases, BF, 4, with_ct=False)
    with pytest.raises(ops._lib.KernelLibraryError, match="tile 1..3"):
        launch()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(o[0][1].isnan().all()) and _frame_intact(o[0][0], devs[0][0]["M"], devs[0][0]["N"])


# ------------------------------------------------------------------------------------------------ 7. second segment
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile", TILES)
def test_second_segment_every_tile(ops, tile, stages):
    for M in R.MS:
        for dtype in (F32, BF):
            _run(ops, (M, N0, 192, "seg2", 0), dtype, tile=tile, stages=stages)
    _run(ops, (280, N0, 192, "seg2", 0), BF, tile=tile, stages=stages, splitk=2, times=2)


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("tile,w", [(3, 64), (1, 128), (2, 128), (0, 64)])
def test_second_segment_grouped(ops, tile, w, G):
    """x2_group_n: output column n reads the X2 columns of group n // w.  tile = 0 with 64-wide groups: the planner ends on the 64 x 64 tile."""
    for M in R.MS:
        for dtype in (F32, BF):
            for splitk in ((0,) if tile == 0 else (1, 2)):
                _run(ops, (M, G * w, 192, f"x2g{w}", 0), dtype, tile=tile, splitk=splitk, times=2 if splitk > 1 else 1)


@pytest.mark.parametrize("tile", [1, 2, 4, 5, 6, 7, 8])
def test_second_segment_grouped_rejected(ops, tile):
    _refused(ops, (105, 128, 192, "x2g64", 0), "x2_group_n=64 is not a multiple", tile=tile)


@pytest.mark.parametrize("tile", [1, 3, 8])
def test_second_segment_slices_of_one_buffer(ops, tile):
    """X and X2 as two column slices of one buffer (the rest of it NaN), the output a slice of a wider one."""
    case = (280, N0, 192, "seg2", 0)
    d = R.operands(*case[:3])
    both = torch.full((280, 192 + R.K2 + 16), NAN, dtype=BF)
    both[:, :192], both[:, 192:192 + R.K2] = d["X"], d["X2"][:, :R.K2]
    both = both.cuda()
    dd, v = _case_dev(case)
    for dtype in (F32, BF):
        outs = _outputs(dd, v, dtype, False)
        ops.gemm(both[:, :192], dd["W"], outs[0][1], X2=both[:, 192:192 + R.K2], W2=dd["W2"], tile=tile, splitk=1)
        _check(dd, v, outs, *_want(case, dtype), f"two slices of one buffer {dtype} tile {tile}")


# ================================================================================================ adapter gradients
GUARD = 1 << 16


def _flat_out(Cw, Rk, Rp, rank_major, start=None):
    """The contiguous fp32 `out` of a gradient problem at the head of a larger buffer: NaN (or `start`) where the result goes, NaN behind it up to the
    padded rank of a rank-major output (ranks >= R must keep it), the sentinel beyond."""
    nan_to = Cw * (Rp if rank_major else Rk)
    big = torch.full((nan_to + GUARD,), SENT, dtype=F32, device="cuda")
    big[:nan_to] = NAN
    if start is not None:
        big[:Cw * Rk] = start
    return big, big[:Cw * Rk], nan_to


def _flat_intact(big, n, nan_to):
    return bool(big[n:nan_to].isnan().all() & (big[nan_to:] == SENT).all())


@functools.lru_cache(maxsize=None)
def _dev_P(M, Cw):
    return _poisoned(R.grad_P(M, Cw))


@functools.lru_cache(maxsize=None)
def _dev_Q(M, Rp, salt=0):
    return _poisoned(R.grad_Q(M, Rp, salt))


@functools.lru_cache(maxsize=None)
def _grad_want(M, Cw, Rp, Rk, rank_major):
    return R.rounded(R.grad_ref(R.grad_P(M, Cw), R.grad_Q(M, Rp), Rk, rank_major), F32).cuda()


@functools.lru_cache(maxsize=None)
def _conv_dev(H, W, Cin, stride):
    g, X, _ = R.conv_problem(H, W, Cin, stride)
    return g, _poisoned(X)


@functools.lru_cache(maxsize=None)
def _conv_want(H, W, Cin, stride, Rp, Rk, rank_major):
    g, _, cols = R.conv_problem(H, W, Cin, stride)
    return R.rounded(R.grad_ref(cols, R.grad_Q(g.M, Rp, 1), Rk, rank_major), F32).cuda()


def _linear_problem(M, Cw, Rp, Rk, rank_major, start=None):
    big, out, nan_to = _flat_out(Cw, Rk, Rp, rank_major, start)
    pr = dict(P=_dev_P(M, Cw), Q=_dev_Q(M, Rp), out=out, M=M, Cw=Cw, R=Rk, rank_major=rank_major, conv=None)
    return pr, big, nan_to, _grad_want(M, Cw, Rp, Rk, rank_major), f"M {M} Cw {Cw} Rp {Rp} R {Rk} rank_major {rank_major}"


def _conv_problem(ops, H, W, Cin, stride, Rp, Rk, rank_major, start=None):
    g, X = _conv_dev(H, W, Cin, stride)
    big, out, nan_to = _flat_out(9 * Cin, Rk, Rp, rank_major, start)
    pr = dict(P=X, Q=_dev_Q(g.M, Rp, 1), out=out, M=g.M, Cw=9 * Cin, R=Rk, rank_major=rank_major,
              conv=ops.ConvGeom(g.B, H, W, Cin, g.Hout, g.Wout, stride=stride))
    return pr, big, nan_to, _conv_want(H, W, Cin, stride, Rp, Rk, rank_major), f"conv {H}x{W} Cin {Cin} stride {stride} Rp {Rp} R {Rk} rank_major {rank_major}"


def _run_plan(ops, probs, Rp, mfma, runs=1, accumulate=False):
    plan = ops.LoraGradPlan([p[0] for p in probs], Rp, torch.device("cuda"))
    assert plan.mfma == int(mfma), "the plan did not pick the kernel family this test is about"
    plan.set_accumulate(accumulate)
    for _ in range(runs):
        plan.run()
    for pr, big, nan_to, want, what in probs:
        _same(pr["out"].view_as(want), want, f"{'mfma' if mfma else 'valu'} {what}")
        assert _flat_intact(big, pr["out"].numel(), nan_to), f"{what}: wrote outside `out`"
    return plan


@pytest.mark.parametrize("Rp", R.PADS)
@pytest.mark.parametrize("mfma", [1, 0])
def test_grad_linear(ops, mfma, Rp):
    """Every M (fewer chunks than waves, a partial last chunk, uneven chunks per wave) x Cw (a partial last 64-column block) x R < Rp, R = Rp x both layouts
    in one plan; the VALU plan holds the Cw = 36 problems that force it."""
    cws = R.GRAD_CWS + (() if mfma else (R.GRAD_CW_VALU,))
    probs = [_linear_problem(M, Cw, Rp, Rk, rm) for M in R.GRAD_MS for Cw in cws for Rk in (Rp - 5, Rp) for rm in (False, True)]
    _run_plan(ops, probs, Rp, mfma)


def _conv_probs(ops, mfma, Rp, stride):
    cins = (64, 192) if mfma else R.CONV_CINS
    return [_conv_problem(ops, H, W, Cin, stride, Rp, Rp - 3, rm) for (H, W) in R.CONV_MAPS for Cin in cins for rm in (False, True)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Rp", [16, 64])
@pytest.mark.parametrize("mfma", [1, 0])
def test_grad_conv(ops, mfma, Rp, stride):
    """P gathered by the forward 3 x 3 geometry, B = 2, maps 5 x 7 and 10 x 14 (image borders inside a 32-token chunk), stride 1 and 2 (odd maps: 3 x 4 out)."""
    _run_plan(ops, _conv_probs(ops, mfma, Rp, stride), Rp, mfma)


@pytest.mark.parametrize("Rp", R.WIDE_RPS)
@pytest.mark.parametrize("mfma", [1, 0])
def test_grad_wide(ops, mfma, Rp):
    """The rank walked in 64-column chunks: R = 65 / 100 / Rp; the ranks >= R of a rank-major `out` keep their NaN, chunks wholly beyond R write nothing."""
    cws = R.GRAD_CWS + (() if mfma else (R.GRAD_CW_VALU,))
    probs = [_linear_problem(M, Cw, Rp, Rk, rm) for M in (33, 280) for Cw in cws for Rk in (65, 100, Rp) for rm in (False, True)]
    _run_plan(ops, probs, Rp, mfma)


@pytest.mark.parametrize("Rp", [16, 64, 192])
@pytest.mark.parametrize("mfma", [1, 0])
def test_grad_accumulate_and_order(ops, mfma, Rp):
    """Four mixed problems whose order the plan's sort by M changes, each result in its own `out`; three accumulating runs onto an integer start value
    give start + 3 x result exactly."""
    Rk = 100 if Rp > 64 else Rp - 5
    specs = [(33, 200, True), (280, 64, False), (1, 200, False), (97, 64 if mfma else R.GRAD_CW_VALU, True)]
    probs = [_linear_problem(M, Cw, Rp, Rk, rm) for (M, Cw, rm) in specs]
    if Rp <= 64:
        probs.insert(2, _conv_problem(ops, 10, 14, 64, 1, Rp, Rp - 3, True))
    _run_plan(ops, probs, Rp, mfma)
    g = torch.Generator().manual_seed(4)
    started = []
    for (pr, _, _, want, what) in probs:
        start = torch.randint(-9, 10, (want.numel(),), generator=g).float().cuda()
        big, out, nan_to = _flat_out(pr["Cw"], pr["R"], Rp, pr["rank_major"], start)
        started.append((dict(pr, out=out), big, nan_to, start.view_as(want) + 3 * want, what + " accumulated"))
    _run_plan(ops, started, Rp, mfma, runs=3, accumulate=True)


# ================================================================================================ weight-gradient chain
@pytest.mark.parametrize("conv", [0, 1])
@pytest.mark.parametrize("M", R.MS)
def test_wgrad_chain(ops, M, conv):
    """wgrad_transpose / wgrad_im2col_t into panels padded to 64 tokens (the pad columns zero: the product runs over them), then dW = dy^T x as an fp32
    product, and once more with accumulate."""
    d = R.wgrad_operands(M, conv)
    Mp = (M + 63) // 64 * 64
    x, dy = _poisoned(d["x"]), _poisoned(d["dy"])
    N, Kw = d["dy"].shape[1], d["cols"].shape[1]
    dyT = torch.full((N, Mp), NAN, dtype=BF, device="cuda")
    xT = torch.full((Kw, Mp), NAN, dtype=BF, device="cuda")
    ops.wgrad_transpose(dy, dyT)
    if conv:
        g = d["geom"]
        ops.wgrad_im2col_t(x, xT, B=g.B, H=g.Hin, W=g.Win)
    else:
        ops.wgrad_transpose(x, xT)
    _same(xT[:, :M], d["cols"].t().to(BF).cuda(), "x panel")
    _same(dyT[:, :M], d["dy"].t().cuda(), "dy panel")
    assert bool((xT[:, M:] == 0).all()) and bool((dyT[:, M:] == 0).all()), "the panels' pad columns must be zero"
    want = R.rounded(d["dW"], F32).cuda()
    for tile in (0, 2):
        big, dW = _framed(N, Kw, F32)
        ops.gemm(dyT, xT, dW, tile=tile)
        _same(dW, want, f"dW M {M} conv {conv} tile {tile}")
        ops.gemm(dyT, xT, dW, tile=tile, accumulate=True)
        _same(dW, 2 * want, f"dW accumulated M {M} conv {conv} tile {tile}")
        assert _frame_intact(big, N, Kw)
