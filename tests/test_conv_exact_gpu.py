"""Bit-exact parity of the convolution kernels (MI355X): sdlt_gemm_bf16 mode 1 / MODE 2 on every tile id, rank pad, ring depth and K split, and
sdlt_wsk_conv, against the fp64 reference of tests/conv_exact_ref.py on small-integer operands.  Every partial sum is an integer far below 2^24
(tests/test_conv_exact_cpu.py asserts it), so the result does not depend on summation order, tile, split or ring depth: every comparison here is
torch.equal, there is no tolerance.  Outputs are views of larger sentinel-filled buffers (stray writes), X is a column view of a wider buffer
whose other columns hold NaN (stray reads).

Instantiations of gemm_kernel<MODE != 0> that gemm_plan reaches (csrc/gemm.hip, the plain rows of GEMM_FAMILIES), all launched here with both ring depths (stages 0 / 2):
  mode 1, rank pad 0:          tiles 1..8                         test_every_tile
  mode 1, rank pad 16:         tiles 1..8                         test_adapter_every_instantiation
  mode 1, rank pads 32 / 64:   tiles 1..6 except (6, 64)          test_adapter_every_instantiation
  MODE 2 (second segment):     tiles 1..8                         test_second_segment_every_tile
and refused, asserted in test_rejected: tiles 7 / 8 with rank pad 32 / 64 (not instantiated), tile 6 with rank pad 64 (LDS).
To add a tile id or a geometry: add it to TILES / conv_exact_ref.GEOMS; the matrices below pick it up.
"""
import functools

import pytest
import torch

from tests import conv_exact_ref as R

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SENT = -24576.0            # exact in bf16; no result of these operands comes near it
TILES = (1, 2, 3, 4, 5, 6, 7, 8)
TILE_ROWS = {1: 128, 2: 64, 3: 64, 4: 256, 5: 128, 6: 256, 7: 256, 8: 128}
SEAM_TILES = (1, 2, 3, 7, 8)
SEAM_SPLITS = {64: (2, 3, 5), 192: (2, 4)}      # Cin = 64: 9 K steps, seams on tap starts; Cin = 192: 27 steps, splits 2 and 4 start inside a tap
GEOM_NAMES = tuple(R.GEOMS)
# (tile, rank pad) the dispatch has a kernel for / refuses
ADAPTER_OK = [(t, p) for t in TILES for p in (16, 32, 64) if not (t in (7, 8) and p > 16) and not (t == 6 and p == 64)]
REJECTED = [(7, 32, "tile id"), (7, 64, "tile id"), (8, 32, "tile id"), (8, 64, "tile id"), (6, 64, "does not fit the 160 KB LDS")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def _poisoned_columns(X):
    """X as a column view of a wider buffer; the other columns are NaN: a read outside the row's Cin columns poisons the result."""
    wide = torch.full((X.shape[0], X.shape[1] + 16), NAN, dtype=X.dtype)
    wide[:, 8:8 + X.shape[1]] = X
    return wide.cuda()[:, 8:8 + X.shape[1]]


def _to_device(d):
    out = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items() if k != "X"}
    out["X"] = _poisoned_columns(d["X"])
    return out


@functools.lru_cache(maxsize=None)
def _dev_tiled(name, Cin):
    return _to_device(R.tiled_operands(name, Cin))


@functools.lru_cache(maxsize=None)
def _ref_tiled(name, Cin, variant, dtype):
    """The reference in the output's format, on the device: computed once, never written."""
    acc, T = R.tiled_reference(name, Cin, variant)
    return R.rounded(acc, dtype).cuda(), (T.cuda() if T is not None else None)


def _framed(M, N, dtype):
    """[M, N] view, NaN-filled, of a sentinel-filled buffer with room for whole 256 x 256 tiles beyond it (a missing mask must not leave the allocation)."""
    rows = (M + 255) // 256 * 256 + 256
    big = torch.full((rows, (N + 255) // 256 * 256 + 8), SENT, dtype=dtype, device="cuda")
    big[:M, :N] = NAN
    return big, big[:M, :N]


def _frame_intact(big, M, N):
    return bool((big[M:] == SENT).all() & (big[:M, N:] == SENT).all())


def _same(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    r0, c0 = idx[0].tolist()
    rows = sorted(set(idx[:, 0].tolist()))
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at ({r0}, {c0}): got {float(got[r0, c0])}, want {float(want[r0, c0])}; "
                         f"rows {rows[:8]}{'...' if len(rows) > 8 else ''}")


def _run(ops, name, Cin, variant, dtype, *, tile, stages, splitk, times=1, with_ct=False):
    """One case on the tiled kernel (forced tile / ring depth / split), `times` launches into the same split-K workspace; checks the frames,
    T_out and Ct and returns the output view."""
    d = _dev_tiled(name, Cin)
    g, N, v = d["geom"], d["N"], R.VARIANTS[variant]
    M = g.M
    want, Twant = _ref_tiled(name, Cin, variant, dtype)
    pad = v.get("pad", 0)
    for rep in range(times):
        big, out = _framed(M, N, dtype)
        Tbig, T = _framed(M, pad, BF) if pad else (None, None)
        kw = R.variant_kwargs(d, v, T)
        Ctbig = Ct = None
        if with_ct:
            Ctbig, Ct = _framed(N, M, BF)
            kw["Ct"] = Ct
        ops.gemm(d["X"], d["W"], out, conv=ops.ConvGeom(**g.as_kwargs()), tile=tile, stages=stages, splitk=splitk, **kw)
        what = f"{name} Cin {Cin} {variant} {dtype} tile {tile} stages {stages} splitk {splitk} launch {rep}"
        _same(out, want, what)
        assert _frame_intact(big, M, N), f"{what}: wrote outside the [M, N] output"
        if pad:
            _same(T, Twant, what + " T_out")
            assert _frame_intact(Tbig, M, pad), f"{what}: wrote outside T_out"
        if with_ct:
            _same(Ct, R.rounded(R.tiled_reference(name, Cin, variant)[0], BF).cuda().t(), what + " Ct")
            assert _frame_intact(Ctbig, N, M), f"{what}: wrote outside Ct"
    return out


# ------------------------------------------------------------------------------------------------ every tile, every geometry, both rings
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("Cin", R.CINS)
@pytest.mark.parametrize("name", GEOM_NAMES)
def test_every_tile(ops, name, Cin, tile, stages):
    for dtype in (F32, BF):
        _run(ops, name, Cin, "plain", dtype, tile=tile, stages=stages, splitk=1)


# ------------------------------------------------------------------------------------------------ split seams
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile", SEAM_TILES)
@pytest.mark.parametrize("Cin,splitk", [(c, s) for c in R.CINS for s in SEAM_SPLITS[c]])
@pytest.mark.parametrize("name", GEOM_NAMES)
def test_split_seams(ops, name, Cin, splitk, tile, stages):
    """Twice into the same workspace (the arrival counters re-arm), onto NaN: the bits of the unsplit launch."""
    for dtype in (F32, BF):
        one = _run(ops, name, Cin, "plain", dtype, tile=tile, stages=stages, splitk=1)
        split = _run(ops, name, Cin, "plain", dtype, tile=tile, stages=stages, splitk=splitk, times=2)
        assert torch.equal(split, one)


# ------------------------------------------------------------------------------------------------ fused adapter
@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile,pad", ADAPTER_OK)
def test_adapter_every_instantiation(ops, tile, pad, stages):
    for dtype in (F32, BF):
        _run(ops, "s1", 64, f"lora{pad}", dtype, tile=tile, stages=stages, splitk=1)


@pytest.mark.parametrize("Cin,splitk", [(64, 1), (64, 3), (192, 1), (192, 2)])
@pytest.mark.parametrize("cs", ["", "cs"])
@pytest.mark.parametrize("tile,pad", [(t, p) for t in (1, 2, 3) for p in (16, 32, 64)] + [(7, 16), (8, 16)])
@pytest.mark.parametrize("name", ["s1", "s2", "flip"])
def test_adapter(ops, name, tile, pad, cs, Cin, splitk):
    """Output and T_out with rank pads 16 / 32 / 64, with and without col_scale, unsplit and split (Cin = 192: the seam inside a tap)."""
    for dtype in (F32, BF):
        _run(ops, name, Cin, f"lora{pad}{cs}", dtype, tile=tile, stages=0, splitk=splitk, times=2 if splitk > 1 else 1)


# ------------------------------------------------------------------------------------------------ second segment behind a convolution (MODE 2)
@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("Cin", R.CINS)
@pytest.mark.parametrize("name", GEOM_NAMES)
def test_second_segment(ops, name, Cin, tile, splitk):
    for dtype in (F32, BF):
        _run(ops, name, Cin, "seg2", dtype, tile=tile, stages=0, splitk=splitk, times=2 if splitk > 1 else 1)


@pytest.mark.parametrize("stages", [0, 2])
@pytest.mark.parametrize("tile", TILES)
def test_second_segment_every_tile(ops, tile, stages):
    for dtype in (F32, BF):
        _run(ops, "s1", 64, "seg2", dtype, tile=tile, stages=stages, splitk=1)


# ------------------------------------------------------------------------------------------------ full epilogue, with the transposed copy
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GEOM_NAMES)
def test_full_epilogue_with_ct(ops, name, tile):
    """bias + per-image row bias + residual + Ct; tiles 1, 3 and 8 also with the rank-16 adapter and col_scale in front of them."""
    for dtype in (F32, BF):
        _run(ops, name, 64, "full", dtype, tile=tile, stages=0, splitk=1, with_ct=True)
        if tile in (1, 3, 8):
            _run(ops, name, 64, "lora16full", dtype, tile=tile, stages=0, splitk=2, times=2, with_ct=True)


# ------------------------------------------------------------------------------------------------ what the dispatch refuses
@pytest.mark.parametrize("tile,pad,why", REJECTED)
def test_rejected(ops, tile, pad, why):
    """No kernel for these: the library's error, nothing written - never another tile in silence."""
    d = _dev_tiled("s1", 64)
    g, N = d["geom"], d["N"]
    for stages in (0, 2):
        big, out = _framed(g.M, N, BF)
        Tbig, T = _framed(g.M, pad, BF)
        with pytest.raises(ops._lib.KernelLibraryError, match=why):
            ops.gemm(d["X"], d["W"], out, conv=ops.ConvGeom(**g.as_kwargs()), tile=tile, stages=stages, splitk=1, **R.variant_kwargs(d, R.VARIANTS[f"lora{pad}"], T))
        torch.cuda.synchronize()
        assert bool(out.isnan().all()) and bool(T.isnan().all()) and _frame_intact(big, g.M, N) and _frame_intact(Tbig, g.M, pad)


def test_planner_keeps_the_forced_tile(ops):
    """A forced tile is the tile that runs: the 256-row tiles on M = 105 would be the planner's last choice, and tile ids outside 1..8 are an error."""
    _run(ops, "small", 64, "plain", F32, tile=6, stages=0, splitk=1)
    d = _dev_tiled("small", 64)
    big, out = _framed(d["geom"].M, d["N"], BF)
    with pytest.raises(ops._lib.KernelLibraryError, match="tile id"):
        ops.gemm(d["X"], d["W"], out, conv=ops.ConvGeom(**d["geom"].as_kwargs()), tile=9, splitk=1)
    torch.cuda.synchronize()
    assert bool(out.isnan().all())


# ------------------------------------------------------------------------------------------------ sdlt_wsk_conv
@functools.lru_cache(maxsize=None)
def _dev_wsk(B, H, W, Cin, flip):
    return _to_device(R.wsk_operands(B, H, W, Cin, flip))


@pytest.mark.parametrize("variant", list(R.WSK_VARIANTS))
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("Cin", R.WSK_CINS)
@pytest.mark.parametrize("B,H,W", R.WSK_MAPS)
def test_wsk_conv_exact(ops, B, H, W, Cin, flip, variant):
    """The entry point called directly, row-major and packed weight: N = 640, the smallest maps the host check takes (48-row images: image boundaries inside
    the 64-row tiles), Cin = 64 / 192 / 320 (uneven step counts over the waves), both tap orders, with and without the rank-16 adapter and T_out."""
    d, v = _dev_wsk(B, H, W, Cin, flip), R.WSK_VARIANTS[variant]
    N, M, K = d["N"], B * H * W, 9 * Cin
    acc, Tref = R.wsk_reference(B, H, W, Cin, flip, variant)
    want = R.rounded(acc, BF).cuda()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    zero = ops.zero_page(d["X"].device)
    wp = torch.empty(N * K, dtype=BF, device="cuda")
    ops._lib.check(lib.sdlt_wsk_pack_weight(d["W"].data_ptr(), K, N, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
    lora = bool(v.get("pad"))
    A, Bu = (d["Adown"][:16], d["Bup"][:, :16]) if lora else (None, None)
    bias = d["bias"] if v.get("bias") else None
    rowb = d["rowbias"] if v.get("rowbias") else None
    res = d["residual"] if v.get("residual") else None
    P = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    L = lambda t: t.stride(0) if t is not None else 0          # noqa: E731
    for wptr, ldw, which in ((d["W"].data_ptr(), K, "row-major"), (wp.data_ptr(), 0, "packed")):
        big, y = _framed(M, N, BF)
        Tbig, T = _framed(M, 16, BF) if lora else (None, None)
        rc = lib.sdlt_wsk_conv(d["X"].data_ptr(), L(d["X"]), wptr, ldw, B, H, W, Cin, N, flip, P(bias), P(rowb), L(rowb), P(res), L(res), y.data_ptr(), L(y),
                               P(A), L(A), P(Bu), L(Bu), R.LORA_SCALE if lora else 0.0, P(T), L(T), zero.data_ptr(), st)
        assert rc == 0, lib.sdlt_last_error()
        what = f"wsk conv {B}x{H}x{W} Cin {Cin} flip {flip} {variant} {which}"
        _same(y, want, what)
        assert _frame_intact(big, M, N), f"{what}: wrote outside the output"
        if lora:
            _same(T, Tref.cuda(), what + " T_out")
            assert _frame_intact(Tbig, M, 16), f"{what}: wrote outside T_out"
