"""Bit-exact parity of the wave-split-K product (sdlt_wsk_gemm / _p / _rowdot / _parts, csrc/wsk.hip) and of the row-strip product of the text
encoders (sdlt_strip_gemm / _pair, csrc/strip.hip) on an MI355X, against the fp64 reference of tests/wsk_exact_ref.py on small-integer operands.
Every partial sum - a wave's quarter of K, a K group, a strip split, a head's or a tile's row sum - is a multiple of 0.25 far below 2^24
(tests/test_wsk_exact_cpu.py asserts it), so no result depends on the wave split, ring depth, refill stagger, tile rotation, strip width, split
count or the order of the float atomics: every comparison here is torch.equal against the reference, never against another launch, and there is no
tolerance.  X, W, O, R, Adown and Bup are views of wider and taller NaN-filled buffers (stray reads poison the result); Y, Y0, T_out and P are
NaN-filled views inside sentinel-filled frames with room for whole tiles beyond them, D and ln_parts carry a sentinel tail (stray writes).
The wave-split-K shapes are the smallest at which each mechanism exists (ops.gemm only routes K >= 1024 and >= 128 tiles here, so the C entry
points are called directly, as tests/test_kernels_gpu.py::test_wsk_gemm does); the strip kernel runs through ops.strip_gemm and ops.pairing().

Instantiations launch_wsk<MBK, JN, R, KG, LN, WP, CONV, RG> of wsk_dispatch<WP, CONV> (R = 3 packed, 2 row-major; each row runs WP = false and true
unless noted), and launch_strip / launch_strip_pair<J, LN, R> of sdlt_strip_gemm / sdlt_strip_gemm_pair - ROUTES below, checked against the two
dispatch ladders by tests/test_wsk_exact_cpu.py::test_route_table:
  launch_wsk<4, 5, R, 0, false, WP>                plain, + bias, + bias + R: test_wsk_plain (every M x N x K), test_wsk_epilogue;
                                                   ln_parts[..., 0]: test_wsk_epilogue[parts]; dotD without an adapter: test_wsk_rowdot
  launch_wsk<4, 5, R, 1, false, WP>                rank pad 16, with and without T_out, col_scale, Y0 with and without R: test_wsk_adapter;
                                                   dotD with Nq = 64 and Nq = M: test_wsk_rowdot; the prefetch hint: test_wsk_prefetch_hint
  launch_wsk<4, 5, R, 1, false, true, false, 2>    rank pad 32, packed only, sdlt_wsk_gemm_p only: test_wsk_rank_pad_32
  launch_wsk<4, 5, R, 3, false, WP>                lora_group_k, G = 2 and 3, seams on and inside the waves' steps: test_wsk_group_k
  launch_wsk<4, 5, R, 0 / 1, true, WP>             OUT OF SCOPE: the folded LayerNorm is nonlinear (rstd); tests/test_kernels_gpu.py::test_wsk_gemm_folded_layernorm
                                                   keeps it under a tolerance.  So is ln_parts[..., 1] (it divides by 80): test_wsk_gemm_row_partials.
  launch_wsk<4, 5, R, 0 / 1, false, WP, true>      wsk_dispatch<*, true> only: tests/test_conv_exact_gpu.py::test_wsk_conv_exact
  launch_strip<1, false, 3>                        16-column strips (N = 16, 48, 2320; 2304 under SDLT_STRIP_WIDE_MIN=4096): test_strip_plain, test_strip_epilogue,
                                                   test_strip_split, test_strip_slabs
  launch_strip<2, false, 2>                        32-column strips (N = 2304): the same tests
  launch_strip_pair<1, false, 3> / <2, false, 2>   test_strip_pair (one launch: pq.launches == 1)
  launch_strip<*, true, *>, launch_strip_pair<*, true, *>   OUT OF SCOPE: the LayerNorm fold, like the activation outputs Y2 / Z, is nonlinear;
                                                   tests/test_kernels_gpu.py::test_strip_gemm keeps them under a tolerance.
Refused before anything is launched (output untouched, sdlt_last_error names the reason): test_wsk_refused, test_strip_refused.  "dotD with N % 64 != 0"
cannot be reached: N % 640 == 0 is checked first and implies it.
To add an instantiation: add its line to ROUTES with the test that runs it, a form to WSK_FORMS / STRIP_FORMS and its cases to the lists of
tests/wsk_exact_ref.py (the CPU file checks every case, and fails on a launch_wsk / launch_strip line that ROUTES does not name)."""
import ctypes as C
import functools

import pytest
import torch

from tests import wsk_exact_ref as R
from tests.test_gemm_exact_gpu import NAN, SENT, _frame_intact, _framed, _poisoned, _same

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD = 12288.0              # what the rows t >= T of a strip output hold before the launch, and must still hold after it (exact in bf16)
KERNELS = "tests/test_kernels_gpu.py::"
# instantiation (as the dispatch ladders spell it) -> the tests of this file that run it, or (None, where it is covered instead)
ROUTES = {
    "launch_wsk<4, 5, R, 0, false, WP>": ("test_wsk_plain", "test_wsk_epilogue", "test_wsk_rowdot"),
    "launch_wsk<4, 5, R, 1, false, WP>": ("test_wsk_adapter", "test_wsk_rowdot", "test_wsk_prefetch_hint"),
    "launch_wsk<4, 5, R, 1, false, true, false, 2>": ("test_wsk_rank_pad_32",),
    "launch_wsk<4, 5, R, 3, false, WP>": ("test_wsk_group_k",),
    "launch_wsk<4, 5, R, 0, true, WP>": (None, KERNELS + "test_wsk_gemm_folded_layernorm"),
    "launch_wsk<4, 5, R, 1, true, WP>": (None, KERNELS + "test_wsk_gemm_folded_layernorm"),
    "launch_wsk<4, 5, R, 0, false, WP, true>": (None, "tests/test_conv_exact_gpu.py::test_wsk_conv_exact"),
    "launch_wsk<4, 5, R, 1, false, WP, true>": (None, "tests/test_conv_exact_gpu.py::test_wsk_conv_exact"),
    "launch_strip<1, false, 3>": ("test_strip_plain", "test_strip_epilogue", "test_strip_split", "test_strip_slabs"),
    "launch_strip<2, false, 2>": ("test_strip_plain", "test_strip_epilogue", "test_strip_split", "test_strip_slabs"),
    "launch_strip_pair<1, false, 3>": ("test_strip_pair",),
    "launch_strip_pair<2, false, 2>": ("test_strip_pair",),
    "launch_strip<1, true, 3>": (None, KERNELS + "test_strip_gemm"),
    "launch_strip<2, true, 2>": (None, KERNELS + "test_strip_gemm"),
    "launch_strip_pair<1, true, 3>": (None, KERNELS + "test_text_encoders_paired_launches_bitwise"),
    "launch_strip_pair<2, true, 2>": (None, KERNELS + "test_text_encoders_paired_launches_bitwise"),
}
# what the tests below run (tests/test_wsk_exact_cpu.py: each is in the reference's lists)
PLAIN_SHAPES = tuple((M, N, K) for (M, N, K, _, _) in R.WSK_PLAIN_CASES)
EPILOGUE_CASES, ADAPTER_CASES, ROWDOT_CASES = R.WSK_EPILOGUE_CASES, R.WSK_ADAPTER_CASES, R.WSK_ROWDOT_CASES
RP32_CASES, GROUP_K_CASES, PREFETCH_CASES = R.WSK_RP32_CASES, R.WSK_GROUP_K_CASES, R.WSK_PREFETCH_CASES
STRIP_NK = tuple((N, K) for N in R.STRIP_NS for K in R.STRIP_KS)
STRIP_EPILOGUE_CASES, STRIP_SPLIT_CASES, STRIP_SLAB_CASES, STRIP_PAIRS = R.STRIP_EPILOGUE_CASES, R.STRIP_SPLIT_CASES, R.STRIP_SLAB_CASES, R.STRIP_PAIRS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _at(got, want, what, where):
    """_same, and on a mismatch also where the first bad element lies (`where(row, column)`)."""
    try:
        _same(got, want, what)
    except AssertionError as e:
        g2 = got.reshape(got.shape[0], -1)
        bad = (g2 != want.reshape(g2.shape)) | g2.isnan()
        r0, c0 = bad.nonzero()[0].tolist()
        raise AssertionError(f"{e}; {where(r0, c0)}") from None


def _wsk_where(r, c):
    """An output element of the wave-split-K kernel: its 64 x 80 tile, and the wave that finishes its 16-row block (wave w adds the four K quarters of row block w)."""
    return f"tile (row {r // R.TILE_M}, column {c // R.TILE_N}), row block / finishing wave {(r % R.TILE_M) // 16}, 16-column unit {(c % R.TILE_N) // 16}"


# ================================================================================================ wave-split-K
@functools.lru_cache(maxsize=None)
def _wsk_dev(M, N, K, gk):
    """The operand set on the device: X, W, O, R, Adown, Bup as views of NaN-filled buffers; the packed copy of W; bias / col_scale as they are."""
    d = R.wsk_operands(M, N, K, gk)
    out = {k: (_poisoned(v) if k in ("X", "W", "O", "residual", "Adown", "Bup") else (v.cuda() if torch.is_tensor(v) else v)) for k, v in d.items()}
    return out


@functools.lru_cache(maxsize=None)
def _packed(M, N, K, gk):
    from sd_lora_trainer_amd import ops as O
    W = _wsk_dev(M, N, K, gk)["W"]
    wp = torch.empty(N * K, dtype=BF, device="cuda")
    O._lib.check(O._lib.load().sdlt_wsk_pack_weight(W.data_ptr(), W.stride(0), N, K, wp.data_ptr(), _stream()), "sdlt_wsk_pack_weight")
    return wp


@functools.lru_cache(maxsize=None)
def _wsk_want(case):
    """The reference in the outputs' formats, on the device: computed once, never written."""
    ref = R.wsk_reference(*case)
    conv = dict(Y=BF, Y0=BF, D=F32, parts=F32)
    return {k: (None if v is None else (v.cuda() if k == "T" else R.rounded(v, conv[k]).cuda())) for k, v in ref.items()}


def _wsk_outputs(case):
    """Framed Y / Y0 / T_out, D and ln_parts with a sentinel tail - fresh for every launch."""
    M, N, K, form, gk = case
    v = R.WSK_FORMS[form]
    o = dict(Y=_framed(M, N, BF))
    if v.get("y0"):
        o["Y0"] = _framed(M, N, BF)
    if v.get("T"):
        o["T"] = _framed(M, R.wsk_t_width(K, v, gk), BF)
    if v.get("dot"):
        n = M * (N // R.HEAD)
        big = torch.full((n + 4096,), SENT, dtype=F32, device="cuda")
        big[:n] = 0.0                                                  # "D must be zero on entry"
        o["D"] = (big, big[:n])
    if v.get("parts"):
        n = M * (N // R.TILE_N) * 2
        big = torch.full((n + 4096,), SENT, dtype=F32, device="cuda")
        big[:n] = NAN
        o["parts"] = (big, big[:n].view(M, N // R.TILE_N, 2))
    return o


def _wsk_block(ops, case, o, packed, **over):
    """The parameter block of a case (sdlt_wsk_gemm_params); `over`: fields set last (the refusals)."""
    M, N, K, form, gk = case
    v, d = R.WSK_FORMS[form], _wsk_dev(M, N, K, gk)
    q = ops._lib.WskGemmParams()
    q.X, q.ldx, q.M, q.N, q.K = d["X"].data_ptr(), d["X"].stride(0), M, N, K
    q.W, q.ldw = (_packed(M, N, K, gk).data_ptr(), 0) if packed else (d["W"].data_ptr(), d["W"].stride(0))
    q.Y, q.ldy = o["Y"][1].data_ptr(), o["Y"][1].stride(0)
    if v.get("bias"):
        q.bias = d["bias"].data_ptr()
    if v.get("R") or v.get("dot"):
        src = d["O"] if v.get("dot") else d["residual"]
        q.R, q.ldr = src.data_ptr(), src.stride(0)
    ad = R.wsk_adapter(d, v, gk)
    if ad:
        q.Adown, q.ld_adown, q.Bup, q.ld_bup = ad[0].data_ptr(), ad[0].stride(0), ad[1].data_ptr(), ad[1].stride(0)
        q.lora_scale, q.lora_rp, q.lora_group_k = R.LORA_SCALE, v["pad"], gk
        if "T" in o:
            q.T_out, q.ld_t = o["T"][1].data_ptr(), o["T"][1].stride(0)
    if v.get("cs"):
        q.col_scale = d["col_scale"].data_ptr()
    if "Y0" in o:
        q.Y0, q.ldy0 = o["Y0"][1].data_ptr(), o["Y0"][1].stride(0)
    if "D" in o:
        q.dotD, q.dot_nq = o["D"][1].data_ptr(), R.wsk_nq(M, v)
    if "parts" in o:
        q.ln_parts = o["parts"][1].data_ptr()
    if v.get("pf"):          # another case's packed weight as "the product that follows"
        Mn, Nn, Kn = R.WSK_REDUCED[(R.WSK_REDUCED.index((M, N, K)) + 1) % len(R.WSK_REDUCED)]
        q.pf_next_w, q.pf_next_n, q.pf_next_k, q.pf_steps = _packed(Mn, Nn, Kn, 0).data_ptr(), Nn, Kn, 2
    for k, val in over.items():
        setattr(q, k, val)
    return q


def _wsk_call(lib, q, entry):
    """`block`: sdlt_wsk_gemm_p; `flat`: the flat entry point that takes the same arguments."""
    if entry == "block":
        return lib.sdlt_wsk_gemm_p(C.byref(q), _stream())
    head = (q.X, q.ldx, q.W, q.ldw, q.M, q.N, q.K, q.bias, q.R, q.ldr, q.Y, q.ldy, q.Adown, q.ld_adown, q.Bup, q.ld_bup, q.lora_scale, q.T_out, q.ld_t, q.lora_group_k)
    if q.dotD:
        return lib.sdlt_wsk_gemm_rowdot(*head, q.dotD, q.dot_nq, _stream())
    if q.ln_parts:
        return lib.sdlt_wsk_gemm_parts(*head, q.ln_parts, _stream())
    return lib.sdlt_wsk_gemm(*head, _stream())


def _flat_can_say(v):
    return not (v.get("cs") or v.get("y0") or v.get("pf") or v.get("pad", 0) > 16)


def _wsk_check(case, o, what):
    M, N, K, form, gk = case
    want = _wsk_want(case)
    _at(o["Y"][1], want["Y"], what, _wsk_where)
    assert _frame_intact(o["Y"][0], M, N), f"{what}: wrote outside Y"
    if "Y0" in o:
        _at(o["Y0"][1], want["Y0"], what + " Y0", _wsk_where)
        assert _frame_intact(o["Y0"][0], M, N), f"{what}: wrote outside Y0"
    if "T" in o:
        tw = want["T"].shape[1]
        _at(o["T"][1], want["T"], what + " T_out", lambda r, c: f"row tile {r // R.TILE_M}, row block / finishing wave {(r % R.TILE_M) // 16}, adapter group {c // 16}")
        assert _frame_intact(o["T"][0], M, tw), f"{what}: wrote outside T_out"
    if "D" in o:
        big, D = o["D"]
        Nq, H = R.wsk_nq(M, R.WSK_FORMS[form]), N // R.HEAD
        _at(D.view(-1, Nq), want["D"].view(-1, Nq), what + " D", lambda r, c: f"batch element {r // H}, head {r % H} (columns {r % H * 64}.., tiles {r % H * 64 // 80} and "
            f"{(r % H * 64 + 63) // 80}), row {(r // H) * Nq + c}")
        assert bool((big[D.numel():] == SENT).all()), f"{what}: wrote behind D"
    if "parts" in o:
        big, parts = o["parts"]
        _at(parts[..., 0], want["parts"], what + " ln_parts[..., 0]", lambda r, c: f"tile (row {r // R.TILE_M}, column {c}), row block / finishing wave {(r % R.TILE_M) // 16}")
        assert not bool(parts[..., 1].isnan().any()), f"{what}: ln_parts[..., 1] was not written"
        assert bool((big[parts.numel():] == SENT).all()), f"{what}: wrote behind ln_parts"


def _wsk_run(ops, case, packed_forms=(False, True)):
    """One case, row-major and packed, through the flat entry point (where one takes the form) and through the parameter block: each against the reference."""
    assert case in R.ALL_WSK_CASES, f"{case} is not among the cases tests/test_wsk_exact_cpu.py checks"
    lib, v = ops._lib.load(), R.WSK_FORMS[case[3]]
    for packed in packed_forms:
        for entry in (("flat", "block") if _flat_can_say(v) else ("block",)):
            o = _wsk_outputs(case)
            rc = _wsk_call(lib, _wsk_block(ops, case, o, packed), entry)
            assert rc == 0, lib.sdlt_last_error()
            _wsk_check(case, o, f"wsk {case} {'packed' if packed else 'row-major'} {entry}")


@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
def test_wsk_plain(ops, M, N, K):
    """Every M x N x K: one / two / odd row-tile counts (both XCD maps), 1 / 3 / 4 / 9 K steps per wave (ring refills, the tile rotation wrapping)."""
    _wsk_run(ops, (M, N, K, "plain", 0))


@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=str)
def test_wsk_epilogue(ops, case):
    """+ bias, + bias + R, and the row sums of the rounded output per 80-column tile (sdlt_wsk_gemm_parts)."""
    _wsk_run(ops, case)


@pytest.mark.parametrize("case", ADAPTER_CASES, ids=str)
def test_wsk_adapter(ops, case):
    """Rank pad 16: with and without T_out, the DoRA column factor, Y0 = the output before the residual, with and without R."""
    _wsk_run(ops, case)


@pytest.mark.parametrize("case", ROWDOT_CASES, ids=str)
def test_wsk_rowdot(ops, case):
    """D onto zeros, Nq = 64 and Nq = M, with and without an adapter; heads straddle the 80-column tiles (two atomic contributions); O is not added to Y."""
    _wsk_run(ops, case)


@pytest.mark.parametrize("case", RP32_CASES, ids=str)
def test_wsk_rank_pad_32(ops, case):
    """Two rank groups of 16 LoRA-down rows: packed weights, parameter block only."""
    _wsk_run(ops, case, packed_forms=(True,))


@pytest.mark.parametrize("case", GROUP_K_CASES, ids=str)
def test_wsk_group_k(ops, case):
    """lora_group_k: T_out [M, 16 G], Bup [N, 16 G]; group seams between the waves' steps, on a wave seam and inside the waves."""
    _wsk_run(ops, case)


@pytest.mark.parametrize("case", PREFETCH_CASES, ids=str)
def test_wsk_prefetch_hint(ops, case):
    """pf_next_w / _n / _k / pf_steps pointing at another packed weight change no bit of Y or T_out."""
    _wsk_run(ops, case)


def _wsk_refused(ops, case, packed, why, entry="block", **over):
    lib = ops._lib.load()
    o = _wsk_outputs(case)
    rc = _wsk_call(lib, _wsk_block(ops, case, o, packed, **over), entry)
    assert rc != 0, f"{case} {over}: not refused"
    msg = lib.sdlt_last_error().decode()
    assert why in msg, f"{case} {over}: refused with '{msg}', expected '{why}'"
    torch.cuda.synchronize()
    for k in ("Y", "Y0", "T"):
        if k in o:
            big, view = o[k]
            assert bool(view.isnan().all()) and _frame_intact(big, view.shape[0], view.shape[1]), f"{case} {over}: refused, yet {k} was written"
    if "D" in o:
        assert bool((o["D"][1] == 0).all()), f"{case} {over}: refused, yet D was written"


def test_wsk_refused(ops):
    """Host-side checks only.  The buffers are those of valid, larger cases."""
    big, four, one = (192, 1280, 768), (128, 640, 1024), (64, 640, 256)
    for packed in (False, True):
        _wsk_refused(ops, big + ("biasR", 0), packed, "M=96", M=96)
        _wsk_refused(ops, big + ("biasR", 0), packed, "N=720", N=720)
        _wsk_refused(ops, big + ("biasR", 0), packed, "K=320", K=320)
        _wsk_refused(ops, big + ("biasR", 0), packed, "M=96", entry="flat", M=96)
        _wsk_refused(ops, big + ("loraT", 0), packed, "lora_rp=64", lora_rp=64)
        _wsk_refused(ops, big + ("loraT", 0), packed, "lora_rp=32", lora_rp=32, lora_group_k=384)
        _wsk_refused(ops, four + ("loraT", 0), packed, "lora_group_k=256", lora_group_k=256)                 # four groups
        _wsk_refused(ops, big + ("loraT", 0), packed, "lora_group_k=288", lora_group_k=288)                  # no multiple of 64
        _wsk_refused(ops, big + ("loraT", 0), packed, "lora_group_k=288", entry="flat", lora_group_k=288)
        d = _wsk_dev(*big, 0)
        _wsk_refused(ops, big + ("biasR", 0), packed, "col_scale (DoRA) needs an adapter", col_scale=d["col_scale"].data_ptr())
        o0 = _framed(192, 1280, BF)
        _wsk_refused(ops, big + ("biasR", 0), packed, "Y0 (the output before the residual) exists for adapter launches", Y0=o0[1].data_ptr(), ldy0=o0[1].stride(0))
        assert bool(o0[1].isnan().all()) and _frame_intact(o0[0], 192, 1280)
        _wsk_refused(ops, one + ("dot64", 0), packed, "O is required", R=None, ldr=0)
        _wsk_refused(ops, one + ("dot64", 0), packed, "O is required", entry="flat", R=None, ldr=0)
    _wsk_refused(ops, big + ("loraT", 0), False, "lora_rp=32", lora_rp=32)                                  # rank pad 32 with a row-major weight


# ================================================================================================ row strip
def _strip_where(Tp, wide):
    def where(r, c):
        w = 32 if wide else 16
        return f"batch element {r // Tp}, token {r % Tp} (row block {(r % Tp) // 16}), strip {c // w} of {w} columns, column block {(c % w) // 16}"
    return where


def _wide(ops, N):
    return N >= ops.STRIP_WIDE_MIN and N % 32 == 0          # csrc/strip.hip strip_wide; the threshold read from the library's own switch


@functools.lru_cache(maxsize=None)
def _strip_W(N, K):
    return _poisoned(R.strip_W(N, K))


@functools.lru_cache(maxsize=None)
def _strip_bias(N):
    return R.strip_bias(N).cuda()


@functools.lru_cache(maxsize=None)
def _strip_rows(kind, B, T, Tp, width):
    """X or R of a case as the kernel reads it: [B Tp, width], the rows t >= T NaN, a view of a wider and taller NaN-filled buffer."""
    src = R.strip_X(B, width) if kind == "X" else R.strip_R(B, width)
    return _poisoned(R.strip_layout(src[:, :T], Tp, NAN))


@functools.lru_cache(maxsize=None)
def _strip_full_dev(B, N, K, form):
    acc, slabs = R.strip_full(B, N, K, form)
    return (R.rounded(acc, BF).cuda() if acc is not None else None), (R.rounded(slabs, F32).cuda() if slabs is not None else None)


def _strip_want(case):
    B, T, Tp, N, K, form = case
    acc, slabs = _strip_full_dev(B, N, K, form)
    return R.strip_layout(acc[:, :T], Tp, PAD) if acc is not None else R.strip_layout(slabs[:, :, :T], Tp, PAD)


def _strip_out(case):
    """(frame, view): Y [B Tp, N] bf16, or P [S, B Tp, N] fp32 between two sentinel slabs (ops.strip_gemm takes a contiguous P); NaN where a result
    goes, PAD in the rows t >= T."""
    B, T, Tp, N, K, form = case
    S = R.STRIP_FORMS[form].get("slabs", 0)
    if S:
        big = torch.full((S + 2, B * Tp, N), SENT, dtype=F32, device="cuda")
        view = big[1:S + 1]
    else:
        big, view = _framed(B * Tp, N, BF)
    view.fill_(NAN)
    view.view(-1, B, Tp, N)[:, :, T:] = PAD
    return big, view


def _strip_issue(ops, case, out):
    B, T, Tp, N, K, form = case
    v = R.STRIP_FORMS[form]
    X, W = _strip_rows("X", B, T, Tp, K), _strip_W(N, K)
    if v.get("slabs"):
        return ops.strip_gemm(X, W, None, B=B, T=T, Tp=Tp, partial=out[1])
    return ops.strip_gemm(X, W, out[1], B=B, T=T, Tp=Tp, bias=_strip_bias(N) if v.get("bias") else None,
                          residual=_strip_rows("R", B, T, Tp, N) if v.get("R") else None, splitk=v.get("split", 1))


def _strip_check(ops, case, out, what):
    B, T, Tp, N, K, form = case
    big, view = out
    want = _strip_want(case)
    if R.STRIP_FORMS[form].get("slabs"):
        for s in range(view.shape[0]):
            _at(view[s], want[s], f"{what} slab {s}", _strip_where(Tp, _wide(ops, N)))
        assert bool((big[0] == SENT).all() & (big[-1] == SENT).all()), f"{what}: wrote outside P"
    else:
        _at(view, want, what, _strip_where(Tp, _wide(ops, N)))
        assert _frame_intact(big, B * Tp, N), f"{what}: wrote outside the output"


def _strip_run(ops, case, times=1):
    assert case in R.ALL_STRIP_CASES, f"{case} is not among the cases tests/test_wsk_exact_cpu.py checks"
    for rep in range(times):
        out = _strip_out(case)
        _strip_issue(ops, case, out)
        _strip_check(ops, case, out, f"strip {case} launch {rep}")


@pytest.mark.parametrize("N,K", STRIP_NK)
def test_strip_plain(ops, N, K):
    """Every B x T x Tp: one token, a full / just-over-full row block, 77 and 80 tokens; pad rows of X are NaN, rows t >= T of the output keep their value."""
    for B in R.STRIP_BS:
        for T in R.STRIP_TS:
            for Tp in R.STRIP_TPS:
                _strip_run(ops, (B, T, Tp, N, K, "plain"))


@pytest.mark.parametrize("case", STRIP_EPILOGUE_CASES, ids=str)
def test_strip_epilogue(ops, case):
    _strip_run(ops, case)


@pytest.mark.parametrize("case", STRIP_SPLIT_CASES, ids=str)
def test_strip_split(ops, case):
    """The in-kernel K split with its last-arriver reduction, twice on the same workspace and counters (the counters re-arm)."""
    _strip_run(ops, case, times=2)


@pytest.mark.parametrize("case", STRIP_SLAB_CASES, ids=str)
def test_strip_slabs(ops, case):
    """Partial fp32 slabs: each slab is the product over its K range; the rows t >= T of every slab are untouched."""
    _strip_run(ops, case)


@pytest.mark.parametrize("pair", STRIP_PAIRS, ids=lambda p: f"{p[0][3]}+{p[1][3]}")
def test_strip_pair(ops, pair):
    """Two problems that differ in N, K, B and T in ONE launch, each against its own reference.  Both take the same strip width under every setting of
    SDLT_STRIP_WIDE_MIN the suite runs (2304 and 2368 are both at or above the default and both below 4096)."""
    a, b = pair
    assert a in R.ALL_STRIP_CASES and b in R.ALL_STRIP_CASES
    assert _wide(ops, a[3]) == _wide(ops, b[3])
    outs = [_strip_out(a), _strip_out(b)]
    with ops.pairing() as pq:
        _strip_issue(ops, a, outs[0])
        _strip_issue(ops, b, outs[1])
    assert pq.launches == 1, f"{pair}: {pq.launches} launches"
    for case, out in zip(pair, outs):
        _strip_check(ops, case, out, f"paired strip {case}")


def _strip_params(ops, case, out, **over):
    B, T, Tp, N, K, form = case
    X, W = _strip_rows("X", B, T, Tp, K), _strip_W(N, K)
    p = ops._lib.StripParams()
    p.X, p.ldx, p.W, p.ldw, p.Y, p.ldy = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), out[1].data_ptr(), out[1].stride(0)
    p.B, p.T, p.Tp, p.N, p.K = B, T, Tp, N, K
    for k, val in over.items():
        setattr(p, k, val)
    return p


def test_strip_refused(ops):
    """Host-side checks only: nothing is launched, the output is unchanged, sdlt_last_error names the reason."""
    lib = ops._lib.load()
    case = (3, 77, 96, 48, 768, "plain")
    slab, cnt = ops.splitk_workspace(torch.device("cuda", torch.cuda.current_device()))
    ws = dict(ws=slab.data_ptr(), ws_bytes=slab.numel(), cnt=cnt.data_ptr(), cnt_len=cnt.numel())
    P = torch.full((3, 3 * 96, 48), NAN, dtype=F32, device="cuda")
    singles = [(dict(T=81), "T=81"), (dict(Tp=64), "Tp=64"), (dict(splitk=4, **ws), "sdlt_strip_gemm: B=3"),
               (dict(P=P.data_ptr(), ldp=48, splitk=3, bias=_strip_bias(48).data_ptr()), "a partial output (P) takes no")]
    for over, why in singles:
        out = _strip_out(case)
        rc = lib.sdlt_strip_gemm(C.byref(_strip_params(ops, case, out, **over)), _stream())
        assert rc != 0, f"{over}: not refused"
        msg = lib.sdlt_last_error().decode()
        assert why in msg, f"{over}: refused with '{msg}', expected '{why}'"
        torch.cuda.synchronize()
        bits = lambda t: t.contiguous().view(torch.int16)      # noqa: E731  (NaN compares unequal to itself)
        assert torch.equal(bits(out[1]), bits(_strip_out(case)[1])) and _frame_intact(out[0], 3 * 96, 48) and bool(P.isnan().all()), f"{over}: refused, yet something was written"
    # pairs: a 32-column problem (the smallest width the library's threshold makes wide) with a 16-column one; an in-kernel split
    n_wide = max(2304, (ops.STRIP_WIDE_MIN + 31) // 32 * 32)
    wide_case = (1, 17, 80, n_wide, 256, "plain")
    assert _wide(ops, n_wide) and not _wide(ops, 48)
    pairs = [((wide_case, {}), (case, {}), "want different strip widths"), ((case, dict(splitk=3, **ws)), ((1, 17, 80, 16, 256, "plain"), {}), "in-kernel K split")]
    for (ca, oa), (cb, ob), why in pairs:
        outs = [_framed(ca[0] * ca[2], ca[3], BF), _framed(cb[0] * cb[2], cb[3], BF)]
        rc = lib.sdlt_strip_gemm_pair(C.byref(_strip_params(ops, ca, outs[0], **oa)), C.byref(_strip_params(ops, cb, outs[1], **ob)), _stream())
        assert rc != 0, f"pair {why}: not refused"
        msg = lib.sdlt_last_error().decode()
        assert why in msg, f"pair refused with '{msg}', expected '{why}'"
        torch.cuda.synchronize()
        for c, o in zip((ca, cb), outs):
            assert bool(o[1].isnan().all()) and _frame_intact(o[0], c[0] * c[2], c[3])
    # ... and ops.pairing() then issues two single launches, each still exact
    a, b = (3, 16, 80, 2304, 768, "bias"), (3, 77, 96, 48, 768, "plain")
    if _wide(ops, a[3]) != _wide(ops, b[3]):
        outs = [_strip_out(a), _strip_out(b)]
        with ops.pairing() as pq:
            _strip_issue(ops, a, outs[0])
            _strip_issue(ops, b, outs[1])
        assert pq.launches == 2
        for c, o in zip((a, b), outs):
            _strip_check(ops, c, o, f"unpaired strip {c}")
