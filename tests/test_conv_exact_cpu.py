"""The exact-arithmetic convolution reference (tests/conv_exact_ref.py) checked without a GPU: conv_ref against torch's own convolutions in
fp64, against the emulation of the kernel's contract (tests/emu_ops.py) with a tolerance of ZERO on every operand set the GPU file
(tests/test_conv_exact_gpu.py) uses, and the bounds that make the arithmetic exact asserted directly."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_exact_ref as R
from tests import emu_ops as E

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

TILED_SETS = [(name, Cin) for name in R.GEOMS for Cin in R.CINS]
WSK_SETS = [(B, H, W, Cin, flip) for (B, H, W) in R.WSK_MAPS for Cin in R.WSK_CINS for flip in (0, 1)]


def _torch_conv(X, Wm, g):
    """The same convolution through F.conv2d / F.conv_transpose2d, in fp64."""
    N = Wm.shape[0]
    x = X.to(F64).reshape(g.B, g.Hin, g.Win, g.Cin).permute(0, 3, 1, 2)
    wk = Wm.to(F64).reshape(N, 3, 3, g.Cin).permute(0, 3, 1, 2)
    if g.tr:
        y = F.conv_transpose2d(x, wk.permute(1, 0, 2, 3), stride=2, padding=1, output_padding=1)
    else:
        if g.ups == 2:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        if g.flip:
            wk = torch.flip(wk, dims=(2, 3))
        y = F.conv2d(x, wk, stride=g.stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(g.M, N)


@pytest.mark.parametrize("kind", ["s1", "s2", "ups", "flip", "tr"])
def test_conv_ref_is_torch_conv(kind):
    """Gaussian operands and odd map sizes (even for stride 2): the nine shifted adds are the library convolution, to fp64 rounding."""
    g = torch.Generator().manual_seed(3)
    geom = R.make_geom(kind, 2, 6 if kind == "s2" else 5, 8 if kind == "s2" else 7, 8)
    X = torch.randn(geom.B * geom.Hin * geom.Win, geom.Cin, generator=g, dtype=F64)
    Wm = torch.randn(11, 9 * geom.Cin, generator=g, dtype=F64)
    got, want = R.conv9(X, Wm, geom), _torch_conv(X, Wm, geom)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name,Cin", TILED_SETS)
def test_tiled_geometries_are_torch_conv(name, Cin):
    """The geometries and integer operands of the GPU file: exact equality with the library convolution."""
    d = R.tiled_operands(name, Cin)
    assert torch.equal(R.conv9(d["X"], d["W"], d["geom"]), _torch_conv(d["X"], d["W"], d["geom"]))


def _check_exact(d, v, ref):
    acc, T = ref
    # the premise, asserted directly: integers or multiples of 0.25, far below 2^24; T small enough for bf16
    assert float(acc.abs().max()) < 2 ** 24
    assert torch.equal(acc * 4, torch.round(acc * 4))
    if not (v.get("cs") or v.get("pad")):
        assert torch.equal(acc, torch.round(acc))
    if T is not None:
        assert float(T.to(F64).abs().max()) <= 256
        Tx = R.conv9(d["X"], d["Adown"][:v["pad"]], d["geom"]) * R.LORA_SCALE
        assert torch.equal(T.to(F64), Tx), "s*T is not exact in bf16"
    g = d["geom"]
    for dtype in (F32, BF):
        T_e = torch.full((g.M, v["pad"]), float("nan"), dtype=BF) if v.get("pad") else None
        out = torch.full((g.M, d["N"]), float("nan"), dtype=dtype)
        E.gemm(d["X"], d["W"], out, conv=E.ConvGeom(**g.as_kwargs()), **R.variant_kwargs(d, v, T_e))
        assert torch.equal(out, R.rounded(acc, dtype)), f"emu_ops.gemm differs from conv_ref ({dtype})"
        if T is not None:
            assert torch.equal(T_e, T), "emu_ops.gemm: T_out differs from conv_ref"


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("name,Cin", TILED_SETS)
def test_tiled_sets_exact(name, Cin, variant):
    _check_exact(R.tiled_operands(name, Cin), R.VARIANTS[variant], R.tiled_reference(name, Cin, variant))


@pytest.mark.parametrize("variant", list(R.WSK_VARIANTS))
@pytest.mark.parametrize("B,H,W,Cin,flip", WSK_SETS)
def test_wsk_sets_exact(B, H, W, Cin, flip, variant):
    _check_exact(R.wsk_operands(B, H, W, Cin, flip), R.WSK_VARIANTS[variant], R.wsk_reference(B, H, W, Cin, flip, variant))


def test_operand_ranges():
    d = R.tiled_operands("s1", 192)
    assert set(d["X"].float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    for k in ("W", "Bup", "W2"):
        assert set(d[k].float().unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert int((d["Adown"] != 0).sum(1).max()) <= 3 and int((d["Adown"] != 0).sum(1).min()) >= 1
    assert set(d["col_scale"].unique().tolist()) <= {0.5, 1.0, 2.0}
    for k in ("bias", "rowbias", "residual"):
        assert torch.equal(d[k].float(), torch.round(d[k].float()))
