"""The exact-arithmetic reference of the linear products and the adapter gradients (tests/gemm_exact_ref.py) checked without a GPU, on every
operand set and variant the GPU file (tests/test_gemm_exact_gpu.py) uses: (a) the fp64 result survives fp32 unchanged, (b) the bounds that make
the arithmetic exact, asserted directly, (c) equality with the emulation of the kernels' contract (tests/emu_ops.py) with a tolerance of ZERO in
fp32 and bf16, (d) equality with a second fp64 formulation written differently (one masked / block-diagonal product instead of per-group loops)."""
import pytest
import torch
import torch.nn.functional as F

from tests import emu_ops as E
from tests import gemm_exact_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")


def _blockdiag_x2(kw, N):
    """The grouped second segment as a plain one: W2 spread block-diagonally over [N, G K2], so that column n meets only its group's X2 columns."""
    kw = dict(kw)
    w = kw.pop("x2_group_n", 0)
    if w:
        W2, k2 = kw["W2"], kw["W2"].shape[1]
        wide = torch.zeros(N, (N // w) * k2, dtype=W2.dtype)
        for g in range(N // w):
            wide[g * w:(g + 1) * w, g * k2:(g + 1) * k2] = W2[g * w:(g + 1) * w]
        kw["W2"] = wide
    return kw


def _masked_formulation(d, kw):
    """The same contract written without group loops: every grouped term is one product against a masked (block-structured) operand."""
    x, w = d["X"].to(F64), d["W"].to(F64)
    M, N, K = d["M"], d["N"], d["K"]
    kw = _blockdiag_x2(kw, N)
    acc = torch.matmul(x, w.t())
    if "X2" in kw:
        acc = acc + torch.matmul(kw["X2"].to(F64), kw["W2"].to(F64).t())
    T = None
    if "lora" in kw:
        A, Bu, s = kw["lora"]
        a, bu = A.to(F64), Bu.to(F64)
        n = torch.arange(N)
        if kw.get("lora_group_k"):
            C, Rp = kw["lora_group_k"], A.shape[0]
            G = K // C
            big = torch.zeros(G * Rp, K, dtype=F64)                      # row g Rp + r = Adown row r, masked to group g's columns
            grp = torch.arange(K) // C
            for g in range(G):
                big[g * Rp:(g + 1) * Rp] = a * (grp == g).to(F64)[None, :]
            T = torch.matmul(x, big.t())
            up = bu
        elif kw.get("lora_group_n"):
            Rp, wd = Bu.shape[1], kw["lora_group_n"]
            G = N // wd
            T = torch.matmul(x, a.t())                                     # [M, G Rp]
            up = torch.zeros(N, G * Rp, dtype=F64)                       # Bup row n sits in the columns of group n // w
            mask = (torch.arange(G * Rp)[None, :] // Rp == (n // wd)[:, None]).to(F64)
            up = bu.repeat(1, G) * mask
        else:
            T, up = torch.matmul(x, a.t()), bu
        T = (T * s).to(F32).to(BF)
        acc = acc + torch.matmul(T.to(F64), up.t())
    scale = torch.full((N,), float(kw.get("alpha", 1.0)), dtype=F64)
    if "col_scale" in kw:
        scale = scale * kw["col_scale"].to(F64)
    acc = acc * scale[None, :]
    if "bias" in kw:
        acc = acc + kw["bias"].to(F64)
    if "rowbias" in kw:
        onehot = F.one_hot(torch.arange(M) // kw["rows_per_batch"], kw["rowbias"].shape[0]).to(F64)
        acc = acc + torch.matmul(onehot, kw["rowbias"].to(F64))
    if "residual" in kw:
        acc = acc + kw["residual"].to(F64)
    return acc, T


@pytest.mark.parametrize("M,N,K,variant,idx", R.ALL_CASES)
def test_gemm_cases_exact(M, N, K, variant, idx):
    v = R.VARIANTS[variant]
    d = R.operands(M, N, K, idx, R.variant_gk(variant))
    acc, T = R.reference(M, N, K, variant, idx)
    # (b) the premise: multiples of 0.25 below 2^20 (so that two more launches accumulated onto |start| <= 16 stay far below 2^24), s*T a multiple
    # of 0.5 with |s*T| <= 3 per adapter group - three +-1 against |x| <= 2, halved - which bf16 (8 significant bits) holds exactly
    assert float(acc.abs().max()) < 2 ** 20
    assert torch.equal(acc * 4, torch.round(acc * 4))
    if not v.get("pad"):
        assert torch.equal(acc * 2, torch.round(acc * 2))
    kw3 = R.variant_kwargs(d, v, four=False)
    if T is not None:
        assert tuple(T.shape) == (M, R.t_width(d, v))
        assert float(T.to(F64).abs().max()) <= 3.0 and torch.equal(T.to(F64) * 2, torch.round(T.to(F64) * 2))
    # (d) the second formulation
    acc2, T2 = _masked_formulation(d, kw3)
    assert torch.equal(acc, acc2), "per-group loops and masked products differ"
    if T is not None:
        assert torch.equal(T, T2)
    # (a) + (c): fp32 holds the fp64 value (rounded() asserts it); the emulation gives the same bits in both output formats, also when accumulating
    for dtype in (F32, BF):
        want = R.rounded(acc, dtype)
        T_e = torch.full((M, R.t_width(d, v)), NAN, dtype=BF) if v.get("pad") else None
        Ct = torch.full((N, M), NAN, dtype=BF)
        out = torch.full((M, N), NAN, dtype=dtype)
        E.gemm(d["X"], d["W"], out, Ct=Ct, **_blockdiag_x2(R.variant_kwargs(d, v, T_e), N))
        assert torch.equal(out, want), f"emu_ops.gemm differs from gemm_ref ({dtype})"
        assert torch.equal(Ct, R.rounded(acc, BF).t()), "emu_ops.gemm: Ct differs"
        if T is not None:
            assert torch.equal(T_e, T), "emu_ops.gemm: T_out differs from gemm_ref"
    out = d["start"].clone()
    for _ in range(2):
        E.gemm(d["X"], d["W"], out, accumulate=True, **_blockdiag_x2(R.variant_kwargs(d, v, None), N))
    assert torch.equal(out, R.rounded(d["start"].to(F64) + 2 * acc, F32))


def test_batched_problems_differ():
    """A swapped operand pointer of a batched launch must show: the problems' results differ from each other."""
    for case in R.BATCH_CASES:
        M, N, K, variant, idx = case
        if idx:
            assert not torch.equal(R.reference(M, N, K, variant, idx)[0], R.reference(M, N, K, variant, 0)[0])


def test_operand_ranges():
    d = R.operands(280, 200, 576)
    for k in ("X", "X2"):
        assert set(d[k].float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    for k in ("W", "Bup", "W2"):
        assert set(d[k].float().unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert int((d["Adown"] != 0).sum(1).max()) <= 3 and int((d["Adown"] != 0).sum(1).min()) >= 1
    assert set(d["col_scale"].unique().tolist()) <= {0.5, 1.0, 2.0}
    for k in ("bias", "rowbias", "residual", "start"):
        assert torch.equal(d[k].float(), torch.round(d[k].float()))
    dk = R.operands(105, 200, 256, 0, 64)                              # K-grouped: the three entries of a row lie inside every group of 64 columns
    per_group = (dk["Adown"] != 0).reshape(-1, 4, 64).sum(2)
    assert int(per_group.max()) <= 3 and int(per_group.min()) >= 1
    for variant, v in R.VARIANTS.items():                              # alpha = 0.5 only on integer products, alpha = 2 with the adapter's halves
        assert v.get("alpha", 1.0) == (2.0 if v.get("cs") else (0.5 if variant == "full" else 1.0))


# ---------------------------------------------------------------------------------------------------------------- adapter gradients
def _grad_sets():
    sets = [(M, Cw, Rp) for M in R.GRAD_MS for Cw in R.GRAD_CWS + (R.GRAD_CW_VALU,) for Rp in R.PADS]
    return sets + [(M, Cw, Rp) for M in (33, 280) for Cw in R.GRAD_CWS + (R.GRAD_CW_VALU,) for Rp in R.WIDE_RPS]


def _ranks(Rp):
    return (65, 100, Rp) if Rp > 64 else (Rp - 5, Rp)


@pytest.mark.parametrize("M,Cw,Rp", _grad_sets())
def test_grad_sets_exact(M, Cw, Rp):
    P, Q = R.grad_P(M, Cw), R.grad_Q(M, Rp)
    for Rk in _ranks(Rp):
        for rank_major in (False, True):
            ref = R.grad_ref(P, Q, Rk, rank_major)
            assert float(ref.abs().max()) <= 4 * M < 2 ** 22 and torch.equal(ref, torch.round(ref))      # (b): integers; 3 accumulated runs stay below 2^24
            want = R.rounded(ref, F32)                                                                   # (a)
            out = torch.full((Cw * Rk,), NAN, dtype=F32)
            plan = E.LoraGradPlan([dict(P=P, Q=Q, out=out, M=M, Cw=Cw, R=Rk, rank_major=rank_major, conv=None)], Rp, "cpu")
            plan.run()
            assert torch.equal(out.view_as(want), want)                                                  # (c)
            plan.set_accumulate(True)
            plan.run(), plan.run()
            assert torch.equal(out.view_as(want), 3 * want)
            alt = torch.einsum("mc,mr->cr", P.to(F64), Q.to(F64))[:, :Rk]                                # (d)
            assert torch.equal(ref, alt.t() if rank_major else alt)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin", R.CONV_CINS)
@pytest.mark.parametrize("H,W", R.CONV_MAPS)
def test_grad_conv_sets_exact(H, W, Cin, stride):
    g, X, cols = R.conv_problem(H, W, Cin, stride)
    x = X.to(F64).reshape(g.B, H, W, Cin).permute(0, 3, 1, 2)
    unf = F.unfold(x, 3, padding=1, stride=stride)                                                       # (d): the library's own im2col, (ci, tap) order
    assert unf.shape[-1] == g.Hout * g.Wout
    assert torch.equal(cols, unf.reshape(g.B, Cin, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * Cin))
    for Rp in (16, 64):
        Q = R.grad_Q(g.M, Rp, salt=1)
        for rank_major in (False, True):
            ref = R.grad_ref(cols, Q, Rp - 3, rank_major)
            want = R.rounded(ref, F32)
            assert float(ref.abs().max()) <= 4 * g.M
            out = torch.full((9 * Cin * (Rp - 3),), NAN, dtype=F32)
            cg = E.ConvGeom(g.B, H, W, Cin, g.Hout, g.Wout, stride=stride)
            E.LoraGradPlan([dict(P=X, Q=Q, out=out, M=g.M, Cw=9 * Cin, R=Rp - 3, rank_major=rank_major, conv=cg)], Rp, "cpu").run()
            assert torch.equal(out.view_as(want), want)


@pytest.mark.parametrize("conv", [0, 1])
@pytest.mark.parametrize("M", R.MS)
def test_wgrad_chain_exact(M, conv):
    """dW = dy^T x through the emulated panels (pad columns zero) and the emulated product, twice with accumulate: the reference's bits."""
    d = R.wgrad_operands(M, conv)
    Mp = (M + 63) // 64 * 64
    dyT = E.wgrad_transpose(d["dy"], torch.full((d["dy"].shape[1], Mp), NAN, dtype=BF))
    if conv:
        g = d["geom"]
        xT = E.wgrad_im2col_t(d["x"], torch.full((9 * 64, Mp), NAN, dtype=BF), B=g.B, H=g.Hin, W=g.Win)
    else:
        xT = E.wgrad_transpose(d["x"], torch.full((d["x"].shape[1], Mp), NAN, dtype=BF))
    assert torch.equal(xT[:, :M].to(F64), d["cols"].t()) and bool((xT[:, M:] == 0).all()) and bool((dyT[:, M:] == 0).all())
    want = R.rounded(d["dW"], F32)
    assert float(d["dW"].abs().max()) <= 4 * M
    dW = torch.full(tuple(want.shape), NAN, dtype=F32)
    E.gemm(dyT, xT, dW)
    assert torch.equal(dW, want)
    E.gemm(dyT, xT, dW, accumulate=True)
    assert torch.equal(dW, 2 * want)
    assert torch.equal(d["dW"], torch.einsum("mn,mk->nk", d["dy"].to(F64), d["cols"]))
