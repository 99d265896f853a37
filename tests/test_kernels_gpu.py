"""Per-kernel parity (MI355X): every C-ABI entry point against the torch restatement of its contract
(tests/emu_ops.py, fp32 math on the same bf16 inputs).  Tolerance for bf16 outputs: 1.5e-2 of the
reference's max-abs (one bf16 ulp is 0.4-0.8 %; accumulation is fp32 on both sides) - written in `close`.
"""
import math
import os

import pytest
import torch

from tests import emu_ops as E

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sd_lora_trainer_amd import ops as O
    O._lib.load()
    return O


def close(got, ref, tol=1.5e-2, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol * scale + 1e-6, f"{what}: max err {err:.4g} vs scale {scale:.4g} (tol {tol})"


def rnd(*shape, g, scale=1.0, dtype=BF):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def dev(*ts):
    return [t.cuda() if t is not None else None for t in ts]


# --------------------------------------------------------------------------------------------- folded LayerNorm
def _ln_case(M, N, K, G, rank, g, mean=0.7, std=1.5):
    """Operands of a LayerNorm folded into the projection behind it, the way unet.Linear.fold_ln / StackedLinear.fold_ln build them:
    raw rows x (non-zero mean), W o gamma, c1, c2, per-adapter A o gamma + constants; plus the UNFOLDED reference y = LN(x), W, A."""
    x = (torch.randn(M, K, generator=g) * std + mean + torch.randn(M, 1, generator=g)).to(BF)
    gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    W32 = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g) * 0.1
    Wg, c1, c2 = E.fold_layernorm(W32, bias, gamma, beta, dtype=BF)
    A32 = [torch.randn(rank, K, generator=g) * K ** -0.5 for _ in range(G)] if rank else []
    Bup = rnd(N, 16, g=g, scale=0.3) if rank else None
    if rank:
        Bup[:, rank:] = 0
    Ag, consts = torch.zeros(G * 16, K, dtype=BF), torch.zeros(G * 32)
    items = [dict(A32=A32[i], gamma=gamma, beta=beta, Ag=Ag[i * 16:(i + 1) * 16], consts=consts[i * 32:(i + 1) * 32]) for i in range(G if rank else 0)]
    E.LnFoldPlan(items, "cpu").run()
    return dict(x=x, gamma=gamma, beta=beta, W32=W32, bias=bias, Wg=Wg, c1=c1, c2=c2, A32=A32, Bup=Bup, Ag=Ag, consts=consts)


def _ln_reference(c, M, N, G, rank, scale, residual=None, geglu=False):
    """The unfolded computation in fp32 on the same bf16 inputs: y = bf16(LN(x)); out = y W^T + b + s bf16(y A^T) B^T (+ residual)."""
    K = c["x"].shape[1]
    y = torch.nn.functional.layer_norm(c["x"].float(), (K,), c["gamma"], c["beta"], 1e-5)
    xf = c["x"].float()
    stats = torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-5)], 1)
    out = y @ c["W32"].t() + c["bias"]
    T = None
    if rank:
        gn = N // G
        T = torch.cat([y @ torch.nn.functional.pad(a, (0, 0, 0, 16 - rank)).t() for a in c["A32"]], 1) * scale
        for i in range(G):
            out[:, i * gn:(i + 1) * gn] += T[:, i * 16:(i + 1) * 16].to(BF).float() @ c["Bup"][i * gn:(i + 1) * gn].float().t()
    if residual is not None:
        out = out + residual.float()
    return out, T, stats, y


@pytest.mark.parametrize("M,N,K,G,rank,tile,stages,mode", [
    (1024, 3840, 1280, 3, 16, 0, 0, "plain"),      # attn1 q|k|v of the 1280-wide blocks (128 x 128 tiles, deep ring)
    (4096, 1920, 640, 3, 16, 0, 0, "plain"),       # ... of the 640-wide blocks (shallow ring)
    (4096, 640, 640, 1, 8, 0, 0, "res"),           # attn2.to_q, 640 wide
    (1000, 960, 320, 3, 4, 0, 0, "plain"),         # SD1.5 320-wide stack: 64 x 64 tiles (group width 320), ragged M
    (2048, 320, 320, 1, 16, 8, 0, "ct"),           # 128 x 160 tile with an adapter + transposed copy
    (256, 1280, 1280, 1, 16, 2, 4, "plain"),       # 64 x 128 tile
    (1024, 10240, 1280, 0, 0, 0, 0, "geglu"),      # ff.net.0.proj + GEGLU, 256 x 160 tiles
    (4096, 5120, 640, 0, 0, 0, 0, "geglu"),
    (300, 640, 320, 0, 0, 3, 0, "geglu"),          # ragged M, 64 x 64 tile
    (256, 2560, 320, 0, 0, 8, 0, "geglu"),
])
def test_gemm_folded_layernorm(ops, M, N, K, G, rank, tile, stages, mode):
    """sdlt_gemm_params.ln_c1: LayerNorm folded into the tiled product - against the UNFOLDED fp32 computation on the same inputs
    (LN -> projection -> adapter), row statistics against torch, T_out against the unfolded adapter product."""
    g = torch.Generator().manual_seed(M + N + K)
    scale = 0.75
    c = _ln_case(M, N, K, max(G, 1), rank, g)
    res = rnd(M, N, g=g) if mode == "res" else None
    ref, Tref, stats_ref, _ = _ln_reference(c, M, N, max(G, 1), rank, scale, residual=res)
    xd, Wg, c1, c2, Ag, consts, Bup, resd = dev(c["x"], c["Wg"], c["c1"], c["c2"], c["Ag"], c["consts"], c["Bup"], res)
    out = torch.empty(M, N, dtype=BF, device="cuda")
    stats = torch.zeros(M, 2, device="cuda")
    T = torch.zeros(M, 16 * max(G, 1), dtype=BF, device="cuda") if rank else None
    kw = dict(bias=c2, ln=(c1, stats, 1e-5, consts if rank else None), tile=tile, stages=stages)
    if rank:
        kw.update(lora=(Ag, Bup, scale, T), lora_group_n=N // G if G > 1 else 0)
    Ct = gout = None
    if mode == "geglu":
        perm = E.geglu_perm(N // 2).cuda()
        Wg, c1, c2 = Wg[perm].contiguous(), c1[perm].contiguous(), c2[perm].contiguous()
        gout = torch.empty(M, N // 2, dtype=BF, device="cuda")
        kw.update(bias=c2, ln=(c1, stats, 1e-5, None), geglu_out=gout)
    if mode == "ct":
        Ct = torch.zeros(N, M, dtype=BF, device="cuda")
        kw["Ct"] = Ct
    if res is not None:
        kw["residual"] = resd
    ops.gemm(xd, Wg, out, **kw)
    torch.cuda.synchronize()
    close(stats[:, 0], stats_ref[:, 0], tol=2e-3, what="mean")
    close(stats[:, 1], stats_ref[:, 1], tol=2e-3, what="rstd")
    if mode == "geglu":
        refp = ref[:, perm.cpu()]
        close(out, refp, what="F1")
        h, gt = ref.chunk(2, dim=1)
        close(gout, h * torch.nn.functional.gelu(gt), tol=2e-2, what="geglu")
    else:
        close(out, ref, what="out")
    if rank:
        close(T, Tref, what="T_out")
    if Ct is not None:
        close(Ct.t(), ref, what="Ct")


@pytest.mark.parametrize("M,N,K,rank,res", [(1024, 1280, 1280, 16, False), (1024, 1280, 1280, 4, True), (512, 1280, 2560, 16, True), (1024, 1280, 1280, 0, True)])
def test_wsk_gemm_folded_layernorm(ops, M, N, K, rank, res):
    """sdlt_wsk_gemm_ln (attn2.to_q of the 1280-wide blocks) against the unfolded fp32 computation; the kernel must be the one that ran."""
    assert ops.wsk_shape(M, N, K, rank > 0) or rank == 0
    g = torch.Generator().manual_seed(M + K + rank)
    scale = 1.0
    c = _ln_case(M, N, K, 1, rank, g, mean=-1.2, std=2.0)
    r = rnd(M, N, g=g) if res else None
    ref, Tref, stats_ref, _ = _ln_reference(c, M, N, 1, rank, scale, residual=r)
    xd, Wg, c1, c2, Ag, consts, Bup, rd = dev(c["x"], c["Wg"], c["c1"], c["c2"], c["Ag"], c["consts"], c["Bup"], r)
    out = torch.empty(M, N, dtype=BF, device="cuda")
    stats = torch.zeros(M, 2, device="cuda")
    T = torch.zeros(M, 16, dtype=BF, device="cuda") if rank else None
    lib = ops._lib.load()
    ops._lib.check(lib.sdlt_wsk_gemm_ln(xd.data_ptr(), K, Wg.data_ptr(), K, M, N, K, c2.data_ptr(), rd.data_ptr() if res else None, N if res else 0, out.data_ptr(), N,
                                        Ag.data_ptr() if rank else None, K if rank else 0, Bup.data_ptr() if rank else None, 16 if rank else 0, scale,
                                        T.data_ptr() if rank else None, 16 if rank else 0, c1.data_ptr(), stats.data_ptr(), 1e-5, consts.data_ptr() if rank else None,
                                        torch.cuda.current_stream().cuda_stream), "sdlt_wsk_gemm_ln")
    torch.cuda.synchronize()
    close(stats[:, 0], stats_ref[:, 0], tol=2e-3, what="mean")
    close(stats[:, 1], stats_ref[:, 1], tol=2e-3, what="rstd")
    close(out, ref, what="out")
    if rank:
        close(T, Tref, what="T_out")
        # ops.gemm routes the same call to the same kernel: identical bits
        out2, T2 = torch.empty_like(out), torch.zeros_like(T)
        ops.gemm(xd, Wg, out2, bias=c2, residual=rd, lora=(Ag, Bup, scale, T2), ln=(c1, stats, 1e-5, consts))
        torch.cuda.synchronize()
        assert torch.equal(out2, out) and torch.equal(T2, T)


@pytest.mark.parametrize("M,N,K,rank", [(1024, 1280, 2560, 0), (1000, 640, 640, 8), (1024, 1280, 1280, 16)])
@pytest.mark.parametrize("ratio", [8.0, 30.0])
def test_folded_layernorm_kwalk_statistics_with_offset(ops, M, N, K, rank, ratio):
    """The consumers that compute the row statistics in their own K walk (no row partials from the producer: sdlt_wsk_gemm_ln, the tiled kernel's ln_c1 path) form
    var = E[x^2] - mean^2 from fp32 sums, which loses (mean / std)^2 of the fp32 precision on rows whose mean dwarfs their spread (the partial-sum path merges centred
    sums and does not).  The bound this test pins: relative error of rstd <= 1e-3 + 3e-6 (1 + (mean / std)^2) - 1.2e-3 at ratio 8 (the UNet's LayerNorm inputs stay
    below 3), 3.7e-3 at 30 - against fp64 statistics of the same bf16 rows."""
    g = torch.Generator().manual_seed(int(M + N + K + ratio))
    std = 1.5
    c = _ln_case(M, N, K, 1, rank, g, mean=ratio * std, std=std)
    xd, Wg, c1, c2, Ag, consts, Bup = dev(c["x"], c["Wg"], c["c1"], c["c2"], c["Ag"], c["consts"], c["Bup"])
    out, stats = torch.empty(M, N, dtype=BF, device="cuda"), torch.zeros(M, 2, device="cuda")
    kw = dict(lora=(Ag, Bup, 1.0, torch.zeros(M, 16, dtype=BF, device="cuda"))) if rank else {}
    ops.gemm(xd, Wg, out, bias=c2, ln=(c1, stats, 1e-5, consts if rank else None), **kw)
    torch.cuda.synchronize()
    x64 = c["x"].double()
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-5)
    bound = 1e-3 + 3e-6 * (1.0 + ratio ** 2)
    assert float(((stats[:, 0].cpu().double() - mean) / mean).abs().max()) <= 1e-5
    err = float(((stats[:, 1].cpu().double() - rstd) / rstd).abs().max())
    assert err <= bound, (err, bound)
    ref, _, _, _ = _ln_reference(c, M, N, 1, rank, 1.0)            # the output stays the unfolded computation's
    close(out, ref, tol=3e-2, what="out")


@pytest.mark.parametrize("M,N,K,G,rank,mode", [(1024, 3840, 1280, 3, 16, "plain"), (1024, 1280, 1280, 1, 16, "ct"), (1024, 10240, 1280, 0, 0, "geglu"),
                                                 (1000, 640, 640, 1, 8, "plain")])
def test_gemm_folded_layernorm_from_row_partials(ops, M, N, K, G, rank, mode):
    """sdlt_gemm_params.ln_parts: the statistics are the sum of the row partials the producing launch left (here: computed from x the way
    sdlt_wsk_gemm_parts does); same contract as the K-walk statistics, checked against the unfolded computation.  (The last case has no kernel
    variant for partials: they are ignored and the K walk computes the statistics - same result.)"""
    g = torch.Generator().manual_seed(M + N + K + 1)
    scale = 1.0
    c = _ln_case(M, N, K, max(G, 1), rank, g, mean=40.0 if mode == "plain" else 0.7)     # (rows whose mean dwarfs their spread: the merged partials stay exact)
    ref, Tref, stats_ref, _ = _ln_reference(c, M, N, max(G, 1), rank, scale)
    P = K // 80
    xt = c["x"].float().view(M, P, 80)
    parts = torch.stack([xt.sum(2), ((xt - xt.mean(2, keepdim=True)) ** 2).sum(2)], 2).contiguous()
    xd, Wg, c1, c2, Ag, consts, Bup, partsd = dev(c["x"], c["Wg"], c["c1"], c["c2"], c["Ag"], c["consts"], c["Bup"], parts)
    out = torch.empty(M, N, dtype=BF, device="cuda")
    stats = torch.zeros(M, 2, device="cuda")
    T = torch.zeros(M, 16 * max(G, 1), dtype=BF, device="cuda") if rank else None
    kw = dict(bias=c2, ln=(c1, stats, 1e-5, consts if rank else None, partsd, P))
    if rank:
        kw.update(lora=(Ag, Bup, scale, T), lora_group_n=N // G if G > 1 else 0)
    gout = Ct = None
    if mode == "geglu":
        perm = E.geglu_perm(N // 2).cuda()
        Wg, c1, c2 = Wg[perm].contiguous(), c1[perm].contiguous(), c2[perm].contiguous()
        gout = torch.empty(M, N // 2, dtype=BF, device="cuda")
        kw.update(bias=c2, ln=(c1, stats, 1e-5, None, partsd, P), geglu_out=gout)
    if mode == "ct":
        Ct = torch.zeros(N, M, dtype=BF, device="cuda")
        kw["Ct"] = Ct
    ops.gemm(xd, Wg, out, **kw)
    torch.cuda.synchronize()
    close(stats[:, 0], stats_ref[:, 0], tol=2e-3, what="mean")
    close(stats[:, 1], stats_ref[:, 1], tol=2e-3, what="rstd")
    if mode == "geglu":
        close(out, ref[:, perm.cpu()], what="F1")
        h, gt = ref.chunk(2, dim=1)
        close(gout, h * torch.nn.functional.gelu(gt), tol=2e-2, what="geglu")
    else:
        close(out, ref, what="out")
    if rank:
        close(T, Tref, what="T_out")
    if Ct is not None:
        close(Ct.t(), ref, what="Ct")


@pytest.mark.parametrize("M,N,K,rank,res", [(1024, 1280, 1280, 16, True), (1024, 1280, 5120, 0, True), (512, 1280, 2560, 8, False)])
def test_wsk_gemm_row_partials(ops, M, N, K, rank, res):
    """sdlt_wsk_gemm_parts: the output is bit-identical to sdlt_wsk_gemm and the partials are (sum, centred sum of squares) of the ROUNDED output rows per
    80-column tile; ops.gemm_emits_parts names exactly these shapes."""
    assert ops.gemm_emits_parts(M, N, K, 16 if rank else 0) == N // 80
    g = torch.Generator().manual_seed(M + K + rank + 7)
    x, w, b = rnd(M, K, g=g), rnd(N, K, g=g, scale=K ** -0.5), torch.randn(N, generator=g)
    r = rnd(M, N, g=g) if res else None
    A, Bu = (rnd(16, K, g=g, scale=K ** -0.5), rnd(N, 16, g=g, scale=0.3)) if rank else (None, None)
    if rank:
        A[rank:] = 0
    xd, wd, bd, rd, Ad, Bd = dev(x, w, b, r, A, Bu)
    o0, o1 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, N, dtype=BF, device="cuda")
    parts = torch.zeros(M, N // 80, 2, device="cuda")
    lora = (Ad, Bd, 1.0, None) if rank else None
    ops.gemm(xd, wd, o0, bias=bd, residual=rd, lora=lora)
    ops.gemm(xd, wd, o1, bias=bd, residual=rd, lora=lora, ln_parts_out=parts)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1)
    ot = o1.float().view(M, N // 80, 80)
    close(parts[:, :, 0], ot.sum(2), tol=1e-4, what="row sums")
    close(parts[:, :, 1], ((ot - ot.mean(2, keepdim=True)) ** 2).sum(2), tol=1e-4, what="centred row sums of squares")


@pytest.mark.parametrize("M,C,rank", [(1024, 1280, 16), (4096, 640, 4), (130, 320, 8)])
def test_layernorm_bwd_y_and_fold_plan(ops, M, C, rank):
    """sdlt_layernorm_bwd_y: dx identical to sdlt_layernorm_bwd, y = the forward kernel's rows; sdlt_ln_fold_adapters against its restatement."""
    g = torch.Generator().manual_seed(M + C)
    x, dy, dres = rnd(M, C, g=g, scale=2.0), rnd(M, C, g=g), rnd(M, C, g=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd, dyd, dresd, gd, bd = dev(x, dy, dres, gamma, beta)
    y0, stats = torch.empty(M, C, dtype=BF, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.layernorm_fwd(xd, y0, stats, gamma=gd, beta=bd)
    dx0, dx1, y1 = (torch.empty(M, C, dtype=BF, device="cuda") for _ in range(3))
    ops.layernorm_bwd(xd, dyd, dx0, stats, gamma=gd, dres=dresd)
    ops.layernorm_bwd(xd, dyd, dx1, stats, gamma=gd, dres=dresd, beta=bd, y_out=y1)
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1) and torch.equal(y0, y1)
    A32 = torch.randn(3, rank, C, generator=g) * C ** -0.5
    Ag_ref, c_ref = torch.zeros(3, 16, C, dtype=BF), torch.zeros(3, 32)
    E.LnFoldPlan([dict(A32=A32[i], gamma=gamma, beta=beta, Ag=Ag_ref[i], consts=c_ref[i]) for i in range(3)], "cpu").run()
    A32d = A32.cuda()
    Ag, cc = torch.full((3, 16, C), 7.0, dtype=BF, device="cuda"), torch.full((3, 32), 7.0, device="cuda")
    ops.LnFoldPlan([dict(A32=A32d[i], gamma=gd, beta=bd, Ag=Ag[i], consts=cc[i]) for i in range(3)], "cuda").run()
    torch.cuda.synchronize()
    assert torch.equal(Ag.cpu(), Ag_ref)
    close(cc, c_ref, tol=1e-4, what="constants")


# --------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,H,K,tile,splitk", [(300, 320, 128, 0, 0), (1024, 640, 320, 7, 0), (1024, 640, 320, 8, 0), (256, 64, 512, 3, 2),
                                                 (1000, 1280, 320, 1, 0), (128, 160, 1024, 2, 4)])
def test_gemm_fused_geglu_epilogues(ops, M, H, K, tile, splitk):
    """sdlt_gemm_params.epi_op: ff.net.0.proj with the GEGLU product as a side output (1) and the dX of ff.net.2 with GEGLU's
    backward as its epilogue (2), both on the interleaved-16 layout; 160-column tiles, split-K, ragged M included."""
    g = torch.Generator().manual_seed(M + H)
    x, w1, b1 = rnd(M, K, g=g), rnd(2 * H, K, g=g, scale=K ** -0.5), torch.randn(2 * H, generator=g)
    perm = E.geglu_perm(H)
    w1p, b1p = w1[perm].contiguous(), b1[perm].contiguous()
    f1_ref, g_ref = torch.empty(M, 2 * H, dtype=BF), torch.empty(M, H, dtype=BF)
    E.gemm(x, w1p, f1_ref, bias=b1p, geglu_out=g_ref)
    # the interleaved layout is a pure column permutation of the ordinary projection
    plain = torch.empty(M, 2 * H, dtype=BF)
    E.gemm(x, w1, plain, bias=b1)
    assert torch.equal(plain[:, perm], f1_ref) and torch.allclose(g_ref.float(), E.geglu_fwd(plain, torch.empty(M, H, dtype=BF)).float(), atol=2e-2, rtol=2e-2)
    xd, wd, bd = dev(x, w1p, b1p)
    f1, gg = torch.empty(M, 2 * H, dtype=BF, device="cuda"), torch.empty(M, H, dtype=BF, device="cuda")
    ops.gemm(xd, wd, f1, bias=bd, geglu_out=gg, tile=tile, splitk=splitk)
    close(f1, f1_ref, what="fused geglu: projection")
    close(gg, g_ref, what="fused geglu: hidden * gelu(gate)")
    dy, w2t = rnd(M, K, g=g), rnd(H, K, g=g, scale=K ** -0.5)          # dX of ff.net.2: dG = dy . W2 with W2^T [H, K]
    df1_ref = torch.empty(M, 2 * H, dtype=BF)
    E.gemm(dy, w2t, None, geglu_bwd=(f1_ref, df1_ref))
    df1 = torch.full((M, 2 * H), 7.0, dtype=BF, device="cuda")
    ops.gemm(dy.cuda(), w2t.cuda(), None, geglu_bwd=(f1_ref.cuda(), df1), tile=tile if tile not in (7, 8) or H % 160 == 0 else 0, splitk=splitk)
    close(df1, df1_ref, tol=2e-2, what="fused geglu backward")


@pytest.mark.parametrize("M,N,K,tile", [(256, 256, 128, 1), (200, 136, 64, 1), (77, 320, 192, 2), (1000, 77, 128, 3),
                                        (1, 1280, 320, 0), (4096, 640, 640, 0), (300, 4, 576, 3), (700, 300, 256, 4),
                                        (333, 260, 320, 5)])
def test_gemm_plain_epilogue(ops, M, N, K, tile):
    g = torch.Generator().manual_seed(M + N + K)
    X, W = rnd(M, K, g=g), rnd(N, K, g=g, scale=1 / math.sqrt(K))
    bias = torch.randn(N, generator=g)
    R = rnd(M, N, g=g)
    rowb = rnd(4, N, g=g)
    rpb = (M + 3) // 4
    for out_dtype in (BF, F32):
        ref = E.gemm(X, W, torch.empty(M, N, dtype=out_dtype), bias=bias, residual=R, rowbias=rowb, rows_per_batch=rpb, alpha=0.5)
        Ct = torch.zeros(N, M + 8, dtype=BF).cuda()
        Xd, Wd, bd, Rd, rbd = dev(X, W, bias, R, rowb)
        out = ops.gemm(Xd, Wd, torch.empty(M, N, dtype=out_dtype, device="cuda"), bias=bd, residual=Rd, rowbias=rbd,
                       rows_per_batch=rpb, alpha=0.5, Ct=Ct, tile=tile)
        close(out, ref, what=f"gemm {M}x{N}x{K} {out_dtype}")
        close(Ct[:, :M], ref.t(), what="gemm Ct")


def test_gemm_strided_views_and_two_segments(ops):
    g = torch.Generator().manual_seed(5)
    M, N, K1, K2 = 520, 192, 128, 64
    big = rnd(M, K1 + K2 + 64, g=g)
    X1, X2 = big[:, :K1], big[:, K1:K1 + K2]
    W = rnd(N, K1 + K2, g=g, scale=0.1)
    ref = E.gemm(X1, W[:, :K1], torch.empty(M, N, dtype=BF), X2=X2, W2=W[:, K1:])
    bigd, Wd = dev(big, W)
    outbig = torch.zeros(M, N + 64, dtype=BF, device="cuda")
    ops.gemm(bigd[:, :K1], Wd[:, :K1], outbig[:, :N], X2=bigd[:, K1:K1 + K2], W2=Wd[:, K1:])
    close(outbig[:, :N], ref, what="2-segment strided")
    assert float(outbig[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K,r,tile", [(256, 256, 128, 16, 1), (333, 200, 192, 4, 2), (77, 640, 2048, 16, 3),
                                          (1024, 1280, 1280, 16, 0), (130, 64, 64, 24, 3), (200, 128, 64, 64, 1),
                                          (600, 256, 384, 16, 4), (600, 256, 384, 32, 4), (300, 256, 384, 64, 5),
                                          (300, 256, 384, 40, 4), (300, 256, 384, 16, 2), (300, 256, 384, 64, 2)])
def test_gemm_fused_lora(ops, M, N, K, r, tile):
    g = torch.Generator().manual_seed(M * 3 + r)
    Rp = 16 if r <= 16 else (32 if r <= 32 else 64)
    X, W = rnd(M, K, g=g), rnd(N, K, g=g, scale=1 / math.sqrt(K))
    A = torch.zeros(Rp, K, dtype=BF)
    A[:r] = rnd(r, K, g=g, scale=1 / math.sqrt(K))
    Bu = torch.zeros(N, Rp, dtype=BF)
    Bu[:, :r] = rnd(N, r, g=g, scale=0.3)
    bias = torch.randn(N, generator=g)
    Tref = torch.empty(M, Rp, dtype=BF)
    ref = E.gemm(X, W, torch.empty(M, N, dtype=BF), lora=(A, Bu, 0.75, Tref), bias=bias)
    Xd, Wd, Ad, Bd, bd = dev(X, W, A, Bu, bias)
    T = torch.full((M, Rp), 7.0, dtype=BF, device="cuda")
    out = ops.gemm(Xd, Wd, torch.empty(M, N, dtype=BF, device="cuda"), lora=(Ad, Bd, 0.75, T), bias=bd, tile=tile)
    close(T, Tref, what="lora T_out")
    close(out, ref, what=f"lora gemm {M}x{N}x{K} r{r}")
    # the adapter must actually contribute
    base = E.gemm(X, W, torch.empty(M, N, dtype=BF), bias=bias)
    assert float((ref.float() - base.float()).abs().max()) > 0.05


@pytest.mark.parametrize("M,N,K,r,tile,splitk", [(256, 256, 1280, 0, 1, 3), (1024, 1280, 1280, 16, 0, 0), (1024, 1280, 5120, 0, 0, 0),
                                                 (77, 640, 2048, 16, 0, 0), (300, 200, 640, 8, 3, 5), (130, 520, 1920, 64, 1, 4)])
def test_gemm_split_k(ops, M, N, K, r, tile, splitk):
    """split-K path: fp32 partial tiles meet in the workspace, last arriver reduces; run twice (counter re-arm)."""
    g = torch.Generator().manual_seed(M + K + r)
    X, W = rnd(M, K, g=g), rnd(N, K, g=g, scale=1 / math.sqrt(K))
    bias, R = torch.randn(N, generator=g), rnd(M, N, g=g)
    lora_c = lora_g = None
    Tref = T = None
    if r:
        Rp = 16 if r <= 16 else (32 if r <= 32 else 64)
        A = torch.zeros(Rp, K, dtype=BF)
        A[:r] = rnd(r, K, g=g, scale=1 / math.sqrt(K))
        Bu = torch.zeros(N, Rp, dtype=BF)
        Bu[:, :r] = rnd(N, r, g=g, scale=0.3)
        Tref, T = torch.empty(M, Rp, dtype=BF), torch.zeros(M, Rp, dtype=BF, device="cuda")
        lora_c, lora_g = (A, Bu, 1.0, Tref), (A.cuda(), Bu.cuda(), 1.0, T)
    ref = E.gemm(X, W, torch.empty(M, N, dtype=BF), lora=lora_c, bias=bias, residual=R)
    Xd, Wd, bd, Rd = dev(X, W, bias, R)
    for rep in range(3):
        out = ops.gemm(Xd, Wd, torch.zeros(M, N, dtype=BF, device="cuda"), lora=lora_g, bias=bd, residual=Rd, tile=tile, splitk=splitk,
                       stages=(0, 2, 0)[rep])
        close(out, ref, what=f"split-K gemm rep {rep}")
        if r:
            close(T, Tref, what="split-K lora T_out")


CONV_CASES = [
    dict(B=2, H=16, W=16, Cin=64, Cout=128, stride=1, ups=1, flip=0, tr=0),
    dict(B=1, H=16, W=24, Cin=128, Cout=64, stride=2, ups=1, flip=0, tr=0),
    dict(B=2, H=8, W=8, Cin=64, Cout=64, stride=1, ups=2, flip=0, tr=0),
    dict(B=2, H=12, W=16, Cin=64, Cout=192, stride=1, ups=1, flip=1, tr=0),
    dict(B=1, H=8, W=12, Cin=128, Cout=64, stride=1, ups=1, flip=1, tr=1),
    dict(B=1, H=64, W=64, Cin=320, Cout=320, stride=1, ups=1, flip=0, tr=0),
]


@pytest.mark.parametrize("c", CONV_CASES)
def test_conv3x3_implicit_gemm(ops, c):
    g = torch.Generator().manual_seed(c["H"] * 7 + c["Cin"])
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    if c["tr"]:
        Hout, Wout = 2 * H, 2 * W
    else:
        Hout, Wout = H * c["ups"] // c["stride"], W * c["ups"] // c["stride"]
    X = rnd(B * H * W, Cin, g=g)
    Wm = rnd(Cout, 9 * Cin, g=g, scale=1 / math.sqrt(9 * Cin))
    bias = torch.randn(Cout, generator=g)
    R = rnd(B * Hout * Wout, Cout, g=g)
    rowb = rnd(B, Cout, g=g)
    for mod, mk, st in ((E, lambda t: t, 0), (ops, lambda t: t.cuda(), 0), (ops, lambda t: t.cuda(), 2)):
        geom = mod.ConvGeom(B, H, W, Cin, Hout, Wout, stride=c["stride"], ups=c["ups"], flip=c["flip"], tr=c["tr"])
        out = mod.gemm(mk(X), mk(Wm), mk(torch.empty(B * Hout * Wout, Cout, dtype=BF)), conv=geom, bias=mk(bias), residual=mk(R),
                       rowbias=mk(rowb), rows_per_batch=Hout * Wout, stages=st)
        if mod is E:
            ref = out
        else:
            close(out, ref, what=f"conv {c} stages {st}")


def test_conv3x3_fused_lora_and_strided_input(ops):
    g = torch.Generator().manual_seed(11)
    B, H, W, Cin, Cout, r, Rp = 2, 16, 16, 64, 128, 8, 16
    wide = rnd(B * H * W, Cin + 64, g=g)
    X = wide[:, 64:]
    Wm = rnd(Cout, 9 * Cin, g=g, scale=1 / math.sqrt(9 * Cin))
    A = torch.zeros(Rp, 9 * Cin, dtype=BF)
    A[:r] = rnd(r, 9 * Cin, g=g, scale=0.05)
    Bu = torch.zeros(Cout, Rp, dtype=BF)
    Bu[:, :r] = rnd(Cout, r, g=g, scale=0.3)
    Tref = torch.empty(B * H * W, Rp, dtype=BF)
    ref = E.gemm(X, Wm, torch.empty(B * H * W, Cout, dtype=BF), conv=E.ConvGeom(B, H, W, Cin, H, W), lora=(A, Bu, 1.0, Tref))
    wd, Wd, Ad, Bd = dev(wide, Wm, A, Bu)
    T = torch.empty(B * H * W, Rp, dtype=BF, device="cuda")
    out = ops.gemm(wd[:, 64:], Wd, torch.empty(B * H * W, Cout, dtype=BF, device="cuda"), conv=ops.ConvGeom(B, H, W, Cin, H, W),
                   lora=(Ad, Bd, 1.0, T))
    close(T, Tref, what="conv lora T")
    close(out, ref, what="conv lora out")


@pytest.mark.parametrize("B,H,W,Cin,Cout,flip,lora,extras", [(1, 32, 32, 128, 1280, 0, False, True), (1, 32, 32, 192, 1280, 1, False, True), (4, 16, 16, 128, 1280, 0, True, True),
                                                              (2, 16, 32, 64, 640, 1, False, False), (1, 32, 32, 320, 1280, 0, True, False), (1, 32, 32, 1280, 1280, 0, False, True)])
def test_wsk_conv(ops, B, H, W, Cin, Cout, flip, lora, extras):
    """sdlt_wsk_conv - the 3 x 3 convolutions of the 32 x 32 level on the wave-split-K kernel (K = 9 Cin split over the waves of ONE workgroup per output tile, no
    split-K partials through HBM) - against the emulation of the tiled kernel's contract (bias, per-image row bias, residual, fused rank-16 adapter with T_out) and
    against the tiled kernel itself; Cin = 192 / 320 give the waves UNEVEN step counts (K / 64 not a multiple of 4), flip = the input gradient's mirrored taps, several
    images per batch, a non-square map; the packed (frozen) weight gives the same bits as the row-major one, and ops.gemm routes these shapes here."""
    g = torch.Generator().manual_seed(B + H + Cin + flip)
    M, K = B * H * W, 9 * Cin
    X = rnd(M, Cin, g=g)
    Wm = rnd(Cout, K, g=g, scale=1 / math.sqrt(K))
    bias = torch.randn(Cout, generator=g) if extras else None
    R = rnd(M, Cout, g=g) if extras else None
    rowb = rnd(B, Cout, g=g) if extras else None
    A = Bu = None
    kw = {}
    Tref = torch.empty(M, 16, dtype=BF)
    if lora:
        A, Bu = rnd(16, K, g=g, scale=0.05), rnd(Cout, 16, g=g, scale=0.3)
        kw = dict(lora=(A, Bu, 0.75, Tref))
    ref = E.gemm(X, Wm, torch.empty(M, Cout, dtype=BF), conv=E.ConvGeom(B, H, W, Cin, H, W, flip=flip), bias=bias, residual=R, rowbias=rowb, rows_per_batch=H * W, **kw)
    Xd, Wd, bd, Rd, rbd, Ad, Bd = dev(X, Wm, bias, R, rowb, A, Bu)
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    zero = ops.zero_page(Xd.device)
    wp = torch.empty(Cout * K, dtype=BF, device="cuda")
    ops._lib.check(lib.sdlt_wsk_pack_weight(Wd.data_ptr(), K, Cout, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
    P = lambda t: t.data_ptr() if t is not None else None      # noqa: E731

    def run(wptr, ldw):
        y, T = torch.full((M, Cout), 7.0, dtype=BF, device="cuda"), torch.full((M, 16), 7.0, dtype=BF, device="cuda")
        rc = lib.sdlt_wsk_conv(Xd.data_ptr(), Cin, wptr, ldw, B, H, W, Cin, Cout, flip, P(bd), P(rbd), Cout if extras else 0, P(Rd), Cout if extras else 0, y.data_ptr(), Cout,
                               P(Ad), K if lora else 0, P(Bd), 16 if lora else 0, 0.75 if lora else 0.0, T.data_ptr() if lora else None, 16 if lora else 0, zero.data_ptr(), st)
        assert rc == 0, lib.sdlt_last_error()
        torch.cuda.synchronize()
        return y, T
    y, T = run(Wd.data_ptr(), K)
    close(y, ref, what="wsk conv")
    if lora:
        close(T, Tref, what="wsk conv T_out")
    yp, Tp = run(wp.data_ptr(), 0)
    assert torch.equal(yp, y) and torch.equal(Tp, T), "packed weight: different bits"
    assert torch.equal(run(wp.data_ptr(), 0)[0], yp)
    # the tiled kernel (an explicit tile keeps it there) and ops.gemm's routing
    geom = ops.ConvGeom(B, H, W, Cin, H, W, flip=flip)
    kwd = dict(bias=bd, residual=Rd, rowbias=rbd, rows_per_batch=H * W)
    y2, T2 = torch.empty(M, Cout, dtype=BF, device="cuda"), torch.empty(M, 16, dtype=BF, device="cuda")
    ops.gemm(Xd, Wd, y2, conv=geom, tile=2, **kwd, **(dict(lora=(Ad, Bd, 0.75, T2)) if lora else {}))
    close(y, y2, tol=1e-2, what="wsk conv vs tiled kernel")
    if ops.wsk_conv_shape(geom, Cout, 16 if lora else 0):
        ops.wsk_mark_frozen(Wd)
        y3, T3 = torch.empty(M, Cout, dtype=BF, device="cuda"), torch.empty(M, 16, dtype=BF, device="cuda")
        ops.gemm(Xd, Wd, y3, conv=geom, **kwd, **(dict(lora=(Ad, Bd, 0.75, T3)) if lora else {}))
        assert torch.equal(y3, y) and (not lora or torch.equal(T3, T)), "ops.gemm did not take the wave-split-K route for this convolution"
        assert Wd.data_ptr() in ops._WSK_PACKED


# --------------------------------------------------------------------------------------------- LoRA grads
def test_lora_grad_grouped(ops):
    g = torch.Generator().manual_seed(21)
    probs_cpu, probs_gpu = [], []
    specs = [(300, 200, 16, 16, False, None), (1024, 640, 4, 16, True, None), (77, 2048, 16, 16, True, None),
             (2 * 8 * 8, 9 * 64, 8, 16, True, (2, 8, 8, 64))]
    for (M, Cw, R, Rp, rank_major, conv) in specs:
        Q = rnd(M, Rp, g=g)
        out = torch.zeros(Cw * R, dtype=F32)
        if conv is None:
            P = rnd(M, Cw, g=g)
            cg_c = cg_g = None
        else:
            B, H, W, Cin = conv
            P = rnd(B * H * W, Cin, g=g)
            cg_c, cg_g = E.ConvGeom(B, H, W, Cin, H, W), ops.ConvGeom(B, H, W, Cin, H, W)
        probs_cpu.append(dict(P=P, Q=Q, out=out, M=M, Cw=Cw, R=R, rank_major=rank_major, conv=cg_c))
        probs_gpu.append(dict(P=P.cuda(), Q=Q.cuda(), out=torch.full((Cw * R,), 3.0, dtype=F32, device="cuda"), M=M, Cw=Cw, R=R,
                              rank_major=rank_major, conv=cg_g))
    E.LoraGradPlan(probs_cpu, 16, "cpu").run()
    plan = ops.LoraGradPlan(probs_gpu, 16, torch.device("cuda"))
    plan.run()
    for pc, pg in zip(probs_cpu, probs_gpu):
        close(pg["out"], pc["out"], tol=2e-3, what=f"lora grad M={pc['M']} Cw={pc['Cw']}")
    plan.set_accumulate(True)
    plan.run()
    for pc, pg in zip(probs_cpu, probs_gpu):
        close(pg["out"], 2 * pc["out"], tol=2e-3, what="lora grad accumulate")


@pytest.mark.parametrize("M,C,K,G,tile,splitk", [(200, 128, 192, 3, 0, 0), (128, 256, 256, 2, 1, 0), (128, 128, 512, 4, 2, 2), (520, 64, 128, 3, 3, 1)])
def test_gemm_grouped_lora(ops, M, C, K, G, tile, splitk):
    """Stacked projections (fused to_q|to_k|to_v): one adapter per group of C output columns."""
    g = torch.Generator().manual_seed(M + C + G)
    Rp = 16
    X, W = rnd(M, K, g=g), rnd(G * C, K, g=g, scale=0.2)
    Ad, Bu = rnd(G * Rp, K, g=g, scale=0.3), rnd(G * C, Rp, g=g, scale=0.3)
    bias = rnd(G * C, g=g).float()
    out_c, T_c = torch.zeros(M, G * C, dtype=BF), torch.zeros(M, G * Rp, dtype=BF)
    E.gemm(X, W, out_c, lora=(Ad, Bu, 0.7, T_c), bias=bias, lora_group_n=C)
    out_g, T_g = torch.zeros(M, G * C, dtype=BF, device="cuda"), torch.zeros(M, G * Rp, dtype=BF, device="cuda")
    ops.gemm(X.cuda(), W.cuda(), out_g, lora=(Ad.cuda(), Bu.cuda(), 0.7, T_g), bias=bias.cuda(), lora_group_n=C, tile=tile, splitk=splitk)
    close(T_g, T_c, tol=1.5e-2, what="grouped lora T_out")
    close(out_g, out_c, tol=1.5e-2, what="grouped lora out")


@pytest.mark.parametrize("splitk", [0, 1])
@pytest.mark.parametrize("M,N,C,G,tile,Rp", [(200, 128, 128, 3, 0, 16), (1024, 256, 192, 2, 1, 16), (130, 64, 64, 4, 3, 16), (520, 320, 128, 3, 2, 16),
                                             (1024, 1280, 1280, 3, 0, 32), (200, 128, 128, 3, 2, 32), (520, 320, 128, 4, 1, 32), (130, 64, 64, 2, 3, 64),
                                             (1024, 256, 192, 3, 1, 64), (128, 2048, 1280, 2, 0, 64)])
def test_gemm_kgrouped_lora(ops, M, N, C, G, tile, splitk, Rp):
    """dX of stacked projections: K = G*C stacked gradients, one adapter (padded rank 16 / 32 / 64) per K group (+ residual)."""
    g = torch.Generator().manual_seed(M + N + G)
    K = G * C
    X, W = rnd(M, K, g=g), rnd(N, K, g=g, scale=0.2)
    Ad, Bu = rnd(Rp, K, g=g, scale=0.3), rnd(N, G * Rp, g=g, scale=0.3)
    res = rnd(M, N, g=g)
    out_c, T_c = torch.zeros(M, N, dtype=BF), torch.zeros(M, G * Rp, dtype=BF)
    E.gemm(X, W, out_c, lora=(Ad, Bu, 0.7, T_c), residual=res, lora_group_k=C)
    out_g, T_g = torch.zeros(M, N, dtype=BF, device="cuda"), torch.zeros(M, G * Rp, dtype=BF, device="cuda")
    ops.gemm(X.cuda(), W.cuda(), out_g, lora=(Ad.cuda(), Bu.cuda(), 0.7, T_g), residual=res.cuda(), lora_group_k=C, tile=tile, splitk=splitk)
    close(T_g, T_c, tol=1.5e-2, what="k-grouped lora T_out")
    close(out_g, out_c, tol=1.5e-2, what="k-grouped lora out")


@pytest.mark.parametrize("Rp", [16, 32, 64])
@pytest.mark.parametrize("mode", ["ngroup", "kgroup"])
def test_gemm_batched(ops, mode, Rp):
    """One launch, several problems of identical shape (the to_k|to_v projections of all cross-attention layers), any adapter rank pad."""
    g = torch.Generator().manual_seed(77)
    nb, M, C, Kc = 5, 128, 128, 256
    if mode == "ngroup":      # forward: shared X, per-problem stacked W [2C, K] with one adapter per C columns
        N, K, kw = 2 * C, Kc, dict(lora_group_n=C)
        mk = lambda: dict(W=rnd(N, K, g=g, scale=0.2), Adown=rnd(2 * Rp, K, g=g, scale=0.3), Bup=rnd(N, Rp, g=g, scale=0.3),
                          T_out=torch.zeros(M, 2 * Rp, dtype=BF), C=torch.zeros(M, N, dtype=BF), Ct=torch.zeros(N, M, dtype=BF))
        X = rnd(M, K, g=g)
    else:                     # backward: per-problem X = stacked gradients [M, 2C], W^T [N, 2C], one adapter per K group
        N, K, kw = Kc, 2 * C, dict(lora_group_k=C)
        mk = lambda: dict(X=rnd(M, K, g=g), W=rnd(N, K, g=g, scale=0.2), Adown=rnd(Rp, K, g=g, scale=0.3), Bup=rnd(N, 2 * Rp, g=g, scale=0.3),
                          T_out=torch.zeros(M, 2 * Rp, dtype=BF), C=torch.zeros(M, N, dtype=BF))
        X = None
    items_c = [mk() for _ in range(nb)]
    items_g = [{k: v.cuda() for k, v in it.items()} for it in items_c]
    def run(mod, items, Xs):
        it0 = items[0]
        x0 = Xs if Xs is not None else it0["X"]
        mod.gemm(x0, it0["W"], it0["C"], lora=(it0["Adown"], it0["Bup"], 0.5, it0["T_out"]), Ct=it0.get("Ct"),
                 batch=mod.GemmBatch(items, x0.device), **kw)
    run(E, items_c, X)
    run(ops, items_g, X.cuda() if X is not None else None)
    for ic, ig in zip(items_c, items_g):
        close(ig["C"], ic["C"], tol=1.5e-2, what=f"batched {mode} C")
        close(ig["T_out"], ic["T_out"], tol=1.5e-2, what=f"batched {mode} T")
        if "Ct" in ic:
            close(ig["Ct"], ic["Ct"], tol=1.5e-2, what="batched Ct")


@pytest.mark.parametrize("Rp,specs,expect_mfma", [
    (64, [(520, 320, 64, True, None), (96, 64, 40, False, None), (2 * 8 * 8, 9 * 64, 64, True, (2, 8, 8, 64))], 1),
    (32, [(333, 128, 24, True, None)], 1),
    (16, [(100, 36, 16, True, None), (2 * 4 * 4, 9 * 32, 8, False, (2, 4, 4, 32))], 0),      # odd shapes -> VALU kernel
])
def test_lora_grad_grouped_ranks_and_fallback(ops, Rp, specs, expect_mfma):
    g = torch.Generator().manual_seed(5 + Rp)
    probs_cpu, probs_gpu = [], []
    for (M, Cw, R, rank_major, conv) in specs:
        Q = rnd(M, Rp, g=g)
        if conv is None:
            P, cg_c, cg_g = rnd(M, Cw, g=g), None, None
        else:
            B, H, W, Cin = conv
            P = rnd(B * H * W, Cin, g=g)
            cg_c, cg_g = E.ConvGeom(B, H, W, Cin, H, W), ops.ConvGeom(B, H, W, Cin, H, W)
        probs_cpu.append(dict(P=P, Q=Q, out=torch.zeros(Cw * R, dtype=F32), M=M, Cw=Cw, R=R, rank_major=rank_major, conv=cg_c))
        probs_gpu.append(dict(P=P.cuda(), Q=Q.cuda(), out=torch.full((Cw * R,), 3.0, dtype=F32, device="cuda"), M=M, Cw=Cw, R=R,
                              rank_major=rank_major, conv=cg_g))
    E.LoraGradPlan(probs_cpu, Rp, "cpu").run()
    plan = ops.LoraGradPlan(probs_gpu, Rp, torch.device("cuda"))
    assert plan.mfma == expect_mfma
    plan.run()
    for pc, pg in zip(probs_cpu, probs_gpu):
        close(pg["out"], pc["out"], tol=2e-3, what=f"lora grad Rp={Rp} M={pc['M']} Cw={pc['Cw']}")


# --------------------------------------------------------------------------------------------- attention
ATTN_CASES = [
    dict(B=2, H=2, Nq=256, Nk=256, Nkp=256, d=64, causal=False, qsplit=1),
    dict(B=1, H=10, Nq=1024, Nk=77, Nkp=80, d=64, causal=False, qsplit=4),
    dict(B=2, H=3, Nq=192, Nk=77, Nkp=80, d=64, causal=False, qsplit=1),
    dict(B=2, H=3, Nq=200, Nk=77, Nkp=128, d=80, causal=False, qsplit=3),
    dict(B=1, H=2, Nq=64, Nk=40, Nkp=40, d=40, causal=False, qsplit=2),
    dict(B=2, H=4, Nq=320, Nk=77, Nkp=128, d=64, causal=False, qsplit=3, accumulate=True),
    dict(B=1, H=8, Nq=256, Nk=256, Nkp=256, d=40, causal=False, qsplit=1),
    dict(B=1, H=2, Nq=128, Nk=128, Nkp=128, d=160, causal=False, qsplit=1),
    dict(B=1, H=4, Nq=128, Nk=128, Nkp=128, d=80, causal=False, qsplit=1),
    dict(B=2, H=2, Nq=77, Nk=77, Nkp=80, d=64, causal=True, qsplit=1),
    # whole 64-row tiles at head width 64: the 32-rows-per-wave kernels (attn32.hip) - odd tile counts per wave group, one tile, more keys than queries
    dict(B=1, H=3, Nq=128, Nk=320, Nkp=320, d=64, causal=False, qsplit=1),
    dict(B=1, H=2, Nq=192, Nk=64, Nkp=64, d=64, causal=False, qsplit=1),
    dict(B=2, H=1, Nq=576, Nk=576, Nkp=576, d=64, causal=False, qsplit=1),
    dict(B=1, H=20, Nq=1024, Nk=1024, Nkp=1024, d=64, causal=False, qsplit=1),
    dict(B=1, H=10, Nq=4096, Nk=4096, Nkp=4096, d=64, causal=False, qsplit=1),      # the 64 x 64 level of SDXL at 1024 px (attn32: 4096 tokens x 10 heads)
    # SD1.5's 160-wide cross-attention heads with a query split: the generic dQ + dK / dV launches, partial dK / dV in per-split slabs (ordered sum; float atomics until round 5)
    dict(B=2, H=2, Nq=320, Nk=77, Nkp=128, d=160, causal=False, qsplit=4),
    # SD1.5's 40-wide heads on a grid large enough for the separate dQ and dK / dV launches (> 2048 workgroups): three 16-column output blocks (DV = 48) in 64-column tiles
    dict(B=5, H=8, Nq=2048, Nk=2048, Nkp=2048, d=40, causal=False, qsplit=1),
]


@pytest.mark.parametrize("c", ATTN_CASES)
def test_attention_fwd_bwd(ops, c):
    g = torch.Generator().manual_seed(c["Nq"] + c["d"])
    B, H, Nq, Nk, Nkp, d = c["B"], c["H"], c["Nq"], c["Nk"], c["Nkp"], c["d"]
    Nqp = (Nq + 7) // 8 * 8
    C = H * d
    scale = 1 / math.sqrt(d)
    Q, dO = rnd(B * Nqp, C, g=g), rnd(B * Nqp, C, g=g)
    K, V = rnd(B * Nkp, C, g=g), rnd(B * Nkp, C, g=g)
    if Nkp > Nk:
        K.view(B, Nkp, C)[:, Nk:] = 0
        V.view(B, Nkp, C)[:, Nk:] = 0
    kw = dict(B=B, H=H, Nq=Nq, Nk=Nk, Nqp=Nqp, Nkp=Nkp, d=d, scale=scale, causal=c["causal"])
    O_ref, L_ref = torch.zeros(B * Nqp, C, dtype=BF), torch.zeros(B * H * Nq)
    E.attn_fwd(Q, K, V, V.t().contiguous(), O_ref, L_ref, **kw)
    dQr, dKr, dVr = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    acc = dict(accumulate_dq=True, accumulate_dk=True) if c.get("accumulate") else {}
    if acc:   # the buffers already hold a gradient (the score side output's): the kernel adds to dQ and dK, overwrites dV
        dQr, dKr = rnd(*Q.shape, g=g).clone(), rnd(*K.shape, g=g).clone()
        dQ0, dK0 = dQr.clone(), dKr.clone()
    E.attn_bwd(Q, K, V, K.t().contiguous(), Q.t().contiguous(), O_ref, L_ref, dO, dO.t().contiguous(), None, dQr, dKr, dVr, **kw, **acc)

    Qd, Kd, Vd, dOd = dev(Q, K, V, dO)
    Kt, Vt, Qt, dOt = Kd.t().contiguous(), Vd.t().contiguous(), Qd.t().contiguous(), dOd.t().contiguous()
    O = torch.zeros(B * Nqp, C, dtype=BF, device="cuda")
    L = torch.zeros(B * H * Nq, device="cuda")
    ops.attn_fwd(Qd, Kd, Vd, Vt, O, L, **kw)
    vq = torch.zeros(B, Nqp, 1, dtype=torch.bool)
    vq[:, :Nq] = True
    vq = vq.reshape(B * Nqp, 1)
    close(O.cpu() * vq, O_ref * vq, what=f"attn fwd {c}")
    close(L, L_ref, tol=2e-3, what="attn lse")
    dQ, dK, dV = (torch.full_like(t, 5.0) for t in (Qd, Kd, Vd))
    if acc:
        dQ, dK = dQ0.cuda(), dK0.cuda()
    D = torch.zeros(B * H * Nq, device="cuda")
    extra = {}
    if c["qsplit"] > 1:
        ns = c["qsplit"]   # the single-pass cross-attention kernel wants one partial slab per query split
        extra = dict(qsplit=ns, dK32=torch.full((ns * B * Nkp, C), float("nan"), device="cuda"), dV32=torch.full((ns * B * Nkp, C), float("nan"), device="cuda"))
    ops.attn_bwd(Qd, Kd, Vd, Kt, Qt, O, L, dOd, dOt, D, dQ, dK, dV, **kw, **extra, **acc)
    close(dQ.cpu() * vq, dQr * vq, tol=2.5e-2, what=f"attn dQ {c}")
    close(dK, dKr, tol=2.5e-2, what=f"attn dK {c}")
    close(dV, dVr, tol=2.5e-2, what=f"attn dV {c}")
    if c["qsplit"] == 1 and not acc and not c["causal"] and Nq == Nqp:
        # d_ready: the row term D = rowsum(dO o O) comes from outside (sdlt_wsk_gemm_rowdot leaves it while it produces dO) - with the pre-pass's own D handed back in,
        # skipping the pre-pass launch must not change a bit; and a forward that is given D clears it (the slots the side output accumulates into)
        D2 = D.clone()
        D.fill_(float("nan"))
        dQ2, dK2, dV2 = (torch.full_like(t, 3.0) for t in (Qd, Kd, Vd))
        ops.attn_bwd(Qd, Kd, Vd, Kt, Qt, O, L, dOd, dOt, D2, dQ2, dK2, dV2, **kw, d_ready=True)
        assert torch.equal(dQ2, dQ) and torch.equal(dK2, dK) and torch.equal(dV2, dV)
        want = (dOd.float() * O.float()).reshape(B, Nq, H, d).sum(-1).permute(0, 2, 1).reshape(-1)
        torch.testing.assert_close(D2, want, rtol=1e-4, atol=1e-5 * float(want.abs().max()))
        O3, L3 = torch.zeros_like(O), torch.zeros_like(L)
        ops.attn_fwd(Qd, Kd, Vd, Vt, O3, L3, **kw, zero_D=D)
        assert torch.equal(O3, O) and torch.equal(L3, L) and float(D.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- norms / element-wise
@pytest.mark.parametrize("B,HW,C1,C2,silu", [(2, 256, 320, 0, True), (1, 1024, 640, 320, True), (2, 64, 128, 64, False),
                                             (1, 4096, 64, 0, True), (1, 100, 1920, 640, True)])
def test_groupnorm_fwd_bwd(ops, B, HW, C1, C2, silu):
    g = torch.Generator().manual_seed(C1 + HW)
    C = C1 + C2
    x1 = rnd(B * HW, C1, g=g) + 0.5
    x2 = rnd(B * HW, C2, g=g, scale=2.0) if C2 else None
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy, dres = rnd(B * HW, C, g=g), rnd(B * HW, C, g=g)
    kw = dict(B=B, HW=HW, eps=1e-5, silu=silu)
    yr = E.groupnorm_fwd(x1, x2, torch.empty(B * HW, C, dtype=BF), None, gamma=gamma, beta=beta, **kw)
    dxr = E.groupnorm_bwd(x1, x2, dy, torch.empty(B * HW, C, dtype=BF), None, None, gamma=gamma, beta=beta, dres=dres, **kw)
    x1d, x2d, gd, bd, dyd, drd = dev(x1, x2, gamma, beta, dy, dres)
    stats, bstats = torch.zeros(B * 64, device="cuda"), torch.zeros(B * 64, device="cuda")
    y = ops.groupnorm_fwd(x1d, x2d, torch.empty(B * HW, C, dtype=BF, device="cuda"), stats, gamma=gd, beta=bd, **kw)
    close(y, yr, what="groupnorm fwd")
    dx = ops.groupnorm_bwd(x1d, x2d, dyd, torch.empty(B * HW, C, dtype=BF, device="cuda"), stats, bstats, gamma=gd, beta=bd, dres=drd, **kw)
    close(dx, dxr, tol=2e-2, what="groupnorm bwd")
    # the statistics are reduced in a fixed order (two-stage, no float atomics): repeated launches - onto dirty output buffers,
    # the scratch counters re-armed by the kernel - are bitwise identical
    for rep in range(3):
        st2, bst2 = torch.full((B * 64,), 7.0 + rep, device="cuda"), torch.full((B * 64,), -3.0, device="cuda")
        y2 = ops.groupnorm_fwd(x1d, x2d, torch.empty(B * HW, C, dtype=BF, device="cuda"), st2, gamma=gd, beta=bd, **kw)
        dx2 = ops.groupnorm_bwd(x1d, x2d, dyd, torch.empty(B * HW, C, dtype=BF, device="cuda"), st2, bst2, gamma=gd, beta=bd, dres=drd, **kw)
        assert torch.equal(st2, stats) and torch.equal(bst2, bstats) and torch.equal(y2, y) and torch.equal(dx2, dx), f"GroupNorm not reproducible (rep {rep})"
    # side output: per-image column sums of the STORED gradient (the time-embedding projection's gradient in a ResnetBlock2D), finished for several norms in one
    # launch; equal to sdlt_colsum over dx up to the order of the fp32 additions, bitwise reproducible, dx itself unchanged
    ns = ops.groupnorm_colsum_splits(B, HW, C)
    ws = torch.full((ns * B * C,), float("nan"), device="cuda")
    dx3 = ops.groupnorm_bwd(x1d, x2d, dyd, torch.empty(B * HW, C, dtype=BF, device="cuda"), stats, bstats, gamma=gd, beta=bd, dres=drd, colsum_ws=ws, **kw)
    assert torch.equal(dx3, dx)
    out16, out32 = torch.zeros(B * C, dtype=BF, device="cuda"), torch.zeros(B * C, device="cuda")
    ops.ColsumFinishPlan([(ws, ns, out16), (ws, ns, out32)], torch.device("cuda")).run()
    want = dx.float().reshape(B, HW, C).sum(1).reshape(-1)
    torch.testing.assert_close(out32, want, rtol=1e-5, atol=1e-4 * float(want.abs().max()))
    assert torch.equal(out16, out32.to(BF))
    two = ops.colsum(dx, torch.zeros(B, C, device="cuda"), B=B, R=HW).reshape(-1)
    torch.testing.assert_close(out32, two, rtol=1e-5, atol=1e-4 * float(want.abs().max()))
    ws2 = torch.zeros_like(ws)
    ops.groupnorm_bwd(x1d, x2d, dyd, torch.empty(B * HW, C, dtype=BF, device="cuda"), stats, bstats, gamma=gd, beta=bd, dres=drd, colsum_ws=ws2, **kw)
    assert torch.equal(ws2, ws)


@pytest.mark.parametrize("M,C", [(77, 768), (1000, 320), (256, 1280), (64, 2048)])
def test_layernorm_fwd_bwd(ops, M, C):
    g = torch.Generator().manual_seed(M + C)
    x = rnd(M, C, g=g) + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy, dres = rnd(M, C, g=g), rnd(M, C, g=g)
    yr = E.layernorm_fwd(x, torch.empty(M, C, dtype=BF), None, gamma=gamma, beta=beta)
    dxr = E.layernorm_bwd(x, dy, torch.empty(M, C, dtype=BF), None, gamma=gamma, dres=dres)
    xd, gd, bd, dyd, drd = dev(x, gamma, beta, dy, dres)
    stats = torch.zeros(M * 2, device="cuda")
    close(ops.layernorm_fwd(xd, torch.empty(M, C, dtype=BF, device="cuda"), stats, gamma=gd, beta=bd), yr, what="ln fwd")
    close(ops.layernorm_bwd(xd, dyd, torch.empty(M, C, dtype=BF, device="cuda"), stats, gamma=gd, dres=drd), dxr, tol=2e-2, what="ln bwd")


def test_elementwise_family(ops):
    g = torch.Generator().manual_seed(77)
    M, Ch = 300, 640
    inp, dout = rnd(M, 2 * Ch, g=g), rnd(M, Ch, g=g)
    close(ops.geglu_fwd(inp.cuda(), torch.empty(M, Ch, dtype=BF, device="cuda")), E.geglu_fwd(inp, torch.empty(M, Ch, dtype=BF)), what="geglu fwd")
    close(ops.geglu_bwd(inp.cuda(), dout.cuda(), torch.empty(M, 2 * Ch, dtype=BF, device="cuda")),
          E.geglu_bwd(inp, dout, torch.empty(M, 2 * Ch, dtype=BF)), what="geglu bwd")
    x, dy = rnd(64, 1280, g=g, scale=2.0), rnd(64, 1280, g=g)
    for op in range(7):
        need_dy = op in (E.MAP_DSILU, E.MAP_ADD, E.MAP_DGELU, E.MAP_DQGELU)
        ref = E.map_bf16(op, x, dy if need_dy else None, torch.empty_like(x))
        got = ops.map_bf16(op, x.cuda(), dy.cuda() if need_dy else None, torch.empty_like(x).cuda())
        close(got, ref, what=f"map op {op}")
    t = torch.tensor([0.0, 10.0, 999.0, 1024.0])
    close(ops.timestep_embedding(t.cuda(), torch.empty(4, 320, dtype=BF, device="cuda")), E.timestep_embedding(t, torch.empty(4, 320, dtype=BF)),
          tol=1e-2, what="timestep embedding")
    a, b = rnd(200, 128, g=g), rnd(200, 192, g=g)
    close(ops.add2d(a.cuda(), b.cuda()[:, 64:], torch.empty(200, 128, dtype=BF, device="cuda")), E.add2d(a, b[:, 64:], torch.empty(200, 128, dtype=BF)), what="add2d")
    up = rnd(2 * 16 * 16, 64, g=g)
    close(ops.sum2x2(up.cuda(), torch.empty(2 * 8 * 8, 64, dtype=BF, device="cuda"), B=2, H=8, W=8), E.sum2x2(up, torch.empty(128, 64, dtype=BF), B=2, H=8, W=8), what="sum2x2")
    xs = rnd(3 * 100, 128, g=g)
    close(ops.colsum(xs.cuda(), torch.empty(3, 128, device="cuda"), B=3, R=100), E.colsum(xs, torch.empty(3, 128), B=3, R=100), tol=2e-3, what="colsum")


@pytest.mark.parametrize("B,gamma,vpred", [(1, 5.0, False), (4, 5.0, False), (3, 0.0, False), (2, 5.0, True)])
def test_add_noise_and_masked_mse(ops, B, gamma, vpred):
    g = torch.Generator().manual_seed(B)
    h = 16
    from oracle import loss_ref as L
    acp = L.ddpm_alphas_cumprod()
    x0, noise = torch.randn(B, 4, h, h, generator=g) * 0.13, torch.randn(B, 4, h, h, generator=g)
    mask = (torch.rand(B, 1, h, h, generator=g) * 0.95 + 0.05).repeat(1, 4, 1, 1).contiguous()
    t = torch.tensor([10, 900, 0, 999][:B])
    noisy_ref = L.add_noise(acp, x0, noise, t)
    out = torch.empty(B * h * h, 64, dtype=BF, device="cuda")
    noisy = torch.empty(B, 4, h, h, device="cuda")
    ops.add_noise_nhwc(x0.cuda(), noise.cuda(), t.cuda(), acp.cuda(), out, noisy)
    close(noisy, noisy_ref, tol=1e-5, what="add_noise nchw")
    close(out[:, :4], noisy_ref.permute(0, 2, 3, 1).reshape(-1, 4), tol=1e-2, what="add_noise nhwc")
    assert float(out[:, 4:].abs().max()) == 0.0
    pred = torch.randn(B * h * h, 4, generator=g)
    loss_ref = L.diffusion_loss(pred.reshape(B, h, h, 4).permute(0, 3, 1, 2), noise, noisy_ref, mask, acp, t, snr_gamma=gamma,
                                prediction_type="v_prediction" if vpred else "epsilon")
    lo_e, dp_e = torch.zeros(1), torch.zeros(B * h * h, 64, dtype=BF)
    E.masked_mse_fwd_bwd(pred, noise, noisy_ref, mask, t, acp, None, lo_e, dp_e, snr_gamma=gamma, v_prediction=vpred)
    sums, lo, dp = torch.full((2 * B * 65,), 9.0, device="cuda"), torch.zeros(1, device="cuda"), torch.empty(B * h * h, 64, dtype=BF, device="cuda")   # finals + partial slices, any contents
    ops.masked_mse_fwd_bwd(pred.cuda(), noise.cuda(), noisy, mask.cuda(), t.cuda(), acp.cuda(), sums, lo, dp, snr_gamma=gamma, v_prediction=vpred)
    close(lo, loss_ref.reshape(1), tol=1e-5, what="masked mse loss vs oracle")
    close(dp, dp_e, tol=1e-2, what="masked mse grad")


@pytest.mark.parametrize("n,wd,growth,l1", [(100_003, 0.004, 1.05, 0.03), (3 * 2048, 0.0, float("inf"), 0.0), (3_000_001, 0.004, 1.02, 0.0)])
def test_prodigy_step_vs_oracle(ops, n, wd, growth, l1):
    """sdlt_prodigy_step (four launches, scalars on the device) against oracle/prodigy_ref.py as the reference builds it
    (optimizer.py:24-34: betas (0.9, 0.99), bias correction, safeguard warm-up, decoupled decay), 10 steps with a
    consistent gradient field so that d really adapts, one lr == 0 step in the middle (must be a no-op)."""
    import math
    from oracle import prodigy_ref as P
    g = torch.Generator().manual_seed(11)
    p_init = torch.randn(n, generator=g) * 0.1
    target = torch.randn(n, generator=g) * 0.1
    opt = P.Prodigy([p_init.clone()], lr=1.0, betas=(0.9, 0.99), decouple=True, use_bias_correction=True, safeguard_warmup=True,
                    weight_decay=wd, growth_rate=growth, d_coef=1.0)
    pd, p0d, md, vd, sd = dev(p_init.clone(), p_init.clone(), torch.zeros(n), torch.zeros(n), torch.zeros(n))
    state = torch.zeros(16)
    state[:3] = 1e-6
    state, acc, l1s = state.cuda(), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
    for i in range(10):
        lr = 0.0 if i == 5 else 1.0
        gr = (opt.params[0] - target) + 0.05 * torch.randn(n, generator=g)
        opt.param_groups[0]["lr"] = lr
        before = pd.clone()
        opt.step([gr + l1 / n * torch.sign(opt.params[0])])
        hyper = torch.tensor([lr, 0.9, 0.99, math.sqrt(0.99), 1e-8, wd, 1.0, growth, l1 / n, 1.0, 1.0, 1.0, 1.0, 0, 0, 0])
        ops.prodigy_step(pd, gr.cuda(), p0d, md, vd, sd, hyper.cuda(), state, acc, l1s)
        if i == 5:
            assert torch.equal(pd, before) and float(state[8]) == 0.0
    st = state.tolist()
    grp = opt.param_groups[0]
    assert grp["d"] > 1.1e-6, "the test field must make d grow"
    assert abs(st[0] - grp["d"]) <= 1e-3 * grp["d"], (st[0], grp["d"])
    assert int(st[6]) == grp["k"] == 9
    assert abs(st[3] - grp["d_numerator"]) <= 1e-3 * abs(grp["d_numerator"])
    d = (pd.cpu() - opt.params[0]).abs().max()
    moved = (opt.params[0] - p_init).abs().max()
    ulp = float(opt.params[0].abs().max()) * 2.0 ** -23        # the parameters only move ~1e-5 in 10 steps from d0 = 1e-6
    assert float(d) <= 2e-3 * float(moved) + 2 * ulp, (float(d), float(moved))
    close(l1s, opt.params[0].abs().sum().reshape(1), tol=2e-2, what="l1 sum")


def test_adamw_and_shadows(ops):
    g = torch.Generator().manual_seed(9)
    n = 100_003
    p, gr = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.01
    m, v = torch.zeros(n), torch.zeros(n)
    pd, gd, md, vd = dev(p.clone(), gr, m.clone(), v.clone())
    l1 = torch.zeros(1, device="cuda")
    hyper = torch.zeros(16)
    for step in (1, 2, 3):
        hyper[:9] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.004, 1 - 0.9 ** step, 1 - 0.999 ** step, 0.03 / n, 1.0])
        E.adamw_fused(p, gr, m, v, hyper)
        ops.adamw_fused(pd, gd, md, vd, hyper.cuda(), l1)
    close(pd, p, tol=1e-5, what="adamw params")
    close(vd, v, tol=1e-5, what="adamw v")
    close(l1, p.abs().sum().reshape(1), tol=2e-2, what="l1 sum (of pre-step params)")
    arena = torch.randn(8000, generator=g)
    ent_c, ent_g = [], []
    specs = [(0, 4, 300, 300), (1200, 70, 4, 4), (1480 + 3 * 64, 8, 64, 9 * 64)]
    ad = arena.cuda()
    for (off, rows, cols, sld) in specs:
        dc, dtc = torch.zeros(max(rows, 16), cols, dtype=BF), torch.zeros(cols, 128, dtype=BF)
        ent_c.append((off, rows, cols, sld, dc, dtc[:, :96]))
        dg, dtg = dc.cuda(), dtc.cuda()
        ent_g.append((off, rows, cols, sld, dg, dtg[:, :96]))
    E.ShadowPlan(ent_c, "cpu").run(arena)
    ops.ShadowPlan(ent_g, torch.device("cuda")).run(ad)
    for c_, g_ in zip(ent_c, ent_g):
        assert torch.equal(g_[4].cpu(), c_[4]) and torch.equal(g_[5].cpu(), c_[5])


def test_ti_kernels_and_gemm_accumulate(ops):
    g = torch.Generator().manual_seed(31)
    B, T, Tp, D, V, n = 2, 77, 128, 768, 500, 3
    table, pos = rnd(V, D, g=g), rnd(T, D, g=g, scale=0.1)
    ids = torch.randint(0, V - n, (B, T), generator=g)
    ids[0, 3:6] = torch.tensor([V - 3, V - 2, V - 1])
    ids[1, 9] = V - 2
    ref = E.embed_gather(table, ids, pos, torch.empty(B * Tp, D, dtype=BF), B=B, T=T, Tp=Tp)
    got = ops.embed_gather(table.cuda(), ids.cuda(), pos.cuda(), torch.full((B * Tp, D), 9.0, dtype=BF, device="cuda"), B=B, T=T, Tp=Tp)
    close(got, ref, what="embed_gather")
    dx = rnd(B * Tp, D, g=g)
    train = torch.arange(V - n, V)
    gref = E.embed_grad(dx, ids, train, torch.zeros(n, D), B=B, T=T, Tp=Tp)
    ggot = ops.embed_grad(dx.cuda(), ids.cuda(), train.cuda(), torch.full((n, D), 5.0, device="cuda"), B=B, T=T, Tp=Tp)
    close(ggot, gref, tol=1e-5, what="embed_grad")
    rows = torch.randn(n, D, generator=g) * 0.02
    gr_c, lo_c = torch.zeros(n, D), torch.zeros(1)
    E.ti_std_reg(rows, gr_c, lo_c, target_mean=0.015, target_var=3e-4, weight=0.005)
    gr_g, lo_g = torch.zeros(n, D, device="cuda"), torch.zeros(1, device="cuda")
    ops.ti_std_reg(rows.cuda(), gr_g, lo_g, target_mean=0.015, target_var=3e-4, weight=0.005)
    close(gr_g, gr_c, tol=1e-4, what="ti_std_reg grad")
    close(lo_g, lo_c, tol=1e-4, what="ti_std_reg loss")
    # fp32 accumulate epilogue (DAAM score sums) and N = 128 padded text axis
    X, W = rnd(300, 128, g=g), rnd(128, 128, g=g, scale=0.1)
    acc_c, acc_g = torch.zeros(300, 128), torch.zeros(300, 128, device="cuda")
    for i in range(3):
        E.gemm(X, W, acc_c, alpha=0.125, accumulate=i > 0)
        ops.gemm(X.cuda(), W.cuda(), acc_g, alpha=0.125, accumulate=i > 0)
    close(acc_g, acc_c, tol=2e-3, what="gemm fp32 accumulate")
    xs = rnd(2 * 100, 128, g=g)
    close(ops.colsum(xs.cuda(), torch.empty(2, 128, dtype=BF, device="cuda"), B=2, R=100), E.colsum(xs, torch.empty(2, 128, dtype=BF), B=2, R=100), what="colsum bf16")


# ------------------------------------------------------------------------------------------------ full fine-tune support
@pytest.mark.parametrize("M,C", [(4096, 320), (77, 64), (130, 8), (2, 1280)])
def test_wgrad_transpose(ops, M, C):
    g = torch.Generator().manual_seed(0)
    Mp = (M + 63) // 64 * 64
    big = torch.randn(M, C + 8, generator=g).to(BF)
    x = big[:, :C]                                                   # strided source rows
    ref = E.wgrad_transpose(x, torch.zeros(C, Mp, dtype=BF))
    out = torch.full((C, Mp), 7.0, dtype=BF, device="cuda")
    acc = torch.full((C,), 0.5, device="cuda")                          # accumulated into (the trainer zeroes the region once per step)
    ops.wgrad_transpose(big.cuda()[:, :C], out, colsum_acc=acc)
    assert torch.equal(out.cpu(), ref)
    close(acc, 0.5 + x.float().sum(0), tol=2e-3, what="column sums (bias gradient) from the transposing pass")


@pytest.mark.parametrize("B,H,W,C,stride,ups", [(2, 16, 16, 64, 1, 1), (1, 8, 12, 320, 1, 1), (2, 16, 16, 128, 2, 1), (1, 8, 8, 64, 1, 2), (3, 5, 7, 8, 1, 1)])
def test_wgrad_im2col_t(ops, B, H, W, C, stride, ups):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * H * W, C, generator=g).to(BF)
    M = B * (H * ups // stride) * (W * ups // stride)
    Mp = (M + 63) // 64 * 64
    ref = E.wgrad_im2col_t(x, torch.zeros(9 * C, Mp, dtype=BF), B=B, H=H, W=W, stride=stride, ups=ups)
    out = torch.full((9 * C, Mp), 7.0, dtype=BF, device="cuda")
    ops.wgrad_im2col_t(x.cuda(), out, B=B, H=H, W=W, stride=stride, ups=ups)
    assert torch.equal(out.cpu(), ref)


def test_weight_gradient_gemm(ops):
    """dW = dY^T X through the transposed panels + sdlt_gemm_bf16 (fp32 output), linear and 3x3 conv (vs autograd)."""
    g = torch.Generator().manual_seed(2)
    M, N, K = 1000, 192, 320
    x, dy = torch.randn(M, K, generator=g).to(BF), torch.randn(M, N, generator=g).to(BF)
    Mp = 1024
    xT, dyT = torch.empty(K, Mp, dtype=BF, device="cuda"), torch.empty(N, Mp, dtype=BF, device="cuda")
    ops.wgrad_transpose(x.cuda(), xT)
    ops.wgrad_transpose(dy.cuda(), dyT)
    dW = torch.zeros(N, K, device="cuda")
    ops.gemm(dyT, xT, dW)
    close(dW, dy.float().t() @ x.float(), tol=2e-3, what="linear dW")
    B, H, W, Cin, Cout = 2, 16, 16, 64, 128
    xi = torch.randn(B * H * W, Cin, generator=g).to(BF)
    dyo = torch.randn(B * H * W, Cout, generator=g).to(BF)
    w = torch.zeros(Cout, Cin, 3, 3, requires_grad=True)
    y = torch.nn.functional.conv2d(xi.float().reshape(B, H, W, Cin).permute(0, 3, 1, 2), w, padding=1)
    (gw,) = torch.autograd.grad(y, w, dyo.float().reshape(B, H, W, Cout).permute(0, 3, 1, 2))
    cols, dyT = torch.empty(9 * Cin, B * H * W, dtype=BF, device="cuda"), torch.empty(Cout, B * H * W, dtype=BF, device="cuda")
    ops.wgrad_im2col_t(xi.cuda(), cols, B=B, H=H, W=W)
    ops.wgrad_transpose(dyo.cuda(), dyT)
    dWc = torch.zeros(Cout, 9 * Cin, device="cuda")
    ops.gemm(dyT, cols, dWc)
    close(dWc, gw.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), tol=2e-3, what="conv dW (tap-major)")


@pytest.mark.parametrize("two,silu", [(False, True), (True, True), (False, False)])
def test_norm_affine_grads(ops, two, silu):
    g = torch.Generator().manual_seed(3)
    B, HW, C = 2, 96, 128
    x = (torch.randn(B * HW, C, generator=g) * 1.5 + 0.3).to(BF)
    dy = torch.randn(B * HW, C, generator=g).to(BF)
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    x1, x2 = (x[:, :48].contiguous(), x[:, 48:].contiguous()) if two else (x, None)
    dgr, dbr = torch.zeros(C), torch.zeros(C)
    E.groupnorm_affine_grad(x1, x2, dy, None, dgr, dbr, B=B, HW=HW, gamma=gamma, beta=beta, eps=1e-5, silu=silu)
    y, stats = torch.empty(B * HW, C, dtype=BF, device="cuda"), torch.zeros(B * 64, device="cuda")
    kw = dict(B=B, HW=HW, gamma=gamma.cuda(), beta=beta.cuda(), eps=1e-5, silu=silu)
    d1, d2 = x1.cuda(), (x2.cuda() if two else None)
    ops.groupnorm_fwd(d1, d2, y, stats, **kw)
    dg, db = torch.full((C,), 9.0, device="cuda"), torch.full((C,), 9.0, device="cuda")
    ops.groupnorm_affine_grad(d1, d2, dy.cuda(), stats, dg, db, **kw)
    close(dg, dgr, tol=5e-3, what="GN dgamma")
    close(db, dbr, tol=5e-3, what="GN dbeta")
    # LayerNorm
    M = 300
    xl, dyl = torch.randn(M, C, generator=g).to(BF), torch.randn(M, C, generator=g).to(BF)
    E.layernorm_affine_grad(xl, dyl, None, dgr, dbr)
    yl, st = torch.empty(M, C, dtype=BF, device="cuda"), torch.zeros(M * 2, device="cuda")
    ops.layernorm_fwd(xl.cuda(), yl, st, gamma=gamma.cuda(), beta=beta.cuda())
    ops.layernorm_affine_grad(xl.cuda(), dyl.cuda(), st, dg, db)
    close(dg, dgr, tol=5e-3, what="LN dgamma")
    close(db, dbr, tol=5e-3, what="LN dbeta")


def test_adamw_fused_into_refresh_tiles(ops):
    """sdlt_adamw_shadow_refresh: AdamW step + both bf16 copies per 64x64 tile (the full fine-tune's optimizer pass), incl. a
    conv-style tensor whose taps are separate descriptors over a strided master ([Cout, 9*Cin], per-tap [Cout, Cin] blocks)."""
    g = torch.Generator().manual_seed(12)
    specs = [(0, 200, 130, 130), (26000, 70, 192, 192)]                       # (offset, rows, cols, src_ld)
    cout, cin, base = 96, 40, 40000
    specs += [(base + tap * cin, cout, cin, 9 * cin) for tap in range(9)]
    n = base + cout * 9 * cin
    p = torch.randn(n, generator=g) * 0.1
    gr, m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
    hyper = torch.zeros(16)
    hyper[:9] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.004, 1 - 0.9 ** 3, 1 - 0.999 ** 3, 0.0, 0.5])
    ent_c, ent_g, outs = [], [], []
    for (off, rows, cols, sld) in specs:
        dc, dtc = torch.zeros(rows, cols + 8, dtype=BF), torch.zeros(cols, rows + 8, dtype=BF)
        dg, dtg = dc.cuda(), dtc.cuda()
        ent_c.append((off, rows, cols, sld, dc[:, :cols], dtc[:, :rows]))
        ent_g.append((off, rows, cols, sld, dg[:, :cols], dtg[:, :rows]))
        outs.append((dc, dtc, dg, dtg))
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    E.ShadowPlan(ent_c, "cpu").adamw(pc, gr, mc, vc, hyper)
    pd, gd, md, vd = dev(p.clone(), gr, m.clone(), v.clone())
    ops.ShadowPlan(ent_g, "cuda").adamw(pd, gd, md, vd, hyper.cuda())
    close(pd, pc, tol=1e-5, what="fused adamw params")
    close(md, mc, tol=1e-5, what="fused adamw m")
    close(vd, vc, tol=1e-5, what="fused adamw v")
    assert torch.equal(pd.cpu()[200 * 130:26000], p[200 * 130:26000])         # elements no descriptor covers are untouched
    for dc, dtc, dg, dtg in outs:
        close(dg, dc, tol=4e-3, what="refreshed operand")
        close(dtg, dtc, tol=4e-3, what="refreshed transposed operand")


def test_gemm_throughput_hint(ops):
    """sdlt_gemm_params.throughput_hint (several jobs share the device): the heuristics pick 256x128 tiles for the >= 320-tile
    classes and the mid-size convs - same results."""
    g = torch.Generator().manual_seed(21)
    ops.THROUGHPUT_HINT = True            # (set_throughput_hint only arms it with SDLT_THROUGHPUT_HINT=1 since round 4: measured slower; the kernels' rule is still checked)
    try:
        for (M, N, K, lora) in [(4096, 1920, 640, False), (4096, 1280, 640, True), (1024, 10240, 1280, False)]:
            X = torch.randn(M, K, generator=g).to(BF)
            W = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
            lo_c = lo_g = None
            if lora:
                A, Bm = (torch.randn(16, K, generator=g) / K ** 0.5).to(BF), (torch.randn(N, 16, generator=g) * 0.1).to(BF)
                lo_c, lo_g = (A, Bm, 0.5, torch.zeros(M, 16, dtype=BF)), (A.cuda(), Bm.cuda(), 0.5, torch.zeros(M, 16, dtype=BF, device="cuda"))
            ref = E.gemm(X, W, torch.zeros(M, N, dtype=BF), lora=lo_c)
            out = ops.gemm(X.cuda(), W.cuda(), torch.zeros(M, N, dtype=BF, device="cuda"), lora=lo_g)
            close(out, ref, what=f"hinted gemm {M}x{N}x{K} lora={lora}")
        Bc, H, Wd, Cin, Cout = 1, 64, 64, 128, 640                      # 4096 x 640 conv: the 160..319-tile conv class
        x = torch.randn(Bc * H * Wd, Cin, generator=g).to(BF)
        w = (torch.randn(Cout, 9 * Cin, generator=g) / (9 * Cin) ** 0.5).to(BF)
        geom = ops.ConvGeom(Bc, H, Wd, Cin, H, Wd)
        ref = E.gemm(x, w, torch.zeros(Bc * H * Wd, Cout, dtype=BF), conv=E.ConvGeom(Bc, H, Wd, Cin, H, Wd) if hasattr(E, "ConvGeom") else geom)
        out = ops.gemm(x.cuda(), w.cuda(), torch.zeros(Bc * H * Wd, Cout, dtype=BF, device="cuda"), conv=geom)
        close(out, ref, what="hinted conv")
    finally:
        ops.set_throughput_hint(False)


def test_splitk_workspace_per_owner(ops):
    """Concurrent jobs must not share split-K slabs / counters: inside `workspace_owner(key)` the workspace belongs to the key, not
    to the stream (torch captures different jobs' graphs on the same internal stream); a split-K GEMM is correct under either."""
    base = ops.splitk_workspace(torch.device("cuda:0"))
    with ops.workspace_owner("job-a"):
        wa = ops.splitk_workspace(torch.device("cuda:0"))
        with ops.workspace_owner("job-b"):
            wb = ops.splitk_workspace(torch.device("cuda:0"))
        assert ops.splitk_workspace(torch.device("cuda:0"))[0].data_ptr() == wa[0].data_ptr()
        g = torch.Generator().manual_seed(4)
        X, W = torch.randn(128, 2048, generator=g).to(BF), (torch.randn(256, 2048, generator=g) / 45).to(BF)
        out = ops.gemm(X.cuda(), W.cuda(), torch.zeros(128, 256, dtype=BF, device="cuda"), splitk=4)
        close(out, E.gemm(X, W, torch.zeros(128, 256, dtype=BF)), what="split-K GEMM under an owner workspace")
    assert len({base[0].data_ptr(), wa[0].data_ptr(), wb[0].data_ptr()}) == 3 and len({base[1].data_ptr(), wa[1].data_ptr(), wb[1].data_ptr()}) == 3
    assert ops.splitk_workspace(torch.device("cuda:0"))[0].data_ptr() == base[0].data_ptr()


# --------------------------------------------------------------------------------------------- DoRA
@pytest.mark.parametrize("M,N,K,r,tile,splitk,conv", [(1024, 1280, 1280, 16, 0, 0, False), (333, 200, 192, 4, 2, 0, False), (256, 256, 1280, 16, 1, 3, False),
                                                      (300, 256, 384, 64, 2, 0, False), (77, 640, 2048, 16, 3, 0, False), (512, 320, 64, 16, 0, 0, True)])
def test_gemm_col_scale(ops, M, N, K, r, tile, splitk, conv):
    """sdlt_gemm_params.col_scale: the product incl. the adapter term times a per-column factor, before bias and residual (DoRA)."""
    g = torch.Generator().manual_seed(M + N + r)
    Rp = 16 if r <= 16 else (32 if r <= 32 else 64)
    geom = None
    if conv:                                  # K = Cin here; the 3x3 operand is [N, 9*Cin]
        Bn, H, Wd_ = 2, 16, 16
        geom = E.ConvGeom(Bn, H, Wd_, K, H, Wd_) if hasattr(E, "ConvGeom") else None
        M, Kw = Bn * H * Wd_, 9 * K
    else:
        Kw = K
    X, W = rnd(M, K, g=g), rnd(N, Kw, g=g, scale=1 / math.sqrt(Kw))
    A = torch.zeros(Rp, Kw, dtype=BF)
    A[:r] = rnd(r, Kw, g=g, scale=1 / math.sqrt(Kw))
    Bu = torch.zeros(N, Rp, dtype=BF)
    Bu[:, :r] = rnd(N, r, g=g, scale=0.3)
    bias, cs = torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g)
    R = rnd(M, N, g=g)
    kw = dict(conv=geom) if conv else {}
    ref = E.gemm(X, W, torch.empty(M, N, dtype=BF), lora=(A, Bu, 0.75, None), bias=bias, residual=R, col_scale=cs, **kw)
    Xd, Wd, Ad, Bd, bd, csd, Rd = dev(X, W, A, Bu, bias, cs, R)
    if conv:
        kw = dict(conv=ops.ConvGeom(Bn, H, Wd_, K, H, Wd_))
    out = ops.gemm(Xd, Wd, torch.empty(M, N, dtype=BF, device="cuda"), lora=(Ad, Bd, 0.75, None), bias=bd, residual=Rd, col_scale=csd, tile=tile,
                   splitk=splitk, **kw)
    close(out, ref, what=f"col_scale gemm {M}x{N}x{Kw} r{r}")
    plain = E.gemm(X, W, torch.empty(M, N, dtype=BF), lora=(A, Bu, 0.75, None), bias=bias, residual=R, **(dict(conv=geom) if conv else {}))
    assert float((ref.float() - plain.float()).abs().max()) > 0.05


@pytest.mark.parametrize("r", [4, 16, 24, 64])
def test_dora_plan_kernels(ops, r):
    """sdlt_dora_refresh (row norms of W + s B A on the matrix cores, scale, scaled B^T), sdlt_dora_scale_wt (linear and 3x3-conv
    layouts) and sdlt_dora_mag_grad (magnitude gradient + dB row scaling) against the torch emulation, several layers per launch."""
    g = torch.Generator().manual_seed(r)
    Rp = 16 if r <= 16 else (32 if r <= 32 else 64)
    s = 0.75
    shapes = [(320, 320, 700), (1280, 2048, 77), (200, 64, 4100), (640, 9 * 64, 1024)]      # (N, K, M); the last one a 3x3 conv, Cin 64
    cpu, gpu = [], []
    for li, (N, K, M) in enumerate(shapes):
        L = dict(W=rnd(N, K, g=g, scale=1 / math.sqrt(K)), A_s=torch.zeros(Rp, K, dtype=BF), B_s=torch.zeros(N, Rp, dtype=BF), s=s,
                 B32=torch.randn(N, r, generator=g) * 0.2, mag=torch.rand(N, generator=g) + 0.5, scale=torch.zeros(N), Bt=torch.zeros(Rp, N, dtype=BF))
        L["A_s"][:r] = rnd(r, K, g=g, scale=1 / math.sqrt(K))
        L["B_s"][:, :r] = L["B32"].to(BF)
        cpu.append(L)
        gpu.append({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in L.items()})
    # transposed dX operands: linear [K, N] (period N) and conv [Cin, 9*Cout_p] (period Cout_p = 640, all valid; one with padding)
    wts_c, wts_g = [], []
    for li, (N, K, M) in enumerate(shapes):
        if li < 3:
            src = rnd(K, N, g=g)
            period, nvalid = N, N
        else:
            src = rnd(64, 9 * 640, g=g)
            period, nvalid = 640, 640
        wts_c.append(dict(src=src, dst=torch.zeros_like(src), scale=cpu[li]["scale"], period=period, nvalid=nvalid))
        wts_g.append(dict(src=src.cuda(), dst=torch.zeros_like(src).cuda(), scale=gpu[li]["scale"], period=period, nvalid=nvalid))
    src = rnd(32, 9 * 256, g=g)                 # padded layout: 200 valid of 256 columns per tap
    wts_c.append(dict(src=src, dst=torch.zeros_like(src), scale=cpu[2]["scale"], period=256, nvalid=200))
    wts_g.append(dict(src=src.cuda(), dst=torch.zeros_like(src).cuda(), scale=gpu[2]["scale"], period=256, nvalid=200))
    grads_c, grads_g = [], []
    for li, (N, K, M) in enumerate(shapes):
        big = rnd(M, N + 64, g=g)               # dY as a column slice of a wider buffer (stacked projections)
        e = dict(dY=big[:, 32:32 + N] if N % 8 == 0 and li == 0 else rnd(M, N, g=g), Y=rnd(M, N, g=g), bias=torch.randn(N, generator=g) if li != 1 else None,
                 mag=cpu[li]["mag"], scale=cpu[li]["scale"], gmag=torch.zeros(N), gB=torch.randn(N, r, generator=g))
        grads_c.append(e)
        eg = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in e.items()}
        if li == 0:
            bg = big.cuda()
            eg["dY"] = bg[:, 32:32 + N]
        eg["mag"], eg["scale"] = gpu[li]["mag"], gpu[li]["scale"]
        grads_g.append(eg)
    for init in (True, False):
        pc = E.DoraPlan(cpu, wts_c, grads_c, r, Rp, "cpu")
        pg = ops.DoraPlan(gpu, wts_g, grads_g, r, Rp, "cuda")
        if not init:
            for Lc, Lg in zip(cpu, gpu):
                m = torch.rand(Lc["mag"].shape, generator=g) + 0.5
                Lc["mag"].copy_(m)
                Lg["mag"].copy_(m)
        pc.refresh(init=init)
        pg.refresh(init=init)
        torch.cuda.synchronize()
        for li, (Lc, Lg) in enumerate(zip(cpu, gpu)):
            close(Lg["mag"], Lc["mag"], tol=2e-3, what=f"layer {li} magnitude (init={init})")
            close(Lg["scale"], Lc["scale"], tol=2e-3, what=f"layer {li} scale")
            close(Lg["Bt"], Lc["Bt"], tol=1e-2, what=f"layer {li} scaled B^T")
            if init:
                assert float((Lg["scale"] - 1).abs().max()) < 1e-6
        for wi, (wc, wg) in enumerate(zip(wts_c, wts_g)):
            close(wg["dst"], wc["dst"], tol=1e-2, what=f"scaled dX operand {wi}")
        if not init:
            assert float((wts_g[-1]["dst"].view(32, 9, 256)[:, :, 200:]).abs().max()) == 0.0
    pc.mag_grad()
    pg.mag_grad()
    torch.cuda.synchronize()
    first = [eg["gmag"].clone() for eg in grads_g]
    for li, (ec, eg) in enumerate(zip(grads_c, grads_g)):
        close(eg["gmag"], ec["gmag"], tol=1e-2, what=f"layer {li} magnitude gradient")
        close(eg["gB"], ec["gB"], tol=1e-5, what=f"layer {li} dB row scaling")
    for ec, eg in zip(grads_c, grads_g):        # fixed-order reduction: bitwise repeatable
        eg["gB"].copy_(ec["gB"].cuda())
    pg.mag_grad()
    torch.cuda.synchronize()
    assert all(torch.equal(a, eg["gmag"]) for a, eg in zip(first, grads_g))


# --------------------------------------------------------------------------------------------- text-encoder row-strip products
@pytest.mark.parametrize("B,N,K,mode", [(1, 1280, 1280, "res"), (1, 3840, 1280, "ln"), (1, 5120, 1280, "ln_act"), (1, 1280, 5120, "res"), (1, 5120, 1280, "dact"),
                                         (1, 1280, 3840, "plain"), (2, 2304, 768, "ln"), (4, 768, 3072, "res"), (1, 3072, 768, "ln_act"), (1, 768, 768, "plain"),
                                         (3, 512, 256, "ln"), (1, 4096, 2560, "dact"), (1, 64, 512, "res")])
def test_strip_gemm(ops, B, N, K, mode):
    _strip_case(ops, B, N, K, mode, None)


@pytest.mark.parametrize("B,N,K,mode,splitk", [(1, 1280, 5120, "res", 4), (1, 1280, 3840, "plain", 3), (2, 768, 3072, "res", 3), (1, 5120, 2560, "ln_act", 2),
                                                (1, 256, 4096, "ln", 16), (1, 1280, 5120, "dact", 5), (1, 1280, 1280, "res", 1)])
def test_strip_gemm_split_k(ops, B, N, K, mode, splitk):
    """The K split of the row-strip product: S workgroups per strip leave fp32 tiles (and partial row statistics) in the workspace, the
    last arriver adds them in split order - same values as the emulation, bitwise identical from launch to launch, counters re-armed."""
    _strip_case(ops, B, N, K, mode, splitk)
    _strip_case(ops, B, N, K, mode, splitk)          # a second round on the re-armed counters


def _strip_case(ops, B, N, K, mode, splitk):
    """sdlt_strip_gemm on every CLIP-L / OpenCLIP-bigG product shape (and odd ones: 1 ... 20 K steps per wave, 16- and 32-column strips):
    plain, + bias + residual, LayerNorm folded in front (statistics from the MFMA side products), activation side output, activation
    derivative factor.  Checked against the emulation of the contract AND, for the folded LayerNorm, against LayerNorm -> Linear on the
    unfolded weights (the reference's order of operations); rows t >= 77 of every batch element must stay untouched."""
    T, Tp = 77, 128
    g = torch.Generator().manual_seed(N + K + B)
    M = B * Tp
    x = rnd(M, K, g=g)
    x[:, :7] += 3.0                                           # a row mean far from zero: the algebraic LayerNorm must cancel it
    x[:, 5] *= 12.0                                           # CLIP-style outlier feature
    w = rnd(N, K, g=g, scale=K ** -0.5).float()
    bias = torch.randn(N, generator=g)
    res = rnd(M, N, g=g)
    pre = rnd(M, N, g=g)
    kind = "gelu" if (N + K) % 512 == 0 else "quick_gelu"
    kw = dict(B=B, T=T, Tp=Tp)
    valid = (torch.arange(M) % Tp) < T
    sentinel = 7.0

    def run(o, use_dev):
        cv = (lambda t: t.cuda()) if use_dev else (lambda t: t)
        out = torch.full((M, N), sentinel, dtype=BF, device="cuda" if use_dev else "cpu")
        extra = {}
        if mode in ("ln", "ln_act"):
            gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(1)), 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(2))
            wg, c1, c2 = E.fold_layernorm(w, bias, gamma, beta, dtype=BF)
            st = torch.zeros(M * 2, dtype=F32, device=out.device)
            a = torch.full((M, N), sentinel, dtype=BF, device=out.device) if mode == "ln_act" else None
            o.strip_gemm(cv(x), cv(wg), out, ln=(cv(c1), cv(c2), 1e-5), stats=st, act_out=(kind, a) if a is not None else None, splitk=splitk, **kw)
            extra = dict(stats=st, a=a, gamma=gamma, beta=beta)
        elif mode == "res":
            o.strip_gemm(cv(x), cv(w.to(BF)), out, bias=cv(bias), residual=cv(res), splitk=splitk, **kw)
        elif mode == "dact":
            o.strip_gemm(cv(x), cv(w.to(BF)), out, dact_in=(kind, cv(pre)), splitk=splitk, **kw)
        else:
            o.strip_gemm(cv(x), cv(w.to(BF)), out, splitk=splitk, **kw)
        return out, extra

    ref, rex = run(E, False)
    got, gex = run(ops, True)
    assert torch.all(got.cpu()[~valid] == sentinel), "rows t >= T were written"
    close(got.cpu()[valid], ref[valid], what=f"strip {mode}")
    if mode in ("ln", "ln_act"):
        xs = x.float()[valid]
        st = gex["stats"].cpu().view(M, 2)[valid]
        close(st[:, 0], xs.mean(1), tol=1e-3, what="strip ln mean")
        close(st[:, 1], torch.rsqrt(xs.var(1, unbiased=False) + 1e-5), tol=2e-3, what="strip ln rstd")
        # the reference's order: LayerNorm (fp32 statistics), then the Linear on the unfolded weights
        ln = torch.nn.functional.layer_norm(xs, (K,), rex["gamma"], rex["beta"], 1e-5)
        plain = ln @ w.to(BF).float().t() + bias
        close(got.cpu()[valid], plain, tol=2.5e-2, what="strip ln vs LayerNorm -> Linear")
        if mode == "ln_act":
            assert torch.all(gex["a"].cpu()[~valid] == sentinel)
            close(gex["a"].cpu()[valid], rex["a"][valid], what="strip activation output")
    # bitwise reproducible (fixed-order reduction of the 8 K slices)
    again, _ = run(ops, True)
    assert torch.equal(again, got)


@pytest.mark.parametrize("B,N,K,S", [(1, 1280, 5120, 3), (1, 1280, 3840, 3), (1, 768, 3072, 4), (2, 768, 2304, 3), (1, 1280, 1280, 1), (1, 512, 768, 2)])
def test_strip_gemm_partial_into_layernorm_bwd(ops, B, N, K, S):
    """The seam-less K split: sdlt_strip_gemm leaves S fp32 tiles per output (uneven step counts included), sdlt_layernorm_bwd_slabs adds
    them in its prologue.  Slabs against the emulation's slices, their sum against the unsplit product, and the LayerNorm backward on
    the slabs against the LayerNorm backward on the summed gradient."""
    T, Tp = 77, 128
    g = torch.Generator().manual_seed(N + K + S)
    M = B * Tp
    dy = rnd(M, K, g=g)
    w = rnd(N, K, g=g, scale=K ** -0.5)
    kw = dict(B=B, T=T, Tp=Tp)
    valid = (torch.arange(M) % Tp) < T
    pr = E.strip_gemm(dy, w, None, partial=torch.zeros(S, M, N), **kw)
    pg = ops.strip_gemm(dy.cuda(), w.cuda(), None, partial=torch.full((S, M, N), 7.0, device="cuda"), **kw)
    assert torch.all(pg.cpu()[:, ~valid] == 7.0)
    for sp in range(S):
        close(pg[sp].cpu()[valid], pr[sp][valid], tol=2e-3, what=f"partial slab {sp}")
    close(pg.sum(0).cpu()[valid], (dy.float() @ w.float().t())[valid], tol=2e-3, what="sum of the slabs")
    assert torch.equal(ops.strip_gemm(dy.cuda(), w.cuda(), None, partial=torch.zeros(S, M, N, device="cuda"), **kw)[:, valid.cuda()], pg[:, valid.cuda()])
    # consumer: LayerNorm backward with the slabs as its incoming gradient
    x, gamma, dres = rnd(M, N, g=g), 1.0 + 0.1 * torch.randn(N, generator=g), rnd(M, N, g=g)
    stats = torch.zeros(M * 2, device="cuda")
    ops.layernorm_fwd(x.cuda(), torch.empty(M, N, dtype=BF, device="cuda"), stats, gamma=gamma.cuda(), beta=torch.zeros(N, device="cuda"))
    pz = pg.clone()
    pz[:, ~valid.cuda()] = 0.0
    ref = E.layernorm_bwd(x, pz.sum(0).cpu(), torch.empty(M, N, dtype=BF), None, gamma=gamma, dres=dres)
    got = ops.layernorm_bwd(x.cuda(), None, torch.empty(M, N, dtype=BF, device="cuda"), stats, gamma=gamma.cuda(), dres=dres.cuda(), dy_slabs=pz)
    close(got, ref, tol=2e-2, what="layernorm bwd on slabs")


@pytest.mark.parametrize("M,N,K,res,bias", [(1024, 1280, 5120, True, True), (1024, 1280, 3840, False, False), (128, 640, 2560, True, False), (2048, 640, 4096, False, True),
                                            (64, 1280, 256, True, True)])
def test_wsk_gemm(ops, M, N, K, res, bias):
    """sdlt_wsk_gemm (64 x 80 tiles, K split over the waves of a workgroup) against fp32 math on the same bf16 operands; both XCD mappings
    of the tiles (rows x columns even / odd), ragged step counts per wave, bitwise reproducible; and ops.gemm routes the ff.net.2 shape to it."""
    import ctypes as C
    g = torch.Generator().manual_seed(M + N + K)
    x, w = rnd(M, K, g=g), rnd(N, K, g=g, scale=K ** -0.5)
    b = torch.randn(N, generator=g) if bias else None
    r = rnd(M, N, g=g) if res else None
    ref = x.float() @ w.float().t() + (b if bias else 0.0) + (r.float() if res else 0.0)
    lib = ops._lib.load()
    xd, wd = x.cuda(), w.cuda()
    bd, rd = (b.cuda() if bias else None), (r.cuda() if res else None)

    def run():
        y = torch.full((M, N), 7.0, dtype=BF, device="cuda")
        rc = lib.sdlt_wsk_gemm(xd.data_ptr(), K, wd.data_ptr(), K, M, N, K, bd.data_ptr() if bias else None, rd.data_ptr() if res else None, N if res else 0,
                               y.data_ptr(), N, None, 0, None, 0, 0.0, None, 0, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.sdlt_last_error()
        return y
    y = run()
    close(y, ref, what="wsk gemm")
    assert torch.equal(run(), y)
    if ops.wsk_shape(M, N, K):
        y2 = torch.empty(M, N, dtype=BF, device="cuda")
        ops.gemm(xd, wd, y2, bias=bd, residual=rd)
        assert torch.equal(y2, y), "ops.gemm did not take the wave-split-K route for this shape"


@pytest.mark.parametrize("M,N,K,res,bias,rank", [(1024, 1280, 1280, True, True, 16), (1024, 1280, 1280, False, False, 8), (512, 1280, 2560, True, False, 4), (128, 640, 256, False, True, 16)])
def test_wsk_gemm_fused_lora(ops, M, N, K, res, bias, rank):
    """sdlt_wsk_gemm with a rank-<=16 adapter riding along, against the emulation of the tiled kernel's LoRA contract (T rounded to bf16
    before the up-projection, T_out = bf16(s X Adown^T)) and against sdlt_gemm_bf16 itself; ops.gemm routes the 1024 x 1280 x 1280 projections here."""
    g = torch.Generator().manual_seed(M + N + K + rank)
    x, w = rnd(M, K, g=g), rnd(N, K, g=g, scale=K ** -0.5)
    A, Bu = torch.zeros(16, K, dtype=BF), torch.zeros(N, 16, dtype=BF)
    A[:rank], Bu[:, :rank] = rnd(rank, K, g=g, scale=1.0 / rank), rnd(N, rank, g=g, scale=0.05)
    b = torch.randn(N, generator=g) if bias else None
    r = rnd(M, N, g=g) if res else None
    scale = 1.5
    ref, tref = torch.empty(M, N, dtype=BF), torch.empty(M, 16, dtype=BF)
    E.gemm(x, w, ref, lora=(A, Bu, scale, tref), bias=b, residual=r)
    lib = ops._lib.load()
    xd, wd, Ad, Bd = x.cuda(), w.cuda(), A.cuda(), Bu.cuda()
    bd, rd = (b.cuda() if bias else None), (r.cuda() if res else None)
    y, T = torch.full((M, N), 7.0, dtype=BF, device="cuda"), torch.full((M, 16), 7.0, dtype=BF, device="cuda")
    rc = lib.sdlt_wsk_gemm(xd.data_ptr(), K, wd.data_ptr(), K, M, N, K, bd.data_ptr() if bias else None, rd.data_ptr() if res else None, N if res else 0,
                           y.data_ptr(), N, Ad.data_ptr(), K, Bd.data_ptr(), 16, scale, T.data_ptr(), 16, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sdlt_last_error()
    close(y, ref, what="wsk gemm + lora")
    close(T, tref, what="wsk T_out")
    y2, T2 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, 16, dtype=BF, device="cuda")
    ops.gemm(xd, wd, y2, lora=(Ad, Bd, scale, T2), bias=bd, residual=rd, tile=2)            # the tiled kernel (an explicit tile keeps it there)
    close(y, y2, tol=1e-2, what="wsk vs tiled kernel")
    close(T, T2, tol=1e-2, what="wsk vs tiled T_out")
    if ops.wsk_shape(M, N, K, True):
        y3, T3 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, 16, dtype=BF, device="cuda")
        ops.gemm(xd, wd, y3, lora=(Ad, Bd, scale, T3), bias=bd, residual=rd)
        assert torch.equal(y3, y) and torch.equal(T3, T), "ops.gemm did not take the wave-split-K route for this shape"


@pytest.mark.parametrize("M,N,gk,G,res", [(1024, 1280, 1280, 3, False), (1024, 1280, 640, 2, True), (256, 640, 256, 3, True)])
def test_wsk_gemm_k_grouped_lora(ops, M, N, gk, G, res):
    """The input gradient of stacked projections on the wave-split-K kernel: K = G groups of gk columns, one rank-16 adapter per group
    (sdlt_gemm_bf16's lora_group_k contract) - against the emulation, the tiled kernel, and through ops.gemm's routing."""
    K = gk * G
    g = torch.Generator().manual_seed(M + N + K)
    x, w = rnd(M, K, g=g), rnd(N, K, g=g, scale=K ** -0.5)
    A, Bu = rnd(16, K, g=g, scale=1.0 / 16), rnd(N, 16 * G, g=g, scale=0.05)
    r = rnd(M, N, g=g) if res else None
    ref, tref = torch.empty(M, N, dtype=BF), torch.empty(M, 16 * G, dtype=BF)
    E.gemm(x, w, ref, lora=(A, Bu, 0.75, tref), residual=r, lora_group_k=gk)
    xd, wd, Ad, Bd, rd = x.cuda(), w.cuda(), A.cuda(), Bu.cuda(), (r.cuda() if res else None)
    y, T = torch.full((M, N), 7.0, dtype=BF, device="cuda"), torch.full((M, 16 * G), 7.0, dtype=BF, device="cuda")
    lib = ops._lib.load()
    rc = lib.sdlt_wsk_gemm(xd.data_ptr(), K, wd.data_ptr(), K, M, N, K, None, rd.data_ptr() if res else None, N if res else 0, y.data_ptr(), N,
                           Ad.data_ptr(), K, Bd.data_ptr(), 16 * G, 0.75, T.data_ptr(), 16 * G, gk, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sdlt_last_error()
    close(y, ref, what="wsk K-grouped lora")
    close(T, tref, what="wsk K-grouped T_out")
    y2, T2 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, 16 * G, dtype=BF, device="cuda")
    ops.gemm(xd, wd, y2, lora=(Ad, Bd, 0.75, T2), residual=rd, lora_group_k=gk, tile=2)
    close(y, y2, tol=1e-2, what="wsk vs tiled kernel (K-grouped)")
    if ops.wsk_shape(M, N, K, True):
        y3, T3 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, 16 * G, dtype=BF, device="cuda")
        ops.gemm(xd, wd, y3, lora=(Ad, Bd, 0.75, T3), residual=rd, lora_group_k=gk)
        assert torch.equal(y3, y) and torch.equal(T3, T)


@pytest.mark.parametrize("M,N,K,rank,dora,side", [(1024, 1280, 1280, 24, False, "res"), (1024, 1280, 1280, 32, False, "parts"), (1024, 1280, 1280, 24, False, "rowdot"),
                                                  (512, 1280, 2560, 20, False, "none"), (128, 640, 256, 32, False, "res"), (1024, 1280, 5120, 24, False, "res"),
                                                  (1024, 1280, 1280, 16, True, "none"), (1024, 1280, 1280, 24, True, "none"), (256, 640, 1024, 8, True, "none"),
                                                  (1024, 1280, 1280, 16, True, "y0"), (1024, 1280, 1280, 24, True, "y0parts")])
def test_wsk_gemm_rank_groups_and_dora(ops, M, N, K, rank, dora, side):
    """sdlt_wsk_gemm_p (round 6): adapter rank pad 32 - the sweep's rank 24, scripts/create_hyperparam_sweep.py:76 - as 2 groups of 16 LoRA-down rows on the
    packed-weight kernel (rank pad 64 is refused: csrc/wsk.hip says why), and DoRA's column factor in the epilogue, against the emulation of the tiled kernel's contract and against sdlt_gemm_bf16 itself; the row-partial and
    row-dot side outputs ride along unchanged; ops.gemm must select this kernel for a frozen weight (asserted through the packed-copy registry and bit equality)."""
    Rp = 16 if rank <= 16 else (32 if rank <= 32 else 64)
    g = torch.Generator().manual_seed(M + N + K + rank + int(dora))
    x, w = rnd(M, K, g=g), rnd(N, K, g=g, scale=K ** -0.5)
    A, Bu = torch.zeros(Rp, K, dtype=BF), torch.zeros(N, Rp, dtype=BF)
    A[:rank], Bu[:, :rank] = rnd(rank, K, g=g, scale=1.0 / rank), rnd(N, rank, g=g, scale=0.05)
    b = torch.randn(N, generator=g)
    r = rnd(M, N, g=g) if side in ("res", "parts", "y0", "y0parts") else None
    cs = (1.0 + 0.2 * torch.randn(N, generator=g)) if dora else None
    want_y0 = side.startswith("y0")
    scale = 1.5
    ref, tref = torch.empty(M, N, dtype=BF), torch.empty(M, Rp, dtype=BF)
    E.gemm(x, w, ref, lora=(A, Bu, scale, tref), bias=b, residual=r, **({"col_scale": cs} if dora else {}))
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    xd, wd, Ad, Bd, bd = x.cuda(), w.cuda(), A.cuda(), Bu.cuda(), b.cuda()
    rd, csd = (r.cuda() if r is not None else None), (cs.cuda() if dora else None)
    wp = torch.empty(N * K, dtype=BF, device="cuda")
    ops._lib.check(lib.sdlt_wsk_pack_weight(wd.data_ptr(), K, N, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
    Nq = 256 if M % 256 == 0 else M
    o = rnd(M, N, g=g).cuda()

    def run(packed=True):
        y, T = torch.full((M, N), 7.0, dtype=BF, device="cuda"), torch.full((M, Rp), 7.0, dtype=BF, device="cuda")
        parts, D = torch.zeros(M, N // 80, 2, device="cuda"), torch.zeros(M * (N // 64), device="cuda")
        y0 = torch.full((M, N), 7.0, dtype=BF, device="cuda")
        q = ops._lib.WskGemmParams()
        q.X, q.ldx, q.W, q.ldw, q.M, q.N, q.K = xd.data_ptr(), K, (wp if packed else wd).data_ptr(), 0 if packed else K, M, N, K
        q.bias, q.Y, q.ldy = bd.data_ptr(), y.data_ptr(), N
        q.Adown, q.ld_adown, q.Bup, q.ld_bup, q.lora_scale, q.lora_rp, q.T_out, q.ld_t = Ad.data_ptr(), K, Bd.data_ptr(), Rp, scale, Rp, T.data_ptr(), Rp
        if rd is not None:
            q.R, q.ldr = rd.data_ptr(), N
        if dora:
            q.col_scale = csd.data_ptr()
        if side in ("parts", "y0parts"):
            q.ln_parts = parts.data_ptr()
        if want_y0:
            q.Y0, q.ldy0 = y0.data_ptr(), N
        if side == "rowdot":
            q.R, q.ldr, q.dotD, q.dot_nq = o.data_ptr(), N, D.data_ptr(), Nq
        rc = lib.sdlt_wsk_gemm_p(C.byref(q), st)
        assert rc == 0, lib.sdlt_last_error()
        torch.cuda.synchronize()
        run.y0 = y0
        return y, T, parts, D
    import ctypes as C
    y, T, parts, D = run()
    close(y, ref, what="wsk gemm_p")
    if want_y0:        # the layer's own output before the residual, from the same launch
        ref0 = torch.empty(M, N, dtype=BF)
        E.gemm(x, w, ref0, lora=(A, Bu, scale, None), bias=b, col_scale=cs)
        close(run.y0, ref0, what="wsk gemm_p Y0")
    close(T, tref, what="wsk gemm_p T_out")
    y1 = run()
    assert all(torch.equal(a_, b_) for a_, b_ in zip((y, T, parts, D), y1)), "not reproducible"
    if Rp == 16:          # the row-major ring gives the same bits (rank pads above 16 exist for packed weights only, and say so)
        assert torch.equal(run(packed=False)[0], y)
    else:
        q = ops._lib.WskGemmParams()
        q.X, q.ldx, q.W, q.ldw, q.M, q.N, q.K, q.Y, q.ldy = xd.data_ptr(), K, wd.data_ptr(), K, M, N, K, y1[0].data_ptr(), N
        q.Adown, q.ld_adown, q.Bup, q.ld_bup, q.lora_scale, q.lora_rp = Ad.data_ptr(), K, Bd.data_ptr(), Rp, scale, Rp
        assert lib.sdlt_wsk_gemm_p(C.byref(q), st) != 0 and b"packed" in lib.sdlt_last_error()
        q.W, q.ldw, q.lora_rp, q.ld_bup = wp.data_ptr(), 0, 64, 64
        assert lib.sdlt_wsk_gemm_p(C.byref(q), st) != 0 and b"lora_rp=64" in lib.sdlt_last_error()
    y2, T2 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, Rp, dtype=BF, device="cuda")
    ops.gemm(xd, wd, y2, lora=(Ad, Bd, scale, T2), bias=bd, residual=rd, tile=2, **({"col_scale": csd} if dora else {}))      # the tiled kernel (an explicit tile keeps it there)
    close(y, y2, tol=1e-2, what="wsk_p vs tiled kernel")
    close(T, T2, tol=1e-2, what="wsk_p vs tiled T_out")
    if side in ("parts", "y0parts"):
        yf = y.float().view(M, N // 80, 80)
        close(parts[:, :, 0], yf.sum(-1), tol=1e-3, what="row partial sums")
        close(parts[:, :, 1], ((yf - yf.mean(-1, keepdim=True)) ** 2).sum(-1), tol=2e-3, what="row partial centred squares")
    if side == "rowdot":
        Dref = (y.float() * o.float()).view(M // Nq, Nq, N // 64, 64).sum(-1).permute(0, 2, 1).reshape(-1)
        close(D, Dref, tol=2e-3, what="row dots")
    if ops.wsk_shape(M, N, K, True):      # ops.gemm: a frozen weight takes this kernel (same bits), an unmarked one stays on the tiled kernel for rank pads above 16
        ops.wsk_mark_frozen(wd)
        y3, T3 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, Rp, dtype=BF, device="cuda")
        kw = {"col_scale": csd} if dora else {}
        if side in ("parts", "y0parts"):
            assert ops.gemm_emits_parts(M, N, K, Rp, wd, dora=dora) == N // 80
            kw["ln_parts_out"] = torch.zeros(M, N // 80, 2, device="cuda")
        if want_y0:
            kw["out0"] = torch.empty(M, N, dtype=BF, device="cuda")
        rdot = dict(O=o, D=torch.zeros_like(D), Nq=Nq, done=False) if side == "rowdot" else None
        ops.gemm(xd, wd, y3, lora=(Ad, Bd, scale, T3), bias=bd, residual=rd, rowdot=rdot, **kw)
        assert wd.data_ptr() in ops._WSK_PACKED and torch.equal(y3, y) and torch.equal(T3, T), "ops.gemm did not select the wave-split-K kernel"
        if side == "rowdot":
            assert rdot["done"] and torch.equal(rdot["D"], D)
        if side in ("parts", "y0parts"):
            assert torch.equal(kw["ln_parts_out"], parts)
        if want_y0:
            assert torch.equal(kw["out0"], run.y0)


@pytest.mark.parametrize("M,N,K,mode", [(1024, 1280, 1280, "plain"), (1024, 1280, 5120, "plain"), (1024, 1280, 10240, "plain"), (64, 1280, 256, "plain"), (128, 640, 512, "plain"),
                                        (128, 640, 768, "lora"), (256, 640, 1024, "plain"), (2048, 640, 4096, "plain"), (1024, 1280, 1280, "lora"), (512, 1280, 2560, "lora"),
                                        (1024, 1280, 3840, "kgroup"), (256, 640, 768, "kgroup"), (1024, 1280, 1280, "ln"), (1024, 1280, 1280, "ln_lora"), (1024, 1280, 5120, "parts"),
                                        (1024, 1280, 1280, "parts_lora")])
def test_wsk_gemm_packed_weight_is_bit_identical(ops, M, N, K, mode):
    """Frozen weights in fragment-major order (sdlt_wsk_pack_weight; W passed with ldw = 0): the weight fragments go from global memory straight into a
    register ring instead of through LDS.  Same arithmetic in the same order - every entry point, adapter form and side output must give the SAME BITS as
    the row-major call (which the tests above pin against fp32 math); step counts per wave of 1, 2, 3, 4, 5, 10, 15, 16, 20, 40 exercise the prologue /
    steady state / drain of the 3-deep ring, and ops.gemm must take the packed route for a weight declared frozen."""
    g = torch.Generator().manual_seed(M + N + K + len(mode))
    lora, kgroup, ln, parts = "lora" in mode or mode == "kgroup", mode == "kgroup", mode.startswith("ln"), mode.startswith("parts")
    G = 3 if kgroup else 1
    x = (rnd(M, K, g=g).float() * (2.0 if ln else 1.0) + (0.7 if ln else 0.0)).to(BF).cuda()
    w = rnd(N, K, g=g, scale=K ** -0.5).cuda()
    b, r = torch.randn(N, generator=g).cuda(), rnd(M, N, g=g).cuda()
    A, Bu = rnd(16, K, g=g, scale=1.0 / 16).cuda(), rnd(N, 16 * G, g=g, scale=0.05).cuda()
    c1, consts = torch.randn(N, generator=g).cuda(), torch.randn(32, generator=g).cuda()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    wp = torch.empty(N * K, dtype=BF, device="cuda")
    ops._lib.check(lib.sdlt_wsk_pack_weight(w.data_ptr(), K, N, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
    # the layout of include/sdlt_kernels.h, element by element
    ref_pack = w.view(N // 80, 5, 16, K // 64, 2, 4, 8).permute(0, 3, 4, 1, 5, 2, 6).contiguous().view(-1)
    assert torch.equal(wp, ref_pack)

    def run(wptr, ldw):
        y = torch.full((M, N), 7.0, dtype=BF, device="cuda")
        T = torch.full((M, 16 * G), 7.0, dtype=BF, device="cuda")
        stats = torch.zeros(M, 2, device="cuda")
        pr = torch.zeros(M, N // 80, 2, device="cuda")
        la = (A.data_ptr(), K, Bu.data_ptr(), 16 * G, 0.75, T.data_ptr(), 16 * G) if lora else (None, 0, None, 0, 0.0, None, 0)
        if ln:
            rc = lib.sdlt_wsk_gemm_ln(x.data_ptr(), K, wptr, ldw, M, N, K, b.data_ptr(), r.data_ptr(), N, y.data_ptr(), N, *la, c1.data_ptr(), stats.data_ptr(), 1e-5,
                                      consts.data_ptr() if lora else None, st)
        elif parts:
            rc = lib.sdlt_wsk_gemm_parts(x.data_ptr(), K, wptr, ldw, M, N, K, b.data_ptr(), r.data_ptr(), N, y.data_ptr(), N, *la, 0, pr.data_ptr(), st)
        else:
            rc = lib.sdlt_wsk_gemm(x.data_ptr(), K, wptr, ldw, M, N, K, b.data_ptr(), r.data_ptr(), N, y.data_ptr(), N, *la, K // G if kgroup else 0, st)
        assert rc == 0, lib.sdlt_last_error()
        torch.cuda.synchronize()
        return y, T, stats, pr
    base, packed = run(w.data_ptr(), K), run(wp.data_ptr(), 0)
    assert float((base[0].float() - 7.0).abs().max()) > 1.0          # (the kernel wrote the output)
    for a_, b_, what in zip(base, packed, ("Y", "T_out", "ln_stats", "ln_parts")):
        assert torch.equal(a_, b_), f"packed weight: {what} differs, max abs diff {float((a_.float() - b_.float()).abs().max())}"
    assert torch.equal(run(wp.data_ptr(), 0)[0], packed[0])          # reproducible
    if mode in ("plain", "lora", "kgroup") and ops.wsk_shape(M, N, K, lora):      # ops.gemm: the packed route for a weight declared frozen, lazily on first use
        ops.wsk_mark_frozen(w)
        y2, T2 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, 16 * G, dtype=BF, device="cuda")
        ops.gemm(x, w, y2, bias=b, residual=r, **(dict(lora=(A, Bu, 0.75, T2), lora_group_k=K // G if kgroup else 0) if lora else {}))
        assert w.data_ptr() in ops._WSK_PACKED and torch.equal(ops._WSK_PACKED[w.data_ptr()][0], wp)
        assert torch.equal(y2, base[0]) and (not lora or torch.equal(T2, base[1]))
        if mode == "plain":
            # the copy follows the tensor: an in-place rewrite is noticed by the next eager call (version counter) and re-packed, wsk_invalidate() drops it,
            # and the registration + copy die with the tensor (a long-lived worker must not keep every model's packed weights alive)
            w.mul_(-1.0)
            ops.gemm(x, w, y2, bias=b, residual=r)
            y3 = torch.empty_like(y2)
            ops._lib.check(lib.sdlt_wsk_gemm(x.data_ptr(), K, w.data_ptr(), K, M, N, K, b.data_ptr(), r.data_ptr(), N, y3.data_ptr(), N, None, 0, None, 0, 0.0, None, 0, 0, st), "sdlt_wsk_gemm")
            assert torch.equal(y2, y3) and not torch.equal(y2, base[0])
            key = w.data_ptr()
            ops.wsk_invalidate(w)
            assert key not in ops._WSK_PACKED and key in ops._WSK_FROZEN
            ops.gemm(x, w, y2, bias=b, residual=r)
            assert key in ops._WSK_PACKED
            del w
            import gc
            gc.collect()
            assert key not in ops._WSK_PACKED and key not in ops._WSK_FROZEN


@pytest.mark.parametrize("B,Nq,N,K,lora,packed", [(1, 1024, 1280, 1280, True, True), (1, 1024, 1280, 1280, True, False), (4, 256, 1280, 1280, True, True), (1, 1024, 1280, 2560, False, True),
                                                  (2, 256, 640, 1280, True, False), (1, 4096, 640, 2560, False, True)])
def test_wsk_gemm_rowdot(ops, B, Nq, N, K, lora, packed):
    """sdlt_wsk_gemm_rowdot: Y = the plain wave-split-K product (same bits) and D[b, h, q] = sum over head h's 64 columns of rounded(Y) o O on a zeroed D - what the
    attention backward's D pre-pass computes from the stored dO.  A head's columns lie in at most two 80-column tiles, so the two float atomics per slot commute: bitwise
    reproducible.  O is NOT added to Y."""
    M, H = B * Nq, N // 64
    g = torch.Generator().manual_seed(M + N + K + int(lora))
    x, w = rnd(M, K, g=g).cuda(), rnd(N, K, g=g, scale=K ** -0.5).cuda()
    o = rnd(M, N, g=g).cuda()
    A, Bu = rnd(16, K, g=g, scale=1.0 / 16).cuda(), rnd(N, 16, g=g, scale=0.05).cuda()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    wptr, ldw = w.data_ptr(), K
    if packed:
        wp = torch.empty(N * K, dtype=BF, device="cuda")
        ops._lib.check(lib.sdlt_wsk_pack_weight(w.data_ptr(), K, N, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
        wptr, ldw = wp.data_ptr(), 0

    def run(dot):
        y, T = torch.full((M, N), 7.0, dtype=BF, device="cuda"), torch.full((M, 16), 7.0, dtype=BF, device="cuda")
        D = torch.zeros(B * H * Nq, device="cuda")
        la = (A.data_ptr(), K, Bu.data_ptr(), 16, 0.75, T.data_ptr(), 16) if lora else (None, 0, None, 0, 0.0, None, 0)
        if dot:
            rc = lib.sdlt_wsk_gemm_rowdot(x.data_ptr(), K, wptr, ldw, M, N, K, None, o.data_ptr(), N, y.data_ptr(), N, *la, 0, D.data_ptr(), Nq, st)
        else:
            rc = lib.sdlt_wsk_gemm(x.data_ptr(), K, wptr, ldw, M, N, K, None, None, 0, y.data_ptr(), N, *la, 0, st)
        assert rc == 0, lib.sdlt_last_error()
        torch.cuda.synchronize()
        return y, T, D
    y0, T0, _ = run(False)
    y1, T1, D1 = run(True)
    assert torch.equal(y0, y1) and torch.equal(T0, T1)
    want = (y1.double() * o.double()).reshape(B, Nq, H, 64).sum(-1).permute(0, 2, 1).reshape(-1)
    torch.testing.assert_close(D1.double(), want, rtol=1e-5, atol=2e-6 * float(want.abs().max()))
    for _ in range(3):
        assert torch.equal(run(True)[2], D1)
    # through ops.gemm: reports the side output, D accumulates onto what is there (the forward zeroes it)
    rd = dict(O=o, D=torch.zeros(B * H * Nq, device="cuda"), Nq=Nq, done=False)
    y2 = torch.empty(M, N, dtype=BF, device="cuda")
    ops.gemm(x, w, y2, **(dict(lora=(A, Bu, 0.75, torch.empty(M, 16, dtype=BF, device="cuda"))) if lora else {}), rowdot=rd)
    if ops.wsk_shape(M, N, K, lora):
        assert rd["done"] and torch.equal(y2, y1) and torch.equal(rd["D"], D1)
    else:
        assert not rd["done"] and float(rd["D"].abs().max()) == 0.0


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("M", [64, 128, 1024])
def test_wsk_entry_points_agree(ops, M, packed):
    """The flat entry points sdlt_wsk_gemm / _ln / _parts / _rowdot, the parameter block sdlt_wsk_gemm_p and ops.gemm are three ways to hand the SAME arguments to the same
    kernel, whose sums are ordered: every output must agree bit for bit (no tolerance).  N = 640, K = 1024: four K steps per wave (more than either ring depth: refills run; a
    tile rotation of up to 3); M = 64 is one row tile (the 1D XCD map), M = 128 two (the 2D map); row-major and packed weights.  ops.gemm: wsk_shape admits K = 1024 only with an
    adapter and from 128 tiles on, so that part runs at M = 1024 (the smallest M the predicate accepts for N = 640) on the adapter forms; the plain product has no admitted M."""
    import ctypes as C
    N, K, Nq, gk = 640, 1024, 64, 512
    g = torch.Generator().manual_seed(M + int(packed))
    x, w = rnd(M, K, g=g).cuda(), rnd(N, K, g=g, scale=K ** -0.5).cuda()
    b, r, o = torch.randn(N, generator=g).cuda(), rnd(M, N, g=g).cuda(), rnd(M, N, g=g).cuda()
    A, Bu, Bu2 = rnd(16, K, g=g, scale=1.0 / 16).cuda(), rnd(N, 16, g=g, scale=0.05).cuda(), rnd(N, 32, g=g, scale=0.05).cuda()
    c1, consts = torch.randn(N, generator=g).cuda(), torch.randn(32, generator=g).cuda()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    wptr, ldw = w.data_ptr(), K
    if packed:
        wp = torch.empty(N * K, dtype=BF, device="cuda")
        ops._lib.check(lib.sdlt_wsk_pack_weight(w.data_ptr(), K, N, K, wp.data_ptr(), st), "sdlt_wsk_pack_weight")
        wptr, ldw = wp.data_ptr(), 0
    forms = ("plain", "lora", "kgroup", "ln", "parts", "rowdot")        # every form but "plain" carries a rank-16 adapter ("kgroup": one per group of 512 columns)

    def outputs(form):         # (D is zeroed before each call)
        G = 2 if form == "kgroup" else 1
        return dict(Y=torch.full((M, N), 7.0, dtype=BF, device="cuda"), T=torch.full((M, 16 * G), 7.0, dtype=BF, device="cuda"), stats=torch.zeros(M, 2, device="cuda"),
                    parts=torch.zeros(M, N // 80, 2, device="cuda"), D=torch.zeros(M * (N // 64), device="cuda"))

    def flat(form):
        t = outputs(form)
        Bu_ = Bu2 if form == "kgroup" else Bu
        la = (A.data_ptr(), K, Bu_.data_ptr(), Bu_.shape[1], 0.75, t["T"].data_ptr(), t["T"].shape[1]) if form != "plain" else (None, 0, None, 0, 0.0, None, 0)
        head, y = (x.data_ptr(), K, wptr, ldw, M, N, K, b.data_ptr()), t["Y"].data_ptr()
        if form == "ln":
            rc = lib.sdlt_wsk_gemm_ln(*head, r.data_ptr(), N, y, N, *la, c1.data_ptr(), t["stats"].data_ptr(), 1e-5, consts.data_ptr(), st)
        elif form == "parts":
            rc = lib.sdlt_wsk_gemm_parts(*head, r.data_ptr(), N, y, N, *la, 0, t["parts"].data_ptr(), st)
        elif form == "rowdot":
            rc = lib.sdlt_wsk_gemm_rowdot(*head, o.data_ptr(), N, y, N, *la, 0, t["D"].data_ptr(), Nq, st)
        else:
            rc = lib.sdlt_wsk_gemm(*head, r.data_ptr(), N, y, N, *la, gk if form == "kgroup" else 0, st)
        assert rc == 0, lib.sdlt_last_error()
        return t

    def block(form):
        t = outputs(form)
        q = ops._lib.WskGemmParams()
        q.X, q.ldx, q.W, q.ldw, q.M, q.N, q.K, q.bias, q.Y, q.ldy = x.data_ptr(), K, wptr, ldw, M, N, K, b.data_ptr(), t["Y"].data_ptr(), N
        q.R, q.ldr = (o if form == "rowdot" else r).data_ptr(), N
        if form != "plain":
            Bu_ = Bu2 if form == "kgroup" else Bu
            q.Adown, q.ld_adown, q.Bup, q.ld_bup, q.lora_scale, q.lora_rp, q.T_out, q.ld_t = A.data_ptr(), K, Bu_.data_ptr(), Bu_.shape[1], 0.75, 16, t["T"].data_ptr(), t["T"].shape[1]
        if form == "kgroup":
            q.lora_group_k = gk
        if form == "ln":
            q.ln_c1, q.ln_stats, q.ln_eps, q.ln_adapter = c1.data_ptr(), t["stats"].data_ptr(), 1e-5, consts.data_ptr()
        if form == "parts":
            q.ln_parts = t["parts"].data_ptr()
        if form == "rowdot":
            q.dotD, q.dot_nq = t["D"].data_ptr(), Nq
        rc = lib.sdlt_wsk_gemm_p(C.byref(q), st)
        assert rc == 0, lib.sdlt_last_error()
        return t

    def via_ops(form, **kw):
        t = outputs(form)
        kw = dict(dict(lora=(A, Bu2 if form == "kgroup" else Bu, 0.75, t["T"]), bias=b, residual=r, lora_group_k=gk if form == "kgroup" else 0), **kw)
        if form == "ln":
            kw["ln"] = (c1, t["stats"], 1e-5, consts)
        if form == "parts":
            kw["ln_parts_out"] = t["parts"]
        if form == "rowdot":
            t["rd"] = kw["rowdot"] = dict(O=o, D=t["D"], Nq=Nq, done=False)
        ops.gemm(x, w, t["Y"], **kw)
        return t

    def same(got, want, what):
        torch.cuda.synchronize()
        for k in ("Y", "T", "stats", "parts", "D"):
            assert torch.equal(got[k], want[k]), f"{what}: {k} differs, max abs diff {float((got[k].float() - want[k].float()).abs().max())}"

    ref = {form: flat(form) for form in forms}
    for form in forms:
        assert float((ref[form]["Y"].float() - 7.0).abs().max()) > 1.0          # (the kernel wrote the output)
        same(block(form), ref[form], f"sdlt_wsk_gemm_p, {form}")
    assert float(ref["rowdot"]["D"].abs().max()) > 0.0 and float(ref["parts"]["parts"].abs().max()) > 0.0 and float(ref["ln"]["stats"].abs().max()) > 0.0
    if not ops.wsk_shape(M, N, K, True):
        return
    if packed:
        ops.wsk_mark_frozen(w)
    for form in forms[1:]:
        t = via_ops(form, **(dict(residual=None) if form == "rowdot" else {}))
        same(t, ref[form], f"ops.gemm, {form}")
        assert form != "rowdot" or t["rd"]["done"]
    assert (w.data_ptr() in ops._WSK_PACKED) == packed and (not packed or torch.equal(ops._WSK_PACKED[w.data_ptr()][0], wp))
    t = via_ops("rowdot")          # with a residual the row-dot form does not apply: the plain adapter product, D untouched, nothing reported
    same(t, ref["lora"], "ops.gemm, rowdot + residual")
    assert not t["rd"]["done"]


@pytest.mark.parametrize("B,sizes,ratio,has", [(1, [(64, 64, 10), (32, 32, 50)], 1.0, [1]), (2, [(64, 64, 3), (32, 32, 6), (16, 16, 6)], 1.0, [1, 0]),
                                               (2, [(32, 32, 4)], 1.0, [1, 1]), (1, [(32, 64, 2), (16, 32, 5)], 2.0, [1]), (2, [(32, 32, 2), (16, 16, 2)], 1.0, [0, 0])])
def test_token_attention_loss_fused(ops, B, sizes, ratio, has):
    """sdlt_token_attention_loss (three launches) against the torch-op form of the same loss (daam.TokenAttentionLoss with FUSED off - the
    arithmetic tests/test_oracle_golden.py pins to the reference's compute_token_attention_loss): loss value and d(weight loss)/dS of every
    resolution, row-major and transposed; SDXL's two and SD1.5's three resolutions, a non-square latent, captions without the trained tokens."""
    import sd_lora_trainer_amd.daam as D
    import sd_lora_trainer_amd.unet as M
    g = torch.Generator().manual_seed(B + len(sizes))
    ntok, train_ids = 3, [900, 901, 902]
    lists = [[1, 5, 6] + (train_ids if has[b] else [7]) + [8, 9, 11, 2] for b in range(B)]
    Hm, Wm = sizes[0][0] * 2, sizes[0][1] * 2
    mask = ((torch.rand(B, 1, Hm, Wm, generator=g) > 0.5).float() * 0.9 + 0.05).repeat(1, 4, 1, 1).contiguous().cuda()
    res = {}
    for fused in (False, True):
        rt = M.Runtime("cuda:0", B)
        ta = D.TokenAttentionLoss(rt, ntok)
        ta.set_captions(lists, train_ids)
        gs = torch.Generator().manual_seed(7)
        for (h, w, nl) in sizes:
            S = torch.zeros(B * h * w, 128)
            S[:, :77] = torch.randn(B * h * w, 77, generator=gs) * 3.0 * nl
            rt.daam_sums[h * w] = [S.cuda(), nl, True]
        D.FUSED = fused
        try:
            loss = ta.forward_backward(mask, ratio, 0.05)
        finally:
            D.FUSED = True
        torch.cuda.synchronize()
        assert (ta._fused_plan(mask, ratio) is not None) if fused else True
        res[fused] = (float(loss), {N: (a.float().cpu().clone(), b_.float().cpu().clone()) for N, (a, b_) in rt.daam_grads.items()})
    l0, g0 = res[False]
    l1, g1 = res[True]
    assert abs(l1 - l0) <= 1e-4 * abs(l0) + 1e-7, (l1, l0)
    for N in g0:
        for a, b_, nm in ((g1[N][0], g0[N][0], "dS"), (g1[N][1], g0[N][1], "dSt")):
            assert a.shape == b_.shape
            err = float((a - b_).abs().max())
            assert err <= 1.5e-2 * float(b_.abs().max()) + 1e-12, f"{nm} N={N}: {err} vs {float(b_.abs().max())}"
    if not any(has):
        assert l1 == 0.0 and all(float(a.abs().max()) == 0.0 for a, _ in g1.values())


@pytest.mark.parametrize("B", [1, 2])
def test_text_encoders_paired_launches_bitwise(B):
    """sdlt_*_pair (strip GEMM, attention forward / backward, slab LayerNorm backward): the two SDXL text encoders issued in lockstep
    (ops.run_paired - layer i of the 768-wide / 12-head encoder in the launches of layer i of the 1280-wide / 20-head one, quick-GELU vs GELU,
    16- vs 32-column strips on fc1) give the bits of the one-after-the-other launches, forward and backward."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import bench as B_
    import sd_lora_trainer_amd.clip as CL
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import ops
    dev = torch.device("cuda", 0)
    rt = M.Runtime(dev, B)
    cfgs = [dict(vocab=600, width=768, layers=3, heads=12, mlp=3072, act="quick_gelu", proj=None),
            dict(vocab=600, width=1280, layers=5, heads=20, mlp=5120, act="gelu", proj=1280)]
    encs = []
    for i, c in enumerate(cfgs):
        sd = B_.make_clip_state(c, dev, seed=40 + i, n_new=3)
        encs.append(CL.ClipTextEncoder(rt, f"pe{i}", sd, heads=c["heads"], act=c["act"], mode="penultimate", with_projection=bool(c["proj"]), n_train=3))
        assert encs[-1].fused
    g = torch.Generator(device=dev).manual_seed(5)
    ids = [torch.randint(0, 600, (B, CL.T_TOKENS), generator=g, device=dev) for _ in encs]
    for t in ids:
        t[:, 1:4] = torch.arange(600, 603, device=dev)          # the trained rows
    pool = torch.arange(B, device=dev) * CL.TP + 7
    W = [c["width"] for c in cfgs]

    def run(paired):
        ctx = torch.zeros(B * CL.TP, sum(W), dtype=rt.act, device=dev)
        fw = [e.forward_steps(i_, B, hidden_out=ctx[:, o:o + w], pool_rows=pool) for e, i_, o, w in zip(encs, ids, (0, W[0]), W)]
        vals = ops.run_paired(fw, min) if paired else [CL._drain(f) for f in fw]
        pooled = vals[1][1].clone()
        gg = torch.Generator(device=dev).manual_seed(6)
        dctx = (torch.randn(B * CL.TP, sum(W), generator=gg, device=dev) * 0.1).to(rt.act)
        dctx.view(B, CL.TP, -1)[:, CL.T_TOKENS:] = 0
        dpool = (torch.randn(B, 1280, generator=gg, device=dev) * 0.1).to(rt.act)
        grads = [torch.zeros(3, w, device=dev) for w in W]
        bw = [e.backward_steps(dctx[:, o:o + w], dpool if e.with_projection else None, g_) for e, o, w, g_ in zip(encs, (0, W[0]), W, grads)]
        if paired:
            ops.run_paired(bw, max)
        else:
            [CL._drain(b) for b in bw]
        torch.cuda.synchronize()
        return ctx.clone(), pooled, [g_.clone() for g_ in grads]

    ref = run(False)
    got = run(True)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    for a, b in zip(ref[2], got[2]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # and the launch count: every op of the shorter encoder rode along
    with ops.pairing() as pq:
        pass
    fw = [e.forward_steps(i_, B, hidden_out=torch.zeros(B * CL.TP, w, dtype=rt.act, device=dev), pool_rows=pool) for e, i_, w in zip(encs, ids, W)]
    n0 = _count_paired(ops, fw, min)
    assert n0 == 5 * max(e.n_run for e in encs), n0


def _count_paired(ops, gens, prefer):
    """Launches ops.run_paired issues for two chains (pairable ops only)."""
    orig = ops._PairQueue.launch
    n = [0]

    def counting(self, recs):
        n[0] += 1 if (len(recs) == 2 and recs[0][0] == recs[1][0] and ops._pair_ok(ops._lib.load(), recs[0], recs[1])) else len(recs)
        return orig(self, recs)
    ops._PairQueue.launch = counting
    try:
        ops.run_paired(gens, prefer)
    finally:
        ops._PairQueue.launch = orig
    return n[0]


@pytest.mark.parametrize("env,select", [(dict(SDLT_XATTN_ROLES="0"), "test_attention_fwd_bwd"), (dict(SDLT_XATTN_ROLES="0", SDLT_XATTN_FIVE="0"), "test_attention_fwd_bwd"),
                                        (dict(SDLT_ATTN_XCD="0", SDLT_ATTN_KS="1", SDLT_ATTN_R32="0"), "test_attention_fwd_bwd"),
                                        (dict(SDLT_ATTN32_KS_FWD="4", SDLT_ATTN32_KS_BWD="4"), "test_attention_fwd_bwd"),
                                        (dict(SDLT_ATTN32_KS_FWD="1", SDLT_ATTN32_KS_BWD="1"), "test_attention_fwd_bwd"),
                                        (dict(SDLT_WSK_STAGGER="0", SDLT_STRIP_WIDE_MIN="4096"), "test_wsk or test_strip"),
                                        (dict(SDLT_LN_FOLD="7", SDLT_LN_FOLD_WIDTH="64", SDLT_LN_PARTS="0"), "file:test_ti_step_gpu.py:trajectory or step"),
                                        (dict(SDLT_LN_FOLD="0"), "file:test_ti_step_gpu.py:trajectory or step"),
                                        # the same attention switch sets on the bit-exact file (tests/test_attn_exact_gpu.py: under switches it takes the planner's route as it comes)
                                        (dict(SDLT_XATTN_ROLES="0"), "file:test_attn_exact_gpu.py:test_"),
                                        (dict(SDLT_XATTN_ROLES="0", SDLT_XATTN_FIVE="0"), "file:test_attn_exact_gpu.py:test_"),
                                        (dict(SDLT_ATTN_XCD="0", SDLT_ATTN_KS="1", SDLT_ATTN_R32="0"), "file:test_attn_exact_gpu.py:test_"),
                                        (dict(SDLT_ATTN32_KS_FWD="4", SDLT_ATTN32_KS_BWD="4"), "file:test_attn_exact_gpu.py:test_"),
                                        (dict(SDLT_ATTN32_KS_FWD="1", SDLT_ATTN32_KS_BWD="1"), "file:test_attn_exact_gpu.py:test_"),
                                        # the bit-exact wave-split-K / row-strip file: unstaggered refills, N = 2304 on the 16-column strips
                                        (dict(SDLT_WSK_STAGGER="0", SDLT_STRIP_WIDE_MIN="4096"), "file:test_wsk_exact_gpu.py:test_")],
                         ids=["single-role", "single-role-128-keys", "plain-order-unsplit-16-rows", "attn32-four-groups", "attn32-one-group", "unstaggered-narrow-strips",
                              "layernorm-fold-every-width-k-walk-statistics", "layernorm-launches", "exact-single-role", "exact-single-role-128-keys",
                              "exact-plain-order-unsplit-16-rows", "exact-attn32-four-groups", "exact-attn32-one-group", "exact-unstaggered-narrow-strips"])
def test_fallback_kernel_paths_in_a_subprocess(env, select):
    """The A/B switches are read once per process, so the non-default kernels behind them (single-role / 128-key cross-attention backward,
    plain workgroup order, unsplit attention forward, unstaggered wave-split-K refills, 16-column strips; step level: the LayerNorm fold at every
    width with K-walk statistics / the LayerNorm launches) run in a child pytest: the same checks must pass on them too."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    target = "test_kernels_gpu.py"
    if select.startswith("file:"):          # "file:<test file>:<-k expression>": a step-level switch checked by that file's tests
        _, target, select = select.split(":", 2)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", target), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", f"({select}) and not subprocess"],       # (never this test itself: a child that selects it spawns children for ever)
                       env=e, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
