"""Self-attention guidance on the GPU: ops.attn_colmass, ops.sag_degrade and ops.sag_apply against tests/sag_ref.py (fp64), and
LatentSampler.sample(sag=) on the toy topology - graph replay against the eager fused loop, one capture for every setting, the plain path untouched."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sd_lora_trainer_amd import ops, sampler as SM  # noqa: E402
from tests import sag_ref as SR  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []      # the lines of profiles/sag_report.txt of this session: the file is rewritten whole, never appended to


def _stab(rows):
    t = torch.zeros(1 + len(rows), 4)
    t[0, 0] = len(rows)
    t[1:, :3] = torch.tensor(rows)
    return t.to(DEV)


@pytest.mark.parametrize("H,d", [(1, 8), (3, 64), (2, 160)])
@pytest.mark.parametrize("N", [4, 64, 70, 200])
def test_attn_colmass(N, H, d):
    """Bar: 4 x the worst error of a plain fp32 torch evaluation of the same formula against fp64 on the same inputs (the margin covers the MFMA's
    summation order); each image's mean mass is 1 within it; two runs give the same bits; the NaN rows 1 and 3 are never read."""
    B, rows, g = 4, [0, 2], torch.Generator().manual_seed(1000 * N + d)
    ld = H * d + 8
    Q, K = (torch.randn(B * N, ld, generator=g).mul(1.5).bfloat16() for _ in range(2))
    scale = d ** -0.5
    s = scale * torch.einsum("bqhd,bkhd->bhqk", Q[:, :H * d].double().view(B, N, H, d), K[:, :H * d].double().view(B, N, H, d))
    L = torch.logsumexp(s, -1).float()                      # sdlt_attn_fwd's convention: natural log, the scale inside, rounded to fp32
    ref = SR.colmass(Q, K, L, B=B, H=H, N=N, d=d, scale=scale, rows=rows)
    bar = 4.0 * float((SR.colmass(Q, K, L, B=B, H=H, N=N, d=d, scale=scale, rows=rows, dtype=torch.float32).double() - ref).abs().max())
    Qd, Kd, Ld = Q.to(DEV), K.to(DEV), L.to(DEV)
    for t in (Qd, Kd, Ld):
        t.view(B, -1)[1::2] = float("nan")
    run = lambda: ops.attn_colmass(Qd, Kd, Ld, torch.full((2, N), -7.0, device=DEV), B=B, H=H, N=N, d=d, scale=scale, n=2, row_off=0, row_stride=2)  # noqa: E731
    out = run()
    err = float((out.double().cpu() - ref).abs().max())
    print(f"colmass N={N} H={H} d={d}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    REPORT.append(f"attn_colmass N={N} H={H} d={d}: max |err| {err:.3e}, bar (4 x fp32 torch) {bar:.3e}, ratio {err / bar:.3f}\n")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sag_report.txt"), "w") as f:
        f.writelines(REPORT)
    assert err <= bar
    assert float((out.double().mean(1) - 1.0).abs().max()) <= bar
    assert torch.equal(out, run())


@pytest.mark.parametrize("h,w,grid", [(5, 5, (2, 3)), (8, 12, (4, 4)), (33, 20, (2, 3)), (33, 20, (4, 4))])
def test_sag_degrade(h, w, grid):
    n, T, g = 3, 1.0, torch.Generator().manual_seed(h * 100 + w)
    x, eps = torch.randn(n, 4, h, w, generator=g) * 3.0, torch.randn(2 * n * h * w, 4, generator=g)
    eps.view(n, 2, -1)[:, 1] = float("nan")                # the positive rows are not read
    mass = T + (0.05 + torch.rand(n, grid[0] * grid[1], generator=g)) * (torch.randint(0, 2, (n, grid[0] * grid[1]), generator=g) * 2 - 1)
    mass[0], mass[1] = mass[0].abs() + T + 0.05, T - 0.05 - (mass[1] - T).abs()      # image 0: blurred everywhere, image 1: nowhere
    taps, stab, ctr = ops.blur_taps(2.0, 4), _stab([(3.7, 0.5, T), (0.9, 0.5, T)]), torch.zeros(2, dtype=torch.int32, device=DEV)
    outs = []
    for row in (0, 1):
        ctr[0] = row
        out = torch.full((n * h * w, 16), 9.0, dtype=torch.bfloat16, device=DEV)
        ops.sag_degrade(x.to(DEV), eps.to(DEV), mass.to(DEV), taps.to(DEV), stab, ctr, out, grid=grid)
        ref = SR.degrade(x, eps, mass, taps, stab[1 + row].cpu(), grid)
        err = (out[:, :4].double().cpu() - ref).abs()
        print(f"degrade {h}x{w} grid {grid} row {row}: worst err / bound {float((err / (2.0 ** -7 * ref.abs() + 1e-6)).max()):.3f}")
        assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-6).all()) and bool((out[:, 4:] == 9.0).all())
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])


def test_sag_apply():
    n, hw, g = 3, 37, torch.Generator().manual_seed(3)
    eps, t = torch.randn(2 * n * hw, 4, generator=g), torch.randn(n * hw, 4, generator=g)
    stab, ctr = _stab([(1.0, 0.25, 1.0), (1.0, 0.75, 1.0)]), torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ed, td = eps.to(DEV), t.to(DEV)
    ops.sag_apply(ed, td, stab, ctr, n, 0)
    t1 = SR.apply(eps, t, 0.75, n, 0)
    assert torch.equal(ed.cpu(), eps) and torch.allclose(td.double().cpu(), t1, rtol=1e-6, atol=0)
    ops.sag_apply(ed[: 4 * hw], td[: 2 * hw], stab, ctr, 2, 1)      # two images: the third's rows stay
    ref = SR.apply(eps[: 4 * hw], td[: 2 * hw].cpu(), None, 2, 1)
    assert torch.allclose(ed[: 4 * hw].double().cpu(), ref, rtol=1e-6, atol=0) and torch.equal(ed[4 * hw:].cpu(), eps[4 * hw:])


def test_sampler_graph_equals_eager_and_one_capture_serves_every_setting():
    from tests.test_render_gpu import TOL_COS, TOL_REL, _cuda, _embeds, _setup
    h = w = 8                                              # the smallest latent the toy's downsampling and the reflection allow: a 2 x 2 mid grid
    cfg, _, _, smp = _setup("tinyxl", n=2)
    embeds, noise = _embeds(cfg, 5, h, w, 2)
    em, noise = _cuda(embeds), noise.to(DEV)
    run = lambda **kw: smp.sample(em, h, w, steps=3, latents=noise.clone(), n_images=2, **kw)  # noqa: E731
    plain = run(graph=True)
    eager, graph = run(fused=True, sag=True), run(graph=True, sag=True)
    assert torch.equal(eager, graph) and bool(torch.isfinite(graph).all()) and not torch.equal(graph, plain)
    assert len(smp._sag_graphs) == 1
    other = run(graph=True, sag=(0.9, 1.5, 0.8))
    assert len(smp._sag_graphs) == 1 and not torch.equal(other, graph) and torch.equal(other, run(fused=True, sag=(0.9, 1.5, 0.8)))
    assert torch.equal(run(graph=True), plain) and torch.equal(run(fused=True), plain)
    # the second forward is the first one's network on the negative rows: the mass of a real forward has mean 1 (L in sdlt_attn_fwd's convention: a wrong base
    # or scale moves it by factors), the clone's context is the negative prompts, and the clone at batch n gives what the parent plan gives at batch 2 n on
    # the same input - within the project's bars for two bf16 evaluations of this network (tests/test_render_gpu.py), far below a wrong row's O(1)
    ss, n = smp._fused["shapes"][(h, w)]["sag"], 2
    assert float((ss["mass"].double().mean(1) - 1.0).abs().max()) <= 1e-4      # 4 keys, fp32 sums of fp32 exponentials of an fp32 L
    assert torch.equal(ss["ctx"].view(n, -1, cfg["cross_dim"])[:, :77], torch.cat([e[1] for e in em]).to(ss["ctx"].dtype))
    (clone,), st = smp._unet_sag.values(), smp._fused
    x2 = ss["x64"].view(n, 1, h * w, 64).expand(n, 2, h * w, 64).reshape(2 * n * h * w, 64).contiguous()
    tid = st["tid"] if cfg["addition"] else None
    a = clone.forward(ss["x64"], st["tf"][:n], ss["ctx"], ss["pooled"], None if tid is None else tid[: 6 * n], B=n, H=h, W=w, train=False).double().reshape(-1)
    b = smp.unet.forward(x2, st["tf"], smp.ctx, smp.pooled, tid, B=2 * n, H=h, W=w, train=False).view(n, 2, -1)[:, 0].double().reshape(-1)
    cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    print(f"clone at batch n against the parent plan at 2 n: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL
    # a UNet setting toggled across calls reaches both forwards: the bits of a fresh sampler that never ran without it
    freeu = (1.2, 1.4, 0.9, 0.2)
    with_freeu = run(graph=True, sag=True, freeu=freeu)
    _, _, _, fresh = _setup("tinyxl", n=2)
    assert torch.equal(with_freeu, fresh.sample(em, h, w, steps=3, latents=noise.clone(), n_images=2, graph=True, sag=True, freeu=freeu))
    assert not torch.equal(with_freeu, graph) and len(smp._unet_sag) == 2 and torch.equal(run(graph=True, sag=True), graph)
