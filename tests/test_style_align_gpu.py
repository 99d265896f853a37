"""Style-aligned batches on the GPU: ops.attn_shared_fwd and ops.adain_affine (csrc/attn_shared.hip) against tests/style_align_ref.py (fp64),
UNet.set_shared_attention against the same UNet on torch AdaIN -> cat -> ops.attn_fwd, and the sampler."""
import math

import pytest
import torch

from tests import style_align_ref as SR

pytestmark = pytest.mark.gpu
BF16, F32, DEV = torch.bfloat16, torch.float32, "cuda"

# (N, H, d, B, G, gs, weight, adain, sharp): N = 24 one partial block, 80 two blocks with a ragged tail (the segment switch lands on the other LDS buffer), 144, 256;
# every head-width instantiation (64: d = 8, 40, 64; 96: 80; 128; 160); G = 1 is plain attention; gs = 2: the interleaved groups of a guided batch
CASES = [(24, 2, 8, 2, 1, 1, 1.0, True, 1), (24, 2, 64, 4, 2, 1, 1.0, False, 1), (80, 2, 64, 4, 2, 1, 0.25, True, 1), (80, 1, 40, 6, 3, 1, 4.0, True, 1),
         (144, 2, 80, 4, 2, 1, 1.0, True, 1), (144, 1, 160, 4, 2, 1, 4.0, False, 1), (256, 2, 64, 4, 2, 1, 1.0, True, 4), (256, 1, 160, 6, 3, 1, 0.25, True, 1),
         (80, 1, 128, 4, 2, 1, 1.0, True, 1), (80, 2, 64, 4, 2, 2, 4.0, True, 1), (144, 1, 64, 2, 1, 1, 1.0, False, 1)]


@pytest.mark.parametrize("N,H,d,B,G,gs,weight,adain,sharp", CASES)
def test_attn_shared_matches_fp64(N, H, d, B, G, gs, weight, adain, sharp):
    # Q, K, V are column views of one [M, 3 C] buffer, every image with its own mean and spread; the tables are ops.adain_affine's own (fp32), given to the
    # kernel and to the reference alike.  Bar: the bf16-P flash bar; with AdaIN + 2 x the error of an fp32 emulation that rounds q' and k' to bf16 (the kernel
    # rounds q' o Ak where the emulation rounds k': another rounding of the same size).  Measured fractions: DESIGN 4.42.
    from sd_lora_trainer_amd import ops
    C, M, scale, shift = H * d, B * N, sharp / math.sqrt(d), math.log(weight)
    g = torch.Generator().manual_seed(1000 * N + d + G)
    x = torch.randn(B, N, 3 * C, generator=g) * (1 + 0.5 * torch.arange(B).view(B, 1, 1)) + 0.5 * torch.arange(B).view(B, 1, 1)
    qkv = x.view(M, 3 * C).to(BF16).to(DEV)
    tabs = None
    if adain:
        A, S = torch.empty(B, 2 * C, device=DEV), torch.empty(B, 2 * C, device=DEV)
        ops.adain_affine(qkv[:, :2 * C], A, S, B=B, N=N, G=G, gs=gs)
        tabs = (A[:, :C], S[:, :C], A[:, C:], S[:, C:])
    cpu = lambda ts: None if ts is None else tuple(t.cpu() for t in ts)  # noqa: E731
    kw = dict(B=B, H=H, N=N, d=d, G=G, gs=gs, scale=scale, shift=shift)
    q, k, v = (qkv.cpu()[:, i * C:(i + 1) * C] for i in range(3))
    ref = SR.attn_shared(q, k, v, tables=cpu(tabs), **kw)
    bar = 1.5e-2 * float(ref.abs().max()) + 1e-6
    if adain:
        emu = SR.attn_shared(q, k, v, tables=cpu(tabs), dtype=F32, round_qk=lambda t: t.to(BF16).to(F32), **kw)
        bar += 2.0 * float((emu.double() - ref).abs().max())

    def run(qkv_):
        buf = torch.full((M + 8, C), 7.0, dtype=BF16, device=DEV)
        ops.attn_shared_fwd(qkv_[:, :C], qkv_[:, C:2 * C], qkv_[:, 2 * C:], buf[:M], tables=tabs, **kw)
        torch.cuda.synchronize()
        assert bool((buf[M:] == 7.0).all()), "rows beyond B N were written"
        return buf[:M].clone()
    out = run(qkv)
    assert torch.equal(out, run(qkv)), "two runs differ"
    err = float((out.double().cpu() - ref).abs().max())
    print(f"attn_shared N={N} H={H} d={d} B={B} G={G} gs={gs} w={weight} adain={adain} sharp={sharp}: max err {err:.3e} = {err / bar:.3f} of the bar {bar:.3e}")
    assert err <= bar
    if B // G > 1:      # NaN in the K and V rows of every picture outside image 0's group changes no bit inside it
        mine = torch.tensor([SR.reference_row(b, G, gs) == 0 for b in range(B)]).repeat_interleave(N).to(DEV)
        bad = qkv.clone()
        bad[~mine, C:] = float("nan")
        assert torch.equal(run(bad)[mine], out[mine])


@pytest.mark.parametrize("N,B,G,gs", [(2, 4, 2, 1), (24, 4, 2, 1), (1000, 4, 2, 1), (1000, 4, 2, 2), (300, 3, 3, 1)])
def test_adain_affine_matches_fp64(N, B, G, gs):
    # 72 columns of a wider buffer (two column blocks, the second partial), among them columns with mean 30 and deviation 0.5: a one-pass sum of squares
    # loses those.  Bar: 4 x the error of the same formula in fp32 torch + one fp32 ulp of the table's largest entry.
    from sd_lora_trainer_amd import ops
    C2, g = 72, torch.Generator().manual_seed(N + 7 * gs)
    x = torch.randn(B, N, C2 + 8, generator=g) * (1 + 0.5 * torch.arange(B).view(B, 1, 1)) + 0.5 * torch.arange(B).view(B, 1, 1)
    x[:, :, 5:C2:9] = 30.0 + 0.5 * torch.randn(B, N, len(range(5, C2, 9)), generator=g)
    X = x.view(B * N, C2 + 8).to(BF16)
    refs, lows = SR.adain_affine(X[:, :C2], B=B, N=N, G=G, gs=gs), SR.adain_affine(X[:, :C2], B=B, N=N, G=G, gs=gs, dtype=F32)
    Xd = X.to(DEV)

    def run():
        A, S = torch.full((B, C2), -7.0, device=DEV), torch.full((B, C2), -7.0, device=DEV)
        ops.adain_affine(Xd[:, :C2], A, S, B=B, N=N, G=G, gs=gs)
        return A.cpu(), S.cpu()
    got = run()
    assert all(torch.equal(a, b) for a, b in zip(got, run())), "two runs differ"
    own = torch.tensor([SR.reference_row(b, G, gs) == b for b in range(B)])
    assert bool((got[0][own] == 1.0).all()) and bool((got[1][own] == 0.0).all())
    for name, o, ref, low in zip("AS", got, refs, lows):
        err = float((o.double() - ref).abs().max())
        bar = 4.0 * float((low.double() - ref).abs().max()) + float(ref.abs().max()) * 2.0 ** -23
        print(f"adain_affine N={N} B={B} G={G} gs={gs} {name}: max err {err:.3e} = {err / bar:.3f} of the bar {bar:.3e}")
        assert err <= bar


def _emulated(q, k, v, O, *, B, H, N, d, G, scale, shift=0.0, tables=None, gs=1):
    """ops.attn_shared_fwd (weight 1) by the existing kernels: torch AdaIN, [own; reference] copies of K and V, ops.attn_fwd at Nk = 2 N (N for a reference)."""
    from sd_lora_trainer_amd import ops
    assert shift == 0.0 and N % 8 == 0
    C, f = H * d, lambda t: t[:, :H * d].float().view(B, N, H * d)
    qa, ka = f(q), f(k)
    if tables is not None:
        Aq, Sq, Ak, Sk = (t[:, :C].reshape(B, 1, C) for t in tables)
        qa, ka = Aq * qa + Sq, Ak * ka + Sk
    for b in range(B):
        r = SR.reference_row(b, G, gs)
        kk = ka[b] if r == b else torch.cat([ka[b], f(k)[r]])
        vv = f(v)[b] if r == b else torch.cat([f(v)[b], f(v)[r]])
        Nk, Ob = kk.shape[0], torch.empty(N, C, dtype=BF16, device=q.device)
        ops.attn_fwd(qa[b].to(BF16).contiguous(), kk.to(BF16).contiguous(), vv.to(BF16).contiguous(), None, Ob, torch.empty(H * N, dtype=F32, device=q.device),
                     B=1, H=H, Nq=N, Nk=Nk, Nqp=N, Nkp=Nk, d=d, scale=scale)
        O[b * N:(b + 1) * N, :C] = Ob
    return O


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_shared_attention(version, monkeypatch):
    # the emulation rounds k' where the kernel rounds q' o Ak: the bar is the kernel's, on the UNet output's range (tests/test_attn_window_gpu.py)
    from oracle import unet_ref as U
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import ops, topology
    B, h, cfg, g = 4, 16, U.CONFIGS[version], torch.Generator().manual_seed(11)
    x, tf = torch.randn(B, 4, h, h, generator=g), torch.tensor([500.0, 200.0, 500.0, 200.0]).cuda()
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    rt = M.Runtime("cuda:0", B)
    ctx = torch.zeros(B, M.CTX_PAD, cfg["cross_dim"], dtype=rt.act, device="cuda")
    ctx[:, :77] = torch.randn(B, 77, cfg["cross_dim"], generator=g).to(rt.act).cuda()
    extra = (torch.randn(B, P, generator=g).to(rt.act).cuda(), torch.tensor([128., 128, 0, 0, 128, 128]).repeat(B).cuda()) if P else ()
    unet = M.UNet(rt, topology.CONFIGS[version], U.init_unet_state(cfg, seed=0), lora_rank=4)
    unet.arena.load(U.init_lora(cfg, 4, seed=1, b_std=0.05))
    x64 = torch.nn.functional.pad(x.permute(0, 2, 3, 1).reshape(-1, 4), (0, 60)).to(rt.act).cuda()
    run = lambda: unet.forward(x64, tf, ctx.view(-1, ctx.shape[-1]), *extra, B=B, H=h, W=h, train=False).clone()  # noqa: E731
    plain = run()
    assert len(unet.set_shared_attention(dict(group=2, shift=0.0, adain=True))) >= 3
    got = run()
    emulated = []
    monkeypatch.setattr(ops, "attn_shared_fwd", lambda *a, **k: (emulated.append(k["N"]), _emulated(*a, **k))[1])
    want = run()
    monkeypatch.undo()
    assert len(emulated) >= 3
    err, bar = float((got - want).abs().max()), 1.5e-2 * float(want.abs().max()) + 1e-6
    rows = got.view(B, -1)
    print(f"unet shared attention {version}: max err {err:.3e} (bar {bar:.3e}); against the plain forward {float((got - plain).abs().max()):.3e}")
    assert err <= bar and float((rows[1::2] - plain.view(B, -1)[1::2]).abs().max()) > 0
    assert unet.set_shared_attention(None) == {} and torch.equal(run(), plain)


def test_sampler_style_align():
    # graph replay == eager bit for bit; the sharing has a direction: another noise and prompt for picture 1 moves picture 1 and no bit of picture 0; pictures
    # >= 1 leave the plain run, picture 0 stays within the kernel's bar of it after one step (its own keys only, by another kernel); nothing sticks
    from tests.test_render_gpu import _cuda, _embeds, _setup
    h = w = 8
    cfg, _, _, smp = _setup("tinyxl", n=2)
    embeds, noise = _embeds(cfg, 5, h, w, 2)
    em, noise = _cuda(embeds), noise.to(DEV)
    run = lambda em_=em, nz=noise, steps=3, **kw: smp.sample(em_, h, w, steps=steps, latents=nz.clone(), n_images=2, **kw)  # noqa: E731
    plain, sa = run(graph=True), dict(weight=1.0, adain=True)
    eager, graph = run(fused=True, style_align=sa), run(graph=True, style_align=sa)
    assert torch.equal(eager, graph) and bool(torch.isfinite(graph).all()) and torch.equal(run(graph=True, style_align=sa), graph)
    assert smp.unet._share is None and torch.equal(run(graph=True), plain)
    assert not torch.equal(graph[1], plain[1])
    noise2 = noise.clone()
    noise2[1] = noise[1].flip(-1)
    other = run([em[0], em[0]], noise2, graph=True, style_align=sa)
    assert torch.equal(other[0], graph[0]) and not torch.equal(other[1], graph[1])
    one, one_plain = run(steps=1, graph=True, style_align=sa), run(steps=1, graph=True)
    err, bar = float((one[0] - one_plain[0]).abs().max()), 1.5e-2 * float(one_plain.abs().max()) + 1e-6
    print(f"picture 0 after one step against the plain run: max err {err:.3e} (bar {bar:.3e})")
    assert err <= bar and not torch.equal(one[1], one_plain[1])
