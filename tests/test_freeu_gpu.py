"""FreeU on the MI355X: the sdlt_freeu kernel against the fp64 torch.fft restatement (tests/freeu_ref.py) under a derived bound, its determinism and
batch independence, neutral parameters, its argument checks; then LatentSampler.sample(freeu=) end to end on the tiny topologies - graph against fused
eager bit for bit, neutral against none, the oracle sampler loop with FreeU at the bars of tests/test_sampler_gpu.py - and a two-pass hires case."""
import functools

import pytest
import torch

from tests import freeu_ref as FR
from tests.test_img2img_gpu import _cuda, _inputs, _setup
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop, without FreeU

pytestmark = pytest.mark.gpu

SENT = -7.25
B_, S_ = 1.4, 0.2
# (H, W, C1, C2, extra leading dimension): each the smallest shape with its reason
SHAPES = {
    "min-2x2": (2, 2, 8, 8, 0),              # the minimum size: one lane group, four rows, the Nyquist bin is the -1 bin
    "odd-3x5": (3, 5, 16, 24, 0),            # odd sizes; 15 rows in a 32-row chunk, 2 and 3 of 8 column lanes in use; C1 / 2 = 8
    "tiny-8x8": (8, 8, 128, 64, 0),          # the tiny models' stage: two chunks, two column tiles of the backbone
    "chunks-64x64": (64, 64, 64, 72, 0),     # 16 chunks of 256 rows (8 trips per row lane); 72 channels: a second column tile with one lane group
    "strided-16x16": (16, 16, 40, 24, 16),   # views with ld > C; C1 / 2 = 20 splits an 8-channel group
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (h, skip) bf16 [4 HW, C] on the CPU and {version: (h', skip') fp64} of B = 4 images; the B = 2 runs take the first two.  Normal data plus a
    per-pixel offset from U(-1, 1), rounded to bf16.  Computed once and shared."""
    H, W, C1, C2, _ = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    off = torch.rand(4 * H * W, 1, generator=g) * 2 - 1
    off.view(4, H * W)[:, 0], off.view(4, H * W)[:, -1] = -1.0, 1.0                # the ends of the offset's range are present in every image
    h = (torch.randn(4 * H * W, C1, generator=g) + off).to(torch.bfloat16)
    skip = (torch.randn(4 * H * W, C2, generator=g) + off).to(torch.bfloat16)
    m = h.double().mean(1).view(4, H * W)
    span = m.amax(1) - m.amin(1)
    assert bool((span >= 0.5).all()), (name, span)                  # version 2's normalisation is well conditioned by construction
    want = {v: FR.freeu_rows(h, skip, 4, H, W, B_, S_, v) for v in (1, 2)}
    return h, skip, want, span


def _run(name, version, B, b=B_, s=S_):
    """ops.freeu on the first B images, into sentinel-filled buffers with a tail -> (h', skip') on the CPU; the sentinels are checked here."""
    from sd_lora_trainer_amd import ops
    H, W, C1, C2, pad = SHAPES[name]
    h, skip, _, _ = _case(name)
    rows = B * H * W

    def dev(t, C):
        buf = torch.full((rows * (C + pad) + 64,), SENT, dtype=torch.bfloat16, device="cuda")
        v = buf[: rows * (C + pad)].view(rows, C + pad)[:, :C]
        if t is not None:
            v.copy_(t[:rows])
        return buf, v

    (_, hv), (_, sv), (hb, ho), (sb, so) = dev(h, C1), dev(skip, C2), dev(None, C1), dev(None, C2)
    tabs = ops.freeu_tables(H, W, "cuda")
    n = ops.freeu_ws_floats(B, H, W, C1, C2)
    ws = torch.full((n + 64,), SENT, device="cuda")
    ops.freeu(hv, sv, ho, so, tabs, ws[:n], B=B, H=H, W=W, b=b, s=s, version=version)
    torch.cuda.synchronize()
    for buf, C in ((hb, C1), (sb, C2)):
        assert bool((buf[rows * (C + pad):] == SENT).all()), "wrote past the end"
        if pad:
            assert bool((buf[: rows * (C + pad)].view(rows, C + pad)[:, C:] == SENT).all()), "wrote between the rows of a strided view"
    assert bool((ws[n:] == SENT).all())
    return ho.cpu(), so.cpu()


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_freeu_kernel(name, version):
    """The bound, per element, with u = 2^-24 (fp32) and the fp64 torch.fft restatement as `want`:
      one rounding to bf16 at the store                 2^-8 |want|        (8 significant bits: half an ulp is at most 2^-8 of the value)
      skip: seven fp32 sums of HW terms each, divided by HW, combined with |weights| <= 1: each sum carries at most HW u max|x| after the division,
            the table entries and the angle-sum products a few u more                                   8 HW u |s - 1| max|x|
      h, version 1: one fp32 product (u) by b as fp32 holds it (u / 2), and their second-order terms     2 u |want|
      h, version 2: the factor (b - 1) n + 1; m, lo, hi are fp32 sums of C1 terms (error <= C1 u max|h| each before the division by C1 ... taken
            without it: an upper bound), n = (m - lo) / (hi - lo) moves by at most 4 of those over (hi - lo), plus a few u of its own arithmetic
                                                                                                        |b - 1| |h| (4 C1 u max|h| / (hi - lo) + 8 u)
    Then: image j of B = 2 and of B = 4 has the same bits; a second run has the same bits; neutral parameters return the input's bits."""
    H, W, C1, C2, _ = SHAPES[name]
    h, skip, want, span = _case(name)
    u, HW = 2.0 ** -24, H * W
    got4 = _run(name, version, 4)
    hw, sw = want[version]
    hd, sd_ = h.double(), skip.double()
    bound_s = 2.0 ** -8 * sw.abs() + 8 * HW * u * abs(S_ - 1) * float(sd_.abs().max())
    if version == 1:
        bound_h = (2.0 ** -8 + 2 * u) * hw.abs()
    else:
        per_img = (4 * C1 * u * float(hd.abs().max()) / span + 8 * u).repeat_interleave(HW)[:, None]
        bound_h = 2.0 ** -8 * hw.abs() + abs(B_ - 1) * hd.abs() * per_img
    eh, es = (got4[0].double() - hw).abs(), (got4[1].double() - sw).abs()
    print(f"{name} v{version}: skip worst err/bound {float((es / bound_s.clamp_min(1e-300)).max()):.3f}, h worst err/bound {float((eh / bound_h.clamp_min(1e-300)).max()):.3f}; "
          f"max err skip {float(es.max()):.3e} h {float(eh.max()):.3e}")
    assert bool((es <= bound_s).all()), (name, version, float((es - bound_s).max()))
    assert bool((eh <= bound_h).all()), (name, version, float((eh - bound_h).max()))
    assert torch.equal(got4[0][:, C1 // 2:], h[:, C1 // 2:])                       # the second half of the backbone: the input's bits
    assert not torch.equal(got4[0][:, : C1 // 2], h[:, : C1 // 2]) and not torch.equal(got4[1], skip)
    got2 = _run(name, version, 2)
    for a, b4 in zip(got2, got4):
        assert torch.equal(a.view(torch.int16), b4[: 2 * HW].view(torch.int16)), "image j depends on the batch it is in"
    for a, b4 in zip(_run(name, version, 4), got4):
        assert torch.equal(a.view(torch.int16), b4.view(torch.int16)), "two runs differ"
    n1, n2 = _run(name, version, 2, b=1.0, s=1.0)
    assert torch.equal(n1.view(torch.int16), h[: 2 * HW].view(torch.int16)) and torch.equal(n2.view(torch.int16), skip[: 2 * HW].view(torch.int16))
    m1, m2 = _run(name, version, 2, b=1.0)                                         # one neutral, one not
    assert torch.equal(m1.view(torch.int16), h[: 2 * HW].view(torch.int16)) and torch.equal(m2.view(torch.int16), got2[1].view(torch.int16))


def test_freeu_negative_zero_and_flat_mean():
    """-0 survives neutral parameters (copied, not x + 0 L); an image whose channel mean is the same at every pixel takes n = 0 in version 2: the
    backbone comes back unchanged, finite."""
    from sd_lora_trainer_amd import ops
    H = W = 4
    h = torch.zeros(2 * 16, 16, dtype=torch.bfloat16, device="cuda")
    h[:, 0::2], h[:, 1::2] = 0.5, -0.5                                            # every row's mean is exactly 0
    skip = -torch.zeros(2 * 16, 8, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ops.freeu_ws_floats(2, H, W, 16, 8), device="cuda")
    tabs = ops.freeu_tables(H, W, "cuda")
    ho, so = ops.freeu(h, skip, torch.empty_like(h), torch.empty_like(skip), tabs, ws, B=2, H=H, W=W, b=1.4, s=1.0, version=2)
    assert torch.equal(so.view(torch.int16), skip.view(torch.int16)) and bool((so.view(torch.int16) == -32768).all())
    assert torch.equal(ho, h)


def test_freeu_errors_launch_nothing():
    from sd_lora_trainer_amd import _lib, ops
    H, W, C1, C2 = 3, 5, 16, 24
    rows = 2 * H * W
    h, skip = torch.randn(rows, C1, device="cuda").bfloat16(), torch.randn(rows, C2, device="cuda").bfloat16()
    ho, so = torch.full_like(h, SENT), torch.full_like(skip, SENT)
    wide = torch.full((rows, 32), SENT, dtype=torch.bfloat16, device="cuda")
    tabs, ws = ops.freeu_tables(H, W, "cuda"), torch.empty(ops.freeu_ws_floats(2, H, W, C1, C2), device="cuda")
    ok = dict(h=h, skip=skip, h_out=ho, skip_out=so, tabs=tabs, ws=ws, B=2, H=H, W=W, b=B_, s=S_, version=1)
    h0, s0 = h.clone(), skip.clone()
    for change in (dict(version=0), dict(version=3), dict(h_out=h), dict(skip_out=skip), dict(h_out=skip[:, :C1]), dict(ws=ws[:50]),
                   dict(h=wide[:, 4:20]),                                          # 8-byte aligned only
                   dict(h=wide[:, :12], h_out=torch.full((rows, 12), SENT, dtype=torch.bfloat16, device="cuda")),      # C1 = 12
                   dict(h=h[: 2 * W], skip=skip[: 2 * W], h_out=ho[: 2 * W], skip_out=so[: 2 * W], H=1, tabs=ops.freeu_tables(1, W, "cuda"))):      # an axis of size 1
        kw = dict(ok, **change)
        args = [kw.pop(k) for k in ("h", "skip", "h_out", "skip_out", "tabs", "ws")]
        with pytest.raises(_lib.KernelLibraryError, match="sdlt_freeu"):
            ops.freeu(*args, **kw)
    with pytest.raises(_lib.KernelLibraryError, match="sdlt_freeu"):
        ops.freeu_ws_floats(2, 1, 5, C1, C2)
    with pytest.raises(AssertionError):
        ops.freeu(h, skip, ho[:-1], so, tabs, ws, B=2, H=H, W=W, b=B_, s=S_)
    with pytest.raises(AssertionError):
        ops.freeu(h.float(), skip, ho, so, tabs, ws, B=2, H=H, W=W, b=B_, s=S_)
    torch.cuda.synchronize()
    assert bool((ho == SENT).all()) and bool((so == SENT).all()) and torch.equal(h, h0) and torch.equal(skip, s0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
FZ = (1.3, 1.4, 0.9, 0.2)


def _metric(got, ref):
    a, b = got.reshape(-1).double(), ref.reshape(-1).double()
    return float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


@pytest.mark.parametrize("fver", [1, 2])
@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_with_freeu(version, fver):
    """8 x 8 latent, 3 steps: up_blocks.0 runs at 2 x 2 and up_blocks.1 at 4 x 4.  Against the oracle sampler loop with FreeU (freeu_ref) at the bars
    tests/test_sampler_gpu.py holds these models to without it.  Measured on the MI355X with these inputs (cos / relative L2), first without FreeU - the
    launch sequence from before FreeU existed - then with it: tiny15 0.999437 / 0.0336 -> version 1 0.999442 / 0.0336, version 2 0.999433 / 0.0337;
    tinyxl 0.999353 / 0.0363 -> version 1 0.999383 / 0.0353, version 2 0.999172 / 0.0422.  None is beyond twice its no-FreeU error."""
    h = w = 8
    steps = 3
    cfg, sd, lora, smp = _setup(version)
    embeds, noise, _ = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    fz = dict(zip(("b1", "b2", "s1", "s2"), FZ), version=fver)
    kw = dict(steps=steps, guidance_scale=8.0, latents=noise.cuda())
    plain = smp.sample(em, h, w, fused=True, **kw).cpu()
    fused = smp.sample(em, h, w, fused=True, freeu=fz, **kw).cpu()
    graph = smp.sample(em, h, w, graph=True, freeu=fz, **kw).cpu()
    assert torch.isfinite(fused).all()
    assert torch.equal(graph, fused)                                               # graph == fused eager, bit for bit, with FreeU on
    assert not torch.equal(fused, plain)
    neutral = dict(b1=1, b2=1, s1=1, s2=1, version=fver)
    assert torch.equal(smp.sample(em, h, w, fused=True, freeu=neutral, **kw).cpu(), plain)
    assert torch.equal(smp.sample(em, h, w, graph=True, freeu=neutral, **kw).cpu(), smp.sample(em, h, w, graph=True, **kw).cpu())
    # another setting is another capture, never a stale replay; the first one is still there
    other = smp.sample(em, h, w, graph=True, freeu=dict(fz, s2=0.6), **kw).cpu()
    assert not torch.equal(other, graph) and torch.equal(smp.sample(em, h, w, graph=True, freeu=fz, **kw).cpu(), graph)
    assert len(smp._graphs) == 4                                                   # fz, neutral, none, other
    assert torch.equal(smp.sample(em, h, w, fused=True, **kw).cpu(), plain)        # freeu=None afterwards: the plain launch sequence again
    # the torch loop runs the same forward: it follows the fused path as closely with FreeU as without
    loop, loop_plain = smp.sample(em, h, w, freeu=fz, **kw).cpu(), smp.sample(em, h, w, **kw).cpu()
    print(f"{version} v{fver}: torch loop vs fused, rel: with FreeU {_metric(loop, fused)[1]:.3e}, without {_metric(loop_plain, plain)[1]:.3e}")
    assert _metric(loop, fused)[1] <= 1e-3 and not torch.equal(loop, loop_plain)
    ref = FR.sample_latents_freeu(cfg, sd, lora, 0.75, embeds[0], noise, steps, freeu=fz)
    ref_plain = FR.sample_latents_freeu(cfg, sd, lora, 0.75, embeds[0], noise, steps, freeu=None)
    (cos0, rel0), (cos1, rel1) = _metric(plain, ref_plain), _metric(fused, ref)
    print(f"{version} v{fver}: without FreeU cos {cos0:.6f} rel {rel0:.4f}; with FreeU cos {cos1:.6f} rel {rel1:.4f} (bars {TOL_COS} / {TOL_REL}); "
          f"FreeU moves the latents by rel {_metric(fused, plain)[1]:.3f}")
    assert cos0 >= TOL_COS and rel0 <= TOL_REL, (version, cos0, rel0)
    assert cos1 >= TOL_COS and rel1 <= TOL_REL, (version, fver, cos1, rel1)


@pytest.mark.parametrize("sampler,img", [("dpmpp_2m", False), ("euler_a", False), ("dpmpp_2m_sde", True), ("euler", True)])
def test_every_family_takes_freeu(sampler, img):
    """The other step launches, from init latents with a mask too: graph == fused bit for bit with FreeU, and different from the run without."""
    h = w = 8
    cfg, sd, lora, smp = _setup("tiny15")
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    em = _cuda(embeds)[0]
    kw = dict(steps=4, guidance_scale=8.0, latents=noise.cuda(), sampler=sampler)
    if sampler in ("euler_a", "dpmpp_2m_sde"):
        kw.update(seeds=[7])
    if img:
        mask = torch.ones(1, 1, h, w)
        mask[..., : w // 2] = 0
        kw.update(init_latents=x0.cuda(), strength=0.75, mask=mask.cuda())
    fused = smp.sample(em, h, w, fused=True, freeu=FZ, **kw).cpu()
    assert torch.isfinite(fused).all()
    assert torch.equal(smp.sample(em, h, w, graph=True, freeu=FZ, **kw).cpu(), fused)
    assert not torch.equal(smp.sample(em, h, w, graph=True, **kw).cpu(), fused)
    if img:
        assert torch.equal(fused[..., : w // 2], x0[..., : w // 2])              # the kept half is still the init latents


def test_hires_runs_freeu_in_both_passes():
    """8 x 8 -> 12 x 12: the second pass (its own UNet instance, as render() rebuilds it) runs FreeU at 3 x 3 and 6 x 6 - odd planes."""
    from sd_lora_trainer_amd import ops
    from sd_lora_trainer_amd import sampler as SM
    cfg, sd, lora, smp1 = _setup("tinyxl")
    _, _, _, smp2 = _setup("tinyxl")
    embeds, noise1, _ = _inputs(cfg, 5, 8, 8, 1)
    noise2 = torch.randn(1, 4, 12, 12, generator=torch.Generator().manual_seed(6))
    em = _cuda(embeds)[0]
    kw1 = dict(steps=3, guidance_scale=8.0, latents=noise1.cuda(), fused=True, size=(64, 64))
    first, first_plain = smp1.sample(em, 8, 8, freeu=FZ, **kw1), smp1.sample(em, 8, 8, **kw1)
    assert not torch.equal(first, first_plain)
    x0 = SM.upscale_latents(ops, first, 12, 12, "bilinear")
    kw2 = dict(steps=4, guidance_scale=8.0, latents=noise2.cuda(), init_latents=x0, strength=0.5, size=(96, 96))
    second = smp2.sample(em, 12, 12, fused=True, freeu=FZ, **kw2).cpu()
    assert torch.isfinite(second).all()
    assert torch.equal(smp2.sample(em, 12, 12, graph=True, freeu=FZ, **kw2).cpu(), second)
    assert not torch.equal(smp2.sample(em, 12, 12, fused=True, **kw2).cpu(), second)
    ref = FR.IR.sample_latents  # the fp32 reference loop of img2img, with the oracle's FreeU inside
    with FR.oracle_freeu(cfg, FZ):
        want = ref(cfg, sd, lora, 0.75, embeds[0], noise2, 4, init_latents=x0.cpu(), strength=0.5, guidance_scale=8.0, size=(96, 96))
    cos, rel = _metric(second, want)
    print(f"hires second pass with FreeU: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (cos, rel)
