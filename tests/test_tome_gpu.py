"""Token merging (csrc/tome.hip): sdlt_tome_match against the cosine similarity in float64 from the bf16-rounded inputs, sdlt_tome_plan against the tables
built from torch.sort(descending=True, stable=True), sdlt_tome_merge / sdlt_tome_unmerge against float64 at one bf16 rounding, UNet.set_token_merge against
the same UNet with plan / merge / unmerge emulated in torch, and the sampler / CLI."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, I32, F32 = torch.bfloat16, torch.int32, torch.float32


def _match(y, B, grid, C, mode, ctr=0, seed=5, layer=2):
    from sd_lora_trainer_amd import ops
    N = grid[0] * grid[1]
    dst, nmax, nidx = torch.full((N // 4,), -1, dtype=I32).cuda(), torch.zeros(B * (N - N // 4)).cuda(), torch.full((B * (N - N // 4),), -1, dtype=I32).cuda()
    ops.tome_match(y, dst, nmax, nidx, B=B, grid=grid, C_=C, mode=mode, seed=seed, ctr=torch.tensor([ctr, 0], dtype=I32).cuda(), layer=layer)
    return dst.cpu().long(), nmax.cpu().view(B, -1), nidx.cpu().long().view(B, -1)


def _scores64(y, dst, B, N, C):      # [B, N_src, N_dst] in float64 from the bf16 values
    yd = y[:, :C].double().cpu().view(B, N, C)
    src = torch.tensor(sorted(set(range(N)) - set(dst.tolist())))
    inv = yd.pow(2).sum(-1).sqrt().reciprocal()
    return (yd[:, src] @ yd[:, dst].transpose(1, 2)) * inv[:, src, None] * inv[:, None, dst]


@pytest.mark.parametrize("mode", ["fixed", "random"])
# (256 destinations per step of the kernel: 48 x 32 is 1.5 steps, waves 2 and 3 of the last wholly past N_dst; 32 x 64 two steps of three K chunks, one ragged)
@pytest.mark.parametrize("grid,C", [((4, 4), 64), ((6, 10), 64), ((16, 16), 320), ((24, 16), 640), ((32, 32), 64), ((48, 32), 64), ((32, 64), 136)])
def test_match_fp64(grid, C, mode):
    (Hg, Wg), B = grid, 2
    N = Hg * Wg
    y = torch.randn(B * N, C + 8, generator=torch.Generator().manual_seed(Hg * Wg + C)).to(BF16).cuda()      # (ld > C)
    dst, nmax, nidx = _match(y, B, grid, C, mode, ctr=3)
    # one destination per cell, inside its cell, cells in raster order
    cy, cx = dst // Wg // 2, dst % Wg // 2
    assert torch.equal(cy * (Wg // 2) + cx, torch.arange(N // 4))
    if mode == "fixed":
        assert bool(((dst // Wg) % 2 == 0).all() and ((dst % Wg) % 2 == 0).all())
    else:
        assert torch.equal(_match(y, B, grid, C, mode, ctr=3)[0], dst) and not torch.equal(_match(y, B, grid, C, mode, ctr=4)[0], dst)
    S, tol = _scores64(y, dst, B, N, C), (C + 8) * 2.0 ** -23
    want = S.max(-1).values
    assert bool((nidx >= 0).all() and (nidx < N // 4).all())
    chosen = S.gather(2, nidx[..., None])[..., 0]
    print(f"tome_match {grid} C={C} {mode}: max |node_max - fp64| {float((nmax.double() - want).abs().max()):.3e}, worst chosen deficit {float((want - chosen).max()):.3e}, tol {tol:.3e}")
    assert bool((chosen >= want - tol).all()) and float((nmax.double() - want).abs().max()) <= tol


@pytest.mark.parametrize("grid,C", [((16, 16), 64), ((16, 16), 256), ((48, 32), 64)])
def test_match_exact(grid, C):
    # entries +-1: norms, 1 / norm and every score are exact and full of ties - the bits of the maximum and the FIRST argmax (48 x 32: across destination blocks)
    B, N = 2, grid[0] * grid[1]
    y = (torch.randint(0, 2, (B * N, C), generator=torch.Generator().manual_seed(C)) * 2 - 1).to(BF16).cuda()
    dst, nmax, nidx = _match(y, B, grid, C, "fixed")
    S = _scores64(y, dst, B, N, C)
    want = S.max(-1).values
    first = torch.where(S == want[..., None], torch.arange(N // 4), N).min(-1).values
    assert torch.equal(nmax, want.float()) and torch.equal(nidx, first)


def test_fixed_destinations_worked_example():
    from tests.test_tome_cpu import FIXED_4X6
    assert _match(torch.ones(2 * 24, 64).to(BF16).cuda(), 2, (4, 6), 64, "fixed")[0].tolist() == FIXED_4X6


# (a plan thread owns ceil(N / 1024) tokens: 34 x 32 two with a ragged end, 66 x 64 five and two destinations, 128 x 128 the full sixteen and four)
PLAN_GRIDS = [(4, 4), (6, 10), (32, 32), (34, 32), (66, 64), (128, 128)]


def _legal_r(N, kind):      # smallest legal, middle, largest legal (N_src itself where (N - N_src) % 8 == 0)
    from sd_lora_trainer_amd import ops
    return {"smallest": N % 8, "middle": ops.tome_rows(N, 0.5), "largest": ops.tome_rows(N, 0.75)}[kind]


@functools.lru_cache(maxsize=None)
def _tables(grid, kind):
    """Hand-made inputs of the plan launch (repeated node_max values; destination 0 gets no source, destination 1 every third) and the tables built on the
    CPU from the stable descending sort."""
    (Hg, Wg), B = grid, 2
    N, g = Hg * Wg, torch.Generator().manual_seed(Hg + Wg)
    Nd, Ns, r = N // 4, N - N // 4, _legal_r(N, kind)
    off = torch.randint(0, 4, (Nd,), generator=g)
    cell = torch.arange(Nd)
    dst = (2 * (cell // (Wg // 2)) + off // 2) * Wg + 2 * (cell % (Wg // 2)) + off % 2
    nmax = torch.randint(0, 5, (B, Ns), generator=g).float() / 4
    nidx = torch.randint(1, Nd, (B, Ns), generator=g)
    nidx[:, ::3] = 1
    src = torch.tensor(sorted(set(range(N)) - set(dst.tolist())))
    tmap, kept, offs, lst = torch.zeros(B, N, dtype=torch.long), torch.zeros(B, N - r, dtype=torch.long), torch.zeros(B, Nd + 1, dtype=torch.long), torch.zeros(B, max(r, 1), dtype=torch.long)
    for b in range(B):
        merged = torch.sort(nmax[b], descending=True, stable=True).indices[:r]
        is_m = torch.zeros(N, dtype=torch.bool)
        is_m[src[merged]] = True
        kept[b] = torch.arange(N)[~is_m]
        tmap[b, kept[b]] = torch.arange(N - r)
        into = torch.full((N,), -1)
        into[src[merged]] = nidx[b, merged]
        tmap[b, is_m] = tmap[b, dst[into[is_m]]]
        groups = [torch.arange(N)[into == j] for j in range(Nd)]
        offs[b, 1:] = torch.tensor([len(q) for q in groups]).cumsum(0)
        lst[b, :r] = torch.cat(groups)
    return dict(B=B, N=N, r=r, dst=dst, nmax=nmax, nidx=nidx, map=tmap, kept=kept, offs=offs, list=lst)


def _dev(t, dtype=I32):
    return t.to(dtype).contiguous().cuda()


@pytest.mark.parametrize("kind", ["smallest", "middle", "largest"])
@pytest.mark.parametrize("grid", PLAN_GRIDS)
def test_plan_exact(grid, kind):
    from sd_lora_trainer_amd import ops
    t = _tables(grid, kind)
    B, N, r = t["B"], t["N"], t["r"]

    def run():
        out = [torch.full((n,), -7, dtype=I32).cuda() for n in (B * N, B * (N - r), B * (N // 4 + 1), B * max(r, 1))]
        ops.tome_plan(_dev(t["nmax"], F32).view(-1), _dev(t["nidx"]).view(-1), _dev(t["dst"]), *out, B=B, grid=grid, r=r)
        return [o.cpu().long() for o in out]
    got = run()
    for name, g_, w in zip(("map", "kept_tok", "offsets", "list"), got, (t["map"], t["kept"], t["offs"], t["list"])):
        if name == "list" and r == 0:
            continue
        assert torch.equal(g_, w.reshape(-1)), name
    assert all(torch.equal(a, b) for a, b in zip(got, run())), "two runs differ"


@pytest.mark.parametrize("kind", ["smallest", "middle", "largest"])
@pytest.mark.parametrize("grid", PLAN_GRIDS)
def test_merge_unmerge_fp64(grid, kind):
    # guard rows after each output keep their sentinel; one bf16 rounding; copies are bit-equal; NaN in a merged source stays in its destination's row
    from sd_lora_trainer_amd import ops
    t, C = _tables(grid, kind), 72
    B, N, r = t["B"], t["N"], t["r"]
    Np, g = N - r, torch.Generator().manual_seed(N + r)
    y = torch.randn(B * N, C + 8, generator=g).to(BF16)
    nan_tok = int(t["list"][0, 0]) if r else None
    if r:
        y[nan_tok] = float("nan")
    tabs = [_dev(t[k]).view(-1) for k in ("dst", "kept", "offs", "list")]
    buf = torch.full((B * Np + 8, C), 7.0, dtype=BF16).cuda()
    ops.tome_merge(y.cuda(), *tabs, buf[:B * Np], B=B, grid=grid, r=r, C_=C)
    ym = buf.cpu()
    assert bool((ym[B * Np:] == 7.0).all()), "rows beyond B N' were written"
    y64 = y[:, :C].double().view(B, N, C)
    for b in range(B):
        ref = y64[b, t["kept"][b]].clone()
        single = torch.ones(Np, dtype=torch.bool)
        for j in range(N // 4):
            q = t["list"][b, t["offs"][b, j]:t["offs"][b, j + 1]]
            if len(q):
                row = t["map"][b, t["dst"][j]]
                ref[row] = (y64[b, t["dst"][j]] + y64[b, q].sum(0)) / (len(q) + 1)
                single[row] = False
        got = ym[b * Np:(b + 1) * Np]
        assert torch.equal(got[single].view(torch.int16), y[b * N + t["kept"][b]][single][:, :C].view(torch.int16)), "a copied row changed"
        nan_row = ref.isnan().any(1)
        assert int(nan_row.sum()) == (1 if r and b == 0 else 0) and torch.equal(got.isnan().any(1), nan_row)
        assert bool(((got.double() - ref).abs()[~nan_row] <= 2.0 ** -8 * ref.abs()[~nan_row] + 1e-6).all())
    res, a = torch.randn(B * N, C, generator=g).to(BF16), ym[:B * Np].clone()
    obuf = torch.full((B * N + 8, C), 7.0, dtype=BF16).cuda()
    ops.tome_unmerge(res.cuda(), a.cuda(), _dev(t["map"]).view(-1), obuf[:B * N], B=B, N=N, Np=Np)
    out = obuf.cpu()
    assert bool((out[B * N:] == 7.0).all()), "rows beyond B N were written"
    rows = (t["map"] + torch.arange(B)[:, None] * Np).view(-1)
    ref = res.double() + a.double()[rows]
    bad = ref.isnan().any(1)
    assert torch.equal(out[:B * N].isnan().any(1), bad)
    if r:
        assert torch.equal(bad.view(B, N)[0], t["map"][0] == t["map"][0, nan_tok]) and not bool(bad.view(B, N)[1].any())
    assert bool(((out[:B * N].double() - ref).abs()[~bad] <= 2.0 ** -8 * ref.abs()[~bad] + 1e-6).all())


def _emu_plan(nmax, nidx, dst, map_, kept, offs, lst, *, B, grid, r):      # plain torch: the stable descending sort decides
    N = grid[0] * grid[1]
    Ns, is_dst = N - N // 4, torch.zeros(N, dtype=torch.bool, device=dst.device)
    is_dst[dst.long()] = True
    src, tok = torch.arange(N, device=dst.device)[~is_dst], torch.arange(N, device=dst.device)
    for b in range(B):
        merged = torch.sort(nmax.view(B, Ns)[b], descending=True, stable=True).indices[:r]
        is_m = torch.zeros_like(is_dst)
        is_m[src[merged]] = True
        k = tok[~is_m]
        m = torch.zeros(N, dtype=torch.long, device=dst.device)
        m[k] = torch.arange(N - r, device=dst.device)
        m[src[merged]] = m[dst.long()[nidx.view(B, Ns)[b, merged].long()]]
        map_.view(B, N)[b], kept.view(B, N - r)[b] = m.to(I32), k.to(I32)


def _emu_merge(y, dst, kept, offs, lst, ym, *, B, grid, r, C_=None, map_=None):      # fp32 sums by index_add over the map the emulated plan left
    N, C = grid[0] * grid[1], y.shape[1]
    for b in range(B):
        acc, cnt = torch.zeros(N - r, C, device=y.device), torch.zeros(N - r, device=y.device)
        acc.index_add_(0, map_.view(B, N)[b].long(), y[b * N:(b + 1) * N].float())
        cnt.index_add_(0, map_.view(B, N)[b].long(), torch.ones(N, device=y.device))
        ym[b * (N - r):(b + 1) * (N - r)] = (acc / cnt[:, None]).to(BF16)
    return ym


def _emu_unmerge(res, a, map_, out, *, B, N, Np):
    rows = (map_.view(B, N).long() + torch.arange(B, device=a.device)[:, None] * Np).view(-1)
    out.copy_((res.float() + a.float()[rows]).to(BF16))
    return out


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_token_merge(version, monkeypatch):
    from oracle import unet_ref as U
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import ops, topology
    B, h, cfg, g = 2, 16, U.CONFIGS[version], torch.Generator().manual_seed(11)
    x, tf = torch.randn(B, 4, h, h, generator=g), torch.tensor([500.0, 200.0]).cuda()
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    rt = M.Runtime("cuda:0", B)
    ctx = torch.zeros(B, M.CTX_PAD, cfg["cross_dim"], dtype=rt.act, device="cuda")
    ctx[:, :77] = torch.randn(B, 77, cfg["cross_dim"], generator=g).to(rt.act).cuda()
    extra = (torch.randn(B, P, generator=g).to(rt.act).cuda(), torch.tensor([128., 128, 0, 0, 128, 128]).repeat(B).cuda()) if P else ()
    unet = M.UNet(rt, topology.CONFIGS[version], U.init_unet_state(cfg, seed=0), lora_rank=4)
    unet.arena.load(U.init_lora(cfg, 4, seed=1, b_std=0.05))
    x64 = torch.nn.functional.pad(x.permute(0, 2, 3, 1).reshape(-1, 4), (0, 60)).to(rt.act).cuda()
    run = lambda **kw: unet.forward(x64, tf, ctx.view(-1, ctx.shape[-1]), *extra, B=B, H=h, W=h, **kw).clone()  # noqa: E731
    plain = run(train=False)
    assert len(unet.set_token_merge((0.5, 0.5), latent=(h, h))) >= 3
    got = run(train=False)
    with pytest.raises(NotImplementedError, match="token_merge is an inference option"):
        run(train=True)
    for other, args in (("set_kv_downsample", ((2,),)), ("set_hypertile", (((2, 2),),))):
        with pytest.raises(ValueError, match="set_token_merge"):
            getattr(unet, other)(*args)
    last = {}
    monkeypatch.setattr(ops, "tome_plan", lambda *a, **k: (last.update(map_=a[3]), _emu_plan(*a, **k))[1])
    monkeypatch.setattr(ops, "tome_merge", lambda *a, **k: _emu_merge(*a, **k, **last))
    monkeypatch.setattr(ops, "tome_unmerge", _emu_unmerge)
    want = run(train=False)
    monkeypatch.undo()
    assert "map_" in last, "the emulations were not reached"
    err, bar = float((got - want).abs().max()), 1.5e-2 * float(want.abs().max()) + 1e-6
    print(f"unet token_merge {version}: max err {err:.3e} (bar {bar:.3e}); against the plain forward {float((got - plain).abs().max()):.3e}")
    assert err <= bar and float((got - plain).abs().max()) > bar
    assert unet.set_token_merge(None) == {} and torch.equal(run(train=False), plain)
    for other, args, msg in (("set_kv_downsample", ((2,),), "kv_downsample factor 2"), ("set_hypertile", (((2, 2),),), "hypertile")):
        getattr(unet, other)(*args)
        with pytest.raises(ValueError, match=msg):
            unet.set_token_merge((0.5,))
        getattr(unet, other)(None)
    with pytest.raises(ValueError, match="is odd"):
        unet.set_token_merge((0.5, 0.5), latent=(18, 18))


@pytest.mark.parametrize("mode", ["random", "fixed"])
def test_sampler_token_merge_paths(mode):
    # graph == fused == torch loop bit for bit; a plain capture and a merged capture replayed alternately on one sampler; the setting does not stick
    from tests.test_img2img_gpu import _cuda, _inputs, _setup
    cfg, sd, lora, smp = _setup("tiny15")
    embeds, noise, _ = _inputs(cfg, 5, 16, 16, 1)
    em, tm = _cuda(embeds)[0], dict(ratio=0.5, depth=1, mode=mode, seed=9)
    paths = dict(torch={}, fused=dict(fused=True), graph=dict(graph=True))
    run = lambda path, **kw: smp.sample(em, 16, 16, steps=4, guidance_scale=8.0, latents=noise.cuda(), **paths[path], **kw).cpu()  # noqa: E731
    plain, merged = run("fused"), run("fused", token_merge=tm)
    assert torch.isfinite(merged).all() and not torch.equal(merged, plain)
    assert torch.equal(run("graph", token_merge=tm), merged) and torch.equal(run("torch", token_merge=tm), merged)
    assert torch.isfinite(run("fused", kv_downsample=2)).all()      # on the grids the last call merged: its setting was cleared first
    for _ in range(2):
        assert torch.equal(run("graph"), plain) and smp.unet._tome is None and torch.equal(run("graph", token_merge=tm), merged)
    assert len(smp._graphs) == 2


def test_render_cli_tome(tmp_path, monkeypatch):
    # a three-step tinyxl job: 128 x 128 px = a 16 x 16 latent, merged on both grids; graph and --eager give one picture; prompts.json records the setting
    import json
    from sd_lora_trainer_amd import ops, render as R, train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_hires_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="tome job", seed=3, resolution=256, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    calls, real = [], ops.tome_match
    monkeypatch.setattr(ops, "tome_match", lambda *a, **k: (calls.append(k["grid"]), real(*a, **k))[1])
    for out, extra in (("graph", []), ("eager", ["--eager"])):
        R.main(["--checkpoint", ckdir, "--prompt", "a photo of a field", "--size", "128", "128", "--steps", "3", "--seed", "11", "--tome", "--tome-depth", "1",
                "--out", str(tmp_path / out)] + extra)
        assert json.load(open(tmp_path / out / "prompts.json"))["tome"] == dict(ratio=0.5, depth=1, mode="random", passes="all")
    assert calls and set(calls) == {(16, 16), (8, 8)}
    pic = lambda d: open(next((tmp_path / d).glob("img_00*.jpg")), "rb").read()  # noqa: E731
    assert pic("graph") == pic("eager")
