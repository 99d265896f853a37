"""sdlt_attn_window_fwd (tiled self-attention, "HyperTile"; csrc/attn_window.hip) against its formula in float64 from the bf16-rounded inputs at the bar of a
bf16-P flash forward (tests/test_attn_couple_gpu.py), UNet.set_hypertile against the same UNet on gather -> ops.attn_fwd -> scatter, and the sampler / CLI."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _tile_of(Hg, Wg, ty, tx):      # [Hg Wg] tile index of every token
    y, x = torch.meshgrid(torch.arange(Hg), torch.arange(Wg), indexing="ij")
    return ((y // (Hg // ty)) * tx + x // (Wg // tx)).reshape(-1)


def _ref64(q, k, v, B, H, Hg, Wg, ty, tx, d, scale):      # a masked softmax over the whole grid: keys outside the query's tile get -inf
    N, same = Hg * Wg, _tile_of(Hg, Wg, ty, tx)
    same = same[:, None] == same[None, :]
    q, k, v = (t.double().cpu().view(B, N, H, d).transpose(1, 2) for t in (q, k, v))
    s = (scale * q @ k.transpose(-1, -2)).masked_fill(~same, float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, H * d)


CASES = [((8, 8), (2, 2), 2, 8, 1), ((16, 24), (2, 3), 2, 64, 1), ((12, 20), (2, 2), 3, 40, 1), ((24, 24), (2, 1), 2, 64, 1), ((24, 24), (1, 2), 2, 64, 1),
         ((16, 16), (1, 1), 2, 64, 4), ((16, 16), (4, 2), 1, 80, 1), ((8, 16), (1, 4), 2, 96, 1)]


@pytest.mark.parametrize("grid,tiles,H,d,sharp", CASES)
def test_attn_window_matches_fp64(grid, tiles, H, d, sharp):
    # Q, K, V are column views of one [M, 3 C] buffer; two runs give the same bits; the guard rows after O stay; NaN in the K and V rows of tile (0, 1) (where
    # there is one) changes no bit of any other tile.  Worst measured fraction of the bar over these cases: DESIGN 4.39.
    from sd_lora_trainer_amd import ops
    (Hg, Wg), (ty, tx), B = grid, tiles, 2
    C, M, scale = H * d, B * Hg * Wg, sharp / math.sqrt(d)
    qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(100 * Hg + Wg + d)).to(BF16).cuda()
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    ref = _ref64(q, k, v, B, H, Hg, Wg, ty, tx, d, scale)

    def run(qkv_):
        buf = torch.full((M + 8, C), 7.0, dtype=BF16, device="cuda")
        ops.attn_window_fwd(qkv_[:, :C], qkv_[:, C:2 * C], qkv_[:, 2 * C:], buf[:M], B=B, H=H, grid=grid, tiles=tiles, d=d, scale=scale)
        torch.cuda.synchronize()
        assert bool((buf[M:] == 7.0).all()), "rows beyond B Hg Wg were written"
        return buf[:M].clone()
    out = run(qkv)
    assert torch.equal(out, run(qkv)), "two runs differ"
    err, bar = float((out.double().cpu() - ref).abs().max()), 1.5e-2 * float(ref.abs().max()) + 1e-6
    print(f"attn_window {grid} {tiles} H={H} d={d}: max err {err:.3e} = {err / bar:.3f} of the bar {bar:.3e}")
    assert err <= bar
    if ty * tx > 1:
        other = (_tile_of(Hg, Wg, ty, tx) != 1).repeat(B).cuda()
        bad = qkv.clone()
        bad[~other, C:] = float("nan")
        got = run(bad)
        assert torch.equal(got[other], out[other]) and bool(torch.isnan(got[~other]).all())


def _emulated(q, k, v, O, *, B, H, grid, tiles, d, scale):
    """ops.attn_window_fwd by the existing kernels: gather the tiles as batch rows (padded to 8 rows, pad keys masked), ops.attn_fwd, scatter."""
    from sd_lora_trainer_amd import ops
    (Hg, Wg), (ty, tx), C = grid, tiles, H * d
    th, tw = Hg // ty, Wg // tx
    n, T = th * tw, B * ty * tx
    Np = (n + 7) // 8 * 8
    def gather(t):
        p = torch.zeros(T, Np, C, dtype=BF16, device=t.device)
        p[:, :n] = t.reshape(B, ty, th, tx, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(T, n, C)
        return p.view(T * Np, C)
    Op, L = torch.empty(T * Np, C, dtype=BF16, device=q.device), torch.empty(T * H * Np, dtype=torch.float32, device=q.device)
    ops.attn_fwd(gather(q), gather(k), gather(v), None, Op, L, B=T, H=H, Nq=n, Nk=n, Nqp=Np, Nkp=Np, d=d, scale=scale)
    O.copy_(Op.view(T, Np, C)[:, :n].reshape(B, ty, tx, th, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B * Hg * Wg, C))
    return O


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_unet_hypertile(version, monkeypatch):
    # the emulation rounds where sdlt_attn_fwd rounds, not where the new kernel does: the bar is the kernel's, on the UNet output's range
    from oracle import unet_ref as U
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import ops, sampler, topology
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
    run = lambda: unet.forward(x64, tf, ctx.view(-1, ctx.shape[-1]), *extra, B=B, H=h, W=h, train=False).clone()  # noqa: E731
    plain = run()
    tiles = sampler.hypertile_plan(h, h, {lv for _, lv in unet._attn_levels()}, 4, 1)
    assert tiles == ((4, 4), (4, 4)) and len(unet.set_hypertile(tiles, latent=(h, h))) >= 3
    got = run()
    emulated = []
    monkeypatch.setattr(ops, "attn_window_fwd", lambda *a, **k: (emulated.append(k["tiles"]), _emulated(*a, **k))[1])
    want = run()
    monkeypatch.undo()
    assert len(emulated) >= 3
    err, bar = float((got - want).abs().max()), 1.5e-2 * float(want.abs().max()) + 1e-6
    print(f"unet hypertile {version}: max err {err:.3e} (bar {bar:.3e}); against the plain forward {float((got - plain).abs().max()):.3e}")
    assert err <= bar and float((got - plain).abs().max()) > bar
    assert unet.set_hypertile(((1, 1),)) == {} and torch.equal(run(), plain)


def test_sampler_hypertile_paths():
    # graph == fused == torch loop bit for bit; a plain capture and a hypertile capture replayed alternately on one sampler; the setting does not stick
    from tests.test_img2img_gpu import _cuda, _inputs, _setup
    cfg, sd, lora, smp = _setup("tiny15")
    embeds, noise, _ = _inputs(cfg, 5, 16, 16, 1)
    em, hp = _cuda(embeds)[0], dict(tile=4, depth=1)
    paths = dict(torch={}, fused=dict(fused=True), graph=dict(graph=True))
    run = lambda path, **kw: smp.sample(em, 16, 16, steps=4, guidance_scale=8.0, latents=noise.cuda(), **paths[path], **kw).cpu()  # noqa: E731
    plain, tiled = run("fused"), run("fused", hypertile=hp)
    assert torch.isfinite(tiled).all() and not torch.equal(tiled, plain)
    assert torch.equal(run("graph", hypertile=hp), tiled) and torch.equal(run("torch", hypertile=hp), tiled)
    for _ in range(2):
        assert torch.equal(run("graph"), plain) and smp.unet._ht is None and torch.equal(run("graph", hypertile=hp), tiled)
    assert len(smp._graphs) == 2


def test_render_cli_hypertile(tmp_path, monkeypatch):
    # a one-step tinyxl job (the toy VAE's factor is 4): 128 x 128 px = a 32 x 32 latent, 32 px tiles = 8 cells, depth 1: both self-attention grids (16 x 16,
    # 8 x 8 tokens) run the tiled launch with 4 x 4 tiles; graph and --eager give one picture
    import json
    from sd_lora_trainer_amd import ops, render as R, train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    from tests.test_hires_gpu import _run
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="hypertile job", seed=3, resolution=256, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tinyxl", "tokenizer_path": tok_dir})
    _, ckdir = _run(T.train(cfg))
    calls, real = [], ops.attn_window_fwd
    monkeypatch.setattr(ops, "attn_window_fwd", lambda *a, **k: (calls.append(k["tiles"]), real(*a, **k))[1])
    for out, extra in (("graph", []), ("eager", ["--eager"])):
        R.main(["--checkpoint", ckdir, "--prompt", "a photo of a field", "--size", "128", "128", "--steps", "3", "--seed", "11", "--hypertile", "32", "--hypertile-depth", "1",
                "--out", str(tmp_path / out)] + extra)
        assert json.load(open(tmp_path / out / "prompts.json"))["hypertile"] == dict(tile_px=32, tile=8, depth=1, passes="all")
    assert calls and set(calls) == {(4, 4)}
    pic = lambda d: open(next((tmp_path / d).glob("img_00*.jpg")), "rb").read()  # noqa: E731
    assert pic("graph") == pic("eager")
