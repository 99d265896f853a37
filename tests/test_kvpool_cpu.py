"""Key / value token downsampling without a GPU: the restatement of sdlt_token_pool (tests/kvpool_ref.py) against torch's own layer_norm, slicing and
avg_pool2d; f = 1 and the pad rows; which transformers UNet.set_kv_downsample gives which factor on the SDXL and SD1.5 wiring; the UNet and the sampler
on the emulated op table; every refusal; the entry point's argument checks; the CLI; and a two-pass render whose first pass runs without the option."""
import json
import os
import types

import pytest
import torch

import sd_lora_trainer_amd.unet as unet_mod
from oracle import unet_ref as U
from sd_lora_trainer_amd import sampler as SM
from sd_lora_trainer_amd import topology
from tests import img2img_ref as IR
from tests import kvpool_ref as KR
from tests.test_guidance_cpu import _FakeLoaded
from tests.test_render_cpu import job  # noqa: F401  (fixture: a two-step tiny15 job trained on the emulated op table)

# (B, H, W, C, f): the shapes of the device test, and f = 1
CASES = [(2, 5, 7, 320, 2), (1, 8, 12, 640, 4), (2, 6, 6, 1280, 3), (1, 9, 4, 640, 4), (2, 5, 7, 320, 1)]


def _rows(B, H, W, C, seed=0):
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + seed)
    x = (torch.randn(B * H * W, C, generator=g) * 1.5 + 0.3 + torch.randn(B * H * W, 1, generator=g)).to(torch.bfloat16)
    return x, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


@pytest.mark.parametrize("mode", KR.MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_restatement_against_torch(case, mode):
    """Window by window against F.layer_norm -> [::f, ::f] / avg_pool2d(ceil_mode=True, count_include_pad=False): fp32 on both sides, so the bar is a
    few fp32 roundings of values of order 5 (1e-5 absolute); the pad rows are exactly zero; f = 1 is the LayerNorm rows themselves."""
    B, H, W, C, f = case
    x, gamma, beta = _rows(B, H, W, C)
    got = KR.token_pool_ref(x, B=B, H=H, W=W, gamma=gamma, beta=beta, eps=1e-5, f=f, mode=mode)
    Ho, Wo, Nk, Nkp = KR.token_pool_rows(H, W, f)
    assert (Ho, Wo) == (-(-H // f), -(-W // f)) and Nk == Ho * Wo and Nkp % 8 == 0 and 0 <= Nkp - Nk < 8
    assert got.dtype == torch.float32 and tuple(got.shape) == (B * Nkp, C)
    want = KR.token_pool_torch(x, B=B, H=H, W=W, gamma=gamma, beta=beta, eps=1e-5, f=f, mode=mode)
    err = float((got.view(B, Nkp, C)[:, :Nk] - want).abs().max())
    print(f"{case} {mode}: max |restatement - torch| {err:.3e}")
    assert err <= 1e-5
    assert bool((got.view(B, Nkp, C)[:, Nk:] == 0).all())
    if f == 1:
        assert torch.equal(got.view(B, Nkp, C)[:, :Nk].reshape(B * H * W, C), KR.layernorm_rows(x, gamma, beta, 1e-5))
    y = torch.full((B * Nkp, C), 7.0)
    assert KR.token_pool(x, y, B=B, H=H, W=W, gamma=gamma, beta=beta, eps=1e-5, f=f, mode=mode) is y and torch.equal(y, got)


def test_partial_windows_divide_by_their_own_count():
    """A constant-per-row input whose LayerNorm output is beta: every area window, whole or partial, returns beta - a divisor of f^2 at the edges would not."""
    B, H, W, C, f = 1, 5, 7, 16, 2
    x = torch.arange(H * W, dtype=torch.float32)[:, None].repeat(1, C).to(torch.bfloat16)
    beta = torch.linspace(-1, 1, C)
    got = KR.token_pool_ref(x, B=B, H=H, W=W, gamma=torch.ones(C), beta=beta, eps=1e-5, f=f, mode="area")
    assert torch.allclose(got[:12], beta.expand(12, C), atol=1e-6)


# ---- which module gets which factor ------------------------------------------------------------------------------------------------------------
class _Skeleton(unet_mod.UNet):
    """The transformers of a topology in UNet.__init__'s order, without weights: what set_kv_downsample walks."""

    def __init__(self, version, ops=KR.emu_kv):
        cfg = topology.CONFIGS[version]
        self.cfg, self.rt, self._kv_ds = cfg, types.SimpleNamespace(ops=ops), None
        n, L = len(cfg["block_out_channels"]), cfg["layers_per_block"]

        def t2d(name, layers):
            return types.SimpleNamespace(name=name, blocks=[types.SimpleNamespace(attn1=types.SimpleNamespace(_kv=None)) for _ in range(layers)])

        tl = cfg["transformer_layers"]
        self.down = [(None, [t2d(f"down_blocks.{i}.attentions.{j}", tl[i]) for j in range(L)] if cfg["down_has_attn"][i] else [], None) for i in range(n)]
        self.mid = (None, t2d("mid_block.attentions.0", tl[-1]), None)
        self.up = [(None, [t2d(f"up_blocks.{i}.attentions.{j}", tl[n - 1 - i]) for j in range(L + 1)] if cfg["up_has_attn"][i] else [], None) for i in range(n)]

    def factors(self):
        ts = [t for _, att, _ in self.down for t in att] + [self.mid[1]] + [t for _, att, _ in self.up for t in att]
        out = {}
        for t in ts:
            kv = {b.attn1._kv for b in t.blocks}
            assert len(kv) == 1                                                      # every layer of a transformer has the same setting
            out[t.name] = kv.pop()
        return out


def _names(prefix, n):
    return {f"{prefix}.attentions.{j}" for j in range(n)}


def test_factor_per_grid_on_sdxl_and_sd15():
    xl = _Skeleton("sdxl")                       # self-attention at H / 2 (640 wide: down_blocks.1, up_blocks.1) and H / 4 (1280: down_blocks.2, mid, up_blocks.0)
    big, small = _names("down_blocks.1", 2) | _names("up_blocks.1", 3), _names("down_blocks.2", 2) | {"mid_block.attentions.0"} | _names("up_blocks.0", 3)
    assert xl.set_kv_downsample((2,)) == {n: 2 for n in big} and xl._kv_ds == ((2,), "nearest")
    assert xl.factors() == dict({n: (2, 0) for n in big}, **{n: None for n in small})
    assert xl.set_kv_downsample((4, 2), "area") == dict({n: 4 for n in big}, **{n: 2 for n in small}) and xl._kv_ds == ((4, 2), "area")
    assert xl.factors() == dict({n: (4, 1) for n in big}, **{n: (2, 1) for n in small})
    assert xl.set_kv_downsample((1, 2)) == {n: 2 for n in small}                     # a factor of 1 leaves its grid alone
    assert xl.factors() == dict({n: None for n in big}, **{n: (2, 0) for n in small})
    for off in (None, (), (1,), (1, 1)):
        xl.set_kv_downsample((2,))
        assert xl.set_kv_downsample(off) == {} and xl._kv_ds is None and set(xl.factors().values()) == {None}
    assert xl.set_kv_downsample((2, 1)) == {n: 2 for n in big} and xl._kv_ds == ((2,), "nearest")      # trailing ones are not part of the setting
    with pytest.raises(ValueError, match="2 token grid"):
        xl.set_kv_downsample((2, 2, 2))
    sd = _Skeleton("sd15")                       # self-attention at H, H / 2, H / 4 and, in the mid block alone, H / 8
    lv = [_names("down_blocks.0", 2) | _names("up_blocks.3", 3), _names("down_blocks.1", 2) | _names("up_blocks.2", 3),
          _names("down_blocks.2", 2) | _names("up_blocks.1", 3), {"mid_block.attentions.0"}]
    assert sd.set_kv_downsample((2,)) == {n: 2 for n in lv[0]}
    assert sd.set_kv_downsample((4, 2)) == dict({n: 4 for n in lv[0]}, **{n: 2 for n in lv[1]})
    assert sd.set_kv_downsample((8, 4, 2, 2)) == {n: f for names, f in zip(lv, (8, 4, 2, 2)) for n in names}
    assert set(sd.factors()) == set().union(*lv)
    with pytest.raises(ValueError, match="4 token grid"):
        sd.set_kv_downsample((2, 2, 2, 2, 2))


def test_set_kv_downsample_refusals():
    sk = _Skeleton("sdxl")
    for bad in ((0,), (2, -1), (2.0,), ("2",), (True,), 1.5):
        with pytest.raises((ValueError, TypeError), match="kv_downsample|iterable"):
            sk.set_kv_downsample(bad)
    with pytest.raises(ValueError, match="mode"):
        sk.set_kv_downsample((2,), "bilinear")
    assert sk._kv_ds is None and set(sk.factors().values()) == {None}                 # a refused setting leaves the plain path
    bare = _Skeleton("sdxl", ops=IR.emu_img)                                          # an op table without the kernel: refused by name, no torch fallback
    with pytest.raises(NotImplementedError, match="sdlt_token_pool"):
        bare.set_kv_downsample((2,))
    assert bare.set_kv_downsample((1,)) == {}                                         # ... which nothing asks for when every factor is 1
    for good, want in ((None, None), ((), None), ((1, 1), None), (2, ((2,), "nearest")), ([4, 2, 1], ((4, 2), "nearest"))):
        assert SM.kv_downsample_args(good) == want
    assert SM.kv_downsample_args((2,), "area") == ((2,), "area")
    for bad in ((0,), (2.5,), ("a",), (True,)):
        with pytest.raises(ValueError, match="kv_downsample"):
            SM.kv_downsample_args(bad)
    with pytest.raises(ValueError, match="kv_downsample_mode"):
        SM.kv_downsample_args((2,), "cubic")


# ---- the UNet and the sampler on the emulated table -------------------------------------------------------------------------------------------
def _model(version, ops=KR.emu_kv, rank=4):
    cfg = U.CONFIGS[version]
    sd, lora = U.init_unet_state(cfg, seed=0), U.init_lora(cfg, rank, seed=1, b_std=0.05)
    rt = unet_mod.Runtime("cpu", 2, act_dtype=torch.float32, ops=ops)
    unet = unet_mod.UNet(rt, topology.CONFIGS[version], sd, lora_rank=rank)
    unet.arena.load(lora)
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    embeds = (mk(1, 77, cfg["cross_dim"]), mk(1, 77, cfg["cross_dim"])) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None))
    return cfg, rt, unet, embeds, mk


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_on_the_emulated_table(version):
    """16 x 16 latent, 3 steps.  (1,) and () are the plain run bit for bit; (2,) moves the latents, stays close to them (the pooled keys still describe
    the same picture) and is the same on the torch loop and the fused loop; the launches are the expected ones: one token_pool per affected
    self-attention and forward, at the largest grid only; afterwards a call without the option is plain again."""
    cfg, rt, unet, embeds, mk = _model(version)
    calls = []
    real = KR.token_pool
    rt.ops = types.ModuleType("spy")
    rt.ops.__dict__.update({k: v for k, v in vars(KR.emu_kv).items() if not k.startswith("__")})
    rt.ops.token_pool = lambda x, y, **kw: (calls.append((kw["H"], kw["W"], kw["f"], kw["mode"])), real(x, y, **kw))[1]
    smp = SM.LatentSampler(rt, unet)
    noise = mk(1, 4, 16, 16)
    kw = dict(steps=3, guidance_scale=8.0, latents=noise)
    plain = smp.sample(embeds, 16, 16, **kw)
    assert torch.equal(smp.sample(embeds, 16, 16, kv_downsample=(1,), **kw), plain) and torch.equal(smp.sample(embeds, 16, 16, kv_downsample=(), **kw), plain)
    assert not calls and unet._kv_ds is None
    ds = smp.sample(embeds, 16, 16, kv_downsample=(2,), **kw)
    grid = 16 if version == "tiny15" else 8                    # tiny15's largest self-attention grid is the latent's, tinyxl's half of it
    per_forward = 3                                            # one transformer of one layer in the down block of that grid, two in the up block
    assert set(calls) == {(grid, grid, 2, 0)} and len(calls) == 3 * per_forward
    cos = float(torch.nn.functional.cosine_similarity(ds.reshape(1, -1), plain.reshape(1, -1)))
    print(f"{version}: cos((2,) nearest, plain) = {cos:.5f}, rel {float((ds - plain).norm() / plain.norm()):.4f}")
    assert torch.isfinite(ds).all() and not torch.equal(ds, plain) and cos >= 0.5      # (random weights: a sanity band, no statement about pictures)
    fused = smp.sample(embeds, 16, 16, kv_downsample=(2,), fused=True, **kw)
    assert float((fused - ds).abs().max()) <= 1e-4 * float(ds.abs().max())
    area = smp.sample(embeds, 16, 16, kv_downsample=(2,), kv_downsample_mode="area", **kw)
    assert not torch.equal(area, ds) and calls[-1] == (grid, grid, 2, 1)
    assert torch.equal(smp.sample(embeds, 16, 16, **kw), plain) and unet._kv_ds is None          # the setting does not stick
    both = smp.sample(embeds, 16, 16, kv_downsample=(2, 2), **kw)
    assert not torch.equal(both, ds) and (grid // 2, grid // 2, 2, 0) in calls
    smp2 = SM.LatentSampler(rt, unet, kv_downsample=(2,))                                        # the constructor's default; sample() overrides it
    assert torch.equal(smp2.sample(embeds, 16, 16, **kw), ds) and torch.equal(smp2.sample(embeds, 16, 16, kv_downsample=(), **kw), plain)
    assert torch.equal(smp2.sample(embeds, 16, 16, kv_downsample_mode="area", **kw), area)


def test_forward_refusals():
    cfg, rt, unet, embeds, mk = _model("tiny15")
    smp = SM.LatentSampler(rt, unet)
    with pytest.raises(ValueError, match="kv_downsample"):
        smp.sample(embeds, 8, 8, steps=1, kv_downsample=(0,))
    with pytest.raises(ValueError, match="kv_downsample_mode"):
        smp.sample(embeds, 8, 8, steps=1, kv_downsample=(2,), kv_downsample_mode="max")
    with pytest.raises(ValueError, match="factor 4 does not fit the 2 x 2"):      # (4, 4, 4) at an 8 x 8 latent: the third grid is 2 x 2
        smp.sample(embeds, 8, 8, steps=1, kv_downsample=(4, 4, 4), latents=mk(1, 4, 8, 8))
    # a training forward, and the backward: refused by name; with the option off again both run as before
    unet.set_kv_downsample((2,))
    x64, tf, ctx = torch.zeros(2 * 64, 64), torch.zeros(2), torch.zeros(2 * unet_mod.CTX_PAD, cfg["cross_dim"])
    with pytest.raises(NotImplementedError, match="kv_downsample"):
        unet.forward(x64, tf, ctx, B=2, H=8, W=8)
    with pytest.raises(NotImplementedError, match="kv_downsample"):
        unet.forward(x64, tf, ctx, B=2, H=8, W=8, train=True)
    with pytest.raises(NotImplementedError, match="kv_downsample"):
        unet.backward(None, None)
    got = unet.forward(x64, tf, ctx, B=2, H=8, W=8, train=False).clone()
    unet.set_kv_downsample(None)
    plain = unet.forward(x64, tf, ctx, B=2, H=8, W=8)
    assert torch.isfinite(got).all() and not torch.equal(got, plain) and torch.equal(unet.forward(x64, tf, ctx, B=2, H=8, W=8, train=False), plain)
    # TrainStep is such a training forward
    import sd_lora_trainer_amd.step as S
    rt1 = unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=KR.emu_kv)
    u1 = unet_mod.UNet(rt1, topology.CONFIGS["tiny15"], U.init_unet_state(cfg, seed=0), lora_rank=4)
    ts = S.TrainStep(rt1, u1, latent_hw=(8, 8))
    g = torch.Generator().manual_seed(3)
    ts.set_batch(torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g), torch.tensor([500]), torch.ones(1, 4, 8, 8),
                 torch.randn(1, 77, cfg["cross_dim"], generator=g), None, None)
    u1.set_kv_downsample((2,))
    with pytest.raises(NotImplementedError, match="kv_downsample"):
        ts.run(1e-4)
    # an op table without the kernel
    _, rt2, bare, _, _ = _model("tiny15", ops=IR.emu_img)
    with pytest.raises(NotImplementedError, match="sdlt_token_pool"):
        SM.LatentSampler(rt2, bare).sample(embeds, 8, 8, steps=1, kv_downsample=(2,))


def test_ops_wrapper_checks():
    """ops.token_pool refuses before it reaches the library: dtype, shapes, the row count of y, the factor."""
    from sd_lora_trainer_amd import ops
    assert ops.token_pool_rows(5, 7, 2) == (3, 4, 12, 16) == KR.token_pool_rows(5, 7, 2) and ops.token_pool_rows(8, 12, 4) == (2, 3, 6, 8)
    assert ops.TOKEN_POOL_MODES == KR.MODES == SM.KV_MODES
    x, g = torch.zeros(2 * 35, 16, dtype=torch.bfloat16), torch.ones(16)
    with pytest.raises(AssertionError):                                           # (CPU tensors: refused like every wrapper's)
        ops.token_pool(x, torch.zeros(32, 16, dtype=torch.bfloat16), B=2, H=5, W=7, gamma=g, beta=g, eps=1e-5, f=2, mode="nearest")


def test_entry_point_validation():
    """Contract violations: a negative code, the entry point's name in the message, nothing launched (no GPU here)."""
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    assert "sdlt_token_pool" in _lib.SYMBOLS
    ok = dict(x=0x100000, ldx=320, B=2, H=5, W=7, C=320, gamma=0x200000, beta=0x210000, eps=1e-5, f=2, mode=1, y=0x300000, ldy=320, Nkp=16)
    order = ("x", "ldx", "B", "H", "W", "C", "gamma", "beta", "eps", "f", "mode", "y", "ldy", "Nkp")
    SHAPE, ALIGN, UNSUPPORTED = -1, -2, -4
    for change, code, word in ((dict(x=None), SHAPE, b"null"), (dict(y=None), SHAPE, b"null"), (dict(gamma=None), SHAPE, b"null"), (dict(beta=None), SHAPE, b"null"),
                               (dict(B=0), SHAPE, b"B=0"), (dict(H=0), SHAPE, b"H=0"), (dict(W=-1), SHAPE, b"W=-1"), (dict(C=0), SHAPE, b"C=0"),
                               (dict(C=12), SHAPE, b"C=12"), (dict(C=1544, ldx=1544, ldy=1544), SHAPE, b"C=1544"),
                               (dict(f=0), SHAPE, b"f=0"), (dict(f=6), SHAPE, b"f=6"), (dict(f=8), SHAPE, b"f=8"),
                               (dict(Nkp=8), SHAPE, b"Nkp=8"), (dict(Nkp=12), SHAPE, b"Nkp=12"), (dict(Nkp=20), SHAPE, b"Nkp=20"),
                               (dict(ldx=312), SHAPE, b"below"), (dict(ldy=8), SHAPE, b"below"),
                               (dict(mode=2), UNSUPPORTED, b"mode=2"), (dict(mode=-1), UNSUPPORTED, b"mode=-1"),
                               (dict(x=0x100008), ALIGN, b"aligned"), (dict(y=0x300002), ALIGN, b"aligned"), (dict(gamma=0x200004), ALIGN, b"aligned"),
                               (dict(beta=0x210008), ALIGN, b"aligned"), (dict(ldx=324), ALIGN, b"aligned"), (dict(ldy=332), ALIGN, b"aligned"),
                               (dict(y=0x100000), SHAPE, b"overlaps"), (dict(y=0x100000 + 2 * (69 * 320 + 312)), SHAPE, b"overlaps"),
                               (dict(x=0x300000 + 2 * (31 * 320 + 312)), SHAPE, b"overlaps"),
                               (dict(B=1 << 20, H=64, W=64, f=64, Nkp=8), SHAPE, b"rows")):
        a = dict(ok, **change)
        assert lib.sdlt_token_pool(*[a[k] for k in order], None) == code, change
        msg = lib.sdlt_last_error()
        assert b"sdlt_token_pool" in msg and word in msg, (change, msg)


# ---- render() and the CLI ---------------------------------------------------------------------------------------------------------------------
def test_render_refuses_before_it_builds(tmp_path):
    from sd_lora_trainer_amd import render as R
    for kw, exc, msg in ((dict(kv_downsample=(0,), kv_downsample_pass="all"), ValueError, "kv_downsample"),
                         (dict(kv_downsample=(2,), kv_downsample_mode="cubic", kv_downsample_pass="all"), ValueError, "kv_downsample_mode"),
                         (dict(kv_downsample=(2,), kv_downsample_pass="second"), ValueError, "kv_downsample_pass"),
                         (dict(kv_downsample=(2,)), ValueError, "kv_downsample_pass='all'")):          # the default pass is "hires", and there is none
        with pytest.raises(exc, match=msg):
            R.render(_FakeLoaded(), ["a"], str(tmp_path / "o"), size=(64, 64), **kw)
    assert not os.path.exists(tmp_path / "o")


def test_cli_arguments(tmp_path, capsys):
    import unittest.mock as mock
    from sd_lora_trainer_amd import render as R
    base = ["--checkpoint", str(tmp_path / "nowhere"), "--out", str(tmp_path / "out")]
    for extra, msg in ((["--kv-downsample", "2"], "--kv-downsample-pass all"), (["--kv-downsample", "2", "--kv-downsample-pass", "hires"], "--kv-downsample-pass all"),
                       (["--kv-downsample-mode", "area"], "need --kv-downsample"), (["--kv-downsample-pass", "all"], "need --kv-downsample"),
                       (["--kv-downsample", "0", "--kv-downsample-pass", "all"], ">= 1"), (["--kv-downsample", "2.5", "--kv-downsample-pass", "all"], "--kv-downsample"),
                       (["--kv-downsample", "--kv-downsample-pass", "all"], "--kv-downsample"),
                       (["--kv-downsample", "2", "--kv-downsample-mode", "cubic", "--hires-scale", "2"], "--kv-downsample-mode"),
                       (["--kv-downsample", "2", "--kv-downsample-pass", "first", "--hires-scale", "2"], "--kv-downsample-pass")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    seen = {}

    def fake_render(loaded, prompts, out, **kw):
        seen.clear()
        seen.update(kw)
        return {}

    with mock.patch.object(R, "load_for_inference", lambda *a, **k: "loaded"), mock.patch.object(R, "render", fake_render):
        R.main(base)
        assert not [k for k in seen if k.startswith("kv_")]                                   # without the flag render() is called as before
        R.main(base + ["--kv-downsample", "2", "--hires-scale", "2"])
        assert (seen["kv_downsample"], seen["kv_downsample_mode"], seen["kv_downsample_pass"]) == ((2,), "nearest", "hires")
        R.main(base + ["--kv-downsample", "4", "2", "--kv-downsample-mode", "area", "--kv-downsample-pass", "all"])
        assert (seen["kv_downsample"], seen["kv_downsample_mode"], seen["kv_downsample_pass"]) == ((4, 2), "area", "all") and "hires" not in seen


def test_hires_render_first_pass_is_plain(job, tmp_path, monkeypatch):  # noqa: F811
    """A two-pass render with --kv-downsample: every first-pass sample() call comes without the option and pools nothing, every second-pass call carries
    it; --kv-downsample-pass all gives it to both; prompts.json records the setting; the pictures differ from the plain render's."""
    from sd_lora_trainer_amd import render as R
    config, ckdir = job
    log, pools = [], []
    real_sample, real_pool = SM.LatentSampler.sample, KR.token_pool

    def spy_sample(self, embeds, h, w, **kw):
        log.append((h, w, kw.get("kv_downsample"), kw.get("kv_downsample_mode")))
        out = real_sample(self, embeds, h, w, **kw)
        log.append((h, w, "unet", self.unet._kv_ds))
        return out

    monkeypatch.setattr(SM.LatentSampler, "sample", spy_sample)
    table = types.ModuleType("emu_kv_spy")
    table.__dict__.update({k: v for k, v in vars(KR.emu_kv).items() if not k.startswith("__")})
    table.token_pool = lambda x, y, **kw: (pools.append((kw["H"], kw["W"], kw["f"])), real_pool(x, y, **kw))[1]
    rt = lambda: unet_mod.Runtime("cpu", 1, act_dtype=torch.float32, ops=table)  # noqa: E731
    common = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", "32", "32", "--steps", "2", "--seed", "5", "--hires-size", "64", "64",
              "--hires-strength", "0.5"]
    R.main(common + ["--out", str(tmp_path / "plain")], runtime=rt())
    assert not pools and all(e[2] in (None, "unet") and e[3] is None for e in log) and "kv_downsample" not in json.load(open(tmp_path / "plain" / "prompts.json"))
    log.clear()
    R.main(common + ["--out", str(tmp_path / "kv"), "--kv-downsample", "2"], runtime=rt())
    assert log == [(8, 8, None, None), (8, 8, "unet", None), (16, 16, (2,), "nearest"), (16, 16, "unet", ((2,), "nearest"))]
    assert pools and set(pools) == {(16, 16, 2)}                                               # tiny15: the largest grid is the latent's; the second pass alone
    assert json.load(open(tmp_path / "kv" / "prompts.json"))["kv_downsample"] == dict(factors=[2], mode="nearest", passes="hires")
    name = next(f for f in sorted(os.listdir(tmp_path / "plain")) if f.startswith("img_00"))
    assert open(tmp_path / "kv" / name, "rb").read() != open(tmp_path / "plain" / name, "rb").read()
    log.clear()
    pools.clear()
    R.main(common + ["--out", str(tmp_path / "all"), "--kv-downsample", "2", "--kv-downsample-mode", "area", "--kv-downsample-pass", "all"], runtime=rt())
    assert [e for e in log if e[2] != "unet"] == [(8, 8, (2,), "area"), (16, 16, (2,), "area")] and set(pools) == {(8, 8, 2), (16, 16, 2)}
    assert json.load(open(tmp_path / "all" / "prompts.json"))["kv_downsample"] == dict(factors=[2], mode="area", passes="all")
