"""Adaptive projected guidance on the MI355X: sdlt_guidance_apg against its contract (tests/apg_ref.guidance_apg: fp64 sums, everything else fp32 in the
contract's order) - exact where the contract takes no sum, within a measured bound elsewhere - over three steps with a running average, at degenerate
and hostile inputs, its independence of the batch, its refusals, LatentSampler.sample(apg=) - graph == fused == torch loop, one capture for every
setting, the restart of the running average inside the replayed graph, apg=None - the fused path against the fp32 reference loop driven by the oracle
UNet, and `python -m sd_lora_trainer_amd.render --apg` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import apg_ref as AR
from tests.test_guidance_gpu import _rel
from tests.test_multistep_gpu import _cuda, _figures, _inputs, _run, _setup
from tests.test_sampler_gpu import TOL_COS, TOL_REL          # the bars of the sampler against the fp32 oracle loop

pytestmark = pytest.mark.gpu

# max |e_gpu - e_ref| / max |e_ref| per image (tests/test_guidance_gpu._rel) over every row of test_kernel_against_contract and the hostile input of
# test_degenerate_and_hostile_input, measured on the MI355X: 2.492e-7, at hw = 35, (eta, tau, beta) = (1, 0, 0.4), phi = 0.7, row 1 (the
# rows without rescale stay below 1.1e-7; the hostile input - a mean 100 standard deviations from zero - gave 1.754e-7 and does not govern here).
# The reference takes the three sums and the two standard deviations in fp64, the kernel from fp32 sums in a fixed order; every other operation is
# the same.  The bar is four times the measured value and may never exceed 1e-5 (tests/test_guidance_gpu.py's rule for RESCALE_TOL)
MEASURED = 2.492e-7
APG_TOL = min(4 * MEASURED, 1e-5)
N, HWS = 3, (1, 35, 351, 3 * 960)                             # one pixel; below one wave; no multiple of the wave or the workgroup; more pixels than threads
G = 7.5
SETTINGS = ((0.0, 0.0, 0.0), (0.3, 2.5, 0.0), (0.0, 15.0, -0.5), (1.0, 0.0, 0.4))
K = 3


def _pair(n, hw, seed, spread=0.12, mean=0.05):
    """eps fp32 [2n hw, 4]: a negative prediction and a positive one close to it, as a UNet's two rows are."""
    g = torch.Generator().manual_seed(seed)
    en = torch.randn(n, 1, hw, 4, generator=g) * 1.1 + mean
    return torch.cat([en, en + spread * torch.randn(n, 1, hw, 4, generator=g)], 1).reshape(2 * n * hw, 4).contiguous()


def _tabs(g, phi, apg, k=K):
    gtab, atab = torch.zeros(1 + k + 2, 4), torch.zeros(1 + k + 2, 4)             # buffers longer than the tables, as the sampler's
    gtab[0, 0] = atab[0, 0] = k
    gtab[1:1 + k, 0], gtab[1:1 + k, 1] = g, phi
    atab[1:1 + k, :3] = torch.tensor(apg)
    return gtab, atab


def _launch(eps, gtab, atab, mom, row, n, ticket=5):
    """-> (the rewritten eps, the buffer afterwards | None), on the CPU; the counter must come back as it went in."""
    from sd_lora_trainer_amd import ops
    e, m = eps.cuda().clone(), None if mom is None else mom.cuda().clone()
    ctr = torch.tensor([row, ticket], dtype=torch.int32).cuda()
    ops.guidance_apg(e, gtab.cuda(), atab.cuda(), m, ctr, n)
    torch.cuda.synchronize()
    assert ctr.cpu().tolist() == [row, ticket]
    return e.cpu(), None if m is None else m.cpu()


def _ref(eps, gtab, atab, mom, row, n):
    m = None if mom is None else mom.clone()
    return AR.guidance_apg(eps.clone(), gtab, atab, m, torch.tensor([row, 0], dtype=torch.int32), n), m


@pytest.fixture(scope="module")
def eps_cases():
    return {hw: [_pair(N, hw, 11 + 7 * row) for row in range(K)] for hw in HWS}


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def test_kernel_against_contract(eps_cases):
    """g in {1, 7.5} x the four settings x phi in {0, 0.7}, rows 0, 1, 2 in sequence with fresh eps each and a buffer NaN-filled before row 0; the
    buffer is compared after every row.  It takes no sum: its bits are the contract's."""
    worst = 0.0
    for hw in HWS:
        # tau = 2.5 of the second setting against this input: the clip is active at the two large sizes and idle at the two small ones
        d = [(e.view(N, 2, -1)[:, 1] - e.view(N, 2, -1)[:, 0], e.view(N, 2, -1)[:, 1]) for e in eps_cases[hw]]
        cs = np.concatenate([AR.scalars(dd, ep, 2.5)[0] for dd, ep in d])
        assert bool((cs < 1.0).all()) if hw >= 351 else bool((cs == 1.0).all()), (hw, cs)
        for g in (1.0, G):
            for apg in SETTINGS:
                for phi in (0.0, 0.7):
                    gtab, atab = _tabs(g, phi, apg)
                    mom_g = mom_r = torch.full((N * hw, 4), float("nan"))
                    for row in range(K):
                        eps, m_in = eps_cases[hw][row], mom_r
                        (got, mom_g), (ref, mom_r) = _launch(eps, gtab, atab, mom_g, row, N), _ref(eps, gtab, atab, mom_r, row, N)
                        v = got.view(N, 2, hw, 4)
                        assert bool(torch.isfinite(got).all()) and torch.equal(v[:, 0], v[:, 1]), (hw, g, apg, phi, row)      # both row blocks hold e
                        if g == 1.0:                                             # guidance off: e_pos exactly, the buffer untouched
                            assert torch.equal(v[:, 0], eps.view(N, 2, hw, 4)[:, 1]) and torch.equal(got, ref) and bool(torch.isnan(mom_g).all())
                            continue
                        if apg[2] != 0.0:
                            assert torch.equal(mom_g, mom_r) and bool(torch.isfinite(mom_g).all()), (hw, apg, phi, row)
                        else:
                            assert bool(torch.isnan(mom_g).all())
                        rel = _rel(got, ref, N)
                        worst = max(worst, rel)
                        print(f"sdlt_guidance_apg hw={hw} apg={apg} phi={phi} row={row}: rel {rel:.3e}")
                        assert rel <= APG_TOL, (hw, apg, phi, row, rel)
                        if row == K - 1 and hw == 351:                           # the published function in fp64 on the same inputs (the last row)
                            e64 = eps.view(N, 2, hw, 4).double()
                            a32 = tuple(float(x) for x in atab[1, :3])
                            m64 = None if apg[2] == 0.0 else m_in.view(N, hw, 4).double()      # (the buffer as the row found it)
                            pub, _ = AR.published(e64[:, 1], e64[:, 0], G, a32[0], a32[1], a32[2], m64)
                            if phi:
                                pub = AR.GR.rescale(e64[:, 1], pub, float(np.float32(phi)))
                            assert float((v[:, 0].double() - pub).abs().max()) <= 32 * 2.0 ** -24 * float(pub.abs().max())
    print(f"sdlt_guidance_apg: worst rel over the rows with g != 1 = {worst:.3e} (bar {APG_TOL:.3e})")
    assert worst <= APG_TOL


def test_degenerate_and_hostile_input():
    hw = 351
    big = _pair(N, hw, 21)
    zero_pos = big.clone().view(N, 2, hw, 4)
    zero_pos[:, 1] = 0.0
    zero_pos = zero_pos.view(-1, 4).contiguous()
    same = big.clone().view(N, 2, hw, 4)
    same[:, 0] = same[:, 1]
    same = same.view(-1, 4).contiguous()
    nan_mom = torch.full((N * hw, 4), float("nan"))
    for phi in (0.0, 0.7):
        # e_pos = 0: S_pp = 0, a = 0; without a clip every scalar is exact, so the bits are the contract's
        for apg in ((0.3, 0.0, 0.0), (0.3, 0.0, -0.5)):
            gtab, atab = _tabs(G, phi, apg)
            (got, m), (ref, mr) = _launch(zero_pos, gtab, atab, nan_mom, 0, N), _ref(zero_pos, gtab, atab, nan_mom, 0, N)
            assert bool(torch.isfinite(got).all()) and torch.equal(got, ref) and (apg[2] == 0.0 or torch.equal(m, mr)), (phi, apg)
        # e_pos = e_neg with a clip: the norm is 0, c = 1, the update is 0 and e = e_pos - through the rescale too (r = 1 exactly)
        for apg in ((0.0, 15.0, 0.0), (0.5, 2.5, -0.5)):
            gtab, atab = _tabs(G, phi, apg)
            got, m = _launch(same, gtab, atab, nan_mom, 0, N)
            ref, _ = _ref(same, gtab, atab, nan_mom, 0, N)
            assert bool(torch.isfinite(got).all()) and torch.equal(got, ref), (phi, apg)
            if phi == 0.0:
                assert torch.equal(got, same)
            assert apg[2] == 0.0 or bool((m == 0).all())
        # tau far above the norm: c == 1 exactly, the clip changes no bit
        ga, aa = _tabs(G, phi, (0.3, 1e6, -0.5))
        gb, ab = _tabs(G, phi, (0.3, 0.0, -0.5))
        (a, ma), (b, mb) = _launch(big, ga, aa, nan_mom, 0, N), _launch(big, gb, ab, nan_mom, 0, N)
        assert torch.equal(a, b) and torch.equal(ma, mb) and _rel(a, _ref(big, ga, aa, nan_mom, 0, N)[0], N) <= APG_TOL
    # a mean a hundred standard deviations from zero: the same bound
    worst = 0.0
    hostile = [_pair(N, hw, 31 + row, mean=100.0) for row in range(2)]
    for apg in ((0.0, 15.0, -0.5), (0.3, 2.5, 0.0)):
        for phi in (0.0, 0.7):
            gtab, atab = _tabs(G, phi, apg)
            mg = mr = nan_mom
            for row in range(2):
                (got, mg), (ref, mr) = _launch(hostile[row], gtab, atab, mg, row, N), _ref(hostile[row], gtab, atab, mr, row, N)
                rel = _rel(got, ref, N)
                worst = max(worst, rel)
                print(f"sdlt_guidance_apg hostile (100 + N(0, 1.1)) apg={apg} phi={phi} row={row}: rel {rel:.3e} (bar {APG_TOL:.3e})")
                assert bool(torch.isfinite(got).all()) and rel <= APG_TOL
    print(f"sdlt_guidance_apg: worst rel at the hostile input = {worst:.3e}")


def test_batch_independence_and_repeatability(eps_cases):
    for hw in HWS:
        eps = eps_cases[hw][0]
        gtab, atab = _tabs(G, 0.7, (0.3, 2.5, -0.5))
        mom = _pair(N, hw, 3).view(N, 2, hw, 4)[:, 0].reshape(N * hw, 4).contiguous()      # a running average from an earlier step
        (a, ma), (b, mb) = _launch(eps, gtab, atab, mom, 1, N), _launch(eps, gtab, atab, mom, 1, N)
        assert torch.equal(a, b) and torch.equal(ma, mb)                         # two runs, the same bits
        alone, m1 = _launch(eps.view(N, 2 * hw, 4)[1].contiguous(), gtab, atab, mom.view(N, hw, 4)[1].contiguous(), 1, 1)
        assert torch.equal(alone, a.view(N, 2 * hw, 4)[1]) and torch.equal(m1, ma.view(N, hw, 4)[1])      # image 1 of n = 3 is the n = 1 launch on its rows
        assert not torch.equal(a.view(N, 2 * hw, 4)[0], a.view(N, 2 * hw, 4)[1]) and not torch.equal(ma, mom)
        # without a buffer there is no momentum, whatever the table says
        c, _ = _launch(eps, gtab, atab, None, 1, N)
        d, _ = _launch(eps, *_tabs(G, 0.7, (0.3, 2.5, 0.0)), None, 1, N)
        assert torch.equal(c, d) and not torch.equal(c, a)


def test_refusals_launch_nothing():
    from sd_lora_trainer_amd import _lib
    lib = _lib.load()
    n, hw = 2, 35
    eps0, mom0 = _pair(n, hw, 5), torch.full((n * hw + 8, 4), 3.0)
    eps, mom = eps0.cuda(), mom0.cuda()
    gtab, atab = (t.cuda() for t in _tabs(G, 0.7, (0.0, 15.0, -0.5)))
    ctr = torch.tensor([1, 0], dtype=torch.int32).cuda()
    ok = dict(eps=eps.data_ptr(), gtab=gtab.data_ptr(), atab=atab.data_ptr(), mom=mom.data_ptr(), ctr=ctr.data_ptr(), n=n, hw=hw, gtab_rows=gtab.shape[0])
    stream = torch.cuda.current_stream().cuda_stream
    for change in (dict(eps=None), dict(gtab=None), dict(atab=None), dict(ctr=None), dict(n=0), dict(hw=0), dict(hw=-1), dict(gtab_rows=1), dict(eps=ok["eps"] + 4),
                   dict(eps=ok["eps"] + 8), dict(mom=ok["mom"] + 4), dict(mom=ok["eps"]), dict(mom=ok["eps"] + 16), dict(mom=ok["eps"] + 2 * n * hw * 16 - 16),
                   dict(mom=ok["eps"] - n * hw * 16 + 16)):
        p = _lib.GuidanceApgParams(**dict(ok, **change))
        rc = lib.sdlt_guidance_apg(C.byref(p), stream)
        torch.cuda.synchronize()
        assert rc < 0 and b"sdlt_guidance_apg" in lib.sdlt_last_error(), change
        assert torch.equal(eps.cpu(), eps0) and torch.equal(mom.cpu(), mom0) and ctr.cpu().tolist() == [1, 0], change


# ---- LatentSampler ---------------------------------------------------------------------------------------------------------------------
H, W, STEPS = 8, 12, 4
APG = (0.0, 15.0, -0.5)


@pytest.mark.parametrize("version", ["tiny15", "tinyxl"])
def test_sampler_paths_captures_and_restart(version):
    cfg, sd, lora, smp = _setup(version, n=1)
    embeds, noise, x0 = _inputs(cfg, 5, H, W, 1)
    em = _cuda(embeds)[0]
    base = dict(steps=STEPS, latents=noise.cuda(), guidance_scale=8.0)
    sd_kw = lambda s: dict(sampler=s, **(dict(seeds=[21]) if s != "euler" else {}))  # noqa: E731
    plain = smp.sample(em, H, W, graph=True, **base).cpu()
    assert torch.equal(smp.sample(em, H, W, graph=True, apg=None, **base).cpu(), plain)      # apg=None is the call without the argument
    guided = smp.sample(em, H, W, graph=True, guidance_rescale=0.7, **base).cpu()
    before = {d: dict(getattr(smp, d)) for d in ("_graphs", "_guided_graphs")}
    assert len(before["_graphs"]) == 1 and len(before["_guided_graphs"]) == 1 and smp._apg_graphs == {}
    first = {}
    for kind in ("euler", "dpmpp_2m_sde"):
        kw = dict(base, apg=APG, **sd_kw(kind))
        out = [smp.sample(em, H, W, **path, **kw).cpu() for path in ({}, dict(fused=True), dict(graph=True))]
        assert bool(torch.isfinite(out[0]).all()) and torch.equal(out[0], out[1]) and torch.equal(out[1], out[2]), kind
        assert not torch.equal(out[2], plain)
        first[kind] = out[2]
        held = dict(smp._apg_graphs)
        # a second picture on the captured graph: the running average restarts inside the graph
        again = smp.sample(em, H, W, graph=True, **kw).cpu()
        assert torch.equal(again, out[2]) and list(smp._apg_graphs) == list(held) and all(smp._apg_graphs[k] is v for k, v in held.items())
        # another setting, with rescale: table contents - the same capture, other bits, and still the torch loop's
        other = dict(kw, apg=(0.5, 2.0, 0.25), guidance_rescale=0.3)
        o = [smp.sample(em, H, W, **path, **other).cpu() for path in ({}, dict(graph=True))]
        assert torch.equal(o[0], o[1]) and not torch.equal(o[1], out[2]) and list(smp._apg_graphs) == list(held)
        assert torch.equal(smp.sample(em, H, W, graph=True, **kw).cpu(), out[2])
    assert len(smp._apg_graphs) == 2 and all(k[-1] == "apg" for k in smp._apg_graphs)
    for d, was in before.items():                                                # the other captures: same keys, same graphs, same bits
        now = getattr(smp, d)
        assert list(now) == list(was) and all(now[k] is v for k, v in was.items()), d
    assert torch.equal(smp.sample(em, H, W, graph=True, **base).cpu(), plain)
    assert torch.equal(smp.sample(em, H, W, graph=True, guidance_rescale=0.7, **base).cpu(), guided)
    # a fresh sampler's first call gives what this one gave first and again
    _, _, _, fresh = _setup(version, n=1)
    for kind in ("euler", "dpmpp_2m_sde"):
        assert torch.equal(fresh.sample(em, H, W, graph=True, apg=APG, **base, **sd_kw(kind)).cpu(), first[kind]), kind


@pytest.mark.parametrize("kind,sigkind", [("euler", "trailing"), ("dpmpp_2m", "karras")])
def test_fused_against_oracle_loop(kind, sigkind):
    """The fused path with APG (eta 0, a threshold that clips, momentum -0.5), rescale 0.7 and guidance on the middle four of six sigmas against the fp32
    reference loop (tests/apg_ref.py: the published function) driven by the oracle UNet, at the bars of DESIGN 4.21.  Measured on the MI355X
    (cos / rel-L2): see DESIGN 4.35."""
    from sd_lora_trainer_amd import sampler as SM
    h = w = 16
    steps, phi, apg = 6, 0.7, (0.0, 4.0, -0.5)
    cfg, sd, lora, smp = _setup("tinyxl")
    embeds, noise, x0 = _inputs(cfg, 5, h, w, 1)
    sig = SM.EulerDiscrete().set_timesteps(steps, 0, sigkind).sigmas.astype(np.float64)
    interval = (float(sig[5] + sig[4]) / 2, float(sig[1] + sig[0]) / 2)
    kw = dict(sampler=kind, sigmas=sigkind, guidance_scale=8.0, guidance_rescale=phi, guidance_interval=interval)
    ref = AR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, apg=apg, **dict(kw, guidance_rescale=float(np.float32(phi))))
    got = smp.sample(_cuda(embeds)[0], h, w, steps=steps, latents=noise.cuda(), fused=True, apg=apg, **kw).cpu()
    assert bool(torch.isfinite(got).all())
    cos, rel = _figures(got, ref)
    print(f"tinyxl {kind} {sigkind} apg {apg} rescale {phi} interval: cos {cos:.6f} rel {rel:.4f}")
    assert cos >= TOL_COS and rel <= TOL_REL, (kind, cos, rel)
    # the controls are what the reference was given: the same loop with plain guidance ends further away
    rel0 = _figures(got, AR.GR.sample_latents(cfg, sd, lora, 0.75, embeds[0], noise, steps, **dict(kw, guidance_rescale=float(np.float32(phi)))))[1]
    print(f"    against the same loop without apg: rel {rel0:.4f}")
    assert rel0 > rel


# ---- render --apg ------------------------------------------------------------------------------------------------------------------------
def test_render_cli_apg(tmp_path, monkeypatch):
    from PIL import Image
    from sd_lora_trainer_amd import render as R
    from sd_lora_trainer_amd import train as T
    from sd_lora_trainer_amd.config import TrainingConfig
    from tests.test_driver_cpu import _tokenizer_dir
    monkeypatch.chdir(tmp_path)
    tok_dir, _ = _tokenizer_dir(tmp_path)
    cfg = TrainingConfig(lora_training_urls="synthetic:4", concept_mode="object", name="apg job", seed=3, resolution=128, train_batch_size=1, max_train_steps=1,
                         checkpointing_steps=1000, lora_rank=8, n_sample_imgs=0, output_dir=str(tmp_path / "job"),
                         pretrained_model={"path": "synthetic:tiny15", "tokenizer_path": tok_dir})
    config, ckdir = _run(T.train(cfg))
    Wp, Hp = 96, 64
    base = ["--checkpoint", ckdir, "--prompt", "a photo of <concept>", "--size", str(Wp), str(Hp), "--steps", "6", "--seed", "11"]
    runs = dict(default=[], apg=["--apg"], again=["--apg"], tuned=["--apg", "--apg-eta", "0.5", "--apg-norm-threshold", "1", "--apg-momentum", "0"],
                all=["--apg", "--guidance-rescale", "0.7", "--sampler", "dpmpp_2m", "--sigmas", "karras"])
    outs, name = {}, "img_00_seed11_scale0.85.jpg"
    for tag, extra in runs.items():
        outs[tag] = str(tmp_path / f"out_{tag}")
        R.main(base + extra + ["--out", outs[tag]])
        assert sorted(f for f in os.listdir(outs[tag]) if f.endswith(".jpg")) == sorted([name, "grid_scale0.85.jpg"]), tag
        assert Image.open(os.path.join(outs[tag], name)).size == (Wp, Hp)
    raw = {tag: open(os.path.join(d, name), "rb").read() for tag, d in outs.items()}
    assert raw["apg"] == raw["again"]
    for a, b in (("apg", "default"), ("tuned", "default"), ("tuned", "apg"), ("all", "apg")):
        assert raw[a] != raw[b], (a, b)
    meta = json.load(open(os.path.join(outs["apg"], "prompts.json")))
    assert meta["apg"] == dict(eta=0.0, norm_threshold=15.0, momentum=-0.5)
    assert json.load(open(os.path.join(outs["tuned"], "prompts.json")))["apg"] == dict(eta=0.5, norm_threshold=1.0, momentum=0.0)
    assert "apg" not in json.load(open(os.path.join(outs["default"], "prompts.json")))
