"""What the validation sampler costs per denoising iteration, three ways in ONE session (alternated, so that clocks and neighbours hit all of
them alike): (a) LatentSampler.sample as train() uses it (torch element-wise launches between the forwards), (b) the eager loop with the fused
sdlt_sampler_step kernel, (c) one replayed hipGraph per iteration.  SDXL topology (random weights), 128 x 128 latent, rank-16 adapters, 25 steps,
n = 1 and n = 2 images per batch ((a) samples the n images one after the other on its batch-2 instance).  --img2img adds the replayed graph
whose step launch is sdlt_sampler_step_img: (d) from init latents at strength 0.6 (15 of the 25 iterations run, no mask) and (e) masked inpainting at
strength 1 (all 25, the mask blend in every one); their time is divided by the iterations that ran.  --sampler / --sigmas add the replayed graph of
each named combination other than the default one - e.g. `--sampler dpmpp_2m` times (f) the iteration whose step launch is sdlt_sampler_step_ms
against (c) - and, with --img2img, its masked variant (`inp`).  The stochastic samplers (`euler_a`, `dpmpp_2m_sde`: step launch sdlt_sampler_step_sde)
are timed at eta = 1 with fixed seeds.  --guidance-rescale F adds (r) the default iteration with the sdlt_guidance pre-pass in it (phi = F) against (c).
--apg adds the default iteration with adaptive projected guidance - (p) sdlt_guidance_apg at eta 0, norm threshold 15, momentum -0.5; (q) the same with
--guidance-rescale's phi (0.7 when not given) - against (c) and (r), and, after the table, the device-event time of 50 back-to-back launches of
sdlt_guidance_apg (momentum and clip on, with and without phi) and of sdlt_guidance (phi) on one image of the latent's size.
--dynthresh adds (t) the default iteration with dynamic thresholding - sdlt_guidance_dyn at mimic 7, percentile 0.999, interpolate 1 - against (c), and,
after the table, the device-event time of 50 back-to-back launches of sdlt_guidance_dyn and of sdlt_guidance (--guidance-rescale's phi, 0.7 when not given)
on one image of the latent's size.
--freeu B1 B2 S1 S2 adds the default iteration with FreeU in its forward - (u) version 1, (v) version 2: six sdlt_freeu calls per forward on SDXL - against
(c); with --trace-iteration the traced loop runs it (version 2 with --freeu-v2).
--kv-downsample SPEC [SPEC ...] adds (k, l, m, ...) the default iteration with key / value token downsampling - SPEC = factors, largest grid first, and
optionally a mode: `2`, `2:area`, `4,2` - against (c); with --trace-iteration the traced loop runs the first SPEC.  --graph-only drops (a) and (b), which
take long at large latents.  --dump FILE saves the final latents of (c), for a bit comparison between two builds.

    python tools/render_bench.py [--out FILE] [--rounds 5] [--version sdxl] [--latent 128] [--n 1 2] [--img2img] [--sampler dpmpp_2m] [--sigmas karras] [--guidance-rescale 0.7] [--apg] [--dynthresh] [--freeu 1.3 1.4 0.9 0.2]
                                  [--kv-downsample 2 2:area 4,2] [--graph-only] [--dump FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_bench.py --trace-iteration --n 1      # kernel time of one iteration: sum the stats

Prints one table: wall milliseconds per iteration (median over the rounds, min .. max) per variant and n, per image in brackets.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(version, n, rank):
    import sd_lora_trainer_amd.unet as M
    from sd_lora_trainer_amd import sampler, topology
    from sd_lora_trainer_amd.train import _random_state
    cfg = topology.CONFIGS[version]
    sd = _random_state(topology.param_shapes(cfg), "cuda:0", seed=0)
    rt = M.Runtime("cuda:0", 2 * n)
    unet = M.UNet(rt, cfg, sd, lora_rank=rank)
    g = torch.Generator(device="cuda").manual_seed(1)
    for e in unet.arena.entries:
        e["A"].copy_(torch.randn(e["A"].shape, generator=g, device="cuda") / rank)
        e["B"].copy_(torch.randn(e["B"].shape, generator=g, device="cuda") * 0.02)
    unet.arena.refresh_shadows()
    smp = sampler.LatentSampler(rt, unet)
    smp.set_lora_scale(0.75)
    return cfg, smp


def embeds(cfg, n):
    g = torch.Generator(device="cuda").manual_seed(2)
    D = cfg["cross_dim"]
    P = cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"] if cfg["addition"] else 0
    mk = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    return [(mk(1, 77, D), mk(1, 77, D)) + ((mk(1, P), mk(1, P)) if cfg["addition"] else (None, None)) for _ in range(n)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launch_times(h, phi, launches=50, rounds=5):
    """Device-event microseconds per launch of the two guidance pre-passes on ONE image of h x h latent pixels (n = 1: one workgroup), `launches` of them
    back to back between two events, median (min .. max) of `rounds` alternated rounds after a warm-up.  The table row has momentum and clip on."""
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    hw = h * h
    src = torch.randn(2 * hw, 4, device="cuda", generator=g)
    src[hw:] = src[:hw] + 0.12 * torch.randn(hw, 4, device="cuda", generator=g)
    eps, mom = src.clone(), torch.zeros(hw, 4, device="cuda")
    ctr = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    tabs = {p: torch.tensor([[2.0, 0, 0, 0], [8.0, p, 0, 0], [8.0, p, 0, 0]], device="cuda") for p in (0.0, phi)}
    atab = torch.tensor([[2.0, 0, 0, 0], [0.0, 15.0, -0.5, 0], [0.0, 15.0, -0.5, 0]], device="cuda")
    kinds = {"sdlt_guidance_apg, phi 0": lambda: ops.guidance_apg(eps, tabs[0.0], atab, mom, ctr, 1),
             f"sdlt_guidance_apg, phi {phi:g}": lambda: ops.guidance_apg(eps, tabs[phi], atab, mom, ctr, 1),
             f"sdlt_guidance, phi {phi:g}": lambda: ops.guidance(eps, tabs[phi], ctr, 1)}
    times = {k: [] for k in kinds}
    for r in range(rounds + 1):
        for k, fn in kinds.items():
            eps.copy_(src)
            mom.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):                       # (in place: later launches see a guided prediction in both row blocks - the same traffic and arithmetic)
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
    lines = [f"# device-event us per launch, n = 1, hw = {hw}, {launches} launches back to back: median (min .. max) of {rounds} rounds, alternated"]
    for k, t in times.items():
        lines.append(f"   {k:<28} {statistics.median(t):>16.2f} {min(t):>8.2f} {max(t):>8.2f}")
    return lines


def dyn_launch_times(h, phi, launches=50, rounds=5):
    """launch_times for sdlt_guidance_dyn (guidance 8, mimic 7, percentile 0.999, interpolate 1) beside sdlt_guidance at phi, in the same session.  eps is
    restored before every timed sequence; within it later launches see a thresholded prediction in both row blocks - the same passes, traffic and histogram load (the deviations
    stay distinct).  The "first launch" row times one launch on the fresh pair, the events' own cost included."""
    from sd_lora_trainer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    hw = h * h
    src = torch.randn(2 * hw, 4, device="cuda", generator=g)
    src[hw:] = src[:hw] + 0.12 * torch.randn(hw, 4, device="cuda", generator=g)
    eps = src.clone()
    ctr = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    gtab = torch.tensor([[2.0, 0, 0, 0], [8.0, phi, 0, 0], [8.0, phi, 0, 0]], device="cuda")
    gdyn = torch.tensor([[2.0, 0, 0, 0], [8.0, 0, 0, 0], [8.0, 0, 0, 0]], device="cuda")
    dtab = torch.tensor([[2.0, 0, 0, 0], [7.0, 0.999, 1.0, 0], [7.0, 0.999, 1.0, 0]], device="cuda")
    kinds = {"sdlt_guidance_dyn": lambda: ops.guidance_dyn(eps, gdyn, dtab, ctr, 1),
             "sdlt_guidance_dyn, first launch": None,
             f"sdlt_guidance, phi {phi:g}": lambda: ops.guidance(eps, gtab, ctr, 1)}
    times = {k: [] for k in kinds}
    for r in range(rounds + 1):
        for k, fn in kinds.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eps.copy_(src)
            if fn is None:                                  # ONE launch on the fresh pair (distinct keys), the event overhead included
                e0.record()
                ops.guidance_dyn(eps, gdyn, dtab, ctr, 1)
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1) * 1e3
            else:
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1) * 1e3 / launches
            if r:
                times[k].append(t)
    lines = [f"# device-event us per launch, n = 1, hw = {hw}, {launches} launches back to back: median (min .. max) of {rounds} rounds, alternated"]
    for k, t in times.items():
        lines.append(f"   {k:<32} {statistics.median(t):>12.2f} {min(t):>8.2f} {max(t):>8.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--version", default="sdxl")
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--trace-iteration", action="store_true", help="run the eager fused loop once and exit (under rocprofv3 --kernel-trace --stats: kernel time per iteration = total / steps, without the one-off pack kernels)")
    ap.add_argument("--img2img", action="store_true", help="also time the graph sampler from init latents: strength 0.6 without a mask, strength 1 with a mask "
                    "(with --trace-iteration: run the masked eager loop instead of the txt2img one)")
    ap.add_argument("--sampler", nargs="+", choices=("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde"), default=["euler"], help="also time the graph sampler with these integrators")
    ap.add_argument("--sigmas", nargs="+", choices=("trailing", "karras"), default=["trailing"], help="... on these noise levels")
    ap.add_argument("--guidance-rescale", type=float, default=0.0, help="also time the default graph sampler with the guidance pre-pass at this rescale weight")
    ap.add_argument("--apg", action="store_true", help="also time the default graph sampler with adaptive projected guidance (with and without the rescale), and the pre-pass launches alone")
    ap.add_argument("--dynthresh", action="store_true", help="also time the default graph sampler with dynamic thresholding, and the pre-pass launch alone")
    ap.add_argument("--freeu", type=float, nargs=4, metavar=("B1", "B2", "S1", "S2"), default=None, help="also time the default graph sampler with FreeU, versions 1 and 2")
    ap.add_argument("--freeu-v2", action="store_true", help="with --trace-iteration --freeu: trace version 2")
    ap.add_argument("--kv-downsample", nargs="+", metavar="SPEC", default=[], help="also time the default graph sampler with key / value token downsampling: "
                    "factors, largest grid first, optionally :mode - 2  2:area  4,2")
    ap.add_argument("--graph-only", action="store_true", help="time the graph variants only (no torch loop, no eager fused loop)")
    ap.add_argument("--dump", default=None, help="save the final latents of variant c to this file (torch.save)")
    a = ap.parse_args()
    kvs = [(tuple(int(f) for f in spec.split(":")[0].split(",")), (spec.split(":") + ["nearest"])[1]) for spec in a.kv_downsample]
    h = a.latent
    lines = [f"# {a.version} topology, {h} x {h} latent, rank {a.rank}, {a.steps} steps, guidance 8; wall ms per denoising iteration: median (min .. max) of {a.rounds} rounds, alternated",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"{'n':>2} {'variant':<28} {'ms / iteration':>16} {'min':>8} {'max':>8} {'ms / iteration / image':>24}"]
    cfg1, smp1 = build(a.version, 1, a.rank)               # (a): today's loop, always a batch-2 instance
    for n in a.n:
        cfg, smp = (cfg1, smp1) if n == 1 else build(a.version, n, a.rank)
        em = embeds(cfg, n)
        noise = torch.randn(n, 4, h, h, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        one = lambda **kw: smp.sample(em if n > 1 else em[0], h, h, steps=a.steps, latents=noise, n_images=n, **kw)  # noqa: E731
        variants = {
            "a torch loop (train())": lambda: [smp1.sample(em[j], h, h, steps=a.steps, latents=noise[j:j + 1]) for j in range(n)],
            "b eager + fused kernel": lambda: one(fused=True),
            "c hipGraph per iteration": lambda: one(graph=True),
        }
        if a.graph_only:
            variants = {k: v for k, v in variants.items() if k.startswith("c ")}
        ran = {k: a.steps for k in variants}                # iterations a call runs
        x0 = mask = None
        if a.img2img:
            g = torch.Generator(device="cuda").manual_seed(4)
            x0 = 0.8 * torch.randn(n, 4, h, h, device="cuda", generator=g)
            mask = (torch.rand(n, 1, h, h, device="cuda", generator=g) > 0.5).float()
            variants["d graph, init latents 0.6"] = lambda: one(graph=True, init_latents=x0, strength=0.6)
            variants["e graph, inpaint 1.0"] = lambda: one(graph=True, init_latents=x0, strength=1.0, mask=mask)
            ran["d graph, init latents 0.6"], ran["e graph, inpaint 1.0"] = min(int(a.steps * 0.6), a.steps), a.steps
        if a.guidance_rescale:
            variants["r graph, guidance rescale"], ran["r graph, guidance rescale"] = (lambda: one(graph=True, guidance_rescale=a.guidance_rescale)), a.steps
        if a.apg:
            phi = a.guidance_rescale or 0.7
            variants["p graph, APG"], ran["p graph, APG"] = (lambda: one(graph=True, apg=(0.0, 15.0, -0.5))), a.steps
            variants["q graph, APG + rescale"], ran["q graph, APG + rescale"] = (lambda: one(graph=True, apg=(0.0, 15.0, -0.5), guidance_rescale=phi)), a.steps
        if a.dynthresh:
            variants["t graph, dynthresh"], ran["t graph, dynthresh"] = (lambda: one(graph=True, dynthresh=(7.0, 0.999, 1.0))), a.steps
        if a.freeu:
            for tag, ver in (("u", 1), ("v", 2)):
                fz = dict(zip(("b1", "b2", "s1", "s2"), a.freeu), version=ver)
                variants[f"{tag} graph, FreeU v{ver}"], ran[f"{tag} graph, FreeU v{ver}"] = (lambda fz=fz: one(graph=True, freeu=fz)), a.steps
        for tag, (fs, mode) in zip("klmnop", kvs):
            name = f"{tag} graph, kv {','.join(map(str, fs))} {mode}"
            variants[name], ran[name] = (lambda fs=fs, mode=mode: one(graph=True, kv_downsample=fs, kv_downsample_mode=mode)), a.steps
        extra = [(s, k) for s in a.sampler for k in a.sigmas if (s, k) != ("euler", "trailing")]
        sd = lambda s: dict(seeds=list(range(n))) if s in ("euler_a", "dpmpp_2m_sde") else {}  # noqa: E731
        for tag, (s, k) in zip("fghij", extra):
            name = f"{tag} graph, {s} {k}"
            variants[name], ran[name] = (lambda s=s, k=k: one(graph=True, sampler=s, sigmas=k, **sd(s))), a.steps
            if a.img2img:
                variants[name + " inp"], ran[name + " inp"] = (lambda s=s, k=k: one(graph=True, sampler=s, sigmas=k, init_latents=x0, strength=1.0, mask=mask, **sd(s))), a.steps
        if a.trace_iteration:                               # the kernels of `steps` eager iterations (+ the one-off weight packing of the first)
            fu = dict(freeu=dict(zip(("b1", "b2", "s1", "s2"), a.freeu), version=2 if a.freeu_v2 else 1)) if a.freeu else {}
            if kvs:
                fu.update(kv_downsample=kvs[0][0], kv_downsample_mode=kvs[0][1])
            one(fused=True, **(dict(init_latents=x0, strength=1.0, mask=mask) if a.img2img else {}), **(dict(sampler=extra[0][0], sigmas=extra[0][1], **sd(extra[0][0])) if extra else {}), **fu)
            torch.cuda.synchronize()
            return
        for k, fn in variants.items():                      # warm-up: buffers, packed weights, the capture
            out = fn()
            if a.dump and k.startswith("c "):
                torch.save(out.cpu(), a.dump)
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn) * 1e3 / ran[k])
        for k, t in times.items():
            med = statistics.median(t)
            lines.append(f"{n:>2} {k:<28} {med:>16.3f} {min(t):>8.3f} {max(t):>8.3f} {med / n:>24.3f}")
        if n != 1:
            del smp
            torch.cuda.empty_cache()
    if a.apg:
        lines += launch_times(h, a.guidance_rescale or 0.7)
    if a.dynthresh:
        lines += dyn_launch_times(h, a.guidance_rescale or 0.7)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
