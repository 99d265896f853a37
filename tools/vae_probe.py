"""Times the full-size VAE (SD/SDXL configuration, random weights): decode of a latent (default 128x128: a 1024 px render) and encode of the picture of
that size, by device events, with the peak memory above the weights and the input.
python tools/vae_probe.py [--attention dense|flash] [--latent H W] [--pass decode|encode|both] [--dump FILE]"""
import argparse
import sys

import torch

sys.path.insert(0, ".")
from oracle import vae_ref as V          # noqa: E402  (weights generator only)
from sd_lora_trainer_amd import vae      # noqa: E402
import sd_lora_trainer_amd.unet as M     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--attention", choices=vae.VAE_ATTENTIONS, default="dense")
ap.add_argument("--latent", type=int, nargs=2, default=(128, 128), metavar=("H", "W"))
ap.add_argument("--pass", dest="passes", choices=("decode", "encode", "both"), default="both")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--dump", default=None, help="save the decoded picture (fp32 tensor) here")
a = ap.parse_args()
cfg = V.CONFIGS["sd"]
sd = {k: v.cuda() for k, v in V.init_state(cfg, seed=0).items()}
h, w = a.latent
g = torch.Generator(device="cuda").manual_seed(1)
for name in (("decode", "encode") if a.passes == "both" else (a.passes,)):
    rt = M.Runtime("cuda:0", 1)
    if name == "decode":
        mod, x = vae.VaeDecoder(rt, sd, attention=a.attention), torch.randn(1, 4, h, w, device="cuda", generator=g)
        fn = lambda: mod.decode(x)  # noqa: E731
    else:
        mod, x = vae.VaeEncoder(rt, sd, attention=a.attention), torch.tanh(torch.randn(1, 3, 8 * h, 8 * w, device="cuda", generator=g))
        fn = lambda: mod.encode_moments(x)  # noqa: E731
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()                            # the first pass allocates the plan's buffers: its peak is the pass's footprint
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"{name} {a.attention} latent {h}x{w}: {min(ms):.1f} ms (min of {a.repeats}: {' '.join(f'{m:.1f}' for m in ms)}), peak {peak / 2**20:.0f} MiB above weights and input, "
          f"out {tuple(out.shape)}, finite {bool(torch.isfinite(out).all())}")
    if a.dump and name == "decode":
        torch.save(out.cpu(), a.dump)
    del mod, out, fn
    torch.cuda.empty_cache()
