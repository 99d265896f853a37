"""Render from a saved checkpoint: what a user does first when a job has ended - load the checkpoint directory train() wrote and make pictures with
prompts of their own (the reference's trainer/checkpoint.py:223 `load_checkpoint`, trainer/inference.py:409-493 `render_images_eval` and
scripts/test_inference.py: own prompt list, a sweep over `lora_scale`, a non-square `render_size`, own step count / guidance / seeds).

    python -m sd_lora_trainer_amd.render --checkpoint DIR --out DIR [--prompt TEXT ...] [--n-validation N] [--lora-scale X ...] [--size W H]
                                         [--steps N] [--guidance G] [--seed S] [--images-per-batch N] [--eager]
                                         [--init-image PATH [--strength S] [--mask PATH | --change-map PATH] [--mask-blur SIGMA]] [--sampler euler|dpmpp_2m|euler_a|dpmpp_2m_sde] [--eta F]
                                         [--sigmas trailing|karras] [--guidance-rescale F] [--guidance-interval SIGMA_LO SIGMA_HI]
                                         [--apg [--apg-eta F] [--apg-norm-threshold F] [--apg-momentum F]]
                                         [--dynthresh [MIMIC] [--dynthresh-percentile F] [--dynthresh-interpolate F]]
                                         [--negative-prompt TEXT] [--freeu B1 B2 S1 S2 [--freeu-v2]]
                                         [--hires-scale F | --hires-size W H] [--hires-strength F] [--hires-steps N] [--hires-upscaler latent|pixel]
                                         [--hires-resample nearest|bilinear|bicubic] [--heatmap [WORD ...]] [--heatmap-grid max|min]
                                         [--kv-downsample F [F2 ...]] [--kv-downsample-mode nearest|area] [--kv-downsample-pass hires|all]
                                         [--vae-tile [T]] [--vae-tile-overlap O] [--tile-diffusion [T]] [--tile-diffusion-overlap O]
                                         [--region MASK.png|x0,y0,x1,y1 PROMPT ...] [--region-feather SIGMA] [--region-base F] [--region-bootstrap SHARE]
                                         [--unet F] [--text-encoder F] [--text-encoder-2 F] [--vae F] [--tokenizer DIR]

DIR is a checkpoint directory of train(): training_args.json (the job's TrainingConfig), adapter_config.json + the kohya adapter file
(`*_lora.safetensors`, `lora_te1_ / lora_te2_` keys for text-encoder adapters, `.dora_scale` for DoRA), the embeddings file and
special_params.json; a full fine-tune (`is_lora` false) has diffusion_pytorch_model.safetensors instead of the adapter files.  The base model is
the job's `pretrained_model` unless given (anything train() accepts, "synthetic:<version>" included).  The sampler runs each denoising iteration
as one replayed hipGraph (sampler.LatentSampler.sample(graph=True)); --eager issues the same kernels from Python.

--init-image starts every image from that picture instead of pure noise (img2img): it is resized to --size (bicubic), encoded by the VAE encoder
of the loaded stack (the posterior's mean times the scaling factor: deterministic) and noised to the point of the schedule that --strength
selects (default 0.6; the last int(steps * strength) steps run).  --mask (white: regenerate, black: keep; nearest-resized to the latent grid)
keeps the black region of the init image: it is put back after every step, and comes out as the encoded image exactly.

--change-map MAP.png is differential diffusion (Levin & Fried 2023, "Giving Each Pixel Its Strength"): the map's luminance, area-resized to the latent
grid, gives every pixel a strength of its own - white the whole --strength, black keep (the encoded image exactly, like a black mask), grey in between.
A pixel with value c is held on the init image's noised trajectory for the first (1 - c) share of the steps that run, then released to finish on its
own: a selection per pixel and step inside the step launch (sdlt_sampler_step_dd), never a mix of two pictures, so a soft edge leaves no halo where
--mask's fixed blend does.  --mask-blur SIGMA (latent pixels) blurs the map on the device first (sdlt_blur_planes, edges replicated) - a hard mask
painted by hand becomes a soft change map; with --mask it blurs the mask, which then goes down the blend path as before.  --change-map excludes --mask
and the hires pass; with every sampler and noise schedule.  Without the flags nothing changes.

--sampler dpmpp_2m integrates with DPM-Solver++ (2M), the second-order multistep solver (sampler.DpmSolverPP2M; the step launch is then
sdlt_sampler_step_ms), instead of first-order Euler: the same trajectory error in about half the steps.  --sigmas karras spaces the noise levels as
Karras et al. 2022 (rho = 7) instead of by trailing timesteps; it combines with either sampler, and both combine with --init-image / --mask.

--sampler euler_a / dpmpp_2m_sde are the stochastic samplers (Euler ancestral; the SDE form of DPM-Solver++ (2M)): fresh Gaussian noise after every
step, made inside the step launch (sdlt_sampler_step_sde) from the image's seed, the step and the pixel, so the replayed graph needs no host work and
the same --seed gives the same files.  --eta (default 1; 0 is the deterministic limit) scales that noise; it is an error with the other samplers.

--guidance-rescale F (0 .. 1) rescales the guided prediction of every step to the standard deviation of the positive one and blends it in with weight
F (Lin et al. 2024, section 3.4; diffusers' guidance_rescale): it takes the over-exposure out of a strong --guidance, and a v-prediction base needs
it.  --guidance-interval SIGMA_LO SIGMA_HI applies guidance only at the steps whose noise level lies in (SIGMA_LO, SIGMA_HI] (Kynkaanniemi et al.
2024).  Both are evaluated by one more launch per iteration (sdlt_guidance) inside the replayed graph; without them nothing changes.
--negative-prompt TEXT replaces the fixed negative prompt of the training-time renders.

--apg is adaptive projected guidance (Sadat et al. 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales"; diffusers'
normalized_guidance, ComfyUI's APG node), the fix for the burnt contrast of a strong --guidance that works before the damage is done: the guidance update
e_pos - e_neg is averaged over the steps with a negative momentum, its norm over the image is clipped, and its part parallel to the positive prediction -
the part that drives saturation - is scaled down.  The defaults are the paper's SDXL settings: --apg-eta 0 (the parallel part is dropped; 1 keeps it),
--apg-norm-threshold 15 (0: no clip), --apg-momentum -0.5 (0: none); the three flags are errors without --apg.  One launch (sdlt_guidance_apg) in
sdlt_guidance's place inside the replayed graph, the running average in a device buffer the launch restarts at the first step, so it needs no weights and
no host work.  It works on the noise prediction (the paper and ComfyUI project the denoised value).  With every sampler, noise schedule,
--guidance-rescale, --guidance-interval, --init-image / --mask / --change-map, --tile-diffusion, --region and --heatmap; both passes of a hires render
use it, each with a running average of its own.  Without the flag nothing changes.

--dynthresh [MIMIC] is dynamic thresholding (the "Dynamic Thresholding (CFG scale fix)" extension of A1111 / ComfyUI / SwarmUI, a latent-space form of
Imagen's dynamic thresholding): sample at --guidance 12-20 for its prompt adherence, but give every latent channel of the prediction the value range it
would have had at the mild scale MIMIC (default 7).  Per image and channel the guided prediction is centred on its mean, clamped to max(the largest
deviation of the MIMIC-scale prediction, the --dynthresh-percentile quantile of its own deviations; default 0.999, 1: the maximum) and scaled back to the
MIMIC prediction's range; --dynthresh-interpolate F (default 1) blends the result with the plain guided prediction.  The defaults are this project's
choice; the two sub-flags are errors without --dynthresh.  One launch (sdlt_guidance_dyn) in sdlt_guidance's place inside the replayed graph; the
quantile is an exact order statistic from a radix select inside the launch, so it needs no host work and repeats bit for bit.  With every sampler, noise
schedule, --guidance-interval, --init-image / --mask / --change-map, --tile-diffusion, --region and --heatmap; both passes of a hires render use it.  Not
with --guidance-rescale or --apg: they are alternative answers to the same fault.  Without the flag nothing changes.

--hires-scale F / --hires-size W H render in two passes (the "hires fix"): a picture much larger than the model was trained for falls apart when it is
sampled in one go (doubled subjects, tiled compositions), so the first pass samples at --size, the result is enlarged on the device
(sdlt_resize_planes) - the latents themselves (--hires-upscaler latent, the default; bilinear) or, through the VAE, the decoded picture (pixel;
bicubic) - noised again to --hires-strength (default 0.6) and the tail of a --hires-steps schedule (default --steps) runs at the large size: an
ordinary img2img trajectory with the same sampler, noise levels and guidance controls.  All first passes run before the UNet is rebuilt once for the
large shape.  It combines with --init-image (the first pass is then img2img), not with --mask.

--freeu B1 B2 S1 S2 turns on FreeU (Si et al. 2024; diffusers' enable_freeu order, e.g. 1.3 1.4 0.9 0.2 for SDXL, 1.5 1.6 0.9 0.2 for SD1.5): in every UNet
forward the skip features entering the first two decoder stages lose their lowest frequencies (factor S) and half of the backbone channels are amplified
(factor B) - it takes the washed-out, over-smoothed look out of a strong --guidance, and needs no weights.  --freeu-v2 scales the backbone by its own
normalised channel mean instead of a constant (the authors' current code; ComfyUI's FreeU_V2).  One more launch pair (sdlt_freeu) per affected resnet
inside the replayed graph; both passes of a hires render use it; without the flag nothing changes.

--heatmap [WORD ...] shows where the prompt's tokens look: per picture one cross-attention heat map for the checkpoint's trigger tokens (when it has any) and one
per WORD, accumulated inside the replayed graph (sdlt_heatmap_accum after every forward: the mean over steps and hooked layers of the raw scores
Q K^T / sqrt(d) of the token's context positions - what the token-attention loss of the training run sees, not softmax probabilities), finished by
sdlt_heatmap_overlay and written beside the picture as <name>_heat_<token>.jpg (all maps of a picture on one colour scale) and <name>_heat.npy (the
normalised maps, fp32 [T, gh, gw]).  A WORD of several BPE pieces is the sum of its pieces' columns; a WORD the prompt does not hold gives a warning, a zero
map and the plain picture.  A map takes at most 8 context positions (HEAT_P: the launch's shape, so that one captured graph serves every prompt): a token
that fills more - a word repeated many times - is mapped by its first 8, with a warning.  --heatmap-grid max (default) takes the finest hooked resolution, min the coarsest.  A hires render maps its second pass.

--kv-downsample F [F2 ...] is "Token Downsampling" (Smith et al. 2024) for large renders: the self-attentions keep every query but take their keys and
values from the tokens downsampled by F per axis, which cuts their score work and their to_k | to_v products by F^2 and needs no weights.  The factors
count from the largest token grid down: 2 is the largest grid only, 4 2 is 4 there and 2 on the next.  --kv-downsample-mode nearest (default, the
paper's) takes every F-th token, area the mean of each F x F window.  One more launch (sdlt_token_pool: LayerNorm and pooling fused) per affected
self-attention inside the replayed graph.  It is meant for the second pass of a hires render - where the grids are large, and after the first pass has
decided the composition - so --kv-downsample-pass defaults to hires and the flag without --hires-scale / --hires-size is an error; all uses it in
every pass.  Without the flag nothing changes.

--vae-tile [T] (diffusers' enable_vae_tiling) runs the VAE in tiles of T x T latent units (default 64: 512 px) that overlap by at least --vae-tile-overlap O
(default 16: 128 px) and are put together on the device with a normalised feather (sdlt_tile_blend; vae.VaeDecoder.decode_tiled,
vae.VaeEncoder.encode_moments_tiled): the decode of every picture, the decode and encode of --hires-upscaler pixel, and the encode of --init-image.  The
VAE's mid-block attention materialises a [pixels, pixels] score matrix - 17 GB at 2048 px, beyond the card at 4096 px - and with tiles it always runs at
the one tile shape, so the decoder is built once and a hires render rebuilds only the UNet.  GroupNorm statistics are per tile: a tiled picture differs
slightly from an untiled one.  Without the flag nothing changes.

--tile-diffusion [T] (MultiDiffusion, Bar-Tal et al. 2023; "Tiled Diffusion" of A1111 / ComfyUI) is the UNet's counterpart: in every pass whose latent
exceeds T x T latent units (default: the job's resolution // 8) the UNet runs on overlapping T x T windows - neighbours share at least
--tile-diffusion-overlap O, default T // 4 - as one batch, cut out of the model input by sdlt_window_gather and fused into one prediction for the whole
latent by sdlt_window_blend at every step; guidance and the step launch run on the whole latent as before (sampler.LatentSampler.sample(tile=)).  One
UNet shape at any picture size, attention cost linear in the picture's area, every window at the size the adapters were trained at.  A pass that fits one
window - the first pass of a hires render at the model's size - stays plain.  Not with --heatmap.  Without the flag nothing changes.

--region MASK.png|x0,y0,x1,y1 PROMPT (repeatable; "Region Prompt Control" of A1111 / ComfyUI Tiled Diffusion; MultiDiffusion section 4.2) says where
things go: "--prompt 'a stormy sky' --region 0,0.5,0.5,1 '<concept>' --region 0.5,0.5,1,1 'a red barn'".  A region is a mask picture (white: the region;
brought to the latent grid the way --mask is) or a box in fractions of the picture, with a prompt of its own - <concept> is allowed, and the prompt takes
the route the main prompt takes.  --prompt is the background: it rules wherever no region has weight.  The UNet runs the whole latent once per region
as one batch of 2 N R rows, copied by sdlt_region_gather and fused by sdlt_region_blend with per-pixel weights at every step, inside the replayed graph
(sampler.LatentSampler.sample(regions=)).  --region-feather SIGMA blurs each mask by a Gaussian of SIGMA latent pixels (sdlt_blur_planes);
--region-base F gives the main prompt the extra weight F everywhere (default 0); --region-bootstrap SHARE (default 0.2, the paper's; 0: off) is the share
of the steps at which a region sees a solid colour noised to the step's level outside its mask, so that its object forms inside.  Not with
--tile-diffusion, --heatmap or --hires-*.  Without the flag nothing changes.
"""
import argparse
import json
import math
import os

import torch
from safetensors.torch import load_file

from . import checkpoint as ckpt
from . import merge as MG
from . import ops as _ops
from . import prompts as P
from . import topology
from .config import TrainingConfig


class Loaded:
    """A checkpoint ready to render: the job's config, the train.RenderStack holding the inference models, and what was read (for inspection)."""

    def __init__(self, config, models, stack, checkpoint_dir, lora, te_lora, embeddings):
        self.config, self.models, self.stack, self.checkpoint_dir = config, models, stack, checkpoint_dir
        self.lora, self.te_lora, self.embeddings = lora, te_lora, embeddings
        self.shape = None                       # (images per batch, h, w) the UNet's buffers were allocated for; tiled diffusion: (images, th, tw, ty, tx)
        self.dec_shape = None                   # (h, w) the VAE decoder's buffers were allocated for: the latent's, or the tile's of a tiled decode

    def load_adapters(self):
        """The checkpoint's adapters into the (re)built UNet."""
        if self.lora is not None:
            self.stack.unet.arena.load(self.lora)

    def prepare(self, n_images, h, w, keep_decoder=False, plan=None, regions=1):
        """The UNet's activation buffers belong to the first latent shape it runs: another batch or size starts from fresh instances.  keep_decoder: the
        VAE decoder is not rebuilt with them (a tiled decode runs at the tile's shape whatever the picture's: prepare_decoder).  plan (a
        sampler.TilePlan): tiled diffusion - the UNet runs at the window's shape on 2 n_images ty tx rows whatever the picture's size, so the shape
        is the windows' extents and counts: another picture size with the same ones keeps the instances.  regions (R > 1): regional prompts - the UNet
        runs at the picture's shape on 2 n_images R rows."""
        shape = (n_images, h, w) if plan is None else (n_images,) + tuple(plan[2:])
        tiles = 1 if plan is None else plan.ty * plan.tx
        if regions > 1:
            shape, tiles = (n_images, h, w, "region", regions), regions
        if self.shape is not None and self.shape != shape or n_images != self.stack.n_images or tiles != getattr(self.stack, "tiles", 1):
            self.stack.keep_decoder = keep_decoder
            try:
                self.stack.build_sampler(n_images, **({} if tiles == 1 else dict(tiles=tiles)))
            finally:
                self.stack.keep_decoder = False
            if not keep_decoder:
                self.dec_shape = None
            self.load_adapters()
        self.shape = shape

    def prepare_decoder(self, h, w):
        """The decoder's buffers belong to the first latent shape it decodes, (h, w): another shape starts from a fresh decoder (the UNet stays)."""
        if self.dec_shape is not None and self.dec_shape != (h, w):
            self.stack.build_decoder()
        self.dec_shape = (h, w)


def _find(checkpoint_dir, suffix):
    return next((os.path.join(checkpoint_dir, f) for f in sorted(os.listdir(checkpoint_dir)) if f.endswith(suffix)), None)


def load_for_inference(checkpoint_dir, pretrained_model=None, device="cuda:0", runtime=None):
    """-> Loaded.  pretrained_model: None (the job's own), a UNet path / "synthetic:<version>", or the dict train() takes; runtime: a unet.Runtime
    whose device and op table the inference instances use (default: `device` with the HIP kernels)."""
    from . import train as T
    from . import unet as M
    args_path = os.path.join(checkpoint_dir, "training_args.json")
    if not os.path.exists(args_path):
        raise FileNotFoundError(f"{checkpoint_dir}: no training_args.json (not a checkpoint directory of train())")
    with open(args_path) as f:
        data = json.load(f)
    for k in ("concept_mode", "n_tokens", "is_lora", "lora_rank", "lora_alpha_multiplier", "use_dora", "pretrained_model"):
        if k not in data:
            raise KeyError(f"{args_path}: key '{k}' is missing")
    config = TrainingConfig(**dict(data, _make_dirs=False))
    config.name, config.seed = data.get("name", config.name), data.get("seed", config.seed)
    if pretrained_model is not None:
        pm = {"path": pretrained_model} if isinstance(pretrained_model, str) else dict(pretrained_model)
        config.pretrained_model = dict({k: v for k, v in (data.get("pretrained_model") or {}).items() if k == "version"}, **pm)
    config.sd_model_version = data.get("sd_model_version") or config.sd_model_version
    pm = config.pretrained_model or {}
    synthetic = str(pm.get("path", "")).startswith("synthetic:")
    # ---- what the directory must hold
    lora_file = acfg = lora_sd = None
    unet_file = os.path.join(checkpoint_dir, "diffusion_pytorch_model.safetensors")
    if config.is_lora:
        lora_file = _find(checkpoint_dir, "_lora.safetensors")
        if lora_file is None:
            raise FileNotFoundError(f"{checkpoint_dir}: no *_lora.safetensors adapter file")
        acfg_path = os.path.join(checkpoint_dir, "adapter_config.json")
        if not os.path.exists(acfg_path):
            raise FileNotFoundError(f"{checkpoint_dir}: no adapter_config.json")
        with open(acfg_path) as f:
            acfg = json.load(f)
        for k in ("r", "lora_alpha"):
            if k not in acfg:
                raise KeyError(f"{acfg_path}: key '{k}' is missing")
        lora_sd = load_file(lora_file)
    elif not os.path.exists(unet_file):
        raise FileNotFoundError(f"{checkpoint_dir}: no diffusion_pytorch_model.safetensors (the job trained the whole UNet: is_lora is false)")
    text_lora = bool(lora_sd) and any(k.startswith("lora_te") for k in lora_sd)
    if not synthetic:
        for i, key in enumerate(("text_encoder_path", "text_encoder_2_path")[: 2 if (config.sd_model_version == "sdxl") else 1]):
            if not pm.get(key):
                raise ValueError(f"pretrained_model['{key}'] is missing: rendering needs the weights of the text encoder(s)"
                                 + (" - the checkpoint holds text-encoder adapters (lora_te* keys) that are applied to them" if text_lora else ""))
    if config.is_lora:
        config.lora_rank = int(acfg["r"])
        config.lora_alpha_multiplier = float(acfg["lora_alpha"]) / float(acfg["r"])          # the kohya file's alpha is r whatever the multiplier was
        config.use_dora = bool(acfg.get("use_dora", config.use_dora))
    rt = runtime or M.Runtime(device, 1)
    models = T.Models(config, rt, build=False)
    if models.tokenizers is None:
        raise ValueError("rendering needs the tokenizer files: pretrained_model['tokenizer_path'] (vocab.json + merges.txt)")
    if models.vae_state() is None:
        raise ValueError("rendering needs the VAE weights: pretrained_model['vae_path']")
    if not config.is_lora:                      # the fine-tuned UNet is the checkpoint's own file
        models.unet_state = lambda: load_file(unet_file)
    te_rank = None
    te_lora = {}
    if text_lora:
        for i, pre in enumerate(ckpt.TEXT_PREFIXES[: len(models.kinds)]):
            te_lora.update(MG._load_text_lora(lora_sd, models.clip_state(i), pre))
        if not te_lora:
            raise KeyError(f"{lora_file}: lora_te* keys that match no module of the text encoder(s)")
        te_rank = next(iter(te_lora.values()))[0].shape[0]
        config.text_encoder_lora_rank = int(te_rank)
    stack = T.RenderStack(config, models, text_lora=text_lora, is_lora=config.is_lora)
    lora = None
    if config.is_lora:
        targets = topology.lora_targets(models.cfg)
        missing = [m for m in targets if ckpt.kohya_key(m) + ".lora_down.weight" not in lora_sd]
        if missing:
            raise KeyError(f"{lora_file}: key '{ckpt.kohya_key(missing[0])}.lora_down.weight' is missing ({len(missing)} of {len(targets)} adapted modules)")
        lora = ckpt.load_lora(lora_file, targets)
    if text_lora:
        stack.te_arena.load(te_lora)
    emb_file = _find(checkpoint_dir, "_embeddings.safetensors")
    rows = None
    if emb_file is not None:
        rows = ckpt.load_embeddings(emb_file)
        for enc, r in zip(stack.encoders, rows):
            assert r.shape[0] == config.n_tokens, (tuple(r.shape), config.n_tokens)
            enc.table[enc.V - config.n_tokens:].copy_(r.to(enc.table.device, enc.table.dtype))
    elif not config.disable_ti:
        raise FileNotFoundError(f"{checkpoint_dir}: no *_embeddings.safetensors (the job trained its trigger tokens)")
    loaded = Loaded(config, models, stack, checkpoint_dir, lora, te_lora or None, rows)
    loaded.load_adapters()
    return loaded


APG_DEFAULT = (0.0, 15.0, -0.5)      # eta, norm threshold, momentum: the SDXL settings of Sadat et al. 2024 (quoted from memory)
APG_KEYS = ("eta", "norm_threshold", "momentum")


def apg_args(apg):
    """render()'s `apg`, checked -> None | (eta, norm_threshold, momentum).  None or False: off; True: APG_DEFAULT; three numbers in that order, or a dict
    with any of the keys eta, norm_threshold, momentum (the others: APG_DEFAULT's).  The ranges are sampler.apg_table's."""
    from . import sampler as SM
    if apg is None or apg is False:
        return None
    if apg is True:
        apg = APG_DEFAULT
    elif isinstance(apg, dict):
        unknown = sorted(set(apg) - set(APG_KEYS))
        if unknown:
            raise ValueError(f"apg: keys {', '.join(APG_KEYS)}; unknown {unknown}")
        apg = tuple(apg.get(k, d) for k, d in zip(APG_KEYS, APG_DEFAULT))
    if not (isinstance(apg, (tuple, list)) and len(apg) == 3 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in apg)):
        raise ValueError(f"apg takes True, (eta, norm_threshold, momentum) or a dict of them, got {apg!r}")
    apg = tuple(float(v) for v in apg)
    SM.apg_table(None, apg, 1)                          # (the ranges)
    return apg


DYN_DEFAULT = (7.0, 0.999, 1.0)      # mimic scale, percentile, interpolate: this project's choice
DYN_KEYS = ("mimic", "percentile", "interpolate")


def dynthresh_args(dynthresh):
    """render()'s `dynthresh`, checked -> None | (mimic, percentile, interpolate).  None or False: off; True: DYN_DEFAULT; three numbers in that order, or a
    dict with any of the keys mimic, percentile, interpolate (the others: DYN_DEFAULT's).  The ranges are sampler.dyn_table's."""
    from . import sampler as SM
    dt = dynthresh
    if dt is None or dt is False:
        return None
    if dt is True:
        dt = DYN_DEFAULT
    elif isinstance(dt, dict):
        unknown = sorted(set(dt) - set(DYN_KEYS))
        if unknown:
            raise ValueError(f"dynthresh: keys {', '.join(DYN_KEYS)}; unknown {unknown}")
        dt = tuple(dt.get(k, d) for k, d in zip(DYN_KEYS, DYN_DEFAULT))
    if not (isinstance(dt, (tuple, list)) and len(dt) == 3 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in dt)):
        raise ValueError(f"dynthresh takes True, (mimic, percentile, interpolate) or a dict of them, got {dynthresh!r}")
    dt = tuple(float(v) for v in dt)
    SM.dyn_table(None, dt, 1)                           # (the ranges)
    return dt


def _scale_tag(s):
    return f"{s:.2f}"


def _open(image):
    from PIL import Image
    return Image.open(image) if isinstance(image, (str, os.PathLike)) else image


def _vae_encoder(loaded):
    """A VAE encoder on the loaded stack's device and op table; its buffers belong to the first image size it encodes."""
    from . import unet as M
    from . import vae as V
    rt = loaded.stack.rt
    return V.VaeEncoder(M.Runtime(rt.device, 1, act_dtype=rt.act, ops=rt.ops), loaded.models.vae_state())


VAE_TILE, VAE_TILE_OVERLAP = 64, 16      # --vae-tile's defaults, in latent units (512 and 128 px with the SD / SDXL VAE)


def vae_tile_args(vae_tile):
    """render()'s `vae_tile`, checked -> None | (tile, overlap) in latent units.  None: off; an int: that tile with the default overlap; (tile, overlap).
    ValueError unless tile >= 2 and 0 <= 2 overlap <= tile (vae.tile_starts)."""
    from . import vae as V
    if vae_tile is None:
        return None
    if isinstance(vae_tile, bool) or not (isinstance(vae_tile, int) or (isinstance(vae_tile, (tuple, list)) and len(vae_tile) == 2
                                                                        and all(isinstance(v, int) and not isinstance(v, bool) for v in vae_tile))):
        raise ValueError(f"vae_tile must be None, a tile length or (tile, overlap) in latent units, got {vae_tile!r}")
    tile, overlap = (vae_tile, VAE_TILE_OVERLAP) if isinstance(vae_tile, int) else vae_tile
    V.tile_starts(tile, tile, overlap)
    return int(tile), int(overlap)


TILE_DIFFUSION_JOB = object()      # --tile-diffusion without a value: no number a user can type


def tile_diffusion_default(config):
    """--tile-diffusion without a value: the job's training resolution in latent units (the size its adapters were trained at)."""
    return int(config.resolution) // 8


@torch.no_grad()
def encode_image(loaded, img, enc=None, vae_tile=None):
    """img [1, 3, H, W] fp32 in about [-1, 1] -> init latents [1, 4, H/f, W/f] fp32: the posterior's mean times the scaling factor (deterministic).
    vae_tile (tile, overlap): through VaeEncoder.encode_moments_tiled."""
    enc = enc or _vae_encoder(loaded)
    mom = enc.encode_moments(img) if vae_tile is None else enc.encode_moments_tiled(img, *vae_tile)
    x0 = mom[:, : mom.shape[1] // 2].float() * loaded.models.cfg["scaling_factor"]
    return x0.contiguous()


@torch.no_grad()
def encode_init(loaded, init_image, mask_image, size, latent_hw, vae_tile=None):
    """-> (init latents [1, 4, h, w] fp32 = posterior mean of the image, resized to `size` = (width, height), times the scaling factor;
    mask [1, 1, h, w] fp32 | None: dataset.latent_mask's resize, 1 regenerate / 0 keep).  Images are paths or PIL images.  vae_tile: encode_image's."""
    from . import dataset as D
    enc = _vae_encoder(loaded)
    f = 2 ** (len(enc.downs) - 1)
    h, w = latent_hw
    if (size[0], size[1]) != (f * w, f * h):
        raise ValueError(f"an init image needs a size that is a multiple of {f}, got {size[0]} x {size[1]}")
    x0 = encode_image(loaded, D.prepare_image(_open(init_image).convert("RGB"), size[0], size[1]), enc, vae_tile)
    mask = None
    if mask_image is not None:
        mask = D.latent_mask(_open(mask_image), size, (h, w), channels=1).reshape(1, 1, h, w).to(loaded.stack.rt.device)
    return x0, mask


HEAT_P = 8          # context positions per map (a launch shape: one capture serves every prompt)


def heat_positions(tokenizers, prompt, words, trigger_tokens, P=HEAT_P, warn=None):
    """The context positions behind each heat map of `prompt` (the text as it is encoded, learned tokens in place) -> (names, cols): names of the T maps -
    "trigger" first when trigger_tokens is not empty, then the words - and cols [T][P] int, -1 padded.  The prompt's row is [bos, ids ..., eos, pad ...]
    cut to 77 as the encoder reads it: id j sits at position 1 + j, and only the first 75 ids survive.  A map collects the positions of every id of
    trigger_tokens, or of every occurrence of the word's BPE pieces as a run; an absent word: all -1 and a warning.  Every tokenizer of the model
    (SDXL has two on one vocabulary) must give the same positions."""
    import warnings
    warn = warn or (lambda m: warnings.warn(m, stacklevel=3))
    per_tok = []
    for tk in tokenizers:
        ids = tk.tokenize_ids(prompt)[: tk.max_length - 2]
        rows = []
        if trigger_tokens:
            trig = set(tk.convert_tokens_to_ids(list(trigger_tokens)))
            rows.append([1 + j for j, v in enumerate(ids) if v in trig])
        for wd in words:
            run = tk.tokenize_ids(wd)
            rows.append([1 + j + q for j in range(len(ids) - len(run) + 1) if run and ids[j: j + len(run)] == run for q in range(len(run))])
        per_tok.append(rows)
    if any(r != per_tok[0] for r in per_tok[1:]):
        raise ValueError(f"heatmap: the model's tokenizers place the tokens of {prompt!r} at different positions: {per_tok}")
    names = (["trigger"] if trigger_tokens else []) + [str(wd) for wd in words]
    cols = []
    for name, pos in zip(names, per_tok[0]):
        pos = sorted(set(pos))
        if not pos:
            warn(f"heatmap: {name!r} is not in the prompt {prompt!r} (or lies past its 77-token cut): its map is empty")
        if len(pos) > P:
            warn(f"heatmap: {name!r} occupies {len(pos)} positions of {prompt!r}; the first {P} are mapped")
        cols.append((pos + [-1] * P)[:P])
    return names, cols


def _heat_tag(name):
    return "".join(ch if ch.isalnum() or ch in "-_" else "_" for ch in name) or "_"


HIRES_KEYS = ("scale", "size", "strength", "steps", "upscaler", "resample")
HIRES_UPSCALERS = ("latent", "pixel")
KV_PASSES = ("hires", "all")      # which passes of a render carry kv_downsample


def hires_args(hires, size, steps, f=8):
    """render()'s `hires` dict, checked and completed -> dict(size (W2, H2), base_size, strength, steps, upscaler, resample).  Keys: scale | size
    (exactly one: sampler.hires_plan), strength (default 0.6: the share of the second schedule that runs), steps (default: the first pass's),
    upscaler "latent" | "pixel", resample "nearest" | "bilinear" | "bicubic" (default: bilinear for latent, bicubic for pixel)."""
    from . import sampler as SM
    unknown = sorted(set(hires) - set(HIRES_KEYS))
    if unknown:
        raise ValueError(f"hires: unknown key(s) {unknown}; known: {HIRES_KEYS}")
    target = SM.hires_plan(size, hires.get("scale"), hires.get("size"), f)
    strength = hires.get("strength")
    strength = 0.6 if strength is None else strength
    if not (isinstance(strength, (int, float)) and 0.0 < strength <= 1.0):
        raise ValueError(f"hires strength must be in (0, 1], got {strength!r}")
    steps2 = hires.get("steps") or steps
    SM.img2img_steps(steps2, strength)
    upscaler = hires.get("upscaler") or "latent"
    if upscaler not in HIRES_UPSCALERS:
        raise ValueError(f"hires upscaler must be one of {HIRES_UPSCALERS}, got {upscaler!r}")
    resample = hires.get("resample") or ("bilinear" if upscaler == "latent" else "bicubic")
    if resample not in SM.RESAMPLE:
        raise ValueError(f"hires resample must be one of {SM.RESAMPLE}, got {resample!r}")
    return dict(size=target, base_size=(int(size[0]), int(size[1])), strength=strength, steps=int(steps2), upscaler=upscaler, resample=resample)


REGION_BOOTSTRAP = 0.2      # --region-bootstrap's default: the share of the steps that bootstrap (MultiDiffusion section 4.2)
REGION_BG_SIZE = 8          # latent units of the solid-colour picture whose encoding is a region's bootstrap background


def region_spec(text):
    """--region's first value -> a box (x0, y0, x1, y1) where it reads as four comma-separated numbers, else the text: a mask picture's path."""
    parts = text.split(",")
    if len(parts) == 4:
        try:
            return tuple(float(v) for v in parts)
        except ValueError:
            pass
    return text


def region_args(regions, region_feather=None, region_base=None, region_bootstrap=None):
    """render()'s `regions`, `region_feather`, `region_base` and `region_bootstrap`, checked -> None | dict(regions [(mask image | box, prompt)], feather,
    base, bootstrap).  regions: None, or a non-empty list of (mask image - a path or PIL image - | box (x0, y0, x1, y1) in fractions of the picture with
    0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1, prompt); at most 7 (sampler.region_plan: 8 with the background).  feather: a Gaussian sigma in latent
    pixels >= 0 (default 0); base >= 0 (default 0); bootstrap: a share of the steps in [0, 1] (default REGION_BOOTSTRAP).  ValueError otherwise, and
    for any of the three without regions."""
    from . import sampler as SM
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)  # noqa: E731
    if regions is None:
        if region_feather is not None or region_base is not None or region_bootstrap is not None:
            raise ValueError("region_feather, region_base and region_bootstrap need regions")
        return None
    regions = list(regions)
    if not regions or len(regions) + 1 > SM.REGION_PLAN_MAX:
        raise ValueError(f"regions: {len(regions)} region(s); 1 .. {SM.REGION_PLAN_MAX - 1} beside the main prompt's")
    out = []
    for item in regions:
        if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[1], str) and item[1].strip()):
            raise ValueError(f"regions: each entry is (mask image | box, prompt), got {item!r}")
        where, prompt = item
        if isinstance(where, (tuple, list)):
            if not (len(where) == 4 and all(num(v) for v in where) and 0.0 <= where[0] < where[2] <= 1.0 and 0.0 <= where[1] < where[3] <= 1.0):
                raise ValueError(f"regions: a box is (x0, y0, x1, y1) in fractions of the picture with 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1, got {where!r}")
            where = tuple(float(v) for v in where)
        out.append((where, prompt))
    feather = 0.0 if region_feather is None else region_feather
    if not (num(feather) and feather >= 0.0):
        raise ValueError(f"region_feather must be a finite number >= 0 (latent pixels), got {region_feather!r}")
    base = 0.0 if region_base is None else region_base
    if not (num(base) and base >= 0.0):
        raise ValueError(f"region_base must be a finite number >= 0, got {region_base!r}")
    boot = REGION_BOOTSTRAP if region_bootstrap is None else region_bootstrap
    if not (num(boot) and 0.0 <= boot <= 1.0):
        raise ValueError(f"region_bootstrap must be a share of the steps in [0, 1], got {region_bootstrap!r}")
    return dict(regions=out, feather=float(feather), base=float(base), bootstrap=float(boot))


def region_masks(loaded, rg, size, latent_hw):
    """The foreground masks of region_args' dict on the latent grid -> fp32 [R - 1, h, w] in [0, 1] on the device: a mask picture by dataset.latent_mask
    (the way --mask is resized), a box filled between round(x0 w) and round(x1 w) (at least one latent pixel), then each blurred by `feather`
    (sampler.blur_map)."""
    from . import dataset as D
    from . import sampler as SM
    h, w = latent_hw
    planes = []
    for where, _ in rg["regions"]:
        if isinstance(where, tuple):
            m = torch.zeros(h, w)
            x0, y0 = min(int(round(where[0] * w)), w - 1), min(int(round(where[1] * h)), h - 1)
            m[y0:max(int(round(where[3] * h)), y0 + 1), x0:max(int(round(where[2] * w)), x0 + 1)] = 1.0
        else:
            m = D.latent_mask(_open(where), size, (h, w), channels=1).reshape(h, w).float()
        planes.append(m)
    masks = torch.stack(planes)[:, None].to(loaded.stack.rt.device)
    return SM.blur_map(loaded.stack.rt.ops, masks, rg["feather"]).reshape(len(planes), h, w).contiguous()


@torch.no_grad()
def region_backgrounds(loaded, R, seed):
    """The bootstrap backgrounds -> fp32 [R, 4] on the device: per region one solid colour drawn from `seed`, encoded once by the VAE encoder at a small
    size (REGION_BG_SIZE latent units), its latent mean over the picture times the scaling factor."""
    enc = _vae_encoder(loaded)
    f = 2 ** (len(enc.downs) - 1)
    colours = torch.rand(R, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0
    dev = loaded.stack.rt.device
    out = []
    for r in range(R):
        img = colours[r].view(1, 3, 1, 1).expand(1, 3, f * REGION_BG_SIZE, f * REGION_BG_SIZE).contiguous().to(dev)
        out.append(encode_image(loaded, img, enc).float().mean(dim=(0, 2, 3)))
    return torch.stack(out)


@torch.no_grad()
def render(loaded, prompts, out_dir, *, lora_scales=None, size=None, steps=25, guidance_scale=8.0, seed=None, images_per_batch=1, token_scale=None,
           graph=True, n_validation=4, init_image=None, strength=None, mask_image=None, sampler="euler", sigmas="trailing", eta=None,
           guidance_rescale=0.0, guidance_interval=None, negative_prompt=None, hires=None, freeu=None, heatmap=None, heatmap_grid="max",
           kv_downsample=None, kv_downsample_mode="nearest", kv_downsample_pass="hires", vae_tile=None, change_map_image=None, mask_blur=None, tile_diffusion=None, regions=None, region_feather=None,
           region_base=None, region_bootstrap=None, apg=None, dynthresh=None):
    """Per adapter scale and prompt: conditioning (prompts.prompt_pair + sampler.blend_conditions, as the training-time renderer) -> latents ->
    VAE decode -> `img_{prompt index:02d}_seed{seed}_scale{scale}.jpg`, plus `grid_scale{scale}.jpg` per scale.  Image i starts from the noise of
    seed + i at every scale.  size = (width, height) in pixels; prompts=None: n_validation validation prompts of the job's concept mode.
    graph=False is the eager loop with the same fused kernel.  init_image (path or PIL image): every image starts from it (encode_init) at
    `strength` (default 0.6) instead of from pure noise, each with its own noise; mask_image: white regenerate, black keep.  sampler "euler" |
    "dpmpp_2m" | "euler_a" | "dpmpp_2m_sde", sigmas "trailing" | "karras", eta (stochastic samplers only; default 1): LatentSampler.sample's; the
    per-step noise of image i is keyed by seed + i, like its initial latents.  guidance_rescale in [0, 1], guidance_interval (sigma_lo, sigma_hi):
    LatentSampler.sample's; negative_prompt: the negative row's text (None: prompts.NEGATIVE_PROMPT).
    apg: None, True (APG_DEFAULT), (eta, norm_threshold, momentum) or a dict of them (apg_args): adaptive projected guidance - LatentSampler.sample's
    `apg` - in every pass, of a hires render too (each pass is a trajectory of its own: the running average restarts); with everything else.
    dynthresh: None, True (DYN_DEFAULT), (mimic, percentile, interpolate) or a dict of them (dynthresh_args): dynamic thresholding - LatentSampler.sample's
    `dynthresh` - in every pass, of a hires render too; not with apg or guidance_rescale > 0 (ValueError).
    hires (a dict, hires_args: scale | size, strength, steps, upscaler, resample): two passes - every image is first sampled at `size`, for all adapter
    scales and prompt batches, its latents staying on the device; they are enlarged (sampler.upscale_latents: the latents, or with upscaler "pixel"
    the decoded picture, encoded again); then the UNet is rebuilt ONCE for the large shape and every second pass runs: sample(init_latents=the
    enlarged latents, strength, steps) with the same sampler, sigmas, eta and guidance controls.  Image i's generator (seed + i) gives the first
    pass's noise with its first draw and the second pass's with its second; the stochastic samplers key the second pass's per-step noise by
    seed + i + 2^32.  SDXL's size conditioning is the base size in the first pass and the final size in the second.
    freeu: (b1, b2, s1, s2) or dict(b1, b2, s1, s2, version=1) - LatentSampler.sample's (sampler.freeu_args): FreeU in every forward, of both passes of a
    hires render too (the setting travels with each sample() call, so the rebuilt UNet has it).
    heatmap: None, or a list of words (may be empty): per picture one cross-attention heat map for the trigger tokens (unless the job trained none) and one
    per word (heat_positions, on the prompt with the learned tokens), accumulated by LatentSampler.sample(heatmap=) on grid heatmap_grid ("max" | "min") -
    in a hires render by the second pass - and written by ops.heatmap_overlay as `<picture>_heat_<token>.jpg` and `<picture>_heat.npy`.
    kv_downsample: integer factors, largest self-attention token grid first - (2,), (4, 2) - with kv_downsample_mode "nearest" | "area":
    LatentSampler.sample's key / value token downsampling (sampler.kv_downsample_args; UNet.set_kv_downsample).  kv_downsample_pass "hires" (default):
    only the second pass of a hires render carries it - that is where the self-attentions are large, and the first pass decides the composition -
    so without `hires` it is refused; "all": every pass.
    vae_tile: None, a tile length or (tile, overlap) in latent units (vae_tile_args; the overlap defaults to 16): every VAE pass of the render - the
    decode of each picture, the decode and encode of the pixel upscaler, the encode of init_image - runs in tiles (VaeDecoder.decode_tiled,
    VaeEncoder.encode_moments_tiled; ops.tile_blend).  The decoder then runs at the tile's shape and is not rebuilt with the UNet by the hires pass.
    change_map_image (path or PIL image; needs init_image, excludes mask_image and hires): differential diffusion - its luminance, area-resized to the
    latent grid (dataset.latent_change_map), is LatentSampler.sample's change_map: white the whole `strength`, black keep.  mask_blur (a sigma in latent
    pixels, >= 0): the change map - or mask_image's mask, which then takes the blend path as before - is blurred on the device first (sampler.blur_map).
    tile_diffusion: None, a window length T or (T, overlap) in latent units (sampler.tile_plan; the overlap defaults to T // 4): tiled diffusion -
    LatentSampler.sample's `tile` - in every pass whose latent exceeds T on an axis: the UNet then runs at the window's shape on 2 images_per_batch ty tx
    rows.  A pass that fits one window - the first pass of a hires render at the model's size - stays plain.  Not with heatmap.
    regions: None, or [(mask image | box (x0, y0, x1, y1) in fractions of the picture, prompt), ...] (region_args): regional prompts -
    LatentSampler.sample's `regions`.  Every prompt of `prompts` is the background of its picture; each region's prompt is encoded by the route the main
    prompt takes (trigger substitution, blend_conditions) and rules where its mask has weight: the UNet then runs on 2 images_per_batch R rows.
    region_feather: a Gaussian sigma in latent pixels that blurs each mask first; region_base: the main prompt's extra weight everywhere;
    region_bootstrap: the share of the steps that run at which a region sees a solid colour (region_backgrounds, from `seed`) noised to the step's
    level outside its mask (default 0.2; 0: off).  Not with tile_diffusion, heatmap or hires.
    -> {scale: [paths]}."""
    from . import train as T
    from . import vae as _vae
    from PIL import Image
    config, stack = loaded.config, loaded.stack
    cfg = loaded.models.cfg
    dev = stack.rt.device
    if prompts is None:
        lists = (config.training_attributes or {}).get("validation_prompts")
        prompts = P.validation_prompts(config.concept_mode, n_validation, config.seed, config.prompt_modifier, lists if isinstance(lists, dict) else None)
    prompts = list(prompts)
    if lora_scales is None:
        lora_scales = [config.sample_imgs_lora_scale or (0.75 if cfg["addition"] else 0.85)]
    if size is None:
        size = config.validation_img_size or (1024 if cfg["addition"] else 768)
    size = (size, size) if isinstance(size, int) else tuple(size)
    seed = config.seed if seed is None else seed
    f = 2 ** (len(stack.decoder.ups) - 1) if hasattr(stack.decoder, "ups") else 8      # 8 for the SD / SDXL VAE
    w, h = size[0] // f, size[1] // f
    n = images_per_batch
    from . import sampler as SM
    sde, eta_given = sampler in SM.SDE_KINDS, eta is not None
    eta = SM.sampler_args(sampler, sigmas, eta)                        # (None: 1)
    if eta_given and not sde:
        raise ValueError(f"eta scales the per-step noise of {SM.SDE_KINDS}; sampler {sampler!r} adds none")
    if not 0.0 <= guidance_rescale <= 1.0:
        raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
    if guidance_interval is not None:
        guidance_interval = tuple(float(v) for v in guidance_interval)
        if len(guidance_interval) != 2 or not guidance_interval[0] < guidance_interval[1]:
            raise ValueError(f"guidance_interval must be (sigma_lo, sigma_hi) with sigma_lo < sigma_hi, got {guidance_interval!r}")
    ag = apg_args(apg)                                                 # (raises before anything is built)
    dt = dynthresh_args(dynthresh)
    if dt is not None and (ag is not None or guidance_rescale):
        raise ValueError("dynthresh does not combine with " + ("apg" if ag is not None else "guidance_rescale") + ": they are alternative answers to the burnt "
                         "contrast of a strong guidance scale")
    if ag is not None:
        SM.require_op(stack.rt.ops, "guidance_apg", " (sdlt_guidance_apg): apg forms the projected prediction by that launch (ops.guidance_apg)", kernel="sdlt_guidance_apg")
    if dt is not None:
        SM.require_op(stack.rt.ops, "guidance_dyn", " (sdlt_guidance_dyn): dynthresh forms the thresholded prediction by that launch (ops.guidance_dyn)", kernel="sdlt_guidance_dyn")
    rg = region_args(regions, region_feather, region_base, region_bootstrap)      # (raises before anything is built)
    if rg is not None:
        for other, name in ((tile_diffusion, "tile_diffusion: windows of regions are not built"), (hires, "hires: the masks would need a second grid"),
                            (heatmap, "heatmap: the hooked score sums are per region row, and fusing them is not built")):
            if other is not None:
                raise ValueError(f"regions do not combine with {name}")
        SM.require_op(stack.rt.ops, "region_blend", " (sdlt_region_blend): regions copy the model input and fuse the predictions by two launches (ops.region_gather, ops.region_blend)")
        if rg["feather"] > 0.0:
            SM.require_op(stack.rt.ops, "blur_planes", ": region_feather blurs the masks on the device by that launch (ops.blur_planes)")
    fz = SM.freeu_args(freeu)                                          # (raises before anything is built)
    hm_names = hm_cols = None
    if heatmap is not None:
        words = [heatmap] if isinstance(heatmap, str) else list(heatmap)
        if heatmap_grid not in SM.HEAT_GRIDS:
            raise ValueError(f"heatmap_grid must be one of {SM.HEAT_GRIDS}, got {heatmap_grid!r}")
        triggers = [] if config.disable_ti else list(config.inserting_list_tokens or [])
        if not triggers and not words:
            raise ValueError("heatmap: this checkpoint has no trigger tokens (the job did not train any), so there is nothing to map without a word: "
                             "name the prompt's words to look at (--heatmap WORD ...)")
        for op in ("heatmap_accum", "heatmap_overlay"):
            SM.require_op(stack.rt.ops, op, f": the heat maps are made by that launch (ops.{op})")
        hm_cols = []
        for p_ in prompts:                                             # positions in the prompt as it is encoded, learned tokens in place
            lora_p = P.prompt_pair(p_, config.token_dict, (config.training_attributes or {}).get("trigger_text", "TOK"), config.name, config.concept_mode,
                                   use_lora=not config.disable_ti)[0]
            hm_names, c_ = heat_positions(loaded.models.tokenizers, lora_p, words, triggers)
            hm_cols.append(c_)
        hm_cols = torch.tensor(hm_cols, dtype=torch.int32)            # [prompts, T, P]
    kd = SM.kv_downsample_args(kv_downsample, kv_downsample_mode)    # (raises before anything is built)
    if kv_downsample_pass not in KV_PASSES:
        raise ValueError(f"kv_downsample_pass must be one of {KV_PASSES}, got {kv_downsample_pass!r}")
    if kd is not None:
        if kv_downsample_pass == "hires" and hires is None:
            raise ValueError("kv_downsample applies to the second pass of a hires render by default and this render has none: pass "
                             "kv_downsample_pass='all' (--kv-downsample-pass all) to use it in a single-pass render")
        SM.require_op(stack.rt.ops, "token_pool", " (sdlt_token_pool): kv_downsample pools the keys' tokens by that launch (ops.token_pool)")
    kd_kw = {} if kd is None else dict(kv_downsample=kd[0], kv_downsample_mode=kd[1])
    vt = vae_tile_args(vae_tile)                                     # (raises before anything is built)
    if vt is not None:
        SM.require_op(stack.rt.ops, "tile_blend", " (sdlt_tile_blend): vae_tile puts the VAE's tiles together by that launch (ops.tile_blend)")
    td_plan = SM.tile_plan(h, w, tile_diffusion)                     # (raises before anything is built)
    td_plan2 = None
    if tile_diffusion is not None:
        if heatmap is not None:
            raise ValueError("heatmap does not combine with tile_diffusion: the hooked score sums are per window, and stitching them is not built")
        SM.require_op(stack.rt.ops, "window_blend", " (sdlt_window_blend): tile_diffusion cuts and fuses the windows by two launches (ops.window_gather, ops.window_blend)")
    if init_image is None and (change_map_image is not None or mask_blur is not None):
        raise ValueError("change_map_image and mask_blur need init_image: the pixels to keep are taken from it")
    if change_map_image is not None and mask_image is not None:
        raise ValueError("change_map_image and mask_image exclude each other: the map selects per pixel and step, the mask blends after every step")
    if change_map_image is not None and hires is not None:
        raise ValueError("hires does not combine with change_map_image: the second pass would need the original at the large size")
    if mask_blur is not None:
        if mask_image is None and change_map_image is None:
            raise ValueError("mask_blur blurs mask_image's mask or change_map_image's map: give one of them")
        if not (isinstance(mask_blur, (int, float)) and not isinstance(mask_blur, bool) and math.isfinite(mask_blur) and mask_blur >= 0.0):
            raise ValueError(f"mask_blur must be a finite number >= 0 (latent pixels), got {mask_blur!r}")
        if mask_blur > 0.0:
            SM.require_op(stack.rt.ops, "blur_planes", ": mask_blur blurs the map on the device by that launch (ops.blur_planes)")
    hi = None
    if hires is not None:
        if mask_image is not None:
            raise ValueError("hires does not combine with mask_image: the mask would need a resize of its own")
        hi = hires_args(hires, size, steps, f)                         # (raises before anything is built)
        td_plan2 = SM.tile_plan(hi["size"][1] // f, hi["size"][0] // f, tile_diffusion)
    for pl in (td_plan, td_plan2):
        SM.window_multiple(cfg, pl, "tile_diffusion")
    img_kw = {}
    if guidance_rescale != 0.0:
        img_kw.update(guidance_rescale=guidance_rescale)
    if guidance_interval is not None:
        img_kw.update(guidance_interval=guidance_interval)
    if ag is not None:
        img_kw.update(apg=ag)
    if dt is not None:
        img_kw.update(dynthresh=dt)
    if (sampler, sigmas) != ("euler", "trailing"):
        img_kw.update(sampler=sampler, sigmas=sigmas)
    if sde:
        img_kw.update(eta=eta)
    if fz is not None:
        img_kw.update(freeu=fz)
    if kv_downsample_pass == "all":
        img_kw.update(kd_kw)
    if init_image is None:
        if mask_image is not None:
            raise ValueError("mask_image needs init_image: the region to keep is taken from it")
        if strength is not None:
            raise ValueError("strength needs init_image")
    else:
        strength = 0.6 if strength is None else strength
        SM.img2img_steps(steps, strength)               # (raises before anything is built)
        x0, mask = encode_init(loaded, init_image, mask_image, size, (h, w), **({} if vt is None else dict(vae_tile=vt)))
        if mask is not None and mask_blur:
            mask = SM.blur_map(stack.rt.ops, mask, mask_blur)
        img_kw.update(init_latents=x0, strength=strength, mask=mask)
        if change_map_image is not None:
            from . import dataset as D
            cmap = D.latent_change_map(_open(change_map_image), size, (h, w)).to(dev)
            img_kw.update(change_map=SM.blur_map(stack.rt.ops, cmap, mask_blur or 0.0))
    td_kw = lambda pl: {} if pl is None else dict(plan=pl)  # noqa: E731
    tile_kw = lambda pl: {} if pl is None else dict(tile=(pl.T, pl.O))  # noqa: E731
    R_ = 1 if rg is None else len(rg["regions"]) + 1
    reg_kw = None
    if rg is not None:                                  # masks, backgrounds and the bootstrap's step count: the same for every picture of the render
        k_run = steps if init_image is None else SM.img2img_steps(steps, strength)[0]
        k_boot = int(round(rg["bootstrap"] * k_run))
        reg_kw = dict(masks=region_masks(loaded, rg, size, (h, w)), base=rg["base"], bootstrap=k_boot,
                      bg=None if k_boot == 0 else region_backgrounds(loaded, R_, seed)[None].expand(n, R_, 4).contiguous())
    loaded.prepare(n, h, w, **({} if vt is None else dict(keep_decoder=True)), **td_kw(td_plan), **({} if rg is None else dict(regions=R_)))
    fused = hasattr(stack.rt.ops, "sampler_step_dd" if change_map_image is not None else "sampler_step_sde" if sde else "sampler_step_ms" if sampler == "dpmpp_2m"
                    else "sampler_step")
    graph = graph and dev.type == "cuda"
    os.makedirs(out_dir, exist_ok=True)
    result = {}

    def sample(embeds, idx, lh, lw, px, noise, kw, seed0, steps=steps, heat=False):
        """One batch: latents [n, 4, lh, lw].  px = (width, height) of the size conditioning; seed0 + i keys image i's per-step noise.  heat: with the
        batch's heat maps -> (latents, maps [n, T, gh, gw])."""
        smp = stack.sampler
        # regional prompts: the same region conditioning for every image of the batch (m images: one list per image; one image: the list itself)
        rk = lambda m: {} if reg_kw is None else dict(regions=dict(reg_kw, embeds=[reg_embeds] * m if m > 1 else reg_embeds, bg=None if reg_kw["bg"] is None else reg_kw["bg"][:m]))  # noqa: E731
        sd = (lambda js: dict(seeds=[seed0 + idx[j] for j in js])) if sde or reg_kw is not None else (lambda js: {})      # (regions: the bootstrap's key)
        hm = (lambda js: dict(heatmap=dict(cols=hm_cols[[idx[j] for j in js]], grid=heatmap_grid))) if heat else (lambda js: {})
        if fused:
            return smp.sample([embeds[i] for i in idx] if n > 1 else embeds[idx[0]], lh, lw, steps=steps, guidance_scale=guidance_scale,
                              size=(px[1], px[0]), latents=noise, graph=graph, fused=True, n_images=n, **kw, **sd(range(n)), **hm(range(n)), **rk(n))
        # an op table without the fused kernel: the torch loop, image by image
        one = lambda v, j: v[j:j + 1] if torch.is_tensor(v) and v.shape[0] == n and n > 1 else v  # noqa: E731
        outs = [smp.sample(embeds[i], lh, lw, steps=steps, guidance_scale=guidance_scale, size=(px[1], px[0]), latents=noise[j:j + 1],
                           **{k: one(v, j) for k, v in kw.items()}, **sd([j]), **hm([j]), **rk(1)) for j, i in enumerate(idx)]
        return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])) if heat else torch.cat(outs)

    def decode(z):
        """One image's latents [1, 4, lh, lw] -> picture [1, 3, f lh, f lw]; the decoder's buffers follow the shape it runs at (the tile's with vae_tile)."""
        lh, lw = z.shape[2:]
        if vt is None:
            loaded.prepare_decoder(lh, lw)
            return stack.decoder.decode(z)
        loaded.prepare_decoder(min(lh, vt[0]), min(lw, vt[0]))
        return stack.decoder.decode_tiled(z, *vt)

    def save(lat, idx, s0, scale, paths):
        lat, heat = lat if isinstance(lat, tuple) else (lat, None)
        for j, i in enumerate(idx[: len(prompts) - s0]):
            chw = _vae.postprocess(decode(lat[j:j + 1] / cfg["scaling_factor"]))
            img = chw[0].permute(1, 2, 0)
            arr = (img.float().cpu().numpy() * 255).round().astype("uint8")
            paths.append(os.path.join(out_dir, f"img_{i:02d}_seed{seed + i}_scale{_scale_tag(scale)}.jpg"))
            Image.fromarray(arr).save(paths[-1], format="JPEG", quality=95)
            if heat is not None:                # all maps of the picture on one scale; the overlays and the normalised maps beside the picture
                import numpy as np
                ops = stack.rt.ops
                lut = getattr(ops, "heatmap_colour_table", _ops.heatmap_colour_table)().to(dev)
                norm, over = ops.heatmap_overlay(heat[j:j + 1].contiguous(), hm_cols[i:i + 1].to(dev), chw[:1].float().contiguous(), lut)
                stem = paths[-1][: -len(".jpg")]
                np.save(stem + "_heat.npy", norm[0].cpu().numpy())
                for t, name in enumerate(hm_names):
                    Image.fromarray(over[0, t].cpu().numpy()).save(f"{stem}_heat_{_heat_tag(name)}.jpg", format="JPEG", quality=95)

    def finish(scale, paths):
        T.make_validation_img_grid(paths, os.path.join(out_dir, f"grid_scale{_scale_tag(scale)}.jpg"))
        result[scale] = paths

    def enlarge(lat, enc):
        """The first pass's latents [n, 4, h, w] -> the second pass's init latents [n, 4, h2, w2]."""
        ops = stack.rt.ops
        if hi["upscaler"] == "latent":
            return SM.upscale_latents(ops, lat, h2, w2, hi["resample"])
        out = []
        for j in range(n):                      # through the VAE: the decoder's output as it is (not clamped), enlarged, the encoder's posterior mean
            img = decode(lat[j:j + 1] / cfg["scaling_factor"])
            out.append(encode_image(loaded, SM.upscale_latents(ops, img, f * h2, f * w2, hi["resample"]), enc, **({} if vt is None else dict(vae_tile=vt))))
        return torch.cat(out)

    if hi is not None:
        w2, h2 = hi["size"][0] // f, hi["size"][1] // f
        if not hasattr(stack.rt.ops, "resize_planes"):
            SM.upscale_latents(stack.rt.ops, None, h2, w2, hi["resample"])      # (raises: no kernel, no fallback)
        kw2 = dict({k: v for k, v in img_kw.items() if k not in ("init_latents", "strength", "mask")}, **kd_kw)      # (kv_downsample: the second pass has it either way)
        enc = _vae_encoder(loaded) if hi["upscaler"] == "pixel" else None
        second = []                             # (index of the scale, embeds, first prompt of the batch, idx, enlarged latents, second noise)
    try:
        for k, scale in enumerate(lora_scales):
            stack.sampler.set_lora_scale(scale)
            embeds = [stack.conditioning(p, scale, token_scale, negative_prompt)[0] for p in prompts]
            reg_embeds = [] if rg is None else [stack.conditioning(p, scale, token_scale, negative_prompt)[0] for _, p in rg["regions"]]
            paths = []
            for s0 in range(0, len(prompts), n):
                idx = [min(s0 + j, len(prompts) - 1) for j in range(n)]          # a short last batch repeats its last prompt
                gens = [torch.Generator(device=dev).manual_seed(seed + i) for i in idx]
                noise = torch.cat([torch.randn(1, 4, h, w, generator=g, device=dev) for g in gens])
                lat = sample(embeds, idx, h, w, size, noise, dict(img_kw, **tile_kw(td_plan)), seed, heat=hm_cols is not None and hi is None)
                if hi is None:
                    save(lat, idx, s0, scale, paths)
                else:                                                            # each generator's second draw: the second pass's noise
                    noise2 = torch.cat([torch.randn(1, 4, h2, w2, generator=g, device=dev) for g in gens])
                    second.append((k, embeds, s0, idx, enlarge(lat, enc), noise2))
            if hi is None:
                finish(scale, paths)
        if hi is not None:
            del enc
            # the one rebuild: the UNet's (and the decoder's) buffers belong to the first shape they ran; a tiled decoder runs at the tile's shape and stays
            loaded.prepare(n, h2, w2, **({} if vt is None else dict(keep_decoder=True)), **td_kw(td_plan2))
            for k, scale in enumerate(lora_scales):
                stack.sampler.set_lora_scale(scale)
                paths = []
                for k1, embeds, s0, idx, x0, noise2 in second:
                    if k1 == k:
                        lat = sample(embeds, idx, h2, w2, hi["size"], noise2, dict(kw2, init_latents=x0, strength=hi["strength"], **tile_kw(td_plan2)), seed + 2 ** 32, hi["steps"],
                                     heat=hm_cols is not None)
                        save(lat, idx, s0, scale, paths)
                finish(scale, paths)
    finally:
        stack.sampler.set_lora_scale(1.0)
    with open(os.path.join(out_dir, "prompts.json"), "w") as fh:
        meta = dict(prompts=prompts, lora_scales=list(lora_scales), size=list(size), steps=steps, guidance_scale=guidance_scale, seed=seed)
        if init_image is not None:
            meta.update(strength=strength, masked=mask_image is not None)
        if change_map_image is not None:
            meta.update(change_map=dict(file=change_map_image if isinstance(change_map_image, str) else None, mask_blur=float(mask_blur or 0.0)))
        elif mask_blur:
            meta.update(mask_blur=float(mask_blur))
        if (sampler, sigmas) != ("euler", "trailing"):
            meta.update(sampler=sampler, sigmas=sigmas)
        if sde:
            meta.update(eta=eta)
        if guidance_rescale != 0.0:
            meta.update(guidance_rescale=guidance_rescale)
        if guidance_interval is not None:
            meta.update(guidance_interval=list(guidance_interval))
        if ag is not None:
            meta.update(apg=dict(zip(APG_KEYS, ag)))
        if dt is not None:
            meta.update(dynthresh=dict(zip(DYN_KEYS, dt)))
        if negative_prompt is not None:
            meta.update(negative_prompt=negative_prompt)
        if hi is not None:
            meta.update(hires=dict(hi, size=list(hi["size"]), base_size=list(hi["base_size"])))
        if fz is not None:
            meta.update(freeu=fz)
        if kd is not None:
            meta.update(kv_downsample=dict(factors=list(kd[0]), mode=kd[1], passes=kv_downsample_pass))
        if hm_cols is not None:
            meta.update(heatmap=dict(maps=hm_names, grid=heatmap_grid, positions=hm_cols.tolist()))
        if vt is not None:
            meta.update(vae_tile=dict(tile=vt[0], overlap=vt[1]))
        if tile_diffusion is not None:                  # (tiles: of the last pass; [1, 1]: every pass fitted one window and ran plain)
            T_, O_ = (tile_diffusion, tile_diffusion // 4) if isinstance(tile_diffusion, int) else tile_diffusion
            pl = td_plan2 if hi is not None else td_plan
            meta.update(tile_diffusion=dict(tile=T_, overlap=O_, tiles=[1, 1] if pl is None else [pl.ty, pl.tx]))
        if rg is not None:
            meta.update(regions=[dict(prompt=p, **(dict(box=list(wh)) if isinstance(wh, tuple) else dict(mask=wh if isinstance(wh, str) else None))) for wh, p in rg["regions"]],
                        region_base=rg["base"], region_bootstrap=rg["bootstrap"], region_feather=rg["feather"])
        json.dump(meta, fh, indent=2)
    return result


def main(argv=None, runtime=None):
    ap = argparse.ArgumentParser(prog="python -m sd_lora_trainer_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True, help="checkpoint directory written by train()")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--prompt", action="append", default=None, help="a prompt (repeatable; <concept> marks the learned concept); default: validation prompts")
    ap.add_argument("--n-validation", type=int, default=4, help="number of validation prompts when no --prompt is given")
    ap.add_argument("--lora-scale", type=float, action="append", default=None, help="adapter weight (repeatable: a sweep); default: the job's sample_imgs_lora_scale")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=None, help="image size in pixels; default: the job's validation_img_size")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--guidance", type=float, default=8.0)
    ap.add_argument("--seed", type=int, default=None, help="image i starts from seed + i; default: the job's seed")
    ap.add_argument("--images-per-batch", type=int, default=1, help="images sampled together (UNet batch 2 N)")
    ap.add_argument("--eager", action="store_true", help="issue every launch from Python instead of replaying one hipGraph per iteration (same kernels)")
    ap.add_argument("--init-image", default=None, help="start from this picture instead of pure noise (img2img); resized to --size")
    ap.add_argument("--strength", type=float, default=None, help="how much of the schedule runs on the init image, in (0, 1]; default 0.6 with --init-image")
    ap.add_argument("--mask", default=None, help="inpainting mask for --init-image: white is regenerated, black is kept")
    ap.add_argument("--change-map", default=None, help="differential diffusion for --init-image: the map's luminance is a strength per pixel - white the "
                    "whole --strength, black keep, grey in between")
    ap.add_argument("--mask-blur", type=float, default=None, metavar="SIGMA", help="blur --change-map's map (or --mask's mask) by a Gaussian of SIGMA latent pixels first")
    ap.add_argument("--sampler", choices=("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde"), default="euler",
                    help="integrator: first-order Euler, DPM-Solver++ (2M) (second order: about half the steps), or their stochastic forms - Euler ancestral, "
                    "DPM-Solver++ (2M) SDE - which add fresh noise after every step")
    ap.add_argument("--eta", type=float, default=None, help="amount of per-step noise of --sampler euler_a / dpmpp_2m_sde, >= 0 (default 1; 0: none)")
    ap.add_argument("--sigmas", choices=("trailing", "karras"), default="trailing", help="noise levels: those of trailing timesteps, or Karras et al. (rho = 7)")
    ap.add_argument("--guidance-rescale", type=float, default=0.0, help="rescale the guided prediction to the positive one's standard deviation, blended with this weight in [0, 1] (default 0: off)")
    ap.add_argument("--guidance-interval", type=float, nargs=2, metavar=("SIGMA_LO", "SIGMA_HI"), default=None,
                    help="apply guidance only at the steps whose noise level lies in (SIGMA_LO, SIGMA_HI]")
    ap.add_argument("--apg", action="store_true", help="adaptive projected guidance (Sadat et al. 2024): project, clip and average the guidance update; "
                    f"defaults eta {APG_DEFAULT[0]:g}, norm threshold {APG_DEFAULT[1]:g}, momentum {APG_DEFAULT[2]:g}")
    ap.add_argument("--apg-eta", type=float, default=None, metavar="F", help="with --apg: weight of the update's part parallel to the positive prediction, in [0, 1]")
    ap.add_argument("--apg-norm-threshold", type=float, default=None, metavar="F", help="with --apg: bound of the update's norm over the image, >= 0 (0: no clip)")
    ap.add_argument("--apg-momentum", type=float, default=None, metavar="F", help="with --apg: weight of the previous steps' running average, in (-1, 1) (0: none)")
    ap.add_argument("--dynthresh", type=float, nargs="?", const=DYN_DEFAULT[0], default=None, metavar="MIMIC",
                    help=f"dynamic thresholding: every latent channel of the guided prediction gets the value range of the prediction at guidance scale MIMIC (default {DYN_DEFAULT[0]:g})")
    ap.add_argument("--dynthresh-percentile", type=float, default=None, metavar="F", help=f"with --dynthresh: the quantile of the prediction's own deviations the clamp stays above, in (0, 1] (default {DYN_DEFAULT[1]:g})")
    ap.add_argument("--dynthresh-interpolate", type=float, default=None, metavar="F", help=f"with --dynthresh: weight of the thresholded prediction against the plain one, in [0, 1] (default {DYN_DEFAULT[2]:g})")
    ap.add_argument("--negative-prompt", default=None, help="the negative prompt; default: the fixed one of the training-time renders")
    ap.add_argument("--hires-scale", type=float, default=None, help="two passes: sample at --size, enlarge by this factor (each axis rounded to the VAE's multiple), finish at the large size")
    ap.add_argument("--hires-size", type=int, nargs=2, metavar=("W", "H"), default=None, help="two passes with the final size given in pixels instead of a factor")
    ap.add_argument("--hires-strength", type=float, default=None, help="how much of the second pass's schedule runs on the enlarged picture, in (0, 1]; default 0.6")
    ap.add_argument("--hires-steps", type=int, default=None, help="step count of the second pass's schedule; default: --steps")
    ap.add_argument("--hires-upscaler", choices=HIRES_UPSCALERS, default=None, help="enlarge the latents (default), or the decoded picture through the VAE")
    ap.add_argument("--hires-resample", choices=("nearest", "bilinear", "bicubic"), default=None, help="resampling filter; default: bilinear for latent, bicubic for pixel")
    ap.add_argument("--freeu", type=float, nargs=4, metavar=("B1", "B2", "S1", "S2"), default=None,
                    help="FreeU: backbone factors B1, B2 and skip low-frequency factors S1, S2 of the first two decoder stages (e.g. 1.3 1.4 0.9 0.2)")
    ap.add_argument("--freeu-v2", action="store_true", help="with --freeu: scale the backbone by its normalised channel mean (FreeU_V2) instead of a constant")
    ap.add_argument("--heatmap", nargs="*", metavar="WORD", default=None,
                    help="write cross-attention heat maps beside every picture: one for the checkpoint's trigger tokens and one per WORD of the prompt; a map takes "
                    f"the first {HEAT_P} context positions of its token (trigger tokens, or a word's BPE pieces over all its occurrences) and warns about more")
    ap.add_argument("--heatmap-grid", choices=("max", "min"), default=None, help="resolution of the maps: the finest (default) or the coarsest hooked attention grid")
    ap.add_argument("--kv-downsample", type=int, nargs="+", metavar="F", default=None,
                    help="key / value token downsampling in the self-attentions: integer factors per axis, largest token grid first (2: the largest grid only; "
                    "4 2: 4 there, 2 on the next); queries stay at full resolution")
    ap.add_argument("--kv-downsample-mode", choices=("nearest", "area"), default=None, help="with --kv-downsample: take every F-th token (default), or the mean of each F x F window")
    ap.add_argument("--kv-downsample-pass", choices=KV_PASSES, default=None,
                    help="with --kv-downsample: hires (default) - only the second pass of a --hires-scale / --hires-size render; all - every pass")
    ap.add_argument("--vae-tile", type=int, nargs="?", const=VAE_TILE, default=None, metavar="T",
                    help=f"run the VAE in tiles of T x T latent units (default {VAE_TILE}: {8 * VAE_TILE} px with the SD / SDXL VAE) blended on the device: bounded memory "
                    "and one decoder shape at any picture size")
    ap.add_argument("--vae-tile-overlap", type=int, default=None, metavar="O",
                    help=f"with --vae-tile: least overlap of neighbouring tiles in latent units, 0 <= 2 O <= T (default {VAE_TILE_OVERLAP})")
    ap.add_argument("--tile-diffusion", type=int, nargs="?", const=TILE_DIFFUSION_JOB, default=None, metavar="T",
                    help="tiled diffusion (MultiDiffusion): where a pass's latent exceeds T x T latent units the UNet runs on overlapping T x T windows, fused "
                    "on the device at every step - one UNet shape at any picture size (default T: the job's resolution // 8)")
    ap.add_argument("--tile-diffusion-overlap", type=int, default=None, metavar="O",
                    help="with --tile-diffusion: least overlap of neighbouring windows in latent units, 0 <= 2 O <= T (default T // 4)")
    ap.add_argument("--region", nargs=2, action="append", default=None, metavar=("MASK.png|x0,y0,x1,y1", "PROMPT"),
                    help="a region with a prompt of its own (repeatable): a mask picture (white: the region) or a box in fractions of the picture; <concept> is "
                    "allowed in PROMPT; --prompt rules wherever no region has weight")
    ap.add_argument("--region-feather", type=float, default=None, metavar="SIGMA", help="with --region: blur each mask by a Gaussian of SIGMA latent pixels")
    ap.add_argument("--region-base", type=float, default=None, metavar="F", help="with --region: extra weight of the main prompt everywhere (default 0)")
    ap.add_argument("--region-bootstrap", type=float, default=None, metavar="SHARE",
                    help=f"with --region: share of the steps at which a region sees a noised solid colour outside its mask (default {REGION_BOOTSTRAP}; 0: off)")
    ap.add_argument("--device", default="cuda:0")
    for flag, key, what in (("--unet", "path", "base UNet weights or synthetic:<version>"), ("--text-encoder", "text_encoder_path", "text encoder state dict"),
                            ("--text-encoder-2", "text_encoder_2_path", "SDXL's second text encoder"), ("--vae", "vae_path", "AutoencoderKL state dict"),
                            ("--tokenizer", "tokenizer_path", "directory with vocab.json + merges.txt")):
        ap.add_argument(flag, dest=key, default=None, help=what + " (default: the job's)")
    a = ap.parse_args(argv)
    if a.init_image is None and (a.mask is not None or a.strength is not None):
        ap.error("--mask and --strength need --init-image")
    if a.init_image is None and (a.change_map is not None or a.mask_blur is not None):
        ap.error("--change-map and --mask-blur need --init-image")
    if a.change_map is not None and a.mask is not None:
        ap.error("--change-map and --mask exclude each other")
    if a.mask_blur is not None and a.mask is None and a.change_map is None:
        ap.error("--mask-blur needs --change-map or --mask")
    if a.mask_blur is not None and not (math.isfinite(a.mask_blur) and a.mask_blur >= 0.0):
        ap.error(f"--mask-blur must be a finite number >= 0, got {a.mask_blur}")
    if a.eta is not None and a.sampler not in ("euler_a", "dpmpp_2m_sde"):
        ap.error(f"--eta needs --sampler euler_a or dpmpp_2m_sde: --sampler {a.sampler} adds no noise")
    if a.eta is not None and not a.eta >= 0.0:
        ap.error(f"--eta must be >= 0, got {a.eta}")
    if not 0.0 <= a.guidance_rescale <= 1.0:
        ap.error(f"--guidance-rescale must be in [0, 1], got {a.guidance_rescale}")
    if a.guidance_interval is not None and not a.guidance_interval[0] < a.guidance_interval[1]:
        ap.error(f"--guidance-interval needs SIGMA_LO < SIGMA_HI, got {a.guidance_interval[0]} {a.guidance_interval[1]}")
    apg = {}
    given = {k: v for k, v in zip(APG_KEYS, (a.apg_eta, a.apg_norm_threshold, a.apg_momentum)) if v is not None}
    if given and not a.apg:
        ap.error("--apg-eta, --apg-norm-threshold and --apg-momentum need --apg")
    if a.apg:
        try:
            apg = dict(apg=apg_args(given or True))
        except ValueError as e:
            ap.error(f"--apg-eta / --apg-norm-threshold / --apg-momentum: {e}")
    dyn = {}
    given = {k: v for k, v in zip(DYN_KEYS[1:], (a.dynthresh_percentile, a.dynthresh_interpolate)) if v is not None}
    if given and a.dynthresh is None:
        ap.error("--dynthresh-percentile and --dynthresh-interpolate need --dynthresh")
    if a.dynthresh is not None:
        if a.apg or a.guidance_rescale:
            ap.error("--dynthresh does not combine with " + ("--apg" if a.apg else "--guidance-rescale") + ": they are alternative answers to the same fault")
        try:
            dyn = dict(dynthresh=dynthresh_args(dict(given, mimic=a.dynthresh)))
        except ValueError as e:
            ap.error(f"--dynthresh / --dynthresh-percentile / --dynthresh-interpolate: {e}")
    if a.strength is not None and not 0.0 < a.strength <= 1.0:
        ap.error(f"--strength must be in (0, 1], got {a.strength}")
    if a.heatmap_grid is not None and a.heatmap is None:
        ap.error("--heatmap-grid needs --heatmap")
    if a.heatmap is not None and any(not w_.strip() for w_ in a.heatmap):
        ap.error("--heatmap takes non-empty words")
    if a.freeu_v2 and a.freeu is None:
        ap.error("--freeu-v2 needs --freeu B1 B2 S1 S2")
    if a.freeu is not None and not all(math.isfinite(v) and v > 0.0 for v in a.freeu):
        ap.error(f"--freeu takes four finite positive numbers, got {' '.join(str(v) for v in a.freeu)}")
    if a.kv_downsample is None and (a.kv_downsample_mode is not None or a.kv_downsample_pass is not None):
        ap.error("--kv-downsample-mode and --kv-downsample-pass need --kv-downsample F [F2 ...]")
    if a.kv_downsample is not None and not all(f_ >= 1 for f_ in a.kv_downsample):
        ap.error(f"--kv-downsample takes integer factors >= 1, got {' '.join(str(f_) for f_ in a.kv_downsample)}")
    if a.kv_downsample is not None and (a.kv_downsample_pass or "hires") == "hires" and a.hires_scale is None and a.hires_size is None:
        ap.error("--kv-downsample applies to the second pass of a hires render by default and this render has none (--hires-scale / --hires-size): "
                 "pass --kv-downsample-pass all to use it in a single-pass render")
    kvd = {} if a.kv_downsample is None else dict(kv_downsample=tuple(a.kv_downsample), kv_downsample_mode=a.kv_downsample_mode or "nearest",
                                                   kv_downsample_pass=a.kv_downsample_pass or "hires")
    if a.vae_tile is None and a.vae_tile_overlap is not None:
        ap.error("--vae-tile-overlap needs --vae-tile [T]")
    vtile = {}
    if a.vae_tile is not None:
        vtile = dict(vae_tile=(a.vae_tile, VAE_TILE_OVERLAP if a.vae_tile_overlap is None else a.vae_tile_overlap))
        try:
            vae_tile_args(vtile["vae_tile"])
        except ValueError as e:
            ap.error(f"--vae-tile / --vae-tile-overlap: {e}")
    if a.tile_diffusion is None and a.tile_diffusion_overlap is not None:
        ap.error("--tile-diffusion-overlap needs --tile-diffusion [T]")
    if a.tile_diffusion is not None and a.tile_diffusion is not TILE_DIFFUSION_JOB:
        from . import sampler as SM
        try:                                            # (without T the overlap is checked by render(), once the job's T is known)
            SM.tile_plan(1, 1, (a.tile_diffusion, a.tile_diffusion // 4 if a.tile_diffusion_overlap is None else a.tile_diffusion_overlap))
        except ValueError as e:
            ap.error(f"--tile-diffusion / --tile-diffusion-overlap: {e}")
    if a.tile_diffusion is not None and a.heatmap is not None:
        ap.error("--tile-diffusion does not combine with --heatmap")
    regs = {}
    if a.region is None:
        if a.region_feather is not None or a.region_base is not None or a.region_bootstrap is not None:
            ap.error("--region-feather, --region-base and --region-bootstrap need --region")
    else:
        for flag, on in (("--tile-diffusion", a.tile_diffusion is not None), ("--heatmap", a.heatmap is not None),
                         ("--hires-scale / --hires-size", any(v is not None for v in (a.hires_scale, a.hires_size, a.hires_strength, a.hires_steps, a.hires_upscaler, a.hires_resample)))):
            if on:
                ap.error(f"--region does not combine with {flag}")
        regs = dict(regions=[(region_spec(where), prompt) for where, prompt in a.region],
                    **{k: v for k, v in dict(region_feather=a.region_feather, region_base=a.region_base, region_bootstrap=a.region_bootstrap).items() if v is not None})
        try:
            region_args(**regs)
        except ValueError as e:
            ap.error(f"--region / --region-feather / --region-base / --region-bootstrap: {e}")
        for where, _ in regs["regions"]:
            if isinstance(where, str) and not os.path.exists(where):
                ap.error(f"--region: {where!r} is neither a box x0,y0,x1,y1 nor a mask picture that exists")
    freeu = None if a.freeu is None else dict(zip(("b1", "b2", "s1", "s2"), a.freeu), version=2 if a.freeu_v2 else 1)
    hires = None
    if a.hires_scale is not None and a.hires_size is not None:
        ap.error("--hires-scale and --hires-size exclude each other")
    if a.hires_scale is None and a.hires_size is None:
        if any(v is not None for v in (a.hires_strength, a.hires_steps, a.hires_upscaler, a.hires_resample)):
            ap.error("--hires-strength, --hires-steps, --hires-upscaler and --hires-resample need --hires-scale or --hires-size")
    else:
        if a.mask is not None:
            ap.error("--hires-scale / --hires-size do not combine with --mask")
        if a.change_map is not None:
            ap.error("--hires-scale / --hires-size do not combine with --change-map")
        if a.hires_strength is not None and not 0.0 < a.hires_strength <= 1.0:
            ap.error(f"--hires-strength must be in (0, 1], got {a.hires_strength}")
        if a.hires_steps is not None and a.hires_steps < 1:
            ap.error(f"--hires-steps must be >= 1, got {a.hires_steps}")
        hires = {k: v for k, v in dict(scale=a.hires_scale, size=a.hires_size, strength=a.hires_strength, steps=a.hires_steps, upscaler=a.hires_upscaler,
                                       resample=a.hires_resample).items() if v is not None}
    over = {k: getattr(a, k) for k in ("path", "text_encoder_path", "text_encoder_2_path", "vae_path", "tokenizer_path") if getattr(a, k)}
    pm = None
    if over and os.path.exists(os.path.join(a.checkpoint, "training_args.json")):
        with open(os.path.join(a.checkpoint, "training_args.json")) as f:
            pm = dict(json.load(f).get("pretrained_model") or {}, **over)
    loaded = load_for_inference(a.checkpoint, pm, device=a.device, runtime=runtime)
    tdiff = {}
    if a.tile_diffusion is not None:                    # T defaults to the job's training resolution in latent units
        T_ = tile_diffusion_default(loaded.config) if a.tile_diffusion is TILE_DIFFUSION_JOB else a.tile_diffusion
        tdiff = dict(tile_diffusion=(T_, T_ // 4 if a.tile_diffusion_overlap is None else a.tile_diffusion_overlap))
    res = render(loaded, a.prompt, a.out, lora_scales=a.lora_scale, size=a.size, steps=a.steps, guidance_scale=a.guidance, seed=a.seed,
                 images_per_batch=a.images_per_batch, graph=not a.eager, n_validation=a.n_validation, init_image=a.init_image, strength=a.strength,
                 mask_image=a.mask, sampler=a.sampler, sigmas=a.sigmas, eta=a.eta, guidance_rescale=a.guidance_rescale,
                 guidance_interval=a.guidance_interval, negative_prompt=a.negative_prompt, **({} if hires is None else dict(hires=hires)),
                 **({} if freeu is None else dict(freeu=freeu)), **kvd, **vtile, **tdiff, **regs, **apg, **dyn,
                 **({} if a.change_map is None else dict(change_map_image=a.change_map)), **({} if a.mask_blur is None else dict(mask_blur=a.mask_blur)),
                 **({} if a.heatmap is None else dict(heatmap=a.heatmap, heatmap_grid=a.heatmap_grid or "max")))
    for scale, paths in res.items():
        print(f"lora_scale {scale}: {len(paths)} image(s), {os.path.join(a.out, 'grid_scale' + _scale_tag(scale) + '.jpg')}")
    return res


if __name__ == "__main__":
    main()
