"""Validation sampling in latent space (/root/reference trainer/inference.py:180-214, 289-385): the UNet of
the training step in inference mode under the reference's render settings - Euler-discrete scheduler with trailing
timestep spacing, 25 steps, classifier-free guidance 8, LoRA adapters scaled by `sample_imgs_lora_scale` (0.75 SDXL / 0.85
SD1.5, main.py:57-61; `set_adapter_scales`, checkpoint.py:31-55) and the trigger-token strength blended between the prompt
with and without the concept (`blend_conditions`, inference.py:180-228).  Produces the final LATENTS; decoding them is the
VAE's job (vae.py).

`EulerDiscrete` restates diffusers' EulerDiscreteScheduler (0.29.2, third party, parity unpinned) for the configuration the
reference builds (`from_config(training scheduler config, timestep_spacing="trailing")`: scaled-linear betas, epsilon or
v prediction, no Karras sigmas): sigma_t = sqrt((1 - abar_t) / abar_t), timesteps = round(arange(T, 0, -T/n)) - 1, sigmas
interpolated at those timesteps plus a final 0, initial noise scaled by sigma_max (trailing spacing), model input x / sqrt(sigma^2 + 1),
x_next = x + d * (sigma_next - sigma) with d = eps (epsilon prediction).

From an init image (`sample(init_latents=, strength=, mask=)`): diffusers' img2img rule keeps the last k = min(int(steps * strength), steps)
entries of the trailing schedule (StableDiffusionImg2ImgPipeline.get_timesteps) and starts from x0 + noise * sigma of the first kept entry
(EulerDiscreteScheduler.add_noise); with a mask (1 regenerate, 0 keep) the known region is put back after every step, noised to the sigma the
step arrived at, from the same noise draw (the legacy inpainting loop of diffusers: latents = init_latents_proper * (1 - mask) + latents * mask).

Differential diffusion (`sample(init_latents=, change_map=)`; Levin & Fried 2023, "Giving Each Pixel Its Strength"): a change map c in [0, 1] gives
every pixel an img2img strength of its own.  A pixel is held on the init latents' noised trajectory (x0 + noise * sigma, the same noise draw) for the
first (1 - c) share of the steps that run, then released to finish on its own - by selection, never by mixing (`hold_map`; c = 0 is kept exactly).

Guidance controls (`sample(guidance_scale=[...], guidance_rescale=, guidance_interval=)`): a guidance scale per step, guidance applied only where
sigma_i lies in (sigma_lo, sigma_hi] (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval"; g_i = 1 elsewhere) and the rescale of Lin et
al. 2024, section 3.4 (diffusers' rescale_noise_cfg: the guided prediction is scaled to the standard deviation of the positive one, per image, and
blended with weight phi).  `guidance_table` holds (g_i, phi_i) per step; ops.guidance evaluates it on the device between the forward and the step
launch, on all three paths.

Adaptive projected guidance (`sample(apg=(eta, norm_threshold, momentum))`; Sadat et al. 2024, "Eliminating Oversaturation and Artifacts of High
Guidance Scales"; diffusers' normalized_guidance): the guidance update e_pos - e_neg is averaged over the steps with a (negative) momentum, its norm
clipped to norm_threshold, and its part parallel to the positive prediction - the part that drives saturation - scaled by eta.  `apg_table` holds
(eta_i, tau_i, beta_i) per step; ops.guidance_apg evaluates it in ops.guidance's place, the running average in a device buffer that the launch itself
restarts at step row 0.

Dynamic thresholding (`sample(dynthresh=(mimic, percentile, interpolate))`; the "Dynamic Thresholding (CFG scale fix)" extension of A1111 / ComfyUI /
SwarmUI, a latent-space form of Imagen's dynamic thresholding): sample at a strong guidance scale, but give every latent channel of the prediction the
value range it would have had at the mild `mimic` scale - the centred guided prediction is clamped to max(the mimic prediction's largest deviation, the
percentile of its own) and scaled back to the mimic prediction's range.  `dyn_table` holds (mimic_i, q_i, psi_i) per step; ops.guidance_dyn evaluates it
in ops.guidance's place, the quantile by an exact radix select inside the launch.
"""
import collections
import math
import numbers

import numpy as np
import torch

from .step import ddpm_alphas_cumprod
from .unet import CTX_PAD, F32


def blend_conditions(embeds1, embeds2, lora_scale, token_scale_power=0.4, min_token_scale=0.5, token_scale=None):
    """inference.py:180-228: linear interpolation between the conditioning WITHOUT the concept (embeds1) and WITH it
    (embeds2); token_scale = min + (1 - min) * lora_scale^power unless given.  embeds = (c, uc[, pc, puc])."""
    if token_scale is None:
        token_scale = min_token_scale + (1 - min_token_scale) * lora_scale ** token_scale_power
    e1, e2 = (tuple(embeds1) + (None, None))[:4], (tuple(embeds2) + (None, None))[:4]      # always (c, uc, pc, puc) like the reference
    out = tuple(None if (a is None or b is None) else (1 - token_scale) * a + token_scale * b for a, b in zip(e1, e2))
    return out, token_scale


class EulerDiscrete:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, prediction_type="epsilon"):
        acp = ddpm_alphas_cumprod(num_train_timesteps, beta_start, beta_end).double().numpy()
        self.sigmas_all = np.sqrt((1 - acp) / acp)
        self.T, self.prediction_type = num_train_timesteps, prediction_type

    def set_timesteps(self, n, start=0, sigmas="trailing"):
        """start: skip the first `start` entries of the schedule (img2img: the trajectory begins at timesteps[start] of the n-step schedule).
        sigmas: "trailing" (diffusers' trailing timestep spacing, the sigmas of those timesteps) | "karras" (KARRAS_RHO-spaced noise levels)."""
        assert 0 <= start < n
        if sigmas == "trailing":
            ts = np.round(np.arange(self.T, 0, -self.T / n))[start:] - 1               # "trailing"
            sig = np.interp(ts, np.arange(self.T), self.sigmas_all)
        elif sigmas == "karras":
            sig = karras_sigmas(n, float(self.sigmas_all[0]), float(self.sigmas_all[-1]))[start:]
            ts = np.interp(np.log(sig), np.log(self.sigmas_all), np.arange(self.T))    # sigmas_all rises with t: the fractional training timestep of each level
        else:
            raise ValueError(f"sigmas must be 'trailing' or 'karras', got {sigmas!r}")
        self.timesteps = ts.astype(np.float32)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        # diffusers 0.29.2 EulerDiscreteScheduler.init_noise_sigma: max(sigmas) for timestep_spacing in ("linspace", "trailing") -
        # the reference's configuration (inference.py:358-360); sqrt(sigma_max^2 + 1) only for "leading"
        self.init_noise_sigma = float(self.sigmas.max())
        self._begin()
        return self

    def set_sigmas(self, sigmas, timesteps=None):
        """A noise-level grid of the caller's own (decreasing; a final 0 is optional and NOT appended), kept in the dtype given: fp64 for order studies."""
        self.sigmas = np.asarray(sigmas)
        n = len(self.sigmas) - 1
        self.timesteps = np.zeros(n, dtype=np.float32) if timesteps is None else np.asarray(timesteps, dtype=np.float32)
        assert n >= 1 and len(self.timesteps) == n and bool((np.diff(self.sigmas) < 0).all())
        self.init_noise_sigma = float(self.sigmas.max())
        self._begin()
        return self

    def _begin(self):
        """A trajectory starts: nothing to prepare for a one-step method."""

    def scale_model_input(self, x, i):
        return x / float(np.sqrt(self.sigmas[i] ** 2 + 1))

    def step(self, model_out, i, x):
        s, sn = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if self.prediction_type == "epsilon":
            d = model_out
        else:                                                                     # v_prediction
            x0 = model_out * (-s / (s * s + 1) ** 0.5) + x / (s * s + 1)
            d = (x - x0) / s
        return x + d * (sn - s)


KARRAS_RHO = 7.0


def karras_sigmas(n, sigma_min, sigma_max, rho=KARRAS_RHO):
    """Karras et al. 2022, eq. 5: sigma_i = (sigma_max^(1/rho) + i / (n - 1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho, i = 0 .. n - 1 (fp64; without the final 0)."""
    ramp = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    lo, hi = sigma_min ** (1.0 / rho), sigma_max ** (1.0 / rho)
    sig = (hi + ramp * (lo - hi)) ** rho
    sig[0] = sigma_max                                      # exactly, not to a rounding of the power
    if n > 1:
        sig[-1] = sigma_min
    return sig


def ms_coefficients(sigmas):
    """DPM-Solver++ (2M) on the grid `sigmas` [k + 1] -> fp64 [k, 3]: (a_i, b_i, c_i) of x_{i+1} = a x + b D_i + c D_{i-1} (module docstring).
    Row 0 (no history yet) and a step to sigma = 0 (h is infinite there) are first order: c = 0 exactly."""
    sig = np.asarray(sigmas, dtype=np.float64)
    k = len(sig) - 1
    out = np.zeros((k, 3), dtype=np.float64)
    h_prev = None
    for i in range(k):
        s, sn = sig[i], sig[i + 1]
        a = sn / s
        if sn == 0.0 or h_prev is None:
            b, c = 1.0 - a, 0.0
        else:
            h = np.log(s) - np.log(sn)                      # lambda_{i+1} - lambda_i, lambda = -log sigma
            r = h_prev / h
            b, c = (1.0 - a) * (1.0 + 1.0 / (2.0 * r)), -(1.0 - a) / (2.0 * r)
        out[i] = (a, b, c)
        h_prev = None if sn == 0.0 else np.log(s) - np.log(sn)
    return out


class DpmSolverPP2M(EulerDiscrete):
    """DPM-Solver++ (2M) (module docstring) on EulerDiscrete's schedules: same sigmas, timesteps, model input and init noise; `step` keeps the previous
    denoised value, so steps are taken in order, i = 0 first (set_timesteps / set_sigmas start a trajectory)."""

    def _begin(self):
        self.coeffs = ms_coefficients(self.sigmas)          # fp64, from the sigmas as stored (fp32 from set_timesteps)
        self._dprev = None

    def denoised(self, model_out, i, x):
        s = float(self.sigmas[i])
        if self.prediction_type == "epsilon":
            return x - model_out * s
        return model_out * (-s / (s * s + 1) ** 0.5) + x / (s * s + 1)

    def step(self, model_out, i, x):
        if i == 0:
            self._dprev = None
        a, b, c = (float(v) for v in self.coeffs[i])
        D = self.denoised(model_out, i, x)
        xn = x * a + D * b
        if c != 0.0:
            xn = xn + self._dprev * c
        self._dprev = D
        return xn


SDE_KINDS = ("euler_a", "dpmpp_2m_sde")


def sde_coefficients(sigmas, kind, eta=1.0):
    """The stochastic samplers on the grid `sigmas` [k + 1] -> fp64 [k, 4]: (a_i, b_i, c_i, d_i) of x_{i+1} = a x + b D_i + c D_{i-1} + d z_i with
    z_i ~ N(0, I) fresh per step.  With s = sigma_i, sn = sigma_{i+1}:
      "euler_a"       k-diffusion's sample_euler_ancestral: sigma_up = min(sn, eta sqrt(sn^2 (s^2 - sn^2) / s^2)), sigma_down = sqrt(sn^2 - sigma_up^2),
                      a = sigma_down / s, b = 1 - a, c = 0, d = sigma_up
      "dpmpp_2m_sde"  k-diffusion's sample_dpmpp_2m_sde (midpoint, s_noise = 1): h = ln s - ln sn, E = -expm1(-(1 + eta) h), a = (sn / s) e^(-eta h),
                      b = E (1 + 1 / (2 r)), c = -E / (2 r), r = h_prev / h, d = sn sqrt(-expm1(-2 eta h)); row 0 and a step to sn = 0 are first
                      order (b = E, c = 0 exactly)
    A row with sn = 0 is (0, 1, 0, 0): x = D, no noise.  eta = 0 is a branch of its own, not a rounding: ms_coefficients' rows with d = 0, and Euler's
    rows (sn / s, 1 - sn / s, 0, 0)."""
    if kind not in SDE_KINDS:
        raise ValueError(f"kind must be one of {SDE_KINDS}, got {kind!r}")
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta!r}")
    sig = np.asarray(sigmas, dtype=np.float64)
    k = len(sig) - 1
    out = np.zeros((k, 4), dtype=np.float64)
    if eta == 0.0:
        if kind == "dpmpp_2m_sde":
            out[:, :3] = ms_coefficients(sig)
        else:
            out[:, 0] = sig[1:] / sig[:-1]
            out[:, 1] = 1.0 - out[:, 0]
        return out
    h_prev = None
    for i in range(k):
        s, sn = sig[i], sig[i + 1]
        if sn == 0.0:
            out[i] = (0.0, 1.0, 0.0, 0.0)
            h_prev = None
        elif kind == "euler_a":
            up = min(sn, eta * np.sqrt(sn * sn * (s * s - sn * sn) / (s * s)))
            a = np.sqrt(sn * sn - up * up) / s
            out[i] = (a, 1.0 - a, 0.0, up)
        else:
            h = np.log(s) - np.log(sn)
            E = -np.expm1(-(1.0 + eta) * h)
            b, c = E, 0.0
            if h_prev is not None:
                r = h_prev / h
                b, c = E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r)
            out[i] = ((sn / s) * np.exp(-eta * h), b, c, sn * np.sqrt(-np.expm1(-2.0 * eta * h)))
            h_prev = h
    return out


class _Stochastic(DpmSolverPP2M):
    """A stochastic sampler on EulerDiscrete's schedules, in DpmSolverPP2M's shape: `step(model_out, i, x, z)` takes the step's noise z ~ N(0, I)
    (ignored on a row with d = 0).  On fp32 tensors model input, denoised value and update are the step kernel's contract (sdlt_sampler_step_sde:
    the table's fp32 factors, one rounding per operation, in its order), so the torch loop and the fused path agree bit for bit."""
    KIND = None

    def __init__(self, *args, eta=1.0, **kw):
        super().__init__(*args, **kw)
        self.eta = eta

    def _begin(self):
        self.coeffs = sde_coefficients(self.sigmas, self.KIND, self.eta)
        self._dprev = None

    def scale_model_input(self, x, i):
        return x * float(1.0 / np.sqrt(np.float64(self.sigmas[i]) ** 2 + 1.0))

    def denoised(self, model_out, i, x):
        if self.prediction_type == "epsilon":
            return x - model_out * float(self.sigmas[i])
        f = np.float32 if x.dtype == torch.float32 else np.float64      # the scalars in the tensors' precision; a full-tensor divisor: IEEE division
        s = f(self.sigmas[i])
        q = s * s + f(1.0)
        return model_out * float(-s / np.sqrt(q)) + x / torch.full_like(x, float(q))

    def step(self, model_out, i, x, z=None):
        if i == 0:
            self._dprev = None
        a, b, c, d = (float(v) for v in self.coeffs[i])
        D = self.denoised(model_out, i, x)
        xn = x * a + D * b
        if c != 0.0:
            xn = xn + self._dprev * c
        if d != 0.0:
            xn = xn + z * d
        self._dprev = D
        return xn


class EulerAncestral(_Stochastic):
    """k-diffusion's sample_euler_ancestral (sde_coefficients)."""
    KIND = "euler_a"


class DpmSolverPP2MSDE(_Stochastic):
    """k-diffusion's sample_dpmpp_2m_sde, midpoint solver, s_noise = 1 (sde_coefficients)."""
    KIND = "dpmpp_2m_sde"


class EulerStepOrder(EulerDiscrete):
    """EulerDiscrete with model input and update in sdlt_sampler_step's contract on fp32 tensors (the table's fp32 factors, one rounding per
    operation, in its order), as _Stochastic restates sdlt_sampler_step_sde: the torch loop and the fused path then agree bit for bit.  The torch loop
    uses it where the guidance pre-pass runs."""

    def scale_model_input(self, x, i):
        return x * float(1.0 / np.sqrt(np.float64(self.sigmas[i]) ** 2 + 1.0))

    def step(self, model_out, i, x):
        f = np.float32
        s, sn = f(self.sigmas[i]), f(self.sigmas[i + 1])
        d = model_out
        if self.prediction_type != "epsilon":                # (the scalars in fp32; full-tensor divisors: IEEE division)
            q = s * s + f(1.0)
            c1 = -s / np.sqrt(q)
            d = (x - (model_out * float(c1) + x / torch.full_like(x, float(q)))) / torch.full_like(x, float(s))
        return x + d * float(sn - s)


def guidance_in_use(guidance_scale, guidance_rescale=0.0, guidance_interval=None):
    """Whether sample() launches the guidance pre-pass: not for a scalar guidance scale without rescale and interval (today's tables and captures)."""
    return not isinstance(guidance_scale, numbers.Real) or guidance_rescale != 0.0 or guidance_interval is not None


def guidance_table(sched, guidance_scale, guidance_rescale=0.0, guidance_interval=None):
    """The device table of ops.guidance for a scheduler whose set_timesteps(n[, start]) has run: fp32 [1 + k, 4] for the k steps that run, row 0
    (k, 0, 0, 0), row 1 + i (g_i, phi_i, 0, 0).  guidance_scale: a number, or one per step that runs; guidance_interval (sigma_lo, sigma_hi): g_i = 1
    where sigma_i lies outside (sigma_lo, sigma_hi]; guidance_rescale in [0, 1] is phi, on the rows whose (fp32) g_i is not 1."""
    k = len(sched.timesteps)
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale!r}")
    if isinstance(guidance_scale, numbers.Real):
        g = np.full(k, float(guidance_scale), dtype=np.float64)
    else:
        g = np.array([float(v) for v in guidance_scale], dtype=np.float64)
        if g.shape != (k,):
            raise ValueError(f"guidance_scale: {len(g)} value(s) for the {k} step(s) that run (one each, or a number)")
    if guidance_interval is not None:
        lo, hi = (float(v) for v in guidance_interval)
        if not lo < hi:
            raise ValueError(f"guidance_interval must be (sigma_lo, sigma_hi) with sigma_lo < sigma_hi, got {guidance_interval!r}")
        sig = np.asarray(sched.sigmas[:k], dtype=np.float64)
        g[~((sig > lo) & (sig <= hi))] = 1.0
    tab = np.zeros((1 + k, 4), dtype=np.float32)
    tab[0, 0] = k
    tab[1:, 0] = g
    tab[1:, 1] = np.where(tab[1:, 0] != 1.0, np.float32(phi), np.float32(0.0))
    return torch.from_numpy(tab)


def apg_table(sched, apg, k=None):
    """The device table of ops.guidance_apg beside guidance_table's, for a scheduler whose set_timesteps(n[, start]) has run: fp32 [1 + k, 4] for the k
    steps that run (None: all of the scheduler's), row 0 (k, 0, 0, 0), row 1 + i (eta_i, tau_i, beta_i, 0).  apg: (eta, norm_threshold, momentum) as
    numbers, or one such tuple per step that runs.  eta in [0, 1] scales the update's part parallel to the positive prediction (1: keep it, 0: drop it),
    norm_threshold >= 0 bounds the update's norm over the image (0: no clip), |momentum| < 1 is the weight of the previous steps' running average
    (0: none; the paper's are negative).  ValueError otherwise."""
    k = len(sched.timesteps) if k is None else k
    rows = list(apg) if isinstance(apg, (tuple, list)) else None
    if rows is not None and len(rows) == 3 and all(isinstance(v, numbers.Real) and not isinstance(v, bool) for v in rows):
        rows = [tuple(rows)] * k
    elif rows is None or len(rows) != k or not all(isinstance(r, (tuple, list)) and len(r) == 3 and
                                                   all(isinstance(v, numbers.Real) and not isinstance(v, bool) for v in r) for r in rows):
        raise ValueError(f"apg takes (eta, norm_threshold, momentum) as three numbers, or one such tuple for each of the {k} step(s) that run, got {apg!r}")
    tab = np.zeros((1 + k, 4), dtype=np.float32)
    tab[0, 0] = k
    for i, (eta, tau, beta) in enumerate(rows):
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"apg: eta must be in [0, 1], got {eta!r}")
        if not (tau >= 0.0 and math.isfinite(tau)):
            raise ValueError(f"apg: norm_threshold must be a finite number >= 0 (0: no clip), got {tau!r}")
        if not abs(beta) < 1.0:
            raise ValueError(f"apg: momentum must lie in (-1, 1), got {beta!r}")
        tab[1 + i, :3] = (eta, tau, beta)
    return torch.from_numpy(tab)


def dyn_table(sched, dynthresh, k=None):
    """The device table of ops.guidance_dyn beside guidance_table's, for a scheduler whose set_timesteps(n[, start]) has run: fp32 [1 + k, 4] for the k
    steps that run (None: all of the scheduler's), row 0 (k, 0, 0, 0), row 1 + i (mimic_i, q_i, psi_i, 0).  dynthresh: (mimic, percentile, interpolate)
    as numbers, or one such tuple per step that runs.  mimic >= 1 is the guidance scale whose value range every channel gets, percentile in (0, 1] the
    quantile of the guided prediction's own deviations that the clamp may not go below (1: the maximum), interpolate in [0, 1] the weight of the
    thresholded prediction against the plain guided one (1: all of it).  ValueError otherwise."""
    k = len(sched.timesteps) if k is None else k
    real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool)  # noqa: E731
    rows = list(dynthresh) if isinstance(dynthresh, (tuple, list)) else None
    if rows is not None and len(rows) == 3 and all(real(v) for v in rows):
        rows = [tuple(rows)] * k
    elif rows is None or len(rows) != k or not all(isinstance(r, (tuple, list)) and len(r) == 3 and all(real(v) for v in r) for r in rows):
        raise ValueError(f"dynthresh takes (mimic, percentile, interpolate) as three numbers, or one such tuple for each of the {k} step(s) that run, got {dynthresh!r}")
    tab = np.zeros((1 + k, 4), dtype=np.float32)
    tab[0, 0] = k
    for i, (mimic, q, psi) in enumerate(rows):
        if not (mimic >= 1.0 and math.isfinite(mimic)):
            raise ValueError(f"dynthresh: mimic must be a finite guidance scale >= 1, got {mimic!r}")
        if not 0.0 < q <= 1.0:
            raise ValueError(f"dynthresh: percentile must lie in (0, 1], got {q!r}")
        if not 0.0 <= psi <= 1.0:
            raise ValueError(f"dynthresh: interpolate must be in [0, 1], got {psi!r}")
        tab[1 + i, :3] = (mimic, q, psi)
    return torch.from_numpy(tab)


SAMPLERS = ("euler", "dpmpp_2m", "euler_a", "dpmpp_2m_sde")
SIGMAS = ("trailing", "karras")


def sampler_args(sampler, sigmas, eta):
    """sample()'s / render()'s `sampler`, `sigmas` and `eta`, checked -> eta (None: 1).  Only the stochastic samplers read eta, so only theirs is checked."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if sigmas not in SIGMAS:
        raise ValueError(f"sigmas must be one of {SIGMAS}, got {sigmas!r}")
    eta = 1.0 if eta is None else eta
    if sampler in SDE_KINDS and not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta!r}")
    return eta


def require_op(ops, name, text, kernel=None):
    """A missing kernel is an error, never a fallback: NotImplementedError unless the op table has `name` (kernel: the name the message gives it)."""
    if not hasattr(ops, name):
        raise NotImplementedError(f"this op table has no {kernel or name} kernel{text}")

TABLE_ROWS = 2 + 1000      # rows of the device step table: two header rows + at most one step per training timestep
MAX_GRAPHS = 4             # captured iterations kept per sampler (one per shape and adapter scale)


def step_table(sched, guidance_scale):
    """The device table of ops.sampler_step for a scheduler whose set_timesteps(n) has run: fp32 [2 + n, 4],
    row 0 (guidance scale, init_noise_sigma, 1 / sqrt(sigma_0^2 + 1), timestep 0), row 1 (n, v prediction, 0, 0),
    row 2 + i (sigma_i, sigma_{i+1}, 1 / sqrt(sigma_{i+1}^2 + 1), timestep of step i + 1; after the last step: timestep 0 again).
    The factors are the fp32 roundings of the fp64 values of the fp32 sigmas (what scale_model_input divides by)."""
    sig, ts = sched.sigmas.astype(np.float64), sched.timesteps
    n = len(ts)
    inv = 1.0 / np.sqrt(sig ** 2 + 1.0)
    tab = np.zeros((2 + n, 4), dtype=np.float32)
    tab[0] = (guidance_scale, sched.init_noise_sigma, inv[0], ts[0])
    tab[1] = (n, 1.0 if sched.prediction_type == "v_prediction" else 0.0, 0.0, 0.0)
    tab[2:, 0], tab[2:, 1], tab[2:, 2] = sig[:-1], sig[1:], inv[1:]
    tab[2:, 3] = np.concatenate([ts[1:], ts[:1]])
    return torch.from_numpy(tab)


def img2img_steps(steps, strength):
    """diffusers' img2img rule -> (k steps to run, index of the first one in the `steps`-entry schedule)."""
    if not (isinstance(strength, (int, float)) and 0.0 < strength <= 1.0):
        raise ValueError(f"strength must be in (0, 1], got {strength!r}")
    k = min(int(steps * strength), steps)
    if k < 1:
        raise ValueError(f"strength {strength} of {steps} steps leaves no step to run (int(steps * strength) = {k})")
    return k, steps - k


def hold_map(c, k):
    """The hold map of a change map for a trajectory of k steps (after strength): c fp32 [..] in [0, 1] -> fp32, integer-valued, same shape and device.
    Step row i (0-based) leaves a pixel on the init latents' noised trajectory iff i + 1 < hold (sdlt_sampler_step_dd; the torch loop alike):
      hold = k + 1                 where c == 0: held after the last step too, where sigma = 0 - the pixel ends as the init latents bit for bit
      hold = ceil((1 - c) k - g)   otherwise (c = 1: 0, never held), in fp64 from the fp32 value, g = k 2^-24
    - the paper's rule "keep before step i iff (1 - c) > i / k", restated for a select after the step; a pixel with c > 0 has hold <= k and always runs
    at least the last step free (in the paper c = 0 does too: the exact keep is this project's addition).  g: an fp32 c stands for a real number
    within 2^-25 of it, so (1 - c) k is known to k 2^-25 only; a product that exceeds an integer by less than twice that counts as the integer.  Without
    it the answer at c = i / k would follow the direction fp32 happened to round c in: fp32(0.9) = 0.89999998 at k = 10 gives (1 - c) k = 1.0000002,
    ceil 2, where 0.9 means 1.  Values outside [0, 1] or non-finite: ValueError."""
    if not (isinstance(k, int) and not isinstance(k, bool) and k >= 1):
        raise ValueError(f"hold_map: k must be a positive step count, got {k!r}")
    c = torch.as_tensor(c)
    if c.dtype != torch.float32:
        raise ValueError(f"change_map must be fp32, got {c.dtype}")
    if c.numel() == 0 or not bool(torch.isfinite(c).all()) or float(c.min()) < 0.0 or float(c.max()) > 1.0:
        raise ValueError("change_map values must be finite and lie in [0, 1] (1 full strength, 0 keep)")
    c64 = c.double()
    held = torch.ceil((1.0 - c64) * k - k * 2.0 ** -24).clamp_(min=0.0)
    return torch.where(c64 == 0.0, torch.full_like(held, float(k + 1)), held).to(torch.float32)


def blur_map(ops, m, sigma):
    """m fp32 [n, 1, h, w] in [0, 1] on the device -> the same blurred by a Gaussian of `sigma` latent pixels (ops.blur_planes with ops.blur_taps, edges
    replicated, the result clamped to [0, 1]: the rounded weights do not sum to exactly 1).  sigma 0: m itself, nothing is launched."""
    if not (isinstance(sigma, (int, float)) and not isinstance(sigma, bool) and math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"mask_blur must be a finite number >= 0 (latent pixels), got {sigma!r}")
    if sigma == 0.0:
        return m
    require_op(ops, "blur_planes", ": mask_blur blurs the map on the device by that launch (ops.blur_planes)")
    m = m.to(F32).contiguous()
    return ops.blur_planes(m, torch.empty_like(m), torch.empty_like(m), ops.blur_taps(sigma).to(m.device), clamp01=True)


RESAMPLE = ("nearest", "bilinear", "bicubic")      # ops.resize_planes' modes 0, 1, 2 (PyTorch's nearest-exact / bilinear / bicubic, align_corners=False)


def hires_plan(size, scale=None, target=None, f=8):
    """The second-pass size of a hires render -> (W2, H2).  size = (W, H) of the first pass in pixels; exactly one of scale (a factor: each axis becomes
    round(axis * scale / f) * f) and target = (W2, H2), a multiple of f (the VAE's factor) on both axes.  The result must not be smaller than the base
    on any axis and must be larger on one."""
    if (scale is None) == (target is None):
        raise ValueError("a hires pass takes either a scale or a target size" + (", not both" if scale is not None else ""))
    W, H = (int(v) for v in size)
    if scale is not None:
        if not (isinstance(scale, (int, float)) and not isinstance(scale, bool) and scale > 0):
            raise ValueError(f"hires scale must be a positive number, got {scale!r}")
        W2, H2 = (int(round(v * scale / f)) * f for v in (W, H))
    else:
        W2, H2 = (int(v) for v in target)
        if W2 % f or H2 % f:
            raise ValueError(f"hires size must be a multiple of {f}, got {W2} x {H2}")
    if W2 < W or H2 < H or (W2, H2) == (W, H):
        raise ValueError(f"hires size {W2} x {H2} must be at least the base size {W} x {H} on both axes and larger on one")
    return W2, H2


def upscale_latents(ops, lat, H, W, mode="bilinear"):
    """lat fp32 [n, c, h, w] on the device -> [n, c, H, W], resampled by ops.resize_planes (mode: one of RESAMPLE).  The c planes of an image are the
    4 latent channels, or the 3 colours of a decoded picture."""
    if mode not in RESAMPLE:
        raise ValueError(f"resample must be one of {RESAMPLE}, got {mode!r}")
    require_op(ops, "resize_planes", ": the hires pass resamples on the device by that launch (ops.resize_planes)")
    lat = lat.to(F32).contiguous()
    out = torch.empty(lat.shape[0], lat.shape[1], H, W, dtype=F32, device=lat.device)
    return ops.resize_planes(lat, out, RESAMPLE.index(mode))


KV_MODES = ("nearest", "area")      # ops.token_pool's modes 0, 1


def kv_downsample_args(factors, mode="nearest"):
    """sample()'s / render()'s `kv_downsample`, checked -> None | (factors, mode).  factors: None, an int or a sequence of ints >= 1, the largest
    self-attention token grid first (UNet.set_kv_downsample); trailing ones are dropped, and nothing but ones is None: off.  mode "nearest" | "area"."""
    if mode not in KV_MODES:
        raise ValueError(f"kv_downsample_mode must be one of {KV_MODES}, got {mode!r}")
    if factors is None:
        return None
    fs = [factors] if isinstance(factors, int) else list(factors)
    if not all(isinstance(f, int) and not isinstance(f, bool) and f >= 1 for f in fs):
        raise ValueError(f"kv_downsample takes integer factors >= 1, largest token grid first, got {factors!r}")
    while fs and fs[-1] == 1:
        fs.pop()
    return (tuple(fs), mode) if fs else None


def freeu_args(freeu):
    """sample()'s / render()'s `freeu`, checked -> None | dict(b1, b2, s1, s2, version).  None; four numbers (b1, b2, s1, s2) - diffusers'
    enable_freeu order, version 1 - or a dict with those keys and optionally version (1: diffusers' constant backbone factor; 2: the authors' current
    code, FreeU_V2: the factor follows the normalised channel mean).  All four finite and positive."""
    if freeu is None:
        return None
    if isinstance(freeu, dict):
        unknown, missing = sorted(set(freeu) - {"b1", "b2", "s1", "s2", "version"}), [k for k in ("b1", "b2", "s1", "s2") if k not in freeu]
        if unknown or missing:
            raise ValueError(f"freeu: keys b1, b2, s1, s2 and optionally version; unknown {unknown}, missing {missing}")
        vals, version = [freeu[k] for k in ("b1", "b2", "s1", "s2")], freeu.get("version", 1)
    else:
        vals, version = list(freeu) if isinstance(freeu, (tuple, list)) else [freeu], 1
    ok = len(vals) == 4 and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0 for v in vals)
    if not ok or isinstance(version, bool) or version not in (1, 2):
        raise ValueError(f"freeu takes four finite positive numbers (b1, b2, s1, s2) and version 1 or 2, got {freeu!r}")
    return dict(b1=float(vals[0]), b2=float(vals[1]), s1=float(vals[2]), s2=float(vals[3]), version=int(version))


TilePlan = collections.namedtuple("TilePlan", "T O th tw ty tx")


def tile_plan(h, w, tile):
    """sample()'s / render()'s `tile` for an h x w latent, checked -> None | TilePlan(T, O, th, tw, ty, tx).  tile: None (off), T, or (T, O): windows of
    T x T latent units whose neighbours overlap by at least O (default T // 4; vae.tile_starts).  None as well where h <= T and w <= T: a pass that fits
    in one window is the plain path.  Otherwise ty x tx windows of th = min(h, T) by tw = min(w, T).  T >= 2 and 0 <= 2 O <= T, or ValueError."""
    if tile is None:
        return None
    ok_int = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
    if not (ok_int(tile) or (isinstance(tile, (tuple, list)) and len(tile) == 2 and all(ok_int(v) for v in tile))):
        raise ValueError(f"tile must be None, a window length or (window, overlap) in latent units, got {tile!r}")
    T, O = (tile, tile // 4) if ok_int(tile) else tile
    if T < 2 or O < 0 or 2 * O > T:
        raise ValueError(f"tiled diffusion needs a window length >= 2 and an overlap with 0 <= 2 * overlap <= window, got window={T} overlap={O}")
    if h < 1 or w < 1:
        raise ValueError(f"tile_plan: a {h} x {w} latent")
    if h <= T and w <= T:
        return None
    from .vae import tile_starts
    ty, tx = len(tile_starts(h, T, O)), len(tile_starts(w, T, O))
    if max(ty, tx) > 64:
        raise ValueError(f"tiled diffusion: {ty} x {tx} windows of {T} for a {h} x {w} latent (at most 64 per axis: a larger window)")
    return TilePlan(T, O, min(h, T), min(w, T), ty, tx)


def grid_multiple(cfg):
    """What both axes of a latent grid the UNet runs at must be a multiple of: every downsampler halves it, every upsampler doubles it back."""
    return 2 ** (len(cfg["block_out_channels"]) - 1)


def window_multiple(cfg, plan, name="tile"):
    """ValueError unless the windows of `plan` (a TilePlan, or None: no windows) obey grid_multiple on both axes; name: the argument the message speaks of."""
    m = grid_multiple(cfg) if plan is not None else 1
    if plan is not None and (plan.th % m or plan.tw % m):
        raise ValueError(f"{name}: a {plan.th} x {plan.tw} window is no multiple of {m} on both axes, which this UNet's downsampling needs"
                         + (" (the rule the latent size itself obeys without windows)" if name == "tile" else ""))


REGION_PLAN_MAX = 8        # regions of sample(regions=) with the background: the UNet batch is 2 n R (the kernels take 16)
REGION_KEYS = ("masks", "embeds", "base", "bootstrap", "bg")


def region_plan(h, w, masks, base=0.0):
    """The tables of regional prompts for an h x w latent -> ops.RegionTables(wn, wraw, R) on the CPU.  masks [R - 1, h, w] in [0, 1]: the foreground
    regions (None or empty: R = 1, the background alone); the background's raw weight is clamp(1 - sum of the foregrounds, 0, 1) + base, base >= 0 the
    main prompt's extra weight everywhere; wn = raw / sum over r, formed in fp64 and rounded once to fp32 - over r it sums to 1 at every pixel, and a
    pixel whose total raw weight is 0 cannot occur (asserted).  ValueError for masks outside [0, 1], a wrong shape, R > 8, or base < 0."""
    from . import ops as _ops
    if masks is not None and torch.is_tensor(masks) and masks.dim() == 3 and masks.shape[0] + 1 > REGION_PLAN_MAX:
        raise ValueError(f"regions: {masks.shape[0] + 1} regions with the background (at most {REGION_PLAN_MAX}: the UNet batch is 2 n R)")
    return _ops.region_tables(h, w, masks, base)


def region_args(regions, h, w, n, k):
    """sample()'s `regions`, checked -> None | dict(tabs, embeds, bootstrap, bg).  regions: None, or dict(masks=, embeds=, base=0.0, bootstrap=0,
    bg=None) - masks [R - 1, h, w] (region_plan), embeds one (c, uc[, pc, puc]) per foreground region per image (one image: the list of R - 1 tuples
    itself), bootstrap the number of steps that bootstrap (an int >= 0; at most the k that run count), bg fp32 [n, R, 4] or None: zeros.  No foreground
    mask (R = 1): None - the plain path."""
    if regions is None:
        return None
    unknown = sorted(set(regions) - set(REGION_KEYS))
    if unknown or "masks" not in regions or "embeds" not in regions:
        raise ValueError(f"regions: keys masks, embeds and optionally base, bootstrap, bg; unknown {unknown}")
    masks = regions["masks"]
    if masks is not None and not torch.is_tensor(masks):
        masks = torch.as_tensor(np.asarray(masks, dtype=np.float32))
    tabs = region_plan(h, w, masks, regions.get("base", 0.0))
    boot = regions.get("bootstrap", 0)
    if not (isinstance(boot, int) and not isinstance(boot, bool) and boot >= 0):
        raise ValueError(f"regions: bootstrap must be a step count >= 0, got {boot!r}")
    R = tabs.R
    em = regions["embeds"]
    em = [] if em is None else list(em)
    per_image = [em] if n == 1 and (not em or torch.is_tensor(em[0][0])) else [list(e) for e in em]
    if len(per_image) != n or any(len(e) != R - 1 for e in per_image):
        raise ValueError(f"regions: embeds must hold one (c, uc[, pc, puc]) per foreground region per image: {n} image(s) x {R - 1} region(s)")
    if R == 1:
        return None
    bg = regions.get("bg")
    if bg is None:
        bg = torch.zeros(n, R, 4, dtype=F32)
    bg = torch.as_tensor(bg)
    if tuple(bg.shape) != (n, R, 4) or not bool(torch.isfinite(bg).all()):
        raise ValueError(f"regions: bg {tuple(bg.shape)}: expected finite fp32 [{n}, {R}, 4], a background latent per image and region")
    return dict(tabs=tabs, embeds=per_image, bootstrap=min(boot, k), bg=bg.to(F32).contiguous())


def region_rtab(sched, k_boot):
    """The bootstrap table of ops.region_gather for a scheduler whose set_timesteps has run: fp32 [ops.REGION_TABLE_ROWS, 2], row i < k_boot
    (sigma_i, 1 / sqrt(sigma_i^2 + 1)) - step_table's factor: fp64 from the fp32 sigma, rounded once - every later row (-1, 0): no bootstrap."""
    from . import ops as _ops
    tab = np.zeros((_ops.REGION_TABLE_ROWS, 2), dtype=np.float32)
    tab[:, 0] = -1.0
    sig = np.asarray(sched.sigmas[:k_boot], dtype=np.float64)
    tab[:k_boot, 0], tab[:k_boot, 1] = sig, 1.0 / np.sqrt(sig ** 2 + 1.0)
    return torch.from_numpy(tab)


HEAT_GRIDS = ("max", "min")


def heatmap_args(heatmap, n, k=None):
    """sample()'s `heatmap`, checked -> None | dict(cols int32 [n, T, P], grid, weights fp32 [k]).  Keys: cols - integer [n, T] or [n, T, P]: the context
    positions (0 .. 76) whose score columns make map t of image i, -1: none (a map without any position is an absent token: it stays zero); grid "max"
    (default: the finest hooked resolution) | "min" (the coarsest: the reference's resize='min' map); weights None (the plain mean over the k steps that
    run) | one number per step that runs."""
    if heatmap is None:
        return None
    unknown = sorted(set(heatmap) - {"cols", "grid", "weights"})
    if unknown or "cols" not in heatmap:
        raise ValueError(f"heatmap: keys cols and optionally grid, weights; unknown {unknown}")
    cols = torch.as_tensor(heatmap["cols"])
    if cols.dim() == 2:
        cols = cols[:, :, None]
    if cols.dim() != 3 or cols.shape[0] != n or cols.shape[1] < 1 or cols.shape[2] < 1 or cols.is_floating_point():
        raise ValueError(f"heatmap cols: integer [{n}, T] or [{n}, T, P], got {tuple(cols.shape)} {cols.dtype}")
    if int(cols.max()) >= 77 or int(cols.min()) < -1:
        raise ValueError("heatmap cols: context positions 0 .. 76, or -1 for none")
    grid = heatmap.get("grid") or "max"
    if grid not in HEAT_GRIDS:
        raise ValueError(f"heatmap grid must be one of {HEAT_GRIDS}, got {grid!r}")
    weights = heatmap.get("weights")
    if k is not None:
        if weights is None:
            weights = [1.0 / k] * k
        weights = [float(v) for v in weights]
        if len(weights) != k or not all(math.isfinite(v) for v in weights):
            raise ValueError(f"heatmap weights: {len(weights)} value(s) for the {k} step(s) that run (one finite number each, or None)")
        weights = torch.tensor(weights, dtype=torch.float32)
    return dict(cols=cols.to(torch.int32).contiguous(), grid=grid, weights=weights)


def heat_entries(rt, h, w):
    """Runtime.daam_sums after a forward at latent size h x w -> [(sums fp32 [B h_r w_r, CTX_PAD], h_r, w_r, layer count)], finest resolution first."""
    out = []
    for N, ent in sorted(rt.daam_sums.items(), reverse=True):
        k = next((k for k in range(16) if (h >> k) * (w >> k) == N), None)
        if k is None or ent[1] < 1:
            raise ValueError(f"heatmap: {N} tokens per image is no level of a {h} x {w} latent")
        out.append((ent[0], h >> k, w >> k, ent[1]))
    if not 1 <= len(out) <= 4:
        raise ValueError(f"heatmap: {len(out)} hooked cross-attention resolution(s); the launch takes 1 .. 4")
    return out


def heat_grid(entries, grid):
    return entries[0][1:3] if grid == "max" else entries[-1][1:3]


def step_table_img(sched, guidance_scale):
    """step_table for ops.sampler_step_img, for a scheduler whose set_timesteps(n, start) has run: the rows of the k = n - start steps that run, and
    row 0 column 1 = the FIRST USED sigma (x = x0 + noise * sigma_0) instead of init_noise_sigma."""
    tab = step_table(sched, guidance_scale)
    tab[0, 1] = float(sched.sigmas[0])
    return tab


def step_table_ms(sched, guidance_scale):
    """The device table of ops.sampler_step_ms for a DpmSolverPP2M whose set_timesteps(n[, start]) has run: fp32 [2 + k, 8].  Columns 0..3 are
    step_table_img's (row 0 column 1 = the first USED sigma, which is init_noise_sigma when nothing is skipped); a step row continues with
    a_i, b_i, c_i, 0 - ms_coefficients in fp64 from the fp32 sigmas, rounded once.  c = 0.0f exactly on first-order rows."""
    return _step_table_wide(sched, guidance_scale, ms_coefficients(sched.sigmas))


def step_table_sde(sched, guidance_scale):
    """The device table of ops.sampler_step_sde for an EulerAncestral / DpmSolverPP2MSDE whose set_timesteps(n[, start]) has run: step_table_ms with
    sde_coefficients in columns 4..7 (column 7 = d, zero in step_table_ms: the 8-float row is unchanged), rounded once."""
    return _step_table_wide(sched, guidance_scale, sched.coeffs)


def _step_table_wide(sched, guidance_scale, coeffs):
    """step_table_img widened to 8-float rows: a step row continues with its row of `coeffs` (fp64 [k, 3 or 4]), rounded once; the rest stays zero."""
    base = step_table_img(sched, guidance_scale)
    tab = torch.zeros(base.shape[0], 8, dtype=torch.float32)
    tab[:, :4] = base
    tab[2:, 4:4 + coeffs.shape[1]] = torch.from_numpy(coeffs.astype(np.float32))
    return tab


def seed_words(seeds, n, generator=None, device="cpu"):
    """-> int32 [n, 2] on `device`: (lo, hi) 32-bit words of each image's 64-bit seed (ops.sampler_step_sde reads them as unsigned).  seeds: n Python
    ints, or None: drawn from `generator`."""
    if seeds is None:
        return torch.randint(-2 ** 31, 2 ** 31, (n, 2), generator=generator, device=device, dtype=torch.int64).to(torch.int32)
    seeds = list(seeds)
    if len(seeds) != n or not all(isinstance(v, int) and not isinstance(v, bool) for v in seeds):
        raise ValueError(f"seeds must be {n} int(s), one per image, got {seeds!r}")
    words = np.array([[v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF] for v in seeds], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32)).to(device)


# The four step launches of the fused / graph path, as data: the op (looked up on the op table when it is called), the builder of its device table,
# that table's key in the persistent state and its row width, whether the launch takes the history buffer and the seeds, the dict of LatentSampler that
# holds its captures, and what the capture key gains: None: nothing; a tuple: (the mask's presence,) + the tuple.
# form: None, or the `form` argument of ops.sampler_step_dd - the launch with a hold map (sample(change_map=)), one family per update it can take.
Family = collections.namedtuple("Family", "op table tab width dprev seeds graphs suffix form", defaults=(None,))
FAMILIES = dict(
    euler=Family("sampler_step", step_table, "table", 4, False, False, "_graphs", None),
    img=Family("sampler_step_img", step_table_img, "table", 4, False, False, "_img_graphs", ()),
    multistep=Family("sampler_step_ms", step_table_ms, "table_ms", 8, True, False, "_ms_graphs", ("multistep",)),
    sde=Family("sampler_step_sde", step_table_sde, "table_ms", 8, True, True, "_sde_graphs", ("sde",)),
    dd_euler=Family("sampler_step_dd", step_table_img, "table", 4, False, False, "_dd_graphs", ("dd", 0), 0),
    dd_ms=Family("sampler_step_dd", step_table_ms, "table_ms", 8, True, False, "_dd_graphs", ("dd", 1), 1),
    dd_sde=Family("sampler_step_dd", step_table_sde, "table_ms", 8, True, True, "_dd_graphs", ("dd", 2), 2),
)


def step_family(sampler, img, held=False):
    """The family of sample(sampler=...): img None: txt2img; held: with a change map."""
    if held:
        return "dd_sde" if sampler in SDE_KINDS else "dd_ms" if sampler == "dpmpp_2m" else "dd_euler"
    return "sde" if sampler in SDE_KINDS else "multistep" if sampler == "dpmpp_2m" else "euler" if img is None else "img"


class Trajectory(collections.namedtuple("Trajectory", "h w steps start sampler sigmas eta seeds guide guidance_scale img hold plan heat size family reg apg dyn", defaults=(None, None, None))):
    """sample()'s arguments, checked and resolved once; both drivers (the torch loop, the fused / graph path) take it.  h, w: the latent; steps: those that
    run, from entry `start` of the steps + start entries of the schedule; sampler, sigmas, eta, seeds: as given; guide: None, or guidance_table's
    (scale(s), rescale, interval) - the pre-pass runs; guidance_scale: the scalar of the step itself (1 with the pre-pass: e - e = 0 takes any); img: None
    or (x0, mask | None, start) (_img_args); hold: None or the change map's hold map; plan: None or the TilePlan; heat: None or heatmap_args' dict with
    its weights; size: (H, W) of SDXL's size conditioning; family: the step launch (FAMILIES); reg: None or region_args' dict (regional prompts); apg: None or apg_table's argument - the pre-pass
    is then ops.guidance_apg (guide is set with it); dyn: None or dyn_table's argument - the pre-pass is then ops.guidance_dyn (guide is set with it; never
    with apg)."""
    __slots__ = ()
    masked = property(lambda self: self.img is not None and self.img[1] is not None)


class LatentSampler:
    """`pipe(prompt_embeds=c, negative_prompt_embeds=uc, ..., num_inference_steps, guidance_scale, generator)` of the
    reference's render loop, up to the latents.  `unet` is an inference instance built for batch 2 (negative | positive, the
    order diffusers concatenates them in); its LoRA arena holds the trained adapters."""

    def __init__(self, rt, unet, prediction_type="epsilon", kv_downsample=None, kv_downsample_mode="nearest", n_images=None):
        """kv_downsample / kv_downsample_mode: the default of sample()'s keywords of the same names (kv_downsample_args).  n_images: the images sampled
        together where the runtime's batch is 2 n_images ty tx - a sampler for tiled diffusion (sample(tile=)) with ty tx windows per image; None:
        rt.B // 2, no windows."""
        self.kv_downsample = kv_downsample_args(kv_downsample, kv_downsample_mode)
        assert rt.B >= 2 and rt.B % 2 == 0, "classifier-free guidance runs the negative and the positive prompt of every image as one pair: an even batch"
        self.rt, self.unet = rt, unet
        self.n = rt.B // 2 if n_images is None else n_images      # images sampled together; image j = rows 2j (negative), 2j + 1 (positive)
        assert self.n >= 1 and rt.B % (2 * self.n) == 0, f"a batch of {rt.B} does not hold the pairs of {self.n} image(s) times a whole number of windows"
        self.tiles = rt.B // (2 * self.n)  # windows per image of the UNet batch (1: the UNet runs on the whole latent)
        self.sched = EulerDiscrete(prediction_type=prediction_type)
        self.sched_ms = DpmSolverPP2M(prediction_type=prediction_type)
        self.sched_sde = dict(euler_a=EulerAncestral(prediction_type=prediction_type), dpmpp_2m_sde=DpmSolverPP2MSDE(prediction_type=prediction_type))
        cfg = unet.cfg
        self.ctx = rt.zeros(rt.B * CTX_PAD, cfg["cross_dim"])
        self.pooled = rt.zeros(rt.B, cfg["proj_class_in"] - 6 * cfg["addition_time_embed_dim"]) if cfg["addition"] else None
        self._fused = None                 # persistent device state of both drivers (the torch loop, the fused / graph path), built on first use
        self._graphs = {}                  # (h, w, n, adapter scale in effect, DoRA) -> hipGraph of one denoising iteration
        self._img_graphs = {}              # the same key + (masked,) -> hipGraph of one iteration whose step launch is ops.sampler_step_img
        self._ms_graphs = {}               # the same key + (masked, "multistep") -> hipGraph of one iteration whose step launch is ops.sampler_step_ms
        self._sde_graphs = {}              # the same key + (masked, "sde") -> hipGraph of one iteration whose step launch is ops.sampler_step_sde
        self._dd_graphs = {}               # the same key + (False, "dd", form) -> hipGraph of one iteration whose step launch is ops.sampler_step_dd
        self._guided_graphs = {}           # any of the four keys above + (its family,) -> hipGraph of that iteration with ops.guidance before the step launch
        self._apg_graphs = {}              # the same + ("apg",) -> hipGraph of that iteration with ops.guidance_apg there instead: a dict of their own, so they evict no other
        self._dyn_graphs = {}              # the guided key + ("dyn",) -> hipGraph of that iteration with ops.guidance_dyn there instead: a dict of their own as well
        # the torch loop where the pre-pass runs: the deterministic samplers in their step kernels' order (dpmpp_2m: the SDE form's eta = 0 rows are
        # ms_coefficients with d = 0)
        self.sched_exact = dict(euler=EulerStepOrder(prediction_type=prediction_type), dpmpp_2m=DpmSolverPP2MSDE(prediction_type=prediction_type, eta=0.0))

    def _fwd_kw(self):
        """Keywords of the UNet forward: with key / value downsampling set it is declared an inference forward (UNet.forward refuses a training one);
        without, the call is the plain one."""
        return {} if getattr(self.unet, "_kv_ds", None) is None else {"train": False}

    def set_lora_scale(self, lora_scale, train_scale=None):
        """set_adapter_scales (checkpoint.py:31-55): every adapter's contribution is multiplied by lora_scale."""
        a = self.unet.arena
        if a is not None:
            if not hasattr(a, "_train_scale"):
                a._train_scale = a.scale if train_scale is None else train_scale
            a.set_scale(a._train_scale * lora_scale)      # (DoRA: the column factors follow the scale in effect)

    @torch.no_grad()
    def sample(self, embeds, h, w, *, steps=25, guidance_scale=8.0, generator=None, size=None, latents=None, graph=False, fused=False, n_images=1,
               init_latents=None, strength=1.0, mask=None, sampler="euler", sigmas="trailing", eta=1.0, seeds=None, guidance_rescale=0.0,
               guidance_interval=None, freeu=None, heatmap=None, kv_downsample=None, kv_downsample_mode=None, change_map=None, tile=None, regions=None, apg=None,
               dynthresh=None):
        """embeds = (c [1,77,D], uc [1,77,D], pc [1,P] | None, puc | None); h, w latent size.  Returns latents [1,4,h,w] fp32
        (still multiplied by the VAE scaling factor, as the pipeline holds them before `vae.decode(latents / scaling_factor)`).
        fused: guidance, the Euler update and the next model input are ONE kernel between two forwards (ops.sampler_step) instead of torch
        element-wise launches; graph: that iteration additionally replayed as a hipGraph (implies fused).  Both sample n_images images together
        on a runtime of batch 2 n_images: embeds is then a list of n_images 4-tuples and the result [n_images, 4, h, w].
        init_latents [n_images | 1, 4, h, w] (the encoded image times the scaling factor): img2img - the last min(int(steps * strength), steps) steps of
        the schedule, from init_latents noised to the first of them (`latents` / `generator` give the noise, as above).  mask [n_images | 1, 1, h, w] in
        [0, 1]: 1 regenerate, 0 keep - the kept region is re-injected after every step and equals init_latents exactly at the end.  strength 1 without a
        mask is txt2img from the noise; a mask of ones is no mask.
        sampler: "euler" | "dpmpp_2m" (DpmSolverPP2M: second-order multistep; fused / graph: the step launch is ops.sampler_step_ms); sigmas: "trailing" |
        "karras" (EulerDiscrete.set_timesteps), with either sampler.
        sampler "euler_a" | "dpmpp_2m_sde" (EulerAncestral, DpmSolverPP2MSDE): fresh noise after every step, its amount set by eta >= 0 (0: the
        deterministic limit), drawn on the device from one 64-bit seed per image - seeds: n_images ints, None: drawn from `generator` after the initial
        latents - the step index and the pixel, so an image's noise does not depend on the batch it is sampled in.  The torch loop takes it from
        ops.sampler_noise, fused / graph make it inside ops.sampler_step_sde: the three paths give the same bits.
        guidance_scale: a number, or one per step that runs; guidance_interval (sigma_lo, sigma_hi): guidance only at the steps whose sigma_i lies
        in (sigma_lo, sigma_hi] (g_i = 1 elsewhere - both rows of a pair still go through the UNet there: the picture changes, the time does not);
        guidance_rescale phi in [0, 1]: the guided prediction rescaled to the positive one's standard deviation and blended with weight phi, on the
        steps with g_i != 1 (guidance_table).  With any of the three in use, ops.guidance forms the prediction on the device between the forward and
        the step launch - in the torch loop too, whose update is then taken in the step kernel's order: the three paths give the same bits.  A
        scalar guidance_scale without the other two launches nothing new.
        freeu: None, or (b1, b2, s1, s2) / dict(b1, b2, s1, s2, version=1): FreeU (freeu_args; UNet.set_freeu) in every forward of the trajectory - one
        ops.freeu call in front of each resnet of the first two up-blocks, on all three paths, with every sampler, init latents and mask.  The values are
        launch arguments, so the graph path keeps one capture per setting.
        heatmap: None, or dict(cols, grid="max", weights=None) (heatmap_args): per-token cross-attention heat maps.  After every forward one launch
        (ops.heatmap_accum) adds the step's weight times the layer mean of the hooked cross-attentions' raw scores Q K^T / sqrt(d) - the positive row
        of each image, the columns `cols` name, every resolution resampled to the grid - into fp32 maps [n_images, T, gh, gw]; the latents are the
        same bits with and without.  The result is then (latents, maps).  On all three paths; columns and weights are device memory, so the graph
        path keeps one capture per (grid, T, P).
        kv_downsample: a tuple of integer factors, largest self-attention token grid first - (2,), (4, 2) - with kv_downsample_mode "nearest" | "area":
        key / value token downsampling (UNet.set_kv_downsample: one ops.token_pool launch per affected self-attention, whose k | v products and score
        work shrink by factor^2) in every forward of the trajectory, on all three paths.  None: the constructor's setting; () or all ones: off, and
        the launch sequence is the plain one.  The setting is part of the capture key.
        change_map [n_images | 1, 1, h, w] fp32 in [0, 1] (needs init_latents; excludes mask): differential diffusion - 1 gives a pixel the whole
        `strength`, 0 keeps it as init_latents exactly, a value between holds it on the init latents' noised trajectory for the first (1 - c) share of
        the steps that run and then releases it (hold_map): a SELECT after every step, never a mix.  With every sampler on all three paths; fused /
        graph: the step launch is ops.sampler_step_dd, whose captures are keyed apart from all others, and the hold map lives in a persistent buffer
        refilled per call, so one capture serves every map, strength and step count.  A map of ones gives the bits of the call without it at
        strength < 1; at strength 1 the trajectory starts from init_latents + noise * sigma_0 (without a map: from the noise alone).
        tile: None, T or (T, O) in latent units (tile_plan; O defaults to T // 4): tiled diffusion (MultiDiffusion, Bar-Tal et al. 2023).  Where the
        latent exceeds T on an axis the UNet runs on ty x tx overlapping windows of min(h, T) x min(w, T) as ONE batch of 2 n_images ty tx rows - the
        sampler is built on a runtime of that batch (LatentSampler(n_images=)) - between two launches: ops.window_gather cuts the windows out of the
        model input, ops.window_blend fuses their predictions with normalised feather weights into one prediction for the whole latent.  Guidance, the
        step launch, init latents, mask, change map and the per-step noise stay at full size and unchanged: every step is affine in the prediction, so
        stepping once on the fused prediction equals stepping every window and averaging.  Every window row of an image carries that image's
        conditioning (SDXL: the whole picture's size).  On all three paths, with every sampler; freeu and kv_downsample act per window.  Starts and
        weights are device memory: one capture per (shape, window counts) serves every overlap.  A latent that fits one window (h <= T and w <= T) is the
        plain path: the same launches and bits as without `tile`.  Not with heatmap (the hooked score sums are per window).
        regions: None, or dict(masks=, embeds=, base=0.0, bootstrap=0, bg=None) (region_args): regional prompts (MultiDiffusion section 4.2).  masks
        [R - 1, h, w] in [0, 1] are the foreground regions, embeds one (c, uc[, pc, puc]) per foreground region per image; the call's own `embeds` is
        region 0, the background.  The UNet runs the whole latent once per region as ONE batch of 2 n_images R rows - the sampler is built on a
        runtime of that batch (LatentSampler(n_images=)) - between two launches: ops.region_gather copies the model input to every region's rows,
        ops.region_blend fuses their predictions with the normalised per-pixel weights (region_plan; base: the main prompt's extra weight
        everywhere).  Batch row 2 (j R + r) + 1 carries region r's positive conditioning, every even row the call's negative one; SDXL's size
        conditioning stays the whole picture's.  bootstrap = k: at the first min(k, steps that run) steps a foreground region's model input is
        replaced, outside its mask (raw weight < 0.5), by a constant background bg [n_images, R, 4] (None: zeros) noised to the step's level - made
        inside the gather launch from the image's seed (`seeds`, as the stochastic samplers; None: drawn from `generator`), the step, the region and
        the pixel - so that the region's object forms inside its mask.  Guidance, the step launch, init latents, mask, change map and the per-step
        noise stay at full size and unchanged; freeu and kv_downsample act per row.  On all three paths, with every sampler.  Masks, weights, bg and
        the bootstrap length are device memory: one capture per (shape, R) serves all of them.  No foreground mask (R = 1) is the plain path: the
        same launches, bits and capture key as without `regions`.  Not with tile or heatmap.
        apg: None, or (eta, norm_threshold, momentum) - numbers, or one tuple per step that runs (apg_table): adaptive projected guidance.  The
        pre-pass is then ops.guidance_apg where it would be ops.guidance - with apg alone too: it counts as guidance in use - on all three paths, with
        every sampler, init latents, mask, change map, and with tile / regions on the fused full-size prediction; guidance_scale, guidance_interval
        and guidance_rescale act as before (g_i = 1 steps pass e_pos through and leave the running average alone).  The three values per step are
        device memory and the running average is a persistent buffer per shape that the launch restarts at step row 0 by itself: one capture (in a
        dict of its own, the key ending in "apg") serves every setting and every picture.  apg=None is the path without it: the same launches,
        capture keys and bits.  The neutral values (1, 0, 0) are still the new launch: e_pos + (g - 1) d equals classifier-free guidance's
        e_neg + g d mathematically, not bit for bit.
        dynthresh: None, or (mimic, percentile, interpolate) - numbers, or one tuple per step that runs (dyn_table): dynamic thresholding.  The
        pre-pass is then ops.guidance_dyn where it would be ops.guidance - with dynthresh alone too: it counts as guidance in use - on all three
        paths, with every sampler, per-step guidance scales, guidance_interval (g_i = 1 steps pass e_pos through), init latents, mask, change map,
        and with tile / regions on the fused full-size prediction.  The three values per step are device memory: one capture (in a dict of its own,
        the guided key plus "dyn") serves every setting.  dynthresh=None is the path without it: the same launches, capture keys and bits.  Not with
        guidance_rescale > 0 and not with apg (ValueError): the three are alternative answers to the same fault."""
        ops = self.rt.ops
        if regions is not None and (tile is not None or heatmap is not None):      # refused before anything is built
            raise ValueError("regions do not combine with " + ("tile: windows of regions are not built" if tile is not None else
                                                               "heatmap: the hooked score sums are per region row, and fusing them is not built"))
        plan = tile_plan(h, w, tile)                        # refused before anything is built
        if plan is not None:
            if heatmap is not None:
                raise ValueError("heatmap does not combine with tile: the hooked score sums are per window, and stitching them is not built")
            window_multiple(self.unet.cfg, plan)
            for op in ("window_blend", "window_gather"):
                require_op(ops, op, " (sdlt_window_blend): sample(tile=...) cuts and fuses the windows by two launches (ops.window_gather, "
                           "ops.window_blend), in the torch loop too", kernel="window_blend")
        reg = None
        if regions is not None:                            # (the step count of the bootstrap is cut to the steps that run below)
            reg = region_args(regions, h, w, n_images, TABLE_ROWS)
        if reg is not None:
            for op in ("region_blend", "region_gather"):
                require_op(ops, op, " (sdlt_region_blend): sample(regions=...) copies the model input to the regions' rows and fuses their predictions "
                           "by two launches (ops.region_gather, ops.region_blend), in the torch loop too", kernel="region_blend")
        rows = reg["tabs"].R if reg is not None else 1 if plan is None else plan.ty * plan.tx
        if rows != self.tiles:
            raise ValueError(f"this sampler's runtime holds {self.tiles} window(s) per image (batch {self.rt.B}, {self.n} image(s)); the call needs "
                             f"{rows}: build it on a runtime of batch 2 n_images ty tx (LatentSampler(n_images=))")
        if change_map is not None:                         # refused before anything is built
            if init_latents is None:
                raise ValueError("change_map needs init_latents: a held pixel follows their noised trajectory")
            if mask is not None:
                raise ValueError("change_map and mask exclude each other: the map selects per pixel and step, the mask blends after every step")
            if graph or fused:
                require_op(ops, "sampler_step_dd", ": sample(change_map=..., graph=False, fused=False) is the torch loop")
        kd = self.kv_downsample
        if kv_downsample is not None or kv_downsample_mode is not None:
            kd = kv_downsample_args(kd[0] if kv_downsample is None and kd is not None else kv_downsample, kv_downsample_mode or (kd[1] if kd is not None else "nearest"))
        if kd != getattr(self.unet, "_kv_ds", None):
            self.unet.set_kv_downsample(*(kd or (None,)))      # (an op table without the kernel raises NotImplementedError here)
        fz = freeu_args(freeu)
        if fz is not None or getattr(self.unet, "_freeu", None) is not None:
            self.unet.set_freeu(fz)          # (None: the plain launch sequence; an op table without the kernel raises NotImplementedError here)
        eta = sampler_args(sampler, sigmas, eta)
        img = self._img_args(init_latents, strength, mask, steps, h, w, n_images, keep=change_map is not None)
        start = 0 if img is None else img[2]
        hold = None if change_map is None else self._hold_args(change_map, steps - start, h, w, n_images)
        hm = heatmap_args(heatmap, n_images, steps - start)      # (the weights: one per step that runs)
        if hm is not None:
            require_op(ops, "heatmap_accum", ": the heat maps are accumulated by that launch (ops.heatmap_accum), in the torch loop too")
        if dynthresh is not None and (apg is not None or guidance_rescale):      # refused before anything is built
            raise ValueError("dynthresh does not combine with " + ("apg" if apg is not None else "guidance_rescale") + ": they are alternative answers to the "
                             "burnt contrast of a strong guidance scale")
        guide = (guidance_scale, guidance_rescale, guidance_interval) if apg is not None or dynthresh is not None or guidance_in_use(guidance_scale, guidance_rescale, guidance_interval) else None
        if apg is not None:
            apg_table(None, apg, steps - start)            # refused before anything is built
            require_op(ops, "guidance_apg", " (sdlt_guidance_apg): sample(apg=...) forms the projected prediction by that launch (ops.guidance_apg), in "
                       "the torch loop too", kernel="sdlt_guidance_apg")
        elif dynthresh is not None:
            dyn_table(None, dynthresh, steps - start)      # refused before anything is built
            require_op(ops, "guidance_dyn", " (sdlt_guidance_dyn): sample(dynthresh=...) forms the thresholded prediction by that launch (ops.guidance_dyn), in "
                       "the torch loop too", kernel="sdlt_guidance_dyn")
        elif guide is not None:
            require_op(ops, "guidance", ": a per-step guidance_scale, guidance_rescale and guidance_interval are evaluated by that launch (ops.guidance), "
                       "in the torch loop too")
        assert 1 <= steps <= TABLE_ROWS - 2
        traj = Trajectory(h, w, steps - start, start, sampler, sigmas, eta, seeds, guide, guidance_scale if guide is None else 1.0, img, hold, plan, hm,
                          size if size is not None else (8 * h, 8 * w), step_family(sampler, img, hold is not None),
                          None if reg is None else dict(reg, bootstrap=min(reg["bootstrap"], steps - start)), apg, dynthresh)
        if graph or fused:
            if traj.family == "sde":
                require_op(ops, "sampler_step_sde", f": sample(sampler={sampler!r}) draws its per-step noise inside that launch")
            if traj.family == "multistep":
                require_op(ops, "sampler_step_ms", ": sample(sampler='dpmpp_2m', graph=False, fused=False) is the torch loop")
            require_op(ops, "sampler_step", ": sample(graph=False, fused=False) is the torch loop")
            if img is not None and hold is None:
                require_op(ops, "sampler_step_img", ": sample(init_latents=..., graph=False, fused=False) is the torch loop")
            assert n_images == self.n, f"the runtime's batch {self.rt.B} samples {self.n} image(s) together, not {n_images}"
            return self._sample_fused(traj, embeds, latents, generator, graph)
        assert n_images == 1 and self.n == 1, "the torch loop samples one image on a batch-2 runtime; several images together: fused=True or graph=True"
        if sampler in SDE_KINDS:
            require_op(ops, "sampler_noise", f": sample(sampler={sampler!r}) takes its per-step noise from that kernel's generator (ops.sampler_noise), "
                       "in the torch loop too", kernel="sampler_step_sde")
        return self._sample_torch(traj, embeds, latents, generator)

    def _sample_torch(self, traj, embeds, latents, generator):
        """The torch loop: the setup and the forward stage of the fused path (_begin, _predict) on the same persistent state, then the scheduler's step,
        the mask's blend or the hold map's select and the next model input as torch operations; the step index is written from the host."""
        rt, h, w = self.rt, traj.h, traj.w
        s = self._scheduler(traj, exact=traj.guide is not None)
        st, sh, x0, noise, heat = self._begin(traj, s, embeds, latents, generator)
        x = noise * s.init_noise_sigma if traj.img is None else x0 + noise * float(s.sigmas[0])
        m, hold = sh["img"]["mask"] if traj.masked else None, None if traj.hold is None else sh["img"]["hold"]
        sde, counted = traj.sampler in SDE_KINDS, heat is not None or traj.guide is not None or traj.reg is not None      # (the gather reads the bootstrap's row)
        if sde:
            z = rt.zeros(1, 4, h, w, dtype=F32)
        if heat is not None and heat["heat"] is not None:
            heat["heat"].zero_()
        for i, t in enumerate(s.timesteps):
            xin = s.scale_model_input(x, i)
            sh["x64"][:, :4] = xin.permute(0, 2, 3, 1).reshape(h * w, 4).repeat(2, 1).to(sh["x64"].dtype)
            st["tf"].fill_(float(t))
            if counted:                            # the heat maps' weight and the pre-pass's row are read at a device counter, as in the fused path
                st["ctr"][0] = i
            eps = self._predict(st, sh, traj, heat).view(2, h, w, 4).permute(0, 3, 1, 2)
            e = eps[1:2] if traj.guide is not None else eps[0:1] + traj.guidance_scale * (eps[1:2] - eps[0:1])      # (the pre-pass: both rows hold the prediction)
            if sde:                                # the kernel's own noise of step i (not drawn where the row adds none)
                x = s.step(e, i, x, rt.ops.sampler_noise(st["seeds"], i, z) if s.coeffs[i, 3] != 0.0 else None)
            else:
                x = s.step(e, i, x)
            if m is not None or hold is not None:
                k = x0 + noise * float(s.sigmas[i + 1])      # the known region, noised to the sigma this step arrived at (0 after the last: init_latents itself)
                # the mask blends it in; differential diffusion selects it while the pixel is held (step row i: i + 1 < hold)
                x = k + m * (x - k) if m is not None else torch.where(hold > float(i + 1), k, x)
        return x if heat is None else (x, heat["heat"].clone())

    def _scheduler(self, traj, exact=False):
        """The scheduler of a trajectory, its timesteps set.  exact (the torch loop where the guidance pre-pass runs): the deterministic samplers in
        their step kernels' order."""
        if traj.sampler in SDE_KINDS:
            s = self.sched_sde[traj.sampler]
            s.eta = traj.eta
        elif exact:
            s = self.sched_exact[traj.sampler]
        else:
            s = self.sched_ms if traj.sampler == "dpmpp_2m" else self.sched
        return s.set_timesteps(traj.steps + traj.start, traj.start, traj.sigmas)

    def _hold_args(self, change_map, k, h, w, n):
        """-> hold_map of sample()'s change_map for the k steps that run, fp32 [n, 1, h, w] on the device."""
        if not torch.is_tensor(change_map) or change_map.dim() != 4 or tuple(change_map.shape[1:]) != (1, h, w) or change_map.shape[0] not in (1, n):
            raise ValueError(f"change_map {tuple(getattr(change_map, 'shape', ()))}: expected a tensor [{n} or 1, 1, {h}, {w}]")
        return hold_map(change_map.to(self.rt.device), k).expand(n, 1, h, w).contiguous()

    def _img_args(self, init_latents, strength, mask, steps, h, w, n, keep=False):
        """-> None (txt2img: no init_latents, or strength 1 without a mask) | (x0 [n, 4, h, w], mask [n, 1, h, w] | None, first step) on the device.
        keep (a change map follows): never None from init latents."""
        if init_latents is None:
            if mask is not None:
                raise ValueError("mask needs init_latents: the region to keep is taken from them")
            if strength != 1.0:
                raise ValueError("strength needs init_latents")
            return None
        _, start = img2img_steps(steps, strength)
        dev = self.rt.device
        if init_latents.dim() != 4 or tuple(init_latents.shape[1:]) != (4, h, w) or init_latents.shape[0] not in (1, n):
            raise ValueError(f"init_latents {tuple(init_latents.shape)}: expected [{n} or 1, 4, {h}, {w}]")
        x0 = init_latents.to(dev, F32).expand(n, 4, h, w).contiguous()
        if mask is not None:
            if mask.dim() != 4 or tuple(mask.shape[1:]) != (1, h, w) or mask.shape[0] not in (1, n):
                raise ValueError(f"mask {tuple(mask.shape)}: expected [{n} or 1, 1, {h}, {w}]")
            mask = mask.to(dev, F32)
            lo, hi = float(mask.min()), float(mask.max())
            if not (lo >= 0.0 and hi <= 1.0):
                raise ValueError(f"mask values must lie in [0, 1] (1 regenerate, 0 keep), got [{lo}, {hi}]")
            # ones everywhere: nothing to keep.  (k + 1 (x - k) rounds twice where the plain step does not, so it is not left to the blend.)
            mask = None if lo == 1.0 else mask.expand(n, 1, h, w).contiguous()
        if mask is None and start == 0 and not keep:
            return None
        return x0, mask, start

    # ---- the persistent state, setup and forward stage of both drivers; the fused / graph path ---------------------------------
    def _scope(self):
        """This sampler's own split-K / norm scratch (ops.workspace_owner), as the training step keeps its own: a captured launch holds the pointers."""
        own = getattr(self.rt.ops, "workspace_owner", None)
        if own is None:
            import contextlib
            return contextlib.nullcontext()
        return own(id(self))

    def _state(self, h, w, plan=None, reg=None):
        """plan (a TilePlan): the shape's state is keyed by the window extents and counts as well, and holds the windows' buffers (_window_state); reg
        (region_args' dict): by the region count, and holds the regions' buffers (_region_state)."""
        rt, n = self.rt, self.n
        if self._fused is None:      # (tid: one row of six per UNET batch row - 2 n without windows)
            self._fused = dict(tf=rt.zeros(2 * n, dtype=F32), tid=rt.zeros(rt.B * 6, dtype=F32), table=rt.zeros(TABLE_ROWS, 4, dtype=F32),
                               ctr=torch.zeros(2, dtype=torch.int32, device=rt.device), shapes={})
        st = self._fused
        key = (h, w, "region", reg["tabs"].R) if reg is not None else (h, w) if plan is None else (h, w) + tuple(plan[2:])
        if key not in st["shapes"]:
            st["shapes"][key] = dict(x=rt.zeros(n, 4, h, w, dtype=F32), x64=rt.zeros(2 * n * h * w, 64))
        if plan is not None:
            self._window_state(st["shapes"][key], h, w, plan)
        if reg is not None:
            self._region_state(st["shapes"][key], h, w, reg)
        return st, st["shapes"][key]

    def _region_state(self, sh, h, w, reg):
        """-> sh["reg"]: the persistent buffers of regional prompts for this shape - the regions' model input x64_regions and timesteps tf_regions, the
        fused prediction eps_full fp32 [2 n h w, 4], the tables wn and wraw, the backgrounds bg and the bootstrap table rtab - allocated once (a
        captured launch holds their pointers); weights, masks and backgrounds are rewritten per call (rtab: by _begin, which knows the schedule):
        another mask set with the same region count is the same buffers and the same capture."""
        rt, n, fresh = self.rt, self.n, reg["tabs"]
        rs = sh.get("reg")
        if rs is None:
            from . import ops as _ops
            tabs = fresh._replace(wn=torch.zeros_like(fresh.wn, device=rt.device), wraw=torch.zeros_like(fresh.wraw, device=rt.device))
            rs = sh["reg"] = dict(tabs=tabs, x64_regions=rt.zeros(rt.B * h * w, 64), tf_regions=rt.zeros(rt.B, dtype=F32),
                                  eps_full=rt.zeros(2 * n * h * w, 4, dtype=F32), bg=rt.zeros(n, fresh.R, 4, dtype=F32),
                                  rtab=rt.zeros(_ops.REGION_TABLE_ROWS, 2, dtype=F32))
        rs["tabs"].wn.copy_(fresh.wn)
        rs["tabs"].wraw.copy_(fresh.wraw)
        rs["bg"].copy_(reg["bg"])
        return rs

    def _region_forward(self, rs, st, x64, tf, tid, h, w):
        """The forward of regional prompts: copy the model input to every region's rows (bootstrap: with the background outside a foreground's mask),
        run the UNet on them as one batch, fuse the predictions -> eps fp32 [2 n h w, 4], the prediction for the whole latent."""
        rt = self.rt
        boot = dict(bg=rs["bg"], rtab=rs["rtab"], ctr=st["ctr"], seeds=st["seeds"])
        rt.ops.region_gather(rs["tabs"], x64, rs["x64_regions"], tf, rs["tf_regions"], n=self.n, H=h, W=w, boot=boot)
        e = self.unet.forward(rs["x64_regions"], rs["tf_regions"], self.ctx, self.pooled, tid, B=rt.B, H=h, W=w, **self._fwd_kw())
        return rt.ops.region_blend(rs["tabs"], e, rs["eps_full"], n=self.n, H=h, W=w)

    def _window_state(self, sh, h, w, plan):
        """-> sh["win"]: the persistent buffers of tiled diffusion for this shape - the windows' model input x64_tiles and timesteps tf_tiles, the fused
        prediction eps_full fp32 [2 n h w, 4], and the tables (ops.window_tables) - allocated once (a captured launch holds their pointers); starts and
        weights are rewritten per call: another overlap with the same window counts is the same buffers and the same capture."""
        rt, n, ops = self.rt, self.n, self.rt.ops
        fresh = ops.window_tables(h, w, plan.T, plan.O)
        assert (fresh.th, fresh.tw, fresh.ty, fresh.tx) == tuple(plan[2:])
        win = sh.get("win")
        if win is None:
            tabs = fresh._replace(**{k: torch.zeros_like(getattr(fresh, k), device=rt.device) for k in ("ys", "xs", "wy", "wx")})
            win = sh["win"] = dict(plan=plan, tabs=tabs, x64_tiles=rt.zeros(rt.B * plan.th * plan.tw, 64), tf_tiles=rt.zeros(rt.B, dtype=F32),
                                   eps_full=rt.zeros(2 * n * h * w, 4, dtype=F32))
        for k in ("ys", "xs", "wy", "wx"):
            getattr(win["tabs"], k).copy_(getattr(fresh, k))
        win["plan"] = plan
        return win

    def _window_forward(self, win, x64, tf, tid, h, w):
        """The forward of tiled diffusion: cut the windows out of the model input, run the UNet on them as one batch, fuse their predictions ->
        eps fp32 [2 n h w, 4], the prediction for the whole latent (what the forward returns without windows)."""
        rt, plan = self.rt, win["plan"]
        rt.ops.window_gather(win["tabs"], x64, win["x64_tiles"], tf, win["tf_tiles"], n=self.n, H=h, W=w)
        e = self.unet.forward(win["x64_tiles"], win["tf_tiles"], self.ctx, self.pooled, tid, B=rt.B, H=plan.th, W=plan.tw, **self._fwd_kw())
        return rt.ops.window_blend(win["tabs"], e, win["eps_full"], n=self.n, H=h, W=w)

    def _load_conditioning(self, st, embeds, size, reg=None):
        """embeds: one (c, uc[, pc, puc]) per image (one image: the tuple itself) -> ctx, pooled and SDXL's size conditioning st["tid"].  UNet batch rows
        2 j tl .. 2 (j + 1) tl - 1 are image j's, (negative, positive) per window: every window row carries the image's conditioning.  reg (regional
        prompts: tl = R): row 2 (j R + r) + 1 then takes region r's positive context and pooled vector for r >= 1; every even row keeps the call's
        negative ones."""
        rt, cfg, n, tl = self.rt, self.unet.cfg, self.n, self.tiles
        per_image = [embeds] if (n == 1 and not isinstance(embeds[0], (tuple, list))) else list(embeds)
        assert len(per_image) == n, "one (c, uc[, pc, puc]) per image"
        cv = self.ctx.view(n, tl, 2, CTX_PAD, -1)
        for j, e in enumerate(per_image):
            c, uc, pc, puc = (tuple(e) + (None, None))[:4]
            cv[j, :, 0, :77].copy_(uc[0])
            cv[j, :, 1, :77].copy_(c[0])
            if cfg["addition"]:
                pv = self.pooled.view(n, tl, 2, -1)
                pv[j, :, 0].copy_(puc[0])
                pv[j, :, 1].copy_(pc[0])
            for r, er in enumerate(reg["embeds"][j] if reg is not None else (), start=1):
                cr, _, pcr, _ = (tuple(er) + (None, None))[:4]
                cv[j, r, 1, :77].copy_(cr[0])
                if cfg["addition"]:
                    pv[j, r, 1].copy_(pcr[0])
        if cfg["addition"]:
            H, W = size
            st["tid"].copy_(torch.tensor([float(H), float(W), 0.0, 0.0, float(H), float(W)] * rt.B))      # original_size, crop, target_size

    def _begin(self, traj, sch, embeds, latents, generator):
        """A trajectory starts, on either driver: the conditioning, the guidance table, the initial noise (`latents`, or drawn from `generator`), the seed
        words - drawn after it - the init latents, mask and hold map, and the heat maps' columns and weights go into the persistent state of the shape
        (_state: a captured launch holds its pointers; the window tables are refilled there).  Only ops the trajectory uses are touched.
        -> (st, sh, x0 | None, noise, heat | None): x0 and noise as the init launch takes them, heat the dict of sh["heat"] for these columns."""
        rt, n, h, w = self.rt, self.n, traj.h, traj.w
        dev = rt.device
        st, sh = self._state(h, w, traj.plan, traj.reg)
        self._load_conditioning(st, embeds, traj.size, traj.reg)
        if traj.reg is not None:                          # the bootstrap's rows of the steps that run; a captured gather holds the buffer
            sh["reg"]["rtab"].copy_(region_rtab(sch, traj.reg["bootstrap"]))
        if traj.guide is not None:                        # a persistent buffer, rewritten per trajectory: a captured pre-pass holds its pointer
            gtab = guidance_table(sch, *traj.guide)
            if "gtab" not in st:
                st["gtab"] = rt.zeros(TABLE_ROWS - 1, 4, dtype=F32)
            st["gtab"][: gtab.shape[0]].copy_(gtab)
        if traj.apg is not None:                          # the table beside gtab, rewritten per trajectory; the running average of the shape's full-size prediction,
            atab = apg_table(sch, traj.apg, traj.steps)   # which the launch restarts at step row 0 itself: nothing to clear here
            if "atab" not in st:
                st["atab"] = rt.zeros(TABLE_ROWS - 1, 4, dtype=F32)
            st["atab"][: atab.shape[0]].copy_(atab)
            if "mom" not in sh:
                sh["mom"] = rt.zeros(n * h * w, 4, dtype=F32)
        if traj.dyn is not None:                          # the table beside gtab, rewritten per trajectory
            dtab = dyn_table(sch, traj.dyn, traj.steps)
            if "dtab" not in st:
                st["dtab"] = rt.zeros(TABLE_ROWS - 1, 4, dtype=F32)
            st["dtab"][: dtab.shape[0]].copy_(dtab)
        noise = latents if latents is not None else torch.randn(n, 4, h, w, generator=generator, device=dev, dtype=F32)
        noise = noise.to(dev, F32).contiguous()
        assert tuple(noise.shape) == (n, 4, h, w)
        if traj.sampler in SDE_KINDS or traj.reg is not None:      # after the initial latents; a captured launch holds the buffer (regions: the bootstrap's key)
            if "seeds" not in st:
                st["seeds"] = torch.zeros(n, 2, dtype=torch.int32, device=dev)
            st["seeds"].copy_(seed_words(traj.seeds, n, generator, dev))
        x0 = None
        if traj.img is not None:                          # init latents, noise, mask and hold map: persistent too; the init launch takes the copies
            im = sh.setdefault("img", {})
            for k, v in (("x0", traj.img[0]), ("noise", noise), ("mask", traj.img[1]), ("hold", traj.hold)):
                if v is not None:
                    if k not in im:
                        im[k] = torch.zeros_like(v)
                    im[k].copy_(v)
            x0, noise = im["x0"], im["noise"]
        heat = None
        if traj.heat is not None:                         # persistent buffers, rewritten per trajectory: a captured launch holds their pointers
            hm = traj.heat
            if "hw" not in st:
                st["hw"] = rt.zeros(TABLE_ROWS, dtype=F32)
            st["hw"][: traj.steps].copy_(hm["weights"])
            hkey = (hm["grid"],) + tuple(hm["cols"].shape[1:])
            heat = sh.setdefault("heat", {}).setdefault(hkey, dict(grid=hm["grid"], cols=torch.zeros_like(hm["cols"], device=dev), heat=None))
            heat["cols"].copy_(hm["cols"])
        return st, sh, x0, noise, heat

    def _step_launch(self, fam, st, sh, eps, x0=None, noise=None, mask=None):
        """The launch of family `fam` (FAMILIES) on the persistent state; eps None: its init entry."""
        f, init = FAMILIES[fam], eps is None
        kw = dict(x0=x0, noise=noise, mask=mask, init=init) if fam != "euler" else dict(noise=noise) if init else {}
        if f.form is not None:                            # the launch with a hold map: no mask; the map is read by a step only
            kw = dict(x0=x0, noise=noise, hold=sh["img"]["hold"], form=f.form, init=init)
        if f.dprev:
            kw["dprev"] = sh["dprev"]
        if f.seeds:
            kw["seeds"] = st["seeds"]
        getattr(self.rt.ops, f.op)(eps, sh["x"], sh["x64"], st["tf"], st[f.tab], st["ctr"], **kw)

    def _predict(self, st, sh, traj, heat):
        """The forward stage of one iteration, on either driver: the UNet on sh["x64"] at st["tf"] - with a tile plan: gather, the forward on the windows,
        blend; with regions: gather, the forward on every region's rows, blend - then ops.heatmap_accum on the forward's score sums (heat, a dict of sh["heat"]: the weight of row ctr[0] of st["hw"]; the maps are
        allocated at the first iteration, when the forward has told the resolutions), then ops.guidance (row ctr[0] of st["gtab"]) where the pre-pass
        runs - with apg: ops.guidance_apg (the same row of st["atab"] as well, the running average in sh["mom"]); with dyn: ops.guidance_dyn (the same row of
        st["dtab"] as well) -> eps fp32 [2 n h w, 4]."""
        u, h, w = self.unet, traj.h, traj.w
        tid = st["tid"] if u.cfg["addition"] else None
        if traj.plan is not None:
            eps = self._window_forward(sh["win"], sh["x64"], st["tf"], tid, h, w)
        elif traj.reg is not None:
            eps = self._region_forward(sh["reg"], st, sh["x64"], st["tf"], tid, h, w)
        else:
            eps = u.forward(sh["x64"], st["tf"], self.ctx, self.pooled, tid, B=2 * self.n, H=h, W=w, **self._fwd_kw())
        if heat is not None:
            ents = heat_entries(self.rt, h, w)
            if heat["heat"] is None:
                heat["heat"] = self.rt.zeros(self.n, heat["cols"].shape[1], *heat_grid(ents, heat["grid"]), dtype=F32)
            self.rt.ops.heatmap_accum(ents, heat["cols"], st["ctr"], st["hw"], heat["heat"], row_off=1, row_stride=2)
        if traj.apg is not None:
            self.rt.ops.guidance_apg(eps, st["gtab"], st["atab"], sh["mom"], st["ctr"], self.n)
        elif traj.dyn is not None:
            self.rt.ops.guidance_dyn(eps, st["gtab"], st["dtab"], st["ctr"], self.n)
        elif traj.guide is not None:
            self.rt.ops.guidance(eps, st["gtab"], st["ctr"], self.n)
        return eps

    def _iteration(self, st, sh, traj, heat):
        """_predict, then the step launch of the trajectory's family.  The Euler launch from init latents takes them (sh["img"]) at every step, as the
        launch with a hold map does; the multistep and stochastic launches read neither the init latents nor the noise without a mask, whatever the
        trajectory started from."""
        eps = self._predict(st, sh, traj, heat)
        im = sh["img"] if traj.masked or traj.family == "img" or traj.hold is not None else dict(x0=None, noise=None, mask=None)
        self._step_launch(traj.family, st, sh, eps, im["x0"], im["noise"], im["mask"] if traj.masked else None)

    def _graph(self, st, sh, traj, heat):
        """The hipGraph of one iteration for this shape and the adapter scale in effect.  The scale is a launch argument of every adapted GEMM
        (baked by capture), hence part of the key; adapters, DoRA factors, token rows, conditioning, table and counter are device memory.
        Each family's step launch is another kernel: its captures live in a dict of their own (FAMILIES), keyed - txt2img Euler apart - by the mask
        pointer's presence as well (without a mask, the multistep and stochastic launches of txt2img and img2img are the same and share a capture).
        Step count, strength, schedule kind, coefficients, which stochastic sampler and eta are in the table; init latents, noise, mask, the previous
        denoised value and the seeds in persistent buffers: one capture serves all of them.
        guided: the captures with the guidance pre-pass in them, in a fifth dict, keyed by the key the iteration has above plus its family, so they
        neither collide with those captures nor evict them; the scales, phi and the interval are in st["gtab"]: one capture per family serves all.
        apg: the captures with ops.guidance_apg instead, in a sixth dict, that key plus "apg"; eta, threshold and momentum are in st["atab"].
        dyn: the captures with ops.guidance_dyn instead, in a seventh dict, the guided key plus "dyn"; the three values per step are in st["dtab"].
        heat: the captures with ops.heatmap_accum in them are keyed by ("heat", grid, T, P) as well - the launch's shape; which columns and which
        step weights are device memory."""
        h, w, fam, masked, guided = traj.h, traj.w, traj.family, traj.masked, traj.guide is not None
        a, f = self.unet.arena, FAMILIES[fam]
        key = (h, w, self.n, None if a is None else float(a.scale), bool(a is not None and a.dora))
        if f.suffix is not None:
            key += (bool(masked),) + f.suffix
        fu = getattr(self.unet, "_freeu", None)
        if fu is not None:                                # FreeU's b, s and version are launch arguments of ops.freeu: a capture per setting
            key += (("freeu",) + fu,)
        if heat is not None:
            key += (("heat", heat["grid"]) + tuple(heat["cols"].shape[1:]),)
        kd = getattr(self.unet, "_kv_ds", None)
        if kd is not None:                                # key / value downsampling changes the launch sequence: a capture per (factors, mode)
            key += (("kv_downsample",) + kd,)
        if "win" in sh:                                   # tiled diffusion: the window extents and counts; starts and weights are device memory
            key += (("tile",) + tuple(sh["win"]["plan"][2:]),)
        if traj.reg is not None:                          # regional prompts: the region count; masks, weights, backgrounds and the bootstrap table are device memory
            key += (("region", traj.reg["tabs"].R),)
        graphs = getattr(self, f.graphs)
        if guided:
            key, graphs = key + (fam,), self._guided_graphs
        if traj.apg is not None:                          # ops.guidance_apg is another launch: captures of their own; eta, threshold and momentum are in st["atab"]
            key, graphs = key + ("apg",), self._apg_graphs
        if traj.dyn is not None:                          # ops.guidance_dyn likewise; mimic, percentile and interpolate are in st["dtab"]
            key, graphs = key + ("dyn",), self._dyn_graphs
        g = graphs.get(key)
        if g is not None:
            return g
        while len(graphs) >= MAX_GRAPHS:                  # a sweep over many scales: the oldest capture goes
            graphs.pop(next(iter(graphs)))
        ops = self.rt.ops
        prefetch = hasattr(ops, "pf_record_begin") and getattr(ops, "WSK_PREFETCH", False)
        side = torch.cuda.Stream(device=self.rt.device)
        side.wait_stream(torch.cuda.current_stream())
        seq = None
        with torch.cuda.stream(side):
            self._iteration(st, sh, traj, heat)     # eager warm-up: every persistent buffer and packed-weight copy exists before the capture
            if prefetch:                                  # next-weight hints of the wave-split-K products, recorded from one eager pass (step.TrainStep.capture)
                ops.pf_record_begin()
                try:
                    self._iteration(st, sh, traj, heat)
                finally:
                    seq = ops.pf_record_end()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if seq:
                ops.pf_replay_begin(seq)
            try:
                self._iteration(st, sh, traj, heat)
            finally:
                if seq:
                    ops.pf_replay_end()
        graphs[key] = g
        return g

    def _sample_fused(self, traj, embeds, latents, generator, graph):
        rt, f = self.rt, FAMILIES[traj.family]
        sch = self._scheduler(traj)
        st, sh, x0, noise, heat = self._begin(traj, sch, embeds, latents, generator)
        tab = f.table(sch, traj.guidance_scale)          # the rows of the steps that run
        if f.tab not in st:                               # (the multistep and stochastic launches share the 8-column table and the history buffer: both are rewritten per trajectory)
            st[f.tab] = rt.zeros(TABLE_ROWS, f.width, dtype=F32)
        if f.dprev and "dprev" not in sh:
            sh["dprev"] = rt.zeros(self.n, 4, traj.h, traj.w, dtype=F32)
        st[f.tab][: tab.shape[0]].copy_(tab)
        init = lambda: self._step_launch(traj.family, st, sh, None, x0=x0, noise=noise)  # noqa: E731
        with self._scope():
            g = None
            if graph:
                init()                                    # (a defined state for the warm-up passes)
                g = self._graph(st, sh, traj, heat)
            init()
            if heat is not None and heat["heat"] is not None:      # (the warm-up passes of a capture accumulated into it)
                heat["heat"].zero_()
            for _ in range(traj.steps):                   # no host read in here: the step index lives in ctr, its scalars in the table
                if g is not None:
                    g.replay()
                else:
                    self._iteration(st, sh, traj, heat)
        return sh["x"].clone() if heat is None else (sh["x"].clone(), heat["heat"].clone())


def render_images(sampler, decoder, embeds_list, render_size, out_dir, train_step, seed, *, scaling_factor, lora_scale,
                  n_steps=25, guidance_scale=8.0):
    """The loop of `render_images` (inference.py:363-385) after prompt encoding: one image per conditioning 4-tuple, ONE
    generator seeded once for all of them, latents -> vae.decode(latents / scaling_factor) -> [0, 1] -> JPEG quality 95 as
    `img_{train_step:04d}_{i}.jpg`; the adapters are set back to scale 1 afterwards.  render_size = (width, height)."""
    import os
    from PIL import Image
    from . import vae as _vae
    os.makedirs(out_dir, exist_ok=True)
    dev = sampler.rt.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    w, h = render_size[0] // 8, render_size[1] // 8
    sampler.set_lora_scale(lora_scale)
    paths = []
    try:
        for i, embeds in enumerate(embeds_list):
            lat = sampler.sample(embeds, h, w, steps=n_steps, guidance_scale=guidance_scale, generator=gen, size=(render_size[1], render_size[0]))
            img = _vae.postprocess(decoder.decode(lat / scaling_factor))[0].permute(1, 2, 0)
            arr = (img.float().cpu().numpy() * 255).round().astype("uint8")
            paths.append(os.path.join(out_dir, f"img_{train_step:04d}_{i}.jpg"))
            Image.fromarray(arr).save(paths[-1], format="JPEG", quality=95)
    finally:
        sampler.set_lora_scale(1.0)
    return paths
