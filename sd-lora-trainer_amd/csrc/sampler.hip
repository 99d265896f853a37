// The step launch of the latent sampler (sampler.py): classifier-free guidance + the sampler's update + repack of the next model input, the ONE
// launch between two UNet forwards, for n images sampled together (UNet batch 2n: image j = rows 2j negative, 2j + 1 positive).  Five C entry
// points (sdlt_sampler_step, _img, _ms, _sde, _dd) share one init kernel, one step kernel body in three compile-time forms and three mask modes, and
// one host launch path.
//
// Shared contract.  x fp32 [n, 4, h, w] is the unscaled latent, updated in place; the model input is x / sqrt(sigma^2 + 1).
//   init:  x   = noise * sigma_0  |  x0 + noise * sigma_0 (x0 given)       sigma_0 = table row 0, column 1 (init_noise_sigma, or the FIRST USED sigma
//          xin = bf16(x * 1 / sqrt(sigma_0^2 + 1))                          when the host skipped the head of the schedule: img2img strength)
//   step:  e   = eps_neg + g (eps_pos - eps_neg)
//          xn  = the form's update (below)
//          k   = x0 + noise * sigma_{i+1} ;  xn = k + m (xn - k)            with a mask only: m = 0 gives k, and k = x0 after the last step (sigma = 0)
//          k   as above ;  xn = (float)(i + 1) < hold ? k : xn              with a hold map only (sdlt_sampler_step_dd): a SELECT, no arithmetic on xn
//          x   = xn ;  xin = bf16(xn * 1 / sqrt(sigma_{i+1}^2 + 1))         columns 0..3 of BOTH rows of the pair in the NHWC buffer [2n h w, ld]
//   both:  t[0 .. 2n) = next timestep, counter = 0 (init) | (i + 1) mod steps
// Everything a sample() call chooses lives in device memory, so a hipGraph that holds this launch serves any step count, strength, guidance scale,
// prediction type, schedule kind and coefficients: `table` is fp32 [2 + steps, W], W = 4 or 8 by form,
//   row 0: guidance scale, sigma_0, 1 / sqrt(sigma_0^2 + 1), timestep 0               row 1: steps, v-prediction (0 / 1), -, -
//   row 2 + i: sigma_i, sigma_{i+1}, 1 / sqrt(sigma_{i+1}^2 + 1), timestep of step i + 1 [, a_i, b_i, c_i, d_i]
// and ctr[0] is the step counter i (ctr[1]: the ticket that orders its update after every workgroup's read); the counter's wrap to 0 starts the
// next trajectory on row 0.  x0 [n, 4, h, w] (the encoded init latents times the scaling factor), noise [n, 4, h, w] (ONE draw for the whole
// trajectory) and mask [n, 1, h, w] (1 = regenerate, 0 = keep) are read by init and by a masked step only.  hold [n, 1, h, w] (differential
// diffusion, sampler.hold_map: integer-valued, the pixel stays on the init latents' noised trajectory while i + 1 < hold) takes the mask's place in
// sdlt_sampler_step_dd, whose parameter block names the form: a held step reads x0, noise and hold where a masked step reads x0, noise and mask.
// hold = 0 never holds (the maskless step's bits); hold > steps holds after the last step too, where sigma = 0 and k = x0 bit for bit.
//
// The forms.
//   EULER      (sdlt_sampler_step, sdlt_sampler_step_img; W = 4)
//          d   = e (epsilon)  |  (x - (e * (-s / sqrt(s^2 + 1)) + x / (s^2 + 1))) / s (v prediction), s = sigma_i
//          xn  = x + d (sigma_{i+1} - sigma_i)
//   MULTISTEP  (sdlt_sampler_step_ms; W = 8) DPM-Solver++ (2M) (Lu et al. 2022, the second-order multistep variant), lambda = -log sigma: with the
//          denoised value D_i,  x_{i+1} = a x + b D_i + c D_{i-1},  a = sigma_{i+1} / sigma_i,  b = (1 - a)(1 + 1 / (2 r)),  c = -(1 - a) / (2 r),
//          r = h_prev / h; the host puts a, b, c into the step's row (fp64 from the fp32 sigmas, rounded once); c = 0 marks a first-order row (the
//          first step that runs, a step to sigma = 0), on which the history is not read.
//          1. e as above
//          2. D   = x - sigma e (epsilon)  |  e * (-sigma / sqrt(sigma^2 + 1)) + x / (sigma^2 + 1) (v prediction)
//          3. xn  = a x + b D
//          4. c != 0 only (uniform over the launch: a scalar branch around the four history loads):  xn = xn + c dprev
//          5. the mask blend | the hold select
//          6. x = xn ;  dprev = D ;  xin, timesteps, counter
//   SDE        (sdlt_sampler_step_sde; W = 8) Euler ancestral and DPM-Solver++ (2M) SDE (k-diffusion's sample_euler_ancestral and sample_dpmpp_2m_sde,
//          midpoint, s_noise = 1): one more term on the multistep form,  x_{i+1} = a x + b D_i + c D_{i-1} + d z_i,  z_i ~ N(0, I) fresh per step,
//          image and element, d in column 7 (sampler.sde_coefficients; zero in the multistep table).
//          4b. d != 0 only (uniform likewise, a scalar branch around the seed loads and the Philox / Box-Muller work):  xn = xn + d z
//          - BEFORE the mask blend: the kept region is re-injected after the noise.  A d = 0 row (the step to sigma = 0; every row at eta = 0)
//          never reads `seeds` and gives the MULTISTEP form's bits; the MULTISTEP form holds no noise path at all (its entry has no seeds).
//          A replayed graph has no host work between two launches, so z is made HERE, from a device-resident seed per image and the step counter
//          the kernel owns.  One Philox4x32-10 call per pixel of an image gives the four channel normals of that pixel:
//            key     = (seed_lo, seed_hi) of that image             seeds: uint32 [n, 2]
//            counter = (pixel index within the image, step row index i, 0, 0x53444531)
//            u_k     = ((word_k >> 9) + 0.5) 2^-23                  23 bits: (2 m + 1) 2^-24 is exact in fp32 and lies strictly inside (0, 1)
//            z_0, z_1 = sqrt(-2 ln u_0) (cos, sin)(2 pi u_1) ;  z_2, z_3 likewise from (u_2, u_3)       (cos, sin)(2 pi u) = sincospif(2 u): 2 u is exact
//          so image j's noise depends on its own seed, the step and the pixel only - not on the batch it is sampled in or its place there.
//          sdlt_sampler_noise writes z alone through the same device function: the torch loop and the tests take the kernel's own noise from it.
//
// A pure HBM kernel of a few hundred KB: one thread per pixel, coalesced 4-byte reads of the planes (the mask once per pixel), one 16-byte read per
// eps row, two 8-byte bf16 stores.  Every load of a pixel is requested before the first use; form and mask mode are template parameters and `c != 0`,
// `d != 0` are uniform over the launch, so no load sits under a per-thread condition (the hold select is per thread, on values already loaded).  Vector stores only.  All arithmetic in fp32, each operation
// rounded once (no contraction: the tests compare bits).
#include "common.h"
#include "philox.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

enum Form { EULER, MULTISTEP, SDE };
enum Mask { MASK_NONE, MASK_BLEND, MASK_HOLD };

// The five public parameter blocks, widened to one: an operand an entry point does not have is NULL.
struct step_args {
  const float* eps;
  float* x;
  const float *x0, *noise, *mask;
  float* dprev;
  void* xin;
  int64_t ld_xin;
  float* timesteps;
  const float* table;
  int32_t* ctr;
  const uint32_t* seeds;
  int32_t n, hw, table_rows;
  const float* hold;
};

// The four channel normals of pixel `px` of an image with key (k0, k1) at step row `step` (philox.h: the generator region.hip shares).
__device__ __forceinline__ void sde_noise4(uint32_t k0, uint32_t k1, uint32_t px, uint32_t step, float z[4]) {
  philox_normal4(px, step, 0u, NOISE_TAG, k0, k1, z);
}

__global__ __launch_bounds__(256) void sampler_noise_kernel(const uint32_t* seeds, int step, int n, int hw, float* out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * hw) return;
  const int j = idx / hw, px = idx - j * hw;
  const uint32_t k0 = seeds[2 * j], k1 = seeds[2 * j + 1];
  float z[4];
  sde_noise4(k0, k1, (uint32_t)px, (uint32_t)step, z);
  float* o = out + (size_t)j * 4 * hw + px;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[(size_t)c * hw] = z[c];
}

// ---- the pieces of a launch, each written once

// What a step reads from the table and the counter: steps clamped to the table, the counter to the steps.  (Init reads row 0, columns 1..3 only:
// the same offsets for both row widths.)
struct step_row {
  int i, steps;
  float g, s, sn, inv, tnext, a, b, c, d;
  bool vpred;
};

template <Form FORM>
__device__ __forceinline__ step_row read_row(const step_args& p) {
  constexpr int W = FORM == EULER ? 4 : 8;
  const float* tab = p.table;
  step_row r = {};
  r.steps = max(1, min((int)tab[W], p.table_rows - 2));
  r.vpred = tab[W + 1] != 0.f;
  r.i = max(0, min(p.ctr[0], r.steps - 1));
  const float* row = tab + W * (2 + r.i);
  r.g = tab[0];
  r.s = row[0];
  r.sn = row[1];
  r.inv = row[2];
  r.tnext = row[3];
  if (FORM != EULER) {
    r.a = row[4];
    r.b = row[5];
    r.c = row[6];
  }
  if (FORM == SDE) r.d = row[7];
  return r;
}

__device__ __forceinline__ void load_planes(const float* p, int hw, float v[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = p[(size_t)c * hw];
}

__device__ __forceinline__ void store_planes(float* p, int hw, const float v[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) p[(size_t)c * hw] = v[c];
}

// The known region noised to the sigma the step arrived at, and the blend with it.
__device__ __forceinline__ float mask_blend(float v, float z, float nz, float sn, float m) {
  const float k = z + nz * sn;
  return k + m * (v - k);
}

// The same k, selected while the pixel is held: step row i leaves it on the noised trajectory iff i + 1 < hold.  A released pixel keeps v's bits.
__device__ __forceinline__ float hold_select(float v, float z, float nz, float sn, float hold, int i) {
  const float k = z + nz * sn;
  return (float)(i + 1) < hold ? k : v;
}

// x and the bf16 model input, into both rows of the pair.
__device__ __forceinline__ void store_repack(const step_args& p, int j, int px, const float xn[4], float inv) {
  const int hw = p.hw;
  store_planes(p.x + (size_t)j * 4 * hw + px, hw, xn);
  uint2 v;
  v.x = pack2bf(xn[0] * inv, xn[1] * inv);
  v.y = pack2bf(xn[2] * inv, xn[3] * inv);
  bf16_t* o = (bf16_t*)p.xin;
  *(uint2*)(o + ((size_t)(2 * j) * hw + px) * p.ld_xin) = v;
  *(uint2*)(o + ((size_t)(2 * j + 1) * hw + px) * p.ld_xin) = v;
}

// The timesteps of the next forward and the counter: written by the workgroup that finishes LAST, after every workgroup has read ctr[0].  Init
// reads no counter, so its first workgroup writes them.
template <bool INIT>
__device__ __forceinline__ void ticket_tail(const step_args& p, float tnext, int next) {
  __shared__ int last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = INIT ? (blockIdx.x == 0) : (atomicAdd(&p.ctr[1], 1) == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!last) return;
  for (int b = threadIdx.x; b < 2 * p.n; b += 256) p.timesteps[b] = tnext;
  if (threadIdx.x == 0) {
    p.ctr[0] = next;
    p.ctr[1] = 0;
  }
}

// ---- the two kernels

template <bool X0>
__global__ __launch_bounds__(256) void sampler_init_kernel(step_args p) {
  const float* tab = p.table;
  const float s0 = tab[1], inv = tab[2], tnext = tab[3];
  const int hw = p.hw;
  const int idx = blockIdx.x * 256 + threadIdx.x;       // pixel of image j
  if (idx < p.n * hw) {
    const int j = idx / hw, px = idx - j * hw;
    const size_t base = (size_t)j * 4 * hw + px;
    float zv[4] = {0.f, 0.f, 0.f, 0.f}, nv[4], xn[4];
    if (X0) load_planes(p.x0 + base, hw, zv);
    load_planes(p.noise + base, hw, nv);                // (noise may be x itself where the entry allows it: read here, written below)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = nv[c] * s0;
      xn[c] = X0 ? zv[c] + v : v;
    }
    store_repack(p, j, px, xn, inv);
  }
  ticket_tail<true>(p, tnext, 0);
}

template <Form FORM, Mask MASK>
__global__ __launch_bounds__(256) void sampler_step_kernel(step_args p) {
  const step_row r = read_row<FORM>(p);
  const bool hist = FORM != EULER && r.c != 0.f;        // uniform: the table row is the same for every thread
  const bool noisy = FORM == SDE && r.d != 0.f;         // uniform likewise
  const int hw = p.hw;
  const int idx = blockIdx.x * 256 + threadIdx.x;       // pixel of image j
  if (idx < p.n * hw) {
    const int j = idx / hw, px = idx - j * hw;
    const size_t base = (size_t)j * 4 * hw + px;
    // ---- every load of this pixel, before anything is used
    const f32x4 en = *(const f32x4*)(p.eps + ((size_t)(2 * j) * hw + px) * 4);
    const f32x4 ep = *(const f32x4*)(p.eps + ((size_t)(2 * j + 1) * hw + px) * 4);
    float xv[4], dv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, nv[4] = {0.f, 0.f, 0.f, 0.f}, m = 1.f;
    uint32_t k0 = 0u, k1 = 0u;
    load_planes(p.x + base, hw, xv);
    if (MASK != MASK_NONE) {
      load_planes(p.x0 + base, hw, zv);
      load_planes(p.noise + base, hw, nv);
      m = (MASK == MASK_HOLD ? p.hold : p.mask)[(size_t)j * hw + px];
    }
    if (hist) load_planes(p.dprev + base, hw, dv);
    if (noisy) {
      k0 = p.seeds[2 * j];
      k1 = p.seeds[2 * j + 1];
    }
    float fresh[4] = {0.f, 0.f, 0.f, 0.f};
    if (noisy) sde_noise4(k0, k1, (uint32_t)px, (uint32_t)r.i, fresh);
    // ---- guidance, the denoised value and the form's update
    const float s = r.s, sn = r.sn, dt = sn - s;
    float c1 = 0.f, c2 = 0.f;
    if (r.vpred) {
      const float q = s * s + 1.f;
      c1 = -s / sqrtf(q);
      c2 = q;
    }
    float xn[4], dn[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = xv[c];
      const float e = en[c] + r.g * (ep[c] - en[c]);
      float v;
      if (FORM == EULER) {
        float d = e;
        if (r.vpred) {
          const float x0 = e * c1 + x / c2;
          d = (x - x0) / s;
        }
        v = x + d * dt;
      } else {
        const float D = r.vpred ? e * c1 + x / c2 : x - s * e;
        v = r.a * x + r.b * D;
        if (hist) v = v + r.c * dv[c];
        if (noisy) v = v + r.d * fresh[c];
        dn[c] = D;
      }
      if (MASK == MASK_BLEND) v = mask_blend(v, zv[c], nv[c], sn, m);
      if (MASK == MASK_HOLD) v = hold_select(v, zv[c], nv[c], sn, m, r.i);
      xn[c] = v;
    }
    if (FORM != EULER) store_planes(p.dprev + base, hw, dn);
    store_repack(p, j, px, xn, r.inv);
  }
  ticket_tail<false>(p, r.tnext, r.i + 1 >= r.steps ? 0 : r.i + 1);
}

// ---- the one host path

// What differs between the entry points, as data.
struct entry_rules {
  Form form;
  const char* name;
  bool img;                  // the entry has x0 / mask operands (its null-pointer text names the mask)
  bool init_needs_x0;        // sdlt_sampler_step_img: init is x0 + noise * sigma_0, always
  const char* alias_text;    // x0 / noise aliasing x: refused with this text; NULL: allowed (sdlt_sampler_step's init, noise == x)
  bool dd;                   // sdlt_sampler_step_dd: every step takes a hold map (its null-pointer text names it)
};

template <Form FORM>
void launch_step(Mask mode, dim3 grid, hipStream_t stream, const step_args& a) {
  if (mode == MASK_HOLD)
    hipLaunchKernelGGL((sampler_step_kernel<FORM, MASK_HOLD>), grid, dim3(256), 0, stream, a);
  else if (mode == MASK_BLEND)
    hipLaunchKernelGGL((sampler_step_kernel<FORM, MASK_BLEND>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((sampler_step_kernel<FORM, MASK_NONE>), grid, dim3(256), 0, stream, a);
}

int sampler_launch(const entry_rules& r, const step_args& a, int init_flag, void* stream) {
  const char* nm = r.name;
  const bool ms = r.form != EULER, sde = r.form == SDE;
  if (a.n < 1 || a.hw < 1 || (int64_t)a.n * a.hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d hw=%d", nm, a.n, a.hw);
  if (a.table_rows < 3) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: table_rows=%d (two header rows + at least one step)", nm, a.table_rows);
  const bool init = init_flag != 0, held = !init && r.dd, masked = !init && (held || a.mask != nullptr);      // masked: the step reads x0 and noise
  if (!a.x || !a.xin || !a.timesteps || !a.table || !a.ctr || (!init && (!a.eps || (ms && !a.dprev) || (sde && !a.seeds))) || (held && !a.hold) ||
      ((init || masked) && !a.noise) || ((masked || (init && r.init_needs_x0)) && !a.x0)) {
    if (r.dd) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null pointer (init=%d, hold=%d)", nm, init_flag, (int)(a.hold != nullptr));
    if (r.img) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null pointer (init=%d, mask=%d)", nm, init_flag, (int)(a.mask != nullptr));
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null pointer (init=%d)", nm, init_flag);
  }
  if (a.ld_xin < 4 || (a.ld_xin & 3) || ((uintptr_t)a.xin & 7)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: xin needs 8-byte rows (ld=%lld)", nm, (long long)a.ld_xin);
  if (!init && ((uintptr_t)a.eps & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: eps must be 16-byte aligned", nm);
  if ((((uintptr_t)a.x | (uintptr_t)a.x0 | (uintptr_t)a.noise | (uintptr_t)a.mask | (uintptr_t)a.dprev | (uintptr_t)a.timesteps | (uintptr_t)a.table |
        (uintptr_t)a.ctr | (uintptr_t)a.hold) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: fp32 / int32 pointers must be 4-byte aligned", nm);
  if (!init && ((uintptr_t)a.seeds & 3)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: seeds must be 4-byte aligned", nm);
  if (r.alias_text && (init || masked) && ((a.x0 != nullptr && a.x0 == a.x) || a.noise == a.x)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: %s", nm, r.alias_text);
  if (ms && !init && (a.dprev == a.x || (masked && (a.dprev == a.x0 || a.dprev == a.noise))))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: dprev is written at every step and may not alias x, x0 or noise", nm);
  if (held && (a.hold == a.x || (ms && a.hold == a.dprev))) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: hold is read while x and dprev are written and may alias neither", nm);
  const Mask mode = held ? MASK_HOLD : masked ? MASK_BLEND : MASK_NONE;
  const dim3 grid((unsigned)(((int64_t)a.n * a.hw + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (init && a.x0 != nullptr)
    hipLaunchKernelGGL((sampler_init_kernel<true>), grid, dim3(256), 0, st, a);
  else if (init)
    hipLaunchKernelGGL((sampler_init_kernel<false>), grid, dim3(256), 0, st, a);
  else if (r.form == EULER)
    launch_step<EULER>(mode, grid, st, a);
  else if (r.form == MULTISTEP)
    launch_step<MULTISTEP>(mode, grid, st, a);
  else
    launch_step<SDE>(mode, grid, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) SDLT_FAIL(SDLT_ERR_LAUNCH, "%s: %s", nm, hipGetErrorString(e));
  return SDLT_OK;
}

}  // namespace

extern "C" int sdlt_sampler_step(const sdlt_sampler_params* p, void* stream) {
  static const entry_rules R = {EULER, "sdlt_sampler_step", false, false, nullptr};
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", R.name);
  const step_args a = {p->eps, p->x, nullptr, p->noise, nullptr, nullptr, p->xin, p->ld_xin, p->timesteps, p->table, p->ctr, nullptr, p->n, p->hw, p->table_rows};
  return sampler_launch(R, a, p->init, stream);
}

extern "C" int sdlt_sampler_step_img(const sdlt_sampler_img_params* p, void* stream) {
  static const entry_rules R = {EULER, "sdlt_sampler_step_img", true, true, "x0 and noise are read at every step and may not alias x"};
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", R.name);
  const step_args a = {p->eps, p->x, p->x0, p->noise, p->mask, nullptr, p->xin, p->ld_xin, p->timesteps, p->table, p->ctr, nullptr, p->n, p->hw, p->table_rows};
  return sampler_launch(R, a, p->init, stream);
}

extern "C" int sdlt_sampler_step_ms(const sdlt_sampler_ms_params* p, void* stream) {
  static const entry_rules R = {MULTISTEP, "sdlt_sampler_step_ms", true, false, "x0 and noise may not alias x"};
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", R.name);
  const step_args a = {p->eps, p->x, p->x0, p->noise, p->mask, p->dprev, p->xin, p->ld_xin, p->timesteps, p->table, p->ctr, nullptr, p->n, p->hw, p->table_rows};
  return sampler_launch(R, a, p->init, stream);
}

extern "C" int sdlt_sampler_step_sde(const sdlt_sampler_sde_params* p, void* stream) {
  static const entry_rules R = {SDE, "sdlt_sampler_step_sde", true, false, "x0 and noise may not alias x"};
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", R.name);
  const step_args a = {p->eps, p->x, p->x0, p->noise, p->mask, p->dprev, p->xin, p->ld_xin, p->timesteps, p->table, p->ctr, p->seeds, p->n, p->hw, p->table_rows};
  return sampler_launch(R, a, p->init, stream);
}

extern "C" int sdlt_sampler_step_dd(const sdlt_sampler_dd_params* p, void* stream) {
  static const entry_rules R[3] = {{EULER, "sdlt_sampler_step_dd", true, true, "x0 and noise are read at every step and may not alias x", true},
                                   {MULTISTEP, "sdlt_sampler_step_dd", true, true, "x0 and noise are read at every step and may not alias x", true},
                                   {SDE, "sdlt_sampler_step_dd", true, true, "x0 and noise are read at every step and may not alias x", true}};
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", R[0].name);
  if (p->form < 0 || p->form > 2) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: form=%d (0 Euler, 1 multistep, 2 SDE)", R[0].name, p->form);
  const step_args a = {p->eps, p->x, p->x0, p->noise, nullptr, p->form != EULER ? p->dprev : nullptr, p->xin, p->ld_xin, p->timesteps, p->table, p->ctr,
                       p->form == SDE ? p->seeds : nullptr, p->n, p->hw, p->table_rows, p->hold};
  return sampler_launch(R[p->form], a, p->init, stream);
}

extern "C" int sdlt_sampler_noise(const uint32_t* seeds, int32_t step, int32_t n, int32_t hw, float* out, void* stream) {
  if (n < 1 || hw < 1 || (int64_t)n * hw > (1 << 28) || step < 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_noise: n=%d hw=%d step=%d", n, hw, step);
  if (!seeds || !out) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_noise: null pointer");
  if (((uintptr_t)seeds | (uintptr_t)out) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_noise: seeds and out must be 4-byte aligned");
  const int blocks = (int)(((int64_t)n * hw + 255) / 256);
  hipLaunchKernelGGL(sampler_noise_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, seeds, (int)step, (int)n, (int)hw, out);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
