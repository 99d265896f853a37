// The step launch of the latent sampler for the two stochastic samplers, Euler ancestral and DPM-Solver++ (2M) SDE (k-diffusion's
// sample_euler_ancestral and sample_dpmpp_2m_sde, midpoint, s_noise = 1), in the sigma parametrisation of sampler_ms.hip.  Both are one more term on
// the multistep form:
//   x_{i+1} = a x + b D_i + c D_{i-1} + d z_i,      z_i ~ N(0, I), fresh per step, image and element
// with a, b, c, d in the step's table row (sampler.sde_coefficients: fp64 from the fp32 sigmas, rounded once; column 7, zero in sampler_ms.hip's
// table, is d).  A replayed graph has no host work between two launches, so z is made HERE, from a device-resident seed per image and the step
// counter the kernel owns.  One Philox4x32-10 call per pixel of an image gives the four channel normals of that pixel:
//   key     = (seed_lo, seed_hi) of that image             seeds: uint32 [n, 2]
//   counter = (pixel index within the image, step row index i, 0, 0x53444531)
//   u_k     = ((word_k >> 9) + 0.5) 2^-23                  23 bits: (2 m + 1) 2^-24 is exact in fp32 and lies strictly inside (0, 1)
//   z_0, z_1 = sqrt(-2 ln u_0) (cos, sin)(2 pi u_1) ;  z_2, z_3 likewise from (u_2, u_3)       (cos, sin)(2 pi u) = sincospif(2 u): 2 u is exact
// so image j's noise depends on its own seed, the step and the pixel only - not on the batch it is sampled in or its place there.
//   step:  e, D, xn = a x + b D (+ c dprev) as sampler_ms.hip
//          d != 0 only:  xn = xn + d z                              BEFORE the mask blend: the kept region is re-injected after the noise
//          mask blend, x, dprev, xin, timesteps, counter as sampler_ms.hip
// `d != 0` is uniform over the launch, a scalar branch around the seed loads and the Philox / Box-Muller work like `c != 0` around the history loads:
// a d = 0 row (the step to sigma = 0; every row at eta = 0) never reads `seeds`, and gives sdlt_sampler_step_ms's bits.  sdlt_sampler_noise writes z
// alone through the same device function: the torch loop and the tests take the kernel's own noise from it.  The rules are sampler_ms.hip's: one
// thread per pixel, every load requested before the first use, no load under a per-thread condition, fp32 with one rounding per operation (no
// contraction: the tests compare bits), vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr uint32_t NOISE_TAG = 0x53444531u;             // counter word 3: keeps these draws apart from any other use of the same seed

// Philox4x32-10 (Salmon et al. 2011, Random123): ten rounds, the key bumped by the Weyl constants between them.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// The four channel normals of pixel `px` of an image with key (k0, k1) at step row `step`.
__device__ __forceinline__ void sde_noise4(uint32_t k0, uint32_t k1, uint32_t px, uint32_t step, float z[4]) {
  uint32_t w[4];
  philox4x32_10(px, step, 0u, NOISE_TAG, k0, k1, w);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u0 = ((float)(w[2 * h] >> 9) + 0.5f) * 0x1p-23f;
    const float u1 = ((float)(w[2 * h + 1] >> 9) + 0.5f) * 0x1p-23f;
    const float r = sqrtf(-2.f * logf(u0));
    float sn, cs;
    sincospif(2.f * u1, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
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

// INIT: IMG = x0 is given.  Step: IMG = a mask is given (x0, noise and mask are read).
template <bool INIT, bool IMG>
__global__ __launch_bounds__(256) void sampler_step_sde_kernel(sdlt_sampler_sde_params p) {
  const float* tab = p.table;
  int i = 0;
  int steps = (int)tab[8];
  steps = max(1, min(steps, p.table_rows - 2));
  float g = 0.f, s = 0.f, sn = 0.f, inv, tnext, ca = 0.f, cb = 0.f, cc = 0.f, cd = 0.f;
  const bool vpred = tab[9] != 0.f;
  if (INIT) {
    sn = tab[1];
    inv = tab[2];
    tnext = tab[3];
  } else {
    i = max(0, min(p.ctr[0], steps - 1));
    const float* row = tab + 8 * (2 + i);
    g = tab[0];
    s = row[0];
    sn = row[1];
    inv = row[2];
    tnext = row[3];
    ca = row[4];
    cb = row[5];
    cc = row[6];
    cd = row[7];
  }
  const bool hist = !INIT && cc != 0.f;                 // uniform: the table row is the same for every thread
  const bool noisy = !INIT && cd != 0.f;                // uniform likewise
  const int hw = p.hw;
  const int idx = blockIdx.x * 256 + threadIdx.x;       // pixel of image j
  if (idx < p.n * hw) {
    const int j = idx / hw, px = idx - j * hw;
    const size_t base = (size_t)j * 4 * hw + px;
    float* xp = p.x + base;
    float* dp = p.dprev + base;
    // ---- every load of this pixel, before anything is used
    f32x4 en = {0.f, 0.f, 0.f, 0.f}, ep = {0.f, 0.f, 0.f, 0.f};
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, nv[4] = {0.f, 0.f, 0.f, 0.f}, m = 1.f;
    uint32_t k0 = 0u, k1 = 0u;
    if (!INIT) {
      en = *(const f32x4*)(p.eps + ((size_t)(2 * j) * hw + px) * 4);
      ep = *(const f32x4*)(p.eps + ((size_t)(2 * j + 1) * hw + px) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) xv[c] = xp[(size_t)c * hw];
    }
    if (IMG) {
#pragma unroll
      for (int c = 0; c < 4; ++c) zv[c] = p.x0[base + (size_t)c * hw];
    }
    if (INIT || IMG) {
#pragma unroll
      for (int c = 0; c < 4; ++c) nv[c] = p.noise[base + (size_t)c * hw];
    }
    if (!INIT && IMG) m = p.mask[(size_t)j * hw + px];
    if (hist) {
#pragma unroll
      for (int c = 0; c < 4; ++c) dv[c] = dp[(size_t)c * hw];
    }
    if (noisy) {
      k0 = p.seeds[2 * j];
      k1 = p.seeds[2 * j + 1];
    }
    float xn[4], dn[4];
    if (INIT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = nv[c] * sn;
        xn[c] = IMG ? zv[c] + v : v;
      }
    } else {
      float fresh[4] = {0.f, 0.f, 0.f, 0.f};
      if (noisy) sde_noise4(k0, k1, (uint32_t)px, (uint32_t)i, fresh);
      float c1 = 0.f, c2 = 0.f;
      if (vpred) {
        const float q = s * s + 1.f;
        c1 = -s / sqrtf(q);
        c2 = q;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = xv[c];
        const float e = en[c] + g * (ep[c] - en[c]);
        const float D = vpred ? e * c1 + x / c2 : x - s * e;
        float v = ca * x + cb * D;
        if (hist) v = v + cc * dv[c];
        if (noisy) v = v + cd * fresh[c];
        if (IMG) {
          const float k = zv[c] + nv[c] * sn;
          v = k + m * (v - k);
        }
        xn[c] = v;
        dn[c] = D;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) xp[(size_t)c * hw] = xn[c];
    if (!INIT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) dp[(size_t)c * hw] = dn[c];
    }
    uint2 v;
    v.x = pack2bf(xn[0] * inv, xn[1] * inv);
    v.y = pack2bf(xn[2] * inv, xn[3] * inv);
    bf16_t* o = (bf16_t*)p.xin;
    *(uint2*)(o + ((size_t)(2 * j) * hw + px) * p.ld_xin) = v;
    *(uint2*)(o + ((size_t)(2 * j + 1) * hw + px) * p.ld_xin) = v;
  }
  // the timesteps of the next forward and the counter: written by the workgroup that finishes LAST, after every workgroup has read ctr[0]
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
    p.ctr[0] = INIT ? 0 : (i + 1 >= steps ? 0 : i + 1);
    p.ctr[1] = 0;
  }
}

}  // namespace

extern "C" int sdlt_sampler_step_sde(const sdlt_sampler_sde_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: n=%d hw=%d", p->n, p->hw);
  if (p->table_rows < 3) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: table_rows=%d (two header rows + at least one step)", p->table_rows);
  const bool init = p->init != 0, masked = !init && p->mask != nullptr, img = init ? p->x0 != nullptr : masked;
  if (!p->x || !p->xin || !p->timesteps || !p->table || !p->ctr || (!init && (!p->eps || !p->dprev || !p->seeds)) || (init && !p->noise) ||
      (masked && (!p->x0 || !p->noise)))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: null pointer (init=%d, mask=%d)", p->init, (int)(p->mask != nullptr));
  if (p->ld_xin < 4 || (p->ld_xin & 3) || ((uintptr_t)p->xin & 7)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_sde: xin needs 8-byte rows (ld=%lld)", (long long)p->ld_xin);
  if (!init && ((uintptr_t)p->eps & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_sde: eps must be 16-byte aligned");
  if ((((uintptr_t)p->x | (uintptr_t)p->x0 | (uintptr_t)p->noise | (uintptr_t)p->mask | (uintptr_t)p->dprev | (uintptr_t)p->timesteps | (uintptr_t)p->table |
        (uintptr_t)p->ctr) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_sde: fp32 / int32 pointers must be 4-byte aligned");
  if (!init && ((uintptr_t)p->seeds & 3)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_sde: seeds must be 4-byte aligned");
  if ((init || masked) && ((p->x0 != nullptr && p->x0 == p->x) || p->noise == p->x)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: x0 and noise may not alias x");
  if (!init && (p->dprev == p->x || (masked && (p->dprev == p->x0 || p->dprev == p->noise))))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_sde: dprev is written at every step and may not alias x, x0 or noise");
  const int blocks = (int)(((int64_t)p->n * p->hw + 255) / 256);
  const dim3 grid(blocks), block(256);
  if (init && img)
    hipLaunchKernelGGL((sampler_step_sde_kernel<true, true>), grid, block, 0, (hipStream_t)stream, *p);
  else if (init)
    hipLaunchKernelGGL((sampler_step_sde_kernel<true, false>), grid, block, 0, (hipStream_t)stream, *p);
  else if (masked)
    hipLaunchKernelGGL((sampler_step_sde_kernel<false, true>), grid, block, 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL((sampler_step_sde_kernel<false, false>), grid, block, 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
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
