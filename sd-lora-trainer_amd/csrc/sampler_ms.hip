// The step launch of the latent sampler for DPM-Solver++ (2M) (Lu et al. 2022, the second-order multistep variant) in the sigma parametrisation of
// sampler.hip: the latent is unscaled, the model input is x / sqrt(sigma^2 + 1), lambda = -log sigma.  With the denoised value D_i the update is
//   x_{i+1} = a x + b D_i + c D_{i-1},   a = sigma_{i+1} / sigma_i,  b = (1 - a)(1 + 1 / (2 r)),  c = -(1 - a) / (2 r),  r = h_prev / h
// and the host puts a, b, c into the step's table row (fp64 from the fp32 sigmas, rounded once); c = 0 marks a first-order row (the first step that
// runs, a step to sigma = 0), on which the history is not read.  One kernel serves txt2img, img2img and masked inpainting:
//   init:  x   = noise * sigma_0  |  x0 + noise * sigma_0 (x0 given)       sigma_0 = table row 0, column 1: the FIRST USED sigma
//          xin = bf16(x * 1 / sqrt(sigma_0^2 + 1))
//   step:  e   = eps_neg + g (eps_pos - eps_neg)
//          D   = x - sigma e (epsilon)  |  e * (-sigma / sqrt(sigma^2 + 1)) + x / (sigma^2 + 1) (v prediction)
//          xn  = a x + b D ;  c != 0 only: xn = xn + c dprev
//          k   = x0 + noise * sigma_{i+1} ;  xn = k + m (xn - k)            with a mask only: m = 0 gives k, and k = x0 after the last step (sigma = 0)
//          x   = xn ;  dprev = D ;  xin = bf16(xn * 1 / sqrt(sigma_{i+1}^2 + 1))
// Table rows are 8 floats (header rows as sampler_img.hip's in columns 0..3); counter, last-workgroup ticket, repack into both rows of the pair and
// the 2n timestep writes are sampler_img.hip's.  Step count, strength, the schedule kind and the coefficients live in the table, so one captured graph
// serves any of them, and the counter's wrap to 0 starts the next trajectory on row 0, first order again.  A pure HBM kernel: one thread per pixel,
// coalesced 4-byte reads of the planes, every load requested before the first use.  The variants are template parameters and `c != 0` is uniform
// over the launch (a scalar branch around the four history loads): no load sits under a per-thread condition.  Vector stores only.  All arithmetic in
// fp32, each operation rounded once (no contraction: the tests compare bits).
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

// INIT: IMG = x0 is given.  Step: IMG = a mask is given (x0, noise and mask are read).
template <bool INIT, bool IMG>
__global__ __launch_bounds__(256) void sampler_step_ms_kernel(sdlt_sampler_ms_params p) {
  const float* tab = p.table;
  int i = 0;
  int steps = (int)tab[8];
  steps = max(1, min(steps, p.table_rows - 2));
  float g = 0.f, s = 0.f, sn = 0.f, inv, tnext, ca = 0.f, cb = 0.f, cc = 0.f;
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
  }
  const bool hist = !INIT && cc != 0.f;                 // uniform: the table row is the same for every thread
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
    float xn[4], dn[4];
    if (INIT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = nv[c] * sn;
        xn[c] = IMG ? zv[c] + v : v;
      }
    } else {
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

extern "C" int sdlt_sampler_step_ms(const sdlt_sampler_ms_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: n=%d hw=%d", p->n, p->hw);
  if (p->table_rows < 3) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: table_rows=%d (two header rows + at least one step)", p->table_rows);
  const bool init = p->init != 0, masked = !init && p->mask != nullptr, img = init ? p->x0 != nullptr : masked;
  if (!p->x || !p->xin || !p->timesteps || !p->table || !p->ctr || (!init && (!p->eps || !p->dprev)) || (init && !p->noise) || (masked && (!p->x0 || !p->noise)))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: null pointer (init=%d, mask=%d)", p->init, (int)(p->mask != nullptr));
  if (p->ld_xin < 4 || (p->ld_xin & 3) || ((uintptr_t)p->xin & 7)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_ms: xin needs 8-byte rows (ld=%lld)", (long long)p->ld_xin);
  if (!init && ((uintptr_t)p->eps & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_ms: eps must be 16-byte aligned");
  if ((((uintptr_t)p->x | (uintptr_t)p->x0 | (uintptr_t)p->noise | (uintptr_t)p->mask | (uintptr_t)p->dprev | (uintptr_t)p->timesteps | (uintptr_t)p->table |
        (uintptr_t)p->ctr) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_ms: fp32 / int32 pointers must be 4-byte aligned");
  if ((init || masked) && ((p->x0 != nullptr && p->x0 == p->x) || p->noise == p->x)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: x0 and noise may not alias x");
  if (!init && (p->dprev == p->x || (masked && (p->dprev == p->x0 || p->dprev == p->noise))))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_ms: dprev is written at every step and may not alias x, x0 or noise");
  const int blocks = (int)(((int64_t)p->n * p->hw + 255) / 256);
  const dim3 grid(blocks), block(256);
  if (init && img)
    hipLaunchKernelGGL((sampler_step_ms_kernel<true, true>), grid, block, 0, (hipStream_t)stream, *p);
  else if (init)
    hipLaunchKernelGGL((sampler_step_ms_kernel<true, false>), grid, block, 0, (hipStream_t)stream, *p);
  else if (masked)
    hipLaunchKernelGGL((sampler_step_ms_kernel<false, true>), grid, block, 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL((sampler_step_ms_kernel<false, false>), grid, block, 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
