// The step launch of the latent sampler when it starts from an init image (img2img) and, with a mask, re-injects the known region after every
// step (inpainting): sampler.hip's kernel with three more fp32 inputs, x0 [n, 4, h, w] (the encoded init latents times the scaling factor),
// noise [n, 4, h, w] (ONE draw for the whole trajectory) and mask [n, 1, h, w] (optional; 1 = regenerate, 0 = keep).
//   init:  x   = x0 + noise * sigma_0                                   sigma_0 = table row 0, column 1: the FIRST USED sigma
//          xin = bf16(x * 1 / sqrt(sigma_0^2 + 1))
//   step:  e, d, xn = x + d (sigma_{i+1} - sigma_i)                      exactly as sampler_step_kernel, epsilon and v prediction
//          k   = x0 + noise * sigma_{i+1} ;  xn = k + m (xn - k)         with a mask only: m = 0 gives k, and k = x0 after the last step (sigma = 0)
//          x   = xn ;  xin = bf16(xn * 1 / sqrt(sigma_{i+1}^2 + 1))
// Same table layout, counter and last-workgroup ticket, same repack into both rows of the pair; strength and step count live in the table
// (the host skips the head of the schedule), so one captured graph serves any of them.  A pure HBM kernel: one thread per pixel, coalesced
// 4-byte reads of the planes (the mask once per pixel), every load requested before the first use (the variants are template parameters: no
// load sits under a condition), vector stores only.  All arithmetic in fp32, each operation rounded once (no contraction: the tests compare bits).
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

template <bool INIT, bool MASK>
__global__ __launch_bounds__(256) void sampler_step_img_kernel(sdlt_sampler_img_params p) {
  const float* tab = p.table;
  int i = 0;
  int steps = (int)tab[4];
  steps = max(1, min(steps, p.table_rows - 2));
  float g = 0.f, s = 0.f, sn = 0.f, inv, tnext;
  const bool vpred = tab[5] != 0.f;
  if (INIT) {
    sn = tab[1];
    inv = tab[2];
    tnext = tab[3];
  } else {
    i = max(0, min(p.ctr[0], steps - 1));
    const float* row = tab + 4 * (2 + i);
    g = tab[0];
    s = row[0];
    sn = row[1];
    inv = row[2];
    tnext = row[3];
  }
  const int hw = p.hw;
  const int idx = blockIdx.x * 256 + threadIdx.x;       // pixel of image j
  if (idx < p.n * hw) {
    const int j = idx / hw, px = idx - j * hw;
    const size_t base = (size_t)j * 4 * hw + px;
    float* xp = p.x + base;
    // ---- every load of this pixel, before anything is used
    f32x4 en = {0.f, 0.f, 0.f, 0.f}, ep = {0.f, 0.f, 0.f, 0.f};
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, nv[4] = {0.f, 0.f, 0.f, 0.f}, m = 1.f;
    if (!INIT) {
      en = *(const f32x4*)(p.eps + ((size_t)(2 * j) * hw + px) * 4);
      ep = *(const f32x4*)(p.eps + ((size_t)(2 * j + 1) * hw + px) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) xv[c] = xp[(size_t)c * hw];
    }
    if (INIT || MASK) {
#pragma unroll
      for (int c = 0; c < 4; ++c) zv[c] = p.x0[base + (size_t)c * hw];
#pragma unroll
      for (int c = 0; c < 4; ++c) nv[c] = p.noise[base + (size_t)c * hw];
    }
    if (MASK) m = p.mask[(size_t)j * hw + px];
    float xn[4];
    if (INIT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) xn[c] = zv[c] + nv[c] * sn;
    } else {
      const float dt = sn - s;
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
        float d = e;
        if (vpred) {
          const float x0 = e * c1 + x / c2;
          d = (x - x0) / s;
        }
        float v = x + d * dt;
        if (MASK) {
          const float k = zv[c] + nv[c] * sn;
          v = k + m * (v - k);
        }
        xn[c] = v;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) xp[(size_t)c * hw] = xn[c];
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

extern "C" int sdlt_sampler_step_img(const sdlt_sampler_img_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_img: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_img: n=%d hw=%d", p->n, p->hw);
  if (p->table_rows < 3) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_img: table_rows=%d (two header rows + at least one step)", p->table_rows);
  const bool init = p->init != 0, masked = !init && p->mask != nullptr;
  if (!p->x || !p->xin || !p->timesteps || !p->table || !p->ctr || (!init && !p->eps) || ((init || masked) && (!p->x0 || !p->noise)))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_img: null pointer (init=%d, mask=%d)", p->init, (int)(p->mask != nullptr));
  if (p->ld_xin < 4 || (p->ld_xin & 3) || ((uintptr_t)p->xin & 7)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_img: xin needs 8-byte rows (ld=%lld)", (long long)p->ld_xin);
  if (!init && ((uintptr_t)p->eps & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_img: eps must be 16-byte aligned");
  if ((((uintptr_t)p->x | (uintptr_t)p->x0 | (uintptr_t)p->noise | (uintptr_t)p->mask | (uintptr_t)p->timesteps | (uintptr_t)p->table | (uintptr_t)p->ctr) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step_img: fp32 / int32 pointers must be 4-byte aligned");
  if ((init || masked) && (p->x0 == p->x || p->noise == p->x)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step_img: x0 and noise are read at every step and may not alias x");
  const int blocks = (int)(((int64_t)p->n * p->hw + 255) / 256);
  const dim3 grid(blocks), block(256);
  if (init)
    hipLaunchKernelGGL((sampler_step_img_kernel<true, false>), grid, block, 0, (hipStream_t)stream, *p);
  else if (masked)
    hipLaunchKernelGGL((sampler_step_img_kernel<false, true>), grid, block, 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL((sampler_step_img_kernel<false, false>), grid, block, 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
