// Classifier-free guidance + Euler-discrete update + repack of the next model input: the ONE launch between two UNet forwards of the
// latent sampler (sampler.py), for n images sampled together (UNet batch 2n: image j = rows 2j negative, 2j + 1 positive).
//   e      = eps_neg + g (eps_pos - eps_neg)
//   d      = e                                                          (epsilon prediction)
//          = (x - (e * (-s / sqrt(s^2 + 1)) + x / (s^2 + 1))) / s       (v prediction), s = sigma_i
//   x     += d (sigma_{i+1} - sigma_i)                                  fp32 [n, 4, h, w], in place
//   xin    = bf16(x * 1 / sqrt(sigma_{i+1}^2 + 1))                      columns 0..3 of BOTH rows of the pair in the NHWC buffer [2n h w, ld]
//   t[0 .. 2n) = next timestep, counter = (i + 1) mod steps
// Everything a sample() call chooses lives in device memory, so a hipGraph that holds this launch serves any step count, guidance
// scale and prediction type: `table` is fp32 [2 + steps, 4],
//   row 0: guidance scale, init_noise_sigma, 1 / sqrt(sigma_0^2 + 1), timestep 0      row 1: steps, v-prediction (0 / 1), -, -
//   row 2 + i: sigma_i, sigma_{i+1}, 1 / sqrt(sigma_{i+1}^2 + 1), timestep of step i + 1
// and ctr[0] is the step counter i (ctr[1]: the ticket that orders its update after every workgroup's read).
// A pure HBM kernel of a few hundred KB: one thread per pixel, coalesced 4-byte reads of the four NCHW planes, one 16-byte read per eps
// row, two 8-byte bf16 stores.  All arithmetic in fp32, each operation rounded once (no contraction: the tests count them).
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void sampler_step_kernel(sdlt_sampler_params p) {
  const float* tab = p.table;
  int i = 0;
  int steps = (int)tab[4];
  steps = max(1, min(steps, p.table_rows - 2));
  float g = 0.f, s = 0.f, sn = 0.f, inv, tnext;
  const bool vpred = tab[5] != 0.f;
  if (p.init) {
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
    float* xp = p.x + (size_t)j * 4 * hw + px;
    float xn[4];
    if (p.init) {
      const float* np_ = p.noise + (size_t)j * 4 * hw + px;
      const float s0 = tab[1];
#pragma unroll
      for (int c = 0; c < 4; ++c) xn[c] = np_[(size_t)c * hw] * s0;
    } else {
      const f32x4 en = *(const f32x4*)(p.eps + ((size_t)(2 * j) * hw + px) * 4);
      const f32x4 ep = *(const f32x4*)(p.eps + ((size_t)(2 * j + 1) * hw + px) * 4);
      const float dt = sn - s;
      float c1 = 0.f, c2 = 0.f;
      if (vpred) {
        const float q = s * s + 1.f;
        c1 = -s / sqrtf(q);
        c2 = q;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = xp[(size_t)c * hw];
        const float e = en[c] + g * (ep[c] - en[c]);
        float d = e;
        if (vpred) {
          const float x0 = e * c1 + x / c2;
          d = (x - x0) / s;
        }
        xn[c] = x + d * dt;
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
    last = p.init ? (blockIdx.x == 0) : (atomicAdd(&p.ctr[1], 1) == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (!last) return;
  for (int b = threadIdx.x; b < 2 * p.n; b += 256) p.timesteps[b] = tnext;
  if (threadIdx.x == 0) {
    p.ctr[0] = p.init ? 0 : (i + 1 >= steps ? 0 : i + 1);
    p.ctr[1] = 0;
  }
}

}  // namespace

extern "C" int sdlt_sampler_step(const sdlt_sampler_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step: n=%d hw=%d", p->n, p->hw);
  if (p->table_rows < 3) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step: table_rows=%d (two header rows + at least one step)", p->table_rows);
  if (!p->x || !p->xin || !p->timesteps || !p->table || !p->ctr || (p->init ? !p->noise : !p->eps))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_sampler_step: null pointer (init=%d)", p->init);
  if (p->ld_xin < 4 || (p->ld_xin & 3) || ((uintptr_t)p->xin & 7)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step: xin needs 8-byte rows (ld=%lld)", (long long)p->ld_xin);
  if (!p->init && ((uintptr_t)p->eps & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_sampler_step: eps must be 16-byte aligned");
  const int blocks = (int)(((int64_t)p->n * p->hw + 255) / 256);
  hipLaunchKernelGGL(sampler_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
