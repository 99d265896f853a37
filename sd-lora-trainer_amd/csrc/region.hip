// sdlt_region_gather / sdlt_region_blend / sdlt_region_noise: the launches that regional prompts (MultiDiffusion section 4.2, "region-based text-to-image
// generation"; sampler.py: sample(regions=)) add to a denoising iteration.  The UNet runs the WHOLE H x W latent once per region, each with
// its own prompt, as ONE batch of 2 n R rows; the step launches, the guidance pre-pass and every buffer they touch stay at full size.  Region 0 is the
// background: the main prompt.
//   full-size rows   ((2 j + s) H + y) W + x                    image j, s = 0 negative | 1 positive: what the step launches read and write
//   region batch     b = 2 (j R + r) + s, pixel row (b H + y) W + x: the pairs stay adjacent, as UNet.forward and sdlt_guidance expect
//   gather   x_regions[b, y, x, 0 .. ld) = x_full[2 j + s, y, x, 0 .. ld)   whole bf16 model-input rows;  tf_regions[b] = tf_full[2 j + s]
//            bootstrap (rtab given, r >= 1, row i = ctr[0] of rtab has sigma_i >= 0, wraw[r, y, x] < 0.5): columns 0 .. 3 of the row, for both s, are
//            bf16((bg[j, r, c] + sigma_i * z_c) * inv_i) - t = sigma_i * z_c, u = bg + t, v = u * inv_i, one fp32 rounding each, then the conversion
//            sampler.hip's repack uses - so that a foreground region's object forms inside its mask: outside it the region sees a constant background
//            noised to the step's level.  Columns 4 and up are copied.  z = philox_normal4(pixel y W + x, i, r, REGION_TAG) under image j's seed
//            words: the noise depends on seed, step, region and pixel only, and the tag keeps it apart from the stochastic samplers' draws.
//            ctr is read, never written.  The branch on sigma_i < 0 is uniform over the launch: without bootstrap the launch is a pure copy.
//   blend    eps_full[2 j + s, y, x, 0 .. 4) = sum over r ascending of wn[r, y, x] * eps_regions[b, y, x, 0 .. 4): u = w * v rounded, acc = acc + u
//            from +0.0, plain operators under `fp contract(off)`, so a torch fp32 restatement gives the same bits (tests/region_ref.py: blend32).
// The blend is a GATHER: one thread per full-size row adds its R terms in a fixed order and stores once - no zeroing launch, no atomics, no dependence
// on launch order.  Both are pure bandwidth kernels.  gather: eight lanes per row, one 16-byte load and store each per 64 columns, so a wave moves
// eight consecutive rows = 1 KB contiguous on both sides.  blend: a workgroup is 64 x 4 full-size rows, the 64 lanes of a wave are 64 consecutive x of
// one y: its store is one 1 KB run, a region's loads one contiguous run of 16-byte rows and 256 bytes of weights.  Row offsets are 64-bit.  Vector
// stores only.  The tables are device memory (one captured graph serves every mask set, background and bootstrap length); whatever they hold, the
// kernels stay in bounds: the step row is clamped to the table's REGION_ROWS rows, and a weight, mask or seed value only changes what is computed.
#include "common.h"
#include "philox.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int RG_T = 256;               // gather: threads of a workgroup
constexpr int RG_LANES = 8;             // gather: lanes per row (16 bytes each per trip)
constexpr int RG_ROWS = RG_T / RG_LANES;
constexpr int RB_X = 64, RB_Y = 4;      // blend: workgroup = 64 x 4 full-size rows
constexpr int R_MAXR = 16;              // regions
constexpr int R_MAXDIM = 16384;         // H, W
constexpr int R_MAXN = 32767;           // images (grid.z = 2 n)
constexpr int R_MAXLD = 4096;           // bf16 elements of a model-input row
constexpr int64_t R_MAXROWS = (int64_t)1 << 40;   // rows of the region batch: with R_MAXLD every byte count below stays far inside 64 bits
constexpr int REGION_ROWS = SDLT_REGION_TABLE_ROWS;      // rows of rtab: one per step of the longest schedule

// The four channel normals of pixel `px` of an image with key (k0, k1) at step row `step` for region r.
__device__ __forceinline__ void region_noise4(uint32_t k0, uint32_t k1, uint32_t px, uint32_t step, uint32_t r, float z[4]) {
  philox_normal4(px, step, r, REGION_TAG, k0, k1, z);
}

// grid (ceil(H W / 32), R, 2 n)
template <bool BOOT>
__global__ __launch_bounds__(RG_T) void region_gather_kernel(sdlt_region_params a, const uint4* __restrict__ x_full, uint4* __restrict__ x_regions, int ld16,
                                                             const float* __restrict__ tf_full, float* __restrict__ tf_regions) {
  const int js = blockIdx.z, r = blockIdx.y;                     // js = 2 j + s; uniform
  const int j = js >> 1;
  const int64_t b = 2 * ((int64_t)j * a.R + r) + (js & 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) tf_regions[b] = tf_full[js];
  const uint32_t hw = (uint32_t)a.H * (uint32_t)a.W;
  const uint32_t px = blockIdx.x * (uint32_t)RG_ROWS + (threadIdx.x >> 3);
  if (px >= hw) return;
  const int lane = threadIdx.x & (RG_LANES - 1);
  const uint4* src = x_full + ((int64_t)js * hw + px) * ld16;
  uint4* dst = x_regions + (b * hw + px) * ld16;
  int c = lane;
  if (BOOT) {
    const int i = max(0, min(a.ctr[0], REGION_ROWS - 1));       // whatever the counter holds, the row is inside the table
    const float sigma = a.rtab[2 * i], inv = a.rtab[2 * i + 1];
    if (r >= 1 && sigma >= 0.f && lane == 0) {                  // (r and sigma: uniform over the launch's workgroup; lane 0 owns columns 0 .. 7)
      uint4 v = src[0];
      if (a.wraw[(int64_t)r * hw + px] < 0.5f) {
        const uint32_t k0 = a.seeds[2 * j], k1 = a.seeds[2 * j + 1];
        const float* bg = a.bg + ((int64_t)j * a.R + r) * 4;
        float z[4], o[4];
        region_noise4(k0, k1, px, (uint32_t)i, (uint32_t)r, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float t = sigma * z[k];
          const float u = bg[k] + t;
          o[k] = u * inv;
        }
        v.x = pack2bf(o[0], o[1]);
        v.y = pack2bf(o[2], o[3]);
      }
      dst[0] = v;
      c += RG_LANES;
    }
  }
  for (; c < ld16; c += RG_LANES) dst[c] = src[c];
}

// grid (ceil(W / 64), ceil(H / 4), 2 n)
__global__ __launch_bounds__(RB_X * RB_Y) void region_blend_kernel(sdlt_region_params a, const float* __restrict__ eps_regions, float* __restrict__ eps_full) {
  const int x = blockIdx.x * RB_X + (threadIdx.x & (RB_X - 1));
  const int y = blockIdx.y * RB_Y + (threadIdx.x >> 6);
  if (x >= a.W || y >= a.H) return;
  const int js = blockIdx.z;
  const int64_t hw = (int64_t)a.H * a.W, px = (int64_t)y * a.W + x;
  const float* e = eps_regions + ((2 * (int64_t)(js >> 1) * a.R + (js & 1)) * hw + px) * 4;      // region 0 of this pair's row; a region further: 2 hw rows
  const float* w = a.wn + px;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int r = 0; r < a.R; ++r) {
    const float t = w[(int64_t)r * hw];
    const f32x4 v = *(const f32x4*)(e + (int64_t)r * 2 * hw * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float u = t * v[c];
      acc[c] = acc[c] + u;
    }
  }
  f32x4 o;
  o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  *(f32x4*)(eps_full + ((int64_t)js * hw + px) * 4) = o;
}

__global__ __launch_bounds__(256) void region_noise_kernel(const uint32_t* seeds, int step, int region, int n, int hw, float* out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * hw) return;
  const int j = idx / hw, px = idx - j * hw;
  const uint32_t k0 = seeds[2 * j], k1 = seeds[2 * j + 1];
  float z[4];
  region_noise4(k0, k1, (uint32_t)px, (uint32_t)step, (uint32_t)region, z);
  float* o = out + (size_t)j * 4 * hw + px;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[(size_t)c * hw] = z[c];
}

// what both entry points refuse about the block's extents; `what` names the entry point
int region_check(const sdlt_region_params* p, const char* what) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", what);
  if (p->n < 1 || p->R < 1 || p->H < 1 || p->W < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d R=%d H=%d W=%d (every extent must be positive)", what, p->n, p->R, p->H, p->W);
  if (p->R > R_MAXR) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: R=%d regions (at most %d)", what, p->R, R_MAXR);
  if (p->H > R_MAXDIM || p->W > R_MAXDIM) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: H=%d W=%d (each at most %d)", what, p->H, p->W, R_MAXDIM);
  if (p->n > R_MAXN) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d images (at most %d)", what, p->n, R_MAXN);
  if (2 * (int64_t)p->n * p->R * p->H * p->W > R_MAXROWS)      // (at most 2^16 2^4 2^28: the product itself cannot overflow)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d with %d regions of %d x %d is more than 2^40 region rows", what, p->n, p->R, p->H, p->W);
  return SDLT_OK;
}

bool overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" int sdlt_region_gather(const sdlt_region_params* p, const void* x_full, void* x_regions, int64_t ld, const float* tf_full, float* tf_regions,
                                  void* stream) {
  const int rc = region_check(p, "sdlt_region_gather");
  if (rc != SDLT_OK) return rc;
  if (!x_full || !x_regions || !tf_full || !tf_regions) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_gather: null pointer");
  const int given = (p->wraw != nullptr) + (p->bg != nullptr) + (p->rtab != nullptr) + (p->ctr != nullptr) + (p->seeds != nullptr);
  if (given != 0 && given != 5)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_gather: bootstrap takes wraw, bg, rtab, ctr and seeds together (%d of 5 given; none: a pure copy)", given);
  if (ld < 8 || ld > R_MAXLD) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_gather: ld=%lld (8 .. %d bf16 elements per row)", (long long)ld, R_MAXLD);
  if (ld % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_gather: ld=%lld must be a multiple of 8 (16-byte row pieces)", (long long)ld);
  if (((uintptr_t)x_full | (uintptr_t)x_regions) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_gather: x_full and x_regions must be 16-byte aligned");
  if (((uintptr_t)tf_full | (uintptr_t)tf_regions) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_gather: tf_full and tf_regions must be 4-byte aligned");
  if (((uintptr_t)p->wraw | (uintptr_t)p->bg | (uintptr_t)p->rtab | (uintptr_t)p->ctr | (uintptr_t)p->seeds) & 3)
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_gather: wraw, bg, rtab, ctr and seeds must be 4-byte aligned");
  const int64_t full_rows = 2 * (int64_t)p->n * p->H * p->W, region_rows = full_rows * p->R;
  if (overlap(x_full, full_rows * ld * 2, x_regions, region_rows * ld * 2))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_gather: x_regions overlaps x_full (threads would read rows that other threads overwrite)");
  const int64_t chunks = ((int64_t)p->H * p->W + RG_ROWS - 1) / RG_ROWS;
  const dim3 grid((unsigned)chunks, (unsigned)p->R, (unsigned)(2 * p->n));
  if (given == 5)
    hipLaunchKernelGGL(region_gather_kernel<true>, grid, dim3(RG_T), 0, (hipStream_t)stream, *p, (const uint4*)x_full, (uint4*)x_regions, (int)(ld / 8),
                       tf_full, tf_regions);
  else
    hipLaunchKernelGGL(region_gather_kernel<false>, grid, dim3(RG_T), 0, (hipStream_t)stream, *p, (const uint4*)x_full, (uint4*)x_regions, (int)(ld / 8),
                       tf_full, tf_regions);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_region_blend(const sdlt_region_params* p, const float* eps_regions, float* eps_full, void* stream) {
  const int rc = region_check(p, "sdlt_region_blend");
  if (rc != SDLT_OK) return rc;
  if (!p->wn || !eps_regions || !eps_full) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_blend: null pointer");
  if (((uintptr_t)eps_regions | (uintptr_t)eps_full) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_blend: eps_regions and eps_full must be 16-byte aligned");
  if ((uintptr_t)p->wn & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_blend: wn must be 4-byte aligned");
  const int64_t full_rows = 2 * (int64_t)p->n * p->H * p->W, region_rows = full_rows * p->R;
  if (overlap(eps_regions, region_rows * 16, eps_full, full_rows * 16))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_blend: eps_full overlaps eps_regions (threads would read rows that other threads overwrite)");
  const dim3 grid((unsigned)((p->W + RB_X - 1) / RB_X), (unsigned)((p->H + RB_Y - 1) / RB_Y), (unsigned)(2 * p->n));
  hipLaunchKernelGGL(region_blend_kernel, grid, dim3(RB_X * RB_Y), 0, (hipStream_t)stream, *p, eps_regions, eps_full);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_region_noise(const uint32_t* seeds, int32_t step, int32_t region, int32_t n, int32_t hw, float* out, void* stream) {
  if (n < 1 || hw < 1 || (int64_t)n * hw > (1 << 28) || step < 0 || region < 0)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_noise: n=%d hw=%d step=%d region=%d", n, hw, step, region);
  if (!seeds || !out) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_region_noise: null pointer");
  if (((uintptr_t)seeds | (uintptr_t)out) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_region_noise: seeds and out must be 4-byte aligned");
  const int blocks = (int)(((int64_t)n * hw + 255) / 256);
  hipLaunchKernelGGL(region_noise_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, seeds, (int)step, (int)region, (int)n, (int)hw, out);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
