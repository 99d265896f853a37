// Per-token cross-attention heat maps of a render (render.py: `heatmap`), from the summed raw scores S = Q K^T / sqrt(d) that the hooked
// cross-attentions leave per resolution in Runtime.daam_sums (fp32 [B h_r w_r, ld], column = context position) - what the token-attention loss sees.
//
// sdlt_heatmap_accum: one launch per denoising iteration, between the UNet forward and the step launch.  For image i, map t, output pixel (y, x):
//     heat[i, t, y, x] += (w_step / sum_r L_r) * sum_r sum_p bicubic(S_r[block(i), :, cols[i, t, p]] as an h_r x w_r plane -> gh x gw)(y, x)
// with w_step = weights[ctr[0]] read on the device, block(i) = row_off + i row_stride the image's positive row block, and cols < 0 skipped.  The
// bicubic arithmetic is sdlt_resize_planes' (resample.h); a resolution whose grid is gh x gw is read as it is.  One thread per output element,
// consecutive threads consecutive x: the stores are contiguous, the loads are one float per tap from rows ld floats apart - a column walk, 16 cache
// lines per plane and thread, which the few hundred KB of a whole launch keep in L2.  It is latency, not a roofline: nothing tuned.
//
// sdlt_heatmap_overlay: once after the loop.  Launch 1 (one workgroup per image): min and max over the image's present maps in a fixed order, the maps
// normalised to [0, 1] (absent maps and a constant image: zeros).  Launch 2 (one thread per output pixel and map): the normalised map sampled
// bilinearly at the pixel (sdlt_resize_planes' mode 1), mapped through the 256-entry colour table with linear interpolation between entries and
// blended over the picture.  Plain C++, vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

#include "resample.h"

namespace {

using namespace resample;

constexpr int HT = 256;              // threads of a workgroup
constexpr int HMAX = 16384;          // largest size of an axis (resample.h's coordinate arithmetic)

__device__ __forceinline__ bool present(const int32_t* c, int P) {
  for (int p = 0; p < P; ++p)
    if (c[p] >= 0) return true;
  return false;
}

__global__ __launch_bounds__(HT) void heat_accum_kernel(sdlt_heatmap_accum_params p) {
  const uint32_t G = (uint32_t)p.gh * (uint32_t)p.gw;
  const uint32_t gid = blockIdx.x * (uint32_t)HT + threadIdx.x;       // n_img * T * G < 2^31 (checked by the entry point)
  if (gid >= (uint32_t)p.n_img * (uint32_t)p.T * G) return;
  const uint32_t it = gid / G, px = gid - it * G;
  const int i = (int)(it / (uint32_t)p.T);
  const int oy = (int)(px / (uint32_t)p.gw), ox = (int)(px - (uint32_t)oy * (uint32_t)p.gw);
  const int32_t* cols = p.cols + (size_t)it * p.P;
  if (!present(cols, p.P)) return;                                    // an absent token: its map stays as it is
  const int step = max(0, min(p.ctr[0], p.weight_rows - 1));
  int layers = 0;
  for (int r = 0; r < p.n_res; ++r) layers += p.layers[r];
  const float scale = p.weights[step] * (1.0f / (float)layers);
  const size_t block = (size_t)p.row_off + (size_t)i * p.row_stride;
  float total = 0.0f;
  for (int r = 0; r < p.n_res; ++r) {
    const int h = p.h[r], w = p.w[r];
    const float* src = p.sums[r] + block * (size_t)h * w * p.ld;      // the image's h w rows
    const bool same = h == p.gh && w == p.gw;
    Axis<4> ax, ay;
    if (!same) {
      axis_cubic(ox, w, p.gw, ax);
      axis_cubic(oy, h, p.gh, ay);
    }
    for (int q = 0; q < p.P; ++q) {
      const int c = min(cols[q], p.ld - 1);                           // (cols is device memory: a position past the row is held inside it, never read beyond)
      if (c < 0) continue;
      float v;
      if (same) {
        v = src[((size_t)oy * w + ox) * p.ld + c];
      } else {
        float hs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float* row = src + (size_t)ay.idx[k] * w * p.ld + c;
          hs[k] = combine<4>(row[(size_t)ax.idx[0] * p.ld], row[(size_t)ax.idx[1] * p.ld], row[(size_t)ax.idx[2] * p.ld], row[(size_t)ax.idx[3] * p.ld], ax.wt);
        }
        v = combine<4>(hs[0], hs[1], hs[2], hs[3], ay.wt);
      }
      total = total + v;
    }
  }
  p.heat[gid] = p.heat[gid] + scale * total;
}

// min / max of the image's present maps, then the maps normalised.  Thread j reads elements j, j + HT, ..; the partial results meet in a fixed tree
// (min and max do not depend on the order anyway).
__global__ __launch_bounds__(HT) void heat_norm_kernel(sdlt_heatmap_overlay_params p) {
  __shared__ float lo_s[HT], hi_s[HT];
  const int i = blockIdx.x, j = threadIdx.x;
  const uint32_t G = (uint32_t)p.gh * (uint32_t)p.gw;
  const float* heat = p.heat + (size_t)i * p.T * G;
  float* norm = p.norm + (size_t)i * p.T * G;
  const int32_t* cols = p.cols + (size_t)i * p.T * p.P;
  float lo = INFINITY, hi = -INFINITY;
  for (int t = 0; t < p.T; ++t) {
    if (!present(cols + (size_t)t * p.P, p.P)) continue;
    for (uint32_t e = j; e < G; e += HT) {
      const float v = heat[(size_t)t * G + e];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  lo_s[j] = lo;
  hi_s[j] = hi;
  __syncthreads();
  for (int o = HT / 2; o > 0; o >>= 1) {
    if (j < o) {
      lo_s[j] = fminf(lo_s[j], lo_s[j + o]);
      hi_s[j] = fmaxf(hi_s[j], hi_s[j + o]);
    }
    __syncthreads();
  }
  lo = lo_s[0];
  hi = hi_s[0];
  const float range = hi - lo;
  const bool flat = !(range > 0.0f);                                  // a constant image, no present map, or a non-finite value: zeros, no division
  for (int t = 0; t < p.T; ++t) {
    const bool here = !flat && present(cols + (size_t)t * p.P, p.P);
    for (uint32_t e = j; e < G; e += HT) norm[(size_t)t * G + e] = here ? (heat[(size_t)t * G + e] - lo) / range : 0.0f;
  }
}

__device__ __forceinline__ uint8_t to_u8(float v) {                    // [0, 255], to nearest (ties to even), clamped
  return (uint8_t)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

__global__ __launch_bounds__(HT) void heat_overlay_kernel(sdlt_heatmap_overlay_params p) {
  const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W, G = (uint32_t)p.gh * (uint32_t)p.gw;
  const uint32_t gid = blockIdx.x * (uint32_t)HT + threadIdx.x;       // n_img * T * HW < 2^31 (checked by the entry point)
  if (gid >= (uint32_t)p.n_img * (uint32_t)p.T * HW) return;
  const uint32_t it = gid / HW, px = gid - it * HW;
  const uint32_t i = it / (uint32_t)p.T;
  const int oy = (int)(px / (uint32_t)p.W), ox = (int)(px - (uint32_t)oy * (uint32_t)p.W);
  const float* img = p.image + (size_t)i * 3 * HW + px;
  uint8_t* out = p.out + (size_t)gid * 3;
  if (!present(p.cols + (size_t)it * p.P, p.P)) {                     // the untouched picture
    for (int c = 0; c < 3; ++c) out[c] = to_u8(img[(size_t)c * HW] * 255.0f);
    return;
  }
  Axis<2> ax, ay;
  axis_linear(ox, p.gw, p.W, ax);
  axis_linear(oy, p.gh, p.H, ay);
  const float* m = p.norm + (size_t)it * G;
  float hs[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float* row = m + (size_t)ay.idx[r] * p.gw;
    hs[r] = combine<2>(row[ax.idx[0]], row[ax.idx[1]], row[ax.idx[0]], row[ax.idx[1]], ax.wt);
  }
  float v = combine<2>(hs[0], hs[1], hs[0], hs[1], ay.wt);
  v = fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f;                           // position in the colour table
  const int k0 = min((int)v, 254);
  const float f = v - (float)k0;
  const uint8_t* c0 = p.lut + 3 * k0;
  const float keep = 1.0f - p.alpha;
  for (int c = 0; c < 3; ++c) {
    const float a = (float)c0[c], b = (float)c0[3 + c];
    const float colour = a + f * (b - a);
    out[c] = to_u8(keep * (img[(size_t)c * HW] * 255.0f) + p.alpha * colour);
  }
}

}  // namespace

extern "C" int sdlt_heatmap_accum(const sdlt_heatmap_accum_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: null parameter block");
  if (!p->cols || !p->ctr || !p->weights || !p->heat) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: null pointer");
  if (p->n_res < 1 || p->n_res > 4) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: n_res=%d (1 .. 4 resolutions)", p->n_res);
  if (p->n_img < 1 || p->T < 1 || p->P < 1 || p->gh < 1 || p->gw < 1 || p->gh > HMAX || p->gw > HMAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: n_img=%d T=%d P=%d gh=%d gw=%d (positive, the grid at most %d)", p->n_img, p->T, p->P, p->gh, p->gw, HMAX);
  if (p->row_off < 0 || p->row_stride < 1 || p->weight_rows < 1 || p->ld < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: row_off=%d row_stride=%d weight_rows=%d ld=%d", p->row_off, p->row_stride, p->weight_rows, p->ld);
  uintptr_t al = (uintptr_t)p->cols | (uintptr_t)p->ctr | (uintptr_t)p->weights | (uintptr_t)p->heat;
  for (int r = 0; r < p->n_res; ++r) {
    if (!p->sums[r]) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: sums[%d] is null", r);
    if (p->h[r] < 1 || p->w[r] < 1 || p->h[r] > HMAX || p->w[r] > HMAX || p->layers[r] < 1)
      SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: resolution %d: h=%d w=%d layers=%d", r, p->h[r], p->w[r], p->layers[r]);
    al |= (uintptr_t)p->sums[r];
  }
  if (al & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_heatmap_accum: pointers must be 4-byte aligned");
  const int64_t outs = (int64_t)p->n_img * p->T * p->gh * p->gw;
  if (outs >= ((int64_t)1 << 31)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_accum: %lld output elements (< 2^31)", (long long)outs);
  hipLaunchKernelGGL(heat_accum_kernel, dim3((unsigned)((outs + HT - 1) / HT)), dim3(HT), 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_heatmap_overlay(const sdlt_heatmap_overlay_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: null parameter block");
  if (!p->heat || !p->cols || !p->image || !p->lut || !p->norm || !p->out) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: null pointer");
  if (p->n_img < 1 || p->T < 1 || p->P < 1 || p->gh < 1 || p->gw < 1 || p->H < 1 || p->W < 1 || p->gh > HMAX || p->gw > HMAX || p->H > HMAX || p->W > HMAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: n_img=%d T=%d P=%d gh=%d gw=%d H=%d W=%d (positive, sizes at most %d)", p->n_img, p->T, p->P, p->gh, p->gw,
              p->H, p->W, HMAX);
  if (!(p->alpha >= 0.0f && p->alpha <= 1.0f)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: alpha=%g (0 .. 1)", (double)p->alpha);
  if (((uintptr_t)p->heat | (uintptr_t)p->cols | (uintptr_t)p->image | (uintptr_t)p->norm) & 3)
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_heatmap_overlay: heat, cols, image and norm must be 4-byte aligned");
  if (p->heat == p->norm) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: norm aliases heat (the minimum is read while the maps are written)");
  const int64_t outs = (int64_t)p->n_img * p->T * p->H * p->W;
  if (outs >= ((int64_t)1 << 31) || (int64_t)p->T * p->gh * p->gw >= ((int64_t)1 << 31))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_heatmap_overlay: %lld output pixels (< 2^31)", (long long)outs);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(heat_norm_kernel, dim3((unsigned)p->n_img), dim3(HT), 0, s, *p);
  hipLaunchKernelGGL(heat_overlay_kernel, dim3((unsigned)((outs + HT - 1) / HT)), dim3(HT), 0, s, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
