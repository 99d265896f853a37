// sdlt_resize_planes: `planes` fp32 images [planes, h, w] resampled to [planes, H, W] - the piece between the two passes of a hires render
// (render.py: the first pass's latents [n, 4, h, w] enlarged in latent space, or the decoder's image [n, 3, 8h, 8w] enlarged in pixel space).
// The modes are PyTorch's align_corners=False conventions (what a user's other tools compute):
//   0 nearest-exact   source index min(floor(((2 d + 1) in) / (2 out)), in - 1), integer arithmetic: no float ties
//   1 bilinear        c = max((d + 0.5) s - 0.5, 0); i0 = floor(c), i1 = min(i0 + 1, in - 1); t = c - i0; weights (1 - t, t)
//   2 bicubic         c = (d + 0.5) s - 0.5 (not clamped); i = floor(c), t = c - i; taps i - 1 .. i + 2, each index clamped to [0, in - 1];
//                     weights: the Keys kernel with A = -0.75 at the distances t + 1, t, 1 - t, (1 - t) + 1, summed about tap i
// with s = in / out ONE fp32 division of the two sizes converted to fp32.  All arithmetic is fp32, one rounding per operation (no contraction),
// in the order include/sdlt_kernels.h writes down: per axis the coordinate, the fraction and the weights; then per output pixel the horizontal sums
// of the source rows it reads (taps left to right), then the vertical sum of those (rows top to bottom).  tests/hires_ref.py restates it in NumPy
// float32 and the GPU tests compare bits.
// One thread per output pixel of an IMAGE (planes_per_image planes that share h, w: the 4 latent channels, the 3 colours): the two axes' indices and
// weights are computed once and reused for every plane of the image.  Consecutive threads are consecutive x of one output row, so the stores of a
// wave are contiguous along W; the loads are 1, 4 or 16 per plane from 1, 2 or 4 source rows.  A launch moves a few hundred KB: it is latency, not
// a roofline - no LDS, no vector loads, nothing tuned.  Vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

#include "resample.h"

namespace {

using namespace resample;

constexpr int RT = 256;              // threads of a workgroup = output pixels of a workgroup
constexpr int RMAX = 16384;          // largest size of an axis: (2 d + 1) in < 2^30 in 32-bit arithmetic

template <int TAPS>
__global__ __launch_bounds__(RT) void resize_kernel(sdlt_resize_params p) {
  const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W;
  const uint32_t images = (uint32_t)(p.planes / p.planes_per_image);
  const uint32_t gid = blockIdx.x * (uint32_t)RT + threadIdx.x;       // images * HW < 2^31 (checked by the entry point)
  if (gid >= images * HW) return;
  const uint32_t img = gid / HW, px = gid - img * HW;
  const int oy = (int)(px / (uint32_t)p.W), ox = (int)(px - (uint32_t)oy * (uint32_t)p.W);
  Axis<TAPS> ax, ay;
  axis<TAPS>(ox, p.w, p.W, ax);
  axis<TAPS>(oy, p.h, p.H, ay);
  const size_t hw = (size_t)p.h * p.w;
  const float* src = p.in + (size_t)img * p.planes_per_image * hw;
  float* dst = p.out + (size_t)img * p.planes_per_image * HW + px;
  for (int c = 0; c < p.planes_per_image; ++c, src += hw, dst += HW) {
    if constexpr (TAPS == 1) {
      *dst = src[(size_t)ay.idx[0] * p.w + ax.idx[0]];
    } else {
      float hs[TAPS];
#pragma unroll
      for (int r = 0; r < TAPS; ++r) {
        const float* row = src + (size_t)ay.idx[r] * p.w;
        hs[r] = combine<TAPS>(row[ax.idx[0]], row[ax.idx[1]], row[ax.idx[TAPS - 2]], row[ax.idx[TAPS - 1]], ax.wt);
      }
      *dst = combine<TAPS>(hs[0], hs[1], hs[TAPS - 2], hs[TAPS - 1], ay.wt);
    }
  }
}

}  // namespace

extern "C" int sdlt_resize_planes(const sdlt_resize_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: null parameter block");
  if (!p->in || !p->out) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: null pointer");
  if (p->planes < 1 || p->planes_per_image < 1 || p->planes % p->planes_per_image != 0)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: planes=%d planes_per_image=%d (positive, planes a multiple of planes_per_image)", p->planes, p->planes_per_image);
  if (p->h < 1 || p->w < 1 || p->H < 1 || p->W < 1 || p->h > RMAX || p->w > RMAX || p->H > RMAX || p->W > RMAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: h=%d w=%d H=%d W=%d (each in 1 .. %d)", p->h, p->w, p->H, p->W, RMAX);
  if (p->mode < 0 || p->mode > 2) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_resize_planes: mode=%d (0 nearest-exact, 1 bilinear, 2 bicubic)", p->mode);
  const int64_t pixels = (int64_t)(p->planes / p->planes_per_image) * p->H * p->W;
  if (pixels >= ((int64_t)1 << 31)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: %lld output pixels per plane set (< 2^31)", (long long)pixels);
  if (((uintptr_t)p->in | (uintptr_t)p->out) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_resize_planes: in and out must be 4-byte aligned");
  const uintptr_t a0 = (uintptr_t)p->in, a1 = a0 + (size_t)p->planes * p->h * p->w * sizeof(float);
  const uintptr_t b0 = (uintptr_t)p->out, b1 = b0 + (size_t)p->planes * p->H * p->W * sizeof(float);
  if (a0 < b1 && b0 < a1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_resize_planes: out aliases in (a thread reads source pixels that other threads' outputs would overwrite)");
  const dim3 grid((unsigned)((pixels + RT - 1) / RT));
  hipStream_t s = (hipStream_t)stream;
  if (p->mode == 0) hipLaunchKernelGGL(resize_kernel<1>, grid, dim3(RT), 0, s, *p);
  else if (p->mode == 1) hipLaunchKernelGGL(resize_kernel<2>, grid, dim3(RT), 0, s, *p);
  else hipLaunchKernelGGL(resize_kernel<4>, grid, dim3(RT), 0, s, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
