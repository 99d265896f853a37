// sdlt_tile_blend: one tile of a tiled VAE decode / encode placed into the whole picture with its feather weights (vae.py: VaeDecoder.decode_tiled,
// VaeEncoder.encode_moments_tiled):
//   out[c, y0 + p, x0 + q] += (wy[p] * wx[q]) * tile[(p tw + q) ld + c]          c < C, p < th, q < tw
//   tile   fp32 NHWC rows [th tw, ld]: the decoder's img buffer (ld = 4, C = 3) or the encoder's moment rows (ld = C = 8), as the last conv left them
//   out    fp32 planar [C, H, W], contiguous; zeroed once by the caller, then one launch per tile in row-major tile order on one stream
//   wy, wx the tile's NORMALISED 1-D weight tables (vae.tile_weights): over the tiles that cover an output sample the products wy wx sum to 1
// Arithmetic, fixed so that a torch fp32 restatement gives the same bits (tests/vaetile_ref.py: blend32): t = wy[p] * wx[q] rounded, then t * v rounded,
// then out + that rounded - three fp32 operations, no contraction: plain operators under `fp contract(off)` like resize.hip and sampler.hip (the
// __fmul_rn / __fadd_rn of the HIP headers are plain operators compiled with the headers' own contraction setting, and hipcc fused a pair of them into
// one v_fma here).  No atomics: a sample is touched by one thread of one launch at a time, and the
// launches of a picture are ordered by the stream, so the result repeats bit for bit.
// A pure bandwidth kernel.  One thread per output (p, q); a workgroup is 64 x 4 of them, so the 64 lanes of a wave are 64 consecutive x of one row:
// every plane access of a wave is one contiguous 256-byte run (read and write: out is accumulated), and the wave's tile reads are 64 consecutive
// rows - one 16-byte load per lane and 4 channels where the rows are 16-byte aligned (ld % 4 == 0 and an aligned base: 1 KB per instruction), scalar
// loads of the C channels otherwise (ld = 3: the unaligned row path).  Plane offsets are 64-bit.  Vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB_X = 64, TB_Y = 4;      // workgroup = 64 x 4 output samples
constexpr int TB_MAXC = 16;             // planes per launch (3 colours, 8 moments; the loop below is bounded by it)
constexpr int TB_MAXDIM = 1 << 20;      // largest extent of an axis of out (a tile lies inside it): y0 + p and x0 + q stay far inside 32 bits

struct TileBlendArgs {
  const float* tile; int64_t ld;
  const float* wy; const float* wx;
  float* out;
  int th, tw, C, H, W, y0, x0;
};

template <bool VEC>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_blend_kernel(TileBlendArgs a) {
  const int q = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1));
  const int p = blockIdx.y * TB_Y + (threadIdx.x >> 6);
  if (q >= a.tw || p >= a.th) return;
  const float t = a.wy[p] * a.wx[q];
  const float* row = a.tile + ((int64_t)p * a.tw + q) * a.ld;
  const int64_t HW = (int64_t)a.H * a.W;
  float* dst = a.out + (int64_t)(a.y0 + p) * a.W + (a.x0 + q);
  for (int c0 = 0; c0 < a.C; c0 += 4, dst += 4 * HW) {
    float v[4];
    if constexpr (VEC) {                  // c0 + 3 < ld: ld is a multiple of 4 and c0 < C <= ld
      const f32x4 r = *(const f32x4*)(row + c0);
      v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < a.C ? row[c0 + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c0 + j < a.C) {
        float* o = dst + j * HW;
        const float u = t * v[j];
        *o = *o + u;
      }
    }
  }
}

}  // namespace

extern "C" int sdlt_tile_blend(const float* tile, int64_t ld, int32_t th, int32_t tw, int32_t C, const float* wy, const float* wx,
                               float* out, int32_t H, int32_t W, int32_t y0, int32_t x0, void* stream) {
  if (!tile || !wy || !wx || !out) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: null pointer");
  if (th < 1 || tw < 1 || H < 1 || W < 1 || C < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: th=%d tw=%d C=%d H=%d W=%d (every extent must be positive)", th, tw, C, H, W);
  if (H > TB_MAXDIM || W > TB_MAXDIM) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: H=%d W=%d (each at most %d)", H, W, TB_MAXDIM);
  if (C > TB_MAXC) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: C=%d planes (at most %d)", C, TB_MAXC);
  if (ld < C) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: ld=%lld below the channel count C=%d", (long long)ld, C);
  if (y0 < 0 || x0 < 0 || (int64_t)y0 + th > H || (int64_t)x0 + tw > W)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: a %d x %d tile at (y0=%d, x0=%d) reaches outside the %d x %d output", th, tw, y0, x0, H, W);
  if (((uintptr_t)tile | (uintptr_t)wy | (uintptr_t)wx | (uintptr_t)out) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_tile_blend: tile, wy, wx and out must be 4-byte aligned");
  const bool vec = (ld % 4 == 0) && (((uintptr_t)tile & 15) == 0);
  const int64_t rows = (int64_t)th * tw;
  const uintptr_t a0 = (uintptr_t)tile, a1 = a0 + (size_t)((rows - 1) * ld + (vec ? ld : (int64_t)C)) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)C * H * W * sizeof(float);
  if (a0 < b1 && b0 < a1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: out overlaps tile (threads would read rows that other threads' sums overwrite)");
  TileBlendArgs a;
  a.tile = tile; a.ld = ld; a.wy = wy; a.wx = wx; a.out = out;
  a.th = th; a.tw = tw; a.C = C; a.H = H; a.W = W; a.y0 = y0; a.x0 = x0;
  const dim3 grid((unsigned)((tw + TB_X - 1) / TB_X), (unsigned)((th + TB_Y - 1) / TB_Y));
  if (grid.y > 65535u) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_tile_blend: th=%d (at most %d rows per tile)", th, 65535 * TB_Y);
  hipStream_t s = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(tile_blend_kernel<true>, grid, dim3(TB_X * TB_Y), 0, s, a);
  else hipLaunchKernelGGL(tile_blend_kernel<false>, grid, dim3(TB_X * TB_Y), 0, s, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
