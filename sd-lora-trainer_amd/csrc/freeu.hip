// sdlt_freeu: FreeU (Si et al., CVPR 2024) on one (backbone, skip) pair of an up-block resnet, issued just before the resnet reads them
// (unet.py: UNet._forward with set_freeu).  Activations are NHWC rows - h bf16 [B HW, C1], skip bf16 [B HW, C2] - and stay that way.
//   skip filter     the published fftn -> fftshift -> mask[crow-1:crow+1, ccol-1:ccol+1] = s -> ifftn(.).real with threshold 1 scales FOUR bins of every
//                   plane: (0, 0), (-1, 0), (0, -1), (-1, -1) of the unshifted spectrum.  Their inverse transform's real part is, with ty = 2 pi y / H,
//                   tx = 2 pi x / W,
//                     L[y, x] = (S0 + Ay cos ty + By sin ty + Ax cos tx + Bx sin tx + Axy cos(ty + tx) + Bxy sin(ty + tx)) / (H W)
//                     S0 = sum v ;  A. = sum v cos(.) ;  B. = sum v sin(.)            seven real weighted column sums per (image, channel)
//                   and the result is skip' = skip + (s - 1) L.  No FFT, no NCHW copy.
//   backbone scale  version 1: h'[:, c] = b h[:, c] for c < C1 / 2.  version 2: m[p] = fp32 mean of h[p, :] over the C1 channels, lo / hi its min / max over
//                   the image's pixels, n = (m - lo) / (hi - lo) (n = 0 where hi == lo), h'[p, c] = h ((b - 1) n + 1) for c < C1 / 2.  Other channels: copied.
// Two launches on the stream, nothing else:
//   1 reduce   an image's HW rows are cut into nchunk <= 16 chunks of R rows (R = ceil(HW / 16) rounded up to a multiple of 32: a function of HW alone);
//              a workgroup owns a chunk x 64-channel tile: lane (rl = t / 8, cl = t % 8) walks rows rl, rl + 32, ... of the chunk with one 16-byte load
//              (8 channels) per row, keeps 7 x 8 fp32 sums, and the 32 row lanes meet by the wave's xor butterfly, then the four waves in ascending order in
//              LDS: 7 x 64 partials go to the workspace.  Version 2: one more workgroup per chunk takes the row means of h (a wave per row, lanes over
//              8-channel groups, the wave's butterfly) and the chunk's min / max of them.
//   2 apply    the same tiling.  A skip workgroup first adds the <= 16 chunk partials of its 64 channels in ascending chunk order (7 x 64 sums from L2 -
//              about as many bytes as the tile itself), then rewrites its rows; an h workgroup takes min / max over the chunk pairs and scales.  16-byte
//              stores.
// No atomics, no hand-off inside a launch, no data-dependent order: image j's result depends on neither B nor j, and repeats bit for bit.  fp32 arithmetic,
// one rounding to bf16 at the store.  s == 1 stores the skip's bits, b == 1 (and every channel >= C1 / 2) the backbone's bits, untouched - x + 0 L would
// turn -0 into +0.  The cos / sin tables come from the host (fp64, rounded once); the (ty + tx) terms by the angle-sum identities.  Vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr int FT = 256;             // threads of a workgroup
constexpr int FCL = 8;              // column lanes: 8 x 8 channels = the 64-channel tile
constexpr int FRL = FT / FCL;       // 32 row lanes
constexpr int FTC = FCL * 8;        // channels of a tile
constexpr int FMAXCH = 16;          // most chunks of an image
constexpr int FK = 7;               // S0, Ay, By, Ax, Bx, Axy, Bxy

struct FreeuArgs {
  const bf16_t* h; const bf16_t* skip; bf16_t* h_out; bf16_t* skip_out;
  int64_t ld_h, ld_s, ld_ho, ld_so;
  const float* ty; const float* tx;       // [2, H] and [2, W]: the cos row, then the sin row
  float* part;                            // [B, nchunk, 7, C2]
  float* mean;                            // [B, HW]            (version 2)
  float* mm;                              // [B, nchunk, 2]     (version 2: min, max of the chunk's row means)
  int B, H, W, HW, C1, C2, R, nchunk, ct1, ct2, version;
  float b, s;
};

__host__ __device__ inline int freeu_chunk_rows(int HW) {
  const int r = (HW + FMAXCH - 1) / FMAXCH;
  return (r + 31) / 32 * 32;
}

// the seven weights of pixel p of an image: 1, cos ty, sin ty, cos tx, sin tx, cos(ty + tx), sin(ty + tx)
__device__ __forceinline__ void freeu_weights(const FreeuArgs& a, int p, float* w) {
  const int y = p / a.W, x = p - y * a.W;
  const float cy = a.ty[y], sy = a.ty[a.H + y], cx = a.tx[x], sx = a.tx[a.W + x];
  w[0] = 1.0f; w[1] = cy; w[2] = sy; w[3] = cx; w[4] = sx;
  w[5] = cy * cx - sy * sx;
  w[6] = sy * cx + cy * sx;
}

__device__ void freeu_reduce_skip(const FreeuArgs& a, int blk, float (*sm)[FK][FTC]) {
  const int tile = blk % a.ct2, chunk = (blk / a.ct2) % a.nchunk, img = blk / (a.ct2 * a.nchunk);
  const int t = threadIdx.x, rl = t / FCL, cl = t % FCL, c = tile * FTC + cl * 8;
  const int p1 = min((chunk + 1) * a.R, a.HW);
  float acc[FK][8];
#pragma unroll
  for (int k = 0; k < FK; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.0f;
  if (c < a.C2) {
    for (int p = chunk * a.R + rl; p < p1; p += FRL) {
      float v[8], w[FK];
      load8(a.skip + ((size_t)img * a.HW + p) * a.ld_s + c, v);
      freeu_weights(a, p, w);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[0][e] += v[e];
#pragma unroll
      for (int k = 1; k < FK; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] += v[e] * w[k];
    }
  }
  // the 8 row lanes of a wave (lane bits 3..5), then the 4 waves in ascending order
#pragma unroll
  for (int k = 0; k < FK; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = acc[k][e];
      x += __shfl_xor(x, 8, 64);
      x += __shfl_xor(x, 16, 64);
      x += __shfl_xor(x, 32, 64);
      acc[k][e] = x;
    }
  if ((t & 63) < FCL) {
#pragma unroll
    for (int k = 0; k < FK; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[t >> 6][k][cl * 8 + e] = acc[k][e];
  }
  __syncthreads();
  for (int o = t; o < FK * FTC; o += FT) {
    const int k = o / FTC, ch = o % FTC;
    if (tile * FTC + ch < a.C2) {
      float x = sm[0][k][ch];
      x += sm[1][k][ch];
      x += sm[2][k][ch];
      x += sm[3][k][ch];
      a.part[(((size_t)img * a.nchunk + chunk) * FK + k) * a.C2 + tile * FTC + ch] = x;
    }
  }
}

__device__ void freeu_reduce_mean(const FreeuArgs& a, int blk, float (*red)[4]) {
  const int chunk = blk % a.nchunk, img = blk / a.nchunk;
  const int t = threadIdx.x, wv = t >> 6, ln = t & 63;
  const int p1 = min((chunk + 1) * a.R, a.HW);
  float lo = INFINITY, hi = -INFINITY;
  for (int p = chunk * a.R + wv; p < p1; p += 4) {
    const bf16_t* row = a.h + ((size_t)img * a.HW + p) * a.ld_h;
    float sum = 0.0f;
    for (int c = ln * 8; c < a.C1; c += 64 * 8) {
      float v[8];
      load8(row + c, v);
      sum += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    const float m = wave_sum(sum) / (float)a.C1;
    if (ln == 0) a.mean[(size_t)img * a.HW + p] = m;
    lo = fminf(lo, m);
    hi = fmaxf(hi, m);
  }
  if (ln == 0) {
    red[0][wv] = lo;
    red[1][wv] = hi;
  }
  __syncthreads();
  if (t == 0) {
    float* o = a.mm + ((size_t)img * a.nchunk + chunk) * 2;
    o[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    o[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__global__ __launch_bounds__(FT) void freeu_reduce_kernel(FreeuArgs a) {
  __shared__ float sm[4][FK][FTC];
  __shared__ float red[2][4];
  const int nskip = a.B * a.nchunk * a.ct2;
  if ((int)blockIdx.x < nskip) freeu_reduce_skip(a, blockIdx.x, sm);
  else freeu_reduce_mean(a, blockIdx.x - nskip, red);
}

__device__ void freeu_apply_skip(const FreeuArgs& a, int blk, float (*tot)[FTC]) {
  const int tile = blk % a.ct2, chunk = (blk / a.ct2) % a.nchunk, img = blk / (a.ct2 * a.nchunk);
  const int t = threadIdx.x, rl = t / FCL, cl = t % FCL, c = tile * FTC + cl * 8;
  const int p1 = min((chunk + 1) * a.R, a.HW);
  const bool filter = a.s != 1.0f;
  if (filter) {
    for (int o = t; o < FK * FTC; o += FT) {
      const int k = o / FTC, ch = o % FTC;
      float x = 0.0f;
      if (tile * FTC + ch < a.C2) {
        const float* src = a.part + ((size_t)img * a.nchunk * FK + k) * a.C2 + tile * FTC + ch;
        for (int q = 0; q < a.nchunk; ++q) x += src[(size_t)q * FK * a.C2];
      }
      tot[k][ch] = x;
    }
    __syncthreads();
  }
  if (c >= a.C2) return;
  float T[FK][8];
  if (filter) {
#pragma unroll
    for (int k = 0; k < FK; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) T[k][e] = tot[k][cl * 8 + e];
  }
  const float g = a.s - 1.0f, hw = (float)a.HW;
  for (int p = chunk * a.R + rl; p < p1; p += FRL) {
    const size_t row = (size_t)img * a.HW + p;
    const bf16_t* src = a.skip + row * a.ld_s + c;
    bf16_t* dst = a.skip_out + row * a.ld_so + c;
    if (!filter) {
      *(uint4*)dst = *(const uint4*)src;
      continue;
    }
    float v[8], w[FK];
    load8(src, v);
    freeu_weights(a, p, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float L = T[0][e];
#pragma unroll
      for (int k = 1; k < FK; ++k) L += T[k][e] * w[k];
      v[e] = v[e] + g * (L / hw);
    }
    store8(dst, v);
  }
}

__device__ void freeu_apply_h(const FreeuArgs& a, int blk) {
  const int tile = blk % a.ct1, chunk = (blk / a.ct1) % a.nchunk, img = blk / (a.ct1 * a.nchunk);
  const int t = threadIdx.x, rl = t / FCL, cl = t % FCL, c = tile * FTC + cl * 8;
  if (c >= a.C1) return;
  const int p1 = min((chunk + 1) * a.R, a.HW), half = a.C1 / 2;
  const bool scale = a.b != 1.0f && c < half;
  float lo = 0.0f, span = 0.0f;
  if (scale && a.version == 2) {
    float hi = -INFINITY;
    lo = INFINITY;
    const float* mm = a.mm + (size_t)img * a.nchunk * 2;
    for (int q = 0; q < a.nchunk; ++q) {
      lo = fminf(lo, mm[2 * q]);
      hi = fmaxf(hi, mm[2 * q + 1]);
    }
    span = hi - lo;
  }
  for (int p = chunk * a.R + rl; p < p1; p += FRL) {
    const size_t row = (size_t)img * a.HW + p;
    const bf16_t* src = a.h + row * a.ld_h + c;
    bf16_t* dst = a.h_out + row * a.ld_ho + c;
    if (!scale) {
      *(uint4*)dst = *(const uint4*)src;
      continue;
    }
    float f = a.b;
    if (a.version == 2) {
      const float n = span == 0.0f ? 0.0f : (a.mean[row] - lo) / span;
      f = (a.b - 1.0f) * n + 1.0f;
    }
    const uint4 raw = *(const uint4*)src;
    float v[8];
    load8(src, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c + e < half ? v[e] * f : v[e];
    store8(dst, v);
    if (c + 8 > half) {                       // the group that straddles C1 / 2 (C1 = 8 (2 k + 1)): its upper channels keep their bits
      const bf16_t* r16 = (const bf16_t*)&raw;
      for (int e = half - c; e < 8; ++e) dst[e] = r16[e];
    }
  }
}

__global__ __launch_bounds__(FT) void freeu_apply_kernel(FreeuArgs a) {
  __shared__ float tot[FK][FTC];
  const int nskip = a.B * a.nchunk * a.ct2;
  if ((int)blockIdx.x < nskip) freeu_apply_skip(a, blockIdx.x, tot);
  else freeu_apply_h(a, blockIdx.x - nskip);
}

bool freeu_overlap(const void* p, int64_t ld, int C, const void* q, int64_t ldq, int Cq, int64_t rows) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + (size_t)((rows - 1) * ld + C) * 2;
  const uintptr_t b0 = (uintptr_t)q, b1 = b0 + (size_t)((rows - 1) * ldq + Cq) * 2;
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int64_t sdlt_freeu_ws_floats(int32_t B, int32_t H, int32_t W, int32_t C1, int32_t C2) {
  if (B < 1 || H < 2 || W < 2 || C1 < 8 || C2 < 8 || (int64_t)B * H * W >= ((int64_t)1 << 31))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu_ws_floats: B=%d H=%d W=%d C1=%d C2=%d (B >= 1, H, W >= 2, C >= 8, B H W < 2^31)", B, H, W, C1, C2);
  const int64_t HW = (int64_t)H * W;
  const int64_t nchunk = (HW + freeu_chunk_rows((int)HW) - 1) / freeu_chunk_rows((int)HW);
  return (int64_t)B * nchunk * FK * C2 + (int64_t)B * HW + (int64_t)B * nchunk * 2;
}

extern "C" int sdlt_freeu(const void* h, int64_t ld_h, const void* skip, int64_t ld_s, void* h_out, int64_t ld_ho, void* skip_out, int64_t ld_so,
                          int32_t B, int32_t H, int32_t W, int32_t C1, int32_t C2, float b, float s, int32_t version,
                          const float* tab_y, const float* tab_x, float* ws, int64_t ws_floats, void* stream) {
  if (!h || !skip || !h_out || !skip_out || !tab_y || !tab_x || !ws) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: null pointer");
  if (B < 1 || H < 2 || W < 2)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: B=%d H=%d W=%d (B >= 1; H, W >= 2: the published mask slice is empty on an axis of size 1)", B, H, W);
  if (C1 < 8 || C2 < 8 || C1 % 8 != 0 || C2 % 8 != 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: C1=%d C2=%d (positive multiples of 8)", C1, C2);
  if (version != 1 && version != 2) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_freeu: version=%d (1 or 2)", version);
  const int64_t rows = (int64_t)B * H * W;
  if (rows >= ((int64_t)1 << 31)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: %lld rows (< 2^31)", (long long)rows);
  if (ld_h < C1 || ld_ho < C1 || ld_s < C2 || ld_so < C2)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: leading dimensions %lld %lld %lld %lld below the widths C1=%d C2=%d", (long long)ld_h, (long long)ld_s,
              (long long)ld_ho, (long long)ld_so, C1, C2);
  if ((((uintptr_t)h | (uintptr_t)skip | (uintptr_t)h_out | (uintptr_t)skip_out) & 15) || ((ld_h | ld_s | ld_ho | ld_so) & 7))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_freeu: h, skip, h_out, skip_out must be 16-byte aligned and their leading dimensions multiples of 8");
  if (((uintptr_t)tab_y | (uintptr_t)tab_x | (uintptr_t)ws) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_freeu: tab_y, tab_x, ws must be 4-byte aligned");
  if (freeu_overlap(h_out, ld_ho, C1, h, ld_h, C1, rows) || freeu_overlap(h_out, ld_ho, C1, skip, ld_s, C2, rows) ||
      freeu_overlap(skip_out, ld_so, C2, h, ld_h, C1, rows) || freeu_overlap(skip_out, ld_so, C2, skip, ld_s, C2, rows) ||
      freeu_overlap(h_out, ld_ho, C1, skip_out, ld_so, C2, rows))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: an output overlaps an input or the other output (a workgroup reads rows that another's stores would overwrite)");
  const int64_t need = sdlt_freeu_ws_floats(B, H, W, C1, C2);
  if (ws_floats < need) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: workspace of %lld floats, %lld needed (sdlt_freeu_ws_floats)", (long long)ws_floats, (long long)need);
  FreeuArgs a;
  a.h = (const bf16_t*)h; a.skip = (const bf16_t*)skip; a.h_out = (bf16_t*)h_out; a.skip_out = (bf16_t*)skip_out;
  a.ld_h = ld_h; a.ld_s = ld_s; a.ld_ho = ld_ho; a.ld_so = ld_so;
  a.ty = tab_y; a.tx = tab_x;
  a.B = B; a.H = H; a.W = W; a.HW = H * W; a.C1 = C1; a.C2 = C2;
  a.R = freeu_chunk_rows(a.HW);
  a.nchunk = (a.HW + a.R - 1) / a.R;
  a.ct1 = (C1 + FTC - 1) / FTC; a.ct2 = (C2 + FTC - 1) / FTC;
  a.version = version; a.b = b; a.s = s;
  a.part = ws;
  a.mean = a.part + (size_t)B * a.nchunk * FK * C2;
  a.mm = a.mean + (size_t)B * a.HW;
  const int64_t nskip = (int64_t)B * a.nchunk * a.ct2, nh = (int64_t)B * a.nchunk * a.ct1;
  const bool want_mean = version == 2 && b != 1.0f;
  const int64_t g1 = (s != 1.0f ? nskip : 0) + (want_mean ? (int64_t)B * a.nchunk : 0);
  if (nskip + nh >= ((int64_t)1 << 31)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_freeu: %lld workgroups (< 2^31)", (long long)(nskip + nh));
  hipStream_t st = (hipStream_t)stream;
  if (g1 > 0) {
    FreeuArgs r = a;
    if (s == 1.0f) r.ct2 = 0;                    // no skip workgroups: the grid is the mean workgroups alone
    hipLaunchKernelGGL(freeu_reduce_kernel, dim3((unsigned)g1), dim3(FT), 0, st, r);
    SDLT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(freeu_apply_kernel, dim3((unsigned)(nskip + nh)), dim3(FT), 0, st, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
