// sdlt_token_pool: the key / value rows of a self-attention whose keys are taken from a spatially downsampled copy of the tokens ("Token Downsampling",
// Smith et al. 2024; unet.py: UNet.set_kv_downsample).  y = pool_f(LayerNorm(x)) in one launch:
//   x      the block's residual stream, NHWC rows [B H W, ldx] bf16 (the rows norm1 reads)
//   y      [B Nkp, ldy] bf16: image b owns rows b Nkp .. b Nkp + Nkp - 1; the first Nk = Ho Wo of them are the pooled tokens (Ho = ceil(H / f),
//          Wo = ceil(W / f), row-major), the Nkp - Nk pad rows are written as zeros HERE (the attention forward loads them and masks their scores:
//          they have to be finite, and no fill launch sits in the replayed graph)
//   mode 0 nearest: output (oy, ox) is the normalised row (oy f, ox f) - the paper's method; only the sampled rows are read and normalised
//   mode 1 area:    the fp32 mean of the normalised rows of the in-image part of the window [oy f, oy f + f) x [ox f, ox f + f); an edge window is
//                   partial and divides by the rows it really has (avg_pool2d(ceil_mode=True, count_include_pad=False))
// The LayerNorm is fused because the mean does not commute with it; the k | v product then runs on normalised rows with the plain weights.
// One wave per OUTPUT row, four per workgroup; the lane layout and the statistics are ln_fwd_kernel's (norm.hip): lane l holds the 8-channel chunks
// l, l + 64, l + 128 of a row in registers (one 16-byte load each, every input row read once), mean and centred variance by the wave's xor butterfly in
// fp32.  The rows of a window are taken in (y, x) order and the next row's loads are issued before the current row's reductions.  fp32 throughout, one
// rounding to bf16 at the store; f == 1 gives sdlt_layernorm_fwd's bits in either mode (x / 1 and 0 + x are exact).  No atomics, no LDS, no order that
// depends on the data or the grid: the result repeats bit for bit.  Vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr int TP_MAXCH = 3;           // 8-channel chunks per lane: C <= 3 * 512 (the UNet's widths are 320, 640, 1280)

struct TokenPoolArgs {
  const bf16_t* x; int64_t ldx;
  bf16_t* y; int64_t ldy;
  const float* gamma; const float* beta;
  int B, H, W, C, f, mode, Ho, Wo, Nk, Nkp;
  float eps;
};

__device__ __forceinline__ void tp_load_row(const TokenPoolArgs& a, int64_t row, int lane, int nch, uint4* xr) {
#pragma unroll
  for (int i = 0; i < TP_MAXCH; ++i) {       // (unconditional, clamped to the row's last chunk: one round trip)
    const int ch = lane + i * 64, cc = ch < nch ? ch : nch - 1;
    xr[i] = *(const uint4*)(a.x + row * a.ldx + cc * 8);
  }
}

__global__ __launch_bounds__(256) void token_pool_kernel(TokenPoolArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t orow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (orow >= (int64_t)a.B * a.Nkp) return;
  const int img = (int)(orow / a.Nkp), o = (int)(orow - (int64_t)img * a.Nkp);
  const int nch = a.C >> 3;
  bf16_t* dst = a.y + orow * a.ldy;
  if (o >= a.Nk) {                           // a pad row
#pragma unroll
    for (int i = 0; i < TP_MAXCH; ++i) {
      const int ch = lane + i * 64;
      if (ch < nch) *(uint4*)(dst + ch * 8) = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const int oy = o / a.Wo, ox = o - oy * a.Wo;
  const int y0 = oy * a.f, x0 = ox * a.f;
  const int wy = a.mode == 0 ? 1 : min(a.f, a.H - y0), wx = a.mode == 0 ? 1 : min(a.f, a.W - x0);
  const int cnt = wy * wx;
  const int64_t base = ((int64_t)img * a.H + y0) * a.W + x0;       // the window's first input row; row (dy, dx) of it is base + dy W + dx
  f32x4 g4[TP_MAXCH][2], b4[TP_MAXCH][2];
#pragma unroll
  for (int i = 0; i < TP_MAXCH; ++i) {
    const int ch = lane + i * 64, cc = ch < nch ? ch : nch - 1;
    g4[i][0] = *(const f32x4*)(a.gamma + cc * 8); g4[i][1] = *(const f32x4*)(a.gamma + cc * 8 + 4);
    b4[i][0] = *(const f32x4*)(a.beta + cc * 8); b4[i][1] = *(const f32x4*)(a.beta + cc * 8 + 4);
  }
  float acc[TP_MAXCH][8];
#pragma unroll
  for (int i = 0; i < TP_MAXCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  uint4 xr[TP_MAXCH], xn[TP_MAXCH];
  tp_load_row(a, base, lane, nch, xr);
  for (int k = 0; k < cnt; ++k) {
    if (k + 1 < cnt) {                       // (wave-uniform) the next row of the window, in flight during this row's reductions
      const int dy = (k + 1) / wx, dx = (k + 1) - dy * wx;
      tp_load_row(a, base + (int64_t)dy * a.W + dx, lane, nch, xn);
    }
    float v[TP_MAXCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TP_MAXCH; ++i) {
      if (lane + i * 64 < nch) {
        const uint32_t w[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[i][2 * j] = bf2f(w[j] & 0xffff); v[i][2 * j + 1] = bf2f(w[j] >> 16); }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
      }
    }
    const float mean = wave_sum(s) / (float)a.C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < TP_MAXCH; ++i) {
      if (lane + i * 64 < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; q += d * d; }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)a.C + a.eps);
#pragma unroll
    for (int i = 0; i < TP_MAXCH; ++i) {
      if (lane + i * 64 < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] += (v[i][j] - mean) * rstd * g4[i][j >> 2][j & 3] + b4[i][j >> 2][j & 3];
      }
    }
#pragma unroll
    for (int i = 0; i < TP_MAXCH; ++i) xr[i] = xn[i];
  }
  const float fc = (float)cnt;
#pragma unroll
  for (int i = 0; i < TP_MAXCH; ++i) {
    const int ch = lane + i * 64;
    if (ch < nch) {
      float out[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = acc[i][j] / fc;
      store8(dst + ch * 8, out);
    }
  }
}

}  // namespace

extern "C" int sdlt_token_pool(const void* x, int64_t ldx, int32_t B, int32_t H, int32_t W, int32_t C, const float* gamma, const float* beta, float eps,
                               int32_t f, int32_t mode, void* y, int64_t ldy, int32_t Nkp, void* stream) {
  if (!x || !y || !gamma || !beta) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 8 || (C % 8) || C > TP_MAXCH * 512)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: B=%d H=%d W=%d C=%d (B, H, W >= 1; C a multiple of 8, 8 .. %d)", B, H, W, C, TP_MAXCH * 512);
  if (f < 1 || f > H || f > W) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: f=%d on a %d x %d grid (1 <= f <= H, W)", f, H, W);
  if (mode != 0 && mode != 1) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_token_pool: mode=%d (0 nearest, 1 area)", mode);
  const int Ho = (H + f - 1) / f, Wo = (W + f - 1) / f;
  const int64_t Nk = (int64_t)Ho * Wo;
  if (Nkp < Nk || (Nkp % 8)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: Nkp=%d (a multiple of 8, >= Nk = %d x %d = %lld)", Nkp, Ho, Wo, (long long)Nk);
  const int64_t rows_in = (int64_t)B * H * W, rows_out = (int64_t)B * Nkp;
  if (rows_in >= ((int64_t)1 << 31) || rows_out >= ((int64_t)1 << 31))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: %lld input rows, %lld output rows (< 2^31)", (long long)rows_in, (long long)rows_out);
  if (ldx < C || ldy < C) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: ldx=%lld ldy=%lld below the width C=%d", (long long)ldx, (long long)ldy, C);
  if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) || ((ldx | ldy) & 7))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_token_pool: x, y, gamma, beta must be 16-byte aligned and ldx, ldy multiples of 8");
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)((rows_in - 1) * ldx + C) * 2, y0 = (uintptr_t)y, y1 = y0 + (size_t)((rows_out - 1) * ldy + C) * 2;
  if (x0 < y1 && y0 < x1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_token_pool: y overlaps x (a wave reads rows that another's stores would overwrite)");
  TokenPoolArgs a;
  a.x = (const bf16_t*)x; a.ldx = ldx; a.y = (bf16_t*)y; a.ldy = ldy; a.gamma = gamma; a.beta = beta;
  a.B = B; a.H = H; a.W = W; a.C = C; a.f = f; a.mode = mode; a.Ho = Ho; a.Wo = Wo; a.Nk = (int)Nk; a.Nkp = Nkp; a.eps = eps;
  hipLaunchKernelGGL(token_pool_kernel, dim3((unsigned)((rows_out + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
