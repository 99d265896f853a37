// Self-attention guidance (SAG, Hong et al. 2023) on gfx950: the three launches a render adds between its two UNet forwards.  include/sdlt_kernels.h has the
// contracts, DESIGN 4.41 the compiler's resource figures.
//
// sdlt_attn_colmass - the attention MASS a key receives:  m[k] = (1 / H) sum over heads h and queries q of softmax_k(scale Q_h[q] . K_h[k])[q, k],
// from Q, K and the log-sum-exp L that sdlt_attn_fwd left (natural log of sum_k exp(scale s)), so p = exp(scale s - L[q]) needs no second softmax pass
// and no [N, N] buffer.  The flash kernels are query-major (a lane owns a query row and sums over keys); this one is KEY-major:
//   * one workgroup of four waves per (block of 64 keys, head, image); wave w owns keys [16 w, 16 w + 16) of the block and keeps their K head slice in
//     registers for the whole walk, as the A operands of the 16x16x32 MFMA (lane (g, i): key i, 8 columns from 8 g of each 32-wide step; zero beyond d);
//   * the workgroup walks the image's queries in blocks of 64.  All four waves need the same Q head slice, so it goes through LDS: one image of 64 rows
//     with a +16-byte padded pitch (the 16 lanes of a B-fragment read hit 16 different rows: the pitch of 2 DP + 16 bytes spreads them over the banks),
//     written by the 16-byte async global -> LDS copies (glds16).  A lane's LDS slot is fixed (piece base + 16 lane), so the lane picks the SOURCE chunk
//     that belongs there; the pad slot and the columns beyond d re-read the head's last chunk (K is zero there).  The block's 64 L values follow by one
//     4-byte async copy per lane of wave 3.  Two buffers: the copies of block j + 1 are issued before block j's arithmetic and ONE barrier per block both
//     publishes a buffer and retires the other;
//   * S^T = K_blk Q_blk^T: accumulator rows are keys (lane (g, i) holds keys 4 g + {0..3} of query i), so p = exp2(s scale log2 e - L[q] log2 e) is added
//     straight into four per-key registers - ascending query blocks, inside a block ascending 16-query groups - and only at the very end the 16 lanes that
//     hold the same keys are folded by four shuffles (xor 8, 4, 2, 1);
//   * queries >= N re-read the image's last row and contribute exactly 0 (the ragged last block only); keys >= N re-read the last row and store nothing;
//   * heads are the grid's y axis: per-head sums go to a workspace fp32 [n, H, N], and a second small launch adds them in ascending h and applies 1 / H
//     once.  No atomics: two runs give the same bits.
// sdlt_sag_degrade - blur-mask-renoise as ONE launch: a 16 x 16 pixel tile with its 4-pixel halo has x0 = x - sigma e_neg formed on the fly into LDS, the
// two passes of the 9-tap blur (x, then y; edges REFLECTED without repeating the edge pixel) run from LDS, the mask select and the re-noising happen at the
// store.  sdlt_sag_apply - the two element-wise phases of the combine.  Both read sigma, scale and threshold from a device table at the sampler's step
// counter, so a captured graph serves every setting.  fp32, one rounding per operation (no contraction), IEEE division and square root.
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/sdlt_kernels.h"

static_assert(sizeof(sdlt_attn_colmass_params) == 88 && sizeof(sdlt_sag_degrade_params) == 88 && sizeof(sdlt_sag_apply_params) == 48,
              "the SAG parameter blocks have no index in sdlt_struct_size: their sizes are part of the header's text");

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KBLK = 64, QB = 64;      // keys per workgroup, queries per LDS block

template <int DP>
__global__ __launch_bounds__(256) void attn_colmass_kernel(const sdlt_attn_colmass_params p) {
  constexpr int NSTR = DP * 2 + 16, CPR = NSTR / 16, IMG = QB * NSTR, NP = IMG / 1024, PW = (NP + 3) / 4, KK = DP / 32;
  static_assert(IMG % 1024 == 0, "a Q image of one query block is a whole number of 1 KB DMA pieces");
  __shared__ __attribute__((aligned(1024))) char smem[2 * IMG + 2 * QB * 4];      // two Q images, then two rows of 64 L values
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  const int N = p.N, d = p.d, h = blockIdx.y, img = blockIdx.z;
  const int64_t b = (int64_t)p.row_off + (int64_t)img * p.row_stride;
  const bf16_t* const Qh = (const bf16_t*)p.Q + b * N * p.ldq + h * d;
  const bf16_t* const Kh = (const bf16_t*)p.K + b * N * p.ldk + h * d;
  const float* const Lh = p.L + (b * p.H + h) * N;

  // K fragments: A operands, lane (g, i) = key k0 + i, 8 columns from 8 g of the 32-wide step (zero beyond d; a key beyond N: the last row, never stored)
  const int k0 = blockIdx.x * KBLK + w * 16;
  bf16x8 kf[KK];
  {
    const bf16_t* Krow = Kh + (int64_t)min(k0 + i, N - 1) * p.ldk;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int col = kk * 32 + g * 8;
      union { uint4 u; bf16x8 v; } c;
      c.u = col < d ? *(const uint4*)(Krow + col) : make_uint4(0, 0, 0, 0);
      kf[kk] = c.v;
    }
  }

  // staging state: piece w + 4 j of the Q image is this wave's; the lane's slot there is row srow[j], and it holds source columns scol[j] ..+8
  int srow[PW], scol[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int c = (w + 4 * j) * 64 + lane, row = c / CPR;
    srow[j] = row;
    scol[j] = min(c - row * CPR, (d >> 3) - 1) * 8;
  }
  auto stage = [&](int qb, int buf) {
    char* const dst = smem + buf * IMG;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int piece = w + 4 * j;
      if (piece < NP) glds16(Qh + (int64_t)min(qb * QB + srow[j], N - 1) * p.ldq + scol[j], dst + piece * 1024);
    }
    if (w == 3)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Lh + min(qb * QB + lane, N - 1)),
                                       (__attribute__((address_space(3))) void*)(smem + 2 * IMG + buf * QB * 4), 4, 0, 0);
  };

  float m[4] = {0.f, 0.f, 0.f, 0.f};      // this lane's share of the mass of keys k0 + 4 g + {0..3}: the queries i, 16 + i, 32 + i, 48 + i of every block
  const float sl2 = p.scale * LOG2E;
  const int nqb = (N + QB - 1) / QB;

  stage(0, 0);
  for (int qb = 0, buf = 0; qb < nqb; ++qb, buf ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // block qb's image is in LDS; every wave is done with the other buffer
    asm volatile("" ::: "memory");
    const char* const Qs = smem + buf * IMG;
    const float* const Ls = (const float*)(smem + 2 * IMG + buf * QB * 4);
    if (qb + 1 < nqb) stage(qb + 1, buf ^ 1);
    const bool ragged = qb == nqb - 1 && (N & (QB - 1));      // (uniform)
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
      const char* const qrow = Qs + (qs * 16 + i) * NSTR + g * 16;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kk], *(const bf16x8*)(qrow + kk * 64), s, 0, 0, 0);
      const float lq = Ls[qs * 16 + i] * LOG2E;
      const bool live = !ragged || qb * QB + qs * 16 + i < N;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[e], sl2, -lq));
        m[e] += live ? pv : 0.f;
      }
    }
  }

#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = m[e];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    const int key = k0 + 4 * g + e;
    if (i == 0 && key < N) p.ws[((int64_t)img * p.H + h) * N + key] = v;
  }
}

// mass[img, k] = (ws[img, 0, k] + ws[img, 1, k] + ...) / H, heads in ascending order
__global__ __launch_bounds__(256) void attn_colmass_finish_kernel(const float* __restrict__ ws, float* __restrict__ mass, int N, int H, float inv_h) {
  const int k = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (k >= N) return;
  const float* src = ws + (int64_t)img * H * N + k;
  float v = src[0];
  for (int h = 1; h < H; ++h) v += src[(int64_t)h * N];
  mass[(int64_t)img * N + k] = v * inv_h;
}

template <int DP>
int colmass_launch(const sdlt_attn_colmass_params& p, hipStream_t s) {
  hipLaunchKernelGGL((attn_colmass_kernel<DP>), dim3((p.N + KBLK - 1) / KBLK, p.H, p.n), dim3(256), 0, s, p);
  SDLT_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_colmass_finish_kernel, dim3((p.N + 255) / 256, p.n), dim3(256), 0, s, (const float*)p.ws, p.mass, p.N, p.H, 1.0f / (float)p.H);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

#pragma clang fp contract(off)

constexpr int SAG_R = 4, TILE = 16, HALO = TILE + 2 * SAG_R, HPITCH = HALO + 1;

// the step row of the table: row 1 + clamp(ctr[0], 0, k - 1)
__device__ __forceinline__ const float* sag_row(const float* stab, const int32_t* ctr, int stab_rows) {
  const int k = max(min((int)stab[0], stab_rows - 1), 1);
  return stab + 4 * (1 + min(max(ctr[0], 0), k - 1));
}

// index -1 reads 1, index n reads n - 2; a tile's overhang beyond the halo of the picture (it feeds no stored pixel) is clamped into it
__device__ __forceinline__ int reflect(int v, int n) {
  v = v < 0 ? -v : v;
  v = v >= n ? 2 * (n - 1) - v : v;
  return min(max(v, 0), n - 1);
}

__global__ __launch_bounds__(256) void sag_degrade_kernel(const sdlt_sag_degrade_params p) {
  __shared__ float x0s[4][HALO][HPITCH];      // x0 of the tile and its halo
  __shared__ float hbs[4][HALO][TILE + 1];    // after the pass along x
  __shared__ float tp[2 * SAG_R + 1];
  const int img = blockIdx.z, ty0 = blockIdx.y * TILE, tx0 = blockIdx.x * TILE, t = threadIdx.x;
  const int h = p.h, w = p.w, hw = h * w;
  const float* const row = sag_row(p.stab, p.ctr, p.stab_rows);
  const float sigma = row[0], thr = row[2];
  const float* const X = p.x + (int64_t)img * 4 * hw;
  const float4* const E = (const float4*)p.eps + (int64_t)2 * img * hw;      // the negative row block of image img
  if (t < 2 * SAG_R + 1) tp[t] = p.taps[t];
  for (int c = t; c < HALO * HALO; c += 256) {
    const int ly = c / HALO, lx = c - ly * HALO;
    const int pix = reflect(ty0 - SAG_R + ly, h) * w + reflect(tx0 - SAG_R + lx, w);
    const float4 e = E[pix];
    x0s[0][ly][lx] = X[pix] - sigma * e.x;
    x0s[1][ly][lx] = X[hw + pix] - sigma * e.y;
    x0s[2][ly][lx] = X[2 * hw + pix] - sigma * e.z;
    x0s[3][ly][lx] = X[3 * hw + pix] - sigma * e.w;
  }
  __syncthreads();
  for (int c = t; c < 4 * HALO * TILE; c += 256) {
    const int ch = c / (HALO * TILE), r = c - ch * (HALO * TILE), ly = r / TILE, lx = r - ly * TILE;
    float acc = tp[0] * x0s[ch][ly][lx];
#pragma unroll
    for (int k = 1; k <= 2 * SAG_R; ++k) acc = acc + tp[k] * x0s[ch][ly][lx + k];
    hbs[ch][ly][lx] = acc;
  }
  __syncthreads();
  const int ly = t >> 4, lx = t & 15, y = ty0 + ly, x = tx0 + lx;
  if (y >= h || x >= w) return;
  const int pix = y * w + x;
  const bool masked = p.mass[(int64_t)img * p.hm * p.wm + (y * p.hm / h) * p.wm + x * p.wm / w] > thr;
  const float4 e = E[pix];
  const float en[4] = {e.x, e.y, e.z, e.w};
  const float den = sqrtf(sigma * sigma + 1.0f);
  float o[4];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    float acc = tp[0] * hbs[ch][ly][lx];
#pragma unroll
    for (int k = 1; k <= 2 * SAG_R; ++k) acc = acc + tp[k] * hbs[ch][ly + k][lx];
    const float base = masked ? acc : x0s[ch][ly + SAG_R][lx + SAG_R];
    o[ch] = (base + sigma * en[ch]) / den;
  }
  uint2 v;
  v.x = pack2bf(o[0], o[1]);
  v.y = pack2bf(o[2], o[3]);
  *(uint2*)((bf16_t*)p.out + ((int64_t)img * hw + pix) * p.ld) = v;
}

// one thread per pixel (four floats) of image j: phase 0  t = s (e_neg - t), phase 1  e_neg += t, e_pos += t
__global__ __launch_bounds__(256) void sag_apply_kernel(float4* __restrict__ eps, float4* __restrict__ tb, const float* __restrict__ stab,
                                                        const int32_t* __restrict__ ctr, int stab_rows, int hw, int phase) {
  const int pix = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (pix >= hw) return;
  float4* const en = eps + (int64_t)2 * img * hw + pix;
  float4* const tt = tb + (int64_t)img * hw + pix;
  const float4 a = *en, b = *tt;
  if (phase == 0) {
    const float s = sag_row(stab, ctr, stab_rows)[1];
    *tt = make_float4(s * (a.x - b.x), s * (a.y - b.y), s * (a.z - b.z), s * (a.w - b.w));
  } else {
    const float4 c = en[hw];
    *en = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    en[hw] = make_float4(c.x + b.x, c.y + b.y, c.z + b.z, c.w + b.w);
  }
}

}  // namespace

extern "C" int sdlt_attn_colmass(const sdlt_attn_colmass_params* pp, void* stream) {
  const char* fn = "sdlt_attn_colmass";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_attn_colmass_params& p = *pp;
  if (!p.Q || !p.K || !p.L || !p.ws || !p.mass) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (Q, K, L, ws, mass are required)", fn);
  if (p.B < 1 || p.H < 1 || p.N < 1 || p.d < 1 || p.n < 1 || p.row_off < 0 || p.row_stride < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d N=%d d=%d n=%d row_off=%d row_stride=%d (extents >= 1, row_off >= 0)", fn, p.B, p.H, p.N, p.d, p.n, p.row_off, p.row_stride);
  if ((int64_t)p.row_off + (int64_t)(p.n - 1) * p.row_stride >= p.B)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: batch row %lld of %d", fn, (long long)p.row_off + (long long)(p.n - 1) * p.row_stride, p.B);
  if ((p.d % 8) || p.d > 160) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: d=%d (d %% 8 == 0, d <= 160)", fn, p.d);
  if ((p.ldq % 8) || (p.ldk % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 8", fn);
  const int64_t C = (int64_t)p.H * p.d;
  if (p.ldq < C || p.ldk < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < H d = %lld", fn, (long long)C);
  if (((uintptr_t)p.Q | (uintptr_t)p.K) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Q, K must be 16-byte aligned", fn);
  if (((uintptr_t)p.L | (uintptr_t)p.ws | (uintptr_t)p.mass) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: L, ws, mass must be 4-byte aligned", fn);
  // in-image row indices and the grid are 32-bit; row offsets into the tensors are 64-bit
  if ((int64_t)p.B * p.N > INT_MAX - QB || C > INT_MAX || p.ldq > INT_MAX || p.ldk > INT_MAX || p.H > 65535 || p.n > 65535)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d N=%d n=%d: an index range exceeds its 32-bit (rows) or 16-bit (grid y, z) bound", fn, p.B, p.H, p.N, p.n);
  hipStream_t s = (hipStream_t)stream;
  return p.d <= 64 ? colmass_launch<64>(p, s) : p.d <= 96 ? colmass_launch<96>(p, s) : p.d <= 128 ? colmass_launch<128>(p, s) : colmass_launch<160>(p, s);
}

extern "C" int sdlt_sag_degrade(const sdlt_sag_degrade_params* pp, void* stream) {
  const char* fn = "sdlt_sag_degrade";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_sag_degrade_params& p = *pp;
  if (!p.x || !p.eps || !p.mass || !p.taps || !p.stab || !p.ctr || !p.out)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (x, eps, mass, taps, stab, ctr, out are required)", fn);
  if (p.n < 1 || p.hm < 1 || p.wm < 1 || p.stab_rows < 2 || p.ld < 4)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d hm=%d wm=%d stab_rows=%d ld=%lld (n, hm, wm >= 1, stab_rows >= 2, ld >= 4)", fn, p.n, p.hm, p.wm, p.stab_rows, (long long)p.ld);
  if (p.h < 5 || p.w < 5) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: a %d x %d latent (the reflected 4-pixel halo needs 5 on both axes)", fn, p.h, p.w);
  if (p.hm > p.h || p.wm > p.w) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: a %d x %d mass grid for a %d x %d latent", fn, p.hm, p.wm, p.h, p.w);
  if (p.h > 32768 || p.w > 32768 || (int64_t)p.h * p.w > (1 << 24) || 2 * (int64_t)p.n * p.h * p.w > INT_MAX || p.n > 65535 || p.ld > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d h=%d w=%d: h, w <= 2^15, h w <= 2^24 and 2 n h w < 2^31", fn, p.n, p.h, p.w);
  if (p.ld % 4) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 4", fn);
  if (((uintptr_t)p.eps & 15) || ((uintptr_t)p.out & 7) || (((uintptr_t)p.x | (uintptr_t)p.mass | (uintptr_t)p.taps | (uintptr_t)p.stab | (uintptr_t)p.ctr) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: eps 16-byte, out 8-byte, x / mass / taps / stab / ctr 4-byte aligned", fn);
  hipLaunchKernelGGL(sag_degrade_kernel, dim3((p.w + TILE - 1) / TILE, (p.h + TILE - 1) / TILE, p.n), dim3(256), 0, (hipStream_t)stream, p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_sag_apply(const sdlt_sag_apply_params* pp, void* stream) {
  const char* fn = "sdlt_sag_apply";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_sag_apply_params& p = *pp;
  if (!p.eps || !p.t || !p.stab || !p.ctr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (eps, t, stab, ctr are required)", fn);
  if (p.n < 1 || p.hw < 1 || p.stab_rows < 2 || p.n > 65535 || 2 * (int64_t)p.n * p.hw > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d hw=%d stab_rows=%d (n, hw >= 1, stab_rows >= 2, 2 n hw < 2^31)", fn, p.n, p.hw, p.stab_rows);
  if (p.phase != 0 && p.phase != 1) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: phase=%d (0: t = s (e_neg - t), 1: eps += t)", fn, p.phase);
  if ((((uintptr_t)p.eps | (uintptr_t)p.t) & 15) || (((uintptr_t)p.stab | (uintptr_t)p.ctr) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: eps, t 16-byte, stab, ctr 4-byte aligned", fn);
  hipLaunchKernelGGL(sag_apply_kernel, dim3((p.hw + 255) / 256, p.n), dim3(256), 0, (hipStream_t)stream, (float4*)p.eps, (float4*)p.t, p.stab, p.ctr, p.stab_rows,
                     p.hw, p.phase);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
