// Region-coupled cross-attention forward on MFMA (gfx950): "Attention Couple", regional prompts inside ONE UNet pass.  Every query keeps one row, attends to
// each region's (<= 128) text keys separately and mixes the R results with its own region weights:
//   O[b, q, hd] = sum over r < Rb of  Wt[r, q] * softmax_k(scale Q[b, q, hd] . K[b, r, k, hd]) V[b, r, k, hd],   Rb = clamp(rcount[b], 1, R)
// Q, O bf16 token-major [B Nq, ld], head hd in columns [hd d, (hd + 1) d), NO pad rows; K, V bf16 [B R Nkp, ld], region r of batch row b in rows
// [(b R + r) Nkp, + Nk); Wt fp32 [R, Nq], shared by the batch rows and not normalised here.  Forward only, no log-sum-exp: a render trains nothing.
//
// Work split: one workgroup of four waves per (batch row, head, 64-query tile); wave w owns queries [16 w, 16 w + 16) and keeps their Q fragments in registers
// for all regions.  All four waves need the same K[b, r] / V[b, r] head slices, so those go through LDS: 32-key blocks of DP columns, filled by the 16-byte async
// global -> LDS copies (glds16) into one of two buffers; the copy of the NEXT live region is issued before the current region's arithmetic, and ONE barrier per
// region both publishes a buffer and retires the other (a buffer is refilled only after the barrier every wave passes once it has finished reading it).  Where two
// buffers do not fit the 160 KB (d = 160 with more than 96 keys) the kernel runs on one buffer and two barriers per region.
// The key row of a region is resident as a whole, so the softmax is exact and runs in registers in one go: no running maximum, no rescale of O.
// Live-region mask: each wave ballots "any non-zero weight" per region over its 16 queries, the four ballots meet in LDS, and regions without weight anywhere in
// the tile are skipped whole (a uniform branch) - with box or hard masks most tiles walk one or two regions.  A region that is live in the tile contributes
// w * o for every query, zero weights included.
// LDS rows: d <= 64 uses attn.hip's 128-byte rows with the 16-byte chunk index XOR-ed by row bits 1 and 3 - conflict-free for the permuted K fragment reads and
// for the transposing V reads alike (attn.hip has the bank arithmetic) - and the wider heads its +16-byte padded pitch.  Both are produced by the DMA itself: a lane's LDS
// slot is fixed (piece base + 16 lane), so the lane picks the SOURCE chunk that belongs there (the XOR-ed one; a pad slot re-reads a valid chunk).
// Rows and columns that do not exist are never read: query rows >= Nq and key rows >= Nk read the last valid row, columns >= d the head's last chunk (Q is zero
// there, and those O columns are not stored); regions >= Rb are not touched at all and may hold NaN.  fp32 scores, bf16 P, fp32 accumulation, regions added in
// ascending r from +0.0, one rounding at the store; no atomics, no workspace: two runs give the same bits.  DESIGN 4.38 has the compiler's resource figures.
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 64, RMAX = 16, NKMAX = 128, LDS_MAX = 160 * 1024;

// attn.hip's tile geometry (see the header comment)
template <int DP> __device__ __host__ constexpr int tile_stride() { return DP == 64 ? 128 : DP * 2 + 16; }
template <int DP> __device__ __forceinline__ int row_sw(int row) { return DP == 64 ? ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2)) : 0; }
// bytes of one K (or V) image of `rows` keys, whole 1 KB DMA pieces
template <int DP> __device__ __host__ constexpr int image_bytes(int rows) { return (rows * tile_stride<DP>() + 1023) & ~1023; }

__device__ __forceinline__ int prow(int i, int half) { return ((i >> 2) << 3) + half * 4 + (i & 3); }
__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
  union { uint4 u; bf16x8 v; } c;
  c.u.x = pack2bf(a[0], a[1]); c.u.y = pack2bf(a[2], a[3]);
  c.u.z = pack2bf(b[0], b[1]); c.u.w = pack2bf(b[2], b[3]);
  return c.v;
}
// (attn.hip's helper) MFMA fragment contracted over the ROW axis of a row-major bf16 LDS tile: lane (g, i) receives rows r0 + 8 g + {0..7} of column c0 + i
__device__ __forceinline__ bf16x8 lds_tr_frag(const char* p, int stride) {
  typedef __attribute__((address_space(3))) bf16x4* lds_ptr;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)p);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(p + 4 * stride));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// One region's K and V head slices -> LDS images at `dst` (K) and `dst + img` (V): 1 KB pieces dealt to the four waves.  LDS slot c of a row holds source chunk
// c ^ row_sw (DP = 64) or chunk c, slot DP / 8 being the pad (padded pitch); rows >= Nk and chunks >= d / 8 re-read the last valid one.
template <int DP>
__device__ __forceinline__ void stage_region(const bf16_t* Kr, const bf16_t* Vr, int64_t ldk, int64_t ldv, int Nk, int dch, char* dst, int img, int w, int lane) {
  constexpr int CPR = tile_stride<DP>() / 16;
  const int np = img >> 10;
  for (int piece = w; piece < np; piece += 4) {
    const int c = piece * 64 + lane, row = c / CPR;
    const int ch = min((c - row * CPR) ^ row_sw<DP>(row), dch - 1), srow = min(row, Nk - 1);
    glds16(Kr + (int64_t)srow * ldk + ch * 8, dst + piece * 1024);
    glds16(Vr + (int64_t)srow * ldv + ch * 8, dst + img + piece * 1024);
  }
}

template <int DP, int NBUF>
__global__ __launch_bounds__(256) void attn_couple_kernel(const sdlt_attn_couple_params p, const int ntile) {
  constexpr int NSTR = tile_stride<DP>(), KK = DP / 32, DF = DP / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  const int Nq = p.Nq, Nk = p.Nk, d = p.d, R = p.R;
  const int nkb = (Nk + 31) >> 5;      // 32-key blocks: two permuted 16-row score fragments each (a fragment's keys are not a contiguous range), one P V contraction step
  const int img = image_bytes<DP>(nkb * 32);
  unsigned* const lm = (unsigned*)(smem + NBUF * 2 * img);     // the waves' live-region ballots

  // workgroups go to the 8 XCDs round-robin by linear id: renumber so that every XCD (one L2 each) runs a contiguous range of the (tile fastest, head, batch row)
  // order - the tiles of one head, which all stream the same R key / value blocks, then share one L2
  int L = blockIdx.x;
  {
    const int n = gridDim.x, k = L & 7, slot = L >> 3, q = n >> 3, r = n & 7;
    L = (k < r ? k * (q + 1) : r * (q + 1) + (k - r) * q) + slot;
  }
  const int bh = L / ntile, q0 = (L - bh * ntile) * BM, b = bh / p.H, hc = (bh - b * p.H) * d;
  const int q = q0 + w * 16 + i, qr = min(q, Nq - 1);
  int Rb = R;
  if (p.rcount) Rb = min(max(__builtin_amdgcn_readfirstlane(p.rcount[b]), 1), R);

  // live regions of this tile
  unsigned live = 0;
  for (int r = 0; r < Rb; ++r)
    if (__builtin_amdgcn_ballot_w64(p.Wt[(int64_t)r * Nq + qr] != 0.f)) live |= 1u << r;
  if (lane == 0) lm[w] = live;

  // Q fragments: B operands of the 16x16x32 MFMA, lane (g, i) = query i, 8 columns from 8 g of the 32-wide step (zero beyond d)
  bf16x8 qf[KK];
  {
    const bf16_t* Qrow = (const bf16_t*)p.Q + ((int64_t)b * Nq + qr) * p.ldq + hc;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int col = kk * 32 + g * 8;
      union { uint4 u; bf16x8 v; } c;
      c.u = col < d ? *(const uint4*)(Qrow + col) : make_uint4(0, 0, 0, 0);
      qf[kk] = c.v;
    }
  }
  __syncthreads();
  live = __builtin_amdgcn_readfirstlane(lm[0] | lm[1] | lm[2] | lm[3]);

  f32x4 acc[DF];
#pragma unroll
  for (int df = 0; df < DF; ++df) acc[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float sl2 = p.scale * LOG2E;
  const int troff = (8 * g + (i >> 2)) * NSTR + (i & 3) * 8;      // transposing-read lane offset inside an image
  const int tsw = row_sw<DP>(8 * g + (i >> 2)) >> 1;              // this lane's XOR on the 32-byte column block of a transposing read
  const bf16_t* const Kb = (const bf16_t*)p.K + (int64_t)b * R * p.Nkp * p.ldk + hc;
  const bf16_t* const Vb = (const bf16_t*)p.V + (int64_t)b * R * p.Nkp * p.ldv + hc;
  const int64_t rk = (int64_t)p.Nkp * p.ldk, rv = (int64_t)p.Nkp * p.ldv;

  int r = live ? __builtin_ctz(live) : -1, buf = 0;
  if (r >= 0) stage_region<DP>(Kb + r * rk, Vb + r * rv, p.ldk, p.ldv, Nk, d >> 3, smem, img, w, lane);
  while (r >= 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // region r's images are in LDS; every wave is done with the other buffer
    asm volatile("" ::: "memory");
    const unsigned rest = live & ~((2u << r) - 1u);
    const int rn = rest ? __builtin_ctz(rest) : -1;
    const char* const Ks = smem + buf * 2 * img;
    const char* const Vs = Ks + img;
    if (NBUF == 2 && rn >= 0) stage_region<DP>(Kb + rn * rk, Vb + rn * rv, p.ldk, p.ldv, Nk, d >> 3, smem + (buf ^ 1) * 2 * img, img, w, lane);
    const float wt = p.Wt[(int64_t)r * Nq + qr];

    // S^T = K Q^T: lane (g, i) holds keys 32 (kf >> 1) + 8 g + 4 (kf & 1) + {0..3} of query i (attn.hip's permuted rows)
    f32x4 s[8];
#pragma unroll
    for (int kf = 0; kf < 8; ++kf) {
      s[kf] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if ((kf >> 1) < nkb) {
        const int krow = (kf >> 1) * 32 + prow(i, kf & 1);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const bf16x8 kfr = *(const bf16x8*)(Ks + krow * NSTR + (((kk * 4 + g) ^ row_sw<DP>(krow)) << 4));
          s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[kk], s[kf], 0, 0, 0);
        }
      }
    }
    // exact softmax over the resident key row: raw scores, the scale rides in the exponent's FMA
    float tmax = -1e30f;
#pragma unroll
    for (int kf = 0; kf < 8; ++kf)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if ((kf >> 1) * 32 + g * 8 + (kf & 1) * 4 + e >= Nk) s[kf][e] = -1e30f;
        tmax = fmaxf(tmax, s[kf][e]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = tmax * sl2;        // finite: key 0 is valid
    float l = 0.f;
#pragma unroll
    for (int kf = 0; kf < 8; ++kf)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kf][e], sl2, -mn));
        s[kf][e] = pv;
        l += pv;
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float coef = wt / l;

    // O_r^T = V^T P^T (V read transposed from its natural image), then acc += (w / l) O_r
    f32x4 o[DF];
#pragma unroll
    for (int df = 0; df < DF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb < nkb) {
        const bf16x8 pf = pack8(s[2 * kb], s[2 * kb + 1]);
#pragma unroll
        for (int df = 0; df < DF; ++df) {
          if (df * 16 < d) {
            const bf16x8 vf = lds_tr_frag(Vs + troff + kb * 32 * NSTR + ((df ^ tsw) << 5), NSTR);
            o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[df], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int df = 0; df < DF; ++df) acc[df] += coef * o[df];

    if constexpr (NBUF == 2) {
      buf ^= 1;
    } else if (rn >= 0) {
      __builtin_amdgcn_s_barrier();      // one buffer: every wave has read region r before it is overwritten
      asm volatile("" ::: "memory");
      stage_region<DP>(Kb + rn * rk, Vb + rn * rv, p.ldk, p.ldv, Nk, d >> 3, smem, img, w, lane);
    }
    r = rn;
  }

  if (q < Nq) {
    bf16_t* const Orow = (bf16_t*)p.O + ((int64_t)b * Nq + q) * p.ldo + hc;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      const int col = df * 16 + g * 4;
      if (col < d) {
        uint2 v;
        v.x = pack2bf(acc[df][0], acc[df][1]);
        v.y = pack2bf(acc[df][2], acc[df][3]);
        *(uint2*)(Orow + col) = v;
      }
    }
  }
}

int couple_dp(int d) {      // attn.hip's attn_dp
  if (d <= 0 || (d % 8)) return -1;
  return d <= 64 ? 64 : d <= 96 ? 96 : d <= 128 ? 128 : d <= 160 ? 160 : -1;
}

template <int DP, int NBUF>
int attn_couple_launch2(const sdlt_attn_couple_params& p, hipStream_t s) {
  const int ntile = (p.Nq + BM - 1) / BM, bytes = NBUF * 2 * image_bytes<DP>((p.Nk + 31) / 32 * 32) + 16;
  if (sdlt_raise_smem((const void*)attn_couple_kernel<DP, NBUF>, LDS_MAX)) SDLT_FAIL(SDLT_ERR_LAUNCH, "sdlt_attn_couple_fwd: LDS attribute");
  hipLaunchKernelGGL((attn_couple_kernel<DP, NBUF>), dim3((unsigned)(p.B * p.H * ntile)), dim3(256), bytes, s, p, ntile);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
template <int DP>
int attn_couple_launch(const sdlt_attn_couple_params& p, hipStream_t s) {
  if constexpr (4 * image_bytes<DP>(NKMAX) + 16 > LDS_MAX)      // d = 160: two buffers of more than 96 keys do not fit
    if (4 * image_bytes<DP>((p.Nk + 31) / 32 * 32) + 16 > LDS_MAX) return attn_couple_launch2<DP, 1>(p, s);
  return attn_couple_launch2<DP, 2>(p, s);
}

// [lo, hi) byte ranges of the operands
struct Span { uintptr_t lo, hi; };
Span span2d(const void* ptr, int64_t rows, int64_t ld, int64_t cols, int elt) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)((rows - 1) * ld + cols) * elt}; }
bool overlaps(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int sdlt_attn_couple_fwd(const sdlt_attn_couple_params* pp, void* stream) {
  const char* fn = "sdlt_attn_couple_fwd";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_attn_couple_params& p = *pp;
  if (!p.Q || !p.K || !p.V || !p.O || !p.Wt) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (Q, K, V, O, Wt are required)", fn);
  if (p.B < 1 || p.H < 1 || p.Nq < 1 || p.Nk < 1 || p.R < 1 || p.d < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d Nq=%d Nk=%d R=%d d=%d (all >= 1)", fn, p.B, p.H, p.Nq, p.Nk, p.R, p.d);
  if (p.R > RMAX || p.Nk > NKMAX || p.Nkp < p.Nk) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: R=%d (<= %d) Nk=%d (<= %d) Nkp=%d (>= Nk)", fn, p.R, RMAX, p.Nk, NKMAX, p.Nkp);
  if (p.Nkp % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Nkp=%d %% 8", fn, p.Nkp);
  const int dp = couple_dp(p.d);
  if (dp < 0) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: d=%d (d %% 8 == 0, d <= 160)", fn, p.d);
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 8", fn);
  const int64_t C = (int64_t)p.H * p.d;
  if (p.ldq < C || p.ldk < C || p.ldv < C || p.ldo < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < H d = %lld", fn, (long long)C);
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Q, K, V, O must be 16-byte aligned", fn);
  if (((uintptr_t)p.Wt | (uintptr_t)p.rcount) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Wt, rcount must be 4-byte aligned", fn);
  // in-row indices (queries up to Nq + 63, columns below ld, the grid B H ceil(Nq / 64)) are 32-bit; row offsets into the tensors are 64-bit
  const int64_t ntile = ((int64_t)p.Nq + BM - 1) / BM;
  if (p.Nq > INT_MAX - BM || C > INT_MAX || (int64_t)p.B * p.H * ntile > INT_MAX || (int64_t)p.B * p.R * p.Nkp > INT_MAX ||
      p.ldq > INT_MAX || p.ldk > INT_MAX || p.ldv > INT_MAX || p.ldo > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d Nq=%d R=%d Nkp=%d: an index range exceeds 32 bits", fn, p.B, p.H, p.Nq, p.R, p.Nkp);
  const Span o = span2d(p.O, (int64_t)p.B * p.Nq, p.ldo, C, 2);
  if (overlaps(o, span2d(p.Q, (int64_t)p.B * p.Nq, p.ldq, C, 2)) || overlaps(o, span2d(p.K, (int64_t)p.B * p.R * p.Nkp, p.ldk, C, 2)) ||
      overlaps(o, span2d(p.V, (int64_t)p.B * p.R * p.Nkp, p.ldv, C, 2)) || overlaps(o, span2d(p.Wt, p.R, p.Nq, p.Nq, 4)) ||
      (p.rcount && overlaps(o, span2d(p.rcount, 1, p.B, p.B, 4))))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: O overlaps an input", fn);
  hipStream_t s = (hipStream_t)stream;
  return dp == 64 ? attn_couple_launch<64>(p, s) : dp == 96 ? attn_couple_launch<96>(p, s) : dp == 128 ? attn_couple_launch<128>(p, s) : attn_couple_launch<160>(p, s);
}
