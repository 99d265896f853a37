// One-pass (flash) attention forward for ONE WIDE HEAD on MFMA (gfx950): the mid-block attention of AutoencoderKL, one head as wide as the block
// (d = 512 for the SD / SDXL VAE, d = 128 for the project's toy VAE), N = h w tokens.  O[b] = softmax(scale Q[b] K[b]^T) V[b], non-causal, no pad rows.
// No [N, N] buffer exists anywhere: fp32 scores live in registers and LDS, the online softmax runs in fp32, P is rounded to bf16 for the P V MFMAs,
// O accumulates in fp32 and is rounded once at the store.  Forward only, no log-sum-exp output: the VAE is frozen and nobody trains through it.
//
// Why not the layout of attn.hip / attn32.hip (a wave owns 16 / 32 query rows x the whole head, K and V tiles shared through LDS): at d = 512 a wave's O
// block alone is 256 accumulator registers per lane for 32 rows, and a 4-wave workgroup re-reads each 64 KB (K, V) tile pair of 32 keys four times from
// LDS for 8.4 MFLOP - about as many LDS cycles (128 B / clk) as MFMA cycles.  Here the HEAD WIDTH is split across the four waves instead:
//   * all four waves share the same BM = 64 query rows; wave w owns columns [w d/4, (w+1) d/4) of Q, K, V and O;
//   * Q K^T: wave w multiplies its Q slice (registers, loaded once) by its K slice - a partial sum over d.  No K element is needed by two waves, so K
//     fragments go global -> registers in MFMA operand order (16-byte loads along d, the contraction axis);
//   * the four [64 x 64] fp32 partials meet in LDS; wave w adds them in a fixed order for query rows [16 w, 16 w + 16), runs the online softmax for those
//     rows (their m and l live in that wave's registers) and broadcasts P (bf16) and the per-row rescale factors through LDS;
//   * P V: wave w owns its d/4 columns of O.  The contraction runs over KEYS, which V (token-major) has along its rows: each wave stages its own
//     [64 keys x d/4] slice of V in a wave-private LDS region with plain 16-byte copies and reads it back with the transposing LDS read
//     (ds_read_b64_tr_b16), as the sibling kernels do.  No V element is needed by two waves either.
// Two workgroup barriers per 64-key tile (partials visible / P visible).  Keys at or beyond Nk are masked in the softmax; their K / V rows (and query rows
// at or beyond Nq) are read from the image's LAST VALID row instead, so no row outside [0, B Nk) / [0, B Nq) is ever touched and no load needs a
// predicate.  No atomics, one summation order: bit-reproducible.  DESIGN 4.37 has the arithmetic and the compiler's resource figures.
#include <climits>
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 64, BN = 64, NW = 4;          // query rows / keys per tile, waves (= slices of d) per workgroup
constexpr int SSTR = BN * 4 + 16;                // bytes per query row of one wave's fp32 partial [BM][BN] (+16: the 16 rows of a lane group spread over the banks)
constexpr int PSTR = BN * 2 + 16;                // bytes per query row of P (bf16)
template <int D> constexpr int vstr() { return D / NW * 2 + 16; }      // bytes per key row of a wave's V slice
template <int D> constexpr int smem_bytes() { return NW * BM * SSTR + BM * PSTR + 2 * BM * 4 + NW * BN * vstr<D>(); }

// (attn.hip's helper) MFMA fragment contracted over the ROW axis of a row-major bf16 LDS tile: lane (g, i) receives rows r0 + 8 g + {0..7} of column
// c0 + i; p = tile + (r0 + 8 g + (i >> 2)) * stride + (c0 + 4 (i & 3)) * 2
__device__ __forceinline__ bf16x8 lds_tr_frag(const char* p, int stride) {
  typedef __attribute__((address_space(3))) bf16x4* lds_ptr;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)p);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(p + 4 * stride));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 as_frag(uint4 u) { return __builtin_bit_cast(bf16x8, u); }

template <int D>
__global__ __launch_bounds__(256) void attn_wide_kernel(const sdlt_attn_wide_params p, const int ntile) {
  constexpr int DS = D / NW, KK = DS / 32, DF = DS / 16, VSTR = vstr<D>(), VCH = DS / 8, NV = BN * VCH / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Sp = smem;                                   // [NW][BM] rows of SSTR bytes: the waves' partial scores, [query][key]
  char* const Pl = Sp + NW * BM * SSTR;                    // [BM] rows of PSTR bytes: P, [query][key]
  float* const al = (float*)(Pl + BM * PSTR);              // [BM] this tile's rescale factor of every query row
  float* const li = al + BM;                               // [BM] 1 / l after the last tile
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  char* const Vw = (char*)(li + BM) + w * BN * VSTR;       // this wave's own V slice, [key][d / 4]

  // workgroups go to the 8 XCDs round-robin by linear id: renumber so that every XCD (one L2 each) runs a contiguous range of the image-major order
  int L = blockIdx.x;
  {
    const int n = gridDim.x, k = L & 7, slot = L >> 3, q = n >> 3, r = n & 7;
    L = (k < r ? k * (q + 1) : r * (q + 1) + (k - r) * q) + slot;
  }
  const int b = L / ntile, q0 = (L - b * ntile) * BM;
  const int Nq = p.Nq, Nk = p.Nk;
  const bf16_t* const Qb = (const bf16_t*)p.Q + (int64_t)b * Nq * p.ldq + w * DS;
  const bf16_t* const Kb = (const bf16_t*)p.K + (int64_t)b * Nk * p.ldk + w * DS;
  const bf16_t* const Vb = (const bf16_t*)p.V + (int64_t)b * Nk * p.ldv + w * DS;

  // Q slice: B operands of the 16x16x32 MFMA, lane (g, i) = row i of the query block, 8 columns from 8 g of the 32-wide step
  bf16x8 qf[4][KK];
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) {
    const int64_t row = min(q0 + qb * 16 + i, Nq - 1);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[qb][kk] = as_frag(*(const uint4*)(Qb + row * p.ldq + kk * 32 + g * 8));
  }
  f32x4 o[4][DF];        // O^T blocks: [query block][16 columns of the slice]: lane (g, i) = columns 4 g .. 4 g + 3 of query row i
#pragma unroll
  for (int qb = 0; qb < 4; ++qb)
#pragma unroll
    for (int df = 0; df < DF; ++df) o[qb][df] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -1e30f, l = 0.f;        // online-softmax state of query row q0 + 16 w + i (the same in the four lanes g)
  const float sl2 = p.scale * LOG2E;

  for (int k0 = 0; k0 < Nk; k0 += BN) {
    // V slice of this tile: global -> registers now, -> LDS after the score MFMAs (the loads fly under them)
    uint4 vr[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = lane + 64 * j, row = c / VCH, ch = c - row * VCH;
      vr[j] = *(const uint4*)(Vb + (int64_t)min(k0 + row, Nk - 1) * p.ldv + ch * 8);
    }
    // partial scores S^T[key][query] over this wave's slice of d
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const bf16_t* krow = Kb + (int64_t)min(k0 + kf * 16 + i, Nk - 1) * p.ldk + g * 8;
      bf16x8 kfr[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) kfr[kk] = as_frag(*(const uint4*)(krow + kk * 32));
#pragma unroll
      for (int qb = 0; qb < 4; ++qb) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[kk], qf[qb][kk], s, 0, 0, 0);
        // lane (g, i): keys 16 kf + 4 g .. + 3 of query 16 qb + i
        *(f32x4*)(Sp + (w * BM + qb * 16 + i) * SSTR + (kf * 16 + g * 4) * 4) = s;
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = lane + 64 * j, row = c / VCH, ch = c - row * VCH;
      *(uint4*)(Vw + row * VSTR + ch * 16) = vr[j];
    }
    __syncthreads();        // every wave's partial is in LDS

    // wave w: query row 16 w + i, lane group g takes keys 16 g .. 16 g + 15: add the four partials in wave order, online softmax
    {
      const int qr = w * 16 + i;
      float t[16];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f32x4 a = *(const f32x4*)(Sp + qr * SSTR + (g * 16 + c * 4) * 4);
#pragma unroll
        for (int ws = 1; ws < NW; ++ws) a += *(const f32x4*)(Sp + (ws * BM + qr) * SSTR + (g * 16 + c * 4) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) t[c * 4 + r] = k0 + g * 16 + c * 4 + r < Nk ? a[r] * sl2 : -1e30f;
      }
      float tmax = t[0];
#pragma unroll
      for (int c = 1; c < 16; ++c) tmax = fmaxf(tmax, t[c]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m, tmax);        // finite: key k0 is valid in every tile
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      float rs = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        t[c] = __builtin_amdgcn_exp2f(t[c] - mn);
        rs += t[c];
      }
      rs += __shfl_xor(rs, 16, 64);
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      uint4 lo, hi;
      lo.x = pack2bf(t[0], t[1]); lo.y = pack2bf(t[2], t[3]); lo.z = pack2bf(t[4], t[5]); lo.w = pack2bf(t[6], t[7]);
      hi.x = pack2bf(t[8], t[9]); hi.y = pack2bf(t[10], t[11]); hi.z = pack2bf(t[12], t[13]); hi.w = pack2bf(t[14], t[15]);
      *(uint4*)(Pl + qr * PSTR + g * 32) = lo;
      *(uint4*)(Pl + qr * PSTR + g * 32 + 16) = hi;
      if (g == 0) al[qr] = alpha;
    }
    __syncthreads();        // P and the rescale factors are in LDS

    // O^T[col][query] = O^T alpha + V^T P^T over this wave's columns
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const float a = al[qb * 16 + i];
      if (__builtin_amdgcn_ballot_w64(a != 1.0f)) {      // (wave-uniform) once the running maxima have settled most blocks skip the rescale
#pragma unroll
        for (int df = 0; df < DF; ++df) o[qb][df] *= a;
      }
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 pf[4];
#pragma unroll
      for (int qb = 0; qb < 4; ++qb) pf[qb] = as_frag(*(const uint4*)(Pl + (qb * 16 + i) * PSTR + (kb * 32 + g * 8) * 2));
#pragma unroll
      for (int df = 0; df < DF; ++df) {
        const bf16x8 vf = lds_tr_frag(Vw + (kb * 32 + 8 * g + (i >> 2)) * VSTR + (df * 16 + 4 * (i & 3)) * 2, VSTR);
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) o[qb][df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb], o[qb][df], 0, 0, 0);
      }
    }
    // (the next tile's partials and V slice are written only after this wave's reads above; P and al only after the next barrier)
  }

  if (g == 0) li[w * 16 + i] = 1.0f / l;
  __syncthreads();
  bf16_t* const Ob = (bf16_t*)p.O + (int64_t)b * Nq * p.ldo + w * DS;
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) {
    const int q = q0 + qb * 16 + i;
    if (q < Nq) {
      const float inv = li[qb * 16 + i];
#pragma unroll
      for (int df = 0; df < DF; ++df) {
        uint2 v;
        v.x = pack2bf(o[qb][df][0] * inv, o[qb][df][1] * inv);
        v.y = pack2bf(o[qb][df][2] * inv, o[qb][df][3] * inv);
        *(uint2*)(Ob + (int64_t)q * p.ldo + df * 16 + g * 4) = v;
      }
    }
  }
}

template <int D>
int attn_wide_launch(const sdlt_attn_wide_params& p, hipStream_t s) {
  const int ntile = (p.Nq + BM - 1) / BM;
  if (sdlt_raise_smem((const void*)attn_wide_kernel<D>, smem_bytes<D>())) SDLT_FAIL(SDLT_ERR_LAUNCH, "sdlt_attn_wide_fwd: LDS attribute");
  hipLaunchKernelGGL(attn_wide_kernel<D>, dim3((unsigned)(p.B * ntile)), dim3(256), smem_bytes<D>(), s, p, ntile);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

}  // namespace

extern "C" int sdlt_attn_wide_fwd(const sdlt_attn_wide_params* pp, void* stream) {
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_attn_wide_fwd: null parameter block");
  const sdlt_attn_wide_params& p = *pp;
  if (!p.Q || !p.K || !p.V || !p.O) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_attn_wide_fwd: null operand (Q, K, V, O are required)");
  if (p.B <= 0 || p.Nq <= 0 || p.Nk <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_attn_wide_fwd: B=%d Nq=%d Nk=%d (all >= 1)", p.B, p.Nq, p.Nk);
  if (p.d != 512 && p.d != 128) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_attn_wide_fwd: d=%d (built for 512 and 128; narrower heads: sdlt_attn_fwd)", p.d);
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_attn_wide_fwd: ld %% 8");
  if (p.ldq < p.d || p.ldk < p.d || p.ldv < p.d || p.ldo < p.d) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_attn_wide_fwd: ld < d");
  // in-image row indices (up to N + 63) and the grid (B ceil(Nq / 64)) are 32-bit; row offsets into the tensors are 64-bit
  if ((int64_t)p.B * (p.Nq > p.Nk ? p.Nq : p.Nk) > (int64_t)INT_MAX - BM)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_attn_wide_fwd: B * max(Nq, Nk) = %lld exceeds 2^31 - 65", (long long)p.B * (p.Nq > p.Nk ? p.Nq : p.Nk));
  return p.d == 512 ? attn_wide_launch<512>(p, (hipStream_t)stream) : attn_wide_launch<128>(p, (hipStream_t)stream);
}
