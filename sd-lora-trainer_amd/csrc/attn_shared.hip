// Style-aligned batches (Hertz et al. 2023, "Style Aligned Image Generation via Shared Attention") on gfx950: shared self-attention as ONE flash kernel and the
// AdaIN tables it reads.  include/sdlt_kernels.h has the contracts, DESIGN 4.42 the compiler's resource figures.
//
// sdlt_attn_shared_fwd - image b of a group of G attends to its own N keys and, unless it is the group's reference r (its first image: r = (b / G) G for groups of
// consecutive images, gs = 1; r = (b / (G gs)) G gs + b % gs where gs groups interleave, as the negative and positive rows of a guided batch do), to r's N keys too:
//   s = scale q' . k'_b[j]  (own)      s = scale q' . K_r[j] + shift  (reference)      O = softmax over both segments (s) [V_b ; V_r]
// with q' = Aq o q + Sq, k' = Ak o k + Sk the AdaIN affines of image b (tables null: identity).  No [own; reference] copy of K or V exists: the kernel walks two
// row ranges.  attn_window.hip's machine (one workgroup of four waves per 64 queries of one head of one image, a wave's 16 queries as MFMA B fragments in
// registers, K / V head slices in 64-key blocks through two LDS buffers filled by the 16-byte async global -> LDS copies, ONE barrier per block, the XOR-ed
// 128-byte rows for d <= 64 and the +16-byte pitch above, online softmax with the scale riding in the exponent's FMA) with three changes:
//   * the walk runs over 2 ceil(N / 64) blocks (ceil(N / 64) for the reference itself); block t >= ceil(N / 64) is block t - ceil(N / 64) of the REFERENCE's rows.
//     The copy of block t + 1 is issued before block t's arithmetic whatever segment it lies in, so the prefetch crosses the boundary, and the running maximum
//     and sum simply carry on: one softmax over both segments;
//   * K is never rewritten.  k' . q' = k . (Ak o q') + Sk . q', so the own segment multiplies the raw keys by the fragments bf16(q' o Ak) and adds the per-query
//     fp32 constant q' . Sk (reduced over the four lane groups once, before the walk), the reference segment multiplies by bf16(q') and adds shift / scale (the
//     reference's own affine is the identity).  Two fragment sets and two scalars per query; q' is formed in fp32 on load and rounded once per set.  Without
//     tables (template AFF = false) there is one set and the constant 0: the registers of a plain flash kernel;
//   * workgroups are numbered (query block fastest, image inside its group, head, group) and renumbered so that an XCD runs a contiguous range: the pictures of a
//     group, which all stream the same reference slices, share one L2.
// Rows >= N and columns >= d are never read: such queries and keys read the image's LAST row (queries store nothing, keys score -1e30, P = 0), columns >= d the
// head's last chunk (Q is zero there and those O columns are not stored).  Only image b and its reference are read: NaN in another group cannot reach this one.
// fp32 scores, bf16 P, fp32 accumulation in ascending blocks (own, then reference), one rounding at the store; no atomics, no workspace: two runs give the same bits.
//
// sdlt_adain_affine - the tables.  Per image and column: mean and unbiased variance over the N tokens, A = std_r / std_b, S = mean_r - A mean_b.  Safe against
// cancellation by per-chunk (n, mean, M2): a workgroup owns 256 rows x 64 columns, keeps its 8 rows x 8 columns per lane in registers, sums them (lane order,
// then 32 row slots in ascending order through LDS) into the chunk mean, then sums the CENTRED squares from the same registers.  (mean, M2) of every chunk go to
// a small fp32 workspace; a finish launch combines the chunks in ascending order (Chan's update) for image b and for its reference and writes the two tables.
// No atomics: two runs give the same bits.
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/sdlt_kernels.h"

static_assert(sizeof(sdlt_attn_shared_params) == 136 && sizeof(sdlt_adain_affine_params) == 64,
              "the shared-attention parameter blocks have no index in sdlt_struct_size: their sizes are part of the header's text");

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 64, KB = 64;      // queries per workgroup, keys per LDS block

// attn.hip's tile geometry (see attn_window.hip)
template <int DP> __device__ __host__ constexpr int tile_stride() { return DP == 64 ? 128 : DP * 2 + 16; }
template <int DP> __device__ __forceinline__ int row_sw(int row) { return DP == 64 ? ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2)) : 0; }

__device__ __forceinline__ int prow(int i, int half) { return ((i >> 2) << 3) + half * 4 + (i & 3); }
__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
  union { uint4 u; bf16x8 v; } c;
  c.u.x = pack2bf(a[0], a[1]); c.u.y = pack2bf(a[2], a[3]);
  c.u.z = pack2bf(b[0], b[1]); c.u.w = pack2bf(b[2], b[3]);
  return c.v;
}
__device__ __forceinline__ bf16x8 pack8(const float* v) {
  union { uint4 u; bf16x8 v; } c;
  c.u.x = pack2bf(v[0], v[1]); c.u.y = pack2bf(v[2], v[3]);
  c.u.z = pack2bf(v[4], v[5]); c.u.w = pack2bf(v[6], v[7]);
  return c.v;
}
// (attn.hip's helper) MFMA fragment contracted over the ROW axis of a row-major bf16 LDS tile: lane (g, i) receives rows r0 + 8 g + {0..7} of column c0 + i
__device__ __forceinline__ bf16x8 lds_tr_frag(const char* p, int stride) {
  typedef __attribute__((address_space(3))) bf16x4* lds_ptr;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)p);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_ptr)(p + 4 * stride));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void load8f(const float* p, float* v) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

template <int DP, bool AFF>
__global__ __launch_bounds__(256) void attn_shared_kernel(const sdlt_attn_shared_params p, const int nqb) {
  constexpr int NSTR = tile_stride<DP>(), CPR = NSTR / 16, IMG = KB * NSTR, NP = IMG / 1024, PW = (NP + 3) / 4, KK = DP / 32, DF = DP / 16;
  static_assert(IMG % 1024 == 0, "a K (or V) image of one key block is a whole number of 1 KB DMA pieces");
  extern __shared__ __attribute__((aligned(1024))) char smem[];      // 4 IMG bytes: two buffers of (K image, V image)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  const int N = p.N, d = p.d;

  int L = blockIdx.x;
  {
    const int nwg = gridDim.x, k = L & 7, slot = L >> 3, q = nwg >> 3, r = nwg & 7;
    L = (k < r ? k * (q + 1) : r * (q + 1) + (k - r) * q) + slot;
  }
  const int rest = L / nqb, q0 = (L - rest * nqb) * BM, rest2 = rest / p.G, bi = rest - rest2 * p.G, grp = rest2 / p.H, hc = (rest2 - grp * p.H) * d;
  const int blk = grp / p.gs, br = blk * p.G * p.gs + (grp - blk * p.gs), b = br + bi * p.gs;      // the reference of group grp, this image: its member bi
  const bf16_t* const Kb = (const bf16_t*)p.K + (int64_t)b * N * p.ldk + hc;
  const bf16_t* const Vb = (const bf16_t*)p.V + (int64_t)b * N * p.ldv + hc;
  const bf16_t* const Kr = (const bf16_t*)p.K + (int64_t)br * N * p.ldk + hc;
  const bf16_t* const Vr = (const bf16_t*)p.V + (int64_t)br * N * p.ldv + hc;

  // Q fragments: B operands of the 16x16x32 MFMA, lane (g, i) = query i, 8 columns from 8 g of the 32-wide step (zero beyond d).  qr: bf16(q') for the
  // reference segment; qo: bf16(q' o Ak) for the own segment, whose logits also get cown = q' . Sk (without tables qo is qr and cown is 0)
  const int tq = q0 + w * 16 + i;
  const int64_t qrow = (int64_t)b * N + min(tq, N - 1);
  bf16x8 qr[KK], qo[AFF ? KK : 1];
  float cown = 0.f;
  {
    const bf16_t* Qrow = (const bf16_t*)p.Q + qrow * p.ldq + hc;
    const int64_t trow = (int64_t)b * p.ldt + hc;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int col = kk * 32 + g * 8;
      union { uint4 u; bf16x8 v; } c;
      c.u = make_uint4(0, 0, 0, 0);
      if constexpr (AFF) qo[kk] = c.v;
      if (col < d) {
        if constexpr (AFF) {
          float x[8], t[8], y[8];
          load8(Qrow + col, x);
          load8f(p.Aq + trow + col, t);
          load8f(p.Sq + trow + col, y);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = __builtin_fmaf(t[e], x[e], y[e]);
          c.v = pack8(x);
          load8f(p.Sk + trow + col, y);
          load8f(p.Ak + trow + col, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            cown = __builtin_fmaf(x[e], y[e], cown);
            x[e] *= t[e];
          }
          qo[kk] = pack8(x);
        } else {
          c.u = *(const uint4*)(Qrow + col);
        }
      }
      qr[kk] = c.v;
    }
    if constexpr (AFF) {
      cown += __shfl_xor(cown, 16, 64);
      cown += __shfl_xor(cown, 32, 64);
    }
  }

  // staging state: piece w + 4 j of an image is this wave's; the lane's LDS slot there is row srow[j], chunk slot c % CPR, which holds source chunk scol[j] / 8
  int srow[PW], scol[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int c = (w + 4 * j) * 64 + lane, row = c / CPR;
    srow[j] = row;
    scol[j] = min((c - row * CPR) ^ row_sw<DP>(row), (d >> 3) - 1) * 8;
  }
  const int nkb = (N + KB - 1) / KB, ntot = bi ? 2 * nkb : nkb;      // (uniform) the reference itself walks its own keys only
  auto stage = [&](int t, char* dst) {      // walk block t (own rows, then the reference's) -> the (K, V) images at dst
    const bool ref = t >= nkb;
    const int k0 = (ref ? t - nkb : t) * KB;
    const bf16_t* const Ks = ref ? Kr : Kb;
    const bf16_t* const Vs = ref ? Vr : Vb;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int piece = w + 4 * j;
      if (piece < NP) {
        const int64_t row = min(k0 + srow[j], N - 1);
        glds16(Ks + row * p.ldk + scol[j], dst + piece * 1024);
        glds16(Vs + row * p.ldv + scol[j], dst + IMG + piece * 1024);
      }
    }
  };

  f32x4 acc[DF];
#pragma unroll
  for (int df = 0; df < DF; ++df) acc[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -1e30f, l = 0.f;      // running maximum of the raw logits of query i (all four g agree), this lane's share of the row sum
  const float sl2 = p.scale * LOG2E;
  const int troff = (8 * g + (i >> 2)) * NSTR + (i & 3) * 8;      // transposing-read lane offset inside an image
  const int tsw = row_sw<DP>(8 * g + (i >> 2)) >> 1;              // this lane's XOR on the 32-byte column block of a transposing read
  const bool ragged = (N & (KB - 1)) != 0;

  // one 64-key block of the walk: qf the segment's fragments, cadd its logit constant in units of the raw score (the scale multiplies both in the exponent)
  auto block = [&](const int t, const int kb, const bf16x8* qf, const float cadd) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // block t's images are in LDS; every wave is done with the other buffer
    asm volatile("" ::: "memory");
    const char* const Ks = smem + (t & 1) * 2 * IMG;
    const char* const Vs = Ks + IMG;
    if (t + 1 < ntot) stage(t + 1, smem + ((t & 1) ^ 1) * 2 * IMG);

    // S^T = K Q^T: lane (g, i) holds keys 64 kb + 32 (kf >> 1) + 8 g + 4 (kf & 1) + {0..3} of query i (attn.hip's permuted rows)
    f32x4 s[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s[kf] = (f32x4){cadd, cadd, cadd, cadd};
      const int krow = (kf >> 1) * 32 + prow(i, kf & 1);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const bf16x8 kfr = *(const bf16x8*)(Ks + krow * NSTR + (((kk * 4 + g) ^ row_sw<DP>(krow)) << 4));
        s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[kk], s[kf], 0, 0, 0);
      }
    }
    if (ragged && kb == nkb - 1) {      // the ragged last block of a segment (uniform): keys beyond the image
      const int k0 = kb * KB + g * 8;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + (kf >> 1) * 32 + (kf & 1) * 4 + e >= N) s[kf][e] = -1e30f;
    }
    float bmax = -1e30f;
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int e = 0; e < 4; ++e) bmax = fmaxf(bmax, s[kf][e]);
    bmax = fmaxf(bmax, __shfl_xor(bmax, 16, 64));
    bmax = fmaxf(bmax, __shfl_xor(bmax, 32, 64));
    const float mnew = fmaxf(m, bmax);      // finite: the block's key 0 exists
    const float alpha = __builtin_amdgcn_exp2f((m - mnew) * sl2), mn = mnew * sl2;
    m = mnew;
    float ls = 0.f;
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kf][e], sl2, -mn));
        s[kf][e] = pv;
        ls += pv;
      }
    l = __builtin_fmaf(l, alpha, ls);
#pragma unroll
    for (int df = 0; df < DF; ++df) acc[df] *= alpha;

    // O^T += V^T P^T (V read transposed from its natural image)
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      const bf16x8 pf = pack8(s[2 * sb], s[2 * sb + 1]);
#pragma unroll
      for (int df = 0; df < DF; ++df) {
        if (df * 16 < d) {
          const bf16x8 vf = lds_tr_frag(Vs + troff + sb * 32 * NSTR + ((df ^ tsw) << 5), NSTR);
          acc[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[df], 0, 0, 0);
        }
      }
    }
  };

  stage(0, smem);
  const bf16x8* const qown = AFF ? qo : qr;
  for (int t = 0; t < nkb; ++t) block(t, t, qown, cown);
  const float cref = p.shift / p.scale;
  for (int t = nkb; t < ntot; ++t) block(t, t - nkb, qr, cref);

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (tq < N) {
    const float inv = 1.0f / l;
    bf16_t* const Orow = (bf16_t*)p.O + qrow * p.ldo + hc;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      const int col = df * 16 + g * 4;
      if (col < d) {
        uint2 v;
        v.x = pack2bf(acc[df][0] * inv, acc[df][1] * inv);
        v.y = pack2bf(acc[df][2] * inv, acc[df][3] * inv);
        *(uint2*)(Orow + col) = v;
      }
    }
  }
}

template <int DP, bool AFF>
int attn_shared_launch(const sdlt_attn_shared_params& p, int nqb, unsigned nwg, hipStream_t s) {
  constexpr int smem = 4 * KB * tile_stride<DP>();
  if (sdlt_raise_smem((const void*)attn_shared_kernel<DP, AFF>, smem)) SDLT_FAIL(SDLT_ERR_LAUNCH, "sdlt_attn_shared_fwd: LDS attribute");
  hipLaunchKernelGGL((attn_shared_kernel<DP, AFF>), dim3(nwg), dim3(256), smem, s, p, nqb);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
template <bool AFF>
int attn_shared_by_d(const sdlt_attn_shared_params& p, int nqb, unsigned nwg, hipStream_t s) {
  return p.d <= 64 ? attn_shared_launch<64, AFF>(p, nqb, nwg, s) : p.d <= 96 ? attn_shared_launch<96, AFF>(p, nqb, nwg, s)
       : p.d <= 128 ? attn_shared_launch<128, AFF>(p, nqb, nwg, s) : attn_shared_launch<160, AFF>(p, nqb, nwg, s);
}

// [lo, hi) byte ranges of the operands
struct Span { uintptr_t lo, hi; };
Span span2d(const void* ptr, int64_t rows, int64_t ld, int64_t cols, int64_t esz) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)((rows - 1) * ld + cols) * esz}; }
bool overlaps(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

constexpr int SR = 256, SC = 64;      // rows and columns of one statistics chunk

// (mean, M2) of rows [256 chunk, +256) of 64 columns of one image -> ws[((b nch + chunk) 2 + {0, 1}) C2 + c]
__global__ __launch_bounds__(256) void adain_chunk_kernel(const sdlt_adain_affine_params p, const int nch) {
  __shared__ float red[32][SC + 1];
  __shared__ float cmean[SC];
  const int t = threadIdx.x, cs = t & 7, rs = t >> 3, chunk = blockIdx.y, b = blockIdx.z;
  const int col = blockIdx.x * SC + cs * 8, r0 = chunk * SR, nrow = min(SR, p.N - r0);
  const bool live = col < p.C2;
  const bf16_t* const X = (const bf16_t*)p.X + ((int64_t)b * p.N + r0) * p.ld + col;
  uint4 raw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = rs + 32 * j;
    raw[j] = live && row < nrow ? *(const uint4*)(X + (int64_t)row * p.ld) : make_uint4(0, 0, 0, 0);
  }
  float v[8], sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    load8((const bf16_t*)&raw[j], v);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] += v[e];      // (rows beyond the chunk are zeros)
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rs][cs * 8 + e] = sum[e];
  __syncthreads();
  if (t < SC) {
    float a = red[0][t];
    for (int r = 1; r < 32; ++r) a += red[r][t];
    cmean[t] = a / (float)nrow;
  }
  __syncthreads();
  float mu[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { mu[e] = cmean[cs * 8 + e]; sum[e] = 0.f; }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    load8((const bf16_t*)&raw[j], v);
    const bool in = rs + 32 * j < nrow;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dlt = in ? v[e] - mu[e] : 0.f;
      sum[e] = __builtin_fmaf(dlt, dlt, sum[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rs][cs * 8 + e] = sum[e];
  __syncthreads();
  const int c = blockIdx.x * SC + t;
  if (t < SC && c < p.C2) {
    float a = red[0][t];
    for (int r = 1; r < 32; ++r) a += red[r][t];
    float* const dst = p.ws + ((int64_t)b * nch + chunk) * 2 * p.C2 + c;
    dst[0] = cmean[t];
    dst[p.C2] = a;
  }
}

// the chunks of one image's column in ascending order (Chan's pairwise update) -> mean and std = sqrt(M2 / (N - 1) + 1e-5)
__device__ __forceinline__ void adain_stats(const float* ws, int N, int nch, int C2, float& mean, float& sd) {
  float mu = ws[0], m2 = ws[C2], na = (float)min(SR, N);
  for (int k = 1; k < nch; ++k) {
    const float nb = (float)min(SR, N - k * SR), dlt = ws[(int64_t)k * 2 * C2] - mu, nn = na + nb;
    mu += dlt * (nb / nn);
    m2 += ws[(int64_t)k * 2 * C2 + C2] + dlt * dlt * (na * nb / nn);
    na = nn;
  }
  mean = mu;
  sd = sqrtf(m2 / (float)(N - 1) + 1e-5f);
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void adain_finish_kernel(const sdlt_adain_affine_params p, const int nch) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, span = p.G * p.gs, r = (b / span) * span + b % p.gs;
  if (c >= p.C2) return;
  float a = 1.0f, s = 0.0f;
  if (b != r) {
    float mb, sb, mr, sr;
    adain_stats(p.ws + (int64_t)b * nch * 2 * p.C2 + c, p.N, nch, p.C2, mb, sb);
    adain_stats(p.ws + (int64_t)r * nch * 2 * p.C2 + c, p.N, nch, p.C2, mr, sr);
    a = sr / sb;
    s = mr - a * mb;
  }
  p.A[(int64_t)b * p.C2 + c] = a;
  p.S[(int64_t)b * p.C2 + c] = s;
}

}  // namespace

extern "C" int sdlt_adain_affine(const sdlt_adain_affine_params* pp, void* stream) {
  const char* fn = "sdlt_adain_affine";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_adain_affine_params& p = *pp;
  if (!p.X || !p.A || !p.S || !p.ws) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (X, A, S, ws are required)", fn);
  if (p.B < 1 || p.N < 2 || p.C2 < 1 || p.G < 1 || p.gs < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d N=%d C2=%d G=%d gs=%d (B, C2, G, gs >= 1; N >= 2: the variance divides by N - 1)", fn, p.B, p.N, p.C2, p.G, p.gs);
  if (p.B % ((int64_t)p.G * p.gs)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: %d interleaved group(s) of G=%d do not divide B=%d", fn, p.gs, p.G, p.B);
  if ((p.C2 % 8) || (p.ld % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: C2 %% 8, ld %% 8", fn);
  if (p.ld < p.C2) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < C2 = %d", fn, p.C2);
  if ((uintptr_t)p.X & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: X must be 16-byte aligned", fn);
  if (((uintptr_t)p.A | (uintptr_t)p.S | (uintptr_t)p.ws) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: A, S, ws must be 4-byte aligned", fn);
  const int nch = (p.N + SR - 1) / SR;
  if ((int64_t)p.B * p.N > INT_MAX || p.ld > INT_MAX || p.B > 65535 || nch > 65535 || (int64_t)p.B * nch * 2 * p.C2 > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d N=%d C2=%d: an index range exceeds its 32-bit (rows, workspace) or 16-bit (grid y, z) bound", fn, p.B, p.N, p.C2);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adain_chunk_kernel, dim3((p.C2 + SC - 1) / SC, nch, p.B), dim3(256), 0, s, p, nch);
  SDLT_CHECK_LAUNCH();
  hipLaunchKernelGGL(adain_finish_kernel, dim3((p.C2 + 255) / 256, p.B), dim3(256), 0, s, p, nch);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_attn_shared_fwd(const sdlt_attn_shared_params* pp, void* stream) {
  const char* fn = "sdlt_attn_shared_fwd";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_attn_shared_params& p = *pp;
  if (!p.Q || !p.K || !p.V || !p.O) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (Q, K, V, O are required)", fn);
  const int ntab = (p.Aq != nullptr) + (p.Sq != nullptr) + (p.Ak != nullptr) + (p.Sk != nullptr);
  if (ntab != 0 && ntab != 4) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: the tables Aq, Sq, Ak, Sk are given together or not at all (%d of 4)", fn, ntab);
  if (p.B < 1 || p.H < 1 || p.N < 1 || p.d < 1 || p.G < 1 || p.gs < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d N=%d d=%d G=%d gs=%d (all >= 1)", fn, p.B, p.H, p.N, p.d, p.G, p.gs);
  if (p.B % ((int64_t)p.G * p.gs)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: %d interleaved group(s) of G=%d do not divide B=%d", fn, p.gs, p.G, p.B);
  if (!(p.scale > 0.f) || !std::isfinite(p.scale) || !std::isfinite(p.shift))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: scale=%g shift=%g (scale > 0, both finite)", fn, (double)p.scale, (double)p.shift);
  if ((p.d % 8) || p.d > 160) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: d=%d (d %% 8 == 0, d <= 160)", fn, p.d);
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 8", fn);
  const int64_t C = (int64_t)p.H * p.d;
  if (p.ldq < C || p.ldk < C || p.ldv < C || p.ldo < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < H d = %lld", fn, (long long)C);
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Q, K, V, O must be 16-byte aligned", fn);
  if (ntab) {
    if (p.ldt < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ldt < H d = %lld", fn, (long long)C);
    if ((p.ldt % 4) || (((uintptr_t)p.Aq | (uintptr_t)p.Sq | (uintptr_t)p.Ak | (uintptr_t)p.Sk) & 15))
      SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ldt %% 4, Aq / Sq / Ak / Sk 16-byte aligned", fn);
  }
  // row indices (B N rows, the workgroup count, columns below ld) are 32-bit; row offsets into the tensors are 64-bit
  const int64_t M = (int64_t)p.B * p.N, nqb = ((int64_t)p.N + BM - 1) / BM, nwg = nqb * p.B * p.H;
  if (M > INT_MAX - KB || C > INT_MAX || nwg > INT_MAX || p.ldq > INT_MAX || p.ldk > INT_MAX || p.ldv > INT_MAX || p.ldo > INT_MAX || p.ldt > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d N=%d: a row index range exceeds 32 bits", fn, p.B, p.H, p.N);
  const Span o = span2d(p.O, M, p.ldo, C, 2);
  if (overlaps(o, span2d(p.Q, M, p.ldq, C, 2)) || overlaps(o, span2d(p.K, M, p.ldk, C, 2)) || overlaps(o, span2d(p.V, M, p.ldv, C, 2)))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: O overlaps an input", fn);
  hipStream_t s = (hipStream_t)stream;
  return ntab ? attn_shared_by_d<true>(p, (int)nqb, (unsigned)nwg, s) : attn_shared_by_d<false>(p, (int)nqb, (unsigned)nwg, s);
}
