// Tiled self-attention forward on MFMA (gfx950): "HyperTile".  The Hg x Wg token grid of every image is cut into ty x tx rectangular tiles of th x tw tokens
// (th = Hg / ty, tw = Wg / tx) and every token attends to the th tw tokens of its own tile only:
//   O[q] = softmax_k(scale Q[q] . K[k]) V[k]   over the keys k of q's tile,   token (y, x) of image b = row b Hg Wg + y Wg + x, tile (y / th, x / tw).
// Q, K, V, O bf16 token-major [B Hg Wg, ld], head hd in columns [hd d, (hd + 1) d), NO pad rows.  Forward only, no log-sum-exp: a render trains nothing.
//
// No gathered copy exists anywhere: the kernel walks the tile map itself.  A tile-local token t is row (tile_y th + t / tw) Wg + tile_x tw + t % tw of its image;
// the one division is paid once per lane, after which a lane's source row advances with its key block by a fixed (rows, columns) step and one conditional wrap.
// Work split: one workgroup of four waves per (image, head, tile, block of 64 tile-local queries); wave w owns queries [16 w, 16 w + 16) and keeps their Q
// fragments in registers.  All four waves need the same K / V head slices of the tile, so those go through LDS in blocks of 64 keys, filled by the 16-byte async
// global -> LDS copies (glds16) into one of two buffers: the copy of block j + 1 is issued before block j's arithmetic, and ONE barrier per block both publishes
// a buffer and retires the other (a buffer is refilled only after the barrier every wave passes once it has finished reading it).
// Workgroups are numbered (query block fastest, tile, head, image) and renumbered so that an XCD (one L2 each) runs a contiguous range of that order: the query
// blocks of one tile, which all stream the same K / V slices, share one L2 (attn.hip's xcd_wg arithmetic).
// A tile can hold thousands of keys, so the softmax is the online one: per 64-key block the running maximum m of the raw scores (the scale rides in the
// exponent's FMA), alpha = exp2((m_old - m_new) scale log2 e) rescales the lane's partial row sum and its O fragments, P goes to bf16 for the P V product.
// LDS rows: d <= 64 uses attn.hip's 128-byte rows with the 16-byte chunk index XOR-ed by row bits 1 and 3 - conflict-free for the permuted K fragment reads and
// for the transposing V reads alike (attn.hip has the bank arithmetic) - and the wider heads its +16-byte padded pitch.  Both are produced by the DMA itself: a
// lane's LDS slot is fixed (piece base + 16 lane), so the lane picks the SOURCE chunk that belongs there (the XOR-ed one; a pad slot re-reads a valid chunk).
// Rows and columns that do not exist are never read: tile-local queries and keys >= th tw read the tile's LAST token (such queries store nothing, such keys get
// a score of -1e30, P = 0), columns >= d the head's last chunk (Q is zero there, and those O columns are not stored).  Nothing outside the tile is read at all:
// NaN in another tile's K or V cannot reach this one.  fp32 scores, bf16 P, fp32 accumulation in ascending key blocks, one rounding at the store; no atomics,
// no workspace: two runs give the same bits.  DESIGN 4.39 has the compiler's resource figures.
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 64, KB = 64;      // queries per workgroup, keys per LDS block

// attn.hip's tile geometry (see the header comment)
template <int DP> __device__ __host__ constexpr int tile_stride() { return DP == 64 ? 128 : DP * 2 + 16; }
template <int DP> __device__ __forceinline__ int row_sw(int row) { return DP == 64 ? ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2)) : 0; }

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

// what the host derives from the parameter block once per launch
struct WinGeo {
  int th, tw, n;        // tile extent and its token count th tw
  int nqb, ntile;       // query blocks per tile, tiles per image
  unsigned adv, dx;     // a 64-token step inside a tile: row offset (64 / tw) Wg + 64 % tw and column 64 % tw, before the wrap
};

template <int DP>
__global__ __launch_bounds__(256) void attn_window_kernel(const sdlt_attn_window_params p, const WinGeo gm) {
  constexpr int NSTR = tile_stride<DP>(), CPR = NSTR / 16, IMG = KB * NSTR, NP = IMG / 1024, PW = (NP + 3) / 4, KK = DP / 32, DF = DP / 16;
  static_assert(IMG % 1024 == 0, "a K (or V) image of one key block is a whole number of 1 KB DMA pieces");
  __shared__ __attribute__((aligned(1024))) char smem[4 * IMG];      // two buffers of (K image, V image)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  const int n = gm.n, d = p.d;
  const unsigned tw = (unsigned)gm.tw, Wg = (unsigned)p.Wg;

  int L = blockIdx.x;
  {
    const int nwg = gridDim.x, k = L & 7, slot = L >> 3, q = nwg >> 3, r = nwg & 7;
    L = (k < r ? k * (q + 1) : r * (q + 1) + (k - r) * q) + slot;
  }
  const int rest = L / gm.nqb, q0 = (L - rest * gm.nqb) * BM, bh = rest / gm.ntile, tile = rest - bh * gm.ntile;
  const int b = bh / p.H, hc = (bh - b * p.H) * d, tyi = tile / p.tx, txi = tile - tyi * p.tx;
  // row of the tile's token 0; offsets inside the tile stay below Hg Wg and are formed in wrapping unsigned arithmetic
  const int64_t row0 = (int64_t)b * p.Hg * p.Wg + (int64_t)tyi * gm.th * p.Wg + (int64_t)txi * gm.tw;
  const unsigned last_off = (unsigned)(gm.th - 1) * Wg + tw - 1u;
  const bf16_t* const Kt = (const bf16_t*)p.K + row0 * p.ldk + hc;
  const bf16_t* const Vt = (const bf16_t*)p.V + row0 * p.ldv + hc;

  // this lane's query: tile-local q0 + 16 w + i (beyond the tile: its last token, nothing stored)
  const int tq = q0 + w * 16 + i;
  unsigned qoff;
  {
    const unsigned t = (unsigned)min(tq, n - 1), y = t / tw;
    qoff = y * Wg + (t - y * tw);
  }
  // Q fragments: B operands of the 16x16x32 MFMA, lane (g, i) = query i, 8 columns from 8 g of the 32-wide step (zero beyond d)
  bf16x8 qf[KK];
  {
    const bf16_t* Qrow = (const bf16_t*)p.Q + (row0 + qoff) * p.ldq + hc;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int col = kk * 32 + g * 8;
      union { uint4 u; bf16x8 v; } c;
      c.u = col < d ? *(const uint4*)(Qrow + col) : make_uint4(0, 0, 0, 0);
      qf[kk] = c.v;
    }
  }

  // staging state: piece w + 4 j of an image is this wave's; the lane's LDS slot there is row srow[j], chunk slot c % CPR, which holds source chunk scol[j] / 8;
  // (sx, soff) = column and row offset inside the tile of token 64 kb + srow[j], advanced with kb
  int srow[PW], scol[PW];
  unsigned sx[PW], soff[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int c = (w + 4 * j) * 64 + lane, row = c / CPR;
    srow[j] = row;
    scol[j] = min((c - row * CPR) ^ row_sw<DP>(row), (d >> 3) - 1) * 8;
    const unsigned y = (unsigned)row / tw;
    sx[j] = (unsigned)row - y * tw;
    soff[j] = y * Wg + sx[j];
  }
  auto stage = [&](int kb, char* dst) {      // key block kb -> the (K, V) images at dst, then the state moves on to kb + 1
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int piece = w + 4 * j;
      if (piece < NP) {
        const unsigned off = kb * KB + srow[j] < n ? soff[j] : last_off;
        glds16(Kt + (int64_t)off * p.ldk + scol[j], dst + piece * 1024);
        glds16(Vt + (int64_t)off * p.ldv + scol[j], dst + IMG + piece * 1024);
      }
      sx[j] += gm.dx;
      soff[j] += gm.adv;
      if (sx[j] >= tw) { sx[j] -= tw; soff[j] += Wg - tw; }
    }
  };

  f32x4 acc[DF];
#pragma unroll
  for (int df = 0; df < DF; ++df) acc[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -1e30f, l = 0.f;      // running maximum of the raw scores of query i (all four g agree), this lane's share of the row sum
  const float sl2 = p.scale * LOG2E;
  const int troff = (8 * g + (i >> 2)) * NSTR + (i & 3) * 8;      // transposing-read lane offset inside an image
  const int tsw = row_sw<DP>(8 * g + (i >> 2)) >> 1;              // this lane's XOR on the 32-byte column block of a transposing read
  const int nkb = (n + KB - 1) / KB;

  stage(0, smem);
  for (int kb = 0, buf = 0; kb < nkb; ++kb, buf ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // block kb's images are in LDS; every wave is done with the other buffer
    asm volatile("" ::: "memory");
    const char* const Ks = smem + buf * 2 * IMG;
    const char* const Vs = Ks + IMG;
    if (kb + 1 < nkb) stage(kb + 1, smem + (buf ^ 1) * 2 * IMG);

    // S^T = K Q^T: lane (g, i) holds keys 64 kb + 32 (kf >> 1) + 8 g + 4 (kf & 1) + {0..3} of query i (attn.hip's permuted rows)
    f32x4 s[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s[kf] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const int krow = (kf >> 1) * 32 + prow(i, kf & 1);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const bf16x8 kfr = *(const bf16x8*)(Ks + krow * NSTR + (((kk * 4 + g) ^ row_sw<DP>(krow)) << 4));
        s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[kk], s[kf], 0, 0, 0);
      }
    }
    if (kb == nkb - 1 && (n & (KB - 1))) {      // the ragged last block (uniform): keys beyond the tile
      const int k0 = kb * KB + g * 8;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + (kf >> 1) * 32 + (kf & 1) * 4 + e >= n) s[kf][e] = -1e30f;
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
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (tq < n) {
    const float inv = 1.0f / l;
    bf16_t* const Orow = (bf16_t*)p.O + (row0 + qoff) * p.ldo + hc;
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

template <int DP>
int attn_window_launch(const sdlt_attn_window_params& p, const WinGeo& gm, unsigned nwg, hipStream_t s) {
  hipLaunchKernelGGL((attn_window_kernel<DP>), dim3(nwg), dim3(256), 0, s, p, gm);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

// [lo, hi) byte ranges of the operands
struct Span { uintptr_t lo, hi; };
Span span2d(const void* ptr, int64_t rows, int64_t ld, int64_t cols) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)((rows - 1) * ld + cols) * 2}; }
bool overlaps(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int sdlt_attn_window_fwd(const sdlt_attn_window_params* pp, void* stream) {
  const char* fn = "sdlt_attn_window_fwd";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_attn_window_params& p = *pp;
  if (!p.Q || !p.K || !p.V || !p.O) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (Q, K, V, O are required)", fn);
  if (p.B < 1 || p.H < 1 || p.Hg < 1 || p.Wg < 1 || p.ty < 1 || p.tx < 1 || p.d < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d Hg=%d Wg=%d ty=%d tx=%d d=%d (all >= 1)", fn, p.B, p.H, p.Hg, p.Wg, p.ty, p.tx, p.d);
  if (p.Hg % p.ty || p.Wg % p.tx) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: %d x %d tiles do not divide the %d x %d token grid", fn, p.ty, p.tx, p.Hg, p.Wg);
  if ((p.d % 8) || p.d > 96) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: d=%d (d %% 8 == 0, d <= 96)", fn, p.d);
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 8", fn);
  const int64_t C = (int64_t)p.H * p.d;
  if (p.ldq < C || p.ldk < C || p.ldv < C || p.ldo < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < H d = %lld", fn, (long long)C);
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Q, K, V, O must be 16-byte aligned", fn);
  // row indices (B Hg Wg rows, the workgroup count, columns below ld) are 32-bit; row offsets into the tensors are 64-bit
  const int64_t HW = (int64_t)p.Hg * p.Wg, M = HW <= INT_MAX ? p.B * HW : HW, n = (int64_t)(p.Hg / p.ty) * (p.Wg / p.tx), nqb = (n + BM - 1) / BM;
  const int64_t nwg = M <= INT_MAX ? (int64_t)p.B * p.ty * p.tx * nqb * p.H : M;      // (B ty tx nqb <= M: the product stays inside 64 bits)
  if (M > INT_MAX - KB || C > INT_MAX || nwg > INT_MAX || p.ldq > INT_MAX || p.ldk > INT_MAX || p.ldv > INT_MAX || p.ldo > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d Hg=%d Wg=%d ty=%d tx=%d: a row index range exceeds 32 bits", fn, p.B, p.H, p.Hg, p.Wg, p.ty, p.tx);
  const Span o = span2d(p.O, M, p.ldo, C);
  if (overlaps(o, span2d(p.Q, M, p.ldq, C)) || overlaps(o, span2d(p.K, M, p.ldk, C)) || overlaps(o, span2d(p.V, M, p.ldv, C)))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: O overlaps an input", fn);
  WinGeo gm;
  gm.th = p.Hg / p.ty; gm.tw = p.Wg / p.tx; gm.n = (int)n; gm.nqb = (int)nqb; gm.ntile = p.ty * p.tx;
  gm.dx = (unsigned)(KB % gm.tw);
  gm.adv = (unsigned)(KB / gm.tw) * (unsigned)p.Wg + gm.dx;
  hipStream_t s = (hipStream_t)stream;
  return p.d <= 64 ? attn_window_launch<64>(p, gm, (unsigned)nwg, s) : attn_window_launch<96>(p, gm, (unsigned)nwg, s);
}
