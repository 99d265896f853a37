// Normalized attention guidance (NAG, Chen et al. 2025) as ONE cross-attention forward on MFMA (gfx950): the negative prompt acts inside the attention.
// For batch row b with m = neg_row[b] in [0, B), query i, over the whole C = H d wide row (all heads):
//   z+ = softmax(scale q K[b]^T) V[b],  z- = softmax(scale q K[m]^T) V[m]  (the same queries),  e = s z+ - (s - 1) z-,
//   n+ = sum_c |z+|,  ne = sum_c |e|,  c = ne <= tau n+ ? 1 : tau n+ / ne,  O = (1 - alpha) z+ + alpha c e.
// Rows with neg_row[b] outside [0, B), and every row when the table row has alpha == 0 or s == 1, get O = z+: plain attention, no second softmax, no
// exchange (the branch is uniform per workgroup).  (s, tau, alpha) = row clamp(ctr[0], 0, tab_rows - 1) of tab (fp32 [tab_rows, 4]); a null ctr means row 0.
// Q, O bf16 token-major [B Nq, ld], head h in columns [h d, (h + 1) d), NO pad rows; K, V bf16 [B Nkp, ld], keys [0, Nk) of a row valid, Nk <= 128.
//
// Work split: the norms run over ALL heads of a token, so one workgroup owns 16 query rows (one MFMA M tile) for all heads.  Its four waves split the HEADS:
// wave w takes heads w, w + 4, ... (NH per wave at most) and keeps the fp32 z+ and z- accumulators of all of them in registers until the norms are known -
// NH DP / 2 registers per lane, 160 at the deepest (5 heads of 64 columns, 2 heads of 160); one wave per SIMD, so the whole register file is the wave's.
// K and V: every wave walks its own heads, so each wave owns a private LDS RING of 32-key tiles (K tiles, then V tiles, of the positive and then the
// negative prompt of head after head: one tile sequence per wave).  Tiles are filled by the 16-byte async global -> LDS copies with NBUF - 1 tiles in flight
// ahead of the one being read; the consumer waits on its own vmcnt only - the waves never meet at a barrier in the head loop.  The positive and the negative
// pass share the ring (a 32-key tile is 4 - 11 KB; four whole K+ V+ K- V- images per wave would be 64 KB and more).  Beyond the last tile the producer
// re-stages the last one, so the in-flight count the consumer waits on stays constant.  The key sets are small (77 rows x C) and stay in L2.
// Scores: key-major S^T = K Q^T on v_mfma_f32_16x16x32_bf16 with attn.hip's permuted key rows, so the probabilities land in the B-operand layout of
// O^T = V^T P^T (V read transposed from its natural tile) without an LDS round trip.  All (<= 128) scores of a query stay in registers: exact softmax, one max,
// one sum, no online rescale.  LDS rows as in attn_couple.hip: 128-byte rows with an XOR swizzle at DP = 64, a +16-byte padded pitch above; the DMA lane
// picks the source chunk that belongs in its slot.
// Norm hand-off: every wave sums |z+| and |e| of its heads per query (in-lane in a fixed order, then across the four lane groups), the four waves exchange
// 16 x 2 floats through LDS at ONE barrier and add them in wave order 0..3; every wave then forms c and stores its heads' columns of O once, as bf16 (8-byte
// stores: the transposed accumulator layout gives a lane four neighbouring columns).  No workspace, no atomics, no second launch: two runs give the same bits.
// Rows and columns that do not exist are never read: query rows >= Nq and key rows >= Nk re-read the last valid row, columns >= d the head's last chunk (Q is
// zero there; those columns enter neither the norms nor the store).  DESIGN 4.43 has the compiler's resource figures.
#include <climits>
#include <cmath>
#include <utility>
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int BM = 16, HMAX = 20, NKMAX = 128, TR = 32;

// attn.hip's tile geometry
template <int DP> __device__ __host__ constexpr int tile_stride() { return DP == 64 ? 128 : DP * 2 + 16; }
template <int DP> __device__ __forceinline__ int row_sw(int row) { return DP == 64 ? ((((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2)) : 0; }
// one 32-key tile in whole 1 KB DMA pieces, and the ring depth: about 32 KB per wave
template <int DP> __device__ __host__ constexpr int tile_bytes() { return (TR * tile_stride<DP>() + 1023) & ~1023; }
template <int DP> __device__ __host__ constexpr int ring_depth() { return DP == 64 ? 8 : DP == 96 ? 4 : 3; }
template <int DP> __device__ __host__ constexpr int lds_bytes() { return 4 * ring_depth<DP>() * tile_bytes<DP>() + 4 * BM * 2 * 4; }

__device__ __forceinline__ int prow(int i, int half) { return ((i >> 2) << 3) + half * 4 + (i & 3); }
__device__ __forceinline__ bf16x8 pack8(const f32x4 a, const f32x4 b) {
  union { uint4 u; bf16x8 v; } c;
  c.u.x = pack2bf(a[0], a[1]); c.u.y = pack2bf(a[2], a[3]);
  c.u.z = pack2bf(b[0], b[1]); c.u.w = pack2bf(b[2], b[3]);
  return c.v;
}
// Every LDS fragment read of the head loop is inline asm with a hand-placed s_waitcnt lgkmcnt, as in attn32.hip: hipcc puts an s_waitcnt vmcnt(0) in front
// of a compiler-visible LDS read that follows an LDS-DMA (it cannot prove that the read does not alias a tile in flight), which would wait for the whole
// ring at every tile.  A tile's reads are issued together and waited for once; `pin` makes their consumers depend on the wait (volatile asms keep their order).
__device__ __forceinline__ uint32_t lds_addr(const char* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p; }
__device__ __forceinline__ bf16x8 lds_b128(uint32_t a) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a));
  return v;
}
// half of an MFMA fragment contracted over the ROW axis of a row-major bf16 LDS tile (attn.hip's lds_tr_frag: lane (g, i) receives rows r0 + 8 g + {0..7} of
// column c0 + i from the reads at p and p + 4 rows)
template <int OFF>
__device__ __forceinline__ bf16x4 lds_tr(uint32_t a) {
  bf16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF));
  return v;
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void pin(bf16x8& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(bf16x4& v) { asm volatile("" : "+v"(v)); }

// The producer's place in the wave's tile sequence: head slot hh, pass (0 positive, 1 negative), v (0 a K tile, 1 a V tile), 32-key block kb, ring slot.
struct Cursor { int hh, pass, v, kb, slot; };
// f(integral_constant 0), f(1), ...: the head slots as compile-time indices - the accumulators of every head are registers, never an indexed array
template <class F, int... I>
__device__ __forceinline__ void for_heads(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }

template <int DP, int NH>
__global__ __launch_bounds__(256) void attn_nag_kernel(const sdlt_attn_nag_params p, const int ntile) {
  constexpr int NSTR = tile_stride<DP>(), KK = DP / 32, DF = DP / 16, TB = tile_bytes<DP>(), PIECES = TB / 1024, NBUF = ring_depth<DP>(), CPR = NSTR / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, i = lane & 15;
  const int Nq = p.Nq, Nk = p.Nk, d = p.d, H = p.H, dch = d >> 3;
  const int nkb = (Nk + TR - 1) / TR;
  const int b = blockIdx.x / ntile, q0 = (blockIdx.x - b * ntile) * BM;
  const int q = q0 + i, qr = min(q, Nq - 1);
  const int nh = w < H ? (H - w + 3) >> 2 : 0;      // heads of this wave: w, w + 4, ...
  char* const ring = smem + w * NBUF * TB;
  float* const nx = (float*)(smem + 4 * NBUF * TB);      // [4 waves][16 queries][n+, ne]

  // the step's setting and this row's negative: uniform in the workgroup
  int trow = 0;
  if (p.ctr) trow = max(0, min(__builtin_amdgcn_readfirstlane(p.ctr[0]), p.tab_rows - 1));
  const float gs = p.tab[trow * 4], tau = p.tab[trow * 4 + 1], alpha = p.tab[trow * 4 + 2];
  int m = __builtin_amdgcn_readfirstlane(p.neg_row[b]);
  const bool nag = m >= 0 && m < p.B && alpha != 0.f && gs != 1.f;
  if (!nag) m = b;
  const int npass = nag ? 2 : 1;

  // producer: stage the cursor's tile into its ring slot and step the cursor; at the end of the sequence it stays on the last tile (re-staged, never read)
  Cursor pc = {0, 0, 0, 0, 0};
  auto stage = [&]() __attribute__((always_inline)) {
    const int64_t ld = pc.v ? p.ldv : p.ldk;
    const bf16_t* const src = (const bf16_t*)(pc.v ? p.V : p.K) + (int64_t)(pc.pass ? m : b) * p.Nkp * ld + (w + 4 * pc.hh) * d;
    char* const dst = ring + pc.slot * TB;
#pragma unroll
    for (int piece = 0; piece < PIECES; ++piece) {
      const int c = piece * 64 + lane, row = c / CPR;
      const int ch = min((c - row * CPR) ^ row_sw<DP>(row), dch - 1), srow = min(pc.kb * TR + row, Nk - 1);
      glds16(src + (int64_t)srow * ld + ch * 8, dst + piece * 1024);
    }
    pc.slot = pc.slot + 1 == NBUF ? 0 : pc.slot + 1;
    const bool last = pc.kb + 1 == nkb && pc.v == 1 && pc.pass + 1 == npass && pc.hh + 1 == nh;
    if (!last) {
      if (++pc.kb == nkb) {
        pc.kb = 0;
        if (++pc.v == 2) {
          pc.v = 0;
          if (++pc.pass == npass) { pc.pass = 0; ++pc.hh; }
        }
      }
    }
  };
  // consumer: refill the slot read last (its reads were waited for: wait_lgkm0 follows every tile's reads), then wait until the oldest tile in flight has landed
  // (vmcnt counts EVERY outstanding vector-memory operation of the wave in issue order: any other one issued after that tile - here the next head's Q loads -
  // only makes the wait longer, never shorter, so the count below is safe whatever else the head loop loads)
  int cslot = 0;
  const uint32_t ring_a = lds_addr(ring);
  auto next_tile = [&]() __attribute__((always_inline)) -> uint32_t {
    stage();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 1) * PIECES) : "memory");
    const uint32_t t = ring_a + cslot * TB;
    cslot = cslot + 1 == NBUF ? 0 : cslot + 1;
    return t;
  };

  f32x4 zp[NH][DF], zn[NH][DF];
  const float sl2 = p.scale * LOG2E;
  const int troff = (8 * g + (i >> 2)) * NSTR + (i & 3) * 8;      // transposing-read lane offset inside a tile
  const int tsw = row_sw<DP>(8 * g + (i >> 2)) >> 1;              // this lane's XOR on the 32-byte column block of a transposing read
  const int koff[2] = {prow(i, 0) * NSTR, prow(i, 1) * NSTR}, ksw[2] = {row_sw<DP>(prow(i, 0)), row_sw<DP>(prow(i, 1))};      // the lane's two key rows of a K tile

  // Q fragments of head slot hh: B operands of the 16x16x32 MFMA, lane (g, i) = query i, 8 columns from 8 g of the 32-wide step (zero beyond d)
  auto load_q = [&](bf16x8 (&qf)[KK], int hh) __attribute__((always_inline)) {
    const bf16_t* Qrow = (const bf16_t*)p.Q + ((int64_t)b * Nq + qr) * p.ldq + (w + 4 * hh) * d;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int col = kk * 32 + g * 8;
      union { uint4 u; bf16x8 v; } c;
      c.u = col < d ? *(const uint4*)(Qrow + col) : make_uint4(0, 0, 0, 0);
      qf[kk] = c.v;
    }
  };
  // one softmax(scale q K^T) V of the head in qf over the next 2 nkb tiles of the sequence -> z
  auto attend = [&](f32x4 (&z)[DF], const bf16x8 (&qf)[KK]) __attribute__((always_inline)) {
    // S^T = K Q^T: lane (g, i) holds keys 32 (kf >> 1) + 8 g + 4 (kf & 1) + {0..3} of query i (attn.hip's permuted rows)
    f32x4 s[8];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[2 * kb] = s[2 * kb + 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (kb < nkb) {
        const uint32_t Ks = next_tile();
        bf16x8 kfr[2][KK];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) kfr[half][kk] = lds_b128(Ks + koff[half] + (((kk * 4 + g) ^ ksw[half]) << 4));
        wait_lgkm0();
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
            pin(kfr[half][kk]);
            s[2 * kb + half] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[half][kk], qf[kk], s[2 * kb + half], 0, 0, 0);
          }
      }
    }
    // exact softmax over the whole key row: raw scores, the scale rides in the exponent's FMA
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
    const float inv = 1.f / l;
    // z^T = V^T P^T (V read transposed from its natural tile), then z /= l
#pragma unroll
    for (int df = 0; df < DF; ++df) z[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb < nkb) {
        const uint32_t Vs = next_tile() + troff;
        const bf16x8 pf = pack8(s[2 * kb], s[2 * kb + 1]);
        bf16x4 vlo[DF], vhi[DF];
#pragma unroll
        for (int df = 0; df < DF; ++df)
          if (df * 16 < d) {
            vlo[df] = lds_tr<0>(Vs + ((df ^ tsw) << 5));
            vhi[df] = lds_tr<4 * NSTR>(Vs + ((df ^ tsw) << 5));
          }
        wait_lgkm0();
#pragma unroll
        for (int df = 0; df < DF; ++df)
          if (df * 16 < d) {
            pin(vlo[df]);
            pin(vhi[df]);
            z[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_shufflevector(vlo[df], vhi[df], 0, 1, 2, 3, 4, 5, 6, 7), pf, z[df], 0, 0, 0);
          }
      }
    }
#pragma unroll
    for (int df = 0; df < DF; ++df) z[df] *= inv;
  };

  if (nh > 0) {
    bf16x8 qf[KK], qn[KK];
    load_q(qf, 0);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) pin(qf[kk]);      // (waited for here, before the ring fills: hipcc waits for a plain load behind LDS-DMAs with vmcnt(0), at every use)
    for (int j = 0; j < NBUF - 1; ++j) stage();
    for_heads([&](auto hc) __attribute__((always_inline)) {
      constexpr int hh = decltype(hc)::value;
      if (hh < nh) {
        if (hh + 1 < nh) load_q(qn, hh + 1);      // (a head ahead: the wait on it does not drain the ring)
        attend(zp[hh], qf);
        if (nag) attend(zn[hh], qf);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
          if (hh + 1 < nh) {
            qf[kk] = qn[kk];
            pin(qf[kk]);      // (the one wait for the next head's Q: once per head, not at every K tile)
          }
      }
    }, std::make_integer_sequence<int, NH>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the re-staged tail tiles: nothing lands in LDS after this wave is done

  float cc = 1.f;
  if (nag) {
    float np_ = 0.f, ne_ = 0.f;
#pragma unroll
    for (int hh = 0; hh < NH; ++hh)
      if (hh < nh) {
#pragma unroll
        for (int df = 0; df < DF; ++df)
          if (df * 16 + g * 4 < d) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float a = zp[hh][df][e], ev = gs * a - (gs - 1.f) * zn[hh][df][e];
              np_ += fabsf(a);
              ne_ += fabsf(ev);
            }
          }
      }
    np_ += __shfl_xor(np_, 16, 64); np_ += __shfl_xor(np_, 32, 64);
    ne_ += __shfl_xor(ne_, 16, 64); ne_ += __shfl_xor(ne_, 32, 64);
    if (g == 0) { nx[(w * BM + i) * 2] = np_; nx[(w * BM + i) * 2 + 1] = ne_; }
    __syncthreads();
    float P = 0.f, E = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) { P += nx[(ww * BM + i) * 2]; E += nx[(ww * BM + i) * 2 + 1]; }      // wave order 0..3 in every wave
    const float lim = tau * P;
    cc = E <= lim ? 1.f : lim / E;
  }

  if (q < Nq) {
    const float ca = 1.f - alpha, cb = alpha * cc;
#pragma unroll
    for (int hh = 0; hh < NH; ++hh)
      if (hh < nh) {
        bf16_t* const Orow = (bf16_t*)p.O + ((int64_t)b * Nq + q) * p.ldo + (w + 4 * hh) * d;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
          const int col = df * 16 + g * 4;
          if (col < d) {
            f32x4 o = zp[hh][df];
            if (nag) {
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = ca * o[e] + cb * (gs * o[e] - (gs - 1.f) * zn[hh][df][e]);
            }
            uint2 v;
            v.x = pack2bf(o[0], o[1]);
            v.y = pack2bf(o[2], o[3]);
            *(uint2*)(Orow + col) = v;
          }
        }
      }
  }
}

int nag_dp(int d) {      // attn.hip's attn_dp
  if (d <= 0 || (d % 8)) return -1;
  return d <= 64 ? 64 : d <= 96 ? 96 : d <= 128 ? 128 : d <= 160 ? 160 : -1;
}
// heads per wave the register file holds at padded width dp: NH dp / 2 accumulator registers per lane, 160 at the most
int nag_nh_max(int dp) { return dp == 64 ? 5 : dp == 96 ? 3 : 2; }

template <int DP, int NH>
int attn_nag_launch(const sdlt_attn_nag_params& p, hipStream_t s) {
  const int ntile = (p.Nq + BM - 1) / BM;
  if (sdlt_raise_smem((const void*)attn_nag_kernel<DP, NH>, lds_bytes<DP>())) SDLT_FAIL(SDLT_ERR_LAUNCH, "sdlt_attn_nag_fwd: LDS attribute");
  hipLaunchKernelGGL((attn_nag_kernel<DP, NH>), dim3((unsigned)(p.B * ntile)), dim3(256), lds_bytes<DP>(), s, p, ntile);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

// [lo, hi) byte ranges of the operands
struct Span { uintptr_t lo, hi; };
Span span2d(const void* ptr, int64_t rows, int64_t ld, int64_t cols, int elt) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)((rows - 1) * ld + cols) * elt}; }
bool overlaps(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" int sdlt_attn_nag_fwd(const sdlt_attn_nag_params* pp, void* stream) {
  const char* fn = "sdlt_attn_nag_fwd";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_attn_nag_params& p = *pp;
  if (!p.Q || !p.K || !p.V || !p.O || !p.neg_row || !p.tab) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (Q, K, V, O, neg_row, tab are required)", fn);
  if (p.B < 1 || p.H < 1 || p.Nq < 1 || p.Nk < 1 || p.d < 1 || p.tab_rows < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d H=%d Nq=%d Nk=%d d=%d tab_rows=%d (all >= 1)", fn, p.B, p.H, p.Nq, p.Nk, p.d, p.tab_rows);
  if (p.H > HMAX || p.Nk > NKMAX || p.Nkp < p.Nk) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: H=%d (<= %d) Nk=%d (<= %d) Nkp=%d (>= Nk)", fn, p.H, HMAX, p.Nk, NKMAX, p.Nkp);
  if (p.Nkp % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Nkp=%d %% 8", fn, p.Nkp);
  const int dp = nag_dp(p.d);
  if (dp < 0) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: d=%d (d %% 8 == 0, d <= 160)", fn, p.d);
  const int nh = (p.H + 3) / 4;
  if (nh > nag_nh_max(dp))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: H=%d heads of d=%d: a wave keeps %d heads' accumulators in registers at this width (H <= %d)", fn, p.H, p.d, nag_nh_max(dp), 4 * nag_nh_max(dp));
  if ((p.ldq % 8) || (p.ldk % 8) || (p.ldv % 8) || (p.ldo % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ld %% 8", fn);
  const int64_t C = (int64_t)p.H * p.d;
  if (p.ldq < C || p.ldk < C || p.ldv < C || p.ldo < C) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld < H d = %lld", fn, (long long)C);
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: Q, K, V, O must be 16-byte aligned", fn);
  if (((uintptr_t)p.neg_row | (uintptr_t)p.tab | (uintptr_t)p.ctr) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: neg_row, tab, ctr must be 4-byte aligned", fn);
  // in-row indices (queries up to Nq + 15, columns below ld, the grid B ceil(Nq / 16)) are 32-bit; row offsets into the tensors are 64-bit
  const int64_t ntile = ((int64_t)p.Nq + BM - 1) / BM;
  if (p.Nq > INT_MAX - BM || (int64_t)p.B * ntile > INT_MAX || (int64_t)p.B * p.Nq > INT_MAX || (int64_t)p.B * p.Nkp > INT_MAX || p.tab_rows > INT_MAX / 4 ||
      p.ldq > INT_MAX || p.ldk > INT_MAX || p.ldv > INT_MAX || p.ldo > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d Nq=%d Nkp=%d tab_rows=%d: an index range exceeds 32 bits", fn, p.B, p.Nq, p.Nkp, p.tab_rows);
  const Span o = span2d(p.O, (int64_t)p.B * p.Nq, p.ldo, C, 2);
  if (overlaps(o, span2d(p.Q, (int64_t)p.B * p.Nq, p.ldq, C, 2)) || overlaps(o, span2d(p.K, (int64_t)p.B * p.Nkp, p.ldk, C, 2)) ||
      overlaps(o, span2d(p.V, (int64_t)p.B * p.Nkp, p.ldv, C, 2)) || overlaps(o, span2d(p.neg_row, 1, p.B, p.B, 4)) ||
      overlaps(o, span2d(p.tab, p.tab_rows, 4, 4, 4)) || (p.ctr && overlaps(o, span2d(p.ctr, 1, 1, 1, 4))))
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: O overlaps an input", fn);
  hipStream_t s = (hipStream_t)stream;
  if (dp == 64) return nh <= 2 ? attn_nag_launch<64, 2>(p, s) : attn_nag_launch<64, 5>(p, s);
  if (dp == 96) return attn_nag_launch<96, 3>(p, s);
  return dp == 128 ? attn_nag_launch<128, 2>(p, s) : attn_nag_launch<160, 2>(p, s);
}
