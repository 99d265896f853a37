// Token merging for self-attention ("ToMe": Bolya & Hoffman, "Token Merging for Fast Stable Diffusion"; unet.py: UNet.set_token_merge), four launches:
//   sdlt_tome_match    every source token's most cosine-similar destination token: one MFMA kernel with a running (max, argmax) in registers
//   sdlt_tome_plan     the r best-matched sources are merged: map, kept_tok and a CSR of merged sources per destination, exact integer work
//   sdlt_tome_merge    ym = the kept rows, a destination's row being the mean of itself and its merged sources
//   sdlt_tome_unmerge  out[t] = residual[t] + a[map[t]]
// The Hg x Wg token grid (both even) is cut into 2 x 2 cells; each cell gives ONE destination token (fixed: its top-left; random: the token at offset
// philox(seed, ctr[0], layer, cell) & 3, the same for every image), destinations in cell raster order, the other 3 N / 4 tokens are sources in ascending
// token index.  include/sdlt_kernels.h has the contract, DESIGN 4.40 the budget.
//
// MATCH.  s(i, j) = dot(y_i, y_j) inv_i inv_j, inv = 1 / sqrt(sum y^2) in fp32 (0 for a zero row), bf16 products accumulated in fp32.  No [N_src, N_dst]
// buffer exists: a workgroup of four waves owns a strip of 32 source rows of one image and walks the destinations 256 at a time - wave w owns destination
// block 256 it + 64 w, so the destination range is split over the waves of a workgroup, not over workgroups, and no partial result ever goes through
// memory (at B = 2, N = 4096 that is 192 workgroups of four waves for 256 CUs).  K goes through LDS in chunks of 64 columns: the 32 source rows (4 KB,
// read by every wave) and the 4 x 64 destination rows (32 KB), gathered BY TOKEN INDEX while staging - nothing is copied.  The loads of step n + 1 are
// in registers while step n's MFMAs run (9 x 16 bytes per lane); LDS rows are 128 bytes with the 16-byte chunk index XOR-ed by the row's low three bits,
// so the 16 rows of a fragment read hit 8 distinct bank groups.  Per chunk a wave issues 2 (source fragments) x 4 (destination tiles) x 2 (k steps)
// v_mfma_f32_16x16x32_bf16 with the destinations as the A operand: lane (g, i) then holds the scores of destinations 4 g + {0..3} of a tile against
// source i, so the running (max, argmax) of a source is per-lane state and needs no cross-lane work until the very end.  sum y^2 of both sides comes
// from the same fragments on the packed bf16 dot product (exact products, fp32 sums) - no pre-pass over y, no buffer of norms.  After a destination block:
// column scale by inv_j, fold in ascending j with a strict >, so ties keep the lowest j.  At the end: the four g of a source, then the four waves through LDS,
// combine with (larger score, then lower index) - a total order, so the result does not depend on how the range was split - and inv_i is applied once.
// The source token table (ascending non-destination tokens) has no closed form in random mode; the index launch in front leaves it in node_idx[b, i],
// which the owning workgroup - the only one that touches those entries - reads at its start and overwrites with the result at its end.
#include <climits>
#include <cmath>
#include "common.h"
#include "philox.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr uint32_t TOME_TAG = 0x544F4D31u;      // counter word 3 of the destination draw
constexpr int SB = 32, DBW = 64, DB = 4 * DBW, KC = 64;      // source rows per workgroup, destination rows per wave and per workgroup step, columns per chunk
constexpr int TOME_MAX_N = 16384;

// ---------------------------------------------------------------------------------------------------------------- index launch
// One workgroup per cell row (token rows 2 cy, 2 cy + 1): the cells' destinations, then the sources of the row pair in ascending token order, which start at
// source index 3 cy Wc.  off[] holds the cell's offset (dy = off >> 1, dx = off & 1); top[] the running count of destinations in the top row.
struct IndexArgs {
  const int32_t* ctr; int32_t* dst_tok; int32_t* node_idx;
  uint32_t k0, k1;
  int B, Hg, Wg, mode, layer;
};

__global__ __launch_bounds__(256) void tome_index_kernel(IndexArgs a) {
  __shared__ unsigned char off[TOME_MAX_N / 4];
  __shared__ short top[TOME_MAX_N / 4 + 1];
  const int cy = blockIdx.x, Wc = a.Wg >> 1, Ns = 3 * (a.Hg >> 1) * Wc, N = a.Hg * a.Wg;
  const uint32_t step = a.mode ? (uint32_t)a.ctr[0] : 0u;
  for (int cx = threadIdx.x; cx < Wc; cx += 256) {
    uint32_t o = 0;
    if (a.mode) {
      uint32_t w[4];
      philox4x32_10((uint32_t)(cy * Wc + cx), step, (uint32_t)a.layer, TOME_TAG, a.k0, a.k1, w);
      o = w[0] & 3u;
    }
    off[cx] = (unsigned char)o;
    a.dst_tok[cy * Wc + cx] = (2 * cy + (int)(o >> 1)) * a.Wg + 2 * cx + (int)(o & 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int cx = 0; cx < Wc; ++cx) { top[cx] = (short)c; c += off[cx] < 2; }
    top[Wc] = (short)c;
  }
  __syncthreads();
  const int ntop = top[Wc];
  for (int e = threadIdx.x; e < 2 * a.Wg; e += 256) {
    const int row = e >= a.Wg, x = e - row * a.Wg, cx = x >> 1, o = off[cx];
    if ((o >> 1) == row && (o & 1) == (x & 1)) continue;      // the cell's destination
    // destinations of the row pair in front of this token: those of its own row in cells < cx, the cell's own if it sits left of x, the whole top row for row 1
    const int mine = row ? cx - top[cx] : top[cx], own = (o >> 1) == row && (int)(o & 1) < (x & 1);
    const int i = 3 * cy * Wc + e - (row ? ntop : 0) - mine - own, t = (2 * cy + row) * a.Wg + x;
    if (i < Ns && t < N)
      for (int b = 0; b < a.B; ++b) a.node_idx[(int64_t)b * Ns + i] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------- match launch
struct MatchArgs {
  const bf16_t* y; int64_t ld;
  const int32_t* dst_tok; float* node_max; int32_t* node_idx;
  int N, Ns, Nd, C;
};

__device__ __forceinline__ float frag_ssq(const bf16x8 x, float s) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bf16x2_hw v = {x[2 * k], x[2 * k + 1]};
    s = __builtin_amdgcn_fdot2_f32_bf16(v, v, s, false);
  }
  return s;
}
__device__ __forceinline__ float inv_norm(float ssq) { return ssq > 0.f ? 1.0f / sqrtf(ssq) : 0.f; }
// (score, index) pairs: the better one is the larger score, then the lower index
__device__ __forceinline__ void take_better(float& s, int& j, float so, int jo) {
  if (so > s || (so == s && jo < j)) { s = so; j = jo; }
}

__global__ __launch_bounds__(256) void tome_match_kernel(MatchArgs a) {
  __shared__ __attribute__((aligned(16))) char src_lds[SB * 128];
  __shared__ __attribute__((aligned(16))) char dst_lds[DB * 128];
  __shared__ float red_s[4][SB];
  __shared__ int red_j[4][SB];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, i = lane & 15;
  const int b = blockIdx.y, s0 = blockIdx.x * SB;
  const bf16_t* const yb = a.y + (int64_t)b * a.N * a.ld;
  int32_t* const idx_b = a.node_idx + (int64_t)b * a.Ns;

  // staging roles: the lane fills 16-byte slot (row, tid & 7) of the source tile and of eight destination rows; the slot holds source chunk slot ^ (row & 7)
  const int srow = tid >> 3, schunk = (tid & 7) ^ (srow & 7);      // (rows srow + 32 j of the destination tile: the same low three bits, the same chunk)
  const int64_t soff = (int64_t)min(max(idx_b[min(s0 + srow, a.Ns - 1)], 0), a.N - 1) * a.ld;      // this lane's source token row (the table the index launch left)
  int64_t doff[8];
  const int nkc = (a.C + KC - 1) / KC, nit = (a.Nd + DB - 1) / DB, nstep = nit * nkc;
  uint4 rs, rd[8];
  auto fetch = [&](int it, int kc) {      // global -> registers: step (it, kc); columns >= C read as zero, destinations >= Nd as the last one (never folded)
    if (kc == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        doff[j] = (int64_t)min(max(a.dst_tok[min(it * DB + srow + 32 * j, a.Nd - 1)], 0), a.N - 1) * a.ld;
    }
    const int col = kc * KC + schunk * 8;
    const bool in = col < a.C;
    rs = in ? *(const uint4*)(yb + soff + col) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) rd[j] = in ? *(const uint4*)(yb + doff[j] + col) : make_uint4(0, 0, 0, 0);
  };

  float best[2] = {-INFINITY, -INFINITY}, ssq_s[2] = {0.f, 0.f};
  int bidx[2] = {0, 0};
  f32x4 acc[2][4];
  float ssq_d[4];
  fetch(0, 0);
  for (int step = 0, it = 0, kc = 0; step < nstep; ++step) {
    if (kc == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ssq_d[t] = 0.f;
        acc[0][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[1][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();      // every wave is done with the previous step's tiles
    *(uint4*)(src_lds + srow * 128 + (tid & 7) * 16) = rs;
#pragma unroll
    for (int j = 0; j < 8; ++j) *(uint4*)(dst_lds + (srow + 32 * j) * 128 + (tid & 7) * 16) = rd[j];
    __syncthreads();
    const int kcn = kc + 1 == nkc ? 0 : kc + 1, itn = kcn ? it : it + 1;
    if (step + 1 < nstep) fetch(itn, kcn);      // in flight during this step's MFMAs

    const char* const dw = dst_lds + w * DBW * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ch = ks * 4 + g;
      bf16x8 sf[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int row = f * 16 + i;
        sf[f] = *(const bf16x8*)(src_lds + row * 128 + ((ch ^ (row & 7)) << 4));
        if (it == 0) ssq_s[f] = frag_ssq(sf[f], ssq_s[f]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = t * 16 + i;
        const bf16x8 df = *(const bf16x8*)(dw + row * 128 + ((ch ^ (row & 7)) << 4));
        ssq_d[t] = frag_ssq(df, ssq_d[t]);
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, sf[0], acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, sf[1], acc[1][t], 0, 0, 0);
      }
    }

    if (kcn == 0) {      // the block's K walk is complete: column scale and fold, ascending j
      const int j0 = it * DB + w * DBW;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float q = ssq_d[t];
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        const float inv = inv_norm(q);      // of destination j0 + 16 t + i, in every lane (g, i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float invj = __shfl(inv, 4 * g + e, 64);
          const int j = j0 + 16 * t + 4 * g + e;
          if (j < a.Nd) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              const float s = acc[f][t][e] * invj;
              if (s > best[f]) { best[f] = s; bidx[f] = j; }
            }
          }
        }
      }
    }
    kc = kcn; it = itn;
  }

  // the four g of a source, then the four waves
#pragma unroll
  for (int f = 0; f < 2; ++f) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float so = __shfl_xor(best[f], o, 64);
      const int jo = __shfl_xor(bidx[f], o, 64);
      take_better(best[f], bidx[f], so, jo);
    }
    ssq_s[f] += __shfl_xor(ssq_s[f], 16, 64);
    ssq_s[f] += __shfl_xor(ssq_s[f], 32, 64);
    if (g == 0) { red_s[w][f * 16 + i] = best[f]; red_j[w][f * 16 + i] = bidx[f]; }
  }
  __syncthreads();
  if (tid < SB && s0 + tid < a.Ns) {      // thread r = lane (g = r >> 4, i = r & 15) of wave 0 holds sum y^2 of source 16 g + i in ssq_s[g]
    float s = red_s[0][tid];
    int j = red_j[0][tid];
#pragma unroll
    for (int k = 1; k < 4; ++k) take_better(s, j, red_s[k][tid], red_j[k][tid]);
    a.node_max[(int64_t)b * a.Ns + s0 + tid] = s * inv_norm(g ? ssq_s[1] : ssq_s[0]);
    idx_b[s0 + tid] = j;
  }
}

// ---------------------------------------------------------------------------------------------------------------- plan launch
// One workgroup of 1024 threads per image.  The r-th largest node_max is found by a four-pass radix select over order-preserving keys (integer histograms
// in LDS: counts do not depend on arrival order); a source is merged when its key is above that value, or equal and among the first `need` equal keys
// in ascending index - the stable descending order.  Thread k owns the contiguous tokens [k per, (k + 1) per), per <= 16, so prefix sums over thread totals
// give source indices, ranks among ties and kept rows in ascending token order.
struct PlanArgs {
  const float* node_max; const int32_t* node_idx; const int32_t* dst_tok;
  int32_t* map; int32_t* kept_tok; int32_t* offsets; int32_t* list;
  int N, Ns, Nd, Np, r;
};

__device__ __forceinline__ uint32_t order_key(float v) {      // larger float <-> larger key; -0 counts as +0
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int block_scan(int v, int* sh, int& total) {      // exclusive prefix sum over the 1024 threads of a workgroup
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) sh[w] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { const int c = sh[k]; base += k < w ? c : 0; tot += c; }
  total = tot;
  return base + x - v;
}

__global__ __launch_bounds__(1024) void tome_plan_kernel(PlanArgs a) {
  constexpr int CH = TOME_MAX_N / 1024;
  __shared__ int sh[16], hist[256], cur[TOME_MAX_N / 4], drow[TOME_MAX_N / 4];
  __shared__ uint32_t sel_prefix;
  __shared__ int sel_need;
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* const nmax = a.node_max + (int64_t)b * a.Ns;
  const int32_t* const nidx = a.node_idx + (int64_t)b * a.Ns;
  int32_t* const map = a.map + (int64_t)b * a.N;
  int32_t* const kept = a.kept_tok + (int64_t)b * a.Np;
  int32_t* const offs = a.offsets + (int64_t)b * (a.Nd + 1);
  int32_t* const list = a.list + (int64_t)b * a.r;

  // destinations marked in map: -1 a source, -(j + 2) destination j
  for (int t = tid; t < a.N; t += 1024) map[t] = -1;
  for (int j = tid; j < a.Nd; j += 1024) cur[j] = 0;
  if (tid == 0) { sel_prefix = 0u; sel_need = a.r; }
  __syncthreads();
  for (int j = tid; j < a.Nd; j += 1024) {
    const uint32_t t = (uint32_t)a.dst_tok[j];
    if (t < (uint32_t)a.N) map[t] = -(j + 2);
  }

  // the r-th largest key and how many of its equals are taken
  uint32_t mask = 0u;
  for (int shift = 24; shift >= 0 && a.r > 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = sel_prefix;
    for (int i = tid; i < a.Ns; i += 1024) {
      const uint32_t k = order_key(nmax[i]);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int c = 0, need = sel_need, bkt = 255;
      for (; bkt > 0; --bkt) {
        if (c + hist[bkt] >= need) break;
        c += hist[bkt];
      }
      sel_prefix = prefix | ((uint32_t)bkt << shift);
      sel_need = need - c;
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  __syncthreads();
  const uint32_t T = sel_prefix;
  const int need = sel_need;

  const int per = (a.N + 1023) / 1024, t0 = min(tid * per, a.N), t1 = min(t0 + per, a.N);
  int nsrc = 0, neq = 0;
  for (int t = t0; t < t1; ++t) nsrc += map[t] == -1;
  int dummy;
  const int sbase = block_scan(nsrc, sh, dummy);
  for (int k = 0; k < nsrc; ++k) neq += sbase + k < a.Ns && order_key(nmax[sbase + k]) == T;
  const int ebase = block_scan(neq, sh, dummy);

  // token types of this thread's chunk, two bits each: 0 destination, 1 kept source, 2 merged source
  uint32_t types = 0u;
  int nkept = 0;
  {
    int i = sbase, e = ebase;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 + u;
      if (t < t1) {
        uint32_t ty = 0u;
        if (map[t] == -1) {
          const uint32_t k = i < a.Ns ? order_key(nmax[i]) : 0u;
          const bool merged = a.r > 0 && i < a.Ns && (k > T || (k == T && e < need));
          e += k == T;
          ++i;
          ty = merged ? 2u : 1u;
        }
        nkept += ty != 2u;
        types |= ty << (2 * u);
      }
    }
  }
  const int kbase = block_scan(nkept, sh, dummy);
  {
    int i = sbase, row = kbase;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 + u;
      if (t < t1) {
        const uint32_t ty = (types >> (2 * u)) & 3u;
        if (ty != 2u) {
          if (row < a.Np) kept[row] = t;
          if (ty == 0u) drow[-map[t] - 2] = row;
          map[t] = row;
          ++row;
        } else {
          atomicAdd(&cur[min(max(nidx[i], 0), a.Nd - 1)], 1);
        }
        i += ty != 0u;
      }
    }
  }
  __syncthreads();

  // CSR offsets; cur[] becomes each destination's fill cursor
  {
    const int perd = (a.Nd + 1023) / 1024, j0 = min(tid * perd, a.Nd), j1 = min(j0 + perd, a.Nd);
    int c = 0, total;
    for (int j = j0; j < j1; ++j) c += cur[j];
    int o = block_scan(c, sh, total);
    for (int j = j0; j < j1; ++j) { const int n = cur[j]; offs[j] = o; cur[j] = o; o += n; }
    if (tid == 0) offs[a.Nd] = total;
  }
  __syncthreads();
  // fill in arrival order, then put every list in ascending order: an entry's place is the number of smaller entries of its list
  {
    int i = sbase;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 + u;
      if (t < t1) {
        const uint32_t ty = (types >> (2 * u)) & 3u;
        if (ty == 2u) {
          const int d = min(max(nidx[i], 0), a.Nd - 1), p = atomicAdd(&cur[d], 1);
          if (p < a.r) list[p] = t;
          map[t] = drow[d];
        }
        i += ty != 0u;
      }
    }
  }
  __syncthreads();
  int pos[CH];
  {
    int i = sbase;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 + u;
      pos[u] = -1;
      if (t < t1) {
        const uint32_t ty = (types >> (2 * u)) & 3u;
        if (ty == 2u) {
          const int d = min(max(nidx[i], 0), a.Nd - 1), lo = offs[d], hi = min(offs[d + 1], a.r);
          int c = lo;
          for (int q = lo; q < hi; ++q) c += list[q] < t;
          pos[u] = c;
        }
        i += ty != 0u;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < CH; ++u)
    if (pos[u] >= 0 && pos[u] < a.r) list[pos[u]] = t0 + u;
}

// ---------------------------------------------------------------------------------------------------------------- merge and unmerge launches
// One wave per output row, four per workgroup; lane l owns the 8-channel chunks l, l + 64, ...
struct MergeArgs {
  const bf16_t* y; int64_t ld;
  const int32_t* dst_tok; const int32_t* kept_tok; const int32_t* offsets; const int32_t* list;
  bf16_t* ym; int64_t ldm;
  int B, N, Nd, Np, Wg, C, r;
};

__global__ __launch_bounds__(256) void tome_merge_kernel(MergeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t orow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (orow >= (int64_t)a.B * a.Np) return;
  const int b = (int)(orow / a.Np), k = (int)(orow - (int64_t)b * a.Np);
  const int t = min(max(a.kept_tok[(int64_t)b * a.Np + k], 0), a.N - 1);
  const int ty = t / a.Wg, tx = t - ty * a.Wg, j = (ty >> 1) * (a.Wg >> 1) + (tx >> 1);
  int lo = 0, hi = 0;
  if (a.dst_tok[j] == t) {
    const int32_t* o = a.offsets + (int64_t)b * (a.Nd + 1) + j;
    lo = min(max(o[0], 0), a.r);
    hi = min(max(o[1], lo), a.r);
  }
  const bf16_t* const yb = a.y + (int64_t)b * a.N * a.ld;
  const int32_t* const list = a.list + (int64_t)b * a.r;
  bf16_t* const dst = a.ym + orow * a.ldm;
  for (int ch = lane; ch < (a.C >> 3); ch += 64) {
    const uint4 own = *(const uint4*)(yb + (int64_t)t * a.ld + ch * 8);
    if (lo == hi) {      // a copy, bit for bit
      *(uint4*)(dst + ch * 8) = own;
      continue;
    }
    float acc[8], v[8];
    load8((const bf16_t*)&own, acc);
    for (int q = lo; q < hi; ++q) {      // ascending source index
      const int s = min(max(list[q], 0), a.N - 1);
      load8(yb + (int64_t)s * a.ld + ch * 8, v);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += v[c];
    }
    const float cnt = (float)(hi - lo + 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] /= cnt;
    store8(dst + ch * 8, acc);
  }
}

struct UnmergeArgs {
  const bf16_t* res; int64_t ldr;
  const bf16_t* a; int64_t lda;
  const int32_t* map;
  bf16_t* out; int64_t ldo;
  int B, N, Np, C;
};

__global__ __launch_bounds__(256) void tome_unmerge_kernel(UnmergeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)a.B * a.N) return;
  const int b = (int)(row / a.N);
  const int64_t arow = (int64_t)b * a.Np + min(max(a.map[row], 0), a.Np - 1);
  for (int ch = lane; ch < (a.C >> 3); ch += 64) {
    float r[8], v[8];
    load8(a.res + row * a.ldr + ch * 8, r);
    load8(a.a + arow * a.lda + ch * 8, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] += v[c];
    store8(a.out + row * a.ldo + ch * 8, r);
  }
}

// [lo, hi) byte ranges of the operands
struct Span { uintptr_t lo, hi; };
Span span2d(const void* ptr, int64_t rows, int64_t ld, int64_t cols, int esize) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)((rows - 1) * ld + cols) * esize}; }
Span span1d(const void* ptr, int64_t n) { return {(uintptr_t)ptr, (uintptr_t)ptr + (size_t)n * 4}; }
bool overlaps(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }
bool any_overlap(const Span* outs, int no, const Span* ins, int ni) {
  for (int o = 0; o < no; ++o) {
    for (int i = 0; i < ni; ++i)
      if (overlaps(outs[o], ins[i])) return true;
    for (int q = o + 1; q < no; ++q)
      if (overlaps(outs[o], outs[q])) return true;
  }
  return false;
}

// the grid checks every entry shares: -> N, or 0 with the error set
int64_t tome_grid(const char* fn, int B, int Hg, int Wg) {
  if (B < 1 || Hg < 1 || Wg < 1) { sdlt_set_error("%s: B=%d Hg=%d Wg=%d (all >= 1)", fn, B, Hg, Wg); return 0; }
  if ((Hg | Wg) & 1) { sdlt_set_error("%s: the %d x %d token grid must be even in both directions (2 x 2 cells)", fn, Hg, Wg); return 0; }
  const int64_t N = (int64_t)Hg * Wg;
  if (N > TOME_MAX_N) { sdlt_set_error("%s: %lld tokens per image (at most %d)", fn, (long long)N, TOME_MAX_N); return 0; }
  if ((int64_t)B * N > INT_MAX) { sdlt_set_error("%s: B=%d images of %lld tokens: a row index exceeds 32 bits", fn, B, (long long)N); return 0; }
  return N;
}

}  // namespace

extern "C" int sdlt_tome_match(const sdlt_tome_match_params* pp, void* stream) {
  const char* fn = "sdlt_tome_match";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_tome_match_params& p = *pp;
  if (!p.y || !p.dst_tok || !p.node_max || !p.node_idx) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (y, dst_tok, node_max, node_idx are required)", fn);
  if (p.mode != 0 && p.mode != 1) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "%s: mode=%d (0 fixed, 1 random)", fn, p.mode);
  if (p.mode == 1 && !p.ctr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (mode random reads ctr)", fn);
  const int64_t N = tome_grid(fn, p.B, p.Hg, p.Wg);
  if (!N) return SDLT_ERR_SHAPE;
  if (p.C < 8) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: C=%d (>= 8)", fn, p.C);
  if (p.ld < p.C || p.ld > INT_MAX) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld=%lld (C=%d <= ld < 2^31)", fn, (long long)p.ld, p.C);
  if ((p.C % 8) || (p.ld % 8) || ((uintptr_t)p.y & 15) || (((uintptr_t)p.ctr | (uintptr_t)p.dst_tok | (uintptr_t)p.node_max | (uintptr_t)p.node_idx) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: C %% 8, ld %% 8, y 16-byte aligned, the tables 4-byte aligned", fn);
  const int64_t Nd = N / 4, Ns = N - Nd;
  const Span outs[3] = {span1d(p.dst_tok, Nd), span1d(p.node_max, p.B * Ns), span1d(p.node_idx, p.B * Ns)};
  const Span ins[2] = {span2d(p.y, p.B * N, p.ld, p.C, 2), p.ctr ? span1d(p.ctr, 1) : Span{0, 0}};
  if (any_overlap(outs, 3, ins, 2)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: an output overlaps an input or another output", fn);
  hipStream_t s = (hipStream_t)stream;
  IndexArgs ia;
  ia.ctr = p.ctr; ia.dst_tok = p.dst_tok; ia.node_idx = p.node_idx; ia.k0 = (uint32_t)p.seed; ia.k1 = (uint32_t)(p.seed >> 32);
  ia.B = p.B; ia.Hg = p.Hg; ia.Wg = p.Wg; ia.mode = p.mode; ia.layer = p.layer;
  hipLaunchKernelGGL(tome_index_kernel, dim3((unsigned)(p.Hg / 2)), dim3(256), 0, s, ia);
  SDLT_CHECK_LAUNCH();
  MatchArgs ma;
  ma.y = (const bf16_t*)p.y; ma.ld = p.ld; ma.dst_tok = p.dst_tok; ma.node_max = p.node_max; ma.node_idx = p.node_idx;
  ma.N = (int)N; ma.Ns = (int)Ns; ma.Nd = (int)Nd; ma.C = p.C;
  hipLaunchKernelGGL(tome_match_kernel, dim3((unsigned)((Ns + SB - 1) / SB), (unsigned)p.B), dim3(256), 0, s, ma);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_tome_plan(const sdlt_tome_plan_params* pp, void* stream) {
  const char* fn = "sdlt_tome_plan";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_tome_plan_params& p = *pp;
  if (!p.node_max || !p.node_idx || !p.dst_tok || !p.map || !p.kept_tok || !p.offsets || !p.list)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (node_max, node_idx, dst_tok, map, kept_tok, offsets, list are required)", fn);
  const int64_t N = tome_grid(fn, p.B, p.Hg, p.Wg);
  if (!N) return SDLT_ERR_SHAPE;
  const int64_t Nd = N / 4, Ns = N - Nd, Np = N - p.r;
  if (p.r < 0 || p.r > Ns) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: r=%d (0 <= r <= N_src = %lld)", fn, p.r, (long long)Ns);
  if (Np % 8) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: N - r = %lld must be a multiple of 8 (the rows attention wants every image to start on)", fn, (long long)Np);
  if (((uintptr_t)p.node_max | (uintptr_t)p.node_idx | (uintptr_t)p.dst_tok | (uintptr_t)p.map | (uintptr_t)p.kept_tok | (uintptr_t)p.offsets | (uintptr_t)p.list) & 3)
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: the tables must be 4-byte aligned", fn);
  const Span outs[4] = {span1d(p.map, p.B * N), span1d(p.kept_tok, p.B * Np), span1d(p.offsets, p.B * (Nd + 1)), span1d(p.list, (int64_t)p.B * (p.r > 0 ? p.r : 1))};
  const Span ins[3] = {span1d(p.node_max, p.B * Ns), span1d(p.node_idx, p.B * Ns), span1d(p.dst_tok, Nd)};
  if (any_overlap(outs, 4, ins, 3)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: an output overlaps an input or another output", fn);
  PlanArgs a;
  a.node_max = p.node_max; a.node_idx = p.node_idx; a.dst_tok = p.dst_tok; a.map = p.map; a.kept_tok = p.kept_tok; a.offsets = p.offsets; a.list = p.list;
  a.N = (int)N; a.Ns = (int)Ns; a.Nd = (int)Nd; a.Np = (int)Np; a.r = p.r;
  hipLaunchKernelGGL(tome_plan_kernel, dim3((unsigned)p.B), dim3(1024), 0, (hipStream_t)stream, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_tome_merge(const sdlt_tome_merge_params* pp, void* stream) {
  const char* fn = "sdlt_tome_merge";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_tome_merge_params& p = *pp;
  if (!p.y || !p.dst_tok || !p.kept_tok || !p.offsets || !p.list || !p.ym)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (y, dst_tok, kept_tok, offsets, list, ym are required)", fn);
  const int64_t N = tome_grid(fn, p.B, p.Hg, p.Wg);
  if (!N) return SDLT_ERR_SHAPE;
  const int64_t Nd = N / 4, Ns = N - Nd, Np = N - p.r;
  if (p.r < 0 || p.r > Ns) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: r=%d (0 <= r <= N_src = %lld)", fn, p.r, (long long)Ns);
  if (Np % 8) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: N - r = %lld must be a multiple of 8", fn, (long long)Np);
  if (p.C < 8) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: C=%d (>= 8)", fn, p.C);
  if (p.ld < p.C || p.ldm < p.C || p.ld > INT_MAX || p.ldm > INT_MAX) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ld=%lld ldm=%lld (C=%d <= ld < 2^31)", fn, (long long)p.ld, (long long)p.ldm, p.C);
  if ((p.C % 8) || (p.ld % 8) || (p.ldm % 8) || (((uintptr_t)p.y | (uintptr_t)p.ym) & 15) ||
      (((uintptr_t)p.dst_tok | (uintptr_t)p.kept_tok | (uintptr_t)p.offsets | (uintptr_t)p.list) & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: C %% 8, ld %% 8, y and ym 16-byte aligned, the tables 4-byte aligned", fn);
  const Span outs[1] = {span2d(p.ym, p.B * Np, p.ldm, p.C, 2)};
  const Span ins[5] = {span2d(p.y, p.B * N, p.ld, p.C, 2), span1d(p.dst_tok, Nd), span1d(p.kept_tok, p.B * Np), span1d(p.offsets, p.B * (Nd + 1)),
                       span1d(p.list, (int64_t)p.B * (p.r > 0 ? p.r : 1))};
  if (any_overlap(outs, 1, ins, 5)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ym overlaps an input", fn);
  MergeArgs a;
  a.y = (const bf16_t*)p.y; a.ld = p.ld; a.dst_tok = p.dst_tok; a.kept_tok = p.kept_tok; a.offsets = p.offsets; a.list = p.list; a.ym = (bf16_t*)p.ym; a.ldm = p.ldm;
  a.B = p.B; a.N = (int)N; a.Nd = (int)Nd; a.Np = (int)Np; a.Wg = p.Wg; a.C = p.C; a.r = p.r;
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)((p.B * Np + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_tome_unmerge(const sdlt_tome_unmerge_params* pp, void* stream) {
  const char* fn = "sdlt_tome_unmerge";
  if (!pp) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", fn);
  const sdlt_tome_unmerge_params& p = *pp;
  if (!p.residual || !p.a || !p.map || !p.out) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null operand (residual, a, map, out are required)", fn);
  if (p.B < 1 || p.N < 1 || p.Np < 1 || p.Np > p.N || p.C < 8) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d N=%d Np=%d C=%d (B >= 1, 1 <= Np <= N, C >= 8)", fn, p.B, p.N, p.Np, p.C);
  if ((int64_t)p.B * p.N > INT_MAX) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d images of %d tokens: a row index exceeds 32 bits", fn, p.B, p.N);
  if (p.ldr < p.C || p.lda < p.C || p.ldo < p.C || p.ldr > INT_MAX || p.lda > INT_MAX || p.ldo > INT_MAX)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ldr=%lld lda=%lld ldo=%lld (C=%d <= ld < 2^31)", fn, (long long)p.ldr, (long long)p.lda, (long long)p.ldo, p.C);
  if ((p.C % 8) || (p.ldr % 8) || (p.lda % 8) || (p.ldo % 8) || (((uintptr_t)p.residual | (uintptr_t)p.a | (uintptr_t)p.out) & 15) || ((uintptr_t)p.map & 3))
    SDLT_FAIL(SDLT_ERR_ALIGN, "%s: C %% 8, ld %% 8, residual, a and out 16-byte aligned, map 4-byte aligned", fn);
  const int64_t M = (int64_t)p.B * p.N;
  const Span outs[1] = {span2d(p.out, M, p.ldo, p.C, 2)};
  const Span ins[3] = {span2d(p.residual, M, p.ldr, p.C, 2), span2d(p.a, (int64_t)p.B * p.Np, p.lda, p.C, 2), span1d(p.map, M)};
  if (any_overlap(outs, 1, ins, 3)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: out overlaps an input", fn);
  UnmergeArgs a;
  a.res = (const bf16_t*)p.residual; a.ldr = p.ldr; a.a = (const bf16_t*)p.a; a.lda = p.lda; a.map = p.map; a.out = (bf16_t*)p.out; a.ldo = p.ldo;
  a.B = p.B; a.N = p.N; a.Np = p.Np; a.C = p.C;
  hipLaunchKernelGGL(tome_unmerge_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
