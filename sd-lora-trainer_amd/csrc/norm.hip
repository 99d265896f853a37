// GroupNorm(32)+SiLU and LayerNorm, forward and dX backward, for NHWC / token-major bf16
// activations (gfx950).  HBM-bound: every kernel moves 16 B per lane, a wave covers 8 rows x 64
// channels (128-B lines), and each thread keeps a FIXED 8-channel column so gamma/beta/mean/rstd
// live in registers for the whole row loop.
//
// Replaces (reference call sites, all reached from main.py:329-336 through diffusers):
//   ResnetBlock2D.norm1/norm2 + SiLU, Transformer2DModel.norm, conv_norm_out  -> groupnorm
//   BasicTransformerBlock.norm1/2/3 (and CLIP LayerNorms)                     -> layernorm
// gamma/beta are frozen in the reference (main.py:109-114), so only dX is produced.
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr int G = 32;

// row pointer for channel c of row r of the (possibly two-tensor, channel-concatenated) input
struct CatIn {
  const bf16_t* x1; int64_t ld1; int C1;
  const bf16_t* x2; int64_t ld2;
  __device__ __forceinline__ const bf16_t* at(int64_t row, int c) const {
    return c < C1 ? x1 + row * ld1 + c : x2 + row * ld2 + (c - C1);
  }
};


// Deterministic two-stage reduction of the per-(batch, group) statistics (no float atomics, no zero fills, no fences: a fixed
// summation order makes two runs - and a hipGraph replay vs the eager pass - bitwise identical).
//   stage 1 (the statistics kernel): the block's 4 waves leave their per-channel sums in LDS; thread t < 64 (statistic slot
//            t = group * 2 + kind) adds the channels of its group that fall into this block, waves 0..3, in a fixed order, and the
//            64 slots (zeros for groups the block does not touch) go to the block's row of the workspace
//            ws[((b * rs + by) * cb + bx) * 64 + t];
//   stage 2 (the PROLOGUE of the kernel that consumes the statistics - it exists anyway, and the launch boundary publishes the rows):
//            every block sums, for the slots of the groups its 64 channels belong to, the rows of all row splits of the blocks
//            covering the group - the 256 threads split (slot, part-of-the-rows), all of a thread's loads in flight at once, the
//            parts combined in order - into LDS.  Every block computes the same bits; the blocks of row split 0 also store them
//            to `out` for later kernels (backward, affine gradients).
__device__ __forceinline__ void gn_block_partials(float (&s)[8], float (&q)[8], int C, float* __restrict__ ws) {
  __shared__ float sch[4][64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, cb = gridDim.x, rs = gridDim.y;
  const int cpg = C / G;
  // lanes with the same (lane&7) hold the same channels: reduce over lane>>3 (xor 8,16,32)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { s[j] += __shfl_xor(s[j], o, 64); q[j] += __shfl_xor(q[j], o, 64); }
  }
  if ((lane >> 3) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { sch[wave][(lane & 7) * 8 + j][0] = s[j]; sch[wave][(lane & 7) * 8 + j][1] = q[j]; }
  }
  __syncthreads();
  if (tid < 64) {
    const int g = tid >> 1, kind = tid & 1;
    const int blo = (int)blockIdx.x * 64;
    const int clo = g * cpg > blo ? g * cpg : blo, chi = (g + 1) * cpg < blo + 64 ? (g + 1) * cpg : blo + 64;
    float a = 0.f;
    for (int c = clo; c < chi; ++c) {
      const int cl = c - blo;
      a += ((sch[0][cl][kind] + sch[1][cl][kind]) + (sch[2][cl][kind] + sch[3][cl][kind]));
    }
    ws[(((size_t)b * rs + blockIdx.y) * cb + blockIdx.x) * 64 + tid] = a;
  }
}

// stage 2: -> fin[64] (LDS; valid for the slots of the groups this block's 64 channels belong to) [+ out, row split 0]
__device__ __forceinline__ void gn_combine_partials(int C, const float* __restrict__ ws, float* __restrict__ fin, float* __restrict__ out) {
  __shared__ float parts[256];
  const int tid = threadIdx.x;
  const int b = blockIdx.z, cb = gridDim.x, rs = gridDim.y;
  const int cpg = C / G;
  const int glo = ((int)blockIdx.x * 64) / cpg, ghi = ((int)blockIdx.x * 64 + 63) / cpg;
  const int ns = (ghi - glo + 1) * 2;                       // slots this block needs
  int p2 = 2;
  while (p2 < ns) p2 <<= 1;                                  // <= 64
  const int sl = tid & (p2 - 1), part = tid / p2, nparts = 256 / p2;
  const int slot = glo * 2 + sl, g = slot >> 1;
  float acc = 0.f;
  if (sl < ns) {
    const int bxlo = (g * cpg) / 64, bxhi = ((g + 1) * cpg - 1) / 64;
    const int nbx = bxhi - bxlo + 1, rows = rs * nbx;
    const float* base = ws + (size_t)b * rs * cb * 64 + slot;
    float a8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a8[u] = 0.f;
    for (int r = part; r < rows; r += nparts * 8) {
      // (eight loads in flight: unconditional, from a clamped row, masked where they are added - under `if (rr < rows)` hipcc issued and awaited them one at a
      // time: eight serial round trips in the prologue of every apply kernel, found in the ISA in round 5)
      float t8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int rr = r + nparts * u, rc = rr < rows ? rr : rows - 1;
        const int by = rc / nbx, bx = bxlo + (rc - by * nbx);
        t8[u] = base[((size_t)by * cb + bx) * 64];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) a8[u] += (r + nparts * u < rows) ? t8[u] : 0.f;
    }
    acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
  }
  parts[tid] = acc;
  __syncthreads();
  if (tid < p2 && tid < ns) {
    float t = parts[tid];
    for (int k = 1; k < nparts; ++k) t += parts[k * p2 + tid];
    fin[slot] = t;
    // ONE writer per slot: a group that straddles two 64-channel blocks is summed by both, but with different (slot, part) splits of the 256 threads when the
    // blocks touch different numbers of groups (C = 1280: 40 channels per group, 2 or 3 groups per block) - the two sums can differ in the last bit, and which one
    // landed in `out` was a race (found in round 5: the forward statistics the backward pass reads differed by an ulp between two passes from the same state,
    // tools/determinism_probe.py - the only nondeterminism of the LoRA / TI step).  The first block of the group stores.
    if (out && blockIdx.y == 0 && (int)blockIdx.x == ((slot >> 1) * cpg) / 64) out[b * 64 + slot] = t;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------- GroupNorm
// grid (C/64, rowsplit, B), block 256 = 4 waves; thread: fixed chunk c0 = bx*64 + (lane&7)*8,
// rows r = ry*32.. step gridDim.y*32, sub-row = wave*8 + lane/8.
// stats[b][g] = {sum, sumsq} accumulated with atomics (zeroed by the entry point).
__global__ __launch_bounds__(256) void gn_stats_kernel(CatIn in, int HW, int C, float* ws) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int c0 = blockIdx.x * 64 + (lane & 7) * 8;
  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
  // (the next row is requested - unconditionally, from a clamped row - before the current one is consumed: a load under `if (r < HW)` with a default made hipcc wait for every
  // load where it was issued, i.e. one exposed round trip per row of the loop; round 5, tools/scan_exposed_waits.py)
  const int rstep = gridDim.y * 32;
  int r = blockIdx.y * 32 + wave * 8 + (lane >> 3);
  uint4 xn = *(const uint4*)in.at((int64_t)b * HW + (r < HW ? r : HW - 1), c0);
  while (r < HW) {
    const uint4 xc = xn;
    r += rstep;
    xn = *(const uint4*)in.at((int64_t)b * HW + (r < HW ? r : HW - 1), c0);
    const uint32_t w[4] = {xc.x, xc.y, xc.z, xc.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = bf2f((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffff));
      s[j] += v; q[j] += v * v;
    }
  }
  gn_block_partials(s, q, C, ws);
}

template <bool SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(CatIn in, int HW, int C, float* stats_out, const float* ws,
                                                        const float* gamma, const float* beta, float eps,
                                                        bf16_t* y, int64_t ldy) {
  __shared__ float stats[G * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int c0 = blockIdx.x * 64 + (lane & 7) * 8;
  // per-channel parameters and the first row are requested BEFORE the statistics are combined (one memory latency instead of three
  // in a row: partial rows -> gamma / beta -> x); the row loop keeps the next row's load in flight
  const f32x4 gv0 = *(const f32x4*)(gamma + c0), gv1 = *(const f32x4*)(gamma + c0 + 4), bv0 = *(const f32x4*)(beta + c0), bv1 = *(const f32x4*)(beta + c0 + 4);
  const int rstep = gridDim.y * 32;
  int r = blockIdx.y * 32 + wave * 8 + (lane >> 3);
  uint4 xn = *(const uint4*)in.at((int64_t)b * HW + (r < HW ? r : HW - 1), c0);      // (unconditional, clamped: see gn_stats_kernel)
  gn_combine_partials(C, ws, stats, stats_out);
  float gm[8], bt[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { gm[j] = j < 4 ? gv0[j & 3] : gv1[j & 3]; bt[j] = j < 4 ? bv0[j & 3] : bv1[j & 3]; }
  const int cpg = C / G;
  const float inv_n = 1.0f / ((float)HW * (float)cpg);
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int g = (c0 + j) / cpg;
    float mean = stats[g * 2] * inv_n;
    float var = fmaxf(stats[g * 2 + 1] * inv_n - mean * mean, 0.f);
    float rstd = rsqrtf(var + eps);
    sc[j] = rstd * gm[j];
    sh[j] = bt[j] - mean * sc[j];
  }
  while (r < HW) {
    const uint4 xc = xn;
    const int64_t row = (int64_t)b * HW + r;
    r += rstep;
    xn = *(const uint4*)in.at((int64_t)b * HW + (r < HW ? r : HW - 1), c0);
    const uint32_t w[4] = {xc.x, xc.y, xc.z, xc.w};
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float z = bf2f((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffff)) * sc[j] + sh[j];
      v[j] = SILU ? silu_f(z) : z;
    }
    store8(y + row * ldy + c0, v);
  }
}

// Backward kernels: gamma / beta of a lane's 8 consecutive channels (two 16-byte loads each) and the forward statistics (sum, sum of squares) of their groups (one 8-byte load per
// channel, mostly the same address), ALL REQUESTED TOGETHER and consumed later by gn_lane_finish - the per-channel form `mean[j] = stats[...] * inv_n` right behind each load made
// eight serial round trips out of the prologue of every GroupNorm backward launch (round 5, tools/scan_exposed_waits.py)
struct GnLaneRaw { f32x4 g0, g1, b0, b1; float2 st[8]; };
__device__ __forceinline__ GnLaneRaw gn_lane_loads(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ stats, int b, int c0, int cpg) {
  GnLaneRaw w;
  w.g0 = *(const f32x4*)(gamma + c0); w.g1 = *(const f32x4*)(gamma + c0 + 4);
  w.b0 = *(const f32x4*)(beta + c0); w.b1 = *(const f32x4*)(beta + c0 + 4);
  int gj[8];
  const int ga = c0 / cpg;
  if (cpg >= 8) {            // 8 consecutive channels cross at most one group boundary
    const int jb = (ga + 1) * cpg - c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) gj[j] = ga + (j >= jb ? 1 : 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) gj[j] = (c0 + j) / cpg;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) w.st[j] = *(const float2*)(stats + (b * G + gj[j]) * 2);
  return w;
}
__device__ __forceinline__ void gn_lane_finish(const GnLaneRaw& w, float inv_n, float eps, float (&mean)[8], float (&rstd)[8], float (&gm)[8], float (&bt)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mean[j] = w.st[j].x * inv_n;
    const float var = fmaxf(w.st[j].y * inv_n - mean[j] * mean[j], 0.f);
    rstd[j] = rsqrtf(var + eps);
    gm[j] = j < 4 ? w.g0[j & 3] : w.g1[j & 3];
    bt[j] = j < 4 ? w.b0[j & 3] : w.b1[j & 3];
  }
}

// backward pass 1: per (b,g): s1 = sum(dz*gamma), s2 = sum(dz*gamma*xhat)
template <bool SILU>
__global__ __launch_bounds__(256) void gn_bwd_stats_kernel(CatIn in, const bf16_t* dy, int64_t lddy, int HW, int C,
                                                            const float* stats, const float* gamma, const float* beta,
                                                            float eps, float* ws) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int c0 = blockIdx.x * 64 + (lane & 7) * 8;
  const int cpg = C / G;
  const float inv_n = 1.0f / ((float)HW * (float)cpg);
  float mean[8], rstd[8], gm[8], bt[8], s1[8], s2[8];
  const GnLaneRaw raw = gn_lane_loads(gamma, beta, stats, b, c0, cpg);
  const int rstep = gridDim.y * 32;
  int r = blockIdx.y * 32 + wave * 8 + (lane >> 3);
  int64_t row = (int64_t)b * HW + (r < HW ? r : HW - 1);
  uint4 xn = *(const uint4*)in.at(row, c0), dn = *(const uint4*)(dy + row * lddy + c0);       // (unconditional, clamped rows; the next row is in flight while this one is consumed)
  gn_lane_finish(raw, inv_n, eps, mean, rstd, gm, bt);
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  while (r < HW) {
    const uint4 xc = xn, dc = dn;
    r += rstep;
    row = (int64_t)b * HW + (r < HW ? r : HW - 1);
    xn = *(const uint4*)in.at(row, c0);
    dn = *(const uint4*)(dy + row * lddy + c0);
    const uint32_t xw[4] = {xc.x, xc.y, xc.z, xc.w}, dw[4] = {dc.x, dc.y, dc.z, dc.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = bf2f((j & 1) ? (xw[j >> 1] >> 16) : (xw[j >> 1] & 0xffff));
      float dz = bf2f((j & 1) ? (dw[j >> 1] >> 16) : (dw[j >> 1] & 0xffff));
      const float xh = (v - mean[j]) * rstd[j];
      if (SILU) dz *= dsilu_f(xh * gm[j] + bt[j]);
      const float dxh = dz * gm[j];
      s1[j] += dxh; s2[j] += dxh * xh;
    }
  }
  gn_block_partials(s1, s2, C, ws);
}

template <bool SILU>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(CatIn in, const bf16_t* dy, int64_t lddy, int HW, int C,
                                                            const float* stats, float* bstats_out, const float* ws, const float* gamma,
                                                            const float* beta, float eps, const bf16_t* dres, int64_t lddres,
                                                            bf16_t* dx, int64_t lddx, float* csws) {
  __shared__ float bstats[G * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int c0 = blockIdx.x * 64 + (lane & 7) * 8;
  const int cpg = C / G;
  const float inv_n = 1.0f / ((float)HW * (float)cpg);
  // (as gn_apply_kernel: parameters, forward statistics and the first row's three tiles are in flight while the partial sums are combined)
  float mean[8], rstd[8], gm[8], bt[8], m1[8], m2[8];
  const GnLaneRaw raw = gn_lane_loads(gamma, beta, stats, b, c0, cpg);
  const int rstep = gridDim.y * 32;
  int r = blockIdx.y * 32 + wave * 8 + (lane >> 3);
  // (unconditional loads from clamped rows; a missing residual gradient reads dy again and is skipped where it would be added)
  const bf16_t* rsrc = dres ? dres : dy;
  const int64_t ldrs = dres ? lddres : lddy;
  uint4 xn, dn, on;
  {
    const int64_t row = (int64_t)b * HW + (r < HW ? r : HW - 1);
    xn = *(const uint4*)in.at(row, c0);
    dn = *(const uint4*)(dy + row * lddy + c0);
    on = *(const uint4*)(rsrc + row * ldrs + c0);
  }
  gn_combine_partials(C, ws, bstats, bstats_out);
  gn_lane_finish(raw, inv_n, eps, mean, rstd, gm, bt);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int g = (c0 + j) / cpg;
    m1[j] = bstats[g * 2] * inv_n;
    m2[j] = bstats[g * 2 + 1] * inv_n;
  }
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  while (r < HW) {
    const uint4 xc = xn, dc = dn, oc = on;
    const int64_t row = (int64_t)b * HW + r;
    r += rstep;
    {      // (dres may alias dx: a row is read before it is written, and rows are disjoint between iterations - the clamped re-read behind the last row is never used)
      const int64_t nrow = (int64_t)b * HW + (r < HW ? r : HW - 1);
      xn = *(const uint4*)in.at(nrow, c0);
      dn = *(const uint4*)(dy + nrow * lddy + c0);
      on = *(const uint4*)(rsrc + nrow * ldrs + c0);
    }
    const uint32_t xw[4] = {xc.x, xc.y, xc.z, xc.w}, dw[4] = {dc.x, dc.y, dc.z, dc.w}, ow[4] = {oc.x, oc.y, oc.z, oc.w};
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = bf2f((j & 1) ? (xw[j >> 1] >> 16) : (xw[j >> 1] & 0xffff));
      float dz = bf2f((j & 1) ? (dw[j >> 1] >> 16) : (dw[j >> 1] & 0xffff));
      const float xh = (v - mean[j]) * rstd[j];
      if (SILU) dz *= dsilu_f(xh * gm[j] + bt[j]);
      const float dxh = dz * gm[j];
      o[j] = (dres ? bf2f((j & 1) ? (ow[j >> 1] >> 16) : (ow[j >> 1] & 0xffff)) : 0.f) + rstd[j] * (dxh - m1[j] - xh * m2[j]);
    }
    store8(dx + row * lddx + c0, o);
    if (csws) {      // column sums of the rows as they were stored (bf16-rounded), see below
#pragma unroll
      for (int j = 0; j < 8; ++j) cs[j] += bf2f(f2bf(o[j]));
    }
  }
  // Side output (ResnetBlock2D: the time-embedding projection is added per image in front of norm2, so its gradient is the column sum over the pixels of this
  // kernel's output): every block leaves the column sums of its rows in csws[(split * B + b) * C + c] - plain stores, no atomics; sdlt_colsum_finish_batch adds
  // the splits in a fixed order for all resnets of the step in one launch (were two launches per resnet: sdlt_colsum over the stored gradient + its finish).
  if (csws) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) cs[j] += __shfl_xor(cs[j], o, 64);
    __shared__ float csh[4][64];
    if ((lane >> 3) == 0)
#pragma unroll
      for (int j = 0; j < 8; ++j) csh[wave][(lane & 7) * 8 + j] = cs[j];
    __syncthreads();
    if (tid < 64) csws[((int64_t)blockIdx.y * gridDim.z + b) * C + blockIdx.x * 64 + tid] = (csh[0][tid] + csh[1][tid]) + (csh[2][tid] + csh[3][tid]);
  }
}

// one launch for many column-sum reductions: out[i] = sum over the splits (in order) of ws[split * n + i]
// (64 columns per workgroup; wave w adds the splits w, w + 4, ... - up to 153 of them for a 320-channel map, a serial chain of as many L2 round trips when one lane walked
// them all: 61 us for 3 MB - and the four partial sums meet in LDS as (S0 + S1) + (S2 + S3): a fixed order)
__global__ __launch_bounds__(256) void colsum_finish_batch_kernel(const sdlt_colsum_finish_desc* descs) {
  __shared__ float part[4][64];
  const sdlt_colsum_finish_desc d = descs[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = blockIdx.x * 64; c0 < d.n; c0 += gridDim.x * 64) {      // (uniform trip count: the barriers below are safe)
    const int i = c0 + lane;
    float a = 0.f;
    if (i < d.n) {
#pragma unroll 8
      for (int sp = wave; sp < d.nsplit; sp += 4) a += d.ws[(int64_t)sp * d.n + i];
    }
    part[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && i < d.n) {
      const float t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      if (d.out32) d.out32[i] = t;
      if (d.out16) ((bf16_t*)d.out16)[i] = f2bf(t);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------- LayerNorm
// one wave per row; lane handles chunks lane, lane+64, ... (C/8 chunks; C <= 2048)
constexpr int LN_MAXCH = 4;

// Every global load of a row (x, gamma, beta / x, dy, gamma, the residual gradient) is ISSUED before the first reduction: the kernels are
// one dependent chain per wave (load -> two wave reductions -> store), and a second round of loads after the reductions cost a second
// L2 / HBM latency per launch - ~600 launches per SDXL step.
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16_t* __restrict__ x, int64_t ldx, int M, int C, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, bf16_t* __restrict__ y, int64_t ldy,
                                                      float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nch = C >> 3;
  uint4 xr[LN_MAXCH];
  f32x4 g4[LN_MAXCH][2], b4[LN_MAXCH][2];
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {      // (unconditional, clamped: one round trip - see ln_bwd_body)
    const int ch = lane + i * 64, cc = ch < nch ? ch : nch - 1;
    xr[i] = *(const uint4*)(x + (int64_t)row * ldx + cc * 8);
    g4[i][0] = *(const f32x4*)(gamma + cc * 8); g4[i][1] = *(const f32x4*)(gamma + cc * 8 + 4);
    b4[i][0] = *(const f32x4*)(beta + cc * 8); b4[i][1] = *(const f32x4*)(beta + cc * 8 + 4);
  }
  float v[LN_MAXCH][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    int ch = lane + i * 64;
    if (ch < nch) {
      const uint32_t w[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[i][2 * j] = bf2f(w[j] & 0xffff); v[i][2 * j + 1] = bf2f(w[j] >> 16); }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[i][j];
    }
  }
  float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    int ch = lane + i * 64;
    if (ch < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { float d = v[i][j] - mean; q += d * d; }
    }
  }
  float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  if (lane == 0 && stats) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    int ch = lane + i * 64;
    if (ch < nch) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * g4[i][j >> 2][j & 3] + b4[i][j >> 2][j & 3];
      store8(y + (int64_t)row * ldy + ch * 8, o);
    }
  }
}

// SLABS: dy arrives as `nslab` fp32 slabs [nslab][M][lddy] (partial outputs of a K-split sdlt_strip_gemm), added here in slab order
// YOUT: the normalised rows y = xhat gamma + beta are written as well (bf16) - for a LayerNorm whose forward was folded into its consumer GEMM
// (sdlt_gemm_params.ln_c1, sdlt_wsk_gemm_ln) no normalised copy exists, and the adapter-gradient launch wants one as its P operand
template <bool SLABS, bool YOUT = false>
__device__ __forceinline__ void ln_bwd_body(const bf16_t* __restrict__ x, int64_t ldx, const void* __restrict__ dy_, int64_t lddy, int nslab, int M,
                                            int C, const float* __restrict__ gamma, const float* __restrict__ stats,
                                            const bf16_t* dres, int64_t lddres, bf16_t* dx, int64_t lddx, const int bx,
                                            const float* __restrict__ beta = nullptr, bf16_t* __restrict__ yout = nullptr, int64_t ldy = 0) {
  const int lane = threadIdx.x & 63;
  const int row = bx * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nch = C >> 3;
  const bf16_t* dy = (const bf16_t*)dy_;
  const float* dy32 = (const float*)dy_;
  uint4 xr[LN_MAXCH], dr[LN_MAXCH], rr[LN_MAXCH];
  f32x4 d32[LN_MAXCH][2];         // (dres may alias dx: read here, before any store of this row - each wave owns its row)
  f32x4 g4[LN_MAXCH][2], b4[YOUT ? LN_MAXCH : 1][2];
  // ONE round trip per wave: every load of the row - and the statistics - is issued unconditionally, from clamped addresses, before anything is consumed.  (Round 5, seen in
  // the ISA: with `if (ch < nch)` / `if (dres)` around the loads and a zero default hipcc copied the loaded registers at each join and put an s_waitcnt vmcnt(0) behind every
  // 8-column chunk - four serial round trips, the statistics a fifth - in a kernel that is nothing but one dependent chain per wave; 253 launches per SDXL step.)  Chunks
  // beyond the row read its last chunk again and are skipped where they would be used; a missing residual gradient reads x instead.
  const float2 mr = *(const float2*)(stats + row * 2);
  const bf16_t* rsrc = dres ? dres + (int64_t)row * lddres : x + (int64_t)row * ldx;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    const int ch = lane + i * 64, cc = ch < nch ? ch : nch - 1;
    xr[i] = *(const uint4*)(x + (int64_t)row * ldx + cc * 8);
    if constexpr (YOUT) { b4[i][0] = *(const f32x4*)(beta + cc * 8); b4[i][1] = *(const f32x4*)(beta + cc * 8 + 4); }
    if constexpr (SLABS) {
      dr[i] = make_uint4(0, 0, 0, 0);
      d32[i][0] = *(const f32x4*)(dy32 + (int64_t)row * lddy + cc * 8);
      d32[i][1] = *(const f32x4*)(dy32 + (int64_t)row * lddy + cc * 8 + 4);
    } else {
      dr[i] = *(const uint4*)(dy + (int64_t)row * lddy + cc * 8);
    }
    g4[i][0] = *(const f32x4*)(gamma + cc * 8); g4[i][1] = *(const f32x4*)(gamma + cc * 8 + 4);
    rr[i] = *(const uint4*)(rsrc + cc * 8);
  }
  if constexpr (SLABS) {          // the other slabs, in slab order (all requested before the first addition is needed)
    for (int sl = 1; sl < nslab; ++sl) {
      f32x4 t[LN_MAXCH][2];
#pragma unroll
      for (int i = 0; i < LN_MAXCH; ++i) {
        const int ch = lane + i * 64, cc = ch < nch ? ch : nch - 1;
        const float* o = dy32 + ((int64_t)sl * M + row) * lddy + cc * 8;
        t[i][0] = *(const f32x4*)o;
        t[i][1] = *(const f32x4*)(o + 4);
      }
#pragma unroll
      for (int i = 0; i < LN_MAXCH; ++i) { d32[i][0] += t[i][0]; d32[i][1] += t[i][1]; }
    }
  }
  const float mean = mr.x, rstd = mr.y;
  float xh[LN_MAXCH][8], dxh[LN_MAXCH][8];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    int ch = lane + i * 64;
    if (ch < nch) {
      const uint32_t xw[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w}, dw[4] = {dr[i].x, dr[i].y, dr[i].z, dr[i].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float vx = bf2f((j & 1) ? (xw[j >> 1] >> 16) : (xw[j >> 1] & 0xffff));
        const float vd = SLABS ? d32[i][j >> 2][j & 3] : bf2f((j & 1) ? (dw[j >> 1] >> 16) : (dw[j >> 1] & 0xffff));
        xh[i][j] = (vx - mean) * rstd;
        dxh[i][j] = vd * g4[i][j >> 2][j & 3];
        s1 += dxh[i][j]; s2 += dxh[i][j] * xh[i][j];
      }
    }
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
#pragma unroll
  for (int i = 0; i < LN_MAXCH; ++i) {
    int ch = lane + i * 64;
    if (ch < nch) {
      const uint32_t rw[4] = {rr[i].x, rr[i].y, rr[i].z, rr[i].w};
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (dres ? bf2f((j & 1) ? (rw[j >> 1] >> 16) : (rw[j >> 1] & 0xffff)) : 0.f) + rstd * (dxh[i][j] - s1 - xh[i][j] * s2);
      store8(dx + (int64_t)row * lddx + ch * 8, o);
      if constexpr (YOUT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = xh[i][j] * g4[i][j >> 2][j & 3] + b4[i][j >> 2][j & 3];
        store8(yout + (int64_t)row * ldy + ch * 8, o);
      }
    }
  }
}

__global__ __launch_bounds__(256) void ln_bwd_y_kernel(const bf16_t* __restrict__ x, int64_t ldx, const void* __restrict__ dy_, int64_t lddy, int M,
                                                        int C, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ stats,
                                                        const bf16_t* dres, int64_t lddres, bf16_t* dx, int64_t lddx, bf16_t* __restrict__ yout, int64_t ldy) {
  ln_bwd_body<false, true>(x, ldx, dy_, lddy, 1, M, C, gamma, stats, dres, lddres, dx, lddx, blockIdx.x, beta, yout, ldy);
}

// Operands of a rank-16 adapter behind a folded LayerNorm (sdlt_ln_fold_adapters): one wave per (adapter, rank row)
__global__ __launch_bounds__(64) void ln_fold_adapter_kernel(const sdlt_ln_fold_desc* __restrict__ descs) {
  const sdlt_ln_fold_desc d = descs[blockIdx.x];
  const int r = blockIdx.y, lane = threadIdx.x;
  bf16_t* dst = (bf16_t*)d.Ag + (int64_t)r * d.ldag;
  float s1 = 0.f, s2 = 0.f;
  if (r < d.rank) {
    const float* a = d.A32 + (int64_t)r * d.lda;
    for (int k = lane * 4; k < d.K; k += 256) {
      const f32x4 av = *(const f32x4*)(a + k), gv = *(const f32x4*)(d.gamma + k), bv = *(const f32x4*)(d.beta + k);
      const uint32_t lo = pack2bf(av[0] * gv[0], av[1] * gv[1]), hi = pack2bf(av[2] * gv[2], av[3] * gv[3]);
      *(uint2*)(dst + k) = make_uint2(lo, hi);
      s1 += bf2f(lo & 0xffff) + bf2f(lo >> 16) + bf2f(hi & 0xffff) + bf2f(hi >> 16);      // cA from the ROUNDED operand: the mean term cancels what the product adds
      s2 += av[0] * bv[0] + av[1] * bv[1] + av[2] * bv[2] + av[3] * bv[3];
    }
  } else {
    for (int k = lane * 4; k < d.K; k += 256) *(uint2*)(dst + k) = make_uint2(0u, 0u);
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (lane == 0) { d.consts[r] = s1; d.consts[16 + r] = s2; }
}

template <bool SLABS>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ x, int64_t ldx, const void* __restrict__ dy_, int64_t lddy, int nslab, int M,
                                                      int C, const float* __restrict__ gamma, const float* __restrict__ stats,
                                                      const bf16_t* dres, int64_t lddres, bf16_t* dx, int64_t lddx) {
  ln_bwd_body<SLABS>(x, ldx, dy_, lddy, nslab, M, C, gamma, stats, dres, lddres, dx, lddx, blockIdx.x);
}
// two independent problems in one launch (blockIdx.y picks): see strip_pair_kernel
__global__ __launch_bounds__(256) void ln_bwd_slabs_pair_kernel(const sdlt_ln_slabs_params a, const sdlt_ln_slabs_params b) {
  const sdlt_ln_slabs_params& p = blockIdx.y == 0 ? a : b;
  ln_bwd_body<true>((const bf16_t*)p.x, p.ldx, p.dy32, p.lddy32, p.nslab, p.M, p.C, p.gamma, p.stats, (const bf16_t*)p.dres, p.lddres, (bf16_t*)p.dx, p.lddx, blockIdx.x);
}

int gn_check(const sdlt_groupnorm_params& p, const char* fn) {
  if (p.B <= 0 || p.HW <= 0 || p.C <= 0 || (p.C % 64)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: B=%d HW=%d C=%d (C %% 64 == 0 required)", fn, p.B, p.HW, p.C);
  if (p.x2 ? ((p.C1 % 8) || p.C1 <= 0 || p.C1 >= p.C || (p.ldx2 % 8)) : (p.C1 != p.C)) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: concat split C1=%d of C=%d", fn, p.C1, p.C);
  if ((p.ldx1 % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ldx %% 8", fn);
  return SDLT_OK;
}

dim3 gn_grid(const sdlt_groupnorm_params& p) {
  int cb = p.C / 64;
  int want = 768 / (cb * p.B);                  // ~3 workgroups per CU in total: every block leaves a row of partial sums that the
                                                // last block to arrive has to read (gn_reduce_finalize), so not too many
  int maxsplit = (p.HW + 31) / 32;
  int rs = want < 1 ? 1 : (want > maxsplit ? maxsplit : want);
  return dim3(cb, rs, p.B);
}

int gn_ws_check(const sdlt_groupnorm_params& p, dim3 grid, const char* fn) {
  const int64_t need = (int64_t)grid.x * grid.y * grid.z * 64;
  if (!p.ws || p.ws_floats < need)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: statistics workspace too small (%lld floats / %d counters needed)", fn, (long long)need, p.B);
  return SDLT_OK;
}

}  // namespace

extern "C" int sdlt_groupnorm_ws_floats(int32_t B, int32_t HW, int32_t C) {
  sdlt_groupnorm_params p{};
  p.B = B; p.HW = HW; p.C = C;
  dim3 g = gn_grid(p);
  return (int)(g.x * g.y * g.z * 64);
}

extern "C" int sdlt_groupnorm_fwd(const sdlt_groupnorm_params* pp, void* stream) {
  const sdlt_groupnorm_params& p = *pp;
  hipStream_t s = (hipStream_t)stream;
  int rc = gn_check(p, "sdlt_groupnorm_fwd");
  if (rc) return rc;
  if (p.ldy % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_groupnorm_fwd: ldy %% 8");
  CatIn in{(const bf16_t*)p.x1, p.ldx1, p.C1, (const bf16_t*)p.x2, p.ldx2};
  dim3 grid = gn_grid(p);
  rc = gn_ws_check(p, grid, "sdlt_groupnorm_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(256), 0, s, in, p.HW, p.C, p.ws);
  if (p.silu)
    hipLaunchKernelGGL(gn_apply_kernel<true>, grid, dim3(256), 0, s, in, p.HW, p.C, p.stats, p.ws, p.gamma, p.beta, p.eps, (bf16_t*)p.y, p.ldy);
  else
    hipLaunchKernelGGL(gn_apply_kernel<false>, grid, dim3(256), 0, s, in, p.HW, p.C, p.stats, p.ws, p.gamma, p.beta, p.eps, (bf16_t*)p.y, p.ldy);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_groupnorm_bwd(const sdlt_groupnorm_params* pp, void* stream) {
  const sdlt_groupnorm_params& p = *pp;
  hipStream_t s = (hipStream_t)stream;
  int rc = gn_check(p, "sdlt_groupnorm_bwd");
  if (rc) return rc;
  if ((p.lddy % 8) || (p.lddx % 8) || (p.dres && (p.lddres % 8))) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_groupnorm_bwd: ld %% 8");
  CatIn in{(const bf16_t*)p.x1, p.ldx1, p.C1, (const bf16_t*)p.x2, p.ldx2};
  dim3 grid = gn_grid(p);
  rc = gn_ws_check(p, grid, "sdlt_groupnorm_bwd");
  if (rc) return rc;
  if (p.silu) {
    hipLaunchKernelGGL(gn_bwd_stats_kernel<true>, grid, dim3(256), 0, s, in, (const bf16_t*)p.dy, p.lddy, p.HW, p.C, p.stats, p.gamma, p.beta, p.eps, p.ws);
    hipLaunchKernelGGL(gn_bwd_apply_kernel<true>, grid, dim3(256), 0, s, in, (const bf16_t*)p.dy, p.lddy, p.HW, p.C, p.stats, p.bstats, p.ws, p.gamma, p.beta, p.eps, (const bf16_t*)p.dres, p.lddres, (bf16_t*)p.dx, p.lddx, p.colsum_ws);
  } else {
    hipLaunchKernelGGL(gn_bwd_stats_kernel<false>, grid, dim3(256), 0, s, in, (const bf16_t*)p.dy, p.lddy, p.HW, p.C, p.stats, p.gamma, p.beta, p.eps, p.ws);
    hipLaunchKernelGGL(gn_bwd_apply_kernel<false>, grid, dim3(256), 0, s, in, (const bf16_t*)p.dy, p.lddy, p.HW, p.C, p.stats, p.bstats, p.ws, p.gamma, p.beta, p.eps, (const bf16_t*)p.dres, p.lddres, (bf16_t*)p.dx, p.lddx, p.colsum_ws);
  }
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_colsum_finish_batch(const sdlt_colsum_finish_desc* descs_dev, int32_t n_desc, int32_t max_n, void* stream) {
  if (n_desc <= 0) return SDLT_OK;
  if (!descs_dev || max_n <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_colsum_finish_batch: descs == NULL or max_n=%d", max_n);
  int gx = (max_n + 63) / 64;
  hipLaunchKernelGGL(colsum_finish_batch_kernel, dim3(gx > 64 ? 64 : gx, n_desc), dim3(256), 0, (hipStream_t)stream, descs_dev);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_layernorm_fwd(const void* x, int64_t ldx, int32_t M, int32_t C, const float* gamma, const float* beta,
                                  float eps, void* y, int64_t ldy, float* stats, void* stream) {
  if (M <= 0 || C <= 0 || (C % 8) || C > LN_MAXCH * 512) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_layernorm_fwd: M=%d C=%d (C%%8==0, C<=%d)", M, C, LN_MAXCH * 512);
  if ((ldx % 8) || (ldy % 8)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_layernorm_fwd: ld %% 8");
  hipLaunchKernelGGL(ln_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, M, C, gamma, beta, eps, (bf16_t*)y, ldy, stats);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_layernorm_bwd(const void* x, int64_t ldx, const void* dy, int64_t lddy, int32_t M, int32_t C,
                                  const float* gamma, const float* stats, const void* dres, int64_t lddres, void* dx,
                                  int64_t lddx, void* stream) {
  if (M <= 0 || C <= 0 || (C % 8) || C > LN_MAXCH * 512) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_layernorm_bwd: M=%d C=%d", M, C);
  if ((ldx % 8) || (lddy % 8) || (lddx % 8) || (dres && (lddres % 8))) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_layernorm_bwd: ld %% 8");
  hipLaunchKernelGGL(ln_bwd_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, dy, lddy, 1, M, C, gamma, stats, (const bf16_t*)dres, lddres, (bf16_t*)dx, lddx);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_layernorm_bwd_y(const void* x, int64_t ldx, const void* dy, int64_t lddy, int32_t M, int32_t C, const float* gamma, const float* beta,
                                    const float* stats, const void* dres, int64_t lddres, void* dx, int64_t lddx, void* y, int64_t ldy, void* stream) {
  if (M <= 0 || C <= 0 || (C % 8) || C > LN_MAXCH * 512) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_layernorm_bwd_y: M=%d C=%d", M, C);
  if (!beta || !y || (ldx % 8) || (lddy % 8) || (lddx % 8) || (ldy % 8) || (dres && (lddres % 8))) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_layernorm_bwd_y: beta / y required, ld %% 8");
  hipLaunchKernelGGL(ln_bwd_y_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, dy, lddy, M, C, gamma, beta, stats,
                     (const bf16_t*)dres, lddres, (bf16_t*)dx, lddx, (bf16_t*)y, ldy);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_ln_fold_adapters(const sdlt_ln_fold_desc* descs, int32_t n, void* stream) {
  if (n <= 0) return SDLT_OK;
  if (!descs) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_ln_fold_adapters: descs == NULL");
  hipLaunchKernelGGL(ln_fold_adapter_kernel, dim3(n, 16), dim3(64), 0, (hipStream_t)stream, descs);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_layernorm_bwd_slabs(const void* x, int64_t ldx, const float* dy32, int64_t lddy32, int32_t nslab, int32_t M, int32_t C,
                                        const float* gamma, const float* stats, const void* dres, int64_t lddres, void* dx, int64_t lddx, void* stream) {
  if (M <= 0 || C <= 0 || (C % 8) || C > LN_MAXCH * 512 || nslab < 1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_layernorm_bwd_slabs: M=%d C=%d nslab=%d", M, C, nslab);
  if ((ldx % 8) || (lddy32 % 4) || (lddx % 8) || (dres && (lddres % 8)) || ((uintptr_t)dy32 & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_layernorm_bwd_slabs: alignment");
  hipLaunchKernelGGL(ln_bwd_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, dy32, lddy32, nslab, M, C, gamma, stats, (const bf16_t*)dres, lddres, (bf16_t*)dx, lddx);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

// reference: none (launch structure only): two sdlt_layernorm_bwd_slabs problems in one launch
extern "C" int sdlt_layernorm_bwd_slabs_pair(const sdlt_ln_slabs_params* pa, const sdlt_ln_slabs_params* pb, void* stream) {
  for (const sdlt_ln_slabs_params* q : {pa, pb}) {
    const sdlt_ln_slabs_params& p = *q;
    if (p.M <= 0 || p.C <= 0 || (p.C % 8) || p.C > LN_MAXCH * 512 || p.nslab < 1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_layernorm_bwd_slabs_pair: M=%d C=%d nslab=%d", p.M, p.C, p.nslab);
    if ((p.ldx % 8) || (p.lddy32 % 4) || (p.lddx % 8) || (p.dres && (p.lddres % 8)) || ((uintptr_t)p.dy32 & 15)) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_layernorm_bwd_slabs_pair: alignment");
  }
  const int ma = (pa->M + 3) / 4, mb = (pb->M + 3) / 4;
  hipLaunchKernelGGL(ln_bwd_slabs_pair_kernel, dim3(ma > mb ? ma : mb, 2), dim3(256), 0, (hipStream_t)stream, *pa, *pb);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
