// Optimizer kernels of the training step (gfx950): fused AdamW (+ L1) on a flat fp32 arena, AdamW and AdamW8bit fused into the bf16 operand-refresh
// tiles (LoRA adapters, every UNet weight of the full fine-tune), AdamW8bit on a flat range (sharded optimizer), Prodigy.
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

// ------------------------------------------------------------------ fused AdamW (+ L1 subgradient), fp32 master params
// reference: torch.optim.AdamW built at trainer/optimizer.py:18 / :113-150, stepped at optimizer.py:270-275,
// L1 penalty main.py:353-356 (grad of l1w * sum|p| / N is l1w*sign(p)/N, folded in here).
// hyper (device, fp32): [0] lr  [1] beta1  [2] beta2  [3] eps  [4] weight_decay  [5] 1-beta1^t  [6] 1-beta2^t
//                       [7] l1 coefficient (= l1_penalty * loss_scale / N_total)  [8] grad scale
struct AdamwHyper { float lr, b1, b2, eps, wd, bc1, bc2, l1c, gs; };
__device__ __forceinline__ AdamwHyper adamw_hyper(const float* hyper) {
  return {hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6], hyper[7], hyper[8]};
}
// torch.optim.AdamW (decoupled decay), L1: + the L1 subgradient of main.py:353-356; rs2 = rsqrtf(bc2), step = lr / bc1 (the caller decides where they are computed)
template <bool L1>
__device__ __forceinline__ void adamw_update(const AdamwHyper& h, float rs2, float step, float& pi, const float g_, float& mi, float& vi) {
  const float gi = L1 ? g_ * h.gs + h.l1c * (pi > 0.f ? 1.f : (pi < 0.f ? -1.f : 0.f)) : g_ * h.gs;
  mi = h.b1 * mi + (1.f - h.b1) * gi;
  vi = h.b2 * vi + (1.f - h.b2) * gi * gi;
  pi = pi * (1.f - h.lr * h.wd) - step * mi / (sqrtf(vi) * rs2 + h.eps);
}

__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, float* l1_partial, int vec) {
  const AdamwHyper h = adamw_hyper(hyper);
  const float rs2 = rsqrtf(h.bc2), step = h.lr / h.bc1;
  float l1 = 0.f;
  auto upd = [&](float& pi, const float g_, float& mi, float& vi) {
    l1 += fabsf(pi);
    adamw_update<true>(h, rs2, step, pi, g_, mi, vi);
  };
  // 16 bytes per lane and stream (seven streams: the kernel is pure HBM traffic); the arenas are 16-byte aligned (checked by the launcher), the
  // last n % 4 elements go one by one
  const int64_t n4 = vec ? n >> 2 : 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = ((const f32x4*)p)[i], mv = ((const f32x4*)m)[i], vv = ((const f32x4*)v)[i];
    const f32x4 gv = ((const f32x4*)g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pi = pv[k], mi = mv[k], vi = vv[k];
      upd(pi, gv[k], mi, vi);
      pv[k] = pi; mv[k] = mi; vv[k] = vi;
    }
    ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
  }
  for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    upd(pi, g[i], mi, vi);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
  if (l1_partial) {      // one atomic per workgroup (16384 wave-level atomics onto one address took longer than the kernel's HBM traffic: 235 us for 713 MB)
    __shared__ float l1w[4];
    l1 = wave_sum(l1);
    if ((threadIdx.x & 63) == 0) l1w[threadIdx.x >> 6] = l1;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += l1w[w];
      atomicAdd(l1_partial, t);
    }
  }
}

// ------------------------------------------------------------------ bf16 compute copies (both orientations) of an fp32 master arena
// one descriptor per parameter tensor [rows, cols] (row stride src_ld in the arena):
//   dst  [rows, ld ]  <- same orientation        dstT [cols, ldT] <- transposed
// One workgroup per 64x64 tile: the fp32 rows are read as 256-B lines, converted once, and both copies leave as
// contiguous runs along their own fast axis (the transposed one through LDS).  Used for the LoRA adapters (a few MB) and
// for every UNet weight of the full fine-tune (2.57 G parameters: 10 GB read, 2 x 5 GB written per step).
// ADAMW: the same tiles also carry the optimizer step (p, g, m, v read, p, m, v written) before the conversion - one pass over
// the 2.57 G parameters of the full fine-tune instead of AdamW's 7 words + the refresh's re-read of p.
__device__ __forceinline__ sdlt_shadow_desc tile_origin(const sdlt_shadow_desc* descs, const int32_t* block_desc, const int32_t* block_first, int& r0, int& c0) {
  const sdlt_shadow_desc d = descs[block_desc[blockIdx.x]];
  const int t = blockIdx.x - block_first[block_desc[blockIdx.x]];
  const int tiles_c = (d.cols + 63) >> 6;
  r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
  return d;
}
// the finished 64 x 72 LDS tile -> dst rows / dstT rows: 16 bf16 per lane, two 16-byte stores where the run is whole and aligned
__device__ __forceinline__ void tile_store(const sdlt_shadow_desc& d, int r0, int c0, const bf16_t (*tile)[72]) {
  const int q = threadIdx.x >> 2, ch = (threadIdx.x & 3) * 16;
  if (d.dst) {
    const int r = r0 + q;
    if (r < d.rows) {
      bf16_t* p = (bf16_t*)d.dst + (int64_t)r * d.ld + c0 + ch;
      if (c0 + ch + 16 <= d.cols && (((uintptr_t)p) & 15) == 0) {
        *(uint4*)p = *(const uint4*)&tile[q][ch];
        *(uint4*)(p + 8) = *(const uint4*)&tile[q][ch + 8];
      } else {
        for (int j = 0; j < 16 && c0 + ch + j < d.cols; ++j) p[j] = tile[q][ch + j];
      }
    }
  }
  if (d.dstT) {
    const int c = c0 + q;
    if (c < d.cols) {
      bf16_t v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = tile[ch + j][q];
      bf16_t* p = (bf16_t*)d.dstT + (int64_t)c * d.ldT + r0 + ch;
      if (r0 + ch + 16 <= d.rows && (((uintptr_t)p) & 15) == 0) {
        *(uint4*)p = *(const uint4*)&v[0];
        *(uint4*)(p + 8) = *(const uint4*)&v[8];
      } else {
        for (int j = 0; j < 16 && r0 + ch + j < d.rows; ++j) p[j] = v[j];
      }
    }
  }
}

template <bool ADAMW>
__global__ __launch_bounds__(256) void shadow_kernel(const sdlt_shadow_desc* descs, const int32_t* block_desc, const int32_t* block_first,
                                                     float* arena, const float* g, float* m, float* v, const float* hyper) {
  __shared__ bf16_t tile[64][72];
  int r0, c0;
  const sdlt_shadow_desc d = tile_origin(descs, block_desc, block_first, r0, c0);
  const int thr = threadIdx.x;
  {
    const int c = c0 + (thr & 63);
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int r = r0 + k * 4 + (thr >> 6);
      float val = 0.f;
      if (r < d.rows && c < d.cols) {
        const int64_t i = d.offset + (int64_t)r * d.src_ld + c;
        val = arena[i];
        if (ADAMW) {          // (no L1 term: main.py:353 applies it to LoRA tensors only)
          const AdamwHyper h = adamw_hyper(hyper);
          float mi = m[i], vi = v[i];
          adamw_update<false>(h, rsqrtf(h.bc2), h.lr / h.bc1, val, g[i], mi, vi);
          arena[i] = val; m[i] = mi; v[i] = vi;
        }
      }
      tile[k * 4 + (thr >> 6)][thr & 63] = f2bf(val);
    }
  }
  __syncthreads();
  tile_store(d, r0, c0, tile);
}

// ------------------------------------------------------------------ AdamW8bit: block-quantised moments, fused into the refresh tiles
// bitsandbytes 0.43.1 `AdamW8bit` (trainer/optimizer.py:19-21; the optimizer full_finetuning_example.json names), restated from its published blockwise
// 8-bit Adam (kOptimizerStatic8bit2StateBlockwise): both moments live as one byte per element - an index into a 256-entry code book ("dynamic" map, signed
// for m, unsigned for v) - times one fp32 absmax per block of 2048 elements.  Per step and block: dequantise, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
// new absmax = max |m|, max v over the block, p += -lr sqrt(bc2) / bc1 * m / (sqrt(v) + sqrt(bc2) eps), then p *= 1 - lr wd, requantise m / absmax and
// v / absmax to the nearest code (m keeps its sign: a code of the other sign moves one step towards it).
// Here a block is one half of a 64 x 64 refresh tile (32 rows x 64 columns = 2048 elements of the weight's [N, K] view) instead of 2048 consecutive elements of
// the flattened tensor: the tile is the unit this pass already owns (fp32 master in, W and W^T bf16 out), so the whole optimizer step stays ONE pass
// - p, g 4 B + m, v 1 B in, p 4 B + m, v 1 B + two bf16 copies out = 20 B per parameter instead of 32 B with fp32 moments.
// m8 / v8: tile-major, uint8 [n_blocks][64][64] (tile b of the descriptor table, element (r, c) of the tile at 4096 b + 64 r + c; positions outside the tensor unused).
// tables (fp32, device): q1[256] | mid1[256] | q2[256] | mid2[256], mid[k] = (q[k] + q[k + 1]) / 2, mid[255] = +inf.  absmax: [n_blocks][4] = {m rows 0-31, m rows 32-63,
// v rows 0-31, v rows 32-63}.  The nearest code is found from the code book's structure (decade i holds 2^i (signed) / 2^(i+1) (unsigned) equally spaced values in
// 10^(i-6) [0.1, 1]: q8_guess) and corrected by at most one step against the two neighbouring midpoints (q8_fix): two LDS reads instead of bnb's eight-step search.
template <bool SIGNED>
__device__ __forceinline__ int q8_guess(float x) {
  const float a = fabsf(x);
  const float L = __builtin_amdgcn_logf(fmaxf(a, 1e-7f)) * 0.30102999566f + 7.f;          // log10(a) + 7 in [0, 7]
  int i = (int)L;
  i = i > 6 ? 6 : i;
  const int n = SIGNED ? (1 << i) : (2 << i);
  // cell j = floor((a 10^(6-i) - 0.1) n / 0.9) = floor(a K - n / 9), K = 10^(6-i) 2^i / 0.9 = exp2(log2(1e6 / 0.9) - i log2(5))   (unsigned book: twice the cells)
  const float K = __builtin_amdgcn_exp2f((SIGNED ? 20.083571662f : 21.083571662f) - (float)i * 2.321928095f);
  int j = (int)(a * K - ldexpf(SIGNED ? (1.f / 9.f) : (2.f / 9.f), i));
  j = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
  const int pos = n - 1 + j;
  return SIGNED ? (x >= 0.f ? 128 + pos : 126 - pos) : pos;               // 0 <= c <= 254: the nearest code or one of its neighbours
}
// ... corrected against the midpoints on either side of the guess (up = mid[c], dn = mid[max(c - 1, 0)]); plain integer arithmetic on the comparisons, so that the
// compiler keeps the two LDS reads unconditional and batched instead of turning a select into a divergent branch per element
__device__ __forceinline__ int q8_fix(int c, float x, float up, float dn) { return c + (int)(x > up) - (int)((c > 0) & (x <= dn)); }

// hyper as for adamw_kernel ([7] unused); the constants every form derives from it
struct Adam8Consts { float b1, b2, gs, step_size, eps2, decay; };
__device__ __forceinline__ Adam8Consts adam8_consts(const float* hyper) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6], gs = hyper[8];
  const float c2 = sqrtf(bc2), step_size = -lr * c2 / bc1, eps2 = c2 * eps, decay = wd > 0.f ? 1.f - lr * wd : 1.f;
  return {b1, b2, gs, step_size, eps2, decay};
}
// one element: decode both moments (tb = q1 | mid1 | q2 | mid2 in LDS), the recurrences (!valid: moments 0), the new parameter
struct Adam8Elem { float mi, vi, val; };
__device__ __forceinline__ Adam8Elem adam8_update(const Adam8Consts& k, const float* tb, uint32_t code_m, uint32_t code_v, float g, float p, float absmax_m, float absmax_v, bool valid) {
  const float gi = g * k.gs;
  float mi = k.b1 * (tb[code_m] * absmax_m) + (1.f - k.b1) * gi;
  float vi = k.b2 * (tb[512 + code_v] * absmax_v) + (1.f - k.b2) * gi * gi;
  if (!valid) mi = vi = 0.f;
  // (hardware square root and reciprocal, 1 ulp each - bnb's own kernel divides with __fdividef)
  return {mi, vi, (p + k.step_size * (mi * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vi) + k.eps2))) * k.decay};
}
// ... and its contribution to the lane's running block maxima
__device__ __forceinline__ void adam8_track(const Adam8Elem& u, float& mn, float& vn, float& mxm, float& mxv) {
  mn = u.mi; vn = u.vi;
  mxm = fmaxf(mxm, fabsf(u.mi));
  mxv = fmaxf(mxv, u.vi);
}
// the lanes' NB running maxima -> the workgroup's (four waves, through red) and their reciprocals (0 for an all-zero block); the barrier also publishes the bf16 tile
template <int NB>
__device__ __forceinline__ void adam8_block_max(float (&mx)[NB], float (&inv)[NB], float (*red)[NB]) {
  typedef float fvec __attribute__((ext_vector_type(NB)));
  fvec w;
#pragma unroll
  for (int u = 0; u < NB; ++u) w[u] = wave_max(mx[u]);
  if ((threadIdx.x & 63) == 0) *(fvec*)&red[threadIdx.x >> 6][0] = w;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    mx[u] = fmaxf(fmaxf(red[0][u], red[1][u]), fmaxf(red[2][u], red[3][u]));
    inv[u] = mx[u] > 0.f ? __builtin_amdgcn_rcpf(mx[u]) : 0.f;
  }
}
// E new moments of one block -> codes: ALL guesses, then ALL midpoint reads (4 E LDS reads in flight), then the fixes and m's sign rule.  E == 4: one dword of each
// moment (o[0]); otherwise E scalar codes
template <int E>
__device__ __forceinline__ void adam8_requant(const float* tb, const float (&mn)[E], const float (&vn)[E], float inv_m, float inv_v, uint32_t (&o1)[E == 4 ? 1 : E],
                                              uint32_t (&o2)[E == 4 ? 1 : E]) {
  float x1[E], x2[E], u1[E], d1[E], u2[E], d2[E];
  int g1[E], g2[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    x1[e] = mn[e] * inv_m;
    x2[e] = vn[e] * inv_v;
    g1[e] = q8_guess<true>(x1[e]);
    g2[e] = q8_guess<false>(x2[e]);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    u1[e] = tb[256 + g1[e]]; d1[e] = tb[256 + (g1[e] > 0 ? g1[e] - 1 : 0)];
    u2[e] = tb[768 + g2[e]]; d2[e] = tb[768 + (g2[e] > 0 ? g2[e] - 1 : 0)];
  }
  uint32_t w1 = 0, w2 = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int q1 = q8_fix(g1[e], x1[e], u1[e], d1[e]);
    q1 += ((q1 < 127) != (mn[e] < 0.f)) ? (mn[e] > 0.f ? 1 : -1) : 0;   // m keeps its sign (codes below 127 are the negative ones; the code of 0 counts as positive)
    const int q2 = q8_fix(g2[e], x2[e], u2[e], d2[e]);
    if constexpr (E == 4) { w1 |= (uint32_t)q1 << (8 * e); w2 |= (uint32_t)q2 << (8 * e); }
    else { o1[e] = (uint32_t)q1; o2[e] = (uint32_t)q2; }
  }
  if constexpr (E == 4) { o1[0] = w1; o2[0] = w2; }
}

// FULL: the tile lies inside the tensor (no row / column tests, no clamped addresses)
template <bool FULL>
__device__ __forceinline__ void adamw8_tile(const sdlt_shadow_desc& d, int r0, int c0, float* arena, const float* g, uint8_t* m8, uint8_t* v8, float* absmax_blk,
                                            const float* hyper, const float* tb, float (*red)[4], bf16_t (*tile)[72]) {
  const int thr = threadIdx.x, wave = thr >> 6, lane = thr & 63;
  const float4 am = *(const float4*)absmax_blk;
  const Adam8Consts kc = adam8_consts(hyper);
  const int c = c0 + lane;
  // element (row r0 + 4 k + wave, column c) = tile origin (uniform: a scalar base address) + a 32-bit per-lane offset
  const int64_t org = d.offset + (int64_t)r0 * d.src_ld + c0;
  float* pa = arena + org;
  const float* pg = g + org;
  // codes: tile-major (4096 per tile, row r of the tile at 64 r): a wave's requests are whole 128-byte lines whatever the tensor's row stride
  uint8_t* pm = m8 + (int64_t)blockIdx.x * 4096;
  uint8_t* pq = v8 + (int64_t)blockIdx.x * 4096;
  const uint32_t lo = (uint32_t)wave * (uint32_t)d.src_ld + lane, rstep = 4u * (uint32_t)d.src_ld;
  const uint32_t clo = (uint32_t)wave * 64u + lane;          // (element (4 k + wave, lane) of the tile)
  // all 64 requests of the lane first (unconditional; ragged tiles read element 0 of the tensor instead), then the arithmetic
  float pv[16], gv[16];
  uint8_t cm[16], cv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const bool ok = FULL || (r0 + k * 4 + wave < d.rows && c < d.cols);
    const uint32_t i = ok ? lo + k * rstep : 0u;
    pv[k] = pa[i]; gv[k] = pg[i]; cm[k] = pm[clo + k * 256]; cv[k] = pq[clo + k * 256];
  }
  __syncthreads();                                                  // the tables are in LDS
  float mn[2][8], vn[2][8], mx[4] = {0.f, 0.f, 0.f, 0.f}, inv[4];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int h = k >> 3;
    const bool ok = FULL || (r0 + k * 4 + wave < d.rows && c < d.cols);
    const Adam8Elem u = adam8_update(kc, tb, cm[k], cv[k], gv[k], pv[k], h ? am.y : am.x, h ? am.w : am.z, ok);
    adam8_track(u, mn[h][k & 7], vn[h][k & 7], mx[h], mx[2 + h]);
    if (ok) pa[lo + k * rstep] = u.val;
    tile[k * 4 + wave][lane] = f2bf(ok ? u.val : 0.f);
  }
  adam8_block_max<4>(mx, inv, red);
  if (thr == 0) *(float4*)absmax_blk = (float4){mx[0], mx[1], mx[2], mx[3]};
#pragma unroll
  for (int h = 0; h < 2; ++h) {                                     // one block of 2048 (8 elements per lane) at a time
    uint32_t q1[8], q2[8];
    adam8_requant<8>(tb, mn[h], vn[h], inv[h], inv[2 + h], q1, q2);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = h * 8 + e;
      if (FULL || (r0 + k * 4 + wave < d.rows && c < d.cols)) { pm[clo + k * 256] = (uint8_t)q1[e]; pq[clo + k * 256] = (uint8_t)q2[e]; }
    }
  }
}

// The same tile with 16-byte accesses (interior tiles of tensors whose rows are 16-byte aligned - every tile of the SDXL UNet but the ragged edges): a lane owns four consecutive
// columns of four rows (row = 16 k + 4 wave + lane / 16), i.e. one float4 of p and g and one dword of codes per row instead of four scalar requests each - 28 memory
// instructions per lane instead of 112, and a quarter of the address arithmetic.
__device__ __forceinline__ void adamw8_tile_vec(const sdlt_shadow_desc& d, int r0, int c0, float* arena, const float* g, uint8_t* m8, uint8_t* v8, float* absmax_blk,
                                                const float* hyper, const float* tb, float (*red)[4], bf16_t (*tile)[72]) {
  const int thr = threadIdx.x, wave = thr >> 6, lane = thr & 63, cq = lane & 15, rq = lane >> 4;
  const float4 am = *(const float4*)absmax_blk;
  const Adam8Consts kc = adam8_consts(hyper);
  const int64_t org = d.offset + (int64_t)r0 * d.src_ld + c0;
  float* pa = arena + org;
  const float* pg = g + org;
  uint8_t* pm = m8 + (int64_t)blockIdx.x * 4096;      // tile-major codes: row r of the tile at 64 r (a wave's four rows are 256 contiguous bytes)
  uint8_t* pq = v8 + (int64_t)blockIdx.x * 4096;
  const uint32_t lo = (uint32_t)(wave * 4 + rq) * (uint32_t)d.src_ld + 4u * cq, rstep = 16u * (uint32_t)d.src_ld;
  const uint32_t clo = (uint32_t)(wave * 4 + rq) * 64u + 4u * cq;
  float4 pv[4], gv[4];
  uint32_t cm[4], cv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = lo + k * rstep;
    pv[k] = *(const float4*)(pa + i); gv[k] = *(const float4*)(pg + i);
    cm[k] = *(const uint32_t*)(pm + clo + k * 1024); cv[k] = *(const uint32_t*)(pq + clo + k * 1024);
  }
  __syncthreads();                                                  // the tables are in LDS
  float mn[4][4], vn[4][4], mx[4] = {0.f, 0.f, 0.f, 0.f}, inv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int h = k >> 1;
    float val[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const Adam8Elem u = adam8_update(kc, tb, (cm[k] >> (8 * e)) & 255u, (cv[k] >> (8 * e)) & 255u, gv[k][e], pv[k][e], h ? am.y : am.x, h ? am.w : am.z, true);
      adam8_track(u, mn[k][e], vn[k][e], mx[h], mx[2 + h]);
      val[e] = u.val;
    }
    *(float4*)(pa + lo + k * rstep) = (float4){val[0], val[1], val[2], val[3]};
    *(uint2*)&tile[k * 16 + wave * 4 + rq][4 * cq] = (uint2){pack2bf(val[0], val[1]), pack2bf(val[2], val[3])};
  }
  adam8_block_max<4>(mx, inv, red);
  if (thr == 0) *(float4*)absmax_blk = (float4){mx[0], mx[1], mx[2], mx[3]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                     // one row (four codes of each moment = one dword each) at a time
    uint32_t w1[1], w2[1];
    adam8_requant<4>(tb, mn[k], vn[k], inv[k >> 1], inv[2 + (k >> 1)], w1, w2);
    *(uint32_t*)(pm + clo + k * 1024) = w1[0]; *(uint32_t*)(pq + clo + k * 1024) = w2[0];
  }
}

// The same update on a FLAT range (the owned slices of the sharded optimizer, data-parallel full fine-tune): one workgroup per block of 2048 CONSECUTIVE elements - bitsandbytes' own
// partition, counted from the start of the range -, eight elements per lane (two float4 of p and g, two dwords of codes), no operand refresh (the masters are all-gathered first).
// absmax: fp32 [ceil(n / 2048)][2] = {m, v}.  n % 4 == 0; the last block may be short.
__global__ __launch_bounds__(256) void adamw8_flat_kernel(float* p, const float* g, uint8_t* m8, uint8_t* v8, float* absmax, int64_t n, const float* tables, const float* hyper) {
  __shared__ float tb[1024];
  __shared__ float red[4][2];
  const int thr = threadIdx.x;
  ((uint4*)tb)[thr] = ((const uint4*)tables)[thr];
  const int64_t e0 = (int64_t)blockIdx.x * 2048 + thr * 8;
  const float2 am = *(const float2*)(absmax + 2 * (int64_t)blockIdx.x);
  const Adam8Consts kc = adam8_consts(hyper);
  float4 pv[2], gv[2];
  uint32_t cm[2], cv[2];
  bool ok[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {      // (unconditional requests; a quad past the end reads the range's first elements and is dropped)
    ok[k] = e0 + 4 * k < n;
    const int64_t i = ok[k] ? e0 + 4 * k : 0;
    pv[k] = *(const float4*)(p + i); gv[k] = *(const float4*)(g + i);
    cm[k] = *(const uint32_t*)(m8 + i); cv[k] = *(const uint32_t*)(v8 + i);
  }
  __syncthreads();
  float mn[2][4], vn[2][4], mx[2] = {0.f, 0.f}, inv[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float val[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const Adam8Elem u = adam8_update(kc, tb, (cm[k] >> (8 * e)) & 255u, (cv[k] >> (8 * e)) & 255u, gv[k][e], pv[k][e], am.x, am.y, ok[k]);
      adam8_track(u, mn[k][e], vn[k][e], mx[0], mx[1]);
      val[e] = u.val;
    }
    if (ok[k]) *(float4*)(p + e0 + 4 * k) = (float4){val[0], val[1], val[2], val[3]};
  }
  adam8_block_max<2>(mx, inv, red);
  if (thr == 0) *(float2*)(absmax + 2 * (int64_t)blockIdx.x) = make_float2(mx[0], mx[1]);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t w1[1], w2[1];
    adam8_requant<4>(tb, mn[k], vn[k], inv[0], inv[1], w1, w2);
    if (ok[k]) { *(uint32_t*)(m8 + e0 + 4 * k) = w1[0]; *(uint32_t*)(v8 + e0 + 4 * k) = w2[0]; }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void shadow_adamw8_kernel(const sdlt_shadow_desc* descs, const int32_t* block_desc, const int32_t* block_first, float* arena, const float* g,
                                                            uint8_t* m8, uint8_t* v8, float* absmax, const float* tables, const float* hyper) {
  __shared__ bf16_t tile[64][72];
  __shared__ float tb[1024];
  __shared__ float red[4][4];
  int r0, c0;
  const sdlt_shadow_desc d = tile_origin(descs, block_desc, block_first, r0, c0);
  const int thr = threadIdx.x;
  ((uint4*)tb)[thr] = ((const uint4*)tables)[thr];
  const bool full = r0 + 64 <= d.rows && c0 + 64 <= d.cols;
  if (full && ((d.offset | d.src_ld) & 3) == 0 && ((((uintptr_t)arena | (uintptr_t)g) & 15) | (((uintptr_t)m8 | (uintptr_t)v8) & 3)) == 0)
    adamw8_tile_vec(d, r0, c0, arena, g, m8, v8, absmax + 4 * (int64_t)blockIdx.x, hyper, tb, red, tile);
  else if (full) adamw8_tile<true>(d, r0, c0, arena, g, m8, v8, absmax + 4 * (int64_t)blockIdx.x, hyper, tb, red, tile);
  else adamw8_tile<false>(d, r0, c0, arena, g, m8, v8, absmax + 4 * (int64_t)blockIdx.x, hyper, tb, red, tile);
  tile_store(d, r0, c0, tile);
}

// ------------------------------------------------------------------ Prodigy
// Prodigy (prodigyopt 1.0, the reference's optional optimizer: trainer/optimizer.py:24-34 for the LoRA tensors,
// :135-145 for the token rows) as a device-resident step over a flat fp32 arena.
//
// The published algorithm makes two passes over the parameters with a global scalar update between them:
//   pass 1  exp_avg / exp_avg_sq / s moving averages (scaled by d), numerator += (d/d0) dlr <g, p0 - p>, denom = sum |s|
//   scalar  d_hat = d_coef numerator / denom ; d grows to at most d * growth_rate, never above the running max of d_hat
//   pass 2  p -= dlr (weight_decay p  +  exp_avg / (sqrt(exp_avg_sq) + d eps))      (decoupled decay)
// The reference implementation synchronises with the host twice per parameter tensor (.item()); here the two sums are
// fp64 device accumulators and the scalar update is a one-thread kernel, so the whole step stays inside the hipGraph.
// Both passes are HBM streams: pass 1 reads p,g,p0,m,v,s and writes m,v,s (9 words per element), pass 2 reads p,m,v and
// writes p (4 words).
enum { ST_D = 0, ST_D0, ST_DMAX, ST_NUM, ST_DENOM, ST_DHAT, ST_K, ST_DLR, ST_ACTIVE };
enum { HY_LR = 0, HY_B1, HY_B2, HY_B3, HY_EPS, HY_WD, HY_DCOEF, HY_GROWTH, HY_L1C, HY_GS, HY_BIASCORR, HY_SAFEGUARD, HY_DECOUPLE };

__global__ void prodigy_begin_kernel(const float* hyper, float* state, double* acc) {
  const float lr = hyper[HY_LR], b1 = hyper[HY_B1], b2 = hyper[HY_B2];
  const float k = state[ST_K];
  float bc = 1.f;
  if (hyper[HY_BIASCORR] != 0.f) bc = sqrtf(1.f - powf(b2, k + 1.f)) / (1.f - powf(b1, k + 1.f));
  state[ST_DLR] = state[ST_D] * lr * bc;
  acc[0] = 0.0;
  acc[1] = 0.0;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void prodigy_accum_kernel(const float* p, const float* g, const float* p0, float* m, float* v, float* s, int64_t n,
                                     const float* hyper, const float* state, double* acc, float* l1_partial) {
  const float lr = hyper[HY_LR], b1 = hyper[HY_B1], b2 = hyper[HY_B2], b3 = hyper[HY_B3], wd = hyper[HY_WD],
              l1c = hyper[HY_L1C], gs = hyper[HY_GS];
  const bool coupled = hyper[HY_DECOUPLE] == 0.f && wd != 0.f;
  const float d = state[ST_D], d0 = state[ST_D0], dlr = state[ST_DLR];
  const float sa = hyper[HY_SAFEGUARD] != 0.f ? (d / d0) * d : (d / d0) * dlr;
  float dot = 0.f, den = 0.f, l1 = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float pi = p[i];
    l1 += fabsf(pi);
    if (lr > 0.f) {
      float gi = g[i] * gs + l1c * (pi > 0.f ? 1.f : (pi < 0.f ? -1.f : 0.f));
      if (coupled) gi += wd * pi;
      dot += gi * (p0[i] - pi);
      m[i] = b1 * m[i] + d * (1.f - b1) * gi;
      v[i] = b2 * v[i] + d * d * (1.f - b2) * gi * gi;
      const float si = b3 * s[i] + sa * gi;
      s[i] = si;
      den += fabsf(si);
    }
  }
  // per-thread partial sums cover n / (grid * 256) elements in fp32; everything above that is accumulated in fp64
  // (one set of atomics per WORKGROUP: per wave they were up to 3 x 16384 serialised updates of three addresses - see adamw_kernel)
  __shared__ double accw[4][2];
  __shared__ float l1w[4];
  double dd = wave_sum_d((double)dot), de = wave_sum_d((double)den);
  l1 = wave_sum(l1);
  if ((threadIdx.x & 63) == 0) {
    accw[threadIdx.x >> 6][0] = dd;
    accw[threadIdx.x >> 6][1] = de;
    l1w[threadIdx.x >> 6] = l1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { a += accw[w][0]; b += accw[w][1]; t += l1w[w]; }
    atomicAdd(&acc[0], a);
    atomicAdd(&acc[1], b);
    if (l1_partial) atomicAdd(l1_partial, t);
  }
}

__global__ void prodigy_scalar_kernel(const float* hyper, float* state, const double* acc) {
  const float lr = hyper[HY_LR], b3 = hyper[HY_B3];
  float d = state[ST_D], d_max = state[ST_DMAX];
  const float d0 = state[ST_D0], dlr = state[ST_DLR];
  const double den = acc[1];
  if (den == 0.0) {  // no progress possible (lr == 0 or all-zero gradients): the reference returns before touching any state
    state[ST_ACTIVE] = 0.f;
    return;
  }
  const double num = (double)state[ST_NUM] * b3 + (double)(d / d0) * dlr * acc[0];
  float d_hat = d;
  if (lr > 0.f) {
    d_hat = (float)(hyper[HY_DCOEF] * num / den);
    if (d == d0) d = fmaxf(d, d_hat);
    d_max = fmaxf(d_max, d_hat);
    d = fminf(d_max, d * hyper[HY_GROWTH]);
  }
  state[ST_NUM] = (float)num;
  state[ST_DENOM] = (float)den;
  state[ST_D] = d;
  state[ST_DMAX] = d_max;
  state[ST_DHAT] = d_hat;
  state[ST_K] += 1.f;
  state[ST_ACTIVE] = 1.f;
}

__global__ void prodigy_apply_kernel(float* p, const float* m, const float* v, int64_t n, const float* hyper, const float* state) {
  if (state[ST_ACTIVE] == 0.f) return;
  const float dlr = state[ST_DLR], de = state[ST_D] * hyper[HY_EPS];
  const float decay = hyper[HY_DECOUPLE] != 0.f ? 1.f - hyper[HY_WD] * dlr : 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = p[i] * decay - dlr * m[i] / (sqrtf(v[i]) + de);
}

inline int grid_for(int64_t work_items, int block = 256) {
  int64_t g = (work_items + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

extern "C" int sdlt_adamw_fused(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, float* l1_sum,
                                void* stream) {
  if (n <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_adamw_fused: n=%lld", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (l1_sum) sdlt_zero_async(l1_sum, sizeof(float), s);
  const int vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n)), dim3(256), 0, s, p, g, m, v, n, hyper, l1_sum, vec);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
extern "C" int sdlt_lora_shadow_refresh(const sdlt_shadow_desc* descs_dev, const int32_t* block_desc_dev, const int32_t* block_first_dev,
                                        int32_t n_blocks, const float* arena, void* stream) {
  if (n_blocks <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_lora_shadow_refresh: n_blocks=%d", n_blocks);
  hipLaunchKernelGGL(shadow_kernel<false>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, block_desc_dev, block_first_dev,
                     const_cast<float*>(arena), (const float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
extern "C" int sdlt_adamw_shadow_refresh(const sdlt_shadow_desc* descs_dev, const int32_t* block_desc_dev, const int32_t* block_first_dev,
                                         int32_t n_blocks, float* p, const float* g, float* m, float* v, const float* hyper, void* stream) {
  if (n_blocks <= 0 || !p || !g || !m || !v || !hyper) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_adamw_shadow_refresh: n_blocks=%d or a null buffer", n_blocks);
  hipLaunchKernelGGL(shadow_kernel<true>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, block_desc_dev, block_first_dev, p, g, m, v, hyper);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
extern "C" int sdlt_adamw8_shadow_refresh(const sdlt_shadow_desc* descs_dev, const int32_t* block_desc_dev, const int32_t* block_first_dev, int32_t n_blocks, float* p,
                                          const float* g, uint8_t* m8, uint8_t* v8, float* absmax, const float* tables, const float* hyper, void* stream) {
  if (n_blocks <= 0 || !p || !g || !m8 || !v8 || !absmax || !tables || !hyper) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_adamw8_shadow_refresh: n_blocks=%d or a null buffer", n_blocks);
  if ((((uintptr_t)absmax | (uintptr_t)tables) & 15) != 0) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_adamw8_shadow_refresh: absmax / tables must be 16-byte aligned");
  hipLaunchKernelGGL(shadow_adamw8_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, block_desc_dev, block_first_dev, p, g, m8, v8, absmax, tables, hyper);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
extern "C" int sdlt_adamw8_flat(float* p, const float* g, uint8_t* m8, uint8_t* v8, float* absmax, int64_t n, const float* tables, const float* hyper, void* stream) {
  if (n <= 0 || (n & 3) || !p || !g || !m8 || !v8 || !absmax || !tables || !hyper) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_adamw8_flat: n=%lld (n %% 4 == 0) or a null buffer", (long long)n);
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)tables) & 15) || (((uintptr_t)m8 | (uintptr_t)v8) & 3) || ((uintptr_t)absmax & 7))
    SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_adamw8_flat: p / g / tables 16-byte, codes 4-byte, absmax 8-byte aligned");
  hipLaunchKernelGGL(adamw8_flat_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, p, g, m8, v8, absmax, n, tables, hyper);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
extern "C" int sdlt_prodigy_step(float* p, const float* g, const float* p0, float* m, float* v, float* s, int64_t n,
                                 const float* hyper, float* state, double* acc, float* l1_sum, void* stream) {
  if (n <= 0 || !p || !g || !p0 || !m || !v || !s || !hyper || !state || !acc)
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_prodigy_step: n=%lld or a null buffer", (long long)n);
  if ((uintptr_t)acc % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_prodigy_step: acc must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (l1_sum) sdlt_zero_async(l1_sum, sizeof(float), st);
  hipLaunchKernelGGL(prodigy_begin_kernel, dim3(1), dim3(1), 0, st, hyper, state, acc);
  hipLaunchKernelGGL(prodigy_accum_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, g, p0, m, v, s, n, hyper, state, acc, l1_sum);
  hipLaunchKernelGGL(prodigy_scalar_kernel, dim3(1), dim3(1), 0, st, hyper, state, acc);
  hipLaunchKernelGGL(prodigy_apply_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, m, v, n, hyper, state);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
