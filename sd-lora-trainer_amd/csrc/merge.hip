// Adapter merge (export): the trained adapters baked into the base weights, the `fuse_lora()` of the reference's inference script
// (scripts/test_inference.py:53) and kohya's merge_lora, for every adapted layer of an arena in ONE batched launch (DoRA: two).
//   LoRA:  W' = W + s B A
//   DoRA:  W' = (m_n / ||W_n + s B_n A||) (W_n + s B_n A)          (peft _apply_dora / merge, per output row n)
// A [rank, K] and B [N, rank] are the arena's fp32 masters; every product accumulates in fp32 and the output (bf16 / fp16 / fp32) is
// rounded once.  One workgroup = one 64 x 64 tile of one layer's [N, K] weight (3x3 conv: the tap-major [Cout, 9 Cin] operand): the
// rank walk is a small fp32 GEMM out of LDS (16 ranks per stage, a 4 x 4 register tile per thread), W is read and W' written once.
// DoRA: phase 1 leaves every tile's row sums of squares of the fp32 merged values in ws[n * tiles_k + tile]; phase 2 recomputes the
// tile, adds those partials in tile order (bitwise reproducible, no atomics) and writes factor * value.
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr int TM = 64, TK = 64, RC = 16;

__device__ __forceinline__ float load_w(const void* W, int dtype, size_t i) {
  if (dtype == 0) return bf2f(((const bf16_t*)W)[i]);
  if (dtype == 1) return (float)((const _Float16*)W)[i];
  return ((const float*)W)[i];
}

__device__ __forceinline__ void store_o(void* O, int dtype, size_t i, float v) {
  if (dtype == 0) ((bf16_t*)O)[i] = f2bf(v);
  else if (dtype == 1) ((_Float16*)O)[i] = (_Float16)v;        // round to nearest even
  else ((float*)O)[i] = v;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const sdlt_merge_desc* descs, const int32_t* block_desc, const int32_t* block_first,
                                                         int out_dtype, int phase) {
  const int di = block_desc[blockIdx.x];
  const sdlt_merge_desc d = descs[di];
  const int tiles_k = (d.K + TK - 1) / TK;
  const int t = blockIdx.x - block_first[di];
  const int tn = t / tiles_k, tk = t - tn * tiles_k;
  const int n0 = tn * TM, k0 = tk * TK;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;      // thread: rows n0 + 4 ty .. +3, columns k0 + 4 tx .. +3
  __shared__ float As[RC][TK];
  __shared__ float Bs[RC][TM + 4];
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int r0 = 0; r0 < d.rank; r0 += RC) {
    {   // A[r0 .. r0 + 15][k0 .. k0 + 63]: thread -> rank row tid / 16, 4 columns
      const int rr = tid >> 4, c = (tid & 15) * 4, r = r0 + rr;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + c + e;
        As[rr][c + e] = (r < d.rank && k < d.K) ? d.A[(size_t)r * d.lda + k] : 0.f;
      }
    }
    {   // B[n0 .. n0 + 63][r0 .. r0 + 15], stored rank-major: thread -> row tid / 4, 4 ranks
      const int row = tid >> 2, rc = (tid & 3) * 4, n = n0 + row;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = r0 + rc + e;
        Bs[rc + e][row] = (r < d.rank && n < d.N) ? d.B[(size_t)n * d.ldb + r] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RC; ++rr) {
      const f32x4 a = *(const f32x4*)&As[rr][tx * 4];
      const f32x4 b = *(const f32x4*)&Bs[rr][ty * 4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(b[i], a[j], acc[i][j]);     // ranks in order: fp32 sum of r products
    }
    __syncthreads();
  }
  // merged fp32 values v = W + s (B A)
  float v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty * 4 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + tx * 4 + j;
      const float w = (n < d.N && k < d.K) ? load_w(d.W, d.w_dtype, (size_t)n * d.ldw + k) : 0.f;
      v[i][j] = fmaf(d.s, acc[i][j], w);
    }
  }
  if (phase == 1) {   // DoRA: this tile's row sums of squares (valid columns only) -> ws
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) ss = (k0 + tx * 4 + j < d.K) ? fmaf(v[i][j], v[i][j], ss) : ss;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);      // the 16 threads of one row group (lanes 16 g .. 16 g + 15)
      const int n = n0 + ty * 4 + i;
      if (tx == 0 && n < d.N) d.ws[(size_t)n * tiles_k + tk] = ss;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty * 4 + i;
    if (n >= d.N) break;
    float c = 1.f;
    if (phase == 2) {
      float ss = 0.f;
      for (int q = 0; q < tiles_k; ++q) ss += d.ws[(size_t)n * tiles_k + q];
      c = d.mag[n] / sqrtf(fmaxf(ss, 1e-30f));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + tx * 4 + j;
      if (k < d.K) store_o(d.out, out_dtype, (size_t)n * d.ldo + k, phase == 2 ? c * v[i][j] : v[i][j]);
    }
  }
}

}  // namespace

extern "C" int sdlt_lora_merge(const sdlt_merge_desc* descs_dev, const int32_t* block_desc_dev, const int32_t* block_first_dev, int32_t n_blocks,
                               int32_t out_dtype, int32_t phase, void* stream) {
  if (n_blocks <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_lora_merge: n_blocks=%d", n_blocks);
  if (out_dtype < 0 || out_dtype > 2) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_lora_merge: out_dtype %d (0 bf16, 1 fp16, 2 fp32)", out_dtype);
  if (phase < 0 || phase > 2) SDLT_FAIL(SDLT_ERR_UNSUPPORTED, "sdlt_lora_merge: phase %d (0 LoRA, 1 / 2 DoRA)", phase);
  hipLaunchKernelGGL(lora_merge_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, block_desc_dev, block_first_dev, out_dtype, phase);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
