// Products with a weight difference (adapter extraction, the inverse of merge.hip): for every layer of a descriptor table, in ONE launch,
//   forward:     Y[N, L] = (W1 - W0) X[K, L]
//   transposed:  Y[K, L] = (W1 - W0)^T X[N, L]
// W0 / W1 [N, K] are the base and the tuned weight (bf16 / fp16 / fp32 each, 3x3 conv: the tap-major [Cout, 9 Cin] operand of merge.hip),
// X / Y fp32, L a multiple of 16 up to 272 (rank + oversampling of the randomized range finder).  The difference is formed in registers in
// fp32 after the two loads - exact for two bf16 / fp16 values, which it is not in bf16 - and goes to LDS only; the product runs on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain), so nothing is rounded below fp32.
// One workgroup = 64 output rows of one layer x ALL L columns, walking the whole reduction in chunks of 32: every weight element is read
// once per launch, no split of the reduction, no atomics - two runs give the same bits.  Per chunk the 64 x 32 differences and the 32 x L
// slab of X are staged in LDS; wave w owns output rows 16 w .. 16 w + 15 and L / 16 accumulators.  The MFMA is issued with X as its first
// operand, so a lane's four results are four consecutive columns of one output row: one 16-byte store.
// Forward launches can also leave the rows' sums of squares of the difference (||W1 - W0||_F^2 without a second pass) in rowsq[N].
#include "common.h"
#include "../../include/sdlt_kernels.h"

namespace {

constexpr int TM = 64, KC = 32, DLD = TM + 16;     // Ds[kk][m]: row stride 80 floats -> the 4 k-quarters of a fragment read hit 2 x 16 banks

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// 8 consecutive elements i0 .. i0 + 7 of a weight as fp32; `valid` of them exist (the others read as 0); vec: 16-byte loads are aligned
__device__ __forceinline__ void load8(const void* W, int dtype, size_t i0, int valid, bool vec, float (&v)[8]) {
  if (valid == 8 && vec) {
    if (dtype == 0) {
      const s16x8 x = *(const s16x8*)((const bf16_t*)W + i0);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = bf2f((bf16_t)x[e]);
    } else if (dtype == 1) {
      const f16x8 x = *(const f16x8*)((const _Float16*)W + i0);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
    } else {
      const f32x4 a = *(const f32x4*)((const float*)W + i0), b = *(const f32x4*)((const float*)W + i0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = a[e], v[4 + e] = b[e];
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float x = 0.f;
    if (e < valid) x = dtype == 0 ? bf2f(((const bf16_t*)W)[i0 + e]) : dtype == 1 ? (float)((const _Float16*)W)[i0 + e] : ((const float*)W)[i0 + e];
    v[e] = x;
  }
}

__device__ __forceinline__ bool vec_ok(const void* W, int64_t ld, int dtype) {
  const int es = dtype == 2 ? 4 : 2;
  return ((uintptr_t)W & 15) == 0 && ((ld * es) & 15) == 0;
}

template <int NBMAX>
__global__ __launch_bounds__(256) void delta_matmul_kernel(const sdlt_delta_desc* descs, const int32_t* block_desc, const int32_t* block_first, int L) {
  constexpr int XLD = NBMAX * 16 + (NBMAX % 2 ? 0 : 16);       // row stride of the X slab, = 16 mod 32 floats
  __shared__ __attribute__((aligned(16))) float Ds[KC * DLD];
  __shared__ __attribute__((aligned(16))) float Xs[KC * XLD];
  const int di = block_desc[blockIdx.x];
  const sdlt_delta_desc d = descs[di];
  const int m0 = (blockIdx.x - block_first[di]) * TM;
  const bool tr = d.transposed != 0;
  const int Md = tr ? d.K : d.N, Rd = tr ? d.N : d.K;          // output rows, reduction length
  const int nb = L >> 4, nq = L >> 2;                          // 16-column blocks, float4 per X row
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const bool v0 = vec_ok(d.W0, d.ldw0, d.dtype0), v1 = vec_ok(d.W1, d.ldw1, d.dtype1);
  f32x4 acc[NBMAX];
#pragma unroll
  for (int j = 0; j < NBMAX; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  for (int r0 = 0; r0 < Rd; r0 += KC) {
    {   // the chunk's differences -> Ds[reduction index][output row]
      float a[8], b[8];
      int n, k;
      if (!tr) n = m0 + (tid >> 2), k = r0 + (tid & 3) * 8;    // thread: one weight row, 8 columns of the chunk
      else n = r0 + (tid >> 3), k = m0 + (tid & 7) * 8;        // thread: one weight row of the chunk, 8 of the tile's 64 columns
      const int valid = n < d.N ? min(max(d.K - k, 0), 8) : 0;
      load8(d.W0, d.dtype0, (size_t)n * d.ldw0 + k, valid, v0, a);
      load8(d.W1, d.dtype1, (size_t)n * d.ldw1 + k, valid, v1, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = b[e] - a[e];
        ss = fmaf(a[e], a[e], ss);
      }
      if (!tr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) Ds[((tid & 3) * 8 + e) * DLD + (tid >> 2)] = a[e];
      } else {
        float* p = &Ds[(tid >> 3) * DLD + (tid & 7) * 8];
        *(f32x4*)p = f32x4{a[0], a[1], a[2], a[3]};
        *(f32x4*)(p + 4) = f32x4{a[4], a[5], a[6], a[7]};
      }
    }
    for (int i = tid; i < KC * nq; i += 256) {   // X[r0 .. r0 + 31][0 .. L): rows past the reduction length are zero
      const int kk = i / nq, c = (i - kk * nq) * 4;
      const int r = r0 + kk;
      *(f32x4*)&Xs[kk * XLD + c] = r < Rd ? *(const f32x4*)(d.X + (size_t)r * d.ldx + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const int kk = 4 * s + lq;
      const float dv = Ds[kk * DLD + 16 * w + l15];
#pragma unroll
      for (int j = 0; j < NBMAX; ++j)
        if (j < nb) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Xs[kk * XLD + 16 * j + l15], dv, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  // lane: output row m0 + 16 w + (lane & 15), columns 16 j + 4 (lane >> 4) .. + 3
  const int m = m0 + 16 * w + l15;
  if (m < Md) {
#pragma unroll
    for (int j = 0; j < NBMAX; ++j)
      if (j < nb) *(f32x4*)(d.Y + (size_t)m * d.ldy + 16 * j + 4 * lq) = acc[j];
  }
  if (!tr && d.rowsq) {   // the 4 threads of a weight row hold its sum of squares in four parts: added in lane order
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    const int n = m0 + (tid >> 2);
    if ((tid & 3) == 0 && n < d.N) d.rowsq[n] = ss;
  }
}

}  // namespace

extern "C" int sdlt_delta_matmul(const sdlt_delta_desc* descs_dev, const int32_t* block_desc_dev, const int32_t* block_first_dev, int32_t n_blocks,
                                 int32_t L, void* stream) {
  if (n_blocks <= 0) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_delta_matmul: n_blocks=%d", n_blocks);
  if (L < 16 || L > 272 || L % 16) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_delta_matmul: L=%d (a multiple of 16, 16..272)", L);
  const dim3 g(n_blocks), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (L <= 32) hipLaunchKernelGGL(delta_matmul_kernel<2>, g, b, 0, s, descs_dev, block_desc_dev, block_first_dev, L);
  else if (L <= 80) hipLaunchKernelGGL(delta_matmul_kernel<5>, g, b, 0, s, descs_dev, block_desc_dev, block_first_dev, L);
  else if (L <= 144) hipLaunchKernelGGL(delta_matmul_kernel<9>, g, b, 0, s, descs_dev, block_desc_dev, block_first_dev, L);
  else hipLaunchKernelGGL(delta_matmul_kernel<17>, g, b, 0, s, descs_dev, block_desc_dev, block_first_dev, L);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
