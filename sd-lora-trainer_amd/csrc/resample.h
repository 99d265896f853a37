// The per-axis index / weight arithmetic and the tap sums of sdlt_resize_planes (include/sdlt_kernels.h writes the order down), shared by resize.hip
// and heatmap.hip.  Everything here is fp32 with one rounding per operation: a file that includes this header turns contraction off first.
#pragma once
#include "common.h"

namespace resample {

template <int TAPS>
struct Axis {
  int idx[TAPS];
  float wt[TAPS];
};

// The Keys kernel, A = -0.75, at the fraction t (u = 1 - t), in the order of the header.  The two pieces are evaluated in their factored forms -
// outer A (x - 1)(x - 2)^2 = A t u^2 at x = t + 1, inner (1 - x)(1 + x - 1.25 x^2) - which have no cancellation: the expanded polynomials lose
// ~1e-6 of a weight near x = 2 (terms of size 6 summing to 0.07).  The weight of tap i itself is never formed: the sum is taken about that tap.
__device__ __forceinline__ float keys_outer(float t, float u) {      // the tap at distance t + 1: A t u u
  float m = -0.75f * t;
  m = m * u;
  return m * u;
}
__device__ __forceinline__ float keys_inner(float t, float u) {      // the tap at distance u = 1 - t: t (1 + u (1 - 1.25 u))
  float m = 1.25f * u;
  m = 1.0f - m;
  m = m * u;
  m = m + 1.0f;
  return m * t;
}

__device__ __forceinline__ void axis_nearest(int d, int in, int out, Axis<1>& a) {
  const uint32_t q = ((uint32_t)(2 * d + 1) * (uint32_t)in) / (uint32_t)(2 * out);
  a.idx[0] = min((int)q, in - 1);
  a.wt[0] = 1.0f;
}
__device__ __forceinline__ void axis_linear(int d, int in, int out, Axis<2>& a) {
  const float s = (float)in / (float)out;
  float c = (float)d + 0.5f;
  c = c * s;
  c = c - 0.5f;
  c = fmaxf(c, 0.0f);
  const int i0 = min((int)c, in - 1);          // c >= 0: truncation is floor; c < in - 0.5 for every d < out (the min never binds)
  const float t = c - (float)i0;
  a.idx[0] = i0;
  a.idx[1] = min(i0 + 1, in - 1);
  a.wt[0] = 1.0f - t;
  a.wt[1] = t;
}
__device__ __forceinline__ void axis_cubic(int d, int in, int out, Axis<4>& a) {
  const float s = (float)in / (float)out;
  float c = (float)d + 0.5f;
  c = c * s;
  c = c - 0.5f;
  const float fl = floorf(c);
  const int i = (int)fl;                       // -1 .. in - 1
  const float t = c - fl;
  const float u = 1.0f - t;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.idx[k] = max(0, min(i - 1 + k, in - 1));
  a.wt[0] = keys_outer(t, u);
  a.wt[1] = 1.0f;                              // (not read: tap i enters the sum as itself)
  a.wt[2] = keys_inner(t, u);
  a.wt[3] = keys_outer(u, t);
}

template <int TAPS>
__device__ __forceinline__ void axis(int d, int in, int out, Axis<TAPS>& a) {
  if constexpr (TAPS == 1) axis_nearest(d, in, out, a);
  else if constexpr (TAPS == 2) axis_linear(d, in, out, a);
  else axis_cubic(d, in, out, a);
}

// One axis' sum of the header.  Bilinear: w_0 a_0 + w_1 a_1 (a_2, a_3 repeat a_0, a_1 and are not read).  Bicubic: about tap 1, the differences first -
// a_1 + w_0 (a_0 - a_1) + w_2 (a_2 - a_1) + w_3 (a_3 - a_1), left to right - so that a constant image comes out as the constant exactly.
template <int TAPS>
__device__ __forceinline__ float combine(float a0, float a1, float a2, float a3, const float* w) {
  if constexpr (TAPS == 2) {
    return w[0] * a0 + w[1] * a1;
  } else {
    float v = a1 + w[0] * (a0 - a1);
    v = v + w[2] * (a2 - a1);
    return v + w[3] * (a3 - a1);
  }
}

}  // namespace resample
