// The guidance pre-pass of the latent sampler: one launch between the UNet forward and whichever step launch follows (sampler.hip: any of its
// four entry points).  It rewrites eps (fp32 [2n hw, 4]; image j = rows 2j negative, 2j + 1 positive) in place so that BOTH row blocks
// of image j hold the final prediction e; the step launch then forms e + g (e - e) = e whatever its own table holds, and needs no change.
//   row i = ctr[0] of gtab (fp32 [1 + k, 4]: row 0 = (k, 0, 0, 0), row 1 + i = (g_i, phi_i, 0, 0)); ctr is read, never written
//   g_i == 1 and phi_i == 0:   e = e_pos                                   guidance off (outside the guidance interval)
//   otherwise                  e_c = e_neg + g_i (e_pos - e_neg)
//   phi_i == 0:                e = e_c                                     a per-step guidance scale; no reduction is run
//   otherwise                  s_pos, s_c = unbiased standard deviations (divisor 4 hw - 1) of e_pos, e_c over the image's 4 hw values
//                              r = s_pos / s_c   (s_c == 0: r = 1)
//                              e = phi_i (e_c r) + (1 - phi_i) e_c         rescale_noise_cfg (Lin et al. 2024, section 3.4) as published
// Both conditions come from the table row: uniform over the launch.  ONE workgroup of 1024 threads per image, so the statistics need no hand-off between
// workgroups and image j's result depends on neither n nor j.  Thread t owns pixels t, t + 1024, ... (one 16-byte load per row) in every pass; the
// deviations are taken about the mean (pass 1: the two sums; pass 2: the two sums of squared deviations; pass 3: the write), because the one-pass
// sum x^2 - (sum x)^2 / N loses everything in fp32 when the mean is far from zero.  The order of every sum is fixed - a thread's pixels in
// ascending order, the xor butterfly of the wave, the sixteen wave totals in ascending order - so the bits repeat from run to run.  The image is read
// three times, from the L2 the forward's last product left it in.  fp32, one rounding per operation (no contraction), IEEE division and square root,
// vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int GT = 1024;            // threads of the workgroup = the pixel stride of a thread
constexpr int GW = GT / 64;         // waves
constexpr int GU = 4;               // pixels of a thread in flight per trip of a reduction pass

// The workgroup's totals of a and b, the same bits in every thread.  `red` is reused by the next call: the leading barrier orders that.
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[GW]) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = red[0][0];
  b = red[1][0];
#pragma unroll
  for (int w = 1; w < GW; ++w) {
    a = a + red[0][w];
    b = b + red[1][w];
  }
}

__global__ __launch_bounds__(GT) void guidance_kernel(sdlt_guidance_params p) {
  __shared__ float red[2][GW];
  const float* tab = p.gtab;
  int k = (int)tab[0];
  k = max(1, min(k, p.gtab_rows - 1));
  const int i = max(0, min(p.ctr[0], k - 1));
  const float g = tab[4 * (1 + i)], phi = tab[4 * (1 + i) + 1];
  const int hw = p.hw;
  float* en_p = p.eps + (size_t)(2 * blockIdx.x) * hw * 4;
  float* ep_p = en_p + (size_t)hw * 4;
  const int t = threadIdx.x;
  if (phi == 0.f) {                                       // uniform
    const bool off = g == 1.f;                            // uniform
    for (int px = t; px < hw; px += GT) {
      const f32x4 en = *(const f32x4*)(en_p + (size_t)px * 4);
      const f32x4 ep = *(const f32x4*)(ep_p + (size_t)px * 4);
      f32x4 e;
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c] = off ? ep[c] : en[c] + g * (ep[c] - en[c]);
      *(f32x4*)(en_p + (size_t)px * 4) = e;
      *(f32x4*)(ep_p + (size_t)px * 4) = e;
    }
    return;
  }
  const float N = (float)(4 * (int64_t)hw);
  // In the three passes a thread takes GU of its pixels per trip, all loads requested before the first use.  A pixel past the end is loaded from the
  // trip's first pixel instead (always inside the image: no load under a per-thread condition) and counts as zero / is not stored.
  // ---- pass 1: the means of e_pos and e_c
  float sp = 0.f, sc = 0.f;
  for (int base = t; base < hw; base += GU * GT) {
    f32x4 en[GU], ep[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int px = base + u * GT < hw ? base + u * GT : base;
      en[u] = *(const f32x4*)(en_p + (size_t)px * 4);
      ep[u] = *(const f32x4*)(ep_p + (size_t)px * 4);
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      float ec[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) ec[c] = en[u][c] + g * (ep[u][c] - en[u][c]);
      const bool in = base + u * GT < hw;
      sp = sp + (in ? (ep[u][0] + ep[u][1]) + (ep[u][2] + ep[u][3]) : 0.f);
      sc = sc + (in ? (ec[0] + ec[1]) + (ec[2] + ec[3]) : 0.f);
    }
  }
  block_sum2(sp, sc, red);
  const float mp = sp / N, mc = sc / N;
  // ---- pass 2: the sums of squared deviations about them
  float qp = 0.f, qc = 0.f;
  for (int base = t; base < hw; base += GU * GT) {
    f32x4 en[GU], ep[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int px = base + u * GT < hw ? base + u * GT : base;
      en[u] = *(const f32x4*)(en_p + (size_t)px * 4);
      ep[u] = *(const f32x4*)(ep_p + (size_t)px * 4);
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      float dp[4], dc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float ec = en[u][c] + g * (ep[u][c] - en[u][c]);
        dp[c] = ep[u][c] - mp;
        dc[c] = ec - mc;
        dp[c] = dp[c] * dp[c];
        dc[c] = dc[c] * dc[c];
      }
      const bool in = base + u * GT < hw;
      qp = qp + (in ? (dp[0] + dp[1]) + (dp[2] + dp[3]) : 0.f);
      qc = qc + (in ? (dc[0] + dc[1]) + (dc[2] + dc[3]) : 0.f);
    }
  }
  block_sum2(qp, qc, red);
  const float s_pos = sqrtf(qp / (N - 1.f)), s_c = sqrtf(qc / (N - 1.f));
  const float r = s_c == 0.f ? 1.f : s_pos / s_c;
  const float om = 1.f - phi;
  // ---- pass 3: e into both row blocks.  Every read of passes 1 and 2 lies before the barriers of block_sum2; a thread rewrites its own pixels only,
  // and a trip's loads (the stand-in of a pixel past the end included) come before its stores.
  for (int base = t; base < hw; base += GU * GT) {
    f32x4 en[GU], ep[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int px = base + u * GT < hw ? base + u * GT : base;
      en[u] = *(const f32x4*)(en_p + (size_t)px * 4);
      ep[u] = *(const f32x4*)(ep_p + (size_t)px * 4);
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      f32x4 e;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float ec = en[u][c] + g * (ep[u][c] - en[u][c]);
        e[c] = phi * (ec * r) + om * ec;
      }
      if (base + u * GT < hw) {
        *(f32x4*)(en_p + (size_t)(base + u * GT) * 4) = e;
        *(f32x4*)(ep_p + (size_t)(base + u * GT) * 4) = e;
      }
    }
  }
}

}  // namespace

extern "C" int sdlt_guidance(const sdlt_guidance_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance: n=%d hw=%d", p->n, p->hw);
  if (p->gtab_rows < 2) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance: gtab_rows=%d (the header row + at least one step)", p->gtab_rows);
  if (!p->eps || !p->gtab || !p->ctr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance: null pointer");
  if ((uintptr_t)p->eps & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance: eps must be 16-byte aligned");
  if (((uintptr_t)p->gtab | (uintptr_t)p->ctr) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance: gtab and ctr must be 4-byte aligned");
  hipLaunchKernelGGL(guidance_kernel, dim3(p->n), dim3(GT), 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

// ---- adaptive projected guidance ----------------------------------------------------------------------------------------------------------
// sdlt_guidance_apg: the pre-pass with the guidance update projected on the positive prediction (Sadat et al. 2024; diffusers' normalized_guidance
// with its MomentumBuffer), in sdlt_guidance's place and shape: ONE workgroup of 1024 threads per image, thread t owns pixels t, t + 1024, ..., every sum
// in the fixed order of block_sum (a thread's pixels ascending, a pixel's four products as (0 + 1) + (2 + 3), the xor butterfly, the sixteen wave
// totals ascending).  Row i = ctr[0] of gtab gives (g, phi), of atab (eta, tau, beta); mo = beta != 0 and mom is given.  Per image, fp32, one rounding
// per operation, in the order written:
//   g == 1:      e = e_pos (copied); mom is neither read nor written
//   pass 1       d = e_pos - e_neg ;  mo: m = d + beta m_prev (m_prev = +0 at i == 0: the buffer is not read), m -> mom, d = m
//                S_dd = sum d d ;  S_dp = sum d e_pos ;  S_pp = sum e_pos e_pos          ONE pass for the three sums, of the UNCLIPPED d
//   scalars      c = tau > 0 and S_dd != 0 ? min(1, tau / sqrt(S_dd)) : 1 ;  a = S_pp == 0 ? 0 : (c S_dp) / S_pp
//   per value    d = c d ;  par = a e_pos ;  orth = d - par ;  e_c = e_pos + (g - 1) (orth + eta par)      (d: mom's m where mo, else e_pos - e_neg again)
//   phi == 0:    e = e_c (pass 2 writes it)
//   otherwise    sdlt_guidance's rescale on e_c: the means (pass 2), the squared deviations about them (pass 3), r = s_pos / s_c (s_c == 0: r = 1),
//                e = phi (e_c r) + (1 - phi) e_c (pass 4 writes it)
// A thread reads m back from the addresses it stored itself.  Every store is a 16-byte vector store of the thread's own pixel; every offset is 64-bit.
namespace {

__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*red)[GW]) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
    red[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  a = red[0][0];
  b = red[1][0];
  c = red[2][0];
#pragma unroll
  for (int w = 1; w < GW; ++w) {
    a = a + red[0][w];
    b = b + red[1][w];
    c = c + red[2][w];
  }
}

// One pass over the image: a thread takes GU of its pixels per trip, all loads requested before the first use; a pixel past the end is loaded from the
// trip's first pixel instead (the thread's own, always inside the image) and reaches f with in = false.  m_p null: nothing is read there, mm = 0.
template <class F>
__device__ __forceinline__ void apg_pass(const float* en_p, const float* ep_p, const float* m_p, int hw, F&& f) {
  const int t = threadIdx.x;
  for (int base = t; base < hw; base += GU * GT) {
    f32x4 en[GU], ep[GU], mm[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int px = base + u * GT < hw ? base + u * GT : base;
      en[u] = *(const f32x4*)(en_p + (size_t)px * 4);
      ep[u] = *(const f32x4*)(ep_p + (size_t)px * 4);
      mm[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m_p != nullptr) mm[u] = *(const f32x4*)(m_p + (size_t)px * 4);      // uniform
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) f(base + u * GT, base + u * GT < hw, en[u], ep[u], mm[u]);
  }
}

struct ApgScalars { float c, a, eta, gm1; };

__device__ __forceinline__ float apg_ec(float d, float ep, const ApgScalars& s) {
  d = s.c * d;
  const float par = s.a * ep;
  const float orth = d - par;
  return ep + s.gm1 * (orth + s.eta * par);
}

__global__ __launch_bounds__(GT) void guidance_apg_kernel(sdlt_guidance_apg_params p) {
  __shared__ float red[3][GW];
  const float* tab = p.gtab;
  int k = (int)tab[0];
  k = max(1, min(k, p.gtab_rows - 1));
  const int i = max(0, min(p.ctr[0], k - 1));
  const float g = tab[4 * (1 + i)], phi = tab[4 * (1 + i) + 1];
  const float eta = p.atab[4 * (1 + i)], tau = p.atab[4 * (1 + i) + 1], beta = p.atab[4 * (1 + i) + 2];
  const int hw = p.hw;
  float* en_p = p.eps + (size_t)(2 * blockIdx.x) * hw * 4;
  float* ep_p = en_p + (size_t)hw * 4;
  const auto write = [&](int px, const f32x4& e) {
    *(f32x4*)(en_p + (size_t)px * 4) = e;
    *(f32x4*)(ep_p + (size_t)px * 4) = e;
  };
  if (g == 1.f) {                                         // uniform: guidance off
    apg_pass(en_p, ep_p, nullptr, hw, [&](int px, bool in, const f32x4&, const f32x4& ep, const f32x4&) {
      if (in) write(px, ep);
    });
    return;
  }
  const bool mo = beta != 0.f && p.mom != nullptr;        // uniform
  float* m_p = mo ? p.mom + (size_t)blockIdx.x * hw * 4 : nullptr;
  // ---- pass 1: the running average and the three sums
  float sdd = 0.f, sdp = 0.f, spp = 0.f;
  apg_pass(en_p, ep_p, mo && i > 0 ? m_p : nullptr, hw, [&](int px, bool in, const f32x4& en, const f32x4& ep, const f32x4& mprev) {
    f32x4 d;
    float dd[4], dp[4], pp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[c] = ep[c] - en[c];
      if (mo) d[c] = d[c] + beta * mprev[c];
      dd[c] = d[c] * d[c];
      dp[c] = d[c] * ep[c];
      pp[c] = ep[c] * ep[c];
    }
    if (mo && in) *(f32x4*)(m_p + (size_t)px * 4) = d;
    sdd = sdd + (in ? (dd[0] + dd[1]) + (dd[2] + dd[3]) : 0.f);
    sdp = sdp + (in ? (dp[0] + dp[1]) + (dp[2] + dp[3]) : 0.f);
    spp = spp + (in ? (pp[0] + pp[1]) + (pp[2] + pp[3]) : 0.f);
  });
  block_sum3(sdd, sdp, spp, red);
  ApgScalars s;
  s.c = tau > 0.f && sdd != 0.f ? fminf(1.f, tau / sqrtf(sdd)) : 1.f;
  s.a = spp == 0.f ? 0.f : (s.c * sdp) / spp;
  s.eta = eta;
  s.gm1 = g - 1.f;
  const auto ec4 = [&](const f32x4& en, const f32x4& ep, const f32x4& m) {
    f32x4 ec;
#pragma unroll
    for (int c = 0; c < 4; ++c) ec[c] = apg_ec(mo ? m[c] : ep[c] - en[c], ep[c], s);
    return ec;
  };
  if (phi == 0.f) {                                       // uniform
    // ---- pass 2: e_c into both row blocks.  Every read of pass 1 lies before the barriers of block_sum3; a thread rewrites its own pixels only.
    apg_pass(en_p, ep_p, m_p, hw, [&](int px, bool in, const f32x4& en, const f32x4& ep, const f32x4& m) {
      const f32x4 ec = ec4(en, ep, m);
      if (in) write(px, ec);
    });
    return;
  }
  const float N = (float)(4 * (int64_t)hw);
  // ---- pass 2: the means of e_pos and e_c
  float sp = 0.f, sc = 0.f, zero = 0.f;
  apg_pass(en_p, ep_p, m_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep, const f32x4& m) {
    const f32x4 ec = ec4(en, ep, m);
    sp = sp + (in ? (ep[0] + ep[1]) + (ep[2] + ep[3]) : 0.f);
    sc = sc + (in ? (ec[0] + ec[1]) + (ec[2] + ec[3]) : 0.f);
  });
  block_sum3(sp, sc, zero, red);
  const float mp = sp / N, mc = sc / N;
  // ---- pass 3: the sums of squared deviations about them
  float qp = 0.f, qc = 0.f;
  apg_pass(en_p, ep_p, m_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep, const f32x4& m) {
    const f32x4 ec = ec4(en, ep, m);
    float dp[4], dc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      dp[c] = ep[c] - mp;
      dc[c] = ec[c] - mc;
      dp[c] = dp[c] * dp[c];
      dc[c] = dc[c] * dc[c];
    }
    qp = qp + (in ? (dp[0] + dp[1]) + (dp[2] + dp[3]) : 0.f);
    qc = qc + (in ? (dc[0] + dc[1]) + (dc[2] + dc[3]) : 0.f);
  });
  block_sum3(qp, qc, zero, red);
  const float s_pos = sqrtf(qp / (N - 1.f)), s_c = sqrtf(qc / (N - 1.f));
  const float r = s_c == 0.f ? 1.f : s_pos / s_c;
  const float om = 1.f - phi;
  // ---- pass 4: e into both row blocks
  apg_pass(en_p, ep_p, m_p, hw, [&](int px, bool in, const f32x4& en, const f32x4& ep, const f32x4& m) {
    const f32x4 ec = ec4(en, ep, m);
    f32x4 e;
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = phi * (ec[c] * r) + om * ec[c];
    if (in) write(px, e);
  });
}

}  // namespace

extern "C" int sdlt_guidance_apg(const sdlt_guidance_apg_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_apg: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28)) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_apg: n=%d hw=%d", p->n, p->hw);
  if (p->gtab_rows < 2) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_apg: gtab_rows=%d (the header row + at least one step)", p->gtab_rows);
  if (!p->eps || !p->gtab || !p->atab || !p->ctr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_apg: null pointer");
  if (((uintptr_t)p->eps | (uintptr_t)p->mom) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance_apg: eps and mom must be 16-byte aligned");
  if (((uintptr_t)p->gtab | (uintptr_t)p->atab | (uintptr_t)p->ctr) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance_apg: gtab, atab and ctr must be 4-byte aligned");
  if (p->mom != nullptr) {
    const uintptr_t e0 = (uintptr_t)p->eps, m0 = (uintptr_t)p->mom, img = (uintptr_t)p->n * (uintptr_t)p->hw * 16;
    if (m0 < e0 + 2 * img && e0 < m0 + img) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_apg: mom overlaps eps");
  }
  hipLaunchKernelGGL(guidance_apg_kernel, dim3(p->n), dim3(GT), 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
