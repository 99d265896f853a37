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

// ---- dynamic thresholding -------------------------------------------------------------------------------------------------------------------
// sdlt_guidance_dyn: the pre-pass that gives every latent channel of the guided prediction the value range it would have had at a mild mimic scale (the
// "Dynamic Thresholding (CFG scale fix)" extension of the common front ends, a latent form of Imagen's dynamic thresholding), in sdlt_guidance's place
// and shape: ONE workgroup of 1024 threads per image, thread t owns pixels t, t + 1024, ..., 16-byte loads, 64-bit offsets, e_g and e_m formed again from
// e_neg and e_pos in every pass, no workspace.  Row i = ctr[0] of gtab gives g, of dtab (mimic, q, psi).  Per image and channel c, fp32, one rounding per
// operation, in the order written:
//   g == 1:      e = e_pos (copied)
//   pass 1       d = e_pos - e_neg ;  e_g = e_neg + g d ;  e_m = e_neg + mimic d ;  the eight sums (e_g and e_m, per channel) in block_sum's fixed order
//                mu_g[c] = sum / hw ;  mu_m[c] = sum / hw
//   pass 2       c_g = e_g - mu_g[c] ;  c_m = e_m - mu_m[c] ;  A[c] = max |c_m| as the integer maximum of the bit patterns (order-free)
//                and the histogram of the top 11 bits of key = bits(|c_g|) - monotone for non-negative floats, -0 maps to 0
//   passes 3, 4  the histograms of the next 10 and the last 10 bits of the keys that match the digits found so far: a most-significant-digit radix
//                select of rank lo = min((int)floorf(q (hw - 1)), hw - 1), EXACT: v_lo is the lo-th smallest key, ties included
//   pass 5       only where rank hi = min(lo + 1, hw - 1) is not among the keys equal to v_lo in some channel: v_hi = the integer minimum of the keys > v_lo
//   scalars      Q = v_lo + w (v_hi - v_lo), w = q (hw - 1) - lo ;  S = max(A, Q)
//   last pass    S == 0: e_d = e_g ;  otherwise e_d = ((min(max(c_g, -S), S) / S) A) + mu_g[c] ;  psi == 1: e = e_d, otherwise e = psi e_d + (1 - psi) e_g
// Histograms are integer LDS atomics (they commute: the bits repeat), 4 channels x 2048 bins = 32 KB; a bin index is a masked digit, always inside its row.
// After each histogram 256 threads per channel scan their 8 (4) bins, and the one thread whose range holds the rank publishes (bin, rank inside it,
// count).  Nothing passes between threads but through LDS; no float atomics; vector stores of the thread's own pixels only.
namespace {

static_assert(GT == 1024, "dyn_pick gives each of the 4 channels 256 threads");
constexpr int DYN_BINS = 2048;      // bins of the widest digit (11 bits); the two 10-bit digits use the first 1024

struct DynShared {
  unsigned hist[4][DYN_BINS];
  float red[8][GW], tot[8];
  unsigned wtot[GW];
  unsigned rank[4], bin[4], cnt[4];  // per channel: the rank among the keys still matching, the digit found, the keys in that bin
  unsigned amax[4], vmin[4];
};

__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

// The workgroup's totals of v[0..7] in block_sum2's order, the same bits in every thread.
__device__ __forceinline__ void block_sum8(float (&v)[8], float (*red)[GW], float* tot) {
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s] = wave_sum(v[s]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) red[s][threadIdx.x >> 6] = v[s];
  }
  __syncthreads();
  if (threadIdx.x < 8) {                                              // thread s adds sum s's sixteen wave totals, ascending: 128 words are not read by all
    float a = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < GW; ++w) a = a + red[threadIdx.x][w];
    tot[threadIdx.x] = a;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s] = tot[s];
}

// One pass over the image, as apg_pass: GU of the thread's pixels per trip, all loads first; a pixel past the end is loaded from the trip's first pixel
// (the thread's own, inside the image) and reaches f with in = false.
template <class F>
__device__ __forceinline__ void dyn_pass(const float* en_p, const float* ep_p, int hw, F&& f) {
  const int t = threadIdx.x;
  for (int base = t; base < hw; base += GU * GT) {
    f32x4 en[GU], ep[GU];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const int px = base + u * GT < hw ? base + u * GT : base;
      en[u] = *(const f32x4*)(en_p + (size_t)px * 4);
      ep[u] = *(const f32x4*)(ep_p + (size_t)px * 4);
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) f(base + u * GT, base + u * GT < hw, en[u], ep[u]);
  }
}

__device__ __forceinline__ void dyn_clear(DynShared& sh) {          // (after a barrier that ends every read of the last histogram)
  unsigned* h = &sh.hist[0][0];
#pragma unroll
  for (int j = 0; j < 4 * DYN_BINS / GT; ++j) h[threadIdx.x + j * GT] = 0u;
}

// The histograms of this digit are complete in sh.hist[c][0 .. nb) (a barrier lies behind the last atomic).  Threads 256 c .. 256 c + 255 scan channel
// c's bins, nb / 256 consecutive ones each; the one thread whose bins hold rank sh.rank[c] publishes sh.bin[c], the rank inside that bin and its count.
// Ends with a barrier: every thread may read the three and clear the histogram.
template <int NB>
__device__ __forceinline__ void dyn_pick(DynShared& sh) {
  constexpr int PER = NB / 256;
  const int t = threadIdx.x, c = t >> 8, l = t & 255;
  const unsigned r = sh.rank[c];
  unsigned h[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    h[j] = sh.hist[c][l * PER + j];
    s += h[j];
  }
  unsigned inc = s;                                                   // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = (unsigned)__shfl_up((int)inc, o, 64);
    if ((t & 63) >= o) inc += v;
  }
  if ((t & 63) == 63) sh.wtot[t >> 6] = inc;
  __syncthreads();
  unsigned below = inc - s;                                           // keys of channel c in the bins before this thread's
  for (int w = 4 * c; w < (t >> 6); ++w) below += sh.wtot[w];
  if (r >= below && r < below + s) {                                  // one thread per channel: the rank is below the channel's count
    unsigned b = 0, hb = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!found) {
        if (r < below + h[j]) {
          b = (unsigned)j;
          hb = h[j];
          found = true;
        } else {
          below += h[j];
        }
      }
    }
    sh.bin[c] = (unsigned)(l * PER) + b;
    sh.rank[c] = r - below;
    sh.cnt[c] = hb;
  }
  __syncthreads();
}

__global__ __launch_bounds__(GT) void guidance_dyn_kernel(sdlt_guidance_dyn_params p) {
  __shared__ DynShared sh;
  const float* tab = p.gtab;
  int k = (int)tab[0];
  k = max(1, min(k, p.gtab_rows - 1));
  const int i = max(0, min(p.ctr[0], k - 1));
  const float g = tab[4 * (1 + i)];
  const float mimic = p.dtab[4 * (1 + i)], q = p.dtab[4 * (1 + i) + 1], psi = p.dtab[4 * (1 + i) + 2];
  const int hw = p.hw, t = threadIdx.x;
  float* en_p = p.eps + (size_t)(2 * blockIdx.x) * hw * 4;
  float* ep_p = en_p + (size_t)hw * 4;
  const auto write = [&](int px, const f32x4& e) {
    *(f32x4*)(en_p + (size_t)px * 4) = e;
    *(f32x4*)(ep_p + (size_t)px * 4) = e;
  };
  if (g == 1.f) {                                         // uniform: guidance off
    dyn_pass(en_p, ep_p, hw, [&](int px, bool in, const f32x4&, const f32x4& ep) {
      if (in) write(px, ep);
    });
    return;
  }
  // ---- pass 1: the means of e_g and e_m per channel
  float sums[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  dyn_pass(en_p, ep_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = ep[c] - en[c];
      const float eg = en[c] + g * d, em = en[c] + mimic * d;
      sums[c] = sums[c] + (in ? eg : 0.f);
      sums[4 + c] = sums[4 + c] + (in ? em : 0.f);
    }
  });
  block_sum8(sums, sh.red, sh.tot);
  float mu_g[4], mu_m[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mu_g[c] = sums[c] / (float)hw;
    mu_m[c] = sums[4 + c] / (float)hw;
  }
  const float pos = q * (float)(hw - 1);
  const int lo = max(0, min((int)floorf(pos), hw - 1)), hi = min(lo + 1, hw - 1);
  const float wq = pos - (float)lo;
  // the key of c_g and the bit pattern of |c_m| of one value
  const auto keys = [&](int c, float en, float ep, unsigned& kg, unsigned& km) {
    const float d = ep - en;
    const float eg = en + g * d, em = en + mimic * d;
    kg = __float_as_uint(eg - mu_g[c]) & 0x7fffffffu;
    km = __float_as_uint(em - mu_m[c]) & 0x7fffffffu;
  };
  dyn_clear(sh);
  if (t < 4) {
    sh.rank[t] = (unsigned)lo;
    sh.amax[t] = 0u;
    sh.vmin[t] = 0xffffffffu;
  }
  __syncthreads();
  // ---- pass 2: A and the first digit (bits 30 .. 20)
  unsigned am[4] = {0u, 0u, 0u, 0u};
  dyn_pass(en_p, ep_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned kg, km;
      keys(c, en[c], ep[c], kg, km);
      if (in) {
        am[c] = max(am[c], km);
        atomicAdd(&sh.hist[c][kg >> 20], 1u);
      }
    }
  });
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    am[c] = wave_max_u(am[c]);
    if ((t & 63) == 0) atomicMax(&sh.amax[c], am[c]);
  }
  __syncthreads();
  dyn_pick<2048>(sh);
  unsigned pre[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) pre[c] = sh.bin[c];
  dyn_clear(sh);                                          // (dyn_pick ended with a barrier: sh.bin is read before the next one, the bins after it)
  __syncthreads();
  // ---- pass 3: the second digit (bits 19 .. 10) of the keys with the first digit found
  dyn_pass(en_p, ep_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned kg, km;
      keys(c, en[c], ep[c], kg, km);
      if (in && (kg >> 20) == pre[c]) atomicAdd(&sh.hist[c][(kg >> 10) & 1023u], 1u);
    }
  });
  __syncthreads();
  dyn_pick<1024>(sh);
#pragma unroll
  for (int c = 0; c < 4; ++c) pre[c] = (pre[c] << 10) | sh.bin[c];
  dyn_clear(sh);
  __syncthreads();
  // ---- pass 4: the last digit (bits 9 .. 0)
  dyn_pass(en_p, ep_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned kg, km;
      keys(c, en[c], ep[c], kg, km);
      if (in && (kg >> 10) == pre[c]) atomicAdd(&sh.hist[c][kg & 1023u], 1u);
    }
  });
  __syncthreads();
  dyn_pick<1024>(sh);
  unsigned vlo[4], vhi[4];
  bool need = false;                                      // uniform: every thread reads the same LDS words
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    vlo[c] = (pre[c] << 10) | sh.bin[c];
    vhi[c] = vlo[c];
    // rank lo is the sh.rank[c]-th of the sh.cnt[c] keys equal to v_lo: rank hi = lo + 1 is one of them too unless lo was the last
    need = need || (hi != lo && sh.rank[c] + 1u >= sh.cnt[c]);
  }
  if (need) {
    // ---- pass 5: the smallest key above v_lo per channel
    unsigned mn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    dyn_pass(en_p, ep_p, hw, [&](int, bool in, const f32x4& en, const f32x4& ep) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        unsigned kg, km;
        keys(c, en[c], ep[c], kg, km);
        if (in && kg > vlo[c]) mn[c] = min(mn[c], kg);
      }
    });
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mn[c] = wave_min_u(mn[c]);
      if ((t & 63) == 0) atomicMin(&sh.vmin[c], mn[c]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (hi != lo && sh.rank[c] + 1u >= sh.cnt[c]) vhi[c] = sh.vmin[c];
  }
  float A[4], S[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    A[c] = __uint_as_float(sh.amax[c]);
    const float v_lo = __uint_as_float(vlo[c]), v_hi = __uint_as_float(vhi[c]);
    const float Q = v_lo + wq * (v_hi - v_lo);
    S[c] = fmaxf(A[c], Q);
  }
  const float om = 1.f - psi;
  // ---- last pass: e into both row blocks.  Every read of the earlier passes lies before a barrier; a thread rewrites its own pixels only, and a
  // trip's loads (the stand-in of a pixel past the end included) come before its stores.
  dyn_pass(en_p, ep_p, hw, [&](int px, bool in, const f32x4& en, const f32x4& ep) {
    f32x4 e;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = ep[c] - en[c];
      const float eg = en[c] + g * d;
      float ed = eg;
      if (S[c] != 0.f) {
        const float cg = eg - mu_g[c];
        ed = ((fminf(fmaxf(cg, -S[c]), S[c]) / S[c]) * A[c]) + mu_g[c];
      }
      e[c] = psi == 1.f ? ed : psi * ed + om * eg;
    }
    if (in) write(px, e);
  });
}

}  // namespace

extern "C" int sdlt_guidance_dyn(const sdlt_guidance_dyn_params* p, void* stream) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_dyn: null parameter block");
  if (p->n < 1 || p->hw < 1 || (int64_t)p->n * p->hw > (1 << 28) || p->hw > (1 << 24))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_dyn: n=%d hw=%d (n hw <= 2^28, hw <= 2^24)", p->n, p->hw);
  if (p->gtab_rows < 2) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_dyn: gtab_rows=%d (the header row + at least one step)", p->gtab_rows);
  if (!p->eps || !p->gtab || !p->dtab || !p->ctr) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_guidance_dyn: null pointer");
  if ((uintptr_t)p->eps & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance_dyn: eps must be 16-byte aligned");
  if (((uintptr_t)p->gtab | (uintptr_t)p->dtab | (uintptr_t)p->ctr) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_guidance_dyn: gtab, dtab and ctr must be 4-byte aligned");
  hipLaunchKernelGGL(guidance_dyn_kernel, dim3(p->n), dim3(GT), 0, (hipStream_t)stream, *p);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
