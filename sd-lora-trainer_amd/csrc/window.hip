// sdlt_window_gather / sdlt_window_blend: the two launches that tiled diffusion (MultiDiffusion; sampler.py: sample(tile=)) adds to a
// denoising iteration.  The UNet runs on overlapping th x tw windows of the full H x W latent as ONE batch of 2 n ty tx rows; the step launches, the
// guidance pre-pass and every buffer they touch stay at full size.
//   full-size rows   ((2 j + s) H + y) W + x                    image j, s = 0 negative | 1 positive: what the step launches read and write
//   tile batch       b = 2 (j ty tx + iy tx + ix) + s, pixel row (b th + p) tw + q: the pairs stay adjacent, as UNet.forward and sdlt_guidance expect
//   gather   x_tiles[b, p, q, 0 .. ld) = x_full[j, s, ys[iy] + p, xs[ix] + q, 0 .. ld)   whole bf16 model-input rows;  tf_tiles[b] = tf_full[2 j + s]
//   blend    eps_full[j, s, y, x, 0 .. 4) = sum over the tiles (iy, ix) that cover (y, x), iy ascending then ix ascending, of
//                                           (wy[iy][y - ys[iy]] * wx[ix][x - xs[ix]]) * eps_tiles[b, y - ys[iy], x - xs[ix], 0 .. 4)
// wy [ty, th], wx [tx, tw] are vae.tile_weights' normalised 1-D tables (g = 1): over the tiles that cover a sample the products sum to 1.
// The blend is a GATHER: one thread per full-size row adds its covering tiles' terms in a fixed order and stores once - no zeroing launch, no atomics,
// no dependence on launch order.  Per term t = wy * wx rounded, u = t * v rounded, acc = acc + u from +0.0: three fp32 operations, plain operators
// under `fp contract(off)` like tileblend.hip, so a torch fp32 restatement gives the same bits (tests/tilediff_ref.py: blend32).  The covering tiles are
// found by scanning all ty and tx starts (three and more tiles may cover a sample: tile_starts(13, 8, 4) = [0, 3, 5]).
// Both are pure bandwidth kernels.  gather: eight lanes per row, one 16-byte load and store each per 64 columns, so a wave moves eight consecutive
// rows = 1 KB contiguous on both sides within a tile row.  blend: a workgroup is 64 x 4 full-size rows, the 64 lanes of a wave are 64 consecutive x
// of one y: its store is one 1 KB run, a covering tile's loads are one contiguous run of 16-byte rows, and the y scan is uniform over the wave.
// Row offsets are 64-bit.  Vector stores only.  The starts are device memory (one captured graph serves every overlap with the same tile counts), so
// the host can refuse a tile LARGER than the grid only; a start that puts a tile outside the grid is handled on the device: gather copies no row from
// outside it, blend's index into a tile is inside the tile by construction - neither reads nor writes out of bounds whatever the tables hold.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int WG_T = 256;               // gather: threads of a workgroup
constexpr int WG_LANES = 8;             // gather: lanes per row (16 bytes each per trip)
constexpr int WG_ROWS = WG_T / WG_LANES;
constexpr int WB_X = 64, WB_Y = 4;      // blend: workgroup = 64 x 4 full-size rows
constexpr int W_MAXT = 64;              // tiles per axis
constexpr int W_MAXDIM = 16384;         // H, W
constexpr int W_MAXN = 32767;           // images (grid.z = 2 n)
constexpr int W_MAXLD = 4096;           // bf16 elements of a model-input row
constexpr int64_t W_MAXROWS = (int64_t)1 << 40;   // rows of the tile batch: with W_MAXLD every byte count below stays far inside 64 bits

// grid (ceil(th tw / 32), ty tx, 2 n)
__global__ __launch_bounds__(WG_T) void window_gather_kernel(sdlt_window_params a, const uint4* __restrict__ x_full, uint4* __restrict__ x_tiles,
                                                             int ld16, const float* __restrict__ tf_full, float* __restrict__ tf_tiles) {
  const int js = blockIdx.z, tile = blockIdx.y;                  // js = 2 j + s
  const int iy = tile / a.tx, ix = tile - iy * a.tx;             // uniform
  const int64_t b = 2 * ((int64_t)(js >> 1) * (a.ty * a.tx) + tile) + (js & 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) tf_tiles[b] = tf_full[js];
  const uint32_t r = blockIdx.x * (uint32_t)WG_ROWS + (threadIdx.x >> 3);
  if (r >= (uint32_t)a.th * (uint32_t)a.tw) return;
  const int p = (int)(r / (uint32_t)a.tw), q = (int)(r - (uint32_t)p * (uint32_t)a.tw);
  const int y = a.ys[iy] + p, x = a.xs[ix] + q;
  if (y < 0 || y >= a.H || x < 0 || x >= a.W) return;            // a start outside the contract: no row is read from outside the grid
  const uint4* src = x_full + (((int64_t)js * a.H + y) * a.W + x) * ld16;
  uint4* dst = x_tiles + (b * a.th * a.tw + r) * ld16;
  for (int c = threadIdx.x & (WG_LANES - 1); c < ld16; c += WG_LANES) dst[c] = src[c];
}

// grid (ceil(W / 64), ceil(H / 4), 2 n)
__global__ __launch_bounds__(WB_X * WB_Y) void window_blend_kernel(sdlt_window_params a, const float* __restrict__ eps_tiles, float* __restrict__ eps_full) {
  const int x = blockIdx.x * WB_X + (threadIdx.x & (WB_X - 1));
  const int y = blockIdx.y * WB_Y + (threadIdx.x >> 6);
  if (x >= a.W || y >= a.H) return;
  const int js = blockIdx.z;
  const int64_t tile0 = (int64_t)(js >> 1) * (a.ty * a.tx);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int iy = 0; iy < a.ty; ++iy) {
    const int p = y - a.ys[iy];
    if (p < 0 || p >= a.th) continue;                            // uniform over the wave
    const float w_y = a.wy[(int64_t)iy * a.th + p];
    for (int ix = 0; ix < a.tx; ++ix) {
      const int q = x - a.xs[ix];
      if (q < 0 || q >= a.tw) continue;
      const float t = w_y * a.wx[(int64_t)ix * a.tw + q];
      const int64_t b = 2 * (tile0 + iy * a.tx + ix) + (js & 1);
      const f32x4 v = *(const f32x4*)(eps_tiles + ((b * a.th + p) * a.tw + q) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float u = t * v[c];
        acc[c] = acc[c] + u;
      }
    }
  }
  f32x4 o;
  o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  *(f32x4*)(eps_full + (((int64_t)js * a.H + y) * a.W + x) * 4) = o;
}

// what both entry points refuse about the block; `what` names the entry point
int window_check(const sdlt_window_params* p, bool weights, const char* what) {
  if (p == nullptr) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null parameter block", what);
  if (!p->ys || !p->xs || (weights && (!p->wy || !p->wx))) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: null table pointer", what);
  if (p->n < 1 || p->H < 1 || p->W < 1 || p->th < 1 || p->tw < 1 || p->ty < 1 || p->tx < 1)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d H=%d W=%d th=%d tw=%d ty=%d tx=%d (every extent must be positive)", what, p->n, p->H, p->W, p->th, p->tw, p->ty, p->tx);
  if (p->ty > W_MAXT || p->tx > W_MAXT) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: ty=%d tx=%d tiles (at most %d per axis)", what, p->ty, p->tx, W_MAXT);
  if (p->H > W_MAXDIM || p->W > W_MAXDIM) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: H=%d W=%d (each at most %d)", what, p->H, p->W, W_MAXDIM);
  if (p->n > W_MAXN) SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d images (at most %d)", what, p->n, W_MAXN);
  if (2 * (int64_t)p->n * p->ty * p->tx * p->th * p->tw > W_MAXROWS)      // (at most 2^16 2^12 2^28: the product itself cannot overflow)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: n=%d with %d x %d windows of %d x %d is more than 2^40 tile rows", what, p->n, p->ty, p->tx, p->th, p->tw);
  if (p->th > p->H || p->tw > p->W)
    SDLT_FAIL(SDLT_ERR_SHAPE, "%s: a %d x %d tile reaches outside the %d x %d grid", what, p->th, p->tw, p->H, p->W);
  uintptr_t tabs = (uintptr_t)p->ys | (uintptr_t)p->xs;
  if (weights) tabs |= (uintptr_t)p->wy | (uintptr_t)p->wx;
  if (tabs & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "%s: ys, xs, wy and wx must be 4-byte aligned", what);
  return SDLT_OK;
}

bool overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" int sdlt_window_gather(const sdlt_window_params* p, const void* x_full, void* x_tiles, int64_t ld, const float* tf_full, float* tf_tiles,
                                  void* stream) {
  const int rc = window_check(p, false, "sdlt_window_gather");
  if (rc != SDLT_OK) return rc;
  if (!x_full || !x_tiles || !tf_full || !tf_tiles) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_window_gather: null pointer");
  if (ld < 8 || ld > W_MAXLD) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_window_gather: ld=%lld (8 .. %d bf16 elements per row)", (long long)ld, W_MAXLD);
  if (ld % 8) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_window_gather: ld=%lld must be a multiple of 8 (16-byte row pieces)", (long long)ld);
  if (((uintptr_t)x_full | (uintptr_t)x_tiles) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_window_gather: x_full and x_tiles must be 16-byte aligned");
  if (((uintptr_t)tf_full | (uintptr_t)tf_tiles) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_window_gather: tf_full and tf_tiles must be 4-byte aligned");
  const int64_t full_rows = 2 * (int64_t)p->n * p->H * p->W, tile_rows = 2 * (int64_t)p->n * p->ty * p->tx * p->th * p->tw;
  if (overlap(x_full, full_rows * ld * 2, x_tiles, tile_rows * ld * 2))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_window_gather: x_tiles overlaps x_full (threads would read rows that other threads overwrite)");
  const int64_t chunks = ((int64_t)p->th * p->tw + WG_ROWS - 1) / WG_ROWS;
  const dim3 grid((unsigned)chunks, (unsigned)(p->ty * p->tx), (unsigned)(2 * p->n));
  hipLaunchKernelGGL(window_gather_kernel, grid, dim3(WG_T), 0, (hipStream_t)stream, *p, (const uint4*)x_full, (uint4*)x_tiles, (int)(ld / 8), tf_full,
                     tf_tiles);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}

extern "C" int sdlt_window_blend(const sdlt_window_params* p, const float* eps_tiles, float* eps_full, void* stream) {
  const int rc = window_check(p, true, "sdlt_window_blend");
  if (rc != SDLT_OK) return rc;
  if (!eps_tiles || !eps_full) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_window_blend: null pointer");
  if (((uintptr_t)eps_tiles | (uintptr_t)eps_full) & 15) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_window_blend: eps_tiles and eps_full must be 16-byte aligned");
  const int64_t full_rows = 2 * (int64_t)p->n * p->H * p->W, tile_rows = 2 * (int64_t)p->n * p->ty * p->tx * p->th * p->tw;
  if (overlap(eps_tiles, tile_rows * 16, eps_full, full_rows * 16))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_window_blend: eps_full overlaps eps_tiles (threads would read rows that other threads overwrite)");
  const dim3 grid((unsigned)((p->W + WB_X - 1) / WB_X), (unsigned)((p->H + WB_Y - 1) / WB_Y), (unsigned)(2 * p->n));
  hipLaunchKernelGGL(window_blend_kernel, grid, dim3(WB_X * WB_Y), 0, (hipStream_t)stream, *p, eps_tiles, eps_full);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
