// sdlt_blur_planes: a separable Gaussian blur of fp32 planes [C, H, W] with replicated edges - a hard mask made into a soft change map (or a soft mask) on
// the latent grid (render.py: `mask_blur`).  Two launches of one kernel, rows then columns, through a caller-given scratch of the same size:
//   scratch[c, y, x] = sum over t = -R .. +R of taps[t + R] * in[c, y, clamp(x + t, 0, W - 1)]
//   out[c, y, x]     = sum over t = -R .. +R of taps[t + R] * scratch[c, clamp(y + t, 0, H - 1), x]        clamp01: then clamped to [0, 1]
//   taps   fp32 [2 R + 1], built on the host (ops.blur_taps: normalised in fp64, rounded once), R <= 64
// Arithmetic, fixed so that a torch fp32 restatement gives the same bits (tests/blur_ref.py): the sum starts from the first product and takes the taps in
// the order -R .. +R, one multiply and one add per tap, each rounded once - plain operators under `fp contract(off)`, like tileblend.hip.  The rounded
// weights do not sum to exactly 1, so a blurred map can leave [0, 1] by an ulp: the render sets clamp01 (two compares and selects: a NaN stays a NaN).
// A launch-latency kernel at its sizes (a 128 x 128 map is 64 KB: both passes together move less than one CU streams in a microsecond, and the pair is
// bounded by two launches).  One thread per output sample; a workgroup is 64 x 4 of them, so the 64 lanes of a wave are 64 consecutive x of one row: the
// column pass reads 2 R + 1 contiguous 256-byte runs per wave, the row pass 2 R + 1 runs shifted by one float each (one or two cache lines, reused from
// L1 / L2).  The taps are read by a wave-uniform index (scalar loads).  No LDS.  Plane offsets are 64-bit.  Vector stores only.
#include "common.h"
#include "../../include/sdlt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int BL_X = 64, BL_Y = 4;      // workgroup = 64 x 4 output samples
constexpr int BL_MAXR = 64;             // largest radius (ops.blur_taps caps 3 sigma there)
constexpr int BL_MAXDIM = 16384;        // largest extent of an axis: grid.y = H / 4 stays below 65536
constexpr int BL_MAXC = 65535;          // planes per launch (grid.z)

struct BlurArgs {
  const float* src;
  float* dst;
  const float* taps;
  int H, W, R, clamp01;
};

template <bool COLS>
__global__ __launch_bounds__(BL_X * BL_Y) void blur_pass_kernel(BlurArgs a) {
  const int x = blockIdx.x * BL_X + (threadIdx.x & (BL_X - 1));
  const int y = blockIdx.y * BL_Y + (threadIdx.x >> 6);
  if (x >= a.W || y >= a.H) return;
  const int64_t plane = (int64_t)blockIdx.z * a.H * a.W;
  const float* src = a.src + plane;
  float acc = 0.f;
  for (int t = -a.R; t <= a.R; ++t) {     // every index is clamped into the plane: no read outside it, whatever R
    const int yy = COLS ? min(max(y + t, 0), a.H - 1) : y;
    const int xx = COLS ? x : min(max(x + t, 0), a.W - 1);
    const float pr = a.taps[t + a.R] * src[(int64_t)yy * a.W + xx];
    acc = t == -a.R ? pr : acc + pr;
  }
  if (COLS && a.clamp01) {
    acc = acc < 0.f ? 0.f : acc;
    acc = acc > 1.f ? 1.f : acc;
  }
  a.dst[plane + (int64_t)y * a.W + x] = acc;
}

bool overlap(const void* p, const void* q, size_t bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" int sdlt_blur_planes(const float* in, float* out, float* scratch, int32_t C, int32_t H, int32_t W, const float* taps, int32_t R, int32_t clamp01,
                                void* stream) {
  if (!in || !out || !scratch || !taps) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_blur_planes: null pointer");
  if (C < 1 || H < 1 || W < 1) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_blur_planes: C=%d H=%d W=%d (every extent must be positive)", C, H, W);
  if (H > BL_MAXDIM || W > BL_MAXDIM || C > BL_MAXC) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_blur_planes: C=%d H=%d W=%d (H, W at most %d, C at most %d)", C, H, W, BL_MAXDIM, BL_MAXC);
  if (R < 0 || R > BL_MAXR) SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_blur_planes: R=%d (0 .. %d)", R, BL_MAXR);
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)scratch | (uintptr_t)taps) & 3) SDLT_FAIL(SDLT_ERR_ALIGN, "sdlt_blur_planes: in, out, scratch and taps must be 4-byte aligned");
  const size_t bytes = (size_t)C * H * W * sizeof(float);
  if (overlap(scratch, in, bytes) || overlap(scratch, out, bytes))
    SDLT_FAIL(SDLT_ERR_SHAPE, "sdlt_blur_planes: scratch overlaps in or out (the column pass reads what the row pass wrote there)");
  const dim3 grid((unsigned)((W + BL_X - 1) / BL_X), (unsigned)((H + BL_Y - 1) / BL_Y), (unsigned)C);
  hipStream_t s = (hipStream_t)stream;
  BlurArgs a;
  a.taps = taps; a.H = H; a.W = W; a.R = R; a.clamp01 = clamp01;
  a.src = in; a.dst = scratch;
  hipLaunchKernelGGL(blur_pass_kernel<false>, grid, dim3(BL_X * BL_Y), 0, s, a);
  SDLT_CHECK_LAUNCH();
  a.src = scratch; a.dst = out;
  hipLaunchKernelGGL(blur_pass_kernel<true>, grid, dim3(BL_X * BL_Y), 0, s, a);
  SDLT_CHECK_LAUNCH();
  return SDLT_OK;
}
