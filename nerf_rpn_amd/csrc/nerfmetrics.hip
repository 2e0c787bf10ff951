// Test-view metrics of a rendered NeRF frame (scripts/nerf_test.py; reference data/scannet/run_nerf.py: render_images_with_metrics
// :231-311 -- img2mse :283, structural_similarity :287, compute_rmse :277 -- and write_images_with_metrics :313-331 -- to8b :325,
// to16b :327).
//
// metrics   one workgroup per kTile x kTile tile of the frame.  The tile owns its pixels for the squared-error sums (unclamped rgb
//           against the target; depth against the target depth where the mask selects it -- an unselected target is never read) and
//           the 7 x 7 windows whose top-left pixel lies in it for SSIM.  skimage crops its SSIM map by 3 on every side, which leaves
//           exactly the windows that lie wholly inside the image, so there is no boundary rule: a window is evaluated iff its
//           top-left pixel is at most (H - 7, W - 7).  The (kTile + 6)^2 clamped rgb and target pixels a tile's windows read are staged
//           in LDS as float32 (the inputs' own format: widening is exact) and widened on use; window sums, the per-window SSIM and
//           every reduction are float64.  Products of two widened float32 values are exact in float64, so the only rounding in a
//           window moment is that of its 48 additions and one division.
// reduce    one workgroup adds the tiles' rows of partial sums in a fixed order.
// No atomics: every tile writes its own row, so repeated runs are bit-equal.
// quantise  to8b(rgb) and to16b(depth / far) in float32 with numpy's operation order (no contraction), truncating as astype does.
#include "common.h"

namespace {

constexpr int kTile = 32;                 // output tile edge; reported by nrpn_nerfmetrics_tile
constexpr int kWin = 7;                   // skimage's default win_size
constexpr int kHalo = kTile + kWin - 1;   // staged pixels per tile edge
constexpr int kLd = kHalo + 1;            // row pitch of the staged planes (bank skew)
constexpr int kThreads = 256;
constexpr int kSums = 8;                  // doubles per row: squared rgb error, ssim sum x 3, squared depth error, valid count, 2 spare

// torch.clamp / np.clip: NaN stays NaN
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// sum over the workgroup in a fixed order: lanes by shuffle, then the four waves in wave order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();                        // scratch may still be read from the previous call
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) s += scratch[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void nerfmetrics_tile_kernel(const float *__restrict__ rgb, const float *__restrict__ target,
                                                                    int H, int W, const float *__restrict__ depth,
                                                                    const float *__restrict__ target_depth,
                                                                    const unsigned char *__restrict__ valid,
                                                                    double *__restrict__ partial) {
  __shared__ float sx[3][kHalo][kLd];     // clamped rgb
  __shared__ float sy[3][kHalo][kLd];     // target
  __shared__ double scratch[kThreads / 64];
  const int t = threadIdx.x;
  const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;

  double sq = 0.0, dsq = 0.0, nv = 0.0;
  for (int i = t; i < kHalo * kHalo; i += kThreads) {
    const int r = i / kHalo, c = i - r * kHalo;
    const int gy = y0 + r, gx = x0 + c;
    float x[3] = {0.f, 0.f, 0.f}, y[3] = {0.f, 0.f, 0.f};
    if (gy < H && gx < W) {
      const int64_t p = (int64_t)gy * W + gx;
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = rgb[p * 3 + k], y[k] = target[p * 3 + k];
      if (r < kTile && c < kTile) {       // a pixel this tile owns
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double d = (double)x[k] - (double)y[k];
          sq += d * d;
        }
        if (valid && valid[p]) {
          const double d = (double)depth[p] - (double)target_depth[p];
          dsq += d * d;
          nv += 1.0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sx[k][r][c] = clamp01(x[k]), sy[k][r][c] = y[k];
  }
  __syncthreads();

  const double c1 = (0.01 * 1.0) * (0.01 * 1.0), c2 = (0.03 * 1.0) * (0.03 * 1.0);      // (K data_range)^2
  const double np = (double)(kWin * kWin), cov_norm = np / (np - 1.0);
  double ss[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < kTile * kTile; i += kThreads) {
    const int wy = i / kTile, wx = i - wy * kTile;
    if (y0 + wy > H - kWin || x0 + wx > W - kWin) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
      for (int dy = 0; dy < kWin; ++dy)
#pragma unroll
        for (int dx = 0; dx < kWin; ++dx) {
          const double a = sx[k][wy + dy][wx + dx], b = sy[k][wy + dy][wx + dx];
          sa += a, sb += b, saa += a * a, sbb += b * b, sab += a * b;
        }
      const double ux = sa / np, uy = sb / np, uxx = saa / np, uyy = sbb / np, uxy = sab / np;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
      ss[k] += (a1 * a2) / (b1 * b2);
    }
  }

  const double out[6] = {sq, ss[0], ss[1], ss[2], dsq, nv};
  double *row = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kSums;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double s = block_sum(out[k], scratch);
    if (t == 0) row[k] = s;
  }
  if (t == 0) row[6] = row[7] = 0.0;
}

// partial [rows][kSums] -> sums [kSums]: thread t adds rows t, t + 256, ... in order, then the threads are added in a fixed order
__global__ __launch_bounds__(kThreads) void nerfmetrics_reduce_kernel(const double *__restrict__ partial, int rows,
                                                                      double *__restrict__ sums) {
  __shared__ double scratch[kThreads / 64];
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int r = threadIdx.x; r < rows; r += kThreads)
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] += partial[(int64_t)r * kSums + k];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const double s = block_sum(acc[k], scratch);
    if (threadIdx.x == 0) sums[k] = s;
  }
}

__global__ void nerfmetrics_to8b_kernel(const float *__restrict__ x, int64_t n, unsigned char *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (unsigned char)(int)__fmul_rn(255.0f, clamp01(x[i]));
}

__global__ void nerfmetrics_to16b_kernel(const float *__restrict__ depth, float far, int64_t n, unsigned short *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (unsigned short)(int)__fmul_rn(65535.0f, clamp01(__fdiv_rn(depth[i], far)));
}

bool frame_ok(int h, int w) { return h >= kWin && w >= kWin && h <= (1 << 20) && w <= (1 << 20) && (int64_t)h * w < ((int64_t)1 << 31); }
int64_t tiles_of(int h, int w) { return cdiv64(h, kTile) * cdiv64(w, kTile); }

}  // namespace

extern "C" {

int nrpn_nerfmetrics_tile(void) { return kTile; }

int64_t nrpn_nerfmetrics_work_bytes(int height, int width) {
  if (!frame_ok(height, width)) return -1;
  return tiles_of(height, width) * kSums * (int64_t)sizeof(double);
}

int nrpn_nerfmetrics_frame(const float *rgb, const float *target, int height, int width, const float *depth, const float *target_depth,
                           const uint8_t *valid, void *work, int64_t work_bytes, double *sums, nrpn_stream_t stream) {
  NRPN_REQUIRE(rgb && target && work && sums, "nerfmetrics_frame: null pointer");
  NRPN_REQUIRE(frame_ok(height, width), "nerfmetrics_frame: %d x %d (the 7 x 7 SSIM window needs at least 7 x 7)", height, width);
  NRPN_REQUIRE((depth != nullptr) == (target_depth != nullptr) && (depth != nullptr) == (valid != nullptr),
               "nerfmetrics_frame: depth, target_depth and valid go together");
  NRPN_REQUIRE(reinterpret_cast<uintptr_t>(work) % 8 == 0 && reinterpret_cast<uintptr_t>(sums) % 8 == 0, "nerfmetrics_frame: alignment");
  const int64_t rows = tiles_of(height, width);
  NRPN_REQUIRE(work_bytes >= rows * kSums * (int64_t)sizeof(double), "nerfmetrics_frame: work buffer of %lld bytes is too small",
               (long long)work_bytes);
  double *partial = static_cast<double *>(work);
  const dim3 grid((unsigned)cdiv64(width, kTile), (unsigned)cdiv64(height, kTile));
  nerfmetrics_tile_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(rgb, target, height, width, depth, target_depth, valid, partial);
  NRPN_LAUNCH_CHECK("nerfmetrics_tile_kernel");
  nerfmetrics_reduce_kernel<<<1, kThreads, 0, as_stream(stream)>>>(partial, (int)rows, sums);
  NRPN_LAUNCH_CHECK("nerfmetrics_reduce_kernel");
  return NRPN_OK;
}

int nrpn_nerfmetrics_quantise(const float *rgb, int64_t num_rgb, uint8_t *rgb8, const float *depth, float far, int64_t num_depth,
                              uint16_t *depth16, nrpn_stream_t stream) {
  NRPN_REQUIRE(num_rgb >= 0 && num_depth >= 0 && num_rgb < ((int64_t)1 << 38) && num_depth < ((int64_t)1 << 38),
               "nerfmetrics_quantise: %lld / %lld values", (long long)num_rgb, (long long)num_depth);
  NRPN_REQUIRE(num_rgb == 0 || (rgb && rgb8), "nerfmetrics_quantise: null rgb pointer");
  NRPN_REQUIRE(num_depth == 0 || (depth && depth16), "nerfmetrics_quantise: null depth pointer");
  if (num_rgb) {
    nerfmetrics_to8b_kernel<<<(unsigned)cdiv64(num_rgb, 256), 256, 0, as_stream(stream)>>>(rgb, num_rgb, rgb8);
    NRPN_LAUNCH_CHECK("nerfmetrics_to8b_kernel");
  }
  if (num_depth) {
    nerfmetrics_to16b_kernel<<<(unsigned)cdiv64(num_depth, 256), 256, 0, as_stream(stream)>>>(depth, far, num_depth, depth16);
    NRPN_LAUNCH_CHECK("nerfmetrics_to16b_kernel");
  }
  return NRPN_OK;
}

}  // extern "C"
