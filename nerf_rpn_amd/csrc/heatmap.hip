// Proposal heatmap of scripts/render_heatmap.py (f4): box splat -> scipy gaussian_filter -> standardisation -> maximum-intensity render.
//   * splat (generate_heatmap :196-204 with gkern_3d :21-33): one lane per voxel, the boxes staged in LDS and visited in box order; every
//     box that contains the voxel adds (gx[i] * gy[j]) * gz[k] in float64 to the float64-widened value, rounded to float32 after each box --
//     numpy's  float32[...] += float64  (the factor tables come from the host, computed with numpy as gkern_3d does).  Bit-identical.
//   * gaussian filter (:205, scipy.ndimage defaults: mode 'reflect' = half-sample symmetric, truncate 4): one launch per axis (x, y, z in
//     that order, as scipy), float64 accumulation in scipy's order (centre tap, then (x[i-q] + x[i+q]) * w[q] for q = r .. 1), float32
//     after each axis.  Reflection has period 2n, so it holds for lines shorter than the radius.  Bit-identical to scipy.
//   * standardisation (:206-207): sum and sum of squared deviations in float64 over a fixed tree (fixed block count, fixed order, no
//     atomics: the same bits on every run), mean and std rounded to float32, then (h - mean) / std in float32 as numpy does.
//   * MIP render (replaces render_volume :243-305, semantics defined in include/nerfrpn.h): exact voxel traversal in float64.
// Compiled with -ffp-contract=off: every comparison with numpy / scipy depends on no FMA contraction.
#include "common.h"

#include <cmath>

namespace {
constexpr int kThreads = 256;
constexpr int kSplatBoxes = 256;      // boxes per LDS stage of the splat
constexpr int kRedBlocks = 512;       // fixed block count of every reduction: the summation tree does not depend on the device
constexpr int kMaxLds = 64 * 1024;
// work slots (doubles) after the two partial arrays
constexpr int kSlotSum = 2 * kRedBlocks, kSlotSq = kSlotSum + 1, kSlotLo = kSlotSum + 2, kSlotHi = kSlotSum + 3;
constexpr int kWorkDoubles = 2 * kRedBlocks + 8;
// tan(30 deg) = 1 / sqrt(3), correctly rounded: vertical field of view 60 degrees
constexpr double kTanHalfFov = 0.57735026918962576451;

// ---------------------------------------------------------------------------------------------------------------------
// splat
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void heatmap_splat_kernel(const int *__restrict__ aabbs, int nbox, const double *__restrict__ fac,
                                                                 const int *__restrict__ offs, int gaussian, int X, int Y, int Z,
                                                                 float *__restrict__ out) {
  __shared__ int sb[kSplatBoxes * 6];
  __shared__ int so[kSplatBoxes];
  const long long n = (long long)X * Y * Z;
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  int i = 0, j = 0, k = 0;
  if (v < n) {
    k = (int)(v % Z);
    const long long t = v / Z;
    j = (int)(t % Y);
    i = (int)(t / Y);
  }
  float acc = 0.f;
  for (int b0 = 0; b0 < nbox; b0 += kSplatBoxes) {
    const int nb = min(kSplatBoxes, nbox - b0);
    __syncthreads();
    for (int t = threadIdx.x; t < nb * 6; t += kThreads) sb[t] = aabbs[(long long)b0 * 6 + t];
    if (gaussian)
      for (int t = threadIdx.x; t < nb; t += kThreads) so[t] = offs[b0 + t];
    __syncthreads();
    if (v < n) {
      for (int b = 0; b < nb; ++b) {
        const int *bb = sb + b * 6;
        if (i < bb[0] || i >= bb[3] || j < bb[1] || j >= bb[4] || k < bb[2] || k >= bb[5]) continue;   // half-open [x1, x2)
        double val = 1.0;
        if (gaussian) {
          const double *g = fac + so[b];
          const int w = bb[3] - bb[0], l = bb[4] - bb[1];
          val = (g[i - bb[0]] * g[w + j - bb[1]]) * g[w + l + k - bb[2]];
        }
        acc = (float)((double)acc + val);
      }
    }
  }
  if (v < n) out[v] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// separable gaussian filter
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_index(int p, int n) {      // scipy 'reflect' (d c b a | a b c d | d c b a), period 2n
  const int period = 2 * n;
  int m = p % period;
  if (m < 0) m += period;
  return m < n ? m : period - 1 - m;
}

// x (AXIS 0) or y (AXIS 1) pass: one lane per output voxel, the lanes of a wave along z, so every tap load is one coalesced row
template <int AXIS>
__global__ __launch_bounds__(kThreads) void gauss_strided_kernel(const float *__restrict__ in, float *__restrict__ out, int X, int Y, int Z,
                                                                 int r, const double *__restrict__ weights) {
  extern __shared__ double sw[];
  for (int t = threadIdx.x; t <= r; t += kThreads) sw[t] = weights[r + t];        // centre, then offsets 1 .. r
  __syncthreads();
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= (long long)X * Y * Z) return;
  const long long t = v / Z;
  const int n = AXIS == 0 ? X : Y;
  const int pos = AXIS == 0 ? (int)(t / Y) : (int)(t % Y);
  const long long stride = AXIS == 0 ? (long long)Y * Z : (long long)Z;
  const float *line = in + (v - pos * stride);
  double acc = (double)line[pos * stride] * sw[0];
  for (int q = r; q >= 1; --q)
    acc += ((double)line[reflect_index(pos - q, n) * stride] + (double)line[reflect_index(pos + q, n) * stride]) * sw[q];
  out[v] = (float)acc;
}

// z pass: `lines` consecutive z lines per block (contiguous in memory) staged in LDS, weights after them
__global__ __launch_bounds__(kThreads) void gauss_z_kernel(const float *__restrict__ in, float *__restrict__ out, long long nlines, int Z,
                                                           int lines, int r, const double *__restrict__ weights) {
  extern __shared__ double dyn[];
  double *sw = dyn;
  float *sl = reinterpret_cast<float *>(dyn + (r + 1));
  const long long first = (long long)blockIdx.x * lines;
  const int nl = (int)min((long long)lines, nlines - first);
  const float *src = in + first * Z;
  for (int t = threadIdx.x; t <= r; t += kThreads) sw[t] = weights[r + t];
  for (int t = threadIdx.x; t < nl * Z; t += kThreads) sl[t] = src[t];
  __syncthreads();
  for (int e = threadIdx.x; e < nl * Z; e += kThreads) {
    const int ln = e / Z, k = e - ln * Z;
    const float *line = sl + ln * Z;
    double acc = (double)line[k] * sw[0];
    for (int q = r; q >= 1; --q) acc += ((double)line[reflect_index(k - q, Z)] + (double)line[reflect_index(k + q, Z)]) * sw[q];
    out[first * Z + e] = (float)acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// deterministic reductions: block partials (fixed grid, grid-stride in index order, LDS tree) -> one block sums them in index order
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double x, double *red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// MODE 0: sum x;  MODE 1: sum (x - mean)^2 with mean = work[kSlotSum] / n
template <int MODE>
__global__ __launch_bounds__(kThreads) void moment_partial_kernel(const float *__restrict__ in, long long n, double *__restrict__ work) {
  __shared__ double red[kThreads];
  const double mean = MODE == 1 ? work[kSlotSum] / (double)n : 0.0;
  double acc = 0.0;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)kRedBlocks * kThreads) {
    const double x = (double)in[e];
    acc += MODE == 0 ? x : (x - mean) * (x - mean);
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) work[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void moment_final_kernel(double *__restrict__ work, int slot) {
  __shared__ double red[kThreads];
  double acc = 0.0;
  for (int b = threadIdx.x; b < kRedBlocks; b += kThreads) acc += work[b];
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) work[slot] = s;
}

__global__ __launch_bounds__(kThreads) void standardize_kernel(const float *__restrict__ in, long long n, const double *__restrict__ work,
                                                               float *__restrict__ out, float *__restrict__ mean_std) {
  const float mean = (float)(work[kSlotSum] / (double)n);
  const float sd = (float)sqrt(work[kSlotSq] / (double)n);
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e == 0 && mean_std) {
    mean_std[0] = mean;
    mean_std[1] = sd;
  }
  if (e < n) out[e] = (in[e] - mean) / sd;
}

// min / max of V = heatmap[::d, ::d, ::d] * value_scale (float32 product, as numpy's  heatmap *= value_scale)
struct Sub {
  int X, Y, Z, d, NX, NY, NZ;
  float scale;
};
__device__ __forceinline__ float sub_value(const float *__restrict__ h, const Sub &s, int i, int j, int k) {
  return h[((long long)i * s.d * s.Y + (long long)j * s.d) * s.Z + (long long)k * s.d] * s.scale;
}

__global__ __launch_bounds__(kThreads) void range_partial_kernel(const float *__restrict__ h, Sub s, double *__restrict__ work) {
  __shared__ float rlo[kThreads], rhi[kThreads];
  const long long n = (long long)s.NX * s.NY * s.NZ;
  float lo = INFINITY, hi = -INFINITY;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)kRedBlocks * kThreads) {
    const int k = (int)(e % s.NZ);
    const long long t = e / s.NZ;
    const float x = sub_value(h, s, (int)(t / s.NY), (int)(t % s.NY), k);
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
  rlo[threadIdx.x] = lo;
  rhi[threadIdx.x] = hi;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      rlo[threadIdx.x] = fminf(rlo[threadIdx.x], rlo[threadIdx.x + st]);
      rhi[threadIdx.x] = fmaxf(rhi[threadIdx.x], rhi[threadIdx.x + st]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    work[blockIdx.x] = rlo[0];
    work[kRedBlocks + blockIdx.x] = rhi[0];
  }
}

__global__ __launch_bounds__(kThreads) void range_final_kernel(double *__restrict__ work) {
  __shared__ float rlo[kThreads], rhi[kThreads];
  float lo = INFINITY, hi = -INFINITY;
  for (int b = threadIdx.x; b < kRedBlocks; b += kThreads) {
    lo = fminf(lo, (float)work[b]);
    hi = fmaxf(hi, (float)work[kRedBlocks + b]);
  }
  rlo[threadIdx.x] = lo;
  rhi[threadIdx.x] = hi;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      rlo[threadIdx.x] = fminf(rlo[threadIdx.x], rlo[threadIdx.x + st]);
      rhi[threadIdx.x] = fmaxf(rhi[threadIdx.x], rhi[threadIdx.x + st]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    work[kSlotLo] = rlo[0];
    work[kSlotHi] = rhi[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// maximum-intensity render: one lane per (pixel, frame)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void render_mip_kernel(const float *__restrict__ h, Sub s, const double *__restrict__ cams,
                                                              const double *__restrict__ jet, int W, int H, const double *__restrict__ work,
                                                              unsigned char *__restrict__ rgb, float *__restrict__ mip) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= W * H) return;
  const int f = blockIdx.y;
  const long long pix = (long long)f * W * H + p;
  const int px = p % W, py = p / W;
  const double *c = cams + 6 * f;
  const double o[3] = {c[0], c[1], c[2]};
  double fx = c[3] - o[0], fy = c[4] - o[1], fz = c[5] - o[2];
  const double fn = sqrt(fx * fx + fy * fy + fz * fz);
  fx = fx / fn; fy = fy / fn; fz = fz / fn;
  double rx = fy, ry = -fx;                          // f x up, up = (0, 0, 1); r_z = 0
  const double rn = sqrt(rx * rx + ry * ry);
  rx = rx / rn; ry = ry / rn;
  const double ux = ry * fz, uy = -(rx * fz), uz = rx * fy - ry * fx;    // r x f
  const double sx = (2.0 * ((double)px + 0.5) / (double)W - 1.0) * kTanHalfFov * ((double)W / (double)H);
  const double sy = (1.0 - 2.0 * ((double)py + 0.5) / (double)H) * kTanHalfFov;
  const double dir[3] = {fx + sx * rx + sy * ux, fy + sx * ry + sy * uy, fz + sy * uz};
  const int nn[3] = {s.NX, s.NY, s.NZ};

  // slab test against [0, n) per axis, s > 0
  double t0 = 0.0, t1 = INFINITY;
  bool hit = true;
  for (int a = 0; a < 3; ++a) {
    if (!(dir[a] == dir[a])) {
      hit = false;
    } else if (dir[a] == 0.0) {
      if (o[a] < 0.0 || o[a] >= (double)nn[a]) hit = false;
    } else {
      const double ta = (0.0 - o[a]) / dir[a], tb = ((double)nn[a] - o[a]) / dir[a];
      t0 = fmax(t0, fmin(ta, tb));
      t1 = fmin(t1, fmax(ta, tb));
    }
  }
  hit = hit && t0 < t1;      // (a degenerate camera gives NaN directions: a miss)
  float m = -INFINITY;
  if (hit) {
    int cell[3];
    for (int a = 0; a < 3; ++a) {
      const double q = o[a] + t0 * dir[a];
      double fl = floor(q);
      if (dir[a] < 0.0 && fl == q) fl -= 1.0;      // on a cell face moving down: the cell below is the one crossed
      cell[a] = (int)fmin(fmax(fl, 0.0), (double)(nn[a] - 1));
    }
    // Amanatides-Woo: the exit parameter of each axis is recomputed from the cell index (no accumulated drift); axes whose faces are
    // crossed at the same parameter step together, so zero-length cells are not visited
    for (int it = 0; it < s.NX + s.NY + s.NZ + 3; ++it) {
      m = fmaxf(m, sub_value(h, s, cell[0], cell[1], cell[2]));
      double te[3];
      for (int a = 0; a < 3; ++a)
        te[a] = dir[a] > 0.0 ? ((double)(cell[a] + 1) - o[a]) / dir[a] : dir[a] < 0.0 ? ((double)cell[a] - o[a]) / dir[a] : INFINITY;
      const double tn = fmin(te[0], fmin(te[1], te[2]));
      if (!(tn < t1)) break;
      bool inside = true;
      for (int a = 0; a < 3; ++a) {
        if (te[a] == tn) cell[a] += dir[a] > 0.0 ? 1 : -1;
        inside = inside && cell[a] >= 0 && cell[a] < nn[a];
      }
      if (!inside) break;
    }
  }
  if (mip) mip[pix] = m;
  unsigned char out[3] = {0, 0, 0};
  if (hit) {
    const float lo = (float)work[kSlotLo], hi = (float)work[kSlotHi];
    float t = hi > lo ? (m - lo) / (hi - lo) : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    const int idx = min((int)(t * 256.f), 255);
    for (int ch = 0; ch < 3; ++ch) out[ch] = (unsigned char)rint(255.0 * jet[idx * 3 + ch] * (double)t);
  }
  rgb[pix * 3 + 0] = out[0];
  rgb[pix * 3 + 1] = out[1];
  rgb[pix * 3 + 2] = out[2];
}

int check_volume(const char *who, int x, int y, int z) {
  if (!(x > 0 && y > 0 && z > 0)) return nrpn_fail(NRPN_ERR_ARG, "%s: bad dims %d x %d x %d", who, x, y, z);
  if ((long long)x * y * z >= (1ll << 40)) return nrpn_fail(NRPN_ERR_ARG, "%s: volume too large", who);
  return NRPN_OK;
}
}  // namespace

extern "C" int nrpn_heatmap_splat(const int32_t *aabbs, int num_boxes, const double *factors, const int32_t *factor_offsets, int kernel_type,
                                  int x, int y, int z, float *out, nrpn_stream_t stream) {
  if (int rc = check_volume("heatmap_splat", x, y, z)) return rc;
  NRPN_REQUIRE(num_boxes >= 0, "heatmap_splat: bad box count %d (K < 0)", num_boxes);
  NRPN_REQUIRE(kernel_type == NRPN_HEATMAP_GAUSSIAN || kernel_type == NRPN_HEATMAP_BOX, "heatmap_splat: bad kernel_type %d", kernel_type);
  NRPN_REQUIRE(out && (num_boxes == 0 || (aabbs && (kernel_type == NRPN_HEATMAP_BOX || (factors && factor_offsets)))),
               "heatmap_splat: null pointer");
  const long long n = (long long)x * y * z;
  hipLaunchKernelGGL(heatmap_splat_kernel, dim3((unsigned)cdiv64(n, kThreads)), dim3(kThreads), 0, as_stream(stream), aabbs, num_boxes,
                     factors, factor_offsets, kernel_type == NRPN_HEATMAP_GAUSSIAN ? 1 : 0, x, y, z, out);
  NRPN_LAUNCH_CHECK("heatmap_splat");
  return NRPN_OK;
}

extern "C" int nrpn_gaussian_filter3d(const float *in, int x, int y, int z, float sigma, int radius, const double *weights, float *work,
                                      float *out, nrpn_stream_t stream) {
  if (int rc = check_volume("gaussian_filter3d", x, y, z)) return rc;
  NRPN_REQUIRE(sigma >= 0.f && std::isfinite(sigma), "gaussian_filter3d: bad sigma %g (negative, NaN or infinite)", (double)sigma);
  NRPN_REQUIRE(radius >= 0, "gaussian_filter3d: bad radius %d", radius);
  NRPN_REQUIRE(in && out && work && weights, "gaussian_filter3d: null pointer");
  NRPN_REQUIRE(in != out && in != work && out != work, "gaussian_filter3d: in, work and out must be distinct buffers");
  const long long n = (long long)x * y * z;
  hipStream_t st = as_stream(stream);
  if (sigma <= 1e-15f) {      // scipy filters only the axes with sigma > 1e-15 and copies otherwise
    NRPN_HIP(hipMemcpyAsync(out, in, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return NRPN_OK;
  }
  const int lines = max(1, kThreads / z);
  const size_t wbytes = (size_t)(radius + 1) * sizeof(double);
  const size_t zbytes = wbytes + (size_t)lines * z * sizeof(float);
  NRPN_REQUIRE(zbytes <= (size_t)kMaxLds, "gaussian_filter3d: z line of %d with radius %d does not fit in LDS", z, radius);
  const unsigned blocks = (unsigned)cdiv64(n, kThreads);
  hipLaunchKernelGGL(gauss_strided_kernel<0>, dim3(blocks), dim3(kThreads), wbytes, st, in, out, x, y, z, radius, weights);
  hipLaunchKernelGGL(gauss_strided_kernel<1>, dim3(blocks), dim3(kThreads), wbytes, st, (const float *)out, work, x, y, z, radius, weights);
  const long long nlines = (long long)x * y;
  hipLaunchKernelGGL(gauss_z_kernel, dim3((unsigned)cdiv64(nlines, lines)), dim3(kThreads), zbytes, st, (const float *)work, out, nlines, z,
                     lines, radius, weights);
  NRPN_LAUNCH_CHECK("gaussian_filter3d");
  return NRPN_OK;
}

extern "C" int nrpn_heatmap_work_doubles(void) { return kWorkDoubles; }

extern "C" int nrpn_heatmap_standardize(const float *in, int64_t n, double *work, float *out, float *mean_std, nrpn_stream_t stream) {
  NRPN_REQUIRE(n > 0 && n < (1ll << 40), "heatmap_standardize: bad element count %lld", (long long)n);
  NRPN_REQUIRE(in && work && out, "heatmap_standardize: null pointer");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(moment_partial_kernel<0>, dim3(kRedBlocks), dim3(kThreads), 0, st, in, (long long)n, work);
  hipLaunchKernelGGL(moment_final_kernel, dim3(1), dim3(kThreads), 0, st, work, kSlotSum);
  hipLaunchKernelGGL(moment_partial_kernel<1>, dim3(kRedBlocks), dim3(kThreads), 0, st, in, (long long)n, work);
  hipLaunchKernelGGL(moment_final_kernel, dim3(1), dim3(kThreads), 0, st, work, kSlotSq);
  hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)cdiv64(n, kThreads)), dim3(kThreads), 0, st, in, (long long)n, (const double *)work,
                     out, mean_std);
  NRPN_LAUNCH_CHECK("heatmap_standardize");
  return NRPN_OK;
}

extern "C" int nrpn_render_mip(const float *heatmap, int x, int y, int z, int downsample, float value_scale, const double *cams,
                               int num_frames, const double *jet, int width, int height, double *work, uint8_t *rgb, float *mip,
                               nrpn_stream_t stream) {
  if (int rc = check_volume("render_mip", x, y, z)) return rc;
  NRPN_REQUIRE(downsample >= 1, "render_mip: bad downsample %d (d < 1)", downsample);
  NRPN_REQUIRE(width > 0 && height > 0 && (long long)width * height < (1ll << 30), "render_mip: bad image size %d x %d", width, height);
  NRPN_REQUIRE(num_frames >= 0 && num_frames < 65536, "render_mip: bad frame count %d", num_frames);
  NRPN_REQUIRE(std::isfinite(value_scale), "render_mip: bad value_scale %g", (double)value_scale);
  if (num_frames == 0) return NRPN_OK;
  NRPN_REQUIRE(heatmap && cams && jet && work && rgb, "render_mip: null pointer");
  Sub s{x, y, z, downsample, (x + downsample - 1) / downsample, (y + downsample - 1) / downsample, (z + downsample - 1) / downsample,
        value_scale};
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(range_partial_kernel, dim3(kRedBlocks), dim3(kThreads), 0, st, heatmap, s, work);
  hipLaunchKernelGGL(range_final_kernel, dim3(1), dim3(kThreads), 0, st, work);
  hipLaunchKernelGGL(render_mip_kernel, dim3((unsigned)cdiv64((long long)width * height, kThreads), (unsigned)num_frames), dim3(kThreads), 0, st,
                     heatmap, s, cams, jet, width, height, (const double *)work, rgb, mip);
  NRPN_LAUNCH_CHECK("render_mip");
  return NRPN_OK;
}
