// PLY export of scripts/visualize_rpn_input.py (f4): cubic zoom of the objectness levels -> score grid -> ASCII point rows.
//   * cubic zoom (get_objectness_grid :145-156, scipy.ndimage.zoom(order=3) with its defaults: mode 'constant', prefilter, grid_mode
//     False): the B-spline prefilter is one lane per line, axes x, y, z in turn, in float64 in scipy's order (gain first, then the causal
//     and anticausal passes with the mirror initialisation; lines of length 1 are left alone).  The interpolation is one lane per output
//     voxel: 4 x 4 x 4 taps at o * (n_in - 1) / (n_out - 1), mirrored indices, weights and summation in scipy's order ((c * wx) * wy) * wz,
//     x taps outermost; a coordinate past n_in - 1 (fp64 rounding of the last output) gives 0, as scipy's constant mode does.  Float32 out.
//   * score grid: the levels' zooms fused per voxel -- float32 rounding of every level kept, float64 sum in level order -- written in
//     the reference's point order (z, then y, then x), then divided by the maximum (NaN-propagating, fixed tree, no atomics).
//   * point rows (write_rgb_to_ply / write_objectness_heatmap_to_ply :127-142): a per-workgroup count of kept points and row bytes, an
//     exclusive scan, then ordered writes of  "%.6f %.6f %.6f %u %u %u\n"  into one byte buffer.  %.6f is exact: the binary value times
//     10^6 in 128-bit integers, rounded half-even.
// Compiled with -ffp-contract=off: the zoom, the score grid and the coordinates are compared bit for bit with numpy / scipy.
#include "common.h"

#include <cmath>

namespace {
constexpr int kThreads = 256;
constexpr int kMaxLevels = 8;
constexpr int kRedBlocks = 512;          // fixed block count of the max reduction
constexpr int kPlyItems = 8;             // points per lane of the PLY passes
constexpr int kPlyChunk = kThreads * kPlyItems;
constexpr int kScanThreads = 1024;
// the cubic B-spline pole sqrt(3) - 2 as scipy writes it (a decimal literal: it differs from sqrt(3.0) - 2.0 in the last bit)
constexpr double kPole = -0.267949192431122706472553658494127633;

struct LevelSet {
  int count;
  int n[kMaxLevels][3];            // input dims of each level
  long long off[kMaxLevels + 1];   // element offset of each level in the packed input / coefficient buffers
  double zn1[kMaxLevels][3];       // pow(pole, n - 1) per axis (host libm, as scipy computes it)
  int o[3];                        // output dims (the same for every level)
};

// ---------------------------------------------------------------------------------------------------------------------
// B-spline prefilter: one lane per (level, line) of axis AXIS, in place on the float64 coefficients (the x pass reads the float32 input)
// ---------------------------------------------------------------------------------------------------------------------
template <int AXIS>
__global__ __launch_bounds__(kThreads) void spline_prefilter_kernel(const float *__restrict__ in, double *__restrict__ coef, LevelSet ls) {
  long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  int l = 0;
  for (; l < ls.count; ++l) {
    const long long lines = (ls.off[l + 1] - ls.off[l]) / ls.n[l][AXIS];
    if (t < lines) break;
    t -= lines;
  }
  if (l == ls.count) return;
  const int NX = ls.n[l][0], NY = ls.n[l][1], NZ = ls.n[l][2];
  const int n = ls.n[l][AXIS];
  long long base, s;
  if (AXIS == 0) {          // lines along x: t = (y, z)
    base = t;
    s = (long long)NY * NZ;
  } else if (AXIS == 1) {   // lines along y: t = (x, z)
    base = (t / NZ) * NY * NZ + t % NZ;
    s = NZ;
  } else {                  // lines along z: t = (x, y)
    base = t * NZ;
    s = 1;
  }
  double *c = coef + ls.off[l] + base;
  const float *src = in + ls.off[l] + base;
  if (n < 2) {
    if (AXIS == 0) c[0] = (double)src[0];
    return;
  }
  const double z = kPole;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int i = 0; i < n; ++i) c[i * s] = (AXIS == 0 ? (double)src[i * s] : c[i * s]) * gain;
  // causal initialisation, mirror boundary
  const double zn1 = ls.zn1[l][AXIS];
  double c0 = c[0] + zn1 * c[(n - 1) * s];
  double zi = z;
  for (int i = 1; i < n - 1; ++i) {
    c0 += zi * (c[i * s] + zn1 * c[(n - 1 - i) * s]);
    zi *= z;
  }
  c0 /= 1.0 - zn1 * zn1;
  c[0] = c0;
  double prev = c0;
  for (int i = 1; i < n; ++i) {
    const double v = c[i * s] + z * prev;
    c[i * s] = v;
    prev = v;
  }
  // anticausal initialisation, mirror boundary
  double next = (z * c[(n - 2) * s] + prev) * z / (z * z - 1.0);
  c[(n - 1) * s] = next;
  for (int i = n - 2; i >= 0; --i) {
    next = z * (next - c[i * s]);
    c[i * s] = next;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// cubic interpolation at output voxel (i, j, k) of level l
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mirror_index(int idx, int len) {     // scipy's whole-sample mirror of a spline index
  if (len <= 1) return 0;
  const int s2 = 2 * len - 2;
  if (idx < 0) {
    idx = s2 * (-idx / s2) + idx;
    idx = idx <= 1 - len ? idx + s2 : -idx;
  } else if (idx >= len) {
    idx -= s2 * (idx / s2);
    if (idx >= len) idx = s2 - idx;
  }
  return idx;
}

struct AxisTaps {
  int idx[4];
  double w[4];
};

// false when the coordinate lies past the last input sample (scipy's constant mode then writes cval = 0)
__device__ __forceinline__ bool axis_taps(int o, int n_in, int n_out, AxisTaps &a) {
  const double zoom = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0;
  const double cc = (double)o * zoom;
  if (cc > (double)(n_in - 1)) return false;
  const double fl = floor(cc);
  const int start = (int)fl - 1;
#pragma unroll
  for (int h = 0; h < 4; ++h) a.idx[h] = mirror_index(start + h, n_in);
  const double y = cc - fl, zz = 1.0 - y;
  a.w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  a.w[2] = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0;
  a.w[0] = zz * zz * zz / 6.0;
  double w3 = 1.0;
  w3 -= a.w[0];
  w3 -= a.w[1];
  w3 -= a.w[2];
  a.w[3] = w3;
  return true;
}

__device__ __forceinline__ float zoom_at(const double *__restrict__ c, const int *n, const int *no, int i, int j, int k) {
  AxisTaps ax, ay, az;
  if (!axis_taps(i, n[0], no[0], ax) || !axis_taps(j, n[1], no[1], ay) || !axis_taps(k, n[2], no[2], az)) return 0.f;
  double t = 0.0;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      const double *row = c + ((long long)ax.idx[a] * n[1] + ay.idx[b]) * n[2];
#pragma unroll
      for (int d = 0; d < 4; ++d) t += ((row[az.idx[d]] * ax.w[a]) * ay.w[b]) * az.w[d];
    }
  return (float)t;
}

__global__ __launch_bounds__(kThreads) void zoom_kernel(const double *__restrict__ coef, LevelSet ls, float *__restrict__ out) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long n = (long long)ls.o[0] * ls.o[1] * ls.o[2];
  if (v >= n) return;
  const int k = (int)(v % ls.o[2]);
  const long long t = v / ls.o[2];
  out[v] = zoom_at(coef, ls.n[0], ls.o, (int)(t / ls.o[1]), (int)(t % ls.o[1]), k);
}

// acc = 0.0; acc += zoom(level l) (float32) for every level in order; written at the point index (k * Y + j) * X + i
__global__ __launch_bounds__(kThreads) void objectness_acc_kernel(const double *__restrict__ coef, LevelSet ls, double *__restrict__ score) {
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long n = (long long)ls.o[0] * ls.o[1] * ls.o[2];
  if (p >= n) return;
  const int i = (int)(p % ls.o[0]);
  const long long t = p / ls.o[0];
  const int j = (int)(t % ls.o[1]), k = (int)(t / ls.o[1]);
  double acc = 0.0;
  for (int l = 0; l < ls.count; ++l) acc += (double)zoom_at(coef + ls.off[l], ls.n[l], ls.o, i, j, k);
  score[p] = acc;
}

// numpy's max: NaN propagates
__device__ __forceinline__ double nan_max(double m, double x) { return (x > m || x != x) ? x : m; }

__device__ __forceinline__ double block_max(double x, double *red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = nan_max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kThreads) void max_partial_kernel(const double *__restrict__ x, long long n, double *__restrict__ work) {
  __shared__ double red[kThreads];
  double m = -INFINITY;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)kRedBlocks * kThreads) m = nan_max(m, x[e]);
  const double r = block_max(m, red);
  if (threadIdx.x == 0) work[blockIdx.x] = r;
}

__global__ __launch_bounds__(kThreads) void max_final_kernel(double *__restrict__ work) {
  __shared__ double red[kThreads];
  double m = -INFINITY;
  for (int b = threadIdx.x; b < kRedBlocks; b += kThreads) m = nan_max(m, work[b]);
  const double r = block_max(m, red);
  if (threadIdx.x == 0) work[kRedBlocks] = r;
}

__global__ __launch_bounds__(kThreads) void divide_kernel(double *__restrict__ x, long long n, const double *__restrict__ work) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e < n) x[e] = x[e] / work[kRedBlocks];
}

// ---------------------------------------------------------------------------------------------------------------------
// PLY point rows
// ---------------------------------------------------------------------------------------------------------------------
struct PlyArgs {
  const float *rgbsigma;      // [sx][sy][sz][4]
  const double *score;        // point order, or null (rgb rows)
  const unsigned char *turbo; // [256][3]
  int sx, sy, sz, rx, ry, rz;
  long long n;
  float threshold;
  double step[3];             // linspace step n / (n - 1) per axis
  double scale, half;         // res.max(), 0.5 * (1.0 / res.max())
};

// "%.6f" of v: sign, integer part and 6 fraction digits of the exact binary value rounded half-even (|v| < 2^44)
struct Fixed6 {
  unsigned long long ip;
  unsigned frac;
  int neg;
};

__device__ __forceinline__ Fixed6 fixed6(double v) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  Fixed6 r;
  r.neg = (int)(bits >> 63);
  int ex = (int)((bits >> 52) & 0x7ff);
  unsigned long long m = bits & ((1ull << 52) - 1);
  if (ex == 0) ex = 1;
  else m |= 1ull << 52;
  const int e = ex - 1075;       // |v| = m * 2^e
  const unsigned __int128 p = (unsigned __int128)m * 1000000u;
  unsigned long long q;
  if (e >= 0) {
    q = (unsigned long long)(p << e);
  } else if (-e >= 127) {
    q = 0;                      // p < 2^73: below half a unit
  } else {
    const int sh = -e;
    const unsigned __int128 qq = p >> sh;
    const unsigned __int128 rem = p - (qq << sh), half = (unsigned __int128)1 << (sh - 1);
    q = (unsigned long long)qq;
    if (rem > half || (rem == half && (q & 1))) ++q;
  }
  r.ip = q / 1000000ull;
  r.frac = (unsigned)(q - r.ip * 1000000ull);
  return r;
}

__device__ __forceinline__ int dec_digits(unsigned long long x) {
  int d = 1;
  while (x >= 10) {
    x /= 10;
    ++d;
  }
  return d;
}

__device__ __forceinline__ int fixed6_len(const Fixed6 &f) { return f.neg + dec_digits(f.ip) + 7; }

__device__ __forceinline__ unsigned char *put_fixed6(unsigned char *o, const Fixed6 &f) {
  if (f.neg) *o++ = '-';
  const int d = dec_digits(f.ip);
  unsigned long long x = f.ip;
  for (int q = d - 1; q >= 0; --q) {
    o[q] = (unsigned char)('0' + x % 10);
    x /= 10;
  }
  o += d;
  *o++ = '.';
  unsigned fr = f.frac;
  for (int q = 5; q >= 0; --q) {
    o[q] = (unsigned char)('0' + fr % 10);
    fr /= 10;
  }
  return o + 6;
}

__device__ __forceinline__ int u8_len(unsigned v) { return v >= 100 ? 3 : v >= 10 ? 2 : 1; }

__device__ __forceinline__ unsigned char *put_u8(unsigned char *o, unsigned v) {
  const int d = u8_len(v);
  for (int q = d - 1; q >= 0; --q) {
    o[q] = (unsigned char)('0' + v % 10);
    v /= 10;
  }
  return o + d;
}

__device__ __forceinline__ double grid_coord(int k, int n, double step, const PlyArgs &a) {
  // numpy's linspace(0, n, n): k * step, the last value exactly n, a single value 0; then / res.max() + 0.5 / res.max()
  const double lv = n == 1 ? 0.0 : (k == n - 1 ? (double)n : (double)k * step);
  return lv / a.scale + a.half;
}

// the row of point p (length only when o is null); 0 when the point is not kept
__device__ int point_row(const PlyArgs &a, long long p, unsigned char *o) {
  // rgb / alpha: point p of rgbsigma.transpose(2, 1, 0, 3), i.e. p = (z * sy + y) * sx + x
  const int x = (int)(p % a.sx);
  const long long t = p / a.sx;
  const int y = (int)(t % a.sy), z = (int)(t / a.sy);
  const float4 v = *reinterpret_cast<const float4 *>(a.rgbsigma + (((long long)x * a.sy + y) * a.sz + z) * 4);
  float alpha = 1.0f - expf(-expf(v.w) / 100.0f);        // density_to_alpha, float32
  if (alpha == alpha) alpha = fminf(fmaxf(alpha, 0.f), 1.f);
  if (!(alpha > a.threshold)) return 0;
  unsigned rgb[3];
  if (a.score) {
    // matplotlib Colormap.__call__ on a float: int(s * 256), s == 1 -> 255, under -> entry 0, over -> entry 255, NaN -> (0, 0, 0)
    const double s = a.score[p];
    if (s != s) {
      rgb[0] = rgb[1] = rgb[2] = 0;
    } else {
      const double xa = s * 256.0;
      const int idx = xa < 0.0 ? 0 : xa >= 256.0 ? 255 : (int)xa;
      for (int c = 0; c < 3; ++c) rgb[c] = a.turbo[idx * 3 + c];
    }
  } else {
    const float c3[3] = {v.x, v.y, v.z};
    for (int c = 0; c < 3; ++c) {
      const float f = c3[c];
      rgb[c] = f > 0.f ? (f < 1.f ? (unsigned)(f * 255.0f) : 255u) : 0u;     // (c * 255).astype(uint8), clamped to [0, 1]; NaN -> 0
    }
  }
  // coordinates: point p of the grid built from res, x fastest
  const int ix = (int)(p % a.rx);
  const long long u = p / a.rx;
  const int iy = (int)(u % a.ry), iz = (int)(u / a.ry);
  const Fixed6 fx = fixed6(grid_coord(ix, a.rx, a.step[0], a)), fy = fixed6(grid_coord(iy, a.ry, a.step[1], a)),
               fz = fixed6(grid_coord(iz, a.rz, a.step[2], a));
  const int len = fixed6_len(fx) + fixed6_len(fy) + fixed6_len(fz) + u8_len(rgb[0]) + u8_len(rgb[1]) + u8_len(rgb[2]) + 6;
  if (o) {
    o = put_fixed6(o, fx);
    *o++ = ' ';
    o = put_fixed6(o, fy);
    *o++ = ' ';
    o = put_fixed6(o, fz);
    for (int c = 0; c < 3; ++c) {
      *o++ = ' ';
      o = put_u8(o, rgb[c]);
    }
    *o = '\n';
  }
  return len;
}

// work: int64 [2 * blocks] = (kept points, row bytes) per workgroup of kPlyChunk points, then their exclusive scan
__global__ __launch_bounds__(kThreads) void ply_count_kernel(PlyArgs a, long long *__restrict__ work) {
  __shared__ long long rc[kThreads], rb[kThreads];
  long long cnt = 0, bytes = 0;
  const long long p0 = (long long)blockIdx.x * kPlyChunk;
  for (int it = 0; it < kPlyItems; ++it) {
    const long long p = p0 + (long long)it * kThreads + threadIdx.x;
    if (p < a.n) {
      const int len = point_row(a, p, nullptr);
      cnt += len > 0;
      bytes += len;
    }
  }
  rc[threadIdx.x] = cnt;
  rb[threadIdx.x] = bytes;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      rc[threadIdx.x] += rc[threadIdx.x + s];
      rb[threadIdx.x] += rb[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    work[2 * blockIdx.x] = rc[0];
    work[2 * blockIdx.x + 1] = rb[0];
  }
}

// exclusive scan of the per-workgroup (count, bytes) in place; totals = (kept points, bytes).  One workgroup, contiguous segments per lane.
__global__ __launch_bounds__(kScanThreads) void ply_scan_kernel(long long *__restrict__ work, int nblocks, long long *__restrict__ totals) {
  __shared__ long long sc[kScanThreads], sb[kScanThreads];
  const int per = (nblocks + kScanThreads - 1) / kScanThreads;
  const int b0 = min(nblocks, (int)threadIdx.x * per), b1 = min(nblocks, b0 + per);
  long long c = 0, b = 0;
  for (int k = b0; k < b1; ++k) {
    c += work[2 * k];
    b += work[2 * k + 1];
  }
  sc[threadIdx.x] = c;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int s = 1; s < kScanThreads; s <<= 1) {      // inclusive Hillis-Steele scan of the segment sums
    long long vc = 0, vb = 0;
    if ((int)threadIdx.x >= s) {
      vc = sc[threadIdx.x - s];
      vb = sb[threadIdx.x - s];
    }
    __syncthreads();
    sc[threadIdx.x] += vc;
    sb[threadIdx.x] += vb;
    __syncthreads();
  }
  c = threadIdx.x ? sc[threadIdx.x - 1] : 0;
  b = threadIdx.x ? sb[threadIdx.x - 1] : 0;
  for (int k = b0; k < b1; ++k) {
    const long long wc = work[2 * k], wb = work[2 * k + 1];
    work[2 * k] = c;
    work[2 * k + 1] = b;
    c += wc;
    b += wb;
  }
  if (threadIdx.x == kScanThreads - 1) {
    totals[0] = sc[kScanThreads - 1];
    totals[1] = sb[kScanThreads - 1];
  }
}

// ordered writes: the rows of workgroup b start at its scanned byte offset, in point order
__global__ __launch_bounds__(kThreads) void ply_write_kernel(PlyArgs a, const long long *__restrict__ work, unsigned char *__restrict__ out) {
  __shared__ int sl[kThreads];
  long long base = work[2 * blockIdx.x + 1];
  const long long p0 = (long long)blockIdx.x * kPlyChunk;
  for (int it = 0; it < kPlyItems; ++it) {
    const long long p = p0 + (long long)it * kThreads + threadIdx.x;
    const int len = p < a.n ? point_row(a, p, nullptr) : 0;
    sl[threadIdx.x] = len;
    __syncthreads();
    for (int s = 1; s < kThreads; s <<= 1) {       // inclusive scan of the row lengths
      const int v = (int)threadIdx.x >= s ? sl[threadIdx.x - s] : 0;
      __syncthreads();
      sl[threadIdx.x] += v;
      __syncthreads();
    }
    if (len > 0) point_row(a, p, out + base + sl[threadIdx.x] - len);
    base += sl[kThreads - 1];
    __syncthreads();
  }
}

int fill_levels(const char *who, const int32_t *h_dims, const double *h_zpow, int count, int x, int y, int z, LevelSet &ls) {
  NRPN_REQUIRE(count >= 1 && count <= kMaxLevels, "%s: bad level count %d (1 .. %d)", who, count, kMaxLevels);
  NRPN_REQUIRE(h_dims && h_zpow, "%s: null pointer", who);
  NRPN_REQUIRE(x > 0 && y > 0 && z > 0 && (long long)x * y * z < (1ll << 40), "%s: bad output dims %d x %d x %d", who, x, y, z);
  ls.count = count;
  ls.o[0] = x;
  ls.o[1] = y;
  ls.o[2] = z;
  ls.off[0] = 0;
  for (int l = 0; l < count; ++l) {
    for (int a = 0; a < 3; ++a) {
      ls.n[l][a] = h_dims[l * 3 + a];
      ls.zn1[l][a] = h_zpow[l * 3 + a];
      NRPN_REQUIRE(ls.n[l][a] > 0 && ls.n[l][a] < (1 << 20), "%s: bad input dims of level %d", who, l);
    }
    ls.off[l + 1] = ls.off[l] + (long long)ls.n[l][0] * ls.n[l][1] * ls.n[l][2];
  }
  NRPN_REQUIRE(ls.off[count] < (1ll << 36), "%s: inputs too large", who);
  return NRPN_OK;
}

void launch_prefilter(const float *in, double *coef, const LevelSet &ls, hipStream_t st) {
  const unsigned bx = (unsigned)cdiv64(ls.off[ls.count], kThreads);     // lines of any axis <= elements
  hipLaunchKernelGGL(spline_prefilter_kernel<0>, dim3(bx), dim3(kThreads), 0, st, in, coef, ls);
  hipLaunchKernelGGL(spline_prefilter_kernel<1>, dim3(bx), dim3(kThreads), 0, st, in, coef, ls);
  hipLaunchKernelGGL(spline_prefilter_kernel<2>, dim3(bx), dim3(kThreads), 0, st, in, coef, ls);
}

int fill_ply(const char *who, const float *rgbsigma, int sx, int sy, int sz, int rx, int ry, int rz, float threshold, const double *score,
             const uint8_t *turbo, PlyArgs &a) {
  NRPN_REQUIRE(sx > 0 && sy > 0 && sz > 0 && rx > 0 && ry > 0 && rz > 0, "%s: bad dims", who);
  const long long n = (long long)sx * sy * sz;
  NRPN_REQUIRE(n == (long long)rx * ry * rz, "%s: resolution %d x %d x %d does not have the grid's %lld points", who, rx, ry, rz, n);
  NRPN_REQUIRE(n < (1ll << 40), "%s: grid too large", who);
  NRPN_REQUIRE(rgbsigma && (!score || turbo), "%s: null pointer", who);
  a.rgbsigma = rgbsigma;
  a.score = score;
  a.turbo = turbo;
  a.sx = sx, a.sy = sy, a.sz = sz, a.rx = rx, a.ry = ry, a.rz = rz;
  a.n = n;
  a.threshold = threshold;
  const int r[3] = {rx, ry, rz};
  for (int k = 0; k < 3; ++k) a.step[k] = r[k] > 1 ? (double)r[k] / (double)(r[k] - 1) : 0.0;
  a.scale = (double)max(rx, max(ry, rz));
  a.half = 0.5 * (1.0 / a.scale);
  return NRPN_OK;
}
}  // namespace

extern "C" int nrpn_zoom_cubic3d(const float *in, int nx, int ny, int nz, const double *h_zpow, int ox, int oy, int oz, double *coef,
                                 float *out, nrpn_stream_t stream) {
  const int32_t dims[3] = {nx, ny, nz};
  LevelSet ls;
  if (int rc = fill_levels("zoom_cubic3d", dims, h_zpow, 1, ox, oy, oz, ls)) return rc;
  NRPN_REQUIRE(in && coef && out, "zoom_cubic3d: null pointer");
  hipStream_t st = as_stream(stream);
  launch_prefilter(in, coef, ls, st);
  const long long n = (long long)ox * oy * oz;
  hipLaunchKernelGGL(zoom_kernel, dim3((unsigned)cdiv64(n, kThreads)), dim3(kThreads), 0, st, (const double *)coef, ls, out);
  NRPN_LAUNCH_CHECK("zoom_cubic3d");
  return NRPN_OK;
}

extern "C" int nrpn_objectness_work_doubles(void) { return kRedBlocks + 8; }

extern "C" int nrpn_objectness_grid(const float *levels, const int32_t *h_level_dims, const double *h_zpow, int num_levels, int x, int y,
                                    int z, double *coef, double *work, double *score, nrpn_stream_t stream) {
  LevelSet ls;
  if (int rc = fill_levels("objectness_grid", h_level_dims, h_zpow, num_levels, x, y, z, ls)) return rc;
  NRPN_REQUIRE(levels && coef && work && score, "objectness_grid: null pointer");
  hipStream_t st = as_stream(stream);
  launch_prefilter(levels, coef, ls, st);
  const long long n = (long long)x * y * z;
  hipLaunchKernelGGL(objectness_acc_kernel, dim3((unsigned)cdiv64(n, kThreads)), dim3(kThreads), 0, st, (const double *)coef, ls, score);
  hipLaunchKernelGGL(max_partial_kernel, dim3(kRedBlocks), dim3(kThreads), 0, st, (const double *)score, n, work);
  hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(kThreads), 0, st, work);
  hipLaunchKernelGGL(divide_kernel, dim3((unsigned)cdiv64(n, kThreads)), dim3(kThreads), 0, st, score, n, (const double *)work);
  NRPN_LAUNCH_CHECK("objectness_grid");
  return NRPN_OK;
}

extern "C" int64_t nrpn_ply_points_work_int64(int64_t n) { return 2 * cdiv64(n, kPlyChunk) + 2; }

extern "C" int nrpn_ply_points_count(const float *rgbsigma, int sx, int sy, int sz, int rx, int ry, int rz, float alpha_threshold,
                                     const double *score, const uint8_t *turbo, int64_t *work, int64_t *totals, nrpn_stream_t stream) {
  PlyArgs a;
  if (int rc = fill_ply("ply_points_count", rgbsigma, sx, sy, sz, rx, ry, rz, alpha_threshold, score, turbo, a)) return rc;
  NRPN_REQUIRE(work && totals, "ply_points_count: null pointer");
  const long long nb = cdiv64(a.n, kPlyChunk);
  NRPN_REQUIRE(nb < (1ll << 31), "ply_points_count: grid too large");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ply_count_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, a, (long long *)work);
  hipLaunchKernelGGL(ply_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (long long *)work, (int)nb, (long long *)totals);
  NRPN_LAUNCH_CHECK("ply_points_count");
  return NRPN_OK;
}

extern "C" int nrpn_ply_points_write(const float *rgbsigma, int sx, int sy, int sz, int rx, int ry, int rz, float alpha_threshold,
                                     const double *score, const uint8_t *turbo, const int64_t *work, uint8_t *out, nrpn_stream_t stream) {
  PlyArgs a;
  if (int rc = fill_ply("ply_points_write", rgbsigma, sx, sy, sz, rx, ry, rz, alpha_threshold, score, turbo, a)) return rc;
  NRPN_REQUIRE(work && out, "ply_points_write: null pointer");
  hipLaunchKernelGGL(ply_write_kernel, dim3((unsigned)cdiv64(a.n, kPlyChunk)), dim3(kThreads), 0, as_stream(stream), a,
                     (const long long *)work, out);
  NRPN_LAUNCH_CHECK("ply_points_write");
  return NRPN_OK;
}
