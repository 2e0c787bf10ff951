// The per-ray float64 arithmetic of compute_weights and raw2outputs (data/scannet/run_nerf.py:419-469) over the merge of a ray's
// two non-decreasing sample lists (forward_with_additonal_samples :504-512), shared by nerfrender.hip (views, the camera-embedding
// objective) and nerfcomposite.hip (the differentiable ray stage): one definition, so the two give the same bits.  Likewise the ray
// of a pixel, raw2depth's walk and sample_3sigma's bins with the inverse-cdf expression, shared by nerfrender.hip and nerftrain.hip.
#pragma once
#include "common.h"

#include <cmath>

namespace nerfray {

constexpr int kRayTile = 64;      // points per tile of the MLP passes (nerf_mlp.cuh kTile), which the size limits count in

// The limits every size query and entry point shares: num_rays rays (below max_rays) in chunks of ``chunk`` with s1 + s2 samples per
// ray; the points of a chunk's pass, rounded up to tiles, are counted in an int
inline bool sizes_ok(int64_t num_rays, int64_t max_rays, int64_t chunk, int s1, int s2) {
  if (num_rays < 1 || num_rays >= max_rays || chunk < 1 || s1 < 1 || s2 < 0 || s1 > 65536 || s2 > 65536) return false;
  const int64_t n = chunk < num_rays ? chunk : num_rays;
  return n < ((int64_t)1 << 31) && n * (s1 > s2 ? s1 : s2) < ((int64_t)1 << 31) - kRayTile;
}

__device__ __forceinline__ double ray_norm(const float *d) {
  const double x = d[0], y = d[1], z = d[2];
  return sqrt(x * x + y * y + z * z);
}

// compute_weights (:419-429) for one sample: alpha from relu(sigma) and dist; T is the transmittance before it and is advanced
__device__ __forceinline__ double sample_weight(double sigma, double dist, double &T) {
  const double alpha = 1.0 - exp(-fmax(sigma, 0.0) * dist);
  const double w = alpha * T;
  T *= 1.0 - alpha + 1e-10;
  return w;
}

struct MergeCursor {      // the order of a ray's two non-decreasing sample lists: the smaller head first, list 1 on a tie
  const float *za, *zb;
  int S1, S2, ia, ib;
  __device__ __forceinline__ bool next(int &i) {
    const bool a = ib >= S2 || (ia < S1 && za[ia] <= zb[ib]);
    i = a ? ia++ : ib++;
    return a;
  }
};

// One ray's samples in merged order: visit(from list 1?, index in that list, z, sigma, dist, T before the sample, weight).  sigma =
// load(from list 1?, index), of type Sig, is what compute_weights puts under the relu; dist is the distance to the next sample times
// |d| = nd, 1e10 |d| after the last; the weight is compute_weights' of the sample in the merged list.  A sample's sigma is loaded with
// its z, one sample ahead of its use: a thread's loop waits on these loads and on little else
template <class Sig, class Load, class Visit>
__device__ __forceinline__ void merged_walk_sigma(const float *za, int S1, const float *zb, int S2, double nd, Load &&load, Visit &&visit) {
  MergeCursor m{za, zb, S1, S2, 0, 0};
  const int S = S1 + S2;
  int i;
  bool a = m.next(i);
  float zc = a ? za[i] : zb[i];
  Sig sg = load(a, i);
  double T = 1.0;
  for (int s = 0; s < S; ++s) {
    int in = i;
    bool an = a;
    float zn = zc;
    Sig sn = sg;
    if (s + 1 < S) {
      an = m.next(in);
      zn = an ? za[in] : zb[in];
      sn = load(an, in);
    }
    const double dist = (s + 1 < S ? (double)zn - (double)zc : 1e10) * nd;
    const double Tb = T;
    const double w = sample_weight((double)sg, dist, T);
    visit(a, i, zc, (double)sg, dist, Tb, w);
    a = an, i = in, zc = zn, sg = sn;
  }
}

// The walk over the lists' own float32 sigma, sa / sb, 4 floats apart: visit(from list 1?, index in that list, z, weight)
template <class Visit>
__device__ __forceinline__ void merged_walk(const float *za, const float *sa, int S1, const float *zb, const float *sb, int S2,
                                            double nd, Visit &&visit) {
  merged_walk_sigma<float>(
      za, S1, zb, S2, nd, [&](bool a, int i) { return a ? sa[4 * i] : sb[4 * i]; },
      [&](bool a, int i, float zc, double, double, double, double w) { visit(a, i, zc, w); });
}

// raw2outputs' sums over a ray (:463-467) in merged order, with the depth moments about the first sample's z
struct RaySums {
  int s = 0;
  double shift = 0.0, acc = 0.0, m1 = 0.0, m2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  // rw: the sample's raw rgb
  __device__ __forceinline__ void add(const float *rw, float zc, double w) {
    if (s == 0) shift = zc;
    const double dz = (double)zc - shift;
    acc += w;
    m1 += w * dz;
    m2 += w * dz * dz;
    c0 += w / (1.0 + exp(-(double)rw[0]));
    c1 += w / (1.0 + exp(-(double)rw[1]));
    c2 += w / (1.0 + exp(-(double)rw[2]));
    ++s;
  }
  __device__ __forceinline__ double depth() const { return shift * acc + m1; }
  // sum w (z - depth)^2 with z - depth = dz - e, e = depth - shift
  __device__ __forceinline__ double var() const {
    const double e = depth() - shift;
    return m2 - 2.0 * e * m1 + e * e * acc;
  }
  // 1 / max(1e-10, depth / acc); a NaN quotient (acc 0) stays NaN, as torch.max keeps it
  __device__ __forceinline__ double disp() const {
    const double q = depth() / acc;
    return 1.0 / (q < 1e-10 ? 1e-10 : q);
  }
};

// The ray of pixel p = v W + u (get_rays as render :108-110 uses it): o = t, d = R [(u - cx) / fx, -(v - cy) / fy, -1],
// float32 in the reference's order.  camera: fx, fy, cx, cy, then c2w[:3, :4] row-major; ray[6] = o, d
__device__ __forceinline__ void pixel_ray(const float *__restrict__ camera, int W, int64_t p, float *__restrict__ ray) {
  const float u = (float)(p % W), v = (float)(p / W);
  const float fx = camera[0], fy = camera[1], cx = camera[2], cy = camera[3];
  const float *m = camera + 4;
  const float a = __fdiv_rn(__fsub_rn(u, cx), fx), b = -__fdiv_rn(__fsub_rn(v, cy), fy), c = -1.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ray[k] = m[4 * k + 3];
    ray[3 + k] = __fadd_rn(__fadd_rn(__fmul_rn(a, m[4 * k]), __fmul_rn(b, m[4 * k + 1])), __fmul_rn(c, m[4 * k + 2]));
  }
}

// raw2depth (:431-435) of one list: sg its sigma, 4 floats apart.  Two walks: the depth, then the variance about it
__device__ __forceinline__ void depth_and_var(const float *z, const float *sg, int S, double nd, double &depth, double &var) {
  depth = 0.0, var = 0.0;
  merged_walk(z, sg, S, nullptr, nullptr, 0, nd, [&](bool, int, float zv, double w) { depth += w * (double)zv; });
  const double d = depth;
  double v = 0.0;
  merged_walk(z, sg, S, nullptr, nullptr, 0, nd, [&](bool, int, float zv, double w) {
    const double dz = (double)zv - d;
    v += dz * dz * w;
  });
  var = v;
}

struct Bins {           // sample_3sigma (:471-478): edges and weights of the N - 1 bins between lo and hi, clamped to [near, far]
  double lo, hi, step, near, far;
  int N;
  __device__ __forceinline__ Bins(double lo_, double hi_, int n, double near_, double far_)
      : lo(lo_), hi(hi_), step((hi_ - lo_) / (double)(n - 1)), near(near_), far(far_), N(n) {}
  __device__ __forceinline__ double edge(int i) const {
    const double t = (double)i / (double)(N - 1);
    const double e = lo * (1.0 - t) + hi * t;
    return fmin(fmax(e, near), far);
  }
  __device__ __forceinline__ double weight(int i) const {       // factor * N(x_i) + the 1e-5 of sample_pdf
    const double x = N > 2 ? -3.0 + 6.0 * (double)i / (double)(N - 2) : -3.0;
    const double factor = (edge(i + 1) - edge(i)) / step;
    return factor * (0.3989422804014327 * exp(-0.5 * x * x)) + 1e-5;
  }
  __device__ __forceinline__ double total() const {
    double t = 0.0;
    for (int i = 0; i < N - 1; ++i) t += weight(i);
    return t;
  }
  // sample_pdf's sample at u between cdf entries below (value cb) and above (value ca)
  __device__ __forceinline__ float sample(double u, int below, double cb, int above, double ca) const {
    double denom = ca - cb;
    if (denom < 1e-5) denom = 1.0;
    const double tt = (u - cb) / denom;
    const double eb = edge(below);
    return (float)(eb + tt * (edge(above) - eb));
  }
};

// compute_samples_around_depth's range (:497-502) from raw2depth's moments, the std clamped below at lower_bound
__device__ __forceinline__ void range_around_depth(double depth, double var, double lower_bound, double &lo, double &hi) {
  const double std = fmax(sqrt(var), lower_bound);
  lo = depth - 3.0 * std, hi = depth + 3.0 * std;
}

// ... and its bins
__device__ __forceinline__ Bins bins_around_depth(double depth, double var, double lower_bound, int N, double near, double far) {
  double lo, hi;
  range_around_depth(depth, var, lower_bound, lo, hi);
  return Bins(lo, hi, N, near, far);
}

}  // namespace nerfray
