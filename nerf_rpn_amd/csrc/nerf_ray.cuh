// The per-ray float64 arithmetic of compute_weights and raw2outputs (data/scannet/run_nerf.py:419-469) over the merge of a ray's
// two non-decreasing sample lists (forward_with_additonal_samples :504-512), shared by nerfrender.hip (views, the camera-embedding
// objective) and nerfcomposite.hip (the differentiable ray stage): one definition, so the two give the same bits.
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

}  // namespace nerfray
