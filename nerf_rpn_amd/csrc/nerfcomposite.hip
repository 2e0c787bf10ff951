// The ray stage of NeRF training as differentiable operations (ops.nerf_composite, ops.nerf_ray_losses; reference
// data/scannet/run_nerf.py: compute_weights :419-429, raw2outputs :437-469, forward_with_additonal_samples :504-512, the losses of
// train :837-847; compute_depth_loss of the fork as DESIGN.md 3.21 assumes it).
//
//   composite forward    one thread per ray: the merge of the two non-decreasing lists, weights, rgb / depth / acc / disp -- the walk and
//                        the sums of nerfrender_composite_kernel (nerf_ray.cuh), with an optional noise under the relu
//   composite backward   one thread per ray, two forward walks and nothing kept: the first adds up total = sum G_j w_j, the second
//                        carries prefix = sum_{j <= i} G_j w_j and gives d alpha_i = G_i T_i - (total - prefix) / (1 - alpha_i + 1e-10).
//                        T_i exists only going forward (dividing it back out of T_S fails once the 1e-10 floor has underflowed it), so
//                        a reverse walk would need T per sample kept; the subtraction's error, 2^-53 sum |G w|, reaches d sigma
//                        times dist (1 - alpha) / (1 - alpha + 1e-10) <= dist and is far below the float32 result's rounding
//   losses forward       one thread per ray: its squared colour error and its Gaussian NLL term in float64, then one workgroup adds the
//                        rays in a fixed order
//   losses backward      one thread per ray: the term again from the same inputs -> g_rgb, g_depth, g_w
// Everything after the float32 inputs is float64; no atomics; repeated calls are bit-equal.  No FMA contraction, as in nerfrender.hip:
// the forward's bits are that kernel's.
#include "nerf_ray.cuh"

namespace {

using namespace nerfray;

constexpr int64_t kMaxRays = (int64_t)1 << 31;
constexpr int kSumThreads = 256;

struct Lists {            // a ray's two sample lists
  const float *raw1, *z1;       // [rays][S1][4]; [S1] (z1_stride 0) or [rays][S1]
  const float *raw2, *z2;       // [rays][S2][4], [rays][S2]
  const float *noise1, *noise2; // [rays][S1], [rays][S2], or both null
  const float *rays_d;          // [rays][3]
  int z1_stride, S1, S2, num_rays;
};

struct RayLists {         // of ray r
  const float *za, *zb, *ra, *rb, *na, *nb;
  double nd;
  __device__ __forceinline__ RayLists(const Lists &l, int r)
      : za(l.z1 + (int64_t)r * l.z1_stride), zb(l.z2 + (int64_t)r * l.S2), ra(l.raw1 + (int64_t)r * l.S1 * 4),
        rb(l.raw2 + (int64_t)r * l.S2 * 4), na(l.noise1 ? l.noise1 + (int64_t)r * l.S1 : nullptr),
        nb(l.noise1 ? l.noise2 + (int64_t)r * l.S2 : nullptr), nd(ray_norm(l.rays_d + (int64_t)r * 3)) {}
  // raw[..., 3] + noise (:426), the sum in float64
  __device__ __forceinline__ double sigma(bool a, int i) const {
    const double s = a ? ra[4 * i + 3] : rb[4 * i + 3];
    return na ? s + (double)(a ? na[i] : nb[i]) : s;
  }
  __device__ __forceinline__ const float *rgb(bool a, int i) const { return a ? ra + 4 * i : rb + 4 * i; }
};

struct MapsOut {
  float *rgb, *depth, *acc, *disp;      // [rays][3], [rays] x 3
  float *weights, *z_vals;              // [rays][S1 + S2]
};

__global__ __launch_bounds__(64) void nerfcomposite_forward_kernel(Lists l, MapsOut o) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= l.num_rays) return;
  const RayLists q(l, r);
  const int64_t row = (int64_t)r * (l.S1 + l.S2);
  RaySums sums;
  merged_walk_sigma<double>(
      q.za, l.S1, q.zb, l.S2, q.nd, [&](bool a, int i) { return q.sigma(a, i); },
      [&](bool a, int i, float zc, double, double, double, double w) {
        const int s = sums.s;
        sums.add(q.rgb(a, i), zc, w);
        o.z_vals[row + s] = zc;
        o.weights[row + s] = (float)w;
      });
  o.rgb[(int64_t)r * 3] = (float)sums.c0;
  o.rgb[(int64_t)r * 3 + 1] = (float)sums.c1;
  o.rgb[(int64_t)r * 3 + 2] = (float)sums.c2;
  o.depth[r] = (float)sums.depth();
  o.acc[r] = (float)sums.acc;
  o.disp[r] = (float)sums.disp();
}

struct Cotangents {       // of rgb_map [rays][3], depth_map [rays], acc_map [rays], weights [rays][S1 + S2]; each may be null
  const float *rgb, *depth, *acc, *w;
};

__device__ __forceinline__ double sigmoid(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

// draw1 [rays][S1][4], draw2 [rays][S2][4]: every entry is written
__global__ __launch_bounds__(64) void nerfcomposite_backward_kernel(Lists l, Cotangents g, float *__restrict__ draw1,
                                                                    float *__restrict__ draw2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= l.num_rays) return;
  const RayLists q(l, r);
  const int64_t row = (int64_t)r * (l.S1 + l.S2);
  double gc[3] = {0.0, 0.0, 0.0};
  if (g.rgb)
    for (int c = 0; c < 3; ++c) gc[c] = g.rgb[(int64_t)r * 3 + c];
  const double gd = g.depth ? (double)g.depth[r] : 0.0, ga = g.acc ? (double)g.acc[r] : 0.0;
  // G of the sample at merged position s
  auto big_g = [&](int s, const float *rw, float zc) {
    const double gw = g.w ? (double)g.w[row + s] : 0.0;
    return ((gw + ((gc[0] * sigmoid(rw[0]) + gc[1] * sigmoid(rw[1])) + gc[2] * sigmoid(rw[2]))) + gd * (double)zc) + ga;
  };
  auto load = [&](bool a, int i) { return q.sigma(a, i); };
  double total = 0.0;
  int s = 0;
  merged_walk_sigma<double>(q.za, l.S1, q.zb, l.S2, q.nd, load, [&](bool a, int i, float zc, double, double, double, double w) {
    total += big_g(s, q.rgb(a, i), zc) * w;
    ++s;
  });
  double prefix = 0.0;
  s = 0;
  float *da = draw1 + (int64_t)r * l.S1 * 4, *db = draw2 + (int64_t)r * l.S2 * 4;
  merged_walk_sigma<double>(q.za, l.S1, q.zb, l.S2, q.nd, load,
                            [&](bool a, int i, float zc, double sg, double dist, double T, double w) {
                              const float *rw = q.rgb(a, i);
                              const double G = big_g(s, rw, zc);
                              prefix += G * w;
                              const double e = exp(-fmax(sg, 0.0) * dist), alpha = 1.0 - e;      // as sample_weight has them
                              const double dalpha = G * T - (total - prefix) / (1.0 - alpha + 1e-10);
                              float *d = a ? da + 4 * i : db + 4 * i;
                              for (int c = 0; c < 3; ++c) {
                                const double sc = sigmoid(rw[c]);
                                d[c] = (float)(gc[c] * w * (sc * (1.0 - sc)));
                              }
                              d[3] = sg > 0.0 ? (float)(dalpha * dist * e) : 0.f;
                              ++s;
                            });
}

// ---- losses ----------------------------------------------------------------------------------------------------------------------
struct LossIn {
  const float *rgb, *target_s;          // [rays][3]
  const float *depth, *z_vals, *weights, *target_d;      // [rays], [rays][S] x 2, [rays][2] (mean, std); null without a depth loss
  const uint8_t *target_vd;             // [rays], non-zero = the ray has a depth target
  int num_rays, S;
};

struct DepthTerm {        // compute_depth_loss for one ray
  bool applied;
  double m, t, v, vc, dvdm;      // dvdm = -2 sum (z - m) w
  __device__ __forceinline__ DepthTerm(const LossIn &in, int r) : applied(false), m(0.0), t(0.0), v(0.0), vc(0.0), dvdm(0.0) {
    if (!in.target_d || !in.target_vd[r]) return;
    m = in.depth[r];
    const float *z = in.z_vals + (int64_t)r * in.S, *w = in.weights + (int64_t)r * in.S;
    double sum = 0.0, lin = 0.0;
    for (int i = 0; i < in.S; ++i) {
      const double dz = (double)z[i] - m;
      sum += dz * dz * (double)w[i];
      lin += dz * (double)w[i];
    }
    v = sum + 1e-5;
    dvdm = -2.0 * lin;
    t = in.target_d[(int64_t)r * 2];
    const double sd = in.target_d[(int64_t)r * 2 + 1];
    applied = fabs(m - t) - sd > 0.0 || sd * sd < v;
    vc = fmax(v, 1e-3);
  }
  __device__ __forceinline__ double nll() const { return 0.5 * (log(vc) + (m - t) * (m - t) / vc); }
};

// terms f64 [rays][2]: the ray's sum of squared colour errors; its Gaussian NLL, 0 unless applied
__global__ __launch_bounds__(64) void nerfraylosses_terms_kernel(LossIn in, double *__restrict__ terms) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= in.num_rays) return;
  double e2 = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double e = (double)in.rgb[(int64_t)r * 3 + c] - (double)in.target_s[(int64_t)r * 3 + c];
    e2 += e * e;
  }
  const DepthTerm d(in, r);
  terms[(int64_t)r * 2] = e2;
  terms[(int64_t)r * 2 + 1] = d.applied ? d.nll() : 0.0;
}

// One workgroup: thread t adds rays t, t + 256, .. in order, then a pairwise tree over the threads.  losses f32 [2]: img_loss =
// sum / (3 rays), depth_loss = sum / rays
__global__ __launch_bounds__(kSumThreads) void nerfraylosses_sum_kernel(const double *__restrict__ terms, int num_rays,
                                                                        float *__restrict__ losses) {
  __shared__ double part[2][kSumThreads];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int r = t; r < num_rays; r += kSumThreads) {
    a += terms[(int64_t)r * 2];
    b += terms[(int64_t)r * 2 + 1];
  }
  part[0][t] = a;
  part[1][t] = b;
  __syncthreads();
  for (int step = kSumThreads / 2; step > 0; step >>= 1) {
    if (t < step) {
      part[0][t] += part[0][t + step];
      part[1][t] += part[1][t + step];
    }
    __syncthreads();
  }
  if (t == 0) {
    losses[0] = (float)(part[0][0] / (3.0 * (double)num_rays));
    losses[1] = (float)(part[1][0] / (double)num_rays);
  }
}

// g_losses f32 [2]: the cotangents of img_loss and depth_loss -> g_rgb [rays][3]; g_depth [rays] and g_w [rays][S] (with a depth loss)
__global__ __launch_bounds__(64) void nerfraylosses_backward_kernel(LossIn in, const float *__restrict__ g_losses, float *__restrict__ g_rgb,
                                                                    float *__restrict__ g_depth, float *__restrict__ g_w) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= in.num_rays) return;
  const double gi = (double)g_losses[0] * 2.0 / (3.0 * (double)in.num_rays);
  for (int c = 0; c < 3; ++c)
    g_rgb[(int64_t)r * 3 + c] = (float)(gi * ((double)in.rgb[(int64_t)r * 3 + c] - (double)in.target_s[(int64_t)r * 3 + c]));
  if (!in.target_d) return;
  const DepthTerm d(in, r);
  float *gw = g_w + (int64_t)r * in.S;
  if (!d.applied) {
    g_depth[r] = 0.f;
    for (int i = 0; i < in.S; ++i) gw[i] = 0.f;
    return;
  }
  const double gl = (double)g_losses[1] / (double)in.num_rays, e = d.m - d.t;
  const double dv = gl * 0.5 * (1.0 / d.vc - e * e / (d.vc * d.vc));      // the clamp passes the gradient of v through, as torch's does
  g_depth[r] = (float)(gl * e / d.vc + dv * d.dvdm);
  const float *z = in.z_vals + (int64_t)r * in.S;
  for (int i = 0; i < in.S; ++i) {
    const double dz = (double)z[i] - d.m;
    gw[i] = (float)(dv * (dz * dz));
  }
}

int check_lists(const char *who, const Lists &l) {
  NRPN_REQUIRE(sizes_ok(l.num_rays, kMaxRays, l.num_rays, l.S1, l.S2), "%s: %d rays with %d + %d samples", who, l.num_rays, l.S1, l.S2);
  NRPN_REQUIRE(l.raw1 && l.z1 && l.rays_d && (l.S2 == 0 || (l.raw2 && l.z2)), "%s: null pointer", who);
  NRPN_REQUIRE(l.z1_stride == 0 || l.z1_stride == l.S1, "%s: z1 stride %d with %d samples", who, l.z1_stride, l.S1);
  NRPN_REQUIRE(!l.noise1 == !l.noise2 || l.S2 == 0, "%s: noise for one list only", who);
  return NRPN_OK;
}

Lists make_lists(const float *raw1, const float *z1, int z1_stride, int s1, const float *raw2, const float *z2, int s2,
                 const float *noise1, const float *noise2, const float *rays_d, int64_t num_rays) {
  // without a second list its pointers are never read: they alias the first so that none is null in the kernel
  return Lists{raw1, z1, s2 ? raw2 : raw1, s2 ? z2 : z1, noise1, s2 ? noise2 : noise1, rays_d, z1_stride, s1, s2,
               (int)(num_rays < kMaxRays ? num_rays : 0)};
}

int check_loss(const char *who, const LossIn &in, int64_t num_rays, int num_samples) {
  NRPN_REQUIRE(sizes_ok(num_rays, kMaxRays, num_rays, (num_samples + 1) / 2, num_samples / 2), "%s: %lld rays with %d samples", who, (long long)num_rays,
               num_samples);
  NRPN_REQUIRE(in.rgb && in.target_s, "%s: null pointer", who);
  NRPN_REQUIRE(!in.target_d || (in.depth && in.z_vals && in.weights && in.target_vd), "%s: a depth target without depth_map, z_vals, weights or target_vd",
               who);
  return NRPN_OK;
}

int blocks_of(int num_rays) { return (num_rays + 63) / 64; }

}  // namespace

extern "C" {

int64_t nrpn_nerfcomposite_work_bytes(int64_t num_rays, int s1, int s2) {
  if (!sizes_ok(num_rays, kMaxRays, num_rays, s1, s2)) return -1;
  return num_rays * 2 * (int64_t)sizeof(double);
}

int nrpn_nerfcomposite_forward(const float *raw1, const float *z1, int z1_stride, int s1, const float *raw2, const float *z2, int s2,
                               const float *noise1, const float *noise2, const float *rays_d, int64_t num_rays, float *rgb_map,
                               float *depth_map, float *acc_map, float *disp_map, float *weights, float *z_vals, nrpn_stream_t stream) {
  const Lists l = make_lists(raw1, z1, z1_stride, s1, raw2, z2, s2, noise1, noise2, rays_d, num_rays);
  NRPN_REQUIRE(num_rays < kMaxRays, "nerfcomposite_forward: %lld rays", (long long)num_rays);
  if (int rc = check_lists("nerfcomposite_forward", l)) return rc;
  NRPN_REQUIRE(rgb_map && depth_map && acc_map && disp_map && weights && z_vals, "nerfcomposite_forward: null output");
  nerfcomposite_forward_kernel<<<blocks_of(l.num_rays), 64, 0, as_stream(stream)>>>(l, MapsOut{rgb_map, depth_map, acc_map, disp_map,
                                                                                               weights, z_vals});
  NRPN_LAUNCH_CHECK("nerfcomposite_forward_kernel");
  return NRPN_OK;
}

int nrpn_nerfcomposite_backward(const float *raw1, const float *z1, int z1_stride, int s1, const float *raw2, const float *z2, int s2,
                                const float *noise1, const float *noise2, const float *rays_d, int64_t num_rays, const float *g_rgb,
                                const float *g_depth, const float *g_acc, const float *g_w, float *draw1, float *draw2,
                                nrpn_stream_t stream) {
  const Lists l = make_lists(raw1, z1, z1_stride, s1, raw2, z2, s2, noise1, noise2, rays_d, num_rays);
  NRPN_REQUIRE(num_rays < kMaxRays, "nerfcomposite_backward: %lld rays", (long long)num_rays);
  if (int rc = check_lists("nerfcomposite_backward", l)) return rc;
  NRPN_REQUIRE(draw1 && (s2 == 0 || draw2), "nerfcomposite_backward: null output");
  nerfcomposite_backward_kernel<<<blocks_of(l.num_rays), 64, 0, as_stream(stream)>>>(l, Cotangents{g_rgb, g_depth, g_acc, g_w}, draw1,
                                                                                     s2 ? draw2 : draw1);
  NRPN_LAUNCH_CHECK("nerfcomposite_backward_kernel");
  return NRPN_OK;
}

int nrpn_nerfraylosses_forward(const float *rgb_map, const float *target_s, const float *depth_map, const float *z_vals,
                               const float *weights, const float *target_d, const uint8_t *target_vd, int64_t num_rays, int num_samples,
                               void *work, int64_t work_bytes, float *losses, nrpn_stream_t stream) {
  const LossIn in{rgb_map, target_s, depth_map, z_vals, weights, target_d, target_vd, (int)(num_rays < kMaxRays ? num_rays : 0), num_samples};
  if (int rc = check_loss("nerfraylosses_forward", in, num_rays, num_samples)) return rc;
  NRPN_REQUIRE(work && losses && work_bytes >= num_rays * 2 * (int64_t)sizeof(double), "nerfraylosses_forward: null pointer, or a work buffer of %lld bytes",
               (long long)work_bytes);
  double *terms = static_cast<double *>(work);
  nerfraylosses_terms_kernel<<<blocks_of(in.num_rays), 64, 0, as_stream(stream)>>>(in, terms);
  NRPN_LAUNCH_CHECK("nerfraylosses_terms_kernel");
  nerfraylosses_sum_kernel<<<1, kSumThreads, 0, as_stream(stream)>>>(terms, in.num_rays, losses);
  NRPN_LAUNCH_CHECK("nerfraylosses_sum_kernel");
  return NRPN_OK;
}

int nrpn_nerfraylosses_backward(const float *rgb_map, const float *target_s, const float *depth_map, const float *z_vals,
                                const float *weights, const float *target_d, const uint8_t *target_vd, int64_t num_rays,
                                int num_samples, const float *g_losses, float *g_rgb, float *g_depth, float *g_w, nrpn_stream_t stream) {
  const LossIn in{rgb_map, target_s, depth_map, z_vals, weights, target_d, target_vd, (int)(num_rays < kMaxRays ? num_rays : 0), num_samples};
  if (int rc = check_loss("nerfraylosses_backward", in, num_rays, num_samples)) return rc;
  NRPN_REQUIRE(g_losses && g_rgb && (!target_d || (g_depth && g_w)), "nerfraylosses_backward: null pointer");
  nerfraylosses_backward_kernel<<<blocks_of(in.num_rays), 64, 0, as_stream(stream)>>>(in, g_losses, g_rgb, g_depth, g_w);
  NRPN_LAUNCH_CHECK("nerfraylosses_backward_kernel");
  return NRPN_OK;
}

}  // extern "C"
