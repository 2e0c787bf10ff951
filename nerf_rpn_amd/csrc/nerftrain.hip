// The front end of a NeRF training step (nerf_train.py; reference data/scannet/run_nerf.py: get_ray_batch_from_one_image :650-670
// after the pixel draw, precompute_depth_sampling :159-162, perturb_z_vals :480-495, and the second sample list of render_rays at
// train time :588-592 = compute_samples_around_depth :497-502 / sample_3sigma :471-478 with the stochastic sample_pdf).
//
//   batch    one launch.  Thread i < R: the ray of pixel pix[i] (nerf_ray.cuh's pixel_ray, nerfrender_rays_kernel's bits), its unit view
//            direction (float64, rounded once), the gathers of image, depth and valid, depth_range = (d, d - 3 s, d + 3 s).  Thread i < R S: one element of the
//            perturbed list z1 = lower + (upper - lower) t_rand.  float32, the reference's operations in its order, no contraction.
//   samples  one launch, one thread per ray, float64 on the float32 inputs: the bins come from the given depth range where
//            depth_range[r][0] >= near and from the walk over (z1, sigma1) elsewhere -- decided per ray on the device; the ray's cdf is
//            a serial sum in bin order kept in the caller's scratch ([entry][ray], so that a wave's accesses to it are contiguous); every
//            u[r][j] is then located by bisection (searchsorted, right) and z2[r][j] written in u's order.  Bins, the walk and the
//            inverse-cdf expression are nerf_ray.cuh's, shared with nerfrender_sample_kernel: with u null (u_j = j / (S - 1)), no depth
//            range and a shared z1 the result is that kernel's, bit for bit.
// No atomics, no allocation, no host synchronisation; a ray's result depends on nothing but the ray.
#include "nerf_ray.cuh"

namespace {

using namespace nerfray;

constexpr int kBlock = 64;      // one wave: a ray's serial chain sets the time, and more waves per workgroup share nothing

struct BatchArgs {
  const float *camera;          // fx, fy, cx, cy, c2w[:3, :4]
  int H, W;
  const int *pix;               // [R]
  const float *image;           // [H][W][3]
  const float *depth;           // [H][W][2] or null
  const uint8_t *valid;         // [H][W] or null
  const float *z;               // [S] or null
  const float *t_rand;          // [R][S] or null
  int S;
  int64_t R;
  float *rays, *viewdirs, *target_s, *target_d, *depth_range, *z1;
  uint8_t *target_vd;
};

__global__ __launch_bounds__(kBlock) void nerftrain_batch_kernel(BatchArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < a.R) {
    int64_t p = a.pix[i];
    const int64_t last = (int64_t)a.H * a.W - 1;
    p = p < 0 ? 0 : p > last ? last : p;          // a pixel outside the image reads its nearest end, never outside the arrays
    float ray[6];
    pixel_ray(a.camera, a.W, p, ray);
    float *o = a.rays + i * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = ray[k];
    // render :127-132: viewdirs = rays_d / norm(rays_d), formed in float64 and rounded once: within half an ulp of the exact direction
    const float *d = ray + 3;
    const double n = ray_norm(d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.viewdirs[i * 3 + k] = (float)((double)d[k] / n);
      a.target_s[i * 3 + k] = a.image[p * 3 + k];
    }
    if (a.depth) {
      const float dm = a.depth[p * 2], ds = a.depth[p * 2 + 1];
      a.target_d[i * 2] = dm;
      a.target_d[i * 2 + 1] = ds;
      a.target_vd[i] = a.valid[p];
      a.depth_range[i * 3] = dm;
      a.depth_range[i * 3 + 1] = __fsub_rn(dm, __fmul_rn(3.0f, ds));
      a.depth_range[i * 3 + 2] = __fadd_rn(dm, __fmul_rn(3.0f, ds));
    }
  }
  if (a.t_rand && i < a.R * a.S) {
    const int s = (int)(i % a.S);
    const float zc = a.z[s];
    // mids = .5 (z[1:] + z[:-1]); upper = cat(mids, z[-1:]); lower = cat(z[:1], mids)
    const float up = s + 1 < a.S ? __fmul_rn(0.5f, __fadd_rn(a.z[s + 1], zc)) : zc;
    const float lo = s > 0 ? __fmul_rn(0.5f, __fadd_rn(zc, a.z[s - 1])) : zc;
    a.z1[i] = __fadd_rn(lo, __fmul_rn(__fsub_rn(up, lo), a.t_rand[i]));
  }
}

// kShared: z1 is one list for every ray, read through a wave-uniform pointer (scalar loads)
template <bool kShared>
__global__ __launch_bounds__(kBlock) void nerftrain_samples_kernel(const float *__restrict__ raw1, const float *__restrict__ z1,
                                                                   const float *__restrict__ rays, const float *__restrict__ depth_range,
                                                                   const float *__restrict__ u, int S, float lower_bound, float near,
                                                                   float far, int num_rays, double *__restrict__ cdf,
                                                                   float *__restrict__ z2) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= num_rays) return;
  double lo, hi;
  bool given = false;
  if (depth_range) {
    const float *dr = depth_range + (int64_t)r * 3;
    given = dr[0] >= near;
    lo = dr[1], hi = dr[2];
  }
  if (!given) {
    const float *za = kShared ? z1 : z1 + (int64_t)r * S;
    double depth, var;
    depth_and_var(za, raw1 + (int64_t)r * S * 4 + 3, S, ray_norm(rays + (int64_t)r * 6 + 3), depth, var);
    range_around_depth(depth, var, (double)lower_bound, lo, hi);
  }
  const Bins b(lo, hi, S, near, far);
  const double total = b.total();
  double *c = cdf + r;                  // entry k of this ray: c[k * num_rays]
  const int64_t ld = num_rays;
  double run = 0.0;
  c[0] = 0.0;
  for (int k = 1; k < S; ++k) {
    run = run + b.weight(k - 1) / total;
    c[k * ld] = run;
  }
  float *out = z2 + (int64_t)r * S;
  const float *ur = u ? u + (int64_t)r * S : nullptr;
  for (int j = 0; j < S; ++j) {
    const double uj = ur ? (double)ur[j] : (double)j / (double)(S - 1);
    int first = 0, n = S;               // k = number of cdf entries <= uj
    while (n > 0) {
      const int half = n >> 1;
      if (c[(first + half) * ld] <= uj) {
        first += half + 1;
        n -= half + 1;
      } else {
        n = half;
      }
    }
    const int below = first > 0 ? first - 1 : 0, above = first < S ? first : S - 1;
    out[j] = b.sample(uj, below, c[below * ld], above, c[above * ld]);
  }
}

constexpr int64_t kMaxTrainRays = (int64_t)1 << 31;

bool train_sizes_ok(int64_t num_rays, int S) { return S >= 2 && sizes_ok(num_rays, kMaxTrainRays, num_rays, S, S); }

}  // namespace

extern "C" {

int64_t nrpn_nerftrain_work_bytes(int64_t num_rays, int num_samples) {
  if (!train_sizes_ok(num_rays, num_samples)) return -1;
  return num_rays * num_samples * (int64_t)sizeof(double);
}

int nrpn_nerftrain_batch(const float *camera, int height, int width, const int *pix, int64_t num_rays, const float *image,
                         const float *depth, const uint8_t *valid, const float *z, const float *t_rand, int num_samples, float *rays,
                         float *viewdirs, float *target_s, float *target_d, uint8_t *target_vd, float *depth_range, float *z1,
                         nrpn_stream_t stream) {
  NRPN_REQUIRE(camera && pix && image && rays && viewdirs && target_s, "nerftrain_batch: null pointer");
  NRPN_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width < kMaxTrainRays, "nerftrain_batch: image %d x %d", height, width);
  NRPN_REQUIRE((depth != nullptr) == (valid != nullptr), "nerftrain_batch: depth and valid go together");
  NRPN_REQUIRE(!depth || (target_d && target_vd && depth_range), "nerftrain_batch: depth without target_d, target_vd or depth_range");
  NRPN_REQUIRE(!t_rand || (z && z1), "nerftrain_batch: t_rand without z or z1");
  const int S = t_rand ? num_samples : 1;
  NRPN_REQUIRE(!t_rand || num_samples >= 1, "nerftrain_batch: %d samples", num_samples);
  NRPN_REQUIRE(sizes_ok(num_rays, kMaxTrainRays, num_rays, S, 0), "nerftrain_batch: %lld rays with %d samples", (long long)num_rays, S);
  const BatchArgs a{camera, height, width, pix, image, depth, valid, z, t_rand, S, num_rays, rays, viewdirs, target_s, target_d,
                    depth_range, z1, target_vd};
  nerftrain_batch_kernel<<<(unsigned)cdiv64(num_rays * S, kBlock), kBlock, 0, as_stream(stream)>>>(a);
  NRPN_LAUNCH_CHECK("nerftrain_batch_kernel");
  return NRPN_OK;
}

int nrpn_nerftrain_samples(const float *raw1, const float *z1, int z1_stride, const float *rays, const float *depth_range,
                           const float *u, int num_samples, float lower_bound, float near, float far, int64_t num_rays, void *work,
                           int64_t work_bytes, float *z2, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw1 && z1 && rays && z2 && work, "nerftrain_samples: null pointer");
  NRPN_REQUIRE(train_sizes_ok(num_rays, num_samples), "nerftrain_samples: %lld rays with %d samples", (long long)num_rays, num_samples);
  NRPN_REQUIRE(z1_stride == 0 || z1_stride == num_samples, "nerftrain_samples: z1_stride %d is neither 0 nor %d", z1_stride, num_samples);
  NRPN_REQUIRE(near <= far, "nerftrain_samples: near %g above far %g", near, far);
  NRPN_REQUIRE(work_bytes >= nrpn_nerftrain_work_bytes(num_rays, num_samples), "nerftrain_samples: work buffer of %lld bytes is too small",
               (long long)work_bytes);
  const unsigned blocks = (unsigned)cdiv64(num_rays, kBlock);
  double *cdf = static_cast<double *>(work);
  if (z1_stride == 0)
    nerftrain_samples_kernel<true><<<blocks, kBlock, 0, as_stream(stream)>>>(raw1, z1, rays, depth_range, u, num_samples, lower_bound, near,
                                                                            far, (int)num_rays, cdf, z2);
  else
    nerftrain_samples_kernel<false><<<blocks, kBlock, 0, as_stream(stream)>>>(raw1, z1, rays, depth_range, u, num_samples, lower_bound,
                                                                             near, far, (int)num_rays, cdf, z2);
  NRPN_LAUNCH_CHECK("nerftrain_samples_kernel");
  return NRPN_OK;
}

}  // extern "C"
