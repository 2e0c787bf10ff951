// Views of a trained NeRF MLP (scripts/nerf_render.py; reference data/scannet/run_nerf.py: render :82-157, render_rays :514-614,
// compute_samples_around_depth :497-502, forward_with_additonal_samples :504-512, raw2outputs :437-469, render_video :184-185).
//
// Per chunk of rays:
//   rays     (frame mode) o = t, d = R [(u - cx) / fx, -(v - cy) / fy, -1] of pixel r = v W + u, float32 in the reference's order
//   trunk    the shared MFMA trunk (nerf_mlp.cuh) over the points o_r + d_r z[r][s] -> raw sigma and g
//   head     one thread per point: v = relu(g + c_r), raw rgb = W_rgb v + b_rgb; c_r = W_d embed_dirs(d_r / |d_r|) + W_c cam + b is
//            computed per ray of the tile in LDS
//   sample   (two-pass) one thread per ray: weights of pass 1 -> depth, std -> clamped +-3 sigma bins -> inverse CDF at linspace(0, 1)
//   trunk + head again over z2, then
//   composite  one thread per ray: merge of the two non-decreasing lists, weights, rgb / depth / acc / disp / depth_std
// The per-ray reductions (sample, composite) run in float64 on the float32 raw and z values: they are a few hundred operations per
// sample next to the 1.2 MFLOP of its MLP query, and the result then carries no summation-order error of its own.  Point positions are
// float32 with the reference's operation order and no contraction (they feed sinf(2^8 p)).  No atomics; a ray's result does not
// depend on its chunk or on the tiles its samples fall into.
#include "nerf_mlp.cuh"

namespace {

using namespace nerfmlp;

constexpr int kMaxViewsCh = 64;       // 3 + 6 multires_views <= 64 (multires_views <= 10)
constexpr int kCtileLd = kHalf + 1;   // bank skew between the rays of a head tile

struct RayPoints {
  const float *rays;      // [rays of the chunk][6]: o, d
  const float *z;         // [S] (z_stride 0) or [rays of the chunk][S] (z_stride S)
  int z_stride, S;
  int64_t num_points;     // rays of the chunk * S
  float cx, cy, cz, scale;
};

// ---- rays ------------------------------------------------------------------------------------------------------------------------
// camera: fx, fy, cx, cy, then c2w[:3, :4] row-major
__global__ void nerfrender_rays_kernel(const float *__restrict__ camera, int W, int64_t ray0, int count, float *__restrict__ rays) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t r = ray0 + i;
  const float u = (float)(r % W), v = (float)(r / W);
  const float fx = camera[0], fy = camera[1], cx = camera[2], cy = camera[3];
  const float *m = camera + 4;
  const float a = __fdiv_rn(__fsub_rn(u, cx), fx), b = -__fdiv_rn(__fsub_rn(v, cy), fy), c = -1.0f;
  float *o = rays + (int64_t)i * 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = m[4 * k + 3];
    o[3 + k] = __fadd_rn(__fadd_rn(__fmul_rn(a, m[4 * k]), __fmul_rn(b, m[4 * k + 1])), __fmul_rn(c, m[4 * k + 2]));
  }
}

// ---- trunk -----------------------------------------------------------------------------------------------------------------------
struct RaySrc {
  const RayPoints &rp;
  int64_t tile0;
  __device__ __forceinline__ void point(int i, float (&p)[3]) const {
    int64_t pi = tile0 + i;
    if (pi > rp.num_points - 1) pi = rp.num_points - 1;       // a partial tile repeats the last point; nothing of it is stored
    const int64_t ray = pi / rp.S;
    const int s = (int)(pi - ray * rp.S);
    const float zv = rp.z[ray * rp.z_stride + s];
    const float *o = rp.rays + ray * 6;
    const float c[3] = {rp.cx, rp.cy, rp.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fmul_rn(__fsub_rn(__fadd_rn(o[a], __fmul_rn(o[3 + a], zv)), c[a]), rp.scale);
  }
};
struct RaySink {
  int64_t tile0, num_points;
  float *raw;
  __device__ __forceinline__ void sigma(int i, float s) const {
    const int64_t pi = tile0 + i;
    if (pi < num_points) raw[pi * 4 + 3] = s;
  }
};

__global__ __launch_bounds__(256) void nerfrender_trunk_kernel(RayPoints rp, int multires, const float *__restrict__ packed,
                                                               float *__restrict__ gbuf, float *__restrict__ raw) {
  extern __shared__ __align__(16) float act[];
  const int64_t tile0 = (int64_t)blockIdx.x * kTile;
  trunk_body(act, packed, multires, 3 + 6 * multires, RaySrc{rp, tile0}, RaySink{tile0, rp.num_points, raw},
             gbuf + (int64_t)blockIdx.x * (kTile * kHalf));
}

// ---- head ------------------------------------------------------------------------------------------------------------------------
// rgb_linear over v = relu(g + c) for one point: g the point's 128 trunk outputs in registers, c[j] the view part of its ray.
// 128-term fmaf chains in j order; W_rgb is wave-uniform and comes through the scalar cache.
__device__ __forceinline__ void rgb_head(const float (&g)[kHalf], const float *c, const float *__restrict__ w, float &r0, float &r1,
                                         float &r2) {
  r0 = r1 = r2 = 0.f;
#pragma unroll
  for (int j = 0; j < kHalf; ++j) {
    const float v = fmaxf(g[j] + c[j], 0.f);
    r0 = fmaf(w[j], v, r0);
    r1 = fmaf(w[kHalf + j], v, r1);
    r2 = fmaf(w[2 * kHalf + j], v, r2);
  }
}

// w_view [128][views_ch + cam_ch]: the view and camera columns of views_linears.0.weight; b_view [128]; cam [cam_ch]
__global__ __launch_bounds__(kTile) void nerfrender_head_kernel(RayPoints rp, const float *__restrict__ packed,
                                                                const float *__restrict__ w_view, const float *__restrict__ b_view,
                                                                const float *__restrict__ cam, int multires_views, int cam_ch,
                                                                const float *__restrict__ gbuf, float *__restrict__ raw) {
  __shared__ float emb[kTile][kMaxViewsCh];
  __shared__ float cbase[kHalf];
  __shared__ float ctile[kTile * kCtileLd];
  const int t = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * kTile;
  const int64_t last = tile0 + kTile - 1 < rp.num_points ? tile0 + kTile - 1 : rp.num_points - 1;
  const int64_t ray_first = tile0 / rp.S;
  const int nr = (int)(last / rp.S - ray_first) + 1;          // rays with a sample in this tile: 1 .. 64
  const int views_ch = 3 + 6 * multires_views, ldv = views_ch + cam_ch;

  for (int j = t; j < kHalf; j += kTile) {
    float c = b_view[j];
    for (int k = 0; k < cam_ch; ++k) c = fmaf(w_view[j * ldv + views_ch + k], cam[k], c);
    cbase[j] = c;
  }
  if (t < nr) {
    const float *d = rp.rays + (ray_first + t) * 6 + 3;
    const float n = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
    const float vd[3] = {__fdiv_rn(d[0], n), __fdiv_rn(d[1], n), __fdiv_rn(d[2], n)};
    for (int a = 0; a < 3; ++a) emb[t][a] = vd[a];
    for (int l = 0; l < multires_views; ++l)
      for (int a = 0; a < 3; ++a) {
        const float arg = vd[a] * ldexpf(1.0f, l);
        emb[t][3 + 6 * l + a] = sinf(arg);
        emb[t][3 + 6 * l + 3 + a] = cosf(arg);
      }
  }
  __syncthreads();
  for (int idx = t; idx < nr * kHalf; idx += kTile) {
    const int ray = idx / kHalf, j = idx - ray * kHalf;
    float c = cbase[j];
    for (int k = 0; k < views_ch; ++k) c = fmaf(w_view[j * ldv + k], emb[ray][k], c);
    ctile[ray * kCtileLd + j] = c;
  }
  __syncthreads();

  const int64_t pi = tile0 + t;
  const int64_t pc = pi < rp.num_points ? pi : rp.num_points - 1;
  const float *crow = ctile + (int)(pc / rp.S - ray_first) * kCtileLd;
  const float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + t;
  float g[kHalf];
#pragma unroll
  for (int j = 0; j < kHalf; ++j) g[j] = gt[j * kTile];
  float r0, r1, r2;
  rgb_head(g, crow, packed + kOffRgbW, r0, r1, r2);
  if (pi < rp.num_points) {
    float *o = raw + pi * 4;
    o[0] = r0 + packed[kOffRgbB];
    o[1] = r1 + packed[kOffRgbB + 1];
    o[2] = r2 + packed[kOffRgbB + 2];
  }
}

// ---- per-ray reductions, float64 ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double ray_norm(const float *d) {
  const double x = d[0], y = d[1], z = d[2];
  return sqrt(x * x + y * y + z * z);
}

// compute_weights (:419-429) for one sample: alpha from relu(sigma) and dist; T is the transmittance before it and is advanced
__device__ __forceinline__ double sample_weight(float sigma, double dist, double &T) {
  const double alpha = 1.0 - exp(-fmax((double)sigma, 0.0) * dist);
  const double w = alpha * T;
  T *= 1.0 - alpha + 1e-10;
  return w;
}

struct Bins {           // sample_3sigma (:471-478): edges and weights of the N - 1 bins between depth -+ 3 std, clamped to [near, far]
  double lo, hi, step, near, far;
  int N;
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
};

// raw [rays][S][4], z [S] shared, rays [rays][6] -> z2 [rays][S]
__global__ void nerfrender_sample_kernel(const float *__restrict__ raw, const float *__restrict__ rays, const float *__restrict__ z, int S,
                                         float near, float far, int num_rays, float *__restrict__ z2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const double nd = ray_norm(rays + (int64_t)r * 6 + 3);
  const float *sg = raw + (int64_t)r * S * 4 + 3;
  double T = 1.0, depth = 0.0;
  for (int s = 0; s < S; ++s) {
    const double dist = (s + 1 < S ? (double)z[s + 1] - (double)z[s] : 1e10) * nd;
    depth += sample_weight(sg[4 * s], dist, T) * (double)z[s];
  }
  T = 1.0;
  double var = 0.0;
  for (int s = 0; s < S; ++s) {
    const double dist = (s + 1 < S ? (double)z[s + 1] - (double)z[s] : 1e10) * nd;
    const double dz = (double)z[s] - depth;
    var += dz * dz * sample_weight(sg[4 * s], dist, T);
  }
  const double std = fmax(sqrt(var), (double)z[S - 1] - (double)z[S - 2]);
  Bins b;
  b.lo = depth - 3.0 * std, b.hi = depth + 3.0 * std, b.N = S, b.near = near, b.far = far;
  b.step = (b.hi - b.lo) / (double)(S - 1);
  double total = 0.0;
  for (int i = 0; i < S - 1; ++i) total += b.weight(i);
  // inverse CDF at u_j = j / (S - 1) (deterministic sample_pdf): k = number of cdf entries <= u (searchsorted, right), cb = cdf[k - 1],
  // ca = cdf[k]; both u and the cdf are non-decreasing, so k only moves forward
  int k = 1;
  double cb = 0.0, ca = b.weight(0) / total;
  float *out = z2 + (int64_t)r * S;
  for (int j = 0; j < S; ++j) {
    const double u = (double)j / (double)(S - 1);
    while (k < S && ca <= u) {
      cb = ca;
      ++k;
      if (k < S) ca = cb + b.weight(k - 1) / total;
    }
    const int below = k - 1, above = k < S ? k : S - 1;
    const double c_above = k < S ? ca : cb;
    double denom = c_above - cb;
    if (denom < 1e-5) denom = 1.0;
    const double tt = (u - cb) / denom;
    const double eb = b.edge(below);
    out[j] = (float)(eb + tt * (b.edge(above) - eb));
  }
}

struct CompositeOut {
  float *rgb, *depth, *acc, *disp, *depth_std;      // [rays][3], [rays] x 4
  float *z_vals, *weights;                          // [rays][S1 + S2] or null
};

// raw1 [rays][S1][4] at z1 (z1_stride 0: shared), raw2 [rays][S2][4] at z2 [rays][S2] (S2 may be 0): merge, weights, maps
__global__ void nerfrender_composite_kernel(const float *__restrict__ raw1, const float *__restrict__ z1, int z1_stride, int S1,
                                            const float *__restrict__ raw2, const float *__restrict__ z2, int S2,
                                            const float *__restrict__ rays, int num_rays, int64_t ray0, CompositeOut o) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const double nd = ray_norm(rays + (int64_t)r * 6 + 3);
  const float *za = z1 + (int64_t)r * z1_stride, *zb = z2 + (int64_t)r * S2;
  const float *ra = raw1 + (int64_t)r * S1 * 4, *rb = raw2 + (int64_t)r * S2 * 4;
  const int S = S1 + S2;
  const int64_t gr = ray0 + r;
  int ia = 0, ib = 0;
  // the current sample: the smaller head of the two lists, list 1 first on a tie
  auto take = [&](const float *&rw) {
    const bool a = ib >= S2 || (ia < S1 && za[ia] <= zb[ib]);
    const float zv = a ? za[ia] : zb[ib];
    rw = a ? ra + 4 * ia : rb + 4 * ib;
    a ? ++ia : ++ib;
    return zv;
  };
  const float *rw;
  float zc = take(rw);
  const double shift = zc;
  double T = 1.0, acc = 0.0, m1 = 0.0, m2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const float *rnext = rw;
    const float zn = s + 1 < S ? take(rnext) : zc;
    const double dist = (s + 1 < S ? (double)zn - (double)zc : 1e10) * nd;
    const double w = sample_weight(rw[3], dist, T);
    const double dz = (double)zc - shift;
    acc += w;
    m1 += w * dz;
    m2 += w * dz * dz;
    c0 += w / (1.0 + exp(-(double)rw[0]));
    c1 += w / (1.0 + exp(-(double)rw[1]));
    c2 += w / (1.0 + exp(-(double)rw[2]));
    if (o.z_vals) o.z_vals[gr * S + s] = zc;
    if (o.weights) o.weights[gr * S + s] = (float)w;
    zc = zn;
    rw = rnext;
  }
  const double depth = shift * acc + m1;
  // sum w (z - depth)^2 with z - depth = dz - e, e = depth - shift
  const double e = depth - shift;
  const double var = m2 - 2.0 * e * m1 + e * e * acc;
  const double q = depth / acc;
  o.rgb[gr * 3] = (float)c0;
  o.rgb[gr * 3 + 1] = (float)c1;
  o.rgb[gr * 3 + 2] = (float)c2;
  o.depth[gr] = (float)depth;
  o.acc[gr] = (float)acc;
  o.disp[gr] = (float)(1.0 / (q < 1e-10 ? 1e-10 : q));          // a NaN quotient (acc 0) stays NaN, as torch.max keeps it
  o.depth_std[gr] = (float)sqrt(fmin(fmax(var, 0.0), 1.0));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Layout {           // of the work buffer, in bytes; every part 16-byte aligned
  int64_t rays, raw1, raw2, z2, gbuf, total;
};
Layout work_layout(int64_t chunk, int s1, int s2) {
  auto al = [](int64_t b) { return (b + 15) / 16 * 16; };
  Layout l{};
  const int smax = s1 > s2 ? s1 : s2;
  l.rays = 0;
  l.raw1 = l.rays + al(chunk * 6 * 4);
  l.raw2 = l.raw1 + al(chunk * s1 * 16);
  l.z2 = l.raw2 + al(chunk * s2 * 16);
  l.gbuf = l.z2 + al(chunk * s2 * 4);
  l.total = l.gbuf + cdiv64(chunk * smax, kTile) * kTile * kHalf * 4;
  return l;
}

struct RenderCall {
  const float *rays, *camera;       // one of them
  int W;
  int64_t num_rays;
  float near, far, cx, cy, cz, scale;
  int multires, multires_views, cam_ch;
  const float *packed, *w_view, *b_view, *cam, *z1;
  int s1, z2_mode;
  const float *z2_in;
  int s2;
  int64_t chunk;
  void *work;
  int64_t work_bytes;
  CompositeOut out;
  float *raw1_out, *z2_out;
  hipStream_t stream;
};

int mlp_pass(const RenderCall &c, RayPoints rp, float *gbuf, float *raw) {
  const int tiles = (int)cdiv64(rp.num_points, kTile);
  nerfrender_trunk_kernel<<<tiles, 256, kLdsBytes, c.stream>>>(rp, c.multires, c.packed, gbuf, raw);
  NRPN_LAUNCH_CHECK("nerfrender_trunk_kernel");
  nerfrender_head_kernel<<<tiles, kTile, 0, c.stream>>>(rp, c.packed, c.w_view, c.b_view, c.cam, c.multires_views, c.cam_ch, gbuf, raw);
  NRPN_LAUNCH_CHECK("nerfrender_head_kernel");
  return NRPN_OK;
}

int render(const RenderCall &c) {
  NRPN_REQUIRE(c.packed && c.w_view && c.b_view && c.z1 && c.work, "nerfrender: null pointer");
  NRPN_REQUIRE(c.cam_ch == 0 || c.cam, "nerfrender: input_ch_cam %d without an embedded_cam", c.cam_ch);
  NRPN_REQUIRE(c.out.rgb && c.out.depth && c.out.acc && c.out.disp && c.out.depth_std, "nerfrender: null output");
  NRPN_REQUIRE(c.num_rays >= 1 && c.num_rays < ((int64_t)1 << 40), "nerfrender: %lld rays", (long long)c.num_rays);
  NRPN_REQUIRE(c.multires >= 0 && 3 + 6 * c.multires <= kEnc, "nerfrender: multires %d does not fit %d encoding columns", c.multires, kEnc);
  NRPN_REQUIRE(c.multires_views >= 0 && 3 + 6 * c.multires_views <= kMaxViewsCh && c.cam_ch >= 0,
               "nerfrender: multires_views %d / input_ch_cam %d", c.multires_views, c.cam_ch);
  NRPN_REQUIRE(c.z2_mode >= 0 && c.z2_mode <= 2, "nerfrender: z2 mode %d", c.z2_mode);
  NRPN_REQUIRE(c.s1 >= 1 && c.s1 <= 65536 && c.s2 >= 0 && c.s2 <= 65536, "nerfrender: %d + %d samples", c.s1, c.s2);
  NRPN_REQUIRE((c.z2_mode == 0) == (c.s2 == 0), "nerfrender: z2 mode %d with %d second-pass samples", c.z2_mode, c.s2);
  NRPN_REQUIRE(c.z2_mode != 1 || (c.s2 == c.s1 && c.s1 >= 3), "nerfrender: depth-guided sampling draws as many samples as pass 1 has, >= 3");
  NRPN_REQUIRE(c.z2_mode != 2 || c.z2_in, "nerfrender: z2 mode 2 without z2");
  NRPN_REQUIRE(c.chunk >= 1, "nerfrender: chunk %lld", (long long)c.chunk);
  const int64_t chunk = c.chunk < c.num_rays ? c.chunk : c.num_rays;
  const int smax = c.s1 > c.s2 ? c.s1 : c.s2;
  NRPN_REQUIRE(chunk * smax < ((int64_t)1 << 31) - kTile, "nerfrender: chunk too large");
  const Layout lay = work_layout(chunk, c.s1, c.s2);
  NRPN_REQUIRE(c.work_bytes >= lay.total, "nerfrender: work buffer of %lld bytes is too small", (long long)c.work_bytes);
  NRPN_LDS(nerfrender_trunk_kernel, kLdsBytes);
  char *wk = static_cast<char *>(c.work);
  float *gbuf = reinterpret_cast<float *>(wk + lay.gbuf);
  for (int64_t r0 = 0; r0 < c.num_rays; r0 += chunk) {
    const int n = (int)(c.num_rays - r0 < chunk ? c.num_rays - r0 : chunk);
    const int blocks = (n + 63) / 64;
    const float *rays;
    if (c.rays) {
      rays = c.rays + r0 * 6;
    } else {
      float *gen = reinterpret_cast<float *>(wk + lay.rays);
      nerfrender_rays_kernel<<<blocks, 64, 0, c.stream>>>(c.camera, c.W, r0, n, gen);
      NRPN_LAUNCH_CHECK("nerfrender_rays_kernel");
      rays = gen;
    }
    float *raw1 = c.raw1_out ? c.raw1_out + r0 * c.s1 * 4 : reinterpret_cast<float *>(wk + lay.raw1);
    float *raw2 = reinterpret_cast<float *>(wk + lay.raw2);
    RayPoints rp{rays, c.z1, 0, c.s1, (int64_t)n * c.s1, c.cx, c.cy, c.cz, c.scale};
    if (int rc = mlp_pass(c, rp, gbuf, raw1)) return rc;
    const float *z2 = nullptr;
    if (c.z2_mode == 1) {
      float *zs = c.z2_out ? c.z2_out + r0 * c.s2 : reinterpret_cast<float *>(wk + lay.z2);
      nerfrender_sample_kernel<<<blocks, 64, 0, c.stream>>>(raw1, rays, c.z1, c.s1, c.near, c.far, n, zs);
      NRPN_LAUNCH_CHECK("nerfrender_sample_kernel");
      z2 = zs;
    } else if (c.z2_mode == 2) {
      z2 = c.z2_in + r0 * c.s2;
    }
    if (z2) {
      RayPoints rp2{rays, z2, c.s2, c.s2, (int64_t)n * c.s2, c.cx, c.cy, c.cz, c.scale};
      if (int rc = mlp_pass(c, rp2, gbuf, raw2)) return rc;
    }
    nerfrender_composite_kernel<<<blocks, 64, 0, c.stream>>>(raw1, c.z1, 0, c.s1, raw2, z2 ? z2 : c.z1, c.s2, rays, n, r0, c.out);
    NRPN_LAUNCH_CHECK("nerfrender_composite_kernel");
  }
  return NRPN_OK;
}

}  // namespace

extern "C" {

int64_t nrpn_nerfrender_work_bytes(int64_t chunk_rays, int s1, int s2) {
  if (chunk_rays < 1 || s1 < 1 || s2 < 0 || s1 > 65536 || s2 > 65536) return -1;
  if (chunk_rays * (s1 > s2 ? s1 : s2) >= ((int64_t)1 << 31) - kTile) return -1;
  return work_layout(chunk_rays, s1, s2).total;
}

int nrpn_nerfrender_samples(const float *raw, const float *rays, const float *z, int num_samples, float near, float far,
                            int64_t num_rays, float *z2, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && rays && z && z2, "nerfrender_samples: null pointer");
  NRPN_REQUIRE(num_samples >= 3 && num_samples <= 65536, "nerfrender_samples: %d samples", num_samples);
  NRPN_REQUIRE(num_rays >= 1 && num_rays < 0x7fffffff, "nerfrender_samples: %lld rays", (long long)num_rays);
  nerfrender_sample_kernel<<<(int)cdiv64(num_rays, 64), 64, 0, as_stream(stream)>>>(raw, rays, z, num_samples, near, far, (int)num_rays, z2);
  NRPN_LAUNCH_CHECK("nerfrender_sample_kernel");
  return NRPN_OK;
}

int nrpn_nerfrender_rays(const float *rays, int64_t num_rays, float near, float far, float center_x, float center_y, float center_z,
                         float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed, const float *w_view,
                         const float *b_view, const float *embedded_cam, const float *z1, int s1, int z2_mode, const float *z2_in, int s2,
                         int64_t chunk, void *work, int64_t work_bytes, float *rgb, float *depth, float *acc, float *disp,
                         float *depth_std, float *z_vals, float *weights, float *raw1_out, float *z2_out, nrpn_stream_t stream) {
  NRPN_REQUIRE(rays, "nerfrender_rays: null rays");
  RenderCall c{rays, nullptr, 0, num_rays, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam,
               packed, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
               CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, as_stream(stream)};
  return render(c);
}

int nrpn_nerfrender_frame(int height, int width, const float *camera, float near, float far, float center_x, float center_y,
                          float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                          const float *w_view, const float *b_view, const float *embedded_cam, const float *z1, int s1, int z2_mode,
                          const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes, float *rgb, float *depth, float *acc,
                          float *disp, float *depth_std, float *z_vals, float *weights, float *raw1_out, float *z2_out,
                          nrpn_stream_t stream) {
  NRPN_REQUIRE(camera && height >= 1 && width >= 1, "nerfrender_frame: camera / %d x %d", height, width);
  RenderCall c{nullptr, camera, width, (int64_t)height * width, near, far, center_x, center_y, center_z, bb_scale, multires,
               multires_views, input_ch_cam, packed, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
               CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, as_stream(stream)};
  return render(c);
}

}  // extern "C"
