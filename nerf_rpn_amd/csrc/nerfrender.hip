// Views of a trained NeRF MLP (scripts/nerf_render.py; reference data/scannet/run_nerf.py: render :82-157, render_rays :514-614,
// compute_samples_around_depth :497-502, forward_with_additonal_samples :504-512, raw2outputs :437-469, render_video :184-185).
//
// Per chunk of rays:
//   rays     (frame mode) o = t, d = R [(u - cx) / fx, -(v - cy) / fy, -1] of pixel r = v W + u, float32 in the reference's order
//   trunk    the shared MFMA trunk (nerf_mlp.cuh) over the points o_r + d_r z[r][s] -> raw sigma and g
//   head     one thread per point: v = relu(g + c_r), raw rgb = W_rgb v + b_rgb; c_r = W_d embed_dirs(d_r / |d_r|) + W_c cam + b is
//            computed per ray of the tile in LDS.  unit_dir, embed_dirs, view_row and rgb_head are nerf_mlp.cuh's, the ones
//            nerfquery.hip runs: a query of the same points and view directions gives the same raw, bit for bit
//   sample   (two-pass) one thread per ray: weights of pass 1 -> depth, std -> clamped +-3 sigma bins -> inverse CDF at linspace(0, 1)
//   trunk + head again over z2, then
//   composite  one thread per ray: merge of the two non-decreasing lists, weights, rgb / depth / acc / disp / depth_std
// The per-ray reductions (sample, composite) run in float64 on the float32 raw and z values: they are a few hundred operations per
// sample next to the 1.2 MFLOP of its MLP query, and the result then carries no summation-order error of its own.  Point positions are
// float32 with the reference's operation order and no contraction (they feed sinf(2^8 p)).  No atomics; a ray's result does not
// depend on its chunk or on the tiles its samples fall into.
#include "nerf_mlp.cuh"
#include "nerf_ray.cuh"

namespace {

using namespace nerfmlp;
using namespace nerfray;      // ray_norm, sample_weight, MergeCursor, merged_walk, RaySums, sizes_ok
static_assert(kRayTile == kTile, "the size limits count the trunk's tiles");

constexpr int kCtileLd = kHalf + 1;   // bank skew between the rays of a head tile

struct RayPoints {
  const float *rays;      // [rays of the chunk][6]: o, d
  const float *z;         // [S] (z_stride 0) or [rays of the chunk][S] (z_stride S)
  int z_stride, S;
  int64_t num_points;     // rays of the chunk * S
  float cx, cy, cz, scale;
  // The world point o + d z of point pi, the product and the sum rounded one after the other (the reference's order; it feeds
  // sinf(2^8 p)).  A partial tile's pi past the end repeats the last point; nothing of it may be stored.
  __device__ __forceinline__ void world(int64_t pi, float (&p)[3]) const {
    if (pi > num_points - 1) pi = num_points - 1;
    const int64_t ray = pi / S;
    const int s = (int)(pi - ray * S);
    const float zv = z[ray * z_stride + s];
    const float *o = rays + ray * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(o[a], __fmul_rn(o[3 + a], zv));
  }
};

// ---- rays ------------------------------------------------------------------------------------------------------------------------
// camera: fx, fy, cx, cy, then c2w[:3, :4] row-major
__global__ void nerfrender_rays_kernel(const float *__restrict__ camera, int W, int64_t ray0, int count, float *__restrict__ rays) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  pixel_ray(camera, W, ray0 + i, rays + (int64_t)i * 6);
}

// ---- trunk (kernel: nerf_mlp.cuh) ------------------------------------------------------------------------------------------------
struct RaySrc {
  const RayPoints &rp;
  int64_t tile0;
  __device__ __forceinline__ void point(int i, float (&p)[3]) const {
    rp.world(tile0 + i, p);
    const float c[3] = {rp.cx, rp.cy, rp.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fmul_rn(__fsub_rn(p[a], c[a]), rp.scale);
  }
};
struct RayTile {          // the tiles of one pass over a chunk's rays
  RayPoints rp;
  int multires;
  float *raw;             // [points of the pass][4]
  __device__ __forceinline__ RaySrc src(unsigned block) const { return {rp, (int64_t)block * kTile}; }
  __device__ __forceinline__ RawSink sink(unsigned block) const { return {(int64_t)block * kTile, rp.num_points, raw}; }
};

// ---- head ------------------------------------------------------------------------------------------------------------------------
// One workgroup of 64 threads, one tile of 64 points: nerf_mlp.cuh's view_row of the tile's rays in LDS, then its rgb_head over the
// point's 128 trunk outputs in registers.  w_view [128][views_ch + cam_ch]: the view and camera columns of views_linears.0.weight;
// b_view [128]; cam [cam_ch]; mask [points][4] (kMask only): the relu's derivative, for the camera-embedding gradient
template <bool kMask>
__device__ __forceinline__ void head_tile(const RayPoints &rp, const float *__restrict__ packed, const float *__restrict__ w_view,
                                          const float *__restrict__ b_view, const float *__restrict__ cam, int multires_views, int cam_ch,
                                          const float *__restrict__ gbuf, float *__restrict__ raw, uint32_t *__restrict__ mask) {
  __shared__ float emb[kTile][kMaxViewsCh];
  __shared__ float cbase[kHalf];
  __shared__ float ctile[kTile * kCtileLd];
  const int t = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * kTile;
  const int64_t last = tile0 + kTile - 1 < rp.num_points ? tile0 + kTile - 1 : rp.num_points - 1;
  const int64_t ray_first = tile0 / rp.S;
  const int nr = (int)(last / rp.S - ray_first) + 1;          // rays with a sample in this tile: 1 .. 64
  const int views_ch = 3 + 6 * multires_views;

  // view_row of every ray of the tile, in two steps: what no ray changes, once; then each ray's view columns
  for (int j = t; j < kHalf; j += kTile) cbase[j] = view_row_cam(j, w_view, b_view, cam, views_ch, cam_ch);
  if (t < nr) {
    float vd[3];
    unit_dir(rp.rays + (ray_first + t) * 6 + 3, vd);
    embed_dirs(emb[t], vd, multires_views);
  }
  __syncthreads();
  for (int idx = t; idx < nr * kHalf; idx += kTile) {
    const int ray = idx / kHalf, j = idx - ray * kHalf;
    ctile[ray * kCtileLd + j] = view_row_dirs(cbase[j], j, w_view, emb[ray], views_ch, cam_ch);
  }
  __syncthreads();

  const int64_t pi = tile0 + t;
  const int64_t pc = pi < rp.num_points ? pi : rp.num_points - 1;
  const float *crow = ctile + (int)(pc / rp.S - ray_first) * kCtileLd;
  const float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + t;
  float g[kHalf];
#pragma unroll
  for (int j = 0; j < kHalf; ++j) g[j] = gt[j * kTile];
  float r[3];
  uint32_t m[4] = {0u, 0u, 0u, 0u};
  rgb_head<kMask, kHalf>([&](int j) { return g[j]; }, crow, packed + kOffRgbW, r, m);
  if (pi < rp.num_points) {
    rgb_store(raw + pi * 4, r, packed);
    if (kMask) *reinterpret_cast<uint4 *>(mask + pi * 4) = make_uint4(m[0], m[1], m[2], m[3]);
  }
}

__global__ __launch_bounds__(kTile) void nerfrender_head_kernel(RayPoints rp, const float *__restrict__ packed,
                                                                const float *__restrict__ w_view, const float *__restrict__ b_view,
                                                                const float *__restrict__ cam, int multires_views, int cam_ch,
                                                                const float *__restrict__ gbuf, float *__restrict__ raw) {
  head_tile<false>(rp, packed, w_view, b_view, cam, multires_views, cam_ch, gbuf, raw, nullptr);
}

// ---- boxes (scripts/nerf_render_boxes.py) ------------------------------------------------------------------------
// A render restricted to K boxes counts a sample if its world point lies in at least one box (keep) or in none (remove); the raw
// values of every other sample become +0, so it has no density and no weight.  A box is 8 doubles: centre, half extents, cos(theta),
// sin(theta) of its rotation about z.  Per pass of a chunk:
//   boxmask   one wave per tile of the pass: a byte per point (counted or not) and a flag per tile (any point counted)
//   trunk     the flagged sibling of the trunk kernel and the flagged head below: a tile whose flag is 0 runs neither
//   boxzero   +0 into raw of every point whose byte is 0, points of skipped tiles included
constexpr int kMaxBoxes = 1024;

// The world point of a sample is RayPoints::world, the point RaySrc normalises; the test is float64 and closed: |R(-theta)(p - c)| <= half extent on each axis.  The box table is read through wave-uniform addresses.  A partial last
// tile tests only its valid points.
__global__ __launch_bounds__(kTile) void nerfrender_boxmask_kernel(RayPoints rp, const double *__restrict__ boxes, int num_boxes,
                                                                   int remove, uint8_t *__restrict__ counted,
                                                                   uint32_t *__restrict__ flags) {
  const int t = threadIdx.x;
  const int64_t pi = (int64_t)blockIdx.x * kTile + t;
  const bool valid = pi < rp.num_points;
  float pf[3];
  rp.world(pi, pf);
  const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
  bool in = false;
  for (int k = 0; k < num_boxes; ++k) {
    const double *b = boxes + (int64_t)k * 8;
    const double dx = p[0] - b[0], dy = p[1] - b[1], dz = p[2] - b[2];
    const double u = b[6] * dx + b[7] * dy, v = b[6] * dy - b[7] * dx;
    in = in || (fabs(u) <= b[3] && fabs(v) <= b[4] && fabs(dz) <= b[5]);
  }
  const bool c = valid && (remove ? !in : in);
  if (valid) counted[pi] = c ? 1 : 0;
  const bool any = __ballot(c) != 0ull;
  if (t == 0) flags[blockIdx.x] = any ? 1u : 0u;
}

// the head of the box path: as nerfrender_head_kernel, for the tiles whose flag is not 0
__global__ __launch_bounds__(kTile) void nerfrender_head_flagged_kernel(RayPoints rp, const float *__restrict__ packed,
                                                                        const float *__restrict__ w_view,
                                                                        const float *__restrict__ b_view, const float *__restrict__ cam,
                                                                        int multires_views, int cam_ch, const float *__restrict__ gbuf,
                                                                        float *__restrict__ raw, const uint32_t *__restrict__ flags) {
  if (flags[blockIdx.x] == 0) return;
  head_tile<false>(rp, packed, w_view, b_view, cam, multires_views, cam_ch, gbuf, raw, nullptr);
}

// raw [points][4]: +0 to the four values of every point that does not count
__global__ __launch_bounds__(256) void nerfrender_boxzero_kernel(const uint8_t *__restrict__ counted, int64_t num_points,
                                                                 float *__restrict__ raw) {
  const int64_t pi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pi < num_points && counted[pi] == 0) *reinterpret_cast<float4 *>(raw + pi * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// tiles_run[pass] = the tiles of the chunk's pass that ran (every tile without skip, else those flagged), added to what the earlier
// chunks left there; one workgroup per pass, fixed-order sums
__global__ __launch_bounds__(256) void nerfrender_boxcount_kernel(const uint32_t *__restrict__ flags1, int tiles1,
                                                                  const uint32_t *__restrict__ flags2, int tiles2, int skip, int first,
                                                                  int64_t *__restrict__ tiles_run) {
  __shared__ int64_t part[256];
  const int t = threadIdx.x, pass = blockIdx.x;
  const uint32_t *flags = pass ? flags2 : flags1;
  const int n = pass ? tiles2 : tiles1;
  int64_t a = 0;
  for (int i = t; i < n; i += 256) a += skip ? (int64_t)(flags[i] != 0) : 1;
  part[t] = a;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) tiles_run[pass] = (first ? 0 : tiles_run[pass]) + part[0];
}

// ---- per-ray reductions, float64 ---------------------------------------------------------------------------------------------
// raw [rays][S][4], z [S] shared, rays [rays][6] -> z2 [rays][S]; Bins and the depth / variance walk are nerf_ray.cuh's
__global__ void nerfrender_sample_kernel(const float *__restrict__ raw, const float *__restrict__ rays, const float *__restrict__ z, int S,
                                         float near, float far, int num_rays, float *__restrict__ z2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const double nd = ray_norm(rays + (int64_t)r * 6 + 3);
  const float *sg = raw + (int64_t)r * S * 4 + 3;
  double depth, var;
  depth_and_var(z, sg, S, nd, depth, var);
  const Bins b = bins_around_depth(depth, var, (double)z[S - 1] - (double)z[S - 2], S, near, far);
  const double total = b.total();
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
    out[j] = b.sample(u, below, cb, above, k < S ? ca : cb);
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
  RaySums sums;
  merged_walk(za, ra + 3, S1, zb, rb + 3, S2, nd, [&](bool a, int i, float zc, double w) {
    const int s = sums.s;
    sums.add(a ? ra + 4 * i : rb + 4 * i, zc, w);
    if (o.z_vals) o.z_vals[gr * S + s] = zc;
    if (o.weights) o.weights[gr * S + s] = (float)w;
  });
  const double depth = sums.depth();
  o.rgb[gr * 3] = (float)sums.c0;
  o.rgb[gr * 3 + 1] = (float)sums.c1;
  o.rgb[gr * 3 + 2] = (float)sums.c2;
  o.depth[gr] = (float)depth;
  o.acc[gr] = (float)sums.acc;
  o.disp[gr] = (float)sums.disp();
  o.depth_std[gr] = (float)sqrt(fmin(fmax(sums.var(), 0.0), 1.0));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxRenderRays = (int64_t)1 << 40, kMaxCamoptRays = (int64_t)1 << 31;

int check_model(const char *who, int multires, int multires_views, int cam_ch) {
  NRPN_REQUIRE(model_ok(multires, 0, 0), "%s: multires %d does not fit %d encoding columns", who, multires, kEnc);
  NRPN_REQUIRE(model_ok(multires, multires_views, cam_ch), "%s: multires_views %d / input_ch_cam %d", who, multires_views, cam_ch);
  return NRPN_OK;
}

// z2_mode 0: one pass; 1: s2 = s1 samples drawn around the first pass's depth; 2: the s2 samples of z2_in
int check_samples(const char *who, int z2_mode, int s1, int s2, const float *z2_in) {
  NRPN_REQUIRE(z2_mode >= 0 && z2_mode <= 2 && (z2_mode == 0) == (s2 == 0), "%s: z2 mode %d with %d second-pass samples", who, z2_mode, s2);
  NRPN_REQUIRE(z2_mode != 1 || (s2 == s1 && s1 >= 3), "%s: depth-guided sampling draws as many samples as pass 1 has, >= 3", who);
  NRPN_REQUIRE(z2_mode != 2 || z2_in, "%s: z2 mode 2 without z2", who);
  return NRPN_OK;
}

struct RayCall {          // what a render and the camera-embedding objective share
  int64_t num_rays;
  float cx, cy, cz, scale;
  int multires;
  const float *packed, *z1;
  int s1, s2;
  int64_t chunk;
  void *work;
  int64_t work_bytes;
  hipStream_t stream;
  const uint4 *split = nullptr;       // the bf16x3 planes of packed: the trunk then runs in that arithmetic (renders only); null: fp32
  int64_t chunk_rays() const { return chunk < num_rays ? chunk : num_rays; }
  int64_t chunks() const { return cdiv64(num_rays, chunk_rays()); }
};

int check_call(const char *who, const RayCall &c, int64_t max_rays) {
  NRPN_REQUIRE(c.packed && c.z1 && c.work, "%s: null pointer", who);
  NRPN_REQUIRE(sizes_ok(c.num_rays, max_rays, c.chunk, c.s1, c.s2), "%s: %lld rays in chunks of %lld with %d + %d samples", who,
               (long long)c.num_rays, (long long)c.chunk, c.s1, c.s2);
  return NRPN_OK;
}

// after check_call: the work buffer holds ``need`` bytes
int check_work(const char *who, const RayCall &c, int64_t need) {
  NRPN_REQUIRE(c.work_bytes >= need, "%s: work buffer of %lld bytes is too small", who, (long long)c.work_bytes);
  return NRPN_OK;
}

struct PassLayout {       // of a chunk's two passes in the work buffer, in bytes; every part 16-byte aligned
  int64_t raw1, raw2, z2, gbuf, end;      // z2: the drawn samples, where the caller keeps them here
};
PassLayout pass_layout(int64_t at, int64_t chunk, int s1, int s2, bool with_z2) {
  PassLayout l{};
  const int smax = s1 > s2 ? s1 : s2;
  l.raw1 = at;
  l.raw2 = l.raw1 + align16(chunk * s1 * 16);
  l.z2 = l.raw2 + align16(chunk * s2 * 16);
  l.gbuf = l.z2 + (with_z2 ? align16(chunk * s2 * 4) : 0);
  l.end = l.gbuf + cdiv64(chunk * smax, kTile) * kTile * kHalf * 4;
  return l;
}
// a render's work buffer: the chunk's generated rays at byte 0, then the passes
PassLayout render_layout(int64_t chunk, int s1, int s2) { return pass_layout(align16(chunk * 6 * 4), chunk, s1, s2, true); }

struct BoxLayout : PassLayout {       // a render's work buffer followed by what the box path keeps per pass
  int64_t counted[2], flags[2], total;      // a byte per point, a uint32 per tile
};
BoxLayout box_layout(int64_t chunk, int s1, int s2) {
  BoxLayout l{render_layout(chunk, s1, s2)};
  l.counted[0] = l.end;
  l.counted[1] = l.counted[0] + align16(chunk * s1);
  l.flags[0] = l.counted[1] + align16(chunk * s2);
  l.flags[1] = l.flags[0] + align16(cdiv64(chunk * s1, kTile) * 4);
  l.total = l.flags[1] + align16(cdiv64(chunk * s2, kTile) * 4);
  return l;
}

struct Chunk {
  int64_t r0;               // its first ray
  int n, blocks;            // rays; workgroups of the one-thread-per-ray kernels
  const float *rays, *z2;   // of its rays; z2 null without a second pass
  const float *zb;          // z2, or z1 without a second pass: the per-ray kernels then read nothing of it
  RayPoints rp[2];          // pass 1 over the shared z1, pass 2 over z2
  int tiles[2];
};
// rays / z2: the call's arrays (whole: the chunk starts at ray r0 of them) or buffers that hold one chunk
Chunk chunk_at(const RayCall &c, int64_t ci, const float *rays, bool rays_whole, const float *z2, bool z2_whole) {
  Chunk k{};
  k.r0 = ci * c.chunk_rays();
  k.n = (int)(c.num_rays - k.r0 < c.chunk_rays() ? c.num_rays - k.r0 : c.chunk_rays());
  k.blocks = (k.n + 63) / 64;
  k.rays = rays + (rays_whole ? k.r0 * 6 : 0);
  k.z2 = c.s2 ? z2 + (z2_whole ? k.r0 * c.s2 : 0) : nullptr;
  k.zb = k.z2 ? k.z2 : c.z1;
  k.rp[0] = RayPoints{k.rays, c.z1, 0, c.s1, (int64_t)k.n * c.s1, c.cx, c.cy, c.cz, c.scale};
  k.rp[1] = RayPoints{k.rays, k.z2, c.s2, c.s2, (int64_t)k.n * c.s2, c.cx, c.cy, c.cz, c.scale};
  for (int pass = 0; pass < 2; ++pass) k.tiles[pass] = (int)cdiv64(k.rp[pass].num_points, kTile);
  return k;
}

// the trunk over pass ``pass`` of a chunk, in the call's arithmetic; flags: of the pass's tiles, and only the flagged ones run
int trunk_pass(const RayCall &c, const Chunk &k, int pass, float *gbuf, float *raw, const uint32_t *flags = nullptr) {
  return launch_trunk(RayTile{k.rp[pass], c.multires, raw}, k.tiles[pass], c.packed, c.split, gbuf, c.stream, flags);
}

struct RenderCall : RayCall {
  const float *rays, *camera;       // one of them
  int W;
  float near, far;
  int multires_views, cam_ch;
  const float *w_view, *b_view, *cam;
  int z2_mode;
  const float *z2_in;
  CompositeOut out;
  float *raw1_out, *z2_out;
  // a render restricted to boxes: the table [num_boxes][8] (null: the plain render), keep or remove, whether tiles without a counted
  // point are skipped, and where the count of the tiles that ran goes (may be null)
  const double *boxes = nullptr;
  int num_boxes = 0, remove = 0, skip = 0;
  int64_t *tiles_run = nullptr;
};

struct BoxBufs {          // of the work buffer, per pass; null without boxes
  uint8_t *counted[2];
  uint32_t *flags[2];
};

int mlp_pass(const RenderCall &c, const Chunk &k, int pass, float *gbuf, float *raw, const BoxBufs &bb) {
  if (!c.boxes) {
    if (int rc = trunk_pass(c, k, pass, gbuf, raw)) return rc;
    nerfrender_head_kernel<<<k.tiles[pass], kTile, 0, c.stream>>>(k.rp[pass], c.packed, c.w_view, c.b_view, c.cam, c.multires_views,
                                                                  c.cam_ch, gbuf, raw);
    NRPN_LAUNCH_CHECK("nerfrender_head_kernel");
    return NRPN_OK;
  }
  nerfrender_boxmask_kernel<<<k.tiles[pass], kTile, 0, c.stream>>>(k.rp[pass], c.boxes, c.num_boxes, c.remove, bb.counted[pass],
                                                                   bb.flags[pass]);
  NRPN_LAUNCH_CHECK("nerfrender_boxmask_kernel");
  const uint32_t *flags = c.skip ? bb.flags[pass] : nullptr;
  if (int rc = trunk_pass(c, k, pass, gbuf, raw, flags)) return rc;
  if (flags) {
    nerfrender_head_flagged_kernel<<<k.tiles[pass], kTile, 0, c.stream>>>(k.rp[pass], c.packed, c.w_view, c.b_view, c.cam,
                                                                          c.multires_views, c.cam_ch, gbuf, raw, flags);
    NRPN_LAUNCH_CHECK("nerfrender_head_flagged_kernel");
  } else {
    nerfrender_head_kernel<<<k.tiles[pass], kTile, 0, c.stream>>>(k.rp[pass], c.packed, c.w_view, c.b_view, c.cam, c.multires_views,
                                                                  c.cam_ch, gbuf, raw);
    NRPN_LAUNCH_CHECK("nerfrender_head_kernel");
  }
  nerfrender_boxzero_kernel<<<(unsigned)cdiv64(k.rp[pass].num_points, 256), 256, 0, c.stream>>>(bb.counted[pass], k.rp[pass].num_points, raw);
  NRPN_LAUNCH_CHECK("nerfrender_boxzero_kernel");
  return NRPN_OK;
}

int render(const RenderCall &c) {
  if (int rc = check_call("nerfrender", c, kMaxRenderRays)) return rc;
  NRPN_REQUIRE(c.w_view && c.b_view, "nerfrender: null pointer");
  NRPN_REQUIRE(c.cam_ch == 0 || c.cam, "nerfrender: input_ch_cam %d without an embedded_cam", c.cam_ch);
  NRPN_REQUIRE(c.out.rgb && c.out.depth && c.out.acc && c.out.disp && c.out.depth_std, "nerfrender: null output");
  if (int rc = check_model("nerfrender", c.multires, c.multires_views, c.cam_ch)) return rc;
  if (int rc = check_samples("nerfrender", c.z2_mode, c.s1, c.s2, c.z2_in)) return rc;
  const BoxLayout lay = box_layout(c.chunk_rays(), c.s1, c.s2);
  if (int rc = check_work("nerfrender", c, c.boxes ? lay.total : lay.end)) return rc;
  char *wk = static_cast<char *>(c.work);
  BoxBufs bb{};
  if (c.boxes)
    for (int pass = 0; pass < 2; ++pass) {
      bb.counted[pass] = reinterpret_cast<uint8_t *>(wk + lay.counted[pass]);
      bb.flags[pass] = reinterpret_cast<uint32_t *>(wk + lay.flags[pass]);
    }
  float *gen = reinterpret_cast<float *>(wk), *gbuf = reinterpret_cast<float *>(wk + lay.gbuf);
  float *raw2 = reinterpret_cast<float *>(wk + lay.raw2);
  // drawn samples go to z2_out or, a chunk at a time, to the work buffer
  float *z2_drawn = c.z2_out ? c.z2_out : reinterpret_cast<float *>(wk + lay.z2);
  for (int64_t ci = 0; ci < c.chunks(); ++ci) {
    const Chunk k = chunk_at(c, ci, c.rays ? c.rays : gen, c.rays != nullptr, c.z2_mode == 1 ? z2_drawn : c.z2_in,
                             c.z2_mode == 2 || c.z2_out);
    if (!c.rays) {
      nerfrender_rays_kernel<<<k.blocks, 64, 0, c.stream>>>(c.camera, c.W, k.r0, k.n, gen);
      NRPN_LAUNCH_CHECK("nerfrender_rays_kernel");
    }
    float *raw1 = c.raw1_out ? c.raw1_out + k.r0 * c.s1 * 4 : reinterpret_cast<float *>(wk + lay.raw1);
    if (int rc = mlp_pass(c, k, 0, gbuf, raw1, bb)) return rc;
    if (c.z2_mode == 1) {
      nerfrender_sample_kernel<<<k.blocks, 64, 0, c.stream>>>(raw1, k.rays, c.z1, c.s1, c.near, c.far, k.n,
                                                              const_cast<float *>(k.z2));      // in z2_drawn
      NRPN_LAUNCH_CHECK("nerfrender_sample_kernel");
    }
    if (k.z2)
      if (int rc = mlp_pass(c, k, 1, gbuf, raw2, bb)) return rc;
    nerfrender_composite_kernel<<<k.blocks, 64, 0, c.stream>>>(raw1, c.z1, 0, c.s1, raw2, k.zb, c.s2, k.rays, k.n, k.r0, c.out);
    NRPN_LAUNCH_CHECK("nerfrender_composite_kernel");
    if (c.boxes && c.tiles_run) {
      nerfrender_boxcount_kernel<<<2, 256, 0, c.stream>>>(bb.flags[0], k.tiles[0], bb.flags[1], k.z2 ? k.tiles[1] : 0, c.skip, ci == 0,
                                                          c.tiles_run);
      NRPN_LAUNCH_CHECK("nerfrender_boxcount_kernel");
    }
  }
  return NRPN_OK;
}

struct BoxArgs {          // what the box entries add to a render; boxes null: the plain render
  const double *boxes = nullptr;
  int num_boxes = 0, mode = 0, skip = 0;
  int64_t *tiles_run = nullptr;
};
// mode 0: keep, 1: remove
int with_boxes(const char *who, RenderCall &c, const BoxArgs &b) {
  if (!b.boxes) return NRPN_OK;
  NRPN_REQUIRE(b.num_boxes >= 0 && b.num_boxes <= kMaxBoxes, "%s: %d boxes, at most %d are supported", who, b.num_boxes, kMaxBoxes);
  NRPN_REQUIRE(b.mode == 0 || b.mode == 1, "%s: mode %d (0: keep, 1: remove)", who, b.mode);
  c.boxes = b.boxes, c.num_boxes = b.num_boxes, c.remove = b.mode, c.skip = b.skip != 0, c.tiles_run = b.tiles_run;
  return NRPN_OK;
}

// the two entries of a render; split: the bf16x3 planes of packed, or null for the fp32 trunk
int render_rays(const float *rays, int64_t num_rays, float near, float far, float center_x, float center_y, float center_z, float bb_scale,
                int multires, int multires_views, int input_ch_cam, const float *packed, const void *split, const float *w_view,
                const float *b_view, const float *embedded_cam, const float *z1, int s1, int z2_mode, const float *z2_in, int s2,
                int64_t chunk, void *work, int64_t work_bytes, const CompositeOut &out, float *raw1_out, float *z2_out,
                nrpn_stream_t stream, const BoxArgs &box = {}) {
  NRPN_REQUIRE(rays, "nerfrender_rays: null rays");
  RenderCall c{{num_rays, center_x, center_y, center_z, bb_scale, multires, packed, z1, s1, s2, chunk, work, work_bytes, as_stream(stream),
                static_cast<const uint4 *>(split)},
               rays, nullptr, 0, near, far, multires_views, input_ch_cam, w_view, b_view, embedded_cam, z2_mode, z2_in, out, raw1_out, z2_out};
  if (int rc = with_boxes("nerfrender_rays_boxes", c, box)) return rc;
  return render(c);
}

int render_frame(int height, int width, const float *camera, float near, float far, float center_x, float center_y, float center_z,
                 float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed, const void *split,
                 const float *w_view, const float *b_view, const float *embedded_cam, const float *z1, int s1, int z2_mode,
                 const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes, const CompositeOut &out, float *raw1_out,
                 float *z2_out, nrpn_stream_t stream, const BoxArgs &box = {}) {
  NRPN_REQUIRE(camera && height >= 1 && width >= 1, "nerfrender_frame: camera / %d x %d", height, width);
  RenderCall c{{(int64_t)height * width, center_x, center_y, center_z, bb_scale, multires, packed, z1, s1, s2, chunk, work, work_bytes,
                as_stream(stream), static_cast<const uint4 *>(split)},
               nullptr, camera, width, near, far, multires_views, input_ch_cam, w_view, b_view, embedded_cam, z2_mode, z2_in, out, raw1_out,
               z2_out};
  if (int rc = with_boxes("nerfrender_frame_boxes", c, box)) return rc;
  return render(c);
}

// ---- camera-embedding objective (scripts/nerf_test.py --task test_opt; run_nerf.py optimize_camera_embedding :193-229) ---------
// The embedding enters the network at views_linears.0 only: sigma, both sample lists and every compositing weight do not depend on
// it.  prepare computes them once per image -- z2, the float64 weight of every sample in its own list's slot, and, for the chunks
// that fit the budget, the trunk's g tiles.  An evaluation at one embedding then runs, per chunk of rays:
//   head       the head above, which also writes the 128-bit mask g + c > 0 of every point
//   colour     one thread per ray, float64: rgb = sum w sigmoid(raw) in merged order (the composite kernel's sum), e = rgb - target,
//              the ray's loss term rw sum e^2 and dL/drgb = 2 rw e
//   backward   one workgroup per tile: d[p][ch] = dL/drgb[ray][ch] w s (1 - s), A[j][ch] = sum_p mask[p][j] d[p][ch] in point order
//   sum_rows   fixed-order float64 sums of the tiles' A, then of the chunks' A and of the rays' loss terms
// and finish: dc[j] = sum_ch W_rgb[ch][j] A[j][ch], grad[k] = sum_j W_c[j][k] dc[j].  No atomics; a ray's rgb and loss term do not
// depend on its chunk or tile, the sums over rays do only in their rounding.
constexpr int kAcols = 3 * kHalf;     // A as [j][ch]
constexpr int kSumRows = 256;         // rows one workgroup of sum_rows adds

__global__ __launch_bounds__(kTile) void nerfcamopt_head_kernel(RayPoints rp, const float *__restrict__ packed,
                                                                const float *__restrict__ w_view, const float *__restrict__ b_view,
                                                                const float *__restrict__ cam, int multires_views, int cam_ch,
                                                                const float *__restrict__ gbuf, float *__restrict__ raw,
                                                                uint32_t *__restrict__ mask) {
  head_tile<true>(rp, packed, w_view, b_view, cam, multires_views, cam_ch, gbuf, raw, mask);
}

// raw1 [rays][S1][4], raw2 [rays][S2][4] (sigma only), z1 [S1] shared, z2 [rays][S2] -> w1 [rays][S1], w2 [rays][S2]: the weight the
// composite kernel gives each sample, in the sample's own list
__global__ void nerfcamopt_weights_kernel(const float *__restrict__ raw1, const float *__restrict__ z1, int S1,
                                          const float *__restrict__ raw2, const float *__restrict__ z2, int S2,
                                          const float *__restrict__ rays, int num_rays, double *__restrict__ w1, double *__restrict__ w2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const double nd = ray_norm(rays + (int64_t)r * 6 + 3);
  double *wa = w1 + (int64_t)r * S1, *wb = w2 + (int64_t)r * S2;
  merged_walk(z1, raw1 + (int64_t)r * S1 * 4 + 3, S1, z2 + (int64_t)r * S2, raw2 + (int64_t)r * S2 * 4 + 3, S2, nd,
              [&](bool a, int i, float, double w) { (a ? wa : wb)[i] = w; });
}

// raw1 / raw2: the heads' rgb; w1 / w2, z2, target [rays][3] and rw [rays] start at the chunk's first ray, terms and rgb likewise
__global__ void nerfcamopt_colour_kernel(const float *__restrict__ raw1, const float *__restrict__ z1, int S1,
                                         const float *__restrict__ raw2, const float *__restrict__ z2, int S2,
                                         const double *__restrict__ w1, const double *__restrict__ w2, const float *__restrict__ target,
                                         const double *__restrict__ rw, int num_rays, double *__restrict__ dl,
                                         double *__restrict__ terms, float *__restrict__ rgb) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const float *ra = raw1 + (int64_t)r * S1 * 4, *rb = raw2 + (int64_t)r * S2 * 4;
  const double *wa = w1 + (int64_t)r * S1, *wb = w2 + (int64_t)r * S2;
  MergeCursor m{z1, z2 + (int64_t)r * S2, S1, S2, 0, 0};
  double c[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < S1 + S2; ++s) {
    int i;
    const bool a = m.next(i);
    const float *p = a ? ra + 4 * i : rb + 4 * i;
    const double w = a ? wa[i] : wb[i];
    c[0] += w / (1.0 + exp(-(double)p[0]));
    c[1] += w / (1.0 + exp(-(double)p[1]));
    c[2] += w / (1.0 + exp(-(double)p[2]));
  }
  const double q = rw[r];
  double e[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    e[ch] = c[ch] - (double)target[(int64_t)r * 3 + ch];
    dl[(int64_t)r * 3 + ch] = 2.0 * q * e[ch];
    if (rgb) rgb[(int64_t)r * 3 + ch] = (float)c[ch];
  }
  terms[r] = q * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
}

// One workgroup of 128 threads (thread j) per tile of 64 points of one pass: raw [points][4], mask [points][4], w [points] (the
// pass's weights, ray-major like the points), dl [rays][3] -> partial [tile][128][3]
__global__ __launch_bounds__(kHalf) void nerfcamopt_backward_kernel(const float *__restrict__ raw, const uint32_t *__restrict__ mask,
                                                                    const double *__restrict__ w, const double *__restrict__ dl, int S,
                                                                    int64_t num_points, double *__restrict__ partial) {
  __shared__ double d[kTile][3];
  __shared__ uint32_t mk[kTile][4];
  const int t = threadIdx.x;
  if (t < kTile) {
    const int64_t pi = (int64_t)blockIdx.x * kTile + t;
    const bool in = pi < num_points;
    const int64_t ray = in ? pi / S : 0;
    const double wp = in ? w[pi] : 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double v = 0.0;
      if (in) {
        const double s = 1.0 / (1.0 + exp(-(double)raw[pi * 4 + ch]));
        v = dl[ray * 3 + ch] * wp * s * (1.0 - s);
      }
      d[t][ch] = v;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) mk[t][q] = in ? mask[pi * 4 + q] : 0u;
  }
  __syncthreads();
  const int word = t >> 5, bit = t & 31;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int p = 0; p < kTile; ++p) {
    const bool on = (mk[p][word] >> bit) & 1u;
    a0 += on ? d[p][0] : 0.0;
    a1 += on ? d[p][1] : 0.0;
    a2 += on ? d[p][2] : 0.0;
  }
  double *o = partial + (int64_t)blockIdx.x * kAcols + t * 3;
  o[0] = a0, o[1] = a1, o[2] = a2;
}

// in [n][width] -> out [ceil(n / 256)][width]: thread (column, lane q of 4) adds rows q, q + 4, .. of its 256 in order, then
// (q0 + q1) + (q2 + q3).  grid (ceil(n / 256), ceil(width / 64))
__global__ __launch_bounds__(256) void nerfcamopt_sum_rows_kernel(const double *__restrict__ in, int64_t n, int width,
                                                                  double *__restrict__ out) {
  __shared__ double part[4][64];
  const int t = threadIdx.x, col = blockIdx.y * 64 + (t & 63), q = t >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kSumRows;
  double a = 0.0;
  if (col < width)
    for (int i = q; i < kSumRows && row0 + i < n; i += 4) a += in[(row0 + i) * width + col];
  part[q][t & 63] = a;
  __syncthreads();
  if (q == 0 && col < width) out[(int64_t)blockIdx.x * width + col] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
}

// A [128][3], loss [1] -> out [1 + cam_ch]: the loss, then grad[k] = sum_j W_c[j][k] sum_ch W_rgb[ch][j] A[j][ch]
__global__ __launch_bounds__(kHalf) void nerfcamopt_finish_kernel(const double *__restrict__ A, const double *__restrict__ loss,
                                                                  const float *__restrict__ packed, const float *__restrict__ w_view,
                                                                  int views_ch, int cam_ch, double *__restrict__ out) {
  __shared__ double dc[kHalf];
  const int j = threadIdx.x;
  const float *wr = packed + kOffRgbW;
  dc[j] = ((double)wr[j] * A[j * 3] + (double)wr[kHalf + j] * A[j * 3 + 1]) + (double)wr[2 * kHalf + j] * A[j * 3 + 2];
  __syncthreads();
  for (int k = j; k < cam_ch; k += kHalf) {
    double g = 0.0;
    for (int i = 0; i < kHalf; ++i) g += (double)w_view[i * (views_ch + cam_ch) + views_ch + k] * dc[i];
    out[1 + k] = g;
  }
  if (j == 0) out[0] = loss[0];
}

// rows of the buffer that sum_rows' levels need after the n input rows
int64_t sum_rows_extra(int64_t n) {
  int64_t total = 0;
  while (n > 1) {
    n = cdiv64(n, kSumRows);
    total += n;
  }
  return total;
}

// buf: n rows of width doubles followed by sum_rows_extra(n) rows -> *result, the row of their sums
int sum_rows(double *buf, int64_t n, int width, hipStream_t stream, const double **result) {
  while (n > 1) {
    const int64_t m = cdiv64(n, kSumRows);
    double *out = buf + n * width;
    nerfcamopt_sum_rows_kernel<<<dim3((unsigned)m, (unsigned)((width + 63) / 64)), 256, 0, stream>>>(buf, n, width, out);
    NRPN_LAUNCH_CHECK("nerfcamopt_sum_rows_kernel");
    buf = out;
    n = m;
  }
  *result = buf;
  return NRPN_OK;
}

struct CamoptLayout : PassLayout {      // of the work buffer, in bytes; every part 16-byte aligned.  prepare uses the passes' part only
  int64_t mask1, mask2, dl, partial, chunk_a, terms, total;
  int64_t tiles1, tiles2, slot_floats;      // g tiles of a full chunk per pass; floats of a chunk's slot in the g cache
};
CamoptLayout camopt_layout(int64_t num_rays, int64_t chunk, int s1, int s2) {
  CamoptLayout l{pass_layout(0, chunk, s1, s2, false)};
  l.tiles1 = cdiv64(chunk * s1, kTile);
  l.tiles2 = cdiv64(chunk * s2, kTile);
  l.slot_floats = (l.tiles1 + l.tiles2) * kTile * kHalf;
  l.mask1 = l.end;
  l.mask2 = l.mask1 + align16(chunk * s1 * 16);
  l.dl = l.mask2 + align16(chunk * s2 * 16);
  l.partial = l.dl + align16(chunk * 3 * 8);
  const int64_t tiles = l.tiles1 + l.tiles2, chunks = cdiv64(num_rays, chunk);
  l.chunk_a = l.partial + (tiles + sum_rows_extra(tiles)) * kAcols * 8;
  l.terms = l.chunk_a + (chunks + sum_rows_extra(chunks)) * kAcols * 8;
  l.total = l.terms + align16((num_rays + sum_rows_extra(num_rays)) * 8);
  return l;
}

struct CamoptCall : RayCall {
  const float *rays;        // [num_rays][6]
  const float *z2;          // [num_rays][s2]
  float *gcache;
  int64_t cached_chunks;
  // where the trunk's g of chunk ci, pass 0 / 1, lives: its slot of the cache, or the scratch every other chunk shares
  float *g_of(const CamoptLayout &lay, int64_t ci, int pass) const {
    if (ci >= cached_chunks) return reinterpret_cast<float *>(static_cast<char *>(work) + lay.gbuf);
    return gcache + ci * lay.slot_floats + (pass ? lay.tiles1 * kTile * kHalf : 0);
  }
};

int camopt_check(const CamoptCall &c, const char *who, int multires_views, int cam_ch) {
  if (int rc = check_call(who, c, kMaxCamoptRays)) return rc;
  if (int rc = check_model(who, c.multires, multires_views, cam_ch)) return rc;
  NRPN_REQUIRE(c.rays && (c.s2 == 0 || c.z2), "%s: null rays, or %d second-pass samples without z2", who, c.s2);
  NRPN_REQUIRE(c.cached_chunks >= 0 && (c.cached_chunks == 0 || c.gcache), "%s: %lld cached chunks without a cache", who,
               (long long)c.cached_chunks);
  return NRPN_OK;
}

int camopt_prepare(const CamoptCall &c, const float *camera, int W, float near, float far, bool draw_z2, float *rays_out, float *z2_out,
                   double *w1, double *w2) {
  if (int rc = camopt_check(c, "nerfcamopt_prepare", 0, 0)) return rc;
  NRPN_REQUIRE(w1 && (c.s2 == 0 || w2) && (!draw_z2 || z2_out), "nerfcamopt_prepare: null output");
  const CamoptLayout lay = camopt_layout(c.num_rays, c.chunk_rays(), c.s1, c.s2);
  if (int rc = check_work("nerfcamopt_prepare", c, lay.end)) return rc;
  char *wk = static_cast<char *>(c.work);
  float *raw1 = reinterpret_cast<float *>(wk + lay.raw1), *raw2 = reinterpret_cast<float *>(wk + lay.raw2);
  for (int64_t ci = 0; ci < c.chunks(); ++ci) {
    const Chunk k = chunk_at(c, ci, c.rays, true, c.z2, true);
    if (camera) {
      nerfrender_rays_kernel<<<k.blocks, 64, 0, c.stream>>>(camera, W, k.r0, k.n, rays_out + k.r0 * 6);
      NRPN_LAUNCH_CHECK("nerfrender_rays_kernel");
    }
    if (int rc = trunk_pass(c, k, 0, c.g_of(lay, ci, 0), raw1)) return rc;
    if (draw_z2) {
      nerfrender_sample_kernel<<<k.blocks, 64, 0, c.stream>>>(raw1, k.rays, c.z1, c.s1, near, far, k.n, z2_out + k.r0 * c.s2);
      NRPN_LAUNCH_CHECK("nerfrender_sample_kernel");
    }
    if (k.z2)
      if (int rc = trunk_pass(c, k, 1, c.g_of(lay, ci, 1), raw2)) return rc;
    nerfcamopt_weights_kernel<<<k.blocks, 64, 0, c.stream>>>(raw1, c.z1, c.s1, raw2, k.zb, c.s2, k.rays, k.n, w1 + k.r0 * c.s1,
                                                             c.s2 ? w2 + k.r0 * c.s2 : w1);
    NRPN_LAUNCH_CHECK("nerfcamopt_weights_kernel");
  }
  return NRPN_OK;
}

int camopt_eval(const CamoptCall &c, int multires_views, int cam_ch, const float *w_view, const float *b_view, const float *cam,
                const double *w1, const double *w2, const float *target, const double *rw, double *out, float *rgb) {
  if (int rc = camopt_check(c, "nerfcamopt_eval", multires_views, cam_ch)) return rc;
  NRPN_REQUIRE(w_view && b_view && cam && cam_ch >= 1 && w1 && (c.s2 == 0 || w2) && target && rw && out,
               "nerfcamopt_eval: null pointer, or no camera embedding");
  const CamoptLayout lay = camopt_layout(c.num_rays, c.chunk_rays(), c.s1, c.s2);
  if (int rc = check_work("nerfcamopt_eval", c, lay.total)) return rc;
  char *wk = static_cast<char *>(c.work);
  float *const raws[2] = {reinterpret_cast<float *>(wk + lay.raw1), reinterpret_cast<float *>(wk + lay.raw2)};
  uint32_t *const masks[2] = {reinterpret_cast<uint32_t *>(wk + lay.mask1), reinterpret_cast<uint32_t *>(wk + lay.mask2)};
  double *dl = reinterpret_cast<double *>(wk + lay.dl), *partial = reinterpret_cast<double *>(wk + lay.partial);
  double *chunk_a = reinterpret_cast<double *>(wk + lay.chunk_a), *terms = reinterpret_cast<double *>(wk + lay.terms);
  for (int64_t ci = 0; ci < c.chunks(); ++ci) {
    const Chunk k = chunk_at(c, ci, c.rays, true, c.z2, true);
    const double *const ws[2] = {w1 + k.r0 * c.s1, c.s2 ? w2 + k.r0 * c.s2 : w1};
    for (int pass = 0; pass < (c.s2 ? 2 : 1); ++pass) {
      float *g = c.g_of(lay, ci, pass);
      if (ci >= c.cached_chunks)        // the same kernel on the same points as in prepare: the same g
        if (int rc = trunk_pass(c, k, pass, g, raws[pass])) return rc;
      nerfcamopt_head_kernel<<<k.tiles[pass], kTile, 0, c.stream>>>(k.rp[pass], c.packed, w_view, b_view, cam, multires_views, cam_ch, g,
                                                                    raws[pass], masks[pass]);
      NRPN_LAUNCH_CHECK("nerfcamopt_head_kernel");
    }
    nerfcamopt_colour_kernel<<<k.blocks, 64, 0, c.stream>>>(raws[0], c.z1, c.s1, raws[1], k.zb, c.s2, ws[0], ws[1], target + k.r0 * 3,
                                                            rw + k.r0, k.n, dl, terms + k.r0, rgb ? rgb + k.r0 * 3 : nullptr);
    NRPN_LAUNCH_CHECK("nerfcamopt_colour_kernel");
    for (int pass = 0; pass < (c.s2 ? 2 : 1); ++pass) {
      nerfcamopt_backward_kernel<<<k.tiles[pass], kHalf, 0, c.stream>>>(raws[pass], masks[pass], ws[pass], dl, k.rp[pass].S,
                                                                        k.rp[pass].num_points,
                                                                        partial + (int64_t)(pass ? k.tiles[0] : 0) * kAcols);
      NRPN_LAUNCH_CHECK("nerfcamopt_backward_kernel");
    }
    const double *a;
    if (int rc = sum_rows(partial, k.tiles[0] + k.tiles[1], kAcols, c.stream, &a)) return rc;
    NRPN_HIP(hipMemcpyAsync(chunk_a + ci * kAcols, a, kAcols * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
  }
  const double *a, *loss;
  if (int rc = sum_rows(chunk_a, c.chunks(), kAcols, c.stream, &a)) return rc;
  if (int rc = sum_rows(terms, c.num_rays, 1, c.stream, &loss)) return rc;
  nerfcamopt_finish_kernel<<<1, kHalf, 0, c.stream>>>(a, loss, c.packed, w_view, 3 + 6 * multires_views, cam_ch, out);
  NRPN_LAUNCH_CHECK("nerfcamopt_finish_kernel");
  return NRPN_OK;
}

}  // namespace

extern "C" {

int64_t nrpn_nerfrender_work_bytes(int64_t chunk_rays, int s1, int s2) {
  if (!sizes_ok(chunk_rays, kMaxRenderRays, chunk_rays, s1, s2)) return -1;
  return render_layout(chunk_rays, s1, s2).end;
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
  return render_rays(rays, num_rays, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam, packed,
                     nullptr, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                     CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream);
}

int nrpn_nerfrender_rays_bf16x3(const float *rays, int64_t num_rays, float near, float far, float center_x, float center_y,
                                float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                                const void *split, const float *w_view, const float *b_view, const float *embedded_cam, const float *z1,
                                int s1, int z2_mode, const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes,
                                float *rgb, float *depth, float *acc, float *disp, float *depth_std, float *z_vals, float *weights,
                                float *raw1_out, float *z2_out, nrpn_stream_t stream) {
  NRPN_REQUIRE(split, "nerfrender_rays: null planes");
  return render_rays(rays, num_rays, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam, packed,
                     split, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                     CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream);
}

int nrpn_nerfrender_frame(int height, int width, const float *camera, float near, float far, float center_x, float center_y,
                          float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                          const float *w_view, const float *b_view, const float *embedded_cam, const float *z1, int s1, int z2_mode,
                          const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes, float *rgb, float *depth, float *acc,
                          float *disp, float *depth_std, float *z_vals, float *weights, float *raw1_out, float *z2_out,
                          nrpn_stream_t stream) {
  return render_frame(height, width, camera, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam,
                      packed, nullptr, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                      CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream);
}

int nrpn_nerfrender_frame_bf16x3(int height, int width, const float *camera, float near, float far, float center_x, float center_y,
                                 float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                                 const void *split, const float *w_view, const float *b_view, const float *embedded_cam, const float *z1,
                                 int s1, int z2_mode, const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes,
                                 float *rgb, float *depth, float *acc, float *disp, float *depth_std, float *z_vals, float *weights,
                                 float *raw1_out, float *z2_out, nrpn_stream_t stream) {
  NRPN_REQUIRE(split, "nerfrender_frame: null planes");
  return render_frame(height, width, camera, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam,
                      packed, split, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                      CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream);
}

int64_t nrpn_nerfrender_boxes_work_bytes(int64_t chunk_rays, int s1, int s2) {
  if (!sizes_ok(chunk_rays, kMaxRenderRays, chunk_rays, s1, s2)) return -1;
  return box_layout(chunk_rays, s1, s2).total;
}

int nrpn_nerfrender_rays_boxes(const float *rays, int64_t num_rays, float near, float far, float center_x, float center_y, float center_z,
                               float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                               const void *split, const float *w_view, const float *b_view, const float *embedded_cam, const float *z1,
                               int s1, int z2_mode, const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes, float *rgb,
                               float *depth, float *acc, float *disp, float *depth_std, float *z_vals, float *weights, float *raw1_out,
                               float *z2_out, const double *boxes, int num_boxes, int mode, int skip, int64_t *tiles_run,
                               nrpn_stream_t stream) {
  NRPN_REQUIRE(boxes, "nerfrender_rays_boxes: null box table (%d boxes)", num_boxes);
  return render_rays(rays, num_rays, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam, packed,
                     split, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                     CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream,
                     BoxArgs{boxes, num_boxes, mode, skip, tiles_run});
}

int nrpn_nerfrender_frame_boxes(int height, int width, const float *camera, float near, float far, float center_x, float center_y,
                                float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                                const void *split, const float *w_view, const float *b_view, const float *embedded_cam, const float *z1,
                                int s1, int z2_mode, const float *z2_in, int s2, int64_t chunk, void *work, int64_t work_bytes, float *rgb,
                                float *depth, float *acc, float *disp, float *depth_std, float *z_vals, float *weights, float *raw1_out,
                                float *z2_out, const double *boxes, int num_boxes, int mode, int skip, int64_t *tiles_run,
                                nrpn_stream_t stream) {
  NRPN_REQUIRE(boxes, "nerfrender_frame_boxes: null box table (%d boxes)", num_boxes);
  return render_frame(height, width, camera, near, far, center_x, center_y, center_z, bb_scale, multires, multires_views, input_ch_cam,
                      packed, split, w_view, b_view, embedded_cam, z1, s1, z2_mode, z2_in, s2, chunk, work, work_bytes,
                      CompositeOut{rgb, depth, acc, disp, depth_std, z_vals, weights}, raw1_out, z2_out, stream,
                      BoxArgs{boxes, num_boxes, mode, skip, tiles_run});
}

int64_t nrpn_nerfcamopt_work_bytes(int what, int64_t num_rays, int64_t chunk_rays, int s1, int s2) {
  if (what < 0 || what > 2 || !sizes_ok(num_rays, kMaxCamoptRays, chunk_rays, s1, s2)) return -1;
  const CamoptLayout l = camopt_layout(num_rays, chunk_rays < num_rays ? chunk_rays : num_rays, s1, s2);
  return what == 0 ? l.end : what == 1 ? l.total : l.slot_floats * 4;
}

int nrpn_nerfcamopt_prepare(const float *rays, int height, int width, const float *camera, int64_t num_rays, float near, float far,
                            float center_x, float center_y, float center_z, float bb_scale, int multires, const float *packed,
                            const float *z1, int s1, int z2_mode, const float *z2_in, int s2, int64_t chunk, void *work,
                            int64_t work_bytes, float *rays_out, float *z2_out, double *w1, double *w2, float *g_cache,
                            int64_t cached_chunks, nrpn_stream_t stream) {
  NRPN_REQUIRE((rays != nullptr) != (camera != nullptr), "nerfcamopt_prepare: give rays or a camera");
  NRPN_REQUIRE(!camera || (rays_out && height >= 1 && width >= 1 && (int64_t)height * width == num_rays),
               "nerfcamopt_prepare: camera / %d x %d for %lld rays", height, width, (long long)num_rays);
  if (int rc = check_samples("nerfcamopt_prepare", z2_mode, s1, s2, z2_in)) return rc;
  CamoptCall c{{num_rays, center_x, center_y, center_z, bb_scale, multires, packed, z1, s1, s2, chunk, work, work_bytes, as_stream(stream)},
               camera ? rays_out : rays, z2_mode == 1 ? z2_out : z2_in, g_cache, cached_chunks};
  return camopt_prepare(c, camera, width, near, far, z2_mode == 1, rays_out, z2_out, w1, w2);
}

int nrpn_nerfcamopt_eval(const float *rays, int64_t num_rays, float center_x, float center_y, float center_z, float bb_scale,
                         int multires, int multires_views, int input_ch_cam, const float *packed, const float *w_view,
                         const float *b_view, const float *embedded_cam, const float *z1, int s1, const float *z2, int s2,
                         const double *w1, const double *w2, const float *target, const double *ray_weight, int64_t chunk,
                         const float *g_cache, int64_t cached_chunks, void *work, int64_t work_bytes, double *loss_grad, float *rgb,
                         nrpn_stream_t stream) {
  CamoptCall c{{num_rays, center_x, center_y, center_z, bb_scale, multires, packed, z1, s1, s2, chunk, work, work_bytes, as_stream(stream)},
               rays, z2, const_cast<float *>(g_cache), cached_chunks};
  return camopt_eval(c, multires_views, input_ch_cam, w_view, b_view, embedded_cam, w1, w2, target, ray_weight, loss_grad, rgb);
}

}  // extern "C"
