// rgb-sigma grid of a trained NeRF MLP (scripts/nerf_extract.py; reference data/scannet/run_nerf.py:1157-1194 with run_network :50-65).
//
// The reference sends every grid point through the whole 8 x 256 MLP once per training pose.  Only views_linears.0 and rgb_linear see
// the pose, so here the trunk runs once per point and the poses loop over a 128-wide head:
//   trunk (one workgroup = 64 points): positional encoding into LDS, the eight pts_linears, feature_linear, alpha_linear and the
//     feature columns W_f of views_linears.0 -- all matrix products on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain), the
//     activations in one [64][324] fp32 LDS image rewritten in place between two barriers per layer, the weights read from L2 in a
//     packed order (nerfmlp_pack_kernel) that makes every B fragment one coalesced 16-byte load per lane.
//     -> sigma (written to the result) and g = W_f f, 128 floats per point, in a scratch that is bounded by the chunk size.
//   head (one thread = one point): for the poses in order v = relu(g + c_p), rgb = W_rgb v + b_rgb, acc += sigmoid(rgb); acc / P.
//     v comes from nerf_mlp.cuh's head_pre / head_relu, which the render's and the query's heads use through rgb_head; the chains
//     over it are rgb_head's, written out (see the kernel).
// No atomics; a point's arithmetic does not depend on its neighbours, its tile or its chunk.
// This unit also holds the two pack kernels and their launcher (nerfmlp::launch_pack) for every packed layout of the library: the
// forward's matrices here, their transposes for nerfquery.hip.  Segment descriptor and index arithmetic: nerf_mlp.cuh.
#include "nerf_mlp.cuh"

namespace {

using namespace nerfmlp;

// ---- pack (segments, pack_elem: nerf_mlp.cuh) -------------------------------------------------------------------------------------
// The two kernels of every pack of the library: nrpn_nerfgrid_pack* below and, through launch_pack, nerfquery.hip's transposes
__global__ void nerfmlp_pack_kernel(const float *__restrict__ raw, float *__restrict__ packed, PackPlan plan) {
  const PackSeg s = plan.seg[blockIdx.y];
  const int64_t total = s.n_out == 0 ? s.kb : (int64_t)(s.ka_pad + s.kb) * s.n_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    packed[s.dst + i] = s.n_out == 0 ? raw[s.src + i] : pack_elem<4>(raw, s, i);
}

__global__ void nerfmlp_pack_split_kernel(const float *__restrict__ raw, unsigned short *__restrict__ planes, int64_t lo_plane,
                                          PackPlan plan) {
  const PackSeg s = plan.seg[blockIdx.y];
  const int64_t total = (int64_t)(s.ka_pad + s.kb) * s.n_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = pack_elem<8>(raw, s, i);
    const __bf16 hb = (__bf16)v;
    planes[s.dst + i] = __builtin_bit_cast(unsigned short, hb);
    planes[lo_plane + s.dst + i] = f32_to_bf16_bits(v - (float)hb);
  }
}

// ---- trunk (kernel: nerf_mlp.cuh) ------------------------------------------------------------------------------------------------
struct GridArgs {
  const float *xs, *ys, *zs;      // linspace values [rx], [ry], [rz]
  int rx, ry, rz;
  float cx, cy, cz, scale;
  int64_t num_points;             // rx * ry * rz
  int layout;                     // 0 flat (N, 4); 1 wlh (rx, ry, rz, 4)
};

__device__ __forceinline__ int64_t out_index(const GridArgs &g, int64_t r) {
  if (g.layout == 0) return r * 4;
  const int ix = (int)(r % g.rx);
  const int64_t t = r / g.rx;
  const int iy = (int)(t % g.ry), iz = (int)(t / g.ry);
  return (((int64_t)ix * g.ry + iy) * g.rz + iz) * 4;
}

// where a tile's points come from (lattice index -> linspace values) and where sigma goes
struct GridSrc {
  GridArgs ga;
  int64_t tile0;
  __device__ __forceinline__ void point(int i, float (&p)[3]) const {
    int64_t pr = tile0 + i;
    if (pr > ga.num_points - 1) pr = ga.num_points - 1;       // a partial tile repeats the last point; nothing of it is stored
    const int ix = (int)(pr % ga.rx);
    const int64_t tq = pr / ga.rx;
    const int iy = (int)(tq % ga.ry), iz = (int)(tq / ga.ry);
    p[0] = (ga.xs[ix] - ga.cx) * ga.scale;
    p[1] = (ga.ys[iy] - ga.cy) * ga.scale;
    p[2] = (ga.zs[iz] - ga.cz) * ga.scale;
  }
};
struct GridSink {
  GridArgs ga;
  int64_t tile0;
  float *out;
  __device__ __forceinline__ void sigma(int i, float s) const {
    const int64_t pr = tile0 + i;
    if (pr < ga.num_points) out[out_index(ga, pr) + 3] = s;
  }
};

struct GridTile {                 // the tiles of a chunk that starts at lattice point point0
  GridArgs ga;
  int multires;
  int64_t point0;
  float *out;
  __device__ __forceinline__ GridSrc src(unsigned block) const { return {ga, point0 + (int64_t)block * kTile}; }
  __device__ __forceinline__ GridSink sink(unsigned block) const { return {ga, point0 + (int64_t)block * kTile, out}; }
};

// ---- head ------------------------------------------------------------------------------------------------------------------------
// One thread per point, its 128 trunk outputs in registers; per pose the chain the render's head runs (rgb_head).  ctab
// [pose][128] is the caller's table of view rows.  It is not view_row's: ops.nerf_grid_query forms it as a matrix product through the
// BLAS, the extraction tests hold that table against the reference, and taking it from view_row would move its bits
__global__ __launch_bounds__(kTile) void nerfgrid_head_kernel(GridArgs ga, const float *__restrict__ packed, int64_t point0,
                                                              const float *__restrict__ gbuf, const float *__restrict__ ctab,
                                                              int num_poses, float *__restrict__ out) {
  const int i = threadIdx.x;
  const int64_t pr = point0 + (int64_t)blockIdx.x * kTile + i;
  const float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + i;
  float g[kHalf];
#pragma unroll
  for (int j = 0; j < kHalf; ++j) g[j] = gt[j * kTile];
  const float b0 = packed[kOffRgbB], b1 = packed[kOffRgbB + 1], b2 = packed[kOffRgbB + 2];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int p = 0; p < num_poses; ++p) {
    const float *c = ctab + (int64_t)p * kHalf;
    // W_rgb is wave-uniform and re-read from the scalar cache every pose: 384 values hoisted out of the loop would not fit the scalar
    // registers (the compiler then parks them in vector lanes); the opaque zero keeps the loads inside
    int wo = 0;
    asm volatile("" : "+s"(wo));
    const float *w = packed + kOffRgbW + wo;
    // rgb_head's chain over nerf_mlp.cuh's pre-activation, written out: through the call the optimised IR of this kernel is the same
    // instruction for instruction, but the module then declares its intrinsics in another order and the backend allocates 174 VGPRs
    // for 166 -- two waves per SIMD for three, and 16 % more time per pose
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) {
      const float v = head_relu(head_pre(g[j], c[j]));
      r0 = fmaf(w[j], v, r0);
      r1 = fmaf(w[kHalf + j], v, r1);
      r2 = fmaf(w[2 * kHalf + j], v, r2);
    }
    a0 += 1.0f / (1.0f + expf(-(r0 + b0)));
    a1 += 1.0f / (1.0f + expf(-(r1 + b1)));
    a2 += 1.0f / (1.0f + expf(-(r2 + b2)));
  }
  if (pr < ga.num_points) {
    const float n = (float)num_poses;
    float *o = out + out_index(ga, pr);
    o[0] = a0 / n;
    o[1] = a1 / n;
    o[2] = a2 / n;
  }
}

// the ten matrices of raw in the packed order: pts_linears 0 .. 7, feature_linear, W_f -> their segments; *src_end: where the small
// tensors start
int matrix_plan(int input_ch, PackPlan &plan, int64_t *src_end) {
  int n = 0;
  int64_t src = 0;
  for (int i = 0; i <= 9; ++i) {
    PackSeg s{};
    s.dst = off_layer(i);
    s.src = src;
    s.n_out = i == 9 ? kHalf : kW;
    if (i == 0) {
      s.ka = input_ch, s.ka_pad = kEnc, s.kb = 0;
    } else if (i == kSkipLayer) {
      s.ka = input_ch, s.ka_pad = kEnc, s.kb = kW;
    } else {
      s.ka = 0, s.ka_pad = 0, s.kb = kW;
    }
    s.ld_o = s.ka + s.kb, s.ld_k = 1;
    src += (int64_t)s.n_out * s.ld_o;
    plan.seg[n++] = s;
  }
  *src_end = src;
  return n;
}

// split: the bf16x3 planes of packed, and the trunk runs in that arithmetic; null: in fp32.  The head is the same kernel either way
int grid_query(const float *xs, const float *ys, const float *zs, int res_x, int res_y, int res_z, float center_x, float center_y,
               float center_z, float bb_scale, int multires, const float *packed, const uint4 *split, const float *ctab, int num_poses,
               int layout, int64_t chunk, void *work, int64_t work_bytes, float *out, nrpn_stream_t stream) {
  NRPN_REQUIRE(xs && ys && zs && packed && ctab && work && out, "nerfgrid_query: null pointer");
  NRPN_REQUIRE(res_x >= 1 && res_y >= 1 && res_z >= 1, "nerfgrid_query: resolution %d x %d x %d", res_x, res_y, res_z);
  NRPN_REQUIRE(model_ok(multires, 0, 0), "nerfgrid_query: multires %d does not fit %d encoding columns", multires, kEnc);
  NRPN_REQUIRE(num_poses >= 1, "nerfgrid_query: no poses");
  NRPN_REQUIRE(layout == 0 || layout == 1, "nerfgrid_query: layout %d", layout);
  const int64_t n = (int64_t)res_x * res_y * res_z;
  NRPN_REQUIRE(n < ((int64_t)1 << 40), "nerfgrid_query: too many points");
  NRPN_REQUIRE(chunk >= 1, "nerfgrid_query: chunk %lld", (long long)chunk);
  const int64_t chunk_tiles = cdiv64(chunk < n ? chunk : n, kTile);
  NRPN_REQUIRE(chunk_tiles <= 0x7fffffff, "nerfgrid_query: chunk too large");
  NRPN_REQUIRE(work_bytes >= chunk_tiles * kTile * kHalf * 4, "nerfgrid_query: work buffer of %lld bytes is too small",
               (long long)work_bytes);
  GridArgs ga{xs, ys, zs, res_x, res_y, res_z, center_x, center_y, center_z, bb_scale, n, layout};
  float *gbuf = static_cast<float *>(work);
  for (int64_t p0 = 0; p0 < n; p0 += chunk_tiles * kTile) {
    const int64_t left = n - p0;
    const int tiles = (int)(left < chunk_tiles * kTile ? cdiv64(left, kTile) : chunk_tiles);
    if (int rc = launch_trunk(GridTile{ga, multires, p0, out}, tiles, packed, split, gbuf, as_stream(stream))) return rc;
    nerfgrid_head_kernel<<<tiles, kTile, 0, as_stream(stream)>>>(ga, packed, p0, gbuf, ctab, num_poses, out);
    NRPN_LAUNCH_CHECK("nerfgrid_head_kernel");
  }
  return NRPN_OK;
}

}  // namespace

int nerfmlp::launch_pack(const float *raw, const PackPlan &plan, int segs, float *packed, unsigned short *planes, int64_t lo_plane,
                         hipStream_t stream) {
  if (packed)
    nerfmlp_pack_kernel<<<dim3(64, segs), 256, 0, stream>>>(raw, packed, plan);
  else
    nerfmlp_pack_split_kernel<<<dim3(64, segs), 256, 0, stream>>>(raw, planes, lo_plane, plan);
  NRPN_LAUNCH_CHECK(packed ? "nerfmlp_pack_kernel" : "nerfmlp_pack_split_kernel");
  return NRPN_OK;
}

extern "C" {

int64_t nrpn_nerfgrid_work_bytes(int what, int64_t num_points) {
  if (what == 0) return kPackedFloats * 4;
  if (what == 2) return kSplitElems * 2;
  if (what == 1 && num_points > 0) return cdiv64(num_points, kTile) * kTile * kHalf * 4;
  return -1;
}

int nrpn_nerfgrid_pack(const float *raw, int input_ch, float *packed, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && packed, "nerfgrid_pack: null pointer");
  NRPN_REQUIRE(input_ch >= 3 && input_ch <= kEnc, "nerfgrid_pack: input_ch %d outside 3 .. %d", input_ch, kEnc);
  PackPlan plan{};
  int64_t src = 0;
  int n = matrix_plan(input_ch, plan, &src);
  const int64_t small[5][2] = {{kOffBias, 9 * kW}, {kOffAlphaW, kW}, {kOffAlphaB, 1}, {kOffRgbW, 3 * kHalf}, {kOffRgbB, 3}};
  for (int i = 0; i < 5; ++i) {
    PackSeg s{};
    s.dst = small[i][0];
    s.src = src;
    s.kb = (int)small[i][1];
    src += s.kb;
    plan.seg[n++] = s;
  }
  NRPN_HIP(hipMemsetAsync(packed, 0, kPackedFloats * 4, as_stream(stream)));
  return launch_pack(raw, plan, n, packed, nullptr, 0, as_stream(stream));
}

int nrpn_nerfgrid_pack_bf16x3(const float *raw, int input_ch, void *planes, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && planes, "nerfgrid_pack_bf16x3: null pointer");
  NRPN_REQUIRE(input_ch >= 3 && input_ch <= kEnc, "nerfgrid_pack_bf16x3: input_ch %d outside 3 .. %d", input_ch, kEnc);
  PackPlan plan{};
  int64_t src = 0;
  const int n = matrix_plan(input_ch, plan, &src);
  return launch_pack(raw, plan, n, nullptr, static_cast<unsigned short *>(planes), kSplitPlane, as_stream(stream));
}

int nrpn_nerfgrid_query(const float *xs, const float *ys, const float *zs, int res_x, int res_y, int res_z, float center_x,
                        float center_y, float center_z, float bb_scale, int multires, const float *packed, const float *ctab,
                        int num_poses, int layout, int64_t chunk, void *work, int64_t work_bytes, float *out, nrpn_stream_t stream) {
  return grid_query(xs, ys, zs, res_x, res_y, res_z, center_x, center_y, center_z, bb_scale, multires, packed, nullptr, ctab, num_poses,
                    layout, chunk, work, work_bytes, out, stream);
}

int nrpn_nerfgrid_query_bf16x3(const float *xs, const float *ys, const float *zs, int res_x, int res_y, int res_z, float center_x,
                               float center_y, float center_z, float bb_scale, int multires, const float *packed, const void *split,
                               const float *ctab, int num_poses, int layout, int64_t chunk, void *work, int64_t work_bytes, float *out,
                               nrpn_stream_t stream) {
  NRPN_REQUIRE(split, "nerfgrid_query: null pointer");
  return grid_query(xs, ys, zs, res_x, res_y, res_z, center_x, center_y, center_z, bb_scale, multires, packed,
                    static_cast<const uint4 *>(split), ctab, num_poses, layout, chunk, work, work_bytes, out, stream);
}

}  // extern "C"
