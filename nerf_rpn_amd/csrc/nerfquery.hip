// The NeRF MLP query as a differentiable operation (ops.nerf_query; reference data/scannet/run_nerf.py: run_network :50-65 as
// network_query_fn, and what loss.backward() of train_nerf :848-849 computes below it).  DESIGN.md 3.20.
//
// Forward, per chunk of points:
//   rays     one workgroup per ray: embed_dirs(viewdir), c_r = W_d embed_dirs + W_c cam + b of views_linears.0
//   trunk    the shared MFMA trunk (nerf_mlp.cuh) over (pts - centre) * scale -> raw sigma and g = W_f f
//   head     one thread per point: v = relu(g + c_r), raw rgb = W_rgb v + b_rgb
// embed_dirs, c_r (view_row) and the head's chains (rgb_head) are nerf_mlp.cuh's, the ones nerfrender.hip runs: on a render's points
// and on view directions formed as unit_dir forms them, raw is the render's bit for bit.
// Backward, per chunk of points, for the cotangent draw [points][4] (nothing is kept between forward and backward):
//   trunk    again, with a sink that keeps the encoding e, h_0 .. h_7 and f of every point of the chunk
//   headbwd  one thread per point: v and dv = (W_rgb^T draw_rgb) [g + c_r > 0], the head's cotangent rows (draw_rgb, dsigma) and
//            the point's [embed_dirs | cam] row
//   dgrad    dX = dY W on the MFMA with W^T packed like the forward weights (nrpn_nerfquery_pack_t: segments of the one pack of
//            nerf_mlp.cuh, run by nerfgrid.hip's kernels), one layer per launch:
//            df = W_f^T dv; dy_7 = (W_feat^T df + dsigma w_alpha) [h_7 > 0]; dy_{i-1} = (W_i[:, h part]^T dy_i) [h_{i-1} > 0].
//            Each result replaces, element for element, the activation whose mask it took (df replaces f).
//   wgrad    dW = dY^T X on the MFMA, the points of the chunk cut into kSlices slices of whole tiles; a wave owns a 64 x 64 block of
//            dW for one slice and adds its points in order; the bias gradient is the column sum of dY, taken by the same waves
//   reduce   adds the slices in slice order in float64 into the float64 gradient, chunk after chunk
// and finish: dcam = W_c^T db_views, everything rounded to float32.  No atomics: for a given chunk size every sum has a fixed order.
//
// backward_dtype "bf16x3" (DESIGN.md 3.24): the dgrads and the wgrads of the trunk's ten matrices run in the split arithmetic of the
// forward (nerf_mlp.cuh) on v_mfma_f32_32x32x16_bf16 -- dgrad on the pre-split planes of W^T (nrpn_nerfquery_pack_t_bf16x3), wgrad on
// operands split on their way through LDS; the column sums of dY are taken from the unsplit dY in the order of the fp32 wgrad.
#include "nerf_mlp.cuh"

namespace {

using namespace nerfmlp;

constexpr int kSlices = 64;           // of a chunk's points in wgrad
constexpr int kHeadCols = 64;         // the head's cotangent rows: draw_rgb, dsigma, zeros (one 64-column block of wgrad)
constexpr int kLdT = kHalf + 1;       // bank skew of headbwd's transposing tile

// packed transposes, in floats: 0 .. 6 pts_linears.1 .. 7 (h part), 7 feature_linear, 8 W_f
constexpr int64_t kSzT = (int64_t)kW * kW;
constexpr int64_t kOffTf = 8 * kSzT;
constexpr int64_t kPackedTFloats = kOffTf + (int64_t)kHalf * kW;

struct Model {
  int multires, multires_views, cam_ch;
  bool ok() const { return model_ok(multires, multires_views, cam_ch); }
  int input_ch() const { return 3 + 6 * multires; }
  int views_ch() const { return 3 + 6 * multires_views; }
  int ldv() const { return views_ch() + cam_ch; }                          // view and camera columns of views_linears.0
  int kv() const { return ldv() ? (ldv() + 63) / 64 * 64 : 64; }          // ... padded to 64-column blocks, at least one
};

// the gradient as one array, in floats: every tensor in torch's layout
struct GradLayout {
  int64_t w_pts[kLayers], w_feat, w_alpha, w_views, w_rgb, b_pts[kLayers], b_feat, b_alpha, b_views, b_rgb, cam, total;
};
GradLayout grad_layout(const Model &m) {
  GradLayout g{};
  int64_t at = 0;
  for (int i = 0; i < kLayers; ++i) {
    g.w_pts[i] = at;
    at += (int64_t)kW * (i == 0 ? m.input_ch() : i == kSkipLayer ? m.input_ch() + kW : kW);
  }
  g.w_feat = at, at += kSzT;
  g.w_alpha = at, at += kW;
  g.w_views = at, at += (int64_t)kHalf * (kW + m.ldv());
  g.w_rgb = at, at += 3 * kHalf;
  for (int i = 0; i < kLayers; ++i) g.b_pts[i] = at, at += kW;
  g.b_feat = at, at += kW;
  g.b_alpha = at, at += 1;
  g.b_views = at, at += kHalf;
  g.b_rgb = at, at += 3;
  g.cam = at, at += m.cam_ch;
  g.total = at;
  return g;
}

// ---- rays ------------------------------------------------------------------------------------------------------------------------
// One workgroup of 128 threads per ray: ctab [ray][128] = nerf_mlp.cuh's view_row of the given viewdir, the row nerfrender's head
// forms; xv [ray][kv] = [embed_dirs | cam | 0]
__global__ __launch_bounds__(kHalf) void nerfquery_rays_kernel(const float *__restrict__ viewdirs, const float *__restrict__ w_view,
                                                               const float *__restrict__ b_view, const float *__restrict__ cam,
                                                               int multires_views, int cam_ch, int kv, float *__restrict__ ctab,
                                                               float *__restrict__ xv) {
  __shared__ float emb[kMaxViewsCh];
  const int j = threadIdx.x;
  const int64_t ray = blockIdx.x;
  const int views_ch = 3 + 6 * multires_views, ldv = views_ch + cam_ch;
  if (j == 0) {
    const float vd[3] = {viewdirs[ray * 3], viewdirs[ray * 3 + 1], viewdirs[ray * 3 + 2]};
    embed_dirs(emb, vd, multires_views);
  }
  __syncthreads();
  ctab[ray * kHalf + j] = view_row(j, w_view, b_view, cam, emb, views_ch, cam_ch);
  if (xv)
    for (int k = j; k < kv; k += kHalf) xv[ray * kv + k] = k < views_ch ? emb[k] : k < ldv ? cam[k - views_ch] : 0.f;
}

// ---- trunk (kernel: nerf_mlp.cuh) ------------------------------------------------------------------------------------------------
struct Points {
  const float *pts;       // [num_points][3], world
  int64_t num_points;     // of the whole call
  int S;                  // points per ray
  float cx, cy, cz, scale;
};

struct PointSrc {
  const Points &pp;
  int64_t tile0;
  __device__ __forceinline__ void point(int i, float (&p)[3]) const {
    int64_t pi = tile0 + i;
    if (pi > pp.num_points - 1) pi = pp.num_points - 1;       // a partial tile repeats the last point; nothing of it is stored
    const float c[3] = {pp.cx, pp.cy, pp.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fmul_rn(__fsub_rn(pp.pts[pi * 3 + a], c[a]), pp.scale);
  }
};

// what the backward keeps of a chunk, row = point of the chunk (whole tiles; the rows past the last point hold a repeated point)
struct Kept {
  float *enc;             // [rows][64]
  float *h;               // [8][rows][256]; then dy_i in place
  float *f;               // [rows][256]; then df in place
  int64_t rows;
};

struct KeepSink {
  static constexpr bool kKeeps = true;
  Kept k;
  int64_t row0;           // of the tile in the chunk
  __device__ __forceinline__ void sigma(int, float) const {}
  __device__ __forceinline__ void keep(int layer, const float *act) const {
    const int t = threadIdx.x;
    if (layer < 0) {
      for (int idx = t; idx < kTile * (kEnc / 4); idx += 256) {
        const int row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4 *>(k.enc + (row0 + row) * kEnc + 4 * c4) = *reinterpret_cast<const float4 *>(act + row * kLd + 4 * c4);
      }
      return;
    }
    float *dst = layer < kLayers ? k.h + (int64_t)layer * k.rows * kW : k.f;
    for (int idx = t; idx < kTile * (kW / 4); idx += 256) {
      const int row = idx >> 6, c4 = idx & 63;
      *reinterpret_cast<float4 *>(dst + (row0 + row) * kW + 4 * c4) = *reinterpret_cast<const float4 *>(act + row * kLd + kEnc + 4 * c4);
    }
  }
};

// the tiles of a chunk that starts at point point0: the forward's, and the backward's, which keeps what this forward computed
struct PointTile {
  Points pp;
  int multires;
  int64_t point0;
  float *raw;             // [num_points][4]
  __device__ __forceinline__ PointSrc src(unsigned block) const { return {pp, point0 + (int64_t)block * kTile}; }
  __device__ __forceinline__ RawSink sink(unsigned block) const { return {point0 + (int64_t)block * kTile, pp.num_points, raw}; }
};
struct KeepTile {
  Points pp;
  int multires;
  int64_t point0;
  Kept kept;
  __device__ __forceinline__ PointSrc src(unsigned block) const { return {pp, point0 + (int64_t)block * kTile}; }
  __device__ __forceinline__ KeepSink sink(unsigned block) const { return {kept, (int64_t)block * kTile}; }
};

// ---- head ------------------------------------------------------------------------------------------------------------------------
// One workgroup of 64 threads, one tile; nerf_mlp.cuh's rgb_head with g streamed from gbuf, eight columns in flight
__global__ __launch_bounds__(kTile) void nerfquery_head_kernel(Points pp, const float *__restrict__ packed, const float *__restrict__ ctab,
                                                               int64_t point0, const float *__restrict__ gbuf, float *__restrict__ raw) {
  const int t = threadIdx.x;
  const int64_t pi = point0 + (int64_t)blockIdx.x * kTile + t;
  const int64_t pc = pi < pp.num_points ? pi : pp.num_points - 1;
  const float *c = ctab + (pc / pp.S) * kHalf;
  const float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + t;
  float r[3];
  rgb_head<false, 8>([&](int j) { return gt[j * kTile]; }, c, packed + kOffRgbW, r, nullptr);
  if (pi < pp.num_points) rgb_store(raw + pi * 4, r, packed);
}

// what headbwd writes, row = point of the chunk; the rows past the last point are zero in dv and dyhead
struct HeadOut {
  float *v, *dv;          // [rows][128]
  float *dyhead;          // [rows][64]: draw_rgb, dsigma, zeros
  float *xvp;             // [rows][kv]: the ray's [embed_dirs | cam | 0]
};

// One workgroup of 64 threads, one tile.  v and the relu's derivative come from the head's own head_pre (nerf_mlp.cuh).
__global__ __launch_bounds__(kTile) void nerfquery_headbwd_kernel(Points pp, const float *__restrict__ packed,
                                                                  const float *__restrict__ ctab, const float *__restrict__ xv, int kv,
                                                                  int64_t point0, const float *__restrict__ gbuf,
                                                                  const float *__restrict__ draw, HeadOut o) {
  __shared__ float tile[kTile * kLdT];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int64_t pi = point0 + row0 + t;
  const bool in = pi < pp.num_points;
  const int64_t pc = in ? pi : pp.num_points - 1;
  const int64_t ray = pc / pp.S;
  const float *c = ctab + ray * kHalf;
  const float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + t;
  const float *w = packed + kOffRgbW;
  const float d0 = in ? draw[pi * 4] : 0.f, d1 = in ? draw[pi * 4 + 1] : 0.f, d2 = in ? draw[pi * 4 + 2] : 0.f;
  const float ds = in ? draw[pi * 4 + 3] : 0.f;
  // v, then dv, through the transposing tile: a thread computes a row, the workgroup stores rows coalesced
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 8
    for (int j = 0; j < kHalf; ++j) {
      const float pre = head_pre(gt[j * kTile], c[j]);
      float val;
      if (pass == 0) {
        val = head_relu(pre);
      } else {
        const float s = fmaf(w[2 * kHalf + j], d2, fmaf(w[kHalf + j], d1, w[j] * d0));
        val = head_on(pre) ? s : 0.f;
      }
      tile[t * kLdT + j] = val;
    }
    __syncthreads();
    float *dst = (pass == 0 ? o.v : o.dv) + row0 * kHalf;
    for (int idx = t; idx < kTile * kHalf; idx += kTile) dst[idx] = tile[(idx >> 7) * kLdT + (idx & (kHalf - 1))];
    __syncthreads();
  }
  // the point's own rows of dyhead and xvp
  float4 *dh = reinterpret_cast<float4 *>(o.dyhead + (row0 + t) * kHeadCols);
  dh[0] = make_float4(d0, d1, d2, ds);
  for (int k = 1; k < kHeadCols / 4; ++k) dh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 *xs = reinterpret_cast<const float4 *>(xv + ray * kv);
  float4 *xd = reinterpret_cast<float4 *>(o.xvp + (row0 + t) * kv);
  for (int k = 0; k < kv / 4; ++k) xd[k] = xs[k];
}

// ---- dgrad -----------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads, one tile: out[p][0 .. 255] = (sum_n dy[p][n] W[n][.] + dsig[p] * alpha_w[.]) [mask[p][.] > 0].  dy
// [rows][K], K = 128 or 256; wt: the packed W^T; dsig: column 3 of dyhead, or null; mask [rows][256] or null; out may be mask.
__global__ __launch_bounds__(256) void nerfquery_dgrad_kernel(const float *__restrict__ dy, int K, const float *__restrict__ wt,
                                                              const float *__restrict__ dyhead, const float *__restrict__ alpha_w,
                                                              const float *mask, float *out) {
  extern __shared__ __align__(16) float act[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int k4 = K >> 2;
  for (int idx = t; idx < kTile * k4; idx += 256) {
    const int row = idx / k4, c4 = idx - row * k4;
    *reinterpret_cast<float4 *>(act + row * kLd + kEnc + 4 * c4) = *reinterpret_cast<const float4 *>(dy + (row0 + row) * K + 4 * c4);
  }
  __syncthreads();
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][c][e] = 0.f;
  const int col0 = wave * 64;
  gemm_tile<2>(act, kEnc, K, reinterpret_cast<const float4 *>(wt), kW, col0, acc);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = col0 + 32 * c + r;
    const float aw = dyhead ? alpha_w[col] : 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t row = row0 + 32 * m + acc_row(e, h);
        float v = acc[m][c][e];
        if (dyhead) v = fmaf(dyhead[row * kHeadCols + 3], aw, v);
        if (mask) v = mask[row * kW + col] > 0.f ? v : 0.f;
        out[row * kW + col] = v;
      }
  }
}

// The same product in the bf16x3 arithmetic: dy split in registers as the forward splits its activations, wt_hi / wt_lo the planes of the
// packed W^T (nrpn_nerfquery_pack_t_bf16x3); the epilogue's arithmetic (the dsigma w_alpha fmaf, the relu mask) is the fp32 kernel's.
// Memory is walked as the trunk's keep() walks it: the tile's loads are all issued before the first is stored to the image, the
// result goes back through the image, and a thread then takes whole float4 of a row -- its 16 mask loads first, then its 16 stores
// (out may be mask; an element is read and written by the same thread only).
// K = 128 without a mask (df) or 256 with one.
template <int K, bool kMask>
__global__ __launch_bounds__(256) void nerfquery_dgrad_split_kernel(const float *__restrict__ dy, const uint4 *__restrict__ wt_hi,
                                                                    const uint4 *__restrict__ wt_lo, const float *__restrict__ dyhead,
                                                                    const float *__restrict__ alpha_w, const float *mask, float *out) {
  constexpr int kInVec = kTile * (K / 4) / 256, kOutVec = kTile * (kW / 4) / 256;       // float4 per thread of the dy and the out tile
  extern __shared__ __align__(16) float act[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  {
    float4 v[kInVec];
#pragma unroll
    for (int i = 0; i < kInVec; ++i) {
      const int idx = t + 256 * i;
      v[i] = *reinterpret_cast<const float4 *>(dy + (row0 + idx / (K / 4)) * K + 4 * (idx % (K / 4)));
    }
#pragma unroll
    for (int i = 0; i < kInVec; ++i) {
      const int idx = t + 256 * i;
      *reinterpret_cast<float4 *>(act + idx / (K / 4) * kLd + kEnc + 4 * (idx % (K / 4))) = v[i];
    }
  }
  __syncthreads();
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][c][e] = 0.f;
  const int col0 = wave * 64;
  gemm_tile_split<2>(act, kEnc, K, wt_hi, wt_lo, kW, col0, acc);
  float ds[2][16];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) ds[m][e] = dyhead ? dyhead[(row0 + 32 * m + acc_row(e, h)) * kHeadCols + 3] : 0.f;
  __syncthreads();                                            // every wave has read dy
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = col0 + 32 * c + r;
    const float aw = dyhead ? alpha_w[col] : 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = acc[m][c][e];
        if (dyhead) v = fmaf(ds[m][e], aw, v);
        act[(32 * m + acc_row(e, h)) * kLd + kEnc + col] = v;
      }
  }
  float4 mk[kOutVec];
  if constexpr (kMask) {
#pragma unroll
    for (int i = 0; i < kOutVec; ++i) {
      const int idx = t + 256 * i;
      mk[i] = *reinterpret_cast<const float4 *>(mask + (row0 + (idx >> 6)) * kW + 4 * (idx & 63));
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kOutVec; ++i) {
    const int idx = t + 256 * i, row = idx >> 6, c4 = idx & 63;
    float4 v = *reinterpret_cast<const float4 *>(act + row * kLd + kEnc + 4 * c4);
    if constexpr (kMask) {
      v.x = mk[i].x > 0.f ? v.x : 0.f;
      v.y = mk[i].y > 0.f ? v.y : 0.f;
      v.z = mk[i].z > 0.f ? v.z : 0.f;
      v.w = mk[i].w > 0.f ? v.w : 0.f;
    }
    *reinterpret_cast<float4 *>(out + (row0 + row) * kW + 4 * c4) = v;
  }
}

// ---- wgrad -----------------------------------------------------------------------------------------------------------------------
constexpr int kWgSteps = 8;           // point pairs per register set
struct WgFrag {
  float a0[kWgSteps], a1[kWgSteps], b0[kWgSteps], b1[kWgSteps];
};
__device__ __forceinline__ void wg_load(WgFrag &f, const float *__restrict__ ap, const float *__restrict__ bp, int ldy, int ldx) {
#pragma unroll
  for (int s = 0; s < kWgSteps; ++s) {
    f.a0[s] = ap[(int64_t)2 * s * ldy];
    f.a1[s] = ap[(int64_t)2 * s * ldy + 32];
    f.b0[s] = bp[(int64_t)2 * s * ldx];
    f.b1[s] = bp[(int64_t)2 * s * ldx + 32];
  }
}
__device__ __forceinline__ void wg_mma(const WgFrag &f, f32x16 (&acc)[2][2], bool sums, double &bs0, double &bs1) {
#pragma unroll
  for (int s = 0; s < kWgSteps; ++s) {
    if (sums) {
      bs0 += (double)f.a0[s];
      bs1 += (double)f.a1[s];
    }
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a0[s], f.b0[s], acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a0[s], f.b1[s], acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a1[s], f.b0[s], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a1[s], f.b1[s], acc[1][1], 0, 0, 0);
  }
}

// dW = dY^T X over the rows of one slice.  dy [rows][ldy], n columns used; x [rows][ldx], kpad columns used (n, kpad multiples of 64).
// A wave owns the 64 x 64 block (nb, kb) of dW for slice blockIdx.y: per pair of points one A and one B value per lane and accumulator
// row / column block, four MFMAs.  partial [slice][n][kpad]; bias (or null) f64 [slice][2][n]: the column sums of dY over the even and
// the odd rows of the slice, added in float64 by the waves with kb = 0 (a bias gradient has no product to hide a float32 sum's
// rounding behind, and the checker's bound on it is a few ulp).
__global__ __launch_bounds__(256) void nerfquery_wgrad_kernel(const float *__restrict__ dy, int ldy, int n, const float *__restrict__ x,
                                                              int ldx, int kpad, int64_t rows, int64_t rows_per_slice,
                                                              float *__restrict__ partial, double *__restrict__ bias) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int kblocks = kpad >> 6;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= (n >> 6) * kblocks) return;
  const int nb = blk / kblocks, kb = blk - nb * kblocks;
  const int64_t slice = blockIdx.y;
  int64_t p0 = slice * rows_per_slice, p1 = p0 + rows_per_slice;
  if (p0 > rows) p0 = rows;
  if (p1 > rows) p1 = rows;
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][c][e] = 0.f;
  double bs0 = 0.0, bs1 = 0.0;
  const bool sums = bias && kb == 0;
  const float *ap = dy + (p0 + h) * ldy + nb * 64 + r;
  const float *bp = x + (p0 + h) * ldx + kb * 64 + r;
  // blocks of kWgSteps point pairs; two register sets alternate as in gemm_tile, so the loads of block n + 1 are in flight during the
  // MFMAs of block n.  Rows come in whole tiles: the block count is a multiple of 4, or 0 for an empty slice
  const int blocks = (int)((p1 - p0) / (2 * kWgSteps));
  WgFrag f0, f1;
  if (blocks > 0) wg_load(f0, ap, bp, ldy, ldx);
  for (int blk = 0; blk < blocks; blk += 2) {
    wg_load(f1, ap + (int64_t)(blk + 1) * 2 * kWgSteps * ldy, bp + (int64_t)(blk + 1) * 2 * kWgSteps * ldx, ldy, ldx);
    __builtin_amdgcn_sched_barrier(0);
    wg_mma(f0, acc, sums, bs0, bs1);
    __builtin_amdgcn_sched_barrier(0);
    const int nx = blk + 2 < blocks ? blk + 2 : blk;            // the last iteration reloads its own block: in bounds, unused
    wg_load(f0, ap + (int64_t)nx * 2 * kWgSteps * ldy, bp + (int64_t)nx * 2 * kWgSteps * ldx, ldy, ldx);
    __builtin_amdgcn_sched_barrier(0);
    wg_mma(f1, acc, sums, bs0, bs1);
    __builtin_amdgcn_sched_barrier(0);
  }
  float *out = partial + slice * n * kpad;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        out[(int64_t)(nb * 64 + 32 * m + acc_row(e, h)) * kpad + kb * 64 + 32 * c + r] = acc[m][c][e];
  if (sums) {
    double *b = bias + (slice * 2 + h) * n + nb * 64 + r;
    b[0] = bs0;
    b[32] = bs1;
  }
}

// ---- wgrad in the bf16x3 arithmetic ------------------------------------------------------------------------------------------------
// The summed index is the point, and the bf16 MFMA wants a lane to hold 8 consecutive points of one channel, while dY and X are
// [point][channel].  A workgroup therefore stages blocks of kWsPts points of the 320 channels its four waves need -- 64 of one
// operand and 256 of the other -- through LDS: a thread reads 8 consecutive points of one channel (a wave: 64 consecutive channels of a
// row, coalesced), splits them once and stores the 16 bytes of each plane at [channel][point].  A channel row is 80 bytes: the 16
// lanes a ds_read_b128 serves together read rows r, r + 1, .. at 16 distinct 16-byte slots of the 256-byte bank window, and so do
// the 8 lanes of a ds_write_b128 in its 128-byte one.  Two LDS images alternate; the next block's global loads are issued before the
// current block's MFMAs and split and stored after them, so one barrier per block suffices.
constexpr int kWsPts = 32;                                   // points per block: two k-steps of the MFMA
constexpr int kWsCols = 320;                                 // staged channels, dY's first
constexpr int kWsRow = kWsPts + 8;                           // bf16 per channel row of a plane
constexpr int kWsOct = kWsCols * (kWsPts / 8) / 256;         // (channel, 8 points) pieces per thread and block: 5
constexpr int kWsPlane = kWsCols * kWsRow;                   // bf16 per plane
constexpr int kWsLdsBytes = 2 * 2 * kWsPlane * 2;            // two images of two planes: 102400
static_assert(kSlices % 8 == 0, "nerfquery_wgrad_split_kernel spreads the slices over 8 XCDs");
static_assert(kTile % (2 * kWsPts) == 0, "a slice of whole tiles is whole pairs of blocks: the two LDS images alternate in pairs");

struct WsPiece {            // one thread's share of a block, unsplit
  float v[kWsOct][8];
};

// As nerfquery_wgrad_kernel without the column sums, kpad 256 or 64, grid (blocks / 4, kSlices): the four waves of a slice's workgroup
// ``group`` own the blocks (nb, kb) = (group, wave) of a 256-column X, or (4 group + wave, 0) of a 64-column one.  Per 16 points a
// wave adds hi hi, hi lo, lo hi of its 64 x 64 block into the same fp32 accumulators, the points in order.
__global__ __launch_bounds__(256) void nerfquery_wgrad_split_kernel(const float *__restrict__ dy, int ldy, int n, const float *__restrict__ x,
                                                                    int ldx, int kpad, int64_t rows, int64_t rows_per_slice,
                                                                    float *__restrict__ partial) {
  extern __shared__ __align__(16) unsigned short ws[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const bool wide_x = kpad == 256;
  const int aw = wide_x ? 64 : 256;                          // staged columns of dY; the other 320 - aw are X's
  // The gridDim.x workgroups of a slice read the same rows of X.  Workgroups go to the 8 XCDs round-robin in launch order, so the
  // (column group, slice) of a workgroup is taken from its launch index such that a slice's workgroups share an XCD and its L2; which
  // workgroup computes a block changes no sum.
  const int launch = blockIdx.x + gridDim.x * blockIdx.y, xcd = launch & 7, in_xcd = launch >> 3;
  const int group = in_xcd % gridDim.x;
  const int64_t slice = xcd + 8 * (in_xcd / gridDim.x);
  const int a0 = group * aw;
  const int ai = wide_x ? 0 : wave, bi = wide_x ? wave : 0;  // the wave's 64-column block among the staged ones
  const int nb = (a0 >> 6) + ai, kb = bi;
  int64_t p0 = slice * rows_per_slice, p1 = p0 + rows_per_slice;
  if (p0 > rows) p0 = rows;
  if (p1 > rows) p1 = rows;
  const int blocks = (int)((p1 - p0) / kWsPts);              // rows come in whole tiles: a multiple of 2, or 0

  const float *src[kWsOct];
  int64_t ld[kWsOct];
  int at[kWsOct];                                            // of the piece in a plane, in bf16
#pragma unroll
  for (int i = 0; i < kWsOct; ++i) {
    const int q = i * 256 + t, c = q % kWsCols, pg = q / kWsCols;
    ld[i] = c < aw ? ldy : ldx;
    src[i] = (c < aw ? dy + a0 + c : x + (c - aw)) + (p0 + 8 * pg) * ld[i];
    at[i] = c * kWsRow + 8 * pg;
  }
  auto load = [&](WsPiece &w, int blk) {
#pragma unroll
    for (int i = 0; i < kWsOct; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) w.v[i][j] = src[i][((int64_t)blk * kWsPts + j) * ld[i]];
  };
  auto store = [&](const WsPiece &w, int image) {
    unsigned short *base = ws + image * 2 * kWsPlane;
#pragma unroll
    for (int i = 0; i < kWsOct; ++i) {
      bf16x8 hi, lo;
      split8(make_float4(w.v[i][0], w.v[i][1], w.v[i][2], w.v[i][3]), make_float4(w.v[i][4], w.v[i][5], w.v[i][6], w.v[i][7]), hi, lo);
      *reinterpret_cast<uint4 *>(base + at[i]) = __builtin_bit_cast(uint4, hi);
      *reinterpret_cast<uint4 *>(base + kWsPlane + at[i]) = __builtin_bit_cast(uint4, lo);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][c][e] = 0.f;
  const int a_at = (ai * 64 + r) * kWsRow + 8 * h, b_at = (aw + bi * 64 + r) * kWsRow + 8 * h;

  auto mma = [&](int image) {
    const unsigned short *img = ws + image * 2 * kWsPlane;
#pragma unroll
    for (int ks = 0; ks < kWsPts / 16; ++ks) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        ah[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(img + a_at + 32 * m * kWsRow + 16 * ks));
        al[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(img + kWsPlane + a_at + 32 * m * kWsRow + 16 * ks));
        bh[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(img + b_at + 32 * m * kWsRow + 16 * ks));
        bl[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(img + kWsPlane + b_at + 32 * m * kWsRow + 16 * ks));
      }
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int m = 0; m < 2; ++m)
            acc[m][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p == 2 ? al[m] : ah[m], p == 1 ? bl[c] : bh[c], acc[m][c], 0, 0, 0);
    }
  };

  // Blocks come in pairs.  Entering the even half of a pair image 0 holds block blk, wb block blk + 1 and wa's loads of block blk + 2
  // are in flight; each half stores the set loaded longest ago into the image read in the half before (behind that half's barrier),
  // re-issues that set three blocks ahead and then multiplies: two blocks of loads are in flight under every block of MFMAs.
  WsPiece wa, wb;
  if (blocks > 0) {
    load(wa, 0);
    load(wb, 1);
    store(wa, 0);
    if (blocks > 2) load(wa, 2);
  }
  __syncthreads();
  for (int blk = 0; blk < blocks; blk += 2) {
    store(wb, 1);
    if (blk + 3 < blocks) load(wb, blk + 3);
    mma(0);
    __syncthreads();
    if (blk + 2 < blocks) store(wa, 0);
    if (blk + 4 < blocks) load(wa, blk + 4);
    mma(1);
    __syncthreads();
  }
  float *out = partial + slice * n * kpad;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        out[(int64_t)(nb * 64 + 32 * m + acc_row(e, h)) * kpad + kb * 64 + 32 * c + r] = acc[m][c][e];
}

// bias f64 [slice][2][n] as nerfquery_wgrad_kernel leaves it, sum for sum: the column sums of the unsplit dY over the even and the odd
// rows of a slice, each added in row order in float64.  One thread per (slice, parity, column); rows come in whole tiles.
constexpr int kCsRows = 32;           // loads in flight per thread
__global__ __launch_bounds__(128) void nerfquery_colsum_kernel(const float *__restrict__ dy, int ldy, int n, int64_t rows,
                                                               int64_t rows_per_slice, double *__restrict__ bias) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), h = threadIdx.x >> 6;
  const int64_t slice = blockIdx.y;
  int64_t p0 = slice * rows_per_slice, p1 = p0 + rows_per_slice;
  if (p0 > rows) p0 = rows;
  if (p1 > rows) p1 = rows;
  const float *ap = dy + (p0 + h) * ldy + col;
  double s = 0.0;
  for (int64_t p = 0; p < p1 - p0; p += 2 * kCsRows) {
    float v[kCsRows];
#pragma unroll
    for (int j = 0; j < kCsRows; ++j) v[j] = ap[(p + 2 * j) * ldy];
#pragma unroll
    for (int j = 0; j < kCsRows; ++j) s += (double)v[j];
  }
  bias[(slice * 2 + h) * n + col] = s;
}

// gacc[dst + i * ld + j] += sum over the parts, in order, of partial[part][row_lo + i][col_lo + j], i < nr, j < nc; float64
template <class T>
__global__ void nerfquery_reduce_kernel(const T *__restrict__ partial, int parts, int n, int kpad, int row_lo, int nr, int col_lo,
                                        int nc, double *__restrict__ gacc, int64_t dst, int ld) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nr * nc) return;
  const int i = idx / nc, j = idx - i * nc;
  const T *p = partial + (int64_t)(row_lo + i) * kpad + col_lo + j;
  double s = 0.0;
#pragma unroll 16
  for (int q = 0; q < parts; ++q) s += (double)p[(int64_t)q * n * kpad];
  gacc[dst + (int64_t)i * ld + j] += s;
}

// grads[i] = (float)gacc[i]; before that dcam[k] = sum_j W_c[j][k] db_views[j] in j order
__global__ void nerfquery_finish_kernel(double *__restrict__ gacc, int64_t total, int64_t cam_at, int64_t b_views_at,
                                        const float *__restrict__ w_view, int views_ch, int cam_ch, float *__restrict__ grads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  double v = gacc[i];
  if (i >= cam_at && i < cam_at + cam_ch) {
    const int k = (int)(i - cam_at);
    v = 0.0;
    for (int j = 0; j < kHalf; ++j) v += (double)w_view[j * (views_ch + cam_ch) + views_ch + k] * gacc[b_views_at + j];
  }
  grads[i] = (float)v;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The nine transposes as segments of nerf_mlp.cuh's pack (raw: nrpn_nerfgrid_pack's): k runs over W's rows and the output column o
// over W's 256 columns from col_off, so the fragment element of (k, o) holds W[k][col_off + o].  Splitting commutes with transposing:
// element for element the planes hold the values of the forward's planes.
constexpr int kPackTSegs = 9;
PackPlan pack_t_plan(int input_ch) {
  PackPlan plan{};
  int64_t src = (int64_t)kW * input_ch;                       // after pts_linears.0
  for (int i = 1; i <= kPackTSegs; ++i) {                     // raw order: pts_linears 1 .. 7, feature_linear, W_f
    const int ld = i == kSkipLayer ? input_ch + kW : kW, K = i == 9 ? kHalf : kW;
    plan.seg[i - 1] = PackSeg{(int64_t)(i - 1) * kSzT, src, kW, 1, ld, i == kSkipLayer ? input_ch : 0, 0, 0, K};
    src += (int64_t)K * ld;
  }
  return plan;
}

struct QueryCall {
  Points pp;
  Model m;
  const float *viewdirs, *packed, *w_view, *b_view, *cam;
  int64_t num_rays, chunk;
  void *work;
  int64_t work_bytes;
  hipStream_t stream;
  const uint4 *split;       // the bf16x3 planes of packed: the trunk then runs in that arithmetic; null: fp32
  const uint4 *split_t;     // the bf16x3 planes of the packed transposes: the backward's dgrads and trunk wgrads then do too (with split)
  int64_t chunk_tiles() const { return cdiv64(chunk < pp.num_points ? chunk : pp.num_points, kTile); }
};

struct Layout {           // of the work buffer, in bytes; every part 16-byte aligned
  int64_t ctab, xv, gbuf, fwd_end;                                             // forward
  int64_t enc, h, f, v, dv, dyhead, xvp, partial, bias, gacc, total;           // backward
  int64_t rows;
};
Layout layout(const Model &m, int64_t num_rays, int64_t chunk_tiles) {
  Layout l{};
  l.rows = chunk_tiles * kTile;
  l.ctab = 0;
  l.xv = l.ctab + num_rays * kHalf * 4;
  l.gbuf = l.xv + align16(num_rays * m.kv() * 4);
  l.fwd_end = l.gbuf + l.rows * kHalf * 4;
  l.enc = l.fwd_end;
  l.h = l.enc + l.rows * kEnc * 4;
  l.f = l.h + l.rows * kLayers * kW * 4;
  l.v = l.f + l.rows * kW * 4;
  l.dv = l.v + l.rows * kHalf * 4;
  l.dyhead = l.dv + l.rows * kHalf * 4;
  l.xvp = l.dyhead + l.rows * kHeadCols * 4;
  l.partial = l.xvp + l.rows * m.kv() * 4;
  l.bias = l.partial + (int64_t)kSlices * (kW > m.kv() / 2 ? kW * kW : kHalf * m.kv()) * 4;
  l.gacc = l.bias + (int64_t)kSlices * 2 * kW * 8;
  l.total = l.gacc + align16(grad_layout(m).total * 8);
  return l;
}

int check(const char *who, const QueryCall &c, bool backward) {
  NRPN_REQUIRE(c.pp.pts && c.viewdirs && c.packed && c.w_view && c.b_view && c.work, "%s: null pointer", who);
  NRPN_REQUIRE(c.m.ok(), "%s: multires %d / multires_views %d / input_ch_cam %d", who, c.m.multires, c.m.multires_views, c.m.cam_ch);
  NRPN_REQUIRE(c.m.cam_ch == 0 || c.cam, "%s: input_ch_cam %d without an embedded_cam", who, c.m.cam_ch);
  NRPN_REQUIRE(query_sizes_ok(c.num_rays, c.pp.S, c.chunk), "%s: %lld rays of %d points in chunks of %lld", who, (long long)c.num_rays, c.pp.S,
               (long long)c.chunk);
  NRPN_REQUIRE(c.chunk_tiles() <= 0x7fffff, "%s: chunk too large", who);
  const Layout l = layout(c.m, c.num_rays, c.chunk_tiles());
  NRPN_REQUIRE(c.work_bytes >= (backward ? l.total : l.fwd_end), "%s: work buffer of %lld bytes is too small", who,
               (long long)c.work_bytes);
  return NRPN_OK;
}

int launch_rays(const QueryCall &c, const Layout &l, bool with_xv) {
  char *wk = static_cast<char *>(c.work);
  nerfquery_rays_kernel<<<(unsigned)c.num_rays, kHalf, 0, c.stream>>>(c.viewdirs, c.w_view, c.b_view, c.cam, c.m.multires_views, c.m.cam_ch,
                                                                      c.m.kv(), reinterpret_cast<float *>(wk + l.ctab),
                                                                      with_xv ? reinterpret_cast<float *>(wk + l.xv) : nullptr);
  NRPN_LAUNCH_CHECK("nerfquery_rays_kernel");
  return NRPN_OK;
}

// c.split (here and in backward): the trunk runs in the bf16x3 arithmetic on it; everything after it is the same
int forward(const QueryCall &c, float *raw) {
  if (int rc = check("nerfquery_forward", c, false)) return rc;
  NRPN_REQUIRE(raw, "nerfquery_forward: null output or planes");
  const Layout l = layout(c.m, c.num_rays, c.chunk_tiles());
  char *wk = static_cast<char *>(c.work);
  const float *ctab = reinterpret_cast<float *>(wk + l.ctab);
  float *gbuf = reinterpret_cast<float *>(wk + l.gbuf);
  if (int rc = launch_rays(c, l, false)) return rc;
  for (int64_t p0 = 0; p0 < c.pp.num_points; p0 += l.rows) {
    const int64_t left = c.pp.num_points - p0;
    const int tiles = (int)cdiv64(left < l.rows ? left : l.rows, kTile);
    if (int rc = launch_trunk(PointTile{c.pp, c.m.multires, p0, raw}, tiles, c.packed, c.split, gbuf, c.stream)) return rc;
    nerfquery_head_kernel<<<tiles, kTile, 0, c.stream>>>(c.pp, c.packed, ctab, p0, gbuf, raw);
    NRPN_LAUNCH_CHECK("nerfquery_head_kernel");
  }
  return NRPN_OK;
}

struct Wgrad {            // one product of the backward and where its rows and columns go
  const float *dy;
  int ldy, n;
  const float *x;
  int ldx, kpad;
  int row_lo, nr, nc;     // rows row_lo .. row_lo + nr of dW, columns 0 .. nc
  int64_t dst;            // of the first of them in the gradient
  int ld;
  int64_t bias_dst;       // of column sum row_lo, or -1
  bool trunk = false;     // one of the trunk's ten matrices: split when the backward is
};

// c.split_t (with c.split): the dgrads and the trunk's wgrads in the bf16x3 arithmetic too, on c.split_t in place of packed_t
int backward(const QueryCall &c, const float *packed_t, const float *draw, float *grads) {
  NRPN_REQUIRE(c.split || !c.split_t, "nerfquery_backward: the split backward belongs to the split forward");
  if (int rc = check("nerfquery_backward", c, true)) return rc;
  NRPN_REQUIRE((c.split_t || packed_t) && draw && grads, "nerfquery_backward: null pointer");
  if (c.split_t) {
    NRPN_LDS((nerfquery_dgrad_split_kernel<kHalf, false>), kLdsBytes);
    NRPN_LDS((nerfquery_dgrad_split_kernel<kW, true>), kLdsBytes);
    NRPN_LDS(nerfquery_wgrad_split_kernel, kWsLdsBytes);
  } else {
    NRPN_LDS(nerfquery_dgrad_kernel, kLdsBytes);
  }
  const Model &m = c.m;
  const Layout l = layout(m, c.num_rays, c.chunk_tiles());
  const GradLayout gl = grad_layout(m);
  char *wk = static_cast<char *>(c.work);
  auto F = [&](int64_t at) { return reinterpret_cast<float *>(wk + at); };
  const float *ctab = F(l.ctab), *xv = F(l.xv);
  float *gbuf = F(l.gbuf), *partial = F(l.partial);
  double *bias = reinterpret_cast<double *>(wk + l.bias);
  double *gacc = reinterpret_cast<double *>(wk + l.gacc);
  const Kept kept{F(l.enc), F(l.h), F(l.f), l.rows};
  const HeadOut ho{F(l.v), F(l.dv), F(l.dyhead), F(l.xvp)};
  const int kv = m.kv(), in_ch = m.input_ch();
  if (int rc = launch_rays(c, l, true)) return rc;
  NRPN_HIP(hipMemsetAsync(gacc, 0, gl.total * 8, c.stream));

  for (int64_t p0 = 0; p0 < c.pp.num_points; p0 += l.rows) {
    const int64_t left = c.pp.num_points - p0;
    const int tiles = (int)cdiv64(left < l.rows ? left : l.rows, kTile);
    const int64_t rows = (int64_t)tiles * kTile, rps = cdiv64(tiles, kSlices) * kTile;
    // h and f of this chunk are laid out for l.rows rows whatever the chunk's own count: Kept::rows is the stride of h's layers
    auto wgrad = [&](const Wgrad &w) -> int {
      const int blocks = (w.n >> 6) * (w.kpad >> 6);
      if (c.split_t && w.trunk) {
        NRPN_REQUIRE((w.kpad == kW || w.kpad == kEnc) && blocks % 4 == 0, "nerfquery_backward: a %d x %d split wgrad", w.n, w.kpad);
        nerfquery_wgrad_split_kernel<<<dim3(blocks / 4, kSlices), 256, kWsLdsBytes, c.stream>>>(w.dy, w.ldy, w.n, w.x, w.ldx, w.kpad, rows, rps,
                                                                                              partial);
        NRPN_LAUNCH_CHECK("nerfquery_wgrad_split_kernel");
        if (w.bias_dst >= 0) {
          nerfquery_colsum_kernel<<<dim3(w.n >> 6, kSlices), 128, 0, c.stream>>>(w.dy, w.ldy, w.n, rows, rps, bias);
          NRPN_LAUNCH_CHECK("nerfquery_colsum_kernel");
        }
      } else {
        nerfquery_wgrad_kernel<<<dim3((blocks + 3) / 4, kSlices), 256, 0, c.stream>>>(w.dy, w.ldy, w.n, w.x, w.ldx, w.kpad, rows, rps, partial,
                                                                                     w.bias_dst >= 0 ? bias : nullptr);
        NRPN_LAUNCH_CHECK("nerfquery_wgrad_kernel");
      }
      if (w.nc > 0) {
        nerfquery_reduce_kernel<float><<<(w.nr * w.nc + 255) / 256, 256, 0, c.stream>>>(partial, kSlices, w.n, w.kpad, w.row_lo, w.nr, 0, w.nc, gacc,
                                                                               w.dst, w.ld);
        NRPN_LAUNCH_CHECK("nerfquery_reduce_kernel");
      }
      if (w.bias_dst >= 0) {
        nerfquery_reduce_kernel<double><<<(w.nr + 255) / 256, 256, 0, c.stream>>>(bias, 2 * kSlices, 1, w.n, 0, 1, w.row_lo, w.nr, gacc, w.bias_dst,
                                                                         w.nr);
        NRPN_LAUNCH_CHECK("nerfquery_reduce_kernel");
      }
      return NRPN_OK;
    };
    auto dgrad = [&](const float *dy, int K, int64_t wt_at, bool alpha, const float *mask, float *out) -> int {
      if (c.split_t) {
        const uint4 *hi = c.split_t + wt_at / 8, *lo = c.split_t + (kPackedTFloats + wt_at) / 8;
        NRPN_REQUIRE((K == kHalf && !mask) || (K == kW && mask), "nerfquery_backward: a split dgrad of K %d", K);
        if (K == kHalf)
          nerfquery_dgrad_split_kernel<kHalf, false><<<tiles, 256, kLdsBytes, c.stream>>>(dy, hi, lo, alpha ? ho.dyhead : nullptr,
                                                                                        c.packed + kOffAlphaW, mask, out);
        else
          nerfquery_dgrad_split_kernel<kW, true><<<tiles, 256, kLdsBytes, c.stream>>>(dy, hi, lo, alpha ? ho.dyhead : nullptr,
                                                                                    c.packed + kOffAlphaW, mask, out);
        NRPN_LAUNCH_CHECK("nerfquery_dgrad_split_kernel");
      } else {
        nerfquery_dgrad_kernel<<<tiles, 256, kLdsBytes, c.stream>>>(dy, K, packed_t + wt_at, alpha ? ho.dyhead : nullptr,
                                                                    c.packed + kOffAlphaW, mask, out);
        NRPN_LAUNCH_CHECK("nerfquery_dgrad_kernel");
      }
      return NRPN_OK;
    };
    auto hl = [&](int i) { return kept.h + (int64_t)i * l.rows * kW; };

    if (int rc = launch_trunk(KeepTile{c.pp, m.multires, p0, kept}, tiles, c.packed, c.split, gbuf, c.stream)) return rc;
    nerfquery_headbwd_kernel<<<tiles, kTile, 0, c.stream>>>(c.pp, c.packed, ctab, xv, kv, p0, gbuf, draw, ho);
    NRPN_LAUNCH_CHECK("nerfquery_headbwd_kernel");
    // rgb_linear and alpha_linear: rows 0 .. 2 and row 3 of the head's cotangent
    if (int rc = wgrad({ho.dyhead, kHeadCols, kHeadCols, ho.v, kHalf, kHalf, 0, 3, kHalf, gl.w_rgb, kHalf, gl.b_rgb})) return rc;
    if (int rc = wgrad({ho.dyhead, kHeadCols, kHeadCols, hl(7), kW, kW, 3, 1, kW, gl.w_alpha, kW, gl.b_alpha})) return rc;
    // views_linears.0: the feature columns, then the view and camera columns
    const int ldw = kW + m.ldv();
    if (int rc = wgrad({ho.dv, kHalf, kHalf, kept.f, kW, kW, 0, kHalf, kW, gl.w_views, ldw, gl.b_views, true})) return rc;
    if (m.ldv() > 0)
      if (int rc = wgrad({ho.dv, kHalf, kHalf, ho.xvp, kv, kv, 0, kHalf, m.ldv(), gl.w_views + kW, ldw, -1})) return rc;
    if (int rc = dgrad(ho.dv, kHalf, kOffTf, false, nullptr, kept.f)) return rc;                          // df
    if (int rc = wgrad({kept.f, kW, kW, hl(7), kW, kW, 0, kW, kW, gl.w_feat, kW, gl.b_feat, true})) return rc;
    if (int rc = dgrad(kept.f, kW, 7 * kSzT, true, hl(7), hl(7))) return rc;                              // dy_7
    for (int i = kLayers - 1; i >= 1; --i) {
      const int ldi = i == kSkipLayer ? in_ch + kW : kW, hoff = i == kSkipLayer ? in_ch : 0;
      if (int rc = wgrad({hl(i), kW, kW, hl(i - 1), kW, kW, 0, kW, kW, gl.w_pts[i] + hoff, ldi, gl.b_pts[i], true})) return rc;
      if (i == kSkipLayer)
        if (int rc = wgrad({hl(i), kW, kW, kept.enc, kEnc, kEnc, 0, kW, in_ch, gl.w_pts[i], ldi, -1, true})) return rc;
      if (int rc = dgrad(hl(i), kW, (int64_t)(i - 1) * kSzT, false, hl(i - 1), hl(i - 1))) return rc;   // dy_{i-1}
    }
    if (int rc = wgrad({hl(0), kW, kW, kept.enc, kEnc, kEnc, 0, kW, in_ch, gl.w_pts[0], in_ch, gl.b_pts[0], true})) return rc;
  }
  nerfquery_finish_kernel<<<(unsigned)cdiv64(gl.total, 256), 256, 0, c.stream>>>(gacc, gl.total, gl.cam, gl.b_views, c.w_view, m.views_ch(),
                                                                                 m.cam_ch, grads);
  NRPN_LAUNCH_CHECK("nerfquery_finish_kernel");
  return NRPN_OK;
}

// the call of an entry point: the arguments the five share; split / split_t: the planes, or null
QueryCall query_call(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x, float center_y,
                     float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                     const float *w_view, const float *b_view, const float *embedded_cam, int64_t chunk, void *work, int64_t work_bytes,
                     nrpn_stream_t stream, const void *split, const void *split_t) {
  return QueryCall{Points{pts, num_rays * num_samples, num_samples, center_x, center_y, center_z, bb_scale},
                   Model{multires, multires_views, input_ch_cam}, viewdirs, packed, w_view, b_view, embedded_cam, num_rays, chunk, work,
                   work_bytes, as_stream(stream), static_cast<const uint4 *>(split), static_cast<const uint4 *>(split_t)};
}

}  // namespace

extern "C" {

int64_t nrpn_nerfquery_work_bytes(int what, int64_t num_rays, int num_samples, int64_t chunk, int multires, int multires_views,
                                  int input_ch_cam) {
  const Model m{multires, multires_views, input_ch_cam};
  if (what == 2 || what == 5) return kPackedTFloats * 4;       // floats, or a hi and a lo bf16 of each
  if (what == 4) return 4 * (int64_t)(kEnc + kLayers * kW + kW + 3 * kHalf + kHeadCols + (m.ok() ? m.kv() : 0));
  if (!m.ok() || !query_sizes_ok(num_rays, num_samples, chunk)) return -1;
  if (what == 3) return grad_layout(m).total;
  const int64_t n = num_rays * num_samples;
  const Layout l = layout(m, num_rays, cdiv64(chunk < n ? chunk : n, kTile));
  return what == 0 ? l.fwd_end : what == 1 ? l.total : -1;
}

int nrpn_nerfquery_pack_t(const float *raw, int input_ch, float *packed_t, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && packed_t, "nerfquery_pack_t: null pointer");
  NRPN_REQUIRE(input_ch >= 3 && input_ch <= kEnc, "nerfquery_pack_t: input_ch %d outside 3 .. %d", input_ch, kEnc);
  return launch_pack(raw, pack_t_plan(input_ch), kPackTSegs, packed_t, nullptr, 0, as_stream(stream));
}

int nrpn_nerfquery_pack_t_bf16x3(const float *raw, int input_ch, void *planes_t, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && planes_t, "nerfquery_pack_t_bf16x3: null pointer");
  NRPN_REQUIRE(input_ch >= 3 && input_ch <= kEnc, "nerfquery_pack_t_bf16x3: input_ch %d outside 3 .. %d", input_ch, kEnc);
  return launch_pack(raw, pack_t_plan(input_ch), kPackTSegs, nullptr, static_cast<unsigned short *>(planes_t), kPackedTFloats,
                     as_stream(stream));
}

int nrpn_nerfquery_forward(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x, float center_y,
                           float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                           const float *w_view, const float *b_view, const float *embedded_cam, int64_t chunk, void *work,
                           int64_t work_bytes, float *raw, nrpn_stream_t stream) {
  return forward(query_call(pts, viewdirs, num_rays, num_samples, center_x, center_y, center_z, bb_scale, multires, multires_views,
                            input_ch_cam, packed, w_view, b_view, embedded_cam, chunk, work, work_bytes, stream, nullptr, nullptr),
                 raw);
}

int nrpn_nerfquery_forward_bf16x3(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x,
                                  float center_y, float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam,
                                  const float *packed, const void *split, const float *w_view, const float *b_view,
                                  const float *embedded_cam, int64_t chunk, void *work, int64_t work_bytes, float *raw,
                                  nrpn_stream_t stream) {
  NRPN_REQUIRE(split, "nerfquery_forward: null output or planes");
  return forward(query_call(pts, viewdirs, num_rays, num_samples, center_x, center_y, center_z, bb_scale, multires, multires_views,
                            input_ch_cam, packed, w_view, b_view, embedded_cam, chunk, work, work_bytes, stream, split, nullptr),
                 raw);
}

int nrpn_nerfquery_backward(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x, float center_y,
                            float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam, const float *packed,
                            const float *packed_t, const float *w_view, const float *b_view, const float *embedded_cam,
                            const float *draw, int64_t chunk, void *work, int64_t work_bytes, float *grads, nrpn_stream_t stream) {
  return backward(query_call(pts, viewdirs, num_rays, num_samples, center_x, center_y, center_z, bb_scale, multires, multires_views,
                             input_ch_cam, packed, w_view, b_view, embedded_cam, chunk, work, work_bytes, stream, nullptr, nullptr),
                  packed_t, draw, grads);
}

int nrpn_nerfquery_backward_bf16x3(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x,
                                   float center_y, float center_z, float bb_scale, int multires, int multires_views, int input_ch_cam,
                                   const float *packed, const void *split, const float *packed_t, const float *w_view,
                                   const float *b_view, const float *embedded_cam, const float *draw, int64_t chunk, void *work,
                                   int64_t work_bytes, float *grads, nrpn_stream_t stream) {
  NRPN_REQUIRE(split, "nerfquery_backward: null pointer");
  return backward(query_call(pts, viewdirs, num_rays, num_samples, center_x, center_y, center_z, bb_scale, multires, multires_views,
                             input_ch_cam, packed, w_view, b_view, embedded_cam, chunk, work, work_bytes, stream, split, nullptr),
                  packed_t, draw, grads);
}

int nrpn_nerfquery_backward_bf16x3_split(const float *pts, const float *viewdirs, int64_t num_rays, int num_samples, float center_x,
                                         float center_y, float center_z, float bb_scale, int multires, int multires_views,
                                         int input_ch_cam, const float *packed, const void *split, const void *split_t,
                                         const float *w_view, const float *b_view, const float *embedded_cam, const float *draw,
                                         int64_t chunk, void *work, int64_t work_bytes, float *grads, nrpn_stream_t stream) {
  NRPN_REQUIRE(split && split_t, "nerfquery_backward: null pointer");
  return backward(query_call(pts, viewdirs, num_rays, num_samples, center_x, center_y, center_z, bb_scale, multires, multires_views,
                             input_ch_cam, packed, w_view, b_view, embedded_cam, chunk, work, work_bytes, stream, split, split_t),
                  nullptr, draw, grads);
}

}  // extern "C"
