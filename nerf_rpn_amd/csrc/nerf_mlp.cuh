// The 8 x 256 trunk of the NeRF MLP of DESIGN.md 3.16 on the exact-fp32 MFMA, shared by nerfgrid.hip (lattice points),
// nerfrender.hip (ray samples) and nerfquery.hip (given points): packed-weight layout (nrpn_nerfgrid_pack), fragment loads, the
// k-ordered MFMA product, the body of one workgroup, and the one kernel and the one launcher that run it.  The arithmetic of a point
// does not depend on the caller, its tile or its neighbours.  trunk_body<true> is the same body with the matrix products in the bf16x3
// arithmetic; the default, trunk_body<false>, is the exact-fp32 code unchanged.
//
// A consumer says where a tile's 64 points come from and where their sigma goes with a Tile: a small struct of values, passed to
// trunk_kernel<kSplit, Tile> by value, with
//   int multires;                    the L of the positional encoding (input_ch = 3 + 6 L)
//   src(block)  -> a source:         point(i, p) gives the normalised position of point i of workgroup ``block``'s tile
//   sink(block) -> a sink:           sigma(i, s) takes alpha_linear's output of that point; optionally keep() (see sink_keeps)
// Both may refer to the Tile they came from, which outlives them.  g = W_f f of the tile goes to gbuf[block] as [column][point].
// launch_trunk(tile, tiles, packed, split, gbuf, stream[, flags]) is the only place that knows there are two arithmetics to launch: the
// planes ``split`` select bf16x3, null selects fp32; per-tile ``flags`` select the sibling kernel that leaves unflagged tiles alone.  The point arithmetic of a source stays in its consumer's translation unit: the
// three are compiled with different contraction flags (Makefile).
//
// Also here, each defined once for the three consumers: the pack of a weight matrix into B fragments (PackSeg, pack_elem, launch_pack:
// the forward's matrices and nerfquery.hip's transposes, fp32 and bf16x3), and what runs after the trunk -- the view branch of
// views_linears.0 (unit_dir, embed_dirs, view_row) and rgb_linear over relu(g + c) (head_pre, rgb_head, rgb_store).  nerf_render and
// nerf_query give the same raw on the same points and view directions because they run these, not copies of them.
#pragma once
#include "common.h"

#include <cmath>
#include <cstddef>
#include <type_traits>

namespace nerfmlp {

constexpr int kTile = 64;        // points per workgroup
constexpr int kEnc = 64;         // columns 0 .. 63 of the LDS image: the encoding (input_ch <= 64, zero-padded)
constexpr int kW = 256;          // hidden width
constexpr int kHalf = 128;       // views_linears.0 width
constexpr int kLd = 324;         // row stride of the LDS image in floats: 16-byte aligned rows, 4-bank skew between rows
constexpr int kLayers = 8;
constexpr int kSkipLayer = 5;    // the layer after skip 4 reads cat([e, h])
constexpr int kLdsBytes = kTile * kLd * 4;
constexpr int kMaxViewsCh = 64;  // 3 + 6 multires_views <= 64 (multires_views <= 10)

// the ranges of (multires, multires_views, input_ch_cam) every entry point accepts
inline bool model_ok(int multires, int multires_views, int cam_ch) {
  return multires >= 0 && 3 + 6 * multires <= kEnc && multires_views >= 0 && 3 + 6 * multires_views <= kMaxViewsCh && cam_ch >= 0 &&
         cam_ch <= 65536;
}

// ... and the sizes nerfquery.hip accepts: num_rays rays of ``samples`` given points each, in chunks of ``chunk`` points (the renders'
// limits, which count rays per chunk and two passes, are nerfray::sizes_ok)
inline bool query_sizes_ok(int64_t num_rays, int samples, int64_t chunk) {
  return num_rays >= 1 && samples >= 1 && samples <= 65536 && num_rays < ((int64_t)1 << 31) && chunk >= 1 &&
         num_rays * samples < ((int64_t)1 << 40);
}

inline int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }

// One (frequency l, axis a) pair of the reference's embedding [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ..] of a 3-vector, x = its
// component a: row is the embedding's first column
__device__ __forceinline__ void embed_freq(float *row, float x, int l, int a) {
  const float arg = x * ldexpf(1.0f, l);
  row[3 + 6 * l + a] = sinf(arg);
  row[3 + 6 * l + 3 + a] = cosf(arg);
}

// packed layout, in floats (include/nerfrpn.h: nrpn_nerfgrid_pack)
constexpr int64_t kOffL0 = 0;
constexpr int64_t kSzL0 = (int64_t)kEnc * kW;
constexpr int64_t kSzSq = (int64_t)kW * kW;
constexpr int64_t kSzSkip = (int64_t)(kEnc + kW) * kW;
__host__ __device__ constexpr int64_t off_layer(int i) {          // i = 0 .. 7 pts_linears, 8 feature_linear, 9 W_f
  return i == 0 ? kOffL0 : kSzL0 + (int64_t)(i - 1) * kSzSq + (i > kSkipLayer ? kSzSkip - kSzSq : 0);
}
constexpr int64_t kOffBias = off_layer(9) + (int64_t)kW * kHalf;   // 9 x 256: pts_linears 0 .. 7, feature_linear
constexpr int64_t kOffAlphaW = kOffBias + 9 * kW;                  // 256
constexpr int64_t kOffAlphaB = kOffAlphaW + kW;                    // 1 (+3 pad)
constexpr int64_t kOffRgbW = kOffAlphaB + 4;                       // 3 x 128
constexpr int64_t kOffRgbB = kOffRgbW + 3 * kHalf;                 // 3 (+1 pad)
constexpr int64_t kPackedFloats = kOffRgbB + 4;

// split planes of the bf16x3 arithmetic, in bf16 elements (include/nerfrpn.h: nrpn_nerfgrid_pack_bf16x3): the hi plane holds the ten
// matrices at the offsets off_layer gives, the lo plane follows it.  Every offset is a multiple of 8: a fragment is one uint4.
constexpr int64_t kSplitPlane = kOffBias;
constexpr int64_t kSplitElems = 2 * kSplitPlane;

// ---- pack: a matrix of raw as the B fragments gemm_tile and gemm_tile_split load ---------------------------------------------------
// One segment of a pack.  W is read at raw[src + (col_off + o) * ld_o + k * ld_k] for output column o and k: ld_o is W's row stride and
// ld_k = 1 for a torch Linear weight [n_out][ld] as the forward multiplies it, and the other way round for its transpose, whose output
// columns are W's columns from col_off.  The packed k axis is [ka k of W, zero-padded to ka_pad][kb k of W from ka on]; a transpose
// has ka = ka_pad = 0.  fp32 (kFrag 4): k-group kg = 8 consecutive k, lane half h takes k = 8 kg + 4 h + j in element j, so the float4
// of (kg, o, h) sits at ((kg * n_out + o) * 2 + h) * 4 of dst.  bf16x3 (kFrag 8): k-step ks = 16 consecutive k, k = 16 ks + 8 h + j, the
// eight bf16 of (ks, o, h) at ((ks * n_out + o) * 2 + h) * 8 of dst in the hi plane, their residuals at the same place of the lo plane;
// padding is zero in both.  n_out == 0: a plain copy of kb floats (fp32 only).
struct PackSeg {
  int64_t dst, src;
  int n_out, ld_o, ld_k, col_off, ka, ka_pad, kb;
};
struct PackPlan {
  PackSeg seg[16];
};

// the value of element i of a segment's fragments, kFrag elements to a fragment
template <int kFrag>
__device__ __forceinline__ float pack_elem(const float *__restrict__ raw, const PackSeg &s, int64_t i) {
  constexpr int kShift = kFrag == 4 ? 2 : 3;
  static_assert(kFrag == 1 << kShift, "fragments of 4 or 8 elements");
  const int j = (int)(i & (kFrag - 1)), h = (int)((i >> kShift) & 1);
  const int64_t q = i >> (kShift + 1);
  const int o = (int)(q % s.n_out), kg = (int)(q / s.n_out);
  int k = 2 * kFrag * kg + kFrag * h + j;
  if (k < s.ka_pad) {
    if (k >= s.ka) return 0.f;
  } else {
    k += s.ka - s.ka_pad;
  }
  return raw[s.src + (int64_t)(s.col_off + o) * s.ld_o + (int64_t)k * s.ld_k];
}

// The ``segs`` segments of plan from raw: into the floats ``packed``, or, packed null, into the bf16x3 planes ``planes`` whose lo plane
// starts lo_plane elements after the hi plane (nerfgrid.hip has the two kernels).  Raises nothing but a failed launch.
int launch_pack(const float *raw, const PackPlan &plan, int segs, float *packed, unsigned short *planes, int64_t lo_plane,
                hipStream_t stream);

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// acc[m][c] += act[32 m .. 32 m + 31][k0 .. k0 + K) * W[:, col0 + 32 c .. + 31]; one wave, NC column blocks.  K / 8 is even.  Two
// register sets alternate, so the loads of k-group n + 1 are in flight during the 8 * NC MFMAs of group n without register copies.
template <int NC>
struct Frag {
  float4 a[2], b[NC];
};

template <int NC>
__device__ __forceinline__ void frag_load(Frag<NC> &f, const float *a_ptr, const float4 *__restrict__ b_ptr, int kg, int n_out) {
  f.a[0] = *reinterpret_cast<const float4 *>(a_ptr + kg * 8);
  f.a[1] = *reinterpret_cast<const float4 *>(a_ptr + 32 * kLd + kg * 8);
#pragma unroll
  for (int c = 0; c < NC; ++c) f.b[c] = b_ptr[(int64_t)kg * n_out * 2 + c * 64];
}

template <int NC>
__device__ __forceinline__ void frag_mma(const Frag<NC> &f, f32x16 (&acc)[2][NC]) {
  const float av[2][4] = {{f.a[0].x, f.a[0].y, f.a[0].z, f.a[0].w}, {f.a[1].x, f.a[1].y, f.a[1].z, f.a[1].w}};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float bv = j == 0 ? f.b[c].x : j == 1 ? f.b[c].y : j == 2 ? f.b[c].z : f.b[c].w;
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][j], bv, acc[m][c], 0, 0, 0);
    }
  }
}

template <int NC>
__device__ __forceinline__ void gemm_tile(const float *act, int k0, int K, const float4 *__restrict__ wp, int n_out, int col0,
                                          f32x16 (&acc)[2][NC]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const float *a_ptr = act + r * kLd + k0 + 4 * h;
  const float4 *b_ptr = wp + ((int64_t)(col0 + r) * 2 + h);
  const int groups = K >> 3;
  Frag<NC> f0, f1;
  frag_load(f0, a_ptr, b_ptr, 0, n_out);
  // the scheduling barriers keep each load block ahead of the MFMA block it overlaps (left alone, the scheduler sinks the loads to
  // their first use and the L2 latency of every group is exposed)
  for (int kg = 0; kg < groups; kg += 2) {
    frag_load(f1, a_ptr, b_ptr, kg + 1, n_out);
    __builtin_amdgcn_sched_barrier(0);
    frag_mma(f0, acc);
    __builtin_amdgcn_sched_barrier(0);
    frag_load(f0, a_ptr, b_ptr, kg + 2 < groups ? kg + 2 : kg, n_out);      // the last iteration reloads its own group: in bounds, unused
    __builtin_amdgcn_sched_barrier(0);
    frag_mma(f1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- bf16x3: x = hi + lo + O(2^-16 x) with hi = bf16(x), lo = bf16(x - hi), both rounded to nearest even; a product is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 into the same fp32 accumulators.  Lane l holds A[row l & 31][k = 8 (l >> 5) + j]
// and B[k = 8 (l >> 5) + j][col l & 31], j = 0 .. 7; the accumulator layout is the fp32 instruction's.  The LDS image stays fp32: a lane
// reads its eight floats of a row (two 16-byte reads) and splits them in registers; the weights come pre-split, one uint4 per plane.
template <int NC>
struct FragSplit {
  float4 a[2][2];
  uint4 bh[NC], bl[NC];
};

template <int NC>
__device__ __forceinline__ void frag_load_split(FragSplit<NC> &f, const float *a_ptr, const uint4 *__restrict__ bh, const uint4 *__restrict__ bl,
                                                int ks, int n_out) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    f.a[m][0] = *reinterpret_cast<const float4 *>(a_ptr + 32 * m * kLd + ks * 16);
    f.a[m][1] = *reinterpret_cast<const float4 *>(a_ptr + 32 * m * kLd + ks * 16 + 4);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    f.bh[c] = bh[(int64_t)ks * n_out * 2 + c * 64];
    f.bl[c] = bl[(int64_t)ks * n_out * 2 + c * 64];
  }
}

__device__ __forceinline__ void split8(const float4 &x0, const float4 &x1, bf16x8 &hi, bf16x8 &lo) {
  const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 hb = (__bf16)x[j];
    hi[j] = hb;
    lo[j] = (__bf16)(x[j] - (float)hb);      // the difference is exact in fp32
  }
}

template <int NC>
__device__ __forceinline__ void frag_mma_split(const FragSplit<NC> &f, f32x16 (&acc)[2][NC]) {
  bf16x8 ah[2], al[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) split8(f.a[m][0], f.a[m][1], ah[m], al[m]);
  // product outermost: the 2 * NC accumulators are independent, so a product's MFMAs do not wait for one another
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, p == 1 ? f.bl[c] : f.bh[c]);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p == 2 ? al[m] : ah[m], b, acc[m][c], 0, 0, 0);
    }
}

// as gemm_tile, K a multiple of 16; hi / lo: the layer's planes, fragment (k-step ks, column o, half h) at (ks * n_out + o) * 2 + h
template <int NC>
__device__ __forceinline__ void gemm_tile_split(const float *act, int k0, int K, const uint4 *__restrict__ hi, const uint4 *__restrict__ lo,
                                                int n_out, int col0, f32x16 (&acc)[2][NC]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const float *a_ptr = act + r * kLd + k0 + 8 * h;
  const uint4 *bh = hi + ((int64_t)(col0 + r) * 2 + h), *bl = lo + ((int64_t)(col0 + r) * 2 + h);
  const int steps = K >> 4;      // even: K is 64, 256 or 320
  FragSplit<NC> f0, f1;
  frag_load_split(f0, a_ptr, bh, bl, 0, n_out);
  for (int ks = 0; ks < steps; ks += 2) {
    frag_load_split(f1, a_ptr, bh, bl, ks + 1, n_out);
    __builtin_amdgcn_sched_barrier(0);
    frag_mma_split(f0, acc);
    __builtin_amdgcn_sched_barrier(0);
    frag_load_split(f0, a_ptr, bh, bl, ks + 2 < steps ? ks + 2 : ks, n_out);      // the last iteration reloads its own step: in bounds, unused
    __builtin_amdgcn_sched_barrier(0);
    frag_mma_split(f1, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// A sink that declares ``static constexpr bool kKeeps = true`` also gets keep(layer, act) once the image holds a layer's output that
// every wave may read: layer -1 the encoding in columns 0 .. 63, 0 .. 7 the post-relu h_i and 8 the feature f in columns 64 .. 319
// (nerfquery.hip keeps them for the backward pass).  Every thread of the workgroup calls it; it may only read the image.
template <class S, class = void>
struct sink_keeps {
  static constexpr bool value = false;
};
template <class S>
struct sink_keeps<S, decltype(void(S::kKeeps))> {
  static constexpr bool value = S::kKeeps;
};

// row of the 32 x 32 accumulator that register reg of this lane holds
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// One workgroup of 256 threads, one tile of 64 points.  act: the kLdsBytes LDS image.  src.point(i, p) gives the normalised position
// of tile point i (a partial tile repeats a valid point; nothing of it may be stored), sink.sigma(i, s) takes alpha_linear's output of
// tile point i; g = W_f f goes to g_tile as [column][point], 128 x 64 floats, for every point of the tile.  kSplit: the ten matrix
// products run in the bf16x3 arithmetic on the planes ``split``; everything else (encoding, bias, relu, alpha_linear) is the same fp32.
template <bool kSplit = false, class Src, class Sink>
__device__ __forceinline__ void trunk_body(float *act, const float *__restrict__ packed, int multires, int input_ch, const Src &src,
                                           const Sink &sink, float *__restrict__ g_tile, const uint4 *__restrict__ split = nullptr) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;

  // encoding: thread = (point i, quarter q of the 3 L (frequency, axis) pairs)
  {
    const int i = t & 63, q = t >> 6;
    float p[3];
    src.point(i, p);
    float *row = act + i * kLd;
    if (q == 0) {
      row[0] = p[0];
      row[1] = p[1];
      row[2] = p[2];
      for (int c = input_ch; c < kEnc; ++c) row[c] = 0.f;
    }
    for (int idx = q; idx < 3 * multires; idx += 4) {
      const int l = idx / 3, a = idx - 3 * l;
      embed_freq(row, p[a], l, a);
    }
  }
  __syncthreads();
  if constexpr (sink_keeps<Sink>::value) sink.keep(-1, act);

  const float4 *wp = reinterpret_cast<const float4 *>(packed);
  const float *bias = packed + kOffBias;
  const int col0 = wave * 64;

  for (int layer = 0; layer <= kLayers; ++layer) {           // 0 .. 7 pts_linears (relu), 8 feature_linear (no relu)
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][c][e] = 0.f;
    const int k0 = (layer == 0 || layer == kSkipLayer) ? 0 : kEnc;
    const int K = layer == 0 ? kEnc : layer == kSkipLayer ? kEnc + kW : kW;
    if constexpr (kSplit)
      gemm_tile_split<2>(act, k0, K, split + off_layer(layer) / 8, split + (kSplitPlane + off_layer(layer)) / 8, kW, col0, acc);
    else
      gemm_tile<2>(act, k0, K, wp + off_layer(layer) / 4, kW, col0, acc);
    if (layer == kLayers && t < kTile) {
      // sigma = alpha_linear(h): h is still in the image; one thread per point, k in order
      const float4 *hrow = reinterpret_cast<const float4 *>(act + t * kLd + kEnc);
      const float *aw = packed + kOffAlphaW;
      float s = 0.f;
      for (int k = 0; k < kW / 4; ++k) {
        const float4 v = hrow[k];
        s = fmaf(v.x, aw[4 * k], s);
        s = fmaf(v.y, aw[4 * k + 1], s);
        s = fmaf(v.z, aw[4 * k + 2], s);
        s = fmaf(v.w, aw[4 * k + 3], s);
      }
      s += packed[kOffAlphaB];
      sink.sigma(t, s);
    }
    __syncthreads();                                          // every wave has read the layer's input
    const bool relu = layer < kLayers;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = col0 + 32 * c + r;
      const float bv = bias[layer * kW + col];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = acc[m][c][e] + bv;
          if (relu) v = fmaxf(v, 0.f);
          act[(32 * m + acc_row(e, h)) * kLd + kEnc + col] = v;
        }
    }
    __syncthreads();
    if constexpr (sink_keeps<Sink>::value) sink.keep(layer, act);
  }

  // g = W_f f: 128 columns, 32 per wave; stored [column][point] so a head reads it coalesced
  {
    f32x16 acc[2][1];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][0][e] = 0.f;
    if constexpr (kSplit)
      gemm_tile_split<1>(act, kEnc, kW, split + off_layer(9) / 8, split + (kSplitPlane + off_layer(9)) / 8, kHalf, wave * 32, acc);
    else
      gemm_tile<1>(act, kEnc, kW, wp + off_layer(9) / 4, kHalf, wave * 32, acc);
    float *gt = g_tile + (wave * 32 + r) * kTile;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 v = {acc[m][0][4 * q], acc[m][0][4 * q + 1], acc[m][0][4 * q + 2], acc[m][0][4 * q + 3]};
        *reinterpret_cast<float4 *>(gt + 32 * m + 8 * q + 4 * h) = v;
      }
  }
}

// the sink of a forward: sigma to raw [point][4]
struct RawSink {
  int64_t tile0, num_points;
  float *raw;
  __device__ __forceinline__ void sigma(int i, float s) const {
    const int64_t pi = tile0 + i;
    if (pi < num_points) raw[pi * 4 + 3] = s;
  }
};

// One workgroup per tile of the launch; gbuf [tiles][128][64]
template <bool kSplit, class Tile>
__global__ __launch_bounds__(256) void trunk_kernel(Tile tile, const float *__restrict__ packed, const uint4 *__restrict__ split,
                                                    float *__restrict__ gbuf) {
  extern __shared__ __align__(16) float act[];
  trunk_body<kSplit>(act, packed, tile.multires, 3 + 6 * tile.multires, tile.src(blockIdx.x), tile.sink(blockIdx.x),
                     gbuf + (int64_t)blockIdx.x * (kTile * kHalf), split);
}

// The same kernel for a launch whose tiles carry a flag each (nerfrender.hip: a render restricted to boxes): a workgroup whose tile's
// flag is 0 returns before the body, so gbuf and the sink get nothing of that tile.  The branch is uniform over the workgroup and comes
// before any barrier.
template <bool kSplit, class Tile>
__global__ __launch_bounds__(256) void trunk_flagged_kernel(Tile tile, const float *__restrict__ packed, const uint4 *__restrict__ split,
                                                            float *__restrict__ gbuf, const uint32_t *__restrict__ flags) {
  extern __shared__ __align__(16) float act[];
  if (flags[blockIdx.x] == 0) return;
  trunk_body<kSplit>(act, packed, tile.multires, 3 + 6 * tile.multires, tile.src(blockIdx.x), tile.sink(blockIdx.x),
                     gbuf + (int64_t)blockIdx.x * (kTile * kHalf), split);
}

// split: the bf16x3 planes of packed, and the trunk runs in that arithmetic; null: in fp32.  flags: one uint32 per tile, and only the
// tiles whose flag is not 0 run (trunk_flagged_kernel); null, or no argument at all, launches trunk_kernel over every tile.  A caller
// that never passes flags does not instantiate the flagged kernel.
template <class Tile, class Flags = std::nullptr_t>
int launch_trunk(const Tile &tile, int tiles, const float *packed, const uint4 *split, float *gbuf, hipStream_t stream,
                 Flags flags = nullptr) {
  if constexpr (!std::is_same_v<Flags, std::nullptr_t>) {
    if (flags) {
      if (split) {
        NRPN_LDS((trunk_flagged_kernel<true, Tile>), kLdsBytes);
        trunk_flagged_kernel<true, Tile><<<tiles, 256, kLdsBytes, stream>>>(tile, packed, split, gbuf, flags);
      } else {
        NRPN_LDS((trunk_flagged_kernel<false, Tile>), kLdsBytes);
        trunk_flagged_kernel<false, Tile><<<tiles, 256, kLdsBytes, stream>>>(tile, packed, nullptr, gbuf, flags);
      }
      NRPN_LAUNCH_CHECK("nerfmlp_trunk_flagged_kernel");
      return NRPN_OK;
    }
  }
  if (split) {
    NRPN_LDS((trunk_kernel<true, Tile>), kLdsBytes);
    trunk_kernel<true, Tile><<<tiles, 256, kLdsBytes, stream>>>(tile, packed, split, gbuf);
  } else {
    NRPN_LDS((trunk_kernel<false, Tile>), kLdsBytes);
    trunk_kernel<false, Tile><<<tiles, 256, kLdsBytes, stream>>>(tile, packed, nullptr, gbuf);
  }
  NRPN_LAUNCH_CHECK("nerfmlp_trunk_kernel");
  return NRPN_OK;
}

// ---- after the trunk: the view branch of views_linears.0 and rgb_linear -----------------------------------------------------------
// Shared by translation units that are compiled with and without FMA contraction (Makefile): every multiply-add below is an explicit
// fmaf, every operation that rounds on its own an explicit __f*_rn, and no other expression holds a multiply next to an add.

// The view direction of a ray direction d: vd = d / n with n = sqrtf((d0 d0 + d1 d1) + d2 d2), every operation rounded on its own.
// nerf_render's head forms it so; a caller of nerf_query that wants the render's rgb bits forms its viewdirs the same way.
__device__ __forceinline__ void unit_dir(const float *d, float (&vd)[3]) {
  const float n = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
  for (int a = 0; a < 3; ++a) vd[a] = __fdiv_rn(d[a], n);
}

// embeddirs_fn of a view direction: row[0 .. 3 + 6 multires_views)
__device__ __forceinline__ void embed_dirs(float *row, const float (&vd)[3], int multires_views) {
#pragma unroll
  for (int a = 0; a < 3; ++a) row[a] = vd[a];
  for (int l = 0; l < multires_views; ++l)
#pragma unroll
    for (int a = 0; a < 3; ++a) embed_freq(row, vd[a], l, a);
}

// c[j] = b[j] + sum_k W_c[j][k] cam[k] + sum_k W_d[j][k] emb[k]: what a ray adds to column j of views_linears.0 before the relu, one fmaf
// chain: the bias, the camera columns in k order, then the view columns in k order.  w_view [128][views_ch + cam_ch]: W_d, then W_c.
// The chain up to the first view column is the same for every ray: view_row_cam gives it, view_row_dirs continues it.
__device__ __forceinline__ float view_row_cam(int j, const float *__restrict__ w_view, const float *__restrict__ b_view,
                                              const float *__restrict__ cam, int views_ch, int cam_ch) {
  float c = b_view[j];
  for (int k = 0; k < cam_ch; ++k) c = fmaf(w_view[j * (views_ch + cam_ch) + views_ch + k], cam[k], c);
  return c;
}
__device__ __forceinline__ float view_row_dirs(float c, int j, const float *__restrict__ w_view, const float *emb, int views_ch,
                                               int cam_ch) {
  for (int k = 0; k < views_ch; ++k) c = fmaf(w_view[j * (views_ch + cam_ch) + k], emb[k], c);
  return c;
}
__device__ __forceinline__ float view_row(int j, const float *__restrict__ w_view, const float *__restrict__ b_view,
                                          const float *__restrict__ cam, const float *emb, int views_ch, int cam_ch) {
  return view_row_dirs(view_row_cam(j, w_view, b_view, cam, views_ch, cam_ch), j, w_view, emb, views_ch, cam_ch);
}

// Column j of views_linears.0 before the relu, the relu, and its derivative: 0 at exactly 0, as torch has it.  The mask the camera
// optimisation stores and the mask nerfquery's backward applies are head_on of head_pre.
__device__ __forceinline__ float head_pre(float g, float c) { return g + c; }
__device__ __forceinline__ float head_relu(float pre) { return fmaxf(pre, 0.f); }
__device__ __forceinline__ bool head_on(float pre) { return pre > 0.f; }

// rgb_linear without its bias over v = relu(g + c) of one point: r[ch] = sum_j W_rgb[ch][j] v[j] as 128-term fmaf chains in j order.
// g(j): the point's trunk output j, from registers or from gbuf; c[j]: the view_row of its ray; w: packed + kOffRgbW, wave-uniform, so
// it comes through the scalar cache.  kMask: bit j of the 128 bits m[0 .. 4), zero on entry, becomes head_on; m is not touched
// otherwise.  kUnroll: the caller's unroll factor of the j loop, kHalf for all of it.  (nerfgrid.hip's per-pose head writes this
// loop out over head_relu(head_pre()): see there.)
template <bool kMask, int kUnroll, class G>
__device__ __forceinline__ void rgb_head(G &&g, const float *c, const float *__restrict__ w, float (&r)[3], uint32_t *m) {
  r[0] = r[1] = r[2] = 0.f;
#pragma unroll kUnroll
  for (int j = 0; j < kHalf; ++j) {
    const float pre = head_pre(g(j), c[j]);
    const float v = head_relu(pre);
    if (kMask) m[j >> 5] |= (uint32_t)head_on(pre) << (j & 31);
    r[0] = fmaf(w[j], v, r[0]);
    r[1] = fmaf(w[kHalf + j], v, r[1]);
    r[2] = fmaf(w[2 * kHalf + j], v, r[2]);
  }
}

// raw rgb of a point: the chains plus rgb_linear's bias
__device__ __forceinline__ void rgb_store(float *o, const float (&r)[3], const float *__restrict__ packed) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = r[ch] + packed[kOffRgbB + ch];
}

}  // namespace nerfmlp
