// rgb-sigma grid of a trained NeRF MLP (scripts/nerf_extract.py; reference data/scannet/run_nerf.py:1157-1194 with run_network :50-65).
//
// The reference sends every grid point through the whole 8 x 256 MLP once per training pose.  Only views_linears.0 and rgb_linear see
// the pose, so here the trunk runs once per point and the poses loop over a 128-wide head:
//   trunk (one workgroup = 64 points): positional encoding into LDS, the eight pts_linears, feature_linear, alpha_linear and the
//     feature columns W_f of views_linears.0 -- all matrix products on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain), the
//     activations in one [64][324] fp32 LDS image rewritten in place between two barriers per layer, the weights read from L2 in a
//     packed order (nerfgrid_pack_kernel) that makes every B fragment one coalesced 16-byte load per lane.
//     -> sigma (written to the result) and g = W_f f, 128 floats per point, in a scratch that is bounded by the chunk size.
//   head (one thread = one point): for the poses in order v = relu(g + c_p), rgb = W_rgb v + b_rgb, acc += sigmoid(rgb); acc / P.
// No atomics; a point's arithmetic does not depend on its neighbours, its tile or its chunk.
#include "common.h"

#include <cmath>

namespace {

constexpr int kTile = 64;        // points per workgroup
constexpr int kEnc = 64;         // columns 0 .. 63 of the LDS image: the encoding (input_ch <= 64, zero-padded)
constexpr int kW = 256;          // hidden width
constexpr int kHalf = 128;       // views_linears.0 width
constexpr int kLd = 324;         // row stride of the LDS image in floats: 16-byte aligned rows, 4-bank skew between rows
constexpr int kLayers = 8;
constexpr int kSkipLayer = 5;    // the layer after skip 4 reads cat([e, h])
constexpr int kLdsBytes = kTile * kLd * 4;

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

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// A matrix W [n_out][ld] (torch Linear layout) becomes B fragments: the k axis is [ka columns of W, zero-padded to ka_pad][kb columns
// of W starting at column ka]; k-group kg = 8 consecutive k; lane half h takes k = 8 kg + 4 h + j in element j, so the float4 of
// (kg, output column o, h) sits at ((kg * n_out + o) * 2 + h) * 4.
struct PackSeg {
  int64_t dst, src;
  int n_out, ld, ka, ka_pad, kb;     // n_out == 0: plain copy of kb floats
};
struct PackPlan {
  PackSeg seg[16];
};

__global__ void nerfgrid_pack_kernel(const float *__restrict__ raw, float *__restrict__ packed, PackPlan plan) {
  const PackSeg s = plan.seg[blockIdx.y];
  const int64_t total = s.n_out == 0 ? s.kb : (int64_t)(s.ka_pad + s.kb) * s.n_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (s.n_out == 0) {
      packed[s.dst + i] = raw[s.src + i];
      continue;
    }
    const int j = (int)(i & 3), h = (int)((i >> 2) & 1);
    const int64_t q = i >> 3;
    const int o = (int)(q % s.n_out), kg = (int)(q / s.n_out);
    const int k = 8 * kg + 4 * h + j;
    float v = 0.f;
    if (k < s.ka_pad) {
      if (k < s.ka) v = raw[s.src + (int64_t)o * s.ld + k];
    } else {
      v = raw[s.src + (int64_t)o * s.ld + s.ka + (k - s.ka_pad)];
    }
    packed[s.dst + i] = v;
  }
}

// ---- trunk -----------------------------------------------------------------------------------------------------------------------
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

// row of the 32 x 32 accumulator that register reg of this lane holds
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

struct GridArgs {
  const float *xs, *ys, *zs;      // linspace values [rx], [ry], [rz]
  int rx, ry, rz;
  float cx, cy, cz, scale;
  int multires, input_ch;
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

__global__ __launch_bounds__(256) void nerfgrid_trunk_kernel(GridArgs ga, const float *__restrict__ packed, int64_t point0,
                                                             float *__restrict__ gbuf, float *__restrict__ out) {
  extern __shared__ __align__(16) float act[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t tile0 = point0 + (int64_t)blockIdx.x * kTile;

  // encoding: thread = (point i, quarter q of the 3 L (frequency, axis) pairs)
  {
    const int i = t & 63, q = t >> 6;
    int64_t pr = tile0 + i;
    if (pr > ga.num_points - 1) pr = ga.num_points - 1;       // a partial tile repeats the last point; nothing of it is stored
    const int ix = (int)(pr % ga.rx);
    const int64_t tq = pr / ga.rx;
    const int iy = (int)(tq % ga.ry), iz = (int)(tq / ga.ry);
    const float p[3] = {(ga.xs[ix] - ga.cx) * ga.scale, (ga.ys[iy] - ga.cy) * ga.scale, (ga.zs[iz] - ga.cz) * ga.scale};
    float *row = act + i * kLd;
    if (q == 0) {
      row[0] = p[0];
      row[1] = p[1];
      row[2] = p[2];
      for (int c = ga.input_ch; c < kEnc; ++c) row[c] = 0.f;
    }
    for (int idx = q; idx < 3 * ga.multires; idx += 4) {
      const int l = idx / 3, a = idx - 3 * l;
      const float arg = p[a] * ldexpf(1.0f, l);
      row[3 + 6 * l + a] = sinf(arg);
      row[3 + 6 * l + 3 + a] = cosf(arg);
    }
  }
  __syncthreads();

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
      const int64_t pr = tile0 + t;
      if (pr < ga.num_points) out[out_index(ga, pr) + 3] = s;
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
  }

  // g = W_f f: 128 columns, 32 per wave; stored [tile][column][point] so the head reads it coalesced
  {
    f32x16 acc[2][1];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][0][e] = 0.f;
    gemm_tile<1>(act, kEnc, kW, wp + off_layer(9) / 4, kHalf, wave * 32, acc);
    float *gt = gbuf + (int64_t)blockIdx.x * (kTile * kHalf) + (wave * 32 + r) * kTile;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 v = {acc[m][0][4 * q], acc[m][0][4 * q + 1], acc[m][0][4 * q + 2], acc[m][0][4 * q + 3]};
        *reinterpret_cast<float4 *>(gt + 32 * m + 8 * q + 4 * h) = v;
      }
  }
}

// ---- head ------------------------------------------------------------------------------------------------------------------------
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
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) {
      const float v = fmaxf(g[j] + c[j], 0.f);
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

}  // namespace

extern "C" {

int64_t nrpn_nerfgrid_work_bytes(int what, int64_t num_points) {
  if (what == 0) return kPackedFloats * 4;
  if (what == 1 && num_points > 0) return cdiv64(num_points, kTile) * kTile * kHalf * 4;
  return -1;
}

int nrpn_nerfgrid_pack(const float *raw, int input_ch, float *packed, nrpn_stream_t stream) {
  NRPN_REQUIRE(raw && packed, "nerfgrid_pack: null pointer");
  NRPN_REQUIRE(input_ch >= 3 && input_ch <= kEnc, "nerfgrid_pack: input_ch %d outside 3 .. %d", input_ch, kEnc);
  PackPlan plan{};
  int n = 0;
  int64_t src = 0;
  for (int i = 0; i <= 9; ++i) {      // the raw order is the packed order: pts_linears 0 .. 7, feature_linear, W_f
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
    s.ld = s.ka + s.kb;
    src += (int64_t)s.n_out * s.ld;
    plan.seg[n++] = s;
  }
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
  nerfgrid_pack_kernel<<<dim3(64, n), 256, 0, as_stream(stream)>>>(raw, packed, plan);
  NRPN_LAUNCH_CHECK("nerfgrid_pack_kernel");
  return NRPN_OK;
}

int nrpn_nerfgrid_query(const float *xs, const float *ys, const float *zs, int res_x, int res_y, int res_z, float center_x,
                        float center_y, float center_z, float bb_scale, int multires, const float *packed, const float *ctab,
                        int num_poses, int layout, int64_t chunk, void *work, int64_t work_bytes, float *out, nrpn_stream_t stream) {
  NRPN_REQUIRE(xs && ys && zs && packed && ctab && work && out, "nerfgrid_query: null pointer");
  NRPN_REQUIRE(res_x >= 1 && res_y >= 1 && res_z >= 1, "nerfgrid_query: resolution %d x %d x %d", res_x, res_y, res_z);
  NRPN_REQUIRE(multires >= 0 && 3 + 6 * multires <= kEnc, "nerfgrid_query: multires %d does not fit %d encoding columns", multires, kEnc);
  NRPN_REQUIRE(num_poses >= 1, "nerfgrid_query: no poses");
  NRPN_REQUIRE(layout == 0 || layout == 1, "nerfgrid_query: layout %d", layout);
  const int64_t n = (int64_t)res_x * res_y * res_z;
  NRPN_REQUIRE(n < ((int64_t)1 << 40), "nerfgrid_query: too many points");
  NRPN_REQUIRE(chunk >= 1, "nerfgrid_query: chunk %lld", (long long)chunk);
  const int64_t chunk_tiles = cdiv64(chunk < n ? chunk : n, kTile);
  NRPN_REQUIRE(chunk_tiles <= 0x7fffffff, "nerfgrid_query: chunk too large");
  NRPN_REQUIRE(work_bytes >= chunk_tiles * kTile * kHalf * 4, "nerfgrid_query: work buffer of %lld bytes is too small",
               (long long)work_bytes);
  NRPN_LDS(nerfgrid_trunk_kernel, kLdsBytes);
  GridArgs ga{xs, ys, zs, res_x, res_y, res_z, center_x, center_y, center_z, bb_scale, multires, 3 + 6 * multires, n, layout};
  float *gbuf = static_cast<float *>(work);
  for (int64_t p0 = 0; p0 < n; p0 += chunk_tiles * kTile) {
    const int64_t left = n - p0;
    const int tiles = (int)(left < chunk_tiles * kTile ? cdiv64(left, kTile) : chunk_tiles);
    nerfgrid_trunk_kernel<<<tiles, 256, kLdsBytes, as_stream(stream)>>>(ga, packed, p0, gbuf, out);
    NRPN_LAUNCH_CHECK("nerfgrid_trunk_kernel");
    nerfgrid_head_kernel<<<tiles, kTile, 0, as_stream(stream)>>>(ga, packed, p0, gbuf, ctab, num_poses, out);
    NRPN_LAUNCH_CHECK("nerfgrid_head_kernel");
  }
  return NRPN_OK;
}

}  // extern "C"
