// The channels-last access layer of the HBM-bound companion kernels (elementwise.hip, swin.hip, fcos.hip, roialign.hip, roipool.hip).
// Tensors are [rows = N*X*Y*Z][C]; a lane owns V consecutive channels of one row.  This header is the one place that says
//   * how V channels are loaded and stored (vecv), and how a bf16 store rounds,
//   * which V a tensor gets (cl_width) and how (dtype, V) picks a kernel instantiation (cl_dispatch),
//   * how a flat lane index becomes (scene, x, y, z, channel group) (voxel_index).
#pragma once
#include "common.h"

typedef unsigned short bf16s;
typedef __attribute__((ext_vector_type(4))) float f4;
typedef __attribute__((ext_vector_type(4))) unsigned short us4;

// V consecutive channels <-> float[V].  V = 4 is an 8-byte (bf16) or 16-byte (fp32) access; V = 8 exists for bf16 only (16 bytes: half the
// instructions per byte on the issue-bound kernels, e.g. the 27 window positions per output of the 3/2/1 pool).  The pointer must be
// aligned to the access.  bf16 stores round to nearest even on the conversion unit, two values per v_cvt_pk_bf16_f32: the result of
// common.h's f32_to_bf16_bits for every input (NaNs come out quiet).
template <typename T, int V> struct vecv;
template <> struct vecv<float, 4> {
  static __device__ __forceinline__ void ld(const float *p, float *o) { const f4 v = *reinterpret_cast<const f4 *>(p); o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
  static __device__ __forceinline__ void st(float *p, const float *o) { *reinterpret_cast<f4 *>(p) = f4{o[0], o[1], o[2], o[3]}; }
};
template <int V> struct vecv<bf16s, V> {
  static_assert(V == 4 || V == 8, "bf16 lanes hold 4 or 8 channels");
  typedef __attribute__((ext_vector_type(V))) unsigned short usv;
  typedef __attribute__((ext_vector_type(V))) float fv;
  typedef __attribute__((ext_vector_type(V))) __bf16 bv;
  static __device__ __forceinline__ void ld(const bf16s *p, float *o) {
    const usv u = *reinterpret_cast<const usv *>(p);
#pragma unroll
    for (int q = 0; q < V; ++q) o[q] = bf16_bits_to_f32(u[q]);
  }
  static __device__ __forceinline__ void st(bf16s *p, const float *o) {
    fv v;
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = o[q];
    *reinterpret_cast<usv *>(p) = __builtin_bit_cast(usv, __builtin_convertvector(v, bv));
  }
};

// V per-channel fp32 parameters as 16-byte loads (p is 16-byte aligned: the channel group starts at a multiple of V >= 4 floats)
template <int V>
__device__ __forceinline__ void ld_params(const float *__restrict__ p, float *o) {
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f4 v = *reinterpret_cast<const f4 *>(p + q);
    o[q] = v[0]; o[q + 1] = v[1]; o[q + 2] = v[2]; o[q + 3] = v[3];
  }
}

#define DISPATCH_T(dtype, ...)                                 \
  if ((dtype) == NRPN_F32) { typedef float T; __VA_ARGS__; }   \
  else { typedef bf16s T; __VA_ARGS__; }

// grid of a grid-stride kernel with 256-lane blocks: one lane per work item up to `cap` blocks
static inline int ew_blocks(long long work, int cap = 8192) { long long b = (work + 255) / 256; return (int)(b > cap ? cap : (b < 1 ? 1 : b)); }

// The width rule: 8 channels per lane for bf16 with C % 8 == 0, else 4 (C % 4 == 0 is every caller's precondition).  With pointers: 8 only
// if each of them (null ones aside) allows 16-byte accesses.
static inline int cl_width(int dtype, int c) { return (dtype == NRPN_BF16 && c % 8 == 0) ? 8 : 4; }
template <typename... P>
static inline int cl_width(int dtype, int c, const P *...ptrs) {
  return ((uintptr_t(0) | ... | reinterpret_cast<uintptr_t>(ptrs)) & 15) == 0 ? cl_width(dtype, c) : 4;
}

// (dtype, width) -> f(cl_tag<T, V>): a generic lambda reads T and V off its argument.  There is no fp32 tag of width 8.
template <typename T_, int V_> struct cl_tag {
  static_assert(V_ == 4 || (V_ == 8 && sizeof(T_) == 2), "8 channels per lane is a bf16 form");
  typedef T_ T;
  static constexpr int V = V_;
};
template <typename F>
static inline void cl_dispatch(int dtype, int width, F &&f) {
  if (dtype == NRPN_F32) f(cl_tag<float, 4>{});
  else if (width == 8) f(cl_tag<bf16s, 8>{});
  else f(cl_tag<bf16s, 4>{});
}

// Flat index g over [N][X][Y][Z][C / V] -> voxel (flat, = g / (C / V)), scene b, (x, y, z) and the first channel cg of the lane's group.
// Two forms with one result: multiply-shift divisors built on the host (common.h FastDiv; g < 2^31), and plain % / on index type I
// (unsigned below 2^31 elements, long long beyond) for the general kernels.
struct VoxelDiv { FastDiv ct, z, y, x; };
static inline VoxelDiv make_voxel_div(int ct, int x, int y, int z) {
  return VoxelDiv{make_fastdiv((unsigned)ct), make_fastdiv((unsigned)z), make_fastdiv((unsigned)y), make_fastdiv((unsigned)x)};
}
struct VoxelIdx { long long vox, b; int cg, x, y, z; };
template <int V>
__device__ __forceinline__ VoxelIdx voxel_index(unsigned g, const VoxelDiv &dv) {
  const unsigned vox = fastdiv(g, dv.ct);
  const int cg = (int)(g - vox * dv.ct.d) * V;
  const unsigned t1 = fastdiv(vox, dv.z), t2 = fastdiv(t1, dv.y), b = fastdiv(t2, dv.x);
  const int z = (int)(vox - t1 * dv.z.d), y = (int)(t1 - t2 * dv.y.d), x = (int)(t2 - b * dv.x.d);
  return VoxelIdx{(long long)vox, (long long)b, cg, x, y, z};
}
template <int V, typename I>
__device__ __forceinline__ VoxelIdx voxel_index(I g, I ct, int nx, int ny, int nz) {
  const I vox = g / ct;
  I v = vox;
  const int z = (int)(v % (I)nz); v /= (I)nz;
  const int y = (int)(v % (I)ny); v /= (I)ny;
  const int x = (int)(v % (I)nx);
  return VoxelIdx{(long long)vox, (long long)(v / (I)nx), (int)(g - vox * ct) * V, x, y, z};
}
