// ScanNet ground-truth boxes (scripts/scannet_generate_bbox.py): per instance the float32 min / max corner and the minimum-area
// oriented rectangle of its vertices' xy projection, all G instances of a scene batched.
//   * membership: a vertex belongs to every instance that lists its segment (sorted segment ids, binary search, CSR segment ->
//     instances).  count -> scan -> fill, the pattern of plyexport.hip; integer atomics only (counters, list cursors).
//   * extremes: one workgroup per instance, fixed LDS trees: xyz min / max (float32, exact) and the support points of 8 xy directions.
//   * interior discard (Akl-Toussaint): a point strictly left of every edge of the closed chain of those 8 input points lies strictly
//     inside their convex hull and cannot be a hull vertex.  The cross products are float64 of float32 differences; a point is kept
//     unless the product clears a rounding allowance, so points on the octagon's edges stay.  Survivors are compacted as 64-bit keys.
//   * hull: keys sorted by (x, y) with a bitonic network whose compares all point the same way (so any length works without padding),
//     then a monotone chain with cross <= 0 pops: duplicates and collinear points drop out, the hull comes out counter-clockwise from
//     the lexicographically smallest vertex.  In LDS up to kLdsPoints survivors; larger instances sort in global memory, one launch
//     per network step over the list of such instances, and run the chain there.
//   * rectangle search: every hull edge against every hull vertex (bounding_area of the reference's MinimumBoundingBox.py), first
//     minimum in edge order -- the result depends only on the set of vertices.
// Compiled with -ffp-contract=off: the float64 expressions are the reference's, operation for operation.
#include "common.h"

#include <cfloat>
#include <cmath>

namespace {
constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kLdsPoints = 4096;                       // survivors sorted and chained in LDS
constexpr int kLdsBytes = (2 * kLdsPoints + 2) * 8;    // keys + hull stack (one entry more: the chain closes on its first point)
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kHdrMaxSurv = 0, kHdrNumBig = 1, kHdrError = 2, kHdrInts = 4;

struct SegMap {
  const int *ids;      // [S] ascending, unique
  const int *offs;     // [S + 1]
  const int *insts;    // [P]
  int S, P, G;
};

// carved from the caller's work buffer
struct Work {
  int *header;                  // [kHdrInts]
  int *n32;                     // [G] vertices per instance
  int *cursor;                  // [G]
  int *surv;                    // [G] survivors of the discard
  int *hcount;                  // [G] hull vertices
  int *biglist;                 // [G] instances with more than kLdsPoints survivors
  long long *off;               // [G + 1] start of an instance's vertex list / keys; its hull starts at off[g] + g
  int *list;                    // [M] vertex indices
  unsigned long long *keys;     // [M]
  unsigned long long *stack;    // [M + G + 1] chain stack of the large instances
  double2 *hull;                // [M + G + 1]
};

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

size_t carve(Work &w, char *base, long long G, long long M) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + at : nullptr;
    at += up16(bytes);
    return p;
  };
  w.header = (int *)take(kHdrInts * 4);
  w.n32 = (int *)take(G * 4);
  w.cursor = (int *)take(G * 4);
  w.surv = (int *)take(G * 4);
  w.hcount = (int *)take(G * 4);
  w.biglist = (int *)take(G * 4);
  w.off = (long long *)take((G + 1) * 8);
  w.list = (int *)take(M * 4);
  w.keys = (unsigned long long *)take(M * 8);
  w.stack = (unsigned long long *)take((M + G + 1) * 8);
  w.hull = (double2 *)take((M + G + 1) * 16);
  return at;
}

__device__ __forceinline__ int seg_find(const SegMap &m, int s) {
  int lo = 0, hi = m.S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (m.ids[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  return (lo < m.S && m.ids[lo] == s) ? lo : -1;
}

// order-preserving float32 -> uint32, and the (x, y) key
__device__ __forceinline__ unsigned enc32(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec32(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__device__ __forceinline__ unsigned long long make_key(float x, float y) { return ((unsigned long long)enc32(x) << 32) | enc32(y); }
__device__ __forceinline__ double key_x(unsigned long long k) { return (double)dec32((unsigned)(k >> 32)); }
__device__ __forceinline__ double key_y(unsigned long long k) { return (double)dec32((unsigned)k); }

// ---------------------------------------------------------------------------------------------------------------------
// membership
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void count_kernel(const int *__restrict__ seg, long long V, SegMap m,
                                                         unsigned long long *__restrict__ cnt) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  const int k = seg_find(m, seg[v]);
  if (k < 0) return;
  const int b = max(0, m.offs[k]), e = min(m.P, m.offs[k + 1]);
  for (int q = b; q < e; ++q) {
    const int g = m.insts[q];
    if ((unsigned)g < (unsigned)m.G) atomicAdd(&cnt[g], 1ull);
  }
}

__global__ __launch_bounds__(kScanThreads) void total_kernel(const long long *__restrict__ cnt, int G, long long *__restrict__ total) {
  __shared__ long long red[kScanThreads];
  long long s = 0;
  for (int g = threadIdx.x; g < G; g += kScanThreads) s += cnt[g];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = kScanThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = red[0];
}

// exclusive scan of the counts -> off; a total other than M (counts of another input) empties every instance and raises the error flag
__global__ __launch_bounds__(kScanThreads) void offsets_kernel(const long long *__restrict__ cnt, int G, long long M, Work w) {
  __shared__ long long sc[kScanThreads];
  const int per = (G + kScanThreads - 1) / kScanThreads;
  const int g0 = min(G, (int)threadIdx.x * per), g1 = min(G, g0 + per);
  long long c = 0;
  for (int g = g0; g < g1; ++g) c += max(0ll, cnt[g]);
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int s = 1; s < kScanThreads; s <<= 1) {
    const long long v = (int)threadIdx.x >= s ? sc[threadIdx.x - s] : 0;
    __syncthreads();
    sc[threadIdx.x] += v;
    __syncthreads();
  }
  const bool ok = sc[kScanThreads - 1] == M;
  c = threadIdx.x ? sc[threadIdx.x - 1] : 0;
  for (int g = g0; g < g1; ++g) {
    const long long n = max(0ll, cnt[g]);
    w.off[g] = ok ? c : 0;
    w.n32[g] = ok ? (int)n : 0;
    w.cursor[g] = 0;
    w.surv[g] = 0;
    w.hcount[g] = 0;
    c += n;
  }
  if (threadIdx.x == 0) {
    w.off[G] = ok ? M : 0;
    w.header[kHdrMaxSurv] = 0;
    w.header[kHdrNumBig] = 0;
    w.header[kHdrError] = ok ? 0 : 1;
  }
}

__global__ __launch_bounds__(kThreads) void fill_kernel(const int *__restrict__ seg, long long V, SegMap m, Work w) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  const int k = seg_find(m, seg[v]);
  if (k < 0) return;
  const int b = max(0, m.offs[k]), e = min(m.P, m.offs[k + 1]);
  for (int q = b; q < e; ++q) {
    const int g = m.insts[q];
    if ((unsigned)g >= (unsigned)m.G) continue;
    const int pos = atomicAdd(&w.cursor[g], 1);
    if (pos < w.n32[g]) w.list[w.off[g] + pos] = (int)v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// extremes and interior discard: one workgroup per instance
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_minmax(float v, bool want_max, float *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const float a = red[threadIdx.x], b = red[threadIdx.x + s];
      red[threadIdx.x] = want_max ? fmaxf(a, b) : fminf(a, b);
    }
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// the support point of one direction: largest value, smallest key among equals (a function of the set of points)
__device__ __forceinline__ unsigned long long block_support(double v, unsigned long long k, double *rv, unsigned long long *rk) {
  rv[threadIdx.x] = v;
  rk[threadIdx.x] = k;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double bv = rv[threadIdx.x + s];
      const unsigned long long bk = rk[threadIdx.x + s];
      if (bv > rv[threadIdx.x] || (bv == rv[threadIdx.x] && bk < rk[threadIdx.x])) {
        rv[threadIdx.x] = bv;
        rk[threadIdx.x] = bk;
      }
    }
    __syncthreads();
  }
  const unsigned long long r = rk[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void direction_values(double x, double y, double *d) {
  d[0] = x;         // E, then counter-clockwise: NE, N, NW, W, SW, S, SE
  d[1] = x + y;
  d[2] = y;
  d[3] = y - x;
  d[4] = -x;
  d[5] = -x - y;
  d[6] = -y;
  d[7] = x - y;
}

__global__ __launch_bounds__(kThreads) void extremes_kernel(const float *__restrict__ vtx, Work w, float *__restrict__ min_pt,
                                                            float *__restrict__ max_pt, double *__restrict__ obb, int *__restrict__ status) {
  __shared__ float redf[kThreads];
  __shared__ double redv[kThreads];
  __shared__ unsigned long long redk[kThreads];
  __shared__ int nsurv;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = w.n32[g];
  const int *list = w.list + w.off[g];
  if (tid == 0) nsurv = 0;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  double best[8];
  unsigned long long bkey[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) best[d] = -INFINITY, bkey[d] = kNoKey;
  for (int i = tid; i < n; i += kThreads) {
    const float *p = vtx + 3ll * list[i];
    const float x = p[0], y = p[1], z = p[2];
    mn[0] = fminf(mn[0], x), mn[1] = fminf(mn[1], y), mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x), mx[1] = fmaxf(mx[1], y), mx[2] = fmaxf(mx[2], z);
    const unsigned long long key = make_key(x, y);
    double dv[8];
    direction_values((double)x, (double)y, dv);
#pragma unroll
    for (int d = 0; d < 8; ++d)
      if (dv[d] > best[d] || (dv[d] == best[d] && key < bkey[d])) best[d] = dv[d], bkey[d] = key;
  }
  for (int a = 0; a < 3; ++a) {
    mn[a] = block_minmax(mn[a], false, redf);
    mx[a] = block_minmax(mx[a], true, redf);
  }
  if (tid == 0) {
    for (int a = 0; a < 3; ++a) min_pt[g * 3 + a] = mn[a], max_pt[g * 3 + a] = mx[a];
    // z as the reference's float32 arithmetic, then widened; the xy part is filled by the rectangle search (NaN unless status 0)
    const float cz = (mn[2] + mx[2]) / 2.0f, dz = mx[2] - mn[2];
    for (int c = 0; c < 7; ++c) obb[g * 7 + c] = NAN;
    if (n >= 3) obb[g * 7 + 2] = (double)cz, obb[g * 7 + 5] = (double)dz;
    status[g] = n < 3 ? 1 : 0;
  }
  if (n < 3) return;      // uniform over the workgroup
  double ex[8], ey[8];
  unsigned long long ek[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    ek[d] = block_support(best[d], bkey[d], redv, redk);
    ex[d] = key_x(ek[d]);
    ey[d] = key_y(ek[d]);
  }
  unsigned long long *keys = w.keys + w.off[g];
  for (int i = tid; i < n; i += kThreads) {
    const float *p = vtx + 3ll * list[i];
    const float xf = p[0], yf = p[1];
    const double px = (double)xf, py = (double)yf;
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int e = (d + 1) & 7;
      const double t1 = (ex[e] - ex[d]) * (py - ey[d]), t2 = (ey[e] - ey[d]) * (px - ex[d]);
      // a degenerate edge (the same support point twice) bounds nothing
      inside = inside && (ek[d] == ek[e] || (t1 - t2) > 8.0 * DBL_EPSILON * (fabs(t1) + fabs(t2)));
    }
    if (!inside) {
      const int pos = atomicAdd(&nsurv, 1);
      keys[pos] = make_key(xf, yf);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int s = nsurv;
    w.surv[g] = s;
    atomicMax(&w.header[kHdrMaxSurv], s);
    if (s > kLdsPoints) w.biglist[atomicAdd(&w.header[kHdrNumBig], 1)] = g;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// sort + monotone chain
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cross3(unsigned long long a, unsigned long long b, unsigned long long c) {
  const double ax = key_x(a), ay = key_y(a);
  return (key_x(b) - ax) * (key_y(c) - ay) - (key_y(b) - ay) * (key_x(c) - ax);
}

// pair t of a network step: the first step of a merge of width k mirrors (i, k - 1 - i), the others compare at distance j
__device__ __forceinline__ void step_pair(long long t, long long k, long long j, bool mirror, long long &i, long long &l) {
  if (mirror) {
    const long long h = k >> 1, blk = t / h, r = t - blk * h;
    i = blk * k + r;
    l = blk * k + (k - 1 - r);
  } else {
    const long long blk = t / j, r = t - blk * j;
    i = blk * 2 * j + r;
    l = i + j;
  }
}

// one thread: sorted keys p[0 .. n) -> counter-clockwise hull in h, returns its vertex count (0 when degenerate); h holds n + 1 entries
template <typename Load, typename Top, typename Push>
__device__ __forceinline__ int monotone_chain(int n, Load p, Top h, Push push) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned long long c = p(i);
    while (k >= 2 && cross3(h(k - 2), h(k - 1), c) <= 0.0) --k;
    push(k++, c);
  }
  const int t = k + 1;
  for (int i = n - 2; i >= 0; --i) {
    const unsigned long long c = p(i);
    while (k >= t && cross3(h(k - 2), h(k - 1), c) <= 0.0) --k;
    push(k++, c);
  }
  return k - 1 >= 3 ? k - 1 : 0;
}

__global__ __launch_bounds__(kThreads) void hull_lds_kernel(Work w, const int *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lds64[];
  unsigned long long *sk = lds64, *hk = lds64 + kLdsPoints;
  __shared__ int hn;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = w.surv[g];
  if (status[g] != 0 || n > kLdsPoints) return;
  const unsigned long long *keys = w.keys + w.off[g];
  for (int i = tid; i < n; i += kThreads) sk[i] = keys[i];
  __syncthreads();
  int P = 1;
  while (P < n) P <<= 1;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += kThreads) {
        long long i, l;
        step_pair(t, k, j, j == (k >> 1), i, l);
        if (l < n) {
          const unsigned long long a = sk[i], b = sk[l];
          if (b < a) sk[i] = b, sk[l] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0)
    hn = monotone_chain(n, [&](int i) { return sk[i]; }, [&](int i) { return hk[i]; }, [&](int i, unsigned long long v) { hk[i] = v; });
  __syncthreads();
  double2 *out = w.hull + w.off[g] + g;
  for (int i = tid; i < hn; i += kThreads) out[i] = make_double2(key_x(hk[i]), key_y(hk[i]));
  if (tid == 0) w.hcount[g] = hn;
}

// one network step over the instances of biglist
__global__ __launch_bounds__(kThreads) void sort_step_kernel(Work w, long long k, long long j, int mirror) {
  const int g = w.biglist[blockIdx.y];
  const long long n = w.surv[g];
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  long long i, l;
  step_pair(t, k, j, mirror != 0, i, l);
  if (l >= n) return;
  unsigned long long *keys = w.keys + w.off[g];
  const unsigned long long a = keys[i], b = keys[l];
  if (b < a) keys[i] = b, keys[l] = a;
}

// chain of a large instance in global memory (one lane; the others convert the result)
__global__ __launch_bounds__(64) void hull_global_kernel(Work w) {
  __shared__ int hn;
  const int g = w.biglist[blockIdx.x], tid = threadIdx.x;
  const int n = w.surv[g];
  const unsigned long long *keys = w.keys + w.off[g];
  unsigned long long *stack = w.stack + w.off[g] + g;      // n + 1 entries
  double2 *out = w.hull + w.off[g] + g;
  if (tid == 0)
    hn = monotone_chain(n, [&](int i) { return keys[i]; }, [&](int i) { return stack[i]; }, [&](int i, unsigned long long v) { stack[i] = v; });
  __syncthreads();
  for (int i = tid; i < hn; i += 64) out[i] = make_double2(key_x(stack[i]), key_y(stack[i]));
  if (tid == 0) w.hcount[g] = hn;
}

// ---------------------------------------------------------------------------------------------------------------------
// rectangle search: bounding_area for every hull edge, first minimum
// ---------------------------------------------------------------------------------------------------------------------
struct Rect {
  double area, len_p, len_o, min_p, min_o, ux, uy;
};

__global__ __launch_bounds__(kThreads) void rect_kernel(Work w, double *__restrict__ obb, int *__restrict__ status) {
  __shared__ double ra[kThreads];
  __shared__ int ri[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (status[g] != 0) return;
  const int H = w.hcount[g];
  if (H < 3) {
    if (tid == 0) {
      status[g] = 2;
      obb[g * 7 + 2] = NAN;
      obb[g * 7 + 5] = NAN;
    }
    return;
  }
  const double2 *h = w.hull + w.off[g] + g;
  Rect best;
  best.area = INFINITY;
  int best_e = 0x7fffffff;
  for (int e = tid; e < H; e += kThreads) {
    const double2 p0 = h[e], p1 = h[e + 1 == H ? 0 : e + 1];
    const double dis = sqrt((p0.x - p1.x) * (p0.x - p1.x) + (p0.y - p1.y) * (p0.y - p1.y));
    const double ux = (p1.x - p0.x) / dis, uy = (p1.y - p0.y) / dis;
    const double ox = -1.0 * uy, oy = ux;
    double min_p = INFINITY, max_p = -INFINITY, min_o = INFINITY, max_o = -INFINITY;
    for (int q = 0; q < H; ++q) {
      const double2 pt = h[q];
      const double dp = ux * pt.x + uy * pt.y, dq = ox * pt.x + oy * pt.y;
      min_p = fmin(min_p, dp), max_p = fmax(max_p, dp);
      min_o = fmin(min_o, dq), max_o = fmax(max_o, dq);
    }
    const double len_p = max_p - min_p, len_o = max_o - min_o, area = len_p * len_o;
    if (area < best.area) {      // ascending e per lane: the first minimum stays
      best = Rect{area, len_p, len_o, min_p, min_o, ux, uy};
      best_e = e;
    }
  }
  ra[tid] = best.area;
  ri[tid] = best_e;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double b = ra[tid + s];
      const int bi = ri[tid + s];
      if (b < ra[tid] || (b == ra[tid] && bi < ri[tid])) ra[tid] = b, ri[tid] = bi;
    }
    __syncthreads();
  }
  const int win = ri[0];
  if (win != 0x7fffffff && win % kThreads == tid && best_e == win) {
    const double angle = atan2(best.uy, best.ux);
    const double c0 = best.min_p + best.len_p / 2, c1 = best.min_o + best.len_o / 2;
    const double ao = angle + M_PI / 2;
    obb[g * 7 + 0] = c0 * cos(angle) + c1 * cos(ao);
    obb[g * 7 + 1] = c0 * sin(angle) + c1 * sin(ao);
    obb[g * 7 + 3] = best.len_p;
    obb[g * 7 + 4] = best.len_o;
    obb[g * 7 + 6] = angle;
  }
}

int fill_segmap(const char *who, const int32_t *seg_ids, const int32_t *seg_offsets, const int32_t *seg_insts, int S, int P, int G,
                SegMap &m) {
  NRPN_REQUIRE(G >= 1 && G < (1 << 20), "%s: bad instance count %d", who, G);
  NRPN_REQUIRE(S >= 0 && P >= 0, "%s: bad segment table sizes %d, %d", who, S, P);
  NRPN_REQUIRE((S == 0 || (seg_ids && seg_offsets)) && (P == 0 || seg_insts), "%s: null pointer", who);
  m = SegMap{seg_ids, seg_offsets, seg_insts, S, P, G};
  return NRPN_OK;
}
}  // namespace

extern "C" int nrpn_scanbox_lds_points(void) { return kLdsPoints; }

extern "C" int64_t nrpn_scanbox_work_bytes(int64_t num_vertices, int num_instances, int64_t num_members) {
  if (num_vertices < 0 || num_instances < 1 || num_members < 0) return -1;
  Work w;
  return (int64_t)carve(w, nullptr, num_instances, num_members);
}

extern "C" int nrpn_scanbox_count(const int32_t *seg_of_vertex, int64_t num_vertices, const int32_t *seg_ids, const int32_t *seg_offsets,
                                  const int32_t *seg_insts, int num_segs, int num_pairs, int num_instances, int64_t *counts,
                                  int64_t *total, nrpn_stream_t stream) {
  SegMap m;
  if (int rc = fill_segmap("scanbox_count", seg_ids, seg_offsets, seg_insts, num_segs, num_pairs, num_instances, m)) return rc;
  NRPN_REQUIRE(num_vertices >= 0 && num_vertices <= (1ll << 30), "scanbox_count: bad vertex count %lld", (long long)num_vertices);
  NRPN_REQUIRE((num_vertices == 0 || seg_of_vertex) && counts && total, "scanbox_count: null pointer");
  hipStream_t st = as_stream(stream);
  NRPN_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * num_instances, st));
  if (num_vertices && num_segs)
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)cdiv64(num_vertices, kThreads)), dim3(kThreads), 0, st, seg_of_vertex,
                       (long long)num_vertices, m, (unsigned long long *)counts);
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(kScanThreads), 0, st, (const long long *)counts, num_instances, (long long *)total);
  NRPN_LAUNCH_CHECK("scanbox_count");
  return NRPN_OK;
}

extern "C" int nrpn_scanbox_reduce(const float *vertices, const int32_t *seg_of_vertex, int64_t num_vertices, const int32_t *seg_ids,
                                   const int32_t *seg_offsets, const int32_t *seg_insts, int num_segs, int num_pairs, int num_instances,
                                   const int64_t *counts, int64_t num_members, void *work, int64_t work_bytes, float *min_pt,
                                   float *max_pt, double *obb, int32_t *status, int32_t *info, nrpn_stream_t stream) {
  SegMap m;
  if (int rc = fill_segmap("scanbox_reduce", seg_ids, seg_offsets, seg_insts, num_segs, num_pairs, num_instances, m)) return rc;
  NRPN_REQUIRE(num_vertices >= 0 && num_vertices <= (1ll << 30), "scanbox_reduce: bad vertex count %lld", (long long)num_vertices);
  NRPN_REQUIRE(num_members >= 0 && num_members < (1ll << 31), "scanbox_reduce: bad member count %lld", (long long)num_members);
  NRPN_REQUIRE((num_vertices == 0 || (vertices && seg_of_vertex)) && counts && work && min_pt && max_pt && obb && status && info,
               "scanbox_reduce: null pointer");
  Work w;
  const size_t need = carve(w, (char *)work, num_instances, num_members);
  NRPN_REQUIRE(work_bytes >= (int64_t)need, "scanbox_reduce: work buffer of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  NRPN_REQUIRE(((uintptr_t)work & 15) == 0, "scanbox_reduce: work buffer not 16-byte aligned");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const long long *)counts, num_instances, (long long)num_members, w);
  if (num_vertices && num_segs)
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv64(num_vertices, kThreads)), dim3(kThreads), 0, st, seg_of_vertex,
                       (long long)num_vertices, m, w);
  hipLaunchKernelGGL(extremes_kernel, dim3(num_instances), dim3(kThreads), 0, st, vertices, w, min_pt, max_pt, obb, status);
  NRPN_HIP(hipMemcpyAsync(info, w.header, kHdrInts * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  NRPN_LAUNCH_CHECK("scanbox_reduce");
  return NRPN_OK;
}

extern "C" int nrpn_scanbox_hull(int num_instances, int64_t num_members, int max_survivors, int num_large, void *work, int64_t work_bytes,
                                 double *obb, int32_t *status, nrpn_stream_t stream) {
  NRPN_REQUIRE(num_instances >= 1 && num_instances < (1 << 20), "scanbox_hull: bad instance count %d", num_instances);
  NRPN_REQUIRE(num_members >= 0 && num_members < (1ll << 31), "scanbox_hull: bad member count %lld", (long long)num_members);
  NRPN_REQUIRE(max_survivors >= 0 && max_survivors <= num_members && num_large >= 0 && num_large <= num_instances && num_large < 65536,
               "scanbox_hull: bad survivor summary (%d, %d)", max_survivors, num_large);
  NRPN_REQUIRE(work && obb && status, "scanbox_hull: null pointer");
  Work w;
  const size_t need = carve(w, (char *)work, num_instances, num_members);
  NRPN_REQUIRE(work_bytes >= (int64_t)need, "scanbox_hull: work buffer of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
  hipStream_t st = as_stream(stream);
  NRPN_LDS(hull_lds_kernel, kLdsBytes);
  hipLaunchKernelGGL(hull_lds_kernel, dim3(num_instances), dim3(kThreads), kLdsBytes, st, w, (const int *)status);
  if (num_large > 0 && max_survivors > kLdsPoints) {
    long long P = 1;
    while (P < max_survivors) P <<= 1;
    const dim3 grid((unsigned)cdiv64(P / 2, kThreads), (unsigned)num_large);
    for (long long k = 2; k <= P; k <<= 1)
      for (long long j = k >> 1; j > 0; j >>= 1)
        hipLaunchKernelGGL(sort_step_kernel, grid, dim3(kThreads), 0, st, w, k, j, j == (k >> 1) ? 1 : 0);
    hipLaunchKernelGGL(hull_global_kernel, dim3(num_large), dim3(64), 0, st, w);
  }
  hipLaunchKernelGGL(rect_kernel, dim3(num_instances), dim3(kThreads), 0, st, w, obb, status);
  NRPN_LAUNCH_CHECK("scanbox_hull");
  return NRPN_OK;
}
