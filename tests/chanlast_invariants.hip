// Host check of the channels-last access layer's host side (csrc/chanlast.cuh): the multiply-shift divisors that make_fastdiv /
// make_voxel_div build, evaluated as the device evaluates them (fastdiv: mulhi(n, m) >> sh, d == 1 keeps n), against plain division;
// and the width rule.  Stand-alone: compile the host side only and run on the CPU,
//   hipcc --cuda-host-only -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined tests/chanlast_invariants.hip -o chanlast_invariants
// Prints the number of checks and exits 0, or prints the first violations and exits 1.
#include "../nerf_rpn_amd/csrc/chanlast.cuh"

#include <cstdio>
#include <vector>

static long long checks = 0, bad = 0;
#define EXPECT(cond, ...)                                            \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond) && ++bad <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

static unsigned host_fastdiv(unsigned n, const FastDiv &f) { return f.d == 1 ? n : (unsigned)(((unsigned long long)n * f.m) >> 32) >> f.sh; }

static const unsigned kMax = 0x7fffffffu;      // the contract: n < 2^31, 1 <= d < 2^31

static std::vector<unsigned> divisors() {
  std::vector<unsigned> d;
  for (unsigned v = 1; v <= 300; ++v) d.push_back(v);
  for (int l = 9; l <= 30; ++l)
    for (int o = -2; o <= 2; ++o) d.push_back((1u << l) + o);
  for (unsigned v : {1000u, 4096u * 3u, 64000u, 65535u, 65537u, 512000u, 999983u, 4096000u, 1u << 30, 0x55555555u, kMax - 2, kMax - 1, kMax}) d.push_back(v);
  return d;
}

static void check_divisor(unsigned d) {
  const FastDiv f = make_fastdiv(d);
  EXPECT(f.d == d, "make_fastdiv(%u).d = %u", d, f.d);
  auto one = [&](unsigned long long n) {
    if (n > kMax) return;
    EXPECT(host_fastdiv((unsigned)n, f) == (unsigned)n / d, "fastdiv(%llu, %u) = %u, want %u", n, d, host_fastdiv((unsigned)n, f), (unsigned)n / d);
  };
  for (unsigned long long n = 0; n < 40; ++n) one(n);
  // around every multiple of d near both ends and at powers of two: where a wrong magic number first shows
  for (unsigned long long q : {1ull, 2ull, 3ull, 7ull, 100ull, 65535ull, (unsigned long long)kMax / d - 1, (unsigned long long)kMax / d, (unsigned long long)kMax / d + 1})
    for (long long o = -2; o <= 2; ++o) { const long long n = (long long)(q * d) + o; if (n >= 0) one((unsigned long long)n); }
  for (int l = 1; l <= 31; ++l)
    for (long long o = -2; o <= 1; ++o) { const long long n = (1ll << l) + o; if (n >= 0) one((unsigned long long)n); }
  unsigned long long x = 88172645463325252ull + d;      // xorshift: a fixed pseudo-random sweep of n
  for (int i = 0; i < 2000; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; one(x & kMax); }
}

static void check_voxel_div(int ct, int nx, int ny, int nz, int scenes) {
  const VoxelDiv dv = make_voxel_div(ct, nx, ny, nz);
  EXPECT(dv.ct.d == (unsigned)ct && dv.x.d == (unsigned)nx && dv.y.d == (unsigned)ny && dv.z.d == (unsigned)nz, "make_voxel_div(%d, %d, %d, %d): divisors in the wrong slots", ct, nx, ny, nz);
  const unsigned long long total = (unsigned long long)scenes * nx * ny * nz * ct;
  if (total == 0 || total > kMax) return;
  auto one = [&](unsigned g) {
    // voxel_index<V>(g, dv), on the host
    const unsigned vox = host_fastdiv(g, dv.ct), t1 = host_fastdiv(vox, dv.z), t2 = host_fastdiv(t1, dv.y), b = host_fastdiv(t2, dv.x);
    const unsigned cgi = g - vox * dv.ct.d, z = vox - t1 * dv.z.d, y = t1 - t2 * dv.y.d, x = t2 - b * dv.x.d;
    unsigned v = g / ct;
    const unsigned wz = v % nz; v /= nz;
    const unsigned wy = v % ny; v /= ny;
    const unsigned wx = v % nx;
    EXPECT(vox == g / ct && cgi == g % ct && z == wz && y == wy && x == wx && b == v / nx,
           "voxel_index(%u) on (%d; %d, %d, %d): (%u; %u, %u, %u; %u), want (%u; %u, %u, %u; %u)", g, ct, nx, ny, nz, b, x, y, z, cgi, v / nx, wx, wy, wz, g % ct);
  };
  const unsigned t = (unsigned)total;
  for (unsigned g = 0; g < t && g < 3000; ++g) one(g);
  for (unsigned g = t > 3000 ? t - 3000 : 0; g < t; ++g) one(g);
  unsigned long long x = 0x9e3779b97f4a7c15ull ^ total;
  for (int i = 0; i < 3000; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; one((unsigned)(x % total)); }
}

static void check_width() {
  alignas(16) static char buf[64];
  for (int c = 4; c <= 4096; c += 4)
    for (int dtype : {(int)NRPN_F32, (int)NRPN_BF16}) {
      const int want = (dtype == NRPN_BF16 && c % 8 == 0) ? 8 : 4;
      EXPECT(cl_width(dtype, c) == want, "cl_width(%d, %d) = %d", dtype, c, cl_width(dtype, c));
      EXPECT(c % cl_width(dtype, c) == 0, "cl_width(%d, %d) does not divide C", dtype, c);
      for (int off : {0, 8, 16, 24, 2})
        for (int off2 : {0, 8, 16}) {
          const bool aligned = off % 16 == 0 && off2 % 16 == 0;
          const void *p = buf + off, *q = buf + off2, *none = nullptr;
          EXPECT(cl_width(dtype, c, p, q, none) == (aligned ? want : 4), "cl_width(%d, %d, +%d, +%d, null) = %d", dtype, c, off, off2, cl_width(dtype, c, p, q, none));
        }
    }
  int seen = 0;
  cl_dispatch(NRPN_F32, 8, [&](auto tag) { seen = decltype(tag)::V * 100 + (int)sizeof(typename decltype(tag)::T); });
  EXPECT(seen == 404, "cl_dispatch(f32, 8) chose %d: fp32 has no 8-wide form", seen);
  cl_dispatch(NRPN_BF16, 8, [&](auto tag) { seen = decltype(tag)::V * 100 + (int)sizeof(typename decltype(tag)::T); });
  EXPECT(seen == 802, "cl_dispatch(bf16, 8) chose %d", seen);
  cl_dispatch(NRPN_BF16, 4, [&](auto tag) { seen = decltype(tag)::V * 100 + (int)sizeof(typename decltype(tag)::T); });
  EXPECT(seen == 402, "cl_dispatch(bf16, 4) chose %d", seen);
  EXPECT(ew_blocks(0) == 1 && ew_blocks(1) == 1 && ew_blocks(257) == 2 && ew_blocks(1ll << 40) == 8192 && ew_blocks(1ll << 40, 1024) == 1024 && ew_blocks(kMax) == 8192,
         "ew_blocks edges");
}

int main() {
  for (unsigned d : divisors()) check_divisor(d);
  const int grids[][3] = {{1, 1, 1}, {9, 7, 5}, {10, 10, 10}, {5, 5, 5}, {160, 160, 160}, {200, 200, 130}, {1, 1, 1290}, {1290, 1, 1}, {3, 1, 2}, {256, 255, 257}};
  for (const auto &g : grids)
    for (int ct : {1, 2, 8, 9, 16, 64, 256})
      for (int scenes : {1, 2, 7}) check_voxel_div(ct, g[0], g[1], g[2], scenes);
  check_voxel_div(1, 1, 1, (int)kMax, 1);      // one axis as long as the contract allows
  check_voxel_div((int)kMax, 1, 1, 1, 1);
  check_width();
  std::printf("%lld checks, %lld violations\n", checks, bad);
  return bad ? 1 : 0;
}
