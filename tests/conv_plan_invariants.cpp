// Stand-alone host check of the launch plans' own invariants (tests/test_conv_plans.py compiles and runs it): includes the planning header
// with a plain C++ compiler and walks the sweep of tests/conv_plan_sweep.py over every plan family.
#include <cstdio>
#include <initializer_list>

#include "../nerf_rpn_amd/csrc/conv_plan.h"

static long long fails = 0, checked = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++checked;                                                            \
    if (!(cond) && ++fails <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

// ks slices of nk steps, ceil(nk / ks) steps each: the last slice is not empty
static bool no_empty_slice(long long nk, long long ks) { return ks >= 1 && plan_cdiv(nk, plan_cdiv(nk, ks)) == ks; }

static const int kGrids[][3] = {{5, 5, 5}, {10, 10, 10}, {20, 20, 20}, {40, 40, 40}, {80, 80, 80}, {160, 160, 160}, {200, 200, 130}, {42, 42, 40},
                                {13, 11, 9}, {420, 1, 1}, {8000, 1, 1}, {70560, 1, 1}};
static const int kCh[] = {16, 32, 64, 96, 128, 256, 264, 512};
static const long long kRows[] = {1, 127, 128, 129, 300, 9000, 33000, 35000, 66000, 70000};

static void check_fwd(const ConvShape &s, const Knobs &kn, bool workspace, bool out_f32, bool stats) {
  const FwdPlan p = fwd_plan(s, kn, workspace, out_f32, stats);
  const char *fmt = "M=%lld cin=%d cout=%d taps=%d es=%d bm=%d code=%d";
#define AT fmt, s.M, s.cin, s.cout, s.taps, s.elem_bytes, kn.bm, p.code
  CHECK(p.wgs > 0 && p.wgs < (1ll << 31), AT);
  const long long nk128 = s.taps * (s.cin * s.elem_bytes / p.kb), nk256 = s.taps * (s.cin / 64);
  if (p.code == 3) CHECK(p.ksplit >= 2 && no_empty_slice(nk128, p.ksplit), AT);
  if (p.code == 2 || p.code == 6) CHECK(p.ksplit >= 2 && p.slices == 1 && no_empty_slice(nk256, p.ksplit), AT);
  if (p.code != 2 && p.code != 3 && p.code != 6) CHECK(p.ksplit == 1 && p.slices == 0, AT);
  CHECK(workspace || (p.ksplit == 1 && p.tail.ks == 0 && p.ws_bytes == 0), AT);
  size_t bytes = 0;
  if (p.ksplit > 1) bytes = (size_t)p.ksplit * s.M * s.cout * 4;
  if (p.tail.ks > 1) {
    const long long mt = plan_cdiv(s.M, 256), nt = (s.cout + 255) / 256;
    CHECK(p.code == 1 && p.ksplit == 1 && !stats && !out_f32 && !s.ragged && s.elem_bytes == 2, AT);
    CHECK(p.tail.tile0 > 0 && p.tail.tile0 < mt && (long long)p.tail.tile0 * 256 < s.M, AT);      // whole rows [0, tile0 * 256) + tail rows = M
    CHECK(p.wgs == p.tail.tile0 * nt + (mt - p.tail.tile0) * nt * p.tail.ks, AT);
    CHECK(no_empty_slice(nk256, p.tail.ks), AT);
    bytes = (size_t)p.tail.ks * (s.M - (long long)p.tail.tile0 * 256) * s.cout * 4;
  } else {
    CHECK(p.tail.ks == 0 && p.tail.tile0 == 0, AT);
  }
  CHECK(p.ws_bytes == bytes, AT);
  CHECK((p.ws_slices > 0) == (bytes > 0), AT);
  // statistics rows: none on K slices, in fp32 or on the opt-in 256x128 tile; always on the bf16 256x256 / halo forms with Cout % 8 == 0
  if (p.code == 2 || p.code == 3 || p.code == 4 || p.code == 6 || s.elem_bytes == 4 || (s.cout & 7)) CHECK(p.stats_rows == 0, AT);
  else if (p.code != 0 && kn.bm != 256) CHECK(p.stats_rows > 0, AT);
  else CHECK((p.stats_rows > 0) == (p.kb == 128 && kn.glds && kn.bm != 256), AT);
#undef AT
}

static void check_rows(const ConvShape &s, const RowsKnobs &kn, bool workspace, bool out_f32) {
  const RowsPlan p = rows_plan(s, kn, workspace, out_f32);
  const char *fmt = "rows=%lld cin=%d cout=%d taps=%d es=%d big=%d";
#define AT fmt, s.M, s.cin, s.cout, s.taps, s.elem_bytes, (int)p.big
  const long long nk = s.taps * (s.cin * s.elem_bytes / 128), mt = plan_cdiv(s.M, 128), nt = (s.cout + 127) / 128;
  CHECK(p.wgs > 0 && p.wgs < (1ll << 31), AT);
  CHECK(no_empty_slice(nk, p.ksplit), AT);
  CHECK(workspace || (p.ksplit == 1 && p.tail.ks == 0 && p.ws_bytes == 0), AT);
  if (p.big) { CHECK(p.ksplit == 1 && p.tail.ks == 0 && p.ws_slices == 0, AT); return; }
  size_t bytes = p.ksplit > 1 ? (size_t)p.ksplit * s.M * s.cout * 4 : 0;
  if (p.tail.ks > 1) {
    CHECK(p.ksplit == 1 && p.tail.tile0 > 0 && p.tail.tile0 < mt && (long long)p.tail.tile0 * 128 < s.M, AT);
    CHECK(p.wgs == p.tail.tile0 * nt + (mt - p.tail.tile0) * nt * p.tail.ks && no_empty_slice(nk, p.tail.ks), AT);
    bytes = (size_t)p.tail.ks * (s.M - (long long)p.tail.tile0 * 128) * s.cout * 4;
  } else {
    CHECK(p.wgs == mt * nt * p.ksplit, AT);
  }
  CHECK(p.ws_bytes == bytes && (p.ws_slices > 0) == (bytes > 0), AT);
#undef AT
}

static void check_wgrad(const ConvShape &s, const WgKnobs &kn, bool rows) {
  const WgPlan p = wgrad_plan(s, s.cin, 0, kn, rows);
  const char *fmt = "M=%lld cin=%d cout=%d wrows=%d taps=%d es=%d form=%d";
#define AT fmt, s.M, s.cin, s.cout, s.wrows, s.taps, s.elem_bytes, (int)p.form
  CHECK(p.wgs > 0 && p.wgs < (1ll << 31), AT);
  CHECK(no_empty_slice(plan_cdiv(s.M, s.elem_bytes == 4 ? 32 : 64), p.ksplit), AT);
  CHECK(p.big == (p.form == WG_BIG || p.form == WG_BIG_PAIR || p.form == WG_BIG_ROWS), AT);
  CHECK(rows == (p.form == WG_ROWS || p.form == WG_BIG_ROWS), AT);
  CHECK(!p.big || (s.elem_bytes == 2 && kn.big && kn.tr), AT);
  CHECK((p.form != WG_PAIR && p.form != WG_BIG_PAIR) || (kn.pack2 && kn.tr && s.taps == 27 && p.ntiles_n == 1), AT);
  CHECK(p.bias_bytes == (size_t)p.ksplit * s.wrows * 4 && p.bias_off % 256 == 0 && p.bias_off >= (rows || s.taps == 1 ? 0 : (size_t)s.M * 4), AT);
#undef AT
}

int main() {
  const Knobs def{1, 0, 1, 1, 128, 0, 1, 2};
  for (const auto &g : kGrids)
    for (int n = 1; n <= (g[1] > 1 ? 2 : 1); ++n)
      for (int cin : kCh)
        for (int cout : kCh)
          for (int ksize : {1, 3})
            for (int dtype : {(int)NRPN_F32, (int)NRPN_BF16}) {
              ConvShape s = conv_shape(n, g[0], g[1], g[2], cin, cout, cout, ksize, dtype);
              for (int wrows : {cout, 2 * cout})
                for (int sw = 0; sw < 4; ++sw) {
                  s.wrows = wrows;
                  const WgKnobs wk{sw != 1, sw != 2, sw != 3};
                  check_wgrad(s, wk, false);
                  if (n == 1 && g[1] == 1) check_wgrad(s, wk, true);
                }
              s.wrows = cout;
              if ((cin * s.elem_bytes) % 64 != 0) continue;
              for (int v = 0; v < 14; ++v) {
                Knobs kn = def;
                if (v >= 1 && v <= 5) kn.bm = 64 << v;      // 128 .. 2048
                if (v == 6) kn.glds = 0;
                if (v == 7) kn.kb = 64;
                if (v == 8) kn.stagger = 0;
                if (v == 9) kn.big_split = 0;
                if (v == 10) kn.halo_xp = 1;
                if (v == 11) kn.halo_xp = 0;
                if (v == 12) kn.halo_auto = 0;
                if (v == 13) kn.dbg = NRPN_CONV_DEBUG_VARIANT;
                for (int fct = 0; fct < 5; ++fct) {       // the queries' facts, then each fact of a call alone, then a ragged call
                  ConvShape t = s;
                  if (fct == 4) t = conv_shape_ragged(s.M, cin, cout, cout, ksize, dtype);
                  check_fwd(t, kn, fct != 1, fct == 2, fct == 3);
                }
              }
            }
  for (long long nrows : kRows)
    for (int cin : kCh)
      for (int cout : kCh)
        for (int ksize : {1, 3})
          for (int dtype : {(int)NRPN_F32, (int)NRPN_BF16}) {
            const ConvShape s = conv_shape_ragged(nrows, cin, cout, cout, ksize, dtype);
            if ((cin * s.elem_bytes) % 128 != 0) continue;
            for (int big = 0; big < 2; ++big)
              for (int tail = 0; tail < 2; ++tail)
                for (int ws = 0; ws < 2; ++ws)
                  for (int of32 = 0; of32 < 2; ++of32) check_rows(s, RowsKnobs{big, tail}, ws != 0, of32 != 0 || dtype == NRPN_F32);
          }
  for (const auto &g : kGrids)
    for (int n = 1; n <= 2 && g[1] > 1; ++n)
      for (int cout : kCh)
        for (int stride : {1, 2})
          for (int es : {4, 2}) {
            const long long M = (long long)n * ((g[0] - 1) / stride + 1) * ((g[1] - 1) / stride + 1) * ((g[2] - 1) / stride + 1);
            const StemWgPlan p = stem_wgrad_plan(M, g[2], cout, stride, es, WgKnobs{1, 1, 1});
            const char *fmt = "stem M=%lld cout=%d stride=%d es=%d zrow=%d";
            CHECK(no_empty_slice(plan_cdiv(M, es == 4 ? 32 : 64), p.slices), fmt, M, cout, stride, es, (int)p.zrow);
            CHECK(p.ws_bytes == (size_t)p.slices * cout * 4 && p.slice_floats == (p.zrow ? 49ll * cout * 32 : (long long)cout * stem_kpad(es)), fmt, M,
                  cout, stride, es, (int)p.zrow);
            CHECK(p.zrow || (p.gemm.form == WG_128 && p.gemm.wgs > 0 && p.gemm.wgs < (1ll << 31) && p.gemm.ksplit == p.slices), fmt, M, cout, stride,
                  es, (int)p.zrow);
          }
  std::printf("%lld checks, %lld failed\n", checked, fails);
  return fails ? 1 : 0;
}
