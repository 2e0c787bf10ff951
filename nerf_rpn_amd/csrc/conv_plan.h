// Launch plans of the conv3d translation unit: which kernel runs, on how many K slices, with which grid, and how many workspace bytes and
// statistics rows that implies.  Every plan is a pure function of (ConvShape, a knob snapshot, the per-call facts that matter); the size /
// plan queries and the launchers of csrc/conv3d.hip read the SAME plan value, so the bytes a query returns are the bytes the launch writes.
// Plain C++ (no HIP types): a host compiler can read this header on its own.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/nerfrpn.h"

// conv_halo.hip: the "halo" form of the 3x3x3 implicit GEMM (4 x 8 x 8 voxel blocks, input halo staged once per channel chunk)
namespace hk { constexpr int TX = 4, TY = 8, TZ = 8; }

static inline long long plan_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// What every plan is computed from; filled once at the entry point.
struct ConvShape {
  long long M;          // output rows (voxels; row-list form: list length)
  int n, gx, gy, gz;    // classic layout: n copies of one gx x gy x gz grid (ragged calls: unused)
  int cin, cout, wrows; // wrows: rows per tap of the packed weights (>= cout)
  int taps;             // 1 or 27
  int elem_bytes;       // 4 (fp32) or 2 (bf16)
  bool ragged;          // segments laid end to end instead of the classic layout
};
static inline ConvShape conv_shape(int n, int gx, int gy, int gz, int cin, int cout, int wrows, int ksize, int dtype) {
  return ConvShape{(long long)n * gx * gy * gz, n, gx, gy, gz, cin, cout, wrows, ksize == 3 ? 27 : 1, dtype == NRPN_F32 ? 4 : 2, false};
}
static inline ConvShape conv_shape_ragged(long long M, int cin, int cout, int wrows, int ksize, int dtype) {
  return ConvShape{M, 0, 1, 1, 1, cin, cout, wrows, ksize == 3 ? 27 : 1, dtype == NRPN_F32 ? 4 : 2, true};
}

// =====================================================================================================================
// forward / dgrad
// =====================================================================================================================
// A call resolves its Knobs from the process-wide defaults (developer switches, tools only) overridden by the caller's nrpn_conv_opts, so
// two threads with different plans never touch shared state while launching.
struct Knobs {
  int glds;        // 1: LDS-DMA loads (buffer_load ... lds), 0: register-staged loads
  int bm;          // tile selector: 0 auto, 128, 256 (wave-specialised 256x128), 512 (256x256, 8 waves), 1024 (256x256, 4 waves), 2048 (halo form)
  int stagger;     // 256x256 8-wave kernel: rotated K-step + staggered DMA issue (default) or the plain loop
  int big_split;   // mid-size grids run the 256x256 kernel on K slices
  int kb;          // K-step bytes of the k1/k3 kernels (64 or 128)
  int dbg;         // tools only: NRPN_CONV_DEBUG_* bits
  int halo_auto;   // 1 (default): the halo form is chosen automatically where it applies (40^3-class grids), 0: only on request (tile 2048)
  int halo_xp;     // halo form: taps paired across chunk boundaries (54 full K-steps per four chunks; Cin % 128 == 0) instead of 14 per chunk
};

// K slices of a launch of fewer than 128 tiles of 128 rows: about `target` workgroups, at least `min_steps` of the nk K-steps per slice, at
// most `cap` slices, none of them empty (every slice writes its whole partial); 1 = not sliced
static inline int k_slices(long long tiles, int nk, int target, int min_nk, int min_steps, int cap) {
  if (tiles >= 128 || nk < min_nk) return 1;
  long long k = (target + tiles - 1) / tiles;
  if (k > nk / min_steps) k = nk / min_steps;
  if (k > cap) k = cap;
  if (k < 2) return 1;
  const long long per = (nk + k - 1) / k;
  k = (nk + per - 1) / per;
  return k < 2 ? 1 : (int)k;
}
// Tail split of a launch of mt x nt tiles = whole rounds of the chip's `slots` workgroup slots + a remainder of at most half a round: the
// remainder's M tiles run on K slices, so that the last round lasts 1 / ks of a round (+ a small epilogue over those rows) instead of a
// whole one.  -> {first tail M tile, ks}; ks 0 = none.
struct TailSplit { int tile0, ks; };
static inline TailSplit tail_split(long long mt, long long nt, int slots, int nk, int min_steps) {
  const TailSplit none{0, 0};
  const long long tiles = mt * nt, rem = tiles % slots;
  if (tiles <= slots || rem == 0 || rem > slots / 2) return none;
  const long long tail_mt = (rem + nt - 1) / nt;
  int ks = (int)(slots / (tail_mt * nt));
  if (ks > 8) ks = 8;
  while (ks > 1 && nk / ks < min_steps) --ks;
  if (ks < 2) return none;
  const int per = (nk + ks - 1) / ks;
  ks = (nk + per - 1) / per;                 // no empty slice
  return ks >= 2 ? TailSplit{(int)(mt - tail_mt), ks} : none;
}

// split the K loop when the (M, N) tiling alone cannot fill 256 CUs (the 10^3 / 5^3 pyramid levels)
static inline int conv_ksplit(const ConvShape &s, const Knobs &kn) {
  const int bn = s.cout <= 64 ? 64 : 128;
  const int kb = (kn.kb == 128 && (s.cin * s.elem_bytes) % 128 == 0) ? 128 : 64;
  return k_slices(plan_cdiv(s.M, 128) * ((s.cout + bn - 1) / bn), s.taps * (s.cin * s.elem_bytes / kb), 384, 16, 8, 64);
}

// Mid-size grids (20^3: M = 8000) give only 32-64 tiles of 256x256: run the big kernel on K slices whose fp32 partials are
// written with plain stores to ws[z][M][Cout] and summed by the epilogue (no atomics).  Returns the slice count, 0 = not used.
static inline int conv_big_split(const ConvShape &s, const Knobs &kn) {
  if (!kn.big_split) return 0;
  if (s.elem_bytes != 2 || !kn.glds || kn.kb != 128 || (kn.bm != 0 && kn.bm != 512 && kn.bm != 1024) || s.cout < 256 || (s.cin * 2) % 128 != 0) return 0;
  const long long tiles = plan_cdiv(s.M, 256) * ((s.cout + 255) / 256);
  // measured inside the bench (20^3 maps): 512->512 (64 tiles, 4 slices) 123 us here vs 204 us on the 128-row kernel, but 256->256
  // (32 tiles, 8 slices of 13 K-steps) 56 us here vs 49 us there -- below ~48 tiles the slices get too short to amortise the 256 KB
  // partial-tile epilogue
  if (tiles < 48 || tiles >= 200) return 0;
  const int nk = s.taps * (s.cin / 64);
  int k = (int)((256 + tiles - 1) / tiles);
  if (k > 8) k = 8;
  while (k > 1 && nk / k < 8) --k;
  return k >= 2 ? k : 0;
}

// Tail split of a 256x256-tile launch on the 256 CUs (eval at 200 x 200 x 130: 323 tiles = 256 + 67).  Only single-column tilings
// (Cout = 256), bf16 in / bf16 out, no fused statistics.
static inline TailSplit conv_tail_split(const ConvShape &s, const Knobs &kn) {
  if (s.elem_bytes != 2 || !kn.glds || kn.kb != 128 || !kn.big_split || s.cout != 256 || (s.cin * 2) % 128 != 0) return TailSplit{0, 0};
  return tail_split(plan_cdiv(s.M, 256), 1, 256, s.taps * (s.cin / 64), 8);
}

// Halo form (conv_halo_kernel): bf16 3x3x3 on a classic grid whose 4 x 8 x 8 blocks waste little and still fill the chip.  It has an
// fp32-output epilogue too (no mask / statistics there: the entry points reject those).
static inline long long halo_tiles(const ConvShape &s) {
  return (long long)s.n * ((s.gx + hk::TX - 1) / hk::TX) * ((s.gy + hk::TY - 1) / hk::TY) * ((s.gz + hk::TZ - 1) / hk::TZ);
}
static inline bool halo_ok(const ConvShape &s, const Knobs &kn) {
  if (s.ragged || s.n <= 0 || s.taps != 27 || s.elem_bytes != 2 || !kn.glds || (s.cin % 32) != 0 || (s.cout & 7) != 0 || s.cout < 256) return false;
  if (kn.bm != 2048 && !(kn.bm == 0 && kn.halo_auto)) return false;
  const long long tiles = halo_tiles(s) * ((s.cout + 255) / 256);
  const double waste = (double)halo_tiles(s) * 256.0 / ((double)s.n * s.gx * s.gy * s.gz);
  if (kn.bm == 2048) return true;                       // forced (tools / tests): any grid
  return tiles >= 200 && waste <= 1.12;
}

// the tile family a (shape, Knobs) pair selects: 0 = 128-row, 1 = 256x256 8-wave, 4 = wave-specialised 256x128, 5 = 256x256 4-wave
static inline int conv_tile_kind(const ConvShape &s, bool sliced_big, const Knobs &kn) {
  const bool wide = kn.kb == 128 && (s.cin * s.elem_bytes) % 128 == 0;
  const bool can = kn.glds && wide && s.cout > 64 && s.elem_bytes == 2;
  const long long tiles_big = plan_cdiv(s.M, 256) * ((s.cout + 255) / 256);
  const bool huge = can && s.cout >= 256 && (sliced_big || kn.bm == 512 || kn.bm == 1024 || (kn.bm == 0 && tiles_big >= 200));
  if (huge) return (kn.bm == 1024 && !s.ragged) ? 5 : 1;
  if (can && kn.bm == 256 && !s.ragged) return 4;
  return 0;
}

// What the forward and the row-list plans share: the K slices of a launch of mt x nt tiles and the fp32 partials they leave in the workspace
struct SlicePlan {
  int ksplit;          // ConvArgs::ksplit: K slices over every row (1 = none)
  TailSplit tail;      // ks > 1: the M tiles from tile0 on run on ks K slices
  long long wgs;       // workgroups of the main launch
  long long ws_row0;   // the fp32 partials cover the rows from here on ...
  int ws_slices;       // ... on this many slices, summed by the epilogue launch (0 = the launch writes no workspace)
  size_t ws_bytes;     // = ws_slices * (M - ws_row0) * cout * 4
};
static inline void plan_slices(SlicePlan &p, const ConvShape &s, int bm, long long nt) {
  const long long mt = plan_cdiv(s.M, bm);
  p.wgs = p.tail.ks > 1 ? p.tail.tile0 * nt + (mt - p.tail.tile0) * nt * p.tail.ks : mt * nt * p.ksplit;
  p.ws_row0 = (long long)p.tail.tile0 * bm;
  p.ws_slices = p.tail.ks > 1 ? p.tail.ks : p.ksplit > 1 ? p.ksplit : 0;
  p.ws_bytes = (size_t)p.ws_slices * (s.M - p.ws_row0) * s.cout * 4;
}

struct FwdPlan : SlicePlan {
  int code;            // what nrpn_conv3d_fwd_plan reports: 0 = 128-row tile, 1 = 256x256 tile (8 waves), 2 = 256x256 tile on K slices,
                       // 3 = 128-row tile on K slices, 4 = wave-specialised 256x128 (opt-in), 5 = 256x256 tile on 4 waves, 6 = the same on K
                       // slices, 7 = halo form of the 3x3x3 kernel (4 x 8 x 8 voxel blocks)
  int kind;            // conv_tile_kind of the launch (code 7: unused)
  int kb;              // K-step bytes of the 128-row kernel: 128 where Cin * elemsize allows it, else 64
  int slices;          // ConvArgs::slices: 1 = the K slices run on the 256x256 kernel
  int halo_variant;    // code 7: nrpn_launch_conv_halo's variant word
  int stats_rows;      // rows P of the partial-statistics buffer [P][2][Cout] the launch fills when asked to; 0 = a kernel without fused
                       // statistics (K-sliced, fp32, narrow K-step or the opt-in variants -- use nrpn_bn_stats on the output instead)
};

// Order of the decisions: halo form, 256x256 on K slices, 128-row on K slices, tile kind, tail split.  The per-call facts besides the shape:
// no workspace = no K slices of any kind; fp32 output or requested statistics = no tail split.  The size / plan queries know none of them
// and plan for the defaults, so they reserve the tail-split bytes also for calls that will not take the tail split.
static inline FwdPlan fwd_plan(const ConvShape &s, const Knobs &kn, bool workspace = true, bool out_f32 = false, bool stats = false) {
  FwdPlan p{};
  p.ksplit = 1;
  p.kb = (kn.kb == 128 && (s.cin * s.elem_bytes) % 128 == 0) ? 128 : 64;
  const bool stats_able = s.elem_bytes == 2 && (s.cout & 7) == 0 && kn.glds && kn.bm != 256;
  if (halo_ok(s, kn)) {
    p.code = 7;
    p.wgs = halo_tiles(s) * ((s.cout + 255) / 256);
    const int v = (kn.dbg >> 12) & 3;          // NRPN_CONV_DEBUG_VARIANT
    const bool xp = s.cin % 128 == 0 && !v && (kn.halo_xp == 1 || (kn.halo_xp == 2 && s.cin >= 256));
    p.halo_variant = v | (xp ? 4 : 0) | (out_f32 ? 8 : 0);
    p.stats_rows = stats_able ? (int)(halo_tiles(s) * 2) : 0;
    return p;
  }
  if (const int bs = workspace ? conv_big_split(s, kn) : 0) {
    p.ksplit = bs; p.slices = 1;
    p.kind = conv_tile_kind(s, true, kn);
    p.code = p.kind == 5 ? 6 : 2;
  } else if (workspace && (p.ksplit = conv_ksplit(s, kn)) > 1) {
    p.code = 3;
  } else {
    p.ksplit = 1;
    p.code = p.kind = conv_tile_kind(s, false, kn);
    if (p.kind == 1 && workspace && !s.ragged && !stats && !out_f32) p.tail = conv_tail_split(s, kn);
  }
  const bool huge = p.kind == 1 || p.kind == 5;
  const int bm = p.kind ? 256 : 128, bn = huge ? 256 : s.cout <= 64 ? 64 : 128;
  plan_slices(p, s, bm, (s.cout + bn - 1) / bn);
  if (stats_able && huge && p.ksplit == 1) p.stats_rows = (int)(plan_cdiv(s.M, 256) * 2);
  else if (stats_able && p.code == 0 && p.kb == 128) p.stats_rows = (int)(plan_cdiv(s.M, 128) * (s.cout <= 64 ? 4 : 2));
  return p;
}

// =====================================================================================================================
// row-list forward / dgrad (128-row tiles of conv_igemm_kernel<..., ROWS>)
// =====================================================================================================================
struct RowsKnobs { int big, tail; };     // nrpn_set_rows_big_tile, nrpn_set_rows_tail_split

// Short lists (the S0 / S1 cones: 2-70 tiles) would leave the chip idle behind a 54-step K loop: they run on K slices whose fp32 partials
// ([slices][nrows][Cout], plain stores) are summed in slice order and scattered by rows_epilogue_kernel.
// Long lists: the 128-row tiling of the S3 cone is a little more than one round of the chip's 512 workgroup slots (33-35 k rows x 2 column
// tiles = 518-552 workgroups), i.e. two rounds in time: tail split.
struct RowsPlan : SlicePlan {
  bool big;            // opt-in 256x256 tile (no K slices, no tail, no epilogue launch); ws_bytes stays what the size query reserves: the
                       // query does not know this form
};
static inline RowsPlan rows_plan(const ConvShape &s, const RowsKnobs &kn, bool workspace = true, bool out_f32 = false) {
  RowsPlan p{};
  const long long mt = plan_cdiv(s.M, 128), nt = (s.cout + 127) / 128;
  const int nk = s.taps * (s.cin * s.elem_bytes / 128);
  p.ksplit = workspace ? k_slices(mt * nt, nk, 256, 12, 6, 32) : 1;
  if (p.ksplit == 1 && workspace && kn.tail) p.tail = tail_split(mt, nt, 512, nk, 6);
  plan_slices(p, s, 128, nt);
  // opt-in (nrpn_set_rows_big_tile): long bf16 lists (>= 96 tiles of 256 rows) of wide layers on the 256x256 tile
  const long long big_tiles = plan_cdiv(s.M, 256) * ((s.cout + 255) / 256);
  if (kn.big && s.elem_bytes == 2 && !out_f32 && p.ksplit == 1 && s.cout >= 256 && (s.cout & 7) == 0 && big_tiles >= 96) {
    p.big = true; p.tail = TailSplit{0, 0}; p.wgs = big_tiles; p.ws_row0 = 0; p.ws_slices = 0;
  }
  return p;
}

// =====================================================================================================================
// weight gradient
// =====================================================================================================================
// How the voxel axis is cut: every (tile, tap, slice) workgroup writes one partial gradient; the slices are summed by the
// unpack kernels.  `ksplit` is trimmed so that no slice is empty (every partial is fully written).
struct WgKnobs {
  int big;     // nrpn_set_wgrad_big_tile: 256x256 wgrad tiles for bf16 layers with Cout, Cin >= 256 (tuning knob)
  int tr;      // nrpn_set_wgrad_transpose_read
  int pack2;   // nrpn_set_wgrad_pack2: two taps per workgroup (conv_wgrad_kernel<..., PACK2>): dense k3 layers whose input row fits half a
               // B-tile row (Cin <= 64); conv_wgrad_big_kernel<false, PACK2> for Cin 128
};
enum WgForm { WG_128, WG_PAIR, WG_BIG, WG_BIG_PAIR, WG_ROWS, WG_BIG_ROWS };
struct WgPlan {
  WgForm form;         // 128x128, pair of taps on 128x128, 256x256, pair of taps on 256x256, row list on 128x128, row list on 256x256
  bool big;            // a 256x256 form (what nrpn_conv3d_wgrad_plan reports)
  bool tr;             // WG_128: transpose-read fragments
  int ksplit;          // slices of the voxel axis = partial gradients
  int ntiles_n;        // WgradArgs::ntiles_n
  long long wgs;
  size_t bias_off;     // workspace = [tap mask: M u32 (k3, not for row lists)][bias partials: ksplit * wrows f32]
  size_t bias_bytes;
};
static inline size_t wgrad_mask_bytes(long long M, int taps) { return taps == 27 ? (size_t)((M * 4 + 255) / 256 * 256) : 0; }
// mode 0: k1 / k3 layers (ncols = Cin);  mode 1: the stem's GEMM form (ncols = Kpad, taps = 1);  rows: row-list form of mode 0
static inline WgPlan wgrad_plan(const ConvShape &s, int ncols, int mode, const WgKnobs &kn, bool rows = false) {
  WgPlan pl{};
  const int kv = s.elem_bytes == 4 ? 32 : 64;
  const long long chunks = (s.M + kv - 1) / kv;
  long long ks = 1;
  const bool big_pair = kn.pack2 && s.taps == 27 && s.cin == 128;
  const bool pair = kn.pack2 && mode == 0 && s.taps == 27 && s.cin <= 64;
  if (mode == 0 && s.elem_bytes == 2 && kn.big && kn.tr && s.cout >= 256 && (s.cin >= 256 || big_pair)) {
    // 256x256 tiles, one 128 KB-LDS workgroup per CU: pick the slice count with the lowest modelled time
    //   t(k) = MFMA time / (fill of whole rounds of 256 CUs) + (k + 1) partial-gradient passes through HBM,
    // e.g. 256->256 @40^3: 27 tiles x 9 slices = 243 workgroups (95 % of a round) instead of 8 (84 %); 512->512 @20^3 stays at 2
    // slices because each extra slice costs another 28 MB partial.
    const int tiles = ((s.wrows + 255) / 256) * ((s.cin + 255) / 256) * (big_pair ? 14 : s.taps);
    const double flops = 2.0 * (double)s.M * s.wrows * s.cin * s.taps;
    const double part_bytes = 4.0 * (double)s.taps * s.wrows * s.cin;
    double best = 1e30;
    for (long long k = 1; k <= 64 && k <= (chunks / 16 > 1 ? chunks / 16 : 1); ++k) {
      const double rounds = (double)tiles * k / 256.0;
      const long long whole = (long long)rounds + ((double)(long long)rounds < rounds ? 1 : 0);
      const double fill = rounds / (double)whole;
      if (fill < 0.5) continue;
      const double t = flops / (fill * 9.0e14) + (double)(k + 1) * part_bytes / 3.0e12;
      if (t < best) { best = t; pl.big = true; ks = k; }
    }
  }
  if (!pl.big) {
    const int tiles = ((s.wrows + 127) / 128) * ((ncols + 127) / 128) * (pair ? 14 : s.taps);
    ks = (1024 + tiles - 1) / tiles;
    if (ks > chunks / 16) ks = chunks / 16;     // >= 16 chunks per workgroup so the 128x128 epilogue stays amortised
    if (ks < 1) ks = 1;
    if (ks > 4096) ks = 4096;
  }
  const long long per = (chunks + ks - 1) / ks;
  pl.ksplit = (int)((chunks + per - 1) / per);
  // the slice count above models the pair forms whenever their switch is on; the row-list kernels and the plain-read 128x128 kernel have
  // no pair form and run one tap per workgroup on that slice count
  const int tile = pl.big ? 256 : 128;
  pl.form = rows ? (pl.big ? WG_BIG_ROWS : WG_ROWS) : pl.big ? (big_pair && s.cin == 128 ? WG_BIG_PAIR : WG_BIG) : (pair && kn.tr ? WG_PAIR : WG_128);
  const bool two = pl.form == WG_PAIR || pl.form == WG_BIG_PAIR;
  pl.tr = kn.tr != 0;
  pl.ntiles_n = two ? 1 : (ncols + tile - 1) / tile;
  pl.wgs = (long long)((s.wrows + tile - 1) / tile) * pl.ntiles_n * (two ? 14 : mode == 0 ? s.taps : 1) * pl.ksplit;
  pl.bias_off = rows ? 0 : wgrad_mask_bytes(s.M, s.taps);
  pl.bias_bytes = (size_t)pl.ksplit * s.wrows * 4;
  return pl;
}

// Stem weight gradient: the z-row form (stride 2, even Z, Cout 64) or the GEMM form of wgrad_plan (mode 1).
static inline int stem_kpad(int elem_bytes) { const int ke = 64 / elem_bytes; return ((343 * 4 + ke - 1) / ke) * ke; }
struct StemWgPlan {
  bool zrow;
  int slices;
  long long slice_floats;   // floats of ONE slice partial: z-row form [49][cout][32], otherwise [cout][Kpad]
  size_t ws_bytes;          // bias partials: slices * cout f32
  WgPlan gemm;              // GEMM form only
};
// M = output voxels
static inline StemWgPlan stem_wgrad_plan(long long M, int gz, int cout, int stride, int elem_bytes, const WgKnobs &kn) {
  StemWgPlan p{};
  p.zrow = stride == 2 && gz % 2 == 0 && cout == 64;
  if (p.zrow) {
    const long long chunks = (M + (elem_bytes == 2 ? 64 : 32) - 1) / (elem_bytes == 2 ? 64 : 32);
    long long k = 73;                                   // 7 dx x 73 slices = 511 workgroups = two per CU
    if (k > chunks / 8) k = chunks / 8;
    if (k < 1) k = 1;
    const long long per = (chunks + k - 1) / k;
    p.slices = (int)((chunks + per - 1) / per);         // no empty slice
    p.slice_floats = (long long)49 * cout * 32;
  } else {
    const int kpad = stem_kpad(elem_bytes);
    p.gemm = wgrad_plan(ConvShape{M, 0, 1, 1, 1, 4, cout, cout, 1, elem_bytes, false}, kpad, 1, kn);
    p.slices = p.gemm.ksplit;
    p.slice_floats = (long long)cout * kpad;
  }
  p.ws_bytes = (size_t)p.slices * cout * 4;
  return p;
}
