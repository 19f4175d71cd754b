// Which kernel family serves a pass: the shape and the request in, a Route value out.  choose_route() is the only place where
// the precedence between the families is written; the entry points (Theta image), run_pass (launches, grid) and mimo_plan /
// mimo_plan_shape (description) all take its Route.  Below the family, two_stage_plan() at the end of this file decides what a
// two-stage pass launches (TwoStagePlan), and label_stats_plan() (mimo_label_stats.hip, LabelStatsPlan in mimo_extra.h) which
// label-statistics kernel closes a label pass: launcher, grid and description read those two values the same way.
// Host only, included by mimo_abi.cpp (and the host tool tools/stage_plan_sweep.cpp); no HIP call below.
#pragma once
#include "mimo_kernels.h"
#include "mimo_extra.h"

#include <cstdint>
#include <cstdlib>

namespace mimo {

struct RouteShape {           // the data a pass runs on
  int D, F, F16, structure;
  int64_t N, n_bad;           // rows; rows with a NaN
  bool aligned16;             // the rows start on a 16-byte boundary
};

struct RouteRequest {         // what the caller asks of the pass
  int src = kSrcEstep;        // kSrcWeights / kSrcLabels: statistics of a caller's table / labels, no E-step in front
  bool gibbs = false;         // label pass (softmax pass otherwise)
  bool tables = false;        // tables kept or the entropy split: not a plain request
  bool stats = true;          // statistics wanted (a softmax pass without them and without tables is bound-only)
  bool weighted = false;      // caller's row weights
  bool device_out = false;
};

enum class Family { Small, Narrow, Mid, MidLabels, Rowwave, RowwaveVi, Fused, TwoStage, LabelStats };   // LabelStats: kSrcLabels only
enum class Image { Generic, Small, Narrow, Mid, MidLabels, RowOwner };                                  // Theta layouts (placements of mimo_theta.h)

struct Route {
  Family family = Family::Fused;
  int narrow_mode = 0;        // Family::Narrow: 1 softmax + statistics, 2 label draw with the label-statistics kernel behind it, 3 label draw + statistics in one pass
  bool promoted = false;      // a bound-only request that runs as the plain pass: its statistics stay in the partial blocks
  Image image = Image::Generic;
  // a label kernel with the label-statistics kernels behind it
  bool label_draw() const { return family == Family::Rowwave || family == Family::MidLabels || (family == Family::Narrow && narrow_mode == 2); }
};

static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

// Tuning knobs of the router.  Process-wide (include/mimo_hip.h): mimo_tune on any context writes them for all.
struct RouteTunables {
  bool small_on = env_int("MIMO_SMALL", 1) != 0;
  bool rowwave_on = env_int("MIMO_ROWWAVE", 1) != 0;
  bool narrow_fused_labels = env_int("MIMO_NARROW_FUSED_LABELS", 1) != 0;
  int bound_promote = env_int("MIMO_BOUND_PROMOTE", 1);          // 0: no bound-only request runs as the plain pass, 2: every shape of the narrow / mid kernels
  int mid_min_d = env_int("MIMO_MID_MIN_D", 0);                  // (mimo_tune "mid_min_d"; 0: the measured rule)
  int mid_narrow_k = env_int("MIMO_MID_NARROW_K", 0);            // (mimo_tune "mid_narrow_k")
  int mid_labels_min_d = env_int("MIMO_MID_LABELS_MIN_D", 0);    // (mimo_tune "mid_labels_min_d")
  int mid_labels_narrow_k = 0;  // (mimo_tune "mid_labels_narrow_k": K from which the label mode goes before the narrow label kernels; 0: measured rule)
  int bound_promote_mid_k = 16; // largest K of a mid-kernel shape whose bound-only pass runs as the plain pass (profiles/r04_bound_pass.txt: N = 2e6, ms generic / plain:
                                // Dz=20 K=16 1.02 / 0.73, Dz=32 K=16 1.73 / 1.51 — but Dz=24 K=32 1.51 / 1.68, Dz=16 K=48 0.99 / 1.31; every narrow shape gains: Dz=2 K=50
                                // 0.37 / 0.16, Dz=1 K=100 0.77 / 0.20, Dz=4 K=128 0.75 / 0.62, Dz=16 K=4 0.65 / 0.23, Dz=32 K=4 1.73 / 0.81)
};
static RouteTunables g_route_tunables;

// Row stride of the data tile (doubles): what fill_args hands the kernels and every coverage predicate below is asked with
inline int route_zs(int K, int D) {
  return (K + 15) / 16 > 12 ? D + 2      // K > 192: every byte counts to keep two workgroups per CU (<= 80 KB each)
                            : ((D + 2) | 1);   // odd stride: conflict-free row reads
}

// Does this (data, K) run on the small-shape VALU kernel (mimo_small.hip)?  Dz <= 4, K <= 32, 16-byte aligned rows.
inline bool use_small(const RouteShape& s, int K, const RouteTunables& t) {
  return t.small_on && small_covers(s.D, K) && s.aligned16;
}

// Label pass on the row-owner kernels (mimo_rowwave.hip): Dz <= 9 (beyond the small-shape kernel's range), full structure, nothing but labels
// (+ their statistics) requested.
inline bool use_rowwave(const RouteShape& s, int K, bool wants_tables, const RouteTunables& t) {
  if (!t.rowwave_on || wants_tables) return false;
  return rowwave_covers(K, s.F16, route_zs(K, s.D)) && label_stats_covers(K, s.D, s.structure);
}

// Passes of the narrow shapes (mimo_narrow.hip: F <= 16 features, 32 < K <= 128 on the 4x4x4 matrix instruction): plain
// requests only — nothing but statistics + scalars (softmax pass) or labels + their statistics (label pass).
// Returns the kernel mode + 1 (1: softmax + statistics, 2: label draw with the label-statistics kernel behind it, 3: label draw +
// statistics in one pass — few components over many features, MIMO_NARROW_FUSED_LABELS=0: off) or 0.
inline int use_narrow(const RouteShape& s, int K, bool gibbs, bool plain, bool stats, const RouteTunables& t) {
  if (!plain) return 0;                 // (the small-shape kernel keeps the generic requests of its range and the shapes below narrow_covers' K)
  const int ZS = route_zs(K, s.D);
  if (!gibbs) return narrow_covers(K, s.F, s.D, ZS, 0) ? 1 : 0;     // (rows with NaN: their mask is the row-weight vector of the pass)
  const bool two = narrow_covers(K, s.F, s.D, ZS, 1) && label_stats_covers(K, s.D, s.structure);
  const bool one = t.narrow_fused_labels && s.n_bad == 0 && narrow_covers(K, s.F, s.D, ZS, 2);
  if (one && !two) return 3;
  // both exist: the fused pass wins while its second product is cheap next to a second pass over Z (profiles/r03_wide_sweep_fused_labels.txt,
  // N = 2e6, us per sweep, label kernel + label statistics / fused: Dz=8 K=4 154 / 93, K=8 154 / 129, K=16 181 / 194; Dz=12 K=8 237 / 208,
  // K=16 312 / 395; Dz=16 K=4 256 / 213, K=8 315 / 374, K=16 430 / 649)
  const int V = narrow_v(K), D = s.D;
  if (one && stats && (V == 1 || (D <= 6 && V <= 6) || (D <= 12 && V <= 3))) return 3;
  return two ? 2 : 0;
}

// Softmax + statistics pass of the mid shapes (mimo_mid.hip): plain requests (statistics + scalars, row weights / the NaN mask
// allowed), full feature map, K <= 32 where neither the narrow kernels (few components) nor the single-pass tile kernels do
// better — measured per shape (profiles/r04_mid_kernel_sweep.txt): from Dz = 17 everything the narrow kernels do not take;
// MIMO_MID_MIN_D moves the lower end (tuning knob)
inline bool use_mid(const RouteShape& s, int K, bool plain, const RouteTunables& t) {
  const int D = s.D;
  if (!plain || !mid_covers(K, D, s.structure)) return false;
  if (t.mid_min_d > 0 || t.mid_narrow_k > 0)       // forced by the caller (tests, sweeps)
    return D >= (t.mid_min_d > 0 ? t.mid_min_d : 5) &&
           (K >= (t.mid_narrow_k > 0 ? t.mid_narrow_k : 33) || !use_narrow(s, K, false, plain, true, t));
  // measured (tools/mid_sweep.py, profiles/r04_mid_kernel_sweep.txt; fraction of the float64 rate, other route -> mid):
  //   K = 17 .. 32: from Dz = 13 (Dz=13 K=32 0.55 -> 0.61, Dz=14 0.58 -> 0.66, Dz=16 0.61 -> 0.64, Dz=20 0.41 -> 0.69, Dz=32 0.48 -> 0.75;
  //                 Dz=12 K=32 0.61 -> 0.57 and Dz=11 0.53 -> 0.50 stay on the tile / row-owner kernels)
  //   K = 13 .. 16: from Dz = 12 against the narrow kernels (Dz=12 K=16 0.41 -> 0.49, Dz=14 0.44 -> 0.58, Dz=16 0.42 -> 0.57; Dz=11 0.45 -> 0.43)
  //   K <= 12: the narrow kernels where they exist (Dz=16 K=12 0.44 = 0.44, Dz=15 0.42 -> 0.38, Dz=20 K=8 0.37 -> 0.30) up to Dz = 23
  //            (Dz=24 K=8 0.31 -> 0.32, Dz=26 K=8 0.19 -> 0.34); beyond them the two-stage path was all there was (Dz=20 K=12 0.18 -> 0.47)
  //   K = 33 .. 48: from Dz = 9 (Dz=9 K=48 0.48 -> 0.55, Dz=12 0.56 -> 0.60, Dz=16 0.57 -> 0.67, Dz=20 0.46 -> 0.71, Dz=26 0.52 -> 0.80; Dz=10, 11: level)
  //   K = 49 .. 64: from Dz = 18 (Dz=18 K=64 0.64 -> 0.68, Dz=20 0.61 -> 0.76, Dz=21 0.66 -> 0.79, one wave per SIMD from Dz = 22: Dz=24 0.57 -> 0.63,
  //                 Dz=28 0.63 -> 0.68; below, ten column blocks do not divide over eight waves and the tile kernels keep K = 64: Dz=16 0.78 against 0.57)
  //   K = 65 .. 96: wherever the kernels exist from Dz = 6 (five / six row blocks instead of the eight the tile and two-stage kernels pay for:
  //                 Dz=8 K=96 0.43 -> 0.56, Dz=9 K=72 0.35 -> 0.56, Dz=12 K=96 0.46 -> 0.62, Dz=14 K=80 0.35 -> 0.71, Dz=16 K=80 0.42 -> 0.60; with one
  //                 wave per SIMD: Dz=16 K=96 0.47 -> 0.61, Dz=20 K=96 0.48 -> 0.66, Dz=23 K=96 0.51 -> 0.66, Dz=26 K=80 0.49 -> 0.66, Dz=28 K=48 0.47 -> 0.66)
  //   K = 97 .. 128 (seven / eight row blocks, one wave per SIMD): K <= 112 from Dz = 8 (Dz=8 K=112 0.49 -> 0.58, Dz=12 0.53 -> 0.62, Dz=20 0.58 -> 0.65);
  //                 K = 113 .. 128 at Dz = 10 .. 15 (Dz=10 0.43 -> 0.51, Dz=14 0.54 -> 0.64; Dz <= 8: the tile kernels, 0.56 against 0.40; Dz >= 16:
  //                 the wide two-stage kernels are level or ahead, Dz=18 0.74 against 0.70)
  if (K >= 113) return D >= 10 && D <= 15;
  if (K >= 97) return D >= 8;
  if (K >= 65) return D >= 6;
  if (K >= 49) return D >= 18;
  if (K >= 33) return D >= 9;
  if (K >= 17) return D >= 13;
  if (K >= 13) return D >= 12;
  if (K <= 4) return !use_narrow(s, K, false, plain, true, t);        // (one slot of the narrow kernels: Dz=28 K=4 0.30 against 0.17 on 16-padded tiles)
  return D >= 24 || !use_narrow(s, K, false, plain, true, t);
}

// Label pass of the mid shapes (mimo_mid.hip, label mode + the label-statistics kernels): K <= 48 at Dz >= 10, plain requests, where it
// measured ahead of the row-owner label kernels (profiles/r04_mid_label_sweep.txt); "mid_labels_min_d" (mimo_tune) moves the lower end
inline bool use_mid_labels(const RouteShape& s, int K, bool wants_tables, const RouteTunables& t) {
  if (wants_tables || !mid_labels_covers(K, s.D, s.structure) || !label_stats_covers(K, s.D, s.structure)) return false;
  if (t.mid_labels_min_d > 0) return s.D >= t.mid_labels_min_d;
  // measured (tools/mid_label_sweep.py, N = 2e6, fraction of the float64 rate of the whole sweep, row-owner label kernels -> mid label mode):
  //   K <= 16 from Dz = 17 (the streamed kernel pads to 32 components: Dz=17 K=16 0.23 -> 0.34, Dz=24 0.28 -> 0.45, Dz=32 0.29 -> 0.47; Dz=28 K=8 0.15 -> 0.26)
  //   K = 33 .. 48 from Dz = 14 (Dz=14 0.45 -> 0.49, Dz=20 0.46 -> 0.55, Dz=28 0.48 -> 0.64); K = 17 .. 32 from Dz = 20 (0.48 -> 0.51, Dz=32 0.56 -> 0.58)
  //   below: the row-owner kernels with Theta resident in LDS stay ahead (Dz=16 K=32 0.51 against 0.41)
  const int D = s.D;
  return K >= 33 ? D >= 14 : K >= 17 ? D >= 20 : D >= 17;
}

inline bool mid_labels_before_narrow(const RouteShape& s, int K, const RouteTunables& t) {
  if (t.mid_labels_narrow_k > 0) return K >= t.mid_labels_narrow_k;
  // measured (profiles/r04_mid_label_sweep.txt, second block): the narrow label kernels stay ahead up to Dz = 20 (Dz=16 K=16 0.34 against 0.33,
  // K=8 0.23 against 0.17); from Dz = 24 their one-wave-per-SIMD variants fall behind for K = 5 .. 8 (Dz=24 K=8 1.11 -> 0.67 ms, Dz=26 1.29 -> 0.74)
  return K >= 5 && s.D >= 24;
}

// Which bound-only requests run as the plain pass.  MIMO_BOUND_PROMOTE = 0: none, 2: every shape of the narrow / mid kernels.
inline bool bound_promote(const RouteShape& s, int K, const RouteTunables& t) {
  if (t.bound_promote == 0) return false;
  const bool md = use_mid(s, K, true, t);
  const bool nv = !md && use_narrow(s, K, false, true, true, t) != 0;
  if (t.bound_promote == 2) return md || nv;
  return (md && K <= t.bound_promote_mid_k) || nv;
}

inline Route choose_route(const RouteShape& s, int K, const RouteRequest& q, const RouteTunables& t) {
  Route r;
  auto is = [&r](Family f, Image im = Image::Generic) { r.family = f; r.image = im; return r; };
  const bool small = use_small(s, K, t);
  const bool fused = fused_covers((K + 15) / 16, s.F16 / 16, q.src);
  if (q.src != kSrcEstep) {             // statistics of a caller's table / labels: no Theta
    if (small) return is(Family::Small);
    if (q.src == kSrcLabels && label_stats_covers(K, s.D, s.structure)) return is(Family::LabelStats);
  } else if (q.gibbs) {
    const int nw = use_narrow(s, K, true, !q.tables, q.stats, t);
    if (!small && use_mid_labels(s, K, q.tables, t) && (!nw || mid_labels_before_narrow(s, K, t))) return is(Family::MidLabels, Image::MidLabels);
    if (nw) { r.narrow_mode = nw; return is(Family::Narrow, Image::Narrow); }
    if (small) return is(Family::Small, Image::Small);
    if (use_rowwave(s, K, q.tables, t)) return is(Family::Rowwave, Image::RowOwner);
  } else {
    // A bound-only request (no statistics, no tables: the full-data pass of every SVI outer iteration, gmm.py:319-326 / ilr.py:270-277
    // of the reference) used to take the generic tile kernels whatever the shape; where the plain pass runs on the narrow or mid kernels
    // those pay for 16 x 16 padding the plain pass does not have, and the plain pass with its statistics left in the partial blocks is
    // the faster bound (bound_promote(): measured rule).
    r.promoted = !q.stats && !q.tables && !q.device_out && bound_promote(s, K, t);
    const bool plain = (q.stats || r.promoted) && !q.tables;
    if (use_mid(s, K, plain, t)) return is(Family::Mid, Image::Mid);                 // mid shapes (K <= 32 over wide rows): mimo_mid.hip
    // narrow shapes (Dz <= 4, 32 < K <= 128; few components over many features): mimo_narrow.hip
    if ((r.narrow_mode = use_narrow(s, K, false, plain, true, t))) return is(Family::Narrow, Image::Narrow);
    if (small) return is(Family::Small, Image::Small);
    // plain softmax + statistics pass at K <= 64, Dz <= 9: the row-owner kernel (Theta in the row-owner image); a caller's row weights stay with the tile kernels
    if (plain && !q.weighted && s.n_bad == 0 && s.D <= 16 && vi_rowwave_covers(K, s.F16, route_zs(K, s.D))) return is(Family::RowwaveVi, Image::RowOwner);
  }
  return is(fused ? Family::Fused : Family::TwoStage);
}

// What a two-stage pass launches: the E-step in front (none for the statistics of a caller's table / labels) and the statistics
// behind it.  Decided here alone: launch_two_stage runs it, route_grid sizes the grid from it, plan_route prints it
// (a route of another family: the empty plan).
struct TwoStagePlan {
  enum Estep { NoEstep, Chunked, Wide } estep = NoEstep;      // estep_chunked_kernel | the pipelined wide_estep_kernel (mimo_wide.hip)
  enum Stats { NoStats, LabelStats, WideColumns, FusedColumns } stats = NoStats;   // label statistics | per column group: 8-wave wide_stats_kernel, fused_kernel
  int stats_src = kSrcWeights;                                // what the statistics read: the (K, N) table or the labels
  int gmax = 0, groups = 0;                                   // (per column group) feature column blocks per statistics launch; launches
};
inline TwoStagePlan two_stage_plan(const Route& route, const KernelArgs& a, int structure, int src) {
  TwoStagePlan p;
  if (route.family != Family::TwoStage) return p;
  if (src == kSrcEstep) p.estep = wide_estep_covers(a.K16, a.D, a.F16, a.gibbs) ? TwoStagePlan::Wide : TwoStagePlan::Chunked;
  p.stats_src = src != kSrcEstep ? src : a.gibbs ? kSrcLabels : kSrcWeights;
  if (!a.do_stats) return p;
  // label-indexed statistics of the labels just drawn: the HBM-bound pass instead of one-hot products per column group
  if (p.stats_src == kSrcLabels && label_stats_covers(a.K, a.D, structure)) { p.stats = TwoStagePlan::LabelStats; return p; }
  p.stats = p.stats_src == kSrcWeights && wide_stats_covers(a.K16, a.D) ? TwoStagePlan::WideColumns : TwoStagePlan::FusedColumns;
  p.gmax = p.stats == TwoStagePlan::WideColumns ? wide_stats_group_ncb(a.K16, a.F16 / 16) : stats_group_ncb(a.K16);
  p.groups = (a.F16 / 16 + p.gmax - 1) / p.gmax;
  return p;
}

}  // namespace mimo
