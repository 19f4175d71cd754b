// Batched softmax pass (gfx950): B independent problems that share Dz and K, each with its own rows and its own (c, b, W),
// in ONE launch.  The rows of all problems are concatenated into one (N_total, Dz) matrix; problem b owns the rows
// [row_off[b], row_off[b + 1]).  A host-built work table gives every workgroup a run of 32-row tiles of ONE problem; how a
// problem's tiles are split depends on its row count alone (batched_tiles_per_wg), so a problem's partial blocks — and,
// through the fixed-order second stage, its results — are bit-identical whatever else is in the batch.
//
// Per tile, on the matrix instruction of the fused tile kernel (v_mfma_f64_16x16x4_f64):
//   1. z~ tile of the problem's rows into LDS (rows past the problem's end are zero, with a zero in the constant slot:
//      their features, weights, statistics and lse terms are all zero)
//   2. feature tile Phi (32 x F16) from the feature table
//   3. L = Theta_b Phi': wave w owns the component row blocks w, w + 4; Theta_b's MFMA A-operand slices come from the
//      problem's slice of the stacked operand image (the single-problem image, one per problem)
//   4. softmax over k (normalise_tile / normalise_tile_chunked of mimo_tile.h, generic mode: sum lse and sum r l per row)
//   5. S += R Phi: the K16 x NCB 16 x 16 output blocks are dealt to the four waves in row-block-major runs (at most 10 per
//      wave: the K16 NCB <= 40 coverage bound is this register budget)
// and one partial block per workgroup at the end.  batched_reduce_kernel sums each problem's blocks in a fixed order and
// unpacks them into the packed per-problem statistics and scalars.
//
// Label modes (LM, the batched Gibbs sweep), on the same work table and the same reduction:
//   kBatchedDraw:  phases 1-3 as above; phase 4 is the inverse-CDF draw of the normalise helpers (gibbs = true) with the
//                  problem's own uniforms (u + row_off[b]) or its own Philox key (seeds[b], counter (local row, sweep)), so a
//                  problem's labels are those of a solo draw over its rows alone; phase 5 is S += one-hot(labels) Phi, its
//                  A operand built from the LDS label array (exact integer counts).
//   kBatchedGiven: labels read from the device (the initial labels of a chain): no L product, no draw, phase 5 as above.
// No scalars are returned in the label modes (their partial blocks carry zeros there).
//
// Table mode (LM = kBatchedWeights, the statistics of a weight table: the drivers' random start, caller-supplied weights),
// on the same work table, the same LDS plan and the same reduction: phases 1-2 as above; then the weight tile
// Lt[row][k] is filled from the problem's slice of a device table (a.resp: the problems' K-major (K, N_b) tables back to
// back, problem b's at element K row_off[b]; exactly 0.0 for rows past the problem's end and for padding components);
// no L product, no normalise phase; phase 5 is the softmax mode's, its A operand read from Lt.  Zero scalars.
// batched_random_resp_kernel writes such a table for the whole batch in one launch (random_resp_column of mimo_device.h).
//
// Row-selection mode (LM = kBatchedSoftmaxRows, the minibatch pass of batched SVI): the softmax mode over a.sel, a list of
// local row indices per problem (problem b's are sel[sel_off[b] .. sel_off[b + 1]), any order, duplicates allowed).  Phase 1
// gathers the z~ tile through the list: tile row r of local tile t is row sel[sel_off[b] + 32 t + r] of the problem; the
// problem's "row count" is its selection's length, and a.work is a table built for those lengths.  Every phase after the tile
// store is the softmax mode's, so the result is that of a plain pass over the gathered rows, bit for bit.  The indices are
// read one tile ahead of the rows they address (three tiles ahead of their use), so the dependent load is never waited for.
//
// Weighted softmax mode (LM = kBatchedSoftmaxWeighted, the inner passes of a mixture of mixtures): the softmax mode with
// ka.u = a.u + row_off[b], the problem's per-row weights: the generic normalise mode writes r_kn w_n back into Lt, so the
// statistics are those of r_kn w_n while the scalars and lse stay those of r_kn (mimo/mixtures/hgmm.py:199-207).  A weight of
// exactly 1.0 leaves every bit of the softmax mode's tile.
//
// Shared batch (a.shared, every mode): the B problems read ONE (N, D) block, Zb = a.Z for all of them; row_off[b] = b N still
// places problem b in every per-problem buffer.  The work table is that of B problems of N rows, so each problem's partial
// blocks are those of a ragged batch of B copies of the block, bit for bit.  outer_resp_kernel (below) is the outer step over
// such a batch's lse.
#include "mimo_batched.h"
#include "mimo_tile.h"

#include <math.h>

namespace mimo {

int batched_tiles_per_wg(int64_t nrows) {
  const int64_t tiles = (nrows + kTile - 1) / kTile;
  const int64_t t = (tiles + 127) / 128;      // at most 128 workgroups per problem: bounds the partial blocks of large problems
  return (int)(t > 4 ? t : 4);
}

static int batched_ncb(int D) { return (feat_count(D) + 15) / 16; }

bool batched_covers(int K, int D) {
  if (D < 1 || D > kBatchedMaxD || K < 1 || K > kBatchedMaxK) return false;
  return ((K + 15) / 16) * batched_ncb(D) <= kBatchedMaxPairs;
}

size_t batched_lds_bytes(const BatchedArgs& a) {
  const int ncb = a.F16 / 16, rbw = a.K16 <= 4 ? 1 : 2;
  return sizeof(double) * ((size_t)kTile * (a.ZS + batched_rs(ncb) + batched_ls(ncb, rbw)) + 16 + 64) + (size_t)a.F16 * 2;
}

// NCB: 16-wide feature column blocks; RBW: component row blocks per wave (1: K <= 64, 2: K <= 128); LM: BatchedLabelMode
template <int NCB, int RBW, int LM = kBatchedSoftmax>
__global__ __launch_bounds__(kWG, 1) void batched_kernel(const BatchedArgs a) {
  constexpr int T = kTile;
  constexpr int NSI = 4 * NCB;                                       // contraction steps of the L product (4 features each)
  constexpr int K16MAX = (RBW == 1 ? 4 : 8) < kBatchedMaxPairs / NCB ? (RBW == 1 ? 4 : 8) : kBatchedMaxPairs / NCB;
  constexpr int SP = (K16MAX * NCB + 3) / 4;                         // statistics blocks per wave at most (<= 10)
  // compile-time row strides: every LDS operand of the two products is a base register + an immediate offset
  constexpr int RS = batched_rs(NCB), LS = batched_ls(NCB, RBW);

  extern __shared__ __align__(16) unsigned char smem[];
  double* Zs = reinterpret_cast<double*>(smem);   // [T][ZS]  z~ rows (z, 1, 0)
  double* Ph = Zs + T * a.ZS;                     // [T][RS]  feature tile
  double* Lt = Ph + T * RS;                       // [T][LS]  l -> r per (row, component)
  double* red = Lt + T * LS;                      // [16]     scalar reduction scratch
  double* etab = red + 16;                        // [64]     2^(j/64) for exp_nonpos
  uint8_t* fe = reinterpret_cast<uint8_t*>(etab + 64);   // [F16][2]
  int* labs = reinterpret_cast<int*>(red);        // [T] labels of the tile (label modes; unused by the softmax and the table mode)
  constexpr bool ROWS = LM == kBatchedSoftmaxRows;                           // the softmax mode over a row selection
  constexpr bool WEIGHTED = LM == kBatchedSoftmaxWeighted;                   // the softmax mode with per-row weights on the statistics
  constexpr bool SOFTMAX = LM == kBatchedSoftmax || ROWS || WEIGHTED;
  constexpr bool HAS_L = SOFTMAX || LM == kBatchedDraw;                      // L product + normalise phase
  constexpr bool A_FROM_LT = SOFTMAX || LM == kBatchedWeights;               // phase 5 reads its A operand from Lt

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int D = a.D, K = a.K, K16 = a.K16, F16 = a.F16;
  const int ZS = a.ZS;
  const int Kpad = 16 * K16;

  const BatchedWork wk = a.work[blockIdx.x];
  const int prob = __builtin_amdgcn_readfirstlane(wk.prob);
  const int tile0 = __builtin_amdgcn_readfirstlane(wk.tile0), ntl = __builtin_amdgcn_readfirstlane(wk.ntiles);
  const int64_t rbeg = a.row_off[prob];
  int64_t nrows = a.row_off[prob + 1] - rbeg;
  const int64_t* selb = nullptr;            // selection mode: the problem's index list; its length is the pass's row count
  if constexpr (ROWS) {
    selb = a.sel + a.sel_off[prob];
    nrows = a.sel_off[prob + 1] - a.sel_off[prob];
  }
  const int64_t Nb = nrows;
  const double* Zb = a.Z + (a.shared ? 0 : rbeg) * D;   // a shared batch: every problem reads the one block (scalar select)
  double* const out_lse = !ROWS && a.lse ? a.lse + rbeg : nullptr;    // (a selection's normalisers have no place in lse)
  const gptr_t th = (gptr_t)(a.theta + (size_t)prob * K16 * NSI * 64);

  for (int e = tid; e < F16 * 2; e += kWG) fe[e] = a.feat[e];
  if (tid < 64) etab[tid] = exp2((double)tid * (1.0 / 64.0));

  // the normalise helpers read the row weights / uniforms / labels of a KernelArgs: none for the softmax (unit weights);
  // the draw reads the problem's slices of the uniforms and labels, or its Philox key, with local rows (row0 = 0)
  KernelArgs ka;
  ka.u = nullptr;
  ka.relabel = nullptr;
  ka.labels = nullptr;
  ka.seed = 0; ka.sweep = 0; ka.row0 = 0;
  if constexpr (LM == kBatchedDraw) {
    ka.u = a.u ? a.u + rbeg : nullptr;
    ka.labels = a.labels + rbeg;
    ka.seed = a.u ? 0 : a.seeds[prob];
    ka.sweep = a.sweep;
    ka.relabel = a.relabel ? a.relabel + (size_t)prob * K : nullptr;
  }
  if constexpr (WEIGHTED) ka.u = a.u + rbeg;   // the generic normalise mode scales the weights it writes back by u[local row]

  // Z tile staging: thread element e = tid + 256 i (T * D <= 512) of the tile; the next tile is read into registers
  // while the current one is processed
  int zoff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + kWG * i;
    const int pt = e / D;
    zoff[i] = e < T * D ? pt * ZS + (e - pt * D) : -1;
  }
  double zr[2];
  // selection mode: element i of this thread lies in tile row zrow[i] and column zcol[i] of every tile, so a tile costs it
  // two index loads; zi[i] is the element offset (index * D + column) of the NEXT load_z's row, -1 past the selection's end.
  // load_z(t) reads the rows through the offsets fetched by load_z(t - 1) and fetches those of tile t + 1 (the calls come
  // in tile order), so no load waits for the index it depends on.
  int zrow[2], zcol[2];
  int64_t zi[2];
  auto load_idx = [&](int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t n = (int64_t)t * T + zrow[i];
      zi[i] = (zoff[i] >= 0 && n < Nb) ? selb[n] * D + zcol[i] : -1;
    }
  };
  if constexpr (ROWS) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + kWG * i;
      zrow[i] = e / D;
      zcol[i] = e - zrow[i] * D;
    }
    load_idx(tile0);
  }
  auto load_z = [&](int t) {
    if constexpr (ROWS) {
#pragma unroll
      for (int i = 0; i < 2; ++i) zr[i] = zi[i] >= 0 ? Zb[zi[i]] : 0.0;
      load_idx(t + 1);
      return;
    }
    const int64_t base = (int64_t)t * T * D, total = Nb * D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t g = base + tid + kWG * i;
      zr[i] = (zoff[i] >= 0 && g < total) ? Zb[g] : 0.0;
    }
  };
  auto store_z = [&](int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (zoff[i] >= 0) Zs[zoff[i]] = zr[i];
    if (tid < T) {
      Zs[tid * ZS + D] = ((int64_t)t * T + tid) < Nb ? 1.0 : 0.0;   // rows past the problem's end contribute nothing
      Zs[tid * ZS + D + 1] = 0.0;                                   // padded features read this slot
    }
  };
  load_z(tile0);
  store_z(tile0);
  load_z(tile0 + 1);

  // Weight tile staging (table mode): thread (row wrow, component group wgrp) holds the components wgrp + 8 i of its row: a
  // wave reads 32 consecutive doubles of each of two components per step.  Like the z~ rows, the next tile's weights are
  // read into registers before the current tile's statistics MFMAs are issued.
  constexpr int NW = LM == kBatchedWeights ? 2 * K16MAX : 1;
  const int wrow = tid & (T - 1), wgrp = tid >> 5;
  double wr[NW];
  auto load_w = [&](int t) {
    const int64_t n = (int64_t)t * T + wrow;
    const double* tb = a.resp + (int64_t)K * rbeg + n;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int k = wgrp + 8 * i;
      wr[i] = (n < Nb && k < K) ? tb[(int64_t)k * Nb] : 0.0;
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int k = wgrp + 8 * i;
      if (k < Kpad) Lt[wrow * LS + k] = wr[i];
    }
  };
  if constexpr (LM == kBatchedWeights) load_w(tile0);

  const int frow = tid & (T - 1), fgrp = tid >> 5;
  wg_sync();   // feature and exp tables are in LDS
  uint32_t w[NCB];
#pragma unroll
  for (int jj = 0; jj < NCB; ++jj) w[jj] = reinterpret_cast<const uint32_t*>(fe)[fgrp * NCB + jj];

  // statistics blocks of this wave: pairs p = wave P + i (row block p / NCB, column block p % NCB), i < npw
  const int npair = K16 * NCB, P = (npair + 3) / 4;
  const int npw = __builtin_amdgcn_readfirstlane(min(max(npair - wave * P, 0), P));
  // per block: the base of its A operands (row 8 q, component 16 rb + j) and B operands (row 8 q, feature 16 cb + j)
  // (label modes: lk = the component of the A operand's lane, 16 rb + j, that the one-hot entry tests for)
  int lo[SP], po[SP], lk[SP];
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    const int p = i < npw ? wave * P + i : 0;
    const int rb = p / NCB, cb = p - rb * NCB;
    lo[i] = 8 * q * LS + 16 * rb + j;
    po[i] = 8 * q * RS + 16 * cb + j;
    lk[i] = 16 * rb + j;
  }
  d4 sacc[SP];
#pragma unroll
  for (int i = 0; i < SP; ++i) sacc[i] = d4{0.0, 0.0, 0.0, 0.0};

  double sc_lse = 0.0, sc_rl = 0.0, sc_prod = 1.0;
  PhiloxBatch pbatch;

  for (int t = tile0; t < tile0 + ntl; ++t) {
    const int64_t n0 = (int64_t)t * T;
    wg_sync();   // z~ tile of this step is in LDS; the previous tile's readers are done

    // ---- feature tile: thread (row frow, group fgrp) writes features [2 NCB fgrp, 2 NCB (fgrp + 1)) ----
    {
      const double* zrow = Zs + frow * ZS;
      double* prow = Ph + frow * RS + fgrp * (2 * NCB);
#pragma unroll
      for (int jj = 0; jj < NCB; ++jj) {
        uint32_t wj = w[jj];
        asm volatile("" : "+v"(wj));
        const double za0 = zrow[wj & 255u], zb0 = zrow[(wj >> 8) & 255u];
        const double za1 = zrow[(wj >> 16) & 255u], zb1 = zrow[wj >> 24];
        prow[2 * jj] = za0 * zb0;
        prow[2 * jj + 1] = za1 * zb1;
      }
    }
    if constexpr (LM == kBatchedGiven) {   // rows past the problem's end get no label: their one-hot row is zero
      if (tid < T) labs[tid] = (n0 + tid) < Nb ? a.labels[rbeg + n0 + tid] : -1;
    }
    if constexpr (LM == kBatchedWeights) store_w();   // (Lt was last read before the barrier at the top of this step)
    wg_sync();
    if constexpr (LM == kBatchedWeights) {
      if (t + 1 < tile0 + ntl) load_w(t + 1);
    }

    if constexpr (HAS_L) {
    // ---- L tile = Theta_b Phi': row block rb = wave + 4 h, both 16-row column groups -------------------
    // A lane (i = j, kk = q) = Theta[16 rb + j][4 s + q]; B lane (kk = q, col = j) = Phi[16 g + j][4 s + q];
    // C/D: reg r of lane (q, j) = component 16 rb + q + 4 r, row 16 g + j
#pragma unroll
    for (int h = 0; h < RBW; ++h) {
      const int rb = wave + 4 * h;
      if (rb < K16) {
        // Theta slices stream from L2 through an 8-deep register ring, B operands are read two steps ahead of their
        // MFMAs; sched_barriers keep hipcc from hoisting every read of the unrolled loop (register pressure)
        constexpr int PD = NSI < 8 ? NSI : 8;
        gptr_t thb = th + (size_t)rb * NSI * 64;
        asm volatile("" : "+s"(thb));   // opaque per tile: slice addresses = scalar base + immediates, not hoisted VGPR pairs
        const gptr_t thr = thb + lane;
        double tr[PD], bq0[3], bq1[3];
#pragma unroll
        for (int e = 0; e < PD; ++e) tr[e] = thr[e * 64];
        const double* p0 = Ph + j * RS + q;
        const double* p1 = Ph + (16 + j) * RS + q;
        bq0[0] = p0[0]; bq1[0] = p1[0];
        if (NSI > 1) { bq0[1] = p0[4]; bq1[1] = p1[4]; }
        d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < NSI; ++s) {
          if (s + 2 < NSI) { bq0[(s + 2) % 3] = p0[4 * (s + 2)]; bq1[(s + 2) % 3] = p1[4 * (s + 2)]; }
          __builtin_amdgcn_sched_barrier(0);
          const double av = tr[s % PD];
          if (s + PD < NSI) tr[s % PD] = thr[(s + PD) * 64];
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bq0[s % 3], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bq1[s % 3], acc1, 0, 0, 0);
        }
        double* lw0 = Lt + j * LS + 16 * rb + q;
        double* lw1 = lw0 + 16 * LS;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lw0[4 * r] = acc0[r];
          lw1[4 * r] = acc1[r];
        }
      }
    }
    wg_sync();

    // ---- softmax over k (8 lanes per row); rows past the problem's end get zero weights and no lse -------------
    // draw: the label of each row into labs (-1 past the problem's end) and the problem's label slice; the Philox batch
    // walks this workgroup's consecutive tiles (stride T rows)
    constexpr bool DRAW = LM == kBatchedDraw;
    constexpr int NM = DRAW ? kFastGibbs : kGeneric;
    if constexpr (RBW == 1)
      normalise_tile<1, NM>(ka, Lt, LS, etab, K, K16, Nb, n0, wave, lane, DRAW, nullptr, nullptr, DRAW ? nullptr : out_lse,
                            sc_lse, sc_rl, sc_prod, labs, pbatch, DRAW ? T : 0);
    else
      normalise_tile_chunked<RBW, NM>(ka, Lt, LS, etab, K, K16, Nb, n0, wave, lane, DRAW, nullptr, nullptr,
                                      DRAW ? nullptr : out_lse, sc_lse, sc_rl, sc_prod, labs, pbatch, DRAW ? T : 0);
    wg_sync();
    }

    // ---- S += R Phi: step s contracts rows {s, s + 8, s + 16, s + 24}; A lane (i = j, kk = q) = R[8 q + s][16 rb + j],
    // B lane (kk = q, col = j) = Phi[8 q + s][16 cb + j]; label modes: R = one-hot(labels), R[n][k] = labs[n] == k ----
    if (a.do_stats) {
      // operands of step s + 1 are read before the MFMAs of step s are issued
      // opaque offsets per tile (not pointers: those would lose the LDS address space): every read below is
      // one of these registers + an immediate, instead of 16 SP loop-invariant addresses pinned in (and spilled from) VGPRs
      int lot[SP], pot[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        lot[i] = lo[i];
        pot[i] = po[i];
        asm volatile("" : "+v"(lot[i]), "+v"(pot[i]));
      }
      double avq[2][SP], bvq[2][SP];
      auto fetch = [&](int s, int slot) {
        int lab = -1;
        if constexpr (!A_FROM_LT) lab = labs[8 * q + s];
#pragma unroll
        for (int i = 0; i < SP; ++i) {
          if (i < npw) {
            if constexpr (A_FROM_LT) avq[slot][i] = Lt[lot[i] + s * LS];
            else avq[slot][i] = lab == lk[i] ? 1.0 : 0.0;
            bvq[slot][i] = Ph[pot[i] + s * RS];
          }
        }
      };
      fetch(0, 0);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (s + 1 < 8) fetch(s + 1, (s + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < SP; ++i)
          if (i < npw) sacc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(avq[s & 1][i], bvq[s & 1][i], sacc[i], 0, 0, 0);
      }
    }

    // ---- stage the next tile's z~ rows (Zs was last read before the barrier after the feature build) ----------
    if (t + 1 < tile0 + ntl) {
      store_z(t + 1);
      load_z(t + 2);
    }
  }

  // ---- partial block of this workgroup ---------------------------------------------------------------------
  const size_t pstride = (size_t)Kpad * F16 + 4;
  double* Pb = a.partials + (size_t)blockIdx.x * pstride;
  if (a.do_stats) {
#pragma unroll
    for (int i = 0; i < SP; ++i) {
      if (i < npw) {
        const int p = wave * P + i;
        const int rb = p / NCB, cb = p - rb * NCB;
#pragma unroll
        for (int r = 0; r < 4; ++r) Pb[(size_t)(16 * rb + q + 4 * r) * F16 + 16 * cb + j] = sacc[i][r];
      }
    }
  }
  if constexpr (!SOFTMAX) {
    // no scalars in the label and table modes (and red, which holds the labels, is left alone)
    if (tid < 4) Pb[(size_t)Kpad * F16 + tid] = 0.0;
    return;
  }
  sc_lse = wave_sum(sc_lse);
  sc_rl = wave_sum(sc_rl);
  wg_sync();
  if (lane == 0) { red[2 * wave] = sc_lse; red[2 * wave + 1] = sc_rl; }
  wg_sync();
  if (tid == 0) {
    double* Ps = Pb + (size_t)Kpad * F16;
    Ps[0] = (red[0] + red[2]) + (red[4] + red[6]);
    Ps[1] = (red[1] + red[3]) + (red[5] + red[7]);
    Ps[2] = 0.0;
    Ps[3] = 0.0;
  }
}

// One thread per (component, feature) entry of a problem (blockIdx.y), plus one for the two scalar sums: the problem's
// partial blocks in ascending order, four interleaved chains combined in a fixed order.
__global__ __launch_bounds__(256) void batched_reduce_kernel(const double* __restrict__ partials, const int32_t* __restrict__ wg_off,
                                                              const uint8_t* __restrict__ feat, int K, int D, int F, int F16, int split,
                                                              double* __restrict__ S, double* __restrict__ scalars) {
  const int b = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Kpad = (K + 15) / 16 * 16;
  const int64_t pstride = (int64_t)Kpad * F16 + 4, nsx = (int64_t)K * F;
  const int g0 = wg_off[b], g1 = wg_off[b + 1];
  auto sum = [&](int64_t off) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int g = g0;
    for (; g + 3 < g1; g += 4) {
      s0 += partials[(int64_t)g * pstride + off];
      s1 += partials[(int64_t)(g + 1) * pstride + off];
      s2 += partials[(int64_t)(g + 2) * pstride + off];
      s3 += partials[(int64_t)(g + 3) * pstride + off];
    }
    for (; g < g1; ++g) s0 += partials[(int64_t)g * pstride + off];
    return (s0 + s1) + (s2 + s3);
  };
  if (S && e < nsx) {
    const int k = (int)(e / F), f = (int)(e - (int64_t)k * F);
    const int aa = feat[2 * f], bb = feat[2 * f + 1];
    const double v = sum((int64_t)k * F16 + f);
    double* Sk = S + ((int64_t)b * K + k) * (1 + D + D * D);
    if (aa == D) Sk[0] = v;                // (D, D): n_k
    else if (bb == D) Sk[1 + aa] = v;      // (a, D): sum r z_a
    else { Sk[1 + D + aa * D + bb] = v; Sk[1 + D + bb * D + aa] = v; }
  }
  if (e == nsx) {
    const double slse = sum((int64_t)Kpad * F16), srl = sum((int64_t)Kpad * F16 + 1);
    // (integer selects: built with -fno-honor-nans, see unpack_stats)
    const long long nan_bits = 0x7ff8000000000000LL;
    scalars[3 * b] = slse;
    scalars[3 * b + 1] = __longlong_as_double(split ? __double_as_longlong(srl) : nan_bits);
    scalars[3 * b + 2] = __longlong_as_double(split ? __double_as_longlong(slse - srl) : nan_bits);
  }
}

typedef void (*batched_fn)(const BatchedArgs);

template <int RBW, int LM>
static batched_fn pick_batched(int ncb) {
  switch (ncb) {
    case 1: return batched_kernel<1, RBW, LM>;
    case 2: return batched_kernel<2, RBW, LM>;
    case 3: return batched_kernel<3, RBW, LM>;
    case 4: return batched_kernel<4, RBW, LM>;
    case 5: return batched_kernel<5, RBW, LM>;
    case 6: return batched_kernel<6, RBW, LM>;
    case 7: return batched_kernel<7, RBW, LM>;
    case 8: return batched_kernel<8, RBW, LM>;
    default: break;
  }
  if constexpr (RBW == 1) {
    if (ncb == 9) return batched_kernel<9, 1, LM>;
    if (ncb == 10) return batched_kernel<10, 1, LM>;
  }
  return nullptr;
}

template <int LM>
static hipError_t launch_mode(const BatchedArgs& a, int grid, hipStream_t stream) {
  if (!batched_covers(a.K, a.D)) return hipErrorInvalidValue;
  const int ncb = a.F16 / 16;
  batched_fn fn = a.K16 <= 4 ? pick_batched<1, LM>(ncb) : pick_batched<2, LM>(ncb);
  if (!fn) return hipErrorInvalidValue;
  if (grid <= 0) return hipSuccess;
  const size_t lds = batched_lds_bytes(a);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kWG), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_batched(const BatchedArgs& a, int grid, hipStream_t stream) {
  return launch_mode<kBatchedSoftmax>(a, grid, stream);
}

hipError_t launch_batched_labels(const BatchedArgs& a, int mode, int grid, hipStream_t stream) {
  if (mode == kBatchedDraw) {
    if (!a.labels || (!a.u && !a.seeds)) return hipErrorInvalidValue;
    return launch_mode<kBatchedDraw>(a, grid, stream);
  }
  if (mode == kBatchedGiven) {
    if (!a.labels) return hipErrorInvalidValue;
    return launch_mode<kBatchedGiven>(a, grid, stream);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_batched_rows(const BatchedArgs& a, int grid, hipStream_t stream) {
  if (!a.sel || !a.sel_off) return hipErrorInvalidValue;
  return launch_mode<kBatchedSoftmaxRows>(a, grid, stream);
}

hipError_t launch_batched_weights(const BatchedArgs& a, int grid, hipStream_t stream) {
  if (!a.resp) return hipErrorInvalidValue;
  return launch_mode<kBatchedWeights>(a, grid, stream);
}

hipError_t launch_batched_weighted(const BatchedArgs& a, int grid, hipStream_t stream) {
  if (!a.u) return hipErrorInvalidValue;
  return launch_mode<kBatchedSoftmaxWeighted>(a, grid, stream);
}

// ---- outer step of a mixture of mixtures over a shared batch -----------------------------------------------------------
// One row per lane, 256 rows per workgroup (blockIdx.x = the row block: the split depends on N alone).  Three sweeps over b, each
// reading lse[b N + n] coalesced across the wave: the maximum, the sum of exponentials, the weights.  log_gating is staged in LDS
// in chunks of kOuterChunk entries, so B is bounded by nothing here; the third sweep also sums every weight over the workgroup's
// rows: a wave butterfly per b, the four wave sums through LDS, added in wave order.  The exponentials of the second sweep are
// recomputed in the third (same inputs, same bits), so nothing per b is held in registers.
constexpr int kOuterChunk = 256;

__global__ __launch_bounds__(kWG) void outer_resp_kernel(const double* __restrict__ lse, const double* __restrict__ log_gating, int B,
                                                         int64_t N, double* __restrict__ w, double* __restrict__ partials) {
  __shared__ double etab[64];
  __shared__ double lg[kOuterChunk];
  __shared__ double red[kOuterChunk][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = (int64_t)blockIdx.x * kWG + tid;
  const bool valid = n < N;
  const double* col = lse + (valid ? n : 0);      // rows past the end read row 0 and contribute nothing
  double* Pb = partials + (size_t)blockIdx.x * ((size_t)B + 1);
  if (tid < 64) etab[tid] = exp2((double)tid * (1.0 / 64.0));

  // every sweep walks the chunks of log_gating through LDS: f(b, lse[b N + n] + log_gating[b], log_gating[b] == -inf)
  auto sweep = [&](auto&& f, auto&& chunk_done) {
    for (int c0 = 0; c0 < B; c0 += kOuterChunk) {
      const int len = min(kOuterChunk, B - c0);
      wg_sync();                                  // the previous chunk's readers are done (first chunk: etab is in LDS)
      if (tid < len) lg[tid] = log_gating[c0 + tid];
      wg_sync();
      for (int i = 0; i < len; ++i) {
        const double g = lg[i];
        f(c0, i, col[(int64_t)(c0 + i) * N] + g, g == -INFINITY);
      }
      chunk_done(c0, len);
    }
  };
  auto nothing = [](int, int) {};

  double m = -INFINITY;
  sweep([&](int, int, double t, bool off) { m = off ? m : fmax(m, t); }, nothing);     // (one entry at least is finite: checked by the host)
  double s = 0.0;
  sweep([&](int, int, double t, bool off) { s += off ? 0.0 : exp_nonpos(t - m, etab); }, nothing);
  sweep([&](int c0, int i, double t, bool off) {
          const double wv = off ? 0.0 : exp_nonpos(t - m, etab) / s;
          if (valid) w[(int64_t)(c0 + i) * N + n] = wv;
          const double ws = wave_sum(valid ? wv : 0.0);
          if (lane == 0) red[i][wave] = ws;
        },
        [&](int c0, int len) {
          wg_sync();
          if (tid < len) Pb[c0 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        });
  const double ll = wave_sum(valid ? m + log(s) : 0.0);
  wg_sync();
  if (lane == 0) red[0][wave] = ll;
  wg_sync();
  if (tid == 0) Pb[B] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
}

// One thread per output (B counts and the log-likelihood): the row blocks' partial sums in ascending order, four interleaved chains
// combined in a fixed order (as batched_reduce_kernel sums a problem's blocks).
__global__ __launch_bounds__(256) void outer_resp_reduce_kernel(const double* __restrict__ partials, int B, int64_t G, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > B) return;
  const int64_t stride = (int64_t)B + 1;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int64_t g = 0;
  for (; g + 3 < G; g += 4) {
    s0 += partials[g * stride + e];
    s1 += partials[(g + 1) * stride + e];
    s2 += partials[(g + 2) * stride + e];
    s3 += partials[(g + 3) * stride + e];
  }
  for (; g < G; ++g) s0 += partials[g * stride + e];
  out[e] = (s0 + s1) + (s2 + s3);
}

size_t outer_resp_partials(int B, int64_t N) { return (size_t)((N + kWG - 1) / kWG) * ((size_t)B + 1); }

hipError_t launch_outer_resp(const double* lse, const double* log_gating, int B, int64_t N, double* w, double* partials, double* out,
                             hipStream_t stream) {
  if (B < 1 || N < 1 || !lse || !log_gating || !w || !partials || !out) return hipErrorInvalidValue;
  const int64_t G = (N + kWG - 1) / kWG;
  if (G > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(outer_resp_kernel, dim3((unsigned)G), dim3(kWG), 0, stream, lse, log_gating, B, N, w, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(outer_resp_reduce_kernel, dim3((unsigned)(((int64_t)B + 1 + 255) / 256)), dim3(256), 0, stream, partials, B, G, out);
  return hipGetLastError();
}

// One thread per row of the concatenated batch: its problem is the last one that starts at or before it (empty problems own no
// row and are stepped over), its Philox counter the row's index WITHIN the problem.
__global__ __launch_bounds__(kWG) void batched_random_resp_kernel(double* __restrict__ resp, const int64_t* __restrict__ row_off,
                                                                  const uint64_t* __restrict__ seeds, int B, int K, int64_t N_total) {
  const int64_t g = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (g >= N_total) return;
  int lo = 0, hi = B;                       // row_off[lo] <= g < row_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (row_off[mid] <= g) lo = mid; else hi = mid;
  }
  const int64_t rbeg = row_off[lo], Nb = row_off[lo + 1] - rbeg, n = g - rbeg;
  random_resp_column(resp + (int64_t)K * rbeg + n, Nb, K, seeds[lo], (uint64_t)n);
}

hipError_t launch_batched_random_resp(double* resp, const int64_t* row_off, const uint64_t* seeds, int B, int K, int64_t N_total,
                                      hipStream_t stream) {
  if (B <= 0 || N_total <= 0) return hipSuccess;
  hipLaunchKernelGGL(batched_random_resp_kernel, dim3((unsigned)((N_total + kWG - 1) / kWG)), dim3(kWG), 0, stream, resp, row_off,
                     seeds, B, K, N_total);
  return hipGetLastError();
}

hipError_t launch_batched_reduce(const double* partials, const int32_t* wg_off, int B, const uint8_t* feat, int K, int D,
                                 int F, int F16, int split, double* S, double* scalars, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int64_t n = (int64_t)K * F + 1;
  hipLaunchKernelGGL(batched_reduce_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, stream, partials, wg_off,
                     feat, K, D, F, F16, split, S, scalars);
  return hipGetLastError();
}

}  // namespace mimo
