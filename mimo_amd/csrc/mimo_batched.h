// Internal interface of the batched softmax, Gibbs label and table passes (mimo_batched.hip): B independent problems that share Dz and K, each with
// its own rows and its own (c, b, W), in one launch.  Not installed; the public surface is include/mimo_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mimo {

constexpr int kBatchedMaxD = 16;        // single-pass feature tile (F = 153 features at Dz = 16)
constexpr int kBatchedMaxK = 128;       // normalise phase: at most 16 components per lane (8 lanes per row)
constexpr int kBatchedMaxPairs = 40;    // K16 * NCB statistics accumulators (16 x 16 blocks) of one workgroup: 10 per wave

// LDS row strides (doubles) of the feature tile and the weight tile: compile-time constants of each instantiation
__host__ __device__ constexpr int batched_rs(int ncb) { return 16 * ncb + 1; }
__host__ __device__ constexpr int batched_ls(int ncb, int rbw) {
  return 16 * ((rbw == 1 ? 4 : 8) < kBatchedMaxPairs / ncb ? (rbw == 1 ? 4 : 8) : kBatchedMaxPairs / ncb) + 2;
}

// One workgroup's share of the work: `ntiles` consecutive 32-row tiles of problem `prob`, starting at its local tile `tile0`.
struct BatchedWork {
  int32_t prob;
  int32_t tile0;
  int32_t ntiles;
  int32_t pad;
};

struct BatchedArgs {
  const double* Z;            // (N_total, D) row-major, the problems' rows concatenated
  const int64_t* row_off;     // [B + 1]: problem b owns rows [row_off[b], row_off[b + 1])
  const BatchedWork* work;    // [G]
  const double* theta;        // [B][K16][F16 / 4][64]: the single-problem operand image, one per problem
  const uint8_t* feat;        // [F16][2] index pairs (a, b) into z~ = [z, 1, 0]
  double* partials;           // [G][K16 * 16 * F16 + 4]
  double* lse;                // (N_total,) or null
  int D, K, K16, F16;
  int ZS;                     // LDS row stride (doubles) of the z~ tile
  int do_stats;
  int shared;                 // 1: Z holds ONE (N, D) block that every problem reads (mimo_upload_batched_shared); row_off[b] = b N still
                              // places the problem's rows in every per-problem buffer (lse, labels, u, resp, sel)
  // label modes (launch_batched_labels) and the weighted softmax mode (launch_batched_weighted) only; the softmax pass reads none
  // of these
  const double* u;            // (N_total,) uniforms of the draw, or null: Philox keyed by seeds[b], counter (local row, sweep);
                              // weighted softmax mode: the per-row weights of the statistics
  const uint64_t* seeds;      // [B] (Philox draw)
  int32_t* labels;            // (N_total,): the labels drawn (kBatchedDraw) or given (kBatchedGiven)
  uint64_t sweep;
  const int32_t* relabel;     // [B][K] or null: KernelArgs::relabel of every problem (some problem has components switched off by c = -inf)
  // table mode (launch_batched_weights) only
  const double* resp;         // the problems' K-major (K, N_b) weight tables back to back: problem b's starts at element K row_off[b]
  // row-selection mode (launch_batched_rows) only
  const int64_t* sel;         // local row indices in [0, N_b), the problems' selections concatenated (checked by the caller)
  const int64_t* sel_off;     // [B + 1]: problem b's selection is sel[sel_off[b] .. sel_off[b + 1])
};

// Label modes of the batched kernel family: the inverse-CDF draw of a Gibbs sweep (with the statistics of the labels
// drawn), or the statistics of labels given on the device (no L product, no draw).
// Table mode: the statistics of a weight table given on the device (no L product, no normalise phase; weights as they are).
// Row-selection mode: the softmax pass over rows gathered through an index list (the minibatch pass of batched SVI).
// Weighted softmax mode: the softmax pass whose statistics are those of r_kn w_n, w = a.u (scalars and lse: those of r_kn).
enum BatchedLabelMode : int { kBatchedSoftmax = 0, kBatchedDraw = 1, kBatchedGiven = 2, kBatchedWeights = 3, kBatchedSoftmaxRows = 4,
                              kBatchedSoftmaxWeighted = 5 };

// Tiles per workgroup for a problem of `nrows` rows: a function of the row count alone (the determinism rule: a problem's
// result does not depend on what else is in the batch).
int batched_tiles_per_wg(int64_t nrows);
bool batched_covers(int K, int D);
size_t batched_lds_bytes(const BatchedArgs& a);
hipError_t launch_batched(const BatchedArgs& a, int grid, hipStream_t stream);
// The label modes (kBatchedDraw / kBatchedGiven) on the same work table; the partial blocks hold the statistics of the labels
// (one-hot operand, exact counts) and zero scalars.
hipError_t launch_batched_labels(const BatchedArgs& a, int mode, int grid, hipStream_t stream);
// The table mode (kBatchedWeights) on the same work table: the partial blocks hold the statistics of a.resp and zero scalars.
hipError_t launch_batched_weights(const BatchedArgs& a, int grid, hipStream_t stream);
// The row-selection mode (kBatchedSoftmaxRows): a.work is a work table built for the SELECTION sizes
// sel_off[b + 1] - sel_off[b] (batched_tiles_per_wg of them), a.partials has room for its grid.  Problem b's partial blocks are
// those launch_batched writes for a batch whose problem b holds the rows Z_b[sel_b] in that order, bit for bit.  Every index
// must lie in [0, N_b): the kernel does not check.
hipError_t launch_batched_rows(const BatchedArgs& a, int grid, hipStream_t stream);
// The weighted softmax mode (kBatchedSoftmaxWeighted) on the upload's work table: a.u holds one weight per row of the batch
// (problem b's at row_off[b]); the statistics blocks are those of r_kn w_n, the scalars and a.lse those of launch_batched.
// With every weight exactly 1.0 the partial blocks are those of launch_batched, bit for bit.
hipError_t launch_batched_weighted(const BatchedArgs& a, int grid, hipStream_t stream);
// The outer step of a mixture of mixtures over a SHARED batch: lse (B, N) holds the B problems' per-row log-normalisers.
// Per row n: t_b = lse[b N + n] + log_gating[b], m = max_b t_b, e_b = exp(t_b - m) (exactly 0 where log_gating[b] = -inf),
// s = sum_b e_b (b ascending); w[b N + n] = e_b / s.  out[b] = sum_n w[b N + n], out[B] = sum_n (m + log s): workgroup g sums
// the rows [256 g, 256 g + 256) into partials[g (B + 1) ..] — a row split that depends on N alone — and a second kernel adds
// the blocks in ascending order.  log_gating, lse, w, partials (outer_resp_partials(B, N) doubles), out: device pointers.
size_t outer_resp_partials(int B, int64_t N);
hipError_t launch_outer_resp(const double* lse, const double* log_gating, int B, int64_t N, double* w, double* partials, double* out,
                             hipStream_t stream);
// Random responsibilities of every problem in one launch, in the layout of BatchedArgs::resp: column n of problem b is
// random_resp_column (mimo_device.h) with key seeds[b] and the LOCAL row n — the table launch_random_resp writes for the
// problem's rows alone at row offset 0, bit for bit.  row_off and seeds are device pointers.
hipError_t launch_batched_random_resp(double* resp, const int64_t* row_off, const uint64_t* seeds, int B, int K, int64_t N_total,
                                      hipStream_t stream);
// Per problem: the fixed-order sum of its workgroups' partial blocks [wg_off[b], wg_off[b + 1]), unpacked into
// S[b] = K x (1 + Dz + Dz^2) (or nothing when S is null) and scalars[b] = {sum lse, sum r l, sum lse - sum r l}
// (the last two NaN unless `split`).
hipError_t launch_batched_reduce(const double* partials, const int32_t* wg_off, int B, const uint8_t* feat, int K, int D,
                                 int F, int F16, int split, double* S, double* scalars, hipStream_t stream);

}  // namespace mimo
