// The batched half of the C-ABI layer: the passes over B problems in one launch (mimo_batched.hip), the device-resident VI loop
// (mimo_vi_batched.hip) and batched prediction (mimo_predict_batched.hip).  The single-problem half is mimo_abi.cpp; what the two
// share is mimo_abi_internal.h.
//
// Every pass is put together from the same steps: the stacked operand image (batched_theta / image_len), room for the partial
// blocks (ensure_partials), the launch over a work table (build_work), and the reduction into the result block with the hand-out
// (reduce_and_deliver; batched_reduce alone inside the VI loop).
//
// What each entry point leaves resident (leaves() below sets the flags; an entry point that fails leaves them as they were set
// up to there).  "statistics" is the block [B][K][1 + Dz + Dz^2] in S_d that mimo_vi_run_batched starts from.
//
//   entry point                          valid afterwards                      dropped
//   mimo_upload_batched, _shared         —                                     everything (set_data), the VI priors
//   mimo_estep_batched, _rows            lse under MIMO_F_KEEP_LSE;            resp, logp, labels, lse without the flag;
//                                        statistics unless MIMO_F_NO_STATS     statistics under MIMO_F_NO_STATS
//   mimo_estep_batched_weighted          as mimo_estep_batched; row weights    as mimo_estep_batched
//   mimo_outer_resp_batched              row weights                           statistics (its sums take the result block)
//   mimo_gibbs_labels_batched            labels; statistics unless NO_STATS    resp, logp, lse
//   mimo_label_stats_batched             statistics                            —
//   mimo_weighted_stats_batched          statistics                            —
//   mimo_random_resp_stats_batched       resp (K); statistics                  —
//   mimo_vi_prior_batched                the priors and the loop state (K)     —
//   mimo_vi_run_batched                  statistics (of the last iteration)    resp, logp, labels, lse
//   mimo_svi_state_batched, _ilr_        the starting posterior of the SVI     the loop's trace and status (reset)
//                                        loop (K), its image and prior terms
//   mimo_svi_run_batched, _ilr_          statistics (of the last minibatch),   resp, logp, labels, lse
//                                        scalars (of the last plain pass)
//   mimo_predict_batched                 —                                     statistics (the outputs take the result block)
//   the getters                          —                                     —
#include "mimo_abi_internal.h"
#include "mimo_kernels.h"
#include "mimo_predict_batched.h"
#include "mimo_selection.h"
#include "mimo_vi_batched.h"
#include "mimo_vi_ilr_batched.h"

#include <algorithm>
#include <cmath>
#include <limits>

using namespace mimo;
using namespace mimo_abi;

// The resident tables an entry point speaks for
enum : unsigned { kResp = 1, kLogp = 2, kLse = 4, kLabels = 8, kRowWeights = 16, kPassTables = kResp | kLogp | kLse | kLabels };

// Of the tables in `of`, exactly those in `valid` are valid from here on; the others keep their state
static void leaves(mimo_ctx* ctx, unsigned of, unsigned valid) {
  if (of & kResp) ctx->resp_valid = (valid & kResp) != 0;
  if (of & kLogp) ctx->logp_valid = (valid & kLogp) != 0;
  if (of & kLse) ctx->lse_valid = (valid & kLse) != 0;
  if (of & kLabels) ctx->labels_valid = (valid & kLabels) != 0;
  if (of & kRowWeights) ctx->batch_w_valid = (valid & kRowWeights) != 0;
}

// off[0 .. B] starts at 0 and never decreases (`name`: what the entry point `me` calls the array)
static int check_offsets(mimo_ctx* ctx, const int64_t* off, int B, const char* me, const char* name) {
  if (off[0] != 0) return fail(ctx, MIMO_E_INVALID, "%s: %s[0] = %lld, must be 0", me, name, (long long)off[0]);
  for (int p = 0; p < B; ++p)
    if (off[p + 1] < off[p]) return fail(ctx, MIMO_E_INVALID, "%s: %s decreases at problem %d", me, name, p);
  return MIMO_OK;
}

// The work table of a batch (build_work_table, mimo_selection.h) under the library's rule for the tiles of one workgroup
static int build_work(mimo_ctx* ctx, const int64_t* off, int B, const char* me, std::vector<BatchedWork>* work,
                      std::vector<int32_t>* wg_off) {
  if (!build_work_table(off, B, batched_tiles_per_wg, work, wg_off)) return fail(ctx, MIMO_E_INVALID, "%s: too many rows", me);
  return MIMO_OK;
}

// ------------------------------------------------------------------------------------------
// Uploads
// ------------------------------------------------------------------------------------------
// The upload of a batch: `N` data rows, the concatenated rows of B problems (row_off[B] = N) or, `shared`, ONE block that all B
// problems read (row_off[b] = b N).  Both forms build the same tables from row_off.
static int upload_batch(mimo_ctx* ctx, const double* Z_host, int64_t N, const int64_t* row_off, int B, int Dz, bool shared,
                        const char* me) {
  int rc;
  if (!Z_host && N > 0) return fail(ctx, MIMO_E_INVALID, "%s: Z is NULL", me);
  // batched mode has no NaN-row semantics: every element must be finite
  for (int64_t i = 0; i < N * Dz; ++i)
    if (!std::isfinite(Z_host[i]))
      return fail(ctx, MIMO_E_INVALID, "%s: row %lld holds a NaN or an infinity", me, (long long)(i / Dz));
  std::vector<BatchedWork> work;
  std::vector<int32_t> wg_off;
  if ((rc = build_work(ctx, row_off, B, me, &work, &wg_off))) return rc;
  if ((rc = set_data(ctx, N, Dz))) return rc;
  if ((rc = set_rows(ctx, Z_host, Rows::HostCopy))) return rc;
  ctx->n_bad = 0; ctx->bad_counts_K = 0; ctx->data_sum_valid = false;
  // the three tables are replaced wholesale: each is as long as this batch needs
  HIP_TRY(ctx, ctx->batch_row_off_d.release());
  HIP_TRY(ctx, ctx->batch_work_d.release());
  HIP_TRY(ctx, ctx->batch_wg_off_d.release());
  if ((rc = ctx->batch_row_off_d.ensure(ctx, (size_t)B + 1))) return rc;
  if ((rc = ctx->batch_work_d.ensure(ctx, work.size()))) return rc;
  if ((rc = ctx->batch_wg_off_d.ensure(ctx, (size_t)B + 1))) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->batch_row_off_d, row_off, ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (!work.empty()) HIP_TRY(ctx, hipMemcpy(ctx->batch_work_d, work.data(), work.size() * sizeof(BatchedWork), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->batch_wg_off_d, wg_off.data(), ((size_t)B + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  ctx->batch_rows.assign(row_off, row_off + B + 1);
  ctx->batch_B = B;
  ctx->batch_G = (int)work.size();
  ctx->batched = true;
  ctx->batch_shared = shared;
  return MIMO_OK;
}

extern "C" {

int mimo_upload_batched(mimo_ctx* ctx, const double* Z_host, const int64_t* row_off, int B, int Dz) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (B < 1 || B > 65535 || !row_off) return fail(ctx, MIMO_E_INVALID, "mimo_upload_batched: B = %d outside [1, 65535] or row_off is NULL", B);
  if (Dz < 1 || Dz > kBatchedMaxD)
    return fail(ctx, MIMO_E_UNSUPPORTED, "mimo_upload_batched: Dz = %d outside [1, %d] (batched pass)", Dz, kBatchedMaxD);
  if ((rc = check_offsets(ctx, row_off, B, "mimo_upload_batched", "row_off"))) return rc;
  return upload_batch(ctx, Z_host, row_off[B], row_off, B, Dz, false, "mimo_upload_batched");
  });
}

int mimo_upload_batched_shared(mimo_ctx* ctx, const double* Z_host, int64_t N, int B, int Dz) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (B < 1 || B > 65535) return fail(ctx, MIMO_E_INVALID, "mimo_upload_batched_shared: B = %d outside [1, 65535]", B);
  if (N < 1) return fail(ctx, MIMO_E_INVALID, "mimo_upload_batched_shared: N = %lld, must be >= 1", (long long)N);
  if (Dz < 1 || Dz > kBatchedMaxD)
    return fail(ctx, MIMO_E_UNSUPPORTED, "mimo_upload_batched_shared: Dz = %d outside [1, %d] (batched pass)", Dz, kBatchedMaxD);
  if (N > std::numeric_limits<int64_t>::max() / ((int64_t)B * kBatchedMaxK))      // B N K: the longest per-problem buffer
    return fail(ctx, MIMO_E_INVALID, "mimo_upload_batched_shared: too many rows");
  std::vector<int64_t> row_off((size_t)B + 1);
  for (int b = 0; b <= B; ++b) row_off[(size_t)b] = (int64_t)b * N;
  return upload_batch(ctx, Z_host, N, row_off.data(), B, Dz, true, "mimo_upload_batched_shared");
  });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// The steps of a batched pass (mimo_batched.hip)
// ------------------------------------------------------------------------------------------
// The checks every batched pass shares (a batch, no pending call, no communicator, the full structure, a covered shape)
static int batched_ready(mimo_ctx* ctx, int K, const char* what) {
  if (!ctx->batched) return fail(ctx, MIMO_E_INVALID, "%s: the context holds no batch (call mimo_upload_batched)", what);
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (ctx->comm)
    return fail(ctx, MIMO_E_UNSUPPORTED, "%s: a communicator is attached (mimo_comm_init); the batched pass "
                "has no reduction over ranks", what);
  if (K < 1) return fail(ctx, MIMO_E_INVALID, "K must be >= 1 (got %d)", K);
  const int D = ctx->D;
  if (ctx->structure != MIMO_STRUCT_FULL)
    return fail(ctx, MIMO_E_UNSUPPORTED, "%s: only the full structure (symmetric W) is covered", what);
  if (!batched_covers(K, D))
    return fail(ctx, MIMO_E_UNSUPPORTED, "%s: K = %d, Dz = %d outside the batched kernels (K <= %d, Dz <= %d, "
                "ceil(K/16) * ceil(F/16) <= %d with F = (Dz+1)(Dz+2)/2)", what, K, D, kBatchedMaxK, kBatchedMaxD, kBatchedMaxPairs);
  return MIMO_OK;
}

// One problem's operand image: the single-problem image of the fused kernels, K16 row blocks of it
static ThetaGeneric batched_placement(const mimo_ctx* ctx, int K) { return {ctx->D, K, ctx->structure, (K + 15) / 16, ctx->F16 / 4}; }
// doubles of the stacked image [B][K16][NS][64] of the batch
static size_t image_len(const mimo_ctx* ctx, int K) { return batched_placement(ctx, K).count() * (size_t)ctx->batch_B; }

// The stacked image of the B problems' (c, b, W), followed by `nextra` uint64 words and then `nextra2` more; on the device at
// ctx->theta_d, the words at ctx->theta_d + image_len.
static int batched_theta(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K, const uint64_t* extra,
                         size_t nextra, const char* what, const uint64_t* extra2 = nullptr, size_t nextra2 = 0) {
  return stage_theta(ctx, batched_placement(ctx, K), c, b, W, ctx->batch_B, extra, nextra, what, nullptr, extra2, nextra2);
}

// `n` 8-byte words for a kernel that reads no operand image (log_gating, the seeds of the random start), through the image's
// pinned buffer; on the device at ctx->theta_d
static int stage_words(mimo_ctx* ctx, const void* src, size_t n) {
  int rc;
  if ((rc = ctx->theta_d.ensure(ctx, n))) return rc;
  if ((rc = ctx->theta_h.ensure(ctx, n))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));    // the staging buffer may still be in flight from the previous call on this stream
  memcpy(ctx->theta_h, src, n * sizeof(double));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->theta_d, ctx->theta_h, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return MIMO_OK;
}

static BatchedArgs batched_args(mimo_ctx* ctx, int K) {
  BatchedArgs a;
  a.Z = ctx->Z; a.row_off = ctx->batch_row_off_d; a.work = ctx->batch_work_d; a.theta = ctx->theta_d; a.feat = ctx->feat_d;
  a.partials = ctx->partials; a.lse = nullptr;
  a.D = ctx->D; a.K = K; a.K16 = (K + 15) / 16; a.F16 = ctx->F16;
  a.ZS = (ctx->D + 2) | 1;
  a.do_stats = 1;
  a.shared = ctx->batch_shared ? 1 : 0;
  a.u = nullptr; a.seeds = nullptr; a.labels = nullptr; a.sweep = 0; a.relabel = nullptr;
  a.resp = nullptr;
  a.sel = nullptr; a.sel_off = nullptr;
  return a;
}

// Room for the partial blocks of a launch over G workgroups (an empty batch still gets one)
static int ensure_partials(mimo_ctx* ctx, int K, size_t G) {
  return ctx->partials.ensure(ctx, partial_stride((K + 15) / 16, ctx->F16) * std::max<size_t>(G, 1));
}

// doubles of the statistics [B][K][1 + Dz + Dz^2] at the front of the result block; the 3 B scalars lie behind them
static size_t batch_stats_len(const mimo_ctx* ctx, int K) { return packed_len(K, ctx->D) * (size_t)ctx->batch_B; }

// Reduce the partial blocks of the launch just queued, per problem over the workgroups of `wg_off` (device), into the result
// block: the statistics (`want_stats`) and the scalars behind them.  The block is the resident statistics from here on.
static int batched_reduce(mimo_ctx* ctx, int K, const int32_t* wg_off, int split, bool want_stats) {
  double* sc_d = ctx->S_d + (want_stats ? batch_stats_len(ctx, K) : 0);
  HIP_TRY(ctx, launch_batched_reduce(ctx->partials, wg_off, ctx->batch_B, ctx->feat_d, K, ctx->D, ctx->F, ctx->F16, split,
                                     want_stats ? ctx->S_d.p : nullptr, sc_d, ctx->stream));
  ctx->batch_stats_valid = want_stats; ctx->batch_stats_K = K;
  return MIMO_OK;
}

// The same reduction for the scalars alone, into their place behind resident statistics of this K, which stay as they are and
// stay valid (the bound's pass of the SVI loop)
static int batched_reduce_scalars(mimo_ctx* ctx, int K, const int32_t* wg_off, int split) {
  HIP_TRY(ctx, launch_batched_reduce(ctx->partials, wg_off, ctx->batch_B, ctx->feat_d, K, ctx->D, ctx->F, ctx->F16, split, nullptr,
                                     ctx->S_d + batch_stats_len(ctx, K), ctx->stream));
  return MIMO_OK;
}

// The end of every pass that returns statistics: room for the result block, the reduction, and the hand-out of S (with
// `want_stats`) and of the 3 B scalars (null: not returned, and not copied).
static int reduce_and_deliver(mimo_ctx* ctx, int K, const int32_t* wg_off, int split, bool want_stats, double* S, double* scalars) {
  const size_t nstats = want_stats ? batch_stats_len(ctx, K) : 0, nsc = 3 * (size_t)ctx->batch_B;
  int rc;
  if ((rc = ensure_block(ctx, nstats + nsc))) return rc;
  if ((rc = batched_reduce(ctx, K, wg_off, split, want_stats))) return rc;
  return hand_out(ctx, scalars ? nstats + nsc : nstats, want_stats ? S : nullptr, nstats, scalars, nstats, nsc);
}

// ------------------------------------------------------------------------------------------
// Softmax passes
// ------------------------------------------------------------------------------------------
// How a softmax pass runs: over the upload's work table (launch_batched, or launch_batched_weighted with the resident row
// weights), or over a selection's own tables, which ride behind the operand image (launch_batched_rows).
struct SoftmaxForm {
  hipError_t (*launch)(const BatchedArgs&, int, hipStream_t);
  int allowed;                        // flags the form takes
  const char* allowed_text;           // ... as its refusal names them
  const double* weights = nullptr;    // launch_batched_weighted: the per-row weights of the statistics (device)
  // the rows form: `sel` (nsel indices) and then the selection's tables (mimo_selection.h) go behind the image in its transfer
  const uint64_t* sel = nullptr;
  size_t nsel = 0;
  const SelectionTables* tables = nullptr;
};

static int softmax_args(mimo_ctx* ctx, const SoftmaxForm& f, const double* c, const double* b, const double* W, int flags,
                        const double* S, const double* scalars, const char* me) {
  if (flags & ~f.allowed) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: only %s", me, flags, f.allowed_text);
  if (!c || !b || !W || !scalars || (!(flags & MIMO_F_NO_STATS) && !S))
    return fail(ctx, MIMO_E_INVALID, "%s: c, b, W, scalars (and S without MIMO_F_NO_STATS) must be non-NULL", me);
  return MIMO_OK;
}

// The softmax pass of a batch in the form `f`; the caller has run batched_ready and its own argument checks.
static int batched_softmax_pass(mimo_ctx* ctx, const SoftmaxForm& f, const double* c, const double* b, const double* W, int K,
                                int flags, double* S, double* scalars, const char* me) {
  int rc;
  if ((rc = softmax_args(ctx, f, c, b, W, flags, S, scalars, me))) return rc;
  if ((rc = batched_theta(ctx, c, b, W, K, f.sel, f.nsel, me, f.tables ? f.tables->words.data() : nullptr,
                          f.tables ? f.tables->words.size() : 0))) return rc;
  const size_t G = f.tables ? f.tables->G : (size_t)ctx->batch_G;
  if ((rc = ensure_partials(ctx, K, G))) return rc;
  const bool no_stats = (flags & MIMO_F_NO_STATS) != 0, keep_lse = (flags & MIMO_F_KEEP_LSE) != 0;
  if (keep_lse && (rc = ctx->lse.ensure(ctx, (size_t)table_rows(ctx)))) return rc;
  leaves(ctx, kPassTables, keep_lse ? kLse : 0);
  BatchedArgs a = batched_args(ctx, K);
  a.lse = keep_lse ? ctx->lse : nullptr;
  a.do_stats = no_stats ? 0 : 1;
  a.u = f.weights;
  const int32_t* wg_off = ctx->batch_wg_off_d;
  if (f.tables) {
    const uint64_t* sel_d = reinterpret_cast<const uint64_t*>(ctx->theta_d.p) + image_len(ctx, K);
    const uint64_t* tables_d = sel_d + f.nsel;
    a.sel = reinterpret_cast<const int64_t*>(sel_d);
    a.sel_off = reinterpret_cast<const int64_t*>(tables_d);
    a.work = reinterpret_cast<const BatchedWork*>(tables_d + f.tables->at_work);
    wg_off = reinterpret_cast<const int32_t*>(tables_d + f.tables->at_wg);
  }
  HIP_TRY(ctx, f.launch(a, (int)G, ctx->stream));
  const int split = (flags & (MIMO_F_ENTROPY_SPLIT | MIMO_F_KEEP_LSE)) ? 1 : 0;
  return reduce_and_deliver(ctx, K, wg_off, split, !no_stats, S, scalars);
}

static const char kPlainFlags[] = "MIMO_F_NO_STATS, MIMO_F_ENTROPY_SPLIT, MIMO_F_KEEP_LSE";

extern "C" {

int mimo_estep_batched(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K, int flags, double* S,
                       double* scalars) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, "mimo_estep_batched"))) return rc;
  const SoftmaxForm plain = {launch_batched, MIMO_F_NO_STATS | MIMO_F_ENTROPY_SPLIT | MIMO_F_KEEP_LSE, kPlainFlags};
  return batched_softmax_pass(ctx, plain, c, b, W, K, flags, S, scalars, "mimo_estep_batched");
  });
}

int mimo_estep_batched_weighted(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K, const double* row_weights,
                                int flags, double* S, double* scalars) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_estep_batched_weighted";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  const int64_t rows = table_rows(ctx);
  if (!row_weights) {
    if (!ctx->batch_w_valid || !ctx->batch_w)
      return fail(ctx, MIMO_E_STATE, "%s: row_weights is NULL and no weights are resident (an earlier call or mimo_outer_resp_batched "
                  "leaves them; an upload drops them)", me);
  } else {
    for (int64_t n = 0; n < rows; ++n)
      if (!(std::isfinite(row_weights[n]) && row_weights[n] >= 0.0))
        return fail(ctx, MIMO_E_INVALID, "%s: weight %lld is negative, NaN or an infinity", me, (long long)n);
    leaves(ctx, kRowWeights, 0);
    if ((rc = ctx->batch_w.ensure(ctx, (size_t)rows))) return rc;
    if (rows > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->batch_w, row_weights, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // row_weights is pageable host memory
    leaves(ctx, kRowWeights, kRowWeights);
  }
  SoftmaxForm weighted = {launch_batched_weighted, MIMO_F_NO_STATS | MIMO_F_ENTROPY_SPLIT | MIMO_F_KEEP_LSE, kPlainFlags};
  weighted.weights = ctx->batch_w;
  return batched_softmax_pass(ctx, weighted, c, b, W, K, flags, S, scalars, me);
  });
}

// The minibatch pass (launch_batched_rows): the softmax pass over a selection of every problem's resident rows.  The call's own
// work table — the selection sizes through batched_tiles_per_wg, as mimo_upload_batched builds its table from the row counts —
// travels with the indices behind the operand image; the upload's tables are left alone.
int mimo_estep_batched_rows(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K, const int64_t* rows,
                            const int64_t* sel_off, int flags, double* S, double* scalars) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_estep_batched_rows";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  SoftmaxForm form = {launch_batched_rows, MIMO_F_NO_STATS | MIMO_F_ENTROPY_SPLIT,
                      "MIMO_F_NO_STATS, MIMO_F_ENTROPY_SPLIT (a selection's normalisers have no place in the resident lse: no "
                      "MIMO_F_KEEP_LSE; the indices are host memory: no MIMO_F_DEVICE_IN)"};
  if ((rc = softmax_args(ctx, form, c, b, W, flags, S, scalars, me))) return rc;      // (first, as every softmax pass refuses)
  if (!rows || !sel_off) return fail(ctx, MIMO_E_INVALID, "%s: rows and sel_off must be non-NULL", me);
  const int B = ctx->batch_B;
  // the kernel gathers through these indices unchecked: every one is checked here, before anything is staged or launched
  if ((rc = check_offsets(ctx, sel_off, B, me, "sel_off"))) return rc;
  SelectionBad bad;
  if (!selection_indices_ok(rows, 1, sel_off, ctx->batch_rows.data(), B, &bad))
    return fail(ctx, MIMO_E_INVALID, "%s: problem %d: index %lld (entry %lld of its selection) outside [0, %lld)", me, bad.prob,
                (long long)bad.index, (long long)bad.entry, (long long)bad.rows);
  SelectionTables tables;
  if (!tables.build(sel_off, B, batched_tiles_per_wg)) return fail(ctx, MIMO_E_INVALID, "%s: too many rows", me);
  form.sel = reinterpret_cast<const uint64_t*>(rows); form.nsel = (size_t)sel_off[B];      // (straight from the caller's array)
  form.tables = &tables;
  return batched_softmax_pass(ctx, form, c, b, W, K, flags, S, scalars, me);
  });
}

int mimo_outer_resp_batched(mimo_ctx* ctx, const double* log_gating, int flags, double* out) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_outer_resp_batched";
  int rc = bind(ctx); if (rc) return rc;
  if (!ctx->batched || !ctx->batch_shared)
    return fail(ctx, MIMO_E_STATE, "%s: the context holds no shared batch (call mimo_upload_batched_shared)", me);
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (!ctx->lse_valid || !ctx->lse)
    return fail(ctx, MIMO_E_STATE, "%s: no lse is resident (run mimo_estep_batched / _weighted with MIMO_F_KEEP_LSE first)", me);
  if (flags != 0) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: none are defined", me, flags);
  if (!log_gating || !out) return fail(ctx, MIMO_E_INVALID, "%s: log_gating and out must be non-NULL", me);
  const int B = ctx->batch_B;
  const int64_t N = ctx->N;
  bool any = false;
  for (int p = 0; p < B; ++p) {
    if (std::isnan(log_gating[p]) || log_gating[p] == std::numeric_limits<double>::infinity())
      return fail(ctx, MIMO_E_INVALID, "%s: log_gating[%d] is NaN or +inf", me, p);
    any = any || std::isfinite(log_gating[p]);
  }
  if (!any) return fail(ctx, MIMO_E_INVALID, "%s: every entry of log_gating is -inf", me);
  if ((rc = stage_words(ctx, log_gating, (size_t)B))) return rc;
  leaves(ctx, kRowWeights, 0);
  if ((rc = ctx->batch_w.ensure(ctx, (size_t)B * (size_t)N))) return rc;
  if ((rc = ctx->partials.ensure(ctx, outer_resp_partials(B, N)))) return rc;
  if ((rc = ensure_block(ctx, (size_t)B + 1))) return rc;
  HIP_TRY(ctx, launch_outer_resp(ctx->lse, ctx->theta_d, B, N, ctx->batch_w, ctx->partials, ctx->S_d, ctx->stream));
  leaves(ctx, kRowWeights, kRowWeights);
  return hand_out(ctx, (size_t)B + 1, out, (size_t)B + 1, nullptr, 0, 0);
  });
}

int mimo_get_row_weights_batched(mimo_ctx* ctx, double* out) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  if (!ctx->batched || !ctx->batch_w_valid)
    return fail(ctx, MIMO_E_STATE, "mimo_get_row_weights_batched: no row weights are resident");
  const size_t rows = (size_t)table_rows(ctx);
  if (rows == 0) return MIMO_OK;
  return copy_out(ctx, out, ctx->batch_w, rows * sizeof(double), true, "mimo_get_row_weights_batched");
  });
}

// ------------------------------------------------------------------------------------------
// Label and table passes
// ------------------------------------------------------------------------------------------
// Their statistics: the partial blocks of the launch just queued, reduced per problem into S (B x K(1+Dz+Dz^2)); the scalars the
// reduction also writes (zeros) are not returned.
static int batched_stats_out(mimo_ctx* ctx, int K, double* S) {
  return reduce_and_deliver(ctx, K, ctx->batch_wg_off_d, 0, true, S, nullptr);
}

int mimo_gibbs_labels_batched(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
                              const uint64_t* seeds, uint64_t sweep, const double* u, int flags, int32_t* labels_out,
                              double* S) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_gibbs_labels_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags & ~MIMO_F_NO_STATS) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: only MIMO_F_NO_STATS", me, flags);
  const bool no_stats = (flags & MIMO_F_NO_STATS) != 0;
  if (!c || !b || !W || (!no_stats && !S))
    return fail(ctx, MIMO_E_INVALID, "%s: c, b, W (and S without MIMO_F_NO_STATS) must be non-NULL", me);
  if (!u && !seeds)
    return fail(ctx, MIMO_E_INVALID, "%s: u and seeds are both NULL (give the uniforms or one Philox seed per problem)", me);
  const int B = ctx->batch_B, G = ctx->batch_G;
  const int64_t N = table_rows(ctx);
  // problems with components switched off by c = -inf: the draw's relabel table of every problem (draw_label, mimo_device.h)
  std::vector<int32_t> relabel;
  for (int p = 0; p < B; ++p) {
    int32_t row[kBatchedMaxK];
    if (!draw_relabel(c + (size_t)p * K, K, row)) continue;
    if (relabel.empty()) {
      relabel.resize(((size_t)B * K + 1) / 2 * 2);
      for (size_t i = 0; i < (size_t)B * K; ++i) relabel[i] = (int32_t)(i % K);
    }
    memcpy(&relabel[(size_t)p * K], row, (size_t)K * sizeof(int32_t));
  }
  // the seeds and the relabel table travel behind the operand image, in its transfer
  const size_t nseeds = u ? 0 : (size_t)B;
  if ((rc = batched_theta(ctx, c, b, W, K, u ? nullptr : seeds, nseeds, me, reinterpret_cast<const uint64_t*>(relabel.data()),
                          relabel.size() / 2))) return rc;
  if ((rc = ctx->labels.ensure(ctx, (size_t)N))) return rc;
  const double* ud = nullptr;
  bool copied = false;        // (u NULL: Philox uniforms from the seeds; the flags admit no MIMO_F_DEVICE_IN)
  if ((rc = stage_input<double>(ctx, u, (size_t)N, flags, ctx->u_d, {}, K, &ud, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // u is pageable host memory
  if (copied) ctx->weights_resident = false;                     // u_d holds uniforms now
  if ((rc = ensure_partials(ctx, K, (size_t)G))) return rc;
  leaves(ctx, kResp | kLogp | kLse, 0);
  BatchedArgs a = batched_args(ctx, K);
  a.do_stats = no_stats ? 0 : 1;
  a.u = ud;
  a.seeds = u ? nullptr : reinterpret_cast<const uint64_t*>(ctx->theta_d + image_len(ctx, K));
  a.labels = ctx->labels;
  a.sweep = sweep;
  if (!relabel.empty()) a.relabel = reinterpret_cast<const int32_t*>(ctx->theta_d + image_len(ctx, K) + nseeds);
  HIP_TRY(ctx, launch_batched_labels(a, kBatchedDraw, G, ctx->stream));
  leaves(ctx, kLabels, kLabels);
  if (!no_stats && (rc = batched_stats_out(ctx, K, S))) return rc;
  if (labels_out && N > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(labels_out, ctx->labels, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}

int mimo_label_stats_batched(mimo_ctx* ctx, const int32_t* labels, int K, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_label_stats_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags != 0) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: none are defined", me, flags);
  if (!S) return fail(ctx, MIMO_E_INVALID, "%s: S is NULL", me);
  const int64_t N = table_rows(ctx);
  const int G = ctx->batch_G;
  // the kernel indexes its accumulators by label: the caller's labels are checked on the host, before anything is staged
  for (int64_t n = 0; labels && n < N; ++n)
    if (labels[n] < 0 || labels[n] >= K)
      return fail(ctx, MIMO_E_INVALID, "%s: label %d of row %lld outside [0, %d)", me, labels[n], (long long)n, K);
  const int32_t* lab = nullptr;
  bool copied = false;        // (flags is 0: the labels are the resident draw or host memory)
  if ((rc = stage_input<int32_t>(ctx, labels, (size_t)N, flags, ctx->lin,
                                 {ctx->labels, ctx->labels_valid && ctx->labels, "mimo_label_stats_batched: labels is NULL and no batched draw is resident"},
                                 K, &lab, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // labels is pageable host memory
  if ((rc = ensure_partials(ctx, K, (size_t)G))) return rc;
  BatchedArgs a = batched_args(ctx, K);
  a.labels = const_cast<int32_t*>(lab);
  HIP_TRY(ctx, launch_batched_labels(a, kBatchedGiven, G, ctx->stream));
  return batched_stats_out(ctx, K, S);
  });
}

// The table pass of a batch (launch_batched_weights over the device table `table`, the problems' K-major (K, N_b) blocks back
// to back) and its statistics
static int batched_table_stats(mimo_ctx* ctx, const double* table, int K, double* S) {
  const int G = ctx->batch_G;
  int rc;
  if ((rc = ensure_partials(ctx, K, (size_t)G))) return rc;
  BatchedArgs a = batched_args(ctx, K);
  a.resp = table;
  HIP_TRY(ctx, launch_batched_weights(a, G, ctx->stream));
  return batched_stats_out(ctx, K, S);
}

int mimo_weighted_stats_batched(mimo_ctx* ctx, const double* resp, int K, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_weighted_stats_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags != 0) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: none are defined", me, flags);
  if (!S) return fail(ctx, MIMO_E_INVALID, "%s: S is NULL", me);
  const double* table = nullptr;
  bool copied = false;        // (flags is 0: the table is the resident one or host memory; its values are taken as they are)
  if ((rc = stage_input<double>(ctx, resp, (size_t)K * (size_t)table_rows(ctx), flags, ctx->win,
                                {ctx->resp, ctx->resp_valid && ctx->resp_K == K && ctx->resp,
                                 "mimo_weighted_stats_batched: resp is NULL and no (K=%d, N_total) table is resident"},
                                K, &table, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // resp is pageable host memory
  return batched_table_stats(ctx, table, K, S);
  });
}

int mimo_random_resp_stats_batched(mimo_ctx* ctx, int K, const uint64_t* seeds, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_random_resp_stats_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags != 0) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: none are defined", me, flags);
  if (!S || !seeds) return fail(ctx, MIMO_E_INVALID, "%s: S and seeds must be non-NULL", me);
  const int B = ctx->batch_B;
  const int64_t N = table_rows(ctx);
  leaves(ctx, kResp, 0);
  if ((rc = ctx->resp.ensure(ctx, (size_t)K * (size_t)N))) return rc;
  if ((rc = stage_words(ctx, seeds, (size_t)B))) return rc;
  HIP_TRY(ctx, launch_batched_random_resp(ctx->resp, ctx->batch_row_off_d, reinterpret_cast<const uint64_t*>(ctx->theta_d.p), B, K, N,
                                          ctx->stream));
  ctx->resp_K = K;
  leaves(ctx, kResp, kResp);
  return batched_table_stats(ctx, ctx->resp, K, S);
  });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Device-resident batched VI and SVI (mimo_vi_batched.hip, mimo_vi_ilr_batched.hip)
// ------------------------------------------------------------------------------------------
// One family is resident at a time (ctx->vi_family indexes kViFamilies), in the same five buffers:
//   vi_prior  the parts of the family's prior call, each [B][...], in the call's order (ViArgs / ViIlrArgs)
//   vi_post   [2][B][post_len]
//   vi_work   [the family's term arrays, B K each | prior terms B | last bound B]
//   vi_theta  the operand images the loop's passes read;  vi_loop  the words, then the trace of one call
// The SVI loop adds svi_sel (the minibatch indices of one call) and svi_tables (SelectionTables, mimo_selection.h).
struct ViFamily {
  int id;                                          // ctx->vi_family
  const char* name;                                // as the refusals name the family
  const char* prior_call;                          // the entry points that install its priors and its starting posterior
  const char* state_call;
  size_t (*post_len)(const mimo_ctx*, int K);      // doubles per problem of the posterior block
  size_t terms;                                    // term arrays at the front of vi_work: vi_work holds terms B K + 2 B doubles
  int (*step)(mimo_ctx*, const ViLoop&);           // the update and the gating kernel in the loop's mode
};

// the family's priors in vi_prior, one after the other: *p, then *p behind `per_bk` doubles per (problem, component)
static const double* next_part(const double** p, const ViLoop& l, size_t per_bk) {
  const double* at = *p;
  *p += (size_t)l.B * l.K * per_bk;
  return at;
}

static int vi_gmm_step(mimo_ctx* ctx, const ViLoop& l) {
  const size_t D = (size_t)l.D;
  ViArgs a{};
  a.loop = l;
  const double* p = ctx->vi_prior;
  a.alpha0 = next_part(&p, l, 1);
  a.pa = next_part(&p, l, D); a.pb = next_part(&p, l, 1); a.pc = next_part(&p, l, D * D); a.pd = next_part(&p, l, 1);
  a.plz = next_part(&p, l, 1);
  a.term = ctx->vi_work;
  HIP_TRY(ctx, launch_vi_update(a, ctx->stream));
  HIP_TRY(ctx, launch_vi_gating(a, ctx->stream));
  return MIMO_OK;
}

static int vi_ilr_step(mimo_ctx* ctx, const ViLoop& l) {
  const size_t dx = (size_t)ctx->vi_dx, dy = (size_t)ctx->vi_dy, dc = dx + 1;
  ViIlrArgs a{};
  a.loop = l;
  const double* p = ctx->vi_prior;
  a.g0 = next_part(&p, l, 1); a.g1 = next_part(&p, l, 1);
  a.pa = next_part(&p, l, dx); a.pb = next_part(&p, l, 1); a.pc = next_part(&p, l, dx * dx); a.pd = next_part(&p, l, 1);
  a.plz = next_part(&p, l, 1);
  a.ma = next_part(&p, l, dy * dc); a.mb = next_part(&p, l, dc * dc); a.mc = next_part(&p, l, dy * dy); a.md = next_part(&p, l, 1);
  a.mlz = next_part(&p, l, 1);
  a.term_b = ctx->vi_work;
  a.term_m = ctx->vi_work + (size_t)l.B * l.K;
  a.dx = ctx->vi_dx; a.dy = ctx->vi_dy; a.gating = ctx->vi_gating;
  HIP_TRY(ctx, launch_vi_ilr_update(a, ctx->stream));
  HIP_TRY(ctx, launch_vi_ilr_gating(a, ctx->stream));
  return MIMO_OK;
}

enum { kViGmm = 0, kViIlr = 1 };
static const ViFamily kViFamilies[2] = {
    {kViGmm, "mixtures of Gaussians (mimo_vi_prior_batched)", "mimo_vi_prior_batched", "mimo_svi_state_batched",
     [](const mimo_ctx* ctx, int K) { return (size_t)ViLayout{K, ctx->D}.count(); }, 1, vi_gmm_step},
    {kViIlr, "mixtures of linear-Gaussian experts (mimo_vi_ilr_prior_batched)", "mimo_vi_ilr_prior_batched",
     "mimo_svi_ilr_state_batched",
     [](const mimo_ctx* ctx, int K) { return (size_t)ViIlrLayout{K, ctx->vi_dx, ctx->vi_dy}.count(); }, 2, vi_ilr_step}};

// doubles the loop's int32 words take at the front of vi_loop
static size_t vi_words_len(int B) { return ((size_t)kViWords * B + 1) / 2; }
static size_t vi_work_len(const mimo_ctx* ctx, int K, const ViFamily& f) { return (f.terms * K + 2) * (size_t)ctx->batch_B; }

// What the loop's entry points share beyond batched_ready: a prior block of this K and of the caller's family (null: either)
static int vi_ready(mimo_ctx* ctx, int K, const char* me, const ViFamily* f) {
  if (!ctx->vi_prior_valid || !ctx->vi_prior)
    return fail(ctx, MIMO_E_STATE, "%s: no prior block is resident (call %s; an upload drops it)", me,
                (f ? f : kViFamilies)->prior_call);
  if (f && ctx->vi_family != f->id)
    return fail(ctx, MIMO_E_STATE, "%s: the resident prior block is that of %s, this call runs %s", me,
                kViFamilies[ctx->vi_family].name, f->name);
  if (ctx->vi_K != K)
    return fail(ctx, MIMO_E_STATE, "%s: the resident prior block is that of K = %d, not K = %d", me, ctx->vi_K, K);
  return MIMO_OK;
}

// What the pass, its reduction, the finish and the family's step read: the conjugate mode, tol = 0
static ViLoop vi_loop_args(mimo_ctx* ctx, int K, const ViFamily& f) {
  const size_t B = (size_t)ctx->batch_B;
  ViLoop l{};
  l.S = ctx->S_d;
  l.scalars = ctx->S_d + batch_stats_len(ctx, K);
  l.post = ctx->vi_post;
  l.prior_terms = ctx->vi_work + vi_work_len(ctx, K, f) - 2 * B;
  l.last = l.prior_terms + B;
  l.words = reinterpret_cast<int32_t*>(ctx->vi_loop.p);
  l.theta = ctx->vi_theta;
  l.trace = ctx->vi_loop + vi_words_len(ctx->batch_B);
  l.B = ctx->batch_B; l.K = K; l.D = ctx->D; l.K16 = (K + 15) / 16; l.NS = ctx->F16 / 4;
  return l;
}

// One part of a prior block or of an uploaded posterior: `len` doubles per problem (at `at` of the family's posterior block)
struct ViPart { const char* name; const double* src; size_t len; size_t at; };

static int vi_parts_finite(mimo_ctx* ctx, const ViPart* parts, int nparts, const char* me) {
  const size_t B = (size_t)ctx->batch_B;
  for (int t = 0; t < nparts; ++t)
    for (size_t i = 0; i < parts[t].len * B; ++i)
      if (!std::isfinite(parts[t].src[i]))
        return fail(ctx, MIMO_E_INVALID, "%s: %s of problem %d holds a NaN or an infinity", me, parts[t].name, (int)(i / parts[t].len));
  return MIMO_OK;
}

// The loop state of a new prior block or a new starting posterior: every problem active, nothing appended, status clear, slot 0
// current; slot 0 of every problem from `slot0` (host, alive up to the caller's wait; null: zeros), slot 1 zero; zero work, zero
// images (the entries no kernel writes — padded features, the b / W entries of padding components — are the zeros pack_theta
// leaves there)
static int vi_reset_loop(mimo_ctx* ctx, int K, const ViFamily& f, const double* slot0) {
  const size_t B = (size_t)ctx->batch_B, half = B * f.post_len(ctx, K);
  static_assert(kViActive == 0, "the words' first row is set to 1 below");
  HIP_TRY(ctx, hipMemsetAsync(ctx->vi_loop, 0, (size_t)kViWords * B * sizeof(int32_t), ctx->stream));
  HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->vi_loop.p), 1, B, ctx->stream));
  if (slot0) HIP_TRY(ctx, hipMemcpyAsync(ctx->vi_post, slot0, half * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->vi_post + (slot0 ? half : 0), 0, (slot0 ? 1 : 2) * half * sizeof(double), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->vi_work, 0, vi_work_len(ctx, K, f) * sizeof(double), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->vi_theta, 0, image_len(ctx, K) * sizeof(double), ctx->stream));
  return MIMO_OK;
}

// What the two prior calls share behind their own argument checks: the parts, checked finite, into vi_prior in their order, room
// for the loop and its reset.  (dx, dy, gating: of the linear-Gaussian experts; they size that family's posterior block.)
static int vi_install_prior(mimo_ctx* ctx, int K, const ViFamily& f, const ViPart* parts, int nparts, int dx, int dy, int gating,
                            const char* me) {
  const size_t B = (size_t)ctx->batch_B;
  int rc;
  if ((rc = vi_parts_finite(ctx, parts, nparts, me))) return rc;
  ctx->vi_prior_valid = false;
  ctx->svi_state_valid = false;
  ctx->vi_dx = dx; ctx->vi_dy = dy; ctx->vi_gating = gating;
  size_t nprior = 0;
  for (int t = 0; t < nparts; ++t) nprior += B * parts[t].len;
  if ((rc = ctx->vi_prior.ensure(ctx, nprior))) return rc;
  if ((rc = ctx->vi_post.ensure(ctx, 2 * B * f.post_len(ctx, K)))) return rc;
  if ((rc = ctx->vi_work.ensure(ctx, vi_work_len(ctx, K, f)))) return rc;
  if ((rc = ctx->vi_theta.ensure(ctx, image_len(ctx, K)))) return rc;
  if ((rc = ctx->vi_loop.ensure(ctx, vi_words_len(ctx->batch_B)))) return rc;
  double* q = ctx->vi_prior;
  for (int t = 0; t < nparts; ++t) {
    HIP_TRY(ctx, hipMemcpyAsync(q, parts[t].src, B * parts[t].len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    q += B * parts[t].len;
  }
  if ((rc = vi_reset_loop(ctx, K, f, nullptr))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // the sources are pageable host memory
  ctx->vi_prior_valid = true;
  ctx->vi_K = K;
  ctx->vi_family = f.id;
  return MIMO_OK;
}

// Room for the loop's words and the trace of a call of `iters` iterations, on the device and in the pinned sibling; *total: their
// doubles.  A longer trace than any before: the words move to the new block.
static int vi_loop_room(mimo_ctx* ctx, int iters, size_t* total) {
  const int B = ctx->batch_B;
  const size_t nwords = vi_words_len(B);
  int rc;
  *total = nwords + (size_t)iters * B;
  if (ctx->vi_loop.cap < *total) {
    Buf<double> grown;
    if ((rc = grown.ensure(ctx, *total))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(grown.p, ctx->vi_loop.p, nwords * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(grown.p, ctx->vi_loop.p);
    std::swap(grown.cap, ctx->vi_loop.cap);
  }
  return ctx->vi_loop_h.ensure(ctx, *total);
}

// The end of a loop call: the words and the trace to the host in one copy behind everything queued, then the caller's arrays
static int vi_loop_out(mimo_ctx* ctx, int iters, size_t total, double* trace, int32_t* n_done, int32_t* status) {
  const int B = ctx->batch_B;
  const size_t nwords = vi_words_len(B);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->vi_loop_h, ctx->vi_loop, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t* words = reinterpret_cast<const int32_t*>(ctx->vi_loop_h.p);
  if (trace) memcpy(trace, ctx->vi_loop_h + nwords, (size_t)iters * B * sizeof(double));
  if (n_done) memcpy(n_done, words + (size_t)kViDone * B, (size_t)B * sizeof(int32_t));
  memcpy(status, words + (size_t)kViStatus * B, (size_t)B * sizeof(int32_t));
  return MIMO_OK;
}

// The loop of both families: the family's update and gating kernel; the pass, its reduction and the finish are shared
static int vi_run(mimo_ctx* ctx, int K, int iters, double tol, int flags, double* trace, int32_t* n_done, int32_t* status,
                  const char* me, const ViFamily& f) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags != 0) return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: none are defined", me, flags);
  if (iters < 1 || iters > 65536) return fail(ctx, MIMO_E_INVALID, "%s: iters = %d outside [1, 65536]", me, iters);
  if (!(tol >= 0.0)) return fail(ctx, MIMO_E_INVALID, "%s: tol = %g must be >= 0", me, tol);
  if (!trace || !n_done || !status) return fail(ctx, MIMO_E_INVALID, "%s: trace, n_done and status must be non-NULL", me);
  if ((rc = vi_ready(ctx, K, me, &f))) return rc;
  if (!ctx->batch_stats_valid || !ctx->S_d)
    return fail(ctx, MIMO_E_STATE, "%s: no statistics are resident (run a batched pass that returns statistics first; an upload and "
                "every call that returns something else drop them)", me);
  if (ctx->batch_stats_K != K)
    return fail(ctx, MIMO_E_STATE, "%s: the resident statistics are those of K = %d, not K = %d", me, ctx->batch_stats_K, K);
  const int B = ctx->batch_B, G = ctx->batch_G;
  size_t total = 0;
  if ((rc = vi_loop_room(ctx, iters, &total))) return rc;
  if ((rc = ensure_partials(ctx, K, (size_t)G))) return rc;
  leaves(ctx, kPassTables, 0);

  ViLoop l = vi_loop_args(ctx, K, f);
  l.tol = tol;
  BatchedArgs a = batched_args(ctx, K);
  a.theta = ctx->vi_theta;
  HIP_TRY(ctx, hipMemsetAsync(l.words + (size_t)kViDone * B, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  for (int it = 0; it < iters; ++it) {
    if ((rc = f.step(ctx, l))) return rc;
    HIP_TRY(ctx, launch_batched(a, G, ctx->stream));
    if ((rc = batched_reduce(ctx, K, ctx->batch_wg_off_d, 0, true))) return rc;
    HIP_TRY(ctx, launch_vi_finish(l, it, ctx->stream));
  }
  return vi_loop_out(ctx, iters, total, trace, n_done, status);
  });
}

// Every problem's current posterior block (in the family's layout) to the host
static int vi_get(mimo_ctx* ctx, int K, double* out, const char* me, const ViFamily& f) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (!out) return fail(ctx, MIMO_E_INVALID, "%s: out is NULL", me);
  if ((rc = vi_ready(ctx, K, me, &f))) return rc;
  const size_t B = (size_t)ctx->batch_B, per = f.post_len(ctx, K);
  std::vector<double> both(2 * B * per);
  std::vector<int32_t> words((size_t)kViWords * B);
  HIP_TRY(ctx, hipMemcpyAsync(both.data(), ctx->vi_post, both.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(words.data(), ctx->vi_loop, words.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t p = 0; p < B; ++p) {
    const size_t slot = words[(size_t)kViSlot * B + p] ? 1 : 0;
    memcpy(out + p * per, both.data() + (slot * B + p) * per, per * sizeof(double));
  }
  return MIMO_OK;
  });
}

// What mimo_svi_state_batched and mimo_svi_ilr_state_batched share behind batched_ready and vi_ready: the parts, checked finite,
// into slot 0 of a loop that is reset as the prior call resets it; then the init mode of the family's update and gating kernel,
// and the status words back.
static int svi_state(mimo_ctx* ctx, int K, const ViPart* parts, int nparts, int32_t* status, const char* me, const ViFamily& f) {
  const size_t B = (size_t)ctx->batch_B, per = f.post_len(ctx, K);
  int rc;
  for (int t = 0; t < nparts; ++t)
    if (!parts[t].src) return fail(ctx, MIMO_E_INVALID, "%s: %s is NULL", me, parts[t].name);
  if (!status) return fail(ctx, MIMO_E_INVALID, "%s: status is NULL", me);
  if ((rc = vi_parts_finite(ctx, parts, nparts, me))) return rc;
  ctx->svi_state_valid = false;
  std::vector<double> block(B * per, 0.0);
  for (int t = 0; t < nparts; ++t)
    for (size_t p = 0; p < B; ++p)
      memcpy(&block[p * per + parts[t].at], parts[t].src + p * parts[t].len, parts[t].len * sizeof(double));
  if ((rc = vi_reset_loop(ctx, K, f, block.data()))) return rc;
  ViLoop l = vi_loop_args(ctx, K, f);
  l.mode = kViInit;
  if ((rc = f.step(ctx, l))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(status, l.words + (size_t)kViStatus * B, B * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the sources are pageable host memory)
  ctx->svi_state_valid = true;
  ctx->svi_t = 0;
  return MIMO_OK;
}

// The SVI loop of both families (as vi_run is): per iteration the selection pass and its reduction (the statistics of the
// minibatch), the blend update and the blend gating, a plain pass over all rows without statistics, its scalar reduction, and the
// finish with tol = 0.  sel_off is the same for every iteration: one work table per call.
static int svi_run(mimo_ctx* ctx, int K, int iters, double step_size, const double* scale, const int64_t* rows,
                   const int64_t* sel_off, const uint64_t* seeds, int flags, double* trace, int32_t* n_done, int32_t* status,
                   const char* me, const ViFamily& f) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (flags & ~MIMO_F_SVI_RESIDENT_START)
    return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: only MIMO_F_SVI_RESIDENT_START", me, flags);
  if (iters < 1 || iters > 65536) return fail(ctx, MIMO_E_INVALID, "%s: iters = %d outside [1, 65536]", me, iters);
  if (!(step_size > 0.0 && step_size <= 1.0)) return fail(ctx, MIMO_E_INVALID, "%s: step_size = %g outside (0, 1]", me, step_size);
  if (!scale || !sel_off || !trace || !n_done || !status)
    return fail(ctx, MIMO_E_INVALID, "%s: scale, sel_off, trace, n_done and status must be non-NULL", me);
  const int B = ctx->batch_B, G = ctx->batch_G;
  for (int p = 0; p < B; ++p)
    if (!(std::isfinite(scale[p]) && scale[p] > 0.0))      // (above 1: a minibatch drawn with replacement, larger than its data set)
      return fail(ctx, MIMO_E_INVALID, "%s: scale[%d] = %g must be finite and > 0", me, p, scale[p]);
  if ((rc = vi_ready(ctx, K, me, &f))) return rc;
  if (!ctx->svi_state_valid)
    return fail(ctx, MIMO_E_STATE, "%s: no starting posterior is resident (call %s after the prior block; an upload and a new prior "
                "block drop it)", me, f.state_call);
  if ((rc = check_offsets(ctx, sel_off, B, me, "sel_off"))) return rc;
  const bool resident_start = (flags & MIMO_F_SVI_RESIDENT_START) != 0;
  if (resident_start && (!ctx->batch_stats_valid || ctx->batch_stats_K != K || !ctx->S_d))
    return fail(ctx, MIMO_E_STATE, "%s: MIMO_F_SVI_RESIDENT_START and no statistics of K = %d are resident (run a batched pass that "
                "returns statistics first)", me, K);
  const int n_sel = iters - (resident_start ? 1 : 0), first = resident_start ? 1 : 0;
  const int64_t per_it = sel_off[B];
  if (n_sel > 0 && per_it > 0 && !rows && !seeds)
    return fail(ctx, MIMO_E_INVALID, "%s: rows and seeds are both NULL (give the indices or one Philox seed per problem)", me);
  // the selection pass gathers through the indices unchecked: every one of every iteration is checked here, before anything is
  // enqueued; the index kernel's own stay below N_b by construction, given a row to draw
  SelectionBad bad;
  if (rows && !selection_indices_ok(rows, n_sel, sel_off, ctx->batch_rows.data(), B, &bad))
    return fail(ctx, MIMO_E_INVALID, "%s: iteration %d, problem %d: index %lld (entry %lld of its selection) outside [0, %lld)", me,
                bad.sel + first, bad.prob, (long long)bad.index, (long long)bad.entry, (long long)bad.rows);
  for (int p = 0; !rows && n_sel > 0 && p < B; ++p)
    if (sel_off[p + 1] > sel_off[p] && ctx->batch_rows[(size_t)p + 1] - ctx->batch_rows[(size_t)p] < 1)
      return fail(ctx, MIMO_E_INVALID, "%s: problem %d has no rows to draw its %lld indices from", me, p,
                  (long long)(sel_off[p + 1] - sel_off[p]));
  SelectionTables tables;
  if (!tables.build(sel_off, B, batched_tiles_per_wg, seeds, scale)) return fail(ctx, MIMO_E_INVALID, "%s: too many rows", me);
  const size_t Gs = tables.G;
  size_t total = 0;
  if ((rc = vi_loop_room(ctx, iters, &total))) return rc;
  if ((rc = ensure_partials(ctx, K, std::max(Gs, (size_t)G)))) return rc;
  if (!resident_start && (rc = ensure_block(ctx, batch_stats_len(ctx, K) + 3 * (size_t)B))) return rc;
  if ((rc = ctx->svi_tables.ensure(ctx, tables.words.size()))) return rc;
  if ((rc = ctx->svi_sel.ensure(ctx, (size_t)std::max(n_sel, 0) * (size_t)per_it))) return rc;
  leaves(ctx, kPassTables, 0);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->svi_tables, tables.words.data(), tables.words.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                              ctx->stream));
  const uint64_t* const tables_d = ctx->svi_tables;
  const int64_t* const sel_off_d = reinterpret_cast<const int64_t*>(tables_d);
  const int32_t* const wg_off_d = reinterpret_cast<const int32_t*>(tables_d + tables.at_wg);
  if (n_sel > 0 && per_it > 0) {
    if (rows) {
      HIP_TRY(ctx, hipMemcpyAsync(ctx->svi_sel, rows, (size_t)n_sel * (size_t)per_it * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    } else {
      for (int s = 0; s < n_sel; s += 65535)      // (a grid's second dimension)
        HIP_TRY(ctx, launch_svi_indices(ctx->svi_sel + (size_t)s * (size_t)per_it, sel_off_d, ctx->batch_row_off_d,
                                        tables_d + tables.at_seeds, B, std::min(n_sel - s, 65535), per_it,
                                        ctx->svi_t + (uint64_t)(first + s), ctx->stream));
    }
  }

  ViLoop l = vi_loop_args(ctx, K, f);         // (tol = 0: SVI has no stopping rule)
  l.mode = kViBlend;
  l.rho = step_size;
  l.one_minus_rho = 1.0 - step_size;
  l.inv_scale = reinterpret_cast<const double*>(tables_d + tables.at_inv);
  BatchedArgs sel_a = batched_args(ctx, K), full_a = batched_args(ctx, K);
  sel_a.theta = full_a.theta = ctx->vi_theta;
  sel_a.sel_off = sel_off_d;
  sel_a.work = reinterpret_cast<const BatchedWork*>(tables_d + tables.at_work);
  full_a.do_stats = 0;
  HIP_TRY(ctx, hipMemsetAsync(l.words + (size_t)kViDone * B, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  for (int it = 0; it < iters; ++it) {
    if (it >= first) {
      sel_a.sel = ctx->svi_sel + (size_t)(it - first) * (size_t)per_it;
      if (Gs) HIP_TRY(ctx, launch_batched_rows(sel_a, (int)Gs, ctx->stream));      // (no slots at all: the reduction leaves zeros)
      if ((rc = batched_reduce(ctx, K, wg_off_d, 0, true))) return rc;
    }
    if ((rc = f.step(ctx, l))) return rc;
    // the bound's pass: all rows, no statistics — the minibatch's stay resident, the scalars go behind them as always
    HIP_TRY(ctx, launch_batched(full_a, G, ctx->stream));
    if ((rc = batched_reduce_scalars(ctx, K, ctx->batch_wg_off_d, 0))) return rc;
    HIP_TRY(ctx, launch_vi_finish(l, it, ctx->stream));
  }
  ctx->svi_t += (uint64_t)iters;
  return vi_loop_out(ctx, iters, total, trace, n_done, status);      // (tables and rows are host memory: alive up to this wait)
  });
}

extern "C" {

int mimo_vi_prior_batched(mimo_ctx* ctx, int K, const double* alpha0, const double* pa, const double* pb, const double* pc,
                          const double* pd, const double* prior_logZ) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_vi_prior_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (!alpha0 || !pa || !pb || !pc || !pd || !prior_logZ)
    return fail(ctx, MIMO_E_INVALID, "%s: alpha0, pa, pb, pc, pd and prior_logZ must be non-NULL", me);
  const size_t k = (size_t)K, D = (size_t)ctx->D;
  const ViPart parts[6] = {{"alpha0", alpha0, k, 0}, {"pa", pa, k * D, 0}, {"pb", pb, k, 0}, {"pc", pc, k * D * D, 0},
                           {"pd", pd, k, 0}, {"prior_logZ", prior_logZ, k, 0}};
  return vi_install_prior(ctx, K, kViFamilies[kViGmm], parts, 6, 0, 0, 0, me);
  });
}

int mimo_vi_run_batched(mimo_ctx* ctx, int K, int iters, double tol, int flags, double* trace, int32_t* n_done, int32_t* status) {
  return vi_run(ctx, K, iters, tol, flags, trace, n_done, status, "mimo_vi_run_batched", kViFamilies[kViGmm]);
}

int mimo_vi_get_batched(mimo_ctx* ctx, int K, double* out) { return vi_get(ctx, K, out, "mimo_vi_get_batched", kViFamilies[kViGmm]); }

int mimo_vi_get_theta_batched(mimo_ctx* ctx, int K, double* theta, double* stats) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_vi_get_theta_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (!theta && !stats) return fail(ctx, MIMO_E_INVALID, "%s: theta and stats are both NULL", me);
  if ((rc = vi_ready(ctx, K, me, nullptr))) return rc;
  if (stats && (!ctx->batch_stats_valid || ctx->batch_stats_K != K || !ctx->S_d))
    return fail(ctx, MIMO_E_STATE, "%s: no statistics of K = %d are resident", me, K);
  const size_t B = (size_t)ctx->batch_B;
  if (theta) HIP_TRY(ctx, hipMemcpyAsync(theta, ctx->vi_theta, image_len(ctx, K) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (stats)
    HIP_TRY(ctx, hipMemcpyAsync(stats, ctx->S_d, (batch_stats_len(ctx, K) + 3 * B) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}

int mimo_vi_ilr_prior_batched(mimo_ctx* ctx, int K, int dx, int dy, int gating_kind, const double* g0, const double* g1,
                              const double* pa, const double* pb, const double* pc, const double* pd, const double* basis_logZ,
                              const double* ma, const double* mb, const double* mc, const double* md, const double* experts_logZ) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_vi_ilr_prior_batched";
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if (gating_kind != MIMO_VI_GATING_DIRICHLET && gating_kind != MIMO_VI_GATING_STICK_BREAKING)
    return fail(ctx, MIMO_E_INVALID, "%s: gating_kind = %d is neither MIMO_VI_GATING_DIRICHLET nor MIMO_VI_GATING_STICK_BREAKING", me,
                gating_kind);
  if (dx < 1 || dy < 1 || dx + dy != ctx->D)
    return fail(ctx, MIMO_E_INVALID, "%s: dx = %d and dy = %d must be >= 1 and add up to the uploaded Dz = %d", me, dx, dy, ctx->D);
  const bool stick = gating_kind == MIMO_VI_GATING_STICK_BREAKING;
  if (!g0 || (stick && !g1) || !pa || !pb || !pc || !pd || !basis_logZ || !ma || !mb || !mc || !md || !experts_logZ)
    return fail(ctx, MIMO_E_INVALID, "%s: g0, (stick-breaking: g1,) the basis' pa, pb, pc, pd, basis_logZ and the experts' ma, mb, mc, "
                "md, experts_logZ must be non-NULL", me);
  const size_t k = (size_t)K, sx = (size_t)dx, sy = (size_t)dy, sc = sx + 1;
  const std::vector<double> zeros(stick ? 0 : (size_t)ctx->batch_B * k, 0.0);      // (a Dirichlet gating has no second part)
  const ViPart parts[12] = {{"g0", g0, k, 0}, {"g1", stick ? g1 : zeros.data(), k, 0},
                            {"pa", pa, k * sx, 0}, {"pb", pb, k, 0}, {"pc", pc, k * sx * sx, 0}, {"pd", pd, k, 0},
                            {"basis_logZ", basis_logZ, k, 0},
                            {"ma", ma, k * sy * sc, 0}, {"mb", mb, k * sc * sc, 0}, {"mc", mc, k * sy * sy, 0}, {"md", md, k, 0},
                            {"experts_logZ", experts_logZ, k, 0}};
  return vi_install_prior(ctx, K, kViFamilies[kViIlr], parts, 12, dx, dy, stick ? kViGatingStick : kViGatingDirichlet, me);
  });
}

int mimo_vi_ilr_run_batched(mimo_ctx* ctx, int K, int iters, double tol, int flags, double* trace, int32_t* n_done, int32_t* status) {
  return vi_run(ctx, K, iters, tol, flags, trace, n_done, status, "mimo_vi_ilr_run_batched", kViFamilies[kViIlr]);
}

int mimo_vi_ilr_get_batched(mimo_ctx* ctx, int K, double* out) {
  return vi_get(ctx, K, out, "mimo_vi_ilr_get_batched", kViFamilies[kViIlr]);
}

int mimo_svi_state_batched(mimo_ctx* ctx, int K, const double* alpha, const double* qa, const double* qb, const double* qc,
                           const double* qd, int32_t* status) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_svi_state_batched";
  const ViFamily& f = kViFamilies[kViGmm];
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if ((rc = vi_ready(ctx, K, me, &f))) return rc;
  const ViLayout L{K, ctx->D};
  const ViNwLayout N = L.nw();
  const size_t k = (size_t)K, D = (size_t)ctx->D;
  const ViPart parts[5] = {{"alpha", alpha, k, (size_t)L.alpha()}, {"qa", qa, k * D, (size_t)N.qa()}, {"qb", qb, k, (size_t)N.qb()},
                           {"qc", qc, k * D * D, (size_t)N.qc()}, {"qd", qd, k, (size_t)N.qd()}};
  return svi_state(ctx, K, parts, 5, status, me, f);
  });
}

int mimo_svi_ilr_state_batched(mimo_ctx* ctx, int K, const double* g0, const double* g1, const double* qa, const double* qb,
                               const double* qc, const double* qd, const double* ma, const double* mKq, const double* mc,
                               const double* md, int32_t* status) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_svi_ilr_state_batched";
  const ViFamily& f = kViFamilies[kViIlr];
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = batched_ready(ctx, K, me))) return rc;
  if ((rc = vi_ready(ctx, K, me, &f))) return rc;
  const ViIlrLayout L{K, ctx->vi_dx, ctx->vi_dy};
  const ViNwLayout N = L.basis();
  const size_t k = (size_t)K, dx = (size_t)ctx->vi_dx, dy = (size_t)ctx->vi_dy, dc = dx + 1;
  const bool stick = ctx->vi_gating == kViGatingStick;
  const std::vector<double> zeros(stick ? 0 : (size_t)ctx->batch_B * k, 0.0);      // (a Dirichlet gating has no second part)
  const ViPart parts[10] = {{"g0", g0, k, (size_t)L.g0()}, {"g1", stick ? g1 : zeros.data(), k, (size_t)L.g1()},
                            {"qa", qa, k * dx, (size_t)N.qa()}, {"qb", qb, k, (size_t)N.qb()},
                            {"qc", qc, k * dx * dx, (size_t)N.qc()}, {"qd", qd, k, (size_t)N.qd()},
                            {"ma", ma, k * dy * dc, (size_t)L.m_a()}, {"mKq", mKq, k * dc * dc, (size_t)L.m_Kq()},
                            {"mc", mc, k * dy * dy, (size_t)L.m_c()}, {"md", md, k, (size_t)L.m_d()}};
  return svi_state(ctx, K, parts, 10, status, me, f);
  });
}

int mimo_svi_run_batched(mimo_ctx* ctx, int K, int iters, double step_size, const double* scale, const int64_t* rows,
                         const int64_t* sel_off, const uint64_t* seeds, int flags, double* trace, int32_t* n_done, int32_t* status) {
  return svi_run(ctx, K, iters, step_size, scale, rows, sel_off, seeds, flags, trace, n_done, status, "mimo_svi_run_batched",
                 kViFamilies[kViGmm]);
}

int mimo_svi_ilr_run_batched(mimo_ctx* ctx, int K, int iters, double step_size, const double* scale, const int64_t* rows,
                             const int64_t* sel_off, const uint64_t* seeds, int flags, double* trace, int32_t* n_done,
                             int32_t* status) {
  return svi_run(ctx, K, iters, step_size, scale, rows, sel_off, seeds, flags, trace, n_done, status, "mimo_svi_ilr_run_batched",
                 kViFamilies[kViIlr]);
}

}  // extern "C"

extern "C" {

// ------------------------------------------------------------------------------------------
// Batched prediction (mimo_predict_batched.hip)
// ------------------------------------------------------------------------------------------
// The rows are an argument: nothing of the context's data, batch or kept tables is read or written.  Buffers: the parameter,
// transform and row_off blocks go through the operand image's pinned staging buffer in ONE transfer (theta_h -> theta_d, restaged
// by every pass); X and y go through the staged-weights workspace `win`, as mimo_predict_flags uses it (pure staging: nothing
// resident lives there, so nothing is invalidated); the outputs are one block of S_d / S_h (ensure_block / hand_out), which drops
// the resident statistics of a batched pass (batch_stats_valid: mimo_vi_run_batched then asks for a new pass).
int mimo_predict_batched(mimo_ctx* ctx, int B, const double* X, const int64_t* row_off, int64_t N_shared, int dx,
                         const double* x_tf, const double* c, const double* b, const double* W, int K,
                         const double* M, const double* Q, const double* Cc, int dy, int mode,
                         const double* y, const double* y_tf, const double* P, const double* ld,
                         double* mu, double* covar, double* nlpd, int flags) {
  return guarded(ctx, [&]() -> int {
  const char* const me = "mimo_predict_batched";
  int rc = bind(ctx); if (rc) return rc;
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (ctx->comm)
    return fail(ctx, MIMO_E_UNSUPPORTED, "%s: a communicator is attached (mimo_comm_init); the batched pass has no ranks", me);
  if (flags & ~MIMO_F_DIAG_VAR)
    return fail(ctx, MIMO_E_INVALID, "%s: flags 0x%x: only MIMO_F_DIAG_VAR (host pointers throughout)", me, flags);
  if (!c || !b || !W || !M || !Q || !Cc || !mu || !covar)
    return fail(ctx, MIMO_E_INVALID, "%s: c, b, W, M, Q, Cc, mu and covar must be non-NULL", me);
  if (B < 1 || K < 1 || (mode != 0 && mode != 1))
    return fail(ctx, MIMO_E_INVALID, "%s: B = %d, K = %d must be >= 1 and mode = %d must be 0 or 1", me, B, K, mode);
  if (!predict_batched_covers(dx, dy) || B > kPredictBatchedMaxB)
    return fail(ctx, MIMO_E_UNSUPPORTED, "%s: dx = %d, dy = %d, B = %d outside the batched prediction kernel (affine experts, "
                "1 <= dx <= %d, 1 <= dy <= %d, B <= %d)", me, dx, dy, B, kPredictBatchedMaxDx, kPredictBatchedMaxDy, kPredictBatchedMaxB);
  if (N_shared < 0) return fail(ctx, MIMO_E_INVALID, "%s: N_shared = %lld is negative", me, (long long)N_shared);
  if (row_off && N_shared != 0)
    return fail(ctx, MIMO_E_INVALID, "%s: row_off and N_shared = %lld are both given (ragged form: N_shared = 0; shared form: "
                "row_off = NULL)", me, (long long)N_shared);
  int64_t max_rows = N_shared;
  if (row_off) {
    if ((rc = check_offsets(ctx, row_off, B, me, "row_off"))) return rc;
    for (int p = 0; p < B; ++p) max_rows = std::max<int64_t>(max_rows, row_off[p + 1] - row_off[p]);
  }
  const bool want_nlpd = nlpd != nullptr, diag = (flags & MIMO_F_DIAG_VAR) != 0;
  if (want_nlpd && (!y || !P || !ld)) return fail(ctx, MIMO_E_INVALID, "%s: nlpd needs y, P and ld", me);
  if (y_tf && !y) return fail(ctx, MIMO_E_INVALID, "%s: y_tf without y", me);
  const int dd[2] = {dx, dy};
  const double* const tfs[2] = {x_tf, y_tf};
  for (int t = 0; t < 2; ++t)
    for (int p = 0; tfs[t] && p < B; ++p)
      for (int i = 0; i < dd[t]; ++i) {
        const double s = tfs[t][((size_t)p * 2 + 1) * dd[t] + i];
        if (s == 0.0 || !std::isfinite(s))
          return fail(ctx, MIMO_E_INVALID, "%s: %s of problem %d: scale[%d] = %g must be finite and nonzero", me, t ? "y_tf" : "x_tf", p, i, s);
      }
  const size_t n_in = (size_t)(row_off ? row_off[B] : N_shared);        // rows of X (and y)
  const size_t n_out = row_off ? n_in : (size_t)N_shared * (size_t)B;   // rows of the outputs
  if (max_rows == 0) return MIMO_OK;                                    // an all-empty batch: nothing to launch
  if (!X) return fail(ctx, MIMO_E_INVALID, "%s: X is NULL", me);

  // one staged block: [gate (c, b, W interleaved per component) | M | Q | Cc | P | ld | x_tf | y_tf | row_off]
  const int dc = dx + 1;
  const size_t BK = (size_t)B * K, gk = 1 + (size_t)dx + (size_t)dx * dx;
  const size_t ng = BK * gk, nM = BK * dy * dc, nQ = BK * dc * dc, nC = BK * dy * dy;
  const size_t nxt = x_tf ? (size_t)B * 2 * dx : 0, nyt = y_tf ? (size_t)B * 2 * dy : 0, nro = row_off ? (size_t)B + 1 : 0;
  const size_t nparam = ng + nM + nQ + 2 * nC + BK + nxt + nyt + nro;
  if ((rc = ctx->theta_d.ensure(ctx, nparam))) return rc;
  if ((rc = ctx->theta_h.ensure(ctx, nparam))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));    // the staging buffer may still be in flight from the previous call on this stream
  double* q = ctx->theta_h;
  for (size_t k = 0; k < BK; ++k) {
    *q++ = c[k];
    memcpy(q, b + k * dx, sizeof(double) * dx); q += dx;
    memcpy(q, W + k * dx * dx, sizeof(double) * dx * dx); q += (size_t)dx * dx;
  }
  memcpy(q, M, sizeof(double) * nM); q += nM;
  memcpy(q, Q, sizeof(double) * nQ); q += nQ;
  memcpy(q, Cc, sizeof(double) * nC); q += nC;
  if (want_nlpd) { memcpy(q, P, sizeof(double) * nC); memcpy(q + nC, ld, sizeof(double) * BK); }
  else memset(q, 0, sizeof(double) * (nC + BK));
  q += nC + BK;
  if (nxt) { memcpy(q, x_tf, sizeof(double) * nxt); q += nxt; }
  if (nyt) { memcpy(q, y_tf, sizeof(double) * nyt); q += nyt; }
  if (nro) memcpy(q, row_off, sizeof(int64_t) * nro);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->theta_d, ctx->theta_h, nparam * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

  // the rows: X, then y
  const size_t nX = n_in * dx, nY = want_nlpd ? n_in * dy : 0;
  if ((rc = ctx->win.ensure(ctx, nX + nY))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->win, X, nX * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (nY) HIP_TRY(ctx, hipMemcpyAsync(ctx->win + nX, y, nY * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

  // the outputs: [mu | second output | nlpd], one block
  const size_t ncov = diag ? 2 * (size_t)dy : (size_t)dy * dy;
  const size_t n_mu = n_out * dy, n_cov = n_out * ncov, n_nl = want_nlpd ? n_out : 0, out = n_mu + n_cov + n_nl;
  if ((rc = ensure_block(ctx, out))) return rc;

  PredictBatchedArgs a{};
  const double* d = ctx->theta_d;
  a.X = ctx->win; a.N_shared = row_off ? 0 : N_shared;
  a.B = B; a.dx = dx; a.dy = dy; a.K = K; a.mode = mode; a.diag = diag ? 1 : 0;
  a.gate = d; a.M = d + ng; a.Q = a.M + nM; a.Cc = a.Q + nQ; a.P = a.Cc + nC; a.ld = a.P + nC;
  const double* tail = a.ld + BK;
  a.x_tf = nxt ? tail : nullptr; tail += nxt;
  a.y_tf = nyt ? tail : nullptr; tail += nyt;
  a.row_off = nro ? reinterpret_cast<const int64_t*>(tail) : nullptr;
  a.y = want_nlpd ? ctx->win + nX : nullptr;
  a.mu = ctx->S_d; a.covar = ctx->S_d + n_mu; a.nlpd = want_nlpd ? ctx->S_d + n_mu + n_cov : nullptr;
  if ((rc = TIMED_HIP(ctx, "predict_batched_kernel", launch_predict_batched(a, max_rows, ctx->stream)))) return rc;
  if (ctx->prof) ctx->prof_n += 1;
  if ((rc = hand_out(ctx, out, mu, n_mu, covar, n_mu, n_cov))) return rc;
  if (want_nlpd) memcpy(nlpd, ctx->S_h + n_mu + n_cov, n_nl * sizeof(double));
  return MIMO_OK;
  });
}

}  // extern "C"
