// What the two halves of the C-ABI layer share: mimo_abi.cpp (single-problem entry points, routing, profiling) and
// mimo_abi_batched.cpp (batched passes, resident VI, batched prediction).  The context, its buffers, the guards every entry point
// runs under, the staging templates, and the helpers of mimo_abi.cpp that the batched half calls.  Not installed; the public
// surface is include/mimo_hip.h.
#pragma once
#include "../../include/mimo_hip.h"
#include "mimo_batched.h"
#include "mimo_theta.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

struct mimo_ctx;

// Defined in mimo_abi.cpp.  Hidden: none of them is part of the library's dynamic symbol table.
namespace mimo_abi {
#pragma GCC visibility push(hidden)
int fail(mimo_ctx* ctx, int code, const char* fmt, ...);
int bind(mimo_ctx* ctx);
size_t packed_len(int K, int D);                  // doubles of a packed statistics block: K x (n, sum z, sum z z^T)
size_t partial_stride(int K16, int F16);          // doubles of one workgroup's partial block
int64_t table_rows(const mimo_ctx* ctx);
int ensure_block(mimo_ctx* ctx, size_t len);
int hand_out(mimo_ctx* ctx, size_t copy_len, double* S, size_t nstats, double* scalars, size_t scalars_at, size_t nscalars);
int copy_out(mimo_ctx* ctx, void* dst, const void* src, size_t bytes, bool valid, const char* what);
int theta_fail(mimo_ctx* ctx, const mimo::ThetaFail& f, const char* what, int p);
int prof_slot(mimo_ctx* ctx, const char* name);
int set_data(mimo_ctx* ctx, int64_t N, int Dz);
enum class Rows { HostCopy, DeviceBorrow, DeviceCopy };
int set_rows(mimo_ctx* ctx, const double* src, Rows how);
#pragma GCC visibility pop
}  // namespace mimo_abi

#define HIP_TRY(ctx, expr)                                                                \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return mimo_abi::fail(ctx, MIMO_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// One owner per allocation: device memory (hipMalloc), or with Pinned its host sibling (hipHostMalloc).  Reads as the pointer it holds.
template <typename T, bool Pinned = false>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;     // elements
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { (void)release(); }
  operator T*() const { return p; }
  // free and forget in one step: the pointer is gone whatever the runtime answers, so nothing is freed twice
  hipError_t release() {
    T* old = p;
    p = nullptr; cap = 0;
    return !old ? hipSuccess : Pinned ? hipHostFree(old) : hipFree(old);
  }
  // room for `count` elements, at least one (an empty data set still gets an allocation).  Grows only; the contents do not survive
  // a growth (the old block is freed before the new one is allocated); a HIP error goes to the context's error buffer.
  int ensure(mimo_ctx* ctx, size_t count) {
    if (count < 1) count = 1;
    if (cap >= count && p) return MIMO_OK;
    HIP_TRY(ctx, release());
    if (Pinned) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault));
    else HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
    cap = count;
    return MIMO_OK;
  }
};

struct mimo_ctx {
  int device = 0;
  int num_cu = 256;       // what the grids are sized from (mimo_tune "num_cu" overrides it for tests)
  int hw_num_cu = 256;
  int resp_skip_log2 = 60;  // fused softmax pass: statistics skip the row blocks whose weights are all < 2^-60 (0: dense)
  hipStream_t own_stream = nullptr;
  ~mimo_ctx() { if (own_stream) (void)hipStreamDestroy(own_stream); }     // (the buffers below free themselves after it)
  hipStream_t stream = nullptr;
  char err[512] = {0};   // fixed buffer: reporting an error never allocates

  // data
  const double* Z = nullptr;  // device
  Buf<double> Z_owned;       // the library's copy of the rows (Z points at it, or at the caller's attached rows)
  int64_t N = 0;
  int D = 0;
  int64_t row0 = 0;

  // feature map for the current D and structure (0: full symmetric W, 1: diagonal W)
  int structure = 0;
  int feat_structure = -1;
  int feat_D = -1;
  int F = 0, F16 = 0;
  std::vector<uint8_t> feat_h;
  Buf<uint8_t> feat_d;
  Buf<uint8_t> feat_full_d;         // full map of the current D (small-shape kernel under a structure hint)
  int feat_full_D = -1;

  // parameter image
  Buf<double> theta_d;
  Buf<double, true> theta_h;  // pinned staging

  // slot order of the components in the fused mean-field pass (mimo_set_component_order); order_K = 0: the identity
  int block_order_on = [] { const char* e = getenv("MIMO_BLOCK_ORDER"); return !e || atoi(e) != 0; }();   // mimo_tune "block_order"
  int order_K = 0;
  alignas(8) int32_t order[256] = {0};                    // order[s] = the component in slot s
  const int32_t* pass_order = nullptr;                    // the pass being launched runs under the order: its device copy (behind the Theta image)

  // per-row certificates of the fused mean-field E-step ("E-step certificates"; mimo_tune "estep_cert").  They
  // exist for the pass that runs the skipping kernel under a component order at K16 = 4, and are allocated by its first reference pass.
  int cert_on = [] { const char* e = getenv("MIMO_ESTEP_CERT"); return !e || atoi(e) != 0; }();
  bool cert_valid = false;                                // cert_k / cert_m / cert_a hold a reference pass of the resident rows, and:
  int cert_K = 0, cert_skip = 0;                          //   its K and resp_skip_log2
  int cert_age = 0;                                       //   certified passes since
  std::vector<double> cert_ref;                           //   what the certificate constants need of its parameters (mimo_host_estep_certificate_ref)
  int32_t cert_order[64] = {0};                           //   its slot order
  uint64_t cert_part[4] = {0, 0, 0, 0};                   //   its partition into row blocks: the blocks' component sets, ascending
  uint64_t cert_prev_part[4] = {0, 0, 0, 0};              // the partition of the last eligible pass, and its K (0: none)
  int cert_prev_K = 0;
  int cert_last = 0;                                      // kind of the last mimo_estep (mimo::Cert)
  Buf<uint8_t> cert_k;                                    // (N,) the three per-row arrays (KernelArgs)
  Buf<double> cert_m, cert_a;
  Buf<unsigned long long> cert_cnt;                       // [4] running totals of the certified passes (KernelArgs::cert_cnt)

  // workspaces
  Buf<double> partials;
  Buf<double> reduced;
  Buf<double> S_d;            // packed stats + 3 scalars
  Buf<double, true> S_h;      // pinned staging

  // optional device-resident tables
  Buf<double> resp;  int resp_K = 0;  bool resp_valid = false;
  Buf<double> logp;  int logp_K = 0;  bool logp_valid = false;
  Buf<double> lse;   bool lse_valid = false;
  Buf<int32_t> labels;  bool labels_valid = false;
  Buf<double> u_d;
  bool weights_resident = false;     // u_d holds the row weights of the last mimo_estep_weighted (not uniforms of a label pass)
  Buf<double> win;    // staged host weights
  Buf<int32_t> lin;   // staged host labels

  // rows with missing values (NaN): zeroed in the owned copy, excluded from every statistic through the mask
  Buf<double> row_mask;                                   // (N,) 1 = complete row
  int64_t n_bad = 0;
  Buf<unsigned long long> cnt_d;                          // [kCntWords]: scan count, labels drawn on NaN rows per component, content checksum of the upload
  uint64_t data_sum[2] = {0, 0};                          // mimo_data_checksum: the rows as mimo_upload received them
  bool data_sum_valid = false;
  Buf<int32_t> labels_tmp;
  Buf<uint32_t> ls_aux;                                    // label histogram + slot table of label_stats_slots_kernel
  Buf<uint16_t> sort_list;   // tiles ranked once for a multi-launch label-statistics pass (label_tile_sort_kernel)
  Buf<uint16_t> sort_start;
  Buf<double> table_tmp;
  int bad_counts_K = 0;         // > 0: cnt_d[kCntLabels ..] holds the label counts of the NaN rows of the last label pass

  // batched mode (mimo_upload_batched): Z holds the rows of B problems back to back; the single-problem entry points refuse
  bool batched = false;
  int batch_B = 0;
  int batch_G = 0;                                         // workgroups of the work table
  std::vector<int64_t> batch_rows;                         // host copy of row_off [B + 1]
  Buf<int64_t> batch_row_off_d;                            // [B + 1]
  Buf<mimo::BatchedWork> batch_work_d;                     // [G]
  Buf<int32_t> batch_wg_off_d;                             // [B + 1]: problem b owns the workgroups [wg_off[b], wg_off[b + 1])
  // shared batch (mimo_upload_batched_shared): Z holds ONE block of N rows that all B problems read; every per-problem buffer
  // (lse, labels, weights, uniforms, tables) still has row_off[B] = B N rows — table_rows() — while ctx->N counts the data rows
  bool batch_shared = false;
  Buf<double> batch_w;                                     // [row_off[B]] per-row weights of mimo_estep_batched_weighted / mimo_outer_resp_batched
  bool batch_w_valid = false;
  // S_d holds the statistics [B][K][1 + Dz + Dz^2] of a batched pass with K = batch_stats_K, its 3 B scalars behind them: set by
  // every batched pass that reduces statistics, cleared wherever the block is handed to something else (ensure_block)
  bool batch_stats_valid = false;
  int batch_stats_K = 0;
  // device-resident batched VI (mimo_vi_batched.hip); the prior block, and with it the loop state, lives from mimo_vi_prior_batched
  // to the next upload
  bool vi_prior_valid = false;
  int vi_K = 0;
  // which family's prior block is resident: 0 mixtures of Gaussians (the layouts below), 1 mixtures of linear-Gaussian experts
  // (mimo_vi_ilr_batched.h: ViIlrArgs / ViIlrLayout in the same buffers), with its dx, dy and gating kind
  int vi_family = 0;
  int vi_dx = 0, vi_dy = 0, vi_gating = 0;
  Buf<double> vi_prior;                                    // [alpha0 B K | pa B K D | pb B K | pc B K D D | pd B K | log Z B K]
  Buf<double> vi_post;                                     // [2][B][ViLayout::count()]
  Buf<double> vi_work;                                     // [terms B K | prior terms B | last bound B]
  Buf<double> vi_theta;                                    // [B][K16][F16 / 4][64]: the operand images the loop's passes read
  Buf<double> vi_loop;                                     // [words: kViWords B int32, padded to doubles | trace of the last call]
  Buf<double, true> vi_loop_h;                             // its pinned sibling
  // device-resident batched SVI (mimo_svi_state_batched / mimo_svi_run_batched) on the loop above: the state lives from its upload
  // to the next prior block or upload
  bool svi_state_valid = false;
  uint64_t svi_t = 0;                                      // iterations since the state upload: the index kernel's Philox counter
  Buf<int64_t> svi_sel;                                    // [selections of a call][sel_off[B]]: the minibatch indices
  Buf<uint64_t> svi_tables;                                // [sel_off B + 1 | work table | wg_off | seeds B | 1 / scale B] of a call

  void* comm = nullptr;         // RCCL communicator (mimo_comm_init): every pass then returns statistics summed over the ranks
  int comm_world = 1;

  // pending asynchronous call (MIMO_F_ASYNC)
  bool pending_async = false;
  size_t pending_slen = 0;
  bool pending_stats = false;

  // profiling: HIP events around every kernel of a pass, on the launch stream
  bool prof = false;
  struct ProfEvent { hipEvent_t e0, e1; int name; };
  std::vector<ProfEvent> pending;
  static constexpr int kProfNames = 16;
  const char* prof_name[kProfNames] = {nullptr};
  double prof_name_ms[kProfNames] = {0.0};
  int64_t prof_name_n[kProfNames] = {0};
  double prof_ms = 0.0;      // all kernels
  int64_t prof_n = 0;        // passes (run_fused calls)
};

// The templates both halves instantiate; static, so each translation unit keeps its own copies
namespace mimo_abi {

// Every extern "C" entry point runs inside this guard: no C++ exception crosses the boundary (include/mimo_hip.h).
// std::bad_alloc (the std::vector staging buffers, the event list of the profiler) -> MIMO_E_NOMEM, anything else ->
// MIMO_E_INTERNAL; the message goes to the fixed error buffer, so the handlers themselves cannot throw.
template <typename F>
static int guarded(mimo_ctx* ctx, F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(ctx, MIMO_E_NOMEM, "out of host memory");
  } catch (const std::exception& e) {
    return fail(ctx, MIMO_E_INTERNAL, "internal error: %s", e.what());
  } catch (...) {
    return fail(ctx, MIMO_E_INTERNAL, "internal error: unknown exception");
  }
}

// The images of B problems' (c, b, W) back to back in the placement `pl`, followed by `nextra` uint64 words and then `nextra2` more
// (copied in the same transfer), on the device at ctx->theta_d.  `what`: the batched entry point (its name leads the error texts), null for a single
// problem.  inline_img: the image goes there and nowhere else — no staging buffer to wait for, no transfer to enqueue.
template <typename Placement>
static int stage_theta(mimo_ctx* ctx, const Placement& pl, const double* c, const double* b, const double* W, int B,
                       const uint64_t* extra, size_t nextra, const char* what, double* inline_img = nullptr,
                       const uint64_t* extra2 = nullptr, size_t nextra2 = 0) {
  const size_t D = ctx->D, K = pl.K, per = pl.count(), total = per * B + nextra + nextra2;
  int rc;
  if (!inline_img) {
    if ((rc = ctx->theta_d.ensure(ctx, total))) return rc;
    if ((rc = ctx->theta_h.ensure(ctx, total))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));    // the staging buffer may still be in flight from the previous call on this stream
  }
  double* img = inline_img ? inline_img : ctx->theta_h;
  for (int p = 0; p < B; ++p) {
    const mimo::ThetaFail f = mimo::pack_theta(pl, ctx->structure, c + p * K, b + p * K * D, W + p * K * D * D, img + per * p);
    if (f.kind) return theta_fail(ctx, f, what, p);
  }
  if (nextra) memcpy(img + per * B, extra, nextra * sizeof(uint64_t));
  if (nextra2) memcpy(img + per * B + nextra, extra2, nextra2 * sizeof(uint64_t));
  if (!inline_img) HIP_TRY(ctx, hipMemcpyAsync(ctx->theta_d, img, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return MIMO_OK;
}

// launch() bracketed by two events on the context's stream when profiling is on
template <typename L>
static int timed_launch(mimo_ctx* ctx, const char* name, L&& launch) {
  if (!ctx->prof) return launch();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(ctx, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return fail(ctx, MIMO_E_HIP, "hipEventCreate failed"); }
  (void)hipEventRecord(e0, ctx->stream);
  const int rc = launch();
  (void)hipEventRecord(e1, ctx->stream);
  if (rc != MIMO_OK) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; }
  ctx->pending.push_back({e0, e1, prof_slot(ctx, name)});
  return MIMO_OK;
}
// (a single launch under its profile name)
#define TIMED_HIP(ctx, name, expr) timed_launch(ctx, name, [&]() -> int { HIP_TRY(ctx, expr); return MIMO_OK; })

// What an entry point reads when the caller passes NULL for an input: the context's own copy `p` if `valid`, else MIMO_E_STATE
// with the entry point's text `missing` (it may print K).  No `missing`: the input is optional and NULL stays NULL.
template <typename T>
struct Resident { const T* p = nullptr; bool valid = false; const char* missing = nullptr; };

// Bring one input of `count` elements to the device and say where to read it (*dev): NULL is the resident copy, under
// MIMO_F_DEVICE_IN the caller's pointer is the device's already, anything else is host memory and goes through `staging` (*copied
// becomes true).  The copy is only enqueued: the source is pageable, so the entry point synchronises once all its inputs are
// queued, and does what else follows from a fresh staging buffer there.
// (P: const T* or T* — KernelArgs holds its tables and labels as writable pointers for the kernels that produce them)
template <typename T, typename P>
static int stage_input(mimo_ctx* ctx, const T* src, size_t count, int flags, Buf<T>& staging, const Resident<T>& res, int K,
                       P* dev, bool* copied) {
  if (!src) {
    if (res.missing && !res.valid) return fail(ctx, MIMO_E_STATE, res.missing, K);
    *dev = const_cast<P>(res.p);
  } else if (flags & MIMO_F_DEVICE_IN) {
    *dev = const_cast<P>(src);
  } else {
    const int rc = staging.ensure(ctx, count);
    if (rc) return rc;
    if (count) HIP_TRY(ctx, hipMemcpyAsync(staging, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *dev = staging;
    *copied = true;
  }
  return MIMO_OK;
}

}  // namespace mimo_abi
