// C-ABI layer of libmimo_hip.so (see include/mimo_hip.h for the contract and the reference
// call sites each entry point replaces).  Host-side work here is O(K D^2): converting the
// canonical (c, b, W) parameters to the feature-space MFMA operand image, and launching /
// sequencing the gfx950 kernels of mimo_kernels.hip on the context's stream.
// The batched entry points live in mimo_abi_batched.cpp; what the two files share is mimo_abi_internal.h.
#include "mimo_abi_internal.h"
#include "mimo_kernels.h"
#include "mimo_extra.h"
#include "mimo_route.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

using namespace mimo;
using namespace mimo_abi;

namespace mimo_comm {      // mimo_comm.cpp (RCCL through dlopen)
int unique_id(char* out128, char* msg, size_t msglen);
int init(void** comm, const char* id128, int rank, int world, char* msg, size_t msglen);
int destroy(void* comm);
int allreduce_sum_f64(void* comm, double* buf, size_t count, hipStream_t stream, char* msg, size_t msglen);
}

// cnt_d: [scan count | labels drawn on NaN rows per component (256) | content checksum of the upload (2)]
constexpr int kCntLabels = 1, kCntChecksum = 257, kCntWords = 259;

static char g_err[512] = {0};

// feature-tile row padding (doubles); MIMO_RS_PAD overrides for bank-conflict experiments
static int rs_pad() {
  static const int v = [] { const char* e = getenv("MIMO_RS_PAD"); return e ? atoi(e) : 1; }();
  return v;
}
// weight-tile row padding (doubles); MIMO_LS_PAD overrides for bank-conflict experiments
// (default 2; 1 for the Dz >= 14, 49 <= K <= 64 shapes of the single-pass kernels — C2: kernel 6.62 -> 6.57 ms, measured with
//  tools/pad_sweep.sh; elsewhere 1 and 2 are within +-2 % of each other, tools/pad_shapes.sh)
static int ls_pad(int K16, int D) {
  static const int v = [] { const char* e = getenv("MIMO_LS_PAD"); return e ? atoi(e) : 0; }();
  return v > 0 ? v : (K16 == 4 && D >= 14 && D <= kMaxFusedD) ? 1 : 2;
}
#ifdef MIMO_STAMPS
static unsigned long long* g_stamps = nullptr;
static int g_stamps_grid = 0;
extern "C" int mimo_debug_stamps_grid() { return g_stamps_grid; }
extern "C" int mimo_debug_stamps_trace(unsigned long long* out128) {   // phase boundaries of workgroups 0 and grid / 2
  return hipMemcpy(out128, g_stamps + (size_t)3 * 8192 * 32, 128 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
static int g_stamps_sel = 0;                       // region: 0 fused / statistics, 1 chunked E-step, 2 wide E-step
extern "C" void mimo_debug_stamps_select(int sel) { g_stamps_sel = sel; }
extern "C" int mimo_debug_stamps(double* out8) {   // mean cycles per wave of each phase, last launch
  std::vector<unsigned long long> h((size_t)g_stamps_grid * 32);
  if (hipMemcpy(h.data(), g_stamps + (size_t)g_stamps_sel * 8192 * 32, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int i = 0; i < 8; ++i) out8[i] = 0;
  for (size_t w = 0; w < h.size() / 8; ++w) for (int i = 0; i < 8; ++i) out8[i] += (double)h[w * 8 + i];
  for (int i = 0; i < 8; ++i) out8[i] /= (double)(h.size() / 8);
  return 0;
}
#endif

int mimo_abi::fail(mimo_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  memcpy(ctx ? ctx->err : g_err, buf, sizeof buf);
  return code;
}

int mimo_abi::bind(mimo_ctx* ctx) {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return MIMO_OK;
}

// doubles of a packed statistics block: K x (n, sum z, sum z z^T)
size_t mimo_abi::packed_len(int K, int D) { return (size_t)K * (1 + D + (size_t)D * D); }
// doubles of one workgroup's partial block: K16 row blocks of 16 components x F16 features, and the scalars behind them
size_t mimo_abi::partial_stride(int K16, int F16) { return (size_t)16 * K16 * F16 + 4; }

// feature table for dimension D: pairs (a,b), a <= b <= D over z~ = [z, 1]; padding -> (D+1,D+1)
static int prepare_features(mimo_ctx* ctx, int D) {
  if (ctx->feat_D == D && ctx->feat_structure == ctx->structure) return MIMO_OK;
  const int st = ctx->structure;
  ctx->F = st == MIMO_STRUCT_DIAG ? diag_feat_count(D) : st == MIMO_STRUCT_LINEAR ? lin_feat_count(D) : feat_count(D);
  ctx->F16 = (ctx->F + 15) / 16 * 16;
  ctx->feat_h.assign((size_t)ctx->F16 * 2, (uint8_t)(D + 1));
  for (int a = 0; a <= D; ++a)
    for (int b = a; b <= D; ++b) {
      const int f = struct_feat_index(st, D, a, b);
      if (f < 0) continue;
      ctx->feat_h[2 * f] = (uint8_t)a;
      ctx->feat_h[2 * f + 1] = (uint8_t)b;
    }
  int rc;
  HIP_TRY(ctx, ctx->feat_d.release());       // replaced wholesale: the table is as long as its map
  if ((rc = ctx->feat_d.ensure(ctx, ctx->feat_h.size()))) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->feat_d, ctx->feat_h.data(), ctx->feat_h.size(), hipMemcpyHostToDevice));
  ctx->feat_D = D;
  ctx->feat_structure = ctx->structure;
  if (D <= kSmallMaxD && ctx->feat_full_D != D) {
    uint8_t full[2 * 16];
    memset(full, D + 1, sizeof full);
    for (int aa = 0; aa <= D; ++aa)
      for (int bb = aa; bb <= D; ++bb) { full[2 * feat_index(D, aa, bb)] = (uint8_t)aa; full[2 * feat_index(D, aa, bb) + 1] = (uint8_t)bb; }
    if ((rc = ctx->feat_full_d.ensure(ctx, sizeof full))) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->feat_full_d, full, sizeof full, hipMemcpyHostToDevice));
    ctx->feat_full_D = D;
  }
  return MIMO_OK;
}

// Rows of the per-row buffers (lse, labels, weights, uniforms, the columns of a table): the data rows, except on a shared batch,
// whose B problems each own all N of them (row_off[B] = B N)
int64_t mimo_abi::table_rows(const mimo_ctx* ctx) {
  return ctx->batched ? ctx->batch_rows[(size_t)ctx->batch_B] : ctx->N;
}

// The single-problem entry points on a context that holds a batch (mimo_upload_batched)
static int single_only(mimo_ctx* ctx) {
  if (ctx->batched)
    return fail(ctx, MIMO_E_INVALID, "the context holds a batch of problems (mimo_upload_batched): single-problem calls need "
                "mimo_upload or mimo_attach first");
  return MIMO_OK;
}

static int check_shapes(mimo_ctx* ctx, int K) {
  if (single_only(ctx)) return MIMO_E_INVALID;
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (!ctx->Z) return fail(ctx, MIMO_E_NODATA, "no data uploaded or attached");
  if (K < 1) return fail(ctx, MIMO_E_INVALID, "K must be >= 1 (got %d)", K);
  if (K > 256) return fail(ctx, MIMO_E_UNSUPPORTED, "K = %d > 256 is not covered by the fused kernels", K);
  ctx->pass_order = nullptr;
  if (ctx->order_K != K) ctx->order_K = 0;       // a component order belongs to its K
  return MIMO_OK;
}

// Does this pass run under the context's component order?  The single-pass softmax + statistics request on the fused tile
// kernel at K <= 64 (resolve_fused: the kFastVI instantiations) and nothing else (include/mimo_hip.h).
static bool order_applies(const mimo_ctx* ctx, const Route& route, const KernelArgs& a) {
  return ctx->order_K == a.K && a.K16 <= 4 && route.family == Family::Fused && route.image == Image::Generic && !route.promoted &&
         a.do_stats && !a.gibbs && !a.split && !a.resp && !a.logp && !a.lse && !a.u && ctx->n_bad == 0;
}

// Per-row certificates of the fused mean-field E-step ("E-step certificates"): the kind of this pass — it runs
// under the context's component order (order_applies) — and, for a certified pass, the table it reads.  The policy is a function
// of the sequence of (K, order, parameters) the context has seen and of nothing the device reports, so every rank of a sharded
// run takes the same kind, and no delivered number depends on it:
//   certificates in force, whose partition into row blocks is this pass's, fewer than kCertRenew certified passes old -> certified
//   else the partition is the one of the previous such pass (it has stood for two passes)                             -> reference
//   else                                                                                                              -> plain
// (while the partition still moves, the clusters have not separated and a reference pass would be thrown away by the next one).
// kCertRenew: on the benchmark's fit a certificate proves 99.6 % of the rows one pass later and 94 % sixteen passes later
// (tests/test_estep_certificate_cpu.py); a reference pass costs what a plain pass costs.
static constexpr int kCertRenew = 16;
static constexpr double kCertEps = 1e-3;
static int cert_plan(mimo_ctx* ctx, const KernelArgs& a, const double* c, const double* b, const double* W, double* tab, int* kind) {
  *kind = kCertNone;
  const int K = a.K, D = ctx->D;
  if (!ctx->cert_on || a.resp_skip <= 0 || a.K16 != 4 || D < 14 || D > kMaxFusedD || ctx->structure != 0 || ctx->N < 1) return MIMO_OK;
  uint64_t part[4] = {0, 0, 0, 0};
  int32_t slot_of[64];
  for (int s = 0; s < K; ++s) { part[s >> 4] |= 1ull << ctx->order[s]; slot_of[ctx->order[s]] = s; }
  std::sort(part, part + 4);
  const bool stood = ctx->cert_prev_K == K && !memcmp(part, ctx->cert_prev_part, sizeof part);
  memcpy(ctx->cert_prev_part, part, sizeof part);
  ctx->cert_prev_K = K;
  if (ctx->cert_valid && (ctx->cert_K != K || ctx->cert_skip != a.resp_skip || memcmp(part, ctx->cert_part, sizeof part))) ctx->cert_valid = false;
  if (ctx->cert_valid && ctx->cert_age < kCertRenew) {
    double out[5 * 64 + 4], t[4 + 2 * 64];
    // (the reference's side was worked out, and its arrays scanned, when this block was stored below; c, b, W are scanned here: the
    // Theta packer, which validates them for the pass, runs behind this plan)
    if (mimo_host_estep_certificate_cur(K, D, ctx->cert_ref.data(), c, b, W, -0.6931471805599453 * a.resp_skip - kCertEps, out, t) == MIMO_OK) {
      memcpy(tab, t, 4 * sizeof(double));
      uint8_t* blk = reinterpret_cast<uint8_t*>(tab + 4 + 128);
      for (int s = 0; s < 64; ++s) {          // by the slot of the REFERENCE pass, which is what the rows' certificates name
        const int k = s < K ? ctx->cert_order[s] : -1;
        tab[4 + s] = k < 0 ? -1e300 : t[4 + k];
        tab[4 + 64 + s] = k < 0 ? 0.0 : t[4 + K + k];
        blk[s] = k < 0 ? 0 : (uint8_t)(slot_of[k] >> 4);
      }
      ctx->cert_age += 1;
      *kind = kCertCertified;
      return MIMO_OK;
    }
    ctx->cert_valid = false;                  // (a precision that is not positive definite: nothing to certify against)
  }
  if (!stood) return MIMO_OK;
  int rc;
  if ((rc = ctx->cert_k.ensure(ctx, (size_t)ctx->N)) || (rc = ctx->cert_m.ensure(ctx, (size_t)ctx->N)) || (rc = ctx->cert_a.ensure(ctx, (size_t)ctx->N))) return rc;
  if (!ctx->cert_cnt.p) {
    if ((rc = ctx->cert_cnt.ensure(ctx, 4))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->cert_cnt, 0, 4 * sizeof(unsigned long long), ctx->stream));
  }
  // what the certified passes need of this reference, once: a refused one (MIMO_E_INVALID) leaves a block that says so, and the
  // first certified pass drops the certificates
  ctx->cert_ref.resize(mimo_host_estep_certificate_ref_size(K, D));
  if ((rc = mimo_host_estep_certificate_ref(K, D, c, b, W, ctx->cert_ref.data())) != MIMO_OK && rc != MIMO_E_INVALID) return rc;
  memcpy(ctx->cert_order, ctx->order, K * sizeof(int32_t));
  memcpy(ctx->cert_part, part, sizeof part);
  ctx->cert_K = K; ctx->cert_skip = a.resp_skip; ctx->cert_age = 0;
  ctx->cert_valid = true;
  *kind = kCertReference;
  return MIMO_OK;
}

static void fill_args(mimo_ctx* ctx, int K, KernelArgs* a) {
  memset(a, 0, sizeof *a);
  a->Z = ctx->Z; a->N = ctx->N; a->D = ctx->D; a->K = K; a->K16 = (K + 15) / 16;
  a->F16 = ctx->F16;
  a->ZS = route_zs(K, ctx->D);
  a->RS = ctx->F16 + rs_pad();
  a->F16_total = ctx->F16;
  a->cb0 = 0;
  a->write_scalars = 1;
  a->LS = a->K16 * 16 + ls_pad(a->K16, ctx->D);
  a->feat = ctx->feat_d;
  a->row0 = ctx->row0;
  a->do_stats = 1;
  a->diag = ctx->structure != 0;
  a->ntiles = (ctx->N + kTile - 1) / kTile;
  a->aux = ctx->ls_aux;
  a->resp_skip = ctx->resp_skip_log2;
}

// Why pack_theta (mimo_theta.h) refused a parameter block, in the wording of the entry points (batched: `what`, problem p)
int mimo_abi::theta_fail(mimo_ctx* ctx, const ThetaFail& f, const char* what, int p) {
  switch (f.kind) {
    case ThetaFail::kBadC:
      return what ? fail(ctx, MIMO_E_INVALID, "%s: c[%d][%d] is NaN or +inf", what, p, f.k)
                  : fail(ctx, MIMO_E_INVALID, "c[%d] is NaN or +inf", f.k);
    case ThetaFail::kLinearW:
      return fail(ctx, MIMO_E_INVALID, "linear structure is set (mimo_set_structure) but W[%d] differs from W[0]", f.k);
    case ThetaFail::kDiagOffDiag:
      return fail(ctx, MIMO_E_INVALID, "diagonal structure is set (mimo_set_structure) but W[%d] has the "
                  "off-diagonal entry (%d,%d)", f.k, f.a, f.b);
    default:
      return what ? fail(ctx, MIMO_E_INVALID, "%s: b or W of problem %d holds a NaN or an infinity", what, p)
                  : fail(ctx, MIMO_E_INVALID, "b or W holds a NaN or an infinity");
  }
}

// The Theta image the route's kernels read (placements: mimo_theta.h), and a->theta.  The structure rules hold for every image;
// the mid images only ever see the full structure (mid_covers / mid_labels_covers admit no other, so use_mid / use_mid_labels
// never route one there).
static int upload_theta_for(mimo_ctx* ctx, const Route& route, const double* c, const double* b, const double* W, int K, KernelArgs* a) {
  const int D = ctx->D, F16 = ctx->F16, st = ctx->structure, ZS = route_zs(K, D);
  // a label pass over components switched off by c = -inf: the draw's relabel table (draw_label, mimo_device.h) rides behind the
  // image, in its transfer.  (An image in the kernel arguments is the small-shape kernel with ONE lane per row: one sequential
  // scan, whose count cannot stop on a component that adds nothing.)
  int32_t relabel[256] = {0};
  const bool off = a->gibbs && draw_relabel(c, K, relabel);
  auto stage = [&](const auto& pl, double* inline_img = nullptr) {
    const bool table = off && !inline_img;
    const int rc = stage_theta(ctx, pl, c, b, W, 1, table ? reinterpret_cast<const uint64_t*>(relabel) : nullptr, table ? (size_t)(K + 1) / 2 : 0,
                               nullptr, inline_img);
    a->theta = ctx->theta_d;
    a->relabel = table ? reinterpret_cast<const int32_t*>(ctx->theta_d + pl.count()) : nullptr;
    return rc;
  };
  switch (route.image) {
    case Image::Small: {
      // one lane per row (G = 1) and at most kThetaInline doubles: Theta goes into the kernel arguments
      const ThetaSmall pl = {D, K, small_g(D, K) * small_kl(D, K)};
      return stage(pl, small_g(D, K) == 1 && pl.count() <= (size_t)kThetaInline ? a->theta_inline : nullptr);
    }
    case Image::Narrow: {
      const int mode = route.narrow_mode - 1, V = narrow_v(K), NSF = narrow_steps(K, ctx->F, D, mode);
      if (!narrow_dt(K, ctx->F, D, mode)) return stage(ThetaNarrow{D, K, st, V, NSF, nullptr});
      const ThetaGroupedOrder order(D);
      return stage(ThetaNarrow{D, K, st, V, NSF, &order});
    }
    case Image::Mid: case Image::MidLabels: {
      const ThetaGroupedOrder order(D);
      return stage(ThetaMid{D, K, (K + 15) / 16, mid_steps(D), mid_pf(), route.image == Image::MidLabels, &order});
    }
    case Image::RowOwner: return stage(ThetaRowOwner{D, K, st, rowwave_kb_shape(K, F16, ZS), rowwave_image_ns(K, F16, ZS)});
    case Image::Generic: break;
  }
  // every wave streams 1 (K <= 64) or up to 4 row blocks, unused ones are zero; the fused kernels step through F16 / 4 slices
  // per row block, the chunked E-step through whole chunks
  const int K16 = (K + 15) / 16;
  ThetaGeneric pl = {D, K, st, K16 <= 4 ? 4 : 16, fused_covers(K16, F16 / 16, kSrcEstep) ? F16 / 4 : chunked_ns_pad(F16)};
  if (!order_applies(ctx, route, *a)) return stage(pl);
  // under a component order: component order[s] goes to slot s, and the order itself rides behind the image (same transfer)
  // for the unpack step, which writes slot s back to row order[s]
  int32_t slot_of[64];
  for (int s = 0; s < K; ++s) slot_of[ctx->order[s]] = s;
  pl.slot_of = slot_of;
  // ... and behind the order, for a certified pass, its table
  double tab[kCertTabLen];
  int kind = kCertNone, rc;
  if ((rc = cert_plan(ctx, *a, c, b, W, tab, &kind))) return rc;
  const size_t nord = (size_t)(K + 1) / 2;
  rc = stage_theta(ctx, pl, c, b, W, 1, reinterpret_cast<const uint64_t*>(ctx->order), nord, nullptr, nullptr,
                   kind == kCertCertified ? reinterpret_cast<const uint64_t*>(tab) : nullptr, kind == kCertCertified ? (size_t)kCertTabLen : 0);
  a->theta = ctx->theta_d;
  ctx->pass_order = reinterpret_cast<const int32_t*>(ctx->theta_d + pl.count());
  a->cert = kind;
  if (kind != kCertNone) {
    a->cert_k = ctx->cert_k; a->cert_m = ctx->cert_m; a->cert_a = ctx->cert_a; a->cert_cnt = ctx->cert_cnt;
    a->cert_tab = ctx->theta_d + pl.count() + nord;
  }
  return rc;
}

// What the router reads of the context
static Route route_for(const mimo_ctx* ctx, int K, const RouteRequest& q) {
  const RouteShape s = {ctx->D, ctx->F, ctx->F16, ctx->structure, ctx->N, ctx->n_bad, reinterpret_cast<uintptr_t>(ctx->Z) % 16 == 0};
  return choose_route(s, K, q, g_route_tunables);
}

// Workgroups of the pass's first kernel (what mimo_plan reports; the label-statistics stage behind a label kernel has label_stats_grid)
static int route_grid(const Route& route, const TwoStagePlan& ts, const KernelArgs& a, int num_cu, int F, int src) {
  switch (route.family) {
    case Family::Small: return small_grid(a, num_cu, src);
    case Family::Narrow: return narrow_grid(a, num_cu, F, route.narrow_mode - 1);
    case Family::Mid: return mid_grid(a, num_cu);
    case Family::MidLabels: return mid_labels_grid(a, num_cu);
    case Family::Rowwave: case Family::RowwaveVi: return rowwave_grid(a, num_cu);
    case Family::LabelStats: return label_stats_grid(label_stats_plan(a.K, a.D, a.diag, a.N), a.N, num_cu);   // (a.diag: the two reduced maps plan alike)
    case Family::TwoStage:
      // two-stage pass on the pipelined E-step (mimo_wide.hip): that kernel is built for two workgroups per CU whatever K is
      // (fused_grid's fallback assumes one for K > 128); the statistics launches of the pass share the grid (partial blocks)
      if (ts.estep == TwoStagePlan::Wide) {
        const int64_t g2 = 2 * (int64_t)num_cu;
        return (int)(g2 < a.ntiles ? g2 : (a.ntiles > 0 ? a.ntiles : 1));
      }
      [[fallthrough]];
    case Family::Fused: break;
  }
  return fused_grid(a, num_cu, src);
}

static void drain_profile(mimo_ctx* ctx) {
  for (auto& pr : ctx->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(pr.e1) == hipSuccess && hipEventElapsedTime(&ms, pr.e0, pr.e1) == hipSuccess) {
      ctx->prof_ms += ms;
      ctx->prof_name_ms[pr.name] += ms;
      ctx->prof_name_n[pr.name] += 1;
    }
    (void)hipEventDestroy(pr.e0);
    (void)hipEventDestroy(pr.e1);
  }
  ctx->pending.clear();
}

int mimo_abi::prof_slot(mimo_ctx* ctx, const char* name) {
  for (int i = 0; i < mimo_ctx::kProfNames; ++i) {
    if (ctx->prof_name[i] == name) return i;
    if (!ctx->prof_name[i]) { ctx->prof_name[i] = name; return i; }
  }
  return mimo_ctx::kProfNames - 1;
}

// buffers of the ranked tiles where the pass's LabelStatsPlan asks for them: several launches (Dz = 10 .. 16: windows) or the one-pass kernel.
// Tiles of 256 rows: label_tile_sort_kernel<256> writes, and label_stats_wide_kernel / label_stats_gram_kernel read, list entries
// [256 t, 256 t + 256) and starts [257 t, 257 t + 256] of the tiles t < ceil(N / 256) and nothing else.
// The one-pass kernel is the only route of its shapes, so it gets its buffers for an empty data set too (one tile nobody reads:
// every workgroup then writes an all-zero block); the windowed launches rank their own tiles without them.
static int prepare_label_presort(mimo_ctx* ctx, KernelArgs& a, const LabelStatsPlan& lp) {
  a.sort_list = nullptr; a.sort_start = nullptr;
  if (lp.ranked < 2 && (lp.ranked < 1 || a.N < 1)) return MIMO_OK;
  const size_t tiles = a.N < 1 ? 1 : (size_t)((a.N + 255) / 256);
  int rc;
  if ((rc = ctx->sort_list.ensure(ctx, tiles * 256))) return rc;
  if ((rc = ctx->sort_start.ensure(ctx, tiles * 257))) return rc;
  a.sort_list = ctx->sort_list; a.sort_start = ctx->sort_start;
  return MIMO_OK;
}

// Two-stage path, the kernels of `ts`: the E-step writes responsibilities / labels, then the statistics kernel
// runs once per group of <= ts.gmax feature column blocks, all into the same partial block.
static int launch_two_stage(mimo_ctx* ctx, KernelArgs& a, int src, const TwoStagePlan& ts, int grid) {
  const int K = a.K, D = a.D;
  const int ncb_total = a.F16 / 16;
  int rc;
  KernelArgs st = a;
  if (ts.estep != TwoStagePlan::NoEstep) {
    KernelArgs e = a;
    e.RS = 16 * kChunkNCB + 1;
    e.split = (a.split || a.resp || a.logp || a.lse) ? 1 : 0;   // include/mimo_hip.h: scalars[1..2] come with the split or any kept table
    if (!e.gibbs && e.do_stats && !e.resp) {       // statistics need the table: keep it internally
      if ((rc = ctx->resp.ensure(ctx, (size_t)K * (size_t)ctx->N))) return rc;
      e.resp = ctx->resp; ctx->resp_K = K; ctx->resp_valid = true;
    }
    if (chunked_lds_bytes(e) > 160 * 1024)
      return fail(ctx, MIMO_E_UNSUPPORTED, "K=%d, Dz=%d needs more LDS than one CU has", K, D);
    if (ts.estep == TwoStagePlan::Wide)                          // pipelined softmax / label pass (mimo_wide.hip)
      rc = TIMED_HIP(ctx, "wide_estep_kernel", launch_wide_estep(e, grid, ctx->stream));
    else
      rc = TIMED_HIP(ctx, "estep_chunked_kernel", launch_estep_chunked(e, grid, ctx->stream));
    if (rc) return rc;
    st.resp = e.resp; st.labels = e.labels; st.write_scalars = 0;
    if (ctx->n_bad > 0 && !e.gibbs && a.do_stats) {     // rows with NaN: their weights are dropped from the statistics
      if ((rc = ctx->table_tmp.ensure(ctx, (size_t)K * (size_t)ctx->N))) return rc;
      HIP_TRY(ctx, launch_mask_table(e.resp, ctx->row_mask, ctx->table_tmp, K, ctx->N, ctx->stream));
      st.resp = ctx->table_tmp;
    }
  }
  if (ts.stats == TwoStagePlan::NoStats) return MIMO_OK;
  if (ts.stats == TwoStagePlan::LabelStats) {
    KernelArgs g = st;
    g.gibbs = 0; g.do_stats = 1; g.logp = nullptr; g.lse = nullptr;
    if ((rc = prepare_label_presort(ctx, g, label_stats_plan(K, D, ctx->structure, g.N)))) return rc;
    return TIMED_HIP(ctx, "label_stats_kernel", launch_label_stats(g, ctx->structure, grid, ctx->stream));
  }
  for (int cb0 = 0; cb0 < ncb_total; cb0 += ts.gmax) {
    KernelArgs g = st;
    const int ncb = ncb_total - cb0 < ts.gmax ? ncb_total - cb0 : ts.gmax;
    g.cb0 = cb0; g.F16 = 16 * ncb; g.RS = g.F16 + 1; g.F16_total = a.F16;
    g.gibbs = 0; g.do_stats = 1; g.logp = nullptr; g.lse = nullptr;
    if (cb0 > 0) g.write_scalars = 0;
    if (ts.stats == TwoStagePlan::WideColumns) {        // 8-wave statistics kernel (mimo_wide.hip)
      rc = TIMED_HIP(ctx, "wide_stats_kernel", launch_wide_stats(g, grid, ctx->stream));
    } else {
      rc = timed_launch(ctx, src == kSrcEstep ? "fused_kernel(statistics of a column group)" : "fused_kernel", [&]() -> int {
        bool unsupported = false;
        HIP_TRY(ctx, launch_fused(g, ts.stats_src, grid, ctx->stream, &unsupported));
        if (unsupported) return fail(ctx, MIMO_E_UNSUPPORTED, "no statistics kernel for K=%d, Dz=%d", K, D);
        return MIMO_OK;
      });
    }
    if (rc) return rc;
  }
  return MIMO_OK;
}

// The partial blocks a pass left behind: how many (the grid of the kernel that wrote them) and how far apart
struct Launched { int grid; size_t pstride; };

// Launch the kernels of route.family, and behind a label kernel (or alone, Family::LabelStats) the label statistics
static int launch_route(mimo_ctx* ctx, KernelArgs& a, int src, const Route& route, Launched* out) {
  const int K = a.K, D = a.D;
  const bool small = route.family == Family::Small;
  if (small) { a.F16_total = 16; a.F16 = 16; }
  const TwoStagePlan ts = two_stage_plan(route, a, ctx->structure, src);
  const int kgrid = route_grid(route, ts, a, ctx->num_cu, ctx->F, src);
  const bool lstats = route.label_draw() || route.family == Family::LabelStats;     // the label-statistics kernels close the pass
  const LabelStatsPlan lp = label_stats_plan(K, D, ctx->structure, a.N);            // (of that stage)
  const int grid = lstats ? label_stats_grid(lp, a.N, ctx->num_cu) : kgrid;         // partial blocks
  *out = {grid, partial_stride(a.K16, a.F16)};
  int rc;
  if ((rc = ctx->partials.ensure(ctx, out->pstride * (size_t)grid))) return rc;
  a.partials = ctx->partials;

#ifdef MIMO_STAMPS
  {
    static unsigned long long* stamps_d = nullptr;
    if (!stamps_d) (void)hipMalloc(reinterpret_cast<void**>(&stamps_d), 4 * 8192 * 4 * 8 * sizeof(unsigned long long));
    a.stamps = stamps_d;
    g_stamps = stamps_d; g_stamps_grid = grid;
  }
#endif
  // a resident-Theta label kernel counts its labels for the slot table of the statistics kernel behind it
  // (not with NaN rows: their labels are masked before the statistics; MIMO_FUSE_LABEL_HIST=0: off)
  static const bool fuse_on = [] { const char* e = getenv("MIMO_FUSE_LABEL_HIST"); return !e || atoi(e) != 0; }();
  const bool fuse_hist = fuse_on && a.do_stats && ctx->n_bad == 0 && a.aux && lp.kind == LabelStatsPlan::Slots;
  rc = MIMO_OK;
  switch (route.family) {
  case Family::LabelStats: break;
  case Family::Rowwave: case Family::Narrow: {
    const bool narrow = route.family == Family::Narrow;
    a.fuse_hist = fuse_hist && (narrow ? route.narrow_mode == 2 : gibbs_rowwave_counts_labels(K, a.F16, a.ZS)) ? 1 : 0;
    rc = timed_launch(ctx, narrow ? "narrow_kernel" : "gibbs_rowwave_kernel", [&]() -> int {
      if (a.fuse_hist) HIP_TRY(ctx, launch_label_hist_reset(a, ctx->stream));
      HIP_TRY(ctx, narrow ? launch_narrow(a, ctx->F, route.narrow_mode - 1, kgrid, ctx->stream) : launch_gibbs_rowwave(a, kgrid, ctx->stream));
      return MIMO_OK;
    });
    break;
  }
  case Family::MidLabels: rc = TIMED_HIP(ctx, "mid_kernel (labels)", launch_mid_labels(a, kgrid, ctx->stream)); break;
  case Family::RowwaveVi: rc = TIMED_HIP(ctx, "vi_rowwave_kernel", launch_vi_rowwave(a, grid, ctx->stream)); break;
  case Family::Mid: rc = TIMED_HIP(ctx, "mid_kernel", launch_mid(a, grid, ctx->stream)); break;
  case Family::Small: case Family::Fused:
    rc = timed_launch(ctx, small ? "small_kernel" : "fused_kernel", [&]() -> int {
      bool unsupported = false;
      hipError_t he = small ? launch_small(a, src, grid, ctx->stream, &unsupported) : launch_fused(a, src, grid, ctx->stream, &unsupported);
      if (unsupported) return fail(ctx, MIMO_E_UNSUPPORTED, "no %s kernel for K=%d, Dz=%d", small ? "small-shape" : "fused", K, D);
      HIP_TRY(ctx, he);
      return MIMO_OK;
    });
    break;
  case Family::TwoStage: rc = launch_two_stage(ctx, a, src, ts, grid); break;
  }
  if (rc) return rc;
  if (lstats && a.do_stats) {
    if ((rc = prepare_label_presort(ctx, a, lp))) return rc;
    if ((rc = TIMED_HIP(ctx, "label_stats_kernel", launch_label_stats(a, ctx->structure, grid, ctx->stream)))) return rc;
  }
  if (ctx->prof) ctx->prof_n += 1;
  return MIMO_OK;
}

// Room for a block of `len` doubles on the device and in its pinned host sibling
int mimo_abi::ensure_block(mimo_ctx* ctx, size_t len) {
  ctx->batch_stats_valid = false;      // whatever the caller puts there next, it says so itself
  const int rc = ctx->S_d.ensure(ctx, len);
  return rc ? rc : ctx->S_h.ensure(ctx, len);
}

// The end of every host delivery.  The first `copy_len` doubles of the device block follow the kernels into the pinned buffer
// (0: they are there already, or on their way); then wait for the stream and hand the caller `nstats` doubles from its front
// and `nscalars` doubles from `scalars_at` on.  A null destination is skipped.
int mimo_abi::hand_out(mimo_ctx* ctx, size_t copy_len, double* S, size_t nstats, double* scalars, size_t scalars_at, size_t nscalars) {
  if (copy_len) HIP_TRY(ctx, hipMemcpyAsync(ctx->S_h, ctx->S_d, copy_len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (S) memcpy(S, ctx->S_h, nstats * sizeof(double));
  if (scalars) memcpy(scalars, ctx->S_h + scalars_at, nscalars * sizeof(double));
  return MIMO_OK;
}

// Reduce the partial blocks of a pass -> unpack; deliver S / scalars to host or device pointers
static int deliver(mimo_ctx* ctx, const KernelArgs& a, int flags, double* S, double* scalars, const Route& route, const Launched& l) {
  const int K = a.K, D = a.D;
  const bool small = route.family == Family::Small;
  const bool async = (flags & MIMO_F_ASYNC) != 0;
  // (a promoted bound pass leaves its statistics in the partial blocks: nothing of them is reduced, all-reduced or copied)
  const bool want_stats = a.do_stats && !route.promoted && (S || async);
  const bool device_out = (flags & MIMO_F_DEVICE_OUT) != 0;
  if (!want_stats && !scalars && !async) return MIMO_OK;

  int rc;
  const size_t slen = packed_len(K, D);
  // the small-shape kernel always accumulates the full feature map: under a structure hint the entries outside
  // the structure are masked to the zeros the hint promises
  const uint8_t* feat = small ? ctx->feat_full_d : ctx->feat_d;
  const int F = small ? feat_count(D) : ctx->F, mask = small ? ctx->structure : 0;
  if (device_out) {
    HIP_TRY(ctx, launch_reduce_unpack(ctx->partials, l.grid, (int64_t)l.pstride, feat, K, D, F, a.F16, want_stats ? S : nullptr, scalars,
                                      ctx->stream, mask, ctx->pass_order));
    if (ctx->comm) {     // sharded through this library: sum over the ranks where the caller wants the block
      char msg[256];
      if (want_stats && (rc = mimo_comm::allreduce_sum_f64(ctx->comm, S, slen, ctx->stream, msg, sizeof msg))) return fail(ctx, rc, "%s", msg);
      if (scalars && (rc = mimo_comm::allreduce_sum_f64(ctx->comm, scalars, 3, ctx->stream, msg, sizeof msg))) return fail(ctx, rc, "%s", msg);
    }
    return MIMO_OK;
  }
  if ((rc = ensure_block(ctx, slen + 4))) return rc;
  // Without a communicator and on the full feature map the reduction writes the packed block straight into the pinned host
  // buffer (device-visible, hipHostMalloc): no device copy of the block, no D2H transfer behind the kernel.
  static const bool direct_on = [] { const char* e = getenv("MIMO_DIRECT_OUT"); return !e || atoi(e) != 0; }();   // tuning knob
  const bool direct = direct_on && !ctx->comm && F == feat_count(D);
  double* dst = direct ? ctx->S_h.p : ctx->S_d.p;
  if (ctx->comm && !want_stats) HIP_TRY(ctx, hipMemsetAsync(ctx->S_d, 0, slen * sizeof(double), ctx->stream));
  HIP_TRY(ctx, launch_reduce_unpack(ctx->partials, l.grid, (int64_t)l.pstride, feat, K, D, F, a.F16, want_stats ? dst : nullptr,
                                    dst + slen, ctx->stream, mask, ctx->pass_order));
  if (ctx->comm) {       // ONE all-reduce(sum, f64) of [K (1 + Dz + Dz^2) + 3] per pass, behind the kernels on the same stream
    char msg[256];
    if ((rc = mimo_comm::allreduce_sum_f64(ctx->comm, ctx->S_d, slen + 3, ctx->stream, msg, sizeof msg))) return fail(ctx, rc, "%s", msg);
  }
  if (!direct) HIP_TRY(ctx, hipMemcpyAsync(ctx->S_h, ctx->S_d, (slen + 4) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (!async) return hand_out(ctx, 0, want_stats ? S : nullptr, slen, scalars, slen, 3);
  ctx->pending_async = true; ctx->pending_slen = slen; ctx->pending_stats = want_stats;     // mimo_wait hands the block out
  return MIMO_OK;
}

// run the pass (the kernels of route.family) -> reduce -> unpack -> S / scalars at the caller's host or device pointers
static int run_pass(mimo_ctx* ctx, KernelArgs& a, int src, int flags, double* S, double* scalars, const Route& route) {
  Launched l;
  const int rc = launch_route(ctx, a, src, route, &l);
  return rc ? rc : deliver(ctx, a, flags, S, scalars, route, l);
}

// Every pass goes through here.  Data without NaN rows: straight to run_pass.  With NaN rows (zeroed in the library's
// copy, ctx->row_mask = 0 there): the log-densities, tables, labels and ELBO scalars are those of the zeroed rows
// (= the reference's normaliser-only log-density), the statistics leave those rows out —
//   softmax pass : the mask becomes the per-row weight vector of the statistics (times the caller's weights, if any);
//   label pass   : labels first (no statistics), then the statistics of the labels with the NaN rows set to -1; the
//                  labels drawn ON the NaN rows are counted per component for the gating update (mimo_nan_info);
//   statistics of a caller's table / labels: masked copies.
static int run_fused(mimo_ctx* ctx, KernelArgs& a, int src, int flags, double* S, double* scalars, const Route& route) {
  if (ctx->n_bad <= 0) return run_pass(ctx, a, src, flags, S, scalars, route);
  int rc;
  const int64_t N = ctx->N;
  ctx->bad_counts_K = 0;
  if (src == kSrcEstep && !a.gibbs) {
    if (!a.u) {
      a.u = ctx->row_mask;
    } else {       // caller's row weights x mask (one column of a "table")
      if ((rc = ctx->table_tmp.ensure(ctx, (size_t)N))) return rc;
      HIP_TRY(ctx, launch_mask_table(a.u, ctx->row_mask, ctx->table_tmp, 1, N, ctx->stream));
      a.u = ctx->table_tmp;
    }
    return run_pass(ctx, a, src, flags, S, scalars, route);
  }
  if ((src == kSrcEstep && a.gibbs) || src == kSrcLabels) {
    const bool want = a.do_stats != 0;
    if (src == kSrcEstep) {
      if (flags & MIMO_F_ASYNC) return fail(ctx, MIMO_E_UNSUPPORTED, "asynchronous label pass on data with NaN rows");
      a.do_stats = 0;
      if ((rc = run_pass(ctx, a, kSrcEstep, flags & ~(MIMO_F_DEVICE_OUT), nullptr, nullptr, route))) return rc;
    }
    if ((rc = ctx->labels_tmp.ensure(ctx, (size_t)N))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->cnt_d + kCntLabels, 0, 256 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_mask_labels(a.labels, ctx->row_mask, ctx->labels_tmp, N, a.K, ctx->cnt_d + kCntLabels, ctx->stream));
    ctx->bad_counts_K = a.K;
    if (!want) return MIMO_OK;
    KernelArgs b = a;
    b.labels = ctx->labels_tmp; b.gibbs = 0; b.do_stats = 1; b.u = nullptr; b.logp = nullptr; b.lse = nullptr; b.resp = nullptr;
    return run_pass(ctx, b, kSrcLabels, flags, S, scalars, route_for(ctx, a.K, {kSrcLabels}));
  }
  // kSrcWeights: statistics of a (K, N) table
  if ((rc = ctx->table_tmp.ensure(ctx, (size_t)a.K * (size_t)N))) return rc;
  HIP_TRY(ctx, launch_mask_table(a.resp, ctx->row_mask, ctx->table_tmp, a.K, N, ctx->stream));
  a.resp = ctx->table_tmp;
  return run_pass(ctx, a, src, flags, S, scalars, route);
}

int mimo_abi::set_data(mimo_ctx* ctx, int64_t N, int Dz) {
  if (N < 0) return fail(ctx, MIMO_E_INVALID, "N must be >= 0");
  if (Dz < 1 || Dz > kMaxD)
    return fail(ctx, MIMO_E_UNSUPPORTED, "Dz = %d outside [1, %d]", Dz, kMaxD);
  ctx->N = N; ctx->D = Dz;
  ctx->order_K = 0;
  ctx->cert_valid = false; ctx->cert_prev_K = 0;
  ctx->batched = false;
  ctx->batch_shared = false;
  ctx->resp_valid = ctx->logp_valid = ctx->lse_valid = ctx->labels_valid = false;
  ctx->weights_resident = false;
  ctx->batch_w_valid = false;
  ctx->batch_stats_valid = false;
  ctx->vi_prior_valid = false;
  ctx->svi_state_valid = false;
  return prepare_features(ctx, Dz);
}

// Replace the resident rows by N x D doubles from `src`: a host block that is copied, the caller's device rows that are borrowed,
// or (scan_nan_rows) borrowed rows that need a copy the library may write.  ctx->Z is null from before the old copy is freed until
// the last step has succeeded, so a failure leaves the context without data (MIMO_E_NODATA) and never with freed rows.
int mimo_abi::set_rows(mimo_ctx* ctx, const double* src, Rows how) {
  const size_t count = (size_t)ctx->N * ctx->D;
  int rc;
  ctx->Z = nullptr;
  if (how != Rows::DeviceCopy) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // kernels of earlier calls may still read the old rows
  HIP_TRY(ctx, ctx->Z_owned.release());
  if (how != Rows::DeviceBorrow) {
    if ((rc = ctx->Z_owned.ensure(ctx, count))) return rc;
    if (how == Rows::DeviceCopy) HIP_TRY(ctx, hipMemcpyAsync(ctx->Z_owned, src, count * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    else if (count) HIP_TRY(ctx, hipMemcpy(ctx->Z_owned, src, count * sizeof(double), hipMemcpyHostToDevice));
    src = ctx->Z_owned;
  }
  ctx->Z = src;
  return MIMO_OK;
}

// The end of every getter: `bytes` of a device table to the caller, or why there is none
int mimo_abi::copy_out(mimo_ctx* ctx, void* dst, const void* src, size_t bytes, bool valid, const char* what) {
  int rc = bind(ctx); if (rc) return rc;
  if (!dst) return fail(ctx, MIMO_E_INVALID, "%s: destination is NULL", what);
  if (!valid || !src) return fail(ctx, MIMO_E_STATE, "%s: table was never produced (pass the MIMO_F_KEEP_* flag)", what);
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" {

const char* mimo_version(void) { return "mimo_hip 0.1 (gfx950, f64 MFMA feature-GEMM)"; }

int mimo_create(mimo_ctx** out, int device) {
  return guarded(nullptr, [&]() -> int {
  if (!out) return fail(nullptr, MIMO_E_INVALID, "mimo_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, MIMO_E_HIP, "mimo_create: no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= ndev)
    return fail(nullptr, MIMO_E_INVALID, "mimo_create: device %d out of range [0,%d)", device, ndev);
  mimo_ctx* ctx = new (std::nothrow) mimo_ctx();
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "mimo_create: out of host memory");
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete ctx; return fail(nullptr, MIMO_E_HIP, "hipSetDevice failed"); }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cu = ctx->hw_num_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return fail(nullptr, MIMO_E_HIP, "hipStreamCreate failed");
  }
  ctx->stream = ctx->own_stream;
  if (ctx->ls_aux.ensure(nullptr, label_stats_aux_words())) { delete ctx; return MIMO_E_HIP; }     // (the text is in g_err)
  *out = ctx;
  return MIMO_OK;
  });
}

int mimo_destroy(mimo_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return MIMO_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  drain_profile(ctx);
  if (ctx->comm) { (void)mimo_comm::destroy(ctx->comm); ctx->comm = nullptr; }
  delete ctx;      // the stream and every buffer go with it
  return MIMO_OK;
  });
}

const char* mimo_last_error(const mimo_ctx* ctx) { return ctx ? ctx->err : g_err; }

int mimo_set_stream(mimo_ctx* ctx, void* hip_stream) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return MIMO_OK;
  });
}

// Find the rows that hold a NaN.  `owned`: Z is the library's copy — such rows are zeroed in place and the mask written;
// otherwise (borrowed device buffer) they are only counted, and if there are any the data is copied first.
static int scan_nan_rows(mimo_ctx* ctx, bool checksum) {
  ctx->n_bad = 0; ctx->bad_counts_K = 0;
  ctx->data_sum_valid = false;
  if (ctx->N <= 0) {
    if (checksum) { ctx->data_sum[0] = ctx->data_sum[1] = 0; ctx->data_sum_valid = true; }
    return MIMO_OK;
  }
  int rc;
  if ((rc = ctx->cnt_d.ensure(ctx, kCntWords))) return rc;
  // flat scan first (one coalesced read of Z): data without a NaN — the usual case — is done after it; the same read
  // yields the content checksum of an upload (before any row is zeroed)
  HIP_TRY(ctx, hipMemsetAsync(ctx->cnt_d, 0, sizeof(unsigned long long), ctx->stream));
  if (checksum) HIP_TRY(ctx, hipMemsetAsync(ctx->cnt_d + kCntChecksum, 0, 2 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_nan_any(ctx->Z, ctx->N * ctx->D, reinterpret_cast<unsigned int*>(ctx->cnt_d.p), ctx->hw_num_cu, ctx->stream,
                              checksum ? ctx->cnt_d + kCntChecksum : nullptr));
  unsigned long long nb = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&nb, ctx->cnt_d, sizeof nb, hipMemcpyDeviceToHost, ctx->stream));
  if (checksum) HIP_TRY(ctx, hipMemcpyAsync(ctx->data_sum, ctx->cnt_d + kCntChecksum, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->data_sum_valid = checksum;
  if (nb == 0) return MIMO_OK;
  HIP_TRY(ctx, hipMemsetAsync(ctx->cnt_d, 0, sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_nan_scan(const_cast<double*>(ctx->Z), ctx->N, ctx->D, nullptr, ctx->cnt_d, false, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&nb, ctx->cnt_d, sizeof nb, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (nb == 0) return MIMO_OK;
  if (ctx->Z != ctx->Z_owned.p && (rc = set_rows(ctx, ctx->Z, Rows::DeviceCopy))) return rc;   // borrowed buffer: never written — work on a copy
  if ((rc = ctx->row_mask.ensure(ctx, (size_t)ctx->N))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->cnt_d, 0, sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_nan_scan(ctx->Z_owned, ctx->N, ctx->D, ctx->row_mask, ctx->cnt_d, true, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->n_bad = (int64_t)nb;
  return MIMO_OK;
}

int mimo_upload(mimo_ctx* ctx, const double* Z_host, int64_t N, int Dz) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!Z_host && N > 0) return fail(ctx, MIMO_E_INVALID, "mimo_upload: Z is NULL");
  if ((rc = set_data(ctx, N, Dz))) return rc;
  if ((rc = set_rows(ctx, Z_host, Rows::HostCopy))) return rc;
  return scan_nan_rows(ctx, true);
  });
}

int mimo_data_checksum(mimo_ctx* ctx, uint64_t out[2]) {
  return guarded(ctx, [&]() -> int {
  if (!ctx || !out) return fail(ctx, MIMO_E_INVALID, "mimo_data_checksum: null argument");
  if (!ctx->Z || !ctx->data_sum_valid) return fail(ctx, MIMO_E_STATE, "mimo_data_checksum: no uploaded rows (attached device rows are not summed)");
  out[0] = ctx->data_sum[0]; out[1] = ctx->data_sum[1];
  return MIMO_OK;
  });
}

int mimo_attach(mimo_ctx* ctx, const double* Z_dev, int64_t N, int Dz) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!Z_dev) return fail(ctx, MIMO_E_INVALID, "mimo_attach: Z is NULL");
  if ((rc = set_data(ctx, N, Dz))) return rc;
  if ((rc = set_rows(ctx, Z_dev, Rows::DeviceBorrow))) return rc;
  return scan_nan_rows(ctx, false);
  });
}

int mimo_set_structure(mimo_ctx* ctx, int structure) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (structure != MIMO_STRUCT_FULL && structure != MIMO_STRUCT_DIAG && structure != MIMO_STRUCT_LINEAR)
    return fail(ctx, MIMO_E_INVALID, "mimo_set_structure: unknown structure %d", structure);
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (ctx->structure == structure) return MIMO_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));    // the feature table may be in use
  ctx->structure = structure;
  ctx->order_K = 0;
  ctx->cert_valid = false; ctx->cert_prev_K = 0;
  return ctx->D > 0 ? prepare_features(ctx, ctx->D) : MIMO_OK;
  });
}

int mimo_set_component_order(mimo_ctx* ctx, const int32_t* order, int K) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (K < 1 || K > 256) return fail(ctx, MIMO_E_INVALID, "mimo_set_component_order: K = %d outside [1, 256]", K);
  if (!order || !ctx->block_order_on) { ctx->order_K = 0; return MIMO_OK; }
  bool seen[256] = {false};
  for (int s = 0; s < K; ++s) {
    if (order[s] < 0 || order[s] >= K)
      return fail(ctx, MIMO_E_INVALID, "mimo_set_component_order: order[%d] = %d is no component of 0 .. %d", s, (int)order[s], K - 1);
    if (seen[order[s]])
      return fail(ctx, MIMO_E_INVALID, "mimo_set_component_order: component %d sits in two slots (the second: %d)", (int)order[s], s);
    seen[order[s]] = true;
  }
  memcpy(ctx->order, order, sizeof(int32_t) * (size_t)K);
  ctx->order_K = K;
  return MIMO_OK;
  });
}

int mimo_set_row_offset(mimo_ctx* ctx, int64_t row0) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  ctx->row0 = row0;
  return MIMO_OK;
  });
}

static int keep_tables(mimo_ctx* ctx, int K, int flags, KernelArgs* a) {
  int rc;
  const size_t kn = (size_t)K * (size_t)ctx->N;
  if (flags & MIMO_F_KEEP_RESP) {
    if ((rc = ctx->resp.ensure(ctx, kn))) return rc;
    a->resp = ctx->resp; ctx->resp_K = K; ctx->resp_valid = true;
  }
  if (flags & MIMO_F_KEEP_LOGP) {
    if ((rc = ctx->logp.ensure(ctx, kn))) return rc;
    a->logp = ctx->logp; ctx->logp_K = K; ctx->logp_valid = true;
  }
  if (flags & MIMO_F_KEEP_LSE) {
    if ((rc = ctx->lse.ensure(ctx, (size_t)ctx->N))) return rc;
    a->lse = ctx->lse; ctx->lse_valid = true;
  }
  return MIMO_OK;
}

int mimo_estep(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
               int flags, double* S, double* scalars) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!c || !b || !W) return fail(ctx, MIMO_E_INVALID, "mimo_estep: c, b, W must be non-NULL");
  const bool no_stats = (flags & MIMO_F_NO_STATS) != 0;
  if (!no_stats && !S && !(flags & MIMO_F_ASYNC))
    return fail(ctx, MIMO_E_INVALID, "mimo_estep: S is NULL without MIMO_F_NO_STATS / MIMO_F_ASYNC");
  KernelArgs a;
  fill_args(ctx, K, &a);
  RouteRequest q;
  q.tables = (flags & (MIMO_F_KEEP_RESP | MIMO_F_KEEP_LOGP | MIMO_F_KEEP_LSE | MIMO_F_ENTROPY_SPLIT)) != 0;
  q.stats = !no_stats;
  q.device_out = (flags & MIMO_F_DEVICE_OUT) != 0;
  const Route route = route_for(ctx, K, q);
  a.do_stats = (no_stats && !route.promoted) ? 0 : 1;
  a.split = (flags & MIMO_F_ENTROPY_SPLIT) ? 1 : 0;
  if ((rc = keep_tables(ctx, K, flags, &a))) return rc;
  ctx->cert_last = kCertNone;
  if ((rc = upload_theta_for(ctx, route, c, b, W, K, &a))) { ctx->cert_valid = false; return rc; }
  if ((rc = run_fused(ctx, a, kSrcEstep, flags, no_stats ? nullptr : S, scalars, route))) { ctx->cert_valid = false; return rc; }
  ctx->cert_last = a.cert;
  return MIMO_OK;
  });
}

int mimo_estep_weighted(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
                        const double* row_weights, int flags, double* S, double* scalars) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!c || !b || !W || (!row_weights && !(flags & MIMO_F_WEIGHTS_RESIDENT)))
    return fail(ctx, MIMO_E_INVALID, "mimo_estep_weighted: c, b, W, row_weights must be non-NULL");
  if (flags & MIMO_F_NO_STATS) return fail(ctx, MIMO_E_INVALID, "mimo_estep_weighted: the weights only enter the statistics");
  if (!S && !(flags & MIMO_F_ASYNC)) return fail(ctx, MIMO_E_INVALID, "mimo_estep_weighted: S is NULL");
  KernelArgs a;
  fill_args(ctx, K, &a);
  // the narrow kernels take the weights on their normaliser (plain requests: statistics + scalars only)
  RouteRequest q;
  q.tables = (flags & (MIMO_F_KEEP_RESP | MIMO_F_KEEP_LOGP | MIMO_F_KEEP_LSE | MIMO_F_ENTROPY_SPLIT)) != 0;
  q.weighted = true;
  const Route route = route_for(ctx, K, q);
  if (route.family == Family::TwoStage)
    return fail(ctx, MIMO_E_UNSUPPORTED, "mimo_estep_weighted: K=%d, Dz=%d runs on the two-stage path, which takes "
                "its weights as a table (mimo_estep + mimo_weighted_stats)", K, ctx->D);
  a.split = (flags & MIMO_F_ENTROPY_SPLIT) ? 1 : 0;
  if ((rc = keep_tables(ctx, K, flags, &a))) return rc;
  bool copied = false;        // MIMO_F_WEIGHTS_RESIDENT: the weights of the last call, whatever row_weights is
  if ((rc = stage_input<double>(ctx, (flags & MIMO_F_WEIGHTS_RESIDENT) ? nullptr : row_weights, (size_t)ctx->N, flags, ctx->u_d,
                                {ctx->u_d, ctx->weights_resident, "mimo_estep_weighted: no row weights are resident on the device"}, K,
                                &a.u, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pageable host memory
  if (copied) ctx->weights_resident = true;                      // u_d holds this call's weights
  if ((rc = upload_theta_for(ctx, route, c, b, W, K, &a))) return rc;
  return run_fused(ctx, a, kSrcEstep, flags, S, scalars, route);
  });
}

int mimo_wait(mimo_ctx* ctx, double* S, double* scalars) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!ctx->pending_async) return fail(ctx, MIMO_E_STATE, "mimo_wait: no asynchronous call is pending");
  const bool no_block = S && !ctx->pending_stats;      // refused once the call has been waited for; nothing is handed out then
  const size_t slen = ctx->pending_slen;
  if ((rc = hand_out(ctx, 0, no_block ? nullptr : S, slen, no_block ? nullptr : scalars, slen, 3))) return rc;
  ctx->pending_async = false;
  if (no_block) return fail(ctx, MIMO_E_STATE, "mimo_wait: the pending call produced no statistics");
  return MIMO_OK;
  });
}

int mimo_gibbs_labels(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
                      uint64_t seed, uint64_t sweep, const double* u, int flags,
                      int32_t* labels_out, double* S) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!c || !b || !W) return fail(ctx, MIMO_E_INVALID, "mimo_gibbs_labels: c, b, W must be non-NULL");
  const bool no_stats = (flags & MIMO_F_NO_STATS) != 0 || !S;
  KernelArgs a;
  fill_args(ctx, K, &a);
  a.gibbs = 1;
  a.do_stats = no_stats ? 0 : 1;
  a.seed = seed; a.sweep = sweep;
  if ((rc = ctx->labels.ensure(ctx, (size_t)ctx->N))) return rc;
  a.labels = ctx->labels; ctx->labels_valid = true;
  if ((rc = keep_tables(ctx, K, flags & (MIMO_F_KEEP_LOGP | MIMO_F_KEEP_LSE), &a))) return rc;
  bool copied = false;        // (u NULL: the kernel draws its own Philox uniforms)
  if ((rc = stage_input<double>(ctx, u, (size_t)ctx->N, flags, ctx->u_d, {}, K, &a.u, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // u is pageable host memory
  if (copied) ctx->weights_resident = false;                     // u_d holds uniforms now
  RouteRequest q;
  q.gibbs = true;
  q.tables = (flags & (MIMO_F_KEEP_LOGP | MIMO_F_KEEP_LSE)) != 0;
  q.stats = !no_stats;
  const Route route = route_for(ctx, K, q);
  if ((rc = upload_theta_for(ctx, route, c, b, W, K, &a))) return rc;
  if ((rc = run_fused(ctx, a, kSrcEstep, flags, no_stats ? nullptr : S, nullptr, route))) return rc;
  if (labels_out && !(flags & MIMO_F_DEVICE_OUT)) {
    HIP_TRY(ctx, hipMemcpyAsync(labels_out, ctx->labels, (size_t)ctx->N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MIMO_OK;
  });
}

int mimo_weighted_stats(mimo_ctx* ctx, const double* resp, int K, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!S) return fail(ctx, MIMO_E_INVALID, "mimo_weighted_stats: S is NULL");
  KernelArgs a;
  fill_args(ctx, K, &a);
  bool copied = false;
  if ((rc = stage_input<double>(ctx, resp, (size_t)K * (size_t)ctx->N, flags, ctx->win,
                                {ctx->resp, ctx->resp_valid && ctx->resp_K == K, "mimo_weighted_stats: resp is NULL and no (K=%d,N) table is resident"},
                                K, &a.resp, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pageable host memory
  return run_fused(ctx, a, kSrcWeights, flags, S, nullptr, route_for(ctx, K, {kSrcWeights}));
  });
}

int mimo_label_stats(mimo_ctx* ctx, const int32_t* labels, int K, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!S) return fail(ctx, MIMO_E_INVALID, "mimo_label_stats: S is NULL");
  KernelArgs a;
  fill_args(ctx, K, &a);
  bool copied = false;
  if ((rc = stage_input<int32_t>(ctx, labels, (size_t)ctx->N, flags, ctx->lin,
                                 {ctx->labels, ctx->labels_valid, "mimo_label_stats: labels is NULL and none are resident"}, K, &a.labels, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pageable host memory
  return run_fused(ctx, a, kSrcLabels, flags, S, nullptr, route_for(ctx, K, {kSrcLabels}));
  });
}

int mimo_sample_from_log(mimo_ctx* ctx, const double* logp, int K, int64_t N, const double* u, uint64_t seed,
                         uint64_t sweep, int flags, int32_t* labels_out, double* lognorms_out) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
  if (K < 1 || N < 0 || !labels_out) return fail(ctx, MIMO_E_INVALID, "mimo_sample_from_log: bad arguments");
  const double *table = nullptr, *ud = nullptr;
  bool table_copied = false, u_copied = false;
  if ((rc = stage_input<double>(ctx, logp, (size_t)K * (size_t)N, flags, ctx->win,
                                {ctx->logp, ctx->logp_valid && ctx->logp_K == K && ctx->N == N,
                                 "mimo_sample_from_log: logp is NULL and no (K=%d, N) log-density table is resident"}, K, &table, &table_copied))) return rc;
  if ((rc = stage_input<double>(ctx, u, (size_t)N, flags, ctx->u_d, {}, K, &ud, &u_copied))) return rc;    // (u NULL: Philox uniforms)
  if (u_copied) ctx->weights_resident = false;         // u_d holds uniforms now
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // pageable host sources
  if ((rc = ctx->lin.ensure(ctx, (size_t)N))) return rc;
  double* ln_d = nullptr;
  if (lognorms_out) {
    if ((rc = ctx->lse.ensure(ctx, (size_t)std::max(N, ctx->N)))) return rc;      // also long enough for the resident rows: it stays their lse buffer
    ctx->lse_valid = false;      // (the buffer is borrowed: whatever log-normaliser it held is gone)
    ln_d = ctx->lse;
  }
  HIP_TRY(ctx, launch_sample_table(table, K, N, ud, seed, sweep, ctx->row0, ctx->lin, ln_d, ctx->stream));
  if (N > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(labels_out, ctx->lin, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (lognorms_out) HIP_TRY(ctx, hipMemcpyAsync(lognorms_out, ln_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}

int mimo_random_resp_stats(mimo_ctx* ctx, int K, uint64_t seed, int flags, double* S) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if ((rc = check_shapes(ctx, K))) return rc;
  if (!S) return fail(ctx, MIMO_E_INVALID, "mimo_random_resp_stats: S is NULL");
  if ((rc = ctx->resp.ensure(ctx, (size_t)K * (size_t)ctx->N))) return rc;
  ctx->resp_K = K; ctx->resp_valid = true;
  HIP_TRY(ctx, launch_random_resp(ctx->resp, K, ctx->N, seed, ctx->row0, ctx->stream));
  KernelArgs a;
  fill_args(ctx, K, &a);
  a.resp = ctx->resp;
  return run_fused(ctx, a, kSrcWeights, flags, S, nullptr, route_for(ctx, K, {kSrcWeights}));
  });
}

int mimo_table_entropy(mimo_ctx* ctx, const double* table, int64_t count, int flags, double* out) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!out || count < 0) return fail(ctx, MIMO_E_INVALID, "mimo_table_entropy: bad arguments");
  const double* src = nullptr;
  bool copied = false;
  if ((rc = stage_input<double>(ctx, table, (size_t)count, flags, ctx->win,
                                {ctx->resp, ctx->resp_valid, "mimo_table_entropy: table is NULL and no resp table is resident"}, 0, &src, &copied))) return rc;
  if (copied) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // pageable host memory
  if (!table) count = (int64_t)ctx->resp_K * ctx->N;             // the whole resident table
  const int nblocks = 1024;
  if ((rc = ctx->partials.ensure(ctx, (size_t)nblocks))) return rc;
  if ((rc = ctx->reduced.ensure(ctx, 4))) return rc;
  HIP_TRY(ctx, launch_table_entropy(src, count, ctx->partials, nblocks, ctx->reduced, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->reduced, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}

int mimo_predict(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
                 const double* M, const double* Q, const double* Cc, int dy, int affine, int mode,
                 const double* y, const double* P, const double* ld,
                 double* mu, double* covar, double* nlpd) {
  return mimo_predict_flags(ctx, c, b, W, K, M, Q, Cc, dy, affine, mode, y, P, ld, mu, covar, nlpd, 0);
}

int mimo_predict_flags(mimo_ctx* ctx, const double* c, const double* b, const double* W, int K,
                       const double* M, const double* Q, const double* Cc, int dy, int affine, int mode,
                       const double* y, const double* P, const double* ld,
                       double* mu, double* covar, double* nlpd, int flags) {
  return guarded(ctx, [&]() -> int {
  const bool dev_in = (flags & MIMO_F_DEVICE_IN) != 0, dev_out = (flags & MIMO_F_DEVICE_OUT) != 0, diag = (flags & MIMO_F_DIAG_VAR) != 0;
  const size_t ncov = diag ? 2 * (size_t)dy : (size_t)dy * dy;        // doubles of the second output per row
  int rc = bind(ctx); if (rc) return rc;
  if (!ctx->Z) return fail(ctx, MIMO_E_NODATA, "mimo_predict: no data resident (call mimo_upload)");
  if ((rc = single_only(ctx))) return rc;
  if (!c || !b || !W || !M || !Q || !Cc || !mu || !covar || K < 1 || (mode != 0 && mode != 1))
    return fail(ctx, MIMO_E_INVALID, "mimo_predict: bad arguments");
  const bool want_nlpd = nlpd != nullptr;
  if (want_nlpd && (!y || !P || !ld)) return fail(ctx, MIMO_E_INVALID, "mimo_predict: nlpd needs y, P and ld");
  const int dx = ctx->D, dc = dx + (affine ? 1 : 0);
  const int64_t N = ctx->N;
  const size_t ng = packed_len(K, dx), nM = (size_t)K * dy * dc, nQ = (size_t)K * dc * dc,
               nC = (size_t)K * dy * dy;
  const size_t nparam = ng + nM + nQ + 2 * nC + K;
  const size_t nout = dev_out ? 0 : (size_t)N * (dy + ncov + 1), nin = (want_nlpd && !dev_in) ? (size_t)N * dy : 0;
  // parameters | outputs | y, all in the staged-weights workspace
  if ((rc = ctx->win.ensure(ctx, nparam + nout + nin + 1))) return rc;
  std::vector<double> h(nparam);
  double* q = h.data();
  for (int k = 0; k < K; ++k) {
    *q++ = c[k];
    memcpy(q, b + (size_t)k * dx, sizeof(double) * dx); q += dx;
    memcpy(q, W + (size_t)k * dx * dx, sizeof(double) * dx * dx); q += (size_t)dx * dx;
  }
  memcpy(q, M, sizeof(double) * nM); q += nM;
  memcpy(q, Q, sizeof(double) * nQ); q += nQ;
  memcpy(q, Cc, sizeof(double) * nC); q += nC;
  if (want_nlpd) { memcpy(q, P, sizeof(double) * nC); memcpy(q + nC, ld, sizeof(double) * K); }
  else memset(q, 0, sizeof(double) * (nC + K));
  double* d = ctx->win;
  HIP_TRY(ctx, hipMemcpyAsync(d, h.data(), nparam * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PredictArgs a{};
  a.Z = ctx->Z; a.N = N; a.dx = dx; a.dc = dc; a.dy = dy; a.K = K; a.mode = mode; a.diag = diag ? 1 : 0;
  a.gate = d; a.M = d + ng; a.Q = a.M + nM; a.Cc = a.Q + nQ; a.P = a.Cc + nC; a.ld = a.P + nC;
  double* out = d + nparam;
  if (dev_out) {
    a.mu = mu; a.covar = covar; a.nlpd = want_nlpd ? nlpd : nullptr;
  } else {
    a.mu = out; a.covar = out + (size_t)N * dy; a.nlpd = want_nlpd ? a.covar + (size_t)N * ncov : nullptr;
  }
  if (want_nlpd) {
    if (dev_in) {
      a.y = y;
    } else {
      double* yd = out + nout;
      HIP_TRY(ctx, hipMemcpyAsync(yd, y, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      a.y = yd;
    }
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // h (pageable) must be consumed before it goes away
  bool unsupported = false;
  rc = timed_launch(ctx, "predict_kernel", [&]() -> int {
    HIP_TRY(ctx, launch_predict(a, ctx->stream, &unsupported));
    return MIMO_OK;
  });
  if (rc) return rc;
  if (unsupported) return fail(ctx, MIMO_E_UNSUPPORTED, "mimo_predict: dy=%d (max %d) or dx=%d not supported", dy, kMaxPredictDy, dx);
  if (ctx->prof) ctx->prof_n += 1;
  if (dev_out) return MIMO_OK;
  if (N > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(mu, a.mu, (size_t)N * dy * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(covar, a.covar, (size_t)N * ncov * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (want_nlpd) HIP_TRY(ctx, hipMemcpyAsync(nlpd, a.nlpd, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}

// mimo_get_*: one of the tables a pass left on the device
enum class Kept { Resp, Logp, Lse, Labels };
static int get_kept(mimo_ctx* ctx, void* out, Kept which, const char* what) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  const size_t n = (size_t)table_rows(ctx);
  switch (which) {
    case Kept::Resp: return copy_out(ctx, out, ctx->resp, ctx->resp_K * n * sizeof(double), ctx->resp_valid, what);
    case Kept::Logp: return copy_out(ctx, out, ctx->logp, ctx->logp_K * n * sizeof(double), ctx->logp_valid, what);
    case Kept::Lse: return copy_out(ctx, out, ctx->lse, n * sizeof(double), ctx->lse_valid, what);
    default: return copy_out(ctx, out, ctx->labels, n * sizeof(int32_t), ctx->labels_valid, what);
  }
  });
}
int mimo_get_resp(mimo_ctx* ctx, double* out) { return get_kept(ctx, out, Kept::Resp, "mimo_get_resp"); }
int mimo_get_logp(mimo_ctx* ctx, double* out) { return get_kept(ctx, out, Kept::Logp, "mimo_get_logp"); }
int mimo_get_lse(mimo_ctx* ctx, double* out) { return get_kept(ctx, out, Kept::Lse, "mimo_get_lse"); }
int mimo_get_labels(mimo_ctx* ctx, int32_t* out) { return get_kept(ctx, out, Kept::Labels, "mimo_get_labels"); }
int mimo_get_resp_columns(mimo_ctx* ctx, const int64_t* cols, int64_t ncols, double* out) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (ncols < 0 || (ncols > 0 && (!cols || !out))) return fail(ctx, MIMO_E_INVALID, "mimo_get_resp_columns: bad arguments");
  if (!ctx->resp_valid || !ctx->resp) return fail(ctx, MIMO_E_STATE, "mimo_get_resp_columns: no responsibility table is resident");
  if (ncols == 0) return MIMO_OK;
  for (int64_t j = 0; j < ncols; ++j)
    if (cols[j] < 0 || cols[j] >= ctx->N) return fail(ctx, MIMO_E_INVALID, "mimo_get_resp_columns: column %lld outside [0, N)", (long long)cols[j]);
  const size_t K = (size_t)ctx->resp_K, words = (size_t)ncols + K * (size_t)ncols;      // indices | gathered block, in the staged-labels / weights workspace
  if ((rc = ctx->table_tmp.ensure(ctx, words))) return rc;
  int64_t* cols_d = reinterpret_cast<int64_t*>(ctx->table_tmp.p);
  double* out_d = ctx->table_tmp + ncols;
  HIP_TRY(ctx, hipMemcpyAsync(cols_d, cols, (size_t)ncols * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_gather_columns(ctx->resp, (int)K, ctx->N, cols_d, ncols, out_d, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, out_d, K * (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MIMO_OK;
  });
}
int mimo_nan_info(mimo_ctx* ctx, int64_t* n_bad, double* row_mask_out, int K, int64_t* label_counts) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (n_bad) *n_bad = ctx->n_bad;
    if (row_mask_out && ctx->N > 0) {
      if (ctx->n_bad > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(row_mask_out, ctx->row_mask, (size_t)ctx->N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      } else {
        for (int64_t i = 0; i < ctx->N; ++i) row_mask_out[i] = 1.0;
      }
    }
    if (label_counts) {
      if (K < 1 || K > 256) return fail(ctx, MIMO_E_INVALID, "mimo_nan_info: K = %d outside [1, 256]", K);
      for (int k = 0; k < K; ++k) label_counts[k] = 0;
      if (ctx->n_bad > 0) {
        if (ctx->bad_counts_K != K) return fail(ctx, MIMO_E_STATE, "mimo_nan_info: no label pass with K = %d has run on this data", K);
        unsigned long long h[256];
        HIP_TRY(ctx, hipMemcpyAsync(h, ctx->cnt_d + kCntLabels, (size_t)K * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < K; ++k) label_counts[k] = (int64_t)h[k];
      }
    }
    return MIMO_OK;
  });
}

int mimo_shader_clock_mhz(mimo_ctx* ctx, double* mhz) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (!mhz) return fail(ctx, MIMO_E_INVALID, "mimo_shader_clock_mhz: out is NULL");
    const int grid = ctx->num_cu * 4;
    if ((rc = ctx->partials.ensure(ctx, (size_t)grid * 2))) return rc;
    unsigned long long* d = reinterpret_cast<unsigned long long*>(ctx->partials.p);
    HIP_TRY(ctx, launch_clock_probe(d, grid, 20000, ctx->stream));      // ~0.3 ms of v_fma_f64 on every SIMD
    std::vector<unsigned long long> h((size_t)grid * 2);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> v;
    for (int g = 0; g < grid; ++g)
      if (h[2 * g + 1] > 0) v.push_back((double)h[2 * g] / (double)h[2 * g + 1] * 100.0);
    if (v.empty()) return fail(ctx, MIMO_E_HIP, "mimo_shader_clock_mhz: no samples");
    std::sort(v.begin(), v.end());
    *mhz = v[v.size() / 2];
    return MIMO_OK;
  });
}

int mimo_lane_exchange_selftest(mimo_ctx* ctx, int* mismatches) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (!mismatches) return fail(ctx, MIMO_E_INVALID, "mimo_lane_exchange_selftest: out is NULL");
    if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
    // round 0: distinct ordinary values; round 4: +0 in lanes of even bit count, -0 in the others, so that every mask pairs the two
    // zeros in both operand orders (the swaps hand the upper half its operands the other way round); rounds 1 .. 3: the values the kernels' reductions meet at their edges (-inf of masked slots,
    // -1e300 of padding components, the clamp of the exponential, denormals, both zeros), permuted so that every mask pairs unequal lanes
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    const double special[] = {-inf, -1e300, den, -den, 0.0, -0.0, 1.0, -707.0, 8e-308, 1.1e-308, -1.1e-308, 3.5, -inf, 0x1p-1074 * 5, -1e-300, 64.0, -0.0};
    constexpr int NS = (int)(sizeof special / sizeof special[0]), R = 5;
    std::vector<double> v(64 * R);
    std::vector<int> iv(64 * R);
    for (int r = 0; r < R; ++r)
      for (int l = 0; l < 64; ++l) {
        v[64 * r + l] = r == 0 ? 1.37 * l - 20.5 + 1e-9 * l * l : r == 4 ? (__builtin_popcount(l) & 1 ? -0.0 : 0.0) : special[(l * (2 * r + 5) + 3 * r) % NS];
        iv[64 * r + l] = r == 0 ? l : (int)(2654435761u * (unsigned)(64 * r + l + 1)) >> (r == 1 ? 3 : 8);      // (sums of two stay inside int)
      }
    if ((rc = ctx->partials.ensure(ctx, (size_t)64 * R + 32 * R + 1))) return rc;
    double* dv = ctx->partials;
    int* div = reinterpret_cast<int*>(dv + 64 * R);
    unsigned int* dout = reinterpret_cast<unsigned int*>(dv + 64 * R + 32 * R);
    HIP_TRY(ctx, hipMemcpyAsync(dv, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(div, iv.data(), iv.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(dout, 0, sizeof(double), ctx->stream));
    HIP_TRY(ctx, launch_lane_exchange_selftest(dv, div, R, dout, ctx->stream));
    unsigned int h = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h, dout, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *mismatches = (int)h;
    return MIMO_OK;
  });
}

int mimo_comm_unique_id(char* id128) {
  return guarded(nullptr, [&]() -> int {
    if (!id128) return fail(nullptr, MIMO_E_INVALID, "mimo_comm_unique_id: id is NULL");
    char msg[256];
    const int rc = mimo_comm::unique_id(id128, msg, sizeof msg);
    return rc ? fail(nullptr, rc, "%s", msg) : MIMO_OK;
  });
}

int mimo_comm_init(mimo_ctx* ctx, const char* id128, int rank, int world) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail(ctx, MIMO_E_INVALID, "mimo_comm_init: bad arguments");
    if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
    if (ctx->comm) { (void)mimo_comm::destroy(ctx->comm); ctx->comm = nullptr; }
    char msg[256];
    void* c = nullptr;
    if ((rc = mimo_comm::init(&c, id128, rank, world, msg, sizeof msg))) return fail(ctx, rc, "%s", msg);
    ctx->comm = c; ctx->comm_world = world;
    return MIMO_OK;
  });
}

int mimo_comm_destroy(mimo_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm) { (void)mimo_comm::destroy(ctx->comm); ctx->comm = nullptr; ctx->comm_world = 1; }
    return MIMO_OK;
  });
}

int mimo_debug_fault(mimo_ctx* ctx, int kind) {
  return guarded(ctx, [&]() -> int {
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) throw std::runtime_error("mimo_debug_fault");
    if (kind == 3) throw 42;
    return kind == 0 ? MIMO_OK : fail(ctx, MIMO_E_INVALID, "mimo_debug_fault: unknown kind %d", kind);
  });
}

int mimo_tune(mimo_ctx* ctx, const char* key, int64_t value) {
  return guarded(ctx, [&]() -> int {
    if (!ctx || !key) return fail(ctx, MIMO_E_INVALID, "mimo_tune: null argument");
    if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
    RouteTunables& t = g_route_tunables;     // process-wide, as sorted_range and narrow_big_vi (include/mimo_hip.h)
    const struct { const char* key; int max; int* knob; } keys[] = {
        {"num_cu", 4096, nullptr}, {"resp_skip_log2", 1000, &ctx->resp_skip_log2}, {"block_order", 1, &ctx->block_order_on}, {"estep_cert", 1, &ctx->cert_on}, {"sorted_range", 80, nullptr}, {"narrow_big_vi", 256, nullptr},
        {"mid_labels_narrow_k", 64, &t.mid_labels_narrow_k}, {"mid_labels_min_d", 64, &t.mid_labels_min_d},
        {"mid_narrow_k", 64, &t.mid_narrow_k}, {"mid_min_d", 64, &t.mid_min_d}};
    for (const auto& m : keys) {
      if (strcmp(key, m.key)) continue;
      if (value < 0 || value > m.max) return fail(ctx, MIMO_E_INVALID, "mimo_tune: %s = %lld outside [0, %d]", key, (long long)value, m.max);
      if (m.knob) {
        *m.knob = (int)value;
        if (m.knob == &ctx->block_order_on && !value) ctx->order_K = 0;     // switched off: an order in force goes with it
      }
      else if (!strcmp(key, "num_cu")) ctx->num_cu = value == 0 ? ctx->hw_num_cu : (int)value;
      else if (!strcmp(key, "sorted_range")) set_sorted_range_cap((int)value);
      else set_narrow_big_vi((int)value);
      return MIMO_OK;
    }
    return fail(ctx, MIMO_E_INVALID, "mimo_tune: unknown key '%s'", key);
  });
}

int mimo_estep_cert_info(mimo_ctx* ctx, int64_t* out6) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (!out6) return fail(ctx, MIMO_E_INVALID, "mimo_estep_cert_info: out is NULL");
    if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
    unsigned long long cnt[4] = {0, 0, 0, 0};
    if (ctx->cert_cnt.p) {
      HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->cert_cnt, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    out6[0] = ctx->cert_last; out6[1] = ctx->cert_valid ? 1 : 0; out6[2] = ctx->cert_age;
    out6[3] = (int64_t)cnt[0]; out6[4] = (int64_t)cnt[1]; out6[5] = (int64_t)cnt[2];
    return MIMO_OK;
  });
}

int mimo_estep_cert_proven_waves(mimo_ctx* ctx, int64_t* out) {
  return guarded(ctx, [&]() -> int {
    int rc = bind(ctx); if (rc) return rc;
    if (!out) return fail(ctx, MIMO_E_INVALID, "mimo_estep_cert_proven_waves: out is NULL");
    if (ctx->pending_async) return fail(ctx, MIMO_E_STATE, "an asynchronous call is pending: call mimo_wait first");
    unsigned long long cnt[4] = {0, 0, 0, 0};
    if (ctx->cert_cnt.p) {
      HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->cert_cnt, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    *out = (int64_t)cnt[3];
    return MIMO_OK;
  });
}

double mimo_philox_uniform(uint64_t seed, uint64_t row, uint64_t sweep) {
  return philox_uniform_host(seed, row, sweep);
}

int mimo_profile(mimo_ctx* ctx, int enable) {
  return guarded(ctx, [&]() -> int {
  if (!ctx) return fail(nullptr, MIMO_E_INVALID, "null context");
  ctx->prof = enable != 0;
  return MIMO_OK;
  });
}

int mimo_profile_read(mimo_ctx* ctx, double* kernel_ms, int64_t* launches, int reset) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  drain_profile(ctx);
  if (kernel_ms) *kernel_ms = ctx->prof_ms;
  if (launches) *launches = ctx->prof_n;
  if (reset) {
    ctx->prof_ms = 0.0; ctx->prof_n = 0;
    for (int i = 0; i < mimo_ctx::kProfNames; ++i) { ctx->prof_name_ms[i] = 0.0; ctx->prof_name_n[i] = 0; }
  }
  return MIMO_OK;
  });
}

int mimo_profile_kernels(mimo_ctx* ctx, char* buf, int len) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!buf || len < 1) return fail(ctx, MIMO_E_INVALID, "mimo_profile_kernels: no buffer");
  drain_profile(ctx);
  int off = 0;
  buf[0] = 0;
  for (int i = 0; i < mimo_ctx::kProfNames && ctx->prof_name[i]; ++i) {
    if (!ctx->prof_name_n[i]) continue;
    const int w = snprintf(buf + off, (size_t)(len - off), "%s\t%.6f\t%lld\n", ctx->prof_name[i], ctx->prof_name_ms[i],
                           (long long)ctx->prof_name_n[i]);
    if (w < 0 || w >= len - off) break;
    off += w;
  }
  return MIMO_OK;
  });
}

// The route of a plain pass (the one run_pass launches from) described without anything that needs a device: kind, launches, passes
// (out8[6] — the grid — stays 0), and a one-line description of the kernels (desc, may be null).  It prints what the Route, the
// TwoStagePlan and the LabelStatsPlan of the pass say and decides nothing itself.  The counters: out8[1] kernels per pass, out8[2] /
// out8[3] writes / reads of the (K, N) table, out8[4] / out8[5] passes over Z / the labels.  "Kernels per pass" counts the kernels that
// read Z and leaves out the helper launches: the label histogram and its reset, label_slots_kernel, the tile sort, the two reduction kernels.
static void plan_route(const mimo_ctx* ctx, const Route& route, const KernelArgs& a, int K, int gibbs, int64_t* out8, char* desc, size_t dlen) {
  const int ncb = a.F16 / 16, D = ctx->D;
  char lst[160] = "";           // the label-statistics stage of a label pass
  auto label_stage = [&]() {
    const LabelStatsPlan lp = label_stats_plan(K, D, ctx->structure, a.N);
    if (lp.kind == LabelStatsPlan::Windows) snprintf(lst, sizeof lst, "%s x %d", lp.name, lp.launches);
    else snprintf(lst, sizeof lst, "%s", lp.name);
    return lp.launches;
  };
  memset(out8, 0, 8 * sizeof(int64_t));
  out8[4] = 1;                           // passes over Z
  out8[5] = gibbs ? 1 : 0;               // passes over the labels
  const Family f = route.family;
  if (f == Family::Mid) {
    out8[0] = MIMO_PLAN_MID; out8[1] = 1;
    if (desc) snprintf(desc, dlen, "mid_kernel<Dz=%d, row blocks %d, %d waves>", D, (K + 15) / 16, mid_rows_per_step(K, D) / 16);
  } else if (f == Family::MidLabels) {
    const int ll = label_stage();
    out8[0] = MIMO_PLAN_MID; out8[1] = 1 + ll; out8[4] = 1 + ll; out8[5] = 1 + ll;
    if (desc) snprintf(desc, dlen, "mid_kernel<Dz=%d, row blocks %d, label draw> + %s", D, (K + 15) / 16, lst);
  } else if (f == Family::Narrow) {
    const int nm = route.narrow_mode;
    out8[0] = MIMO_PLAN_NARROW; out8[1] = nm == 2 ? 2 : 1;
    if (nm == 2) { out8[4] = 2; out8[5] = 2; }       // label kernel + label-statistics kernel (nm == 3: one kernel, labels written once)
    if (nm == 2) label_stage();
    if (desc) snprintf(desc, dlen, "narrow_kernel<%d slots, %d steps%s, %s>%s%s", narrow_v(K), narrow_steps(K, ctx->F, D, nm - 1),
                       narrow_dt(K, ctx->F, D, nm - 1) ? ", grouped" : "", nm == 1 ? "softmax + statistics" : nm == 2 ? "label draw" : "label draw + statistics",
                       nm == 2 ? " + " : "", nm == 2 ? lst : "");
  } else if (f == Family::Small) {
    out8[0] = MIMO_PLAN_SMALL; out8[1] = 1;
    if (desc) snprintf(desc, dlen, "small_kernel<%d components per lane, %d lanes per row>", small_kl(D, K), small_g(D, K));
  } else if (f == Family::RowwaveVi) {
    out8[0] = MIMO_PLAN_ROWWAVE_VI; out8[1] = 1;
    if (desc) snprintf(desc, dlen, "vi_rowwave_kernel<%d row blocks>", K <= 32 ? 2 : 4);
  } else if (f == Family::Rowwave) {
    const int ll = label_stage();     // (> 1: the sliced statistics of the large shapes)
    out8[0] = MIMO_PLAN_ROWWAVE; out8[1] = 1 + ll;
    out8[4] = 1 + ll;                    // Z: label kernel + every statistics launch
    out8[5] = 1 + ll;                    // labels written once, read once per statistics launch
    if (desc) snprintf(desc, dlen, "%s<%d row blocks> + %s", gibbs_rowwave_counts_labels(K, ctx->F16, a.ZS) ? "gibbs_rowwave_kernel" : "gibbs_stream_kernel",
                       rowwave_kb_shape(K, ctx->F16, a.ZS), lst);
  } else if (f == Family::Fused) {
    out8[0] = MIMO_PLAN_FUSED; out8[1] = 1;
    if (desc) snprintf(desc, dlen, "fused_kernel<%d column blocks, %d row block%s per wave%s>", ncb, a.K16 <= 4 ? 1 : a.K16 <= 8 ? 2 : a.K16 <= 12 ? 3 : 4,
                       a.K16 <= 4 ? "" : "s", K <= 32 && D >= 7 ? ", work split over the waves" : "");
  } else {
    const TwoStagePlan ts = two_stage_plan(route, a, ctx->structure, kSrcEstep);
    const char* est = ts.estep == TwoStagePlan::Wide ? "wide_estep_kernel" : "estep_chunked_kernel";
    const int groups = ts.groups;
    out8[0] = MIMO_PLAN_TWO_STAGE;
    if (ts.stats == TwoStagePlan::LabelStats) {      // label-indexed statistics
      const int ll = label_stage();
      out8[1] = 1 + ll; out8[4] = 1 + ll; out8[5] = 1 + ll;
      if (desc) snprintf(desc, dlen, "%s (label draw) + %s", est, lst);
    } else {
      out8[1] = 1 + groups;
      out8[2] = gibbs ? 0 : 1;             // the (K, N) responsibility table goes through HBM
      out8[3] = gibbs ? 0 : groups;        // and is read once per statistics launch
      out8[4] = 1 + groups;                // Z: the E-step + every statistics launch
      out8[5] = gibbs ? 1 + groups : 0;
      if (desc) snprintf(desc, dlen, "%s (%s) + %s x %d", est, gibbs ? "label draw" : "softmax -> (K, N) table",
                         ts.stats == TwoStagePlan::WideColumns ? "wide_stats_kernel" : "fused_kernel (statistics)", groups);
    }
  }
}

int mimo_plan(mimo_ctx* ctx, int K, int gibbs, int64_t* out8) {
  return guarded(ctx, [&]() -> int {
  int rc = bind(ctx); if (rc) return rc;
  if (!out8) return fail(ctx, MIMO_E_INVALID, "mimo_plan: out is NULL");
  if (!ctx->Z) return fail(ctx, MIMO_E_NODATA, "no data uploaded or attached");
  if ((rc = single_only(ctx))) return rc;
  if (K < 1 || K > 256) return fail(ctx, MIMO_E_UNSUPPORTED, "K = %d outside [1, 256]", K);
  KernelArgs a;
  fill_args(ctx, K, &a);
  a.gibbs = gibbs ? 1 : 0;
  const Route route = route_for(ctx, K, {kSrcEstep, gibbs != 0});
  plan_route(ctx, route, a, K, gibbs, out8, nullptr, 0);
  if (order_applies(ctx, route, a)) out8[0] |= MIMO_PLAN_ORDERED;
  out8[6] = route_grid(route, two_stage_plan(route, a, ctx->structure, kSrcEstep), a, ctx->num_cu, ctx->F, kSrcEstep);
  out8[7] = ctx->num_cu;
  return MIMO_OK;
  });
}

int mimo_plan_shape(int Dz, int K, int structure, int64_t N, int gibbs, int64_t* out8, char* desc, int desc_len) {
  return guarded(nullptr, [&]() -> int {
  if (!out8) return fail(nullptr, MIMO_E_INVALID, "mimo_plan_shape: out is NULL");
  if (Dz < 1 || Dz > kMaxD || K < 1 || K > 256 || N < 0 || structure < 0 || structure > 2)
    return fail(nullptr, MIMO_E_UNSUPPORTED, "mimo_plan_shape: Dz = %d, K = %d, structure = %d outside the library's range", Dz, K, structure);
  mimo_ctx ctx;                        // a description of the data, never a device context: no HIP call below
  alignas(16) static const double aligned_rows[2] = {0.0, 0.0};
  ctx.Z = aligned_rows; ctx.N = N; ctx.D = Dz; ctx.structure = structure;
  ctx.F = structure == MIMO_STRUCT_DIAG ? diag_feat_count(Dz) : structure == MIMO_STRUCT_LINEAR ? lin_feat_count(Dz) : feat_count(Dz);
  ctx.F16 = (ctx.F + 15) / 16 * 16;
  KernelArgs a;
  fill_args(&ctx, K, &a);
  a.gibbs = gibbs ? 1 : 0;
  if (desc && desc_len > 0) desc[0] = 0;
  plan_route(&ctx, route_for(&ctx, K, {kSrcEstep, gibbs != 0}), a, K, gibbs, out8, desc, desc && desc_len > 0 ? (size_t)desc_len : 0);
  return MIMO_OK;
  });
}

}  // extern "C"
