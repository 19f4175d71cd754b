// Device-resident batched VI (gfx950): what stands between two batched softmax passes of B mixtures of Gaussians — the conjugate
// update of the K Normal-Wishart blocks and of the Dirichlet gating from the resident statistics, the canonical form (c, b, W) as
// the operand image the next pass reads, the prior terms of the bound and the stopping rule — as three small kernels, so that a
// whole mean-field iteration is five stream-ordered launches and no host round trip:
//
//   vi_update_kernel   one wave per (problem, component): the arithmetic of mimo_host_gmm_vi_sweep + mimo_host_nw_vi + one
//                      component of mimo_host_nw_vlb (mimo_host.cpp), the Dz x Dz block in LDS
//   vi_gating_kernel   one wave per problem: the Dirichlet update, E[log pi], c_total into the image, the Dirichlet term of
//                      mimo_host_gmm_vi_bound and the sum of the component terms
//   (launch_batched, launch_batched_reduce: the pass and its reduction, mimo_batched.hip)
//   vi_finish_kernel   one lane per problem: the bound into the trace, the stopping rule
//
// The update and the gating kernel are templates over the mode (ViMode): the conjugate update above, the SVI blend of the current
// slot's natural parameters with it, or the derived parts of an uploaded posterior; svi_indices_kernel draws the minibatch indices
// of the SVI loop (mimo_svi_run_batched).
//
// All float64, plain launches, no atomics.  Every sum runs in a fixed order that depends on (K, Dz) alone and every workgroup
// works on one problem, so a problem's numbers do not depend on what else is in the batch, bit for bit (the batch's determinism
// rule, mimo_batched.hip).  A problem that has stopped is skipped by the update and the gating kernel: its posterior block and
// its operand image stay exactly as they are.  A problem whose status word is set is skipped too and keeps the posterior block
// of its last complete iteration (the blocks are double-buffered); its operand image and its resident statistics are undefined
// from then on: the other components' workgroups of the failing iteration may or may not have written their entries.
//
// Reference semantics: those the host routines cite — mimo/distributions/composite.py:50-72,106-128 (Normal-Wishart),
// wishart.py:139-143, dirichlet.py:31-33,78-97, bayesian.py:78-83, mixtures/gmm.py:275-285.
#include "mimo_vi_batched.h"
#include "mimo_batched.h"
#include "mimo_device.h"

#include <math.h>

namespace mimo {

namespace {

constexpr double kViLog2Pi = 1.8378770664093454835606594728112;
constexpr double kViLog2 = 0.69314718055994530941723212145818;
constexpr double kViLogPi = 1.1447298858494001741434273513531;
constexpr long long kViNanBits = 0x7ff8000000000000LL;     // (integer selects: the kernels are built with -fno-honor-nans)
constexpr int kViLd = 17;                                  // LDS row stride of the Dz x Dz blocks (Dz <= 16)

__device__ __forceinline__ bool vi_pos_finite(double v) {
  const long long b = __double_as_longlong(v);
  return b > 0 && b < 0x7ff0000000000000LL;
}

__device__ __forceinline__ bool vi_finite(double v) {
  return (__double_as_longlong(v) & 0x7fffffffffffffffLL) < 0x7ff0000000000000LL;
}

// psi(x) for x > 0: the host routine's algorithm (mimo_host.cpp: recurrence up to x >= 10, then the asymptotic series).  Anything
// else (zero, negative, NaN, infinity) returns NaN at once: the recurrence would not end on a large negative argument.
__device__ double vi_digamma(double x) {
  if (!vi_pos_finite(x)) return __longlong_as_double(kViNanBits);
  double r = 0.0;
  while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
  const double f = 1.0 / (x * x);
  const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 + f * (-1.0 / 132.0
                   + f * (691.0 / 32760.0 + f * (-1.0 / 12.0)))))));
  return r + log(x) - 0.5 / x + t;
}

// feature of the pair (a, b), a <= b <= D, in the full map (feat_index of mimo_kernels.h)
__device__ __forceinline__ int vi_feat(int D, int a, int b) { return a * (D + 1) - a * (a - 1) / 2 + (b - a); }

// offset of entry (k, feature f) in one problem's image: ThetaGeneric::at (mimo_theta.h) with the identity order
__device__ __forceinline__ size_t vi_theta_at(int NS, int k, int f) {
  return ((size_t)(k >> 4) * NS + (f >> 2)) * 64 + (f & 3) * 16 + (k & 15);
}

template <int M>
__global__ __launch_bounds__(64) void vi_update_kernel(const ViArgs a) {
  __shared__ double Qc[16 * kViLd];     // c of the posterior's natural parameters
  __shared__ double U[16 * kViLd];      // C = c - kappa m m' -> its upper Cholesky factor
  __shared__ double X[16 * kViLd];      // U^-1
  __shared__ double Wm[16 * kViLd];     // W = nu psi
  __shared__ double vec[8][16];         // m, qa, pa, b, digamma terms, lgamma terms, row sums <qc, W>, <pc, W>
  double* const mv = vec[0];
  double* const qav = vec[1];
  double* const pav = vec[2];
  double* const bv = vec[3];
  double* const dgv = vec[4];
  double* const lgv = vec[5];
  double* const rqv = vec[6];
  double* const rpv = vec[7];

  const int lane = threadIdx.x;
  const int B = a.B, K = a.K, D = a.D, DD = D * D;
  const int prob = blockIdx.x / K, k = blockIdx.x - prob * K;
  if (!a.words[kViActive * B + prob] || a.words[kViStatus * B + prob]) return;
  const int cur = a.words[kViSlot * B + prob], slot = 1 - cur;
  const ViLayout L{K, D};
  double* const P = a.post + ((size_t)slot * B + prob) * L.count();
  const double* const C = a.post + ((size_t)cur * B + prob) * L.count();      // the current block (read in the blend and init modes)
  const size_t bk = (size_t)prob * K + k;
  const double* const Sk = a.S + bk * (size_t)(1 + D + DD);
  const double* const pck = a.pc + bk * DD;
  const double rho = a.rho, omr = a.one_minus_rho;
  double inv = 0.0;
  if constexpr (M == kViBlend) inv = a.inv_scale[prob];

  // eta_post = eta_prior + statistics (conjugate), or the mode's form of it (vi_eta)
  const double n = vi_stat<M>(Sk, 0);
  const double pb = a.pb[bk], pd = a.pd[bk];
  const double qb = vi_eta<M>(pb, n, vi_cur<M>(C, L.qb() + k), rho, omr, inv);
  const double qd = vi_eta<M>(pd, n, vi_cur<M>(C, L.qd() + k), rho, omr, inv);
  const int ej = lane & 15, ei0 = lane >> 4;        // element (ei0 + 4 r, ej) of a Dz x Dz block, r = 0 .. 3
  if (lane < D) {
    const double p = a.pa[bk * D + lane];
    const double q = vi_eta<M>(p, vi_stat<M>(Sk, 1 + lane), vi_cur<M>(C, L.qa() + k * D + lane), rho, omr, inv);
    pav[lane] = p;
    qav[lane] = q;
    mv[lane] = q / qb;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D)
      Qc[i * kViLd + ej] = vi_eta<M>(pck[i * D + ej], vi_stat<M>(Sk, 1 + D + i * D + ej), vi_cur<M>(C, L.qc() + k * DD + i * D + ej),
                                     rho, omr, inv);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) U[i * kViLd + ej] = Qc[i * kViLd + ej] - qb * mv[i] * mv[ej];
  }
  wg_sync();

  // upper Cholesky C = U'U, right-looking (spd_inverse4 of mimo_host.cpp, one matrix per wave)
  bool bad = false;
  double sl = 0.0;
  for (int j = 0; j < D; ++j) {
    double d = U[j * kViLd + j];
    if (!vi_pos_finite(d)) { bad = true; d = 1.0; }
    const double piv = sqrt(d);
    sl += log(piv);
    const double inv = 1.0 / piv;
    wg_sync();
    if (lane >= j && lane < D) U[j * kViLd + lane] *= inv;
    wg_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ei0 + 4 * r;
      if (i > j && i < D && ej >= i && ej < D) U[i * kViLd + ej] -= U[j * kViLd + i] * U[j * kViLd + ej];
    }
    wg_sync();
  }
  if (bad) {      // (uniform: every lane read the same pivots)
    if (lane == 0) atomicOr(&a.words[kViStatus * B + prob], kViNotPosDef);
    return;
  }

  // X = U^-1 by row back-substitution: lane c owns column c (it reads only entries of X it wrote itself)
  if (lane < D) {
    const int c = lane;
    for (int i = c; i >= 0; --i) {
      double x = i == c ? 1.0 : 0.0;
      for (int kk = i + 1; kk <= c; ++kk) x -= U[i * kViLd + kk] * X[kk * kViLd + c];
      X[i * kViLd + c] = x * (1.0 / U[i * kViLd + i]);
    }
  }
  wg_sync();

  // psi = C^-1 = X X' (entry (i, j) and its mirror run the same chain: psi is symmetric bit for bit), W = nu psi
  const double nu = qd + D;
  double psi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    psi[r] = 0.0;
    if (i < D && ej < D) {
      double v = 0.0;
      for (int c = i > ej ? i : ej; c < D; ++c) v += X[i * kViLd + c] * X[ej * kViLd + c];
      psi[r] = v;
      Wm[i * kViLd + ej] = nu * v;
    }
  }
  wg_sync();

  // per row: b = W m, <qc, W>, <pc, W>; the digamma and lgamma terms
  if (lane < D) {
    const int i = lane;
    double s = 0.0, rq = 0.0, rp = 0.0;
    for (int j = 0; j < D; ++j) {
      const double w = Wm[i * kViLd + j];
      s += w * mv[j];
      rq += Qc[i * kViLd + j] * w;
      rp += pck[i * D + j] * w;
    }
    bv[i] = s;
    rqv[i] = rq;
    rpv[i] = rp;
    dgv[i] = vi_digamma(0.5 * (nu - i));
    lgv[i] = lgamma(0.5 * nu - 0.5 * i);
  }
  wg_sync();

  // the scalars, on every lane alike (ascending sums of at most 16 terms)
  double mWm = 0.0, dg = 0.0, mg = 0.25 * D * (D - 1) * kViLogPi, qaE1 = 0.0, paE1 = 0.0, qcW = 0.0, pcW = 0.0;
  for (int i = 0; i < D; ++i) {
    mWm += mv[i] * bv[i];
    dg += dgv[i];
    mg += lgv[i];
    qaE1 += qav[i] * bv[i];
    paE1 += pav[i] * bv[i];
    qcW += rqv[i];
    pcW += rpv[i];
  }
  const double hld = -sl;
  const double E2 = -0.5 * (D / qb + mWm);
  const double E4 = 0.5 * (dg + D * kViLog2 + 2.0 * hld);
  const double cc = -0.5 * D * kViLog2Pi + E2 + E4;
  // the component's term of the bound (mimo_host_nw_vlb)
  const double log_base = -0.5 * D * kViLog2Pi;
  const double logZq = -0.5 * D * log(qb) + (0.5 * nu * D * kViLog2 + mg + nu * hld);
  const double iq = qaE1 + qb * E2 - 0.5 * qcW + qd * E4;
  const double ip = paE1 + pb * E2 - 0.5 * pcW + pd * E4;
  const double term = (logZq - log_base - iq) - (a.plz[bk] - log_base - ip);

  // a canonical form or a term that is not finite (a digamma argument <= 0, an overflow): the host packing path refuses such a
  // block (theta_entries), here it sets the problem's status and, like a bad pivot, writes nothing for this component
  bool lane_bad = lane < D && !vi_finite(bv[lane]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D && !vi_finite(Wm[i * kViLd + ej])) lane_bad = true;
  }
  if (__any(lane_bad) || !vi_finite(cc) || !vi_finite(term)) {
    if (lane == 0) atomicOr(&a.words[kViStatus * B + prob], kViNotFinite);
    return;
  }

  // ---- outputs: the posterior block, the term, the b / W entries of the operand image ---------------------------------------
  double* const th = a.theta + (size_t)prob * a.K16 * a.NS * 64;
  if (lane < D) {
    P[L.qa() + k * D + lane] = qav[lane];
    P[L.mus() + k * D + lane] = mv[lane];
    P[L.bb() + k * D + lane] = bv[lane];
    th[vi_theta_at(a.NS, k, vi_feat(D, lane, D))] = bv[lane];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) {
      const int e = k * DD + i * D + ej;
      const double w = Wm[i * kViLd + ej];
      P[L.qc() + e] = Qc[i * kViLd + ej];
      P[L.psis() + e] = psi[r];
      P[L.W() + e] = w;
      if (i == ej) th[vi_theta_at(a.NS, k, vi_feat(D, i, i))] = -0.5 * w;
      else if (i < ej) th[vi_theta_at(a.NS, k, vi_feat(D, i, ej))] = -0.5 * (w + Wm[ej * kViLd + i]);
    }
  }
  if (lane == 0) {
    P[L.qb() + k] = qb;
    P[L.qd() + k] = qd;
    P[L.nus() + k] = nu;
    P[L.hld() + k] = hld;
    P[L.cc() + k] = cc;
    P[L.E2() + k] = E2;
    P[L.E4() + k] = E4;
    a.term[bk] = term;
  }
}

template <int M>
__global__ __launch_bounds__(64) void vi_gating_kernel(const ViArgs a) {
  // alpha, alpha0, lgamma(alpha), lgamma(alpha0), (alpha - 1) E, (alpha0 - 1) E, terms, E[log pi], c_total
  __shared__ double t[9][kBatchedMaxK];
  __shared__ double red[8];
  const int lane = threadIdx.x;
  const int B = a.B, K = a.K, D = a.D;
  const int prob = blockIdx.x;
  if (!a.words[kViActive * B + prob] || a.words[kViStatus * B + prob]) return;
  const int cur = a.words[kViSlot * B + prob], slot = 1 - cur;
  const ViLayout L{K, D};
  double* const P = a.post + ((size_t)slot * B + prob) * L.count();
  const double* const C = a.post + ((size_t)cur * B + prob) * L.count();      // the current block (read in the blend and init modes)
  const size_t sstride = (size_t)(1 + D + D * D);
  double inv = 0.0;
  if constexpr (M == kViBlend) inv = a.inv_scale[prob];

  // Dirichlet gating: alpha = ((alpha0 - 1) + n) + 1; the blend runs on the natural parameter alpha - 1 (gating.py: std_to_nat /
  // nat_to_std around CategoricalWithDirichlet.meanfield_sgd); init keeps the uploaded alpha itself
  for (int k = lane; k < K; k += 64) {
    const size_t bk = (size_t)prob * K + k;
    const double a0 = a.alpha0[bk];
    if constexpr (M == kViInit) t[0][k] = C[L.alpha() + k];
    else t[0][k] = vi_eta<M>(a0 - 1.0, a.S[bk * sstride], vi_cur<M>(C, L.alpha() + k) - 1.0, a.rho, a.one_minus_rho, inv) + 1.0;
    t[1][k] = a0;
  }
  wg_sync();
  double s = 0.0, s0 = 0.0;
  for (int k = 0; k < K; ++k) { s += t[0][k]; s0 += t[1][k]; }      // on every lane alike, ascending
  const double ds = vi_digamma(s);
  double* const th = a.theta + (size_t)prob * a.K16 * a.NS * 64;
  const int fdd = vi_feat(D, D, D);
  bool lane_bad = false;
  for (int k = lane; k < K; k += 64) {
    const double al = t[0][k], a0 = t[1][k];
    const double elp = vi_digamma(al) - ds;
    const double ct = P[L.cc() + k] + elp;
    lane_bad = lane_bad || !vi_finite(elp) || !vi_finite(ct);
    t[7][k] = elp;
    t[8][k] = ct;
    t[2][k] = lgamma(al);
    t[3][k] = lgamma(a0);
    t[4][k] = (al - 1.0) * elp;
    t[5][k] = (a0 - 1.0) * elp;
    t[6][k] = a.term[(size_t)prob * K + k];
  }
  if (__any(lane_bad)) {                     // (alpha <= 0: theta_entries refuses a NaN c) nothing of the gating is written
    if (lane == 0) atomicOr(&a.words[kViStatus * B + prob], kViNotFinite);
    return;
  }
  for (int k = lane; k < K; k += 64) {       // (each lane reads back what it wrote itself)
    const double ct = t[8][k];
    P[L.alpha() + k] = t[0][k];
    P[L.elp() + k] = t[7][k];
    P[L.c_total() + k] = ct;
    th[vi_theta_at(a.NS, k, fdd)] = ct < kPadLogDensity ? kPadLogDensity : ct;      // (theta_entries of mimo_theta.h; ct is finite)
  }
  for (int k = K + lane; k < 16 * a.K16; k += 64) th[vi_theta_at(a.NS, k, fdd)] = kPadLogDensity;
  wg_sync();
  if (lane < 5) {                            // lq, lp, iq, ip, the component terms: ascending k, one sum per lane
    double v = 0.0;
    for (int k = 0; k < K; ++k) v += t[2 + lane][k];
    red[lane] = v;
  }
  wg_sync();
  if (lane == 0) {
    const double dir = ((red[0] - lgamma(s)) - red[2]) - ((red[1] - lgamma(s0)) - red[3]);
    if (!vi_finite(dir + red[4])) {          // the slot does not become current
      atomicOr(&a.words[kViStatus * B + prob], kViNotFinite);
      return;
    }
    P[L.vlb()] = dir;
    P[L.vlb() + 1] = red[4];
    a.prior_terms[prob] = dir + red[4];
    a.words[kViSlot * B + prob] = slot;      // the block just written is the problem's current one
  }
}

__global__ __launch_bounds__(256) void vi_finish_kernel(const ViArgs a, int it) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int B = a.B;
  if (b >= B) return;
  double v = __longlong_as_double(kViNanBits);
  if (a.words[kViActive * B + b] && !a.words[kViStatus * B + b]) {
    v = a.prior_terms[b] + a.scalars[3 * b];
    if (!vi_finite(v)) {                     // (the pass overflowed) nothing is appended
      a.words[kViStatus * B + b] |= kViNotFinite;
      v = __longlong_as_double(kViNanBits);
    } else {
      const int total = a.words[kViTotal * B + b];
      if (total >= 1 && fabs(v - a.last[b]) < a.tol) a.words[kViActive * B + b] = 0;
      a.last[b] = v;
      a.words[kViTotal * B + b] = total + 1;
      a.words[kViDone * B + b] += 1;
    }
  }
  a.trace[(size_t)it * B + b] = v;
}

// one lane per (iteration, problem, slot): the grid's x runs over the slots of one iteration, y over the iterations
__global__ __launch_bounds__(256) void svi_indices_kernel(int64_t* sel, const int64_t* sel_off, const int64_t* row_off,
                                                          const uint64_t* seeds, int B, int64_t per_it, uint64_t t0) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_it) return;
  int lo = 0, hi = B - 1;                      // the problem whose slots hold e: the last b with sel_off[b] <= e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sel_off[mid] <= e) lo = mid; else hi = mid - 1;
  }
  const int64_t nb = row_off[lo + 1] - row_off[lo];
  if (nb < 1) return;                          // (refused by the caller)
  const int64_t j = e - sel_off[lo];
  const double u = philox_uniform(seeds[lo], (uint64_t)j, t0 + blockIdx.y);
  int64_t idx = (int64_t)(u * (double)nb);
  if (idx > nb - 1) idx = nb - 1;
  sel[(int64_t)blockIdx.y * per_it + e] = idx;
}

// (the init mode reads no statistics; the blend reads one factor per problem)
bool vi_args_ok(const ViArgs& a) {
  if (a.mode != kViConjugate && a.mode != kViBlend && a.mode != kViInit) return false;
  if (a.mode == kViBlend && !a.inv_scale) return false;
  return a.B >= 1 && a.K >= 1 && a.K <= kBatchedMaxK && a.D >= 1 && a.D <= 16 && a.K16 == (a.K + 15) / 16 && a.NS >= 1 &&
         (a.S || a.mode == kViInit) && (a.scalars || a.mode == kViInit) && a.alpha0 && a.pa && a.pb && a.pc && a.pd && a.plz &&
         a.post && a.term && a.prior_terms && a.last && a.words && a.theta && a.trace;
}

}  // namespace

hipError_t launch_vi_update(const ViArgs& a, hipStream_t stream) {
  if (!vi_args_ok(a) || (int64_t)a.B * a.K > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.B * a.K));
  if (a.mode == kViBlend) hipLaunchKernelGGL(vi_update_kernel<kViBlend>, grid, dim3(64), 0, stream, a);
  else if (a.mode == kViInit) hipLaunchKernelGGL(vi_update_kernel<kViInit>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(vi_update_kernel<kViConjugate>, grid, dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_vi_gating(const ViArgs& a, hipStream_t stream) {
  if (!vi_args_ok(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.B);
  if (a.mode == kViBlend) hipLaunchKernelGGL(vi_gating_kernel<kViBlend>, grid, dim3(64), 0, stream, a);
  else if (a.mode == kViInit) hipLaunchKernelGGL(vi_gating_kernel<kViInit>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(vi_gating_kernel<kViConjugate>, grid, dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_vi_finish(const ViArgs& a, int it, hipStream_t stream) {
  if (!vi_args_ok(a) || it < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vi_finish_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, stream, a, it);
  return hipGetLastError();
}

hipError_t launch_svi_indices(int64_t* sel, const int64_t* sel_off, const int64_t* row_off, const uint64_t* seeds, int B, int n_it,
                              int64_t per_it, uint64_t t0, hipStream_t stream) {
  if (!sel || !sel_off || !row_off || !seeds || B < 1 || n_it < 0 || n_it > 65535 || per_it < 0 ||
      (per_it + 255) / 256 > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  if (n_it == 0 || per_it == 0) return hipSuccess;
  hipLaunchKernelGGL(svi_indices_kernel, dim3((unsigned)((per_it + 255) / 256), (unsigned)n_it), dim3(256), 0, stream, sel, sel_off,
                     row_off, seeds, B, per_it, t0);
  return hipGetLastError();
}

}  // namespace mimo
