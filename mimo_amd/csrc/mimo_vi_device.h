// Device code the resident loops share (mimo_vi_batched.hip, mimo_vi_ilr_batched.hip; included by those two only): the constants
// and predicates, the entry of the natural parameters in a mode (vi_eta), the problem prologue of the update and gating kernels,
// the Cholesky inverse of a small block, the Normal-Wishart block of one (problem, component) on one wave (vi_nw_block) with its
// store, and the writers of the operand image's b / W and c_total entries.
#pragma once
#include "mimo_vi_batched.h"
#include "mimo_batched.h"
#include "mimo_device.h"

#include <math.h>
#include <type_traits>

namespace mimo {

namespace {

constexpr double kViLog2Pi = 1.8378770664093454835606594728112;
constexpr double kViLog2 = 0.69314718055994530941723212145818;
constexpr double kViLogPi = 1.1447298858494001741434273513531;
constexpr long long kViNanBits = 0x7ff8000000000000LL;     // (integer selects: the kernels are built with -fno-honor-nans)
constexpr int kViLd = 17;                                  // LDS row stride of the small blocks (every side <= 16)
constexpr int kViBlk = 16 * kViLd;

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

// One entry of the posterior's natural parameters in mode M (ViMode): prior + s as the conjugate update always
// formed it; the current entry; or the SVI blend in the operation order of _ConjugateBlock._apply_sgd and the gatings'
// meanfield_sgd (distributions/bayesian.py), with contraction off so that no product is fused into the add behind it
template <int M>
__device__ __forceinline__ double vi_eta(double prior, double s, double cur, double rho, double omr, double inv) {
  if constexpr (M == kViConjugate) {
    return prior + s;
  } else if constexpr (M == kViInit) {
    return cur;
  } else {
#pragma clang fp contract(off)
    const double t = inv * s;
    const double u = prior + t;
    const double v = rho * u;
    const double w = omr * cur;
    return w + v;
  }
}
// what vi_eta reads beside the prior: entry i of the current block (not in the conjugate mode), of the statistics (not in the init mode)
template <int M>
__device__ __forceinline__ double vi_cur(const double* C, size_t i) {
  if constexpr (M == kViConjugate) return 0.0; else return C[i];
}
template <int M>
__device__ __forceinline__ double vi_stat(const double* S, size_t i) {
  if constexpr (M == kViInit) return 0.0; else return S[i];
}

// The prologue of the update and gating kernels for problem `prob`, whose posterior block holds `count` doubles: false (the
// kernel returns at once) when the problem is not active or its status word is set; else P, the block being written (the slot
// that is not current), C, the current one (read in the blend and init modes), and the blend's 1 / scale.
struct ViProblem {
  double* P;
  const double* C;
  int slot;
  double inv;
};
template <int M>
__device__ __forceinline__ bool vi_problem(const ViLoop& l, int prob, int count, ViProblem& p) {
  if (!l.words[kViActive * l.B + prob] || l.words[kViStatus * l.B + prob]) return false;
  const int cur = l.words[kViSlot * l.B + prob];
  p.slot = 1 - cur;
  p.P = l.post + ((size_t)p.slot * l.B + prob) * count;
  p.C = l.post + ((size_t)cur * l.B + prob) * count;
  p.inv = 0.0;
  if constexpr (M == kViBlend) p.inv = l.inv_scale[prob];
  return true;
}

// a status bit of problem `prob`: nothing of this workgroup is written, and the slot does not become current
__device__ __forceinline__ void vi_fail(const ViLoop& l, int prob, int lane, int bit) {
  if (lane == 0) atomicOr(&l.words[kViStatus * l.B + prob], bit);
}

// The n x n block in U (its upper triangle is read) -> its upper Cholesky factor U'U in place (right-looking: spd_inverse4 of
// mimo_host.cpp, one matrix per wave), X = U^-1, `sl` the sum of the pivots' logarithms.  One wave; false when a pivot is not
// positive and finite (uniform: every lane reads the same pivots).  The inverse is then X X'.
__device__ bool vi_chol_inv(double* U, double* X, int n, int lane, double& sl) {
  const int ej = lane & 15, ei0 = lane >> 4;
  bool bad = false;
  sl = 0.0;
  for (int j = 0; j < n; ++j) {
    double d = U[j * kViLd + j];
    if (!vi_pos_finite(d)) { bad = true; d = 1.0; }
    const double piv = sqrt(d);
    sl += log(piv);
    const double inv = 1.0 / piv;
    wg_sync();
    if (lane >= j && lane < n) U[j * kViLd + lane] *= inv;
    wg_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ei0 + 4 * r;
      if (i > j && i < n && ej >= i && ej < n) U[i * kViLd + ej] -= U[j * kViLd + i] * U[j * kViLd + ej];
    }
    wg_sync();
  }
  if (bad) return false;
  // row back-substitution: lane c owns column c (it reads only entries of X it wrote itself)
  if (lane < n) {
    const int c = lane;
    for (int i = c; i >= 0; --i) {
      double x = i == c ? 1.0 : 0.0;
      for (int kk = i + 1; kk <= c; ++kk) x -= U[i * kViLd + kk] * X[kk * kViLd + c];
      X[i * kViLd + c] = x * (1.0 / U[i * kViLd + i]);
    }
  }
  wg_sync();
  return true;
}

// entry (i, j) of X X' (entry (i, j) and its mirror run the same chain: the product is symmetric bit for bit)
__device__ __forceinline__ double vi_xxt(const double* X, int n, int i, int j) {
  double v = 0.0;
  for (int c = i > j ? i : j; c < n; ++c) v += X[i * kViLd + c] * X[j * kViLd + c];
  return v;
}

// ---- the Normal-Wishart block of one (problem, component) on one wave -----------------------------------------------------------
// The arithmetic of mimo_host_nw_vi and one component of mimo_host_nw_vlb (mimo_host.cpp) on an n x n block, n <= 16.
struct ViNwIn {
  const double* pa; const double* pb; const double* pc; const double* pd; const double* plz;   // this component's prior entries
  const double* s0;           // the statistics: n,
  const double* sx;           //   sum r x (n entries),
  const double* sxx;          //   sum r x x' with the row stride `stride`
  int stride;
  const double* C;            // the problem's current block, its parts at `N` (blend and init modes)
  ViNwLayout N;
  int k, n;
  double rho, omr, inv;
};
// the caller's LDS: four blocks and eight vectors of 16 (m, qa, pa, b, digamma terms, lgamma terms, row sums <qc, W>, <pc, W>)
struct ViNwLds {
  double* Qc;                 // c of the posterior's natural parameters
  double* U;                  // C = c - kappa m m' -> its upper Cholesky factor
  double* X;                  // U^-1
  double* W;                  // W = nu psi
  double (*vec)[16];
  __device__ double* m() const { return vec[0]; }
  __device__ double* qa() const { return vec[1]; }
  __device__ double* b() const { return vec[3]; }
};
struct ViNwOut {
  double n;                   // the count the block read (0 in the init mode)
  double qb, qd, nu, hld, E2, E4, cc, term;
  double psi[4];              // psi of element (lane / 16 + 4 r, lane % 16), r = 0 .. 3
};

// false on a pivot that is not positive and finite (nothing of `o` is then defined)
template <int M>
__device__ __forceinline__ bool vi_nw_block(const ViNwIn& in, const ViNwLds& s, int lane, ViNwOut& o) {
  double* const mv = s.vec[0];
  double* const qav = s.vec[1];
  double* const pav = s.vec[2];
  double* const bv = s.vec[3];
  double* const dgv = s.vec[4];
  double* const lgv = s.vec[5];
  double* const rqv = s.vec[6];
  double* const rpv = s.vec[7];
  const int D = in.n, k = in.k;
  const ViNwLayout& N = in.N;
  const double* const C = in.C;
  const double rho = in.rho, omr = in.omr, inv = in.inv;

  // eta_post = eta_prior + statistics (conjugate), or the mode's form of it (vi_eta)
  const double n = vi_stat<M>(in.s0, 0);
  const double pb = *in.pb, pd = *in.pd;
  const double qb = vi_eta<M>(pb, n, vi_cur<M>(C, N.qb() + k), rho, omr, inv);
  const double qd = vi_eta<M>(pd, n, vi_cur<M>(C, N.qd() + k), rho, omr, inv);
  const int ej = lane & 15, ei0 = lane >> 4;        // element (ei0 + 4 r, ej) of the block, r = 0 .. 3
  if (lane < D) {
    const double p = in.pa[lane];
    const double q = vi_eta<M>(p, vi_stat<M>(in.sx, lane), vi_cur<M>(C, N.qa() + k * D + lane), rho, omr, inv);
    pav[lane] = p;
    qav[lane] = q;
    mv[lane] = q / qb;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D)
      s.Qc[i * kViLd + ej] = vi_eta<M>(in.pc[i * D + ej], vi_stat<M>(in.sxx, i * in.stride + ej),
                                       vi_cur<M>(C, N.qc() + (k * D + i) * D + ej), rho, omr, inv);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) s.U[i * kViLd + ej] = s.Qc[i * kViLd + ej] - qb * mv[i] * mv[ej];
  }
  wg_sync();
  double sl;
  if (!vi_chol_inv(s.U, s.X, D, lane, sl)) return false;

  // psi = C^-1 = X X', W = nu psi
  const double nu = qd + D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    o.psi[r] = 0.0;
    if (i < D && ej < D) {
      const double v = vi_xxt(s.X, D, i, ej);
      o.psi[r] = v;
      s.W[i * kViLd + ej] = nu * v;
    }
  }
  wg_sync();

  // per row: b = W m, <qc, W>, <pc, W>; the digamma and lgamma terms
  if (lane < D) {
    const int i = lane;
    double sb = 0.0, rq = 0.0, rp = 0.0;
    for (int j = 0; j < D; ++j) {
      const double w = s.W[i * kViLd + j];
      sb += w * mv[j];
      rq += s.Qc[i * kViLd + j] * w;
      rp += in.pc[i * D + j] * w;
    }
    bv[i] = sb;
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
  const double log_base = -0.5 * D * kViLog2Pi;
  const double cc = log_base + E2 + E4;
  // the component's term of the bound (mimo_host_nw_vlb)
  const double logZq = -0.5 * D * log(qb) + (0.5 * nu * D * kViLog2 + mg + nu * hld);
  const double iq = qaE1 + qb * E2 - 0.5 * qcW + qd * E4;
  const double ip = paE1 + pb * E2 - 0.5 * pcW + pd * E4;
  o.term = (logZq - log_base - iq) - (*in.plz - log_base - ip);
  o.n = n; o.qb = qb; o.qd = qd; o.nu = nu; o.hld = hld; o.E2 = E2; o.E4 = E4; o.cc = cc;
  return true;
}

// the block's thirteen parts into the posterior block P, at the sub-layout N
__device__ __forceinline__ void vi_nw_store(double* P, const ViNwLayout& N, int k, int n, int lane, const ViNwLds& s, const ViNwOut& o) {
  const int ej = lane & 15, ei0 = lane >> 4;
  if (lane < n) {
    P[N.qa() + k * n + lane] = s.qa()[lane];
    P[N.mus() + k * n + lane] = s.m()[lane];
    P[N.bb() + k * n + lane] = s.b()[lane];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < n && ej < n) {
      const int e = (k * n + i) * n + ej;
      P[N.qc() + e] = s.Qc[i * kViLd + ej];
      P[N.psis() + e] = o.psi[r];
      P[N.W() + e] = s.W[i * kViLd + ej];
    }
  }
  if (lane == 0) {
    P[N.qb() + k] = o.qb;
    P[N.qd() + k] = o.qd;
    P[N.nus() + k] = o.nu;
    P[N.hld() + k] = o.hld;
    P[N.cc() + k] = o.cc;
    P[N.E2() + k] = o.E2;
    P[N.E4() + k] = o.E4;
  }
}

// ---- the operand image (ThetaGeneric, identity order) ---------------------------------------------------------------------------
// the image of problem `prob`
__device__ __forceinline__ double* vi_image(const ViLoop& l, int prob) { return l.theta + (size_t)prob * l.K16 * l.NS * 64; }

// this lane's entries of the canonical form's D vector `b` and D x D block `W` (LDS, stride kViLd) are all finite
__device__ __forceinline__ bool vi_bw_finite(int D, int lane, const double* b, const double* W) {
  const int ej = lane & 15, ei0 = lane >> 4;
  bool ok = !(lane < D && !vi_finite(b[lane]));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D && !vi_finite(W[i * kViLd + ej])) ok = false;
  }
  return ok;
}

// the b / W entries of component k from the same two
__device__ __forceinline__ void vi_image_bw(double* th, int NS, int D, int k, int lane, const double* b, const double* W) {
  const int ej = lane & 15, ei0 = lane >> 4;
  if (lane < D) th[vi_theta_at(NS, k, vi_feat(D, lane, D))] = b[lane];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) {
      const double w = W[i * kViLd + ej];
      if (i == ej) th[vi_theta_at(NS, k, vi_feat(D, i, i))] = -0.5 * w;
      else if (i < ej) th[vi_theta_at(NS, k, vi_feat(D, i, ej))] = -0.5 * (w + W[ej * kViLd + i]);
    }
  }
}

// c_total of the K components from `ct` (LDS; finite: each lane reads back what it wrote itself), clamped as theta_entries of
// mimo_theta.h clamps it, and of the padding components
__device__ __forceinline__ void vi_image_c(double* th, int NS, int D, int K, int K16, int lane, const double* ct) {
  const int fdd = vi_feat(D, D, D);
  for (int k = lane; k < K; k += 64) th[vi_theta_at(NS, k, fdd)] = ct[k] < kPadLogDensity ? kPadLogDensity : ct[k];
  for (int k = K + lane; k < 16 * K16; k += 64) th[vi_theta_at(NS, k, fdd)] = kPadLogDensity;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the loop half of both families' argument checks (the init mode reads no statistics; the blend reads one factor per problem)
inline bool vi_loop_ok(const ViLoop& l) {
  if (l.mode != kViConjugate && l.mode != kViBlend && l.mode != kViInit) return false;
  if (l.mode == kViBlend && !l.inv_scale) return false;
  return l.B >= 1 && l.K >= 1 && l.K <= kBatchedMaxK && l.D >= 1 && l.D <= 16 && l.K16 == (l.K + 15) / 16 && l.NS >= 1 &&
         (l.S || l.mode == kViInit) && (l.scalars || l.mode == kViInit) && l.post && l.prior_terms && l.last && l.words &&
         l.theta && l.trace;
}

// launch(M) with the runtime mode as a compile-time constant M::value: the template argument of the update and gating kernels
template <typename F>
void vi_for_mode(int mode, F&& launch) {
  if (mode == kViBlend) launch(std::integral_constant<int, kViBlend>{});
  else if (mode == kViInit) launch(std::integral_constant<int, kViInit>{});
  else launch(std::integral_constant<int, kViConjugate>{});
}

}  // namespace

}  // namespace mimo
