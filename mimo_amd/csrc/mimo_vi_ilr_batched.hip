// Device-resident batched VI for mixtures of linear-Gaussian experts (gfx950): what stands between two batched softmax passes of B
// BayesianMixtureOfLinearGaussians — the conjugate update of the K basis blocks (Normal-Wishart over x), of the K affine experts
// (matrix-normal-Wishart of y | x~ = [x, 1]) and of the gating (Dirichlet or truncated stick-breaking) from the resident joint
// statistics over z = [x, y], the joint canonical form (c, b, W) as the operand image the next pass reads, the prior terms of the
// bound — as two small kernels beside the pass, its reduction and vi_finish_kernel (mimo_vi_batched.hip):
//
//   vi_ilr_update_kernel   one wave per (problem, component): the block slicing of split_joint_stats, the arithmetic of
//                          mimo_host_nw_vi on the dx x dx block and of mimo_host_mnw_vi (affine branch) on the expert block, the
//                          sum of embed_joint, both blocks' terms of the bound; every small block in LDS
//   vi_ilr_gating_kernel   one wave per problem: the Dirichlet or stick-breaking update, E[log pi], c_total into the image, the
//                          gating's term of the bound and the sums of the blocks' terms
//
// Both kernels are templates over the mode (ViMode, mimo_vi_batched.h): the conjugate update, the SVI blend of the current slot's
// natural parameters with it, or the derived parts of an uploaded posterior.
//
// All float64, plain launches, no atomics but the status word's.  Every sum runs in a fixed order that depends on (K, dx, dy)
// alone and every workgroup works on one problem, so a problem's numbers do not depend on what else is in the batch, bit for bit.
// Stopped and failed problems: as in mimo_vi_batched.hip (skipped; the posterior blocks are double-buffered).
//
// Reference semantics: mimo/mixtures/ilr.py:178-189,211-226; distributions/bayesian.py:151-159,173-176 (stick-breaking), 225-230,
// 258-265 (basis), 839-844,854-858,933-947 (experts); composite.py:50-72,95-128 (Normal-Wishart), 577-599,622-664
// (matrix-normal-Wishart); wishart.py:129-143; dirichlet.py:31-33,78-97 (Dirichlet), 108-112,195-214 (stick-breaking).
#include "mimo_vi_ilr_batched.h"
#include "mimo_batched.h"
#include "mimo_device.h"

#include <math.h>

namespace mimo {

namespace {

constexpr double kIlrLog2Pi = 1.8378770664093454835606594728112;
constexpr double kIlrLog2 = 0.69314718055994530941723212145818;
constexpr double kIlrLogPi = 1.1447298858494001741434273513531;
constexpr long long kIlrNanBits = 0x7ff8000000000000LL;    // (integer selects: the kernels are built with -fno-honor-nans)
constexpr int kLd = 17;                                    // LDS row stride of the small blocks (every side <= 16)
constexpr int kBlk = 16 * kLd;

// (the helpers of mimo_vi_batched.hip, restated: that file keeps its own)
__device__ __forceinline__ bool ilr_pos_finite(double v) {
  const long long b = __double_as_longlong(v);
  return b > 0 && b < 0x7ff0000000000000LL;
}

__device__ __forceinline__ bool ilr_finite(double v) {
  return (__double_as_longlong(v) & 0x7fffffffffffffffLL) < 0x7ff0000000000000LL;
}

// psi(x) for x > 0 (recurrence up to x >= 10, then the asymptotic series); anything else returns NaN at once
__device__ double ilr_digamma(double x) {
  if (!ilr_pos_finite(x)) return __longlong_as_double(kIlrNanBits);
  double r = 0.0;
  while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
  const double f = 1.0 / (x * x);
  const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 + f * (-1.0 / 132.0
                   + f * (691.0 / 32760.0 + f * (-1.0 / 12.0)))))));
  return r + log(x) - 0.5 / x + t;
}

// feature of the pair (a, b), a <= b <= D, in the full map; offset of entry (k, feature f) in one problem's image (ThetaGeneric)
__device__ __forceinline__ int ilr_feat(int D, int a, int b) { return a * (D + 1) - a * (a - 1) / 2 + (b - a); }
__device__ __forceinline__ size_t ilr_theta_at(int NS, int k, int f) {
  return ((size_t)(k >> 4) * NS + (f >> 2)) * 64 + (f & 3) * 16 + (k & 15);
}

// The n x n block in U (its upper triangle is read) -> its upper Cholesky factor U'U in place (right-looking), X = U^-1, `sl` the
// sum of the pivots' logarithms.  One wave; false when a pivot is not positive and finite (uniform: every lane reads the same
// pivots).  The inverse is then X X'.
__device__ bool ilr_chol_inv(double* U, double* X, int n, int lane, double& sl) {
  const int ej = lane & 15, ei0 = lane >> 4;
  bool bad = false;
  sl = 0.0;
  for (int j = 0; j < n; ++j) {
    double d = U[j * kLd + j];
    if (!ilr_pos_finite(d)) { bad = true; d = 1.0; }
    const double piv = sqrt(d);
    sl += log(piv);
    const double inv = 1.0 / piv;
    wg_sync();
    if (lane >= j && lane < n) U[j * kLd + lane] *= inv;
    wg_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ei0 + 4 * r;
      if (i > j && i < n && ej >= i && ej < n) U[i * kLd + ej] -= U[j * kLd + i] * U[j * kLd + ej];
    }
    wg_sync();
  }
  if (bad) return false;
  // row back-substitution: lane c owns column c (it reads only entries of X it wrote itself)
  if (lane < n) {
    const int c = lane;
    for (int i = c; i >= 0; --i) {
      double x = i == c ? 1.0 : 0.0;
      for (int kk = i + 1; kk <= c; ++kk) x -= U[i * kLd + kk] * X[kk * kLd + c];
      X[i * kLd + c] = x * (1.0 / U[i * kLd + i]);
    }
  }
  wg_sync();
  return true;
}

// entry (i, j) of X X' (entry (i, j) and its mirror run the same chain: the product is symmetric bit for bit)
__device__ __forceinline__ double ilr_xxt(const double* X, int n, int i, int j) {
  double v = 0.0;
  for (int c = i > j ? i : j; c < n; ++c) v += X[i * kLd + c] * X[j * kLd + c];
  return v;
}

template <int M>
__global__ __launch_bounds__(64) void vi_ilr_update_kernel(const ViIlrArgs a) {
  __shared__ double Bq[kBlk];       // basis: c of the posterior's natural parameters
  __shared__ double Bp[kBlk];       // basis: psi
  __shared__ double Bw[kBlk];       // basis: W1 = nu psi
  __shared__ double U[kBlk];        // the block being factorised -> its upper Cholesky factor
  __shared__ double X[kBlk];        // U^-1
  __shared__ double Kq[kBlk];       // experts: Kq = pb + S_x~x~ (dc x dc)
  __shared__ double Ki[kBlk];       // Kq^-1
  __shared__ double Am[kBlk];       // a = pa + S_yx~ (dy x dc)
  __shared__ double Mm[kBlk];       // M = a Kq^-1
  __shared__ double Cq[kBlk];       // c = pc + S_yy (dy x dy)
  __shared__ double Ps[kBlk];       // psi = (c - a M')^-1
  __shared__ double E1m[kBlk];      // nu psi M (dy x dc)
  __shared__ double E2m[kBlk];      // -1/2 (dy Kq^-1 + M'E1) (dc x dc)
  __shared__ double W2[kBlk];       // the experts' W over z (D x D)
  __shared__ double Wj[kBlk];       // the joint W
  __shared__ double vec[16][16];
  double* const mv = vec[0];        // basis: m, qa, pa, b1, digamma terms, lgamma terms, row sums <qc, W1>, <pc, W1>
  double* const qav = vec[1];
  double* const pav = vec[2];
  double* const b1v = vec[3];
  double* const dgv = vec[4];
  double* const lgv = vec[5];
  double* const rqv = vec[6];
  double* const rpv = vec[7];
  double* const b2v = vec[8];       // experts: b2 over z; the joint b; row sums of the six inner products
  double* const bjv = vec[9];
  double* const raq = vec[10];      // <a, E1>, <pa, E1> per row of y
  double* const rap = vec[11];
  double* const rkq = vec[12];      // <Kq, E2>, <pb, E2> per row of x~
  double* const rkp = vec[13];
  double* const rcq = vec[14];      // <c, nu psi>, <pc, nu psi> per row of y
  double* const rcp = vec[15];

  const int lane = threadIdx.x;
  const int B = a.loop.B, K = a.loop.K, dx = a.dx, dy = a.dy, dc = dx + 1, D = dx + dy, DD = D * D;
  const int prob = blockIdx.x / K, k = blockIdx.x - prob * K;
  int32_t* const words = a.loop.words;
  if (!words[kViActive * B + prob] || words[kViStatus * B + prob]) return;
  const int cur = words[kViSlot * B + prob], slot = 1 - cur;
  const ViIlrLayout L{K, dx, dy};
  double* const P = a.loop.post + ((size_t)slot * B + prob) * L.count();
  const double* const C = a.loop.post + ((size_t)cur * B + prob) * L.count();      // the current block (blend and init modes)
  const double rho = a.loop.rho, omr = a.loop.one_minus_rho;
  double inv = 0.0;
  if constexpr (M == kViBlend) inv = a.loop.inv_scale[prob];
  const size_t bk = (size_t)prob * K + k;
  const double* const Sk = a.loop.S + bk * (size_t)(1 + D + DD);
  const double* const sx = Sk + 1;            // sum r z
  const double* const sxx = Sk + 1 + D;       // sum r z z'
  const int ej = lane & 15, ei0 = lane >> 4;  // element (ei0 + 4 r, ej) of a block, r = 0 .. 3

  // ---- basis: the Normal-Wishart update on (sum r x, n, sum r x x', n) ---------------------------------------------------------
  // (every eta below: prior + statistics in the conjugate mode, the mode's form of it otherwise — vi_eta, mimo_vi_batched.h)
  const double n = vi_stat<M>(Sk, 0);
  const double* const pck = a.pc + bk * dx * dx;
  const double pb = a.pb[bk], pd = a.pd[bk];
  const double qb = vi_eta<M>(pb, n, vi_cur<M>(C, L.b_qb() + k), rho, omr, inv);
  const double qd = vi_eta<M>(pd, n, vi_cur<M>(C, L.b_qd() + k), rho, omr, inv);
  if (lane < dx) {
    const double p = a.pa[bk * dx + lane];
    const double q = vi_eta<M>(p, vi_stat<M>(sx, lane), vi_cur<M>(C, L.b_qa() + k * dx + lane), rho, omr, inv);
    pav[lane] = p;
    qav[lane] = q;
    mv[lane] = q / qb;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dx && ej < dx)
      Bq[i * kLd + ej] = vi_eta<M>(pck[i * dx + ej], vi_stat<M>(sxx, i * D + ej), vi_cur<M>(C, L.b_qc() + (k * dx + i) * dx + ej), rho,
                                   omr, inv);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dx && ej < dx) U[i * kLd + ej] = Bq[i * kLd + ej] - qb * mv[i] * mv[ej];
  }
  wg_sync();
  double sl1;
  if (!ilr_chol_inv(U, X, dx, lane, sl1)) {
    if (lane == 0) atomicOr(&words[kViStatus * B + prob], kViNotPosDef);
    return;
  }
  const double nu1 = qd + dx;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dx && ej < dx) {
      const double v = ilr_xxt(X, dx, i, ej);
      Bp[i * kLd + ej] = v;
      Bw[i * kLd + ej] = nu1 * v;
    }
  }
  wg_sync();
  if (lane < dx) {
    const int i = lane;
    double s = 0.0, rq = 0.0, rp = 0.0;
    for (int j = 0; j < dx; ++j) {
      const double w = Bw[i * kLd + j];
      s += w * mv[j];
      rq += Bq[i * kLd + j] * w;
      rp += pck[i * dx + j] * w;
    }
    b1v[i] = s;
    rqv[i] = rq;
    rpv[i] = rp;
    dgv[i] = ilr_digamma(0.5 * (nu1 - i));
    lgv[i] = lgamma(0.5 * nu1 - 0.5 * i);
  }
  wg_sync();
  double cc1, term1, hld1, E2b, E4b;
  {
    double mWm = 0.0, dg = 0.0, mg = 0.25 * dx * (dx - 1) * kIlrLogPi, qaE1 = 0.0, paE1 = 0.0, qcW = 0.0, pcW = 0.0;
    for (int i = 0; i < dx; ++i) {      // on every lane alike, ascending
      mWm += mv[i] * b1v[i];
      dg += dgv[i];
      mg += lgv[i];
      qaE1 += qav[i] * b1v[i];
      paE1 += pav[i] * b1v[i];
      qcW += rqv[i];
      pcW += rpv[i];
    }
    hld1 = -sl1;
    E2b = -0.5 * (dx / qb + mWm);
    E4b = 0.5 * (dg + dx * kIlrLog2 + 2.0 * hld1);
    const double log_base = -0.5 * dx * kIlrLog2Pi;
    cc1 = log_base + E2b + E4b;
    const double logZq = -0.5 * dx * log(qb) + (0.5 * nu1 * dx * kIlrLog2 + mg + nu1 * hld1);
    const double iq = qaE1 + qb * E2b - 0.5 * qcW + qd * E4b;
    const double ip = paE1 + pb * E2b - 0.5 * pcW + pd * E4b;
    term1 = (logZq - log_base - iq) - (a.plz[bk] - log_base - ip);
  }
  wg_sync();      // (dgv, lgv are reused below)

  // ---- experts: the matrix-normal-Wishart update on (sum r y x~', sum r x~ x~', sum r y y', n), x~ = [x, 1] -------------------
  const double* const mak = a.ma + bk * dy * dc;
  const double* const mbk = a.mb + bk * dc * dc;
  const double* const mck = a.mc + bk * dy * dy;
  const double md = a.md[bk];
  const double qdm = vi_eta<M>(md, n, vi_cur<M>(C, L.m_d() + k), rho, omr, inv);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc)        // the last column of y x~' is sum r y
      Am[i * kLd + ej] = vi_eta<M>(mak[i * dc + ej], ej < dx ? vi_stat<M>(sxx, (dx + i) * D + ej) : vi_stat<M>(sx, dx + i),
                                   vi_cur<M>(C, L.m_a() + (k * dy + i) * dc + ej), rho, omr, inv);
    if (i < dc && ej < dc) {      // the border of x~ x~' is sum r x and n
      const double s = i < dx ? (ej < dx ? vi_stat<M>(sxx, i * D + ej) : vi_stat<M>(sx, i)) : (ej < dx ? vi_stat<M>(sx, ej) : n);
      const double v = vi_eta<M>(mbk[i * dc + ej], s, vi_cur<M>(C, L.m_Kq() + (k * dc + i) * dc + ej), rho, omr, inv);
      Kq[i * kLd + ej] = v;
      U[i * kLd + ej] = v;
    }
    if (i < dy && ej < dy)
      Cq[i * kLd + ej] = vi_eta<M>(mck[i * dy + ej], vi_stat<M>(sxx, (dx + i) * D + dx + ej),
                                   vi_cur<M>(C, L.m_c() + (k * dy + i) * dy + ej), rho, omr, inv);
  }
  wg_sync();
  double slK;
  if (!ilr_chol_inv(U, X, dc, lane, slK)) {
    if (lane == 0) atomicOr(&words[kViStatus * B + prob], kViNotPosDef);
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dc && ej < dc) Ki[i * kLd + ej] = ilr_xxt(X, dc, i, ej);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // M = a Kq^-1
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc) {
      double s = 0.0;
      for (int q = 0; q < dc; ++q) s += Am[i * kLd + q] * Ki[q * kLd + ej];
      Mm[i * kLd + ej] = s;
    }
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // C = c - a M' (entry (i, j) and its mirror run the chain of the upper one)
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dy) {
      const int lo = i < ej ? i : ej, hi = i < ej ? ej : i;
      double s = Cq[lo * kLd + hi];
      for (int q = 0; q < dc; ++q) s -= Am[lo * kLd + q] * Mm[hi * kLd + q];
      U[i * kLd + ej] = s;
    }
  }
  wg_sync();
  double slC;
  if (!ilr_chol_inv(U, X, dy, lane, slC)) {
    if (lane == 0) atomicOr(&words[kViStatus * B + prob], kViNotPosDef);
    return;
  }
  const double nu2 = qdm + dy + 1.0 - dc;
  const double hld2 = -slC;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dy) Ps[i * kLd + ej] = ilr_xxt(X, dy, i, ej);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // E1 = nu psi M
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc) {
      double s = 0.0;
      for (int q = 0; q < dy; ++q) s += Ps[i * kLd + q] * Mm[q * kLd + ej];
      E1m[i * kLd + ej] = nu2 * s;
    }
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // E2 = -1/2 (dy Kq^-1 + M'E1), the chain of the upper entry for both mirrors
    const int i = ei0 + 4 * r;
    if (i < dc && ej < dc) {
      const int lo = i < ej ? i : ej, hi = i < ej ? ej : i;
      double s = 0.0;
      for (int q = 0; q < dy; ++q) s += Mm[q * kLd + lo] * E1m[q * kLd + hi];
      E2m[i * kLd + ej] = -0.5 * (dy * Ki[lo * kLd + hi] + s);
    }
  }
  wg_sync();
  // the canonical form over z (bayesian.py:933-947) and the joint one (embed_joint)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) {
      double w;
      if (i < dx && ej < dx) w = -2.0 * E2m[i * kLd + ej];
      else if (i >= dx && ej >= dx) w = nu2 * Ps[(i - dx) * kLd + ej - dx];
      else if (i >= dx) w = -E1m[(i - dx) * kLd + ej];
      else w = -E1m[(ej - dx) * kLd + i];
      W2[i * kLd + ej] = w;
      Wj[i * kLd + ej] = (i < dx && ej < dx) ? w + Bw[i * kLd + ej] : w;
    }
  }
  if (lane < D) {
    const double v = lane < dx ? 2.0 * E2m[lane * kLd + dx] : E1m[(lane - dx) * kLd + dx];
    b2v[lane] = v;
    bjv[lane] = lane < dx ? v + b1v[lane] : v;
  }
  // per row: the six inner products of the bound's term; the digamma and lgamma terms
  if (lane < 16) {
    const int i = lane;
    double aq = 0.0, ap = 0.0, kq = 0.0, kp = 0.0, cq = 0.0, cp = 0.0;
    if (i < dy) {
      for (int j = 0; j < dc; ++j) {
        const double e = E1m[i * kLd + j];
        aq += Am[i * kLd + j] * e;
        ap += mak[i * dc + j] * e;
      }
      for (int j = 0; j < dy; ++j) {
        const double w = nu2 * Ps[i * kLd + j];
        cq += Cq[i * kLd + j] * w;
        cp += mck[i * dy + j] * w;
      }
      dgv[i] = ilr_digamma(0.5 * (nu2 - i));
      lgv[i] = lgamma(0.5 * nu2 - 0.5 * i);
    }
    if (i < dc)
      for (int j = 0; j < dc; ++j) {
        const double e = E2m[i * kLd + j];
        kq += Kq[i * kLd + j] * e;
        kp += mbk[i * dc + j] * e;
      }
    raq[i] = aq; rap[i] = ap; rkq[i] = kq; rkp[i] = kp; rcq[i] = cq; rcp[i] = cp;
  }
  wg_sync();
  double dg = 0.0, mg = 0.25 * dy * (dy - 1) * kIlrLogPi, aE1 = 0.0, paE1 = 0.0, cW = 0.0, pcW = 0.0, kE2 = 0.0, pkE2 = 0.0;
  for (int i = 0; i < dy; ++i) {      // on every lane alike, ascending
    dg += dgv[i];
    mg += lgv[i];
    aE1 += raq[i];
    paE1 += rap[i];
    cW += rcq[i];
    pcW += rcp[i];
  }
  for (int i = 0; i < dc; ++i) {
    kE2 += rkq[i];
    pkE2 += rkp[i];
  }
  const double E4m = 0.5 * (dg + dy * kIlrLog2 + 2.0 * hld2);
  const double cc2 = -0.5 * dy * kIlrLog2Pi + E4m + E2m[dx * kLd + dx];
  const double lbm = -0.5 * dy * dc * kIlrLog2Pi;
  const double logZqm = -0.5 * dy * (2.0 * slK) + (0.5 * nu2 * dy * kIlrLog2 + mg + nu2 * hld2);
  const double iqm = aE1 + kE2 - 0.5 * cW + qdm * E4m;
  const double ipm = paE1 + pkE2 - 0.5 * pcW + md * E4m;
  const double term2 = (logZqm - lbm - iqm) - (a.mlz[bk] - lbm - ipm);
  const double ccj = cc1 + cc2;

  // a canonical form or a term that is not finite (a digamma argument <= 0, an overflow): the problem's status, nothing written
  bool lane_bad = lane < D && !ilr_finite(bjv[lane]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D && !ilr_finite(Wj[i * kLd + ej])) lane_bad = true;
  }
  if (__any(lane_bad) || !ilr_finite(ccj) || !ilr_finite(term1) || !ilr_finite(term2)) {
    if (lane == 0) atomicOr(&words[kViStatus * B + prob], kViNotFinite);
    return;
  }

  // ---- outputs: the posterior block, the terms, the b / W entries of the operand image ----------------------------------------
  double* const th = a.loop.theta + (size_t)prob * a.loop.K16 * a.loop.NS * 64;
  const int NS = a.loop.NS;
  if (lane < dx) {
    P[L.b_qa() + k * dx + lane] = qav[lane];
    P[L.b_mus() + k * dx + lane] = mv[lane];
    P[L.b_bb() + k * dx + lane] = b1v[lane];
  }
  if (lane < D) {
    P[L.m_bb() + k * D + lane] = b2v[lane];
    P[L.bb() + k * D + lane] = bjv[lane];
    th[ilr_theta_at(NS, k, ilr_feat(D, lane, D))] = bjv[lane];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dx && ej < dx) {
      const int e = (k * dx + i) * dx + ej;
      P[L.b_qc() + e] = Bq[i * kLd + ej];
      P[L.b_psis() + e] = Bp[i * kLd + ej];
      P[L.b_W() + e] = Bw[i * kLd + ej];
    }
    if (i < dy && ej < dc) {
      const int e = (k * dy + i) * dc + ej;
      P[L.m_a() + e] = Am[i * kLd + ej];
      P[L.m_Ms() + e] = Mm[i * kLd + ej];
      P[L.m_E1() + e] = E1m[i * kLd + ej];
    }
    if (i < dc && ej < dc) {
      const int e = (k * dc + i) * dc + ej;
      P[L.m_Kq() + e] = Kq[i * kLd + ej];
      P[L.m_Kinv() + e] = Ki[i * kLd + ej];
      P[L.m_E2() + e] = E2m[i * kLd + ej];
    }
    if (i < dy && ej < dy) {
      const int e = (k * dy + i) * dy + ej;
      P[L.m_c() + e] = Cq[i * kLd + ej];
      P[L.m_psis() + e] = Ps[i * kLd + ej];
    }
    if (i < D && ej < D) {
      const int e = k * DD + i * D + ej;
      const double w = Wj[i * kLd + ej];
      P[L.m_W() + e] = W2[i * kLd + ej];
      P[L.W() + e] = w;
      if (i == ej) th[ilr_theta_at(NS, k, ilr_feat(D, i, i))] = -0.5 * w;
      else if (i < ej) th[ilr_theta_at(NS, k, ilr_feat(D, i, ej))] = -0.5 * (w + Wj[ej * kLd + i]);
    }
  }
  if (lane == 0) {
    P[L.b_qb() + k] = qb;
    P[L.b_qd() + k] = qd;
    P[L.b_nus() + k] = nu1;
    P[L.b_hld() + k] = hld1;
    P[L.b_cc() + k] = cc1;
    P[L.b_E2() + k] = E2b;
    P[L.b_E4() + k] = E4b;
    P[L.m_d() + k] = qdm;
    P[L.m_nus() + k] = nu2;
    P[L.m_hld() + k] = hld2;
    P[L.m_E4() + k] = E4m;
    P[L.m_cc() + k] = cc2;
    a.term_b[bk] = term1;
    a.term_m[bk] = term2;
  }
}

template <int M>
__global__ __launch_bounds__(64) void vi_ilr_gating_kernel(const ViIlrArgs a) {
  // g0, g1 of the posterior, of the prior; E[log stick | pi], E[log rest]; E[log pi]; c_total; six summands of the gating's term;
  // the basis terms, the experts' terms
  __shared__ double t[16][kBatchedMaxK];
  __shared__ double red[8];
  const int lane = threadIdx.x;
  const int B = a.loop.B, K = a.loop.K, D = a.loop.D;
  const int prob = blockIdx.x;
  int32_t* const words = a.loop.words;
  if (!words[kViActive * B + prob] || words[kViStatus * B + prob]) return;
  const int cur = words[kViSlot * B + prob], slot = 1 - cur;
  const ViIlrLayout L{K, a.dx, a.dy};
  double* const P = a.loop.post + ((size_t)slot * B + prob) * L.count();
  const double* const C = a.loop.post + ((size_t)cur * B + prob) * L.count();      // the current block (blend and init modes)
  const double rho = a.loop.rho, omr = a.loop.one_minus_rho;
  double inv = 0.0;
  if constexpr (M == kViBlend) inv = a.loop.inv_scale[prob];
  const size_t sstride = (size_t)(1 + D + D * D);
  const bool stick = a.gating == kViGatingStick;

  for (int k = lane; k < K; k += 64) t[8][k] = vi_stat<M>(a.loop.S, ((size_t)prob * K + k) * sstride);      // the counts
  wg_sync();
  double lgs = 0.0, lgs0 = 0.0;      // Dirichlet: lgamma of the sums
  if (stick) {
    // gamma = gamma0 + n; delta = delta0 + counts of all later sticks, summed from the last stick down (stick_acc_counts)
    if (lane == 0) {
      double s = 0.0;
      t[9][K - 1] = 0.0;
      for (int k = K - 1; k >= 1; --k) { s += t[8][k]; t[9][k - 1] = s; }
    }
    wg_sync();
    for (int k = lane; k < K; k += 64) {
      const size_t bk = (size_t)prob * K + k;
      const double g0 = a.g0[bk], d0 = a.g1[bk];
      // (blend: CategoricalWithStickBreaking.meanfield_sgd on the gammas and the deltas themselves)
      const double g = vi_eta<M>(g0, t[8][k], vi_cur<M>(C, L.g0() + k), rho, omr, inv);
      const double d = vi_eta<M>(d0, t[9][k], vi_cur<M>(C, L.g1() + k), rho, omr, inv);
      const double dsum = ilr_digamma(g + d);
      t[0][k] = g; t[1][k] = d; t[2][k] = g0; t[3][k] = d0;
      t[4][k] = ilr_digamma(g) - dsum;      // E[log stick]
      t[5][k] = ilr_digamma(d) - dsum;      // E[log rest]
    }
    wg_sync();
    if (lane == 0) {                        // E[log pi_k] = E[log stick_k] + sum_{j<k} E[log rest_j], ascending
      double s = 0.0;
      for (int k = 0; k < K; ++k) {
        t[6][k] = t[4][k] + s;
        s += t[5][k];
      }
    }
    wg_sync();
  } else {
    // alpha = ((alpha0 - 1) + n) + 1
    for (int k = lane; k < K; k += 64) {
      const double a0 = a.g0[(size_t)prob * K + k];
      // (blend: on the natural parameter alpha - 1, CategoricalWithDirichlet.meanfield_sgd; init: the uploaded alpha itself)
      if constexpr (M == kViInit) t[0][k] = C[L.g0() + k];
      else t[0][k] = vi_eta<M>(a0 - 1.0, t[8][k], vi_cur<M>(C, L.g0() + k) - 1.0, rho, omr, inv) + 1.0;
      t[1][k] = 0.0;
      t[2][k] = a0;
      t[3][k] = 0.0;
    }
    wg_sync();
    double s = 0.0, s0 = 0.0;
    for (int k = 0; k < K; ++k) { s += t[0][k]; s0 += t[2][k]; }      // on every lane alike, ascending
    const double ds = ilr_digamma(s);
    lgs = lgamma(s);
    lgs0 = lgamma(s0);
    for (int k = lane; k < K; k += 64) {
      t[4][k] = ilr_digamma(t[0][k]) - ds;
      t[5][k] = 0.0;
      t[6][k] = t[4][k];
    }
    wg_sync();
  }

  double* const th = a.loop.theta + (size_t)prob * a.loop.K16 * a.loop.NS * 64;
  const int fdd = ilr_feat(D, D, D);
  bool lane_bad = false;
  for (int k = lane; k < K; k += 64) {
    const double g = t[0][k], d = t[1][k], g0 = t[2][k], d0 = t[3][k], es = t[4][k], er = t[5][k];
    const double elp = t[6][k];
    const double ct = (P[L.b_cc() + k] + P[L.m_cc() + k]) + elp;
    lane_bad = lane_bad || !ilr_finite(elp) || !ilr_finite(ct) || !ilr_finite(er);
    t[7][k] = ct;
    if (stick) {
      t[8][k] = (lgamma(g) + lgamma(d)) - lgamma(g + d);           // betaln of the posterior, of the prior
      t[9][k] = (lgamma(g0) + lgamma(d0)) - lgamma(g0 + d0);
      t[10][k] = (g - 1.0) * es;
      t[11][k] = (d - 1.0) * er;
      t[12][k] = (g0 - 1.0) * es;
      t[13][k] = (d0 - 1.0) * er;
    } else {
      t[8][k] = lgamma(g);
      t[9][k] = lgamma(g0);
      t[10][k] = (g - 1.0) * es;
      t[11][k] = 0.0;
      t[12][k] = (g0 - 1.0) * es;
      t[13][k] = 0.0;
    }
    t[14][k] = a.term_b[(size_t)prob * K + k];
    t[15][k] = a.term_m[(size_t)prob * K + k];
  }
  if (__any(lane_bad)) {                     // nothing of the gating is written
    if (lane == 0) atomicOr(&words[kViStatus * B + prob], kViNotFinite);
    return;
  }
  for (int k = lane; k < K; k += 64) {       // (each lane reads back what it wrote itself)
    const double ct = t[7][k];
    P[L.g0() + k] = t[0][k];
    P[L.g1() + k] = t[1][k];
    P[L.elp() + k] = t[6][k];
    P[L.c_total() + k] = ct;
    th[ilr_theta_at(a.loop.NS, k, fdd)] = ct < kPadLogDensity ? kPadLogDensity : ct;
  }
  for (int k = K + lane; k < 16 * a.loop.K16; k += 64) th[ilr_theta_at(a.loop.NS, k, fdd)] = kPadLogDensity;
  wg_sync();
  if (lane < 8) {                            // ascending k, one sum per lane
    double v = 0.0;
    for (int k = 0; k < K; ++k) v += t[8 + lane][k];
    red[lane] = v;
  }
  wg_sync();
  if (lane == 0) {
    const double gate = ((red[0] - lgs) - (red[2] + red[3])) - ((red[1] - lgs0) - (red[4] + red[5]));
    const double prior_terms = (gate + red[6]) + red[7];
    if (!ilr_finite(prior_terms)) {          // the slot does not become current
      atomicOr(&words[kViStatus * B + prob], kViNotFinite);
      return;
    }
    P[L.vlb()] = gate;
    P[L.vlb() + 1] = red[6];
    P[L.vlb() + 2] = red[7];
    a.loop.prior_terms[prob] = prior_terms;
    words[kViSlot * B + prob] = slot;        // the block just written is the problem's current one
  }
}

bool ilr_args_ok(const ViIlrArgs& a) {
  const ViArgs& l = a.loop;
  if (l.mode != kViConjugate && l.mode != kViBlend && l.mode != kViInit) return false;
  if (l.mode == kViBlend && !l.inv_scale) return false;
  return l.B >= 1 && l.K >= 1 && l.K <= kBatchedMaxK && a.dx >= 1 && a.dy >= 1 && a.dx + a.dy <= 16 && l.D == a.dx + a.dy &&
         l.K16 == (l.K + 15) / 16 && l.NS >= 1 && (a.gating == kViGatingDirichlet || a.gating == kViGatingStick) &&
         (l.S || l.mode == kViInit) && (l.scalars || l.mode == kViInit) && l.post && l.prior_terms && l.last && l.words && l.theta && l.trace && a.g0 && a.g1 && a.pa && a.pb && a.pc &&
         a.pd && a.plz && a.ma && a.mb && a.mc && a.md && a.mlz && a.term_b && a.term_m;
}

}  // namespace

hipError_t launch_vi_ilr_update(const ViIlrArgs& a, hipStream_t stream) {
  if (!ilr_args_ok(a) || (int64_t)a.loop.B * a.loop.K > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.loop.B * a.loop.K));
  if (a.loop.mode == kViBlend) hipLaunchKernelGGL(vi_ilr_update_kernel<kViBlend>, grid, dim3(64), 0, stream, a);
  else if (a.loop.mode == kViInit) hipLaunchKernelGGL(vi_ilr_update_kernel<kViInit>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(vi_ilr_update_kernel<kViConjugate>, grid, dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_vi_ilr_gating(const ViIlrArgs& a, hipStream_t stream) {
  if (!ilr_args_ok(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.loop.B);
  if (a.loop.mode == kViBlend) hipLaunchKernelGGL(vi_ilr_gating_kernel<kViBlend>, grid, dim3(64), 0, stream, a);
  else if (a.loop.mode == kViInit) hipLaunchKernelGGL(vi_ilr_gating_kernel<kViInit>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(vi_ilr_gating_kernel<kViConjugate>, grid, dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mimo
