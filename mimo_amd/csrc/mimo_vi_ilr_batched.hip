// Device-resident batched VI for mixtures of linear-Gaussian experts (gfx950): what stands between two batched softmax passes of B
// BayesianMixtureOfLinearGaussians — the conjugate update of the K basis blocks (Normal-Wishart over x), of the K affine experts
// (matrix-normal-Wishart of y | x~ = [x, 1]) and of the gating (Dirichlet or truncated stick-breaking) from the resident joint
// statistics over z = [x, y], the joint canonical form (c, b, W) as the operand image the next pass reads, the prior terms of the
// bound — as two small kernels beside the pass, its reduction and vi_finish_kernel (mimo_vi_batched.hip):
//
//   vi_ilr_update_kernel   one wave per (problem, component): the block slicing of split_joint_stats, the arithmetic of
//                          mimo_host_nw_vi on the dx x dx block (vi_nw_block of mimo_vi_device.h, the block of the GMM loop) and
//                          of mimo_host_mnw_vi (affine branch) on the expert block, the
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
#include "mimo_vi_device.h"

namespace mimo {

namespace {

template <int M>
__global__ __launch_bounds__(64) void vi_ilr_update_kernel(const ViIlrArgs a) {
  __shared__ double Bq[kViBlk];       // basis: c of the posterior's natural parameters
  __shared__ double Bw[kViBlk];       // basis: W1 = nu psi
  __shared__ double U[kViBlk];        // the block being factorised -> its upper Cholesky factor
  __shared__ double X[kViBlk];        // U^-1
  __shared__ double Kq[kViBlk];       // experts: Kq = pb + S_x~x~ (dc x dc)
  __shared__ double Ki[kViBlk];       // Kq^-1
  __shared__ double Am[kViBlk];       // a = pa + S_yx~ (dy x dc)
  __shared__ double Mm[kViBlk];       // M = a Kq^-1
  __shared__ double Cq[kViBlk];       // c = pc + S_yy (dy x dy)
  __shared__ double Ps[kViBlk];       // psi = (c - a M')^-1
  __shared__ double E1m[kViBlk];      // nu psi M (dy x dc)
  __shared__ double E2m[kViBlk];      // -1/2 (dy Kq^-1 + M'E1) (dc x dc)
  __shared__ double W2[kViBlk];       // the experts' W over z (D x D)
  __shared__ double Wj[kViBlk];       // the joint W
  __shared__ double vec[16][16];    // 0 .. 7: the basis block's (ViNwLds); 4, 5 again for the experts' digamma and lgamma terms
  double* const dgv = vec[4];
  double* const lgv = vec[5];
  double* const b2v = vec[8];       // experts: b2 over z; the joint b; row sums of the six inner products
  double* const bjv = vec[9];
  double* const raq = vec[10];      // <a, E1>, <pa, E1> per row of y
  double* const rap = vec[11];
  double* const rkq = vec[12];      // <Kq, E2>, <pb, E2> per row of x~
  double* const rkp = vec[13];
  double* const rcq = vec[14];      // <c, nu psi>, <pc, nu psi> per row of y
  double* const rcp = vec[15];

  const ViLoop& l = a.loop;
  const int lane = threadIdx.x;
  const int K = l.K, dx = a.dx, dy = a.dy, dc = dx + 1, D = dx + dy, DD = D * D;
  const int prob = blockIdx.x / K, k = blockIdx.x - prob * K;
  const ViIlrLayout L{K, dx, dy};
  ViProblem pr;
  if (!vi_problem<M>(l, prob, L.count(), pr)) return;
  double* const P = pr.P;
  const double* const C = pr.C;
  const double rho = l.rho, omr = l.one_minus_rho, inv = pr.inv;
  const size_t bk = (size_t)prob * K + k;
  const double* const Sk = l.S + bk * (size_t)(1 + D + DD);
  const double* const sx = Sk + 1;            // sum r z
  const double* const sxx = Sk + 1 + D;       // sum r z z'
  const int ej = lane & 15, ei0 = lane >> 4;  // element (ei0 + 4 r, ej) of a block, r = 0 .. 3

  // ---- basis: the Normal-Wishart update on (sum r x, n, sum r x x', n): the x block of the joint statistics ---------------------
  const ViNwLds nw{Bq, U, X, Bw, vec};
  const ViNwIn in{a.pa + bk * dx, a.pb + bk, a.pc + bk * dx * dx, a.pd + bk, a.plz + bk, Sk, sx, sxx, D,
                  C, L.basis(), k, dx, rho, omr, inv};
  ViNwOut o1;
  if (!vi_nw_block<M>(in, nw, lane, o1)) return vi_fail(l, prob, lane, kViNotPosDef);
  const double* const b1v = nw.b();
  wg_sync();      // (dgv, lgv are reused below)

  // ---- experts: the matrix-normal-Wishart update on (sum r y x~', sum r x~ x~', sum r y y', n), x~ = [x, 1] -------------------
  const double* const mak = a.ma + bk * dy * dc;
  const double* const mbk = a.mb + bk * dc * dc;
  const double* const mck = a.mc + bk * dy * dy;
  const double md = a.md[bk];
  const double n = o1.n;
  const double qdm = vi_eta<M>(md, n, vi_cur<M>(C, L.m_d() + k), rho, omr, inv);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc)        // the last column of y x~' is sum r y
      Am[i * kViLd + ej] = vi_eta<M>(mak[i * dc + ej], ej < dx ? vi_stat<M>(sxx, (dx + i) * D + ej) : vi_stat<M>(sx, dx + i),
                                   vi_cur<M>(C, L.m_a() + (k * dy + i) * dc + ej), rho, omr, inv);
    if (i < dc && ej < dc) {      // the border of x~ x~' is sum r x and n
      const double s = i < dx ? (ej < dx ? vi_stat<M>(sxx, i * D + ej) : vi_stat<M>(sx, i)) : (ej < dx ? vi_stat<M>(sx, ej) : n);
      const double v = vi_eta<M>(mbk[i * dc + ej], s, vi_cur<M>(C, L.m_Kq() + (k * dc + i) * dc + ej), rho, omr, inv);
      Kq[i * kViLd + ej] = v;
      U[i * kViLd + ej] = v;
    }
    if (i < dy && ej < dy)
      Cq[i * kViLd + ej] = vi_eta<M>(mck[i * dy + ej], vi_stat<M>(sxx, (dx + i) * D + dx + ej),
                                   vi_cur<M>(C, L.m_c() + (k * dy + i) * dy + ej), rho, omr, inv);
  }
  wg_sync();
  double slK;
  if (!vi_chol_inv(U, X, dc, lane, slK)) return vi_fail(l, prob, lane, kViNotPosDef);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dc && ej < dc) Ki[i * kViLd + ej] = vi_xxt(X, dc, i, ej);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // M = a Kq^-1
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc) {
      double s = 0.0;
      for (int q = 0; q < dc; ++q) s += Am[i * kViLd + q] * Ki[q * kViLd + ej];
      Mm[i * kViLd + ej] = s;
    }
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // C = c - a M' (entry (i, j) and its mirror run the chain of the upper one)
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dy) {
      const int lo = i < ej ? i : ej, hi = i < ej ? ej : i;
      double s = Cq[lo * kViLd + hi];
      for (int q = 0; q < dc; ++q) s -= Am[lo * kViLd + q] * Mm[hi * kViLd + q];
      U[i * kViLd + ej] = s;
    }
  }
  wg_sync();
  double slC;
  if (!vi_chol_inv(U, X, dy, lane, slC)) return vi_fail(l, prob, lane, kViNotPosDef);
  const double nu2 = qdm + dy + 1.0 - dc;
  const double hld2 = -slC;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dy) Ps[i * kViLd + ej] = vi_xxt(X, dy, i, ej);
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // E1 = nu psi M
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc) {
      double s = 0.0;
      for (int q = 0; q < dy; ++q) s += Ps[i * kViLd + q] * Mm[q * kViLd + ej];
      E1m[i * kViLd + ej] = nu2 * s;
    }
  }
  wg_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {      // E2 = -1/2 (dy Kq^-1 + M'E1), the chain of the upper entry for both mirrors
    const int i = ei0 + 4 * r;
    if (i < dc && ej < dc) {
      const int lo = i < ej ? i : ej, hi = i < ej ? ej : i;
      double s = 0.0;
      for (int q = 0; q < dy; ++q) s += Mm[q * kViLd + lo] * E1m[q * kViLd + hi];
      E2m[i * kViLd + ej] = -0.5 * (dy * Ki[lo * kViLd + hi] + s);
    }
  }
  wg_sync();
  // the canonical form over z (bayesian.py:933-947) and the joint one (embed_joint)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < D && ej < D) {
      double w;
      if (i < dx && ej < dx) w = -2.0 * E2m[i * kViLd + ej];
      else if (i >= dx && ej >= dx) w = nu2 * Ps[(i - dx) * kViLd + ej - dx];
      else if (i >= dx) w = -E1m[(i - dx) * kViLd + ej];
      else w = -E1m[(ej - dx) * kViLd + i];
      W2[i * kViLd + ej] = w;
      Wj[i * kViLd + ej] = (i < dx && ej < dx) ? w + Bw[i * kViLd + ej] : w;
    }
  }
  if (lane < D) {
    const double v = lane < dx ? 2.0 * E2m[lane * kViLd + dx] : E1m[(lane - dx) * kViLd + dx];
    b2v[lane] = v;
    bjv[lane] = lane < dx ? v + b1v[lane] : v;
  }
  // per row: the six inner products of the bound's term; the digamma and lgamma terms
  if (lane < 16) {
    const int i = lane;
    double aq = 0.0, ap = 0.0, kq = 0.0, kp = 0.0, cq = 0.0, cp = 0.0;
    if (i < dy) {
      for (int j = 0; j < dc; ++j) {
        const double e = E1m[i * kViLd + j];
        aq += Am[i * kViLd + j] * e;
        ap += mak[i * dc + j] * e;
      }
      for (int j = 0; j < dy; ++j) {
        const double w = nu2 * Ps[i * kViLd + j];
        cq += Cq[i * kViLd + j] * w;
        cp += mck[i * dy + j] * w;
      }
      dgv[i] = vi_digamma(0.5 * (nu2 - i));
      lgv[i] = lgamma(0.5 * nu2 - 0.5 * i);
    }
    if (i < dc)
      for (int j = 0; j < dc; ++j) {
        const double e = E2m[i * kViLd + j];
        kq += Kq[i * kViLd + j] * e;
        kp += mbk[i * dc + j] * e;
      }
    raq[i] = aq; rap[i] = ap; rkq[i] = kq; rkp[i] = kp; rcq[i] = cq; rcp[i] = cp;
  }
  wg_sync();
  double dg = 0.0, mg = 0.25 * dy * (dy - 1) * kViLogPi, aE1 = 0.0, paE1 = 0.0, cW = 0.0, pcW = 0.0, kE2 = 0.0, pkE2 = 0.0;
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
  const double E4m = 0.5 * (dg + dy * kViLog2 + 2.0 * hld2);
  const double cc2 = -0.5 * dy * kViLog2Pi + E4m + E2m[dx * kViLd + dx];
  const double lbm = -0.5 * dy * dc * kViLog2Pi;
  const double logZqm = -0.5 * dy * (2.0 * slK) + (0.5 * nu2 * dy * kViLog2 + mg + nu2 * hld2);
  const double iqm = aE1 + kE2 - 0.5 * cW + qdm * E4m;
  const double ipm = paE1 + pkE2 - 0.5 * pcW + md * E4m;
  const double term2 = (logZqm - lbm - iqm) - (a.mlz[bk] - lbm - ipm);
  const double ccj = o1.cc + cc2;

  // a canonical form or a term that is not finite (a digamma argument <= 0, an overflow): the problem's status, nothing written
  if (__any(!vi_bw_finite(D, lane, bjv, Wj)) || !vi_finite(ccj) || !vi_finite(o1.term) || !vi_finite(term2))
    return vi_fail(l, prob, lane, kViNotFinite);

  // ---- outputs: the posterior block, the terms, the b / W entries of the operand image ----------------------------------------
  vi_nw_store(P, L.basis(), k, dx, lane, nw, o1);
  vi_image_bw(vi_image(l, prob), l.NS, D, k, lane, bjv, Wj);
  if (lane < D) {
    P[L.m_bb() + k * D + lane] = b2v[lane];
    P[L.bb() + k * D + lane] = bjv[lane];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ei0 + 4 * r;
    if (i < dy && ej < dc) {
      const int e = (k * dy + i) * dc + ej;
      P[L.m_a() + e] = Am[i * kViLd + ej];
      P[L.m_Ms() + e] = Mm[i * kViLd + ej];
      P[L.m_E1() + e] = E1m[i * kViLd + ej];
    }
    if (i < dc && ej < dc) {
      const int e = (k * dc + i) * dc + ej;
      P[L.m_Kq() + e] = Kq[i * kViLd + ej];
      P[L.m_Kinv() + e] = Ki[i * kViLd + ej];
      P[L.m_E2() + e] = E2m[i * kViLd + ej];
    }
    if (i < dy && ej < dy) {
      const int e = (k * dy + i) * dy + ej;
      P[L.m_c() + e] = Cq[i * kViLd + ej];
      P[L.m_psis() + e] = Ps[i * kViLd + ej];
    }
    if (i < D && ej < D) {
      const int e = k * DD + i * D + ej;
      P[L.m_W() + e] = W2[i * kViLd + ej];
      P[L.W() + e] = Wj[i * kViLd + ej];
    }
  }
  if (lane == 0) {
    P[L.m_d() + k] = qdm;
    P[L.m_nus() + k] = nu2;
    P[L.m_hld() + k] = hld2;
    P[L.m_E4() + k] = E4m;
    P[L.m_cc() + k] = cc2;
    a.term_b[bk] = o1.term;
    a.term_m[bk] = term2;
  }
}

template <int M>
__global__ __launch_bounds__(64) void vi_ilr_gating_kernel(const ViIlrArgs a) {
  // g0, g1 of the posterior, of the prior; E[log stick | pi], E[log rest]; E[log pi]; c_total; six summands of the gating's term;
  // the basis terms, the experts' terms
  __shared__ double t[16][kBatchedMaxK];
  __shared__ double red[8];
  const ViLoop& l = a.loop;
  const int lane = threadIdx.x;
  const int K = l.K, D = l.D;
  const int prob = blockIdx.x;
  const ViIlrLayout L{K, a.dx, a.dy};
  ViProblem pr;
  if (!vi_problem<M>(l, prob, L.count(), pr)) return;
  double* const P = pr.P;
  const double* const C = pr.C;
  const double rho = l.rho, omr = l.one_minus_rho, inv = pr.inv;
  const size_t sstride = (size_t)(1 + D + D * D);
  const bool stick = a.gating == kViGatingStick;

  for (int k = lane; k < K; k += 64) t[8][k] = vi_stat<M>(l.S, ((size_t)prob * K + k) * sstride);      // the counts
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
      const double dsum = vi_digamma(g + d);
      t[0][k] = g; t[1][k] = d; t[2][k] = g0; t[3][k] = d0;
      t[4][k] = vi_digamma(g) - dsum;      // E[log stick]
      t[5][k] = vi_digamma(d) - dsum;      // E[log rest]
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
    const double ds = vi_digamma(s);
    lgs = lgamma(s);
    lgs0 = lgamma(s0);
    for (int k = lane; k < K; k += 64) {
      t[4][k] = vi_digamma(t[0][k]) - ds;
      t[5][k] = 0.0;
      t[6][k] = t[4][k];
    }
    wg_sync();
  }

  bool lane_bad = false;
  for (int k = lane; k < K; k += 64) {
    const double g = t[0][k], d = t[1][k], g0 = t[2][k], d0 = t[3][k], es = t[4][k], er = t[5][k];
    const double elp = t[6][k];
    const double ct = (P[L.basis().cc() + k] + P[L.m_cc() + k]) + elp;
    lane_bad = lane_bad || !vi_finite(elp) || !vi_finite(ct) || !vi_finite(er);
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
  if (__any(lane_bad)) return vi_fail(l, prob, lane, kViNotFinite);      // nothing of the gating is written
  for (int k = lane; k < K; k += 64) {       // (each lane reads back what it wrote itself)
    P[L.g0() + k] = t[0][k];
    P[L.g1() + k] = t[1][k];
    P[L.elp() + k] = t[6][k];
    P[L.c_total() + k] = t[7][k];
  }
  vi_image_c(vi_image(l, prob), l.NS, D, K, l.K16, lane, t[7]);
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
    if (!vi_finite(prior_terms)) return vi_fail(l, prob, lane, kViNotFinite);      // the slot does not become current
    P[L.vlb()] = gate;
    P[L.vlb() + 1] = red[6];
    P[L.vlb() + 2] = red[7];
    l.prior_terms[prob] = prior_terms;
    l.words[kViSlot * l.B + prob] = pr.slot;      // the block just written is the problem's current one
  }
}

bool ilr_args_ok(const ViIlrArgs& a) {
  return vi_loop_ok(a.loop) && a.dx >= 1 && a.dy >= 1 && a.loop.D == a.dx + a.dy &&
         (a.gating == kViGatingDirichlet || a.gating == kViGatingStick) && a.g0 && a.g1 && a.pa && a.pb && a.pc && a.pd && a.plz &&
         a.ma && a.mb && a.mc && a.md && a.mlz && a.term_b && a.term_m;
}

}  // namespace

hipError_t launch_vi_ilr_update(const ViIlrArgs& a, hipStream_t stream) {
  if (!ilr_args_ok(a) || (int64_t)a.loop.B * a.loop.K > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  vi_for_mode(a.loop.mode, [&](auto m) {
    hipLaunchKernelGGL(vi_ilr_update_kernel<decltype(m)::value>, dim3((unsigned)(a.loop.B * a.loop.K)), dim3(64), 0, stream, a);
  });
  return hipGetLastError();
}

hipError_t launch_vi_ilr_gating(const ViIlrArgs& a, hipStream_t stream) {
  if (!ilr_args_ok(a)) return hipErrorInvalidValue;
  vi_for_mode(a.loop.mode, [&](auto m) {
    hipLaunchKernelGGL(vi_ilr_gating_kernel<decltype(m)::value>, dim3((unsigned)a.loop.B), dim3(64), 0, stream, a);
  });
  return hipGetLastError();
}

}  // namespace mimo
