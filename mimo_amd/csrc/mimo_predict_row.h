// The per-row body of the register-form prediction kernels: everything predict_reg_kernel (mimo_predict.hip) and
// predict_batched_kernel (mimo_predict_batched.hip) do once a thread holds its row x~ = [x, 1] in registers — the gate maximum,
// the expert loop, the mixture or arg-max moments, the diagonal or full second output and the predictive log-density.  ONE copy:
// the solo kernel calls it with its PredictArgs, the batched kernel with a PredictArgs view of the workgroup's problem (the
// problem's parameter blocks, its output blocks, N = its row count) and the row's LOCAL index — so a problem's results are the
// solo kernel's, bit for bit, by construction.
#pragma once
#include "mimo_device.h"

namespace mimo {

typedef const double __attribute__((address_space(4)))* cptr_t;       // constant address space: uniform loads become s_load

// a: every pointer and scalar must be wave-uniform (the blocks are read through the constant address space).  x: the row, x[DX] = 1.
// n: the row's index within a.mu / a.covar / a.nlpd / a.N.  etab: the exponential table in LDS (exp_tab_entry_c, published).
// load_y(d): the d-th target of the row (0 on an invalid lane); called only where a.nlpd is set, inside the log-density section.
template <int DY, int DX, typename YLoad>
__device__ __forceinline__ void predict_row(const PredictArgs& a, const double (&x)[DX + 1], const int64_t n, const bool valid,
                                            const double* etab, YLoad&& load_y) {
  constexpr int DC = DX + 1;                   // affine: x~ = [x, 1]
  const cptr_t gate_p = (cptr_t)a.gate, M_p = (cptr_t)a.M, Q_p = (cptr_t)a.Q, Cc_p = (cptr_t)a.Cc;
  const int K = a.K;

  auto gate = [&](int k) {
    const cptr_t t = gate_p + (size_t)k * (1 + DX + DX * DX);
    double l = t[0];
#pragma unroll
    for (int i = 0; i < DX; ++i) {
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < DX; ++j) q = fma(t[1 + DX + i * DX + j], x[j], q);
      l = fma(x[i], t[1 + i] - 0.5 * q, l);
    }
    return l;
  };
  auto expert = [&](int k, double (&m)[DY], double& cs) {
    const cptr_t Mk = M_p + (size_t)k * DY * DC;
    const cptr_t Qk = Q_p + (size_t)k * DC * DC;
#pragma unroll
    for (int d = 0; d < DY; ++d) m[d] = 0.0;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < DC; ++i) {
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < DC; ++j) r = fma(Qk[i * DC + j], x[j], r);
      q = fma(x[i], r, q);
#pragma unroll
      for (int d = 0; d < DY; ++d) m[d] = fma(Mk[d * DC + i], x[i], m[d]);
    }
    cs = 1.0 + q;
  };

  double mx = -1e308, ssum = 0.0;
  double amu[DY], aS[DY][DY];
#pragma unroll
  for (int d = 0; d < DY; ++d) {
    amu[d] = 0.0;
#pragma unroll
    for (int e = 0; e < DY; ++e) aS[d][e] = 0.0;
  }
  int best = 0;
  if (a.mode == 1) {            // argmax only (first maximum, as np.argmax)
    for (int k = 0; k < K; ++k) {
      const double l = gate(k);
      if (l > mx) { mx = l; best = k; }
    }
  } else {
    for (int k = 0; k < K; ++k) mx = fmax(mx, gate(k));
    for (int k = 0; k < K; ++k) {
      const double w = exp_nonpos_t2048c(gate(k) - mx, etab);
      double m[DY], cs;
      expert(k, m, cs);
      const cptr_t Ck = Cc_p + (size_t)k * DY * DY;
      ssum += w;
#pragma unroll
      for (int d = 0; d < DY; ++d) {
        amu[d] = fma(w, m[d], amu[d]);
#pragma unroll
        for (int e = 0; e < DY; ++e) aS[d][e] = fma(w, fma(cs, Ck[d * DY + e], m[d] * m[e]), aS[d][e]);
      }
    }
  }
  if (a.mode == 1) {
    double m[DY], cs;
    expert(best, m, cs);
    const cptr_t Ck = Cc_p + (size_t)best * DY * DY;
    if (valid) {
#pragma unroll
      for (int d = 0; d < DY; ++d) {
        a.mu[n * DY + d] = m[d];
        if (a.diag) {
          const double v = cs * Ck[d * DY + d];
          a.covar[n * DY + d] = v;
          a.covar[(a.N + n) * DY + d] = sqrt(v);
        } else {
#pragma unroll
          for (int e = 0; e < DY; ++e) a.covar[(n * DY + d) * DY + e] = cs * Ck[d * DY + e];
        }
      }
    }
    if (a.nlpd) {               // the log-normaliser is still needed for the weights inside nlpd
      ssum = 0.0;
      for (int k = 0; k < K; ++k) ssum += exp_nonpos_t2048c(gate(k) - mx, etab);
    }
  } else if (valid) {
    const double inv = 1.0 / ssum;
#pragma unroll
    for (int d = 0; d < DY; ++d) amu[d] *= inv;
#pragma unroll
    for (int d = 0; d < DY; ++d) {
      a.mu[n * DY + d] = amu[d];
      if (a.diag) {
        const double v = aS[d][d] * inv - amu[d] * amu[d];
        a.covar[n * DY + d] = v;
        a.covar[(a.N + n) * DY + d] = sqrt(v);
      } else {
#pragma unroll
        for (int e = 0; e < DY; ++e) a.covar[(n * DY + d) * DY + e] = aS[d][e] * inv - amu[d] * amu[e];
      }
    }
  }
  if (a.nlpd) {
    const double lse = mx + log(ssum);
    double yv[DY];
#pragma unroll
    for (int d = 0; d < DY; ++d) yv[d] = load_y(d);
    double tm = -INFINITY, ts = 0.0;
    for (int k = 0; k < K; ++k) {
      const double w = exp(gate(k) - lse);
      double m[DY], cs;
      expert(k, m, cs);
      const cptr_t Pk = (cptr_t)a.P + (size_t)k * DY * DY;
      double q = 0.0;
#pragma unroll
      for (int d = 0; d < DY; ++d) {
        double r = 0.0;
#pragma unroll
        for (int e = 0; e < DY; ++e) r = fma(Pk[d * DY + e], yv[e] - m[e], r);
        q = fma(yv[d] - m[d], r, q);
      }
      const double lpl = -0.5 * q / cs - 0.5 * DY * 1.8378770664093453 + 0.5 * (((cptr_t)a.ld)[k] - DY * log(cs));
      const double t = lpl + log(w + 2.2250738585072014e-308);
      if (t > tm) { ts = ts * exp(tm - t) + 1.0; tm = t; }
      else ts += exp(t - tm);
    }
    if (valid) a.nlpd[n] = -(tm + log(ts));
  }
}

}  // namespace mimo
