// Device-resident batched VI (gfx950): what stands between two batched softmax passes of B mixtures of Gaussians — the conjugate
// update of the K Normal-Wishart blocks and of the Dirichlet gating from the resident statistics, the canonical form (c, b, W) as
// the operand image the next pass reads, the prior terms of the bound and the stopping rule — as three small kernels, so that a
// whole mean-field iteration is five stream-ordered launches and no host round trip:
//
//   vi_update_kernel   one wave per (problem, component): the arithmetic of mimo_host_gmm_vi_sweep + mimo_host_nw_vi + one
//                      component of mimo_host_nw_vlb (mimo_host.cpp), the Dz x Dz block in LDS: vi_nw_block of mimo_vi_device.h,
//                      which the basis of the linear-Gaussian experts' loop (mimo_vi_ilr_batched.hip) runs too
//   vi_gating_kernel   one wave per problem: the Dirichlet update, E[log pi], c_total into the image, the Dirichlet term of
//                      mimo_host_gmm_vi_bound and the sum of the component terms
//   (launch_batched, launch_batched_reduce: the pass and its reduction, mimo_batched.hip)
//   vi_finish_kernel   one lane per problem: the bound into the trace, the stopping rule (both families)
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
#include "mimo_vi_device.h"

namespace mimo {

namespace {

template <int M>
__global__ __launch_bounds__(64) void vi_update_kernel(const ViArgs a) {
  __shared__ double Qc[kViBlk], U[kViBlk], X[kViBlk], Wm[kViBlk];
  __shared__ double vec[8][16];
  const ViLoop& l = a.loop;
  const int lane = threadIdx.x;
  const int K = l.K, D = l.D, DD = D * D;
  const int prob = blockIdx.x / K, k = blockIdx.x - prob * K;
  const ViLayout L{K, D};
  ViProblem p;
  if (!vi_problem<M>(l, prob, L.count(), p)) return;
  const size_t bk = (size_t)prob * K + k;
  const double* const Sk = l.S + bk * (size_t)(1 + D + DD);
  const ViNwLds s{Qc, U, X, Wm, vec};
  const ViNwIn in{a.pa + bk * D, a.pb + bk, a.pc + bk * DD, a.pd + bk, a.plz + bk, Sk, Sk + 1, Sk + 1 + D, D,
                  p.C, L.nw(), k, D, l.rho, l.one_minus_rho, p.inv};
  ViNwOut o;
  if (!vi_nw_block<M>(in, s, lane, o)) return vi_fail(l, prob, lane, kViNotPosDef);

  // a canonical form or a term that is not finite (a digamma argument <= 0, an overflow): the host packing path refuses such a
  // block (theta_entries), here it sets the problem's status and, like a bad pivot, writes nothing for this component
  if (__any(!vi_bw_finite(D, lane, s.b(), Wm)) || !vi_finite(o.cc) || !vi_finite(o.term))
    return vi_fail(l, prob, lane, kViNotFinite);

  vi_nw_store(p.P, L.nw(), k, D, lane, s, o);
  vi_image_bw(vi_image(l, prob), l.NS, D, k, lane, s.b(), Wm);
  if (lane == 0) a.term[bk] = o.term;
}

template <int M>
__global__ __launch_bounds__(64) void vi_gating_kernel(const ViArgs a) {
  // alpha, alpha0, lgamma(alpha), lgamma(alpha0), (alpha - 1) E, (alpha0 - 1) E, terms, E[log pi], c_total
  __shared__ double t[9][kBatchedMaxK];
  __shared__ double red[8];
  const ViLoop& l = a.loop;
  const int lane = threadIdx.x;
  const int K = l.K, D = l.D;
  const int prob = blockIdx.x;
  const ViLayout L{K, D};
  ViProblem p;
  if (!vi_problem<M>(l, prob, L.count(), p)) return;
  double* const P = p.P;
  const size_t sstride = (size_t)(1 + D + D * D);

  // Dirichlet gating: alpha = ((alpha0 - 1) + n) + 1; the blend runs on the natural parameter alpha - 1 (gating.py: std_to_nat /
  // nat_to_std around CategoricalWithDirichlet.meanfield_sgd); init keeps the uploaded alpha itself
  for (int k = lane; k < K; k += 64) {
    const size_t bk = (size_t)prob * K + k;
    const double a0 = a.alpha0[bk];
    if constexpr (M == kViInit) t[0][k] = p.C[L.alpha() + k];
    else t[0][k] = vi_eta<M>(a0 - 1.0, l.S[bk * sstride], vi_cur<M>(p.C, L.alpha() + k) - 1.0, l.rho, l.one_minus_rho, p.inv) + 1.0;
    t[1][k] = a0;
  }
  wg_sync();
  double s = 0.0, s0 = 0.0;
  for (int k = 0; k < K; ++k) { s += t[0][k]; s0 += t[1][k]; }      // on every lane alike, ascending
  const double ds = vi_digamma(s);
  bool lane_bad = false;
  for (int k = lane; k < K; k += 64) {
    const double al = t[0][k], a0 = t[1][k];
    const double elp = vi_digamma(al) - ds;
    const double ct = P[L.nw().cc() + k] + elp;
    lane_bad = lane_bad || !vi_finite(elp) || !vi_finite(ct);
    t[7][k] = elp;
    t[8][k] = ct;
    t[2][k] = lgamma(al);
    t[3][k] = lgamma(a0);
    t[4][k] = (al - 1.0) * elp;
    t[5][k] = (a0 - 1.0) * elp;
    t[6][k] = a.term[(size_t)prob * K + k];
  }
  // (alpha <= 0: theta_entries refuses a NaN c) nothing of the gating is written
  if (__any(lane_bad)) return vi_fail(l, prob, lane, kViNotFinite);
  for (int k = lane; k < K; k += 64) {       // (each lane reads back what it wrote itself)
    P[L.alpha() + k] = t[0][k];
    P[L.elp() + k] = t[7][k];
    P[L.c_total() + k] = t[8][k];
  }
  vi_image_c(vi_image(l, prob), l.NS, D, K, l.K16, lane, t[8]);
  wg_sync();
  if (lane < 5) {                            // lq, lp, iq, ip, the component terms: ascending k, one sum per lane
    double v = 0.0;
    for (int k = 0; k < K; ++k) v += t[2 + lane][k];
    red[lane] = v;
  }
  wg_sync();
  if (lane == 0) {
    const double dir = ((red[0] - lgamma(s)) - red[2]) - ((red[1] - lgamma(s0)) - red[3]);
    if (!vi_finite(dir + red[4])) return vi_fail(l, prob, lane, kViNotFinite);      // the slot does not become current
    P[L.vlb()] = dir;
    P[L.vlb() + 1] = red[4];
    l.prior_terms[prob] = dir + red[4];
    l.words[kViSlot * l.B + prob] = p.slot;  // the block just written is the problem's current one
  }
}

__global__ __launch_bounds__(256) void vi_finish_kernel(const ViLoop a, int it) {
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

bool vi_args_ok(const ViArgs& a) {
  return vi_loop_ok(a.loop) && a.alpha0 && a.pa && a.pb && a.pc && a.pd && a.plz && a.term;
}

}  // namespace

hipError_t launch_vi_update(const ViArgs& a, hipStream_t stream) {
  if (!vi_args_ok(a) || (int64_t)a.loop.B * a.loop.K > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  vi_for_mode(a.loop.mode, [&](auto m) {
    hipLaunchKernelGGL(vi_update_kernel<decltype(m)::value>, dim3((unsigned)(a.loop.B * a.loop.K)), dim3(64), 0, stream, a);
  });
  return hipGetLastError();
}

hipError_t launch_vi_gating(const ViArgs& a, hipStream_t stream) {
  if (!vi_args_ok(a)) return hipErrorInvalidValue;
  vi_for_mode(a.loop.mode, [&](auto m) {
    hipLaunchKernelGGL(vi_gating_kernel<decltype(m)::value>, dim3((unsigned)a.loop.B), dim3(64), 0, stream, a);
  });
  return hipGetLastError();
}

hipError_t launch_vi_finish(const ViLoop& l, int it, hipStream_t stream) {
  if (!vi_loop_ok(l) || it < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vi_finish_kernel, dim3((unsigned)((l.B + 255) / 256)), dim3(256), 0, stream, l, it);
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
