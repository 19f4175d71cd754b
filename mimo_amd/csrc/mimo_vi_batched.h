// Internal interface of the device-resident batched VI loop (mimo_vi_batched.hip): the conjugate update, the canonical form and
// the prior terms of the bound of B mixtures of Gaussians (Dirichlet gating, untied Normal-Wishart components) between two
// batched softmax passes, without a host round trip.  Not installed; the public surface is include/mimo_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mimo {

// The thirteen parts of K Normal-Wishart blocks over n dimensions, from offset `base` of a posterior block (the components of
// ViLayout, the basis of ViIlrLayout):
//   qa K n | qb K | qc K n n | qd K | mus K n | psis K n n | nus K | hld K | cc K | bb K n | W K n n | E2 K | E4 K
struct ViNwLayout {
  int K, n, base;
  __host__ __device__ int kn() const { return K * n; }
  __host__ __device__ int knn() const { return K * n * n; }
  __host__ __device__ int qa() const { return base; }
  __host__ __device__ int qb() const { return qa() + kn(); }
  __host__ __device__ int qc() const { return qb() + K; }
  __host__ __device__ int qd() const { return qc() + knn(); }
  __host__ __device__ int mus() const { return qd() + K; }
  __host__ __device__ int psis() const { return mus() + kn(); }
  __host__ __device__ int nus() const { return psis() + knn(); }
  __host__ __device__ int hld() const { return nus() + K; }
  __host__ __device__ int cc() const { return hld() + K; }
  __host__ __device__ int bb() const { return cc() + K; }
  __host__ __device__ int W() const { return bb() + kn(); }
  __host__ __device__ int E2() const { return W() + knn(); }
  __host__ __device__ int E4() const { return E2() + K; }
  __host__ __device__ int end() const { return E4() + K; }
};

// One problem's posterior block, in the part order of the host-native sweep's output block (distributions/native_sweep.py, untied):
//   alpha K | the Normal-Wishart parts over Dz (nw()) | E[log pi] K | c_total K |
//   bound terms 2 (Dirichlet term, sum of the component terms)
struct ViLayout {
  int K, D;
  __host__ __device__ int alpha() const { return 0; }
  __host__ __device__ ViNwLayout nw() const { return {K, D, K}; }
  __host__ __device__ int elp() const { return nw().end(); }
  __host__ __device__ int c_total() const { return elp() + K; }
  __host__ __device__ int vlb() const { return c_total() + K; }
  __host__ __device__ int count() const { return vlb() + 2; }
};

// The loop's per-problem words, one int32 row of B each: [active | status | appended in all | appended in this call | current slot]
enum ViWord : int { kViActive = 0, kViStatus = 1, kViTotal = 2, kViDone = 3, kViSlot = 4, kViWords = 5 };
// status bits
constexpr int kViNotPosDef = 1;      // a component's posterior block C = c - kappa m m' is not positive definite
constexpr int kViNotFinite = 2;      // a canonical form (c, b, W), a term of the bound or the bound itself is not finite

// How the update and the gating kernel form the posterior's natural parameters (wave-uniform, ViLoop::mode):
//   conjugate  eta = eta_prior + S                                            (coordinate descent: mimo_vi_run_batched)
//   blend      eta = (1 - rho) eta_cur + rho (eta_prior + inv_scale_b S)      (the SVI step: mimo_svi_run_batched), eta_cur the
//              natural parameters of the problem's current slot; the products are not contracted into the sums, in the order of
//              _ConjugateBlock._apply_sgd: t = inv S, u = eta_prior + t, v = rho u, w = (1 - rho) eta_cur, w + v
//   init       eta = eta_cur: no statistics are read (mimo_svi_state_batched: the derived parts, the image and the prior terms of
//              an uploaded posterior)
// Everything behind eta is the same code in all three, and the block goes to the slot that is not current.
enum ViMode : int { kViConjugate = 0, kViBlend = 1, kViInit = 2 };

// What the pass, its reduction and vi_finish_kernel read, and what the update and gating kernels of both families share
struct ViLoop {
  const double* S;            // [B][K][1 + D + D^2]: the resident statistics block (launch_batched_reduce)
  const double* scalars;      // [B][3]: the scalars of the same reduction
  double* post;               // [2][B][the family's layout's count()]: two slots per problem; words[kViSlot][b] names the current
                              // one.  An iteration writes the other slot and the gating kernel makes it current once the whole
                              // problem is done, so a problem that fails keeps the block it had
  double* prior_terms;        // [B]: the gating's term + the sums of the component terms (gating kernel -> finish kernel)
  double* last;               // [B]: the bound appended last
  int32_t* words;             // [kViWords][B]
  double* theta;              // [B][K16][NS][64]: the operand images the batched pass reads (ThetaGeneric, identity order)
  double* trace;              // [iters][B] of this call
  int B, K, D, K16, NS;
  double tol;
  // the SVI step (mode != kViConjugate); the zeros of ViLoop{} are the conjugate update
  int mode;                   // ViMode
  double rho, one_minus_rho;  // the step size and 1 - rho as the host rounds it
  const double* inv_scale;    // [B]: 1 / scale_b as the host rounds it, scale_b = batch size / N_b (blend only)
};

struct ViArgs {
  ViLoop loop;                // post: [2][B][ViLayout::count()]
  // the priors' natural parameters and log-partitions
  const double* alpha0;       // [B][K]
  const double* pa;           // [B][K][D]
  const double* pb;           // [B][K]
  const double* pc;           // [B][K][D][D]
  const double* pd;           // [B][K]
  const double* plz;          // [B][K]
  double* term;               // [B][K]: the components' terms of the bound (update kernel -> gating kernel)
};

// update: one wave per (problem, component); gating: one wave per problem.  Both return at once for a problem that is not active
// or whose status word is set.
hipError_t launch_vi_update(const ViArgs& a, hipStream_t stream);
hipError_t launch_vi_gating(const ViArgs& a, hipStream_t stream);
// finish (behind the pass and its reduction), iteration `it` of this call: trace[it][b] = prior_terms[b] + scalars[b][0] for an
// active problem (NaN otherwise), and active[b] = 0 once two consecutive bounds are closer than tol.
hipError_t launch_vi_finish(const ViLoop& l, int it, hipStream_t stream);

// The minibatch indices of `n_it` SVI iterations, one lane per (iteration, problem, slot): for iteration i < n_it, problem b and
// slot j < sel_off[b + 1] - sel_off[b],
//   sel[i sel_off[B] + sel_off[b] + j] = min((int64)(philox_uniform(seeds[b], j, t0 + i) N_b), N_b - 1),  N_b = row_off[b + 1] - row_off[b]
// (a draw with replacement; a problem without rows gets no slots: the caller checks).  All pointers are device pointers.
hipError_t launch_svi_indices(int64_t* sel, const int64_t* sel_off, const int64_t* row_off, const uint64_t* seeds, int B, int n_it,
                              int64_t per_it, uint64_t t0, hipStream_t stream);

}  // namespace mimo
