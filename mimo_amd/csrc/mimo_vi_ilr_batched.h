// Internal interface of the device-resident batched VI loop for mixtures of linear-Gaussian experts (mimo_vi_ilr_batched.hip): the
// conjugate update of the basis (Normal-Wishart over x), of the affine experts (matrix-normal-Wishart of y | [x, 1]) and of the
// gating (Dirichlet or truncated stick-breaking), the joint canonical form over z = [x, y] and the prior terms of the bound of B
// models between two batched softmax passes, without a host round trip.  The loop's words, its status bits, its pass and its finish
// kernel are those of mimo_vi_batched.h.  Not installed; the public surface is include/mimo_hip.h.
#pragma once
#include "mimo_vi_batched.h"

namespace mimo {

// gating kinds (the public MIMO_VI_GATING_* of include/mimo_hip.h)
constexpr int kViGatingDirichlet = 0;
constexpr int kViGatingStick = 1;

// One problem's posterior block.  dc = dx + 1 (affine experts), D = dx + dy.
//   gating   g0 K (alpha | gamma) | g1 K (zeros | delta) | E[log pi] K
//   basis    the Normal-Wishart parts over dx (ViNwLayout, mimo_vi_batched.h)
//   experts  a K dy dc | Kq K dc^2 | c K dy^2 | d K | Ms K dy dc | psis K dy^2 | nus K | hld K | Kinv K dc^2 | E1 K dy dc |
//            E2 K dc^2 | E4 K | cc K | bb K D | W K D^2
//   joint    c_total K | bb K D | W K D^2
//   bound    3: the gating term, the summed basis terms, the summed expert terms
struct ViIlrLayout {
  int K, dx, dy;
  __host__ __device__ int dc() const { return dx + 1; }
  __host__ __device__ int D() const { return dx + dy; }
  __host__ __device__ int g0() const { return 0; }
  __host__ __device__ int g1() const { return K; }
  __host__ __device__ int elp() const { return 2 * K; }
  __host__ __device__ ViNwLayout basis() const { return {K, dx, 3 * K}; }
  // experts
  __host__ __device__ int m_a() const { return basis().end(); }
  __host__ __device__ int m_Kq() const { return m_a() + K * dy * dc(); }
  __host__ __device__ int m_c() const { return m_Kq() + K * dc() * dc(); }
  __host__ __device__ int m_d() const { return m_c() + K * dy * dy; }
  __host__ __device__ int m_Ms() const { return m_d() + K; }
  __host__ __device__ int m_psis() const { return m_Ms() + K * dy * dc(); }
  __host__ __device__ int m_nus() const { return m_psis() + K * dy * dy; }
  __host__ __device__ int m_hld() const { return m_nus() + K; }
  __host__ __device__ int m_Kinv() const { return m_hld() + K; }
  __host__ __device__ int m_E1() const { return m_Kinv() + K * dc() * dc(); }
  __host__ __device__ int m_E2() const { return m_E1() + K * dy * dc(); }
  __host__ __device__ int m_E4() const { return m_E2() + K * dc() * dc(); }
  __host__ __device__ int m_cc() const { return m_E4() + K; }
  __host__ __device__ int m_bb() const { return m_cc() + K; }
  __host__ __device__ int m_W() const { return m_bb() + K * D(); }
  // joint
  __host__ __device__ int c_total() const { return m_W() + K * D() * D(); }
  __host__ __device__ int bb() const { return c_total() + K; }
  __host__ __device__ int W() const { return bb() + K * D(); }
  __host__ __device__ int vlb() const { return W() + K * D() * D(); }
  __host__ __device__ int count() const { return vlb() + 3; }
};

// The priors of one batch, in the order mimo_vi_ilr_prior_batched stores them:
//   g0 B K | g1 B K | basis pa B K dx | pb B K | pc B K dx^2 | pd B K | log Z B K |
//   experts ma B K dy dc | mb B K dc^2 | mc B K dy^2 | md B K | log Z B K
struct ViIlrArgs {
  ViLoop loop;                // post: [2][B][ViIlrLayout::count()]; D = dx + dy
  const double* g0;           // [B][K] alpha0 | gamma0
  const double* g1;           // [B][K] unused | delta0
  const double* pa; const double* pb; const double* pc; const double* pd; const double* plz;      // basis
  const double* ma; const double* mb; const double* mc; const double* md; const double* mlz;      // experts
  double* term_b;             // [B][K]: the basis blocks' terms of the bound (update kernel -> gating kernel)
  double* term_m;             // [B][K]: the experts' terms
  int dx, dy, gating;
};

// update: one wave per (problem, component); gating: one wave per problem.  Both return at once for a problem that is not active
// or whose status word is set.  (The iteration's finish is launch_vi_finish on a.loop.)
hipError_t launch_vi_ilr_update(const ViIlrArgs& a, hipStream_t stream);
hipError_t launch_vi_ilr_gating(const ViIlrArgs& a, hipStream_t stream);

}  // namespace mimo
