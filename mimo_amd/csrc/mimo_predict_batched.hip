// Posterior-predictive mixture moments of B independent ILR models in one launch (mimo_predict_batched; reference: the loop of
// examples/ilr/evaluate_sinc_parallel.py:196-201 over mimo/mixtures/ilr.py:374-430): the register-form prediction of
// mimo_predict.hip with the problem as the grid's second dimension.  One thread per query row, 256 rows per workgroup,
// grid = (max_b ceil(N_b / 256), B), prob = blockIdx.y; the per-row body is predict_row (mimo_predict_row.h), the solo kernel's.
//
// A row's result depends on no other row and on nothing of the batch but its own problem's blocks: no work table, no
// partial sums — a problem's outputs are the same bits alone, at any position of any batch, in the ragged and in the shared
// form.  prob, the row range and every per-problem base pointer are functions of blockIdx.y and of loads through the constant
// address space at uniform addresses: they stay in scalar registers, and the parameter loads of the component loops stay s_load.
// A workgroup whose first row lies past its problem's end returns before the table barrier (a uniform branch).
//
// Standardisation (x_tf / y_tf, the (shift, scale) rows of Standardizer.transform): x_i = (X[n, i] - shift_i) / scale_i as one IEEE
// subtraction and one IEEE division (no reciprocal, nothing to contract) — the bits NumPy computes.
#include "mimo_predict_batched.h"
#include "mimo_predict_row.h"

namespace mimo {

typedef const int64_t __attribute__((address_space(4)))* ciptr_t;

template <int DY, int DX>
__global__ __launch_bounds__(256) void predict_batched_kernel(const PredictBatchedArgs a) {
  constexpr int DC = DX + 1;
  __shared__ double etab[kExpTab];
  const int tid = threadIdx.x;
  const int prob = blockIdx.y;
  // the problem's query rows [in0, in0 + Nb) of X (and y), its outputs from row out0 on
  int64_t in0 = 0, out0 = (int64_t)prob * a.N_shared, Nb = a.N_shared;
  if (a.row_off) {
    const ciptr_t ro = (ciptr_t)a.row_off;
    in0 = out0 = ro[prob];
    Nb = ro[prob + 1] - in0;
  }
  const int64_t n0 = (int64_t)blockIdx.x * 256;
  if (n0 >= Nb) return;                        // uniform: the whole workgroup leaves before the barrier
  for (int e = tid; e < kExpTab; e += 256) etab[e] = exp_tab_entry_c(e);
  wg_sync();

  const int K = a.K;
  const size_t kp = (size_t)prob * K;
  PredictArgs r;                               // the problem as the solo kernel would see it
  r.Z = nullptr; r.N = Nb; r.dx = DX; r.dc = DC; r.dy = DY; r.K = K; r.mode = a.mode; r.diag = a.diag;
  r.gate = a.gate + kp * (1 + DX + DX * DX);
  r.M = a.M + kp * (DY * DC);
  r.Q = a.Q + kp * (DC * DC);
  r.Cc = a.Cc + kp * (DY * DY);
  r.P = a.P + kp * (DY * DY);
  r.ld = a.ld + kp;
  r.y = nullptr;
  r.mu = a.mu + out0 * DY;
  r.covar = a.covar + out0 * (a.diag ? 2 * DY : DY * DY);
  r.nlpd = a.nlpd ? a.nlpd + out0 : nullptr;

  const int64_t n = n0 + tid;                  // local row
  const bool valid = n < Nb;
  double x[DC];
  {
#pragma clang fp contract(off)
    const double* xr = a.X + (in0 + n) * DX;
    if (a.x_tf) {
      const cptr_t tf = (cptr_t)a.x_tf + (size_t)prob * 2 * DX;
#pragma unroll
      for (int i = 0; i < DX; ++i) x[i] = valid ? (xr[i] - tf[i]) / tf[DX + i] : 0.0;
    } else {
#pragma unroll
      for (int i = 0; i < DX; ++i) x[i] = valid ? xr[i] : 0.0;
    }
  }
  x[DX] = 1.0;
  predict_row<DY, DX>(r, x, n, valid, etab, [&](int d) {
#pragma clang fp contract(off)
    if (!valid) return 0.0;
    const double v = a.y[(in0 + n) * DY + d];
    if (!a.y_tf) return v;
    const cptr_t tf = (cptr_t)a.y_tf + (size_t)prob * 2 * DY;
    return (v - tf[d]) / tf[DY + d];
  });
}

typedef void (*predict_batched_fn)(const PredictBatchedArgs);
template <int DX>
static predict_batched_fn pick_dy(int dy) {
  switch (dy) {
    case 1: return predict_batched_kernel<1, DX>; case 2: return predict_batched_kernel<2, DX>;
    case 3: return predict_batched_kernel<3, DX>; case 4: return predict_batched_kernel<4, DX>;
    case 5: return predict_batched_kernel<5, DX>; case 6: return predict_batched_kernel<6, DX>;
    case 7: return predict_batched_kernel<7, DX>; case 8: return predict_batched_kernel<8, DX>;
  }
  return nullptr;
}

bool predict_batched_covers(int dx, int dy) {
  return dx >= 1 && dx <= kPredictBatchedMaxDx && dy >= 1 && dy <= kPredictBatchedMaxDy;
}

hipError_t launch_predict_batched(const PredictBatchedArgs& a, int64_t max_rows, hipStream_t stream) {
  predict_batched_fn fn = nullptr;
  switch (a.dx) {
    case 1: fn = pick_dy<1>(a.dy); break; case 2: fn = pick_dy<2>(a.dy); break;
    case 3: fn = pick_dy<3>(a.dy); break; case 4: fn = pick_dy<4>(a.dy); break;
    case 5: fn = pick_dy<5>(a.dy); break; case 6: fn = pick_dy<6>(a.dy); break;
    case 7: fn = pick_dy<7>(a.dy); break; case 8: fn = pick_dy<8>(a.dy); break;
  }
  if (!fn || a.B < 1 || a.B > kPredictBatchedMaxB) return hipErrorInvalidValue;
  if (max_rows <= 0) return hipSuccess;
  const int64_t gx = (max_rows + 255) / 256;
  if (gx > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((unsigned)gx, (unsigned)a.B), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mimo
