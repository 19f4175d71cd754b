// Internal interface of the batched prediction kernel (mimo_predict_batched.hip): the posterior-predictive moments of B ILR models
// that share K, dx and dy, each with its own parameter blocks and its own query rows (or all on one shared set of rows), in one
// launch.  Not installed; the public surface is include/mimo_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mimo {

constexpr int kPredictBatchedMaxDx = 8;      // the row lives in registers: the shapes of predict_reg_kernel (affine experts, dc = dx + 1)
constexpr int kPredictBatchedMaxDy = 8;
constexpr int kPredictBatchedMaxB = 65535;   // the problem is blockIdx.y

struct PredictBatchedArgs {
  const double* X;            // ragged: (row_off[B], dx), the problems' query rows concatenated; shared: (N_shared, dx)
  const int64_t* row_off;     // [B + 1] on the device, or null: the shared form
  int64_t N_shared;           // rows of the shared form (0 in the ragged form)
  int B, dx, dy, K, mode, diag;
  const double* x_tf;         // [B][2][dx] (shift, scale) or null: rows as they are
  const double* y_tf;         // [B][2][dy] or null
  const double* gate;         // [B][K][1 + dx + dx*dx]
  const double* M;            // [B][K][dy][dx + 1]
  const double* Q;            // [B][K][dx + 1][dx + 1]
  const double* Cc;           // [B][K][dy][dy]
  const double* P;            // [B][K][dy][dy]  (read only with nlpd)
  const double* ld;           // [B][K]
  const double* y;            // rows in the form of X, dy columns; or null
  // problem b's blocks start at row o_b = row_off[b] (ragged) or b N_shared (shared), in the solo layouts with N = N_b:
  double* mu;                 // o_b dy
  double* covar;              // o_b dy dy, or with diag o_b 2 dy: [var (N_b, dy) | std (N_b, dy)]
  double* nlpd;               // o_b, or null
};

bool predict_batched_covers(int dx, int dy);
// max_rows: the largest problem's row count (the grid's x extent); nothing is launched for an all-empty batch
hipError_t launch_predict_batched(const PredictBatchedArgs& a, int64_t max_rows, hipStream_t stream);

}  // namespace mimo
