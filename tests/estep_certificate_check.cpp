// mimo_host_estep_certificate under AddressSanitizer + UBSan: built together with mimo_amd/csrc/mimo_host.cpp as a stand-alone
// host program (tests/test_estep_certificate_cpu.py).  Every input and output sits in a heap block of exactly its length, so an
// entry read or written past the end is a sanitizer error; what comes back must be finite where a bound exists, ordered
// (rho <= 1 <= rho_bar for a reference compared with itself), and the same on a second call.
#include "../include/mimo_hip.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

static void posterior(std::mt19937_64& g, int K, int D, double move, const std::vector<double>* from, std::vector<double>& c,
                      std::vector<double>& b, std::vector<double>& W) {
  std::normal_distribution<double> nd;
  c.assign((size_t)K, 0.0); b.assign((size_t)K * D, 0.0); W.assign((size_t)K * D * D, 0.0);
  for (int k = 0; k < K; ++k) {
    std::vector<double> A((size_t)D * D);
    for (auto& v : A) v = nd(g);
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        double s = i == j ? 0.5 : 0.0;
        for (int r = 0; r < D; ++r) s += A[(size_t)i * D + r] * A[(size_t)j * D + r] / D;
        W[((size_t)k * D + i) * D + j] = from ? (*from)[((size_t)k * D + i) * D + j] * (1.0 + move) + move * s : s;
      }
    for (int i = 0; i < D; ++i) b[(size_t)k * D + i] = 3.0 * nd(g);
    c[k] = k % 7 == 0 ? -800.0 : -20.0 + nd(g);        // every seventh component sits far under the others
  }
}

static int check(int K, int D, double move, const char* what) {
  std::mt19937_64 g((unsigned)(K * 131 + D));
  std::vector<double> c0, b0, W0, c, b, W;
  posterior(g, K, D, 0.0, nullptr, c0, b0, W0);
  if (move == 0.0) { c = c0; b = b0; W = W0; }
  else posterior(g, K, D, move, &W0, c, b, W);
  std::vector<double> out((size_t)5 * K + 4, -7.0), table((size_t)4 + 2 * K, -7.0), out2(out), table2(table);
  int rc = mimo_host_estep_certificate(K, D, c0.data(), b0.data(), W0.data(), c.data(), b.data(), W.data(), -41.6, out.data(), table.data());
  if (rc != MIMO_OK) { printf("%s K=%d D=%d: rc=%d\n", what, K, D, rc); return 1; }
  for (int k = 0; k < K; ++k) {
    const double rho = out[2 * (size_t)K + k], rhob = out[3 * (size_t)K + k], d = out[4 * (size_t)K + k];
    if (!(rho >= 0.0 && rho <= 1.0 && rhob >= 1.0 && d >= 0.0) || !std::isfinite(out[k]) || !std::isfinite(out[(size_t)K + k])) {
      printf("%s K=%d D=%d: component %d: rho %g rho_bar %g d %g\n", what, K, D, k, rho, rhob, d);
      return 1;
    }
    if (move == 0.0 && (rho != 1.0 || rhob != 1.0 || d != 0.0)) { printf("%s K=%d D=%d: the reference against itself moved\n", what, K, D); return 1; }
  }
  rc = mimo_host_estep_certificate(K, D, c0.data(), b0.data(), W0.data(), c.data(), b.data(), W.data(), -41.6, out2.data(), table2.data());
  if (rc != MIMO_OK || out2 != out || table2 != table) { printf("%s K=%d D=%d: a second call differs\n", what, K, D); return 1; }
  rc = mimo_host_estep_certificate(K, D, c0.data(), b0.data(), W0.data(), c.data(), b.data(), W.data(), -41.6, out2.data(), nullptr);
  if (rc != MIMO_OK || out2 != out) { printf("%s K=%d D=%d: without the table the constants differ\n", what, K, D); return 1; }
  return 0;
}

int main() {
  for (int K : {1, 2, 17, 64, 256})
    for (int D : {1, 3, 16, 32}) {
      if (check(K, D, 0.0, "itself")) return 1;
      if (check(K, D, 0.01, "small move")) return 1;
      if (check(K, D, 5.0, "large move")) return 1;
    }
  // the rejections
  const int K = 8, D = 4;
  std::mt19937_64 g(3);
  std::vector<double> c, b, W, out((size_t)5 * K + 4), table((size_t)4 + 2 * K);
  posterior(g, K, D, 0.0, nullptr, c, b, W);
  auto call = [&](int k, int d, const double* pc, const double* pb, const double* pW, double* po) {
    return mimo_host_estep_certificate(k, d, pc, pb, pW, c.data(), b.data(), W.data(), -41.6, po, table.data());
  };
  int bad = 0;
  bad += call(0, D, c.data(), b.data(), W.data(), out.data()) != MIMO_E_INVALID;
  bad += call(K, 0, c.data(), b.data(), W.data(), out.data()) != MIMO_E_INVALID;
  bad += call(K, D, nullptr, b.data(), W.data(), out.data()) != MIMO_E_INVALID;
  bad += call(K, D, c.data(), nullptr, W.data(), out.data()) != MIMO_E_INVALID;
  bad += call(K, D, c.data(), b.data(), nullptr, out.data()) != MIMO_E_INVALID;
  bad += call(K, D, c.data(), b.data(), W.data(), nullptr) != MIMO_E_INVALID;
  bad += call(257, 1, c.data(), b.data(), W.data(), out.data()) != MIMO_E_UNSUPPORTED;
  bad += call(1, 33, c.data(), b.data(), W.data(), out.data()) != MIMO_E_UNSUPPORTED;
  std::vector<double> Wbad(W);
  Wbad[5] = std::nan("");
  bad += call(K, D, c.data(), b.data(), Wbad.data(), out.data()) != MIMO_E_INVALID;
  Wbad = W;
  Wbad[(size_t)2 * D * D] = -1.0;                        // component 2 is not positive definite
  bad += call(K, D, c.data(), b.data(), Wbad.data(), out.data()) != MIMO_E_INVALID;
  if (bad) { printf("%d rejections missing\n", bad); return 1; }
  printf("estep certificate ok\n");
  return 0;
}
