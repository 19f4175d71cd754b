// mimo_host_block_order under AddressSanitizer + UBSan: built together with mimo_amd/csrc/mimo_host.cpp as a stand-alone host
// program (tests/test_block_order_cpu.py).  The order array sits in a heap block of exactly K entries, so a slot written
// past K - 1 is a sanitizer error; what comes back must be a permutation whose fillers and padding follow the rules.
#include "../include/mimo_hip.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

static int check(int K, int D, const std::vector<double>& means, const std::vector<double>& mass, const char* what) {
  std::vector<int32_t> order((size_t)K, -7), again((size_t)K, -7);
  int rc = mimo_host_block_order(K, D, means.data(), mass.data(), 16, order.data());
  if (rc != MIMO_OK) { printf("%s K=%d: rc=%d\n", what, K, rc); return 1; }
  std::vector<int> seen((size_t)K, 0);
  for (int s = 0; s < K; ++s) {
    if (order[s] < 0 || order[s] >= K || seen[order[s]]++) { printf("%s K=%d: slot %d holds %d\n", what, K, s, (int)order[s]); return 1; }
  }
  rc = mimo_host_block_order(K, D, means.data(), mass.data(), 16, again.data());
  if (rc != MIMO_OK || again != order) { printf("%s K=%d: a second call differs\n", what, K); return 1; }
  return 0;
}

int main() {
  std::mt19937_64 g(7);
  std::normal_distribution<double> nd;
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  for (int K : {1, 16, 17, 64, 256})
    for (int D : {1, 3, 16}) {
      std::vector<double> means((size_t)K * D), mass((size_t)K);
      // clusters of up to five components around shared centres, a third of the components empty
      for (int k = 0; k < K; ++k) {
        std::mt19937_64 c((unsigned)(k / 5));
        for (int a = 0; a < D; ++a) means[(size_t)k * D + a] = 6.0 * nd(c) + 0.01 * nd(g);
        mass[k] = ud(g) < 0.33 ? 1e-3 : 10.0 + 1000.0 * ud(g);
      }
      if (check(K, D, means, mass, "clustered")) return 1;
      for (auto& m : mass) m = 50.0;                         // no filler at all
      if (check(K, D, means, mass, "all active")) return 1;
      for (auto& m : mass) m = 0.0;                          // fillers only
      if (check(K, D, means, mass, "all fillers")) return 1;
      for (auto& v : means) v = 1.0;                         // every distance ties at zero, one heavy component
      for (auto& m : mass) m = 2.0;
      mass[0] = 1e6;
      if (check(K, D, means, mass, "all tied")) return 1;
      means[0] = 1e200;                                      // a squared distance beyond float32 (and float64)
      if (check(K, D, means, mass, "huge distance")) return 1;
    }
  // the rejections
  std::vector<double> m(64 * 4, 0.5), w(64, 3.0);
  std::vector<int32_t> o(64);
  int bad = 0;
  bad += mimo_host_block_order(0, 4, m.data(), w.data(), 16, o.data()) != MIMO_E_INVALID;
  bad += mimo_host_block_order(64, 0, m.data(), w.data(), 16, o.data()) != MIMO_E_INVALID;
  bad += mimo_host_block_order(64, 4, m.data(), w.data(), 8, o.data()) != MIMO_E_INVALID;
  bad += mimo_host_block_order(64, 4, nullptr, w.data(), 16, o.data()) != MIMO_E_INVALID;
  bad += mimo_host_block_order(64, 4, m.data(), nullptr, 16, o.data()) != MIMO_E_INVALID;
  bad += mimo_host_block_order(64, 4, m.data(), w.data(), 16, nullptr) != MIMO_E_INVALID;
  bad += mimo_host_block_order(257, 1, m.data(), m.data(), 16, o.data()) != MIMO_E_UNSUPPORTED;
  m[17] = std::nan("");
  bad += mimo_host_block_order(64, 4, m.data(), w.data(), 16, o.data()) != MIMO_E_INVALID;
  m[17] = 0.5; w[3] = INFINITY;
  bad += mimo_host_block_order(64, 4, m.data(), w.data(), 16, o.data()) != MIMO_E_INVALID;
  if (bad) { printf("%d rejections missing\n", bad); return 1; }
  printf("block order ok\n");
  return 0;
}
