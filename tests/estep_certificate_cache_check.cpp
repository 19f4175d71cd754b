// The two-part form of mimo_host_estep_certificate (mimo_host_estep_certificate_ref once per reference, then
// mimo_host_estep_certificate_cur per pass) against the public one-part function, under AddressSanitizer + UBSan: built together with
// mimo_amd/csrc/mimo_host.cpp as a stand-alone host program (tests/test_estep_certificate_cache_cpu.py).  On the same inputs the two
// forms must leave the same bytes in `out` and `table` and return the same code, refusals included.  Every array sits in a heap
// block of exactly its length.
#include "../include/mimo_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

struct Params { std::vector<double> c, b, W; };

// K random SPD precisions (A A' / D + I / 2), linear terms and offsets; every seventh component sits far under the others
static Params reference(std::mt19937_64& g, int K, int D) {
  std::normal_distribution<double> nd;
  Params p;
  p.c.assign((size_t)K, 0.0); p.b.assign((size_t)K * D, 0.0); p.W.assign((size_t)K * D * D, 0.0);
  for (int k = 0; k < K; ++k) {
    std::vector<double> A((size_t)D * D);
    for (auto& v : A) v = nd(g);
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        double s = i == j ? 0.5 : 0.0;
        for (int r = 0; r < D; ++r) s += A[(size_t)i * D + r] * A[(size_t)j * D + r] / D;
        p.W[((size_t)k * D + i) * D + j] = s;
      }
    for (int i = 0; i < D; ++i) p.b[(size_t)k * D + i] = 3.0 * nd(g);
    p.c[k] = k % 7 == 0 ? -800.0 : -20.0 + nd(g);
  }
  return p;
}

// the reference moved by `move`: W (1 + move) + move (a fresh SPD matrix), b and c by move sigma.  Component 0 keeps W0 to the bit;
// component 1 (where there is one) takes 100 W0, past the grid: no upper eigenvalue bound, gamma = -1e300, delta = 0.
static Params moved(std::mt19937_64& g, const Params& r, int K, int D, double move) {
  std::normal_distribution<double> nd;
  const Params f = reference(g, K, D);
  Params p = r;
  for (int k = 0; k < K; ++k) {
    for (size_t e = 0; e < (size_t)D * D; ++e) {
      const size_t i = (size_t)k * D * D + e;
      p.W[i] = k == 0 ? r.W[i] : k == 1 ? 100.0 * r.W[i] : r.W[i] * (1.0 + move) + move * f.W[i];
    }
    for (int i = 0; i < D; ++i) p.b[(size_t)k * D + i] += move * nd(g);
    p.c[k] += move * nd(g);
  }
  return p;
}

static int fails = 0;

// both forms on (r, p); `ref` is the caller's block, which may hold an earlier reference's leftovers (rebuild) or this reference's
// block from an earlier call (reuse)
static void compare(const char* what, int K, int D, const Params& r, const Params& p, std::vector<double>& ref, bool rebuild, bool with_table, int want) {
  std::vector<double> out((size_t)5 * K + 4, -7.0), table((size_t)4 + 2 * K, -7.0), out2(out), table2(table);
  const int rc = mimo_host_estep_certificate(K, D, r.c.data(), r.b.data(), r.W.data(), p.c.data(), p.b.data(), p.W.data(), -41.6, out.data(),
                                             with_table ? table.data() : nullptr);
  if (rebuild) {
    const int rr = mimo_host_estep_certificate_ref(K, D, r.c.data(), r.b.data(), r.W.data(), ref.data());
    if (rr != MIMO_OK && rr != MIMO_E_INVALID) { printf("%s K=%d D=%d: the reference part returns %d\n", what, K, D, rr); ++fails; return; }
  }
  const int rc2 = mimo_host_estep_certificate_cur(K, D, ref.data(), p.c.data(), p.b.data(), p.W.data(), -41.6, out2.data(), with_table ? table2.data() : nullptr);
  if (rc != want || rc2 != rc || memcmp(out.data(), out2.data(), out.size() * sizeof(double)) || memcmp(table.data(), table2.data(), table.size() * sizeof(double))) {
    printf("%s K=%d D=%d: one part returns %d (expected %d), two parts %d; out %s, table %s\n", what, K, D, rc, want, rc2,
           memcmp(out.data(), out2.data(), out.size() * sizeof(double)) ? "differs" : "equal",
           memcmp(table.data(), table2.data(), table.size() * sizeof(double)) ? "differs" : "equal");
    ++fails;
  }
  if (rc == MIMO_OK && with_table && K >= 2 && !(table[4 + 1] == -1e300 && table[4 + K + 1] == 0.0)) {
    printf("%s K=%d D=%d: component 1 at 100 W0 has an upper bound (gamma %g, delta %g)\n", what, K, D, table[4 + 1], table[4 + K + 1]);
    ++fails;
  }
  if (rc == MIMO_OK && !(out[2 * (size_t)K] == 1.0 && out[3 * (size_t)K] == 1.0)) {
    printf("%s K=%d D=%d: component 0 at W0 to the bit: rho %g, rho_bar %g\n", what, K, D, out[2 * (size_t)K], out[3 * (size_t)K]);
    ++fails;
  }
}

int main() {
  for (int K : {1, 3, 4, 5, 49, 64})
    for (int D : {1, 14, 16, 32}) {
      std::mt19937_64 g((unsigned)(K * 131 + D));
      const size_t len = mimo_host_estep_certificate_ref_size(K, D);
      if (!len) { printf("K=%d D=%d: no block size\n", K, D); return 1; }
      std::vector<double> ref(len, std::nan(""));
      const Params r = reference(g, K, D);
      // one reference block, three current posteriors (small, large, small move); the last one without the table
      compare("small move", K, D, r, moved(g, r, K, D, 0.01), ref, true, true, MIMO_OK);
      compare("large move, block reused", K, D, r, moved(g, r, K, D, 5.0), ref, false, true, MIMO_OK);
      compare("small move, block reused, no table", K, D, r, moved(g, r, K, D, 0.02), ref, false, false, MIMO_OK);
      // a current W that is not positive definite, in the last group: both refuse, after the same groups
      Params bad = moved(g, r, K, D, 0.01);
      bad.W[(size_t)(K - 1) * D * D] = -1.0;
      compare("W not positive definite", K, D, r, bad, ref, false, true, MIMO_E_INVALID);
      bad = moved(g, r, K, D, 0.01);
      bad.b[(size_t)K * D - 1] = std::nan("");
      compare("NaN in b", K, D, r, bad, ref, false, true, MIMO_E_INVALID);
      // a second reference in the same buffer: nothing of the first may be left
      const Params r2 = reference(g, K, D);
      compare("second reference, same buffer", K, D, r2, moved(g, r2, K, D, 0.3), ref, true, true, MIMO_OK);
      // a reference that is refused, then a good one again in the same buffer
      Params r3 = r2;
      r3.W[(size_t)(K / 2) * D * D] = -1.0;
      compare("W0 not positive definite", K, D, r3, moved(g, r2, K, D, 0.01), ref, true, true, MIMO_E_INVALID);
      r3 = r2;
      r3.c[K - 1] = INFINITY;
      compare("infinite c0", K, D, r3, moved(g, r2, K, D, 0.01), ref, true, true, MIMO_E_INVALID);
      compare("first reference again", K, D, r, moved(g, r, K, D, 0.05), ref, true, true, MIMO_OK);
    }
  // the rejections of the two parts themselves
  {
    const int K = 8, D = 4;
    std::mt19937_64 g(3);
    const Params r = reference(g, K, D), p = moved(g, r, K, D, 0.01);
    std::vector<double> ref(mimo_host_estep_certificate_ref_size(K, D)), out((size_t)5 * K + 4), table((size_t)4 + 2 * K);
    int bad = 0;
    bad += mimo_host_estep_certificate_ref_size(0, D) != 0 || mimo_host_estep_certificate_ref_size(K, 33) != 0 || mimo_host_estep_certificate_ref_size(257, D) != 0;
    bad += mimo_host_estep_certificate_ref(K, D, nullptr, r.b.data(), r.W.data(), ref.data()) != MIMO_E_INVALID;
    bad += mimo_host_estep_certificate_ref(K, D, r.c.data(), r.b.data(), r.W.data(), nullptr) != MIMO_E_INVALID;
    bad += mimo_host_estep_certificate_ref(257, 1, r.c.data(), r.b.data(), r.W.data(), ref.data()) != MIMO_E_UNSUPPORTED;
    bad += mimo_host_estep_certificate_ref(K, D, r.c.data(), r.b.data(), r.W.data(), ref.data()) != MIMO_OK;
    bad += mimo_host_estep_certificate_cur(K, D, nullptr, p.c.data(), p.b.data(), p.W.data(), -41.6, out.data(), table.data()) != MIMO_E_INVALID;
    bad += mimo_host_estep_certificate_cur(K, D, ref.data(), p.c.data(), p.b.data(), p.W.data(), -41.6, nullptr, table.data()) != MIMO_E_INVALID;
    bad += mimo_host_estep_certificate_cur(K - 4, D, ref.data(), p.c.data(), p.b.data(), p.W.data(), -41.6, out.data(), table.data()) != MIMO_E_INVALID;   // another K's block
    bad += mimo_host_estep_certificate_cur(K, D, ref.data(), p.c.data(), p.b.data(), p.W.data(), -41.6, out.data(), table.data()) != MIMO_OK;
    if (bad) { printf("%d rejections wrong\n", bad); return 1; }
  }
  if (fails) { printf("%d comparisons failed\n", fails); return 1; }
  printf("estep certificate cache ok\n");
  return 0;
}
