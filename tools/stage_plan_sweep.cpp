// Every sub-kernel decision below the family level, as text: what label_stats_plan and two_stage_plan answer over
// structure 0 .. 2 x Dz 1 .. 32 x N in {0, 1, 2^17 - 1, 2^17, 1e7} x K 1 .. 256, one line per maximal run of K with equal answers.
// Host only (no HIP call, no GPU needed).  Two builds of the library decide alike exactly when their outputs are identical
// (profiles/stage_plan_equivalence.txt compares this tree with its parent that way).  From the repository root, after the library is built:
//   hipcc -std=c++17 -Imimo_amd/csrc tools/stage_plan_sweep.cpp -Lmimo_amd -lmimo_hip -Wl,-rpath,$PWD/mimo_amd -o tools/stage_plan_sweep
//   tools/stage_plan_sweep | sha256sum
// Per line:  ls: covered, kind (- none, P per component, S slots, W windows, R ranked tiles), launches, ranked-tile buffers (0 none,
// 1 used when present, 2 required), grid at 8 and 256 CUs | ts, for the softmax pass (vi), the label pass (gibbs) and the statistics of
// a caller's table (W) / labels (L): E-step (- none, c chunked, w wide), statistics (- none, l label, w wide columns, f fused columns), gmax.
#include "mimo_route.h"

#include <cstdio>
#include <cstring>
#include <string>
using namespace mimo;

int main() {
  const int64_t Ns[] = {0, 1, (1 << 17) - 1, 1 << 17, 10000000};
  Route two_stage;
  two_stage.family = Family::TwoStage;
  for (int st = 0; st < 3; ++st)
    for (int D = 1; D <= 32; ++D)
      for (int64_t N : Ns) {
        std::string prev;
        int k0 = 1;
        for (int K = 1; K <= 257; ++K) {
          char line[256] = "";
          if (K <= 256) {
            KernelArgs a;
            memset(&a, 0, sizeof a);
            const int F = st == 1 ? diag_feat_count(D) : st == 2 ? lin_feat_count(D) : feat_count(D);
            a.K = K; a.D = D; a.N = N; a.diag = st != 0; a.K16 = (K + 15) / 16; a.F16 = (F + 15) / 16 * 16; a.do_stats = 1;
            const LabelStatsPlan lp = label_stats_plan(K, D, st, N);
            int n = snprintf(line, sizeof line, "ls cov=%d kind=%c launches=%d ranked=%d grid8=%d grid256=%d | ts", (int)label_stats_covers(K, D, st),
                             "-PSWR"[lp.kind], lp.launches, lp.ranked, label_stats_grid(lp, N, 8), label_stats_grid(lp, N, 256));
            const struct { const char* name; int src, gibbs; } passes[4] = {{"vi", kSrcEstep, 0}, {"gibbs", kSrcEstep, 1}, {"W", kSrcWeights, 0}, {"L", kSrcLabels, 0}};
            for (const auto& q : passes) {
              a.gibbs = q.gibbs;
              const TwoStagePlan ts = two_stage_plan(two_stage, a, st, q.src);
              n += snprintf(line + n, sizeof line - n, " %s=%c%c%d", q.name, "-cw"[ts.estep], "-lwf"[ts.stats], ts.gmax);
            }
          }
          if (prev != line) {
            if (!prev.empty()) printf("st=%d D=%d N=%lld K=%d..%d %s\n", st, D, (long long)N, k0, K - 1, prev.c_str());
            prev = line; k0 = K;
          }
        }
      }
  return 0;
}
