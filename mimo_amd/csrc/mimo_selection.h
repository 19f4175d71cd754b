// The work table of a batch and the small tables of a row selection (mimo_estep_batched_rows, the SVI loop), as the batched pass
// reads them.  Host only: needs the HIP headers (mimo_batched.h) but makes no HIP call and has no context —
// tests/selection_tables_check.cpp drives it on the CPU.  The rule for the tiles of one workgroup is an argument
// (batched_tiles_per_wg of mimo_batched.hip in the library).
#pragma once
#include "mimo_batched.h"
#include "mimo_kernels.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace mimo {

// The work table of B problems with the rows [off[b], off[b + 1]): problem b's tiles in runs of tiles_per_wg(N_b), a function of
// N_b alone; problem b owns the workgroups [wg_off[b], wg_off[b + 1]).  wg_off gets B + 2 entries (whole uint64 words for the
// caller that stages it behind an operand image).  False: more workgroups than an int32 counts.
inline bool build_work_table(const int64_t* off, int B, int (*tiles_per_wg)(int64_t), std::vector<BatchedWork>* work,
                             std::vector<int32_t>* wg_off) {
  work->clear();
  *wg_off = std::vector<int32_t>((size_t)B + 2, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t nb = off[b + 1] - off[b];
    const int64_t tiles = (nb + kTile - 1) / kTile;
    const int tpw = tiles_per_wg(nb);
    for (int64_t t = 0; t < tiles; t += tpw)
      work->push_back(BatchedWork{b, (int32_t)t, (int32_t)std::min<int64_t>(tpw, tiles - t), 0});
    if (work->size() > (size_t)INT32_MAX) return false;
    (*wg_off)[(size_t)b + 1] = (int32_t)work->size();
  }
  return true;
}

// A selection's small tables, one block of uint64 words:
//   [sel_off (B + 1) | work table (2 words per workgroup) | wg_off (int32, B + 1, in whole words) | seeds B | 1 / scale B]
// The last two only with `scale` (the SVI loop; the seeds are zeros without `seeds`).  at_*: the word where each part starts
// (at_seeds = at_inv = the end without `scale`); G workgroups.
struct SelectionTables {
  std::vector<uint64_t> words;
  size_t at_work = 0, at_wg = 0, at_seeds = 0, at_inv = 0, G = 0;

  // sel_off[0 .. B] starts at 0 and never decreases (the caller checks).  False: build_work_table refused.
  bool build(const int64_t* sel_off, int B, int (*tiles_per_wg)(int64_t), const uint64_t* seeds = nullptr,
             const double* scale = nullptr) {
    static_assert(sizeof(BatchedWork) == 2 * sizeof(uint64_t), "a work table entry is two words of the block");
    std::vector<BatchedWork> work;
    std::vector<int32_t> wg_off;
    if (!build_work_table(sel_off, B, tiles_per_wg, &work, &wg_off)) return false;
    const size_t nb = (size_t)B, nwg = (nb + 2) / 2;
    G = work.size();
    at_work = nb + 1;
    at_wg = at_work + 2 * G;
    at_seeds = at_wg + nwg;
    at_inv = at_seeds + (scale ? nb : 0);
    words.assign(at_inv + (scale ? nb : 0), 0);
    memcpy(words.data(), sel_off, (nb + 1) * sizeof(int64_t));
    if (G) memcpy(words.data() + at_work, work.data(), G * sizeof(BatchedWork));
    memcpy(words.data() + at_wg, wg_off.data(), nwg * sizeof(uint64_t));
    if (scale && seeds) memcpy(words.data() + at_seeds, seeds, nb * sizeof(uint64_t));
    for (size_t p = 0; scale && p < nb; ++p) {
      const double inv = 1.0 / scale[p];      // (as `1. / scale` of the host step rounds it)
      memcpy(words.data() + at_inv + p, &inv, sizeof(double));
    }
    return true;
  }
};

// The first index of `n_sel` selections that lies outside its problem's rows: selection s holds sel_off[B] indices at
// rows + s sel_off[B], those of problem p at [sel_off[p], sel_off[p + 1]), each to lie in [0, N_p), N_p = row_off[p + 1] -
// row_off[p].  The kernel gathers through the indices unchecked.
struct SelectionBad { int sel, prob; int64_t index, entry, rows; };
inline bool selection_indices_ok(const int64_t* rows, int n_sel, const int64_t* sel_off, const int64_t* row_off, int B,
                                 SelectionBad* bad) {
  for (int p = 0; p < B; ++p) {
    const int64_t nb = row_off[p + 1] - row_off[p];
    for (int s = 0; s < n_sel; ++s)
      for (int64_t i = sel_off[p]; i < sel_off[p + 1]; ++i) {
        const int64_t r = rows[(int64_t)s * sel_off[B] + i];
        if (r < 0 || r >= nb) {
          *bad = SelectionBad{s, p, r, i - sel_off[p], nb};
          return false;
        }
      }
  }
  return true;
}

}  // namespace mimo
