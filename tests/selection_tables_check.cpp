// The small tables of a row selection (SelectionTables, mimo_selection.h) and the index check in front of them, on the CPU: the
// words as mimo_estep_batched_rows and the SVI loop stage them for the batched pass — [sel_off | work table | wg_off | seeds |
// 1 / scale] — written out by hand for the small cases.  Built with AddressSanitizer + UBSan by tests/test_selection_tables_cpu.py.
#include "../mimo_amd/csrc/mimo_selection.h"

#include <cstdio>
#include <vector>

using namespace mimo;

static int g_bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_bad; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the library's rule for a problem of at most 128 * 4 tiles (batched_tiles_per_wg): runs of four 32-row tiles, 128 rows
static int four_tiles(int64_t) { return 4; }

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, sizeof u); return u; }
// a work table entry's two words: (prob, tile0), (ntiles, pad = 0); two int32 of wg_off in one word
static uint64_t lo_hi(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

struct Case {
  const char* name;
  std::vector<int64_t> sel_off;
  std::vector<uint64_t> seeds;
  std::vector<double> scale;
  std::vector<uint64_t> want;
  size_t at_work, at_wg, at_seeds, at_inv, G;
};

static void run(const Case& c) {
  const int B = (int)c.sel_off.size() - 1;
  SelectionTables t;
  const bool ok = t.build(c.sel_off.data(), B, four_tiles, c.seeds.empty() ? nullptr : c.seeds.data(),
                          c.scale.empty() ? nullptr : c.scale.data());
  EXPECT(ok, "%s: build refused", c.name);
  EXPECT(t.G == c.G && t.at_work == c.at_work && t.at_wg == c.at_wg && t.at_seeds == c.at_seeds && t.at_inv == c.at_inv,
         "%s: G %zu at_work %zu at_wg %zu at_seeds %zu at_inv %zu", c.name, t.G, t.at_work, t.at_wg, t.at_seeds, t.at_inv);
  EXPECT(t.words.size() == c.want.size(), "%s: %zu words, want %zu", c.name, t.words.size(), c.want.size());
  for (size_t i = 0; i < t.words.size() && i < c.want.size(); ++i)
    EXPECT(t.words[i] == c.want[i], "%s: word %zu = 0x%llx, want 0x%llx", c.name, i, (unsigned long long)t.words[i],
           (unsigned long long)c.want[i]);
  // the words in a heap block of exactly their count, read as the device reads them: a part past the end is a sanitizer error
  std::vector<uint64_t> dev(t.words);
  const int32_t* wg = reinterpret_cast<const int32_t*>(dev.data() + t.at_wg);
  const BatchedWork* work = reinterpret_cast<const BatchedWork*>(dev.data() + t.at_work);
  EXPECT(wg[0] == 0 && (size_t)wg[B] == t.G, "%s: wg_off runs 0 .. %d, G = %zu", c.name, wg[B], t.G);
  for (int b = 0; b < B; ++b)
    for (int g = wg[b]; g < wg[b + 1]; ++g) {
      const int64_t tiles = (c.sel_off[b + 1] - c.sel_off[b] + 31) / 32;
      EXPECT(work[g].prob == b && work[g].tile0 == 4 * (g - wg[b]) && work[g].ntiles >= 1 && work[g].tile0 + work[g].ntiles <= tiles &&
             work[g].pad == 0, "%s: workgroup %d = (%d, %d, %d)", c.name, g, work[g].prob, work[g].tile0, work[g].ntiles);
    }
}

int main() {
  const std::vector<Case> cases = {
      // B = 1: wg_off (B + 1 = 2 int32) fills one word
      {"B=1", {0, 5}, {}, {}, {0, 5, lo_hi(0, 0), lo_hi(1, 0), lo_hi(0, 1)}, 2, 4, 5, 5, 1},
      // B = 2: wg_off (3 int32) takes two words, the last half zero; problem 0 selects nothing, problem 1 one run and one row more
      {"B=2, empty + 129", {0, 0, 129}, {}, {},
       {0, 0, 129, lo_hi(1, 0), lo_hi(4, 0), lo_hi(1, 4), lo_hi(1, 0), lo_hi(0, 0), lo_hi(2, 0)}, 3, 7, 9, 9, 2},
      // exactly one run of four tiles
      {"B=2, 128 + 1", {0, 128, 129}, {}, {},
       {0, 128, 129, lo_hi(0, 0), lo_hi(4, 0), lo_hi(1, 0), lo_hi(1, 0), lo_hi(0, 1), lo_hi(2, 0)}, 3, 7, 9, 9, 2},
      // every selection empty: no work table at all
      {"B=2, all empty", {0, 0, 0}, {}, {}, {0, 0, 0, lo_hi(0, 0), lo_hi(0, 0)}, 3, 3, 5, 5, 0},
      {"B=3, all empty, scale", {0, 0, 0, 0}, {}, {1.0, 2.0, 0.5},
       {0, 0, 0, 0, lo_hi(0, 0), lo_hi(0, 0), 0, 0, 0, bits(1.0), bits(0.5), bits(2.0)}, 4, 4, 6, 9, 0},
      // the SVI loop's tail: the seeds (zeros without them) and 1 / scale as a double division rounds it
      {"B=1, seeds + scale", {0, 5}, {7}, {0.25}, {0, 5, lo_hi(0, 0), lo_hi(1, 0), lo_hi(0, 1), 7, bits(4.0)}, 2, 4, 5, 6, 1},
      {"B=2, scale alone", {0, 0, 129}, {}, {0.5, 3.0},
       {0, 0, 129, lo_hi(1, 0), lo_hi(4, 0), lo_hi(1, 4), lo_hi(1, 0), lo_hi(0, 0), lo_hi(2, 0), 0, 0, bits(2.0), bits(1.0 / 3.0)},
       3, 7, 9, 11, 2},
      {"B=2, seeds + scale", {0, 1, 2}, {0xffffffffffffffffull, 3}, {0.5, 0.125},
       {0, 1, 2, lo_hi(0, 0), lo_hi(1, 0), lo_hi(1, 0), lo_hi(1, 0), lo_hi(0, 1), lo_hi(2, 0), 0xffffffffffffffffull, 3, bits(2.0),
        bits(8.0)}, 3, 7, 9, 11, 2},
  };
  for (const Case& c : cases) run(c);

  // the index check: two selections over problems of 10 and 7 rows, two slots each
  const int64_t row_off[3] = {0, 10, 17}, sel_off[3] = {0, 2, 4};
  const std::vector<int64_t> good = {0, 9, 0, 6, 9, 0, 6, 0};
  SelectionBad bad{};
  EXPECT(selection_indices_ok(good.data(), 2, sel_off, row_off, 2, &bad), "0 and N_b - 1 refused");
  EXPECT(selection_indices_ok(good.data(), 0, sel_off, row_off, 2, &bad), "no selection refused");
  struct { size_t at; int64_t value; int sel, prob; int64_t entry, rows; } const wrong[] = {
      {0, -1, 0, 0, 0, 10}, {1, 10, 0, 0, 1, 10}, {3, 7, 0, 1, 1, 7}, {6, -1, 1, 1, 0, 7}, {5, 10, 1, 0, 1, 10}};
  for (const auto& w : wrong) {
    std::vector<int64_t> rows(good);
    rows[w.at] = w.value;
    bad = SelectionBad{};
    EXPECT(!selection_indices_ok(rows.data(), 2, sel_off, row_off, 2, &bad), "index %lld at %zu accepted", (long long)w.value, w.at);
    EXPECT(bad.sel == w.sel && bad.prob == w.prob && bad.index == w.value && bad.entry == w.entry && bad.rows == w.rows,
           "index %lld at %zu: reported (%d, %d, %lld, %lld, %lld)", (long long)w.value, w.at, bad.sel, bad.prob, (long long)bad.index,
           (long long)bad.entry, (long long)bad.rows);
    // one selection: the second is not read
    if (w.sel == 1) EXPECT(selection_indices_ok(rows.data(), 1, sel_off, row_off, 2, &bad), "the second selection was read");
  }
  if (g_bad) { printf("%d failures\n", g_bad); return 1; }
  printf("selection tables ok\n");
  return 0;
}
