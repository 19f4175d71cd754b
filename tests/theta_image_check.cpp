// Every Theta operand image of mimo_theta.h, packed on the CPU and read back through a reader written from the KERNEL side's
// layout comments (mimo_kernels.h KernelArgs::theta and the small-shape kernel, mimo_extra.h narrow / mid, mimo_rowwave.hip
// "Operand image"), not from the placement code.  Built with AddressSanitizer + UBSan by tests/test_theta_image_cpu.py: every
// image lives in a heap block of exactly count() doubles, so a write past the image is a sanitizer error.
#include "../mimo_amd/csrc/mimo_theta.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

using namespace mimo;

static int g_bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_bad; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---- the feature orders, by walking them -------------------------------------------------------------------------------------
struct Order { int D; std::vector<int> pos; int n = 0; int at(int a, int b) const { return pos[(size_t)a * (D + 1) + b]; } };
// row-major upper triangle of z~ = [z, 1]; grouped: every row of the triangle starts on a whole step of 4
static Order full_order(int D, bool grouped = false) {
  Order o{D, std::vector<int>((size_t)(D + 1) * (D + 1), -1)};
  for (int a = 0; a <= D; ++a) {
    for (int b = a; b <= D; ++b) o.pos[(size_t)a * (D + 1) + b] = o.n++;
    if (grouped) o.n = (o.n + 3) / 4 * 4;
  }
  return o;
}
// diagonal structure: z_a^2 at a, z_a at D + a, 1 at 2 D; linear structure: z_a at a, 1 at D
static Order reduced_order(int D, int structure) {
  Order o{D, std::vector<int>((size_t)(D + 1) * (D + 1), -1)};
  for (int a = 0; a < D; ++a) {
    if (structure == MIMO_STRUCT_DIAG) o.pos[(size_t)a * (D + 1) + a] = a;
    o.pos[(size_t)a * (D + 1) + D] = structure == MIMO_STRUCT_DIAG ? D + a : a;
  }
  o.pos[(size_t)D * (D + 1) + D] = structure == MIMO_STRUCT_DIAG ? 2 * D : D;
  o.n = structure == MIMO_STRUCT_DIAG ? 2 * D + 1 : D + 1;
  return o;
}
static Order struct_order(int D, int structure) { return structure == MIMO_STRUCT_FULL ? full_order(D) : reduced_order(D, structure); }

// ---- the readers: offset of Theta[k][feature f] as the kernels address it ---------------------------------------------------------
using Reader = std::function<size_t(int k, int a, int b)>;
// tile kernels: [row block][step][64], A-operand lane 16 (f % 4) + k % 16
static Reader read_generic(Order o, int NS) {
  return [=](int k, int a, int b) { const int f = o.at(a, b); return ((size_t)(k / 16) * NS + f / 4) * 64 + 16 * (f % 4) + k % 16; };
}
// small-shape kernel: [G KL][F] row-major over the full map
static Reader read_small(int D) {
  const Order o = full_order(D);
  return [=](int k, int a, int b) { return (size_t)k * o.n + o.at(a, b); };
}
// narrow kernels: slice s V + c, entry 4 kk + j = Theta[component j V + c][feature 4 s + kk]
static Reader read_narrow(Order o, int V) {
  return [=](int k, int a, int b) { const int f = o.at(a, b), j = k / V, c = k % V; return ((size_t)(f / 4) * V + c) * 16 + 4 * (f % 4) + j; };
}
// slot i of row block rb = component (i & 3) V + 4 rb + (i >> 2), V = 4 KB: found by search
static void owner_slot(int k, int KB, int* rb_out, int* i_out) {
  *rb_out = *i_out = -1;
  for (int rb = 0; rb < KB; ++rb)
    for (int i = 0; i < 16; ++i)
      if ((i & 3) * 4 * KB + 4 * rb + (i >> 2) == k) { *rb_out = rb; *i_out = i; }
}
// mid kernels: slice (s, rb), entry 16 kk + i = Theta[16 rb + i][grouped feature 4 s + kk]; label pass: the permuted slots
static Reader read_mid(int D, int KB, bool labels) {
  const Order o = full_order(D, true);
  return [=](int k, int a, int b) {
    const int g = o.at(a, b);
    int rb = k / 16, i = k % 16;
    if (labels) owner_slot(k, KB, &rb, &i);
    return ((size_t)(g / 4) * KB + rb) * 64 + 16 * (g % 4) + i;
  };
}
// row-owner kernels: slice e = s KB + rb, lane (i = lane & 15, kk = lane >> 4) holds Theta[comp(i, rb)][4 s + kk]
static Reader read_rowowner(Order o, int KB) {
  return [=](int k, int a, int b) {
    const int f = o.at(a, b);
    int rb, i;
    owner_slot(k, KB, &rb, &i);
    return ((size_t)(f / 4) * KB + rb) * 64 + 16 * (f % 4) + i;
  };
}

// ---- inputs: every entry the structure reads is non-zero, and the image values they give are distinct ------------------------------
struct Model { int D, K; std::vector<double> c, b, W; };
static Model make_model(int D, int K, int structure, unsigned seed) {
  Model m{D, K, std::vector<double>(K), std::vector<double>((size_t)K * D), std::vector<double>((size_t)K * D * D, 0.0)};
  unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
  auto next = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return 1.0 + (double)(s >> 24) / (double)(1ull << 40); };   // [1, 2)
  for (auto& v : m.c) v = -next();
  for (auto& v : m.b) v = next() + 2.0;
  for (int k = 0; k < K; ++k)
    for (int a = 0; a < D; ++a)
      for (int bb = 0; bb < D; ++bb)
        if (structure == MIMO_STRUCT_FULL || a == bb) m.W[((size_t)k * D + a) * D + bb] = next() + (a == bb ? 8.0 : 4.0);
  if (structure == MIMO_STRUCT_LINEAR) for (int k = 1; k < K; ++k) std::copy(m.W.begin(), m.W.begin() + D * D, m.W.begin() + (size_t)k * D * D);
  return m;
}
struct Entry { int k, a, b; double v; };
static std::vector<Entry> expected_entries(const Model& m, int structure) {
  std::vector<Entry> e;
  const int D = m.D;
  for (int k = 0; k < m.K; ++k) {
    const double* W = m.W.data() + (size_t)k * D * D;
    e.push_back({k, D, D, m.c[k]});
    for (int a = 0; a < D; ++a) e.push_back({k, a, D, m.b[(size_t)k * D + a]});
    if (structure == MIMO_STRUCT_LINEAR) continue;
    for (int a = 0; a < D; ++a) {
      e.push_back({k, a, a, -0.5 * W[a * D + a]});
      if (structure == MIMO_STRUCT_FULL) for (int bb = a + 1; bb < D; ++bb) e.push_back({k, a, bb, -0.5 * (W[a * D + bb] + W[bb * D + a])});
    }
  }
  std::vector<double> vals;
  for (const Entry& x : e) vals.push_back(x.v);
  std::sort(vals.begin(), vals.end());
  EXPECT(std::adjacent_find(vals.begin(), vals.end()) == vals.end() && std::find(vals.begin(), vals.end(), 0.0) == vals.end(),
         "test inputs: image values not distinct and non-zero");
  return e;
}
static bool same_bits(double x, double y) { return memcmp(&x, &y, sizeof x) == 0; }

// Packs B problems back to back, `tail` doubles behind them (the batched passes' trailing words), into a block of `cap` doubles
// (0: exactly what the images need) and checks the four properties on every slice.
template <typename P>
static void check_image(const char* name, const P& pl, int structure, const Reader& rd, size_t want_count, int want_slots,
                        int B = 1, size_t tail = 0, size_t cap = 0) {
  const size_t per = pl.count();
  EXPECT(per == want_count && pl.slots() == want_slots, "%s: count %zu (want %zu), slots %d (want %d)", name, per, want_count, pl.slots(), want_slots);
  if (per != want_count) return;
  if (!cap) cap = per * B + tail;
  const double sentinel = 12345.678;
  double* img = new double[cap];
  std::fill(img, img + cap, sentinel);
  std::vector<Model> ms;
  for (int p = 0; p < B; ++p) {
    ms.push_back(make_model(pl.D, pl.K, structure, 17 * p + pl.K));
    const ThetaFail f = pack_theta(pl, structure, ms[p].c.data(), ms[p].b.data(), ms[p].W.data(), img + per * p);
    EXPECT(f.kind == ThetaFail::kNone, "%s: problem %d refused (kind %d)", name, p, (int)f.kind);
  }
  for (int p = 0; p < B; ++p) {
    const double* ip = img + per * p;
    const std::vector<Entry> e = expected_entries(ms[p], structure);
    for (const Entry& x : e) {
      const size_t off = rd(x.k, x.a, x.b);
      EXPECT(off < per && same_bits(ip[off], x.v), "%s: problem %d entry (k=%d, %d,%d) at %zu", name, p, x.k, x.a, x.b, off);
    }
    for (int k = pl.K; k < want_slots; ++k) {
      const size_t off = rd(k, pl.D, pl.D);
      EXPECT(off < per && same_bits(ip[off], kPadLogDensity), "%s: problem %d padding slot %d at %zu", name, p, k, off);
    }
    const size_t nz = per - (size_t)std::count(ip, ip + per, 0.0);
    EXPECT(nz == e.size() + (size_t)(want_slots - pl.K), "%s: problem %d: %zu non-zero elements, %zu entries + %d padding slots", name, p, nz,
           e.size(), want_slots - pl.K);
  }
  EXPECT(std::count(img + per * B, img + cap, sentinel) == (long)(cap - per * B), "%s: wrote behind the images", name);
  delete[] img;
}

// ---- refused inputs: kind and indices, and nothing past count() touched (the block is exactly count() doubles) -----------------
template <typename P>
static void check_failures(const char* name, const std::function<P(int structure)>& make, const Reader& rd) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  auto run = [&](int structure, const std::function<void(Model&)>& spoil, double** keep = nullptr) {
    const P pl = make(structure);
    Model m = make_model(pl.D, pl.K, structure, 99);
    spoil(m);
    double* img = new double[pl.count()];
    const ThetaFail f = pack_theta(pl, structure, m.c.data(), m.b.data(), m.W.data(), img);
    if (keep) *keep = img; else delete[] img;
    return f;
  };
  const P full = make(MIMO_STRUCT_FULL);
  const int D = full.D, DD = D * D;
  ThetaFail f = run(MIMO_STRUCT_FULL, [&](Model& m) { m.c[1] = nan; });
  EXPECT(f.kind == ThetaFail::kBadC && f.k == 1, "%s: c[1] = NaN -> kind %d, k %d", name, (int)f.kind, f.k);
  f = run(MIMO_STRUCT_FULL, [&](Model& m) { m.c[1] = inf; });
  EXPECT(f.kind == ThetaFail::kBadC && f.k == 1, "%s: c[1] = +inf -> kind %d, k %d", name, (int)f.kind, f.k);
  double* img = nullptr;
  f = run(MIMO_STRUCT_FULL, [&](Model& m) { m.c[1] = -inf; }, &img);
  EXPECT(f.kind == ThetaFail::kNone && same_bits(img[rd(1, D, D)], kPadLogDensity), "%s: c[1] = -inf -> kind %d", name, (int)f.kind);
  delete[] img;
  f = run(MIMO_STRUCT_FULL, [&](Model& m) { m.b[(size_t)2 * D + 1] = nan; });
  EXPECT(f.kind == ThetaFail::kNonFinite, "%s: NaN in b -> kind %d", name, (int)f.kind);
  f = run(MIMO_STRUCT_FULL, [&](Model& m) { m.W[(size_t)2 * DD + 1] = inf; });
  EXPECT(f.kind == ThetaFail::kNonFinite, "%s: inf in W -> kind %d", name, (int)f.kind);
  f = run(MIMO_STRUCT_LINEAR, [&](Model& m) { m.W[(size_t)2 * DD + D + 1] += 1.0; });
  EXPECT(f.kind == ThetaFail::kLinearW && f.k == 2, "%s: linear, W[2] != W[0] -> kind %d, k %d", name, (int)f.kind, f.k);
  f = run(MIMO_STRUCT_DIAG, [&](Model& m) { m.W[(size_t)1 * DD + 0 * D + 2] = 0.5; });
  EXPECT(f.kind == ThetaFail::kDiagOffDiag && f.k == 1 && f.a == 0 && f.b == 2, "%s: diagonal, W[1][0][2] != 0 -> kind %d, (%d; %d,%d)", name,
         (int)f.kind, f.k, f.a, f.b);
}

int main() {
  const int FULL = MIMO_STRUCT_FULL, DIAG = MIMO_STRUCT_DIAG, LIN = MIMO_STRUCT_LINEAR;
  // generic tile image: four row blocks streamed for K <= 64 (sixteen beyond), NS = F16 / 4 or whole chunks of the two-stage path
  check_image("generic D=2 K=5", ThetaGeneric{2, 5, FULL, 4, 4}, FULL, read_generic(struct_order(2, FULL), 4), 4 * 4 * 64, 16);
  check_image("generic D=16 K=17 diagonal", ThetaGeneric{16, 17, DIAG, 4, 12}, DIAG, read_generic(struct_order(16, DIAG), 12), 4 * 12 * 64, 32);
  check_image("generic D=3 K=2 linear", ThetaGeneric{3, 2, LIN, 4, 4}, LIN, read_generic(struct_order(3, LIN), 4), 4 * 4 * 64, 16);
  EXPECT(chunked_ns_pad(16) == 72, "chunked_ns_pad(16) = %d", chunked_ns_pad(16));
  check_image("generic D=2 K=65 two-stage", ThetaGeneric{2, 65, FULL, 16, chunked_ns_pad(16)}, FULL, read_generic(struct_order(2, FULL), 72), 16 * 72 * 64, 80);
  // batched: K16 row blocks per problem, the problems back to back, two trailing words
  check_image("batched B=3 D=2 K=17", ThetaGeneric{2, 17, FULL, 2, 4}, FULL, read_generic(struct_order(2, FULL), 4), 2 * 4 * 64, 32, 3, 2);
  // small: into the 40 doubles of KernelArgs::theta_inline, and the staged form
  check_image("small D=2 Kp=4 inline", ThetaSmall{2, 3, 4}, FULL, read_small(2), 4 * 6, 4, 1, 0, kThetaInline);
  check_image("small D=4 Kp=16", ThetaSmall{4, 13, 16}, FULL, read_small(4), 16 * 15, 16);
  check_image("small D=4 Kp=16 diagonal", ThetaSmall{4, 13, 16}, DIAG, read_small(4), 16 * 15, 16);
  // narrow: plain over the structure's map, grouped over the padded rows of the triangle
  check_image("narrow D=2 K=50", ThetaNarrow{2, 50, FULL, 13, 2, nullptr}, FULL, read_narrow(struct_order(2, FULL), 13), 2 * 13 * 16, 52);
  check_image("narrow D=8 K=20 diagonal", ThetaNarrow{8, 20, DIAG, 6, 5, nullptr}, DIAG, read_narrow(struct_order(8, DIAG), 6), 5 * 6 * 16, 24);
  const int grouped_dkv[2][3] = {{5, 4, 1}, {6, 9, 3}};
  for (const auto& dkv : grouped_dkv) {
    const int D = dkv[0], K = dkv[1], V = dkv[2];
    const Order g = full_order(D, true);
    const ThetaGroupedOrder order(D);
    check_image("narrow grouped", ThetaNarrow{D, K, FULL, V, g.n / 4, &order}, FULL, read_narrow(g, V), (size_t)(g.n / 4) * V * 16, 4 * V);
  }
  {   // mid, D = 9, K = 17: two row blocks, sixteen zero slices behind the image
    const int D = 9, K = 17, KB = 2, pf = 16, NS = full_order(D, true).n / 4;
    const ThetaGroupedOrder order(D);
    check_image("mid D=9 K=17", ThetaMid{D, K, KB, NS, pf, false, &order}, FULL, read_mid(D, KB, false), ((size_t)NS * KB + pf) * 64, 32);
    check_image("mid labels D=9 K=17", ThetaMid{D, K, KB, NS, pf, true, &order}, FULL, read_mid(D, KB, true), ((size_t)NS * KB + pf) * 64, 32);
    EXPECT(read_mid(D, KB, true)(16, D, D) != read_mid(D, KB, false)(16, D, D), "mid labels: component 16 is not permuted");
  }
  // row-owner: resident (NS = F16 / 4) and streamed (NS padded to whole chunks)
  check_image("row-owner KB=1 K=5", ThetaRowOwner{2, 5, FULL, 1, 4}, FULL, read_rowowner(struct_order(2, FULL), 1), 4 * 1 * 64, 16);
  check_image("row-owner KB=2 K=20", ThetaRowOwner{2, 20, FULL, 2, 7}, FULL, read_rowowner(struct_order(2, FULL), 2), 7 * 2 * 64, 32);
  check_image("row-owner KB=2 K=20 diagonal", ThetaRowOwner{3, 20, DIAG, 2, 4}, DIAG, read_rowowner(struct_order(3, DIAG), 2), 4 * 2 * 64, 32);

  check_failures<ThetaGeneric>("generic", [](int st) { return ThetaGeneric{3, 4, st, 4, 4}; }, read_generic(struct_order(3, FULL), 4));
  check_failures<ThetaNarrow>("narrow", [](int st) { return ThetaNarrow{3, 20, st, 6, 3, nullptr}; }, read_narrow(struct_order(3, FULL), 6));

  if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
  printf("theta images ok\n");
  return 0;
}
