// (c, b, W) -> the Theta operand image a kernel family reads.  Host only: needs the HIP headers (mimo_kernels.h, mimo_extra.h)
// but makes no HIP call and has no context — tests/theta_image_check.cpp drives it on the CPU.  Three parts: ONE enumerator
// (theta_entries) that walks a problem's components, applies the structure rules and hands every real entry (k, a, b, value) to
// a callable; one PLACEMENT per image, a small value that knows the image's element count, its padded component slots and the
// offset of entry (k, a, b); and pack_theta, which runs the first through the second.  A new kernel family adds a placement and
// nothing else.
//   entries over z~ = [z, 1]: (D,D): c_k ; (a,D): b_k[a] ; (a,a): -W_aa/2 ; (a,b), a<b: -(W_ab + W_ba)/2
#pragma once
#include "../../include/mimo_hip.h"
#include "mimo_kernels.h"
#include "mimo_extra.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace mimo {

struct ThetaFail {             // why a parameter block was refused; the caller owns the wording
  enum Kind { kNone = 0, kBadC, kLinearW, kDiagOffDiag, kNonFinite } kind = kNone;
  int k = 0, a = 0, b = 0;     // kBadC, kLinearW: component k; kDiagOffDiag: entry (a, b) of W[k]
};

constexpr double kThetaMax = std::numeric_limits<double>::max();
inline bool theta_finite(double v) { return std::fabs(v) <= kThetaMax; }

// feature of the pair (a, b), a <= b <= D, in the map of the structure; -1: not in the map
inline int struct_feat_index(int structure, int D, int a, int b) {
  if (structure == MIMO_STRUCT_DIAG) return (a == b || b == D) ? diag_feat_index(D, a, b) : -1;
  if (structure == MIMO_STRUCT_LINEAR) return b == D ? a : -1;
  return feat_index(D, a, b);
}

// The entries of one problem's K components, in component order, as put(k, a, b, value).  Structure rules (mimo_set_structure):
// linear: no W entry, and every W[k] is bytewise W[0] (the common quadratic term stays with the caller); diagonal: W_aa only, and
// an off-diagonal entry must be exactly zero; full: every entry.  A bad c[k] or a structure violation stops at that k; a NaN or
// an infinity in b or W is reported once, behind the last component.
template <typename Put>
inline ThetaFail theta_entries(int D, int K, int structure, const double* c, const double* b, const double* W, Put&& put) {
  bool finite = true;
  auto chk = [&finite](double v) { finite = finite && theta_finite(v); return v; };
  for (int k = 0; k < K; ++k) {
    const double* bk = b + (size_t)k * D;
    const double* Wk = W + (size_t)k * D * D;
    if (c[k] != c[k] || c[k] > kThetaMax) return {ThetaFail::kBadC, k};      // NaN or +inf
    // a component switched off by its weight (log 0 = -inf in c_k, gmm.py:84 of the host mirror) enters like a
    // padding component: l = -1e300 for every datum, r = 0 — an infinite operand would turn the zero features of the
    // rows past N into NaN statistics
    put(k, D, D, c[k] < kPadLogDensity ? kPadLogDensity : c[k]);
    for (int a = 0; a < D; ++a) put(k, a, D, chk(bk[a]));
    if (structure == MIMO_STRUCT_LINEAR) {
      if (k > 0 && memcmp(Wk, W, sizeof(double) * D * D) != 0) return {ThetaFail::kLinearW, k};
      continue;
    }
    for (int a = 0; a < D; ++a) {
      put(k, a, a, chk(-0.5 * Wk[a * D + a]));
      for (int bb = a + 1; bb < D; ++bb) {
        if (structure == MIMO_STRUCT_FULL) put(k, a, bb, chk(-0.5 * (Wk[a * D + bb] + Wk[bb * D + a])));
        else if (Wk[a * D + bb] != 0.0 || Wk[bb * D + a] != 0.0) return {ThetaFail::kDiagOffDiag, k, a, bb};
      }
    }
  }
  if (!finite) return {ThetaFail::kNonFinite};
  return {};
}

// ---- placements: count() doubles in the image, slots() component slots (those from K on are padding), at(k, a, b) the offset
// of an entry the enumerator hands out ----------------------------------------------------------------------------------------

// tile kernels (mimo_kernels.h, KernelArgs::theta): [RB][NS][64], component k in slot k % 16 of row block k / 16, feature f in
// lane quarter f % 4 of step f / 4.  RB row blocks are streamed (the rest stay zero); NS = F16 / 4 for the single-pass kernels
// and the per-problem slice of the batched ones, chunked_ns_pad(F16) for the two-stage path.
// slot_of (mimo_set_component_order; null: the identity): component k < K sits in slot slot_of[k], a permutation of 0 .. K-1; the
// padding slots stay where they are.
struct ThetaGeneric {
  int D, K, structure, RB, NS;
  const int32_t* slot_of = nullptr;
  size_t count() const { return (size_t)RB * NS * 64; }
  int slots() const { return (K + 15) / 16 * 16; }
  size_t at(int k, int a, int b) const {
    const int f = struct_feat_index(structure, D, a, b);
    const int s = slot_of && k < K ? slot_of[k] : k;
    return ((size_t)(s / 16) * NS + f / 4) * 64 + (f % 4) * 16 + s % 16;
  }
};

// small-shape kernel (mimo_kernels.h): [Kp][F] row-major over the FULL feature map whatever the structure (a structure hint
// only decides which entries of W are read)
struct ThetaSmall {
  int D, K, Kp;
  size_t count() const { return (size_t)Kp * feat_count(D); }
  int slots() const { return Kp; }
  size_t at(int k, int a, int b) const { return (size_t)k * feat_count(D) + feat_index(D, a, b); }
};

// 4 step + index of every feature of the full map in the grouped order (narrow_group_pos), built once per image
struct ThetaGroupedOrder {
  uint16_t pos[(kMaxD + 1) * (kMaxD + 2) / 2];
  explicit ThetaGroupedOrder(int D) {
    for (int a = 0; a <= D; ++a)
      for (int b = a; b <= D; ++b) {
        int st, j;
        narrow_group_pos(D, a, b, &st, &j);
        pos[feat_index(D, a, b)] = (uint16_t)(4 * st + j);
      }
  }
};

// component k of the kernels whose output lane holds a contiguous quarter of V = 4 KB components (row-owner and mid label
// kernels): slot k / V + 4 (k % 4) of row block (k % V) / 4
inline void theta_owner_slot(int k, int V, int* rb, int* i) { const int t = k % V; *rb = t / 4; *i = k / V + 4 * (t % 4); }

// narrow kernels (mimo_extra.h): [NSF][V][16]; slice s V + c, entry 4 kk + j = Theta[component j V + c][feature 4 s + kk], over
// the structure's map — or, grouped (narrow_dt, full map only), over the grouped order
struct ThetaNarrow {
  int D, K, structure, V, NSF;
  const ThetaGroupedOrder* grouped;     // null: plain
  size_t count() const { return (size_t)NSF * V * 16; }
  int slots() const { return 4 * V; }
  size_t at(int k, int a, int b) const {
    const int g = grouped ? grouped->pos[feat_index(D, a, b)] : struct_feat_index(structure, D, a, b);
    return ((size_t)(g / 4) * V + k % V) * 16 + 4 * (g % 4) + k / V;
  }
};

// mid kernels (mimo_extra.h): [steps][KB][64] in the grouped order + pf zero slices; the label pass permutes the components
// as the row-owner image does.  Full structure only (mid_covers / mid_labels_covers admit nothing else).
struct ThetaMid {
  int D, K, KB, NS, pf;
  bool labels;
  const ThetaGroupedOrder* grouped;
  size_t count() const { return ((size_t)NS * KB + pf) * 64; }
  int slots() const { return 16 * KB; }
  size_t at(int k, int a, int b) const {
    const int g = grouped->pos[feat_index(D, a, b)];
    int rb = k / 16, i = k % 16;
    if (labels) theta_owner_slot(k, 4 * KB, &rb, &i);
    return ((size_t)(g / 4) * KB + rb) * 64 + 16 * (g % 4) + i;
  }
};

// row-owner kernels (mimo_rowwave.hip): [NS][KB][64] over the structure's map, an output lane holds a contiguous quarter of
// the components (NS: whole chunks where the label kernel streams Theta)
struct ThetaRowOwner {
  int D, K, structure, KB, NS;
  size_t count() const { return (size_t)NS * KB * 64; }
  int slots() const { return 16 * KB; }
  size_t at(int k, int a, int b) const {
    const int f = struct_feat_index(structure, D, a, b);
    int rb, i;
    theta_owner_slot(k, 4 * KB, &rb, &i);
    return ((size_t)(f / 4) * KB + rb) * 64 + (f % 4) * 16 + i;
  }
};

// One problem's image: zeros, the entries, and c = kPadLogDensity in the padding slots — l = -1e300 for every datum, so the
// normalise phase needs no "does this component exist" test (exp -> 0, never the maximum, zero weight in the statistics).
// On a failure the image is left half written and must not be used.
template <typename Placement>
inline ThetaFail pack_theta(const Placement& pl, int structure, const double* c, const double* b, const double* W, double* img) {
  memset(img, 0, pl.count() * sizeof(double));
  const ThetaFail f = theta_entries(pl.D, pl.K, structure, c, b, W, [&](int k, int a, int bb, double v) { img[pl.at(k, a, bb)] = v; });
  if (f.kind) return f;
  for (int k = pl.K; k < pl.slots(); ++k) img[pl.at(k, pl.D, pl.D)] = kPadLogDensity;
  return f;
}

}  // namespace mimo
