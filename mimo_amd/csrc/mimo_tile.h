// Device-side pieces of the tile kernels shared by mimo_kernels.hip and mimo_pipe.hip: the Philox batch of the label draw,
// the compile-time feature map, the per-datum normalisation of an LDS-resident L tile, the diagnostic phase stamps.
#pragma once
// Exponential of the tile kernels' normalise phase: 64-entry table + quintic (exp_nonpos, 15 instructions), or — E2K, the
// single-pass E-step kernels at Dz >= 14 — the 2048-entry table with the pre-compensated scale (exp_nonpos_t2048c, 12
// instructions, 16 KB of LDS more per workgroup).  Dz >= 14 runs two workgroups per CU with either table (54 - 64 KB + 16 KB <= 80 KB);
// below, the larger table costs the third workgroup and more than it gives (measured, round 3: C2 kernel 6.71 -> 6.60 ms with it,
// C4 — Dz = 12, three workgroups — 2.13 -> 2.24 ms).
#include "mimo_device.h"

#include <math.h>
#include <type_traits>
#include <utility>

namespace mimo {

#ifndef MIMO_EXP_CHAINS
#define MIMO_EXP_CHAINS 8   // independent exp chains the normalise phase keeps in flight (register-array variant)
#endif

// The 8 lanes that share a datum would all run the same ten Philox rounds (~20 64-bit multiplies + ~40 integer
// instructions on the pipe the f64 MFMAs use).  Instead a wave draws, every 8th tile, the uniforms of its 8 data
// rows for the NEXT 8 tiles of the workgroup's grid-stride walk — lane (pt = lane & 7, j = lane >> 3) holds the
// uniform of row pt of tile t + j * stride — and each tile fetches its value with one lane exchange.  The counter
// is still (global row, sweep): the labels are the same labels.  Used by the K <= 64 kernels only: in the K > 64
// kernels (RBW = 4, already at the 256-register cap) the two extra loop-carried registers pushed other loop-carried
// values into scratch — 3.6 GB of spill writes per launch at C3 for a 4 % gain — so those draw per tile.
struct PhiloxBatch {
  double u = 0.0;
  int used = 8;     // tiles consumed from the batch (8 = empty)
};
__device__ __forceinline__ double philox_for_tile(PhiloxBatch& pb, const KernelArgs& a, const int64_t n, const int lane,
                                                  const int64_t tile_stride_rows) {
  if (pb.used == 8) {     // wave-uniform
    pb.u = philox_uniform(a.seed, (uint64_t)(a.row0 + n + (int64_t)(lane >> 3) * tile_stride_rows), a.sweep);
    pb.used = 0;
  }
  const double uu = __shfl(pb.u, (pb.used << 3) | (lane & 7));
  pb.used += 1;
  return uu;
}

#ifdef MIMO_STAMPS
// diagnostic build: per-wave cycle sums of the phases of the tile loop (never in the shipped library)
#define STAMP(i)                                                                          \
  do {                                                                                    \
    unsigned long long t_;                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    st_sum[i] += t_ - st_prev;                                                            \
    st_prev = t_;                                                                         \
  } while (0)
#else
#define STAMP(i) do {} while (0)
#endif

// ------------------------------------------------------------------------------------------
// Compile-time feature map for the E-step modes (DS = Dz known at compile time): feature f of
// z~ = [z, 1] is z~_a z~_b with (a,b) the f-th pair of the upper triangle, row-major; padded
// features (f >= F) read the zero slot z~[D+1].
// ------------------------------------------------------------------------------------------
template <int D, int F>
struct FeatAB {
  static constexpr int find_a() {
    int a = 0, base = 0;
    while (a <= D && base + (D + 1 - a) <= F) { base += D + 1 - a; ++a; }
    return a;
  }
  static constexpr int base_of(int a) {
    int b = 0;
    for (int i = 0; i < a; ++i) b += D + 1 - i;
    return b;
  }
  static constexpr bool pad = F >= (D + 1) * (D + 2) / 2;
  static constexpr int a = pad ? D + 1 : find_a();
  static constexpr int b = pad ? D + 1 : a + (F - base_of(a));
};

// lane (row = lane & 31, parity = lane >> 5) of wave W writes features W*FW + 2i + parity, i < FW/2.
// ZB: the two parities of a pair almost always differ by one position of ONE operand (same a, b + 1), so the parity rides on
// an LDS address instead of a per-lane select: zl[d] = z~[d] for both halves of the wave, zb[d] = z~[d + parity] (the same row
// read 8 bytes further on in the upper half; zb[D] is z~[D] or the zero slot).  An operand whose index is the same for both
// features comes from zl, one that steps by one from zb: static registers, no v_cndmask.  Only the pairs that straddle the
// end of a triangle row — (a, D) beside (a+1, a+1), 8 of the 77 pairs at Dz = 16 — keep a select, for their b operand
// alone (the a operand steps by one).  A select between z~[i] and z~[j] is two v_cndmask_b32: 101 of them beside the 77
// products of the Dz = 16 kernel, 17 now; 20 VALU fewer per wave-tile at C2 (profiles/r07_c2_valu_trim.txt).  The factors of
// every product are the doubles they were.  !ZB (the instantiations fused_kernel leaves as they were): both operands selected.
template <int D, int I0, int I1, bool ZB>
__device__ __forceinline__ double feature_operand(const double (&zl)[D + 2], const double (&zb)[D + 1], const bool parity) {
  if constexpr (I1 == I0) return zl[I0];
  else if constexpr (ZB && I1 == I0 + 1 && I0 <= D) return zb[I0];
  else return parity ? zl[I1] : zl[I0];
}
template <int D, int FW, int W, bool ZB, int... I>
__device__ __forceinline__ void build_features_static(const double (&zl)[D + 2], const double (&zb)[D + 1],
                                                      double* __restrict__ prow, const bool parity,
                                                      std::integer_sequence<int, I...>) {
  ((prow[W * FW + 2 * I] =
        feature_operand<D, FeatAB<D, W * FW + 2 * I>::a, FeatAB<D, W * FW + 2 * I + 1>::a, ZB>(zl, zb, parity) *
        feature_operand<D, FeatAB<D, W * FW + 2 * I>::b, FeatAB<D, W * FW + 2 * I + 1>::b, ZB>(zl, zb, parity)),
   ...);
}

// ------------------------------------------------------------------------------------------
// Per-datum normalisation over k of one 32-row tile held in LDS as Lt[row][component]:
// 8 lanes per datum, 2*K16 consecutive components per lane (<= 8 here: RBW = 1), fully unrolled.
// Softmax -> r written back in place, or inverse-CDF categorical draw -> label (LDS + HBM).
// SKIP (softmax of the fast VI mode): also the member masks of the responsibility skip.  Row pt is live in row block b
// when one of its 16 components there has l - m >= lnt = ln tau, i.e. e >= tau; r = e / sum e <= e, so every weight
// of a row left out of block b is below tau.  live[b] (32 bits, LDS) gets bit pt for each live row of the tile: wave w
// writes byte w of every word (its rows 8w .. 8w+7), so the words need no clearing between tiles.
// LX: the butterfly stages (lane ^ 8, ^ 16, ^ 32) of the maximum, the sums and the label count exchange lanes in registers
// (lane_xor_max / lane_xor_sum, mimo_device.h) instead of through __shfl_xor; the caller says which, same bits either way.
// CERT (SKIP at K16 = 4, DESIGN section 4 "E-step certificates"), everything delivered bit for bit what CERT = 0 delivers:
//   kCertReference  also stores, per row < N, the slot of the largest l, that l, and the largest l outside its row block.  The
//                   block maxima exist after the lane ^ 8 stage; the stages ^ 16 and ^ 32 then carry the pair (largest,
//                   second largest block maximum): the second largest IS the largest outside the winner's block.  One lane
//                   per row stores: of the lanes whose own maximum equals the row's, the lowest.
//   kCertCertified  cert_row is the offset from Lt of the 8 doubles this lane loads: its slots of row pt where they were contracted
//                   this tile, else 8 doubles of -inf kept in LDS, not the stale tile.  Such a lane belongs to a row proven dead in its block: the
//                   maximum lies elsewhere, its exponentials are 0 where CERT = 0 has values below 2^-60 (48 of them at most:
//                   under half an ulp of a sum >= 1, which they meet only at the ^ 16 and ^ 32 stages), its live bit is clear
//                   either way, and nothing reads the weights it writes back.  cert_live != 0 (scalar): the wave's eight rows are
//                   all proven; cert_row is then the lane's TWO slots of the row's own block and cert_live the wave's four live
//                   bytes (the proven wave, at the top of the function).
// ------------------------------------------------------------------------------------------
// {max, min} of v and the value of lane ^ MASK (MASK 16 or 32: the swap hands them over in lane-dependent order)
template <int MASK>
__device__ __forceinline__ void lane_xor_maxmin(double v, double& hi, double& lo) {
  const LanePair l = lane_xor_pair<MASK>(__double2loint(v)), h = lane_xor_pair<MASK>(__double2hiint(v));
  const double x = __hiloint2double(h.a, l.a), y = __hiloint2double(h.b, l.b);
  hi = fmax(x, y);
  lo = fmin(x, y);
}
template <int RBW, int MODE, bool E2K = false, bool SKIP = false, bool LX = false, int CERT = 0>
__device__ __forceinline__ void normalise_tile(const KernelArgs& a, double* __restrict__ Lt, const int LS,
                                               const double* __restrict__ etab, const int K, const int K16,
                                               const int64_t N, const int64_t n0, const int wave, const int lane,
                                               const bool gibbs, double* const out_logp, double* const out_resp,
                                               double* const out_lse, double& sc_lse, double& sc_rl, double& sc_prod,
                                               int* __restrict__ labs, PhiloxBatch& pb,
                                               const int64_t tstride, const double lnt = 0.0,
                                               uint32_t* __restrict__ live = nullptr, const int cert_row = 0,
                                               const uint32_t cert_live = 0) {
        static_assert(RBW == 1, "register variant: at most 8 components per lane");
        static_assert(!SKIP || MODE == kFastVI, "responsibility skip: softmax of the fast VI mode only");
        static_assert(CERT == 0 || (SKIP && LX), "certificates: the skipping softmax pass, lane exchanges in registers");
        const int pt = 8 * wave + (lane & 7), part = lane >> 3;
        if constexpr (CERT == kCertCertified) {
          // Proven wave (cert_live != 0, scalar: all eight rows of this wave proven, K16 = 4): every row is live in its own row block
          // and in no other, so the eight lanes of a row share that block's 16 slots, two each (cert_row: slots 2 part and 2 part
          // + 1 of the block), instead of six of them pushing the -inf row through eight exponentials each.  Same bits: with
          // p_c = e_2c + e_2c+1 in lane c the stages ^8, ^16, ^32 add ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), which is
          // tree_sum8 of slots 0 .. 7 plus tree_sum8 of slots 8 .. 15, the block sum of the eight-slot map after its ^8 stage; what
          // that map adds to it at ^16 and ^32 is below half an ulp of a sum >= 1 (above).  The maximum is exact in any order, and
          // it lies in the block.  The wave's live bytes are cert_live itself (the caller made them from the rows' block bits):
          // no compare, no ballot.  Only the two weights are written back: the statistics of block b read the rows live in b.
          if (cert_live != 0) {
            double* src = Lt + cert_row;
            double x0 = src[0], x1 = src[1];
            double m = fmax(x0, x1);
            m = butterfly_max<LX, 8>(m);
            m = butterfly_max<LX, 16>(m);
            m = butterfly_max<LX, 32>(m);
            if (lane < K16) reinterpret_cast<uint8_t*>(live)[4 * lane + wave] = (uint8_t)(cert_live >> (8 * lane));
            x0 = E2K ? exp_nonpos_t2048c(x0 - m, etab) : exp_nonpos(x0 - m, etab);
            x1 = E2K ? exp_nonpos_t2048c(x1 - m, etab) : exp_nonpos(x1 - m, etab);
            double ssum = x0 + x1;
            ssum = butterfly_sum<LX, 8>(ssum);
            ssum = butterfly_sum<LX, 16>(ssum);
            ssum = butterfly_sum<LX, 32>(ssum);
            double inv = __builtin_amdgcn_rcp(ssum);
            inv = fma(fma(-ssum, inv, 1.0), inv, inv);
            inv = fma(fma(-ssum, inv, 1.0), inv, inv);
            if (part == 0) {            // (a proven row lies inside N)
              sc_lse += m;
              sc_prod *= ssum;
            }
            src[0] = x0 * inv;
            src[1] = x1 * inv;
            return;
          }
        }
        const int CPP = 2 * K16, k0 = part * CPP;
        const int64_t n = n0 + pt;
        const bool valid = n < N;
        double* row = Lt + pt * LS + k0;

        auto body = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        // Padding components (k >= K inside the last row block) carry l = kPadLogDensity from the operand
        // image, so only the HBM table writes test k < K.  FULL: this lane owns all 8 slots (K16 = 4) and no
        // slot test is compiled at all; otherwise slots c >= CPP belong to the next lane and are masked.
        auto ok = [&](int c) { return FULL || c < CPP; };
        // x[] holds l, then exp(l - max), then the weight written back — one register array
        double x[8], lsave[8];
        if constexpr (CERT == kCertCertified && FULL) {
          const double* src = Lt + cert_row;        // the lane's slots of the tile, or the -inf row: one select, made by the caller
#pragma unroll
          for (int c = 0; c < 8; ++c) x[c] = src[c];
        } else {
#pragma unroll
          for (int c = 0; c < 8; ++c) x[c] = ok(c) ? row[c] : -INFINITY;
        }
        if (out_logp && valid) {
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (c < CPP && k0 + c < K) out_logp[(int64_t)(k0 + c) * N + n] = x[c];
        }
        const double ml = tree_max8(x);     // the lane's own maximum (SKIP, FULL: kept for the live mask)
        double m = butterfly_max<LX, 8>(ml);
        if constexpr (CERT == kCertReference && FULL) {
          double m16, s16, s32, t32, u32;
          lane_xor_maxmin<16>(m, m16, s16);         // (largest, second largest) of this pair of row blocks
          lane_xor_maxmin<32>(m16, m, t32);         // m: fmax of the same two values as below, the same bits
          lane_xor_maxmin<32>(s16, s32, u32);
          const double second = fmax(t32, s32);     // the largest block maximum but one = the largest l outside the winner's block
          const bool cand = valid && ml == m;
          const uint64_t bal = __builtin_amdgcn_ballot_w64(cand);
          const uint64_t mine = (bal >> (lane & 7)) & 0x0101010101010101ull;      // bit 8 p: part p of this row is a candidate
          if (cand && (mine & ((1ull << (8 * part)) - 1ull)) == 0) {              // the lowest candidate part of the row stores
            int cs = 7;
#pragma unroll
            for (int c = 6; c >= 0; --c) cs = x[c] == ml ? c : cs;
            a.cert_k[n] = (uint8_t)(k0 + cs);
            a.cert_m[n] = m;
            a.cert_a[n] = second;
          }
        } else {
          m = butterfly_max<LX, 16>(m);
          m = butterfly_max<LX, 32>(m);
        }

        if constexpr (SKIP) {
          uint32_t bytes = 0;               // byte b: the live rows of this wave in row block b
          if constexpr (FULL) {
            // The lane's 8 slots lie in one row block (part >> 1), and x -> fl(x - m) is monotone, so "one of the slots
            // has l - m >= lnt" is exactly ml - m >= lnt: one subtract and one compare instead of eight of each with
            // their selects, and ONE ballot holds all four row blocks — lanes 16 b .. 16 b + 15 are the two parts of
            // block b, rows 8 wave + (0 .. 7) each; the OR of the two bytes is scalar work.  Same decisions, same masks;
            // 23 VALU fewer per wave-tile at C2 (profiles/r07_c2_valu_trim.txt).  (The builtin takes the predicate as it
            // is: __ballot() goes through an int, a v_cndmask and a v_cmp_ne of their own.)
            const uint64_t bal = __builtin_amdgcn_ballot_w64(valid && ml - m >= lnt);
#pragma unroll
            for (int b = 0; b < 4; ++b)
              bytes |= (uint32_t)(((bal >> (16 * b)) | (bal >> (16 * b + 8))) & 0xFFu) << (8 * b);
          } else {
            // 2*K16 < 8 slots may straddle two row blocks: per slot.  Bit b of lb: one of this lane's slots in row block
            // b is live (masked slots hold -inf: never live).
            uint32_t lb = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c)
              if (ok(c) && x[c] - m >= lnt) lb |= 1u << ((k0 + c) >> 4);
            if (!valid) lb = 0;
            // per row block: ballot over the wave (bit 8 part + i: row 8 wave + i), OR over the 8 parts -> one byte
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (b < K16) {
                const uint64_t bal = __ballot((lb >> b) & 1u);
                uint32_t v = (uint32_t)bal | (uint32_t)(bal >> 32);
                v |= v >> 16;
                v |= v >> 8;
                bytes |= (v & 0xFFu) << (8 * b);
              }
            }
          }
          if (lane < K16) reinterpret_cast<uint8_t*>(live)[4 * lane + wave] = (uint8_t)(bytes >> (8 * lane));
        }

#pragma unroll
        for (int c = 0; c < 8; ++c) {
          // (a component switched off by c_k = -inf carries l = -1e300: its e is exp(-707) = 8e-308, not 0, and
          // e * l would add -8e-8 per datum to sum_k r l — its term is 0 * (-inf) := 0, like the padding's)
          if constexpr (MODE == kGeneric) lsave[c] = (c < CPP && k0 + c < K && x[c] > kOffLogDensity) ? x[c] : 0.0;
          x[c] = E2K ? exp_nonpos_t2048c(x[c] - m, etab) : exp_nonpos(x[c] - m, etab);      // masked / padding slots -> 0
        }
        double sel = 0.0;
        if constexpr (MODE == kGeneric) {   // sum_k e l only feeds the entropy split of the ELBO (scalars[1..2])
          double t[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) t[c] = x[c] * lsave[c];
          sel = tree_sum8(t);
          sel = butterfly_sum<LX, 8>(sel);
          sel = butterfly_sum<LX, 16>(sel);
          sel = butterfly_sum<LX, 32>(sel);
        }

        if (!gibbs) {
          double ssum = tree_sum8(x);
          ssum = butterfly_sum<LX, 8>(ssum);
          ssum = butterfly_sum<LX, 16>(ssum);
          ssum = butterfly_sum<LX, 32>(ssum);
          // 1 / sum: v_rcp_f64 seed + two Newton steps (5 dependent f64 ops instead of the IEEE divide's
          // ~12; every one of them waits for a matrix-pipe slot); relative error <= 1 ulp-ish (2^-52).
          double inv = __builtin_amdgcn_rcp(ssum);
          inv = fma(fma(-ssum, inv, 1.0), inv, inv);
          inv = fma(fma(-ssum, inv, 1.0), inv, inv);
          if constexpr (MODE == kGeneric) {
            const double lse = m + log(ssum);
            if (part == 0 && valid) {
              sc_lse += lse;
              sc_rl += sel * inv;
              if (out_lse) out_lse[n] = lse;
            }
          } else {
            // fast modes only need sum_n lse_n = sum_n m_n + log prod_n ssum_n: the product of the per-datum
            // sums (each in [1, K]) is accumulated and its log taken once per 64 tiles by the caller.
            if (part == 0 && valid) {
              sc_lse += m;
              sc_prod *= ssum;
            }
          }
          const double scale = valid ? inv : 0.0;
          // per-row weights (generic mode only; a.u doubles as the weight vector of a mean-field pass): the
          // statistics are those of r_kn w_n, the tables and the ELBO scalars those of r_kn
          // (mimo/mixtures/hgmm.py:199-207: resp * weights feeds the update, the unweighted resp the bound)
          double wrow = 1.0;
          if constexpr (MODE == kGeneric) wrow = (a.u && valid) ? a.u[n] : 1.0;
          if (out_resp && valid) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
              if (c < CPP && k0 + c < K) out_resp[(int64_t)(k0 + c) * N + n] = x[c] * scale;
          }
          const double wscale = MODE == kGeneric ? scale * wrow : scale;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            x[c] *= wscale;
            if (ok(c)) row[c] = x[c];
          }
        } else {
          // inverse-CDF draw (mimo/utils/stats.py:10-17): label = #{k : u * cum[K-1] > cum[k]} with
          // cum = cumsum_k exp(l_k - lse).  The count is invariant to the common factor 1/sum e, so the
          // UNNORMALISED cumulative sums E_k = sum_{j<=k} e_j are compared with u * E_K (same labels up
          // to last-bit ties; no per-component scaling, no one-hot table: only the label is kept).
          scan8(x);                                  // local inclusive cumulative sums
          const double cum = x[7];
          double incl = cum;  // inclusive scan over the 8 parts of this datum
          {
            double v = __shfl_up(incl, 8);  if (part >= 1) incl += v;
            v = __shfl_up(incl, 16);        if (part >= 2) incl += v;
            v = __shfl_up(incl, 32);        if (part >= 4) incl += v;
          }
          double excl = __shfl_up(incl, 8);
          if (part == 0) excl = 0.0;
          const double ctot = __shfl(excl + cum, 56 + (lane & 7));  // == last cumulative value
          if constexpr (MODE == kGeneric) {
            const double lse = m + log(ctot);
            if (part == 0 && valid) {
              sc_lse += lse;
              sc_rl += sel / ctot;
              if (out_lse) out_lse[n] = lse;
            }
          } else {
            if (part == 0 && valid) {
              sc_lse += m;
              sc_prod *= ctot;
            }
          }
          const double uu = a.u ? (valid ? a.u[n] : 0.0) : philox_for_tile(pb, a, n, lane, tstride);
          const double tl = uu * ctot - excl;   // threshold in this lane's local cumulative scale
          int cnt = 0;
#pragma unroll
          for (int c = 0; c < 8; ++c)     // (padding slots can only be counted above the last real one: capped below)
            cnt += (ok(c) && tl > x[c]) ? 1 : 0;
          cnt = butterfly_sum<LX, 8>(cnt);
          cnt = butterfly_sum<LX, 16>(cnt);
          cnt = butterfly_sum<LX, 32>(cnt);
          const int label = draw_label(cnt, K, a.relabel, uu);
          if (part == 0) {
            labs[pt] = valid ? label : -1;      // the statistics phase builds its one-hot operand from this
            if (valid && a.labels) a.labels[n] = label;
          }
        }
        };
        // (certificates run at K16 = 4 only: that instantiation does not carry the other body, nor the scalars it keeps across tiles)
        if (CERT == kCertCertified || CPP == 8) body(std::true_type{});
        else body(std::false_type{});
}

// Same contract for lanes that own up to 8*RBW components (RBW > 1), processed in chunks of 8.
//   pass 1: max (8 independent chains across the chunks, then a tree)
//   pass 2: e = exp(l - max) written back in place, chunk totals T[ch] (trees) kept in registers
//   pass 3: softmax: e scaled by 1/sum.  Gibbs: the chunk that holds the crossing is located from the
//           chunk totals, and only ITS eight e are read back, scanned and compared — 8 LDS reads and 12
//           compares instead of 32 + 32.
template <int RBW, int MODE, bool LX = false>
__device__ __forceinline__ void normalise_tile_chunked(const KernelArgs& a, double* __restrict__ Lt, const int LS,
                                                       const double* __restrict__ etab, const int K, const int K16,
                                                       const int64_t N, const int64_t n0, const int wave,
                                                       const int lane, const bool gibbs, double* const out_logp,
                                                       double* const out_resp, double* const out_lse,
                                                       double& sc_lse, double& sc_rl, double& sc_prod,
                                                       int* __restrict__ labs, PhiloxBatch& pb,
                                                       const int64_t tstride) {
  const int pt = 8 * wave + (lane & 7), part = lane >> 3;
  const int CPP = 2 * K16, k0 = part * CPP;
  const int64_t n = n0 + pt;
  const bool valid = n < N;
  double* row = Lt + pt * LS + k0;
  // padding components carry l = kPadLogDensity (operand image): only HBM table writes test k < K.
  // FULL: the lane owns all 8*RBW slots (K16 = 4*RBW) and no slot test is compiled.
  auto body = [&](auto full_c) {
  constexpr bool FULL = decltype(full_c)::value;
  auto ok = [&](int c) { return FULL || c < CPP; };
  auto active = [&](int c) { return ok(c) && k0 + c < K; };

  double mv[8];
#pragma unroll
  for (int cc = 0; cc < 8; ++cc) mv[cc] = -INFINITY;
#pragma unroll
  for (int ch = 0; ch < RBW; ++ch) {
    if (FULL || 8 * ch < CPP) {
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        const int c = 8 * ch + cc;
        const double l = ok(c) ? row[c] : -INFINITY;
        if (out_logp && valid && active(c)) out_logp[(int64_t)(k0 + c) * N + n] = l;
        mv[cc] = fmax(mv[cc], l);
      }
    }
  }
  double m = tree_max8(mv);
  m = butterfly_max<LX, 8>(m);
  m = butterfly_max<LX, 16>(m);
  m = butterfly_max<LX, 32>(m);

  double T[RBW], selv[RBW];
#pragma unroll
  for (int ch = 0; ch < RBW; ++ch) {
    T[ch] = 0.0;
    selv[ch] = 0.0;
    if (FULL || 8 * ch < CPP) {
      double x[8], lc[8];
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) lc[cc] = ok(8 * ch + cc) ? row[8 * ch + cc] : -INFINITY;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) x[cc] = exp_nonpos(lc[cc] - m, etab);
      T[ch] = tree_sum8(x);
      if constexpr (MODE == kGeneric) {
        double t[8];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)     // (switched-off components: see normalise_tile)
          t[cc] = x[cc] * ((active(8 * ch + cc) && lc[cc] > kOffLogDensity) ? lc[cc] : 0.0);
        selv[ch] = tree_sum8(t);
      }
#pragma unroll
      for (int cc = 0; cc < 8; ++cc)        // e replaces l in place (softmax: scaled in pass 3; Gibbs: the
        if (ok(8 * ch + cc)) row[8 * ch + cc] = x[cc];   // crossing chunk is read back in pass 3)
    }
    __builtin_amdgcn_sched_barrier(0);   // one chunk of exp chains in flight at a time (register pressure)
  }
  // exclusive prefix of the chunk totals (base[ch] = sum of the chunks before ch) and the lane total
  double base[RBW + 1];
  base[0] = 0.0;
#pragma unroll
  for (int ch = 0; ch < RBW; ++ch) base[ch + 1] = base[ch] + T[ch];
  const double cum = base[RBW];
  double sel = 0.0;
  if constexpr (MODE == kGeneric) {
#pragma unroll
    for (int ch = 0; ch < RBW; ++ch) sel += selv[ch];
    sel = butterfly_sum<LX, 8>(sel);
    sel = butterfly_sum<LX, 16>(sel);
    sel = butterfly_sum<LX, 32>(sel);
  }

  if (!gibbs) {
    double ssum = cum;
    ssum = butterfly_sum<LX, 8>(ssum);
    ssum = butterfly_sum<LX, 16>(ssum);
    ssum = butterfly_sum<LX, 32>(ssum);
    double inv = __builtin_amdgcn_rcp(ssum);
    inv = fma(fma(-ssum, inv, 1.0), inv, inv);
    inv = fma(fma(-ssum, inv, 1.0), inv, inv);
    if constexpr (MODE == kGeneric) {
      const double lse = m + log(ssum);
      if (part == 0 && valid) {
        sc_lse += lse;
        sc_rl += sel * inv;
        if (out_lse) out_lse[n] = lse;
      }
    } else {
      if (part == 0 && valid) {
        sc_lse += m;
        sc_prod *= ssum;
      }
    }
    const double scale = valid ? inv : 0.0;
    double wrow = 1.0;   // per-row weights: see normalise_tile
    if constexpr (MODE == kGeneric) wrow = (a.u && valid) ? a.u[n] : 1.0;
#pragma unroll
    for (int c = 0; c < 8 * RBW; ++c) {
      if (ok(c)) {
        const double r = row[c] * scale;
        row[c] = MODE == kGeneric ? r * wrow : r;
        if (out_resp && valid && k0 + c < K) out_resp[(int64_t)(k0 + c) * N + n] = r;
      }
      if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    // scale-invariant inverse CDF on the unnormalised cumulative sums (see normalise_tile)
    double incl = cum;
    {
      double v = __shfl_up(incl, 8);  if (part >= 1) incl += v;
      v = __shfl_up(incl, 16);        if (part >= 2) incl += v;
      v = __shfl_up(incl, 32);        if (part >= 4) incl += v;
    }
    double excl = __shfl_up(incl, 8);
    if (part == 0) excl = 0.0;
    const double ctot = __shfl(excl + cum, 56 + (lane & 7));
    if constexpr (MODE == kGeneric) {
      const double lse = m + log(ctot);
      if (part == 0 && valid) {
        sc_lse += lse;
        sc_rl += sel / ctot;
        if (out_lse) out_lse[n] = lse;
      }
    } else {
      if (part == 0 && valid) {
        sc_lse += m;
        sc_prod *= ctot;
      }
    }
    const double uu = a.u ? (valid ? a.u[n] : 0.0) : philox_uniform(a.seed, (uint64_t)(a.row0 + n), a.sweep);
    const double tl = uu * ctot - excl;
    // chunk of the crossing: j = #{ch : tl > cumulative sum at the END of chunk ch}
    int j = 0;
#pragma unroll
    for (int ch = 0; ch < RBW; ++ch) j += (tl > base[ch + 1]) ? 1 : 0;
    // components of this lane that exist at all (the count if tl lies above every cumulative sum)
    int cnt;
    if ((!FULL && 8 * j >= CPP) || j >= RBW) {
      cnt = CPP;      // above every cumulative sum of this lane (padding slots included: capped below)
    } else {
      double bj = base[0];
#pragma unroll
      for (int ch = 1; ch < RBW; ++ch) bj = (j == ch) ? base[ch] : bj;
      const double* rj = row + 8 * j;
      double x[8];
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) x[cc] = (FULL || 8 * j + cc < CPP) ? rj[cc] : 0.0;
      scan8(x);
      const double tj = tl - bj;
      cnt = 8 * j;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) cnt += ((FULL || 8 * j + cc < CPP) && tj > x[cc]) ? 1 : 0;
    }
    cnt = butterfly_sum<LX, 8>(cnt);
    cnt = butterfly_sum<LX, 16>(cnt);
    cnt = butterfly_sum<LX, 32>(cnt);
    const int label = draw_label(cnt, K, a.relabel, uu);
    if (part == 0) {
      labs[pt] = valid ? label : -1;
      if (valid && a.labels) a.labels[n] = label;
    }
  }
  };
  if (CPP == 8 * RBW) body(std::true_type{});
  else body(std::false_type{});
}

}  // namespace mimo
