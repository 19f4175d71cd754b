// Device-side helpers shared by the gfx950 kernel files (mimo_kernels.hip: MFMA tile kernels; mimo_small.hip: the
// VALU kernel for tiny K x F; mimo_rowwave.hip: the large-K Gibbs label kernel and the label-statistics pass).
#pragma once
#include "mimo_kernels.h"

#include <math.h>

namespace mimo {

// Workgroup barrier with the wave's own LDS traffic drained first.  hipcc places `s_waitcnt lgkmcnt(0)` in front
// of an s_barrier only where its memory model asks for it, and for LDS-only ordering at workgroup scope it does
// not: LLVM assumes the LDS operations of all waves execute in ONE total order, so stores issued before the
// barrier would be seen by loads other waves issue after it.  On gfx950 with two workgroups resident per CU that
// does not hold: a wave signalled the loop-top barrier with its z-tile stores still queued (behind the co-resident
// workgroup's bank-conflicted traffic), the other waves built the feature tile from the PREVIOUS tile's rows, and
// 2-8 rows of a tile came out wrong — sporadically, only on tiles after a workgroup's first, only with two
// workgroups per CU (found with a lane-layout experiment that made the window wide: 35 of 48 stress runs bad,
// 0 of 120 with this wait; DESIGN.md section 4 has the story).  88 of the 179
// kernel instantiations had such a barrier (tools/check_barrier_waits.py, a CFG dataflow over the emitted ISA,
// now part of the CPU tests).  The explicit wait costs nothing measurable: most barriers had it already.
__device__ __forceinline__ void wg_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

typedef double d4 __attribute__((ext_vector_type(4)));
// explicit global address space: a generic pointer that went through an opaque asm loads with flat_load,
// which also counts on lgkmcnt and would make every LDS-operand wait an L2 round trip
typedef const double __attribute__((address_space(1)))* gptr_t;


// ------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  key = (seed_lo, seed_hi), counter = (row_lo, row_hi,
// sweep_lo, sweep_hi); the uniform is the 53-bit float built from the first two output words.
// ------------------------------------------------------------------------------------------
__host__ __device__ inline double philox_uniform(uint64_t seed, uint64_t row, uint64_t sweep) {
  uint32_t c0 = (uint32_t)row, c1 = (uint32_t)(row >> 32);
  uint32_t c2 = (uint32_t)sweep, c3 = (uint32_t)(sweep >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

// The label of an inverse-CDF draw from `cnt`, the number of cumulative sums below the threshold u cum_K (label = #{k : u cum_K >
// cum_k}, capped at the last component: u < 1 never exceeds cum_K, its rounding may).  A component switched off by c_k = -inf has
// cum_k == cum_{k-1} and cannot be drawn with u > 0 — but the kernels compare u cum_K - (prefix of the lanes, chunks or row
// blocks in front) with LOCAL cumulative sums, and where a switched-off component opens a lane's or a chunk's slots, or closes
// the row, the prefix scans' last bit can leave the count on it.  `relabel` (KernelArgs::relabel; null when every component is
// live) sends such a count to the nearest live component below: the crossing lies within rounding of that one's upper boundary.
// (u = 0 draws component 0 whatever its weight, as the reference's rule does.)
__device__ __forceinline__ int draw_label(int cnt, int K, const int32_t* __restrict__ relabel, double u) {
  const int label = cnt < K ? cnt : K - 1;
  return (relabel && u > 0.0) ? relabel[label] : label;
}

// One column of the random initial responsibilities (random_resp_kernel of mimo_small.hip, batched_random_resp_kernel of
// mimo_batched.hip): out[k stride] = v_k / sum_j v_j, v_k = the Philox uniform of key `seed`, counter (row, k), moved to
// (0, 1] (a column of zeros cannot happen).  The sum runs over k ascending, then ONE reciprocal, then v inv: both kernels
// go through here, so a problem's table is the same bits solo and in a batch.
__device__ __forceinline__ void random_resp_column(double* __restrict__ out, int64_t stride, int K, uint64_t seed, uint64_t row) {
  double tot = 0.0;
  for (int k = 0; k < K; ++k) {
    const double v = philox_uniform(seed, row, (uint64_t)k) + 1.1102230246251565e-16;
    out[(int64_t)k * stride] = v;
    tot += v;
  }
  const double inv = 1.0 / tot;
  for (int k = 0; k < K; ++k) out[(int64_t)k * stride] *= inv;
}

// ------------------------------------------------------------------------------------------
// Lane exchanges with a compile-time XOR mask, in registers.  __shfl_xor(v, MASK) is ds_bpermute_b32 per 32-bit word:
// a per-lane address (v_xor, v_cmp, v_cndmask, v_lshlrev) and a round trip through the LDS pipe, queued behind the
// co-resident wave's MFMA operand reads, with s_waitcnt lgkmcnt(0) behind it.  A butterfly reduction needs neither:
//   MASK 1, 2   DPP quad_perm;   MASK 4   DPP row_shr:4 into banks 1, 3 and row_shl:4 into banks 0, 2;
//   MASK 8      DPP row_ror:8 (rotation by half a row of 16 lanes = lane ^ 8);
//   MASK 16, 32 v_permlane16_swap / v_permlane32_swap, which are HALF exchanges: the odd rows (upper half) of the first
//               operand trade places with the even rows (lower half) of the second.  With both operands a copy of v, one
//               result then holds the lane's own value and the other its partner's — which of the two depends on the
//               lane, and a commutative op(a, b) does not care: no select.
// lane_xor_pair returns {a, b} = {v, v of lane ^ MASK} in lane-dependent order; lane_xor_max / lane_xor_sum return
// op(v, v of lane ^ MASK), bit for bit what op(v, __shfl_xor(v, MASK)) returns (max and + are commutative, signed zeros
// included: v_max_f64 orders -0 < +0 whichever operand holds which).  All 64 lanes must be active.
// ------------------------------------------------------------------------------------------
struct LanePair { int a, b; };
template <int MASK>
__device__ __forceinline__ LanePair lane_xor_pair(int v) {
  static_assert(MASK == 1 || MASK == 2 || MASK == 4 || MASK == 8 || MASK == 16 || MASK == 32, "one bit of a wave64 lane index");
  if constexpr (MASK == 32) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return {(int)r[0], (int)r[1]};
  } else if constexpr (MASK == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return {(int)r[0], (int)r[1]};
  } else if constexpr (MASK == 8) {
    return {v, __builtin_amdgcn_update_dpp(v, v, 0x128 /* row_ror:8 */, 0xf, 0xf, false)};
  } else if constexpr (MASK == 4) {
    const int up = __builtin_amdgcn_update_dpp(v, v, 0x114 /* row_shr:4 */, 0xf, 0xa, false);     // lanes 4-7, 12-15 <- lane - 4
    return {v, __builtin_amdgcn_update_dpp(up, v, 0x104 /* row_shl:4 */, 0xf, 0x5, false)};       // lanes 0-3, 8-11  <- lane + 4
  } else {
    return {v, __builtin_amdgcn_update_dpp(v, v, MASK == 1 ? 0xb1 /* quad_perm:[1,0,3,2] */ : 0x4e /* [2,3,0,1] */, 0xf, 0xf, false)};
  }
}
template <int MASK>
__device__ __forceinline__ double lane_xor_max(double v) {
  const LanePair lo = lane_xor_pair<MASK>(__double2loint(v)), hi = lane_xor_pair<MASK>(__double2hiint(v));
  return fmax(__hiloint2double(hi.a, lo.a), __hiloint2double(hi.b, lo.b));
}
template <int MASK>
__device__ __forceinline__ double lane_xor_sum(double v) {
  const LanePair lo = lane_xor_pair<MASK>(__double2loint(v)), hi = lane_xor_pair<MASK>(__double2hiint(v));
  return __hiloint2double(hi.a, lo.a) + __hiloint2double(hi.b, lo.b);
}
template <int MASK>
__device__ __forceinline__ int lane_xor_sum(int v) {
  const LanePair p = lane_xor_pair<MASK>(v);
  return p.a + p.b;
}
// One stage of a butterfly with the exchange chosen at compile time (REG: in registers, else __shfl_xor): kernels whose
// register allocation the register form would move for the worse keep the form they had, same bits either way.
template <bool REG, int MASK, typename T>
__device__ __forceinline__ T butterfly_sum(T v) {
  if constexpr (REG) return lane_xor_sum<MASK>(v);
  else return v + __shfl_xor(v, MASK);
}
template <bool REG, int MASK>
__device__ __forceinline__ double butterfly_max(double v) {
  if constexpr (REG) return lane_xor_max<MASK>(v);
  else return fmax(v, __shfl_xor(v, MASK));
}

// ... and the whole butterfly over the G adjacent lanes of a group, stages 1, 2, .. G / 2 (G a power of two)
template <bool REG, int G, int S = 1, typename T>
__device__ __forceinline__ T group_sum(T v) {
  if constexpr (S < G) return group_sum<REG, G, 2 * S>(butterfly_sum<REG, S>(v));
  else return v;
}
template <bool REG, int G, int S = 1>
__device__ __forceinline__ double group_max(double v) {
  if constexpr (S < G) return group_max<REG, G, 2 * S>(butterfly_max<REG, S>(v));
  else return v;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}


// exp(x) for x <= 0 in 10 float64 pipe operations + 4 integer ones (the f64 VALU shares its pipe with the
// f64 MFMA on gfx950 and the normalise phase is bound by its instruction count, so every instruction of
// the softmax is paid in matrix issue slots):
//   n = rint(x * 64/ln2) via the 1.5*2^52 trick, r = x - n ln2/64 in ONE fma (|r| <= ln2/128),
//   exp(x) = 2^(n>>6) * tab[n & 63] * (1 + r + ... + r^5/120),  tab[j] = 2^(j/64) in LDS.
// The single-constant reduction leaves an error of |n| * 1.2e-18 in r, i.e. a relative error of
// 1.1e-16 * |x| in the result — an ABSOLUTE error below 4e-17 for every x <= 0 (max of |x| e^x), which is
// what a sum of exponentials whose largest term is 1 sees.  The argument is clamped at -707 (also -inf and the
// -1e300 of padding components): everything below returns exp(-707) = 8e-308, the smallest value whose exponent
// field the integer add below cannot underflow — zero for every purpose here (sums whose largest term is 1), and
// one v_max_f64 instead of a 64-bit compare and two selects per element.  The shift by 6 goes through an opaque
// asm: LLVM otherwise rewrites ((n >> 6) << 20) + hi as shift, mask and a 64-bit add (3 instructions for 2).
//
// The argument-reduction constants of all five exponentials, named once.  The two fractions of ln2 are hex literals — the doubles
// nearest ln2 / 64 and ln2 / 2048, the same 53 bits at two exponents — and the assertions tie every constant to ln2 =
// 0x1.62e42fefa39efp-1 (a decimal ln2 / 2048 that was off by 1.41e-14 relative once cost the 2048-entry variants a factor of 127 in
// their error, unseen by any whole-array comparison).  The contract — relative error ~ 2^-53 |x|, absolute error < 4e-17 — is held
// per entry against a longdouble reference over x in [-703, 0] by tests/test_gpu_softmax_accuracy.py.
constexpr double k64_Ln2 = 92.33248261689366;            // 64 / ln2    (0x1.71547652b82fep+6)
constexpr double kLn2_64 = 0x1.62e42fefa39efp-7;         // ln2 / 64
constexpr double k2048_Ln2 = 2954.639443740597;          // 2048 / ln2  (0x1.71547652b82fep+11)
constexpr double kLn2_2048 = 0x1.62e42fefa39efp-12;      // ln2 / 2048
static_assert(kLn2_2048 * 32 == kLn2_64, "ln2 / 2048 and ln2 / 64 must be the same bits, five exponents apart");
static_assert(kLn2_64 * 64 == 0x1.62e42fefa39efp-1, "ln2 / 64 must be the double nearest ln2, scaled");
static_assert(k2048_Ln2 - 32 * k64_Ln2 <= 0x1p-41 && 32 * k64_Ln2 - k2048_Ln2 <= 0x1p-41, "2048 / ln2 must be within one ulp of 32 (64 / ln2)");
static_assert(k64_Ln2 * kLn2_64 - 1.0 <= 0x1p-51 && 1.0 - k64_Ln2 * kLn2_64 <= 0x1p-51, "64 / ln2 and ln2 / 64 must be reciprocal to two ulps");
__device__ inline double exp_nonpos(double x, const double* __restrict__ tab) {
  x = fmax(x, -707.0);
  const double t = fma(x, k64_Ln2, 6755399441055744.0);
  const int n = __double2loint(t);
  const double nf = t - 6755399441055744.0;
  const double r = fma(nf, -kLn2_64, x);
  double q = fma(r, 1.0 / 120.0, 1.0 / 24.0);
  q = fma(r, q, 1.0 / 6.0);
  q = fma(r, q, 0.5);
  q = fma(r, q, 1.0);
  const double e = tab[n & 63] * fma(r, q, 1.0);
  int n6;
  asm("v_ashrrev_i32 %0, 6, %1" : "=v"(n6) : "v"(n));
  return __hiloint2double(__double2hiint(e) + (n6 << 20), __double2loint(e));
}

// exp(x), x <= 0, with a 2048-entry table of 2^(i/2048) (16 KB of LDS, where a kernel has them to spare: the row-owner kernels, the small-shape kernel): the reduced
// argument is <= ln2/4096, a cubic is enough (r^4/24 < 4e-17) — 13 instructions instead of the 15 of exp_nonpos, and
// the row-owner label kernel issues 64 of them per lane and step.  Same argument clamp, same single-constant reduction with the
// SAME 53 bits of ln2 (kLn2_2048 = kLn2_64 / 32, asserted above): n is 32 times larger and the constant's error 32 times smaller, so
// the reduction error is exp_nonpos's — relative error 1.1e-16 |x|, an absolute error below 4e-17 for every x <= 0.  It holds only
// while kLn2_2048 is the double nearest ln2 / 2048: every unit in its last place costs another 1.4 * 2^-53 |x|.
constexpr int kExpTab = 2048;
__device__ __forceinline__ double exp_nonpos_t2048(double x, const double* __restrict__ tab) {
  x = fmax(x, -707.0);
  const double t = fma(x, k2048_Ln2, 6755399441055744.0);                  // 1.5 * 2^52
  const int n = __double2loint(t);
  const double nf = t - 6755399441055744.0;
  const double r = fma(nf, -kLn2_2048, x);
  double q = fma(r, 1.0 / 6.0, 0.5);
  q = fma(r, q, 1.0);
  const double e = tab[n & (kExpTab - 1)] * fma(r, q, 1.0);
  int nh;
  asm("v_ashrrev_i32 %0, 11, %1" : "=v"(nh) : "v"(n));
  return __hiloint2double(__double2hiint(e) + (nh << 20), __double2loint(e));
}

// The same exponential with ONE integer instruction for the factor 2^(n >> 11) instead of two: table entry i holds the bit
// pattern of 2^(i/2048) with (i << 9) subtracted from its high word, so that adding (n << 9) — n = 2048 (n >> 11) + i — to
// the high word lands on hi(2^(i/2048)) + ((n >> 11) << 20): the low bits of n cancel by construction (v_lshl_add_u32 in
// place of v_ashrrev_i32 + v_lshl_add_u32).  12 instructions with the subtraction of the row maximum; same error bound.
__device__ __forceinline__ double exp_tab_entry_c(int i) {
  const double v = exp2((double)i * (1.0 / kExpTab));
  return __hiloint2double(__double2hiint(v) - (i << 9), __double2loint(v));
}
__device__ __forceinline__ double exp_nonpos_t2048c(double x, const double* __restrict__ tab) {
  x = fmax(x, -707.0);
  const double t = fma(x, k2048_Ln2, 6755399441055744.0);                  // 1.5 * 2^52
  const int n = __double2loint(t);
  const double nf = t - 6755399441055744.0;
  const double r = fma(nf, -kLn2_2048, x);
  double q = fma(r, 1.0 / 6.0, 0.5);
  q = fma(r, q, 1.0);
  const double tv = tab[n & (kExpTab - 1)];
  int hi;
  asm("v_lshl_add_u32 %0, %1, 9, %2" : "=v"(hi) : "v"(n), "v"(__double2hiint(tv)));
  return __hiloint2double(hi, __double2loint(tv)) * fma(r, q, 1.0);
}

// ... in two halves, so that a kernel can put a batch of table reads in flight before it needs the first of them (hipcc
// otherwise keeps two lookups in flight and waits ~25 cycles after each read: the LDS round trip of every pair of
// exponentials lay open in narrow_kernel, 31 % of the pipe idle at three waves per SIMD):
//   exp_c_issue:  reduced argument r and the integer n (table index n & 2047, scale n >> 11);   the caller reads tab[n & 2047]
//   exp_c_finish: cubic in r times the scaled table entry
__device__ __forceinline__ void exp_c_issue(double x, double& r, int& n) {
  x = fmax(x, -707.0);
  const double t = fma(x, k2048_Ln2, 6755399441055744.0);
  n = __double2loint(t);
  r = fma(t - 6755399441055744.0, -kLn2_2048, x);
}
__device__ __forceinline__ double exp_c_finish(double r, int n, double tv) {
  double q = fma(r, 1.0 / 6.0, 0.5);
  q = fma(r, q, 1.0);
  int hi;
  asm("v_lshl_add_u32 %0, %1, 9, %2" : "=v"(hi) : "v"(n), "v"(__double2hiint(tv)));
  return __hiloint2double(hi, __double2loint(tv)) * fma(r, q, 1.0);
}

// ------------------------------------------------------------------------------------------
// Short dependency chains.  The f64 VALU shares its pipe with the f64 MFMA, and the wave of the OTHER
// workgroup on this SIMD is usually inside a matrix phase: every time this wave has no ready f64
// instruction (it waits for the previous result), the pipe goes to an MFMA for 64 cycles.  A dependent
// chain therefore costs ~70 cycles per link, an independent group ~6 per instruction (measured with
// what-if builds at C3: the 32-link max / running-sum / compare chains were 45 % of the normalise phase).
// All reductions below are trees, the cumulative sum is a Kogge-Stone scan.
// ------------------------------------------------------------------------------------------
// (mimo_kernels.hip is compiled with -fno-honor-nans: without it LLVM puts a canonicalising self-max in front
// of every fmax whose operands may be signalling NaNs — anything that came out of memory or a lane exchange —
// which doubled the f64 instructions of the max tree: 21 -> 10 v_max_f64 per lane at K = 64.  No kernel here
// computes with NaNs: the host rejects NaN input.)
__device__ __forceinline__ double tree_max8(const double (&v)[8]) {
  return fmax(fmax(fmax(v[0], v[1]), fmax(v[2], v[3])), fmax(fmax(v[4], v[5]), fmax(v[6], v[7])));
}
__device__ __forceinline__ double tree_sum8(const double (&v)[8]) {   // == scan8(v)[7], bit for bit
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}
__device__ __forceinline__ void scan8(double (&x)[8]) {               // inclusive, 3 levels
  double a[8], b[8];
  a[0] = x[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) a[i] = x[i - 1] + x[i];
  b[0] = a[0]; b[1] = a[1];
#pragma unroll
  for (int i = 2; i < 8; ++i) b[i] = a[i - 2] + a[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = b[i];
#pragma unroll
  for (int i = 4; i < 8; ++i) x[i] = b[i - 4] + b[i];
}

}  // namespace mimo
