// gfx950 kernels for the statistics of hard labels (the second half of a Gibbs sweep: S[label_n] += phi(z_n)), K <= 256:
//
//   label_stats_kernel<DZ, FS>         Dz <= 9 (reduced feature maps: Dz <= 16), every component the same number of threads
//   label_stats_slots_kernel<DZ, FS>   Dz <= 9, K >= 17, N >= 2^17: threads in proportion to the components' rows
//                                      (label_hist_kernel + label_slots_kernel build the slot table)
//   label_stats_wide_kernel<DZ, FP>    Dz = 10 .. 16: a component's threads split the features; windows of 128 components
//   label_stats_gram_kernel<DZ>        Dz >= 17 (and K > 128 from Dz = 15): one pass over the tiles ranked by
//   label_tile_sort_kernel<256>        ... this kernel, Gram matrices per component on the matrix cores
//
// and the routing between them: label_stats_plan decides kernel, launches, ranked-tile buffers and grid rule once;
// label_stats_covers, label_stats_grid and launch_label_stats read its LabelStatsPlan.
//
// The statistics of hard labels are a scatter; done deterministically without float atomics: per tile of rows a bitmap per
// component (integer atomic OR: order-free), stable ranks by popcount, then the threads of a component walk ITS rows in
// ascending order and accumulate the features in registers across all tiles of the workgroup.  The kernels are bound by
// HBM (the data once + 4 bytes per row) up to Dz = 9.
//
// Reference behaviour reproduced: mimo/mixtures/gmm.py:227-237 (resample_components' statistics), gaussian.py:491-502,
// data.py:160-169.
#include "mimo_device.h"
#include "mimo_extra.h"

#include <cstdlib>

namespace mimo {

// diagnostic builds (-DMIMO_STAMPS, make stamps): cycles per phase of the label-statistics kernels, summed per wave
#ifdef MIMO_STAMPS
#define LS_STAMP_INIT unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_t0 = __builtin_amdgcn_s_memtime();
#define LS_STAMP(i) { const unsigned long long t1_ = __builtin_amdgcn_s_memtime(); st_[i] += t1_ - st_t0; st_t0 = t1_; }
#define LS_STAMP_STORE if (a.stamps && (threadIdx.x & 63) == 0) { for (int i_ = 0; i_ < 8; ++i_) a.stamps[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + i_] = st_[i_]; }
#else
#define LS_STAMP_INIT
#define LS_STAMP(i)
#define LS_STAMP_STORE
#endif

// ------------------------------------------------------------------------------------------
// Statistics of hard labels, K <= 256, Dz <= 9, full feature map.  Workgroup = 256 threads; with Kp = the power of two
// >= K, thread t works for component t % Kp as part t / Kp of P = 256 / Kp: it takes every P-th row of that component's
// list (K > 128: one thread per component; K = 32: eight threads share a component, so all four waves accumulate).
// Its F accumulators (n_k, sum z, upper triangle of sum z z') live in registers across all tiles; the parts of a
// component are added in part order at the end (fixed association).
// Per tile of kLsTile rows:  z tile + labels -> LDS;  bitmap[k] |= 1 << row (integer atomics: the result does not
// depend on their order);  stable position of every row inside its component's list = popcount of the lower bits;
// thread k adds its rows in ascending row order.  Partial block per workgroup in the tile kernels' layout.
// ------------------------------------------------------------------------------------------
constexpr int kLsTile = 512;
constexpr int kLsWideTile = 256;     // tile of the Dz > 10 variants (their z tile is wider)

// FS: feature set — 0: full map (n, sum z, upper triangle of sum z z'), 1: diagonal structure (sum z_a^2, sum z_a, n in the
// order of diag_feat_index), 2: linear structure (sum z_a, n): the reduced maps of mimo_set_structure, Dz <= 16.
template <int DZ, int FS = 0>
__global__ __launch_bounds__(kWG, 2) void label_stats_kernel(const KernelArgs a) {
  constexpr int F = FS == 0 ? (DZ + 1) * (DZ + 2) / 2 : FS == 1 ? 2 * DZ + 1 : DZ + 1;
  constexpr int ZS = DZ <= 2 ? 2 : DZ <= 6 ? 6 : DZ <= 10 ? 10 : DZ <= 14 ? 14 : 18;   // 16-byte aligned rows, odd stride in 16-byte units (random rows: no systematic bank conflicts)
  constexpr int T = DZ <= 10 ? kLsTile : kLsWideTile, NW = T / 32;           // rows per tile, bitmap words per component
  constexpr int RPT = T / kWG;                       // rows per thread and tile
  constexpr int ZPT = (T * DZ + kWG - 1) / kWG;     // z elements per thread
  __shared__ __align__(16) double Zt[T * ZS];
  __shared__ __align__(16) uint32_t bitmap[kWG * NW];   // [k][word] — k-major so that thread k reads 16 consecutive words
  __shared__ uint16_t list[T];
  __shared__ int start[kWG + 1];
  __shared__ int cnts[kWG];
  __shared__ int wsum[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int64_t N = a.N;
  const int64_t ntiles = (N + T - 1) / T;
  int Kp = 1;
  while (Kp < K) Kp <<= 1;
  const int P = kWG / Kp, myk = tid & (Kp - 1), mypart = tid / Kp;      // (Kp <= 256: K <= 256)

  double acc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) acc[f] = 0.0;

  double zr[ZPT];
  int lab[2] = {-1, -1};
  auto load_tile = [&](int64_t t) {
    const int64_t base = t * T * DZ, total = N * DZ;
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
      const int64_t g = base + tid + (int64_t)kWG * i;
      zr[i] = (tid + kWG * i < T * DZ && g < total) ? a.Z[g] : 0.0;
    }
#pragma unroll
    for (int h = 0; h < RPT; ++h) {
      const int64_t n = t * T + tid + kWG * h;
      const int l = n < N ? a.labels[n] : -1;
      lab[h] = l < K ? l : -1;            // a label outside [0, K) (a caller's vector) is skipped, never an index
    }
  };
  if (blockIdx.x < ntiles) load_tile(blockIdx.x);
  LS_STAMP_INIT

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    wg_sync();                        // the previous tile's readers are done
    LS_STAMP(0)
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
      const int e = tid + kWG * i;
      if (e < T * DZ) { const int r = e / DZ; Zt[r * ZS + (e - r * DZ)] = zr[i]; }
    }
    {
      uint4* bm = reinterpret_cast<uint4*>(bitmap + tid * NW);
#pragma unroll
      for (int w = 0; w < NW / 4; ++w) bm[w] = uint4{0u, 0u, 0u, 0u};
    }
    const int l0 = lab[0], l1 = lab[1];
    if (t + gridDim.x < ntiles) load_tile(t + gridDim.x);
    LS_STAMP(1)
    wg_sync();
    LS_STAMP(2)
    if (l0 >= 0) atomicOr(&bitmap[l0 * NW + (tid >> 5)], 1u << (tid & 31));
    if (RPT > 1 && l1 >= 0) atomicOr(&bitmap[l1 * NW + ((tid + kWG) >> 5)], 1u << (tid & 31));
    wg_sync();
    LS_STAMP(3)
    // rows of component tid, and the exclusive prefix over the components (where its list starts)
    int cntk = 0;
    {
      const uint4* bm = reinterpret_cast<const uint4*>(bitmap + tid * NW);
#pragma unroll
      for (int w = 0; w < NW / 4; ++w) {
        const uint4 v = bm[w];
        cntk += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
      }
    }
    int incl = cntk;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int v = __shfl_up(incl, s);
      if (lane >= s) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    wg_sync();
    int off = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) off += w < wave ? wsum[w] : 0;
    start[tid] = off + incl - cntk;
    cnts[tid] = cntk;
    wg_sync();
    LS_STAMP(4)
    // stable position of each row in its component's list
    auto place = [&](int l, int row) {
      if (l < 0) return;
      const uint32_t* bm = bitmap + l * NW;
      const int wq = row >> 5;
      int rank = __popc(bm[wq] & ((1u << (row & 31)) - 1u));
      for (int w = 0; w < wq; ++w) rank += __popc(bm[w]);
      list[start[l] + rank] = (uint16_t)row;
    };
    place(l0, tid);
    if (RPT > 1) place(l1, tid + kWG);
    wg_sync();
    LS_STAMP(5)
    // thread (component myk, part mypart): every P-th row of the component's list, ascending
    const int st = start[myk], cmine = cnts[myk];
    for (int p = mypart; p < cmine; p += P) {
      const int row = list[st + p];
      const double* zp = Zt + row * ZS;
      double z[DZ];
#pragma unroll
      for (int d = 0; d < DZ; ++d) z[d] = zp[d];
      if constexpr (FS == 0) {
        int f = 0;
#pragma unroll
        for (int i = 0; i < DZ; ++i) {
#pragma unroll
          for (int jx = i; jx < DZ; ++jx) { acc[f] = fma(z[i], z[jx], acc[f]); ++f; }
          acc[f] += z[i]; ++f;
        }
      } else if constexpr (FS == 1) {
#pragma unroll
        for (int i = 0; i < DZ; ++i) { acc[i] = fma(z[i], z[i], acc[i]); acc[DZ + i] += z[i]; }
      } else {
#pragma unroll
        for (int i = 0; i < DZ; ++i) acc[i] += z[i];
      }
      acc[F - 1] += 1.0;
    }
    LS_STAMP(6)
  }
  LS_STAMP_STORE

  // per-workgroup partial block [16 K16][F16_total] (+ 4 scalars: none from this pass)
  const int FT = a.F16_total;
  const size_t pstride = (size_t)a.K16 * 16 * FT + 4;
  double* P_out = a.partials + (size_t)blockIdx.x * pstride;
  if (P > 1) {
    // add the parts of every component in part order, eight features at a time through LDS
    static_assert(sizeof(double) * T * ZS >= sizeof(double) * kWG * 8 || sizeof(uint32_t) * kWG * NW >= sizeof(double) * kWG * 8,
                  "reduction scratch fits the bitmap or the z tile");
    double* red = sizeof(uint32_t) * kWG * NW >= sizeof(double) * kWG * 8 ? reinterpret_cast<double*>(bitmap) : Zt;   // [kWG][8]
#pragma unroll
    for (int f0 = 0; f0 < F; f0 += 8) {
      wg_sync();
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (f0 + i < F) red[tid * 8 + i] = acc[f0 + i];
      wg_sync();
      if (mypart == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (f0 + i < F) {
            double s = acc[f0 + i];
            for (int q = 1; q < P; ++q) s += red[(q * Kp + myk) * 8 + i];
            acc[f0 + i] = s;
          }
        }
      }
    }
  }
  if (mypart == 0 && myk < a.K16 * 16) {
#pragma unroll
    for (int f = 0; f < F; ++f) P_out[(size_t)myk * FT + f] = myk < K ? acc[f] : 0.0;
  }
  if (P > 1 && Kp < a.K16 * 16) {       // rows of the partial block between Kp and 16 K16 (K = 17 .. 31 -> Kp = 32 covers them; K <= 16 -> Kp = 16 = 16 K16)
    for (int k = Kp + tid; k < a.K16 * 16; k += kWG)
      for (int f = 0; f < F; ++f) P_out[(size_t)k * FT + f] = 0.0;
  }
  if (tid == 0 && a.write_scalars) {
    double* Ps = P_out + (size_t)a.K16 * 16 * FT;
    Ps[0] = 0.0; Ps[1] = 0.0; Ps[2] = 0.0; Ps[3] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// The same pass with the 256 threads of a workgroup assigned to components IN PROPORTION TO THEIR ROWS (K >= 17, Dz <= 9,
// N >= 2^17).  label_stats_kernel gives every component the same number of threads; a DP-GMM sweep at Kmax = 256 keeps its
// rows on a few dozen components, so one lane in eight works while the others wait for it (N = 1e7, Dz = 8, K = 256: 378 us with
// the rows on 32 components against 239 us for uniformly drawn labels; phase stamps of tools/stamps_label_stats.py: list
// placement 22 %, accumulation 22 %, prefix scan 13 % of the wave time, the rest waiting for the tile).  Here:
//   label_hist_kernel    counts the labels of the whole launch (integer atomics: order-free),
//   label_slots_kernel   hands out the 256 slots: one per NON-EMPTY component, the rest in proportion to the counts,
//   label_stats_slots_kernel  slot (component k, part p of n_k) takes the rows of rank p, p + n_k, .. of ITS component's
//                        ascending list of the tile; the parts of a component are added in part order at the end.
// The result is a function of the label vector alone (the slot table is built from it): run-to-run bit-identical.
// Also new against label_stats_kernel: a row's place in the list is one lookup (per-component prefix of the bitmap's word
// popcounts) instead of a loop over the words below it; rows on an odd stride read with 8-byte loads; bitmap rows padded off
// the 64-byte stride that put every component's words into the same banks.
// What the slot table cannot fix: the labels of a real C3 sweep (tools/c3_label_stats.py) sit on 34 components above 1 % — and on 205
// more with a handful of rows each, so 239 of the 256 slots are taken before any helper is handed out (369 us with this kernel, 372 us
// with label_stats_kernel, N = 1e7).  Taking the slots away from components under 1 row in 1024 and adding their rare rows straight
// into the partial block in global memory was tried: a row costs a dependent L2 round trip per feature there, and the busiest owner
// thread holds every tile's barrier (4.4 ms).  Those rows need accumulators next to the CU — LDS has no room for 205 x 48 doubles
// next to the tile — or a sorted second pass; neither is built.
// Tried and dropped on the way (tools/label_stats_time.py): a kernel that walked the set bits of a component's bitmap
// directly (no prefix scan, no list): its divergent bit loop cost ~1000 cycles per iteration whatever the body (152 against
// 87 us, Dz = 8, K = 256, N = 2e6); and 512-thread workgroups over 1024-row tiles with 256 helper slots: indifferent to the
// skew (309 us either way) but one workgroup per CU, whose five serial phases nothing overlaps (239 us before, uniform labels).
// ------------------------------------------------------------------------------------------
// Measured and not kept: two tiles in flight ahead of the one in LDS — no change (D=8 K=256 N=1e7 246.5 -> 244.7 us; D=9 spills: 271 -> 310 us);
// the next row's index and values fetched under this row's products — slower (246.5 -> 267.1 us).
#ifndef MIMO_LS_PAIRS
#define MIMO_LS_PAIRS 1              // even Dz: rows travel HBM -> registers -> LDS 16 bytes at a time (half the load / store instructions of the staging phase)
#endif
constexpr int kLsSlots = kWG;                  // aux layout (uint32): hist[256] | nparts[256] | first slot[256] | slot table[256]
constexpr int kLsAuxWords = 256 * 4;

__global__ __launch_bounds__(kWG) void label_hist_kernel(const int32_t* __restrict__ labels, int64_t N, int K, uint32_t* __restrict__ aux) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  wg_sync();
  for (int64_t n = (int64_t)blockIdx.x * kWG + threadIdx.x; n < N; n += (int64_t)gridDim.x * kWG) {
    const int l = labels[n];
    if (l >= 0 && l < K) atomicAdd(&h[l], 1u);
  }
  wg_sync();
  if (h[threadIdx.x]) atomicAdd(&aux[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(kWG) void label_slots_kernel(uint32_t* __restrict__ aux, int K) {
  __shared__ uint32_t sc[kWG];
  const int k = threadIdx.x;
  const uint32_t ck = k < K ? aux[k] : 0u;
  sc[k] = ck;
  wg_sync();
  unsigned long long tot = 0ull;
  uint32_t ne = 0u;
  for (int i = 0; i < kWG; ++i) { tot += sc[i]; ne += sc[i] ? 1u : 0u; }
  // one slot per non-empty component + floor(spare count_k / total) of the spare ones (their sum cannot exceed the spare)
  const uint32_t nk = ck ? 1u + (uint32_t)(((unsigned long long)(kLsSlots - ne) * ck) / tot) : 0u;
  wg_sync();
  sc[k] = nk;
  wg_sync();
  uint32_t base = 0u, used = 0u;
  for (int i = 0; i < kWG; ++i) { if (i < k) base += sc[i]; used += sc[i]; }
  aux[256 + k] = nk;
  aux[512 + k] = base;
  wg_sync();
  for (uint32_t j = 0; j < nk; ++j) aux[768 + base + j] = (uint32_t)k | (j << 16);
  if ((uint32_t)k >= used) aux[768 + k] = 0xffffffffu;                 // slots nobody got
}

constexpr int ls_feat(int DZ, int FS) { return FS == 0 ? (DZ + 1) * (DZ + 2) / 2 : FS == 1 ? 2 * DZ + 1 : DZ + 1; }

template <int DZ, int FS = 0>
__global__ __launch_bounds__(kWG, (DZ <= 2 ? 3 : 2)) void label_stats_slots_kernel(const KernelArgs a) {
  constexpr int F = ls_feat(DZ, FS);
#ifdef MIMO_LS_ODD_STRIDE
  constexpr int ZS = DZ | 1;
#else
  constexpr int ZS = DZ <= 2 ? 2 : DZ <= 6 ? 6 : DZ <= 10 ? 10 : DZ <= 14 ? 14 : 18;   // 16-byte aligned rows, odd stride in 16-byte units
#endif
  constexpr int T = kLsTile, NW = T / 32;                  // 512 rows, 16 bitmap words per component
  constexpr int BS = NW + 4, PS = NW + 8;                  // padded row strides of the bitmap (words: 80 bytes) and of its prefix table (u16: 48 bytes)
  constexpr int RPT = T / kWG;                             // 2 rows per thread and tile
  constexpr int ZPT = (T * DZ + kWG - 1) / kWG;
  constexpr bool PAIRS = MIMO_LS_PAIRS && DZ % 2 == 0 && ZS % 2 == 0 && ZPT % 2 == 0;
  __shared__ __align__(16) double Zt[T * ZS > kWG * 8 ? T * ZS : kWG * 8];           // (the epilogue's red[256][8] aliases it)
  __shared__ __align__(16) uint32_t bitmap[kWG * BS];
  __shared__ __align__(16) uint16_t wpre[kWG * PS];                                  // set bits below word w of component k
  __shared__ uint16_t list[T];
  __shared__ int start[kWG];
  __shared__ int cnts[kWG];
  __shared__ int wsum[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int64_t N = a.N;
  const int64_t ntiles = (N + T - 1) / T;
  const uint32_t* aux = a.aux;
  const uint32_t ent = aux[768 + tid];
  const bool live = ent != 0xffffffffu;
  const int myk = live ? (int)(ent & 0xffffu) : 0, mypart = live ? (int)(ent >> 16) : 0;
  const int nparts = live ? (int)aux[256 + myk] : 1;

  double acc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) acc[f] = 0.0;

  // one tile in flight ahead of the one in LDS
  double zr[ZPT];
  int lab[RPT];
  auto load_tile = [&](int64_t t, double (&zd)[ZPT], int (&ld)[RPT]) {
    const int64_t base = t * T * DZ, total = N * DZ;
    if constexpr (PAIRS) {             // element pair e = 2 (tid + 256 i): both in one row (Dz even), 16-byte aligned in HBM and in LDS
      typedef double d2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int i = 0; i < ZPT / 2; ++i) {
        const int e = 2 * (tid + kWG * i);
        const int64_t g = base + e;
        d2 v = d2{0.0, 0.0};
        if (e < T * DZ && g < total) v = *reinterpret_cast<const d2*>(a.Z + g);      // (g even, total even: the pair is inside the data)
        zd[2 * i] = v.x; zd[2 * i + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < ZPT; ++i) {
        const int64_t g = base + tid + (int64_t)kWG * i;
        zd[i] = (tid + kWG * i < T * DZ && g < total) ? a.Z[g] : 0.0;
      }
    }
#pragma unroll
    for (int h = 0; h < RPT; ++h) {
      const int64_t n = t * T + tid + kWG * h;
      const int l = n < N ? a.labels[n] : -1;
      ld[h] = l < K ? l : -1;            // a label outside [0, K) (a caller's vector) is skipped, never an index
    }
  };
  if (blockIdx.x < ntiles) load_tile(blockIdx.x, zr, lab);
  LS_STAMP_INIT

  auto process = [&](int64_t t, double (&zb)[ZPT], int (&lb)[RPT]) {      // tile t from the register set (zb, lb), which is then refilled with the next tile
    wg_sync();                        // the previous tile's readers are done
    LS_STAMP(0)
    if constexpr (PAIRS) {
      typedef double d2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int i = 0; i < ZPT / 2; ++i) {
        const int e = 2 * (tid + kWG * i);
        if (e < T * DZ) { const int r = e / DZ; *reinterpret_cast<d2*>(Zt + r * ZS + (e - r * DZ)) = d2{zb[2 * i], zb[2 * i + 1]}; }
      }
    } else {
#pragma unroll
      for (int i = 0; i < ZPT; ++i) {
        const int e = tid + kWG * i;
        if (e < T * DZ) { const int r = e / DZ; Zt[r * ZS + (e - r * DZ)] = zb[i]; }
      }
    }
    {
      uint4* bm = reinterpret_cast<uint4*>(bitmap + tid * BS);
#pragma unroll
      for (int w = 0; w < NW / 4; ++w) bm[w] = uint4{0u, 0u, 0u, 0u};
    }
    int l01[RPT];
#pragma unroll
    for (int h = 0; h < RPT; ++h) l01[h] = lb[h];
#ifndef MIMO_LS_WHATIF_NOLOAD          // (diagnostic what-if: every tile re-uses the first tile's rows — no HBM traffic)
    if (t + (int64_t)gridDim.x < ntiles) load_tile(t + (int64_t)gridDim.x, zb, lb);
#endif
    LS_STAMP(1)
    wg_sync();
    LS_STAMP(2)
#pragma unroll
    for (int h = 0; h < RPT; ++h)
      if (l01[h] >= 0) atomicOr(&bitmap[l01[h] * BS + ((tid + kWG * h) >> 5)], 1u << (tid & 31));
    wg_sync();
    LS_STAMP(3)
    // rows of component tid, the prefix of its bitmap words, and the exclusive prefix over the components
    int cntk = 0;
    {
      const uint4* bm = reinterpret_cast<const uint4*>(bitmap + tid * BS);
      uint4* wp = reinterpret_cast<uint4*>(wpre + tid * PS);
#pragma unroll
      for (int w8 = 0; w8 < NW / 8; ++w8) {              // eight words in, eight 16-bit prefixes out
        const uint4 v0 = bm[2 * w8], v1 = bm[2 * w8 + 1];
        const uint32_t p0 = cntk;           cntk += __popc(v0.x);
        const uint32_t p1 = cntk;           cntk += __popc(v0.y);
        const uint32_t p2 = cntk;           cntk += __popc(v0.z);
        const uint32_t p3 = cntk;           cntk += __popc(v0.w);
        const uint32_t p4 = cntk;           cntk += __popc(v1.x);
        const uint32_t p5 = cntk;           cntk += __popc(v1.y);
        const uint32_t p6 = cntk;           cntk += __popc(v1.z);
        const uint32_t p7 = cntk;           cntk += __popc(v1.w);
        wp[w8] = uint4{p0 | (p1 << 16), p2 | (p3 << 16), p4 | (p5 << 16), p6 | (p7 << 16)};
      }
    }
    int incl = cntk;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const int v = __shfl_up(incl, sft);
      if (lane >= sft) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    wg_sync();
    int off = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) off += w < wave ? wsum[w] : 0;
    start[tid] = off + incl - cntk;
    cnts[tid] = cntk;
    wg_sync();
    LS_STAMP(4)
    // stable position of each row in its component's list: one prefix lookup + one popcount
#pragma unroll
    for (int h = 0; h < RPT; ++h) {
      const int l = l01[h], row = tid + kWG * h;
      if (l >= 0) {
        const int wq = row >> 5;
        const int rank = (int)wpre[l * PS + wq] + __popc(bitmap[l * BS + wq] & ((1u << (row & 31)) - 1u));
        list[start[l] + rank] = (uint16_t)row;
      }
    }
    wg_sync();
    LS_STAMP(5)
    // slot (component myk, part mypart of nparts): every nparts-th row of the component's list, ascending
    if (live) {
      const int st = start[myk], cmine = cnts[myk];
      for (int p = mypart; p < cmine; p += nparts) {
        const int row = list[st + p];
        const double* zp = Zt + row * ZS;
        double z[DZ];
#pragma unroll
        for (int d = 0; d < DZ; ++d) z[d] = zp[d];
        if constexpr (FS == 0) {
          int f = 0;
#pragma unroll
          for (int i = 0; i < DZ; ++i) {
#pragma unroll
            for (int jx = i; jx < DZ; ++jx) { acc[f] = fma(z[i], z[jx], acc[f]); ++f; }
            acc[f] += z[i]; ++f;
          }
        } else if constexpr (FS == 1) {
#pragma unroll
          for (int i = 0; i < DZ; ++i) { acc[i] = fma(z[i], z[i], acc[i]); acc[DZ + i] += z[i]; }
        } else {
#pragma unroll
          for (int i = 0; i < DZ; ++i) acc[i] += z[i];
        }
        acc[F - 1] += 1.0;
      }
    }
    LS_STAMP(6)
  };
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) process(t, zr, lab);
  LS_STAMP_STORE

  // per-workgroup partial block [16 K16][F16_total]: the slots of a component are neighbours; part 0 adds them in part order, eight
  // features at a time, and writes the component's row; a component without rows in the whole launch has no slot: zeros
  const int FT = a.F16_total;
  const size_t pstride = (size_t)a.K16 * 16 * FT + 4;
  double* P_out = a.partials + (size_t)blockIdx.x * pstride;
  double* red = Zt;                                      // [256][8]
  const bool owner = live && mypart == 0;
#pragma unroll
  for (int f0 = 0; f0 < F; f0 += 8) {
    wg_sync();
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (f0 + i < F) red[tid * 8 + i] = acc[f0 + i];
    wg_sync();
    if (owner) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (f0 + i < F) {
          double s2 = acc[f0 + i];
          for (int q = 1; q < nparts; ++q) s2 += red[(tid + q) * 8 + i];
          acc[f0 + i] = s2;
        }
      }
    }
  }
  if (owner) {
#pragma unroll
    for (int f = 0; f < F; ++f) P_out[(size_t)myk * FT + f] = acc[f];
  }
  if (tid < a.K16 * 16 && (tid >= K || aux[256 + tid] == 0u)) {
    for (int f = 0; f < F; ++f) P_out[(size_t)tid * FT + f] = 0.0;
  }
  if (tid == 0 && a.write_scalars) {
    double* Ps = P_out + (size_t)a.K16 * 16 * FT;
    Ps[0] = 0.0; Ps[1] = 0.0; Ps[2] = 0.0; Ps[3] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// The same pass for Dz = 10 .. 16 (F = 66 .. 153 features: too many accumulators for one thread).  The 256 / Kp threads of
// a component split the FEATURES first — thread slice s takes the rows i = s, s + FP, ... of the upper triangle
// (sum z_i z_j for j >= i, and sum z_i; slice 0 also the count) — and, if threads are left (Kp < 256 / FP), the rows of
// the component's list as in label_stats_kernel.  FP = 4 for K <= 64, 2 for K <= 128 (Dz <= 12).  Tiles of 256 rows.
// ------------------------------------------------------------------------------------------
constexpr int slice_count(int DZ, int FP, int S) {
  int n = S == 0 ? 1 : 0;
  for (int i = S; i < DZ; i += FP) n += DZ - i + 1;
  return n;
}

template <int DZ, int FP, int S, int MAXA>
__device__ __forceinline__ void slice_accumulate(double (&acc)[MAXA], const double (&z)[DZ]) {
  int a = 0;
#pragma unroll
  for (int i = S; i < DZ; i += FP) {
#pragma unroll
    for (int j = i; j < DZ; ++j) { acc[a] = fma(z[i], z[j], acc[a]); ++a; }
    acc[a] += z[i]; ++a;
  }
  if constexpr (S == 0) acc[a] += 1.0;
}

template <int DZ, int FP, int S, int MAXA>
__device__ __forceinline__ void slice_store(const double (&acc)[MAXA], double* __restrict__ Pk) {
  constexpr int F = (DZ + 1) * (DZ + 2) / 2;
  int a = 0;
#pragma unroll
  for (int i = S; i < DZ; i += FP) {
    const int f0 = i * (DZ + 1) - i * (i - 1) / 2;       // feature (i, i); (i, j) follows at f0 + j - i, (i, DZ) at f0 + DZ - i
#pragma unroll
    for (int j = i; j < DZ; ++j) { Pk[f0 + j - i] = acc[a]; ++a; }
    Pk[f0 + DZ - i] = acc[a]; ++a;
  }
  if constexpr (S == 0) Pk[F - 1] = acc[a];
}

template <int DZ, int FP>
__global__ __launch_bounds__(kWG, 2) void label_stats_wide_kernel(const KernelArgs a) {
  constexpr int F = (DZ + 1) * (DZ + 2) / 2;
  constexpr int ZS = DZ <= 10 ? 10 : DZ <= 14 ? 14 : 18;     // 16-byte aligned rows, odd stride in 16-byte units
  constexpr int T = kLsWideTile, NW = T / 32;
  constexpr int ZPT = (T * DZ + kWG - 1) / kWG;
  constexpr int MAXA = slice_count(DZ, FP, 0);                // slice 0 is the largest
  static_assert(FP == 2 || FP == 4, "feature slices per component");
  __shared__ __align__(16) double Zt[T * ZS];
  __shared__ __align__(16) uint32_t bitmap[kWG * NW];
  __shared__ __align__(16) uint16_t list[T];
  __shared__ int start[kWG + 1];
  __shared__ int cnts[kWG];
  __shared__ int wsum[4];
  __shared__ double red[kWG * 8];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the launch takes the components k0 .. k0 + K - 1 of the a.K the labels run over (a window of at most 256 / FP: K > 128 at
  // Dz = 10 .. 16 is two launches of 128, each reads Z once)
  const int k0 = a.k0;
  const int K = a.K - k0 < kWG / FP ? a.K - k0 : kWG / FP;
  const int64_t N = a.N;
  const int64_t ntiles = (N + T - 1) / T;
  int Kp = 1;
  while (Kp < K) Kp <<= 1;
  const int P = kWG / Kp, RP = P / FP;
  const int myk = tid & (Kp - 1), part = tid / Kp, fslice = part % FP, rpart = part / FP;

  double acc[MAXA];
#pragma unroll
  for (int i = 0; i < MAXA; ++i) acc[i] = 0.0;

  double zr[ZPT];
  int lab;
  auto load_tile = [&](int64_t t) {
    const int64_t base = t * T * DZ, total = N * DZ;
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
      const int64_t g = base + tid + (int64_t)kWG * i;
      zr[i] = (tid + kWG * i < T * DZ && g < total) ? a.Z[g] : 0.0;
    }
    const int64_t n = t * T + tid;
    const int l = ((n < N && !a.presort) ? a.labels[n] : -1) - k0;
    lab = (l >= 0 && l < K) ? l : -1;       // outside the window (or outside [0, a.K): a caller's vector): skipped
  };
  if (blockIdx.x < ntiles) load_tile(blockIdx.x);

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    wg_sync();
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
      const int e = tid + kWG * i;
      if (e < T * DZ) { const int r = e / DZ; Zt[r * ZS + (e - r * DZ)] = zr[i]; }
    }
    int st, cmine;
    if (a.presort) {                   // (uniform) the tile was ranked once for all the launches: label_tile_sort_kernel
      const uint16_t* sg = a.sort_start + (size_t)t * 257 + (k0);
      const bool mine = myk < K;
      const int s0 = mine ? (int)sg[myk] : 0, s1 = mine ? (int)sg[myk + 1] : 0;
      if (tid < T / 2) reinterpret_cast<uint32_t*>(list)[tid] = reinterpret_cast<const uint32_t*>(a.sort_list + (size_t)t * T)[tid];
      if (t + gridDim.x < ntiles) load_tile(t + gridDim.x);
      st = s0; cmine = s1 - s0;
      wg_sync();
    } else {
      {
        uint4* bm = reinterpret_cast<uint4*>(bitmap + tid * NW);
  #pragma unroll
        for (int w = 0; w < NW / 4; ++w) bm[w] = uint4{0u, 0u, 0u, 0u};
      }
      const int l0 = lab;
      if (t + gridDim.x < ntiles) load_tile(t + gridDim.x);
      wg_sync();
      if (l0 >= 0) atomicOr(&bitmap[l0 * NW + (tid >> 5)], 1u << (tid & 31));
      wg_sync();
      int cntk = 0;
      {
        const uint4* bm = reinterpret_cast<const uint4*>(bitmap + tid * NW);
  #pragma unroll
        for (int w = 0; w < NW / 4; ++w) {
          const uint4 v = bm[w];
          cntk += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        }
      }
      int incl = cntk;
  #pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int v = __shfl_up(incl, s);
        if (lane >= s) incl += v;
      }
      if (lane == 63) wsum[wave] = incl;
      wg_sync();
      int off = 0;
  #pragma unroll
      for (int w = 0; w < 4; ++w) off += w < wave ? wsum[w] : 0;
      start[tid] = off + incl - cntk;
      cnts[tid] = cntk;
      wg_sync();
      if (l0 >= 0) {
        const uint32_t* bm = bitmap + l0 * NW;
        const int wq = tid >> 5;
        int rank = __popc(bm[wq] & ((1u << (tid & 31)) - 1u));
        for (int w = 0; w < wq; ++w) rank += __popc(bm[w]);
        list[start[l0] + rank] = (uint16_t)tid;
      }
      wg_sync();
      st = start[myk]; cmine = cnts[myk];
    }
    for (int p = rpart; p < cmine; p += RP) {
      const int row = list[st + p];
      const double* zp = Zt + row * ZS;
      double z[DZ];
#pragma unroll
      for (int d = 0; d < DZ; ++d) z[d] = zp[d];
      switch (fslice) {      // (uniform per wave when Kp >= 64)
        case 0: slice_accumulate<DZ, FP, 0, MAXA>(acc, z); break;
        case 1: slice_accumulate<DZ, FP, 1, MAXA>(acc, z); break;
        case 2: if constexpr (FP == 4) slice_accumulate<DZ, FP, 2, MAXA>(acc, z); break;
        default: if constexpr (FP == 4) slice_accumulate<DZ, FP, 3, MAXA>(acc, z); break;
      }
    }
  }

  const int FT = a.F16_total;
  const size_t pstride = (size_t)a.K16 * 16 * FT + 4;
  double* P_out = a.partials + (size_t)blockIdx.x * pstride;
  if (RP > 1) {          // add the row parts of every (component, slice) in part order, eight accumulators at a time
#pragma unroll
    for (int f0 = 0; f0 < MAXA; f0 += 8) {
      wg_sync();
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (f0 + i < MAXA) red[tid * 8 + i] = acc[f0 + i];
      wg_sync();
      if (rpart == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (f0 + i < MAXA) {
            double s = acc[f0 + i];
            for (int qq = 1; qq < RP; ++qq) s += red[((qq * FP + fslice) * Kp + myk) * 8 + i];
            acc[f0 + i] = s;
          }
        }
      }
    }
  }
  // rows of the partial block without a component (the first window's launch)
  if (k0 == 0)
    for (int k = a.K + tid; k < a.K16 * 16; k += kWG)
      for (int f = 0; f < F; ++f) P_out[(size_t)k * FT + f] = 0.0;
  if (rpart == 0 && myk < K) {
    double* Pk = P_out + (size_t)(k0 + myk) * FT;
    switch (fslice) {
      case 0: slice_store<DZ, FP, 0, MAXA>(acc, Pk); break;
      case 1: slice_store<DZ, FP, 1, MAXA>(acc, Pk); break;
      case 2: if constexpr (FP == 4) slice_store<DZ, FP, 2, MAXA>(acc, Pk); break;
      default: if constexpr (FP == 4) slice_store<DZ, FP, 3, MAXA>(acc, Pk); break;
    }
  }
  if (tid == 0 && a.write_scalars && k0 == 0) {
    double* Ps = P_out + (size_t)a.K16 * 16 * FT;
    Ps[0] = 0.0; Ps[1] = 0.0; Ps[2] = 0.0; Ps[3] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// The ranking of a tile's labels — bitmap per component, popcount ranks, prefix over the components, the rows in component order —
// is the same in every launch of the windowed label statistics (two launches at Dz = 10 .. 16, K > 128), and the one-pass kernel
// below takes its rows from it: it runs ONCE here, and the consumers read the list (2 bytes per row) and the per-component starts
// (257 x 2 bytes per tile) instead — two workgroup barriers per tile instead of six.  T = the consumers' tile (256 rows).
// ------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kWG) void label_tile_sort_kernel(const int32_t* __restrict__ labels, int64_t N, int K,
                                                              uint16_t* __restrict__ list_out, uint16_t* __restrict__ start_out) {
  constexpr int NW = T / 32;
  __shared__ __align__(16) uint32_t bitmap[kWG * NW];
  __shared__ int start[kWG + 1];
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = (N + T - 1) / T;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t n = t * T + tid;
    int l0 = (tid < T && n < N) ? labels[n] : -1;
    if (l0 >= K) l0 = -1;
    {
      uint4* bm = reinterpret_cast<uint4*>(bitmap + tid * NW);
#pragma unroll
      for (int w = 0; w < NW / 4; ++w) bm[w] = uint4{0u, 0u, 0u, 0u};
    }
    wg_sync();
    if (l0 >= 0) atomicOr(&bitmap[l0 * NW + (tid >> 5)], 1u << (tid & 31));
    wg_sync();
    int cntk = 0;
    {
      const uint4* bm = reinterpret_cast<const uint4*>(bitmap + tid * NW);
#pragma unroll
      for (int w = 0; w < NW / 4; ++w) {
        const uint4 v = bm[w];
        cntk += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
      }
    }
    int incl = cntk;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int v = __shfl_up(incl, s);
      if (lane >= s) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    wg_sync();
    int off = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) off += w < wave ? wsum[w] : 0;
    start[tid] = off + incl - cntk;
    if (tid == kWG - 1) start[kWG] = off + incl;
    wg_sync();
    uint16_t* so = start_out + (size_t)t * 257;
    so[tid] = (uint16_t)start[tid];
    if (tid == 0) so[256] = (uint16_t)start[kWG];
    if (l0 >= 0) {
      const uint32_t* bm = bitmap + l0 * NW;
      const int wq = tid >> 5;
      int rank = __popc(bm[wq] & ((1u << (tid & 31)) - 1u));
      for (int w = 0; w < wq; ++w) rank += __popc(bm[w]);
      list_out[(size_t)t * T + start[l0] + rank] = (uint16_t)tid;
    }
    wg_sync();                           // bitmap / start are rewritten by the next tile
  }
}
// rank the tiles of a.labels once for the windowed launches or the one-pass kernel
static hipError_t launch_label_tile_sort(const KernelArgs& a, int grid, hipStream_t stream) {
  if (!a.sort_list || !a.sort_start) return hipErrorInvalidValue;
  hipLaunchKernelGGL(label_tile_sort_kernel<kLsWideTile>, dim3(grid), dim3(kWG), 0, stream, a.labels, a.N, a.K, a.sort_list, a.sort_start);
  return hipGetLastError();
}
static bool label_presort_on() {
  static const bool on = [] { const char* e = getenv("MIMO_LABEL_PRESORT"); return !e || atoi(e) != 0; }();   // tuning knob
  return on;
}

// ------------------------------------------------------------------------------------------
// Label statistics from the ranked tiles in ONE pass over Z whatever Dz is (Dz = 17 .. 32, and K > 128 from Dz = 15), on the
// matrix cores.  A workgroup walks the components one after the other: for component k the rows of the workgroup's tile range are
// looked up in the ranked tiles (label_tile_sort_kernel: list + starts) and gathered 64 at a time into LDS.  The statistics of ONE
// component's rows are a Gram matrix, z~' z~ over those rows (z~ = [z, 1]: second moments, sums and the count are its entries), and
// the rows arrive sorted by component: per group of four rows one v_mfma_f64_16x16x4_f64 per 16 x 16 tile of the upper triangle
// (1 tile up to Dz = 15, 3 up to Dz = 31, 6 at Dz = 32), operands straight from the gathered rows in LDS — 1 - 2 reads of 512 bytes
// per matrix instruction, 1.5 KB per row at Dz = 32 (a VALU kernel that gave every thread up to three features read two factors per
// product from LDS, 9 KB per row at Dz = 32, and was bound by the LDS pipe at 1.3 - 1.6 TB/s of Z).  Each wave owns tiles of the
// triangle (no cross-wave sum); a component's accumulators go to the partial block when its last row is done (first range writes,
// later ranges add), rows of a group that belong to the next component are masked to zero.  Rows are taken in ascending order,
// ranges in ascending order per workgroup, the blocks are reduced in block order: run-to-run bit-identical.
// ------------------------------------------------------------------------------------------
constexpr int kSortedRange = 80;                 // tiles (of 256 rows) per range at most (N = 1e7 on 512 workgroups: 77)
#ifndef MIMO_GRAM_WHATIF
#define MIMO_GRAM_WHATIF 0           // diagnostic builds: 1 no batches (bookkeeping only), 2 no flushes to the partial block (results are wrong)
#endif
#ifndef MIMO_GRAM_BATCH
#define MIMO_GRAM_BATCH 0            // 0: 64 rows per step (128 measured 4 - 6 % faster at two workgroups per CU, but costs the third and fourth)
#endif
// ranges of at most 40 tiles (20 KB of ids) and 64-row batches: 37 - 45 KB of LDS, four (three at Dz = 32) workgroups per CU — the
// pass has three phases of comparable length that one workgroup runs one after the other (range bookkeeping, gather + staging,
// products: what-if builds, profiles/r04_label_stats_gram.txt), so it takes co-resident workgroups to overlap them
// (measured, N = 1e7, two -> four workgroups per CU: Dz=20 K=64 981 -> 779 us, Dz=24 K=200 1149 -> 975, Dz=28 K=16 1052 -> 812, Dz=31 K=128
//  1190 -> 1068 with three; Dz = 32 — six tiles, 45 KB, 1.2 MB of partial block per workgroup at K = 256 — loses with three
//  (K=128 1672 -> 1900, K=256 1858 -> 2400) and keeps two workgroups over ranges of 80 tiles)
constexpr int gram_range(int DZ) { return DZ <= 31 ? 40 : 80; }
constexpr int gram_wgs_per_cu(int DZ) { return DZ <= 31 ? 4 : 2; }      // (registers: 85 .. 133; four per CU cap them at 128: Dz=31 1437 us with three, 1068 with four)
template <int DZ>
__global__ __launch_bounds__(kWG, gram_wgs_per_cu(DZ)) void label_stats_gram_kernel(const KernelArgs a, int R) {
  constexpr int F = (DZ + 1) * (DZ + 2) / 2;
  constexpr int TT = (DZ + 1 + 15) / 16;                               // 16-wide tiles per side of the Gram matrix of z~
  constexpr int NTL = TT * (TT + 1) / 2;                               // tiles of the upper triangle: 1, 3 or 6
  constexpr int TPW = (NTL + 3) / 4;                                   // tiles per wave: 1, 1 or 2
  constexpr int T = kLsWideTile, B = MIMO_GRAM_BATCH > 0 ? MIMO_GRAM_BATCH : 64;    // rows gathered per step
  constexpr int ZS = 16 * TT + 1;                                      // rows [z, 1, 0 ..] padded to whole tiles; odd stride
  constexpr int GPT = (B * DZ + kWG - 1) / kWG;                        // gathered elements per thread and batch
  __shared__ __align__(16) double zbuf[B * ZS];
  __shared__ uint16_t ids[gram_range(DZ) * T];
  __shared__ int kbase[kWG + 1];
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int K = a.K;
  const int64_t N = a.N;
  const int64_t ntiles = (N + T - 1) / T, nranges = (ntiles + R - 1) / R;
  const int FT = a.F16_total;
  const size_t pstride = (size_t)a.K16 * 16 * FT + 4;
  double* P = a.partials + (size_t)blockIdx.x * pstride;

  // this wave's tiles (ti <= tj) of the triangle, in row-major order of the triangle: tile index wave + 4 i
  int ti[TPW], tj[TPW];
  bool has[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = wave + 4 * i;
    has[i] = t < NTL;
    int r = 0, t0 = 0;
    while (r + 1 < TT && t0 + (TT - r) <= t) { t0 += TT - r; ++r; }
    ti[i] = r; tj[i] = has[i] ? r + (t - t0) : r;
  }
  for (int e = tid; e < a.K16 * 16 * FT; e += kWG) {                  // rows / columns of the block no accumulator reaches
    const int k = e / FT, f = e - k * FT;
    if (k >= K || f >= F) P[e] = 0.0;
  }
  if (tid == 0 && a.write_scalars) { double* Ps = P + (size_t)a.K16 * 16 * FT; Ps[0] = 0.0; Ps[1] = 0.0; Ps[2] = 0.0; Ps[3] = 0.0; }
  for (int e = tid; e < B * ZS; e += kWG) zbuf[e] = 0.0;              // the padding columns stay zero: written once

  d4 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  // component k is complete: this wave's tiles -> the partial block.  Register r of lane (q, j) of tile (ti, tj) is the entry
  // (a, b) = (16 ti + 4 r + q, 16 tj + j) of z~' z~: feature (a, b) for a <= b <= Dz
  auto flush = [&](int k, bool first) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if (has[i]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ra = 16 * ti[i] + 4 * r + q, cb = 16 * tj[i] + j;
          if (ra <= cb && cb <= DZ) {
            double* dst = P + (size_t)k * FT + (ra * (DZ + 1) - ra * (ra - 1) / 2 + (cb - ra));
            *dst = first ? acc[i][r] : *dst + acc[i][r];
          }
        }
      }
      acc[i] = d4{0.0, 0.0, 0.0, 0.0};
    }
  };

  bool first = true;
  for (int64_t rg = blockIdx.x; rg < nranges; rg += gridDim.x) {
    const int64_t t0 = rg * R;
    const int nt = (int)(ntiles - t0 < R ? ntiles - t0 : R);
    // ---- the rows of the range by component (thread k = component k): counts, prefix over the components, ids
    wg_sync();
    int cntk = 0;
    if (tid < K) {
#pragma unroll 8
      for (int t = 0; t < nt; ++t) {
        const uint16_t* sg = a.sort_start + (size_t)(t0 + t) * 257 + tid;
        cntk += (int)sg[1] - (int)sg[0];
      }
    }
    int incl = cntk;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const int v = __shfl_up(incl, sft);
      if (lane >= sft) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    wg_sync();
    int off = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) off += w < wave ? wsum[w] : 0;
    int o = off + incl - cntk;
    kbase[tid] = o;
    if (tid == kWG - 1) kbase[kWG] = off + incl;
    if (tid < K)
      for (int tb = 0; tb < nt; tb += 4) {
        int s0[4], c[4];
        uint16_t l0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = tb + i < nt ? tb + i : nt - 1;
          const uint16_t* sg = a.sort_start + (size_t)(t0 + t) * 257 + tid;
          s0[i] = sg[0]; c[i] = tb + i < nt ? (int)sg[1] - s0[i] : 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = tb + i < nt ? tb + i : nt - 1;
          l0[i] = c[i] > 0 ? a.sort_list[(size_t)(t0 + t) * T + s0[i]] : (uint16_t)0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = tb + i;
          if (c[i] > 0) {
            ids[o++] = (uint16_t)((t << 8) | l0[i]);
            const uint16_t* lg = a.sort_list + (size_t)(t0 + t) * T + s0[i];
            for (int m = 1; m < c[i]; ++m) ids[o++] = (uint16_t)((t << 8) | lg[m]);
          }
        }
      }
    wg_sync();
    if (first) {                                         // components without a row in the workgroup's first range: zero rows
      for (int e = tid; e < K * F; e += kWG) {
        const int k = e / F, f = e - k * F;
        if (kbase[k + 1] == kbase[k]) P[(size_t)k * FT + f] = 0.0;
      }
    }
#if MIMO_GRAM_WHATIF == 1
    const int nrows = 0;                                 // (diagnostic: ranges, counts and id lists only)
#else
    const int nrows = kbase[kWG];
#endif
    double gz[2][GPT];                                   // two batches in flight ahead of the one in LDS
    auto fetch = [&](int pos, double (&g)[GPT]) {
      const int nb = nrows - pos < B ? nrows - pos : B;
#pragma unroll
      for (int i = 0; i < GPT; ++i) {
        const int e = tid + kWG * i, r = e / DZ, col = e - r * DZ;
        double v = 0.0;
        if (e < B * DZ && r < nb) {
          const int id = ids[pos + r];
          const int64_t n = (t0 + (id >> 8)) * T + (id & 255);
          v = a.Z[n * DZ + col];
        }
        g[i] = v;
      }
    };
    if (nrows > 0) fetch(0, gz[0]);
    if (nrows > B) fetch(B, gz[1]);
    int k = 0;
    auto step = [&](int pos, double (&g)[GPT]) {
      const int nb = nrows - pos < B ? nrows - pos : B;
#pragma unroll
      for (int i = 0; i < GPT; ++i) {
        const int e = tid + kWG * i, r = e / DZ, col = e - r * DZ;
        if (e < B * DZ) zbuf[r * ZS + col] = g[i];
      }
      for (int e = tid; e < B; e += kWG) zbuf[e * ZS + DZ] = 1.0;
      wg_sync();
      if (pos + 2 * B < nrows) fetch(pos + 2 * B, g);
      int r = 0;
      while (r < nb) {                                   // (uniform control flow: kbase is the same for every thread)
        while (kbase[k + 1] <= pos + r) ++k;
        const int kend = kbase[k + 1] - pos;
        const int rend = kend < nb ? kend : nb;
        // groups of four rows of component k; the lanes whose row lies past the segment read zeros
        // (U groups per iteration, all their operand reads in flight before the first product: one group at a time is an LDS round
        //  trip + a dependent matrix instruction per four rows — ~200 cycles whatever Dz is, measured as a pass whose time did not
        //  depend on Dz: 0.97 - 1.2 ms per 1e7 rows from Dz = 17 to 31)
        constexpr int U = 4;
        for (; r < rend; r += 4 * U) {
          double av[U][TPW], bv[U][TPW];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int rr = r + 4 * u + q;
            const bool inside = rr < rend;
            const double* zr = zbuf + (inside ? rr : 0) * ZS + j;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
              av[u][i] = inside ? zr[16 * ti[i]] : 0.0;
              bv[u][i] = inside ? zr[16 * tj[i]] : 0.0;
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < TPW; ++i)
              if (has[i]) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][i], bv[u][i], acc[i], 0, 0, 0);
        }
        r = rend;
#if MIMO_GRAM_WHATIF != 2
        if (kend <= nb) flush(k, first);                 // component k is complete
#endif
      }
      wg_sync();
    };
    for (int pos = 0; pos < nrows; pos += 2 * B) {
      step(pos, gz[0]);
      if (pos + B < nrows) step(pos + B, gz[1]);
    }
    first = false;
  }
  if (first) {                                           // a workgroup without a range: an all-zero block
    for (int e = tid; e < K * FT; e += kWG) {
      const int k = e / FT, f = e - k * FT;
      if (f < F) P[(size_t)k * FT + f] = 0.0;
    }
  }
}

static int g_sorted_range_cap = kSortedRange;
void set_sorted_range_cap(int tiles) { g_sorted_range_cap = tiles < 1 || tiles > kSortedRange ? kSortedRange : tiles; }
template <int DZ>
static hipError_t launch_sorted(const KernelArgs& a, int grid, hipStream_t stream) {
  hipError_t e = launch_label_tile_sort(a, grid, stream);
  if (e != hipSuccess) return e;
  const int64_t ntiles = (a.N + kLsWideTile - 1) / kLsWideTile;
  int R = (int)((ntiles + grid - 1) / (grid > 0 ? grid : 1));            // one range per workgroup where the cap allows (no second round for a few)
  R = R < 1 ? 1 : R > g_sorted_range_cap ? g_sorted_range_cap : R;      // (mimo_tune "sorted_range" lowers the cap: several ranges per workgroup at test sizes)
  hipLaunchKernelGGL(label_stats_gram_kernel<DZ>, dim3(grid), dim3(kWG), 0, stream, a, R > gram_range(DZ) ? gram_range(DZ) : R);
  return hipGetLastError();
}

// The one decision about the statistics stage of a label pass: which kernel closes it, in how many launches, whether it takes the ranked
// tiles, what its grid is sized from.  launch_label_stats and label_stats_grid below and the C-ABI layer (presort buffers, the histogram
// fused into the label kernel, mimo_plan's description) read this value.  structure: MIMO_STRUCT_*.  In order of precedence:
//   Slots         K = 17 .. 256 at Dz <= 9 with at least 2^17 rows, any structure (MIMO_LABEL_STATS_SLOTS=0: the round-2 kernel, tuning knob)
//   Ranked        full map, Dz >= 17; and K > 128 from Dz = 15 (against the two windows of label_stats_wide_kernel, N = 2e6, ms: Dz=16 K=256
//                 0.36 -> 0.27, K=192 0.32 -> 0.25, Dz=15 K=160 0.26 -> 0.24; Dz=14 K=200 0.23 -> 0.25 and Dz=13 K=256 0.25 -> 0.26 stay windowed)
//   PerComponent  reduced maps up to Dz = 16 (at most 2 Dz + 1 accumulators), the full map up to Dz = 9
//   Windows       full map, Dz = 10 .. 16: four feature slices per component up to K = 64, two beyond; 128 components per launch
LabelStatsPlan label_stats_plan(int K, int D, int structure, int64_t N) {
  static const bool slots_on = [] { const char* e = getenv("MIMO_LABEL_STATS_SLOTS"); return !e || atoi(e) != 0; }();
  LabelStatsPlan p = {LabelStatsPlan::None, 1, 0, D <= (structure != 0 ? 10 : 9) ? kLsTile : kLsWideTile, 2, ""};
  if (K < 1 || K > 256 || D < 1 || D > kMaxD) return p;
  if (slots_on && K >= 17 && D <= 9 && N >= (1 << 17)) {
    p.kind = LabelStatsPlan::Slots; p.name = "label_slots_kernel + label_stats_slots_kernel";
    if (D <= 2) p.per_cu = 3;                    // (52 KB of LDS, <= 88 registers: three per CU)
  } else if (structure == 0 && (D >= 17 || (D >= 15 && K > 128))) {
    p.kind = LabelStatsPlan::Ranked; p.name = "label_tile_sort_kernel + label_stats_gram_kernel";
    p.ranked = 2; p.per_cu = gram_wgs_per_cu(D);
  } else if (D <= (structure != 0 ? 16 : 9)) {
    p.kind = LabelStatsPlan::PerComponent; p.name = "label_stats_kernel";
  } else if (structure == 0 && D <= 16) {
    p.kind = LabelStatsPlan::Windows; p.name = "label_stats_wide_kernel";
    p.launches = (K + 127) / 128; p.ranked = K > 128 ? 1 : 0;
  }
  return p;
}
bool label_stats_covers(int K, int D, int structure) {
  return K >= rowwave_min_k() && label_stats_plan(K, D, structure, INT64_MAX).kind != LabelStatsPlan::None;
}
size_t label_stats_aux_words() { return kLsAuxWords; }
// (the grid fixes the number of partial blocks, and with it the order of the sums)
int label_stats_grid(const LabelStatsPlan& p, int64_t N, int num_cu) {
  const int64_t tiles = (N + p.tile - 1) / p.tile;
  int64_t g = (int64_t)num_cu * p.per_cu;
  if (g > tiles) g = tiles;
  return (int)(g < 1 ? 1 : g);
}

template <int FS>
static void (*pick_label_stats_slots(int D))(const KernelArgs) {
  switch (D) {
    case 1: return label_stats_slots_kernel<1, FS>;   case 2: return label_stats_slots_kernel<2, FS>;
    case 3: return label_stats_slots_kernel<3, FS>;   case 4: return label_stats_slots_kernel<4, FS>;
    case 5: return label_stats_slots_kernel<5, FS>;   case 6: return label_stats_slots_kernel<6, FS>;
    case 7: return label_stats_slots_kernel<7, FS>;   case 8: return label_stats_slots_kernel<8, FS>;
    case 9: return label_stats_slots_kernel<9, FS>;
  }
  return nullptr;
}

template <int FS>
static void (*pick_label_stats_struct(int D))(const KernelArgs) {
  switch (D) {
    case 1: return label_stats_kernel<1, FS>;   case 2: return label_stats_kernel<2, FS>;
    case 3: return label_stats_kernel<3, FS>;   case 4: return label_stats_kernel<4, FS>;
    case 5: return label_stats_kernel<5, FS>;   case 6: return label_stats_kernel<6, FS>;
    case 7: return label_stats_kernel<7, FS>;   case 8: return label_stats_kernel<8, FS>;
    case 9: return label_stats_kernel<9, FS>;
    default: break;
  }
  if constexpr (FS != 0) {          // the reduced maps reach Dz = 16 with one thread per component (the full map: wide kernel)
    switch (D) {
      case 10: return label_stats_kernel<10, FS>; case 11: return label_stats_kernel<11, FS>;
      case 12: return label_stats_kernel<12, FS>; case 13: return label_stats_kernel<13, FS>;
      case 14: return label_stats_kernel<14, FS>; case 15: return label_stats_kernel<15, FS>;
      case 16: return label_stats_kernel<16, FS>;
    }
  }
  return nullptr;
}

// zero the histogram in front of a label kernel that counts its own labels (KernelArgs::fuse_hist)
hipError_t launch_label_hist_reset(const KernelArgs& a, hipStream_t stream) {
  return a.aux ? hipMemsetAsync(a.aux, 0, 256 * sizeof(uint32_t), stream) : hipErrorInvalidValue;
}

// structure: 0 full, 1 diagonal, 2 linear (MIMO_STRUCT_*)
hipError_t launch_label_stats(const KernelArgs& a, int structure, int grid, hipStream_t stream) {
  typedef void (*fn_t)(const KernelArgs);
  const LabelStatsPlan p = label_stats_plan(a.K, a.D, structure, a.N);
  fn_t fn = nullptr;
  switch (p.kind) {
  case LabelStatsPlan::None: break;
  case LabelStatsPlan::Slots:
    if (!a.aux) return hipErrorInvalidValue;
    fn = structure == 1 ? pick_label_stats_slots<1>(a.D) : structure == 2 ? pick_label_stats_slots<2>(a.D) : pick_label_stats_slots<0>(a.D);
    if (!fn) return hipErrorInvalidValue;
    if (!a.fuse_hist) {       // (else: the label kernel of this pass counted them, launch_label_hist_reset ran in front of it)
      hipError_t e = hipMemsetAsync(a.aux, 0, 256 * sizeof(uint32_t), stream);
      if (e != hipSuccess) return e;
      int hg = (int)((a.N + kWG * 16 - 1) / (kWG * 16));
      if (hg > 1024) hg = 1024;
      hipLaunchKernelGGL(label_hist_kernel, dim3(hg), dim3(kWG), 0, stream, a.labels, a.N, a.K, a.aux);
    }
    hipLaunchKernelGGL(label_slots_kernel, dim3(1), dim3(kWG), 0, stream, a.aux, a.K);
    break;
  case LabelStatsPlan::Ranked:          // (the only kernel of its shapes: without the presort buffers, launch_label_tile_sort's error)
    switch (a.D) {
#define MIMO_SD(d) case d: return launch_sorted<d>(a, grid, stream);
      MIMO_SD(10) MIMO_SD(11) MIMO_SD(12) MIMO_SD(13) MIMO_SD(14) MIMO_SD(15) MIMO_SD(16) MIMO_SD(17) MIMO_SD(18) MIMO_SD(19) MIMO_SD(20)
      MIMO_SD(21) MIMO_SD(22) MIMO_SD(23) MIMO_SD(24) MIMO_SD(25) MIMO_SD(26) MIMO_SD(27) MIMO_SD(28) MIMO_SD(29) MIMO_SD(30) MIMO_SD(31) MIMO_SD(32)
#undef MIMO_SD
    }
    break;
  case LabelStatsPlan::PerComponent:
    fn = structure == 1 ? pick_label_stats_struct<1>(a.D) : structure == 2 ? pick_label_stats_struct<2>(a.D) : pick_label_stats_struct<0>(a.D);
    break;
  case LabelStatsPlan::Windows: {
    static const fn_t wide4[7] = {label_stats_wide_kernel<10, 4>, label_stats_wide_kernel<11, 4>, label_stats_wide_kernel<12, 4>,
                                  label_stats_wide_kernel<13, 4>, label_stats_wide_kernel<14, 4>, label_stats_wide_kernel<15, 4>,
                                  label_stats_wide_kernel<16, 4>};
    static const fn_t wide2[7] = {label_stats_wide_kernel<10, 2>, label_stats_wide_kernel<11, 2>, label_stats_wide_kernel<12, 2>,
                                  label_stats_wide_kernel<13, 2>, label_stats_wide_kernel<14, 2>, label_stats_wide_kernel<15, 2>,
                                  label_stats_wide_kernel<16, 2>};
    fn = a.K <= 64 ? wide4[a.D - 10] : wide2[a.D - 10];
    if (p.launches < 2) break;
    // windows of 128 components, one launch each into the same partial block
    const bool presort = label_presort_on() && a.sort_list && a.sort_start;
    if (presort) {
      hipError_t e = launch_label_tile_sort(a, grid, stream);
      if (e != hipSuccess) return e;
    }
    for (int k0 = 0; k0 < a.K; k0 += 128) {
      KernelArgs w = a;
      w.presort = presort ? 1 : 0;
      w.k0 = k0;
      hipLaunchKernelGGL(fn, dim3(grid), dim3(kWG), 0, stream, w);
    }
    return hipGetLastError();
  }
  }
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kWG), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mimo