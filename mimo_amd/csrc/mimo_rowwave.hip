// gfx950 row-owner kernels of the Gibbs sweep at K <= 256 (BASELINE config C3: DP-GMM with Kmax = 256, D = 8) and of the
// mean-field pass at K <= 64, Dz <= 9:
//
//   gibbs_rowwave_kernel<KB, NS4>   label pass:  l = Theta . Phi'  ->  inverse-CDF draw, nothing but the labels leaves
//   gibbs_stream_kernel<KB, ZI>     the same with Theta streamed through LDS where it does not fit (up to Dz = 32)
//   vi_rowwave_kernel<KB, NS4>      softmax + weighted statistics on the same row-owner waves
//
// (the statistics of the labels just drawn: mimo_label_stats.hip)
//
// Why not the fused tile kernel (mimo_kernels.hip, RBW = 4) for this shape: there a workgroup shares one 32-row tile,
// the l tile goes through LDS twice (66 KB per workgroup), four barriers per tile, and the 96 accumulator registers
// of the statistics push the kernel into scratch (C3: 8.1 ms, 42 % of the float64 matrix peak).  Here the roles are
// swapped — "row-owner" waves:
//
//   * Theta (K x F16, 98 KB at K = 256, Dz = 8) is loaded into LDS ONCE per workgroup and only read afterwards;
//   * a wave owns 16 data rows per step: B operand Phi[row j][4s + q] is built on the fly from the wave's own z rows
//     (2 LDS reads + 1 product per contraction step, shared by the K/16 MFMAs of the step), A operand = Theta slices
//     straight from LDS, accumulators = the l values of ALL components of the wave's 16 rows (4 K/16 doubles per lane);
//   * the components are permuted in the operand image so that lane (q, j) ends up with a CONTIGUOUS quarter of the
//     components of row j: max, exp, cumulative sums and the inverse-CDF count run in registers, three cross-lane
//     steps per row, no LDS round trip and no workgroup barrier anywhere in the loop.
//
// Reference behaviour reproduced: mimo/mixtures/gmm.py:227-237 (resample_labels), mimo/utils/stats.py:8-21
// (label = #{k : u cum_K > cum_k}).
#include "mimo_device.h"

#include <cstdlib>
#include <type_traits>

namespace mimo {
// Lane exchanges of the per-row reductions in registers (mimo_device.h) — but for the instantiations {KB, NS4} the register form
// costs an occupancy step (label kernel: 168 -> 170 VGPRs, three workgroups' worth of waves -> two) or VGPRs (softmax kernel):
// those keep __shfl_xor, same bits (profiles/r08_c2_lane_exchange.txt).  No instantiation of the streamed label kernel moves.
// (Lists from a `make resources` comparison of both forms: see fused_lane_regs in mimo_kernels.hip for how to regenerate them.)
constexpr bool gibbs_rowwave_lane_regs(int KB, int NS4) { return !((KB == 4 && NS4 == 9) || (KB == 6 && NS4 == 6) || (KB == 8 && NS4 == 5)); }
constexpr bool vi_rowwave_lane_regs(int KB, int NS4) { return !((KB == 2 && NS4 == 1) || (KB == 4 && NS4 == 3)); }

// ------------------------------------------------------------------------------------------
// Label pass.  KB = row blocks (16 components each) the accumulators cover; K <= 16 KB.
// Operand image (host, ThetaRowOwner of mimo_theta.h): slice e = s KB + rb, lane (i = lane & 15, kk = lane >> 4) holds
// Theta[comp(i, rb)][4 s + kk] with comp(i, rb) = (i & 3) V + 4 rb + (i >> 2), V = 4 KB: output lane (q, j)
// register r of row block rb (= A-row q + 4 r) is component q V + 4 rb + r of data row j.
// ------------------------------------------------------------------------------------------
constexpr int kRowWaveWG = 512;     // 8 wavefronts: two per SIMD (the accumulators need 8 KB VGPRs per lane)

template <int KB, int NS4>
__global__ __launch_bounds__(kRowWaveWG, 1) void gibbs_rowwave_kernel(const KernelArgs a) {
  constexpr int V = 4 * KB;          // components per lane
  constexpr int NCH = KB / 2;        // chunks of 8 components (two row blocks) for the cumulative sums
  static_assert(KB % 2 == 0 && KB >= 2 && KB <= 16, "row blocks per wave");
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NS = 4 * NS4;                        // contraction steps (F16 / 4): compile-time, the step loop is straight-line
  const int ZS = a.ZS;
  double* Th = reinterpret_cast<double*>(smem);      // [(NS KB + 4)][64]   (+4: the operand prefetch runs past the end)
  double* etab = Th + (size_t)(NS * KB + 4) * 64;    // [kExpTab]
  double* Zall = etab + kExpTab;                     // [8 waves][16][ZS]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, j = lane & 15;
  const int D = a.D, K = a.K;
  const int64_t N = a.N;
  double* Zw = Zall + (size_t)wave * 16 * ZS;

  for (int e = tid; e < NS * KB * 64; e += kRowWaveWG) Th[e] = a.theta[e];
  for (int e = tid; e < 4 * 64; e += kRowWaveWG) Th[NS * KB * 64 + e] = 0.0;
  for (int e = tid; e < kExpTab; e += kRowWaveWG) etab[e] = exp_tab_entry_c(e);
  // a.fuse_hist: the histogram of the labels this launch draws, for the slot table of label_stats_slots_kernel — 16 LDS atomics per
  // wave step here instead of a pass of its own over the labels (label_hist_kernel: 36 us at N = 1e7, same-address atomics of skewed labels)
  __shared__ uint32_t hloc[256];
  if (tid < 256) hloc[tid] = 0u;
  wg_sync();

  // z rows of a 16-row step: element e = lane + 64 i of the (16, D) block, i < ZI (16 D <= 144 up to Dz = 9, <= 256 up to 16)
  constexpr int ZI = 4;     // (16 Dz <= 256: Dz <= 16 — full maps beyond Dz = 9 and the reduced maps of structured blocks)
  const int64_t nsteps = (N + 15) / 16;
  const int64_t nwaves = (int64_t)gridDim.x * (kRowWaveWG / 64), wv = (int64_t)blockIdx.x * (kRowWaveWG / 64) + wave;
  int zoff[ZI];
#pragma unroll
  for (int i = 0; i < ZI; ++i) {
    const int e = lane + 64 * i, r = e / D;
    zoff[i] = e < 16 * D ? r * ZS + (e - r * D) : -1;
  }
  double zr[ZI];
  auto load_z = [&](int64_t t) {
    const int64_t base = t * 16 * D, total = N * D;
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int64_t gidx = base + lane + 64 * i;
      zr[i] = (zoff[i] >= 0 && gidx < total) ? a.Z[gidx] : 0.0;
    }
  };
  if (wv < nsteps) load_z(wv);

  const double* zrow = Zw + j * ZS;
  const double* thl = Th + lane;
  // B operand of step s, lane (q, j): feature 4 s + q of row j = z~[a] z~[b]; the two LDS addresses are fixed for the
  // whole kernel (2 NS registers), so a step costs two LDS reads and one product; beyond 16 steps (Dz > 9) the two
  // byte offsets share one register per step (two more integer instructions per step)
  constexpr bool kPacked = NS > 16;
  const double* fpa[kPacked ? 1 : NS];
  const double* fpb[kPacked ? 1 : NS];
  uint32_t fo[kPacked ? NS : 1];
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2) {
    if constexpr (kPacked) {
      fo[s2] = 8u * a.feat[2 * (4 * s2 + q)] | (8u * a.feat[2 * (4 * s2 + q) + 1]) << 16;
    } else {
      fpa[s2] = zrow + a.feat[2 * (4 * s2 + q)];
      fpb[s2] = zrow + a.feat[2 * (4 * s2 + q) + 1];
    }
  }
  auto feature = [&](int s2) -> double {
    if constexpr (kPacked) {
      const char* zb = reinterpret_cast<const char*>(zrow);
      return *reinterpret_cast<const double*>(zb + (fo[s2] & 0xffffu)) * *reinterpret_cast<const double*>(zb + (fo[s2] >> 16));
    } else {
      return *fpa[s2] * *fpb[s2];
    }
  };
  // Philox uniforms four steps at a time: lane (q, j) draws the uniform of row j of this wave's step t + q nwaves
  double ubatch = 0.0;
  int uphase = 0;

  for (int64_t t = wv; t < nsteps; t += nwaves) {
    const int64_t n = t * 16 + j;
    const bool valid = n < N;
    // ---- stage this step's z~ rows in the wave's own LDS block (LDS operations of one wave execute in order)
#pragma unroll
    for (int i = 0; i < ZI; ++i)
      if (zoff[i] >= 0) Zw[zoff[i]] = zr[i];
    if (q == 0) {
      Zw[j * ZS + D] = valid ? 1.0 : 0.0;     // rows past N: every feature 0, l = 0, never written
      Zw[j * ZS + D + 1] = 0.0;               // padded features read this slot
    }
    if (t + nwaves < nsteps) load_z(t + nwaves);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- L (16 KB x 16) = Theta . Phi' ---------------------------------------------------------------
    d4 acc[KB];
#pragma unroll
    for (int rb = 0; rb < KB; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
    constexpr int PF = 4;              // Theta slices in flight; slice e = s KB + rb sits in slot e % PF
    double ring[PF];
#pragma unroll
    for (int e = 0; e < PF; ++e) ring[e] = thl[e * 64];
    double bq = feature(0);
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) {            // NS is a multiple of 4: slot (s2 KB + rb) % PF is static
      const double bcur = bq;
      if (s2 + 1 < NS) bq = feature(s2 + 1);
#pragma unroll
      for (int rb = 0; rb < KB; ++rb) {
        const int e = s2 * KB + rb;
        const double av = ring[e % PF];
        ring[e % PF] = thl[(e + PF) * 64];       // (the last step reads the 4 zero slices behind the image)
        acc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bcur, acc[rb], 0, 0, 0);
      }
    }

    // ---- draw: lane (q, j) holds components q V .. q V + V - 1 of row j, x[4 rb + r] = acc[rb][r] ----------
    __builtin_amdgcn_s_setprio(2);
    double m;
    {
      double mv[4] = {acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
#pragma unroll
      for (int rb = 1; rb < KB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mv[r] = fmax(mv[r], acc[rb][r]);
      m = fmax(fmax(mv[0], mv[1]), fmax(mv[2], mv[3]));
      m = butterfly_max<gibbs_rowwave_lane_regs(KB, NS4), 16>(m);
      m = butterfly_max<gibbs_rowwave_lane_regs(KB, NS4), 32>(m);
    }
    // e = exp(l - max), then inclusive cumulative sums inside chunks of 8 (independent chains across the chunks)
    double base[NCH + 1];
    base[0] = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      double x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = exp_nonpos_t2048c(acc[2 * c + (i >> 2)][i & 3] - m, etab);
#pragma unroll
      for (int i = 1; i < 8; ++i) x[i] += x[i - 1];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[2 * c + (i >> 2)][i & 3] = x[i];
      base[c + 1] = x[7];
      __builtin_amdgcn_sched_barrier(0);       // one chunk of exp chains in flight at a time (register pressure)
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) base[c + 1] += base[c];      // base[c] = sum of the chunks before c
    const double cum = base[NCH];
    double incl = cum;                          // inclusive scan over the four quarters of the row (lanes j, j+16, ..)
    {
      double v = __shfl_up(incl, 16);  if (q >= 1) incl += v;
      v = __shfl_up(incl, 32);         if (q >= 2) incl += v;
    }
    double excl = __shfl_up(incl, 16);
    if (q == 0) excl = 0.0;
    const double ctot = __shfl(incl, 48 + j);
    double uu;
    if (a.u) {
      uu = valid ? a.u[n] : 0.0;
    } else {
      if (uphase == 0)        // (wave-uniform) the same counters as one draw per step: the labels are the same labels
        ubatch = philox_uniform(a.seed, (uint64_t)(a.row0 + (t + (int64_t)q * nwaves) * 16 + j), a.sweep);
      uu = __shfl(ubatch, uphase * 16 + j);
      uphase = (uphase + 1) & 3;
    }
    const double tl = uu * ctot - excl;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const double tc = tl - base[c];
#pragma unroll
      for (int i = 0; i < 8; ++i) cnt += tc > acc[2 * c + (i >> 2)][i & 3] ? 1 : 0;
    }
    cnt = butterfly_sum<gibbs_rowwave_lane_regs(KB, NS4), 16>(cnt);
    cnt = butterfly_sum<gibbs_rowwave_lane_regs(KB, NS4), 32>(cnt);
    const int label = draw_label(cnt, K, a.relabel, uu);
    if (q == 0 && valid) {
      a.labels[n] = label;
      if (a.fuse_hist) atomicAdd(&hloc[label], 1u);
    }
    __builtin_amdgcn_s_setprio(0);
  }
  if (a.fuse_hist) {                       // (wave-uniform)
    wg_sync();
    if (tid < 256 && hloc[tid]) atomicAdd(&a.aux[tid], hloc[tid]);
  }
}

// ------------------------------------------------------------------------------------------
// The same label pass where Theta does not fit LDS (K F16 8 bytes: 327 KB at K = 256, Dz = 16; 590 KB at K = 128, Dz = 32):
// the operand image STREAMS through a double buffer in chunks of NSC contraction steps (48 KB), the workgroup's eight waves
// walk the chunks together — one barrier per chunk, i.e. per NSC KB = 96 matrix instructions of every wave — and the next
// chunk (cyclic: Theta does not change from step to step) is fetched from L2 into registers under the current chunk's
// products and stored behind them.  The accumulators carry the l values of all components across the chunks, the draw is the
// one of gibbs_rowwave_kernel.  The feature pair of a step comes from a small LDS table (NS x 4 packed byte offsets) instead of
// 2 NS address registers.  These shapes ran on the tile kernels' pipelined E-step (wide_estep_kernel: K = 128, Dz = 16 at 49 % of
// the FP64 rate in the label pass against 74 % for the row-owner kernel at K = 64).
// L2 -> LDS traffic: the whole image per 128 rows (Dz = 16, K = 256: 2.5 KB per row, 25 GB per 1e7 rows — a quarter of the
// pass's matrix time at the 10 TB/s the L2s deliver, and hidden under it).
// ------------------------------------------------------------------------------------------
#ifndef MIMO_STREAM_TAIL
// 0: all padded steps computed, 1: a (wave-uniform) guard per step, 2: the guarded loop for a partial last chunk only.  One box,
// N = 2e6, label pass + statistics in us (profiles/r03_stream_tail_variants.txt), variants 0 / 1 / 2: Dz=16, K=128 1924 / 1746 / 1807;
// Dz=20, K=64 1653 / 1521 / 1549; Dz=24, K=64 2143 / 2020 / 2071; Dz=16, K=256 3381 / 3278 / 6364 (the two loop bodies of variant 2
// spill there); shapes without padding Dz=32, K=128 6232 / 6180 / 6476, Dz=12, K=192 1992 / 2050 / 2184
#define MIMO_STREAM_TAIL 1
#endif
constexpr int stream_nsc(int KB) { return KB <= 2 ? 48 : KB <= 4 ? 24 : KB <= 6 ? 16 : KB <= 8 ? 12 : KB <= 14 ? 8 : 6; }   // (NSC KB: a multiple of 16)

template <int KB, int ZI>
__global__ __launch_bounds__(kRowWaveWG, 1) void gibbs_stream_kernel(const KernelArgs a, int NSP, int NS) {
  constexpr int V = 4 * KB, NCH = KB / 2, NSC = stream_nsc(KB);
  constexpr int CH = NSC * KB * 64;                   // doubles per chunk
  constexpr int NLD = CH / (2 * kRowWaveWG);          // 16-byte loads per thread and chunk
  static_assert(KB % 2 == 0 && KB >= 2 && KB <= 16 && CH % (2 * kRowWaveWG) == 0, "row blocks per wave / chunk geometry");
  typedef double d2 __attribute__((ext_vector_type(2)));
  extern __shared__ __align__(16) unsigned char smem[];
  const int ZS = a.ZS;
  double* buf = reinterpret_cast<double*>(smem);      // [2][CH]
  double* etab = buf + 2 * CH;                        // [kExpTab]
  double* Zall = etab + kExpTab;                      // [8 waves][16][ZS]
  uint32_t* ftab = reinterpret_cast<uint32_t*>(Zall + (size_t)(kRowWaveWG / 64) * 16 * ZS);   // [NSP][4] packed byte offsets of a step's feature pair

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, j = lane & 15;
  const int D = a.D, K = a.K;
  const int64_t N = a.N;
  const int nch = NSP / NSC;                          // chunks per pass over the image (host: NSP is a multiple of NSC)
  double* Zw = Zall + (size_t)wave * 16 * ZS;

  for (int e = tid; e < kExpTab; e += kRowWaveWG) etab[e] = exp_tab_entry_c(e);
  for (int e = tid; e < NSP * 4; e += kRowWaveWG) {
    const int f = e;                                  // feature 4 s + q; beyond the table: the zero slot of z~
    const uint32_t fa = f < a.F16 ? a.feat[2 * f] : (uint32_t)(D + 1), fb = f < a.F16 ? a.feat[2 * f + 1] : (uint32_t)(D + 1);
    ftab[e] = 8u * fa | (8u * fb) << 16;
  }
  {                                                   // chunk 0 -> buffer 0 (the loop's first barrier publishes it)
    const d2* src = reinterpret_cast<const d2*>(a.theta) + tid;
    d2* dst = reinterpret_cast<d2*>(buf) + tid;
#pragma unroll
    for (int i = 0; i < NLD; ++i) dst[i * kRowWaveWG] = src[i * kRowWaveWG];
  }

  const int64_t nsteps = (N + 127) / 128;             // workgroup steps: 8 waves x 16 rows
  int zoff[ZI];
#pragma unroll
  for (int i = 0; i < ZI; ++i) {
    const int e = lane + 64 * i, r = e / D;
    zoff[i] = e < 16 * D ? r * ZS + (e - r * D) : -1;
  }
  double zr[ZI];
  auto load_z = [&](int64_t t) {
    const int64_t base = (t * 8 + wave) * 16 * D, total = N * D;
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int64_t gidx = base + lane + 64 * i;
      zr[i] = (zoff[i] >= 0 && gidx < total) ? a.Z[gidx] : 0.0;
    }
  };
  if ((int64_t)blockIdx.x < nsteps) load_z(blockIdx.x);

  const char* zb = reinterpret_cast<const char*>(Zw + j * ZS);
  auto feature = [&](int s) -> double {
    const uint32_t u = ftab[4 * s + q];
    return *reinterpret_cast<const double*>(zb + (u & 0xffffu)) * *reinterpret_cast<const double*>(zb + (u >> 16));
  };
  double ubatch = 0.0;
  int uphase = 0;
  int gc = 0;                                          // chunks done: chunk gc lives in buffer gc & 1

  for (int64_t t = blockIdx.x; t < nsteps; t += gridDim.x) {
    const int64_t n = (t * 8 + wave) * 16 + j;
    const bool valid = n < N;
#pragma unroll
    for (int i = 0; i < ZI; ++i)
      if (zoff[i] >= 0) Zw[zoff[i]] = zr[i];
    if (q == 0) {
      Zw[j * ZS + D] = valid ? 1.0 : 0.0;     // rows past N: every feature 0, l = 0, never written
      Zw[j * ZS + D + 1] = 0.0;
    }
    if (t + gridDim.x < nsteps) load_z(t + gridDim.x);

    d4 acc[KB];
#pragma unroll
    for (int rb = 0; rb < KB; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nch; ++c, ++gc) {
      wg_sync();                               // chunk gc stands in its buffer; everybody is done with the other one
      const double* bc = buf + (gc & 1) * CH + lane;
      // the next chunk of the cyclic walk: global -> registers now, registers -> the other buffer behind the products
      d2 stg[NLD];
      {
        const int cn = c + 1 < nch ? c + 1 : 0;
        const d2* src = reinterpret_cast<const d2*>(a.theta + (size_t)cn * CH) + tid;
#pragma unroll
        for (int i = 0; i < NLD; ++i) stg[i] = src[i * kRowWaveWG];
      }
      constexpr int PF = 4;
      double ring[PF];
#pragma unroll
      for (int e = 0; e < PF; ++e) ring[e] = bc[e * 64];
      const int s0 = c * NSC;
      // steps of this chunk that carry features (wave-uniform): the image is padded to whole chunks with zero rows, and the
      // products of the padding — up to a fifth of the pass at Dz = 16, K = 96 / 128 or Dz = 20, K = 64 — are skipped
      const int lim = NS - s0;
      double bq = feature(s0);
      auto products = [&](auto guarded) {
#pragma unroll
        for (int s2 = 0; s2 < NSC; ++s2) {
          if (!decltype(guarded)::value || s2 < lim) {
            const double bcur = bq;
            if (s2 + 1 < NSC) bq = feature(s0 + s2 + 1);
#pragma unroll
            for (int rb = 0; rb < KB; ++rb) {
              const int e = s2 * KB + rb;
              const double av = ring[e % PF];
              if (e + PF < NSC * KB) ring[e % PF] = bc[(e + PF) * 64];
              acc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bcur, acc[rb], 0, 0, 0);
            }
          }
        }
      };
#if MIMO_STREAM_TAIL == 0
      products(std::false_type{});
#elif MIMO_STREAM_TAIL == 1
      products(std::true_type{});
#else
      if (lim >= NSC) products(std::false_type{}); else products(std::true_type{});
#endif
      {
        d2* dst = reinterpret_cast<d2*>(buf + ((gc + 1) & 1) * CH) + tid;
#pragma unroll
        for (int i = 0; i < NLD; ++i) dst[i * kRowWaveWG] = stg[i];
      }
    }

    // ---- draw: lane (q, j) holds components q V .. q V + V - 1 of row j, x[4 rb + r] = acc[rb][r] (as gibbs_rowwave_kernel)
    __builtin_amdgcn_s_setprio(2);
    double m;
    {
      double mv[4] = {acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
#pragma unroll
      for (int rb = 1; rb < KB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mv[r] = fmax(mv[r], acc[rb][r]);
      m = fmax(fmax(mv[0], mv[1]), fmax(mv[2], mv[3]));
      m = butterfly_max<true, 16>(m);
      m = butterfly_max<true, 32>(m);
    }
    double base[NCH + 1];
    base[0] = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      double x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = exp_nonpos_t2048c(acc[2 * c + (i >> 2)][i & 3] - m, etab);
#pragma unroll
      for (int i = 1; i < 8; ++i) x[i] += x[i - 1];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[2 * c + (i >> 2)][i & 3] = x[i];
      base[c + 1] = x[7];
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) base[c + 1] += base[c];
    const double cum = base[NCH];
    double incl = cum;
    {
      double v = __shfl_up(incl, 16);  if (q >= 1) incl += v;
      v = __shfl_up(incl, 32);         if (q >= 2) incl += v;
    }
    double excl = __shfl_up(incl, 16);
    if (q == 0) excl = 0.0;
    const double ctot = __shfl(incl, 48 + j);
    double uu;
    if (a.u) {
      uu = valid ? a.u[n] : 0.0;
    } else {
      if (uphase == 0)        // four workgroup steps at a time: lane (q, j) draws row j of this wave's step t + q gridDim.x
        ubatch = philox_uniform(a.seed, (uint64_t)(a.row0 + ((t + (int64_t)q * gridDim.x) * 8 + wave) * 16 + j), a.sweep);
      uu = __shfl(ubatch, uphase * 16 + j);
      uphase = (uphase + 1) & 3;
    }
    const double tl = uu * ctot - excl;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const double tc = tl - base[c];
#pragma unroll
      for (int i = 0; i < 8; ++i) cnt += tc > acc[2 * c + (i >> 2)][i & 3] ? 1 : 0;
    }
    cnt = butterfly_sum<true, 16>(cnt);
    cnt = butterfly_sum<true, 32>(cnt);
    const int label = draw_label(cnt, K, a.relabel, uu);
    if (q == 0 && valid) a.labels[n] = label;
    __builtin_amdgcn_s_setprio(0);
  }
}

// contraction steps of the streamed image: F16 / 4 padded to whole chunks
int stream_ns_pad(int KB, int F16) { const int nsc = stream_nsc(KB), ns = F16 / 4; return (ns + nsc - 1) / nsc * nsc; }
size_t stream_lds_bytes(int KB, int F16, int ZS) {
  return sizeof(double) * ((size_t)2 * stream_nsc(KB) * KB * 64 + kExpTab + (size_t)(kRowWaveWG / 64) * 16 * ZS)
         + sizeof(uint32_t) * (size_t)stream_ns_pad(KB, F16) * 4;
}

size_t rowwave_lds_bytes(int KB, int NS, int ZS) {
  return sizeof(double) * ((size_t)(NS * KB + 4) * 64 + kExpTab + (size_t)(kRowWaveWG / 64) * 16 * ZS);
}

int rowwave_kb(int K) {           // row blocks the kernel is instantiated for: 2, 4, .., 16
  int kb = (K + 15) / 16;
  kb += kb & 1;
  return kb < 2 ? 2 : kb;
}

// Smallest K that takes the row-owner route (tuning knob; default: every K).  Measured against the fused tile kernels,
// N = 1e7 (tools/midk_time.py, labels + statistics): K = 64, D = 8 sweep 2.50 -> 1.69 ms, K = 32: 1.99 -> 1.05, K = 17: 1.94 ->
// 1.07, K = 16: 1.54 -> 1.05, K = 8: 1.52 -> 1.00, D = 5, K = 16: 1.52 -> 0.82, D = 7, K = 4: 1.43 -> 0.98 (the last three
// only since the label-statistics pass spreads a component's rows over 256 / Kp threads: with one thread per
// component they lost).  Also the smallest K of the label statistics (mimo_label_stats.hip).
int rowwave_min_k() {
  static const int v = [] { const char* e = getenv("MIMO_ROWWAVE_MIN_K"); return e ? atoi(e) : 1; }();
  return v;
}

// K <= 256 (from rowwave_min_k) at Dz <= 9 (F16 <= 64); Dz 10 .. 16 (F16 <= 160) while the operand image fits LDS next to
// the exp table: K <= 64, and K <= 128 up to Dz = 12 (the instantiations below)
static bool rowwave_resident(int K, int F16, int ZS) {
  if (K < rowwave_min_k() || K > 256 || F16 > 160) return false;
  const int kb = rowwave_kb(K);
  if (F16 > 64 && !(kb <= 4 || (kb <= 8 && F16 <= 96))) return false;
  return rowwave_lds_bytes(kb, F16 / 4, ZS) + 1024 <= 160 * 1024;      // (+ the kernel's static 1 KB label histogram)
}
// Row blocks for the shape: rowwave_kb(K), except that the streamed walk of 193 <= K <= 224 (14 row blocks: chunks of 8 steps = 57 KB,
// two of them + the z rows of Dz >= 25 do not fit 160 KB) runs with 16 (chunks of 6 steps = 49 KB) — 14 % more matrix work, no table
int rowwave_kb_shape(int K, int F16, int ZS) {
  const int kb = rowwave_kb(K);
  if (kb == 14 && !rowwave_resident(K, F16, ZS) && stream_lds_bytes(14, F16, ZS) > 160 * 1024) return 16;
  return kb;
}
// ... and beyond that, up to Dz = 32 (F16 <= 576), with Theta streamed through LDS (MIMO_ROWWAVE_STREAM=0: off, tuning knob)
static bool rowwave_streams(int K, int F16, int ZS) {
  static const bool on = [] { const char* e = getenv("MIMO_ROWWAVE_STREAM"); return !e || atoi(e) != 0; }();
  if (!on || K < rowwave_min_k() || K > 256 || F16 > 576 || rowwave_resident(K, F16, ZS)) return false;
  return stream_lds_bytes(rowwave_kb_shape(K, F16, ZS), F16, ZS) <= 160 * 1024;
}
bool rowwave_covers(int K, int F16, int ZS) { return rowwave_resident(K, F16, ZS) || rowwave_streams(K, F16, ZS); }
// contraction steps the operand image must hold for (K, F16): F16 / 4, or whole chunks of the streamed walk
int rowwave_image_ns(int K, int F16, int ZS) {
  return rowwave_streams(K, F16, ZS) ? stream_ns_pad(rowwave_kb_shape(K, F16, ZS), F16) : F16 / 4;
}

typedef void (*rowwave_fn)(const KernelArgs);
template <int NS4>
static rowwave_fn pick_rowwave_kb(int kb) {
  switch (kb) {
    case 2: return gibbs_rowwave_kernel<2, NS4>;
    case 4: return gibbs_rowwave_kernel<4, NS4>;
    case 6: return gibbs_rowwave_kernel<6, NS4>;
    case 8: return gibbs_rowwave_kernel<8, NS4>;
    case 10: return gibbs_rowwave_kernel<10, NS4>;
    case 12: return gibbs_rowwave_kernel<12, NS4>;
    case 14: return gibbs_rowwave_kernel<14, NS4>;
    case 16: return gibbs_rowwave_kernel<16, NS4>;
  }
  return nullptr;
}
template <int NS4>
static rowwave_fn pick_rowwave_wide(int kb) {      // Dz 10 .. 16: K <= 64 (and K <= 128 while F16 <= 96)
  switch (kb) {
    case 2: return gibbs_rowwave_kernel<2, NS4>;
    case 4: return gibbs_rowwave_kernel<4, NS4>;
    case 6: if constexpr (NS4 <= 6) return gibbs_rowwave_kernel<6, NS4>; else return nullptr;
    case 8: if constexpr (NS4 <= 6) return gibbs_rowwave_kernel<8, NS4>; else return nullptr;
  }
  return nullptr;
}
static rowwave_fn pick_rowwave(int kb, int F16) {
  switch (F16 / 16) {
    case 1: return pick_rowwave_kb<1>(kb);
    case 2: return pick_rowwave_kb<2>(kb);
    case 3: return pick_rowwave_kb<3>(kb);
    case 4: return pick_rowwave_kb<4>(kb);
    case 5: return pick_rowwave_wide<5>(kb);
    case 6: return pick_rowwave_wide<6>(kb);
    case 7: return pick_rowwave_wide<7>(kb);
    case 8: return pick_rowwave_wide<8>(kb);
    case 9: return pick_rowwave_wide<9>(kb);
    case 10: return pick_rowwave_wide<10>(kb);
  }
  return nullptr;
}

int rowwave_grid(const KernelArgs& a, int num_cu) {
  const int64_t steps = (a.N + 15) / 16, need = (steps + 7) / 8;
  int64_t g = num_cu;
  if (g > need) g = need;
  return (int)(g < 1 ? 1 : g);
}

typedef void (*stream_fn)(const KernelArgs, int, int);
template <int ZI>
static stream_fn pick_stream(int kb) {
  switch (kb) {
    case 2: return gibbs_stream_kernel<2, ZI>;    case 4: return gibbs_stream_kernel<4, ZI>;
    case 6: return gibbs_stream_kernel<6, ZI>;    case 8: return gibbs_stream_kernel<8, ZI>;
    case 10: return gibbs_stream_kernel<10, ZI>;  case 12: return gibbs_stream_kernel<12, ZI>;
    case 14: return gibbs_stream_kernel<14, ZI>;  case 16: return gibbs_stream_kernel<16, ZI>;
  }
  return nullptr;
}

hipError_t launch_gibbs_rowwave(const KernelArgs& a, int grid, hipStream_t stream) {
  if (rowwave_streams(a.K, a.F16, a.ZS)) {
    const int kb = rowwave_kb_shape(a.K, a.F16, a.ZS);
    stream_fn fn = 16 * a.D <= 256 ? pick_stream<4>(kb) : pick_stream<8>(kb);
    if (!fn || a.D > 32) return hipErrorInvalidValue;
    const size_t lds = stream_lds_bytes(kb, a.F16, a.ZS);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int64_t need = (a.N + 127) / 128;
    int g = grid;
    if (g > need) g = (int)(need < 1 ? 1 : need);
    hipLaunchKernelGGL(fn, dim3(g), dim3(kRowWaveWG), lds, stream, a, stream_ns_pad(kb, a.F16), a.F16 / 4);
    return hipGetLastError();
  }
  const int kb = rowwave_kb(a.K);
  rowwave_fn fn = pick_rowwave(kb, a.F16);
  if (!fn) return hipErrorInvalidValue;
  const size_t lds = rowwave_lds_bytes(kb, a.F16 / 4, a.ZS);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kRowWaveWG), lds, stream, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Mean-field / EM pass (softmax + weighted statistics) on row-owner waves: K <= 64, Dz <= 9.
// Through the tile kernels this regime runs at 44 - 60 % of its MFMA time (N = 1e7, D = 8: K = 64 2.58 ms against a
// floor of 1.56 ms, K = 32 1.90 ms): one 32-row tile per workgroup, four barriers per tile, the l / r tile through LDS
// for all four waves.  Here a wave owns 16 rows for BOTH products:
//   L = Theta . Phi'   exactly as in gibbs_rowwave_kernel (Theta in LDS, B operand built on the fly);
//   softmax over the lane's contiguous quarter of the components in registers;
//   the wave's r values go to a wave-private LDS block Rt[row][slot] (slot = 16 rb + 4 r + q: the A-operand order of
//   the second product), then  S += R . Phi :  A = Rt[row 4t + kk][16 rb + i], B = Phi[row 4t + kk][16 cb + j] built
//   on the fly from the same z rows; the wave keeps its OWN K x F16 statistic block in registers (KB NCB accumulator
//   quads: 96 VGPRs at K = 64, Dz = 8) across all its steps.  No workgroup barrier in the loop.
// At the end the 8 waves of the workgroup add their blocks through LDS in wave order, one accumulator quad at a time.
// S-row i of row block rb holds component (i & 3) V + 4 rb + (i >> 2) (the permutation of the operand image).
// ------------------------------------------------------------------------------------------
template <int KB, int NS4>
__global__ __launch_bounds__(kRowWaveWG, 1) void vi_rowwave_kernel(const KernelArgs a) {
  constexpr int V = 4 * KB, NS = 4 * NS4, NCB = NS4;
  constexpr int RS2 = 16 * KB + 8;                    // row stride of the wave's r block (doubles)
  static_assert(KB == 2 || KB == 4, "K <= 64");
  extern __shared__ __align__(16) unsigned char smem[];
  const int ZS = a.ZS;
  double* Th = reinterpret_cast<double*>(smem);       // [(NS KB + 4)][64]
  double* etab = Th + (size_t)(NS * KB + 4) * 64;     // [kExpTab]
  double* Zall = etab + kExpTab;                      // [8][16][ZS]
  double* Rall = Zall + (size_t)(kRowWaveWG / 64) * 16 * ZS;   // [8][16][RS2]
  double* sred = Rall + (size_t)(kRowWaveWG / 64) * 16 * RS2;  // [8]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, j = lane & 15;
  const int D = a.D, K = a.K;
  const int64_t N = a.N;
  double* Zw = Zall + (size_t)wave * 16 * ZS;
  double* Rt = Rall + (size_t)wave * 16 * RS2;

  for (int e = tid; e < NS * KB * 64; e += kRowWaveWG) Th[e] = a.theta[e];
  for (int e = tid; e < 4 * 64; e += kRowWaveWG) Th[NS * KB * 64 + e] = 0.0;
  for (int e = tid; e < kExpTab; e += kRowWaveWG) etab[e] = exp_tab_entry_c(e);
  wg_sync();

  const int64_t nsteps = (N + 15) / 16;
  const int64_t nwaves = (int64_t)gridDim.x * (kRowWaveWG / 64), wv = (int64_t)blockIdx.x * (kRowWaveWG / 64) + wave;
  constexpr int ZI = 4;      // 16 Dz <= 256 elements per step (Dz <= 16: the reduced feature maps of structured blocks)
  int zoff[ZI];
#pragma unroll
  for (int i = 0; i < ZI; ++i) {
    const int e = lane + 64 * i, r = e / D;
    zoff[i] = e < 16 * D ? r * ZS + (e - r * D) : -1;
  }
  double zr[ZI];
  auto load_z = [&](int64_t t) {
    const int64_t base = t * 16 * D, total = N * D;
#pragma unroll
    for (int i = 0; i < ZI; ++i) {
      const int64_t gidx = base + lane + 64 * i;
      zr[i] = (zoff[i] >= 0 && gidx < total) ? a.Z[gidx] : 0.0;
    }
  };
  if (wv < nsteps) load_z(wv);

  const double* zrow = Zw + j * ZS;
  const double* thl = Th + lane;
  constexpr bool kPacked = KB == 4 && NS > 12;        // (K > 32 at Dz = 9: the two offsets of a step share a register)
  const double* fpa[kPacked ? 1 : NS];
  const double* fpb[kPacked ? 1 : NS];
  uint32_t fo[kPacked ? NS : 1];
#pragma unroll
  for (int s2 = 0; s2 < NS; ++s2) {
    if constexpr (kPacked) {
      fo[s2] = 8u * a.feat[2 * (4 * s2 + q)] | (8u * a.feat[2 * (4 * s2 + q) + 1]) << 16;
    } else {
      fpa[s2] = zrow + a.feat[2 * (4 * s2 + q)];
      fpb[s2] = zrow + a.feat[2 * (4 * s2 + q) + 1];
    }
  }
  auto feature = [&](int s2) -> double {
    if constexpr (kPacked) {
      const char* zb = reinterpret_cast<const char*>(zrow);
      return *reinterpret_cast<const double*>(zb + (fo[s2] & 0xffffu)) * *reinterpret_cast<const double*>(zb + (fo[s2] >> 16));
    } else {
      return *fpa[s2] * *fpb[s2];
    }
  };
  // second product: lane (kk = q, col j) builds feature 16 cb + j of row 4 t + kk; A operand = Rt[4 t + kk][16 rb + i], i = j
  const double* zk = Zw + q * ZS;                     // row kk of the step's block; row 4 t + kk is 4 t ZS doubles further
  int spa[NCB], spb[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    spa[cb] = a.feat[2 * (16 * cb + j)];
    spb[cb] = a.feat[2 * (16 * cb + j) + 1];
  }
  const double* rk = Rt + q * RS2 + j;
  double* rw = Rt + j * RS2 + q;                      // this lane's r values: slot 16 rb + 4 r + q of row j

  d4 sacc[KB][NCB];
#pragma unroll
  for (int rb = 0; rb < KB; ++rb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) sacc[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};
  double sc_lse = 0.0, sc_prod = 1.0;
  int since_flush = 0;

  for (int64_t t = wv; t < nsteps; t += nwaves) {
    const int64_t n = t * 16 + j;
    const bool valid = n < N;
#pragma unroll
    for (int i = 0; i < ZI; ++i)
      if (zoff[i] >= 0) Zw[zoff[i]] = zr[i];
    if (q == 0) {
      Zw[j * ZS + D] = valid ? 1.0 : 0.0;     // rows past N: every feature 0 — l = 0, and nothing reaches the statistics
      Zw[j * ZS + D + 1] = 0.0;
    }
    if (t + nwaves < nsteps) load_z(t + nwaves);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- L = Theta . Phi' ------------------------------------------------------------------------
    d4 acc[KB];
#pragma unroll
    for (int rb = 0; rb < KB; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
    {
      constexpr int PF = 4;
      double ring[PF];
#pragma unroll
      for (int e = 0; e < PF; ++e) ring[e] = thl[e * 64];
      double bq = feature(0);
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) {
        const double bcur = bq;
        if (s2 + 1 < NS) bq = feature(s2 + 1);
#pragma unroll
        for (int rb = 0; rb < KB; ++rb) {
          const int e = s2 * KB + rb;
          const double av = ring[e % PF];
          ring[e % PF] = thl[(e + PF) * 64];
          acc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bcur, acc[rb], 0, 0, 0);
        }
      }
    }

    // ---- softmax over the row's components (this lane: components q V .. q V + V - 1) ------------------
    __builtin_amdgcn_s_setprio(2);
    double m;
    {
      double mv[4] = {acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
#pragma unroll
      for (int rb = 1; rb < KB; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mv[r] = fmax(mv[r], acc[rb][r]);
      m = fmax(fmax(mv[0], mv[1]), fmax(mv[2], mv[3]));
      m = butterfly_max<vi_rowwave_lane_regs(KB, NS4), 16>(m);
      m = butterfly_max<vi_rowwave_lane_regs(KB, NS4), 32>(m);
    }
    double sv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rb = 0; rb < KB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[rb][r] = exp_nonpos_t2048c(acc[rb][r] - m, etab);
        sv[r] += acc[rb][r];
      }
    double ssum = (sv[0] + sv[1]) + (sv[2] + sv[3]);
    ssum = butterfly_sum<vi_rowwave_lane_regs(KB, NS4), 16>(ssum);
    ssum = butterfly_sum<vi_rowwave_lane_regs(KB, NS4), 32>(ssum);
    double inv = __builtin_amdgcn_rcp(ssum);
    inv = fma(fma(-ssum, inv, 1.0), inv, inv);
    inv = fma(fma(-ssum, inv, 1.0), inv, inv);
    if (q == 0 && valid) { sc_lse += m; sc_prod *= ssum; }
    // (rows past N need no masking of r: all their features are 0, they add nothing to S)
#pragma unroll
    for (int rb = 0; rb < KB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) rw[16 * rb + 4 * r] = acc[rb][r] * inv;
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- S += R . Phi: four rows per MFMA step -------------------------------------------------------
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const double* zt = zk + (size_t)(4 * t4) * ZS;
      double bv[NCB], av[KB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) bv[cb] = zt[spa[cb]] * zt[spb[cb]];
#pragma unroll
      for (int rb = 0; rb < KB; ++rb) av[rb] = rk[4 * t4 * RS2 + 16 * rb];
#pragma unroll
      for (int rb = 0; rb < KB; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          sacc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rb], bv[cb], sacc[rb][cb], 0, 0, 0);
    }
    if (++since_flush == 64) {         // K^64 <= 64^64 = 2^384 stays inside the float64 range
      sc_lse += log(sc_prod);
      sc_prod = 1.0;
      since_flush = 0;
    }
  }

  // ---- per-workgroup partial block: the eight waves' blocks added in wave order, one accumulator quad at a time ----
  const int FT = a.F16_total;
  const size_t pstride = (size_t)a.K16 * 16 * FT + 4;
  double* P = a.partials + (size_t)blockIdx.x * pstride;
  double* red = Th;                                    // [8 waves][4][64] per quad: 16 KB of the (now idle) operand image
#pragma unroll
  for (int rb = 0; rb < KB; ++rb) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      wg_sync();
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = sacc[rb][cb][r];
      wg_sync();
      if (wave < 4) {                                  // wave r adds register r of the eight waves
        double s2 = red[(0 * 4 + wave) * 64 + lane];
#pragma unroll
        for (int w = 1; w < kRowWaveWG / 64; ++w) s2 += red[(w * 4 + wave) * 64 + lane];
        const int i = q + 4 * wave;                    // S-row of register `wave` in lane (q, j)
        const int k = (i & 3) * V + 4 * rb + (i >> 2);
        if (k < a.K16 * 16) P[(size_t)k * FT + 16 * cb + j] = k < K ? s2 : 0.0;
      }
    }
  }
  sc_lse += log(sc_prod);
  sc_lse = wave_sum(sc_lse);
  wg_sync();
  if (lane == 0) sred[wave] = sc_lse;
  wg_sync();
  if (tid == 0 && a.write_scalars) {
    double* Ps = P + (size_t)a.K16 * 16 * FT;
    double s2 = 0.0;
    for (int w = 0; w < kRowWaveWG / 64; ++w) s2 += sred[w];
    Ps[0] = s2; Ps[1] = 0.0; Ps[2] = 0.0; Ps[3] = 0.0;
  }
}

size_t vi_rowwave_lds_bytes(int KB, int NS, int ZS) {
  return sizeof(double) * ((size_t)(NS * KB + 4) * 64 + kExpTab + (size_t)(kRowWaveWG / 64) * 16 * (ZS + 16 * KB + 8) + 8);
}

// K <= 64, Dz <= 9 (F16 <= 64), from the same K as the label route
bool vi_rowwave_covers(int K, int F16, int ZS) {
  static const bool on = [] { const char* e = getenv("MIMO_ROWWAVE_VI"); return !e || atoi(e) != 0; }();   // tuning knob
  if (!on || K < rowwave_min_k() || K > 64 || F16 > 64) return false;
  if (K > 32 && F16 > 48) return false;       // Dz = 9 with four row blocks: 128 + 32 accumulator registers spill (136 B)
  // measured against the tile kernels (tools/vi_route_time.py, N = 1e7, pass kernels): K <= 32 wins (D = 8: K = 32 1.87 -> 1.37 ms,
  // K = 24 1.80 -> 1.38, K = 16 1.39 -> 1.33; D = 5, K = 32 1.39 -> 1.03; D = 3, K = 24 1.04 -> 0.75) except Dz = 9 at K <= 16
  // (1.47 -> 1.58); 33 <= K <= 48 pays for 64 component slots (D = 7, K = 33: 2.07 -> 2.33); 49 <= K <= 64 wins a little at
  // Dz = 5 .. 8 (D = 8: 2.53 -> 2.41) and loses at Dz <= 4 (D = 1: 1.18 -> 1.32)
  if (K <= 32) { if (F16 == 64 && K <= 16) return false; }
  else if (K < 49 || F16 < 32) return false;
  return vi_rowwave_lds_bytes(K <= 32 ? 2 : 4, F16 / 4, ZS) <= 160 * 1024;
}

hipError_t launch_vi_rowwave(const KernelArgs& a, int grid, hipStream_t stream) {
  typedef void (*fn_t)(const KernelArgs);
  static const fn_t t2[4] = {vi_rowwave_kernel<2, 1>, vi_rowwave_kernel<2, 2>, vi_rowwave_kernel<2, 3>, vi_rowwave_kernel<2, 4>};
  static const fn_t t4[4] = {vi_rowwave_kernel<4, 1>, vi_rowwave_kernel<4, 2>, vi_rowwave_kernel<4, 3>, vi_rowwave_kernel<4, 4>};
  const int kb = a.K <= 32 ? 2 : 4, ns4 = a.F16 / 16;
  if (ns4 < 1 || ns4 > 4 || a.K > 64) return hipErrorInvalidValue;
  fn_t fn = kb == 2 ? t2[ns4 - 1] : t4[ns4 - 1];
  const size_t lds = vi_rowwave_lds_bytes(kb, a.F16 / 4, a.ZS);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kRowWaveWG), lds, stream, a);
  return hipGetLastError();
}

// the label pass of (K, F16) runs on gibbs_rowwave_kernel (Theta resident), the kernel that can count its labels
bool gibbs_rowwave_counts_labels(int K, int F16, int ZS) { return rowwave_resident(K, F16, ZS); }

}  // namespace mimo
