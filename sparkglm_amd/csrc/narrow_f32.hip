// narrow_f32.hip -- the narrow-design (p <= 64) fused IRLS pass over a float32-stored design.
//
// The design lies in HBM as float (column-major, leading dimension ld in floats, whole column
// octets, zero past p); y / m / offset / prior, beta, eta and every partial stay fp64.  A float
// widens to a double exactly, so the pass is the fp64 pass (narrow.hip) of the design rounded to
// float: the same rowmath.hpp row arithmetic, the Gram on v_mfma_f64_16x16x4_f64, the same partial
// layout (tiles | X'Wz | NS scalars | X'1 slot) behind which reduce_partials_kernel, the all-reduce
// and the solves run unchanged.  What differs is the data movement:
//
//   * one 16-byte LDS-DMA lane carries FOUR rows of one column, so a 1 KiB wave-instruction is
//     CPI = 256 / NRB columns of an NRB-row block and a block of the fp64 kernel's byte size holds
//     twice the rows: NRB = 64 for p <= 32, 32 above.  The family arithmetic then fills all 64
//     lanes (p <= 32) or 32 lanes (above) from ONE block: no block pairs, no register stash;
//   * the LDS that frees goes to a deeper ring: 3 buffers per wave at p <= 32 (8 waves at p <= 16,
//     4 waves at p <= 32, where 8 waves x 2 buffers of 10 KiB leave no room for the Poisson
//     tables), 2 buffers x 8 waves above;
//   * w and w z of a block are written over its y and m slots (every lane has read its row's
//     values by then; LDS operations of one wave complete in order), so a wave's LDS is its ring;
//   * every operand is widened once after its LDS read (v_cvt_f64_f32): the row stage widens x
//     before its fp64 FMA into eta, the Gram widens x once for av = x w, xz += x wz and both MFMA
//     operands.  Nothing is formed in fp32.
//
// LDS image of one block: column c at c NRB floats; the column's NRB / 4 16-byte slots (4 rows
// each) are permuted, slot s holding rows 4 (s ^ f(c)) .. + 3, f(c) = c & 15 at NRB = 64 and
// (c & 7) ^ ((c >> 3) & 1) at NRB = 32, applied on the DMA source address.  Row r of column c is
// at c NRB + 4 ((r >> 2) ^ f(c)) + (r & 3).  No pad between the 16-column blocks.
//
// Bank argument (4-byte banks; a wave's access is served in groups of lanes whose bytes fill the
// bank width once: 32 or 64 lanes of a b32 read, 8 or 16 of a b128):
//   * Gram operand read, ds_read_b128: the k-steps are ordered so that lane (rq, cl) owns rows
//     16 q + 4 rq .. + 3 of column 16 b + cl -- ONE slot, slot index (4 q + rq) ^ f(cl) of a column
//     whose base is a multiple of NRB / 4 slots (0 mod 8).  Over 8 consecutive cl (rq fixed)
//     f(cl) mod 8 takes 8 values, so the 8 lanes cover all 32 banks once; over 16 consecutive cl
//     the slot index mod 16 is cl ^ const (NRB = 64) or 8 (cl & 1) + (const ^ (cl & 7) ^ (cl >> 3))
//     (NRB = 32, column bases alternate 0 / 8 mod 16), 16 values either way: 64 banks once.  Four
//     k-steps per read; the MFMA sums over k, so which four rows a k-step takes is free as long
//     as A, B and w agree.
//   * row-stage read, ds_read_b32: lane (g, rl) reads row rl of column LPR u + g.  At NRB = 64
//     (LPR = 1) the 64 lanes read the 64 floats of one column, permuted: every bank once.  At
//     NRB = 32 lanes 0..31 read the 32 floats of column 2 u, lanes 32..63 those of column 2 u + 1,
//     which lie 32 floats further: 32 banks once per half, 64 banks once per wave.
//   * w / w z for the Gram: the 16 lanes of one rq read the same 32 bytes (a broadcast).
//
// vmcnt: a block is DMA_X = NC / CPI column-group instructions plus DMA_V row-vector instructions
// (2 at NRB = 64: 4 vectors x 64 rows x 8 B = 2 KiB; 1 at NRB = 32), always all of them (column
// groups past the stored ones re-load the last stored group, as narrow.hip), and an IRLS block
// without in-pass statistics issues exactly one eta store.  The loop is
//   wait(block i) ; row stage (eta store) ; Gram ; stage block i + NBUF
// so younger than block i's DMA are NBUF - 1 block DMAs and, from the (NBUF - 1)-th block of the
// range on, NBUF - 1 eta stores (fewer before: the wait then names none and waits a little longer);
// the last NBUF - 1 blocks of a range wait for everything.
//
//   P16  NRB  NW  NBUF  DMA_X + DMA_V  vmcnt (no eta / eta)   LDS per workgroup
//    1    64   8    3      4 + 2          12 / 14             144 KiB (+ tables)
//    2    64   4    3      8 + 2          20 / 22             120 KiB (+ tables)
//    3    32   8    2      6 + 1           7 /  8             112 KiB (+ tables)
//    4    32   8    2      8 + 1           9 / 10             144 KiB (+ tables)
//
// Shared with narrow.hip, in narrow_core.hpp: the issue priorities by phase, the lane helpers, gram_kstep
// (its T4 form included: the same lane layout, the same accumulators), the weighted k-step around it and
// the Poisson table prologue.  The row step and the epilogue are still this file's own: as shared
// functions they changed some kernels' register figures (profiles/narrow_core_isa.txt).
#include <algorithm>
#include <type_traits>

#include "narrow_core.hpp"

namespace sglm {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

template <int P16>
struct FGeo {
  static_assert(P16 >= 1 && P16 <= 4, "narrow variants: p <= 64");
  static constexpr int NRB = P16 <= 2 ? 64 : 32;     // rows per block
  static constexpr int NW = P16 == 2 ? 4 : 8;        // waves per workgroup, one workgroup per CU
  static constexpr int NBUF = P16 <= 2 ? 3 : 2;      // ring depth per wave
  static constexpr int LPR = 64 / NRB;               // row-stage lanes per row
  static constexpr int NC = 16 * P16;                // padded columns
  static constexpr int T = P16 * (P16 + 1) / 2;      // lower-triangular 16 x 16 tiles
  static constexpr int CPI = 256 / NRB;              // columns per DMA wave-instruction (1 KiB)
  static constexpr int SLOTS = NRB / 4;              // 16-byte slots per column
  static constexpr int DMA_X = NC / CPI;             // column-group wave-instructions per block
  static constexpr int DMA_V = (4 * NRB * 8) / 1024; // y | m | offset | prior wave-instructions per block
  static constexpr int LPER = NRB == 64 ? 4 : 2;     // period of the swizzle over column groups
  static constexpr int BSTR = 16 * NRB;              // floats between 16-column blocks (no pad)
  static constexpr int XF = NC * NRB;                // floats of X per buffer
  static constexpr int BUF = XF / 2 + 4 * NRB;       // doubles per buffer: X | y, m, offset, prior
  static constexpr int WAVE_LDS = NBUF * BUF;        // doubles per wave
  static constexpr int PSZ = T * 256 + NC + 5;       // one wave partial (tiles | X'Wz | 5 scalars)
  static constexpr int LDS = (NW * WAVE_LDS > (NW / 2) * PSZ) ? NW * WAVE_LDS : (NW / 2) * PSZ;
  static constexpr int DMA_BLOCK = DMA_X + DMA_V;
  static constexpr int younger(int blocks, int eta_stores) { return blocks * DMA_BLOCK + eta_stores; }
  static_assert(LPER <= DMA_X && DMA_X % LPER == 0, "whole swizzle periods");
  static_assert((LDS + 2 * POIS_TAB + 8) * 8 <= 160 * 1024, "LDS budget, the Poisson tables included");
  static_assert(younger(NBUF - 1, NBUF - 1) < 64, "vmcnt range");
};
static_assert(FGeo<1>::younger(2, 2) == 14 && FGeo<2>::younger(2, 0) == 20 && FGeo<4>::younger(1, 1) == 10,
              "the header's vmcnt table");

// slot permutation of column c (the header's f)
template <int NRB>
__device__ __forceinline__ constexpr int fsw(int c) { return NRB == 64 ? (c & 15) : ((c & 7) ^ ((c >> 3) & 1)); }

// IRLS / STATS / T4 as irls_narrow_kernel's; PassArgs::X32 is the design, PassArgs::ld its leading
// dimension in floats (a multiple of 64: the last 64-row block of a shard whose n_pad is an odd multiple
// of RB reads zero rows of X; its row vectors are re-read from the 32 rows before, never past n_pad).
template <int P16, int FAM, int LNK, bool IRLS, bool STATS = false, bool T4 = false>
__global__ void __launch_bounds__(64 * FGeo<P16>::NW, 1) irls_narrow_f32_kernel(PassArgs a) {
  using G = FGeo<P16>;
  constexpr int NRB = G::NRB, LPR = G::LPR, CPL = G::NC / LPR, NBUF = G::NBUF;
  constexpr bool PTAB = !IRLS && FAM == FAM_POISSON;
  constexpr bool YTAB = IRLS && (FAM == FAM_POISSON || FAM == FAM_NEGBIN) && LNK == LNK_LOG;
  __shared__ double lds[G::LDS + (PTAB ? 2 * POIS_TAB + 8 : (YTAB ? POIS_TAB : 0))];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* wl = lds + wv * G::WAVE_LDS;
  double* ptab = lds + G::LDS;           // PTAB: [2][POIS_TAB]; YTAB: [POIS_TAB]
  double* pconst = ptab + 2 * POIS_TAB;  // init_const (PTAB)
  const double* ylogy = YTAB ? ptab : nullptr;
  fill_poisson_tables<FAM, LNK, PTAB, YTAB, 64 * G::NW>(ptab, a);

  const int64_t n_pad = a.nblocks * RB;
  const int64_t nb = (n_pad + NRB - 1) / NRB;  // NRB-row blocks
  const int64_t gw = (int64_t)blockIdx.x * G::NW + wv, nwt = (int64_t)gridDim.x * G::NW;
  const int64_t b0 = nb * gw / nwt, b1 = nb * (gw + 1) / nwt;
  const int ngrp_stored = ((a.p + 7) / 8 * 8) / G::CPI;  // X stores whole column octets
  constexpr bool irls = IRLS;
  const int mode = IRLS ? (int)MODE_IRLS : a.mode;
  const bool has_eta = irls && !STATS && a.eta_out != nullptr;
  constexpr bool INIT_CONST = !IRLS && (FAM == FAM_POISSON || FAM == FAM_GAMMA);
  constexpr bool XS = STATS || INIT_CONST;  // the extra scalar accumulators are live
  using SL = StatsSlots<FAM>;

  // DMA sources of the next block to stage (blocks are staged in order from b0): lane -> (column cc of
  // the group, slot j); one 64-bit pointer per swizzle class
  const float* dsrc[G::LPER];
  {
    const int cc = lane / G::SLOTS, j = lane % G::SLOTS;
#pragma unroll
    for (int o = 0; o < G::LPER; ++o)
      dsrc[o] = a.X32 + b0 * NRB + (int64_t)cc * a.ld + 4 * (j ^ fsw<NRB>(G::CPI * o + cc));
  }
  // row vectors: instruction k carries 2 / LPR of the four vectors, NRB / 2 lanes (2 rows each) per vector
  const double* vsrc[G::DMA_V];
  const int vr2 = 2 * (lane % (NRB / 2));
#pragma unroll
  for (int k = 0; k < G::DMA_V; ++k) {
    const int v = k * (128 / NRB) + lane / (NRB / 2);  // 0 y, 1 m, 2 offset, 3 prior (absent: y again)
    const double* p = a.y;
    if (v == 1 && a.m) p = a.m;
    if (v == 2 && a.off) p = a.off;
    if (v == 3 && a.prior) p = a.prior;
    vsrc[k] = p + vr2;
  }
  int64_t vrow = b0 * NRB;  // first row of the next block to stage
  // row stage: lane (g, rl), g < LPR, covers columns LPR u + g of row rl
  const int g = lane / NRB, rl = lane % NRB;
  double bcol[CPL];
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const int c = LPR * u + g;
    bcol[u] = (a.beta && c < a.p) ? a.beta[c] : 0.0;
    // LPR = 1: beta is wave-uniform and would live in SGPRs, which then spill (2 CPL of them); VGPRs are free here
    if constexpr (LPR == 1) asm volatile("" : "+v"(bcol[u]));
  }

  d4 acc[G::T];
#pragma unroll
  for (int t = 0; t < G::T; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  double xz[P16];
#pragma unroll
  for (int b = 0; b < P16; ++b) xz[b] = 0.0;
  double s_dev = 0.0, s_aux = 0.0, s_pear = 0.0, s_ll = 0.0, s_bad = 0.0;

  const int cl = lane & 15, rq = lane >> 4;
  const bool do_gram = !a.no_gram;
  // eta reads (floats): column c = LPR u + g at (c >> 4) BSTR + (c & 15) NRB + 4 ((rl >> 2) ^ f(c)) + (rl & 3);
  // for u = EC j + k the lane part depends on k only, j moves by BSTR (immediate)
  constexpr int EC = 16 / LPR;
  int eoff[EC];
#pragma unroll
  for (int k = 0; k < EC; ++k) {
    const int c = LPR * k + g;
    eoff[k] = c * NRB + 4 * ((rl >> 2) ^ fsw<NRB>(c)) + (rl & 3);
  }
  // Gram operand reads: lane (rq, cl) reads the slot of rows 16 q + 4 rq .. + 3 of column 16 b + cl
  int goff[NRB / 16];
#pragma unroll
  for (int q = 0; q < NRB / 16; ++q) goff[q] = cl * NRB + 4 * ((4 * q + rq) ^ fsw<NRB>(cl));

  // DMA of the next block into buffer BUFI: DMA_X + DMA_V wave-instructions, always (the header's vmcnt).
  // Non-temporal in the IRLS passes (a shard streamed once per pass), the default in the initial pass.
  auto stage_next = [&](auto bufc) {
    constexpr int BUFI = decltype(bufc)::value;
    double* dst = wl + BUFI * G::BUF;
    int64_t cs = (int64_t)G::CPI * a.ld;
    asm volatile("" : "+s"(cs));  // keeps the groups' offsets on the scalar unit, formed here (narrow.hip)
    int64_t co = 0;
#pragma unroll
    for (int o = 0; o < G::DMA_X; ++o) {
      if (o > 0 && o < ngrp_stored) co += cs;  // uniform: groups past the stored columns repeat the last
      __builtin_amdgcn_global_load_lds((const void*)(dsrc[o % G::LPER] + co), (lds_void*)((float*)dst + o * 256), 16, 0,
                                       IRLS ? DMA_NT : 0);
    }
#pragma unroll
    for (int o = 0; o < G::LPER; ++o) dsrc[o] += NRB;
    // the last 64-row block of a shard may pass n_pad by RB rows: those lanes re-read the RB rows before
    const int64_t ro = (NRB == 64 && vrow + vr2 >= n_pad) ? vrow - RB : vrow;
#pragma unroll
    for (int k = 0; k < G::DMA_V; ++k)
      __builtin_amdgcn_global_load_lds((const void*)(vsrc[k] + ro), (lds_void*)(dst + G::XF / 2 + 128 * k), 16, 0,
                                       IRLS ? DMA_NT : 0);
    vrow += NRB;
  };
  // eta: every LDS read of the row's columns issued before the first FMA; each x widened once
  auto eta_of = [&](const float* xs) {
    double e4[4] = {0.0, 0.0, 0.0, 0.0};
    float xv[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) xv[u] = xs[eoff[u % EC] + (u / EC) * G::BSTR];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < CPL; ++u) e4[u & 3] += (double)xv[u] * bcol[u];
    double e = (e4[0] + e4[1]) + (e4[2] + e4[3]);
    if constexpr (LPR == 2) e = xor32_sum(e);
    return e;
  };
  const bool hm = a.m != nullptr, ho = a.off != nullptr, hp = a.prior != nullptr;

  auto block = [&](auto bufc, int64_t blk) {
    constexpr int BUFI = decltype(bufc)::value;
    __builtin_amdgcn_s_setprio(PRIO_ROWS);
    // block blk landed; what may still fly: the header's vmcnt
    if (blk + NBUF - 1 >= b1) wait_vm<0>();
    else if (has_eta && blk - b0 >= NBUF - 1) wait_vm<G::younger(NBUF - 1, NBUF - 1)>();
    else wait_vm<G::younger(NBUF - 1, 0)>();
    double* vv = wl + BUFI * G::BUF + G::XF / 2;
    const float* xs = (const float*)(wl + BUFI * G::BUF);

    // ---- row stage: one row per lane (NRB = 64) or per lane pair (NRB = 32) ----
    double eta = irls ? eta_of(xs) : 0.0;
    // absent vectors' slots hold y (finite): read unconditionally, selected
    const double yv = vv[rl];
    const double m1 = vv[NRB + rl], o1 = vv[2 * NRB + rl], p1 = vv[3 * NRB + rl];
    const double mv = hm ? m1 : 1.0, ov = ho ? o1 : 0.0, pv = hp ? p1 : 1.0;
    if (irls) eta = eta + ov;
    if (LPR == 1 || lane < NRB) {
      const int64_t row = blk * NRB + rl;
      // one store per block, always issued (every block starts below n_pad)
      if (has_eta && row < n_pad) a.eta_out[row] = eta;
      double w = 0.0, wz = 0.0;
      if (row < a.n) {
        if constexpr (STATS)
          pass_row_stats<FAM>(eta, yv, ov, pv, w, wz, s_dev, s_aux, s_pear, s_ll, s_bad, true, ylogy);
        else if (!(PTAB && poisson_init_row(pconst, ptab, yv, ov, pv, w, wz, s_dev, s_aux, s_ll))) {
          pass_row(FAM, LNK, mode, eta, yv, mv, ov, pv, a.mu0, a.ybar, a.m != nullptr, w, wz, s_dev, s_aux, true,
                   !IRLS, ylogy, a.link, a.theta);
          if constexpr (INIT_CONST) s_ll += init_stats_const<FAM>(yv, pv);
        }
      }
      // over the block's y and m slots (read above by this wave)
      vv[rl] = w;
      vv[NRB + rl] = wz;
    }

    // ---- Gramian: NRB / 16 operand reads of 4 k-steps each ----
    __builtin_amdgcn_s_setprio(PRIO_GRAM);
    if (do_gram) {
#pragma unroll
      for (int q = 0; q < NRB / 16; ++q) {
        f4 xf[P16];
#pragma unroll
        for (int b = 0; b < P16; ++b) xf[b] = *(const f4*)(xs + goff[q] + G::BSTR * b);
        const d2* wp = (const d2*)(vv + 16 * q + 4 * rq);
        const d2* zp = (const d2*)(vv + NRB + 16 * q + 4 * rq);
        const d2 w01 = wp[0], w23 = wp[1], z01 = zp[0], z23 = zp[1];
        const double wr[4] = {w01[0], w01[1], w23[0], w23[1]}, wzr[4] = {z01[0], z01[1], z23[0], z23[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // (LMX = false: no X'1 sums here, so the x1 argument is never read -- nullptr stands in)
          weighted_kstep<T4, false>(acc, xz, nullptr, [&](int b) { return (double)xf[b][i]; }, wr[i], wzr[i]);
        }
      }
    }
    // every LDS read of this buffer has returned before the DMA may overwrite it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (blk + NBUF < b1) stage_next(bufc);
  };

  if (b0 < b1) stage_next(std::integral_constant<int, 0>{});
  if (b0 + 1 < b1) stage_next(std::integral_constant<int, 1>{});
  if constexpr (NBUF > 2)
    if (b0 + 2 < b1) stage_next(std::integral_constant<int, 2>{});
#pragma unroll 1
  for (int64_t blk = b0; blk < b1; blk += NBUF) {
    block(std::integral_constant<int, 0>{}, blk);
    if (blk + 1 < b1) block(std::integral_constant<int, 1>{}, blk + 1);
    if constexpr (NBUF > 2)
      if (blk + 2 < b1) block(std::integral_constant<int, 2>{}, blk + 2);
  }

  // ---- wave partial: X'Wz over the 4 row lanes of each column, scalars over the wave ----
#pragma unroll
  for (int b = 0; b < P16; ++b) xz[b] = xor32_sum(xor16_sum(xz[b]));
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    s_dev += __shfl_xor(s_dev, o);
    s_aux += __shfl_xor(s_aux, o);
    if constexpr (XS) {
      s_pear += __shfl_xor(s_pear, o);
      s_ll += __shfl_xor(s_ll, o);
      s_bad += __shfl_xor(s_bad, o);
    }
  }

  // ---- fixed-order fold over the NW waves in LDS (narrow.hip's tree), one partial per workgroup ----
  wait_vm<0>();
  __syncthreads();
#pragma unroll 1
  for (int n = G::NW; n > 1;) {
    const int h = (n + 1) / 2;
    if (wv >= h && wv < n) {
      double* reg = lds + (wv - h) * G::PSZ;
#pragma unroll
      for (int t = 0; t < G::T; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) reg[t * 256 + 64 * j + lane] = acc[t][j];
      if (lane < 16) {
#pragma unroll
        for (int b = 0; b < P16; ++b) reg[G::T * 256 + 16 * b + lane] = xz[b];
      }
      if (lane == 0) {
        reg[G::T * 256 + G::NC] = s_dev;
        reg[G::T * 256 + G::NC + 1] = s_aux;
        reg[G::T * 256 + G::NC + 2] = s_pear;
        reg[G::T * 256 + G::NC + 3] = s_ll;
        reg[G::T * 256 + G::NC + 4] = s_bad;
      }
    }
    __syncthreads();
    if (wv < n - h) {
      const double* reg = lds + wv * G::PSZ;
#pragma unroll
      for (int t = 0; t < G::T; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] += reg[t * 256 + 64 * j + lane];
#pragma unroll
      for (int b = 0; b < P16; ++b) xz[b] += reg[G::T * 256 + 16 * b + (lane & 15)];
      s_dev += reg[G::T * 256 + G::NC];
      s_aux += reg[G::T * 256 + G::NC + 1];
      if constexpr (XS) {
        s_pear += reg[G::T * 256 + G::NC + 2];
        s_ll += reg[G::T * 256 + G::NC + 3];
        s_bad += reg[G::T * 256 + G::NC + 4];
      }
    }
    __syncthreads();
    n = h;
  }
  if (wv == 0) {
    double* out = a.partials + (int64_t)blockIdx.x * a.stride;
#pragma unroll
    for (int t = 0; t < G::T; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) out[t * 256 + 64 * j + lane] = acc[t][j];
    if (lane < 16) {
#pragma unroll
      for (int b = 0; b < P16; ++b) out[G::T * 256 + 16 * b + lane] = xz[b];
    }
    if (lane < NS) {
      double v = lane == S_DEV ? s_dev : lane == S_SUMW ? s_aux : 0.0;
      if constexpr (STATS) {
        if (lane == SL::S2) v = s_pear;
        if (lane == SL::S3) v = s_ll;
        if (lane == SL::S4) v = s_bad;
      }
      if constexpr (INIT_CONST) {
        if (lane == S_AUX2) v = s_ll;
      }
      out[G::T * 256 + G::NC + lane] = v;
    }
  }
}

template <int P16, int FAM, int LNK>
void launch_f32_fl(const PassArgs& a, dim3 gr, dim3 bl, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  constexpr bool SP = stats_in_pass_family(FAM, LNK);
  if constexpr (P16 == 2 && FAM == FAM_GAUSSIAN) {  // gaussian at p <= 20 (gram_kstep T4)
    if (a.p <= 20) {
      if (a.mode == MODE_IRLS)
        hipExtLaunchKernelGGL((irls_narrow_f32_kernel<P16, FAM, LNK, true, false, true>), gr, bl, 0, st, e0, e1, 0, a);
      else
        hipExtLaunchKernelGGL((irls_narrow_f32_kernel<P16, FAM, LNK, false, false, true>), gr, bl, 0, st, e0, e1, 0, a);
      return;
    }
  }
  if (a.mode == MODE_IRLS && SP && a.stats_in_pass && !(FAM == FAM_BINOMIAL && a.m))
    hipExtLaunchKernelGGL((irls_narrow_f32_kernel<P16, FAM, LNK, true, SP>), gr, bl, 0, st, e0, e1, 0, a);
  else if (a.mode == MODE_IRLS)
    hipExtLaunchKernelGGL((irls_narrow_f32_kernel<P16, FAM, LNK, true>), gr, bl, 0, st, e0, e1, 0, a);
  else
    hipExtLaunchKernelGGL((irls_narrow_f32_kernel<P16, FAM, LNK, false>), gr, bl, 0, st, e0, e1, 0, a);
}

template <int P16>
hipError_t launch_f32_p(const PassArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const dim3 gr(grid), bl(64 * FGeo<P16>::NW);
  const bool ok = dispatch_family_link(a.family, a.link, [&](auto F, auto L) {
    launch_f32_fl<P16, decltype(F)::value, decltype(L)::value>(a, gr, bl, st, e0, e1);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// dst [rows x cols, ld ldd] = src [ld lds] converted (double -> float rounds to nearest even)
template <class TS, class TD>
__global__ void convert_kernel(const TS* __restrict__ src, int64_t lds, TD* __restrict__ dst, int64_t ldd, int64_t rows,
                               int cols) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x)
    for (int c = 0; c < cols; ++c) dst[(int64_t)c * ldd + i] = (TD)src[(int64_t)c * lds + i];
}

template <class TS, class TD>
hipError_t launch_convert(const TS* src, int64_t lds, TD* dst, int64_t ldd, int64_t rows, int cols, hipStream_t st) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>(65536, (rows + 255) / 256);
  hipLaunchKernelGGL((convert_kernel<TS, TD>), dim3((unsigned)blocks), dim3(256), 0, st, src, lds, dst, ldd, rows, cols);
  return hipGetLastError();
}

}  // namespace

int narrow_f32_rows_per_wg(int P16) {
  switch (P16) {
    case 1: return FGeo<1>::NRB * FGeo<1>::NW;
    case 2: return FGeo<2>::NRB * FGeo<2>::NW;
    case 3: return FGeo<3>::NRB * FGeo<3>::NW;
    default: return FGeo<4>::NRB * FGeo<4>::NW;
  }
}

hipError_t launch_narrow_f32(int P16, const PassArgs& a, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (!a.X32 || a.ld % 64 != 0 || a.mode == MODE_LM_GRAM || a.mode == MODE_LM_RESID) return hipErrorInvalidValue;
  switch (P16) {
    case 1: return launch_f32_p<1>(a, grid, st, e0, e1);
    case 2: return launch_f32_p<2>(a, grid, st, e0, e1);
    case 3: return launch_f32_p<3>(a, grid, st, e0, e1);
    case 4: return launch_f32_p<4>(a, grid, st, e0, e1);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_round_f32(const double* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int cols,
                            hipStream_t st) {
  return launch_convert(src, lds, dst, ldd, rows, cols, st);
}
hipError_t launch_widen_f32(const float* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int cols,
                            hipStream_t st) {
  return launch_convert(src, lds, dst, ldd, rows, cols, st);
}

}  // namespace sglm
