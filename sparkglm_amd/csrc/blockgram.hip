// blockgram.hip -- every block of a block-structured weighted Gram from one read of X (gfx950; multinom.cpp;
// DESIGN.md 4, K16): G_jk = sum_i omega_jk(i) x_i x_i' for the M = K (K - 1) / 2 pairs 1 <= j <= k <= K - 1 of a
// multinomial model on a resident design with p <= 64, 2 <= K <= 16.
//
//   BG_HESS  omega_jj = pw pi_j sum_{l != j} pi_l (no 1 - pi_j),  omega_jk = -pw pi_j pi_k: the Hessian's blocks
//   BG_MEAT  omega_jk = r_j r_k,  r_j = pw (1[y = j] - pi_j),  r_y = pw sum_{l != y} pi_l: the sandwich's meat
//
// One workgroup of 4 waves per CU streams a contiguous range of 64-row blocks.  A block is staged in LDS by
// LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, the instructions dealt over the four waves): X as
// two 32-row halves in narrow.hip's NRB = 32 image (column c at (c / 16) BSTR + (c % 16) 32, row r in slot
// r ^ 2 (c % 16), the swizzle applied on the source address: the MFMA operand reads are conflict-free ds_read_b64),
// and beside it the block's 64 rows of P_0 .. P_{K-1}, the prior weights and y -- coalesced, 512 B each.
//
// Weights.  A thread per row and wave per pair residue (m mod 4) forms omega_m(row) for the slice's pairs from the
// staged values in registers and leaves it in LDS as om[m][half][row % 4][row / 4 % 8]: lane (rq, cl) of the
// MFMA layout needs omega of row 4 s + rq of a half at k-step s, eight consecutive doubles that every one of its
// 16 lanes reads at the same address (a broadcast).  Nothing of omega goes to HBM.
//
// Gram.  v_mfma_f64_16x16x4_f64 with the rows as k, gram_kstep's operand layout: lane (rq, cl) holds
// xv[b] = X[row 4 s + rq][column 16 b + cl]; tile (bi, bj) of pair m accumulates (omega_m xv[bi]) x xv[bj].
// The (tile, pair) accumulators are dealt over the waves so that the tile of an accumulator slot is known at
// compile time and the pair at run time: slot (c, t) of wave w is tile t of pair 4 c + ((w - t) mod 4).  Every
// tile's pairs are spread over all four waves, rotated by the tile index, so M = 3 at P16 = 2 is 2, 2, 3, 2
// accumulators a wave and not three waves of three; a wave keeps its C T accumulators (C <= CMAX, 8 registers each,
// VGPRs and AGPRs under __launch_bounds__(256, 1)) for the whole launch.  The slice's pair count is a run-time
// argument; C is the bucket 1, 2, 4 or CMAX that holds ceil(count / 4), and the loop over c ends at the count.
//
// Pipeline: a ring of three staged blocks and two omega images, one barrier a block.  After the barrier of
// block i every wave has finished the Gram of block i - 1 and the weights of block i, and block i + 1 has landed
// (each wave waited for its own DMA instructions with vmcnt(0) before the barrier); then block i + 2 is issued
// into the buffer of block i - 1, the weights of block i + 1 are formed and the Gram of block i runs.
//
// Reduction: each workgroup stores its tiles to a.part [grid][stride], launch_part_sum adds them in a fixed order.
// No floating-point atomics; the grid depends on the shape and the device only: two calls are bitwise equal.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "waitcnt.hpp"

namespace sglm {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int BG_NW = 4;                // waves per workgroup
constexpr int BG_NT = 64 * BG_NW;
constexpr int BG_ROWS = 64;             // rows per staged block: two halves of 32
constexpr int BG_NBUF = 3;              // staged blocks in the ring
constexpr int BG_VSLOT = MN_MAX_K + 2;  // staged row vectors: P_0 .. P_{K-1}, the prior weights, y
constexpr int BG_VINST = 3;             // vector DMA instructions a wave issues at most (two vectors each)
static_assert(2 * BG_NW * BG_VINST >= BG_VSLOT && BG_VSLOT % 2 == 0, "every vector has an instruction");

// Pairs per tile and wave at most: C T accumulators of 8 registers a wave, 4 C pairs a slice.  From the compiler's
// resource report at build time (-Rpass-analysis=kernel-resource-usage), see DESIGN.md 4 K16 for the table; every
// instantiation is free of scratch.  P16 = 1, 2: the two omega images bound C (LDS), not the registers.
constexpr int bg_cmax(int P16) { return P16 == 1 ? 16 : P16 == 2 ? 15 : P16 == 3 ? 7 : 4; }

template <int P16>
struct BGeo {
  static_assert(P16 >= 1 && P16 <= 4, "block Gram: p <= 64");
  static constexpr int T = P16 * (P16 + 1) / 2;
  static constexpr int BSTR = 16 * 32 + 2;            // narrow.hip NGeo::BSTR at NRB = 32
  static constexpr int XSUB = P16 * BSTR;             // one 32-row half
  static constexpr int XB = 2 * XSUB;
  static constexpr int BUF = XB + BG_VSLOT * BG_ROWS;  // doubles per staged block
  static constexpr int XINST = 2 * P16;               // X DMA instructions per wave and block (4 columns x 32 rows)
};

template <int P16, int MODE, int C>
__global__ void __launch_bounds__(BG_NT, 1) block_gram_kernel(BlockGramArgs a) {
  using G = BGeo<P16>;
  constexpr int T = G::T, NP = 4 * C, OM = NP * BG_ROWS;
  static_assert((BG_NBUF * G::BUF + 2 * OM) * 8 + NP * 4 <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) double lds[BG_NBUF * G::BUF + 2 * OM];
  __shared__ int spair[NP];  // j | k << 8 of the slice's pair, 0 past its count
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K;
  if (tid < NP) {
    int v = 0;
    if (tid < a.cnt) {
      int m = a.m0 + tid, j = 1;
      while (m >= K - j) {
        m -= K - j;
        j += 1;
      }
      v = j | ((j + m) << 8);
    }
    spair[tid] = v;
  }
  const int64_t nb = (a.n + BG_ROWS - 1) / BG_ROWS;
  const int64_t b0 = nb * blockIdx.x / gridDim.x, b1 = nb * (blockIdx.x + 1) / gridDim.x;
  const int nblk = (int)(b1 - b0);
  const int64_t ld = a.ld;

  // ---- the DMA of one block: this wave's share of the X instructions and of the row vectors ----
  // X instruction o = 4 i + wv: half o & 1, column group o >> 1 (4 columns); lane -> column cc, row pair jr.
  // Groups past the stored column octets re-load the last stored group (their tiles are never unpacked).
  const int xh = wv & 1, xcc = lane >> 4, xjr = lane & 15;
  const int ngs = (a.p + 7) / 8 * 2;
  // vector instruction o = 4 i + wv: vectors 2 o and 2 o + 1; lane -> vector, row pair vr.  Vectors past y are y.
  const int nvi = (K + 3) / 2;
  const int vr = lane & 31;
  const double* vsrc[BG_VINST];
#pragma unroll
  for (int i = 0; i < BG_VINST; ++i) {
    const int v = 2 * (4 * i + wv) + (lane >> 5);
    const double* s = a.y;
    if (v < K) s = a.P + (int64_t)v * ld;
    else if (v == K && a.prior) s = a.prior;
    vsrc[i] = s + 2 * vr;
  }
  auto stage = [&](int buf, int64_t blk) {
    double* dst = lds + buf * G::BUF;
    // a half past the padded rows (ld is a multiple of 32, not of 64) re-loads the half before it: omega is 0 there
    int64_t xrow = blk * BG_ROWS + 32 * xh;
    if (xrow >= ld) xrow -= 32;
#pragma unroll
    for (int i = 0; i < G::XINST; ++i) {
      const int grp = 2 * i + (wv >> 1);
      const int gs = grp < ngs ? grp : ngs - 1;  // uniform
      const int c16 = 4 * (grp & 3) + xcc;
      const double* src = a.X + xrow + ((2 * xjr) ^ (2 * c16)) + (int64_t)(4 * gs + xcc) * ld;
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (lds_void*)(dst + xh * G::XSUB + (grp >> 2) * G::BSTR + (grp & 3) * 128), 16, 0,
                                       DMA_NT);
    }
    int64_t vrow = blk * BG_ROWS;
    if (vrow + 32 * (vr >> 4) >= ld) vrow -= 32;
#pragma unroll
    for (int i = 0; i < BG_VINST; ++i) {
      const int o = 4 * i + wv;
      if (o < nvi)  // uniform
        __builtin_amdgcn_global_load_lds((const void*)(vsrc[i] + vrow), (lds_void*)(dst + G::XB + o * 128), 16, 0, 0);
    }
  };

  // ---- omega of one staged block's rows: thread (wave wv, row lane) forms the pairs m = 4 c + wv ----
  const bool has_prior = a.prior != nullptr;
  const int oidx = (lane >> 5) * 32 + (lane & 3) * 8 + ((lane & 31) >> 2);
  auto weights = [&](int buf, int ob, int64_t blk) {
    const double* vv = lds + buf * G::BUF + G::XB + lane;
    double* om = lds + BG_NBUF * G::BUF + ob * OM + oidx;
    const double pw = has_prior ? vv[K * BG_ROWS] : 1.0;
    const bool live = blk * BG_ROWS + lane < a.n && pw > 0.0;
    int yc = 0;
    double sy = 0.0;
    if (MODE == BG_MEAT && live) {
      const double yv = vv[(K + 1) * BG_ROWS];
      yc = yv >= 0.0 && yv < (double)K ? (int)yv : 0;
      for (int l = 0; l < K; ++l)
        if (l != yc) sy += vv[l * BG_ROWS];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int m = 4 * c + wv;
      const int jk = spair[m];
      const int j = jk & 255, k = jk >> 8;  // uniform
      double w = 0.0;
      if (j != 0 && live) {
        const double pj = vv[j * BG_ROWS], pk = vv[k * BG_ROWS];
        if (MODE == BG_MEAT) {
          const double rj = pw * (j == yc ? sy : -pj);
          const double rk = pw * (k == yc ? sy : -pk);
          w = rj * rk;
        } else if (j == k) {
          double f = 0.0;
          for (int l = 0; l < K; ++l)
            if (l != j) f += vv[l * BG_ROWS];
          w = pw * (pj * f);
        } else {
          w = -(pw * (pj * pk));
        }
      }
      om[m * BG_ROWS] = w;
    }
  };

  // ---- the Gram of one staged block: 16 k-steps of 4 rows ----
  d4 acc[C][T];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int t = 0; t < T; ++t) acc[c][t] = d4{0.0, 0.0, 0.0, 0.0};
  const int cl = lane & 15, rq = lane >> 4;
  const int cn = (a.cnt + 3) / 4;  // the c in use
  int xoff[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) xoff[s] = cl * 32 + ((4 * s + rq) ^ (2 * cl));
  auto gram = [&](int buf, int ob) {
    const double* xs = lds + buf * G::BUF;
    const double* om = lds + BG_NBUF * G::BUF + ob * OM + rq * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        double xv[P16];
#pragma unroll
        for (int b = 0; b < P16; ++b) xv[b] = xs[h * G::XSUB + b * G::BSTR + xoff[s]];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (c >= cn) break;  // uniform
          int t = 0;
#pragma unroll
          for (int bi = 0; bi < P16; ++bi)
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj, ++t) {
              const int m = 4 * c + ((wv - t) & 3);
              const double w = om[m * BG_ROWS + h * 32 + s];
              acc[c][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w * xv[bi], xv[bj], acc[c][t], 0, 0, 0);
            }
        }
      }
  };

  if (nblk > 0) stage(0, b0);
  if (nblk > 1) stage(1, b0 + 1);
  wait_vm<0>();
  __syncthreads();  // (the pair table too)
  if (nblk > 0) weights(0, 0, b0);
  int buf = 0, nbuf = 2;  // the buffers of block it and of block it + 2
#pragma unroll 1
  for (int it = 0; it < nblk; ++it) {
    wait_vm<0>();
    __syncthreads();
    if (it + 2 < nblk) stage(nbuf, b0 + it + 2);
    const int buf1 = buf + 1 == BG_NBUF ? 0 : buf + 1;
    if (it + 1 < nblk) weights(buf1, (it + 1) & 1, b0 + it + 1);
    gram(buf, it & 1);
    nbuf = buf;
    buf = buf1;
  }

  double* out = a.part + (int64_t)blockIdx.x * a.stride;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int m = 4 * c + ((wv - t) & 3);
      if (m < a.cnt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(m * T + t) * BG_TILE + 64 * j + lane] = acc[c][t][j];
      }
    }
}

typedef void (*BgKernel)(BlockGramArgs);

// the bucket C = 1, 2, 4 or CMAX that holds c pairs per tile and wave
template <int P16, int MODE>
BgKernel bg_kernel(int c) {
  if (c <= 1) return block_gram_kernel<P16, MODE, 1>;
  if (c <= 2) return block_gram_kernel<P16, MODE, 2>;
  if (c <= 4) return block_gram_kernel<P16, MODE, 4>;
  return block_gram_kernel<P16, MODE, bg_cmax(P16)>;
}

template <int MODE>
BgKernel bg_kernel_p(int P16, int c) {
  switch (P16) {
    case 1: return bg_kernel<1, MODE>(c);
    case 2: return bg_kernel<2, MODE>(c);
    case 3: return bg_kernel<3, MODE>(c);
    case 4: return bg_kernel<4, MODE>(c);
    default: return nullptr;
  }
}

}  // namespace

// Where the block kernel measured faster than a weight kernel and a Gram pass per block pair (DESIGN.md 4 K16,
// profiles/multinom_bench.jsonl): K >= 4 at p <= 48.  At K = 2 and 3 a wave has too few accumulators to cover the
// barrier and the weights of a block (1.12 to 3.4 x the per-block route), and at p = 64 the kernel ran 1.19 x
// (K = 3) and 1.26 x (K = 8) the tuned passes' time.
bool blockgram_preferred(int P16, int K) { return P16 >= 1 && P16 <= 3 && K >= 4; }

int blockgram_pairs_per_slice(int P16) { return P16 >= 1 && P16 <= 4 ? 4 * bg_cmax(P16) : 0; }

int blockgram_slices(int P16, int K) {
  const int M = K * (K - 1) / 2, cap = blockgram_pairs_per_slice(P16);
  return cap ? (M + cap - 1) / cap : 0;
}

// the largest slice's tiles: the slices are as even as the count allows (the first M % slices take one more)
int64_t blockgram_stride(int P16, int K) {
  const int M = K * (K - 1) / 2, ns = blockgram_slices(P16, K);
  return ns ? (int64_t)((M + ns - 1) / ns) * (P16 * (P16 + 1) / 2) * BG_TILE : 0;
}

int blockgram_grid(int ncu, int64_t n) {
  const int64_t nb = std::min<int64_t>((n + BG_ROWS - 1) / BG_ROWS, (int64_t)1 << 30);
  return std::max(1, (int)std::min<int64_t>(nb, (int64_t)ncu));
}

hipError_t launch_blockgram(int mode, int P16, BlockGramArgs a, int grid, double* out, hipStream_t st) {
  const int K = a.K, M = K * (K - 1) / 2, ns = blockgram_slices(P16, K);
  if (ns == 0 || K < 2 || K > MN_MAX_K || a.p > 16 * P16 || a.n <= 0 || a.ld % RB != 0 || a.ld < a.n ||
      (mode != BG_HESS && mode != BG_MEAT))
    return hipErrorInvalidValue;
  const int T = P16 * (P16 + 1) / 2;
  a.stride = blockgram_stride(P16, K);
  int m0 = 0;
  for (int s = 0; s < ns; ++s) {
    a.m0 = m0;
    a.cnt = M / ns + (s < M % ns ? 1 : 0);
    const int c = (a.cnt + 3) / 4;
    BgKernel k = mode == BG_HESS ? bg_kernel_p<BG_HESS>(P16, c) : bg_kernel_p<BG_MEAT>(P16, c);
    hipLaunchKernelGGL(k, dim3(grid), dim3(BG_NT), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    const int len = a.cnt * T * BG_TILE;
    if (hipError_t e = launch_part_sum(a.part, grid, (int)a.stride, len, out + (int64_t)m0 * T * BG_TILE, st)) return e;
    m0 += a.cnt;
  }
  return hipSuccess;
}

}  // namespace sglm
