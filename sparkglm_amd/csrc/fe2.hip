// fe2.hip -- the kernels of the two-way fixed-effects IRLS: a second absorbed factor beside the cluster
// factor (gfx950; fe2.cpp).  No floating-point atomics: every sum is formed per chunk (or
// segment) in list order and joined by cluster.hip's combine tree, so every order of summation is a function
// of (ids1, ids2, n, p) alone.
//
// fe2_list_sum_kernel   R[k, :] = sum over chunk k of factor 2's row list of [w x | w z | w].  One wave per
//   (chunk, 64-column slab): segment_sum_kernel's structure with the 32 staged rows addressed through the
//   list -- lane l loads row l % 32 of column 2 q + l / 32, the products go transposed into LDS (row stride
//   65 doubles), the next 32 rows are loaded into registers before the walk, and in the walk a lane owns a
//   column and adds the staged rows in list order.  The two row vectors ride along as columns p and p + 1:
//   w z and w (the check: y and m - y), which fe.hip's fe_weights_kernel stored per row -- no kernel here
//   evaluates a row's family or link.
// fe2_gather_kernel     R[k, :] = sum over unit k of v_i src[id_i, :], src a row-major level matrix: one wave
//   per (unit, slab), a lane owns a column, every gathered row is one contiguous read.  The units are the
//   segments of the cluster factor (rows consecutive) or the chunks of factor 2's list.
// fe2_update_kernel     one thread per (level, column): the Gauss-Seidel update of a level's coefficients and
//   the stop rule's maxima -- a fixed tree within the workgroup, then an integer max on the bit patterns of
//   the non-negative doubles, which is order-independent.
// fe2_cross_kernel      S_X' Y over the levels on v_mfma_f64_16x16x4_f64: one wave per (slice of levels,
//   16 x 16 tile); fe2_cross_reduce_kernel adds the slices in ascending order.
// Every index a kernel reads (list, id) was validated on the host when the factor was declared.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace sglm {

namespace {

constexpr int F2_SUB = 32;  // rows staged per step
constexpr int F2_LDW = 65;  // LDS row stride in doubles
constexpr int F2_WG_PER_CU = 16;
static_assert(FE2_CHUNK % F2_SUB == 0, "chunks are whole staged steps");

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64) fe2_list_sum_kernel(Fe2ListSumArgs a) {
  __shared__ double xs[F2_SUB * F2_LDW];
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int pc = a.p + 2;
  const int nslab = (pc + 63) / 64;
  const int64_t units = a.nchunk * nslab;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t k = a.order ? a.order[unit / nslab] : unit / nslab;
    const int c0 = (int)(unit % nslab) * 64;
    const int nc = min(64, pc - c0);
    const int64_t q0 = a.chunk_start[k], q1 = a.chunk_start[k + 1];
    double v[32];
    // the staged values of positions [s0, s0 + 32): a position past the chunk reads nothing
    auto stage = [&](int64_t s0) {
      const int64_t q = s0 + r;
      const bool ok = q < q1;
      const int64_t row = ok ? a.list[q] : 0;
      const double u = ok && a.p > 0 ? a.v[row] : 0.0;
#pragma unroll
      for (int t = 0; t < 32; ++t) {
        const int cc = c0 + 2 * t + h;
        double x = 0.0;
        if (ok) {
          if (cc < a.p) x = u * a.X[(int64_t)cc * a.ld + row];
          else if (cc == a.p) x = a.r0[row];
          else if (cc == a.p + 1) x = a.r1[row];
        }
        v[t] = x;
      }
    };
    stage(q0);
    double acc = 0.0;
    for (int64_t s0 = q0; s0 < q1; s0 += F2_SUB) {
      __syncthreads();  // the previous step's walk has read xs
#pragma unroll
      for (int t = 0; t < 32; ++t) xs[r * F2_LDW + 2 * t + h] = v[t];
      __syncthreads();
      if (s0 + F2_SUB < q1) stage(s0 + F2_SUB);
      const int nr = (int)min((int64_t)F2_SUB, q1 - s0);
      for (int i = 0; i < nr; ++i) acc += xs[i * F2_LDW + lane];
    }
    if (lane < nc) a.R[k * pc + c0 + lane] = acc;
  }
}

__global__ void __launch_bounds__(64) fe2_gather_kernel(Fe2GatherArgs a) {
  const int lane = threadIdx.x;
  const int nslab = (a.nc + 63) / 64;
  const int64_t units = a.nunit * nslab;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t k = a.order ? a.order[unit / nslab] : unit / nslab;
    const int col = (int)(unit % nslab) * 64 + lane;
    const bool on = col < a.nc;
    const int64_t q0 = a.start[k], q1 = a.start[k + 1];
    double acc = 0.0;
    int64_t q = q0;
    // four rows in flight: the ids and weights first, then the four gathered rows; added in list order
    for (; q + 4 <= q1; q += 4) {
      int64_t row[4];
      double u[4], x[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) row[t] = a.list ? a.list[q + t] : q + t;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        u[t] = a.v[row[t]];
        x[t] = on ? a.src[(int64_t)a.id[row[t]] * a.lds + col] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = fma(u[t], x[t], acc);
    }
    for (; q < q1; ++q) {
      const int64_t row = a.list ? a.list[q] : q;
      const double x = on ? a.src[(int64_t)a.id[row] * a.lds + col] : 0.0;
      acc = fma(a.v[row], x, acc);
    }
    if (on) a.R[k * a.nc + col] = acc;
  }
}

__global__ void __launch_bounds__(256) fe2_update_kernel(Fe2UpdateArgs a) {
  __shared__ unsigned long long sd[256], sm[256];
  const int j = blockIdx.y;  // column: p is z
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double d = 0.0, mag = 0.0;
  if (l < a.L) {
    const double W = a.S[(int64_t)(a.p + 1) * a.ldS + l];
    double y = 0.0;
    if (W > 0.0 && !(a.pin && a.pin[l])) y = (a.S[(int64_t)j * a.ldS + l] - a.T[(int64_t)j * a.ldS + l]) / W;
    const double old = a.Y[l * a.ldy + j];
    a.Y[l * a.ldy + j] = y;
    d = fabs(y - old);
    mag = fabs(y);
  }
  // non-negative doubles order as their bit patterns do (a NaN above every number: it reaches the host)
  sd[threadIdx.x] = (unsigned long long)__double_as_longlong(d);
  sm[threadIdx.x] = (unsigned long long)__double_as_longlong(mag);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sd[threadIdx.x] = max(sd[threadIdx.x], sd[threadIdx.x + s]);
      sm[threadIdx.x] = max(sm[threadIdx.x], sm[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMax(&a.stop[j], sd[0]);
    atomicMax(&a.stop[a.ldy + j], sm[0]);
  }
}

__global__ void __launch_bounds__(64) fe2_cross_kernel(Fe2CrossArgs a, int ntj, int PR, int PC) {
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int ti = (int)blockIdx.y / ntj, tj = (int)blockIdx.y % ntj;
  const int f = s < a.nslice[0] ? 0 : 1;
  const int64_t sl = f ? s - a.nslice[0] : s;
  const int64_t k0 = sl * a.slice_rows[f], k1 = min(k0 + a.slice_rows[f], a.L[f]);
  const int i = ti * 16 + (lane & 15), jc = tj * 16 + (lane & 15), kk = lane >> 4;
  const double* S = a.S[f];
  const double* Y = a.Y[f];
  const int64_t ldS = a.ldS[f];
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  // A[i][k] = S[level k, column i] (lane: i = lane & 15, k = lane >> 4), B[k][j] = Y[level k, column j]
  for (int64_t k = k0; k < k1; k += 4) {
    const int64_t kr = k + kk;
    const bool ok = kr < k1;
    const double av = ok && i < a.p ? S[(int64_t)i * ldS + kr] : 0.0;
    const double bv = ok && jc <= a.p ? Y[kr * a.ldy + jc] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
  // D: column = lane & 15, row = (lane >> 4) + 4 reg
  double* out = a.part + (int64_t)s * PR * PC;
#pragma unroll
  for (int t = 0; t < 4; ++t) out[(int64_t)(ti * 16 + (lane >> 4) + 4 * t) * PC + tj * 16 + (lane & 15)] = acc[t];
}

__global__ void __launch_bounds__(256) fe2_cross_reduce_kernel(const double* part, int nslice, int64_t len, double* out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= len) return;
  double s = 0.0;
  for (int k = 0; k < nslice; ++k) s += part[(int64_t)k * len + t];
  out[t] = s;
}

__global__ void __launch_bounds__(256) fe2_offset_kernel(Fe2OffsetArgs a) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < a.ld; row += (int64_t)gridDim.x * 256)
    a.out[row] = row < a.n ? ((a.off ? a.off[row] : 0.0) + a.alpha[a.id1[row]]) + a.gamma[a.id2[row]] : 0.0;
}

__global__ void __launch_bounds__(256) fe2_effect_kernel(Fe2EffectArgs a) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= a.L || !(a.W[l] > 0.0)) return;  // no weight: the effect is not identified and stays what it was
  const double* y = a.Y + l * a.ldy;
  double dot = 0.0;
  for (int j = 0; j < a.p; ++j) dot = fma(y[j], a.beta[j], dot);
  a.eff[l] += y[a.p] - dot;
}

__global__ void __launch_bounds__(256) fe2_normalise_kernel(Fe2NormArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.G + a.H) return;
  const int c = t < a.G ? a.comp1[t] : a.comp2[t - a.G];
  if (c < 0) return;
  const double shift = a.gamma_raw[a.low[c]];
  if (t < a.G) a.alpha[t] += shift;
  else a.gamma[t - a.G] = a.gamma_raw[t - a.G] - shift;
}

__global__ void __launch_bounds__(256) fe2_meat_kernel(Fe2MeatArgs a) {
  const int64_t total = a.ld * (a.p + 1);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t g = t % a.ld;
    const int j = (int)(t / a.ld);
    if (j == a.p) {
      a.y[g] = 0.0;
      continue;
    }
    double v = 0.0;
    if (g < a.G) v = (a.Su[t] - a.Su[(int64_t)a.p * a.ld + g] * a.Y1[g * a.ldy + j]) - a.Tu[t];
    a.X[t] = v;
  }
}

inline unsigned blocks_of(int64_t n, int64_t cap = 65536) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
}

}  // namespace

// one wave per unit until the device is full: nothing depends on the grid
int fe2_grid(int ncu, int64_t units) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)ncu * F2_WG_PER_CU));
}

hipError_t launch_fe2_list_sum(const Fe2ListSumArgs& a, int ncu, hipStream_t st) {
  if (a.p < 0 || (a.p > 0 && (!a.X || !a.v)) || !a.r0 || !a.r1 || !a.list || !a.chunk_start || !a.R)
    return hipErrorInvalidValue;
  if (a.nchunk < 1) return hipSuccess;
  const int64_t units = a.nchunk * ((a.p + 2 + 63) / 64);
  hipLaunchKernelGGL(fe2_list_sum_kernel, dim3(fe2_grid(ncu, units)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_gather(const Fe2GatherArgs& a, int ncu, hipStream_t st) {
  if (a.nc < 1 || !a.v || !a.id || !a.src || !a.start || !a.R) return hipErrorInvalidValue;
  if (a.nunit < 1) return hipSuccess;
  const int64_t units = a.nunit * ((a.nc + 63) / 64);
  hipLaunchKernelGGL(fe2_gather_kernel, dim3(fe2_grid(ncu, units)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_update(const Fe2UpdateArgs& a, hipStream_t st) {
  if (a.L < 1 || a.p < 0 || !a.S || !a.T || !a.Y || !a.stop || (a.L + 255) / 256 > 0x7fffffff)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe2_update_kernel, dim3((unsigned)((a.L + 255) / 256), (unsigned)(a.p + 1)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_cross(const Fe2CrossArgs& a, double* out, hipStream_t st) {
  if (a.p < 1 || !a.part || !out || a.nslice[0] < 0 || a.nslice[1] < 0 || a.nslice[0] + a.nslice[1] < 1)
    return hipErrorInvalidValue;
  const int nti = (a.p + 15) / 16, ntj = (a.p + 1 + 15) / 16;
  const int PR = 16 * nti, PC = 16 * ntj, ns = a.nslice[0] + a.nslice[1];
  hipLaunchKernelGGL(fe2_cross_kernel, dim3((unsigned)ns, (unsigned)(nti * ntj)), dim3(64), 0, st, a, ntj, PR, PC);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t len = (int64_t)PR * PC;
  hipLaunchKernelGGL(fe2_cross_reduce_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, a.part, ns, len, out);
  return hipGetLastError();
}

hipError_t launch_fe2_offset(const Fe2OffsetArgs& a, hipStream_t st) {
  if (a.ld < 1 || !a.alpha || !a.gamma || !a.id1 || !a.id2 || !a.out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe2_offset_kernel, dim3(blocks_of(a.ld)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_effect(const Fe2EffectArgs& a, hipStream_t st) {
  if (a.L < 1 || !a.Y || !a.W || !a.beta || !a.eff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe2_effect_kernel, dim3(blocks_of(a.L, (int64_t)1 << 30)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_normalise(const Fe2NormArgs& a, hipStream_t st) {
  if (a.G + a.H < 1 || !a.alpha || !a.gamma || !a.gamma_raw || !a.comp1 || !a.comp2 || !a.low)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe2_normalise_kernel, dim3(blocks_of(a.G + a.H, (int64_t)1 << 30)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_fe2_meat(const Fe2MeatArgs& a, hipStream_t st) {
  if (a.ld < 1 || !a.Su || !a.Tu || !a.Y1 || !a.X || !a.y) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fe2_meat_kernel, dim3(blocks_of(a.ld * (a.p + 1))), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sglm
