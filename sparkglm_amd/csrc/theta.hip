// theta.hip -- the negative binomial's theta by maximum likelihood (MASS::theta.ml).
//
// theta_terms_kernel makes one streaming read of y, the eta the last pass stored and the prior weights -- X is
// not read -- and sums, at a given theta and with mu = unlink(eta), w the prior weight:
//   T_SCORE  sum w [psi(theta + y) - psi(theta) + log theta + 1 - log(theta + mu) - (y + theta)/(mu + theta)]
//   T_INFO   sum w [-psi'(theta + y) + psi'(theta) - 1/theta + 2/(mu + theta) - (y + theta)/(mu + theta)^2]
//   T_LL     sum w dnbinom(y, theta, mu, log)      (LL instantiation only: the Newton steps need no lgamma)
//   T_MOM    sum w (y/mu - 1)^2,  T_SUMW  sum w   (theta.ml's starting value sum w / sum w (y/mu - 1)^2)
// The bracketed terms are grouped so that each group is formed without cancellation -- at a large theta every
// one of psi(theta + y) - psi(theta), log theta - log(theta + mu) and 1 - (y + theta)/(mu + theta) is O(1/theta)
// while the row's score is O(1/theta^2):
//   D = psi(theta + y) - psi(theta)   small integer counts: the exact sum_{k < y} 1/(theta + k); every other row:
//       digamma_diff_pos (polygamma.hpp: the series subtracted term by term, log1p(y/theta) + ..., all terms >= 0)
//   score row = D + log(theta/(mu + theta)) + (mu - y)/(mu + theta)      (the log as log1p(-mu/(mu + theta)))
//   T = psi'(theta) - psi'(theta + y)  small integer counts: sum_{k < y} 1/(theta + k)^2, else trigamma_diff_pos
//   info row  = T - mu/(theta (mu + theta)) + (mu - y)/(mu + theta)^2
// No group is a difference of two rounded function values; the three groups of a row do cancel against each
// other (that is the row's conditioning, tests/theta_reference.py's scale S).  The log-likelihood row is the
// textbook sum of six terms and cancels at a large theta (3e-9 relative at theta = 1e8).
// One partial of NS slots per workgroup (a contiguous row range, lanes then waves in a fixed order);
// reduce_stats_kernel sums the partials in a fixed order, Neumaier-compensated.  No atomics: run-to-run bitwise.
// Rows >= n are never read; a row of prior weight 0 contributes exactly 0 whatever its y and mu.  A row whose y is
// not a finite value >= 0 makes the sums NaN (SGLM_EINVAL on the host); no loop's trip count depends on the data
// beyond the bounds THETA_SUM_MAX and POLYGAMMA_DIFF_TRIPS.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rowmath.hpp"

namespace sglm {

namespace {

// integer counts below this take the exact finite sums (at most THETA_SUM_MAX - 1 reciprocals)
constexpr int THETA_SUM_MAX = 17;

template <bool LL>
__global__ void __launch_bounds__(256) theta_terms_kernel(ThetaArgs a) {
  __shared__ double red[4][THETA_NT];
  const double th = a.theta;
  // the launch's constants (every thread forms them: ~100 instructions against its rows' thousands)
  const double lg0 = LL ? lgamma(th) : 0.0, tlt = LL ? th * log(th) : 0.0;
  double s[THETA_NT];
#pragma unroll
  for (int k = 0; k < THETA_NT; ++k) s[k] = 0.0;
  const int64_t per = (a.n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = per * blockIdx.x, hi = (lo + per < a.n) ? lo + per : a.n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double pw = a.prior ? a.prior[i] : 1.0;
    const double y = a.y[i];
    const double eta = a.eta[i];
    if (pw == 0.0) continue;
    const double mu = unlink_fn_x(a.link, eta);
    const double mt = mu + th;
    double D = 0.0, T = 0.0;
    // A count must be >= 0 and finite: any other y (negative, a missing-value sentinel, NaN, Inf) makes the
    // row's terms NaN -- the sums then are NaN and the host returns SGLM_EINVAL, as the pass kernels' invalid
    // rows do.  Every loop of a row is bounded whatever the data: the finite sums by THETA_SUM_MAX - 1 trips,
    // the polygamma differences by POLYGAMMA_DIFF_TRIPS, a count that theta alone sets (polygamma.hpp).
    if (!(y >= 0.0) || !(y < INFINITY)) {
      D = T = NAN;
    } else if (y < (double)THETA_SUM_MAX && y == floor(y)) {
      const int ky = (int)y;
      for (int k = 0; k < ky; ++k) {
        const double r = 1.0 / (th + (double)k);
        D += r;
        T += r * r;
      }
    } else {
      polygamma_diff_pos(th, y, &D, &T);
    }
    const double q = mu / mt, e = (mu - y) / mt;
    // log(theta/(mu + theta)): log1p where theta dominates (q rounds, 1 - q would cancel), the plain log otherwise
    const double lq = q < 0.5 ? log1p(-q) : log(th / mt);
    s[T_SCORE] += pw * ((D + lq) + e);
    s[T_INFO] += pw * ((T - q / th) + e / mt);
    if constexpr (LL)
      s[T_LL] += pw * (((((lgamma(th + y) - lg0) - lgamma(y + 1.0)) + tlt) + y * log(mu + (y == 0.0 ? 1.0 : 0.0))) -
                       (th + y) * log(mt));
    const double u = y / mu - 1.0;
    s[T_MOM] += pw * (u * u);
    s[T_SUMW] += pw;
  }
#pragma unroll
  for (int k = 0; k < THETA_NT; ++k) {
    double v = s[k];
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    a.partials[(int64_t)blockIdx.x * NS + k] =
        k < THETA_NT ? ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k] : 0.0;
  }
}

}  // namespace

hipError_t launch_theta_terms(const ThetaArgs& a, int grid, bool loglik, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  if (grid < 1 || !a.y || !a.eta || !a.partials) return hipErrorInvalidValue;
  if (loglik) hipExtLaunchKernelGGL(theta_terms_kernel<true>, dim3(grid), dim3(256), 0, st, e0, e1, 0, a);
  else hipExtLaunchKernelGGL(theta_terms_kernel<false>, dim3(grid), dim3(256), 0, st, e0, e1, 0, a);
  return hipGetLastError();
}

}  // namespace sglm
