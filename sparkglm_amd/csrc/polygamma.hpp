// polygamma.hpp -- digamma and trigamma of x > 0 (the device libm has neither; theta.hip).  Plain C++ that also
// compiles for the host, so that tests/test_negbin_api.py checks the very functions against scipy on the CPU.
//
// The recurrences psi(x) = psi(x + 1) - 1/x, psi'(x) = psi'(x + 1) + 1/x^2 up to x >= 10, then the asymptotic
// (Bernoulli) series through the x^-14 / x^-15 terms -- the first omitted terms are 0.44 x^-16 and 7.1 x^-17,
// below 1e-16 relative from x = 10 (at the customary switch x >= 6 they are 1.6e-13 and 4e-13).
//
// Domain and trip count: the argument must be positive.  Anything else -- zero, a negative value (a count column
// with a negative or sentinel entry reaches theta + y < 0), NaN -- returns NaN before the recurrence, so the
// loop runs for 0 < x < 10 only: at most 10 trips, whatever the data (x + 1 > x holds on that whole range).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SGLM_HD __host__ __device__ __forceinline__
#else
#define SGLM_HD inline
#endif

namespace sglm {

constexpr int POLYGAMMA_MAX_TRIPS = 10;

SGLM_HD double digamma_pos(double x) {
  if (!(x > 0.0)) return NAN;
  double r = 0.0;
  for (int k = 0; k < POLYGAMMA_MAX_TRIPS && x < 10.0; ++k) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  const double t =
      f * (1.0 / 12.0 -
           f * (1.0 / 120.0 -
                f * (1.0 / 252.0 - f * (1.0 / 240.0 - f * (1.0 / 132.0 - f * (691.0 / 32760.0 - f * (1.0 / 12.0)))))));
  return r + ((log(x) - 0.5 / x) - t);
}
SGLM_HD double trigamma_pos(double x) {
  if (!(x > 0.0)) return NAN;
  double r = 0.0;
  for (int k = 0; k < POLYGAMMA_MAX_TRIPS && x < 10.0; ++k) {
    r += 1.0 / (x * x);
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  const double t =
      f * (1.0 / 6.0 -
           f * (1.0 / 30.0 -
                f * (1.0 / 42.0 - f * (1.0 / 30.0 - f * (5.0 / 66.0 - f * (691.0 / 2730.0 - f * (7.0 / 6.0)))))));
  return r + ((1.0 / x) * (1.0 + t) + 0.5 * f);
}

}  // namespace sglm
