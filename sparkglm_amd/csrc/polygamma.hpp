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
//
// Stated accuracy (tests/test_theta_reference.py asserts it against mpmath on the host, x over (0, 1e12]):
//   digamma_pos   |error| <= 8 * 2^-52 * max(|psi(x)|, 1)    (psi has a zero at 1.4616...: the recurrence's ten
//                 reciprocals and the log are of size 2 to 3 there whatever psi's own size, so absolute)
//   trigamma_pos  <= 5 ulp
//
// The differences over a count y >= 0 (theta.hip's D and T) are NOT formed from those two values: at a large
// theta both would be differences of two numbers of size log theta (1/theta) with a result of size y/theta
// (y/theta^2).  digamma_diff_pos / trigamma_diff_pos subtract the asymptotic series term by term instead, with
// a = theta, b = theta + y, ra = 1/a, rb = 1/b, A = ra - rb = y ra rb, f = ra^2, g = rb^2, f - g = A (ra + rb):
//   psi(b) - psi(a)   = log1p(y/a) + A/2 + (P(f) - P(g)),                  psi(x)  = log x - 1/(2x) - P(1/x^2)
//   psi'(a) - psi'(b) = A (1 + (ra + rb)/2 + P2(g)) + ra (P2(f) - P2(g)),  psi'(x) = 1/x + 1/(2x^2) + P2(1/x^2)/x
// where P(f) - P(g) = (f - g) Q(f, g) exactly, Q the quotient of P(u) - P(f) by u - f from Horner's own partial
// sums (synthetic division): every term above is >= 0 and no difference of rounded values is formed anywhere.
// Both arguments must be in the series' range, so a theta < 16 is first moved up by the recurrences' own
// differences, 1/(theta + k) - 1/(theta + y + k) = y / ((theta + k)(theta + y + k)) >= 0 and its square
// counterpart -- m = ceil(16 - theta) <= 16 trips (POLYGAMMA_DIFF_TRIPS), a count that depends on theta
// alone, never on y.  The switch is at 16, not at 10, because the differences see the series' truncation
// magnified by its order: the first omitted terms leave 7 x^-16 (psi) and 120 x^-16 (psi') relative, which is
// 6 and 108 units of 2^-53 at x = 10 and 0.01 at x = 16.
//   digamma_diff_pos, trigamma_diff_pos   <= 6 ulp  (theta over [0.01, 1e12], y over [2^-20, 1e9]; y = 0: 0)
// (a term of the move is two reciprocals and two or three products, 2 to 2.5 ulp, the series' part log1p and its
// rounded argument, 2 ulp, or five products; the sums are of positive terms, half an ulp of a partial sum each,
// and on the host the largest error met is 3.3 ulp -- 6 is the statement the tests of theta.hip's rows build on)
// Anything but theta > 0 and 0 <= y < Inf returns NaN before the loop.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SGLM_HD __host__ __device__ __forceinline__
#else
#define SGLM_HD inline
#endif

namespace sglm {

constexpr int POLYGAMMA_MAX_TRIPS = 10;
constexpr int POLYGAMMA_DIFF_TRIPS = 16;

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

// D = psi(theta + y) - psi(theta) and T = psi'(theta) - psi'(theta + y) together (they share every quotient)
SGLM_HD void polygamma_diff_pos(double th, double y, double* D, double* T) {
  if (!(th > 0.0) || !(y >= 0.0) || !(y < INFINITY)) {
    *D = *T = NAN;
    return;
  }
  double d = 0.0, t = 0.0, a = th;
  for (int k = 0; k < POLYGAMMA_DIFF_TRIPS && a < 16.0; ++k) {
    const double ra = 1.0 / a, rb = 1.0 / (a + y);
    const double A = (y * ra) * rb;
    d += A;
    t += A * (ra + rb);
    a = th + (double)(k + 1);
  }
  const double b = a + y;
  const double ra = 1.0 / a, rb = 1.0 / b;
  const double u = y * ra, A = u * rb, sr = ra + rb;
  const double f = ra * ra, g = rb * rb, fg = A * sr;
  // P(u) = u (c1 - u (c2 - u (...))): Horner at f keeps its partial sums, Horner at g over them is Q(f, g)
  const double p7 = 1.0 / 12.0, p6 = 691.0 / 32760.0 - f * p7, p5 = 1.0 / 132.0 - f * p6, p4 = 1.0 / 240.0 - f * p5,
               p3 = 1.0 / 252.0 - f * p4, p2 = 1.0 / 120.0 - f * p3, p1 = 1.0 / 12.0 - f * p2;
  const double Q = p1 - g * (p2 - g * (p3 - g * (p4 - g * (p5 - g * (p6 - g * p7)))));
  const double s7 = 7.0 / 6.0, s6 = 691.0 / 2730.0 - f * s7, s5 = 5.0 / 66.0 - f * s6, s4 = 1.0 / 30.0 - f * s5,
               s3 = 1.0 / 42.0 - f * s4, s2 = 1.0 / 30.0 - f * s3, s1 = 1.0 / 6.0 - f * s2;
  const double Q2 = s1 - g * (s2 - g * (s3 - g * (s4 - g * (s5 - g * (s6 - g * s7)))));
  const double P2g =
      g * (1.0 / 6.0 -
           g * (1.0 / 30.0 -
                g * (1.0 / 42.0 - g * (1.0 / 30.0 - g * (5.0 / 66.0 - g * (691.0 / 2730.0 - g * (7.0 / 6.0)))))));
  *D = d + (log1p(u) + (0.5 * A + fg * Q));
  *T = t + (A * (1.0 + (0.5 * sr + P2g)) + (fg * Q2) * ra);
}
SGLM_HD double digamma_diff_pos(double th, double y) {
  double D, T;
  polygamma_diff_pos(th, y, &D, &T);
  return D;
}
SGLM_HD double trigamma_diff_pos(double th, double y) {
  double D, T;
  polygamma_diff_pos(th, y, &D, &T);
  return T;
}

}  // namespace sglm
