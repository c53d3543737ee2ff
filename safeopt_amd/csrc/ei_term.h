// The device functions every expected-improvement kernel shares (ei.hip: the row kernel of
// sgp_ei_eval, the grid kernel of sgp_grid_ei, the particle kernel of an 'ei' swarm): ln Phi, ln(phi + z Phi) and the alpha of one
// row -- LogEI (Ament, Daulton, Eriksson, Balandat, Bakshy 2023, "Unexpected improvements to
// expected improvement for Bayesian optimization").  ONE definition, so that alpha has the
// same bits wherever it is formed; the translation unit that includes it is compiled with
// -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

// Branch points of ei_log_h (tests/_ei_ref.py restates them)
#define SGP_EI_Z_DIRECT (-1.0)     // z >= this: the direct form
#define SGP_EI_Z_ASYMPT (-1.0e6)   // z <  this: the asymptotic form

// ln Phi(z), with t = |z| / sqrt 2, e = erfcx(t) (mes_term's forms):
//   z <  0:  ln Phi = ln(e / 2) - t^2
//   z >= 0:  ln Phi = log1p(-q),  q = e exp(-t^2) / 2 = Phi(-z)
// Finite for every z with a finite z^2 / 2; 0 exactly once q underflows, +inf included.
__device__ __forceinline__ double ei_log_ndtr(double z) {
  const double t = fabs(z) * 0.70710678118654752440;
  const double e = erfcx(t);
  if (z < 0.0) return log(0.5 * e) - t * t;
  return log1p(-(0.5 * e * exp(-(t * t))));
}

// ln h(z), h(z) = phi(z) + z Phi(z) = E max(z + eps, 0), eps ~ N(0, 1):
//   z >= -1:          ln(exp(-z^2 / 2) / sqrt(2 pi) + z erfc(-z / sqrt 2) / 2)
//   -1e6 <= z < -1:   ln(1 - sqrt(pi) t erfcx(t)) - z^2 / 2 - ln(2 pi) / 2,  t = -z / sqrt 2
//                     (h = phi (1 + z Phi / phi), Phi / phi = sqrt(pi / 2) erfcx(t))
//   z < -1e6:         -z^2 / 2 - ln(2 pi) / 2 - 2 ln|z|
// The middle form loses z^2 ulp to the cancellation in 1 - sqrt(pi) t erfcx(t) = 1 / z^2 -
// 3 / z^4 + ..., which is what the unit EPS (1 + z^2 / 2) of its tests allows (the value
// itself is -z^2 / 2 to leading order); below -1e6 the term 3 / z^4 the last form drops is
// under 3e-12 of 1 / z^2, far inside that rounding.  Increasing in z, +inf at z = +inf, finite
// for every z with a finite z^2 / 2.
__device__ __forceinline__ double ei_log_h(double z) {
  if (z >= SGP_EI_Z_DIRECT) {
    const double phi = exp(-0.5 * (z * z)) * 0.39894228040143267794;
    const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
    return log(phi + z * Phi);
  }
  const double tail = -0.5 * (z * z) - 0.91893853320467274178;
  if (z < SGP_EI_Z_ASYMPT) return tail - 2.0 * log(-z);
  const double t = -z * 0.70710678118654752440;
  return log(1.0 - 1.77245385090551602730 * t * erfcx(t)) + tail;
}

// (What a call fixes for all its rows, struct EiTerm, is declared in common.h: FitnessArgs
// carries one for an 'ei' swarm.)

// alpha of one row: mean / var point at the row's entry of GP 0, GP g `stride` doubles on
//   z = (mean_0 - tau - xi) / sigma_0,  sigma_g = sqrt(max(var_g, 1e-15))
//   EI: a = ln(max(var_0, 1e-15)) / 2 + ln h(z)      PI: a = ln Phi(z)
//   a += ln Phi((mean_g - fmin_g) / sigma_g) for every g with a finite fmin_g, in the order of g
__device__ __forceinline__ double ei_alpha(const double* mean, const double* var,
                                           int64_t stride, double tau, const EiTerm& p) {
  const double v0 = fmax(var[0], 1e-15);
  const double z = (mean[0] - tau - p.xi) / sqrt(v0);
  double a = p.kind == SGP_EI_EI ? 0.5 * log(v0) + ei_log_h(z) : ei_log_ndtr(z);
  for (int g = 0; g < p.G; ++g) {
    const double f = p.fmin[g];
    if (f > -INFINITY && f < INFINITY) {
      const double sg = sqrt(fmax(var[g * stride], 1e-15));
      a += ei_log_ndtr((mean[g * stride] - f) / sg);
    }
  }
  return a;
}
