// The device function every information-theoretic safe exploration kernel shares (ise.hip: the
// row kernel of sgp_ise_eval and the grid kernel of sgp_grid_ise): the approximate mutual
// information between a measurement at x and the safety indicator of z, for one GP.
// ONE definition, so that the term has the same bits wherever it is formed; the translation unit
// that includes it is compiled with -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>

// Bottero et al. 2022: with mu = mean(z) - fmin, vz = var(z), vx = var(x), c = cov(z, x),
// s = the noise of a measurement, c1 = 1 / (pi ln 2), t = c1 mu^2 / vz, r2 = c^2 / (vx vz),
//   I = ln2 [e^-t - sqrt(A / B) e^(-t (s + vx) / B)],  A = s + vx (1 - r2),
//                                                      B = s + vx + (2 c1 - 1) r2 vx.
// The stable form: with q = r2 vx and e = q / B,  A / B = 1 - 2 c1 e  and
// (s + vx) / B = 1 + (1 - 2 c1) e, so
//   I = -ln2 e^-t expm1(log1p(-2 c1 e) / 2 - t (1 - 2 c1) e):
// no difference of nearly equal numbers, >= 0, exactly 0 at c = 0, <= ln2 e^-t, finite for every
// finite input.  The variances are clipped at 1e-15 as everywhere in the library; r2 and
// w = 2 c1 e are clipped at 1 (s = 0 and r2 = 1 can round the quotient above it; w = 1 gives
// log1p = -inf, expm1 = -1 and I = ln2 e^-t).
constexpr double kIseC1 = 0.45922409426328514;     // 1 / (pi ln 2)
constexpr double kIseLn2 = 0.6931471805599453;

__device__ __forceinline__ double ise_term(double mu, double vz, double vx, double c, double s) {
  vz = fmax(vz, 1e-15);
  vx = fmax(vx, 1e-15);
  const double t = kIseC1 * (mu * mu) / vz;
  const double r2 = fmin((c * c) / (vx * vz), 1.0);
  const double q = r2 * vx;
  const double B = (s + vx) + (2.0 * kIseC1 - 1.0) * q;
  const double e = q / B;
  const double w = fmin(2.0 * kIseC1 * e, 1.0);
  return -kIseLn2 * exp(-t) * expm1(0.5 * log1p(-w) - t * ((1.0 - 2.0 * kIseC1) * e));
}
