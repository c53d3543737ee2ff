// The device functions every max-value entropy search kernel shares (mes.hip: the row kernel
// of sgp_mes_eval, the grid kernel of sgp_grid_mes, the particle kernel of a 'mes' swarm): one
// term, the alpha of one row from the staged maxima, and the staging of the maxima in LDS.
// ONE definition, so that alpha has the same bits wherever it is formed; the translation unit
// that includes it is compiled with -ffp-contract=off (build.py).
#pragma once
#include <hip/hip_runtime.h>

// term(g) = g phi(g) / (2 Phi(g)) - ln Phi(g), with t = |g| / sqrt 2, e = erfcx(t),
// x = exp(-t^2), q = e x / 2 = Phi(-|g|):
//   g <  0:  phi / Phi = sqrt(2 / pi) / e          ln Phi = ln(e / 2) - t^2
//   g >= 0:  phi / Phi = x / sqrt(2 pi) / (1 - q)  ln Phi = log1p(-q)
// For g >= 38.6 x underflows to 0 and the term is exactly 0; the product g x 0 is not formed
// (g = +inf, from a floor of +inf, would make it NaN).
__device__ __forceinline__ double mes_term(double g) {
  const double t = fabs(g) * 0.70710678118654752440;
  const double e = erfcx(t);
  const double x = exp(-(t * t));
  const double q = 0.5 * e * x;
  double r, lnp;
  if (g < 0.0) {
    r = 0.79788456080286535588 / e;
    lnp = log(0.5 * e) - t * t;
  } else {
    r = x / 2.50662827463100050242 / (1.0 - q);
    lnp = log1p(-q);
  }
  const double gr = x > 0.0 || g < 0.0 ? g * r : 0.0;
  return 0.5 * gr - lnp;
}

// alpha of one row; ys: the K floored maxima (LDS)
__device__ __forceinline__ double mes_alpha(double mu, double v, const double* ys, int K) {
  const double sigma = sqrt(fmax(v, 1e-15));
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc += mes_term((ys[k] - mu) / sigma);
  return acc / double(K);
}

__device__ __forceinline__ void stage_ystar(double* ys, const double* ystar, int K,
                                            const double* floor) {
  if (int(threadIdx.x) < K) ys[threadIdx.x] = fmax(ystar[threadIdx.x], floor[0]);
  __syncthreads();
}
