// The fitness shaping of SafeOptSwarm._compute_particle_fitness
// (gp_opt.py:925-1013) and SafeOptSwarm._compute_penalty (gp_opt.py:874-899),
// shared by k_fitness_small (swarm.hip: the pass behind the posterior sweep of a
// fitness call, launch_sweep in sweep.hip) and the few-points kernels (swarm.hip).
#pragma once
#include "common.h"

// SafeOptSwarm._compute_penalty (gp_opt.py:874-899) for one value.
__device__ __forceinline__ double swarm_penalty(double slack) {
  double pen = fmin(slack, 0.0);
  if (slack < 0.0 && slack > -0.001) pen *= 2.0;
  if (slack <= -0.001 && slack > -0.1) pen *= 5.0;
  if (slack <= -0.1 && slack > -1.0) pen *= 10.0;
  if (slack < -1.0) pen = -300.0 * (pen * pen);   // -300 * pen ** 2: the square first
  return pen;
}

// One particle from the posterior of its G GPs (post(g, &mu, &var)): the value
// the swarm maximises and the particle's safety flag.  Same formulas, same order
// as the sweep's epilogue.
// kSwarmThompson (sgp_swarm_*_path, internal): the maximizers' safety rule and
// penalty with the uncertainty term replaced by the value of a sample path and
// interest = 1,
//   value = f(x) / scaling[0] + total_pen.
// The path term is not a function of the posterior: *value is total_pen here and
// k_swarm_path (paths.hip) completes it, in that operation order.
// kSwarmMes (sgp_swarm_*_mes, internal): the same branch -- *value is total_pen, and
// k_swarm_mes (mes.hip) adds alpha of GP 0's posterior: value = alpha + total_pen.
// kSwarmIse (sgp_swarm_*_ise, internal): the same branch again -- k_swarm_ise (swarm_ise.hip)
// adds alpha = max_t pair(p, t) over the staged targets: value = alpha + total_pen.
// kSwarmEi (sgp_swarm_*_ei, internal): the same branch once more -- k_swarm_ei (ei.hip) adds the
// log expected improvement of the G GPs' posterior: value = alpha + total_pen (or, in free
// mode, replaces value and flag: value = alpha, safe = 1).
// HALL (a hallucinated swarm, sgp_swarm_*_hall; maximizers and expanders): down(g) is what
// the pending picks of the batch take off the variance of GP g here, and the `values` term
// ALONE is formed from sd_h = sqrt(max(var - down, 1e-15)); lower, upper, both interests,
// the slack, the penalty and the safety flag stay those of the real posterior.  var_h(g, v)
// receives the hallucinated variance.
struct NoDown {
  __device__ __forceinline__ double operator()(int) const { return 0.0; }
};
struct NoVarH {
  __device__ __forceinline__ void operator()(int, double) const {}
};
template <bool HALL = false, typename Post, typename Down = NoDown, typename VarH = NoVarH>
__device__ __forceinline__ void shape_particle(const FitnessArgs& f, int G, Post post,
                                               double* value, bool* is_safe,
                                               Down down = Down(), VarH var_h = VarH()) {
  const int st = f.swarm_type;
  const int Geff = (st == SGP_SWARM_GREEDY) ? 1 : G;
  bool safe = true;
  double values = 0.0, interest = 1.0, total_pen = 0.0, lower = 0.0;
  for (int g = 0; g < Geff; ++g) {
    double mu, var;
    post(g, &mu, &var);
    const double sd = sqrt(var);
    double sd_w = sd;                    // the standard deviation of the width term
    if (HALL) {
      const double vh = fmax(var - down(g), 1e-15);
      var_h(g, vh);
      sd_w = sqrt(vh);
    }
    lower = mu - f.beta * sd;
    if (g == 0) {
      values = sd_w / f.scaling[0];
      if (st == SGP_SWARM_EXPANDERS) interest = double(G);
      if (st == SGP_SWARM_MAXIMIZERS) {
        const double upper = mu + f.beta * sd;
        const double z = 10.0 * (upper - f.best_lower_bound) / f.scaling[0];
        interest = 1.0 / (1.0 + exp(-z));  // scipy.special.expit
      }
    } else {
      values = fmax(values, sd_w / f.scaling[g]);
    }
    if (f.fmin[g] != -INFINITY) {
      double slack = lower - f.fmin[g];
      safe = safe && (slack >= 0.0);
      if (st != SGP_SWARM_SAFE_SET) {
        slack = slack / f.scaling[g];
        total_pen += swarm_penalty(slack);
        if (st == SGP_SWARM_EXPANDERS) {
          const double z = slack / 0.2;   // scipy.stats.norm.pdf(slack, scale=0.2)
          interest *= exp(-0.5 * z * z) / 2.5066282746310002 / 0.2;
        }
      }
    }
  }
  if (st == SGP_SWARM_GREEDY) {
    *value = lower;
    *is_safe = true;
  } else if (st == SGP_SWARM_SAFE_SET) {
    *value = lower;
    *is_safe = safe;
  } else if (st == kSwarmThompson || st == kSwarmMes || st == kSwarmIse || st == kSwarmEi) {
    *value = total_pen;
    *is_safe = safe;
  } else {
    *value = (values + total_pen) * interest;
    *is_safe = safe;
  }
}
