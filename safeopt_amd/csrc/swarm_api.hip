// The swarm entry points of the C ABI (include/safeopt_hip.h): host-side launch sequences
// around the kernels of swarm.hip, paths.hip, swarm_batch.hip, mes.hip, swarm_ise.hip, ei.hip and
// the posterior sweeps.  Eighteen exported fitness / run functions (plain, hallucinated, Thompson,
// 'mes', 'ise' and 'ei': one fitness, one run and one sharded run each) fill SwarmSpec / SwarmState / PsoSchedule
// (common.h) and share ONE fitness routine and ONE run routine.
#include <string.h>

#include <cmath>

#include "common.h"
#include "small_path.h"

// Fitness of P <= kSmallPoints particles (row-major, device) through the
// small-point posterior path: mean / var per GP, then the shaping kernel.
static int fitness_small(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                         int G, const double* pts_rowmajor, int64_t P,
                         const FitnessArgs& fa) {
  const int Geff = (fa.swarm_type == SGP_SWARM_GREEDY) ? 1 : G;
  double* mv;
  SGP_TRY(sgp_scratch(ctx, kSlotPartials, size_t(2) * SGP_MAX_GPS * kSmallPoints * sizeof(double),
                      &mv));
  SmallBufs sb;
  SGP_TRY(small_reserve(ctx, gps_host, Geff, int(P), &sb));
  double* mean = mv;
  double* var = mv + size_t(SGP_MAX_GPS) * kSmallPoints;
  SGP_TRY(posterior_small_all(ctx, gps_dev, gps_host, Geff, pts_rowmajor, int(P), sb,
                              mean, var));
  return launch_fitness_small(ctx, G, P, mean, var, fa);
}

static bool small_path_pays_all(sgp_gp* const* gps, int G, int64_t P) {
  for (int g = 0; g < G; ++g)
    if (!small_path_pays(gps[g], P)) return false;
  return true;
}

// The clones of a hallucinated swarm (sgp_swarm_fitness_hall / sgp_swarm_run_hall) against
// the GPs they were cloned from: maximizers or expanders, every clone in the call's context
// with the source's input dimension and kernel and gps[g].n + b observations for ONE b in
// 1 .. SGP_MAX_BATCH.  host: their descriptors, `share` as collect_gps sets it.
static int hall_clones(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                       int swarm_type, GpDev* host, int* b_out) {
  SGP_CHECK(ctx, swarm_type == SGP_SWARM_MAXIMIZERS || swarm_type == SGP_SWARM_EXPANDERS,
            "a hallucinated swarm is a maximizers or an expanders swarm, not type %d",
            swarm_type);
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS && gps[0], "no GP");
  SGP_CHECK(ctx, clones != nullptr, "no clones");
  for (int g = 0; g < G; ++g) {
    SGP_CHECK(ctx, gps[g] && clones[g], "GP %d or its clone is missing", g);
    SGP_CHECK(ctx, gps[g]->ctx == ctx && clones[g]->ctx == ctx,
              "GP %d or its clone lives in another context than the call (device %d)", g,
              ctx->device);
    SGP_CHECK(ctx, clones[g]->kern.d == gps[g]->kern.d &&
                       memcmp(&clones[g]->kern, &gps[g]->kern, sizeof(KernDesc)) == 0,
              "clone %d has another input dimension or kernel than its GP", g);
  }
  const int64_t b = clones[0]->n - gps[0]->n;
  SGP_CHECK(ctx, b >= 1 && b <= SGP_MAX_BATCH,
            "clone 0 holds %lld observations, its GP %lld: 1 .. %d pending picks",
            (long long)clones[0]->n, (long long)gps[0]->n, SGP_MAX_BATCH);
  for (int g = 1; g < G; ++g)
    SGP_CHECK(ctx, clones[g]->n == gps[g]->n + b,
              "clone %d holds %lld observations, its GP %lld: not the %lld pending picks of "
              "clone 0", g, (long long)clones[g]->n, (long long)gps[g]->n, (long long)b);
  SGP_TRY(collect_gps(ctx, clones, G, gps[0]->kern.d, host));
  *b_out = int(b);
  return 0;
}

// type, beta, best lower bound, and fmin / scaling padded to SGP_MAX_GPS
static FitnessArgs make_fitness_args(const SwarmSpec& s) {
  FitnessArgs fa{};
  fa.swarm_type = s.swarm_type;
  fa.beta = s.beta;
  fa.best_lower_bound = s.best_lower_bound;
  for (int i = 0; i < SGP_MAX_GPS; ++i) {
    fa.fmin[i] = (i < s.G) ? s.fmin[i] : -INFINITY;
    fa.scaling[i] = (i < s.G) ? s.scaling[i] : 1.0;
  }
  if (s.mes) fa.mes = *s.mes;
  if (s.ei) fa.ei = *s.ei;
  fa.ise = nullptr;            // (the routine points it at what it staged)
  return fa;
}

// a path comes with kSwarmThompson, maxima with kSwarmMes, targets with kSwarmIse, an incumbent
// with kSwarmEi, the public types otherwise
static bool swarm_type_ok(const SwarmSpec& s) {
  if (s.ei)
    return s.swarm_type == kSwarmEi && s.ei->on && !s.path && !s.clones && !s.mes && !s.ise;
  if (s.ise) return s.swarm_type == kSwarmIse && !s.path && !s.clones && !s.mes;
  if (s.path) return s.swarm_type == kSwarmThompson && !s.mes;
  if (s.mes) return s.swarm_type == kSwarmMes;
  return s.swarm_type >= SGP_SWARM_GREEDY && s.swarm_type <= SGP_SWARM_SAFE_SET;
}

// The checks a Thompson entry point makes in front of its early return; behind that
// return it stages the path (swarm_path_stage: ONCE per call; neither routine below asks
// for the two slots the path lives in)
static int path_checks(sgp_ctx* ctx, sgp_gp* const* gps, int G, int m) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G >= 1 && gps[0], "no GP");
  SGP_CHECK(ctx, gps[0]->ctx == ctx, "GP 0 lives in another context (device %d) than the "
            "call (device %d)", gps[0]->ctx ? gps[0]->ctx->device : -1, ctx->device);
  return swarm_path_ready(gps[0], m);
}

// The order of the argument checks, per entry point, that the two routines keep ("type":
// "Invalid swarm type"; "clones": the checks of hall_clones, its collect_gps of the clones
// last; "path": GP 0's context, then swarm_path_ready; "GPs": collect_gps of the GPs):
//   sgp_swarm_fitness       type, "no GP", return 0 if P <= 0, GPs
//   sgp_swarm_fitness_hall  "no clones", type, "no GP", clones, return 0 if P <= 0, GPs
//   sgp_swarm_fitness_path  "no GP", path, return 0 if P <= 0, GPs
//   sgp_swarm_run[_shard]   type, "no GP", "bad swarm size", "bad block", "needs a
//                           communicator", GPs
//   sgp_swarm_run_hall[_shard]  "no clones"; P <= 0 and P_total <= 0: clones, return; else
//                           type, "no GP", "bad swarm size", "bad block", communicator,
//                           clones, GPs (an empty block of a sharded swarm: "bad swarm size")
//   sgp_swarm_run_path[_shard]  "no GP", path, return 0 if P <= 0 and P_total <= 0, then as
//                           sgp_swarm_run_shard (an empty block of a sharded swarm is the
//                           "bad swarm size" error, not a silent return: the other ranks
//                           would wait in the all-gather)
//   sgp_swarm_fitness_mes   "no GP", "maxima" (mes_checks: 1 <= K <= SGP_MAX_MES, every ystar[k]
//                           finite), "the floor is NaN", return 0 if P <= 0, GPs
//   sgp_swarm_run_mes[_shard]  "no GP", "maxima", "the floor is NaN", return 0 if P <= 0 and
//                           P_total <= 0, then as sgp_swarm_run_shard (an empty block of a
//                           sharded swarm: "bad swarm size", as for a path run)
//   sgp_swarm_fitness_ise   "no GP", "targets" (swarm_ise_checks: 1 <= T <= SGP_MAX_ISE; targets,
//                           zmean and zvar present and finite, every zvar >= 0), "no GP is
//                           active", return 0 if P <= 0, "test outputs" (pairs / cov above
//                           G P T = 2^24), GPs; the targets and operands are staged behind GPs
//   sgp_swarm_run_ise[_shard]  "no GP", "targets", "no GP is active", return 0 if P <= 0 and
//                           P_total <= 0, then as sgp_swarm_run_shard (an empty block of a
//                           sharded swarm: "bad swarm size", as for a path run); staged behind GPs
//   sgp_swarm_fitness_ei    "no GP", "kind" (SGP_EI_EI / SGP_EI_PI), "tau" (finite), "xi" (finite,
//                           >= 0), "weigh" then "free" (0 or 1), with weigh "fmin" (no fmin[g] NaN
//                           or +inf), return 0 if P <= 0, GPs (which bounds G by SGP_MAX_GPS)
//   sgp_swarm_run_ei[_shard]  "no GP", "kind", "tau", "xi", "weigh", "free", "fmin", return 0 if
//                           P <= 0 and P_total <= 0, then as sgp_swarm_run_shard (an empty block
//                           of a sharded swarm: "bad swarm size", as for a path run)
// A Thompson, a 'mes', an 'ise' and an 'ei' call pass "type" and the second "no GP" by
// construction.

// All five fitness entry points: import the points, the real posterior and the shaping
// pass (few-points path or sweep), with clones the downdate (launch_swarm_down) in front of
// the shaping, with a path the path term (launch_swarm_path) behind it, with maxima alpha
// (launch_swarm_mes, inside launch_fitness_small where mean and var are at hand), with targets
// alpha of the 'ise' rule (launch_swarm_ise, likewise; the targets and operands are staged
// here, ONCE, behind the last check), with an incumbent alpha of the 'ei' rule (launch_swarm_ei,
// likewise; its constants travel by value, nothing is staged).
static int swarm_fitness(sgp_ctx* ctx, const SwarmSpec& s, const double* particles, int64_t P,
                         double* values, uint8_t* safe, double* var_h) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, swarm_type_ok(s), "Invalid swarm type %d", s.swarm_type);
  SGP_CHECK(ctx, s.G >= 1 && s.gps[0], "no GP");
  const int G = s.G;
  GpDev host[SGP_MAX_GPS], chost[SGP_MAX_GPS];
  int b = 0;
  if (s.clones) SGP_TRY(hall_clones(ctx, s.gps, s.clones, G, s.swarm_type, chost, &b));
  if (P <= 0) return 0;
  const int d = s.gps[0]->kern.d;
  SGP_TRY(collect_gps(ctx, s.gps, G, d, host));
  const size_t nv = size_t(P) * 8;
  const SwarmFitLayout l = swarm_fit_layout(P, d, G, s.clones != nullptr);   // (common.h)
  double* stage;
  char* work;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, nv * d, &stage));
  SGP_TRY(sgp_scratch(ctx, kSlotWork, l.bytes, &work));
  const SwarmFitBufs fb = swarm_fit_bufs(work, l);
  SGP_TRY(sgp_h2d(ctx, stage, particles, nv * d));
  SGP_TRY(launch_import_points(ctx, stage, P, d, d, 1, fb.pts));
  SGP_TRY(sgp_h2d(ctx, fb.gpdev, host, sizeof(GpDev) * G));
  FitnessArgs fa = make_fitness_args(s);
  fa.values = fb.values;
  fa.safe = fb.safe;
  const SweepPoints sp{fb.pts, P, 1, P};
  SwarmIse ise{};
  if (s.ise) {
    SGP_TRY(swarm_ise_stage(ctx, s.gps, host, G, d, s.fmin, *s.ise, P, &ise));
    ise.gps_dev = fb.gpdev;
    ise.base = sp.base;
    ise.stride_row = sp.stride_row;
    ise.stride_col = sp.stride_col;
    fa.ise = &ise;
  }
  if (s.clones) {
    SGP_TRY(sgp_h2d(ctx, fb.clones, chost, sizeof(GpDev) * G));
    SGP_TRY(launch_swarm_down(ctx, fb.clones, G, d, b, sp, fb.down));
    fa.down = fb.down;
    fa.var_h = var_h ? fb.var_h : nullptr;
  }
  if (small_path_pays_all(s.gps, G, P)) {
    SGP_TRY(fitness_small(ctx, fb.gpdev, host, G, stage, P, fa));
  } else {
    SGP_TRY(launch_sweep_fitness(ctx, fb.gpdev, host, G, d, sp, fa));
  }
  // (kSwarmThompson in fitness.h leaves the penalty in the values: the path term on top)
  if (s.path)
    SGP_TRY(launch_swarm_path(ctx, fb.gpdev, d, *s.path, sp, fa.scaling[0], fb.values));
  SGP_TRY(sgp_d2h(ctx, values, fb.values, nv));
  SGP_TRY(sgp_d2h(ctx, safe, fb.safe, size_t(P)));
  if (s.clones && var_h) SGP_TRY(sgp_d2h(ctx, var_h, fb.var_h, size_t(G) * nv));
  if (s.ise) SGP_TRY(swarm_ise_read(ctx, *s.ise, ise, G, P));
  return 0;
}

// SwarmOptimization.init_swarm / run_swarm (swarm.py:61-146) with the state in
// HBM and the fitness fused in: one call = the whole run, one host round trip.
// The particles [p0, p0 + P) of a swarm of Pt; P < Pt: a rank's block of a sharded
// swarm -- the global best goes through the record all-gather.
// s.path: a Thompson swarm, s.clones: a hallucinated swarm (the downdate in front of every
// shaping pass), s.mes: a 'mes' swarm (alpha behind every shaping pass, launched by
// launch_fitness_small), s.ise: an 'ise' swarm (likewise, the targets and operands staged once
// behind the checks), s.ei: an 'ei' swarm (likewise, nothing staged); all five always take the
// general launches below.
static int swarm_run(sgp_ctx* ctx, const SwarmSpec& s, const SwarmState& st,
                     const PsoSchedule& sch) {
  const int G = s.G, init = sch.init, iters = sch.iters;
  const int64_t P = st.P, p0 = st.p0, Pt = st.Pt;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, swarm_type_ok(s), "Invalid swarm type %d", s.swarm_type);
  SGP_CHECK(ctx, G >= 1 && s.gps[0], "no GP");
  SGP_CHECK(ctx, P >= 1 && iters >= 0, "bad swarm size %lld / iterations %d",
            (long long)P, iters);
  SGP_CHECK(ctx, p0 >= 0 && p0 + P <= Pt, "bad block [%lld, %lld) of a swarm of %lld",
            (long long)p0, (long long)(p0 + P), (long long)Pt);
  const bool shard = P < Pt;
  bool comm;
  SGP_TRY(comm_or_single(ctx, &comm));   // (several ranks always come with a communicator)
  SGP_CHECK(ctx, comm || !shard,
            "a block of %lld of a swarm of %lld particles needs a communicator in the "
            "context (sgp_comm_init / sgp_comm_init_host)", (long long)P, (long long)Pt);
  const int world = comm ? ctx->world : 1;
  const int d = s.gps[0]->kern.d;
  GpDev host[SGP_MAX_GPS], chost[SGP_MAX_GPS];
  int hall_b = 0;
  if (s.clones) SGP_TRY(hall_clones(ctx, s.gps, s.clones, G, s.swarm_type, chost, &hall_b));
  SGP_TRY(collect_gps(ctx, s.gps, G, d, host));
  const size_t nd = size_t(P) * d * 8, nv = size_t(P) * 8;
  const size_t nrand = sch.rand ? (size_t(init ? 1 : 0) + 2 * size_t(iters)) * nd : 0;
  const SwarmRunLayout l =
      swarm_run_layout(P, d, G, shard ? world : 0, s.clones != nullptr);   // (common.h)
  char* buf;
  double* drand = nullptr;
  SGP_TRY(sgp_scratch(ctx, kSlotWork, l.bytes, &buf));
  if (sch.rand) SGP_TRY(sgp_scratch(ctx, kSlotStage, nrand, &drand));
  const SwarmRunBufs rb = swarm_run_bufs(buf, l);
  const double* dbounds = st.bounds ? rb.bounds : nullptr;
  SGP_TRY(sgp_h2d(ctx, rb.pos, st.positions, nd));
  if (!init) {
    SGP_TRY(sgp_h2d(ctx, rb.vel, st.velocities, nd));
    SGP_TRY(sgp_h2d(ctx, rb.best, st.best_positions, nd));
    SGP_TRY(sgp_h2d(ctx, rb.best_values, st.best_values, nv));
    SGP_TRY(sgp_h2d(ctx, rb.gbest, st.global_best, size_t(d) * 8));
  }
  SGP_TRY(sgp_h2d(ctx, rb.vscale, st.velocity_scale, size_t(d) * 8));
  if (st.bounds) SGP_TRY(sgp_h2d(ctx, rb.bounds, st.bounds, size_t(d) * 16));
  if (sch.rand) SGP_TRY(sgp_h2d(ctx, drand, sch.rand, nrand));
  SGP_TRY(sgp_h2d(ctx, rb.gpdev, host, sizeof(GpDev) * G));
  if (s.clones) SGP_TRY(sgp_h2d(ctx, rb.clones, chost, sizeof(GpDev) * G));
  FitnessArgs fa = make_fitness_args(s);
  fa.values = rb.values;
  fa.safe = rb.safe;
  if (s.clones) fa.down = rb.down;
  const SweepPoints sp{rb.pos, P, d, 1};          // row-major (P, d) in place
  SwarmIse ise{};
  if (s.ise) {
    SGP_TRY(swarm_ise_stage(ctx, s.gps, host, G, d, s.fmin, *s.ise, P, &ise));
    ise.gps_dev = rb.gpdev;
    ise.base = sp.base;
    ise.stride_row = sp.stride_row;
    ise.stride_col = sp.stride_col;
    fa.ise = &ise;
  }
  // (the paths and the posterior kernel follow the whole swarm: same bits on every rank)
  const bool few = Pt <= kSmallSwarm && small_path_pays_all(s.gps, G, Pt);
  // a small swarm against GPs with few observations (SafeOptSwarm's defaults on the
  // reference's own examples: 20 particles, n <= 20): the posterior is one sweep launch
  // (sweep_tiny.hip up to 48 observations), everything else of the iteration the same ONE
  // workgroup as on the few-points path -- two launches per iteration instead of five
  const bool few_swept = Pt <= kSmallSwarm && !few;
  const double* r = drand;
  double inertia = sch.inertia0;
  if ((few || few_swept) && !shard && !s.path && !s.clones && !s.mes && !s.ise && !s.ei) {
    // small swarm: three launches per iteration -- k(X, particles), the block
    // products on the matrix cores, and ONE workgroup for everything else
    // (fitness, bests, and the move that opens the next iteration)
    const int Geff = (s.swarm_type == SGP_SWARM_GREEDY) ? 1 : G;
    SmallBufs sb{};
    ConfOut post{};
    if (few) {
      SGP_TRY(small_reserve(ctx, host, Geff, int(P), &sb));
    } else {
      const size_t np = size_t(Geff) * size_t(P);
      SGP_TRY(sgp_reserve(ctx, &ctx->pair_post, 2 * np * sizeof(double)));
      post.mean = static_cast<double*>(ctx->pair_post.p);
      post.var = post.mean + np;
      for (int i = 0; i < SGP_MAX_GPS; ++i) post.fmin[i] = -INFINITY;
    }
    PsoSmallArgs ps{};
    ps.pos = rb.pos;
    ps.vel = rb.vel;
    ps.best = rb.best;
    ps.best_values = rb.best_values;
    ps.gbest = rb.gbest;
    ps.vscale = rb.vscale;
    ps.bounds = dbounds;
    ps.seed = sch.seed;
    ps.P = int(P);
    ps.d = d;
    auto step = [&](int is_init, int it_next) -> int {   // it_next < 0: no move
      if (few)
        SGP_TRY(posterior_small_all(ctx, rb.gpdev, host, Geff, rb.pos, int(P), sb, nullptr,
                                    nullptr));
      else
        SGP_TRY(launch_sweep_conf(ctx, rb.gpdev, host, Geff, d, sp, post));
      ps.init = is_init;
      ps.move = it_next >= 0;
      ps.rand = r;
      ps.draw = uint32_t(it_next + 1);
      ps.inertia = inertia;
      SGP_TRY(launch_pso_small_step(ctx, rb.gpdev, G, sb, fa, ps, few ? nullptr : post.mean,
                                    few ? nullptr : post.var));
      if (ps.move) {
        if (r) r += 2 * size_t(P) * d;
        inertia += sch.step_size;
      }
      return 0;
    };
    if (init) {
      SGP_TRY(launch_pso_init_vel(ctx, P, d, rb.vel, rb.vscale, r, sch.seed));
      if (r) r += size_t(P) * d;
      SGP_TRY(step(1, iters > 0 ? 0 : -1));
    } else if (iters > 0) {
      SGP_TRY(launch_pso_move(ctx, P, d, rb.pos, rb.vel, rb.best, rb.gbest, rb.vscale, dbounds,
                              inertia, r, sch.seed, 1u));
      if (r) r += 2 * size_t(P) * d;
      inertia += sch.step_size;
    }
    for (int it = 0; it < iters; ++it)
      SGP_TRY(step(0, it + 1 < iters ? it + 1 : -1));
  } else {
    // (up to kSmallPoints particles still take the few-points posterior; a block of a
    // small swarm takes these launches, the arithmetic of k_pso_small_step)
    const bool few_points = small_path_pays_all(s.gps, G, Pt);
    auto fitness = [&]() -> int {
      // a hallucinated swarm: what the pending picks take off the variances, for the shaping
      if (s.clones) SGP_TRY(launch_swarm_down(ctx, rb.clones, G, d, hall_b, sp, rb.down));
      SGP_TRY(few_points ? fitness_small(ctx, rb.gpdev, host, G, rb.pos, P, fa)
                         : launch_sweep_fitness(ctx, rb.gpdev, host, G, d, sp, fa, Pt));
      // a Thompson swarm: the path term on top of the penalty the shaping left
      return s.path ? launch_swarm_path(ctx, rb.gpdev, d, *s.path, sp, fa.scaling[0], rb.values)
                    : 0;
    };
    // personal bests, then the global best: of the block, or merged over the ranks
    auto bests = [&](int is_init) -> int {
      if (!shard)
        return launch_pso_best(ctx, P, d, rb.values, rb.safe, rb.pos, rb.best, rb.best_values,
                               rb.gbest, is_init);
      SGP_TRY(launch_pso_best(ctx, P, d, rb.values, rb.safe, rb.pos, rb.best, rb.best_values,
                              rb.gbest, is_init, rb.rec, p0));
      SGP_TRY(coll_allgather(ctx, rb.rec, rb.recs, swarm_rec_bytes(d)));
      return launch_pso_gbest_merge(ctx, rb.recs, world, d, rb.gbest);
    };
    const int64_t e0 = p0 * d, e2 = Pt * d + p0 * d;
    if (init) {
      SGP_TRY(launch_pso_init_vel(ctx, P, d, rb.vel, rb.vscale, r, sch.seed, e0));
      if (r) r += size_t(P) * d;
      SGP_TRY(fitness());
      SGP_TRY(bests(1));
    }
    for (int it = 0; it < iters; ++it) {
      SGP_TRY(launch_pso_move(ctx, P, d, rb.pos, rb.vel, rb.best, rb.gbest, rb.vscale, dbounds,
                              inertia, r, sch.seed, uint32_t(it + 1), e0, e2));
      if (r) r += 2 * size_t(P) * d;
      inertia += sch.step_size;
      SGP_TRY(fitness());
      SGP_TRY(bests(0));
    }
  }
  SGP_TRY(sgp_d2h(ctx, st.positions, rb.pos, nd));
  SGP_TRY(sgp_d2h(ctx, st.velocities, rb.vel, nd));
  SGP_TRY(sgp_d2h(ctx, st.best_positions, rb.best, nd));
  SGP_TRY(sgp_d2h(ctx, st.best_values, rb.best_values, nv));
  return sgp_d2h(ctx, st.global_best, rb.gbest, size_t(d) * 8);
}

// A Thompson run: check, stage the path, run
static int swarm_run_path(sgp_ctx* ctx, SwarmSpec s, const SwarmState& st,
                          const PsoSchedule& sch, const double* const pin[4], int m) {
  SGP_TRY(path_checks(ctx, s.gps, s.G, m));
  if (st.P <= 0 && st.Pt <= 0) return 0;
  SwarmPath path;
  SGP_TRY(swarm_path_stage(s.gps[0], pin[0], pin[1], m, pin[2], pin[3], &path));
  s.path = &path;
  return swarm_run(ctx, s, st, sch);
}

// The checks a 'mes' entry point makes in front of its early return; behind that return it
// stages the maxima (swarm_mes_stage: ONCE per call, in kSlotMesIn, which neither routine
// above asks for)
static int swarm_mes_checks(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* ystar, int K,
                            double floor) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G >= 1 && gps[0], "no GP");
  SGP_TRY(mes_checks(ctx, ystar, K));
  SGP_CHECK(ctx, !std::isnan(floor), "the floor is NaN");
  return 0;
}

// post: the block also holds [2][P] for the posterior of GP 0 (a fitness call)
static int swarm_mes_stage(sgp_ctx* ctx, const double* ystar, int K, double floor, int64_t P,
                           bool post, SwarmMes* out) {
  const SwarmMesLayout l = swarm_mes_layout(P, post);   // (common.h)
  char* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotMesIn, l.bytes, &buf));
  SGP_TRY(sgp_h2d(ctx, buf + l.ystar, ystar, size_t(K) * 8));
  out->ystar = reinterpret_cast<const double*>(buf + l.ystar);
  out->K = K;
  out->floor = floor;
  out->post = post ? reinterpret_cast<double*>(buf + l.post) : nullptr;
  return 0;
}

// The checks an 'ei' entry point makes in front of its early return, and the call's constants
// as the kernel takes them (by value: nothing is staged on the device).  The weights walk the
// G GPs of the call; collect_gps, behind the early return, bounds G by SGP_MAX_GPS.
static int swarm_ei_checks(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* fmin, int kind,
                           double tau, double xi, int weigh, int free_mode, SwarmEi* out) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G >= 1 && gps[0], "no GP");
  SGP_CHECK(ctx, kind == SGP_EI_EI || kind == SGP_EI_PI, "kind = %d is not SGP_EI_EI / SGP_EI_PI",
            kind);
  SGP_CHECK(ctx, std::isfinite(tau), "the incumbent tau = %g is not finite", tau);
  SGP_CHECK(ctx, std::isfinite(xi) && xi >= 0.0, "xi = %g is negative or not finite", xi);
  SGP_CHECK(ctx, weigh == 0 || weigh == 1, "weigh = %d is not 0 or 1", weigh);
  SGP_CHECK(ctx, free_mode == 0 || free_mode == 1, "free = %d is not 0 or 1", free_mode);
  SwarmEi e{};
  e.term.kind = kind;
  e.term.G = G;
  e.term.xi = xi;
  for (int g = 0; g < SGP_MAX_GPS; ++g) {
    e.term.fmin[g] = weigh && g < G ? fmin[g] : -INFINITY;
    SGP_CHECK(ctx, e.term.fmin[g] < INFINITY, "fmin[%d] is NaN or +inf", g);   // (NaN < inf is false)
  }
  e.tau = tau;
  e.on = 1;
  e.free = free_mode;
  *out = e;
  return 0;
}

extern "C" {

int sgp_swarm_fitness(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                      const double* particles, int64_t P, double beta,
                      const double* fmin, const double* scaling,
                      double best_lower_bound, double* values, uint8_t* safe) {
  const SwarmSpec s{gps, G, swarm_type, beta, fmin, scaling, best_lower_bound, nullptr, nullptr};
  return swarm_fitness(ctx, s, particles, P, values, safe, nullptr);
}

int sgp_swarm_fitness_hall(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                           int swarm_type, const double* particles, int64_t P, double beta,
                           const double* fmin, const double* scaling, double best_lower_bound,
                           double* values, uint8_t* safe, double* var_h) {
  SGP_CHECK(ctx, clones != nullptr, "no clones");
  const SwarmSpec s{gps, G, swarm_type, beta, fmin, scaling, best_lower_bound, nullptr, clones};
  return swarm_fitness(ctx, s, particles, P, values, safe, var_h);
}

int sgp_swarm_fitness_path(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                           int64_t P, double beta, const double* fmin, const double* scaling,
                           const double* Omega, const double* phase, int m, const double* w,
                           const double* v, double* values, uint8_t* safe) {
  SGP_TRY(path_checks(ctx, gps, G, m));
  if (P <= 0) return 0;
  SwarmPath path;
  SGP_TRY(swarm_path_stage(gps[0], Omega, phase, m, w, v, &path));
  const SwarmSpec s{gps, G, kSwarmThompson, beta, fmin, scaling, 0.0, &path, nullptr};
  return swarm_fitness(ctx, s, particles, P, values, safe, nullptr);
}

int sgp_swarm_run(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                  double beta, const double* fmin, const double* scaling,
                  double best_lower_bound, int64_t P, double* positions,
                  double* velocities, double* best_positions, double* best_values,
                  double* global_best, const double* velocity_scale,
                  const double* bounds, int init, int iters, double inertia0,
                  double step_size, const double* rand, uint64_t seed) {
  return sgp_swarm_run_shard(ctx, gps, G, swarm_type, beta, fmin, scaling, best_lower_bound, P,
                             positions, velocities, best_positions, best_values, global_best,
                             velocity_scale, bounds, init, iters, inertia0, step_size, rand,
                             seed, 0, P);
}

int sgp_swarm_run_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                        double beta, const double* fmin, const double* scaling,
                        double best_lower_bound, int64_t P, double* positions,
                        double* velocities, double* best_positions, double* best_values,
                        double* global_best, const double* velocity_scale,
                        const double* bounds, int init, int iters, double inertia0,
                        double step_size, const double* rand, uint64_t seed, int64_t p0,
                        int64_t P_total) {
  const SwarmSpec s{gps, G, swarm_type, beta, fmin, scaling, best_lower_bound, nullptr, nullptr};
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  return swarm_run(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed});
}

int sgp_swarm_run_hall(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                       int swarm_type, double beta, const double* fmin, const double* scaling,
                       double best_lower_bound, int64_t P, double* positions,
                       double* velocities, double* best_positions, double* best_values,
                       double* global_best, const double* velocity_scale,
                       const double* bounds, int init, int iters, double inertia0,
                       double step_size, const double* rand, uint64_t seed) {
  return sgp_swarm_run_hall_shard(ctx, gps, clones, G, swarm_type, beta, fmin, scaling,
                                  best_lower_bound, P, positions, velocities, best_positions,
                                  best_values, global_best, velocity_scale, bounds, init, iters,
                                  inertia0, step_size, rand, seed, 0, P);
}

int sgp_swarm_run_hall_shard(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                             int swarm_type, double beta, const double* fmin,
                             const double* scaling, double best_lower_bound, int64_t P,
                             double* positions, double* velocities, double* best_positions,
                             double* best_values, double* global_best,
                             const double* velocity_scale, const double* bounds, int init,
                             int iters, double inertia0, double step_size, const double* rand,
                             uint64_t seed, int64_t p0, int64_t P_total) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, clones != nullptr, "no clones");
  if (P <= 0 && P_total <= 0) {
    GpDev chost[SGP_MAX_GPS];
    int b;
    return hall_clones(ctx, gps, clones, G, swarm_type, chost, &b);
  }
  const SwarmSpec s{gps, G, swarm_type, beta, fmin, scaling, best_lower_bound, nullptr, clones};
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  return swarm_run(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed});
}

int sgp_swarm_run_path(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                       const double* fmin, const double* scaling, int64_t P, double* positions,
                       double* velocities, double* best_positions, double* best_values,
                       double* global_best, const double* velocity_scale,
                       const double* bounds, int init, int iters, double inertia0,
                       double step_size, const double* rand, uint64_t seed,
                       const double* Omega, const double* phase, int m, const double* w,
                       const double* v) {
  return sgp_swarm_run_path_shard(ctx, gps, G, beta, fmin, scaling, P, positions, velocities,
                                  best_positions, best_values, global_best, velocity_scale,
                                  bounds, init, iters, inertia0, step_size, rand, seed, Omega,
                                  phase, m, w, v, 0, P);
}

int sgp_swarm_run_path_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const double* scaling, int64_t P,
                             double* positions, double* velocities, double* best_positions,
                             double* best_values, double* global_best,
                             const double* velocity_scale, const double* bounds, int init,
                             int iters, double inertia0, double step_size, const double* rand,
                             uint64_t seed, const double* Omega, const double* phase, int m,
                             const double* w, const double* v, int64_t p0, int64_t P_total) {
  const SwarmSpec s{gps, G, kSwarmThompson, beta, fmin, scaling, 0.0, nullptr, nullptr};
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  const double* const pin[4] = {Omega, phase, w, v};
  return swarm_run_path(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed},
                        pin, m);
}

int sgp_swarm_fitness_mes(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                          int64_t P, double beta, const double* fmin, const double* scaling,
                          const double* ystar, int K, double floor, double* values,
                          uint8_t* safe, double* post) {
  SGP_TRY(swarm_mes_checks(ctx, gps, G, ystar, K, floor));
  if (P <= 0) return 0;
  SwarmMes mes;
  SGP_TRY(swarm_mes_stage(ctx, ystar, K, floor, P, post != nullptr, &mes));
  const SwarmSpec s{gps, G, kSwarmMes, beta, fmin, scaling, 0.0, nullptr, nullptr, &mes};
  SGP_TRY(swarm_fitness(ctx, s, particles, P, values, safe, nullptr));
  if (post) SGP_TRY(sgp_d2h(ctx, post, mes.post, 2 * size_t(P) * 8));
  return 0;
}

int sgp_swarm_run_mes(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                      const double* fmin, const double* scaling, int64_t P, double* positions,
                      double* velocities, double* best_positions, double* best_values,
                      double* global_best, const double* velocity_scale,
                      const double* bounds, int init, int iters, double inertia0,
                      double step_size, const double* rand, uint64_t seed,
                      const double* ystar, int K, double floor) {
  return sgp_swarm_run_mes_shard(ctx, gps, G, beta, fmin, scaling, P, positions, velocities,
                                 best_positions, best_values, global_best, velocity_scale,
                                 bounds, init, iters, inertia0, step_size, rand, seed, ystar, K,
                                 floor, 0, P);
}

int sgp_swarm_run_mes_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, const double* scaling, int64_t P,
                            double* positions, double* velocities, double* best_positions,
                            double* best_values, double* global_best,
                            const double* velocity_scale, const double* bounds, int init,
                            int iters, double inertia0, double step_size, const double* rand,
                            uint64_t seed, const double* ystar, int K, double floor,
                            int64_t p0, int64_t P_total) {
  SGP_TRY(swarm_mes_checks(ctx, gps, G, ystar, K, floor));
  if (P <= 0 && P_total <= 0) return 0;
  SwarmMes mes;
  SGP_TRY(swarm_mes_stage(ctx, ystar, K, floor, P, false, &mes));
  const SwarmSpec s{gps, G, kSwarmMes, beta, fmin, scaling, 0.0, nullptr, nullptr, &mes};
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  return swarm_run(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed});
}

int sgp_swarm_fitness_ise(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                          int64_t P, double beta, const double* fmin, const double* scaling,
                          const double* targets, const double* zmean, const double* zvar, int T,
                          double* values, uint8_t* safe, double* alpha, int64_t* target,
                          double* post, double* pairs, double* cov) {
  const SwarmIseIn in{targets, zmean, zvar, T, alpha, target, post, pairs, cov};
  SGP_TRY(swarm_ise_checks(ctx, gps, G, fmin, in));
  if (P <= 0) return 0;
  SGP_TRY(swarm_ise_out_check(ctx, G, P, in));
  const SwarmSpec s{gps, G, kSwarmIse, beta, fmin, scaling, 0.0, nullptr, nullptr, nullptr, &in};
  return swarm_fitness(ctx, s, particles, P, values, safe, nullptr);
}

int sgp_swarm_run_ise(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                      const double* fmin, const double* scaling, int64_t P, double* positions,
                      double* velocities, double* best_positions, double* best_values,
                      double* global_best, const double* velocity_scale,
                      const double* bounds, int init, int iters, double inertia0,
                      double step_size, const double* rand, uint64_t seed,
                      const double* targets, const double* zmean, const double* zvar, int T) {
  return sgp_swarm_run_ise_shard(ctx, gps, G, beta, fmin, scaling, P, positions, velocities,
                                 best_positions, best_values, global_best, velocity_scale,
                                 bounds, init, iters, inertia0, step_size, rand, seed, targets,
                                 zmean, zvar, T, 0, P);
}

int sgp_swarm_run_ise_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, const double* scaling, int64_t P,
                            double* positions, double* velocities, double* best_positions,
                            double* best_values, double* global_best,
                            const double* velocity_scale, const double* bounds, int init,
                            int iters, double inertia0, double step_size, const double* rand,
                            uint64_t seed, const double* targets, const double* zmean,
                            const double* zvar, int T, int64_t p0, int64_t P_total) {
  const SwarmIseIn in{targets, zmean, zvar, T, nullptr, nullptr, nullptr, nullptr, nullptr};
  SGP_TRY(swarm_ise_checks(ctx, gps, G, fmin, in));
  if (P <= 0 && P_total <= 0) return 0;
  const SwarmSpec s{gps, G, kSwarmIse, beta, fmin, scaling, 0.0, nullptr, nullptr, nullptr, &in};
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  return swarm_run(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed});
}

int sgp_swarm_fitness_ei(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                         int64_t P, double beta, const double* fmin, const double* scaling,
                         int kind, double tau, double xi, int weigh, int free_mode,
                         double* values, uint8_t* safe, double* alpha, double* post) {
  SwarmEi ei;
  SGP_TRY(swarm_ei_checks(ctx, gps, G, fmin, kind, tau, xi, weigh, free_mode, &ei));
  if (P <= 0) return 0;
  SGP_CHECK(ctx, G <= SGP_MAX_GPS, "%d GPs, supported 1..%d", G, SGP_MAX_GPS);
  const SwarmEiLayout l = swarm_ei_layout(P, G, alpha != nullptr, post != nullptr);   // (common.h)
  if (l.bytes) {
    char* buf;
    SGP_TRY(sgp_scratch(ctx, kSlotEiIn, l.bytes, &buf));
    if (alpha) ei.alpha = reinterpret_cast<double*>(buf + l.alpha);
    if (post) ei.post = reinterpret_cast<double*>(buf + l.post);
  }
  SwarmSpec s{gps, G, kSwarmEi, beta, fmin, scaling, 0.0, nullptr, nullptr, nullptr};
  s.ei = &ei;
  SGP_TRY(swarm_fitness(ctx, s, particles, P, values, safe, nullptr));
  if (alpha) SGP_TRY(sgp_d2h(ctx, alpha, ei.alpha, size_t(P) * 8));
  if (post) SGP_TRY(sgp_d2h(ctx, post, ei.post, 2 * size_t(G) * size_t(P) * 8));
  return 0;
}

int sgp_swarm_run_ei(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta, const double* fmin,
                     const double* scaling, int64_t P, double* positions, double* velocities,
                     double* best_positions, double* best_values, double* global_best,
                     const double* velocity_scale, const double* bounds, int init, int iters,
                     double inertia0, double step_size, const double* rand, uint64_t seed,
                     int kind, double tau, double xi, int weigh, int free_mode) {
  return sgp_swarm_run_ei_shard(ctx, gps, G, beta, fmin, scaling, P, positions, velocities,
                                best_positions, best_values, global_best, velocity_scale,
                                bounds, init, iters, inertia0, step_size, rand, seed, kind, tau,
                                xi, weigh, free_mode, 0, P);
}

int sgp_swarm_run_ei_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                           const double* fmin, const double* scaling, int64_t P,
                           double* positions, double* velocities, double* best_positions,
                           double* best_values, double* global_best,
                           const double* velocity_scale, const double* bounds, int init,
                           int iters, double inertia0, double step_size, const double* rand,
                           uint64_t seed, int kind, double tau, double xi, int weigh,
                           int free_mode, int64_t p0, int64_t P_total) {
  SwarmEi ei;
  SGP_TRY(swarm_ei_checks(ctx, gps, G, fmin, kind, tau, xi, weigh, free_mode, &ei));
  if (P <= 0 && P_total <= 0) return 0;
  SwarmSpec s{gps, G, kSwarmEi, beta, fmin, scaling, 0.0, nullptr, nullptr, nullptr};
  s.ei = &ei;
  const SwarmState st{positions, velocities, best_positions, best_values, global_best,
                      velocity_scale, bounds, P, p0, P_total};
  return swarm_run(ctx, s, st, PsoSchedule{init, iters, inertia0, step_size, rand, seed});
}

// SafeOptSwarm safe-set growth, gp_opt.py:1089-1111 (kernels in swarm.hip).
int sgp_swarm_grow(sgp_ctx* ctx, sgp_gp* gp0, const double* S, int64_t m,
                   const double* B, int64_t n, double scale2, double thr,
                   uint8_t* accept) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp0 != nullptr, "no GP");
  SGP_CHECK(ctx, m >= 0 && n >= 0 && n <= INT32_MAX, "bad sizes m=%lld n=%lld",
            (long long)m, (long long)n);
  if (n == 0) return 0;
  const int d = gp0->kern.d;
  const GrowLayout l = grow_layout(m, n, d);          // (common.h)
  char* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotWork, l.bytes + 64, &buf));
  const GrowBufs gb = grow_bufs(buf, l);
  SGP_TRY(sgp_h2d(ctx, gb.S, S, size_t(m) * d * 8));
  SGP_TRY(sgp_h2d(ctx, gb.B, B, size_t(n) * d * 8));
  SGP_TRY(launch_swarm_grow(ctx, gp0->kern, gb.S, m, gb.B, int(n), scale2, thr, gb));
  return sgp_d2h(ctx, accept, gb.accept, size_t(n));
}

}  // extern "C"
