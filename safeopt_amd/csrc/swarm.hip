// SafeOptSwarm safe-set growth on the device.
//
// Replaces the step after every maximizer / expander swarm run
// (safeopt/gp_opt.py:1089-1111): with C = k(B, [S; B]) / scaling[0]^2 for the
// swarm's best positions B (n x d) against the current safe set S (m x d),
// candidate j is appended iff C[j, p] <= 0.95 for every point p of S and for
// every candidate accepted before it.  The reference materialises the
// n x (m + n) matrix on the host and loops over j; here the covariance matrix is
// never stored and the order is resolved in ceil(n / kGrowBlock) serial steps:
//   k_grow_vs_set      : every candidate against S -- a 1-D grid over (tile of 256
//                        candidates x chunk of S staged in LDS), one flag per candidate
//   per block of kGrowBlock candidates, in order:
//     k_grow_vs_accepted : the block against the candidates accepted in EARLIER blocks,
//                          over the chip (tile x chunk of the accepted list in LDS)
//     k_grow_block       : one workgroup: the block's strictly lower triangular conflict
//                          matrix as bitmasks, the order resolved by one wave over those
//                          bitmasks, the accepted candidates appended to the list in order
// Every covariance is kern_eval<D>(kd, candidate, other) / scale2 with the candidate
// first, as the reference's row j of C.  Against S the values fold with fmax (a NaN
// value drops out) and the candidate is rejected iff !(max <= thr); against accepted
// candidates any value with !(c <= thr) rejects (NaN rejects).  Scratch: GrowLayout
// (common.h).
#include "kern_eval.h"
#include "fitness.h"
#include "small_path.h"

namespace {

constexpr int kGrowTile = 256;    // candidates per workgroup of the chip-wide kernels
constexpr int kGrowChunk = 512;   // safe-set points / accepted candidates staged in LDS
constexpr int kGrowWords = kGrowBlock / 64;

template <int D>
__global__ __launch_bounds__(kGrowTile) void k_grow_vs_set(KernDesc kd, const double* S,
                                                           int64_t m, const double* B, int n,
                                                           int ntile, double scale2,
                                                           double thr, uint8_t* flag) {
  __shared__ double sh[kGrowChunk * D];
  const int tile = int(blockIdx.x % unsigned(ntile));
  const int64_t p0 = int64_t(blockIdx.x / unsigned(ntile)) * kGrowChunk;
  const int np = int(min(int64_t(kGrowChunk), m - p0));
  for (int e = threadIdx.x; e < np * D; e += kGrowTile) sh[e] = S[p0 * D + e];
  __syncthreads();
  const int j = tile * kGrowTile + int(threadIdx.x);
  if (j >= n || flag[j]) return;       // (a flag set by another chunk: nothing to add)
  double b[D];
#pragma unroll
  for (int k = 0; k < D; ++k) b[k] = B[int64_t(j) * D + k];
  double mx = -INFINITY;
  for (int p = 0; p < np; ++p) {
    mx = fmax(mx, kern_eval<D>(kd, b, sh + p * D) / scale2);
    if (!(mx <= thr)) break;           // (mx is never NaN: fmax drops NaN values)
  }
  if (!(mx <= thr)) flag[j] = 1;
}

template <int D>
__global__ __launch_bounds__(kGrowTile) void k_grow_vs_accepted(KernDesc kd, const double* B,
                                                                int j0, int nb, int ntile,
                                                                const int* list,
                                                                const int* count, double scale2,
                                                                double thr, uint8_t* flag) {
  __shared__ double sh[kGrowChunk * D];
  const int na = *count;
  const int tile = int(blockIdx.x % unsigned(ntile));
  const int a0 = int(blockIdx.x / unsigned(ntile)) * kGrowChunk;
  if (a0 >= na) return;                // (uniform: fewer accepted than the grid allows)
  const int np = min(kGrowChunk, na - a0);
  for (int e = threadIdx.x; e < np * D; e += kGrowTile) {
    const int a = e / D;
    sh[e] = B[int64_t(list[a0 + a]) * D + (e - a * D)];
  }
  __syncthreads();
  const int r = tile * kGrowTile + int(threadIdx.x);
  if (r >= nb) return;
  const int j = j0 + r;
  if (flag[j]) return;
  double b[D];
#pragma unroll
  for (int k = 0; k < D; ++k) b[k] = B[int64_t(j) * D + k];
  for (int p = 0; p < np; ++p)
    if (!(kern_eval<D>(kd, b, sh + p * D) / scale2 <= thr)) {
      flag[j] = 1;
      break;
    }
}

template <int D>
__global__ __launch_bounds__(1024) void k_grow_block(KernDesc kd, const double* B, int j0,
                                                     int nb, double scale2, double thr,
                                                     const uint8_t* flag, int* list,
                                                     int* count, uint8_t* accept) {
  __shared__ double sb[kGrowBlock * D];
  __shared__ unsigned long long conf[kGrowBlock][kGrowWords];   // bit k of row i: k < i clashes
  __shared__ unsigned long long alive[kGrowWords], acc[kGrowWords];
  const int t = threadIdx.x;
  const int na = *count;               // (thread 0 writes it back after the last barrier)
  for (int e = t; e < nb * D; e += 1024) sb[e] = B[int64_t(j0) * D + e];
  {
    const bool ok = t < nb && !flag[j0 + t];
    const unsigned long long w = __ballot(ok);
    if ((t & 63) == 0 && (t >> 6) < kGrowWords) alive[t >> 6] = w;
  }
  __syncthreads();
  // conflict words: item (i, w) = row i against the candidates 64 w .. 64 w + 63 before it
  for (int it = t; it < kGrowBlock * kGrowWords; it += 1024) {
    const int i = it / kGrowWords, w = it % kGrowWords;
    unsigned long long word = 0;
    if (i < nb && w <= (i >> 6) && ((alive[i >> 6] >> (i & 63)) & 1ULL)) {
      const unsigned long long live = alive[w];
      const int kend = min(64, i - 64 * w);
      for (int q = 0; q < kend; ++q)
        if ((live >> q) & 1ULL)
          if (!(kern_eval<D>(kd, sb + i * D, sb + (64 * w + q) * D) / scale2 <= thr))
            word |= 1ULL << q;
    }
    conf[i][w] = word;
  }
  __syncthreads();
  // the order: lane l holds word l of the accepted bits; candidate i is accepted iff it is
  // alive and clashes with none of the accepted candidates before it
  if (t < 64) {
    unsigned long long a = 0;
    for (int i = 0; i < nb; ++i) {
      if (!((alive[i >> 6] >> (i & 63)) & 1ULL)) continue;    // (wave-uniform)
      const unsigned long long c = t < kGrowWords ? conf[i][t] : 0ULL;
      const unsigned long long hit = __ballot((c & a) != 0ULL);
      if (hit == 0ULL && t == (i >> 6)) a |= 1ULL << (i & 63);
    }
    if (t < kGrowWords) acc[t] = a;
  }
  __syncthreads();
  // accept[] of the block and the accepted candidates appended in order
  if (t < nb) {
    const int w = t >> 6;
    const unsigned long long bit = 1ULL << (t & 63);
    const bool ok = (acc[w] & bit) != 0ULL;
    accept[j0 + t] = ok ? 1 : 0;
    if (ok) {
      int pos = na + __popcll(acc[w] & (bit - 1ULL));
      for (int v = 0; v < w; ++v) pos += __popcll(acc[v]);
      list[pos] = j0 + t;
    }
  }
  if (t == 0) {
    int tot = na;
    for (int v = 0; v < kGrowWords; ++v) tot += __popcll(acc[v]);
    *count = tot;
  }
}

template <int D>
int grow_launches(sgp_ctx* ctx, const KernDesc& kd, const double* S, int64_t m,
                  const double* B, int n, double scale2, double thr, const GrowBufs& gb) {
  const int ntile = (n + kGrowTile - 1) / kGrowTile;
  const int64_t nchunk = (m + kGrowChunk - 1) / kGrowChunk;
  SGP_CHECK(ctx, int64_t(ntile) * nchunk <= INT32_MAX, "safe set too large (m=%lld, n=%d)",
            (long long)m, n);
  if (nchunk > 0)
    hipLaunchKernelGGL(k_grow_vs_set<D>, dim3(unsigned(ntile * nchunk)), dim3(kGrowTile), 0,
                       ctx->stream, kd, S, m, B, n, ntile, scale2, thr, gb.flag);
  for (int j0 = 0; j0 < n; j0 += kGrowBlock) {
    const int nb = min(kGrowBlock, n - j0);
    if (j0 > 0) {
      // as many chunks as the earlier blocks could have accepted; the surplus returns at once
      const int bt = (nb + kGrowTile - 1) / kGrowTile;
      const int nc = (j0 + kGrowChunk - 1) / kGrowChunk;
      hipLaunchKernelGGL(k_grow_vs_accepted<D>, dim3(unsigned(bt * nc)), dim3(kGrowTile), 0,
                         ctx->stream, kd, B, j0, nb, bt, gb.list, gb.count, scale2, thr,
                         gb.flag);
    }
    hipLaunchKernelGGL(k_grow_block<D>, dim3(1), dim3(1024), 0, ctx->stream, kd, B, j0, nb,
                       scale2, thr, gb.flag, gb.list, gb.count, gb.accept);
  }
  return 0;
}

}  // namespace

int launch_swarm_grow(sgp_ctx* ctx, const KernDesc& kd, const double* S, int64_t m,
                      const double* B, int n, double scale2, double thr, const GrowBufs& gb) {
  SGP_HIP(ctx, hipMemsetAsync(gb.flag, 0, size_t(n), ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(gb.count, 0, sizeof(int), ctx->stream));
#define GROW_CASE(DD) \
  case DD:            \
    SGP_TRY(grow_launches<DD>(ctx, kd, S, m, B, n, scale2, thr, gb)); \
    break;
  switch (kd.d) {
    GROW_CASE(1) GROW_CASE(2) GROW_CASE(3) GROW_CASE(4)
    GROW_CASE(5) GROW_CASE(6) GROW_CASE(7) GROW_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", kd.d, SGP_MAX_D);
      return -2;
  }
#undef GROW_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// ---- particle swarm on the device ---------------------------------------------------
// SwarmOptimization.init_swarm / run_swarm (safeopt/swarm.py:61-146) with the
// swarm state resident in HBM for the whole run; the fitness is the posterior
// sweep + shaping pass (launch_sweep_fitness) on the same buffers.  This file is
// built with -ffp-contract=off and the update below mirrors NumPy's evaluation
// order, so that with the reference's own random numbers (rand != nullptr,
// drawn by np.random.rand on the host in the reference's order) the run is
// bit-identical to the host implementation.
namespace {

// Philox4x32-10 (Salmon et al., SC'11): counter-based, no state to keep.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0,
                                             uint32_t k1) {
  const uint64_t p0 = uint64_t(0xD2511F53u) * c[0];
  const uint64_t p1 = uint64_t(0xCD9E8D57u) * c[2];
  const uint32_t n0 = uint32_t(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = uint32_t(p0 >> 32) ^ c[3] ^ k1;
  c[1] = uint32_t(p1);
  c[3] = uint32_t(p0);
  c[0] = n0;
  c[2] = n2;
}

// e-th uniform double in [0, 1) of stream (seed, draw): 53 random bits.
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint32_t draw,
                                                 uint64_t e) {
  uint32_t c[4] = {uint32_t(e >> 1), uint32_t(e >> 33), draw, 0x5afe0b7u};
  uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint64_t bits = (e & 1) ? ((uint64_t(c[2]) << 32) | c[3])
                                : ((uint64_t(c[0]) << 32) | c[1]);
  return double(bits >> 11) * (1.0 / 9007199254740992.0);
}

// velocities = rand(P, d) * velocity_scale          (swarm.py:75-76)
__global__ void k_pso_init_vel(int64_t P, int d, double* vel,
                               const double* vscale, const double* rand,
                               uint64_t seed, int64_t e0) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= P * d) return;
  const double r = rand ? rand[e] : philox_uniform(seed, 0u, uint64_t(e0 + e));
  vel[e] = r * vscale[e % d];
}

// one velocity / position update                     (swarm.py:98-123)
__global__ void k_pso_move(int64_t P, int d, double* pos, double* vel,
                           const double* best, const double* gbest,
                           const double* vscale, const double* bounds,
                           double inertia, const double* rand, uint64_t seed,
                           uint32_t draw, int64_t e0, int64_t e2) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= P * d) return;
  const int k = int(e % d);
  const double x = pos[e];
  const double to_global = gbest[k] - x;
  const double to_own = best[e] - x;
  // r = rand(2 P, d); r1 = r[:P], r2 = r[P:] (of the whole swarm: element e0 + e, e2 + e)
  const double r1 = rand ? rand[e] : philox_uniform(seed, draw, uint64_t(e0 + e));
  const double r2 = rand ? rand[P * d + e]
                         : philox_uniform(seed, draw, uint64_t(e2 + e));
  double v = vel[e] * inertia;
  v = v + (r1 * to_own + r2 * to_global) / vscale[k];
  const double vmax = 10.0 * vscale[k];
  v = fmin(fmax(v, -vmax), vmax);
  vel[e] = v;
  double xn = x + v;
  if (bounds) xn = fmin(fmax(xn, bounds[2 * k]), bounds[2 * k + 1]);
  pos[e] = xn;
}

// personal bests                                     (swarm.py:77-79, 138-143)
__global__ void k_pso_best(int64_t P, int d, const double* values,
                           const uint8_t* safe, const double* pos, double* best,
                           double* best_values, int init) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const bool better = init || (values[i] > best_values[i] && safe[i]);
  if (better) {
    best_values[i] = values[i];
    for (int k = 0; k < d; ++k) best[i * d + k] = pos[i * d + k];
  }
}

// global_best = best_positions[argmax(best_values)], first index on ties; rec: the
// record of a rank's block instead (value | p0 + index | x[d])
__global__ __launch_bounds__(1024) void k_pso_gbest(int64_t P, int d,
                                                    const double* best_values,
                                                    const double* best,
                                                    double* gbest, double* rec,
                                                    int64_t p0) {
  __shared__ double sv[1024 / 64];
  __shared__ long long si[1024 / 64];
  double v = -INFINITY;
  long long idx = -1;
  for (int64_t i = threadIdx.x; i < P; i += 1024) {
    const double x = best_values[i];
    if (idx < 0 || x > v) {      // strided scan keeps the lowest index per thread
      v = x;
      idx = i;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const long long oi = __shfl_xor(idx, o, 64);
    if (oi >= 0 && (idx < 0 || ov > v || (ov == v && oi < idx))) {
      v = ov;
      idx = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 1024 / 64; ++w)
      if (si[w] >= 0 && (idx < 0 || sv[w] > v || (sv[w] == v && si[w] < idx))) {
        v = sv[w];
        idx = si[w];
      }
    if (rec) {
      rec[0] = v;
      rec[1] = __longlong_as_double(p0 + idx);
      for (int k = 0; k < d; ++k) rec[2 + k] = best[idx * d + k];
    } else {
      for (int k = 0; k < d; ++k) gbest[k] = best[idx * d + k];
    }
  }
}

// the swarm's global best from the records of the ranks (rank order = order of the
// blocks): the largest value, the lowest global index on ties -- the rule of k_pso_gbest
__global__ void k_pso_gbest_merge(const double* recs, int world, int d, double* gbest) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int best = 0;
  for (int r = 1; r < world; ++r) {
    const double* a = recs + size_t(r) * (2 + d);
    const double* b = recs + size_t(best) * (2 + d);
    const long long ia = __double_as_longlong(a[1]), ib = __double_as_longlong(b[1]);
    if (a[0] > b[0] || (a[0] == b[0] && ia < ib)) best = r;
  }
  for (int k = 0; k < d; ++k) gbest[k] = recs[size_t(best) * (2 + d) + 2 + k];
}

// Fitness of a few particles from resident mean / var ([G][P]): the path of
// SafeOptSwarm._compute_particle_fitness for P <= kSmallPoints.
__global__ void k_fitness_small(int G, int64_t P, const double* mean,
                                const double* var, FitnessArgs f) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= P) return;
  double out;
  bool ok;
  shape_particle(f, G,
                 [&](int g, double* mu, double* v) {
                   *mu = mean[int64_t(g) * P + i];
                   *v = var[int64_t(g) * P + i];
                 },
                 &out, &ok);
  f.values[i] = out;
  f.safe[i] = ok ? 1 : 0;
}

// The same for a hallucinated swarm (f.down, launch_swarm_down in front of it): the width
// term from var_h = max(var - down, 1e-15), everything else from the real posterior.
__global__ void k_fitness_hall(int G, int64_t P, const double* mean, const double* var,
                               FitnessArgs f) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= P) return;
  double out;
  bool ok;
  shape_particle<true>(
      f, G,
      [&](int g, double* mu, double* v) {
        *mu = mean[int64_t(g) * P + i];
        *v = var[int64_t(g) * P + i];
      },
      &out, &ok, [&](int g) { return f.down[int64_t(g) * P + i]; },
      [&](int g, double vh) {
        if (f.var_h) f.var_h[int64_t(g) * P + i] = vh;
      });
  f.values[i] = out;
  f.safe[i] = ok ? 1 : 0;
}

// One PSO iteration of a small swarm (P <= kSmallSwarm) behind the two posterior launches
// (k_small_kb, k_small_mfma), in ONE workgroup: block sums -> mean / var of every
// GP, fitness, personal bests, global best (first index on ties) and the move
// that opens the next iteration.  Same arithmetic, statement for statement, as
// k_small_post + k_fitness_small + k_pso_best + k_pso_gbest + k_pso_move.
// post_mean != nullptr: the posterior comes from a sweep ([G][P] mean | var, the GPs with
// fewer observations than the few-points path wants): no block sums, the rest as above.
__global__ __launch_bounds__(1024) void k_pso_small_step(const GpDev* gps, int G,
                                                         SmallBufs sb, FitnessArgs f,
                                                         PsoSmallArgs ps,
                                                         const double* post_mean,
                                                         const double* post_var) {
  __shared__ double sh[4][16][16];
  __shared__ double smean[SGP_MAX_GPS][kSmallSwarm], svar[SGP_MAX_GPS][kSmallSwarm];
  __shared__ double sbv[kSmallSwarm];
  const int t = threadIdx.x, P = ps.P, d = ps.d;
  const int Geff = (f.swarm_type == SGP_SWARM_GREEDY) ? 1 : G;
  // block sums of (GP, pass) pairs, four pairs side by side
  const int grp = t >> 8, tl = t & 255, npairs = post_mean ? 0 : Geff * sb.passes;
  if (post_mean) {
    for (int e = t; e < Geff * P; e += 1024) {
      smean[e / P][e % P] = post_mean[e];
      svar[e / P][e % P] = post_var[e];
    }
  }
  for (int base = 0; base < npairs; base += 4) {
    const int pair = base + grp;
    const bool valid = pair < npairs;
    const int g = valid ? pair / sb.passes : 0, pass = valid ? pair % sb.passes : 0;
    const double tot = small_block_sum(sb.part + g * sb.part_stride, sb.nblk_max,
                                       valid ? gps[g].nblk : 0, pass, sh[grp], tl);
    const int p = pass * 16 + (tl & 15);
    if (valid && (tl >> 4) == 0 && p < P) {
      smean[g][p] = sb.mtmp[g * sb.passes * 16 + p];
      svar[g][p] = fmax(gps[g].kern.kdiag - tot, 1e-15);      // GPy clip
    }
  }
  __syncthreads();
  if (t < P) {
    double out;
    bool ok;
    shape_particle(f, G,
                   [&](int g, double* mu, double* v) {
                     *mu = smean[g][t];
                     *v = svar[g][t];
                   },
                   &out, &ok);
    f.values[t] = out;
    f.safe[t] = ok ? 1 : 0;
    // personal bests (k_pso_best)
    const bool better = ps.init || (out > ps.best_values[t] && ok);
    double bv = ps.best_values[t];
    if (better) {
      bv = out;
      ps.best_values[t] = out;
      for (int k = 0; k < d; ++k) ps.best[t * d + k] = ps.pos[t * d + k];
    }
    sbv[t] = bv;
  }
  __syncthreads();
  // global best: argmax of the personal bests, first index on ties (k_pso_gbest)
  if (t < 64) {
    double v = t < P ? sbv[t] : -INFINITY;
    long long idx = t < P ? t : -1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const long long oi = __shfl_xor(idx, o, 64);
      if (oi >= 0 && (idx < 0 || ov > v || (ov == v && oi < idx))) {
        v = ov;
        idx = oi;
      }
    }
    if (t < d) ps.gbest[t] = ps.best[idx * d + t];
  }
  if (!ps.move) return;
  __syncthreads();
  // the move that opens the next iteration (k_pso_move)
  for (int e = t; e < P * d; e += 1024) {
    const int k = e % d;
    const double x = ps.pos[e];
    const double to_global = ps.gbest[k] - x;
    const double to_own = ps.best[e] - x;
    const double r1 = ps.rand ? ps.rand[e] : philox_uniform(ps.seed, ps.draw, uint64_t(e));
    const double r2 = ps.rand ? ps.rand[P * d + e]
                              : philox_uniform(ps.seed, ps.draw, uint64_t(P * d + e));
    double v = ps.vel[e] * ps.inertia;
    v = v + (r1 * to_own + r2 * to_global) / ps.vscale[k];
    const double vmax = 10.0 * ps.vscale[k];
    v = fmin(fmax(v, -vmax), vmax);
    ps.vel[e] = v;
    double xn = x + v;
    if (ps.bounds) xn = fmin(fmax(xn, ps.bounds[2 * k]), ps.bounds[2 * k + 1]);
    ps.pos[e] = xn;
  }
}

}  // namespace

int launch_pso_init_vel(sgp_ctx* ctx, int64_t P, int d, double* vel,
                        const double* vscale, const double* rand, uint64_t seed,
                        int64_t e0) {
  hipLaunchKernelGGL(k_pso_init_vel, dim3(unsigned((P * d + 255) / 256)),
                     dim3(256), 0, ctx->stream, P, d, vel, vscale, rand, seed, e0);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_pso_move(sgp_ctx* ctx, int64_t P, int d, double* pos, double* vel,
                    const double* best, const double* gbest, const double* vscale,
                    const double* bounds, double inertia, const double* rand,
                    uint64_t seed, uint32_t draw, int64_t e0, int64_t e2) {
  hipLaunchKernelGGL(k_pso_move, dim3(unsigned((P * d + 255) / 256)), dim3(256), 0,
                     ctx->stream, P, d, pos, vel, best, gbest, vscale, bounds,
                     inertia, rand, seed, draw, e0, e2 < 0 ? P * d : e2);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_pso_best(sgp_ctx* ctx, int64_t P, int d, const double* values,
                    const uint8_t* safe, const double* pos, double* best,
                    double* best_values, double* gbest, int init, double* rec,
                    int64_t p0) {
  hipLaunchKernelGGL(k_pso_best, dim3(unsigned((P + 255) / 256)), dim3(256), 0,
                     ctx->stream, P, d, values, safe, pos, best, best_values, init);
  hipLaunchKernelGGL(k_pso_gbest, dim3(1), dim3(1024), 0, ctx->stream, P, d,
                     best_values, best, gbest, rec, p0);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_pso_gbest_merge(sgp_ctx* ctx, const double* recs, int world, int d, double* gbest) {
  hipLaunchKernelGGL(k_pso_gbest_merge, dim3(1), dim3(64), 0, ctx->stream, recs, world, d,
                     gbest);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_fitness_small(sgp_ctx* ctx, int G, int64_t P, const double* mean,
                         const double* var, FitnessArgs fa) {
  if (fa.down)
    hipLaunchKernelGGL(k_fitness_hall, dim3(unsigned((P + 255) / 256)), dim3(256),
                       0, ctx->stream, G, P, mean, var, fa);
  else
    hipLaunchKernelGGL(k_fitness_small, dim3(unsigned((P + 255) / 256)), dim3(256),
                       0, ctx->stream, G, P, mean, var, fa);
  SGP_HIP(ctx, hipGetLastError());
  // a 'mes' swarm: alpha of GP 0's posterior (mean[0][p], var[0][p]) on top of the penalty
  // the shaping left in the values -- both posterior routes end here
  if (fa.swarm_type == kSwarmMes) return launch_swarm_mes(ctx, P, mean, var, fa.mes, fa.values);
  // an 'ise' swarm: alpha over the staged targets, from every active GP's posterior
  if (fa.swarm_type == kSwarmIse)
    return launch_swarm_ise(ctx, G, P, mean, var, fa.fmin, *fa.ise, fa.values);
  // an 'ei' swarm: log expected improvement from all G GPs' posterior, on top of the penalty
  // (or, free, in its place)
  if (fa.swarm_type == kSwarmEi)
    return launch_swarm_ei(ctx, G, P, mean, var, fa.ei, fa.values, fa.safe);
  return 0;
}

int launch_pso_small_step(sgp_ctx* ctx, const GpDev* gps_dev, int G, const SmallBufs& sb,
                          FitnessArgs fa, PsoSmallArgs ps, const double* post_mean,
                          const double* post_var) {
  hipLaunchKernelGGL(k_pso_small_step, dim3(1), dim3(1024), 0, ctx->stream, gps_dev, G,
                     sb, fa, ps, post_mean, post_var);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
