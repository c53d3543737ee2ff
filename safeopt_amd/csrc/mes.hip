// Max-value entropy search (Wang & Jegelka 2017, "Max-value entropy search for efficient
// Bayesian optimization") over the resident posterior of the objective GP:
//
//   sigma    = sqrt(max(v, 1e-15))
//   y_k      = max(y*_k, floor)                     k = 0 .. K - 1  (floor = -inf: none)
//   gamma_k  = (y_k - mu) / sigma
//   alpha(x) = (1 / K) sum_k term(gamma_k),         the terms added in the order of k
//   term(g)  = g phi(g) / (2 Phi(g)) - ln Phi(g)
//
// y*_k are maxima of the objective (the per-path maxima of sgp_grid_paths over the safe set).
// The default floor is the largest posterior mean of the candidates' safe set: a maximum
// cannot lie below a value the mean already reaches, and a y*_k that does -- the random
// Fourier prior of a path is approximate, and its maximum is taken over S only -- would give
// gamma < 0, a term that grows like gamma^2 / 2 and a pick that collapses onto the row with
// the smallest sigma.
//
// term() through ONE scaled complementary error function, finite and accurate over the whole
// range, +inf included (mes_term): the naive form is inf / NaN from gamma = -38 down and has
// no digits left above +8.
//
// One thread per row, K <= 64 terms per row, each an erfcx, an exp and a log or log1p in
// fp64: the pass is bound by the fp64 VALU, not by the 17 bytes per row it reads.  The K
// floored maxima are staged in LDS once per workgroup (every lane reads the same word: a
// broadcast).  A row's alpha is a function of (mu, v, y, floor) alone -- the same device
// function (mes_term.h) and the same order of additions in the row kernel (sgp_mes_eval), in
// the grid kernel and in the particle kernel of a 'mes' swarm (k_swarm_mes, behind the shaping
// pass of sgp_swarm_fitness_mes / sgp_swarm_run_mes) -- so it has the same bits whatever N,
// the launch shape, the row's position or the rank.  The arg-max is an epilogue: per-workgroup (value, local row) pairs, one small
// final kernel; the largest value, the lowest row among equals, rows outside the mask never.
// No atomics.  The floor is reduced on the device and read from device memory by the grid
// kernel: nothing comes back to the host between the two.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "mes_term.h"
#include "sweep_shared.h"

namespace {

constexpr int kMesThreads = 256;              // rows of a workgroup of the row / grid kernels
constexpr int kMesFloorWg = 1024;             // workgroups of the floor reduction, at most
constexpr int64_t kMesEvalRows = 1 << 20;     // rows per launch of sgp_mes_eval
constexpr long long kNoRow = std::numeric_limits<long long>::max();

// (value, row) pairs: the larger value, the lower row among equals
__device__ __forceinline__ void take_better(double& v, long long& i, double v2, long long i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// sgp_mes_eval: out[r] = alpha(mean[r], var[r])
__global__ __launch_bounds__(kMesThreads) void k_mes_rows(const double* mean, const double* var,
                                                          int64_t N, const double* ystar, int K,
                                                          const double* floor, double* out) {
  __shared__ double ys[SGP_MAX_MES];
  stage_ystar(ys, ystar, K, floor);
  const int64_t row = int64_t(blockIdx.x) * kMesThreads + threadIdx.x;
  if (row < N) out[row] = mes_alpha(mean[row], var[row], ys, K);
}

struct MesArgs {
  const double* mean;     // [N] of GP 0
  const double* var;
  int64_t N;
  const double* ystar;    // [K]
  int K;
  const double* floor;    // one word
  const uint8_t* mask1;   // a candidate row has a byte set in mask1 or mask2; both null: every row
  const uint8_t* mask2;
  double* alpha;          // [N], or null
  double* pval;           // [gridDim.x] best value of the workgroup's rows
  long long* pidx;        //   ... and its LOCAL row (kNoRow: none)
};

__global__ __launch_bounds__(kMesThreads) void k_mes_grid(MesArgs a) {
  __shared__ double ys[SGP_MAX_MES];
  __shared__ double rv[kMesThreads / 64];
  __shared__ long long ri[kMesThreads / 64];
  stage_ystar(ys, a.ystar, a.K, a.floor);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = int64_t(blockIdx.x) * kMesThreads + tid;
  double v = -INFINITY;
  long long i = kNoRow;
  if (row < a.N) {
    const double al = mes_alpha(a.mean[row], a.var[row], ys, a.K);
    if (a.alpha) a.alpha[row] = al;
    const bool all = !a.mask1 && !a.mask2;
    if (all || (a.mask1 && a.mask1[row]) || (a.mask2 && a.mask2[row])) {
      v = al;
      i = row;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double v2 = __shfl_xor(v, o, 64);
    const long long i2 = __shfl_xor(i, o, 64);
    take_better(v, i, v2, i2);
  }
  if (lane == 0) {
    rv[wave] = v;
    ri[wave] = i;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kMesThreads / 64; ++w) take_better(v, i, rv[w], ri[w]);
    a.pval[blockIdx.x] = v;
    a.pidx[blockIdx.x] = i;
  }
}

// One workgroup: the best of the workgroups' pairs -> out[0] = value, out[1] = GLOBAL row
// (as int64; -inf and -1 when no row qualified).
__global__ __launch_bounds__(256) void k_mes_final(const double* pval, const long long* pidx,
                                                   int nwg, int64_t goff, double* out) {
  __shared__ double sv[256];
  __shared__ long long si[256];
  const int tid = threadIdx.x;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int w = tid; w < nwg; w += 256) take_better(v, i, pval[w], pidx[w]);
  sv[tid] = v;
  si[tid] = i;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) take_better(sv[tid], si[tid], sv[tid + o], si[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = si[0] == kNoRow ? -INFINITY : sv[0];
    reinterpret_cast<long long*>(out)[1] = si[0] == kNoRow ? -1 : si[0] + goff;
  }
}

// The ranks' records {value, GLOBAL row (-1: the shard has no candidate)} in rank order ->
// the record of the whole grid: take_better's order, a record without a row never wins.
__global__ __launch_bounds__(64) void k_mes_merge(const double* recs, int world, double* out) {
  if (threadIdx.x != 0) return;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int r = 0; r < world; ++r) {
    const long long i2 = reinterpret_cast<const long long*>(recs)[2 * r + 1];
    if (i2 >= 0) take_better(v, i, recs[2 * r], i2);
  }
  out[0] = i == kNoRow ? -INFINITY : v;
  reinterpret_cast<long long*>(out)[1] = i == kNoRow ? -1 : i;
}

// part[b] = max of mean over the mask rows workgroup b walks (-inf: none); mask null: all
__global__ __launch_bounds__(256) void k_mes_floor(const double* mean, const uint8_t* mask,
                                                   int64_t N, double* part) {
  __shared__ double rv[4];
  double v = -INFINITY;
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < N; r += int64_t(gridDim.x) * 256)
    if (!mask || mask[r]) v = fmax(v, mean[r]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) rv[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(rv[0], rv[1]), fmax(rv[2], rv[3]));
}

__global__ void k_mes_set(double* p, double v) {
  if (threadIdx.x == 0) p[0] = v;
}

// The fitness term of a 'mes' swarm (sgp_swarm_fitness_mes / sgp_swarm_run_mes), behind the
// shaping pass of fitness.h (kSwarmMes): one thread per particle,
//   values[p] = alpha(mean[p], var[p]) + values[p],
// mean / var the posterior of GP 0 the shaping pass has just consumed, values[p] the
// total_pen it left.  The maxima are floored by the floor of the kernel argument while they
// are staged; alpha is mes_alpha's, the bits of k_mes_rows on the same (mu, v).
// post: [2][P] receives mu | v, or null.
__global__ __launch_bounds__(kMesThreads) void k_swarm_mes(const double* mean, const double* var,
                                                           int64_t P, const double* ystar, int K,
                                                           double floor, double* values,
                                                           double* post) {
  __shared__ double ys[SGP_MAX_MES];
  if (int(threadIdx.x) < K) ys[threadIdx.x] = fmax(ystar[threadIdx.x], floor);
  __syncthreads();
  const int64_t p = int64_t(blockIdx.x) * kMesThreads + threadIdx.x;
  if (p >= P) return;
  const double mu = mean[p], v = var[p];
  const double alpha = mes_alpha(mu, v, ys, K);
  values[p] = alpha + values[p];
  if (post) {
    post[p] = mu;
    post[P + p] = v;
  }
}

inline unsigned mes_blocks(int64_t N) { return unsigned((N + kMesThreads - 1) / kMesThreads); }

}  // namespace

// The argument checks the entry points share (common.h).
int mes_checks(sgp_ctx* ctx, const double* ystar, int K) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, K >= 1 && K <= SGP_MAX_MES, "K = %d maxima (1 .. SGP_MAX_MES = %d)", K,
            SGP_MAX_MES);
  for (int k = 0; k < K; ++k)
    SGP_CHECK(ctx, std::isfinite(ystar[k]), "ystar[%d] is not finite", k);
  return 0;
}

// values[p] = alpha_p + values[p] for the P particles whose posterior of GP 0 is mean / var
// (common.h).  The events time the kernel for scripts/bench_swarm_mes.py, as grid_mes times its
// row kernel; no flops are booked.
int launch_swarm_mes(sgp_ctx* ctx, int64_t P, const double* mean, const double* var,
                     const SwarmMes& m, double* values) {
  if (P <= 0) return 0;
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 0.0));
  hipLaunchKernelGGL(k_swarm_mes, dim3(mes_blocks(P)), dim3(kMesThreads), 0, ctx->stream, mean,
                     var, P, m.ystar, m.K, m.floor, values, m.post);
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}

namespace {

// The block of a grid call in kSlotMesPart, nwg workgroups of the grid kernel, nf of the
// floor reduction, world ranks (0: no communicator):
//   pval[nwg] | pidx[nwg] | fpart[nf] | own[2] | out[2] | floor | recs[world][2]
// out: the record {value, global row} the call returns, with the floor behind it -- ONE
// read-back of three words; the final kernel writes it.  With a communicator the final
// kernel writes own, this rank's record, instead, and the merge of the gathered records out.
struct MesScratch {
  double* pval;
  long long* pidx;
  double *fpart, *own, *out, *floor, *recs;
};
inline size_t mes_scratch_bytes(int nwg, int nf, int world) {
  return (2 * size_t(nwg) + size_t(nf) + 5 + 2 * size_t(world)) * 8;
}
inline MesScratch mes_scratch(double* base, int nwg, int nf) {
  MesScratch s;
  s.pval = base;
  s.pidx = reinterpret_cast<long long*>(base + nwg);
  s.fpart = base + 2 * size_t(nwg);
  s.own = s.fpart + nf;
  s.out = s.own + 2;
  s.floor = s.own + 4;
  s.recs = s.own + 5;
  return s;
}

int grid_mes(sgp_grid* g, const double* ystar, int K, int rows, int floor_mode,
             double floor_value, double* alpha, double* value, int64_t* gidx,
             double* floor_used, bool merge) {
  sgp_ctx* ctx = g->ctx;
  SGP_TRY(mes_checks(ctx, ystar, K));
  SGP_CHECK(ctx, rows == SGP_MES_ALL || rows == SGP_MES_S || rows == SGP_MES_MG,
            "rows = %d is not SGP_MES_ALL / SGP_MES_S / SGP_MES_MG", rows);
  SGP_CHECK(ctx, floor_mode == SGP_MES_FLOOR_NONE || floor_mode == SGP_MES_FLOOR_MEAN ||
            floor_mode == SGP_MES_FLOOR_VALUE,
            "floor_mode = %d is not SGP_MES_FLOOR_NONE / _MEAN / _VALUE", floor_mode);
  SGP_CHECK(ctx, floor_mode != SGP_MES_FLOOR_VALUE || !std::isnan(floor_value),
            "the floor is NaN");
  SGP_CHECK(ctx, value && gidx && floor_used, "value, gidx and floor_used are required");
  SGP_CHECK(ctx, g->post_valid,
            "the grid holds no current posterior: run a confidence pass (sgp_grid_confidence "
            "/ sgp_grid_posterior) first");
  bool comm = false;
  if (merge) SGP_TRY(comm_or_single(ctx, &comm));
  const int world = comm ? ctx->world : 0;
  const int64_t N = g->N;
  const int nwg = int(mes_blocks(N));
  const int nf = int(std::min<int64_t>((N + 255) / 256, kMesFloorWg));
  double *in, *part;
  SGP_TRY(sgp_scratch(ctx, kSlotMesIn, (kMesHead + (alpha ? size_t(N) : 0)) * 8, &in));
  SGP_TRY(sgp_scratch(ctx, kSlotMesPart, mes_scratch_bytes(nwg, nf, world), &part));
  const MesScratch ms = mes_scratch(part, nwg, nf);
  SGP_TRY(sgp_h2d(ctx, in, ystar, size_t(K) * 8));
  if (floor_mode == SGP_MES_FLOOR_MEAN) {
    hipLaunchKernelGGL(k_mes_floor, dim3(unsigned(nf)), dim3(256), 0, ctx->stream, g->mean,
                       rows == SGP_MES_ALL ? nullptr : g->S, N, ms.fpart);
    SGP_HIP(ctx, hipGetLastError());
    SGP_TRY(launch_reduce_max(ctx, ms.fpart, nf, ms.floor));
    if (comm) SGP_TRY(coll_allreduce_max_f64(ctx, ms.floor, 1));
  } else {
    hipLaunchKernelGGL(k_mes_set, dim3(1), dim3(64), 0, ctx->stream, ms.floor,
                       floor_mode == SGP_MES_FLOOR_VALUE ? floor_value : -INFINITY);
    SGP_HIP(ctx, hipGetLastError());
  }
  MesArgs a{};
  a.mean = g->mean;
  a.var = g->var;
  a.N = N;
  a.ystar = in;
  a.K = K;
  a.floor = ms.floor;
  a.mask1 = rows == SGP_MES_ALL ? nullptr : rows == SGP_MES_S ? g->S : g->M;
  a.mask2 = rows == SGP_MES_MG ? g->Gm : nullptr;
  a.alpha = alpha ? in + kMesHead : nullptr;
  a.pval = ms.pval;
  a.pidx = ms.pidx;
  SweepTimer tm;
  // (the events time the row kernel for scripts/bench_mes.py; no flops are booked: the
  // context's counter is the posterior sweep's algorithmic count, and a term's operations
  // are library calls whose count depends on the toolchain)
  SGP_TRY(tm.begin(ctx, 0.0));
  hipLaunchKernelGGL(k_mes_grid, dim3(unsigned(nwg)), dim3(kMesThreads), 0, ctx->stream, a);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(tm.end(ctx));
  hipLaunchKernelGGL(k_mes_final, dim3(1), dim3(256), 0, ctx->stream, ms.pval, ms.pidx, nwg,
                     g->goff, comm ? ms.own : ms.out);
  SGP_HIP(ctx, hipGetLastError());
  if (comm) {
    SGP_TRY(coll_allgather(ctx, ms.own, ms.recs, 16));
    hipLaunchKernelGGL(k_mes_merge, dim3(1), dim3(64), 0, ctx->stream, ms.recs, world, ms.out);
    SGP_HIP(ctx, hipGetLastError());
  }
  // one read-back of the result: out[2] and the floor behind it
  double h[3];
  SGP_TRY(sgp_d2h(ctx, h, ms.out, sizeof(h)));
  *value = h[0];
  memcpy(gidx, &h[1], 8);
  *floor_used = h[2];
  if (alpha) SGP_TRY(sgp_d2h(ctx, alpha, a.alpha, size_t(N) * 8));
  return 0;
}

}  // namespace

int sgp_mes_eval(sgp_ctx* ctx, const double* mean, const double* var, int64_t N,
                 const double* ystar, int K, double floor, double* out) {
  SGP_TRY(mes_checks(ctx, ystar, K));
  SGP_CHECK(ctx, !std::isnan(floor), "the floor is NaN");
  if (N <= 0) return 0;
  const int64_t step = std::min(N, kMesEvalRows);
  double* in;
  SGP_TRY(sgp_scratch(ctx, kSlotMesIn, (kMesHead + 3 * size_t(step)) * 8, &in));
  double head[SGP_MAX_MES + 1] = {0.0};
  memcpy(head, ystar, size_t(K) * 8);
  head[SGP_MAX_MES] = floor;
  SGP_TRY(sgp_h2d(ctx, in, head, sizeof(head)));
  double *m = in + kMesHead, *v = m + step, *o = v + step;
  for (int64_t r0 = 0; r0 < N; r0 += step) {
    const int64_t rows = std::min(step, N - r0);
    SGP_TRY(sgp_h2d(ctx, m, mean + r0, size_t(rows) * 8));
    SGP_TRY(sgp_h2d(ctx, v, var + r0, size_t(rows) * 8));
    hipLaunchKernelGGL(k_mes_rows, dim3(mes_blocks(rows)), dim3(kMesThreads), 0, ctx->stream, m,
                       v, rows, in, K, in + SGP_MAX_MES, o);
    SGP_HIP(ctx, hipGetLastError());
    SGP_TRY(sgp_d2h(ctx, out + r0, o, size_t(rows) * 8));
  }
  return 0;
}

int sgp_grid_mes(sgp_grid* g, const double* ystar, int K, int rows, int floor_mode,
                 double floor_value, double* alpha, double* value, int64_t* gidx,
                 double* floor_used) {
  return grid_mes(g, ystar, K, rows, floor_mode, floor_value, alpha, value, gidx, floor_used,
                  false);
}

int sgp_grid_mes_comm(sgp_grid* g, const double* ystar, int K, int rows, int floor_mode,
                      double floor_value, double* alpha, double* value, int64_t* gidx,
                      double* floor_used) {
  return grid_mes(g, ystar, K, rows, floor_mode, floor_value, alpha, value, gidx, floor_used,
                  true);
}
