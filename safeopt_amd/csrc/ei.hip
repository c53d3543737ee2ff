// Expected improvement and probability of improvement over the resident posterior, as
// logarithms (LogEI: Ament et al. 2023), optionally weighed by the probability of feasibility
// of the constraints (EIC: Gelbart et al. 2014, Gardner et al. 2014).  With the objective GP 0,
// an incumbent tau, a margin xi >= 0 and sigma_g = sqrt(max(var_g, 1e-15)):
//
//   z     = (mean_0 - tau - xi) / sigma_0
//   EI:   alpha = ln(max(var_0, 1e-15)) / 2 + ln(phi(z) + z Phi(z))     = ln EI
//   PI:   alpha = ln Phi(z)                                             = ln PI
//   alpha += ln Phi((mean_g - fmin_g) / sigma_g)  for every g with a finite fmin_g, in order
//
// EI itself underflows to 0 on almost every row of a converged run (sigma tiny, the incumbent
// far above the row), and its arg-max is then the lowest row among equals; the logarithm stays
// finite and ordered (ei_term.h).
//
// One thread per row, grid-stride.  The mask byte is read first: a row outside the candidate
// mask costs one byte unless the caller asked for the alpha array.  mean[g][i] / var[g][i] of
// consecutive lanes are consecutive doubles.  A row's alpha is a function of its own (mean_g,
// var_g) and of (fmin, tau, xi, kind) alone -- the same device function in the row kernel
// (sgp_ei_eval), in the grid kernel and in the particle kernel of an 'ei' swarm (k_swarm_ei,
// behind the shaping pass of sgp_swarm_fitness_ei / sgp_swarm_run_ei) -- so it has the same
// bits whatever N, the launch shape, the row's position or the rank.  The arg-max is an epilogue: per-workgroup (value, local row)
// pairs, one small final kernel; the largest value, the lowest row among equals, rows outside
// the mask never.  No atomics.  The incumbent of SGP_EI_TAU_MEAN is reduced on the device and
// read from device memory by the grid kernel: nothing comes back to the host between the two.
// (The arg-max, final, merge and mean-reduction kernels are this file's own copies of mes.hip's.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "sweep_shared.h"
#include "ei_term.h"

namespace {

constexpr int kEiThreads = 256;              // rows of a workgroup per stride of the kernels
constexpr int kEiMaxWg = 8192;               // workgroups of the grid kernel, at most
constexpr int kEiTauWg = 1024;               // workgroups of the incumbent reduction, at most
constexpr int64_t kEiEvalRows = 1 << 18;     // rows per launch of sgp_ei_eval
constexpr long long kNoRow = std::numeric_limits<long long>::max();

// (value, row) pairs: the larger value, the lower row among equals
__device__ __forceinline__ void take_better(double& v, long long& i, double v2, long long i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// sgp_ei_eval: out[r] = alpha of row r of mean / var [G][stride]
__global__ __launch_bounds__(kEiThreads) void k_ei_rows(const double* mean, const double* var,
                                                        int64_t N, int64_t stride, double tau,
                                                        EiTerm p, double* out) {
  for (int64_t row = int64_t(blockIdx.x) * kEiThreads + threadIdx.x; row < N;
       row += int64_t(gridDim.x) * kEiThreads)
    out[row] = ei_alpha(mean + row, var + row, stride, tau, p);
}

struct EiArgs {
  const double* mean;     // [G][N]
  const double* var;
  int64_t N;
  const double* tau;      // one word; -inf: there is no incumbent, hence no pick
  const uint8_t* mask1;   // a candidate row has a byte set in mask1 or mask2; both null: every row
  const uint8_t* mask2;
  double* alpha;          // [N], or null
  double* pval;           // [gridDim.x] best value of the workgroup's rows
  long long* pidx;        //   ... and its LOCAL row (kNoRow: none)
  EiTerm p;
};

__global__ __launch_bounds__(kEiThreads) void k_ei_grid(EiArgs a) {
  __shared__ double rv[kEiThreads / 64];
  __shared__ long long ri[kEiThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double tau = a.tau[0];
  const bool none = tau == -INFINITY;
  const bool all = !a.mask1 && !a.mask2;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int64_t row = int64_t(blockIdx.x) * kEiThreads + tid; row < a.N;
       row += int64_t(gridDim.x) * kEiThreads) {
    const bool cand = !none && (all || (a.mask1 && a.mask1[row]) || (a.mask2 && a.mask2[row]));
    if (!cand && !a.alpha) continue;
    const double al = none ? -INFINITY : ei_alpha(a.mean + row, a.var + row, a.N, tau, a.p);
    if (a.alpha) a.alpha[row] = al;
    if (cand) take_better(v, i, al, row);
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
    for (int w = 1; w < kEiThreads / 64; ++w) take_better(v, i, rv[w], ri[w]);
    a.pval[blockIdx.x] = v;
    a.pidx[blockIdx.x] = i;
  }
}

// One workgroup: the best of the workgroups' pairs -> out[0] = value, out[1] = GLOBAL row
// (as int64; -inf and -1 when no row qualified).
__global__ __launch_bounds__(256) void k_ei_final(const double* pval, const long long* pidx,
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
__global__ __launch_bounds__(64) void k_ei_merge(const double* recs, int world, double* out) {
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
__global__ __launch_bounds__(256) void k_ei_tau(const double* mean, const uint8_t* mask,
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

__global__ void k_ei_set(double* p, double v) {
  if (threadIdx.x == 0) p[0] = v;
}

inline unsigned ei_blocks(int64_t N) {
  return unsigned(std::max<int64_t>(1, std::min<int64_t>((N + kEiThreads - 1) / kEiThreads,
                                                         kEiMaxWg)));
}

// The fitness term of an 'ei' swarm (sgp_swarm_fitness_ei / sgp_swarm_run_ei), behind the
// shaping pass of fitness.h (kSwarmEi): one thread per particle, grid-stride,
//   a = ei_alpha of the particle's posterior, mean / var [G][P] as the shaping pass has just
//       consumed them -- the bits of k_ei_rows on the same (mean_g, var_g);
//   safe mode:  values[p] = a + values[p], values[p] the total_pen the shaping left;
//   free mode:  values[p] = a, safe[p] = 1 -- penalty and safety rule switched off.
// alpha: [P] receives a, or null.  post: [G][2][P] receives mean | var per GP, or null.
__global__ __launch_bounds__(kEiThreads) void k_swarm_ei(const double* mean, const double* var,
                                                         int64_t P, double tau, EiTerm term,
                                                         int free, double* values,
                                                         uint8_t* safe, double* alpha,
                                                         double* post) {
  for (int64_t p = int64_t(blockIdx.x) * kEiThreads + threadIdx.x; p < P;
       p += int64_t(gridDim.x) * kEiThreads) {
    const double a = ei_alpha(mean + p, var + p, P, tau, term);
    if (alpha) alpha[p] = a;
    if (post) {
      for (int g = 0; g < term.G; ++g) {
        post[(2 * g) * P + p] = mean[g * P + p];
        post[(2 * g + 1) * P + p] = var[g * P + p];
      }
    }
    if (free) {
      values[p] = a;
      safe[p] = 1;
    } else {
      values[p] = a + values[p];
    }
  }
}

// The checks the entry points share, and the call's constants as the kernels take them
int ei_term(sgp_ctx* ctx, int G, const double* fmin, int kind, double xi, EiTerm* p) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS, "G = %d GPs (1 .. SGP_MAX_GPS = %d)", G,
            SGP_MAX_GPS);
  SGP_CHECK(ctx, kind == SGP_EI_EI || kind == SGP_EI_PI, "kind = %d is not SGP_EI_EI / SGP_EI_PI",
            kind);
  SGP_CHECK(ctx, std::isfinite(xi) && xi >= 0.0, "xi = %g is negative or not finite", xi);
  p->kind = kind;
  p->G = G;
  p->xi = xi;
  for (int g = 0; g < SGP_MAX_GPS; ++g) {
    p->fmin[g] = fmin && g < G ? fmin[g] : -INFINITY;
    SGP_CHECK(ctx, p->fmin[g] < INFINITY, "fmin[%d] is NaN or +inf", g);   // (NaN < inf is false)
  }
  return 0;
}

// The block of a grid call in kSlotEiPart, nwg workgroups of the grid kernel, nf of the
// incumbent reduction, world ranks (0: no communicator):
//   pval[nwg] | pidx[nwg] | fpart[nf] | own[2] | out[2] | tau | recs[world][2]
// out: the record {value, global row} the call returns, with the incumbent behind it -- ONE
// read-back of three words; the final kernel writes it.  With a communicator the final
// kernel writes own, this rank's record, instead, and the merge of the gathered records out.
struct EiScratch {
  double* pval;
  long long* pidx;
  double *fpart, *own, *out, *tau, *recs;
};
inline size_t ei_scratch_bytes(int nwg, int nf, int world) {
  return (2 * size_t(nwg) + size_t(nf) + 5 + 2 * size_t(world)) * 8;
}
inline EiScratch ei_scratch(double* base, int nwg, int nf) {
  EiScratch s;
  s.pval = base;
  s.pidx = reinterpret_cast<long long*>(base + nwg);
  s.fpart = base + 2 * size_t(nwg);
  s.own = s.fpart + nf;
  s.out = s.own + 2;
  s.tau = s.own + 4;
  s.recs = s.own + 5;
  return s;
}

int grid_ei(sgp_grid* g, int kind, int rows, int tau_mode, double tau_value, double xi,
            const double* fmin, double* alpha, double* value, int64_t* gidx, double* tau_used,
            bool merge) {
  sgp_ctx* ctx = g->ctx;
  EiTerm p;
  SGP_TRY(ei_term(ctx, g->G, fmin, kind, xi, &p));
  SGP_CHECK(ctx, rows == SGP_MES_ALL || rows == SGP_MES_S || rows == SGP_MES_MG,
            "rows = %d is not SGP_MES_ALL / SGP_MES_S / SGP_MES_MG", rows);
  SGP_CHECK(ctx, tau_mode == SGP_EI_TAU_MEAN || tau_mode == SGP_EI_TAU_VALUE,
            "tau_mode = %d is not SGP_EI_TAU_MEAN / SGP_EI_TAU_VALUE", tau_mode);
  SGP_CHECK(ctx, tau_mode != SGP_EI_TAU_VALUE || std::isfinite(tau_value),
            "the incumbent tau = %g is not finite", tau_value);
  SGP_CHECK(ctx, value && gidx && tau_used, "value, gidx and tau_used are required");
  SGP_CHECK(ctx, g->post_valid,
            "the grid holds no current posterior: run a confidence pass (sgp_grid_confidence "
            "/ sgp_grid_posterior) first");
  bool comm = false;
  if (merge) SGP_TRY(comm_or_single(ctx, &comm));
  const int world = comm ? ctx->world : 0;
  const int64_t N = g->N;
  const int nwg = int(ei_blocks(N));
  const int nf = int(std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, kEiTauWg)));
  double *al = nullptr, *part;
  if (alpha) SGP_TRY(sgp_scratch(ctx, kSlotEiIn, std::max<size_t>(size_t(N), 1) * 8, &al));
  SGP_TRY(sgp_scratch(ctx, kSlotEiPart, ei_scratch_bytes(nwg, nf, world), &part));
  const EiScratch es = ei_scratch(part, nwg, nf);
  if (tau_mode == SGP_EI_TAU_MEAN) {
    hipLaunchKernelGGL(k_ei_tau, dim3(unsigned(nf)), dim3(256), 0, ctx->stream, g->mean,
                       rows == SGP_MES_ALL ? nullptr : g->S, N, es.fpart);
    SGP_HIP(ctx, hipGetLastError());
    SGP_TRY(launch_reduce_max(ctx, es.fpart, nf, es.tau));
    if (comm) SGP_TRY(coll_allreduce_max_f64(ctx, es.tau, 1));
  } else {
    hipLaunchKernelGGL(k_ei_set, dim3(1), dim3(64), 0, ctx->stream, es.tau, tau_value);
    SGP_HIP(ctx, hipGetLastError());
  }
  EiArgs a{};
  a.mean = g->mean;
  a.var = g->var;
  a.N = N;
  a.tau = es.tau;
  a.mask1 = rows == SGP_MES_ALL ? nullptr : rows == SGP_MES_S ? g->S : g->M;
  a.mask2 = rows == SGP_MES_MG ? g->Gm : nullptr;
  a.alpha = al;
  a.pval = es.pval;
  a.pidx = es.pidx;
  a.p = p;
  SweepTimer tm;
  // (the events time the row kernel for scripts/bench_ei.py; no flops are booked, as for
  // sgp_grid_mes)
  SGP_TRY(tm.begin(ctx, 0.0));
  hipLaunchKernelGGL(k_ei_grid, dim3(unsigned(nwg)), dim3(kEiThreads), 0, ctx->stream, a);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(tm.end(ctx));
  hipLaunchKernelGGL(k_ei_final, dim3(1), dim3(256), 0, ctx->stream, es.pval, es.pidx, nwg,
                     g->goff, comm ? es.own : es.out);
  SGP_HIP(ctx, hipGetLastError());
  if (comm) {
    SGP_TRY(coll_allgather(ctx, es.own, es.recs, 16));
    hipLaunchKernelGGL(k_ei_merge, dim3(1), dim3(64), 0, ctx->stream, es.recs, world, es.out);
    SGP_HIP(ctx, hipGetLastError());
  }
  // one read-back of the result: out[2] and the incumbent behind it
  double h[3];
  SGP_TRY(sgp_d2h(ctx, h, es.out, sizeof(h)));
  *value = h[0];
  memcpy(gidx, &h[1], 8);
  *tau_used = h[2];
  if (alpha && N > 0) SGP_TRY(sgp_d2h(ctx, alpha, al, size_t(N) * 8));
  return 0;
}

}  // namespace

// The term of an 'ei' swarm over the P particles whose posterior is mean / var [G][P]
// (common.h).  The events time the kernel for scripts/bench_swarm_ei.py, as grid_ei times its
// row kernel; no flops are booked.
int launch_swarm_ei(sgp_ctx* ctx, int G, int64_t P, const double* mean, const double* var,
                    const SwarmEi& m, double* values, uint8_t* safe) {
  if (P <= 0) return 0;
  SGP_CHECK(ctx, m.on && m.term.G == G, "the term of an 'ei' swarm is set for %d GPs, not %d",
            m.term.G, G);
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 0.0));
  hipLaunchKernelGGL(k_swarm_ei, dim3(ei_blocks(P)), dim3(kEiThreads), 0, ctx->stream, mean, var,
                     P, m.tau, m.term, m.free, values, safe, m.alpha, m.post);
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}

int sgp_ei_eval(sgp_ctx* ctx, const double* mean, const double* var, int64_t N, int G,
                const double* fmin, int kind, double tau, double xi, double* out) {
  EiTerm p;
  SGP_TRY(ei_term(ctx, G, fmin, kind, xi, &p));
  SGP_CHECK(ctx, std::isfinite(tau), "the incumbent tau = %g is not finite", tau);
  if (N <= 0) return 0;
  const int64_t step = std::min(N, kEiEvalRows);
  double* in;
  SGP_TRY(sgp_scratch(ctx, kSlotEiIn, (2 * size_t(G) + 1) * size_t(step) * 8, &in));
  double *m = in, *v = m + size_t(G) * step, *o = v + size_t(G) * step;
  for (int64_t r0 = 0; r0 < N; r0 += step) {
    const int64_t rows = std::min(step, N - r0);
    for (int g = 0; g < G; ++g) {
      SGP_TRY(sgp_h2d(ctx, m + g * step, mean + g * N + r0, size_t(rows) * 8));
      SGP_TRY(sgp_h2d(ctx, v + g * step, var + g * N + r0, size_t(rows) * 8));
    }
    hipLaunchKernelGGL(k_ei_rows, dim3(ei_blocks(rows)), dim3(kEiThreads), 0, ctx->stream, m, v,
                       rows, step, tau, p, o);
    SGP_HIP(ctx, hipGetLastError());
    SGP_TRY(sgp_d2h(ctx, out + r0, o, size_t(rows) * 8));
  }
  return 0;
}

int sgp_grid_ei(sgp_grid* g, int kind, int rows, int tau_mode, double tau_value, double xi,
                const double* fmin, double* alpha, double* value, int64_t* gidx,
                double* tau_used) {
  return grid_ei(g, kind, rows, tau_mode, tau_value, xi, fmin, alpha, value, gidx, tau_used,
                 false);
}

int sgp_grid_ei_comm(sgp_grid* g, int kind, int rows, int tau_mode, double tau_value, double xi,
                     const double* fmin, double* alpha, double* value, int64_t* gidx,
                     double* tau_used) {
  return grid_ei(g, kind, rows, tau_mode, tau_value, xi, fmin, alpha, value, gidx, tau_used,
                 true);
}
