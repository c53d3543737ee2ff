// A batch of query points by hallucinated observations (GP-BUCB, Desautels et al. 2014, on
// SafeOpt's selection rule): one launch per pick.  The posterior variance does not depend on
// what is measured, so a pending pick x* is appended to private copies of the GPs
// (sgp_gp_clone, sgp_gp_append) and the record of that append {w = Ky^-1 k(X, x*), 1 / s2, x*}
// downdates a variance buffer of its own,
//   c(x) = k(x, x*) - k(X, x)^T w,   var_h(x) = max(var_h(x) - c(x)^2 / s2, 1e-15),
// next to the resident posterior, which is only read: the means, Q, S, M and G stay those of
// the real data.  The same pass forms the intervals mean -+ beta sqrt(var_h), their value
// under SafeOpt's rule on the rows of the mask that are not picked yet, and the best
// (value, global row) pair of the workgroup; a small kernel reduces the pairs.
//
// The layout is k_rank1's (expander.hip), which does the same per-row work on the resident
// arrays: 64 rows per workgroup, lane (r, q) = (lane & 15, lane >> 4) handles row r and the
// training points j = q (mod 4), two shuffles fold the four partial dot products; n
// covariance evaluations and n FMAs per row and GP on the fp64 VALU, no n^2 term.
#include "common.h"
#include "set_order.h"

namespace {

constexpr int kBatchLds = 6144;   // doubles of staged training data (48 KB), as kRank1Lds

// c(x) of one GP for the row of this lane.  `stage` holds the GP's scaled training rows and
// its update vector when they fit (block-uniform; the caller's barriers frame the reuse).
template <int D>
__device__ __forceinline__ double batch_cx(const GpDev& gp, const double* x, double* stage,
                                           const double* tab) {
  const int tid = threadIdx.x, lane = tid & 63;
  const KernFast<D> kf(gp.kern);
  double xs[D];
  kf.prep(x, xs);
  const int np = gp.n_pad;
  const bool staged = np * (D + 1) <= kBatchLds;      // block-uniform
  const double* Xj = gp.Xs + (lane >> 4) * D;
  const double* w = gp.upd_w + (lane >> 4);
  if (staged) {
    __syncthreads();                                   // previous GP's readers
    for (int e = tid; e < np * D; e += 256) stage[e] = gp.Xs[e];
    for (int e = tid; e < np; e += 256) stage[np * D + e] = gp.upd_w[e];
    __syncthreads();
    Xj = stage + (lane >> 4) * D;
    w = stage + np * D + (lane >> 4);
  }
  double dot = 0.0;
  const int nsteps = np >> 2;
#pragma unroll 1
  for (int s = 0; s < nsteps; s += 4) {   // n_pad is a multiple of 16
    double kq[4];
    kf.template many<4>(xs, Xj + s * 4 * D, 4 * D, tab, kq);
#pragma unroll
    for (int q = 0; q < 4; ++q) dot = fma(w[(s + q) * 4], kq[q], dot);
  }
  dot = sum_lane_groups(dot);
  return kf.raw(x, gp.upd + 2, tab) - dot;
}

template <int D>
__global__ __launch_bounds__(256) void k_batch_pick(const GpDev* gps, int G, SweepPoints pts,
                                                    BatchArgs ba) {
  __shared__ double tab[kExpTabSize];
  __shared__ Pair sh[4];
  __shared__ double stage[kBatchLds];   // [n_pad][D] scaled rows | [n_pad] w
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t row = int64_t(blockIdx.x) * 64 + wave * 16 + (lane & 15);
  const bool valid = row < pts.N;
  const int64_t rrow = valid ? row : pts.N - 1;
  const bool writer = valid && (lane < 16);

  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k)
    x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];

  // GPs that share the factor of the GP in front of them (GpDev::share) had the same point
  // appended: the same w and k(X, x), hence the same c(x) -- computed once, as in k_rank1
  double cx = 0.0;
  double width = -INFINITY, u0 = 0.0;
  for (int g = 0; g < G; ++g) {
    const GpDev& gp = gps[g];
    if (!(g > 0 && gp.share >= 0)) cx = batch_cx<D>(gp, x, stage, tab);
    const double mean = ba.mean[int64_t(g) * pts.N + rrow];
    const double var =
        fmax(ba.var_in[int64_t(g) * pts.N + rrow] - cx * cx * gp.upd[1], 1e-15);
    if (writer) ba.var_out[int64_t(g) * pts.N + row] = var;
    const double sd = sqrt(var);
    const double lo = mean - ba.beta * sd;
    const double up = mean + ba.beta * sd;
    if (g == 0) u0 = up;
    width = fmax(width, (up - lo) / ba.scaling[g]);
  }

  Pair p{-INFINITY, -1};
  if (writer) {
    const bool in_mask =
        ba.mode == SGP_ARGMAX_MG_WIDTH ? (ba.M[row] || ba.Gm[row]) : ba.S[row] != 0;
    if (in_mask) {
      const int64_t gi = ba.goff + row;
      bool taken = false;
      for (int k = 0; k < ba.n_picked; ++k) taken = taken || ba.picked[k] == gi;
      if (!taken) p = Pair{ba.mode == SGP_ARGMAX_MG_WIDTH ? width : u0, gi};
    }
  }
  const Pair win = block_best<true>(p, sh);
  if (tid == 0) {
    ba.part_v[blockIdx.x] = win.v;
    ba.part_i[blockIdx.x] = win.i;
  }
}

__global__ __launch_bounds__(256) void k_batch_final(const double* in_v, const int64_t* in_i,
                                                     int n, double* out_v, int64_t* out_i) {
  __shared__ Pair sh[4];
  Pair best{-INFINITY, -1};
  for (int e = threadIdx.x; e < n; e += 256) {
    const Pair p{in_v[e], in_i[e]};
    if (before_first(p, best)) best = p;
  }
  const Pair win = block_best<true>(best, sh);
  if (threadIdx.x == 0) {
    out_v[0] = win.i >= 0 ? win.v : -INFINITY;
    out_i[0] = win.i;
  }
}

// The record of a rank that takes no part in a pick (`stop`: its bordered append met a
// non-positive pivot) -- {-inf, -1, 1} --, or the stop word 0 behind the pair k_batch_final
// leaves.  rec: value | row | stop, 8 bytes each.
__global__ void k_batch_stop(double* rec, int stop) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t* w = reinterpret_cast<int64_t*>(rec);
  if (stop) {
    rec[0] = -INFINITY;
    w[1] = -1;
  }
  w[2] = stop ? 1 : 0;
}

// The ranks' records of one pick (value | global row | stop, gathered in rank order) merged
// by ONE wave in the order of before_first: the largest value, the lowest global row among
// equal values, a record without a row (-1) never in front of one with a row; out[2] = the
// maximum of the stop words.  No row on any rank: -inf / -1.
__global__ __launch_bounds__(64) void k_batch_merge(const double* recs, int world, double* out) {
  const int lane = threadIdx.x;
  const int64_t* w = reinterpret_cast<const int64_t*>(recs);
  Pair best{-INFINITY, -1};
  int64_t stop = 0;
  for (int r = lane; r < world; r += 64) {
    const Pair p{recs[3 * r], w[3 * r + 1]};
    if (before_first(p, best)) best = p;
    stop = w[3 * r + 2] > stop ? w[3 * r + 2] : stop;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    Pair q;
    q.v = __shfl_xor(best.v, o, 64);
    q.i = __shfl_xor(best.i, o, 64);
    if (before_first(q, best)) best = q;
    const int64_t s = __shfl_xor(stop, o, 64);
    stop = s > stop ? s : stop;
  }
  if (lane == 0) {
    out[0] = best.i >= 0 ? best.v : -INFINITY;
    reinterpret_cast<int64_t*>(out)[1] = best.i;
    reinterpret_cast<int64_t*>(out)[2] = stop;
  }
}

}  // namespace

int batch_num_blocks(int64_t N) { return int((N + 63) / 64); }

int launch_batch_pick(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                      BatchArgs ba, double* res_v, int64_t* res_i) {
  const int nblocks = batch_num_blocks(pts.N);
#define BATCH_CASE(DD)                                                             \
  case DD:                                                                         \
    hipLaunchKernelGGL(k_batch_pick<DD>, dim3(nblocks), dim3(256), 0, ctx->stream, \
                       gps_dev, G, pts, ba);                                       \
    break;
  switch (d) {
    BATCH_CASE(1) BATCH_CASE(2) BATCH_CASE(3) BATCH_CASE(4)
    BATCH_CASE(5) BATCH_CASE(6) BATCH_CASE(7) BATCH_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef BATCH_CASE
  SGP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_batch_final, dim3(1), dim3(256), 0, ctx->stream, ba.part_v, ba.part_i,
                     nblocks, res_v, res_i);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_batch_stop(sgp_ctx* ctx, double* rec, int stop) {
  hipLaunchKernelGGL(k_batch_stop, dim3(1), dim3(64), 0, ctx->stream, rec, stop);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_batch_merge(sgp_ctx* ctx, const double* recs, int world, double* out) {
  hipLaunchKernelGGL(k_batch_merge, dim3(1), dim3(64), 0, ctx->stream, recs, world, out);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
