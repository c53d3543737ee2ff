// The refresh of the resident posterior after a BLOCK append (sgp_gp_append_block, DESIGN.md
// 4.4b): sgp_grid_rankb_update.  The dense L'^-1 after b appended rows is the old L^-1
// bordered by b rows, and for a grid row x, with X' the data after the block,
//   t_j(x) = sum_{i <= n0+j} L'^-1[n0+j][i] k(X'_i, x),   j = 0 .. b-1 in that order,
//   mean(x) += sum_j t_j(x) gamma_j,   var(x) = max(var(x) - sum_j t_j(x)^2, 1e-15),
// gamma_j = (row n0+j of L'^-1) . y' from the GP's block record (RankbArgs::blk).  One pass with
// n + b covariance evaluations per row and GP, where b rank-1 refreshes (k_rank1) take about
// b n; the FMAs are the same.  Then Q, S and the workgroup's max l_0 over safe rows as
// k_rank1's epilogue writes them, for every GP of the launch.
//
// The layout is k_rank1's and k_swarm_down's (swarm_batch.hip): 64 rows per 256-thread
// workgroup, lane (r, q) = (lane & 15, lane >> 4) handles row r and the training points
// i = q (mod 4), SGP_MAX_BLOCK accumulators per lane, X' and the tail block staged through
// LDS in chunks of kBlkChunk training points, the tail block transposed ([point][tail row],
// pitch kBlkPitch: a lane reads its 16 coefficients of a point as eight 16-byte words, the
// four points of a wave in different banks), two shuffles fold the four partial sums.  Every
// covariance is evaluated once per row and GP (kern_eval.h) and never stored.  Sums in a
// fixed order, no atomics: a row's bits depend on its coordinates and the GPs alone -- not
// on N, the row's position or the shard.  fp64 VALU work; no matrix instructions (the fp64
// MFMA shares the pipe at the same peak).
//
// GPs that share the factor of the GP in front of them (GpDev::share) and were flagged with
// the same b have the same tail rows and the same k(X', x), hence the same t_j: they are
// computed for the first of them and kept (k_rank1's have_cx rule); only gamma differs.  An
// unflagged GP in between breaks the chain.
#include "kern_eval.h"

namespace {

constexpr int kBlkAcc = SGP_MAX_BLOCK;   // tail rows = accumulators per lane
constexpr int kBlkChunk = 128;           // training points staged per chunk (a multiple of 16)
constexpr int kBlkPitch = 18;            // doubles between the staged coefficients of two points
static_assert(kBlkAcc == 16 && kBlkPitch >= kBlkAcc && kBlkPitch % 2 == 0,
              "the coefficients of a point are read as eight aligned 16-byte words");

template <int D>
__global__ __launch_bounds__(256) void k_rankb(const GpDev* gps, int G, SweepPoints pts,
                                               RankbArgs rb) {
  const Rank1Args& ra = rb.r;
  __shared__ double tab[kExpTabSize];
  __shared__ double red[4];
  __shared__ double sx[kBlkChunk * D];             // scaled rows of X'
  // tail block, transposed (read as 16-byte words)
  __shared__ __attribute__((aligned(16))) double st[kBlkChunk * kBlkPitch];
  exp_tab_init(tab);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * 64 + wave * 16 + (lane & 15);
  const bool valid = row < pts.N;
  const int64_t rrow = valid ? row : pts.N - 1;
  const bool writer = valid && (lane < 16);

  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];

  bool safe = true;
  double l0 = 0.0;
  double t[kBlkAcc];                               // accumulators, then t_j of the last leader
  int b_keep = 0;                                  // > 0: t[] holds the t_j of the GP in front
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    double mean = ra.mean[int64_t(g) * pts.N + rrow];
    double var = ra.var[int64_t(g) * pts.N + rrow];
    if (ra.which[g]) {
      const GpDev& gp = gps[g];
      const double* blk = rb.blk[g];
      const int b = min(max(int(blk[kBlkB]), 1), kBlkAcc);        // (block-uniform)
      if (!(gp.share >= 0 && b_keep == b)) {
        const KernFast<D> kf(gp.kern);
        double xs[D];
        kf.prep(x, xs);
        const int n = gp.n, n0 = n - b;            // row n0 + j has n0 + j + 1 entries
#pragma unroll
        for (int j = 0; j < kBlkAcc; ++j) t[j] = 0.0;
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += kBlkChunk) {
          const int nc = min(kBlkChunk, (n - c0 + 15) & ~15);   // <= n_pad - c0
          __syncthreads();                         // the table; the previous chunk's readers
          for (int e = tid; e < nc * D; e += 256) {
            const int i = c0 + e / D;
            sx[e] = i < n ? gp.Xs[int64_t(c0) * D + e] : 0.0;
          }
          for (int e = tid; e < nc * kBlkAcc; e += 256) {
            const int il = e / kBlkAcc, j = e - il * kBlkAcc;
            const int i = c0 + il, r = n0 + j;
            st[il * kBlkPitch + j] = (j < b && i <= r) ? gp.Linv[int64_t(r) * gp.ld + i] : 0.0;
          }
          __syncthreads();
#pragma unroll 1
          for (int s = 0; s < nc; s += 16) {       // points s + 4 v + q, v = 0 .. 3
            double kq[4];
            kf.template many<4>(xs, sx + (s + q) * D, 4 * D, tab, kq);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const double2_t* cf =
                  reinterpret_cast<const double2_t*>(st + (s + 4 * v + q) * kBlkPitch);
#pragma unroll
              for (int h = 0; h < kBlkAcc / 2; ++h) {
                const double2_t c = cf[h];
                t[2 * h] = fma(c.x, kq[v], t[2 * h]);
                t[2 * h + 1] = fma(c.y, kq[v], t[2 * h + 1]);
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < kBlkAcc; ++j) t[j] = sum_lane_groups(t[j]);
        b_keep = b;
      }
      // (rows behind b: zero coefficients, t = 0; gamma is zero there as well)
      double dm = 0.0, dn = 0.0;
#pragma unroll
      for (int j = 0; j < kBlkAcc; ++j) {
        dm = fma(t[j], blk[kBlkGamma + j], dm);
        dn = fma(t[j], t[j], dn);
      }
      mean += dm;
      var = fmax(var - dn, 1e-15);
      if (writer) {
        ra.mean[int64_t(g) * pts.N + row] = mean;
        ra.var[int64_t(g) * pts.N + row] = var;
      }
    } else {
      b_keep = 0;
    }
    const double sd = sqrt(var);
    const double lo = mean - ra.beta * sd;
    const double up = mean + ra.beta * sd;
    if (g == 0) l0 = lo;
    safe = safe && (lo > ra.fmin[g]);
    if (writer) {
      const double2 qv = make_double2(lo, up);
      *reinterpret_cast<double2*>(ra.Q + (row * G + g) * 2) = qv;
    }
  }
  if (writer) ra.S[row] = safe ? 1 : 0;
  double v = (writer && safe) ? l0 : -INFINITY;
  v = wave_max(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (tid == 0)
    ra.partial[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

}  // namespace

int launch_rankb(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                 const RankbArgs& ra) {
  if (pts.N <= 0) return 0;
  const int nblocks = rank1_num_blocks(pts.N);
#define RB_CASE(DD)                                                                       \
  case DD:                                                                                \
    hipLaunchKernelGGL(k_rankb<DD>, dim3(nblocks), dim3(256), 0, ctx->stream, gps_dev, G, \
                       pts, ra);                                                          \
    break;
  switch (d) {
    RB_CASE(1) RB_CASE(2) RB_CASE(3) RB_CASE(4)
    RB_CASE(5) RB_CASE(6) RB_CASE(7) RB_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef RB_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
