// The downdate of a hallucinated swarm (sgp_swarm_fitness_hall / sgp_swarm_run_hall,
// DESIGN.md 4.13): GP-BUCB on SafeOptSwarm's rule.  A clone of every GP holds the real data
// plus the b pending picks of the batch (sgp_gp_clone, sgp_gp_append), so its dense L'^-1
// is the real L^-1 bordered by b rows, and for a particle x
//   t_j(x) = (row n0 + j of L'^-1) . k(X', x),   j = 0 .. b-1   (n0 = n - b real rows),
//   down(x) = sum_j t_j(x)^2                      in the order j = 0 .. b-1,
// is what the pending picks take off the real posterior variance: var_h = max(var - down,
// 1e-15) in the shaping pass (fitness.h).  No second posterior is formed: b short dot
// products on top of the real one.
//
// The layout is k_batch_pick's (batch.hip): 64 particles per 256-thread workgroup, lane
// (r, q) = (lane & 15, lane >> 4) handles particle r and the training points i = q (mod 4),
// two shuffles fold the four partial dot products.  The tail rows go in passes of kDownAcc:
// every lane keeps kDownAcc accumulators, X' and the tail block are staged through LDS in
// chunks of kDownChunk training points, the tail block transposed ([point][row of the pass],
// pitch kDownPitch: a lane reads its 16 coefficients of a point as eight 16-byte words, the
// four points of a wave in different banks).  k(X', x) is evaluated on the fly (kern_eval.h)
// and never stored: (n + b) ceil(b / 16) covariances and about b (n + b) FMAs per particle
// and factor on the fp64 VALU.  Sums in a fixed order, no atomics: down of a particle
// depends on its coordinates and the clones alone -- not on P, its row or the launch.
// blockIdx.y is the GP; a clone that shares the factor of a clone in front of it
// (GpDev::share) is skipped and receives its leader's down.
#include "kern_eval.h"

namespace {

constexpr int kDownAcc = 16;      // tail rows of a pass = accumulators per lane
constexpr int kDownChunk = 128;   // training points staged per chunk (a multiple of 16)
constexpr int kDownPitch = 18;    // doubles between the staged coefficients of two points

template <int D>
__global__ __launch_bounds__(256) void k_swarm_down(const GpDev* clones, int G, int b,
                                                    SweepPoints pts, double* down) {
  __shared__ double tab[kExpTabSize];
  __shared__ double sx[kDownChunk * D];            // scaled rows of X'
  // tail block of the pass, transposed (read as 16-byte words)
  __shared__ __attribute__((aligned(16))) double st[kDownChunk * kDownPitch];
  const int g = blockIdx.y;
  const GpDev& gp = clones[g];
  if (gp.share >= 0) return;                       // (block-uniform: its leader writes for it)
  exp_tab_init(tab);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * 64 + wave * 16 + (lane & 15);
  const bool valid = row < pts.N;
  const int64_t rrow = valid ? row : pts.N - 1;

  const KernFast<D> kf(gp.kern);
  double x[D], xs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];
  kf.prep(x, xs);

  const int n = gp.n, n0 = n - b;
  double dn = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < b; j0 += kDownAcc) {
    const int nj = min(kDownAcc, b - j0);
    const int ncol = n0 + j0 + nj;                 // row n0 + j has n0 + j + 1 entries
    double acc[kDownAcc];
#pragma unroll
    for (int jj = 0; jj < kDownAcc; ++jj) acc[jj] = 0.0;
#pragma unroll 1
    for (int c0 = 0; c0 < ncol; c0 += kDownChunk) {
      const int nc = min(kDownChunk, (ncol - c0 + 15) & ~15);   // <= n_pad - c0
      __syncthreads();                             // the table; the previous chunk's readers
      for (int e = tid; e < nc * D; e += 256) {
        const int i = c0 + e / D;
        sx[e] = i < n ? gp.Xs[int64_t(c0) * D + e] : 0.0;
      }
      for (int e = tid; e < nc * kDownAcc; e += 256) {
        const int il = e / kDownAcc, jj = e - il * kDownAcc;
        const int i = c0 + il, r = n0 + j0 + jj;
        st[il * kDownPitch + jj] = (jj < nj && i <= r) ? gp.Linv[int64_t(r) * gp.ld + i] : 0.0;
      }
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nc; s += 16) {           // points s + 4 v + q, v = 0 .. 3
        double kq[4];
        kf.template many<4>(xs, sx + (s + q) * D, 4 * D, tab, kq);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double2_t* cf =
              reinterpret_cast<const double2_t*>(st + (s + 4 * v + q) * kDownPitch);
#pragma unroll
          for (int h = 0; h < kDownAcc / 2; ++h) {
            const double2_t c = cf[h];
            acc[2 * h] = fma(c.x, kq[v], acc[2 * h]);
            acc[2 * h + 1] = fma(c.y, kq[v], acc[2 * h + 1]);
          }
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < kDownAcc; ++jj) {        // (rows behind nj: zero coefficients, t = 0)
      const double t = sum_lane_groups(acc[jj]);
      dn += t * t;
    }
  }
  if (valid && lane < 16) {
    down[int64_t(g) * pts.N + row] = dn;
    for (int f = g + 1; f < G; ++f)
      if (clones[f].share == g) down[int64_t(f) * pts.N + row] = dn;
  }
}

}  // namespace

int launch_swarm_down(sgp_ctx* ctx, const GpDev* clones_dev, int G, int d, int b,
                      SweepPoints pts, double* down) {
  const dim3 grid(unsigned((pts.N + 63) / 64), unsigned(G));
#define DOWN_CASE(DD)                                                                    \
  case DD:                                                                               \
    hipLaunchKernelGGL(k_swarm_down<DD>, grid, dim3(256), 0, ctx->stream, clones_dev, G, \
                       b, pts, down);                                                    \
    break;
  switch (d) {
    DOWN_CASE(1) DOWN_CASE(2) DOWN_CASE(3) DOWN_CASE(4)
    DOWN_CASE(5) DOWN_CASE(6) DOWN_CASE(7) DOWN_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef DOWN_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
