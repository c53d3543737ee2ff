// The rank-1 expander test on the device (safeopt/gp_opt.py:577-606): does the observation of a
// candidate x_c at its upper bound lift an unsafe row above fmin?  With k_c = k(X, x_c),
// t = L^-1 k_c, w = Ky^-1 k_c and s2 = prior - |t|^2 the updated posterior at a row x is a
// closed form in c(x) = k(x, x_c) - k(X, x)^T w: n covariances and n FMAs per (row, candidate)
// instead of a refit, and an exact pre-filter that needs ONE covariance decides most rows.
// This file, top to bottom:
//   * the scan kernels: k_expander (up to 16 candidates per launch), k_expander_filter /
//     k_expander_list (one candidate: pre-filter, then the listed rows), k_expander_many
//     (thousands of candidates in groups of 16, ManyRows / many_*: DESIGN.md section 4.2);
//   * the operand kernels (k_expk, k_expt_mm, k_expw_mm; k_expkt, k_expw1 for one candidate)
//     and expander_operands_all;
//   * k_pass_aux / agg / sagg and the launchers launch_expander_many, launch_expander_check;
//   * k_rank1 and launch_rank1, the refresh of the resident posterior after an append or a
//     removal: the same closed form, applied to every row.  It stays in this translation
//     unit because two of its instances (d = 2) compile to another instruction stream
//     in a file of their own, with or without sweep.hip's flags
//     (profiles/expander_split/SUMMARY.txt).
// The scratch blocks the kernels read and write are laid out in expander_layout.h; the entry
// points are in expander_api.hip.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "expander_layout.h"
#include "sets_front.h"
#include "sweep_shared.h"

namespace {

// ---- expander check ---------------------------------------------------------
// One MFMA row block = up to 16 candidates: acc[cand, pt] = sum_j w_c[j] K[j,pt].
// The 16 rows of a wave are row0 + (lane & 15); lane >> 4 selects the candidate
// quad.  `unsafe` marks the lanes whose row takes part.
template <int D>
__device__ __forceinline__ void expander_rows(const GpDev* gps, int G,
                                              const SweepPoints& pts,
                                              const ExpanderArgs& ea,
                                              int64_t rrow, bool unsafe,
                                              const double* tab, int lane) {
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k)
    x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];

  for (int g = 0; g < G; ++g) {
    if (!ea.active[g]) continue;
    const GpDev& gp = gps[g];
    const KernFast<D> kf(gp.kern);
    const double mu = ea.mean[int64_t(g) * pts.N + rrow];
    const double var = ea.var[int64_t(g) * pts.N + rrow];
    const double kdiag = gp.kern.kdiag;

    // Exact pre-filter.  |c(x)| <= k(x,x_c) + |L^-1 k_x| |L^-1 k_c| with
    // |L^-1 k_x|^2 = k(x,x) - var(x), so an upper bound of the updated lower
    // confidence bound costs ONE covariance evaluation per (row, candidate)
    // instead of n.  Rows far from x_c and from the data (most of the unsafe
    // set) cannot reach fmin and skip the n-term contraction below.
    double kxc[4];
    bool possible = false;
    const double qx = fmax(kdiag - var, 0.0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cand = (lane >> 4) + 4 * r;
      kxc[r] = 0.0;
      if (cand < ea.m && unsafe) {
        kxc[r] = kf.raw(x, ea.xc + cand * D, tab);
        // (the smaller of the two bounds on the posterior covariance: k_expander_many)
        const double tn2c = ea.tn2[g * 16 + cand];
        const double cmax =
            fmin(fabs(kxc[r]) + sqrt(qx * tn2c),
                 sqrt((var + 1e-12 * kdiag) * (fmax(kdiag - tn2c, 0.0) + 1e-12 * kdiag))) *
            (1.0 + 1e-9);
        const double mu2 = mu + fabs(ea.delta[g * 16 + cand]) * cmax;
        const double var2 =
            fmax(var - cmax * cmax * ea.inv_s2[g * 16 + cand], 1e-15);
        const double l2max = mu2 - ea.beta * sqrt(var2);
        possible = possible ||
                   ((l2max + 1e-9 * (fabs(mu2) + 1.0) >= ea.fmin[g]) &&
                    (kxc[r] >= ea.near_frac * kdiag));
      }
    }
    if (__ballot(possible) == 0ull) continue;  // wave-uniform

    gptr_t W = (gptr_t)ea.Wpack + int64_t(g) * ea.wstride + lane;
    gptr_t Xj = (gptr_t)gp.Xs + (lane >> 4) * D;
    double xs[D];
    kf.prep(x, xs);
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    const int nsteps = gp.n_pad >> 2;  // multiple of 4 (n_pad is 16-aligned)
    // operands of 16 training points per iteration, fetched one iteration ahead
    // (the loop is otherwise a chain of exposed global-memory latencies)
    double a[4], xr[4][D], an[4], xn[4][D];
    auto fetch = [&](int s0, double (&ao)[4], double (&xo)[4][D]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ao[q] = W[(s0 + q) * 64];
#pragma unroll
        for (int k = 0; k < D; ++k) xo[q][k] = Xj[(s0 + q) * 4 * D + k];
      }
    };
    fetch(0, a, xr);
#pragma unroll 1
    for (int s0 = 0; s0 < nsteps; s0 += 4) {
      if (s0 + 4 < nsteps) fetch(s0 + 4, an, xn);
      double kv[4];
      kf.template many<4>(xs, &xr[0][0], D, tab, kv);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], kv[q], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = an[q];
#pragma unroll
        for (int k = 0; k < D; ++k) xr[q][k] = xn[q][k];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // f64 16x16x4 C/D layout: col = lane & 15, row = (lane >> 4) + 4 r
      const int cand = (lane >> 4) + 4 * r;
      bool hit = false;
      if (cand < ea.m && unsafe) {
        const double cx = kxc[r] - acc[r];
        const double mu2 = mu + cx * ea.delta[g * 16 + cand];
        const double var2 =
            fmax(var - cx * cx * ea.inv_s2[g * 16 + cand], 1e-15);
        const double l2 = mu2 - ea.beta * sqrt(var2);
        hit = l2 >= ea.fmin[g];
      }
      const unsigned long long b = __ballot(hit);
      if (lane == 0 && b != 0ull) {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
          if ((b >> (16 * grp)) & 0xffffull)
            atomicOr(&ea.flags[(grp + 4 * r) * G + g], 1);
        }
      }
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_expander(const GpDev* gps, int G,
                                                  SweepPoints pts,
                                                  ExpanderArgs ea) {
  __shared__ double tab[kExpTabSize];
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t row = int64_t(blockIdx.x) * 64 + wave * 16 + (lane & 15);
  const bool valid = row < pts.N;
  const int64_t rrow = valid ? row : pts.N - 1;
  const bool unsafe = valid && (ea.S[rrow] == 0);
  // skip waves with no unsafe row (wave-uniform)
  if (__ballot(unsafe) == 0ull) return;
  expander_rows<D>(gps, G, pts, ea, rrow, unsafe, tab, lane);
}

// Many candidates in ONE pass over the unsafe rows (sgp_grid_expander_pass; the expander
// loop of gp_opt.py:557-612 where it has to visit hundreds or thousands of candidates): the
// candidates come in groups of 16 -- the operand blocks of k_expander, laid out
// [group][GP][...] -- and a wave keeps its 16 rows, their posterior and the GP's kernel while
// it walks the groups: pre-filter (one covariance per row and candidate), and only where a
// row could be lifted above fmin the n-term contraction on the matrix cores.  Same tests,
// same arithmetic per (row, candidate) as k_expander.
//
// Three launches.  The rows that pass the pre-filter for ANY candidate are few and they sit
// together (the band next to the safe set whose lower bound is just below fmin: 500 of 750000
// unsafe rows in the converged state of bench.py, in 290 of 47000 waves) -- and such a row
// passes it for nearly EVERY candidate, so a scan that tested and contracted in place left the
// pair tests and the matrix products of a whole pass to a few hundred waves, one block after
// the other (all but 0.1 ms of a pass).  So
//   MODE 0, the scan of the grid, only looks for the waves with a block that passes the BLOCK
//           test (one group per lane, out at the first one) -> a list of waves per GP
//           (ea.wlist, ea.wcount);
//   MODE 2  takes the listed waves and the groups kManyTestChunk at a time -- an item per wave
//           of the launch, as many as the chip has -- and finds the ROWS that pass the block
//           test of the row alone for some group (kernels of several parts, which have no
//           block test: the pair test for some candidate) -> a list of rows per GP (ea.list,
//           ea.count; a row once: ea.wmask);
//   MODE 1  takes the listed rows 16 at a time and the groups kManyChunk at a time -- an item
//           per wave; with few items 4 at a time, an item per workgroup, its four waves a
//           quarter of the training points each -- and runs the same tests and the contraction
//           of what is left of them.
constexpr int kManyKbRow = 80;     // doubles between the k-rows of a wave's transpose buffer
constexpr int kManyChunk = 8;      // groups of an item of MODE 1
constexpr int kManyTestChunk = 32; //                   of MODE 2
constexpr int kManyListBlocks = 1024;   // workgroups of MODE 1 / 2 (4 items at a time each)
constexpr int kManyCoopItems = 1024;    // MODE 1: up to that many items of 4 groups go one per workgroup
#ifdef EXPM_STATS
__device__ unsigned long long g_expm_stats[32];
extern "C" void sgp_debug_expm_stats(unsigned long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_expm_stats), sizeof(g_expm_stats));
  if (reset) { unsigned long long z[32] = {}; hipMemcpyToSymbol(HIP_SYMBOL(g_expm_stats), z, sizeof(z)); }
}
#define EXPM_STAT(i, v) do { const unsigned long long v_ = (unsigned long long)(v); \
    if (lane == 0) atomicAdd(&g_expm_stats[i], v_); } while (0)
#else
#define EXPM_STAT(i, v) do {} while (0)
#endif

// A wave's 16 rows (lane & 15) of one GP, what the tests need of them, and the tests.  SINGLE:
// a kernel of one part (resolved per GP at the top of the launch: the code of a pass is tens
// of KB and a wave at a time per SIMD runs it -- the paths it does not take stay out of the
// instruction cache, and the loops below are rolled where four independent chains are enough).
template <int D, bool SINGLE>
struct ManyRows {
  KernFast<D> kf;
  double x[D], xlo[D], xhi[D];
  double mu, var, sqx, svx, mu_hi, var_lo, sqx_hi, svx_hi, beta2, fmin;
  bool unsafe;
  int g, G, m_total;

  __device__ __forceinline__ ManyRows(const GpDev& gp, int g_, int G_, const ExpanderArgs& ea,
                                      const double (&x_)[D], double mu_, double var_, bool unsafe_)
      : kf(gp.kern), mu(mu_), var(var_), unsafe(unsafe_), g(g_), G(G_), m_total(ea.m) {
    const double kdiag = gp.kern.kdiag;
    // bounding box of the wave's unsafe rows (consecutive rows of the grid: a short segment)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      x[k] = x_[k];
      xlo[k] = -wave_max(unsafe ? -x[k] : -INFINITY);
      xhi[k] = wave_max(unsafe ? x[k] : -INFINITY);
    }
    // ... and the extremes of their posterior: with the group's extremes (k_pass_agg) an upper
    // bound of what ANY pair of the block can reach
    mu_hi = wave_max(unsafe ? mu : -INFINITY);
    const double var_hi = wave_max(unsafe ? var : -INFINITY);
    var_lo = -wave_max(unsafe ? -var : -INFINITY);
    sqx_hi = sqrt(fmax(kdiag - var_lo, 0.0));
    svx_hi = sqrt(var_hi + 1e-12 * kdiag);
    // |L^-1 k_x| and the posterior standard deviation of the row (+ room for the rounding
    // of a variance that is a difference of O(k(x,x)) terms)
    sqx = sqrt(fmax(kdiag - var, 0.0));
    svx = sqrt(var + 1e-12 * kdiag);
    beta2 = ea.beta * ea.beta;
    fmin = ea.fmin[g];
  }
  static __device__ __forceinline__ double fmin2(double a, double b) { return ::fmin(a, b); }

  // mu + |delta| c - beta sqrt(var - c^2 / s2) + slack >= fmin for the largest |c| allowed
  __device__ __forceinline__ bool reach(double cmax, double mu_, double var_, double dl, double is2) const {
    const double mu2 = fma(dl, cmax, mu_);
    const double var2 = fmax(var_ - cmax * cmax * is2, 1e-15);
    const double room = mu2 + 1e-9 * (fabs(mu2) + 1.0) - fmin;
    return room >= 0.0 && room * room * (1.0 + 1e-9) >= beta2 * var2;
  }

  // The BLOCK test, one group per lane: the covariance of the closest points of the wave's
  // box and the group's box with the extremes of both sides bounds what any of the block's 256
  // pairs can reach -- most blocks are far apart and end here, for a fraction of an
  // instruction per pair (single-part kernels).
  __device__ __forceinline__ bool block(const ExpanderArgs& ea, int zz, const double* tab) const {
    return block_at(ea.box, ea.agg, zz, tab);
  }
  // (boxes / extremes: of the groups, or of the supergroups of 8 groups)
  __device__ __forceinline__ bool block_at(const double* boxes, const double* aggs, int zz,
                                           const double* tab) const {
    if (!SINGLE) return true;
    const double* bx = boxes + int64_t(zz) * 2 * D;
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double gap = fmax(fmax(bx[k] - xhi[k], xlo[k] - bx[D + k]), 0.0) * kf.sc[k];
      r2 = fma(gap, gap, r2);
    }
    const double kmax = kf.of_r2s(r2, tab);
    const double* ag = aggs + (int64_t(zz) * G + g) * 4;
    const double cmax = fmin2(fma(sqx_hi, ag[2], kmax), svx_hi * ag[3]) * (1.0 + 1e-9);
    return reach(cmax, mu_hi, var_lo, ag[0], ag[1]);
  }

  // The same bound for the lane's OWN row against group zz (its box, its extremes): what the
  // pair tests of the row with the group's 16 candidates -- neighbours along a grid line -- can
  // reach, for one covariance evaluation instead of 16.
  __device__ __forceinline__ bool row_block(const ExpanderArgs& ea, int zz, const double* tab) const {
    const double* bx = ea.box + int64_t(zz) * 2 * D;
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double gap = fmax(fmax(bx[k] - x[k], x[k] - bx[D + k]), 0.0) * kf.sc[k];
      r2 = fma(gap, gap, r2);
    }
    const double kmax = kf.of_r2s(r2, tab);
    const double* ag = ea.agg + (int64_t(zz) * G + g) * 4;
    const double cmax = fmin2(fma(sqx, ag[2], kmax), svx * ag[3]) * (1.0 + 1e-9);
    return unsafe && reach(cmax, mu, var, ag[0], ag[1]);
  }

  // The PAIR tests of four groups, the lane's row against the candidates (lane >> 4) + 4 r of
  // each: an upper bound of the updated lower bound from ONE covariance evaluation per (row,
  // candidate).  c(x) is the POSTERIOR covariance of the two:
  //   |c| <= |k(x, x_c)| + |L^-1 k_x| |L^-1 k_c|        (k_expander's bound: small far
  //                                                      from the data and the candidate)
  //   |c| <= sd(x) sd(x_c)                               (Cauchy-Schwarz on the posterior:
  //                                                      small NEXT to the data)
  // -- with the second one the rows an observation has pinned below fmin drop out for every
  // candidate.  Squares instead of square roots (|L^-1 k_c|, sd(x_c): k_pass_aux).  The four
  // groups' loads and evaluations overlap (no branch around them); p[b]: a pair of group b passes.
  __device__ __forceinline__ void pair4(const ExpanderArgs& ea, const int (&z)[4], int lane,
                                        const double* tab, bool (&p)[4]) const {
#pragma unroll
    for (int b4 = 0; b4 < 4; ++b4) p[b4] = false;
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
      const int cand = (lane >> 4) + 4 * r;
#pragma unroll
      for (int b4 = 0; b4 < 4; ++b4) {
        const int m = min(16, m_total - 16 * z[b4]);
        const int cc = min(cand, m - 1);
        const int64_t zo = (int64_t(z[b4]) * G + g) * 16 + cc;
        const double kxc = kf.template raw_t<SINGLE>(x, ea.xc + (int64_t(z[b4]) * 16 + cc) * D, tab);
        const double cmax = fmin2(fma(sqx, ea.stn[zo], fabs(kxc)), svx * ea.svc[zo]) * (1.0 + 1e-9);
        p[b4] = p[b4] || (cand < m && unsafe && reach(cmax, mu, var, fabs(ea.delta[zo]), ea.inv_s2[zo]));
      }
    }
  }
};

// The groups of `mask` (bit j: group zlo + j) whose pair test passes for some pair, four groups
// at a time; rows: the 16-bit mask of the wave's rows with such a pair.
template <int D, bool SINGLE>
__device__ __forceinline__ unsigned long long many_pairs(const ManyRows<D, SINGLE>& rw,
                                                         const ExpanderArgs& ea, int zlo,
                                                         unsigned long long mask, const double* tab,
                                                         int lane, unsigned& rows) {
  unsigned long long todo = 0ull;
#pragma unroll 1
  while (mask != 0ull) {
    int jb[4], zb[4];
    jb[0] = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
    mask &= mask - 1ull;
#pragma unroll
    for (int b4 = 1; b4 < 4; ++b4) {
      jb[b4] = mask != 0ull ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask)) : jb[0];
      mask &= mask - (mask != 0ull ? 1ull : 0ull);
    }
#pragma unroll
    for (int b4 = 0; b4 < 4; ++b4) zb[b4] = zlo + jb[b4];
    bool p[4];
    rw.pair4(ea, zb, lane, tab, p);
#pragma unroll
    for (int b4 = 0; b4 < 4; ++b4) {
      const unsigned long long pb = __ballot(p[b4]);
      if (pb != 0ull) {                                        // wave-uniform
        todo |= 1ull << jb[b4];
        rows |= unsigned((pb | (pb >> 16) | (pb >> 32) | (pb >> 48)) & 0xffffull);
      }
    }
  }
  return todo;
}

// MODE 1: the wave's 16 listed rows against the groups [zlo, zhi), tests and contraction.
template <int D, bool SINGLE>
__device__ __forceinline__ void many_rows(const GpDev& gp, const ManyRows<D, SINGLE>& rw,
                                          const ExpanderArgs& ea, int zlo, int zhi, const double* tab,
                                          double* kbw, double* rowbuf, double* red, int lane,
                                          int wave, bool coop) {
  const KernFast<D>& kf = rw.kf;
  const int g = rw.g, G = rw.G;
  const int m_total = ea.m;
  double xs[D];
  kf.template prep_t<SINGLE>(rw.x, xs);
  const int nsteps = gp.n_pad >> 2;
  gptr_t Xj = (gptr_t)gp.Xs + (lane >> 4) * D;
  // the wave's rows for the final test of a block: [row][x | mean | var | unsafe]
  __builtin_amdgcn_wave_barrier();
  if (lane < 16) {
    double* rb = rowbuf + lane * (D + 3);
#pragma unroll
    for (int k = 0; k < D; ++k) rb[k] = rw.x[k];
    rb[D] = rw.mu;
    rb[D + 1] = rw.var;
    rb[D + 2] = rw.unsafe ? 1.0 : 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  // (16 rows x 16 candidates) blocks that passed the tests go kQ at a time: ONE evaluation of
  // the rows' covariances with the training points feeds the matrix products of all kQ blocks
  // (the evaluation, ~25 fp64 instructions per value, costs three times the four matrix
  // instructions it feeds)
  constexpr int kQ = 4;
  unsigned zpack = 0u;            // the queue: group zlo + byte q of zpack (an item has <= 64 groups)
  int nq = 0;
  auto zq = [&](int q) { return zlo + int((zpack >> (8 * q)) & 0xffu); };
  // The matrix products run on v_mfma_f64_4x4x4_4b_f64 -- the fp64 instruction that reaches
  // the chip's peak; the 16 x 16 x 4 form stops at two thirds of it --: per k-step four
  // instructions whose B operands are the rows' covariances with row quad m broadcast to
  // all four quads (the LDS transpose of the sweeps, broadcast_quads), A = the packed
  // Ky^-1 k_c as it is (lane 16 k + candidate).  D[blk][i][j] -> lane 16 i + 4 blk + j: a lane
  // ends with ONE candidate, 4 blk + i, at the four rows 4 m + j -- whose x, mean and
  // variance it reads from the wave's row buffer.
  // `coop` (few items in the launch: the pass waits for the longest of them): the four waves of
  // the workgroup hold the SAME rows and queue (same tests on the same data), each takes a
  // quarter of the training points, the partial products meet in LDS and wave j finishes block
  // j -- an item is a chain of n / 64 evaluations, not n / 16.  Otherwise a wave has its own
  // item and all training points.
  auto flush = [&]() {
    double acc[kQ][4];
#pragma unroll
    for (int j = 0; j < kQ; ++j)
#pragma unroll
      for (int m4 = 0; m4 < 4; ++m4) acc[j][m4] = 0.0;
    const int nit = nsteps >> 2;                       // (n_pad is a multiple of 16)
    const int sbeg = coop ? 4 * ((nit * wave) >> 2) : 0;
    const int send = coop ? 4 * ((nit * (wave + 1)) >> 2) : nsteps;
    double xr[4][D], xn[4][D];
    auto fetch = [&](int s0, double (&xo)[4][D]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < D; ++k) xo[q][k] = Xj[(s0 + q) * 4 * D + k];
    };
    if (sbeg < send) fetch(sbeg, xr);
#pragma unroll 1
    for (int s0 = sbeg; s0 < send; s0 += 4) {
      if (s0 + 4 < send) fetch(s0 + 4, xn);
      // the A operands of all queued blocks are requested in front of the evaluation: their
      // latency (L2) passes under it and under the other wave of the SIMD (no second set of
      // them a step ahead: its 32 registers are the second wave)
      double a[kQ][4];
#pragma unroll
      for (int j = 0; j < kQ; ++j) {
        if (j < nq) {                     // (wave-uniform)
          gptr_t W = (gptr_t)ea.Wpack + (int64_t(zq(j)) * G + g) * ea.wstride + lane;
#pragma unroll
          for (int q = 0; q < 4; ++q) a[j][q] = W[(s0 + q) * 64];
        }
      }
      double kv[4];
      kf.template manyn_t<4, SINGLE>(xs, &xr[0][0], D, tab, kv);
      double kb[4][4];
      broadcast_quads<kManyKbRow>(kv, kbw, lane, kb);
#pragma unroll
      for (int j = 0; j < kQ; ++j) {
        if (j < nq) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m4 = 0; m4 < 4; ++m4)
              acc[j][m4] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[j][q], kb[m4][q], acc[j][m4], 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < D; ++k) xr[q][k] = xn[q][k];
    }
#pragma unroll
    for (int j = 0; j < kQ; ++j)
#pragma unroll
      for (int m4 = 0; m4 < 4; ++m4) red[((wave * kQ + j) * 4 + m4) * 64 + lane] = acc[j][m4];
    if (coop) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    // the final test of the blocks (coop: block j belongs to wave j), the products from LDS
    const int cand = 4 * ((lane >> 2) & 3) + (lane >> 4);
    const int jlo = coop ? wave : 0, jhi = coop ? min(wave + 1, nq) : nq;
#pragma unroll 1
    for (int j = jlo; j < jhi; ++j) {
      const int z = zq(j);
      const int m = min(16, m_total - 16 * z);
      const int64_t zo = (int64_t(z) * G + g) * 16;
      const double* xc = ea.xc + int64_t(z) * 16 * D;
      bool hit = false;
      if (cand < m) {
        const double dl = ea.delta[zo + cand], is2 = ea.inv_s2[zo + cand];
#pragma unroll
        for (int m4 = 0; m4 < 4; ++m4) {
          const double* rb = rowbuf + (4 * m4 + (lane & 3)) * (D + 3);
          if (rb[D + 2] != 0.0) {                       // an unsafe row of the grid
            double dot = red[(((coop ? 0 : wave) * kQ + j) * 4 + m4) * 64 + lane];
            if (coop) {                                 // (in the order of the training points)
#pragma unroll
              for (int w = 1; w < 4; ++w) dot += red[((w * kQ + j) * 4 + m4) * 64 + lane];
            }
            const double cx = kf.template raw_t<SINGLE>(rb, xc + cand * D, tab) - dot;
            const double mu2 = rb[D] + cx * dl;
            const double var2 = fmax(rb[D + 1] - cx * cx * is2, 1e-15);
            hit = hit || (mu2 - ea.beta * sqrt(var2) >= ea.fmin[g]);
          }
        }
      }
      if (hit) atomicOr(&ea.flags[(int64_t(z) * 16 + cand) * G + g], 1);
    }
    if (coop) __syncthreads();
    nq = 0;
  };
  // The item's groups (at most 64): the block test one group per lane, a finer test for the
  // groups that are left, then the blocks that pass it, four per evaluation.
  static_assert(kManyChunk <= 64, "one block test per item");
  EXPM_STAT(8, 1);
  const unsigned long long mask = __ballot(zlo + lane < zhi && rw.block(ea, zlo + lane, tab));
  unsigned long long todo = 0ull;
  if (SINGLE && gp.n_pad <= 256) {
    // ... which for a kernel of one part and a small factor is the block test of the ROW
    // against the group, four groups at a time (lane = 16 group + row): one covariance
    // evaluation per (row, group) instead of 16 -- the candidates of a group are neighbours
    // along a grid line, their box and extremes bound nearly what the pairs themselves do.
    // (From n = 257 on a block that the pair test would have dropped costs more than the test:
    // full_sets at n = 637 5.3 ms against 3.6.)
#pragma unroll 1
    for (int z4 = zlo; z4 < zhi; z4 += 4) {
      const int zz = z4 + (lane >> 4);
      const bool p = zz < zhi && ((mask >> (zz - zlo)) & 1ull) != 0ull && rw.row_block(ea, zz, tab);
      const unsigned long long pb = __ballot(p);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((pb >> (16 * q)) & 0xffffull) todo |= 1ull << (z4 + q - zlo);     // wave-uniform
    }
  } else {
    unsigned rows = 0u;
    todo = many_pairs<D, SINGLE>(rw, ea, zlo, mask, tab, lane, rows);
  }
#pragma unroll 1
  while (todo != 0ull) {
    zpack = 0u;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      if (todo != 0ull) {
        zpack |= unsigned(__builtin_amdgcn_readfirstlane(__builtin_ctzll(todo))) << (8 * q);
        todo &= todo - 1ull;
        nq = q + 1;
        EXPM_STAT(9, 1);
      }
    }
    flush();
  }
}

// One GP of a launch (see k_expander_many).
template <int D, int MODE, bool SINGLE>
__device__ __forceinline__ void many_gp(const GpDev* gps, int g, int G, const SweepPoints& pts,
                                        const ExpanderArgs& ea, int ngroups, const double* tab,
                                        double* kbw, double* rowbuf, double* red, int lane, int wave) {
  const int64_t nwaves = (pts.N + 15) >> 4;        // 16-row segments of the shard
  auto rows_of = [&](int64_t rrow, bool unsafe) {
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
      x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];
    return ManyRows<D, SINGLE>(gps[g], g, G, ea, x, ea.mean[int64_t(g) * pts.N + rrow],
                               ea.var[int64_t(g) * pts.N + rrow], unsafe);
  };
  if (MODE == 0) {
    const int64_t wid = int64_t(blockIdx.x) * 4 + wave;
    const int64_t row = wid * 16 + (lane & 15);
    const bool valid = row < pts.N;
    const int64_t rrow = valid ? row : pts.N - 1;
    const bool unsafe = valid && (ea.S[rrow] == 0);
    if (__ballot(unsafe) == 0ull) return;          // (wave-uniform)
    const ManyRows<D, SINGLE> rw = rows_of(rrow, unsafe);
    // (the block test alone, 64 groups at a time: no wave of the scan waits for a chain of
    // pair tests -- the waves next to the band pass the block test for most groups and the
    // pair test for none)
    // Two levels: the SUPERGROUPS of 8 consecutive groups first, one per lane (a far segment is
    // done after one test per 64 x 128 candidates), then the groups of the supergroups that
    // pass, eight supergroups at a time (lane = 8 supergroup + group).
    bool some = false;
    EXPM_STAT(0, 1); EXPM_STAT(1, __popcll(__ballot(unsafe) & 0xffffull));
    const int nsuper = (ngroups + 7) >> 3;
#pragma unroll 1
    for (int Z0 = 0; Z0 < nsuper && !some; Z0 += 64) {
      const int ZZ = Z0 + lane;
      unsigned long long sm = __ballot(ZZ < nsuper && rw.block_at(ea.sbox, ea.sagg, ZZ, tab));
      EXPM_STAT(2, min(64, nsuper - Z0));
#pragma unroll 1
      while (sm != 0ull && !some) {
        int mine = -1;
#pragma unroll
        for (int sidx = 0; sidx < 8; ++sidx) {
          const int bpos = sm != 0ull ? __builtin_amdgcn_readfirstlane(__builtin_ctzll(sm)) : -1;
          if ((lane >> 3) == sidx) mine = bpos;
          sm &= sm - (sm != 0ull ? 1ull : 0ull);
        }
        const int zz = 8 * (Z0 + mine) + (lane & 7);
        some = __ballot(mine >= 0 && zz < ngroups && rw.block(ea, zz, tab)) != 0ull;
        EXPM_STAT(4, 1);
      }
    }
    EXPM_STAT(3, some);
    if (some && lane == 0) {
      const int at = atomicAdd(&ea.wcount[g], 1);
      ea.wlist[int64_t(g) * nwaves + at] = int(wid);
      ea.wmask[int64_t(g) * nwaves + at] = 0u;
    }
  } else if (MODE == 2) {
    const int nch = (ngroups + kManyTestChunk - 1) / kManyTestChunk;
    const int64_t total = int64_t(ea.wcount[g]) * nch;
#pragma unroll 1
    for (int64_t item = int64_t(blockIdx.x) * 4 + wave; item < total; item += int64_t(gridDim.x) * 4) {
      const int hw = int(item / nch), gc = int(item - int64_t(hw) * nch);
      const int64_t row = int64_t(ea.wlist[int64_t(g) * nwaves + hw]) * 16 + (lane & 15);
      const bool valid = row < pts.N;
      const int64_t rrow = valid ? row : pts.N - 1;
      const bool unsafe = valid && (ea.S[rrow] == 0);
      const ManyRows<D, SINGLE> rw = rows_of(rrow, unsafe);
      const int zlo = gc * kManyTestChunk, zhi = min(ngroups, (gc + 1) * kManyTestChunk);
      unsigned hot = 0u;
      if (SINGLE) {
        // row against group, four groups at a time (lane = 16 group + row): no pair tests here
        bool some = false;
#pragma unroll 4
        for (int zz = zlo + (lane >> 4); zz < zhi; zz += 4) some = rw.row_block(ea, zz, tab) || some;
        const unsigned long long pb = __ballot(some);
        hot = unsigned((pb | (pb >> 16) | (pb >> 32) | (pb >> 48)) & 0xffffull);
      } else {
        static_assert(kManyTestChunk <= 64, "one mask per item");
        many_pairs<D, SINGLE>(rw, ea, zlo, (zhi - zlo >= 64) ? ~0ull : ((1ull << (zhi - zlo)) - 1ull),
                              tab, lane, hot);
      }
      EXPM_STAT(16, 1); EXPM_STAT(17, __popc(hot));
      if (hot != 0u) {                           // (wave-uniform) the rows no other item listed
        int base = 0;
        if (lane == 0) {
          hot &= ~atomicOr(&ea.wmask[int64_t(g) * nwaves + hw], hot);
          if (hot != 0u) base = atomicAdd(&ea.count[g], __popc(hot));
        }
        hot = __builtin_amdgcn_readfirstlane(hot);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane < 16 && ((hot >> lane) & 1u))
          ea.list[int64_t(g) * pts.N + base + __popc(hot & ((1u << lane) - 1u))] = int(rrow);
      }
    }
  } else {
    // an item = 16 listed rows x a chunk of groups.  Few items (one round of the chip's
    // workgroups at 4 groups each): an item per WORKGROUP, its waves split the training points
    // (many_rows, coop); otherwise an item of kManyChunk groups per wave.
    const int cnt = ea.count[g];
    const int nrb = (cnt + 15) >> 4;
    const bool coop = int64_t(nrb) * ((ngroups + 3) >> 2) <= kManyCoopItems;
    const int chunk = coop ? 4 : kManyChunk;
    const int nch = (ngroups + chunk - 1) / chunk;
    const int64_t total = int64_t(nrb) * nch;
    // (coop: the item and the trip count are uniform over the workgroup -- barriers inside)
    // Items in chunk-major order, and a contiguous range of them per XCD (workgroup b runs on
    // XCD b % 8, each with its own L2): the waves in flight at a time then contract the SAME
    // few chunks against different rows -- the groups' A operands (n x 16 doubles each, 10 MB
    // a pass of 6000 candidates at n = 217) are fetched into an L2 once instead of once per
    // 16 rows.
    const int per = coop ? 1 : 4;                                  // items of a workgroup at a time
    const int64_t share = (total + 7) >> 3;                        // of an XCD
    const int64_t xend = min(total, share * ((blockIdx.x & 7) + 1));
    const int64_t step = int64_t(gridDim.x >> 3) * per;
#pragma unroll 1
    for (int64_t item = share * (blockIdx.x & 7) + int64_t(blockIdx.x >> 3) * per + (coop ? 0 : wave);
         item < xend; item += step) {
      const int gc = int(item / nrb), rb = int(item - int64_t(gc) * nrb);
      const int idx = rb * 16 + (lane & 15);
      const bool unsafe = idx < cnt;
      const int64_t rrow = ea.list[int64_t(g) * pts.N + (unsafe ? idx : cnt - 1)];
      const ManyRows<D, SINGLE> rw = rows_of(rrow, unsafe);
      many_rows<D, SINGLE>(gps[g], rw, ea, gc * chunk, min(ngroups, (gc + 1) * chunk), tab,
                           kbw, rowbuf, red, lane, wave, coop);
    }
  }
}

template <int D, int MODE>
__global__ __launch_bounds__(256) void k_expander_many(const GpDev* gps, int G,
                                                       SweepPoints pts, ExpanderArgs ea,
                                                       int ngroups) {
  __shared__ double tab[kExpTabSize];
  __shared__ __attribute__((aligned(16))) double kbuf[MODE == 1 ? 4 : 1][4 * kManyKbRow];   // B-operand transposes
  __shared__ double rows_sh[MODE == 1 ? 4 : 1][16 * (D + 3)];
  __shared__ double red[MODE == 1 ? 4 * 4 * 4 * 64 : 1];     // [wave][block][m4][lane] partial products
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  double* kbw = kbuf[MODE == 1 ? wave : 0];
  double* rowbuf = rows_sh[MODE == 1 ? wave : 0];
  for (int g = 0; g < G; ++g) {
    if (!ea.active[g]) continue;
    if (__builtin_amdgcn_readfirstlane(int(gps[g].kern.n_parts == 1)))
      many_gp<D, MODE, true>(gps, g, G, pts, ea, ngroups, tab, kbw, rowbuf, red, lane, wave);
    else
      many_gp<D, MODE, false>(gps, g, G, pts, ea, ngroups, tab, kbw, rowbuf, red, lane, wave);
  }
}

// Single candidate (the probe of the first candidate and its exact re-scan):
// the pre-filter runs with one row per lane over the whole shard and appends
// the rows that could be lifted above fmin to a list (a few per cent of the
// unsafe set); k_expander_list then computes c(x) = k(x,x_c) - w . k(X,x) for
// those rows only, one row per lane and the training rows / w through LDS --
// with a single candidate the contraction is a dot product, not a matrix
// product.  Same pre-filter and the same update formulas as k_expander.
template <int D>
__global__ __launch_bounds__(256) void k_expander_filter(const GpDev* gps, int G,
                                                         SweepPoints pts,
                                                         ExpanderArgs ea,
                                                         int* count, int* list) {
  __shared__ double tab[kExpTabSize];
  exp_tab_init(tab);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const bool valid = row < pts.N;
  const int64_t rrow = valid ? row : pts.N - 1;
  // (the row is fetched together with its S flag, not after it)
  const uint8_t sflag = ea.S[rrow];
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k)
    x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];
  const bool unsafe = valid && (sflag == 0);
  if (__ballot(unsafe) == 0ull) return;
  bool possible = false;
  if (unsafe) {
    for (int g = 0; g < G; ++g) {
      if (!ea.active[g]) continue;
      const GpDev& gp = gps[g];
      const KernFast<D> kf(gp.kern);
      const double mu = ea.mean[int64_t(g) * pts.N + rrow];
      const double var = ea.var[int64_t(g) * pts.N + rrow];
      const double kdiag = gp.kern.kdiag;
      const double qx = fmax(kdiag - var, 0.0);
      const double kxc = kf.raw(x, ea.xc, tab);
      // |c(x)| <= |k(x, x_c)| + |L^-1 k_x| |L^-1 k_c| and, Cauchy-Schwarz on the POSTERIOR
      // covariance, |c(x)| <= sd(x) sd(x_c): the second bound drops the rows an observation
      // has pinned below fmin, which the first one lists for every candidate
      const double tn2c = ea.tn2[g * 16];
      const double cmax =
          fmin(fabs(kxc) + sqrt(qx * tn2c),
               sqrt((var + 1e-12 * kdiag) * (fmax(kdiag - tn2c, 0.0) + 1e-12 * kdiag))) *
          (1.0 + 1e-9);
      const double mu2 = mu + fabs(ea.delta[g * 16]) * cmax;
      const double var2 = fmax(var - cmax * cmax * ea.inv_s2[g * 16], 1e-15);
      const double l2max = mu2 - ea.beta * sqrt(var2);
      possible = possible ||
                 ((l2max + 1e-9 * (fabs(mu2) + 1.0) >= ea.fmin[g]) &&
                  (kxc >= ea.near_frac * kdiag));
    }
  }
  const unsigned long long b = __ballot(possible);
  if (b == 0ull) return;
  int at = 0;
  if (lane == 0) at = atomicAdd(count, __popcll(b));
  at = __builtin_amdgcn_readfirstlane(at);
  if (possible) list[at + __popcll(b & ((1ull << lane) - 1ull))] = int(row);
}

constexpr int kExpLds = 6144;     // doubles of staged training data, at most (48 KB)

template <int D>
__global__ __launch_bounds__(256) void k_expander_list(const GpDev* gps, int G,
                                                       SweepPoints pts,
                                                       ExpanderArgs ea,
                                                       const int* count,
                                                       const int* list,
                                                       int stage_cap) {
  __shared__ double tab[kExpTabSize];
  extern __shared__ double stage[];      // [n_pad][D] scaled rows | [n_pad] w
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63;
  const int nrows = *count;
  // 16 rows per wave (lane & 15); the four 16-lane groups split the training
  // points (j = 4 s + (lane >> 4)) and fold their partial dot products at the end
  const int first = (blockIdx.x * 4 + (tid >> 6)) * 16, stride = gridDim.x * 64;
  for (int g = 0; g < G; ++g) {
    if (!ea.active[g]) continue;
    const GpDev& gp = gps[g];
    const KernFast<D> kf(gp.kern);
    const int np = gp.n_pad;
    // w_j of the single candidate sits in lane 16 (j & 3) of k-step j >> 2 of
    // the packed operand
    const double* Wp = ea.Wpack + int64_t(g) * ea.wstride;
    const bool staged = np * (D + 1) <= stage_cap;      // block-uniform
    const double* Xj = gp.Xs;
    if (staged) {
      __syncthreads();                                   // previous GP's readers
      for (int e = tid; e < np * D; e += 256) stage[e] = gp.Xs[e];
      for (int j = tid; j < np; j += 256)
        stage[np * D + j] = Wp[(j >> 2) * 64 + (j & 3) * 16];
      __syncthreads();
      Xj = stage;
    }
    const double kdiag = gp.kern.kdiag;
    for (int i0 = first; i0 < nrows; i0 += stride) {
      const bool valid = i0 + (lane & 15) < nrows;
      const int64_t rrow = list[valid ? i0 + (lane & 15) : i0];
      double x[D], xs[D];
#pragma unroll
      for (int k = 0; k < D; ++k)
        x[k] = pts.base[rrow * pts.stride_row + k * pts.stride_col];
      kf.prep(x, xs);
      const double mu = ea.mean[int64_t(g) * pts.N + rrow];
      const double var = ea.var[int64_t(g) * pts.N + rrow];
      double dot = 0.0;
      const int ph = lane >> 4;
#pragma unroll 1
      for (int s0 = 0; s0 < (np >> 2); s0 += 4) {   // 16 training points / step
        double kq[4], wq[4];
        kf.template many<4>(xs, Xj + (s0 * 4 + ph) * D, 4 * D, tab, kq);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          wq[q] = staged ? stage[np * D + (s0 + q) * 4 + ph]
                         : Wp[(s0 + q) * 64 + ph * 16];
#pragma unroll
        for (int q = 0; q < 4; ++q) dot = fma(wq[q], kq[q], dot);
      }
      dot = sum_lane_groups(dot);
      const double kxc = kf.raw(x, ea.xc, tab);
      bool hit = false;
      if (valid && kxc >= ea.near_frac * kdiag) {
        const double cx = kxc - dot;
        const double mu2 = mu + cx * ea.delta[g * 16];
        const double var2 = fmax(var - cx * cx * ea.inv_s2[g * 16], 1e-15);
        hit = mu2 - ea.beta * sqrt(var2) >= ea.fmin[g];
      }
      if (__ballot(hit) != 0ull && lane == 0) atomicOr(&ea.flags[g], 1);
    }
  }
}

}  // namespace

// ---- operands of the rank-1 expander test, all GPs per launch ----------------------
// For candidate c and GP g:  k_c = k(X, x_c),  t = L^-1 k_c,  w = L^-T t = Ky^-1 k_c
// (packed as an MFMA A operand: cand x j),  s2 = prior - |t|^2,  delta = resid / s2.
namespace {
struct ExpGpSel {
  int active[SGP_MAX_GPS];
};

// 2 .. thousands of candidates (sgp_grid_expander_batch, sgp_grid_expander_pass) in groups of
// 16; every per-candidate array is laid out [group][GP slot][...] (ExpanderOps::Gs slots), the
// group's candidate count is what is left of `m` behind the groups in front.  The two
// triangular products are matrix products of 16-candidate panels on v_mfma_f64_16x16x4_f64:
// per (group, GP) the panels Kc and T are [j][16 candidates] -- 64 consecutive doubles are a
// B operand (k_expt_mm: lane 16 k + c <- [4 s + k][c]) or an A operand (k_expw_mm) as they lie.
constexpr int kOpGroups = 2;       // groups of a wave: one operand of L^-1 feeds that many products

// Kc[group][g][j][c] = k(x_c, X_j); zero for j >= n (the padding meets zeros of L^-1) and c >= m
template <int D>
__global__ __launch_bounds__(256) void k_expk(const GpDev* gps, ExpGpSel sel,
                                              const double* xc, int m, double* Kc,
                                              int64_t ldk, int Gs) {
  const int g = blockIdx.y;
  if (!sel.active[g]) return;
  const int z = blockIdx.z;
  xc += int64_t(z) * kMaxRhs * D;
  m = min(kMaxRhs, m - kMaxRhs * z);
  const GpDev& gp = gps[g];
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= gp.n_pad) return;
  double* out = Kc + ((int64_t(z) * Gs + g) * ldk + j) * kMaxRhs;
  double xj[D];
#pragma unroll
  for (int k = 0; k < D; ++k) xj[k] = gp.Xpad[int64_t(j) * D + k];
  for (int c = 0; c < kMaxRhs; ++c)
    out[c] = (j < gp.n && c < m) ? kern_eval<D>(gp.kern, xc + c * D, xj) : 0.0;
}

// T[group][g][i][c] = sum_{j <= i} Li[i][j] Kc[..][j][c]: a wave per (row block of 16, kOpGroups
// groups); A = the packed L^-1 of the sweeps (GpDev::Apack: zero above the diagonal and in the
// padding), B = the panel.  D: column (candidate) = lane & 15, rows (lane >> 4) + 4 r.
__global__ __launch_bounds__(256) void k_expt_mm(const GpDev* gps, ExpGpSel sel,
                                                 const double* Kc, double* Tt,
                                                 int64_t ldk, int Gs, int ngroups) {
  const int g = blockIdx.y;
  if (!sel.active[g]) return;
  const GpDev& gp = gps[g];
  const int b = blockIdx.x;
  if (b >= gp.nblk) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int z0 = (blockIdx.z * 4 + wave) * kOpGroups;
  if (z0 >= ngroups) return;
  const int nsteps = gp.n_pad >> 2;
  const double* A = gp.Apack + int64_t(b) * nsteps * 64 + lane;
  // narrow packing of the last row block (k_pack): its rows 4..15 repeat rows 0..3
  const bool dup = b == gp.nblk - 1 && gp.narrow && (lane & 15) >= 4;
  const double* B[kOpGroups];
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q)
    B[q] = Kc + (int64_t(min(z0 + q, ngroups - 1)) * Gs + g) * ldk * kMaxRhs + lane;
  double4_t acc[kOpGroups];
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int send = (b + 1) * 4;                 // up to the diagonal block
  constexpr int kInFlight = 4;
#pragma unroll 1
  for (int s = 0; s < send; s += kInFlight) {   // (send is a multiple of 4)
    double av[kInFlight], bv[kOpGroups][kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      av[i] = A[(s + i) * 64];
#pragma unroll
      for (int q = 0; q < kOpGroups; ++q) bv[q][i] = B[q][(s + i) * 64];
    }
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      const double a = dup ? 0.0 : av[i];
#pragma unroll
      for (int q = 0; q < kOpGroups; ++q)
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[q][i], acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q) {
    if (z0 + q < ngroups) {
      double* T = Tt + (int64_t(z0 + q) * Gs + g) * ldk * kMaxRhs;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        T[(16 * b + (lane >> 4) + 4 * r) * kMaxRhs + (lane & 15)] = acc[q][r];
    }
  }
}

// W[c][j] = sum_{i >= j} Li[i][j] T[..][i][c] straight into the packed operand
// (Wpack[(j / 4) * 64 + (j % 4) * 16 + c], zero for j >= n and c >= m): a wave per (column block
// of 16, kOpGroups groups); A = the panel, B = rows of the dense L^-1 (16 consecutive columns).
// D: column j = lane & 15, rows (candidates) (lane >> 4) + 4 r.  The wave of column block 0 walks
// over every row: it also leaves s2 / delta / |t|^2 of its candidates.
__global__ __launch_bounds__(256) void k_expw_mm(const GpDev* gps, ExpGpSel sel,
                                                 const double* Tt, int64_t ldk, ExpanderOps ops,
                                                 int ngroups) {
  const int g = blockIdx.y;
  if (!sel.active[g]) return;
  const GpDev& gp = gps[g];
  const int jb = blockIdx.x;
  if (jb >= gp.nblk) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int z0 = (blockIdx.z * 4 + wave) * kOpGroups;
  if (z0 >= ngroups) return;
  const int n = gp.n;
  const int j = 16 * jb + (lane & 15);
  const double* A[kOpGroups];
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q)
    A[q] = Tt + (int64_t(min(z0 + q, ngroups - 1)) * ops.Gs + g) * ldk * kMaxRhs + lane;
  const double* Bp = gp.Linv + int64_t(lane >> 4) * gp.ld + min(j, n - 1);
  double4_t acc[kOpGroups];
  double ss[kOpGroups];
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q) {
    acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    ss[q] = 0.0;
  }
  const int send = (n + 3) >> 2;
  constexpr int kInFlight = 4;
#pragma unroll 1
  for (int s = 4 * jb; s < send; s += kInFlight) {
    double av[kOpGroups][kInFlight], bv[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      const int row = 4 * (s + i) + (lane >> 4);
      bv[i] = Bp[int64_t(min(4 * (s + i), n - 1 - (lane >> 4))) * gp.ld];
      bv[i] = (row < n && row >= j && j < n) ? bv[i] : 0.0;
      // (rows >= n of the panel are zero: k_expt_mm, the padding of Apack)
#pragma unroll
      for (int q = 0; q < kOpGroups; ++q) av[q][i] = A[q][min(s + i, (gp.n_pad >> 2) - 1) * 64];
    }
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
#pragma unroll
      for (int q = 0; q < kOpGroups; ++q) {
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][i], bv[i], acc[q], 0, 0, 0);
        ss[q] = (s + i < send) ? fma(av[q][i], av[q][i], ss[q]) : ss[q];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kOpGroups; ++q) {
    const int z = z0 + q;
    if (z >= ngroups) break;
    const int m = min(kMaxRhs, ops.m - kMaxRhs * z);
    if (j < gp.n_pad) {
      double* Wp = ops.Wpack + (int64_t(z) * ops.Gs + g) * ops.wstride;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = (lane >> 4) + 4 * r;
        Wp[(j >> 2) * 64 + (j & 3) * 16 + c] = (j < n && c < m) ? acc[q][r] : 0.0;
      }
    }
    if (jb == 0) {
      double t2 = ss[q];
      t2 += __shfl_xor(t2, 16, 64);
      t2 += __shfl_xor(t2, 32, 64);
      const int c = lane;
      if (c < m) {
        const int64_t o = (int64_t(z) * ops.Gs + g) * 16 + c;
        const double s2 = gp.prior - t2;
        ops.inv_s2[o] = 1.0 / s2;
        ops.delta[o] = ops.resid[o] / s2;
        ops.tn2[o] = t2;
      }
    }
  }
}

// One candidate (the fused single-GPU step and the probe of the first candidate):
// T[g][0][i] with k_c evaluated where it is needed -- lane l of the wave that owns
// row i evaluates k(x_c, X_j) for its j = l, l + 64, ... <= i -- instead of a
// separate launch that writes k_c out first.
template <int D>
__global__ __launch_bounds__(256) void k_expkt(const GpDev* gps, ExpGpSel sel,
                                               const double* xc, double* Tt,
                                               int64_t ldk, FrontArgs fa, int g_writer) {
  const int g = blockIdx.y;
  if (!sel.active[g]) return;
  const GpDev& gp = gps[g];
  const int lane = threadIdx.x & 63;
  double x[D];
  if (fa.nb > 0) {
    // one-rank chain: the candidate is not staged yet -- the last step of the front half
    // runs here (sets_front.h); one workgroup leaves the result block and the staged
    // operand for the kernels behind this one
    const int64_t top = front_final_fold(fa, blockIdx.x == 0 && g == g_writer);
#pragma unroll
    for (int k = 0; k < D; ++k)
      x[k] = top >= 0 ? fa.pts[int64_t(k) * fa.N + (top - fa.goff)] : 0.0;
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xc[k];
  }
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= gp.n) return;
  const double* row = gp.Linv + int64_t(i) * gp.ld;
  double acc = 0.0;
  for (int j = lane; j <= i; j += 64) {
    double xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xj[k] = gp.Xpad[int64_t(j) * D + k];
    acc = fma(row[j], kern_eval<D>(gp.kern, x, xj), acc);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) Tt[int64_t(g) * kMaxRhs * ldk + i] = acc;
}

// ... and W[0][j] for it: 64 columns per workgroup, the 16 waves split the rows
// i >= j0 (four loads in flight per lane), one fold through LDS.
__global__ __launch_bounds__(1024) void k_expw1(const GpDev* gps, ExpGpSel sel,
                                                const double* Tt, int64_t ldk,
                                                ExpanderOps ops) {
  __shared__ double sh[16][64];
  const int g = blockIdx.y;
  if (!sel.active[g]) return;
  const GpDev& gp = gps[g];
  const int n = gp.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64, j = j0 + lane;
  if (j0 >= gp.n_pad) return;
  const double* T = Tt + int64_t(g) * kMaxRhs * ldk;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (j < n) {
    const double* col = gp.Linv + j;
    int i = j0 + wave;
    for (; i + 48 < n; i += 64) {
      const double l0 = (i >= j) ? col[int64_t(i) * gp.ld] : 0.0;
      const double l1 = (i + 16 >= j) ? col[int64_t(i + 16) * gp.ld] : 0.0;
      const double l2 = (i + 32 >= j) ? col[int64_t(i + 32) * gp.ld] : 0.0;
      const double l3 = (i + 48 >= j) ? col[int64_t(i + 48) * gp.ld] : 0.0;
      a0 = fma(l0, T[i], a0);
      a1 = fma(l1, T[i + 16], a1);
      a2 = fma(l2, T[i + 32], a2);
      a3 = fma(l3, T[i + 48], a3);
    }
    for (; i < n; i += 16)
      if (i >= j) a0 = fma(col[int64_t(i) * gp.ld], T[i], a0);
  }
  sh[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (wave == 0 && j < gp.n_pad) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += sh[w][lane];
    double* Wp = ops.Wpack + int64_t(g) * ops.wstride + (j >> 2) * 64 + (j & 3) * 16;
    Wp[0] = (j < n) ? tot : 0.0;
#pragma unroll
    for (int c = 1; c < kMaxRhs; ++c) Wp[c] = 0.0;
  }
  if (blockIdx.x == 0 && wave == 1) {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s = fma(T[i], T[i], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      const double s2 = gp.prior - s;
      ops.inv_s2[g * 16] = 1.0 / s2;
      ops.delta[g * 16] = ops.resid[g * 16] / s2;
      ops.tn2[g * 16] = s;
    }
  }
}

}  // namespace

int expander_operands_all(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                          int G, int d, const ExpanderOps& ops, const FrontArgs* fold) {
  int n_max = 0, np_max = 0, g_writer = -1;
  ExpGpSel sel{};
  FrontArgs fa{};
  if (fold) fa = *fold;
  for (int g = 0; g < G; ++g) {
    sel.active[g] = ops.active[g];
    if (!ops.active[g]) continue;
    if (g_writer < 0) g_writer = g;
    n_max = std::max(n_max, gps_host[g].n);
    np_max = std::max(np_max, gps_host[g].n_pad);
  }
  if (n_max == 0) {
    // no GP with a constraint: nothing evaluates the candidate, the fold has no host
    if (fold) return launch_front_final(ctx, *fold);
    return 0;
  }
  SGP_CHECK(ctx, !fold || ops.m == 1, "the front fold goes with one candidate");
  const int64_t ldk = (np_max + 31) / 32 * 32;
  const int ngroups = (ops.m + kMaxRhs - 1) / kMaxRhs;
  SGP_CHECK(ctx, ngroups == 1 || ops.Gs == G, "ExpanderOps::Gs = %d for %d GPs", ops.Gs, G);
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(2) * ngroups * G * kMaxRhs * ldk * sizeof(double),
                      &buf));
  double* Kc = buf;
  double* Tt = buf + size_t(ngroups) * G * kMaxRhs * ldk;
  if (ops.m == 1) {
#define EXPKT_CASE(DD)                                                        \
  case DD:                                                                    \
    hipLaunchKernelGGL(k_expkt<DD>, dim3((n_max + 3) / 4, G), dim3(256), 0,   \
                       ctx->stream, gps_dev, sel, ops.xc, Tt, ldk, fa,        \
                       g_writer);                                             \
    break;
    switch (d) {
      EXPKT_CASE(1) EXPKT_CASE(2) EXPKT_CASE(3) EXPKT_CASE(4)
      EXPKT_CASE(5) EXPKT_CASE(6) EXPKT_CASE(7) EXPKT_CASE(8)
      default:
        sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
        return -2;
    }
#undef EXPKT_CASE
    hipLaunchKernelGGL(k_expw1, dim3((np_max + 63) / 64, G), dim3(1024), 0,
                       ctx->stream, gps_dev, sel, Tt, ldk, ops);
    SGP_HIP(ctx, hipGetLastError());
    return 0;
  }
#define EXPK_CASE(DD)                                                         \
  case DD:                                                                    \
    hipLaunchKernelGGL(k_expk<DD>, dim3((np_max + 255) / 256, G, ngroups), dim3(256), 0,\
                       ctx->stream, gps_dev, sel, ops.xc, ops.m, Kc, ldk, G); \
    break;
  switch (d) {
    EXPK_CASE(1) EXPK_CASE(2) EXPK_CASE(3) EXPK_CASE(4)
    EXPK_CASE(5) EXPK_CASE(6) EXPK_CASE(7) EXPK_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef EXPK_CASE
  const int zblocks = (ngroups + 4 * kOpGroups - 1) / (4 * kOpGroups);
  hipLaunchKernelGGL(k_expt_mm, dim3(np_max / 16, G, zblocks), dim3(256), 0, ctx->stream,
                     gps_dev, sel, Kc, Tt, ldk, G, ngroups);
  hipLaunchKernelGGL(k_expw_mm, dim3(np_max / 16, G, zblocks), dim3(256), 0, ctx->stream,
                     gps_dev, sel, Tt, ldk, ops, ngroups);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}


// |L^-1 k_c| and sd(x_c) of every candidate of a pass, from tn2 = |L^-1 k_c|^2
__global__ void k_pass_aux(const GpDev* gps, int G, const double* tn2, double* stn, double* svc,
                           int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int g = (e >> 4) % G;
  const double t = tn2[e];
  stn[e] = sqrt(fmax(t, 0.0)) * (1.0 + 1e-12);
  svc[e] = sqrt(fmax(gps[g].kern.kdiag - t, 0.0) + 1e-12 * gps[g].kern.kdiag);
}

// Per group of 16 candidates: the largest |delta|, 1 / s2, |L^-1 k_c|, sd(x_c) of every GP
// (agg[(z G + g) 4 ..]) and the bounding box of the candidates' rows (box[z][2][d], raw
// coordinates) -- what lets a wave decide for a whole (16 rows x 16 candidates) block at once.
__global__ void k_pass_agg(int G, int d, int m_total, const double* xc, const double* delta,
                           const double* inv_s2, const double* stn, const double* svc,
                           double* agg, double* box, int ngroups) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ngroups * G) {
    const int z = e / G;
    const int m = min(16, m_total - 16 * z);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int c = 0; c < m; ++c) {
      a0 = fmax(a0, fabs(delta[int64_t(e) * 16 + c]));
      a1 = fmax(a1, inv_s2[int64_t(e) * 16 + c]);
      a2 = fmax(a2, stn[int64_t(e) * 16 + c]);
      a3 = fmax(a3, svc[int64_t(e) * 16 + c]);
    }
    agg[int64_t(e) * 4 + 0] = a0;
    agg[int64_t(e) * 4 + 1] = a1;
    agg[int64_t(e) * 4 + 2] = a2;
    agg[int64_t(e) * 4 + 3] = a3;
  }
  if (e < ngroups * d) {
    const int z = e / d, k = e - z * d;
    const int m = min(16, m_total - 16 * z);
    double lo = INFINITY, hi = -INFINITY;
    for (int c = 0; c < m; ++c) {
      const double v = xc[(int64_t(z) * 16 + c) * d + k];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    box[(int64_t(z) * 2 + 0) * d + k] = lo;
    box[(int64_t(z) * 2 + 1) * d + k] = hi;
  }
}

// ... and the same per SUPERGROUP of 8 consecutive groups, from the groups' values (the scan of
// the grid tests those first: k_expander_many, MODE 0)
__global__ void k_pass_sagg(int G, int d, const double* agg, const double* box, double* sagg,
                            double* sbox, int ngroups) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nsuper = (ngroups + 7) >> 3;
  if (e < nsuper * G) {
    const int Z = e / G, g = e - Z * G;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int z = 8 * Z; z < min(8 * Z + 8, ngroups); ++z)
      for (int q = 0; q < 4; ++q) a[q] = fmax(a[q], agg[(int64_t(z) * G + g) * 4 + q]);
    for (int q = 0; q < 4; ++q) sagg[int64_t(e) * 4 + q] = a[q];
  }
  if (e < nsuper * d) {
    const int Z = e / d, k = e - Z * d;
    double lo = INFINITY, hi = -INFINITY;
    for (int z = 8 * Z; z < min(8 * Z + 8, ngroups); ++z) {
      lo = fmin(lo, box[(int64_t(z) * 2 + 0) * d + k]);
      hi = fmax(hi, box[(int64_t(z) * 2 + 1) * d + k]);
    }
    sbox[(int64_t(Z) * 2 + 0) * d + k] = lo;
    sbox[(int64_t(Z) * 2 + 1) * d + k] = hi;
  }
}

int launch_expander_many(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                         ExpanderArgs ea) {
  if (pts.N <= 0 || ea.m <= 0) return 0;
  const int nblocks = int((pts.N + 63) / 64);
  const int ngroups = (ea.m + 15) / 16;
  // the waves with a possible pair and the rows that pass the pair test for some candidate, per
  // GP (HotLayout)
  {
    const HotLayout hl = hot_layout(pts.N, G);
    char* hot;
    SGP_TRY(sgp_scratch(ctx, kSlotHot, hl.bytes, &hot));
    const HotBufs hb = hot_bufs(hot, hl);
    ea.count = hb.count;
    ea.wcount = hb.wcount;
    ea.wlist = hb.wlist;
    ea.wmask = hb.wmask;
    ea.list = hb.list;
    SGP_HIP(ctx, hipMemsetAsync(hot, 0, kHotHead * sizeof(int), ctx->stream));
  }
  {
    const int n = ngroups * G * 16;
    hipLaunchKernelGGL(k_pass_aux, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, gps_dev, G,
                       ea.tn2, const_cast<double*>(ea.stn), const_cast<double*>(ea.svc), n);
    const int na = ngroups * (G > d ? G : d);
    hipLaunchKernelGGL(k_pass_agg, dim3((na + 255) / 256), dim3(256), 0, ctx->stream, G, d, ea.m,
                       ea.xc, ea.delta, ea.inv_s2, ea.stn, ea.svc, const_cast<double*>(ea.agg),
                       const_cast<double*>(ea.box), ngroups);
    const int ns = ((ngroups + 7) / 8) * (G > d ? G : d);
    hipLaunchKernelGGL(k_pass_sagg, dim3((ns + 255) / 256), dim3(256), 0, ctx->stream, G, d, ea.agg,
                       ea.box, const_cast<double*>(ea.sagg), const_cast<double*>(ea.sbox), ngroups);
  }
#define EXPM_CASE(DD)                                                         \
  case DD:                                                                    \
    hipLaunchKernelGGL((k_expander_many<DD, 0>), dim3(nblocks), dim3(256), 0, \
                       ctx->stream, gps_dev, G, pts, ea, ngroups);            \
    hipLaunchKernelGGL((k_expander_many<DD, 2>), dim3(kManyListBlocks),       \
                       dim3(256), 0, ctx->stream, gps_dev, G, pts, ea,        \
                       ngroups);                                              \
    hipLaunchKernelGGL((k_expander_many<DD, 1>), dim3(kManyListBlocks),       \
                       dim3(256), 0, ctx->stream, gps_dev, G, pts, ea,        \
                       ngroups);                                              \
    break;
  switch (d) {
    EXPM_CASE(1) EXPM_CASE(2) EXPM_CASE(3) EXPM_CASE(4)
    EXPM_CASE(5) EXPM_CASE(6) EXPM_CASE(7) EXPM_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef EXPM_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_expander_check(sgp_ctx* ctx, const GpDev* gps_dev,
                          const GpDev* gps_host, int G, int d, SweepPoints pts,
                          ExpanderArgs ea) {
  if (pts.N <= 0) return 0;
  const int nblocks = int((pts.N + 63) / 64);
  const bool listed = ea.m == 1 && ea.count && ea.list;
  // the listed rows are a few per cent of the shard at most, and the loop over
  // the training points is a chain of LDS latencies: as many waves per CU as the
  // staged training data (LDS) allows
  int np_max = 0;
  for (int g = 0; g < G; ++g)
    if (ea.active[g]) np_max = std::max(np_max, gps_host[g].n_pad);
  int stage_cap = np_max * (d + 1);
  if (stage_cap > kExpLds) stage_cap = 0;              // read from L2 instead
  const int per_cu = std::max(1, std::min(8, int(144 * 1024 / (stage_cap * 8 + 1024))));
  const int nfilter = int((pts.N + 255) / 256), nlist = ctx->num_cu * per_cu;
#define EXP_CASE(DD)                                                          \
  case DD:                                                                    \
    if (listed) {                                                             \
      hipLaunchKernelGGL(k_expander_filter<DD>, dim3(nfilter), dim3(256), 0,  \
                         ctx->stream, gps_dev, G, pts, ea, ea.count, ea.list);\
      hipLaunchKernelGGL(k_expander_list<DD>, dim3(nlist), dim3(256),         \
                         size_t(stage_cap) * 8, ctx->stream, gps_dev, G, pts, \
                         ea, ea.count, ea.list, stage_cap);                   \
    } else {                                                                  \
      hipLaunchKernelGGL(k_expander<DD>, dim3(nblocks), dim3(256), 0,         \
                         ctx->stream, gps_dev, G, pts, ea);                   \
    }                                                                         \
    break;
  switch (d) {
    EXP_CASE(1) EXP_CASE(2) EXP_CASE(3) EXP_CASE(4)
    EXP_CASE(5) EXP_CASE(6) EXP_CASE(7) EXP_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef EXP_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}


namespace {

// ---- rank-1 update of the resident posterior --------------------------------------
// After one appended observation (x*, y*) the posterior at every row changes by
// a closed form (the same algebra as the expander test); per row and updated
// GP this is n covariance evaluations and n FMAs on the VALU -- no n^2 term.
// Lane (r, q) = (lane & 15, lane >> 4) handles row r and training points
// j = q (mod 4); the four partial dot products are folded with two shuffles.
// kRemove: the record is that of a REMOVAL (sgp_gp_remove) -- the row x_i that left, written
// as an append of it to the reduced GP would write it -- and the update runs backwards:
// mean -= c alpha_i, var += c^2 P_ii, with c(x) = k(x, x_i) - k(X_new, x)^T w as before.
constexpr int kRank1Lds = 6144;   // doubles of staged training data (48 KB)

// mean / var of a row after the record {u0, u1} of an append (kKind = kRank1Append), of a
// removal, or of a re-weighting in place (sgp_gp_reweigh: cx = c(x) / P_ii, u0 = P_ii eta, u1 =
// tau P_ii^2 of either sign)
template <int kKind>
__device__ __forceinline__ void rank1_apply(double cx, double u0, double u1, double& mean,
                                            double& var) {
  if (kKind == kRank1Remove) {
    mean = fma(-cx, u0, mean);
    var = fmax(var + cx * cx * u1, 1e-15);
  } else if (kKind == kRank1Reweigh) {
    mean = fma(cx, u0, mean);
    var = fmax(var + cx * cx * u1, 1e-15);
  } else {
    mean = fma(cx, u0, mean);
    var = fmax(var - cx * cx * u1, 1e-15);
  }
}

template <int D, int kKind>
__global__ __launch_bounds__(256) void k_rank1(const GpDev* gps, int G,
                                               SweepPoints pts, Rank1Args ra) {
  __shared__ double tab[kExpTabSize];
  __shared__ double red[4];
  __shared__ double stage[kRank1Lds];   // [n_pad][D] scaled rows | [n_pad] w
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

  bool safe = true;
  double l0 = 0.0;
  // GPs that share the factor of the GP in front of them (GpDev::share: same inputs,
  // kernel, noise and fitting history -- the outputs of a multi-output GP, with their one
  // new observation at the same x*) have the same w and the same k(X, x), hence the same
  // c(x): it is computed for the first of them and kept; only (y* - mu) / s^2 differs.
  bool have_cx = false;
  double cx_keep = 0.0;
  for (int g = 0; g < G; ++g) {
    double mean = ra.mean[int64_t(g) * pts.N + rrow];
    double var = ra.var[int64_t(g) * pts.N + rrow];
    if (ra.which[g] && gps[g].share >= 0 && have_cx) {
      const GpDev& gp = gps[g];
      rank1_apply<kKind>(cx_keep, gp.upd[0], gp.upd[1], mean, var);
      if (writer) {
        ra.mean[int64_t(g) * pts.N + row] = mean;
        ra.var[int64_t(g) * pts.N + row] = var;
      }
    } else if (ra.which[g]) {
      const GpDev& gp = gps[g];
      const KernFast<D> kf(gp.kern);
      double xs[D];
      kf.prep(x, xs);
      // training rows and the update vector: through LDS when they fit (one
      // coalesced pass per workgroup instead of a global round trip per step)
      const int np = gp.n_pad;
      const bool staged = np * (D + 1) <= kRank1Lds;      // block-uniform
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
      const double cx = kf.raw(x, gp.upd + 2, tab) - dot;
      cx_keep = cx;
      have_cx = true;
      rank1_apply<kKind>(cx, gp.upd[0], gp.upd[1], mean, var);
      if (writer) {
        ra.mean[int64_t(g) * pts.N + row] = mean;
        ra.var[int64_t(g) * pts.N + row] = var;
      }
    } else {
      have_cx = false;
    }
    const double sd = sqrt(var);
    const double lo = mean - ra.beta * sd;
    const double up = mean + ra.beta * sd;
    if (g == 0) l0 = lo;
    safe = safe && (lo > ra.fmin[g]);
    if (writer) {
      const double2 q = make_double2(lo, up);
      *reinterpret_cast<double2*>(ra.Q + (row * G + g) * 2) = q;
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

int rank1_num_blocks(int64_t N) { return int((N + 63) / 64); }

int launch_rank1(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d,
                 SweepPoints pts, Rank1Args ra, int kind) {
  if (pts.N <= 0) return 0;
  const int nblocks = rank1_num_blocks(pts.N);
#define R1_CASE(DD)                                                           \
  case DD:                                                                    \
    if (kind == kRank1Remove)                                                 \
      hipLaunchKernelGGL((k_rank1<DD, kRank1Remove>), dim3(nblocks), dim3(256), 0,  \
                         ctx->stream, gps_dev, G, pts, ra);                   \
    else if (kind == kRank1Reweigh)                                           \
      hipLaunchKernelGGL((k_rank1<DD, kRank1Reweigh>), dim3(nblocks), dim3(256), 0, \
                         ctx->stream, gps_dev, G, pts, ra);                   \
    else                                                                      \
      hipLaunchKernelGGL((k_rank1<DD, kRank1Append>), dim3(nblocks), dim3(256), 0,  \
                         ctx->stream, gps_dev, G, pts, ra);                   \
    break;
  switch (d) {
    R1_CASE(1) R1_CASE(2) R1_CASE(3) R1_CASE(4)
    R1_CASE(5) R1_CASE(6) R1_CASE(7) R1_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef R1_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
