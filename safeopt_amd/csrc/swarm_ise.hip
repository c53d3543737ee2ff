// Information-theoretic safe exploration (ise.hip) with the roles swapped: the fitness term of
// an 'ise' swarm (sgp_swarm_fitness_ise / sgp_swarm_run_ise).  The P moving particles x_p are the
// ROWS, a fixed set of T target points z_t the COLUMNS:
//
//   c_g(x_p, z_t) = k_g(x_p, z_t) - k_g(x_p, X) W_g[:, t],      W_g = Ky^-1 k_g(X, z_t)
//   pair(p, t)    = sum over the active GPs g, in the order of g, of
//                   ise_term(zmean[g][t] - fmin[g], zvar[g][t], var_g(x_p), c_g(x_p, z_t), s_g)
//   alpha[p]      = max_t pair(p, t),   target[p] = the lowest t attaining it
//   values[p]     = alpha[p] + values[p]            (values[p]: the total_pen the shaping left)
//
// W_g is formed once per call by the operand kernels of the grid rule (launch_ise_operands,
// ise.hip), [n_pad][Tp] with Tp = T rounded up to 64, zero in the padding.  var_g(x_p) is the
// posterior variance the fitness call has just formed: both posterior routes end in
// launch_fitness_small with mean[G][P] and var[G][P] at hand, and the kernel is launched there.
//
// The kernel (k_swarm_ise) is k_ise_rows' shape: a workgroup takes tiles of 64 particles, 16 per
// wave.  Lane (r, k) = (lane & 15, lane >> 4) evaluates k_g(x_r, X_{4 s + k}) in the A-operand
// layout of v_mfma_f64_16x16x4_f64 and feeds it to the MFMAs of four 16-target column blocks;
// W_g goes through LDS in stages of 64 training rows.  In the D layout (column = lane & 15, rows
// (lane >> 4) + 4 reg) the lane then evaluates k_g(x, z_t) for its 16 (particle, target) pairs,
// subtracts, applies ise_term and adds it to the pair's sum, GP after GP.  The blocks of 64
// targets are walked INSIDE the workgroup, k(x, X) evaluated again per block (DESIGN.md 4.17
// for the choice), so a particle's maximum is formed in one place: every lane keeps the best
// (pair, t) of its four rows over its columns of the block -- ascending t, a strict > keeps the
// lowest --, the 16 lanes that hold one row's columns are folded by four shuffles, and one lane
// per row carries the result from block to block (a word pair per row in scratch, touched by
// that thread alone); the lower t wins among equals at every level.  No atomics.  Neither k(x, X) nor the covariances
// reach memory (the optional test outputs aside).  A padding column t >= T is excluded BY
// INDEX, whatever its value; a padding training row meets a zero row of W.
//
// A particle's alpha, target and pairs depend on its coordinates, the GPs and the target set
// alone (a row of an MFMA's result is a function of that row of A), a pair's covariance on the
// particle and the target alone (a column is a function of that column of B, and a column of W
// does not depend on T or its position).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ise_term.h"
#include "sweep_shared.h"

namespace {

constexpr int kSwiRows = 64;                  // particles of a tile (16 per wave)
constexpr int kSwiCols = 64;                  // targets of a column block (4 MFMA blocks)
constexpr int kSwiChunk = 64;                 // rows of W per LDS stage = 16 k-steps
constexpr int kSwiPitch = kSwiCols + 16;      // = 16 mod 32 doubles (ise.hip, paths.hip)
constexpr int64_t kSwiMaxOut = int64_t(1) << 24;   // G P T of the test outputs, at most
constexpr int kNoCol = 0x7fffffff;

struct SwiArgs {
  const GpDev* gps;
  int G;
  unsigned active;
  double fmin[SGP_MAX_GPS];
  double s[SGP_MAX_GPS];
  const double* W[SGP_MAX_GPS];
  const double* base;            // the particles (SweepPoints)
  int64_t P, stride_row, stride_col;
  const double* mean;            // [G][P]
  const double* var;
  const double* tg;              // [Tp][D]
  const double* zmean;           // [G][Tp]
  const double* zvar;
  int T, Tp;
  double* values;                // [P]: total_pen in, alpha + total_pen out
  double* alpha;                 // [P] or null
  long long* target;
  double* post;                  // [G][2][P] or null
  double* pairs;                 // [P][T] or null
  double* cov;                   // [G][P][T] or null
  double* bestv;                 // [P] the rows' best pair over the blocks in front (Tp > 64)
  long long* bestt;              // [P] ... and its column
};

template <int D>
__global__ __launch_bounds__(256) void k_swarm_ise(SwiArgs a) {
  __shared__ double tab[kExpTabSize];
  __shared__ double sB[kSwiChunk * kSwiPitch];
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, lc = lane & 15;
  const int Tp = a.Tp;
  const int64_t P = a.P;
  const int64_t ntiles = (P + kSwiRows - 1) / kSwiRows;
  // The column blocks OUTSIDE the workgroup's tiles: the workgroups of a launch (one per CU,
  // each with its share of the tiles) then walk the slabs W_g[:, col0 .. col0 + 64) in step, and
  // a slab is fetched from HBM once and found in L2 by everyone else.  (Tiles outside, every
  // workgroup is on a slab of its own after a while: measured 1.5 x slower at 16 blocks.)
  for (int col0 = 0; col0 < Tp; col0 += kSwiCols)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kSwiRows + wave * 16;
    if (col0 == 0 && a.post && tid < kSwiRows && tile * kSwiRows + tid < P) {
      const int64_t p = tile * kSwiRows + tid;
      for (int g = 0; g < a.G; ++g) {
        a.post[(int64_t(g) * 2) * P + p] = a.mean[int64_t(g) * P + p];
        a.post[(int64_t(g) * 2 + 1) * P + p] = a.var[int64_t(g) * P + p];
      }
    }
    double x[D];
    {
      const int64_t r = row0 + lc < P ? row0 + lc : P - 1;
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = a.base[r * a.stride_row + k * a.stride_col];
    }
    // the best (pair, t) of the lane's rows kq + 4 reg over its columns of this block
    double bv[4];
    int bt[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      bv[reg] = -INFINITY;
      bt[reg] = kNoCol;
    }

    {
      double pair[4][4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) pair[cb][reg] = 0.0;

      for (int g = 0; g < a.G; ++g) {
        if (!((a.active >> g) & 1u)) continue;
        const GpDev& gp = a.gps[g];
        KernFast<D> kf(gp.kern);
        double xs[D];
        kf.prep(x, xs);
        double4_t acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};
        // ---- k_g(x, X) W_g: A[r][j] = k(x_r, X_j); per block of 16 training points the lane
        // holds av[s] = k(x, X_{16 jb + 4 s + kq}), the A operand of k-step 4 jb + s
        const double* Wg = a.W[g];
        const int n_pad = gp.n_pad;
        for (int k0 = 0; k0 < n_pad; k0 += kSwiChunk) {
          const int kc = min(kSwiChunk, n_pad - k0);          // a multiple of 16
          __syncthreads();
          for (int e = tid; e < kc * kSwiCols; e += 256) {
            const int r = e >> 6, c = e & 63;
            sB[r * kSwiPitch + c] = Wg[int64_t(k0 + r) * Tp + col0 + c];
          }
          __syncthreads();
          for (int jb = 0; jb < kc / 16; ++jb) {
            double av[4];
            kf.template many<4>(xs, gp.Xs + int64_t(k0 + 16 * jb + kq) * D, 4 * D, tab, av);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const double* b = sB + (16 * jb + 4 * s + kq) * kSwiPitch + lc;
#pragma unroll
              for (int cb = 0; cb < 4; ++cb)
                acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[16 * cb], acc[cb], 0, 0, 0);
            }
          }
        }
        // ---- D layout: column = lane & 15, rows kq + 4 reg of the wave's 16
        const double fmin = a.fmin[g], sg = a.s[g];
        // (the lane's four targets; a padding column repeats the last one, its results are
        // dropped)
        double cs[4][D], mu[4], vz[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const int col = min(col0 + 16 * cb + lc, a.T - 1);
          double z[D];
#pragma unroll
          for (int k = 0; k < D; ++k) z[k] = a.tg[int64_t(col) * D + k];
          kf.prep(z, cs[cb]);
          mu[cb] = a.zmean[int64_t(g) * Tp + col] - fmin;
          vz[cb] = a.zvar[int64_t(g) * Tp + col];
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t orow = row0 + kq + 4 * reg;
          const int64_t oc = orow < P ? orow : P - 1;
          double xr[D], xrs[D];
#pragma unroll
          for (int k = 0; k < D; ++k) xr[k] = a.base[oc * a.stride_row + k * a.stride_col];
          kf.prep(xr, xrs);
          const double vx = a.var[int64_t(g) * P + oc];
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            const double proj = reg == 0 ? acc[cb].x : reg == 1 ? acc[cb].y
                                                     : reg == 2 ? acc[cb].z : acc[cb].w;
            const double c = kf(xrs, cs[cb], tab) - proj;
            pair[cb][reg] += ise_term(mu[cb], vz[cb], vx, c, sg);
            const int col = col0 + 16 * cb + lc;
            if (a.cov && orow < P && col < a.T)
              a.cov[(int64_t(g) * P + orow) * a.T + col] = c;
          }
        }
      }

#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int col = col0 + 16 * cb + lc;
        if (col >= a.T) continue;              // a padding column never wins: by index
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t orow = row0 + kq + 4 * reg;
          if (a.pairs && orow < P) a.pairs[orow * a.T + col] = pair[cb][reg];
          // (the lane's columns ascend with cb: > keeps the lowest t among equals)
          if (pair[cb][reg] > bv[reg]) {
            bv[reg] = pair[cb][reg];
            bt[reg] = col;
          }
        }
      }
    }

    // fold the 16 lanes that hold one row's columns: the larger pair, the lower t among equals
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) {
        const double v2 = __shfl_xor(bv[reg], o, 64);
        const int t2 = __shfl_xor(bt[reg], o, 64);
        if (v2 > bv[reg] || (v2 == bv[reg] && t2 < bt[reg])) {
          bv[reg] = v2;
          bt[reg] = t2;
        }
      }
      const int64_t orow = row0 + kq + 4 * reg;
      if (lc == 0 && orow < P) {
        // ... then over the column blocks: the row's best so far lies in bestv / bestt, written
        // and read by this thread alone (a workgroup has the same tiles in every block); the
        // blocks ascend, so the earlier one wins among equals
        double v = bv[reg];
        long long t = bt[reg];
        if (col0 > 0 && !(v > a.bestv[orow])) {
          v = a.bestv[orow];
          t = a.bestt[orow];
        }
        if (col0 + kSwiCols < Tp) {
          a.bestv[orow] = v;
          a.bestt[orow] = t;
        } else {
          // (no column qualified -- every pair NaN: -inf and -1)
          const double al = t == kNoCol ? -INFINITY : v;
          if (a.alpha) a.alpha[orow] = al;
          if (a.target) a.target[orow] = t == kNoCol ? -1 : t;
          a.values[orow] = al + a.values[orow];
        }
      }
    }
  }
}

#define SWI_DISPATCH(d, call)                                                      \
  switch (d) {                                                                     \
    case 1: call(1); break;                                                        \
    case 2: call(2); break;                                                        \
    case 3: call(3); break;                                                        \
    case 4: call(4); break;                                                        \
    case 5: call(5); break;                                                        \
    case 6: call(6); break;                                                        \
    case 7: call(7); break;                                                        \
    case 8: call(8); break;                                                        \
    default:                                                                       \
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);         \
      return -2;                                                                   \
  }

// The blocks of an 'ise' swarm call, in doubles.
//   kSlotSwarmIseW:   W_g[n_pad_g][Tp] of every active GP, one after the other | T[n_max][Tp]
//   kSlotSwarmIseIn:  tg[Tp][d] | zmean[G][Tp] | zvar[G][Tp] | bestv[P] | bestt[P] (the kernel's
//                     running best of every row, block to block)
//   kSlotSwarmIseOut: alpha[P] | target[P] | post[G][2][P] | pairs[P][T] | cov[G][P][T], each only
//                     when the fitness call asks for it
struct SwiLayout {
  size_t w[SGP_MAX_GPS], t, w_words;
  size_t tg, zmean, zvar, bestv, bestt, in_words;
  size_t alpha, target, post, pairs, cov, out_words;
};
SwiLayout swi_layout(const GpDev* host, int G, unsigned active, int d, int T, int Tp, int64_t P,
                     const SwarmIseIn& in) {
  SwiLayout l{};
  size_t off = 0, n_max = 0;
  for (int g = 0; g < G; ++g) {
    l.w[g] = off;
    if (!((active >> g) & 1u)) continue;
    off += size_t(host[g].n_pad) * Tp;
    n_max = std::max(n_max, size_t(host[g].n));
  }
  l.t = off;
  l.w_words = off + n_max * Tp;
  l.tg = 0;
  l.zmean = l.tg + size_t(Tp) * d;
  l.zvar = l.zmean + size_t(G) * Tp;
  l.bestv = l.zvar + size_t(G) * Tp;
  l.bestt = l.bestv + size_t(P);
  l.in_words = l.bestt + size_t(P);
  const size_t np = size_t(P);
  l.alpha = 0;
  l.target = l.alpha + (in.alpha ? np : 0);
  l.post = l.target + (in.target ? np : 0);
  l.pairs = l.post + (in.post ? 2 * size_t(G) * np : 0);
  l.cov = l.pairs + (in.pairs ? np * T : 0);
  l.out_words = l.cov + (in.cov ? size_t(G) * np * T : 0);
  return l;
}

unsigned swi_active(int G, const double* fmin) {
  unsigned active = 0;
  for (int q = 0; q < G; ++q)
    if (std::isfinite(fmin[q])) active |= 1u << q;
  return active;
}

}  // namespace

// The checks an 'ise' entry point makes in front of its early return (common.h)
int swarm_ise_checks(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* fmin,
                     const SwarmIseIn& in) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS && gps && gps[0], "no GP");
  const int T = in.T;
  SGP_CHECK(ctx, T >= 1 && T <= SGP_MAX_ISE, "T = %d targets (1 .. SGP_MAX_ISE = %d)", T,
            SGP_MAX_ISE);
  SGP_CHECK(ctx, in.targets && in.zmean && in.zvar, "targets, zmean and zvar are required");
  const int d = std::max(gps[0]->kern.d, 1);          // targets are (T, d) rows
  for (int64_t i = 0; i < int64_t(T) * d; ++i)
    SGP_CHECK(ctx, std::isfinite(in.targets[i]), "target %lld has a coordinate that is not finite",
              (long long)(i / d));
  for (int64_t i = 0; i < int64_t(G) * T; ++i) {
    SGP_CHECK(ctx, std::isfinite(in.zmean[i]), "zmean[%lld][%lld] is not finite",
              (long long)(i / T), (long long)(i % T));
    SGP_CHECK(ctx, std::isfinite(in.zvar[i]) && in.zvar[i] >= 0.0,
              "zvar[%lld][%lld] is not a variance (finite, >= 0)", (long long)(i / T),
              (long long)(i % T));
  }
  SGP_CHECK(ctx, fmin && swi_active(G, fmin) != 0,
            "no GP is active: every fmin is infinite or NaN");
  return 0;
}

int swarm_ise_out_check(sgp_ctx* ctx, int G, int64_t P, const SwarmIseIn& in) {
  SGP_CHECK(ctx, !(in.pairs || in.cov) || int64_t(G) * P * in.T <= kSwiMaxOut,
            "pairs / cov are test outputs: G P T = %lld exceeds 2^24",
            (long long)(int64_t(G) * P * in.T));
  return 0;
}

// Stages targets, their posterior and the operands of every active GP, ONCE per call, behind
// the checks of the fitness / run routine (host: collect_gps' descriptors).
int swarm_ise_stage(sgp_ctx* ctx, sgp_gp* const* gps, const GpDev* host, int G, int d,
                    const double* fmin, const SwarmIseIn& in, int64_t P, SwarmIse* out) {
  SGP_CHECK(ctx, d >= 1 && d <= SGP_MAX_D, "input dimension %d not in 1..%d", d, SGP_MAX_D);
  const int T = in.T, Tp = (T + kSwiCols - 1) / kSwiCols * kSwiCols;
  const unsigned active = swi_active(G, fmin);
  const SwiLayout l = swi_layout(host, G, active, d, T, Tp, P, in);
  double *wbuf, *inb, *outb = nullptr;
  SGP_TRY(sgp_scratch(ctx, kSlotSwarmIseW, l.w_words * 8, &wbuf));
  SGP_TRY(sgp_scratch(ctx, kSlotSwarmIseIn, l.in_words * 8, &inb));
  if (l.out_words) SGP_TRY(sgp_scratch(ctx, kSlotSwarmIseOut, l.out_words * 8, &outb));
  // one upload of tg | zmean | zvar, zero in the padding
  std::vector<double> blk(l.bestv, 0.0);
  memcpy(&blk[l.tg], in.targets, size_t(T) * d * 8);
  for (int q = 0; q < G; ++q) {
    memcpy(&blk[l.zmean + size_t(q) * Tp], in.zmean + size_t(q) * T, size_t(T) * 8);
    memcpy(&blk[l.zvar + size_t(q) * Tp], in.zvar + size_t(q) * T, size_t(T) * 8);
  }
  SGP_TRY(sgp_h2d(ctx, inb, blk.data(), l.bestv * 8));
  SGP_HIP(ctx, hipMemsetAsync(wbuf, 0, l.t * 8, ctx->stream));
  SwarmIse m{};
  for (int q = 0; q < G; ++q) {
    m.s[q] = gps[q]->noise_var + 1e-8;
    m.n_pad[q] = host[q].n_pad;
    if (!((active >> q) & 1u)) continue;
    SGP_TRY(launch_ise_operands(ctx, gps[q], inb + l.tg, T, Tp, wbuf + l.w[q], wbuf + l.t));
    m.W[q] = wbuf + l.w[q];
  }
  m.tg = inb + l.tg;
  m.zmean = inb + l.zmean;
  m.zvar = inb + l.zvar;
  m.bestv = inb + l.bestv;
  m.bestt = reinterpret_cast<long long*>(inb + l.bestt);
  m.T = T;
  m.Tp = Tp;
  m.active = active;
  m.alpha = in.alpha ? outb + l.alpha : nullptr;
  m.target = in.target ? reinterpret_cast<long long*>(outb + l.target) : nullptr;
  m.post = in.post ? outb + l.post : nullptr;
  m.pairs = in.pairs ? outb + l.pairs : nullptr;
  m.cov = in.cov ? outb + l.cov : nullptr;
  // (an inactive GP's block of cov stays zero)
  if (m.cov) SGP_HIP(ctx, hipMemsetAsync(m.cov, 0, size_t(G) * size_t(P) * T * 8, ctx->stream));
  m.d = d;
  *out = m;
  return 0;
}

// The outputs of a fitness call back to the host
int swarm_ise_read(sgp_ctx* ctx, const SwarmIseIn& in, const SwarmIse& m, int G, int64_t P) {
  const size_t np = size_t(P);
  if (in.alpha) SGP_TRY(sgp_d2h(ctx, in.alpha, m.alpha, np * 8));
  if (in.target) SGP_TRY(sgp_d2h(ctx, in.target, m.target, np * 8));
  if (in.post) SGP_TRY(sgp_d2h(ctx, in.post, m.post, 2 * size_t(G) * np * 8));
  if (in.pairs) SGP_TRY(sgp_d2h(ctx, in.pairs, m.pairs, np * m.T * 8));
  if (in.cov) SGP_TRY(sgp_d2h(ctx, in.cov, m.cov, size_t(G) * np * m.T * 8));
  return 0;
}

// values[p] = alpha_p + values[p] for the P particles whose posterior is mean / var [G][P]
// (common.h).  The events time the kernel for scripts/bench_swarm_ise.py; the flops booked are
// the matrix work, 2 P Tp n_pad per active GP.
int launch_swarm_ise(sgp_ctx* ctx, int G, int64_t P, const double* mean, const double* var,
                     const double* fmin, const SwarmIse& m, double* values) {
  if (P <= 0) return 0;
  SwiArgs a{};
  a.gps = m.gps_dev;
  a.G = G;
  a.active = m.active;
  double flops = 0.0;
  for (int q = 0; q < G; ++q) {
    a.fmin[q] = fmin[q];
    a.s[q] = m.s[q];
    a.W[q] = m.W[q];
    if ((m.active >> q) & 1u) flops += 2.0 * double(P) * m.Tp * m.n_pad[q];
  }
  a.base = m.base;
  a.P = P;
  a.stride_row = m.stride_row;
  a.stride_col = m.stride_col;
  a.mean = mean;
  a.var = var;
  a.tg = m.tg;
  a.zmean = m.zmean;
  a.zvar = m.zvar;
  a.T = m.T;
  a.Tp = m.Tp;
  a.values = values;
  a.alpha = m.alpha;
  a.target = m.target;
  a.post = m.post;
  a.pairs = m.pairs;
  a.cov = m.cov;
  a.bestv = m.bestv;
  a.bestt = m.bestt;
  const int64_t ntiles = (P + kSwiRows - 1) / kSwiRows;
  // one workgroup per CU (the instance holds 256 VGPRs), each with its share of the tiles
  const unsigned nwg = unsigned(std::min<int64_t>(ntiles, std::max(ctx->num_cu, 1)));
  const int d = m.d;
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, flops));
#define CALL(DD) \
  hipLaunchKernelGGL(k_swarm_ise<DD>, dim3(nwg), dim3(256), 0, ctx->stream, a)
  SWI_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}
