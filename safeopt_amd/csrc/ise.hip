// Information-theoretic safe exploration (Bottero, Luis, Vinogradska, Berkenkamp, Peters 2022,
// "Information-theoretic safe exploration with Gaussian processes") over the resident posterior:
// measure the safe row x whose observation tells most about whether some other row z is safe,
//
//   pair(x, z) = sum over the active GPs g, in the order of g, of I_g(x; z)      (ise_term.h)
//   alpha(x)   = max_z pair(x, z),   target(x) = the lowest row z attaining it,
//
// a GP being active when its fmin is finite.  I_g needs, next to the resident mean and variance,
// the posterior covariance of every row z with every candidate x_j,
//
//   c_g(z, x_j) = k_g(z, x_j) - k_g(z, X) W_g[:, j],    W_g = Ky^-1 k_g(X, x_j),
//
// which is the covariance the big expander passes form (expander.hip, k_expander_many); here
// an entropy term and a max / arg-max over z consume it.
//
// Operands (once per call and active GP): k_g(X, x_j) by the covariance-matrix kernel of the
// factorisation, then the two triangular products with the dense L^-1 (k_ise_fwd, k_ise_bwd),
// every sum in a fixed order that depends on n alone.  W_g lies [n_pad][K_pad], the B-operand
// order of the row kernel, zero in the padding.
//
// The row kernel (k_ise_rows) is k_paths' shape: a workgroup takes tiles of 64 rows, 16 per
// wave, and a block of 64 candidates.  Lane (r, k) = (lane & 15, lane >> 4) evaluates
// k_g(z_r, X_{4 s + k}) ONCE, already in the A-operand layout of v_mfma_f64_16x16x4_f64, and
// feeds it to the MFMAs of the four 16-candidate column blocks; W_g goes through LDS in stages
// of 64 training rows.  In the D layout (column = lane & 15, rows (lane >> 4) + 4 reg) the lane
// then evaluates k_g(z, x_j) for its 16 (row, candidate) pairs, subtracts, applies ise_term and
// adds it to the pair's sum -- GP after GP, so the sum is formed in the order of g.  Neither
// k_g(z, X) nor the covariances reach memory (the optional test outputs aside).  Every lane
// keeps the best (pair, row) of its candidates over all tiles of its workgroup; the workgroups'
// partials ([workgroups <= kIseMaxWg][K_pad]: bounded) are folded by k_ise_final, one workgroup
// per candidate, and k_ise_pick takes the best candidate.  The lowest row wins among equals at
// every level.  No atomics.
//
// A candidate's W column, its covariances, its pairs, alpha and target depend on the candidate
// and the rows alone: not on K, not on its position in cand.  (A column of an MFMA's result is
// a function of that column of B.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "expander_layout.h"
#include "ise_term.h"
#include "sweep_shared.h"

namespace {

constexpr int kIseThreads = 256;              // rows of a workgroup of sgp_ise_eval's kernel
constexpr int64_t kIseEvalRows = 1 << 20;     // rows per launch of sgp_ise_eval
constexpr int kIseRows = 64;                  // rows of a tile (16 per wave)
constexpr int kIseCols = 64;                  // candidates of a workgroup (4 column blocks)
constexpr int kIseChunk = 64;                 // rows of W per LDS stage = 16 k-steps
constexpr int kIsePitch = kIseCols + 16;      // = 16 mod 32 doubles (paths.hip)
constexpr int kIseMaxWg = 512;                // row workgroups of a launch (each walks tiles)
constexpr int64_t kIseMaxOut = int64_t(1) << 24;   // G K N_local of the test outputs, at most
constexpr long long kNoRow = std::numeric_limits<long long>::max();

// (value, row) pairs: the larger value, the lower row among equals
__device__ __forceinline__ void take_better(double& v, long long& i, double v2, long long i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// sgp_ise_eval: out[r] = I(mu[r], vz[r], vx[r], c[r]; s)
__global__ __launch_bounds__(kIseThreads) void k_ise_eval(const double* mu, const double* vz,
                                                          const double* vx, const double* c,
                                                          int64_t N, double s, double* out) {
  const int64_t row = int64_t(blockIdx.x) * kIseThreads + threadIdx.x;
  if (row < N) out[row] = ise_term(mu[row], vz[row], vx[row], c[row], s);
}

// The candidates' coordinates and variances: xc[j][k] = pts[k][idx[j]], vx[g][j] = var[g][idx[j]]
__global__ __launch_bounds__(256) void k_ise_gather(const double* pts, const double* var,
                                                    int64_t N, int d, int G, const int64_t* idx,
                                                    int K, int Kp, double* xc, double* vx) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const int64_t r = idx[j];
  for (int k = 0; k < d; ++k) xc[int64_t(j) * d + k] = pts[int64_t(k) * N + r];
  for (int g = 0; g < G; ++g) vx[int64_t(g) * Kp + j] = var[int64_t(g) * N + r];
}

// T[j][c] = sum_{i <= j} Linv[j][i] U[i][c]: one workgroup per row j and block of 64 columns,
// thread (q, s) = (tid >> 6, tid & 63) the terms i = q, q + 4, ... in order, then
// (p0 + p1) + (p2 + p3) -- k_path_fwd's order
__global__ __launch_bounds__(256) void k_ise_fwd(const double* Linv, int64_t ld, int Kp,
                                                 const double* U, double* T) {
  __shared__ double part[4][64];
  const int j = blockIdx.x, s = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t c = int64_t(blockIdx.y) * 64 + s;
  double acc = 0.0;
  for (int i = q; i <= j; i += 4) acc = fma(Linv[int64_t(j) * ld + i], U[int64_t(i) * Kp + c], acc);
  part[q][s] = acc;
  __syncthreads();
  if (q == 0) T[int64_t(j) * Kp + c] = (part[0][s] + part[1][s]) + (part[2][s] + part[3][s]);
}

// W[j][c] = sum_{j <= i < n} Linv[i][j] T[i][c]
__global__ __launch_bounds__(256) void k_ise_bwd(const double* Linv, int64_t ld, int n, int Kp,
                                                 const double* T, double* W) {
  __shared__ double part[4][64];
  const int j = blockIdx.x, s = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t c = int64_t(blockIdx.y) * 64 + s;
  double acc = 0.0;
  for (int i = j + q; i < n; i += 4) acc = fma(Linv[int64_t(i) * ld + j], T[int64_t(i) * Kp + c], acc);
  part[q][s] = acc;
  __syncthreads();
  if (q == 0) W[int64_t(j) * Kp + c] = (part[0][s] + part[1][s]) + (part[2][s] + part[3][s]);
}

struct IseArgs {
  const GpDev* gps;
  int G;
  unsigned active;               // bit g: GP g has a finite fmin
  double fmin[SGP_MAX_GPS];
  double s[SGP_MAX_GPS];         // noise_var + 1e-8
  const double* W[SGP_MAX_GPS];  // [n_pad][Kp], zero padded; null for an inactive GP
  const double* pts;             // SoA [D][N]
  const double* mean;            // [G][N]
  const double* var;
  const uint8_t* skip;           // rows with a byte set are no z (S); null: every row is one
  int64_t N;
  const double* xc;              // [K][D] candidates
  const double* vx;              // [G][Kp] their variances
  int K, Kp;
  double* pairs;                 // [K][N], or null
  double* cov;                   // [G][K][N], or null
  double* pval;                  // [gridDim.x][Kp] best pair of the workgroup's rows
  long long* pidx;               //   ... and its LOCAL row (kNoRow: none)
};

template <int D>
__global__ __launch_bounds__(256) void k_ise_rows(IseArgs a) {
  __shared__ double tab[kExpTabSize];
  __shared__ double sB[kIseChunk * kIsePitch];
  __shared__ double rv[4][kIseCols];
  __shared__ long long ri[4][kIseCols];
  exp_tab_init(tab);
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, lc = lane & 15;
  const int col0 = blockIdx.y * kIseCols;
  const int Kp = a.Kp;
  double bv[4];
  long long bi[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    bv[cb] = -INFINITY;
    bi[cb] = kNoRow;
  }
  const int64_t ntiles = (a.N + kIseRows - 1) / kIseRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kIseRows + wave * 16;
    double x[D];
    {
      const int64_t r = row0 + lc < a.N ? row0 + lc : a.N - 1;
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = a.pts[k * a.N + r];
    }
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
      // ---- k_g(z, X) W_g: A[r][j] = k(z_r, X_j); per block of 16 training points the lane
      // holds av[s] = k(z, X_{16 jb + 4 s + kq}), the A operand of k-step 4 jb + s
      const double* Wg = a.W[g];
      const int n_pad = gp.n_pad;
      for (int k0 = 0; k0 < n_pad; k0 += kIseChunk) {
        const int kc = min(kIseChunk, n_pad - k0);          // a multiple of 16
        __syncthreads();
        for (int e = tid; e < kc * kIseCols; e += 256) {
          const int r = e >> 6, c = e & 63;
          sB[r * kIsePitch + c] = Wg[int64_t(k0 + r) * Kp + col0 + c];
        }
        __syncthreads();
        for (int jb = 0; jb < kc / 16; ++jb) {
          double av[4];
          kf.template many<4>(xs, gp.Xs + int64_t(k0 + 16 * jb + kq) * D, 4 * D, tab, av);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double* b = sB + (16 * jb + 4 * s + kq) * kIsePitch + lc;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
              acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[16 * cb], acc[cb], 0, 0, 0);
          }
        }
      }
      // ---- D layout: column = lane & 15, rows kq + 4 reg of the wave's 16
      const double fmin = a.fmin[g], sg = a.s[g];
      // (the lane's four candidates; a padding column repeats the last one, its results
      // are dropped)
      double cs[4][D], vxc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int col = min(col0 + 16 * cb + lc, a.K - 1);
        double xcand[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xcand[k] = a.xc[int64_t(col) * D + k];
        kf.prep(xcand, cs[cb]);
        vxc[cb] = a.vx[int64_t(g) * Kp + col0 + 16 * cb + lc];
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t orow = row0 + kq + 4 * reg;
        const int64_t oc = orow < a.N ? orow : a.N - 1;
        double z[D], zs[D];
#pragma unroll
        for (int k = 0; k < D; ++k) z[k] = a.pts[k * a.N + oc];
        kf.prep(z, zs);
        const double mu = a.mean[int64_t(g) * a.N + oc] - fmin;
        const double vz = a.var[int64_t(g) * a.N + oc];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const double proj = reg == 0 ? acc[cb].x : reg == 1 ? acc[cb].y
                                                   : reg == 2 ? acc[cb].z : acc[cb].w;
          const double c = kf(zs, cs[cb], tab) - proj;
          pair[cb][reg] += ise_term(mu, vz, vxc[cb], c, sg);
          const int col = col0 + 16 * cb + lc;
          if (a.cov && orow < a.N && col < a.K)
            a.cov[(int64_t(g) * a.K + col) * a.N + orow] = c;
        }
      }
    }

#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int col = col0 + 16 * cb + lc;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t orow = row0 + kq + 4 * reg;
        if (orow >= a.N || col >= a.K) continue;
        if (a.pairs) a.pairs[int64_t(col) * a.N + orow] = pair[cb][reg];
        // (rows ascend with reg and with the tile: > keeps the lowest row among equals)
        if ((!a.skip || !a.skip[orow]) && pair[cb][reg] > bv[cb]) {
          bv[cb] = pair[cb][reg];
          bi[cb] = orow;
        }
      }
    }
  }

  // fold the four k-quarters of a wave, then the four waves
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double v2 = __shfl_xor(bv[cb], o, 64);
      const long long i2 = __shfl_xor(bi[cb], o, 64);
      take_better(bv[cb], bi[cb], v2, i2);
    }
    if (kq == 0) {
      rv[wave][16 * cb + lc] = bv[cb];
      ri[wave][16 * cb + lc] = bi[cb];
    }
  }
  __syncthreads();
  if (tid < kIseCols) {
    double v = rv[0][tid];
    long long i = ri[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) take_better(v, i, rv[w][tid], ri[w][tid]);
    a.pval[int64_t(blockIdx.x) * Kp + col0 + tid] = v;
    a.pidx[int64_t(blockIdx.x) * Kp + col0 + tid] = i;
  }
}

// One workgroup per candidate: the best of the workgroups' partials -> alpha[j], target[j]
// (GLOBAL row; -inf and -1 when no row qualified)
__global__ __launch_bounds__(256) void k_ise_final(const double* pval, const long long* pidx,
                                                   int nwg, int Kp, int64_t goff, double* alpha,
                                                   long long* target) {
  __shared__ double sv[256];
  __shared__ long long si[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int w = tid; w < nwg; w += 256)
    take_better(v, i, pval[int64_t(w) * Kp + j], pidx[int64_t(w) * Kp + j]);
  sv[tid] = v;
  si[tid] = i;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) take_better(sv[tid], si[tid], sv[tid + o], si[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    alpha[j] = si[0] == kNoRow ? -INFINITY : sv[0];
    target[j] = si[0] == kNoRow ? -1 : si[0] + goff;
  }
}

// One workgroup: the candidate with the largest alpha, the lowest GLOBAL row among equals, a
// candidate without a target never -> res[0] = value, res[1] = its global row (as int64; -inf
// and -1 when no candidate has a target).  idx: the candidates' LOCAL rows.
__global__ __launch_bounds__(256) void k_ise_pick(const double* alpha, const long long* target,
                                                  const int64_t* idx, int K, int64_t goff,
                                                  double* res) {
  __shared__ double sv[256];
  __shared__ long long si[256];
  const int tid = threadIdx.x;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int j = tid; j < K; j += 256)
    if (target[j] >= 0) take_better(v, i, alpha[j], idx[j] + goff);
  sv[tid] = v;
  si[tid] = i;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) take_better(sv[tid], si[tid], sv[tid + o], si[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    res[0] = si[0] == kNoRow ? -INFINITY : sv[0];
    reinterpret_cast<long long*>(res)[1] = si[0] == kNoRow ? -1 : si[0];
  }
}

#define ISE_DISPATCH(d, call)                                                      \
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

inline unsigned ise_blocks(int64_t N) { return unsigned((N + kIseThreads - 1) / kIseThreads); }

// The blocks of a grid call, in doubles.
//   kSlotIseIn:   idx[Kp] (int64, local rows) | xc[Kp][d] | vx[G][Kp]
//   kSlotIseW:    W_g[n_pad_g][Kp] of every active GP, one after the other | T[n_max][Kp]
//   kSlotIsePart: pval[nwg][Kp] | pidx[nwg][Kp] | alpha[Kp] | target[Kp] | res[2]
//   kSlotIseOut:  pairs[K][N] | cov[G][K][N]   (the test outputs, when asked for)
struct IseLayout {
  size_t idx, xc, vx, in_words;
  size_t w[SGP_MAX_GPS], t, w_words;
  size_t pval, pidx, alpha, target, res, part_words;
};
IseLayout ise_layout(const GpDev* host, int G, unsigned active, int d, int Kp, int nwg) {
  IseLayout l{};
  l.idx = 0;
  l.xc = l.idx + size_t(Kp);
  l.vx = l.xc + size_t(Kp) * d;
  l.in_words = l.vx + size_t(G) * Kp;
  size_t off = 0, n_max = 0;
  for (int g = 0; g < G; ++g) {
    l.w[g] = off;
    if (!((active >> g) & 1u)) continue;
    off += size_t(host[g].n_pad) * Kp;
    n_max = std::max(n_max, size_t(host[g].n));
  }
  l.t = off;
  l.w_words = off + n_max * Kp;
  l.pval = 0;
  l.pidx = l.pval + size_t(nwg) * Kp;
  l.alpha = l.pidx + size_t(nwg) * Kp;
  l.target = l.alpha + size_t(Kp);
  l.res = l.target + size_t(Kp);
  l.part_words = l.res + 2;
  return l;
}

}  // namespace

int sgp_ise_eval(sgp_ctx* ctx, const double* mu, const double* vz, const double* vx,
                 const double* c, int64_t N, double s, double* out) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, s >= 0.0, "s = %g is not a noise variance (>= 0)", s);   // (NaN fails it too)
  if (N <= 0) return 0;
  const int64_t step = std::min(N, kIseEvalRows);
  double* in;
  SGP_TRY(sgp_scratch(ctx, kSlotIseIn, 5 * size_t(step) * 8, &in));
  double *dm = in, *dz = dm + step, *dx = dz + step, *dc = dx + step, *o = dc + step;
  for (int64_t r0 = 0; r0 < N; r0 += step) {
    const int64_t rows = std::min(step, N - r0);
    SGP_TRY(sgp_h2d(ctx, dm, mu + r0, size_t(rows) * 8));
    SGP_TRY(sgp_h2d(ctx, dz, vz + r0, size_t(rows) * 8));
    SGP_TRY(sgp_h2d(ctx, dx, vx + r0, size_t(rows) * 8));
    SGP_TRY(sgp_h2d(ctx, dc, c + r0, size_t(rows) * 8));
    hipLaunchKernelGGL(k_ise_eval, dim3(ise_blocks(rows)), dim3(kIseThreads), 0, ctx->stream, dm,
                       dz, dx, dc, rows, s, o);
    SGP_HIP(ctx, hipGetLastError());
    SGP_TRY(sgp_d2h(ctx, out + r0, o, size_t(rows) * 8));
  }
  return 0;
}

int sgp_grid_ise(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, const int64_t* cand,
                 int K, int about, double* alpha, int64_t* target, double* value, int64_t* gidx,
                 double* pairs, double* cov) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  // ---- every refusal before anything is launched, staged or written
  SGP_CHECK(ctx, K >= 1 && K <= SGP_MAX_ISE, "K = %d candidates (1 .. SGP_MAX_ISE = %d)", K,
            SGP_MAX_ISE);
  SGP_CHECK(ctx, about == SGP_ISE_UNSAFE || about == SGP_ISE_ALL,
            "about = %d is not SGP_ISE_UNSAFE / SGP_ISE_ALL", about);
  SGP_CHECK(ctx, gps && fmin && cand && alpha && target && value && gidx,
            "gps, fmin, cand, alpha, target, value and gidx are required");
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS && G == g->G, "grid was created for %d GPs, got %d",
            g->G, G);
  const int64_t N = g->N;
  for (int j = 0; j < K; ++j)
    SGP_CHECK(ctx, cand[j] >= g->goff && cand[j] < g->goff + N,
              "candidate %d = row %lld is outside the shard [%lld, %lld)", j, (long long)cand[j],
              (long long)g->goff, (long long)(g->goff + N));
  unsigned active = 0;
  for (int q = 0; q < G; ++q)
    if (std::isfinite(fmin[q])) active |= 1u << q;
  SGP_CHECK(ctx, active != 0, "no GP is active: every fmin is infinite or NaN");
  SGP_CHECK(ctx, g->post_valid,
            "the grid holds no current posterior: run a confidence pass (sgp_grid_confidence "
            "/ sgp_grid_posterior) first");
  SGP_CHECK(ctx, !(pairs || cov) || int64_t(G) * K * N <= kIseMaxOut,
            "pairs / cov are test outputs: G K N_local = %lld exceeds 2^24",
            (long long)(int64_t(G) * K * N));
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));      // (fitted, this context, d columns; stages gpdev)
  const int d = g->d;
  SGP_CHECK(ctx, d >= 1 && d <= SGP_MAX_D, "input dimension %d not in 1..%d", d, SGP_MAX_D);

  const int Kp = (K + kIseCols - 1) / kIseCols * kIseCols;
  const int64_t ntiles = (N + kIseRows - 1) / kIseRows;
  const int nwg = int(std::min<int64_t>(ntiles, kIseMaxWg));
  const IseLayout l = ise_layout(host, G, active, d, Kp, nwg);
  double *in, *wbuf, *part, *outb = nullptr;
  SGP_TRY(sgp_scratch(ctx, kSlotIseIn, l.in_words * 8, &in));
  SGP_TRY(sgp_scratch(ctx, kSlotIseW, l.w_words * 8, &wbuf));
  SGP_TRY(sgp_scratch(ctx, kSlotIsePart, l.part_words * 8, &part));
  const size_t pair_words = pairs ? size_t(K) * N : 0;
  const size_t cov_words = cov ? size_t(G) * K * N : 0;
  if (pairs || cov) SGP_TRY(sgp_scratch(ctx, kSlotIseOut, (pair_words + cov_words) * 8, &outb));

  // ---- candidates: local rows up, coordinates and variances gathered on the device
  std::vector<int64_t> idx(size_t(Kp), 0);
  for (int j = 0; j < K; ++j) idx[j] = cand[j] - g->goff;
  int64_t* idx_dev = reinterpret_cast<int64_t*>(in + l.idx);
  SGP_TRY(sgp_h2d(ctx, idx_dev, idx.data(), size_t(Kp) * 8));
  SGP_HIP(ctx, hipMemsetAsync(in + l.xc, 0, (l.in_words - l.xc) * 8, ctx->stream));
  hipLaunchKernelGGL(k_ise_gather, dim3(unsigned((K + 255) / 256)), dim3(256), 0, ctx->stream,
                     g->pts, g->var, N, d, G, idx_dev, K, Kp, in + l.xc, in + l.vx);
  SGP_HIP(ctx, hipGetLastError());

  // ---- operands: W_g = L^-T (L^-1 k_g(X, x_j)), [n_pad][Kp], zero in the padding
  SGP_HIP(ctx, hipMemsetAsync(wbuf, 0, l.t * 8, ctx->stream));
  double flops = 0.0;
  for (int q = 0; q < G; ++q) {
    if (!((active >> q) & 1u)) continue;
    sgp_gp* gp = gps[q];
    const int n = int(gp->n);
    double *Wq = wbuf + l.w[q], *T = wbuf + l.t;
    const double* Linv = static_cast<const double*>(gp->Linv.p);
    SGP_TRY(launch_kernel_matrix(ctx, gp->kern, static_cast<const double*>(gp->X.p), n,
                                 in + l.xc, K, Wq, Kp, 0, 0.0, INT64_MAX));
    const dim3 grid(unsigned(n), unsigned(Kp / 64));
    hipLaunchKernelGGL(k_ise_fwd, grid, dim3(256), 0, ctx->stream, Linv, int64_t(gp->ld), Kp, Wq,
                       T);
    hipLaunchKernelGGL(k_ise_bwd, grid, dim3(256), 0, ctx->stream, Linv, int64_t(gp->ld), n, Kp,
                       T, Wq);
    SGP_HIP(ctx, hipGetLastError());
    flops += 2.0 * double(N) * host[q].n_pad * Kp;
  }

  // ---- the rows
  IseArgs a{};
  a.gps = g->gpdev;
  a.G = G;
  a.active = active;
  for (int q = 0; q < G; ++q) {
    a.fmin[q] = fmin[q];
    a.s[q] = gps[q]->noise_var + 1e-8;
    a.W[q] = (active >> q) & 1u ? wbuf + l.w[q] : nullptr;
  }
  a.pts = g->pts;
  a.mean = g->mean;
  a.var = g->var;
  a.skip = about == SGP_ISE_UNSAFE ? g->S : nullptr;
  a.N = N;
  a.xc = in + l.xc;
  a.vx = in + l.vx;
  a.K = K;
  a.Kp = Kp;
  a.pairs = pairs ? outb : nullptr;
  a.cov = cov ? outb + pair_words : nullptr;
  a.pval = part + l.pval;
  a.pidx = reinterpret_cast<long long*>(part + l.pidx);
  if (cov) SGP_HIP(ctx, hipMemsetAsync(a.cov, 0, cov_words * 8, ctx->stream));
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, flops));
#define CALL(DD)                                                                              \
  hipLaunchKernelGGL(k_ise_rows<DD>, dim3(unsigned(nwg), unsigned(Kp / kIseCols)), dim3(256), 0, \
                     ctx->stream, a)
  ISE_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(tm.end(ctx));
  double* alpha_dev = part + l.alpha;
  long long* target_dev = reinterpret_cast<long long*>(part + l.target);
  hipLaunchKernelGGL(k_ise_final, dim3(unsigned(K)), dim3(256), 0, ctx->stream, a.pval, a.pidx,
                     nwg, Kp, g->goff, alpha_dev, target_dev);
  hipLaunchKernelGGL(k_ise_pick, dim3(1), dim3(256), 0, ctx->stream, alpha_dev, target_dev,
                     idx_dev, K, g->goff, part + l.res);
  SGP_HIP(ctx, hipGetLastError());
  // one read-back of alpha | target | {value, gidx}: contiguous in the block
  std::vector<double> h(2 * size_t(Kp) + 2);
  SGP_TRY(sgp_d2h(ctx, h.data(), alpha_dev, h.size() * 8));
  memcpy(alpha, h.data(), size_t(K) * 8);
  memcpy(target, h.data() + Kp, size_t(K) * 8);
  *value = h[2 * size_t(Kp)];
  memcpy(gidx, &h[2 * size_t(Kp) + 1], 8);
  if (pairs) SGP_TRY(sgp_d2h(ctx, pairs, a.pairs, pair_words * 8));
  if (cov) SGP_TRY(sgp_d2h(ctx, cov, a.cov, cov_words * 8));
  return 0;
}
