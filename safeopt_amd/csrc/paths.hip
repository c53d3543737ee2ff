// Posterior sample PATHS by pathwise conditioning (Wilson et al. 2020, "Efficiently sampling
// functions from Gaussian process posteriors"): a path is a function,
//
//   phi_i(x)   = sqrt(2 v / m) cos(omega_i . x + b_i)          i = 1 .. m,  v = k(x, x)
//   V[:, s]    = alpha - Ky^-1 (Phi(X) W[:, s] + E[:, s])      (sgp_gp_path_weights)
//   f_s(x)     = sum_i W[i, s] phi_i(x) + sum_j k(x, X_j) V[j, s]
//
// O(m + n) per row and path, no N x N matrix, evaluated anywhere and any number of times --
// where the exact draw of joint.hip stops at SGP_MAX_JOINT rows.
//
// The hot kernel (k_paths) is ONE GEMM-shaped product on v_mfma_f64_16x16x4_f64:
//   [Phi(x) | k(x, X)]  (rows x (m + n))   times   [amp W ; V]  ((m + n) x S).
// A workgroup takes tiles of 64 rows, 16 per wave.  Lane (r, k) = (lane & 15, lane >> 4) of a
// wave evaluates entry (row r, k-index k) of a 16 x 4 block of the left matrix -- a cosine
// or a covariance (kern_eval.h), each ONCE, already in the A-operand layout -- and feeds it to
// the MFMAs of all ceil(S / 16) column blocks.  The right matrix goes through LDS in stages of
// kPathChunk rows (pitch = 16 mod 32 doubles: the two k-rows a 32-lane half of ds_read_b64
// touches lie on opposite halves of the banks).  Neither Phi nor k(x, X) reaches memory.
//
// The arg-max per path is an epilogue: every lane keeps the best (value, row) of the rows and
// columns it owns over all tiles of its workgroup, the workgroup folds them, k_paths_final
// folds the workgroups.  Lowest row wins a tie at every level.  With values == NULL no N x S
// array exists.
//
// Every sum is formed in a fixed order (no atomics), and a row's result does not depend on
// where the row sits in a launch: same inputs, same bits -- for a call repeated, for a subset
// of the rows, for the grid's resident rows against the same rows passed in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sweep_shared.h"

namespace {

constexpr int kPathRows = 64;       // rows of a tile (16 per wave)
constexpr int kPathChunk = 64;      // rows of [W ; V] per LDS stage = 16 k-steps
constexpr int kPathMaxPitch = 80;   // S_pad = 64 -> pitch 80
constexpr int kPathMaxWg = 4096;    // workgroups of a launch (each walks tiles with that stride)
constexpr int64_t kPathEvalRows = 1 << 20;   // rows per launch of sgp_gp_paths_eval
constexpr long long kNoRow = std::numeric_limits<long long>::max();

struct PathArgs {
  const GpDev* gps;
  const double* pts;      // SoA [D][ldp]
  int64_t ldp;
  int64_t N;
  const double* OmB;      // [m4][D + 1]: frequency | phase; zero rows behind m
  const double* B;        // [m4 + ncov][Sp]: amp W (zero rows behind m), then V (zero padded)
  int m4;                 // features rounded up to 4
  int ncov;               // 0 (features only) or the GP's n_pad
  int S, Sp, pitch;
  const uint8_t* mask;    // rows that count for the arg-max; null: all
  double* values;         // [N][S], or null
  double* pval;           // [gridDim.x][Sp] partial maxima, or null (no arg-max)
  long long* pidx;        //   ... and their LOCAL rows (kNoRow: none)
};

// (value, row) pairs: the larger value, the lower row among equals
__device__ __forceinline__ void take_better(double& v, long long& i, double v2, long long i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_paths(PathArgs a) {
  __shared__ double tab[kExpTabSize];
  __shared__ double sB[kPathChunk * kPathMaxPitch];
  __shared__ double sOm[kPathChunk * (D + 1)];
  __shared__ double rv[4][64];
  __shared__ long long ri[4][64];
  exp_tab_init(tab);
  __syncthreads();
  const GpDev& gp = a.gps[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, lc = lane & 15;
  const int ncb = a.Sp / 16, Sp = a.Sp, pitch = a.pitch;
  KernFast<D> kf(gp.kern);
  double bv[4];
  long long bi[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    bv[cb] = -INFINITY;
    bi[cb] = kNoRow;
  }
  const int64_t ntiles = (a.N + kPathRows - 1) / kPathRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kPathRows + wave * 16;
    double x[D], xs[D];
    {
      const int64_t r = row0 + lc < a.N ? row0 + lc : a.N - 1;
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = a.pts[k * a.ldp + r];
    }
    kf.prep(x, xs);
    double4_t acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};

    // ---- features: A[r][k] = cos(omega_k . x_r + b_k), amp folded into W
    for (int k0 = 0; k0 < a.m4; k0 += kPathChunk) {
      const int kc = min(kPathChunk, a.m4 - k0);
      __syncthreads();
      for (int e = tid; e < kc * Sp; e += 256) {
        const int r = e / Sp, c = e - r * Sp;
        sB[r * pitch + c] = a.B[int64_t(k0 + r) * Sp + c];
      }
      for (int e = tid; e < kc * (D + 1); e += 256) sOm[e] = a.OmB[int64_t(k0) * (D + 1) + e];
      __syncthreads();
      for (int u = 0; u < kc / 4; ++u) {
        const int r = 4 * u + kq;
        const double* om = sOm + r * (D + 1);
        double arg = om[D];
#pragma unroll
        for (int k = 0; k < D; ++k) arg = fma(om[k], x[k], arg);
        const double av = cos(arg);
        const double* b = sB + r * pitch + lc;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (cb < ncb)
            acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[16 * cb], acc[cb], 0, 0, 0);
      }
    }

    // ---- covariances: A[r][j] = k(x_r, X_j); per block of 16 training points the lane holds
    // av[s] = k(x, X_{16 jb + 4 s + kq}), the A operand of k-step 4 jb + s
    for (int k0 = 0; k0 < a.ncov; k0 += kPathChunk) {
      const int kc = min(kPathChunk, a.ncov - k0);          // a multiple of 16
      __syncthreads();
      for (int e = tid; e < kc * Sp; e += 256) {
        const int r = e / Sp, c = e - r * Sp;
        sB[r * pitch + c] = a.B[int64_t(a.m4 + k0 + r) * Sp + c];
      }
      __syncthreads();
      for (int jb = 0; jb < kc / 16; ++jb) {
        double av[4];
        kf.template many<4>(xs, gp.Xs + int64_t(k0 + 16 * jb + kq) * D, 4 * D, tab, av);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double* b = sB + (16 * jb + 4 * s + kq) * pitch + lc;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            if (cb < ncb)
              acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[16 * cb], acc[cb], 0, 0, 0);
        }
      }
    }

    // ---- D layout: column = lane & 15, rows kq + 4 reg of the wave's 16
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      if (cb >= ncb) continue;
      const int col = 16 * cb + lc;
      const double v[4] = {acc[cb].x, acc[cb].y, acc[cb].z, acc[cb].w};
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t orow = row0 + kq + 4 * reg;
        if (orow >= a.N || col >= a.S) continue;
        if (a.values) a.values[orow * a.S + col] = v[reg];
        // (rows ascend with reg and with the tile: > keeps the lowest row among equals)
        if (a.pval && (!a.mask || a.mask[orow]) && v[reg] > bv[cb]) {
          bv[cb] = v[reg];
          bi[cb] = orow;
        }
      }
    }
  }

  if (!a.pval) return;
  // fold the four k-quarters of a wave, then the four waves
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    if (cb >= ncb) continue;
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
  if (tid < Sp) {
    double v = rv[0][tid];
    long long i = ri[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) take_better(v, i, rv[w][tid], ri[w][tid]);
    a.pval[int64_t(blockIdx.x) * Sp + tid] = v;
    a.pidx[int64_t(blockIdx.x) * Sp + tid] = i;
  }
}

// One workgroup per path: the best of the workgroups' partials -> best_val[s], best_idx[s]
// (GLOBAL row, -1 and -inf when no row qualified).
__global__ __launch_bounds__(256) void k_paths_final(const double* pval, const long long* pidx,
                                                     int nwg, int Sp, int64_t goff, double* out_v,
                                                     int64_t* out_i) {
  __shared__ double sv[256];
  __shared__ long long si[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int w = tid; w < nwg; w += 256) take_better(v, i, pval[int64_t(w) * Sp + s], pidx[int64_t(w) * Sp + s]);
  sv[tid] = v;
  si[tid] = i;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      take_better(sv[tid], si[tid], sv[tid + o], si[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    out_v[s] = sv[0];
    out_i[s] = si[0] == kNoRow ? -1 : int64_t(si[0]) + goff;
  }
}

// The ranks' records -> the result of the whole grid (sgp_grid_paths_comm).  A record is what
// k_paths_final leaves: [Sp] best values | [Sp] GLOBAL rows (-1: no row of that shard
// qualified); recs holds `world` of them in rank order.  Thread s folds path s in the order of
// take_better -- the largest value, the lowest global row among equals; a record without a row
// never wins against one with a row -- and writes out[s] | out[Sp + s] (-inf / -1 when no
// shard qualified).  world x S pairs: one workgroup.
__global__ __launch_bounds__(64) void k_paths_merge(const double* recs, int world, int S, int Sp,
                                                    double* out) {
  const int s = threadIdx.x;
  if (s >= S) return;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int r = 0; r < world; ++r) {
    const double* rec = recs + int64_t(r) * 2 * Sp;
    const long long i2 = reinterpret_cast<const long long*>(rec + Sp)[s];
    if (i2 >= 0) take_better(v, i, rec[s], i2);
  }
  out[s] = i == kNoRow ? -INFINITY : v;
  reinterpret_cast<long long*>(out + Sp)[s] = i == kNoRow ? -1 : i;
}

// ---- V = alpha 1^T - L^-T (L^-1 (U + E)) from the dense inverse factor ----------------------
// One workgroup per row j, thread (q, s) = (tid >> 6, tid & 63): the terms i = q, q + 4, ...
// of column s in order, then (p0 + p1) + (p2 + p3).
__global__ __launch_bounds__(256) void k_path_fwd(const double* Linv, int64_t ld, int n, int S,
                                                  const double* U, const double* E, double* T) {
  __shared__ double part[4][64];
  const int j = blockIdx.x, s = threadIdx.x & 63, q = threadIdx.x >> 6;
  double acc = 0.0;
  if (s < S)
    for (int i = q; i <= j; i += 4)
      acc = fma(Linv[int64_t(j) * ld + i], U[int64_t(i) * S + s] + E[int64_t(i) * S + s], acc);
  part[q][s] = acc;
  __syncthreads();
  if (q == 0 && s < S) T[int64_t(j) * S + s] = (part[0][s] + part[1][s]) + (part[2][s] + part[3][s]);
}

__global__ __launch_bounds__(256) void k_path_bwd(const double* Linv, int64_t ld, int n, int S,
                                                  const double* T, const double* alpha,
                                                  double* V) {
  __shared__ double part[4][64];
  const int j = blockIdx.x, s = threadIdx.x & 63, q = threadIdx.x >> 6;
  double acc = 0.0;
  if (s < S)
    for (int i = j + q; i < n; i += 4)
      acc = fma(Linv[int64_t(i) * ld + j], T[int64_t(i) * S + s], acc);
  part[q][s] = acc;
  __syncthreads();
  if (q == 0 && s < S)
    V[int64_t(j) * S + s] = alpha[j] - ((part[0][s] + part[1][s]) + (part[2][s] + part[3][s]));
}

#define PATH_DISPATCH(d, call)                                                     \
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

int path_blocks(int64_t N) {
  return int(std::min<int64_t>((N + kPathRows - 1) / kPathRows, kPathMaxWg));
}

int launch_paths(sgp_ctx* ctx, int d, const PathArgs& pa) {
  SGP_CHECK(ctx, d >= 1 && d <= SGP_MAX_D, "input dimension %d not in 1..%d", d, SGP_MAX_D);
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 2.0 * double(pa.N) * (pa.m4 + pa.ncov) * pa.S));
#define CALL(DD) \
  hipLaunchKernelGGL(k_paths<DD>, dim3(unsigned(path_blocks(pa.N))), dim3(256), 0, ctx->stream, pa)
  PATH_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}

// The argument checks of the three entry points.
int path_ready(sgp_gp* gp, int m, int S) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, m >= 1 && m <= SGP_MAX_FEATURES, "m = %d features (1 .. SGP_MAX_FEATURES = %d)",
            m, SGP_MAX_FEATURES);
  SGP_CHECK(ctx, S >= 1 && S <= SGP_MAX_PATHS, "S = %d paths (1 .. SGP_MAX_PATHS = %d)", S,
            SGP_MAX_PATHS);
  return 0;
}

// The operands every launch shares: the GP descriptor, [omega | b] and [amp W ; V], padded
// with zeros (a padded feature is cos(0) times a zero weight, a padded training row a finite
// covariance times a zero weight).  V == nullptr: features only.
int path_stage(sgp_gp* gp, const double* Omega, const double* phase, int m, const double* W,
               const double* V, int S, PathArgs* pa) {
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  const int m4 = (m + 3) / 4 * 4;
  const int Sp = (S + 15) / 16 * 16;
  const int ncov = V ? gp->n_pad : 0;
  std::vector<double> om(size_t(m4) * (d + 1), 0.0), B(size_t(m4 + ncov) * Sp, 0.0);
  const double amp = std::sqrt(2.0 * gp->kern.kdiag / double(m));
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k < d; ++k) om[size_t(i) * (d + 1) + k] = Omega[size_t(i) * d + k];
    om[size_t(i) * (d + 1) + d] = phase[i];
    for (int s = 0; s < S; ++s) B[size_t(i) * Sp + s] = amp * W[size_t(i) * S + s];
  }
  if (V)
    for (int64_t j = 0; j < gp->n; ++j)
      for (int s = 0; s < S; ++s) B[size_t(m4 + j) * Sp + s] = V[size_t(j) * S + s];
  GpDev* gdev;
  double *om_dev, *B_dev;
  SGP_TRY(sgp_scratch(ctx, kSlotGpDev, sizeof(GpDev), &gdev));
  SGP_TRY(sgp_scratch(ctx, kSlotPathOm, om.size() * sizeof(double), &om_dev));
  SGP_TRY(sgp_scratch(ctx, kSlotPathB, B.size() * sizeof(double), &B_dev));
  SGP_TRY(sgp_h2d(ctx, gdev, &gp->dev, sizeof(GpDev)));
  SGP_TRY(sgp_h2d(ctx, om_dev, om.data(), om.size() * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, B_dev, B.data(), B.size() * sizeof(double)));
  *pa = PathArgs{};
  pa->gps = gdev;
  pa->OmB = om_dev;
  pa->B = B_dev;
  pa->m4 = m4;
  pa->ncov = ncov;
  pa->S = S;
  pa->Sp = Sp;
  pa->pitch = Sp % 32 == 16 ? Sp : Sp + 16;
  return 0;
}


// ---- one path at the particles of a swarm (sgp_swarm_fitness_path / sgp_swarm_run_path) ------
// values[p] = f(x_p) / scaling0 + values[p]: the path term of a Thompson swarm's fitness on
// top of the penalty the shaping pass (fitness.h, kSwarmThompson) left in values[p],
//   f(x) = sum_i amp w_i cos(omega_i . x + b_i) + sum_j k(x, X_j) v_j.
// A ROW kernel: one column has nothing for the matrix pipe to share between columns, so the
// m + n cosines and covariances of a row are VALU work and the products with them.  16
// lanes per particle (4 particles a wave, 16 a workgroup): lane l = (kq, c) = (l & 3, l >> 2)
// takes the features l, l + 16, ... and, of every fourth block of 16 training rows (jb = c,
// c + 4, ...), the rows 16 jb + kq + 4 s -- the access pattern of k_paths, KernFast::many<4>.
// Each lane sums its terms in that order into one accumulator, then the 16 lanes fold by
// xor 1, 2, 4, 8 (IEEE addition commutes: every lane ends with the same bits).  The order
// depends on m and n alone: a particle's value does not depend on P, on its row or on the
// launch.  No atomics; neither Phi nor k(x, X) reaches memory.
constexpr int kRowLanes = 16;        // lanes of a particle
constexpr int kRowParticles = 16;    // particles of a workgroup

template <int D>
__global__ __launch_bounds__(256) void k_swarm_path(const GpDev* gps, SwarmPath sp,
                                                    SweepPoints pts, double scaling0,
                                                    double* values) {
  __shared__ double tab[kExpTabSize];
  exp_tab_init(tab);
  __syncthreads();
  const GpDev& gp = gps[0];
  const int tid = threadIdx.x, l = tid & (kRowLanes - 1), kq = l & 3, c = l >> 2;
  const int64_t p = int64_t(blockIdx.x) * kRowParticles + (tid >> 4);
  const int64_t r = p < pts.N ? p : pts.N - 1;    // (a spare group repeats the last row)
  KernFast<D> kf(gp.kern);
  double x[D], xs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = pts.base[r * pts.stride_row + k * pts.stride_col];
  kf.prep(x, xs);
  double acc = 0.0;
  // ---- features: cos(omega_i . x + b_i) amp w_i (a padded feature: cos(0) times zero)
  for (int i = l; i < sp.m16; i += kRowLanes) {
    const double* om = sp.om + int64_t(i) * (D + 1);
    double arg = om[D];
#pragma unroll
    for (int k = 0; k < D; ++k) arg = fma(om[k], x[k], arg);
    acc = fma(cos(arg), sp.wv[i], acc);
  }
  // ---- covariances: k(x, X_j) v_j (a padded training row: finite times zero)
  const double* v = sp.wv + sp.m16;
  for (int jb = c; jb < sp.ncov / 16; jb += 4) {
    double av[4];
    kf.template many<4>(xs, gp.Xs + int64_t(16 * jb + kq) * D, 4 * D, tab, av);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = fma(av[s], v[16 * jb + 4 * s + kq], acc);
  }
#pragma unroll
  for (int o = 1; o < kRowLanes; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (l == 0 && p < pts.N) values[p] = acc / scaling0 + values[p];
}
}  // namespace

int swarm_path_ready(sgp_gp* gp, int m) { return path_ready(gp, m, 1); }

// [omega | b], then [amp w ; v], zero padded: features to 16 (one per lane of a particle),
// training rows to the GP's n_pad
int swarm_path_stage(sgp_gp* gp, const double* Omega, const double* phase, int m,
                     const double* w, const double* v, SwarmPath* out) {
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  const int m16 = (m + kRowLanes - 1) / kRowLanes * kRowLanes;
  std::vector<double> om(size_t(m16) * (d + 1), 0.0), wv(size_t(m16) + gp->n_pad, 0.0);
  const double amp = std::sqrt(2.0 * gp->kern.kdiag / double(m));
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k < d; ++k) om[size_t(i) * (d + 1) + k] = Omega[size_t(i) * d + k];
    om[size_t(i) * (d + 1) + d] = phase[i];
    wv[i] = amp * w[i];
  }
  for (int64_t j = 0; j < gp->n; ++j) wv[size_t(m16) + j] = v[j];
  double *om_dev, *wv_dev;
  SGP_TRY(sgp_scratch(ctx, kSlotPathOm, om.size() * sizeof(double), &om_dev));
  SGP_TRY(sgp_scratch(ctx, kSlotPathB, wv.size() * sizeof(double), &wv_dev));
  SGP_TRY(sgp_h2d(ctx, om_dev, om.data(), om.size() * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, wv_dev, wv.data(), wv.size() * sizeof(double)));
  *out = SwarmPath{om_dev, wv_dev, m16, gp->n_pad};
  return 0;
}

int launch_swarm_path(sgp_ctx* ctx, const GpDev* gps_dev, int d, const SwarmPath& path,
                      SweepPoints pts, double scaling0, double* values) {
  if (pts.N <= 0) return 0;
  const int64_t nwg = (pts.N + kRowParticles - 1) / kRowParticles;
  SGP_CHECK(ctx, nwg <= INT32_MAX, "%lld particles are too many for one launch",
            (long long)pts.N);
#define CALL(DD)                                                                              \
  hipLaunchKernelGGL(k_swarm_path<DD>, dim3(unsigned(nwg)), dim3(256), 0, ctx->stream, gps_dev, \
                     path, pts, scaling0, values)
  PATH_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int sgp_gp_path_weights(sgp_gp* gp, const double* Omega, const double* phase, int m,
                        const double* W, const double* E, int S, double* V_out) {
  SGP_TRY(path_ready(gp, m, S));
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  const int64_t n = gp->n;
  PathArgs pa;
  SGP_TRY(path_stage(gp, Omega, phase, m, W, nullptr, S, &pa));
  // Phi(X) W by the feature half of k_paths, the training rows as the points
  double *pts, *buf;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(n) * d * sizeof(double), &pts));
  SGP_TRY(sgp_scratch(ctx, kSlotPathOut, 4 * size_t(n) * S * sizeof(double), &buf));
  std::vector<double> soa(size_t(n) * d);
  for (int64_t r = 0; r < n; ++r)
    for (int k = 0; k < d; ++k) soa[size_t(k) * n + r] = gp->xhost[size_t(r) * d + k];
  SGP_TRY(sgp_h2d(ctx, pts, soa.data(), soa.size() * sizeof(double)));
  const size_t ns = size_t(n) * S;
  double *U = buf, *Ed = buf + ns, *T = buf + 2 * ns, *Vd = buf + 3 * ns;
  SGP_TRY(sgp_h2d(ctx, Ed, E, ns * sizeof(double)));
  pa.pts = pts;
  pa.ldp = n;
  pa.N = n;
  pa.values = U;
  SGP_TRY(launch_paths(ctx, d, pa));
  const double* Linv = static_cast<const double*>(gp->Linv.p);
  hipLaunchKernelGGL(k_path_fwd, dim3(unsigned(n)), dim3(256), 0, ctx->stream, Linv,
                     int64_t(gp->ld), int(n), S, U, Ed, T);
  hipLaunchKernelGGL(k_path_bwd, dim3(unsigned(n)), dim3(256), 0, ctx->stream, Linv,
                     int64_t(gp->ld), int(n), S, T, static_cast<const double*>(gp->alpha.p), Vd);
  SGP_HIP(ctx, hipGetLastError());
  return sgp_d2h(ctx, V_out, Vd, ns * sizeof(double));
}

int sgp_gp_paths_eval(sgp_gp* gp, const double* Omega, const double* phase, int m,
                      const double* W, const double* V, int S, const double* Xnew, int64_t N,
                      int64_t stride_row, int64_t stride_col, double* out) {
  SGP_TRY(path_ready(gp, m, S));
  if (N <= 0) return 0;
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  PathArgs pa;
  SGP_TRY(path_stage(gp, Omega, phase, m, W, V, S, &pa));
  const int64_t step = std::min(N, kPathEvalRows);
  double *pts, *vals;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(step) * d * sizeof(double), &pts));
  SGP_TRY(sgp_scratch(ctx, kSlotPathOut, size_t(step) * S * sizeof(double), &vals));
  std::vector<double> soa(size_t(step) * d);
  for (int64_t r0 = 0; r0 < N; r0 += step) {
    const int64_t rows = std::min(step, N - r0);
    // one SoA copy whatever the strides: the same bits for every layout
    for (int64_t r = 0; r < rows; ++r)
      for (int k = 0; k < d; ++k)
        soa[size_t(k) * rows + r] = Xnew[(r0 + r) * stride_row + k * stride_col];
    SGP_TRY(sgp_h2d(ctx, pts, soa.data(), size_t(rows) * d * sizeof(double)));
    pa.pts = pts;
    pa.ldp = rows;
    pa.N = rows;
    pa.values = vals;
    SGP_TRY(launch_paths(ctx, d, pa));
    SGP_TRY(sgp_d2h(ctx, out + size_t(r0) * S, vals, size_t(rows) * S * sizeof(double)));
  }
  return 0;
}

// sgp_grid_paths, and with `merge` sgp_grid_paths_comm: the shard's records all-gathered over
// the context's communicator and merged on the device before the one read-back.
static int grid_paths(sgp_grid* g, sgp_gp* gp, const double* Omega, const double* phase, int m,
                      const double* W, const double* V, int S, int mask, double* values,
                      double* best_val, int64_t* best_idx, bool merge) {
  SGP_TRY(path_ready(gp, m, S));
  sgp_ctx* ctx = gp->ctx;
  SGP_CHECK(ctx, g->ctx == ctx, "the GP lives in another context (device %d) than the grid "
            "(device %d)", ctx->device, g->ctx->device);
  SGP_CHECK(ctx, gp->kern.d == g->d, "GP input_dim %d != %d columns of the grid", gp->kern.d,
            g->d);
  SGP_CHECK(ctx, (best_val != nullptr) == (best_idx != nullptr),
            "best_val and best_idx come together");
  if (!values && !best_val) return 0;
  PathArgs pa;
  SGP_TRY(path_stage(gp, Omega, phase, m, W, V, S, &pa));
  pa.pts = g->pts;
  pa.ldp = g->N;
  pa.N = g->N;
  pa.mask = mask ? g->S : nullptr;
  if (values)
    SGP_TRY(sgp_scratch(ctx, kSlotPathOut, size_t(g->N) * S * sizeof(double), &pa.values));
  const int nwg = path_blocks(g->N);
  bool comm = false;
  if (merge && best_val) SGP_TRY(comm_or_single(ctx, &comm));
  const int world = comm ? ctx->world : 1;
  double* res = nullptr;
  if (best_val) {
    // [nwg][Sp] values | [nwg][Sp] rows | [Sp] best values | [Sp] best rows; with a
    // communicator behind them: the ranks' [2 Sp] records | the merged [Sp] values | [Sp] rows
    double* part;
    const size_t recs = comm ? size_t(world) + 1 : 0;
    SGP_TRY(sgp_scratch(ctx, kSlotPathPart,
                        2 * (size_t(nwg) + 1 + recs) * pa.Sp * sizeof(double), &part));
    pa.pval = part;
    pa.pidx = reinterpret_cast<long long*>(part + size_t(nwg) * pa.Sp);
    res = part + 2 * size_t(nwg) * pa.Sp;
  }
  SGP_TRY(launch_paths(ctx, g->d, pa));
  if (best_val) {
    hipLaunchKernelGGL(k_paths_final, dim3(unsigned(S)), dim3(256), 0, ctx->stream, pa.pval,
                       pa.pidx, nwg, pa.Sp, g->goff, res, reinterpret_cast<int64_t*>(res + pa.Sp));
    SGP_HIP(ctx, hipGetLastError());
    if (comm) {
      // (the record's entries behind S are never read: k_paths_merge stops at S)
      double* all = res + 2 * size_t(pa.Sp);
      double* merged = all + 2 * size_t(world) * pa.Sp;
      SGP_TRY(coll_allgather(ctx, res, all, 2 * size_t(pa.Sp) * sizeof(double)));
      hipLaunchKernelGGL(k_paths_merge, dim3(1), dim3(64), 0, ctx->stream, all, world, S, pa.Sp,
                         merged);
      SGP_HIP(ctx, hipGetLastError());
      res = merged;
    }
    if (merge) {
      // one read-back of the result
      double h[2 * SGP_MAX_PATHS];
      SGP_TRY(sgp_d2h(ctx, h, res, 2 * size_t(pa.Sp) * sizeof(double)));
      memcpy(best_val, h, size_t(S) * sizeof(double));
      memcpy(best_idx, h + pa.Sp, size_t(S) * sizeof(int64_t));
    } else {
      SGP_TRY(sgp_d2h(ctx, best_val, res, size_t(S) * sizeof(double)));
      SGP_TRY(sgp_d2h(ctx, best_idx, res + pa.Sp, size_t(S) * sizeof(int64_t)));
    }
  }
  if (values) SGP_TRY(sgp_d2h(ctx, values, pa.values, size_t(g->N) * S * sizeof(double)));
  return 0;
}

int sgp_grid_paths(sgp_grid* g, sgp_gp* gp, const double* Omega, const double* phase, int m,
                   const double* W, const double* V, int S, int mask, double* values,
                   double* best_val, int64_t* best_idx) {
  return grid_paths(g, gp, Omega, phase, m, W, V, S, mask, values, best_val, best_idx, false);
}

int sgp_grid_paths_comm(sgp_grid* g, sgp_gp* gp, const double* Omega, const double* phase, int m,
                        const double* W, const double* V, int S, int mask, double* values,
                        double* best_val, int64_t* best_idx) {
  return grid_paths(g, gp, Omega, phase, m, W, V, S, mask, values, best_val, best_idx, true);
}
