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
// a function of that column of B.)  Nor on the shard the rows lie in: sgp_grid_ise_at takes the
// candidates BY VALUE (global row, coordinates, variances) and runs the same kernels over this
// shard's rows, and sgp_grid_ise_comm merges the ranks' alpha | target blocks behind one
// all-gather (k_ise_merge: the largest alpha, the lowest global target among equals) -- the bits
// of one rank over the whole grid, on every rank.
//
// The candidates themselves -- the K safe rows with the largest
//   key = sum over the active g, in the order of g, of log1p(var_g / s_g) / 2 --
// are chosen where the variances are, by the pattern of the big passes (sets.hip: k_pass_hist,
// k_pass_list): sgp_grid_ise_keys (count, min and max of the shard's keys), sgp_grid_ise_hist
// (kPassBins bins over an agreed range, integer counts) and sgp_grid_ise_list (the safe rows at
// or above a threshold in ascending row, compacted by prefix sums: deterministic).  Three
// HBM-bound reads of var and S.  The device's log1p is not NumPy's to the last bit, so the
// device only ever picks a SUPERSET (SafeOpt._ise_select) and the host orders it exactly.
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

// ---- candidate selection: the keys of the safe rows ------------------------------------------
struct IseKeyArgs {
  const double* var;             // [G][N]
  const uint8_t* S;
  int64_t N;
  int G;
  unsigned active;
  double s[SGP_MAX_GPS];         // noise_var + 1e-8
};

// (built without contraction: a product and a sum, as NumPy forms key + 0.5 * log1p(var / s))
__device__ __forceinline__ double ise_key(const IseKeyArgs& a, int64_t r) {
  double key = 0.0;
  for (int g = 0; g < a.G; ++g)
    if ((a.active >> g) & 1u) key = key + 0.5 * log1p(a.var[int64_t(g) * a.N + r] / a.s[g]);
  return key;
}

constexpr int kIseKeyWg = 1024;               // workgroups of k_ise_keys, at most

// part[b] = {count, min, max} of the keys of the safe rows workgroup b walks
__global__ __launch_bounds__(256) void k_ise_keys(IseKeyArgs a, double* part) {
  __shared__ double rc[4], rlo[4], rhi[4];
  double cnt = 0.0, lo = INFINITY, hi = -INFINITY;      // (a count below 2^53: exact)
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < a.N; r += int64_t(gridDim.x) * 256) {
    if (!a.S[r]) continue;
    const double key = ise_key(a, r);
    cnt += 1.0;
    lo = fmin(lo, key);
    hi = fmax(hi, key);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    rc[threadIdx.x >> 6] = cnt;
    rlo[threadIdx.x >> 6] = lo;
    rhi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[3 * blockIdx.x + 0] = (rc[0] + rc[1]) + (rc[2] + rc[3]);
    part[3 * blockIdx.x + 1] = fmin(fmin(rlo[0], rlo[1]), fmin(rlo[2], rlo[3]));
    part[3 * blockIdx.x + 2] = fmax(fmax(rhi[0], rhi[1]), fmax(rhi[2], rhi[3]));
  }
}

// One workgroup: out[3] = the fold of the workgroups' {count, min, max}
__global__ __launch_bounds__(256) void k_ise_keys_final(const double* part, int nwg, double* out) {
  __shared__ double sc[256], slo[256], shi[256];
  const int tid = threadIdx.x;
  double cnt = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int w = tid; w < nwg; w += 256) {
    cnt += part[3 * w];
    lo = fmin(lo, part[3 * w + 1]);
    hi = fmax(hi, part[3 * w + 2]);
  }
  sc[tid] = cnt;
  slo[tid] = lo;
  shi[tid] = hi;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      sc[tid] += sc[tid + o];
      slo[tid] = fmin(slo[tid], slo[tid + o]);
      shi[tid] = fmax(shi[tid], shi[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = sc[0];
    out[1] = slo[0];
    out[2] = shi[0];
  }
}

// k_pass_hist's rule (sets.hip): bin = int((key - lo) * (kPassBins / (hi - lo))), clamped
__global__ __launch_bounds__(256) void k_ise_hist(IseKeyArgs a, double lo, double hi,
                                                  unsigned* hist) {
  __shared__ unsigned sh[kPassBins];
  for (int b = threadIdx.x; b < kPassBins; b += 256) sh[b] = 0;
  __syncthreads();
  const double scale = double(kPassBins) / (hi - lo);
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < a.N; r += int64_t(gridDim.x) * 256) {
    if (!a.S[r]) continue;
    int b = int((ise_key(a, r) - lo) * scale);
    b = b < 0 ? 0 : (b >= kPassBins ? kPassBins - 1 : b);
    atomicAdd(&sh[b], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kPassBins; b += 256)
    if (sh[b]) atomicAdd(&hist[b], sh[b]);
}

// The list, k_pass_count / k_pass_scan / k_pass_list's way: counts[c] = the rows chunk c (256
// consecutive rows) lists; their exclusive prefix sum; then every listed row behind its chunk's
// offset -- ascending row, whatever the order the workgroups run in.
__device__ __forceinline__ bool ise_take(const IseKeyArgs& a, int64_t r, double thr, double* key) {
  if (r >= a.N || !a.S[r]) return false;
  *key = ise_key(a, r);
  return *key >= thr;
}

__global__ __launch_bounds__(256) void k_ise_count(IseKeyArgs a, double thr, int* counts) {
  __shared__ int wc[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r0 = int64_t(blockIdx.x) * 256; r0 < a.N; r0 += int64_t(gridDim.x) * 256) {
    double key;
    const unsigned long long b = __ballot(ise_take(a, r0 + threadIdx.x, thr, &key));
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[r0 / 256] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
    __syncthreads();
  }
}

// exclusive prefix sum of the chunk counts (in place), the total into *total (k_pass_scan)
__global__ __launch_bounds__(1024) void k_ise_scan(int* counts, int nchunks, long long* total) {
  __shared__ int part[1024];
  __shared__ int carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nchunks; base += 1024) {
    const int i = base + t;
    const int v = i < nchunks ? counts[i] : 0;
    part[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int u = (t >= o) ? part[t - o] : 0;
      __syncthreads();
      part[t] += u;
      __syncthreads();
    }
    if (i < nchunks) counts[i] = carry + part[t] - v;
    __syncthreads();
    if (t == 1023) carry += part[1023];
    __syncthreads();
  }
  if (t == 0) *total = carry;
}

// rec[p] = {global row (int64), key, x[d], var[G]} of the p-th listed row, p < cap
__global__ __launch_bounds__(256) void k_ise_fill(IseKeyArgs a, const double* pts, int d,
                                                  int64_t goff, double thr, const int* offsets,
                                                  int cap, double* rec) {
  __shared__ int wc[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int words = 2 + d + a.G;
  for (int64_t r0 = int64_t(blockIdx.x) * 256; r0 < a.N; r0 += int64_t(gridDim.x) * 256) {
    const int64_t r = r0 + threadIdx.x;
    double key = 0.0;
    const bool take = ise_take(a, r, thr, &key);
    const unsigned long long b = __ballot(take);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    int at = offsets[r0 / 256];
    for (int q = 0; q < wave; ++q) at += wc[q];
    at += __popcll(b & ((1ull << lane) - 1ull));
    if (take && at < cap) {
      double* o = rec + int64_t(at) * words;
      reinterpret_cast<long long*>(o)[0] = goff + r;
      o[1] = key;
      for (int k = 0; k < d; ++k) o[2 + k] = pts[int64_t(k) * a.N + r];
      for (int g = 0; g < a.G; ++g) o[2 + d + g] = a.var[int64_t(g) * a.N + r];
    }
    __syncthreads();
  }
}

// The ranks' alpha | target blocks ([world][2][Kp], in rank order) -> the whole grid's:
// per candidate the largest alpha, the lowest GLOBAL target among equals; a rank without a
// target (-inf / -1) never wins, none on any rank gives -inf / -1.
__global__ __launch_bounds__(256) void k_ise_merge(const double* recs, int world, int K, int Kp,
                                                   double* alpha, long long* target) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  double v = -INFINITY;
  long long i = kNoRow;
  for (int r = 0; r < world; ++r) {
    const double* blk = recs + int64_t(r) * 2 * Kp;
    const long long t = reinterpret_cast<const long long*>(blk + Kp)[j];
    if (t >= 0) take_better(v, i, blk[j], t);
  }
  alpha[j] = i == kNoRow ? -INFINITY : v;
  target[j] = i == kNoRow ? -1 : i;
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
//                 | recs[world][2][Kp] | malpha[Kp] | mtarget[Kp] | mres[2]
//                 (world ranks of sgp_grid_ise_comm, 0 otherwise: the gathered alpha | target
//                 blocks and their merge, read back in one piece like alpha | target | res)
//   kSlotIseOut:  pairs[K][N] | cov[G][K][N]   (the test outputs, when asked for)
struct IseLayout {
  size_t idx, xc, vx, in_words;
  size_t w[SGP_MAX_GPS], t, w_words;
  size_t pval, pidx, alpha, target, res, recs, malpha, mtarget, mres, part_words;
};
IseLayout ise_layout(const GpDev* host, int G, unsigned active, int d, int Kp, int nwg,
                     int world) {
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
  l.recs = l.res + 2;
  l.malpha = l.recs + size_t(world) * 2 * Kp;
  l.mtarget = l.malpha + size_t(Kp);
  l.mres = l.mtarget + size_t(Kp);
  l.part_words = world ? l.mres + 2 : l.recs;
  return l;
}

// The scratch of a selection call, in kSlotIsePart (doubles):
//   part[kIseKeyWg][3] | out[3] | total (int64) | hist[kPassBins] (u32) | counts[N / 256 + 2] (i32)
struct IseSelLayout {
  size_t part, out, total, hist, counts, words;
};
IseSelLayout ise_sel_layout(int64_t N) {
  IseSelLayout l{};
  l.part = 0;
  l.out = l.part + 3 * size_t(kIseKeyWg);
  l.total = l.out + 3;
  l.hist = l.total + 1;
  l.counts = l.hist + kPassBins / 2;
  l.words = l.counts + (size_t(N / 256 + 2) + 1) / 2;
  return l;
}

// The refusals the selection entry points share with sgp_grid_ise, before anything is launched
// or written; fills the key arguments.
int ise_key_args(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, IseKeyArgs* a) {
  sgp_ctx* ctx = g->ctx;
  SGP_CHECK(ctx, gps && fmin, "gps and fmin are required");
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS && G == g->G, "grid was created for %d GPs, got %d",
            g->G, G);
  unsigned active = 0;
  for (int q = 0; q < G; ++q)
    if (std::isfinite(fmin[q])) active |= 1u << q;
  SGP_CHECK(ctx, active != 0, "no GP is active: every fmin is infinite or NaN");
  SGP_CHECK(ctx, g->post_valid,
            "the grid holds no current posterior: run a confidence pass (sgp_grid_confidence "
            "/ sgp_grid_posterior) first");
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  a->var = g->var;
  a->S = g->S;
  a->N = g->N;
  a->G = G;
  a->active = active;
  for (int q = 0; q < G; ++q) a->s[q] = gps[q]->noise_var + 1e-8;
  return 0;
}

inline unsigned ise_key_blocks(int64_t N) {
  return unsigned(std::min<int64_t>((N + 255) / 256, kIseKeyWg));
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

// W = Ky^-1 k(X, x_j) of the K points xc [K][d] (device), [n_pad][Kp] with Kp a multiple of 64
// and W zeroed by the caller; T: [n][Kp] workspace (common.h).  The covariance-matrix kernel of
// the factorisation, then k_ise_fwd and k_ise_bwd: a column's sums run in an order that depends
// on n alone, so a column has the same bits whatever K, Kp or its position.
int launch_ise_operands(sgp_ctx* ctx, sgp_gp* gp, const double* xc, int K, int Kp, double* W,
                        double* T) {
  const int n = int(gp->n);
  const double* Linv = static_cast<const double*>(gp->Linv.p);
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, static_cast<const double*>(gp->X.p), n, xc, K, W,
                               Kp, 0, 0.0, INT64_MAX));
  const dim3 grid(unsigned(n), unsigned(Kp / 64));
  hipLaunchKernelGGL(k_ise_fwd, grid, dim3(256), 0, ctx->stream, Linv, int64_t(gp->ld), Kp, W, T);
  hipLaunchKernelGGL(k_ise_bwd, grid, dim3(256), 0, ctx->stream, Linv, int64_t(gp->ld), n, Kp, T,
                     W);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

namespace {

// The body of sgp_grid_ise, sgp_grid_ise_at and sgp_grid_ise_comm: the same operand kernels,
// k_ise_rows, k_ise_final and k_ise_pick.  by_value: the candidates' coordinates xc_host [K][d]
// and variances vx_host [G][K] come from the host and cand holds GLOBAL rows of the whole grid,
// read by the pick's tie rule and returned, nothing else; otherwise cand are rows of this shard
// and both are gathered from the resident arrays.  merge: the ranks' alpha | target blocks are
// all-gathered and merged in the grid's stream before the pick (a collective).
int grid_ise(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, const int64_t* cand,
             int K, int about, bool by_value, const double* xc_host, const double* vx_host,
             double* alpha, int64_t* target, double* value, int64_t* gidx, double* pairs,
             double* cov, bool merge) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  // ---- every refusal before anything is launched, staged or written
  SGP_CHECK(ctx, K >= 1 && K <= SGP_MAX_ISE, "K = %d candidates (1 .. SGP_MAX_ISE = %d)", K,
            SGP_MAX_ISE);
  SGP_CHECK(ctx, about == SGP_ISE_UNSAFE || about == SGP_ISE_ALL,
            "about = %d is not SGP_ISE_UNSAFE / SGP_ISE_ALL", about);
  SGP_CHECK(ctx, gps && fmin && cand && alpha && target && value && gidx,
            "gps, fmin, cand, alpha, target, value and gidx are required");
  SGP_CHECK(ctx, !by_value || (xc_host && vx_host), "xc and vx are required");
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS && G == g->G, "grid was created for %d GPs, got %d",
            g->G, G);
  const int64_t N = g->N;
  const int64_t goff = by_value ? 0 : g->goff;       // what the candidates' rows are relative to
  for (int j = 0; j < K; ++j) {
    if (by_value)
      SGP_CHECK(ctx, cand[j] >= 0, "candidate %d = row %lld is negative", j, (long long)cand[j]);
    else
      SGP_CHECK(ctx, cand[j] >= g->goff && cand[j] < g->goff + N,
                "candidate %d = row %lld is outside the shard [%lld, %lld)", j,
                (long long)cand[j], (long long)g->goff, (long long)(g->goff + N));
  }
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
  bool comm = false;
  if (merge) SGP_TRY(comm_or_single(ctx, &comm));
  const int world = comm ? ctx->world : 0;
  const IseLayout l = ise_layout(host, G, active, d, Kp, nwg, world);
  double *in, *wbuf, *part, *outb = nullptr;
  SGP_TRY(sgp_scratch(ctx, kSlotIseIn, l.in_words * 8, &in));
  SGP_TRY(sgp_scratch(ctx, kSlotIseW, l.w_words * 8, &wbuf));
  SGP_TRY(sgp_scratch(ctx, kSlotIsePart, l.part_words * 8, &part));
  const size_t pair_words = pairs ? size_t(K) * N : 0;
  const size_t cov_words = cov ? size_t(G) * K * N : 0;
  if (pairs || cov) SGP_TRY(sgp_scratch(ctx, kSlotIseOut, (pair_words + cov_words) * 8, &outb));

  int64_t* idx_dev = reinterpret_cast<int64_t*>(in + l.idx);
  if (by_value) {
    // ---- candidates by value: the whole block idx | xc | vx in one upload, zero in the padding
    std::vector<double> blk(l.in_words, 0.0);
    for (int j = 0; j < K; ++j) memcpy(&blk[l.idx + j], &cand[j], 8);
    memcpy(&blk[l.xc], xc_host, size_t(K) * d * 8);
    for (int q = 0; q < G; ++q)
      memcpy(&blk[l.vx + size_t(q) * Kp], vx_host + size_t(q) * K, size_t(K) * 8);
    SGP_TRY(sgp_h2d(ctx, in, blk.data(), l.in_words * 8));
  } else {
    // ---- candidates: local rows up, coordinates and variances gathered on the device
    std::vector<int64_t> idx(size_t(Kp), 0);
    for (int j = 0; j < K; ++j) idx[j] = cand[j] - g->goff;
    SGP_TRY(sgp_h2d(ctx, idx_dev, idx.data(), size_t(Kp) * 8));
    SGP_HIP(ctx, hipMemsetAsync(in + l.xc, 0, (l.in_words - l.xc) * 8, ctx->stream));
    hipLaunchKernelGGL(k_ise_gather, dim3(unsigned((K + 255) / 256)), dim3(256), 0, ctx->stream,
                       g->pts, g->var, N, d, G, idx_dev, K, Kp, in + l.xc, in + l.vx);
    SGP_HIP(ctx, hipGetLastError());
  }

  // ---- operands: W_g = L^-T (L^-1 k_g(X, x_j)), [n_pad][Kp], zero in the padding
  SGP_HIP(ctx, hipMemsetAsync(wbuf, 0, l.t * 8, ctx->stream));
  double flops = 0.0;
  for (int q = 0; q < G; ++q) {
    if (!((active >> q) & 1u)) continue;
    SGP_TRY(launch_ise_operands(ctx, gps[q], in + l.xc, K, Kp, wbuf + l.w[q], wbuf + l.t));
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
  SGP_HIP(ctx, hipGetLastError());
  if (comm) {
    // the ranks' alpha | target blocks (contiguous, 2 Kp words), merged candidate by candidate
    SGP_TRY(coll_allgather(ctx, alpha_dev, part + l.recs, 2 * size_t(Kp) * 8));
    alpha_dev = part + l.malpha;
    target_dev = reinterpret_cast<long long*>(part + l.mtarget);
    hipLaunchKernelGGL(k_ise_merge, dim3(unsigned((K + 255) / 256)), dim3(256), 0, ctx->stream,
                       part + l.recs, world, K, Kp, alpha_dev, target_dev);
  }
  // (alpha | target | res and malpha | mtarget | mres are laid out alike)
  hipLaunchKernelGGL(k_ise_pick, dim3(1), dim3(256), 0, ctx->stream, alpha_dev, target_dev,
                     idx_dev, K, goff, alpha_dev + 2 * size_t(Kp));
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

}  // namespace

int sgp_grid_ise(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, const int64_t* cand,
                 int K, int about, double* alpha, int64_t* target, double* value, int64_t* gidx,
                 double* pairs, double* cov) {
  return grid_ise(g, gps, G, fmin, cand, K, about, false, nullptr, nullptr, alpha, target, value,
                  gidx, pairs, cov, false);
}

int sgp_grid_ise_at(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin,
                    const int64_t* cand, const double* xc, const double* vx, int K, int about,
                    double* alpha, int64_t* target, double* value, int64_t* gidx) {
  return grid_ise(g, gps, G, fmin, cand, K, about, true, xc, vx, alpha, target, value, gidx,
                  nullptr, nullptr, false);
}

int sgp_grid_ise_comm(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin,
                      const int64_t* cand, const double* xc, const double* vx, int K, int about,
                      double* alpha, int64_t* target, double* value, int64_t* gidx) {
  return grid_ise(g, gps, G, fmin, cand, K, about, true, xc, vx, alpha, target, value, gidx,
                  nullptr, nullptr, true);
}

// ---- candidate selection ------------------------------------------------------------------------
int sgp_grid_ise_keys(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, int64_t* count,
                      double* key_min, double* key_max) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, count && key_min && key_max, "count, key_min and key_max are required");
  IseKeyArgs a{};
  SGP_TRY(ise_key_args(g, gps, G, fmin, &a));
  const IseSelLayout l = ise_sel_layout(g->N);
  double* w;
  SGP_TRY(sgp_scratch(ctx, kSlotIsePart, l.words * 8, &w));
  const unsigned nwg = ise_key_blocks(g->N);
  hipLaunchKernelGGL(k_ise_keys, dim3(nwg), dim3(256), 0, ctx->stream, a, w + l.part);
  hipLaunchKernelGGL(k_ise_keys_final, dim3(1), dim3(256), 0, ctx->stream, w + l.part, int(nwg),
                     w + l.out);
  SGP_HIP(ctx, hipGetLastError());
  double h[3];
  SGP_TRY(sgp_d2h(ctx, h, w + l.out, sizeof(h)));
  *count = int64_t(h[0]);
  *key_min = h[1];
  *key_max = h[2];
  return 0;
}

int sgp_grid_ise_hist(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, double key_lo,
                      double key_hi, uint32_t* hist) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, hist, "hist is required");
  SGP_CHECK(ctx, std::isfinite(key_lo) && std::isfinite(key_hi) && key_hi > key_lo,
            "empty key range %g .. %g", key_lo, key_hi);
  IseKeyArgs a{};
  SGP_TRY(ise_key_args(g, gps, G, fmin, &a));
  const IseSelLayout l = ise_sel_layout(g->N);
  double* w;
  SGP_TRY(sgp_scratch(ctx, kSlotIsePart, l.words * 8, &w));
  unsigned* hist_dev = reinterpret_cast<unsigned*>(w + l.hist);
  SGP_HIP(ctx, hipMemsetAsync(hist_dev, 0, kPassBins * sizeof(unsigned), ctx->stream));
  hipLaunchKernelGGL(k_ise_hist, dim3(ise_key_blocks(g->N)), dim3(256), 0, ctx->stream, a, key_lo,
                     key_hi, hist_dev);
  SGP_HIP(ctx, hipGetLastError());
  return sgp_d2h(ctx, hist, hist_dev, kPassBins * sizeof(uint32_t));
}

int sgp_grid_ise_list(sgp_grid* g, sgp_gp* const* gps, int G, const double* fmin, double thr,
                      int cap, int64_t* count, int64_t* gidx, double* key, double* x,
                      double* var) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, count, "count is required");
  SGP_CHECK(ctx, cap >= 0 && (cap == 0 || (gidx && key && x && var)),
            "cap = %d rows need gidx, key, x and var", cap);
  SGP_CHECK(ctx, !std::isnan(thr), "the threshold is NaN");
  SGP_CHECK(ctx, g->N < (int64_t(1) << 31), "%lld rows", (long long)g->N);
  IseKeyArgs a{};
  SGP_TRY(ise_key_args(g, gps, G, fmin, &a));
  const int64_t N = g->N;
  const int d = g->d, words = 2 + d + G;
  const IseSelLayout l = ise_sel_layout(N);
  double *w, *rec = nullptr;
  SGP_TRY(sgp_scratch(ctx, kSlotIsePart, l.words * 8, &w));
  // (at most min(cap, N) records are written, whatever the count)
  const int room = int(std::min<int64_t>(cap, N));
  if (room) SGP_TRY(sgp_scratch(ctx, kSlotIseIn, size_t(room) * words * 8, &rec));
  int* counts = reinterpret_cast<int*>(w + l.counts);
  long long* total = reinterpret_cast<long long*>(w + l.total);
  const int nchunks = int((N + 255) / 256);
  const unsigned nb = unsigned(std::min(nchunks, 2048));
  hipLaunchKernelGGL(k_ise_count, dim3(nb), dim3(256), 0, ctx->stream, a, thr, counts);
  hipLaunchKernelGGL(k_ise_scan, dim3(1), dim3(1024), 0, ctx->stream, counts, nchunks, total);
  if (room)
    hipLaunchKernelGGL(k_ise_fill, dim3(nb), dim3(256), 0, ctx->stream, a, g->pts, d, g->goff,
                       thr, counts, room, rec);
  SGP_HIP(ctx, hipGetLastError());
  long long n = 0;
  SGP_TRY(sgp_d2h(ctx, &n, total, 8));
  *count = n;
  const size_t m = size_t(std::min<long long>(n, room));
  if (m == 0) return 0;
  std::vector<double> host(m * words);
  SGP_TRY(sgp_d2h(ctx, host.data(), rec, host.size() * 8));
  for (size_t p = 0; p < m; ++p) {
    const double* r = &host[p * words];
    memcpy(&gidx[p], r, 8);
    key[p] = r[1];
    memcpy(x + p * d, r + 2, size_t(d) * 8);
    memcpy(var + p * G, r + 2 + d, size_t(G) * 8);
  }
  return 0;
}
