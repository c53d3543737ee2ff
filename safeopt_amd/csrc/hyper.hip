// Log marginal likelihood of a fitted GP and its gradient in the hyper-parameters.
//
// What GPy's ExactGaussianInference + Stationary.update_gradients_full do behind
// gp.log_likelihood() / gp.optimize(), from what factor_gp leaves on the device (the dense
// L^-1 of Ky = K + (noise + 1e-8 + jitter) I, alpha = Ky^-1 y, the raw X and Y):
//
//   log p(y) = -1/2 y^T alpha - sum_i log L_ii - n/2 log 2 pi,   L_ii = 1 / (L^-1)_ii
//   d/dtheta = 1/2 sum_ij W_ij dKy_ij/dtheta,   W = alpha alpha^T - Ky^-1,
//   Ky^-1    = L^-T L^-1:  (Ky^-1)_ij = sum_{k >= max(i, j)} (L^-1)_ki (L^-1)_kj
//
// With s = inv_ls[p][a], D_a = x_ia - x_ja, r_p^2 = sum_a (D_a s_pa)^2, k = prod_p v_p f_p(r_p):
//   dk/dv_p  = k / v_p                      -> one accumulator  sum W k  serves every v_p
//   dk/ds_pa = (k / f_p) c_p(r_p) D_a^2 s_pa   (exact at r = 0, no division by r)
//     RBF        c = -exp(-r^2 / 2)
//     Matern-3/2 c = -3 exp(-sqrt(3) r)
//     Matern-5/2 c = -(5/3) (1 + sqrt(5) r) exp(-sqrt(5) r)
//   dKy/dnoise = I  (diag(r) for a GP with noise scales: sgp_gp::rhost)
//
// k_lml_tiles: one workgroup per lower-triangular 64 x 64 tile of the (i, j) pairs.  Its four
// waves form the tile of Ky^-1 on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: the A and
// the B operand are both rows of the dense L^-1, 16 consecutive doubles per k -- no packing)
// and contract it in registers with the evaluated derivative tile: neither Ky^-1 nor any
// dK/dtheta reaches memory.  Off-diagonal tiles count twice.  Every tile writes its
// 2 + P d sums to a slot of its own; k_lml_final adds the slots in a fixed order (no
// floating-point atomics: the same theta gives the same bits) together with the log and
// y^T alpha terms and writes the result block.
//
// The leave-one-out predictions, their log pseudo-likelihood and its gradient
// (sgp_gp_loo, sgp_gp_loo_lml) come from the same resident data: see "leave-one-out" below.
#include "kern_eval.h"

namespace {

constexpr int kTile = 64;
constexpr int kMaxAcc = 2 + SGP_MAX_PARTS * SGP_MAX_D;   // noise | sum W k | [p][a]

__host__ __device__ inline int lml_words(int n_parts, int d) { return 2 + n_parts + n_parts * d; }

// f_p(r) and c_p(r) of one part
__device__ __forceinline__ void part_eval(int kind, double r2, double* f, double* c) {
  if (kind == SGP_RBF) {
    const double e = exp(-0.5 * r2);
    *f = e;
    *c = -e;
    return;
  }
  const double r = sqrt(r2);
  if (kind == SGP_MATERN32) {
    const double a = 1.7320508075688772 * r;
    const double e = exp(-a);
    *f = (1.0 + a) * e;
    *c = -3.0 * e;
    return;
  }
  const double a = 2.23606797749979 * r;
  const double e = exp(-a);
  *f = (1.0 + a + (5.0 / 3.0) * r2) * e;
  *c = -(5.0 / 3.0) * (1.0 + a) * e;
}

// tile t of the lower triangle, row-major: (0,0) (1,0) (1,1) (2,0) ...
__device__ __forceinline__ void tile_of(int t, int* ti, int* tj) {
  int i = int((sqrt(8.0 * double(t) + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  while (i * (i + 1) / 2 > t) --i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

// acc[q] += sum_k M_k,i0+. M_k,j0+16q+. over k = k_begin .. n - 1 on the matrix cores: the
// wave's 16 rows i0 .. i0 + 15 x 64 columns j0 .. of M^T M, M dense row-major with pitch ld.
// Both operands of a k-step are 16 consecutive doubles of row k (lane: column `col`, k-step
// row `kq`).  Rows k >= n and columns >= n are never read (a bordered update may have left
// anything there).  The one copy of the operand layout: k_lml_tiles and k_loo_kinv.
__device__ __forceinline__ void mtm_tile(const double* __restrict__ M, int64_t ld, int n,
                                         int i0, int j0, int col, int kq, int k_begin,
                                         double4_t (&acc)[4]) {
  const bool a_ok = i0 + col < n;
  bool b_ok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) b_ok[q] = j0 + 16 * q + col < n;
  constexpr int kInFlight = 4;           // k-steps whose loads are issued before the first use
  for (int k0 = k_begin; k0 < n; k0 += 4 * kInFlight) {
    double av[kInFlight], bv[kInFlight][4];
#pragma unroll
    for (int s = 0; s < kInFlight; ++s) {
      const int k = k0 + 4 * s + kq;
      const double* row = M + int64_t(k) * ld;
      const bool ok = k < n;
      av[s] = (ok && a_ok) ? row[i0 + col] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[s][q] = (ok && b_ok[q]) ? row[j0 + 16 * q + col] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < kInFlight; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s][q], acc[q], 0, 0, 0);
  }
}

// LOO = true (sgp_gp_loo_lml): the same tile loop and the same contraction with the weight
// of the leave-one-out pseudo-likelihood, G = 1/2 (u alpha^T + alpha u^T) - C^T C.  `Li` is
// then C = diag(sqrt(b)) Ky^-1 (k_loo_kinv), a FULL matrix: (C^T C)_ij = sum_k C_ki C_kj
// over every k, both operands again 16 consecutive doubles of row k.  LOO = false is the
// kernel as it was (`u` unused).
template <int D, bool LOO>
__global__ __launch_bounds__(256) void k_lml_tiles(KernDesc kd, const double* __restrict__ Li,
                                                   int64_t ld, int n,
                                                   const double* __restrict__ X,
                                                   const double* __restrict__ alpha,
                                                   const double* __restrict__ u,
                                                   const double* __restrict__ rs,
                                                   double* __restrict__ part) {
  __shared__ double sh[4][kMaxAcc];
  int ti, tj;
  tile_of(blockIdx.x, &ti, &tj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = ti * kTile + 16 * wave, j0 = tj * kTile;
  const int col = lane & 15, kq = lane >> 4;

  // ---- Ky^-1 tile: rows i0 .. i0 + 15 of this wave x 64 columns ---------------------------
  // (L^-1)_ki = 0 for k < i: the sum starts at the wave's first row (C is full: at 0).
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  mtm_tile(Li, ld, n, i0, j0, col, kq, LOO ? 0 : i0, acc);

  // ---- contraction with the derivative tile ------------------------------------------------
  // D layout: column j = j0 + 16 q + (lane & 15), rows i = i0 + (lane >> 4) + 4 r
  double s_noise = 0.0, s_k = 0.0;
  double s_ls[SGP_MAX_PARTS][D];
#pragma unroll
  for (int p = 0; p < SGP_MAX_PARTS; ++p)
#pragma unroll
    for (int a = 0; a < D; ++a) s_ls[p][a] = 0.0;
  double vprod = 1.0;
  for (int p = 0; p < kd.n_parts; ++p) vprod *= kd.variance[p];

  double xi[4][D], ai[4], ui[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + kq + 4 * r;
    ai[r] = i < n ? alpha[i] : 0.0;
    if constexpr (LOO) ui[r] = i < n ? 0.5 * u[i] : 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) xi[r][a] = i < n ? X[int64_t(i) * D + a] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + 16 * q + col;
    double xj[D];
    const double aj = j < n ? alpha[j] : 0.0;
    double uj = 0.0;
    if constexpr (LOO) uj = j < n ? 0.5 * u[j] : 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) xj[a] = j < n ? X[int64_t(j) * D + a] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + kq + 4 * r;
      if (i >= n || j >= n) continue;
      double w;
      if constexpr (LOO) {
        w = fma(ui[r], aj, fma(ai[r], uj, -acc[q][r]));
      } else {
        w = fma(ai[r], aj, -acc[q][r]);
      }
      if (i == j) s_noise += rs ? w * rs[i] : w;    // dKy/dnoise = diag(r)
      double d2[D];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const double t = xi[r][a] - xj[a];
        d2[a] = t * t;
      }
      double f[SGP_MAX_PARTS], c[SGP_MAX_PARTS];
#pragma unroll
      for (int p = 0; p < SGP_MAX_PARTS; ++p) {
        f[p] = 1.0;
        c[p] = 0.0;
        if (p < kd.n_parts) {
          double r2 = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) r2 = fma(d2[a], kd.inv_ls[p][a] * kd.inv_ls[p][a], r2);
          part_eval(kd.kind[p], r2, &f[p], &c[p]);
        }
      }
      const double wv = w * vprod;
      s_k = fma(wv, (f[0] * f[1]) * (f[2] * f[3]), s_k);
#pragma unroll
      for (int p = 0; p < SGP_MAX_PARTS; ++p) {
        if (p < kd.n_parts) {
          double others = 1.0;           // k / f_p without dividing (f_p may underflow)
#pragma unroll
          for (int o = 0; o < SGP_MAX_PARTS; ++o)
            if (o != p) others *= f[o];
          const double h = wv * others * c[p];
#pragma unroll
          for (int a = 0; a < D; ++a) s_ls[p][a] = fma(h, d2[a], s_ls[p][a]);
        }
      }
    }
  }

  // ---- lanes -> wave -> workgroup, fixed order ------------------------------------------------
  auto wave_sum = [](double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  s_noise = wave_sum(s_noise);
  s_k = wave_sum(s_k);
  if (lane == 0) {
    sh[wave][0] = s_noise;
    sh[wave][1] = s_k;
  }
#pragma unroll
  for (int p = 0; p < SGP_MAX_PARTS; ++p) {
    if (p < kd.n_parts) {
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const double v = wave_sum(s_ls[p][a]);
        if (lane == 0) sh[wave][2 + p * D + a] = v;
      }
    }
  }
  __syncthreads();
  const int nacc = 2 + kd.n_parts * D;
  if (int(threadIdx.x) < nacc) {
    const int t = threadIdx.x;
    const double v = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
    part[int64_t(blockIdx.x) * kMaxAcc + t] = (ti == tj) ? v : 2.0 * v;
  }
}

// Sum of v over the 256 threads of the workgroup, the same tree every time.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (int(threadIdx.x) < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// out = [ log p | d/dnoise | d/dv_p | d/dinv_ls[p][a] | info ]  (info as a double)
__global__ __launch_bounds__(256) void k_lml_final(KernDesc kd, const double* __restrict__ Li,
                                                   int64_t ld, int n,
                                                   const double* __restrict__ Y,
                                                   const double* __restrict__ alpha,
                                                   const double* __restrict__ part, int ntiles,
                                                   const int* __restrict__ info,
                                                   double* __restrict__ out) {
  __shared__ double sh[256];
  const int t = threadIdx.x, P = kd.n_parts, d = kd.d;
  double ya = 0.0, lg = 0.0;
  for (int i = t; i < n; i += 256) {
    ya = fma(Y[i], alpha[i], ya);
    lg += log(Li[int64_t(i) * ld + i]);        // = -log L_ii
  }
  ya = block_sum(ya, sh);
  lg = block_sum(lg, sh);
  if (t == 0) {
    out[0] = -0.5 * ya + lg - 0.5 * double(n) * 1.8378770664093453;   // log 2 pi
    out[lml_words(P, d)] = double(*info);
  }
  const int nacc = 2 + P * d;
  for (int a = 0; a < nacc; ++a) {
    double s = 0.0;
    for (int b = t; b < ntiles; b += 256) s += part[int64_t(b) * kMaxAcc + a];
    s = block_sum(s, sh);
    if (t == 0) {
      if (a == 0) {
        out[1] = 0.5 * s;
      } else if (a == 1) {
        for (int p = 0; p < P; ++p) out[2 + p] = 0.5 * s / kd.variance[p];
      } else {
        const int p = (a - 2) / d, c = (a - 2) % d;
        out[2 + P + p * d + c] = 0.5 * s * kd.inv_ls[p][c];
      }
    }
  }
}

// ---- leave-one-out ---------------------------------------------------------------------------
// From the same resident L^-1 and alpha (Rasmussen & Williams 5.4.2), all i together:
//   P_ii = (Ky^-1)_ii = sum_{k >= i} (L^-1)_ki^2,   mu_-i = y_i - alpha_i / P_ii,
//   var_-i = 1 / P_ii (of the noisy y_i),           z_i = alpha_i / sqrt(P_ii),
//   L_LOO = sum_i [ 1/2 log P_ii - 1/2 z_i^2 - 1/2 log 2 pi ]
//   dL_LOO/dtheta = sum_ij G_ij dKy_ij/dtheta,  G = 1/2 (u alpha^T + alpha u^T) - C^T C,
//   a_i = alpha_i / P_ii,  b_i = 1/2 (1 + z_i^2) / P_ii,  u = Ky^-1 a,  C = diag(sqrt(b)) Ky^-1
// k_loo_diag -> k_loo_cols -> k_loo_sum give the predictions (one pass over the lower
// triangle of L^-1, no row or column >= n and nothing above the diagonal is read: this also
// runs on a factor that bordered updates and removals have left); the gradient adds two
// triangular mat-vecs (u), k_loo_kinv (C, on the matrix cores), k_lml_tiles<D, true> and
// k_loo_final.  Every sum has a fixed order.
constexpr int kLooChunk = 128;          // rows of L^-1 per workgroup of k_loo_diag

// The vectors of a LOO call (kSlotLooVec), np = n rounded up to 64:
//   [chunks][np] partial column sums | a | sqrt(b) | t | u | mean | var | [sum, info] | terms
//   | flags (int)
struct LooVec {
  double *ppart, *a, *sb, *t, *u, *mean, *var, *tail, *term;
  int* flag;
  int np, chunks;
};
inline int loo_chunks(int n) { return (n + kLooChunk - 1) / kLooChunk; }
inline size_t loo_vec_bytes(int n) {
  const size_t np = size_t((n + 63) / 64) * 64;
  return (size_t(loo_chunks(n)) + 7) * np * sizeof(double) + 2 * sizeof(double) +
         np * sizeof(int);
}
inline LooVec loo_vec(double* b, int n) {
  LooVec v;
  v.np = (n + 63) / 64 * 64;
  v.chunks = loo_chunks(n);
  v.ppart = b;
  v.a = v.ppart + size_t(v.chunks) * v.np;
  v.sb = v.a + v.np;
  v.t = v.sb + v.np;
  v.u = v.t + v.np;
  v.mean = v.u + v.np;
  v.var = v.mean + v.np;
  v.tail = v.var + v.np;
  v.term = v.tail + 2;
  v.flag = reinterpret_cast<int*>(v.term + v.np);
  return v;
}

// Partial column sums of squares: workgroup (x, y) takes columns 64 x .. 64 x + 63 (one per
// lane: a row load is 512 contiguous bytes) and rows kLooChunk y .. of chunk y, its four
// waves every fourth row.  ppart[y][j] is written for every j < np (0 where the chunk lies
// above the diagonal).
__global__ __launch_bounds__(256) void k_loo_diag(const double* __restrict__ Li, int64_t ld,
                                                  int n, int np, double* __restrict__ ppart) {
  __shared__ double sh[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64, j = j0 + lane;
  const int r0 = blockIdx.y * kLooChunk, r1 = min(r0 + kLooChunk, n);
  double s0 = 0.0, s1 = 0.0;
  if (j < n && r1 > j0) {
    // (rows in front of the column block's first hold nothing of it)
    int k = r0 + wave;
    if (k < j0) k += (j0 - k + 3) / 4 * 4;
    for (; k + 4 < r1; k += 8) {
      const double v0 = k >= j ? Li[int64_t(k) * ld + j] : 0.0;
      const double v1 = k + 4 >= j ? Li[int64_t(k + 4) * ld + j] : 0.0;
      s0 = fma(v0, v0, s0);
      s1 = fma(v1, v1, s1);
    }
    if (k < r1) {
      const double v0 = k >= j ? Li[int64_t(k) * ld + j] : 0.0;
      s0 = fma(v0, v0, s0);
    }
  }
  sh[wave][lane] = s0 + s1;
  __syncthreads();
  if (wave == 0 && j < np)
    ppart[int64_t(blockIdx.y) * np + j] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

// Per observation: P_ii (the chunks in their order), the prediction, a, sqrt(b), the term of
// L_LOO, and the flag of a P_ii that is not positive and finite (everything of it 0 then).
__global__ __launch_bounds__(256) void k_loo_cols(int n, const double* __restrict__ Y,
                                                  const double* __restrict__ alpha, LooVec v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= v.np) return;
  double mean = 0.0, var = 0.0, a = 0.0, sb = 0.0, term = 0.0;
  int flag = 0;
  if (i < n) {
    double P = 0.0;
    for (int c = i / kLooChunk; c < v.chunks; ++c) P += v.ppart[int64_t(c) * v.np + i];
    if (P > 0.0 && isfinite(P)) {
      const double al = alpha[i];
      a = al / P;
      const double z2 = al * a;
      mean = Y[i] - a;
      var = 1.0 / P;
      sb = sqrt(0.5 * (1.0 + z2) / P);
      term = 0.5 * log(P) - 0.5 * z2 - 0.5 * 1.8378770664093453;   // log 2 pi
    } else {
      flag = 1;
    }
  }
  v.mean[i] = mean;
  v.var[i] = var;
  v.a[i] = a;
  v.sb[i] = sb;
  v.term[i] = term;
  v.flag[i] = flag;
}

// first flagged observation, 1-based, or 0: the same tree every time
__device__ __forceinline__ int block_first(const int* flag, int n, int* shi) {
  int first = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += 256)
    if (flag[i] && i < first) first = i;
  __syncthreads();
  shi[threadIdx.x] = first;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (int(threadIdx.x) < o) shi[threadIdx.x] = min(shi[threadIdx.x], shi[threadIdx.x + o]);
    __syncthreads();
  }
  return shi[0] == 0x7fffffff ? 0 : shi[0] + 1;
}

// tail = [ L_LOO | info ]
__global__ __launch_bounds__(256) void k_loo_sum(int n, LooVec v) {
  __shared__ double sh[256];
  __shared__ int shi[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += v.term[i];
  s = block_sum(s, sh);
  const int bad = block_first(v.flag, n, shi);
  if (threadIdx.x == 0) {
    v.tail[0] = s;
    v.tail[1] = double(bad);
  }
}

// C = diag(sqrt(b)) Ky^-1, n x n with pitch ldc: one workgroup per lower 64 x 64 tile forms
// the tile of Ky^-1 with the loop of k_lml_tiles and writes it scaled by its rows' sqrt(b),
// and -- off the diagonal -- its transpose, scaled by the columns', through LDS so that both
// stores run along rows of C.
__global__ __launch_bounds__(256) void k_loo_kinv(const double* __restrict__ Li, int64_t ld,
                                                  int n, const double* __restrict__ sb,
                                                  double* __restrict__ Cm, int64_t ldc) {
  __shared__ double sh[kTile][kTile + 1];
  int ti, tj;
  tile_of(blockIdx.x, &ti, &tj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = ti * kTile + 16 * wave, j0 = tj * kTile;
  const int col = lane & 15, kq = lane >> 4;
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  mtm_tile(Li, ld, n, i0, j0, col, kq, i0, acc);      // (L^-1)_ki = 0 for k < i
  // D layout: column j = j0 + 16 q + (lane & 15), rows i = i0 + (lane >> 4) + 4 r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int li = 16 * wave + kq + 4 * r, i = ti * kTile + li;
    const double si = i < n ? sb[i] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lj = 16 * q + col, j = j0 + lj;
      if (i < n && j < n) Cm[int64_t(i) * ldc + j] = si * acc[q][r];
      sh[lj][li] = acc[q][r];
    }
  }
  if (ti == tj) return;                  // (uniform: the tile is already whole)
  __syncthreads();
  for (int rr = 0; rr < 16; ++rr) {
    const int lj = 16 * wave + rr, j = j0 + lj, i = ti * kTile + lane;
    if (j < n && i < n) Cm[int64_t(j) * ldc + i] = sb[j] * sh[lj][lane];
  }
}

// out = [ L_LOO | d/dnoise | d/dv_p | d/dinv_ls[p][a] | info ]: the slots in k_lml_final's
// order; info = the factorisation's pivot word, else the first P_ii that is not positive.
__global__ __launch_bounds__(256) void k_loo_final(KernDesc kd, const double* __restrict__ part,
                                                   int ntiles, const double* __restrict__ tail,
                                                   const int* __restrict__ info,
                                                   double* __restrict__ out) {
  __shared__ double sh[256];
  const int t = threadIdx.x, P = kd.n_parts, d = kd.d;
  if (t == 0) {
    out[0] = tail[0];
    out[lml_words(P, d)] = *info != 0 ? double(*info) : tail[1];
  }
  const int nacc = 2 + P * d;
  for (int a = 0; a < nacc; ++a) {
    double s = 0.0;
    for (int b = t; b < ntiles; b += 256) s += part[int64_t(b) * kMaxAcc + a];
    s = block_sum(s, sh);
    if (t == 0) {
      if (a == 0) {
        out[1] = s;
      } else if (a == 1) {
        for (int p = 0; p < P; ++p) out[2 + p] = s / kd.variance[p];
      } else {
        const int p = (a - 2) / d, c = (a - 2) % d;
        out[2 + P + p * d + c] = s * kd.inv_ls[p][c];
      }
    }
  }
}

// k_loo_diag .. k_loo_sum on the resident factor; *v: where the results lie
int enqueue_loo(sgp_gp* gp, LooVec* v) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n);
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotLooVec, loo_vec_bytes(n), &buf));
  *v = loo_vec(buf, n);
  const double* Li = static_cast<const double*>(gp->Linv.p);
  hipLaunchKernelGGL(k_loo_diag, dim3(v->np / 64, v->chunks), dim3(256), 0, ctx->stream, Li,
                     int64_t(gp->ld), n, v->np, v->ppart);
  SGP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_loo_cols, dim3((v->np + 255) / 256), dim3(256), 0, ctx->stream, n,
                     static_cast<const double*>(gp->Y.p),
                     static_cast<const double*>(gp->alpha.p), *v);
  SGP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_loo_sum, dim3(1), dim3(256), 0, ctx->stream, n, *v);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

}  // namespace

int lml_result_words(const KernDesc& kd) { return lml_words(kd.n_parts, kd.d) + 1; }

// Enqueues the two kernels on a GP that factor_gp has just factorised (deferred pivot check:
// `info_dev` is the factorisation's pivot word, copied into the result block); `out_dev` has
// lml_result_words doubles.
int launch_lml(sgp_gp* gp, const int* info_dev, double* out_dev) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n);
  const int nt = (n + kTile - 1) / kTile;
  const int ntiles = nt * (nt + 1) / 2;
  double* part;
  SGP_TRY(sgp_scratch(ctx, kSlotPartials, size_t(ntiles) * kMaxAcc * sizeof(double), &part));
  const double* Li = static_cast<const double*>(gp->Linv.p);
  const double* X = static_cast<const double*>(gp->X.p);
  const double* Y = static_cast<const double*>(gp->Y.p);
  const double* alpha = static_cast<const double*>(gp->alpha.p);
  const double* rs = gp->rhost.empty() ? nullptr : static_cast<const double*>(gp->R.p);
#define LML_CASE(DD)                                                                       \
  case DD:                                                                                 \
    hipLaunchKernelGGL((k_lml_tiles<DD, false>), dim3(ntiles), dim3(256), 0, ctx->stream,  \
                       gp->kern, Li, int64_t(gp->ld), n, X, alpha,                         \
                       static_cast<const double*>(nullptr), rs, part);                     \
    break;
  switch (gp->kern.d) {
    LML_CASE(1) LML_CASE(2) LML_CASE(3) LML_CASE(4)
    LML_CASE(5) LML_CASE(6) LML_CASE(7) LML_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", gp->kern.d, SGP_MAX_D);
      return -2;
  }
#undef LML_CASE
  SGP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_lml_final, dim3(1), dim3(256), 0, ctx->stream, gp->kern, Li,
                     int64_t(gp->ld), n, Y, alpha, part, ntiles, info_dev, out_dev);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// mean | var (np doubles each, np = n rounded up to 64) | L_LOO | info behind each other on the
// device, from the factor as it stands: *out_dev points at them.
int launch_loo(sgp_gp* gp, const double** out_dev, int* np) {
  LooVec v;
  SGP_TRY(enqueue_loo(gp, &v));
  *out_dev = v.mean;
  *np = v.np;
  return 0;
}

// The LOO objective and gradient of a GP that factor_gp has just factorised, in the result
// block of launch_lml.  Garbage in, garbage out after a failed pivot (the pivot word says so).
int launch_loo_lml(sgp_gp* gp, const int* info_dev, double* out_dev) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n);
  const int nt = (n + kTile - 1) / kTile;
  const int ntiles = nt * (nt + 1) / 2;
  const int64_t ldc = int64_t(nt) * kTile;
  LooVec v;
  SGP_TRY(enqueue_loo(gp, &v));
  double* part;
  double* Cm;
  SGP_TRY(sgp_scratch(ctx, kSlotPartials, size_t(ntiles) * kMaxAcc * sizeof(double), &part));
  SGP_TRY(sgp_scratch(ctx, kSlotLooC, size_t(ldc) * size_t(n) * sizeof(double), &Cm));
  const double* Li = static_cast<const double*>(gp->Linv.p);
  const double* X = static_cast<const double*>(gp->X.p);
  const double* alpha = static_cast<const double*>(gp->alpha.p);
  const double* rs = gp->rhost.empty() ? nullptr : static_cast<const double*>(gp->R.p);
  // u = L^-T (L^-1 a)
  SGP_TRY(tri_mv_dense(ctx, Li, gp->ld, n, v.a, 0, 1, v.t, 0));
  SGP_TRY(tri_mtv_dense(ctx, Li, gp->ld, n, v.t, 0, 1, v.u, 0, n));
  hipLaunchKernelGGL(k_loo_kinv, dim3(ntiles), dim3(256), 0, ctx->stream, Li, int64_t(gp->ld),
                     n, v.sb, Cm, ldc);
  SGP_HIP(ctx, hipGetLastError());
#define LOO_CASE(DD)                                                                      \
  case DD:                                                                                \
    hipLaunchKernelGGL((k_lml_tiles<DD, true>), dim3(ntiles), dim3(256), 0, ctx->stream,  \
                       gp->kern, Cm, ldc, n, X, alpha, v.u, rs, part);                    \
    break;
  switch (gp->kern.d) {
    LOO_CASE(1) LOO_CASE(2) LOO_CASE(3) LOO_CASE(4)
    LOO_CASE(5) LOO_CASE(6) LOO_CASE(7) LOO_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", gp->kern.d, SGP_MAX_D);
      return -2;
  }
#undef LOO_CASE
  SGP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_loo_final, dim3(1), dim3(256), 0, ctx->stream, gp->kern, part, ntiles,
                     v.tail, info_dev, out_dev);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
