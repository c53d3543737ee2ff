// GP "set_XY" on the device: kernel matrix, Cholesky, L^-1, alpha.
//
// Replaces what GPy's ExactGaussianInference does behind gp.set_XY
// (safeopt/gp_opt.py:227, 267, 275):  Ky = k(X,X) + (noise + 1e-8) I,
// L = jitchol(Ky), Ky^-1 via the triangular inverse, alpha = Ky^-1 y.
// n <= a few thousand, so n^3/3 <= ~3 GFLOP: a recursive blocked algorithm
// (32x32 leaves in LDS + one tiled fp64 GEMM kernel) is launch-bound, not
// flop-bound, and runs replicated on every GPU (no communication).
// Also here: the one-row updates behind sgp_gp_append / _pop / _remove and the posterior of
// a FEW points (small_path.h).  (The operands of the expander test: expander.hip.)
//
//   factor(A[0:s]):  s == 32 -> leaf (potf2 + triangular inverse in LDS)
//     else split h:  factor(A11); L21 = A21 Linv11^T; A22 -= L21 L21^T;
//                    factor(A22); Linv21 = -Linv22 (L21 Linv11)
#include <algorithm>
#include "small_path.h"

#include "kern_eval.h"
#include "sets_front.h"

namespace {

constexpr int NB = 32;  // leaf size

// ---- covariance matrix --------------------------------------------------------
// out[i*ld + j] = k(X1_i, X2_j) (+ diag_add on i == j when symmetric_diag; diag_vec != null:
// + diag_vec[i] instead, the diagonal of a GP with noise scales -- one addend chosen, one
// addition, so that equal addends give equal bits).
// Rows/cols >= n_valid (padding of a square factorisation matrix) become the
// identity so the padded Cholesky stays well defined.
template <int D>
__global__ void k_kernel_matrix(KernDesc kd, const double* X1, int64_t n1,
                                const double* X2, int64_t n2, double* out,
                                int64_t ld, int symmetric_diag, double diag_add,
                                int64_t n_valid, const double* diag_vec) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t i = int64_t(blockIdx.y) * blockDim.y + threadIdx.y;
  if (i >= n1 || j >= n2) return;
  double v;
  if (i >= n_valid || j >= n_valid) {
    v = (i == j) ? 1.0 : 0.0;
  } else {
    double a[D], b[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      a[k] = X1[i * D + k];
      b[k] = X2[j * D + k];
    }
    v = kern_eval<D>(kd, a, b);
    if (symmetric_diag && i == j) {
      const double add = diag_vec ? diag_vec[i] : diag_add;
      v += add;
    }
  }
  out[i * ld + j] = v;
}

// The diagonal addends of a GP with noise scales: s r_i + jitter (at r_i = 1 the bits of the
// scalar s + jitter of a GP without scales).
__global__ void k_scaled_diag(double* out, int n, const double* r, double s, double jitter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fma(s, r[i], jitter);
}

// ---- leaf: 32x32 Cholesky + inverse of the factor, one workgroup --------------
// A (ld) holds the symmetric block (lower part used); on exit A's lower part is
// L, and Linv (ldi) receives L^-1 (lower).  info[0] = first bad pivot (1-based,
// offset by `row0`) if a pivot is not positive / not finite.
__global__ __launch_bounds__(256) void k_leaf(double* A, int64_t ld,
                                              double* Linv, int64_t ldi,
                                              int row0, int* info) {
  __shared__ double a[NB][NB + 1];
  __shared__ double inv[NB][NB + 1];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e / NB, j = e % NB;
    a[i][j] = (j <= i) ? A[i * ld + j] : 0.0;
    inv[i][j] = 0.0;
  }
  __syncthreads();
  for (int k = 0; k < NB; ++k) {
    const double piv = a[k][k];
    if (!(piv > 0.0) || !isfinite(piv)) {
      if (tid == 0 && bad == 0) bad = row0 + k + 1;
      __syncthreads();
      break;
    }
    const double dk = sqrt(piv);
    __syncthreads();
    if (tid == 0) a[k][k] = dk;
    if (tid > k && tid < NB) a[tid][k] /= dk;
    __syncthreads();
    // trailing update: a[i][j] -= a[i][k] a[j][k], k < j <= i
    for (int e = tid; e < NB * NB; e += 256) {
      const int i = e / NB, j = e % NB;
      if (j > k && j <= i) a[i][j] -= a[i][k] * a[j][k];
    }
    __syncthreads();
  }
  if (bad != 0) {
    if (tid == 0) atomicCAS(info, 0, bad);
    return;
  }
  // inverse by forward substitution, one column per thread
  if (tid < NB) {
    const int j = tid;
    for (int i = j; i < NB; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= a[i][k] * inv[k][j];
      inv[i][j] = s / a[i][i];
    }
  }
  __syncthreads();
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e / NB, j = e % NB;
    if (j <= i) {
      A[i * ld + j] = a[i][j];
      Linv[i * ldi + j] = inv[i][j];
    }
  }
}

// ---- tiled fp64 GEMM: C = alpha * A * op(B) + beta * C ------------------------
// Row-major, 64x64 tile per workgroup, 4x4 micro-tile per thread, K step 16.
// transB: op(B) = B^T with B given as (n x k).  lowerB: B (k x n) is lower
// triangular (entries with row < col are skipped = treated as 0); lowerA: same
// for A (m x k).
template <bool TRANSB>
__global__ __launch_bounds__(256) void k_gemm(int m, int n, int k, double alpha,
                                              const double* A, int64_t lda,
                                              const double* B, int64_t ldb,
                                              double beta, double* C,
                                              int64_t ldc) {
  __shared__ double As[16][64 + 1];  // As[kk][i]
  __shared__ double Bs[16][64 + 1];  // Bs[kk][j]
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < k; k0 += 16) {
    for (int e = tid; e < 64 * 16; e += 256) {
      {  // A tile: rows i0..i0+63, cols k0..k0+15
        const int i = e >> 4, kk = e & 15;
        const int gi = i0 + i, gk = k0 + kk;
        As[kk][i] = (gi < m && gk < k) ? A[int64_t(gi) * lda + gk] : 0.0;
      }
      if (TRANSB) {  // B is (n x k): Bs[kk][j] = B[j0+j][k0+kk]
        const int j = e >> 4, kk = e & 15;
        const int gj = j0 + j, gk = k0 + kk;
        Bs[kk][j] = (gj < n && gk < k) ? B[int64_t(gj) * ldb + gk] : 0.0;
      } else {  // B is (k x n)
        const int kk = e >> 6, j = e & 63;
        const int gj = j0 + j, gk = k0 + kk;
        Bs[kk][j] = (gj < n && gk < k) ? B[int64_t(gk) * ldb + gj] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = As[kk][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = i0 + ty + 16 * r;
    if (gi >= m) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gj = j0 + tx + 16 * c;
      if (gj >= n) continue;
      double* p = C + int64_t(gi) * ldc + gj;
      const double old = (beta == 0.0) ? 0.0 : beta * (*p);
      *p = alpha * acc[r][c] + old;
    }
  }
}

int gemm(sgp_ctx* ctx, bool transB, int m, int n, int k, double alpha,
         const double* A, int64_t lda, const double* B, int64_t ldb,
         double beta, double* C, int64_t ldc) {
  if (m <= 0 || n <= 0) return 0;
  dim3 grid((n + 63) / 64, (m + 63) / 64);
  if (transB)
    hipLaunchKernelGGL(k_gemm<true>, grid, dim3(256), 0, ctx->stream, m, n, k,
                       alpha, A, lda, B, ldb, beta, C, ldc);
  else
    hipLaunchKernelGGL(k_gemm<false>, grid, dim3(256), 0, ctx->stream, m, n, k,
                       alpha, A, lda, B, ldb, beta, C, ldc);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// Recursive Cholesky + inverse on the n_f x n_f device matrices A (-> L) and
// Li (-> L^-1, must be zero-initialised); T is an n_f x n_f workspace.
int factor_rec(sgp_ctx* ctx, double* A, double* Li, double* T, int64_t ld,
               int off, int s, int* info_dev) {
  double* Ad = A + int64_t(off) * ld + off;
  double* Ld = Li + int64_t(off) * ld + off;
  if (s <= NB) {
    hipLaunchKernelGGL(k_leaf, dim3(1), dim3(256), 0, ctx->stream, Ad, ld, Ld,
                       ld, off, info_dev);
    SGP_HIP(ctx, hipGetLastError());
    return 0;
  }
  const int h = ((s / NB + 1) / 2) * NB;  // split at a leaf boundary
  const int r = s - h;
  SGP_TRY(factor_rec(ctx, A, Li, T, ld, off, h, info_dev));
  double* A21 = Ad + int64_t(h) * ld;
  double* A22 = Ad + int64_t(h) * ld + h;
  double* Li21 = Ld + int64_t(h) * ld;
  double* Li22 = Ld + int64_t(h) * ld + h;
  double* T21 = T + int64_t(off + h) * ld + off;
  // T21 = A21 * Linv11^T ; A21 <- T21  (L21)
  SGP_TRY(gemm(ctx, true, r, h, h, 1.0, A21, ld, Ld, ld, 0.0, T21, ld));
  SGP_HIP(ctx, hipMemcpy2DAsync(A21, ld * sizeof(double), T21,
                                ld * sizeof(double), h * sizeof(double), r,
                                hipMemcpyDeviceToDevice, ctx->stream));
  // A22 -= L21 L21^T
  SGP_TRY(gemm(ctx, true, r, r, h, -1.0, A21, ld, A21, ld, 1.0, A22, ld));
  SGP_TRY(factor_rec(ctx, A, Li, T, ld, off + h, r, info_dev));
  // Linv21 = -Linv22 * (L21 * Linv11)
  SGP_TRY(gemm(ctx, false, r, h, h, 1.0, A21, ld, Ld, ld, 0.0, T21, ld));
  SGP_TRY(gemm(ctx, false, r, h, r, -1.0, Li22, ld, T21, ld, 0.0, Li21, ld));
  return 0;
}

// ---- pack L^-1 into MFMA A-operand order ----------------------------------------
// Apack[(b * nsteps + s) * 64 + lane] = Linv[16 b + (lane & 15)][4 s + (lane >> 4)]
// (zero outside the n x n lower triangle): lane = 16 k + row, which is the A
// operand map of v_mfma_f64_16x16x4_f64 AND of v_mfma_f64_4x4x4_4b_f64 when its
// four blocks are four 4-row groups (A[blk][i][k] <- lane 16k + 4blk + i).
//
// Narrow last row block (n - 16 (nblk - 1) <= 4 real rows): its four 4-row
// groups all hold the SAME real rows 16 b + (lane & 3).  With
// v_mfma_f64_4x4x4_4b_f64 the four groups are the instruction's four blocks, so
// B may then hold a different point quad per block -- the plain covariance
// register, no broadcast -- and ONE instruction per k-step covers all 16 points
// of the wave (the padding rows would otherwise cost 3 of every 4 MFMAs of the
// row block that meets EVERY j-block).
__global__ void k_pack(const double* Li, int64_t ld, int n, int nblk,
                       int nsteps, int narrow, double* Apack) {
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = int64_t(nblk) * nsteps * 64;
  if (e >= total) return;
  const int lane = int(e & 63);
  const int64_t bs = e >> 6;
  const int s = int(bs % nsteps);
  const int b = int(bs / nsteps);
  const int i = 16 * b + ((narrow && b == nblk - 1) ? (lane & 3) : (lane & 15));
  const int j = 4 * s + (lane >> 4);
  double v = 0.0;
  if (i < n && j <= i) v = Li[int64_t(i) * ld + j];
  Apack[e] = v;
}

// Lower-triangular products with up to 16 right-hand sides, V and the results
// stored one vector per row (pitch ldv / ldo).  Both read L^-1 exactly once,
// coalesced along its rows, in a fixed summation order (every rank of a
// multi-GPU run computes bit-identical operands).  (kMaxRhs: common.h)

// T[c][i] = sum_{j <= i} Li[i][j] V[c][j]: one wave per row i.
__global__ __launch_bounds__(256) void k_tri_mv(const double* Li, int64_t ld,
                                                int n, const double* V,
                                                int64_t ldv, int m, double* T,
                                                int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  double acc[kMaxRhs];
#pragma unroll
  for (int c = 0; c < kMaxRhs; ++c) acc[c] = 0.0;
  const double* row = Li + int64_t(i) * ld;
  for (int j = lane; j <= i; j += 64) {
    const double l = row[j];
#pragma unroll
    for (int c = 0; c < kMaxRhs; ++c)
      if (c < m) acc[c] = fma(l, V[c * ldv + j], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < kMaxRhs; ++c) {
    if (c < m) {
      double v = acc[c];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) T[c * ldo + i] = v;
    }
  }
}

// W[c][j] = sum_{i >= j} Li[i][j] T[c][i] for j < n, 0 for n <= j < n_out:
// one workgroup per 64 columns, its 8 waves take every 8th row.
__global__ __launch_bounds__(512) void k_tri_mtv(const double* Li, int64_t ld,
                                                 int n, const double* T,
                                                 int64_t ldt, int m, double* W,
                                                 int64_t ldo, int n_out) {
  __shared__ double sh[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64, j = j0 + lane;
  double acc[kMaxRhs];
#pragma unroll
  for (int c = 0; c < kMaxRhs; ++c) acc[c] = 0.0;
  if (j < n) {
    for (int i = j0 + wave; i < n; i += 8) {
      const double l = (i >= j) ? Li[int64_t(i) * ld + j] : 0.0;
#pragma unroll
      for (int c = 0; c < kMaxRhs; ++c)
        if (c < m) acc[c] = fma(l, T[c * ldt + i], acc[c]);
    }
  }
  for (int c = 0; c < m; ++c) {           // m is uniform: barriers are safe
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxRhs; ++k) v = (k == c) ? acc[k] : v;
    sh[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && j < n_out) {
      double tot = 0.0;
#pragma unroll
      for (int w = 0; w < 8; ++w) tot += sh[w][lane];
      W[c * ldo + j] = (j < n) ? tot : 0.0;
    }
    __syncthreads();
  }
}

int launch_tri_mv(sgp_ctx* ctx, const double* Li, int64_t ld, int n,
                  const double* V, int64_t ldv, int m, double* T, int64_t ldo) {
  hipLaunchKernelGGL(k_tri_mv, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, Li,
                     ld, n, V, ldv, m, T, ldo);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

int launch_tri_mtv(sgp_ctx* ctx, const double* Li, int64_t ld, int n,
                   const double* T, int64_t ldt, int m, double* W, int64_t ldo,
                   int n_out) {
  hipLaunchKernelGGL(k_tri_mtv, dim3((n_out + 63) / 64), dim3(512), 0,
                     ctx->stream, Li, ld, n, T, ldt, m, W, ldo, n_out);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// Xpad = zero-padded X; Xs = Xpad * scale0 per column (products of parts: copy);
// XA = the same rows and alpha interleaved per block of 16 training points:
// [16 d of Xs | 16 of alpha] (GpDev::XA)
__global__ void k_pad_rows(const double* X, const double* alpha, int n, int n_pad,
                           int d, KernDesc kd, double* Xpad, double* Xs,
                           double* XA) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_pad * d) return;
  const double v = (e < n * d) ? X[e] : 0.0;
  const double vs = (kd.n_parts == 1) ? v * kd.scale0[e % d] : v;
  Xpad[e] = v;
  Xs[e] = vs;
  const int row = e / d, col = e - row * d, jb = row >> 4, r = row & 15;
  double* blk = XA + size_t(jb) * (16 * d + 16);
  blk[r * d + col] = vs;
  if (col == 0) blk[16 * d + r] = alpha[row];     // zero beyond n (publish_gp)
}


}  // namespace

int factor_dense(sgp_ctx* ctx, double* A, double* Li, double* T, int64_t ld, int s,
                 int* info_dev) {
  return factor_rec(ctx, A, Li, T, ld, 0, s, info_dev);
}

int gemm_dense(sgp_ctx* ctx, bool transB, int m, int n, int k, double alpha, const double* A,
               int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
  return gemm(ctx, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
}

int tri_mv_dense(sgp_ctx* ctx, const double* Li, int64_t ld, int n, const double* V,
                 int64_t ldv, int m, double* T, int64_t ldo) {
  return launch_tri_mv(ctx, Li, ld, n, V, ldv, m, T, ldo);
}

int tri_mtv_dense(sgp_ctx* ctx, const double* Li, int64_t ld, int n, const double* T,
                  int64_t ldt, int m, double* W, int64_t ldo, int n_out) {
  return launch_tri_mtv(ctx, Li, ld, n, T, ldt, m, W, ldo, n_out);
}

int launch_kernel_matrix(sgp_ctx* ctx, const KernDesc& kd, const double* X1,
                         int64_t n1, const double* X2, int64_t n2, double* out,
                         int64_t ld, int symmetric_diag, double diag_add,
                         int64_t n_valid, const double* diag_vec) {
  if (n1 <= 0 || n2 <= 0) return 0;
  dim3 block(64, 4);
  dim3 grid(unsigned((n2 + 63) / 64), unsigned((n1 + 3) / 4));
#define KM_CASE(DD)                                                            \
  case DD:                                                                     \
    hipLaunchKernelGGL(k_kernel_matrix<DD>, grid, block, 0, ctx->stream, kd,   \
                       X1, n1, X2, n2, out, ld, symmetric_diag, diag_add,      \
                       n_valid, diag_vec);                                     \
    break;
  switch (kd.d) {
    KM_CASE(1) KM_CASE(2) KM_CASE(3) KM_CASE(4)
    KM_CASE(5) KM_CASE(6) KM_CASE(7) KM_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", kd.d, SGP_MAX_D);
      return -2;
  }
#undef KM_CASE
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// Everything the sweeps read, derived from the dense L^-1 (ld = gp->ld),
// gp->X and gp->alpha (first n entries valid): packed operand matrix, padded /
// pre-scaled inputs, zero-padded alpha, device descriptor.
int publish_gp(sgp_gp* gp) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), np = gp->n_pad, d = gp->kern.d;
  double* Li = static_cast<double*>(gp->Linv.p);
  const int nblk = np / 16, nsteps = np / 4;
  const int64_t total = int64_t(nblk) * nsteps * 64;
  // (SGP_NO_NARROW=1: the A/B switch of profiles/)
  static const bool no_narrow = getenv("SGP_NO_NARROW") != nullptr;
  const int narrow = (!no_narrow && n - 16 * (nblk - 1) <= 4) ? 1 : 0;
  // (capacity for every n up to the pitch of L^-1: one-row appends then never
  // reallocate -- a reallocation is a hipMalloc and a stream sync)
  const size_t cap_rows = size_t(std::max(gp->ld, np));
  SGP_TRY(sgp_reserve(ctx, &gp->Apack,
                      (cap_rows / 16) * (cap_rows / 4) * 64 * sizeof(double)));
  hipLaunchKernelGGL(k_pack, dim3(unsigned((total + 255) / 256)), dim3(256), 0,
                     ctx->stream, Li, int64_t(gp->ld), n, nblk, nsteps, narrow,
                     static_cast<double*>(gp->Apack.p));
  SGP_TRY(sgp_reserve(ctx, &gp->Xpad, cap_rows * d * sizeof(double)));
  SGP_TRY(sgp_reserve(ctx, &gp->Xs, cap_rows * d * sizeof(double)));
  SGP_TRY(sgp_reserve(ctx, &gp->XA, (cap_rows / 16 + 1) * (16 * d + 16) * sizeof(double)));
  hipLaunchKernelGGL(k_pad_rows, dim3((np * d + 255) / 256), dim3(256), 0,
                     ctx->stream, static_cast<double*>(gp->X.p),
                     static_cast<double*>(gp->alpha.p), n, np, d,
                     gp->kern, static_cast<double*>(gp->Xpad.p),
                     static_cast<double*>(gp->Xs.p), static_cast<double*>(gp->XA.p));
  SGP_HIP(ctx, hipGetLastError());
  gp->dev.Apack = static_cast<double*>(gp->Apack.p);
  gp->dev.Xpad = static_cast<double*>(gp->Xpad.p);
  gp->dev.Xs = static_cast<double*>(gp->Xs.p);
  gp->dev.alpha = static_cast<double*>(gp->alpha.p);
  gp->dev.XA = static_cast<double*>(gp->XA.p);
  gp->dev.upd_w = static_cast<double*>(gp->updw.p);
  gp->dev.upd = static_cast<double*>(gp->upd.p);
  gp->dev.n = n;
  gp->dev.n_pad = np;
  gp->dev.nblk = nblk;
  gp->dev.narrow = narrow;
  gp->dev.last_rows = n - 16 * (nblk - 1);
  gp->dev.share = -1;       // (only collect_gps, which sees the other GPs, may set it)
  gp->dev.Linv = Li;
  gp->dev.ld = gp->ld;
  gp->dev.prior = gp->kern.kdiag + gp->noise_var + 1e-8 + gp->jitter;
  gp->dev.kern = gp->kern;
  return 0;
}

// Build Ky (with gp->jitter), factor, invert, pack, alpha.  *info = 0 or the
// 1-based index of the first non-positive pivot.  Buffers are sized for
// gp->ld >= n_f rows so later one-row appends need no reallocation.
// info_dev_out != nullptr: the pivot word is NOT read back (no stream sync) -- the caller
// gets its device address and reads it with its own result (hyper.hip); everything behind
// the factorisation is enqueued regardless, on garbage when a pivot failed.
int factor_gp(sgp_gp* gp, int* info, const int** info_dev_out) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), nf = gp->n_f, np = gp->n_pad, ld = gp->ld;
  const size_t mat = size_t(ld) * ld * sizeof(double);
  SGP_TRY(sgp_reserve(ctx, &gp->Kmat, mat));
  SGP_TRY(sgp_reserve(ctx, &gp->Linv, mat));
  SGP_TRY(sgp_reserve(ctx, &gp->work, mat));
  SGP_TRY(sgp_reserve(ctx, &gp->tvec, size_t(ld) * sizeof(double) + 64));
  SGP_TRY(sgp_reserve(ctx, &gp->alpha, size_t(ld + 16) * sizeof(double)));
  SGP_TRY(sgp_reserve(ctx, &gp->updw, size_t(ld + 16) * sizeof(double)));
  SGP_TRY(sgp_reserve(ctx, &gp->upd, size_t(SGP_MAX_D + 2) * sizeof(double)));
  double* K = static_cast<double*>(gp->Kmat.p);
  double* Li = static_cast<double*>(gp->Linv.p);
  double* T = static_cast<double*>(gp->work.p);
  double* tv = static_cast<double*>(gp->tvec.p);
  int* info_dev = reinterpret_cast<int*>(tv + ld);
  gp->upd_valid = false;
  gp->rem_valid = false;
  gp->blk_valid = false;
  gp->rw_valid = false;

  // padded rows of X are never read: n_valid = n turns them into identity
  const double* diag_vec = nullptr;
  if (!gp->rhost.empty()) {          // (tvec is free until alpha is formed)
    hipLaunchKernelGGL(k_scaled_diag, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, tv, n,
                       static_cast<const double*>(gp->R.p), gp->noise_var + 1e-8, gp->jitter);
    SGP_HIP(ctx, hipGetLastError());
    diag_vec = tv;
  }
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, static_cast<double*>(gp->X.p),
                               nf, static_cast<double*>(gp->X.p), nf, K, ld, 1,
                               gp->noise_var + 1e-8 + gp->jitter, n, diag_vec));
  SGP_HIP(ctx, hipMemsetAsync(Li, 0, mat, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
  SGP_TRY(factor_rec(ctx, K, Li, T, ld, 0, nf, info_dev));
  if (info_dev_out) {
    *info_dev_out = info_dev;
  } else {
    SGP_TRY(sgp_d2h(ctx, info, info_dev, sizeof(int)));
    if (*info != 0) return 0;
  }

  SGP_TRY(launch_tri_mv(ctx, Li, ld, n, static_cast<double*>(gp->Y.p), 0, 1, tv, 0));
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, tv, 0, 1,
                         static_cast<double*>(gp->alpha.p), 0, np));
  return publish_gp(gp);
}

// ---- one-row updates --------------------------------------------------------------
// Bordered Cholesky: with k = k(X, x*), t = L^-1 k, w = L^-T t = Ky^-1 k,
// s2 = k(x*,x*) + noise + 1e-8 + jitter - |t|^2:
//   new row of L^-1 = [ -w^T / s , 1 / s ],
//   alpha <- [ alpha - w r / s2 ; r / s2 ],  r = y* - k^T alpha  (= y* - mu(x*)).
// The record {w, r/s2, 1/s2, x*} is kept for the rank-1 update of the resident
// posterior (k_rank1).  One workgroup; n <= a few thousand.
__global__ __launch_bounds__(1024) void k_append_finish(
    double* Li, int64_t ld, int n, int d, const double* kc, const double* Tt,
    const double* Wt, double prior, double y, const double* xnew, double* alpha,
    double* updw, double* upd, int n_pad_new, int* info) {
  __shared__ double sh[2][1024 / 64];
  double a = 0.0, b = 0.0;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    a = fma(Tt[j], Tt[j], a);
    b = fma(kc[j], alpha[j], b);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  double tn2 = 0.0, mu = 0.0;
  for (int w = 0; w < int(blockDim.x >> 6); ++w) {
    tn2 += sh[0][w];
    mu += sh[1][w];
  }
  const double s2 = prior - tn2;
  // GPy would retry with jitter here; report and let the host refit instead
  if (!(s2 > 1e-12 * prior) || !isfinite(s2)) {
    if (threadIdx.x == 0) info[0] = n + 1;
    return;
  }
  const double sd = sqrt(s2);
  const double r = y - mu;
  for (int j = threadIdx.x; j < n_pad_new; j += blockDim.x) {
    if (j < n) {
      const double w = Wt[j];
      Li[int64_t(n) * ld + j] = -w / sd;
      alpha[j] -= w * r / s2;
      updw[j] = w;
    } else {
      if (j == n) {
        Li[int64_t(n) * ld + n] = 1.0 / sd;
        alpha[n] = r / s2;
      } else {
        alpha[j] = 0.0;
      }
      updw[j] = 0.0;
    }
  }
  if (threadIdx.x == 0) {
    upd[0] = r / s2;
    upd[1] = 1.0 / s2;
    info[0] = 0;
  }
  if (threadIdx.x < d) upd[2 + threadIdx.x] = xnew[threadIdx.x];
}

// gp->X already holds the new row at index gp->n (uploaded by the caller);
// gp->Y gets y.  On success n grows by one; *info != 0 leaves the GP untouched.
int append_gp(sgp_gp* gp, double y, int* info, double r) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), ld = gp->ld, d = gp->kern.d;
  double* Li = static_cast<double*>(gp->Linv.p);
  double* X = static_cast<double*>(gp->X.p);
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(3) * ld * 8 + 64, &buf));
  double* Kc = buf;
  double* Tt = buf + ld;
  double* Wt = buf + 2 * size_t(ld);
  int* info_dev = reinterpret_cast<int*>(buf + 3 * size_t(ld));
  const double* xnew = X + size_t(n) * d;
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, xnew, 1, X, n, Kc, ld, 0, 0.0,
                               INT64_MAX));
  SGP_TRY(launch_tri_mv(ctx, Li, ld, n, Kc, ld, 1, Tt, ld));
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, Tt, ld, 1, Wt, ld, n));
  const int np_new = (n + 1 + 15) / 16 * 16;
  const double prior = row_prior(gp, r);
  hipLaunchKernelGGL(k_append_finish, dim3(1), dim3(1024), 0, ctx->stream, Li,
                     int64_t(ld), n, d, Kc, Tt, Wt, prior, y, xnew,
                     static_cast<double*>(gp->alpha.p),
                     static_cast<double*>(gp->updw.p),
                     static_cast<double*>(gp->upd.p), np_new, info_dev);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(sgp_d2h(ctx, info, info_dev, sizeof(int)));
  if (*info != 0) return 0;
  gp->n = n + 1;
  gp->n_pad = np_new;
  gp->n_f = (n + 1 + 31) / 32 * 32;
  gp->upd_valid = true;
  gp->rem_valid = false;
  gp->blk_valid = false;
  gp->rw_valid = false;
  return publish_gp(gp);
}

// ---- block append ----------------------------------------------------------------------
// b rows at once: with Kc = k(X, Xnew), T = L^-1 Kc, W = L^-T T (one vector
// per new row, pitch `pitch`),
//   C = k(Xnew, Xnew) + (noise + 1e-8 + jitter) I - T^T T = Lc Lc^T,
//   rows n0 .. n0+b-1 of L^-1 = Lc^-1 [ -W^T | I ],
//   gamma_j = (row n0+j) . y' = sum_{c <= j} Lc^-1[j][c] (y_c - k_c^T alpha),
//   alpha <- [alpha; 0] + sum_j (row n0+j)^T gamma_j       (j = 0 .. b-1, in that order).
// One workgroup: the b (b + 1) / 2 + b dot products over the old rows go one per wave, lanes
// striding, folded by shuffles; thread 0 factors the corner with k_append_finish's pivot rule
// (pivot j = the s2 a one-row append of row j behind rows 0 .. j-1 would meet); nothing of the
// GP is written before every pivot has passed.  blk receives the block record (common.h, kBlk*).
struct BlockPriors {
  double v[SGP_MAX_BLOCK];   // k(x,x) + (noise + 1e-8) r_j + jitter of new row j
};
__global__ __launch_bounds__(1024) void k_append_block_finish(
    double* Li, int64_t ld, int n0, int b, const double* Kc, const double* Tt, const double* Wt,
    int64_t pitch, const double* Knn, BlockPriors pri, const double* ynew, double* alpha,
    double* blk, int n_pad_new, int* info) {
  constexpr int B = SGP_MAX_BLOCK;
  __shared__ double cm[B][B + 1];    // T^T T (lower), then Lc
  __shared__ double inv[B][B + 1];   // Lc^-1 (lower), zero above the diagonal
  __shared__ double res[B], gam[B];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npairs = b * (b + 1) / 2;
  for (int p = wave; p < npairs + b; p += 1024 / 64) {
    int a = 0, c = p - npairs;
    const double *u = Kc + (p >= npairs ? c : 0) * pitch, *v = alpha;
    if (p < npairs) {
      while ((a + 1) * (a + 2) / 2 <= p) ++a;
      c = p - a * (a + 1) / 2;
      u = Tt + a * pitch;
      v = Tt + c * pitch;
    }
    double s = 0.0;
    for (int i = lane; i < n0; i += 64) s = fma(u[i], v[i], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      if (p < npairs) cm[a][c] = s;
      else res[c] = ynew[c] - s;
    }
  }
  if (tid == 0) bad = 0;
  for (int e = tid; e < B * (B + 1); e += 1024) (&inv[0][0])[e] = 0.0;
  __syncthreads();
  if (tid == 0) {
    for (int j = 0; j < b && bad == 0; ++j) {
      for (int c = 0; c <= j; ++c) {
        const double prior = pri.v[j];
        double s = (c == j ? prior : Knn[j * B + c]) - cm[j][c];
        for (int k = 0; k < c; ++k) s -= cm[j][k] * cm[c][k];
        if (c < j) {
          cm[j][c] = s / cm[c][c];
        } else if (!(s > 1e-12 * prior) || !isfinite(s)) {
          // GPy would retry with jitter here; report and let the host refit instead
          bad = n0 + j + 1;
        } else {
          cm[j][j] = sqrt(s);
        }
      }
    }
  }
  __syncthreads();
  if (bad != 0) {
    if (tid == 0) info[0] = bad;
    return;
  }
  if (tid < b) {                      // column tid of Lc^-1 by forward substitution
    const int c = tid;
    for (int i = c; i < b; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= cm[i][k] * inv[k][c];
      inv[i][c] = s / cm[i][i];
    }
  }
  __syncthreads();
  if (tid < B) {
    double g = 0.0;
    for (int c = 0; c <= tid && tid < b; ++c) g = fma(inv[tid][c], res[c], g);
    gam[tid] = g;                     // (zero behind b)
  }
  __syncthreads();
  for (int i = tid; i < n_pad_new; i += 1024) {
    if (i < n0) {
      double w[B];
#pragma unroll
      for (int c = 0; c < B; ++c) w[c] = (c < b) ? Wt[c * pitch + i] : 0.0;
      double da = 0.0;
#pragma unroll 1
      for (int j = 0; j < b; ++j) {   // (inv is zero above the diagonal, w behind b)
        double row = 0.0;
#pragma unroll
        for (int c = 0; c < B; ++c) row = fma(inv[j][c], w[c], row);
        Li[int64_t(n0 + j) * ld + i] = -row;
        da = fma(-row, gam[j], da);
      }
      alpha[i] += da;
    } else if (i < n0 + b) {
      const int c = i - n0;
      double da = 0.0;
      for (int j = 0; j < b; ++j) {
        Li[int64_t(n0 + j) * ld + i] = inv[j][c];
        da = fma(inv[j][c], gam[j], da);
      }
      alpha[i] = da;
    } else {
      alpha[i] = 0.0;
    }
  }
  if (tid < B) blk[kBlkGamma + tid] = gam[tid];
  if (tid == 0) {
    blk[kBlkB] = double(b);
    blk[kBlkN0] = double(n0);
    info[0] = 0;
  }
}

// gp->X / gp->Y already hold the new rows at gp->n .. gp->n + b - 1 (uploaded by the caller).
// On success n grows by b; *info != 0 leaves the GP untouched.
int append_block_gp(sgp_gp* gp, int b, int* info, const double* r) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), ld = gp->ld, d = gp->kern.d;
  double* Li = static_cast<double*>(gp->Linv.p);
  double* X = static_cast<double*>(gp->X.p);
  SGP_TRY(sgp_reserve(ctx, &gp->blk, size_t(kBlkWords) * sizeof(double)));
  double* buf;
  const size_t vec = size_t(SGP_MAX_BLOCK) * ld;
  SGP_TRY(sgp_scratch(ctx, kSlotStage,
                      (3 * vec + SGP_MAX_BLOCK * SGP_MAX_BLOCK) * sizeof(double) + 64, &buf));
  double* Kc = buf;
  double* Tt = buf + vec;
  double* Wt = buf + 2 * vec;
  double* Knn = buf + 3 * vec;
  int* info_dev = reinterpret_cast<int*>(Knn + SGP_MAX_BLOCK * SGP_MAX_BLOCK);
  const double* xnew = X + size_t(n) * d;
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, xnew, b, X, n, Kc, ld, 0, 0.0, INT64_MAX));
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, xnew, b, xnew, b, Knn, SGP_MAX_BLOCK, 0, 0.0,
                               INT64_MAX));
  SGP_TRY(launch_tri_mv(ctx, Li, ld, n, Kc, ld, b, Tt, ld));
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, Tt, ld, b, Wt, ld, n));
  const int np_new = (n + b + 15) / 16 * 16;
  BlockPriors prior;
  for (int j = 0; j < SGP_MAX_BLOCK; ++j) prior.v[j] = row_prior(gp, (r && j < b) ? r[j] : 1.0);
  hipLaunchKernelGGL(k_append_block_finish, dim3(1), dim3(1024), 0, ctx->stream, Li,
                     int64_t(ld), n, b, Kc, Tt, Wt, int64_t(ld), Knn, prior,
                     static_cast<const double*>(gp->Y.p) + n, static_cast<double*>(gp->alpha.p),
                     static_cast<double*>(gp->blk.p), np_new, info_dev);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(sgp_d2h(ctx, info, info_dev, sizeof(int)));
  if (*info != 0) return 0;
  gp->n = n + b;
  gp->n_pad = np_new;
  gp->n_f = (n + b + 31) / 32 * 32;
  gp->upd_valid = false;
  gp->rem_valid = false;
  gp->blk_valid = true;
  gp->rw_valid = false;
  return publish_gp(gp);
}

// Drop the last row: the leading principal block of a lower-triangular inverse
// is the inverse of the leading block, so only alpha has to be recomputed.
int pop_gp(sgp_gp* gp) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n) - 1, ld = gp->ld;
  double* Li = static_cast<double*>(gp->Linv.p);
  double* tv = static_cast<double*>(gp->tvec.p);
  gp->n = n;
  gp->n_pad = (n + 15) / 16 * 16;
  gp->n_f = (n + 31) / 32 * 32;
  gp->upd_valid = false;
  gp->rem_valid = false;
  gp->blk_valid = false;
  gp->rw_valid = false;
  SGP_TRY(launch_tri_mv(ctx, Li, ld, n, static_cast<double*>(gp->Y.p), 0, 1, tv, 0));
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, tv, 0, 1,
                         static_cast<double*>(gp->alpha.p), 0, gp->n_pad));
  return publish_gp(gp);
}

// ---- removal of ANY row --------------------------------------------------------------
// With M = L^-1 and c = column i of M (zero above row i):  P_ii = |c|^2 = (Ky^-1)_ii and
// p = M^T c = column i of Ky^-1.  The reduced GP follows in closed form:
//   w = -p_{-i} / P_ii  (= Ky_new^-1 k(X_new, x_i)),   alpha_new = alpha_{-i} + w alpha_i,
// and L_new^-1 = M with column i deleted after the Givens rotations that fold c_k into c_i,
// k = i+1 .. n-1 in that order:  gamma_i = c_i, gamma_k^2 = gamma_{k-1}^2 + c_k^2,
// cs_k = gamma_{k-1} / gamma_k, sn_k = c_k / gamma_k, applied to the rows (i, k).  Row i
// collects what is thrown away; every row k keeps its zeros and a positive diagonal
// (cs_k M_kk).  {w, alpha_i, P_ii, x_i} is the record of the removal, in the layout of the
// append record: what appending x_i to the reduced GP would write (k_rank1<.., true>).

// The scratch of a removal (kSlotStage), in doubles, L = the pitch of L^-1: everything is
// formed here, and the pivot word read back, before the GP is touched.
struct RemoveBufs {
  double *c, *p, *cs, *sn;   // [L] column i of M (zero above i), M^T c, the rotations
  double *w, *alpha;         // [L + 16] the record's w and alpha_new, zero padded to n_pad
  double *X, *Y;             // [L d], [L]: the rows behind i, one row up
  double* rec;               // [2 + SGP_MAX_D] alpha_i | P_ii | x_i
  int* info;
};
inline size_t remove_scratch_bytes(int ld, int d) {
  return (size_t(ld) * (7 + d) + 32 + 2 + SGP_MAX_D) * sizeof(double) + 64;
}
inline RemoveBufs remove_bufs(double* b, int ld, int d) {
  RemoveBufs r;
  r.c = b;
  r.p = r.c + ld;
  r.cs = r.p + ld;
  r.sn = r.cs + ld;
  r.w = r.sn + ld;
  r.alpha = r.w + ld + 16;
  r.X = r.alpha + ld + 16;
  r.Y = r.X + size_t(ld) * d;
  r.rec = r.Y + ld;
  r.info = reinterpret_cast<int*>(r.rec + 2 + SGP_MAX_D);
  return r;
}

// c, P_ii and the rotation coefficients: one workgroup.  gamma_k^2 is a running sum of
// squares -- a scan in a fixed order: every thread owns a run of consecutive k, the runs'
// sums are scanned through the wave and then over the 16 waves.  info: 0, or index + 1
// when P_ii or a gamma is not positive and finite.
__global__ __launch_bounds__(1024) void k_remove_coef(const double* Li, int64_t ld, int n,
                                                      int i, RemoveBufs rb) {
  __shared__ double sh[1024 / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < i; k += 1024) rb.c[k] = 0.0;
  const int m = n - i;                         // entries i .. n-1 of the column
  const int per = (m + 1023) / 1024;
  const int e0 = min(tid * per, m), e1 = min(e0 + per, m);
  double local = 0.0;
  for (int e = e0; e < e1; ++e) {
    const double ck = Li[int64_t(i + e) * ld + i];
    rb.c[i + e] = ck;
    local = fma(ck, ck, local);
  }
  double v = local;                            // inclusive scan of the wave's runs
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) sh[wave] = v;
  double before = __shfl_up(v, 1, 64);         // the runs in front of this one, in the wave
  if (lane == 0) before = 0.0;
  __syncthreads();
  double base = 0.0, total = 0.0;
  for (int w = 0; w < 1024 / 64; ++w) {
    if (w < wave) base += sh[w];
    total += sh[w];
  }
  bool bad = false;
  double s = base + before;                    // gamma_{k-1}^2 in front of the run
  for (int e = e0; e < e1; ++e) {
    const double ck = rb.c[i + e];             // (written by this thread)
    const double s1 = fma(ck, ck, s);
    if (e > 0) {
      const double g1 = sqrt(s1);
      rb.cs[i + e] = sqrt(s) / g1;
      rb.sn[i + e] = ck / g1;
    }
    bad = bad || !(s1 > 0.0) || !isfinite(s1);
    s = s1;
  }
  bad = bad || !(total > 0.0) || !isfinite(total);
  const int bad_any = __syncthreads_or(bad);
  if (tid == 0) {
    rb.rec[1] = total;
    rb.info[0] = bad_any ? i + 1 : 0;
  }
}

// The images of what changes besides L^-1: w and alpha_new (zero behind n - 1, up to the
// new n_pad), the record, and the rows of X / Y behind i moved one up.
__global__ void k_remove_stage(const double* alpha, const double* X, const double* Y, int n,
                               int d, int i, int n_pad_new, RemoveBufs rb) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const double Pii = rb.rec[1];
  if (e < n_pad_new) {
    double w = 0.0, a = 0.0;
    if (e < n - 1) {
      const int src = e + (e >= i ? 1 : 0);
      w = -rb.p[src] / Pii;
      a = fma(w, alpha[i], alpha[src]);
    }
    rb.w[e] = w;
    rb.alpha[e] = a;
  }
  if (e >= i && e < n - 1) rb.Y[e] = Y[e + 1];
  if (e >= i * d && e < (n - 1) * d) rb.X[e] = X[e + d];
  if (e == 0) rb.rec[0] = alpha[i];
  if (e < d) rb.rec[2 + e] = X[i * d + e];
}

// out = M with the rotations applied and row / column i deleted; one thread per column j of
// M: rho = M[i][j], then rows k = max(i + 1, j) .. n-1 in order (the loads of a row are
// coalesced over the lanes and do not depend on rho).  `out` is zero where nothing is written.
__global__ __launch_bounds__(64) void k_remove_rotate(const double* M, double* out, int64_t ld,
                                                      int n, int i, const double* cs,
                                                      const double* sn) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n || j == i) return;
  const int jo = j - (j > i ? 1 : 0);
  for (int k = j; k < i; ++k) out[int64_t(k) * ld + jo] = M[int64_t(k) * ld + j];
  double rho = (j < i) ? M[int64_t(i) * ld + j] : 0.0;
  int k = max(i + 1, j);
  constexpr int kU = 8;                        // loads in flight per lane
  for (; k + kU <= n; k += kU) {
    double mv[kU], c[kU], s[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      mv[u] = M[int64_t(k + u) * ld + j];
      c[u] = cs[k + u];
      s[u] = sn[k + u];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      out[int64_t(k + u - 1) * ld + jo] = fma(c[u], mv[u], -(s[u] * rho));
      rho = fma(c[u], rho, s[u] * mv[u]);
    }
  }
  for (; k < n; ++k) {
    const double mv = M[int64_t(k) * ld + j], c = cs[k], s = sn[k];
    out[int64_t(k - 1) * ld + jo] = fma(c, mv, -(s * rho));
    rho = fma(c, rho, s * mv);
  }
}

// ... and the images copied over the GP, once the pivot word has said yes.
__global__ void k_remove_commit(RemoveBufs rb, int n, int d, int i, int n_pad_new,
                                double* alpha, double* updw, double* upd, double* X, double* Y) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_pad_new) {
    alpha[e] = rb.alpha[e];
    updw[e] = rb.w[e];
  }
  if (e >= i && e < n - 1) Y[e] = rb.Y[e];
  if (e >= i * d && e < (n - 1) * d) X[e] = rb.X[e];
  if (e < 2 + d) upd[e] = rb.rec[e];
}

int remove_gp(sgp_gp* gp, int index, int* info) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), ld = gp->ld, d = gp->kern.d, i = index;
  const size_t mat = size_t(ld) * ld * sizeof(double);
  // (a clone has no spare matrix before its first refit)
  SGP_TRY(sgp_reserve(ctx, &gp->work, mat));
  double* Li = static_cast<double*>(gp->Linv.p);
  double* out = static_cast<double*>(gp->work.p);
  double* X = static_cast<double*>(gp->X.p);
  double* Y = static_cast<double*>(gp->Y.p);
  double* alpha = static_cast<double*>(gp->alpha.p);
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, remove_scratch_bytes(ld, d), &buf));
  const RemoveBufs rb = remove_bufs(buf, ld, d);
  const int np_new = (n - 1 + 15) / 16 * 16;
  const int elems = std::max(np_new, std::max((n - 1) * d, 2 + d));
  hipLaunchKernelGGL(k_remove_coef, dim3(1), dim3(1024), 0, ctx->stream, Li, int64_t(ld), n, i,
                     rb);
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, rb.c, 0, 1, rb.p, 0, n));
  hipLaunchKernelGGL(k_remove_stage, dim3((elems + 255) / 256), dim3(256), 0, ctx->stream,
                     alpha, X, Y, n, d, i, np_new, rb);
  SGP_HIP(ctx, hipMemsetAsync(out, 0, mat, ctx->stream));
  hipLaunchKernelGGL(k_remove_rotate, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, Li, out,
                     int64_t(ld), n, i, rb.cs, rb.sn);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(sgp_d2h(ctx, info, rb.info, sizeof(int)));
  if (*info != 0) return 0;
  hipLaunchKernelGGL(k_remove_commit, dim3((elems + 255) / 256), dim3(256), 0, ctx->stream, rb,
                     n, d, i, np_new, alpha, static_cast<double*>(gp->updw.p),
                     static_cast<double*>(gp->upd.p), X, Y);
  SGP_HIP(ctx, hipGetLastError());
  std::swap(gp->Linv, gp->work);
  gp->n = n - 1;
  gp->n_pad = np_new;
  gp->n_f = (n - 1 + 31) / 32 * 32;
  gp->upd_valid = false;
  gp->rem_valid = true;
  gp->blk_valid = false;
  gp->rw_valid = false;
  return publish_gp(gp);
}

// ---- re-weighting ONE observation in place ------------------------------------------------
// Ky' = Ky + delta e_i e_i^T (delta = s (r' - r)), y_i -> y_i + dy.  With
// M = L^-1, c = column i of M, P_ii = |c|^2, p = M^T c:
//   tau = delta / (1 + delta P_ii),  eta = (dy - delta alpha_i) / (1 + delta P_ii),
//   alpha' = alpha + eta p,  Ky'^-1 = M^T (I - tau c c^T) M = (F M)^T (F M),
// F lower triangular with F^T F = I - tau c c^T.  With the running sums q_k = 1 + delta
// sum_{i <= j <= k} c_j^2 (q_{i-1} = 1, q_{n-1} = 1 + delta P_ii) the rows of F M are
//   M'[k] = sqrt(q_{k-1} / q_k) M[k] - delta c_k / sqrt(q_{k-1} q_k) S_k,
//   S_k = sum_{i <= j < k} c_j M[j]                      (k = i .. n-1; rows above i stay).
// Every q_k lies between 1 and 1 + delta P_ii: all are positive exactly when the last one is.
// The scratch is that of a removal: cs holds sqrt(q_{k-1} / q_k), sn the factor of S_k.

// c, P_ii and the row coefficients: one workgroup, the scan of k_remove_coef.  info: 0, or
// index + 1 when P_ii or a q_k is not positive and finite.
__global__ __launch_bounds__(1024) void k_reweigh_coef(const double* Li, int64_t ld, int n, int i,
                                                       double delta, RemoveBufs rb) {
  __shared__ double sh[1024 / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < i; k += 1024) rb.c[k] = 0.0;
  const int m = n - i;                         // entries i .. n-1 of the column
  const int per = (m + 1023) / 1024;
  const int e0 = min(tid * per, m), e1 = min(e0 + per, m);
  double local = 0.0;
  for (int e = e0; e < e1; ++e) {
    const double ck = Li[int64_t(i + e) * ld + i];
    rb.c[i + e] = ck;
    local = fma(ck, ck, local);
  }
  double v = local;                            // inclusive scan of the wave's runs
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) sh[wave] = v;
  double before = __shfl_up(v, 1, 64);         // the runs in front of this one, in the wave
  if (lane == 0) before = 0.0;
  __syncthreads();
  double base = 0.0, total = 0.0;
  for (int w = 0; w < 1024 / 64; ++w) {
    if (w < wave) base += sh[w];
    total += sh[w];
  }
  bool bad = false;
  double s = base + before;                    // sum of squares in front of the run
  for (int e = e0; e < e1; ++e) {
    const double ck = rb.c[i + e];             // (written by this thread)
    const double s1 = fma(ck, ck, s);
    const double q0 = fma(delta, s, 1.0), q1 = fma(delta, s1, 1.0);
    rb.cs[i + e] = sqrt(q0 / q1);
    rb.sn[i + e] = -delta * ck / sqrt(q0 * q1);
    bad = bad || !(q1 > 0.0) || !isfinite(q1);
    s = s1;
  }
  const double qn = fma(delta, total, 1.0);
  bad = bad || !(total > 0.0) || !isfinite(total) || !(qn > 0.0) || !isfinite(qn);
  const int bad_any = __syncthreads_or(bad);
  if (tid == 0) {
    rb.rec[1] = total;
    rb.info[0] = bad_any ? i + 1 : 0;
  }
}

// The images of what changes besides L^-1: alpha' (zero behind n, up to n_pad) and the record
// in the layout of an append record: x_i, w = -p / P_ii off row i (so that k(x, x_i) -
// k(X, x)^T w = c(x) / P_ii with c(x) = k(X, x)^T p), upd[0] = P_ii eta, upd[1] = tau P_ii^2.
__global__ void k_reweigh_stage(const double* alpha, const double* X, const double* Y, int n,
                                int d, int i, int n_pad, double y_new, double delta,
                                RemoveBufs rb) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const double Pii = rb.rec[1];
  const double q = fma(delta, Pii, 1.0);
  const double eta = ((y_new - Y[i]) - delta * alpha[i]) / q;
  if (e < n_pad) {
    double w = 0.0, a = 0.0;
    if (e < n) {
      if (e != i) w = -rb.p[e] / Pii;
      a = fma(eta, rb.p[e], alpha[e]);
    }
    rb.w[e] = w;
    rb.alpha[e] = a;
  }
  if (e == 0) {
    rb.X[0] = Pii * eta;                       // (rec[1] is read by every thread: staged apart)
    rb.X[1] = delta / q * Pii * Pii;
  }
  if (e < d) rb.rec[2 + e] = X[i * d + e];
}

// out = F M; one thread per column j of M, rows k = max(i, j) .. n-1 in order with the running
// sum S (the loads of a row are coalesced over the lanes and do not depend on S); the rows
// above i are copied.  `out` is zero where nothing is written.
__global__ __launch_bounds__(64) void k_reweigh_rows(const double* M, double* out, int64_t ld,
                                                     int n, int i, const double* c,
                                                     const double* sd, const double* g) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  for (int k = j; k < i; ++k) out[int64_t(k) * ld + j] = M[int64_t(k) * ld + j];
  double S = 0.0;
  int k = max(i, j);
  constexpr int kU = 8;                        // loads in flight per lane
  for (; k + kU <= n; k += kU) {
    double mv[kU], cc[kU], a[kU], b[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      mv[u] = M[int64_t(k + u) * ld + j];
      cc[u] = c[k + u];
      a[u] = sd[k + u];
      b[u] = g[k + u];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      out[int64_t(k + u) * ld + j] = fma(a[u], mv[u], b[u] * S);
      S = fma(cc[u], mv[u], S);
    }
  }
  for (; k < n; ++k) {
    const double mv = M[int64_t(k) * ld + j];
    out[int64_t(k) * ld + j] = fma(sd[k], mv, g[k] * S);
    S = fma(c[k], mv, S);
  }
}

// ... and the images copied over the GP, once the pivot word has said yes.
__global__ void k_reweigh_commit(RemoveBufs rb, int d, int i, int n_pad, double y_new,
                                 double* alpha, double* updw, double* upd, double* Y) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_pad) {
    alpha[e] = rb.alpha[e];
    updw[e] = rb.w[e];
  }
  if (e < 2) upd[e] = rb.X[e];
  else if (e < 2 + d) upd[e] = rb.rec[e];
  if (e == 0) Y[i] = y_new;
}

int reweigh_gp(sgp_gp* gp, int index, double y_new, double delta, int* info) {
  sgp_ctx* ctx = gp->ctx;
  const int n = int(gp->n), ld = gp->ld, d = gp->kern.d, i = index, np = gp->n_pad;
  const size_t mat = size_t(ld) * ld * sizeof(double);
  // (a clone has no spare matrix before its first refit)
  SGP_TRY(sgp_reserve(ctx, &gp->work, mat));
  double* Li = static_cast<double*>(gp->Linv.p);
  double* out = static_cast<double*>(gp->work.p);
  double* alpha = static_cast<double*>(gp->alpha.p);
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, remove_scratch_bytes(ld, d), &buf));
  const RemoveBufs rb = remove_bufs(buf, ld, d);
  const int elems = std::max(np, 2 + d);
  hipLaunchKernelGGL(k_reweigh_coef, dim3(1), dim3(1024), 0, ctx->stream, Li, int64_t(ld), n, i,
                     delta, rb);
  SGP_TRY(launch_tri_mtv(ctx, Li, ld, n, rb.c, 0, 1, rb.p, 0, n));
  hipLaunchKernelGGL(k_reweigh_stage, dim3((elems + 255) / 256), dim3(256), 0, ctx->stream,
                     alpha, static_cast<const double*>(gp->X.p),
                     static_cast<const double*>(gp->Y.p), n, d, i, np, y_new, delta, rb);
  SGP_HIP(ctx, hipMemsetAsync(out, 0, mat, ctx->stream));
  hipLaunchKernelGGL(k_reweigh_rows, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, Li, out,
                     int64_t(ld), n, i, rb.c, rb.cs, rb.sn);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(sgp_d2h(ctx, info, rb.info, sizeof(int)));
  if (*info != 0) return 0;
  hipLaunchKernelGGL(k_reweigh_commit, dim3((elems + 255) / 256), dim3(256), 0, ctx->stream, rb,
                     d, i, np, y_new, alpha, static_cast<double*>(gp->updw.p),
                     static_cast<double*>(gp->upd.p), static_cast<double*>(gp->Y.p));
  SGP_HIP(ctx, hipGetLastError());
  std::swap(gp->Linv, gp->work);
  gp->upd_valid = false;
  gp->rem_valid = false;
  gp->blk_valid = false;
  gp->rw_valid = true;
  return publish_gp(gp);
}

// ---- posterior of a FEW points -------------------------------------------------------
// SafeOptSwarm's default swarm has 20 particles and SafeOpt asks for the
// posterior of single points (gp_opt.py:1117, 1132): one 64-row tile of the
// sweep kernel would walk through all n^2/512 block products on ONE compute
// unit.  For P <= kSmallPoints the work is spread over the chip the other way
// round -- one workgroup per 16-row block of L^-1, 16 points per pass:
//   k_small_kb   : Kb = k(X, pts) in MFMA B-operand order, zero padded
//   k_small_mfma : |L^-1 Kb|^2 per (row block, point) on the matrix cores (the
//                  packed A operands of the sweep), 16 waves splitting the
//                  k-steps; the last row block also forms alpha . Kb
//   k_small_post : var = k(x,x) - sum over row blocks, GPy clip
// Three launches for ALL GPs (blockIdx.z = GP) whose time does not depend on
// n^2 per compute unit.
template <int D>
__global__ void k_small_kb(const GpDev* gps, const double* pts, int P, SmallBufs sb) {
  const GpDev& gp = gps[blockIdx.z];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int pass = blockIdx.y;
  if (e >= (gp.n_pad / 4) * 64) return;
  const int lane = e & 63, s = e >> 6;
  const int pt = pass * 16 + (lane & 15), j = 4 * s + (lane >> 4);
  double v = 0.0;
  if (pt < P && j < gp.n) {
    double a[D], b[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      a[k] = pts[int64_t(pt) * D + k];
      b[k] = gp.Xpad[int64_t(j) * D + k];
    }
    v = kern_eval<D>(gp.kern, a, b);
  }
  sb.Kb[blockIdx.z * sb.kb_stride + int64_t(pass) * sb.nsteps_max * 64 + e] = v;
}

// One workgroup per 16-row block of L^-1 and pass of 16 points; its 16 waves
// split the k-steps (the last row block has n / 4 of them: with four waves it was
// a chain of n / 16 exposed load latencies) and fold their partial products
// through LDS.
constexpr int kSmallWaves = 16;

__global__ __launch_bounds__(64 * kSmallWaves) void k_small_mfma(const GpDev* gps,
                                                                 SmallBufs sb) {
  __shared__ double4_t sh[kSmallWaves][64];
  __shared__ double shm[kSmallWaves][16];
  const GpDev& gp = gps[blockIdx.z];
  const int nblk = gp.nblk, nsteps = gp.n_pad / 4;
  const int blk = blockIdx.x, pass = blockIdx.y;
  if (blk >= nblk) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* A = gp.Apack + int64_t(blk) * nsteps * 64 + lane;
  const double* B = sb.Kb + blockIdx.z * sb.kb_stride +
                    int64_t(pass) * sb.nsteps_max * 64 + lane;
  const bool last = blk == nblk - 1;            // covers every k-step: the mean
  // narrow packing of the last row block (k_pack): its rows 4..15 repeat rows 0..3
  const bool dup = last && gp.narrow && (lane & 15) >= 4;
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  double m = 0.0;
  const int send = (blk + 1) * 4;               // up to the diagonal block
  constexpr int kInFlight = 8;                  // k-steps of a wave per batch (16: slower)
  for (int s = wave; s < send; s += kInFlight * kSmallWaves) {
    // all loads of the batch are issued before the first use
    double av[kInFlight], bv[kInFlight], al[kInFlight];
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      const int si = s + i * kSmallWaves;
      const bool ok = si < send;
      av[i] = (ok && !dup) ? A[si * 64] : 0.0;
      bv[i] = ok ? B[si * 64] : 0.0;
      al[i] = (ok && last) ? gp.alpha[4 * si + (lane >> 4)] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kInFlight; ++i) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[i], acc, 0, 0, 0);
      m = fma(al[i], bv[i], m);
    }
  }
  sh[wave][lane] = acc;
  if (last) {
    m += __shfl_xor(m, 16, 64);
    m += __shfl_xor(m, 32, 64);
    if (lane < 16) shm[wave][lane] = m;
  }
  __syncthreads();
  if (wave == 0) {
    // D layout: column (point) = lane & 15, rows (lane >> 4) + 4 r
    double4_t t = sh[0][lane];
#pragma unroll
    for (int w = 1; w < kSmallWaves; ++w) t += sh[w][lane];
    double ss = (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (lane < 16) {
      sb.part[blockIdx.z * sb.part_stride + (int64_t(pass) * sb.nblk_max + blk) * 16 + lane] = ss;
      if (last) {
        double mm = shm[0][lane];
#pragma unroll
        for (int w = 1; w < kSmallWaves; ++w) mm += shm[w][lane];
        sb.mtmp[(blockIdx.z * sb.passes + pass) * 16 + lane] = mm;
      }
    }
  }
}

// var = k(x,x) - sum over the row blocks (small_block_sum), GPy clip.  One
// workgroup per pass of 16 points and GP; mean / var are [G][P].
__global__ __launch_bounds__(256) void k_small_post(const GpDev* gps, SmallBufs sb,
                                                    int P, double* mean, double* var) {
  __shared__ double sh[16][16];
  const int g = blockIdx.y, pass = blockIdx.x;
  const GpDev& gp = gps[g];
  const double tot = small_block_sum(sb.part + g * sb.part_stride, sb.nblk_max,
                                     gp.nblk, pass, sh);
  const int p = pass * 16 + (threadIdx.x & 15);
  if ((threadIdx.x >> 4) == 0 && p < P) {
    mean[int64_t(g) * P + p] = sb.mtmp[g * sb.passes * 16 + p];
    var[int64_t(g) * P + p] = fmax(gp.kern.kdiag - tot, 1e-15);      // GPy clip
  }
}

bool small_path_pays(const sgp_gp* gp, int64_t P) {
  // The sweep needs >= 256 tiles of 64 rows to fill the chip; a tile walks
  // through all n^2 / 512 block products on one compute unit (n = 2000: 2.8 ms
  // whatever the number of tiles up to 512).  The few-points path spreads
  // (P / 16) x (n / 16) workgroups of a few microseconds each over the chip:
  // n = 2000, P = 2000: 0.3 ms.  Below n ~ 128 a tile is as short as the three
  // launches (measured crossover, scripts/dev/swarm_small.py: n between 50 and 200).
  return P >= 1 && P <= kSmallPoints && gp->n >= 128;
}

int small_reserve(sgp_ctx* ctx, const GpDev* gps_host, int G, int P, SmallBufs* sb) {
  int np_max = 0;
  for (int g = 0; g < G; ++g) np_max = std::max(np_max, gps_host[g].n_pad);
  sb->passes = (P + 15) / 16;
  sb->nsteps_max = np_max / 4;
  sb->nblk_max = np_max / 16;
  sb->kb_stride = int64_t(sb->passes) * sb->nsteps_max * 64;
  sb->part_stride = int64_t(sb->passes) * sb->nblk_max * 16;
  double* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotSmall,
                      size_t(G) * (sb->kb_stride + sb->part_stride + sb->passes * 16) * sizeof(double),
                      &buf));
  sb->Kb = buf;
  sb->part = buf + size_t(G) * sb->kb_stride;
  sb->mtmp = sb->part + size_t(G) * sb->part_stride;
  return 0;
}

// |L^-1 k(X, pts)|^2 per row block and alpha . k(X, pts) of all G GPs (two
// launches); `post` adds the block sums -> mean / var [G][P].
int posterior_small_all(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                        int G, const double* pts_rowmajor, int P, const SmallBufs& sb,
                        double* mean, double* var) {
  const int d = gps_host[0].kern.d;
  ctx->last_sweep = 4;
#define SMALL_CASE(DD)                                                         \
  case DD:                                                                     \
    hipLaunchKernelGGL(k_small_kb<DD>,                                         \
                       dim3((sb.nsteps_max * 64 + 255) / 256, sb.passes, G),   \
                       dim3(256), 0, ctx->stream, gps_dev, pts_rowmajor, P, sb);\
    break;
  switch (d) {
    SMALL_CASE(1) SMALL_CASE(2) SMALL_CASE(3) SMALL_CASE(4)
    SMALL_CASE(5) SMALL_CASE(6) SMALL_CASE(7) SMALL_CASE(8)
    default:
      sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
      return -2;
  }
#undef SMALL_CASE
  hipLaunchKernelGGL(k_small_mfma, dim3(sb.nblk_max, sb.passes, G),
                     dim3(64 * kSmallWaves), 0, ctx->stream, gps_dev, sb);
  if (mean && var)
    hipLaunchKernelGGL(k_small_post, dim3(sb.passes, G), dim3(256), 0, ctx->stream,
                       gps_dev, sb, P, mean, var);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
