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
//   dKy/dnoise = I
//
// k_lml_tiles: one workgroup per lower-triangular 64 x 64 tile of the (i, j) pairs.  Its four
// waves form the tile of Ky^-1 on the fp64 matrix cores (v_mfma_f64_16x16x4_f64: the A and
// the B operand are both rows of the dense L^-1, 16 consecutive doubles per k -- no packing)
// and contract it in registers with the evaluated derivative tile: neither Ky^-1 nor any
// dK/dtheta reaches memory.  Off-diagonal tiles count twice.  Every tile writes its
// 2 + P d sums to a slot of its own; k_lml_final adds the slots in a fixed order (no
// floating-point atomics: the same theta gives the same bits) together with the log and
// y^T alpha terms and writes the result block.
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

template <int D>
__global__ __launch_bounds__(256) void k_lml_tiles(KernDesc kd, const double* __restrict__ Li,
                                                   int64_t ld, int n,
                                                   const double* __restrict__ X,
                                                   const double* __restrict__ alpha,
                                                   double* __restrict__ part) {
  __shared__ double sh[4][kMaxAcc];
  int ti, tj;
  tile_of(blockIdx.x, &ti, &tj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = ti * kTile + 16 * wave, j0 = tj * kTile;
  const int col = lane & 15, kq = lane >> 4;

  // ---- Ky^-1 tile: rows i0 .. i0 + 15 of this wave x 64 columns ---------------------------
  // (L^-1)_ki = 0 for k < i: the sum starts at the wave's first row.  Rows k >= n and
  // columns >= n are never read (a bordered update may have left anything there).
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  const bool a_ok = i0 + col < n;
  bool b_ok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) b_ok[q] = j0 + 16 * q + col < n;
  constexpr int kInFlight = 4;           // k-steps whose loads are issued before the first use
  for (int k0 = i0; k0 < n; k0 += 4 * kInFlight) {
    double av[kInFlight], bv[kInFlight][4];
#pragma unroll
    for (int s = 0; s < kInFlight; ++s) {
      const int k = k0 + 4 * s + kq;
      const double* row = Li + int64_t(k) * ld;
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

  double xi[4][D], ai[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + kq + 4 * r;
    ai[r] = i < n ? alpha[i] : 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) xi[r][a] = i < n ? X[int64_t(i) * D + a] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + 16 * q + col;
    double xj[D];
    const double aj = j < n ? alpha[j] : 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) xj[a] = j < n ? X[int64_t(j) * D + a] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + kq + 4 * r;
      if (i >= n || j >= n) continue;
      const double w = fma(ai[r], aj, -acc[q][r]);
      if (i == j) s_noise += w;
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
#define LML_CASE(DD)                                                                       \
  case DD:                                                                                 \
    hipLaunchKernelGGL(k_lml_tiles<DD>, dim3(ntiles), dim3(256), 0, ctx->stream, gp->kern, \
                       Li, int64_t(gp->ld), n, X, alpha, part);                            \
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
