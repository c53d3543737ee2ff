// Joint posterior of N points: gp.predict_noiseless(Xnew, full_cov=True) and posterior
// sample paths (GPy: Posterior._raw_predict with full_cov, GP.posterior_samples_f).
//
//   V     = L^-1 k(X, X*)            (n_pad x N, k_joint_whiten)
//   mean  = k(X*, X) alpha           (the same kernel)
//   Sigma = k(X*, X*) - V^T V        (N x N,    k_joint_syrk)
//   C     = chol(Sigma + jitter I)   (factor_dense: the recursion that factorises Ky)
//   out   = mean 1^T + C Z           (k_joint_draw)
//
// Layout of V: row j = whitened training direction, pitch ldv = N rounded up to 64, the point
// index contiguous -- both MFMA operands of the SYRK (A[i][k] = V[k][i], B[k][j] = V[k][j]) are
// then runs of 16 consecutive doubles per k.  k_joint_whiten writes ALL of it: the rows n ..
// n_pad come out of the zero rows of Apack, the columns N .. ldv are stored as zeros.
//
// Device memory: the draw holds Sigma (-> C), the inverse factor the recursion produces along
// the way and its workspace, three N_pad x N_pad arrays (N_pad = N rounded up to 32): 1.6 GB at
// N = SGP_MAX_JOINT = 8192, plus V (n_pad x ldv).  predict_cov needs Sigma and V only.
//
// Every sum is formed in a fixed order (no atomics): same GP, same inputs, same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sweep_shared.h"

namespace {

// ---- V = L^-1 k(X, X*), mean = k(X*, X) alpha --------------------------------------------
// One workgroup = 64 points (16 per wave) x kWhitenRows row blocks of L^-1.  Per block of 16
// training points the covariances are evaluated ONCE, in the B-operand layout of
// v_mfma_f64_16x16x4_f64 (lane 16 k + c holds k(X_{4 s + k}, x_c)), and contracted with every
// row block of the group at or below that block (Apack is zero above the diagonal: those
// products are skipped, as in the sweeps).  The group that owns the last row block walks all
// training points and also forms the mean.
constexpr int kWhitenRows = 8;

template <int D>
__global__ __launch_bounds__(256) void k_joint_whiten(const GpDev* gps, const double* pts,
                                                      int N, double* V, int64_t ldv,
                                                      double* mean) {
  __shared__ double tab[kExpTabSize];
  exp_tab_init(tab);
  __syncthreads();
  const GpDev& gp = gps[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kq = lane >> 4;
  const int nblk = gp.nblk, nsteps = gp.n_pad / 4;
  const int b0 = blockIdx.y * kWhitenRows;
  const int bend = min(b0 + kWhitenRows, nblk);
  const int pt = blockIdx.x * 64 + wave * 16 + (lane & 15);     // < ldv
  const bool real = pt < N;
  KernFast<D> kf(gp.kern);
  double x[D], xs[D];
  {
    const int64_t pr = real ? pt : N - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = pts[pr * D + k];
  }
  kf.prep(x, xs);
  const bool with_mean = bend == nblk;
  const bool narrow = gp.narrow != 0;
  double4_t acc[kWhitenRows];
#pragma unroll
  for (int r = 0; r < kWhitenRows; ++r) acc[r] = double4_t{0.0, 0.0, 0.0, 0.0};
  double m = 0.0;
  for (int jb = 0; jb < bend; ++jb) {
    // b[s] = k(X_{16 jb + 4 s + kq}, x): the B operand of k-step 4 jb + s
    double b[4];
    kf.template many<4>(xs, gp.Xs + int64_t(16 * jb + kq) * D, 4 * D, tab, b);
    if (with_mean) {
#pragma unroll
      for (int s = 0; s < 4; ++s) m = fma(gp.alpha[16 * jb + 4 * s + kq], b[s], m);
    }
#pragma unroll
    for (int r = 0; r < kWhitenRows; ++r) {
      const int blk = b0 + r;
      if (blk < jb || blk >= bend) continue;          // (uniform over the workgroup)
      const double* A = gp.Apack + (int64_t(blk) * nsteps + 4 * jb) * 64 + lane;
      // narrow packing of the last row block (k_pack): its rows 4..15 repeat rows 0..3
      const bool dup = narrow && blk == nblk - 1 && (lane & 15) >= 4;
      double a[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = A[s * 64];
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(dup ? 0.0 : a[s], b[s], acc[r], 0, 0, 0);
    }
  }
  // D layout: column (point) = lane & 15, rows kq + 4 reg
#pragma unroll
  for (int r = 0; r < kWhitenRows; ++r) {
    const int blk = b0 + r;
    if (blk >= bend) continue;
    double* out = V + int64_t(16 * blk + kq) * ldv + pt;
    out[0] = real ? acc[r].x : 0.0;
    out[4 * ldv] = real ? acc[r].y : 0.0;
    out[8 * ldv] = real ? acc[r].z : 0.0;
    out[12 * ldv] = real ? acc[r].w : 0.0;
  }
  if (with_mean) {
    m = sum_lane_groups(m);
    if (lane < 16 && real) mean[pt] = m;
  }
}

// ---- Sigma = k(X*, X*) - V^T V ---------------------------------------------------------------
// One workgroup per 64 x 64 tile (bi >= bj) of Sigma, wave w = the 16 rows 16 w .. of the tile
// against its four 16-column blocks.  The accumulators START as the covariance tile (the C
// operand; the diagonal is the prior variance exactly, + diag_add), the A operand is -V, so
// the MFMAs subtract V^T V from it.  The two 16 x 64 panels of V of a stage go through LDS,
// double-buffered: the loads of stage c + 1 are in flight while stage c is multiplied.  Row
// pitch 80 doubles: the two k-rows a 32-lane half of ds_read_b64 touches lie 160 dwords
// apart, on opposite halves of the 64 banks.  The workgroup writes the entries with i >= j
// and their mirror images: Sigma is symmetric bit for bit.  Rows / columns N .. Np are the
// identity (the padding of the 32 x 32 factorisation leaves).
constexpr int kStageRows = 16;
constexpr int kPanelPitch = 80;

template <int D>
__global__ __launch_bounds__(256) void k_joint_syrk(const GpDev* gps, const double* pts, int N,
                                                    int Np, const double* V, int64_t ldv,
                                                    double diag_add, double* Sigma,
                                                    int64_t ld) {
  __shared__ double sA[2][kStageRows][kPanelPitch];
  __shared__ double sB[2][kStageRows][kPanelPitch];
  __shared__ double tab[kExpTabSize];
  exp_tab_init(tab);
  __syncthreads();
  const GpDev& gp = gps[0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, lc = lane & 15;
  // tile pair of the lower triangle: t = bi (bi + 1) / 2 + bj
  const int t = blockIdx.x;
  int bi = int((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  while (bi * (bi + 1) / 2 > t) --bi;
  const int bj = t - bi * (bi + 1) / 2;
  const int i0 = bi * 64, j0 = bj * 64;

  // C operand: the covariance tile
  KernFast<D> kf(gp.kern);
  const double kdiag = gp.kern.kdiag;
  double4_t acc[4];
  {
    double xi[4][D];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + 16 * wave + kq + 4 * reg;
      const int64_t ir = i < N ? i : N - 1;
      double x[D];
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = pts[ir * D + k];
      kf.prep(x, xi[reg]);
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int j = j0 + 16 * tt + lc;
      const int64_t jr = j < N ? j : N - 1;
      double x[D], xj[D];
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = pts[jr * D + k];
      kf.prep(x, xj);
      double c[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + 16 * wave + kq + 4 * reg;
        double v = kf(xi[reg], xj, tab);
        if (i == j) v = kdiag + diag_add;
        if (i >= N || j >= N) v = (i == j) ? 1.0 : 0.0;
        c[reg] = v;
      }
      acc[tt] = double4_t{c[0], c[1], c[2], c[3]};
    }
  }

  // panels: 16 rows x 64 columns each, two 16-byte pieces per thread and panel
  const int prow = tid >> 5, pcol = (tid & 31) * 2;        // rows prow and prow + 8
  const double* gA = V + int64_t(prow) * ldv + i0 + pcol;
  const double* gB = V + int64_t(prow) * ldv + j0 + pcol;
  const int nstages = gp.n_pad / kStageRows;
  double2_t ra[2], rb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ra[h] = *reinterpret_cast<const double2_t*>(gA + int64_t(8 * h) * ldv);
    rb[h] = *reinterpret_cast<const double2_t*>(gB + int64_t(8 * h) * ldv);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    *reinterpret_cast<double2_t*>(&sA[0][prow + 8 * h][pcol]) = ra[h];
    *reinterpret_cast<double2_t*>(&sB[0][prow + 8 * h][pcol]) = rb[h];
  }
  __syncthreads();
  for (int c = 0; c < nstages; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nstages;
    if (more) {
      const int64_t off = int64_t(c + 1) * kStageRows * ldv;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ra[h] = *reinterpret_cast<const double2_t*>(gA + off + int64_t(8 * h) * ldv);
        rb[h] = *reinterpret_cast<const double2_t*>(gB + off + int64_t(8 * h) * ldv);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const double a = -sA[buf][4 * s + kq][16 * wave + lc];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt)
        acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[buf][4 * s + kq][16 * tt + lc],
                                                       acc[tt], 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<double2_t*>(&sA[buf ^ 1][prow + 8 * h][pcol]) = ra[h];
        *reinterpret_cast<double2_t*>(&sB[buf ^ 1][prow + 8 * h][pcol]) = rb[h];
      }
    }
    __syncthreads();
  }

  // C/D map of v_mfma_f64_16x16x4_f64: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    const int j = j0 + 16 * tt + lc;
    const double v[4] = {acc[tt].x, acc[tt].y, acc[tt].z, acc[tt].w};
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = i0 + 16 * wave + kq + 4 * reg;
      if (i < Np && j < Np && i >= j) {
        Sigma[int64_t(i) * ld + j] = v[reg];
        if (i != j) Sigma[int64_t(j) * ld + i] = v[reg];
      }
    }
  }
}

// ---- out = mean 1^T + C Z ----------------------------------------------------------------------
// C lower triangular (the upper part of the array is never read), Z and out (N x S)
// row-major.  One wave per row and 16 columns of Z; the lanes stride over j, then a fixed
// butterfly.
constexpr int kDrawCols = 16;

__global__ __launch_bounds__(256) void k_joint_draw(const double* C, int64_t ld, int N,
                                                    const double* Z, int S, const double* mean,
                                                    double* out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int s0 = blockIdx.y * kDrawCols;
  if (i >= N) return;
  const int ns = min(kDrawCols, S - s0);
  double acc[kDrawCols];
#pragma unroll
  for (int q = 0; q < kDrawCols; ++q) acc[q] = 0.0;
  const double* row = C + int64_t(i) * ld;
  for (int j = lane; j <= i; j += 64) {
    const double c = row[j];
    const double* z = Z + int64_t(j) * S + s0;
#pragma unroll
    for (int q = 0; q < kDrawCols; ++q)
      if (q < ns) acc[q] = fma(c, z[q], acc[q]);
  }
  const double mu = mean[i];
#pragma unroll
  for (int q = 0; q < kDrawCols; ++q) {
    if (q < ns) {
      double v = acc[q];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) out[int64_t(i) * S + s0 + q] = mu + v;
    }
  }
}

// A/B yardstick (SGP_JOINT_SYRK=valu): Vt[i][r] = V[r][i], the row-major left operand the
// VALU GEMM of the factorisation wants.
__global__ void k_joint_transpose(const double* V, int64_t ldv, int rows, int N, double* Vt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y * blockDim.y + threadIdx.y;
  if (i < N && r < rows) Vt[int64_t(i) * rows + r] = V[int64_t(r) * ldv + i];
}

template <int D>
void launch_whiten_d(sgp_ctx* ctx, const GpDev* gdev, const GpDev& gh, const double* pts, int N,
                     double* V, int64_t ldv, double* mean) {
  const dim3 grid(unsigned(ldv / 64), unsigned((gh.nblk + kWhitenRows - 1) / kWhitenRows));
  hipLaunchKernelGGL(k_joint_whiten<D>, grid, dim3(256), 0, ctx->stream, gdev, pts, N, V, ldv,
                     mean);
}

template <int D>
void launch_syrk_d(sgp_ctx* ctx, const GpDev* gdev, const double* pts, int N, int Np,
                   const double* V, int64_t ldv, double diag_add, double* Sigma, int64_t ld) {
  const int tiles = int(ldv / 64);
  hipLaunchKernelGGL(k_joint_syrk<D>, dim3(unsigned(tiles * (tiles + 1) / 2)), dim3(256), 0,
                     ctx->stream, gdev, pts, N, Np, V, ldv, diag_add, Sigma, ld);
}

#define JOINT_DISPATCH(d, call)                                                    \
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

// The device side of one joint prediction: staged points, V, mean and (on request) Sigma.
struct JointBufs {
  int N, Np;          // points; rounded up to 32 (= pitch of Sigma / Li / T)
  int64_t ldv;        // N rounded up to 64
  double* pts;        // [N][d]
  GpDev* gdev;
  double* V;          // [n_pad][ldv]
  double* mean;       // [N]
  double* diag;       // [N] diagonal of Sigma at jitter 0 (draw)
  int* info;          // pivot word of the factorisation
  double* Sigma;      // [Np][Np]
};

int joint_stage(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                int64_t stride_col, bool want_sigma, JointBufs* jb) {
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  jb->N = int(N);
  jb->Np = int((N + 31) / 32) * 32;
  jb->ldv = (N + 63) / 64 * 64;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(N) * d * sizeof(double), &jb->pts));
  SGP_TRY(sgp_scratch(ctx, kSlotGpDev, sizeof(GpDev), &jb->gdev));
  SGP_TRY(sgp_scratch(ctx, kSlotWork, size_t(gp->n_pad) * jb->ldv * sizeof(double), &jb->V));
  SGP_TRY(sgp_scratch(ctx, kSlotSmall, (2 * size_t(N) + 1) * sizeof(double), &jb->mean));
  jb->diag = jb->mean + N;
  jb->info = reinterpret_cast<int*>(jb->diag + N);
  jb->Sigma = nullptr;
  if (want_sigma)
    SGP_TRY(sgp_scratch(ctx, kSlotJointA, size_t(jb->Np) * jb->Np * sizeof(double), &jb->Sigma));
  // one dense row-major copy whatever the strides: the same bits for every layout
  std::vector<double> tmp(size_t(N) * d);
  for (int64_t r = 0; r < N; ++r)
    for (int k = 0; k < d; ++k) tmp[size_t(r) * d + k] = Xnew[r * stride_row + k * stride_col];
  SGP_TRY(sgp_h2d(ctx, jb->pts, tmp.data(), tmp.size() * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, jb->gdev, &gp->dev, sizeof(GpDev)));
  return 0;
}

int joint_whiten(sgp_gp* gp, const JointBufs& jb) {
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 1.0 * gp->n * gp->n * jb.N));
#define CALL(DD) launch_whiten_d<DD>(ctx, jb.gdev, gp->dev, jb.pts, jb.N, jb.V, jb.ldv, jb.mean)
  JOINT_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}

// The same Sigma from the kernels the factorisation already has: k(X*, X*) written out, then
// the VALU k_gemm of factor.hip for the N x N x n product (all of it: it knows no triangle).
// The only other kernel in the library that can form this product, kept as the yardstick of
// k_joint_syrk (scripts/bench_joint.py); the two triangles are equal within rounding only.
int joint_syrk_valu(sgp_gp* gp, const JointBufs& jb, double diag_add) {
  sgp_ctx* ctx = gp->ctx;
  const int np = gp->n_pad;
  double* Vt;
  SGP_TRY(sgp_scratch(ctx, kSlotJointVt, size_t(jb.N) * np * sizeof(double), &Vt));
  hipLaunchKernelGGL(k_joint_transpose, dim3(unsigned((jb.N + 63) / 64), unsigned((np + 3) / 4)),
                     dim3(64, 4), 0, ctx->stream, jb.V, jb.ldv, np, jb.N, Vt);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(launch_kernel_matrix(ctx, gp->kern, jb.pts, jb.Np, jb.pts, jb.Np, jb.Sigma, jb.Np, 1,
                               diag_add, jb.N));
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 1.0 * jb.N * jb.N * gp->n));
  SGP_TRY(gemm_dense(ctx, false, jb.N, jb.N, np, -1.0, Vt, np, jb.V, jb.ldv, 1.0, jb.Sigma,
                     jb.Np));
  return tm.end(ctx);
}

int joint_syrk(sgp_gp* gp, const JointBufs& jb, double diag_add) {
  sgp_ctx* ctx = gp->ctx;
  const int d = gp->kern.d;
  static const bool valu = getenv("SGP_JOINT_SYRK") && !strcmp(getenv("SGP_JOINT_SYRK"), "valu");
  if (valu) return joint_syrk_valu(gp, jb, diag_add);
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 1.0 * jb.N * jb.N * gp->n));
#define CALL(DD) \
  launch_syrk_d<DD>(ctx, jb.gdev, jb.pts, jb.N, jb.Np, jb.V, jb.ldv, diag_add, jb.Sigma, jb.Np)
  JOINT_DISPATCH(d, CALL)
#undef CALL
  SGP_HIP(ctx, hipGetLastError());
  return tm.end(ctx);
}

}  // namespace

int joint_predict_cov(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                      int64_t stride_col, double* mean, double* cov) {
  sgp_ctx* ctx = gp->ctx;
  JointBufs jb;
  SGP_TRY(joint_stage(gp, Xnew, N, stride_row, stride_col, cov != nullptr, &jb));
  SGP_TRY(joint_whiten(gp, jb));
  if (cov) {
    SGP_TRY(joint_syrk(gp, jb, 0.0));
    SGP_HIP(ctx, hipMemcpy2DAsync(cov, size_t(N) * sizeof(double), jb.Sigma,
                                  size_t(jb.Np) * sizeof(double), size_t(N) * sizeof(double),
                                  size_t(N), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (mean) return sgp_d2h(ctx, mean, jb.mean, size_t(N) * sizeof(double));
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int joint_posterior_draw(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                         int64_t stride_col, const double* Z, int S, double* out, double* mean,
                         int* chol_info, double* jitter_used) {
  sgp_ctx* ctx = gp->ctx;
  JointBufs jb;
  SGP_TRY(joint_stage(gp, Xnew, N, stride_row, stride_col, true, &jb));
  const size_t mat = size_t(jb.Np) * jb.Np * sizeof(double);
  double *Li, *T, *zo;
  SGP_TRY(sgp_scratch(ctx, kSlotJointLi, mat, &Li));
  SGP_TRY(sgp_scratch(ctx, kSlotJointT, mat, &T));
  SGP_TRY(sgp_scratch(ctx, kSlotJointZ, 2 * size_t(N) * S * sizeof(double), &zo));
  SGP_TRY(joint_whiten(gp, jb));
  // Sigma + jitter I -> C in the lower part of jb.Sigma.  A failed attempt has overwritten
  // Sigma: every attempt forms it again (the retries are the rare case).
  auto attempt = [&](double jitter, int* info) -> int {
    SGP_TRY(joint_syrk(gp, jb, jitter));
    if (jitter == 0.0)
      SGP_HIP(ctx, hipMemcpy2DAsync(jb.diag, sizeof(double), jb.Sigma,
                                    size_t(jb.Np + 1) * sizeof(double), sizeof(double),
                                    size_t(N), hipMemcpyDeviceToDevice, ctx->stream));
    SGP_HIP(ctx, hipMemsetAsync(Li, 0, mat, ctx->stream));
    SGP_HIP(ctx, hipMemsetAsync(jb.info, 0, sizeof(int), ctx->stream));
    SweepTimer tm;
    SGP_TRY(tm.begin(ctx, 1.0 * N * N * N / 3.0));
    SGP_TRY(factor_dense(ctx, jb.Sigma, Li, T, jb.Np, jb.Np, jb.info));
    SGP_TRY(tm.end(ctx));
    return sgp_d2h(ctx, info, jb.info, sizeof(int));
  };
  auto diag_mean = [&](double* dm) -> int {
    std::vector<double> dg(static_cast<size_t>(N), 0.0);
    SGP_TRY(sgp_d2h(ctx, dg.data(), jb.diag, size_t(N) * sizeof(double)));
    double s = 0.0;
    for (double v : dg) s += v;
    *dm = s / double(N);
    return 0;
  };
  int info = 0;
  double jitter = 0.0;
  SGP_TRY(jitchol_loop(diag_mean, attempt, &info, &jitter));
  if (chol_info) *chol_info = info;
  if (jitter_used) *jitter_used = jitter;
  if (info != 0) {
    sgp_set_error(ctx, "joint covariance not positive definite, even with jitter (pivot %d)",
                  info);
    return info > 0 ? info : -2;
  }
  double* zdev = zo;
  double* odev = zo + size_t(N) * S;
  SGP_TRY(sgp_h2d(ctx, zdev, Z, size_t(N) * S * sizeof(double)));
  SweepTimer tm;
  SGP_TRY(tm.begin(ctx, 1.0 * N * N * S));
  hipLaunchKernelGGL(k_joint_draw, dim3(unsigned((N + 3) / 4), unsigned((S + kDrawCols - 1) / kDrawCols)),
                     dim3(256), 0, ctx->stream, jb.Sigma, int64_t(jb.Np), int(N), zdev, S, jb.mean,
                     odev);
  SGP_HIP(ctx, hipGetLastError());
  SGP_TRY(tm.end(ctx));
  SGP_TRY(sgp_d2h(ctx, out, odev, size_t(N) * S * sizeof(double)));
  if (mean) SGP_TRY(sgp_d2h(ctx, mean, jb.mean, size_t(N) * sizeof(double)));
  return 0;
}
