/*
 * safeopt_hip.h -- C ABI of libsafeopt_hip.so (MI355X / gfx950, HIP + RCCL).
 *
 * The drop-in boundary for SafeOpt's GP-posterior + safe-set hot path.  The
 * reference (befelix/SafeOpt, pure Python) has no FFI; its seam is the
 * duck-typed "GPy model" handle plus the NumPy sweep in safeopt/gp_opt.py.
 * Every entry point below names the reference call site(s) it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes stub
 * a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no C++ / torch types.
 *   - every function returns 0 on success; <0 = HIP/RCCL/runtime error,
 *     >0 = numerical failure (e.g. Cholesky info).  sgp_last_error() gives
 *     the message.  No exception crosses the ABI.
 *   - all host buffers are borrowed for the duration of the call only;
 *     outputs go to caller-allocated buffers.  All real data is float64,
 *     masks are uint8 (NumPy bool), indices int64.
 *   - one sgp_ctx per (process, device); calls on one ctx are serialised by
 *     the caller (the reference is single-threaded too).
 */
#ifndef SAFEOPT_HIP_H
#define SAFEOPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGP_MAX_D 8        /* input dimension incl. context columns            */
#define SGP_MAX_PARTS 4    /* factors of a product kernel                      */
#define SGP_MAX_GPS 8      /* objective + constraints                          */
#define SGP_TOPK 16        /* expander candidates examined per pass            */
#define SGP_MAX_JOINT 8192 /* rows of one joint prediction                     */
#define SGP_MAX_PATHS 64   /* sample paths of one call                         */
#define SGP_MAX_FEATURES 16384 /* random Fourier features of a sample path     */
#define SGP_MAX_BATCH 64   /* query points of one hallucinated batch           */
#define SGP_MAX_MES 64     /* maxima of one max-value entropy search (= SGP_MAX_PATHS) */
#define SGP_MAX_BLOCK 16   /* observations of one block append                 */
#define SGP_MAX_ISE 4096   /* candidates of one information-theoretic safe exploration */

/* kernel kinds: GPy.kern.RBF / Matern32 / Matern52 (Stationary.K_of_r)        */
enum { SGP_RBF = 0, SGP_MATERN32 = 1, SGP_MATERN52 = 2 };
/* sgp_grid_download selectors                                                 */
enum { SGP_Q = 0, SGP_S = 1, SGP_M = 2, SGP_G = 3, SGP_MEAN = 4, SGP_VAR = 5,
       SGP_CAND = 6, SGP_WIDTH = 7, SGP_VAR_H = 8 };
/* sgp_grid_argmax modes                                                       */
enum { SGP_ARGMAX_MG_WIDTH = 0, SGP_ARGMAX_UCB = 1, SGP_ARGMAX_LCB = 2 };
/* sgp_swarm_fitness swarm types (gp_opt.py:901-1013)                          */
enum { SGP_SWARM_GREEDY = 0, SGP_SWARM_MAXIMIZERS = 1, SGP_SWARM_EXPANDERS = 2,
       SGP_SWARM_SAFE_SET = 3 };

typedef struct sgp_ctx sgp_ctx;   /* device, stream, scratch, RCCL communicator */
typedef struct sgp_gp sgp_gp;     /* one GP: data, L^-1 (packed), alpha         */
typedef struct sgp_grid sgp_grid; /* resident candidate rows + Q/S/M/G          */

/* ---- context ---------------------------------------------------------------*/
int sgp_device_count(int* n);
int sgp_create(int device, sgp_ctx** out);
void sgp_destroy(sgp_ctx* ctx);
/* message of the last failing call on ctx (ctx may be NULL: process-global)   */
const char* sgp_last_error(sgp_ctx* ctx);
int sgp_sync(sgp_ctx* ctx);

/* ---- GP handle: replaces GPy.models.GPRegression as SafeOpt uses it --------
 * kernel = product over n_parts of  variance_p * k_kind_p(r_p),
 * r_p^2 = sum_k ((x_k - x'_k) * inv_ls[p*d + k])^2   (inv_ls = 0 on columns
 * outside the part's active_dims; = 1/lengthscale otherwise).               */
int sgp_gp_create(sgp_ctx* ctx, int d, int n_parts, const int* kinds,
                  const double* variances, const double* inv_ls,
                  double noise_var, sgp_gp** out);
void sgp_gp_destroy(sgp_gp* gp);
/* gp.set_XY (gp_opt.py:227, 267, 275): K = k(X,X), Ky = K + (noise+1e-8) I,
 * L = jitchol(Ky), L^-1, alpha = Ky^-1 Y -- all on the device.  X is (n,d)
 * row-major, Y is (n).  chol_info: 0 ok, k>0 = pivot k not positive even
 * after 5 jitter escalations (GPy jitchol); jitter_used: diagonal jitter.    */
int sgp_gp_set_data(sgp_gp* gp, const double* X, const double* Y, int64_t n,
                    int* chol_info, double* jitter_used);
/* gp.set_XY with ONE more / ONE fewer row -- what add_new_data_point
 * (gp_opt.py:230-255 -> :227) and remove_last_data_point (:269-278 -> :275) do
 * every iteration: bordered update of L^-1 and alpha, O(n^2) instead of the
 * O(n^3) re-factorisation.  append: info = 0 ok,
 * > 0 the bordered pivot is not positive (refit with sgp_gp_set_data, which
 * applies GPy's jitter), -1 no spare capacity (same remedy).                  */
int sgp_gp_append(sgp_gp* gp, const double* x, double y, int* info);
int sgp_gp_pop(sgp_gp* gp);
/* b observations at once (X (b,d) row-major, y (b), 1 <= b <= SGP_MAX_BLOCK): the bordered
 * update with a b x b corner.  With n0 = n, Kc = k(X_old, X), T = L^-1 Kc,
 * W = L^-T T:  C = k(X, X) + (noise + 1e-8 + jitter) I - T^T T = Lc Lc^T, rows n0 .. n0+b-1
 * of the dense L^-1 become Lc^-1 [ -W^T | I ], gamma_j = (row n0+j) . y, and
 * alpha <- [alpha; 0] + sum_j (row n0+j)^T gamma_j.  One read-back, one re-pack of the sweep
 * operands; every sum in a fixed order.  info = 0 ok; n0 + j + 1: pivot j of C fails the test
 * of sgp_gp_append (s2_j > 1e-12 (k(x,x) + noise + 1e-8 + jitter), finite); -1: n + b exceeds
 * the row capacity -- in both cases the GP is exactly as it was (refit with
 * sgp_gp_set_data).  On success the GP carries the BLOCK RECORD {b, n0, gamma} for
 * sgp_grid_rankb_update instead of a one-row record; any other change of the GP drops it, a
 * clone carries none.  The host bookkeeping (shared factors) is that of b sgp_gp_append.   */
int sgp_gp_append_block(sgp_gp* gp, const double* X, const double* y, int b, int* info);
/* Forget training row `index` (0 .. n-1, n >= 2), whichever it is: an O(n^2) downdate of
 * L^-1 and alpha instead of the refit gp.set_XY would cost (the reference has only
 * remove_last_data_point).  With M = L^-1, c = column index of M, P_ii = |c|^2 and
 * p = M^T c:  w = -p_{-i} / P_ii,  alpha_new = alpha_{-i} + w alpha_i, and L_new^-1 = M
 * without column i after the rotations that fold c_k into c_i, k = i+1 .. n-1 (DESIGN.md
 * 4.4a).  Kernel, noise, jitter and row capacity of the fit stay.  Every sum is formed in a
 * fixed order: the same inputs give the same bits.  It leaves the record of the removal
 * {w, alpha_i, P_ii, x_i} for sgp_grid_rank1_remove -- also for index == n-1, unlike
 * sgp_gp_pop.  info = 0 ok; > 0: P_ii or a rotation is not positive and finite -- the GP
 * is untouched (refit the reduced data with sgp_gp_set_data).  An index outside 0 .. n-1,
 * n == 1 and a GP that is not fitted are errors.                                          */
int sgp_gp_remove(sgp_gp* gp, int64_t index, int* info);
/* Per-observation noise.  Observation i has a NOISE SCALE r_i > 0:
 *   Ky = K + diag((noise_var + 1e-8) r_i) + jitter I       (the jitter is not scaled).
 * A GP that never received a scale holds none, runs the code without scales and returns its
 * bits; r = NULL below means all ones and takes that path, and all ones given explicitly
 * give the same bits.  k measurements (y_j, rho_j) at one input are, for the posterior, ONE
 * observation with r = 1 / sum 1/rho_j and y = r sum y_j / rho_j.  sgp_gp_remove, sgp_gp_pop
 * and sgp_gp_clone carry the scales along; GPs with different scales share no factor; the
 * noise slot of sgp_gp_lml / sgp_gp_loo_lml is the derivative in noise_var with
 * dKy/dnoise_var = diag(r).  A scale that is not finite or not positive is an error, and
 * nothing is written.
 * sgp_gp_set_data_w: sgp_gp_set_data with the n scales r (or NULL).                        */
int sgp_gp_set_data_w(sgp_gp* gp, const double* X, const double* Y, const double* r,
                      int64_t n, int* chol_info, double* jitter_used);
/* sgp_gp_append with the scale *r of the new row (r = NULL: 1); the pivot rule uses the
 * row's own diagonal k(x,x) + (noise + 1e-8) r + jitter.                                   */
int sgp_gp_append_w(sgp_gp* gp, const double* x, double y, const double* r, int* info);
/* sgp_gp_append_block with the b scales of the new rows (or NULL) on the corner's diagonal. */
int sgp_gp_append_block_w(sgp_gp* gp, const double* X, const double* y, const double* r,
                          int b, int* info);
/* Observation `index` (0 .. n-1) becomes (y_new, r_new) IN PLACE: Ky' = Ky + delta e_i e_i^T
 * with delta = (noise + 1e-8) (r_new - r_i), y_i -> y_i + dy.  n and the inputs stay.  With
 * M = L^-1, c = column i of M, P_ii = |c|^2, p = M^T c:
 *   tau = delta / (1 + delta P_ii),  eta = (dy - delta alpha_i) / (1 + delta P_ii),
 *   alpha' = alpha + eta p,  L'^-1 = F M with F lower triangular, F^T F = I - tau c c^T:
 *   q_k = 1 + delta sum_{i <= j <= k} c_j^2,
 *   row k of L'^-1 = sqrt(q_{k-1} / q_k) M[k] - delta c_k / sqrt(q_{k-1} q_k) sum_{i<=j<k} c_j M[j]
 * for k = i .. n-1; the rows above i stay.  O(n^2), written into the spare matrix and
 * committed after the pivot word has been read; every sum in a fixed order (the same inputs
 * give the same bits).  It leaves the REWEIGH RECORD {x_i, w = -p / P_ii off row i,
 * P_ii eta, tau P_ii^2} for sgp_grid_rank1_reweigh.  info = 0 ok; > 0: P_ii or a q_k is not
 * positive and finite -- the GP is untouched (refit with sgp_gp_set_data_w).  An index
 * outside 0 .. n-1, a y_new that is not finite, a scale that is not finite or not positive
 * and a GP that is not fitted are errors; nothing is written.                              */
int sgp_gp_reweigh(sgp_gp* gp, int64_t index, double y_new, double r_new, int* info);
/* The n noise scales as the device holds them (ones for a GP without scales): a test hook. */
int sgp_gp_get_noise_scale(sgp_gp* gp, double* r_out);
/* gp.predict_noiseless / gp._raw_predict (gp_opt.py:469, 591, 929, 973, 1117,
 * 1132; utilities.py:203, 282, 355).  Xnew element (r,c) at
 * Xnew[r*stride_row + c*stride_col] (strides in elements: C or F order).
 * var is clipped to [1e-15, inf) like GPy.                                   */
int sgp_gp_predict(sgp_gp* gp, const double* Xnew, int64_t N,
                   int64_t stride_row, int64_t stride_col, double* mean,
                   double* var);
/* An edited hyper-parameter (kern.variance / kern.lengthscale / noise_var written in
 * place; GPy refits through its parameter observers): the kernel descriptor of the GP is
 * rewritten in place -- same d, kinds and number of parts; variances[n_parts],
 * inv_ls[n_parts * d] as in sgp_gp_create -- and the RESIDENT data are factorised again.
 * No buffer is reallocated and X / Y are not uploaded again.  Jitter retries, chol_info
 * and jitter_used as sgp_gp_set_data (on failure the GP has no data any more).      */
int sgp_gp_set_hyper(sgp_gp* gp, const double* variances, const double* inv_ls,
                     double noise_var, int* chol_info, double* jitter_used);
/* gp.log_likelihood() and its gradient (GPy: ExactGaussianInference,
 * Stationary.update_gradients_full) at a full set of hyper-parameters, in one device ->
 * host copy.  As sgp_gp_set_hyper, but WITHOUT jitter retries (jitter = 0): *info = 0, or
 * the first non-positive pivot of Ky = K + (noise_var + 1e-8) I -- that theta is
 * infeasible, `out` is meaningless and the GP stays unfitted (data resident) until the
 * next sgp_gp_lml / sgp_gp_set_hyper / sgp_gp_set_data succeeds.  With P = n_parts:
 *   out[0]                log p(y | X, theta) = -1/2 y^T alpha - sum_i log L_ii - n/2 log 2 pi
 *   out[1]                d/d noise_var
 *   out[2 .. 2+P)         d/d variance[p]
 *   out[2+P .. 2+P+P*d)   d/d inv_ls[p*d + a]   (0 for a column the part does not use)
 * The gradient is 1/2 sum_ij W_ij dKy_ij/dtheta, W = alpha alpha^T - Ky^-1,
 * Ky^-1 = L^-T L^-1.  With s = inv_ls[p][a], D_a = x_ia - x_ja,
 * r_p^2 = sum_a (D_a s_pa)^2 and k = prod_p v_p f_p(r_p):
 *   dk/dv_p = k / v_p,   dKy/dnoise_var = I,   dk/ds_pa = (k / f_p) c_p(r_p) D_a^2 s_pa,
 *   RBF        f = exp(-r^2/2)                              c = -f
 *   Matern-3/2 f = (1 + sqrt3 r) exp(-sqrt3 r)              c = -3 exp(-sqrt3 r)
 *   Matern-5/2 f = (1 + sqrt5 r + 5 r^2/3) exp(-sqrt5 r)    c = -5/3 (1 + sqrt5 r) exp(-sqrt5 r)
 * (exact at r = 0).  The sums are formed in a fixed order: the same theta on the same
 * data returns the same bits.  On success the GP is fitted at theta.               */
int sgp_gp_lml(sgp_gp* gp, const double* variances, const double* inv_ls,
               double noise_var, double* out, int* info);
/* Leave-one-out predictions of a fitted GP (Rasmussen & Williams 5.4.2), every observation
 * predicted from all the others, in closed form from the resident L^-1 and alpha -- O(n^2)
 * for all n together, whatever appends and removals led to the factor:
 *   P_ii = (Ky^-1)_ii = sum_{k >= i} (L^-1)_ki^2
 *   mean[i] = y_i - alpha_i / P_ii
 *   var[i]  = 1 / P_ii      (of the NOISY y_i: noise_var + 1e-8 + jitter included)
 *   *sum_log_pred = sum_i [ -1/2 log var[i] - 1/2 (y_i - mean[i])^2 / var[i] - 1/2 log 2 pi ]
 * n = 1 gives the prior: mean 0, var Ky_11.  *info = 0, or i + 1 for the first P_ii that
 * is not positive and finite -- nothing is written then.  Deterministic: the column sums
 * are formed in a fixed order.  A GP that is not fitted is an error.                     */
int sgp_gp_loo(sgp_gp* gp, double* mean, double* var, double* sum_log_pred, int* info);
/* The leave-one-out log pseudo-likelihood L_LOO (= *sum_log_pred of sgp_gp_loo) and its
 * gradient at a full set of hyper-parameters: arguments, result block, jitter = 0 and the
 * contract of sgp_gp_lml -- the data are factorised at theta; *info = the first non-positive
 * pivot (or the first P_ii that is not positive and finite) leaves the GP unfitted with its
 * data resident, otherwise the GP is fitted at theta:
 *   out[0]                L_LOO
 *   out[1]                d/d noise_var
 *   out[2 .. 2+P)         d/d variance[p]
 *   out[2+P .. 2+P+P*d)   d/d inv_ls[p*d + a]   (0 for a column the part does not use)
 * The gradient is sum_ij G_ij dKy_ij/dtheta (R&W eq. 5.13 rearranged), with
 *   a_i = alpha_i / P_ii,   b_i = 1/2 (1 + alpha_i^2 / P_ii) / P_ii,   u = Ky^-1 a,
 *   G = 1/2 (u alpha^T + alpha u^T) - C^T C,   C = diag(sqrt(b)) Ky^-1,
 * and dKy/dtheta as for sgp_gp_lml.  Deterministic.  Device memory: C, n x n doubles (n
 * rounded up to 64 in one direction), in scratch of the CONTEXT: it grows to the largest n
 * asked for and stays allocated after the call, until sgp_destroy -- 33 MB once n = 2000
 * has been evaluated, 2.1 GB at the 16384 observations a GP can hold.                      */
int sgp_gp_loo_lml(sgp_gp* gp, const double* variances, const double* inv_ls,
                   double noise_var, double* out, int* info);
/* gp.predict_noiseless(Xnew, full_cov=True) (GPy: Posterior._raw_predict): mean (N), cov
 * (N x N row-major, exactly symmetric).  cov = k(X*,X*) - V^T V, V = L^-1 k(X,X*); its
 * diagonal is NOT clipped (GPy clips only the full_cov=False variance).  Strides as
 * sgp_gp_predict; N <= SGP_MAX_JOINT.  cov may be NULL (mean only), mean may be NULL.
 * Deterministic: the sums are formed in a fixed order.  Device memory: V (n x N) and cov.  */
int sgp_gp_predict_cov(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                       int64_t stride_col, double* mean, double* cov);
/* gp.posterior_samples_f(Xnew, size=S) with the caller's normals: out (N x S row-major) =
 * mean 1^T + C Z, C the lower Cholesky factor of cov + jitter_used * I, Z (N x S row-major).
 * Jitter as GPy's jitchol / sgp_gp_set_data: 0 first, then mean(diag cov) * 1e-6, times 10
 * per retry, five retries; chol_info > 0 (also the return value) = pivot still not
 * positive, out is then not written.  mean may be NULL.  Deterministic.  Device memory:
 * three N_pad x N_pad arrays, N_pad = N rounded up to 32 -- 1.6 GB at N = SGP_MAX_JOINT.   */
int sgp_gp_posterior_draw(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                          int64_t stride_col, const double* Z, int S, double* out,
                          double* mean, int* chol_info, double* jitter_used);
/* ---- posterior sample PATHS by pathwise conditioning (Wilson et al. 2020, "Efficiently
 * sampling functions from Gaussian process posteriors").  A path is a function: a random-
 * Fourier-feature draw from the prior plus a kernel-weighted update from the data,
 *   phi_i(x)   = sqrt(2 v / m) cos(omega_i . x + b_i)        i = 1 .. m,  v = prod_p v_p
 *   prior_s(x) = sum_i W[i,s] phi_i(x)
 *   V[:,s]     = alpha - Ky^-1 (Phi(X) W[:,s] + E[:,s])      Phi(X)[j,i] = phi_i(X_j)
 *   f_s(x)     = prior_s(x) + sum_j k(x, X_j) V[j,s]
 * with Ky = K + (noise_var + 1e-8) I (+ the jitter of the fit), L and alpha of the GP as they
 * stand.  O(m + n) per row and path, no N x N matrix (sgp_gp_posterior_draw stops at
 * SGP_MAX_JOINT rows), evaluated anywhere, any number of times.  The caller brings the random
 * numbers (safeopt_amd/paths.py draws them with NumPy): Omega (m x d row-major; omega_i = the
 * sum over the parts of a draw from the part's spectral measure), phase (m; uniform on
 * [0, 2 pi)), W (m x S row-major; standard normal), E (n x S row-major; normal with variance
 * noise_var + 1e-8).  1 <= m <= SGP_MAX_FEATURES, 1 <= S <= SGP_MAX_PATHS; the GP must be
 * fitted.  Every sum is formed in a fixed order (no atomics): the same inputs give the same
 * bits, and a row's values do not depend on the other rows of the call.
 *
 * sgp_gp_path_weights: V_out (n x S row-major).  Phi(X) W is formed by the kernel that
 * evaluates the paths, with the training rows as the points; Ky^-1 is applied as
 * L^-T (L^-1 u) from the resident dense L^-1.                                            */
int sgp_gp_path_weights(sgp_gp* gp, const double* Omega, const double* phase, int m,
                        const double* W, const double* E, int S, double* V_out);
/* out (N x S row-major) = f_s at the rows of Xnew (strides as sgp_gp_predict; N is not
 * limited; N <= 0 returns 0 and writes nothing).  One kernel: [Phi(x) | k(x, X)] times
 * [W ; V] on the fp64 matrix pipe, the features and covariances evaluated on the fly.     */
int sgp_gp_paths_eval(sgp_gp* gp, const double* Omega, const double* phase, int m,
                      const double* W, const double* V, int S, const double* Xnew, int64_t N,
                      int64_t stride_row, int64_t stride_col, double* out);
/* test hook: dense L^-1 (n x n, row-major) and alpha (n)                     */
int sgp_gp_get_factor(sgp_gp* gp, double* Linv, double* alpha);
/* A second GP with the state of src, device to device: kernel, noise, jitter, training data,
 * L^-1, alpha, the record of the last append, and row capacity for at least SGP_MAX_BATCH
 * one-row appends.  The packed operands are formed again from the copied L^-1 by the kernels
 * that formed the source's: the clone predicts the bits of src.  It is appended to, refitted
 * and destroyed independently of src (src is only read, and may be destroyed first); clones of
 * GPs that share a factor (sgp_ctx_set_share) share among themselves after equal appends.
 * What SafeOpt.optimize_batch appends its pending picks to: sgp_gp_append followed by
 * sgp_gp_pop does not give a GP back bit for bit (pop recomputes alpha).                 */
int sgp_gp_clone(sgp_gp* src, sgp_gp** out);
/* gp.kern.K(X, X2) (gp_opt.py:847, 1093; utilities.py:89, 135): out is
 * (n1,n2) row-major; X1 (n1,d), X2 (n2,d) row-major.                         */
int sgp_kern_K(sgp_ctx* ctx, int d, int n_parts, const int* kinds,
               const double* variances, const double* inv_ls, const double* X1,
               int64_t n1, const double* X2, int64_t n2, double* out);

/* ---- resident candidate grid: SafeOpt.inputs / Q / S / M / G ----------------
 * (gp_opt.py:358-390).  `base` element (r,c) at byte offset
 * r*stride_row_B + c*stride_col_B (the stock grid is F-ordered); rows are
 * this rank's shard, global index = global_offset + local row.               */
int sgp_grid_create(sgp_ctx* ctx, const double* base, int64_t N, int d,
                    int64_t stride_row_B, int64_t stride_col_B, int G,
                    int64_t global_offset, sgp_grid** out);
void sgp_grid_destroy(sgp_grid* grid);
/* SafeOpt.context setter (gp_opt.py:439-451): fill the last nc columns       */
int sgp_grid_set_context(sgp_grid* grid, const double* c, int nc);
/* Declares the rows a TENSOR grid, which is what SafeOpt's parameter_set is
 * (linearly_spaced_combinations, utilities.py:21-54, followed by constant context
 * columns, gp_opt.py:439-451): global row i has column k equal to
 * values_k[(i / stride[k]) % count[k]], values = the d axes concatenated (count[k]
 * doubles each; count 1 = a constant column).  The declaration is checked against the
 * resident rows bit for bit; *ok = 1 when it holds, 0 when it does not (nothing
 * changes then).  On a verified tensor grid the sweeps of GPs whose kernels are
 * products of RBF parts -- k(X_j, x) is then a product of one factor per axis -- read
 * per-axis factor tables instead of evaluating the covariance (same results within
 * rounding; sgp_ctx_set_sweep(... + 8) switches it off).  Replaces nothing in the
 * reference: gp.predict_noiseless(self.inputs) (gp_opt.py:469) evaluates every
 * covariance of the grid in full.                                               */
int sgp_grid_set_axes(sgp_grid* grid, int d, const int64_t* count,
                      const int64_t* stride, const double* values, int* ok);
/* update_confidence_intervals + compute_safe_set (gp_opt.py:453-481), fused:
 * for every GP mean/var over all rows, Q[:,2i] = mean - beta*std,
 * Q[:,2i+1] = mean + beta*std, S = all(Q[:, ::2] > fmin).
 * out2 = { max(l0[S]) or -inf, any(S) }  (local rows); out2 == NULL: no read-
 * back and no stream sync, the value stays on the device for
 * sgp_grid_sets_fused.                                                        */
int sgp_grid_confidence(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, double* out2);
/* gp.predict_noiseless(self.inputs) for every GP (gp_opt.py:469, and the
 * re-predictions of the expander loop, :585-602): refreshes the resident
 * mean / var only -- Q, S, M, G are not touched.  Needed when the intervals
 * were assigned by hand (opt.Q = ...) or the data changed without an interval
 * update before compute_sets().                                              */
int sgp_grid_posterior(sgp_grid* grid, sgp_gp* const* gps, int G);
/* update_confidence_intervals after ONE sgp_gp_append on the GPs flagged in
 * which[]: closed-form rank-1 update of the resident mean/var,
 *   c(x) = k(x,x*) - k(X,x)^T Ky^-1 k(X,x*),  mean += c r / s2,
 *   var = max(var - c^2 / s2, 1e-15),
 * O(n) per row instead of the O(n^2) sweep, then Q and S for all GPs from the
 * resident mean/var with the given beta.  out2 as sgp_grid_confidence.        */
int sgp_grid_rank1_update(sgp_grid* grid, sgp_gp* const* gps, int G,
                          const int* which, double beta, const double* fmin,
                          double* out2);
/* ... and after ONE sgp_gp_remove on the GPs flagged in which[]: with x_i the row that
 * left and w, alpha_i, P_ii of its record,
 *   c(x) = k(x,x_i) - k(X_new,x)^T w,  mean -= c alpha_i,
 *   var = max(var + c^2 P_ii, 1e-15),
 * then Q and S for all GPs; out2, the deferred form, context columns and shared factors
 * as sgp_grid_rank1_update.  Each of the two refuses the other's record (and a GP whose
 * newest change left none).                                                     */
int sgp_grid_rank1_remove(sgp_grid* grid, sgp_gp* const* gps, int G,
                          const int* which, double beta, const double* fmin,
                          double* out2);
/* ... and after ONE sgp_gp_reweigh on the GPs flagged in which[]: with x_i the re-weighted
 * row and w, u0 = P_ii eta, u1 = tau P_ii^2 of its record,
 *   c(x) = k(x,x_i) - k(X,x)^T w  (= k(X,x)^T p / P_ii),  mean += c u0,
 *   var = max(var + c^2 u1, 1e-15)     (the sign of the change is that of delta),
 * then Q and S for all GPs; out2, the deferred form, context columns and shared factors
 * as sgp_grid_rank1_update.  Each of the three refuses the other two's records.          */
int sgp_grid_rank1_reweigh(sgp_grid* grid, sgp_gp* const* gps, int G,
                           const int* which, double beta, const double* fmin,
                           double* out2);
/* ... and after ONE sgp_gp_append_block on the GPs flagged in which[] (b_g from the GP's block
 * record, it may differ per GP): per row x, with X' the data after the block and
 *   t_j(x) = sum_{i <= n0+j} L^-1[n0+j][i] k(X'_i, x),   j = 0 .. b-1 in that order,
 *   mean += sum_j t_j gamma_j,   var = max(var - sum_j t_j^2, 1e-15),
 * n + b covariance evaluations per row and GP where b rank-1 updates take about b n; then Q
 * and S for all GPs; out2, the deferred form and context columns as sgp_grid_rank1_update.  A
 * GP that shares the factor of a flagged GP in front of it with the same b takes that GP's
 * t_j.  Fixed summation order, no atomics: a row's result depends on its coordinates and the
 * GPs alone.  A flagged GP without a valid block record is an error that names it; mean,
 * var, Q and S are then untouched.                                              */
int sgp_grid_rankb_update(sgp_grid* grid, sgp_gp* const* gps, int G, const int* which,
                          double beta, const double* fmin, double* out2);
/* replace Q by host values (N x 2G row-major) and recompute S (tests, and
 * users who edit opt.Q by hand).                                             */
int sgp_grid_upload_Q(sgp_grid* grid, const double* Q, const double* fmin,
                      double* out2);
/* gp_opt.py:511-513: M = S & (u0 >= max_l); out = max(u0[M]-l0[M]) or -inf   */
int sgp_grid_maximizers(sgp_grid* grid, double max_l, double* out);
/* gp_opt.py:527-540: candidate mask.  full_sets=0: s = S & ~M &
 * (max_i (u_i-l_i)/scaling_i > max_var) & any_i(u_i-l_i > thr_beta_i);
 * full_sets=1: s = S.  Also clears G.  counts = {#candidates, #unsafe}.      */
int sgp_grid_candidates(sgp_grid* grid, double max_var, const double* scaling,
                        const double* thr_beta, int full_sets, int64_t* counts);
/* gp_opt.py:542-552: next <=k candidates in visiting order after the cut
 * (cut_w, cut_idx), i.e. descending w = max_i(u_i - l_i), ties: higher global
 * index first.  mode 1 (full_sets): ascending global index after cut_idx.
 * Start with cut_w = +inf, cut_idx = INT64_MAX (mode 1: cut_idx = -1).       */
int sgp_grid_topk(sgp_grid* grid, int mode, double cut_w, int64_t cut_idx,
                  int k, double* w_out, int64_t* gidx_out, int* n_out);
/* rows of the resident arrays for m GLOBAL indices owned by this rank:
 * x (m,d), mean (m,G), var (m,G), Q (m,2G)                                   */
int sgp_grid_gather_rows(sgp_grid* grid, const int64_t* gidx, int m, double* x,
                         double* mean, double* var, double* Q);
/* expander test of gp_opt.py:579-606 for m<=SGP_TOPK candidates at once, as a
 * rank-1 posterior update instead of two re-factorisations: for every GP i
 * with finite fmin_i, flags[c*G+i] = any over UNSAFE local rows x of
 *   mu2 - beta*sqrt(var2) >= fmin_i,
 *   mu2 = mu_i(x) + c(x) (u_i(x_c) - mu_i(x_c)) / s2,
 *   var2 = max(var_i(x) - c(x)^2 / s2, 1e-15),
 *   c(x) = k(x,x_c) - k(X,x)^T Ky^-1 k(X,x_c),  s2 = var_i(x_c)+noise+1e-8.
 * xc (m,d), mu_c/u_c (m,G) come from sgp_grid_gather_rows on the owner.
 * near_frac > 0 restricts the scan to rows with k(x,x_c) >= near_frac*k(x,x)
 * (a cheap first probe: a hit there already proves the candidate an expander;
 * no hit proves nothing, repeat with near_frac = 0 for the exact answer).     */
int sgp_grid_expander_check(sgp_grid* grid, sgp_gp* const* gps, int G,
                            double beta, const double* fmin, int m,
                            const double* xc, const double* mu_c,
                            const double* u_c, double near_frac,
                            int32_t* flags);
/* Lipschitz variant, gp_opt.py:558-576: flags[c*G+i] = any over unsafe rows
 * of u_i(x_c) - L_i * ||x_c - x||_2 >= fmin_i                                */
int sgp_grid_lipschitz_check(sgp_grid* grid, int G, const double* fmin,
                             const double* lipschitz, int m, const double* xc,
                             const double* u_c, int32_t* flags);
/* N-rank variant of sgp_grid_sets_front after sgp_grid_confidence(out2 = NULL):
 * max(l0[S]) and the maximiser width are all-reduced in stream (RCCL on the
 * context's stream, device-resident operands), so the front half of
 * compute_sets costs one device round trip per rank instead of three.
 * out5[0] = GLOBAL max(u0[M]-l0[M]); *max_l_out = GLOBAL max(l0[S]) (-inf: no
 * safe point on any rank); the other outputs (out5 has SIX entries, as for
 * sgp_grid_sets_front) describe this rank's shard.                            */
int sgp_grid_sets_front_comm(sgp_grid* grid, const double* scaling,
                             const double* thr_beta, double* out5, double* x_top,
                             double* mean_top, double* q_top, double* max_l_out);
/* Fused passes (one stream sync each; results identical to the step-by-step
 * calls above):
 * front = gp_opt.py:511-552: M and max_var (have_max_var = 0; with
 *   have_max_var = 1 the caller already ran sgp_grid_maximizers and passes the
 *   all-reduced max_var), candidate mask, counts, this shard's first
 *   candidate in visiting order and its rows.
 *   out5 (SIX entries) = {max(u0[M]-l0[M]) (0 if given), #candidates, #unsafe,
 *           w_top, idx_top or -1, #candidates of this shard whose width equals
 *           w_top bit for bit (exact ties decide the reference's visiting
 *           order, gp_opt.py:542-552)}
 * back = expander test of ONE candidate on this shard's unsafe rows
 *   (gp_opt.py:579-606), G mark if mark != 0 and every active GP certified it
 *   (gp_opt.py:615; single rank only), then the M|G arg-max (:642-644).       */
int sgp_grid_sets_front(sgp_grid* grid, double max_l, int have_max_var,
                        double max_var, const double* scaling,
                        const double* thr_beta, double* out5, double* x_top,
                        double* mean_top, double* q_top);
int sgp_grid_sets_back(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                       const double* fmin, const double* xc, const double* mu_c,
                       const double* u_c, double near_frac, int64_t gidx_c,
                       int mark, const double* scaling, int32_t* flags,
                       double* value, int64_t* gidx);
/* Both halves in one call and ONE stream sync (single GPU): the first candidate
 * stays on the device, the probe scan (near_frac) runs on it, G is marked if
 * every active GP certifies it, and the M|G arg-max follows.  Outputs as in
 * sgp_grid_sets_front + sgp_grid_sets_back, plus out5[5] (SIX entries here) =
 * number of candidates whose width equals the first one's bit for bit (> 1: the
 * reference's argsort()[::-1] decides among them, gp_opt.py:542-552; the host
 * settles it); flags are void when out5 reports no candidate or no unsafe row
 * (G is then left untouched).  max_l = NaN: use
 * the value a preceding sgp_grid_confidence / _rank1_update call with
 * out2 == NULL left on the device, and report it in *max_l_out (-inf = no safe
 * point) -- a whole SafeOpt.optimize() is then one device round trip.        */
int sgp_grid_sets_fused(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, double max_l, const double* scaling,
                        const double* thr_beta, double near_frac, double* out5,
                        double* x_top, double* mean_top, double* q_top,
                        int32_t* flags, double* value, int64_t* gidx,
                        double* max_l_out);
/* One pass of the expander loop (safeopt/gp_opt.py:557-612) over the next k <= 16
 * candidates behind the cut (cut_w, cut_idx) in visiting order -- sgp_grid_topk,
 * sgp_grid_gather_rows and the exact sgp_grid_expander_check of those rows -- with one
 * stream synchronisation instead of three host round trips: w_out / gidx_out / n_out as
 * sgp_grid_topk, flags[c * G + i] != 0: candidate c lifts an unsafe row above fmin_i.
 * One rank (the shard is the grid).                                                 */
int sgp_grid_expander_batch(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, int mode, double cut_w, int64_t cut_idx,
                            int k, double* w_out, int64_t* gidx_out, int* n_out,
                            int32_t* flags);

/* A pass of the expander loop over MANY candidates (safeopt/gp_opt.py:557-612 where the
 * loop goes far: no expander among the first candidates -- or none at all, the state of a
 * converged run -- and full_sets = True, :553-555, which visits every safe row): the next
 * ~want candidates behind the cut in visiting order (key descending -- the interval width,
 * or minus the row index with mode = 1 -- then index descending; strictly behind: key <
 * cut_w, or key == cut_w and row < cut_idx) are chosen by a histogram of the keys over
 * [key_lo, key_hi] (no sort) and ALL of them tested in ONE scan of the unsafe rows: the
 * rank-1 test of sgp_grid_expander_check per (row, candidate).  Two stream synchronisations
 * per pass whatever its size.
 *   out6 = { candidates tested, expanders among them,
 *            mode 0: key and global row of the FIRST expander in visiting order (nothing is
 *                    marked in G: the caller settles exact ties, gp_opt.py:542-552),
 *            key below which the candidates are still untested (-inf: none left; finite
 *            with 0 tested: the histogram counted keys an ulp below the edge of the picked bin,
 *            which the list does not take -- go on with cut_w = key_hi = this key),
 *            scaling != NULL and mode 0: the global row of sgp_grid_argmax(SGP_ARGMAX_MG_WIDTH)
 *            taken behind the test (gp_opt.py:631-641) -- the next query point when the pass
 *            ends the loop without an expander, for no further round trip; else -1 }
 *   mode 1 (full_sets): every expander of the pass is marked in G on the device.
 * No GP with a constraint (every fmin_i = -inf): nothing is an expander (gp_opt.py:559, 580:
 * the loop over the GPs only continues) -- 0 hits, nothing marked.
 * One rank (the shard is the grid).                                                  */
int sgp_grid_expander_pass(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                           const double* fmin, int mode, double cut_w, int64_t cut_idx,
                           double key_lo, double key_hi, int want, const double* scaling,
                           double* out6);
/* The same pass with Lipschitz certificates (safeopt/gp_opt.py:558-576 in place of :577-606):
 * candidate c is an expander when for every GP i with a constraint some unsafe row x has
 * u_i(x_c) - L_i |x_c - x|_2 >= fmin_i -- the comparison of sgp_grid_lipschitz_check per
 * (row, candidate), the pairs pruned by bounding boxes of 16 rows / 16 candidates.
 * Selection, modes and out6 as sgp_grid_expander_pass.  One rank.                       */
int sgp_grid_lipschitz_pass(sgp_grid* grid, int G, const double* fmin,
                            const double* lipschitz, int mode, double cut_w,
                            int64_t cut_idx, double key_lo, double key_hi, int want,
                            const double* scaling, double* out6);

/* The same pass on N ranks (safeopt/gp_opt.py:557-612 on a row-sharded grid), in three calls
 * with the ranks' agreement in between: (1) this shard's 4096-bin histogram of the keys of its
 * candidates behind the cut, over [key_lo, key_hi] -- the ranks sum the histograms and pick
 * ONE threshold thr; (2) this shard's candidates behind the cut with key >= thr (at most cap):
 * global rows, keys, the rows themselves [count][d] and u_i - mu_i [count][G] -- the ranks
 * gather them into one list; (3) the rank-1 test of ALL K listed candidates against this
 * shard's unsafe rows: flags[c * G + i] != 0 when candidate c lifts one of them above fmin_i
 * -- the ranks OR the flags; the first expander in visiting order is the hit with the
 * largest (key, row).  mode as in sgp_grid_expander_pass.                               */
int sgp_grid_pass_hist(sgp_grid* grid, int mode, double cut_w, int64_t cut_idx, double key_lo,
                       double key_hi, uint32_t* hist4096);
int sgp_grid_pass_list(sgp_grid* grid, int mode, double cut_w, int64_t cut_idx, double thr,
                       int cap, int* count, int64_t* gidx, double* key, double* x, double* resid);
int sgp_grid_pass_test(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                       const double* fmin, int K, const double* xc, const double* resid,
                       int32_t* flags);
/* The test of (3) with Lipschitz certificates (safeopt/gp_opt.py:558-576): xc [K][d] and the
 * candidates' upper bounds uc [K][G] -- sgp_grid_pass_list with mode | 2 returns u_i in place of
 * u_i - mu_i -- against this shard's unsafe rows; flags as above (one value per candidate, set
 * for every GP: the comparison is monotone in the distance).                            */
int sgp_grid_pass_lipschitz_test(sgp_grid* grid, int G, const double* fmin,
                                 const double* lipschitz, int K, const double* xc,
                                 const double* uc, int32_t* flags);

/* SMALL grids -- the reference's own regime (safeopt/gp_opt.py:651-675 on the 1000-point
 * grid of examples/1d_example.ipynb with n <= 20 observations; BASELINE.json config 1):
 * one whole SafeOpt.optimize() = update_confidence_intervals (gp_opt.py:453-476) +
 * compute_sets (:483-615) + the arg-max of get_new_query_point (:635-649) in ONE launch
 * of one workgroup and one read-back, for grids of at most 16384 rows and GPs with at most
 * 48 observations.  The expander test of the first candidate is the exact scan over all
 * unsafe rows.  Outputs as sgp_grid_sets_fused; Q / S / M / G / mean / var / candidate
 * mask and widths stay resident as the large-grid path leaves them.
 * sgp_grid_step_small_ok: 1 when the grid and the GPs qualify.                        */
int sgp_grid_step_small(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, const double* scaling,
                        const double* thr_beta, double* out5, double* x_top,
                        double* mean_top, double* q_top, int32_t* flags, double* value,
                        int64_t* gidx, double* max_l_out);
int sgp_grid_step_small_ok(sgp_grid* grid, sgp_gp* const* gps, int G);
/* A FLEET of such problems in one call: sgp_grid_step_small for B grids of ONE context side
 * by side, one workgroup per member, one launch per kernel instance present (input
 * dimension, observation class 24 / 32 / 48, single-part kernels or not).  Member b computes
 * the bits sgp_grid_step_small(grids[b], ...) computes and leaves the same arrays resident.
 * Per member, packed at fixed strides: gps [B][SGP_MAX_GPS] handles (entries behind G[b]
 * ignored, NULL by convention), G [B], beta [B], fmin / scaling / thr_beta [B][SGP_MAX_GPS]
 * (the first G[b] read); out5 [B][6], x_top [B][SGP_MAX_D], mean_top [B][SGP_MAX_GPS],
 * q_top [B][2 SGP_MAX_GPS], flags [B][SGP_MAX_GPS], value [B], gidx [B], max_l_out [B] --
 * each row as the one-problem call fills its output of that name.
 * Refused with an error that names the first offending member, before anything is launched
 * or written: B < 1; a NULL grid; a member sgp_grid_step_small_ok refuses; members of
 * different contexts; one grid twice; one GP under two members.                          */
int sgp_grid_step_small_many(sgp_grid* const* grids, sgp_gp* const* gps, const int* G, int B,
                             const double* beta, const double* fmin, const double* scaling,
                             const double* thr_beta, double* out5, double* x_top,
                             double* mean_top, double* q_top, int32_t* flags, double* value,
                             int64_t* gidx, double* max_l_out);
/* ... and when its first candidate is no expander: the expander test of gp_opt.py:579-606
 * for EVERY candidate of the list (global row indices, any order) in two launches and one
 * round trip; flags[c * G + i] != 0: candidate c lifts an unsafe row above fmin_i.  The
 * caller walks the flags in the reference's visiting order (gp_opt.py:542-557).         */
int sgp_grid_expanders_small(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const int64_t* gidx, int m,
                             int32_t* flags);
/* The same for EVERY candidate of the grid (the mask of sgp_grid_candidates / the one-launch
 * step), listed on the device in row order: global rows, widths (max_i (u_i - l_i), the key of
 * the visiting order, safeopt/gp_opt.py:542-552) and flags of the first *count candidates in
 * one read-back -- the caller sorts and walks them.  *count > cap: only *count is valid.  */
int sgp_grid_expanders_small_all(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                                 const double* fmin, int cap, int* count, int64_t* gidx,
                                 double* width, int32_t* flags);

/* The same on N ranks (row shards, sgp_comm_init on the grid's context) after a
 * confidence pass without read-back: max l0[S] and the maximiser width are
 * all-reduced in stream; every rank's first candidate (with its row, counts and
 * tie count) goes through ONE in-stream all-gather and is merged on the device
 * into the first candidate of the WHOLE grid in the visiting order of
 * gp_opt.py:542-552; every rank scans its own unsafe rows for it, the G flags are
 * all-reduced (max) in stream (gp_opt.py:611-612: any over all rows), the owner
 * of the candidate marks G if every active GP certified it, and the (value,
 * index) pairs of the local M|G arg-maxima are all-gathered and merged
 * (gp_opt.py:635, 642-644: first index among equals).  One stream sync; every
 * rank returns the same numbers: counts are totals over the grid, indices are
 * global.  Without a communicator (one rank) it equals sgp_grid_sets_fused with
 * max_l = NaN.                                                                  */
int sgp_grid_sets_fused_comm(sgp_grid* grid, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const double* scaling,
                             const double* thr_beta, double near_frac, double* out5,
                             double* x_top, double* mean_top, double* q_top,
                             int32_t* flags, double* value, int64_t* gidx,
                             double* max_l_out);
/* gp_opt.py:615: G[idx] = True for owned global indices                      */
int sgp_grid_mark_expanders(sgp_grid* grid, const int64_t* gidx, int m);
/* ... and G[gidx] = False: when exact ties in the visiting order
 * (gp_opt.py:542-552, argsort()[::-1]) make another candidate of the same
 * width the first expander.                                                    */
int sgp_grid_unmark_expanders(sgp_grid* grid, const int64_t* gidx, int m);
/* get_new_query_point / get_maximum arg-max (gp_opt.py:635, 642-644,
 * 708-710), first (lowest) global index wins among equal values.
 * value = -inf and gidx = -1 when the masked set is empty.                   */
int sgp_grid_argmax(sgp_grid* grid, int mode, const double* scaling,
                    double* value, int64_t* gidx);
/* The paths of sgp_gp_paths_eval over the grid's RESIDENT rows (nothing is uploaded per
 * row), the same bits.  values (N x S row-major) may be NULL.  best_val[S] / best_idx[S]
 * (both or neither): per path the maximum and its GLOBAL row (global_offset + local row),
 * over all rows (mask = 0) or over the rows of the safe set S (mask = 1); the lowest row
 * wins a tie; -inf / -1 when no row qualifies.  The arg-max is an epilogue of the
 * evaluation (per-workgroup partial pairs, one small final kernel): with values == NULL
 * no N x S array exists anywhere.  A Thompson pick inside the safe set.                  */
int sgp_grid_paths(sgp_grid* grid, sgp_gp* gp, const double* Omega, const double* phase, int m,
                   const double* W, const double* V, int S, int mask, double* values,
                   double* best_val, int64_t* best_idx);
/* sgp_grid_paths on a grid whose context has a communicator (sgp_comm_init or
 * sgp_comm_init_host): the N-rank Thompson pick.  Every rank evaluates the paths over its
 * resident rows; its S records (best value, GLOBAL row) are all-gathered -- in stream on
 * RCCL, through the host transport otherwise -- and one small kernel merges the world x S
 * records per path: the largest value, the lowest global row among equals; a shard without
 * a qualifying row (-inf / -1) never wins against one with a row, and no qualifying row on
 * any shard gives -inf / -1.  Every rank returns the same best_val[S] / best_idx[S], after
 * ONE read-back of the merged result.  values (the rank's N_local x S block) stays optional
 * and rank-local.  Every rank must pass the same paths and make the call (a collective).
 * Without a communicator (one rank) it equals sgp_grid_paths.                             */
int sgp_grid_paths_comm(sgp_grid* grid, sgp_gp* gp, const double* Omega, const double* phase,
                        int m, const double* W, const double* V, int S, int mask,
                        double* values, double* best_val, int64_t* best_idx);
/* Max-value entropy search (Wang & Jegelka 2017).  With K maxima ystar[K] of the objective
 * (the per-path maxima of sgp_grid_paths over the safe set) and a floor m,
 *   sigma = sqrt(max(var, 1e-15)),  y_k = max(ystar[k], m),  gamma_k = (y_k - mean) / sigma,
 *   alpha = (1 / K) sum_k term(gamma_k),  term(g) = g phi(g) / (2 Phi(g)) - ln Phi(g),
 * the terms added in the order of k.  term is evaluated through one scaled complementary
 * error function (csrc/mes.hip: mes_term): finite over the whole range, 0 exactly from
 * gamma = 38.6 on, +inf included.  A row's alpha depends on (mean, var, ystar, m) alone: the
 * same bits from sgp_mes_eval and from sgp_grid_mes, whatever N, the row's position or the
 * rank.  1 <= K <= SGP_MAX_MES and every ystar[k] finite, or the call fails with nothing
 * launched.
 *
 * sgp_mes_eval: alpha at N arbitrary points from HOST arrays mean[N], var[N] -> out[N];
 * floor may be +-inf (-inf: no floor), not NaN.  N <= 0 returns 0 and writes nothing.       */
enum { SGP_MES_ALL = 0, SGP_MES_S = 1, SGP_MES_MG = 2 };          /* candidate rows            */
enum { SGP_MES_FLOOR_NONE = 0, SGP_MES_FLOOR_MEAN = 1, SGP_MES_FLOOR_VALUE = 2 };
int sgp_mes_eval(sgp_ctx* ctx, const double* mean, const double* var, int64_t N,
                 const double* ystar, int K, double floor, double* out);
/* alpha over the grid's RESIDENT posterior of GP 0 -- a pass that sweeps it
 * (sgp_grid_confidence, sgp_grid_posterior, sgp_grid_step_small) must have run on the rows as
 * they are (sgp_grid_set_context voids it), else the call fails; the call takes no GPs, so
 * that the pass saw their current data is the caller's business (SafeOpt tracks it) -- and
 * its arg-max over the candidate
 * rows: every row (rows = SGP_MES_ALL), the rows of S (SGP_MES_S) or of M | G as they stand on
 * the device (SGP_MES_MG); value and gidx = GLOBAL row (global_offset + local row), the lowest
 * row among equal values, -inf / -1 when no row qualifies.  alpha (N_local) may be NULL.
 * The floor: none (SGP_MES_FLOOR_NONE), floor_value (SGP_MES_FLOOR_VALUE, +-inf allowed), or
 * the maximum of the mean of GP 0 over the rows of S -- over all rows with SGP_MES_ALL, over S
 * with SGP_MES_MG too -- (SGP_MES_FLOOR_MEAN; -inf when S is empty): reduced on the device
 * and read from device memory by the row pass, no host round trip in between.  floor_used
 * returns the floor applied.  One read-back of {value, gidx, floor}, one more of alpha when
 * asked for.  Q, S, M, G, mean and var are only read.                                        */
int sgp_grid_mes(sgp_grid* grid, const double* ystar, int K, int rows, int floor_mode,
                 double floor_value, double* alpha, double* value, int64_t* gidx,
                 double* floor_used);
/* sgp_grid_mes over the shards of all ranks of the context's communicator (sgp_comm_init or
 * sgp_comm_init_host): the floor of SGP_MES_FLOOR_MEAN is all-reduced (max), the ranks' records
 * {value, GLOBAL row} are all-gathered and merged on the device -- the largest value, the
 * lowest global row among equals, a shard without a candidate never wins -- all in the grid's
 * stream (through the host transport otherwise), then ONE read-back.  Every rank returns the
 * same value, gidx and floor_used; alpha stays the rank's N_local rows.  A collective: every
 * rank calls it with the same ystar.  Without a communicator it equals sgp_grid_mes.         */
int sgp_grid_mes_comm(sgp_grid* grid, const double* ystar, int K, int rows, int floor_mode,
                      double floor_value, double* alpha, double* value, int64_t* gidx,
                      double* floor_used);

/* Expected improvement and probability of improvement as logarithms (LogEI: Ament, Daulton,
 * Eriksson, Balandat, Bakshy 2023), optionally weighed by the probability that the constraints
 * hold (EIC: Gelbart et al. 2014, Gardner et al. 2014).  With the objective GP 0, an incumbent
 * tau, a margin xi >= 0 and sigma_g = sqrt(max(var_g, 1e-15)), per row
 *   z = (mean_0 - tau - xi) / sigma_0,
 *   SGP_EI_EI:  alpha = ln(max(var_0, 1e-15)) / 2 + ln(phi(z) + z Phi(z))   (= ln EI),
 *   SGP_EI_PI:  alpha = ln Phi(z)                                           (= ln PI),
 *   alpha += ln Phi((mean_g - fmin_g) / sigma_g) for every g with a finite fmin_g, in the
 *   order of g (fmin NULL or fmin_g = -inf: GP g is not weighed; NaN and +inf are refused).
 * Both logarithms through the scaled complementary error function (csrc/ei_term.h): finite
 * and ordered where EI itself underflows to 0.  A row's alpha depends on its own (mean_g,
 * var_g) and on (fmin, tau, xi, kind) alone: the same bits from sgp_ei_eval and from
 * sgp_grid_ei, whatever N, the row's position or the rank.
 *
 * sgp_ei_eval: alpha at N arbitrary points from HOST arrays mean[G][N], var[G][N] -> out[N].
 * 1 <= G <= SGP_MAX_GPS, a known kind, tau finite, xi finite and >= 0, or the call fails with
 * nothing launched and nothing written.  N <= 0 returns 0 and writes nothing.              */
enum { SGP_EI_EI = 0, SGP_EI_PI = 1 };                            /* kind                      */
enum { SGP_EI_TAU_MEAN = 1, SGP_EI_TAU_VALUE = 2 };               /* the incumbent             */
int sgp_ei_eval(sgp_ctx* ctx, const double* mean, const double* var, int64_t N, int G,
                const double* fmin, int kind, double tau, double xi, double* out);
/* alpha over the grid's RESIDENT posterior [G][N] (the rule of sgp_grid_mes: a pass that sweeps
 * it must have run on the rows as they are, else the call fails) and its arg-max over the
 * candidate rows in the same pass: every row (rows = SGP_MES_ALL), the rows of S (SGP_MES_S) or
 * of M | G as they stand on the device (SGP_MES_MG); value and gidx = GLOBAL row, the lowest
 * row among equal values, -inf / -1 when no row qualifies.  Rows outside the mask skip the
 * evaluation unless alpha (N_local, may be NULL) is asked for.  The incumbent: tau_value, finite
 * (SGP_EI_TAU_VALUE), or the maximum of the mean of GP 0 over the rows of S -- over all rows
 * with SGP_MES_ALL, over S with SGP_MES_MG too -- (SGP_EI_TAU_MEAN): reduced on the device and
 * read from device memory by the row pass, no host round trip in between.  With an empty S
 * there is no incumbent and no pick: alpha is all -inf, tau_used = -inf.  fmin: G values, or
 * NULL.  tau_used returns the incumbent applied.  One read-back of {value, gidx, tau}, one more
 * of alpha when asked for.  Q, S, M, G, mean and var are only read.                         */
int sgp_grid_ei(sgp_grid* grid, int kind, int rows, int tau_mode, double tau_value, double xi,
                const double* fmin, double* alpha, double* value, int64_t* gidx,
                double* tau_used);
/* sgp_grid_ei over the shards of all ranks of the context's communicator (sgp_comm_init or
 * sgp_comm_init_host): the incumbent of SGP_EI_TAU_MEAN is all-reduced (max), the ranks' records
 * {value, GLOBAL row} are all-gathered and merged on the device -- the largest value, the
 * lowest global row among equals, a shard without a candidate never wins -- all in the grid's
 * stream (through the host transport otherwise), then ONE read-back.  Every rank returns the
 * same value, gidx and tau_used; alpha stays the rank's N_local rows.  A collective: every
 * rank calls it with the same arguments.  Without a communicator it equals sgp_grid_ei.     */
int sgp_grid_ei_comm(sgp_grid* grid, int kind, int rows, int tau_mode, double tau_value,
                     double xi, const double* fmin, double* alpha, double* value,
                     int64_t* gidx, double* tau_used);

/* Information-theoretic safe exploration (Bottero, Luis, Vinogradska, Berkenkamp, Peters 2022):
 * the approximate mutual information, in nats, between a noisy measurement at x and the safety
 * indicator [f(z) >= fmin] of a row z.  With mu = mean(z) - fmin, vz = max(var(z), 1e-15),
 * vx = max(var(x), 1e-15), c = cov(z, x), s the variance of the measurement's noise and
 * c1 = 1 / (pi ln 2):
 *   t = c1 mu^2 / vz,  r2 = min(c^2 / (vx vz), 1),  q = r2 vx,  B = (s + vx) + (2 c1 - 1) q,
 *   e = q / B,  w = min(2 c1 e, 1),
 *   I = -ln2 exp(-t) expm1(log1p(-w) / 2 - t (1 - 2 c1) e)
 * (csrc/ise_term.h: ise_term) -- the stable form of ln2 [e^-t - sqrt(A / B) e^(-t (s + vx) / B)],
 * A = s + vx (1 - r2): >= 0, 0 exactly at c = 0, <= ln2 e^-t, finite for every finite input.  A
 * term depends on (mu, vz, vx, c, s) alone: the same bits from sgp_ise_eval and from
 * sgp_grid_ise, whatever N, the row's position or the launch.
 *
 * sgp_ise_eval: the term at N arbitrary points from HOST arrays mu[N], vz[N], vx[N], c[N] ->
 * out[N].  N <= 0 returns 0 and writes nothing; a NaN or negative s is refused with nothing
 * launched.                                                                                  */
enum { SGP_ISE_UNSAFE = 0, SGP_ISE_ALL = 1 };                     /* the rows z                */
int sgp_ise_eval(sgp_ctx* ctx, const double* mu, const double* vz, const double* vx,
                 const double* c, int64_t N, double s, double* out);
/* The K candidates cand[K] (GLOBAL rows of this rank's shard; duplicates allowed) against the
 * rows z of the grid -- the rows outside S as it stands on the device (about = SGP_ISE_UNSAFE)
 * or every row (SGP_ISE_ALL) -- over the grid's RESIDENT posterior (the rule of sgp_grid_mes: a
 * pass that sweeps it must have run since the rows last changed).  A GP g is active when
 * fmin[g] is finite; with s_g = noise_var_g + 1e-8 and c_g the posterior covariance
 *   c_g(z, x) = k_g(z, x) - k_g(X, z)^T Ky^-1 k_g(X, x),
 *   pair(x, z) = sum over the active g, in the order of g, of I_g(x; z),
 *   alpha[j]   = max_z pair(cand[j], z)        (-inf when no row qualifies),
 *   target[j]  = the lowest GLOBAL row z attaining it                  (-1),
 *   value, gidx = the largest alpha and its candidate's global row, the lowest such row among
 *                 equal values (-inf / -1 when no row qualifies).
 * The operands Ky^-1 k_g(X, x_j) are formed once per call; the row kernel contracts them with
 * k_g(z, X), evaluated once per tile of rows, on the fp64 matrix cores (csrc/ise.hip).  No
 * atomics; partials bounded by 512 x K pairs.  A candidate's alpha, target and row of pairs
 * depend on the candidate alone, not on K or on its position in cand.  pairs (K x N_local) and
 * cov (G x K x N_local, zeros for an inactive GP) may be NULL: test and diagnostic outputs,
 * refused when G K N_local > 2^24.
 * Refused, with nothing launched or written: K < 1 or K > SGP_MAX_ISE; an unknown `about`; a
 * candidate outside the shard; no active GP; a grid without a current posterior; a GP that is
 * not fitted, lives in another context or has another input dimension.  One rank: the call
 * never communicates.  Q, S, M, G, mean and var are only read.                               */
int sgp_grid_ise(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin,
                 const int64_t* cand, int K, int about, double* alpha, int64_t* target,
                 double* value, int64_t* gidx, double* pairs, double* cov);
/* sgp_grid_ise with the candidates BY VALUE: cand[K] are GLOBAL rows anywhere in the whole grid
 * (>= 0; read by the pick's tie rule and returned as gidx, nothing else), xc[K][d] their
 * coordinates and vx[G][K] their variances, host arrays -- on a row-sharded grid a candidate
 * usually lies in another rank's shard.  The same operand kernels, row kernel and reductions as
 * sgp_grid_ise over this shard's rows: with the resident coordinates and variances of rows of
 * this shard it returns the bits of sgp_grid_ise.  alpha, target, value, gidx as there (the
 * shard's: -inf / -1 where none of ITS rows qualifies as z).  Refusals as sgp_grid_ise, with a
 * negative row or a missing xc / vx in place of a candidate outside the shard.  Never
 * communicates.                                                                              */
int sgp_grid_ise_at(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin,
                    const int64_t* cand, const double* xc, const double* vx, int K, int about,
                    double* alpha, int64_t* target, double* value, int64_t* gidx);
/* sgp_grid_ise_at over the shards of all ranks of the context's communicator (sgp_comm_init or
 * sgp_comm_init_host), in the grid's stream: ONE all-gather of the ranks' alpha | target blocks,
 * a merge per candidate -- the largest alpha, the lowest global target among equals, a rank
 * without a target (-inf / -1) never wins --, the pick over the merged values, then ONE
 * read-back.  Every rank returns the same alpha, target, value and gidx: what sgp_grid_ise
 * returns on one rank that holds the whole grid, bit for bit (a pair depends on the candidate
 * and the row alone).  A collective: every rank calls it with the same candidates.  Without a
 * communicator it equals sgp_grid_ise_at.                                                    */
int sgp_grid_ise_comm(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin,
                      const int64_t* cand, const double* xc, const double* vx, int K, int about,
                      double* alpha, int64_t* target, double* value, int64_t* gidx);
/* Choosing the candidates of sgp_grid_ise where the variances are.  The key of a row of S is
 *   key = sum over the active g, in the order of g, of log1p(var_g / s_g) / 2,
 * s_g = noise_var_g + 1e-8, over the RESIDENT var and S (only read).  The device's log1p is not
 * the host's to the last bit: a caller that must reproduce a host ordering lists a superset and
 * orders it itself (SafeOpt._ise_select).  Three HBM-bound passes, the pattern of
 * sgp_grid_pass_hist / sgp_grid_pass_list; each refuses as sgp_grid_ise does (G of the grid, no
 * active GP, no current posterior, a GP that is not fitted or lives in another context) with
 * nothing launched or written.
 *   sgp_grid_ise_keys: *count = the rows of S in this shard, *key_min / *key_max their
 *     smallest and largest key (+inf / -inf when there is none).
 *   sgp_grid_ise_hist: hist[4096] = how many of the shard's safe rows fall into each of 4096
 *     equal bins over [key_lo, key_hi], bin = int((key - key_lo) * (4096 / (key_hi - key_lo)))
 *     clamped to 0 .. 4095 (sgp_grid_pass_hist's rule); integer counts, key_hi > key_lo.
 *   sgp_grid_ise_list: the shard's safe rows with key >= thr in ASCENDING global row, compacted
 *     by prefix sums (deterministic): gidx[m], key[m] (the device's), x[m][d] and var[m][G] (the
 *     bits of the resident arrays).  *count = the rows that qualify, even above cap; only the
 *     first min(*count, cap) are written.                                                    */
int sgp_grid_ise_keys(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin,
                      int64_t* count, double* key_min, double* key_max);
int sgp_grid_ise_hist(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin,
                      double key_lo, double key_hi, uint32_t* hist);
int sgp_grid_ise_list(sgp_grid* grid, sgp_gp* const* gps, int G, const double* fmin, double thr,
                      int cap, int64_t* count, int64_t* gidx, double* key, double* x,
                      double* var);
/* One pick of a batch by hallucinated observations (GP-BUCB, Desautels et al. 2014, on
 * SafeOpt's rule, safeopt/gp_opt.py:635-649; the reference has no batch mode).  gps are CLONES
 * (sgp_gp_clone) of the grid's GPs, every one with the pending pick x* appended
 * (sgp_gp_append; any y: only the variance is read) -- checked as sgp_grid_rank1_update
 * checks its records.  In one pass over the rows, per GP i,
 *   var_h_i(x) = max(v_i(x) - c_i(x)^2 / s2_i, 1e-15),   c, s2 as in sgp_grid_rank1_update,
 * v = the resident var (first != 0: the first downdate of a batch; var_h is never read before
 * it is written) or var_h as the pick before left it, and the intervals
 * l = mean - beta sqrt(var_h), u = mean + beta sqrt(var_h) from the RESIDENT mean.  Then the
 * arg-max of
 *   mode SGP_ARGMAX_MG_WIDTH: max_i (u_i - l_i) / scaling_i over the rows of M | G,
 *   mode SGP_ARGMAX_UCB:      u_0 over the rows of S,
 * over the rows that are not among picked[n_picked] (GLOBAL rows, n_picked <= SGP_MAX_BATCH);
 * the lowest global row wins among equal values; value = -inf, gidx = -1 when no row is
 * eligible (var_h is downdated all the same).  Q, S, M, G, mean and var are only read.  One
 * launch of the row kernel, a small final kernel, one read-back.  The pick of the SHARD the
 * grid holds: the call never communicates, whatever communicator the context has (the pick
 * over all ranks: sgp_grid_batch_next_comm).  var_h (G,N) is a buffer of the grid, allocated
 * by the first call: sgp_grid_download(SGP_VAR_H).                                        */
int sgp_grid_batch_next(sgp_grid* grid, sgp_gp* const* gps, int G, int first, int mode,
                        double beta, const double* scaling, const int64_t* picked,
                        int n_picked, double* value, int64_t* gidx);
/* sgp_grid_batch_next on a grid whose context has a communicator (sgp_comm_init or
 * sgp_comm_init_host): one pick of a batch over the shards of all ranks.  Every rank runs the
 * row kernel and the final kernel of sgp_grid_batch_next over its resident rows; its record
 * {value, GLOBAL row, stop} is all-gathered -- ONE collective per pick, in stream on RCCL,
 * through the host transport otherwise -- and one one-wave kernel merges the world records:
 * the largest value, the lowest global row among equal values; a shard without an eligible
 * row (-inf / -1) never wins against one with a row, and no eligible row on any shard gives
 * -inf / -1.  *stop_any = the maximum of the ranks' stop words.  Every rank returns the same
 * (value, gidx, stop_any) after ONE read-back of the merged record.
 * stop != 0: this rank takes no part in the pick (the bordered append of its clones met a
 * non-positive pivot) but still makes the call -- a collective, every rank must arrive: no
 * row kernel runs, var_h stays as it was, the clones' append records are not looked at, and
 * the rank contributes {-inf, -1, 1}.  The ranks end the batch together on stop_any.
 * picked[] are global rows, the same on every rank.  Everything else -- modes, first, the
 * refusals (no append record, another mode, n_picked > SGP_MAX_BATCH, first = 0 before a
 * downdate) -- as sgp_grid_batch_next; without a communicator (one rank) it equals
 * sgp_grid_batch_next, with *stop_any = stop.                                            */
int sgp_grid_batch_next_comm(sgp_grid* grid, sgp_gp* const* gps, int G, int first, int mode,
                             double beta, const double* scaling, const int64_t* picked,
                             int n_picked, int stop, double* value, int64_t* gidx,
                             int* stop_any);
/* copy a resident array to the host: Q (N,2G) f64 | S/M/G (N) u8 |
 * mean/var/var_h (G,N) f64 (var_h: after a sgp_grid_batch_next[_comm])       */
/* S / M / G of the shard from the host: the reference's arrays are mutated in place
 * (safeopt/gp_opt.py:481, 505-506, 511, 615) and user code may write into them; the next
 * arg-max (get_new_query_point, gp_opt.py:635-649) reads what was uploaded.            */
int sgp_grid_upload_mask(sgp_grid* grid, int what, const uint8_t* mask);
int sgp_grid_download(sgp_grid* grid, int what, void* out);

/* ---- SafeOptSwarm._compute_particle_fitness (gp_opt.py:901-1013) -----------
 * particles (P,d) row-major; values (P) f64; safe (P) u8.                    */
int sgp_swarm_fitness(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                      const double* particles, int64_t P, double beta,
                      const double* fmin, const double* scaling,
                      double best_lower_bound, double* values, uint8_t* safe);

/* The fitness of a THOMPSON swarm: a swarm that climbs one posterior sample path f of GP 0
 * (one column of sgp_gp_path_weights: Omega (m x d), phase (m), w (m), v (n)) inside the
 * safe region.  With mu_g, var_g the posterior of GP g at x and lower_g = mu_g - beta
 * sqrt(var_g), for every GP with a finite fmin[g]:
 *   slack = lower_g - fmin[g];  safe &= slack >= 0;  total_pen += penalty(slack / scaling[g])
 * (the penalty and safety rule of SGP_SWARM_MAXIMIZERS), and
 *   values = f(x) / scaling[0] + total_pen.
 * The posterior is formed by the kernels sgp_swarm_fitness takes for that P and n; the path
 * term f(x) = sum_i amp w_i cos(omega_i . x + b_i) + sum_j k(x, X_j) v_j is one more launch:
 * a row kernel on the fp64 VALU, 16 lanes per particle, no Phi or k(x, X) in memory.  Sums in
 * a fixed order, no atomics: a particle's value depends on its coordinates and the path
 * alone -- not on P, its row or the launch -- and the same inputs give the same bits.
 * Limits and failures of sgp_gp_paths_eval (1 <= m <= SGP_MAX_FEATURES, GP 0 fitted);
 * P <= 0 returns 0 and writes nothing.  particles (P,d) row-major; values (P) f64; safe
 * (P) u8.                                                                      */
int sgp_swarm_fitness_path(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                           int64_t P, double beta, const double* fmin, const double* scaling,
                           const double* Omega, const double* phase, int m, const double* w,
                           const double* v, double* values, uint8_t* safe);

/* The fitness of a HALLUCINATED swarm (GP-BUCB on SafeOptSwarm's rule):
 * clones[g] is a private copy of gps[g] (sgp_gp_clone) with the b pending picks of a batch
 * appended (sgp_gp_append; any y: only the variance is read), 1 <= b <= SGP_MAX_BATCH, the
 * same b for every GP.  With t_j(x) = (row n_g + j of the clone's L^-1) . k(X', x),
 *   down_g(x) = sum_j t_j(x)^2  (j = 0 .. b-1, in that order),
 *   var_h_g(x) = max(var_g(x) - down_g(x), 1e-15),
 * the width term is values = max_g sqrt(var_h_g) / scaling[g]; the lower and upper bounds,
 * both interests, the slack, the penalty and `safe` are those of sgp_swarm_fitness, bit for
 * bit, from the real mean and variance: hallucinated widths rank points, safety is never
 * judged on them.  The result is (values + total_pen) * interest.  swarm_type is
 * SGP_SWARM_MAXIMIZERS or SGP_SWARM_EXPANDERS.  The real posterior is formed by the kernels
 * sgp_swarm_fitness takes for that P and n; down is one more launch in front of the shaping
 * pass: a row kernel on the fp64 VALU that evaluates k(X', x) on the fly, sums in a fixed
 * order, no atomics -- down of a particle depends on its coordinates and the clones alone,
 * not on P, its row or the launch.  var_h (G,P) receives the hallucinated variances, or NULL.
 * Refused: another swarm type, a clone whose n is not gps[g].n + b for one common b in
 * 1 .. SGP_MAX_BATCH, a clone or GP in another context, a clone with another input
 * dimension or kernel than its GP.  P <= 0 returns 0 and writes nothing.        */
int sgp_swarm_fitness_hall(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                           int swarm_type, const double* particles, int64_t P, double beta,
                           const double* fmin, const double* scaling, double best_lower_bound,
                           double* values, uint8_t* safe, double* var_h);

/* The fitness of a MES swarm: max-value entropy search (Wang & Jegelka 2017; the rule of
 * sgp_grid_mes) without a grid.  ystar[K] are K maxima of the objective (GP 0) over the safe
 * region, floor a value no maximum can lie below (-inf: none; +-inf allowed, NaN refused).
 * With mu_g, var_g the posterior of GP g at x and lower_g = mu_g - beta sqrt(var_g), for every
 * GP with a finite fmin[g]:
 *   slack = lower_g - fmin[g];  safe &= slack >= 0;  total_pen += penalty(slack / scaling[g])
 * (the penalty and safety rule of SGP_SWARM_MAXIMIZERS), and with
 *   sigma = sqrt(max(var_0, 1e-15)),  y_k = max(ystar[k], floor),  gamma_k = (y_k - mu_0) / sigma,
 *   alpha = (1 / K) sum_k term(gamma_k)   (the terms added in the order of k; sgp_mes_eval),
 *   values = alpha + total_pen;
 * alpha has the bits of sgp_mes_eval on post; a particle's value depends on its posterior and
 * (ystar, floor) alone -- not on P, its row or the launch -- and the same inputs give the same
 * bits.  The posterior is formed by the kernels sgp_swarm_fitness takes for that P and n; alpha
 * is one more launch behind the shaping pass: one thread per particle on the fp64 VALU, the K
 * floored maxima staged in LDS once per workgroup, no atomics.  The maxima are staged on the
 * device once per call.  post (2,P) receives the posterior of GP 0 the term was formed from
 * (row 0 the mean, row 1 the variance), or NULL.  scaling[0] does not scale alpha (it is a
 * number of nats, not a function value).
 * Checked in this order: G >= 1 and gps[0]; 1 <= K <= SGP_MAX_MES and every ystar[k] finite;
 * floor not NaN -- a refused call writes nothing; P <= 0 then returns 0 and writes nothing;
 * then the checks of sgp_swarm_fitness (GP 0 .. G-1 fitted, in ctx, one input dimension).
 * particles (P,d) row-major; values (P) f64; safe (P) u8.                             */
int sgp_swarm_fitness_mes(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                          int64_t P, double beta, const double* fmin, const double* scaling,
                          const double* ystar, int K, double floor, double* values,
                          uint8_t* safe, double* post);

/* ---- SafeOptSwarm safe-set growth (gp_opt.py:1089-1111) ---------------------
 * After a maximizer / expander swarm run the reference appends, in order, every
 * best position B_j (n,d row-major) whose prior correlation
 * gp.kern.K(B_j, p) / scaling[0]^2 is <= thr (0.95) with every point p of the
 * safe set S (m,d row-major) and with every B_i accepted before it.
 * scale2 = scaling[0]^2; accept (n) u8 = 1 for the rows to append.            */
int sgp_swarm_grow(sgp_ctx* ctx, sgp_gp* gp0, const double* S, int64_t m,
                   const double* B, int64_t n, double scale2, double thr,
                   uint8_t* accept);

/* ---- SwarmOptimization on the device (swarm.py:61-146) -----------------------
 * init_swarm (init != 0: velocities = rand * velocity_scale, personal bests :=
 * positions / their fitness, global best := arg-max, unmasked as in the
 * reference) followed by `iters` iterations of run_swarm (inertia0, += step per
 * iteration; velocity clip 10 * velocity_scale; positions clipped to bounds
 * (d,2) when given), the fitness being the fused posterior kernel of
 * sgp_swarm_fitness.  State arrays are row-major (P,d) / (P) / (d), in and out
 * (with init only `positions` is read).
 * rand != NULL: the uniform numbers in the order the reference draws them --
 * P*d for init, then 2*P*d per iteration (np.random.rand(2*P, d): r1 rows, r2
 * rows) -- the run is then bit-identical to the host implementation.
 * rand == NULL: counter-based device generator (Philox4x32-10) keyed by seed. */
int sgp_swarm_run(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                  double beta, const double* fmin, const double* scaling,
                  double best_lower_bound, int64_t P, double* positions,
                  double* velocities, double* best_positions, double* best_values,
                  double* global_best, const double* velocity_scale,
                  const double* bounds, int init, int iters, double inertia0,
                  double step, const double* rand, uint64_t seed);

/* sgp_swarm_run for a Thompson swarm: the fitness is that of sgp_swarm_fitness_path, the
 * state arrays, init / iters / inertia, rand and seed as for sgp_swarm_run.  One call is the
 * whole run: the path is staged on the device once per call, nothing but the state arrays
 * crosses PCIe.  A path run ALWAYS takes the general launches -- move, fitness (posterior,
 * shaping, path term), personal bests, global best -- also for a swarm the one-workgroup
 * step of sgp_swarm_run would take (a 20-particle Thompson swarm simply uses them): with
 * rand != NULL the run is bit-identical to the host loop over sgp_swarm_fitness_path.
 * The whole swarm in one call (a rank's block: sgp_swarm_run_path_shard).  P <= 0 returns
 * 0 and writes nothing.                                                        */
int sgp_swarm_run_path(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                       const double* fmin, const double* scaling, int64_t P, double* positions,
                       double* velocities, double* best_positions, double* best_values,
                       double* global_best, const double* velocity_scale,
                       const double* bounds, int init, int iters, double inertia0,
                       double step, const double* rand, uint64_t seed,
                       const double* Omega, const double* phase, int m, const double* w,
                       const double* v);

/* sgp_swarm_run for a hallucinated swarm: the fitness is that of sgp_swarm_fitness_hall,
 * everything else as for sgp_swarm_run.  Like a path run it ALWAYS takes the general
 * launches -- move, fitness (downdate, posterior, shaping), personal bests, global best --
 * never the one-workgroup step of a small swarm: with rand != NULL the run is bit-identical
 * to the host loop over sgp_swarm_fitness_hall.  The whole swarm in one call (a rank's
 * block: sgp_swarm_run_hall_shard).  The refusals of sgp_swarm_fitness_hall; P <= 0 returns 0
 * and writes nothing.                                                           */
int sgp_swarm_run_hall(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                       int swarm_type, double beta, const double* fmin, const double* scaling,
                       double best_lower_bound, int64_t P, double* positions,
                       double* velocities, double* best_positions, double* best_values,
                       double* global_best, const double* velocity_scale,
                       const double* bounds, int init, int iters, double inertia0,
                       double step, const double* rand, uint64_t seed);

/* sgp_swarm_run on a rank's contiguous block of particles [p0, p0 + P) of a swarm
 * of P_total (shard_range): the state arrays hold the block's P rows.  After the
 * personal bests of init and of every iteration each rank's best (value, global
 * index, x) is all-gathered over the context's communicator (in stream on RCCL,
 * or the host transport of sgp_comm_init_host) and the global best is the largest
 * value, the lowest global index on ties -- on every rank, as for the whole swarm.
 * Philox mode draws the numbers of the block's global elements (p0*d + e; r2:
 * P_total*d + p0*d + e), so a block draws what the whole run draws for it; with
 * rand != NULL the caller passes the block's rows of every draw (P*d for init,
 * then per iteration its P r1 rows and its P r2 rows).  The posterior kernel and
 * the few-points / small-swarm choices follow P_total.  p0 = 0, P = P_total is
 * sgp_swarm_run; P < P_total needs a communicator on ctx.                     */
int sgp_swarm_run_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, int swarm_type,
                        double beta, const double* fmin, const double* scaling,
                        double best_lower_bound, int64_t P, double* positions,
                        double* velocities, double* best_positions, double* best_values,
                        double* global_best, const double* velocity_scale,
                        const double* bounds, int init, int iters, double inertia0,
                        double step, const double* rand, uint64_t seed, int64_t p0,
                        int64_t P_total);

/* sgp_swarm_run_path on a rank's block [p0, p0 + P) of a Thompson swarm of P_total: the
 * block, the merge of the global best after init and after every iteration, the Philox
 * indexing and the layout of rand are those of sgp_swarm_run_shard; the path is staged once
 * per call on every rank (every rank passes the same path).  p0 = 0, P = P_total is
 * sgp_swarm_run_path; P < P_total needs a communicator on ctx, and P >= 1 on every rank. */
int sgp_swarm_run_path_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const double* scaling, int64_t P,
                             double* positions, double* velocities, double* best_positions,
                             double* best_values, double* global_best,
                             const double* velocity_scale, const double* bounds, int init,
                             int iters, double inertia0, double step, const double* rand,
                             uint64_t seed, const double* Omega, const double* phase, int m,
                             const double* w, const double* v, int64_t p0, int64_t P_total);

/* sgp_swarm_run_hall on a rank's block [p0, p0 + P) of a hallucinated swarm of P_total: the
 * block, the merge of the global best after init and after every iteration, the Philox
 * indexing and the layout of rand are those of sgp_swarm_run_shard; the posterior kernel
 * follows P_total; every rank passes clones with the same pending picks.  The downdate is
 * per particle (sgp_swarm_fitness_hall), so a block computes the bits the whole swarm
 * computes for its particles.  The refusals of sgp_swarm_run_hall.  p0 = 0, P = P_total is
 * sgp_swarm_run_hall; P < P_total needs a communicator on ctx, and P >= 1 on every rank.  */
int sgp_swarm_run_hall_shard(sgp_ctx* ctx, sgp_gp* const* gps, sgp_gp* const* clones, int G,
                             int swarm_type, double beta, const double* fmin,
                             const double* scaling, double best_lower_bound, int64_t P,
                             double* positions, double* velocities, double* best_positions,
                             double* best_values, double* global_best,
                             const double* velocity_scale, const double* bounds, int init,
                             int iters, double inertia0, double step, const double* rand,
                             uint64_t seed, int64_t p0, int64_t P_total);

/* sgp_swarm_run for a MES swarm: the fitness is that of sgp_swarm_fitness_mes (post = NULL),
 * the state arrays, init / iters / inertia, rand and seed as for sgp_swarm_run, ystar / K /
 * floor in place of the path of sgp_swarm_run_path.  One call is the whole run: the maxima are
 * staged on the device once per call.  Like a path run it ALWAYS takes the general launches --
 * move, fitness (posterior, shaping, alpha), personal bests, global best -- never the
 * one-workgroup step of a small swarm: with rand != NULL the run is bit-identical to the host
 * loop over sgp_swarm_fitness_mes.  The whole swarm in one call (a rank's block:
 * sgp_swarm_run_mes_shard).  The refusals of sgp_swarm_fitness_mes, in its order; P <= 0
 * returns 0 and writes nothing.                                                   */
int sgp_swarm_run_mes(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                      const double* fmin, const double* scaling, int64_t P, double* positions,
                      double* velocities, double* best_positions, double* best_values,
                      double* global_best, const double* velocity_scale,
                      const double* bounds, int init, int iters, double inertia0,
                      double step, const double* rand, uint64_t seed,
                      const double* ystar, int K, double floor);

/* sgp_swarm_run_mes on a rank's block [p0, p0 + P) of a MES swarm of P_total: the block, the
 * merge of the global best after init and after every iteration, the Philox indexing and the
 * layout of rand are those of sgp_swarm_run_shard; the posterior kernel follows P_total; every
 * rank passes the same ystar and floor.  alpha is per particle, so a block computes the bits
 * the whole swarm computes for its particles.  P <= 0 and P_total <= 0 returns 0; an empty
 * block of a sharded swarm is refused ("bad swarm size"), as is a block without a
 * communicator on ctx.  p0 = 0, P = P_total is sgp_swarm_run_mes.                    */
int sgp_swarm_run_mes_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, const double* scaling, int64_t P,
                            double* positions, double* velocities, double* best_positions,
                            double* best_values, double* global_best,
                            const double* velocity_scale, const double* bounds, int init,
                            int iters, double inertia0, double step, const double* rand,
                            uint64_t seed, const double* ystar, int K, double floor,
                            int64_t p0, int64_t P_total);

/* The fitness of an ISE swarm: information-theoretic safe exploration (Bottero et al. 2022; the
 * rule of sgp_grid_ise) without a grid.  The particles x_p are the points a measurement may be
 * taken at, targets (T,d) a fixed set of points z_t whose safety the measurement should tell
 * about, zmean / zvar (G,T) their posterior (noiseless).  GP g is active when fmin[g] is
 * finite; s_g = noise_var_g + 1e-8.  With var_g(x_p) the posterior variance at the particle,
 *   c_g(x_p, z_t) = k_g(x_p, z_t) - k_g(x_p, X) Ky^-1 k_g(X, z_t)
 *   pair(p, t)    = sum over the active g, in the order of g, of
 *                   I(zmean[g][t] - fmin[g], zvar[g][t], var_g(x_p), c_g(x_p, z_t); s_g)
 *                   (I: the term of sgp_ise_eval)
 *   alpha[p]      = max_t pair(p, t),   target[p] = the lowest t attaining it
 *   values[p]     = alpha[p] + total_pen[p]
 * with the penalty and the safety flag of SGP_SWARM_MAXIMIZERS (sgp_swarm_fitness_mes).
 * scaling does not scale alpha (a number of nats).  A particle's alpha, target, value and row
 * of pairs depend on its coordinates, the GPs and the target set alone -- not on P, its row or
 * the launch; a pair's covariance on the particle and the target alone -- not on T or the
 * target's position.  The posterior is formed by the kernels sgp_swarm_fitness takes for that P
 * and n; alpha is one more launch behind the shaping pass (k_swarm_ise: 2 P T n flop per active
 * GP on the fp64 matrix cores, no atomics); targets and operands are staged once per call.
 * alpha (P), target (P), post (G,2,P: mean | var per GP), pairs (P,T) and cov (G,P,T; zeros for
 * an inactive GP) may be NULL; pairs and cov are test outputs, refused above G P T = 2^24.
 * Checked in this order, a refused call launches and writes nothing: G >= 1 and gps[0];
 * 1 <= T <= SGP_MAX_ISE; targets, zmean and zvar present and finite, every zvar >= 0; one GP
 * active; P <= 0 then returns 0; the size of the test outputs; then the checks of
 * sgp_swarm_fitness.                                                                */
int sgp_swarm_fitness_ise(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                          int64_t P, double beta, const double* fmin, const double* scaling,
                          const double* targets, const double* zmean, const double* zvar, int T,
                          double* values, uint8_t* safe, double* alpha, int64_t* target,
                          double* post, double* pairs, double* cov);

/* sgp_swarm_run for an ISE swarm: the fitness is that of sgp_swarm_fitness_ise (no outputs),
 * everything else as for sgp_swarm_run_mes, targets / zmean / zvar / T in place of ystar / K /
 * floor.  Targets and operands are staged once per call; the run ALWAYS takes the general
 * launches: with rand != NULL it is bit-identical to the host loop over sgp_swarm_fitness_ise.
 * The refusals of sgp_swarm_fitness_ise, in its order; P <= 0 returns 0 and writes nothing. */
int sgp_swarm_run_ise(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                      const double* fmin, const double* scaling, int64_t P, double* positions,
                      double* velocities, double* best_positions, double* best_values,
                      double* global_best, const double* velocity_scale,
                      const double* bounds, int init, int iters, double inertia0,
                      double step, const double* rand, uint64_t seed,
                      const double* targets, const double* zmean, const double* zvar, int T);

/* sgp_swarm_run_ise on a rank's block [p0, p0 + P) of an ISE swarm of P_total: everything as
 * sgp_swarm_run_mes_shard; every rank passes the same targets, zmean and zvar.  P <= 0 and
 * P_total <= 0 returns 0; an empty block of a sharded swarm is refused ("bad swarm size"), as
 * is a block without a communicator on ctx.  p0 = 0, P = P_total is sgp_swarm_run_ise.  */
int sgp_swarm_run_ise_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, const double* scaling, int64_t P,
                            double* positions, double* velocities, double* best_positions,
                            double* best_values, double* global_best,
                            const double* velocity_scale, const double* bounds, int init,
                            int iters, double inertia0, double step, const double* rand,
                            uint64_t seed, const double* targets, const double* zmean,
                            const double* zvar, int T, int64_t p0, int64_t P_total);

/* The fitness of an EI swarm: log expected improvement / log probability of improvement (the
 * rule of sgp_grid_ei) without a grid.  With mu_g, var_g the posterior of GP g at x (GP 0 the
 * objective), sigma_g = sqrt(max(var_g, 1e-15)), the incumbent tau and the margin xi >= 0,
 *   z = (mu_0 - tau - xi) / sigma_0
 *   SGP_EI_EI:  alpha = ln(max(var_0, 1e-15)) / 2 + ln(phi(z) + z Phi(z)),
 *   SGP_EI_PI:  alpha = ln Phi(z),
 *   weigh = 1:  alpha += ln Phi((mu_g - fmin[g]) / sigma_g) for every g with a finite fmin[g],
 *               in the order of g (weigh = 0: no weights);
 *   free = 0:   values = alpha + total_pen, safe as for SGP_SWARM_MAXIMIZERS
 *               (sgp_swarm_fitness_mes; fmin drives penalty and flag whatever weigh is);
 *   free = 1:   values = alpha, safe = 1 -- penalty and safety rule switched off: with weigh
 *               the EIC baseline over the bounds, NOT a safe pick.
 * scaling does not scale alpha (a logarithm, not a function value).  A particle's alpha, value
 * and flag depend on its coordinates, the GPs and (kind, tau, xi, fmin, weigh, free) alone --
 * not on P, its row, the launch, the block or the rank -- and alpha has the bits of sgp_ei_eval
 * on the posterior `post` the call returns.  The posterior is formed by the kernels
 * sgp_swarm_fitness takes for that P and n (a block of a sharded run: P_total and n; a call of
 * up to 4096 particles on GPs of 128 observations or more takes the few-points posterior, whose
 * last bits may differ from the sweep's); alpha is one more launch behind the shaping pass
 * (k_swarm_ei: one thread per particle on the fp64 VALU, no LDS, no atomics; its constants
 * travel by value, nothing is staged).  alpha (P) and post (G,2,P: mean | var per GP) may be
 * NULL.
 * Checked in this order, a refused call launches and writes nothing: G >= 1 and gps[0]; a
 * known kind; tau finite; xi finite and >= 0; weigh, then free, 0 or 1; with weigh no fmin[g]
 * NaN or +inf; P <= 0 then returns 0; then the checks of sgp_swarm_fitness.            */
int sgp_swarm_fitness_ei(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* particles,
                         int64_t P, double beta, const double* fmin, const double* scaling,
                         int kind, double tau, double xi, int weigh, int free_mode,
                         double* values, uint8_t* safe, double* alpha, double* post);

/* sgp_swarm_run for an EI swarm: the fitness is that of sgp_swarm_fitness_ei (no outputs),
 * everything else as for sgp_swarm_run_mes, kind / tau / xi / weigh / free in place of ystar /
 * K / floor.  The run ALWAYS takes the general launches -- move, fitness (posterior, shaping,
 * alpha), personal bests, global best: with rand != NULL it is bit-identical to the host loop
 * over sgp_swarm_fitness_ei.  The refusals of sgp_swarm_fitness_ei, in its order; P <= 0
 * returns 0 and writes nothing.                                                      */
int sgp_swarm_run_ei(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta, const double* fmin,
                     const double* scaling, int64_t P, double* positions, double* velocities,
                     double* best_positions, double* best_values, double* global_best,
                     const double* velocity_scale, const double* bounds, int init, int iters,
                     double inertia0, double step, const double* rand, uint64_t seed,
                     int kind, double tau, double xi, int weigh, int free_mode);

/* sgp_swarm_run_ei on a rank's block [p0, p0 + P) of an EI swarm of P_total: everything as
 * sgp_swarm_run_mes_shard; every rank passes the same kind, tau, xi, weigh and free.  alpha is
 * per particle, so a block computes the bits the whole swarm computes for its particles.
 * P <= 0 and P_total <= 0 returns 0; an empty block of a sharded swarm is refused ("bad swarm
 * size"), as is a block without a communicator on ctx.  p0 = 0, P = P_total is
 * sgp_swarm_run_ei.                                                                  */
int sgp_swarm_run_ei_shard(sgp_ctx* ctx, sgp_gp* const* gps, int G, double beta,
                           const double* fmin, const double* scaling, int64_t P,
                           double* positions, double* velocities, double* best_positions,
                           double* best_values, double* global_best,
                           const double* velocity_scale, const double* bounds, int init,
                           int iters, double inertia0, double step, const double* rand,
                           uint64_t seed, int kind, double tau, double xi, int weigh,
                           int free_mode, int64_t p0, int64_t P_total);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -------------------------
 * The only cross-rank traffic of the path is a handful of scalars per
 * iteration (max / any / arg-max / top-k merge).                             */
int sgp_comm_unique_id(void* id128);              /* rank 0: ncclGetUniqueId  */
int sgp_comm_init(sgp_ctx* ctx, const void* id128, int rank, int world);
int sgp_comm_count(sgp_ctx* ctx, int* n);           /* ncclCommCount: ranks that
                                                     * really joined (1 without a
                                                     * communicator)              */
/* The same role for a caller that brings its own transport (TCP, MPI, shared memory;
 * ranks that share a GPU or have no xGMI between them): three collectives on HOST
 * buffers -- in-place all-reduce(max) of n f64 / n i32, all-gather of nbytes per rank
 * into rank order -- returning 0 on success.  The N-rank entry points
 * (sgp_grid_sets_front_comm, sgp_grid_sets_fused_comm) then stage their device operands
 * through the host around these calls (stream sync, D2H, callback, H2D) at exactly the
 * points where they enqueue RCCL collectives otherwise; sgp_comm_allreduce_max /
 * _allgather / _barrier call them directly.  A context has one transport.           */
typedef int (*sgp_host_allreduce_max_f64)(void* user, double* buf, int n);
typedef int (*sgp_host_allreduce_max_i32)(void* user, int32_t* buf, int n);
typedef int (*sgp_host_allgather)(void* user, const void* send, void* recv, int64_t nbytes);
int sgp_comm_init_host(sgp_ctx* ctx, int rank, int world,
                       sgp_host_allreduce_max_f64 allreduce_f64,
                       sgp_host_allreduce_max_i32 allreduce_i32,
                       sgp_host_allgather allgather, void* user);
int sgp_comm_allreduce_max(sgp_ctx* ctx, double* buf, int n);   /* in place   */
int sgp_comm_allgather(sgp_ctx* ctx, const void* send, void* recv,
                       int64_t nbytes);           /* recv = world*nbytes      */
int sgp_comm_barrier(sgp_ctx* ctx);

/* ---- measurement -----------------------------------------------------------*/
/* hipEvent pair on the ctx stream around a region of calls                   */
int sgp_timer_start(sgp_ctx* ctx);
int sgp_timer_stop(sgp_ctx* ctx, float* ms);
/* per-launch hipEvent timing of the posterior sweep kernel (the dominant
 * kernel): enable, run, then read {total ms, launches, algorithmic flops}    */
int sgp_profile_enable(sgp_ctx* ctx, int on);
int sgp_profile_read(sgp_ctx* ctx, double* total_ms, int64_t* launches,
                     double* flops);
/* ... and the time of the LAST timed launch alone (0 when none ran): the term of a 'mes'
 * swarm is the last timed launch of a sgp_swarm_fitness_mes call, behind the sweep's     */
int sgp_profile_read_last(sgp_ctx* ctx, double* ms);
/* device allocations (hipMalloc) this context has made so far: buffers grow on
 * demand, and a growth is an allocation plus a stream sync -- a steady-state
 * loop (same n, same grid) must leave this number unchanged                  */
int64_t sgp_ctx_alloc_count(sgp_ctx* ctx);

/* Which kernel runs gp.predict_noiseless over a grid / a swarm
 * (safeopt/gp_opt.py:469, 929, 973).  0 = automatic (the paired-wave kernel once
 * a GP has more than 256 training rows, csrc/sweep_pair.hip; the VALU kernel up to
 * 48, csrc/sweep_tiny.hip; the resident-factor kernel for 49 .. 128 observations of
 * single-part kernels up to d = 4, csrc/sweep_mid.hip; the 4-wave kernel otherwise),
 * 1 = always the 4-wave kernel (csrc/sweep.hip), 2 = always the paired-wave kernel,
 * 3 = automatic without the VALU kernel and the one-launch step; + 4: the
 * paired-wave kernel does not cut remainder tiles into runs of chunks (same bits
 * either way, tests/test_gpu_posterior.py); + 8: no factor tables on tensor grids
 * (sgp_grid_set_axes); + 16: the 4-wave kernel streams small factors through its
 * double buffer instead of keeping them in LDS for the launch (same bits either
 * way); + 32: the paired-wave kernel runs one 16-point block of training points per
 * stage instead of merging the thin stages of a triangular chunk (the schedule until
 * round 5: another summation order, same results within rounding); + 64: in the paired-wave kernel a GP with the
 * training inputs and kernel of the GP in front evaluates its own covariances instead
 * of receiving that GP's (same bits either way, tests/test_gpu_pair_hand.py).  Same results
 * within rounding between the two kernels; the switch exists for A/B measurements and tests.  Returns
 * the previous setting.                                                        */
int sgp_ctx_set_sweep(sgp_ctx* ctx, int which);
/* Which kernel ran the LAST posterior sweep of this context (tests of the selection,
 * A/B scripts): 0 = none yet, 1 = the 4-wave kernel (n <= 256, csrc/sweep.hip),
 * 2 = the paired-wave kernel (csrc/sweep_pair.hip), 3 = the VALU kernel for GPs with
 * at most 48 observations (csrc/sweep_tiny.hip -- the regime of the reference's own
 * examples), 4 = the few-points path (csrc/factor.hip), 5 = the one-launch step of a
 * small grid (csrc/step_small.hip), 6 = the resident-factor kernel for 49 .. 128
 * observations (csrc/sweep_mid.hip); + 256: the paired-wave kernel handed covariances
 * from a GP to GPs with the same inputs and kernel (see sgp_ctx_set_sweep, + 64).    */
int sgp_ctx_last_sweep(sgp_ctx* ctx);

/* Multi-output case: consecutive GPs of a launch with bit-identical training
 * inputs, kernel, noise and fitting history have the same L^-1, so the variance
 * contraction of gp.predict_noiseless (safeopt/gp_opt.py:466-476 loops over the
 * GPs independently) is computed once and only alpha . k per GP: up to two such
 * followers per leader take their alpha . k from the covariances the leader's
 * sweep evaluates anyway (both sweep kernels; single-part kernels, d <= 4 / 3),
 * further ones keep covariance-only stages in the paired-wave kernel.  Identical
 * results bit for bit (tests/test_gpu_posterior.py).  on = 1 (default) / 0; returns
 * the previous setting.                                                         */
int sgp_ctx_set_share(sgp_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* SAFEOPT_HIP_H */
