// Internal declarations shared by the translation units of libsafeopt_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "safeopt_hip.h"

// ---- error plumbing ---------------------------------------------------------
void sgp_set_error(sgp_ctx* ctx, const char* fmt, ...);

#define SGP_HIP(ctx, call)                                                     \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      sgp_set_error((ctx), "%s:%d %s -> %s", __FILE__, __LINE__, #call,        \
                    hipGetErrorString(e_));                                    \
      return -1;                                                               \
    }                                                                          \
  } while (0)

#define SGP_CHECK(ctx, cond, ...)                                              \
  do {                                                                         \
    if (!(cond)) {                                                             \
      sgp_set_error((ctx), __VA_ARGS__);                                       \
      return -2;                                                               \
    }                                                                          \
  } while (0)

#define SGP_TRY(expr)                                                          \
  do {                                                                         \
    int r_ = (expr);                                                           \
    if (r_ != 0) return r_;                                                    \
  } while (0)

// ---- device-side descriptors ------------------------------------------------
struct KernDesc {
  int d;
  int n_parts;
  int kind[SGP_MAX_PARTS];
  double variance[SGP_MAX_PARTS];
  double inv_ls[SGP_MAX_PARTS][SGP_MAX_D];
  double kdiag;  // product of the variances = k(x, x)
  // Single-part kernels: inputs are stored pre-multiplied by scale0 =
  // inv_ls[0] * kern_unit(kind[0]), in units where the exponent of the
  // covariance is a plain square / norm (see kern_eval.h, KernFast).
  double scale0[SGP_MAX_D];
  // Products of parts in the sweep (KernFast::manyn_t): squared weights
  // wsq[p][k] = (inv_ls[p][k] * kern_unit(kind[p]))^2 on the squared RAW coordinate
  // differences (zero for a column the part does not use, and for p >= n_parts);
  // the exponents of the parts then ADD: one 2^(U/32) per covariance.
  double wsq[SGP_MAX_PARTS][SGP_MAX_D];
};

// Input scaling of the fast covariance path: with z = x * inv_ls * kern_unit,
//   RBF      exp(-r^2/2)   = 2^(-|dz|^2 / 32)        kern_unit = sqrt(16 / ln 2)
//   Matern   exp(-sqrt(nu2) r) = 2^(-|dz| / 32)      kern_unit = sqrt(3|5) * 32 / ln 2
inline double kern_unit(int kind) {
  return kind == SGP_RBF ? 4.804489635145799
                         : (kind == SGP_MATERN32 ? 79.962275540715
                                                 : 103.23085383134594);
}

// One GP as the sweep kernels see it.  All pointers are device pointers.
struct GpDev {
  const double* Apack;  // L^-1 in MFMA A-operand order: [nblk][n_pad/4][64],
                        // zero above the diagonal and in the padding rows
  const double* Xpad;   // training inputs, [n_pad][d], zero padded
  const double* Xs;     // = Xpad * kern.scale0 for single-part kernels,
                        //   else = Xpad (KernFast::operator() convention)
  const double* alpha;  // Ky^-1 y, [n_pad], zero padded
  const double* XA;     // per j-block of 16 training points: [16 d of Xs | 16 of
                        // alpha], contiguous -- ONE LDS-DMA source per stage of
                        // the paired sweep (sweep_pair.hip)
  int n;                // training points
  int n_pad;            // n rounded up to 16
  int nblk;             // n_pad / 16
  int share;            // >= 0: this GP has the same training inputs, kernel and noise
                        // as the GP in front of it in the launch (the multi-output
                        // case): same L^-1, so the paired sweep takes |L^-1 k|^2
                        // from that GP and only forms alpha . k (collect_gps)
                        // <= -2: a COVARIANCE TWIN of GP -2 - share (gp_cov_lead): same
                        // training inputs and kernel, but its own noise, jitter or
                        // history, hence its own L^-1 -- k(X, x) is the leader's, which
                        // the paired sweep hands down instead of evaluating it again
                        // (sweep_pair.hip, "hand-down").  Every other reader tests
                        // share >= 0 only: a twin is a GP with a factor of its own.
                        // (Test the sign, never share == -1.  The mark lives in this
                        // field because a field of its own would move `kern` and change
                        // the stride of gps[g] in every kernel of the library)
  int narrow;           // 1: the last row block has <= 4 real rows and Apack holds
                        // them in the "narrow" form (k_pack): the sweep then needs
                        // one MFMA per k-step for that block instead of four
  int last_rows;        // real rows of the last row block (1..16): the 4-wave sweep
                        // takes a last block of <= 12 rows as 1..3 narrow 4-row groups
                        // (sweep.hip, narrow_groups)
  // record of the last one-row append (sgp_gp_append), consumed by the
  // rank-1 update of the resident posterior: w = Ky_old^-1 k(X_old, x*)
  // (zero padded to n_pad), upd[0] = (y* - mu(x*)) / s2, upd[1] = 1 / s2,
  // upd[2..2+d) = x*
  // ... or of the last removal (sgp_gp_remove), the same four things for the row x_i that
  // left, as an append of it to the reduced GP would write them: w = Ky_new^-1 k(X_new, x_i),
  // upd[0] = alpha_i, upd[1] = (Ky_old^-1)_ii, upd[2..2+d) = x_i
  const double* upd_w;
  const double* upd;
  // dense L^-1 (row pitch ld) and k(x,x) + noise + 1e-8 + jitter: what the
  // operands of the rank-1 expander test are built from (expander.hip, k_expw_mm)
  const double* Linv;
  int64_t ld;
  double prior;
  KernDesc kern;
};
// The record of the last block append (sgp_gp_append_block), consumed by the rank-b refresh of
// the resident posterior (block.hip), in a small device buffer of the GP's own (sgp_gp::blk), in
// doubles: [0] = b, [1] = n0 (the rows in front of the block), [2 .. 2 + b) = gamma_j = (row
// n0 + j of L^-1) . y, zero behind b.  The launch hands the kernel the buffers of its flagged
// GPs (RankbArgs): GpDev stays as every sweep kernel knows it.
constexpr int kBlkB = 0, kBlkN0 = 1, kBlkGamma = 2, kBlkWords = 2 + SGP_MAX_BLOCK;

// GP whose covariances k(X, x) are bit for bit those of `g` (GpDev::share <= -2), or -1
inline int gp_cov_lead(const GpDev& g) { return g.share <= -2 ? -2 - g.share : -1; }

// A candidate grid that is a TENSOR grid (linearly_spaced_combinations,
// safeopt/utilities.py:21-54: global row i has column k equal to
// axis_k[(i / stride_k) % count_k]), declared with sgp_grid_set_axes and verified on
// the device, together with per-axis factor tables of every GP whose kernel is a
// product of RBF parts: k(X_j, x) = prod_k E_k[idx_k(x)][j].  The sweep then reads d
// table entries per covariance instead of evaluating an exponential (sweep.hip, SEP).
struct SepLaunch {
  int naxes;                  // axes with more than one point (1..4), in order of their
                              // stride in the flat index; constant columns (contexts)
                              // are folded into the tables of axis 0
  uint32_t count[4];          // points of axis a
  int64_t goff;               // global index of the shard's first row
  // per GP and axis: [n_pad / 16][count][16] doubles, entry 4 k4 + q of a block of 16
  // = training point 16 jb + 4 q + k4 (the four values of a lane side by side)
  const double* tab[SGP_MAX_GPS][4];
};

// ---- device scratch (sgp_ctx::scratch) --------------------------------------
// One buffer per slot, grown on demand.  Asking for a slot may reallocate it (and under
// SGP_POISON=2 fills it with 0xFF), which voids every pointer into it that is still held.
// Hence the rule every call chain keeps: a slot is never asked for below (in a callee of)
// a caller that still holds a pointer into it.  The one exception are the KEPT slots: an
// entry point sizes and fills them, and a callee asks for them again with the same size
// to find the contents in place (SGP_POISON=2 leaves them alone).
enum ScratchSlot : int {
  // (the blocks of the expander test -- slots 0, 7 .. 12 and expander_batch's part of slot 1 --
  // are laid out in expander_layout.h)
  kSlotList = 0,        // the rows the pre-filter of ONE candidate lists (enqueue_expander)
  kSlotResult = 1,      // small result blocks the entry points read back: maximizers,
                        // candidates, topk, argmax, expander_batch (BatchReadLayout),
                        // sets_front[_comm], sets_fused[_comm]
  kSlotPartials = 2,    // per-workgroup partials of the sets.hip launchers (candidates, topk,
                        // argmax[_marked], the fused front, read by its fold); set_axes'
                        // mismatch count; fitness_small's mean | var; a batch pick's pairs
                        // and result (BatchScratch)
  kSlotStage = 3,       // host rows staged for a launch: gp_predict, kern_K, grid_create,
                        // swarm_fitness, swarm_run's random numbers (swarm_api.hip);
                        // factor.hip: append_gp; expander.hip: expander_operands_all
  kSlotWork = 4,        // gp_predict's points, kern_K's matrix; swarm_api.hip: the block of a
                        // fitness call (SwarmFitLayout), a run (SwarmRunLayout), swarm_grow
                        // (GrowLayout)
  kSlotGpDev = 5,       // gp_predict's GP descriptor
  kSlotSmall = 6,       // small_reserve (few-points path), upload_local_idx,
                        // comm_allreduce_max, comm_allgather
  kSlotOperands = 7,    // kept: operands of <= SGP_TOPK candidates (ExpanderLayout, expander_bufs:
                        // staged by expander_batch / sets_fused[_comm], asked for again by
                        // enqueue_expander); expanders_small[_all] (SmallLayout); gather_rows,
                        // lipschitz_check
  kSlotPass = 8,        // kept: the scratch of a big pass (PassLayout: list | histogram |
                        // PassSel | counts), the selection carried from pass_list on
  kSlotManyOps = 9,     // kept: operands of m listed candidates (ManyLayout, expander_many_test),
                        // the Lipschitz work block (LipLayout), pass_list's gathered rows
                        // (PassListLayout)
  kSlotManyW = 10,      // kept: their W operands (ManyLayout::w_bytes)
  kSlotManyFlags = 11,  // kept: their flags, the pass result in the tail behind them
                        // (FlagsLayout, FlagTail)
  kSlotHot = 12,        // launch_expander_many (HotLayout) / launch_lipschitz_many
                        // (LipHotLayout): the hot waves and rows
  kSlotJointA = 13,     // joint.hip: Sigma (N_pad x N_pad), the Cholesky factor in its lower part
  kSlotJointLi = 14,    // ... the inverse factor the recursion forms along the way
  kSlotJointT = 15,     // ... and its workspace
  kSlotJointZ = 16,     // ... Z | out of a draw (N x S each)
  kSlotJointVt = 17,    // ... V transposed, for the VALU yardstick of the SYRK only
  kSlotPathOm = 18,     // paths.hip: [omega | b] of the features
  kSlotPathB = 19,      // ... [amp W ; V], zero padded
  kSlotPathOut = 20,    // ... path values (rows x S); path_weights' U | E | T | V
  kSlotPathPart = 21,   // ... per-workgroup (value, row) partials of the arg-max, the result
  kSlotLooVec = 22,     // hyper.hip: the vectors of a leave-one-out call (LooVec)
  kSlotLooC = 23,       // ... C = diag(sqrt(b)) Ky^-1 of sgp_gp_loo_lml (n x n: like every slot
                        // it stays at its largest size until sgp_destroy, 2.1 GB after one
                        // call at kMaxObservations)
  kSlotMesIn = 24,      // mes.hip: ystar | floor of sgp_mes_eval, its rows' mean | var | out; ystar
                        // and the alpha array of a grid call; swarm_api.hip: ystar and post of a
                        // 'mes' swarm call (SwarmMesLayout) -- neither swarm_fitness nor
                        // swarm_run asks for this slot, so what the entry point staged stays put
  kSlotMesPart = 25,    // ... per-workgroup (value, row) pairs and floor partials of a grid call,
                        // its records and result (MesScratch)
  kSlotIseIn = 26,      // ise.hip (IseLayout): the candidates' rows | coordinates | variances of a
                        // grid call; mu | vz | vx | c | out of sgp_ise_eval's rows; the records
                        // of sgp_grid_ise_list
  kSlotIseW = 27,       // ... the operands W_g of the active GPs, the workspace T behind them
  kSlotIsePart = 28,    // ... per-workgroup (pair, row) partials, alpha | target | result, the
                        // ranks' gathered blocks and their merge; the partials, histogram and
                        // chunk counts of a selection call (IseSelLayout)
  kSlotIseOut = 29,     // ... pairs | cov, the test outputs of a grid call that asks for them
  kSlotSwarmIseW = 30,  // swarm_ise.hip (SwarmIseLayout): the operands W_g of an 'ise' swarm call, the
                        // workspace T behind them -- staged ONCE per call; neither swarm_fitness
                        // nor swarm_run asks for the three slots, so they stay put
  kSlotSwarmIseIn = 31, // ... targets[Tp][d] | zmean[G][Tp] | zvar[G][Tp] | bestv[P] | bestt[P]
  kSlotSwarmIseOut = 32,// ... alpha[P] | target[P] | post[G][2][P] | pairs[P][T] | cov[G][P][T] of a
                        // fitness call that asks for them
  kSlotEiIn = 33,       // ei.hip: mean[G] | var[G] | out of sgp_ei_eval's rows; the alpha array of a
                        // grid call; swarm_api.hip: alpha and post of an 'ei' swarm fitness call
                        // (SwarmEiLayout)
  kSlotEiPart = 34,     // ... per-workgroup (value, row) pairs and incumbent partials of a grid
                        // call, its records and result (EiScratch)
  kScratchSlots
};
inline bool scratch_kept(ScratchSlot s) { return s >= kSlotOperands && s <= kSlotManyFlags; }
// The head of kSlotMesIn, in doubles: ystar[SGP_MAX_MES] | floor, the rows' arrays behind it
constexpr size_t kMesHead = SGP_MAX_MES + 8;
// The block of a 'mes' swarm call in kSlotMesIn (sgp_swarm_fitness_mes, sgp_swarm_run_mes[_shard]):
//   ystar[SGP_MAX_MES] (the first K staged, ONCE per call) | 8 doubles unused |
//   post[2][P] f64 (mean | var of GP 0; a fitness call that asks for it)
struct SwarmMesLayout {
  size_t ystar, post, bytes;
};
constexpr SwarmMesLayout swarm_mes_layout(int64_t P, bool post) {
  SwarmMesLayout l{};
  l.ystar = 0;
  l.post = kMesHead * 8;
  l.bytes = l.post + (post && P > 0 ? 2 * size_t(P) * 8 : 0);
  return l;
}
static_assert(swarm_mes_layout(3, true).post >= SGP_MAX_MES * 8 &&
                  swarm_mes_layout(3, true).bytes == swarm_mes_layout(3, true).post + 48 &&
                  swarm_mes_layout(3, false).bytes == swarm_mes_layout(3, false).post,
              "SwarmMesLayout: post overlaps the maxima or ends outside the block");

// ---- host-side objects ------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct sgp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // small pinned staging area for scalar H2D / D2H traffic
  void* pinned = nullptr;
  size_t pinned_cap = 0;
  // device scratch (grown on demand)
  DevBuf scratch[kScratchSlots];
  int64_t n_allocs = 0;       // hipMalloc calls so far (sgp_ctx_alloc_count)
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool profiling = false;
  std::vector<hipEvent_t> prof_events;  // start/stop pairs of sweep launches
  size_t prof_used = 0;
  double prof_flops = 0.0;
  // stage table of the posterior sweep (sweep.hip: stage_table)
  DevBuf stage_tab;
  std::vector<uint64_t> stage_sig;
  int stage_count = 0;
  int stage_slots = 0;       // 2-KB positions of all stages of that table
  // ... and of the paired sweep (sweep_pair.hip: pair_stage_table)
  DevBuf pstage_tab;
  std::vector<uint64_t> pstage_sig;
  int pstage_count = 0;
  std::vector<int> pstage_chunk_start;   // first stage of every accumulator chunk, then
                                         // the stage count
  int pstage_chunk_off[SGP_MAX_GPS + 1] = {0};   // first chunk number of every GP
  DevBuf pair_split;                     // per-lane partial sums of split remainder tiles
  DevBuf pair_hand;                      // B-operand images a leader hands to its covariance
                                         // twins: [workgroup][j-block][pair][256]
  DevBuf pair_post;                      // [G][P] mean | var of a swarm (sweep_pair.hip)
  int sweep_partials = 0;     // partials of max l0[S] the last confidence sweep left
  int sweep_choice = 0;       // sgp_ctx_set_sweep: 0 auto, 1 4-wave, 2 paired, 3 auto (mid kernel asked for)
  int last_sweep = 0;         // kernel of the last posterior sweep (sgp_ctx_last_sweep; + 256: with the hand-down)
  int share_factors = 1;      // sgp_ctx_set_share: GPs with identical (X, kernel, noise)
                              // share the variance contraction (paired sweep)
  // sgp_grid_step_small: its result block lives in host memory the device writes directly
  // (pinned, mapped, coherent), the last word is a completion counter the host spins on
  double* step_host = nullptr;
  double* step_dev = nullptr;      // the same memory as the device sees it
  // ... and of the one-rank chain of the large-grid path (sgp_grid_sets_fused): result
  // block + the per-workgroup results of the last arg-max pass
  double* sets_host = nullptr;
  double* sets_dev = nullptr;
  size_t sets_cap = 0;             // doubles
  uint64_t step_seq = 0;
  // sgp_grid_step_small_many: one result block per member of the fleet, [B][kStepResWords]
  // in host memory of the same kind (an array of its own: step_host stays the block of the
  // one-problem call), the pinned staging buffer the records and GP descriptors of a call
  // are built in, and their place on the device -- all three grown on demand
  double* fleet_host = nullptr;
  double* fleet_dev = nullptr;
  size_t fleet_cap = 0;            // members
  void* fleet_stage = nullptr;
  size_t fleet_stage_cap = 0;      // bytes
  DevBuf fleet_recs;
  // RCCL
  void* comm = nullptr;  // ncclComm_t
  int rank = 0, world = 1;
  // ... or the caller's collectives on host buffers (sgp_comm_init_host): the library
  // stages the device operands of an N-rank step through the host around them
  struct HostComm {
    int (*allreduce_max_f64)(void*, double*, int) = nullptr;
    int (*allreduce_max_i32)(void*, int32_t*, int) = nullptr;
    int (*allgather)(void*, const void*, void*, int64_t) = nullptr;
    void* user = nullptr;
  } hostcomm;
  int num_cu = 256;
};

constexpr int64_t kMaxObservations = 16384;    // training points of a GP, at most
struct sgp_gp {
  sgp_ctx* ctx = nullptr;
  KernDesc kern;
  double noise_var = 0.0;
  double jitter = 0.0;
  int64_t n = 0;
  int n_pad = 0;  // multiple of 16 (sweep blocks)
  int n_f = 0;    // multiple of 32 (factorisation leaves)
  int ld = 0;     // leading dimension / row capacity of Linv, Kmat, work
  uint64_t serial = 0;           // unique per sgp_gp_create
  uint64_t data_version = 0;     // bumped by every fit / append / removal
  std::vector<double> xhost;     // host copy of the training rows (n x d): the EXACT
                                 // check behind a hash match of two GPs' inputs
  std::vector<uint64_t> xhash;   // xhash[i]: hash of the first i + 1 training rows
  uint64_t prov = 0;             // hash of the operations that led to this factor
                                 // (fit at n, appends, removals): two GPs with equal
                                 // inputs AND equal history have the same bits in L^-1
  bool upd_valid = false;  // dev.upd* describes the step to the current data
  bool rem_valid = false;  // ... as the record of a REMOVAL (sgp_gp_remove): the row that left,
                           // in the layout of an append of that row to the reduced GP
  bool blk_valid = false;  // `blk` describes the step to the current data: the last change was
                           // a block append (sgp_gp_append_block); a clone carries none
  bool rw_valid = false;   // ... as the record of a RE-WEIGHTING in place (sgp_gp_reweigh): x_i,
                           // w = -p / P_ii off row i, upd[0] = P_ii eta, upd[1] = tau P_ii^2
  // noise scales r_i of the observations (Ky = K + diag((noise_var + 1e-8) r_i) + jitter I):
  // empty = the GP never received one, all ones, and runs the code without scales.  `R` is the
  // device image of rhost (sync_scales), read by the fit and the likelihood kernels.
  std::vector<double> rhost;
  bool factored = true;    // false: sgp_gp_lml / sgp_gp_loo_lml met a non-positive pivot: the data are
                           // resident, the factor is not valid until the next fit
  DevBuf X, Y, Xpad, Xs, XA, alpha, Apack, Linv, Kmat, work, tvec, updw, upd, blk, R;
  GpDev dev;      // filled by set_data
};

struct sgp_grid {
  sgp_ctx* ctx = nullptr;
  int64_t N = 0;
  int d = 0;
  int G = 0;
  int64_t goff = 0;
  double* pts = nullptr;     // SoA [d][N]
  double* Q = nullptr;       // [N][2G]
  double* mean = nullptr;    // [G][N]
  double* var = nullptr;     // [G][N]
  double* var_h = nullptr;   // [G][N] hallucinated variances of a batch (sgp_grid_batch_next):
                             // allocated by the first batch, written before it is read
  uint8_t* S = nullptr;      // [N]
  uint8_t* M = nullptr;
  uint8_t* Gm = nullptr;
  uint8_t* cand = nullptr;   // candidate mask s
  double* w = nullptr;       // [N] max_i(u_i - l_i) of candidates
  double* partial = nullptr; // block partials
  int64_t partial_cap = 0;
  GpDev* gpdev = nullptr;    // [SGP_MAX_GPS] device copy of descriptors
  GpDev gpdev_host[SGP_MAX_GPS];   // ... and what it holds (stage_gpdev)
  int gpdev_count = 0;
  double* scal = nullptr;    // [8] resident scalars: [0] = max l0 over S
  int l0_pending = 0;        // > 0: scal[0] is still spread over that many
                             // entries of `partial` (deferred confidence pass)
  bool post_valid = false;   // mean / var hold the posterior of the resident rows: set by the
                             // passes that sweep them (sgp_grid_confidence, sgp_grid_posterior,
                             // sgp_grid_step_small), cleared when the rows change
                             // (sgp_grid_set_context); what sgp_grid_mes asks for
  // tensor-grid structure (sgp_grid_set_axes; SepLaunch)
  bool axes_valid = false;
  uint32_t ax_count[SGP_MAX_D] = {0};
  uint32_t ax_stride[SGP_MAX_D] = {0};
  int ax_off[SGP_MAX_D] = {0};          // first entry of column k's axis in ax_vals
  std::vector<double> ax_host;          // axis values, concatenated
  DevBuf ax_vals;                       // ... on the device
  uint64_t ax_version = 0;              // bumped when an axis value changes (context)
  DevBuf sep_tab[SGP_MAX_GPS];          // factor tables of the GP in slot g
  uint64_t sep_key[SGP_MAX_GPS][3] = {{0}};   // (gp serial, data version, axes version)
};

// ---- helpers (api.hip) ------------------------------------------------------
int sgp_reserve(sgp_ctx* ctx, DevBuf* b, size_t bytes);
void* scratch_slot(sgp_ctx* ctx, ScratchSlot slot, size_t bytes);  // nullptr on failure
// *out = `bytes` of the slot, or the usual error (through SGP_TRY)
template <class T>
inline int sgp_scratch(sgp_ctx* ctx, ScratchSlot slot, size_t bytes, T** out) {
  *out = static_cast<T*>(scratch_slot(ctx, slot, bytes));
  SGP_CHECK(ctx, *out, "device allocation failed: %s", ctx->err.c_str());
  return 0;
}
int sgp_poison(sgp_ctx* ctx, void* p, size_t bytes);       // SGP_POISON=1: fill a fresh allocation with 0xFF
int sgp_h2d(sgp_ctx* ctx, void* dst, const void* src, size_t bytes);
int sgp_d2h(sgp_ctx* ctx, void* dst, const void* src, size_t bytes);  // syncs
// host[g] = descriptor of gps[g] (fitted, in ctx, input dimension d), GpDev::share set
int collect_gps(sgp_ctx* ctx, sgp_gp* const* gps, int G, int d, GpDev* host);

// GPy's util.linalg.jitchol around any factorisation: attempt(jitter, &info) factorises with
// that much added to the diagonal (info = 0, or the first pivot that is not positive); after a
// failure at 0 the jitter starts at diag_mean() * 1e-6 -- asked for only then -- and grows
// tenfold per retry, five retries.  *info / *jitter_used describe the last attempt.
template <class DiagMean, class Attempt>
inline int jitchol_loop(DiagMean diag_mean, Attempt attempt, int* info, double* jitter_used) {
  *info = 0;
  *jitter_used = 0.0;
  SGP_TRY(attempt(0.0, info));
  if (*info != 0) {
    double dm = 0.0;
    SGP_TRY(diag_mean(&dm));
    double jitter = dm * 1e-6;
    for (int t = 0; t < 5 && *info != 0 && std::isfinite(jitter); ++t) {
      *jitter_used = jitter;
      SGP_TRY(attempt(jitter, info));
      jitter *= 10.0;
    }
  }
  return 0;
}

// ---- kernel launchers (implemented in the .hip files) -----------------------
// factor.hip
// Cholesky factor (-> lower part of A) and its inverse (-> Li, zeroed by the caller) of the
// s x s matrix A, s a multiple of 32; T: workspace; all three with pitch ld.  *info_dev
// (zeroed by the caller) receives the first pivot that is not positive (1-based).
int factor_dense(sgp_ctx* ctx, double* A, double* Li, double* T, int64_t ld, int s,
                 int* info_dev);
// C (m x n) = alpha A (m x k) op(B) + beta C, row-major, op(B) = B^T with B (n x k) when transB:
// the VALU GEMM of the factorisation
int gemm_dense(sgp_ctx* ctx, bool transB, int m, int n, int k, double alpha, const double* A,
               int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
// joint.hip: the bodies of sgp_gp_predict_cov / sgp_gp_posterior_draw behind the argument checks
int joint_predict_cov(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                      int64_t stride_col, double* mean, double* cov);
int joint_posterior_draw(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                         int64_t stride_col, const double* Z, int S, double* out, double* mean,
                         int* chol_info, double* jitter_used);
// T[c][i] = sum_{j <= i} Li[i][j] V[c][j]  and  W[c][j] = sum_{i >= j} Li[i][j] T[c][i]
// (0 for n <= j < n_out): the triangular mat-vecs behind alpha, m <= 16 right-hand sides
int tri_mv_dense(sgp_ctx* ctx, const double* Li, int64_t ld, int n, const double* V,
                 int64_t ldv, int m, double* T, int64_t ldo);
int tri_mtv_dense(sgp_ctx* ctx, const double* Li, int64_t ld, int n, const double* T,
                  int64_t ldt, int m, double* W, int64_t ldo, int n_out);
int launch_kernel_matrix(sgp_ctx* ctx, const KernDesc& kd, const double* X1,
                         int64_t n1, const double* X2, int64_t n2, double* out,
                         int64_t ld, int symmetric_diag, double diag_add,
                         int64_t n_valid, const double* diag_vec = nullptr);
// Kmat -> Linv, Apack, alpha (info_dev_out: the pivot word stays on the device, factor.hip)
int factor_gp(sgp_gp* gp, int* info, const int** info_dev_out = nullptr);
// hyper.hip: log marginal likelihood and gradient of a GP factor_gp has just factorised
int lml_result_words(const KernDesc& kd);   // 2 + P + P d values and the pivot word
int launch_lml(sgp_gp* gp, const int* info_dev, double* out_dev);
// ... the leave-one-out objective and gradient in the same block, likewise
int launch_loo_lml(sgp_gp* gp, const int* info_dev, double* out_dev);
// leave-one-out predictions from the factor as it stands: *out_dev = [mean | var] (*np doubles
// each, n rounded up to 64) | sum of the log predictive densities | info (as a double)
int launch_loo(sgp_gp* gp, const double** out_dev, int* np);
// row n already in gp->X; r: the noise scale of the new row (1: as without scales)
int append_gp(sgp_gp* gp, double y, int* info, double r = 1.0);
// rows n .. n + b - 1 already in gp->X / gp->Y, 1 <= b <= SGP_MAX_BLOCK, n + b <= ld; *info != 0
// leaves the GP untouched; r: the b noise scales of the new rows, or null (all ones)
int append_block_gp(sgp_gp* gp, int b, int* info, const double* r = nullptr);
int pop_gp(sgp_gp* gp);
// observation `index` becomes (y_new, noise variance + delta) in place;
// *info != 0 leaves the GP untouched
int reweigh_gp(sgp_gp* gp, int index, double y_new, double delta, int* info);
// the diagonal of Ky at a row of noise scale r, k(x,x) + (noise_var + 1e-8) r + jitter, in the
// evaluation order of the unscaled code: at r = 1 the same bits
inline double row_prior(const sgp_gp* gp, double r) {
  return gp->kern.kdiag + gp->noise_var * r + 1e-8 * r + gp->jitter;
}
// row `index` leaves (0 <= index < n, n >= 2); *info != 0 leaves the GP untouched
int remove_gp(sgp_gp* gp, int index, int* info);
int publish_gp(sgp_gp* gp);  // Apack / Xpad / Xs / dev descriptor from Linv
// right-hand sides of a triangular product, candidates of a group of the expander test
constexpr int kMaxRhs = 16;
// expander.hip
struct ExpanderOps {      // all arrays on the device; [g] blocks as noted
  const double* xc;       // [m][d] candidates
  const double* resid;    // [G][16]  u_c - mu_c
  double* Wpack;          // [G][wstride]  A operands (cand x j) of Ky^-1 k_c
  double* delta;          // [G][16]
  double* inv_s2;         // [G][16]
  double* tn2;            // [G][16]
  int64_t wstride;
  int m;                  // candidates; more than 16: groups of 16, arrays [group][Gs][...]
  int Gs;                 // GP slots of the [group][Gs] layouts (the launch's G)
  int active[SGP_MAX_GPS];
};
struct FrontArgs;   // sets_front.h: the fold of the front half's last step into k_expkt
// operands of every active GP in three launches (all GPs per launch)
int expander_operands_all(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                          int G, int d, const ExpanderOps& ops,
                          const FrontArgs* fold = nullptr);

// sweep.hip
struct SweepPoints {
  const double* base;
  int64_t N;
  int64_t stride_row;  // elements
  int64_t stride_col;
};
struct ConfOut {
  double* Q;        // [N][2G] or null
  double* mean;     // [G][N]
  double* var;      // [G][N]
  uint8_t* S;       // [N] or null
  double* partial;  // [nblocks] max l0 over safe rows of the block, or null
  double beta;
  double fmin[SGP_MAX_GPS];
};
// The swarm type of sgp_swarm_fitness_path / sgp_swarm_run_path inside the library (the
// public entry points that take a swarm type keep to SGP_SWARM_GREEDY .. SGP_SWARM_SAFE_SET)
constexpr int kSwarmThompson = 4;
// ... and of sgp_swarm_fitness_mes / sgp_swarm_run_mes: max-value entropy search.  The shaping
// pass treats it as kSwarmThompson (value = total_pen, the maximizers' safety rule); the term
// on top is alpha of GP 0's posterior (launch_swarm_mes behind the shaping launch)
constexpr int kSwarmMes = 5;
// The maxima of a 'mes' swarm as the kernel takes them
struct SwarmMes {
  const double* ystar;   // [K] on the device (SwarmMesLayout), not floored
  int K;                 // 1 .. SGP_MAX_MES; 0: not a 'mes' swarm
  double floor;          // -inf: none
  double* post;          // [2][P] on the device: receives mean | var of GP 0, or null
};
// mes.hip: 1 <= K <= SGP_MAX_MES and every ystar[k] (host) finite
int mes_checks(sgp_ctx* ctx, const double* ystar, int K);
// values[p] = alpha(mean[p], var[p]) + values[p] over P particles (k_swarm_mes)
int launch_swarm_mes(sgp_ctx* ctx, int64_t P, const double* mean, const double* var,
                     const SwarmMes& m, double* values);
// ... and of sgp_swarm_fitness_ise / sgp_swarm_run_ise: information-theoretic safe exploration.
// The same branch of the shaping pass; the term on top is alpha = max_t pair(p, t) over the
// staged targets (launch_swarm_ise behind the shaping launch)
constexpr int kSwarmIse = 6;
// ... and of sgp_swarm_fitness_ei / sgp_swarm_run_ei: log expected improvement.  The same
// branch of the shaping pass; the term on top is ei_alpha (ei_term.h) of all G GPs' posterior
// (launch_swarm_ei behind the shaping launch)
constexpr int kSwarmEi = 7;
// What an expected-improvement call fixes for all its rows (a kernel argument by value; the
// arithmetic on it is ei_term.h's alone)
struct EiTerm {
  int kind;                  // SGP_EI_EI | SGP_EI_PI
  int G;                     // GPs of the posterior; the feasibility weights walk all of them
  double xi;
  double fmin[SGP_MAX_GPS];  // -inf: GP g is not weighed
};
// The incumbent of an 'ei' swarm as the kernel takes it
struct SwarmEi {
  EiTerm term;
  double tau;
  int on;                // 0: not an 'ei' swarm
  int free;              // 1: values = alpha, safe = 1 (no penalty, no safety rule)
  double* alpha;         // [P] on the device: receives alpha, or null
  double* post;          // [G][2][P] on the device: receives mean | var per GP, or null
};
// ei.hip: values[p] = ei_alpha(p) + values[p] (free: = ei_alpha(p), safe[p] = 1) over P
// particles whose posterior is mean / var [G][P] (k_swarm_ei)
int launch_swarm_ei(sgp_ctx* ctx, int G, int64_t P, const double* mean, const double* var,
                    const SwarmEi& m, double* values, uint8_t* safe);
// The block of an 'ei' swarm fitness call in kSlotEiIn (sgp_swarm_fitness_ei; neither
// swarm_fitness nor swarm_run asks for this slot): alpha[P] | post[G][2][P], each only when
// the call asks for it
struct SwarmEiLayout {
  size_t alpha, post, bytes;
};
constexpr SwarmEiLayout swarm_ei_layout(int64_t P, int G, bool alpha, bool post) {
  SwarmEiLayout l{};
  l.alpha = 0;
  l.post = alpha && P > 0 ? size_t(P) * 8 : 0;
  l.bytes = l.post + (post && P > 0 ? 2 * size_t(G) * size_t(P) * 8 : 0);
  return l;
}
static_assert(swarm_ei_layout(3, 2, true, true).post == 24 &&
                  swarm_ei_layout(3, 2, true, true).bytes == 24 + 96 &&
                  swarm_ei_layout(3, 2, false, true).bytes == 96 &&
                  swarm_ei_layout(3, 2, true, false).bytes == 24,
              "SwarmEiLayout: post overlaps alpha or ends outside the block");
// ise.hip: W = Ky^-1 k(X, x_j) of the K points xc [K][d] (device) in [n_pad][Kp], Kp a multiple
// of 64, W zeroed by the caller, T an [n][Kp] workspace: the operand kernels of sgp_grid_ise
int launch_ise_operands(sgp_ctx* ctx, sgp_gp* gp, const double* xc, int K, int Kp, double* W,
                        double* T);
// The targets of an 'ise' swarm as the kernel takes them (swarm_ise.hip), all on the device
struct SwarmIse {
  const double* W[SGP_MAX_GPS];  // [n_pad][Tp], zero padded; null for an inactive GP
  const double* tg;              // [Tp][d] targets, zero rows behind T
  const double* zmean;           // [G][Tp] the targets' posterior
  const double* zvar;
  int T, Tp;                     // 1 .. SGP_MAX_ISE, rounded up to 64
  unsigned active;               // bit g: GP g has a finite fmin
  double s[SGP_MAX_GPS];         // noise_var + 1e-8
  int n_pad[SGP_MAX_GPS];        // rows of W_g
  double* alpha;                 // [P], or null
  long long* target;             // [P], or null
  double* post;                  // [G][2][P] mean | var per GP, or null
  double* pairs;                 // [P][T], or null
  double* cov;                   // [G][P][T] (zeroed by the stage), or null
  double* bestv;                 // [P] scratch of the kernel: a row's best pair, block to block
  long long* bestt;              // [P] ... and its column
  // what the fitness / run routine adds: the particles and the descriptors on the device
  const GpDev* gps_dev;
  const double* base;            // SweepPoints of the particles
  int64_t stride_row, stride_col;
  int d;
};
// values[p] = max_t pair(p, t) + values[p] over P particles whose posterior is mean / var [G][P]
int launch_swarm_ise(sgp_ctx* ctx, int G, int64_t P, const double* mean, const double* var,
                     const double* fmin, const SwarmIse& m, double* values);
struct FitnessArgs {
  int swarm_type;
  double beta;
  double fmin[SGP_MAX_GPS];
  double scaling[SGP_MAX_GPS];
  double best_lower_bound;
  double* values;
  uint8_t* safe;
  // a hallucinated swarm (sgp_swarm_*_hall; null otherwise): [G][P] what the pending picks
  // of the batch take off the variance (launch_swarm_down) -- the width term alone sees
  // var_h = max(var - down, 1e-15); var_h: [G][P] receives it, or null
  const double* down;
  double* var_h;
  // a 'mes' swarm (swarm_type == kSwarmMes; K = 0 otherwise): read by launch_fitness_small on
  // the host, which launches the term behind the shaping kernel -- no kernel reads it
  SwarmMes mes;
  // an 'ei' swarm (swarm_type == kSwarmEi; on = 0 otherwise): likewise read by
  // launch_fitness_small on the host alone -- no kernel reads it
  SwarmEi ei;
  // an 'ise' swarm (swarm_type == kSwarmIse; null otherwise): a HOST pointer, read by
  // launch_fitness_small alone, which launches the term behind the shaping kernel
  const SwarmIse* ise;
};
// rows_sharded: the rows are a rank's shard of a grid -- the sweep kernel is then chosen
// by the GPs alone (the same on every rank), never by the number of rows
int launch_sweep_conf(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                      int G, int d, SweepPoints pts, ConfOut out,
                      const SepLaunch* sep = nullptr, bool rows_sharded = false);
// per-axis factor tables of one GP (SepLaunch::tab): out[a] = table of axis a =
// column cols[a] (count[cols[a]] points); the columns with one point are folded into
// out[0]
int launch_sep_tables(sgp_ctx* ctx, const GpDev& gp, int d, const uint32_t* count,
                      const double* axis_vals, const int* axis_off, int naxes,
                      const int* cols, double* const* out);
size_t sep_table_doubles(const GpDev& gp, uint32_t count);
// j-blocks a factor table has at least: the resident-factor kernel walks the j-blocks of the
// LARGEST factor of its launch (up to kMidMaxNB, sweep_mid.hip; at least 4) for every GP -- the
// blocks beyond a GP's own meet zeros of its L^-1, but they have to be there, and finite
constexpr int kSepMinBlocks = 8;
// rows == the declared tensor grid?  *mismatch (device int) counts the differences
int launch_verify_axes(sgp_grid* g, int* mismatch_dev);
int launch_sweep_fitness(sgp_ctx* ctx, const GpDev* gps_dev,
                         const GpDev* gps_host, int G, int d, SweepPoints pts,
                         FitnessArgs fa, int64_t sel_rows = -1);
// paths.hip: ONE sample path of GP 0 as the fitness term of a Thompson swarm
struct SwarmPath {
  const double* om;   // [m16][d + 1]: frequency | phase, zero rows behind m
  const double* wv;   // [m16] amp w (zeros behind m), then [n_pad] v (zero padded)
  int m16;            // features rounded up to 16
  int ncov;           // the GP's n_pad
};
// the argument checks of sgp_gp_paths_eval for one path
int swarm_path_ready(sgp_gp* gp, int m);
// stages the path on the device (once per entry-point call)
int swarm_path_stage(sgp_gp* gp, const double* Omega, const double* phase, int m,
                     const double* w, const double* v, SwarmPath* out);
// values[p] = f(x_p) / scaling0 + values[p] over the rows of pts, gps_dev[0] the path's GP
int launch_swarm_path(sgp_ctx* ctx, const GpDev* gps_dev, int d, const SwarmPath& path,
                      SweepPoints pts, double scaling0, double* values);
// swarm_batch.hip: down[g][p] = sum_j t_j(x_p)^2 over the b tail rows of clone g's L^-1 (the
// pending picks of a hallucinated batch), for the rows of pts; the clones' descriptors with
// GpDev::share as collect_gps sets it
int launch_swarm_down(sgp_ctx* ctx, const GpDev* clones_dev, int G, int d, int b,
                      SweepPoints pts, double* down);
// swarm_api.hip: what the sgp_swarm_fitness* / sgp_swarm_run* entry points hand to the
// one fitness routine and the one run routine.
struct SwarmSpec {             // what the fitness is
  sgp_gp* const* gps;
  int G;
  int swarm_type;              // SGP_SWARM_*, kSwarmThompson with a path, kSwarmMes with maxima
  double beta;
  const double* fmin;          // [G]
  const double* scaling;       // [G]
  double best_lower_bound;
  const SwarmPath* path;       // a Thompson swarm: the STAGED path; null otherwise
  sgp_gp* const* clones;       // a hallucinated swarm: [G]; null otherwise
  const SwarmMes* mes;         // a 'mes' swarm: the STAGED maxima; null otherwise
  const struct SwarmIseIn* ise = nullptr;   // an 'ise' swarm: the caller's targets (host); the two
                               // routines stage them behind their checks (swarm_ise_stage)
  const SwarmEi* ei = nullptr; // an 'ei' swarm: incumbent, term and output buffers; null otherwise
};
struct SwarmIseIn {
  const double *targets, *zmean, *zvar;   // (T,d), (G,T), (G,T) on the host
  int T;
  // outputs of a fitness call (host), each may be null
  double* alpha;
  int64_t* target;
  double *post, *pairs, *cov;
};
// swarm_ise.hip.  "no GP", 1 <= T <= SGP_MAX_ISE, targets / zmean / zvar present and finite with
// every zvar >= 0, one GP active: the checks in front of an entry point's early return
int swarm_ise_checks(sgp_ctx* ctx, sgp_gp* const* gps, int G, const double* fmin,
                     const SwarmIseIn& in);
// pairs / cov are test outputs: G P T <= 2^24
int swarm_ise_out_check(sgp_ctx* ctx, int G, int64_t P, const SwarmIseIn& in);
// targets, their posterior and the operands onto the device, ONCE per call (host: collect_gps')
int swarm_ise_stage(sgp_ctx* ctx, sgp_gp* const* gps, const GpDev* host, int G, int d,
                    const double* fmin, const SwarmIseIn& in, int64_t P, SwarmIse* out);
// the outputs a fitness call asked for, back to the host
int swarm_ise_read(sgp_ctx* ctx, const SwarmIseIn& in, const SwarmIse& m, int G, int64_t P);
struct SwarmState {            // the caller's arrays (host), rows [p0, p0 + P) of a swarm of Pt
  double *positions, *velocities, *best_positions, *best_values, *global_best;
  const double *velocity_scale, *bounds;   // bounds may be null
  int64_t P, p0, Pt;
};
struct PsoSchedule {
  int init, iters;
  double inertia0, step_size;
  const double* rand;          // null: the device generator with `seed`
  uint64_t seed;
};
// api.hip: the context's collectives on DEVICE operands -- RCCL in stream, or the host
// transport of sgp_comm_init_host (sgp_grid_paths_comm merges its records behind one)
// (defined inside api.hip's extern "C" block)
extern "C" int comm_or_single(sgp_ctx* ctx, bool* comm);   // is there one?  Error: rank of several without
// recv (device) = the nbytes of every rank, in rank order
extern "C" int coll_allgather(sgp_ctx* ctx, const void* send, void* recv, size_t nbytes);
// dev[n] (device) = the element-wise maximum over the ranks; no communicator: untouched
extern "C" int coll_allreduce_max_f64(sgp_ctx* ctx, double* dev, size_t n);
// few-points posterior / small-swarm step: small_path.h
constexpr int kSmallPoints = 4096;  // few-points posterior path (factor.hip)
constexpr int kSmallSwarm = 64;     // ... with the whole PSO step in one workgroup (swarm.hip)
struct ExpanderArgs {
  const double* Wpack;   // [G][n_pad_max/4][64] MFMA A-operand (cand x j)
  const double* xc;      // [m][d]
  const double* delta;   // [G][16]  (u_c - mu_c) / s2
  const double* inv_s2;  // [G][16]
  const double* tn2;     // [G][16]  |L^-1 k(X, x_c)|^2
  const double* stn;     // k_expander_many: [group][G][16] |L^-1 k_c| and the posterior
  const double* svc;     // standard deviation at x_c (written by launch_expander_many)
  const double* agg;     // ... [group][G][4] extremes of a group, box [group][2][d] (k_pass_agg)
  const double* box;
  const double* sagg;    // the same per SUPERGROUP of 8 consecutive groups (the scan of the grid
  const double* sbox;    // tests those first): [super][G][4], [super][2][d]
  int m;
  double beta;
  double fmin[SGP_MAX_GPS];
  int active[SGP_MAX_GPS];
  const uint8_t* S;
  const double* mean;    // [G][N]
  const double* var;
  int32_t* flags;        // [16][G] device
  int64_t wstride;       // doubles between consecutive GPs in Wpack
  double near_frac;      // >0: only rows with k(x,x_c) >= near_frac * k(x,x)
  int* count;            // m == 1: number of rows that passed the pre-filter
  int* list;             //         (zeroed by the caller) / their local indices
  int* wcount;           // k_expander_many: the 16-row segments with a possible pair, per GP
  int* wlist;            // (count, [G][N / 16] segments, masks of their listed rows); count /
  unsigned* wmask;       // list: the rows that pass the pair test of some candidate, [G][N]
};
// expander.hip
int launch_expander_check(sgp_ctx* ctx, const GpDev* gps_dev,
                          const GpDev* gps_host, int G, int d, SweepPoints pts,
                          ExpanderArgs ea);
// ea.m candidates in groups of 16, every per-candidate array [group][G][...] (flags
// [candidate][G]): expander.hip, k_expander_many
int launch_expander_many(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                         ExpanderArgs ea);
struct Rank1Args {
  double* Q;
  double* mean;
  double* var;
  uint8_t* S;
  double* partial;
  double beta;
  double fmin[SGP_MAX_GPS];
  int which[SGP_MAX_GPS];
};
int rank1_num_blocks(int64_t N);
// kind: the records are append records, removal records (sgp_gp_remove) -- both signs of the
// update flip -- or reweigh records (sgp_gp_reweigh): mean += c u0, var += c^2 u1
constexpr int kRank1Append = 0, kRank1Remove = 1, kRank1Reweigh = 2;
int launch_rank1(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d,
                 SweepPoints pts, Rank1Args ra, int kind = kRank1Append);
// block.hip: the same refresh after a block append on the flagged GPs (their records: blk); partials
// as launch_rank1 leaves them (rank1_num_blocks)
struct RankbArgs {
  Rank1Args r;
  const double* blk[SGP_MAX_GPS];   // the block records of the flagged GPs (device), else null
};
int launch_rankb(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                 const RankbArgs& ra);

// batch.hip: one pick of a hallucinated batch (sgp_grid_batch_next).  Every GP carries the
// append record of the previous pick: var_out = max(var_in - c(x)^2 / s2, 1e-15) per row and
// GP (var_in = the resident var for the first downdate of a batch, var_h afterwards), the
// intervals mean -+ beta sqrt(var_out), and the masked arg-max of their value over the rows
// not picked before, in the same pass.
struct BatchArgs {
  const double* mean;       // [G][N] resident, read only
  const double* var_in;     // [G][N]
  double* var_out;          // [G][N] (may be var_in: a row is read and written by one lane)
  const uint8_t* S;         // [N] masks, read only
  const uint8_t* M;
  const uint8_t* Gm;
  int mode;                 // SGP_ARGMAX_MG_WIDTH | SGP_ARGMAX_UCB
  double beta;
  double scaling[SGP_MAX_GPS];
  int64_t goff;
  int n_picked;
  int64_t picked[SGP_MAX_BATCH];   // global rows
  double* part_v;           // [blocks] best value of the workgroup's rows
  int64_t* part_i;          // [blocks] ... and its global row (-1: no eligible row)
};
int batch_num_blocks(int64_t N);
// The scratch of a pick, in kSlotPartials: [nb] values | [nb] rows | value | row -- the
// per-workgroup pairs and the pair the final kernel leaves behind them (read back together)
struct BatchScratch {
  double* part_v;
  int64_t* part_i;
  double* res_v;
  int64_t* res_i;
};
inline size_t batch_scratch_bytes(int nb) { return (size_t(nb) + 1) * 16; }
inline BatchScratch batch_scratch(void* base, int nb) {
  double* v = static_cast<double*>(base);
  int64_t* i = reinterpret_cast<int64_t*>(v + nb);
  return BatchScratch{v, i, reinterpret_cast<double*>(i + nb), i + nb + 1};
}
// the downdate and the per-workgroup pairs, then the final pair into (res_v, res_i)
int launch_batch_pick(sgp_ctx* ctx, const GpDev* gps_dev, int G, int d, SweepPoints pts,
                      BatchArgs ba, double* res_v, int64_t* res_i);
// A pick over the ranks (sgp_grid_batch_next_comm): behind the scratch of the shard's pick,
//   stop | records[world][3] | merged[3]
// (value, res_i) and `stop` are this rank's record {value, global row, stop}, 8 bytes each;
// the records are gathered in rank order and merged into {value, row, stop_any}.
constexpr size_t kBatchRecBytes = 24;
inline size_t batch_comm_scratch_bytes(int nb, int world) {
  return batch_scratch_bytes(nb) + 8 + (size_t(world) + 1) * kBatchRecBytes;
}
struct BatchCommScratch {
  double* rec;      // = BatchScratch::res_v
  double* recs;
  double* merged;
};
inline BatchCommScratch batch_comm_scratch(const BatchScratch& bs, int world) {
  double* rec = bs.res_v;
  return BatchCommScratch{rec, rec + 3, rec + 3 + 3 * size_t(world)};
}
// rec[2] = stop; with stop also rec[0..1] = {-inf, -1} (the rank runs no row kernel)
int launch_batch_stop(sgp_ctx* ctx, double* rec, int stop);
// k_batch_merge: one wave over the world records, before_first's order, the maximum stop
int launch_batch_merge(sgp_ctx* ctx, const double* recs, int world, double* out);

// sweep_tiny.hip: do the GPs of a launch go through the VALU kernel (every one with at most
// 48 observations)?
bool tiny_sweep_wanted(const sgp_ctx* ctx, const GpDev* gh, int Geff, int64_t rows,
                       bool rows_sharded);

// sweep_mid.hip: 49 .. 128 observations, single-part kernels, d <= 4, all GPs resident in LDS
bool mid_sweep_wanted(const sgp_ctx* ctx, const GpDev* gh, int Geff, int d);
// ... 129 .. 256 observations with factor tables (a tensor grid, RBF parts): in passes of row blocks
bool mid_passes_wanted(const sgp_ctx* ctx, const GpDev* gh, int Geff, const SepLaunch* sep,
                       const ConfOut& conf);

// sweep_pair.hip: does the launch take the paired-wave kernel (a GP with more than 256 rows)?
bool pair_sweep_wanted(const sgp_ctx* ctx, const GpDev* gh, int Geff);

// step_small.hip: a whole SafeOpt.optimize() of a small grid in one launch
constexpr int64_t kStepSmallRows = 16384;
bool step_small_eligible(const sgp_ctx* ctx, const GpDev* gh, int G, int64_t N);
// ... of many problems at once: opaque records of step_record_bytes() each, filled on the
// host (step_record_fill), uploaded by the caller and launched one group -- a run of `count`
// records of one kernel instance, step_group_key: 0 .. kStepGroupKeys - 1 -- at a time
constexpr int kStepGroupKeys = SGP_MAX_D * 3 * 2;
size_t step_record_bytes();
int step_group_key(int d, const GpDev* gh, int G);
void step_record_fill(void* rec, const sgp_grid* g, const GpDev* gps_dev, int G, double beta,
                      const double* fmin, const double* scaling, const double* thr_beta,
                      double* res, uint64_t seq);
int launch_step_small_group(sgp_ctx* ctx, int key, const void* recs_dev, int count);
int launch_step_small(sgp_grid* g, const GpDev* gps_dev, const GpDev* gh, int G, double beta,
                      const double* fmin, const double* scaling, const double* thr_beta,
                      double* res, uint64_t seq);
// count_dev != nullptr: the list was formed on the device, m is its room and *count_dev its length
int launch_cand_all(sgp_grid* g, const GpDev* gps_dev, const GpDev* gh, int G, double beta,
                    const double* fmin, const int64_t* clist_dev, int m, double* ops,
                    int32_t* flags, const int* count_dev = nullptr);
int launch_small_pack(sgp_grid* g, const int* list_dev, const int* count_dev, int cap,
                      int64_t* hdr, int64_t* clist, double* wout, int32_t* flags);
size_t cand_ops_doubles(int m, int G);
constexpr int kStepResWords = 64;     // doubles of the block: res_words(d, G) <= 50 (sets_front.h),
                                      // the last one the completion word

// sets.hip
int launch_reduce_max(sgp_ctx* ctx, const double* in, int64_t n, double* out);
int launch_safe_set(sgp_grid* g, const double* fmin);  // from Q -> S, partial
int launch_maximizers(sgp_grid* g, double max_l,
                      const double* max_l_dev = nullptr);  // device value wins
int launch_candidates(sgp_grid* g, double max_var, const double* max_width_dev,
                      const double* scaling, const double* thr_beta,
                      int full_sets, unsigned long long* counts_dev);
int launch_gather_top(sgp_grid* g, const int64_t* gidx_dev, double* x,
                      double* mean, double* Q);
int launch_stage_batch(sgp_grid* g, const int64_t* gidx_dev, const int* nfound_dev, int K,
                       double* xc, int n_xc_resid, int32_t* flags, int n_flag_words);
int launch_stage_top(sgp_grid* g, const double* x_top, const double* mean_top,
                     const double* q_top, double* xc, double* resid);
int launch_mark_top_if(sgp_grid* g, const int64_t* gidx_dev, const int* nfound_dev,
                       const int32_t* flags_dev, const double* fmin);
int launch_mark_if(sgp_grid* g, int64_t li, const int32_t* flags_dev,
                   const double* fmin);
// a pass of the expander loop over many candidates (sets.hip): selection by a histogram of
// kPassBins keys into a PassSel, operand staging, hits
constexpr int kPassBins = 4096;
// (internal linkage, like the pass kernels of sets.hip whose symbols name it: the launchers
// take it as void*)
namespace {
struct PassSel {
  double thr;      // the pass = candidates behind the cut with key >= thr
  int count;       // ... as k_pass_list counted them
  int est;         // ... as the histogram promised
};
}  // namespace
int launch_pass_select(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, double lo,
                       double hi, int want, void* sel_dev, int* list_dev, unsigned* hist_dev,
                       int* counts_dev);
int launch_pass_hist(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, double lo, double hi,
                     unsigned* hist_dev);
int launch_pass_list(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, void* sel_dev,
                     int* list_dev, int* counts_dev);
int launch_pass_gather(sgp_grid* g, const int* list_dev, int count, int mode, int64_t* gidx,
                       double* key, double* x, double* resid);
int launch_pass_stage(sgp_grid* g, const int* list_dev, int count, double* xc, double* resid);
// the Lipschitz test of many candidates (sets.hip: k_lip_*): rows and upper bounds staged from
// list_dev (local rows) or copied from the host arrays; work: the block of LipLayout
// (expander_layout.h) on the device
int launch_lipschitz_many(sgp_grid* g, int G, const double* fmin, const double* lipschitz,
                          const int* list_dev, int count, const double* xc_in, const double* uc_in,
                          double* work, int32_t* flags_dev);
int launch_pass_result(sgp_grid* g, const int* list_dev, int count, const int32_t* flags_dev,
                       const double* fmin, int mode, double* res_dev);
int launch_topk(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, int k,
                double* w_out_dev, int64_t* idx_out_dev, int* n_out_dev);
int launch_count_ties(sgp_grid* g, const double* w_top_dev, const int* n_found_dev,
                      int* ties_dev);
int launch_lipschitz(sgp_grid* g, int G, const double* fmin,
                     const double* lipschitz, int m, const double* xc_dev,
                     const double* uc_dev, int32_t* flags_dev);
int launch_argmax(sgp_grid* g, int mode, const double* scaling,
                  double* value_dev, int64_t* idx_dev);
int launch_sets_front_fused(sgp_grid* g, double max_l, const double* l0_part,
                            int n_l0, const double* max_l_dev,
                            const double* scaling, const double* thr_beta,
                            double* res, double* max_l_slot, double* xc,
                            int n_xc_resid, int32_t* flags, int n_flag_words,
                            FrontArgs* fold = nullptr);
int launch_front_final(sgp_ctx* ctx, const FrontArgs& fa);
int argmax_marked_blocks(int64_t N);
int launch_merge_front(sgp_grid* g, const double* all, int world, int nfront, double* res,
                       double* xc, int n_xc_resid, int32_t* flags, int n_flag_words);
int launch_merge_argmax(sgp_ctx* ctx, const double* all, int world, double* out_v,
                        int64_t* out_i);
int launch_argmax_marked(sgp_grid* g, const double* scaling, const double* fmin,
                         const int32_t* flags_dev, const int64_t* cand_gidx_dev,
                         const int* nfound_dev, int32_t* flags_out,
                         double* value_dev, int64_t* idx_dev, double* host_part = nullptr);
int launch_fill_cols(sgp_grid* g, const double* c, int nc);
int launch_gather_rows(sgp_grid* g, const int64_t* lidx_dev, int m, double* x,
                       double* mean, double* var, double* Q);
int launch_mark(sgp_grid* g, const int64_t* lidx_dev, int m, int value = 1);
// sgp_swarm_grow's block in kSlotWork, sized from m, n and d (kGrowBlock fixes the serial
// step, not the size):
//   S[m][d] f64 | B[n][d] f64 | list[n] i32 (accepted candidates, in order) |
//   count (i32, padded to 8 B) | flag[n] u8 (1: rejected by S or by a candidate accepted
//   in an earlier block) | accept[n] u8 (the result, read back)
constexpr int kGrowBlock = 512;   // candidates whose order one workgroup resolves (swarm.hip)
struct GrowBufs {
  double* S;
  double* B;
  int* list;
  int* count;
  uint8_t* flag;
  uint8_t* accept;
};
struct GrowLayout {
  size_t S, B, list, count, flag, accept, bytes;
};
inline GrowLayout grow_layout(int64_t m, int64_t n, int d) {
  GrowLayout l;
  l.S = 0;
  l.B = l.S + size_t(m) * d * 8;
  l.list = l.B + size_t(n) * d * 8;
  l.count = l.list + (size_t(n) * 4 + 7) / 8 * 8;
  l.flag = l.count + 8;
  l.accept = l.flag + size_t(n);
  l.bytes = l.accept + size_t(n);
  return l;
}
inline GrowBufs grow_bufs(char* base, const GrowLayout& l) {
  return GrowBufs{reinterpret_cast<double*>(base + l.S), reinterpret_cast<double*>(base + l.B),
                  reinterpret_cast<int*>(base + l.list), reinterpret_cast<int*>(base + l.count),
                  reinterpret_cast<uint8_t*>(base + l.flag),
                  reinterpret_cast<uint8_t*>(base + l.accept)};
}
int launch_swarm_grow(sgp_ctx* ctx, const KernDesc& kd, const double* S, int64_t m,
                      const double* B, int n, double scale2, double thr, const GrowBufs& gb);
// The block of a swarm fitness call in kSlotWork (swarm_fitness, swarm_api.hip), P particles
// of d columns against G GPs:
//   pts[d][P] f64 | values[P] f64 | gpdev[SGP_MAX_GPS] | safe[P] u8 (padded to 8 B) |
//   with clones: clones[SGP_MAX_GPS] | down[G][P] f64 | var_h[G][P] f64
// and 64 bytes of slack behind the last region.
static_assert(sizeof(GpDev) % 8 == 0, "GpDev arrays keep what follows them 8-byte aligned");
struct SwarmFitLayout {
  size_t pts, values, gpdev, safe, clones, down, var_h, bytes;
};
struct SwarmFitBufs {
  double *pts, *values;
  GpDev* gpdev;
  uint8_t* safe;
  GpDev* clones;
  double *down, *var_h;
};
constexpr SwarmFitLayout swarm_fit_layout(int64_t P, int d, int G, bool clones) {
  const size_t nv = size_t(P) * 8, gd = sizeof(GpDev) * SGP_MAX_GPS;
  const size_t hall = clones ? size_t(G) * nv : 0;
  SwarmFitLayout l{};
  l.pts = 0;
  l.values = l.pts + nv * d;
  l.gpdev = l.values + nv;
  l.safe = l.gpdev + gd;
  l.clones = l.safe + (size_t(P) + 7) / 8 * 8;
  l.down = l.clones + (clones ? gd : 0);
  l.var_h = l.down + hall;
  l.bytes = l.var_h + hall + 64;
  return l;
}
inline SwarmFitBufs swarm_fit_bufs(char* base, const SwarmFitLayout& l) {
  return SwarmFitBufs{reinterpret_cast<double*>(base + l.pts),
                      reinterpret_cast<double*>(base + l.values),
                      reinterpret_cast<GpDev*>(base + l.gpdev),
                      reinterpret_cast<uint8_t*>(base + l.safe),
                      reinterpret_cast<GpDev*>(base + l.clones),
                      reinterpret_cast<double*>(base + l.down),
                      reinterpret_cast<double*>(base + l.var_h)};
}
// The block of a swarm run in kSlotWork (swarm_run, swarm_api.hip), the rank's P particles;
// world: the ranks of a sharded run, 0 for a whole swarm:
//   pos | vel | best [P][d] f64 each | best_values | values [P] f64 each |
//   gbest[d] | vscale[d] | bounds[2 d] | gpdev[SGP_MAX_GPS] |
//   sharded: this rank's record, then the gathered ones (value | index | x[d] each) |
//   safe[P] u8 | 64 bytes of slack |
//   with clones, from the next multiple of 64 bytes: clones[SGP_MAX_GPS] | down[G][P] f64
struct SwarmRunLayout {
  size_t pos, vel, best, best_values, values, gbest, vscale, bounds, gpdev, rec, recs, safe,
      clones, down, bytes;
};
struct SwarmRunBufs {
  double *pos, *vel, *best, *best_values, *values, *gbest, *vscale, *bounds;
  GpDev* gpdev;
  double *rec, *recs;
  uint8_t* safe;
  GpDev* clones;
  double* down;
};
constexpr size_t swarm_rec_bytes(int d) { return size_t(2 + d) * 8; }
constexpr SwarmRunLayout swarm_run_layout(int64_t P, int d, int G, int world, bool clones) {
  const size_t nd = size_t(P) * d * 8, nv = size_t(P) * 8, dd = size_t(d) * 8;
  const size_t gd = sizeof(GpDev) * SGP_MAX_GPS, nrec = swarm_rec_bytes(d);
  SwarmRunLayout l{};
  l.pos = 0;
  l.vel = l.pos + nd;
  l.best = l.vel + nd;
  l.best_values = l.best + nd;
  l.values = l.best_values + nv;
  l.gbest = l.values + nv;
  l.vscale = l.gbest + dd;
  l.bounds = l.vscale + dd;
  l.gpdev = l.bounds + 2 * dd;
  l.rec = l.gpdev + gd;
  l.recs = l.rec + (world ? nrec : 0);
  l.safe = l.recs + size_t(world) * nrec;
  const size_t plain = l.safe + size_t(P) + 64;
  l.clones = (plain + 63) / 64 * 64;
  l.down = l.clones + gd;
  l.bytes = clones ? l.down + size_t(G) * nv : plain;
  return l;
}
inline SwarmRunBufs swarm_run_bufs(char* base, const SwarmRunLayout& l) {
  auto f64 = [base](size_t off) { return reinterpret_cast<double*>(base + off); };
  return SwarmRunBufs{f64(l.pos), f64(l.vel), f64(l.best), f64(l.best_values), f64(l.values),
                      f64(l.gbest), f64(l.vscale), f64(l.bounds),
                      reinterpret_cast<GpDev*>(base + l.gpdev), f64(l.rec), f64(l.recs),
                      reinterpret_cast<uint8_t*>(base + l.safe),
                      reinterpret_cast<GpDev*>(base + l.clones), f64(l.down)};
}
// Every f64 / GpDev region of the two layouts starts on an 8-byte boundary, a region ends
// where the next one starts or in front of it, the last one inside `bytes`.
constexpr bool swarm_fit_layout_ok(int64_t P, int d, int G, bool clones) {
  const SwarmFitLayout l = swarm_fit_layout(P, d, G, clones);
  const size_t nv = size_t(P) * 8, gd = sizeof(GpDev) * SGP_MAX_GPS, np = size_t(P);
  const size_t at[] = {l.pts, l.values, l.gpdev, l.safe, l.clones, l.down, l.var_h, l.bytes};
  const size_t len[] = {nv * d, nv, gd, np, gd, size_t(G) * nv, size_t(G) * nv};
  const int n = clones ? 7 : 4;
  for (int i = 0; i < n; ++i) {
    if (i != 3 && at[i] % 8 != 0) return false;            // (3: safe, bytes)
    if (at[i] + len[i] > (i + 1 < n ? at[i + 1] : l.bytes)) return false;
  }
  return true;
}
constexpr bool swarm_run_layout_ok(int64_t P, int d, int G, int world, bool clones) {
  const SwarmRunLayout l = swarm_run_layout(P, d, G, world, clones);
  const size_t nd = size_t(P) * d * 8, nv = size_t(P) * 8, dd = size_t(d) * 8;
  const size_t gd = sizeof(GpDev) * SGP_MAX_GPS, nrec = swarm_rec_bytes(d);
  const size_t at[] = {l.pos, l.vel, l.best, l.best_values, l.values, l.gbest, l.vscale,
                       l.bounds, l.gpdev, l.rec, l.recs, l.safe, l.clones, l.down};
  const size_t len[] = {nd, nd, nd, nv, nv, dd, dd, 2 * dd, gd, world ? nrec : 0,
                        size_t(world) * nrec, size_t(P), gd, size_t(G) * nv};
  const int n = clones ? 14 : 12;
  for (int i = 0; i < n; ++i) {
    if (i != 11 && at[i] % 8 != 0) return false;           // (11: safe, bytes)
    if (at[i] + len[i] > (i + 1 < n ? at[i + 1] : l.bytes)) return false;
  }
  return !clones || l.clones % 64 == 0;
}
static_assert(swarm_fit_layout_ok(1, 1, 1, false) && swarm_fit_layout_ok(1, 1, 1, true) &&
                  swarm_fit_layout_ok(65, 3, SGP_MAX_GPS, true) &&
                  swarm_fit_layout_ok(33, 3, 2, false),
              "SwarmFitLayout: a region is misaligned or overlaps its neighbour");
static_assert(swarm_run_layout_ok(1, 1, 1, 0, false) && swarm_run_layout_ok(1, 1, 1, 0, true) &&
                  swarm_run_layout_ok(65, 3, SGP_MAX_GPS, 0, true) &&
                  swarm_run_layout_ok(33, 3, 2, 4, false) &&
                  swarm_run_layout_ok(33, 3, 2, 4, true),
              "SwarmRunLayout: a region is misaligned or overlaps its neighbour");
// The swarm kernels take the rank's block of particles [p0, p0 + P) of a swarm of P_total:
// e0 / e2 are the global element indices of the block's first r1 / r2 number on the
// device generator (0 / P d for a whole swarm).
int launch_pso_init_vel(sgp_ctx* ctx, int64_t P, int d, double* vel,
                        const double* vscale, const double* rand, uint64_t seed,
                        int64_t e0 = 0);
int launch_pso_move(sgp_ctx* ctx, int64_t P, int d, double* pos, double* vel,
                    const double* best, const double* gbest, const double* vscale,
                    const double* bounds, double inertia, const double* rand,
                    uint64_t seed, uint32_t draw, int64_t e0 = 0, int64_t e2 = -1);
// rec != nullptr: the global best of the block goes to the record
//   value | global index (i64) | x[d]
// (what the ranks gather; k_pso_gbest_merge picks the swarm's) instead of to gbest
int launch_pso_best(sgp_ctx* ctx, int64_t P, int d, const double* values,
                    const uint8_t* safe, const double* pos, double* best,
                    double* best_values, double* gbest, int init, double* rec = nullptr,
                    int64_t p0 = 0);
int launch_pso_gbest_merge(sgp_ctx* ctx, const double* recs, int world, int d, double* gbest);
int launch_import_points(sgp_ctx* ctx, const double* src, int64_t N, int d,
                         int64_t stride_row, int64_t stride_col, double* dst);
