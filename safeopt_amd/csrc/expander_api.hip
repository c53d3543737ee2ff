// The expander-test entry points of the C ABI (include/safeopt_hip.h): sgp_grid_expander_check,
// _expander_batch, _expander_pass, _lipschitz_pass, the N-rank pass in three calls
// (_pass_hist, _pass_list, _pass_test, _pass_lipschitz_test) and _expanders_small[_all] --
// host-side launch sequences around the kernels of expander.hip, sets.hip and step_small.hip.
// Every scratch block they size and carve is defined in expander_layout.h.
#include <string.h>

#include <cmath>
#include <vector>

#include "expander_layout.h"
#include "sets_front.h"

// doubles between consecutive GPs of a W operand block: the largest factor's n_pad / 4 k-steps
static int64_t w_stride(const GpDev* host, int G) {
  int np_max = 0;
  for (int i = 0; i < G; ++i) np_max = host[i].n_pad > np_max ? host[i].n_pad : np_max;
  return int64_t(np_max / 4) * 64;
}

// The operands of an expander test of up to SGP_TOPK candidates (kept slot: staged by the
// caller, on the device or from the host, then built by enqueue_expander).
int expander_bufs(sgp_grid* g, const GpDev* host, int G, ExpanderBufs* b) {
  const int64_t wstride = w_stride(host, G);
  const ExpanderLayout l = expander_layout(g->d, G, wstride);
  char* buf;
  SGP_TRY(sgp_scratch(g->ctx, kSlotOperands, l.bytes, &buf));
  *b = expander_bufs_at(buf, l, wstride);
  return 0;
}

// fmin of every GP slot and the GPs with a constraint, for the operands and the scan
static void fill_fmin_active(const double* fmin, int G, ExpanderArgs* ea, ExpanderOps* ops) {
  for (int i = 0; i < SGP_MAX_GPS; ++i) {
    ea->fmin[i] = (i < G) ? fmin[i] : -INFINITY;
    ea->active[i] = (i < G) && (fmin[i] != -INFINITY);
    ops->active[i] = ea->active[i];
  }
}

// Enqueue the expander test of m <= SGP_TOPK candidates (operands + scan) on the GPs `host`,
// staged in g->gpdev; the flags stay on the device (eb.flags).  xc == nullptr: eb already
// holds the candidates and zeroed flags (launch_stage_batch, the front fold, k_merge_front);
// else they come from the host arrays xc / mu_c / u_c.
int enqueue_expander(sgp_grid* g, const GpDev* host, const ExpanderBufs& eb, double beta,
                     const double* fmin, int m, const double* xc, const double* mu_c,
                     const double* u_c, double near_frac, const FrontArgs* fold) {
  sgp_ctx* ctx = g->ctx;
  const int d = g->d, G = g->G;
  SGP_CHECK(ctx, m >= 1 && m <= SGP_TOPK, "m = %d not in 1..%d", m, SGP_TOPK);
  if (xc) {
    // pinned staging block: xc | resid (descriptors have their own slot); previous users of
    // this block have completed (every call that writes it syncs before returning)
    const size_t hb = eb.l.staged + sizeof(GpDev) * SGP_MAX_GPS;
    SGP_CHECK(ctx, hb <= ctx->pinned_cap / 2, "staging buffer too small");
    char* stage = static_cast<char*>(ctx->pinned) + ctx->pinned_cap / 2;
    memset(stage, 0, eb.l.staged);
    memcpy(stage, xc, size_t(m) * d * 8);
    double* resid = reinterpret_cast<double*>(stage + eb.l.resid);
    for (int c = 0; c < m; ++c)
      for (int i = 0; i < G; ++i)
        resid[size_t(i) * 16 + c] = u_c[c * G + i] - mu_c[c * G + i];
    SGP_HIP(ctx, hipMemcpyAsync(eb.xc, stage, eb.l.staged, hipMemcpyHostToDevice,
                                ctx->stream));
    SGP_HIP(ctx, hipMemsetAsync(eb.flags, 0, eb.l.zeroed, ctx->stream));
  }
  ExpanderArgs ea{};
  ExpanderOps ops{};
  fill_fmin_active(fmin, G, &ea, &ops);
  ops.xc = eb.xc;
  ops.resid = eb.resid;
  ops.Wpack = eb.W;
  ops.delta = eb.delta;
  ops.inv_s2 = eb.inv_s2;
  ops.tn2 = eb.tn2;
  ops.wstride = eb.wstride;
  ops.m = m;
  SGP_TRY(expander_operands_all(ctx, g->gpdev, host, G, d, ops, fold));
  ea.Wpack = eb.W;
  ea.xc = eb.xc;
  ea.delta = eb.delta;
  ea.inv_s2 = eb.inv_s2;
  ea.tn2 = eb.tn2;
  ea.m = m;
  ea.beta = beta;
  ea.S = g->S;
  ea.mean = g->mean;
  ea.var = g->var;
  ea.flags = eb.flags;
  ea.wstride = eb.wstride;
  ea.near_frac = near_frac;
  // single candidate: pre-filter + listed contraction; the counter sits in the tail
  // behind the flags (zeroed with them), the list in scratch
  ea.count = &eb.tail->count;
  if (m == 1) SGP_TRY(sgp_scratch(ctx, kSlotList, (size_t(g->N) + 64) * sizeof(int), &ea.list));
  SweepPoints sp{g->pts, g->N, 1, g->N};
  return launch_expander_check(ctx, g->gpdev, host, G, d, sp, ea);
}

int sgp_grid_expander_check(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, int m, const double* xc,
                            const double* mu_c, const double* u_c,
                            double near_frac, int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  ExpanderBufs eb;
  SGP_TRY(expander_bufs(g, host, G, &eb));
  SGP_TRY(enqueue_expander(g, host, eb, beta, fmin, m, xc, mu_c, u_c, near_frac));
  std::vector<int32_t> fl(size_t(SGP_TOPK) * G);
  SGP_TRY(sgp_d2h(ctx, fl.data(), eb.flags, fl.size() * 4));
  memcpy(flags, fl.data(), size_t(m) * G * 4);
  return 0;
}

// One pass of the expander loop (gp_opt.py:557-612) over the next k candidates in visiting
// order with ONE stream synchronisation: top-k behind the cut -> their rows staged on the
// device as the operands of the test -> the exact scan over the unsafe rows -> widths,
// global indices, count and flags in one read-back.  (The step-by-step entry points --
// sgp_grid_topk, _gather_rows, _expander_check -- need a host round trip each; a grid
// without expanders, the usual state of a converged run, visits ALL its candidates every
// iteration.)  One rank: on N ranks the candidates of the shards are merged on the host.
int sgp_grid_expander_batch(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                            const double* fmin, int mode, double cut_w, int64_t cut_idx,
                            int k, double* w_out, int64_t* gidx_out, int* n_out,
                            int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SGP_CHECK(ctx, k >= 1 && k <= SGP_TOPK, "k = %d not in 1..%d", k, SGP_TOPK);
  constexpr BatchReadLayout rl = batch_read_layout();
  char* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, rl.bytes, &res));
  double* wd = reinterpret_cast<double*>(res + rl.w);
  int64_t* id = reinterpret_cast<int64_t*>(res + rl.idx);
  int* nd = reinterpret_cast<int*>(res + rl.n);
  if (mode == 1) cut_w = (cut_idx < 0) ? INFINITY : -double(cut_idx);
  SGP_TRY(launch_topk(g, mode, cut_w, cut_idx, k, wd, id, nd));
  ExpanderBufs eb;
  SGP_TRY(expander_bufs(g, host, G, &eb));
  SGP_TRY(launch_stage_batch(g, id, nd, k, eb.xc, int(eb.l.staged / 8), eb.flags,
                             int(eb.l.zeroed / 4)));
  SGP_TRY(enqueue_expander(g, host, eb, beta, fmin, k, nullptr, nullptr, nullptr, 0.0));
  // flags behind the top-k block of the scratch: one read-back for both
  SGP_HIP(ctx, hipMemcpyAsync(res + rl.flags, eb.flags, size_t(SGP_TOPK) * G * 4,
                              hipMemcpyDeviceToDevice, ctx->stream));
  char hbuf[rl.bytes];
  SGP_TRY(sgp_d2h(ctx, hbuf, res, batch_read_span(G)));
  memcpy(w_out, hbuf + rl.w, size_t(k) * sizeof(double));
  memcpy(gidx_out, hbuf + rl.idx, size_t(k) * sizeof(int64_t));
  memcpy(n_out, hbuf + rl.n, sizeof(int));
  memcpy(flags, hbuf + rl.flags, size_t(k) * G * 4);
  return 0;
}

// The scratch of a big pass (kept slot): the listed candidates (local rows) | the key
// histogram | the selection | per-chunk counts of the listing
static int pass_scratch(sgp_grid* g, PassScratch* ps) {
  const PassLayout l = pass_layout(g->N);
  char* sb;
  SGP_TRY(sgp_scratch(g->ctx, kSlotPass, l.bytes, &sb));
  *ps = pass_bufs(sb, l);
  return 0;
}

// The expander test of m listed candidates in one scan of the unsafe rows (k_expander_many):
// the operand / W / flag blocks of the kept slots, the operands of every active GP (staged
// GPs `host`), the scan.  The candidates are the first m of the device list of a pass
// (list) or come from the host: xc [m][d], resid [m][G] = u_g - mu_g at the candidate.
// *flags_dev: [m][G] flags, then their tail (ManyLayout::fl).
static int expander_many_test(sgp_grid* g, const GpDev* host, double beta, const double* fmin,
                              int m, const int* list, const double* xc, const double* resid,
                              int32_t** flags_dev) {
  sgp_ctx* ctx = g->ctx;
  const int d = g->d, G = g->G;
  const int64_t wstride = w_stride(host, G);
  const ManyLayout l = many_layout(m, d, G, wstride);
  double* ob;
  double* Wp;
  int32_t* dfl;
  SGP_TRY(sgp_scratch(ctx, kSlotManyOps, l.bytes, &ob));
  SGP_TRY(sgp_scratch(ctx, kSlotManyW, l.w_bytes, &Wp));
  SGP_TRY(sgp_scratch(ctx, kSlotManyFlags, l.fl.bytes, &dfl));
  const ManyBufs mb = many_bufs(ob, l);
  if (list) {
    SGP_HIP(ctx, hipMemsetAsync(ob, 0, l.staged, ctx->stream));
    SGP_TRY(launch_pass_stage(g, list, m, mb.xc, mb.resid));
  } else {
    std::vector<double> st(l.staged / 8, 0.0);
    memcpy(st.data(), xc, size_t(m) * d * 8);
    double* sres = st.data() + l.resid / 8;
    for (int c = 0; c < m; ++c)
      for (int i = 0; i < G; ++i)
        sres[(size_t(c >> 4) * G + i) * 16 + (c & 15)] = resid[size_t(c) * G + i];
    SGP_TRY(sgp_h2d(ctx, ob, st.data(), l.staged));
  }
  SGP_HIP(ctx, hipMemsetAsync(dfl, 0, l.flag_bytes, ctx->stream));
  ExpanderArgs ea{};
  ExpanderOps ops{};
  fill_fmin_active(fmin, G, &ea, &ops);
  ops.xc = mb.xc;
  ops.resid = mb.resid;
  ops.Wpack = Wp;
  ops.delta = mb.delta;
  ops.inv_s2 = mb.inv_s2;
  ops.tn2 = mb.tn2;
  ops.wstride = wstride;
  ops.m = m;
  ops.Gs = G;
  SGP_TRY(expander_operands_all(ctx, g->gpdev, host, G, d, ops, nullptr));
  ea.Wpack = Wp;
  ea.xc = mb.xc;
  ea.delta = mb.delta;
  ea.inv_s2 = mb.inv_s2;
  ea.tn2 = mb.tn2;
  ea.stn = mb.stn;
  ea.svc = mb.svc;
  ea.agg = mb.agg;
  ea.box = mb.box;
  ea.sagg = mb.sagg;
  ea.sbox = mb.sbox;
  ea.m = m;
  ea.beta = beta;
  ea.S = g->S;
  ea.mean = g->mean;
  ea.var = g->var;
  ea.flags = dfl;
  ea.wstride = wstride;
  ea.near_frac = 0.0;
  SweepPoints sp{g->pts, g->N, 1, g->N};
  SGP_TRY(launch_expander_many(ctx, g->gpdev, G, d, sp, ea));
  *flags_dev = dfl;
  return 0;
}

// The work and flag blocks of the Lipschitz test of m candidates (launch_lipschitz_many);
// *flags: [m][G], then their tail (LipLayout::fl).
static int lipschitz_bufs(sgp_grid* g, int m, double** work, int32_t** flags) {
  const LipLayout l = lip_layout(m, g->d, g->G);
  SGP_TRY(sgp_scratch(g->ctx, kSlotManyOps, l.bytes, work));
  return sgp_scratch(g->ctx, kSlotManyFlags, l.fl.bytes, flags);
}

// A pass of the expander loop over MANY candidates (gp_opt.py:557-612 where the loop has to
// go far: no expander among the first candidates -- or none at all, the state of a converged
// run -- and full_sets, which visits every safe row).  The next ~`want` candidates behind
// the cut (visiting order: key descending -- the width, or minus the row index in full_sets
// mode -- then index descending), chosen by a histogram of the keys instead of a sort, are
// ALL tested in one scan of the unsafe rows (k_expander_many); two stream synchronisations
// (the size of the pass, its result) whatever the number of candidates.
//   mode 0: out6 = { candidates tested, expanders among them, key and global row of the
//           FIRST expander in visiting order (nothing is marked: the caller settles exact
//           ties and marks), key below which the candidates are still untested (-inf: none
//           left), 0 }
//   mode 1: every expander of the pass is marked in G; out6[2..3] unused.
// key_lo / key_hi: range of the keys still behind the cut (histogram range; mode 0:
// 0 .. the width of the cut).  One rank.
//
// The selection of such a pass: *count candidates listed in ps, out6[0] / out6[4] set.
static int pass_select(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, double key_lo,
                       double key_hi, int want, double* out6, PassScratch* ps, int* count) {
  sgp_ctx* ctx = g->ctx;
  SGP_CHECK(ctx, want >= 1, "want = %d", want);
  SGP_CHECK(ctx, key_hi > key_lo, "empty key range %g .. %g", key_lo, key_hi);
  SGP_CHECK(ctx, g->N < (int64_t(1) << 31), "%lld rows", (long long)g->N);
  for (int i = 0; i < 6; ++i) out6[i] = 0.0;
  SGP_TRY(pass_scratch(g, ps));
  SGP_TRY(launch_pass_select(g, mode, cut_w, cut_idx, key_lo, key_hi, want, ps->sel, ps->list,
                             ps->hist, ps->counts));
  PassSel hs;
  SGP_TRY(sgp_d2h(ctx, &hs, ps->sel, sizeof(hs)));
  *count = hs.count;
  out6[0] = double(hs.count);
  // Nothing listed is the end only when the histogram counted nothing either (est == 0: thr is
  // -inf then).  The histogram bins by a product, the list compares with the bin's lower edge: a
  // key an ulp below the edge is counted in the picked bin and not listed.  The caller goes on
  // from thr (cut and top of the key range), where those keys fall into the top bin.
  out6[4] = (hs.count == 0 && hs.est == 0) ? -INFINITY : hs.thr;
  return 0;
}

// No GP with a constraint: the reference's loop over the GPs only continues (gp_opt.py:559,
// 580) and G_safe stays False -- the listed candidates count as tested, none is a hit, nothing
// is marked, and no arg-max is taken (-1: unknown).
static bool any_constraint(const double* fmin, int G) {
  for (int i = 0; i < G; ++i)
    if (fmin[i] != -INFINITY) return true;
  return false;
}

static int pass_without_constraint(double* out6) {
  out6[1] = 0.0;
  out6[2] = -INFINITY;
  out6[3] = -1.0;
  out6[5] = -1.0;
  return 0;
}

// the result of a pass and, behind it in the same read-back, the arg-max of the step
// (gp_opt.py:631-641 over M | G) for the case that the pass ends the loop without a hit
static int pass_result_and_argmax(sgp_grid* g, const int* list, int count, int32_t* dfl,
                                  size_t flag_bytes, const double* fmin, int mode,
                                  const double* scaling, double* out6) {
  sgp_ctx* ctx = g->ctx;
  double* res = flag_tail(dfl, flag_bytes)->res;
  SGP_TRY(launch_pass_result(g, list, count, dfl, fmin, mode, res));
  const bool spec = scaling != nullptr && mode == 0;
  if (spec)
    SGP_TRY(launch_argmax(g, SGP_ARGMAX_MG_WIDTH, scaling, res + 3,
                          reinterpret_cast<int64_t*>(res + 4)));
  double hr[5];
  static_assert(sizeof(hr) == sizeof(FlagTail::res), "the five words of a pass result");
  SGP_TRY(sgp_d2h(ctx, hr, res, sizeof(hr)));
  out6[1] = hr[0];
  out6[2] = hr[1];
  int64_t bi;
  memcpy(&bi, &hr[2], 8);
  out6[3] = double(bi);
  int64_t ai = -1;
  if (spec) memcpy(&ai, &hr[4], 8);
  out6[5] = double(ai);
  return 0;
}

int sgp_grid_expander_pass(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                           const double* fmin, int mode, double cut_w, int64_t cut_idx,
                           double key_lo, double key_hi, int want, const double* scaling,
                           double* out6) {
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  PassScratch ps;
  int count = 0;
  SGP_TRY(pass_select(g, mode, cut_w, cut_idx, key_lo, key_hi, want, out6, &ps, &count));
  if (count == 0) return 0;
  if (!any_constraint(fmin, G)) return pass_without_constraint(out6);
  int32_t* dfl;
  SGP_TRY(expander_many_test(g, host, beta, fmin, count, ps.list, nullptr, nullptr, &dfl));
  return pass_result_and_argmax(g, ps.list, count, dfl, many_flag_bytes(count, G),
                                fmin, mode, scaling, out6);
}

// The same pass with Lipschitz certificates (gp_opt.py:558-576 instead of :577-606): selection
// as above, then the distance test of ALL listed candidates in one scan (k_lip_*).  out6 as
// sgp_grid_expander_pass.  One rank.
int sgp_grid_lipschitz_pass(sgp_grid* g, int G, const double* fmin, const double* lipschitz,
                            int mode, double cut_w, int64_t cut_idx, double key_lo,
                            double key_hi, int want, const double* scaling, double* out6) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G == g->G, "grid was created for %d GPs, got %d", g->G, G);
  PassScratch ps;
  int count = 0;
  SGP_TRY(pass_select(g, mode, cut_w, cut_idx, key_lo, key_hi, want, out6, &ps, &count));
  if (count == 0) return 0;
  if (!any_constraint(fmin, G)) return pass_without_constraint(out6);
  double* work;
  int32_t* dfl;
  SGP_TRY(lipschitz_bufs(g, count, &work, &dfl));
  SGP_TRY(launch_lipschitz_many(g, G, fmin, lipschitz, ps.list, count, nullptr, nullptr, work, dfl));
  return pass_result_and_argmax(g, ps.list, count, dfl, lip_layout(count, g->d, G).flag_bytes,
                                fmin, mode, scaling, out6);
}

// ---- the same pass on N ranks, in three calls with the ranks' agreement in between ----------
// (SafeOpt._visit_in_big_passes_nrank): every rank's histogram of the keys behind the cut
// (the ranks sum them and pick ONE threshold), every rank's candidates above it with what the
// other ranks need of them (the ranks gather them: the same list everywhere), and the test of
// ALL those candidates against this rank's unsafe rows (the ranks OR the flags).
int sgp_grid_pass_hist(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, double key_lo,
                       double key_hi, uint32_t* hist) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, key_hi > key_lo, "empty key range %g .. %g", key_lo, key_hi);
  PassScratch ps;
  SGP_TRY(pass_scratch(g, &ps));
  SGP_TRY(launch_pass_hist(g, mode, cut_w, cut_idx, key_lo, key_hi, ps.hist));
  return sgp_d2h(ctx, hist, ps.hist, kPassBins * sizeof(uint32_t));
}

int sgp_grid_pass_list(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, double thr, int cap,
                       int* count, int64_t* gidx, double* key, double* x, double* resid) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, g->N < (int64_t(1) << 31), "%lld rows", (long long)g->N);
  PassScratch ps;
  SGP_TRY(pass_scratch(g, &ps));
  PassSel hs = {thr, 0, 0};
  SGP_TRY(sgp_h2d(ctx, ps.sel, &hs, sizeof(hs)));
  const int upper = mode & 2;            // resid = u_i (Lipschitz certificates) instead of u_i - mu_i
  mode &= 1;
  SGP_TRY(launch_pass_list(g, mode, cut_w, cut_idx, ps.sel, ps.list, ps.counts));
  SGP_TRY(sgp_d2h(ctx, &hs, ps.sel, sizeof(hs)));
  *count = hs.count;
  if (hs.count == 0) return 0;
  SGP_CHECK(ctx, hs.count <= cap, "%d candidates above the threshold, room for %d", hs.count, cap);
  const int d = g->d, G = g->G;
  const PassListLayout l = pass_list_layout(hs.count, d, G);
  double* ob;
  SGP_TRY(sgp_scratch(ctx, kSlotManyOps, l.bytes, &ob));
  const PassListBufs pb = pass_list_bufs(ob, l);
  SGP_TRY(launch_pass_gather(g, ps.list, hs.count, mode | upper, pb.gidx, pb.key, pb.x, pb.resid));
  std::vector<double> host(l.bytes / 8);
  SGP_TRY(sgp_d2h(ctx, host.data(), ob, l.bytes));
  const PassListBufs hp = pass_list_bufs(host.data(), l);
  memcpy(gidx, hp.gidx, size_t(hs.count) * 8);
  memcpy(key, hp.key, size_t(hs.count) * 8);
  memcpy(x, hp.x, size_t(hs.count) * d * 8);
  memcpy(resid, hp.resid, size_t(hs.count) * G * 8);
  return 0;
}

// xc [K][d], resid [K][G] (u_g - mu_g at the candidate): flags[c * G + i] != 0 when candidate c
// lifts one of THIS shard's unsafe rows above fmin_i.
int sgp_grid_pass_test(sgp_grid* g, sgp_gp* const* gps, int G, double beta, const double* fmin,
                       int K, const double* xc, const double* resid, int32_t* flags) {
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  if (K <= 0) return 0;
  int32_t* dfl;
  SGP_TRY(expander_many_test(g, host, beta, fmin, K, nullptr, xc, resid, &dfl));
  return sgp_d2h(g->ctx, flags, dfl, size_t(K) * G * 4);
}

// ... and with Lipschitz certificates: the distance test of ALL K gathered candidates (rows xc
// [K][d], upper bounds uc [K][G]: sgp_grid_pass_list with mode | 2) against this shard's unsafe
// rows; flags[c * G + i] != 0: some unsafe row of the shard is in reach of candidate c for every
// GP with a constraint (one flag per candidate, see k_lip_items) -- the ranks OR them.
int sgp_grid_pass_lipschitz_test(sgp_grid* g, int G, const double* fmin, const double* lipschitz,
                                 int K, const double* xc, const double* uc, int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G == g->G, "grid was created for %d GPs, got %d", g->G, G);
  if (K <= 0) return 0;
  if (!any_constraint(fmin, G)) {
    memset(flags, 0, size_t(K) * G * 4);
    return 0;
  }
  double* work;
  int32_t* dfl;
  SGP_TRY(lipschitz_bufs(g, K, &work, &dfl));
  SGP_TRY(launch_lipschitz_many(g, G, fmin, lipschitz, nullptr, K, xc, uc, work, dfl));
  return sgp_d2h(ctx, flags, dfl, size_t(K) * G * 4);
}

// Every candidate of a small grid at once (step_small.hip: k_cand_ops, k_cand_scan):
// flags[c * G + i] != 0 when candidate gidx[c] lifts an unsafe row above fmin_i after the
// rank-1 update by (x_c, u_i(x_c)) -- the test of gp_opt.py:579-606 for m candidates in
// two launches and one round trip.  Grids of at most kStepSmallRows rows, GPs with at most 48
// observations (sgp_grid_step_small_ok).
int sgp_grid_expanders_small(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const int64_t* gidx, int m, int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  if (m <= 0) return 0;
  SGP_CHECK(ctx, step_small_eligible(ctx, host, G, g->N),
            "sgp_grid_expanders_small: %lld rows / a GP with more than 48 observations",
            (long long)g->N);
  for (int c = 0; c < m; ++c)
    SGP_CHECK(ctx, gidx[c] >= g->goff && gidx[c] < g->goff + g->N,
              "candidate %lld is not a row of this grid", (long long)gidx[c]);
  const SmallLayout l = small_layout(m, G, cand_ops_doubles(m, G), false);
  char* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotOperands, l.bytes, &buf));
  const SmallCandBufs sb = small_bufs(buf, l);
  SGP_TRY(sgp_h2d(ctx, sb.rows, gidx, size_t(m) * 8));
  SGP_HIP(ctx, hipMemsetAsync(sb.flags, 0, size_t(m) * G * 4, ctx->stream));
  SGP_TRY(launch_cand_all(g, g->gpdev, host, G, beta, fmin, sb.rows, m, sb.ops, sb.flags));
  return sgp_d2h(ctx, flags, sb.flags, size_t(m) * G * 4);
}

// ... of EVERY candidate of the grid, listed on the device in row order: global rows, widths and
// flags come back in ONE read-back (the candidate mask and the widths do not travel first).
// *count > cap: nothing else is valid (the caller takes the two-step path).
int sgp_grid_expanders_small_all(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                                 const double* fmin, int cap, int* count, int64_t* gidx,
                                 double* width, int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  *count = 0;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SGP_CHECK(ctx, cap >= 1, "cap = %d", cap);
  SGP_CHECK(ctx, step_small_eligible(ctx, host, G, g->N),
            "sgp_grid_expanders_small_all: %lld rows / a GP with more than 48 observations",
            (long long)g->N);
  if (cap > g->N) cap = int(g->N);
  // the list: every candidate, row order (the selection of the big passes with no threshold)
  PassScratch ps;
  SGP_TRY(pass_scratch(g, &ps));
  PassSel hs = {-INFINITY, 0, 0};
  SGP_TRY(sgp_h2d(ctx, ps.sel, &hs, sizeof(hs)));
  SGP_TRY(launch_pass_list(g, 0, INFINITY, -1, ps.sel, ps.list, ps.counts));
  const int* count_dev = &ps.sel->count;
  // [count | rows | widths | flags] for the read-back, the operands behind them
  const SmallLayout l = small_layout(cap, G, cand_ops_doubles(cap, G), true);
  char* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotOperands, l.bytes, &buf));
  const SmallCandBufs sb = small_bufs(buf, l);
  SGP_TRY(launch_small_pack(g, ps.list, count_dev, cap, sb.count, sb.rows, sb.widths, sb.flags));
  SGP_TRY(launch_cand_all(g, g->gpdev, host, G, beta, fmin, sb.rows, cap, sb.ops, sb.flags,
                          count_dev));
  std::vector<char> hb(l.read);
  SGP_TRY(sgp_d2h(ctx, hb.data(), buf, l.read));
  const SmallCandBufs hp = small_bufs(hb.data(), l);
  int64_t n64;
  memcpy(&n64, hp.count, 8);
  *count = int(n64);
  if (n64 > cap) return 0;
  memcpy(gidx, hp.rows, size_t(n64) * 8);
  memcpy(width, hp.widths, size_t(n64) * 8);
  memcpy(flags, hp.flags, size_t(n64) * G * 4);
  return 0;
}
