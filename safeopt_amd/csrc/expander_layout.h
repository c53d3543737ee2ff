// Every scratch block of the expander test, defined once: a struct of byte offsets, the
// constexpr function that computes them from the shape, a function that turns a base pointer
// into typed pointers, and a constexpr check (with static_asserts at the corner shapes) that
// every f64 / i64 region is 8-byte aligned and ends at or in front of the next one, the last
// one inside `bytes`.  Whoever sizes a slot and whoever carves it -- expander_api.hip, api.hip,
// expander.hip, sets.hip -- go through these functions, so the two cannot drift apart.
#pragma once

#include "common.h"

constexpr size_t align8(size_t b) { return (b + 7) & ~size_t(7); }
constexpr size_t exp_groups(int64_t m) { return (size_t(m) + kMaxRhs - 1) / kMaxRhs; }

// n regions at at[i] of len[i] bytes inside `bytes`; f64[i]: the region holds 8-byte values
constexpr bool regions_ok(const size_t* at, const size_t* len, const bool* f64, int n,
                          size_t bytes) {
  for (int i = 0; i < n; ++i) {
    if (f64[i] && at[i] % 8 != 0) return false;
    if (at[i] + len[i] > (i + 1 < n ? at[i + 1] : bytes)) return false;
  }
  return true;
}

// ---- the tail behind a flags array -----------------------------------------------------
// 64 bytes from the first 8-byte boundary behind the flags, zeroed with them where a counter
// is used: what the launches that follow a test leave for the same read-back.
struct FlagTail {
  // sgp_grid_sets_back: value | row (i64) of the arg-max.  pass_result_and_argmax:
  // hits | key | row (i64) of the first hit | value | row (i64) of the arg-max
  double res[5];
  int32_t count;      // ONE candidate: the rows that passed the pre-filter (k_expander_filter)
  int32_t pad[5];
};
static_assert(sizeof(FlagTail) == 64 && offsetof(FlagTail, count) % 4 == 0, "FlagTail");
struct FlagsLayout {
  size_t flags, tail, bytes;
};
constexpr FlagsLayout flags_layout(size_t flag_bytes) {
  FlagsLayout l{};
  l.flags = 0;
  l.tail = align8(flag_bytes);
  l.bytes = l.tail + sizeof(FlagTail);
  return l;
}
inline FlagTail* flag_tail(int32_t* flags, size_t flag_bytes) {
  return reinterpret_cast<FlagTail*>(reinterpret_cast<char*>(flags) +
                                     flags_layout(flag_bytes).tail);
}
constexpr bool flags_layout_ok(size_t flag_bytes) {
  const FlagsLayout l = flags_layout(flag_bytes);
  const size_t at[] = {l.flags, l.tail}, len[] = {flag_bytes, sizeof(FlagTail)};
  const bool f64[] = {false, true};
  return regions_ok(at, len, f64, 2, l.bytes);
}

// ---- kSlotOperands: the operands of up to SGP_TOPK candidates ----------------------------
//   xc[SGP_TOPK][d] | resid[G][16] | delta | inv_s2 | tn2 | flags[SGP_TOPK][G] | tail | W[G][wstride]
// xc | resid are staged together (`staged` bytes), flags and tail are zeroed together
// (`zeroed` bytes).
struct ExpanderLayout {
  size_t xc, resid, delta, inv_s2, tn2, flags, tail, W, bytes;
  size_t staged, zeroed;
};
struct ExpanderBufs {
  double *xc, *resid, *delta, *inv_s2, *tn2, *W;
  int32_t* flags;
  FlagTail* tail;
  int64_t wstride;
  ExpanderLayout l;
};
constexpr ExpanderLayout expander_layout(int d, int G, int64_t wstride) {
  const size_t bv = size_t(G) * kMaxRhs * 8;
  const FlagsLayout f = flags_layout(size_t(SGP_TOPK) * G * 4);
  ExpanderLayout l{};
  l.xc = 0;
  l.resid = l.xc + size_t(SGP_TOPK) * d * 8;
  l.delta = l.resid + bv;
  l.inv_s2 = l.delta + bv;
  l.tn2 = l.inv_s2 + bv;
  l.flags = l.tn2 + bv;
  l.tail = l.flags + f.tail;
  l.W = l.flags + f.bytes;
  l.bytes = l.W + size_t(G) * size_t(wstride) * 8;
  l.staged = l.delta;
  l.zeroed = f.bytes;
  return l;
}
inline ExpanderBufs expander_bufs_at(char* base, const ExpanderLayout& l, int64_t wstride) {
  auto f64 = [base](size_t off) { return reinterpret_cast<double*>(base + off); };
  return ExpanderBufs{f64(l.xc), f64(l.resid), f64(l.delta), f64(l.inv_s2), f64(l.tn2), f64(l.W),
                      reinterpret_cast<int32_t*>(base + l.flags),
                      reinterpret_cast<FlagTail*>(base + l.tail), wstride, l};
}
constexpr bool expander_layout_ok(int d, int G, int64_t wstride) {
  const ExpanderLayout l = expander_layout(d, G, wstride);
  const size_t bv = size_t(G) * kMaxRhs * 8;
  const size_t at[] = {l.xc, l.resid, l.delta, l.inv_s2, l.tn2, l.flags, l.tail, l.W};
  const size_t len[] = {size_t(SGP_TOPK) * d * 8, bv, bv, bv, bv, size_t(SGP_TOPK) * G * 4,
                        sizeof(FlagTail), size_t(G) * size_t(wstride) * 8};
  const bool f64[] = {true, true, true, true, true, false, true, true};
  return regions_ok(at, len, f64, 8, l.bytes) && l.staged == l.resid + bv &&
         l.zeroed == l.W - l.flags;
}

// ---- the blocks of a big pass: m candidates in groups of 16 --------------------------------
// kSlotManyOps, every per-candidate array [group][G][16]:
//   xc[groups 16][d] | resid | delta | inv_s2 | tn2 | stn | svc | agg[group][G][4] |
//   box[group][2][d] | 8 doubles | sagg[super][G][4] | sbox[super][2][d]
// with room for groups / 8 + 1 supergroups; xc | resid are staged together.
// kSlotManyW: W[group][G][wstride].  kSlotManyFlags: flags[groups 16][G] | tail.
struct ManyLayout {
  size_t xc, resid, delta, inv_s2, tn2, stn, svc, agg, box, sagg, sbox, bytes;
  size_t staged;
  size_t w_bytes;
  size_t flag_bytes;
  FlagsLayout fl;
};
struct ManyBufs {
  double *xc, *resid, *delta, *inv_s2, *tn2, *stn, *svc, *agg, *box, *sagg, *sbox;
};
constexpr size_t many_supers_room(size_t ngroups) { return ngroups / 8 + 1; }
constexpr size_t many_flag_bytes(int64_t m, int G) { return exp_groups(m) * kMaxRhs * G * 4; }
constexpr ManyLayout many_layout(int64_t m, int d, int G, int64_t wstride) {
  const size_t ng = exp_groups(m), nv = ng * G * kMaxRhs * 8, ns = many_supers_room(ng);
  ManyLayout l{};
  l.xc = 0;
  l.resid = l.xc + ng * kMaxRhs * d * 8;
  l.delta = l.resid + nv;
  l.inv_s2 = l.delta + nv;
  l.tn2 = l.inv_s2 + nv;
  l.stn = l.tn2 + nv;
  l.svc = l.stn + nv;
  l.agg = l.svc + nv;
  l.box = l.agg + ng * G * 4 * 8;
  l.sagg = l.box + (ng * 2 * d + 8) * 8;
  l.sbox = l.sagg + ns * 4 * G * 8;
  l.bytes = l.sbox + ns * 2 * d * 8;
  l.staged = l.delta;
  l.w_bytes = ng * G * size_t(wstride) * 8;
  l.flag_bytes = many_flag_bytes(m, G);
  l.fl = flags_layout(l.flag_bytes);
  return l;
}
inline ManyBufs many_bufs(double* base, const ManyLayout& l) {
  auto f64 = [base](size_t off) { return base + off / 8; };
  return ManyBufs{f64(l.xc), f64(l.resid), f64(l.delta), f64(l.inv_s2), f64(l.tn2), f64(l.stn),
                  f64(l.svc), f64(l.agg), f64(l.box), f64(l.sagg), f64(l.sbox)};
}
constexpr bool many_layout_ok(int64_t m, int d, int G, int64_t wstride) {
  const ManyLayout l = many_layout(m, d, G, wstride);
  const size_t ng = exp_groups(m), nv = ng * G * kMaxRhs * 8, ns = (ng + 7) / 8;
  const size_t at[] = {l.xc, l.resid, l.delta, l.inv_s2, l.tn2, l.stn, l.svc, l.agg, l.box,
                       l.sagg, l.sbox};
  const size_t len[] = {ng * kMaxRhs * d * 8, nv, nv, nv, nv, nv, nv, ng * G * 4 * 8,
                        ng * 2 * d * 8, ns * 4 * G * 8, ns * 2 * d * 8};
  const bool f64[] = {true, true, true, true, true, true, true, true, true, true, true};
  return regions_ok(at, len, f64, 11, l.bytes) && l.staged == l.resid + nv &&
         size_t(m) * G * 4 <= l.flag_bytes && flags_layout_ok(l.flag_bytes);
}

// ---- the Lipschitz work block (kSlotManyOps; launch_lipschitz_many) ------------------------
//   xc[m][d] | uc[m][G] | box[group][2][d] | rad[group] | 8 doubles;  flags[m][G] | tail
struct LipLayout {
  size_t xc, uc, box, rad, bytes;
  size_t flag_bytes;
  FlagsLayout fl;
};
struct LipBufs {
  double *xc, *uc, *box, *rad;
};
constexpr LipLayout lip_layout(int64_t m, int d, int G) {
  const size_t ng = exp_groups(m);
  LipLayout l{};
  l.xc = 0;
  l.uc = l.xc + size_t(m) * d * 8;
  l.box = l.uc + size_t(m) * G * 8;
  l.rad = l.box + ng * 2 * d * 8;
  l.bytes = l.rad + (ng + 8) * 8;
  l.flag_bytes = size_t(m) * G * 4;
  l.fl = flags_layout(l.flag_bytes);
  return l;
}
inline LipBufs lip_bufs(double* base, const LipLayout& l) {
  return LipBufs{base + l.xc / 8, base + l.uc / 8, base + l.box / 8, base + l.rad / 8};
}
constexpr bool lip_layout_ok(int64_t m, int d, int G) {
  const LipLayout l = lip_layout(m, d, G);
  const size_t ng = exp_groups(m);
  const size_t at[] = {l.xc, l.uc, l.box, l.rad};
  const size_t len[] = {size_t(m) * d * 8, size_t(m) * G * 8, ng * 2 * d * 8, ng * 8};
  const bool f64[] = {true, true, true, true};
  return regions_ok(at, len, f64, 4, l.bytes) && flags_layout_ok(l.flag_bytes);
}

// ---- kSlotHot: the hot segments of a scan over N rows (ints) -------------------------------
// launch_expander_many:  count[G] | wcount[G] | wlist[G][N / 16] | wmask[G][N / 16] | list[G][N]
// launch_lipschitz_many: wcount | wlist[N / 16]
// The counters are the first kHotHead ints, zeroed per launch.
constexpr size_t kHotHead = 64;
static_assert(2 * SGP_MAX_GPS <= kHotHead && SGP_MAX_GPS <= 32, "kSlotHot: room for the counters");
struct HotLayout {
  size_t count, wcount, wlist, wmask, list, bytes;
};
struct HotBufs {
  int *count, *wcount, *wlist;
  unsigned* wmask;
  int* list;
};
constexpr size_t hot_segments(int64_t N) { return size_t((N + 15) >> 4); }
constexpr HotLayout hot_layout(int64_t N, int G) {
  const size_t nw = hot_segments(N);
  HotLayout l{};
  l.count = 0;
  l.wcount = 32 * 4;
  l.wlist = kHotHead * 4;
  l.wmask = l.wlist + size_t(G) * nw * 4;
  l.list = l.wmask + size_t(G) * nw * 4;
  l.bytes = l.list + size_t(G) * size_t(N) * 4;
  return l;
}
inline HotBufs hot_bufs(char* base, const HotLayout& l) {
  auto i32 = [base](size_t off) { return reinterpret_cast<int*>(base + off); };
  return HotBufs{i32(l.count), i32(l.wcount), i32(l.wlist),
                 reinterpret_cast<unsigned*>(base + l.wmask), i32(l.list)};
}
constexpr bool hot_layout_ok(int64_t N, int G) {
  const HotLayout l = hot_layout(N, G);
  const size_t nw = hot_segments(N);
  const size_t at[] = {l.count, l.wcount, l.wlist, l.wmask, l.list};
  const size_t len[] = {size_t(G) * 4, size_t(G) * 4, G * nw * 4, G * nw * 4,
                        size_t(G) * size_t(N) * 4};
  const bool f64[] = {false, false, false, false, false};
  return regions_ok(at, len, f64, 5, l.bytes) && l.wlist == kHotHead * 4;
}
struct LipHotLayout {
  size_t wcount, wlist, bytes;
};
constexpr LipHotLayout lip_hot_layout(int64_t N) {
  return LipHotLayout{0, kHotHead * 4, (kHotHead + hot_segments(N)) * 4};
}

// ---- kSlotPass: the scratch of a big pass ------------------------------------------------
//   list[N] (local rows, padded to 64 B) | hist[kPassBins] | PassSel (256 B) | counts[N / 256 + 2]
struct PassLayout {
  size_t list, hist, sel, counts, bytes;
};
struct PassScratch {
  int* list;
  unsigned* hist;
  PassSel* sel;
  int* counts;
};
constexpr size_t kPassSelRoom = 256;
static_assert(sizeof(PassSel) <= kPassSelRoom && alignof(PassSel) <= 8, "PassSel has 256 bytes");
constexpr PassLayout pass_layout(int64_t N) {
  PassLayout l{};
  l.list = 0;
  l.hist = (size_t(N) * 4 + 63) & ~size_t(63);
  l.sel = l.hist + kPassBins * sizeof(unsigned);
  l.counts = l.sel + kPassSelRoom;
  l.bytes = l.counts + (size_t(N) / 256 + 2) * 4;
  return l;
}
inline PassScratch pass_bufs(char* base, const PassLayout& l) {
  return PassScratch{reinterpret_cast<int*>(base + l.list),
                     reinterpret_cast<unsigned*>(base + l.hist),
                     reinterpret_cast<PassSel*>(base + l.sel),
                     reinterpret_cast<int*>(base + l.counts)};
}
constexpr bool pass_layout_ok(int64_t N) {
  const PassLayout l = pass_layout(N);
  const size_t at[] = {l.list, l.hist, l.sel, l.counts};
  const size_t len[] = {size_t(N) * 4, kPassBins * sizeof(unsigned), kPassSelRoom,
                        (size_t(N) / 256 + 2) * 4};
  const bool f64[] = {false, false, true, false};
  return regions_ok(at, len, f64, 4, l.bytes);
}

// ---- read-back blocks ------------------------------------------------------------------
// sgp_grid_expander_batch (kSlotResult): w[16] | idx[16] (i64) | n | flags[SGP_TOPK][G], one copy
struct BatchReadLayout {
  size_t w, idx, n, flags, bytes;
};
constexpr BatchReadLayout batch_read_layout() { return BatchReadLayout{0, 512, 1024, 1032, 2048}; }
constexpr size_t batch_read_span(int G) {
  return batch_read_layout().flags + size_t(SGP_TOPK) * G * 4;
}
constexpr bool batch_read_layout_ok() {
  const BatchReadLayout l = batch_read_layout();
  const size_t at[] = {l.w, l.idx, l.n, l.flags};
  const size_t len[] = {SGP_TOPK * 8, SGP_TOPK * 8, 4, size_t(SGP_TOPK) * SGP_MAX_GPS * 4};
  const bool f64[] = {true, true, false, false};
  return regions_ok(at, len, f64, 4, l.bytes);
}

// sgp_grid_expanders_small[_all] (kSlotOperands), room for m candidates:
//   listed (_all): count (i64) | rows[m] (i64) | widths[m] | flags[m][G] (padded to 8 B) | operands
//   else:                        rows[m]                   | flags[m][G]                 | operands
// `read` bytes from the start travel back in one copy; operands: cand_ops_doubles(m, G).
struct SmallLayout {
  size_t count, rows, widths, flags, ops, bytes;
  size_t read;
};
struct SmallCandBufs {
  int64_t *count, *rows;
  double* widths;
  int32_t* flags;
  double* ops;
};
constexpr SmallLayout small_layout(int64_t m, int G, size_t ops_doubles, bool listed) {
  SmallLayout l{};
  l.count = 0;
  l.rows = l.count + (listed ? 8 : 0);
  l.widths = l.rows + size_t(m) * 8;
  l.flags = l.widths + (listed ? size_t(m) * 8 : 0);
  l.ops = l.flags + align8(size_t(m) * G * 4);
  l.bytes = l.ops + ops_doubles * 8;
  l.read = l.ops;
  return l;
}
inline SmallCandBufs small_bufs(char* base, const SmallLayout& l) {
  return SmallCandBufs{reinterpret_cast<int64_t*>(base + l.count),
                       reinterpret_cast<int64_t*>(base + l.rows),
                       reinterpret_cast<double*>(base + l.widths),
                       reinterpret_cast<int32_t*>(base + l.flags),
                       reinterpret_cast<double*>(base + l.ops)};
}
constexpr bool small_layout_ok(int64_t m, int G, size_t ops_doubles, bool listed) {
  const SmallLayout l = small_layout(m, G, ops_doubles, listed);
  const size_t at[] = {l.count, l.rows, l.widths, l.flags, l.ops};
  const size_t len[] = {listed ? size_t(8) : 0, size_t(m) * 8, listed ? size_t(m) * 8 : 0,
                        size_t(m) * G * 4, ops_doubles * 8};
  const bool f64[] = {true, true, true, false, true};
  return regions_ok(at, len, f64, 5, l.bytes);
}

// sgp_grid_pass_list (kSlotManyOps): gidx[count] (i64) | key[count] | x[count][d] | resid[count][G]
struct PassListLayout {
  size_t gidx, key, x, resid, bytes;
};
struct PassListBufs {
  int64_t* gidx;
  double *key, *x, *resid;
};
constexpr PassListLayout pass_list_layout(int64_t count, int d, int G) {
  const size_t c = size_t(count) * 8;
  return PassListLayout{0, c, 2 * c, (2 + size_t(d)) * c, (2 + size_t(d) + size_t(G)) * c};
}
inline PassListBufs pass_list_bufs(double* base, const PassListLayout& l) {
  return PassListBufs{reinterpret_cast<int64_t*>(base + l.gidx / 8), base + l.key / 8,
                      base + l.x / 8, base + l.resid / 8};
}

// the corner shapes: 1 candidate, ragged last groups (17, 129 candidates: 2 and 9 groups, the
// supergroup tail groups / 8 + 1), SGP_MAX_GPS, SGP_MAX_D
constexpr bool many_shapes_ok(int64_t m) {
  return many_layout_ok(m, 1, 1, 64) && many_layout_ok(m, SGP_MAX_D, SGP_MAX_GPS, 64 * 64) &&
         many_layout_ok(m, 3, 2, 0) && lip_layout_ok(m, 1, 1) &&
         lip_layout_ok(m, SGP_MAX_D, SGP_MAX_GPS) && lip_layout_ok(m, 3, 3) &&
         small_layout_ok(m, 1, 7, false) && small_layout_ok(m, 3, 7, true) &&
         small_layout_ok(m, SGP_MAX_GPS, 0, true) && hot_layout_ok(m, 1) &&
         hot_layout_ok(m, SGP_MAX_GPS) && pass_layout_ok(m) && flags_layout_ok(size_t(m) * 4) &&
         flags_layout_ok(size_t(m) * 3 * 4);
}
static_assert(many_shapes_ok(1) && many_shapes_ok(16) && many_shapes_ok(17) &&
                  many_shapes_ok(128) && many_shapes_ok(129) && many_shapes_ok(100001),
              "a scratch block of a pass: a region is misaligned or overlaps its neighbour");
static_assert(many_supers_room(exp_groups(129)) == 2 && many_supers_room(exp_groups(128)) == 2 &&
                  many_supers_room(exp_groups(1)) == 1,
              "ManyLayout: room for the supergroup tail");
static_assert(expander_layout_ok(1, 1, 64) && expander_layout_ok(SGP_MAX_D, SGP_MAX_GPS, 4096 * 64) &&
                  expander_layout_ok(3, 3, 0) && batch_read_layout_ok(),
              "ExpanderLayout: a region is misaligned or overlaps its neighbour");

// ---- shared between api.hip and expander_api.hip --------------------------------------------
// The preamble of the grid entry points that take GPs: the device, the G the grid was made
// for, the GPs' descriptors in `host` and, staged, in g->gpdev.  (defined inside api.hip's
// extern "C" block)
extern "C" int grid_gps(sgp_grid* g, sgp_gp* const* gps, int G, GpDev* host);
// expander_api.hip: the kSlotOperands block for the GPs `host`, and the test of m <= SGP_TOPK
// candidates on it (operands + scan), the flags left on the device
int expander_bufs(sgp_grid* g, const GpDev* host, int G, ExpanderBufs* b);
int enqueue_expander(sgp_grid* g, const GpDev* host, const ExpanderBufs& eb, double beta,
                     const double* fmin, int m, const double* xc, const double* mu_c,
                     const double* u_c, double near_frac, const FrontArgs* fold = nullptr);
