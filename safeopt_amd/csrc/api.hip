// C ABI of libsafeopt_hip.so -- see include/safeopt_hip.h for the contract and
// the reference call site each entry point replaces.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <new>

#include <atomic>
#include <chrono>

#include "common.h"
#include "expander_layout.h"
#include "sets_front.h"
#include "small_path.h"

namespace {
std::string g_err;  // errors raised without a context

struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t,
                            ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t,
                            ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
};
Rccl g_rccl;

// RCCL is loaded lazily: single-GPU runs never touch it.
int load_rccl(sgp_ctx* ctx) {
  if (g_rccl.lib) return 0;
  const char* names[] = {"librccl.so.1", "librccl.so",
                         "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* nm : names) {
    g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib) {
    sgp_set_error(ctx, "cannot dlopen librccl.so: %s", dlerror());
    return -3;
  }
#define SYM(field, name)                                                       \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(                     \
      dlsym(g_rccl.lib, name));                                                \
  if (!g_rccl.field) {                                                         \
    sgp_set_error(ctx, "librccl.so lacks %s", name);                           \
    return -3;                                                                 \
  }
  SYM(GetUniqueId, "ncclGetUniqueId")
  SYM(CommInitRank, "ncclCommInitRank")
  SYM(CommDestroy, "ncclCommDestroy")
  SYM(AllReduce, "ncclAllReduce")
  SYM(AllGather, "ncclAllGather")
  SYM(GetErrorString, "ncclGetErrorString")
  SYM(CommCount, "ncclCommCount")
#undef SYM
  return 0;
}

#define SGP_NCCL(ctx, call)                                                    \
  do {                                                                         \
    ncclResult_t r_ = (call);                                                  \
    if (r_ != ncclSuccess) {                                                   \
      sgp_set_error((ctx), "%s:%d %s -> %s", __FILE__, __LINE__, #call,        \
                    g_rccl.GetErrorString(r_));                                \
      return -4;                                                               \
    }                                                                          \
  } while (0)

int fill_kern(sgp_ctx* ctx, KernDesc* kd, int d, int n_parts, const int* kinds,
              const double* variances, const double* inv_ls) {
  SGP_CHECK(ctx, d >= 1 && d <= SGP_MAX_D, "input dimension %d not in 1..%d", d,
            SGP_MAX_D);
  SGP_CHECK(ctx, n_parts >= 1 && n_parts <= SGP_MAX_PARTS,
            "kernel has %d parts, supported 1..%d", n_parts, SGP_MAX_PARTS);
  memset(kd, 0, sizeof(*kd));
  kd->d = d;
  kd->n_parts = n_parts;
  kd->kdiag = 1.0;
  for (int p = 0; p < n_parts; ++p) {
    SGP_CHECK(ctx, kinds[p] >= SGP_RBF && kinds[p] <= SGP_MATERN52,
              "unknown kernel kind %d", kinds[p]);
    kd->kind[p] = kinds[p];
    kd->variance[p] = variances[p];
    kd->kdiag *= variances[p];
    for (int k = 0; k < d; ++k) {
      kd->inv_ls[p][k] = inv_ls[p * d + k];
      const double w = kd->inv_ls[p][k] * kern_unit(kinds[p]);
      kd->wsq[p][k] = w * w;
    }
  }
  for (int k = 0; k < d; ++k)
    kd->scale0[k] = kd->inv_ls[0][k] * kern_unit(kd->kind[0]);
  return 0;
}

}  // namespace

// (common.h: swarm_api.hip collects its GPs the same way)
int collect_gps(sgp_ctx* ctx, sgp_gp* const* gps, int G, int d, GpDev* host) {
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS, "%d GPs, supported 1..%d", G,
            SGP_MAX_GPS);
  for (int g = 0; g < G; ++g) {
    SGP_CHECK(ctx, gps[g] && gps[g]->n > 0, "GP %d has no data", g);
    SGP_CHECK(ctx, gps[g]->factored, "GP %d is not fitted (infeasible hyper-parameters)", g);
    SGP_CHECK(ctx, gps[g]->ctx == ctx,
              "GP %d lives in another context (device %d) than the grid "
              "(device %d): no stream ordering, foreign device pointers",
              g, gps[g]->ctx ? gps[g]->ctx->device : -1, ctx->device);
    SGP_CHECK(ctx, gps[g]->kern.d == d, "GP %d input_dim %d != %d", g,
              gps[g]->kern.d, d);
    host[g] = gps[g]->dev;
    // same inputs, kernel, noise and jitter as the GP in front: same factor (the
    // factorisation is deterministic), only alpha differs
    host[g].share = -1;
    if (ctx->share_factors && g > 0) {
      const sgp_gp *a = gps[g - 1], *b = gps[g];
      if (a != b && a->n == b->n && !a->xhash.empty() && a->xhash.size() == size_t(a->n) &&
          b->xhash.size() == size_t(b->n) && a->xhash.back() == b->xhash.back() &&
          a->prov == b->prov &&
          memcmp(&a->kern, &b->kern, sizeof(KernDesc)) == 0 &&
          a->noise_var == b->noise_var && a->jitter == b->jitter &&
          a->rhost == b->rhost &&        // (noise scales: both none, or the same values)
          // (the hashes only nominate: a collision must not hand one GP the other's
          // |L^-1 k|^2 -- the rows themselves decide, a few KB of memcmp per launch)
          a->xhost.size() == b->xhost.size() &&
          memcmp(a->xhost.data(), b->xhost.data(), a->xhost.size() * sizeof(double)) == 0)
        host[g].share = host[g - 1].share >= 0 ? host[g - 1].share : g - 1;
    }
    // same inputs and kernel as the GP in front, whatever the noise, the jitter and the
    // history (the constraints of a SafeOpt problem: add_new_data_point gives every GP the
    // same x): the same covariances k(X, x), not the same factor.  Set whether factors
    // are shared or not; a GP that shares the factor keeps that mark (riding wins)
    if (host[g].share < 0 && g > 0) {
      const sgp_gp *a = gps[g - 1], *b = gps[g];
      if (a != b && a->n == b->n && !a->xhash.empty() && a->xhash.size() == size_t(a->n) &&
          b->xhash.size() == size_t(b->n) && a->xhash.back() == b->xhash.back() &&
          memcmp(&a->kern, &b->kern, sizeof(KernDesc)) == 0 &&
          a->xhost.size() == b->xhost.size() &&
          memcmp(a->xhost.data(), b->xhost.data(), a->xhost.size() * sizeof(double)) == 0) {
        const int lead = host[g - 1].share >= 0 ? host[g - 1].share
                                                : (host[g - 1].share <= -2 ? gp_cov_lead(host[g - 1]) : g - 1);
        host[g].share = -2 - lead;
      }
    }
  }
  return 0;
}

namespace {
// FNV-1a over the bytes of training rows, chained row by row (sgp_gp::xhash)
uint64_t hash_rows(uint64_t h, const double* rows, size_t count) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(rows);
  for (size_t i = 0; i < count * sizeof(double); ++i) {
    h ^= b[i];
    h *= 1099511628211ull;
  }
  return h;
}
}  // namespace

void sgp_set_error(sgp_ctx* ctx, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  g_err = buf;
}

// SGP_POISON=1 (debugging): every fresh device allocation is filled with 0xFF bytes -- NaN as
// doubles, -1 as integers -- so that a kernel that reads what nobody wrote shows in the results
// instead of depending on what an earlier call left at that address.
int sgp_poison(sgp_ctx* ctx, void* p, size_t bytes) {
  static const bool on = getenv("SGP_POISON") && atoi(getenv("SGP_POISON")) != 0;
  if (!on) return 0;
  SGP_HIP(ctx, hipMemsetAsync(p, 0xFF, bytes, ctx->stream));    // (in stream order: in front of every use)
  return 0;
}

int sgp_reserve(sgp_ctx* ctx, DevBuf* b, size_t bytes) {
  if (bytes <= b->cap && b->p) return 0;
  size_t cap = bytes < 256 ? 256 : bytes;
  if (b->p) {
    // a buffer that grows once usually grows again (one observation per BO
    // iteration): leave room, every growth is a hipMalloc and a stream sync
    if (cap < b->cap + b->cap / 2) cap = b->cap + b->cap / 2;
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SGP_HIP(ctx, hipFree(b->p));
    b->p = nullptr;
    b->cap = 0;
  }
  SGP_HIP(ctx, hipMalloc(&b->p, cap));
  b->cap = cap;
  ++ctx->n_allocs;
  SGP_TRY(sgp_poison(ctx, b->p, cap));
  return 0;
}

void* scratch_slot(sgp_ctx* ctx, ScratchSlot slot, size_t bytes) {
  if (sgp_reserve(ctx, &ctx->scratch[slot], bytes) != 0) return nullptr;
  // SGP_POISON=2: ... and a scratch slot every time it is asked for (what a call finds there
  // from the call before is as good as unwritten), except the kept slots (common.h)
  static const bool every = getenv("SGP_POISON") && atoi(getenv("SGP_POISON")) == 2;
  if (every && !scratch_kept(slot) &&
      hipMemsetAsync(ctx->scratch[slot].p, 0xFF, bytes, ctx->stream) != hipSuccess)
    return nullptr;
  return ctx->scratch[slot].p;
}

// Host <-> device copies.  Small transfers go through the pinned staging
// buffer so the async copy really is asynchronous w.r.t. pageable memory.
int sgp_h2d(sgp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  SGP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice,
                              ctx->stream));
  // the source is a borrowed (pageable) host buffer: complete before return
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int sgp_d2h(sgp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  if (bytes <= ctx->pinned_cap) {
    SGP_HIP(ctx, hipMemcpyAsync(ctx->pinned, src, bytes, hipMemcpyDeviceToHost,
                                ctx->stream));
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(dst, ctx->pinned, bytes);
  } else {
    SGP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost,
                                ctx->stream));
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

extern "C" {

// ---- context ------------------------------------------------------------------
int sgp_device_count(int* n) {
  *n = 0;
  hipError_t e = hipGetDeviceCount(n);
  if (e != hipSuccess) {
    *n = 0;
    sgp_set_error(nullptr, "hipGetDeviceCount -> %s", hipGetErrorString(e));
    (void)hipGetLastError();
    return -1;
  }
  return 0;
}

int sgp_create(int device, sgp_ctx** out) {
  *out = nullptr;
  sgp_ctx* ctx = new (std::nothrow) sgp_ctx();
  if (!ctx) return -1;
  ctx->device = device;
#define CREATE_HIP(call)                                                       \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      sgp_set_error(nullptr, "%s -> %s", #call, hipGetErrorString(e_));        \
      delete ctx;                                                              \
      return -1;                                                               \
    }                                                                          \
  } while (0)
  CREATE_HIP(hipSetDevice(device));
  CREATE_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  ctx->pinned_cap = 1 << 16;
  CREATE_HIP(hipHostMalloc(&ctx->pinned, ctx->pinned_cap, hipHostMallocDefault));
  CREATE_HIP(hipEventCreate(&ctx->ev0));
  CREATE_HIP(hipEventCreate(&ctx->ev1));
  hipDeviceProp_t prop;
  CREATE_HIP(hipGetDeviceProperties(&prop, device));
  ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
#undef CREATE_HIP
  *out = ctx;
  return 0;
}

void sgp_destroy(sgp_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm && g_rccl.CommDestroy)
    g_rccl.CommDestroy(static_cast<ncclComm_t>(ctx->comm));
  for (auto& b : ctx->scratch)
    if (b.p) (void)hipFree(b.p);
  if (ctx->stage_tab.p) (void)hipFree(ctx->stage_tab.p);
  if (ctx->pstage_tab.p) (void)hipFree(ctx->pstage_tab.p);
  if (ctx->pair_split.p) (void)hipFree(ctx->pair_split.p);
  if (ctx->pair_hand.p) (void)hipFree(ctx->pair_hand.p);
  if (ctx->pair_post.p) (void)hipFree(ctx->pair_post.p);
  for (auto e : ctx->prof_events) (void)hipEventDestroy(e);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->step_host) (void)hipHostFree(ctx->step_host);
  if (ctx->sets_host) (void)hipHostFree(ctx->sets_host);
  if (ctx->fleet_host) (void)hipHostFree(ctx->fleet_host);
  if (ctx->fleet_stage) (void)hipHostFree(ctx->fleet_stage);
  if (ctx->fleet_recs.p) (void)hipFree(ctx->fleet_recs.p);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* sgp_last_error(sgp_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_err.c_str();
}

int sgp_sync(sgp_ctx* ctx) {
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---- GP -----------------------------------------------------------------------
int sgp_gp_create(sgp_ctx* ctx, int d, int n_parts, const int* kinds,
                  const double* variances, const double* inv_ls,
                  double noise_var, sgp_gp** out) {
  *out = nullptr;
  KernDesc kd;
  SGP_TRY(fill_kern(ctx, &kd, d, n_parts, kinds, variances, inv_ls));
  sgp_gp* gp = new (std::nothrow) sgp_gp();
  SGP_CHECK(ctx, gp != nullptr, "out of host memory");
  gp->ctx = ctx;
  static uint64_t next_serial = 1;
  gp->serial = next_serial++;
  gp->kern = kd;
  gp->noise_var = noise_var;
  *out = gp;
  return 0;
}

void sgp_gp_destroy(sgp_gp* gp) {
  if (!gp) return;
  sgp_ctx* ctx = gp->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  DevBuf* bufs[] = {&gp->X, &gp->Y, &gp->Xpad, &gp->Xs, &gp->XA, &gp->alpha, &gp->Apack,
                    &gp->Linv, &gp->Kmat, &gp->work, &gp->tvec, &gp->updw,
                    &gp->upd, &gp->blk, &gp->R};
  for (DevBuf* b : bufs)
    if (b->p) (void)hipFree(b->p);
  delete gp;
}

// Factorise the resident data at gp->kern / gp->noise_var as GPy's util.linalg.jitchol does:
// plain attempt, then jitter = mean(diag)*1e-6, *10 per retry, at most 5 retries.
static int fit_with_jitter(sgp_gp* gp, int* chol_info, double* jitter_used) {
  sgp_ctx* ctx = gp->ctx;
  gp->jitter = 0.0;
  gp->factored = true;
  int info = 0;
  double jitter = 0.0;
  SGP_TRY(jitchol_loop(
      [&](double* dm) {
        *dm = gp->kern.kdiag + gp->noise_var + 1e-8;
        if (!gp->rhost.empty()) {        // mean of the diagonal with noise scales
          double rs = 0.0;
          for (double r : gp->rhost) rs += r;
          *dm = gp->kern.kdiag + (gp->noise_var + 1e-8) * (rs / double(gp->rhost.size()));
        }
        return 0;
      },
      [&](double j, int* i) {
        gp->jitter = j;
        return factor_gp(gp, i);
      },
      &info, &jitter));
  if (chol_info) *chol_info = info;
  if (jitter_used) *jitter_used = gp->jitter;
  if (info != 0) {
    gp->n = 0;
    sgp_set_error(ctx, "not positive definite, even with jitter (pivot %d)",
                  info);
    return info > 0 ? info : -2;
  }
  return 0;
}

// The hyper-parameters of a GP rewritten in place (same d, kinds and number of parts): the
// descriptor with its derived fields, nothing else.  The factor no longer belongs to it:
// the version moves (factor tables, the grid's copy of the descriptor) and the rank-1
// record of the last append is dropped.
static int rewrite_hyper(sgp_gp* gp, const double* variances, const double* inv_ls,
                         double noise_var) {
  sgp_ctx* ctx = gp->ctx;
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, std::isfinite(noise_var), "noise_var is not finite");
  KernDesc kd;
  SGP_TRY(fill_kern(ctx, &kd, gp->kern.d, gp->kern.n_parts, gp->kern.kind, variances, inv_ls));
  gp->kern = kd;
  gp->noise_var = noise_var;
  ++gp->data_version;
  gp->upd_valid = false;
  gp->rem_valid = false;
  gp->blk_valid = false;
  gp->rw_valid = false;
  // (a refit at the current n: the history of appends and removals no longer matters)
  gp->prov = 0x9e3779b97f4a7c15ull ^ uint64_t(gp->n);
  return 0;
}

// The device image of the noise scales follows the host's (a GP without scales has none)
static int sync_scales(sgp_gp* gp) {
  if (gp->rhost.empty()) return 0;
  sgp_ctx* ctx = gp->ctx;
  SGP_TRY(sgp_reserve(ctx, &gp->R, size_t(std::max<int64_t>(gp->ld, gp->n)) * sizeof(double)));
  return sgp_h2d(ctx, gp->R.p, gp->rhost.data(), gp->rhost.size() * sizeof(double));
}

static bool scales_ok(const double* r, int64_t n) {
  for (int64_t i = 0; r && i < n; ++i)
    if (!std::isfinite(r[i]) || !(r[i] > 0.0)) return false;
  return true;
}

// the bits of a scale, folded into the history of a factor (sgp_gp::prov)
static uint64_t scale_bits(double r) {
  uint64_t u;
  memcpy(&u, &r, sizeof(u));
  return u * 0x9e3779b97f4a7c15ull;
}

int sgp_gp_set_data(sgp_gp* gp, const double* X, const double* Y, int64_t n,
                    int* chol_info, double* jitter_used) {
  return sgp_gp_set_data_w(gp, X, Y, nullptr, n, chol_info, jitter_used);
}

int sgp_gp_set_data_w(sgp_gp* gp, const double* X, const double* Y, const double* r, int64_t n,
                      int* chol_info, double* jitter_used) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, n >= 1 && n <= kMaxObservations, "n = %lld training points unsupported",
            (long long)n);
  SGP_CHECK(ctx, scales_ok(r, n), "a noise scale is not finite or not positive");
  const int d = gp->kern.d;
  ++gp->data_version;
  gp->n = n;
  gp->n_pad = int((n + 15) / 16) * 16;
  gp->n_f = int((n + 31) / 32) * 32;
  // row capacity: room for 64+ one-row appends before the next reallocation
  if (gp->ld < gp->n_f) gp->ld = int((n + 64 + 63) / 64) * 64;
  SGP_TRY(sgp_reserve(ctx, &gp->X, size_t(gp->ld) * d * sizeof(double)));
  SGP_TRY(sgp_reserve(ctx, &gp->Y, size_t(gp->ld) * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, gp->X.p, X, size_t(n) * d * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, gp->Y.p, Y, size_t(n) * sizeof(double)));
  gp->xhost.assign(X, X + size_t(n) * d);
  gp->xhash.resize(size_t(n));
  {
    uint64_t h = 14695981039346656037ull;
    for (int64_t i = 0; i < n; ++i) {
      h = hash_rows(h, X + i * d, size_t(d));
      gp->xhash[size_t(i)] = h;
    }
    gp->prov = 0x9e3779b97f4a7c15ull ^ uint64_t(n);
  }
  if (r) gp->rhost.assign(r, r + n);
  else gp->rhost.clear();
  SGP_TRY(sync_scales(gp));
  return fit_with_jitter(gp, chol_info, jitter_used);
}

int sgp_gp_set_hyper(sgp_gp* gp, const double* variances, const double* inv_ls,
                     double noise_var, int* chol_info, double* jitter_used) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(rewrite_hyper(gp, variances, inv_ls, noise_var));
  return fit_with_jitter(gp, chol_info, jitter_used);
}

int sgp_gp_lml(sgp_gp* gp, const double* variances, const double* inv_ls, double noise_var,
               double* out, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(rewrite_hyper(gp, variances, inv_ls, noise_var));
  gp->jitter = 0.0;
  gp->factored = false;          // until the pivot word says otherwise
  const int words = lml_result_words(gp->kern);
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, size_t(words) * sizeof(double), &res));
  const int* info_dev = nullptr;
  int unused = 0;
  SGP_TRY(factor_gp(gp, &unused, &info_dev));
  SGP_TRY(launch_lml(gp, info_dev, res));
  double host[3 + SGP_MAX_PARTS + SGP_MAX_PARTS * SGP_MAX_D];
  SGP_TRY(sgp_d2h(ctx, host, res, size_t(words) * sizeof(double)));
  *info = int(host[words - 1]);
  gp->factored = *info == 0;
  memcpy(out, host, size_t(words - 1) * sizeof(double));
  return 0;
}

int sgp_gp_loo_lml(sgp_gp* gp, const double* variances, const double* inv_ls, double noise_var,
                   double* out, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(rewrite_hyper(gp, variances, inv_ls, noise_var));
  gp->jitter = 0.0;
  gp->factored = false;          // until the info word says otherwise
  const int words = lml_result_words(gp->kern);
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, size_t(words) * sizeof(double), &res));
  const int* info_dev = nullptr;
  int unused = 0;
  SGP_TRY(factor_gp(gp, &unused, &info_dev));
  SGP_TRY(launch_loo_lml(gp, info_dev, res));
  double host[3 + SGP_MAX_PARTS + SGP_MAX_PARTS * SGP_MAX_D];
  SGP_TRY(sgp_d2h(ctx, host, res, size_t(words) * sizeof(double)));
  *info = int(host[words - 1]);
  gp->factored = *info == 0;
  memcpy(out, host, size_t(words - 1) * sizeof(double));
  return 0;
}

int sgp_gp_loo(sgp_gp* gp, double* mean, double* var, double* sum_log_pred, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  const double* dev = nullptr;
  int np = 0;
  SGP_TRY(launch_loo(gp, &dev, &np));
  std::vector<double> host(size_t(2) * np + 2);
  SGP_TRY(sgp_d2h(ctx, host.data(), dev, host.size() * sizeof(double)));
  *info = int(host[size_t(2) * np + 1]);
  if (*info != 0) return 0;
  const size_t n = size_t(gp->n);
  memcpy(mean, host.data(), n * sizeof(double));
  memcpy(var, host.data() + np, n * sizeof(double));
  *sum_log_pred = host[size_t(2) * np];
  return 0;
}

int sgp_gp_append(sgp_gp* gp, const double* x, double y, int* info) {
  return sgp_gp_append_w(gp, x, y, nullptr, info);
}

int sgp_gp_append_w(sgp_gp* gp, const double* x, double y, const double* r, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, scales_ok(r, 1), "the noise scale is not finite or not positive");
  *info = -1;
  if (gp->n + 1 > gp->ld) return 0;  // no room: caller refits with set_data
  const int d = gp->kern.d;
  double* X = static_cast<double*>(gp->X.p);
  double* Y = static_cast<double*>(gp->Y.p);
  SGP_TRY(sgp_h2d(ctx, X + size_t(gp->n) * d, x, size_t(d) * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, Y + gp->n, &y, sizeof(double)));
  const int64_t n0 = gp->n;
  ++gp->data_version;
  SGP_TRY(append_gp(gp, y, info, r ? *r : 1.0));
  if (gp->n == n0 + 1) {
    if (r || !gp->rhost.empty()) {
      gp->rhost.resize(size_t(n0), 1.0);
      gp->rhost.push_back(r ? *r : 1.0);
      SGP_TRY(sync_scales(gp));
    }
    gp->xhost.resize(size_t(n0) * d);
    gp->xhost.insert(gp->xhost.end(), x, x + d);
    gp->xhash.resize(size_t(n0));
    gp->xhash.push_back(hash_rows(n0 > 0 ? gp->xhash.back() : 14695981039346656037ull, x,
                                  size_t(d)));
    gp->prov = gp->prov * 1099511628211ull + 2;
    if (r) gp->prov ^= scale_bits(*r);
  }
  return 0;
}

int sgp_gp_append_block(sgp_gp* gp, const double* X, const double* y, int b, int* info) {
  return sgp_gp_append_block_w(gp, X, y, nullptr, b, info);
}

int sgp_gp_append_block_w(sgp_gp* gp, const double* X, const double* y, const double* rs, int b,
                          int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, b >= 1 && b <= SGP_MAX_BLOCK, "a block of %d observations (1..%d)", b,
            SGP_MAX_BLOCK);
  SGP_CHECK(ctx, scales_ok(rs, b), "a noise scale is not finite or not positive");
  *info = -1;
  if (gp->n + b > gp->ld) return 0;  // no room: caller refits with set_data
  const int d = gp->kern.d;
  const int64_t n0 = gp->n;
  double* Xd = static_cast<double*>(gp->X.p);
  double* Yd = static_cast<double*>(gp->Y.p);
  SGP_TRY(sgp_h2d(ctx, Xd + size_t(n0) * d, X, size_t(b) * d * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, Yd + n0, y, size_t(b) * sizeof(double)));
  SGP_TRY(append_block_gp(gp, b, info, rs));
  if (gp->n != n0 + b) return 0;               // a pivot is not positive: the GP is as it was
  // the books of b one-row appends: equal histories keep a shared factor shared
  gp->data_version += uint64_t(b);
  gp->xhost.resize(size_t(n0) * d);
  gp->xhost.insert(gp->xhost.end(), X, X + size_t(b) * d);
  gp->xhash.resize(size_t(n0));
  for (int r = 0; r < b; ++r) {
    gp->xhash.push_back(hash_rows(gp->xhash.empty() ? 14695981039346656037ull : gp->xhash.back(),
                                  X + size_t(r) * d, size_t(d)));
    gp->prov = gp->prov * 1099511628211ull + 2;
    if (rs) gp->prov ^= scale_bits(rs[r]);
  }
  if (rs || !gp->rhost.empty()) {
    gp->rhost.resize(size_t(n0), 1.0);
    for (int j = 0; j < b; ++j) gp->rhost.push_back(rs ? rs[j] : 1.0);
    SGP_TRY(sync_scales(gp));
  }
  return 0;
}

int sgp_gp_pop(sgp_gp* gp) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 1, "cannot remove the only training point");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  ++gp->data_version;
  SGP_TRY(pop_gp(gp));
  gp->xhost.resize(size_t(gp->n) * gp->kern.d);
  gp->xhash.resize(size_t(gp->n));
  if (!gp->rhost.empty()) gp->rhost.resize(size_t(gp->n));   // (the device image: a prefix)
  gp->prov = gp->prov * 1099511628211ull + 3;
  return 0;
}

int sgp_gp_remove(sgp_gp* gp, int64_t index, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, gp->n > 1, "cannot remove the only training point");
  SGP_CHECK(ctx, index >= 0 && index < gp->n, "row %lld of %lld training points",
            (long long)index, (long long)gp->n);
  *info = -1;
  const int64_t n0 = gp->n;
  SGP_TRY(remove_gp(gp, int(index), info));
  if (gp->n != n0 - 1) return 0;               // pivot not positive: the GP is as it was
  ++gp->data_version;
  const size_t d = size_t(gp->kern.d), i = size_t(index);
  gp->xhost.erase(gp->xhost.begin() + i * d, gp->xhost.begin() + (i + 1) * d);
  gp->xhash.resize(size_t(gp->n));
  uint64_t h = i > 0 ? gp->xhash[i - 1] : 14695981039346656037ull;
  for (size_t r = i; r < size_t(gp->n); ++r) {
    h = hash_rows(h, gp->xhost.data() + r * d, d);
    gp->xhash[r] = h;
  }
  // (the row that left is part of the history: equal removals keep a shared factor shared)
  gp->prov = (gp->prov * 1099511628211ull + 5) ^ (uint64_t(index) * 0x9e3779b97f4a7c15ull);
  if (!gp->rhost.empty()) {
    gp->rhost.erase(gp->rhost.begin() + i);
    SGP_TRY(sync_scales(gp));
  }
  return 0;
}

int sgp_gp_reweigh(sgp_gp* gp, int64_t index, double y_new, double r_new, int* info) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, index >= 0 && index < gp->n, "row %lld of %lld training points",
            (long long)index, (long long)gp->n);
  SGP_CHECK(ctx, std::isfinite(y_new), "y_new is not finite");
  SGP_CHECK(ctx, scales_ok(&r_new, 1), "the noise scale is not finite or not positive");
  *info = -1;
  const size_t i = size_t(index);
  const double r_old = gp->rhost.empty() ? 1.0 : gp->rhost[i];
  const double s = gp->noise_var + 1e-8;
  const double delta = s * r_new - s * r_old;
  SGP_TRY(reweigh_gp(gp, int(index), y_new, delta, info));
  if (*info != 0) return 0;                    // pivot not positive: the GP is as it was
  ++gp->data_version;
  if (r_new != r_old) {
    gp->rhost.resize(size_t(gp->n), 1.0);
    gp->rhost[i] = r_new;
    SGP_TRY(sync_scales(gp));
  }
  // (equal re-weightings keep a shared factor shared)
  gp->prov = (gp->prov * 1099511628211ull + 7) ^ (uint64_t(index) * 0x9e3779b97f4a7c15ull) ^
             scale_bits(r_new);
  return 0;
}

int sgp_gp_get_noise_scale(sgp_gp* gp, double* r_out) {
  sgp_ctx* ctx = gp->ctx;
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  const size_t n = size_t(gp->n);
  if (gp->rhost.empty()) {
    for (size_t i = 0; i < n; ++i) r_out[i] = 1.0;
    return 0;
  }
  // the device image, which is what the kernels read
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  return sgp_d2h(ctx, r_out, gp->R.p, n * sizeof(double));
}

int sgp_gp_predict(sgp_gp* gp, const double* Xnew, int64_t N,
                   int64_t stride_row, int64_t stride_col, double* mean,
                   double* var) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  if (N <= 0) return 0;
  const int d = gp->kern.d;
  // stage the rows through a dense row-major device copy
  double* stage;
  double* pts;
  GpDev* gdev;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, size_t(N) * d * sizeof(double), &stage));
  SGP_TRY(sgp_scratch(ctx, kSlotWork, size_t(N) * (d + 2) * sizeof(double), &pts));
  SGP_TRY(sgp_scratch(ctx, kSlotGpDev, sizeof(GpDev), &gdev));
  if (small_path_pays(gp, N)) {
    // a few points: triangular multi-RHS products instead of one sweep tile
    std::vector<double> tmp(size_t(N) * d);
    for (int64_t r = 0; r < N; ++r)
      for (int k = 0; k < d; ++k)
        tmp[size_t(r) * d + k] = Xnew[r * stride_row + k * stride_col];
    SGP_TRY(sgp_h2d(ctx, stage, tmp.data(), tmp.size() * sizeof(double)));
    double* mvs = pts;                        // [mean N | var N]
    SGP_TRY(sgp_h2d(ctx, gdev, &gp->dev, sizeof(GpDev)));
    SmallBufs sb;
    SGP_TRY(small_reserve(ctx, &gp->dev, 1, int(N), &sb));
    SGP_TRY(posterior_small_all(ctx, gdev, &gp->dev, 1, stage, int(N), sb, mvs, mvs + N));
    SGP_TRY(sgp_d2h(ctx, mean, mvs, size_t(N) * sizeof(double)));
    return sgp_d2h(ctx, var, mvs + N, size_t(N) * sizeof(double));
  }
  if (stride_col == 1 && stride_row == d) {
    SGP_TRY(sgp_h2d(ctx, stage, Xnew, size_t(N) * d * sizeof(double)));
    SGP_TRY(launch_import_points(ctx, stage, N, d, d, 1, pts));
  } else if (stride_row == 1 && stride_col == N) {
    SGP_TRY(sgp_h2d(ctx, pts, Xnew, size_t(N) * d * sizeof(double)));
  } else {
    // generic strides: gather on the host into pinned-free scratch
    std::vector<double> tmp(size_t(N) * d);
    for (int64_t r = 0; r < N; ++r)
      for (int k = 0; k < d; ++k)
        tmp[size_t(k) * N + r] = Xnew[r * stride_row + k * stride_col];
    SGP_TRY(sgp_h2d(ctx, pts, tmp.data(), tmp.size() * sizeof(double)));
  }
  SGP_TRY(sgp_h2d(ctx, gdev, &gp->dev, sizeof(GpDev)));
  double* mv = pts + size_t(N) * d;
  SweepPoints sp{pts, N, 1, N};
  ConfOut co{};
  co.Q = nullptr;
  co.mean = mv;
  co.var = mv + N;
  co.S = nullptr;
  co.partial = nullptr;
  co.beta = 0.0;
  SGP_TRY(launch_sweep_conf(ctx, gdev, &gp->dev, 1, d, sp, co));
  SGP_TRY(sgp_d2h(ctx, mean, mv, size_t(N) * sizeof(double)));
  SGP_TRY(sgp_d2h(ctx, var, mv + N, size_t(N) * sizeof(double)));
  return 0;
}

// The checks sgp_gp_predict makes, for the joint calls (which also cap N).
static int joint_ready(sgp_gp* gp, int64_t N) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  SGP_CHECK(ctx, N <= SGP_MAX_JOINT, "N = %lld rows in one joint prediction (SGP_MAX_JOINT = %d)",
            (long long)N, SGP_MAX_JOINT);
  return 0;
}

int sgp_gp_predict_cov(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                       int64_t stride_col, double* mean, double* cov) {
  SGP_TRY(joint_ready(gp, N));
  if (N <= 0 || (!mean && !cov)) return 0;
  return joint_predict_cov(gp, Xnew, N, stride_row, stride_col, mean, cov);
}

int sgp_gp_posterior_draw(sgp_gp* gp, const double* Xnew, int64_t N, int64_t stride_row,
                          int64_t stride_col, const double* Z, int S, double* out, double* mean,
                          int* chol_info, double* jitter_used) {
  SGP_TRY(joint_ready(gp, N));
  SGP_CHECK(gp->ctx, S >= 0, "S = %d samples", S);
  if (N <= 0 || S == 0) return 0;
  return joint_posterior_draw(gp, Xnew, N, stride_row, stride_col, Z, S, out, mean, chol_info,
                              jitter_used);
}

int sgp_gp_get_factor(sgp_gp* gp, double* Linv, double* alpha) {
  sgp_ctx* ctx = gp->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, gp->n > 0, "GP has no data");
  SGP_CHECK(ctx, gp->factored, "GP is not fitted (infeasible hyper-parameters)");
  const int64_t n = gp->n;
  if (Linv) {
    SGP_HIP(ctx, hipMemcpy2DAsync(Linv, n * sizeof(double), gp->Linv.p,
                                  size_t(gp->ld) * sizeof(double),
                                  n * sizeof(double), n, hipMemcpyDeviceToHost,
                                  ctx->stream));
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (alpha) SGP_TRY(sgp_d2h(ctx, alpha, gp->alpha.p, n * sizeof(double)));
  return 0;
}

// A second GP with the state of src.  The buffers that carry state (X, Y, L^-1, alpha, the
// append record) are copied device to device at the pitch of the clone, which has room for
// SGP_MAX_BATCH more rows; the workspaces of a refit (Kmat, work) are left to the first refit;
// the operands of the sweeps come from publish_gp, i.e. from the kernels that formed the
// source's out of the same L^-1, X and alpha.
int sgp_gp_clone(sgp_gp* src, sgp_gp** out) {
  *out = nullptr;
  sgp_ctx* ctx = src->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, src->n > 0, "GP has no data");
  SGP_CHECK(ctx, src->factored, "GP is not fitted (infeasible hyper-parameters)");
  sgp_gp* gp = nullptr;
  {
    int kinds[SGP_MAX_PARTS];
    double variances[SGP_MAX_PARTS], inv_ls[SGP_MAX_PARTS * SGP_MAX_D];
    const KernDesc& k = src->kern;
    for (int p = 0; p < k.n_parts; ++p) {
      kinds[p] = k.kind[p];
      variances[p] = k.variance[p];
      for (int a = 0; a < k.d; ++a) inv_ls[p * k.d + a] = k.inv_ls[p][a];
    }
    SGP_TRY(sgp_gp_create(ctx, k.d, k.n_parts, kinds, variances, inv_ls, src->noise_var, &gp));
  }
  gp->kern = src->kern;              // (the very bytes: collect_gps compares descriptors)
  gp->jitter = src->jitter;
  gp->n = src->n;
  gp->n_pad = src->n_pad;
  gp->n_f = src->n_f;
  gp->data_version = src->data_version;
  gp->xhost = src->xhost;
  gp->xhash = src->xhash;
  gp->prov = src->prov;
  gp->upd_valid = src->upd_valid;
  gp->rem_valid = src->rem_valid;
  gp->rw_valid = src->rw_valid;
  gp->rhost = src->rhost;
  gp->factored = true;
  const int d = src->kern.d, ld0 = src->ld;
  const int ld = std::max(ld0, int((src->n + SGP_MAX_BATCH + 63) / 64) * 64);
  gp->ld = ld;
  auto fail = [&](int rc) {
    sgp_gp_destroy(gp);
    return rc;
  };
  struct {
    DevBuf* dst;
    const DevBuf* from;
    size_t bytes, copy;
  } bufs[] = {
      {&gp->X, &src->X, size_t(ld) * d * 8, size_t(ld0) * d * 8},
      {&gp->Y, &src->Y, size_t(ld) * 8, size_t(ld0) * 8},
      {&gp->alpha, &src->alpha, size_t(ld + 16) * 8, size_t(ld0 + 16) * 8},
      {&gp->updw, &src->updw, size_t(ld + 16) * 8, size_t(ld0 + 16) * 8},
      {&gp->upd, &src->upd, size_t(SGP_MAX_D + 2) * 8, size_t(SGP_MAX_D + 2) * 8},
      {&gp->tvec, nullptr, size_t(ld) * 8 + 64, 0},
      {&gp->Linv, nullptr, size_t(ld) * ld * 8, 0}};
  for (auto& b : bufs) {
    if (sgp_reserve(ctx, b.dst, b.bytes) != 0) return fail(-1);
    if (b.copy && hipMemcpyAsync(b.dst->p, b.from->p, b.copy, hipMemcpyDeviceToDevice,
                                 ctx->stream) != hipSuccess) {
      sgp_set_error(ctx, "sgp_gp_clone: device copy failed");
      return fail(-1);
    }
  }
  // L^-1: zero above the diagonal and behind the data at the new pitch, as factor_gp leaves it
  if (hipMemsetAsync(gp->Linv.p, 0, size_t(ld) * ld * 8, ctx->stream) != hipSuccess ||
      hipMemcpy2DAsync(gp->Linv.p, size_t(ld) * 8, src->Linv.p, size_t(ld0) * 8,
                       size_t(ld0) * 8, size_t(ld0), hipMemcpyDeviceToDevice,
                       ctx->stream) != hipSuccess) {
    sgp_set_error(ctx, "sgp_gp_clone: device copy of L^-1 failed");
    return fail(-1);
  }
  if (int rc = sync_scales(gp)) return fail(rc);
  if (int rc = publish_gp(gp)) return fail(rc);
  *out = gp;
  return 0;
}

int sgp_kern_K(sgp_ctx* ctx, int d, int n_parts, const int* kinds,
               const double* variances, const double* inv_ls, const double* X1,
               int64_t n1, const double* X2, int64_t n2, double* out) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  KernDesc kd;
  SGP_TRY(fill_kern(ctx, &kd, d, n_parts, kinds, variances, inv_ls));
  if (n1 <= 0 || n2 <= 0) return 0;
  const size_t b1 = size_t(n1) * d * sizeof(double);
  const size_t b2 = size_t(n2) * d * sizeof(double);
  const size_t bo = size_t(n1) * n2 * sizeof(double);
  double* x1;
  double* o;
  SGP_TRY(sgp_scratch(ctx, kSlotStage, b1 + b2, &x1));
  SGP_TRY(sgp_scratch(ctx, kSlotWork, bo, &o));
  double* x2 = x1 + size_t(n1) * d;
  SGP_TRY(sgp_h2d(ctx, x1, X1, b1));
  SGP_TRY(sgp_h2d(ctx, x2, X2, b2));
  SGP_TRY(launch_kernel_matrix(ctx, kd, x1, n1, x2, n2, o, n2, 0, 0.0,
                               std::numeric_limits<int64_t>::max()));
  SGP_TRY(sgp_d2h(ctx, out, o, bo));
  return 0;
}

// ---- grid ---------------------------------------------------------------------
int sgp_grid_create(sgp_ctx* ctx, const double* base, int64_t N, int d,
                    int64_t stride_row_B, int64_t stride_col_B, int G,
                    int64_t global_offset, sgp_grid** out) {
  *out = nullptr;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, N >= 1, "empty grid");
  SGP_CHECK(ctx, d >= 1 && d <= SGP_MAX_D, "input dimension %d not in 1..%d", d,
            SGP_MAX_D);
  SGP_CHECK(ctx, G >= 1 && G <= SGP_MAX_GPS, "%d GPs, supported 1..%d", G,
            SGP_MAX_GPS);
  SGP_CHECK(ctx, stride_row_B % 8 == 0 && stride_col_B % 8 == 0,
            "grid strides must be multiples of 8 bytes");
  sgp_grid* g = new (std::nothrow) sgp_grid();
  SGP_CHECK(ctx, g != nullptr, "out of host memory");
  g->ctx = ctx;
  g->N = N;
  g->d = d;
  g->G = G;
  g->goff = global_offset;
  const size_t nd = size_t(N) * sizeof(double);
  g->partial_cap = N / 16 + 32 + 2048;   // (+ the split launches of sweep_pair.hip)
  struct {
    void** p;
    size_t bytes;
  } allocs[] = {{(void**)&g->pts, nd * d},      {(void**)&g->Q, nd * 2 * G},
                {(void**)&g->mean, nd * G},     {(void**)&g->var, nd * G},
                {(void**)&g->S, size_t(N)},     {(void**)&g->M, size_t(N)},
                {(void**)&g->Gm, size_t(N)},    {(void**)&g->cand, size_t(N)},
                {(void**)&g->w, nd},
                {(void**)&g->partial, size_t(g->partial_cap) * sizeof(double)},
                {(void**)&g->gpdev, sizeof(GpDev) * SGP_MAX_GPS},
                {(void**)&g->scal, 64}};
  for (auto& a : allocs) {
    hipError_t e = hipMalloc(a.p, a.bytes);
    if (e != hipSuccess) {
      sgp_set_error(ctx, "hipMalloc(%zu) -> %s", a.bytes, hipGetErrorString(e));
      sgp_grid_destroy(g);
      return -1;
    }
    ++ctx->n_allocs;
    SGP_TRY(sgp_poison(ctx, *a.p, a.bytes));
  }
  SGP_HIP(ctx, hipMemsetAsync(g->S, 0, N, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(g->M, 0, N, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(g->Gm, 0, N, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(g->cand, 0, N, ctx->stream));
  // defined contents before the first sweep (zero mean, zero variance, Q = 0)
  SGP_HIP(ctx, hipMemsetAsync(g->mean, 0, nd * G, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(g->var, 0, nd * G, ctx->stream));
  SGP_HIP(ctx, hipMemsetAsync(g->Q, 0, nd * 2 * G, ctx->stream));
  // upload the rows; the resident layout is SoA [d][N] (= the F-ordered array
  // linearly_spaced_combinations returns, so the common case is one memcpy)
  const int64_t sr = stride_row_B / 8, sc = stride_col_B / 8;
  if (sr == 1 && sc == N) {
    SGP_TRY(sgp_h2d(ctx, g->pts, base, nd * d));
  } else if (sc == 1 && sr == d) {
    double* stage;
    SGP_TRY(sgp_scratch(ctx, kSlotStage, nd * d, &stage));
    SGP_TRY(sgp_h2d(ctx, stage, base, nd * d));
    SGP_TRY(launch_import_points(ctx, stage, N, d, d, 1, g->pts));
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    std::vector<double> tmp(size_t(N) * d);
    for (int64_t r = 0; r < N; ++r)
      for (int k = 0; k < d; ++k) tmp[size_t(k) * N + r] = base[r * sr + k * sc];
    SGP_TRY(sgp_h2d(ctx, g->pts, tmp.data(), nd * d));
  }
  *out = g;
  return 0;
}

void sgp_grid_destroy(sgp_grid* g) {
  if (!g) return;
  sgp_ctx* ctx = g->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  void* ptrs[] = {g->pts, g->Q,    g->mean, g->var,     g->S,    g->M,
                  g->Gm,  g->cand, g->w,    g->partial, g->gpdev, g->scal};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (g->var_h) (void)hipFree(g->var_h);
  if (g->ax_vals.p) (void)hipFree(g->ax_vals.p);
  for (DevBuf& b : g->sep_tab)
    if (b.p) (void)hipFree(b.p);
  delete g;
}

int sgp_grid_set_context(sgp_grid* g, const double* c, int nc) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, nc >= 0 && nc <= g->d && nc <= SGP_MAX_GPS,
            "bad number of context columns %d", nc);
  if (nc == 0) return 0;
  g->post_valid = false;     // the rows change: mean / var describe the old ones
  if (g->axes_valid) {
    // the context columns are constant columns of the tensor grid: new axis values
    for (int i = 0; i < nc; ++i) {
      const int k = g->d - nc + i;
      if (g->ax_count[k] != 1) {
        g->axes_valid = false;      // (declared otherwise: the declaration is void)
        break;
      }
      g->ax_host[size_t(g->ax_off[k])] = c[i];
    }
    if (g->axes_valid) {
      SGP_TRY(sgp_h2d(ctx, g->ax_vals.p, g->ax_host.data(), g->ax_host.size() * sizeof(double)));
      ++g->ax_version;
    }
  }
  return launch_fill_cols(g, c, nc);
}

// SafeOpt's parameter_set is a tensor grid (linearly_spaced_combinations,
// utilities.py:21-54) followed by constant context columns (gp_opt.py:439-451): global
// row i has column k equal to values_k[(i / stride[k]) % count[k]].  The declaration is
// checked against the resident rows bit for bit; *ok = 1 when it holds (the sweeps
// then take per-axis factor tables for RBF kernels), 0 when not (nothing changes).
int sgp_grid_set_axes(sgp_grid* g, int d, const int64_t* count, const int64_t* stride,
                      const double* values, int* ok) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  *ok = 0;
  g->axes_valid = false;
  SGP_CHECK(ctx, d == g->d, "grid has %d columns, %d axes declared", g->d, d);
  int64_t total = 1, nvals = 0;
  for (int k = 0; k < d; ++k) {
    SGP_CHECK(ctx, count[k] >= 1 && stride[k] >= 1, "axis %d: count %lld, stride %lld", k,
              (long long)count[k], (long long)stride[k]);
    if (count[k] > 1) total *= count[k];
    nvals += count[k];
    if (total >= (int64_t(1) << 31) || count[k] * stride[k] >= (int64_t(1) << 31)) return 0;
  }
  // (32-bit index arithmetic in the sweep)
  if (g->goff + g->N > total || g->goff + g->N >= (int64_t(1) << 31)) return 0;
  g->ax_host.assign(values, values + nvals);
  int off = 0;
  for (int k = 0; k < d; ++k) {
    g->ax_count[k] = uint32_t(count[k]);
    g->ax_stride[k] = uint32_t(stride[k]);
    g->ax_off[k] = off;
    off += int(count[k]);
  }
  SGP_TRY(sgp_reserve(ctx, &g->ax_vals, size_t(nvals) * sizeof(double)));
  SGP_TRY(sgp_h2d(ctx, g->ax_vals.p, g->ax_host.data(), size_t(nvals) * sizeof(double)));
  int* mism;
  SGP_TRY(sgp_scratch(ctx, kSlotPartials, 256, &mism));
  SGP_HIP(ctx, hipMemsetAsync(mism, 0, sizeof(int), ctx->stream));
  SGP_TRY(launch_verify_axes(g, mism));
  int bad = 0;
  SGP_TRY(sgp_d2h(ctx, &bad, mism, sizeof(int)));
  if (bad != 0) return 0;
  // the strides must chain: sorted by stride, each is the product of the counts below
  {
    int ord[SGP_MAX_D], na = 0;
    for (int k = 0; k < d; ++k)
      if (count[k] > 1) ord[na++] = k;
    std::sort(ord, ord + na, [&](int a, int b) { return stride[a] < stride[b]; });
    int64_t expect = 1;
    for (int i = 0; i < na; ++i) {
      if (stride[ord[i]] != expect) return 0;
      expect *= count[ord[i]];
    }
  }
  g->axes_valid = true;
  ++g->ax_version;
  *ok = 1;
  return 0;
}

// The tensor-grid description of a sweep over grid g with the GPs of `host`, or
// nullptr when the grid is not one / a kernel is not a product of RBF parts / the
// switch is off.  Builds (or reuses) the factor tables of every GP.
static const SepLaunch* sep_launch(sgp_grid* g, sgp_gp* const* gps, const GpDev* host, int G,
                                   SepLaunch* sl) {
  sgp_ctx* ctx = g->ctx;
  static const bool off = getenv("SGP_NO_SEP") != nullptr;
  if (off || !g->axes_valid || (ctx->sweep_choice & 8)) return nullptr;
  for (int i = 0; i < G; ++i)
    for (int p = 0; p < host[i].kern.n_parts; ++p)
      if (host[i].kern.kind[p] != SGP_RBF) return nullptr;
  int cols[SGP_MAX_D], na = 0;
  for (int k = 0; k < g->d; ++k)
    if (g->ax_count[k] > 1) cols[na++] = k;
  if (na < 1 || na > 3) return nullptr;      // (4 axes: evaluated, launch_posterior)
  // (GPs with few observations are swept by the VALU kernel, which evaluates: no tables to
  // build or refresh at every append)
  if (tiny_sweep_wanted(ctx, host, G, g->N, /*rows_sharded=*/true)) return nullptr;
  // A table is nblk x count x 128 bytes per axis -- with ONE long axis that is the whole
  // n_pad x N covariance matrix (a 1-D grid of 1e6 points, n = 544: 4.3 GB) -- and the sweeps
  // address it with 32-bit offsets.  Beyond a budget that keeps tables an L2 / Infinity-Cache
  // affair (and far below the 4 GB where the offsets would wrap) the covariances are
  // evaluated instead.
  constexpr size_t kSepBudgetBytes = size_t(256) << 20;       // per GP, all axes
  // The paired kernel (factors of more than 256 rows) streams 2-33 MB of packed factor per
  // GP through the 4-MB L2 of an XCD once per tile: tables that do not fit NEXT to that
  // stream are evicted between two uses of a line and every read becomes a fabric request
  // (config 4: 3 x 1.6 MB of tables, 43 GB per 8e6-row launch against 3.6 GB evaluated --
  // 126 x the algorithmic bytes for 2-3 % of time; profiles/r05/ab_tables.txt).  There the
  // tables are used only while all of them fit half an L2 (SGP_SEP_PAIR=1: always).
  static const bool pair_always = getenv("SGP_SEP_PAIR") && atoi(getenv("SGP_SEP_PAIR")) == 1;
  const bool paired = pair_sweep_wanted(ctx, host, G);
  size_t all_bytes = 0;
  for (int i = 0; i < G; ++i) {
    size_t bytes = 0;
    for (int a = 0; a < na; ++a)
      bytes += sep_table_doubles(host[i], g->ax_count[cols[a]]) * sizeof(double);
    if (bytes > kSepBudgetBytes) return nullptr;
    if (host[i].share < 0) all_bytes += bytes;
  }
  if (paired && !pair_always && all_bytes > (size_t(2) << 20)) return nullptr;
  std::sort(cols, cols + na, [&](int a, int b) { return g->ax_stride[a] < g->ax_stride[b]; });
  sl->naxes = na;
  sl->goff = g->goff;
  for (int a = 0; a < na; ++a) sl->count[a] = g->ax_count[cols[a]];
  for (int i = 0; i < G; ++i) {
    // (a follower of a shared factor has its leader's inputs and kernel: same tables)
    const int src = host[i].share >= 0 ? host[i].share : i;
    if (src != i) {
      for (int a = 0; a < na; ++a) sl->tab[i][a] = sl->tab[src][a];
      continue;
    }
    size_t need = 0, offa[4];
    for (int a = 0; a < na; ++a) {
      offa[a] = need;
      need += sep_table_doubles(host[i], sl->count[a]);
    }
    const uint64_t key[3] = {gps[i]->serial, gps[i]->data_version, g->ax_version};
    const bool fresh = g->sep_tab[i].p && g->sep_tab[i].cap >= need * sizeof(double) &&
                       memcmp(g->sep_key[i], key, sizeof(key)) == 0;
    // (room for the appends to come: a growing table must not reallocate every step)
    if (!g->sep_tab[i].p || g->sep_tab[i].cap < need * sizeof(double))
      if (sgp_reserve(ctx, &g->sep_tab[i], (need + need / 4) * sizeof(double)) != 0)
        return nullptr;
    double* out[4];
    for (int a = 0; a < na; ++a) {
      out[a] = static_cast<double*>(g->sep_tab[i].p) + offa[a];
      sl->tab[i][a] = out[a];
    }
    if (!fresh) {
      if (launch_sep_tables(ctx, host[i], g->d, g->ax_count,
                            static_cast<const double*>(g->ax_vals.p), g->ax_off, na, cols,
                            out) != 0)
        return nullptr;
      memcpy(g->sep_key[i], key, sizeof(key));
    }
  }
  return sl;
}

// max l0 over S ends up in g->scal[0]; out2 == nullptr defers the read-back
// (sgp_grid_sets_fused picks the value up on the device and reports it).
static int finish_safe_partials(sgp_grid* g, int nblocks, double* out2) {
  sgp_ctx* ctx = g->ctx;
  g->l0_pending = 0;
  if (!out2 && nblocks <= 4096) {
    // no read-back: the consumer (sgp_grid_sets_fused) folds the partials
    // itself; anything else that needs scal[0] calls settle_max_l first
    g->l0_pending = nblocks;
    return 0;
  }
  SGP_TRY(launch_reduce_max(ctx, g->partial, nblocks, g->scal));
  if (!out2) return 0;
  double m = 0.0;
  SGP_TRY(sgp_d2h(ctx, &m, g->scal, sizeof(double)));
  out2[0] = m;
  out2[1] = (m > -INFINITY) ? 1.0 : 0.0;
  return 0;
}

// scal[0] = max l0[S] when a deferred confidence pass left it as partials
static int settle_max_l(sgp_grid* g) {
  if (g->l0_pending > 0) {
    SGP_TRY(launch_reduce_max(g->ctx, g->partial, g->l0_pending, g->scal));
    g->l0_pending = 0;
  }
  return 0;
}

// GP descriptors -> g->gpdev through a fixed slot of the pinned staging block
// (no stream sync: the slot always holds the descriptors of this very call or
// of an identical earlier one that may still be in flight).
static int stage_gpdev(sgp_grid* g, const GpDev* host, int G) {
  sgp_ctx* ctx = g->ctx;
  // (the set passes of a step follow its confidence pass with the same GPs)
  if (G == g->gpdev_count && memcmp(g->gpdev_host, host, sizeof(GpDev) * G) == 0)
    return 0;
  memcpy(g->gpdev_host, host, sizeof(GpDev) * G);
  g->gpdev_count = G;
  char* slot = static_cast<char*>(ctx->pinned) + ctx->pinned_cap -
               sizeof(GpDev) * SGP_MAX_GPS;
  memcpy(slot, host, sizeof(GpDev) * G);
  SGP_HIP(ctx, hipMemcpyAsync(g->gpdev, slot, sizeof(GpDev) * G,
                              hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// The preamble of the grid entry points that take GPs: the device, the G the grid was made
// for, the GPs' descriptors in `host` and, staged, in g->gpdev.  (declared in expander_layout.h)
int grid_gps(sgp_grid* g, sgp_gp* const* gps, int G, GpDev* host) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G == g->G, "grid was created for %d GPs, got %d", g->G, G);
  SGP_TRY(collect_gps(ctx, gps, G, g->d, host));
  return stage_gpdev(g, host, G);
}

// `words` doubles of zeroed host memory the device writes directly (pinned, mapped,
// coherent): *host, and *dev as the device sees it
static int mapped_block(sgp_ctx* ctx, size_t words, double** host, double** dev) {
  void* h = nullptr;
  SGP_HIP(ctx, hipHostMalloc(&h, words * 8, hipHostMallocMapped | hipHostMallocCoherent));
  memset(h, 0, words * 8);
  void* dv = nullptr;
  SGP_HIP(ctx, hipHostGetDevicePointer(&dv, h, 0));
  *host = static_cast<double*>(h);
  *dev = static_cast<double*>(dv);
  return 0;
}

int sgp_grid_confidence(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, double* out2) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SweepPoints sp{g->pts, g->N, 1, g->N};
  ConfOut co{};
  co.Q = g->Q;
  co.mean = g->mean;
  co.var = g->var;
  co.S = g->S;
  co.partial = g->partial;
  co.beta = beta;
  for (int i = 0; i < SGP_MAX_GPS; ++i) co.fmin[i] = (i < G) ? fmin[i] : -INFINITY;
  SepLaunch sl;
  SGP_TRY(launch_sweep_conf(ctx, g->gpdev, host, G, g->d, sp, co,
                            sep_launch(g, gps, host, G, &sl), /*rows_sharded=*/true));
  g->post_valid = true;
  return finish_safe_partials(g, ctx->sweep_partials, out2);
}

int sgp_grid_posterior(sgp_grid* g, sgp_gp* const* gps, int G) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SweepPoints sp{g->pts, g->N, 1, g->N};
  ConfOut co{};            // Q, S, partial stay null: mean / var only
  co.mean = g->mean;
  co.var = g->var;
  co.beta = 0.0;
  for (int i = 0; i < SGP_MAX_GPS; ++i) co.fmin[i] = -INFINITY;
  SepLaunch sl;
  SGP_TRY(launch_sweep_conf(ctx, g->gpdev, host, G, g->d, sp, co,
                            sep_launch(g, gps, host, G, &sl), /*rows_sharded=*/true));
  g->post_valid = true;
  return 0;
}

// sgp_grid_rank1_update / sgp_grid_rank1_remove / sgp_grid_rank1_reweigh: the flagged GPs
// carry the record of an append / of a removal / of a re-weighting (the three flags exclude
// each other: every entry point refuses the other two's records)
static int rank1_refresh(sgp_grid* g, sgp_gp* const* gps, int G, const int* which, double beta,
                         const double* fmin, double* out2, int kind) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  Rank1Args ra{};
  for (int i = 0; i < SGP_MAX_GPS; ++i) {
    ra.fmin[i] = (i < G) ? fmin[i] : -INFINITY;
    ra.which[i] = (i < G) ? which[i] : 0;
    if (i < G && which[i]) {
      if (kind == kRank1Remove)
        SGP_CHECK(ctx, gps[i]->rem_valid,
                  "GP %d has no removal record for a rank-1 update", i);
      else if (kind == kRank1Reweigh)
        SGP_CHECK(ctx, gps[i]->rw_valid,
                  "GP %d has no reweigh record for a rank-1 update", i);
      else
        SGP_CHECK(ctx, gps[i]->upd_valid,
                  "GP %d has no append record for a rank-1 update", i);
    }
  }
  ra.Q = g->Q;
  ra.mean = g->mean;
  ra.var = g->var;
  ra.S = g->S;
  ra.partial = g->partial;
  ra.beta = beta;
  SweepPoints sp{g->pts, g->N, 1, g->N};
  // (post_valid stays as it is: the refresh keeps a swept posterior current, it makes none)
  SGP_TRY(launch_rank1(ctx, g->gpdev, G, g->d, sp, ra, kind));
  return finish_safe_partials(g, rank1_num_blocks(g->N), out2);
}

int sgp_grid_rank1_update(sgp_grid* g, sgp_gp* const* gps, int G,
                          const int* which, double beta, const double* fmin,
                          double* out2) {
  return rank1_refresh(g, gps, G, which, beta, fmin, out2, kRank1Append);
}

int sgp_grid_rank1_remove(sgp_grid* g, sgp_gp* const* gps, int G, const int* which,
                          double beta, const double* fmin, double* out2) {
  return rank1_refresh(g, gps, G, which, beta, fmin, out2, kRank1Remove);
}

int sgp_grid_rank1_reweigh(sgp_grid* g, sgp_gp* const* gps, int G, const int* which,
                           double beta, const double* fmin, double* out2) {
  return rank1_refresh(g, gps, G, which, beta, fmin, out2, kRank1Reweigh);
}

int sgp_grid_rankb_update(sgp_grid* g, sgp_gp* const* gps, int G, const int* which,
                          double beta, const double* fmin, double* out2) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  RankbArgs rb{};
  Rank1Args& ra = rb.r;
  for (int i = 0; i < SGP_MAX_GPS; ++i) {
    ra.fmin[i] = (i < G) ? fmin[i] : -INFINITY;
    ra.which[i] = (i < G) ? which[i] : 0;
    rb.blk[i] = nullptr;
    if (i < G && which[i]) {
      SGP_CHECK(ctx, gps[i]->blk_valid && gps[i]->blk.p,
                "GP %d has no block record for a rank-b update", i);
      rb.blk[i] = static_cast<const double*>(gps[i]->blk.p);
    }
  }
  ra.Q = g->Q;
  ra.mean = g->mean;
  ra.var = g->var;
  ra.S = g->S;
  ra.partial = g->partial;
  ra.beta = beta;
  SweepPoints sp{g->pts, g->N, 1, g->N};
  // (post_valid stays as it is, as in rank1_refresh)
  SGP_TRY(launch_rankb(ctx, g->gpdev, G, g->d, sp, rb));
  return finish_safe_partials(g, rank1_num_blocks(g->N), out2);
}

int sgp_grid_upload_Q(sgp_grid* g, const double* Q, const double* fmin,
                      double* out2) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(sgp_h2d(ctx, g->Q, Q, size_t(g->N) * 2 * g->G * sizeof(double)));
  SGP_TRY(launch_safe_set(g, fmin));
  return finish_safe_partials(g, int((g->N + 255) / 256), out2);
}

int sgp_grid_maximizers(sgp_grid* g, double max_l, double* out) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(launch_maximizers(g, max_l));
  double* red;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, 64, &red));
  SGP_TRY(launch_reduce_max(ctx, g->partial, (g->N + 255) / 256, red));
  return sgp_d2h(ctx, out, red, sizeof(double));
}

int sgp_grid_candidates(sgp_grid* g, double max_var, const double* scaling,
                        const double* thr_beta, int full_sets,
                        int64_t* counts) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  unsigned long long* cd;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, 64, &cd));
  SGP_TRY(launch_candidates(g, max_var, nullptr, scaling, thr_beta, full_sets,
                            cd));
  return sgp_d2h(ctx, counts, cd, 2 * sizeof(int64_t));
}

int sgp_grid_topk(sgp_grid* g, int mode, double cut_w, int64_t cut_idx, int k,
                  double* w_out, int64_t* gidx_out, int* n_out) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, k >= 1 && k <= 64, "k = %d not in 1..64", k);
  char* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, 2048, &res));
  double* wd = reinterpret_cast<double*>(res);
  int64_t* id = reinterpret_cast<int64_t*>(res + 512);
  int* nd = reinterpret_cast<int*>(res + 1024);
  if (mode == 1) cut_w = (cut_idx < 0) ? INFINITY : -double(cut_idx);
  SGP_TRY(launch_topk(g, mode, cut_w, cut_idx, k, wd, id, nd));
  char host[1024 + 8];
  SGP_TRY(sgp_d2h(ctx, host, res, 1024 + 8));
  memcpy(w_out, host, size_t(k) * sizeof(double));
  memcpy(gidx_out, host + 512, size_t(k) * sizeof(int64_t));
  memcpy(n_out, host + 1024, sizeof(int));
  return 0;
}

static int upload_local_idx(sgp_grid* g, const int64_t* gidx, int m,
                            int64_t** dev) {
  sgp_ctx* ctx = g->ctx;
  SGP_CHECK(ctx, m >= 1 && m <= 4096, "m = %d rows out of range", m);
  std::vector<int64_t> li(m);
  for (int j = 0; j < m; ++j) {
    li[j] = gidx[j] - g->goff;
    SGP_CHECK(ctx, li[j] >= 0 && li[j] < g->N,
              "global index %lld is not owned by this shard",
              (long long)gidx[j]);
  }
  int64_t* d;
  SGP_TRY(sgp_scratch(ctx, kSlotSmall, size_t(m) * 8, &d));
  SGP_TRY(sgp_h2d(ctx, d, li.data(), size_t(m) * 8));
  *dev = d;
  return 0;
}

int sgp_grid_gather_rows(sgp_grid* g, const int64_t* gidx, int m, double* x,
                         double* mean, double* var, double* Q) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  int64_t* li = nullptr;
  SGP_TRY(upload_local_idx(g, gidx, m, &li));
  const int d = g->d, G = g->G;
  const size_t per = size_t(d) + 4 * size_t(G);
  double* o;
  SGP_TRY(sgp_scratch(ctx, kSlotOperands, size_t(m) * per * 8, &o));
  double* ox = o;
  double* om = ox + size_t(m) * d;
  double* ov = om + size_t(m) * G;
  double* oq = ov + size_t(m) * G;
  SGP_TRY(launch_gather_rows(g, li, m, ox, om, ov, oq));
  std::vector<double> host(size_t(m) * per);
  SGP_TRY(sgp_d2h(ctx, host.data(), o, host.size() * 8));
  memcpy(x, host.data(), size_t(m) * d * 8);
  memcpy(mean, host.data() + size_t(m) * d, size_t(m) * G * 8);
  memcpy(var, host.data() + size_t(m) * (d + G), size_t(m) * G * 8);
  memcpy(Q, host.data() + size_t(m) * (d + 2 * G), size_t(m) * 2 * G * 8);
  return 0;
}

int sgp_grid_mark_expanders(sgp_grid* g, const int64_t* gidx, int m) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  if (m <= 0) return 0;
  int64_t* li = nullptr;
  SGP_TRY(upload_local_idx(g, gidx, m, &li));
  return launch_mark(g, li, m, 1);
}

int sgp_grid_unmark_expanders(sgp_grid* g, const int64_t* gidx, int m) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  if (m <= 0) return 0;
  int64_t* li = nullptr;
  SGP_TRY(upload_local_idx(g, gidx, m, &li));
  return launch_mark(g, li, m, 0);
}

int sgp_grid_lipschitz_check(sgp_grid* g, int G, const double* fmin,
                             const double* lipschitz, int m, const double* xc,
                             const double* u_c, int32_t* flags) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, G == g->G, "grid was created for %d GPs, got %d", g->G, G);
  SGP_CHECK(ctx, m >= 1 && m <= SGP_TOPK, "m = %d not in 1..%d", m, SGP_TOPK);
  const int d = g->d;
  const size_t bx = size_t(m) * d * 8, bu = size_t(m) * G * 8,
               bf = size_t(m) * G * 4;
  char* buf;
  SGP_TRY(sgp_scratch(ctx, kSlotOperands, bx + bu + bf + 64, &buf));
  double* dx = reinterpret_cast<double*>(buf);
  double* du = reinterpret_cast<double*>(buf + bx);
  int32_t* df = reinterpret_cast<int32_t*>(buf + bx + bu);
  SGP_TRY(sgp_h2d(ctx, dx, xc, bx));
  SGP_TRY(sgp_h2d(ctx, du, u_c, bu));
  SGP_HIP(ctx, hipMemsetAsync(df, 0, bf, ctx->stream));
  SGP_TRY(launch_lipschitz(g, G, fmin, lipschitz, m, dx, du, df));
  return sgp_d2h(ctx, flags, df, bf);
}

int sgp_grid_argmax(sgp_grid* g, int mode, const double* scaling, double* value,
                    int64_t* gidx) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  char* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, 64, &res));
  SGP_TRY(launch_argmax(g, mode, scaling, reinterpret_cast<double*>(res),
                        reinterpret_cast<int64_t*>(res + 8)));
  char host[16];
  SGP_TRY(sgp_d2h(ctx, host, res, 16));
  memcpy(value, host, 8);
  memcpy(gidx, host + 8, 8);
  return 0;
}

// One pick of a hallucinated batch: csrc/batch.hip.  The GPs are clones that carry the append
// record of the pending pick; nothing the real step left on the grid is written.
// batch_checks: what every entry refuses, whether or not its rank takes part in the pick.
static int batch_checks(sgp_ctx* ctx, int mode, int n_picked) {
  SGP_CHECK(ctx, mode == SGP_ARGMAX_MG_WIDTH || mode == SGP_ARGMAX_UCB,
            "sgp_grid_batch_next: mode %d is not SGP_ARGMAX_MG_WIDTH / SGP_ARGMAX_UCB", mode);
  SGP_CHECK(ctx, n_picked >= 0 && n_picked <= SGP_MAX_BATCH,
            "sgp_grid_batch_next: %d rows picked before (SGP_MAX_BATCH = %d)", n_picked,
            SGP_MAX_BATCH);
  return 0;
}

// The shard's pick, enqueued: the row kernel and k_batch_final leave {value, global row} in
// bs->res_v / res_i.  extra: bytes of scratch the caller wants behind the pick's.
static int batch_enqueue(sgp_grid* g, sgp_gp* const* gps, int G, int first, int mode,
                         double beta, const double* scaling, const int64_t* picked,
                         int n_picked, size_t extra, BatchScratch* bs) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SGP_TRY(batch_checks(ctx, mode, n_picked));
  for (int i = 0; i < G; ++i)
    SGP_CHECK(ctx, gps[i]->upd_valid, "GP %d has no append record for a hallucinated downdate",
              i);
  SGP_CHECK(ctx, first || g->var_h, "sgp_grid_batch_next: first = 0 before a first downdate");
  const size_t vbytes = size_t(g->N) * g->G * sizeof(double);
  if (!g->var_h) {
    SGP_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&g->var_h), vbytes));
    ++ctx->n_allocs;
    SGP_TRY(sgp_poison(ctx, g->var_h, vbytes));
  }
  const int nb = batch_num_blocks(g->N);
  void* scr;
  SGP_TRY(sgp_scratch(ctx, kSlotPartials, batch_scratch_bytes(nb) + extra, &scr));
  *bs = batch_scratch(scr, nb);
  BatchArgs ba{};
  ba.mean = g->mean;
  ba.var_in = first ? g->var : g->var_h;
  ba.var_out = g->var_h;
  ba.S = g->S;
  ba.M = g->M;
  ba.Gm = g->Gm;
  ba.mode = mode;
  ba.beta = beta;
  for (int i = 0; i < SGP_MAX_GPS; ++i) ba.scaling[i] = (i < G) ? scaling[i] : 1.0;
  ba.goff = g->goff;
  ba.n_picked = n_picked;
  for (int k = 0; k < n_picked; ++k) ba.picked[k] = picked[k];
  ba.part_v = bs->part_v;
  ba.part_i = bs->part_i;
  SweepPoints sp{g->pts, g->N, 1, g->N};
  return launch_batch_pick(ctx, g->gpdev, G, g->d, sp, ba, bs->res_v, bs->res_i);
}

int sgp_grid_batch_next(sgp_grid* g, sgp_gp* const* gps, int G, int first, int mode,
                        double beta, const double* scaling, const int64_t* picked,
                        int n_picked, double* value, int64_t* gidx) {
  sgp_ctx* ctx = g->ctx;
  BatchScratch bs;
  SGP_TRY(batch_enqueue(g, gps, G, first, mode, beta, scaling, picked, n_picked, 0, &bs));
  char res[16];
  SGP_TRY(sgp_d2h(ctx, res, bs.res_v, 16));
  memcpy(value, res, 8);
  memcpy(gidx, res + 8, 8);
  return 0;
}

// The pick over the shards of all ranks: this rank's record {value, global row, stop} behind
// its own pick (or {-inf, -1, 1} without one), ONE all-gather, k_batch_merge, ONE read-back.
int sgp_grid_batch_next_comm(sgp_grid* g, sgp_gp* const* gps, int G, int first, int mode,
                             double beta, const double* scaling, const int64_t* picked,
                             int n_picked, int stop, double* value, int64_t* gidx,
                             int* stop_any) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  bool comm;
  SGP_TRY(comm_or_single(ctx, &comm));
  stop = stop != 0;
  if (!comm) {
    *stop_any = stop;
    if (!stop)
      return sgp_grid_batch_next(g, gps, G, first, mode, beta, scaling, picked, n_picked,
                                 value, gidx);
    SGP_TRY(batch_checks(ctx, mode, n_picked));
    *value = -INFINITY;
    *gidx = -1;
    return 0;
  }
  const int world = ctx->world;
  const int nb = batch_num_blocks(g->N);
  const size_t extra = batch_comm_scratch_bytes(nb, world) - batch_scratch_bytes(nb);
  BatchScratch bs;
  if (stop) {
    // (no row kernel: var_h stays as it was; the call is still made -- the other ranks wait
    // in the all-gather)
    SGP_TRY(batch_checks(ctx, mode, n_picked));
    void* scr;
    SGP_TRY(sgp_scratch(ctx, kSlotPartials, batch_scratch_bytes(nb) + extra, &scr));
    bs = batch_scratch(scr, nb);
  } else {
    SGP_TRY(batch_enqueue(g, gps, G, first, mode, beta, scaling, picked, n_picked, extra, &bs));
  }
  const BatchCommScratch cs = batch_comm_scratch(bs, world);
  SGP_TRY(launch_batch_stop(ctx, cs.rec, stop));
  SGP_TRY(coll_allgather(ctx, cs.rec, cs.recs, kBatchRecBytes));
  SGP_TRY(launch_batch_merge(ctx, cs.recs, world, cs.merged));
  char res[kBatchRecBytes];
  SGP_TRY(sgp_d2h(ctx, res, cs.merged, kBatchRecBytes));
  int64_t any;
  memcpy(value, res, 8);
  memcpy(gidx, res + 8, 8);
  memcpy(&any, res + 16, 8);
  *stop_any = any != 0;
  return 0;
}

int sgp_grid_upload_mask(sgp_grid* g, int what, const uint8_t* mask) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  uint8_t* dst = what == SGP_S ? g->S : what == SGP_M ? g->M : what == SGP_G ? g->Gm : nullptr;
  SGP_CHECK(ctx, dst, "sgp_grid_upload_mask: selector %d is not SGP_S / SGP_M / SGP_G", what);
  return sgp_h2d(ctx, dst, mask, size_t(g->N));
}

int sgp_grid_download(sgp_grid* g, int what, void* out) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = size_t(g->N), G = size_t(g->G);
  switch (what) {
    case SGP_Q: return sgp_d2h(ctx, out, g->Q, N * 2 * G * 8);
    case SGP_S: return sgp_d2h(ctx, out, g->S, N);
    case SGP_M: return sgp_d2h(ctx, out, g->M, N);
    case SGP_G: return sgp_d2h(ctx, out, g->Gm, N);
    case SGP_MEAN: return sgp_d2h(ctx, out, g->mean, N * G * 8);
    case SGP_VAR: return sgp_d2h(ctx, out, g->var, N * G * 8);
    case SGP_CAND: return sgp_d2h(ctx, out, g->cand, N);     // expander candidates
    case SGP_WIDTH: return sgp_d2h(ctx, out, g->w, N * 8);   // max_i (u_i - l_i)
    case SGP_VAR_H:
      SGP_CHECK(ctx, g->var_h, "no hallucinated variances yet (sgp_grid_batch_next)");
      return sgp_d2h(ctx, out, g->var_h, N * G * 8);
  }
  sgp_set_error(ctx, "unknown array selector %d", what);
  return -2;
}

// The ABI's outputs of a step (null: not asked for) ...
struct StepOut {
  double* out5;
  double* x_top;
  double* mean_top;
  double* q_top;
  int32_t* flags;
  double* value;
  int64_t* gidx;
  double* max_l;
};

// ... from a host copy of its result block (sets_front.h): out5 = { max width, candidates,
// unsafe rows, w_top, global index of the first candidate (-1: the shard / grid has none),
// the candidates that share its width }.
static void unpack_result(const double* h, int d, int G, const StepOut& o) {
  unsigned long long cnt[2];
  int64_t idx;
  int nfound, ntied;
  memcpy(cnt, &h[kResCounts], 16);
  memcpy(&idx, &h[kResTopIdx], 8);
  memcpy(&nfound, &h[kResFound], 4);
  memcpy(&ntied, reinterpret_cast<const char*>(&h[kResFound]) + 4, 4);
  o.out5[0] = h[kResMaxWidth];
  o.out5[1] = double(cnt[0]);
  o.out5[2] = double(cnt[1]);
  o.out5[3] = h[kResTopW];
  o.out5[4] = (nfound > 0) ? double(idx) : -1.0;
  o.out5[5] = double(ntied);
  memcpy(o.x_top, &h[kResX], size_t(d) * 8);
  memcpy(o.mean_top, &h[res_mean(d)], size_t(G) * 8);
  memcpy(o.q_top, &h[res_q(d, G)], size_t(2 * G) * 8);
  if (o.flags) memcpy(o.flags, &h[res_flags(d, G)], size_t(G) * 4);
  if (o.value) *o.value = h[res_value(d, G)];
  if (o.gidx) memcpy(o.gidx, &h[res_index(d, G)], 8);
  if (o.max_l) *o.max_l = h[res_max_l(d, G)];
}
static_assert(res_words(SGP_MAX_D, SGP_MAX_GPS) < kStepResWords, "result block too large");

// ... read back from the device (the first `words` words)
static int read_result(sgp_grid* g, const double* res_dev, int words, const StepOut& o) {
  double h[kStepResWords];
  SGP_TRY(sgp_d2h(g->ctx, h, res_dev, size_t(words) * 8));
  unpack_result(h, g->d, g->G, o);
  return 0;
}

// The first candidate in visiting order behind the max width and counts of a front block:
// w_top, its index, n_found, the ties and its rows
static int front_first(sgp_grid* g, double* res) {
  const int d = g->d, G = g->G;
  SGP_TRY(launch_topk(g, 0, INFINITY, INT64_MAX, 1, res + kResTopW,
                      reinterpret_cast<int64_t*>(res + kResTopIdx),
                      reinterpret_cast<int*>(res + kResFound)));
  // (the fused single-rank pass counts the ties in k_front_final; here nothing
  // else writes that word)
  SGP_TRY(launch_count_ties(g, res + kResTopW, reinterpret_cast<const int*>(res + kResFound),
                            reinterpret_cast<int*>(res + kResFound) + 1));
  return launch_gather_top(g, reinterpret_cast<int64_t*>(res + kResTopIdx), res + kResX,
                           res + res_mean(d), res + res_q(d, G));
}

// Single-rank fast path, front half of compute_sets (gp_opt.py:511-552) with
// ONE stream sync: M, max_var, candidate mask, counts and the first candidate
// in visiting order together with its rows.
int sgp_grid_sets_front(sgp_grid* g, double max_l, int have_max_var,
                        double max_var, const double* scaling,
                        const double* thr_beta, double* out5, double* x_top,
                        double* mean_top, double* q_top) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  const int d = g->d, G = g->G;
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, size_t(res_words(d, G) + 8) * 8, &res));
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(res + kResCounts);
  if (have_max_var) {
    // multi-rank: M is already set (sgp_grid_maximizers) and max_var is the
    // all-reduced value
    SGP_HIP(ctx, hipMemsetAsync(res + kResMaxWidth, 0, 8, ctx->stream));
    SGP_TRY(launch_candidates(g, max_var, nullptr, scaling, thr_beta, 0, counts));
  } else {
    SGP_TRY(launch_maximizers(g, max_l));
    SGP_TRY(launch_reduce_max(ctx, g->partial, (g->N + 255) / 256, res + kResMaxWidth));
    SGP_TRY(launch_candidates(g, 0.0, res + kResMaxWidth, scaling, thr_beta, 0, counts));
  }
  SGP_TRY(front_first(g, res));
  return read_result(g, res, res_front(d, G), {out5, x_top, mean_top, q_top});
}

// ---- the collectives of the N-rank step on DEVICE operands -------------------------
// Two transports behind one table: RCCL on the context's stream (sgp_comm_init: the
// collective is one more operation in the stream, no host round trip), or the caller's
// own collectives on host buffers (sgp_comm_init_host: stream sync + D2H, the callback,
// H2D behind it -- ranks without a GPU each / without xGMI between them, and the way the
// in-stream step is exercised with real foreign data on a one-GPU box).
static bool have_comm(const sgp_ctx* ctx) {
  return ctx->comm != nullptr || ctx->hostcomm.allgather != nullptr;
}
int coll_allreduce_max_f64(sgp_ctx* ctx, double* dev, size_t n) {
  if (ctx->comm) {
    SGP_NCCL(ctx, g_rccl.AllReduce(dev, dev, n, ncclFloat64, ncclMax,
                                   static_cast<ncclComm_t>(ctx->comm), ctx->stream));
    return 0;
  }
  if (!ctx->hostcomm.allreduce_max_f64) return 0;
  std::vector<double> h(n);
  SGP_TRY(sgp_d2h(ctx, h.data(), dev, n * 8));
  SGP_CHECK(ctx, ctx->hostcomm.allreduce_max_f64(ctx->hostcomm.user, h.data(), int(n)) == 0,
            "host collective (all-reduce max, %zu f64) failed", n);
  return sgp_h2d(ctx, dev, h.data(), n * 8);
}

static int coll_allreduce_max_i32(sgp_ctx* ctx, int32_t* dev, size_t n) {
  if (ctx->comm) {
    SGP_NCCL(ctx, g_rccl.AllReduce(dev, dev, n, ncclInt32, ncclMax,
                                   static_cast<ncclComm_t>(ctx->comm), ctx->stream));
    return 0;
  }
  if (!ctx->hostcomm.allreduce_max_i32) return 0;
  std::vector<int32_t> h(n);
  SGP_TRY(sgp_d2h(ctx, h.data(), dev, n * 4));
  SGP_CHECK(ctx, ctx->hostcomm.allreduce_max_i32(ctx->hostcomm.user, h.data(), int(n)) == 0,
            "host collective (all-reduce max, %zu i32) failed", n);
  return sgp_h2d(ctx, dev, h.data(), n * 4);
}

// recv (device) = the nbytes of every rank, in rank order
int coll_allgather(sgp_ctx* ctx, const void* send, void* recv, size_t nbytes) {
  if (ctx->comm) {
    SGP_NCCL(ctx, g_rccl.AllGather(send, recv, nbytes, ncclInt8,
                                   static_cast<ncclComm_t>(ctx->comm), ctx->stream));
    return 0;
  }
  if (!ctx->hostcomm.allgather) {
    SGP_HIP(ctx, hipMemcpyAsync(recv, send, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  }
  std::vector<char> hs(nbytes), hr(nbytes * size_t(ctx->world));
  SGP_TRY(sgp_d2h(ctx, hs.data(), send, nbytes));
  SGP_CHECK(ctx, ctx->hostcomm.allgather(ctx->hostcomm.user, hs.data(), hr.data(),
                                         int64_t(nbytes)) == 0,
            "host collective (all-gather, %zu bytes per rank) failed", nbytes);
  return sgp_h2d(ctx, recv, hr.data(), hr.size());
}

// have_comm(ctx) -- or the error of a rank of several without a communicator
int comm_or_single(sgp_ctx* ctx, bool* comm) {
  *comm = have_comm(ctx);
  SGP_CHECK(ctx, *comm || ctx->world <= 1,
            "rank %d of %d has no communicator in the grid's context: the "
            "in-stream collectives cannot run (sgp_comm_init on THIS context)",
            ctx->rank, ctx->world);
  return 0;
}

// Front half of compute_sets on this rank's shard with the cross-rank scalars kept
// on the device: max l0[S] (left in g->scal[0] by a confidence pass without
// read-back) and the maximiser width are all-reduced IN STREAM, the kernels read
// them from device memory; `res` (device) receives the front block.  Without a
// communicator (one rank) the all-reduces are skipped.
static int front_half_in_stream(sgp_grid* g, const double* scaling, const double* thr_beta,
                                double* res) {
  sgp_ctx* ctx = g->ctx;
  SGP_TRY(settle_max_l(g));
  bool comm;
  SGP_TRY(comm_or_single(ctx, &comm));
  if (comm) SGP_TRY(coll_allreduce_max_f64(ctx, g->scal, 1));
  SGP_TRY(launch_maximizers(g, 0.0, g->scal));
  SGP_TRY(launch_reduce_max(ctx, g->partial, (g->N + 255) / 256, res + kResMaxWidth));
  if (comm) SGP_TRY(coll_allreduce_max_f64(ctx, res + kResMaxWidth, 1));
  SGP_TRY(launch_candidates(g, 0.0, res + kResMaxWidth, scaling, thr_beta, 0,
                            reinterpret_cast<unsigned long long*>(res + kResCounts)));
  return front_first(g, res);
}

// N-rank front half with the cross-rank scalars kept on the device: max l0[S]
// (left in g->scal[0] by a confidence pass without read-back) and the maximiser
// width are all-reduced IN STREAM (RCCL on the context's stream), the kernels
// read them from device memory, and one read-back returns this rank's counts,
// its first candidate and the global max l0.  Without a communicator (one
// rank) the all-reduces are skipped.
int sgp_grid_sets_front_comm(sgp_grid* g, const double* scaling,
                             const double* thr_beta, double* out5, double* x_top,
                             double* mean_top, double* q_top, double* max_l_out) {
  sgp_ctx* ctx = g->ctx;
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  const int d = g->d, G = g->G;
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, size_t(res_words(d, G) + 8) * 8, &res));
  SGP_TRY(front_half_in_stream(g, scaling, thr_beta, res));
  SGP_HIP(ctx, hipMemcpyAsync(res + res_max_l(d, G), g->scal, 8,
                              hipMemcpyDeviceToDevice, ctx->stream));
  StepOut o{out5, x_top, mean_top, q_top};
  o.max_l = max_l_out;
  return read_result(g, res, res_words(d, G), o);
}

// Back half for ONE candidate (the common case: the first candidate is the
// expander): probe scan, conditional G mark and the M|G arg-max with one sync.
int sgp_grid_sets_back(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                       const double* fmin, const double* xc, const double* mu_c,
                       const double* u_c, double near_frac, int64_t gidx_c,
                       int mark, const double* scaling, int32_t* flags,
                       double* value, int64_t* gidx) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  const int64_t li = gidx_c - g->goff;
  SGP_CHECK(ctx, !mark || (li >= 0 && li < g->N),
            "candidate %lld is not owned by this shard", (long long)gidx_c);
  ExpanderBufs eb;
  SGP_TRY(expander_bufs(g, host, G, &eb));
  SGP_TRY(enqueue_expander(g, host, eb, beta, fmin, 1, xc, mu_c, u_c, near_frac));
  if (mark) SGP_TRY(launch_mark_if(g, li, eb.flags, fmin));
  // results in the tail behind the flags: value (f64) | index (i64), one read-back for both
  double* res = eb.tail->res;
  SGP_TRY(launch_argmax(g, SGP_ARGMAX_MG_WIDTH, scaling, res,
                        reinterpret_cast<int64_t*>(res + 1)));
  const size_t at = eb.l.tail - eb.l.flags;
  std::vector<char> hb(at + 16);
  SGP_TRY(sgp_d2h(ctx, hb.data(), eb.flags, hb.size()));
  memcpy(flags, hb.data(), size_t(G) * 4);
  memcpy(value, hb.data() + at, 8);
  memcpy(gidx, hb.data() + at + 8, 8);
  return 0;
}

// Single-rank fast path, both halves with ONE stream sync: the front half
// leaves the first candidate on the device, the probe scan runs on it right
// away, G is marked if it is certified and the M|G arg-max follows.  The host
// decides afterwards which of the results apply (no candidate / nothing unsafe:
// the back results are void except the arg-max; candidate not certified: the
// exact scan and the general loop take over).
int sgp_grid_sets_fused(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, double max_l, const double* scaling,
                        const double* thr_beta, double near_frac, double* out5,
                        double* x_top, double* mean_top, double* q_top,
                        int32_t* flags, double* value, int64_t* gidx,
                        double* max_l_out) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  const int d = g->d, nres = res_words(d, G);
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, size_t(nres + 8) * 8, &res));
  // max_l = NaN: the confidence pass was issued without read-back; the value
  // is in g->scal[0] or still spread over the sweep's per-wave partials
  const bool resident = max_l != max_l;
  const bool pending = resident && g->l0_pending > 0;
  ExpanderBufs eb;
  SGP_TRY(expander_bufs(g, host, G, &eb));
  // Seven launches and one stream synchronisation: maximisers -> candidates (+ the first
  // one per workgroup) -> [k_expkt: first candidate of the shard, staged as the operand of
  // the expander test, AND L^-1 k_c] -> k_expw1 -> pre-filter -> listed rows -> conditional
  // G mark + M|G arg-max per workgroup.  The reductions in between are folded into the
  // consumers; the result block and the arg-max partials land in mapped host memory, where
  // the last level of the arg-max is taken (no final launch, no read-back copy).
  // Grids beyond ~2.5e8 rows (or SGP_SETS_COPY set) keep the block in scratch: the front
  // and the arg-max end in launches of their own (k_front_final, k_argmax_final_f), and one
  // read-back copy returns the block.
  const int nbp = argmax_marked_blocks(g->N);
  const size_t part_at = size_t(nres) + 8 - (nres & 1);      // (16-byte aligned pairs)
  const size_t need = size_t(nres) + 8 + 2 * size_t(nbp);
  static const bool copy = getenv("SGP_SETS_COPY") != nullptr;
  const bool mapped = !copy && need * 8 <= (size_t(4) << 20);
  if (mapped && ctx->sets_cap < need) {
    if (ctx->sets_host) (void)hipHostFree(ctx->sets_host);
    ctx->sets_host = nullptr;
    ctx->sets_cap = 0;
    const size_t cap = std::max<size_t>(need, 4096);
    SGP_TRY(mapped_block(ctx, cap, &ctx->sets_host, &ctx->sets_dev));
    ctx->sets_cap = cap;
  }
  double* dres = mapped ? ctx->sets_dev : res;     // the block the host reads
  FrontArgs fold{};
  SGP_TRY(launch_sets_front_fused(
      g, max_l, pending ? g->partial : nullptr, g->l0_pending,
      (resident && !pending) ? g->scal : nullptr, scaling, thr_beta, res,
      dres + res_max_l(d, G), eb.xc, int(eb.l.staged / 8), eb.flags, int(eb.l.zeroed / 4),
      mapped ? &fold : nullptr));
  fold.res_host = dres;
  g->l0_pending = 0;
  SGP_TRY(enqueue_expander(g, host, eb, beta, fmin, 1, nullptr, nullptr, nullptr, near_frac,
                           mapped ? &fold : nullptr));
  SGP_TRY(launch_argmax_marked(
      g, scaling, fmin, eb.flags, reinterpret_cast<int64_t*>(res + kResTopIdx),
      reinterpret_cast<int*>(res + kResFound), reinterpret_cast<int32_t*>(dres + res_flags(d, G)),
      mapped ? nullptr : dres + res_value(d, G),
      mapped ? nullptr : reinterpret_cast<int64_t*>(dres + res_index(d, G)),
      mapped ? ctx->sets_dev + part_at : nullptr));
  const StepOut o{out5, x_top, mean_top, q_top, flags, value, gidx, max_l_out};
  if (!mapped) {
    SGP_TRY(read_result(g, res, nres, o));
  } else {
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unpack_result(ctx->sets_host, d, G, o);
    // np.argmax over the workgroups' results: largest value, first index among equals
    const double* hpart = ctx->sets_host + part_at;
    const int64_t* hidx = reinterpret_cast<const int64_t*>(hpart + nbp);
    double bv = -INFINITY;
    int64_t bi = -1;
    for (int e = 0; e < nbp; ++e) {
      const int64_t i = hidx[e];
      if (i < 0) continue;
      const double v = hpart[e];
      if (bi < 0 || v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
      }
    }
    *value = bv;
    *gidx = bi;
  }
  if (max_l_out && !resident) *max_l_out = max_l;
  return 0;
}

// A whole SafeOpt.optimize() of a SMALL grid -- intervals, S, M, candidates, the exact
// expander test of the first candidate, the G mark and the arg-max -- in ONE launch of one
// workgroup and one read-back (step_small.hip).  Same result block as sgp_grid_sets_fused.
int sgp_grid_step_small(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                        const double* fmin, const double* scaling, const double* thr_beta,
                        double* out5, double* x_top, double* mean_top, double* q_top,
                        int32_t* flags, double* value, int64_t* gidx, double* max_l_out) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  SGP_CHECK(ctx, step_small_eligible(ctx, host, G, g->N),
            "sgp_grid_step_small: %lld rows / a GP with more than 48 observations "
            "(sgp_grid_step_small_ok)", (long long)g->N);
  if (!ctx->step_host) SGP_TRY(mapped_block(ctx, kStepResWords, &ctx->step_host, &ctx->step_dev));
  g->l0_pending = 0;
  const uint64_t seq = ++ctx->step_seq;
  SGP_TRY(launch_step_small(g, g->gpdev, host, G, beta, fmin, scaling, thr_beta, ctx->step_dev,
                            seq));
  g->post_valid = true;
  // No read-back copy, no stream synchronisation: the kernel writes its result block into
  // host memory and a completion word behind it; spin on that word (a launch of 20-40 us),
  // fall back to the stream when it does not turn up.
  {
    volatile uint64_t* done = reinterpret_cast<volatile uint64_t*>(ctx->step_host) +
                              (kStepResWords - 1);
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t spins = 0;
    while (*done != seq) {
      if ((++spins & 1023u) == 0 &&
          std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
        SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SGP_CHECK(ctx, *done == seq, "sgp_grid_step_small: the kernel left no result");
        break;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  double hostres[kStepResWords];
  memcpy(hostres, ctx->step_host, size_t(res_words(g->d, G)) * 8);
  static const bool stamps = getenv("SGP_STEP_STAMPS") != nullptr;
  if (stamps) {      // (-DSTEP_STAMPS builds of step_small.hip)
    const uint64_t* st = reinterpret_cast<const uint64_t*>(ctx->step_host) + 40;
    static int shown = 0;
    if (++shown % 500 == 0) {
      fprintf(stderr, "step stamps (ticks):");
      for (int i = 1; i < 8; ++i) fprintf(stderr, " %d:%lld", i, (long long)(st[i] - st[i - 1]));
      fprintf(stderr, "\n");
    }
  }
  unpack_result(hostres, g->d, G, {out5, x_top, mean_top, q_top, flags, value, gidx, max_l_out});
  return 0;
}

// 1 when sgp_grid_step_small serves this grid with these GPs (at most kStepSmallRows rows, every GP
// with at most 48 observations, sweep kernel not forced), else 0
int sgp_grid_step_small_ok(sgp_grid* g, sgp_gp* const* gps, int G) {
  if (!g || G != g->G || G < 1 || G > SGP_MAX_GPS) return 0;
  GpDev host[SGP_MAX_GPS];
  for (int i = 0; i < G; ++i) {
    if (!gps[i] || gps[i]->n <= 0 || gps[i]->ctx != g->ctx) return 0;
    host[i] = gps[i]->dev;
  }
  return step_small_eligible(g->ctx, host, G, g->N) ? 1 : 0;
}

// A FLEET of small problems in one call: what sgp_grid_step_small does for one grid, for B
// grids of one context side by side -- one workgroup per member (step_small.hip:
// k_step_small_many), one launch per kernel instance present (input dimension, observation
// class, single-part or not), back to back in the context's stream.  Every member gets its
// own record, its own result block in mapped host memory and its own completion word; the
// records and the GP descriptors they point to go up in ONE copy.  Nothing is launched or
// written before every member has been checked.
int sgp_grid_step_small_many(sgp_grid* const* grids, sgp_gp* const* gps, const int* G, int B,
                             const double* beta, const double* fmin, const double* scaling,
                             const double* thr_beta, double* out5, double* x_top,
                             double* mean_top, double* q_top, int32_t* flags, double* value,
                             int64_t* gidx, double* max_l_out) {
  sgp_ctx* ctx = (grids && B >= 1 && grids[0]) ? grids[0]->ctx : nullptr;
  SGP_CHECK(ctx, B >= 1, "sgp_grid_step_small_many: %d members, at least 1 expected", B);
  SGP_CHECK(ctx, grids && grids[0], "sgp_grid_step_small_many: member 0 has no grid");
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  // ---- every refusal, in member order
  struct Seen {
    const void* p;
    int member;
    bool operator<(const Seen& o) const { return p < o.p || (p == o.p && member < o.member); }
  };
  static thread_local std::vector<Seen> seen_grid, seen_gp;
  static thread_local std::vector<GpDev> hosts;
  static thread_local std::vector<int> first, key, order;
  seen_grid.clear();
  seen_gp.clear();
  hosts.clear();
  first.assign(size_t(B) + 1, 0);
  key.assign(size_t(B), 0);
  for (int b = 0; b < B; ++b) {
    sgp_grid* g = grids[b];
    SGP_CHECK(ctx, g, "sgp_grid_step_small_many: member %d has no grid", b);
    SGP_CHECK(ctx, g->ctx == ctx,
              "sgp_grid_step_small_many: member %d lives in another context than member 0", b);
    sgp_gp* const* mg = gps + size_t(b) * SGP_MAX_GPS;
    GpDev host[SGP_MAX_GPS];
    bool ok = G[b] == g->G && G[b] >= 1 && G[b] <= SGP_MAX_GPS;
    SGP_CHECK(ctx, ok, "sgp_grid_step_small_many: member %d: grid was created for %d GPs, got %d",
              b, g->G, G[b]);
    if (collect_gps(ctx, mg, G[b], g->d, host) != 0) {
      const std::string why = ctx->err;
      sgp_set_error(ctx, "sgp_grid_step_small_many: member %d: %s", b, why.c_str());
      return -2;
    }
    SGP_CHECK(ctx, step_small_eligible(ctx, host, G[b], g->N),
              "sgp_grid_step_small_many: member %d: %lld rows / a GP with more than 48 "
              "observations (sgp_grid_step_small_ok)", b, (long long)g->N);
    seen_grid.push_back({g, b});
    for (int i = 0; i < G[b]; ++i) {
      seen_gp.push_back({mg[i], b});
      hosts.push_back(host[i]);
    }
    first[size_t(b) + 1] = first[size_t(b)] + G[b];
    key[size_t(b)] = step_group_key(g->d, host, G[b]);
  }
  {
    int bad_grid = B, bad_gp = B;
    std::sort(seen_grid.begin(), seen_grid.end());
    for (size_t i = 1; i < seen_grid.size(); ++i)
      if (seen_grid[i].p == seen_grid[i - 1].p) bad_grid = std::min(bad_grid, seen_grid[i].member);
    std::sort(seen_gp.begin(), seen_gp.end());
    // (one member may name a GP twice, as sgp_grid_step_small allows; two members may not
    // share one: the members of a fleet are independent problems)
    for (size_t i = 1; i < seen_gp.size(); ++i)
      if (seen_gp[i].p == seen_gp[i - 1].p && seen_gp[i].member != seen_gp[i - 1].member)
        bad_gp = std::min(bad_gp, seen_gp[i].member);
    SGP_CHECK(ctx, bad_grid == B || bad_gp < bad_grid,
              "sgp_grid_step_small_many: member %d uses the grid of an earlier member", bad_grid);
    SGP_CHECK(ctx, bad_gp == B,
              "sgp_grid_step_small_many: member %d uses a GP of an earlier member", bad_gp);
  }
  // ---- room: result blocks, staging buffer, records on the device
  if (ctx->fleet_cap < size_t(B)) {
    if (ctx->fleet_host) {
      SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipHostFree(ctx->fleet_host);
    }
    ctx->fleet_host = nullptr;
    ctx->fleet_cap = 0;
    const size_t cap = std::max<size_t>(size_t(B) + size_t(B) / 2, 64);
    SGP_TRY(mapped_block(ctx, cap * kStepResWords, &ctx->fleet_host, &ctx->fleet_dev));
    ctx->fleet_cap = cap;
  }
  const size_t rb = step_record_bytes();
  const size_t gp_at = (size_t(B) * rb + 15) & ~size_t(15);
  const size_t bytes = gp_at + hosts.size() * sizeof(GpDev);
  if (ctx->fleet_stage_cap < bytes) {
    if (ctx->fleet_stage) {
      SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipHostFree(ctx->fleet_stage);
    }
    ctx->fleet_stage = nullptr;
    ctx->fleet_stage_cap = 0;
    const size_t cap = bytes + bytes / 2;
    SGP_HIP(ctx, hipHostMalloc(&ctx->fleet_stage, cap, hipHostMallocDefault));
    ctx->fleet_stage_cap = cap;
  }
  SGP_TRY(sgp_reserve(ctx, &ctx->fleet_recs, bytes));
  // ---- records, grouped by kernel instance (a counting sort: members keep their order
  // inside a group), each pointing at its member's slot of the result array
  int gstart[kStepGroupKeys + 1] = {0};
  for (int b = 0; b < B; ++b) ++gstart[key[size_t(b)] + 1];
  for (int k = 0; k < kStepGroupKeys; ++k) gstart[k + 1] += gstart[k];
  order.assign(size_t(B), 0);
  {
    int at[kStepGroupKeys];
    for (int k = 0; k < kStepGroupKeys; ++k) at[k] = gstart[k];
    for (int b = 0; b < B; ++b) order[size_t(at[key[size_t(b)]]++)] = b;
  }
  char* stage = static_cast<char*>(ctx->fleet_stage);
  char* dev = static_cast<char*>(ctx->fleet_recs.p);
  memcpy(stage + gp_at, hosts.data(), hosts.size() * sizeof(GpDev));
  const uint64_t seq0 = ctx->step_seq;          // member b: seq0 + 1 + b
  ctx->step_seq += uint64_t(B);
  for (int r = 0; r < B; ++r) {
    const int b = order[size_t(r)];
    sgp_grid* g = grids[b];
    g->l0_pending = 0;
    const GpDev* gd = reinterpret_cast<const GpDev*>(dev + gp_at) + first[size_t(b)];
    step_record_fill(stage + size_t(r) * rb, g, gd, G[b], beta[b],
                     fmin + size_t(b) * SGP_MAX_GPS, scaling + size_t(b) * SGP_MAX_GPS,
                     thr_beta + size_t(b) * SGP_MAX_GPS,
                     ctx->fleet_dev + size_t(b) * kStepResWords, seq0 + 1 + uint64_t(b));
  }
  SGP_HIP(ctx, hipMemcpyAsync(dev, stage, bytes, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < kStepGroupKeys; ++k)
    if (gstart[k + 1] > gstart[k])
      SGP_TRY(launch_step_small_group(ctx, k, dev + size_t(gstart[k]) * rb,
                                      gstart[k + 1] - gstart[k]));
  for (int b = 0; b < B; ++b) grids[b]->post_valid = true;
  // ---- the B completion words: one deadline for all of them, then the stream
  {
    const auto t0 = std::chrono::steady_clock::now();
    bool synced = false;
    for (int b = 0; b < B; ++b) {
      volatile uint64_t* done = reinterpret_cast<volatile uint64_t*>(
          ctx->fleet_host + size_t(b) * kStepResWords) + (kStepResWords - 1);
      const uint64_t seq = seq0 + 1 + uint64_t(b);
      uint32_t spins = 0;
      while (*done != seq) {
        if (synced || ((++spins & 1023u) == 0 &&
                       std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200))) {
          if (!synced) SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
          synced = true;
          SGP_CHECK(ctx, *done == seq,
                    "sgp_grid_step_small_many: the kernel left no result for member %d", b);
          break;
        }
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  for (int b = 0; b < B; ++b) {
    const size_t s = size_t(b);
    double hostres[kStepResWords];
    memcpy(hostres, ctx->fleet_host + s * kStepResWords, size_t(res_words(grids[b]->d, G[b])) * 8);
    unpack_result(hostres, grids[b]->d, G[b],
                  {out5 + s * 6, x_top + s * SGP_MAX_D, mean_top + s * SGP_MAX_GPS,
                   q_top + s * 2 * SGP_MAX_GPS, flags + s * SGP_MAX_GPS, value + s, gidx + s,
                   max_l_out + s});
  }
  return 0;
}

// N-rank certified step with ONE stream sync (the N-rank counterpart of
// sgp_grid_sets_fused; gp_opt.py:511-557, 611-612, 635, 642-644): the front half of
// sgp_grid_sets_front_comm on this rank's shard, then IN STREAM
//   all-gather of every rank's front block  -> k_merge_front: the first candidate
//     of the whole grid in visiting order, total counts, ties over all shards,
//     staged as the operand of the expander test on every rank;
//   the probe scan of that candidate over this rank's unsafe rows;
//   all-reduce (max) of the G flags;
//   conditional G mark by the rank that owns the candidate + local M | G arg-max;
//   all-gather of the (value, index) pairs -> k_merge_argmax.
// Every rank reads back the same block.  Without a communicator (one rank) the
// collectives are skipped and the merges run over one block.
int sgp_grid_sets_fused_comm(sgp_grid* g, sgp_gp* const* gps, int G, double beta,
                             const double* fmin, const double* scaling,
                             const double* thr_beta, double near_frac, double* out5,
                             double* x_top, double* mean_top, double* q_top,
                             int32_t* flags, double* value, int64_t* gidx,
                             double* max_l_out) {
  sgp_ctx* ctx = g->ctx;
  GpDev host[SGP_MAX_GPS];
  SGP_TRY(grid_gps(g, gps, G, host));
  bool comm;
  SGP_TRY(comm_or_single(ctx, &comm));
  const int world = comm ? ctx->world : 1;
  // device block: merged result | this rank's front block | gathered front blocks | this
  // rank's (value, index) | gathered pairs
  const int d = g->d, nres = res_words(d, G);
  const size_t nfront = size_t(res_front(d, G));
  const size_t total = nres + 1 + nfront * (1 + size_t(world)) + 2 * (1 + size_t(world));
  double* res;
  SGP_TRY(sgp_scratch(ctx, kSlotResult, (total + 8) * 8, &res));
  double* mine = res + nres + 1;
  double* all = mine + nfront;
  double* pair = all + nfront * size_t(world);
  double* pairs = pair + 2;
  ExpanderBufs eb;
  SGP_TRY(expander_bufs(g, host, G, &eb));

  // ---- front half on this shard
  SGP_TRY(front_half_in_stream(g, scaling, thr_beta, mine));

  // ---- first candidate of the whole grid
  const double* blocks = mine;
  if (comm) {
    SGP_TRY(coll_allgather(ctx, mine, all, nfront * 8));
    blocks = all;
  }
  SGP_TRY(launch_merge_front(g, blocks, world, int(nfront), res, eb.xc,
                             int(eb.l.staged / 8), eb.flags, int(eb.l.zeroed / 4)));
  // ---- probe scan over this shard, flags over all shards
  SGP_TRY(enqueue_expander(g, host, eb, beta, fmin, 1, nullptr, nullptr, nullptr, near_frac));
  if (comm) SGP_TRY(coll_allreduce_max_i32(ctx, eb.flags, size_t(G)));
  // ---- conditional G mark (owner of the candidate) + arg-max over the whole grid
  SGP_TRY(launch_argmax_marked(
      g, scaling, fmin, eb.flags, reinterpret_cast<int64_t*>(res + kResTopIdx),
      reinterpret_cast<int*>(res + kResFound), reinterpret_cast<int32_t*>(res + res_flags(d, G)),
      pair, reinterpret_cast<int64_t*>(pair + 1)));
  const double* prs = pair;
  if (comm) {
    SGP_TRY(coll_allgather(ctx, pair, pairs, 16));
    prs = pairs;
  }
  SGP_TRY(launch_merge_argmax(ctx, prs, world, res + res_value(d, G),
                              reinterpret_cast<int64_t*>(res + res_index(d, G))));
  SGP_HIP(ctx, hipMemcpyAsync(res + res_max_l(d, G), g->scal, 8,
                              hipMemcpyDeviceToDevice, ctx->stream));
  return read_result(g, res, nres, {out5, x_top, mean_top, q_top, flags, value, gidx, max_l_out});
}

// ---- swarm: the sgp_swarm_* entry points live in swarm_api.hip ------------------------

// ---- timing ---------------------------------------------------------------------
int64_t sgp_ctx_alloc_count(sgp_ctx* ctx) { return ctx ? ctx->n_allocs : -1; }

int sgp_ctx_set_share(sgp_ctx* ctx, int on) {
  if (!ctx) return -1;
  const int old = ctx->share_factors;
  if (on == 0 || on == 1) ctx->share_factors = on;
  return old;
}

int sgp_ctx_last_sweep(sgp_ctx* ctx) { return ctx ? ctx->last_sweep : 0; }

int sgp_ctx_set_sweep(sgp_ctx* ctx, int which) {
  if (!ctx) return -1;
  const int old = ctx->sweep_choice;
  if (which >= 0 && which < 128) ctx->sweep_choice = which;
  return old;
}

int sgp_timer_start(sgp_ctx* ctx) {
  SGP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return 0;
}

int sgp_timer_stop(sgp_ctx* ctx, float* ms) {
  SGP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  SGP_HIP(ctx, hipEventSynchronize(ctx->ev1));
  SGP_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  return 0;
}

int sgp_profile_enable(sgp_ctx* ctx, int on) {
  ctx->profiling = on != 0;
  ctx->prof_used = 0;
  ctx->prof_flops = 0.0;
  return 0;
}

int sgp_profile_read(sgp_ctx* ctx, double* total_ms, int64_t* launches,
                     double* flops) {
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double tot = 0.0;
  for (size_t i = 0; i + 1 < ctx->prof_used; i += 2) {
    float ms = 0.f;
    SGP_HIP(ctx, hipEventElapsedTime(&ms, ctx->prof_events[i],
                                     ctx->prof_events[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = int64_t(ctx->prof_used / 2);
  *flops = ctx->prof_flops;
  return 0;
}

int sgp_profile_read_last(sgp_ctx* ctx, double* ms) {
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *ms = 0.0;
  if (ctx->prof_used < 2) return 0;
  float t = 0.f;
  SGP_HIP(ctx, hipEventElapsedTime(&t, ctx->prof_events[ctx->prof_used - 2],
                                   ctx->prof_events[ctx->prof_used - 1]));
  *ms = t;
  return 0;
}

// ---- RCCL -----------------------------------------------------------------------
int sgp_comm_unique_id(void* id128) {
  SGP_TRY(load_rccl(nullptr));
  ncclUniqueId id;
  SGP_NCCL(nullptr, g_rccl.GetUniqueId(&id));
  memcpy(id128, &id, sizeof(id));
  return 0;
}

int sgp_comm_init(sgp_ctx* ctx, const void* id128, int rank, int world) {
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_TRY(load_rccl(ctx));
  SGP_CHECK(ctx, world >= 1 && rank >= 0 && rank < world,
            "bad rank %d / world %d", rank, world);
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t comm;
  SGP_NCCL(ctx, g_rccl.CommInitRank(&comm, world, id, rank));
  ctx->comm = comm;
  ctx->rank = rank;
  ctx->world = world;
  return 0;
}

int sgp_comm_init_host(sgp_ctx* ctx, int rank, int world,
                       sgp_host_allreduce_max_f64 allreduce_f64,
                       sgp_host_allreduce_max_i32 allreduce_i32,
                       sgp_host_allgather allgather, void* user) {
  SGP_CHECK(ctx, world >= 1 && rank >= 0 && rank < world,
            "bad rank %d / world %d", rank, world);
  SGP_CHECK(ctx, !ctx->comm, "the context already has an RCCL communicator");
  SGP_CHECK(ctx, allreduce_f64 && allreduce_i32 && allgather,
            "sgp_comm_init_host: all three collectives are required");
  ctx->hostcomm.allreduce_max_f64 = allreduce_f64;
  ctx->hostcomm.allreduce_max_i32 = allreduce_i32;
  ctx->hostcomm.allgather = allgather;
  ctx->hostcomm.user = user;
  ctx->rank = rank;
  ctx->world = world;
  return 0;
}

int sgp_comm_count(sgp_ctx* ctx, int* n) {
  *n = 1;
  if (ctx->hostcomm.allgather) {  // (the caller's transport: its word for it)
    *n = ctx->world;
    return 0;
  }
  if (!ctx->comm) return 0;       // no communicator: a single rank
  SGP_NCCL(ctx, g_rccl.CommCount(static_cast<ncclComm_t>(ctx->comm), n));
  return 0;
}

// Small host -> device copy through the pinned staging half (no stream sync:
// the collective and the read-back that follow are ordered behind it and the
// read-back's sync completes all three); large payloads take the synchronous
// path.
static int stage_h2d(sgp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes > ctx->pinned_cap / 4) return sgp_h2d(ctx, dst, src, bytes);
  char* slot = static_cast<char*>(ctx->pinned) + ctx->pinned_cap / 2;
  memcpy(slot, src, bytes);
  SGP_HIP(ctx, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice,
                              ctx->stream));
  return 0;
}

int sgp_comm_allreduce_max(sgp_ctx* ctx, double* buf, int n) {
  if ((ctx->world <= 1 && !ctx->comm) || n <= 0) return 0;
  if (!ctx->comm && ctx->hostcomm.allreduce_max_f64) {
    SGP_CHECK(ctx, ctx->hostcomm.allreduce_max_f64(ctx->hostcomm.user, buf, n) == 0,
              "host collective (all-reduce max) failed");
    return 0;
  }
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, ctx->comm, "sgp_comm_init was not called");
  double* d;
  SGP_TRY(sgp_scratch(ctx, kSlotSmall, size_t(n) * 8, &d));
  SGP_TRY(stage_h2d(ctx, d, buf, size_t(n) * 8));
  SGP_NCCL(ctx, g_rccl.AllReduce(d, d, size_t(n), ncclFloat64, ncclMax,
                                 static_cast<ncclComm_t>(ctx->comm),
                                 ctx->stream));
  return sgp_d2h(ctx, buf, d, size_t(n) * 8);
}

int sgp_comm_allgather(sgp_ctx* ctx, const void* send, void* recv,
                       int64_t nbytes) {
  if (nbytes <= 0) return 0;
  if (ctx->world <= 1 && !ctx->comm) {
    memcpy(recv, send, size_t(nbytes));
    return 0;
  }
  if (!ctx->comm && ctx->hostcomm.allgather) {
    SGP_CHECK(ctx, ctx->hostcomm.allgather(ctx->hostcomm.user, send, recv, nbytes) == 0,
              "host collective (all-gather) failed");
    return 0;
  }
  SGP_HIP(ctx, hipSetDevice(ctx->device));
  SGP_CHECK(ctx, ctx->comm, "sgp_comm_init was not called");
  char* d;
  SGP_TRY(sgp_scratch(ctx, kSlotSmall, size_t(nbytes) * (size_t(ctx->world) + 1), &d));
  char* r = d + nbytes;
  SGP_TRY(stage_h2d(ctx, d, send, size_t(nbytes)));
  SGP_NCCL(ctx, g_rccl.AllGather(d, r, size_t(nbytes), ncclInt8,
                                 static_cast<ncclComm_t>(ctx->comm),
                                 ctx->stream));
  return sgp_d2h(ctx, recv, r, size_t(nbytes) * size_t(ctx->world));
}

int sgp_comm_barrier(sgp_ctx* ctx) {
  double z = 0.0;
  SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return sgp_comm_allreduce_max(ctx, &z, 1);
}

}  // extern "C"
