// posterior_sweep: the dominant kernel of the path.
//
// Replaces gp.predict_noiseless(self.inputs) + the Q update of
// SafeOpt.update_confidence_intervals (safeopt/gp_opt.py:453-476), the safe-set
// test (:478-481), the posterior half of SafeOptSwarm._compute_particle_fitness
// (:901-1013; the shaping is k_fitness_small on the sweep's mean / var, launch_sweep
// below).
// This file: the 4-wave kernel k_sweep for factors up to 256 rows (config 2) with its stage
// table, the dispatch to the other sweep kernels (sweep_tiny.hip, sweep_mid.hip, and the
// paired-wave kernel of sweep_pair.hip above 256 rows), and the per-axis factor tables of
// tensor grids.  (The expander test and the rank-1 refresh: expander.hip.)
//
// For a tile of candidate rows the kernel forms the covariance tile
// K[j, pt] = k(X_j, x_pt) ON THE FLY in registers and contracts it with
// A = L^-1 (lower triangular, pre-packed in MFMA operand order) on the fp64
// matrix cores (v_mfma_f64_4x4x4_4b_f64, see "matrix part" below):
//     var(pt)  = k(x,x) - || A K[:, pt] ||^2          (n^2 flops / row)
//     mean(pt) = alpha . K[:, pt]                      (2n flops / row)
// K (n x N doubles, 4 GB per GP at n = 500, N = 1e6) is never written to memory.
//
// Work split: workgroup = kNW = 4 waves, wave w owns 16 rows (the MFMA N dimension);
// the waves of a workgroup share the staged A chunk through LDS (LDS-DMA,
// double buffered, one barrier per stage).  The rows of A are processed in
// chunks of 16 MFMA row blocks (256 rows) held in 16 accumulator slots per wave;
// the triangular structure is exploited at 16x16 block granularity.  The kernel
// is persistent; the (tile, GP, chunk, j-block) loop nest is flattened into one
// stage sequence described by a small table the HOST builds (StageEnt), so the
// per-stage bookkeeping is one scalar load and a few scalar ALU instructions.
//
// What sets the speed (profiles/r02/probes.txt): the fp64 MFMA occupies its SIMD
// for 16 cycles and a co-resident wave gets ONE issue slot per MFMA of its
// partner, of any instruction type.  Everything that is not an MFMA therefore
// costs wall time roughly in proportion to its instruction COUNT; the stage loop
// below is written for few instructions per MFMA:
//   * accumulator slots are ordered so that the active ones are a prefix
//     (slot s <-> row block bend-1-s): one compare + branch per executed slot;
//   * the covariance operand is broadcast to the four column quads through a
//     wave-private LDS transpose (2 stores + 8 16-byte loads instead of 32
//     swizzles);
//   * covariances needed again by a later accumulator chunk are re-evaluated,
//     not parked in global memory (a slab of 64-459 MB and ~12 GB of traffic per
//     launch in round 1 for 3-5 %).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "small_path.h"
#include "sweep_shared.h"
#include "sweep_slots.h"

namespace {

// 1: a wave's share of the next A chunk (slots w, w + 4, ..) is copied piecewise
// between the slots of the running stage instead of in one burst behind the barrier
// (the paired kernel's finding, profiles/r03/experiments.txt section 4)

constexpr int kJC = 16;                // training points per stage (one j-block)
constexpr int kSteps = kJC / 4;        // MFMA k-steps per stage
constexpr int kNW = 4;                 // waves per workgroup (two workgroups per CU)
constexpr int kSL = 16;                // accumulator slots per wave

// LDS layout for kSL accumulator slots per wave (kSL x 16 rows of L^-1 per chunk):
//   [2][A chunk | training rows | alpha]  exp table  [kNW] broadcast buffers
// 16 slots: 256 VGPRs, two waves per SIMD (two 4-wave workgroups per CU).  (32
// slots with one wave per SIMD and AGPRs, 8-wave workgroups and an explicit
// ping-pong of the two waves of a SIMD were measured and dropped:
// profiles/r02/experiments.txt, commits 1869720 and ad93c1b.)
// A wave's broadcast buffer holds 4 k-rows of 64 doubles, kKbRow doubles apart
// (an odd multiple of 16: the k-rows then sit on disjoint banks).  The padding
// between them doubles as the staging area of the wave's Q rows (kQCap doubles):
// 48 doubles per k-row up to d = 4 (Q rows of up to 6 GPs), 16 beyond (2 GPs) --
// what keeps two workgroups per CU inside 160 KB of LDS.
// R: alpha chunks of up to R riders behind the leader's (kSweepRide, see launch_posterior)
template <int D, int R = 0>
struct Lay {
  static constexpr int kATile = kSL * kSteps * 64;          // doubles
  static constexpr int kXTile = kJC * D;
  static constexpr int kBuf = kATile + kXTile + kJC * (1 + R);   // + alpha chunk(s)
  static constexpr int kTabOff = 2 * kBuf;                  // exp table
  static constexpr int kKbOff = kTabOff + kExpTabSize;
  static constexpr int kKbRow = D <= 4 ? 112 : 80;
  static constexpr int kKbBuf = 4 * kKbRow;
  static constexpr int kQPad = kKbRow - 64;                 // doubles per k-row
  static constexpr int kQMaxG = kQPad / 8;                  // 16 rows x 2 G doubles
  static constexpr size_t bytes() {
    return (size_t(kKbOff) + size_t(kNW) * kKbBuf) * sizeof(double);
  }
  // double2 number i of a wave's staged Q block -> offset (doubles) in its buffer
  static __device__ __forceinline__ int qoff(int i) {
    return (i / (kQPad / 2)) * kKbRow + 64 + 2 * (i % (kQPad / 2));
  }
};

// One stage of the flattened (GP, chunk, j-block) sequence of a tile, built on
// the host (stage_table) with ABSOLUTE device addresses: no pointer arithmetic per
// stage on the device, one scalar load per entry.  Position t of the staged A chunk
// holds row block bend-1-t of the chunk, k-steps 4 jb .. 4 jb + 3; its source is
// a_src - t * rs_bytes.
struct StageEnt {
  uint64_t a_src;      // device address of position 0's 2 KB
  uint64_t xa;         // device address of the j-block's [16 d rows | 16 alpha] (GpDev::XA);
                       // launches on factor tables (SEP): of its 16 alpha
  uint32_t rs_bytes;   // bytes between consecutive row blocks in Apack
  uint32_t jb;         // j-block: training points 16 jb .. 16 jb + 15
  uint32_t word;       // see SW_*
  uint32_t slot0;      // 2-KB positions of the stages in front of this one (resident mode)
};
enum : uint32_t {
  SW_NACT_MASK = 63u,       // active slots 0 .. nact-1 (1..32)
  SW_CHUNK_END = 1u << 6,   // last j-block of an accumulator chunk: fold
  SW_GP_END = 1u << 7,      // last stage of a GP: row epilogue
  SW_TILE_END = 1u << 8,    // last stage of the tile
  SW_MEAN = 1u << 9,        // stage of the LAST chunk: accumulate alpha . k
  SW_NARROW = 1u << 10,     // slot 0 is the last row block with <= 12 real rows: taken
                            // as SW_NGRP narrow 4-row groups (narrow_groups)
  SW_G_SHIFT = 12,          // GP index (3 bits)
  SW_NGRP_SHIFT = 16,       // narrow groups of slot 0 (1..3)
  SW_FIRST = 1u << 18,      // first stage (j-block 0) of an accumulator chunk
  SW_NSL_SHIFT = 19         // slots of the stage's chunk (1..16; 5 bits)
};

// Timing experiments ("what does the kernel cost without X"; results are wrong
// with any bit set): built only with -DSGP_INSTRUMENT, selected at run time by
// SGP_ABLATE=<mask>: 1 no stage barrier, 2 no LDS-DMA, 4 no covariance
// evaluation, 8 no MFMA, 16 no mean/var/Q stores, 32 no per-GP epilogue at all.
#ifdef SGP_INSTRUMENT
#define SGP_ABL(mask) (p.ablate & (mask))
#else
#define SGP_ABL(mask) false
#endif

struct SweepParams {
  const GpDev* gps;
  int G;
#ifdef SGP_INSTRUMENT
  int ablate;      // timing experiments (scripts/ablate.py), see SGP_ABL
#endif
  SweepPoints pts;
  ConfOut conf;
  const StageEnt* stages;   // [nstages] one tile's stage sequence (all GPs)
  int nstages;
  // Small factors stay in LDS for the whole launch (n <= ~112 rows in all GPs together):
  // every stage's positions are copied ONCE, packed back to back, the [rows | alpha]
  // blocks behind them from byte res_xbase on -- no LDS-DMA, no wait and no barrier per
  // stage, the waves of a workgroup run free.  0: the chunks are streamed (double buffer).
  int resident;
  unsigned res_xbase;
  int single;               // every GP has a one-part kernel (pre-scaled inputs)
  long long ride_delta[SGP_MAX_GPS];   // rider g: bytes from its leader's XA to its own
  int nride[SGP_MAX_GPS];   // riders of GP g: the GPs g + 1 .. g + nride[g] share its
                            // factor AND its covariances (GpDev::share) and have no stages
                            // of their own -- their alpha . k is formed in g's stages
  SepLaunch sep;            // tensor grid + factor tables (instances with SEP > 0)
#ifdef SGP_STAMPS
  unsigned long long* stamps;   // [blocks][4 waves][8] cycles per phase (debug build)
#endif
};

// Per-phase cycle stamps of the stage loop (-DSGP_STAMPS, scripts/dev): s_memtime at
// the phase boundaries, summed per wave.  Perturbs the run (every stamp drains the
// LDS / scalar-load counter); for attribution only.
#ifdef SGP_STAMPS
#define SGP_STAMP(i)                                                   \
  do {                                                                 \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();        \
    stamp_acc[i] += (unsigned int)(t_ - stamp_prev);                   \
    stamp_prev = t_;                                                   \
  } while (0)
#else
#define SGP_STAMP(i) do {} while (0)
#endif

// the stage table is read-only for the whole launch: constant address space, so
// that an entry is ONE scalar load (a plain global pointer becomes a vector load
// with a full memory wait, since the kernel also stores to global memory)
typedef const __attribute__((address_space(4))) StageEnt* stage_ptr_t;
__device__ __forceinline__ StageEnt load_stage(stage_ptr_t t, int i) {
  StageEnt e;      // member-wise: scalar loads
  e.a_src = t[i].a_src;
  e.xa = t[i].xa;
  e.rs_bytes = t[i].rs_bytes;
  e.jb = t[i].jb;
  e.word = t[i].word;
  e.slot0 = t[i].slot0;
  return e;
}
typedef const __attribute__((address_space(4))) GpDev* gpdev_cptr_t;

constexpr int kSweepRide = 2;      // riders per leader (what two workgroups' LDS holds)

// ---- matrix part ------------------------------------------------------------------
// v_mfma_f64_4x4x4_4b_f64 is the fp64 matrix instruction that reaches the chip's
// peak on gfx950 (74-77 TFLOP/s measured vs 49 for v_mfma_f64_16x16x4_f64).  Its
// operand maps (probed):
//   A[blk][i][k] <- lane 16k + 4blk + i     B[blk][k][j] <- lane 16k + 4blk + j
//   D[blk][i][j] -> lane 16i + 4blk + j
// Used with blk = 4-row group: the A operand is then the SAME register the
// 16x16x4 form takes (lane = 16k + row, row = 4blk + i), one instruction is a
// 16-row x 4-column x 4-deep product, and a 16-column slab needs four of them
// (m = 0..3) whose B operands are the covariance register with column quad m
// broadcast to all four quads of each 16-lane row.  (cbsz / abid do NOT
// broadcast for this opcode on gfx950 -- probed, scripts/dev/probe_cbsz.hip.)
// Accumulator component m of a slot holds rows 4((l>>2)&3) + (l>>4), column
// 4m + (l&3).

// (broadcast_quads: sweep_shared.h)

// A operands of one slot: the 4 k-steps of the staged j-block.
__device__ __forceinline__ void load_slot(double (&ops)[4], const double* aT,
                                          int slot) {
#pragma unroll
  for (int q = 0; q < 4; ++q) ops[q] = aT[(slot * kSteps + q) * 64];
}

// One 16-wide j-block against accumulator slots 0..nact-1: a slot is 16 MFMAs on
// four independent accumulators (groups of four separated by one wait state --
// measured: a dense stream without them runs 17.4 cycles per MFMA instead of
// 16.25, profiles/r02/probes.txt); the next slot's A operands are read from LDS
// while they execute (the read of slot nact is harmless: it stays inside the
// stage buffer; the empty asm keeps the compiler from sinking the reads into the
// next slot's block, where their latency would be exposed).  The active slots are
// a prefix, so the guards nest: the first inactive slot leaves the whole sequence
// with one branch.
//
// The MFMA goes through inline asm with the accumulator tied to destination AND
// addend: the builtin lets the register allocator rename the destination, which
// costs v_mov_b64 copies at every join of the guarded sequence.
// (mfma_acc: sweep_shared.h)

//
// Slot 0 of the last chunk is the LAST row block.  With <= 12 real rows it is taken as
// 1..3 NARROW 4-row groups: the A operand of group g carries rows 4 g .. 4 g + 3 in
// all four MFMA blocks -- read from the staged slot (standard layout, lane = 16 k +
// row) with the lane address 16 k + 4 g + (lane & 3): the replication is a broadcast
// read of LDS, no special packing -- so the plain covariance register kv[q], a
// different point quad per block, is the B operand and ONE instruction per k-step
// and group covers all 16 points (accumulator accx[g]: rows l >> 4 of the group,
// point l & 15).  n = 200: 8 real rows in the 13th block, 8 MFMAs per stage instead
// of 16 in the one slot that meets EVERY j-block.  The groups need kv only, not the
// broadcast operands: they are issued in front of the LDS transpose, whose round
// trip passes under them.
constexpr int kMaxNg = 2;     // (three groups, 9..12 rows: measured, no gain over a full slot)
// ONE asm statement for all groups, the groups a GP does not have skipped by a scalar
// branch INSIDE it: variants of the sequence at the source level, or a slot that is
// narrow on one path and full on the other, make the register allocator duplicate
// the 64 accumulators around the joins (400+ bytes of scratch).  Hence also: the
// narrow groups are a region of their own in FRONT of the full slots (position 0 of
// the staged chunk; the full slots then start at position 1) and touch no register
// of theirs.
// Per group four DEPENDENT MFMAs on one accumulator: the addend must not be read
// before the previous result is written (4 wait states for this opcode; nothing pads
// inside asm).  s_nop 1 in front: kv / the register copies the compiler may place
// here are VALU writes, two wait states before an MFMA may read them -- the hazard
// recogniser does not see into the asm.
#define SGP_NARROW_GROUP(ACC, A0, A1, A2, A3)                       \
  "v_mfma_f64_4x4x4_4b_f64 " ACC ", " A0 ", %[k0], " ACC "\n\ts_nop 4\n\t" \
  "v_mfma_f64_4x4x4_4b_f64 " ACC ", " A1 ", %[k1], " ACC "\n\ts_nop 4\n\t" \
  "v_mfma_f64_4x4x4_4b_f64 " ACC ", " A2 ", %[k2], " ACC "\n\ts_nop 4\n\t" \
  "v_mfma_f64_4x4x4_4b_f64 " ACC ", " A3 ", %[k3], " ACC "\n\ts_nop 4\n\t"
__device__ __forceinline__ void narrow_groups(int ngrp, double (&accx)[kMaxNg],
                                              const double (&an)[kMaxNg][4],
                                              const double (&kv)[4]) {
  constexpr int g1 = kMaxNg > 1 ? 1 : 0, g2 = kMaxNg > 2 ? 2 : 0;
  if constexpr (kMaxNg == 1) {
    asm volatile("s_nop 1\n\t" SGP_NARROW_GROUP("%[c0]", "%[a00]", "%[a01]", "%[a02]", "%[a03]")
                 : [c0] "+v"(accx[0])
                 : [a00] "v"(an[0][0]), [a01] "v"(an[0][1]), [a02] "v"(an[0][2]),
                   [a03] "v"(an[0][3]),
                   [k0] "v"(kv[0]), [k1] "v"(kv[1]), [k2] "v"(kv[2]), [k3] "v"(kv[3]));
  } else if constexpr (kMaxNg == 2) {
    // two groups: their chains interleaved (the partner's instruction and s_nop 2 make
    // the 4 wait states of a dependent pair), the second group's half skipped by a branch
    // per k-step when the GP has one group only
#define SGP_NARROW_STEP(Q, A0, A1, K)                                                  \
  "v_mfma_f64_4x4x4_4b_f64 %[c0], " A0 ", " K ", %[c0]\n\t"                             \
  "s_cbranch_scc1 .Lsgp_n1_" #Q "_%=\n\t"                                               \
  "v_mfma_f64_4x4x4_4b_f64 %[c1], " A1 ", " K ", %[c1]\n\t"                             \
  ".Lsgp_n1_" #Q "_%=:\n\ts_nop 3\n\t"
    asm volatile("s_cmp_lt_u32 %[ng], 2\n\ts_nop 0\n\t"
                 SGP_NARROW_STEP(0, "%[a00]", "%[a10]", "%[k0]")
                 SGP_NARROW_STEP(1, "%[a01]", "%[a11]", "%[k1]")
                 SGP_NARROW_STEP(2, "%[a02]", "%[a12]", "%[k2]")
                 SGP_NARROW_STEP(3, "%[a03]", "%[a13]", "%[k3]")
                 "s_nop 2"      // (a VALU instruction may read the results next: 6 wait states)
                 : [c0] "+v"(accx[0]), [c1] "+v"(accx[g1])
                 : [a00] "v"(an[0][0]), [a01] "v"(an[0][1]), [a02] "v"(an[0][2]),
                   [a03] "v"(an[0][3]),
                   [a10] "v"(an[g1][0]), [a11] "v"(an[g1][1]), [a12] "v"(an[g1][2]),
                   [a13] "v"(an[g1][3]),
                   [k0] "v"(kv[0]), [k1] "v"(kv[1]), [k2] "v"(kv[2]), [k3] "v"(kv[3]),
                   [ng] "s"(ngrp)
                 : "scc");
#undef SGP_NARROW_STEP
  } else {
    asm volatile("s_nop 1\n\t" SGP_NARROW_GROUP("%[c0]", "%[a00]", "%[a01]", "%[a02]", "%[a03]")
                 "s_cmp_lt_u32 %[ng], 2\n\ts_cbranch_scc1 .Lsgp_narrow_end_%=\n\t"
                 SGP_NARROW_GROUP("%[c1]", "%[a10]", "%[a11]", "%[a12]", "%[a13]")
                 "s_cmp_lt_u32 %[ng], 3\n\ts_cbranch_scc1 .Lsgp_narrow_end_%=\n\t"
                 SGP_NARROW_GROUP("%[c2]", "%[a20]", "%[a21]", "%[a22]", "%[a23]")
                 ".Lsgp_narrow_end_%=:"
                 : [c0] "+v"(accx[0]), [c1] "+v"(accx[g1]), [c2] "+v"(accx[g2])
                 : [a00] "v"(an[0][0]), [a01] "v"(an[0][1]), [a02] "v"(an[0][2]),
                   [a03] "v"(an[0][3]),
                   [a10] "v"(an[g1][0]), [a11] "v"(an[g1][1]), [a12] "v"(an[g1][2]),
                   [a13] "v"(an[g1][3]),
                   [a20] "v"(an[g2][0]), [a21] "v"(an[g2][1]), [a22] "v"(an[g2][2]),
                   [a23] "v"(an[g2][3]),
                   [k0] "v"(kv[0]), [k1] "v"(kv[1]), [k2] "v"(kv[2]), [k3] "v"(kv[3]),
                   [ng] "s"(ngrp)
                 : "scc");
  }
}
#undef SGP_NARROW_GROUP
// SEP > 0: the rows are a tensor grid with SEP axes and every kernel is a product of
// RBF parts (SepLaunch): a covariance is the product of SEP table entries -- two
// 16-byte loads per axis, lane and stage, issued one stage ahead, instead of ~22 fp64
// instructions per value.  (Instantiated with D = 1: the rows themselves are not read.)
// RES: the factors are small enough to stay in LDS for the whole launch (SweepParams::
// res_xbase) -- instances of their own, so that the streaming instances carry none of it.
template <int D, bool SINGLE, int R = 0, int SEP = 0, bool RES = false>
__global__ __launch_bounds__(64 * kNW, 2) void k_sweep(SweepParams p) {
  constexpr int kTilePts = 16 * kNW;
  // (2 kMaxNg doubles live across the evaluation: where the registers are to be had)
  constexpr bool kAnEarly = SEP > 0 && SEP <= 2 && !(SEP == 2 && R > 0);
  // d >= 5 (and products at d = 4): no registers for the raw row of this tile and of
  // the next one -- the row is read (an L2 hit) where a GP's scaled row is formed
  constexpr bool kLeanX = SEP == 0 && (D >= 5 || (D == 4 && !SINGLE));
  // the entry operands of the slot sequence: requested at the top of the stage (8
  // registers across the evaluation) or, where those are not to be had, in front of it
  constexpr bool kEntryEarly = D <= 5;
  // where the LDS-DMA of the next stage is issued: at the top of the stage, or in front
  // of the full slots (measured per variant: with factor tables the table loads want
  // the head of the queue)
  constexpr bool kDmaLate = SEP > 0;
  typedef Lay<D, R> L;
  constexpr int kATile = L::kATile, kBuf = L::kBuf, kXTile = L::kXTile;
  constexpr int kTabOff = L::kTabOff, kKbOff = L::kKbOff, kKbBuf = L::kKbBuf;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const double* tab = lds + kTabOff;
  exp_tab_init(lds + kTabOff);   // visible after the first staging barrier

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* kbw = lds + kKbOff + wave * kKbBuf;
  const int ntiles = int((p.pts.N + kTilePts - 1) / kTilePts);
  const stage_ptr_t stages = (stage_ptr_t)(p.stages);
  const gpdev_cptr_t gpc = (gpdev_cptr_t)(p.gps);
  const int nstages = p.nstages;
  const int tstep = int(gridDim.x);
  const uint32_t lds0 = lds_addr_of(lds);
  const uint32_t voff = uint32_t(lane) * 16u;

  int tile = int(blockIdx.x);          // tile of the stage being multiplied
  if (tile >= ntiles) return;
  int left = ((ntiles - tile + tstep - 1) / tstep) * nstages;   // stages still to go
  int tile_p = tile;                   // tile of the stage being prefetched

  // candidate rows of the current tile (and, prefetched, of the next one)
  auto load_x = [&](int t, double (&xo)[D]) {
    int64_t r = int64_t(t) * kTilePts + wave * 16 + (lane & 15);
    r = r < p.pts.N ? r : p.pts.N - 1;
#pragma unroll
    for (int k = 0; k < D; ++k)
      xo[k] = __builtin_nontemporal_load(p.pts.base + r * p.pts.stride_row + k * p.pts.stride_col);
  };
  double x[kLeanX ? 1 : D], xnext[kLeanX ? 1 : D];
  if constexpr (!kLeanX) {
    if (SEP == 0) load_x(tile, x);
#pragma unroll
    for (int k = 0; k < D; ++k) xnext[k] = SEP == 0 ? x[k] : 0.0;
  }
  // SEP: byte offsets of this lane's row (lane & 15) and training points (4 (lane >> 4)
  // .. + 3 of a block of 16) in the tables of the tile being PREFETCHED; axis a's index
  // = (global row / stride_a) % count_a with stride_a = count_0 .. count_{a-1}
  constexpr int kAx = SEP > 0 ? SEP : 1;
  uint32_t soff[kAx];
  auto sep_offsets = [&](int t) {
    int64_t r = int64_t(t) * kTilePts + wave * 16 + (lane & 15);
    r = r < p.pts.N ? r : p.pts.N - 1;
    uint32_t q = uint32_t(p.sep.goff + r);
#pragma unroll
    for (int a = 0; a < kAx; ++a) {
      uint32_t idx = q;
      if (a + 1 < kAx) {
        const uint32_t c = p.sep.count[a];
        const uint32_t qn = q / c;
        idx = q - qn * c;
        q = qn;
      }
      soff[a] = idx * 128u + uint32_t(lane >> 4) * 32u;
    }
  };
  // the factors of the stage about to be multiplied (loaded one stage ahead); the
  // tables of the GP being prefetched stay in scalar registers
  double4_t efn[kAx];
  const char* sep_tab[kAx];
  uint32_t sep_pitch[kAx];
  int sep_g = -1;
  auto sep_fetch = [&](const StageEnt& e) {
    const int g = int(e.word >> SW_G_SHIFT) & 7;
    if (g != sep_g) {
      sep_g = g;
#pragma unroll
      for (int a = 0; a < kAx; ++a) {
        sep_tab[a] = reinterpret_cast<const char*>(uniform_ptr(p.sep.tab[g][a]));
        sep_pitch[a] = __builtin_amdgcn_readfirstlane(p.sep.count[a] * 128u);
      }
    }
    // (explicitly GLOBAL loads: a flat load also counts on lgkmcnt, and every LDS wait
    // of the stage would sit out its latency)
    typedef const __attribute__((address_space(1))) double4_t* gvec_t;
#pragma unroll
    for (int a = 0; a < kAx; ++a) {
      const char* src = sep_tab[a] + e.jb * sep_pitch[a];      // (<= 256 MB per GP: sep_launch)
      efn[a] = *(gvec_t)(reinterpret_cast<const double4_t*>(src + soff[a]));
    }
  };

  // What a stage needs besides its table entry comes by LDS-DMA from absolute
  // addresses of the entry: the A chunk (position t = row block bend-1-t, 2 KB each;
  // wave w copies positions w, w + kNW, ..) and the block [16 d rows | 16 alpha] of the
  // j-block (one instruction of one wave; SEP: the 16 alpha only), + the alpha
  // blocks of the riders behind it.
  auto prefetch_to = [&](const StageEnt& e, uint32_t a_dst, uint32_t x_dst) {
    const int nact = int(e.word & SW_NACT_MASK);
    const uint64_t src0 = e.a_src - uint64_t(uint32_t(wave)) * e.rs_bytes;
    const uint64_t step = uint64_t(e.rs_bytes) * kNW;
#pragma unroll
    for (int i = 0; i < kSL / kNW; ++i)
      if (nact > wave + kNW * i)
        dma_2k(src0 - uint64_t(i) * step, a_dst + uint32_t(wave + kNW * i) * 2048u, voff);
    if (wave == kNW - 1) {
      if (SEP > 0) {
        if (lane < 8) dma_1k(e.xa, x_dst + kXTile * 8u, voff);
      } else {
        constexpr int kLanes = 8 * D + 8;              // 16 bytes each
        if (lane < (kLanes < 64 ? kLanes : 64)) dma_1k(e.xa, x_dst, voff);
        if (kLanes > 64) {
          if (lane < kLanes - 64) dma_1k(e.xa + 1024, x_dst + 1024, voff);
        }
      }
      if (R > 0) {
        const int g = int(e.word >> SW_G_SHIFT) & 7;
        const int nr = p.nride[g];
        const uint64_t al = SEP > 0 ? e.xa : e.xa + 128u * D;
        for (int f = 0; f < nr; ++f)       // (wave-uniform)
          if (lane < 8)
            dma_1k(al + uint64_t(p.ride_delta[g + 1 + f]),
                   x_dst + uint32_t(kXTile + kJC * (1 + f)) * 8u, voff);
      }
    }
  };
  auto prefetch = [&](const StageEnt& e, int buf) {
    const uint32_t a_dst = lds0 + uint32_t(buf) * (kBuf * 8u);
    prefetch_to(e, a_dst, a_dst + kATile * 8u);
  };
  // resident mode: where stage si of the sequence lives (bytes from lds0)
  constexpr uint32_t kXBlk = uint32_t(kXTile + kJC * (1 + R)) * 8u;
  constexpr bool resident = RES;

  // Stage cursors: the stage being multiplied (its entry word in wcur), the stage
  // being prefetched (entry e1, one ahead) and the stage whose entry is being loaded
  // (two ahead: a scalar load issued a whole stage before its use).
  KernFast<D> kf;
  double kdiag;
  int nr_cur = 0;
  auto load_gp = [&](int g) {
    if (SEP == 0) kf.load_const(&p.gps[g].kern);
    kdiag = gpc[g].kern.kdiag;
    if (R > 0) nr_cur = p.nride[g];
  };
  StageEnt e1 = load_stage(stages, 0);
  load_gp(int(e1.word >> SW_G_SHIFT) & 7);
  if (resident) {
#pragma unroll 1
    for (int si = 0; si < nstages; ++si) {
      const StageEnt es = load_stage(stages, si);
      prefetch_to(es, lds0 + es.slot0 * 2048u, lds0 + p.res_xbase + uint32_t(si) * kXBlk);
    }
  } else {
    prefetch(e1, 0);
  }
  if (SEP > 0) {
    sep_offsets(tile);
    sep_fetch(e1);
  }
  uint32_t wcur = e1.word;
  uint32_t s0cur = e1.slot0;           // (resident mode: position 0 / index of the stage
  int sicur = 0;                       //  being multiplied)
  int si1 = nstages > 1 ? 1 : 0;       // index of the stage being prefetched
  if (si1 == 0) tile_p += tstep;
  if (left > 1) e1 = load_stage(stages, si1);
  wait_dma();
  __syncthreads();

  // per-GP state
  double xs[D];
  double ssq_run = 0.0, mean = 0.0;   // folded squares of the GP's finished chunks (per lane)
  double mean_r[R > 0 ? R : 1];      // alpha . k of the riders of the GP being swept
#pragma unroll
  for (int f = 0; f < (R > 0 ? R : 1); ++f) mean_r[f] = 0.0;
  double accx[kMaxNg];              // narrow groups of slot 0 (narrow_groups)
#pragma unroll
  for (int g = 0; g < kMaxNg; ++g) accx[g] = 0.0;
  // per-tile state of the row epilogue
  bool safe = true;
  double l0 = 0.0;
  double lmax = -INFINITY;   // max l0 over the safe rows this wave has seen
  bool gp_start = true;

#ifdef SGP_STAMPS
  unsigned int stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
#endif
  int par = 0;
#pragma unroll 1
  while (true) {
    // the stage's positions and its [rows | alpha] block: the buffer of this parity, or
    // (resident mode) where the stage was copied to at the start
    const uint32_t a_off = resident ? s0cur * 2048u : uint32_t(par) * (kBuf * 8u);
    const uint32_t x_off = resident ? p.res_xbase + uint32_t(sicur) * kXBlk
                                    : a_off + kATile * 8u;
    double* cbuf = lds + (a_off >> 3);

    // SEP: the covariances of THIS stage from the factors fetched a stage ago (their
    // registers take the next stage's right below)
    double kv[4];
    if (SEP > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        kv[q] = efn[0][q];
#pragma unroll
        for (int a = 1; a < kAx; ++a) kv[q] *= efn[a][q];
      }
      // (... BEFORE the next stage's factors are requested: loads complete in order, so a
      // wait for these values placed behind the new requests would sit out THEIR latency)
      asm volatile("" : "+v"(kv[0]), "+v"(kv[1]), "+v"(kv[2]), "+v"(kv[3]));
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- prefetch: the stage after this one (possibly of the next tile)
    const bool more = left > 1;
    const uint32_t wnext = e1.word;
    const uint32_t s0next = e1.slot0;
    if (more) {
      if (!kDmaLate && !resident && !SGP_ABL(2)) prefetch(e1, par ^ 1);
      const bool next_tile = si1 == 0;
      if (SEP == 0) {
        if constexpr (!kLeanX) {
          if (next_tile) load_x(tile_p, xnext);
        }
      } else {
        if (next_tile) sep_offsets(tile_p);
        sep_fetch(e1);
      }
    }
    // the entry after that: loaded now, first used at the top of the next stage
    int si2 = si1 + 1;
    if (si2 == nstages) {
      si2 = 0;
      tile_p += tstep;
    }
    StageEnt e2 = e1;
    if (left > 2) e2 = load_stage(stages, si2);

    SGP_STAMP(0);   // prefetch issue, table entry
    // ---- this stage: 16 training points against the active row blocks
    if (SEP == 0 && gp_start) {
      if constexpr (kLeanX) {
        double xr[D];
        load_x(tile, xr);
        kf.template prep_t<SINGLE>(xr, xs);
      } else {
        kf.template prep_t<SINGLE>(x, xs);
      }
      gp_start = false;
    }
    const double* xT = lds + (x_off >> 3);
    const double* alT = xT + kXTile;
    // A operands of the narrow groups (position 0 of the staged chunk), read FIRST in
    // the stage: they arrive under the evaluation.  (All kMaxNg groups whether the GP
    // has them or not: the reads stay inside the slot.)
    const int ngrp = (wcur & SW_NARROW) ? int(wcur >> SW_NGRP_SHIFT) & 3 : 0;
    // the full slots of this stage (sweep_slots.h): the operands of the first one are
    // requested now
    const int nfull = int(wcur & SW_NACT_MASK) - (ngrp > 0 ? 1 : 0);
    const uint32_t abase = lds0 + a_off + uint32_t(lane) * 8u +
                           (ngrp > 0 ? kSteps * 512u : 0u);
    SgpEntryOps entry;
    if (kEntryEarly && nfull > 0 && !SGP_ABL(8))
      sgp_slots_prefetch(nfull, cbuf + lane + (ngrp > 0 ? kSteps * 64 : 0), entry);
    double an[kMaxNg][4];
    auto load_an = [&]() {
      const double* aN = cbuf + (lane & 0x33);
#pragma unroll
      for (int g = 0; g < kMaxNg; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) an[g][q] = aN[q * 64 + 4 * g];
      }
    };
    if (kAnEarly && ngrp > 0 && !SGP_ABL(8)) load_an();
    if (SEP > 0) {
      // (done at the top of the stage)
    } else if (!SGP_ABL(4)) {
      kf.template many4_t<SINGLE>(xs, xT + (lane >> 4) * D, 4 * D, tab, kv);
    } else {
      kv[0] = xs[0]; kv[1] = xs[0] + 1.0; kv[2] = xs[0] + 2.0; kv[3] = xs[0] + 3.0;
    }
    if (wcur & SW_MEAN) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        mean = fma(alT[q * 4 + (lane >> 4)], kv[q], mean);
      if (R > 0) {
#pragma unroll
        for (int f = 0; f < R; ++f) {
          if (f < nr_cur) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              mean_r[f] = fma(alT[kJC * (1 + f) + q * 4 + (lane >> 4)], kv[q], mean_r[f]);
          }
        }
      }
    }
    // the narrow groups of the last row block (position 0 of the staged chunk): they
    // need kv only -- issued in front of the LDS transpose, whose round trip passes
    // under them
    SGP_STAMP(1);   // covariance evaluation (+ alpha . k)
    if (ngrp > 0 && !SGP_ABL(8)) {
      if (!kAnEarly) load_an();
      narrow_groups(ngrp, accx, an, kv);
    }
    SGP_STAMP(2);   // narrow groups
    double kb[4][4];
    if (!SGP_ABL(8)) broadcast_quads<L::kKbRow>(kv, kbw, lane, kb);
#ifdef SGP_STAMPS
    asm volatile("" : "+v"(kb[0][0]), "+v"(kb[1][0]), "+v"(kb[2][0]), "+v"(kb[3][0]));
    asm volatile("" : "+v"(kb[0][3]), "+v"(kb[1][3]), "+v"(kb[2][3]), "+v"(kb[3][3]));
#endif
    SGP_STAMP(3);   // LDS transpose round trip
    if (kDmaLate && more && !resident && !SGP_ABL(2)) prefetch(e1, par ^ 1);
    if (!SGP_ABL(8)) {
      // the full slots: sweep_slots.h (hand-written, accumulators in a0..a127)
      if (!kEntryEarly && nfull > 0)
        sgp_slots_prefetch(nfull, cbuf + lane + (ngrp > 0 ? kSteps * 64 : 0), entry);
      if (nfull > 0) sgp_slots(nfull, int(wcur & SW_FIRST), abase, kb, entry);
    }

    SGP_STAMP(4);   // full slots
    if (wcur & SW_CHUNK_END) {
      // squares of the chunk's accumulators, folded at once to this lane's share of
      // |L^-1 k|^2 for its point (lane l: point l & 15): ONE register survives the chunk
      // (the chunk's slots: what its LAST stage -- this one -- has active is the
      // diagonal block only; the table carries the chunk's slot count)
      double sq[4] = {0.0, 0.0, 0.0, 0.0};
      const int nsl = (int(wcur >> SW_NSL_SHIFT) & 31) - (ngrp > 0 ? 1 : 0);
      if (nsl > 0 && !SGP_ABL(8)) sgp_fold_slots(nsl, sq);
      // lane 16 i' + 4 blk + j' of sq[m]: the squares for point 4 m + j' of row group
      // blk on the DIAGONAL lanes i' = j' only (cross terms elsewhere)
      if ((lane >> 4) != (lane & 3)) sq[0] = sq[1] = sq[2] = sq[3] = 0.0;
      // sq[m]: partial sums for column 4m + (lane & 3) over this lane's rows.
      // Transposing fold over the lanes that share (lane & 3): after the xor-4
      // and xor-8 exchanges each lane holds the quad of its OWN column
      // (lane & 15) = 4 ((lane >> 2) & 3) + (lane & 3).
      const bool a0 = (lane & 4) != 0, a1 = (lane & 8) != 0;
      // (exchanges by DPP row rotations, the lane-group sums below by permlane swaps --
      // sweep_shared.h: same values in the same order as the ds_bpermute forms, without
      // their LDS round trips on the tile's critical path)
      const double v0 = (a0 ? sq[1] : sq[0]) + take_xor4(a0 ? sq[0] : sq[1], a0);
      const double v1 = (a0 ? sq[3] : sq[2]) + take_xor4(a0 ? sq[2] : sq[3], a0);
      double t = (a1 ? v1 : v0) + take_xor8(a1 ? v0 : v1);
      // (the narrow groups: rows l >> 4 of the group, point l & 15 already)
#pragma unroll
      for (int g = 0; g < kMaxNg; ++g) {
        t = fma(accx[g], accx[g], t);
        accx[g] = 0.0;
      }
      ssq_run += t;
    }

    if ((wcur & SW_GP_END) && !SGP_ABL(32)) {
      // ... then the 4 k-rows
      const double sumsq = sum_lane_groups_valu(ssq_run);
      const double mu = sum_lane_groups_valu(mean);
      ssq_run = 0.0;
      mean = 0.0;

      const int g = int(wcur >> SW_G_SHIFT) & 7;
      const int64_t row = int64_t(tile) * kTilePts + wave * 16 + (lane & 15);
      const bool writer = (row < p.pts.N) && (lane < 16);
      // one GP's posterior at the wave's rows -> mean / var, its interval, the safe
      // set (update_confidence_intervals + compute_safe_set, gp_opt.py:453-481)
      auto emit = [&](int gi, double mu_i, double kdiag_i) {
        const double var = fmax(kdiag_i - sumsq, 1e-15);  // GPy clip
        const double sd = sqrt(var);
        const double lo = mu_i - p.conf.beta * sd;
        const double up = mu_i + p.conf.beta * sd;
        if (gi == 0) l0 = lo;
        safe = safe && (lo > p.conf.fmin[gi]);
        if (writer && !SGP_ABL(16)) {
          // streaming rows in / results out: non-temporal, so that they do not push
          // the L^-1 chunks every workgroup re-reads out of the 4 MB L2 of the XCD
          __builtin_nontemporal_store(mu_i, p.conf.mean + int64_t(gi) * p.pts.N + row);
          __builtin_nontemporal_store(var, p.conf.var + int64_t(gi) * p.pts.N + row);
        }
        // Q row = [l0, u0, l1, u1, ...] (gp_opt.py:375): the intervals of the G
        // passes are collected in the padding of the wave's broadcast buffer
        // and leave as ONE contiguous block per wave at the end of the tile --
        // full 128-byte lines from all 64 lanes instead of 16-byte pieces of a
        // row from 16 lanes per GP
        if (p.conf.Q && lane < 16 && !SGP_ABL(16)) {
          if (p.G <= L::kQMaxG)
            *reinterpret_cast<double2_t*>(kbw + L::qoff(lane * p.G + gi)) =
                double2_t{lo, up};
          else if (writer)
            *reinterpret_cast<double2_t*>(p.conf.Q + (row * p.G + gi) * 2) =
                double2_t{lo, up};
        }
      };
      emit(g, mu, kdiag);
      if (R > 0) {
        // riders: the leader's |L^-1 k|^2, their own alpha . k and prior variance
#pragma unroll
        for (int f = 0; f < R; ++f) {
          if (f < nr_cur) {
            const double mu_f = sum_lane_groups_valu(mean_r[f]);
            mean_r[f] = 0.0;
            emit(g + 1 + f, mu_f, gpc[g + 1 + f].kern.kdiag);
          }
        }
      }

      if (wcur & SW_TILE_END) {
        if (p.conf.Q && p.G <= L::kQMaxG && !SGP_ABL(16)) {
          const int64_t row0 = int64_t(tile) * kTilePts + wave * 16;
          const int64_t rows_left = p.pts.N - row0;
          const int nq = (rows_left >= 16 ? 16 : (rows_left > 0 ? int(rows_left) : 0)) * p.G;
          __builtin_amdgcn_wave_barrier();
          double2_t* dst = reinterpret_cast<double2_t*>(p.conf.Q) + row0 * p.G;
          for (int i = lane; i < nq; i += 64)
            __builtin_nontemporal_store(
                *reinterpret_cast<const double2_t*>(kbw + L::qoff(i)), dst + i);
          __builtin_amdgcn_wave_barrier();
        }
        if (p.conf.S) {
          if (writer) p.conf.S[row] = safe ? 1 : 0;
          // running maximum of l0 over the safe rows (folded over the wave and
          // written once, when the wave has walked all its tiles)
          lmax = fmax(lmax, (writer && safe) ? l0 : -INFINITY);
        }
        safe = true;
        l0 = 0.0;
        if constexpr (!kLeanX) {
#pragma unroll
          for (int k = 0; k < D; ++k) x[k] = xnext[k];
        }
        tile += tstep;
      }
      if (more) {   // hyper-parameters of the next GP
        const int g_n = int(wnext >> SW_G_SHIFT) & 7;
        if (g_n != g || R > 0) load_gp(g_n);
      }
      gp_start = true;
    }

    SGP_STAMP(5);   // chunk fold, row epilogue
    if (!more) break;
    if (!resident) {
      wait_dma();       // (asm copies: the compiler does not count them)
      SGP_STAMP(6);   // wait for this wave's LDS-DMA
      if (!SGP_ABL(1)) __syncthreads();
      SGP_STAMP(7);   // barrier
    }
    par ^= 1;
    wcur = wnext;
    s0cur = s0next;
    sicur = si1;
    e1 = e2;
    si1 = si2;
    --left;
  }
#ifdef SGP_STAMPS
  if (lane == 0) {
    unsigned long long* o = p.stamps + (size_t(blockIdx.x) * kNW + wave) * 8;
    for (int i = 0; i < 8; ++i) o[i] = stamp_acc[i];
  }
#endif
  if (p.conf.S) {
    lmax = wave_max(lmax);
    if (lane == 0) p.conf.partial[int(blockIdx.x) * kNW + wave] = lmax;
  }
}


// ---- launch -----------------------------------------------------------------------
// The stage sequence of one tile: for every GP, for every chunk of 16 row blocks
// of L^-1, the j-blocks 0 .. bend-1 (only the slots at or below the diagonal are
// active).  Depends on the block counts only, so it is rebuilt (and uploaded)
// when a GP crosses a multiple of 16 training points, not per launch.
// Narrow 4-row groups the last row block of a GP is taken as (0: a full block).
// SGP_NO_NARROW=1: never (A/B runs); =2: only the one-group form of round 3.
int narrow_groups_of(const GpDev& gp) {
  static const int mode = getenv("SGP_NO_NARROW") ? atoi(getenv("SGP_NO_NARROW")) : 0;
  const int ng = (gp.last_rows + 3) / 4;
  if (mode == 1 || ng > kMaxNg) return 0;
  if (mode == 2 && ng > 1) return 0;
  return ng;
}

int stage_table(sgp_ctx* ctx, const GpDev* gh, int Geff, int d, bool sep, int kIB,
                const bool* rides, const StageEnt** dev, int* nstages) {
  // (entries hold absolute addresses: rebuilt when a block count OR a buffer address
  // changes; the buffers are sized for the pitch of L^-1, so one-row appends keep them)
  std::vector<uint64_t> sig(1, uint64_t(Geff));
  sig.push_back(uint64_t(kIB) | (uint64_t(d) << 8) | (uint64_t(sep) << 16));
  int last_staged = 0;
  for (int g = 0; g < Geff; ++g) {
    sig.push_back(uint64_t(gh[g].nblk));
    sig.push_back(uint64_t(narrow_groups_of(gh[g])) | (uint64_t(rides[g]) << 2));
    sig.push_back(reinterpret_cast<uint64_t>(gh[g].Apack));
    sig.push_back(reinterpret_cast<uint64_t>(gh[g].XA));
    if (!rides[g]) last_staged = g;
  }
  if (sig == ctx->stage_sig && ctx->stage_tab.p) {
    *dev = static_cast<const StageEnt*>(ctx->stage_tab.p);
    *nstages = ctx->stage_count;
    return 0;
  }
  std::vector<StageEnt> tab;
  const uint64_t xa_block = uint64_t(16 * d + 16) * sizeof(double);
  uint32_t slots_total = 0;       // 2-KB positions of all stages (resident mode)
  for (int g = 0; g < Geff; ++g) {
    if (rides[g]) continue;       // (its alpha . k is formed in its leader's stages)
    const int nblk = gh[g].nblk, nsteps = gh[g].n_pad / 4;
    const int nchunks = (nblk + kIB - 1) / kIB;
    const uint64_t apack = reinterpret_cast<uint64_t>(gh[g].Apack);
    const uint64_t xa = reinterpret_cast<uint64_t>(gh[g].XA) + (sep ? 128u * uint64_t(d) : 0u);
    for (int c = 0; c < nchunks; ++c) {
      const int b0 = c * kIB, nib = std::min(kIB, nblk - b0), bend = b0 + nib;
      for (int jb = 0; jb < bend; ++jb) {
        StageEnt e{};
        e.a_src = apack + (uint64_t(bend - 1) * nsteps + 4 * uint64_t(jb)) * 512;
        e.xa = xa + uint64_t(jb) * xa_block;
        e.rs_bytes = uint32_t(nsteps) * 512u;
        e.jb = uint32_t(jb);
        e.word = uint32_t(std::min(nib, bend - jb)) | (uint32_t(g) << SW_G_SHIFT);
        e.slot0 = slots_total;
        slots_total += uint32_t(std::min(nib, bend - jb));
        if (jb == 0) e.word |= SW_FIRST;
        e.word |= uint32_t(nib) << SW_NSL_SHIFT;
        if (jb == bend - 1) e.word |= SW_CHUNK_END;
        if (c == nchunks - 1) e.word |= SW_MEAN;
        // slot 0 of the last chunk = the last row block
        if (c == nchunks - 1 && narrow_groups_of(gh[g]) > 0)
          e.word |= SW_NARROW | (uint32_t(narrow_groups_of(gh[g])) << SW_NGRP_SHIFT);
        if (c == nchunks - 1 && jb == bend - 1) {
          e.word |= SW_GP_END;
          if (g == last_staged) e.word |= SW_TILE_END;
        }
        tab.push_back(e);
      }
    }
  }
  SGP_TRY(sgp_reserve(ctx, &ctx->stage_tab, tab.size() * sizeof(StageEnt)));
  SGP_TRY(sgp_h2d(ctx, ctx->stage_tab.p, tab.data(), tab.size() * sizeof(StageEnt)));
  ctx->stage_sig = sig;
  ctx->stage_count = int(tab.size());
  ctx->stage_slots = int(slots_total);
  *dev = static_cast<const StageEnt*>(ctx->stage_tab.p);
  *nstages = ctx->stage_count;
  return 0;
}

// persistent: as many workgroups as are resident at once (256 VGPRs per thread
// -> 8 waves per CU) walk over the tiles
int sweep_grid_blocks(int num_cu, int64_t N) {
  const int64_t ntiles = (N + 16 * kNW - 1) / (16 * kNW);
  const int64_t resident = int64_t(num_cu) * (8 / kNW);
  return int(ntiles < resident ? ntiles : resident);
}

template <int D, bool SINGLE, int R = 0, int SEP = 0>
int launch_sweep_v(sgp_ctx* ctx, const SweepParams& p, double flops) {
  static bool attr_set = false;
  if (!attr_set) {
    SGP_HIP(ctx, hipFuncSetAttribute(
                     reinterpret_cast<const void*>(&k_sweep<D, SINGLE, R, SEP, false>),
                     hipFuncAttributeMaxDynamicSharedMemorySize,
                     int(Lay<D, R>::bytes())));
    SGP_HIP(ctx, hipFuncSetAttribute(
                     reinterpret_cast<const void*>(&k_sweep<D, SINGLE, R, SEP, true>),
                     hipFuncAttributeMaxDynamicSharedMemorySize,
                     int(Lay<D, R>::bytes())));
    attr_set = true;
  }
  const int nblocks = sweep_grid_blocks(ctx->num_cu, p.pts.N);
  SweepTimer timer;
  SGP_TRY(timer.begin(ctx, flops));
  SweepParams pp = p;
  {
    // small factors: every stage's positions stay in LDS for the whole launch
    // (SGP_NO_RESIDENT=1 / sgp_ctx_set_sweep(+ 16): stream them, A/B runs)
    typedef Lay<D, R> L;
    static const bool off = getenv("SGP_NO_RESIDENT") != nullptr;
    const size_t xblk = size_t(L::kXTile + kJC * (1 + R)) * 8;
    const size_t need = size_t(ctx->stage_slots) * 2048 + size_t(p.nstages) * xblk;
    pp.resident = (!off && !(ctx->sweep_choice & 16) && need <= size_t(2 * L::kBuf) * 8) ? 1 : 0;
    pp.res_xbase = unsigned(ctx->stage_slots) * 2048u;
  }
#ifdef SGP_INSTRUMENT
  static const int ablate = getenv("SGP_ABLATE") ? atoi(getenv("SGP_ABLATE")) : 0;
  pp.ablate = ablate;
#endif
  const size_t lds_bytes = Lay<D, R>::bytes();
#ifdef SGP_STAMPS
  static unsigned long long* stamps_dev = nullptr;
  if (!stamps_dev) SGP_HIP(ctx, hipMalloc(&stamps_dev, size_t(4096) * kNW * 8 * 8));
  pp.stamps = stamps_dev;
#endif
  if (pp.resident)
    hipLaunchKernelGGL((k_sweep<D, SINGLE, R, SEP, true>), dim3(nblocks),
                       dim3(64 * kNW), lds_bytes, ctx->stream, pp);
  else
    hipLaunchKernelGGL((k_sweep<D, SINGLE, R, SEP, false>), dim3(nblocks),
                       dim3(64 * kNW), lds_bytes, ctx->stream, pp);
  SGP_HIP(ctx, hipGetLastError());
#ifdef SGP_STAMPS
  {
    std::vector<unsigned long long> h(size_t(nblocks) * kNW * 8);
    SGP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SGP_HIP(ctx, hipMemcpy(h.data(), stamps_dev, h.size() * 8, hipMemcpyDeviceToHost));
    static const char* names[8] = {"prefetch", "evaluate", "narrow", "transpose", "slots",
                                   "fold+epilogue", "dma-wait", "barrier"};
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tot = 0;
    for (size_t w = 0; w < size_t(nblocks) * kNW; ++w)
      for (int i = 0; i < 8; ++i) sum[i] += double(h[w * 8 + i]);
    for (int i = 0; i < 8; ++i) tot += sum[i];
    fprintf(stderr, "stamps (ticks per wave, %% of loop):");
    for (int i = 0; i < 8; ++i)
      fprintf(stderr, "  %s %.0f (%.1f%%)", names[i], sum[i] / (double(kNW) * nblocks),
              100.0 * sum[i] / tot);
    fprintf(stderr, "  | loop %.0f\n", tot / (double(kNW) * nblocks));
  }
#endif
  return timer.end(ctx);
}

// the instance of an input dimension: with riders, one-part kernels, products
template <int D>
int launch_sweep_d(sgp_ctx* ctx, const SweepParams& p, double flops) {
  if constexpr (D <= 3) {       // (the d = 4 instance with riders would spill)
    bool riders = false;
    for (int g = 0; g < SGP_MAX_GPS; ++g) riders = riders || p.nride[g] > 0;
    if (riders) return launch_sweep_v<D, true, kSweepRide>(ctx, p, flops);
  }
  return p.single ? launch_sweep_v<D, true>(ctx, p, flops)
                  : launch_sweep_v<D, false>(ctx, p, flops);
}

// tensor grid + RBF kernels: the instances that read factor tables (SEP axes; D = 1:
// they do not read the rows).  Riders as in the generic instances.
template <int SEP>
int launch_sweep_sep(sgp_ctx* ctx, const SweepParams& p, double flops) {
  bool riders = false;
  for (int g = 0; g < SGP_MAX_GPS; ++g) riders = riders || p.nride[g] > 0;
  if (riders) return launch_sweep_v<1, true, kSweepRide, SEP>(ctx, p, flops);
  return launch_sweep_v<1, true, 0, SEP>(ctx, p, flops);
}

int launch_posterior(sgp_ctx* ctx, const SweepArgs& a, const GpDev* gh, int d, int Geff,
                     double flops, const SepLaunch* sep, bool rows_sharded, int64_t sel_rows);

// fit: a swarm-fitness call (null: a confidence sweep into a.conf).
// rows_sharded: the rows are a rank's shard of a grid (sgp_grid_*) -- the kernel is then
// chosen by the GPs alone, never by the number of rows (same kernel on every rank).
// sel_rows >= 0: the kernel is chosen as for that many rows (a rank's block of a sharded
// swarm: the kernel of the whole swarm, sgp_swarm_run_shard)
int launch_sweep(sgp_ctx* ctx, const SweepArgs& a, const GpDev* gh, int d,
                 const FitnessArgs* fit = nullptr, const SepLaunch* sep = nullptr,
                 bool rows_sharded = false, int64_t sel_rows = -1) {
  // algorithmic flops: G * (n^2 + 2n) per row
  double flops = 0.0;
  const int Geff = (fit && fit->swarm_type == SGP_SWARM_GREEDY) ? 1 : a.G;
  for (int g = 0; g < Geff; ++g)
    flops += (double(gh[g].n) * gh[g].n + 2.0 * gh[g].n) * double(a.pts.N);
  if (a.pts.N <= 0) return 0;
  SweepArgs q = a;
  if (fit) {
    // SafeOptSwarm._compute_particle_fitness (gp_opt.py:901-1013) = the posterior of
    // the swarm's GPs (the sweep, mean / var only) + the shaping of fitness.h on
    // those (k_fitness_small: one thread per particle).  The particles are few next
    // to a grid: the 16 bytes per (GP, particle) in between cost nothing, and the
    // sweep kernels need no second set of instances (which spilled registers).
    const size_t np = size_t(Geff) * size_t(a.pts.N);
    SGP_TRY(sgp_reserve(ctx, &ctx->pair_post, 2 * np * sizeof(double)));
    q.conf = ConfOut{};
    q.conf.mean = static_cast<double*>(ctx->pair_post.p);
    q.conf.var = q.conf.mean + np;
    q.G = Geff;
    for (int i = 0; i < SGP_MAX_GPS; ++i) q.conf.fmin[i] = -INFINITY;
  }
  int rc = launch_posterior(ctx, q, gh, d, Geff, flops, sep, rows_sharded, sel_rows);
  if (rc != 0 || !fit) return rc;
  return launch_fitness_small(ctx, a.G, a.pts.N, q.conf.mean, q.conf.var, *fit);
}

// The confidence sweep proper: the paired-wave kernel from 257 rows of L^-1 on, the 4-wave
// kernel below, the resident-factor kernel (sweep_mid.hip) for 49 .. 128 observations of
// single-part kernels, the VALU kernel (sweep_tiny.hip) up to 48 observations.
int launch_posterior(sgp_ctx* ctx, const SweepArgs& a, const GpDev* gh, int d, int Geff,
                     double flops, const SepLaunch* sep, bool rows_sharded, int64_t sel_rows) {
  if (tiny_sweep_wanted(ctx, gh, Geff, sel_rows >= 0 ? sel_rows : a.pts.N, rows_sharded)) {
    ctx->last_sweep = 3;
    return launch_sweep_tiny(ctx, a, gh, d, Geff, flops);    // (sets ctx->sweep_partials)
  }
  if (mid_sweep_wanted(ctx, gh, Geff, d) || mid_passes_wanted(ctx, gh, Geff, sep, a.conf)) {
    ctx->last_sweep = 6;
    return launch_sweep_mid(ctx, a, gh, d, Geff, flops, sep);   // (sets ctx->sweep_partials)
  }
  if (pair_sweep_wanted(ctx, gh, Geff)) {
    ctx->last_sweep = 2;
    return launch_sweep_pair(ctx, a, gh, d, Geff, flops, sep);   // (sets ctx->sweep_partials)
  }
  ctx->last_sweep = 1;
  ctx->sweep_partials = sweep_grid_blocks(ctx->num_cu, a.pts.N) * kNW;
  SweepParams q{};
  q.gps = a.gps;
  q.G = a.G;
  q.pts = a.pts;
  q.conf = a.conf;
  q.single = 1;
  for (int g = 0; g < Geff; ++g) q.single = q.single && gh[g].kern.n_parts == 1;
  // followers of a shared factor ride in their leader's stages (sweep_shared.h)
  // (tensor-grid instances: one set of tables per leader, whatever the input dimension)
  bool rides[SGP_MAX_GPS];
  assign_riders(gh, Geff, sep ? 1 : d, q.single != 0 || sep != nullptr, kSweepRide, 3, rides,
                q.nride, q.ride_delta);
  SGP_TRY(stage_table(ctx, gh, Geff, d, sep != nullptr, kSL, rides, &q.stages, &q.nstages));
  if (sep) {
    q.sep = *sep;
    switch (sep->naxes) {
      case 1: return launch_sweep_sep<1>(ctx, q, flops);
      case 2: return launch_sweep_sep<2>(ctx, q, flops);
      case 3: return launch_sweep_sep<3>(ctx, q, flops);
      // (4 axes: 32 registers of factors in flight -- the instance would spill; the
      // covariances are evaluated, below)
    }
  }
  switch (d) {
    case 1: return launch_sweep_d<1>(ctx, q, flops);
    case 2: return launch_sweep_d<2>(ctx, q, flops);
    case 3: return launch_sweep_d<3>(ctx, q, flops);
    case 4: return launch_sweep_d<4>(ctx, q, flops);
    case 5: return launch_sweep_d<5>(ctx, q, flops);
    case 6: return launch_sweep_d<6>(ctx, q, flops);
    case 7: return launch_sweep_d<7>(ctx, q, flops);
    case 8: return launch_sweep_d<8>(ctx, q, flops);
  }
  sgp_set_error(ctx, "input dimension %d not in 1..%d", d, SGP_MAX_D);
  return -2;
}

}  // namespace

int launch_sweep_conf(sgp_ctx* ctx, const GpDev* gps_dev, const GpDev* gps_host,
                      int G, int d, SweepPoints pts, ConfOut out, const SepLaunch* sep,
                      bool rows_sharded) {
  return launch_sweep(ctx, SweepArgs{gps_dev, G, pts, out}, gps_host, d, nullptr, sep,
                      rows_sharded);
}

int launch_sweep_fitness(sgp_ctx* ctx, const GpDev* gps_dev,
                         const GpDev* gps_host, int G, int d, SweepPoints pts,
                         FitnessArgs fa, int64_t sel_rows) {
  return launch_sweep(ctx, SweepArgs{gps_dev, G, pts, ConfOut{}}, gps_host, d, &fa, nullptr,
                      false, sel_rows);
}


// ---- tensor grids: per-axis factor tables (SepLaunch) -------------------------------
// E_a[jb][i][4 k4 + q] = 2^(-W_k (axis_k[i] - X_{j k})^2 / 32), k = column of axis a,
// j = 16 jb + 4 q + k4, W_k = sum over the parts of their squared weights on column k
// (KernDesc::wsq: the exponents of RBF parts add).  Axis 0's table also carries the
// product of the variances and the factors of the constant columns (contexts).
struct SepCols {
  int naxes, d;
  int cols[4];
  uint32_t count[SGP_MAX_D];
  int off[SGP_MAX_D];
};
__global__ __launch_bounds__(256) void k_sep_table(GpDev gp, SepCols sc, int a,
                                                   const double* vals, double* out) {
  const int k = sc.cols[a];
  const uint32_t count = sc.count[k];
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t total = int64_t(gp.nblk > kSepMinBlocks ? gp.nblk : kSepMinBlocks) * count * 16;
  if (e >= total) return;
  const int pos = int(e & 15);
  const uint32_t i = uint32_t((e >> 4) % count);
  const int jb = int((e >> 4) / count);
  const int j = 16 * jb + 4 * (pos & 3) + (pos >> 2);
  if (jb >= gp.nblk) {            // (beyond the GP's own blocks: see kSepMinBlocks)
    out[e] = 0.0;
    return;
  }
  const double* xj = gp.Xpad + int64_t(j) * sc.d;
  auto weight = [&](int col) {
    double W = 0.0;
    for (int p = 0; p < gp.kern.n_parts; ++p) W += gp.kern.wsq[p][col];
    return W;
  };
  double dx = vals[sc.off[k] + i] - xj[k];
  double u = weight(k) * dx * dx;
  double scale = 1.0;
  if (a == 0) {
    scale = gp.kern.kdiag;
    for (int c = 0; c < sc.d; ++c) {
      if (sc.count[c] != 1) continue;
      dx = vals[sc.off[c]] - xj[c];
      u += weight(c) * dx * dx;
    }
  }
  out[e] = scale * exp2(-u * (1.0 / 32.0));
}

size_t sep_table_doubles(const GpDev& gp, uint32_t count) {
  return size_t(std::max(gp.nblk, kSepMinBlocks)) * count * 16;
}

int launch_sep_tables(sgp_ctx* ctx, const GpDev& gp, int d, const uint32_t* count,
                      const double* axis_vals, const int* axis_off, int naxes,
                      const int* cols, double* const* out) {
  SepCols sc{};
  sc.naxes = naxes;
  sc.d = d;
  for (int a = 0; a < naxes; ++a) sc.cols[a] = cols[a];
  for (int k = 0; k < d; ++k) {
    sc.count[k] = count[k];
    sc.off[k] = axis_off[k];
  }
  for (int a = 0; a < naxes; ++a) {
    const int64_t total = int64_t(sep_table_doubles(gp, count[cols[a]]));
    hipLaunchKernelGGL(k_sep_table, dim3(unsigned((total + 255) / 256)), dim3(256), 0,
                       ctx->stream, gp, sc, a, axis_vals, out[a]);
  }
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}

// rows of the grid against the declared axes, bit for bit
__global__ __launch_bounds__(256) void k_verify_axes(const double* pts, int64_t N, int d,
                                                     int64_t goff, const double* vals,
                                                     const uint32_t* meta, int* mismatch) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= N) return;
  const uint32_t gi = uint32_t(goff + i);
  int bad = 0;
  for (int k = 0; k < d; ++k) {
    const uint32_t cnt = meta[3 * k], str = meta[3 * k + 1], off = meta[3 * k + 2];
    const double want = vals[off + (gi / str) % cnt];
    bad |= __double_as_longlong(want) != __double_as_longlong(pts[int64_t(k) * N + i]);
  }
  if (bad) atomicAdd(mismatch, 1);
}

int launch_verify_axes(sgp_grid* g, int* mismatch_dev) {
  sgp_ctx* ctx = g->ctx;
  uint32_t meta[3 * SGP_MAX_D];
  for (int k = 0; k < g->d; ++k) {
    meta[3 * k] = g->ax_count[k];
    meta[3 * k + 1] = g->ax_stride[k];
    meta[3 * k + 2] = uint32_t(g->ax_off[k]);
  }
  uint32_t* meta_dev = reinterpret_cast<uint32_t*>(mismatch_dev + 4);   // (same scratch slot)
  SGP_TRY(sgp_h2d(ctx, meta_dev, meta, sizeof(uint32_t) * 3 * g->d));
  hipLaunchKernelGGL(k_verify_axes, dim3(unsigned((g->N + 255) / 256)), dim3(256), 0,
                     ctx->stream, g->pts, g->N, g->d, g->goff,
                     static_cast<const double*>(g->ax_vals.p), meta_dev, mismatch_dev);
  SGP_HIP(ctx, hipGetLastError());
  return 0;
}
