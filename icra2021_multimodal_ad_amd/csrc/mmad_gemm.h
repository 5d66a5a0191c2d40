// Internal GEMM interface (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "mmad_common.h"

// split-K control block: per-launch arrival counters + flags use fewer than
// MMAD_SK_ERR_WORD words (mmad_gemm_splitk checks); this word records a combine that timed out (sticky until read
// by mmad_gemm_status / mmad_ae_status)
#define MMAD_SK_ERR_WORD 8191
#define MMAD_SK_SLAB_TILES 832

enum GemmEpiKind {
  GEMM_EPI_FWD = 0,         // y = BNaffine(act(acc + bias)); optional Welford partials
  GEMM_EPI_MSE = 1,         // dz = gscale*(acc + bias - target); partials (sum dz, sum d^2)
  GEMM_EPI_BWD_DATA = 2,    // dx = acc; optional column-sum partials
  GEMM_EPI_BWD_WEIGHT = 3,  // dW = acc (fp32 out)
  GEMM_EPI_SCORE = 4,       // as FWD (eval) + row-sum of (y - ref)^2, optional diff out
};

struct GemmEpi {
  int M, N;              // valid rows / cols of the output
  void* out;             // output, ld = ldo elements
  int ldo;
  const float* bias;     // [Np]
  int act;
  float slope;
  const float* bn_scale; // eval-mode BN affine (nullable)
  const float* bn_shift;
  float* part;           // partials [Mp/32][2][ldpart]
  int ldpart;
  const float* target;   // MSE target (fp32 user input), ld = ldt
  int ldt;
  int tmod;              // MSE target row = row % tmod (k-expanded VIB decoder)
  float gscale;          // MSE gradient scale (2 for sum-MSE, 2/k for VIB)
  const void* ref;       // SCORE reference activations (same dtype as out)
  int ldref;
  float* rowsq;          // SCORE row partials [Np/128][ldrow]: sum_j colw[j]*(y-ref)^2
  const float* colw;     // SCORE per-column weights (nullable = 1); ref nullable = 0
  int ldrow;
  float* diff;           // SCORE optional fp32 diff output
  int lddiff;
  // MMAD_BF16X3 (mmad_gemm_x3.hip) only; ignored by the other dtypes' kernels.
  // out32 (nullable): an fp32 copy of y, [Mp][ld32].  a_lo / b_lo (nullable):
  // the operands' lo planes where they do not follow the hi plane at
  // +rows*ld elements (the executor's weight planes are [2][n_weight]).
  // out is the hi plane [Mp][ldo], its lo plane follows at +Mp*ldo; ref is fp32.
  float* out32;
  int ld32;
  const void* a_lo;
  const void* b_lo;
  // FWD/MSE: folded train-mode BN of the producer: bias += sum_p bpart[p][n]
  const float* bpart;    // [bparts][bpstride] (nullable)
  int bparts, bpstride;
  // BWD_WEIGHT on a train-mode BN producer's raw activation a (x = a*s + t):
  // dW = b_scale[k] * (dz^T a) + b_shift[k] * db[n], db[n] = sum_p gb_src[p][n]
  const float* b_scale;  // indexed by k (nullable)
  const float* b_shift;
  const float* gb_src;
  int gb_parts, gb_stride;
  // BWD_DATA: BatchNorm-backward column partials of the produced dy
  const void* bn_a;      // pre-BN activation, same shape/ld as out (nullable)
  const float* bn_mean;
  const float* bn_rstd;
  double* bn_part;       // [Mp/64][2][ldo]: (sum dy, sum dy*xhat), fp64
  // MSE: one loss partial (sum d^2) per output tile, [mmad_gemm_ntiles(plan)]
  float* lossp;
  // BWD_WEIGHT: torch.optim.Adam step fused into the epilogue (nullable p).
  // Weight tile: p/m/v share the dW layout (ld = ldo); shadow gets bf16(p).
  float* ad_p;
  float* ad_m;
  float* ad_v;
  void* ad_shadow;
  float ad_w1, ad_w2, ad_eps, ad_step, ad_bc2;   // Adam: w = float(1 - beta) (mmad_adam_consts)
  int dw_nostore;        // with ad_p: do not materialise dW (Adam consumed it)
  // ... and the layer's small segment [bias | gamma | beta], spread over all
  // blocks; the first bNp elements take g = sum of bias partials.
  float* sm_p;
  float* sm_g;
  float* sm_m;
  float* sm_v;
  int sm_n;
  int sm_bN, sm_bNp;     // bias entries (valid / padded); their g = db from gb_src
  // split-K (nullable = off): fp32 partial-tile slabs and the per-tile
  // arrival counter + flag words (zero before a launch; every launch leaves
  // them zero).  Sizes: mmad_gemm_splitk_bytes.  The split factor itself is
  // a deterministic function of the shape (mmad_gemm_splitk).
  float* sk_slab;
  unsigned* sk_ctl;
  // set by the launcher: split factor, XCD-aware grouped tile order
  int splitk;
  int tiles_n, group_m;
  int persist_tiles;   // persistent grid (knob 12): every block loops over these tiles
  int tile_force;        // caller's tile choice + 1 (0 = none; ignored if it does not fit)
  // graph-captured step (nullable): MSE target = dyn->x, Adam step terms
  // from dyn (see MmadDyn)
  const MmadDyn* dyn;
  // Train-mode BatchNorm fused into the producing GEMM (bn_sync != null):
  // the tiles_m blocks of one output column tile publish their column
  // partials (sc1 stores), meet at a counter barrier (bn_sync[tn] arrivals,
  // reset by the last arriver, which bumps the generation word
  // bn_sync[MMAD_BN_EXIT + tn] the others poll; zero before the first launch)
  // and each finishes the whole-batch statistics for its columns itself.
  // Needs every block of the grid co-resident (mmad_gemm_bn_fusable), S = 1.
  //  FWD: part = Welford partials; writes out = a (pre-BN activation) and
  //       bn_y = BN(a) = a*scale + shift; the tm == 0 blocks write
  //       bn_save_mean/rstd and update the running statistics (nullable).
  //  BWD_DATA: bn_part = fp64 (sum dy, sum dy*xhat) per 64 rows; writes
  //       bn_dz = act'(a) * dBN(dy) (out unused), bn_dbpart = per-64-row
  //       column sums of dz, and (tm == 0) bn_dgamma / bn_dbeta.
  unsigned* bn_sync;
  unsigned* bn_err;      // sticky timeout word (barrier never completed)
  const float* bn_gamma;
  const float* bn_beta;
  float* bn_rmean;
  float* bn_rvar;
  float bn_mom, bn_eps;
  float* bn_save_mean;
  float* bn_save_rstd;
  void* bn_y;
  void* bn_dz;
  float* bn_dgamma;
  float* bn_dbeta;
  float* bn_dbpart;
  int bn_act;            // BWD_DATA: the BN producer's activation (act' from a)
  int dbg;               // diagnostics (tools/gemm_phase): 1 skip main loop, 2 skip epilogue,
                         // 4 force the split-K combine's timeout path (tests),
                         // 8 skip the FWD Welford partial stores
  // host only (nullable): an event completed by the launch itself
  // (hipExtLaunchKernel's stop event) instead of a separate hipEventRecord
  // behind it, whose marker packet holds the stream's next dispatch
  hipEvent_t done_ev;
  // host only (nullable): an event that takes the launch's start time
  // (hipExtLaunchKernel's start event; the executor's in-step kernel probe)
  hipEvent_t start_ev;
  // MMAD_BF16X3 SCORE only (nullable pair; last, so no other field moves): the
  // fp32 diff d = y - ref written as split planes, hi = bf16(d), lo =
  // bf16(d - hi), element (row, col) at dp_hi / dp_lo + row * lddp + dp_col +
  // col.  Valid rows / columns only; lddp and dp_col are arbitrary (a layer's
  // slot inside a concatenated operand may start at an odd column), so the
  // stores are scalar, as the fp32 diff's are.
  void* dp_hi;
  void* dp_lo;
  int lddp, dp_col;
};

// The slots of the tune table (include/mmad.h; mmad_tune_set), spelled after
// their _native.KNOB keys.  The numbers are the public ones and never move.
enum MmadKnob {
  KNOB_TILE = 0,
  KNOB_GROUP_M = 1,
  KNOB_AUTOTUNE = 2,
  KNOB_DBG = 3,
  KNOB_SPLITK = 4,
  KNOB_TILE_ADAM = 5,
  KNOB_TILE_BWD_DATA = 6,
  KNOB_TILE_FWD = 7,
  KNOB_TILE_ADAM_MAIN = 8,
  KNOB_SPLITK_DW = 9,
  KNOB_SPLITK_DW_BLOCKS = 10,
  KNOB_SPLITK_DW_MIN_STAGES = 11,
  KNOB_PERSIST = 12,
  KNOB_BN_APPLY_RB = 13,
  KNOB_DP_FORK_ROWS = 14,
  KNOB_SIDE_CU_HELD = 15,
  KNOB_BN_MODE = 16,
  KNOB_BN_MODE_BWD = 17,
  KNOB_BN_FUSED_ROWS = 18,
  KNOB_DW_MAIN = 19,
  KNOB_PAIR_ROWS = 20,
  KNOB_DW_MAIN_PING = 21,
  KNOB_EV_EVERY = 22,
  KNOB_LOSS_SIDE = 23,
  KNOB_DP_SMALL_AT = 24,
  KNOB_KEEP_GRADS = 25,
  KNOB_SIDE_PRIO = 26,
  KNOB_EVENT_SYSFENCE = 27,
  KNOB_DP_SHARD = 28,
  KNOB_SIDE_HOLD = 29,
  KNOB_DP_BUCKET_MIB = 30,
  KNOB_EV_ON_KERNEL = 31,
  KNOB_SPLITK_DW_F32_BLOCKS = 32,
  KNOB_DW_LATE = 33,
  KNOB_FORK_ON_KERNEL = 34,
  KNOB_FORK_PAIR_BELOW = 35,
  KNOB_COUNT_
};
static_assert(KNOB_COUNT_ == MMAD_KNOB_COUNT, "MmadKnob names every slot of the tune table");

int mmad_knob(MmadKnob k);     // the tune table (mmad_tune_set)
int mmad_group_override();

int mmad_tile_override();
int mmad_autotune_enabled();
int mmad_dbg_override();
int mmad_persist_override();   // knob 12
int mmad_splitk_override();   // 0 = shape rule; 1, 2, 4, 8, 16 = forced split factor
int mmad_splitk_dw_override();     // the same for the dW GEMMs only (knob 9)
int mmad_splitk_dw_blocks();       // dW split rule: target 64x64-tile blocks (knob 10)
int mmad_splitk_dw_min_stages();   // dW split rule: minimum K stages per slice (knob 11)
int mmad_splitk_dw_f32_blocks();   // fp32 dW split rule from 2048 rows: target blocks (knob 32)
int mmad_tile_adam_override();  // >= 0: tile of the Adam-fused dW GEMMs (-2: shape rule)
int mmad_tile_adam_for(int Mp, int Np, int K);   // ... for a shape
int mmad_tile_adam_main_override();  // >= 0: ... of those on the main stream
int mmad_tile_adam_main_for(int Mp, int Np, int K);   // ... for a shape (-2: rule)
int mmad_tile_epi_override(int epi);  // >= 0: tile of this epilogue's GEMMs

// A GEMM as the dispatcher sees it when it picks a tile: everything the rule
// for "which kernel runs" depends on (mmad_gemm_mfma.hip: tile_allowed,
// tile_runs), and nothing else.
struct GemmProblem {
  int dtype, epi;   // MMAD_F32 / MMAD_BF16, GemmEpiKind
  int Mp, Np;       // padded output shape
  int splitk;       // split factor (1 = none)
  bool fused_bn;    // train-mode BN fused into the launch (GemmEpi::bn_sync)
  bool partials;    // column partials read or written (GemmEpi::part / bpart)
  int act;          // MMAD_ACT_*
};
// the tile whose kernel runs when `cfg` is chosen for `p` (a register-direct
// tile outside its epilogue runs as its row-quad twin), or -1 when `cfg` may
// not be chosen for it.  Pure: no device, no knob.
int mmad_gemm_tile(int cfg, const GemmProblem& p);

// The launch of every GEMM kernel here: `args` holds one pointer per kernel
// parameter.  The events (nullable) ride on the launch itself through the
// extended entry point; a launch without them takes the plain one (the one
// `<<<>>>` ends in), so captured graphs hold the same node either way.
inline int mmad_gemm_launch(const void* fn, dim3 grid, dim3 block, hipStream_t s, hipEvent_t start_ev,
                            hipEvent_t done_ev, void** args) {
  if (start_ev || done_ev)
    (void)hipExtLaunchKernel(fn, grid, block, args, 0, s, start_ev, done_ev, 0);
  else
    (void)hipLaunchKernel(fn, grid, block, args, 0, s);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

// tile configuration a problem will run with (autotuned on first dispatch of
// the shape; a static heuristic before that / when tuning is off)
int mmad_gemm_plan(int Mp, int Np, int K, int epi, int dtype);
// output tiles of a configuration (= MSE loss partials written)
int mmad_gemm_ntiles(int cfg, int Mp, int Np);
// upper bound of mmad_gemm_ntiles over all configurations
int mmad_gemm_tiles(int Mp, int Np);

// split-K factor the dispatcher uses for a shape when the caller provides
// split-K workspace (1, 2, 4, 8 or 16; a function of the shape and epilogue
// only, so every tile configuration of a shape accumulates in the same order)
int mmad_gemm_splitk(int Mp, int Np, int K, int dtype, int epi);
// split-K workspace sufficient for every launch (shape-independent bound)
void mmad_gemm_splitk_bytes(int Mp, int Np, size_t* slab_bytes, size_t* ctl_bytes);
// read (and clear) the timeout word of a split-K control block after syncing
// `s`: MMAD_OK, or MMAD_EHIP with the error string set
int mmad_gemm_read_status(unsigned* ctl, hipStream_t s, const char* who);

// offset of the generation words inside a fused-BN barrier block; words per block
#define MMAD_BN_EXIT 64
#define MMAD_BN_SYNC_WORDS 128
// can a GEMM with the fused train-mode BN epilogue (bn_sync) run this shape:
// is there a fitting tile configuration whose whole grid is co-resident on
// the current device?  (the per-column-tile barrier needs every block of a
// column resident; with the whole grid resident, work of other streams can
// delay it but never block it)
bool mmad_gemm_bn_fusable(int dtype, int epi, int Mp, int Np);

// the split-bf16 GEMM (MMAD_BF16X3; FWD without statistics and SCORE only),
// reached through mmad_gemm_dispatch
int mmad_gemm_x3_dispatch(int epi, const void* A, int lda, const void* B, int ldb, int Mp, int Np,
                          int K, const GemmEpi& ep, hipStream_t s);

// ---- grouped dW launch: up to MMAD_GEMM_GROUP_MAX dW (+ Adam) GEMMs of the
// 64x64 tile in ONE launch.  The narrow layers' dW GEMMs (a few dozen tiles,
// a 64-stage K loop each at 4096 rows) are bound by one block's latency, not
// by throughput; side by side in one grid they cost about the slowest
// member's time instead of the sum.  Every output tile runs gemm_body exactly
// as in its stand-alone launch (same block index, block count, tile order, K
// order), so the bits are the separate launches'.
#define MMAD_GEMM_GROUP_MAX 4
// one member as the caller states it
struct GemmGroupProblem {
  const void *A, *B;
  int lda, ldb;
  int Mp, Np, K;
  GemmEpi ep;          // done_ev / start_ev ignored (the launch's are arguments)
};
// one member as the kernel reads it: its block range is [first_block,
// first_block + roundup(ntiles, 8)), so blockIdx & 7 (the XCD label the tile
// order relies on) stays the member-local index's; blocks past ntiles idle
struct GemmGroupEntry {
  const void *A, *B;
  int lda, ldb, K;
  int first_block, ntiles;
  GemmEpi ep;
};
struct GemmGroupTable {
  int n;
  GemmGroupEntry e[MMAD_GEMM_GROUP_MAX];
};
static_assert(sizeof(GemmGroupTable) <= 4096, "grouped dW launch: the table is a kernel argument");
// padded blocks a member of Mp x Np outputs takes in a grouped launch
inline int mmad_gemm_group_blocks(int Mp, int Np) { return ((Mp / 64) * (Np / 64) + 7) & ~7; }
// blocks of the grouped kernel resident on the current device at once (0 if
// unknown: no device)
int mmad_gemm_group_capacity(int dtype);
// Launch `n` BWD_WEIGHT problems as one grid on `s`; done_ev / start_ev
// (nullable) ride on the launch.  Returns MMAD_OK, an error, or
// MMAD_GEMM_GROUP_REFUSED with nothing launched -- more than
// MMAD_GEMM_GROUP_MAX members, a split-K member, a member the tile rule
// (mmad_tile_adam_for, a forced tile) does not put on the 64x64 tile, or more
// padded blocks than the kernel's resident capacity: the caller then launches
// the members separately.
#define MMAD_GEMM_GROUP_REFUSED 1
int mmad_gemm_dispatch_group(int dtype, int n, const GemmGroupProblem* problems, hipStream_t s,
                             hipEvent_t done_ev = nullptr, hipEvent_t start_ev = nullptr);

// cfg_used (nullable) receives the tile configuration launched
int mmad_gemm_dispatch(int dtype, int epi, const void* A, int lda, const void* B, int ldb, int Mp,
                       int Np, int K, const GemmEpi& ep, hipStream_t s, int* cfg_used = nullptr);
