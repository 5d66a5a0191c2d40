/*
 * mmad.h -- C-ABI of the MI355X-native autoencoder train-and-score hot path.
 *
 * The reference (Yoo-Youngjae/ICRA2021_multimodal_ad) has no FFI: its hot path
 * is stock torch modules behind a Python plugin surface.  Each entry point
 * below names the reference interface it replaces (file:line, relative to the
 * reference repo root).  The Python mirror of that surface
 * (icra2021_multimodal_ad_amd/) binds these with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Device pointers unless stated.  All
 *    tensors are caller-owned; nothing here allocates device memory.
 *  - Packed layouts: every feature and batch dimension is padded to a
 *    multiple of mmad_pad_granule() (128) with zeros; a [rows][cols] matrix
 *    has leading dimension = padded cols.  "M/N/K" are the valid sizes,
 *    "Mp/Np/Kp" the padded ones.
 *  - dtype selects the activation/weight storage type of the GEMM operands
 *    (MMAD_F32: exact-fp32 parity path on f32 MFMA; MMAD_BF16: bf16 storage,
 *    fp32 accumulation; MMAD_BF16X3: split-bf16 planes, eval / score path
 *    only, see below).  Gradients, optimizer state, BN statistics and all
 *    reductions are fp32.
 *  - MMAD_BF16X3 ("x3"): a packed [Mp][ld] matrix is two bf16 planes in one
 *    allocation of fp32's size -- hi [Mp][ld], then lo at +Mp*ld elements --
 *    with hi = RNE_bf16(x), lo = RNE_bf16(x - float(hi)), zero padding in both;
 *    it stands for float(hi) + float(lo).  GEMMs form hi.hi + (hi.lo + lo.hi)
 *    on the bf16 matrix cores with fp32 accumulation (fp32-class results at
 *    three bf16 MFMAs per step).  Accepted by mmad_pack_input,
 *    mmad_unpack_output, mmad_fc_fwd (stats == NULL), mmad_fc_fwd_score,
 *    mmad_nap_score and mmad_vib_reparam_fwd (deterministic); every other operator returns
 *    MMAD_EUNSUPPORTED for it and launches nothing.
 *  - Every call returns 0 (MMAD_OK) or a negative status; the message is in
 *    mmad_last_error_string() (thread-local).  No exceptions cross the ABI.
 *  - stream is a hipStream_t passed as void* (0 = legacy default stream).
 */
#ifndef MMAD_H_
#define MMAD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMAD_ABI_VERSION 1

enum { MMAD_OK = 0, MMAD_EINVAL = -1, MMAD_EUNSUPPORTED = -2, MMAD_EHIP = -3, MMAD_ERCCL = -4 };
enum { MMAD_F32 = 0, MMAD_BF16 = 1, MMAD_BF16X3 = 2 };
/* modules/activation.py:20-45 (names 'leakyrelu', 'relu', 'sigmoid', 'tanh', None) */
enum { MMAD_ACT_NONE = 0, MMAD_ACT_LEAKYRELU = 1, MMAD_ACT_RELU = 2, MMAD_ACT_SIGMOID = 3,
       MMAD_ACT_TANH = 4, MMAD_ACT_LOGSIGMOID = 5, MMAD_ACT_SOFTMAX = 6, MMAD_ACT_LOGSOFTMAX = 7 };

const char* mmad_last_error_string(void);
int mmad_abi_version(void);
int mmad_pad_granule(void);
/* Tuning knobs (no reference counterpart).  One process-wide table, set only
 * through mmad_tune_set (the library reads no environment variables).  GEMM
 * knobs are read per dispatch; the executor's schedule knobs (14-31, 33-35) are
 * copied into a handle by mmad_ae_create, so set them before creating it.
 * For an executor handle, whether knobs 4 / 9 / 10 / 32 can split a GEMM at
 * all is fixed at mmad_ae_create as well: the handle's workspace holds the
 * split-K slabs only if one of them allowed a split then (4 > 1; 4 == 0 and,
 * bf16: 9 > 1 or 10 > 0, fp32: 32 > 0).  With the slabs the factor follows
 * the knobs per dispatch; without them no GEMM of the handle ever splits.
 *   0  GEMM tile override (-1 autotuned; 0 = 128x128/512 thr, 1 = 256x128,
 *      2 = 128x256, 3 = 64x64/256 thr, 4 = 64x128, 5 = 128x128/256 thr,
 *      6 = 256x256/512 thr (bf16 forward / MSE / score GEMMs without fused BN
 *      or split-K); a tile that does not fit a shape falls back to the tuned one)
 *   1  XCD tile-group height override (-1 rule)
 *   2  per-shape autotune on first dispatch (1, default) or static heuristic (0)
 *   3  diagnostics bits (tools/gemm_phase; 4 = force the split-K combine's
 *      timeout path, tests only)
 *   4  split-K factor override for GEMMs given split-K workspace (0 = shape
 *      rule, 1/2/4/8/16); 9 = the same for the dW GEMMs only; 10 / 11 = the dW
 *      split rule's target number of 64x64-tile blocks (0 = no split, default)
 *      and minimum K stages per slice (8)
 *   5  tile of the Adam-fused dW GEMMs (-2 shape rule, -1 autotuned); 8 = of
 *      those on the main stream at the end of the backward (default 0 =
 *      128x128; -2 = 128x128 where its grid covers >= 200 CUs, else knob 5;
 *      -1 = knob 5);
 *      6 / 7 = tile of the bwd-data / forward GEMMs (-1 autotuned)
 *   12 persistent grid for the forward-type GEMMs without a fused BN or a
 *      split (0 off; any other value: persistent whenever the tiles exceed
 *      one resident round -- with fewer tiles the ordinary grid is the same
 *      launch)
 *   13 BN-backward apply kernel: 128-row slabs per block (1, 2 or 4; any other
 *      value = 1; halved until it divides the row slabs; the column partials
 *      are merged once per block; default 2)
 *   14 data parallel: from this many padded rows, each side-stream dW GEMM
 *      starts at its own dz instead of with its bucket's lowest layer (1024;
 *      0 = one fork per bucket)
 *   15 schedule study: the side stream created behind a CU mask that leaves
 *      this many CUs to the main stream alone (0 = off; the masked stream is
 *      blocking, so call the step on a created non-blocking stream)
 *   16 train-mode BN schedule (-1 dtype default: bf16 fused, fp32 apply;
 *      0 apply kernels, 1 fold into the consumer, 2 fused into the GEMMs)
 *   17 backward BN schedule (-1 = the forward's, 2 = fused into bwd-data)
 *   18 fused BN up to this many padded rows per call (2048; fold above)
 *   19 dW GEMMs of the last layers on the main stream (2)
 *   20 ping-pong weight shadows from this many padded rows (4096); 21 = main-
 *      stream dW GEMMs then (1)
 *   22 record the bwd-data event every n-th side-stream layer (2)
 *   23 reduce the loss on the side stream right after the forward (1)
 *   24 data parallel: exchange the small bucket after this layer's bwd-data (1)
 *   25 also materialise dW in the fused step (0)
 *   26 side stream at the highest priority instead of the lowest (0)
 *   27 executor events with the system-scope fence (0)
 *   28 data parallel: sharded weight buckets (reduce-scatter, Adam on 1/N,
 *      all-gather; 1) or all-reduce + full Adam (0)
 *   29 schedule study: every side-stream dW + Adam GEMM held until the main
 *      stream has enqueued the whole bwd-data chain (0)
 *   30 data parallel: minimum exchange bucket in MiB of fp32 gradient;
 *      consecutive layers (backward order) share a bucket until it holds this
 *      much (8; 0 = one bucket per layer)
 *   31 the bwd-data GEMM's hand-off event to the side stream completed by the
 *      launch itself (hipExtLaunchKernel stop event, 1) or recorded behind it
 *      (0: a marker packet that holds the main stream's next dispatch)
 *   32 exact-fp32 dW GEMMs contracting over >= 2048 rows: split K until the
 *      launch has about this many 64x64-tile blocks, >= 16 K stages per
 *      slice (1024; 0 = never split an fp32 GEMM)
 *   33 ping-pong steps: the side-stream dW + Adam GEMMs of the top this many
 *      layers start once the main stream has also finished the layer's
 *      bwd-data GEMM and BN-backward apply, instead of at its dz (0)
 *   34 ping-pong steps: each side-stream dW's fork event completed by the
 *      launch that produces the layer's dz (BN-backward apply or bwd-data
 *      GEMM, hipExtLaunchKernel stop event) instead of a marker packet on the
 *      main stream; the top layer forks through the loss reduction's wait on
 *      the MSE launch (1; 0 = markers)
 *   35 ping-pong steps: from this layer down the side-stream dW GEMMs fork in
 *      pairs -- every other layer's dz gets no fork event and its dW is issued
 *      with the next lower layer's (0 = every layer forks) */
#define MMAD_KNOB_COUNT 36
int mmad_tune_set(int knob, int value);
int mmad_tune_get(int knob, int* value);
/* The split-K factor the dispatcher picks for a padded GEMM shape (Mp x Np
 * output, K deep) with epilogue `epi` (0 fwd, 1 MSE, 2 bwd-data, 3 dW,
 * 4 score) under the current knobs: 1, 2, 4, 8 or 16 (query only). */
int mmad_gemm_splitk_for(int Mp, int Np, int K, int dtype, int epi);
/* The GEMM tile whose kernel runs when tile `forced_cfg` (0-9) is forced
 * through knob 0 for a padded Mp x Np problem of `dtype` (MMAD_F32 /
 * MMAD_BF16) and epilogue `epi` (as above) with split factor `splitk`
 * (1 = none), a fused train-mode BN or not, column partials (BN statistics /
 * folded-BN bias partials) present or not, and activation `act`: forced_cfg
 * itself, or the row-quad tile of the same shape a register-direct tile
 * (7, 8 -> 6; 9 -> 1) runs as with partials or a non-piecewise-linear
 * activation; -1 when that tile may not be chosen for the problem (the
 * dispatcher then takes the tuned one).  A pure function of its arguments: it
 * reads no knob and touches no device (query only).
 *
 * The knob table and these two queries describe the dispatcher of this build;
 * they are not covered by MMAD_ABI_VERSION (a knob or a tile may be added or
 * retired without bumping it). */
int mmad_gemm_tile_for(int forced_cfg, int dtype, int epi, int Mp, int Np, int splitk, int fused_bn,
                       int has_partials, int act);

/* ------------------------------------------------------------------------
 * Layer operators
 * ---------------------------------------------------------------------- */

/* Split-K workspace for the calling thread's layer-operator GEMMs below
 * (optional; no reference counterpart).  Shapes with few output tiles then
 * split their K loop over 2 or 4 workgroups (a fixed factor per shape) that
 * combine in-launch.  ws: device memory of >= mmad_gemm_ws_bytes() bytes,
 * 256-byte aligned, ZEROED before first use (every launch leaves its control
 * words zero); it must not be shared by GEMMs running concurrently on
 * different streams.  ws = NULL turns it off. */
size_t mmad_gemm_ws_bytes(void);
int mmad_gemm_set_workspace(void* ws, size_t bytes);
/* Synchronises `stream` and reports (then clears) a split-K combine that timed
 * out in the calling thread's layer-operator workspace since the last check:
 * MMAD_EHIP and the error string if one did (its output tiles were not
 * written), MMAD_OK otherwise (also without a workspace). */
int mmad_gemm_status(void* stream);

/* FCLayer.forward, layers/fc_layer.py:37-48 (nn.Linear -> Activation -> BN).
 * y[Mp][Np] = bn_affine(act(x[Mp][Kp] . w[Np][Kp]^T + bias[Np])).
 * bn_scale/bn_shift (nullable): eval-mode BatchNorm1d as a per-column affine
 * (see mmad_bn_eval_affine).  stats (nullable, fp32 [Mp/32][2][Np]): per
 * 32-row chunk Welford (mean, M2) of the post-activation values, consumed by
 * mmad_bn_train_apply for train-mode BN.  Rows >= M and cols >= N are written 0.
 * MMAD_BF16X3: stats must be NULL (MMAD_EUNSUPPORTED otherwise). */
int mmad_fc_fwd(int dtype, int M, int N, int K, int Mp, int Np, int Kp, const void* x,
                const void* w, const float* bias, int act, float slope, const float* bn_scale,
                const float* bn_shift, void* y, float* stats, void* stream);

/* Last decoder layer fused with Loss('mse', reduction='sum') forward+backward
 * (modules/loss.py:31-32,47-52; model_builder.py:42):
 * d = x.w^T + bias - target; dz = grad_scale*d (dtype, [Mp][Np]);
 * partials fp32 [Mp/32][2][Np] = (sum_rows dz, sum_rows d^2). */
int mmad_fc_fwd_mse(int dtype, int M, int N, int K, int Mp, int Np, int Kp, const void* x,
                    const void* w, const float* bias, const float* target, int ld_target,
                    float grad_scale, void* dz, float* partials, void* stream);

/* Eval-mode FCLayer.forward fused with the per-window squared-diff reduction
 * of reconstruction_aggregation.py:22-28: y as mmad_fc_fwd (eval affine), and
 * rowsq[Np/128][Mp] = per-128-column partial sums of (y - ref)^2; diff
 * (nullable, fp32, ld_diff) receives y - ref for the valid region.
 * MMAD_BF16X3: ref is FP32 [Mp][Np] (not planes) and is subtracted from the
 * fp32 value of y before y is rounded to its planes, so the diff carries the
 * GEMM's precision, not the storage's; only its valid region is read. */
int mmad_fc_fwd_score(int dtype, int M, int N, int K, int Mp, int Np, int Kp, const void* x,
                      const void* w, const float* bias, int act, float slope,
                      const float* bn_scale, const float* bn_shift, void* y, const void* ref,
                      float* rowsq, float* diff, int ld_diff, void* stream);

/* FCLayer.forward for at most 16 rows, as a weight stream (the online scoring
 * path's layer operator; no reference counterpart): one block per 16 output
 * columns reads its rows of w once, straight into MFMA fragments.
 *   y[16][Np] = bn_affine(act(x[16][Kp] . w[Np][Kp]^T + bias[Np]))
 * x: packed [16][Kp] of dtype (MMAD_F32 / MMAD_BF16), rows >= M zero, w as
 * mmad_fc_fwd takes it, both 16-byte aligned; Kp a multiple of 128, Np of 16;
 * M in 1..16.  y (nullable): rows >= M and columns >= N are written 0.
 * rowsq non-null selects the score epilogue: d = y - ref on the fp32 value of
 * y (ref nullable = 0; ref_dtype MMAD_F32 or dtype; row stride ldref; only
 * rows < M, columns < N are read), rowsq fp32 [Np/16][16] = per 16-column tile
 * and row the sum of colw[n] d^2 (colw nullable = 1) over the tile's columns
 * < N, rows >= M zero; diff (nullable, fp32 [16][lddiff]): d for the columns
 * < N of all 16 rows, rows >= M as 0, nothing else.  With ref = NULL, act
 * none and colw this is the NAP run's GEMM (mmad_nap_score, K = W, N = R).
 * Activations: none, LeakyReLU, ReLU, sigmoid, tanh.  The result depends on
 * the operands alone (fixed summation order, no atomics). */
int mmad_fc_rows16(int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
                   const float* bias, int act, float slope, const float* bn_scale,
                   const float* bn_shift, void* y, const void* ref, int ref_dtype, int ldref,
                   float* diff, int lddiff, const float* colw, float* rowsq, void* stream);

/* The same operator for M in 1..64 rows: ceil(M / 16) row tiles against ONE
 * stream of w (a lane loads a chunk's weight fragments once and issues one
 * MFMA group per row tile).  Arguments and refusals as mmad_fc_rows16, with
 * 64-row layouts: x packed [64][Kp] (rows >= M zero), y [64][Np], diff fp32
 * [64][lddiff], rowsq fp32 [Np/16][64]; rows M..63 of y, diff (columns < N) and
 * rowsq are written 0, nothing beyond row 63.  Row i of the result equals, bit
 * for bit, the same row pushed through mmad_fc_rows16 in any 16-row group:
 * every row's accumulator sees the same products in the same order. */
int mmad_fc_rows64(int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
                   const float* bias, int act, float slope, const float* bn_scale,
                   const float* bn_shift, void* y, const void* ref, int ref_dtype, int ldref,
                   float* diff, int lddiff, const float* colw, float* rowsq, void* stream);

/* The same operator for up to MMAD_MAX_BANK independent members in one launch
 * per element type (the sensor bank's layer step, mmad_online_bank_score): a
 * descriptor holds the arguments of mmad_fc_rows16 / mmad_fc_rows64, dtype
 * included; `rows` (16 or 64) is shared, M may differ.  A block finds its
 * (member, 16-column tile) in a prefix table of per-member tile counts passed
 * by value in the kernel arguments; no atomics, no grid-wide wait, no flag in
 * memory, no cooperative launch.  Members of MMAD_F32 and of MMAD_BF16 in one
 * call are two launches.  Every member's y, diff and rowsq -- the zeroed rows
 * >= M and columns >= N included -- equal, bit for bit, what mmad_fc_rows16 /
 * mmad_fc_rows64 write for that member alone (the same per-tile body and K
 * order; all members ride ceil(max M / 16) row tiles, and a row tile past a
 * member's own M reads zero rows of x and writes the zeros the single form
 * writes).  A descriptor with N == 0 is an empty member: it owns no blocks and
 * none of its other fields is read.  d: a HOST array.
 * MMAD_EINVAL, nothing launched: n outside 1..MMAD_MAX_BANK, rows other than
 * 16 / 64, a null d, any non-empty member that mmad_fc_rows16 / mmad_fc_rows64
 * refuses (MMAD_EUNSUPPORTED where they return it). */
#define MMAD_MAX_BANK 8
typedef struct mmad_fc_rows_desc {
  int dtype, M, N, K, Np, Kp;
  const void* x; const void* w; const float* bias;
  int act; float slope;
  const float* bn_scale; const float* bn_shift;
  void* y;
  const void* ref; int ref_dtype, ldref;
  float* diff; int lddiff;
  const float* colw; float* rowsq;
} mmad_fc_rows_desc;
int mmad_fc_rows_group(int rows, int n, const mmad_fc_rows_desc* d, void* stream);

/* Mean square of column groups of an fp32 matrix: the per-modality anomaly
 * scores (no reference counterpart).  bounds: HOST array of G + 1 strictly
 * ascending columns, 0 <= bounds[0], bounds[G] <= ldd, 1 <= G <=
 * MMAD_MAX_GROUPS; group g is the columns [bounds[g], bounds[g + 1]) -- any
 * boundaries, contiguous by construction (a caller who wants a gap names it
 * as a group and ignores its row).
 *   out[g][n]   = sum_c d[n][c]^2 / (bounds[g + 1] - bounds[g])     n < N
 *   flags[g][n] = out[g][n] > thresholds[g]
 * d fp32 [N][ldd] (device, 4-byte aligned; rows whose base is 16-byte aligned
 * are read with 16-byte loads); out fp32 [G][ld_out], flags (nullable) uint8
 * [G][ld_flags], thresholds (nullable: every flag 0) fp32 [G] in device
 * memory; strict >, so a NaN threshold flags nothing.  Columns >= N of out and
 * flags are not written.  The summation order of one (row, group) depends on
 * the group's two bounds alone (lane-strided accumulation over aligned column
 * quads, then a fixed shuffle tree; no atomics): a row's result is the same
 * bits whatever N, ldd, the row's position or the other groups are.
 * MMAD_EINVAL, nothing launched: G outside 1..MMAD_MAX_GROUPS, bounds null,
 * negative, not strictly ascending or past ldd, N < 1, a null d or out, a
 * leading dimension of out / flags below N. */
#define MMAD_MAX_GROUPS 8
int mmad_group_sq(int64_t N, const float* d, int64_t ldd, const int* bounds, int G,
                  const float* thresholds, float* out, int64_t ld_out, uint8_t* flags,
                  int64_t ld_flags, void* stream);

/* BatchNorm1d eval affine (layers/fc_layer.py:33): scale = gamma/sqrt(rv+eps),
 * shift = beta - rm*scale, for N columns (padded columns -> 0). */
int mmad_bn_eval_affine(int N, int Np, const float* gamma, const float* beta, const float* rm,
                        const float* rv, float eps, float* scale, float* shift, void* stream);

/* BatchNorm1d train-mode forward (layers/fc_layer.py:39-45; torch
 * native_batch_norm): merges the Welford partials of mmad_fc_fwd, normalises
 * a -> y with batch statistics (biased var), updates running stats
 * (momentum, unbiased var), saves mean / rstd for backward. */
int mmad_bn_train_apply(int dtype, int M, int N, int Mp, int Np, const void* a,
                        const float* stats, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps,
                        float* save_mean, float* save_rstd, void* y, void* stream);

/* NAP run (utils/metric.py:183-238; Rotater.run utils/normalize.py:72-103 and
 * Standardizer.run :36-45 folded into one GEMM + epilogue):
 *   score[m] = (1/R) sum_{j<R} w[j] * (sum_k x[m][k] vt[j][k] + bias[j])^2
 * with vt = V^T of the rotation, bias = -(mu_r V + mu_s), w = 1/var (0 on
 * padding).  x: packed concatenated diffs [Mp][Kp] (dtype), vt [Rp][Kp]
 * (dtype); rowsq: fp32 workspace [Rp/128][Mp]; score fp32 [M].
 * MMAD_BF16X3: x is planes [2][Mp][Kp] and vt planes [2][Rp][Kp]
 * (mmad_pack_input / mmad_split_planes); bias and w stay fp32. */
int mmad_nap_score(int dtype, int M, int K, int R, int Mp, int Kp, int Rp, const void* x,
                   const void* vt, const float* bias, const float* w, float* rowsq, float* score,
                   void* stream);

/* NAP fit (Rotater.fit utils/normalize.py:52-70, then Standardizer.fit
 * :25-34 on the rotated train diffs; utils/metric.py:183-238 fits both on the
 * train diffs).  x: train diffs, device fp32 [N][ldx] (concatenated layers).
 * Outputs (device fp32): mu_r [W] = mean(x), v [W][R] (R = min(N, W)) = the
 * right singular vectors of x - mu_r in descending singular-value order (the
 * eigenvectors of the fp64 Gram, rocSOLVER dsyevd; column signs are the
 * solver's, as the reference's are its SVD's -- NAP scores do not depend on
 * them), mu_s [R] / var [R] = mean and ddof-1 variance of rot = (x - mu_r) v
 * (fp32 product, fp64 statistics as np.cov).  N >= 2.  Deterministic.
 * Synchronises `stream` once (eigensolver convergence flag). */
size_t mmad_nap_fit_ws_bytes(int64_t N, int W);
int mmad_nap_fit(int64_t N, int W, const float* x, int64_t ldx, float* mu_r, float* v, float* mu_s,
                 float* var, void* ws, size_t ws_bytes, void* stream);

/* Streaming NAP fit: mmad_nap_fit's fit accumulated batch by batch, so the
 * train diffs never exist as one matrix.  A batch is a device fp32 matrix
 * d[B][ld] with W valid columns (ld >= W; whatever lies past them is neither
 * read nor written).  state: a caller-owned, 256-byte aligned device buffer of
 * mmad_nap_fit_state_bytes(W) bytes (-1: bad W), whatever the batch sizes.
 * The caller runs three passes over the same batches, N rows in all:
 *   begin;  accumulate_sums(batch)...;  finish_mean(N) -> mu_r [W]
 *   accumulate_gram(batch, mu_r)...;    solve(N) -> v [W][R], R = min(N, W)
 *   accumulate_rot(batch, mu_r)...;     finish(N) -> mu_s [R], var [R]
 * accumulate_sums: fp64 column sums, rows in order; mu_r = fp32(S / N).
 * accumulate_gram: first centres the batch IN PLACE (d -= mu_r, fp32, rows < B
 *   and columns < W only: padding stays what it was), then adds its Gram to
 *   the running fp64 G on v_mfma_f64_16x16x4_f64 (exact products; only the
 *   upper-triangular 128x128 tiles are kept).
 * solve: mirrors G into a second matrix (G stays readable), rocSOLVER dsyevd,
 *   eigenvectors in descending order as mmad_nap_fit; synchronises `stream`.
 * accumulate_rot: takes the batch UNCENTRED, as the first pass saw it, and
 *   leaves it untouched: rot = fp32(d - mu_r) v per 2048-row chunk through the
 *   exact-fp32 GEMM, fp64 sum / sum of squares per column.
 * finish: mu_s = fp32(mean), var = fp32(sum (rot - mean)^2 / (N - 1)).
 * No atomics: for the same batches a repeated fit is bit-identical.
 * mmad_nap_fit_state_layout: info int64[3] = byte offsets of the fp64 column
 * sums [W] and of G [W][W] (row-major, upper triangle valid) in the state,
 * and the state's size.  MMAD_EINVAL (nothing launched): N < 2, B < 1, a null
 * pointer, ld < W, a state that is too small or unaligned. */
int64_t mmad_nap_fit_state_bytes(int W);
int mmad_nap_fit_state_layout(int W, int64_t* info);
int mmad_nap_fit_begin(int W, void* state, int64_t state_bytes, void* stream);
int mmad_nap_fit_accumulate_sums(int W, int B, const float* d, int64_t ld, void* state,
                                 int64_t state_bytes, void* stream);
int mmad_nap_fit_finish_mean(int W, int64_t N, void* state, int64_t state_bytes, float* mu_r,
                             void* stream);
int mmad_nap_fit_accumulate_gram(int W, int B, float* d, int64_t ld, const float* mu_r, void* state,
                                 int64_t state_bytes, void* stream);
int mmad_nap_fit_solve(int W, int64_t N, void* state, int64_t state_bytes, float* v, void* stream);
int mmad_nap_fit_accumulate_rot(int W, int64_t N, int B, const float* d, int64_t ld,
                                const float* mu_r, void* state, int64_t state_bytes, void* stream);
int mmad_nap_fit_finish(int W, int64_t N, void* state, int64_t state_bytes, float* mu_s, float* var,
                        void* stream);

/* Backward of Linear (autograd of layers/fc_layer.py:38):
 * dx[Mp][Kp] = dz[Mp][Np] . w[Np][Kp]; colsum (nullable, [Mp/32][2][Kp]
 * slot 0) = per-chunk column sums of dx (bias grad of a no-BN producer). */
int mmad_fc_bwd_data(int dtype, int M, int N, int K, int Mp, int Np, int Kp, const void* dz,
                     const void* w, void* dx, float* colsum, void* stream);

/* dW[Np][Kp] (fp32) = dz[Mp][Np]^T . x[Mp][Kp] (K = batch). */
int mmad_fc_bwd_weight(int dtype, int Mp, int Np, int Kp, const void* dz, const void* x,
                       float* dw, void* stream);

/* n (1 to 4) such dW GEMMs over the same Mp padded rows in ONE launch of the
 * 64x64 tile: dw[i][Np[i]][Kp[i]] = dz[i]^T . x[i], the bits of
 * mmad_fc_bwd_weight for each.  MMAD_EUNSUPPORTED if the problems' blocks
 * (each rounded up to 8) exceed one resident round of the kernel. */
int mmad_fc_bwd_weight_group(int dtype, int n, int Mp, const int* Np, const int* Kp, const void* const* dz,
                             const void* const* x, float* const* dw, void* stream);

/* The standalone Activation module (modules/activation.py:20-45) on fp32
 * [M][ld] rows of N values: act = any MMAD_ACT_* (softmax / logsoftmax over
 * each row, dim=-1, max-subtracted; logsigmoid = -softplus(-x); leaky slope
 * `slope`).  mmad_activation_bwd: dx from the forward OUTPUT y and dy
 * (sigmoid y(1-y), tanh 1-y^2, relu/leaky by the sign of y, logsigmoid
 * 1-exp(y), softmax y(dy - sum dy y), logsoftmax dy - exp(y) sum dy).
 * x / y / dy / dx may share ld; y may alias x (in place), dx may alias dy. */
int mmad_activation_fwd(int act, float slope, int M, int N, const float* x, int64_t ldx, float* y,
                        int64_t ldy, void* stream);
int mmad_activation_bwd(int act, float slope, int M, int N, const float* y, int64_t ldy,
                        const float* dy, int64_t lddy, float* dx, int64_t lddx, void* stream);

/* dW as mmad_fc_bwd_weight with torch.optim.Adam's step (as mmad_adam) fused
 * into the GEMM epilogue (loss.backward() + optimizer.step() for one
 * nn.Linear weight, models/auto_encoder.py:73-75): p/m/v fp32 [Np][Kp] are
 * updated in place, shadow (nullable, bf16 [Np][Kp]) receives bf16(p), dw
 * (nullable) the gradient itself.  Padding rows/columns of p/m/v must be zero
 * (they stay zero: their gradient is zero). */
int mmad_fc_bwd_weight_adam(int dtype, int Mp, int Np, int Kp, const void* dz, const void* x,
                            float* p, float* m, float* v, void* shadow, float* dw, float beta1,
                            float beta2, float eps, float step_size, float bc2_sqrt, void* stream);

/* Backward of BN(train) o Activation (layers/fc_layer.py:38-45):
 * dbeta = sum dy, dgamma = sum dy*xhat, da = gamma*rstd/M*(M dy - dbeta - xhat dgamma),
 * dz = da * act'(a).  Writes dz (dtype), dgamma/dbeta (fp32 [Np]) and db
 * partials ([Mp/128][Np], consumed by mmad_colsum).  ws: >= mmad_bn_act_bwd_ws(Mp,Np) bytes. */
size_t mmad_bn_act_bwd_ws(int Mp, int Np);
int mmad_bn_act_bwd(int dtype, int act, float slope, int M, int N, int Mp, int Np, const void* dy,
                    const void* a, const float* save_mean, const float* save_rstd,
                    const float* gamma, void* dz, float* dgamma, float* dbeta, float* db_partials,
                    void* ws, void* stream);

/* Backward of Activation alone (an FCLayer without BN, layers/fc_layer.py:38):
 * dz = dy * act'(a) from the activation output a (packed [Mp][Np], dtype;
 * rows >= M -> 0) and db partials fp32 [Mp/128][Np] (column sums of dz, the
 * bias gradient; reduce with mmad_colsum). */
int mmad_act_bwd(int dtype, int act, float slope, int M, int Mp, int Np, const void* dy,
                 const void* a, void* dz, float* db_partials, void* stream);

/* out[j] = scale * sum_{i<n_parts} partials[i*part_stride + j], j < N (Np padded -> 0). */
int mmad_colsum(int n_parts, int N, int Np, const float* partials, int part_stride, float scale,
                float* out, void* stream);

/* out[0] = scale * sum of n floats (single block, deterministic). */
int mmad_sum(int64_t n, const float* x, float scale, float* out, int accumulate, void* stream);
/* modules/loss.py:47-52, Loss('mse', reduction) called on its own (inside the
 * autoencoder it is fused into the last decoder GEMM): loss_out[0] = sum (mean
 * != 0: mean) of (y_hat - y)^2 over n fp32 elements, deterministic order.
 * work: device scratch of mmad_mse_loss_ws_floats() floats.  mmad_mse_grad:
 * d_yhat = g[0] * (2 or 2/n) * (y_hat - y), d_y = -d_yhat (either nullable;
 * g = the upstream scalar gradient on the device, nullable = 1). */
int mmad_mse_loss_ws_floats(void);
int mmad_mse_loss(int64_t n, const float* y_hat, const float* y, int mean, float* loss_out, float* work,
                  void* stream);
int mmad_mse_grad(int64_t n, const float* y_hat, const float* y, const float* g, int mean, float* d_yhat,
                  float* d_y, void* stream);

/* Elementwise split of n fp32 values into the two bf16 planes of MMAD_BF16X3:
 * hi[i] = RNE_bf16(src[i]), lo[i] = RNE_bf16(src[i] - float(hi[i])). */
int mmad_split_planes(int64_t n, const float* src, void* hi, void* lo, void* stream);

/* f32 [M][ld_x] -> packed dtype [Mp][Kp] (zero padding; MMAD_BF16X3: both planes). */
int mmad_pack_input(int dtype, int M, int K, int Mp, int Kp, const float* x, int ld_x, void* out,
                    void* stream);

/* packed dtype [Mp][Np] -> f32 [M][ld_out] (valid region).  MMAD_BF16X3:
 * hi + lo, with Mp = M rounded up to the pad granule (the lo plane's offset). */
int mmad_unpack_output(int dtype, int M, int N, int Np, const void* y, float* out, int ld_out,
                       void* stream);

/* torch.optim.Adam step (novelty_detection.py:90; amsgrad=False,
 * weight_decay=0) over a flat fp32 buffer of n params, rounded as torch's
 * CPU _single_tensor_adam rounds it:
 * m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g;
 * p += (-step_size * m) / (sqrt(v)/bc2_sqrt + eps); step_size = lr/(1-b1^t),
 * with 1-b1 and 1-b2 formed in double from the decimal each float beta came
 * from (0.9f -> 0.9), as torch forms them from the optimizer's Python floats.
 * shadow (nullable, bf16) receives bf16(p) for the first n_shadow elements. */
int mmad_adam(int64_t n, float* p, const float* g, float* m, float* v, float beta1, float beta2,
              float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
              void* stream);

/* variational_info_bottleneck reparameterisation
 * (decorators/variational_info_bottleneck.py:22-24,34,37): enc_out [Mp][ld_enc]
 * (dtype) holds mu | logvar in cols [0,btl) | [btl,2btl) of the first B rows;
 * z[row = kk*B + b][c] = eps*exp(0.5*logvar) + mu written packed into
 * z (dtype, [Mpz][ld_z]) for kk < k.  eps: injected fp32 [k][B][btl]
 * (nullable -> Philox N(0,1) from seed/offset; the draw is stored to eps_out,
 * nullable).  deterministic != 0 -> z = mu (no_grad and not stochastic).
 * kl_partial (nullable): fp32 partial sums of
 * -0.5*(1 + lv - mu^2 - exp(lv)) over the first B rows (build-defined KL,
 * SURVEY §8 a10'), one per 256 elements of the packed z buffer:
 * ceil(roundup(k*B, 128) * ld_z / 256) floats, all written.  Only their sum
 * is defined; which partial holds which rows is not.
 * MMAD_BF16X3: only deterministic != 0 with kl_partial == NULL (z = mu, a
 * copy of both planes; B rounded up to the granule locates enc_out's lo
 * plane); MMAD_EUNSUPPORTED otherwise. */
int mmad_vib_reparam_fwd(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                         const float* eps, float* eps_out, uint64_t seed, uint64_t offset,
                         int deterministic, void* z, int ld_z, float* kl_partial, void* stream);

/* Backward of the reparameterisation + beta*KL: dz [k*B rows][ld_dz] (dtype)
 * -> d_enc_out (dtype [Mp][ld_denc], mu|logvar columns); colsum (nullable)
 * receives column-sum partials [Mp/128][ld_denc] for the encoder's last bias;
 * with colsum given, ld_denc must be a multiple of 64 (the column slab of the
 * reduction; MMAD_EINVAL otherwise, nothing launched). */
int mmad_vib_reparam_bwd(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                         const float* eps, const void* dz, int ld_dz, float beta_kl,
                         void* d_enc_out, int ld_denc, float* colsum, void* stream);

/* ------------------------------------------------------------------------
 * Whole-autoencoder executor (AutoEncoder.step / validate / forward and
 * get_diffs, models/auto_encoder.py:36-91, reconstruction_aggregation.py:6-37):
 * sequences the layer operators above on one stream with no host sync.
 * ---------------------------------------------------------------------- */
typedef struct mmad_ae mmad_ae;

/* widths: encoder widths [n_enc+1] then decoder widths [n_dec+1]; hidden
 * layers (all but the last of each module) are Linear->LeakyReLU(slope)->BN,
 * last layers Linear only (model_builder.py:21-37).  vib != 0: encoder output
 * is 2*btl (mu|logvar) and dec_widths[0] = btl. */
int mmad_ae_create(mmad_ae** out, int dtype, int n_enc, const int* enc_widths, int n_dec,
                   const int* dec_widths, int vib, float slope, float bn_eps, float bn_momentum);
void mmad_ae_destroy(mmad_ae* h);

/* Flat fp32 parameter layout (padded): all weights first ([Np][Kp] per layer,
 * encoder then decoder), then per layer bias[Np], gamma[Np], beta[Np].
 * info (int64[7] per layer): w_off, b_off, gamma_off (-1), beta_off (-1),
 * Kp, Np, bn_off (offset into the [2][n_bn] running-stat buffer, -1).
 * totals (int64[4]): n_params, n_weight (= bf16 shadow length), n_bn, n_layers. */
int mmad_ae_layout(const mmad_ae* h, int64_t* info, int64_t* totals);

/* Device workspace bytes for a batch of B windows and k VIB samples. */
int64_t mmad_ae_workspace_bytes(const mmad_ae* h, int B, int k);

/* Bind caller-owned device buffers (all fp32 flat, layout above).
 * shadow: bf16 weights (MMAD_BF16) or NULL (MMAD_F32 reads params). */
int mmad_ae_bind(mmad_ae* h, float* params, float* grads, float* adam_m, float* adam_v,
                 void* shadow, float* running /* [2][n_bn]: mean then var */);

/* Refresh the bf16 weight shadow from the fp32 params (after a host-side
 * load_state_dict or any external parameter write).  MMAD_F32: refreshes the
 * score planes if attached (mmad_ae_set_score_planes), otherwise a no-op. */
int mmad_ae_sync_shadow(mmad_ae* h, void* stream);

/* Split-bf16 scoring for an MMAD_F32 handle.  planes: bf16 [2][n_weight] (hi
 * then lo), caller-owned; NULL detaches.  With planes attached,
 * mmad_ae_forward(train_bn = 0), mmad_ae_score and mmad_ae_score_stream run
 * their GEMMs as MMAD_BF16X3 (activations as planes, per-layer references and
 * diffs in fp32); everything else on the handle -- train_bn = 1 forwards,
 * every training entry point, Adam -- runs exactly as without them.  The
 * handle keeps the planes fresh: mmad_ae_bind, this call and every entry point
 * that writes weights mark them stale, and the three scoring entry points
 * re-split the weight region (one mmad_split_planes launch on the caller's
 * stream, outside any graph replay) when they are.  External parameter writes
 * (load_state_dict) follow the bf16 shadow's contract: call
 * mmad_ae_sync_shadow, which refreshes the planes of an F32 handle.
 * mmad_ae_workspace_bytes grows (fp32 reference copies, carved after every
 * other buffer) while planes are attached; attaching or detaching drops the
 * cached score graphs.  MMAD_EINVAL on a bf16 handle. */
int mmad_ae_set_score_planes(mmad_ae* h, void* planes);
/* dtype of the eval / score GEMMs: MMAD_F32, MMAD_BF16 or MMAD_BF16X3 (-1: null handle) */
int mmad_ae_score_dtype(const mmad_ae* h);

/* bf16 only: a second n_weight-element bf16 buffer (NULL turns it off).  The
 * fused step (mmad_ae_train_step) then writes the updated weights into the
 * other buffer while its backward still reads the current one, and the two
 * swap at the end of the step, so each layer's dW+Adam GEMM overlaps that
 * layer's bwd-data GEMM.  mmad_ae_sync_shadow refreshes both. */
int mmad_ae_set_shadow_pair(mmad_ae* h, void* alt);

/* Grouped dW launches of the single-GPU ping-pong step (a shadow pair set, no
 * communicator, not graph-captured): walking the side-stream layers top-down,
 * consecutive layers whose dW + Adam GEMM takes the 64x64 tile (knob 5's rule)
 * are issued as ONE launch at the lowest member's fork instead of one launch
 * each, while the group stays within `blocks` padded 64x64-tile blocks (each
 * member's tiles rounded up to 8; a member takes at most half of `blocks` -- a
 * larger launch fills the chip by itself) and `members` members (at most 4).  The
 * higher members record no fork event of their own.  Every output tile runs
 * the code of its stand-alone launch, so no bit of the step changes.
 * blocks: 0 = off (every dW its own launch), -1 = one resident round of the
 * kernel on the device (512 blocks on MI355X), < -1 = leave as it is;
 * members: 1 = off, <= 0 = leave as it is.  A group the
 * dispatcher cannot take (a split-K member, a member knob 0 / 5 move off the
 * 64x64 tile, more blocks than one resident round) runs as separate launches.
 * The schedule knobs of the tune table are fixed when the handle is created;
 * this one may be changed between steps.  A new handle starts at
 * (MMAD_DW_GROUP_BLOCKS_DEFAULT, 4). */
#define MMAD_DW_GROUP_BLOCKS_DEFAULT (-1)
int mmad_ae_set_dw_group(mmad_ae* h, int blocks, int members);
/* The grouping rule itself (pure: it reads its arguments and knob 5 only).
 * Layers l_hi - 1 down to l_lo of an n_layers model with padded dW shapes
 * Np[l] x Kp[l], contracting over rows[l] padded rows: group_of[l] receives the
 * index of the layer's group in launch order, or -1 for a launch of its own.
 * Returns the number of groups. */
int mmad_dw_group_plan(int n_layers, const int* Np, const int* Kp, const int* rows, int l_lo, int l_hi,
                       int budget, int members, int* group_of);

/* the bf16 shadow the next kernels will read (changes after each fused step
 * when a pair is set) */
const void* mmad_ae_current_shadow(const mmad_ae* h);

/* AutoEncoder.step forward+backward (models/auto_encoder.py:57-73): x fp32
 * [B][ld_x]; writes grads and loss_out[0] (device fp32; sum-MSE, or
 * recon/k + beta*KL for VIB).  eps (VIB, nullable) as mmad_vib_reparam_fwd. */
int mmad_ae_train_fwd_bwd(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                          uint64_t seed, uint64_t offset, float beta_kl, float* loss_out,
                          void* ws, int64_t ws_bytes, void* stream);

/* One whole AutoEncoder.step (models/auto_encoder.py:57-77) with
 * optimizer.step() fused in: forward + sum-MSE + backward as in
 * mmad_ae_train_fwd_bwd, and each layer's Adam update (hyper-parameters as
 * mmad_ae_adam, step = t) issued on the executor's side stream right after
 * that layer's dW GEMM, overlapping the rest of the backward.  With a
 * communicator attached (mmad_ae_set_comm) the gradients are all-reduced per
 * layer before their Adam update and the returned loss is the global sum.
 * On return every kernel is enqueued and ordered before later work on
 * `stream`. */
int mmad_ae_train_step(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                       uint64_t seed, uint64_t offset, float beta_kl, float lr, float beta1,
                       float beta2, float adam_eps, int step, float* loss_out, void* ws,
                       int64_t ws_bytes, void* stream);

/* mmad_ae_train_step replayed as ONE captured hipGraph (the whole step's
 * ~45 kernels, side-stream dW/Adam overlap included) after a 64-byte
 * host->device copy of this call's values (x, loss_out, eps, seed/offset, the
 * Adam bias-correction terms of `step`): same arguments, same results bit for
 * bit.  The first call of a signature (B, k, ld_x, x alignment, eps given or
 * not, ws, beta_kl, Adam betas/eps) runs eagerly and captures; rebinding the
 * buffers drops the captures.  With a communicator or a shadow pair attached,
 * or if capture is unavailable, it runs the eager step instead. */
int mmad_ae_train_step_graph(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                             uint64_t seed, uint64_t offset, float beta_kl, float lr, float beta1,
                             float beta2, float adam_eps, int step, float* loss_out, void* ws,
                             int64_t ws_bytes, void* stream);
/* number of captured train-step graphs (-1 for a null handle) */
int mmad_ae_train_graph_count(const mmad_ae* h);

/* loss.backward() after mmad_ae_forward(train_bn=1) on the same workspace
 * (autograd path of AutoEncoder.forward): dxhat fp32 [B][ld] = dL/dx_hat;
 * writes all parameter gradients.  Not for the VIB model. */
int mmad_ae_backward(mmad_ae* h, const float* dxhat, int ld, int B, void* ws, int64_t ws_bytes,
                     void* stream);

/* ------------------------------------------------------------------------
 * Data-parallel gradient exchange (RCCL over xGMI)
 * The reference trains in one process (novelty_detection.py:90); with one
 * process per GPU the exchange is a sum all-reduce of the gradients (the loss
 * is sum-reduced, model_builder.py:42).  RCCL is resolved from the copy
 * already loaded in the process (torch's), so there is one RCCL instance.
 * ---------------------------------------------------------------------- */
typedef struct mmad_comm mmad_comm;
int mmad_comm_unique_id_bytes(void);
/* rank 0: fills out[mmad_comm_unique_id_bytes()] (host memory) */
int mmad_comm_get_unique_id(void* out);
/* every rank, with the current HIP device set to its GPU */
int mmad_comm_create(mmad_comm** out, const void* unique_id, int nranks, int rank);
/* single-GPU loopback communicator for testing the exchange schedule: its
 * "all-reduce" scales the bucket by `scale` (= the sum over `scale` identical
 * shards) after a short delay */
int mmad_comm_create_loopback(mmad_comm** out, float scale);
/* ... posing as rank `rank` of `nranks` (tests of the sharded step's shard
 * arithmetic on one GPU: its reduce-scatter scales this rank's slice of the
 * bucket -- the slice RCCL's in-place reduce-scatter writes -- and its
 * all-gather leaves the other ranks' shards untouched) */
int mmad_comm_create_loopback_ranks(mmad_comm** out, float scale, int nranks, int rank);
void mmad_comm_destroy(mmad_comm* c);
/* in-place fp32 sum all-reduce of buf[n] on stream */
int mmad_allreduce_bucket(mmad_comm* c, float* buf, int64_t n, void* stream);
/* this communicator's rank / number of ranks (a loopback communicator: the
 * rank / nranks given to its create call; 0 / 1 for mmad_comm_create_loopback) */
int mmad_comm_rank(const mmad_comm* c);
int mmad_comm_size(const mmad_comm* c);
/* sharded exchange, in place (n divisible by the rank count): sum
 * reduce-scatter of fp32 buf[n] leaving rank r's sum in buf[r*n/N, (r+1)*n/N);
 * all-gather of every rank's shard of buf[n] (dtype MMAD_F32 or MMAD_BF16).
 * Loopback: the reduce-scatter scales only this rank's slice
 * [r*n/N, (r+1)*n/N) by the loopback's scale (after the same short delay),
 * the all-gather does nothing. */
int mmad_reduce_scatter_bucket(mmad_comm* c, float* buf, int64_t n, void* stream);
/* the same on bf16 buf[n] (RCCL's bf16 sum; loopback: bf16(x * scale)) */
int mmad_reduce_scatter_bucket_bf16(mmad_comm* c, void* buf, int64_t n, void* stream);
int mmad_all_gather_bucket(mmad_comm* c, void* buf, int64_t n, int dtype, void* stream);
/* Attach (c != NULL) or detach a communicator.  With one attached,
 * mmad_ae_train_step runs the data-parallel step: each layer's dW lands in the
 * grads buffer, is all-reduced on the executor's comm stream as soon as it is
 * complete (overlapping the rest of the backward), then Adam-updated there;
 * bias/gamma/beta grads and the loss follow in one final bucket.  BatchNorm
 * statistics stay per shard (DDP semantics).
 * Sharded weight buckets (knob 28, default on; a bucket whose size the rank
 * count does not divide falls back to the all-reduce): reduce-scatter of the
 * fp32 gradient, Adam on this rank's 1/N of the bucket (p, m, v), then an
 * all-gather of the updated bf16 weight shadow (bf16 model: 4 + 2 bytes per
 * parameter on the wire instead of 8, the Adam state stream divided by N) or
 * of the fp32 weights (fp32 model).  The bf16 model's fp32 master weights and
 * every model's Adam moments are then current only on their owning rank:
 * mmad_ae_dp_sync_master (collective: every rank, same point) all-gathers
 * them; mmad_ae_dp_master_stale says whether one is due. */
int mmad_ae_set_comm(mmad_ae* h, mmad_comm* c);
/* Optional bf16 gradient exchange for the sharded buckets (NULL: off, the
 * default): `buf` is an n_weight-element bf16 scratch buffer; each sharded
 * bucket's fp32 gradient is rounded to bf16 into it, reduce-scattered in bf16
 * (half the bytes on the wire), and this rank's summed slice is widened back to
 * fp32 before its Adam.  Not the reference's arithmetic (its gradients are
 * summed in fp32): an opt-in for exchange-bound runs. */
int mmad_ae_set_grad_bf16(mmad_ae* h, void* buf);
int mmad_ae_dp_sync_master(mmad_ae* h, void* stream);
int mmad_ae_dp_master_stale(const mmad_ae* h);

/* optimizer.step() (models/auto_encoder.py:75) on the bound buffers. */
int mmad_ae_adam(mmad_ae* h, float lr, float beta1, float beta2, float eps, int step,
                 void* stream);
/* The same on the parameter range [off, off + n) of the flat buffers (off a
 * multiple of 4; the bf16 shadow is written where the range covers weights):
 * Adam is elementwise, so the ranges of a partition give mmad_ae_adam's bits.
 * Used by the torch-exchange data-parallel step, one range per bucket. */
int mmad_ae_adam_range(mmad_ae* h, float lr, float beta1, float beta2, float eps, int step,
                       int64_t off, int64_t n, void* stream);
/* Torch-exchange data parallelism (no counterpart; the path taken when the
 * native communicator is not attached): with dW events on, every
 * mmad_ae_train_fwd_bwd records one event after each layer's dW GEMM and one
 * after its bwd-data GEMM (the last reader of its weights);
 * mmad_ae_wait_dw makes `stream` wait for both, so a caller can all-reduce and
 * Adam-update a bucket while the rest of the backward runs.  mmad_ae_dw_plan
 * writes the weight buckets in backward order (the native exchange's plan,
 * knob 30): offset and length in the flat gradient buffer and the bucket's
 * lowest layer (the one to wait for); returns their count (< 0: error). */
int mmad_ae_dw_events(mmad_ae* h, int on);
int mmad_ae_wait_dw(mmad_ae* h, int layer, void* stream);
int mmad_ae_dw_plan(const mmad_ae* h, int max_n, int64_t* off, int64_t* n, int* layer_lo);

/* AutoEncoder.forward (models/auto_encoder.py:46-50): x_hat fp32 [B][ld_out].
 * train_bn != 0: batch-stat BN + running-stat update (module.train()).
 * loss_out (nullable): sum-MSE of x_hat vs x (AutoEncoder.validate). */
int mmad_ae_forward(mmad_ae* h, const float* x, int ld_x, int B, int train_bn, float* x_hat,
                    int ld_out, float* loss_out, void* ws, int64_t ws_bytes, void* stream);

/* get_diffs + per-window squared-diff sums (reconstruction_aggregation.py:6-37,
 * utils/metric.py:133,171): layer_sq fp32 [n_enc+1][B] with layer_sq[l][b] =
 * sum_c d_l[b][c]^2.  diffs (nullable): fp32 [B][sum widths] concatenated
 * d_0 | d_1 | ... (SAP/NAP layout). */
int mmad_ae_score(mmad_ae* h, const float* x, int ld_x, int B, float* layer_sq, float* diffs,
                  void* ws, int64_t ws_bytes, void* stream);

/* Streaming scoring pass (NoveltyDetecter.test -> get_diffs over a whole
 * dataset, novelty_detection.py:15-38 / reconstruction_aggregation.py:6-37,
 * BASELINE config C5): x fp32 [N][ld_x] in device memory, scored in batches of
 * `batch` windows (the last one ragged); layer_sq fp32, row l at
 * layer_sq + l*ld_sq (ld_sq >= N), same values as mmad_ae_score per batch.
 * ws sized by mmad_ae_workspace_bytes(h, batch, 1).
 * use_graph != 0: the first call for a given (x, ld_x, N, batch, layer_sq,
 * ld_sq, ws, weight buffer) runs eagerly and captures the pass as one hipGraph;
 * later calls replay it with a single hipGraphLaunch on `stream` (up to 8
 * passes cached per handle; weights and BN running statistics are read at
 * replay time, so training in between is seen). */
int mmad_ae_score_stream(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch,
                         float* layer_sq, int64_t ld_sq, void* ws, int64_t ws_bytes, int use_graph,
                         void* stream);
/* Streamed NAP: the NAP score of every window from the scoring pass itself.
 * mmad_ae_set_nap attaches a fit over the concatenated diffs of the diff
 * layers [start, end) (0 = x_hat - x, 1 + e = encoder layer e; 0 <= start <
 * end <= n_enc + 1), W = the sum of their widths, Kp / Rp = W / R rounded up
 * to the pad granule: vt fp32 [Rp][Kp] (V^T, zero padding), bias [Rp], w [Rp]
 * as mmad_nap_score takes them, all caller-owned device buffers that must
 * outlive the attachment and are read when a pass runs (a replayed graph
 * included: re-fitting them in place is seen).  dtype = the NAP GEMM's:
 *  - MMAD_F32 (exact; any handle dtype -- a bf16 handle's fp32 diffs feed it);
 *  - MMAD_BF16X3: needs score planes attached (mmad_ae_score_dtype ==
 *    MMAD_BF16X3, else MMAD_EINVAL and nothing is launched) and vt_planes,
 *    bf16 [2][Rp][Kp], 16-byte aligned like vt, which this call fills from vt
 *    with one mmad_split_planes launch on `stream` (once: after re-fitting vt
 *    in place, attach again).  vt_planes is ignored for MMAD_F32.
 * vt == NULL detaches.  While a fit is attached mmad_ae_workspace_bytes grows
 * by the packed NAP operand [Mp][Kp] and the NAP GEMM's row partials, carved
 * after every other buffer (no other offset moves); attaching or detaching
 * drops the cached score graphs.  Every other entry point runs exactly as
 * without a fit.
 * mmad_ae_score_nap / mmad_ae_score_nap_stream: as mmad_ae_score (diffs ==
 * NULL) / mmad_ae_score_stream -- the same layer_sq bits -- and nap fp32 [B] /
 * [N] (device) = the NAP score of each window.  Per batch, in the same stream
 * or captured graph, the score GEMMs of the layers in range write their diffs
 * straight into the packed operand (fp32 through the diff output, planes
 * through the x3 score epilogue's diff-plane output; its padding is zeroed
 * for every batch), then the NAP GEMM and its column sum run as
 * mmad_nap_score's do.  With an MMAD_F32 NAP GEMM the scores equal, bit for
 * bit, mmad_ae_score(diffs) -> the range's columns -> mmad_pack_input ->
 * mmad_nap_score at the same batch size.  The graph cache key also covers nap
 * and vt.  MMAD_EINVAL (nothing launched): nap == NULL, no fit attached, or an
 * MMAD_BF16X3 fit whose score planes were detached.
 * mmad_ae_nap_operand (query; tests, debugging): info int64[5] = byte offset
 * of the packed operand in a workspace carved for B windows, its rows Mp, its
 * leading dimension Kp, W, the NAP GEMM dtype (MMAD_BF16X3: hi plane at the
 * offset, lo plane Mp*Kp bf16 elements on). */
int mmad_ae_set_nap(mmad_ae* h, int start, int end, int R, const float* vt, const float* bias,
                    const float* w, int dtype, void* vt_planes, void* stream);
int mmad_ae_score_nap(mmad_ae* h, const float* x, int ld_x, int B, float* layer_sq, float* nap,
                      void* ws, int64_t ws_bytes, void* stream);
int mmad_ae_score_nap_stream(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch,
                             float* layer_sq, int64_t ld_sq, float* nap, void* ws, int64_t ws_bytes,
                             int use_graph, void* stream);
int mmad_ae_nap_operand(const mmad_ae* h, int B, int64_t* info);

/* Streaming NAP fit from the scoring pass: the fit of the concatenated diffs
 * of the diff layers [start, end) over the N windows x [N][ld_x], the diffs
 * never materialised.  Three eager passes over x in batches of `batch`
 * windows on the handle's score path (whatever its score dtype); in each, the
 * in-range score GEMMs write a batch's diffs as fp32 into a packed operand
 * [Mp][Kp] (as the streamed NAP score's fp32 operand) and the mmad_nap_fit_*
 * step of that pass reads it: sums; centre + Gram, then solve; rotated
 * moments.  At most one batch of diffs exists at any time.  Outputs as
 * mmad_nap_fit (W = the range's width, R = min(N, W)); fit_state: an
 * mmad_nap_fit_state_bytes(W) buffer, left holding the sums and G.  ws:
 * mmad_ae_nap_fit_workspace_bytes(h, batch, start, end) bytes (-1: bad
 * arguments) = the scoring workspace of `batch` windows, its offsets
 * unchanged, followed by the operand and the pass's layer sums.  No fit needs
 * to be attached and an attached one, the graph cache and every other entry
 * point's results are untouched.  Synchronises `stream` (the solve).
 * MMAD_EINVAL (nothing launched): N < 2, a bad layer range, a null output, a
 * workspace or fit state that is too small. */
int64_t mmad_ae_nap_fit_workspace_bytes(const mmad_ae* h, int batch, int start, int end);
int mmad_ae_nap_fit_stream(mmad_ae* h, int start, int end, const float* x, int ld_x, int64_t N,
                           int batch, float* mu_r, float* v, float* mu_s, float* var,
                           void* fit_state, int64_t fit_bytes, void* ws, int64_t ws_bytes,
                           void* stream);

/* Online scoring: the scores of B <= 16 windows now (the deployment loop,
 * test_file/realtime_tester.py:291-309), as about 20 short weight-streaming
 * launches (mmad_fc_rows16 per layer) instead of the batch path's 128-row
 * tiles.  state: a caller-owned, 256-byte aligned device buffer of
 * mmad_ae_online_state_bytes(h) bytes (-1: null handle; a pure function of the
 * handle's layers, dtype and attached fit, independent of
 * mmad_ae_workspace_bytes) holding the packed input, every layer's 16-row
 * outputs, the folded BN constants, the row partials and, with a fit
 * attached, the packed NAP operand [16][Kp] (its padding zeroed when the
 * handle first sees the buffer; valid columns rewritten by every call, rows
 * >= B as zero).
 * x fp32 [B][ld_x] (device).  out fp32 [n_enc + 4][16]: rows 0..n_enc =
 * layer_sq as mmad_ae_score, then BASE = layer_sq[0] / D, SAP = the mean of
 * d^2 over the diff layers [sap_start, sap_end) with the reference's clamping
 * (utils/metric.py:155-171), and NAP -- written only with an MMAD_F32 fit
 * attached (mmad_ae_set_nap; its own layer range), else left untouched.
 * Columns >= B of every row are left untouched.  flags (nullable) uint8
 * [3][16]: flag[m][b] = score_m[b] > thresholds[m] for BASE, SAP, NAP (the
 * strict > of get_f1_score's prediction rule; 0 for a NaN threshold, for
 * thresholds == NULL and for NAP without a fit); thresholds fp32 [3] in
 * device memory, read when the pass runs.
 * use_graph != 0: the first call for a given (x, ld_x, B, range, out, flags,
 * thresholds, state, weight buffer, fit) runs eagerly and captures; later
 * calls are one hipGraphLaunch (up to 8 cached per handle, counted by
 * mmad_ae_graph_count and dropped by mmad_ae_clear_graphs, attach / detach
 * with the score graphs).  Weights, BN running statistics, the fit's vt / bias
 * / w and the thresholds are read at replay time.
 * MMAD_EINVAL, nothing launched: B outside 1..16, a null or too small state,
 * an unbound handle, score planes attached (mmad_ae_score_dtype ==
 * MMAD_BF16X3: split-bf16 planes are not supported on this path) or an
 * MMAD_BF16X3 fit attached. */
int64_t mmad_ae_online_state_bytes(const mmad_ae* h);
int mmad_ae_online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                         const float* thresholds, float* out, uint8_t* flags, void* state,
                         int64_t state_bytes, int use_graph, void* stream);

/* The online pass for B in 1..64 windows (mmad_fc_rows64 per layer): the same
 * launch list, scores and refusals as mmad_ae_online_score, with every 16 of
 * its layouts a 64.  state: mmad_ae_online_state_bytes64(h) bytes (the packed
 * input, every layer's 64-row outputs, pass-2 outputs, folded BN constants,
 * row partials [Np/16][64] and, with a fit attached, the NAP operand [64][Kp]
 * and its partials); out fp32 [n_enc + 4][64], flags uint8 [3][64], columns
 * >= B untouched.  Window i's scores and flags equal, bit for bit, those of
 * mmad_ae_online_score on any group of <= 16 windows that holds it.  The
 * captured passes share the handle's 8 online graphs with the 16-row entry
 * point; the row capacity is part of a pass's signature, and a 16-row and a
 * 64-row state may take turns on one handle.
 * MMAD_EINVAL, nothing launched: B outside 1..64, else as above. */
int64_t mmad_ae_online_state_bytes64(const mmad_ae* h);
int mmad_ae_online_score64(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                           const float* thresholds, float* out, uint8_t* flags, void* state,
                           int64_t state_bytes, int use_graph, void* stream);

/* The online pass with per-modality scores: mmad_ae_online_score (rows = 16)
 * or mmad_ae_online_score64 (rows = 64) -- the same launches on the same
 * state, the same out and flags to the bit -- plus ONE more launch,
 * mmad_group_sq on d0 = x_hat - x, the fp32 diffs the decoder's last launch
 * forms.  bounds / G as mmad_group_sq takes them, over the input columns
 * (bounds[G] <= D).  group_out fp32 [G][rows]: the mean of d0^2 over each
 * group's columns; group_flags (nullable) uint8 [G][rows] = group_out >
 * group_thresholds[g] (fp32 [G], device, read when the pass runs; nullable:
 * flags 0).  Unlike out, ALL `rows` columns are written: columns >= B as score
 * 0 and flag 0.  Window i's group scores are the same bits alone, in a 16-row
 * pass, in a 64-row pass, and from mmad_group_sq over a batch holding the same
 * d0 row.
 * d0 is read where the pass already stores it (the NAP operand, when the
 * attached fit's range starts at diff layer 0); otherwise the last launch's
 * diff output points at gstate, a second caller-owned, 256-byte aligned device
 * buffer of mmad_ae_online_groups_bytes(h, rows) bytes ([rows][Kp0] fp32; -1
 * for a null handle or rows other than 16 / 64), always required.
 * A grouped pass has its own graph signature (the group buffers, G and the
 * bounds' values are part of it) in the handle's 8 online graphs: grouped and
 * ungrouped callers may take turns on one handle.
 * MMAD_EINVAL, nothing launched: rows other than 16 / 64, G outside
 * 1..MMAD_MAX_GROUPS, bounds null / not strictly ascending / bounds[G] > D, a
 * null group_out, gstate null, too small or misaligned, and every refusal of
 * mmad_ae_online_score. */
int64_t mmad_ae_online_groups_bytes(const mmad_ae* h, int rows);
int mmad_ae_online_score_groups(mmad_ae* h, const float* x, int ld_x, int B, int sap_start,
                                int sap_end, const float* thresholds, float* out, uint8_t* flags,
                                void* state, int64_t state_bytes, int use_graph, void* stream,
                                int rows, const int* bounds, int G, const float* group_thresholds,
                                float* group_out, uint8_t* group_flags, void* gstate,
                                int64_t gstate_bytes);

/* Split-K / fused-BN health of the executor workspace `ws` (as
 * mmad_gemm_status): a no-op returning MMAD_OK for a handle whose schedule,
 * fixed at mmad_ae_create, holds neither the split-K slabs (tuning knobs 4 /
 * 9 / 10 / 32, above) nor a fused BN mode (16 / 17), whatever the knobs say
 * now; otherwise synchronises `stream` and returns MMAD_EHIP if any GEMM combine
 * of the calls since the last check timed out. */
int mmad_ae_status(mmad_ae* h, void* ws, int64_t ws_bytes, void* stream);

/* Kernel probe (measurement only; no reference counterpart): from now on the
 * executor brackets ONE GEMM launch per call with a pair of timing events on
 * the stream that launch runs on -- kind 0: the forward (or MSE / score) GEMM
 * of `layer`, kind 1: its dW GEMM (Adam fused in mmad_ae_train_step) -- for
 * the next `capacity` calls.  layer < 0 or capacity 0 turns it off.  A
 * probed launch on the main stream starts its clock only after the side
 * stream's earlier work (in probed calls only), so the pair brackets the
 * launch's own execution as a profiler's kernel record does.  Kinds 2 / 3:
 * the same launches (forward / dW) timed by events attached to the launch
 * itself (hipExtLaunchKernel start / stop: the kernel's own start and end) and
 * no wait for the side stream -- the launch as it runs in the step's schedule,
 * beside the side stream's work, cheap enough to stay on through a timed
 * region (bench.py's roofline).
 * mmad_ae_probe_read synchronises on the recorded events and writes up to
 * max_n durations (ms) in call order; returns how many (or < 0). */
int mmad_ae_probe(mmad_ae* h, int kind, int layer, int capacity);
int mmad_ae_probe_read(mmad_ae* h, float* ms, int max_n);
/* Layers (bit l) the last probed launch covered: one layer, or layers 0 and 1
 * when the main-stream tail ran its two Adam-fused dW GEMMs as one launch
 * (mmad_gemm_pair_kernel, MMAD_DW_PAIR). */
int mmad_ae_probe_layers(const mmad_ae* h);

/* number of cached score graphs, online passes included (-1 for a null
 * handle); drop them all */
int mmad_ae_graph_count(const mmad_ae* h);
int mmad_ae_clear_graphs(mmad_ae* h);

/* ------------------------------------------------------------------------
 * Anomaly-score metrics on the device (utils/metric.py, sklearn/numpy on the
 * host in the reference).  Scores fp32, labels uint8 (nonzero = anomaly,
 * novelty_detection.py:31-34), all device pointers; workspace caller-owned,
 * 256-byte aligned, sized by the *_ws_bytes queries.  Results fp64, device.
 * ---------------------------------------------------------------------- */
/* get_auc_roc :29-44 (roc_curve + auc; ties count one half, NaN with one
 * class) and get_auc_prc :97-116 (trapezoid over precision_recall_curve's
 * points): out[4] = auroc, aupr, n_pos, n_neg. */
size_t mmad_rank_metrics_ws_bytes(int64_t n);
int mmad_rank_metrics(int64_t n, const float* score, const uint8_t* label, double* out, void* ws,
                      size_t ws_bytes, void* stream);
/* get_f1_score :118-130 (threshold = np.quantile(valid, q), linear rule;
 * prediction test > threshold) and get_confusion_matrix :83-95 (test >=
 * threshold): out[10] = threshold, f1, p, r, precision, recall, tp, fp, fn,
 * tn (undefined ratios are NaN, as numpy's 0/0).  The quantile is the linear
 * rule taken in float64 (virtual index q (n_valid - 1), numpy's _lerp between
 * the two neighbours) and rounded once to fp32:
 * float32(np.quantile(float64(valid), q)).  numpy's own path for a float32
 * array forms the index and the interpolation in fp32 and can land some fp32
 * steps away; the threshold returned is the one the counts were taken at. */
size_t mmad_threshold_metrics_ws_bytes(int64_t n_valid);
int mmad_threshold_metrics(int64_t n_valid, const float* valid, int64_t n_test, const float* test,
                           const uint8_t* label, double q, double* out, void* ws, size_t ws_bytes,
                           void* stream);

/* HSR_Net multimodal fusion producer (utils/data_loaders.py:152-229; replaces
 * the per-window loop HSR_Net.forward :179-229 that TabularDataset runs at
 * :400-424).  One call fuses n windows.  Inputs fp32 device rows, each
 * nullable: r [n][3*32*32] (hand RGB), d [n][32*32] (head depth), t [n] (F/T
 * scalar), m [n][13] (MFCCs).  weights: fp32 [mmad_hsr_weight_count()] packed
 * conv1r w,b | conv2r | conv3r | conv1d | conv2d | conv3d | conv1l | conv2l
 * (torch layouts [co][ci][k..]).  unimodal == 0: r, d, t, m all required, row =
 * channel-major [27][8][8] = rgb 1024 | depth 512 | F/T 64 | mic 128 (1728);
 * unimodal != 0: the block of the last non-null modality of (r, d, t, m)
 * alone, as the reference keeps (:190-221).  out fp32 [n][ld_out]; columns
 * past the row width are not written.  The LiDAR branch (l) is never fed by
 * the reference and has no entry point. */
int mmad_hsr_weight_count(void);
int mmad_hsr_fuse(int n, const float* r, const float* d, const float* t, const float* m,
                  const float* weights, int unimodal, float* out, int ld_out, void* stream);

/* Sensor-stream normalisation of the dataset ingest (TabularDataset,
 * utils/data_loaders.py:233-434): norm_vec_np (:447-456) = per column
 * (v - min) / (max - min) over the n windows in float64, NaN (constant
 * column) -> 0, cast to fp32 -- for the hand-camera / head-depth pixel arrays
 * (:338-378), the F/T weight (:380-385) and the MFCCs (:386-394).
 * v: device [n][F] of type vtype (MMAD_SRC_*: the PNG arrays' uint8 / uint16
 * or the CSV's float64, converted exactly inside the kernel).
 * layout MMAD_NORM_FLAT: out fp32 [n][F]; MMAD_NORM_IMG24: F = C*24*32 in the
 * reference's HWC flatten, reinterpreted [C][24][32] (its .view) and
 * nearest-upsampled to [C][32][32] (its F.interpolate(size=32)): out fp32
 * [n][C*1024], ready for mmad_hsr_fuse.  ws: mmad_minmax_norm_ws_bytes. */
#define MMAD_SRC_F64 0
#define MMAD_SRC_U8 1
#define MMAD_SRC_U16 2
#define MMAD_SRC_I32 3
#define MMAD_SRC_F32 4
#define MMAD_NORM_FLAT 0
#define MMAD_NORM_IMG24 1
size_t mmad_minmax_norm_ws_bytes(int64_t n, int F);
int mmad_minmax_norm(int64_t n, int F, const void* v, int vtype, int layout, float* out, void* ws,
                     size_t ws_bytes, void* stream);

/* Microphone front end: MFCCs from raw PCM (save_mfcc_from_wav,
 * utils/data_loaders.py:676-701, the same recipe as concatdata_maker.py:15-49)
 * and norm_vec (:703-712) of the latest frames, the stage of
 * get_realtime_dataloader (:734-737) ahead of mmad_hsr_fuse.  The arithmetic
 * is librosa 0.8's: melspectrogram(y, sr, n_fft, hop_length = n_fft, n_mels)
 * -- frame t covers samples t*n_fft - n_fft/2 .. + n_fft - 1 of y, both ends
 * reflect-padded (-i -> i, L-1+i -> L-1-i), times the periodic Hann window,
 * power |X_k|^2 of bins 0..n_fft/2, S = mel filterbank . power --
 * power_to_db(S, ref=np.max): dB = 10 log10(max(1e-10, S)) - 10 log10(max(1e-10,
 * max S)), floored at max(dB) - 80, both maxima over EVERY frame and mel of
 * the call (a window's MFCCs depend on the buffer it came in, as in the
 * reference) -- and mfcc = DCT-II ortho(dB)[:n_mfcc].  Everything after the
 * PCM load is fp64; the stores are fp32.
 * Parameters: sr (Hz), n_fft 16..4410 (= the hop: the reference always calls
 * with window_size == stride; 4410 is the deployment's 0.1 s at 44.1 kHz, 2205
 * the ETL's after librosa.load resamples to 22050), n_mels 1..128, n_mfcc
 * 1..n_mels.
 * mmad_mfcc_frames: librosa's centred frame count 1 + (L + 2*(n_fft/2) -
 * n_fft) / n_fft of L samples; -1 when L < n_fft/2 + 1 (no reflection exists).
 * mmad_mfcc_filterbank: HOST function, no GPU: librosa.filters.mel(sr, n_fft,
 * n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney') in double -- Slaney mel
 * scale (linear below 1 kHz, log above, logstep = ln(6.4)/27), triangles from
 * the ramps, each filter times 2 / (f[i+2] - f[i]) -- dense into the host
 * array fb [n_mels][n_fft/2+1].
 * mmad_mfcc_plan_bytes / mmad_mfcc_plan_init: the plan is a caller-owned,
 * 256-byte aligned device buffer (as the online state is) that the host
 * fills once, in double, with the periodic Hann window 0.5 - 0.5 cos(2 pi
 * n/N), the twiddle table cos/sin(2 pi j/N), j = 0..N-1, the filterbank's
 * nonzero runs and the DCT basis rows 0..n_mfcc-1, and copies over on
 * `stream` (the call returns when the copy has read its host staging; it is
 * not capturable).  No library-global state: the plan's header names its
 * parameters and the kernels write nothing when a call's differ.  plan_bytes
 * returns -1 for parameters out of range.
 * mmad_mfcc_ws_bytes: the caller-owned, 256-byte aligned scratch of a call
 * with n_frames frames: the power spectra (rows of 4410/2 + 1 bins whatever
 * n_fft is), the mel power [n_frames][n_mels], the per-frame maxima and the
 * fp64 coefficients; -1 for arguments out of range.
 * mmad_mfcc: pcm: DEVICE [L] of pcm_type MMAD_PCM_I16 (cast to float without
 * scaling, as the reference does) or MMAD_PCM_F32.  out: fp32 [n_frames][n_mfcc],
 * every frame.  norm_out: nullable fp32 [keep][n_mfcc], 1 <= keep <= n_frames:
 * norm_vec of the LAST keep frames, (hi - lo) (v - min) / (max - min) + lo with
 * min and max over all keep*n_mfcc values (max == min: what IEEE division
 * gives, the reference's own result).  Three launches on `stream`, no host
 * synchronisation (capturable), no atomics, fixed reduction order: a call's
 * bits repeat.  Returns MMAD_EINVAL and launches nothing for parameters out
 * of range, a null pcm / plan / out / ws, a plan or workspace too small or
 * misaligned, L too short, keep out of range or an unknown pcm_type. */
#define MMAD_PCM_I16 0
#define MMAD_PCM_F32 1
int64_t mmad_mfcc_frames(int64_t L, int n_fft);
int mmad_mfcc_filterbank(int sr, int n_fft, int n_mels, double* fb);
int64_t mmad_mfcc_plan_bytes(int sr, int n_fft, int n_mels, int n_mfcc);
int mmad_mfcc_plan_init(void* plan, int64_t bytes, int sr, int n_fft, int n_mels, int n_mfcc,
                        void* stream);
int64_t mmad_mfcc_ws_bytes(int64_t n_frames, int n_mels);
int mmad_mfcc(const void* pcm, int pcm_type, int64_t L, int sr, int n_fft, int n_mels, int n_mfcc,
              const void* plan, int64_t plan_bytes, float* out, int64_t keep, float lo, float hi,
              float* norm_out, void* ws, int64_t ws_bytes, void* stream);

/* mmad_hsr_fuse on the sensor queues as they are: r [n][3072] and d [n][1024]
 * of element type r_type / d_type (MMAD_SRC_U8 or MMAD_SRC_F32: the camera
 * queues' uint8 frames, or fp32), t fp32 [n], each mapped inside the loads by
 * norm_vec (utils/data_loaders.py:703-712) from its (lo, hi) range to [-1, 1]
 * -- fp32, every operation rounded on its own, ((2 (v - lo)) / (hi - lo)) + (-1)
 * with a correctly rounded division and no contraction, hi - lo formed in
 * double and rounded once: the bits of the elementwise chain in IEEE fp32
 * followed by mmad_hsr_fuse.  m fp32 [n][13] is taken as it is (mmad_mfcc's
 * norm_out).  weights, unimodal, the nullable modalities, out and ld_out as
 * mmad_hsr_fuse (columns past the row width are not written); one launch.
 * MMAD_EINVAL, nothing launched: every refusal of mmad_hsr_fuse, and for a
 * modality the call reads: an element type other than U8 / F32, hi == lo, a
 * pointer not aligned to two of its elements (the u8 loads are 2-byte pairs). */
int mmad_hsr_fuse_raw(int n, const void* r, int r_type, const void* d, int d_type, const float* t,
                      const float* m, float r_lo, float r_hi, float d_lo, float d_hi, float t_lo,
                      float t_hi, const float* weights, int unimodal, float* out, int ld_out,
                      void* stream);

/* One tick of the deployment loop from device-resident raw buffers to scores:
 * mmad_mfcc's three launches (pcm [L] -> mfcc_out [n_frames][n_mfcc] and
 * mfcc_norm [B][n_mfcc], the last B frames to [-1, 1]), mmad_hsr_fuse_raw of
 * r, d, t and mfcc_norm (the fused row, range_in = r, d, t as (lo, hi) pairs)
 * into x [B][ld_x], then the online pass on x: mmad_ae_online_score (rows 16)
 * or mmad_ae_online_score64 (rows 64), or with bounds != NULL
 * mmad_ae_online_score_groups.  out, flags and the group outputs are the bits
 * those entry points produce on the same x.  norm_rcp: 0 = the quotient of
 * mmad_hsr_fuse_raw (IEEE division); != 0 = the product with fl(1 / (hi - lo)),
 * rounded once, in its place -- what torch's device kernels compute for
 * tensor / Python scalar, so that a tick reproduces, bit for bit, a row that
 * was normalised by torch on the device (OnlineScorer.score_sensors); the
 * two differ in the last place of about half the uint8 values.  It is part of
 * the graph signature.  The arguments travel in one flat
 * struct; every buffer is caller-owned device memory with the alignment its
 * own entry point asks for, and the sizes are checked against
 * mmad_mfcc_plan_bytes, mmad_mfcc_ws_bytes, mmad_mfcc_frames * n_mfcc * 4
 * (mfcc_out_bytes), B * n_mfcc * 4 (mfcc_norm_bytes), mmad_hsr_weight_count
 * (hsr_weight_count), mmad_ae_online_state_bytes[64] and
 * mmad_ae_online_groups_bytes.
 * use_graph != 0: the first call for a signature -- the online pass's own plus
 * the sensor pointers and types, L, the MFCC parameters, plan, workspace and
 * outputs, the weight buffer and the ranges -- runs eagerly and captures one
 * linear chain on one stream; later calls are one hipGraphLaunch.  The
 * captures share the handle's 8 online graphs (mmad_ae_graph_count,
 * mmad_ae_clear_graphs).  Every buffer is read at replay time: new samples,
 * frames or repacked weights in the same buffers need no new capture.
 * MMAD_EINVAL, nothing launched and nothing captured: a null argument struct,
 * a model input width other than the fused row's 1728, mfcc_out / mfcc_norm /
 * hsr_weights too small, and every refusal of mmad_mfcc, mmad_hsr_fuse_raw and
 * the online entry point the call selects. */
typedef struct mmad_tick_args {
  /* the raw queues */
  const void* pcm; int pcm_type; int64_t L;
  const void* r; int r_type;
  const void* d; int d_type;
  const float* t;
  float range_in[6];
  int norm_rcp;
  /* the microphone front end */
  int sr, n_fft, n_mels, n_mfcc;
  const void* plan; int64_t plan_bytes;
  float* mfcc_out; int64_t mfcc_out_bytes;
  float* mfcc_norm; int64_t mfcc_norm_bytes;
  void* mfcc_ws; int64_t mfcc_ws_bytes;
  /* the fusion producer */
  const float* hsr_weights; int hsr_weight_count;
  /* the online pass */
  float* x; int ld_x, B, rows, sap_start, sap_end;
  const float* thresholds; float* out; uint8_t* flags;
  void* state; int64_t state_bytes;
  /* per-modality scores (bounds == NULL: none) */
  const int* bounds; int G;
  const float* group_thresholds; float* group_out; uint8_t* group_flags;
  void* gstate; int64_t gstate_bytes;
} mmad_tick_args;
int mmad_ae_online_tick(mmad_ae* h, const mmad_tick_args* a, int use_graph, void* stream);

/* Sensor bank: the online pass of up to MMAD_MAX_BANK independent models (the
 * fused detector and its unimodal siblings: separate handles, not the column
 * groups of one model) on ONE shared input, sharing launches.  The pass walks
 * the steps of the single pass once -- pack, BN fold, pass 1 layer by layer,
 * pass 2 layer by layer, NAP, finish -- and issues one grouped launch per
 * step over the members that have that step (mmad_fc_rows_group and the
 * grouped pack / fold / finish kernels; a layer step is two launches when its
 * members are of both element types; the VIB reparameterisation and
 * mmad_group_sq stay one launch per member that uses them).  Members may
 * differ in depth, width, dtype, VIB, attached fit and groups.  Every member's
 * out, flags, group_out and group_flags are, bit for bit, what its own
 * mmad_ae_online_score / _score64 / _score_groups call writes given
 * x + col0[i] with the same ld_x.
 * create: handles[i] (not owned; they outlive the bank) reads the columns
 * [col0[i], col0[i] + D_i) of the shared x; rows (16 / 64) is every member's
 * row capacity.  mmad_online_bank_state_bytes(bank, i) is member i's
 * mmad_ae_online_state_bytes (rows 16) or _bytes64 (rows 64): a member's state
 * (and gstate) may be the very buffers its own calls use, bank and single
 * calls taking turns.
 * members[i]: the per-member arguments of mmad_ae_online_score_groups (bounds
 * == NULL: an ungrouped member), as a HOST array of the bank's n entries.
 * The grouped pack kernel reads x with 16-byte loads: x + col0[i] must be
 * 16-byte aligned and ld_x a multiple of 4.
 * use_graph != 0: the first call for a signature (every member's own
 * signature, on the shared x) runs eagerly and captures one linear chain on
 * one stream -- no parallel branches, no second stream; later calls are one
 * hipGraphLaunch.  The bank owns up to 8 captured passes
 * (mmad_online_bank_graph_count; mmad_online_bank_destroy drops them) and
 * every buffer is read at replay time, as for the handle's online graphs.
 * Re-attaching a fit to a member makes a new signature only if the fit's
 * buffers moved: destroy and re-create the bank after changing a member's
 * fit.  mmad_online_bank_graph_nodes: the kernel-node count of the last
 * captured pass (0 before the first capture).
 * mmad_online_bank_tick is mmad_ae_online_tick with the bank pass in place of
 * the single pass: of `a` it reads the raw queues, the front end, the fusion
 * producer and x, ld_x, B, rows; the single pass's fields (sap_start ..
 * gstate_bytes) are ignored in favour of members[].  The fused row (ld_x >=
 * 1728) is required of x, not of any member: a bank may hold no fused member
 * (a bank of one `mic` model is the unimodal tick).  All members read the one
 * fused row, i.e. one set of HSR weights.
 * MMAD_EINVAL, nothing launched and nothing captured: n outside
 * 1..MMAD_MAX_BANK, rows other than 16 / 64 (create; tick: a->rows other than
 * the bank's), a null handle, col0[i] < 0, more than 64 BatchNorm layers over
 * all members; col0[i] + D_i > ld_x, a misaligned x + col0[i] or ld_x, and
 * every refusal of the member's own online entry point (and, for the tick, of
 * mmad_mfcc and mmad_hsr_fuse_raw).
 * These entries are additive: MMAD_ABI_VERSION stays 1 and covers them from
 * this header on (the struct layouts below included). */
typedef struct mmad_online_bank mmad_online_bank;
typedef struct mmad_bank_member {
  int sap_start, sap_end;
  const float* thresholds; float* out; uint8_t* flags;
  void* state; int64_t state_bytes;
  const int* bounds; int G;
  const float* group_thresholds; float* group_out; uint8_t* group_flags;
  void* gstate; int64_t gstate_bytes;
} mmad_bank_member;
int mmad_online_bank_create(mmad_online_bank** bank, int n, mmad_ae* const* handles, const int* col0,
                            int rows);
void mmad_online_bank_destroy(mmad_online_bank* bank);
int64_t mmad_online_bank_state_bytes(const mmad_online_bank* bank, int i);
int mmad_online_bank_score(mmad_online_bank* bank, const float* x, int ld_x, int B,
                           const mmad_bank_member* members, int use_graph, void* stream);
int mmad_online_bank_tick(mmad_online_bank* bank, const mmad_tick_args* a,
                          const mmad_bank_member* members, int use_graph, void* stream);
int mmad_online_bank_graph_nodes(const mmad_online_bank* bank);
int mmad_online_bank_graph_count(const mmad_online_bank* bank);

#ifdef __cplusplus
}
#endif
#endif /* MMAD_H_ */
