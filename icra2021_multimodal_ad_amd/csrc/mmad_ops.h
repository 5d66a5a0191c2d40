// Internal (non-ABI) launchers shared by the executor.
#pragma once
#include <stdint.h>

#include "mmad_common.h"

int mmad_matrix_colsum_partials(int dtype, int M, int Mp, int Np, const void* x, float* part,
                                void* stream);
int mmad_sum2d(int rows, int cols, const float* x, int64_t ld, float scale, float* out,
               int accumulate, void* stream);
int mmad_sse_partials(int dtype, int M, int N, int Np, const void* y, const float* x, int ldx,
                      float* part, int nparts, void* stream);
int mmad_to_bf16(int64_t n, const float* x, void* y, void* stream);
int mmad_from_bf16(int64_t n, const void* x, float* y, void* stream);
// zero the padding of `planes` packed [Mp][Kp] matrices of esize-byte elements
// (2 or 4) that follow each other: columns >= K of rows < M and rows >= M whole
int mmad_zero_pad(int esize, int planes, int M, int K, int Mp, int Kp, void* x, void* stream);
int64_t mmad_vib_kl_parts(int B, int k, int ld_z);
// as the C-ABI forms, with the per-call values read from `dyn` (nullable)
int mmad_pack_input_dyn(int dtype, int M, int K, int Mp, int Kp, const float* x, int ld_x,
                        void* out, const MmadDyn* dyn, void* stream);
int mmad_vib_reparam_fwd_dyn(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                             const float* eps, float* eps_out, uint64_t seed, uint64_t offset,
                             int deterministic, void* z, int ld_z, float* kl_partial,
                             const MmadDyn* dyn, void* stream);

// ---- weight-streaming operator and the online pass (mmad_skinny.hip)
// y[rows][Np] = epi(x[rows][Kp] . w[Np][Kp]^T), M <= rows valid rows
// (mmad_fc_rows16: rows = 16, mmad_fc_rows64: rows = 64): ceil(M / 16) row
// tiles computed, all `rows` rows written, nothing at or past row `rows`
struct MmadSkinny {
  int rows;              // 16 or 64: the packed row capacity of x, y, diff and rowsq
  int M, N, Np, Kp;
  const void* x;         // [rows][Kp] (dtype), rows >= M zero
  const void* w;         // [Np][Kp] (dtype)
  const float* bias;     // [Np], nullable
  int act;
  float slope;
  const float *scale, *shift;   // eval-BN affine [Np], nullable (both or neither)
  void* y;               // [rows][Np] (dtype), nullable; rows >= M and columns >= N written 0
  const void* ref;       // score reference (fp32 if ref_f32, else dtype), nullable = 0
  int ref_f32, ldref;
  float* diff;           // fp32 [rows][lddiff], nullable: columns < N, rows >= M written 0
  int lddiff;
  const float* colw;     // per-column weight of d^2, nullable = 1
  float* rowsq;          // [Np/16][rows], non-null selects the score epilogue
};
int mmad_skinny_launch(int dtype, const MmadSkinny& a, void* stream);

#define MMAD_ONLINE_MAX_LAYERS 32
#define MMAD_ONLINE_MAX_DIFF 16
// BN layers in layer order: offsets into the running-stat layout ([2][n_bn])
// and of gamma / beta in the flat parameter buffer
struct MmadOnlineFold {
  int n, n_bn;
  int bn_off[MMAD_ONLINE_MAX_LAYERS], N[MMAD_ONLINE_MAX_LAYERS];
  int64_t g_off[MMAD_ONLINE_MAX_LAYERS], be_off[MMAD_ONLINE_MAX_LAYERS];
};
int mmad_online_fold(const MmadOnlineFold& f, const float* params, const float* running, float eps,
                     float* scale, float* shift, void* stream);
// every [rows] below: the `rows` (16 or 64) that mmad_online_finish is given
struct MmadOnlineFinish {
  int B, n_diff;                          // valid rows, diff layers (n_enc + 1)
  const float* rs[MMAD_ONLINE_MAX_DIFF];  // row partials [tiles][rows] per diff layer
  int tiles[MMAD_ONLINE_MAX_DIFF], widths[MMAD_ONLINE_MAX_DIFF];
  int sap_start, sap_end;                 // clamped: 0 <= start < end <= n_diff
  const float* nap_rs;                    // NAP row partials, null = no NAP score
  int nap_tiles;
  float nap_scale;                        // 1 / R
  float* out;                             // [n_diff + 3][rows]
  uint8_t* flags;                         // [3][rows], nullable
  const float* thresholds;                // [3], nullable
};
int mmad_online_finish(const MmadOnlineFinish& f, int rows, void* stream);

// ---- grouped forms (the sensor bank, mmad_online_bank_*): one launch over up
// to MMAD_MAX_BANK members, each member's bits those of the single form above.
// A block finds its member in a prefix table of per-member block counts that
// travels by value in the kernel arguments; no atomics, no wait between blocks.
// dtype[i]: MMAD_F32 / MMAD_BF16; members of one element type share a launch
// (at most two launches); a[i].N == 0: the member owns no blocks here
int mmad_skinny_group_launch(int rows, int n, const int* dtype, const MmadSkinny* a, void* stream);
struct MmadPackMember {
  int dtype, K, Kp;      // MMAD_F32 / MMAD_BF16
  const float* x;        // [M][ld_x]; 16-byte aligned rows or not (vec, set by the launcher)
  void* out;             // [rows][Kp]
};
int mmad_pack_input_group(int n, int M, int rows, int ld_x, const MmadPackMember* m, void* stream);
// all members' BN layers in one table: member i owns layers [first[i], first[i + 1])
#define MMAD_BANK_MAX_BN 64
struct MmadOnlineFoldMember {
  const float *params, *running;
  float *scale, *shift;
  float eps;
  int n_bn;
};
struct MmadOnlineFoldGroup {
  int n;
  int first[MMAD_MAX_BANK + 1];
  MmadOnlineFoldMember m[MMAD_MAX_BANK];
  int bn_off[MMAD_BANK_MAX_BN], N[MMAD_BANK_MAX_BN];
  int64_t g_off[MMAD_BANK_MAX_BN], be_off[MMAD_BANK_MAX_BN];
};
int mmad_online_fold_group(const MmadOnlineFoldGroup& g, void* stream);
int mmad_online_finish_group(int n, const MmadOnlineFinish* f, int rows, void* stream);

// ---- column-group mean squares (mmad_group_sq, mmad_group.hip): the bounds
// travel in the argument struct.  n_flag: rows >= n_flag get flag 0 whatever
// their score (the online pass's padding rows; the C-ABI form sets it to N)
struct MmadGroupSq {
  const float* d;        // [N][ldd] fp32
  int64_t ldd, N, n_flag;
  int G;
  int bounds[MMAD_MAX_GROUPS + 1];
  const float* thr;      // [G], nullable
  float* out;            // [G][ldo]
  int64_t ldo;
  uint8_t* flags;        // [G][ldf], nullable
  int64_t ldf;
};
int mmad_group_sq_launch(const MmadGroupSq& a, void* stream);

// ---- the refusals of mmad_mfcc and mmad_hsr_fuse_raw on their own: the
// entry points' argument lists without the stream (range_in: r, d, t as
// (lo, hi) pairs), nothing launched.  mmad_ae_online_tick runs them ahead of
// its first launch; the entry points themselves start with them.
int mmad_mfcc_check(const void* pcm, int pcm_type, int64_t L, int sr, int n_fft, int n_mels, int n_mfcc,
                    const void* plan, int64_t plan_bytes, const float* out, int64_t keep,
                    const float* norm_out, const void* ws, int64_t ws_bytes);
int mmad_hsr_fuse_raw_check(int n, const void* r, int r_type, const void* d, int d_type, const float* t,
                            const float* m, const float* range_in, const float* weights, int unimodal,
                            const float* out, int ld_out);
// mmad_hsr_fuse_raw with the ranges as an array and the tick's norm_rcp
// (include/mmad.h, mmad_tick_args): rcp != 0 multiplies by fl(1 / (hi - lo))
// where the entry point divides
int mmad_hsr_fuse_raw_launch(int n, const void* r, int r_type, const void* d, int d_type, const float* t,
                             const float* m, const float* range_in, int rcp, const float* weights, int unimodal,
                             float* out, int ld_out, void* stream);

#define MMAD_MAX_REDUCE_JOBS 24
struct MmadReduceJob {
  const float* src;   // partials, row i at src + i*stride
  float* dst;         // [Np] (column job) or [1] (scalar job)
  int nparts, stride, N, Np;
  float scale;
  int scalar;         // 1: dst[0] = scale*sum(all) + scale2*sum(src2[0:n2])
  const float* src2;
  int n2;
  float scale2;
};
struct MmadReduceJobs {
  MmadReduceJob j[MMAD_MAX_REDUCE_JOBS];
  const MmadDyn* dyn;   // non-null: scalar jobs write dyn->loss (graph-captured step)
};
int mmad_reduce_jobs(const MmadReduceJobs& jobs, int n_jobs, int max_np, void* stream);

// One Adam segment.  If bsrc != null the first bNp elements take their
// gradient from bias partials: g[e] = sum_i bsrc[i*bstride + e] (e < bN,
// else 0), written back to g (the bias grad is finalised inside the update).
struct MmadAdamSeg {
  float* p; float* g; float* m; float* v; void* shadow; int64_t n;
  const float* bsrc; int bparts, bstride, bN, bNp;
};
// Adam constants as torch.optim.Adam forms them from its double hyper-
// parameters (recovered from the floats: mmad_decimal_of); w = float(1 - beta)
struct MmadAdamConsts { float w1, w2, eps, step_size, bc2_sqrt; };
double mmad_decimal_of(float f);
MmadAdamConsts mmad_adam_consts(float lr, float beta1, float beta2, float eps, int step);
// flat Adam with the constants already formed (w1, w2: MmadAdamConsts)
int mmad_adam_w(int64_t n, float* p, const float* g, float* m, float* v, float w1, float w2,
                float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
                void* stream);
// mmad_adam_w with the step terms read from `dyn` when non-null (graph capture)
int mmad_adam_dyn(int64_t n, float* p, const float* g, float* m, float* v, float w1, float w2,
                  float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
                  const MmadDyn* dyn, void* stream);
int mmad_adam2(const MmadAdamSeg& s0, const MmadAdamSeg& s1, float w1, float w2, float eps,
               float step_size, float bc2_sqrt, void* stream);

int mmad_bn_finalize(int M, int N, int Mp, int Np, const float* stats, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, float* save_mean, float* save_rstd, float* scale, float* shift,
                     void* stream);
// train-mode BN finalize of a producer layer (Np columns) fused with the
// fold into its consumer's weights: wout[n][k] = W[n][k] * scale[k] (dtype of
// the GEMM), cpart[k/64][n] = sum_{k in block} shift[k] * W[n][k].
// W: fp32 master [Nc_p][Np]; grid (Np/64) x (Nc_p/64).
int mmad_bn_finalize_fold(int dtype, int M, int N, int Mp, int Np, const float* stats,
                          const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* save_mean,
                          float* save_rstd, float* scale, float* shift, const float* W, int Nc_p,
                          void* wout, float* cpart, void* stream);
int mmad_bn_act_bwd_apply(int dtype, int act, float slope, int M, int N, int Mp, int Np,
                          const void* dy, const void* a, const float* save_mean,
                          const float* save_rstd, const float* gamma, const double* part,
                          int nparts, void* dz, float* dgamma, float* dbeta, float* db_partials,
                          void* stream);
// the same, with `done` (nullable) completed by the launch itself
// (hipExtLaunchKernel stop event: no marker packet behind it)
int mmad_bn_act_bwd_apply_ev(int dtype, int act, float slope, int M, int N, int Mp, int Np,
                             const void* dy, const void* a, const float* save_mean,
                             const float* save_rstd, const float* gamma, const double* part,
                             int nparts, void* dz, float* dgamma, float* dbeta, float* db_partials,
                             void* stream, void* done);
