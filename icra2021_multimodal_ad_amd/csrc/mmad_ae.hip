// Whole-autoencoder executor (mmad_ae_* in include/mmad.h).
//
// Replaces the reference's per-op Python dispatch of AutoEncoder.step /
// validate / forward (models/auto_encoder.py:36-91) and get_diffs
// (reconstruction_aggregation.py:6-37): one host call enqueues the whole
// forward + backward (+ Adam) or scoring sequence, no host syncs, no device
// allocation (caller workspace).
//
// Train-mode dataflow per hidden layer l (Linear -> LeakyReLU -> BN):
//   fwd GEMM -> a_l + Welford partials in its epilogue -> bn_fold (mean, rstd,
//   scale s, shift t, running stats; W'_{l+1} = W_{l+1} diag(s) and the
//   partial bias sum_k t[k] W_{l+1}[n][k]) -> the consumer GEMM contracts the
//   raw a_l with W'; the normalised y_l is never written to HBM.  Backward: the
//   bwd-data GEMM epilogue emits the BN-backward column partials of dy_l;
//   bn_act_bwd_apply produces dz_l; the dW GEMM against the raw a_{l-1}, fixed
//   up in its epilogue (s[k] acc + t[k] db[n]), runs on a side stream with that
//   layer's Adam update fused into the epilogue (single-GPU step), overlapping
//   the remaining backward chain on the main stream.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmad_common.h"
#include "mmad_gemm.h"
#include "mmad_ops.h"
#include "mmad_comm.h"

#define RET_IF(x)                    \
  do {                               \
    int r_ = (x);                    \
    if (r_ != MMAD_OK) return r_;    \
  } while (0)

// Executor events only order work between streams of this device, so they
// skip the system-scope fence (L2 writeback for host visibility) that a
// default event adds at record time.  Each record still leaves a ~5 us bubble
// on the main stream (~6 us with the fence; 0.513 vs 0.521 ms/step).
// Device-scope release/acquire (the same as a kernel boundary on one stream)
// still orders the data.  Knob 27 restores the default.
static unsigned ev_flags(int sysfence) {
  return sysfence ? (unsigned)hipEventDisableTiming
                  : (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
}

struct AeLayer {
  int K, N, Kp, Np;
  int act, bn, enc;
  int64_t w_off, b_off, g_off, be_off, bn_off;
};

struct mmad_ae {
  int dtype, n_enc, n_dec, vib, btl;
  float slope, bn_eps, bn_mom;
  std::vector<AeLayer> L;
  int64_t n_params, n_weight, n_bn;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *running = nullptr;
  void* shadow = nullptr;
  // bf16 ping-pong: the fused step's Adam writes the new weights into
  // shadow_alt while this step's backward still reads shadow, then the two
  // swap; so a dW GEMM need not wait for its layer's bwd-data GEMM
  void* shadow_alt = nullptr;
  // split-bf16 scoring (mmad_ae_set_score_planes, F32 handles): bf16
  // [2][n_weight] weight planes; the eval forward / score GEMMs then run as
  // MMAD_BF16X3.  planes_stale: the fp32 weights were (or may have been)
  // written since the last split; the scoring entry points re-split first
  void* planes = nullptr;
  bool planes_stale = true;
  // streamed NAP (mmad_ae_set_nap): the fit of the concatenated diffs of the
  // diff layers [start, end) (0 = x_hat - x, 1 + e = encoder layer e), all
  // caller-owned.  dtype: the NAP GEMM's (MMAD_F32: fp32 operand written
  // through the score GEMMs' diff output; MMAD_BF16X3: plane operand written
  // through their diff-plane output, vt split into vt_planes at attach)
  struct NapFit {
    bool on = false;
    int start = 0, end = 0, K = 0, Kp = 0, R = 0, Rp = 0, dtype = MMAD_F32;
    const float *vt = nullptr, *bias = nullptr, *w = nullptr;
    void* vt_planes = nullptr;
  } nap;
  // side stream + events for the dW / Adam overlap (created at bind time)
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> ev_fork, ev_data;
  hipEvent_t ev_join = nullptr;
  hipEvent_t ev_loss = nullptr;   // fused step: forward done -> the loss reduction on the side stream
  // the schedule, copied from the tune table at create (include/mmad.h knobs
  // 16-27): one schedule per handle, whatever the table says later
  unsigned ev_flags_ = 0;
  int loss_side = 1;      // knob 23: reduce the loss on the side stream after the forward
  int side_prio_hi = 0;   // knob 26
  // knob 15: > 0 = the side stream is created behind a CU mask that leaves
  // this many CUs (evenly spaced over the mask) to the main stream alone
  int side_cu_held = 0;
  // data-parallel step: the small bucket (bias / gamma / beta grads + loss)
  // goes on the comm stream right after the bwd-data GEMM of this layer
  // (ahead of this layer's and the lower layers' weight buckets); knob 24
  int dp_small_at = 1;
  // data-parallel step: sharded weight buckets (knob 28); master_stale: the
  // bf16 model's fp32 master weights / every model's Adam moments are
  // current only on their owning rank since the last mmad_ae_dp_sync_master
  int dp_shard = 1;
  // data-parallel step: consecutive layers' weight gradients (backward
  // order) share one exchange bucket until it holds at least dp_bucket_mib
  // MiB of fp32 gradient (knob 30; 0 = one bucket per layer)
  int dp_bucket_mib = 8;
  // data-parallel step: from this many padded rows each side-stream dW GEMM
  // is issued as soon as its own dz is complete instead of with its bucket's
  // closing layer (knob 14; 0 = one fork per bucket)
  int dp_fork_rows = 1024;
  bool master_stale = false;
  int mse_tiles = 0;   // loss partials written by the last MSE GEMM
  // data parallelism: RCCL communicator (not owned), its stream and events
  mmad_comm* comm = nullptr;
  hipStream_t cstream = nullptr;
  std::vector<hipEvent_t> ev_dw;
  // torch-exchange data parallelism (mmad_ae_dw_events): the forward+backward
  // without Adam records ev_xdw[l] after dW_l and ev_xdata[l] after bwd-data of
  // l.  System-scope fences (unlike the executor's own events): the exchange
  // may read the gradients with a copy engine, which does not see the L2
  bool dw_events = false;
  std::vector<hipEvent_t> ev_xdw, ev_xdata;
  // optional bf16 gradient exchange (mmad_ae_set_grad_bf16): n_weight bf16
  void* grad_bf16 = nullptr;
  hipEvent_t ev_small = nullptr, ev_cdone = nullptr;
  // schedule study (knob 29): every side-stream dW + Adam GEMM held until the
  // main stream has enqueued the whole bwd-data chain (ev_hold), to separate
  // the chain's in-step contention from its barrier costs
  int side_hold = 0;
  // knob 33 (ping-pong steps): the side-stream dW + Adam GEMMs of the top
  // dw_late layers fork behind the layer's bwd-data + BN apply instead of at
  // its dz, so the largest dW does not share the CUs with the apply below it
  int dw_late = 0;
  // knob 34 (ping-pong steps): each side-stream dW's fork event (dz_l ready)
  // completed by the launch that produces dz_l (the BN-backward apply or the
  // bwd-data GEMM: hipExtLaunchKernel stop event) instead of a marker packet
  // recorded on the main stream before the bwd-data GEMM of l -- each marker
  // held the main stream's next dispatch ~5 us; the top layer's fork is the
  // loss reduction's wait on the MSE launch, already on the side stream
  int fork_on_kernel = 1;
  // knob 35 (ping-pong steps): from this layer down, side-stream dW GEMMs
  // fork in pairs -- every other layer's dz gets no fork event and its dW is
  // issued with the next lower layer's (where the side stream lags the chain
  // by more than a layer anyway, each fork saved is a ~5-us hold on the
  // main stream; 0 = every layer forks)
  int fork_pair_below = 0;
  // ping-pong steps (mmad_ae_set_dw_group): consecutive side-stream layers
  // whose dW + Adam GEMM takes the 64x64 tile are issued as ONE grouped launch
  // (mmad_gemm_dispatch_group) at the lowest member's fork -- at 4096 rows
  // each of the narrow layers' launches is one block's 64-stage K loop,
  // 23-25 us for 16 to 135 blocks, and they ran back to back.  blocks = the
  // group's budget of padded blocks (0 = off: every dW its own launch; < 0 =
  // one resident round of the kernel), members = at most this many per group
  int dw_group_blocks = MMAD_DW_GROUP_BLOCKS_DEFAULT;
  int dw_group_members = MMAD_GEMM_GROUP_MAX;
  hipEvent_t ev_hold = nullptr;
  // fused step: dW GEMMs of layers < dw_main run on the caller's stream
  // (knob 19; tools/sched_sweep.py: 0.499 ms (2) vs 0.512 (1) vs 0.523 (3));
  // keep_grads (knob 25): also write dW to the grads buffer
  int dw_main = 2;
  // ping-pong schedule per call from this many padded rows (bf16 with a
  // shadow pair; knob 20), with dw_main_ping main-stream dW GEMMs (knob 21):
  // VIB B=4096 0.941-0.945 vs 0.995-0.999 ms/step, B=1024 0.450-0.455 vs
  // 0.442-0.449 (profiles/r02bu_*, r02bv_*)
  int pair_rows = 4096;
  int dw_main_ping = 1;
  int keep_grads = 0;
  // train-mode BN: fold the batch statistics into the consumer's weights
  // (bn_fold_k; the bf16 throughput path) or normalise the activations into y
  // (bn_train_apply_k; the exact-fp32 parity path: folding contracts the raw,
  // un-centred activations and cancels the mean back out, which costs the
  // fp32 path ~10x the reference's rounding error on BN-producer layers).
  // Set at create from the dtype and knob 16.
  int fold = 1;
  // train-mode BN inside the producing GEMM (bn_mode 2, MMAD_BN_MODE): the
  // forward GEMM's epilogue finishes the batch statistics and writes y, the
  // bwd-data GEMM's epilogue writes dz (a per-column-tile barrier between the
  // blocks of one column, mmad_gemm_mfma.hip) -- no finalize / fold / apply
  // launches.  Layers whose grid cannot be co-resident fall back to mode 0
  // (apply kernels).  0 = apply kernels, 1 = fold, 2 = fused (knob 16).  Default: bf16
  // 2 up to bn_fused_rows padded rows per call (measured: D=2048 B=1024
  // 0.495 ms/step fused vs 0.531 apply vs 0.536 fold; B=4096 VIB 1.33 fused
  // vs 1.32 apply vs 1.27 fold -- more tiles per column, longer barrier
  // waits), fold above; fp32 0 (the parity path).
  int bn_mode = 0;
  // backward BN schedule override for the bf16 path (knob 17: -1 =
  // the forward's; 2 = fused into the bwd-data GEMMs whatever the forward did:
  // the fused backward needs only a, the saved mean / rstd and gamma, which
  // every forward schedule leaves)
  int bn_mode_bwd = -1;
  int bn_fused_rows = 2048;   // knob 18
  // fused step: record the "bwd-data of l done" event only every ev_every-th
  // side-stream layer (each record costs a bubble on the main stream); the dW
  // GEMMs of the layers in between wait for the next recorded one (knob 22;
  // c2 0.435-0.440 vs 0.442-0.444 with 1, profiles/r02bv_*)
  int ev_every = 2;
  // the main stream's hand-off events (bwd-data -> side-stream dW, MSE ->
  // side-stream loss) completed by the GEMM launch itself (knob 31)
  int ev_on_kernel = 1;
  // hipGraph cache for mmad_ae_score_stream: one captured graph per
  // (input, output, workspace, N, batch) pass, replayed with one launch
  struct ScoreGraph {
    const float* x; int64_t ld_x, N; int batch; float* sq; int64_t ld_sq; void* ws;
    const void* wts;   // weight operand base (the bf16 shadow may be re-pointed)
    float* nap;        // NAP output (null: a pass without it) and the fit it was captured with
    const void* nap_vt;
    hipGraphExec_t exec;
  };
  std::vector<ScoreGraph> graphs;
  hipStream_t gstream = nullptr;   // capture stream (the caller's may be the null stream)
  // the same for mmad_ae_online_score: one captured 16-row pass per call
  // signature.  online_ready: the state buffer whose NAP operand this handle
  // has zeroed (its padding is never written again)
  struct OnlineGraph {
    const float* x; int ld_x, B, sap_start, sap_end; const float* thr; float* out; uint8_t* flags;
    void* state; const void* wts; const void* nap_vt;
    hipGraphExec_t exec;
  };
  std::vector<OnlineGraph> ographs;
  const void* online_ready = nullptr;
  // kernel probe (mmad_ae_probe): timing events around ONE GEMM launch of
  // the step, on the stream it is launched on (bench roofline, in situ)
  mutable int probe_id = -1;
  mutable int probe_n = 0;
  mutable unsigned probe_mask = 0;    // layers the last probed launch covered (bit l)
  std::vector<hipEvent_t> probe_ev;   // [2 * capacity]: start, end pairs
  hipEvent_t probe_sync = nullptr;    // a main-stream probe's start waits for the side stream
  // probe kinds 2 / 3: the events ride on the launch itself (hipExtLaunchKernel
  // start / stop: the kernel's own start and end, as rocprofv3's kernel records)
  // and nothing waits for the side stream -- the launch as it runs in the
  // step's schedule, so the probe can stay on through a timed region
  bool probe_kev = false;
  // hipGraph-captured fused train steps (mmad_ae_train_step_graph): one per
  // call signature, replayed after a host->device copy of the per-call values
  // (a ring of pinned host slots, each reused only once its copy has run)
  struct TrainGraph {
    int B, k, ld_x, xvec, has_eps, dw_main, ev_every, keep_grads;
    const void* ws;
    const void* shadow;   // the bf16 shadow the captured kernels read / write
    float beta_kl, b1, b2, aeps;
    hipGraphExec_t exec;
  };
  std::vector<TrainGraph> tgraphs;
  static constexpr int kDynSlots = 64;
  MmadDyn* dyn_host = nullptr;
  hipEvent_t dyn_ev[kDynSlots] = {};
  bool dyn_used[kDynSlots] = {};
  int dyn_next = 0;
  bool capturing = false;
  bool graph_broken = false;
  // workspace whose split-K control block this handle has zeroed
  const void* ws_zeroed = nullptr;
  void clear_train_graphs() {
    for (auto& g : tgraphs) (void)hipGraphExecDestroy(g.exec);
    tgraphs.clear();
  }
  ~mmad_ae() {
    clear_train_graphs();
    for (auto e : dyn_ev)
      if (e) (void)hipEventDestroy(e);
    if (dyn_host) (void)hipHostFree(dyn_host);
    for (auto e : probe_ev) (void)hipEventDestroy(e);
    if (probe_sync) (void)hipEventDestroy(probe_sync);
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
    for (auto& g : ographs) (void)hipGraphExecDestroy(g.exec);
    if (gstream) (void)hipStreamDestroy(gstream);
    for (auto e : ev_fork) (void)hipEventDestroy(e);
    for (auto e : ev_data) (void)hipEventDestroy(e);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (ev_hold) (void)hipEventDestroy(ev_hold);
    if (ev_loss) (void)hipEventDestroy(ev_loss);
    for (auto e : ev_dw) (void)hipEventDestroy(e);
    for (auto e : ev_xdw) (void)hipEventDestroy(e);
    for (auto e : ev_xdata) (void)hipEventDestroy(e);
    if (ev_small) (void)hipEventDestroy(ev_small);
    if (ev_cdone) (void)hipEventDestroy(ev_cdone);
    if (cstream) (void)hipStreamDestroy(cstream);
    if (side) (void)hipStreamDestroy(side);
  }
};

struct LayerWS {
  void *out, *y, *dy, *dz;
  float *stats, *mean, *rstd, *scale, *shift, *dbpart, *rowsq;
  float* ref32;     // x3 scoring: fp32 copy of an encoder layer's pass-1 output (else null)
  double* bnpart;   // fp64 BN-backward column partials [Mp/64][2][Np]
  // consumer of a train-mode BN producer: W*scale (GEMM dtype) and the
  // per-64-column partials of sum_k shift[k] W[n][k]
  void* wf;
  float* cpart;
  // this call: BN of the layer fused into its forward GEMM / into the
  // bwd-data GEMM of the next layer (bias gradient partials per 64 rows)
  bool fwd_fused, bwd_fused;
  unsigned* sync_f;   // fused-BN barrier counters (MMAD_BN_SYNC_WORDS each)
  unsigned* sync_b;
};
struct AeWS {
  int B, k, Mpe, Mpd;
  MmadDyn* dyn_dev = nullptr;    // device slot for the per-call values (graph-captured step)
  const MmadDyn* dyn = nullptr;  // set: kernels read x / loss / noise / Adam terms from dyn_dev
  void *xin, *zbuf, *dzin;
  float *eps, *klpart, *misc, *lossp;
  int64_t kl_parts;
  // split-K workspace per stream (0 = caller's stream, 1 = side stream);
  // the two control blocks are contiguous (one memset per call)
  float* sk_slab[2];
  unsigned* sk_ctl[2];
  size_t sk_ctl_bytes;   // both split-K control blocks + the fused-BN counters
  unsigned* bn_err;      // fused-BN barrier timeout word
  int bn_mode;           // this call's train-mode BN schedule (0 apply, 1 fold, 2 fused)
  int bn_mode_bwd;       // ... of the backward (2: fused into the bwd-data GEMMs; else the apply kernel)
  // this call's fused-step schedule: ping-pong the bf16 weight shadows (the
  // Adam of layer l writes the shadow the NEXT step reads, so dW_l waits only
  // for dz_l) and how many of the last dW GEMMs run on the main stream
  bool ping = false;
  int dw_main = 2;
  std::vector<LayerWS> l;
  // streamed NAP (a fit attached, else null): the packed operand [Mpe][nap.Kp]
  // (fp32, or bf16 planes [2][Mpe][nap.Kp]) and the NAP GEMM's row partials
  void* nap_x = nullptr;
  float* nap_rowsq = nullptr;
  int64_t nap_x_off = -1;   // byte offset of nap_x in the workspace
  int64_t bytes;
};

static size_t esz(int dtype) { return dtype == MMAD_BF16 ? 2 : 4; }

// can the dispatcher choose a split-K factor > 1 for this handle's GEMMs?
// (any dtype: a forced override, knob 4; bf16: the dW rule, when a dW
// override or the dW split target is set; fp32: knob 32's dW rule -- by
// default nothing splits)
static bool splitk_possible(int dtype) {
  const int o = mmad_splitk_override();
  if (o > 1) return true;
  if (o == 1) return false;
  if (dtype != MMAD_BF16) return mmad_splitk_dw_f32_blocks() > 0;
  return mmad_splitk_dw_override() > 1 || mmad_splitk_dw_blocks() > 0;
}

static void carve(const mmad_ae* h, int B, int k, char* base, AeWS& w) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) -> char* {
    off = (off + 255) / 256 * 256;
    char* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  };
  const size_t es = esz(h->dtype);
  {
    // split-K control words first: at a batch-independent offset, so
    // mmad_ae_status can find them whatever batch the last call used
    size_t slab = 0, ctl = 0;
    mmad_gemm_splitk_bytes(0, 0, &slab, &ctl);
    ctl = (ctl + 255) / 256 * 256;
    // + fused-BN barrier counters: 2 blocks per layer, then the error word
    const size_t bn_ctl = ((size_t)(2 * h->L.size() * MMAD_BN_SYNC_WORDS + 64) * 4 + 255) / 256 * 256;
    w.sk_ctl_bytes = 2 * ctl + bn_ctl;
    char* c = take((int64_t)w.sk_ctl_bytes);
    w.sk_ctl[0] = (unsigned*)c;
    w.sk_ctl[1] = c ? (unsigned*)(c + ctl) : nullptr;
    unsigned* bc = c ? (unsigned*)(c + 2 * ctl) : nullptr;
    w.bn_err = bc ? bc + 2 * h->L.size() * MMAD_BN_SYNC_WORDS : nullptr;
    w.l.resize(h->L.size());
    for (size_t i = 0; i < h->L.size(); ++i) {
      w.l[i].sync_f = bc ? bc + (2 * i) * MMAD_BN_SYNC_WORDS : nullptr;
      w.l[i].sync_b = bc ? bc + (2 * i + 1) * MMAD_BN_SYNC_WORDS : nullptr;
      w.l[i].fwd_fused = w.l[i].bwd_fused = false;
    }
  }
  w.B = B;
  w.k = k;
  w.Mpe = mmad_roundup(B, MMAD_PAD);
  w.Mpd = mmad_roundup(B * k, MMAD_PAD);
  const int nL = (int)h->L.size();
  w.xin = take((int64_t)w.Mpe * h->L[0].Kp * es);
  w.zbuf = w.dzin = nullptr;
  w.eps = w.klpart = nullptr;
  w.kl_parts = 0;
  if (h->vib) {
    const AeLayer& d0 = h->L[h->n_enc];
    w.zbuf = take((int64_t)w.Mpd * d0.Kp * es);
    w.dzin = take((int64_t)w.Mpd * d0.Kp * es);
    w.eps = (float*)take((int64_t)k * B * h->btl * 4);
    w.kl_parts = mmad_vib_kl_parts(B, k, d0.Kp);
    w.klpart = (float*)take(w.kl_parts * 4);
  }
  w.misc = (float*)take(1024 * 4);
  w.dyn_dev = (MmadDyn*)take(sizeof(MmadDyn));
  w.dyn = nullptr;
  {
    // the split-K partial slabs (54.5 MB per stream) only when the current
    // knobs let the dispatcher split one of this handle's GEMMs; without a
    // slab it never splits.  Sized per call from the knobs in force, so a
    // later override grows the workspace the next size query reports (and a
    // caller that skipped the query gets "workspace too small", not an overrun)
    size_t slab = 0, ctl = 0;
    if (splitk_possible(h->dtype)) mmad_gemm_splitk_bytes(0, 0, &slab, &ctl);
    w.sk_slab[0] = slab ? (float*)take((int64_t)slab) : nullptr;
    w.sk_slab[1] = slab ? (float*)take((int64_t)slab) : nullptr;
  }
  {
    const AeLayer& last = h->L[nL - 1];
    w.lossp = (float*)take((int64_t)(w.Mpd / 64) * (last.Np / 64) * 4);
  }
  for (int i = 0; i < nL; ++i) {
    const AeLayer& a = h->L[i];
    const int Mp = a.enc ? w.Mpe : w.Mpd;
    const int64_t mat = (int64_t)Mp * a.Np * es;
    LayerWS& s = w.l[i];
    s.out = take(mat);
    s.y = a.bn ? take(mat) : nullptr;
    s.dy = take(mat);
    s.dz = a.bn ? take(mat) : nullptr;
    s.stats = (float*)take((int64_t)(Mp / MMAD_PART_ROWS) * 2 * a.Np * 4);
    s.mean = (float*)take(a.Np * 4);
    s.rstd = (float*)take(a.Np * 4);
    s.scale = (float*)take(a.Np * 4);
    s.shift = (float*)take(a.Np * 4);
    s.bnpart = (double*)take((int64_t)(Mp / 64) * 2 * a.Np * 8);
    s.dbpart = (float*)take((int64_t)(Mp / 64) * a.Np * 4);   // 128-row (apply) or 64-row (fused) parts
    s.rowsq = (float*)take((int64_t)(a.Np / 128) * Mp * 4);
    const bool folded = i > 0 && h->L[i - 1].bn;
    s.wf = folded ? take((int64_t)a.Np * a.Kp * es) : nullptr;
    s.cpart = folded ? (float*)take((int64_t)(a.Kp / 64) * a.Np * 4) : nullptr;
  }
  // x3 scoring: the fp32 references of pass 2, after every other buffer (no
  // existing offset moves when planes are attached or detached)
  for (int i = 0; i < nL; ++i) {
    const AeLayer& a = h->L[i];
    w.l[i].ref32 = (h->planes && a.enc) ? (float*)take((int64_t)w.Mpe * a.Np * 4) : nullptr;
  }
  // streamed NAP: after those, so neither attachment moves the other's offsets
  // (both element types fill the same bytes: 4 per operand element)
  w.nap_x = nullptr;
  w.nap_rowsq = nullptr;
  w.nap_x_off = -1;
  if (h->nap.on) {
    w.nap_x = take((int64_t)w.Mpe * h->nap.Kp * 4);
    w.nap_x_off = off - (int64_t)w.Mpe * h->nap.Kp * 4;
    w.nap_rowsq = (float*)take((int64_t)(h->nap.Rp / 128) * w.Mpe * 4);
  }
  w.bytes = (off + 255) / 256 * 256;
}

// ---------------------------------------------------------------------------
int mmad_ae_create(mmad_ae** out, int dtype, int n_enc, const int* enc_widths, int n_dec,
                   const int* dec_widths, int vib, float slope, float bn_eps, float bn_momentum) {
  MMAD_CHECK_ARG(out != nullptr, "ae_create: null out");
  *out = nullptr;
  MMAD_CHECK_ARG(dtype == MMAD_F32 || dtype == MMAD_BF16, "ae_create: bad dtype %d", dtype);
  MMAD_CHECK_ARG(n_enc >= 1 && n_dec >= 1 && enc_widths && dec_widths, "ae_create: bad layers");
  for (int i = 0; i <= n_enc; ++i) MMAD_CHECK_ARG(enc_widths[i] >= 1, "ae_create: bad enc width");
  for (int i = 0; i <= n_dec; ++i) MMAD_CHECK_ARG(dec_widths[i] >= 1, "ae_create: bad dec width");
  MMAD_CHECK_ARG(dec_widths[n_dec] == enc_widths[0], "ae_create: decoder must reconstruct input");
  if (vib)
    MMAD_CHECK_ARG(enc_widths[n_enc] == 2 * dec_widths[0],
                   "ae_create: VIB encoder output must be 2*btl");
  else
    MMAD_CHECK_ARG(enc_widths[n_enc] == dec_widths[0], "ae_create: bottleneck mismatch");
  mmad_ae* h = new mmad_ae();
  h->dtype = dtype;
  h->n_enc = n_enc;
  h->n_dec = n_dec;
  h->vib = vib;
  h->btl = dec_widths[0];
  h->slope = slope;
  h->bn_eps = bn_eps;
  h->bn_mom = bn_momentum;
  {
    // the schedule knobs (include/mmad.h 16-27), read once for this handle
    const int m = mmad_knob(16);
    h->fold = dtype == MMAD_BF16;
    h->bn_mode = dtype == MMAD_BF16 ? 2 : 0;
    if (m >= 0 && m <= 2) {
      h->bn_mode = m;
      h->fold = m != 0 && dtype == MMAD_BF16;   // fold: mode 1, mode 2's fallback
    }
    h->bn_mode_bwd = mmad_knob(17);
    h->bn_fused_rows = mmad_knob(18);
    h->dw_main = mmad_knob(19);
    h->pair_rows = mmad_knob(20);
    h->dw_main_ping = mmad_knob(21);
    h->ev_every = mmad_knob(22);
    h->ev_on_kernel = mmad_knob(31);
    h->loss_side = mmad_knob(23);
    h->dp_small_at = mmad_knob(24);
    h->keep_grads = mmad_knob(25);
    h->side_prio_hi = mmad_knob(26);
    h->side_cu_held = mmad_knob(15);
    h->dp_shard = mmad_knob(28);
    h->side_hold = mmad_knob(29);
    h->dw_late = mmad_knob(33);
    h->fork_on_kernel = mmad_knob(34);
    h->fork_pair_below = mmad_knob(35);
    h->dp_bucket_mib = mmad_knob(30) < 0 ? 0 : mmad_knob(30);
    h->dp_fork_rows = mmad_knob(14);
    h->ev_flags_ = ev_flags(mmad_knob(27));
  }
  for (int side = 0; side < 2; ++side) {
    const int n = side == 0 ? n_enc : n_dec;
    const int* wd = side == 0 ? enc_widths : dec_widths;
    for (int i = 0; i < n; ++i) {
      AeLayer a{};
      a.K = wd[i];
      a.N = wd[i + 1];
      a.Kp = mmad_roundup(a.K, MMAD_PAD);
      a.Np = mmad_roundup(a.N, MMAD_PAD);
      a.bn = i < n - 1;
      a.act = a.bn ? MMAD_ACT_LEAKYRELU : MMAD_ACT_NONE;
      a.enc = side == 0;
      h->L.push_back(a);
    }
  }
  int64_t off = 0;
  for (auto& a : h->L) { a.w_off = off; off += (int64_t)a.Np * a.Kp; }
  h->n_weight = off;
  int64_t bn = 0;
  for (auto& a : h->L) {
    a.b_off = off; off += a.Np;
    a.g_off = a.be_off = a.bn_off = -1;
    if (a.bn) {
      a.g_off = off; off += a.Np;
      a.be_off = off; off += a.Np;
      a.bn_off = bn; bn += a.Np;
    }
  }
  h->n_params = off;
  h->n_bn = bn;
  *out = h;
  return MMAD_OK;
}

void mmad_ae_destroy(mmad_ae* h) { delete h; }

int mmad_ae_layout(const mmad_ae* h, int64_t* info, int64_t* totals) {
  MMAD_CHECK_ARG(h && info && totals, "ae_layout: null arg");
  for (size_t i = 0; i < h->L.size(); ++i) {
    const AeLayer& a = h->L[i];
    int64_t* r = info + 7 * i;
    r[0] = a.w_off; r[1] = a.b_off; r[2] = a.g_off; r[3] = a.be_off;
    r[4] = a.Kp; r[5] = a.Np; r[6] = a.bn_off;
  }
  totals[0] = h->n_params;
  totals[1] = h->n_weight;
  totals[2] = h->n_bn;
  totals[3] = (int64_t)h->L.size();
  return MMAD_OK;
}

int64_t mmad_ae_workspace_bytes(const mmad_ae* h, int B, int k) {
  if (!h || B < 1 || k < 1) return -1;
  AeWS w;
  carve(h, B, k, nullptr, w);
  return w.bytes;
}

int mmad_ae_bind(mmad_ae* h, float* params, float* grads, float* adam_m, float* adam_v,
                 void* shadow, float* running) {
  MMAD_CHECK_ARG(h && params, "ae_bind: null params");
  MMAD_CHECK_ARG(h->dtype != MMAD_BF16 || shadow, "ae_bind: bf16 needs a shadow buffer");
  h->clear_train_graphs();   // captured steps bake the buffer addresses in
  h->params = params;
  h->grads = grads;
  h->m = adam_m;
  h->v = adam_v;
  h->shadow = shadow;
  h->running = running;
  h->planes_stale = true;
  if (!h->side) {
    // lowest priority: the side stream fills CUs the critical chain leaves idle
    int least = 0, greatest = 0;
    MMAD_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    // (knob 26: the highest priority instead, for schedule sweeps)
    if (h->side_cu_held > 0) {
      // schedule study: the side stream's dW + Adam GEMMs kept off side_cu_held
      // CUs so the bwd-data / BN-apply chain always has CUs of its own.  The
      // masked stream is created blocking at the default priority (the API
      // takes neither), so the caller's stream must be a created non-blocking
      // one, not the legacy null stream, or every side launch serialises
      int dev = 0, ncu = 0;
      MMAD_HIP_CHECK(hipGetDevice(&dev));
      MMAD_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
      const int held = std::min(h->side_cu_held, ncu - 1), stride = std::max(1, ncu / std::max(1, held));
      std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
      for (int i = 0, n_held = 0; i < ncu; ++i) {
        const bool hold = n_held < held && i % stride == stride - 1;
        n_held += hold;
        if (!hold) mask[i / 32] |= 1u << (i % 32);
      }
      MMAD_HIP_CHECK(hipExtStreamCreateWithCUMask(&h->side, (uint32_t)mask.size(), mask.data()));
    } else {
      MMAD_HIP_CHECK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking,
                                                 h->side_prio_hi ? greatest : least));
    }
    const size_t n = h->L.size();
    h->ev_fork.resize(n);
    h->ev_data.resize(n);
    for (size_t i = 0; i < n; ++i) {
      MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_fork[i], h->ev_flags_));
      MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_data[i], h->ev_flags_));
    }
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_join, h->ev_flags_));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_hold, h->ev_flags_));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_loss, h->ev_flags_));
  }
  return MMAD_OK;
}

int mmad_ae_set_shadow_pair(mmad_ae* h, void* alt) {
  MMAD_CHECK_ARG(h && h->params, "ae_set_shadow_pair: unbound");
  MMAD_CHECK_ARG(!alt || h->dtype == MMAD_BF16, "ae_set_shadow_pair: bf16 handles only");
  MMAD_CHECK_ARG(alt != h->shadow, "ae_set_shadow_pair: alt aliases the shadow");
  h->shadow_alt = alt;
  return MMAD_OK;
}

const void* mmad_ae_current_shadow(const mmad_ae* h) { return h ? h->shadow : nullptr; }

// dtype of the eval forward / score GEMMs
static int score_dt(const mmad_ae* h) { return h->planes ? MMAD_BF16X3 : h->dtype; }

// re-split the weight region into the score planes if a weight write may have
// happened since the last split (one launch on the caller's stream)
static int refresh_planes(mmad_ae* h, hipStream_t st, bool force = false) {
  if (!h->planes || !(h->planes_stale || force)) return MMAD_OK;
  RET_IF(mmad_split_planes(h->n_weight, h->params, h->planes, (char*)h->planes + h->n_weight * 2, st));
  h->planes_stale = false;
  return MMAD_OK;
}

int mmad_ae_set_score_planes(mmad_ae* h, void* planes) {
  MMAD_CHECK_ARG(h, "ae_set_score_planes: null handle");
  MMAD_CHECK_ARG(h->dtype == MMAD_F32, "ae_set_score_planes: fp32 handles only (a bf16 handle "
                 "scores on its own shadow)");
  MMAD_CHECK_ARG(((uintptr_t)planes) % 16 == 0, "ae_set_score_planes: planes must be 16-byte aligned");
  h->planes = planes;
  h->planes_stale = true;
  return mmad_ae_clear_graphs(h);   // captured passes bake the operand dtype and addresses in
}

int mmad_ae_score_dtype(const mmad_ae* h) { return h ? score_dt(h) : -1; }

// first column of diff layer j in the concatenated diffs (j = n_enc + 1: their width)
static int diff_col(const mmad_ae* h, int j) {
  int c = 0;
  for (int i = 0; i < j; ++i) c += i == 0 ? h->L[0].K : h->L[i - 1].N;
  return c;
}

int mmad_ae_set_nap(mmad_ae* h, int start, int end, int R, const float* vt, const float* bias,
                    const float* w, int dtype, void* vt_planes, void* stream) {
  MMAD_CHECK_ARG(h, "ae_set_nap: null handle");
  if (!vt) {   // detach
    if (h->nap.on) {
      h->nap = mmad_ae::NapFit{};
      return mmad_ae_clear_graphs(h);
    }
    return MMAD_OK;
  }
  MMAD_CHECK_ARG(start >= 0 && end > start && end <= h->n_enc + 1,
                 "ae_set_nap: bad layer range [%d, %d) of %d diff layers", start, end, h->n_enc + 1);
  MMAD_CHECK_ARG(R >= 1 && bias && w, "ae_set_nap: bad fit (R=%d, null bias / w)", R);
  MMAD_CHECK_ARG(dtype == MMAD_F32 || dtype == MMAD_BF16X3,
                 "ae_set_nap: the NAP GEMM runs as MMAD_F32 or MMAD_BF16X3 (dtype %d)", dtype);
  mmad_ae::NapFit f;
  f.on = true;
  f.start = start;
  f.end = end;
  f.K = diff_col(h, end) - diff_col(h, start);
  f.Kp = mmad_roundup(f.K, MMAD_PAD);
  f.R = R;
  f.Rp = mmad_roundup(R, MMAD_PAD);
  f.dtype = dtype;
  f.vt = vt;
  f.bias = bias;
  f.w = w;
  if (dtype == MMAD_BF16X3) {
    MMAD_CHECK_ARG(score_dt(h) == MMAD_BF16X3, "ae_set_nap: an MMAD_BF16X3 NAP GEMM needs score planes "
                   "attached (mmad_ae_set_score_planes): its operand is written by the x3 score GEMMs");
    MMAD_CHECK_ARG(vt_planes && ((uintptr_t)vt_planes) % 16 == 0 && ((uintptr_t)vt) % 16 == 0,
                   "ae_set_nap: MMAD_BF16X3 needs 16-byte aligned vt and vt_planes");
    f.vt_planes = vt_planes;
    const int64_t n = (int64_t)f.Rp * f.Kp;
    RET_IF(mmad_split_planes(n, vt, vt_planes, (char*)vt_planes + n * 2, stream));
  }
  h->nap = f;
  return mmad_ae_clear_graphs(h);   // captured passes bake the operand layout and the fit's addresses in
}

int mmad_ae_nap_operand(const mmad_ae* h, int B, int64_t* info) {
  MMAD_CHECK_ARG(h && info && B >= 1, "ae_nap_operand: bad arguments");
  MMAD_CHECK_ARG(h->nap.on, "ae_nap_operand: no NAP fit attached");
  AeWS w;
  carve(h, B, 1, nullptr, w);
  info[0] = w.nap_x_off;
  info[1] = w.Mpe;
  info[2] = h->nap.Kp;
  info[3] = h->nap.K;
  info[4] = h->nap.dtype;
  return MMAD_OK;
}

int mmad_ae_sync_shadow(mmad_ae* h, void* stream) {
  MMAD_CHECK_ARG(h && h->params, "ae_sync_shadow: unbound");
  if (h->dtype != MMAD_BF16) return refresh_planes(h, (hipStream_t)stream, true);
  if (h->shadow_alt) RET_IF(mmad_to_bf16(h->n_weight, h->params, h->shadow_alt, stream));
  return mmad_to_bf16(h->n_weight, h->params, h->shadow, stream);
}

// the shadow the fused step's Adam writes (bf16 only)
static void* adam_shadow(const mmad_ae* h, const AeLayer& a, bool ping) {
  if (h->dtype != MMAD_BF16) return nullptr;
  return (char*)(ping && h->shadow_alt ? h->shadow_alt : h->shadow) + a.w_off * 2;
}

// ---------------------------------------------------------------------------
static const void* weights(const mmad_ae* h, const AeLayer& a) {
  if (h->dtype == MMAD_BF16) return (const char*)h->shadow + a.w_off * 2;
  return h->params + a.w_off;
}
// the weight operand of an eval / score GEMM of dtype dt: for MMAD_BF16X3 the
// layer's hi plane, with its lo plane (n_weight elements on) set in ep
static const void* weights_dt(const mmad_ae* h, const AeLayer& a, int dt, GemmEpi& ep) {
  if (dt != MMAD_BF16X3) return weights(h, a);
  ep.b_lo = (const char*)h->planes + (h->n_weight + a.w_off) * 2;
  return (const char*)h->planes + a.w_off * 2;
}

// input of layer l; in train mode a BN producer's output stays pre-BN (a): the
// forward reads it against the folded weights, the dW GEMM fixes up with
// (scale, shift) in its epilogue
static const void* input_of(const mmad_ae* h, const AeWS& w, int l, bool train,
                            const float** scale, const float** shift) {
  *scale = *shift = nullptr;
  if (l == 0) return w.xin;
  if (h->vib && l == h->n_enc) return w.zbuf;
  const AeLayer& p = h->L[l - 1];
  const LayerWS& ps = w.l[l - 1];
  if (!p.bn) return ps.out;
  if (!train || w.bn_mode != 1) return ps.y;
  *scale = ps.scale;
  *shift = ps.shift;
  return ps.out;
}


static int prepare_ws(const mmad_ae* h, int B, int k, void* ws, int64_t ws_bytes, AeWS& w,
                      hipStream_t st) {
  MMAD_CHECK_ARG(B >= 1 && k >= 1, "bad batch B=%d k=%d", B, k);
  MMAD_CHECK_ARG(h->vib || k == 1, "k>1 needs the VIB head");
  carve(h, B, k, (char*)ws, w);
  MMAD_CHECK_ARG(ws && ws_bytes >= w.bytes, "workspace too small (%lld < %lld bytes)",
                 (long long)ws_bytes, (long long)w.bytes);
  MMAD_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "workspace must be 256-byte aligned");
  // split-K arrival counters / flags must be zero before a split GEMM runs;
  // every split GEMM leaves them zero again, so a workspace is zeroed once
  // when this handle first sees it (and mmad_ae_status re-zeroes after a
  // timed-out combine); only when a split can be chosen at all
  w.bn_mode = h->bn_mode;
  w.ping = false;
  w.dw_main = h->dw_main;
  if (w.bn_mode == 2 && w.Mpd > h->bn_fused_rows) w.bn_mode = h->fold ? 1 : 0;
  if (w.bn_mode == 1 && !h->fold) w.bn_mode = 0;
  w.bn_mode_bwd = (h->bn_mode_bwd >= 0 && h->fold) ? h->bn_mode_bwd : w.bn_mode;
  if ((splitk_possible(h->dtype) || h->bn_mode == 2 || h->bn_mode_bwd == 2) &&
      ws != h->ws_zeroed) {
    MMAD_HIP_CHECK(hipMemsetAsync(w.sk_ctl[0], 0, w.sk_ctl_bytes, st));
    const_cast<mmad_ae*>(h)->ws_zeroed = ws;
  }
  return MMAD_OK;
}

// probe ids: PROBE_FWD + layer (forward / MSE / score GEMM of the layer),
// PROBE_DW + layer (its dW GEMM, with the fused Adam in the fused step)
enum { PROBE_FWD = 0, PROBE_DW = 64 };

// GEMM dispatch with the split-K workspace of the stream it runs on
// data-parallel weight buckets: walking the layers in backward order,
// consecutive layers join one bucket until it holds >= dp_bucket_mib MiB of
// fp32 gradient (layer 0 always closes the last).  The weights are one
// contiguous buffer in layer order, so a bucket of layers l_lo..l_hi is the
// range [w_off(l_lo), w_off(l_hi) + Np * Kp).  Fewer, larger buckets: fewer
// exchange calls and events on the host (the DP step was host-bound with one
// bucket per layer, profiles/r03z_*) and larger collectives.  The step and
// mmad_ae_dp_sync_master use the same plan; a sharded bucket's rank-r slice is
// [r * n / N, (r + 1) * n / N).  last_of[l] = the bucket whose lowest layer is
// l (-1 if none).
struct DpBucket {
  int l_hi, l_lo;
  int64_t off, n;
};
static void dp_plan(const mmad_ae* h, std::vector<DpBucket>& out) {
  out.clear();
  const int nL = (int)h->L.size();
  const int64_t min_n = (int64_t)h->dp_bucket_mib * (1 << 20) / 4;
  int hi = nL - 1;
  int64_t acc = 0;
  for (int l = nL - 1; l >= 0; --l) {
    acc += (int64_t)h->L[l].Np * h->L[l].Kp;
    if (acc >= min_n || l == 0) {
      out.push_back(DpBucket{hi, l, h->L[l].w_off, acc});
      hi = l - 1;
      acc = 0;
    }
  }
}

static int ae_gemm(const mmad_ae* h, const AeWS& w, int dt, int epi, const void* A, int lda,
                   const void* B, int ldb, int Mp, int Np, int K, GemmEpi ep, hipStream_t s,
                   int* cfg = nullptr, int probe = -1) {
  const int r = (h->side && s == h->side) ? 1 : 0;
  ep.sk_slab = w.sk_slab[r];
  ep.sk_ctl = w.sk_ctl[r];
  const bool rec = probe >= 0 && probe == h->probe_id && !h->capturing &&
                   2 * h->probe_n < (int)h->probe_ev.size();
  if (rec && !h->probe_kev && h->side && s != h->side && h->probe_sync) {
    // a probed main-stream launch starts its clock once the side stream's
    // earlier GEMMs are done: its blocks (a whole CU's LDS each on the tail
    // tiles) wait for those CUs anyway, and the event pair then brackets the
    // launch's own execution, first dispatch to completion, as rocprofv3's
    // kernel records do (without it the pair also held ~4 us of that wait on
    // the c2 tail: 31.2 vs 26.8 us, profiles/r08o_prof_c2)
    MMAD_HIP_CHECK(hipEventRecord(h->probe_sync, h->side));
    MMAD_HIP_CHECK(hipStreamWaitEvent(s, h->probe_sync, 0));
  }
  // kernel-attached events only where the launch carries no hand-off event
  const bool kev = rec && h->probe_kev && !ep.done_ev;
  if (kev) {
    ep.start_ev = h->probe_ev[2 * h->probe_n];
    ep.done_ev = h->probe_ev[2 * h->probe_n + 1];
  } else if (rec) {
    MMAD_HIP_CHECK(hipEventRecord(h->probe_ev[2 * h->probe_n], s));
  }
  const int rc = mmad_gemm_dispatch(dt, epi, A, lda, B, ldb, Mp, Np, K, ep, s, cfg);
  if (rc != MMAD_OK) return rc;
  if (rec) {
    if (!kev) MMAD_HIP_CHECK(hipEventRecord(h->probe_ev[2 * h->probe_n + 1], s));
    ++h->probe_n;
    h->probe_mask = 1u << (probe % 64);
  }
  return MMAD_OK;
}

// Which side-stream dW + Adam GEMMs share a grouped launch.  Layers l_hi - 1
// down to l_lo are visited in backward order; consecutive layers the tile
// rule (mmad_tile_adam_for) puts on the 64x64 tile, with at most budget / 2
// padded blocks each, join the open group while it stays within `budget`
// padded blocks and `members` members; any other layer, or one that would not
// fit, closes it.  group_of[l] = the group's
// index (in launch order), or -1 for a layer with a launch of its own (a group
// of one is the ordinary launch).  Returns the number of groups.  A function
// of its arguments and knob 5 only.
int mmad_dw_group_plan(int n_layers, const int* Np, const int* Kp, const int* rows, int l_lo, int l_hi,
                       int budget, int members, int* group_of) {
  if (n_layers <= 0 || !Np || !Kp || !rows || !group_of) return 0;
  for (int l = 0; l < n_layers; ++l) group_of[l] = -1;
  if (members > MMAD_GEMM_GROUP_MAX) members = MMAD_GEMM_GROUP_MAX;
  if (budget <= 0 || members < 2) return 0;
  int groups = 0, first = -1, count = 0, blocks = 0;
  auto close = [&]() {
    if (count >= 2) {
      for (int m = first; m > first - count; --m) group_of[m] = groups;
      ++groups;
    }
    first = -1;
    count = blocks = 0;
  };
  for (int l = (l_hi < n_layers ? l_hi : n_layers) - 1; l >= (l_lo > 0 ? l_lo : 0); --l) {
    const bool fits_tile = Np[l] > 0 && Kp[l] > 0 && Np[l] % 64 == 0 && Kp[l] % 64 == 0 &&
                           mmad_tile_adam_for(Np[l], Kp[l], rows[l]) == 3;
    const int bl = fits_tile ? mmad_gemm_group_blocks(Np[l], Kp[l]) : 0;
    // a member takes at most half the budget: with the budget at one resident
    // round (two blocks per CU) a larger launch has a block on every CU and is
    // bound by throughput, not by one block's latency -- held back for a
    // group it would only start later (c3: layer 7, 280 blocks; layer 2, 352)
    if (!fits_tile || 2 * bl > budget) {
      close();
      continue;
    }
    if (count == members || blocks + bl > budget) close();
    if (count == 0) first = l;
    ++count;
    blocks += bl;
  }
  close();
  return groups;
}

// a side-stream dW GEMM of the backward waiting to be issued (run_backward)
struct PendingDW {
  const void *dz, *in;
  int lda, ldb, M, N, K;
  GemmEpi ep;
  int layer;
};

// the grouped form of ae_gemm for `n` deferred side-stream dW GEMMs: one
// launch, or MMAD_GEMM_GROUP_REFUSED with nothing launched.  The probe of any
// member's PROBE_DW id brackets the whole launch; the mask names every member.
static int ae_gemm_group(const mmad_ae* h, const AeWS& w, int dt, const PendingDW* q, int n, hipStream_t s) {
  if (n > MMAD_GEMM_GROUP_MAX) return MMAD_GEMM_GROUP_REFUSED;
  const int r = (h->side && s == h->side) ? 1 : 0;
  GemmGroupProblem gp[MMAD_GEMM_GROUP_MAX];
  unsigned mask = 0;
  bool hit = false;
  for (int i = 0; i < n; ++i) {
    gp[i] = GemmGroupProblem{q[i].dz, q[i].in, q[i].lda, q[i].ldb, q[i].M, q[i].N, q[i].K, q[i].ep};
    gp[i].ep.sk_slab = w.sk_slab[r];
    gp[i].ep.sk_ctl = w.sk_ctl[r];
    mask |= 1u << (q[i].layer % 32);
    hit = hit || PROBE_DW + q[i].layer == h->probe_id;
  }
  const bool rec = hit && !h->capturing && 2 * h->probe_n < (int)h->probe_ev.size();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (rec && h->probe_kev) {
    e0 = h->probe_ev[2 * h->probe_n];
    e1 = h->probe_ev[2 * h->probe_n + 1];
  } else if (rec) {
    MMAD_HIP_CHECK(hipEventRecord(h->probe_ev[2 * h->probe_n], s));
  }
  const int rc = mmad_gemm_dispatch_group(dt, n, gp, s, e1, e0);
  if (rc != MMAD_OK) return rc;
  if (rec) {
    if (!h->probe_kev) MMAD_HIP_CHECK(hipEventRecord(h->probe_ev[2 * h->probe_n + 1], s));
    ++h->probe_n;
    h->probe_mask = mask;
  }
  return MMAD_OK;
}

static inline int rows_of(const AeWS& w, const AeLayer& a) { return a.enc ? w.B : w.B * w.k; }
static inline int prows_of(const AeWS& w, const AeLayer& a) { return a.enc ? w.Mpe : w.Mpd; }
static float* running_mean(const mmad_ae* h, const AeLayer& a) { return h->running + a.bn_off; }
static float* running_var(const mmad_ae* h, const AeLayer& a) {
  return h->running + h->n_bn + a.bn_off;
}

static GemmEpi fwd_epi(const mmad_ae* h, const AeWS& w, const AeLayer& a, const LayerWS& s,
                       int M, void* out, bool folded) {
  GemmEpi ep{};
  ep.M = M;
  ep.N = a.N;
  ep.out = out;
  ep.ldo = a.Np;
  ep.bias = h->params + a.b_off;
  ep.act = a.act;
  ep.slope = h->slope;
  ep.ldpart = a.Np;
  if (folded) {
    ep.bpart = s.cpart;
    ep.bparts = a.Kp / 64;
    ep.bpstride = a.Np;
  }
  (void)w;
  return ep;
}

// mode 0 = train (MSE-fused last layer), 1 = eval, 2 = train BN, plain last layer
// mse_done (nullable): an event the train-mode MSE GEMM launch completes itself
static int run_forward(mmad_ae* h, AeWS& w, const float* x, int ld_x, int mode, const float* eps,
                       uint64_t seed, uint64_t offset, hipStream_t st, hipEvent_t mse_done = nullptr) {
  const int dt = mode == 1 ? score_dt(h) : h->dtype;
  const bool x3 = dt == MMAD_BF16X3;
  const int nL = (int)h->L.size();
  const int B = w.B, k = w.k;
  const bool train = mode != 1;
  RET_IF(mmad_pack_input_dyn(dt, B, h->L[0].K, w.Mpe, h->L[0].Kp, x, ld_x, w.xin, w.dyn, st));
  for (int l = 0; l < nL; ++l) {
    const AeLayer& a = h->L[l];
    LayerWS& s = w.l[l];
    const int M = rows_of(w, a), Mp = prows_of(w, a);
    const float *isc, *ish;
    const void* in = input_of(h, w, l, train, &isc, &ish);
    const bool folded = isc != nullptr;             // train mode, BN producer
    const void* wt = folded ? s.wf : weights(h, a);
    if (mode == 0 && l == nL - 1) {
      GemmEpi ep = fwd_epi(h, w, a, s, M, s.out, folded);
      ep.act = MMAD_ACT_NONE;
      ep.part = s.stats;
      ep.target = x;
      ep.ldt = ld_x;
      ep.tmod = B;
      ep.gscale = 2.0f / (float)k;
      ep.lossp = w.lossp;
      ep.dyn = w.dyn;
      ep.done_ev = mse_done;
      int cfg = 0;
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_MSE, in, a.Kp, wt, a.Kp, Mp, a.Np, a.Kp, ep, st, &cfg,
                     PROBE_FWD + l));
      h->mse_tiles = mmad_gemm_ntiles(cfg, Mp, a.Np);
    } else if (a.bn && train) {
      GemmEpi ep = fwd_epi(h, w, a, s, M, s.out, folded);
      ep.part = s.stats;
      s.fwd_fused = w.bn_mode == 2 && mmad_gemm_bn_fusable(dt, GEMM_EPI_FWD, Mp, a.Np);
      if (s.fwd_fused) {
        // BN finished inside the GEMM: a (for the backward) and y = BN(a)
        ep.bn_sync = s.sync_f;
        ep.bn_err = w.bn_err;
        ep.bn_gamma = h->params + a.g_off;
        ep.bn_beta = h->params + a.be_off;
        ep.bn_rmean = running_mean(h, a);
        ep.bn_rvar = running_var(h, a);
        ep.bn_mom = h->bn_mom;
        ep.bn_eps = h->bn_eps;
        ep.bn_save_mean = s.mean;
        ep.bn_save_rstd = s.rstd;
        ep.bn_y = s.y;
      }
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_FWD, in, a.Kp, wt, a.Kp, Mp, a.Np, a.Kp, ep, st, nullptr,
                     PROBE_FWD + l));
      if (s.fwd_fused) {
        // nothing left to launch
      } else if (w.bn_mode != 1) {
        // exact-fp32 path: normalise into y (the consumer GEMM and its dW read
        // y as the reference's layers do: no fold, no fix-up cancellation)
        RET_IF(mmad_bn_train_apply(dt, M, a.N, Mp, a.Np, s.out, s.stats, h->params + a.g_off,
                                   h->params + a.be_off, running_mean(h, a), running_var(h, a),
                                   h->bn_mom, h->bn_eps, s.mean, s.rstd, s.y, st));
      } else if (l + 1 < nL) {
        // statistics -> (scale, shift) -> folded into layer l+1's weights/bias
        const AeLayer& c = h->L[l + 1];
        LayerWS& cs = w.l[l + 1];
        RET_IF(mmad_bn_finalize_fold(dt, M, a.N, Mp, a.Np, s.stats, h->params + a.g_off,
                                     h->params + a.be_off, running_mean(h, a), running_var(h, a),
                                     h->bn_mom, h->bn_eps, s.mean, s.rstd, s.scale, s.shift,
                                     h->params + c.w_off, c.Np, cs.wf, cs.cpart, st));
      } else {
        RET_IF(mmad_bn_finalize(M, a.N, Mp, a.Np, s.stats, h->params + a.g_off,
                                h->params + a.be_off, running_mean(h, a), running_var(h, a),
                                h->bn_mom, h->bn_eps, s.mean, s.rstd, s.scale, s.shift, st));
      }
    } else if (a.bn) {
      RET_IF(mmad_bn_eval_affine(a.N, a.Np, h->params + a.g_off, h->params + a.be_off,
                                 running_mean(h, a), running_var(h, a), h->bn_eps, s.scale,
                                 s.shift, st));
      GemmEpi ep = fwd_epi(h, w, a, s, M, s.y, folded);
      ep.bn_scale = s.scale;
      ep.bn_shift = s.shift;
      const void* we = x3 ? weights_dt(h, a, dt, ep) : wt;
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_FWD, in, a.Kp, we, a.Kp, Mp, a.Np, a.Kp, ep, st, nullptr,
                     PROBE_FWD + l));
    } else {
      GemmEpi ep = fwd_epi(h, w, a, s, M, s.out, folded);
      const void* we = x3 ? weights_dt(h, a, dt, ep) : wt;
      if (x3 && l == nL - 1) {
        // x_hat also in fp32 (the layer's unused dy buffer): mmad_ae_forward
        // unpacks / reduces that copy, not the re-rounded planes
        ep.out32 = (float*)s.dy;
        ep.ld32 = a.Np;
      }
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_FWD, in, a.Kp, we, a.Kp, Mp, a.Np, a.Kp, ep, st, nullptr,
                     PROBE_FWD + l));
    }
    if (h->vib && l == h->n_enc - 1) {
      const AeLayer& d0 = h->L[h->n_enc];
      RET_IF(mmad_vib_reparam_fwd_dyn(dt, B, h->btl, k, s.out, a.Np, eps, w.eps, seed, offset,
                                      mode == 1 ? 1 : 0, w.zbuf, d0.Kp,
                                      mode == 0 ? w.klpart : nullptr, mode == 0 ? w.dyn : nullptr, st));
    }
  }
  return MMAD_OK;
}

// where the bias gradient partials of layer l live after the backward of l+1
struct BiasSrc { const float* src; int nparts, stride; };
static BiasSrc bias_src(const mmad_ae* h, const AeWS& w, int l, bool from_mse) {
  const AeLayer& a = h->L[l];
  const LayerWS& s = w.l[l];
  const int Mp = prows_of(w, a);
  const int nL = (int)h->L.size();
  if (l == nL - 1 && from_mse) return {s.stats, Mp / MMAD_PART_ROWS, 2 * a.Np};
  if (a.bn && s.bwd_fused) return {s.dbpart, Mp / 64, a.Np};   // fused bwd-data epilogue
  if (l == nL - 1 || a.bn || (h->vib && l == h->n_enc - 1)) return {s.dbpart, Mp / 128, a.Np};
  return {s.stats, Mp / MMAD_PART_ROWS, 2 * a.Np};  // bwd-data epilogue column sums
}

using AdamHyper = MmadAdamConsts;   // w1 = float(1 - beta1), w2 = float(1 - beta2), ...

static int finish_reductions(mmad_ae* h, AeWS& w, bool biases, bool from_mse, float beta_kl,
                             float* loss_out, hipStream_t st);

// One backward pass: the main-stream bwd-data chain (bwd_data_step), written
// once, and one of three dW policies hooked in before and after each step --
// plain (no Adam), data-parallel (Adam after the bucket's exchange) and fused
// (single GPU, Adam in the dW epilogue).  This is the state they share.
struct BwdRun {
  mmad_ae* h;
  AeWS& w;
  hipStream_t st, side;
  // non-null: the step's Adam update runs in the dW epilogues (fused) or
  // after each bucket's exchange (data parallel, h->comm)
  const AdamHyper* adam;
  // the last layer's dz and bias partials come from the MSE-fused forward
  // epilogue; otherwise the caller has packed dL/dx_hat into its dy buffer
  bool from_mse;
  // the side stream already waits for the MSE launch (the fused step's loss
  // reduction), so the top layer's dW needs no fork of its own
  bool side_after_mse;
  float beta_kl;
  float* dp_loss;                   // data parallel: the loss output (dp_small_bucket)
  int nL;
  bool fork_kev;                    // fork events ride the producing launch (knob 34)
  std::vector<PendingDW> pending;   // dW GEMMs waiting for a recorded event
  std::vector<char> fork_done;      // ev_fork[l] completed by the launch that produced dz_l
  // grouped dW launches (single-GPU ping-pong step only): grp[l] = the group
  // layer l's dW + Adam GEMM is issued with, -1 = a launch of its own
  std::vector<int> grp;
  std::vector<DpBucket> plan;       // data parallel: the exchange buckets (dp_plan)
  size_t next_bucket = 0;

  bool dp() const { return adam && h->comm; }
  bool fused() const { return adam && !h->comm; }
  // the exchange bucket still open (data parallel), and whether layer l closes it
  const DpBucket* open_bucket() const { return next_bucket < plan.size() ? &plan[next_bucket] : nullptr; }
  const DpBucket* closes_bucket(int l) const {
    return open_bucket() && open_bucket()->l_lo == l ? open_bucket() : nullptr;
  }
  // ping-pong shadows (bf16): the fused Adam of dW_l writes the other shadow,
  // so dW_l may start as soon as dz_l is complete
  bool ping(int l) const { return fused() && w.ping && l >= w.dw_main; }
  bool late(int l) const { return ping(l) && l >= nL - h->dw_late; }
  // does layer l's side-stream dW (ping) get a fork event of its own (knob 35)?
  bool fork_ev(int l) const {
    // a group forks once, at its lowest member
    if (grp[l] >= 0) return l == 0 || grp[l - 1] != grp[l];
    const int P = h->fork_pair_below;
    if (P <= 0 || l > P || l == w.dw_main) return true;
    return (P - l) % 2 == 1;
  }
  // does layer l's side-stream dW fork behind dz_l (ping, not late)?
  bool forks_at_dz(int l) const { return ping(l) && !late(l) && fork_ev(l); }
  // the top layer's dz is the MSE output, which the side stream has waited
  // for already (the loss reduction): no fork
  bool fork_none(int l) const {
    return ping(l) && !late(l) && l == nL - 1 && from_mse && side_after_mse && fork_kev;
  }
  // does someone wait for ev_data[l] (bwd-data of l done)?  The DP exchange
  // of the bucket l closes, and the fused step's side-stream dW GEMMs without
  // ping-pong shadows (every ev_every-th layer; the lowest side layer always
  // records, flushing the deferred ones)
  bool needs_data_ev(int l) const {
    if (dp()) return closes_bucket(l) != nullptr;
    if (!fused() || ping(l) || l < w.dw_main) return false;
    return h->ev_every <= 1 || l == w.dw_main || (l - w.dw_main) % h->ev_every == 0;
  }
};

// `ev` recorded on `from`, waited for on `to`
static int hand_off(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  MMAD_HIP_CHECK(hipEventRecord(ev, from));
  MMAD_HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
  return MMAD_OK;
}

static const void* dz_of(const BwdRun& r, int l) {
  const AeLayer& a = r.h->L[l];
  const LayerWS& s = r.w.l[l];
  return (l == r.nL - 1) ? (r.from_mse ? s.out : s.dy) : (a.bn ? s.dz : s.dy);
}

// Layer l's dW problem.  Only once the bwd-data of layer l+1 has been emitted:
// bias_src(l) reads the bwd_fused flag that step sets.
static PendingDW make_dw(const BwdRun& r, int l) {
  const mmad_ae* h = r.h;
  const AeWS& w = r.w;
  const AeLayer& a = h->L[l];
  const float *isc, *ish;
  const void* in = input_of(h, w, l, true, &isc, &ish);
  GemmEpi e{};
  e.M = a.Np;
  e.N = a.Kp;
  e.out = h->grads + a.w_off;
  e.ldo = a.Kp;
  if (isc) {
    // dW against the raw producer activation, fixed up in the epilogue
    e.b_scale = isc;
    e.b_shift = ish;
  }
  if (r.fused()) {
    // this layer's Adam update in the epilogue: the weight tile's terms ...
    e.ad_p = h->params + a.w_off;
    e.ad_m = h->m + a.w_off;
    e.ad_v = h->v + a.w_off;
    e.ad_shadow = adam_shadow(h, a, w.ping);
    // the gradient is consumed by the fused Adam in registers; materialise
    // it only when asked (h->keep_grads)
    e.dw_nostore = h->keep_grads ? 0 : 1;
    e.ad_w1 = r.adam->w1;
    e.ad_w2 = r.adam->w2;
    e.ad_eps = r.adam->eps;
    e.ad_step = r.adam->step_size;
    e.ad_bc2 = r.adam->bc2_sqrt;
    e.dyn = w.dyn;
    // ... and the small segment [bias | gamma | beta]'s
    e.sm_p = h->params + a.b_off;
    e.sm_g = h->grads + a.b_off;
    e.sm_m = h->m + a.b_off;
    e.sm_v = h->v + a.b_off;
    e.sm_n = a.bn ? 3 * a.Np : a.Np;
    e.sm_bN = a.N;
    e.sm_bNp = a.Np;
  }
  if (isc || r.fused()) {
    const BiasSrc bs = bias_src(h, w, l, r.from_mse);
    e.gb_src = bs.src;
    e.gb_parts = bs.nparts;
    e.gb_stride = bs.stride;
  }
  return PendingDW{dz_of(r, l), in, a.Np, a.Kp, a.Np, a.Kp, prows_of(w, a), e, l};
}

static int launch_dw(const BwdRun& r, const PendingDW& q, hipStream_t s) {
  return ae_gemm(r.h, r.w, r.h->dtype, GEMM_EPI_BWD_WEIGHT, q.dz, q.lda, q.in, q.ldb, q.M, q.N, q.K,
                 q.ep, s, nullptr, PROBE_DW + q.layer);
}

// issue the deferred dW GEMMs in order on `s`: members of one group (adjacent
// in issue order) as one launch, every other -- and a group the dispatcher
// refuses -- as its own
static int flush(BwdRun& r, hipStream_t s) {
  std::vector<PendingDW>& p = r.pending;
  for (size_t i = 0; i < p.size();) {
    const int gid = r.grp[p[i].layer];
    size_t j = i + 1;
    while (gid >= 0 && j < p.size() && r.grp[p[j].layer] == gid) ++j;
    int rc = MMAD_GEMM_GROUP_REFUSED;
    if (j - i >= 2) rc = ae_gemm_group(r.h, r.w, r.h->dtype, &p[i], (int)(j - i), s);
    if (rc == MMAD_GEMM_GROUP_REFUSED) {
      for (size_t m = i; m < j; ++m) RET_IF(launch_dw(r, p[m], s));
    } else if (rc != MMAD_OK) {
      return rc;
    }
    i = j;
  }
  p.clear();
  return MMAD_OK;
}

// which of its two events a chain step got completed on the main stream
struct ChainPlaced { bool done, fork; };

// The main-stream chain element: bwd-data GEMM of layer l (dz_l -> dy_{l-1})
// plus what turns dy_{l-1} into dz_{l-1} outside a GEMM epilogue (the VIB
// reparameterisation backward, the BN + activation backward apply).  The only
// writer of bwd_fused.  done_ev (nullable) is to complete with the GEMM,
// fork_below (nullable) with the launch that produces dz_{l-1}; a launch
// completes one event, and done_ev goes first.  done_ev that cannot ride the
// GEMM is recorded behind it when a BN apply follows, and is otherwise left
// to the caller; fork_below is only ever attached.
static int bwd_data_step(BwdRun& r, int l, hipEvent_t done_ev, hipEvent_t fork_below, ChainPlaced* placed) {
  *placed = ChainPlaced{false, false};
  if (l == 0) return MMAD_OK;
  mmad_ae* h = r.h;
  AeWS& w = r.w;
  const int dt = h->dtype;
  const AeLayer& a = h->L[l];
  const AeLayer& p = h->L[l - 1];
  LayerWS& ps = w.l[l - 1];
  const int Mp = prows_of(w, a), Mpp = prows_of(w, p);
  GemmEpi ep{};
  ep.M = rows_of(w, a);
  ep.N = a.K;
  ep.ldo = a.Kp;
  ep.ldpart = a.Kp;
  const bool hop = h->vib && l == h->n_enc;
  if (hop) {
    ep.out = w.dzin;
  } else if (!p.bn) {
    ep.out = ps.dy;
    ep.part = ps.stats;
  } else {
    ep.out = ps.dy;
    ep.bn_a = ps.out;
    ep.bn_mean = ps.mean;
    ep.bn_rstd = ps.rstd;
    ep.bn_part = ps.bnpart;
    ps.bwd_fused = w.bn_mode_bwd == 2 && mmad_gemm_bn_fusable(dt, GEMM_EPI_BWD_DATA, Mp, a.Kp);
    if (ps.bwd_fused) {
      // BN + activation backward of layer l-1 inside this GEMM: dz directly
      ep.out = nullptr;
      ep.bn_sync = ps.sync_b;
      ep.bn_err = w.bn_err;
      ep.bn_gamma = h->params + p.g_off;
      ep.bn_dz = ps.dz;
      ep.bn_dgamma = h->grads + p.g_off;
      ep.bn_dbeta = h->grads + p.be_off;
      ep.bn_dbpart = ps.dbpart;
      ep.bn_act = p.act;
      ep.slope = h->slope;
    }
  }
  // dz_{l-1} comes from the BN apply launch; across the VIB hop, from the
  // reparameterisation backward, and neither event rides a launch
  const bool apply = !hop && p.bn && !ps.bwd_fused;
  if (!hop && done_ev && h->ev_on_kernel && !h->capturing) {
    ep.done_ev = done_ev;
    placed->done = true;
  } else if (!hop && fork_below && !apply) {
    ep.done_ev = fork_below;
    placed->fork = true;
  }
  RET_IF(ae_gemm(h, w, dt, GEMM_EPI_BWD_DATA, dz_of(r, l), a.Np, weights(h, a), a.Kp, Mp, a.Kp, a.Np, ep,
                 r.st));
  if (hop)
    return mmad_vib_reparam_bwd(dt, w.B, h->btl, w.k, ps.out, p.Np, w.eps, w.dzin, a.Kp, r.beta_kl,
                                ps.dy, p.Np, ps.dbpart, r.st);
  if (p.bn && done_ev && !placed->done) {
    MMAD_HIP_CHECK(hipEventRecord(done_ev, r.st));
    placed->done = true;
  }
  if (apply) {
    RET_IF(mmad_bn_act_bwd_apply_ev(dt, p.act, h->slope, rows_of(w, p), p.N, Mpp, p.Np, ps.dy, ps.out,
                                    ps.mean, ps.rstd, h->params + p.g_off, ps.bnpart, Mpp / 64, ps.dz,
                                    h->grads + p.g_off, h->grads + p.be_off, ps.dbpart, r.st, fork_below));
    placed->fork = fork_below != nullptr;
  }
  return MMAD_OK;
}

// ---- plain policy (no Adam): dW_l forks at dz_l and overlaps the chain below
static int plain_before(BwdRun& r, int l) {
  mmad_ae* h = r.h;
  RET_IF(hand_off(h->ev_fork[l], r.st, r.side));
  RET_IF(launch_dw(r, make_dw(r, l), r.side));
  if (h->dw_events) MMAD_HIP_CHECK(hipEventRecord(h->ev_xdw[l], r.side));
  return MMAD_OK;
}
static int plain_after(BwdRun& r, int l) {
  // torch exchange: W_l is read for the last time by the bwd-data of l
  if (r.h->dw_events && l > 0) MMAD_HIP_CHECK(hipEventRecord(r.h->ev_xdata[l], r.st));
  return MMAD_OK;
}

// ---- data-parallel policy: dW GEMMs per exchange bucket, Adam after the exchange
static int dp_before(BwdRun& r, int l) {
  mmad_ae* h = r.h;
  const DpBucket* cur = r.open_bucket();
  const DpBucket* bk = r.closes_bucket(l);
  // a bucket made only of the last dw_main layers of the chain runs its dW
  // GEMMs on the main stream, idle by then, instead of behind the side
  // stream's backlog (the exchange tail waits for them)
  const bool on_main = cur && cur->l_hi < r.w.dw_main;
  // below dp_fork_rows rows (host-bound steps, every event call counts) the dW
  // GEMMs of a bucket's layers are issued together once the layer that closes
  // it has its dz (one fork per bucket), then the bucket's event
  // from dp_fork_rows rows the step is GPU-bound: a side-stream bucket's dW
  // GEMMs then start at their own dz (one fork each) instead of queueing
  // until the bucket's lowest layer
  const bool each = h->dp_fork_rows > 0 && prows_of(r.w, h->L[l]) >= h->dp_fork_rows && cur && !on_main;
  // (a bucket whose upper layers were below the row threshold: their dW GEMMs
  // go first, so the bucket's event below covers them too)
  r.pending.push_back(make_dw(r, l));
  if (!each && !bk) return MMAD_OK;
  hipStream_t ds = on_main ? r.st : r.side;
  if (!on_main) RET_IF(hand_off(h->ev_fork[l], r.st, r.side));
  RET_IF(flush(r, ds));
  if (bk) MMAD_HIP_CHECK(hipEventRecord(h->ev_dw[l], ds));
  return MMAD_OK;
}

// the small bucket [all bias | gamma | beta grads] + the loss: the last
// bwd-data (just enqueued) has produced every bias partial and the loss
// partials are the forward's: reduce them on the main stream now and queue
// the bucket's exchange + Adam on the comm stream ahead of the remaining
// weight buckets, so it runs while their dW GEMMs still compute instead of
// after them
static int dp_small_bucket(BwdRun& r) {
  mmad_ae* h = r.h;
  const AdamHyper* ad = r.adam;
  RET_IF(finish_reductions(h, r.w, true, true, r.beta_kl, r.dp_loss, r.st));
  RET_IF(hand_off(h->ev_small, r.st, h->cstream));
  const int64_t ns = h->n_params - h->n_weight;
  RET_IF(mmad_allreduce_pair(h->comm, h->grads + h->n_weight, ns, r.dp_loss, 1, h->cstream));
  return mmad_adam_w(ns, h->params + h->n_weight, h->grads + h->n_weight, h->m + h->n_weight,
                     h->v + h->n_weight, ad->w1, ad->w2, ad->eps, ad->step_size, ad->bc2_sqrt, nullptr, 0,
                     h->cstream);
}

// exchange the bucket layer l closes (layers bk.l_hi .. l, one contiguous
// weight range) on the comm stream as soon as its last dW GEMM is complete,
// then its Adam update (which rewrites the bucket's weights, so it also waits
// for the main stream's bwd-data of layer l, the last GEMM of the chain that
// reads them)
static int exchange_bucket(BwdRun& r, const DpBucket& bk, int l) {
  mmad_ae* h = r.h;
  const AdamHyper* ad = r.adam;
  hipStream_t cs = h->cstream;
  const bool bf16 = h->dtype == MMAD_BF16;
  MMAD_HIP_CHECK(hipStreamWaitEvent(cs, h->ev_data[l], 0));
  const int nr = mmad_comm_size(h->comm) > 0 ? mmad_comm_size(h->comm) : 1;
  MMAD_HIP_CHECK(hipStreamWaitEvent(cs, h->ev_dw[l], 0));
  const int64_t n = bk.n, boff = bk.off;
  if (h->dp_shard && n % nr == 0 && (n / nr) % 4 == 0) {
    // ZeRO-1 form: reduce-scatter, Adam on this rank's shard, all-gather
    // of the updated weights the next step reads (bf16 shadow / fp32 p)
    const int64_t cnt = n / nr, off = boff + (int64_t)mmad_comm_rank(h->comm) * cnt;
    if (h->grad_bf16) {
      // bf16 on the wire: round the bucket, reduce-scatter, widen this rank's slice
      char* gb = (char*)h->grad_bf16;
      RET_IF(mmad_to_bf16(n, h->grads + boff, gb + boff * 2, cs));
      RET_IF(mmad_reduce_scatter_bucket_bf16(h->comm, gb + boff * 2, n, cs));
      RET_IF(mmad_from_bf16(cnt, gb + off * 2, h->grads + off, cs));
    } else {
      RET_IF(mmad_reduce_scatter_bucket(h->comm, h->grads + boff, n, cs));
    }
    void* sh = bf16 ? (void*)((char*)h->shadow + off * 2) : nullptr;
    RET_IF(mmad_adam_w(cnt, h->params + off, h->grads + off, h->m + off, h->v + off, ad->w1, ad->w2,
                       ad->eps, ad->step_size, ad->bc2_sqrt, sh, bf16 ? cnt : 0, cs));
    if (bf16)
      RET_IF(mmad_all_gather_bucket(h->comm, (char*)h->shadow + boff * 2, n, MMAD_BF16, cs));
    else
      RET_IF(mmad_all_gather_bucket(h->comm, h->params + boff, n, MMAD_F32, cs));
    if (nr > 1) h->master_stale = true;
  } else {
    RET_IF(mmad_allreduce_bucket(h->comm, h->grads + boff, n, cs));
    void* sh = adam_shadow(h, h->L[l], r.w.ping);
    RET_IF(mmad_adam_w(n, h->params + boff, h->grads + boff, h->m + boff, h->v + boff, ad->w1, ad->w2,
                       ad->eps, ad->step_size, ad->bc2_sqrt, sh, bf16 ? n : 0, cs));
  }
  ++r.next_bucket;
  return MMAD_OK;
}

// ---- fused single-GPU policy: dW_l with this layer's Adam update fused into
// its epilogue.  It rewrites W_l, so without ping-pong shadows it starts only
// once the main stream has finished reading W_l (bwd-data of l); the rest of
// the chain keeps overlapping it.
static void fused_plan_groups(BwdRun& r) {
  mmad_ae* h = r.h;
  if (!r.w.ping || h->capturing || h->side_hold || h->dw_group_blocks == 0) return;
  std::vector<int> np(r.nL), kp(r.nL), rows(r.nL);
  for (int l = 0; l < r.nL; ++l) {
    np[l] = h->L[l].Np;
    kp[l] = h->L[l].Kp;
    rows[l] = prows_of(r.w, h->L[l]);
  }
  const int budget = h->dw_group_blocks < 0 ? mmad_gemm_group_capacity(h->dtype) : h->dw_group_blocks;
  mmad_dw_group_plan(r.nL, np.data(), kp.data(), rows.data(), r.w.dw_main, r.nL - h->dw_late, budget,
                     h->dw_group_members, r.grp.data());
}
static int fused_before(BwdRun& r, int l) {
  // dz_l is complete: the fork of a ping-pong dW that the producing launch
  // did not carry
  if (r.forks_at_dz(l) && !r.fork_none(l) && !r.fork_done[l])
    MMAD_HIP_CHECK(hipEventRecord(r.h->ev_fork[l], r.st));
  return MMAD_OK;
}
static int fused_after(BwdRun& r, int l) {
  mmad_ae* h = r.h;
  PendingDW q = make_dw(r, l);
  if (l < r.w.dw_main) {
    // the last dW GEMMs of the chain go to the main stream, which is idle
    // by then, instead of queueing behind the side stream's backlog
    q.ep.tile_force = mmad_tile_adam_main_for(q.M, q.N, q.K) + 1;
    return launch_dw(r, q, r.st);
  }
  // deferred dW GEMMs go out ahead of this one
  r.pending.push_back(q);
  if (h->side_hold) return MMAD_OK;   // all of them behind the chain (run_backward)
  if (r.ping(l)) {
    // no fork of its own: issued with the next lower layer's dW
    if (!r.late(l) && !r.fork_ev(l)) return MMAD_OK;
    if (r.late(l))
      RET_IF(hand_off(h->ev_fork[l], r.st, r.side));
    else if (!r.fork_none(l))
      MMAD_HIP_CHECK(hipStreamWaitEvent(r.side, h->ev_fork[l], 0));
  } else {
    if (!r.needs_data_ev(l)) return MMAD_OK;
    MMAD_HIP_CHECK(hipStreamWaitEvent(r.side, h->ev_data[l], 0));
  }
  return flush(r, r.side);
}

// backward through every layer: the chain on `st`, the dW GEMMs where the
// policy puts them, the side stream joined back into `st` at the end
static int run_backward(mmad_ae* h, AeWS& w, bool from_mse, float beta_kl, const AdamHyper* adam,
                        hipStream_t st, float* dp_loss = nullptr, bool side_after_mse = false) {
  const int nL = (int)h->L.size();
  BwdRun r{h, w, st, h->side, adam, from_mse, side_after_mse, beta_kl, dp_loss, nL,
           h->fork_on_kernel && !h->capturing};
  r.fork_done.assign(nL, 0);
  r.grp.assign(nL, -1);
  if (r.dp()) dp_plan(h, r.plan);
  if (r.fused()) fused_plan_groups(r);
  const int small_at = nL > h->dp_small_at ? h->dp_small_at : 0;
  for (int l = nL - 1; l >= 0; --l) {
    // DP and plain issue dW_l before the bwd-data of l, fused after it
    RET_IF(!adam ? plain_before(r, l) : r.dp() ? dp_before(r, l) : fused_before(r, l));
    const bool need = r.needs_data_ev(l);
    // dz_{l-1} is produced by this step: its side-stream dW fork rides on that launch
    const bool fork_below = l > 0 && r.fork_kev && r.forks_at_dz(l - 1);
    ChainPlaced placed;
    RET_IF(bwd_data_step(r, l, need ? h->ev_data[l] : nullptr, fork_below ? h->ev_fork[l - 1] : nullptr,
                         &placed));
    if (placed.fork) r.fork_done[l - 1] = 1;
    if (!adam) RET_IF(plain_after(r, l));
    if (r.dp() && dp_loss && l == small_at) RET_IF(dp_small_bucket(r));
    // ev_data[l] that the chain step could neither attach nor place ahead of a BN apply
    if (need && !placed.done) MMAD_HIP_CHECK(hipEventRecord(h->ev_data[l], st));
    if (r.fused()) RET_IF(fused_after(r, l));
    if (const DpBucket* bk = r.closes_bucket(l)) RET_IF(exchange_bucket(r, *bk, l));
  }
  if (h->side_hold && !r.pending.empty()) {
    RET_IF(hand_off(h->ev_hold, st, r.side));
    RET_IF(flush(r, r.side));
  }
  MMAD_CHECK_ARG(r.pending.empty(), "ae backward: deferred dW GEMMs left unissued");
  // join the side stream back into the main stream
  return hand_off(h->ev_join, r.side, st);
}

// bias grads of every layer (when Adam did not finalise them) + the loss
static int finish_reductions(mmad_ae* h, AeWS& w, bool biases, bool from_mse, float beta_kl,
                             float* loss_out, hipStream_t st) {
  MmadReduceJobs jobs{};
  int n = 0, max_np = 1;
  const int nL = (int)h->L.size();
  if (biases) {
    for (int l = 0; l < nL; ++l) {
      const AeLayer& a = h->L[l];
      const BiasSrc bs = bias_src(h, w, l, from_mse);
      MmadReduceJob& j = jobs.j[n++];
      j.src = bs.src;
      j.dst = h->grads + a.b_off;
      j.nparts = bs.nparts;
      j.stride = bs.stride;
      j.N = a.N;
      j.Np = a.Np;
      j.scale = 1.f;
      max_np = a.Np > max_np ? a.Np : max_np;
    }
  }
  if (loss_out) {
    const AeLayer& last = h->L[nL - 1];
    MmadReduceJob& j = jobs.j[n++];
    j.scalar = 1;
    j.src = w.lossp;                        // one sum of d^2 per MSE-GEMM output tile
    j.dst = loss_out;
    j.nparts = 1;
    j.stride = 0;
    j.N = h->mse_tiles;
    j.Np = j.N;
    j.scale = 1.f / (float)w.k;
    if (h->vib) {
      j.src2 = w.klpart;
      j.n2 = (int)w.kl_parts;
      j.scale2 = beta_kl;
    }
  }
  if (n == 0) return MMAD_OK;
  jobs.dyn = loss_out ? w.dyn : nullptr;
  return mmad_reduce_jobs(jobs, n, max_np, st);
}

int mmad_ae_train_fwd_bwd(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                          uint64_t seed, uint64_t offset, float beta_kl, float* loss_out,
                          void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->running, "ae_train: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && loss_out, "ae_train: bad input");
  AeWS w;
  RET_IF(prepare_ws(h, B, k, ws, ws_bytes, w, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  RET_IF(run_forward(h, w, x, ld_x, 0, eps, seed, offset, st));
  RET_IF(run_backward(h, w, true, beta_kl, nullptr, st));
  return finish_reductions(h, w, true, true, beta_kl, loss_out, st);
}

static AdamHyper adam_hyper(float lr, float b1, float b2, float eps, int step) {
  return mmad_adam_consts(lr, b1, b2, eps, step);
}

int mmad_ae_train_step(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                       uint64_t seed, uint64_t offset, float beta_kl, float lr, float beta1,
                       float beta2, float adam_eps, int step, float* loss_out, void* ws,
                       int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->running && h->m && h->v,
                 "ae_train_step: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && loss_out, "ae_train_step: bad input");
  MMAD_CHECK_ARG(step >= 1, "ae_train_step: step must be >= 1");
  h->planes_stale = true;
  AeWS w;
  RET_IF(prepare_ws(h, B, k, ws, ws_bytes, w, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  const AdamHyper ah = adam_hyper(lr, beta1, beta2, adam_eps, step);
  // ping-pong schedule (bf16 with a shadow pair, large calls, single process)
  w.ping = h->shadow_alt && !h->comm && !h->capturing && w.Mpe >= h->pair_rows;
  if (w.ping) w.dw_main = h->dw_main_ping;
  // the side stream's loss reduction waits on the MSE launch's own completion
  const bool loss_ev_on_kernel = !h->comm && h->loss_side && h->ev_on_kernel && !h->capturing;
  RET_IF(run_forward(h, w, x, ld_x, 0, eps, seed, offset, st, loss_ev_on_kernel ? h->ev_loss : nullptr));
  if (!h->comm && !h->loss_side) {
    RET_IF(run_backward(h, w, true, beta_kl, &ah, st));
    RET_IF(finish_reductions(h, w, false, true, beta_kl, loss_out, st));
    if (w.ping) std::swap(h->shadow, h->shadow_alt);
    return MMAD_OK;
  }
  if (!h->comm) {
    // the loss needs only the forward's MSE (and KL) partials: reduce it on
    // the side stream now, off the main stream's tail (the backward joins the
    // side stream back into the caller's before the step ends)
    if (!loss_ev_on_kernel) MMAD_HIP_CHECK(hipEventRecord(h->ev_loss, st));
    MMAD_HIP_CHECK(hipStreamWaitEvent(h->side, h->ev_loss, 0));
    RET_IF(finish_reductions(h, w, false, true, beta_kl, loss_out, h->side));
    RET_IF(run_backward(h, w, true, beta_kl, &ah, st, nullptr, true));
    if (w.ping) std::swap(h->shadow, h->shadow_alt);
    return MMAD_OK;
  }
  // data parallel: per-layer weight buckets and (ahead of layer 0's) the
  // small bucket [all bias | gamma | beta grads] + the loss, each with its
  // Adam, on the comm stream (run_backward); then join
  RET_IF(run_backward(h, w, true, beta_kl, &ah, st, loss_out));
  MMAD_HIP_CHECK(hipEventRecord(h->ev_cdone, h->cstream));
  MMAD_HIP_CHECK(hipStreamWaitEvent(st, h->ev_cdone, 0));
  return MMAD_OK;
}

int mmad_ae_train_step_graph(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                             uint64_t seed, uint64_t offset, float beta_kl, float lr, float beta1,
                             float beta2, float adam_eps, int step, float* loss_out, void* ws,
                             int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->running && h->m && h->v,
                 "ae_train_step_graph: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && loss_out, "ae_train_step_graph: bad input");
  MMAD_CHECK_ARG(step >= 1, "ae_train_step_graph: step must be >= 1");
  h->planes_stale = true;
  if (h->comm || h->graph_broken)   // eager schedule for these
    return mmad_ae_train_step(h, x, ld_x, B, k, eps, seed, offset, beta_kl, lr, beta1, beta2,
                              adam_eps, step, loss_out, ws, ws_bytes, stream);
  AeWS w;
  hipStream_t st = (hipStream_t)stream;
  RET_IF(prepare_ws(h, B, k, ws, ws_bytes, w, st));
  const AdamHyper ah = adam_hyper(lr, beta1, beta2, adam_eps, step);
  // this call's values -> pinned slot -> the workspace's device slot
  if (!h->dyn_host) {
    MMAD_HIP_CHECK(hipHostMalloc((void**)&h->dyn_host, sizeof(MmadDyn) * mmad_ae::kDynSlots,
                                 hipHostMallocDefault));
    for (auto& e : h->dyn_ev) MMAD_HIP_CHECK(hipEventCreateWithFlags(&e, h->ev_flags_));
  }
  const int slot = h->dyn_next;
  h->dyn_next = (slot + 1) % mmad_ae::kDynSlots;
  if (h->dyn_used[slot]) MMAD_HIP_CHECK(hipEventSynchronize(h->dyn_ev[slot]));
  MmadDyn& d = h->dyn_host[slot];
  d.x = x;
  d.loss = loss_out;
  d.eps = eps;
  d.seed = seed;
  d.offset = offset;
  d.ad_step = ah.step_size;
  d.ad_bc2 = ah.bc2_sqrt;
  MMAD_HIP_CHECK(hipMemcpyAsync(w.dyn_dev, &d, sizeof(MmadDyn), hipMemcpyHostToDevice, st));
  MMAD_HIP_CHECK(hipEventRecord(h->dyn_ev[slot], st));
  h->dyn_used[slot] = true;
  const int xvec = ((uintptr_t)x % 16 == 0 && ld_x % 4 == 0) ? 1 : 0;
  for (auto& g : h->tgraphs) {
    if (g.B == B && g.k == k && g.ld_x == ld_x && g.xvec == xvec && g.has_eps == (eps != nullptr) &&
        g.ws == ws && g.shadow == h->shadow && g.dw_main == h->dw_main && g.ev_every == h->ev_every &&
        g.keep_grads == h->keep_grads && g.beta_kl == beta_kl && g.b1 == beta1 && g.b2 == beta2 &&
        g.aeps == adam_eps) {
      MMAD_HIP_CHECK(hipGraphLaunch(g.exec, st));
      return MMAD_OK;
    }
  }
  // first call of this signature: run it eagerly (reading the same device
  // slot; this also settles every GEMM tile choice, which cannot be timed
  // under capture), then capture the identical launch sequence
  w.dyn = w.dyn_dev;
  RET_IF(run_forward(h, w, x, ld_x, 0, eps, seed, offset, st));
  RET_IF(run_backward(h, w, true, beta_kl, &ah, st));
  RET_IF(finish_reductions(h, w, false, true, beta_kl, loss_out, st));
  if (!h->gstream) MMAD_HIP_CHECK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    h->graph_broken = true;
    (void)hipGetLastError();
    return MMAD_OK;
  }
  h->capturing = true;
  int rc = run_forward(h, w, x, ld_x, 0, eps, seed, offset, h->gstream);
  if (rc == MMAD_OK) rc = run_backward(h, w, true, beta_kl, &ah, h->gstream);
  if (rc == MMAD_OK) rc = finish_reductions(h, w, false, true, beta_kl, loss_out, h->gstream);
  h->capturing = false;
  const hipError_t ec = hipStreamEndCapture(h->gstream, &graph);
  hipGraphExec_t exec = nullptr;
  hipError_t ei = hipErrorUnknown;
  if (rc == MMAD_OK && ec == hipSuccess && graph)
    ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (rc != MMAD_OK || ec != hipSuccess || ei != hipSuccess) {
    // this step already ran eagerly; later calls stay eager
    h->graph_broken = true;
    (void)hipGetLastError();
    return MMAD_OK;
  }
  if (h->tgraphs.size() >= 16) {
    (void)hipGraphExecDestroy(h->tgraphs.front().exec);
    h->tgraphs.erase(h->tgraphs.begin());
  }
  h->tgraphs.push_back({B, k, ld_x, xvec, eps != nullptr, h->dw_main, h->ev_every, h->keep_grads, ws,
                        h->shadow, beta_kl, beta1, beta2, adam_eps, exec});
  return MMAD_OK;
}

int mmad_ae_train_graph_count(const mmad_ae* h) { return h ? (int)h->tgraphs.size() : -1; }

int mmad_ae_set_comm(mmad_ae* h, mmad_comm* c) {
  MMAD_CHECK_ARG(h, "ae_set_comm: null handle");
  MMAD_CHECK_ARG(h->side, "ae_set_comm: bind the handle first");
  MMAD_CHECK_ARG(c == h->comm || !h->master_stale,
                 "ae_set_comm: the master weights are sharded over the ranks of the attached "
                 "communicator: mmad_ae_dp_sync_master on every rank first");
  if (c && !h->cstream) {
    // highest priority: the exchange must not queue behind the dW GEMMs
    int least = 0, greatest = 0;
    MMAD_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    MMAD_HIP_CHECK(hipStreamCreateWithPriority(&h->cstream, hipStreamNonBlocking, greatest));
    // the events RCCL's reads of a bucket wait on keep the system-scope
    // fence (a transport may move the bytes with a copy engine, which does
    // not see the L2); one per bucket and step
    h->ev_dw.resize(h->L.size());
    for (auto& e : h->ev_dw) MMAD_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_small, hipEventDisableTiming));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_cdone, h->ev_flags_));
  }
  h->comm = c;
  return MMAD_OK;
}

int mmad_ae_dp_master_stale(const mmad_ae* h) { return h && h->master_stale ? 1 : 0; }

int mmad_ae_set_grad_bf16(mmad_ae* h, void* buf) {
  MMAD_CHECK_ARG(h && h->params, "ae_set_grad_bf16: unbound handle");
  MMAD_CHECK_ARG(!buf || ((uintptr_t)buf % 16 == 0), "ae_set_grad_bf16: buffer must be 16-byte aligned");
  h->grad_bf16 = buf;
  return MMAD_OK;
}

int mmad_ae_dw_events(mmad_ae* h, int on) {
  MMAD_CHECK_ARG(h && h->side, "ae_dw_events: bind the handle first");
  if (on && h->ev_xdw.empty()) {
    h->ev_xdw.resize(h->L.size());
    h->ev_xdata.resize(h->L.size());
    for (auto& e : h->ev_xdw) MMAD_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : h->ev_xdata) MMAD_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  h->dw_events = on != 0;
  return MMAD_OK;
}

int mmad_ae_wait_dw(mmad_ae* h, int layer, void* stream) {
  MMAD_CHECK_ARG(h && h->dw_events, "ae_wait_dw: dW events are off (mmad_ae_dw_events)");
  MMAD_CHECK_ARG(layer >= 0 && layer < (int)h->L.size(), "ae_wait_dw: bad layer %d", layer);
  MMAD_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->ev_xdw[layer], 0));
  if (layer > 0) MMAD_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->ev_xdata[layer], 0));
  return MMAD_OK;
}

int mmad_ae_dw_plan(const mmad_ae* h, int max_n, int64_t* off, int64_t* n, int* layer_lo) {
  MMAD_CHECK_ARG(h && h->params, "ae_dw_plan: unbound handle");
  std::vector<DpBucket> plan;
  dp_plan(h, plan);
  MMAD_CHECK_ARG(max_n >= (int)plan.size() && off && n && layer_lo,
                 "ae_dw_plan: room for %d buckets needed", (int)plan.size());
  for (size_t i = 0; i < plan.size(); ++i) {
    off[i] = plan[i].off;
    n[i] = plan[i].n;
    layer_lo[i] = plan[i].l_lo;
  }
  return (int)plan.size();
}

int mmad_ae_dp_sync_master(mmad_ae* h, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->m && h->v, "ae_dp_sync_master: unbound handle");
  h->planes_stale = true;
  if (!h->comm || !h->master_stale) return MMAD_OK;
  hipStream_t st = (hipStream_t)stream;
  const int nr = mmad_comm_size(h->comm);
  std::vector<DpBucket> plan;
  dp_plan(h, plan);
  for (const DpBucket& b : plan) {
    const int64_t n = b.n, boff = b.off;
    if (!(n % nr == 0 && (n / nr) % 4 == 0)) continue;   // an all-reduced bucket: already current
    if (h->dtype == MMAD_BF16) RET_IF(mmad_all_gather_bucket(h->comm, h->params + boff, n, MMAD_F32, st));
    RET_IF(mmad_all_gather_bucket(h->comm, h->m + boff, n, MMAD_F32, st));
    RET_IF(mmad_all_gather_bucket(h->comm, h->v + boff, n, MMAD_F32, st));
  }
  h->master_stale = false;
  return MMAD_OK;
}

int mmad_ae_backward(mmad_ae* h, const float* dxhat, int ld, int B, void* ws, int64_t ws_bytes,
                     void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads, "ae_backward: unbound handle");
  MMAD_CHECK_ARG(!h->vib, "ae_backward: the VIB model trains through mmad_ae_train_fwd_bwd");
  AeWS w;
  RET_IF(prepare_ws(h, B, 1, ws, ws_bytes, w, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  const int nL = (int)h->L.size();
  const AeLayer& last = h->L[nL - 1];
  LayerWS& s = w.l[nL - 1];
  MMAD_CHECK_ARG(dxhat && ld >= last.N, "ae_backward: bad dxhat");
  RET_IF(mmad_pack_input(h->dtype, B, last.N, w.Mpd, last.Np, dxhat, ld, s.dy, st));
  RET_IF(mmad_matrix_colsum_partials(h->dtype, B, w.Mpd, last.Np, s.dy, s.dbpart, st));
  RET_IF(run_backward(h, w, false, 0.f, nullptr, st));
  return finish_reductions(h, w, true, false, 0.f, nullptr, st);
}

int mmad_ae_adam(mmad_ae* h, float lr, float beta1, float beta2, float eps, int step,
                 void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->m && h->v, "ae_adam: unbound handle");
  MMAD_CHECK_ARG(step >= 1, "ae_adam: step must be >= 1");
  h->planes_stale = true;
  const AdamHyper ah = adam_hyper(lr, beta1, beta2, eps, step);
  return mmad_adam_w(h->n_params, h->params, h->grads, h->m, h->v, ah.w1, ah.w2, eps, ah.step_size,
                   ah.bc2_sqrt, h->dtype == MMAD_BF16 ? h->shadow : nullptr,
                   h->dtype == MMAD_BF16 ? h->n_weight : 0, stream);
}

int mmad_ae_adam_range(mmad_ae* h, float lr, float beta1, float beta2, float eps, int step,
                       int64_t off, int64_t n, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->m && h->v, "ae_adam_range: unbound handle");
  MMAD_CHECK_ARG(step >= 1, "ae_adam_range: step must be >= 1");
  h->planes_stale = true;
  MMAD_CHECK_ARG(off >= 0 && n >= 0 && off + n <= h->n_params && off % 4 == 0,
                 "ae_adam_range: bad range [%lld, +%lld)", (long long)off, (long long)n);
  const AdamHyper ah = adam_hyper(lr, beta1, beta2, eps, step);
  // the bf16 shadow covers the weights [0, n_weight)
  void* sh = nullptr;
  int64_t nsh = 0;
  if (h->dtype == MMAD_BF16 && off < h->n_weight) {
    sh = (char*)h->shadow + off * 2;
    nsh = h->n_weight - off < n ? h->n_weight - off : n;
  }
  return mmad_adam_w(n, h->params + off, h->grads + off, h->m + off, h->v + off, ah.w1, ah.w2, eps,
                   ah.step_size, ah.bc2_sqrt, sh, nsh, stream);
}

int mmad_ae_forward(mmad_ae* h, const float* x, int ld_x, int B, int train_bn, float* x_hat,
                    int ld_out, float* loss_out, void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->running, "ae_forward: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K, "ae_forward: bad input");
  AeWS w;
  RET_IF(prepare_ws(h, B, 1, ws, ws_bytes, w, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  const bool x3 = !train_bn && h->planes;
  if (x3) RET_IF(refresh_planes(h, st));
  RET_IF(run_forward(h, w, x, ld_x, train_bn ? 2 : 1, nullptr, 0x5eed, 0, st));
  const AeLayer& last = h->L.back();
  // (x3: the last GEMM's fp32 copy of x_hat, run_forward)
  const void* xh = x3 ? w.l.back().dy : w.l.back().out;
  if (x_hat) RET_IF(mmad_unpack_output(h->dtype, B, last.N, last.Np, xh, x_hat, ld_out, st));
  if (loss_out) {
    RET_IF(mmad_sse_partials(h->dtype, B, last.N, last.Np, xh, x, ld_x, w.misc, 256, st));
    RET_IF(mmad_sum(256, w.misc, 1.f, loss_out, 0, st));
  }
  return MMAD_OK;
}

// one batch of the scoring pass on a prepared workspace; layer_sq row l at
// layer_sq + l*ld_sq
// nap (nullable; needs a fit and no caller diffs): the in-range score GEMMs
// write their diffs straight into the packed NAP operand, then the NAP GEMM
// and its column sum write nap[0..B)
// fit (nullable, without nap; the streaming NAP fit): the diffs of its layers
// go, as fp32, into its own packed operand and nothing else changes
struct DiffSink {
  int start, end, K, Kp;   // diff layers [start, end), their width and its padding
  bool x3;                 // bf16 plane operand (the attached fit's x3 NAP GEMM)
  void* x;                 // [Mpe][Kp]
};
static int score_batch(mmad_ae* h, const float* x, int ld_x, int B, float* layer_sq,
                       int64_t ld_sq, float* diffs, AeWS& w, hipStream_t st, float* nap = nullptr,
                       const DiffSink* fit = nullptr) {
  // x3 (score planes attached): activations travel as bf16 planes, every
  // reference of a diff stays fp32 -- pass 1 leaves an fp32 copy of each
  // encoder output (ref32), the decoder's last layer scores against the
  // caller's x itself, and the SCORE epilogue subtracts before it rounds
  const int dt = score_dt(h);
  const bool x3 = dt == MMAD_BF16X3;
  const int nL = (int)h->L.size();
  RET_IF(mmad_pack_input(dt, B, h->L[0].K, w.Mpe, h->L[0].Kp, x, ld_x, w.xin, st));
  int ld_diff = h->L[0].K;
  for (int e = 0; e < h->n_enc; ++e) ld_diff += h->L[e].N;
  const mmad_ae::NapFit& nf = h->nap;
  const bool nap_x3 = nap && nf.dtype == MMAD_BF16X3;
  const bool routed = nap || fit;
  const DiffSink sk = nap ? DiffSink{nf.start, nf.end, nf.K, nf.Kp, nap_x3, w.nap_x}
                          : (fit ? *fit : DiffSink{});
  // route diff layer j's diffs into the operand (columns relative to the range's first)
  auto nap_route = [&](GemmEpi& ep, int j) {
    if (!routed || j < sk.start || j >= sk.end) return;
    const int col = diff_col(h, j) - diff_col(h, sk.start);
    if (sk.x3) {
      ep.dp_hi = sk.x;
      ep.dp_lo = (char*)sk.x + (size_t)w.Mpe * sk.Kp * 2;
      ep.lddp = sk.Kp;
      ep.dp_col = col;
    } else {
      ep.diff = (float*)sk.x + col;
      ep.lddiff = sk.Kp;
    }
  };
  // the operand's padding, every batch: a ragged batch's workspace is carved
  // at other offsets than the full batches', so nothing survives from them
  if (routed)
    RET_IF(mmad_zero_pad(sk.x3 ? 2 : 4, sk.x3 ? 2 : 1, B, sk.K, w.Mpe, sk.Kp, sk.x, st));
  // pass 1: eval forward; the decoder's last layer scores d0 = x_hat - x
  for (int l = 0; l < nL; ++l) {
    const AeLayer& a = h->L[l];
    LayerWS& s = w.l[l];
    const int M = rows_of(w, a), Mp = prows_of(w, a);
    const float *isc, *ish;
    const void* in = input_of(h, w, l, false, &isc, &ish);
    GemmEpi ep = fwd_epi(h, w, a, s, M, a.bn ? s.y : s.out, false);
    if (a.bn) {
      RET_IF(mmad_bn_eval_affine(a.N, a.Np, h->params + a.g_off, h->params + a.be_off,
                                 running_mean(h, a), running_var(h, a), h->bn_eps, s.scale,
                                 s.shift, st));
      ep.bn_scale = s.scale;
      ep.bn_shift = s.shift;
    }
    const void* wt = weights_dt(h, a, dt, ep);
    if (l == nL - 1) {
      ep.ref = x3 ? (const void*)x : w.xin;
      ep.ldref = x3 ? ld_x : a.Np;
      ep.rowsq = s.rowsq;
      ep.ldrow = Mp;
      ep.diff = diffs;
      ep.lddiff = ld_diff;
      nap_route(ep, 0);
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_SCORE, in, a.Kp, wt, a.Kp, Mp, a.Np, a.Kp, ep, st));
    } else {
      if (x3 && a.enc) {
        ep.out32 = s.ref32;
        ep.ld32 = a.Np;
      }
      RET_IF(ae_gemm(h, w, dt, GEMM_EPI_FWD, in, a.Kp, wt, a.Kp, Mp, a.Np, a.Kp, ep, st));
    }
    if (h->vib && l == h->n_enc - 1) {
      RET_IF(mmad_vib_reparam_fwd(dt, B, h->btl, 1, s.out, a.Np, nullptr, nullptr, 0, 0, 1, w.zbuf,
                                  h->L[h->n_enc].Kp, nullptr, st));
    }
  }
  // pass 2: x_hat through the encoder, diff against pass-1 activations
  const void* cur = w.l[nL - 1].out;
  int coff = h->L[0].K;
  for (int e = 0; e < h->n_enc; ++e) {
    const AeLayer& a = h->L[e];
    LayerWS& s = w.l[e];
    GemmEpi ep = fwd_epi(h, w, a, s, B, s.dy, false);
    if (a.bn) {
      ep.bn_scale = s.scale;
      ep.bn_shift = s.shift;
    }
    ep.ref = x3 ? (const void*)s.ref32 : (a.bn ? s.y : s.out);
    ep.ldref = a.Np;
    ep.rowsq = s.rowsq;
    ep.ldrow = w.Mpe;
    ep.diff = diffs ? diffs + coff : nullptr;
    ep.lddiff = ld_diff;
    nap_route(ep, e + 1);
    const void* wt = weights_dt(h, a, dt, ep);
    RET_IF(ae_gemm(h, w, dt, GEMM_EPI_SCORE, cur, a.Kp, wt, a.Kp, w.Mpe, a.Np, a.Kp, ep, st));
    coff += a.N;
    cur = s.dy;
  }
  // per-window sums: layer_sq[0] from the decoder's last layer, [1+e] from pass 2
  MmadReduceJobs jobs{};
  const AeLayer& last = h->L[nL - 1];
  jobs.j[0] = MmadReduceJob{w.l[nL - 1].rowsq, layer_sq, last.Np / 128, w.Mpd, B, B, 1.f, 0,
                            nullptr, 0, 0.f};
  for (int e = 0; e < h->n_enc; ++e)
    jobs.j[e + 1] = MmadReduceJob{w.l[e].rowsq, layer_sq + (size_t)(e + 1) * ld_sq,
                                  h->L[e].Np / 128, w.Mpe, B, B, 1.f, 0, nullptr, 0, 0.f};
  MMAD_CHECK_ARG(h->n_enc + 1 <= MMAD_MAX_REDUCE_JOBS, "too many encoder layers");
  RET_IF(mmad_reduce_jobs(jobs, h->n_enc + 1, B, st));
  if (!nap) return MMAD_OK;
  // the NAP run as mmad_nap_score forms it: one SCORE GEMM (no reference, bias
  // after the product, colw = w) and the column sum of its row partials
  GemmEpi ep{};
  ep.M = B; ep.N = nf.R; ep.out = nullptr; ep.ldo = nf.Rp; ep.bias = nf.bias; ep.act = MMAD_ACT_NONE;
  ep.ref = nullptr; ep.ldref = nf.Rp; ep.rowsq = w.nap_rowsq; ep.ldrow = w.Mpe; ep.colw = nf.w;
  const void* vt = nap_x3 ? (const void*)nf.vt_planes : (const void*)nf.vt;
  RET_IF(ae_gemm(h, w, nf.dtype, GEMM_EPI_SCORE, w.nap_x, nf.Kp, vt, nf.Kp, w.Mpe, nf.Rp, nf.Kp, ep, st));
  // (N = Np = B: nothing past nap[B) is written -- the next batch's scores, or the caller's memory)
  return mmad_colsum(nf.Rp / 128, B, B, w.nap_rowsq, w.Mpe, 1.f / (float)nf.R, nap, st);
}

// a NAP-writing entry point's preconditions (nothing is launched on failure)
static int check_nap(const mmad_ae* h, const float* nap, const char* who) {
  MMAD_CHECK_ARG(nap, "%s: null nap output", who);
  MMAD_CHECK_ARG(h->nap.on, "%s: no NAP fit attached (mmad_ae_set_nap)", who);
  MMAD_CHECK_ARG(h->nap.dtype != MMAD_BF16X3 || score_dt(h) == MMAD_BF16X3,
                 "%s: the attached fit's MMAD_BF16X3 NAP GEMM needs the score planes it was attached with", who);
  return MMAD_OK;
}

int mmad_ae_score_nap(mmad_ae* h, const float* x, int ld_x, int B, float* layer_sq, float* nap,
                      void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->running, "ae_score_nap: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && layer_sq, "ae_score_nap: bad args");
  RET_IF(check_nap(h, nap, "ae_score_nap"));
  AeWS w;
  carve(h, B >= 1 ? B : 1, 1, nullptr, w);
  MMAD_CHECK_ARG(B >= 1 && ws && ws_bytes >= w.bytes, "ae_score_nap: bad batch or workspace too small");
  RET_IF(refresh_planes(h, (hipStream_t)stream));
  RET_IF(prepare_ws(h, B, 1, ws, ws_bytes, w, (hipStream_t)stream));
  return score_batch(h, x, ld_x, B, layer_sq, B, nullptr, w, (hipStream_t)stream, nap);
}

int mmad_ae_score(mmad_ae* h, const float* x, int ld_x, int B, float* layer_sq, float* diffs,
                  void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->running, "ae_score: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && layer_sq, "ae_score: bad args");
  RET_IF(refresh_planes(h, (hipStream_t)stream));
  AeWS w;
  RET_IF(prepare_ws(h, B, 1, ws, ws_bytes, w, (hipStream_t)stream));
  return score_batch(h, x, ld_x, B, layer_sq, B, diffs, w, (hipStream_t)stream);
}

// base of the weight operand the score GEMMs read (a captured pass's key)
static const void* score_weights(const mmad_ae* h) {
  return h->planes ? (const void*)h->planes : weights(h, h->L[0]);
}

// the whole N-window pass, batch by batch, on stream st
static int score_pass(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch, float* layer_sq,
                      int64_t ld_sq, float* nap, void* ws, int64_t ws_bytes, hipStream_t st) {
  for (int64_t s0 = 0; s0 < N; s0 += batch) {
    const int B = (int)std::min<int64_t>(batch, N - s0);
    AeWS w;
    RET_IF(prepare_ws(h, B, 1, ws, ws_bytes, w, st));
    RET_IF(score_batch(h, x + s0 * ld_x, ld_x, B, layer_sq + s0, ld_sq, nullptr, w, st,
                       nap ? nap + s0 : nullptr));
  }
  return MMAD_OK;
}

// the streaming pass, with the NAP output (nullable: the pass without NAP)
static int score_stream(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch, float* layer_sq,
                        int64_t ld_sq, float* nap, void* ws, int64_t ws_bytes, int use_graph,
                        void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->running, "ae_score_stream: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && layer_sq && N >= 1 && batch >= 1 && ld_sq >= N,
                 "ae_score_stream: bad args (N=%lld batch=%d ld_sq=%lld)", (long long)N, batch,
                 (long long)ld_sq);
  hipStream_t st = (hipStream_t)stream;
  // stale score planes are re-split here, on the caller's stream and outside
  // the captured pass: a replay reads whatever the planes hold when it runs
  RET_IF(refresh_planes(h, st));
  const void* nap_vt = nap ? (const void*)h->nap.vt : nullptr;
  if (!use_graph) return score_pass(h, x, ld_x, N, batch, layer_sq, ld_sq, nap, ws, ws_bytes, st);
  for (auto& g : h->graphs) {
    if (g.x == x && g.ld_x == ld_x && g.N == N && g.batch == batch && g.sq == layer_sq &&
        g.ld_sq == ld_sq && g.ws == ws && g.wts == score_weights(h) && g.nap == nap &&
        g.nap_vt == nap_vt) {
      MMAD_HIP_CHECK(hipGraphLaunch(g.exec, st));
      return MMAD_OK;
    }
  }
  // first pass of this shape: run it eagerly (that also settles every GEMM
  // tile choice, which cannot be timed under capture), then capture the same
  // launches on the handle's capture stream for the next calls
  RET_IF(score_pass(h, x, ld_x, N, batch, layer_sq, ld_sq, nap, ws, ws_bytes, st));
  if (!h->gstream) MMAD_HIP_CHECK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  MMAD_HIP_CHECK(hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
  const int rc = score_pass(h, x, ld_x, N, batch, layer_sq, ld_sq, nap, ws, ws_bytes, h->gstream);
  const hipError_t ec = hipStreamEndCapture(h->gstream, &graph);
  if (rc != MMAD_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  MMAD_HIP_CHECK(ec);
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  MMAD_HIP_CHECK(ei);
  if (h->graphs.size() >= 8) {   // bounded cache: drop the oldest pass
    (void)hipGraphExecDestroy(h->graphs.front().exec);
    h->graphs.erase(h->graphs.begin());
  }
  h->graphs.push_back({x, ld_x, N, batch, layer_sq, ld_sq, ws, score_weights(h), nap, nap_vt, exec});
  return MMAD_OK;
}

int mmad_ae_score_stream(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch,
                         float* layer_sq, int64_t ld_sq, void* ws, int64_t ws_bytes, int use_graph,
                         void* stream) {
  return score_stream(h, x, ld_x, N, batch, layer_sq, ld_sq, nullptr, ws, ws_bytes, use_graph, stream);
}

int mmad_ae_score_nap_stream(mmad_ae* h, const float* x, int ld_x, int64_t N, int batch,
                             float* layer_sq, int64_t ld_sq, float* nap, void* ws, int64_t ws_bytes,
                             int use_graph, void* stream) {
  MMAD_CHECK_ARG(h, "ae_score_nap_stream: null handle");
  RET_IF(check_nap(h, nap, "ae_score_nap_stream"));
  MMAD_CHECK_ARG(batch >= 1 && ws && ws_bytes >= mmad_ae_workspace_bytes(h, batch, 1),
                 "ae_score_nap_stream: bad batch or workspace too small");
  return score_stream(h, x, ld_x, N, batch, layer_sq, ld_sq, nap, ws, ws_bytes, use_graph, stream);
}

// ---- streaming NAP fit ------------------------------------------------------
// the fit's part of its workspace, after the scoring workspace of `batch`
// windows: the packed fp32 operand [Mpe][Kp] and the passes' layer sums
struct NapFitWS {
  int W, Kp;
  int64_t score_bytes, x_off, sq_off, bytes;
};
static bool nap_fit_carve(const mmad_ae* h, int batch, int start, int end, NapFitWS& f) {
  if (!h || batch < 1 || start < 0 || end <= start || end > h->n_enc + 1) return false;
  f.W = diff_col(h, end) - diff_col(h, start);
  f.Kp = mmad_roundup(f.W, MMAD_PAD);
  const int64_t Mp = mmad_roundup(batch, MMAD_PAD);
  f.score_bytes = mmad_ae_workspace_bytes(h, batch, 1);
  f.x_off = (f.score_bytes + 255) / 256 * 256;
  f.sq_off = f.x_off + Mp * f.Kp * 4;
  f.bytes = f.sq_off + (int64_t)(h->n_enc + 1) * Mp * 4;
  return true;
}

int64_t mmad_ae_nap_fit_workspace_bytes(const mmad_ae* h, int batch, int start, int end) {
  NapFitWS f;
  return nap_fit_carve(h, batch, start, end, f) ? f.bytes : -1;
}

int mmad_ae_nap_fit_stream(mmad_ae* h, int start, int end, const float* x, int ld_x, int64_t N,
                           int batch, float* mu_r, float* v, float* mu_s, float* var,
                           void* fit_state, int64_t fit_bytes, void* ws, int64_t ws_bytes,
                           void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->running, "ae_nap_fit_stream: unbound handle");
  MMAD_CHECK_ARG(start >= 0 && end > start && end <= h->n_enc + 1,
                 "ae_nap_fit_stream: bad layer range [%d, %d) of %d diff layers", start, end, h->n_enc + 1);
  MMAD_CHECK_ARG(N >= 2, "ae_nap_fit_stream: a fit needs N >= 2 windows (N=%lld)", (long long)N);
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && batch >= 1, "ae_nap_fit_stream: bad input or batch");
  MMAD_CHECK_ARG(mu_r && v && mu_s && var, "ae_nap_fit_stream: null output");
  NapFitWS f;
  nap_fit_carve(h, batch, start, end, f);
  MMAD_CHECK_ARG(ws && ws_bytes >= f.bytes, "ae_nap_fit_stream: workspace too small (%lld < %lld bytes)",
                 (long long)ws_bytes, (long long)f.bytes);
  MMAD_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "ae_nap_fit_stream: workspace must be 256-byte aligned");
  const int64_t need = mmad_nap_fit_state_bytes(f.W);
  MMAD_CHECK_ARG(fit_state && need > 0 && fit_bytes >= need && ((uintptr_t)fit_state) % 256 == 0,
                 "ae_nap_fit_stream: fit state too small or unaligned (%lld < %lld bytes)",
                 (long long)fit_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  float* op = (float*)((char*)ws + f.x_off);
  float* sq = (float*)((char*)ws + f.sq_off);
  const DiffSink sink{start, end, f.W, f.Kp, false, op};
  RET_IF(refresh_planes(h, st));
  RET_IF(mmad_nap_fit_begin(f.W, fit_state, fit_bytes, stream));
  for (int pass = 0; pass < 3; ++pass) {
    for (int64_t s0 = 0; s0 < N; s0 += batch) {
      const int B = (int)std::min<int64_t>(batch, N - s0);
      AeWS w;
      RET_IF(prepare_ws(h, B, 1, ws, f.score_bytes, w, st));
      RET_IF(score_batch(h, x + s0 * ld_x, ld_x, B, sq, w.Mpe, nullptr, w, st, nullptr, &sink));
      if (pass == 0)
        RET_IF(mmad_nap_fit_accumulate_sums(f.W, B, op, f.Kp, fit_state, fit_bytes, stream));
      else if (pass == 1)
        RET_IF(mmad_nap_fit_accumulate_gram(f.W, B, op, f.Kp, mu_r, fit_state, fit_bytes, stream));
      else
        RET_IF(mmad_nap_fit_accumulate_rot(f.W, N, B, op, f.Kp, mu_r, fit_state, fit_bytes, stream));
    }
    if (pass == 0)
      RET_IF(mmad_nap_fit_finish_mean(f.W, N, fit_state, fit_bytes, mu_r, stream));
    else if (pass == 1)
      RET_IF(mmad_nap_fit_solve(f.W, N, fit_state, fit_bytes, v, stream));
    else
      RET_IF(mmad_nap_fit_finish(f.W, N, fit_state, fit_bytes, mu_s, var, stream));
  }
  return MMAD_OK;
}

int mmad_ae_status(mmad_ae* h, void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h, "ae_status: null handle");
  // no split-K GEMM / fused-BN barrier can have run unless the dtype /
  // override / BN mode allows one
  if ((!splitk_possible(h->dtype) && h->bn_mode != 2 && h->bn_mode_bwd != 2) || !ws)
    return MMAD_OK;
  AeWS w;
  carve(h, 1, 1, (char*)ws, w);
  MMAD_CHECK_ARG(ws_bytes >= w.bytes, "ae_status: workspace too small");
  for (int r = 0; r < 2; ++r)
    RET_IF(mmad_gemm_read_status(w.sk_ctl[r], (hipStream_t)stream, "ae_status"));
  if ((h->bn_mode == 2 || h->bn_mode_bwd == 2) && w.bn_err) {
    unsigned word = 0;
    MMAD_HIP_CHECK(hipMemcpyAsync(&word, w.bn_err, sizeof(word), hipMemcpyDeviceToHost, (hipStream_t)stream));
    MMAD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (word) {
      // re-zero every control word (a barrier that gave up may have left
      // counters raised) for the next call
      MMAD_HIP_CHECK(hipMemsetAsync(w.sk_ctl[0], 0, w.sk_ctl_bytes, (hipStream_t)stream));
      MMAD_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
      mmad_set_error("ae_status: a fused BatchNorm column barrier timed out; the outputs of that "
                     "call are invalid");
      return MMAD_EHIP;
    }
  }
  return MMAD_OK;
}

int mmad_ae_probe(mmad_ae* h, int kind, int layer, int capacity) {
  MMAD_CHECK_ARG(h, "ae_probe: null handle");
  MMAD_CHECK_ARG(kind >= 0 && kind <= 3,
                 "ae_probe: kind must be 0 / 1 (forward / dW GEMM) or 2 / 3 (the same, kernel-attached events)");
  MMAD_CHECK_ARG(capacity >= 0 && capacity <= 4096, "ae_probe: capacity out of range");
  MMAD_CHECK_ARG(layer < 0 || layer < (int)h->L.size(), "ae_probe: bad layer %d", layer);
  for (auto e : h->probe_ev) (void)hipEventDestroy(e);
  h->probe_ev.clear();
  h->probe_n = 0;
  h->probe_id = -1;
  h->probe_mask = 0;
  h->probe_kev = kind >= 2;
  if (layer < 0 || capacity == 0) return MMAD_OK;
  h->probe_ev.resize(2 * (size_t)capacity, nullptr);
  for (auto& e : h->probe_ev) MMAD_HIP_CHECK(hipEventCreate(&e));
  if (!h->probe_sync) MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->probe_sync, hipEventDisableTiming));
  h->probe_id = ((kind & 1) == 0 ? PROBE_FWD : PROBE_DW) + layer;
  return MMAD_OK;
}

int mmad_ae_probe_layers(const mmad_ae* h) { return h ? (int)h->probe_mask : -1; }

int mmad_ae_set_dw_group(mmad_ae* h, int blocks, int members) {
  if (!h) {
    mmad_set_error("ae_set_dw_group: null handle");
    return MMAD_EINVAL;
  }
  if (blocks >= -1) h->dw_group_blocks = blocks;
  if (members > 0) h->dw_group_members = members;
  return MMAD_OK;
}

int mmad_ae_probe_read(mmad_ae* h, float* ms, int max_n) {
  if (!h || !ms || max_n < 0) {
    mmad_set_error("ae_probe_read: bad arguments");
    return MMAD_EINVAL;
  }
  const int n = std::min(h->probe_n, max_n);
  for (int i = 0; i < n; ++i) {
    MMAD_HIP_CHECK(hipEventSynchronize(h->probe_ev[2 * i + 1]));
    MMAD_HIP_CHECK(hipEventElapsedTime(&ms[i], h->probe_ev[2 * i], h->probe_ev[2 * i + 1]));
  }
  return n;
}

int mmad_ae_graph_count(const mmad_ae* h) {
  return h ? (int)(h->graphs.size() + h->ographs.size()) : -1;
}

int mmad_ae_clear_graphs(mmad_ae* h) {
  MMAD_CHECK_ARG(h, "ae_clear_graphs: null handle");
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
  h->graphs.clear();
  for (auto& g : h->ographs) (void)hipGraphExecDestroy(g.exec);
  h->ographs.clear();
  h->online_ready = nullptr;   // a new fit: another operand width
  return MMAD_OK;
}

// ---- online scoring: B <= 16 windows through the 16-row weight stream -------
// (mmad_skinny.hip).  The batch path above pads such a call to 128 rows and
// spends its ~30 launches on zeros; here every layer is one launch that reads
// its weights once.  All buffers live in a caller-owned state, carved below.
struct OnlineWS {
  void* xin = nullptr;             // packed input [16][Kp0]
  std::vector<void*> y, p2;        // pass-1 outputs per layer; pass-2 outputs per encoder layer
  void* zbuf = nullptr;            // VIB: z [128][Kp] as mmad_vib_reparam_fwd writes it
  float *scale = nullptr, *shift = nullptr;   // folded eval-BN constants [n_bn]
  std::vector<float*> rs;          // row partials per diff layer [Np/16][16]
  float* nap_x = nullptr;          // packed NAP operand [16][nap.Kp] (fp32)
  float* nap_rs = nullptr;         // the NAP launch's row partials [Rp/16][16]
  int64_t bytes = 0;
};

static void online_carve(const mmad_ae* h, char* base, OnlineWS& o) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) -> char* {
    off = (off + 255) / 256 * 256;
    char* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  };
  const int64_t E = (int64_t)esz(h->dtype);
  const int nL = (int)h->L.size();
  o.xin = take(16 * h->L[0].Kp * E);
  o.y.resize(nL);
  for (int l = 0; l < nL; ++l) o.y[l] = take(16 * h->L[l].Np * E);
  if (h->vib) o.zbuf = take((int64_t)MMAD_PAD * h->L[h->n_enc].Kp * E);
  o.p2.resize(h->n_enc);
  for (int e = 0; e < h->n_enc; ++e) o.p2[e] = take(16 * h->L[e].Np * E);
  o.scale = (float*)take(std::max<int64_t>(h->n_bn, 1) * 4);
  o.shift = (float*)take(std::max<int64_t>(h->n_bn, 1) * 4);
  o.rs.resize(h->n_enc + 1);
  o.rs[0] = (float*)take((int64_t)h->L[nL - 1].Np * 4);   // [Np/16][16]
  for (int e = 0; e < h->n_enc; ++e) o.rs[e + 1] = (float*)take((int64_t)h->L[e].Np * 4);
  if (h->nap.on) {
    o.nap_x = (float*)take(16 * (int64_t)h->nap.Kp * 4);
    o.nap_rs = (float*)take((int64_t)h->nap.Rp * 4);
  }
  o.bytes = (off + 255) / 256 * 256;
}

int64_t mmad_ae_online_state_bytes(const mmad_ae* h) {
  if (!h) return -1;
  OnlineWS o;
  online_carve(h, nullptr, o);
  return o.bytes;
}

// the launches of one pass on stream st (eager, or into a capture)
static int online_pass(mmad_ae* h, const float* x, int ld_x, int B, int s0, int s1, const float* thr,
                       float* out, uint8_t* flags, const OnlineWS& o, hipStream_t st) {
  const int dt = h->dtype;
  const int nL = (int)h->L.size();
  const mmad_ae::NapFit& nf = h->nap;
  RET_IF(mmad_pack_input(dt, B, h->L[0].K, 16, h->L[0].Kp, x, ld_x, o.xin, st));
  MmadOnlineFold f{};
  f.n_bn = (int)h->n_bn;
  for (const AeLayer& a : h->L)
    if (a.bn) {
      f.bn_off[f.n] = (int)a.bn_off; f.N[f.n] = a.N; f.g_off[f.n] = a.g_off; f.be_off[f.n] = a.be_off;
      ++f.n;
    }
  RET_IF(mmad_online_fold(f, h->params, h->running, h->bn_eps, o.scale, o.shift, st));
  // diff layer j's diffs into the NAP operand (columns relative to the range's first)
  auto route = [&](MmadSkinny& a, int j) {
    if (!nf.on || j < nf.start || j >= nf.end) return;
    a.diff = o.nap_x + (diff_col(h, j) - diff_col(h, nf.start));
    a.lddiff = nf.Kp;
  };
  auto layer = [&](const AeLayer& L, const void* in, void* y) {
    MmadSkinny a{};
    a.M = B; a.N = L.N; a.Np = L.Np; a.Kp = L.Kp;
    a.x = in; a.w = weights(h, L); a.bias = h->params + L.b_off; a.act = L.act; a.slope = h->slope;
    if (L.bn) { a.scale = o.scale + L.bn_off; a.shift = o.shift + L.bn_off; }
    a.y = y;
    return a;
  };
  // pass 1: eval forward; the decoder's last layer scores d0 = x_hat - x
  for (int l = 0; l < nL; ++l) {
    const AeLayer& L = h->L[l];
    const void* in = l == 0 ? o.xin : (h->vib && l == h->n_enc ? o.zbuf : o.y[l - 1]);
    MmadSkinny a = layer(L, in, o.y[l]);
    if (l == nL - 1) {
      a.ref = o.xin; a.ref_f32 = 0; a.ldref = h->L[0].Kp;
      a.rowsq = o.rs[0];
      route(a, 0);
    }
    RET_IF(mmad_skinny_launch(dt, a, st));
    if (h->vib && l == h->n_enc - 1)
      RET_IF(mmad_vib_reparam_fwd(dt, B, h->btl, 1, o.y[l], L.Np, nullptr, nullptr, 0, 0, 1, o.zbuf,
                                  h->L[h->n_enc].Kp, nullptr, st));
  }
  // pass 2: x_hat through the encoder, each layer against its pass-1 output
  const void* cur = o.y[nL - 1];
  for (int e = 0; e < h->n_enc; ++e) {
    const AeLayer& L = h->L[e];
    MmadSkinny a = layer(L, cur, o.p2[e]);
    a.ref = o.y[e]; a.ref_f32 = 0; a.ldref = L.Np;
    a.rowsq = o.rs[e + 1];
    route(a, e + 1);
    RET_IF(mmad_skinny_launch(dt, a, st));
    cur = o.p2[e];
  }
  // the NAP run: the same kernel on the fit's fp32 V^T (K = W, N = R), bias
  // after the product, colw = 1 / var, no reference
  if (nf.on) {
    MmadSkinny a{};
    a.M = B; a.N = nf.R; a.Np = nf.Rp; a.Kp = nf.Kp;
    a.x = o.nap_x; a.w = nf.vt; a.bias = nf.bias; a.act = MMAD_ACT_NONE;
    a.colw = nf.w; a.rowsq = o.nap_rs;
    RET_IF(mmad_skinny_launch(MMAD_F32, a, st));
  }
  MmadOnlineFinish fin{};
  fin.B = B; fin.n_diff = h->n_enc + 1;
  fin.rs[0] = o.rs[0]; fin.tiles[0] = h->L[nL - 1].Np / 16; fin.widths[0] = h->L[0].K;
  for (int e = 0; e < h->n_enc; ++e) {
    fin.rs[e + 1] = o.rs[e + 1]; fin.tiles[e + 1] = h->L[e].Np / 16; fin.widths[e + 1] = h->L[e].N;
  }
  fin.sap_start = s0; fin.sap_end = s1;
  if (nf.on) { fin.nap_rs = o.nap_rs; fin.nap_tiles = nf.Rp / 16; fin.nap_scale = 1.f / (float)nf.R; }
  fin.out = out; fin.flags = flags; fin.thresholds = thr;
  return mmad_online_finish(fin, st);
}

int mmad_ae_online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                         const float* thresholds, float* out, uint8_t* flags, void* state,
                         int64_t state_bytes, int use_graph, void* stream) {
  MMAD_CHECK_ARG(h, "ae_online_score: null handle");
  MMAD_CHECK_ARG(B >= 1 && B <= 16, "ae_online_score: B=%d outside 1..16 (the batch path, "
                 "mmad_ae_score_stream, serves larger calls)", B);
  const int64_t need = mmad_ae_online_state_bytes(h);
  MMAD_CHECK_ARG(state && state_bytes >= need, "ae_online_score: online state null or too small "
                 "(%lld < %lld bytes, mmad_ae_online_state_bytes)", (long long)(state ? state_bytes : 0),
                 (long long)need);
  MMAD_CHECK_ARG(((uintptr_t)state) % 256 == 0, "ae_online_score: state must be 256-byte aligned");
  MMAD_CHECK_ARG(h->params && h->running, "ae_online_score: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && out, "ae_online_score: bad args (null x / out, ld_x=%d)", ld_x);
  MMAD_CHECK_ARG(score_dt(h) != MMAD_BF16X3, "ae_online_score: score planes attached "
                 "(MMAD_BF16X3): split-bf16 planes are not supported on the online path");
  MMAD_CHECK_ARG(!h->nap.on || h->nap.dtype == MMAD_F32, "ae_online_score: the attached fit's NAP "
                 "GEMM is MMAD_BF16X3: not supported on the online path (attach an MMAD_F32 fit)");
  const int nd = h->n_enc + 1;
  MMAD_CHECK_ARG(nd <= MMAD_ONLINE_MAX_DIFF && (int)h->L.size() <= MMAD_ONLINE_MAX_LAYERS,
                 "ae_online_score: too many layers");
  // the reference's clamping (utils/metric.py:155-171)
  int s0 = sap_start < 0 ? 0 : sap_start, s1 = sap_end;
  if (s0 > nd - 1) s0 = nd - 1;
  if (s1 - s0 < 1) s1 = s0 + 1;
  if (s1 > nd) s1 = nd;
  hipStream_t st = (hipStream_t)stream;
  OnlineWS o;
  online_carve(h, (char*)state, o);
  if (h->nap.on && h->online_ready != state) {
    MMAD_HIP_CHECK(hipMemsetAsync(o.nap_x, 0, 16 * (size_t)h->nap.Kp * 4, st));
    h->online_ready = state;
  }
  if (!use_graph) return online_pass(h, x, ld_x, B, s0, s1, thresholds, out, flags, o, st);
  const void* wts = weights(h, h->L[0]);
  const void* nap_vt = h->nap.on ? (const void*)h->nap.vt : nullptr;
  for (auto& g : h->ographs) {
    if (g.x == x && g.ld_x == ld_x && g.B == B && g.sap_start == s0 && g.sap_end == s1 &&
        g.thr == thresholds && g.out == out && g.flags == flags && g.state == state && g.wts == wts &&
        g.nap_vt == nap_vt) {
      MMAD_HIP_CHECK(hipGraphLaunch(g.exec, st));
      return MMAD_OK;
    }
  }
  RET_IF(online_pass(h, x, ld_x, B, s0, s1, thresholds, out, flags, o, st));
  if (!h->gstream) MMAD_HIP_CHECK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  MMAD_HIP_CHECK(hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
  const int rc = online_pass(h, x, ld_x, B, s0, s1, thresholds, out, flags, o, h->gstream);
  const hipError_t ec = hipStreamEndCapture(h->gstream, &graph);
  if (rc != MMAD_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  MMAD_HIP_CHECK(ec);
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  MMAD_HIP_CHECK(ei);
  if (h->ographs.size() >= 8) {   // bounded cache: drop the oldest pass
    (void)hipGraphExecDestroy(h->ographs.front().exec);
    h->ographs.erase(h->ographs.begin());
  }
  h->ographs.push_back({x, ld_x, B, s0, s1, thresholds, out, flags, state, wts, nap_vt, exec});
  return MMAD_OK;
}
