// Internal (non-ABI) state of the whole-autoencoder executor: the handle, the
// workspace carve and the helpers shared by mmad_ae.hip (lifecycle, workspace, forward, Adam,
// status, probe), mmad_ae_train.hip (training executor, data parallel), mmad_ae_score.hip
// (batch / streaming score path, NAP fit) and mmad_ae_online.hip (16-row online path), plus
// the one capture-and-replay cache behind their hipGraph paths.
#pragma once
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

namespace mmad_ae_impl {

struct AeLayer {
  int K, N, Kp, Np;
  int act, bn, enc;
  int64_t w_off, b_off, g_off, be_off, bn_off;
};

// Bounded cache of instantiated hipGraphs, oldest first.  Key: a plain struct
// with operator== holding everything a captured pass bakes in (its call
// signature).  A hit is a linear scan over at most `cap` keys, no allocation.
template <class Key>
class GraphCache {
 public:
  explicit GraphCache(size_t cap) : cap_(cap) {}
  GraphCache(const GraphCache&) = delete;
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() { clear(); }
  hipGraphExec_t find(const Key& key) const {
    for (const Entry& e : entries_)
      if (e.key == key) return e.exec;
    return nullptr;
  }
  // takes ownership of exec; a full cache drops its oldest entry
  void insert(const Key& key, hipGraphExec_t exec) {
    if (entries_.size() >= cap_) {
      (void)hipGraphExecDestroy(entries_.front().exec);
      entries_.erase(entries_.begin());
    }
    entries_.push_back(Entry{key, exec});
  }
  void clear() {
    for (Entry& e : entries_) (void)hipGraphExecDestroy(e.exec);
    entries_.clear();
  }
  size_t size() const { return entries_.size(); }

 private:
  struct Entry { Key key; hipGraphExec_t exec; };
  std::vector<Entry> entries_;
  size_t cap_;
};

// the key of a captured mmad_ae_score_stream pass: one graph per (input,
// output, workspace, N, batch)
struct ScoreKey {
  const float* x; int64_t ld_x, N; int batch; float* sq; int64_t ld_sq; void* ws;
  const void* wts;   // weight operand base (the bf16 shadow may be re-pointed)
  float* nap;        // NAP output (null: a pass without it) and the fit it was captured with
  const void* nap_vt;
  bool operator==(const ScoreKey& o) const {
    return x == o.x && ld_x == o.ld_x && N == o.N && batch == o.batch && sq == o.sq &&
           ld_sq == o.ld_sq && ws == o.ws && wts == o.wts && nap == o.nap && nap_vt == o.nap_vt;
  }
};
// ... of a captured mmad_ae_online_score / mmad_ae_online_score64 pass; rows:
// the entry point's row capacity (16 / 64: other kernels, other layouts).  A
// grouped pass (mmad_ae_online_score_groups) adds G > 0, the bounds' values
// (zero beyond G) and its buffers; an ungrouped one leaves them all zero
// A sensor tick (mmad_ae_online_tick) adds what its front launches read and
// write: the raw queues and their types, the MFCC parameters and buffers, the
// packed HSR weights and the ranges; a pass without the front leaves them zero
struct TickKey {
  const void *pcm = nullptr, *r = nullptr, *d = nullptr, *t = nullptr;
  int pcm_type = 0, r_type = 0, d_type = 0;
  int64_t L = 0;
  int sr = 0, n_fft = 0, n_mels = 0, n_mfcc = 0;
  const void *plan = nullptr, *mfcc_ws = nullptr, *mfcc_out = nullptr, *mfcc_norm = nullptr, *hsr_w = nullptr;
  float range_in[6] = {};
  int norm_rcp = 0;
  bool operator==(const TickKey& o) const {
    return norm_rcp == o.norm_rcp && pcm == o.pcm && r == o.r && d == o.d && t == o.t && pcm_type == o.pcm_type && r_type == o.r_type &&
           d_type == o.d_type && L == o.L && sr == o.sr && n_fft == o.n_fft && n_mels == o.n_mels &&
           n_mfcc == o.n_mfcc && plan == o.plan && mfcc_ws == o.mfcc_ws && mfcc_out == o.mfcc_out &&
           mfcc_norm == o.mfcc_norm && hsr_w == o.hsr_w && std::equal(range_in, range_in + 6, o.range_in);
  }
};
struct OnlineKey {
  const float* x; int ld_x, B, sap_start, sap_end; const float* thr; float* out; uint8_t* flags;
  void* state; const void* wts; const void* nap_vt;
  int rows;
  int G = 0;
  int bounds[MMAD_MAX_GROUPS + 1] = {};
  const float* gthr = nullptr; float* gout = nullptr; uint8_t* gflags = nullptr; void* gstate = nullptr;
  TickKey tick;
  bool operator==(const OnlineKey& o) const {
    return x == o.x && ld_x == o.ld_x && B == o.B && sap_start == o.sap_start && sap_end == o.sap_end &&
           thr == o.thr && out == o.out && flags == o.flags && state == o.state && wts == o.wts &&
           nap_vt == o.nap_vt && rows == o.rows && G == o.G &&
           std::equal(bounds, bounds + MMAD_MAX_GROUPS + 1, o.bounds) && gthr == o.gthr &&
           gout == o.gout && gflags == o.gflags && gstate == o.gstate && tick == o.tick;
  }
};
// ... of a captured fused train step (mmad_ae_train_step_graph)
struct TrainKey {
  int B, k, ld_x, xvec, has_eps, dw_main, ev_every, keep_grads;
  const void* ws;
  const void* shadow;   // the bf16 shadow the captured kernels read / write
  float beta_kl, b1, b2, aeps;
  bool operator==(const TrainKey& o) const {
    return B == o.B && k == o.k && ld_x == o.ld_x && xvec == o.xvec && has_eps == o.has_eps &&
           ws == o.ws && shadow == o.shadow && dw_main == o.dw_main && ev_every == o.ev_every &&
           keep_grads == o.keep_grads && beta_kl == o.beta_kl && b1 == o.b1 && b2 == o.b2 &&
           aeps == o.aeps;
  }
};

// The schedule of one executor handle: built once from the tune table by
// schedule_from_knobs (mmad_ae.hip) when the handle is created and constant
// from then on -- one schedule per handle, whatever the table says later.
// Nothing else in the executor reads a schedule knob.  (The grouped-dW budget,
// mmad_ae::dw_group_blocks / dw_group_members, is the one schedule choice that
// can change after create, through mmad_ae_set_dw_group; it is not in here.)
// AeWS carries each call's resolution of these (bn_mode, bn_mode_bwd, dw_main,
// ping).
struct AeSchedule {
  unsigned ev_flags_ = 0;   // flags of the executor's events (knob 27; ev_flags, mmad_ae.hip)
  int loss_side = 1;     // knob 23: reduce the loss on the side stream after the forward
  int side_prio_hi = 0;   // knob 26
  // knob 15: > 0 = the side stream is created behind a CU mask that leaves
  // this many CUs (evenly spaced over the mask) to the main stream alone
  int side_cu_held = 0;
  // data-parallel step: the small bucket (bias / gamma / beta grads + loss)
  // goes on the comm stream right after the bwd-data GEMM of this layer
  // (ahead of this layer's and the lower layers' weight buckets); knob 24
  int dp_small_at = 1;
  // data-parallel step: sharded weight buckets (knob 28)
  int dp_shard = 1;
  // data-parallel step: consecutive layers' weight gradients (backward
  // order) share one exchange bucket until it holds at least dp_bucket_mib
  // MiB of fp32 gradient (knob 30; 0 = one bucket per layer)
  int dp_bucket_mib = 8;
  // data-parallel step: from this many padded rows each side-stream dW GEMM
  // is issued as soon as its own dz is complete instead of with its bucket's
  // closing layer (knob 14; 0 = one fork per bucket)
  int dp_fork_rows = 1024;
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
  // blocks of one column, mmad_gemm_body.h) -- no finalize / fold / apply
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
  // the workspace holds the two split-K partial slabs (54.5 MB per stream):
  // the dispatcher could choose a split factor > 1 for one of this handle's
  // GEMMs under the knobs in force at create (4; bf16: 9, 10; fp32: 32).
  // Without the slabs no GEMM of the handle ever splits, with them the
  // dispatcher follows the current knobs; either way the workspace layout
  // depends on (handle, B, k) only
  bool splitk_ws = false;
};

// Move-only owner of one HIP resource (an event, a stream, a pinned
// allocation): null by default, converts to the raw handle, released with D
template <class T, auto D>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Owned& operator=(Owned&& o) noexcept { std::swap(p_, o.p_); return *this; }   // o releases the old one
  ~Owned() { reset(); }
  operator T() const { return p_; }
  T* put() { reset(); return &p_; }   // the out-parameter of a create call
  void reset() { if (p_) (void)D(p_); p_ = nullptr; }
 private:
  T p_ = nullptr;
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// `ev` recorded on `from`, waited for on `to`
inline int hand_off(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  MMAD_HIP_CHECK(hipEventRecord(ev, from));
  MMAD_HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
  return MMAD_OK;
}

// side stream + events for the dW / Adam overlap (created at bind time)
struct SideState {
  Stream stream;
  std::vector<Event> ev_fork, ev_data;
  Event ev_join;
  Event ev_loss;   // fused step: forward done -> the loss reduction on the side stream
  Event ev_hold;   // sched.side_hold: the bwd-data chain is enqueued
  int create(const AeSchedule& sched, size_t n_layers);   // all or nothing (mmad_ae.hip)
};

struct DpState {
  // sharded data-parallel steps (sched.dp_shard): the bf16 model's fp32 master
  // weights / every model's Adam moments are current only on their owning
  // rank since the last mmad_ae_dp_sync_master
  bool master_stale = false;
  // data parallelism: RCCL communicator (not owned), its stream and events
  mmad_comm* comm = nullptr;
  Stream cstream;
  std::vector<Event> ev_dw;
  Event ev_small, ev_cdone;
  // torch-exchange data parallelism (mmad_ae_dw_events): the forward+backward
  // without Adam records ev_xdw[l] after dW_l and ev_xdata[l] after bwd-data of
  // l.  System-scope fences (unlike the executor's own events): the exchange
  // may read the gradients with a copy engine, which does not see the L2
  bool dw_events = false;
  std::vector<Event> ev_xdw, ev_xdata;
  // optional bf16 gradient exchange (mmad_ae_set_grad_bf16): n_weight bf16
  void* grad_bf16 = nullptr;
  // the comm stream and its events / the torch-exchange events: each built in a local, moved in when complete
  int create_comm(const AeSchedule& sched, size_t n_layers) {
    DpState d;
    // highest priority: the exchange must not queue behind the dW GEMMs
    int least = 0, greatest = 0;
    MMAD_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    MMAD_HIP_CHECK(hipStreamCreateWithPriority(d.cstream.put(), hipStreamNonBlocking, greatest));
    // the events RCCL's reads of a bucket wait on keep the system-scope
    // fence (a transport may move the bytes with a copy engine, which does
    // not see the L2); one per bucket and step
    d.ev_dw.resize(n_layers);
    for (Event& e : d.ev_dw) MMAD_HIP_CHECK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(d.ev_small.put(), hipEventDisableTiming));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(d.ev_cdone.put(), sched.ev_flags_));
    cstream = std::move(d.cstream), ev_dw = std::move(d.ev_dw);
    ev_small = std::move(d.ev_small), ev_cdone = std::move(d.ev_cdone);
    return MMAD_OK;
  }
  int create_dw_events(size_t n_layers) {
    std::vector<Event> xdw(n_layers), xdata(n_layers);
    for (Event& e : xdw) MMAD_HIP_CHECK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    for (Event& e : xdata) MMAD_HIP_CHECK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    ev_xdw = std::move(xdw), ev_xdata = std::move(xdata);
    return MMAD_OK;
  }
};

// kernel probe (mmad_ae_probe): timing events around ONE GEMM launch of
// the step, on the stream it is launched on (bench roofline, in situ)
struct Probe {
  int id = -1, n = 0;
  unsigned mask = 0;        // layers the last probed launch covered (bit l)
  std::vector<Event> ev;    // [2 * capacity]: start, end pairs
  Event sync;               // a main-stream probe's start waits for the side stream
  // probe kinds 2 / 3: the events ride on the launch itself (hipExtLaunchKernel
  // start / stop: the kernel's own start and end, as rocprofv3's kernel records)
  // and nothing waits for the side stream -- the launch as it runs in the
  // step's schedule, so the probe can stay on through a timed region
  bool kev = false;
  // One launch on `s`, bracketed if it is the probed one (`hit`) and the probe has room: launch(start, stop)
  // issues it, with the two events to attach to it or nulls.  layers: the mask a bracketed launch leaves.
  // No probe under capture; has_done_ev: the launch carries a hand-off event already
  template <class Launch>
  int bracket(bool hit, unsigned layers, bool capturing, hipStream_t s, hipStream_t side, bool has_done_ev,
              Launch launch) {
    const bool rec = hit && !capturing && 2 * n < (int)ev.size();
    if (rec && !kev && side && s != side && sync) {
      // a probed main-stream launch starts its clock once the side stream's
      // earlier GEMMs are done: its blocks (a whole CU's LDS each on the tail
      // tiles) wait for those CUs anyway, and the event pair then brackets the
      // launch's own execution, first dispatch to completion, as rocprofv3's
      // kernel records do (without it the pair also held ~4 us of that wait on
      // the c2 tail: 31.2 vs 26.8 us, profiles/r08o_prof_c2)
      RET_IF(hand_off(sync, side, s));
    }
    // kernel-attached events only where the launch carries no hand-off event
    const bool attach = rec && kev && !has_done_ev;
    if (rec && !attach) MMAD_HIP_CHECK(hipEventRecord(ev[2 * n], s));
    const int rc = attach ? launch(ev[2 * n], ev[2 * n + 1]) : launch(nullptr, nullptr);
    if (rc != MMAD_OK) return rc;
    if (rec) {
      if (!attach) MMAD_HIP_CHECK(hipEventRecord(ev[2 * n + 1], s));
      ++n;
      mask = layers;
    }
    return MMAD_OK;
  }
};

// hipGraph-captured fused train steps (mmad_ae_train_step_graph): one per
// call signature, replayed after a host->device copy of the per-call values
// (a ring of pinned host slots, each reused only once its copy has run)
struct TrainGraphs {
  GraphCache<TrainKey> graphs{16};
  static constexpr int kDynSlots = 64;
  Owned<MmadDyn*, hipHostFree> dyn_host;
  Event dyn_ev[kDynSlots];
  bool dyn_used[kDynSlots] = {};
  int dyn_next = 0;
  bool broken = false;
  // this call's values -> the next pinned slot -> dev, on st (the ring: made on first use, all or nothing)
  int stage(const MmadDyn& d, MmadDyn* dev, unsigned ev_flags, hipStream_t st);
};

}  // namespace mmad_ae_impl

struct mmad_ae {
  int dtype, n_enc, n_dec, vib, btl;
  float slope, bn_eps, bn_mom;
  std::vector<mmad_ae_impl::AeLayer> L;
  int64_t n_params, n_weight, n_bn;
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *running = nullptr;
  void* shadow = nullptr;
  // bf16 ping-pong: the fused step's Adam writes the new weights into
  // shadow_alt while this step's backward still reads shadow, then the two
  // swap; so a dW GEMM need not wait for its layer's bwd-data GEMM
  void* shadow_alt = nullptr;
  // the schedule (tune-table knobs 14-31, 33-35 and the split-K slab decision),
  // fixed at create
  mmad_ae_impl::AeSchedule sched;
  int mse_tiles = 0;   // loss partials written by the last MSE GEMM
  // ping-pong steps (mmad_ae_set_dw_group): consecutive side-stream layers
  // whose dW + Adam GEMM takes the 64x64 tile are issued as ONE grouped launch
  // (mmad_gemm_dispatch_group) at the lowest member's fork -- at 4096 rows
  // each of the narrow layers' launches is one block's 64-stage K loop,
  // 23-25 us for 16 to 135 blocks, and they ran back to back.  blocks = the
  // group's budget of padded blocks (0 = off: every dW its own launch; < 0 =
  // one resident round of the kernel), members = at most this many per group
  int dw_group_blocks = MMAD_DW_GROUP_BLOCKS_DEFAULT;
  int dw_group_members = MMAD_GEMM_GROUP_MAX;
  // a capture of one of the three caches' passes is open on gstream
  // (capture_graph): no timing probe, no kernel-attached hand-off events
  bool capturing = false;
  // workspace whose split-K control block this handle has zeroed
  const void* ws_zeroed = nullptr;
  mmad_ae_impl::SideState side;
  mmad_ae_impl::DpState dp;
  mmad_ae_impl::Probe probe;
  mmad_ae_impl::Stream gstream;   // capture stream (the caller's may be the null stream)
  // the three graph caches after gstream: destroyed ahead of the stream they were captured on
  mmad_ae_impl::TrainGraphs train;
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
  // hipGraph cache for mmad_ae_score_stream: one captured graph per
  // (input, output, workspace, N, batch) pass, replayed with one launch
  mmad_ae_impl::GraphCache<mmad_ae_impl::ScoreKey> graphs{8};
  // the same for mmad_ae_online_score / _score64: one captured pass per call
  // signature.  online_ready: the state buffer whose NAP operand this handle
  // has zeroed (its padding is never written again); a 64-row state is held
  // as its address + 1 (states are 256-byte aligned), so one buffer carved
  // both ways, or two states taking turns, are zeroed again at each change
  mmad_ae_impl::GraphCache<mmad_ae_impl::OnlineKey> ographs{8};
  const void* online_ready = nullptr;
};

namespace mmad_ae_impl {

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

// where score_batch routes the diffs of a range of diff layers (the attached
// fit's NAP operand, or the streaming NAP fit's own)
struct DiffSink {
  int start, end, K, Kp;   // diff layers [start, end), their width and its padding
  bool x3;                 // bf16 plane operand (the attached fit's x3 NAP GEMM)
  void* x;                 // [Mpe][Kp]
};

inline size_t esz(int dtype) { return dtype == MMAD_BF16 ? 2 : 4; }
// dtype of the eval forward / score GEMMs
inline int score_dt(const mmad_ae* h) { return h->planes ? MMAD_BF16X3 : h->dtype; }
inline int rows_of(const AeWS& w, const AeLayer& a) { return a.enc ? w.B : w.B * w.k; }
inline int prows_of(const AeWS& w, const AeLayer& a) { return a.enc ? w.Mpe : w.Mpd; }
inline float* running_mean(const mmad_ae* h, const AeLayer& a) { return h->running + a.bn_off; }
inline float* running_var(const mmad_ae* h, const AeLayer& a) {
  return h->running + h->n_bn + a.bn_off;
}

// mmad_ae.hip
void carve(const mmad_ae* h, int B, int k, char* base, AeWS& w);
int prepare_ws(mmad_ae* h, int B, int k, void* ws, int64_t ws_bytes, AeWS& w, hipStream_t st);
int refresh_planes(mmad_ae* h, hipStream_t st, bool force = false);
const void* weights(const mmad_ae* h, const AeLayer& a);
const void* weights_dt(const mmad_ae* h, const AeLayer& a, int dt, GemmEpi& ep);
const void* input_of(const mmad_ae* h, const AeWS& w, int l, bool train, const float** scale,
                     const float** shift);
GemmEpi fwd_epi(const mmad_ae* h, const AeWS& w, const AeLayer& a, const LayerWS& s, int M, void* out,
                bool folded);
int ae_gemm(mmad_ae* h, const AeWS& w, int dt, int epi, const void* A, int lda, const void* B,
            int ldb, int Mp, int Np, int K, GemmEpi ep, hipStream_t s, int* cfg = nullptr,
            int probe = -1);
// probe ids: PROBE_FWD + layer (forward / MSE / score GEMM of the layer),
// PROBE_DW + layer (its dW GEMM, with the fused Adam in the fused step)
enum { PROBE_FWD = 0, PROBE_DW = 64 };
// the forward: train with the MSE-fused last layer, eval, or train BN with a plain last layer
enum class FwdMode { TrainMse, Eval, TrainBnPlain };
// mse_done (nullable): an event the train-mode MSE GEMM launch completes itself
int run_forward(mmad_ae* h, AeWS& w, const float* x, int ld_x, FwdMode mode, const float* eps, uint64_t seed,
                uint64_t offset, hipStream_t st, hipEvent_t mse_done = nullptr);
// mmad_ae_score.hip
int diff_col(const mmad_ae* h, int j);

// Capture the launches `pass(stream)` issues into an instantiated graph: on
// the handle's capture stream (created on first use), thread-local mode, with
// h->capturing set for the duration.  The capture is always ended and the
// hipGraph always destroyed.  The caller has run the same pass eagerly first
// (that settles every GEMM tile choice, which cannot be timed under capture).
// Returns which stage failed -- the caller owns the policy -- with the pass's
// own code in rc (GC_PASS) or the HIP error in err (every other stage).
enum GraphCaptureStage { GC_OK = 0, GC_BEGIN, GC_PASS, GC_END, GC_INSTANTIATE };
struct GraphCaptureResult {
  GraphCaptureStage stage;
  int rc;
  hipError_t err;
};
// the capture itself, on *gstream (created on first use); kernel_nodes, if
// given, receives the captured graph's kernel-node count
template <class Pass>
GraphCaptureResult capture_graph_on(Stream* gstream, Pass pass, hipGraphExec_t* exec,
                                    int* kernel_nodes = nullptr) {
  *exec = nullptr;
  hipError_t e = *gstream ? hipSuccess : hipStreamCreateWithFlags(gstream->put(), hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamBeginCapture(*gstream, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return {GC_BEGIN, MMAD_OK, e};
  const int rc = pass(*gstream);
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(*gstream, &graph);
  if (e == hipSuccess && !graph) e = hipErrorUnknown;
  GraphCaptureResult res{GC_OK, rc, e};
  if (rc != MMAD_OK) {
    res.stage = GC_PASS;
  } else if (e != hipSuccess) {
    res.stage = GC_END;
  } else if ((res.err = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
    res.stage = GC_INSTANTIATE;
  }
  if (graph && kernel_nodes && res.stage == GC_OK) {
    size_t nn = 0;
    *kernel_nodes = 0;
    if (hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess && nn) {
      std::vector<hipGraphNode_t> nodes(nn);
      if (hipGraphGetNodes(graph, nodes.data(), &nn) == hipSuccess)
        for (size_t i = 0; i < nn; ++i) {
          hipGraphNodeType t;
          if (hipGraphNodeGetType(nodes[i], &t) == hipSuccess && t == hipGraphNodeTypeKernel) ++*kernel_nodes;
        }
    }
  }
  if (graph) (void)hipGraphDestroy(graph);
  return res;
}
template <class Pass>
GraphCaptureResult capture_graph(mmad_ae* h, Pass pass, hipGraphExec_t* exec) {
  h->capturing = true;
  const GraphCaptureResult res = capture_graph_on(&h->gstream, pass, exec);
  h->capturing = false;
  return res;
}
// the score / online policy: the failed stage's error is the call's (the
// pass's own code and error string first, then the HIP error)
inline int capture_error(const GraphCaptureResult& r) {
  if (r.stage == GC_PASS) return r.rc;
  MMAD_HIP_CHECK(r.err);
  return MMAD_OK;
}
// ... and the one replay routine of the score and online paths: a hit launches
// the cached graph on the caller's stream; a miss runs the pass there eagerly
// (that also settles every GEMM tile choice, which cannot be timed under
// capture), captures the same launches with capture(pass, &exec) -- capture_graph
// or capture_graph_on, on the owner's capture stream -- and keeps the graph for
// the next calls.  Nothing is inserted unless every stage succeeded
template <class Key, class Capture, class Pass>
int replay_or_capture(GraphCache<Key>& cache, const Key& key, hipStream_t st, Capture capture, Pass pass) {
  if (hipGraphExec_t hit = cache.find(key)) {
    MMAD_HIP_CHECK(hipGraphLaunch(hit, st));
    return MMAD_OK;
  }
  RET_IF(pass(st));
  hipGraphExec_t exec = nullptr;
  RET_IF(capture_error(capture(pass, &exec)));
  cache.insert(key, exec);   // bounded cache: drops the oldest pass
  return MMAD_OK;
}

}  // namespace mmad_ae_impl
