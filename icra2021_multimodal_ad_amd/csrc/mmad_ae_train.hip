// Training side of the whole-autoencoder executor: the backward's bwd-data
// chain and its three dW policies, the dW group rule, the eager and graph
// train steps and the data-parallel entry points (forward: mmad_ae.hip).
#include "mmad_ae_impl.h"

using namespace mmad_ae_impl;

// the shadow the fused step's Adam writes (bf16 only)
static void* adam_shadow(const mmad_ae* h, const AeLayer& a, bool ping) {
  if (h->dtype != MMAD_BF16) return nullptr;
  return (char*)(ping && h->shadow_alt ? h->shadow_alt : h->shadow) + a.w_off * 2;
}

// data-parallel weight buckets: walking the layers in backward order,
// consecutive layers join one bucket until it holds >= dp_bucket_mib MiB of
// fp32 gradient (layer 0 always closes the last).  The weights are one
// contiguous buffer in layer order, so a bucket of layers l_lo..l_hi is the
// range [w_off(l_lo), w_off(l_hi) + Np * Kp).  Fewer, larger buckets: fewer
// exchange calls and events on the host (the DP step was host-bound with one
// bucket per layer, profiles/r03z_*) and larger collectives.  The step and
// mmad_ae_dp_sync_master use the same plan; a sharded bucket's rank-r slice is
// [r * n / N, (r + 1) * n / N).
struct DpBucket { int l_hi, l_lo; int64_t off, n; };
static void dp_plan(const mmad_ae* h, std::vector<DpBucket>& out) {
  out.clear();
  const int nL = (int)h->L.size();
  const int64_t min_n = (int64_t)h->sched.dp_bucket_mib * (1 << 20) / 4;
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

// Which side-stream dW + Adam GEMMs share a grouped launch.  Layers l_hi - 1
// down to l_lo are visited in backward order; consecutive layers the tile
// rule (mmad_tile_adam_for) puts on the 64x64 tile, with at most budget / 2
// padded blocks each, join the open group while it stays within `budget`
// padded blocks and `members` members; any other layer, or one that would not
// fit, closes it.  group_of[l] = the group's index (in launch order), or -1
// for a layer with a launch of its own (a group of one is the ordinary launch).
// Returns the number of groups.  A function of its arguments and knob 5 only.
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
static int ae_gemm_group(mmad_ae* h, const AeWS& w, int dt, const PendingDW* q, int n, hipStream_t s) {
  if (n > MMAD_GEMM_GROUP_MAX) return MMAD_GEMM_GROUP_REFUSED;
  const int r = (h->side.stream && s == h->side.stream) ? 1 : 0;
  GemmGroupProblem gp[MMAD_GEMM_GROUP_MAX];
  unsigned mask = 0;
  bool hit = false;
  for (int i = 0; i < n; ++i) {
    gp[i] = GemmGroupProblem{q[i].dz, q[i].in, q[i].lda, q[i].ldb, q[i].M, q[i].N, q[i].K, q[i].ep};
    gp[i].ep.sk_slab = w.sk_slab[r];
    gp[i].ep.sk_ctl = w.sk_ctl[r];
    mask |= 1u << (q[i].layer % 32);
    hit = hit || PROBE_DW + q[i].layer == h->probe.id;
  }
  // (groups exist in the fused policy only, which flushes on the side stream: the bracket's side wait never runs)
  return h->probe.bracket(hit, mask, h->capturing, s, h->side.stream, false, [&](hipEvent_t start, hipEvent_t stop) {
    return mmad_gemm_dispatch_group(dt, n, gp, s, stop, start);
  });
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

// One backward pass: the main-stream bwd-data chain (bwd_data_step), written
// once, and one of three dW policies hooked in before and after each step --
// plain (no Adam), data-parallel (Adam after the bucket's exchange) and fused
// (single GPU, Adam in the dW epilogue).  This is the state they share.
struct BwdRun {
  mmad_ae* h;
  AeWS& w;
  hipStream_t st, side;
  // non-null: the step's Adam update runs in the dW epilogues (fused) or
  // after each bucket's exchange (data parallel, h->dp.comm)
  const MmadAdamConsts* adam;
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

  bool dp() const { return adam && h->dp.comm; }
  bool fused() const { return adam && !h->dp.comm; }
  // the exchange bucket still open (data parallel), and whether layer l closes it
  const DpBucket* open_bucket() const { return next_bucket < plan.size() ? &plan[next_bucket] : nullptr; }
  const DpBucket* closes_bucket(int l) const {
    return open_bucket() && open_bucket()->l_lo == l ? open_bucket() : nullptr;
  }
  // ping-pong shadows (bf16): the fused Adam of dW_l writes the other shadow,
  // so dW_l may start as soon as dz_l is complete
  bool ping(int l) const { return fused() && w.ping && l >= w.dw_main; }
  bool late(int l) const { return ping(l) && l >= nL - h->sched.dw_late; }
  // does layer l's side-stream dW (ping) get a fork event of its own (knob 35)?
  bool fork_ev(int l) const {
    // a group forks once, at its lowest member
    if (grp[l] >= 0) return l == 0 || grp[l - 1] != grp[l];
    const int P = h->sched.fork_pair_below;
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
    return h->sched.ev_every <= 1 || l == w.dw_main || (l - w.dw_main) % h->sched.ev_every == 0;
  }
};

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
    // it only when asked (h->sched.keep_grads)
    e.dw_nostore = h->sched.keep_grads ? 0 : 1;
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
  if (!hop && done_ev && h->sched.ev_on_kernel && !h->capturing) {
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
  RET_IF(hand_off(h->side.ev_fork[l], r.st, r.side));
  RET_IF(launch_dw(r, make_dw(r, l), r.side));
  if (h->dp.dw_events) MMAD_HIP_CHECK(hipEventRecord(h->dp.ev_xdw[l], r.side));
  return MMAD_OK;
}
static int plain_after(BwdRun& r, int l) {
  // torch exchange: W_l is read for the last time by the bwd-data of l
  if (r.h->dp.dw_events && l > 0) MMAD_HIP_CHECK(hipEventRecord(r.h->dp.ev_xdata[l], r.st));
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
  const bool each = h->sched.dp_fork_rows > 0 && prows_of(r.w, h->L[l]) >= h->sched.dp_fork_rows && cur && !on_main;
  // (a bucket whose upper layers were below the row threshold: their dW GEMMs
  // go first, so the bucket's event below covers them too)
  r.pending.push_back(make_dw(r, l));
  if (!each && !bk) return MMAD_OK;
  hipStream_t ds = on_main ? r.st : r.side;
  if (!on_main) RET_IF(hand_off(h->side.ev_fork[l], r.st, r.side));
  RET_IF(flush(r, ds));
  if (bk) MMAD_HIP_CHECK(hipEventRecord(h->dp.ev_dw[l], ds));
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
  const MmadAdamConsts* ad = r.adam;
  RET_IF(finish_reductions(h, r.w, true, true, r.beta_kl, r.dp_loss, r.st));
  RET_IF(hand_off(h->dp.ev_small, r.st, h->dp.cstream));
  const int64_t ns = h->n_params - h->n_weight;
  RET_IF(mmad_allreduce_pair(h->dp.comm, h->grads + h->n_weight, ns, r.dp_loss, 1, h->dp.cstream));
  return mmad_adam_w(ns, h->params + h->n_weight, h->grads + h->n_weight, h->m + h->n_weight,
                     h->v + h->n_weight, ad->w1, ad->w2, ad->eps, ad->step_size, ad->bc2_sqrt, nullptr, 0,
                     h->dp.cstream);
}

// exchange the bucket layer l closes (layers bk.l_hi .. l, one contiguous
// weight range) on the comm stream as soon as its last dW GEMM is complete,
// then its Adam update (which rewrites the bucket's weights, so it also waits
// for the main stream's bwd-data of layer l, the last GEMM of the chain that
// reads them)
static int exchange_bucket(BwdRun& r, const DpBucket& bk, int l) {
  mmad_ae* h = r.h;
  const MmadAdamConsts* ad = r.adam;
  hipStream_t cs = h->dp.cstream;
  const bool bf16 = h->dtype == MMAD_BF16;
  MMAD_HIP_CHECK(hipStreamWaitEvent(cs, h->side.ev_data[l], 0));
  const int nr = mmad_comm_size(h->dp.comm) > 0 ? mmad_comm_size(h->dp.comm) : 1;
  MMAD_HIP_CHECK(hipStreamWaitEvent(cs, h->dp.ev_dw[l], 0));
  const int64_t n = bk.n, boff = bk.off;
  if (h->sched.dp_shard && n % nr == 0 && (n / nr) % 4 == 0) {
    // ZeRO-1 form: reduce-scatter, Adam on this rank's shard, all-gather
    // of the updated weights the next step reads (bf16 shadow / fp32 p)
    const int64_t cnt = n / nr, off = boff + (int64_t)mmad_comm_rank(h->dp.comm) * cnt;
    if (h->dp.grad_bf16) {
      // bf16 on the wire: round the bucket, reduce-scatter, widen this rank's slice
      char* gb = (char*)h->dp.grad_bf16;
      RET_IF(mmad_to_bf16(n, h->grads + boff, gb + boff * 2, cs));
      RET_IF(mmad_reduce_scatter_bucket_bf16(h->dp.comm, gb + boff * 2, n, cs));
      RET_IF(mmad_from_bf16(cnt, gb + off * 2, h->grads + off, cs));
    } else {
      RET_IF(mmad_reduce_scatter_bucket(h->dp.comm, h->grads + boff, n, cs));
    }
    void* sh = bf16 ? (void*)((char*)h->shadow + off * 2) : nullptr;
    RET_IF(mmad_adam_w(cnt, h->params + off, h->grads + off, h->m + off, h->v + off, ad->w1, ad->w2,
                       ad->eps, ad->step_size, ad->bc2_sqrt, sh, bf16 ? cnt : 0, cs));
    if (bf16)
      RET_IF(mmad_all_gather_bucket(h->dp.comm, (char*)h->shadow + boff * 2, n, MMAD_BF16, cs));
    else
      RET_IF(mmad_all_gather_bucket(h->dp.comm, h->params + boff, n, MMAD_F32, cs));
    if (nr > 1) h->dp.master_stale = true;
  } else {
    RET_IF(mmad_allreduce_bucket(h->dp.comm, h->grads + boff, n, cs));
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
  if (!r.w.ping || h->capturing || h->sched.side_hold || h->dw_group_blocks == 0) return;
  std::vector<int> np(r.nL), kp(r.nL), rows(r.nL);
  for (int l = 0; l < r.nL; ++l) {
    np[l] = h->L[l].Np;
    kp[l] = h->L[l].Kp;
    rows[l] = prows_of(r.w, h->L[l]);
  }
  const int budget = h->dw_group_blocks < 0 ? mmad_gemm_group_capacity(h->dtype) : h->dw_group_blocks;
  mmad_dw_group_plan(r.nL, np.data(), kp.data(), rows.data(), r.w.dw_main, r.nL - h->sched.dw_late, budget,
                     h->dw_group_members, r.grp.data());
}
static int fused_before(BwdRun& r, int l) {
  // dz_l is complete: the fork of a ping-pong dW that the producing launch
  // did not carry
  if (r.forks_at_dz(l) && !r.fork_none(l) && !r.fork_done[l])
    MMAD_HIP_CHECK(hipEventRecord(r.h->side.ev_fork[l], r.st));
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
  if (h->sched.side_hold) return MMAD_OK;   // all of them behind the chain (run_backward)
  if (r.ping(l)) {
    // no fork of its own: issued with the next lower layer's dW
    if (!r.late(l) && !r.fork_ev(l)) return MMAD_OK;
    if (r.late(l))
      RET_IF(hand_off(h->side.ev_fork[l], r.st, r.side));
    else if (!r.fork_none(l))
      MMAD_HIP_CHECK(hipStreamWaitEvent(r.side, h->side.ev_fork[l], 0));
  } else {
    if (!r.needs_data_ev(l)) return MMAD_OK;
    MMAD_HIP_CHECK(hipStreamWaitEvent(r.side, h->side.ev_data[l], 0));
  }
  return flush(r, r.side);
}

// backward through every layer: the chain on `st`, the dW GEMMs where the
// policy puts them, the side stream joined back into `st` at the end
static int run_backward(mmad_ae* h, AeWS& w, bool from_mse, float beta_kl, const MmadAdamConsts* adam,
                        hipStream_t st, float* dp_loss = nullptr, bool side_after_mse = false) {
  const int nL = (int)h->L.size();
  BwdRun r{h, w, st, h->side.stream, adam, from_mse, side_after_mse, beta_kl, dp_loss, nL,
           h->sched.fork_on_kernel && !h->capturing};
  r.fork_done.assign(nL, 0);
  r.grp.assign(nL, -1);
  if (r.dp()) dp_plan(h, r.plan);
  if (r.fused()) fused_plan_groups(r);
  const int small_at = nL > h->sched.dp_small_at ? h->sched.dp_small_at : 0;
  for (int l = nL - 1; l >= 0; --l) {
    // DP and plain issue dW_l before the bwd-data of l, fused after it
    RET_IF(!adam ? plain_before(r, l) : r.dp() ? dp_before(r, l) : fused_before(r, l));
    const bool need = r.needs_data_ev(l);
    // dz_{l-1} is produced by this step: its side-stream dW fork rides on that launch
    const bool fork_below = l > 0 && r.fork_kev && r.forks_at_dz(l - 1);
    ChainPlaced placed;
    RET_IF(bwd_data_step(r, l, need ? h->side.ev_data[l] : nullptr, fork_below ? h->side.ev_fork[l - 1] : nullptr,
                         &placed));
    if (placed.fork) r.fork_done[l - 1] = 1;
    if (!adam) RET_IF(plain_after(r, l));
    if (r.dp() && dp_loss && l == small_at) RET_IF(dp_small_bucket(r));
    // ev_data[l] that the chain step could neither attach nor place ahead of a BN apply
    if (need && !placed.done) MMAD_HIP_CHECK(hipEventRecord(h->side.ev_data[l], st));
    if (r.fused()) RET_IF(fused_after(r, l));
    if (const DpBucket* bk = r.closes_bucket(l)) RET_IF(exchange_bucket(r, *bk, l));
  }
  if (h->sched.side_hold && !r.pending.empty()) {
    RET_IF(hand_off(h->side.ev_hold, st, r.side));
    RET_IF(flush(r, r.side));
  }
  MMAD_CHECK_ARG(r.pending.empty(), "ae backward: deferred dW GEMMs left unissued");
  // join the side stream back into the main stream
  return hand_off(h->side.ev_join, r.side, st);
}

int mmad_ae_train_fwd_bwd(mmad_ae* h, const float* x, int ld_x, int B, int k, const float* eps,
                          uint64_t seed, uint64_t offset, float beta_kl, float* loss_out,
                          void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->running, "ae_train: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && loss_out, "ae_train: bad input");
  AeWS w;
  RET_IF(prepare_ws(h, B, k, ws, ws_bytes, w, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  RET_IF(run_forward(h, w, x, ld_x, FwdMode::TrainMse, eps, seed, offset, st));
  RET_IF(run_backward(h, w, true, beta_kl, nullptr, st));
  return finish_reductions(h, w, true, true, beta_kl, loss_out, st);
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
  const MmadAdamConsts ah = mmad_adam_consts(lr, beta1, beta2, adam_eps, step);
  // ping-pong schedule (bf16 with a shadow pair, large calls, single process)
  w.ping = h->shadow_alt && !h->dp.comm && !h->capturing && w.Mpe >= h->sched.pair_rows;
  if (w.ping) w.dw_main = h->sched.dw_main_ping;
  // the side stream's loss reduction waits on the MSE launch's own completion
  const bool loss_ev_on_kernel = !h->dp.comm && h->sched.loss_side && h->sched.ev_on_kernel && !h->capturing;
  RET_IF(run_forward(h, w, x, ld_x, FwdMode::TrainMse, eps, seed, offset, st, loss_ev_on_kernel ? h->side.ev_loss : nullptr));
  if (!h->dp.comm) {
    if (h->sched.loss_side) {
      // the loss needs only the forward's MSE (and KL) partials: reduce it on
      // the side stream now, off the main stream's tail (the backward joins the
      // side stream back into the caller's before the step ends)
      if (!loss_ev_on_kernel) MMAD_HIP_CHECK(hipEventRecord(h->side.ev_loss, st));
      MMAD_HIP_CHECK(hipStreamWaitEvent(h->side.stream, h->side.ev_loss, 0));
      RET_IF(finish_reductions(h, w, false, true, beta_kl, loss_out, h->side.stream));
    }
    RET_IF(run_backward(h, w, true, beta_kl, &ah, st, nullptr, h->sched.loss_side != 0));
    if (!h->sched.loss_side) RET_IF(finish_reductions(h, w, false, true, beta_kl, loss_out, st));
    if (w.ping) std::swap(h->shadow, h->shadow_alt);
    return MMAD_OK;
  }
  // data parallel: per-layer weight buckets and (ahead of layer 0's) the
  // small bucket [all bias | gamma | beta grads] + the loss, each with its
  // Adam, on the comm stream (run_backward); then join
  RET_IF(run_backward(h, w, true, beta_kl, &ah, st, loss_out));
  return hand_off(h->dp.ev_cdone, h->dp.cstream, st);
}

int TrainGraphs::stage(const MmadDyn& d, MmadDyn* dev, unsigned ev_flags, hipStream_t st) {
  if (!dyn_host) {
    TrainGraphs t;
    MMAD_HIP_CHECK(hipHostMalloc((void**)t.dyn_host.put(), sizeof(MmadDyn) * kDynSlots, hipHostMallocDefault));
    for (Event& e : t.dyn_ev) MMAD_HIP_CHECK(hipEventCreateWithFlags(e.put(), ev_flags));
    dyn_host = std::move(t.dyn_host);
    std::move(t.dyn_ev, t.dyn_ev + kDynSlots, dyn_ev);
  }
  const int slot = dyn_next;
  dyn_next = (slot + 1) % kDynSlots;
  if (dyn_used[slot]) MMAD_HIP_CHECK(hipEventSynchronize(dyn_ev[slot]));
  dyn_host[slot] = d;
  MMAD_HIP_CHECK(hipMemcpyAsync(dev, &dyn_host[slot], sizeof(MmadDyn), hipMemcpyHostToDevice, st));
  MMAD_HIP_CHECK(hipEventRecord(dyn_ev[slot], st));
  dyn_used[slot] = true;
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
  if (h->dp.comm || h->train.broken)   // eager schedule for these
    return mmad_ae_train_step(h, x, ld_x, B, k, eps, seed, offset, beta_kl, lr, beta1, beta2,
                              adam_eps, step, loss_out, ws, ws_bytes, stream);
  AeWS w;
  hipStream_t st = (hipStream_t)stream;
  RET_IF(prepare_ws(h, B, k, ws, ws_bytes, w, st));
  const MmadAdamConsts ah = mmad_adam_consts(lr, beta1, beta2, adam_eps, step);
  const MmadDyn d{x, loss_out, eps, seed, offset, ah.step_size, ah.bc2_sqrt};
  RET_IF(h->train.stage(d, w.dyn_dev, h->sched.ev_flags_, st));
  const int xvec = ((uintptr_t)x % 16 == 0 && ld_x % 4 == 0) ? 1 : 0;
  const TrainKey key{B, k, ld_x, xvec, eps != nullptr, h->sched.dw_main, h->sched.ev_every, h->sched.keep_grads, ws,
                     h->shadow, beta_kl, beta1, beta2, adam_eps};
  if (hipGraphExec_t hit = h->train.graphs.find(key)) {
    MMAD_HIP_CHECK(hipGraphLaunch(hit, st));
    return MMAD_OK;
  }
  // first call of this signature: run it eagerly (reading the same device
  // slot; this also settles every GEMM tile choice, which cannot be timed
  // under capture), then capture the identical launch sequence
  w.dyn = w.dyn_dev;
  auto pass = [&](hipStream_t s) {
    RET_IF(run_forward(h, w, x, ld_x, FwdMode::TrainMse, eps, seed, offset, s));
    RET_IF(run_backward(h, w, true, beta_kl, &ah, s));
    return finish_reductions(h, w, false, true, beta_kl, loss_out, s);
  };
  RET_IF(pass(st));
  hipGraphExec_t exec = nullptr;
  if (capture_graph(h, pass, &exec).stage != GC_OK) {
    // this step already ran eagerly; later calls stay eager
    h->train.broken = true;
    (void)hipGetLastError();
    return MMAD_OK;
  }
  h->train.graphs.insert(key, exec);
  return MMAD_OK;
}

int mmad_ae_train_graph_count(const mmad_ae* h) { return h ? (int)h->train.graphs.size() : -1; }

int mmad_ae_set_comm(mmad_ae* h, mmad_comm* c) {
  MMAD_CHECK_ARG(h, "ae_set_comm: null handle");
  MMAD_CHECK_ARG(h->side.stream, "ae_set_comm: bind the handle first");
  MMAD_CHECK_ARG(c == h->dp.comm || !h->dp.master_stale,
                 "ae_set_comm: the master weights are sharded over the ranks of the attached "
                 "communicator: mmad_ae_dp_sync_master on every rank first");
  if (c && !h->dp.cstream) RET_IF(h->dp.create_comm(h->sched, h->L.size()));
  h->dp.comm = c;
  return MMAD_OK;
}

int mmad_ae_dp_master_stale(const mmad_ae* h) { return h && h->dp.master_stale ? 1 : 0; }

int mmad_ae_set_grad_bf16(mmad_ae* h, void* buf) {
  MMAD_CHECK_ARG(h && h->params, "ae_set_grad_bf16: unbound handle");
  MMAD_CHECK_ARG(!buf || ((uintptr_t)buf % 16 == 0), "ae_set_grad_bf16: buffer must be 16-byte aligned");
  h->dp.grad_bf16 = buf;
  return MMAD_OK;
}

int mmad_ae_dw_events(mmad_ae* h, int on) {
  MMAD_CHECK_ARG(h && h->side.stream, "ae_dw_events: bind the handle first");
  if (on && h->dp.ev_xdw.empty()) RET_IF(h->dp.create_dw_events(h->L.size()));
  h->dp.dw_events = on != 0;
  return MMAD_OK;
}

int mmad_ae_wait_dw(mmad_ae* h, int layer, void* stream) {
  MMAD_CHECK_ARG(h && h->dp.dw_events, "ae_wait_dw: dW events are off (mmad_ae_dw_events)");
  MMAD_CHECK_ARG(layer >= 0 && layer < (int)h->L.size(), "ae_wait_dw: bad layer %d", layer);
  MMAD_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->dp.ev_xdw[layer], 0));
  if (layer > 0) MMAD_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->dp.ev_xdata[layer], 0));
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
  if (!h->dp.comm || !h->dp.master_stale) return MMAD_OK;
  hipStream_t st = (hipStream_t)stream;
  const int nr = mmad_comm_size(h->dp.comm);
  std::vector<DpBucket> plan;
  dp_plan(h, plan);
  for (const DpBucket& b : plan) {
    const int64_t n = b.n, boff = b.off;
    if (!(n % nr == 0 && (n / nr) % 4 == 0)) continue;   // an all-reduced bucket: already current
    if (h->dtype == MMAD_BF16) RET_IF(mmad_all_gather_bucket(h->dp.comm, h->params + boff, n, MMAD_F32, st));
    RET_IF(mmad_all_gather_bucket(h->dp.comm, h->m + boff, n, MMAD_F32, st));
    RET_IF(mmad_all_gather_bucket(h->dp.comm, h->v + boff, n, MMAD_F32, st));
  }
  h->dp.master_stale = false;
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

int mmad_ae_set_dw_group(mmad_ae* h, int blocks, int members) {
  MMAD_CHECK_ARG(h, "ae_set_dw_group: null handle");
  if (blocks >= -1) h->dw_group_blocks = blocks;
  if (members > 0) h->dw_group_members = members;
  return MMAD_OK;
}
