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
//
// This file: the handle's lifecycle, the workspace, the forward, Adam, status and the probe.
// The training executor (backward, train steps, data parallel) is mmad_ae_train.hip, the score path
// mmad_ae_score.hip, the 16-row online path mmad_ae_online.hip; mmad_ae_impl.h holds what the four share.
#include "mmad_ae_impl.h"

using namespace mmad_ae_impl;

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

// can the dispatcher choose a split-K factor > 1 for the GEMMs of a handle of
// this dtype under the knobs as they stand?  Asked once per handle, by
// schedule_from_knobs.  (any dtype: a forced override, knob 4; bf16: the dW
// rule, when a dW override or the dW split target is set; fp32: knob 32's dW
// rule, on by default from 2048 rows)
static bool splitk_possible(int dtype) {
  const int o = mmad_splitk_override();
  if (o > 1) return true;
  if (o == 1) return false;
  if (dtype != MMAD_BF16) return mmad_splitk_dw_f32_blocks() > 0;
  return mmad_splitk_dw_override() > 1 || mmad_splitk_dw_blocks() > 0;
}

// The schedule of a new handle, from the tune table as it stands now
// (include/mmad.h knobs 14-31, 33-35; 4 / 9 / 10 / 32 for the split-K slabs).
// The only place in the executor that reads a schedule knob.
static AeSchedule schedule_from_knobs(int dtype) {
  AeSchedule s;
  const int m = mmad_knob(KNOB_BN_MODE);
  s.fold = dtype == MMAD_BF16;
  s.bn_mode = dtype == MMAD_BF16 ? 2 : 0;
  if (m >= 0 && m <= 2) {
    s.bn_mode = m;
    s.fold = m != 0 && dtype == MMAD_BF16;   // fold: mode 1, mode 2's fallback
  }
  s.bn_mode_bwd = mmad_knob(KNOB_BN_MODE_BWD);
  s.bn_fused_rows = mmad_knob(KNOB_BN_FUSED_ROWS);
  s.dw_main = mmad_knob(KNOB_DW_MAIN);
  s.pair_rows = mmad_knob(KNOB_PAIR_ROWS);
  s.dw_main_ping = mmad_knob(KNOB_DW_MAIN_PING);
  s.ev_every = mmad_knob(KNOB_EV_EVERY);
  s.ev_on_kernel = mmad_knob(KNOB_EV_ON_KERNEL);
  s.loss_side = mmad_knob(KNOB_LOSS_SIDE);
  s.dp_small_at = mmad_knob(KNOB_DP_SMALL_AT);
  s.keep_grads = mmad_knob(KNOB_KEEP_GRADS);
  s.side_prio_hi = mmad_knob(KNOB_SIDE_PRIO);
  s.side_cu_held = mmad_knob(KNOB_SIDE_CU_HELD);
  s.dp_shard = mmad_knob(KNOB_DP_SHARD);
  s.side_hold = mmad_knob(KNOB_SIDE_HOLD);
  s.dw_late = mmad_knob(KNOB_DW_LATE);
  s.fork_on_kernel = mmad_knob(KNOB_FORK_ON_KERNEL);
  s.fork_pair_below = mmad_knob(KNOB_FORK_PAIR_BELOW);
  s.dp_bucket_mib = std::max(0, mmad_knob(KNOB_DP_BUCKET_MIB));
  s.dp_fork_rows = mmad_knob(KNOB_DP_FORK_ROWS);
  s.ev_flags_ = ev_flags(mmad_knob(KNOB_EVENT_SYSFENCE));
  s.splitk_ws = splitk_possible(dtype);
  return s;
}

void mmad_ae_impl::carve(const mmad_ae* h, int B, int k, char* base, AeWS& w) {
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
    // the split-K partial slabs (54.5 MB per stream) only for a handle whose
    // schedule holds them (AeSchedule::splitk_ws, fixed at create: every
    // offset below is the same in every call on the handle); without a slab
    // the dispatcher never splits
    size_t slab = 0, ctl = 0;
    if (h->sched.splitk_ws) mmad_gemm_splitk_bytes(0, 0, &slab, &ctl);
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
  h->sched = schedule_from_knobs(dtype);
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

int SideState::create(const AeSchedule& sched, size_t n_layers) {
  SideState s;
  // lowest priority: the side stream fills CUs the critical chain leaves idle
  int least = 0, greatest = 0;
  MMAD_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  // (knob 26: the highest priority instead, for schedule sweeps)
  if (sched.side_cu_held > 0) {
    // schedule study: the side stream's dW + Adam GEMMs kept off side_cu_held
    // CUs so the bwd-data / BN-apply chain always has CUs of its own.  The
    // masked stream is created blocking at the default priority (the API
    // takes neither), so the caller's stream must be a created non-blocking
    // one, not the legacy null stream, or every side launch serialises
    int dev = 0, ncu = 0;
    MMAD_HIP_CHECK(hipGetDevice(&dev));
    MMAD_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const int held = std::min(sched.side_cu_held, ncu - 1), stride = std::max(1, ncu / std::max(1, held));
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int i = 0, n_held = 0; i < ncu; ++i) {
      const bool hold = n_held < held && i % stride == stride - 1;
      n_held += hold;
      if (!hold) mask[i / 32] |= 1u << (i % 32);
    }
    MMAD_HIP_CHECK(hipExtStreamCreateWithCUMask(s.stream.put(), (uint32_t)mask.size(), mask.data()));
  } else {
    MMAD_HIP_CHECK(hipStreamCreateWithPriority(s.stream.put(), hipStreamNonBlocking,
                                               sched.side_prio_hi ? greatest : least));
  }
  s.ev_fork.resize(n_layers);
  s.ev_data.resize(n_layers);
  for (size_t i = 0; i < n_layers; ++i) {
    MMAD_HIP_CHECK(hipEventCreateWithFlags(s.ev_fork[i].put(), sched.ev_flags_));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(s.ev_data[i].put(), sched.ev_flags_));
  }
  for (Event* e : {&s.ev_join, &s.ev_hold, &s.ev_loss})
    MMAD_HIP_CHECK(hipEventCreateWithFlags(e->put(), sched.ev_flags_));
  *this = std::move(s);
  return MMAD_OK;
}

int mmad_ae_bind(mmad_ae* h, float* params, float* grads, float* adam_m, float* adam_v,
                 void* shadow, float* running) {
  MMAD_CHECK_ARG(h && params, "ae_bind: null params");
  MMAD_CHECK_ARG(h->dtype != MMAD_BF16 || shadow, "ae_bind: bf16 needs a shadow buffer");
  if (!h->side.stream) RET_IF(h->side.create(h->sched, h->L.size()));
  h->train.graphs.clear();   // captured steps bake the buffer addresses in
  h->params = params;
  h->grads = grads;
  h->m = adam_m;
  h->v = adam_v;
  h->shadow = shadow;
  h->running = running;
  h->planes_stale = true;
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

// re-split the weight region into the score planes if a weight write may have
// happened since the last split (one launch on the caller's stream)
int mmad_ae_impl::refresh_planes(mmad_ae* h, hipStream_t st, bool force) {
  if (!h->planes || !(h->planes_stale || force)) return MMAD_OK;
  RET_IF(mmad_split_planes(h->n_weight, h->params, h->planes, (char*)h->planes + h->n_weight * 2, st));
  h->planes_stale = false;
  return MMAD_OK;
}

int mmad_ae_sync_shadow(mmad_ae* h, void* stream) {
  MMAD_CHECK_ARG(h && h->params, "ae_sync_shadow: unbound");
  if (h->dtype != MMAD_BF16) return refresh_planes(h, (hipStream_t)stream, true);
  if (h->shadow_alt) RET_IF(mmad_to_bf16(h->n_weight, h->params, h->shadow_alt, stream));
  return mmad_to_bf16(h->n_weight, h->params, h->shadow, stream);
}

// ---------------------------------------------------------------------------
const void* mmad_ae_impl::weights(const mmad_ae* h, const AeLayer& a) {
  if (h->dtype == MMAD_BF16) return (const char*)h->shadow + a.w_off * 2;
  return h->params + a.w_off;
}
// the weight operand of an eval / score GEMM of dtype dt: for MMAD_BF16X3 the
// layer's hi plane, with its lo plane (n_weight elements on) set in ep
const void* mmad_ae_impl::weights_dt(const mmad_ae* h, const AeLayer& a, int dt, GemmEpi& ep) {
  if (dt != MMAD_BF16X3) return weights(h, a);
  ep.b_lo = (const char*)h->planes + (h->n_weight + a.w_off) * 2;
  return (const char*)h->planes + a.w_off * 2;
}

// input of layer l; in train mode a BN producer's output stays pre-BN (a): the
// forward reads it against the folded weights, the dW GEMM fixes up with
// (scale, shift) in its epilogue
const void* mmad_ae_impl::input_of(const mmad_ae* h, const AeWS& w, int l, bool train,
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

int mmad_ae_impl::prepare_ws(mmad_ae* h, int B, int k, void* ws, int64_t ws_bytes, AeWS& w,
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
  // timed-out combine); only on a handle that holds the split-K slabs or
  // fuses BN -- no other handle's kernels read the words
  w.bn_mode = h->sched.bn_mode;
  w.ping = false;
  w.dw_main = h->sched.dw_main;
  if (w.bn_mode == 2 && w.Mpd > h->sched.bn_fused_rows) w.bn_mode = h->sched.fold ? 1 : 0;
  if (w.bn_mode == 1 && !h->sched.fold) w.bn_mode = 0;
  w.bn_mode_bwd = (h->sched.bn_mode_bwd >= 0 && h->sched.fold) ? h->sched.bn_mode_bwd : w.bn_mode;
  if ((h->sched.splitk_ws || h->sched.bn_mode == 2 || h->sched.bn_mode_bwd == 2) &&
      ws != h->ws_zeroed) {
    MMAD_HIP_CHECK(hipMemsetAsync(w.sk_ctl[0], 0, w.sk_ctl_bytes, st));
    h->ws_zeroed = ws;
  }
  return MMAD_OK;
}

// GEMM dispatch with the split-K workspace of the stream it runs on
int mmad_ae_impl::ae_gemm(mmad_ae* h, const AeWS& w, int dt, int epi, const void* A, int lda,
                          const void* B, int ldb, int Mp, int Np, int K, GemmEpi ep, hipStream_t s,
                          int* cfg, int probe) {
  const int r = (h->side.stream && s == h->side.stream) ? 1 : 0;
  ep.sk_slab = w.sk_slab[r];
  ep.sk_ctl = w.sk_ctl[r];
  const bool hit = probe >= 0 && probe == h->probe.id;
  auto launch = [&](hipEvent_t start, hipEvent_t stop) {
    if (stop) ep.start_ev = start, ep.done_ev = stop;
    return mmad_gemm_dispatch(dt, epi, A, lda, B, ldb, Mp, Np, K, ep, s, cfg);
  };
  return h->probe.bracket(hit, hit ? 1u << (probe % 64) : 0u, h->capturing, s, h->side.stream, ep.done_ev, launch);
}

GemmEpi mmad_ae_impl::fwd_epi(const mmad_ae* h, const AeWS& w, const AeLayer& a, const LayerWS& s,
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

int mmad_ae_impl::run_forward(mmad_ae* h, AeWS& w, const float* x, int ld_x, FwdMode mode, const float* eps,
                              uint64_t seed, uint64_t offset, hipStream_t st, hipEvent_t mse_done) {
  const bool eval = mode == FwdMode::Eval, mse = mode == FwdMode::TrainMse;
  const int dt = eval ? score_dt(h) : h->dtype;
  const bool x3 = dt == MMAD_BF16X3;
  const int nL = (int)h->L.size();
  const int B = w.B, k = w.k;
  const bool train = !eval;
  RET_IF(mmad_pack_input_dyn(dt, B, h->L[0].K, w.Mpe, h->L[0].Kp, x, ld_x, w.xin, w.dyn, st));
  for (int l = 0; l < nL; ++l) {
    const AeLayer& a = h->L[l];
    LayerWS& s = w.l[l];
    const int M = rows_of(w, a), Mp = prows_of(w, a);
    const float *isc, *ish;
    const void* in = input_of(h, w, l, train, &isc, &ish);
    const bool folded = isc != nullptr;             // train mode, BN producer
    const void* wt = folded ? s.wf : weights(h, a);
    if (mse && l == nL - 1) {
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
                                      eval ? 1 : 0, w.zbuf, d0.Kp, mse ? w.klpart : nullptr,
                                      mse ? w.dyn : nullptr, st));
    }
  }
  return MMAD_OK;
}

int mmad_ae_adam(mmad_ae* h, float lr, float beta1, float beta2, float eps, int step,
                 void* stream) {
  MMAD_CHECK_ARG(h && h->params && h->grads && h->m && h->v, "ae_adam: unbound handle");
  MMAD_CHECK_ARG(step >= 1, "ae_adam: step must be >= 1");
  h->planes_stale = true;
  const MmadAdamConsts ah = mmad_adam_consts(lr, beta1, beta2, eps, step);
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
  const MmadAdamConsts ah = mmad_adam_consts(lr, beta1, beta2, eps, step);
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
  RET_IF(run_forward(h, w, x, ld_x, train_bn ? FwdMode::TrainBnPlain : FwdMode::Eval, nullptr, 0x5eed, 0, st));
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

int mmad_ae_status(mmad_ae* h, void* ws, int64_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(h, "ae_status: null handle");
  // no split-K GEMM / fused-BN barrier can have run unless the handle's
  // schedule holds the split-K slabs / a fused BN mode
  if ((!h->sched.splitk_ws && h->sched.bn_mode != 2 && h->sched.bn_mode_bwd != 2) || !ws)
    return MMAD_OK;
  AeWS w;
  carve(h, 1, 1, (char*)ws, w);
  MMAD_CHECK_ARG(ws_bytes >= w.bytes, "ae_status: workspace too small");
  for (int r = 0; r < 2; ++r)
    RET_IF(mmad_gemm_read_status(w.sk_ctl[r], (hipStream_t)stream, "ae_status"));
  if ((h->sched.bn_mode == 2 || h->sched.bn_mode_bwd == 2) && w.bn_err) {
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
  Probe& p = h->probe;
  p.ev.clear();
  p.n = 0;
  p.id = -1;
  p.mask = 0;
  p.kev = kind >= 2;
  if (layer < 0 || capacity == 0) return MMAD_OK;
  std::vector<Event> ev(2 * (size_t)capacity);
  for (Event& e : ev) MMAD_HIP_CHECK(hipEventCreate(e.put()));
  if (!p.sync) MMAD_HIP_CHECK(hipEventCreateWithFlags(p.sync.put(), hipEventDisableTiming));
  p.ev = std::move(ev);
  p.id = ((kind & 1) == 0 ? PROBE_FWD : PROBE_DW) + layer;
  return MMAD_OK;
}

int mmad_ae_probe_layers(const mmad_ae* h) { return h ? (int)h->probe.mask : -1; }

int mmad_ae_probe_read(mmad_ae* h, float* ms, int max_n) {
  MMAD_CHECK_ARG(h && ms && max_n >= 0, "ae_probe_read: bad arguments");
  const int n = std::min(h->probe.n, max_n);
  for (int i = 0; i < n; ++i) {
    MMAD_HIP_CHECK(hipEventSynchronize(h->probe.ev[2 * i + 1]));
    MMAD_HIP_CHECK(hipEventElapsedTime(&ms[i], h->probe.ev[2 * i], h->probe.ev[2 * i + 1]));
  }
  return n;
}

int mmad_ae_graph_count(const mmad_ae* h) { return h ? (int)(h->graphs.size() + h->ographs.size()) : -1; }

int mmad_ae_clear_graphs(mmad_ae* h) {
  MMAD_CHECK_ARG(h, "ae_clear_graphs: null handle");
  h->graphs.clear();
  h->ographs.clear();
  h->online_ready = nullptr;   // a new fit: another operand width
  return MMAD_OK;
}
