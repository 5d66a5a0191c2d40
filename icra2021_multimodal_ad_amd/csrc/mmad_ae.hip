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
// This file: the handle's lifecycle, the workspace, the eval forward and the
// training executor.  The score path is mmad_ae_score.hip, the 16-row online
// path mmad_ae_online.hip; mmad_ae_impl.h holds what the three share.
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

int mmad_ae_bind(mmad_ae* h, float* params, float* grads, float* adam_m, float* adam_v,
                 void* shadow, float* running) {
  MMAD_CHECK_ARG(h && params, "ae_bind: null params");
  MMAD_CHECK_ARG(h->dtype != MMAD_BF16 || shadow, "ae_bind: bf16 needs a shadow buffer");
  h->tgraphs.clear();   // captured steps bake the buffer addresses in
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
    if (h->sched.side_cu_held > 0) {
      // schedule study: the side stream's dW + Adam GEMMs kept off side_cu_held
      // CUs so the bwd-data / BN-apply chain always has CUs of its own.  The
      // masked stream is created blocking at the default priority (the API
      // takes neither), so the caller's stream must be a created non-blocking
      // one, not the legacy null stream, or every side launch serialises
      int dev = 0, ncu = 0;
      MMAD_HIP_CHECK(hipGetDevice(&dev));
      MMAD_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
      const int held = std::min(h->sched.side_cu_held, ncu - 1), stride = std::max(1, ncu / std::max(1, held));
      std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
      for (int i = 0, n_held = 0; i < ncu; ++i) {
        const bool hold = n_held < held && i % stride == stride - 1;
        n_held += hold;
        if (!hold) mask[i / 32] |= 1u << (i % 32);
      }
      MMAD_HIP_CHECK(hipExtStreamCreateWithCUMask(&h->side, (uint32_t)mask.size(), mask.data()));
    } else {
      MMAD_HIP_CHECK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking,
                                                 h->sched.side_prio_hi ? greatest : least));
    }
    const size_t n = h->L.size();
    h->ev_fork.resize(n);
    h->ev_data.resize(n);
    for (size_t i = 0; i < n; ++i) {
      MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_fork[i], h->sched.ev_flags_));
      MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_data[i], h->sched.ev_flags_));
    }
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_join, h->sched.ev_flags_));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_hold, h->sched.ev_flags_));
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_loss, h->sched.ev_flags_));
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

// the shadow the fused step's Adam writes (bf16 only)
static void* adam_shadow(const mmad_ae* h, const AeLayer& a, bool ping) {
  if (h->dtype != MMAD_BF16) return nullptr;
  return (char*)(ping && h->shadow_alt ? h->shadow_alt : h->shadow) + a.w_off * 2;
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


int mmad_ae_impl::prepare_ws(const mmad_ae* h, int B, int k, void* ws, int64_t ws_bytes, AeWS& w,
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
    const_cast<mmad_ae*>(h)->ws_zeroed = ws;
  }
  return MMAD_OK;
}

// probe ids: PROBE_FWD + layer (forward / MSE / score GEMM of the layer),
// PROBE_DW + layer (its dW GEMM, with the fused Adam in the fused step)
enum { PROBE_FWD = 0, PROBE_DW = 64 };

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

// GEMM dispatch with the split-K workspace of the stream it runs on
int mmad_ae_impl::ae_gemm(const mmad_ae* h, const AeWS& w, int dt, int epi, const void* A, int lda,
                          const void* B, int ldb, int Mp, int Np, int K, GemmEpi ep, hipStream_t s,
                          int* cfg, int probe) {
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
  const bool each = h->sched.dp_fork_rows > 0 && prows_of(r.w, h->L[l]) >= h->sched.dp_fork_rows && cur && !on_main;
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
  if (h->sched.dp_shard && n % nr == 0 && (n / nr) % 4 == 0) {
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
  if (h->sched.side_hold) return MMAD_OK;   // all of them behind the chain (run_backward)
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
  if (h->sched.side_hold && !r.pending.empty()) {
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
  w.ping = h->shadow_alt && !h->comm && !h->capturing && w.Mpe >= h->sched.pair_rows;
  if (w.ping) w.dw_main = h->sched.dw_main_ping;
  // the side stream's loss reduction waits on the MSE launch's own completion
  const bool loss_ev_on_kernel = !h->comm && h->sched.loss_side && h->sched.ev_on_kernel && !h->capturing;
  RET_IF(run_forward(h, w, x, ld_x, 0, eps, seed, offset, st, loss_ev_on_kernel ? h->ev_loss : nullptr));
  if (!h->comm && !h->sched.loss_side) {
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
    for (auto& e : h->dyn_ev) MMAD_HIP_CHECK(hipEventCreateWithFlags(&e, h->sched.ev_flags_));
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
  const TrainKey key{B, k, ld_x, xvec, eps != nullptr, h->sched.dw_main, h->sched.ev_every, h->sched.keep_grads, ws,
                     h->shadow, beta_kl, beta1, beta2, adam_eps};
  if (hipGraphExec_t hit = h->tgraphs.find(key)) {
    MMAD_HIP_CHECK(hipGraphLaunch(hit, st));
    return MMAD_OK;
  }
  // first call of this signature: run it eagerly (reading the same device
  // slot; this also settles every GEMM tile choice, which cannot be timed
  // under capture), then capture the identical launch sequence
  w.dyn = w.dyn_dev;
  auto pass = [&](hipStream_t s) {
    RET_IF(run_forward(h, w, x, ld_x, 0, eps, seed, offset, s));
    RET_IF(run_backward(h, w, true, beta_kl, &ah, s));
    return finish_reductions(h, w, false, true, beta_kl, loss_out, s);
  };
  RET_IF(pass(st));
  hipGraphExec_t exec = nullptr;
  if (capture_graph(h, pass, &exec).stage != GC_OK) {
    // this step already ran eagerly; later calls stay eager
    h->graph_broken = true;
    (void)hipGetLastError();
    return MMAD_OK;
  }
  h->tgraphs.insert(key, exec);
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
    MMAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_cdone, h->sched.ev_flags_));
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
  h->graphs.clear();
  h->ographs.clear();
  h->online_ready = nullptr;   // a new fit: another operand width
  return MMAD_OK;
}
