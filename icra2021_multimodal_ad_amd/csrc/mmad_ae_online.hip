// ---- online scoring: B <= 16 windows through the 16-row weight stream, or
// B <= 64 through the 64-row one (mmad_skinny.hip).  The batch path
// (mmad_ae_score.hip) pads such a call to 128 rows and spends its ~30 launches
// on zeros; here every layer is one launch that reads its weights once.  All
// buffers live in a caller-owned state, carved below for `rows` = 16 or 64.
// Every entry point -- the scorer's three, the sensor tick, the bank and its
// tick -- checks its members into OnlineMember records (member_check), and one
// function (online_walk) issues their launch list, eagerly or into the capture
// that replay_or_capture (mmad_ae_impl.h) replays from then on.
#include "mmad_ae_impl.h"

using namespace mmad_ae_impl;

struct OnlineWS {
  void* xin = nullptr;             // packed input [rows][Kp0]
  std::vector<void*> y, p2;        // pass-1 outputs per layer; pass-2 outputs per encoder layer
  void* zbuf = nullptr;            // VIB: z [128][Kp] as mmad_vib_reparam_fwd writes it
  float *scale = nullptr, *shift = nullptr;   // folded eval-BN constants [n_bn]
  std::vector<float*> rs;          // row partials per diff layer [Np/16][rows]
  float* nap_x = nullptr;          // packed NAP operand [rows][nap.Kp] (fp32)
  float* nap_rs = nullptr;         // the NAP launch's row partials [Rp/16][rows]
  int64_t bytes = 0;
};

static void online_carve(const mmad_ae* h, char* base, OnlineWS& o, int rows) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) -> char* {
    off = (off + 255) / 256 * 256;
    char* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  };
  const int64_t E = (int64_t)esz(h->dtype), R = rows;
  const int nL = (int)h->L.size();
  o.xin = take(R * h->L[0].Kp * E);
  o.y.resize(nL);
  for (int l = 0; l < nL; ++l) o.y[l] = take(R * h->L[l].Np * E);
  if (h->vib) o.zbuf = take((int64_t)MMAD_PAD * h->L[h->n_enc].Kp * E);
  o.p2.resize(h->n_enc);
  for (int e = 0; e < h->n_enc; ++e) o.p2[e] = take(R * h->L[e].Np * E);
  o.scale = (float*)take(std::max<int64_t>(h->n_bn, 1) * 4);
  o.shift = (float*)take(std::max<int64_t>(h->n_bn, 1) * 4);
  o.rs.resize(h->n_enc + 1);
  o.rs[0] = (float*)take(h->L[nL - 1].Np / 16 * R * 4);   // [Np/16][rows]
  for (int e = 0; e < h->n_enc; ++e) o.rs[e + 1] = (float*)take(h->L[e].Np / 16 * R * 4);
  if (h->nap.on) {
    o.nap_x = (float*)take(R * h->nap.Kp * 4);
    o.nap_rs = (float*)take(h->nap.Rp / 16 * R * 4);
  }
  o.bytes = (off + 255) / 256 * 256;
}

static int64_t online_state_bytes(const mmad_ae* h, int rows) {
  if (!h) return -1;
  OnlineWS o;
  online_carve(h, nullptr, o, rows);
  return o.bytes;
}

int64_t mmad_ae_online_state_bytes(const mmad_ae* h) { return online_state_bytes(h, 16); }
int64_t mmad_ae_online_state_bytes64(const mmad_ae* h) { return online_state_bytes(h, 64); }

int64_t mmad_ae_online_groups_bytes(const mmad_ae* h, int rows) {
  if (!h || (rows != 16 && rows != 64)) return -1;
  return ((int64_t)rows * h->L[0].Kp * 4 + 255) / 256 * 256;
}

// the launch list of one member's pass, step by step.  list / len: the
// weight-stream launches of pass 1 (every layer), of pass 2 (the encoder
// again) and the NAP run (one launch, with a fit attached)
enum { PASS1, PASS2, NAP_RUN, N_LISTS };
struct OnlinePlan {
  MmadPackMember pack;
  MmadOnlineFold fold;
  MmadSkinny list[N_LISTS][MMAD_ONLINE_MAX_LAYERS];
  int len[N_LISTS];
  MmadGroupSq gsq;   // a grouped member's (key.G > 0)
  MmadOnlineFinish fin;
};

// one checked member of a call: a scorer call or a tick has one, a bank call
// one per handle.  key: the member's graph signature, which is also the record
// of its arguments -- x, ld_x, B, rows, the outputs, the clamped SAP range
// and, for a grouped member (G > 0), the bounds and the groups' buffers
// (gstate: where d0 goes).  plan: filled by online_walk, not by the check
struct OnlineMember {
  mmad_ae* h;
  OnlineWS o;   // the carved state
  OnlineKey key;
  OnlinePlan plan;
};

// every refusal of the entry points for one member, nothing launched.  a: the
// member's arguments as mmad_bank_member and mmad_tick_args both name them;
// rows = 16 (mmad_ae_online_score) or 64 (_score64); grouped: the grouped
// form's own refusals (rows, G, bounds) come first
template <class Args>
static int member_check(mmad_ae* h, const float* x, int ld_x, int B, int rows, const Args& a, bool grouped,
                        OnlineMember& m) {
  OnlineKey& k = m.key;
  k = OnlineKey{};
  if (grouped) {
    MMAD_CHECK_ARG(rows == 16 || rows == 64, "ae_online_score_groups: rows=%d (16 or 64)", rows);
    MMAD_CHECK_ARG(a.G >= 1 && a.G <= MMAD_MAX_GROUPS, "ae_online_score_groups: G=%d outside 1..%d", a.G,
                   MMAD_MAX_GROUPS);
    MMAD_CHECK_ARG(a.bounds && a.bounds[0] >= 0, "ae_online_score_groups: bounds null or bounds[0] negative");
    k.G = a.G;
    for (int g = 0; g <= k.G; ++g) k.bounds[g] = a.bounds[g];
    for (int g = 0; g < k.G; ++g)
      MMAD_CHECK_ARG(k.bounds[g] < k.bounds[g + 1], "ae_online_score_groups: bounds not strictly ascending "
                     "(bounds[%d]=%d, bounds[%d]=%d)", g, k.bounds[g], g + 1, k.bounds[g + 1]);
    k.gthr = a.group_thresholds; k.gout = a.group_out; k.gflags = a.group_flags;
  }
  MMAD_CHECK_ARG(h, "ae_online_score: null handle");
  if (grouped) {
    MMAD_CHECK_ARG(k.bounds[k.G] <= h->L[0].K, "ae_online_score_groups: bounds[G]=%d exceeds the "
                   "input width D=%d", k.bounds[k.G], h->L[0].K);
    MMAD_CHECK_ARG(k.gout, "ae_online_score_groups: null group_out");
    const int64_t gneed = mmad_ae_online_groups_bytes(h, rows);
    MMAD_CHECK_ARG(a.gstate && a.gstate_bytes >= gneed, "ae_online_score_groups: gstate null or too small "
                   "(%lld < %lld bytes, mmad_ae_online_groups_bytes)",
                   (long long)(a.gstate ? a.gstate_bytes : 0), (long long)gneed);
    MMAD_CHECK_ARG(((uintptr_t)a.gstate) % 256 == 0, "ae_online_score_groups: gstate must be 256-byte aligned");
    k.gstate = a.gstate;
  }
  const char* sfx = rows == 16 ? "" : "64";
  MMAD_CHECK_ARG(B >= 1 && B <= rows, "ae_online_score%s: B=%d outside 1..%d (the batch path, "
                 "mmad_ae_score_stream, serves larger calls)", sfx, B, rows);
  const int64_t need = online_state_bytes(h, rows);
  MMAD_CHECK_ARG(a.state && a.state_bytes >= need, "ae_online_score: online state null or too small "
                 "(%lld < %lld bytes, mmad_ae_online_state_bytes%s)", (long long)(a.state ? a.state_bytes : 0),
                 (long long)need, sfx);
  MMAD_CHECK_ARG(((uintptr_t)a.state) % 256 == 0, "ae_online_score: state must be 256-byte aligned");
  MMAD_CHECK_ARG(h->params && h->running, "ae_online_score: unbound handle");
  MMAD_CHECK_ARG(x && ld_x >= h->L[0].K && a.out, "ae_online_score: bad args (null x / out, ld_x=%d)", ld_x);
  MMAD_CHECK_ARG(score_dt(h) != MMAD_BF16X3, "ae_online_score: score planes attached "
                 "(MMAD_BF16X3): split-bf16 planes are not supported on the online path");
  MMAD_CHECK_ARG(!h->nap.on || h->nap.dtype == MMAD_F32, "ae_online_score: the attached fit's NAP "
                 "GEMM is MMAD_BF16X3: not supported on the online path (attach an MMAD_F32 fit)");
  const int nd = h->n_enc + 1;
  MMAD_CHECK_ARG(nd <= MMAD_ONLINE_MAX_DIFF && (int)h->L.size() <= MMAD_ONLINE_MAX_LAYERS,
                 "ae_online_score: too many layers");
  // the reference's clamping (utils/metric.py:155-171)
  int s0 = a.sap_start < 0 ? 0 : a.sap_start, s1 = a.sap_end;
  if (s0 > nd - 1) s0 = nd - 1;
  if (s1 - s0 < 1) s1 = s0 + 1;
  if (s1 > nd) s1 = nd;
  m.h = h;
  online_carve(h, (char*)a.state, m.o, rows);
  k.x = x; k.ld_x = ld_x; k.B = B; k.sap_start = s0; k.sap_end = s1;
  k.thr = a.thresholds; k.out = a.out; k.flags = a.flags; k.state = a.state;
  k.wts = weights(h, h->L[0]);
  k.nap_vt = h->nap.on ? (const void*)h->nap.vt : nullptr;
  k.rows = rows;
  return MMAD_OK;
}

// a checked member's launch list; a grouped member is one more launch, nothing
// else moves
static void online_plan(OnlineMember& m) {
  mmad_ae* h = m.h;
  const OnlineWS& o = m.o;
  const OnlineKey& k = m.key;
  OnlinePlan& p = m.plan;
  const int dt = h->dtype, rows = k.rows, B = k.B;
  const int nL = (int)h->L.size();
  const mmad_ae::NapFit& nf = h->nap;
  p.pack = MmadPackMember{dt, h->L[0].K, h->L[0].Kp, k.x, o.xin};
  MmadOnlineFold& f = p.fold;
  f = MmadOnlineFold{};
  f.n_bn = (int)h->n_bn;
  for (const AeLayer& a : h->L)
    if (a.bn) {
      f.bn_off[f.n] = (int)a.bn_off; f.N[f.n] = a.N; f.g_off[f.n] = a.g_off; f.be_off[f.n] = a.be_off;
      ++f.n;
    }
  // diff layer j's diffs into the NAP operand (columns relative to the range's first)
  auto route = [&](MmadSkinny& a, int j) {
    if (!nf.on || j < nf.start || j >= nf.end) return;
    a.diff = o.nap_x + (diff_col(h, j) - diff_col(h, nf.start));
    a.lddiff = nf.Kp;
  };
  auto layer = [&](const AeLayer& L, const void* in, void* y) {
    MmadSkinny a{};
    a.rows = rows; a.M = B; a.N = L.N; a.Np = L.Np; a.Kp = L.Kp;
    a.x = in; a.w = weights(h, L); a.bias = h->params + L.b_off; a.act = L.act; a.slope = h->slope;
    if (L.bn) { a.scale = o.scale + L.bn_off; a.shift = o.shift + L.bn_off; }
    a.y = y;
    return a;
  };
  const bool grouped = k.G > 0;
  const float* d0 = nullptr;   // grouped member: where the last decoder launch leaves d0
  int ldd0 = 0;
  // pass 1: eval forward; the decoder's last layer scores d0 = x_hat - x
  p.len[PASS1] = nL;
  for (int l = 0; l < nL; ++l) {
    const AeLayer& L = h->L[l];
    const void* in = l == 0 ? o.xin : (h->vib && l == h->n_enc ? o.zbuf : o.y[l - 1]);
    MmadSkinny& a = p.list[PASS1][l] = layer(L, in, o.y[l]);
    if (l == nL - 1) {
      a.ref = o.xin; a.ref_f32 = 0; a.ldref = h->L[0].Kp;
      a.rowsq = o.rs[0];
      route(a, 0);
      if (grouped) {
        // d0 where the pass stores it already (the fit's operand), else into
        // the groups buffer: the kernel and rowsq are the ungrouped pass's
        if (!a.diff) { a.diff = (float*)k.gstate; a.lddiff = h->L[0].Kp; }
        d0 = a.diff; ldd0 = a.lddiff;
      }
    }
  }
  if (grouped) {
    // all `rows` rows: rows >= B hold d = 0, so score 0 (and flag 0: n_flag)
    MmadGroupSq& q = p.gsq;
    q = MmadGroupSq{};
    q.d = d0; q.ldd = ldd0; q.N = rows; q.n_flag = B; q.G = k.G;
    for (int g = 0; g <= k.G; ++g) q.bounds[g] = k.bounds[g];
    q.thr = k.gthr; q.out = k.gout; q.ldo = rows; q.flags = k.gflags; q.ldf = rows;
  }
  // pass 2: x_hat through the encoder, each layer against its pass-1 output
  p.len[PASS2] = h->n_enc;
  const void* cur = o.y[nL - 1];
  for (int e = 0; e < h->n_enc; ++e) {
    const AeLayer& L = h->L[e];
    MmadSkinny& a = p.list[PASS2][e] = layer(L, cur, o.p2[e]);
    a.ref = o.y[e]; a.ref_f32 = 0; a.ldref = L.Np;
    a.rowsq = o.rs[e + 1];
    route(a, e + 1);
    cur = o.p2[e];
  }
  // the NAP run: the same kernel on the fit's fp32 V^T (K = W, N = R), bias
  // after the product, colw = 1 / var, no reference
  p.len[NAP_RUN] = nf.on;
  if (nf.on) {
    MmadSkinny& a = p.list[NAP_RUN][0] = MmadSkinny{};
    a.rows = rows; a.M = B; a.N = nf.R; a.Np = nf.Rp; a.Kp = nf.Kp;
    a.x = o.nap_x; a.w = nf.vt; a.bias = nf.bias; a.act = MMAD_ACT_NONE;
    a.colw = nf.w; a.rowsq = o.nap_rs;
  }
  MmadOnlineFinish& fin = p.fin;
  fin = MmadOnlineFinish{};
  fin.B = B; fin.n_diff = h->n_enc + 1;
  fin.rs[0] = o.rs[0]; fin.tiles[0] = h->L[nL - 1].Np / 16; fin.widths[0] = h->L[0].K;
  for (int e = 0; e < h->n_enc; ++e) {
    fin.rs[e + 1] = o.rs[e + 1]; fin.tiles[e + 1] = h->L[e].Np / 16; fin.widths[e + 1] = h->L[e].N;
  }
  fin.sap_start = k.sap_start; fin.sap_end = k.sap_end;
  if (nf.on) { fin.nap_rs = o.nap_rs; fin.nap_tiles = nf.Rp / 16; fin.nap_scale = 1.f / (float)nf.R; }
  fin.out = k.out; fin.flags = k.flags; fin.thresholds = k.thr;
}

// the BN fold of the walk's members: the single launcher, or the bank's
static int fold_step(const OnlineMember* m, int n, bool bank, hipStream_t st) {
  if (!bank)
    return mmad_online_fold(m->plan.fold, m->h->params, m->h->running, m->h->bn_eps, m->o.scale, m->o.shift, st);
  MmadOnlineFoldGroup fg{};
  fg.n = n;
  for (int i = 0; i < n; ++i) {
    const MmadOnlineFold& f = m[i].plan.fold;
    const mmad_ae* h = m[i].h;
    int e = fg.first[i];
    for (int l = 0; l < f.n; ++l, ++e) {
      fg.bn_off[e] = f.bn_off[l]; fg.N[e] = f.N[l]; fg.g_off[e] = f.g_off[l]; fg.be_off[e] = f.be_off[l];
    }
    fg.first[i + 1] = e;
    fg.m[i] = MmadOnlineFoldMember{h->params, h->running, m[i].o.scale, m[i].o.shift, h->bn_eps, f.n_bn};
  }
  return mmad_online_fold_group(fg, st);
}

// step s of one of the plans' lists, over the members that reach it (N = 0: none here)
static int layer_step(const OnlineMember* m, int n, bool bank, int list, int s, hipStream_t st) {
  MmadSkinny a[MMAD_MAX_BANK];
  int dt[MMAD_MAX_BANK];
  for (int i = 0; i < n; ++i) {
    const OnlinePlan& p = m[i].plan;
    a[i] = s < p.len[list] ? p.list[list][s] : MmadSkinny{};
    dt[i] = list == NAP_RUN ? MMAD_F32 : m[i].h->dtype;
  }
  return bank ? mmad_skinny_group_launch(m->key.rows, n, dt, a, st) : mmad_skinny_launch(dt[0], a[0], st);
}

// the launch list of n checked members on stream st (eager, or into a
// capture), its order written once: the members' plans, then every step as
// the single launcher for a scorer's member or (bank) as the grouped one over
// the members that have the step -- a bank of one included.  B, rows and ld_x
// are the call's: m[0]'s are everyone's.  The VIB reparameterisation and the
// group squares stay one launch per member
static int online_walk(OnlineMember* m, int n, bool bank, hipStream_t st) {
  const OnlineKey& k = m->key;
  MmadPackMember pk[MMAD_MAX_BANK];
  MmadOnlineFinish fin[MMAD_MAX_BANK];
  int len[N_LISTS] = {};
  for (int i = 0; i < n; ++i) {
    online_plan(m[i]);
    pk[i] = m[i].plan.pack;
    fin[i] = m[i].plan.fin;
    for (int t = 0; t < N_LISTS; ++t) len[t] = std::max(len[t], m[i].plan.len[t]);
  }
  RET_IF(bank ? mmad_pack_input_group(n, k.B, k.rows, k.ld_x, pk, st)
              : mmad_pack_input(pk->dtype, k.B, pk->K, k.rows, pk->Kp, pk->x, k.ld_x, pk->out, st));
  RET_IF(fold_step(m, n, bank, st));
  for (int s = 0; s < len[PASS1]; ++s) {
    RET_IF(layer_step(m, n, bank, PASS1, s, st));
    for (int i = 0; i < n; ++i) {   // VIB: the reparameterisation reads the encoder's last output
      const mmad_ae* h = m[i].h;
      if (h->vib && s == h->n_enc - 1)
        RET_IF(mmad_vib_reparam_fwd(h->dtype, k.B, h->btl, 1, m[i].o.y[s], h->L[s].Np, nullptr, nullptr, 0, 0, 1,
                                    m[i].o.zbuf, h->L[h->n_enc].Kp, nullptr, st));
    }
  }
  for (int i = 0; i < n; ++i)
    if (m[i].key.G > 0) RET_IF(mmad_group_sq_launch(m[i].plan.gsq, st));
  for (int s = 0; s < len[PASS2]; ++s) RET_IF(layer_step(m, n, bank, PASS2, s, st));
  if (len[NAP_RUN]) RET_IF(layer_step(m, n, bank, NAP_RUN, 0, st));
  return bank ? mmad_online_finish_group(n, fin, k.rows, st) : mmad_online_finish(fin[0], k.rows, st);
}

// once per state: the NAP operand's padding is zeroed here and never written
// again (mmad_ae::online_ready)
static int online_zero_nap(const OnlineMember& m, hipStream_t st) {
  mmad_ae* h = m.h;
  const void* tag = (const char*)m.key.state + (m.key.rows == 16 ? 0 : 1);
  if (h->nap.on && h->online_ready != tag) {
    MMAD_HIP_CHECK(hipMemsetAsync(m.o.nap_x, 0, (size_t)m.key.rows * h->nap.Kp * 4, st));
    h->online_ready = tag;
  }
  return MMAD_OK;
}

// the refusals of the tick's front launches (mmad_mfcc, mmad_hsr_fuse_raw)
// and what they add to a pass's graph signature; nothing launched
static int tick_front_check(const mmad_tick_args* a, TickKey& k) {
  RET_IF(mmad_mfcc_check(a->pcm, a->pcm_type, a->L, a->sr, a->n_fft, a->n_mels, a->n_mfcc, a->plan, a->plan_bytes,
                         a->mfcc_out, a->B, a->mfcc_norm, a->mfcc_ws, a->mfcc_ws_bytes));
  const int64_t F = mmad_mfcc_frames(a->L, a->n_fft);
  MMAD_CHECK_ARG(a->mfcc_norm && a->mfcc_out_bytes >= F * a->n_mfcc * 4 &&
                 a->mfcc_norm_bytes >= (int64_t)a->B * a->n_mfcc * 4,
                 "ae_online_tick: mfcc_out / mfcc_norm null or too small (%lld / %lld bytes for %lld / %d frames)",
                 (long long)a->mfcc_out_bytes, (long long)a->mfcc_norm_bytes, (long long)F, a->B);
  MMAD_CHECK_ARG(a->n_mfcc == 13, "ae_online_tick: n_mfcc=%d, the fusion producer reads 13 coefficients a frame",
                 a->n_mfcc);
  MMAD_CHECK_ARG(a->hsr_weight_count >= mmad_hsr_weight_count(), "ae_online_tick: %d packed HSR weights, needs %d",
                 a->hsr_weight_count, mmad_hsr_weight_count());
  RET_IF(mmad_hsr_fuse_raw_check(a->B, a->r, a->r_type, a->d, a->d_type, a->t, a->mfcc_norm, a->range_in,
                                 a->hsr_weights, 0, a->x, a->ld_x));
  k.pcm = a->pcm; k.r = a->r; k.d = a->d; k.t = a->t;
  k.pcm_type = a->pcm_type; k.r_type = a->r_type; k.d_type = a->d_type;
  k.L = a->L; k.sr = a->sr; k.n_fft = a->n_fft; k.n_mels = a->n_mels; k.n_mfcc = a->n_mfcc;
  k.plan = a->plan; k.mfcc_ws = a->mfcc_ws; k.mfcc_out = a->mfcc_out; k.mfcc_norm = a->mfcc_norm;
  k.hsr_w = a->hsr_weights;
  for (int i = 0; i < 6; ++i) k.range_in[i] = a->range_in[i];
  k.norm_rcp = a->norm_rcp != 0;
  return MMAD_OK;
}

// the front launches: MFCC, then the fused row into a->x
static int tick_front(const mmad_tick_args* a, hipStream_t s) {
  RET_IF(mmad_mfcc(a->pcm, a->pcm_type, a->L, a->sr, a->n_fft, a->n_mels, a->n_mfcc, a->plan, a->plan_bytes,
                   a->mfcc_out, a->B, -1.f, 1.f, a->mfcc_norm, a->mfcc_ws, a->mfcc_ws_bytes, s));
  return mmad_hsr_fuse_raw_launch(a->B, a->r, a->r_type, a->d, a->d_type, a->t, a->mfcc_norm, a->range_in,
                                  a->norm_rcp, a->hsr_weights, 0, a->x, a->ld_x, s);
}

// ---- the sensor bank: the walk over up to MMAD_MAX_BANK handles on one
// shared input, one grouped launch per step (include/mmad.h)
struct BankKey {
  int n = 0;
  OnlineKey k[MMAD_MAX_BANK];   // member i's own signature on x + col0[i]; a tick's front in k[0].tick
  bool operator==(const BankKey& o) const { return n == o.n && std::equal(k, k + n, o.k); }
};

struct mmad_online_bank {
  int n = 0, rows = 0;
  mmad_ae* h[MMAD_MAX_BANK] = {};
  int col0[MMAD_MAX_BANK] = {};
  Stream gstream;             // capture stream; ahead of the graphs captured on it, destroyed after them
  GraphCache<BankKey> graphs{8};
  int nodes = 0;              // kernel nodes of the last captured pass
};

// the launches of a checked call -- (front: a tick's front launches, then) the
// walk over its members -- eagerly, or (use_graph) as the replay of their
// capture, made on the first call.  b: the bank the call came through (its n
// members under bkey, in its own cache, captured on its own stream), or null:
// the one member of a scorer call or tick, in its handle's cache
static int online_run(OnlineMember* m, mmad_online_bank* b, const BankKey* bkey, const mmad_tick_args* front,
                      int use_graph, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int n = b ? b->n : 1;
  for (int i = 0; i < n; ++i) RET_IF(online_zero_nap(m[i], st));
  auto pass = [&](hipStream_t s) {
    if (front) RET_IF(tick_front(front, s));
    return online_walk(m, n, b != nullptr, s);
  };
  if (!use_graph) return pass(st);
  if (b)
    return replay_or_capture(b->graphs, *bkey, st, [&](auto& p, hipGraphExec_t* exec) {
      return capture_graph_on(&b->gstream, p, exec, &b->nodes);
    }, pass);
  return replay_or_capture(m->h->ographs, m->key, st,
                           [&](auto& p, hipGraphExec_t* exec) { return capture_graph(m->h, p, exec); }, pass);
}

static int online_score(mmad_ae* h, const float* x, int ld_x, int B, int rows, const mmad_bank_member& a,
                        bool grouped, int use_graph, void* stream) {
  OnlineMember m;
  RET_IF(member_check(h, x, ld_x, B, rows, a, grouped, m));
  return online_run(&m, nullptr, nullptr, nullptr, use_graph, stream);
}

int mmad_ae_online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                         const float* thresholds, float* out, uint8_t* flags, void* state,
                         int64_t state_bytes, int use_graph, void* stream) {
  const mmad_bank_member a{sap_start, sap_end, thresholds, out, flags, state, state_bytes};
  return online_score(h, x, ld_x, B, 16, a, false, use_graph, stream);
}

int mmad_ae_online_score64(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                           const float* thresholds, float* out, uint8_t* flags, void* state,
                           int64_t state_bytes, int use_graph, void* stream) {
  const mmad_bank_member a{sap_start, sap_end, thresholds, out, flags, state, state_bytes};
  return online_score(h, x, ld_x, B, 64, a, false, use_graph, stream);
}

int mmad_ae_online_score_groups(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                                const float* thresholds, float* out, uint8_t* flags, void* state,
                                int64_t state_bytes, int use_graph, void* stream, int rows,
                                const int* bounds, int G, const float* group_thresholds, float* group_out,
                                uint8_t* group_flags, void* gstate, int64_t gstate_bytes) {
  const mmad_bank_member a{sap_start, sap_end, thresholds, out, flags, state, state_bytes, bounds, G,
                           group_thresholds, group_out, group_flags, gstate, gstate_bytes};
  return online_score(h, x, ld_x, B, rows, a, true, use_graph, stream);
}

// ---- the sensor tick: mmad_mfcc -> mmad_hsr_fuse_raw -> the walk, one
// launch list (one graph).  Every component's refusals run first; the front
// launches are the components' own entry points on the one stream.
int mmad_ae_online_tick(mmad_ae* h, const mmad_tick_args* a, int use_graph, void* stream) {
  MMAD_CHECK_ARG(h && a, "ae_online_tick: null handle or arguments");
  MMAD_CHECK_ARG(a->rows == 16 || a->rows == 64, "ae_online_tick: rows=%d (16 or 64)", a->rows);
  OnlineMember m;
  RET_IF(member_check(h, a->x, a->ld_x, a->B, a->rows, *a, a->bounds != nullptr, m));
  MMAD_CHECK_ARG(h->L[0].K == 1728, "ae_online_tick: the model's input width %d is not the fused row's 1728",
                 h->L[0].K);
  RET_IF(tick_front_check(a, m.key.tick));
  return online_run(&m, nullptr, nullptr, a, use_graph, stream);
}

int mmad_online_bank_create(mmad_online_bank** bank, int n, mmad_ae* const* handles, const int* col0, int rows) {
  MMAD_CHECK_ARG(bank, "online_bank_create: null bank");
  *bank = nullptr;
  MMAD_CHECK_ARG(n >= 1 && n <= MMAD_MAX_BANK, "online_bank_create: n=%d outside 1..%d", n, MMAD_MAX_BANK);
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "online_bank_create: rows=%d (16 or 64)", rows);
  MMAD_CHECK_ARG(handles && col0, "online_bank_create: null handles or col0");
  int n_bn_layers = 0;
  for (int i = 0; i < n; ++i) {
    MMAD_CHECK_ARG(handles[i], "online_bank_create: null handle %d", i);
    MMAD_CHECK_ARG(col0[i] >= 0, "online_bank_create: col0[%d]=%d negative", i, col0[i]);
    for (const AeLayer& a : handles[i]->L) n_bn_layers += a.bn ? 1 : 0;
  }
  MMAD_CHECK_ARG(n_bn_layers <= MMAD_BANK_MAX_BN, "online_bank_create: %d BatchNorm layers over all members "
                 "(at most %d)", n_bn_layers, MMAD_BANK_MAX_BN);
  mmad_online_bank* b = new mmad_online_bank;
  b->n = n; b->rows = rows;
  for (int i = 0; i < n; ++i) { b->h[i] = handles[i]; b->col0[i] = col0[i]; }
  *bank = b;
  return MMAD_OK;
}

void mmad_online_bank_destroy(mmad_online_bank* bank) { delete bank; }

int64_t mmad_online_bank_state_bytes(const mmad_online_bank* bank, int i) {
  if (!bank || i < 0 || i >= bank->n) return -1;
  return online_state_bytes(bank->h[i], bank->rows);
}

int mmad_online_bank_graph_nodes(const mmad_online_bank* bank) { return bank ? bank->nodes : -1; }
int mmad_online_bank_graph_count(const mmad_online_bank* bank) { return bank ? (int)bank->graphs.size() : -1; }

// a checked bank call: its members and the call's signature
struct BankCall {
  OnlineMember m[MMAD_MAX_BANK];
  BankKey key;
};

// every refusal of a bank call: the bank's own on each member's columns, then
// the member's; nothing launched
static int bank_check(mmad_online_bank* b, const float* x, int ld_x, int B, const mmad_bank_member* m,
                      BankCall& c) {
  MMAD_CHECK_ARG(b && m, "online_bank: null bank or members");
  MMAD_CHECK_ARG(x, "online_bank: null x");
  c.key.n = b->n;
  for (int i = 0; i < b->n; ++i) {
    mmad_ae* h = b->h[i];
    const int D = h->L[0].K;
    MMAD_CHECK_ARG((int64_t)b->col0[i] + D <= ld_x, "online_bank: member %d reads columns [%d, %d) of a row of "
                   "ld_x=%d", i, b->col0[i], b->col0[i] + D, ld_x);
    const float* xi = x + b->col0[i];
    MMAD_CHECK_ARG((uintptr_t)xi % 16 == 0 && ld_x % 4 == 0, "online_bank: member %d: x + col0=%d must be "
                   "16-byte aligned and ld_x=%d a multiple of 4 (the grouped pack reads 16-byte quads)", i,
                   b->col0[i], ld_x);
    RET_IF(member_check(h, xi, ld_x, B, b->rows, m[i], m[i].bounds != nullptr, c.m[i]));
    c.key.k[i] = c.m[i].key;
  }
  return MMAD_OK;
}

int mmad_online_bank_score(mmad_online_bank* bank, const float* x, int ld_x, int B,
                           const mmad_bank_member* members, int use_graph, void* stream) {
  BankCall c;
  RET_IF(bank_check(bank, x, ld_x, B, members, c));
  return online_run(c.m, bank, &c.key, nullptr, use_graph, stream);
}

int mmad_online_bank_tick(mmad_online_bank* bank, const mmad_tick_args* a, const mmad_bank_member* members,
                          int use_graph, void* stream) {
  MMAD_CHECK_ARG(bank && a && members, "online_bank_tick: null bank, arguments or members");
  MMAD_CHECK_ARG(a->rows == bank->rows, "online_bank_tick: rows=%d, the bank's is %d", a->rows, bank->rows);
  BankCall c;
  RET_IF(bank_check(bank, a->x, a->ld_x, a->B, members, c));
  RET_IF(tick_front_check(a, c.key.k[0].tick));
  return online_run(c.m, bank, &c.key, a, use_graph, stream);
}
