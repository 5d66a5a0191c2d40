// ---- online scoring: B <= 16 windows through the 16-row weight stream, or
// B <= 64 through the 64-row one (mmad_skinny.hip).  The batch path
// (mmad_ae_score.hip) pads such a call to 128 rows and spends its ~30 launches
// on zeros; here every layer is one launch that reads its weights once.  All
// buffers live in a caller-owned state, carved below for `rows` = 16 or 64: the
// two entry points share the carve, the launch list and the kernels and differ
// in the row capacity of every buffer.
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

// per-modality scores of a grouped pass (mmad_ae_online_score_groups)
struct OnlineGroups {
  int G;
  int bounds[MMAD_MAX_GROUPS + 1];
  const float* thr;   // [G], nullable
  float* out;         // [G][rows]
  uint8_t* flags;     // [G][rows], nullable
  float* d0;          // the groups buffer [rows][Kp0]
};

// the launch list of one model's pass, step by step: what online_pass
// launches one by one and the bank (bank_pass) launches step-wise over its
// members.  p1 / p2: the weight-stream launches of pass 1 (every layer) and
// pass 2 (the encoder again)
struct OnlinePlan {
  mmad_ae* h;
  int dt, B, rows, ld_x;
  MmadPackMember pack;
  MmadOnlineFold fold;
  std::vector<MmadSkinny> p1, p2;
  int vib_after = -1;   // VIB: the pass-1 layer whose output the reparameterisation reads
  const void* vib_in = nullptr;
  int vib_ld = 0;
  bool grouped = false;
  MmadGroupSq gsq;
  bool nap = false;
  MmadSkinny napa;
  MmadOnlineFinish fin;
};

static int plan_vib(const OnlinePlan& p, const OnlineWS& o, hipStream_t st) {
  const mmad_ae* h = p.h;
  return mmad_vib_reparam_fwd(p.dt, p.B, h->btl, 1, p.vib_in, p.vib_ld, nullptr, nullptr, 0, 0, 1, o.zbuf,
                              h->L[h->n_enc].Kp, nullptr, st);
}

// gr: null, or the groups of a grouped pass -- one more launch, nothing else moves
static void online_plan(mmad_ae* h, const float* x, int ld_x, int B, int s0, int s1, const float* thr,
                        float* out, uint8_t* flags, const OnlineWS& o, int rows, const OnlineGroups* gr,
                        OnlinePlan& p) {
  const int dt = h->dtype;
  const int nL = (int)h->L.size();
  const mmad_ae::NapFit& nf = h->nap;
  p.h = h; p.dt = dt; p.B = B; p.rows = rows; p.ld_x = ld_x;
  p.pack = MmadPackMember{dt, h->L[0].K, h->L[0].Kp, x, o.xin};
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
  const float* d0 = nullptr;   // grouped pass: where the last decoder launch leaves d0
  int ldd0 = 0;
  // pass 1: eval forward; the decoder's last layer scores d0 = x_hat - x
  for (int l = 0; l < nL; ++l) {
    const AeLayer& L = h->L[l];
    const void* in = l == 0 ? o.xin : (h->vib && l == h->n_enc ? o.zbuf : o.y[l - 1]);
    MmadSkinny a = layer(L, in, o.y[l]);
    if (l == nL - 1) {
      a.ref = o.xin; a.ref_f32 = 0; a.ldref = h->L[0].Kp;
      a.rowsq = o.rs[0];
      route(a, 0);
      if (gr) {
        // d0 where the pass stores it already (the fit's operand), else into
        // the groups buffer: the kernel and rowsq are the ungrouped pass's
        if (!a.diff) { a.diff = gr->d0; a.lddiff = h->L[0].Kp; }
        d0 = a.diff; ldd0 = a.lddiff;
      }
    }
    p.p1.push_back(a);
    if (h->vib && l == h->n_enc - 1) { p.vib_after = l; p.vib_in = o.y[l]; p.vib_ld = L.Np; }
  }
  p.grouped = gr != nullptr;
  if (gr) {
    // all `rows` rows: rows >= B hold d = 0, so score 0 (and flag 0: n_flag)
    MmadGroupSq& q = p.gsq;
    q = MmadGroupSq{};
    q.d = d0; q.ldd = ldd0; q.N = rows; q.n_flag = B; q.G = gr->G;
    for (int g = 0; g <= gr->G; ++g) q.bounds[g] = gr->bounds[g];
    q.thr = gr->thr; q.out = gr->out; q.ldo = rows; q.flags = gr->flags; q.ldf = rows;
  }
  // pass 2: x_hat through the encoder, each layer against its pass-1 output
  const void* cur = o.y[nL - 1];
  for (int e = 0; e < h->n_enc; ++e) {
    const AeLayer& L = h->L[e];
    MmadSkinny a = layer(L, cur, o.p2[e]);
    a.ref = o.y[e]; a.ref_f32 = 0; a.ldref = L.Np;
    a.rowsq = o.rs[e + 1];
    route(a, e + 1);
    p.p2.push_back(a);
    cur = o.p2[e];
  }
  // the NAP run: the same kernel on the fit's fp32 V^T (K = W, N = R), bias
  // after the product, colw = 1 / var, no reference
  p.nap = nf.on;
  if (nf.on) {
    MmadSkinny& a = p.napa;
    a = MmadSkinny{};
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
  fin.sap_start = s0; fin.sap_end = s1;
  if (nf.on) { fin.nap_rs = o.nap_rs; fin.nap_tiles = nf.Rp / 16; fin.nap_scale = 1.f / (float)nf.R; }
  fin.out = out; fin.flags = flags; fin.thresholds = thr;
}

// the launches of one pass on stream st (eager, or into a capture)
static int online_pass(mmad_ae* h, const float* x, int ld_x, int B, int s0, int s1, const float* thr,
                       float* out, uint8_t* flags, const OnlineWS& o, int rows, hipStream_t st,
                       const OnlineGroups* gr = nullptr) {
  OnlinePlan p;
  online_plan(h, x, ld_x, B, s0, s1, thr, out, flags, o, rows, gr, p);
  RET_IF(mmad_pack_input(p.dt, B, p.pack.K, rows, p.pack.Kp, x, ld_x, o.xin, st));
  RET_IF(mmad_online_fold(p.fold, h->params, h->running, h->bn_eps, o.scale, o.shift, st));
  for (int l = 0; l < (int)p.p1.size(); ++l) {
    RET_IF(mmad_skinny_launch(p.dt, p.p1[l], st));
    if (l == p.vib_after) RET_IF(plan_vib(p, o, st));
  }
  if (p.grouped) RET_IF(mmad_group_sq_launch(p.gsq, st));
  for (const MmadSkinny& a : p.p2) RET_IF(mmad_skinny_launch(p.dt, a, st));
  if (p.nap) RET_IF(mmad_skinny_launch(MMAD_F32, p.napa, st));
  return mmad_online_finish(p.fin, rows, st);
}

int64_t mmad_ae_online_groups_bytes(const mmad_ae* h, int rows) {
  if (!h || (rows != 16 && rows != 64)) return -1;
  return ((int64_t)rows * h->L[0].Kp * 4 + 255) / 256 * 256;
}

// the grouped forms' own refusals (rows, G, bounds); fills gr but for d0
static int groups_check(int rows, const int* bounds, int G, const float* group_thresholds, float* group_out,
                        uint8_t* group_flags, OnlineGroups& gr) {
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "ae_online_score_groups: rows=%d (16 or 64)", rows);
  MMAD_CHECK_ARG(G >= 1 && G <= MMAD_MAX_GROUPS, "ae_online_score_groups: G=%d outside 1..%d", G,
                 MMAD_MAX_GROUPS);
  MMAD_CHECK_ARG(bounds && bounds[0] >= 0, "ae_online_score_groups: bounds null or bounds[0] negative");
  gr = OnlineGroups{};
  gr.G = G;
  for (int g = 0; g <= G; ++g) gr.bounds[g] = bounds[g];
  for (int g = 0; g < G; ++g)
    MMAD_CHECK_ARG(bounds[g] < bounds[g + 1], "ae_online_score_groups: bounds not strictly ascending "
                   "(bounds[%d]=%d, bounds[%d]=%d)", g, bounds[g], g + 1, bounds[g + 1]);
  gr.thr = group_thresholds; gr.out = group_out; gr.flags = group_flags;
  return MMAD_OK;
}

// one call of an entry point, checked: the carved state, the clamped SAP range
// and the pass's graph signature
struct OnlineCall {
  OnlineWS o;
  int s0, s1;
  OnlineKey key;
};

// every refusal of the entry points; rows = 16 (mmad_ae_online_score) or 64
// (_score64); gr: the grouped form's arguments, checked here (d0 filled in).
// Nothing is launched.
static int online_check(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                        const float* thresholds, float* out, uint8_t* flags, void* state,
                        int64_t state_bytes, int rows, OnlineGroups* gr, void* gstate,
                        int64_t gstate_bytes, OnlineCall& c) {
  MMAD_CHECK_ARG(h, "ae_online_score: null handle");
  if (gr) {
    MMAD_CHECK_ARG(gr->bounds[gr->G] <= h->L[0].K, "ae_online_score_groups: bounds[G]=%d exceeds the "
                   "input width D=%d", gr->bounds[gr->G], h->L[0].K);
    MMAD_CHECK_ARG(gr->out, "ae_online_score_groups: null group_out");
    const int64_t gneed = mmad_ae_online_groups_bytes(h, rows);
    MMAD_CHECK_ARG(gstate && gstate_bytes >= gneed, "ae_online_score_groups: gstate null or too small "
                   "(%lld < %lld bytes, mmad_ae_online_groups_bytes)",
                   (long long)(gstate ? gstate_bytes : 0), (long long)gneed);
    MMAD_CHECK_ARG(((uintptr_t)gstate) % 256 == 0, "ae_online_score_groups: gstate must be 256-byte aligned");
    gr->d0 = (float*)gstate;
  }
  const char* sfx = rows == 16 ? "" : "64";
  MMAD_CHECK_ARG(B >= 1 && B <= rows, "ae_online_score%s: B=%d outside 1..%d (the batch path, "
                 "mmad_ae_score_stream, serves larger calls)", sfx, B, rows);
  const int64_t need = online_state_bytes(h, rows);
  MMAD_CHECK_ARG(state && state_bytes >= need, "ae_online_score: online state null or too small "
                 "(%lld < %lld bytes, mmad_ae_online_state_bytes%s)", (long long)(state ? state_bytes : 0),
                 (long long)need, sfx);
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
  c.s0 = s0; c.s1 = s1;
  online_carve(h, (char*)state, c.o, rows);
  const void* nap_vt = h->nap.on ? (const void*)h->nap.vt : nullptr;
  c.key = OnlineKey{x, ld_x, B, s0, s1, thresholds, out, flags, state, weights(h, h->L[0]), nap_vt, rows};
  if (gr) {
    c.key.G = gr->G;
    for (int g = 0; g <= gr->G; ++g) c.key.bounds[g] = gr->bounds[g];
    c.key.gthr = gr->thr; c.key.gout = gr->out; c.key.gflags = gr->flags; c.key.gstate = gstate;
  }
  return MMAD_OK;
}

// a checked call's launches: pass(stream) eagerly, or (use_graph) the replay
// of its capture under key, made on the first call
template <class Pass>
static int online_run(mmad_ae* h, const OnlineWS& o, const OnlineKey& key, int use_graph, hipStream_t st,
                      Pass pass) {
  const void* tag = (const char*)key.state + (key.rows == 16 ? 0 : 1);   // mmad_ae::online_ready
  if (h->nap.on && h->online_ready != tag) {
    MMAD_HIP_CHECK(hipMemsetAsync(o.nap_x, 0, (size_t)key.rows * h->nap.Kp * 4, st));
    h->online_ready = tag;
  }
  if (!use_graph) return pass(st);
  if (hipGraphExec_t hit = h->ographs.find(key)) {
    MMAD_HIP_CHECK(hipGraphLaunch(hit, st));
    return MMAD_OK;
  }
  RET_IF(pass(st));
  hipGraphExec_t exec = nullptr;
  RET_IF(capture_error(capture_graph(h, pass, &exec)));
  h->ographs.insert(key, exec);   // bounded cache: drops the oldest pass
  return MMAD_OK;
}

static int online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                        const float* thresholds, float* out, uint8_t* flags, void* state,
                        int64_t state_bytes, int use_graph, void* stream, int rows,
                        OnlineGroups* gr = nullptr, void* gstate = nullptr, int64_t gstate_bytes = 0) {
  OnlineCall c;
  RET_IF(online_check(h, x, ld_x, B, sap_start, sap_end, thresholds, out, flags, state, state_bytes, rows, gr,
                      gstate, gstate_bytes, c));
  return online_run(h, c.o, c.key, use_graph, (hipStream_t)stream, [&](hipStream_t s) {
    return online_pass(h, x, ld_x, B, c.s0, c.s1, thresholds, out, flags, c.o, rows, s, gr);
  });
}

int mmad_ae_online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                         const float* thresholds, float* out, uint8_t* flags, void* state,
                         int64_t state_bytes, int use_graph, void* stream) {
  return online_score(h, x, ld_x, B, sap_start, sap_end, thresholds, out, flags, state, state_bytes,
                      use_graph, stream, 16);
}

int mmad_ae_online_score64(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                           const float* thresholds, float* out, uint8_t* flags, void* state,
                           int64_t state_bytes, int use_graph, void* stream) {
  return online_score(h, x, ld_x, B, sap_start, sap_end, thresholds, out, flags, state, state_bytes,
                      use_graph, stream, 64);
}

int mmad_ae_online_score_groups(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                                const float* thresholds, float* out, uint8_t* flags, void* state,
                                int64_t state_bytes, int use_graph, void* stream, int rows,
                                const int* bounds, int G, const float* group_thresholds, float* group_out,
                                uint8_t* group_flags, void* gstate, int64_t gstate_bytes) {
  OnlineGroups gr{};
  RET_IF(groups_check(rows, bounds, G, group_thresholds, group_out, group_flags, gr));
  return online_score(h, x, ld_x, B, sap_start, sap_end, thresholds, out, flags, state, state_bytes,
                      use_graph, stream, rows, &gr, gstate, gstate_bytes);
}

// ---- the sensor tick: mmad_mfcc -> mmad_hsr_fuse_raw -> the pass above, one
// launch list (one graph).  Every component's refusals run first; the launches
// are the components' own entry points on the one stream.
static int tick_front_check(const mmad_tick_args* a, TickKey& k);
static int tick_front(const mmad_tick_args* a, hipStream_t s);

int mmad_ae_online_tick(mmad_ae* h, const mmad_tick_args* a, int use_graph, void* stream) {
  MMAD_CHECK_ARG(h && a, "ae_online_tick: null handle or arguments");
  MMAD_CHECK_ARG(a->rows == 16 || a->rows == 64, "ae_online_tick: rows=%d (16 or 64)", a->rows);
  OnlineGroups gr{};
  const bool grouped = a->bounds != nullptr;
  if (grouped)
    RET_IF(groups_check(a->rows, a->bounds, a->G, a->group_thresholds, a->group_out, a->group_flags, gr));
  OnlineCall c;
  RET_IF(online_check(h, a->x, a->ld_x, a->B, a->sap_start, a->sap_end, a->thresholds, a->out, a->flags,
                      a->state, a->state_bytes, a->rows, grouped ? &gr : nullptr, a->gstate, a->gstate_bytes, c));
  MMAD_CHECK_ARG(h->L[0].K == 1728, "ae_online_tick: the model's input width %d is not the fused row's 1728",
                 h->L[0].K);
  RET_IF(tick_front_check(a, c.key.tick));
  return online_run(h, c.o, c.key, use_graph, (hipStream_t)stream, [&](hipStream_t s) {
    RET_IF(tick_front(a, s));
    return online_pass(h, a->x, a->ld_x, a->B, c.s0, c.s1, a->thresholds, a->out, a->flags, c.o, a->rows, s,
                       grouped ? &gr : nullptr);
  });
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

// ---- the sensor bank: the passes of up to MMAD_MAX_BANK handles on one
// shared input, step by step, one grouped launch per step (include/mmad.h)
struct BankKey {
  int n = 0;
  OnlineKey k[MMAD_MAX_BANK];   // member i's own signature on x + col0[i]; a tick's front in k[0].tick
  bool operator==(const BankKey& o) const { return n == o.n && std::equal(k, k + n, o.k); }
};

struct mmad_online_bank {
  int n = 0, rows = 0;
  mmad_ae* h[MMAD_MAX_BANK] = {};
  int col0[MMAD_MAX_BANK] = {};
  GraphCache<BankKey> graphs{8};
  hipStream_t gstream = nullptr;   // capture stream
  int nodes = 0;                   // kernel nodes of the last captured pass
  ~mmad_online_bank() {
    graphs.clear();
    if (gstream) (void)hipStreamDestroy(gstream);
  }
};

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

// a checked bank call: every member's checked call, groups and launch list
struct BankCall {
  OnlineCall c[MMAD_MAX_BANK];
  OnlineGroups gr[MMAD_MAX_BANK];
  OnlinePlan p[MMAD_MAX_BANK];
  BankKey key;
};

// every refusal of a bank call, then the members' launch lists; nothing launched
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
    const bool grouped = m[i].bounds != nullptr;
    if (grouped)
      RET_IF(groups_check(b->rows, m[i].bounds, m[i].G, m[i].group_thresholds, m[i].group_out, m[i].group_flags,
                          c.gr[i]));
    RET_IF(online_check(h, xi, ld_x, B, m[i].sap_start, m[i].sap_end, m[i].thresholds, m[i].out, m[i].flags,
                        m[i].state, m[i].state_bytes, b->rows, grouped ? &c.gr[i] : nullptr, m[i].gstate,
                        m[i].gstate_bytes, c.c[i]));
    c.key.k[i] = c.c[i].key;
    online_plan(h, xi, ld_x, B, c.c[i].s0, c.c[i].s1, m[i].thresholds, m[i].out, m[i].flags, c.c[i].o, b->rows,
                grouped ? &c.gr[i] : nullptr, c.p[i]);
  }
  return MMAD_OK;
}

// the bank's launches on stream st: the steps of online_pass, each over the
// members that have it
static int bank_pass(const mmad_online_bank* b, const BankCall& c, hipStream_t st) {
  const int n = b->n, rows = b->rows;
  const OnlinePlan* p = c.p;
  MmadPackMember pk[MMAD_MAX_BANK];
  MmadOnlineFoldGroup fg{};
  MmadOnlineFinish fin[MMAD_MAX_BANK];
  size_t n1 = 0, n2 = 0;
  bool any_nap = false;
  fg.n = n;
  for (int i = 0; i < n; ++i) {
    pk[i] = p[i].pack;
    const MmadOnlineFold& f = p[i].fold;
    const mmad_ae* h = p[i].h;
    const OnlineWS& o = c.c[i].o;
    int e = fg.first[i];
    for (int l = 0; l < f.n; ++l, ++e) {
      fg.bn_off[e] = f.bn_off[l]; fg.N[e] = f.N[l]; fg.g_off[e] = f.g_off[l]; fg.be_off[e] = f.be_off[l];
    }
    fg.first[i + 1] = e;
    fg.m[i] = MmadOnlineFoldMember{h->params, h->running, o.scale, o.shift, h->bn_eps, f.n_bn};
    fin[i] = p[i].fin;
    n1 = std::max(n1, p[i].p1.size());
    n2 = std::max(n2, p[i].p2.size());
    any_nap = any_nap || p[i].nap;
  }
  RET_IF(mmad_pack_input_group(n, p[0].B, rows, p[0].ld_x, pk, st));
  RET_IF(mmad_online_fold_group(fg, st));
  MmadSkinny a[MMAD_MAX_BANK];
  int dt[MMAD_MAX_BANK];
  // step s of a launch list over the members that reach it (N = 0: none here)
  auto step = [&](auto list, size_t s) {
    for (int i = 0; i < n; ++i) {
      const std::vector<MmadSkinny>& v = list(p[i]);
      a[i] = s < v.size() ? v[s] : MmadSkinny{};
      dt[i] = p[i].dt;
    }
    return mmad_skinny_group_launch(rows, n, dt, a, st);
  };
  for (size_t s = 0; s < n1; ++s) {
    RET_IF(step([](const OnlinePlan& q) -> const std::vector<MmadSkinny>& { return q.p1; }, s));
    for (int i = 0; i < n; ++i)
      if ((int)s == p[i].vib_after) RET_IF(plan_vib(p[i], c.c[i].o, st));
  }
  for (int i = 0; i < n; ++i)
    if (p[i].grouped) RET_IF(mmad_group_sq_launch(p[i].gsq, st));
  for (size_t s = 0; s < n2; ++s)
    RET_IF(step([](const OnlinePlan& q) -> const std::vector<MmadSkinny>& { return q.p2; }, s));
  if (any_nap) {
    for (int i = 0; i < n; ++i) {
      a[i] = p[i].nap ? p[i].napa : MmadSkinny{};
      dt[i] = MMAD_F32;
    }
    RET_IF(mmad_skinny_group_launch(rows, n, dt, a, st));
  }
  return mmad_online_finish_group(n, fin, rows, st);
}

// a checked bank call's launches: eagerly, or (use_graph) the replay of its
// capture, made on the first call (online_run's policy, the bank's own cache)
template <class Pass>
static int bank_run(mmad_online_bank* b, const BankCall& c, int use_graph, hipStream_t st, Pass pass) {
  for (int i = 0; i < b->n; ++i) {
    mmad_ae* h = b->h[i];
    const OnlineKey& key = c.key.k[i];
    const void* tag = (const char*)key.state + (key.rows == 16 ? 0 : 1);   // mmad_ae::online_ready
    if (h->nap.on && h->online_ready != tag) {
      MMAD_HIP_CHECK(hipMemsetAsync(c.c[i].o.nap_x, 0, (size_t)key.rows * h->nap.Kp * 4, st));
      h->online_ready = tag;
    }
  }
  if (!use_graph) return pass(st);
  if (hipGraphExec_t hit = b->graphs.find(c.key)) {
    MMAD_HIP_CHECK(hipGraphLaunch(hit, st));
    return MMAD_OK;
  }
  RET_IF(pass(st));
  hipGraphExec_t exec = nullptr;
  int nodes = 0;
  RET_IF(capture_error(capture_graph_on(&b->gstream, pass, &exec, &nodes)));
  b->nodes = nodes;
  b->graphs.insert(c.key, exec);   // bounded cache: drops the oldest pass
  return MMAD_OK;
}

int mmad_online_bank_score(mmad_online_bank* bank, const float* x, int ld_x, int B,
                           const mmad_bank_member* members, int use_graph, void* stream) {
  BankCall c;
  RET_IF(bank_check(bank, x, ld_x, B, members, c));
  return bank_run(bank, c, use_graph, (hipStream_t)stream, [&](hipStream_t s) { return bank_pass(bank, c, s); });
}

int mmad_online_bank_tick(mmad_online_bank* bank, const mmad_tick_args* a, const mmad_bank_member* members,
                          int use_graph, void* stream) {
  MMAD_CHECK_ARG(bank && a && members, "online_bank_tick: null bank, arguments or members");
  MMAD_CHECK_ARG(a->rows == bank->rows, "online_bank_tick: rows=%d, the bank's is %d", a->rows, bank->rows);
  BankCall c;
  RET_IF(bank_check(bank, a->x, a->ld_x, a->B, members, c));
  RET_IF(tick_front_check(a, c.key.k[0].tick));
  return bank_run(bank, c, use_graph, (hipStream_t)stream, [&](hipStream_t s) {
    RET_IF(tick_front(a, s));
    return bank_pass(bank, c, s);
  });
}
