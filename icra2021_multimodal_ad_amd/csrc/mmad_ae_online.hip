// ---- online scoring: B <= 16 windows through the 16-row weight stream, or
// B <= 64 through the 64-row one (mmad_skinny.hip).  The batch path
// (mmad_ae_score.hip) pads such a call to 128 rows and spends its ~30 launches
// on zeros; here every layer is one launch that reads its weights once.  All
// buffers live in a caller-owned state, carved below for `rows` = 16 or 64: the
// two entry points share the carve and the launch list and differ in the row
// capacity of every buffer and in the two kernels behind it.
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

int64_t mmad_ae_online_state_bytes(const mmad_ae* h) {
  if (!h) return -1;
  OnlineWS o;
  online_carve(h, nullptr, o, 16);
  return o.bytes;
}

int64_t mmad_ae_online_state_bytes64(const mmad_ae* h) {
  if (!h) return -1;
  OnlineWS o;
  online_carve(h, nullptr, o, 64);
  return o.bytes;
}

// the launches of one pass on stream st (eager, or into a capture)
static int online_pass(mmad_ae* h, const float* x, int ld_x, int B, int s0, int s1, const float* thr,
                       float* out, uint8_t* flags, const OnlineWS& o, int rows, hipStream_t st) {
  const int dt = h->dtype;
  const auto launch = rows == 16 ? mmad_skinny_launch : mmad_skinny_rows_launch;
  const int nL = (int)h->L.size();
  const mmad_ae::NapFit& nf = h->nap;
  RET_IF(mmad_pack_input(dt, B, h->L[0].K, rows, h->L[0].Kp, x, ld_x, o.xin, st));
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
    RET_IF(launch(dt, a, st));
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
    RET_IF(launch(dt, a, st));
    cur = o.p2[e];
  }
  // the NAP run: the same kernel on the fit's fp32 V^T (K = W, N = R), bias
  // after the product, colw = 1 / var, no reference
  if (nf.on) {
    MmadSkinny a{};
    a.M = B; a.N = nf.R; a.Np = nf.Rp; a.Kp = nf.Kp;
    a.x = o.nap_x; a.w = nf.vt; a.bias = nf.bias; a.act = MMAD_ACT_NONE;
    a.colw = nf.w; a.rowsq = o.nap_rs;
    RET_IF(launch(MMAD_F32, a, st));
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
  return rows == 16 ? mmad_online_finish(fin, st) : mmad_online_finish64(fin, st);
}

// both entry points; rows = 16 (mmad_ae_online_score) or 64 (_score64)
static int online_score(mmad_ae* h, const float* x, int ld_x, int B, int sap_start, int sap_end,
                        const float* thresholds, float* out, uint8_t* flags, void* state,
                        int64_t state_bytes, int use_graph, void* stream, int rows) {
  MMAD_CHECK_ARG(h, "ae_online_score: null handle");
  const char* sfx = rows == 16 ? "" : "64";
  MMAD_CHECK_ARG(B >= 1 && B <= rows, "ae_online_score%s: B=%d outside 1..%d (the batch path, "
                 "mmad_ae_score_stream, serves larger calls)", sfx, B, rows);
  const int64_t need = rows == 16 ? mmad_ae_online_state_bytes(h) : mmad_ae_online_state_bytes64(h);
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
  hipStream_t st = (hipStream_t)stream;
  OnlineWS o;
  online_carve(h, (char*)state, o, rows);
  const void* tag = (const char*)state + (rows == 16 ? 0 : 1);   // mmad_ae::online_ready
  if (h->nap.on && h->online_ready != tag) {
    MMAD_HIP_CHECK(hipMemsetAsync(o.nap_x, 0, (size_t)rows * h->nap.Kp * 4, st));
    h->online_ready = tag;
  }
  auto pass = [&](hipStream_t s) {
    return online_pass(h, x, ld_x, B, s0, s1, thresholds, out, flags, o, rows, s);
  };
  if (!use_graph) return pass(st);
  const void* nap_vt = h->nap.on ? (const void*)h->nap.vt : nullptr;
  const OnlineKey key{x, ld_x, B, s0, s1, thresholds, out, flags, state, weights(h, h->L[0]), nap_vt, rows};
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
