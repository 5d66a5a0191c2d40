// Scoring side of the whole-autoencoder executor (mmad_ae_score* / *_nap* in
// include/mmad.h): the batch score pass, its streaming and graph-replayed
// form, the streamed NAP score and the streaming NAP fit.  The handle and the
// helpers shared with the training executor are in mmad_ae_impl.h.
#include "mmad_ae_impl.h"

using namespace mmad_ae_impl;

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
int mmad_ae_impl::diff_col(const mmad_ae* h, int j) {
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

// one batch of the scoring pass on a prepared workspace; layer_sq row l at
// layer_sq + l*ld_sq
// nap (nullable; needs a fit and no caller diffs): the in-range score GEMMs
// write their diffs straight into the packed NAP operand, then the NAP GEMM
// and its column sum write nap[0..B)
// fit (nullable, without nap; the streaming NAP fit): the diffs of its layers
// go, as fp32, into its own packed operand and nothing else changes
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
  auto pass = [&](hipStream_t s) {
    return score_pass(h, x, ld_x, N, batch, layer_sq, ld_sq, nap, ws, ws_bytes, s);
  };
  if (!use_graph) return pass(st);
  const ScoreKey key{x, ld_x, N, batch, layer_sq, ld_sq, ws, score_weights(h), nap, nap_vt};
  return replay_or_capture(h->graphs, key, st,
                           [&](auto& p, hipGraphExec_t* exec) { return capture_graph(h, p, exec); }, pass);
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
