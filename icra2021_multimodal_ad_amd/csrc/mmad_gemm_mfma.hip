// MFMA GEMM for the fc_module stack on gfx950: host planning and launch.  The
// kernels are in mmad_gemm_body.h (tile body) over mmad_gemm_dev.h (tiles, LDS
// images, helpers); tile 8's two kernels are compiled in mmad_gemm_b4.hip.
#include "mmad_gemm_body.h"

#include <cstdlib>
#include <map>
#include <mutex>

// tile 8's kernels (mmad_gemm_b4.hip)
const void* mmad_gemm_b4_kernel(int epi);

// -------------------------------------------------------------------------
// host-side planning and launch
//
// "Which kernel runs for this problem" is answered here and nowhere else:
//   TILES        what a tile is: its numbers (from Cfg<N>) and its kind;
//   tile_allowed / tile_runs
//                which tiles may be chosen for a GemmProblem, and the tile
//                whose kernel then runs (a register-direct tile outside its
//                epilogue runs as its row-quad base: same shape, same bits);
//   kernel_of    (tile, persistent) -> kernel instantiation, from TILES.
// The dispatcher, the tuner, the planners and the launch path only read
// these.  A new tile of an existing kind is entered in ONE place: its row of
// TILES (next to its Cfg<N> and NCFG); a new kind adds its flag and its
// clause in tile_allowed.
// -------------------------------------------------------------------------
struct Tile {
  int BM, BN, NT;
  bool big;       // a 256x256 tile
  bool xst;       // stores register-direct (MFMA operands swapped)
  int base;       // the row-quad tile of the same shape (itself unless xst)
  bool persist;   // has a persistent form (mmad_gemm_kernel_p, knob 12)
};
template <int C>
constexpr Tile tile(bool big = false, bool xst = false, int base = C, bool persist = false) {
  return {Cfg<C>::BM, Cfg<C>::BN, Cfg<C>::NT, big, xst, base, persist};
}
constexpr Tile TILES[NCFG] = {
    tile<0>(),
    tile<1>(false, false, 1, true),
    tile<2>(false, false, 2, true),
    tile<3>(),
    tile<4>(),
    tile<5>(),
    tile<CFG_BIG>(true, false, CFG_BIG, true),
    tile<CFG_XST>(true, true, CFG_BIG, true),
    tile<CFG_B4>(true, true, CFG_BIG),
    tile<CFG_XST1>(false, true, 1),
};
// callers size buffers from the tile that runs (the MSE loss partials), and
// the fallback is meant to change no bit: a base keeps its tile's shape
constexpr bool bases_keep_shape() {
  for (int c = 0; c < NCFG; ++c) {
    const Tile &t = TILES[c], &b = TILES[t.base];
    if (b.BM != t.BM || b.BN != t.BN || b.xst || (!t.xst && t.base != c)) return false;
  }
  return true;
}
static_assert(bases_keep_shape(), "a tile's row-quad base must have its shape");

// may `cfg` be chosen for `p`?  (Co-residency of a fused-BN grid is a device
// query the callers apply on top.)
static bool tile_allowed(int cfg, const GemmProblem& p) {
  if (cfg < 0 || cfg >= NCFG) return false;
  const Tile& t = TILES[cfg];
  const int e = p.epi;
  if (p.dtype != MMAD_BF16 && p.dtype != MMAD_F32) return false;
  if (e < GEMM_EPI_FWD || e > GEMM_EPI_SCORE) return false;
  if (p.Mp <= 0 || p.Np <= 0 || p.Mp % t.BM || p.Np % t.BN) return false;
  // 256x256: bf16 forward-type epilogues; register-direct: eval forward / score
  const bool bf16_in = p.dtype == MMAD_BF16;
  if (t.big && !(bf16_in && (e == GEMM_EPI_FWD || e == GEMM_EPI_MSE || e == GEMM_EPI_SCORE))) return false;
  if (t.xst && !(bf16_in && (e == GEMM_EPI_FWD || e == GEMM_EPI_SCORE))) return false;
  // the score epilogue reduces rows over 128-column groups inside one tile
  if (e == GEMM_EPI_SCORE && t.BN < 128) return false;
  // neither kind combines split-K slices or joins the fused-BN column barrier
  if ((t.big || t.xst) && (p.splitk > 1 || p.fused_bn)) return false;
  if (p.fused_bn && e != GEMM_EPI_FWD && e != GEMM_EPI_BWD_DATA) return false;
  return true;
}

// the tile whose kernel is launched when an allowed `cfg` is chosen: the
// register-direct epilogue has no column partials (the BN statistics need the
// row-quad layout) and piecewise-linear activations only
static int tile_runs(int cfg, const GemmProblem& p) {
  const Tile& t = TILES[cfg];
  return t.xst && (p.partials || !act_is_linear_piecewise(p.act)) ? t.base : cfg;
}

int mmad_gemm_tile(int cfg, const GemmProblem& p) { return tile_allowed(cfg, p) ? tile_runs(cfg, p) : -1; }

int mmad_gemm_ntiles(int cfg, int Mp, int Np) { return (Mp / TILES[cfg].BM) * (Np / TILES[cfg].BN); }

int mmad_gemm_tiles(int Mp, int Np) { return (Mp / 64) * (Np / 64); }

// static choice when autotuning is off or impossible (stream capture)
template <typename Pred>
static int heuristic_cfg(int Mp, int Np, Pred allowed) {
  const int order[] = {CFG_BIG, 1, 0, 5, 4, 3};
  const int want[] = {512, 200, 200, 200, 160, 0};
  for (int i = 0; i < 6; ++i) {
    const int c = order[i];
    if (!allowed(c)) continue;
    if (mmad_gemm_ntiles(c, Mp, Np) >= want[i]) return c;
  }
  for (int c : {4, 0, 3, 5, 2, 1})
    if (allowed(c)) return c;
  return -1;
}

// group height balancing the per-XCD A-panel (gm*BM rows) and B-panel
// ((ntiles/8/gm)*BN cols) footprints
static int plan_group_m(int ntiles, int tiles_m, int BM, int BN) {
  const double per_xcd = ntiles / 8.0;
  int gm = (int)(sqrt(per_xcd * BN / BM) + 0.5);
  const int env_gm = mmad_group_override();
  if (env_gm > 0) gm = env_gm;
  return gm < 1 ? 1 : (gm > tiles_m ? tiles_m : gm);
}

// ---- the kernel table: (tile, persistent) -> instantiation, or null --------
// Generated from TILES: tile C is instantiated for the (operand type,
// epilogue) pairs its kind takes (big_ok / xst_ok), its persistent form for
// the forward-type bf16 pairs (big_ok's) if the table gives it one.
template <typename T, typename TO, bool AK, bool BK_, int EPI, int C = 0>
static const void* kernel_of(int cfg, bool persistent) {
  if constexpr (C < NCFG) {
    if (cfg != C) return kernel_of<T, TO, AK, BK_, EPI, C + 1>(cfg, persistent);
    constexpr Tile t = TILES[C];
    if constexpr ((!t.big || big_ok<T, EPI>()) && (!t.xst || xst_ok<T, EPI>())) {
      if (persistent) {
        if constexpr (t.persist && big_ok<T, EPI>()) return (const void*)mmad_gemm_kernel_p<T, TO, AK, BK_, C, EPI>;
      } else if constexpr (C == CFG_B4) {
        return mmad_gemm_b4_kernel(EPI);   // compiled in the 4-wave translation unit
      } else {
        return (const void*)mmad_gemm_kernel<T, TO, AK, BK_, C, EPI>;
      }
    }
  }
  return nullptr;
}
static const void* kernel_for(int dtype, int epi, int cfg, bool persistent) {
#define MMAD_EPIS(T)                                                                              \
  switch (epi) {                                                                                  \
    case GEMM_EPI_FWD: return kernel_of<T, T, true, true, GEMM_EPI_FWD>(cfg, persistent);         \
    case GEMM_EPI_MSE: return kernel_of<T, T, true, true, GEMM_EPI_MSE>(cfg, persistent);         \
    case GEMM_EPI_SCORE: return kernel_of<T, T, true, true, GEMM_EPI_SCORE>(cfg, persistent);     \
    case GEMM_EPI_BWD_DATA: return kernel_of<T, T, true, false, GEMM_EPI_BWD_DATA>(cfg, persistent); \
    case GEMM_EPI_BWD_WEIGHT:                                                                     \
      return kernel_of<T, float, false, false, GEMM_EPI_BWD_WEIGHT>(cfg, persistent);             \
  }                                                                                               \
  return nullptr
  if (dtype == MMAD_BF16) { MMAD_EPIS(bf16); }
  MMAD_EPIS(float);
#undef MMAD_EPIS
}

// ---- the capacity cache: blocks of a kernel resident on a device at once ----
// CUs x min(occupancy API, the LDS bound); 0 if unknown.  The persistent grid
// is this rounded down to a multiple of 8 (XCD labels); a fused-BN grid must
// not exceed it (its column barrier needs every block resident).
namespace {
std::mutex g_cap_mu;
std::map<std::pair<int, const void*>, int> g_cap;   // (device, kernel) -> resident blocks
}  // namespace

static int kernel_capacity(const void* fn, int threads) {
  int dev = 0;
  if (!fn || hipGetDevice(&dev) != hipSuccess) return 0;
  const auto key = std::make_pair(dev, fn);
  {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    auto it = g_cap.find(key);
    if (it != g_cap.end()) return it->second;
  }
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    per_cu = 0;
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.sharedSizeBytes > 0) {
    const int lds_bound = (int)(163840 / fa.sharedSizeBytes);
    per_cu = per_cu < lds_bound ? per_cu : lds_bound;
  }
  (void)hipGetLastError();
  const int cap = per_cu > 0 && cus > 0 ? per_cu * cus : 0;
  std::lock_guard<std::mutex> lk(g_cap_mu);
  g_cap[key] = cap;
  return cap;
}

// the whole grid of an allowed `cfg` resident at once
static bool coresident(int cfg, const GemmProblem& p) {
  const int run = tile_runs(cfg, p);
  return mmad_gemm_ntiles(run, p.Mp, p.Np) <=
         kernel_capacity(kernel_for(p.dtype, p.epi, run, false), TILES[run].NT);
}

bool mmad_gemm_bn_fusable(int dtype, int epi, int Mp, int Np) {
  if (Mp % 128 || Np % 128 || Np / 64 > MMAD_BN_EXIT) return false;
  const GemmProblem p{dtype, epi, Mp, Np, 1, true, false, MMAD_ACT_NONE};
  for (int c = 0; c < NCFG; ++c)
    if (tile_allowed(c, p) && coresident(c, p)) return true;
  return false;
}

// launch the kernel of `cfg` (a tile_runs result) for `p`
static int launch_tile(const GemmProblem& p, int cfg, const void* A, int lda, const void* B, int ldb, int K,
                       const GemmEpi& ep_in, hipStream_t s) {
  const Tile& t = TILES[cfg];
  const int tiles_m = p.Mp / t.BM, tiles_n = p.Np / t.BN, ntiles = tiles_m * tiles_n;
  GemmEpi ep = ep_in;
  ep.tiles_n = tiles_n;
  ep.group_m = plan_group_m(ntiles, tiles_m, t.BM, t.BN);
  const void* fn = kernel_for(p.dtype, p.epi, cfg, false);
  int grid = ntiles * p.splitk;
  if (!fn) {
    mmad_set_error("gemm: tile configuration %d does not support this dtype / epilogue", cfg);
    return MMAD_EUNSUPPORTED;
  }
  // persistent grid: forward-type bf16 epilogues without a fused BN or a
  // split, when the tiles exceed one resident round (knob 12: any nonzero
  // value; with fewer tiles the ordinary grid is the same launch)
  if (mmad_persist_override() != 0 && p.splitk == 1 && !p.fused_bn && t.persist) {
    const void* pfn = kernel_for(p.dtype, p.epi, cfg, true);
    const int cap = kernel_capacity(pfn, t.NT) & ~7;
    if (cap > 0 && ntiles > cap) {
      ep.persist_tiles = ntiles;
      fn = pfn;
      grid = cap;
    }
  }
  void* args[] = {&A, &lda, &B, &ldb, &K, &ep};
  return mmad_gemm_launch(fn, dim3(grid), dim3(t.NT), s, ep.start_ev, ep.done_ev, args);
}

// ---- autotune: time every fitting tile config once per problem shape -------
namespace {
struct TuneKey {
  int dtype, epi, Mp, Np, K, bnf;
  bool operator<(const TuneKey& o) const {
    const int a[6] = {dtype, epi, Mp, Np, K, bnf}, b[6] = {o.dtype, o.epi, o.Mp, o.Np, o.K, o.bnf};
    for (int i = 0; i < 6; ++i)
      if (a[i] != b[i]) return a[i] < b[i];
    return false;
  }
};
std::mutex g_tune_mu;
std::map<TuneKey, int> g_tune;
}  // namespace

template <typename Pred>
static int tune_cfg(const GemmProblem& p, Pred allowed, const void* A, int lda, const void* B, int ldb, int K,
                    const GemmEpi& ep, hipStream_t s, int* out_cfg) {
  // the trial launches must be side-effect free beyond the outputs the real
  // launch rewrites: no fused Adam while timing
  GemmEpi et = ep;
  et.done_ev = nullptr;   // the real launch below completes the caller's event
  et.start_ev = nullptr;
  et.ad_p = nullptr;
  et.sm_p = nullptr;
  et.bn_rmean = nullptr;   // fused BN: no running-statistics update while timing
  et.bn_rvar = nullptr;
  hipEvent_t e0, e1;
  MMAD_HIP_CHECK(hipEventCreate(&e0));
  MMAD_HIP_CHECK(hipEventCreate(&e1));
  int best = -1;
  float best_ms = 1e30f;
  int rc = MMAD_OK;
  for (int c = 0; c < NCFG && rc == MMAD_OK; ++c) {
    if (!allowed(c)) continue;
    if (c == CFG_B4) continue;   // the 4-wave tile: forced only (measured slower)
    const int run = tile_runs(c, p);
    rc = launch_tile(p, run, A, lda, B, ldb, K, et, s);   // warm
    if (rc != MMAD_OK) break;
    float ms = 0.f;
    hipError_t e = hipEventRecord(e0, s);
    for (int r = 0; r < 3 && rc == MMAD_OK && e == hipSuccess; ++r)
      rc = launch_tile(p, run, A, lda, B, ldb, K, et, s);
    if (rc != MMAD_OK) break;
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) {
      mmad_set_error("gemm autotune: HIP error %d (%s)", (int)e, hipGetErrorString(e));
      rc = MMAD_EHIP;
      break;
    }
    if (ms < best_ms) { best_ms = ms; best = c; }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != MMAD_OK) return rc;
  if (best < 0) {
    mmad_set_error("gemm autotune: no tile configuration fits (Mp=%d Np=%d epi=%d)", p.Mp, p.Np, p.epi);
    return MMAD_EUNSUPPORTED;
  }
  *out_cfg = best;
  return MMAD_OK;
}

// split factor for a shape (1, 2, 4, 8 or 16): a function of the shape and
// the epilogue only, so every tile configuration of a shape accumulates over
// K in the same order
int mmad_gemm_splitk(int Mp, int Np, int K, int dtype, int epi) {
  const int bk = dtype == MMAD_BF16 ? 64 : 32;            // K per stage
  const int t128 = (Mp / 128) * (Np / 128);              // 128x128 output tiles
  const int t64 = (Mp / 64) * (Np / 64);                 // 64x64 output tiles
  // workspace bounds (mmad_gemm_splitk_bytes): S * t128 <= MMAD_SK_SLAB_TILES slab tiles,
  // (1 + S) control words per tile of the smallest configuration
  auto ok = [&](int S) {
    return K % (S * bk) == 0 && K / S >= 4 * bk && S * t128 <= MMAD_SK_SLAB_TILES && t64 * (1 + S) < MMAD_SK_ERR_WORD;
  };
  auto valid = [](int S) { return S == 1 || S == 2 || S == 4 || S == 8 || S == 16; };
  const int env = mmad_splitk_override();
  if (valid(env)) return ok(env) ? env : 1;
  // the exact-fp32 parity path keeps one sequential K order per output (the
  // order closest to the reference's; a different fp32 order can flip the
  // LeakyReLU branch of a pre-activation at rounding level, e.g. 5.6e-7 in
  // tests/golden/mm192.npz); split-K is the bf16 performance path's -- except,
  // behind knob 32, the fp32 dW GEMMs of large batches: a gradient feeds no
  // branch, and contracting over >= 2048 rows the narrow layers' few 64x64
  // tiles run one f32-MFMA K loop each at 1/16 of the bf16 rate
  if (dtype != MMAD_BF16) {
    const int target = mmad_splitk_dw_f32_blocks();
    if (epi != GEMM_EPI_BWD_WEIGHT || target <= 0 || K < 2048) return 1;
    int best = 1;
    for (int S = 2; S <= 16; S *= 2)
      if (ok(S) && t64 * S <= target && K / S >= 16 * bk) best = S;
    return best;
  }
  if (epi == GEMM_EPI_BWD_WEIGHT) {
    const int envw = mmad_splitk_dw_override();
    if (valid(envw)) return ok(envw) ? envw : 1;
    // dW = dz^T a contracts over the batch: the narrow layers have few
    // output tiles and a long K loop.  Split until the launch has about
    // SK_DW_BLOCKS 64x64-tile blocks, keeping >= SK_DW_MIN_STAGES K stages
    // per slice (tools/splitk_sweep.py, profiles/r02*_splitk_dw*.log)
    const int target = mmad_splitk_dw_blocks(), min_st = mmad_splitk_dw_min_stages();
    int best = 1;
    for (int S = 2; S <= 16; S *= 2)
      if (ok(S) && t64 * S <= target && K / S >= min_st * bk) best = S;
    return best;
  }
  // forward / bwd-data at the bench shapes (B=1024, widths 2048..100): the
  // in-launch combine (slab round trip + ticket) costs more than the extra
  // CUs buy back, so no split; the override keeps the others reachable
  return 1;
}

// shape-independent bound: S * Mp * Np <= MMAD_SK_SLAB_TILES * 128 * 128 slab
// floats (832: split-K 4 of c2's largest forward / bwd-data GEMMs at 128x128);
// per launch (1 + S) control words per 64x64 tile < MMAD_SK_ERR_WORD
void mmad_gemm_splitk_bytes(int Mp, int Np, size_t* slab_bytes, size_t* ctl_bytes) {
  (void)Mp;
  (void)Np;
  if (slab_bytes) *slab_bytes = (size_t)MMAD_SK_SLAB_TILES * 128 * 128 * 4;
  if (ctl_bytes) *ctl_bytes = (size_t)(MMAD_SK_ERR_WORD + 1) * 4;
}

int mmad_gemm_read_status(unsigned* ctl, hipStream_t s, const char* who) {
  if (!ctl) return MMAD_OK;
  unsigned word = 0;
  MMAD_HIP_CHECK(hipMemcpyAsync(&word, ctl + MMAD_SK_ERR_WORD, sizeof(word), hipMemcpyDeviceToHost, s));
  MMAD_HIP_CHECK(hipStreamSynchronize(s));
  if (word == 0) return MMAD_OK;
  // a slice that gave up may still have raised its flag after the combine
  // cleared it: every launch of the failed one has finished now (stream
  // synchronised), so re-zero the whole control block for the next launch
  size_t slab = 0, ctl_bytes = 0;
  mmad_gemm_splitk_bytes(0, 0, &slab, &ctl_bytes);
  MMAD_HIP_CHECK(hipMemsetAsync(ctl, 0, ctl_bytes, s));
  MMAD_HIP_CHECK(hipStreamSynchronize(s));
  mmad_set_error("%s: a split-K GEMM combine timed out waiting for a slice; its output tiles were "
                 "not written (results invalid)", who);
  return MMAD_EHIP;
}

int mmad_gemm_plan(int Mp, int Np, int K, int epi, int dtype) {
  // the plain problem of the shape: no split, fused BN, partials or activation
  const GemmProblem p{dtype, epi, Mp, Np, 1, false, false, MMAD_ACT_NONE};
  auto allowed = [&](int c) { return tile_allowed(c, p); };
  int cfg = mmad_tile_override();
  if (!allowed(cfg)) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tune.find(TuneKey{dtype, epi, Mp, Np, K, 0});
    cfg = it != g_tune.end() ? it->second : heuristic_cfg(Mp, Np, allowed);
  }
  return cfg < 0 ? cfg : tile_runs(cfg, p);
}

int mmad_gemm_dispatch(int dtype, int epi, const void* A, int lda, const void* B, int ldb, int Mp,
                       int Np, int K, const GemmEpi& ep_in, hipStream_t s, int* cfg_used) {
  MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && K % 128 == 0,
                 "gemm: padded dims must be multiples of 128 (Mp=%d Np=%d K=%d)", Mp, Np, K);
  MMAD_CHECK_ARG(Mp > 0 && Np > 0 && K > 0, "gemm: empty problem");
  if (dtype == MMAD_BF16X3) {
    // its own kernel and single tile (mmad_gemm_x3.hip): no plan, no tuning
    GemmEpi ex = ep_in;
    ex.dbg = 0;
    if (cfg_used) *cfg_used = 0;
    return mmad_gemm_x3_dispatch(epi, A, lda, B, ldb, Mp, Np, K, ex, s);
  }
  MMAD_CHECK_ARG(dtype == MMAD_BF16 || dtype == MMAD_F32, "gemm: bad dtype %d", dtype);
  MMAD_CHECK_ARG(epi >= GEMM_EPI_FWD && epi <= GEMM_EPI_SCORE, "gemm: bad epilogue %d", epi);
  GemmEpi ep = ep_in;
  ep.dbg = mmad_dbg_override();
  const bool bnf = ep.bn_sync != nullptr;
  MMAD_CHECK_ARG(!bnf || epi == GEMM_EPI_FWD || epi == GEMM_EPI_BWD_DATA,
                 "gemm: fused BN only for the forward / bwd-data epilogues");
  MMAD_CHECK_ARG(!bnf || Np / 64 <= MMAD_BN_EXIT, "gemm: fused BN: Np=%d too wide", Np);
  // the fused BN barrier needs one block per output tile (no split) and the
  // whole grid resident
  ep.splitk = (ep.sk_slab && ep.sk_ctl && !bnf) ? mmad_gemm_splitk(Mp, Np, K, dtype, epi) : 1;
  const GemmProblem p{dtype, epi, Mp, Np, ep.splitk, bnf, ep.part || ep.bpart, ep.act};
  auto allowed = [&](int c) { return tile_allowed(c, p) && (!bnf || coresident(c, p)); };
  const int env = mmad_tile_override();
  const int env_epi = ep.ad_p ? mmad_tile_adam_for(Mp, Np, K) : mmad_tile_epi_override(epi);
  int cfg;
  const int force = ep.tile_force - 1;
  if (allowed(force)) {
    cfg = force;
  } else if (allowed(env_epi)) {
    cfg = env_epi;
  } else if (allowed(env)) {
    cfg = env;   // forced tile (tuning / tests); a shape it does not fit falls through
  } else {
    const TuneKey key{dtype, epi, Mp, Np, K, bnf ? 1 : 0};
    int found = -1;
    {
      std::lock_guard<std::mutex> lk(g_tune_mu);
      auto it = g_tune.find(key);
      if (it != g_tune.end()) found = it->second;
    }
    if (found >= 0) {
      cfg = found;
    } else {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(s, &cs);
      if (mmad_autotune_enabled() && cs == hipStreamCaptureStatusNone) {
        int rc = tune_cfg(p, allowed, A, lda, B, ldb, K, ep, s, &cfg);
        if (rc != MMAD_OK) return rc;
      } else {
        cfg = heuristic_cfg(Mp, Np, allowed);
        if (cfg < 0) {
          mmad_set_error("gemm: no co-resident tile configuration for the fused BN epilogue "
                         "(Mp=%d Np=%d)", Mp, Np);
          return MMAD_EUNSUPPORTED;
        }
      }
      std::lock_guard<std::mutex> lk(g_tune_mu);
      g_tune[key] = cfg;
    }
  }
  const int run = tile_runs(cfg, p);
  if (cfg_used) *cfg_used = run;
  return launch_tile(p, run, A, lda, B, ldb, K, ep, s);
}

// ---- the grouped dW launch ------------------------------------------------
static const void* group_kernel(int dtype) {
  return dtype == MMAD_BF16 ? (const void*)mmad_gemm_group_kernel<bf16>
         : dtype == MMAD_F32 ? (const void*)mmad_gemm_group_kernel<float> : nullptr;
}

int mmad_gemm_group_capacity(int dtype) { return kernel_capacity(group_kernel(dtype), TILES[3].NT); }

// the tile a stand-alone dispatch of this member would take without consulting
// the tuner (-1: it would), by mmad_gemm_dispatch's own order of precedence
static int group_member_tile(const GemmProblem& p, const GemmEpi& ep, int K) {
  const int cand[3] = {ep.tile_force - 1,
                       ep.ad_p ? mmad_tile_adam_for(p.Mp, p.Np, K) : mmad_tile_epi_override(p.epi),
                       mmad_tile_override()};
  for (int c : cand)
    if (tile_allowed(c, p)) return tile_runs(c, p);
  return -1;
}

int mmad_gemm_dispatch_group(int dtype, int n, const GemmGroupProblem* problems, hipStream_t s,
                             hipEvent_t done_ev, hipEvent_t start_ev) {
  MMAD_CHECK_ARG(n > 0 && problems, "gemm group: empty group");
  const void* fn = group_kernel(dtype);
  if (n > MMAD_GEMM_GROUP_MAX || !fn) return MMAD_GEMM_GROUP_REFUSED;
  GemmGroupTable g{};
  g.n = n;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    const GemmGroupProblem& q = problems[i];
    MMAD_CHECK_ARG(q.Mp > 0 && q.Np > 0 && q.K > 0 && q.Mp % 128 == 0 && q.Np % 128 == 0 && q.K % 128 == 0,
                   "gemm group: padded dims must be multiples of 128 (Mp=%d Np=%d K=%d)", q.Mp, q.Np, q.K);
    const int S = (q.ep.sk_slab && q.ep.sk_ctl) ? mmad_gemm_splitk(q.Mp, q.Np, q.K, dtype, GEMM_EPI_BWD_WEIGHT) : 1;
    const GemmProblem p{dtype, GEMM_EPI_BWD_WEIGHT, q.Mp, q.Np, S, false, false, q.ep.act};
    if (S != 1 || q.ep.bn_sync || group_member_tile(p, q.ep, q.K) != 3) return MMAD_GEMM_GROUP_REFUSED;
    const Tile& t = TILES[3];
    const int tiles_m = q.Mp / t.BM, tiles_n = q.Np / t.BN, ntiles = tiles_m * tiles_n;
    GemmGroupEntry& e = g.e[i];
    e.A = q.A;
    e.B = q.B;
    e.lda = q.lda;
    e.ldb = q.ldb;
    e.K = q.K;
    e.first_block = blocks;
    e.ntiles = ntiles;
    // the member's epilogue as launch_tile would pass it
    e.ep = q.ep;
    e.ep.dbg = mmad_dbg_override();
    e.ep.splitk = 1;
    e.ep.tiles_n = tiles_n;
    e.ep.group_m = plan_group_m(ntiles, tiles_m, t.BM, t.BN);
    e.ep.done_ev = nullptr;
    e.ep.start_ev = nullptr;
    blocks += mmad_gemm_group_blocks(q.Mp, q.Np);
  }
  const int cap = kernel_capacity(fn, TILES[3].NT);
  if (cap <= 0 || blocks > cap) return MMAD_GEMM_GROUP_REFUSED;
  void* args[] = {&g};
  return mmad_gemm_launch(fn, dim3(blocks), dim3(TILES[3].NT), s, start_ev, done_ev, args);
}
