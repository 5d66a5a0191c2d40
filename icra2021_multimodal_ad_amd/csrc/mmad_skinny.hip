// Weight-streaming layer operator for at most 16 valid rows (mmad_fc_rows16)
// or at most 64 (mmad_fc_rows64) -- one kernel, skinny_k<T, RT>, behind both --
// and the small kernels of the online scoring pass (mmad_ae_online_score /
// _score64, mmad_ae_online.hip).
//
// y[rows][N] = epi(x[rows][K] . W[N][K]^T); rows = 16 or 64 is the packed row
// capacity of every buffer, M <= rows of them are valid.  The work is one pass
// over W, so the kernel is built as a weight stream, not as a GEMM tile.  One
// block per 16 output columns; its waves split K in interleaved chunks (wave w
// takes chunks w, w + NW, ...: the block's loads stay contiguous along each
// weight row); every lane loads its MFMA B fragment straight from global
// memory with 16-byte loads, a chunk (4 loads of W, 4 of each row tile of x)
// ahead of the MFMAs that consume it, and W never passes through LDS.
//
// RT = ceil(M / 16) row tiles (the instantiation, 1..4) ride one weight
// stream: a lane loads a chunk's W fragments once and issues one MFMA group
// per row tile, each with its own A fragments (rows 16 t + (lane & 15) of x)
// and its own accumulator.  A row's accumulator sees the same products in the
// same order whatever RT and rows are, so a row's bits are equal through both
// entry points, by construction.  Row tiles >= RT are neither loaded nor
// computed; their rows below `rows` are written as zero and nothing at or past
// row `rows` is touched.  The waves' 16x16 fp32 accumulators meet in LDS; wave
// t adds tile t's in wave order and runs its epilogue (waves beyond NW take
// t + NW, ...): no atomics, no split-K slab, no barrier between blocks, so a
// launch's bits depend on nothing but its operands.
// ROWS (= MmadSkinny::rows) enters only the addressing -- the epilogue's tile
// loop and the rowsq index -- and is a template argument because as a runtime
// value it cost 2..4 VGPRs (DESIGN.md "Online scoring"); a 16-row call only
// ever launches RT = 1, so ten instantiations: two dtypes x (1 + 4).
// Packed layouts: x [rows][Kp], y [rows][Np], diff [rows][lddiff],
// rowsq [Np/16][rows].
//
// Fragment maps (gfx950):
//   v_mfma_f32_16x16x32_bf16: lane l holds k = 8 (l >> 4) .. + 7 of row / column
//     l & 15 -- one 16-byte load per operand.
//   v_mfma_f32_16x16x4_f32: lane l holds ONE k (l >> 4) of row / column l & 15.
//     A lane loads 4 consecutive k (16 bytes) and MFMA j takes element j of
//     both operands' quads: k = 4 (l >> 4) + j of the 16-k step -- the same
//     products as the natural order, summed in another, fixed order.
//   C/D (both): column l & 15, rows 4 (l >> 4) + reg.
#include <type_traits>

#include "mmad_common.h"
#include "mmad_ops.h"

// waves per block and the weight loads' cache policy: compile-time constants
// (DESIGN.md "Online scoring" has the measurements behind them)
#ifndef MMAD_SKINNY_WAVES
#define MMAD_SKINNY_WAVES 4
#endif
#ifndef MMAD_SKINNY_NT
#define MMAD_SKINNY_NT 0
#endif

namespace {

constexpr int NW = MMAD_SKINNY_WAVES;
constexpr int U = 4;   // 16-byte loads per operand and chunk

template <typename T> struct Frag;
template <> struct Frag<bf16> { typedef bf16x8 V; static constexpr int KL = 8; };
template <> struct Frag<float> { typedef floatx4 V; static constexpr int KL = 4; };

template <typename V> __device__ __forceinline__ V load_w(const V* p) {
#if MMAD_SKINNY_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

template <int RT>
__device__ __forceinline__ void mma(floatx4 (&acc)[RT], const bf16x8 (&a)[RT][U], const bf16x8 (&b)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][u], b[u], acc[t], 0, 0, 0);
}
template <int RT>
__device__ __forceinline__ void mma(floatx4 (&acc)[RT], const floatx4 (&a)[RT][U], const floatx4 (&b)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < RT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][u][j], b[u][j], acc[t], 0, 0, 0);
}

// one block's work: the 16 output columns of tile `tile` of a (the body of
// skinny_k, and of skinny_group_k for the member the block belongs to)
template <typename T, int RT, int ROWS>
__device__ __forceinline__ void skinny_tile(const MmadSkinny& a, const int tile) {
  typedef typename Frag<T>::V V;
  constexpr int KL = Frag<T>::KL;   // k per lane and load
  constexpr int CK = 4 * KL * U;    // k per chunk: 128 (bf16) / 64 (fp32) = 256 bytes of a row
  __shared__ floatx4 red[NW][RT][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int n0 = tile * 16;
  const T* wp = (const T*)a.w + (size_t)(n0 + c16) * a.Kp + g * KL;
  const T* xp = (const T*)a.x + (size_t)c16 * a.Kp + g * KL;
  const size_t xt = (size_t)16 * a.Kp;   // one row tile of x
  const int nch = a.Kp / CK;
  floatx4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  V bw[U], ax[RT][U];
  int c = wv;
  if (c < nch) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bw[u] = load_w((const V*)(wp + (size_t)c * CK + u * 4 * KL));
#pragma unroll
      for (int t = 0; t < RT; ++t) ax[t][u] = *(const V*)(xp + t * xt + (size_t)c * CK + u * 4 * KL);
    }
  }
  while (c < nch) {
    V bn[U], an[RT][U];
    const int cn = c + NW;
    const bool more = cn < nch;   // wave-uniform
    if (more) {   // the next chunk's loads fly over this chunk's MFMAs
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bn[u] = load_w((const V*)(wp + (size_t)cn * CK + u * 4 * KL));
#pragma unroll
        for (int t = 0; t < RT; ++t) an[t][u] = *(const V*)(xp + t * xt + (size_t)cn * CK + u * 4 * KL);
      }
    }
    mma<RT>(acc, ax, bw);
    if (!more) break;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bw[u] = bn[u];
#pragma unroll
      for (int t = 0; t < RT; ++t) ax[t][u] = an[t][u];
    }
    c = cn;
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) red[wv][t][lane] = acc[t];
  __syncthreads();

  // ---- epilogue of row tile t: column n, rows 16 t + 4 g + r
  const int n = n0 + c16;
  const bool nv = n < a.N;
  const float b = a.bias ? a.bias[n] : 0.f;
  const float sc = a.scale ? a.scale[n] : 1.f;
  const float sh = a.shift ? a.shift[n] : 0.f;
  const float cw = a.colw ? a.colw[n] : 1.f;
  for (int t = wv; 16 * t < ROWS; t += NW) {   // wave-uniform
    floatx4 s = {0.f, 0.f, 0.f, 0.f};   // tiles >= RT: every row is >= M
    if (t < RT) {
      s = red[0][t][lane];
#pragma unroll
      for (int w = 1; w < NW; ++w) s += red[w][t][lane];
    }
    float sq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * t + 4 * g + r;
      const bool valid = nv && m < a.M;
      float v = apply_act(s[r] + b, a.act, a.slope);
      if (a.scale) v = v * sc + sh;
      v = valid ? v : 0.f;
      if (a.y) ((T*)a.y)[(size_t)m * a.Np + n] = from_f32<T>(v);
      sq[r] = 0.f;
      if (a.rowsq) {
        float rf = 0.f;
        if (a.ref && valid)
          rf = a.ref_f32 ? ((const float*)a.ref)[(size_t)m * a.ldref + n]
                         : to_f32<T>(((const T*)a.ref)[(size_t)m * a.ldref + n]);
        const float d = v - rf;   // invalid: 0 - 0
        if (a.diff && nv) a.diff[(size_t)m * a.lddiff + n] = d;
        sq[r] = d * d * cw;
      }
    }
    if (a.rowsq) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sq[r] += __shfl_xor(sq[r], o);
        if (c16 == 0) a.rowsq[(size_t)tile * ROWS + 16 * t + 4 * g + r] = sq[r];
      }
    }
  }
}

template <typename T, int RT, int ROWS>
__global__ __launch_bounds__(NW * 64) void skinny_k(const MmadSkinny a) {
  skinny_tile<T, RT, ROWS>(a, blockIdx.x);
}

// mmad_fc_rows_group: the members of one element type in one grid.  Member i
// owns the blocks [first[i], first[i + 1]) -- its 16-column tiles in order;
// the walk over the table is block-uniform, the member's arguments are scalar
// loads from the kernel arguments
struct SkinnyGroup {
  int n;
  int first[MMAD_MAX_BANK + 1];
  MmadSkinny m[MMAD_MAX_BANK];
};
template <typename T, int RT, int ROWS>
__global__ __launch_bounds__(NW * 64) void skinny_group_k(const SkinnyGroup g) {
  const int b = blockIdx.x;
  if (b >= g.first[g.n]) return;
  int i = 0;
  while (b >= g.first[i + 1]) ++i;
  skinny_tile<T, RT, ROWS>(g.m[i], b - g.first[i]);
}

// eval-BN (scale, shift) of one BN element: j of the [n_bn] running-stat
// layout, its layer found among the n layers of (bn_off, N, g_off, be_off)
__device__ __forceinline__ void fold_elem(const int j, const int n, const int n_bn, const int* bn_off,
                                          const int* N, const int64_t* g_off, const int64_t* be_off,
                                          const float* __restrict__ params, const float* __restrict__ running,
                                          const float eps, float* __restrict__ scale, float* __restrict__ shift) {
  int i = 0;
  while (i + 1 < n && j >= bn_off[i + 1]) ++i;
  const int c = j - bn_off[i];
  float s = 0.f, t = 0.f;
  if (c < N[i]) {
    s = params[g_off[i] + c] * (float)(1.0 / sqrt((double)running[n_bn + j] + (double)eps));
    t = params[be_off[i] + c] - running[j] * s;
  }
  scale[j] = s;
  shift[j] = t;
}

// eval-BN (scale, shift) of every BN layer in one grid (mmad_bn_eval_affine
// per layer): element j of the [n_bn] running-stat layout
__global__ __launch_bounds__(256) void online_fold_k(const MmadOnlineFold f, const float* __restrict__ params,
                                                     const float* __restrict__ running, float eps,
                                                     float* __restrict__ scale, float* __restrict__ shift) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= f.n_bn) return;
  fold_elem(j, f.n, f.n_bn, f.bn_off, f.N, f.g_off, f.be_off, params, running, eps, scale, shift);
}

// ... of every member of a bank: blk[i] .. blk[i + 1] are member i's blocks
struct FoldGroupBlocks { int blk[MMAD_MAX_BANK + 1]; };
__global__ __launch_bounds__(256) void online_fold_group_k(const MmadOnlineFoldGroup g, const FoldGroupBlocks p) {
  const int b = blockIdx.x;
  if (b >= p.blk[g.n]) return;
  int i = 0;
  while (b >= p.blk[i + 1]) ++i;
  const MmadOnlineFoldMember& m = g.m[i];
  const int j = (b - p.blk[i]) * 256 + threadIdx.x;
  if (j >= m.n_bn) return;
  const int l0 = g.first[i];
  fold_elem(j, g.first[i + 1] - l0, m.n_bn, g.bn_off + l0, g.N + l0, g.g_off + l0, g.be_off + l0, m.params,
            m.running, m.eps, m.scale, m.shift);
}

// one block of 512: the row partials summed in tile order (left to right, 8
// loads at a time, per (layer, row)), then BASE / SAP / NAP and flags.
// rs [tiles][ROWS], out [n_diff + 3][ROWS], flags [3][ROWS]
template <int ROWS>
__device__ __forceinline__ void online_finish_body(const MmadOnlineFinish& f) {
  __shared__ float lsq[MMAD_ONLINE_MAX_DIFF + 1][ROWS];
  const int b = threadIdx.x % ROWS;
  for (int j = threadIdx.x / ROWS; j < f.n_diff + (f.nap_rs ? 1 : 0); j += 512 / ROWS) {
    const float* p = j < f.n_diff ? f.rs[j] : f.nap_rs;
    const int nt = j < f.n_diff ? f.tiles[j] : f.nap_tiles;
    float s = 0.f;
    int t = 0;
    for (; t + 8 <= nt; t += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(t + u) * ROWS + b];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; t < nt; ++t) s += p[(size_t)t * ROWS + b];
    lsq[j][b] = s;
  }
  __syncthreads();
  if (threadIdx.x >= ROWS || b >= f.B) return;
  float* out = f.out;
  for (int l = 0; l < f.n_diff; ++l) out[l * ROWS + b] = lsq[l][b];
  const float base = lsq[0][b] / (float)f.widths[0];
  float ss = 0.f;
  int wsum = 0;
  for (int l = f.sap_start; l < f.sap_end; ++l) {
    ss += lsq[l][b];
    wsum += f.widths[l];
  }
  const float sap = ss / (float)wsum;
  out[f.n_diff * ROWS + b] = base;
  out[(f.n_diff + 1) * ROWS + b] = sap;
  float nap = 0.f;
  if (f.nap_rs) {
    nap = lsq[f.n_diff][b] * f.nap_scale;
    out[(f.n_diff + 2) * ROWS + b] = nap;
  }
  if (f.flags) {
    // strict >: get_f1_score's prediction rule; a NaN threshold compares false
    const float* th = f.thresholds;
    f.flags[b] = th ? (uint8_t)(base > th[0]) : 0;
    f.flags[ROWS + b] = th ? (uint8_t)(sap > th[1]) : 0;
    f.flags[2 * ROWS + b] = (th && f.nap_rs) ? (uint8_t)(nap > th[2]) : 0;
  }
}
template <int ROWS>
__global__ __launch_bounds__(512) void online_finish_k(const MmadOnlineFinish f) {
  online_finish_body<ROWS>(f);
}
// one block per member of a bank
struct FinishGroup { MmadOnlineFinish f[MMAD_MAX_BANK]; };
template <int ROWS>
__global__ __launch_bounds__(512) void online_finish_group_k(const FinishGroup g) {
  online_finish_body<ROWS>(g.f[blockIdx.x]);
}

// the one choice of instantiation, for both kernel families: f(RT, ROWS) as
// integral constants, RT = the row tiles the M valid rows take (M <= rows: a
// 16-row call only ever takes RT = 1)
template <int V> using Int = std::integral_constant<int, V>;
template <class F>
void with_tiles(int rows, int M, F f) {
  if (rows == 16) return f(Int<1>{}, Int<16>{});
  switch ((M + 15) / 16) {
    case 1: return f(Int<1>{}, Int<64>{});
    case 2: return f(Int<2>{}, Int<64>{});
    case 3: return f(Int<3>{}, Int<64>{});
    default: return f(Int<4>{}, Int<64>{});
  }
}

template <typename T>
void launch(const MmadSkinny& a, hipStream_t s) {
  with_tiles(a.rows, a.M, [&](auto rt, auto rows) {
    skinny_k<T, decltype(rt)::value, decltype(rows)::value><<<dim3(a.Np / 16), dim3(NW * 64), 0, s>>>(a);
  });
}

// the members of element type T (mask bit i) as one launch, all on RT row tiles
template <typename T>
void launch_group(int rows, int n, unsigned mask, const MmadSkinny* a, hipStream_t s) {
  SkinnyGroup g{};
  int maxM = 1;
  for (int i = 0; i < n; ++i) {
    g.first[i + 1] = g.first[i];
    if (!(mask >> i & 1)) continue;
    g.m[i] = a[i];
    g.first[i + 1] += a[i].Np / 16;
    maxM = a[i].M > maxM ? a[i].M : maxM;
  }
  g.n = n;
  with_tiles(rows, maxM, [&](auto rt, auto rw) {
    skinny_group_k<T, decltype(rt)::value, decltype(rw)::value><<<dim3(g.first[n]), dim3(NW * 64), 0, s>>>(g);
  });
}

// every refusal of the operator, nothing launched
int skinny_check(int dtype, const MmadSkinny& a) {
  const int R = a.rows;
  MMAD_CHECK_ARG(R == 16 || R == 64, "fc_rows: rows=%d (16 or 64)", R);
  MMAD_CHECK_ARG(dtype == MMAD_F32 || dtype == MMAD_BF16, "fc_rows%d: dtype %d (MMAD_F32 or MMAD_BF16)", R, dtype);
  MMAD_CHECK_ARG(a.M >= 1 && a.M <= R, "fc_rows%d: M=%d outside 1..%d", R, a.M, R);
  MMAD_CHECK_ARG(a.N >= 1 && a.N <= a.Np && a.Np % 16 == 0 && a.Kp >= MMAD_PAD && a.Kp % MMAD_PAD == 0,
                 "fc_rows%d: bad sizes N=%d Np=%d Kp=%d (Np a multiple of 16, Kp of %d)", R, a.N, a.Np, a.Kp,
                 MMAD_PAD);
  MMAD_CHECK_ARG(a.x && a.w && ((uintptr_t)a.x | (uintptr_t)a.w) % 16 == 0,
                 "fc_rows%d: x and w must be non-null and 16-byte aligned", R);
  MMAD_CHECK_ARG(a.y || a.rowsq, "fc_rows%d: neither y nor rowsq to write", R);
  MMAD_CHECK_ARG(a.rowsq || (!a.ref && !a.diff && !a.colw), "fc_rows%d: ref / diff / colw need rowsq", R);
  if (a.act < MMAD_ACT_NONE || a.act > MMAD_ACT_TANH) {
    mmad_set_error("fc_rows%d: activation %d has no per-element epilogue", R, a.act);
    return MMAD_EUNSUPPORTED;
  }
  return MMAD_OK;
}

// the C-ABI arguments' own refusals (mmad_fc_rows16 / 64, a descriptor of
// mmad_fc_rows_group), then MmadSkinny
int fc_rows_args(int rows, int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
                 const float* bias, int act, float slope, const float* bn_scale, const float* bn_shift, void* y,
                 const void* ref, int ref_dtype, int ldref, float* diff, int lddiff, const float* colw,
                 float* rowsq, MmadSkinny& a) {
  MMAD_CHECK_ARG(K >= 1 && K <= Kp, "fc_rows%d: K=%d outside 1..Kp=%d", rows, K, Kp);
  MMAD_CHECK_ARG(!bn_scale == !bn_shift, "fc_rows%d: bn_scale and bn_shift go together", rows);
  MMAD_CHECK_ARG(!ref || ((ref_dtype == MMAD_F32 || ref_dtype == dtype) && ldref >= N),
                 "fc_rows%d: ref is fp32 or the operand dtype, ldref >= N", rows);
  MMAD_CHECK_ARG(!diff || lddiff >= N, "fc_rows%d: lddiff < N", rows);
  a = MmadSkinny{};
  a.rows = rows; a.M = M; a.N = N; a.Np = Np; a.Kp = Kp;
  a.x = x; a.w = w; a.bias = bias; a.act = act; a.slope = slope;
  a.scale = bn_scale; a.shift = bn_shift; a.y = y;
  a.ref = ref; a.ref_f32 = ref_dtype == MMAD_F32; a.ldref = ldref;
  a.diff = diff; a.lddiff = lddiff; a.colw = colw; a.rowsq = rowsq;
  return MMAD_OK;
}

// mmad_fc_rows16 / mmad_fc_rows64
int fc_rows(int rows, int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
            const float* bias, int act, float slope, const float* bn_scale, const float* bn_shift, void* y,
            const void* ref, int ref_dtype, int ldref, float* diff, int lddiff, const float* colw,
            float* rowsq, void* stream) {
  MmadSkinny a;
  const int rc = fc_rows_args(rows, dtype, M, N, K, Np, Kp, x, w, bias, act, slope, bn_scale, bn_shift, y, ref,
                              ref_dtype, ldref, diff, lddiff, colw, rowsq, a);
  return rc != MMAD_OK ? rc : mmad_skinny_launch(dtype, a, stream);
}

}  // namespace

int mmad_skinny_launch(int dtype, const MmadSkinny& a, void* stream) {
  const int rc = skinny_check(dtype, a);
  if (rc != MMAD_OK) return rc;
  if (dtype == MMAD_BF16)
    launch<bf16>(a, (hipStream_t)stream);
  else
    launch<float>(a, (hipStream_t)stream);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_skinny_group_launch(int rows, int n, const int* dtype, const MmadSkinny* a, void* stream) {
  MMAD_CHECK_ARG(n >= 1 && n <= MMAD_MAX_BANK, "fc_rows_group: n=%d outside 1..%d", n, MMAD_MAX_BANK);
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "fc_rows_group: rows=%d (16 or 64)", rows);
  MMAD_CHECK_ARG(dtype && a, "fc_rows_group: null members");
  unsigned mask[2] = {0, 0};   // members by element type; N == 0: in neither
  for (int i = 0; i < n; ++i) {
    if (a[i].N == 0) continue;
    MMAD_CHECK_ARG(a[i].rows == rows, "fc_rows_group: member %d of %d rows in a call of %d", i, a[i].rows, rows);
    const int rc = skinny_check(dtype[i], a[i]);
    if (rc != MMAD_OK) return rc;
    mask[dtype[i] == MMAD_BF16] |= 1u << i;
  }
  if (mask[0]) launch_group<float>(rows, n, mask[0], a, (hipStream_t)stream);
  if (mask[1]) launch_group<bf16>(rows, n, mask[1], a, (hipStream_t)stream);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_fc_rows_group(int rows, int n, const mmad_fc_rows_desc* d, void* stream) {
  MMAD_CHECK_ARG(n >= 1 && n <= MMAD_MAX_BANK, "fc_rows_group: n=%d outside 1..%d", n, MMAD_MAX_BANK);
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "fc_rows_group: rows=%d (16 or 64)", rows);
  MMAD_CHECK_ARG(d, "fc_rows_group: null descriptors");
  MmadSkinny a[MMAD_MAX_BANK];
  int dt[MMAD_MAX_BANK];
  for (int i = 0; i < n; ++i) {
    const mmad_fc_rows_desc& m = d[i];
    a[i] = MmadSkinny{};
    dt[i] = m.dtype;
    if (m.N == 0) continue;
    const int rc = fc_rows_args(rows, m.dtype, m.M, m.N, m.K, m.Np, m.Kp, m.x, m.w, m.bias, m.act, m.slope,
                                m.bn_scale, m.bn_shift, m.y, m.ref, m.ref_dtype, m.ldref, m.diff, m.lddiff,
                                m.colw, m.rowsq, a[i]);
    if (rc != MMAD_OK) return rc;
  }
  return mmad_skinny_group_launch(rows, n, dt, a, stream);
}

int mmad_fc_rows16(int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
                   const float* bias, int act, float slope, const float* bn_scale, const float* bn_shift,
                   void* y, const void* ref, int ref_dtype, int ldref, float* diff, int lddiff,
                   const float* colw, float* rowsq, void* stream) {
  return fc_rows(16, dtype, M, N, K, Np, Kp, x, w, bias, act, slope, bn_scale, bn_shift, y, ref, ref_dtype,
                 ldref, diff, lddiff, colw, rowsq, stream);
}

int mmad_fc_rows64(int dtype, int M, int N, int K, int Np, int Kp, const void* x, const void* w,
                   const float* bias, int act, float slope, const float* bn_scale, const float* bn_shift,
                   void* y, const void* ref, int ref_dtype, int ldref, float* diff, int lddiff,
                   const float* colw, float* rowsq, void* stream) {
  return fc_rows(64, dtype, M, N, K, Np, Kp, x, w, bias, act, slope, bn_scale, bn_shift, y, ref, ref_dtype,
                 ldref, diff, lddiff, colw, rowsq, stream);
}

int mmad_online_fold(const MmadOnlineFold& f, const float* params, const float* running, float eps,
                     float* scale, float* shift, void* stream) {
  if (f.n_bn == 0) return MMAD_OK;
  online_fold_k<<<(f.n_bn + 255) / 256, 256, 0, (hipStream_t)stream>>>(f, params, running, eps, scale, shift);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_online_finish(const MmadOnlineFinish& f, int rows, void* stream) {
  MMAD_CHECK_ARG(f.n_diff >= 1 && f.n_diff <= MMAD_ONLINE_MAX_DIFF, "online_finish: %d diff layers", f.n_diff);
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "online_finish: rows=%d (16 or 64)", rows);
  if (rows == 16)
    online_finish_k<16><<<1, 512, 0, (hipStream_t)stream>>>(f);
  else
    online_finish_k<64><<<1, 512, 0, (hipStream_t)stream>>>(f);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_online_fold_group(const MmadOnlineFoldGroup& g, void* stream) {
  MMAD_CHECK_ARG(g.n >= 1 && g.n <= MMAD_MAX_BANK && g.first[g.n] <= MMAD_BANK_MAX_BN,
                 "online_fold_group: %d members, %d BatchNorm layers (at most %d, %d)", g.n,
                 g.n >= 1 && g.n <= MMAD_MAX_BANK ? g.first[g.n] : 0, MMAD_MAX_BANK, MMAD_BANK_MAX_BN);
  FoldGroupBlocks p{};
  for (int i = 0; i < g.n; ++i) p.blk[i + 1] = p.blk[i] + (g.m[i].n_bn + 255) / 256;
  if (p.blk[g.n] == 0) return MMAD_OK;
  online_fold_group_k<<<p.blk[g.n], 256, 0, (hipStream_t)stream>>>(g, p);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_online_finish_group(int n, const MmadOnlineFinish* f, int rows, void* stream) {
  MMAD_CHECK_ARG(n >= 1 && n <= MMAD_MAX_BANK && f, "online_finish_group: n=%d outside 1..%d", n, MMAD_MAX_BANK);
  MMAD_CHECK_ARG(rows == 16 || rows == 64, "online_finish_group: rows=%d (16 or 64)", rows);
  FinishGroup g{};
  for (int i = 0; i < n; ++i) {
    MMAD_CHECK_ARG(f[i].n_diff >= 1 && f[i].n_diff <= MMAD_ONLINE_MAX_DIFF,
                   "online_finish_group: member %d has %d diff layers", i, f[i].n_diff);
    g.f[i] = f[i];
  }
  if (rows == 16)
    online_finish_group_k<16><<<n, 512, 0, (hipStream_t)stream>>>(g);
  else
    online_finish_group_k<64><<<n, 512, 0, (hipStream_t)stream>>>(g);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}
