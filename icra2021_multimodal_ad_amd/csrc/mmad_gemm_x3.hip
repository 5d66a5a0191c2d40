// Split-bf16 ("x3") GEMM for the eval / score path on gfx950 (CDNA4).
//
// An fp32 operand x is stored as two bf16 planes, hi = bf16(x) and
// lo = bf16(x - hi) (MMAD_BF16X3, include/mmad.h).  The product is formed as
//   A.B^T ~= Ahi.Bhi^T + (Ahi.Blo^T + Alo.Bhi^T)
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: three bf16 MFMAs per
// fragment pair instead of the 16 quarter-rate f32 MFMAs of the exact path.
// The two cross terms have their own accumulator, added to the hi.hi one once
// in the epilogue (small terms first); lo.lo (<= 2^-18 of |a||b|) is dropped.
// Nothing is split in registers: the producers (mmad_split_planes, the pack
// kernel, this kernel's own epilogue) write both planes to HBM and the K loop
// only moves them global -> LDS -> MFMA (the in-register split
// made the round-10 probe VALU-bound).
//
// C[Mp][Np] = A[Mp][K] . B[Np][K]^T, both operands K-major (the only layouts
// the eval / score path uses).  One tile: 128x128, 512 threads (waves 2x4,
// wave tile 64x32), K stage = 64 (128 B per row and plane): the four panels
// A-hi, A-lo, B-hi, B-lo are 64 KB per stage, two stages in a ring.  Panels
// use the K-major LDS image of mmad_gemm_dev.h (16-byte chunk j of row r
// stored at j ^ ((r >> 1) & 7), filled by global_load_lds, read with one
// ds_read_b128 per fragment).  The MFMA operands are swapped (B first), so a
// lane's accumulator quad is 4 consecutive columns of one output row and the
// epilogue stores straight from registers: 8 B per plane, 16 B of fp32.
// The SCORE epilogue can also leave the fp32 diff as a plane pair inside a
// caller's packed x3 operand (GemmEpi::dp_hi: the streamed NAP operand).
// No split-K, no fused BN, no persistent grid; the K order is fixed, so the
// result bits do not depend on the grid order.
#include "mmad_common.h"
#include "mmad_gemm.h"

#include <hip/hip_ext.h>

#include <cmath>

namespace {

constexpr int X_BM = 128, X_BN = 128, X_BK = 64, X_NT = 512;
constexpr int X_WM = 2, X_WN = 4;
constexpr int X_TM = X_BM / X_WM / 16, X_TN = X_BN / X_WN / 16;   // 4 x 2 MFMA tiles per wave
constexpr int X_RB = 128;                        // bytes per LDS row (64 bf16)
constexpr int X_PANEL = X_BM * X_RB;             // 16 KB per plane panel
constexpr int X_SLOT = 4 * X_PANEL;              // A-hi | A-lo | B-hi | B-lo
constexpr int X_NS = 2;
constexpr int X_CHUNKS = X_PANEL / 16 / X_NT;    // global_load_lds per thread and panel
static_assert(X_BM == X_BN && X_CHUNKS * 16 * X_NT == X_PANEL, "panel / thread mismatch");
static_assert(X_NS * X_SLOT <= 163840, "LDS budget");

__device__ __forceinline__ int x_swz(int r) { return (r >> 1) & 7; }

// one 16-byte-per-lane LDS-DMA into the wave's 1 KiB at `dst` (wave-uniform);
// inline asm for the reason given at dma16 in mmad_gemm_dev.h
__device__ __forceinline__ void x_dma16(const void* src, char* dst) {
  const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(MMAD_LDS void*)dst);
  asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(src), "{m0}"(lds) : "memory");
}

// one stage of one plane panel: rows r0.. of G (K-major, ld elements), k0..k0+63
__device__ __forceinline__ void x_issue_panel(char* img, const bf16* __restrict__ G, int ld, int r0,
                                              int k0, int tid) {
#pragma unroll
  for (int i = 0; i < X_CHUNKS; ++i) {
    const int p = X_NT * i + tid;                  // LDS position (16 B units)
    const int row = p >> 3;
    const int j = (p & 7) ^ x_swz(row);
    x_dma16(G + (size_t)(r0 + row) * ld + k0 + j * 8, img + (X_NT * i + (tid & ~63)) * 16);
  }
}

// 16x16x32 operand fragment: lane&15 = row, lane group g owns k = 8g..8g+7
__device__ __forceinline__ bf16x8 x_frag(const char* img, int rbase, int kk, int lane) {
  const int m = rbase + (lane & 15);
  return *(const bf16x8*)(img + m * X_RB + (((kk * 4 + (lane >> 4)) ^ x_swz(m)) << 4));
}

__device__ __forceinline__ void x_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

struct X3Args {
  const bf16 *a_hi, *a_lo, *b_hi, *b_lo;
  int lda, ldb, K;
  bf16 *o_hi, *o_lo;       // output planes (nullable together)
};

// XCD-aware grouped tile order, as tile_coord in mmad_gemm_dev.h (S = 1)
__device__ __forceinline__ void x_tile(const GemmEpi& ep, int bid, int nblk, int& tm, int& tn) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int tiles_m = nblk / ep.tiles_n;
  const int per_group = ep.group_m * ep.tiles_n;
  const int first_m = (tile / per_group) * ep.group_m;
  const int gsz = min(tiles_m - first_m, ep.group_m);
  tm = first_m + (tile % per_group) % gsz;
  tn = (tile % per_group) / gsz;
}

template <int EPI>
__global__ __launch_bounds__(X_NT, 1) void mmad_gemm_x3_kernel(X3Args ar, GemmEpi ep) {
  __shared__ __attribute__((aligned(16))) char smem[X_NS * X_SLOT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / X_WN, wn = w % X_WN;
  int tm, tn;
  x_tile(ep, blockIdx.x, gridDim.x, tm, tn);
  const int m0 = tm * X_BM, n0 = tn * X_BN;
  const int nt = ar.K / X_BK;

  floatx4 acc_h[X_TM][X_TN], acc_x[X_TM][X_TN];
#pragma unroll
  for (int i = 0; i < X_TM; ++i)
#pragma unroll
    for (int j = 0; j < X_TN; ++j) {
      acc_h[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
      acc_x[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

  auto issue = [&](int s) {
    char* base = smem + (s % X_NS) * X_SLOT;
    const int k0 = s * X_BK;
    x_issue_panel(base, ar.a_hi, ar.lda, m0, k0, tid);
    x_issue_panel(base + X_PANEL, ar.a_lo, ar.lda, m0, k0, tid);
    x_issue_panel(base + 2 * X_PANEL, ar.b_hi, ar.ldb, n0, k0, tid);
    x_issue_panel(base + 3 * X_PANEL, ar.b_lo, ar.ldb, n0, k0, tid);
  };

  // two-slot ring, one barrier per stage: stage t has landed (the only one in
  // flight) and every wave has finished reading slot t+1's previous contents
  // before stage t+1 is issued under the MFMAs of stage t
  const int ra = wm * 16 * X_TM, rb = wn * 16 * X_TN;
  issue(0);
  for (int t = 0; t < nt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    x_barrier();
    if (t + 1 < nt) issue(t + 1);
    const char* sa = smem + (t % X_NS) * X_SLOT;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 ah[X_TM], al[X_TM], bh[X_TN], bl[X_TN];
#pragma unroll
      for (int i = 0; i < X_TM; ++i) {
        ah[i] = x_frag(sa, ra + i * 16, kk, lane);
        al[i] = x_frag(sa + X_PANEL, ra + i * 16, kk, lane);
      }
#pragma unroll
      for (int j = 0; j < X_TN; ++j) {
        bh[j] = x_frag(sa + 2 * X_PANEL, rb + j * 16, kk, lane);
        bl[j] = x_frag(sa + 3 * X_PANEL, rb + j * 16, kk, lane);
      }
      // fixed order per accumulator: hi.lo, lo.hi (cross accumulator), hi.hi
#pragma unroll
      for (int i = 0; i < X_TM; ++i)
#pragma unroll
        for (int j = 0; j < X_TN; ++j)
          acc_x[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], ah[i], acc_x[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < X_TM; ++i)
#pragma unroll
        for (int j = 0; j < X_TN; ++j)
          acc_x[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], al[i], acc_x[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < X_TM; ++i)
#pragma unroll
        for (int j = 0; j < X_TN; ++j)
          acc_h[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], ah[i], acc_h[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: y = bn_affine(act(acc + bias)) in fp32, from registers.
  // Lane (g, c): row = tile row c of fragment row i, columns 4g..4g+3 of
  // fragment column j.
  const int g = lane >> 4, c = lane & 15;
  float rsum[X_TM];
#pragma unroll
  for (int i = 0; i < X_TM; ++i) rsum[i] = 0.f;
#pragma unroll
  for (int j = 0; j < X_TN; ++j) {
    const int col0 = n0 + rb + j * 16 + 4 * g;
    const floatx4 b4 = ep.bias ? *(const floatx4*)(ep.bias + col0) : floatx4{0.f, 0.f, 0.f, 0.f};
    const floatx4 s4 = ep.bn_scale ? *(const floatx4*)(ep.bn_scale + col0) : floatx4{1.f, 1.f, 1.f, 1.f};
    const floatx4 t4 = ep.bn_shift ? *(const floatx4*)(ep.bn_shift + col0) : floatx4{0.f, 0.f, 0.f, 0.f};
    floatx4 w4{1.f, 1.f, 1.f, 1.f};
    if constexpr (EPI == GEMM_EPI_SCORE) {
      if (ep.colw) w4 = *(const floatx4*)(ep.colw + col0);
    }
#pragma unroll
    for (int i = 0; i < X_TM; ++i) {
      const int row = m0 + ra + i * 16 + c;
      const bool rok = row < ep.M;
      floatx4 y;
      bf16x4 yh, yl;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = (acc_x[i][j][e] + acc_h[i][j][e]) + b4[e];
        float v = apply_act(z, ep.act, ep.slope);
        if (ep.bn_scale) v = v * s4[e] + t4[e];
        v = (rok && col0 + e < ep.N) ? v : 0.f;
        y[e] = v;
        yh[e] = (bf16)v;
        yl[e] = (bf16)(v - (float)yh[e]);
      }
      if constexpr (EPI == GEMM_EPI_SCORE) {
        // diff against the fp32 reference before anything is rounded to planes
        const float* rp = (const float*)ep.ref;
        float* dp = ep.diff ? ep.diff + (size_t)row * ep.lddiff + col0 : nullptr;
        // ... and as split planes (a packed x3 operand's slot: scalar stores,
        // any lddp / dp_col; rows >= M and columns >= N are not written)
        const size_t po = (size_t)row * ep.lddp + ep.dp_col + col0;
        bf16* ph = ep.dp_hi ? (bf16*)ep.dp_hi + po : nullptr;
        bf16* pl = ep.dp_hi ? (bf16*)ep.dp_lo + po : nullptr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = rok && col0 + e < ep.N;
          const float rv = (rp && ok) ? rp[(size_t)row * ep.ldref + col0 + e] : 0.f;
          const float d = y[e] - rv;
          rsum[i] = fmaf(d * d, w4[e], rsum[i]);
          if (dp && ok) dp[e] = d;
          if (ph && ok) {
            const bf16 dh = (bf16)d;
            ph[e] = dh;
            pl[e] = (bf16)(d - (float)dh);
          }
        }
      }
      if (ar.o_hi) {
        const size_t o = (size_t)row * ep.ldo + col0;
        *(bf16x4*)(ar.o_hi + o) = yh;
        *(bf16x4*)(ar.o_lo + o) = yl;
      }
      if (ep.out32) *(floatx4*)(ep.out32 + (size_t)row * ep.ld32 + col0) = y;
    }
  }
  if constexpr (EPI == GEMM_EPI_SCORE) {
    // row sums over the tile's 128 columns: lane groups, then the 4 column
    // waves through LDS in a fixed order
    float* red = (float*)smem;                     // [X_WN][X_BM]
    x_barrier();                                   // every wave is done with the ring
#pragma unroll
    for (int i = 0; i < X_TM; ++i) {
      const float s = sum_lane_groups(rsum[i]);
      if (g == 0) red[wn * X_BM + ra + i * 16 + c] = s;
    }
    __syncthreads();
    if (tid < X_BM) {
      const float tot = (red[tid] + red[X_BM + tid]) + (red[2 * X_BM + tid] + red[3 * X_BM + tid]);
      ep.rowsq[(size_t)tn * ep.ldrow + m0 + tid] = tot;
    }
  }
}

int x_group_m(int ntiles, int tiles_m) {
  int gm = (int)(sqrt(ntiles / 8.0) + 0.5);
  const int o = mmad_group_override();
  if (o > 0) gm = o;
  return gm < 1 ? 1 : (gm > tiles_m ? tiles_m : gm);
}

}  // namespace

int mmad_gemm_x3_dispatch(int epi, const void* A, int lda, const void* B, int ldb, int Mp, int Np,
                          int K, const GemmEpi& ep_in, hipStream_t s) {
  if (epi != GEMM_EPI_FWD && epi != GEMM_EPI_SCORE) {
    mmad_set_error("gemm x3: only the forward and score epilogues run on split-bf16 planes (epi %d)", epi);
    return MMAD_EUNSUPPORTED;
  }
  if (ep_in.part || ep_in.bpart || ep_in.bn_sync) {
    mmad_set_error("gemm x3: no BatchNorm statistics / folded-BN partials / fused BN on this path");
    return MMAD_EUNSUPPORTED;
  }
  MMAD_CHECK_ARG(A && B, "gemm x3: null operand");
  MMAD_CHECK_ARG(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0, "gemm x3: bad leading dims");
  MMAD_CHECK_ARG(epi != GEMM_EPI_SCORE || ep_in.rowsq, "gemm x3: score needs rowsq");
  MMAD_CHECK_ARG(ep_in.out || epi == GEMM_EPI_SCORE, "gemm x3: null output");
  MMAD_CHECK_ARG(!ep_in.out || ep_in.ldo % 4 == 0, "gemm x3: ldo must be a multiple of 4");
  MMAD_CHECK_ARG(!ep_in.out32 || (ep_in.ld32 % 4 == 0 && ep_in.ld32 >= Np), "gemm x3: bad ld32");
  MMAD_CHECK_ARG((ep_in.dp_hi == nullptr) == (ep_in.dp_lo == nullptr), "gemm x3: diff planes come as a pair");
  MMAD_CHECK_ARG(!ep_in.dp_hi || (epi == GEMM_EPI_SCORE && ep_in.dp_col >= 0 &&
                                  ep_in.lddp >= ep_in.dp_col + ep_in.N),
                 "gemm x3: diff planes need the score epilogue and lddp >= dp_col + N");
  GemmEpi ep = ep_in;
  X3Args ar{};
  ar.a_hi = (const bf16*)A;
  ar.a_lo = ep.a_lo ? (const bf16*)ep.a_lo : ar.a_hi + (size_t)Mp * lda;
  ar.b_hi = (const bf16*)B;
  ar.b_lo = ep.b_lo ? (const bf16*)ep.b_lo : ar.b_hi + (size_t)Np * ldb;
  ar.lda = lda;
  ar.ldb = ldb;
  ar.K = K;
  ar.o_hi = (bf16*)ep.out;
  ar.o_lo = ep.out ? (bf16*)ep.out + (size_t)Mp * ep.ldo : nullptr;
  const int tiles_m = Mp / X_BM, tiles_n = Np / X_BN, ntiles = tiles_m * tiles_n;
  ep.tiles_n = tiles_n;
  ep.group_m = x_group_m(ntiles, tiles_m);
  const void* fn = epi == GEMM_EPI_FWD ? (const void*)mmad_gemm_x3_kernel<GEMM_EPI_FWD>
                                       : (const void*)mmad_gemm_x3_kernel<GEMM_EPI_SCORE>;
  void* args[] = {&ar, &ep};
  return mmad_gemm_launch(fn, dim3(ntiles), dim3(X_NT), s, ep.start_ev, ep.done_ev, args);
}
