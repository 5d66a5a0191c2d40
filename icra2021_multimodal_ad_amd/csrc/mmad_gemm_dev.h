// MFMA GEMM for the fc_module encoder/decoder stack on gfx950 (CDNA4).
//
// One kernel template covers the three contractions of an FCLayer
// (layers/fc_layer.py:37-48 forward; its autograd backward):
//   forward      y  = x  . W^T  (+bias, act, BN-eval affine | BN-train stats
//                                 | MSE grad/loss | score-diff epilogues)
//   backward-dx  dx = dz . W     (B operand is MN-major: W stored [out][in])
//   backward-dW  dW = dz^T . x   (both operands MN-major: K = batch)
// Operands stay in the caller's row-major packed layout; an MN-major operand
// is transposed on the LDS read side with ds_read_b64_tr_b16 (bf16) or plain
// per-k reads (f32), so no transposed copies are ever materialised in HBM.
//
// Block tiles (CFG), one block per CU:
//   0: 128x128, 512 threads (waves 2x4, wave tile 64x32), 4-stage ring
//   1: 256x128, 512 threads (waves 4x2, wave tile 64x64), 3-stage ring
//   2: 128x256, 512 threads (waves 2x4, wave tile 64x64), 3-stage ring
//   3:  64x64,  256 threads (waves 2x2, wave tile 32x32), 4-stage ring
//   4:  64x128, 256 threads (waves 2x2, wave tile 32x64), 5-stage ring
//   5: 128x128, 256 threads (waves 2x2, wave tile 64x64), 4-stage ring
// The 8-wave tiles run two waves per SIMD (one wave's LDS reads and barrier
// wait hide behind the other's MFMAs) and carry the large layers; the small
// tiles give the narrow layers enough blocks.  Which one a shape gets is
// measured on first use (mmad_gemm_dispatch autotune): the accumulation
// order over K is the same for every tile, so the choice never changes a
// result bit.  Tiles 6-9 (256x256 and the register-direct forms) are
// described at their Cfg<N>.  Which tiles may run a problem, which tile then
// runs and which instantiation that is, is decided in one block of the host
// part (mmad_gemm_mfma.hip): the tile table TILES, the rule tile_allowed /
// tile_runs over a GemmProblem, and kernel_of generated from the table.  A
// new tile is entered once: its Cfg<N> and its row of TILES.
// K stage = 128 bytes of K per operand row (BK = 64 bf16 / 32 f32), staged
// global -> LDS by global_load_lds (16 B/lane, no registers), NS-stage ring
// with a counted vmcnt and a raw s_barrier so NS-2 stages stay in flight
// across every barrier.
//
// LDS images:
//  * K-major operand: [rows][128 B], 16-byte chunk j stored at j ^ ((row>>1)&7)
//    -> conflict-free ds_read_b128 (natural k order) / ds_read_b64 pairs.
//  * MN-major operand: [BK][rows*esize], 16-byte chunk XOR-swizzled per k-row
//    so the tr-reads of one 32-lane half (8 k-rows) hit disjoint banks.
// bf16 k-slot order inside one 32-deep MFMA step: lane group g (= lane>>4)
// owns k = 8g..8g+7 in both operands whatever their layout (one ds_read_b128
// from a K-major image, two ds_read_b64_tr_b16 from an MN-major one).  The
// backward GEMMs used a permuted order {4g..4g+3} U {16+4g..16+4g+3} before,
// which cost the K-major operand two ds_read_b64 per fragment and measured
// 2x the LDS cycles of the forward loop (SQ_LDS_BANK_CONFLICT 1.7M vs 13k).
//
// This header: the tile table Cfg<N>, the LDS images and their DMA issue, the
// fragment reads, the MFMA / wait helpers, the fused-BN column barrier and the
// tile order.  mmad_gemm_body.h: the tile body and the kernels.
// mmad_gemm_mfma.hip: host planning and launch.  mmad_gemm_b4.hip: tile 8's
// translation unit.
#pragma once
#include "mmad_common.h"
#include "mmad_gemm.h"

#include <hip/hip_ext.h>

#include <cmath>
#include <type_traits>

namespace {

constexpr int MMAD_KB = 128;   // bytes of K per LDS row per stage

template <int CFG> struct Cfg;
template <> struct Cfg<0> { static constexpr int BM = 128, BN = 128, WM = 2, WN = 4, NS = 4, NT = 512; };
template <> struct Cfg<1> { static constexpr int BM = 256, BN = 128, WM = 4, WN = 2, NS = 3, NT = 512; };
template <> struct Cfg<2> { static constexpr int BM = 128, BN = 256, WM = 2, WN = 4, NS = 3, NT = 512; };
template <> struct Cfg<3> { static constexpr int BM = 64, BN = 64, WM = 2, WN = 2, NS = 4, NT = 256; };
template <> struct Cfg<4> { static constexpr int BM = 64, BN = 128, WM = 2, WN = 2, NS = 5, NT = 256; };
template <> struct Cfg<5> { static constexpr int BM = 128, BN = 128, WM = 2, WN = 2, NS = 4, NT = 256; };
// 256x256, 8 waves (2 x 4, wave tile 128x64), a 2-slot ring: twice the
// operand reuse of 256x128 (128 FLOP per staged byte), for the large-row
// bf16 GEMMs of the forward / score / MSE epilogues without the fused BN
// (C5 scoring at 65,536 rows; a round-3 stand-alone loop study, since removed: 0.47-0.55 of peak at
// 16384 x 2048 x 1664 vs 0.33 for 256x128); its epilogue staging fills LDS
constexpr int CFG_BIG = 6;
template <> struct Cfg<6> { static constexpr int BM = 256, BN = 256, WM = 2, WN = 4, NS = 2, NT = 512; };
// 7: 256x256, CFG 6's loop with the MFMA operands swapped (W first): each
// lane's accumulator quad is then 4 consecutive COLUMNS of one output row, so
// the forward / score epilogue stores from registers -- one v_permlane16_swap
// pair turns two column tiles' quads into a 16-byte chunk per lane, 64 B per
// row per store instruction -- with no LDS staging round trip (the score row
// sums meet across the two waves of a 128-column group in 4 KB of LDS).
// Eval forward / score only (no column partials: the BN statistics need the
// row-quad layout); the dispatcher runs CFG 6 in its place otherwise (same
// tile, same bits).
constexpr int CFG_XST = 7;
template <> struct Cfg<7> { static constexpr int BM = 256, BN = 256, WM = 2, WN = 4, NS = 2, NT = 512; };
// 8: 256x256, FOUR waves (2 x 2, wave tile 128x128: 256 accumulator
// registers per lane, in AGPRs), otherwise CFG 7 (swapped operands,
// register-direct epilogue).  One wave per SIMD: per 32-deep step a wave
// issues 64 MFMAs against 16 fragment reads, a third fewer LDS reads per MFMA
// than the 8-wave 128x64 wave tiles.  Compiled in its own translation unit
// (mmad_gemm_b4.hip, csrc/Makefile) WITHOUT the VGPR-form MFMA
// flag the other tiles use: 256 + ~150 registers need the AGPR half of the
// file; the host side reaches it through mmad_gemm_b4_kernel.
constexpr int CFG_B4 = 8;
template <> struct Cfg<8> { static constexpr int BM = 256, BN = 256, WM = 2, WN = 2, NS = 2, NT = 256; };
// 9: CFG 1 (256x128, 8 waves of 64x64) with CFG 7's swapped operands and
// register-direct epilogue: the large-row forward / score GEMMs whose output
// width is not a multiple of 256 (C5: every layer but the 2048-wide ones)
constexpr int CFG_XST1 = 9;
template <> struct Cfg<9> { static constexpr int BM = 256, BN = 128, WM = 4, WN = 2, NS = 3, NT = 512; };
constexpr int NCFG = 10;
// which (operand type, epilogue) pairs the 256x256 tiles (6, 7, 8) and the
// register-direct tiles (7, 8, 9) are instantiated for; the host-side tile
// table and tile_allowed (mmad_gemm_mfma.hip) state the same per problem
template <typename T, int EPI>
constexpr bool big_ok() {
  return sizeof(T) == 2 && (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_MSE || EPI == GEMM_EPI_SCORE);
}
template <typename T, int EPI>
constexpr bool xst_ok() {
  return sizeof(T) == 2 && (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_SCORE);
}

template <typename T, bool KMAJ, int ROWS, int NT>
struct Img {
  static constexpr int ES = sizeof(T);
  static constexpr int KB = MMAD_KB;
  static constexpr int BK = KB / ES;                  // K per stage
  static constexpr int RB = KMAJ ? KB : ROWS * ES;    // bytes per LDS row
  static constexpr int BYTES = ROWS * KB;             // image bytes (both layouts)
  static constexpr int CPROW = RB / 16;               // 16 B chunks per LDS row
  static constexpr int CHUNKS = BYTES / 16 / NT;      // global_load_lds per thread
  static_assert(CHUNKS >= 1 && BYTES % (16 * NT) == 0, "image/threads mismatch");
};

// 16-byte-chunk XOR swizzle of LDS row `r` (an involution):
//  * K-major, 128 B rows: (r>>1)&7;
//  * MN-major bf16 (rows are k): one transposed read of a 32-lane half covers
//    k rows {0..3, 8..11} (+4 for the second read) of a 32-deep step, 32 B of
//    each; >= 256 B rows start every k row on bank 0, so the XOR takes
//    (k&3) | ((k>>3)&1)<<2 (even chunk steps of 8 banks); 128 B rows alternate
//    bank halves by k parity, so (k>>1)&1 | ((k>>3)&1)<<1 (the XOR must stay
//    inside the row's 8 chunks).  Conflict-free for both reads of a half;
//  * MN-major f32 (rows >= 256 B): r&7 (spreads the 4-row-apart ds_read_b32 groups).
template <typename T, bool KMAJ, int RB>
__device__ __forceinline__ int swz(int r) {
  static_assert(KMAJ || RB >= (sizeof(T) == 2 ? 128 : 256), "MN-major row too short for its swizzle");
  if constexpr (KMAJ) return (r >> 1) & 7;
  else if constexpr (sizeof(T) == 2)
    return RB >= 256 ? (((r & 3) | (((r >> 3) & 1) << 2)) << 1)
                     : ((((r >> 1) & 1) | (((r >> 3) & 1) << 1)) << 1);
  else return r & 7;
}

// One 16-byte-per-lane LDS-DMA (global_load_lds_dwordx4) into the wave's
// 1 KiB at `dst` (wave-uniform), as inline asm.  Through the builtin, hipcc's
// wait-count pass tracks the DMA as an LDS write it cannot tell apart from
// the transposing fragment reads (ds_read_b64_tr_b16) of other ring slots
// and puts an s_waitcnt vmcnt(0) in front of them -- inside the main loop
// that drains the whole NS-stage ring every K stage.  Hidden from that pass,
// the ring is ordered exactly as designed: counted vmcnt + workgroup barrier
// before a slot is read, a barrier before it is refilled.  (Compiler-tracked
// loads only see MORE operations outstanding than they count, so their own
// waits stay correct, just stricter.)
__device__ __forceinline__ void dma16(const void* src, char* dst) {
  const unsigned lds = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(MMAD_LDS void*)dst);
  asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(src), "{m0}"(lds) : "memory");
}

// issue one stage of one operand: global -> LDS, 16 B per lane, no registers
template <typename T, bool KMAJ, int ROWS, int NT>
__device__ __forceinline__ void issue_stage(char* img, const T* __restrict__ G, int ld, int r0,
                                            int k0, int tid) {
  using I = Img<T, KMAJ, ROWS, NT>;
  constexpr int EPC = 16 / sizeof(T);
#pragma unroll
  for (int i = 0; i < I::CHUNKS; ++i) {
    const int p = NT * i + tid;                        // LDS position (16 B units)
    const int row = p / I::CPROW;
    const int j = (p % I::CPROW) ^ swz<T, KMAJ, I::RB>(row);
    const T* src = KMAJ ? G + (size_t)(r0 + row) * ld + k0 + j * EPC
                        : G + (size_t)(k0 + row) * ld + r0 + j * EPC;
    dma16(src, img + (NT * i + (tid & ~63)) * 16);
  }
}

// chunk i (< Img::CHUNKS) of one stage of one operand (issue_stage = all i)
template <typename T, bool KMAJ, int ROWS, int NT>
__device__ __forceinline__ void issue_chunk(char* img, const T* __restrict__ G, int ld, int r0, int k0,
                                            int tid, int i) {
  using I = Img<T, KMAJ, ROWS, NT>;
  constexpr int EPC = 16 / sizeof(T);
  const int p = NT * i + tid;
  const int row = p / I::CPROW;
  const int j = (p % I::CPROW) ^ swz<T, KMAJ, I::RB>(row);
  const T* src = KMAJ ? G + (size_t)(r0 + row) * ld + k0 + j * EPC
                      : G + (size_t)(k0 + row) * ld + r0 + j * EPC;
  dma16(src, img + (NT * i + (tid & ~63)) * 16);
}

// ---- bf16 fragment reads (16x16x32 MFMA operand) ---------------------------
// Natural k order for both layouts: lane group g owns k = 8g..8g+7 (K-major:
// one ds_read_b128; MN-major: two ds_read_b64_tr_b16 of k rows 8g..8g+3 and
// 8g+4..8g+7).  (NAT = false, the older permuted order {4g..4g+3} U
// {16+4g..16+4g+3}, is kept for the K-major reader only.)
template <bool KMAJ, bool NAT, int ROWS>
__device__ __forceinline__ bf16x8 frag_bf16(const char* img, int rbase, int kk, int lane) {
  using I = Img<bf16, KMAJ, ROWS, 256>;   // RB only
  const int g = lane >> 4;
  if constexpr (KMAJ) {
    const int m = rbase + (lane & 15);
    const int f = swz<bf16, true, I::RB>(m);
    if constexpr (NAT) {
      return *(const bf16x8*)(img + m * I::RB + (((kk * 4 + g) ^ f) << 4));
    } else {
      const int c1 = (kk * 8 + g) ^ (f << 1);          // 8-byte units
      const int c2 = (kk * 8 + 4 + g) ^ (f << 1);
      bf16x4 lo = *(const bf16x4*)(img + m * I::RB + c1 * 8);
      bf16x4 hi = *(const bf16x4*)(img + m * I::RB + c2 * 8);
      return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  } else {
    static_assert(NAT, "MN-major reads deliver the natural k order");
    const int q = (lane >> 2) & 3, p = lane & 3;
    const int k1 = kk * 32 + 8 * g + q, k2 = k1 + 4;
    const int byte = (rbase + 4 * p) * 2;
    const int j = byte >> 4, within = byte & 15;
    const MMAD_LDS char* base = (const MMAD_LDS char*)img;
    short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (MMAD_LDS short4v*)(base + k1 * I::RB + ((j ^ swz<bf16, false, I::RB>(k1)) << 4) + within));
    short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (MMAD_LDS short4v*)(base + k2 * I::RB + ((j ^ swz<bf16, false, I::RB>(k2)) << 4) + within));
    bf16x4 l4 = __builtin_bit_cast(bf16x4, lo);
    bf16x4 h4 = __builtin_bit_cast(bf16x4, hi);
    return __builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

// ---- f32 fragment reads (16x16x4 MFMA, 4 steps per 16-deep chunk) -------
template <bool KMAJ, int ROWS>
__device__ __forceinline__ floatx4 frag_f32(const char* img, int rbase, int kc, int lane) {
  using I = Img<float, KMAJ, ROWS, 256>;  // RB only
  const int g = lane >> 4;
  if constexpr (KMAJ) {
    const int m = rbase + (lane & 15);
    const int j = (kc * 4 + g) ^ swz<float, true, I::RB>(m);
    return *(const floatx4*)(img + m * I::RB + j * 16);
  } else {
    const int col = rbase + (lane & 15);
    const int j = col >> 2, within = (col & 3) * 4;
    floatx4 r;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = kc * 16 + 4 * g + s;
      r[s] = *(const float*)(img + k * I::RB + ((j ^ swz<float, false, I::RB>(k)) << 4) + within);
    }
    return r;
  }
}

// every phase of the main loop pinned in issue order
#define MMAD_SB() __builtin_amdgcn_sched_barrier(0)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- pipelined main-loop helpers -------------------------------------------
// One K stage (128 B of K per operand row) = two sub-steps: 32-deep bf16
// MFMA steps, or 16-deep f32 steps (4 x 16x16x4 MFMAs each).
template <typename T> struct SubFrag;
template <> struct SubFrag<bf16> { using F = bf16x8; };
template <> struct SubFrag<float> { using F = floatx4; };

template <typename T, bool AK, bool BK_, bool NAT, int BM, int BN, int TM, int TN>
__device__ __forceinline__ void read_sub(const char* sa, const char* sb, int ra, int rb, int sub,
                                         int lane, typename SubFrag<T>::F (&fa)[TM],
                                         typename SubFrag<T>::F (&fb)[TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    if constexpr (sizeof(T) == 2) fa[i] = frag_bf16<AK, NAT, BM>(sa, ra + i * 16, sub, lane);
    else fa[i] = frag_f32<AK, BM>(sa, ra + i * 16, sub, lane);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    if constexpr (sizeof(T) == 2) fb[j] = frag_bf16<BK_, NAT, BN>(sb, rb + j * 16, sub, lane);
    else fb[j] = frag_f32<BK_, BN>(sb, rb + j * 16, sub, lane);
  }
}

// MFMAs of fragment rows i in [H*TM/2, (H+1)*TM/2): a sub-step is issued as
// two such groups with the next fragment reads between them
// row_hook(i) runs after the MFMAs of fragment row i: the next stage's
// LDS-DMA is spread over them (a burst of DMA issues right after the barrier
// delays the MFMAs behind it: +10-12 % in the round-3 loop study, profiles/r03c_*)
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};
// (SW: the operands swapped -- W first -- for the register-direct epilogue)
template <typename T, int TM, int TN, int H, bool SW = false, typename Hook = NoHook>
__device__ __forceinline__ void mma_half(floatx4 (&acc)[TM][TN], const typename SubFrag<T>::F (&fa)[TM],
                                         const typename SubFrag<T>::F (&fb)[TN], Hook row_hook = Hook{}) {
#pragma unroll
  for (int i = H * TM / 2; i < (H + 1) * TM / 2; ++i) {
    row_hook(i);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (sizeof(T) == 2) {
        acc[i][j] = SW ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
      }
    }
  }
}

// lgkmcnt(0) as a real s_waitcnt (vmcnt/expcnt at max) so the compiler's own
// counter bookkeeping sees it
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// no more issues: stage t+1 must land, rem = nt-t-2 later stages may stay in flight
template <int NL>
__device__ __forceinline__ void wait_tail(int rem) {
  if (rem >= 3) wait_vmcnt<3 * NL>();
  else if (rem == 2) wait_vmcnt<2 * NL>();
  else if (rem == 1) wait_vmcnt<NL>();
  else wait_vmcnt<0>();
}

// the same with X more (younger) loads allowed in flight: the dW GEMM's Adam
// state prefetch, issued after the last ring DMA
template <int NL, int X>
__device__ __forceinline__ void wait_tail_x(int rem) {
  static_assert(3 * NL + X <= 63, "vmcnt range");
  if (rem >= 3) wait_vmcnt<3 * NL + X>();
  else if (rem == 2) wait_vmcnt<2 * NL + X>();
  else if (rem == 1) wait_vmcnt<NL + X>();
  else wait_vmcnt<X>();
}

__device__ __forceinline__ void block_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- cross-workgroup hand-off of the fused-BN column partials -------------
// Agent-scope relaxed atomics lower to sc1 global loads / stores (L1
// bypassed, written through): producers store every partial sc1, wait for
// their stores, meet at a workgroup barrier, and one lane adds to the column
// counter; one lane polls it with sc1 loads, the block joins it at a barrier
// and then reads the partials with sc1 loads only (MI355X_MICROARCH.md,
// hand-off table row 1: no release / acquire fences needed).
__device__ __forceinline__ void st_sc1(float* p, float v) {
  __hip_atomic_store((unsigned*)p, __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store((unsigned long long*)p, __builtin_bit_cast(unsigned long long, v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
  return __builtin_bit_cast(float, __hip_atomic_load((unsigned*)p, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __builtin_bit_cast(double, __hip_atomic_load((unsigned long long*)p, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT));
}

// Barrier of the `target` blocks sharing one output column tile: counter
// ctr[0] and generation word ctr[MMAD_BN_EXIT].  Each block reads the
// generation (`gen0`, read before it arrives: the caller loads it early),
// adds one arrival; the last arriver resets the counter and bumps the
// generation, the others poll the generation (sc1).  The counter is zero
// again when the barrier opens, whatever tile configuration used it last.
// Bounded: a barrier that does not open within ~2^20 polls (about a second)
// sets the sticky error word and returns false (the caller skips its
// outputs; the host reports it through mmad_ae_status) instead of hanging.
__device__ __forceinline__ unsigned col_gen(const unsigned* ctr) {
  return __hip_atomic_load(ctr + MMAD_BN_EXIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// arrive: after every wave's partial stores have landed, one lane adds an
// arrival; the last arriver resets the counter and opens the barrier
__device__ __forceinline__ void col_arrive(unsigned* ctr, unsigned target, int tid, unsigned* shw) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partial stores landed
  __syncthreads();                                   // ... and every other wave's
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned last = 0u;
    if (old + 1u == target) {
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(ctr + MMAD_BN_EXIT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = 1u;
    }
    shw[1] = last;   // read by lane 0 only (col_wait)
  }
}
// wait: lane 0 polls the generation word unless its block arrived last; the
// block joins it at a workgroup barrier (then reads the partials, sc1)
__device__ __forceinline__ bool col_wait(unsigned* ctr, unsigned gen0, unsigned* err, int tid,
                                         unsigned* shw) {
  if (tid == 0) {
    unsigned ok = shw[1];
    for (unsigned spins = 0; !ok && spins < (1u << 20); ++spins) {
      if (col_gen(ctr) != gen0) {
        ok = 1u;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (!ok) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    shw[0] = ok;
  }
  __syncthreads();
  return shw[0] != 0u;
}

}  // namespace

// -------------------------------------------------------------------------
// Train-mode BatchNorm of the producer layer never touches the operands here:
// the forward folds it into the consumer's weights and bias (bn_fold_k: the
// B operand is W*scale, the bias gets sum_k shift*W via bpart partials), the
// dW GEMM contracts the raw activation and fixes up in the epilogue
// (dW = scale[k] * acc + shift[k] * db[n]).  Every GEMM is a plain MFMA
// contraction.
// XCD-aware order (1-D grid).  Under round-robin dispatch, blocks with equal
// bid % 8 share an XCD (speed only, never correctness); each such set gets a
// contiguous range of logical blocks lt; the S split-K blocks of one output
// tile are consecutive in lt (one XCD), and tiles are grouped group_m M-tiles
// at a time so every XCD works on a compact rectangle whose A/B panels stay
// in its L2.
struct TileCoord {
  int tm, tn, tile, sk;
};
__device__ __forceinline__ TileCoord tile_coord(const GemmEpi& ep, int bid, int nblk, int S) {
  TileCoord tc;
  const int ntl = nblk / S;
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
  const int lt = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  tc.tile = lt / S;
  tc.sk = lt - tc.tile * S;
  const int tiles_m = ntl / ep.tiles_n;
  const int per_group = ep.group_m * ep.tiles_n;
  const int first_m = (tc.tile / per_group) * ep.group_m;
  const int gsz = min(tiles_m - first_m, ep.group_m);
  tc.tm = first_m + (tc.tile % per_group) % gsz;
  tc.tn = (tc.tile % per_group) / gsz;
  return tc;
}
