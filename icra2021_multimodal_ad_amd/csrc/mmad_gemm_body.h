// The MFMA GEMM's tile body and its kernels (device code only; the tiles,
// LDS images and helpers are in mmad_gemm_dev.h, host planning and launch in
// mmad_gemm_mfma.hip).
//
// TileTraits<T, TO, AK, BK, CFG, EPI> holds every compile-time constant of one
// instantiation, each declared once, and gemm_body as a static member, so the
// constants are in scope in it unqualified.  gemm_body is still one scope:
// prologue and prefetches -> main loop (256x256 | ring) -> split-K combine ->
// epilogue (register-direct | register phase -> LDS-staged store -> fused BN
// forward | small-segment Adam | bwd-data BN).  Each of those phases was
// tried as a forced-inline function taking the values it uses as plain
// arguments, one at a time; each changed the instruction stream of the
// kernels that use it (profiles/gemm_body_split.json), so they
// stay inline.
#pragma once
#include "mmad_gemm_dev.h"

template <typename T, typename TO, bool AK, bool BK_, int CFG, int EPI>
struct TileTraits {
  using C = Cfg<CFG>;
  static constexpr int BM = C::BM, BN = C::BN, WM = C::WM, WN = C::WN, NS = C::NS, NT = C::NT;
  static constexpr int TM = BM / WM / 16, TN = BN / WN / 16;   // 16x16 MFMA tiles per wave
  static constexpr int NW = NT / 64;
  static_assert(WM * WN == NW && TM % 2 == 0, "wave grid");
  using IA = Img<T, AK, BM, NT>;
  using IB = Img<T, BK_, BN, NT>;
  using FR = typename SubFrag<T>::F;
  // bf16: every operand layout delivers the natural k order (lane group g owns
  // k = 8g..8g+7), so a K-major operand is one ds_read_b128 per fragment
  static constexpr bool NAT = true;
  static constexpr int SLOT = IA::BYTES + IB::BYTES;
  static constexpr int NL = IA::CHUNKS + IB::CHUNKS;          // vm ops per thread per stage
  static constexpr bool FWDLIKE = EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_MSE || EPI == GEMM_EPI_SCORE;
  static constexpr bool BIG = CFG == CFG_BIG || CFG == CFG_XST || CFG == CFG_B4;
  static constexpr bool XST = CFG == CFG_XST || CFG == CFG_B4 || CFG == CFG_XST1;
  static_assert(!BIG || big_ok<T, EPI>(), "256x256 tile: bf16 forward-type epilogues only");
  static_assert(!XST || xst_ok<T, EPI>(), "CFG 7 / 8 / 9: bf16 eval forward / score only");
  // prefetched bias partials per lane (none for the 256x256 tile: its
  // 128 accumulator registers leave no room to hold them across the loop)
  static constexpr int QB = BIG ? 0 : 8;
  static constexpr int QG = 32;                               // prefetched dW row-sum partials
  static constexpr int OSTRIDE = BN * (int)sizeof(TO) + 16;
  static constexpr int OBYTES = BM * OSTRIDE + (EPI == GEMM_EPI_BWD_DATA ? BM * BN / 2 : 0);   // + fp64 [BM/16][BN]
  // fused train-mode BN: per-column merge results (2 x fp64 [BN]) + a flag word
  // (fwd: 4 chunk-group Welford merges + scale/shift; bwd-data: the sums --
  // its chunk-group sums reuse the fp64 piece scratch)
  static constexpr int XBYTES = BIG ? 0
                                : EPI == GEMM_EPI_FWD ? 12 * BN * 8 + 2 * BN * 4 + 64
                                : EPI == GEMM_EPI_BWD_DATA ? 6 * BN * 8 + 64 : 0;
  // transposed epilogue staging (bf16 outputs of the forward-type epilogues
  // without a fused BN): the tile goes to LDS column-major, 8 B per lane per
  // MFMA fragment (ds_write_b64), and comes back row-major, 16 B per lane,
  // through ds_read_b64_tr_b16 (the LDS-staged store); column stride CS, 8-byte
  // granules XOR-swizzled by (col >> 1) & 7: conflict-free on both sides
  static constexpr bool TSTG = sizeof(TO) == 2 && (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_MSE ||
                                                   EPI == GEMM_EPI_SCORE);
  static constexpr int TCS = BM * 2 + 64;
  static constexpr int TBYTES = TSTG ? BN * TCS : 0;
  static constexpr int LDS_A = (NS * SLOT > OBYTES + XBYTES) ? NS * SLOT : OBYTES + XBYTES;
  static constexpr int LDS_BYTES = LDS_A > TBYTES ? LDS_A : TBYTES;
  static_assert((NS - 1) * NL <= 63, "vmcnt range");
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  // the coalesced store of the staged tile
  static constexpr int CPR = BN * (int)sizeof(TO) / 16;  // 16-byte chunks per output row
  static constexpr int OEPC = 16 / (int)sizeof(TO);
  static constexpr int ITERS = BM * CPR / NT;
  static constexpr int CPR128 = 128 * (int)sizeof(TO) / 16;  // chunks per 128-column score group
  // Adam on the dW tile: chunks per thread loaded (p / m / v) before any is stored
  static constexpr int A_AG = ITERS < 4 ? ITERS : 4;
  static_assert(ITERS % A_AG == 0, "Adam chunk groups");
  // (not for the 8-wave 256x128 / 128x256 tiles: their 48 prefetch registers
  // spill beside the larger accumulator set)
  static constexpr bool APF_OK = EPI == GEMM_EPI_BWD_WEIGHT && !BIG && CFG != 1 && CFG != 2 &&
                                 3 * NL + 3 * A_AG <= 63;
  // bwd-data BN partials: thread groups per column, 16-row pieces, pieces per thread
  static constexpr int B_NG = NT / BN, B_PIECES = BM / 16;
  static constexpr int B_PPT = (B_PIECES + B_NG - 1) / B_NG;
  static constexpr bool BPF_OK = EPI == GEMM_EPI_BWD_DATA && !BIG && B_PIECES % B_NG == 0 && B_PPT <= 2 &&
                                 3 * NL + 16 * B_PPT <= 63;


  // The body of one output tile; `bid` / `nblk` = the block index / block count.
  // Persistent CFG 7 (mmad_gemm_kernel_p): `pre` = this tile's first two K
  // stages were issued by the previous tile's epilogue; `next_bid` >= 0 = issue
  // that tile's first two stages at the start of this tile's epilogue (its
  // stores then drain under the next tile's prologue instead of before it).
  // (PST: the persistent kernel's own instantiation -- shared with the ordinary
  // kernel, the body's lambdas would have two callers and stay out of line)
  template <bool PST>
  static __device__ __forceinline__ void gemm_body(const T* __restrict__ A, int lda, const T* __restrict__ B,
                                                   int ldb, int K, const GemmEpi& ep, const int bid,
                                                   const int nblk, const int tid_in, const bool pre = false,
                                                   const int next_bid = -1) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    const int tid = tid_in, lane = tid & 63, w = tid >> 6;
    const int wm = w / WN, wn = w % WN;
    const int S = ep.splitk > 1 ? ep.splitk : 1;
    const int ntl = nblk / S;                 // output tiles
    const TileCoord tc = tile_coord(ep, bid, nblk, S);
    const int tm = tc.tm, tn = tc.tn, tile = tc.tile, sk = tc.sk;
    const int m0 = tm * BM, n0 = tn * BN;
    const int Ks = K / S, kbase = sk * Ks;
    const int nt = (ep.dbg & 1) ? 0 : Ks / IA::BK;

    floatx4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    // ---- epilogue constants, loaded before the main loop: their latency hides
    // under it instead of stalling the epilogue.  (Ordinary loads older than
    // every LDS-DMA of the ring; only used after the loop.)
    const int g = lane >> 4, c = lane & 15;
    const int rw = m0 + wm * 16 * TM;  // first row of this wave
    const int cw = n0 + wn * 16 * TN;  // first col of this wave
    float e_b[TN], e_s[TN], e_t[TN], e_p[TN][QB > 0 ? QB : 1];
    // (the 256x256 tile loads them after the loop: no registers to spare)
    auto load_epi_consts = [&]() {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = cw + j * 16 + c;
        e_b[j] = ep.bias ? ep.bias[col] : 0.f;
        e_s[j] = ep.bn_scale ? ep.bn_scale[col] : 1.f;
        e_t[j] = ep.bn_shift ? ep.bn_shift[col] : 0.f;
        if (EPI != GEMM_EPI_SCORE && ep.bpart) {
          // folded-BN bias partials: lane group g takes partials g, g+4, ...
#pragma unroll
          for (int q = 0; q < QB; ++q) {
            const int pp = min(g + 4 * q, ep.bparts - 1);
            e_p[j][q] = ep.bpart[(size_t)pp * ep.bpstride + col];
          }
        }
      }
    };
    if constexpr (FWDLIKE && !BIG && !XST) load_epi_consts();

    // fused BN: this column's barrier generation, read before this block can
    // arrive (its latency hides under the main loop)
    unsigned gen0 = 0u;
    if constexpr (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_BWD_DATA) {
      if (ep.bn_sync && tid == 0) gen0 = col_gen(ep.bn_sync + tn);
    }
    // BatchNorm parameters / statistics of this thread's column (tid % BN, the
    // epilogues' column), read before the main loop: their round trip hides
    // under it instead of following the loop or the column barrier
    float bnp_g = 0.f, bnp_b = 0.f, bnp_rm = 0.f, bnp_rv = 0.f, bnp_mu = 0.f, bnp_rs = 0.f;
    if constexpr ((EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_BWD_DATA) && !BIG) {
      const int bc = n0 + tid % BN;
      const int bcc = bc < ep.N ? bc : ep.N - 1;   // clamped: an unconditional load
      if constexpr (EPI == GEMM_EPI_FWD) {
        if (ep.bn_sync) {
          bnp_g = ep.bn_gamma[bcc];
          bnp_b = ep.bn_beta[bcc];
          if (ep.bn_rmean && tm == 0) {
            bnp_rm = ep.bn_rmean[bcc];
            bnp_rv = ep.bn_rvar[bcc];
          }
        }
      } else {
        if (ep.bn_part) {
          bnp_mu = ep.bn_mean[bc];
          bnp_rs = ep.bn_rstd[bc];
        }
        if (ep.bn_sync) bnp_g = ep.bn_gamma[bcc];
      }
    }
    float e_g[QG];
    // db[n] (bias gradient of this layer's output n) is needed by the dW fix-up
    // (BN producer) and by the fused bias Adam (column-tile-0 blocks)
    const bool need_db = EPI == GEMM_EPI_BWD_WEIGHT && ep.gb_src &&
                         (ep.b_scale || (ep.sm_p && tn == 0));
    if constexpr (EPI == GEMM_EPI_BWD_WEIGHT) {
      if (ep.b_scale) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = cw + j * 16 + c;
          e_s[j] = ep.b_scale[col];
          e_t[j] = ep.b_shift[col];
        }
      }
      if (need_db) {
        // db[n] partials of this block's rows, one row per thread (tid < BM)
        if (tid < BM) {
#pragma unroll
          for (int q = 0; q < QG; ++q) {
            const int pp = min(q, ep.gb_parts - 1);
            e_g[q] = ep.gb_src[(size_t)pp * ep.gb_stride + m0 + tid];
          }
        }
      }
    }

    auto issue = [&](int s) {
      char* base = smem + (s % NS) * SLOT;
      const int k0 = kbase + s * IA::BK;
      issue_stage<T, AK, BM, NT>(base, A, lda, m0, k0, tid);
      issue_stage<T, BK_, BN, NT>(base + IA::BYTES, B, ldb, n0, k0, tid);
    };
    // chunk q (< NL) of stage s: A chunks first, then B
    auto issue_q = [&](int s, int q) {
      char* base = smem + (s % NS) * SLOT;
      const int k0 = kbase + s * IA::BK;
      // persistent body: the chunk's source address is recomputed at every
      // issue (an opaque thread index): hoisted out of the K loop, the 64-bit
      // addresses of every chunk stay live across it and spill, and each
      // scratch reload's vmcnt wait drains the DMA ring
      int t = tid;
      if constexpr (PST) asm volatile("" : "+v"(t));
      if (q < IA::CHUNKS) issue_chunk<T, AK, BM, NT>(base, A, lda, m0, k0, t, q);
      else issue_chunk<T, BK_, BN, NT>(base + IA::BYTES, B, ldb, n0, k0, t, q - IA::CHUNKS);
    };

    // ---- main loop: NS-slot LDS ring, all slots in flight; fragment registers
    // double-buffered one sub-step ahead.  Per stage t:
    //   F1 <- (t, sub 1) issued between the two MFMA halves of F0 = (t, sub 0);
    //   wait stage t+1 landed + own reads of slot t done; barrier; refill slot t
    //   with stage t+NS; F0 <- (t+1, sub 0) between the two halves of F1.
    // The loop bodies are straight-line (peeled: issue phase / tail / last) so
    // hipcc's lgkmcnt bookkeeping stays exact, and sched_barriers pin the order.
    const int ra = wm * 16 * TM, rb = wn * 16 * TN;
    // Adam-fused dW: the first chunk group of the tile's p / m / v is loaded
    // right after the ring's last DMA issue, so its HBM round trip runs under
    // the K loop's last NS-1 stages instead of after the loop (the tail waits
    // let these APF younger loads stay in flight; APF = 0: not prefetched)
    floatx4 pf_p[A_AG], pf_m[A_AG], pf_v[A_AG];
    bool pf = false;
    auto adam_prefetch = [&]() {
#pragma unroll
      for (int u = 0; u < A_AG; ++u) {
        const int idx = u * NT + tid;
        const size_t off = (size_t)(m0 + idx / CPR) * ep.ldo + n0 + (idx % CPR) * (16 / (int)sizeof(TO));
        pf_p[u] = *(const floatx4*)(ep.ad_p + off);
        pf_m[u] = *(const floatx4*)(ep.ad_m + off);
        pf_v[u] = *(const floatx4*)(ep.ad_v + off);
      }
    };
    // the layer's small Adam segment [bias | gamma | beta] this block updates in
    // its epilogue (bias: the column-tile-0 blocks, one row per thread; gamma |
    // beta: 4 per thread of the first tiles): read before the main loop, as
    // nothing else writes it during this launch and its gradients are final
    float smp_p = 0.f, smp_m = 0.f, smp_v = 0.f;
    floatx4 smq_g{}, smq_p{}, smq_m{}, smq_v{};
    bool smq = false;
    if constexpr (APF_OK) {
      if (ep.sm_p) {
        if (tn == 0 && tid < BM && m0 + tid < ep.sm_bNp) {
          smp_p = ep.sm_p[m0 + tid];
          smp_m = ep.sm_m[m0 + tid];
          smp_v = ep.sm_v[m0 + tid];
        }
        const int i4 = ep.sm_bNp + (tile * NT + tid) * 4;
        if (i4 < ep.sm_n) {
          smq_g = *(const floatx4*)(ep.sm_g + i4);
          smq_p = *(const floatx4*)(ep.sm_p + i4);
          smq_m = *(const floatx4*)(ep.sm_m + i4);
          smq_v = *(const floatx4*)(ep.sm_v + i4);
          smq = true;
        }
      }
    }
    // bwd-data with the BatchNorm-backward partials: this thread's pre-BN
    // activations a (16 rows x PPT pieces of one column, the epilogue's own
    // pattern) prefetched the same way, raw (converted only where used)
    TO pf_a[BPF_OK ? B_PPT : 1][16];
    bool pfa = false;
    auto bn_a_prefetch = [&]() {
      const TO* an = (const TO*)ep.bn_a;
      const int cc = tid % BN, grp = tid / BN;
#pragma unroll
      for (int u = 0; u < B_PPT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          pf_a[u][r] = an[(size_t)(m0 + (grp + u * B_NG) * 16 + r) * ep.ldo + n0 + cc];
    };
    if constexpr (BIG) {
      // 256x256 tile (bf16, both operands K-major): a 2-slot ring, one barrier
      // per stage after both 32-deep sub-steps; the fragment registers of a
      // sub-step are re-read row by row under the MFMAs that free them (their
      // lifetimes do not overlap, so the 128 accumulators fit beside them), and
      // stage t+2 is issued over the MFMA rows of stage t+1's first sub-step
      // (the round-3 loop study's "256x256 nb2 st0 di1", profiles/r03d_*)
      if (nt > 0) {
        FR fa[2][TM], fb[2][TN];
        auto rd = [&](int t, int kk, int sl) {
          const char* base = smem + (t % NS) * SLOT;
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[sl][i] = frag_bf16<true, true, BM>(base, ra + i * 16, kk, lane);
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[sl][j] = frag_bf16<true, true, BN>(base + IA::BYTES, rb + j * 16, kk, lane);
        };
        int pend = -1;
        // diagnostics (dbg bit 16, loop studies only): no DMA after the
        // prologue (the MFMAs read stale slots)
        const bool d_nodma = ep.dbg & 16;
        if (!(PST && pre)) {
          issue(0);
          if (nt > 1) issue(1);
        }
        // (pre: the previous tile's epilogue stores are younger than these
        // stages -- wait for everything)
        if (nt > 1 && !(PST && pre)) wait_vmcnt<NL>();
        else wait_vmcnt<0>();
        block_barrier();
        rd(0, 0, 0);
        for (int t = 0; t < nt; ++t) {
          const char* base = smem + (t % NS) * SLOT;
#pragma unroll
          for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = XST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[0][j], fa[0][i], acc[i][j], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
            if (pend >= 0 && !d_nodma) {
#pragma unroll
              for (int q = 0; q < NL; ++q)
                if (q * TM / NL == i) issue_q(pend, q);
            }
            if (i == 0) {
#pragma unroll
              for (int j = 0; j < TN; ++j)
                fb[1][j] = frag_bf16<true, true, BN>(base + IA::BYTES, rb + j * 16, 1, lane);
            }
            fa[1][i] = frag_bf16<true, true, BM>(base, ra + i * 16, 1, lane);
          }
          pend = -1;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = XST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[1][j], fa[1][i], acc[i][j], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][i], fb[1][j], acc[i][j], 0, 0, 0);
          if (t + 1 < nt) {
            wait_vmcnt<0>();                   // stage t+1 landed (the only one in flight)
            wait_lgkm0();
            block_barrier();                   // stage t+1 visible; slot t free
            if (t + 2 < nt) pend = t + 2;
            rd(t + 1, 0, 0);
          }
        }
      }
    } else if (nt > 0) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        if (s < nt) issue(s);
      if (nt >= NS) wait_vmcnt<(NS - 1) * NL>();
      else wait_vmcnt<0>();
      block_barrier();
      FR f0a[TM], f0b[TN], f1a[TM], f1b[TN];
      read_sub<T, AK, BK_, NAT, BM, BN, TM, TN>(smem, smem + IA::BYTES, ra, rb, 0, lane, f0a, f0b);
      wait_lgkm0();
      auto step = [&](int t, auto issue_c, auto last_c, auto pf_c) {
        constexpr bool ISSUE = decltype(issue_c)::value, LAST = decltype(last_c)::value;
        constexpr bool PF = decltype(pf_c)::value;   // the Adam prefetch is in flight
        const char* sa = smem + (t % NS) * SLOT;
        mma_half<T, TM, TN, 0, XST>(acc, f0a, f0b);
        MMAD_SB();
        read_sub<T, AK, BK_, NAT, BM, BN, TM, TN>(sa, sa + IA::BYTES, ra, rb, 1, lane, f1a, f1b);
        MMAD_SB();
        mma_half<T, TM, TN, 1, XST>(acc, f0a, f0b);
        MMAD_SB();
        if constexpr (!LAST) {
          if constexpr (ISSUE) {
            wait_vmcnt<(NS - 2) * NL>();
          } else if constexpr (PF && APF_OK) {
            wait_tail_x<NL, 3 * A_AG>(nt - t - 2);
          } else if constexpr (PF && BPF_OK) {
            wait_tail_x<NL, 16 * B_PPT>(nt - t - 2);
          } else {
            wait_tail<NL>(nt - t - 2);
          }
          wait_lgkm0();
          block_barrier();                     // stage t+1 visible; slot t free
          MMAD_SB();
        }
        // stage t+NS into the freed slot t, spread over this sub-step's MFMA rows
        auto dma_row = [&](int i) {
          if constexpr (ISSUE) {
#pragma unroll
            for (int q = 0; q < NL; ++q)
              if (q * TM / NL == i) issue_q(t + NS, q);
          }
        };
        mma_half<T, TM, TN, 0, XST>(acc, f1a, f1b, dma_row);
        MMAD_SB();
        if constexpr (!LAST) {
          const char* sn = smem + ((t + 1) % NS) * SLOT;
          read_sub<T, AK, BK_, NAT, BM, BN, TM, TN>(sn, sn + IA::BYTES, ra, rb, 0, lane, f0a, f0b);
        }
        MMAD_SB();
        mma_half<T, TM, TN, 1, XST>(acc, f1a, f1b, dma_row);
        MMAD_SB();
      };
      using T_ = std::true_type;
      using F_ = std::false_type;
      int t = 0;
      bool apf = false;
      if constexpr (APF_OK) apf = ep.ad_p != nullptr && nt > NS;
      if constexpr (BPF_OK) apf = ep.bn_part != nullptr && ep.bn_a != nullptr && nt > NS;
      if (apf) {
        // the last issuing stage, then the prefetch behind its DMA
        for (; t < nt - NS - 1; ++t) step(t, T_{}, F_{}, F_{});
        step(t++, T_{}, F_{}, F_{});
        MMAD_SB();
        if constexpr (APF_OK) {
          adam_prefetch();
          pf = true;
        }
        if constexpr (BPF_OK) {
          bn_a_prefetch();
          pfa = true;
        }
        MMAD_SB();
        for (; t < nt - 1; ++t) step(t, F_{}, F_{}, T_{});
        step(nt - 1, F_{}, T_{}, T_{});
      } else {
        for (; t < nt - NS; ++t) step(t, T_{}, F_{}, F_{});
        for (; t < nt - 1; ++t) step(t, F_{}, F_{}, F_{});
        step(nt - 1, F_{}, T_{}, F_{});
      }
    }

    // ---- split-K combine (ticket first, no spin on a block that has not run):
    // the first S-1 blocks of a tile to finish publish their partial tile as an
    // sc1 (write-through) slab + flag; the last one adds the slabs in split
    // order (p0 + p1 + ... : independent of arrival order) and runs the
    // epilogue.  Counters / flags start at 0 (caller memset) and the last block
    // resets them, so consecutive launches on one stream reuse them.
    // (the 256x256 tile never splits: its combine would need a second set of
    // 128 accumulator registers; the dispatcher does not pick it for a split)
    if (!BIG && S > 1) {
      unsigned* cnt = ep.sk_ctl + tile;
      unsigned* flg = ep.sk_ctl + ntl + (size_t)tile * S;
      __syncthreads();
      unsigned* shw = (unsigned*)smem;
      if (tid == 0) shw[0] = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const unsigned ticket = shw[0];
      float* slab_t = ep.sk_slab + (size_t)tile * S * (BM * BN);
      const int frag0 = w * TM * TN;
      if (ticket + 1 < (unsigned)S) {
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(slab_t + (size_t)sk * (BM * BN), 0, BM * BN * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, acc[i][j]), rs,
                                                   ((frag0 + i * TN + j) * 64 + lane) * 16, 0, 16 /*sc1*/);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(flg + sk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
      if (tid == 0) {
        // a slice that never publishes (it cannot happen with every block of
        // the grid resident or queued, but a bounded spin must not combine a
        // stale slab): flag the launch as failed and skip the epilogue; the
        // host reads the word with mmad_gemm_status / mmad_ae_status.
        // dbg bit 4 forces the timeout path (tests).
        unsigned timed_out = 0u;
        for (int s2 = 0; s2 < S; ++s2) {
          if (s2 == sk) continue;
          bool ok = false;
          if (!(ep.dbg & 4)) {
            for (unsigned spins = 0; spins < (1u << 24); ++spins) {
              if (__hip_atomic_load(flg + s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                ok = true;
                break;
              }
              __builtin_amdgcn_s_sleep(1);
            }
          }
          if (!ok) timed_out = 1u;
          __hip_atomic_store(flg + s2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (timed_out)
          __hip_atomic_store(ep.sk_ctl + MMAD_SK_ERR_WORD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        shw[1] = timed_out;
      }
      __syncthreads();
      if (shw[1]) return;
      asm volatile("" ::: "memory");           // every slab load below is sc1
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(slab_t, 0, S * BM * BN * 4, 0x00020000);
      // Every load is unconditional and issued before any use (a select of
      // "register or load" per fragment would make hipcc branch around each
      // load and wait for it: one memory round trip per fragment).
      if (S == 2) {
        // p0 + p1 == p1 + p0 (IEEE addition commutes): arrival order is irrelevant
        const int other = (1 - sk) * BM * BN * 4;
        floatx4 ob[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            ob[i][j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       rs, other + ((frag0 + i * TN + j) * 64 + lane) * 16, 0, 16));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] += ob[i][j];
      } else {
        // ((p0 + p1) + p2) + ... in split order, G slabs per round trip (slot
        // sk was never written: loaded anyway, then replaced by acc).  G = 2
        // / 1 for the larger wave tiles (register budget: no spills).
        constexpr int G = TM * TN <= 4 ? 4 : (TM * TN <= 8 ? 2 : 1);
        floatx4 r[TM][TN];
        for (int t0 = 0; t0 < S; t0 += G) {
          floatx4 lb[G][TM][TN];
#pragma unroll
          for (int u = 0; u < G; ++u)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                lb[u][i][j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                              rs, (t0 + u) * BM * BN * 4 + ((frag0 + i * TN + j) * 64 + lane) * 16, 0, 16));
                asm volatile("" : "+v"(lb[u][i][j]));   // materialise: no branch around the load
              }
#pragma unroll
          for (int u = 0; u < G; ++u) {
            const int t = t0 + u;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                const floatx4 e = t == sk ? acc[i][j] : lb[u][i][j];
                r[i][j] = t == 0 ? e : r[i][j] + e;
              }
          }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = r[i][j];
      }
    }

    if (ep.dbg & 2) {  // diagnostics: main loop only (keep acc live)
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) sum += acc[i][j][0];
      if (sum == 1.2345e-30f) ((float*)ep.out)[tid] = sum;
      return;
    }
    if constexpr (XST) {
      if (PST && next_bid >= 0) {
        // persistent: the next tile's first two K stages into the ring now (every
        // wave has consumed its last fragments: the barrier orders the refill)
        __syncthreads();
        const TileCoord nc = tile_coord(ep, next_bid, nblk, 1);
#pragma unroll
        for (int st2 = 0; st2 < 2; ++st2) {
          if (st2 < nt) {
            char* base = smem + st2 * SLOT;
            issue_stage<T, AK, BM, NT>(base, A, lda, nc.tm * BM, st2 * IA::BK, tid);
            issue_stage<T, BK_, BN, NT>(base + IA::BYTES, B, ldb, nc.tn * BN, st2 * IA::BK, tid);
          }
        }
      }
      // ===================== CFG 7 epilogue (registers -> HBM) ================
      // acc[i][j] of lane (c, g): output row rw + i*16 + c, columns
      // cw + j*16 + 4g .. +3 (W was the MFMA's first operand).  Per element the
      // same arithmetic as the row-quad epilogue below: act(acc + bias), then
      // the BN-eval affine, masked outside M x N, rounded to bf16.  Column tiles
      // 2h and 2h+1 are stored together: v_permlane16_swap of their quads gives
      // lane g the 8 columns 8(g>>1) .. +7 of tile 2h + (g&1) (16 B).
      // (piecewise-linear activations only: LeakyReLU / ReLU / none; sigmoid /
      // tanh layers run on CFG 6, tile_runs)
      const bool pw_relu = ep.act == MMAD_ACT_RELU;
      const float pw_lo = act_lo_slope(ep.act, ep.slope);
      auto cvec = [&](const float* p, int col, float dflt) -> floatx4 {
        return p ? *(const floatx4*)(p + col) : floatx4{dflt, dflt, dflt, dflt};
      };
      TO* out = (TO*)ep.out;
      const int jl = g & 1, coff = 8 * (g >> 1);
      // score: every reference chunk of the tile loaded in one round trip when
      // they fit (TM x TN/2 <= 8 chunks: the 256x128 tile), per column pair
      // otherwise
      constexpr bool REF_ALL = EPI == GEMM_EPI_SCORE && TM * (TN / 2) <= 8;
      uint4v rall[REF_ALL ? TN / 2 : 1][REF_ALL ? TM : 1];
      if constexpr (REF_ALL) {
        // (one branch around the whole group: a per-chunk "ref ? load : 0"
        // becomes a branch and a wait per load)
        if (ep.ref) {
#pragma unroll
          for (int h = 0; h < TN / 2; ++h)
#pragma unroll
            for (int i = 0; i < TM; ++i)
              rall[h][i] = *(const uint4v*)((const TO*)ep.ref + (size_t)(rw + i * 16 + c) * ep.ldref + cw +
                                            (2 * h + jl) * 16 + coff);
        } else {
#pragma unroll
          for (int h = 0; h < TN / 2; ++h)
#pragma unroll
            for (int i = 0; i < TM; ++i) rall[h][i] = uint4v{0u, 0u, 0u, 0u};
        }
      }
      float rsum[EPI == GEMM_EPI_SCORE ? TM : 1];   // this wave's 64-column row sums (WN = 4)
      float rsum2[EPI == GEMM_EPI_SCORE ? TM : 1][2];   // (WN = 2) the two 64-column halves
#pragma unroll
      for (int h = 0; h < TN / 2; ++h) {
        floatx4 cb[2], cs[2], ct[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int col = cw + (2 * h + u) * 16 + 4 * g;
          cb[u] = cvec(ep.bias, col, 0.f);
          cs[u] = cvec(ep.bn_scale, col, 1.f);
          ct[u] = cvec(ep.bn_shift, col, 0.f);
        }
        const int col0 = cw + (2 * h + jl) * 16 + coff;   // this lane's chunk after the swap
        uint4v rvs[EPI == GEMM_EPI_SCORE ? TM : 1];
        if constexpr (EPI == GEMM_EPI_SCORE) {
          if constexpr (REF_ALL) {
#pragma unroll
            for (int i = 0; i < TM; ++i) rvs[i] = rall[h][i];
          } else if (ep.ref) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
              rvs[i] = *(const uint4v*)((const TO*)ep.ref + (size_t)(rw + i * 16 + c) * ep.ldref + col0);
          } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) rvs[i] = uint4v{0u, 0u, 0u, 0u};
          }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = rw + i * 16 + c;
          unsigned d[2][2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int j = 2 * h + u;
            bf16x4 q;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int col = cw + j * 16 + 4 * g + r;
              float v = acc[i][j][r];
              v = fmaf(apply_act_pw(v + cb[u][r], pw_relu, pw_lo), cs[u][r], ct[u][r]);
              v = (row < ep.M && col < ep.N) ? v : 0.f;
              q[r] = (bf16)v;
            }
            const uint2v qq = __builtin_bit_cast(uint2v, q);
            d[u][0] = qq[0];
            d[u][1] = qq[1];
          }
          const auto s0 = __builtin_amdgcn_permlane16_swap(d[0][0], d[1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(d[0][1], d[1][1], false, false);
          const uint4v v = uint4v{s0[0], s1[0], s0[1], s1[1]};
          if (out) *(uint4v*)(out + (size_t)row * ep.ldo + col0) = v;
          if constexpr (EPI == GEMM_EPI_SCORE) {
            const TO* pv = (const TO*)&v;
            const TO* pr = (const TO*)&rvs[i];
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
              const floatx4 w4 = cvec(ep.colw, col0 + e, 1.f);
              wv[e] = w4[0]; wv[e + 1] = w4[1]; wv[e + 2] = w4[2]; wv[e + 3] = w4[3];
            }
            float sq = 0.f, dd[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              dd[e] = to_f32<TO>(pv[e]) - to_f32<TO>(pr[e]);
              sq = fmaf(dd[e] * dd[e], wv[e], sq);
            }
            if (ep.diff && row < ep.M) {
              float* dp = ep.diff + (size_t)row * ep.lddiff + col0;
#pragma unroll
              for (int e = 0; e < 8; ++e)
                if (col0 + e < ep.N) dp[e] = dd[e];
            }
            // chunks 4h + {0, 1, 2, 3} of the wave's 8 sit in lanes g = 0, 2,
            // 1, 3: (k0 + k1) + (k2 + k3), the row-major butterfly's order
            sq += lane_xor32(sq);
            sq += lane_xor16(sq);
            if constexpr (TN == 4) {
              rsum[i] = h == 0 ? sq : rsum[i] + sq;
            } else {
              // 128 columns per wave: ((Q0 + Q1) + (Q2 + Q3)), written here
              static_assert(TN == 8, "one 128-column group per wave");
              if (h == 0 || h == 2) rsum2[i][h >> 1] = sq;
              else rsum2[i][h >> 1] = rsum2[i][h >> 1] + sq;
              if (h == 3 && g == 0)
                ep.rowsq[(size_t)(cw >> 7) * ep.ldrow + row] = rsum2[i][0] + rsum2[i][1];
            }
          }
        }
      }
      if constexpr (EPI == GEMM_EPI_SCORE && TN == 4) {
        // the two waves of a 128-column group: (k0..k7) + (k8..k15), through
        // [WN][BM] floats of LDS (a persistent block's: behind the ring, which
        // its next tile's stages fill; otherwise at its start)
        static_assert(!PST || NS * SLOT + WN * BM * 4 <= LDS_BYTES, "row-sum exchange beside the ring");
        float* srs = (float*)(smem + (PST ? NS * SLOT : 0));
        __syncthreads();                           // ring reads / every wave's row sums below
        if (g == 0) {
#pragma unroll
          for (int i = 0; i < TM; ++i) srs[wn * BM + wm * 16 * TM + i * 16 + c] = rsum[i];
        }
        __syncthreads();
        constexpr int GROUPS = BN / 128;
        static_assert(WN == 2 * GROUPS && NT >= GROUPS * BM, "two waves per 128-column group");
        if (tid < GROUPS * BM) {
          const int gi = tid / BM, rl = tid % BM;
          const float tot = srs[(2 * gi) * BM + rl] + srs[(2 * gi + 1) * BM + rl];
          ep.rowsq[(size_t)((n0 >> 7) + gi) * ep.ldrow + m0 + rl] = tot;
        }
      }
      return;
    }
    if constexpr (FWDLIKE && BIG) load_epi_consts();
    // ===================== epilogue, register phase ==========================
    // per-call values of a graph-captured step come from device memory
    const float* tgt = ep.target;
    float ad_step = ep.ad_step, ad_bc2 = ep.ad_bc2;
    if (ep.dyn) {
      if constexpr (EPI == GEMM_EPI_MSE) tgt = ep.dyn->x;
      if constexpr (EPI == GEMM_EPI_BWD_WEIGHT) {
        ad_step = ep.dyn->ad_step;
        ad_bc2 = ep.dyn->ad_bc2;
      }
    }
    float db_own = 0.f;                        // db[m0 + tid] (tid < BM, need_db)
    if constexpr (EPI == GEMM_EPI_BWD_WEIGHT) {
      if (need_db && tid < BM) {
        // sequential partial order (= the flat reduction's)
#pragma unroll
        for (int q = 0; q < QG; ++q) db_own += q < ep.gb_parts ? e_g[q] : 0.f;
        for (int q = QG; q < ep.gb_parts; ++q) db_own += ep.gb_src[(size_t)q * ep.gb_stride + m0 + tid];
      }
      if (ep.b_scale) {
        __syncthreads();                       // ring LDS no longer read
        float* gbl = (float*)smem;
        if (tid < BM) gbl[tid] = db_own;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float db = gbl[wm * 16 * TM + i * 16 + 4 * g + r];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j][r] = fmaf(e_s[j], acc[i][j][r], e_t[j] * db);
          }
      }
    }
    // activations: the piecewise-linear ones (LeakyReLU / ReLU / none, the hot
    // path) are applied branch-free inside the register phase below; the
    // others (sigmoid / tanh, FWD / SCORE only) by a pre-pass over the
    // accumulators, acc = act(acc + bias) -- the same value the fused form
    // computes -- after which the register phase applies no activation.  One
    // instance of the register phase either way (two instances cost registers:
    // spills in the 256-row tiles).
    const bool pw_act = !FWDLIKE || EPI == GEMM_EPI_MSE || act_is_linear_piecewise(ep.act);
    const bool pw_relu = ep.act == MMAD_ACT_RELU;
    const float pw_lo = act_lo_slope(ep.act, ep.slope);
    float ebias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = cw + j * 16 + c;
      float bias = 0.f;
      if constexpr (FWDLIKE) {
        bias = e_b[j];
        if (EPI != GEMM_EPI_SCORE && ep.bpart) {
          // + sum_k shift[k] W[n][k]: lane-group sums, then ((g0+g1)+(g2+g3))
          float t = 0.f;
#pragma unroll
          for (int q = 0; q < QB; ++q) t += g + 4 * q < ep.bparts ? e_p[j][q] : 0.f;
          for (int p = 4 * QB + g; p < ep.bparts; p += 4) t += ep.bpart[(size_t)p * ep.bpstride + col];
          t = sum_lane_groups(t);
          bias += t;
        }
      }
      ebias[j] = bias;
    }
    if constexpr (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_SCORE) {
      if (!pw_act) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = apply_act(acc[i][j][r] + ebias[j], ep.act, ep.slope);
      }
    }
    // MSE: every target value of this lane's accumulators loaded up front, all
    // in flight together (issued inside the loop below they went out a column
    // fragment at a time, one HBM round trip each); the fragment registers of
    // the finished K loop hold them.  Same values, same arithmetic.  c3's MSE
    // GEMM (4096 x 1658 -> 2048) 51.2 -> 39.9 us on its tile, c2's 18.9 -> 16.0
    // (profiles/r10/r10h_mse_target_prefetch_ab.jsonl).  bf16 only: the fp32
    // tiles would spill.
    constexpr bool TPF = EPI == GEMM_EPI_MSE && sizeof(T) == 2 && TM * TN <= 16;
    float tpf[TPF ? TN : 1][TPF ? TM : 1][4];
    if constexpr (TPF) {
      int trow[TM][4];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) trow[i][r] = (rw + i * 16 + 4 * g + r) % ep.tmod;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = cw + j * 16 + c;
        const int cc = col < ep.N ? col : ep.N - 1;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) tpf[j][i][r] = tgt[(size_t)trow[i][r] * ep.ldt + cc];
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = cw + j * 16 + c;
      const bool cvalid = col < ep.N;
      const float bias = ebias[j];
      float sc = 1.f, sh = 0.f;
      if constexpr (FWDLIKE) {
        sc = e_s[j];
        sh = e_t[j];
      }
      float s1[TM / 2], s2[TM / 2];
#pragma unroll
      for (int p = 0; p < TM / 2; ++p) { s1[p] = 0.f; s2[p] = 0.f; }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rw + i * 16 + 4 * g + r;
          const bool valid = cvalid && row < ep.M;
          float v = acc[i][j][r];
          if (EPI == GEMM_EPI_FWD || EPI == GEMM_EPI_SCORE) {
            // pinned: tile-independent (act already applied by the pre-pass
            // when it is not piecewise-linear)
            const float a = apply_act_pw(v + bias, pw_relu, pw_lo);
            v = fmaf(pw_act ? a : v, sc, sh);
            v = valid ? v : 0.f;
            s1[i >> 1] += v;
          } else if (EPI == GEMM_EPI_MSE) {
            // unconditional load at a clamped column (row % tmod is always a
            // target row): a load guarded per element makes hipcc branch around
            // each one and wait for it, one round trip per element
            const float tv = TPF ? tpf[TPF ? j : 0][TPF ? i : 0][r]
                                 : tgt[(size_t)(row % ep.tmod) * ep.ldt + (col < ep.N ? col : ep.N - 1)];
            const float d = valid ? v + bias - tv : 0.f;
            v = ep.gscale * d;
            s1[i >> 1] += v;
            s2[i >> 1] += d * d;
          } else if (EPI == GEMM_EPI_BWD_DATA) {
            v = valid ? v : 0.f;
            s1[i >> 1] += v;
          }
          acc[i][j][r] = v;
        }
      }
      if (ep.part) {
#pragma unroll
        for (int p = 0; p < TM / 2; ++p) {
          float a1 = s1[p];
          if constexpr (EPI == GEMM_EPI_BWD_DATA) {
            // (the same value through ds_bpermute: the lane-swap form's two
            // temporaries per reduction spill the fused-BN bwd-data tiles)
            a1 += __shfl_xor(a1, 16);
            a1 += __shfl_xor(a1, 32);
          } else {
            a1 = sum_lane_groups(a1);
          }
          const int crow = rw + p * 32;
          const int chunk = crow / MMAD_PART_ROWS;
          float* part = ep.part + (size_t)chunk * 2 * ep.ldpart;
          if (EPI == GEMM_EPI_FWD) {
            // Welford partial: mean and M2 of the valid rows of this 32-row chunk
            int cnt = ep.M - crow;
            cnt = cnt < 0 ? 0 : (cnt > 32 ? 32 : cnt);
            const float mean = cnt > 0 ? a1 / (float)cnt : 0.f;
            float q = 0.f;
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = crow + ii * 16 + 4 * g + r;
                const float dv = acc[2 * p + ii][j][r] - mean;
                q += (row < ep.M) ? dv * dv : 0.f;
              }
            q = sum_lane_groups(q);
            if (g == 0 && !(ep.dbg & 8)) {
              if (ep.bn_sync) {   // handed to the other blocks of this column: sc1
                st_sc1(part + col, mean);
                st_sc1(part + ep.ldpart + col, q);
              } else {
                part[col] = mean;
                part[ep.ldpart + col] = q;
              }
            }
          } else if (EPI == GEMM_EPI_MSE) {
            float a2 = s2[p];
            a2 = sum_lane_groups(a2);
            if (g == 0) { part[col] = a1; part[ep.ldpart + col] = a2; }
          } else if (EPI == GEMM_EPI_BWD_DATA) {
            if (g == 0) part[col] = a1;
          }
        }
      }
    }


    // ===================== epilogue, LDS-staged coalesced store ===============
    // fused BN (forward): the Welford partials are out -- arrive at the column
    // barrier now, store the a tile while the other blocks catch up
    unsigned* bn_shw = (unsigned*)(smem + OBYTES + XBYTES - 64);
    if constexpr (EPI == GEMM_EPI_FWD && !BIG) {
      if (ep.bn_sync) col_arrive(ep.bn_sync + tn, (unsigned)(ntl / ep.tiles_n), tid, bn_shw);
    }
    __syncthreads();  // main-loop LDS no longer read
    if constexpr (EPI == GEMM_EPI_MSE) {
      if (ep.lossp) {
        // one loss partial per output tile: sum of d^2 = sum (dz/gscale)^2
        float lt_sum = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) lt_sum += acc[i][j][r] * acc[i][j][r];
        lt_sum = wave_sum(lt_sum) / (ep.gscale * ep.gscale);
        float* red = (float*)smem;
        if (lane == 0) red[w] = lt_sum;
        __syncthreads();
        if (tid == 0) {
          float t = 0.f;
#pragma unroll
          for (int q = 0; q < NW; ++q) t += red[q];
          ep.lossp[tile] = t;
        }
        __syncthreads();
      }
    }
    // transposed staging for this tile.  Only the non-256 FWD tiles can carry a
    // fused BN (whose epilogue re-stages row-major): for every other forward-
    // type tile the choice is a compile-time constant, so the row-major path is
    // not instantiated beside it (registers).  dbg 512 (A/B): row-major b16.
    constexpr bool TSTG_ONLY = TSTG && (EPI != GEMM_EPI_FWD || BIG);
    const bool tstg = TSTG_ONLY ? true : (TSTG && !ep.bn_sync && !(ep.dbg & 512));
    auto tsw = [](int col) { return ((col >> 1) & 7) << 3; };
    if (TSTG && tstg) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int rl0 = wm * 16 * TM + i * 16 + 4 * g;
          const int cl = wn * 16 * TN + j * 16 + c;
          bf16x4 q;
#pragma unroll
          for (int r = 0; r < 4; ++r) q[r] = (bf16)acc[i][j][r];
          *(bf16x4*)(smem + cl * TCS + ((rl0 * 2) ^ tsw(cl))) = q;
        }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rl = wm * 16 * TM + i * 16 + 4 * g + r;
            const int cl = wn * 16 * TN + j * 16 + c;
            *(TO*)(smem + rl * OSTRIDE + cl * (int)sizeof(TO)) = from_f32<TO>(acc[i][j][r]);
          }
    }
    __syncthreads();
    TO* out = (TO*)ep.out;
    if (EPI == GEMM_EPI_BWD_WEIGHT && ep.ad_p) {
      // torch.optim.Adam on the dW tile (4 fp32 per chunk), same formula as
      // adam_k.  p/m/v of AG chunks are loaded before any of them is stored
      // (the three state arrays may alias as far as the compiler knows).
#pragma unroll
      for (int i0 = 0; i0 < ITERS; i0 += A_AG) {
        floatx4 P[A_AG], Mm[A_AG], Vv[A_AG];
        size_t off[A_AG];
#pragma unroll
        for (int u = 0; u < A_AG; ++u) {
          const int idx = (i0 + u) * NT + tid;
          const int rl = idx / CPR, ch = idx % CPR;
          off[u] = (size_t)(m0 + rl) * ep.ldo + n0 + ch * OEPC;
        }
        if (i0 == 0 && pf) {
          // the first group was loaded under the K loop (adam_prefetch)
#pragma unroll
          for (int u = 0; u < A_AG; ++u) {
            P[u] = pf_p[u];
            Mm[u] = pf_m[u];
            Vv[u] = pf_v[u];
          }
        } else {
#pragma unroll
          for (int u = 0; u < A_AG; ++u) {
            P[u] = *(const floatx4*)(ep.ad_p + off[u]);
            Mm[u] = *(const floatx4*)(ep.ad_m + off[u]);
            Vv[u] = *(const floatx4*)(ep.ad_v + off[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < A_AG; ++u) {
          const int idx = (i0 + u) * NT + tid;
          const int rl = idx / CPR, ch = idx % CPR;
          const uint4v v = *(const uint4v*)(smem + rl * OSTRIDE + ch * 16);
          if (!ep.dw_nostore) *(uint4v*)(out + off[u]) = v;
          adam4(P[u], Mm[u], Vv[u], __builtin_bit_cast(floatx4, v), ep.ad_w1, ep.ad_w2, ep.ad_eps,
                ad_step, ad_bc2);
          bf16x4 sh;
#pragma unroll
          for (int e = 0; e < 4; ++e) sh[e] = (bf16)P[u][e];
          *(floatx4*)(ep.ad_p + off[u]) = P[u];
          *(floatx4*)(ep.ad_m + off[u]) = Mm[u];
          *(floatx4*)(ep.ad_v + off[u]) = Vv[u];
          if (ep.ad_shadow) *(bf16x4*)((bf16*)ep.ad_shadow + off[u]) = sh;
        }
      }
    } else if (TSTG && tstg) {
      // read back row-major: iteration u covers a 16-row x 32-column block
      // (row block rb = wave's, column block cb); lane (n = lane & 15, g = lane >> 4)
      // gets row rbase + n, columns cbase + 8g .. + 7 (two tr-reads of 4), one
      // 16-B store.  A wave walks its row blocks, and per row block the column
      // blocks in order, so the 4 blocks of a 128-column score group are
      // consecutive iterations of one lane.
      constexpr int RB = BM / 16, CB = BN / 32, RBW = RB / NW, NB = RBW * CB;
      static_assert(!TSTG || (RB % NW == 0 && NB == ITERS), "transposed staging geometry");
      const int n16 = lane & 15, q4 = (lane >> 2) & 3, p4 = lane & 3;
      const MMAD_LDS char* lds = (const MMAD_LDS char*)smem;
      uint4v rvs[EPI == GEMM_EPI_SCORE ? NB : 1];
      if constexpr (EPI == GEMM_EPI_SCORE) {
        if (ep.ref) {
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int rbase = (w * RBW + u / CB) * 16, cbase = (u % CB) * 32;
            rvs[u] = *(const uint4v*)((const TO*)ep.ref + (size_t)(m0 + rbase + n16) * ep.ldref + n0 +
                                      cbase + 8 * g);
          }
        } else {
#pragma unroll
          for (int u = 0; u < NB; ++u) rvs[u] = uint4v{0u, 0u, 0u, 0u};
        }
      }
      float gpart[2] = {0.f, 0.f};   // SCORE: (T0 + T1), then T2 of one 128-column group
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int rbase = (w * RBW + u / CB) * 16, cbase = (u % CB) * 32;
        const int k1 = cbase + 8 * g + q4, k2 = k1 + 4;
        const int rb2 = (rbase + 4 * p4) * 2;
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (MMAD_LDS short4v*)(lds + k1 * TCS + (rb2 ^ tsw(k1))));
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (MMAD_LDS short4v*)(lds + k2 * TCS + (rb2 ^ tsw(k2))));
        const bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
        const bf16x8 v8 = __builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7);
        const uint4v v = __builtin_bit_cast(uint4v, v8);
        const int row = m0 + rbase + n16;
        const int col = n0 + cbase + 8 * g;
        if (out) *(uint4v*)(out + (size_t)row * ep.ldo + col) = v;
        if constexpr (EPI == GEMM_EPI_SCORE) {
          const uint4v rv = rvs[u];
          const TO* pv = (const TO*)&v;
          const TO* pr = (const TO*)&rv;
          float wv[8];
#pragma unroll
          for (int e = 0; e < 8; e += 4) {
            const floatx4 w4 = ep.colw ? *(const floatx4*)(ep.colw + col + e) : floatx4{1.f, 1.f, 1.f, 1.f};
            wv[e] = w4[0]; wv[e + 1] = w4[1]; wv[e + 2] = w4[2]; wv[e + 3] = w4[3];
          }
          float sq = 0.f, dd[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            dd[e] = to_f32<TO>(pv[e]) - to_f32<TO>(pr[e]);
            sq = fmaf(dd[e] * dd[e], wv[e], sq);
          }
          if (ep.diff && row < ep.M) {
            float* dp = ep.diff + (size_t)row * ep.lddiff + col;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (col + e < ep.N) dp[e] = dd[e];
          }
          // the 16 chunks k = 4 (cb % 4) + g of a 128-column group combine as
          // the row-major path's butterfly (k ^ 1, k ^ 2, k ^ 4, k ^ 8):
          // lanes g ^ 1 and g ^ 2 here, then the group's blocks in registers
          sq = sum_lane_groups(sq);
          const int qb = (u % CB) & 3;
          if (qb == 0 || qb == 2) gpart[qb >> 1] = sq;
          else if (qb == 1) gpart[0] = gpart[0] + sq;
          else {
            const float tot = gpart[0] + (gpart[1] + sq);
            if (g == 0) ep.rowsq[(size_t)(col / 128) * ep.ldrow + row] = tot;
          }
        }
      }
    } else {
      // SCORE: every reference chunk loaded before the loop's stores.  ref
      // null = 0 (NAP run: sum of squared outputs); colw: per-column weights
      uint4v rvs[EPI == GEMM_EPI_SCORE ? ITERS : 1];
      if constexpr (EPI == GEMM_EPI_SCORE) {
        // one branch around the whole group (a per-chunk "ref ? load : 0"
        // became a branch per load and a wait after the first one)
        if (ep.ref) {
#pragma unroll
          for (int it = 0; it < ITERS; ++it) {
            const int idx = it * NT + tid;
            const int rl = idx / CPR, ch = idx % CPR;
            rvs[it] = *(const uint4v*)((const TO*)ep.ref + (size_t)(m0 + rl) * ep.ldref + n0 + ch * OEPC);
          }
        } else {
#pragma unroll
          for (int it = 0; it < ITERS; ++it) rvs[it] = uint4v{0u, 0u, 0u, 0u};
        }
      }
      // SCORE per-column weights of this thread's columns (NAP run; 1 without)
      float wcol[EPI == GEMM_EPI_SCORE ? OEPC : 1];
      if constexpr (EPI == GEMM_EPI_SCORE && NT % CPR == 0) {
        const int col0 = n0 + (tid % CPR) * OEPC;
        if (ep.colw) {
#pragma unroll
          for (int e = 0; e < OEPC; e += 4) {
            const floatx4 w4 = *(const floatx4*)(ep.colw + col0 + e);
            wcol[e] = w4[0]; wcol[e + 1] = w4[1]; wcol[e + 2] = w4[2]; wcol[e + 3] = w4[3];
          }
        } else {
#pragma unroll
          for (int e = 0; e < OEPC; ++e) wcol[e] = 1.f;
        }
      }
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int idx = it * NT + tid;
        const int rl = idx / CPR, ch = idx % CPR;
        const uint4v v = *(const uint4v*)(smem + rl * OSTRIDE + ch * 16);
        const int row = m0 + rl;
        const int col = n0 + ch * OEPC;
        if (out) {
          *(uint4v*)(out + (size_t)row * ep.ldo + col) = v;
        }
        if constexpr (EPI == GEMM_EPI_SCORE) {
          const uint4v rv = rvs[it];
          const TO* pv = (const TO*)&v;
          const TO* pr = (const TO*)&rv;
          float sq = 0.f;
          float dd[OEPC];
          float wv[OEPC];
          if constexpr (NT % CPR == 0) {
            // this thread's columns are the same in every iteration: loaded once
#pragma unroll
            for (int e = 0; e < OEPC; ++e) wv[e] = wcol[e];
          } else {
#pragma unroll
            for (int e = 0; e < OEPC; e += 4) {
              const floatx4 w4 = ep.colw ? *(const floatx4*)(ep.colw + col + e) : floatx4{1.f, 1.f, 1.f, 1.f};
              wv[e] = w4[0]; wv[e + 1] = w4[1]; wv[e + 2] = w4[2]; wv[e + 3] = w4[3];
            }
          }
#pragma unroll
          for (int e = 0; e < OEPC; ++e) {
            dd[e] = to_f32<TO>(pv[e]) - to_f32<TO>(pr[e]);
            sq = fmaf(dd[e] * dd[e], wv[e], sq);
          }
          if (ep.diff && row < ep.M) {
            float* dp = ep.diff + (size_t)row * ep.lddiff + col;
#pragma unroll
            for (int e = 0; e < OEPC; ++e)
              if (col + e < ep.N) dp[e] = dd[e];
          }
#pragma unroll
          for (int o = 1; o < CPR128; o <<= 1) sq += __shfl_xor(sq, o);
          if (ch % CPR128 == 0) ep.rowsq[(size_t)(col / 128) * ep.ldrow + row] = sq;
        }
      }
    }
    if constexpr (EPI == GEMM_EPI_FWD && !BIG) {
      if (ep.bn_sync) {
        // ---- fused BatchNorm(train) of this layer (layers/fc_layer.py:37-48,
        // Linear -> act -> BN): whole-batch mean / variance merged from every
        // block's Welford partials (one sequential chunk order: every block of
        // the column computes the same bits), then y = a*scale + shift from the
        // fp32 activations still in registers
        const unsigned tiles_m = (unsigned)(ntl / ep.tiles_n);
        double* s_gn = (double*)(smem + OBYTES);          // [4][BN] group merges
        double* s_gm = s_gn + 4 * BN;
        double* s_gq = s_gm + 4 * BN;
        float* s_sc = (float*)(s_gq + 4 * BN);
        float* s_sh = s_sc + BN;
        static_assert(12 * BN * 8 + 2 * BN * 4 <= XBYTES - 64, "fused-BN scratch");
        if (!col_wait(ep.bn_sync + tn, gen0, ep.bn_err, tid, bn_shw)) return;
        {
          // chunk group q (= 0..3) merges partials q, q+4, ... in order (Chan et
          // al. pairwise update); the threads of a column split the groups;
          // every partial of a group is loaded before the first use
          constexpr int NGT = NT / BN;
          const int cc = tid % BN, grp = tid / BN, col = n0 + cc;
          const int nparts = (int)tiles_m * BM / MMAD_PART_ROWS;   // a multiple of 4
          for (int q = grp; q < 4; q += NGT) {
            double n = 0.0, mean = 0.0, m2 = 0.0;
            constexpr int U = 8;
            for (int u0 = 0; u0 < nparts / 4; u0 += U) {
              float mb[U], qb[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int i = q + 4 * min(u0 + u, nparts / 4 - 1);
                mb[u] = ld_sc1(ep.part + (size_t)i * 2 * ep.ldpart + col);
                qb[u] = ld_sc1(ep.part + ((size_t)i * 2 + 1) * ep.ldpart + col);
              }
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int i = q + 4 * (u0 + u);
                int cnt = ep.M - i * MMAD_PART_ROWS;
                cnt = cnt < 0 ? 0 : (cnt > MMAD_PART_ROWS ? MMAD_PART_ROWS : cnt);
                if (u0 + u >= nparts / 4 || cnt == 0) continue;
                const double nb = (double)cnt, nn = n + nb, d = (double)mb[u] - mean;
                mean += d * (nb / nn);
                m2 += (double)qb[u] + d * d * (n * nb / nn);
                n = nn;
              }
            }
            s_gn[q * BN + cc] = n;
            s_gm[q * BN + cc] = mean;
            s_gq[q * BN + cc] = m2;
          }
        }
        __syncthreads();
        if (tid < BN) {
          const int c = n0 + tid;
          double n = 0.0, mean = 0.0, m2 = 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double nb = s_gn[q * BN + tid];
            if (nb == 0.0) continue;
            const double nn = n + nb, d = s_gm[q * BN + tid] - mean;
            mean += d * (nb / nn);
            m2 += s_gq[q * BN + tid] + d * d * (n * nb / nn);
            n = nn;
          }
          const float var = n > 0.0 ? (float)(m2 / n) : 0.f;
          const float mu = (float)mean;
          float sc = 0.f, sh = 0.f;
          if (c < ep.N) {
            const float rstd = (float)(1.0 / sqrt((double)var + (double)ep.bn_eps));
            sc = bnp_g * rstd;                 // gamma / beta of column c (prefetched)
            sh = bnp_b - mu * sc;
            if (tm == 0) {
              ep.bn_save_mean[c] = mu;
              ep.bn_save_rstd[c] = rstd;
              if (ep.bn_rmean) {
                const float unb = ep.M > 1 ? var * (float)ep.M / (float)(ep.M - 1) : var;
                ep.bn_rmean[c] = (1.f - ep.bn_mom) * bnp_rm + ep.bn_mom * mu;
                ep.bn_rvar[c] = (1.f - ep.bn_mom) * bnp_rv + ep.bn_mom * unb;
              }
            }
          } else if (tm == 0) {
            ep.bn_save_mean[c] = 0.f;
            ep.bn_save_rstd[c] = 0.f;
          }
          s_sc[tid] = sc;
          s_sh[tid] = sh;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int rl = wm * 16 * TM + i * 16 + 4 * g + r;
              const int cl = wn * 16 * TN + j * 16 + c;
              // from the stored (TO-rounded) a, as the backward's xhat sees it
              const float av = to_f32<TO>(from_f32<TO>(acc[i][j][r]));
              const float yv = m0 + rl < ep.M ? av * s_sc[cl] + s_sh[cl] : 0.f;
              *(TO*)(smem + rl * OSTRIDE + cl * (int)sizeof(TO)) = from_f32<TO>(yv);
            }
        __syncthreads();
        TO* yo = (TO*)ep.bn_y;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
          const int idx = it * NT + tid;
          const int rl = idx / CPR, ch = idx % CPR;
          const uint4v v = *(const uint4v*)(smem + rl * OSTRIDE + ch * 16);
          *(uint4v*)(yo + (size_t)(m0 + rl) * ep.ldo + n0 + ch * OEPC) = v;
        }
      }
    }
    if constexpr (EPI == GEMM_EPI_BWD_WEIGHT) {
      if (ep.sm_p) {   // with or without the weight tile's own Adam (ad_p)
        // the layer's small segment [bias | gamma | beta].  Bias: the
        // column-tile-0 blocks, one output row per thread, g = db (computed
        // above from the same partials the flat path reduces, same order).
        if (tn == 0 && tid < BM && m0 + tid < ep.sm_bNp) {
          const int n = m0 + tid;
          float g = ep.gb_src ? (n < ep.sm_bN ? db_own : 0.f) : ep.sm_g[n];
          if (ep.gb_src) ep.sm_g[n] = g;
          float pp, mm, vv;
          if constexpr (APF_OK) {
            pp = smp_p;                        // prefetched before the main loop
            mm = smp_m;
            vv = smp_v;
          } else {
            pp = ep.sm_p[n];
            mm = ep.sm_m[n];
            vv = ep.sm_v[n];
          }
          adam_elem(pp, mm, vv, g, ep.ad_w1, ep.ad_w2, ep.ad_eps, ad_step, ad_bc2);
          ep.sm_p[n] = pp;
          ep.sm_m[n] = mm;
          ep.sm_v[n] = vv;
        }
        // gamma | beta (grads already final), 4 per thread over all tiles
        int q = tile * NT + tid;
        if (smq) {
          // the first chunk was read before the main loop
          const int i4 = ep.sm_bNp + q * 4;
          floatx4 pp = smq_p, mm = smq_m, vv = smq_v;
          adam4(pp, mm, vv, smq_g, ep.ad_w1, ep.ad_w2, ep.ad_eps, ad_step, ad_bc2);
          *(floatx4*)(ep.sm_p + i4) = pp;
          *(floatx4*)(ep.sm_m + i4) = mm;
          *(floatx4*)(ep.sm_v + i4) = vv;
          q += ntl * NT;
        }
        for (; ep.sm_bNp + q * 4 < ep.sm_n; q += ntl * NT) {
          const int i4 = ep.sm_bNp + q * 4;
          const floatx4 gg = *(const floatx4*)(ep.sm_g + i4);
          floatx4 pp = *(floatx4*)(ep.sm_p + i4), mm = *(floatx4*)(ep.sm_m + i4);
          floatx4 vv = *(floatx4*)(ep.sm_v + i4);
          adam4(pp, mm, vv, gg, ep.ad_w1, ep.ad_w2, ep.ad_eps, ad_step, ad_bc2);
          *(floatx4*)(ep.sm_p + i4) = pp;
          *(floatx4*)(ep.sm_m + i4) = mm;
          *(floatx4*)(ep.sm_v + i4) = vv;
        }
      }
    }
    if constexpr (EPI == GEMM_EPI_BWD_DATA) {
      if (ep.bn_part) {
        // sum over rows of dy and dy*xhat, xhat = (a - mean)*rstd, per 64-row
        // chunk, in fp64 (torch's CPU BatchNorm backward reduces in double) and
        // in one canonical order for every tile configuration: 16-row pieces
        // summed row by row, then ((p0 + p1) + p2) + p3 per chunk.  Pieces
        // pc = grp, grp + NG, ... of this thread stay in registers; the two sums
        // go through one [PIECES][BN] fp64 LDS scratch in turn.
        const int cc = tid % BN, grp = tid / BN;
        const int col = n0 + cc;
        const double mu = bnp_mu, rs = bnp_rs;   // bn_mean / bn_rstd[col] (prefetched)
        const TO* an = (const TO*)ep.bn_a;
        double* scr = (double*)(smem + BM * OSTRIDE);    // [PIECES][BN]
        double ps1[B_PPT], ps2[B_PPT];
        // fused BN: this thread's a values kept for the dz pass (up to 32
        // registers; the 8-wave 256-row / 256-column tiles reload them instead)
        constexpr bool AREG = B_PPT <= 2;
        float areg[AREG ? B_PPT : 1][16];
        // this thread's a values: the ones prefetched under the K loop, or all
        // loaded here in one block (issued together, one round trip)
        TO araw[B_PPT][16];
        bool have_a = false;
        if constexpr (BPF_OK && B_PPT == B_PPT) {
          if (pfa) {
#pragma unroll
            for (int u = 0; u < B_PPT; ++u)
#pragma unroll
              for (int r = 0; r < 16; ++r) araw[u][r] = pf_a[u][r];
            have_a = true;
          }
        }
        if (!have_a) {
#pragma unroll
          for (int u = 0; u < B_PPT; ++u) {
            const int pc = grp + u * B_NG;
            if (pc < B_PIECES) {
#pragma unroll
              for (int r = 0; r < 16; ++r) araw[u][r] = an[(size_t)(m0 + pc * 16 + r) * ep.ldo + col];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < B_PPT; ++u) {
          const int pc = grp + u * B_NG;
          double s1 = 0.0, s2 = 0.0;
          if (pc < B_PIECES) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = pc * 16 + r;
              const double dy = to_f32<TO>(*(const TO*)(smem + rl * OSTRIDE + cc * (int)sizeof(TO)));
              const float avf = to_f32<TO>(araw[u][r]);
              if constexpr (AREG) areg[u][r] = avf;   // kept for the fused dz below
              const double av = avf;
              s1 += dy;
              s2 += dy * ((av - mu) * rs);
            }
          }
          ps1[u] = s1;
          ps2[u] = s2;
        }
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
          for (int u = 0; u < B_PPT; ++u) {
            const int pc = grp + u * B_NG;
            if (pc < B_PIECES) scr[pc * BN + cc] = which ? ps2[u] : ps1[u];
          }
          __syncthreads();
          for (int c4 = grp; c4 < BM / 64; c4 += B_NG) {
            double t = scr[(4 * c4) * BN + cc];
#pragma unroll
            for (int q = 1; q < 4; ++q) t += scr[(4 * c4 + q) * BN + cc];
            double* dst = ep.bn_part + (size_t)((m0 + c4 * 64) / 64) * 2 * ep.ldo + which * ep.ldo + col;
            if (ep.bn_sync) st_sc1(dst, t);   // handed to the other blocks of this column
            else *dst = t;
          }
          __syncthreads();
        }
        if (ep.bn_sync) {
          // ---- fused BatchNorm(train) + activation backward of the producer:
          // whole-batch sums from every block's partials, then
          // dz = act'(a) * gamma*rstd/M * (M dy - sum dy - xhat sum dy*xhat)
          // (fp64 bracket, as bn_bwd_apply_k) in place in the staged tile
          const unsigned tiles_m = (unsigned)(ntl / ep.tiles_n);
          double* s_g1 = scr;                               // [4][BN] group sums (scr is free here)
          double* s_g2 = (double*)(smem + OBYTES);          // [4][BN]
          double* s_t1 = s_g2 + 4 * BN;
          double* s_t2 = s_t1 + BN;
          static_assert(B_PIECES >= 4, "group sums need 4 x BN doubles of the piece scratch");
          static_assert(6 * BN * 8 <= XBYTES - 64, "fused-BN scratch");
          col_arrive(ep.bn_sync + tn, tiles_m, tid, bn_shw);
          if (!col_wait(ep.bn_sync + tn, gen0, ep.bn_err, tid, bn_shw)) return;
          {
            // chunk group q (= 0..3) sums partials q, q+4, ... in order; the
            // threads of a column split the groups, each group's loads in flight
            // together; then ((g0 + g1) + g2) + g3
            const int nch = (int)tiles_m * BM / 64;
            for (int q = grp; q < 4; q += B_NG) {
              double t1 = 0.0, t2 = 0.0;
              constexpr int U = 8;
              const int per = (nch - q + 3) / 4;          // chunks q, q+4, ... < nch
              for (int u0 = 0; u0 < per; u0 += U) {
                double p1[U], p2[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                  const int i = q + 4 * min(u0 + u, per - 1);
                  p1[u] = ld_sc1(ep.bn_part + (size_t)i * 2 * ep.ldo + col);
                  p2[u] = ld_sc1(ep.bn_part + ((size_t)i * 2 + 1) * ep.ldo + col);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                  if (u0 + u < per) { t1 += p1[u]; t2 += p2[u]; }
              }
              s_g1[q * BN + cc] = t1;
              s_g2[q * BN + cc] = t2;
            }
          }
          __syncthreads();
          if (tid < BN) {
            const int c = n0 + tid;
            double t1 = ((s_g1[tid] + s_g1[BN + tid]) + s_g1[2 * BN + tid]) + s_g1[3 * BN + tid];
            double t2 = ((s_g2[tid] + s_g2[BN + tid]) + s_g2[2 * BN + tid]) + s_g2[3 * BN + tid];
            if (c >= ep.N) { t1 = 0.0; t2 = 0.0; }
            if (tm == 0) {
              ep.bn_dbeta[c] = (float)t1;
              ep.bn_dgamma[c] = (float)t2;
            }
            s_t1[tid] = t1;
            s_t2[tid] = t2;
          }
          __syncthreads();
          const double t1 = s_t1[cc], t2 = s_t2[cc];
          const double cf = col < ep.N ? (double)bnp_g * rs / (double)ep.M : 0.0;
          const double Md = (double)ep.M;
          // (the piece sums go straight to the fp64 piece scratch: its group-sum
          // use above is finished)
#pragma unroll AREG ? B_PPT : 1
          for (int u = 0; u < B_PPT; ++u) {
            const int pc = grp + u * B_NG;
            double sz = 0.0;
            if (pc < B_PIECES) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int rl = pc * 16 + r;
                TO* slot = (TO*)(smem + rl * OSTRIDE + cc * (int)sizeof(TO));
                const double dy = to_f32<TO>(*slot);
                float av;
                if constexpr (AREG) av = areg[u][r];
                else av = to_f32<TO>(an[(size_t)(m0 + rl) * ep.ldo + col]);
                const double xh = ((double)av - mu) * rs;
                const double da = cf * (Md * dy - t1 - xh * t2);
                float d = (float)(da * (double)act_grad_from_out(av, ep.bn_act, ep.slope));
                d = m0 + rl < ep.M ? d : 0.f;
                const TO dt = from_f32<TO>(d);
                *slot = dt;
                sz += (double)to_f32<TO>(dt);
              }
              scr[pc * BN + cc] = sz;
            }
          }
          __syncthreads();
          for (int c4 = grp; c4 < BM / 64; c4 += B_NG) {
            double t = scr[(4 * c4) * BN + cc];
#pragma unroll
            for (int q = 1; q < 4; ++q) t += scr[(4 * c4 + q) * BN + cc];
            ep.bn_dbpart[(size_t)((m0 + c4 * 64) / 64) * ep.ldo + col] = (float)t;
          }
          // coalesced store of the dz tile
          TO* dzo = (TO*)ep.bn_dz;
#pragma unroll
          for (int it = 0; it < ITERS; ++it) {
            const int idx = it * NT + tid;
            const int rl = idx / CPR, ch = idx % CPR;
            const uint4v v = *(const uint4v*)(smem + rl * OSTRIDE + ch * 16);
            *(uint4v*)(dzo + (size_t)(m0 + rl) * ep.ldo + n0 + ch * OEPC) = v;
          }
        }
      }
    }
  }
};

template <typename T, typename TO, bool AK, bool BK_, int CFG, int EPI>
__global__ __launch_bounds__(Cfg<CFG>::NT, 1) void mmad_gemm_kernel(const T* __restrict__ A, int lda,
                                                           const T* __restrict__ B, int ldb, int K,
                                                           GemmEpi ep) {
  TileTraits<T, TO, AK, BK_, CFG, EPI>::template gemm_body<false>(A, lda, B, ldb, K, ep, blockIdx.x, gridDim.x, threadIdx.x);
}

// Persistent form (knob 12) of the forward-type bf16 GEMMs at large row
// counts (C5 scoring: 65,536 rows, 8 rounds of tiles): one block per resident
// slot walks the logical tiles v = blockIdx.x, + gridDim.x, ... (gridDim a
// multiple of 8, so v & 7 -- the XCD label of the tile order -- stays the
// block's own).  Per tile the body is gemm_body's, so every output bit is the
// non-persistent kernel's; what changes is that the next tile's prologue
// (LDS-DMA of its first stages) is issued right after this tile's epilogue
// stores instead of after a block retirement and a new dispatch.  Never with
// a fused BN (its column barrier needs every tile of a column resident) or a
// split (the combine's last arriver waits for its sibling slices).
template <typename T, typename TO, bool AK, bool BK_, int CFG, int EPI>
__global__ __launch_bounds__(Cfg<CFG>::NT, 1) void mmad_gemm_kernel_p(const T* __restrict__ A, int lda,
                                                             const T* __restrict__ B, int ldb, int K,
                                                             GemmEpi ep) {
  const int nt = ep.persist_tiles;
  for (int v = blockIdx.x; v < nt; v += gridDim.x) {
    // the thread index passes through an opaque move every tile, so nothing
    // derived from it is hoisted out of the tile loop (hoisted, those values
    // stay live across the whole body and the 256-row tiles spill)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    if constexpr (CFG == CFG_XST) {
      const int nx = v + (int)gridDim.x;
      TileTraits<T, TO, AK, BK_, CFG, EPI>::template gemm_body<true>(A, lda, B, ldb, K, ep, v, nt, tid, v != (int)blockIdx.x,
                                                nx < nt ? nx : -1);
    } else {
      TileTraits<T, TO, AK, BK_, CFG, EPI>::template gemm_body<true>(A, lda, B, ldb, K, ep, v, nt, tid);
    }
    __syncthreads();
  }
}

// Grouped dW (+ Adam) launch on the 64x64 tile (mmad_gemm_dispatch_group): the
// block picks its problem from blockIdx.x against the members' first_block
// (ascending; uniform over the block, so the entry is read with scalar loads
// straight from the kernel-argument table) and runs gemm_body as block
// v = blockIdx.x - first_block of that problem's own ntiles-block grid.
// first_block is a multiple of 8, so v & 7 is blockIdx.x & 7.
template <typename T>
__global__ __launch_bounds__(Cfg<3>::NT, 1) void mmad_gemm_group_kernel(const GemmGroupTable g) {
  const int b = blockIdx.x;
  int i = 0;
#pragma unroll
  for (int j = 1; j < MMAD_GEMM_GROUP_MAX; ++j)
    if (j < g.n && b >= g.e[j].first_block) i = j;
  const GemmGroupEntry& e = g.e[i];
  const int v = b - e.first_block;
  if (v >= e.ntiles) return;   // padding block
  TileTraits<T, float, false, false, 3, GEMM_EPI_BWD_WEIGHT>::template gemm_body<false>((const T*)e.A, e.lda, (const T*)e.B, e.ldb, e.K,
                                                            e.ep, v, e.ntiles, threadIdx.x);
}
