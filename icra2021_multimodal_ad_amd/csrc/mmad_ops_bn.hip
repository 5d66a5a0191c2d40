// BatchNorm1d forward around the MFMA GEMMs: the eval affine, the train-mode
// apply, the finalize and the fold into the consumer's weights.  HBM-bound.
#include "mmad_ops_dev.h"

namespace {
// ---------------------------------------------------------------------------
// BN eval affine: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale
__global__ void bn_eval_affine_k(int N, int Np, const float* gamma, const float* beta,
                                 const float* rm, const float* rv, float eps, float* scale,
                                 float* shift) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Np) return;
  if (j < N) {
    float s = gamma[j] * (float)(1.0 / sqrt((double)rv[j] + (double)eps));
    scale[j] = s;
    shift[j] = beta[j] - rm[j] * s;
  } else {
    scale[j] = 0.f;
    shift[j] = 0.f;
  }
}

// Merge the GEMM-epilogue Welford partials of 64 columns -> (mean, var) in LDS
// (the merge in fp64, as torch's CPU BatchNorm accumulates its statistics).
__device__ void merge_welford(int M, int nparts, const float* stats, int Np, int n0, float* s_mean,
                              float* s_var) {
  __shared__ double pm[4][SLAB_COLS], pq[4][SLAB_COLS], pn[4][SLAB_COLS];
  const int tid = threadIdx.x, c = tid & 63, grp = tid >> 6;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int i = grp; i < nparts; i += 4) {
    int cnt = M - i * MMAD_PART_ROWS;
    cnt = cnt < 0 ? 0 : (cnt > MMAD_PART_ROWS ? MMAD_PART_ROWS : cnt);
    if (cnt == 0) continue;
    const double mb = stats[(size_t)i * 2 * Np + n0 + c];
    const double qb = stats[((size_t)i * 2 + 1) * Np + n0 + c];
    const double nb = (double)cnt;
    const double nn = n + nb;
    const double d = mb - mean;
    mean += d * (nb / nn);
    m2 += qb + d * d * (n * nb / nn);
    n = nn;
  }
  pm[grp][c] = mean;
  pq[grp][c] = m2;
  pn[grp][c] = n;
  __syncthreads();
  if (tid < SLAB_COLS) {
    double n1 = 0.0, mu = 0.0, q = 0.0;
    for (int g = 0; g < 4; ++g) {
      const double nb = pn[g][tid];
      if (nb == 0.0) continue;
      const double nn = n1 + nb;
      const double d = pm[g][tid] - mu;
      mu += d * (nb / nn);
      q += pq[g][tid] + d * d * (n1 * nb / nn);
      n1 = nn;
    }
    s_mean[tid] = (float)mu;
    s_var[tid] = n1 > 0.0 ? (float)(q / n1) : 0.f;  // biased variance (normalisation)
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void bn_train_apply_k(int M, int N, int Np, const T* __restrict__ a,
                                                        const float* __restrict__ stats, int nparts,
                                                        const float* gamma, const float* beta,
                                                        float* rmean, float* rvar, float momentum,
                                                        float eps, float* save_mean,
                                                        float* save_rstd, T* __restrict__ y) {
  __shared__ float s_mean[SLAB_COLS], s_var[SLAB_COLS], s_sc[SLAB_COLS], s_sh[SLAB_COLS];
  const int n0 = blockIdx.x * SLAB_COLS, r0 = blockIdx.y * SLAB_ROWS, tid = threadIdx.x;
  merge_welford(M, nparts, stats, Np, n0, s_mean, s_var);
  if (tid < SLAB_COLS) {
    const int col = n0 + tid;
    float sc = 0.f, sh = 0.f;
    if (col < N) {
      const float rstd = (float)(1.0 / sqrt((double)s_var[tid] + (double)eps));
      sc = gamma[col] * rstd;
      sh = beta[col] - s_mean[tid] * sc;
      if (blockIdx.y == 0) {
        save_mean[col] = s_mean[tid];
        save_rstd[col] = rstd;
        const float unb = M > 1 ? s_var[tid] * (float)M / (float)(M - 1) : s_var[tid];
        rmean[col] = (1.f - momentum) * rmean[col] + momentum * s_mean[tid];
        rvar[col] = (1.f - momentum) * rvar[col] + momentum * unb;
      }
    } else if (blockIdx.y == 0) {
      save_mean[col] = 0.f;
      save_rstd[col] = 0.f;
    }
    s_sc[tid] = sc;
    s_sh[tid] = sh;
  }
  __syncthreads();
  constexpr int V = Vec<T>::N;
  constexpr int CPR = SLAB_COLS / V;
  for (int idx = tid; idx < SLAB_ROWS * CPR; idx += 256) {
    const int rl = idx / CPR, ch = idx % CPR;
    const int row = r0 + rl;
    const size_t off = (size_t)row * Np + n0 + ch * V;
    uint4v raw = *(const uint4v*)(a + off);
    T* e = (T*)&raw;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float v = to_f32<T>(e[k]) * s_sc[ch * V + k] + s_sh[ch * V + k];
      e[k] = from_f32<T>(row < M ? v : 0.f);
    }
    *(uint4v*)(y + off) = raw;
  }
}

// Train-mode BN finalize only: batch mean/rstd, per-column affine for the
// consumers' normalise-on-load, running-stat update.  One thread per column:
// every chunk partial is loaded up front (one memory round trip), then merged
// sequentially in chunk order (Chan et al. pairwise Welford update).
__global__ __launch_bounds__(64) void bn_finalize_k(int M, int N, int Np, const float* __restrict__ stats,
                                                    int nparts, const float* gamma, const float* beta,
                                                    float* rmean, float* rvar, float momentum,
                                                    float eps, float* save_mean, float* save_rstd,
                                                    float* scale, float* shift) {
  constexpr int U = 16;
  const int col = blockIdx.x * 64 + threadIdx.x;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int i0 = 0; i0 < nparts; i0 += U) {
    float mb[U], qb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u < nparts ? i0 + u : nparts - 1;
      mb[u] = stats[(size_t)i * 2 * Np + col];
      qb[u] = stats[((size_t)i * 2 + 1) * Np + col];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u;
      int cnt = M - i * MMAD_PART_ROWS;
      cnt = cnt < 0 ? 0 : (cnt > MMAD_PART_ROWS ? MMAD_PART_ROWS : cnt);
      if (i >= nparts || cnt == 0) continue;
      const double nb = (double)cnt, nn = n + nb, d = (double)mb[u] - mean;
      mean += d * (nb / nn);
      m2 += (double)qb[u] + d * d * (n * nb / nn);
      n = nn;
    }
  }
  const float var = n > 0.0 ? (float)(m2 / n) : 0.f;
  if (col < N) {
    const float rstd = (float)(1.0 / sqrt((double)var + (double)eps));
    const float sc = gamma[col] * rstd;
    save_mean[col] = mean;
    save_rstd[col] = rstd;
    scale[col] = sc;
    shift[col] = beta[col] - mean * sc;
    const float unb = M > 1 ? var * (float)M / (float)(M - 1) : var;
    rmean[col] = (1.f - momentum) * rmean[col] + momentum * mean;
    rvar[col] = (1.f - momentum) * rvar[col] + momentum * unb;
  } else {
    save_mean[col] = 0.f;
    save_rstd[col] = 0.f;
    scale[col] = 0.f;
    shift[col] = 0.f;
  }
}

// Finalize + fold.  Block (kb, nb): the 64 producer columns k0..k0+63 (its
// statistics merge is recomputed per n-block: 16 KB of L2 reads) and the
// 64 * FOLD_RPT consumer rows n0.. of W.  Merge order: 4 chunk groups
// (g, g+4, ...) each sequential, then ((g0 + g1) + g2) + g3.
template <typename TW, int FOLD_RPT>
__global__ __launch_bounds__(256) void bn_fold_k(int M, int N, int Np, const float* __restrict__ stats,
                                                 int nparts, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* rmean,
                                                 float* rvar, float momentum, float eps,
                                                 float* save_mean, float* save_rstd, float* scale,
                                                 float* shift, const float* __restrict__ W,
                                                 TW* __restrict__ wout, float* __restrict__ cpart,
                                                 int cp_stride) {
  // all of a group's partials in flight at once (128 partial rows = 4096
  // windows in one round trip; the merge order below is unchanged)
  constexpr int U = 32;
  __shared__ double pm[4][64], pq[4][64], pn[4][64];
  __shared__ float s_sc[64], s_sh[64];
  const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64 * FOLD_RPT, tid = threadIdx.x;
  // W tile loads first (independent of the statistics): rows r + 64 i, 16 columns
  const int r = tid >> 2, cq = (tid & 3) * 16;
  floatx4 wv[FOLD_RPT][4];
#pragma unroll
  for (int i = 0; i < FOLD_RPT; ++i)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      wv[i][u] = *(const floatx4*)(W + (size_t)(n0 + r + 64 * i) * Np + k0 + cq + 4 * u);
  {
    // shifted sums about chunk 0's mean K (no division in the chain: the
    // pairwise Welford update it replaced held a dependent fp64 division per
    // chunk, ~4.6 us of a 4096-row fold, tools/fold_probe.py):
    //   S1 = sum n_i (mean_i - K),  S2 = sum [M2_i + n_i (mean_i - K)^2],
    //   mean = K + S1 / n,  M2 = S2 - S1^2 / n
    // (K is within ~std/sqrt(32) of the batch mean, so S1^2 / n stays a few
    // per cent of S2: no cancellation to speak of in fp64)
    const int c = tid & 63, grp = tid >> 6;
    const double K = stats[k0 + c];
    double n = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i0 = grp; i0 < nparts; i0 += 4 * U) {
      float mb[U], qb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = min(i0 + 4 * u, nparts - 1);
        mb[u] = stats[(size_t)i * 2 * Np + k0 + c];
        qb[u] = stats[((size_t)i * 2 + 1) * Np + k0 + c];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + 4 * u;
        int cnt = M - i * MMAD_PART_ROWS;
        cnt = cnt < 0 ? 0 : (cnt > MMAD_PART_ROWS ? MMAD_PART_ROWS : cnt);
        if (i >= nparts || cnt == 0) continue;
        const double nb = (double)cnt, d = (double)mb[u] - K;
        n += nb;
        s1 = fma(nb, d, s1);
        s2 += fma(nb * d, d, (double)qb[u]);
      }
    }
    pm[grp][c] = s1;
    pq[grp][c] = s2;
    pn[grp][c] = n;
  }
  __syncthreads();
  if (tid < 64) {
    const double n1 = ((pn[0][tid] + pn[1][tid]) + pn[2][tid]) + pn[3][tid];
    const double t1 = ((pm[0][tid] + pm[1][tid]) + pm[2][tid]) + pm[3][tid];
    const double t2 = ((pq[0][tid] + pq[1][tid]) + pq[2][tid]) + pq[3][tid];
    const double K = stats[k0 + tid];
    const double mud = n1 > 0.0 ? K + t1 / n1 : 0.0;
    const double q = n1 > 0.0 ? fmax(t2 - t1 * (t1 / n1), 0.0) : 0.0;
    const float mu = (float)mud;
    const float var = n1 > 0.0 ? (float)(q / n1) : 0.f;
    const int col = k0 + tid;
    float sc = 0.f, sh = 0.f;
    if (col < N) {
      const float rstd = (float)(1.0 / sqrt((double)var + (double)eps));
      sc = gamma[col] * rstd;
      sh = beta[col] - mu * sc;
      if (blockIdx.y == 0) {
        save_mean[col] = mu;
        save_rstd[col] = rstd;
        const float unb = M > 1 ? var * (float)M / (float)(M - 1) : var;
        rmean[col] = (1.f - momentum) * rmean[col] + momentum * mu;
        rvar[col] = (1.f - momentum) * rvar[col] + momentum * unb;
      }
    } else if (blockIdx.y == 0) {
      save_mean[col] = 0.f;
      save_rstd[col] = 0.f;
    }
    if (blockIdx.y == 0) {
      scale[col] = sc;
      shift[col] = sh;
    }
    s_sc[tid] = sc;
    s_sh[tid] = sh;
  }
  __syncthreads();
  // W' = W * scale (row r, 16 columns), c = sum shift * W (sequential, then
  // the 4 quarter-row lanes combined ((q0 + q1) + (q2 + q3)))
#pragma unroll
  for (int i = 0; i < FOLD_RPT; ++i) {
    const int row = n0 + r + 64 * i;
    float cs = 0.f;
    TW o[16];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kl = cq + 4 * u + e;
        o[4 * u + e] = from_f32<TW>(wv[i][u][e] * s_sc[kl]);
        cs += s_sh[kl] * wv[i][u][e];
      }
    TW* dst = wout + (size_t)row * Np + k0 + cq;
#pragma unroll
    for (int v = 0; v < 16 * (int)sizeof(TW) / 16; ++v)
      *((uint4v*)dst + v) = *((const uint4v*)o + v);
    cs += __shfl_xor(cs, 1);
    cs += __shfl_xor(cs, 2);
    if ((tid & 3) == 0) cpart[(size_t)blockIdx.x * cp_stride + row] = cs;
  }
}
}  // namespace

int mmad_bn_eval_affine(int N, int Np, const float* gamma, const float* beta, const float* rm,
                        const float* rv, float eps, float* scale, float* shift, void* stream) {
  MMAD_CHECK_ARG(N >= 0 && Np >= N, "bn_eval_affine: bad sizes");
  if (Np == 0) return MMAD_OK;
  bn_eval_affine_k<<<nblk(Np, 256), 256, 0, (hipStream_t)stream>>>(N, Np, gamma, beta, rm, rv, eps,
                                                                    scale, shift);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_bn_train_apply(int dtype, int M, int N, int Mp, int Np, const void* a, const float* stats,
                        const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps, float* save_mean,
                        float* save_rstd, void* y, void* stream) {
  return mmad_by_elem(dtype, "bn_train_apply", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && M >= 1 && M <= Mp && N <= Np,
                   "bn_train_apply: bad sizes M=%d Mp=%d N=%d Np=%d", M, Mp, N, Np);
    dim3 grd(Np / SLAB_COLS, Mp / SLAB_ROWS);
    bn_train_apply_k<T><<<grd, 256, 0, (hipStream_t)stream>>>(
        M, N, Np, (const T*)a, stats, Mp / MMAD_PART_ROWS, gamma, beta, running_mean, running_var,
        momentum, eps, save_mean, save_rstd, (T*)y);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_bn_finalize(int M, int N, int Mp, int Np, const float* stats, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, float* save_mean, float* save_rstd, float* scale, float* shift,
                     void* stream) {
  MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && M >= 1 && M <= Mp && N <= Np,
                 "bn_finalize: bad sizes");
  bn_finalize_k<<<Np / 64, 64, 0, (hipStream_t)stream>>>(
      M, N, Np, stats, Mp / MMAD_PART_ROWS, gamma, beta, running_mean, running_var, momentum, eps,
      save_mean, save_rstd, scale, shift);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_bn_finalize_fold(int dtype, int M, int N, int Mp, int Np, const float* stats,
                          const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* save_mean,
                          float* save_rstd, float* scale, float* shift, const float* W, int Nc_p,
                          void* wout, float* cpart, void* stream) {
  MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && Nc_p % 64 == 0 && M >= 1 && M <= Mp && N <= Np,
                 "bn_finalize_fold: bad sizes");
  MMAD_CHECK_ARG(Nc_p % 128 == 0, "bn_finalize_fold: consumer rows not a multiple of 128");
  // consumer rows per block: 64 * RPT (the Welford merge is recomputed per
  // block, so fewer, taller blocks read fewer partials)
  constexpr int RPT = 2;   // 64-row consumer groups per block (4 measured no faster, r02bj_*)
  return mmad_by_elem(dtype, "bn_finalize_fold", [&](auto e) -> int {
    using TW = typename decltype(e)::type;
    dim3 grd(Np / 64, Nc_p / (64 * RPT));
    bn_fold_k<TW, RPT><<<grd, 256, 0, (hipStream_t)stream>>>(
        M, N, Np, stats, Mp / MMAD_PART_ROWS, gamma, beta, running_mean, running_var, momentum, eps,
        save_mean, save_rstd, scale, shift, W, (TW*)wout, cpart, Nc_p);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}
