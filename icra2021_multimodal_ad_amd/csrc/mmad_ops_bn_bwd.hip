// BatchNorm(train) + activation backward, and the activation backward of a
// layer without BatchNorm, on 64-column x 128-row slabs.
#include "mmad_ops_dev.h"
#include "mmad_gemm.h"

#include <hip/hip_ext.h>
#include <type_traits>

namespace {
// ---------------------------------------------------------------------------
// BN(train) + activation backward.  Pass 1: per-slab partial sums of dy and
// dy*xhat.  Pass 2: finalise dgamma/dbeta, dz, and db partials.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_k(int M, int Np, const T* __restrict__ dy,
                                                       const T* __restrict__ a,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ rstd,
                                                       double* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  constexpr int CPR = SLAB_COLS / V;
  constexpr int RG = 256 / CPR;  // row groups
  __shared__ double s1[RG][SLAB_COLS], s2[RG][SLAB_COLS];
  const int n0 = blockIdx.x * SLAB_COLS, r0 = blockIdx.y * SLAB_ROWS, tid = threadIdx.x;
  const int ch = tid % CPR, rg = tid / CPR;
  double acc1[V], acc2[V], mu[V], rs[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    acc1[k] = 0.0;
    acc2[k] = 0.0;
    mu[k] = mean[n0 + ch * V + k];
    rs[k] = rstd[n0 + ch * V + k];
  }
  for (int rl = rg; rl < SLAB_ROWS; rl += RG) {
    const int row = r0 + rl;
    if (row >= M) break;
    const size_t off = (size_t)row * Np + n0 + ch * V;
    uint4v rd = *(const uint4v*)(dy + off);
    uint4v ra = *(const uint4v*)(a + off);
    const T* pd = (const T*)&rd;
    const T* pa = (const T*)&ra;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double d = to_f32<T>(pd[k]);
      acc1[k] += d;
      acc2[k] += d * (((double)to_f32<T>(pa[k]) - mu[k]) * rs[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    s1[rg][ch * V + k] = acc1[k];
    s2[rg][ch * V + k] = acc2[k];
  }
  __syncthreads();
  if (tid < SLAB_COLS) {
    double t1 = 0.0, t2 = 0.0;
    for (int g = 0; g < RG; ++g) { t1 += s1[g][tid]; t2 += s2[g][tid]; }
    part[((size_t)blockIdx.y * 2) * Np + n0 + tid] = t1;
    part[((size_t)blockIdx.y * 2 + 1) * Np + n0 + tid] = t2;
  }
}

// dz = act'(a) * gamma*rstd/M * (M*dy - sum(dy) - xhat*sum(dy*xhat)) over RB
// 64-column x 128-row slabs; sums from the bwd-data GEMM epilogue partials,
// merged once per block.  The first slab's loads (dy, a, the column
// constants, the partials) are issued before any use, so the block's first
// slab costs one memory round trip; each later slab's dy / a are loaded
// under the previous slab's arithmetic.  Per slab the same arithmetic and
// the same db-partial order as RB = 1 (bit-identical for every RB).  LK: the
// activation is LeakyReLU (the AE's), known at compile time -- with a run-time
// act the per-element switch stays inside the unrolled loop, 32 branch chains
// per row group and slab
template <typename T, int PU, int RB, bool LK>
__global__ __launch_bounds__(256) void bn_bwd_apply_k(int act_rt, float slope, int M, int N, int Np,
                                                      int nparts, const T* __restrict__ dy,
                                                      const T* __restrict__ a,
                                                      const float* __restrict__ mean,
                                                      const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma,
                                                      const double* __restrict__ part,
                                                      T* __restrict__ dz, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, float* __restrict__ dbpart) {
  constexpr int V = Vec<T>::N;
  constexpr int CPR = SLAB_COLS / V;      // threads per row
  constexpr int RG = 256 / CPR;           // row groups
  constexpr int RPT = SLAB_ROWS / RG;     // rows per thread and slab
  const int act = LK ? (int)MMAD_ACT_LEAKYRELU : act_rt;
  // PU: partial chunks per group loaded at once (16 from 2048 rows: one round
  // trip for all of a 4096-row batch's 64 chunks; same summation order)
  __shared__ double s_red[RG][SLAB_COLS];
  __shared__ double s_p1[4][SLAB_COLS], s_p2[4][SLAB_COLS];
  const int n0 = blockIdx.x * SLAB_COLS, tid = threadIdx.x;
  const int ch = tid % CPR, rg = tid / CPR;
  // (1) this thread's dy / a rows of the first slab
  uint4v rd[RPT], ra[RPT];
  auto load_slab = [&](int slab) {
    const int r0 = slab * SLAB_ROWS;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const size_t off = (size_t)(r0 + rg + i * RG) * Np + n0 + ch * V;
      rd[i] = *(const uint4v*)(dy + off);
      ra[i] = *(const uint4v*)(a + off);
    }
  };
  load_slab(blockIdx.y * RB);
  // (2) partial sums: 4 groups of 64 columns, group g sums chunks g, g+4, ...
  {
    const int c = tid & 63, grp = tid >> 6;
    double t1 = 0.0, t2 = 0.0;
    for (int i0 = grp; i0 < nparts; i0 += 4 * PU) {
      double p1[PU], p2[PU];
#pragma unroll
      for (int u = 0; u < PU; ++u) {
        const int i = i0 + 4 * u < nparts ? i0 + 4 * u : grp;
        p1[u] = part[((size_t)i * 2) * Np + n0 + c];
        p2[u] = part[((size_t)i * 2 + 1) * Np + n0 + c];
      }
#pragma unroll
      for (int u = 0; u < PU; ++u)
        if (i0 + 4 * u < nparts) { t1 += p1[u]; t2 += p2[u]; }
    }
    s_p1[grp][c] = t1;
    s_p2[grp][c] = t2;
  }
  __syncthreads();
  if (tid < SLAB_COLS) {
    double t1 = ((s_p1[0][tid] + s_p1[1][tid]) + s_p1[2][tid]) + s_p1[3][tid];
    double t2 = ((s_p2[0][tid] + s_p2[1][tid]) + s_p2[2][tid]) + s_p2[3][tid];
    const int col = n0 + tid;
    if (col >= N) { t1 = 0.0; t2 = 0.0; }
    s_p1[0][tid] = t1;
    s_p2[0][tid] = t2;
    if (blockIdx.y == 0) { dbeta[col] = (float)t1; dgamma[col] = (float)t2; }
  }
  __syncthreads();
  // (3) column constants (loaded after the partials: their registers are free by then)
  float mu[V], rs[V], gm[V];
#pragma unroll
  for (int k = 0; k < V; k += 4) {
    const int col = n0 + ch * V + k;
    *(floatx4*)&mu[k] = *(const floatx4*)(mean + col);
    *(floatx4*)&rs[k] = *(const floatx4*)(rstd + col);
    *(floatx4*)&gm[k] = *(const floatx4*)(gamma + col);
  }
  // da = gamma rstd / M (M dy - sum dy - xhat sum dy xhat): the bracket nearly
  // cancels, so on the exact-fp32 path it is evaluated in fp64 (as the
  // reference's CPU BatchNorm backward does its reductions), dz and its column
  // sums too.  The bf16 path (this kernel runs there from 2048 rows, c3 / c4)
  // rounds dz to 8 bits: its bracket in fp32 (M * dy exact, M a power of two
  // at the bench shapes; the column sums rounded once), which halves the
  // kernel's registers and doubles its waves per SIMD -- a 4096-row apply ran
  // at 2.2-2.5 TB/s with the fp64 bracket (tools/apply_probe.py)
  using CT = std::conditional_t<sizeof(T) == 2, float, double>;
  const CT invM = (CT)1 / (CT)M;
  CT cf[V], dbv[V], dgv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int col = n0 + ch * V + k;
    cf[k] = col < N ? (CT)gm[k] * (CT)rs[k] * invM : (CT)0;
    dbv[k] = (CT)s_p1[0][ch * V + k];
    dgv[k] = (CT)s_p2[0][ch * V + k];
  }
  for (int sb = 0; sb < RB; ++sb) {
    const int slab = blockIdx.y * RB + sb;
    const int r0 = slab * SLAB_ROWS;
    CT accb[V];
#pragma unroll
    for (int k = 0; k < V; ++k) accb[k] = (CT)0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int row = r0 + rg + i * RG;
      const T* pd = (const T*)&rd[i];
      const T* pa = (const T*)&ra[i];
      T* po = (T*)&rd[i];      // dz over dy in place: element k is read before it is written
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float av = to_f32<T>(pa[k]);
        const CT xh = ((CT)av - (CT)mu[k]) * (CT)rs[k];
        const CT da = cf[k] * ((CT)M * (CT)to_f32<T>(pd[k]) - dbv[k] - xh * dgv[k]);
        float d = (float)(da * (CT)act_grad_from_out(av, act, slope));
        d = row < M ? d : 0.f;
        const T dt = from_f32<T>(d);
        po[k] = dt;
        accb[k] += (CT)to_f32<T>(dt);
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i)
      *(uint4v*)(dz + (size_t)(r0 + rg + i * RG) * Np + n0 + ch * V) = rd[i];
    // the next slab's rows load under this slab's reduction
    if (sb + 1 < RB) load_slab(slab + 1);
#pragma unroll
    for (int k = 0; k < V; ++k) s_red[rg][ch * V + k] = accb[k];
    __syncthreads();
    if (tid < SLAB_COLS) {
      double t = 0.0;
      for (int g = 0; g < RG; ++g) t += s_red[g][tid];
      dbpart[(size_t)slab * Np + n0 + tid] = (float)t;
    }
    if (sb + 1 < RB) __syncthreads();   // s_red reused by the next slab
  }
}

// Activation backward without BatchNorm (an FCLayer with bn=False):
// dz = dy * act'(a) from the activation OUTPUT a, plus the per-slab column
// sums of dz (the bias gradient) -> db partials [Mp/128][Np]
template <typename T>
__global__ __launch_bounds__(256) void act_bwd_k(int act, float slope, int M, int Np,
                                                 const T* __restrict__ dy, const T* __restrict__ a,
                                                 T* __restrict__ dz, float* __restrict__ dbpart) {
  constexpr int V = Vec<T>::N;
  constexpr int CPR = SLAB_COLS / V;
  constexpr int RG = 256 / CPR;
  __shared__ double s_red[RG][SLAB_COLS];
  const int n0 = blockIdx.x * SLAB_COLS, r0 = blockIdx.y * SLAB_ROWS, tid = threadIdx.x;
  const int ch = tid % CPR, rg = tid / CPR;
  double acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.0;
  for (int rl = rg; rl < SLAB_ROWS; rl += RG) {
    const int row = r0 + rl;
    const size_t off = (size_t)row * Np + n0 + ch * V;
    const uint4v rd = *(const uint4v*)(dy + off);
    const uint4v ra = *(const uint4v*)(a + off);
    const T* pd = (const T*)&rd;
    const T* pa = (const T*)&ra;
    uint4v ro;
    T* po = (T*)&ro;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float d = to_f32<T>(pd[k]) * act_grad_from_out(to_f32<T>(pa[k]), act, slope);
      d = row < M ? d : 0.f;
      po[k] = from_f32<T>(d);
      acc[k] += (double)to_f32<T>(po[k]);
    }
    *(uint4v*)(dz + off) = ro;
  }
#pragma unroll
  for (int k = 0; k < V; ++k) s_red[rg][ch * V + k] = acc[k];
  __syncthreads();
  if (tid < SLAB_COLS) {
    double t = 0.0;
    for (int g = 0; g < RG; ++g) t += s_red[g][tid];
    dbpart[(size_t)blockIdx.y * Np + n0 + tid] = (float)t;
  }
}

// the apply kernel for run-time (rb, lk): every form has the same signature
template <typename T, int PU, int RB> auto bn_bwd_apply_for(bool lk) {
  return lk ? bn_bwd_apply_k<T, PU, RB, true> : bn_bwd_apply_k<T, PU, RB, false>;
}
template <typename T, int PU> auto bn_bwd_apply_for(int rb, bool lk) {
  return rb == 4   ? bn_bwd_apply_for<T, PU, 4>(lk)
         : rb == 2 ? bn_bwd_apply_for<T, PU, 2>(lk)
                   : bn_bwd_apply_for<T, PU, 1>(lk);
}
}  // namespace

int mmad_bn_act_bwd_apply(int dtype, int act, float slope, int M, int N, int Mp, int Np,
                          const void* dy, const void* a, const float* save_mean,
                          const float* save_rstd, const float* gamma, const double* part,
                          int nparts, void* dz, float* dgamma, float* dbeta, float* db_partials,
                          void* stream) {
  return mmad_bn_act_bwd_apply_ev(dtype, act, slope, M, N, Mp, Np, dy, a, save_mean, save_rstd, gamma,
                                  part, nparts, dz, dgamma, dbeta, db_partials, stream, nullptr);
}

int mmad_bn_act_bwd_apply_ev(int dtype, int act, float slope, int M, int N, int Mp, int Np,
                             const void* dy, const void* a, const float* save_mean,
                             const float* save_rstd, const float* gamma, const double* part,
                             int nparts, void* dz, float* dgamma, float* dbeta, float* db_partials,
                             void* stream, void* done) {
  MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && M >= 0 && M <= Mp && N <= Np && nparts >= 0 &&
                     dy && a && save_mean && save_rstd && gamma && part && dz && dgamma && dbeta &&
                     db_partials,
                 "bn_act_bwd_apply: bad arguments");
  // 128-row slabs per block (knob 13: 1, 2 or 4; any other value = 1; halved
  // until it divides the row slabs): the column partials are merged once per
  // block instead of once per 128-row slab
  int rb = mmad_knob(KNOB_BN_APPLY_RB);
  if (rb != 1 && rb != 2 && rb != 4) rb = 1;
  while (rb > 1 && (Mp / SLAB_ROWS) % rb) rb >>= 1;
  const bool wide = nparts > 4 * 8;   // 16 partial chunks per round trip (8 no faster, r02bj_*)
  const bool lk = act == MMAD_ACT_LEAKYRELU;
  return mmad_by_elem(dtype, "bn_act_bwd_apply", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    const auto kern = wide ? bn_bwd_apply_for<T, 16>(rb, lk) : bn_bwd_apply_for<T, 8>(rb, lk);
    const dim3 grd(Np / SLAB_COLS, Mp / (SLAB_ROWS * rb));
    hipStream_t s = (hipStream_t)stream;
    // `done` (nullable) completes with the kernel: the launch's own stop event
    auto launch = [&](auto... args) {
      if (done)
        hipExtLaunchKernelGGL(kern, grd, dim3(256), 0u, s, nullptr, (hipEvent_t)done, 0u, args...);
      else
        kern<<<grd, 256, 0, s>>>(args...);
    };
    launch(act, slope, M, N, Np, nparts, (const T*)dy, (const T*)a, save_mean, save_rstd, gamma, part,
           (T*)dz, dgamma, dbeta, db_partials);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

size_t mmad_bn_act_bwd_ws(int Mp, int Np) { return (size_t)(Mp / SLAB_ROWS) * 2 * Np * sizeof(double); }

int mmad_bn_act_bwd(int dtype, int act, float slope, int M, int N, int Mp, int Np, const void* dy,
                    const void* a, const float* save_mean, const float* save_rstd,
                    const float* gamma, void* dz, float* dgamma, float* dbeta, float* db_partials,
                    void* ws, void* stream) {
  return mmad_by_elem(dtype, "bn_act_bwd", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && M >= 1 && M <= Mp && N <= Np,
                   "bn_act_bwd: bad sizes");
    dim3 grd(Np / SLAB_COLS, Mp / SLAB_ROWS);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    bn_bwd_reduce_k<T><<<grd, 256, 0, s>>>(M, Np, (const T*)dy, (const T*)a, save_mean, save_rstd,
                                           part);
    bn_bwd_apply_k<T, 8, 1, false><<<grd, 256, 0, s>>>(act, slope, M, N, Np, Mp / SLAB_ROWS,
                                                       (const T*)dy, (const T*)a, save_mean,
                                                       save_rstd, gamma, part, (T*)dz, dgamma, dbeta,
                                                       db_partials);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_act_bwd(int dtype, int act, float slope, int M, int Mp, int Np, const void* dy,
                 const void* a, void* dz, float* db_partials, void* stream) {
  return mmad_by_elem(dtype, "act_bwd", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    MMAD_CHECK_ARG(Mp % 128 == 0 && Np % 128 == 0 && M >= 0 && M <= Mp && dy && a && dz && db_partials,
                   "act_bwd: bad arguments");
    dim3 grd(Np / SLAB_COLS, Mp / SLAB_ROWS);
    act_bwd_k<T><<<grd, 256, 0, (hipStream_t)stream>>>(act, slope, M, Np, (const T*)dy, (const T*)a,
                                                       (T*)dz, db_partials);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}
