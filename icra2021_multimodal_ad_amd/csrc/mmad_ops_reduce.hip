// Column and scalar reductions (bias gradients, losses) and the standalone MSE loss.
#include "mmad_ops_dev.h"

namespace {
// column sums of a packed matrix -> partials [Mp/128][Np]
template <typename T>
__global__ __launch_bounds__(256) void matrix_colsum_k(int M, int Np, const T* __restrict__ x,
                                                       float* __restrict__ part) {
  constexpr int V = Vec<T>::N;
  constexpr int CPR = SLAB_COLS / V;
  constexpr int RG = 256 / CPR;
  __shared__ float s_red[RG][SLAB_COLS];
  const int n0 = blockIdx.x * SLAB_COLS, r0 = blockIdx.y * SLAB_ROWS, tid = threadIdx.x;
  const int ch = tid % CPR, rg = tid / CPR;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  for (int rl = rg; rl < SLAB_ROWS; rl += RG) {
    const int row = r0 + rl;
    if (row >= M) break;
    uint4v r = *(const uint4v*)(x + (size_t)row * Np + n0 + ch * V);
    const T* p = (const T*)&r;
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] += to_f32<T>(p[k]);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) s_red[rg][ch * V + k] = acc[k];
  __syncthreads();
  if (tid < SLAB_COLS) {
    float t = 0.f;
    for (int g = 0; g < RG; ++g) t += s_red[g][tid];
    part[(size_t)blockIdx.y * Np + n0 + tid] = t;
  }
}

__global__ void colsum_k(int n_parts, int N, int Np, const float* __restrict__ part,
                         int stride, float scale, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Np) return;
  float t = 0.f;
  if (j < N)
    for (int i = 0; i < n_parts; ++i) t += part[(size_t)i * stride + j];
  out[j] = scale * t;
}

__global__ __launch_bounds__(1024) void sum2d_k(int rows, int cols, const float* __restrict__ x,
                                                int64_t ld, float scale, float* out, int accumulate) {
  __shared__ float red[16];
  float t = 0.f;
  const int64_t n = (int64_t)rows * cols;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const int64_t r = i / cols, c = i % cols;
    t += x[r * ld + c];
  }
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += red[i];
    out[0] = (accumulate ? out[0] : 0.f) + scale * s;
  }
}

// ---------------------------------------------------------------------------
// One launch for all end-of-backward reductions (bias grads, loss): job j,
// block x covers 256 output columns; scalar jobs run in block x == 0 only.
__global__ __launch_bounds__(256) void reduce_jobs_k(MmadReduceJobs jobs) {
  const MmadReduceJob& jb = jobs.j[blockIdx.y];
  const int tid = threadIdx.x;
  if (jb.scalar) {
    if (blockIdx.x != 0) return;
    __shared__ float red[4];
    float t = 0.f;
    for (int i = 0; i < jb.nparts; ++i)
      for (int c = tid; c < jb.N; c += 256) t += jb.src[(size_t)i * jb.stride + c];
    t *= jb.scale;
    float t2 = 0.f;
    for (int c = tid; c < jb.n2; c += 256) t2 += jb.src2[c];
    t += jb.scale2 * t2;
    t = wave_sum(t);
    if ((tid & 63) == 0) red[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) (jobs.dyn ? jobs.dyn->loss : jb.dst)[0] = red[0] + red[1] + red[2] + red[3];
    return;
  }
  const int j = blockIdx.x * 256 + tid;
  if (j >= jb.Np) return;
  float t = 0.f;
  if (j < jb.N) {
    // sequential partial order (the fused dW epilogue's and the flat Adam's),
    // with 32 partial loads in flight per round trip (the data-parallel step
    // reduces every layer's bias partials here: 128 dependent loads per column
    // at 4096 rows took 70 us on the step's critical tail)
    constexpr int U = 32;
    int i = 0;
    for (; i + U <= jb.nparts; i += U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = jb.src[(size_t)(i + u) * jb.stride + j];
#pragma unroll
      for (int u = 0; u < U; ++u) t += v[u];
    }
    for (; i < jb.nparts; ++i) t += jb.src[(size_t)i * jb.stride + j];
  }
  jb.dst[j] = jb.scale * t;
}

template <typename T>
__global__ void sse_k(int M, int N, int Np, const T* __restrict__ y, const float* __restrict__ x,
                      int ldx, float* __restrict__ part) {
  __shared__ float red[4];
  float t = 0.f;
  const int64_t n = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / N), col = (int)(i % N);
    const float d = to_f32<T>(y[(size_t)row * Np + col]) - x[(size_t)row * ldx + col];
    t += d * d;
  }
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------------------
// Standalone reconstruction loss, modules/loss.py:47-52 (Loss('mse',
// reduction)): sum (or mean) of (y_hat - y)^2 and its gradient.  (Inside the
// autoencoder the sum-MSE is fused into the last decoder GEMM's epilogue;
// this is the plugin-surface Loss called on its own.)  Deterministic: a fixed
// grid of MSE_PARTS blocks, each a fixed strided order, then one block sums
// the partials in order.
constexpr int MSE_PARTS = 256;
__global__ __launch_bounds__(256) void mse_partials_k(int64_t n, const float* __restrict__ a,
                                                      const float* __restrict__ b, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  const bool vec = (((uintptr_t)a | (uintptr_t)b) % 16) == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)MSE_PARTS * 256) {
    const floatx4 x = ((const floatx4*)a)[i], y = ((const floatx4*)b)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = x[e] - y[e];
      acc = fmaf(d, d, acc);
    }
  }
  for (int64_t i = 4 * n4 + blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)MSE_PARTS * 256) {
    const float d = a[i] - b[i];
    acc = fmaf(d, d, acc);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void mse_grad_k(int64_t n, const float* __restrict__ a,
                                                  const float* __restrict__ b, const float* __restrict__ g,
                                                  float scale, float* __restrict__ da, float* __restrict__ db) {
  const float s = scale * (g ? g[0] : 1.f);
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = s * (a[i] - b[i]);
    if (da) da[i] = d;
    if (db) db[i] = -d;
  }
}
}  // namespace

// Np: whole 64-column slabs (the rule mmad_vib_reparam_bwd documents for its colsum)
int mmad_matrix_colsum_partials(int dtype, int M, int Mp, int Np, const void* x, float* part,
                                void* stream) {
  MMAD_CHECK_ARG(Mp % 128 == 0 && Np % SLAB_COLS == 0 && M >= 0 && M <= Mp && x && part,
                 "matrix_colsum_partials: bad arguments");
  return mmad_by_elem(dtype, "matrix_colsum_partials", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    dim3 grd(Np / SLAB_COLS, Mp / SLAB_ROWS);
    matrix_colsum_k<T><<<grd, 256, 0, (hipStream_t)stream>>>(M, Np, (const T*)x, part);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_colsum(int n_parts, int N, int Np, const float* partials, int part_stride, float scale,
                float* out, void* stream) {
  MMAD_CHECK_ARG(n_parts >= 0 && N <= Np, "colsum: bad sizes");
  if (Np == 0) return MMAD_OK;
  colsum_k<<<nblk(Np, 256), 256, 0, (hipStream_t)stream>>>(n_parts, N, Np, partials, part_stride,
                                                            scale, out);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_sum2d(int rows, int cols, const float* x, int64_t ld, float scale, float* out,
               int accumulate, void* stream) {
  MMAD_CHECK_ARG(rows >= 0 && cols >= 0, "sum2d: bad sizes");
  sum2d_k<<<1, 1024, 0, (hipStream_t)stream>>>(rows, cols, x, ld, scale, out, accumulate);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_sum(int64_t n, const float* x, float scale, float* out, int accumulate, void* stream) {
  MMAD_CHECK_ARG(n >= 0 && n < (1LL << 31), "sum: bad n");
  return mmad_sum2d(1, (int)n, x, n, scale, out, accumulate, stream);
}

int mmad_reduce_jobs(const MmadReduceJobs& jobs, int n_jobs, int max_np, void* stream) {
  MMAD_CHECK_ARG(n_jobs >= 1 && n_jobs <= MMAD_MAX_REDUCE_JOBS, "reduce_jobs: bad job count");
  dim3 grd((max_np + 255) / 256, n_jobs);
  reduce_jobs_k<<<grd, 256, 0, (hipStream_t)stream>>>(jobs);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_sse_partials(int dtype, int M, int N, int Np, const void* y, const float* x, int ldx,
                      float* part, int nparts, void* stream) {
  MMAD_CHECK_ARG(M >= 0 && N >= 0 && N <= Np && nparts >= 1 && y && x && part,
                 "sse_partials: bad arguments");
  return mmad_by_elem(dtype, "sse_partials", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    sse_k<T><<<nparts, 256, 0, (hipStream_t)stream>>>(M, N, Np, (const T*)y, x, ldx, part);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_mse_loss_ws_floats(void) { return MSE_PARTS; }

int mmad_mse_loss(int64_t n, const float* y_hat, const float* y, int mean, float* loss_out, float* work,
                  void* stream) {
  MMAD_CHECK_ARG(n >= 1 && y_hat && y && loss_out && work, "mse_loss: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  mse_partials_k<<<MSE_PARTS, 256, 0, s>>>(n, y_hat, y, work);
  MMAD_LAUNCH_CHECK();
  return mmad_sum(MSE_PARTS, work, mean ? (float)(1.0 / (double)n) : 1.f, loss_out, 0, stream);
}

int mmad_mse_grad(int64_t n, const float* y_hat, const float* y, const float* g, int mean, float* d_yhat,
                  float* d_y, void* stream) {
  MMAD_CHECK_ARG(n >= 1 && y_hat && y && (d_yhat || d_y), "mse_grad: bad arguments");
  const float scale = mean ? (float)(2.0 / (double)n) : 2.f;
  const int64_t blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
  mse_grad_k<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(n, y_hat, y, g, scale, d_yhat, d_y);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}
