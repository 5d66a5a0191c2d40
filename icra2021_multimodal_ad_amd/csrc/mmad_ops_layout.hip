// Packed layouts: fp32 windows into the GEMMs' padded [Mp][Kp] matrices (and
// split-bf16 plane pairs) and back, the padding fill, flat fp32 <-> bf16 copies.
#include "mmad_ops_dev.h"

namespace {
// PU output chunks per thread (chunk u of the block at blockIdx*256*PU +
// u*256 + tid): every chunk's loads are issued before the first conversion,
// PU x V/4 16-B loads in flight per thread
template <typename T, int PU>
__device__ __forceinline__ void pack_chunks(int M, int K, int Mp, int Kp, const float* __restrict__ x, int ldx,
                                            int vec, T* __restrict__ out, int block) {
  constexpr int V = Vec<T>::N;
  const int cpr = Kp / V;
  const int64_t total = (int64_t)Mp * cpr;
  const int64_t base = (int64_t)block * blockDim.x * PU + threadIdx.x;
  floatx4 f[PU][V / 4];
  bool full[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    const int64_t idx = base + (int64_t)u * blockDim.x;
    const int row = (int)(idx / cpr), c0 = (int)(idx % cpr) * V;
    full[u] = vec && idx < total && row < M && c0 + V <= K;
    if (full[u]) {
      // 16-B aligned rows (checked by the launcher): V/4 dwordx4 loads
      const float* src = x + (size_t)row * ldx + c0;
#pragma unroll
      for (int q = 0; q < V / 4; ++q) f[u][q] = *(const floatx4*)(src + 4 * q);
    }
  }
#pragma unroll
  for (int u = 0; u < PU; ++u) {
    const int64_t idx = base + (int64_t)u * blockDim.x;
    if (idx >= total) continue;
    const int row = (int)(idx / cpr), c0 = (int)(idx % cpr) * V;
    uint4v r;
    T* p = (T*)&r;
    if (full[u]) {
#pragma unroll
      for (int k = 0; k < V; ++k) p[k] = from_f32<T>(f[u][k / 4][k % 4]);
    } else {
      const float* src = x + (size_t)row * ldx + c0;
#pragma unroll
      for (int k = 0; k < V; ++k) p[k] = from_f32<T>((row < M && c0 + k < K) ? src[k] : 0.f);
    }
    *(uint4v*)(out + (size_t)row * Kp + c0) = r;
  }
}
template <typename T, int PU>
__global__ void pack_input_k(int M, int K, int Mp, int Kp, const float* __restrict__ x, int ldx,
                             int vec, T* __restrict__ out, const MmadDyn* __restrict__ dyn) {
  if (dyn) x = dyn->x;
  pack_chunks<T, PU>(M, K, Mp, Kp, x, ldx, vec, out, blockIdx.x);
}

// mmad_pack_input_group: member i packs its columns of the shared rows with
// the blocks [first[i], first[i + 1]), each by its own element type
struct PackGroup {
  int n, M, Mp, ldx;
  int first[MMAD_MAX_BANK + 1];
  int vec[MMAD_MAX_BANK];
  MmadPackMember m[MMAD_MAX_BANK];
};
template <int PU>
__global__ void pack_input_group_k(const PackGroup g) {
  const int b = blockIdx.x;
  if (b >= g.first[g.n]) return;
  int i = 0;
  while (b >= g.first[i + 1]) ++i;
  const MmadPackMember& m = g.m[i];
  if (m.dtype == MMAD_BF16)
    pack_chunks<bf16, PU>(g.M, m.K, g.Mp, m.Kp, m.x, g.ldx, g.vec[i], (bf16*)m.out, b - g.first[i]);
  else
    pack_chunks<float, PU>(g.M, m.K, g.Mp, m.Kp, m.x, g.ldx, g.vec[i], (float*)m.out, b - g.first[i]);
}

// MMAD_BF16X3 producers: fp32 -> the (hi, lo) bf16 planes
__device__ __forceinline__ void split_elem(float x, bf16& hi, bf16& lo) {
  hi = (bf16)x;
  lo = (bf16)(x - (float)hi);
}

// 4 values per thread; vec: src 16-byte and hi / lo 8-byte aligned
__global__ __launch_bounds__(256) void split_planes_k(int64_t n, const float* __restrict__ x,
                                                      bf16* __restrict__ hi, bf16* __restrict__ lo,
                                                      int vec) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (vec && i4 + 4 <= n) {
    const floatx4 v = *(const floatx4*)(x + i4);
    bf16x4 h, l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bf16 a, b;
      split_elem(v[k], a, b);
      h[k] = a;
      l[k] = b;
    }
    *(bf16x4*)(hi + i4) = h;
    *(bf16x4*)(lo + i4) = l;
  } else {
    for (int64_t i = i4; i < n && i < i4 + 4; ++i) split_elem(x[i], hi[i], lo[i]);
  }
}

// f32 [M][ldx] -> planes [2][Mp][Kp], 8 values (one 16-byte chunk per plane) per thread
__global__ __launch_bounds__(256) void pack_planes_k(int M, int K, int Mp, int Kp,
                                                     const float* __restrict__ x, int ldx, int vec,
                                                     bf16* __restrict__ out,
                                                     const MmadDyn* __restrict__ dyn) {
  if (dyn) x = dyn->x;
  const int cpr = Kp / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Mp * cpr) return;
  const int row = (int)(idx / cpr), c0 = (int)(idx % cpr) * 8;
  float f[8];
  if (vec && row < M && c0 + 8 <= K) {
    const float* src = x + (size_t)row * ldx + c0;
    const floatx4 a = *(const floatx4*)src, b = *(const floatx4*)(src + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[k] = a[k]; f[4 + k] = b[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = (row < M && c0 + k < K) ? x[(size_t)row * ldx + c0 + k] : 0.f;
  }
  bf16x8 h, l;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    bf16 a, b;
    split_elem(f[k], a, b);
    h[k] = a;
    l[k] = b;
  }
  const size_t o = (size_t)row * Kp + c0;
  *(bf16x8*)(out + o) = h;
  *(bf16x8*)(out + (size_t)Mp * Kp + o) = l;
}

__global__ void unpack_planes_k(int M, int N, int Np, const bf16* __restrict__ hi,
                                const bf16* __restrict__ lo, float* __restrict__ out, int ldo) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)M * N) return;
  const int row = (int)(idx / N), col = (int)(idx % N);
  const size_t o = (size_t)row * Np + col;
  out[(size_t)row * ldo + col] = (float)hi[o] + (float)lo[o];
}

template <typename T>
__global__ void unpack_k(int M, int N, int Np, const T* __restrict__ y, float* __restrict__ out,
                         int ldo) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)M * N) return;
  const int row = (int)(idx / N), col = (int)(idx % N);
  out[(size_t)row * ldo + col] = to_f32<T>(y[(size_t)row * Np + col]);
}

__global__ void to_bf16_k(int64_t n, const float* __restrict__ x, bf16* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (bf16)x[i];
}
__global__ void from_bf16_k(int64_t n, const bf16* __restrict__ x, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (float)x[i];
}
}  // namespace

// one block per row of one plane: columns >= K of a valid row, the whole row from M on
template <typename T>
__global__ __launch_bounds__(256) void zero_pad_k(int M, int K, int Mp, int Kp, T* __restrict__ x) {
  const int row = blockIdx.x;
  T* p = x + ((size_t)blockIdx.y * Mp + row) * Kp;
  for (int c = (row < M ? K : 0) + threadIdx.x; c < Kp; c += 256) p[c] = (T)0.f;
}

int mmad_pack_input_dyn(int dtype, int M, int K, int Mp, int Kp, const float* x, int ld_x,
                        void* out, const MmadDyn* dyn, void* stream) {
  MMAD_CHECK_ARG(M <= Mp && K <= Kp && Kp % 8 == 0 && ld_x >= K, "pack_input: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  // with dyn the source is read at run time: x is the current call's value
  // (same alignment class is required of every later replay, see mmad_ae)
  const int vec = ((uintptr_t)x % 16 == 0 && ld_x % 4 == 0) ? 1 : 0;
  if (dtype == MMAD_BF16X3) {
    MMAD_CHECK_ARG(Mp % MMAD_PAD == 0 && ((uintptr_t)out % 16) == 0, "pack_input: bad plane buffer");
    const int64_t n = (int64_t)Mp * (Kp / 8);
    pack_planes_k<<<nblk(n, 256), 256, 0, s>>>(M, K, Mp, Kp, x, ld_x, vec, (bf16*)out, dyn);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  }
  return mmad_by_elem(dtype, "pack_input", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    const int64_t n = (int64_t)Mp * (Kp / Vec<T>::N);
    pack_input_k<T, 4><<<nblk(n, 256 * 4), 256, 0, s>>>(M, K, Mp, Kp, x, ld_x, vec, (T*)out, dyn);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_pack_input(int dtype, int M, int K, int Mp, int Kp, const float* x, int ld_x, void* out,
                    void* stream) {
  return mmad_pack_input_dyn(dtype, M, K, Mp, Kp, x, ld_x, out, nullptr, stream);
}

int mmad_pack_input_group(int n, int M, int rows, int ld_x, const MmadPackMember* m, void* stream) {
  MMAD_CHECK_ARG(n >= 1 && n <= MMAD_MAX_BANK && m, "pack_input_group: n=%d outside 1..%d", n, MMAD_MAX_BANK);
  MMAD_CHECK_ARG(M <= rows, "pack_input_group: bad sizes");
  PackGroup g{};
  g.n = n; g.M = M; g.Mp = rows; g.ldx = ld_x;
  for (int i = 0; i < n; ++i) {
    MMAD_CHECK_ARG(m[i].dtype == MMAD_F32 || m[i].dtype == MMAD_BF16, "pack_input_group: bad dtype %d",
                   m[i].dtype);
    MMAD_CHECK_ARG(m[i].K <= m[i].Kp && m[i].Kp % 8 == 0 && ld_x >= m[i].K && m[i].x && m[i].out,
                   "pack_input_group: bad sizes");
    g.m[i] = m[i];
    g.vec[i] = ((uintptr_t)m[i].x % 16 == 0 && ld_x % 4 == 0) ? 1 : 0;
    const int V = m[i].dtype == MMAD_BF16 ? Vec<bf16>::N : Vec<float>::N;
    g.first[i + 1] = g.first[i] + (int)nblk((int64_t)rows * (m[i].Kp / V), 256 * 4);
  }
  pack_input_group_k<4><<<g.first[n], 256, 0, (hipStream_t)stream>>>(g);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_split_planes(int64_t n, const float* src, void* hi, void* lo, void* stream) {
  MMAD_CHECK_ARG(n >= 0 && (n == 0 || (src && hi && lo)), "split_planes: bad arguments");
  if (n == 0) return MMAD_OK;
  const int vec = ((uintptr_t)src % 16 == 0 && (uintptr_t)hi % 8 == 0 && (uintptr_t)lo % 8 == 0) ? 1 : 0;
  split_planes_k<<<nblk((n + 3) / 4, 256), 256, 0, (hipStream_t)stream>>>(n, src, (bf16*)hi, (bf16*)lo,
                                                                         vec);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_unpack_output(int dtype, int M, int N, int Np, const void* y, float* out, int ld_out,
                       void* stream) {
  MMAD_CHECK_ARG(N <= Np && ld_out >= N, "unpack_output: bad sizes");
  const int64_t n = (int64_t)M * N;
  if (n == 0) return MMAD_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMAD_BF16X3) {
    const bf16* hi = (const bf16*)y;
    unpack_planes_k<<<nblk(n, 256), 256, 0, s>>>(M, N, Np, hi, hi + (size_t)mmad_roundup(M, MMAD_PAD) * Np,
                                                 out, ld_out);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  }
  return mmad_by_elem(dtype, "unpack_output", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    unpack_k<T><<<nblk(n, 256), 256, 0, s>>>(M, N, Np, (const T*)y, out, ld_out);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int mmad_zero_pad(int esize, int planes, int M, int K, int Mp, int Kp, void* x, void* stream) {
  MMAD_CHECK_ARG(x && (esize == 2 || esize == 4) && planes >= 1 && M >= 0 && K >= 0 && M <= Mp && K <= Kp,
                 "zero_pad: bad arguments");
  if (M == Mp && K == Kp) return MMAD_OK;
  const dim3 grid(Mp, planes);
  if (esize == 2)
    zero_pad_k<bf16><<<grid, 256, 0, (hipStream_t)stream>>>(M, K, Mp, Kp, (bf16*)x);
  else
    zero_pad_k<float><<<grid, 256, 0, (hipStream_t)stream>>>(M, K, Mp, Kp, (float*)x);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_to_bf16(int64_t n, const float* x, void* y, void* stream) {
  if (n == 0) return MMAD_OK;
  to_bf16_k<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, x, (bf16*)y);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_from_bf16(int64_t n, const void* x, float* y, void* stream) {
  if (n == 0) return MMAD_OK;
  from_bf16_k<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, (const bf16*)x, y);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}
