// The variational-information-bottleneck waist: z = mu + eps * exp(logvar / 2)
// with its KL partials, its backward, and the Philox noise source.
#include "mmad_ops_dev.h"

namespace {
// ---------------------------------------------------------------------------
// Philox4x32-10 counter-based RNG -> N(0,1) via Box-Muller
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
  const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
  c[0] = hi1 ^ c[1] ^ k0;
  c[1] = lo1;
  c[2] = hi0 ^ c[3] ^ k1;
  c[3] = lo0;
}
__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t offset, uint64_t idx) {
  uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float u1 = ((c[0] >> 8) + 1) * (1.0f / 16777217.0f);  // (0,1]
  const float u2 = (c[1] >> 8) * (1.0f / 16777216.0f);
  return sqrtf(-2.f * __logf(u1)) * __cosf(6.2831853071795864f * u2);
}

template <typename T>
__global__ __launch_bounds__(256) void vib_fwd_k(int B, int btl, int k, const T* __restrict__ enc,
                                                 int ld_enc, const float* __restrict__ eps,
                                                 float* __restrict__ eps_out, uint64_t seed,
                                                 uint64_t offset, int det, T* __restrict__ z,
                                                 int ld_z, int Mpz, float* kl_part,
                                                 const MmadDyn* __restrict__ dyn) {
  // one thread per element of the packed z buffer [Mpz][ld_z]; rows < B also
  // contribute the KL term of their (mu, logvar) pair.
  __shared__ float red[4];
  if (dyn) {
    eps = dyn->eps;
    seed = dyn->seed;
    offset = dyn->offset;
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)Mpz * ld_z;
  float kl = 0.f;
  if (idx < total) {
    const int row = (int)(idx / ld_z), c = (int)(idx % ld_z);
    float out = 0.f;
    if (c < btl && row < k * B) {
      const int kk = row / B, b = row % B;
      const float mu = to_f32<T>(enc[(size_t)b * ld_enc + c]);
      const float lv = to_f32<T>(enc[(size_t)b * ld_enc + btl + c]);
      if (det) {
        out = mu;
      } else {
        const size_t ei = ((size_t)kk * B + b) * btl + c;
        const float e = eps ? eps[ei] : philox_normal(seed, offset, ei);
        if (eps_out) eps_out[ei] = e;
        out = e * __expf(0.5f * lv) + mu;
      }
      if (kk == 0 && kl_part) kl = -0.5f * (1.f + lv - mu * mu - __expf(lv));
    }
    z[idx] = from_f32<T>(out);
  }
  if (kl_part) {
    kl = wave_sum(kl);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kl;
    __syncthreads();
    if (threadIdx.x == 0) kl_part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vib_bwd_k(int B, int btl, int k, const T* __restrict__ enc,
                                                 int ld_enc, const float* __restrict__ eps,
                                                 const T* __restrict__ dz, int ld_dz, float beta,
                                                 T* __restrict__ denc, int ld_denc, int Mpe) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Mpe * ld_denc) return;
  const int b = (int)(idx / ld_denc), c = (int)(idx % ld_denc);
  float out = 0.f;
  if (b < B && c < 2 * btl) {
    const int cc = c < btl ? c : c - btl;
    const float mu = to_f32<T>(enc[(size_t)b * ld_enc + cc]);
    const float lv = to_f32<T>(enc[(size_t)b * ld_enc + btl + cc]);
    if (c < btl) {
      float s = 0.f;
      for (int kk = 0; kk < k; ++kk) s += to_f32<T>(dz[((size_t)kk * B + b) * ld_dz + cc]);
      out = s + beta * mu;
    } else {
      const float sig = __expf(0.5f * lv);
      float s = 0.f;
      for (int kk = 0; kk < k; ++kk)
        s += to_f32<T>(dz[((size_t)kk * B + b) * ld_dz + cc]) * eps[((size_t)kk * B + b) * btl + cc];
      out = 0.5f * sig * s + 0.5f * beta * (__expf(lv) - 1.f);
    }
  }
  denc[idx] = from_f32<T>(out);
}
}  // namespace

int mmad_vib_reparam_fwd(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                         const float* eps, float* eps_out, uint64_t seed, uint64_t offset,
                         int deterministic, void* z, int ld_z, float* kl_partial, void* stream) {
  return mmad_vib_reparam_fwd_dyn(dtype, B, btl, k, enc_out, ld_enc, eps, eps_out, seed, offset,
                                  deterministic, z, ld_z, kl_partial, nullptr, stream);
}

int mmad_vib_reparam_fwd_dyn(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                             const float* eps, float* eps_out, uint64_t seed, uint64_t offset,
                             int deterministic, void* z, int ld_z, float* kl_partial,
                             const MmadDyn* dyn, void* stream) {
  MMAD_CHECK_ARG(B >= 1 && btl >= 1 && k >= 1 && ld_enc >= 2 * btl && ld_z >= btl,
                 "vib_reparam_fwd: bad sizes");
  const int Mpz = mmad_roundup(k * B, MMAD_PAD);
  const int64_t n = (int64_t)Mpz * ld_z;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MMAD_BF16X3) {
    if (!deterministic || kl_partial) {
      mmad_set_error("vib_reparam_fwd: MMAD_BF16X3 is deterministic only (z = mu, no KL partials)");
      return MMAD_EUNSUPPORTED;
    }
    // z = mu: the same copy on each plane
    const bf16* e = (const bf16*)enc_out;
    bf16* zz = (bf16*)z;
    const size_t eo = (size_t)mmad_roundup(B, MMAD_PAD) * ld_enc, zo = (size_t)Mpz * ld_z;
    for (int p = 0; p < 2; ++p)
      vib_fwd_k<bf16><<<nblk(n, 256), 256, 0, s>>>(B, btl, k, e + p * eo, ld_enc, nullptr, nullptr, 0, 0,
                                                   1, zz + p * zo, ld_z, Mpz, nullptr, nullptr);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  }
  return mmad_by_elem(dtype, "vib_reparam_fwd", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    vib_fwd_k<T><<<nblk(n, 256), 256, 0, s>>>(B, btl, k, (const T*)enc_out, ld_enc, eps, eps_out, seed,
                                              offset, deterministic, (T*)z, ld_z, Mpz, kl_partial, dyn);
    MMAD_LAUNCH_CHECK();
    return MMAD_OK;
  });
}

int64_t mmad_vib_kl_parts(int B, int k, int ld_z) {
  const int Mpz = mmad_roundup(k * B, MMAD_PAD);
  return ((int64_t)Mpz * ld_z + 255) / 256;
}

int mmad_vib_reparam_bwd(int dtype, int B, int btl, int k, const void* enc_out, int ld_enc,
                         const float* eps, const void* dz, int ld_dz, float beta_kl,
                         void* d_enc_out, int ld_denc, float* colsum, void* stream) {
  return mmad_by_elem(dtype, "vib_reparam_bwd", [&](auto e) -> int {
    using T = typename decltype(e)::type;
    MMAD_CHECK_ARG(B >= 1 && btl >= 1 && k >= 1 && ld_denc >= 2 * btl, "vib_reparam_bwd: bad sizes");
    // the column sums run on 64-column slabs with 16-byte loads
    MMAD_CHECK_ARG(!colsum || ld_denc % SLAB_COLS == 0,
                   "vib_reparam_bwd: colsum needs ld_denc to be a multiple of 64, got %d", ld_denc);
    const int Mpe = mmad_roundup(B, MMAD_PAD);
    const int64_t n = (int64_t)Mpe * ld_denc;
    vib_bwd_k<T><<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(B, btl, k, (const T*)enc_out, ld_enc, eps,
                                                                (const T*)dz, ld_dz, beta_kl,
                                                                (T*)d_enc_out, ld_denc, Mpe);
    MMAD_LAUNCH_CHECK();
    if (colsum) return mmad_matrix_colsum_partials(dtype, B, Mpe, ld_denc, d_enc_out, colsum, stream);
    return MMAD_OK;
  });
}
