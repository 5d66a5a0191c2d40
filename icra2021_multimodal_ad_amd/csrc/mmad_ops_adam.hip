// Adam: the flat and the two-segment update, and the constants as torch forms them.
#include "mmad_ops_dev.h"

#include <charconv>
#include <cmath>
#include <system_error>

namespace {
// ---------------------------------------------------------------------------
// Adam (torch.optim.Adam, single-tensor formula) over a flat buffer
__global__ __launch_bounds__(256) void adam_k(int64_t n, float* __restrict__ p,
                                              const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, float w1, float w2, float eps,
                                              float step_size, float bc2_sqrt, bf16* shadow,
                                              int64_t n_shadow, const MmadDyn* dyn) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (dyn) {   // graph-captured step: this step's bias-correction terms
    step_size = dyn->ad_step;
    bc2_sqrt = dyn->ad_bc2;
  }
  if (i4 + 4 <= n) {
    floatx4 pp = *(floatx4*)(p + i4), gg = *(const floatx4*)(g + i4);
    floatx4 mm = *(floatx4*)(m + i4), vv = *(floatx4*)(v + i4);
    adam4(pp, mm, vv, gg, w1, w2, eps, step_size, bc2_sqrt);
    *(floatx4*)(p + i4) = pp;
    *(floatx4*)(m + i4) = mm;
    *(floatx4*)(v + i4) = vv;
    if (shadow && i4 + 4 <= n_shadow) {
      bf16x4 s;
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = (bf16)pp[k];
      *(bf16x4*)(shadow + i4) = s;
    } else if (shadow) {   // a shadow shorter than the buffer, ending inside this quad
      for (int k = 0; k < 4 && i4 + k < n_shadow; ++k) shadow[i4 + k] = (bf16)pp[k];
    }
  } else {
    for (int64_t i = i4; i < n; ++i) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam_elem(pp, mm, vv, g[i], w1, w2, eps, step_size, bc2_sqrt);
      p[i] = pp;
      m[i] = mm;
      v[i] = vv;
      if (shadow && i < n_shadow) shadow[i] = (bf16)pp;
    }
  }
}

// Adam over two flat segments (a layer's weights and its bias/gamma/beta)
__global__ __launch_bounds__(256) void adam2_k(MmadAdamSeg s0, MmadAdamSeg s1, float w1, float w2,
                                               float eps, float step_size, float bc2_sqrt) {
  int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const MmadAdamSeg* sg = &s0;
  if (i4 >= s0.n) { i4 -= s0.n; sg = &s1; }
  if (i4 >= sg->n) return;
  float* p = sg->p + i4;
  float* g = sg->g + i4;
  float* m = sg->m + i4;
  float* v = sg->v + i4;
  floatx4 gg;
  if (sg->bsrc && i4 < sg->bNp) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = (int)i4 + k;
      float t = 0.f;
      if (e < sg->bN)
        for (int i = 0; i < sg->bparts; ++i) t += sg->bsrc[(size_t)i * sg->bstride + e];
      gg[k] = t;
    }
    *(floatx4*)g = gg;
  } else {
    gg = *(const floatx4*)g;
  }
  floatx4 pp = *(floatx4*)p, mm = *(floatx4*)m, vv = *(floatx4*)v;
  adam4(pp, mm, vv, gg, w1, w2, eps, step_size, bc2_sqrt);
  *(floatx4*)p = pp;
  *(floatx4*)m = mm;
  *(floatx4*)v = vv;
  if (sg->shadow) {
    bf16x4 sh;
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k] = (bf16)pp[k];
    *(bf16x4*)((bf16*)sg->shadow + i4) = sh;
  }
}
}  // namespace

int mmad_adam_dyn(int64_t n, float* p, const float* g, float* m, float* v, float w1, float w2,
                  float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
                  const MmadDyn* dyn, void* stream) {
  MMAD_CHECK_ARG(n >= 0 && n_shadow >= 0 && n_shadow <= n, "adam: bad sizes");
  if (n == 0) return MMAD_OK;
  MMAD_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0,
                 "adam: buffers must be 16-byte aligned");
  adam_k<<<nblk((n + 3) / 4, 256), 256, 0, (hipStream_t)stream>>>(
      n, p, g, m, v, w1, w2, eps, step_size, bc2_sqrt, (bf16*)shadow, n_shadow, dyn);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_adam_w(int64_t n, float* p, const float* g, float* m, float* v, float w1, float w2,
                float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
                void* stream) {
  return mmad_adam_dyn(n, p, g, m, v, w1, w2, eps, step_size, bc2_sqrt, shadow, n_shadow, nullptr,
                       stream);
}

int mmad_adam(int64_t n, float* p, const float* g, float* m, float* v, float beta1, float beta2,
              float eps, float step_size, float bc2_sqrt, void* shadow, int64_t n_shadow,
              void* stream) {
  // public entry: the caller's betas; the update constants as torch forms them
  const MmadAdamConsts c = mmad_adam_consts(1e-3f, beta1, beta2, eps, 1);
  return mmad_adam_w(n, p, g, m, v, c.w1, c.w2, eps, step_size, bc2_sqrt, shadow, n_shadow, stream);
}

int mmad_adam2(const MmadAdamSeg& s0, const MmadAdamSeg& s1, float w1, float w2, float eps,
               float step_size, float bc2_sqrt, void* stream) {
  MMAD_CHECK_ARG(s0.n % 4 == 0 && s1.n % 4 == 0, "adam2: segment lengths must be multiples of 4");
  const int64_t n4 = (s0.n + s1.n) / 4;
  if (n4 == 0) return MMAD_OK;
  adam2_k<<<nblk(n4, 256), 256, 0, (hipStream_t)stream>>>(s0, s1, w1, w2, eps, step_size,
                                                          bc2_sqrt);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

double mmad_decimal_of(float f) {
  // the shortest decimal that rounds to f, as a double: the Python float a
  // caller's optimizer holds (0.9, 0.999, 1e-3) when it reached us as float.
  // std::to_chars / from_chars: shortest round-trip form, independent of the
  // process locale (snprintf / strtod read LC_NUMERIC's decimal point).  A
  // hyper-parameter that was not a short decimal (a scheduler's lr) comes
  // back as the shortest decimal of its float, i.e. within the float's
  // rounding of the caller's double -- the float ABI carries no more.
  char buf[64];
  const auto r = std::to_chars(buf, buf + sizeof buf, f);
  if (r.ec != std::errc()) return (double)f;
  double d = 0.0;
  const auto q = std::from_chars(buf, r.ptr, d);
  return q.ec == std::errc() && q.ptr == r.ptr ? d : (double)f;
}

MmadAdamConsts mmad_adam_consts(float lr, float beta1, float beta2, float eps, int step) {
  // torch.optim.Adam (_single_tensor_adam): 1 - beta, lr / (1 - beta1^t) and
  // sqrt(1 - beta2^t) in double from the optimizer's double hyper-parameters,
  // each cast to float where torch casts it (the scalar operand of a float op)
  const double b1 = mmad_decimal_of(beta1), b2 = mmad_decimal_of(beta2), l = mmad_decimal_of(lr);
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  MmadAdamConsts c;
  c.w1 = (float)(1.0 - b1);
  c.w2 = (float)(1.0 - b2);
  c.eps = eps;
  c.step_size = (float)(l / bc1);
  c.bc2_sqrt = (float)pow(bc2, 0.5);
  return c;
}
