// Shared by the layer-operator units (mmad_ops_*.hip): the column-slab
// geometry of their kernels and the launchers' one element-type dispatch.
#pragma once
#include "mmad_common.h"
#include "mmad_ops.h"

// one 64-column x 128-row slab per 256-thread block (grid = Np/64 x Mp/128)
#define SLAB_COLS 64
#define SLAB_ROWS 128

namespace {
template <typename T> struct Vec { static constexpr int N = 16 / sizeof(T); };  // per 16-byte access
}  // namespace

static inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }

// f(MmadElem<float>{}) for MMAD_F32, f(MmadElem<bf16>{}) for MMAD_BF16 (f: a
// generic lambda returning the launcher's status).  Any other dtype is refused
// here and f is not called, so nothing is launched: MMAD_BF16X3 as unsupported
// (an operator with a plane form branches on it before it comes here).
template <typename T> struct MmadElem { using type = T; };
template <typename F> static inline int mmad_by_elem(int dtype, const char* who, F&& f) {
  switch (dtype) {
    case MMAD_F32: return f(MmadElem<float>{});
    case MMAD_BF16: return f(MmadElem<bf16>{});
    case MMAD_BF16X3:
      mmad_set_error("%s: MMAD_BF16X3 covers the eval / score path only", who);
      return MMAD_EUNSUPPORTED;
  }
  mmad_set_error("%s: bad dtype %d", who, dtype);
  return MMAD_EINVAL;
}
