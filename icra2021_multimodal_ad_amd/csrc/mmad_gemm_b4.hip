// The 4-wave 256x256 translation unit: tile 8's two kernels only, compiled
// without the VGPR-form MFMA flag (csrc/Makefile, B4FLAGS) so the 256
// accumulator registers live in AGPRs.
#include "mmad_gemm_body.h"

const void* mmad_gemm_b4_kernel(int epi) {
  if (epi == GEMM_EPI_FWD) return (const void*)mmad_gemm_kernel<bf16, bf16, true, true, CFG_B4, GEMM_EPI_FWD>;
  if (epi == GEMM_EPI_SCORE) return (const void*)mmad_gemm_kernel<bf16, bf16, true, true, CFG_B4, GEMM_EPI_SCORE>;
  return nullptr;
}
