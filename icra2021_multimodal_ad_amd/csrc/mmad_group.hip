// Column-group mean squares of an fp32 matrix (mmad_group_sq): the
// per-modality anomaly scores of the online and batch scoring passes.
//
//   out[g][n] = sum_{c in [b_g, b_{g+1})} d[n][c]^2 / (b_{g+1} - b_g)
//
// One wave per (row, group) pair, four rows per block, no LDS, no atomics.
//
// Summation rule -- a function of b_g and b_{g+1} alone, not of N, the row, ldd
// or the other groups: fixed lane-strided accumulation, then a fixed shuffle
// tree.  Columns are taken in ALIGNED QUADS of absolute columns 4q .. 4q + 3.
// With q0 = b_g >> 2, quad q belongs to lane (q - q0) & 63, and a lane takes
// its quads in ascending order.  Element j of a quad goes to the lane's
// accumulator j: acc[j] = fma(v, v, acc[j]); columns of a boundary quad that
// lie outside the group are not read and add nothing.  Then
// s = (acc[0] + acc[1]) + (acc[2] + acc[3]) and the xor tree 32, 16, 8, 4, 2, 1
// over the wave; lane 0 divides by the width.
//
// Loads: a quad wholly inside the group is ONE 16-byte load where the row's
// base address is 16-byte aligned (wave-uniform test), else four 4-byte loads
// of the same values into the same accumulators; the head and tail quads of an
// unaligned group are masked scalar loads.  The interior loop issues four
// quads' loads ahead of their fmas.  Nothing outside [b_g, b_{g+1}) is read.
#include "mmad_common.h"
#include "mmad_ops.h"

namespace {

constexpr int GW = 4;   // waves (rows) per block

__device__ __forceinline__ floatx4 load_quad(const float* p, bool vec) {
  if (vec) return *(const floatx4*)p;
  return floatx4{p[0], p[1], p[2], p[3]};
}

__device__ __forceinline__ void add_quad(float (&acc)[4], const floatx4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = __fmaf_rn(v[j], v[j], acc[j]);
}

// the columns of quad q inside [b0, b1), one masked scalar load each
__device__ __forceinline__ void add_partial(float (&acc)[4], const float* row, int q, int b0, int b1) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * q + j;
    if (c >= b0 && c < b1) {
      const float v = row[c];
      acc[j] = __fmaf_rn(v, v, acc[j]);
    }
  }
}

__global__ __launch_bounds__(GW * 64) void group_sq_k(const MmadGroupSq a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x % a.G;
  const int64_t n = (int64_t)(blockIdx.x / a.G) * GW + wv;
  if (n >= a.N) return;   // wave-uniform; no barrier below
  const int b0 = a.bounds[g], b1 = a.bounds[g + 1];
  const float* row = a.d + n * a.ldd;
  const bool vec = ((uintptr_t)row & 15) == 0;
  const int q0 = b0 >> 2;
  const int qa = (b0 + 3) >> 2, qb = b1 >> 2;   // quads wholly inside: [qa, qb)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (qa > qb) {   // the group lies inside one quad
    if (lane == 0) add_partial(acc, row, q0, b0, b1);
  } else {
    if (qa != q0 && lane == 0) add_partial(acc, row, q0, b0, b1);   // head
    int q = q0 + lane;
    if (q < qa) q += 64;
    for (; q + 192 < qb; q += 256) {
      floatx4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = load_quad(row + 4 * (q + 64 * u), vec);
#pragma unroll
      for (int u = 0; u < 4; ++u) add_quad(acc, v[u]);
    }
    for (; q < qb; q += 64) add_quad(acc, load_quad(row + 4 * q, vec));
    if ((b1 & 3) && lane == ((qb - q0) & 63)) add_partial(acc, row, qb, b0, b1);   // tail
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (lane != 0) return;
  const float v = s / (float)(b1 - b0);
  a.out[(int64_t)g * a.ldo + n] = v;
  // strict >: get_f1_score's prediction rule; a NaN threshold compares false
  if (a.flags)
    a.flags[(int64_t)g * a.ldf + n] = (a.thr && n < a.n_flag) ? (uint8_t)(v > a.thr[g]) : 0;
}

}  // namespace

int mmad_group_sq_launch(const MmadGroupSq& a, void* stream) {
  MMAD_CHECK_ARG(a.G >= 1 && a.G <= MMAD_MAX_GROUPS, "group_sq: G=%d outside 1..%d", a.G, MMAD_MAX_GROUPS);
  MMAD_CHECK_ARG(a.bounds[0] >= 0, "group_sq: bounds[0]=%d is negative", a.bounds[0]);
  for (int g = 0; g < a.G; ++g)
    MMAD_CHECK_ARG(a.bounds[g] < a.bounds[g + 1], "group_sq: bounds not strictly ascending "
                   "(bounds[%d]=%d, bounds[%d]=%d)", g, a.bounds[g], g + 1, a.bounds[g + 1]);
  MMAD_CHECK_ARG(a.bounds[a.G] <= a.ldd, "group_sq: bounds[G]=%d exceeds ldd=%lld", a.bounds[a.G],
                 (long long)a.ldd);
  MMAD_CHECK_ARG(a.N >= 1 && a.d && ((uintptr_t)a.d & 3) == 0, "group_sq: N=%lld, d null or not "
                 "4-byte aligned", (long long)a.N);
  MMAD_CHECK_ARG(a.out && a.ldo >= a.N, "group_sq: null out or ld_out=%lld < N", (long long)a.ldo);
  MMAD_CHECK_ARG(!a.flags || a.ldf >= a.N, "group_sq: ld_flags=%lld < N", (long long)a.ldf);
  const int64_t blocks = (a.N + GW - 1) / GW * a.G;
  MMAD_CHECK_ARG(blocks <= 0x7fffffffLL, "group_sq: N=%lld rows x G=%d exceed the grid", (long long)a.N, a.G);
  group_sq_k<<<(unsigned)blocks, GW * 64, 0, (hipStream_t)stream>>>(a);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_group_sq(int64_t N, const float* d, int64_t ldd, const int* bounds, int G,
                  const float* thresholds, float* out, int64_t ld_out, uint8_t* flags,
                  int64_t ld_flags, void* stream) {
  MMAD_CHECK_ARG(G >= 1 && G <= MMAD_MAX_GROUPS, "group_sq: G=%d outside 1..%d", G, MMAD_MAX_GROUPS);
  MMAD_CHECK_ARG(bounds, "group_sq: null bounds");
  MmadGroupSq a{};
  a.d = d; a.ldd = ldd; a.N = N; a.n_flag = N; a.G = G;
  for (int g = 0; g <= G; ++g) a.bounds[g] = bounds[g];
  a.thr = thresholds; a.out = out; a.ldo = ld_out; a.flags = flags; a.ldf = ld_flags;
  return mmad_group_sq_launch(a, stream);
}
