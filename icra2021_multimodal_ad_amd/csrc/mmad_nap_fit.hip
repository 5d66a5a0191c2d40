// NAP fit on the device (utils/metric.py:183-238 fits it on the train diffs):
//   Rotater.fit     utils/normalize.py:52-70   mu_r = mean(x), V = right
//                                              singular vectors of x - mu_r
//   Standardizer.fit utils/normalize.py:25-34 on the rotated train diffs
//                                              rot = (x - mu_r) V (fp32 matmul,
//                                              Rotater.run :72-103):
//                                              mu_s = mean(rot), var = ddof-1
//                                              variance of rot (np.cov, fp64)
//
// Schedule (all on the caller's stream, caller-owned workspace):
//   1. column means of x, fp64 partials per row chunk, reduced in chunk order
//      -> mu_r (fp32, as the reference's x.float().mean(0))
//   2. Gram G = xc^T xc in fp64 (xc = fp32(x - mu_r) formed on the fly while
//      staging tiles in LDS), upper-triangular 64x64 tile set, mirrored
//   3. eigendecomposition of G (rocSOLVER dsyevd, the one library call; the
//      right singular vectors of xc are G's eigenvectors), descending order
//      -> V [W][R], R = min(N, W)
//   4. rot = xc V in fp32 (LDS-tiled FMA), column sum / sum of squares in
//      fp64 per row chunk, reduced in chunk order -> mu_s, var
// Every reduction has a fixed order: the fit is deterministic.
//
// rocSOLVER / rocBLAS are resolved at run time from the copies already in the
// process (torch's librocsolver.so.0 / librocblas.so.5), falling back to
// dlopen by soname: one instance per process, no link-time dependency.
#include <dlfcn.h>
#include <mutex>

#include "mmad_common.h"

namespace {

constexpr int MEAN_COLS = 256;     // columns per block of the mean pass
constexpr int MEAN_ROWS = 2048;    // rows per partial
constexpr int GT = 64;             // Gram / rotation output tile
constexpr int GK = 32;             // rows (Gram) / features (rotation) per LDS stage
constexpr int ROT_ROWS = 1024;     // rows per rotation-statistics partial

__global__ __launch_bounds__(256) void nap_colsum_k(int64_t N, int W, const float* __restrict__ x,
                                                    int64_t ldx, double* __restrict__ part) {
  const int c = blockIdx.x * MEAN_COLS + threadIdx.x;
  if (c >= W) return;
  const int64_t r0 = (int64_t)blockIdx.y * MEAN_ROWS;
  const int64_t r1 = r0 + MEAN_ROWS < N ? r0 + MEAN_ROWS : N;
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += (double)x[r * ldx + c];
  part[(int64_t)blockIdx.y * W + c] = s;
}

__global__ __launch_bounds__(256) void nap_mean_k(int64_t N, int W, int nparts,
                                                  const double* __restrict__ part,
                                                  float* __restrict__ mu) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * W + c];
  mu[c] = (float)(s / (double)N);
}

// G[i][j] = sum_n xc[n][i] xc[n][j], tiles (ti <= tj) of 64x64, 256 threads,
// 4x4 outputs per thread (rows ty + 16a, cols tx + 16b: conflict-free LDS reads)
__global__ __launch_bounds__(256) void nap_gram_k(int64_t N, int W, const float* __restrict__ x,
                                                  int64_t ldx, const float* __restrict__ mu,
                                                  int T, double* __restrict__ G) {
  // linear upper-triangular tile index -> (ti, tj), ti <= tj
  int t = blockIdx.x, ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  const int tj = ti + t;
  const int i0 = ti * GT, j0 = tj * GT;
  __shared__ double As[GK][GT];
  __shared__ double Bs[GK][GT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4] = {};
  const int lc = tid & 63, lr = tid >> 6;   // loader: column lc, rows lr + 4q
  const int ci = i0 + lc, cj = j0 + lc;
  const float mi = ci < W ? mu[ci] : 0.f, mj = cj < W ? mu[cj] : 0.f;
  for (int64_t n0 = 0; n0 < N; n0 += GK) {
#pragma unroll
    for (int q = 0; q < GK / 4; ++q) {
      const int r = lr + 4 * q;
      const int64_t n = n0 + r;
      float a = 0.f, b = 0.f;
      if (n < N) {
        if (ci < W) a = x[n * ldx + ci] - mi;   // fp32 centring, as the reference's x - mu
        if (cj < W) b = x[n * ldx + cj] - mj;
      }
      As[r][lc] = (double)a;
      Bs[r][lc] = (double)b;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < GK; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = As[k][ty + 16 * u]; bv[u] = Bs[k][tx + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[u][w] = fma(av[u], bv[w], acc[u][w]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * w;
      if (i < W && j < W) {
        G[(int64_t)i * W + j] = acc[u][w];
        G[(int64_t)j * W + i] = acc[u][w];
      }
    }
}

// dsyevd leaves eigenvectors in the columns of the (column-major) matrix in
// ascending eigenvalue order: V[i][r] = A[i + (W-1-r) W], r < R
__global__ __launch_bounds__(256) void nap_evec_k(int W, int R, const double* __restrict__ A,
                                                  float* __restrict__ v) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)W * R) return;
  const int i = (int)(e / R), r = (int)(e % R);
  v[e] = (float)A[(int64_t)(W - 1 - r) * W + i];
}

// rot = xc V (fp32, Rotater.run's matmul): per block a 64-column slice of rot
// over a ROT_ROWS row chunk, as 64x64 sub-tiles; per column the fp64 sums of
// rot and rot^2 over the chunk -> part[chunk][2][R]
__global__ __launch_bounds__(256) void nap_rotstats_k(int64_t N, int W, int R,
                                                      const float* __restrict__ x, int64_t ldx,
                                                      const float* __restrict__ mu,
                                                      const float* __restrict__ v,
                                                      double* __restrict__ part) {
  __shared__ float Xs[GT][GK + 1];
  __shared__ float Vs[GK][GT];
  __shared__ double red[2][16][GT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int c0 = blockIdx.x * GT;
  const int64_t rbeg = (int64_t)blockIdx.y * ROT_ROWS;
  const int64_t rend = rbeg + ROT_ROWS < N ? rbeg + ROT_ROWS : N;
  double s1[4] = {}, s2[4] = {};
  for (int64_t m0 = rbeg; m0 < rend; m0 += GT) {
    float acc[4][4] = {};
    for (int k0 = 0; k0 < W; k0 += GK) {
      // X tile [64 rows][32 features]: thread -> feature tid & 31, rows (tid >> 5) + 8q
#pragma unroll
      for (int q = 0; q < GT / 8; ++q) {
        const int r = (tid >> 5) + 8 * q, k = tid & 31;
        const int64_t n = m0 + r;
        const int f = k0 + k;
        Xs[r][k] = (n < rend && f < W) ? x[n * ldx + f] - mu[f] : 0.f;
      }
      // V tile [32 features][64 columns]
#pragma unroll
      for (int q = 0; q < GK / 4; ++q) {
        const int k = (tid >> 6) + 4 * q, c = tid & 63;
        const int f = k0 + k;
        Vs[k][c] = (f < W && c0 + c < R) ? v[(int64_t)f * R + c0 + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < GK; ++k) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { av[u] = Xs[ty + 16 * u][k]; bv[u] = Vs[k][tx + 16 * u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[u][w] = fmaf(av[u], bv[w], acc[u][w]);
      }
      __syncthreads();
    }
    // rows past the chunk end hold 0 (zero X rows): they add nothing
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const double r = (double)acc[u][w];
        s1[w] += r;
        s2[w] += r * r;
      }
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    red[0][ty][tx + 16 * w] = s1[w];
    red[1][ty][tx + 16 * w] = s2[w];
  }
  __syncthreads();
  if (tid < 2 * GT) {
    const int which = tid / GT, c = tid % GT;
    double s = 0.0;
    for (int y = 0; y < 16; ++y) s += red[which][y][c];
    if (c0 + c < R) part[((int64_t)blockIdx.y * 2 + which) * R + c0 + c] = s;
  }
}

__global__ __launch_bounds__(256) void nap_stats_k(int64_t N, int R, int nparts,
                                                   const double* __restrict__ part,
                                                   float* __restrict__ mu_s,
                                                   float* __restrict__ var) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= R) return;
  double s1 = 0.0, s2 = 0.0;
  for (int p = 0; p < nparts; ++p) {
    s1 += part[((int64_t)p * 2 + 0) * R + c];
    s2 += part[((int64_t)p * 2 + 1) * R + c];
  }
  const double mean = s1 / (double)N;
  mu_s[c] = (float)mean;
  const double ss = s2 - s1 * mean;                  // sum (rot - mean)^2
  var[c] = (float)((ss > 0.0 ? ss : 0.0) / (double)(N - 1));
}

// ---- rocSOLVER (run-time resolved) ---------------------------------------
typedef void* rb_handle;
struct SolverApi {
  int (*create_handle)(rb_handle*);
  int (*destroy_handle)(rb_handle);
  int (*set_stream)(rb_handle, hipStream_t);
  int (*dsyevd)(rb_handle, int evect, int uplo, int n, double* A, int lda, double* D, double* E,
                int* info);
  bool ok;
};
constexpr int RB_EVECT_ORIGINAL = 211;   // rocblas_evect_original
constexpr int RB_FILL_UPPER = 121;       // rocblas_fill_upper

void* find_lib(const char* sym, const char* soname) {
  if (dlsym(RTLD_DEFAULT, sym)) return RTLD_DEFAULT;
  return dlopen(soname, RTLD_NOW | RTLD_GLOBAL);
}

const SolverApi& solver() {
  static SolverApi api{};
  static std::once_flag once;
  std::call_once(once, [] {
    void* hb = find_lib("rocblas_create_handle", "librocblas.so.5");
    void* hs = find_lib("rocsolver_dsyevd", "librocsolver.so.0");
    if (!hb || !hs) return;
    api.create_handle = (decltype(api.create_handle))dlsym(hb, "rocblas_create_handle");
    api.destroy_handle = (decltype(api.destroy_handle))dlsym(hb, "rocblas_destroy_handle");
    api.set_stream = (decltype(api.set_stream))dlsym(hb, "rocblas_set_stream");
    api.dsyevd = (decltype(api.dsyevd))dlsym(hs, "rocsolver_dsyevd");
    api.ok = api.create_handle && api.destroy_handle && api.set_stream && api.dsyevd;
  });
  return api;
}

// eigendecomposition of the symmetric A [W][W] in place (eigenvectors in its
// columns, ascending eigenvalues in D); synchronises s for the convergence flag
int eig_sym(const SolverApi& api, int W, double* A, double* D, double* E, int* info_dev,
            hipStream_t s) {
  rb_handle h = nullptr;
  if (api.create_handle(&h) != 0) {
    mmad_set_error("nap_fit: rocblas_create_handle failed");
    return MMAD_EHIP;
  }
  int st = api.set_stream(h, s);
  if (st == 0) st = api.dsyevd(h, RB_EVECT_ORIGINAL, RB_FILL_UPPER, W, A, W, D, E, info_dev);
  int info = 0;
  const hipError_t ce = hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, s);
  const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(s) : ce;
  api.destroy_handle(h);
  if (st != 0) {
    mmad_set_error("nap_fit: rocsolver_dsyevd returned status %d", st);
    return MMAD_EHIP;
  }
  MMAD_HIP_CHECK(se);
  if (info != 0) {
    mmad_set_error("nap_fit: eigensolver did not converge (info=%d)", info);
    return MMAD_EHIP;
  }
  return MMAD_OK;
}

struct FitWS {
  double* G;       // [W][W]
  double* D;       // [W] eigenvalues
  double* E;       // [W] dsyevd scratch
  double* mpart;   // [ceil(N / MEAN_ROWS)][W]
  double* rpart;   // [ceil(N / ROT_ROWS)][2][R]
  int* info;
  size_t total;
};

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

FitWS carve_fit(int64_t N, int W, char* base) {
  const int64_t R = N < W ? N : W;
  FitWS w{};
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al256(bytes); return p; };
  w.G = (double*)take((size_t)W * W * 8);
  w.D = (double*)take((size_t)W * 8);
  w.E = (double*)take((size_t)W * 8);
  w.mpart = (double*)take((size_t)((N + MEAN_ROWS - 1) / MEAN_ROWS) * W * 8);
  w.rpart = (double*)take((size_t)((N + ROT_ROWS - 1) / ROT_ROWS) * 2 * R * 8);
  w.info = (int*)take(sizeof(int));
  w.total = o;
  return w;
}

}  // namespace

size_t mmad_nap_fit_ws_bytes(int64_t N, int W) {
  if (N < 2 || W < 1) return 0;
  return carve_fit(N, W, nullptr).total;
}

int mmad_nap_fit(int64_t N, int W, const float* x, int64_t ldx, float* mu_r, float* v, float* mu_s,
                 float* var, void* ws, size_t ws_bytes, void* stream) {
  MMAD_CHECK_ARG(N >= 2 && W >= 1 && W <= 46340 && ldx >= W && x && mu_r && v && mu_s && var && ws,
                 "nap_fit: bad arguments (N=%lld W=%d ldx=%lld)", (long long)N, W, (long long)ldx);
  MMAD_CHECK_ARG(N / MEAN_ROWS < 65535 && N / ROT_ROWS < 65535, "nap_fit: N=%lld too large",
                 (long long)N);
  const FitWS w = carve_fit(N, W, (char*)ws);
  MMAD_CHECK_ARG(ws_bytes >= w.total, "nap_fit: workspace %zu < %zu bytes", ws_bytes, w.total);
  MMAD_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "nap_fit: workspace must be 256-byte aligned");
  const SolverApi& api = solver();
  if (!api.ok) {
    mmad_set_error("nap_fit: rocSOLVER / rocBLAS not found in the process (librocsolver.so.0)");
    return MMAD_EHIP;
  }
  hipStream_t s = (hipStream_t)stream;
  const int R = (int)(N < W ? N : W);
  const int mparts = (int)((N + MEAN_ROWS - 1) / MEAN_ROWS);
  nap_colsum_k<<<dim3((W + MEAN_COLS - 1) / MEAN_COLS, mparts), 256, 0, s>>>(N, W, x, ldx, w.mpart);
  MMAD_LAUNCH_CHECK();
  nap_mean_k<<<(W + 255) / 256, 256, 0, s>>>(N, W, mparts, w.mpart, mu_r);
  MMAD_LAUNCH_CHECK();
  const int T = (W + GT - 1) / GT;
  nap_gram_k<<<T * (T + 1) / 2, 256, 0, s>>>(N, W, x, ldx, mu_r, T, w.G);
  MMAD_LAUNCH_CHECK();
  {
    const int rc = eig_sym(api, W, w.G, w.D, w.E, w.info, s);
    if (rc != MMAD_OK) return rc;
  }
  const int64_t nv = (int64_t)W * R;
  nap_evec_k<<<(unsigned)((nv + 255) / 256), 256, 0, s>>>(W, R, w.G, v);
  MMAD_LAUNCH_CHECK();
  const int rparts = (int)((N + ROT_ROWS - 1) / ROT_ROWS);
  nap_rotstats_k<<<dim3((R + GT - 1) / GT, rparts), 256, 0, s>>>(N, W, R, x, ldx, mu_r, v, w.rpart);
  MMAD_LAUNCH_CHECK();
  nap_stats_k<<<(R + 255) / 256, 256, 0, s>>>(N, R, rparts, w.rpart, mu_s, var);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

// ---------------------------------------------------------------------------
// Streaming fit: the same fit accumulated batch by batch into a caller-owned
// fit state, so the train diffs never exist as one matrix.  Three passes over
// the batches (the caller regenerates them each time):
//   1. column sums: nap_colsum_k partials per 2048-row chunk, added to the
//      running fp64 sums in chunk order -> mu_r as nap_mean_k forms it
//   2. centre the batch in place (valid region only), then the Gram of the
//      batch on v_mfma_f64_16x16x4_f64 into the running upper-triangular G;
//      after the last batch G is mirrored into A and eig_sym / nap_evec_k run
//      as in mmad_nap_fit
//   3. rot = (d - mu_r) V per 2048-row chunk through the exact-fp32 GEMM
//      (mmad_fc_fwd, weight V^T, zero bias, no activation); its Welford
//      partials per 32 rows become fp64 sum / sum of squares, added in chunk
//      order -> mu_s, var by nap_stats_k
// Every kernel is an ordinary grid; no atomics, every reduction order is fixed
// by (W, the batch sizes), so a repeated fit is bit-identical.
namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int SUM_PARTS = 64;    // column-sum partials per launch (64 x 2048 rows)
constexpr int FT = 128;          // Gram output tile of a block (4 waves, 64x64 each)
constexpr int FK = 32;           // batch rows per LDS stage
constexpr int FLD = FT + 16;     // LDS row stride: the 4 rows a wave reads fall in 4 bank groups
constexpr int ROT_CHUNK = 2048;  // rows per rotation GEMM

// S[c] += part[0][c] + part[1][c] + ... one partial at a time (nap_mean_k's order)
__global__ __launch_bounds__(256) void fs_addsum_k(int W, int nparts, const double* __restrict__ part,
                                                   double* __restrict__ S) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  double s = S[c];
  for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * W + c];
  S[c] = s;
}

// d[r][c] -= mu[c] on the valid region only: padding rows / columns stay as
// they are (zero), or they would enter the Gram as -mu
__global__ __launch_bounds__(256) void fs_centre_k(int B, int W, float* __restrict__ d, int64_t ld,
                                                   const float* __restrict__ mu) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  const float m = mu[c];
  for (int r = blockIdx.y; r < B; r += gridDim.y) d[(int64_t)r * ld + c] -= m;
}

// G[i][j] += sum_{n < B} d[n][i] d[n][j] for the upper-triangular 128x128 tile
// set, one block per tile (it alone reads and writes that tile of G).  The
// contraction runs over rows, so both MFMA operands are MN-major: lane l of a
// wave feeds A = d[n + (l >> 4)][i + (l & 15)] and B likewise, straight out of
// the row-major LDS stage.  fp32 -> fp64 on the way in: every product is exact.
// Rows >= B and columns >= W are staged as 0, never read.
__global__ __launch_bounds__(256) void fs_gram_k(int B, int W, const float* __restrict__ d,
                                                 int64_t ld, int T, double* __restrict__ G) {
  int t = blockIdx.x, ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const int i0 = ti * FT, j0 = tj * FT;
  __shared__ float As[FK][FLD];
  __shared__ float Bs[FK][FLD];
  const float(*Bp)[FLD] = diag ? As : Bs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
  const int lr = lane >> 4, lc = lane & 15;
  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
  doublex4 acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wi + 16 * u + lr + 4 * r, j = j0 + wj + 16 * v + lc;
        acc[u][v][r] = (i < W && j < W) ? G[(int64_t)i * W + j] : 0.0;
      }
  // loader: column tid & 127, rows (tid >> 7) + 2q of the stage
  const int sc = tid & 127, sr = tid >> 7;
  const int ci = i0 + sc, cj = j0 + sc;
  float ra[FK / 2], rb[FK / 2];
  auto fetch = [&](int n0) {
#pragma unroll
    for (int q = 0; q < FK / 2; ++q) {
      const int n = n0 + sr + 2 * q;
      ra[q] = (n < B && ci < W) ? d[(int64_t)n * ld + ci] : 0.f;
      rb[q] = (!diag && n < B && cj < W) ? d[(int64_t)n * ld + cj] : 0.f;
    }
  };
  fetch(0);
  for (int n0 = 0; n0 < B; n0 += FK) {
    __syncthreads();   // the previous stage has been consumed
#pragma unroll
    for (int q = 0; q < FK / 2; ++q) {
      As[sr + 2 * q][sc] = ra[q];
      if (!diag) Bs[sr + 2 * q][sc] = rb[q];
    }
    __syncthreads();
    if (n0 + FK < B) fetch(n0 + FK);   // in flight under this stage's MFMAs
#pragma unroll
    for (int k0 = 0; k0 < FK; k0 += 4) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = (double)As[k0 + lr][wi + 16 * u + lc];
        b[u] = (double)Bp[k0 + lr][wj + 16 * u + lc];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wi + 16 * u + lr + 4 * r, j = j0 + wj + 16 * v + lc;
        if (i < W && j < W) G[(int64_t)i * W + j] = acc[u][v][r];
      }
}

// A = the full symmetric matrix of G's upper triangle (G itself is kept)
__global__ __launch_bounds__(256) void fs_mirror_k(int W, const double* __restrict__ G,
                                                   double* __restrict__ A) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= W) return;
  A[(int64_t)i * W + j] = i <= j ? G[(int64_t)i * W + j] : G[(int64_t)j * W + i];
}

// vt [Rp][Kp] = V^T of nap_evec_k's V (row r = eigenvector W-1-r), zero padded
__global__ __launch_bounds__(256) void fs_vt_k(int W, int R, int Kp, const double* __restrict__ A,
                                               float* __restrict__ vt) {
  const int i = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (i >= Kp) return;
  vt[(int64_t)r * Kp + i] = (r < R && i < W) ? (float)A[(int64_t)(W - 1 - r) * W + i] : 0.f;
}

// stage [Mp][Kp] = fp32(d - mu) on the valid region, 0 elsewhere
__global__ __launch_bounds__(256) void fs_pack_k(int B, int W, const float* __restrict__ d, int64_t ld,
                                                 const float* __restrict__ mu, int Mp, int Kp,
                                                 float* __restrict__ stage) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Kp) return;
  const float m = c < W ? mu[c] : 0.f;
  for (int r = blockIdx.y; r < Mp; r += gridDim.y)
    stage[(int64_t)r * Kp + c] = (r < B && c < W) ? d[(int64_t)r * ld + c] - m : 0.f;
}

// the rotation GEMM's Welford partials (mean, M2 of the valid rows of each
// 32-row chunk) as fp64 sum / sum of squares, added to rsum [2][R] in chunk order
__global__ __launch_bounds__(256) void fs_rotsum_k(int B, int R, int Rp, const float* __restrict__ stats,
                                                   double* __restrict__ rsum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= R) return;
  double s1 = rsum[c], s2 = rsum[R + c];
  for (int p = 0; p * MMAD_PART_ROWS < B; ++p) {
    const int left = B - p * MMAD_PART_ROWS;
    const double cnt = left < MMAD_PART_ROWS ? left : MMAD_PART_ROWS;
    const double mean = stats[(int64_t)p * 2 * Rp + c], q = stats[((int64_t)p * 2 + 1) * Rp + c];
    s1 += cnt * mean;
    s2 += q + cnt * mean * mean;
  }
  rsum[c] = s1;
  rsum[R + c] = s2;
}

struct FitState {
  double* S;       // [W] running column sums
  double* G;       // [W][W] running Gram, upper-triangular tiles
  double* A;       // [W][W] mirrored G -> eigenvectors
  double* D;       // [W] eigenvalues
  double* E;       // [W] dsyevd scratch
  double* spart;   // [SUM_PARTS][W] column-sum partials of one launch
  double* rsum;    // [2][R] running sum / sum of squares of rot
  float* vt;       // [Kp][Kp] V^T, rows >= R zero
  float* zero;     // [Kp] the rotation GEMM's bias
  float* stage;    // [ROT_CHUNK][Kp] centred rows of one chunk
  float* y;        // [ROT_CHUNK][Kp] rot of one chunk
  float* stats;    // [ROT_CHUNK / 32][2][Kp]
  int* info;
  int64_t off_S, off_G, total;
};

FitState carve_state(int W, char* base) {
  const size_t Kp = (size_t)mmad_roundup(W, MMAD_PAD);
  FitState f{};
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al256(bytes); return p; };
  f.off_S = (int64_t)o;
  f.S = (double*)take((size_t)W * 8);
  f.off_G = (int64_t)o;
  f.G = (double*)take((size_t)W * W * 8);
  f.A = (double*)take((size_t)W * W * 8);
  f.D = (double*)take((size_t)W * 8);
  f.E = (double*)take((size_t)W * 8);
  f.spart = (double*)take((size_t)SUM_PARTS * W * 8);
  f.rsum = (double*)take((size_t)2 * W * 8);
  f.vt = (float*)take(Kp * Kp * 4);
  f.zero = (float*)take(Kp * 4);
  f.stage = (float*)take((size_t)ROT_CHUNK * Kp * 4);
  f.y = (float*)take((size_t)ROT_CHUNK * Kp * 4);
  f.stats = (float*)take((size_t)(ROT_CHUNK / MMAD_PART_ROWS) * 2 * Kp * 4);
  f.info = (int*)take(sizeof(int));
  f.total = (int64_t)o;
  return f;
}

// the checks every streaming entry point shares (nothing is launched on failure)
int check_state(const char* who, int W, const void* state, int64_t state_bytes) {
  MMAD_CHECK_ARG(W >= 1 && W <= 46340, "%s: bad width W=%d", who, W);
  MMAD_CHECK_ARG(state && ((uintptr_t)state) % 256 == 0, "%s: the fit state must be a 256-byte aligned buffer", who);
  const int64_t need = carve_state(W, nullptr).total;
  MMAD_CHECK_ARG(state_bytes >= need, "%s: fit state %lld < %lld bytes", who, (long long)state_bytes,
                 (long long)need);
  return MMAD_OK;
}
int check_batch(const char* who, int W, int B, const float* d, int64_t ld) {
  MMAD_CHECK_ARG(B >= 1 && d && ld >= W, "%s: bad batch (B=%d ld=%lld W=%d)", who, B, (long long)ld, W);
  return MMAD_OK;
}
#define FS_RET_IF(expr) do { const int rc_ = (expr); if (rc_ != MMAD_OK) return rc_; } while (0)

}  // namespace

int64_t mmad_nap_fit_state_bytes(int W) {
  if (W < 1 || W > 46340) return -1;
  return carve_state(W, nullptr).total;
}

int mmad_nap_fit_state_layout(int W, int64_t* info) {
  MMAD_CHECK_ARG(W >= 1 && W <= 46340 && info, "nap_fit_state_layout: bad arguments");
  const FitState f = carve_state(W, nullptr);
  info[0] = f.off_S;
  info[1] = f.off_G;
  info[2] = f.total;
  return MMAD_OK;
}

int mmad_nap_fit_begin(int W, void* state, int64_t state_bytes, void* stream) {
  FS_RET_IF(check_state("nap_fit_begin", W, state, state_bytes));
  const FitState f = carve_state(W, (char*)state);
  hipStream_t s = (hipStream_t)stream;
  // S and G are contiguous; rsum, vt and the zero bias likewise
  MMAD_HIP_CHECK(hipMemsetAsync(f.S, 0, (size_t)((char*)f.A - (char*)f.S), s));
  MMAD_HIP_CHECK(hipMemsetAsync(f.rsum, 0, (size_t)((char*)f.stage - (char*)f.rsum), s));
  return MMAD_OK;
}

int mmad_nap_fit_accumulate_sums(int W, int B, const float* d, int64_t ld, void* state,
                                 int64_t state_bytes, void* stream) {
  FS_RET_IF(check_state("nap_fit_accumulate_sums", W, state, state_bytes));
  FS_RET_IF(check_batch("nap_fit_accumulate_sums", W, B, d, ld));
  const FitState f = carve_state(W, (char*)state);
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0; r0 < B; r0 += SUM_PARTS * MEAN_ROWS) {
    const int rows = B - r0 < SUM_PARTS * MEAN_ROWS ? B - r0 : SUM_PARTS * MEAN_ROWS;
    const int parts = (rows + MEAN_ROWS - 1) / MEAN_ROWS;
    nap_colsum_k<<<dim3((W + MEAN_COLS - 1) / MEAN_COLS, parts), 256, 0, s>>>(rows, W, d + (int64_t)r0 * ld, ld,
                                                                               f.spart);
    MMAD_LAUNCH_CHECK();
    fs_addsum_k<<<(W + 255) / 256, 256, 0, s>>>(W, parts, f.spart, f.S);
    MMAD_LAUNCH_CHECK();
  }
  return MMAD_OK;
}

int mmad_nap_fit_finish_mean(int W, int64_t N, void* state, int64_t state_bytes, float* mu_r,
                             void* stream) {
  FS_RET_IF(check_state("nap_fit_finish_mean", W, state, state_bytes));
  MMAD_CHECK_ARG(N >= 2 && mu_r, "nap_fit_finish_mean: N=%lld < 2 or null mu_r", (long long)N);
  const FitState f = carve_state(W, (char*)state);
  nap_mean_k<<<(W + 255) / 256, 256, 0, (hipStream_t)stream>>>(N, W, 1, f.S, mu_r);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_nap_fit_accumulate_gram(int W, int B, float* d, int64_t ld, const float* mu_r, void* state,
                                 int64_t state_bytes, void* stream) {
  FS_RET_IF(check_state("nap_fit_accumulate_gram", W, state, state_bytes));
  FS_RET_IF(check_batch("nap_fit_accumulate_gram", W, B, d, ld));
  MMAD_CHECK_ARG(mu_r, "nap_fit_accumulate_gram: null mu_r");
  const FitState f = carve_state(W, (char*)state);
  hipStream_t s = (hipStream_t)stream;
  fs_centre_k<<<dim3((W + 255) / 256, B < 1024 ? B : 1024), 256, 0, s>>>(B, W, d, ld, mu_r);
  MMAD_LAUNCH_CHECK();
  const int T = (W + FT - 1) / FT;
  fs_gram_k<<<T * (T + 1) / 2, 256, 0, s>>>(B, W, d, ld, T, f.G);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_nap_fit_solve(int W, int64_t N, void* state, int64_t state_bytes, float* v, void* stream) {
  FS_RET_IF(check_state("nap_fit_solve", W, state, state_bytes));
  MMAD_CHECK_ARG(N >= 2 && v, "nap_fit_solve: N=%lld < 2 or null v", (long long)N);
  const SolverApi& api = solver();
  if (!api.ok) {
    mmad_set_error("nap_fit_solve: rocSOLVER / rocBLAS not found in the process (librocsolver.so.0)");
    return MMAD_EHIP;
  }
  const FitState f = carve_state(W, (char*)state);
  hipStream_t s = (hipStream_t)stream;
  const int R = (int)(N < W ? N : W), Kp = mmad_roundup(W, MMAD_PAD);
  fs_mirror_k<<<dim3((W + 255) / 256, W), 256, 0, s>>>(W, f.G, f.A);
  MMAD_LAUNCH_CHECK();
  FS_RET_IF(eig_sym(api, W, f.A, f.D, f.E, f.info, s));
  const int64_t nv = (int64_t)W * R;
  nap_evec_k<<<(unsigned)((nv + 255) / 256), 256, 0, s>>>(W, R, f.A, v);
  MMAD_LAUNCH_CHECK();
  fs_vt_k<<<dim3((Kp + 255) / 256, Kp), 256, 0, s>>>(W, R, Kp, f.A, f.vt);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}

int mmad_nap_fit_accumulate_rot(int W, int64_t N, int B, const float* d, int64_t ld,
                                const float* mu_r, void* state, int64_t state_bytes, void* stream) {
  FS_RET_IF(check_state("nap_fit_accumulate_rot", W, state, state_bytes));
  FS_RET_IF(check_batch("nap_fit_accumulate_rot", W, B, d, ld));
  MMAD_CHECK_ARG(N >= 2 && mu_r, "nap_fit_accumulate_rot: N=%lld < 2 or null mu_r", (long long)N);
  const FitState f = carve_state(W, (char*)state);
  hipStream_t s = (hipStream_t)stream;
  const int R = (int)(N < W ? N : W), Kp = mmad_roundup(W, MMAD_PAD), Rp = mmad_roundup(R, MMAD_PAD);
  for (int r0 = 0; r0 < B; r0 += ROT_CHUNK) {
    const int rows = B - r0 < ROT_CHUNK ? B - r0 : ROT_CHUNK;
    const int Mp = mmad_roundup(rows, MMAD_PAD);
    fs_pack_k<<<dim3((Kp + 255) / 256, Mp < 1024 ? Mp : 1024), 256, 0, s>>>(rows, W, d + (int64_t)r0 * ld, ld,
                                                                             mu_r, Mp, Kp, f.stage);
    MMAD_LAUNCH_CHECK();
    FS_RET_IF(mmad_fc_fwd(MMAD_F32, rows, R, W, Mp, Rp, Kp, f.stage, f.vt, f.zero, MMAD_ACT_NONE, 0.f,
                          nullptr, nullptr, f.y, f.stats, stream));
    fs_rotsum_k<<<(R + 255) / 256, 256, 0, s>>>(rows, R, Rp, f.stats, f.rsum);
    MMAD_LAUNCH_CHECK();
  }
  return MMAD_OK;
}

int mmad_nap_fit_finish(int W, int64_t N, void* state, int64_t state_bytes, float* mu_s, float* var,
                        void* stream) {
  FS_RET_IF(check_state("nap_fit_finish", W, state, state_bytes));
  MMAD_CHECK_ARG(N >= 2 && mu_s && var, "nap_fit_finish: N=%lld < 2 or a null output", (long long)N);
  const FitState f = carve_state(W, (char*)state);
  const int R = (int)(N < W ? N : W);
  nap_stats_k<<<(R + 255) / 256, 256, 0, (hipStream_t)stream>>>(N, R, 1, f.rsum, mu_s, var);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}
