// Microphone front end: MFCCs from raw PCM on the device (include/mmad.h,
// "Microphone front end").  Restates save_mfcc_from_wav
// (utils/data_loaders.py:676-701): librosa 0.8's melspectrogram (centred,
// reflect-padded frames, periodic Hann, n_fft = hop) -> power_to_db(ref=max,
// top_db=80) -> DCT-II ortho [:n_mfcc], and norm_vec (:703-712) of the last
// `keep` frames.  Three launches, everything after the PCM load in fp64:
//   mfcc_power_k   (frame, chunk of bins): windowed frame + twiddle table in
//                  LDS, direct DFT with an exact integer twiddle index;
//   mfcc_mel_k     one block per frame: sparse mel sums + the frame's maximum;
//   mfcc_finish_k  one block: global maximum, dB + clamp, DCT, out, norm_out.
// No atomics, no grid barrier, every reduction in a fixed order.
#include <math.h>

#include <vector>

#include "mmad_common.h"
#include "mmad_ops.h"

namespace {

constexpr int MFCC_NFFT_MIN = 16;
constexpr int MFCC_NFFT_MAX = 4410;
constexpr int MFCC_MELS_MAX = 128;
constexpr int MFCC_BINS_MAX = MFCC_NFFT_MAX / 2 + 1;   // power row stride in the workspace
constexpr int64_t MFCC_MAGIC = 0x4346464d44414d4dLL;   // "MMADMFCC"
constexpr int MFCC_HEADER = 8;                         // int64 words ahead of the tables
constexpr double MFCC_PI = 3.14159265358979323846;

// plan (doubles unless noted), 256-byte aligned, filled once by plan_init:
//   header int64[8]: magic, sr, n_fft, n_mels, n_mfcc, nnz, 0, 0 (the kernels
//                        check it against the call's parameters)
//   twiddle [n_fft][2]   cos, sin (2 pi j / n_fft)
//   window  [n_fft]      periodic Hann
//   dct     [n_mfcc][n_mels]
//   int32   fb_lo[n_mels], fb_cnt[n_mels], fb_off[n_mels]  (padded to 8 bytes)
//   fbw     [2 (n_fft/2 + 1)]  the filters' nonzero weights, filter after
//                        filter: a bin lies inside at most two triangles, so
//                        nnz <= 2 bins whatever sr is, and the plan's size
//                        needs no filterbank to compute
struct PlanLayout {
  int64_t twiddle, window, dct, idx, fbw, fbw_cap, bytes;   // offsets in doubles; bytes total
};
PlanLayout plan_layout(int n_fft, int n_mels, int n_mfcc) {
  PlanLayout p;
  p.twiddle = MFCC_HEADER;
  p.window = p.twiddle + 2 * (int64_t)n_fft;
  p.dct = p.window + n_fft;
  p.idx = p.dct + (int64_t)n_mfcc * n_mels;
  p.fbw = p.idx + (3 * (int64_t)n_mels + 1) / 2;
  p.fbw_cap = 2 * (int64_t)(n_fft / 2 + 1);
  p.bytes = ((p.fbw + p.fbw_cap) * 8 + 255) / 256 * 256;
  return p;
}

bool params_ok(int sr, int n_fft, int n_mels, int n_mfcc) {
  return sr >= 1 && n_fft >= MFCC_NFFT_MIN && n_fft <= MFCC_NFFT_MAX && n_mels >= 1 &&
         n_mels <= MFCC_MELS_MAX && n_mfcc >= 1 && n_mfcc <= n_mels;
}

// librosa.core.hz_to_mel / mel_to_hz, htk=False (Slaney)
const double F_SP = 200.0 / 3, MIN_LOG_HZ = 1000.0, MIN_LOG_MEL = MIN_LOG_HZ / F_SP;
double hz_to_mel(double f) {
  const double logstep = log(6.4) / 27.0;
  return f >= MIN_LOG_HZ ? MIN_LOG_MEL + log(f / MIN_LOG_HZ) / logstep : f / F_SP;
}
double mel_to_hz(double m) {
  const double logstep = log(6.4) / 27.0;
  return m >= MIN_LOG_MEL ? MIN_LOG_HZ * exp(logstep * (m - MIN_LOG_MEL)) : F_SP * m;
}
// np.linspace(a, b, n)[i], n >= 2
double linspace_at(double a, double b, int n, int i) {
  return i == n - 1 ? b : (double)i * ((b - a) / (n - 1)) + a;
}

// librosa.filters.mel(sr, n_fft, n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney')
void filterbank(int sr, int n_fft, int n_mels, double* fb) {
  const int nb = n_fft / 2 + 1;
  const double fmax = sr / 2.0, mel_lo = hz_to_mel(0.0), mel_hi = hz_to_mel(fmax);
  std::vector<double> f(n_mels + 2);
  for (int i = 0; i < n_mels + 2; ++i) f[i] = mel_to_hz(linspace_at(mel_lo, mel_hi, n_mels + 2, i));
  for (int m = 0; m < n_mels; ++m) {
    const double d0 = f[m + 1] - f[m], d1 = f[m + 2] - f[m + 1], enorm = 2.0 / (f[m + 2] - f[m]);
    for (int k = 0; k < nb; ++k) {
      const double fk = linspace_at(0.0, fmax, nb, k);
      const double lower = -(f[m] - fk) / d0, upper = (f[m + 2] - fk) / d1;
      const double w = lower < upper ? lower : upper;
      fb[(int64_t)m * nb + k] = (w > 0.0 ? w : 0.0) * enorm;
    }
  }
}

// each filter's nonzero run (a triangle: contiguous); returns the total count
int64_t sparse_ranges(const double* fb, int nb, int n_mels, int* lo, int* cnt) {
  int64_t nnz = 0;
  for (int m = 0; m < n_mels; ++m) {
    int a = nb, b = -1;
    for (int k = 0; k < nb; ++k)
      if (fb[(int64_t)m * nb + k] != 0.0) {
        if (k < a) a = k;
        b = k;
      }
    lo[m] = b < 0 ? 0 : a;
    cnt[m] = b < 0 ? 0 : b - a + 1;
    nnz += cnt[m];
  }
  return nnz;
}

// what the kernels need of the plan; every kernel checks the header first and
// writes nothing when it is not the plan the host launched for
struct PlanView {
  const int64_t* header;
  const double *twiddle, *window, *dct, *fbw;
  const int *fb_lo, *fb_cnt, *fb_off;
  int sr, n_fft, n_mels, n_mfcc;
};
__device__ __forceinline__ bool plan_matches(const PlanView& p) {
  return p.header[0] == MFCC_MAGIC && p.header[1] == p.sr && p.header[2] == p.n_fft &&
         p.header[3] == p.n_mels && p.header[4] == p.n_mfcc;
}

// ---- stage A: power spectrum ------------------------------------------------
// One block per (frame, chunk of owned bins).  LDS: the twiddle table [N][2]
// and the windowed frame [N], fp64 (105,840 B at N = 4410).  A thread owns bin
// k and walks n with idx = k n mod N kept by idx += k; if (idx >= N) idx -= N.
// Even and odd n accumulate apart: for even N,
//   w^{(N/2 - k) n} = (-1)^n conj(w^{k n}),
// so the same gathers also give bin N/2 - k (even sums minus odd sums) and a
// thread owns bins 0..N/4 only.  Odd N (2205): every bin 0..N/2 is owned.
template <typename T>
__global__ __launch_bounds__(256) void mfcc_power_k(const T* __restrict__ pcm, int64_t L, PlanView p,
                                                    int chunks, int owned, double* __restrict__ power) {
  __shared__ alignas(16) double sm[3 * MFCC_NFFT_MAX];
  if (!plan_matches(p)) return;
  const int N = p.n_fft;
  double2* tw = (double2*)sm;
  double* xs = sm + 2 * N;
  const int64_t frame = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const int64_t first = frame * N - N / 2;
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    int64_t i = first + j;
    i = i < 0 ? -i : i;
    i = i >= L ? 2 * (L - 1) - i : i;
    xs[j] = (double)pcm[i] * p.window[j];
    tw[j] = ((const double2*)p.twiddle)[j];
  }
  __syncthreads();
  const int k = chunk * blockDim.x + threadIdx.x;
  if (k >= owned) return;
  double re_e = 0, im_e = 0, re_o = 0, im_o = 0;
  int idx = 0;
  const int pairs = N >> 1;
#pragma unroll 4
  for (int q = 0; q < pairs; ++q) {
    const double2 a = tw[idx];
    idx += k;
    idx = idx >= N ? idx - N : idx;
    const double2 b = tw[idx];
    idx += k;
    idx = idx >= N ? idx - N : idx;
    const double x0 = xs[2 * q], x1 = xs[2 * q + 1];
    re_e = fma(x0, a.x, re_e);
    im_e = fma(x0, a.y, im_e);
    re_o = fma(x1, b.x, re_o);
    im_o = fma(x1, b.y, im_o);
  }
  if (N & 1) {
    const double2 a = tw[idx];
    const double x0 = xs[N - 1];
    re_e = fma(x0, a.x, re_e);
    im_e = fma(x0, a.y, im_e);
  }
  double* row = power + frame * MFCC_BINS_MAX;
  const double re = re_e + re_o, im = im_e + im_o;
  row[k] = re * re + im * im;
  if (!(N & 1)) {
    const int k2 = N / 2 - k;
    const double re2 = re_e - re_o, im2 = im_e - im_o;
    if (k2 != k) row[k2] = re2 * re2 + im2 * im2;
  }
}

// ---- stage B: mel power and the frame's maximum ----------------------------
__global__ __launch_bounds__(MFCC_MELS_MAX) void mfcc_mel_k(PlanView p, const double* __restrict__ power,
                                                            double* __restrict__ mel,
                                                            double* __restrict__ fmax_out) {
  __shared__ double red[MFCC_MELS_MAX];
  if (!plan_matches(p)) return;
  const int64_t frame = blockIdx.x;
  const int m = threadIdx.x;
  double s = 0.0;
  if (m < p.n_mels) {
    const double* row = power + frame * MFCC_BINS_MAX + p.fb_lo[m];
    const double* w = p.fbw + p.fb_off[m];
    const int cnt = p.fb_cnt[m];
    for (int i = 0; i < cnt; ++i) s = fma(w[i], row[i], s);
    mel[frame * p.n_mels + m] = s;
  }
  red[m] = s;   // mel power is >= 0: the padding lanes' 0 never wins over a real maximum
  __syncthreads();
  for (int h = MFCC_MELS_MAX / 2; h > 0; h >>= 1) {
    if (m < h) red[m] = red[m] > red[m + h] ? red[m] : red[m + h];
    __syncthreads();
  }
  if (m == 0) fmax_out[frame] = red[0];
}

// ---- stage C: decibels, DCT, out, norm_out ----------------------------------
constexpr int FIN_THREADS = 256;

__device__ __forceinline__ double block_max(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int h = FIN_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = red[t] > red[t + h] ? red[t] : red[t + h];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(FIN_THREADS) void mfcc_finish_k(PlanView p, int64_t F, double* __restrict__ mel,
                                                             const double* __restrict__ fmax_in,
                                                             double* __restrict__ mf64,
                                                             float* __restrict__ out, int64_t keep, double lo,
                                                             double hi, float* __restrict__ norm_out) {
  __shared__ double red[FIN_THREADS];
  if (!plan_matches(p)) return;
  const int t = threadIdx.x, M = p.n_mels, C = p.n_mfcc;
  double mx = 0.0;
  for (int64_t f = t; f < F; f += FIN_THREADS) mx = fmax_in[f] > mx ? fmax_in[f] : mx;
  const double gmax = block_max(mx, red);
  // power_to_db(S, ref=np.max, amin=1e-10, top_db=80): log_spec.max() is the
  // maximal element's ref - ref = 0 exactly, so the floor is -80
  const double ref = 10.0 * log10(gmax > 1e-10 ? gmax : 1e-10);
  for (int64_t e = t; e < F * M; e += FIN_THREADS) {
    const double s = mel[e];
    const double db = 10.0 * log10(s > 1e-10 ? s : 1e-10) - ref;
    mel[e] = db > -80.0 ? db : -80.0;
  }
  __syncthreads();
  const int64_t kept0 = (F - keep) * C;
  double vmin = INFINITY, vmax = -INFINITY;
  for (int64_t o = t; o < F * C; o += FIN_THREADS) {
    const int64_t f = o / C;
    const int c = (int)(o - f * C);
    const double* b = p.dct + (int64_t)c * M;
    const double* d = mel + f * M;
    double v = 0.0;
    for (int m = 0; m < M; ++m) v = fma(b[m], d[m], v);
    out[o] = (float)v;
    mf64[o] = v;
    if (o >= kept0) {
      vmin = v < vmin ? v : vmin;
      vmax = v > vmax ? v : vmax;
    }
  }
  if (!norm_out) return;
  // norm_vec over the kept frames' values: (hi - lo) (v - min) / (max - min) + lo
  vmax = block_max(vmax, red);
  vmin = -block_max(-vmin, red);   // ends in a barrier: mf64 is visible to the block
  const double r_out = hi - lo, r_in = vmax - vmin;
  for (int64_t o = t; o < keep * C; o += FIN_THREADS)
    norm_out[o] = (float)(r_out * (mf64[kept0 + o] - vmin) / r_in + lo);
}

// workspace (doubles): power [F][MFCC_BINS_MAX] | mel [F][n_mels] | fmax [F] |
// mfcc [F][n_mels] (n_mfcc <= n_mels)
int64_t ws_doubles(int64_t F, int n_mels) { return F * (MFCC_BINS_MAX + 2 * (int64_t)n_mels + 1); }

}  // namespace

int64_t mmad_mfcc_frames(int64_t L, int n_fft) {
  if (n_fft < 1 || L < n_fft / 2 + 1) return -1;
  return 1 + (L + 2 * (int64_t)(n_fft / 2) - n_fft) / n_fft;
}

int mmad_mfcc_filterbank(int sr, int n_fft, int n_mels, double* fb) {
  MMAD_CHECK_ARG(params_ok(sr, n_fft, n_mels, 1) && fb,
                 "mfcc_filterbank: bad arguments (sr=%d n_fft=%d n_mels=%d; n_fft 16..4410, n_mels 1..128)", sr,
                 n_fft, n_mels);
  filterbank(sr, n_fft, n_mels, fb);
  return MMAD_OK;
}

int64_t mmad_mfcc_plan_bytes(int sr, int n_fft, int n_mels, int n_mfcc) {
  if (!params_ok(sr, n_fft, n_mels, n_mfcc)) return -1;
  return plan_layout(n_fft, n_mels, n_mfcc).bytes;
}

int mmad_mfcc_plan_init(void* plan, int64_t bytes, int sr, int n_fft, int n_mels, int n_mfcc, void* stream) {
  MMAD_CHECK_ARG(params_ok(sr, n_fft, n_mels, n_mfcc),
                 "mfcc_plan_init: bad parameters (sr=%d n_fft=%d n_mels=%d n_mfcc=%d; n_fft 16..4410, n_mels "
                 "1..128, n_mfcc 1..n_mels)", sr, n_fft, n_mels, n_mfcc);
  MMAD_CHECK_ARG(plan && ((uintptr_t)plan & 255) == 0, "mfcc_plan_init: plan null or not 256-byte aligned");
  const int nb = n_fft / 2 + 1;
  std::vector<double> fb((size_t)n_mels * nb);
  std::vector<int> lo(n_mels), cnt(n_mels);
  filterbank(sr, n_fft, n_mels, fb.data());
  const int64_t nnz = sparse_ranges(fb.data(), nb, n_mels, lo.data(), cnt.data());
  const PlanLayout pl = plan_layout(n_fft, n_mels, n_mfcc);
  MMAD_CHECK_ARG(bytes >= pl.bytes, "mfcc_plan_init: plan of %lld bytes, needs %lld", (long long)bytes,
                 (long long)pl.bytes);
  MMAD_CHECK_ARG(nnz <= pl.fbw_cap, "mfcc_plan_init: %lld filter weights exceed the plan's %lld", (long long)nnz,
                 (long long)pl.fbw_cap);
  std::vector<double> host((size_t)pl.bytes / 8, 0.0);
  int64_t* hd = (int64_t*)host.data();
  hd[0] = MFCC_MAGIC, hd[1] = sr, hd[2] = n_fft, hd[3] = n_mels, hd[4] = n_mfcc, hd[5] = nnz;
  for (int j = 0; j < n_fft; ++j) {
    const double a = 2.0 * MFCC_PI * j / n_fft;
    host[pl.twiddle + 2 * j] = cos(a);
    host[pl.twiddle + 2 * j + 1] = sin(a);
    host[pl.window + j] = 0.5 - 0.5 * cos(a);
  }
  // scipy.fftpack.dct(type=2, norm='ortho') rows 0..n_mfcc-1
  for (int c = 0; c < n_mfcc; ++c)
    for (int m = 0; m < n_mels; ++m)
      host[pl.dct + (int64_t)c * n_mels + m] =
          c == 0 ? sqrt(1.0 / n_mels) : sqrt(2.0 / n_mels) * cos(MFCC_PI * (2 * m + 1) * c / (2.0 * n_mels));
  int* ix = (int*)(host.data() + pl.idx);
  int64_t off = 0;
  for (int m = 0; m < n_mels; ++m) {
    ix[m] = lo[m], ix[n_mels + m] = cnt[m], ix[2 * n_mels + m] = (int)off;
    for (int i = 0; i < cnt[m]; ++i) host[pl.fbw + off + i] = fb[(int64_t)m * nb + lo[m] + i];
    off += cnt[m];
  }
  hipStream_t s = (hipStream_t)stream;
  MMAD_HIP_CHECK(hipMemcpyAsync(plan, host.data(), (size_t)pl.bytes, hipMemcpyHostToDevice, s));
  // the staging vector dies with this call: the copy must have read it
  MMAD_HIP_CHECK(hipStreamSynchronize(s));
  return MMAD_OK;
}

int64_t mmad_mfcc_ws_bytes(int64_t n_frames, int n_mels) {
  if (n_frames < 1 || n_mels < 1 || n_mels > MFCC_MELS_MAX) return -1;
  return (ws_doubles(n_frames, n_mels) * 8 + 255) / 256 * 256;
}

// the launch shape of F frames: 128-thread blocks while they all fit on the
// chip's 256 CUs at once (one block a CU at n_fft 4410: LDS), 256-thread
// blocks beyond
struct PowerGrid { int owned, threads, chunks; };
static PowerGrid power_grid(int64_t F, int n_fft) {
  PowerGrid g;
  g.owned = (n_fft & 1) ? n_fft / 2 + 1 : n_fft / 4 + 1;
  g.threads = F * ((g.owned + 127) / 128) > 256 ? 256 : 128;
  g.chunks = (g.owned + g.threads - 1) / g.threads;
  return g;
}

int mmad_mfcc_check(const void* pcm, int pcm_type, int64_t L, int sr, int n_fft, int n_mels, int n_mfcc,
                    const void* plan, int64_t plan_bytes, const float* out, int64_t keep,
                    const float* norm_out, const void* ws, int64_t ws_bytes) {
  MMAD_CHECK_ARG(params_ok(sr, n_fft, n_mels, n_mfcc),
                 "mfcc: bad parameters (sr=%d n_fft=%d n_mels=%d n_mfcc=%d; n_fft 16..4410, n_mels 1..128, "
                 "n_mfcc 1..n_mels)", sr, n_fft, n_mels, n_mfcc);
  MMAD_CHECK_ARG(pcm && plan && out && ws, "mfcc: null pcm, plan, out or ws");
  MMAD_CHECK_ARG(pcm_type == MMAD_PCM_I16 || pcm_type == MMAD_PCM_F32, "mfcc: unknown pcm_type %d", pcm_type);
  MMAD_CHECK_ARG(((uintptr_t)plan & 255) == 0 && ((uintptr_t)ws & 255) == 0,
                 "mfcc: plan or ws not 256-byte aligned");
  const int64_t F = mmad_mfcc_frames(L, n_fft);
  MMAD_CHECK_ARG(F >= 1, "mfcc: L=%lld too short for n_fft=%d (needs n_fft/2 + 1 samples to reflect)",
                 (long long)L, n_fft);
  MMAD_CHECK_ARG(keep >= 1 && keep <= F, "mfcc: keep=%lld outside 1..%lld frames", (long long)keep, (long long)F);
  MMAD_CHECK_ARG(ws_bytes >= mmad_mfcc_ws_bytes(F, n_mels), "mfcc: workspace of %lld bytes, needs %lld",
                 (long long)ws_bytes, (long long)mmad_mfcc_ws_bytes(F, n_mels));
  const PlanLayout pl = plan_layout(n_fft, n_mels, n_mfcc);
  MMAD_CHECK_ARG(plan_bytes >= pl.bytes, "mfcc: plan of %lld bytes, needs %lld", (long long)plan_bytes,
                 (long long)pl.bytes);
  MMAD_CHECK_ARG(F * power_grid(F, n_fft).chunks < (1LL << 31), "mfcc: %lld frames are too many for one call",
                 (long long)F);
  return MMAD_OK;
}

int mmad_mfcc(const void* pcm, int pcm_type, int64_t L, int sr, int n_fft, int n_mels, int n_mfcc,
              const void* plan, int64_t plan_bytes, float* out, int64_t keep, float lo, float hi, float* norm_out,
              void* ws, int64_t ws_bytes, void* stream) {
  const int rc = mmad_mfcc_check(pcm, pcm_type, L, sr, n_fft, n_mels, n_mfcc, plan, plan_bytes, out, keep, norm_out,
                                 ws, ws_bytes);
  if (rc != MMAD_OK) return rc;
  const int64_t F = mmad_mfcc_frames(L, n_fft);
  const PlanLayout pl = plan_layout(n_fft, n_mels, n_mfcc);
  const PowerGrid pg = power_grid(F, n_fft);
  const int owned = pg.owned, threads = pg.threads, chunks = pg.chunks;

  PlanView v;
  const double* base = (const double*)plan;
  v.header = (const int64_t*)plan;
  v.twiddle = base + pl.twiddle, v.window = base + pl.window, v.dct = base + pl.dct, v.fbw = base + pl.fbw;
  v.fb_lo = (const int*)(base + pl.idx), v.fb_cnt = v.fb_lo + n_mels, v.fb_off = v.fb_cnt + n_mels;
  v.sr = sr, v.n_fft = n_fft, v.n_mels = n_mels, v.n_mfcc = n_mfcc;
  double* power = (double*)ws;
  double* mel = power + F * MFCC_BINS_MAX;
  double* fmax = mel + F * n_mels;
  double* mf64 = fmax + F;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(F * chunks);
  if (pcm_type == MMAD_PCM_I16)
    mfcc_power_k<int16_t><<<grid, threads, 0, s>>>((const int16_t*)pcm, L, v, chunks, owned, power);
  else
    mfcc_power_k<float><<<grid, threads, 0, s>>>((const float*)pcm, L, v, chunks, owned, power);
  MMAD_LAUNCH_CHECK();
  mfcc_mel_k<<<(unsigned)F, MFCC_MELS_MAX, 0, s>>>(v, power, mel, fmax);
  MMAD_LAUNCH_CHECK();
  mfcc_finish_k<<<1, FIN_THREADS, 0, s>>>(v, F, mel, fmax, mf64, out, keep, (double)lo, (double)hi, norm_out);
  MMAD_LAUNCH_CHECK();
  return MMAD_OK;
}
