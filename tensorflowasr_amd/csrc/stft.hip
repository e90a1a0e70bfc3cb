// Ragged STFT / ISTFT pair with librosa 0.9 semantics (center=True, reflect padding, a periodic Hann window of win_length
// zero-padded to n_fft), the reference's SignalSpecAug on top of it in one frame-local pass, and librosa's phase vocoder: behind
// mi355asr_stft_ragged, mi355asr_istft_ragged, mi355asr_spec_aug and mi355asr_phase_vocoder of include/mi355asr.h.
//
// frame_kernel: one workgroup (four waves) per frame, both DFT stages of both directions on v_mfma_f32_16x16x4_f32 (exact fp32
// products), through the factorisation fft_stft.hip uses, N = 32 x N2 with N2 = 32 (1024) or 64 (2048):
//   forward, n = N2 n1 + n2, k = k1 + 32 k2:
//     A[k1][n2] = sum_n1 W32^(n1 k1) xw[N2 n1 + n2]              stage 1: [64 (re | im of k1)] x [32] times [32] x [N2]
//     B[k1][n2] = A[k1][n2] W_N^(n2 k1)                          twiddle, written transposed
//     X[k1 + 32 k2] = sum_n2 W_N2^(n2 k2) B[k1][n2], k2 < N2/2   stage 2: [N2 (re | im of k2)] x [2 N2] times [2 N2] x [32]
//     X[N/2] = sum_n (-1)^n xw[n]                                a wave reduction in a fixed order
//   inverse, k = N2 k1 + k2, n = p + 32 q, on the full Hermitian spectrum F (F[N - k] = conj F[k], Im F[0] = Im F[N/2] = 0):
//     A[p][k2] = sum_k1 conj W32^(p k1) F[N2 k1 + k2]            stage 1: [64] x [64] times [64 (re | im of k1)] x [N2]
//     B[p][k2] = A[p][k2] conj W_N^(k2 p)                        twiddle, written transposed
//     y[p + 32 q] = Re sum_k2 conj W_N2^(k2 q) B[p][k2] / N      stage 2: [N2] x [2 N2] times [2 N2] x [32]
// Every product is T x M with T a table computed in float64 on the host and packed in fragment order (the A operand: one
// coalesced 256-byte load per MFMA) and M a matrix in LDS (the B operand); the accumulator tiles are shared out over the four
// waves, each tile one chain over k ascending.  A frame is computed from its own samples alone, so a row of a ragged batch
// equals the row alone bit for bit, and nothing depends on timing (no atomics).
//   MODE_STFT:    samples -> spectrum in memory
//   MODE_ISTFT:   spectrum in memory -> windowed time-domain frame (win_length samples) in the workspace
//   MODE_SPECAUG: samples -> spectrum in LDS -> the blocks around the centres zeroed -> windowed frame in the workspace; the
//                 spectrum never leaves the chip
// ola_kernel: owner computes.  The thread of output sample n adds the ceil(win_length / hop) frames that cover it in ascending
// frame order, and the squared window along with them, and divides where the sum exceeds tiny(float32).
// vocoder_kernel: one lane owns one bin of one row and walks the output frames; the time step t * rate is float64, the expected
// phase advance comes from a host table reduced modulo 2 pi in float64, and the accumulated phase is kept in [-pi, pi].
#include "common.h"
#include "dft_mfma.h"
#include "model.h"

namespace {

constexpr int kStftThreads = 256;
constexpr int kOlaTile = 256;                            // outputs per workgroup of ola_kernel
constexpr int kLDT = 48;                                 // row stride of the transposed matrix between the stages
constexpr int kSpecAugBins = 513;
enum { MODE_STFT = 0, MODE_ISTFT = 1, MODE_SPECAUG = 2 };

struct StftTables {
  const float* win;       // [N] the padded window
  const float* wsq;       // [N] its square (float64, rounded once)
  DftTables dft;          // twiddles and packed stage matrices; T4 carries 1 / N
  const float* phi;       // [N/2 + 1] pi hop k / (N/2) reduced to [-pi, pi] in float64
};

struct FrameArgs {
  StftTables t;
  const void* x;          // [B, Lpad] float or int16 (MODE_STFT, MODE_SPECAUG)
  const int32_t* len;     // [B]
  int64_t Lpad;
  float* S;               // [B, Fpad, N/2 + 1, 2]: written by MODE_STFT, read by MODE_ISTFT
  const int32_t* frames_in;   // [B] (MODE_ISTFT)
  int32_t* frames_out;    // [B] or null (MODE_STFT)
  const int32_t* centres; // [B, Npad, 2] (h_, w_)
  const int32_t* counts;  // [B]
  float* fr;              // [B, Fpad, win] windowed frames
  int Fpad, Npad, window, win, hop;
};

DEV float to_f32(float v) { return v; }
DEV float to_f32(int16_t v) { return (float)v * (1.0f / 32768.0f); }

// frames of a row of L samples: reflect padding needs L >= N/2 + 1
DEV int row_frames(int64_t L, int N, int hop) { return L >= N / 2 + 1 ? 1 + (int)(L / hop) : 0; }

template <int N2, typename T, int MODE>
__global__ __launch_bounds__(kStftThreads) void frame_kernel(FrameArgs a) {
  constexpr int N = 32 * N2, LDX = N2 + 8, BINS = N / 2 + 1;
  __shared__ __attribute__((aligned(16))) float bufA[2 * 32 * LDX];   // the windowed frame / the full spectrum / the inverse
  __shared__ __attribute__((aligned(16))) float bufD[64 * LDX];       // stage-1 output / the half spectrum (re [N/2], im [N/2])
  __shared__ __attribute__((aligned(16))) float bufT[2 * N2 * kLDT];  // twiddled, transposed
  __shared__ float red[8];                                            // [0..3] wave partials, [4] the Nyquist bin
  const int tid = threadIdx.x;
  const int b = blockIdx.y, f = blockIdx.x;
  int F;
  int64_t L = 0;
  if constexpr (MODE == MODE_ISTFT) {
    F = a.frames_in[b];
    F = F < 0 ? 0 : (F > a.Fpad ? a.Fpad : F);
  } else {
    L = a.len[b];
    L = L < 0 ? 0 : (L > a.Lpad ? a.Lpad : L);
    F = row_frames(L, N, a.hop);
    F = F > a.Fpad ? a.Fpad : F;
    if constexpr (MODE == MODE_STFT)
      if (a.frames_out && f == 0 && tid == 0) a.frames_out[b] = F;
  }
  if (f >= F) {                                                       // uniform over the workgroup
    if constexpr (MODE == MODE_STFT) {
      float* row = a.S + ((size_t)b * a.Fpad + f) * (2 * BINS);
      for (int i = tid; i < 2 * BINS; i += kStftThreads) row[i] = 0.0f;
    }
    return;
  }
  float* Sre = bufD;
  float* Sim = bufD + N / 2;

  if constexpr (MODE != MODE_ISTFT) {
    // ---- the windowed frame, reflect-padded by N/2: sample j = f hop + n - N/2, -j below 0, 2 (L - 1) - j from L on
    const T* x = reinterpret_cast<const T*>(a.x) + (size_t)b * a.Lpad;
    float part = 0.0f;
    for (int n = tid; n < N; n += kStftThreads) {
      int64_t j = (int64_t)f * a.hop + n - N / 2;
      if (j < 0) j = -j;
      if (j >= L) j = 2 * (L - 1) - j;
      j = j < 0 ? 0 : (j >= L ? L - 1 : j);                           // cannot happen for f < F; keeps any index inside the row
      const float v = to_f32(x[j]) * a.t.win[n];
      bufA[(n / N2) * LDX + (n % N2)] = v;
      part += v;                                                      // n and tid have the same parity: the sign comes below
    }
    if (tid & 1) part = -part;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) part += __shfl_xor(part, off);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    // ---- forward stage 1: bufD[(re | im) k1][n2]
    dft_block_gemm<kStftThreads, 4, N2 / 16, 8>(a.t.dft.T1, bufA, LDX, [&](int r, int col, float v) { bufD[r * LDX + col] = v; });
    __syncthreads();
    // ---- twiddle, transposed: bufT[(re | im) n2][k1]
    for (int i = tid; i < 32 * N2; i += kStftThreads) {
      const int k1 = i / N2, n2 = i - k1 * N2;
      const float are = bufD[k1 * LDX + n2], aim = bufD[(32 + k1) * LDX + n2];
      const float tc = a.t.dft.twc[i], ts = a.t.dft.tws[i];
      bufT[n2 * kLDT + k1] = fmaf(are, tc, __fmul_rn(aim, ts));
      bufT[(N2 + n2) * kLDT + k1] = fmaf(aim, tc, -__fmul_rn(are, ts));
    }
    const float nyq = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    // ---- forward stage 2: row r < N2/2 is Re X[32 r + col], row N2/2 + r is Im X[32 r + col]
    dft_block_gemm<kStftThreads, N2 / 16, 2, N2 / 2>(a.t.dft.T2, bufT, kLDT, [&](int r, int col, float v) { bufD[r * 32 + col] = v; });
    if (tid == 0) red[4] = nyq;
    __syncthreads();
  }

  if constexpr (MODE == MODE_STFT) {
    float* row = a.S + ((size_t)b * a.Fpad + f) * (2 * BINS);
    for (int k = tid; k < BINS; k += kStftThreads) {
      row[2 * k] = k < N / 2 ? Sre[k] : red[4];
      row[2 * k + 1] = k < N / 2 ? Sim[k] : 0.0f;
    }
    return;
  }

  if constexpr (MODE == MODE_ISTFT) {
    const float* row = a.S + ((size_t)b * a.Fpad + f) * (2 * BINS);
    for (int k = tid; k < BINS; k += kStftThreads) {
      if (k < N / 2) {
        Sre[k] = row[2 * k];
        Sim[k] = row[2 * k + 1];
      } else {
        red[4] = row[2 * k];
      }
    }
    __syncthreads();
  }

  if constexpr (MODE == MODE_SPECAUG) {
    // ---- SignalSpecAug's blocks: centre (h_, w_) zeroes bins [max(h_ - window, 0), h_ + window) of the frames
    //      [max(w_ - window, 0), w_ + window)
    int cnt = a.counts[b];
    cnt = cnt < 0 ? 0 : (cnt > a.Npad ? a.Npad : cnt);
    const int32_t* ce = a.centres + (size_t)b * a.Npad * 2;
    const int64_t win = a.window;
    // a thread looks at every 256th centre and zeroes the bins of those that cover this frame itself (about 2 window cnt / F
    // of them do): zeroing twice is zeroing once, so the order of the centres does not matter
    for (int ci = tid; ci < cnt; ci += kStftThreads) {
      const int64_t h_ = ce[2 * ci], w_ = ce[2 * ci + 1];
      const int64_t wlo = w_ - win > 0 ? w_ - win : 0;
      if (f < wlo || f >= w_ + win) continue;
      const int64_t klo = h_ - win > 0 ? h_ - win : 0;
      const int64_t khi = h_ + win < BINS ? h_ + win : BINS;
      for (int64_t k = klo; k < khi; ++k) {
        if (k < N / 2) {
          Sre[k] = 0.0f;
          Sim[k] = 0.0f;
        } else {
          red[4] = 0.0f;
        }
      }
    }
    __syncthreads();
  }

  // ---- the full spectrum: bufA[(re | im) k1][k2], k = N2 k1 + k2
  for (int k = tid; k < N; k += kStftThreads) {
    const int kk = k <= N / 2 ? k : N - k;
    const float re = kk == N / 2 ? red[4] : Sre[kk];
    float im = (kk == N / 2 || kk == 0) ? 0.0f : Sim[kk];
    if (k > N / 2) im = -im;
    const int o = (k / N2) * LDX + (k % N2);
    bufA[o] = re;
    bufA[32 * LDX + o] = im;
  }
  __syncthreads();
  // ---- inverse stage 1: bufD[(re | im) p][k2]
  dft_block_gemm<kStftThreads, 4, N2 / 16, 16>(a.t.dft.T3, bufA, LDX, [&](int r, int col, float v) { bufD[r * LDX + col] = v; });
  __syncthreads();
  for (int i = tid; i < 32 * N2; i += kStftThreads) {
    const int p = i / N2, k2 = i - p * N2;
    const float are = bufD[p * LDX + k2], aim = bufD[(32 + p) * LDX + k2];
    const float tc = a.t.dft.twc[i], ts = a.t.dft.tws[i];
    bufT[k2 * kLDT + p] = fmaf(are, tc, -__fmul_rn(aim, ts));
    bufT[(N2 + k2) * kLDT + p] = fmaf(are, ts, __fmul_rn(aim, tc));
  }
  __syncthreads();
  // ---- inverse stage 2: bufA[32 q + p] = y[n], 1 / N included in the table
  dft_block_gemm<kStftThreads, N2 / 16, 2, N2 / 2>(a.t.dft.T4, bufT, kLDT, [&](int r, int col, float v) { bufA[r * 32 + col] = v; });
  __syncthreads();
  const int off = (N - a.win) / 2;
  float* out = a.fr + ((size_t)b * a.Fpad + f) * a.win;
  for (int j = tid; j < a.win; j += kStftThreads) out[j] = bufA[j + off] * a.t.win[j + off];
}

struct OlaArgs {
  const float* fr;        // [B, Fpad, win]
  const float* wsq;       // [N]
  const int32_t* frames;  // [B], or null: from len
  const int32_t* len;     // [B]
  const int32_t* out_len; // [B], or null: hop (F - 1)
  const void* x;          // [B, Lpad], or null; rows without a frame are copied from it (spec_aug)
  float* y;               // [B, Opad]
  int64_t Lpad, Opad;
  int Fpad, N, win, hop;
};

template <typename T>
__global__ __launch_bounds__(kOlaTile) void ola_kernel(OlaArgs a) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * kOlaTile + threadIdx.x;
  if (n >= a.Opad) return;
  int F;
  int64_t L = 0;
  if (a.frames) {
    F = a.frames[b];
    F = F < 0 ? 0 : F;
  } else {
    L = a.len[b];
    L = L < 0 ? 0 : (L > a.Lpad ? a.Lpad : L);
    F = row_frames(L, a.N, a.hop);
  }
  F = F > a.Fpad ? a.Fpad : F;
  float* y = a.y + (size_t)b * a.Opad;
  if (a.x && F == 0) {                                                // too short for a frame: the row as it came
    y[n] = n < L ? to_f32(reinterpret_cast<const T*>(a.x)[(size_t)b * a.Lpad + n]) : 0.0f;
    return;
  }
  int64_t ol = F > 0 ? (int64_t)a.hop * (F - 1) : 0;
  if (a.out_len) ol = a.out_len[b] < 0 ? 0 : a.out_len[b];
  if (n >= ol || F == 0) {
    y[n] = 0.0f;
    return;
  }
  const int off = (a.N - a.win) / 2;
  const int64_t m = n + a.N / 2 - off;                                // frame f covers m when 0 <= m - f hop < win
  const int64_t lo = m - a.win + 1;
  int64_t f0 = lo > 0 ? (lo + a.hop - 1) / a.hop : 0;
  int64_t f1 = m >= 0 ? m / a.hop : -1;
  if (f1 > F - 1) f1 = F - 1;
  const float* fr = a.fr + (size_t)b * a.Fpad * a.win;
  float acc = 0.0f, wss = 0.0f;
  for (int64_t f = f0; f <= f1; ++f) {
    const int j = (int)(m - f * a.hop);
    acc += fr[(size_t)f * a.win + j];
    wss += a.wsq[j + off];
  }
  y[n] = wss > 1.17549435e-38f ? acc / wss : acc;
}

struct VocoderArgs {
  const float* S;         // [B, Fpad, bins, 2]
  float* O;               // [B, Tpad, bins, 2]
  const int32_t* frames;  // [B]
  const double* rates;    // [B]
  const int32_t* tcount;  // [B]
  const float* phi;       // [bins]
  int Fpad, Tpad, bins;
};

DEV float wrap_pi(float v) {                                          // v - 2 pi round(v / 2 pi), 2 pi as two floats
  const float r = rintf(v * 0.15915494309189535f);
  v = fmaf(-r, 6.2831854820251465f, v);
  return fmaf(-r, -1.7484555e-07f, v);
}

__global__ __launch_bounds__(kStftThreads) void vocoder_kernel(VocoderArgs a) {
  const int k = blockIdx.x * kStftThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (k >= a.bins) return;
  int F = a.frames[b];
  F = F < 0 ? 0 : (F > a.Fpad ? a.Fpad : F);
  int Tn = a.tcount[b];
  Tn = Tn < 0 ? 0 : (Tn > a.Tpad ? a.Tpad : Tn);
  const double rate = a.rates[b];
  const float* S = a.S + (size_t)b * a.Fpad * a.bins * 2 + 2 * k;
  float* O = a.O + (size_t)b * a.Tpad * a.bins * 2 + 2 * k;
  const size_t fs = (size_t)a.bins * 2;
  const float phi = a.phi[k];
  float pa = F > 0 ? atan2f(S[1], S[0]) : 0.0f;
  for (int t = 0; t < Tn; ++t) {
    const double step = (double)t * rate;
    const int64_t i0 = (int64_t)step;
    const float alpha = (float)(step - (double)i0);
    float c0r = 0.f, c0i = 0.f, c1r = 0.f, c1i = 0.f;
    if (i0 >= 0 && i0 < F) { c0r = S[i0 * fs]; c0i = S[i0 * fs + 1]; }
    if (i0 + 1 >= 0 && i0 + 1 < F) { c1r = S[(i0 + 1) * fs]; c1i = S[(i0 + 1) * fs + 1]; }
    const float m0 = sqrtf(fmaf(c0r, c0r, c0i * c0i)), m1 = sqrtf(fmaf(c1r, c1r, c1i * c1i));
    const float mag = fmaf(alpha, m1, (1.0f - alpha) * m0);
    O[t * fs] = mag * cosf(pa);
    O[t * fs + 1] = mag * sinf(pa);
    const float dp = wrap_pi(atan2f(c1i, c1r) - atan2f(c0i, c0r) - phi);
    pa = wrap_pi(pa + (phi + dp));
  }
  for (int t = Tn; t < a.Tpad; ++t) {
    O[t * fs] = 0.0f;
    O[t * fs + 1] = 0.0f;
  }
}

// ---- host: sizes, tables ------------------------------------------------------------------------------------------------------------
struct StftGeo { int N2, N, win, hop; };

int stft_geo(int n_fft, int win, int hop, StftGeo* g) {
  if (n_fft == 1024 && win == 800 && hop == 160) { *g = StftGeo{32, 1024, 800, 160}; return 0; }
  if (n_fft == 2048 && win == 2048 && hop == 512) { *g = StftGeo{64, 2048, 2048, 512}; return 0; }
  return fail(MI355ASR_EINVAL, "stft: (n_fft, win_length, hop) = (%d, %d, %d) is neither (1024, 800, 160) nor (2048, 2048, 512)", n_fft,
              win, hop);
}

// one set of tables per device and size
int get_tables(const StftGeo& g, StftTables* t) {
  static TableCache<int, StftTables> cache;
  return cache.get(g.N, t, [&g](std::vector<float>* buf) {
    const int N = g.N, off = (N - g.win) / 2;
    const size_t win = buf->size();
    append_hann(g.win, N, off, false, buf);
    const size_t wsq = buf->size();
    append_hann(g.win, N, off, true, buf);
    const DftOffsets at = append_dft_tables(N, 1.0 / N, buf);
    // the vocoder's expected phase advance linspace(0, pi hop, bins)[k] = pi hop k / (N/2), modulo 2 pi: the angle is
    // 2 pi (hop k mod N) / N exactly
    const size_t phi = buf->size();
    for (int k = 0; k <= N / 2; ++k) {
      int64_t r = ((int64_t)g.hop * k) % N;
      if (r > N / 2) r -= N;
      buf->push_back((float)(2.0 * kPi * (double)r / (double)N));
    }
    return [=](const float* d) { return StftTables{d + win, d + wsq, dft_pointers(d, at), d + phi}; };
  });
}

template <int MODE>
int launch_frames(const StftGeo& g, const FrameArgs& a, int dtype, int B, hipStream_t s) {
  const dim3 grid((unsigned)a.Fpad, (unsigned)B), block(kStftThreads);
  if (g.N2 == 32) {
    if (dtype == MI355ASR_DT_I16) hipLaunchKernelGGL((frame_kernel<32, int16_t, MODE>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((frame_kernel<32, float, MODE>), grid, block, 0, s, a);
  } else {
    if (dtype == MI355ASR_DT_I16) hipLaunchKernelGGL((frame_kernel<64, int16_t, MODE>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((frame_kernel<64, float, MODE>), grid, block, 0, s, a);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_ola(const OlaArgs& a, int dtype, int B, hipStream_t s) {
  const dim3 grid((unsigned)((a.Opad + kOlaTile - 1) / kOlaTile), (unsigned)B), block(kOlaTile);
  if (dtype == MI355ASR_DT_I16) hipLaunchKernelGGL(ola_kernel<int16_t>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(ola_kernel<float>, grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

constexpr int kMaxFrames = 1 << 22;

int check_batch(const char* who, int32_t B, int64_t cols, const char* cols_name) {
  if (B < 1 || B > 65535) return fail(MI355ASR_EINVAL, "%s: need 1 <= B <= 65535 (got %d)", who, B);
  if (cols < 1 || cols > kMaxExtent32) return fail(MI355ASR_EINVAL, "%s: need 1 <= %s < 2^31 - 65536 (got %lld)", who, cols_name, (long long)cols);
  return 0;
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int mi355asr_stft_frames(int32_t n_fft, int32_t win_length, int32_t hop, int64_t n_samples, int32_t* frames) {
  StftGeo g;
  if (!frames) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = stft_geo(n_fft, win_length, hop, &g)) return rc;
  *frames = n_samples >= g.N / 2 + 1 && n_samples <= kMaxExtent32 ? 1 + (int32_t)(n_samples / g.hop) : 0;
  return 0;
}

int mi355asr_stft_ragged(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad, int32_t n_fft,
                         int32_t win_length, int32_t hop, float* S_dev, int32_t Fpad, int32_t* frames_dev, void* stream) {
  StftGeo g;
  if (!x_dev || !len_dev || !S_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (dtype != MI355ASR_DT_F32 && dtype != MI355ASR_DT_I16) return fail(MI355ASR_EINVAL, "stft: input dtype %d is neither float32 nor int16", dtype);
  if (int rc = stft_geo(n_fft, win_length, hop, &g)) return rc;
  if (int rc = check_batch("stft", B, Lpad, "Lpad")) return rc;
  if (Fpad < 1 || Fpad > kMaxFrames) return fail(MI355ASR_EINVAL, "stft: need 1 <= Fpad <= %d (got %d)", kMaxFrames, Fpad);
  FrameArgs a{};
  if (int rc = get_tables(g, &a.t)) return rc;
  a.x = x_dev; a.len = len_dev; a.Lpad = Lpad; a.S = S_dev; a.frames_out = frames_dev;
  a.Fpad = Fpad; a.win = g.win; a.hop = g.hop;
  return launch_frames<MODE_STFT>(g, a, dtype, B, (hipStream_t)stream);
}

int mi355asr_istft_workspace_bytes(int32_t B, int32_t Fpad, int32_t n_fft, int32_t win_length, int32_t hop, size_t* ws_bytes) {
  StftGeo g;
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = stft_geo(n_fft, win_length, hop, &g)) return rc;
  if (B < 1 || B > 65535 || Fpad < 1 || Fpad > kMaxFrames) return fail(MI355ASR_EINVAL, "istft: need 1 <= B <= 65535 and 1 <= Fpad <= %d (got %d, %d)", kMaxFrames, B, Fpad);
  *ws_bytes = round16((size_t)B * Fpad * g.win * sizeof(float));
  return 0;
}

int mi355asr_istft_ragged(const float* S_dev, const int32_t* frames_dev, int32_t B, int32_t Fpad, int32_t n_fft, int32_t win_length,
                          int32_t hop, const int32_t* out_len_dev, float* y_dev, int64_t Opad, void* ws_dev, size_t ws_bytes,
                          void* stream) {
  StftGeo g;
  size_t need = 0;
  if (!S_dev || !frames_dev || !y_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = mi355asr_istft_workspace_bytes(B, Fpad, n_fft, win_length, hop, &need)) return rc;
  if (int rc = stft_geo(n_fft, win_length, hop, &g)) return rc;
  if (int rc = check_batch("istft", B, Opad, "Opad")) return rc;
  if (ws_bytes < need) return fail(MI355ASR_EINVAL, "istft: the workspace has %zu bytes, %zu are needed", ws_bytes, need);
  if ((uintptr_t)ws_dev & 15) return fail(MI355ASR_EINVAL, "istft: the workspace must be 16-byte aligned");
  FrameArgs a{};
  if (int rc = get_tables(g, &a.t)) return rc;
  a.S = const_cast<float*>(S_dev); a.frames_in = frames_dev; a.fr = (float*)ws_dev;
  a.Fpad = Fpad; a.win = g.win; a.hop = g.hop;
  if (int rc = launch_frames<MODE_ISTFT>(g, a, MI355ASR_DT_F32, B, (hipStream_t)stream)) return rc;
  OlaArgs o{};
  o.fr = a.fr; o.wsq = a.t.wsq; o.frames = frames_dev; o.out_len = out_len_dev; o.y = y_dev; o.Opad = Opad;
  o.Fpad = Fpad; o.N = g.N; o.win = g.win; o.hop = g.hop;
  return launch_ola(o, MI355ASR_DT_F32, B, (hipStream_t)stream);
}

int mi355asr_spec_aug_workspace_bytes(int32_t B, int64_t Lpad, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = check_batch("spec_aug", B, Lpad, "Lpad")) return rc;
  *ws_bytes = round16((size_t)B * (size_t)(1 + Lpad / 160) * 800 * sizeof(float));
  return 0;
}

int mi355asr_spec_aug(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad, const int32_t* centres_dev,
                      int32_t Npad, const int32_t* counts_dev, int32_t window, float* y_dev, int64_t Opad, void* ws_dev,
                      size_t ws_bytes, void* stream) {
  StftGeo g;
  size_t need = 0;
  hipStream_t s = (hipStream_t)stream;
  if (!x_dev || !len_dev || !counts_dev || !y_dev || !ws_dev || (Npad > 0 && !centres_dev)) return fail(MI355ASR_EINVAL, "null pointer");
  if (dtype != MI355ASR_DT_F32 && dtype != MI355ASR_DT_I16) return fail(MI355ASR_EINVAL, "spec_aug: input dtype %d is neither float32 nor int16", dtype);
  if (window < 0) return fail(MI355ASR_EINVAL, "spec_aug: window = %d is negative", window);
  if (Npad < 0) return fail(MI355ASR_EINVAL, "spec_aug: Npad = %d is negative", Npad);
  if (int rc = mi355asr_spec_aug_workspace_bytes(B, Lpad, &need)) return rc;
  if (int rc = check_batch("spec_aug", B, Opad, "Opad")) return rc;
  if (ws_bytes < need) return fail(MI355ASR_EINVAL, "spec_aug: the workspace has %zu bytes, %zu are needed", ws_bytes, need);
  if ((uintptr_t)ws_dev & 15) return fail(MI355ASR_EINVAL, "spec_aug: the workspace must be 16-byte aligned");
  if (int rc = stft_geo(1024, 800, 160, &g)) return rc;
  // the counts are read back before anything is launched: random.sample of the reference cannot draw more than 513 bins
  std::vector<int32_t> counts((size_t)B);
  HIP_TRY(hipMemcpyAsync(counts.data(), counts_dev, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b)
    if (counts[b] < 0 || counts[b] > kSpecAugBins || counts[b] > Npad)
      return fail(MI355ASR_EINVAL, "spec_aug: row %d has %d centres (0 .. min(%d, Npad = %d))", b, counts[b], kSpecAugBins, Npad);
  FrameArgs a{};
  if (int rc = get_tables(g, &a.t)) return rc;
  a.x = x_dev; a.len = len_dev; a.Lpad = Lpad; a.centres = centres_dev; a.counts = counts_dev; a.fr = (float*)ws_dev;
  a.Fpad = (int)(1 + Lpad / g.hop); a.Npad = Npad; a.window = window; a.win = g.win; a.hop = g.hop;
  if (int rc = launch_frames<MODE_SPECAUG>(g, a, dtype, B, s)) return rc;
  OlaArgs o{};
  o.fr = a.fr; o.wsq = a.t.wsq; o.len = len_dev; o.x = x_dev; o.y = y_dev; o.Lpad = Lpad; o.Opad = Opad;
  o.Fpad = a.Fpad; o.N = g.N; o.win = g.win; o.hop = g.hop;
  return launch_ola(o, dtype, B, s);
}

int mi355asr_phase_vocoder_workspace_bytes(int32_t B, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535) return fail(MI355ASR_EINVAL, "phase_vocoder: need 1 <= B <= 65535 (got %d)", B);
  *ws_bytes = round16((size_t)B * sizeof(double)) + round16((size_t)B * sizeof(int32_t));
  return 0;
}

int mi355asr_phase_vocoder(const float* S_dev, const int32_t* frames_dev, int32_t B, int32_t Fpad, int32_t n_fft, int32_t win_length,
                           int32_t hop, const double* rates_host, const int32_t* out_frames_host, float* O_dev, int32_t Tpad,
                           void* ws_dev, size_t ws_bytes, void* stream) {
  StftGeo g;
  size_t need = 0;
  hipStream_t s = (hipStream_t)stream;
  if (!S_dev || !frames_dev || !rates_host || !out_frames_host || !O_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = stft_geo(n_fft, win_length, hop, &g)) return rc;
  if (int rc = mi355asr_phase_vocoder_workspace_bytes(B, &need)) return rc;
  if (Fpad < 1 || Fpad > kMaxFrames || Tpad < 1 || Tpad > kMaxFrames)
    return fail(MI355ASR_EINVAL, "phase_vocoder: need 1 <= Fpad, Tpad <= %d (got %d, %d)", kMaxFrames, Fpad, Tpad);
  if (ws_bytes < need) return fail(MI355ASR_EINVAL, "phase_vocoder: the workspace has %zu bytes, %zu are needed", ws_bytes, need);
  if ((uintptr_t)ws_dev & 15) return fail(MI355ASR_EINVAL, "phase_vocoder: the workspace must be 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    if (!(rates_host[b] > 0.0) || !(rates_host[b] <= 1e6)) return fail(MI355ASR_EINVAL, "phase_vocoder: row %d has rate %g (must be in (0, 1e6])", b, rates_host[b]);
    if (out_frames_host[b] < 0 || out_frames_host[b] > Tpad) return fail(MI355ASR_EINVAL, "phase_vocoder: row %d has %d output frames (0 .. Tpad = %d)", b, out_frames_host[b], Tpad);
  }
  VocoderArgs a{};
  StftTables t;
  if (int rc = get_tables(g, &t)) return rc;
  double* rates = (double*)ws_dev;
  int32_t* tc = (int32_t*)((char*)ws_dev + round16((size_t)B * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(rates, rates_host, (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(tc, out_frames_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  a.S = S_dev; a.O = O_dev; a.frames = frames_dev; a.rates = rates; a.tcount = tc; a.phi = t.phi;
  a.Fpad = Fpad; a.Tpad = Tpad; a.bins = g.N / 2 + 1;
  hipLaunchKernelGGL(vocoder_kernel, dim3((unsigned)((a.bins + kStftThreads - 1) / kStftThreads), (unsigned)B), dim3(kStftThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
