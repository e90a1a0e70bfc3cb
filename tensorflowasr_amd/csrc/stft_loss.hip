// The VAD trainer's losses: the multi-resolution STFT loss of vad/utils/stft.py (TFMultiResolutionSTFT) with its gradient with
// respect to the predicted waveform, and the sums behind VADTrainer.mask_loss / binary_accuracy / F1: behind
// mi355asr_stft_loss_workspace_bytes, mi355asr_stft_loss and mi355asr_vad_mask_stats of include/mi355asr.h.
//
// tf.signal.stft semantics: frame f of a row holds the samples f step .. f step + frame_length - 1 (no centring, no padding of
// the row), times a periodic Hann window of frame_length, zero-padded at the END to fft_length; a row of L samples has
// F = 1 + (L - frame_length) / step frames, 0 when L < frame_length.
//
// loss_frame_kernel<N2, GRAD>: one workgroup (four waves) per frame of one row.  The predicted and the true frame go through the
// two-stage DFT of stft.hip together, N = 32 x N2 with N2 = 16 (512), 32 (1024) or 64 (2048), as the columns [pred | truth] of
// one B operand on v_mfma_f32_16x16x4_f32 (exact fp32 products, tables computed in float64 and packed in fragment order):
//     A[k1][n2] = sum_n1 W32^(n1 k1) xw[N2 n1 + n2]              stage 1: [64 (re | im of k1)] x [32] times [32] x [2 N2]
//     B[k1][n2] = A[k1][n2] W_N^(n2 k1)                          twiddle, written transposed
//     X[k1 + 32 k2] = sum_n2 W_N2^(n2 k2) B[k1][n2], k2 < N2/2   stage 2: [N2 (re | im of k2)] x [2 N2] times [2 N2] x [64]
//     X[N/2] = sum_n (-1)^n xw[n]                                a wave reduction in a fixed order
//   From the two spectra in LDS every bin forms, in float64, p = sqrt(|P|^2 + 1e-7) + 1e-6 and t likewise.
//   GRAD = false: the frame's three sums  sum (p - t)^2, sum p^2, sum (log p - log t)^2  (float64, fixed order) go to the
//     workspace; the spectra never leave the chip.
//   GRAD = true (after loss_reduce_kernel has formed the row's norms): the spectra are recomputed, dL/dp is formed per bin,
//     multiplied by P / sqrt(|P|^2 + 1e-7), and the transpose of the real DFT is applied as the inverse stages of stft.hip on the
//     Hermitian extension (G[k] / 2 at k and its conjugate at N - k; the tables carry no 1 / N):
//     A[p][k2] = sum_k1 conj W32^(p k1) F[N2 k1 + k2];  B = A conj W_N^(k2 p);  y[p + 32 q] = Re sum_k2 conj W_N2^(k2 q) B[p][k2]
//     The first frame_length samples times the window go to the workspace.
// loss_reduce_kernel: one wave per (row, resolution): lane l adds the frames l, l + 64, ... in ascending order, the 64 lanes are
//   added by a fixed butterfly, all in float64 -> sc, mag, frames and the row's norms for the gradient.
// loss_ola_kernel: owner computes.  The thread of sample n adds the frames that cover it, resolution 0 first, ascending frames
//   within a resolution, and writes every element of the gradient (0 where nothing reaches).
// mask_stats_kernel: one workgroup; float64 / int64 sums in a fixed order, then (on request) the gradient from the totals.
// A row is computed from its own samples alone and nothing depends on timing (no atomics): a row of a ragged batch equals the
// row alone bit for bit.
#include "common.h"
#include "dft_mfma.h"
#include "model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLossOlaTile = 256;                        // outputs per workgroup of loss_ola_kernel
constexpr int kLDT1 = 48;                                // row stride of the transposed matrix, one signal
constexpr int kLDT2 = 72;                                // two signals side by side
constexpr int kMaxRes = 4;

struct LossTables {
  const float* win;       // [N] periodic Hann of frame_length, zero from frame_length on
  DftTables dft;          // twiddles and packed stage matrices; the last two are the transpose: T4 carries no 1 / N
};

struct LossFrameArgs {
  LossTables t;
  const float* truth;     // row b at truth + b ld_t
  const float* pred;
  int64_t ld_t, ld_p;
  const int32_t* len;     // [B] or null (Lpad)
  int64_t Lpad;
  double* part;           // [B, Fpad, 3] the frame's sums
  const double* norms;    // [B, R, 2] D = ||p - t||, Np = ||p||            (GRAD)
  const float* w_sc;      // [B, R]                                          (GRAD)
  const float* w_mag;     // [B, R]
  float* fr;              // [B, Fpad, fl] windowed gradient frames          (GRAD)
  int Fpad, fl, step, r, R;
};

DEV int64_t row_len(const int32_t* len, int b, int64_t Lpad) {
  if (!len) return Lpad;
  const int64_t L = len[b];
  return L < 0 ? 0 : (L > Lpad ? Lpad : L);
}
DEV int loss_frames(int64_t L, int fl, int step) { return L >= fl ? 1 + (int)((L - fl) / step) : 0; }

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int N2, bool GRAD>
__global__ __launch_bounds__(kThreads) void loss_frame_kernel(LossFrameArgs a) {
  constexpr int N = 32 * N2, LDX2 = 2 * N2 + 8, LDX1 = N2 + 8, BINS = N / 2 + 1;
  // bufU: the two windowed frames [32][pred N2 | truth N2], then the twiddled transposed matrix [2 N2][pred 32 | truth 32], then
  //       (GRAD) the Hermitian gradient spectrum [(re | im) k1][k2] and its twiddled transposed matrix
  // bufD: stage-1 output [64][2 N2], then the two half spectra [(re | im) k2][pred 32 | truth 32], then (GRAD) the inverse stages
  constexpr int U = cmax(cmax(32 * LDX2, 2 * N2 * kLDT2), GRAD ? 64 * LDX1 : 0);
  __shared__ __attribute__((aligned(16))) float bufU[U];
  __shared__ __attribute__((aligned(16))) float bufD[64 * LDX2];
  __shared__ float red[8];                                            // wave partials of the two Nyquist bins
  __shared__ double redd[12];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, f = blockIdx.x;
  const int64_t L = row_len(a.len, b, a.Lpad);
  const int F = loss_frames(L, a.fl, a.step);
  if (f >= F) return;                                                 // uniform over the workgroup

  // ---- the two windowed frames: samples f step + n, n < frame_length; zero from there to N
  {
    const float* xp = a.pred + (size_t)b * a.ld_p + (size_t)f * a.step;
    const float* xt = a.truth + (size_t)b * a.ld_t + (size_t)f * a.step;
    float np = 0.0f, nt = 0.0f;
    for (int n = tid; n < N; n += kThreads) {
      float vp = 0.0f, vt = 0.0f;
      if (n < a.fl) {
        const float w = a.t.win[n];
        vp = xp[n] * w;
        vt = xt[n] * w;
      }
      const int o = (n / N2) * LDX2 + (n % N2);
      bufU[o] = vp;
      bufU[o + N2] = vt;
      np += vp;                                                       // n and tid have the same parity: the sign comes below
      nt += vt;
    }
    if (tid & 1) {
      np = -np;
      nt = -nt;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      np += __shfl_xor(np, off);
      nt += __shfl_xor(nt, off);
    }
    if ((tid & 63) == 0) {
      red[tid >> 6] = np;
      red[4 + (tid >> 6)] = nt;
    }
  }
  __syncthreads();
  // ---- forward stage 1: bufD[(re | im) k1][pred n2 | truth n2]
  dft_block_gemm<kThreads, 4, 2 * N2 / 16, 8>(a.t.dft.T1, bufU, LDX2, [&](int r, int col, float v) { bufD[r * LDX2 + col] = v; });
  __syncthreads();
  // ---- twiddle, transposed: bufU[(re | im) n2][pred k1 | truth k1]
  for (int i = tid; i < 2 * 32 * N2; i += kThreads) {
    const int sig = i / (32 * N2), j = i - sig * (32 * N2);
    const int k1 = j / N2, n2 = j - k1 * N2;
    const float are = bufD[k1 * LDX2 + sig * N2 + n2], aim = bufD[(32 + k1) * LDX2 + sig * N2 + n2];
    const float tc = a.t.dft.twc[j], ts = a.t.dft.tws[j];
    bufU[n2 * kLDT2 + 32 * sig + k1] = fmaf(are, tc, __fmul_rn(aim, ts));
    bufU[(N2 + n2) * kLDT2 + 32 * sig + k1] = fmaf(aim, tc, -__fmul_rn(are, ts));
  }
  const float nyq_p = (red[0] + red[1]) + (red[2] + red[3]);
  const float nyq_t = (red[4] + red[5]) + (red[6] + red[7]);
  __syncthreads();
  // ---- forward stage 2: row r < N2/2 is Re X[32 r + col], row N2/2 + r is Im X[32 r + col]; columns 32 .. 63 are the truth
  dft_block_gemm<kThreads, N2 / 16, 4, N2 / 2>(a.t.dft.T2, bufU, kLDT2, [&](int r, int col, float v) { bufD[r * 64 + col] = v; });
  __syncthreads();

  double cA = 0.0, cB = 0.0, cM = 0.0;
  if constexpr (GRAD) {
    const double D = a.norms[((size_t)b * a.R + a.r) * 2], Np = a.norms[((size_t)b * a.R + a.r) * 2 + 1];
    const double wsc = (double)a.w_sc[(size_t)b * a.R + a.r], wmag = (double)a.w_mag[(size_t)b * a.R + a.r];
    if (D > 0.0) {                                                    // D == 0: the spectral-convergence term contributes 0
      cA = wsc / (D * (Np + 1e-6));
      cB = wsc * D / (Np * (Np + 1e-6) * (Np + 1e-6));
    }
    cM = wmag * 2.0 / ((double)F * (double)BINS);
  }
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = tid; k < BINS; k += kThreads) {
    float pre, pim, tre, tim;
    if (k < N / 2) {
      const int o = (k >> 5) * 64 + (k & 31);
      pre = bufD[o]; pim = bufD[(N2 / 2) * 64 + o]; tre = bufD[o + 32]; tim = bufD[(N2 / 2) * 64 + o + 32];
    } else {
      pre = nyq_p; pim = 0.0f; tre = nyq_t; tim = 0.0f;
    }
    const double ps = sqrt((double)pre * pre + (double)pim * pim + 1e-7), p = ps + 1e-6;
    const double t = sqrt((double)tre * tre + (double)tim * tim + 1e-7) + 1e-6;
    const double d = log(p / t);
    if constexpr (!GRAD) {
      s1 += (p - t) * (p - t);
      s2 += p * p;
      s3 += d * d;
    } else {
      const double g = (cA * (p - t) - cB * p + cM * d / p) / ps;
      const bool edge = k == 0 || k == N / 2;                         // Im X is identically 0 there
      const float gre = (float)(edge ? g * pre : 0.5 * g * pre), gim = (float)(edge ? 0.0 : 0.5 * g * pim);
      const int o = (k / N2) * LDX1 + (k % N2);
      bufU[o] = gre;
      bufU[32 * LDX1 + o] = gim;
      if (!edge) {
        const int k2 = N - k, o2 = (k2 / N2) * LDX1 + (k2 % N2);
        bufU[o2] = gre;
        bufU[32 * LDX1 + o2] = -gim;
      }
    }
  }

  if constexpr (!GRAD) {
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if ((tid & 63) == 0) {
      redd[3 * (tid >> 6)] = s1;
      redd[3 * (tid >> 6) + 1] = s2;
      redd[3 * (tid >> 6) + 2] = s3;
    }
    __syncthreads();
    if (tid < 3) a.part[((size_t)b * a.Fpad + f) * 3 + tid] = (redd[tid] + redd[3 + tid]) + (redd[6 + tid] + redd[9 + tid]);
  } else {
    __syncthreads();
    // ---- transposed stage 1: bufD[(re | im) p][k2]
    dft_block_gemm<kThreads, 4, N2 / 16, 16>(a.t.dft.T3, bufU, LDX1, [&](int r, int col, float v) { bufD[r * LDX1 + col] = v; });
    __syncthreads();
    for (int i = tid; i < 32 * N2; i += kThreads) {
      const int p = i / N2, k2 = i - p * N2;
      const float are = bufD[p * LDX1 + k2], aim = bufD[(32 + p) * LDX1 + k2];
      const float tc = a.t.dft.twc[i], ts = a.t.dft.tws[i];
      bufU[k2 * kLDT1 + p] = fmaf(are, tc, -__fmul_rn(aim, ts));
      bufU[(N2 + k2) * kLDT1 + p] = fmaf(are, ts, __fmul_rn(aim, tc));
    }
    __syncthreads();
    // ---- transposed stage 2: bufD[32 q + p] = dL / d xw[n]
    dft_block_gemm<kThreads, N2 / 16, 2, N2 / 2>(a.t.dft.T4, bufU, kLDT1, [&](int r, int col, float v) { bufD[r * 32 + col] = v; });
    __syncthreads();
    float* out = a.fr + ((size_t)b * a.Fpad + f) * a.fl;
    for (int j = tid; j < a.fl; j += kThreads) out[j] = bufD[j] * a.t.win[j];
  }
}

struct LossRes {
  int fl, step, bins, Fpad;
  size_t part_off;        // doubles from the start of the workspace
  size_t fr_off;          // floats from the start of the frame area
};

struct LossReduceArgs {
  LossRes res[kMaxRes];
  const double* ws;
  const int32_t* len;
  int64_t Lpad;
  float* sc;              // [B, R]
  float* mag;             // [B, R]
  int32_t* frames;        // [B, R]
  double* norms;          // [B, R, 2]
  int R;
};

__global__ __launch_bounds__(64) void loss_reduce_kernel(LossReduceArgs a) {
  const int r = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const LossRes q = a.res[r];
  const int F = loss_frames(row_len(a.len, b, a.Lpad), q.fl, q.step);
  const double* part = a.ws + q.part_off + (size_t)b * q.Fpad * 3;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int f = lane; f < F; f += 64) {
    s1 += part[3 * (size_t)f];
    s2 += part[3 * (size_t)f + 1];
    s3 += part[3 * (size_t)f + 2];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  if (lane == 0) {
    const double D = sqrt(s1), Np = sqrt(s2);
    const size_t o = (size_t)b * a.R + r;
    a.sc[o] = F > 0 ? (float)(D / (Np + 1e-6)) : 0.0f;
    a.mag[o] = F > 0 ? (float)(s3 / ((double)F * (double)q.bins)) : __builtin_nanf("");
    a.frames[o] = F;
    a.norms[2 * o] = D;
    a.norms[2 * o + 1] = Np;
  }
}

struct LossOlaArgs {
  LossRes res[kMaxRes];
  const float* fr;
  const int32_t* len;
  int64_t Lpad, ld_g;
  float* grad;            // row b at grad + b ld_g, Lpad elements
  int R;
};

__global__ __launch_bounds__(kLossOlaTile) void loss_ola_kernel(LossOlaArgs a) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * kLossOlaTile + threadIdx.x;
  if (n >= a.Lpad) return;
  const int64_t L = row_len(a.len, b, a.Lpad);
  float acc = 0.0f;
  if (n < L) {
    for (int r = 0; r < a.R; ++r) {
      const LossRes q = a.res[r];
      const int F = loss_frames(L, q.fl, q.step);
      const int64_t lo = n - q.fl + 1;
      const int64_t f0 = lo > 0 ? (lo + q.step - 1) / q.step : 0;
      int64_t f1 = n / q.step;
      if (f1 > F - 1) f1 = F - 1;
      const float* fr = a.fr + q.fr_off + (size_t)b * q.Fpad * q.fl;
      for (int64_t f = f0; f <= f1; ++f) acc += fr[(size_t)f * q.fl + (size_t)(n - f * q.step)];
    }
  }
  a.grad[(size_t)b * a.ld_g + n] = acc;
}

struct MaskStatsArgs {
  const float* labels;    // (b, t) at labels + b ld_lab + t
  const float* logits;
  const int32_t* counts;  // [B] or null (T)
  int64_t ld_lab, ld_x, ld_g;
  double* sums;           // [4] sum loss one, sum one, sum loss zero, sum zero
  long long* cnt;         // [4] TP, FP, FN, TN
  float* grad;            // or null
  float thr;
  int B, T;
};

__global__ __launch_bounds__(kThreads) void mask_stats_kernel(MaskStatsArgs a) {
  __shared__ double sd[4][4];
  __shared__ long long sc[4][4];
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)a.B * a.T;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long long c[4] = {0, 0, 0, 0};
  for (int64_t i = tid; i < total; i += kThreads) {
    const int b = (int)(i / a.T), t = (int)(i - (int64_t)b * a.T);
    int cn = a.counts ? a.counts[b] : a.T;
    cn = cn < 0 ? 0 : (cn > a.T ? a.T : cn);
    if (t >= cn) continue;
    const float xf = a.logits[(size_t)b * a.ld_x + t], z = a.labels[(size_t)b * a.ld_lab + t];
    const double x = (double)xf;
    const double l = (x > 0.0 ? x : 0.0) - x * (double)z + log1p(exp(-fabs(x)));
    const bool one = z == 1.0f, zero = z == 0.0f, pos = xf > a.thr;
    if (one) { s[0] += l; s[1] += 1.0; }
    if (zero) { s[2] += l; s[3] += 1.0; }
    c[0] += one && pos;
    c[1] += zero && pos;
    c[2] += one && !pos;
    c[3] += zero && !pos;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s[i] = wave_sum(s[i]);
    c[i] = wave_sum(c[i]);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sd[tid >> 6][i] = s[i];
      sc[tid >> 6][i] = c[i];
    }
  }
  __syncthreads();
  if (tid < 4) {
    a.sums[tid] = (sd[0][tid] + sd[1][tid]) + (sd[2][tid] + sd[3][tid]);
    a.cnt[tid] = (sc[0][tid] + sc[1][tid]) + (sc[2][tid] + sc[3][tid]);
  }
  if (!a.grad) return;
  const double w1 = 1.0 / (((sd[0][1] + sd[1][1]) + (sd[2][1] + sd[3][1])) + 1e-6);
  const double w0 = 1.0 / (((sd[0][3] + sd[1][3]) + (sd[2][3] + sd[3][3])) + 1e-6);
  for (int64_t i = tid; i < total; i += kThreads) {
    const int b = (int)(i / a.T), t = (int)(i - (int64_t)b * a.T);
    int cn = a.counts ? a.counts[b] : a.T;
    cn = cn < 0 ? 0 : (cn > a.T ? a.T : cn);
    float g = 0.0f;
    if (t < cn) {
      const double x = (double)a.logits[(size_t)b * a.ld_x + t];
      const float z = a.labels[(size_t)b * a.ld_lab + t];
      const double e = exp(-fabs(x));
      const double sig = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
      const double w = z == 1.0f ? w1 : (z == 0.0f ? w0 : 0.0);
      g = (float)((sig - (double)z) * w);
    }
    a.grad[(size_t)b * a.ld_g + t] = g;
  }
}

// ---- host: sizes, tables ------------------------------------------------------------------------------------------------------------
// one set of tables per device, fft_length and frame_length
int get_tables(int N, int fl, LossTables* t) {
  static TableCache<std::pair<int, int>, LossTables> cache;
  return cache.get({N, fl}, t, [N, fl](std::vector<float>* buf) {
    const size_t win = buf->size();
    append_hann(fl, N, 0, false, buf);
    const DftOffsets at = append_dft_tables(N, 1.0, buf);
    return [=](const float* d) { return LossTables{d + win, dft_pointers(d, at)}; };
  });
}

template <bool GRAD>
int launch_loss_frames(int N, const LossFrameArgs& a, int B, hipStream_t s) {
  const dim3 grid((unsigned)a.Fpad, (unsigned)B), block(kThreads);
  if (N == 512) hipLaunchKernelGGL((loss_frame_kernel<16, GRAD>), grid, block, 0, s, a);
  else if (N == 1024) hipLaunchKernelGGL((loss_frame_kernel<32, GRAD>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((loss_frame_kernel<64, GRAD>), grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

struct LossPlan {
  LossRes res[kMaxRes];
  size_t norms_off;       // bytes
  size_t fr_bytes_off;    // bytes: start of the frame area
  size_t total;
};

int loss_plan(int32_t B, int64_t Lpad, int32_t R, const int32_t* fft, const int32_t* fl, const int32_t* step, bool want_grad,
              LossPlan* p) {
  if (!fft || !fl || !step) return fail(MI355ASR_EINVAL, "stft_loss: null pointer in the resolution arrays");
  if (R < 1 || R > kMaxRes) return fail(MI355ASR_EINVAL, "stft_loss: need 1 <= resolutions <= %d (got %d)", kMaxRes, R);
  if (B < 1 || B > 65535) return fail(MI355ASR_EINVAL, "stft_loss: need 1 <= B <= 65535 (got %d)", B);
  if (Lpad < 1 || Lpad > kMaxExtent32) return fail(MI355ASR_EINVAL, "stft_loss: need 1 <= Lpad < 2^31 - 65536 (got %lld)", (long long)Lpad);
  size_t o = 0;
  for (int r = 0; r < R; ++r) {
    if (fft[r] != 512 && fft[r] != 1024 && fft[r] != 2048)
      return fail(MI355ASR_EINVAL, "stft_loss: fft_length[%d] = %d is not 512, 1024 or 2048", r, fft[r]);
    if (fl[r] < 1 || fl[r] > fft[r])
      return fail(MI355ASR_EINVAL, "stft_loss: need 1 <= frame_length[%d] <= fft_length (got %d, %d)", r, fl[r], fft[r]);
    if (step[r] < 1 || step[r] > fl[r])
      return fail(MI355ASR_EINVAL, "stft_loss: need 1 <= frame_step[%d] <= frame_length (got %d, %d)", r, step[r], fl[r]);
    LossRes& q = p->res[r];
    q.fl = fl[r]; q.step = step[r]; q.bins = fft[r] / 2 + 1;
    q.Fpad = Lpad >= fl[r] ? 1 + (int)((Lpad - fl[r]) / step[r]) : 0;
    q.part_off = o / sizeof(double);
    o += align256((size_t)B * q.Fpad * 3 * sizeof(double));
  }
  p->norms_off = o;
  o += align256((size_t)B * R * 2 * sizeof(double));
  p->fr_bytes_off = o;
  size_t fo = 0;
  for (int r = 0; r < R; ++r) {
    p->res[r].fr_off = fo / sizeof(float);
    if (want_grad) fo += align256((size_t)B * p->res[r].Fpad * p->res[r].fl * sizeof(float));
  }
  p->total = o + fo;
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_stft_loss_workspace_bytes(int32_t B, int64_t Lpad, int32_t R, const int32_t* fft_lengths, const int32_t* frame_lengths,
                                       const int32_t* frame_steps, int32_t want_grad, size_t* bytes) {
  LossPlan p{};
  if (!bytes) return fail(MI355ASR_EINVAL, "stft_loss: null pointer bytes");
  if (int rc = loss_plan(B, Lpad, R, fft_lengths, frame_lengths, frame_steps, want_grad != 0, &p)) return rc;
  *bytes = p.total;
  return 0;
}

int mi355asr_stft_loss(const float* truth_dev, int64_t ld_truth, const float* pred_dev, int64_t ld_pred, const int32_t* len_dev,
                       int32_t B, int64_t Lpad, int32_t R, const int32_t* fft_lengths, const int32_t* frame_lengths,
                       const int32_t* frame_steps, float* sc_dev, float* mag_dev, int32_t* frames_dev, const float* w_sc_dev,
                       const float* w_mag_dev, float* grad_dev, int64_t ld_grad, void* ws_dev, size_t ws_bytes, void* stream) {
  LossPlan p{};
  hipStream_t s = (hipStream_t)stream;
  if (!truth_dev) return fail(MI355ASR_EINVAL, "stft_loss: null pointer truth_dev");
  if (!pred_dev) return fail(MI355ASR_EINVAL, "stft_loss: null pointer pred_dev");
  if (!sc_dev || !mag_dev || !frames_dev) return fail(MI355ASR_EINVAL, "stft_loss: null output pointer (sc_dev, mag_dev, frames_dev)");
  if (!ws_dev) return fail(MI355ASR_EINVAL, "stft_loss: null pointer ws_dev");
  if (grad_dev && (!w_sc_dev || !w_mag_dev)) return fail(MI355ASR_EINVAL, "stft_loss: grad_dev needs w_sc_dev and w_mag_dev");
  if (int rc = loss_plan(B, Lpad, R, fft_lengths, frame_lengths, frame_steps, grad_dev != nullptr, &p)) return rc;
  if (ld_truth < 0 || ld_pred < 0 || (B > 1 && (ld_truth < Lpad || ld_pred < Lpad)))
    return fail(MI355ASR_EINVAL, "stft_loss: the row strides ld_truth=%lld, ld_pred=%lld are smaller than Lpad=%lld", (long long)ld_truth,
                (long long)ld_pred, (long long)Lpad);
  if (grad_dev && B > 1 && ld_grad < Lpad)
    return fail(MI355ASR_EINVAL, "stft_loss: ld_grad=%lld lets the gradient rows overlap (Lpad=%lld)", (long long)ld_grad, (long long)Lpad);
  if ((uintptr_t)ws_dev & 15) return fail(MI355ASR_EINVAL, "stft_loss: the workspace must be 16-byte aligned");
  if (ws_bytes < p.total) return fail(MI355ASR_EWORKSPACE, "stft_loss: the workspace has %zu bytes, %zu are needed", ws_bytes, p.total);
  LossTables tabs[kMaxRes];
  for (int r = 0; r < R; ++r)
    if (int rc = get_tables(fft_lengths[r], frame_lengths[r], &tabs[r])) return rc;
  char* w = (char*)ws_dev;
  double* norms = (double*)(w + p.norms_off);
  float* frames_area = (float*)(w + p.fr_bytes_off);
  for (int pass = 0; pass < (grad_dev ? 2 : 1); ++pass) {
    for (int r = 0; r < R; ++r) {
      if (p.res[r].Fpad < 1) continue;
      LossFrameArgs a{};
      a.t = tabs[r]; a.truth = truth_dev; a.pred = pred_dev; a.ld_t = ld_truth; a.ld_p = ld_pred; a.len = len_dev; a.Lpad = Lpad;
      a.part = (double*)ws_dev + p.res[r].part_off; a.norms = norms; a.w_sc = w_sc_dev; a.w_mag = w_mag_dev;
      a.fr = frames_area + p.res[r].fr_off; a.Fpad = p.res[r].Fpad; a.fl = p.res[r].fl; a.step = p.res[r].step; a.r = r; a.R = R;
      if (int rc = pass == 0 ? launch_loss_frames<false>(fft_lengths[r], a, B, s) : launch_loss_frames<true>(fft_lengths[r], a, B, s))
        return rc;
    }
    if (pass == 0) {
      LossReduceArgs q{};
      for (int r = 0; r < R; ++r) q.res[r] = p.res[r];
      q.ws = (const double*)ws_dev; q.len = len_dev; q.Lpad = Lpad; q.sc = sc_dev; q.mag = mag_dev; q.frames = frames_dev;
      q.norms = norms; q.R = R;
      hipLaunchKernelGGL(loss_reduce_kernel, dim3((unsigned)R, (unsigned)B), dim3(64), 0, s, q);
      HIP_TRY(hipGetLastError());
    } else {
      LossOlaArgs o{};
      for (int r = 0; r < R; ++r) o.res[r] = p.res[r];
      o.fr = frames_area; o.len = len_dev; o.Lpad = Lpad; o.ld_g = ld_grad; o.grad = grad_dev; o.R = R;
      hipLaunchKernelGGL(loss_ola_kernel, dim3((unsigned)((Lpad + kLossOlaTile - 1) / kLossOlaTile), (unsigned)B), dim3(kLossOlaTile), 0,
                         s, o);
      HIP_TRY(hipGetLastError());
    }
  }
  return 0;
}

int mi355asr_vad_mask_stats(const float* labels_dev, int64_t ld_lab, const float* logits_dev, int64_t ld_x, const int32_t* counts_dev,
                            int32_t B, int32_t T, float threshold, double* sums_dev, int64_t* counts_out_dev, float* grad_dev,
                            int64_t ld_grad, void* stream) {
  if (!labels_dev) return fail(MI355ASR_EINVAL, "vad_mask_stats: null pointer labels_dev");
  if (!logits_dev) return fail(MI355ASR_EINVAL, "vad_mask_stats: null pointer logits_dev");
  if (!sums_dev || !counts_out_dev) return fail(MI355ASR_EINVAL, "vad_mask_stats: null output pointer (sums_dev, counts_out_dev)");
  if (B < 1 || T < 1 || (int64_t)B * T > kMaxExtent32) return fail(MI355ASR_EINVAL, "vad_mask_stats: need B, T >= 1 and B * T < 2^31 - 65536 (got %d, %d)", B, T);
  if (ld_lab < 0 || ld_x < 0 || (B > 1 && (ld_lab < T || ld_x < T)))
    return fail(MI355ASR_EINVAL, "vad_mask_stats: the row strides ld_lab=%lld, ld_x=%lld are smaller than T=%d", (long long)ld_lab, (long long)ld_x, T);
  if (grad_dev && B > 1 && ld_grad < T) return fail(MI355ASR_EINVAL, "vad_mask_stats: ld_grad=%lld lets the gradient rows overlap", (long long)ld_grad);
  if (!(threshold == threshold)) return fail(MI355ASR_EINVAL, "vad_mask_stats: the threshold is NaN");
  if (((uintptr_t)sums_dev & 7) || ((uintptr_t)counts_out_dev & 7)) return fail(MI355ASR_EINVAL, "vad_mask_stats: sums_dev and counts_out_dev must be 8-byte aligned");
  MaskStatsArgs a{};
  a.labels = labels_dev; a.logits = logits_dev; a.counts = counts_dev; a.ld_lab = ld_lab; a.ld_x = ld_x; a.ld_g = ld_grad;
  a.sums = sums_dev; a.cnt = (long long*)counts_out_dev; a.grad = grad_dev; a.thr = threshold; a.B = B; a.T = T;
  hipLaunchKernelGGL(mask_stats_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
