// Far-field simulation (the reference's augmentations/augments.py: SignalRIR, SignalNoise and Augmentation.process's clip and
// 16-bit quantisation) behind mi355asr_rir_generate, mi355asr_fir_ragged and mi355asr_mix_snr of include/mi355asr.h.
//
// fir_ragged_kernel: y[n] = sum_k h[k] x[n - k], the full convolution of every row of a ragged batch with its own filter, as the
// product of a sample matrix with 16 x 16 Toeplitz blocks on v_mfma_f32_16x16x4_f32 (an exact fp32 FMA chain).  With
// X[i][c] = x[16 i + c] and T_m[c][j] = h[16 m + j - c], Y[i][:] = sum_m X[i - m][:] T_m and y[16 i + j] = Y[i][j]: every block is
// dense, so the matrix pipe does 2 L K useful FLOP per row and nothing else.  A workgroup owns 4096 consecutive outputs, a wave
// 1024 of them as FOUR accumulator tiles whose rows interleave (tile t, row r is i = i0 + t + 4 r): the A fragment of (tile t,
// block m) holds the samples of rows i - m, so it is the fragment of (tile t + 1, block m + 1) -- one new 16-byte LDS read of
// samples and four dword reads of taps feed sixteen MFMAs.  The k index of a block is permuted (lane group g, sub-step s <-> c =
// 4 g + s) so that the four sub-steps of a lane are four consecutive samples.  Samples lie in LDS with four floats of padding per
// 64 (rows of a fragment are 64 samples apart: the padding spreads them over the banks); the filter is staged 256 blocks (4096
// taps) at a time.  Samples outside [0, in_len) and taps outside [0, K) are staged as zeros and never read from memory.
// An output is ONE chain over m ascending, sub-steps ascending, zero terms included, whatever the batch around it: a row of a
// ragged batch equals the row alone bit for bit.
//
// rir_kernel: the image-source method (Habets' rir_generator, omnidirectional microphone, 3-D, unlimited order), owner computes.
// A workgroup owns 256 consecutive samples of one response.  Round by round its threads each take one (mx, my, mz, q) and test
// that image's four (j, k) variants: distance in float64, kept when its window [fdist - Tw/2 + 1, fdist + Tw/2] meets the segment.
// The kept images go into an LDS list in image order (a prefix sum over the threads' counts: the order does not depend on timing),
// each with what depends on the image alone -- fdist, the gain (float64 product of the reflection coefficients over 4 pi d,
// rounded once), the fractional delay f and sin / cos of pi f / 2 and 2 pi f / Tw.  Then thread n adds, in list order and in
// float64, the contribution of every listed image whose window covers n.  With kk = n - fdist an integer, the window and the sinc
// need no trigonometry per sample: sin(pi (kk - f) / 2) is +-sin(pi f / 2) or +-cos(pi f / 2) by kk mod 4, and
// cos(2 pi (kk - f) / Tw) comes from a Tw-entry table of cos / sin(2 pi kk / Tw) by the angle-difference formula.  No atomics:
// the result is the same bits in every run and in every batch.
// rir_highpass_kernel: the generator's 100 Hz high-pass recurrence, float64, one lane per response over samples staged in LDS.
//
// mix_snr_kernel: one workgroup per row; both powers in float64 by a fixed tree, g rounded to fp32 once, y = fma(g, d, x).
#include "common.h"
#include "model.h"

namespace {

// ---- ragged FIR -------------------------------------------------------------------------------------------------------------------
constexpr int kFirThreads = 256;
constexpr int kFirTile = 4096;                          // outputs per workgroup: 4 waves x 4 tiles x 16 rows x 16 columns
constexpr int kFirMC = 256;                             // Toeplitz blocks (16 taps each) per staged piece of the filter
constexpr int kFirMaxK = 16384;
constexpr int kFirSpan = 16 * (kFirMC + kFirTile / 16); // samples a piece's blocks touch: 8192
constexpr int kFirXs = kFirSpan + 4 * (kFirSpan / 64);  // with 4 floats of padding per 64
constexpr int kFirHs = 16 * kFirMC + 32;                // taps 16 (first block) - 16 .. 16 (last block + 1) + 15

struct FirArgs {
  const void* x;          // [B, Lpad] float or int16
  const int32_t* in_len;  // [B]
  const float* h;         // [B, Kpad] ([1, Kpad]: h_stride = 0)
  float* y;               // [B, Opad]
  int64_t Lpad, h_stride, Opad;
  int K, vec_x;           // vec_x: rows of x start on 16-byte boundaries
};

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }

template <typename T>
__global__ __launch_bounds__(kFirThreads) void fir_ragged_kernel(FirArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kFirXs];
  __shared__ __attribute__((aligned(16))) float hs[kFirHs];
  const int b = blockIdx.y;
  const int64_t L = a.in_len[b] > 0 ? ((int64_t)a.in_len[b] < a.Lpad ? (int64_t)a.in_len[b] : a.Lpad) : 0;
  const int64_t out_len = L > 0 ? L + a.K - 1 : 0;
  const int64_t N0 = (int64_t)blockIdx.x * kFirTile;
  float* yrow = a.y + (int64_t)b * a.Opad;
  if (N0 >= out_len) {                                  // nothing of the row here: zeros
    for (int i = threadIdx.x; i < kFirTile; i += kFirThreads)
      if (N0 + i < a.Opad) yrow[N0 + i] = 0.0f;
    return;
  }
  const T* x = reinterpret_cast<const T*>(a.x) + (int64_t)b * a.Lpad;
  const float* h = a.h + (int64_t)b * a.h_stride;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const bool active = N0 + 1024 * w < out_len;          // wave-uniform: this wave has outputs of the row
  const float* xl = xs + 68 * r + 4 * g;                // row r of a fragment lies 64 samples = 68 floats further
  const float* hl = hs + 16 + r - 4 * g;
  // the fragment of the rows i0 + d + 4 r of this wave, d = tile - block, relative to the staged span
  auto xfrag = [&](int d) {
    const int nb = 16 * (64 * w + d + kFirMC);
    return *reinterpret_cast<const f32x4*>(xl + nb + 4 * (nb >> 6));
  };
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int Mtot = (a.K + 14) / 16 + 1;                 // blocks m with a tap 16 m + j - c inside [0, K)
  for (int q = 0; q * kFirMC < Mtot; ++q) {
    const int Mc = Mtot - q * kFirMC < kFirMC ? Mtot - q * kFirMC : kFirMC;
    const int Mr = (Mc + 3) & ~3;                       // whole groups of four blocks; the surplus taps are staged as zeros
    __syncthreads();                                    // the previous piece's readers are done
    const int k0 = 16 * q * kFirMC - 16;
    for (int p = threadIdx.x; p < 16 * Mr + 32; p += kFirThreads) {
      const int k = k0 + p;
      hs[p] = (k >= 0 && k < a.K) ? h[k] : 0.0f;
    }
    const int64_t xlo = N0 - (int64_t)16 * (q + 1) * kFirMC;       // sample of span position 0: a multiple of 64
    const int p_lo = (16 * (kFirMC - Mr + 1)) & ~63;
    for (int p = p_lo + 4 * threadIdx.x; p < kFirSpan; p += 4 * kFirThreads) {
      const int64_t n = xlo + p;
      float v[4];
      if (a.vec_x && n >= 0 && n + 4 <= L) {
        if constexpr (sizeof(T) == 4) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(x + n);
          v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
        } else {
          const uint2 u = *reinterpret_cast<const uint2*>(x + n);
          v[0] = to_float((int16_t)(u.x & 0xffffu)); v[1] = to_float((int16_t)(u.x >> 16));
          v[2] = to_float((int16_t)(u.y & 0xffffu)); v[3] = to_float((int16_t)(u.y >> 16));
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (n + e >= 0 && n + e < L) ? to_float(x[n + e]) : 0.0f;
      }
      *reinterpret_cast<f32x4*>(xs + p + 4 * (p >> 6)) = f32x4{v[0], v[1], v[2], v[3]};
    }
    __syncthreads();
    if (!active) continue;
    f32x4 fr[4];
    fr[1] = xfrag(1); fr[2] = xfrag(2); fr[3] = xfrag(3);
    for (int mm = 0; mm < Mr; mm += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fr[(4 - u) & 3] = xfrag(-(mm + u));
        const float* hp = hl + 16 * (mm + u);
        const float bv[4] = {hp[0], hp[-1], hp[-2], hp[-3]};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = mfma4(fr[(t - u) & 3][s], bv[s], acc[t]);
      }
    }
  }
  // accumulator register e of tile t: row 4 g + e of the tile, column r
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t n = N0 + 16 * (64 * w + t + 4 * (4 * g + e)) + r;
      if (n < a.Opad) yrow[n] = n < out_len ? acc[t][e] : 0.0f;
    }
}

// ---- SNR mixing -------------------------------------------------------------------------------------------------------------------
constexpr int kMixThreads = 1024;

struct MixArgs {
  const float* x;         // [B, Lpad]
  const int32_t* len;     // [B]
  const float* d;         // [B, Dpad]
  const float* snr_db;    // [B]
  float* y;               // [B, Lpad]
  int64_t Lpad, Dpad;
  int quantise;
};

// DESCENDING offsets (32, 16, .. 1), unlike common.h's wave_sum: kept apart on purpose, the two orders round a float64 sum differently
__device__ __forceinline__ double wave_sum_descending(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kMixThreads) void mix_snr_kernel(MixArgs a) {
  __shared__ double red[2][kMixThreads / 64];
  __shared__ float g_sh;
  const int b = blockIdx.x;
  const int64_t L = a.len[b] > 0 ? ((int64_t)a.len[b] < a.Lpad ? (int64_t)a.len[b] : a.Lpad) : 0;
  const float* x = a.x + (int64_t)b * a.Lpad;
  const float* d = a.d + (int64_t)b * a.Dpad;
  float* y = a.y + (int64_t)b * a.Lpad;
  double px = 0.0, pd = 0.0;
  for (int64_t i = threadIdx.x; i < L; i += kMixThreads) {
    const double xv = x[i], dv = d[i];
    px += xv * xv;
    pd += dv * dv;
  }
  px = wave_sum_descending(px);
  pd = wave_sum_descending(pd);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = px;
    red[1][threadIdx.x >> 6] = pd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sx = 0.0, sd = 0.0;
    for (int i = 0; i < kMixThreads / 64; ++i) {
      sx += red[0][i];
      sd += red[1][i];
    }
    g_sh = (sx > 0.0 && sd > 0.0) ? (float)sqrt(sx / exp10((double)a.snr_db[b] / 10.0) / sd) : 0.0f;
  }
  __syncthreads();
  const float g = g_sh;
  for (int64_t i = threadIdx.x; i < a.Lpad; i += kMixThreads) {
    float v = 0.0f;
    if (i < L) {
      v = __builtin_fmaf(g, d[i], x[i]);
      if (a.quantise) v = truncf(fminf(fmaxf(v, -1.0f), 1.0f) * 32768.0f) * (1.0f / 32768.0f);
    }
    y[i] = v;
  }
}

// ---- image-source room impulse responses ------------------------------------------------------------------------------------------
constexpr int kRirThreads = 256;                        // = samples per workgroup
constexpr int kRirMaxN = 16384;
constexpr int kRirMaxOrder = 255;                       // images per axis and side: n_d = ceil(nsample / (2 L_d)) <= this
constexpr int kRirMaxTw = 1024;                         // window taps: fs <= 128 kHz
constexpr int kRirList = 4 * kRirThreads;               // images a round can keep
constexpr int kRirIn = 20;                              // doubles per row of params_host
// a row of the device table (doubles): room, source, receiver in samples; six reflection coefficients; cTs; nsample; hp; n_d;
// Tw; the high-pass coefficients B1, B2, A1, R1
constexpr int kRirRow = 28;
enum { RT_L = 0, RT_S = 3, RT_R = 6, RT_BETA = 9, RT_CTS = 15, RT_NS = 16, RT_HP = 17, RT_ND = 18, RT_TW = 21, RT_B1 = 22, RT_B2 = 23,
       RT_A1 = 24, RT_R1 = 25 };

struct RirArgs {
  const double* table;    // [B, kRirRow]
  float* h;               // [B, Kpad]
  int Kpad;
};

__global__ __launch_bounds__(kRirThreads) void rir_kernel(RirArgs a) {
  __shared__ double bp[6][kRirMaxOrder + 2];            // beta_a ^ e
  __shared__ __attribute__((aligned(16))) float list[kRirList * 8];
  __shared__ float ck[kRirMaxTw], sk[kRirMaxTw];        // cos / sin(2 pi kk / Tw) at kk = i - Tw/2 + 1
  __shared__ int wsum[kRirThreads / 64];
  const double* tb = a.table + (size_t)blockIdx.y * kRirRow;
  float* hrow = a.h + (size_t)blockIdx.y * a.Kpad;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nsample = (int)tb[RT_NS], Tw = (int)tb[RT_TW], half = Tw / 2;
  const int n0 = blockIdx.x * kRirThreads, n = n0 + tid;
  if (n0 >= nsample) {
    if (n < a.Kpad) hrow[n] = 0.0f;
    return;
  }
  const int nx = (int)tb[RT_ND], ny = (int)tb[RT_ND + 1], nz = (int)tb[RT_ND + 2];
  if (tid < 6) {
    const double beta = tb[RT_BETA + tid];
    const int top = (tid < 2 ? nx : tid < 4 ? ny : nz) + 1;
    double p = 1.0;
    for (int e = 0; e <= top; ++e) {
      bp[tid][e] = p;
      p *= beta;
    }
  }
  for (int i = tid; i < Tw; i += kRirThreads) {
    const double ang = 2.0 * (double)(i - half + 1) / (double)Tw;
    ck[i] = (float)cospi(ang);
    sk[i] = (float)sinpi(ang);
  }
  const double Lx = tb[RT_L], Ly = tb[RT_L + 1], Lz = tb[RT_L + 2];
  const double sx = tb[RT_S], sy = tb[RT_S + 1], sz = tb[RT_S + 2];
  const double rx = tb[RT_R], ry = tb[RT_R + 1], rz = tb[RT_R + 2];
  const double inv_norm = 1.0 / (4.0 * 3.14159265358979323846 * tb[RT_CTS]);
  const int Ny = 2 * ny + 1, Nz = 2 * nz + 1;
  const int pairs = (2 * nx + 1) * Ny * Nz * 2;
  // images whose window meets [n0, n0 + 255]: fdist in [f_lo, f_hi], and fdist < nsample; the test on squares is one wider on
  // both sides (a rounded square root can land on the integer next to it), the exact test follows the root
  const int f_lo = n0 - half > 0 ? n0 - half : 0;
  const int f_top = n0 + kRirThreads - 2 + half;
  const int f_hi = f_top < nsample - 1 ? f_top : nsample - 1;
  const double lo2 = f_lo > 0 ? (double)(f_lo - 1) * (double)(f_lo - 1) : 0.0;
  const double hi2 = (double)(f_hi + 2) * (double)(f_hi + 2);
  double acc = 0.0;
  for (int base = 0; base < pairs; base += kRirThreads) {
    const int id = base + tid;
    double d2[4] = {0.0, 0.0, 0.0, 0.0};
    int mx = 0, my = 0, mz = 0, qq = 0, keep = 0;
    if (id < pairs) {
      const int tri = id >> 1;
      qq = id & 1;
      const int az = tri % Nz, rest = tri / Nz;
      mz = az - nz; my = rest % Ny - ny; mx = rest / Ny - nx;
      const double dx = (double)(1 - 2 * qq) * sx - rx + 2.0 * (double)mx * Lx;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = e >> 1, k = e & 1;
        const double dy = (double)(1 - 2 * j) * sy - ry + 2.0 * (double)my * Ly;
        const double dz = (double)(1 - 2 * k) * sz - rz + 2.0 * (double)mz * Lz;
        d2[e] = dx * dx + dy * dy + dz * dz;
        if (d2[e] >= lo2 && d2[e] < hi2) keep |= 1 << e;
      }
    }
    double dist[4];
    int fd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dist[e] = 0.0; fd[e] = 0;
      if (keep & (1 << e)) {
        dist[e] = sqrt(d2[e]);
        fd[e] = (int)floor(dist[e]);
        if (fd[e] < f_lo || fd[e] > f_hi || !(dist[e] > 0.0)) keep &= ~(1 << e);
      }
    }
    // this thread's place in the list: the images before it in image order
    const int cnt = __popc(keep);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    __syncthreads();                                    // the previous round's readers of the list and of wsum are done
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int off = incl - cnt, total = 0;
#pragma unroll
    for (int i = 0; i < kRirThreads / 64; ++i) {
      if (i < wv) off += wsum[i];
      total += wsum[i];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (keep & (1 << e)) {
        const int j = e >> 1, k = e & 1;
        const int ex1 = mx - qq < 0 ? qq - mx : mx - qq, ex2 = mx < 0 ? -mx : mx;
        const int ey1 = my - j < 0 ? j - my : my - j, ey2 = my < 0 ? -my : my;
        const int ez1 = mz - k < 0 ? k - mz : mz - k, ez2 = mz < 0 ? -mz : mz;
        const double gain = bp[0][ex1] * bp[1][ex2] * bp[2][ey1] * bp[3][ey2] * bp[4][ez1] * bp[5][ez2] * inv_norm / dist[e];
        const float f = (float)(dist[e] - (double)fd[e]);
        const double fdbl = (double)f;
        float* ent = list + 8 * off;
        // 0.25 = the window's 0.5 times Fc = 0.5
        *reinterpret_cast<f32x4*>(ent) = f32x4{__int_as_float(fd[e]), (float)(0.25 * gain), f, (float)sinpi(0.5 * fdbl)};
        *reinterpret_cast<f32x4*>(ent + 4) = f32x4{(float)cospi(0.5 * fdbl), (float)sinpi(2.0 * fdbl / (double)Tw),
                                                  (float)cospi(2.0 * fdbl / (double)Tw), 0.0f};
        ++off;
      }
    }
    __syncthreads();
    for (int i = 0; i < total; ++i) {
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(list + 8 * i);
      const int kk = n - __float_as_int(e0.x);
      if (kk > -half && kk <= half) {
        const f32x4 e1 = *reinterpret_cast<const f32x4*>(list + 8 * i + 4);
        const float t = (float)kk - e0.z;
        const int ph = kk & 3;
        const float num = ph == 0 ? -e0.w : ph == 1 ? e1.x : ph == 2 ? e0.w : -e1.x;
        const float sinc = t == 0.0f ? 1.0f : num / (1.57079632679489662f * t);
        const float win = 1.0f + (ck[kk + half - 1] * e1.z + sk[kk + half - 1] * e1.y);
        acc += (double)(e0.y * win * sinc);
      }
    }
  }
  if (n < a.Kpad) hrow[n] = n < nsample ? (float)acc : 0.0f;
}

constexpr int kHpChunk = 4096;

__global__ __launch_bounds__(256) void rir_highpass_kernel(RirArgs a) {
  __shared__ __attribute__((aligned(16))) float buf[kHpChunk];
  const double* tb = a.table + (size_t)blockIdx.x * kRirRow;
  if (tb[RT_HP] == 0.0) return;
  float* hrow = a.h + (size_t)blockIdx.x * a.Kpad;
  const int nsample = (int)tb[RT_NS];
  const double B1 = tb[RT_B1], B2 = tb[RT_B2], A1 = tb[RT_A1], R1 = tb[RT_R1];
  double y1 = 0.0, y2 = 0.0;                            // lane 0's state: Y[1], Y[2] of the recurrence
  for (int c0 = 0; c0 < nsample; c0 += kHpChunk) {
    const int cn = nsample - c0 < kHpChunk ? nsample - c0 : kHpChunk;
    for (int i = threadIdx.x; i < cn; i += 256) buf[i] = hrow[c0 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < cn; ++i) {
        const double y0 = B1 * y1 + (B2 * y2 + (double)buf[i]);
        buf[i] = (float)(y0 + A1 * y1 + R1 * y2);
        y2 = y1;
        y1 = y0;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cn; i += 256) hrow[c0 + i] = buf[i];
    __syncthreads();
  }
}

// one row of params_host -> one row of the device table, or EINVAL naming what is wrong
int rir_row(const double* p, int row, int Kpad, double* t) {
  const double* Lm = p; const double* sm = p + 3; const double* rm = p + 6;
  const double c = p[9], fs = p[10], T60 = p[11];
  const double* beta = p + 12;
  const double hp = p[18], ns = p[19];
  if (!(c > 0.0) || !(fs > 0.0)) return fail(MI355ASR_EINVAL, "rir row %d: sound speed %g and sample rate %g must be positive", row, c, fs);
  if (!(ns >= 1.0) || ns > kRirMaxN || ns != floor(ns) || ns > Kpad)
    return fail(MI355ASR_EINVAL, "rir row %d: nsample = %g is outside 1 .. min(%d, Kpad = %d)", row, ns, kRirMaxN, Kpad);
  bool same = true;
  for (int d = 0; d < 3; ++d) {
    if (!(Lm[d] > 0.0)) return fail(MI355ASR_EINVAL, "rir row %d: room dimension %d is %g", row, d, Lm[d]);
    if (!(sm[d] >= 0.0 && sm[d] <= Lm[d]) || !(rm[d] >= 0.0 && rm[d] <= Lm[d]))
      return fail(MI355ASR_EINVAL, "rir row %d: source %g or receiver %g is outside the room (axis %d, 0 .. %g m)", row, sm[d], rm[d], d, Lm[d]);
    same = same && sm[d] == rm[d];
  }
  if (same) return fail(MI355ASR_EINVAL, "rir row %d: the source is at the receiver (distance 0)", row);
  double bt[6];
  if (T60 > 0.0) {
    const double V = Lm[0] * Lm[1] * Lm[2], S = 2.0 * (Lm[0] * Lm[2] + Lm[1] * Lm[2] + Lm[0] * Lm[1]);
    const double alpha = 24.0 * V * log(10.0) / (c * S * T60);
    if (alpha > 1.0)
      return fail(MI355ASR_EINVAL, "rir row %d: reverberation_time = %g s is too short for this room (alpha = %g > 1)", row, T60, alpha);
    for (int i = 0; i < 6; ++i) bt[i] = sqrt(1.0 - alpha);
  } else {
    for (int i = 0; i < 6; ++i) {
      if (!(fabs(beta[i]) <= 1.0)) return fail(MI355ASR_EINVAL, "rir row %d: reflection coefficient %d is %g", row, i, beta[i]);
      bt[i] = beta[i];
    }
  }
  const double cTs = c / fs;
  const int Tw = 2 * (int)floor(0.004 * fs + 0.5);
  if (Tw < 2 || Tw > kRirMaxTw) return fail(MI355ASR_EINVAL, "rir row %d: sample rate %g gives a window of %d taps (2 .. %d)", row, fs, Tw, kRirMaxTw);
  for (int d = 0; d < 3; ++d) {
    t[RT_L + d] = Lm[d] / cTs; t[RT_S + d] = sm[d] / cTs; t[RT_R + d] = rm[d] / cTs;
    const double nd = ceil(ns / (2.0 * t[RT_L + d]));
    if (nd > kRirMaxOrder)
      return fail(MI355ASR_EINVAL, "rir row %d: axis %d of %g m needs %g images per side for %g samples (at most %d)", row, d, Lm[d], nd, ns, kRirMaxOrder);
    t[RT_ND + d] = nd;
  }
  for (int i = 0; i < 6; ++i) t[RT_BETA + i] = bt[i];
  t[RT_CTS] = cTs; t[RT_NS] = ns; t[RT_HP] = hp != 0.0 ? 1.0 : 0.0; t[RT_TW] = Tw;
  const double W = 2.0 * 3.14159265358979323846 * 100.0 / fs, R1 = exp(-W);
  t[RT_B1] = 2.0 * R1 * cos(W); t[RT_B2] = -R1 * R1; t[RT_A1] = -(1.0 + R1); t[RT_R1] = R1;
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_fir_ragged(const void* x_dev, int32_t dtype, const int32_t* in_len_dev, int32_t B, int64_t Lpad, const float* h_dev,
                        int32_t K, int64_t Kpad, int32_t shared_filter, float* y_dev, int64_t Opad, void* stream) {
  if (!x_dev || !in_len_dev || !h_dev || !y_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (dtype != MI355ASR_DT_F32 && dtype != MI355ASR_DT_I16) return fail(MI355ASR_EINVAL, "fir: input dtype %d is neither float32 nor int16", dtype);
  if (K < 1 || K > kFirMaxK || Kpad < K) return fail(MI355ASR_EINVAL, "fir: need 1 <= K <= %d and Kpad >= K (got K = %d, Kpad = %lld)", kFirMaxK, K, (long long)Kpad);
  if (B < 1 || B > 65535 || Lpad < 1 || Opad < 1 || Lpad > INT32_MAX - 2 * kFirMaxK)
    return fail(MI355ASR_EINVAL, "fir: need 1 <= B <= 65535, 1 <= Lpad < 2^31 - 32768, Opad >= 1 (got %d, %lld, %lld)", B, (long long)Lpad, (long long)Opad);
  const int64_t gx = (Opad + kFirTile - 1) / kFirTile;
  if (gx > INT32_MAX) return fail(MI355ASR_EINVAL, "fir: Opad = %lld gives too many tiles", (long long)Opad);
  const size_t esz = dtype == MI355ASR_DT_F32 ? 4 : 2;
  FirArgs a{};
  a.x = x_dev; a.in_len = in_len_dev; a.h = h_dev; a.y = y_dev; a.Lpad = Lpad; a.h_stride = shared_filter ? 0 : Kpad; a.Opad = Opad; a.K = K;
  a.vec_x = !((uintptr_t)x_dev & 15) && (Lpad * esz) % 16 == 0;
  const dim3 grid((unsigned)gx, (unsigned)B), block(kFirThreads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MI355ASR_DT_F32) hipLaunchKernelGGL(fir_ragged_kernel<float>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(fir_ragged_kernel<int16_t>, grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_mix_snr(const float* x_dev, const int32_t* len_dev, const float* d_dev, const float* snr_db_dev, int32_t B, int64_t Lpad,
                     int64_t Dpad, int32_t quantise, float* y_dev, void* stream) {
  if (!x_dev || !len_dev || !d_dev || !snr_db_dev || !y_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || Lpad < 1 || Dpad < Lpad)
    return fail(MI355ASR_EINVAL, "mix: need B >= 1 and 1 <= Lpad <= Dpad (got %d, %lld, %lld)", B, (long long)Lpad, (long long)Dpad);
  MixArgs a{};
  a.x = x_dev; a.len = len_dev; a.d = d_dev; a.snr_db = snr_db_dev; a.y = y_dev; a.Lpad = Lpad; a.Dpad = Dpad; a.quantise = quantise != 0;
  hipLaunchKernelGGL(mix_snr_kernel, dim3((unsigned)B), dim3(kMixThreads), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_rir_workspace_bytes(int32_t B, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535) return fail(MI355ASR_EINVAL, "rir: need 1 <= B <= 65535 (got %d)", B);
  *ws_bytes = (size_t)B * kRirRow * sizeof(double);
  return 0;
}

int mi355asr_rir_generate(const double* params_host, int32_t B, float* h_dev, int32_t Kpad, void* ws_dev, size_t ws_bytes, void* stream) {
  if (!params_host || !h_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535 || Kpad < 1) return fail(MI355ASR_EINVAL, "rir: need 1 <= B <= 65535 and Kpad >= 1 (got %d, %d)", B, Kpad);
  if ((uintptr_t)ws_dev & 7) return fail(MI355ASR_EINVAL, "rir: the workspace must be 8-byte aligned");
  if (ws_bytes < (size_t)B * kRirRow * sizeof(double)) return fail(MI355ASR_EWORKSPACE, "rir: workspace too small: %zu bytes", ws_bytes);
  std::vector<double> table((size_t)B * kRirRow, 0.0);
  bool any_hp = false;
  for (int b = 0; b < B; ++b) {
    if (int rc = rir_row(params_host + (size_t)b * kRirIn, b, Kpad, &table[(size_t)b * kRirRow])) return rc;
    any_hp = any_hp || table[(size_t)b * kRirRow + RT_HP] != 0.0;
  }
  hipStream_t s = (hipStream_t)stream;
  // the table comes from pageable host memory: the runtime stages it before the call returns, nothing is waited for
  HIP_TRY(hipMemcpyAsync(ws_dev, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, s));
  RirArgs a{};
  a.table = (const double*)ws_dev; a.h = h_dev; a.Kpad = Kpad;
  hipLaunchKernelGGL(rir_kernel, dim3((unsigned)((Kpad + kRirThreads - 1) / kRirThreads), (unsigned)B), dim3(kRirThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  if (any_hp) {
    hipLaunchKernelGGL(rir_highpass_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
