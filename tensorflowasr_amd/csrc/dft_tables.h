// Host tables of the two-stage MFMA DFT, N = 32 x N2 with N2 = 16 (512), 32 (1024) or 64 (2048): what stft.hip and stft_loss.hip
// upload for dft_block_gemm (dft_mfma.h) and their twiddle passes.  Plain C++17 without a HIP include, so that a host-only program
// can build and dump the tables (tools/dft_tables_dump, tests/test_dft_tables_host.py).  Every value is computed in float64 and
// rounded to float once.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mi355 {

constexpr double kPi = 3.14159265358979323846;

// cos / sin of 2 pi (a b mod M) / M
inline double cosm(int64_t a, int64_t b, int64_t M) { return std::cos(2.0 * kPi * (double)((a * b) % M) / (double)M); }
inline double sinm(int64_t a, int64_t b, int64_t M) { return std::sin(2.0 * kPi * (double)((a * b) % M) / (double)M); }

// T [M][K] (double) -> fragment order [M / 16][K / 4][64]: the A operand of v_mfma_f32_16x16x4_f32, lane holds
// T[16 mt + (lane & 15)][4 ks + (lane >> 4)], one coalesced 256-byte load per MFMA
inline void pack_frag(const std::vector<double>& T, int M, int K, std::vector<float>* out) {
  const size_t base = out->size();
  out->resize(base + (size_t)M * K);
  for (int mt = 0; mt < M / 16; ++mt)
    for (int ks = 0; ks < K / 4; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        (*out)[base + ((size_t)mt * (K / 4) + ks) * 64 + lane] = (float)T[(size_t)(16 * mt + (lane & 15)) * K + 4 * ks + (lane >> 4)];
}

// A periodic Hann window of win samples at [offset, offset + win) of N, zero elsewhere: N floats appended to buf, the window or
// (squared) its square formed in float64
inline void append_hann(int win, int N, int offset, bool squared, std::vector<float>* buf) {
  for (int n = 0; n < N; ++n) {
    const int j = n - offset;
    const double w = j >= 0 && j < win ? 0.5 - 0.5 * std::cos(2.0 * kPi * j / win) : 0.0;
    buf->push_back((float)(squared ? w * w : w));
  }
}

// where append_dft_tables put its six tables (floats from the start of buf)
struct DftOffsets { size_t twc, tws, T1, T2, T3, T4; };

// Appends the two twiddle tables [32][N2] and the four packed stage matrices to buf.  t4_scale multiplies the last stage of the
// inverse: 1.0 / N for the inverse DFT, 1.0 for the transpose of the forward one (a power of two, so the product is exact and the
// one rounding is the conversion to float).
inline DftOffsets append_dft_tables(int N, double t4_scale, std::vector<float>* buf) {
  const int N2 = N / 32, H = N2 / 2;
  DftOffsets at;
  at.twc = buf->size();
  for (int k1 = 0; k1 < 32; ++k1)
    for (int n2 = 0; n2 < N2; ++n2) buf->push_back((float)cosm(k1, n2, N));
  at.tws = buf->size();
  for (int k1 = 0; k1 < 32; ++k1)
    for (int n2 = 0; n2 < N2; ++n2) buf->push_back((float)sinm(k1, n2, N));
  std::vector<double> T;
  // forward stage 1 [64][32]: rows k1 cos, rows 32 + k1 -sin
  T.assign(64 * 32, 0.0);
  for (int k1 = 0; k1 < 32; ++k1)
    for (int n1 = 0; n1 < 32; ++n1) {
      T[k1 * 32 + n1] = cosm(k1, n1, 32);
      T[(32 + k1) * 32 + n1] = -sinm(k1, n1, 32);
    }
  at.T1 = buf->size();
  pack_frag(T, 64, 32, buf);
  // forward stage 2 [2 H][2 N2]: Re = C Bre + S Bim, Im = -S Bre + C Bim
  T.assign((size_t)2 * H * 2 * N2, 0.0);
  for (int k2 = 0; k2 < H; ++k2)
    for (int n2 = 0; n2 < N2; ++n2) {
      const double c = cosm(k2, n2, N2), s = sinm(k2, n2, N2);
      T[(size_t)k2 * 2 * N2 + n2] = c;
      T[(size_t)k2 * 2 * N2 + N2 + n2] = s;
      T[(size_t)(H + k2) * 2 * N2 + n2] = -s;
      T[(size_t)(H + k2) * 2 * N2 + N2 + n2] = c;
    }
  at.T2 = buf->size();
  pack_frag(T, 2 * H, 2 * N2, buf);
  // inverse stage 1 [64][64]: Re = C Fre - S Fim, Im = S Fre + C Fim
  T.assign(64 * 64, 0.0);
  for (int p = 0; p < 32; ++p)
    for (int k1 = 0; k1 < 32; ++k1) {
      const double c = cosm(p, k1, 32), s = sinm(p, k1, 32);
      T[p * 64 + k1] = c;
      T[p * 64 + 32 + k1] = -s;
      T[(32 + p) * 64 + k1] = s;
      T[(32 + p) * 64 + 32 + k1] = c;
    }
  at.T3 = buf->size();
  pack_frag(T, 64, 64, buf);
  // inverse stage 2 [N2][2 N2]: y = (C Bre - S Bim) t4_scale
  T.assign((size_t)N2 * 2 * N2, 0.0);
  for (int q = 0; q < N2; ++q)
    for (int k2 = 0; k2 < N2; ++k2) {
      T[(size_t)q * 2 * N2 + k2] = cosm(q, k2, N2) * t4_scale;
      T[(size_t)q * 2 * N2 + N2 + k2] = -sinm(q, k2, N2) * t4_scale;
    }
  at.T4 = buf->size();
  pack_frag(T, N2, 2 * N2, buf);
  return at;
}

}  // namespace mi355
