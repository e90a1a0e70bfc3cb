// The device side of the two-stage MFMA DFT that stft.hip and stft_loss.hip share: the tile helper, the six table pointers of a
// kernel argument, and the cache that uploads a set of host tables (dft_tables.h) once per device and key.
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"
#include "dft_tables.h"
#include "model.h"

namespace mi355 {

// D[M = 16 MT][N = 16 NT] = T[M][K = 4 KS] * Bm[K][N]: T packed as [mt][ks][lane] = T[16 mt + (lane & 15)][4 ks + (lane >> 4)]
// (pack_frag), Bm in LDS with row stride ldb; store(row, col, value) receives every element once.  The accumulator tiles are
// shared out over the THREADS / 64 waves of the workgroup, each tile one chain over k ascending.
template <int THREADS, int MT, int NT, int KS, typename Store>
DEV void dft_block_gemm(const float* __restrict__ Tp, const float* Bm, int ldb, Store store) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll 1
  for (int t = wave; t < MT * NT; t += THREADS / 64) {
    const int mt = t / NT, nt = t - mt * NT;
    const float* tp = Tp + (size_t)mt * KS * 64 + lane;
    const float* bp = Bm + g * ldb + 16 * nt + c;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int ks = 0; ks < KS; ++ks) acc = mfma4(tp[ks * 64], bp[4 * ks * ldb], acc);
    store(16 * mt + 4 * g + 0, 16 * nt + c, acc.x);
    store(16 * mt + 4 * g + 1, 16 * nt + c, acc.y);
    store(16 * mt + 4 * g + 2, 16 * nt + c, acc.z);
    store(16 * mt + 4 * g + 3, 16 * nt + c, acc.w);
  }
}

struct DftTables {
  const float* twc;       // [32][N2] cos(2 pi k1 n2 / N)
  const float* tws;       // [32][N2] sin(2 pi k1 n2 / N)
  const float* T1;        // packed stage matrices, forward 1 and 2, inverse 1 and 2
  const float* T2;
  const float* T3;
  const float* T4;
};

inline DftTables dft_pointers(const float* d, const DftOffsets& at) {
  return DftTables{d + at.twc, d + at.tws, d + at.T1, d + at.T2, d + at.T3, d + at.T4};
}

// One set of tables per device and key, built and uploaded on first use and kept for the life of the process.  build(&buf)
// appends the host tables to buf and returns a callable (const float* device_base) -> Tables that places them.
template <typename Key, typename Tables>
struct TableCache {
  std::mutex mu;
  std::map<std::pair<int, Key>, Tables> map;

  template <typename Build>
  int get(const Key& key, Tables* t, Build build) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = map.find({dev, key});
    if (it == map.end()) {
      std::vector<float> buf;
      const auto place = build(&buf);
      float* d = nullptr;
      HIP_TRY(hipMalloc(&d, buf.size() * sizeof(float)));
      HIP_TRY(hipMemcpy(d, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
      it = map.emplace(std::make_pair(dev, key), place(d)).first;
    }
    *t = it->second;
    return 0;
  }
};

}  // namespace mi355
