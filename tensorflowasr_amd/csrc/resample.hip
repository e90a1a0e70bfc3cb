// Polyphase resampling (scipy.signal.resample_poly with its default Kaiser filter) behind mi355asr_resample* of include/mi355asr.h.
//
// With g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g, half = 10 max(up, down) and an n = 2 half + 1 tap filter h
// (designed on the host, float64, rounded once to fp32), output k of a row of L samples is
//     c = k down + half,  p = c mod up,  jh = c div up,      y[k] = sum_{m = 0 .. K-1} hp[p][m] x[jh - m]
// with hp[p][m] = h[p + m up] (0 past the filter's end), K = ceil(n / up) and x = 0 outside [0, L).  Every output is ONE fp32 FMA
// chain over m = 0 .. K-1 in that order, zero terms included, in both kernels of this file: that is what makes a row of a ragged
// batch equal the row alone, and the concatenated output of a stream equal the one-shot call, bit for bit.
//
// resample_kernel: one workgroup per (row, group of output tiles).  The filter lies in LDS phase-major with an odd row stride Ks
// (threads of a wave read different phases: distinct banks); per tile the input span the tile's outputs touch is staged in LDS with
// 16-byte loads (int16 input is converted there, x / 32768, exact), each thread item computes kR outputs that lie `up` apart --
// they share their phase, so one tap read feeds kR FMAs -- and the tile's outputs leave through LDS as 16-byte stores.  A ratio
// whose span does not fit (hundreds of input samples per output) reads its samples through the caches instead (STAGE = false):
// the same chain, the same bits.  Output indices, k down and the row offsets are 64-bit.
//
// resample_stream_kernel: one workgroup per named stream slot.  A slot's device state is a ring of K - 1 + max_packet samples,
// ring[j mod cap] = x[j]: the K - 1 samples before the packet are all that pending outputs still need (the first output that is
// not final after N samples has jh >= N).  Positions are the caller's (64-bit, host): the launcher turns them into small
// per-slot integers, so the kernel's arithmetic is 32-bit and a step waits for nothing.  The step reads the ring's history,
// writes the packet behind it (disjoint cells), and runs the same tile routine on [history | packet | zeros].
#include "model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kR = 4;                    // outputs per thread item
constexpr int kTileTarget = 1024;        // outputs per tile: the next multiple of up * kR
constexpr int kMaxRatio = 640;           // max(up, down): the filter (<= 12801 taps + row padding) fits in LDS
constexpr size_t kLdsBudget = 80 * 1024; // two workgroups per CU
constexpr int kTableInts = 8;            // per named slot: slot, packet samples, outputs, ring position, base_q, base_r

struct RsPlan {
  int up, down, half, K, Ks, tile, hp_floats, span_cap, staged;
  size_t lds;
};

int make_plan(int up, int down, RsPlan* p) {
  if (up < 1 || down < 1 || std::max(up, down) > kMaxRatio)
    return fail(MI355ASR_EINVAL, "resample: ratio %d/%d is outside 1 <= up, down <= %d", up, down, kMaxRatio);
  const int mr = std::max(up, down);
  p->up = up; p->down = down; p->half = 10 * mr;
  const int n = 2 * p->half + 1;
  p->K = (n + up - 1) / up;
  p->Ks = p->K | 1;
  p->hp_floats = (up * p->Ks + 3) & ~3;
  const int unit = up * kR;
  p->tile = unit * ((kTileTarget + unit - 1) / unit);
  // samples a tile's outputs touch, from any phase of its first output, plus the slack of staging from an 8-sample boundary
  const int64_t span = ((int64_t)(up - 1) + (int64_t)(p->tile - 1) * down) / up + p->K;
  const int64_t cap = (span + 8 + 8 + 3) & ~(int64_t)3;
  const size_t staged_bytes = ((size_t)p->hp_floats + (size_t)cap + (size_t)p->tile) * sizeof(float);
  p->staged = staged_bytes <= kLdsBudget;
  p->span_cap = p->staged ? (int)cap : 0;
  p->lds = p->staged ? staged_bytes : (size_t)p->hp_floats * sizeof(float);
  return 0;
}

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }

// samples of a staged span: xs[i] = x[j_lo + i]
struct LdsSamples {
  const float* xs;
  __device__ __forceinline__ float operator()(int i) const { return xs[i]; }
};

// samples of one row straight from memory: zero outside [0, L), which is never read
template <typename T>
struct RowSamples {
  const T* x;
  int64_t j_lo, L;
  __device__ __forceinline__ float operator()(int i) const {
    const int64_t j = j_lo + i;
    return (j >= 0 && j < L) ? to_float(x[j]) : 0.0f;
  }
};

// samples of a stream step relative to the packet's first sample: history from the ring, the packet, zeros after it
struct StreamSamples {
  const float* ring;
  const float* pkt;
  int ring_pos, cap, P, j_lo;        // ring_pos = (samples before the packet) mod cap
  __device__ __forceinline__ float operator()(int i) const {
    const int j = j_lo + i;
    if (j >= P) return 0.0f;
    if (j >= 0) return pkt[j];
    int r = ring_pos + j;            // j >= -(K - 1) > -cap
    if (r < 0) r += cap;
    return ring[r];
  }
};

// The outputs [0, tile) of a tile whose first output has c = (c div up) up + base_r; sample index 0 is (c div up) - (K - 1).
// n_valid of them exist (the rest are written as 0), n_store are inside the output row.  STAGE: through ys (LDS) as 16-byte stores.
template <bool STAGE, class X>
__device__ __forceinline__ void fir_tile(const float* hp, X xs, float* ys, int up, int down, int K, int Ks, int tile, int base_r,
                                         int n_valid, int n_store, float* y, bool vec_y) {
  const int items = tile / kR;
  for (int u = threadIdx.x; u < items; u += kThreads) {
    const int q = u / up, ph = u - q * up;
    const int i0 = q * up * kR + ph;
    if (i0 >= n_valid) {
      if (STAGE) {
#pragma unroll
        for (int r = 0; r < kR; ++r) ys[i0 + r * up] = 0.0f;
      } else {
#pragma unroll
        for (int r = 0; r < kR; ++r)
          if (i0 + r * up < n_store) y[i0 + r * up] = 0.0f;
      }
      continue;
    }
    const int t = base_r + i0 * down;
    const int jrel = t / up, p = t - jrel * up;
    const float* hrow = hp + p * Ks;
    const int top = jrel + K - 1;
    float acc[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = 0.0f;
    for (int m = 0; m < K; ++m) {
      const float h = hrow[m];
#pragma unroll
      for (int r = 0; r < kR; ++r) acc[r] = __builtin_fmaf(h, xs(top - m + r * down), acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int i = i0 + r * up;
      const float v = i < n_valid ? acc[r] : 0.0f;
      if (STAGE) ys[i] = v;
      else if (i < n_store) y[i] = v;
    }
  }
  if (STAGE) {
    __syncthreads();
    if (vec_y) {
      for (int i = threadIdx.x * 4; i < n_store; i += kThreads * 4) {
        if (i + 4 <= n_store) *reinterpret_cast<float4*>(y + i) = *reinterpret_cast<const float4*>(ys + i);
        else for (int e = i; e < n_store; ++e) y[e] = ys[e];
      }
    } else {
      for (int i = threadIdx.x; i < n_store; i += kThreads) y[i] = ys[i];
    }
  }
}

__device__ __forceinline__ void stage_filter(float* hp, const float* filt, int hp_floats) {
  for (int i = threadIdx.x * 4; i < hp_floats; i += kThreads * 4)
    *reinterpret_cast<float4*>(hp + i) = *reinterpret_cast<const float4*>(filt + i);
}

struct RsArgs {
  const void* x;          // [B, Lpad] float or int16
  const int32_t* in_len;  // [B]
  const float* filt;      // [hp_floats] phase-major, row stride Ks
  float* y;               // [B, Opad]
  int64_t Lpad, Opad, tiles;
  int up, down, half, K, Ks, tile, hp_floats, span_cap, tiles_per_wg;
  int vec_x, vec_y;       // rows of x / y start on 16-byte boundaries
};

template <typename T, bool STAGE>
__global__ __launch_bounds__(kThreads) void resample_kernel(RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hp = lds;
  float* xs = lds + a.hp_floats;
  float* ys = xs + a.span_cap;
  const int b = blockIdx.y;
  const int64_t L = a.in_len[b] > 0 ? ((int64_t)a.in_len[b] < a.Lpad ? (int64_t)a.in_len[b] : a.Lpad) : 0;
  const int64_t out_len = (L * a.up + a.down - 1) / a.down;
  const T* x = reinterpret_cast<const T*>(a.x) + (int64_t)b * a.Lpad;
  float* yrow = a.y + (int64_t)b * a.Opad;
  const int64_t t_begin = (int64_t)blockIdx.x * a.tiles_per_wg;
  const int64_t t_end = t_begin + a.tiles_per_wg < a.tiles ? t_begin + a.tiles_per_wg : a.tiles;
  constexpr int kVec = 16 / (int)sizeof(T);       // samples per 16-byte load
  bool filter_in = false;
  for (int64_t tt = t_begin; tt < t_end; ++tt) {
    const int64_t k0 = tt * a.tile;
    const int64_t left = a.Opad - k0;
    const int n_store = left < a.tile ? (int)left : a.tile;
    float* y = yrow + k0;
    if (k0 >= out_len) {                           // nothing of the row here: zeros
      if (a.vec_y) {
        for (int i = threadIdx.x * 4; i < n_store; i += kThreads * 4) {
          if (i + 4 <= n_store) *reinterpret_cast<float4*>(y + i) = make_float4(0.f, 0.f, 0.f, 0.f);
          else for (int e = i; e < n_store; ++e) y[e] = 0.0f;
        }
      } else {
        for (int i = threadIdx.x; i < n_store; i += kThreads) y[i] = 0.0f;
      }
      continue;
    }
    if (!filter_in) {
      stage_filter(hp, a.filt, a.hp_floats);
      filter_in = true;
    }
    const int n_valid = out_len - k0 < a.tile ? (int)(out_len - k0) : a.tile;
    const int64_t c0 = k0 * a.down + a.half;
    const int64_t base_q = c0 / a.up;
    const int base_r = (int)(c0 - base_q * a.up);
    const int64_t j_lo = base_q - (a.K - 1);
    if (STAGE) {
      // the span from the 16-byte boundary at or below j_lo (floor, also for negative j_lo)
      const int64_t j_al = j_lo - (((j_lo % kVec) + kVec) % kVec);
      const int shift = (int)(j_lo - j_al);
      const int span = (int)(((int64_t)base_r + (int64_t)(a.tile - 1) * a.down) / a.up) + a.K + shift;
      __syncthreads();                             // the previous tile's readers of xs and ys are done
      for (int i = threadIdx.x * kVec; i < span; i += kThreads * kVec) {
        const int64_t j = j_al + i;
        float v[kVec];
        if (a.vec_x && j >= 0 && j + kVec <= L) {
          if constexpr (sizeof(T) == 4) {
            const float4 w = *reinterpret_cast<const float4*>(x + j);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
          } else {
            const uint4 w = *reinterpret_cast<const uint4*>(x + j);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[2 * e] = to_float((int16_t)(ww[e] & 0xffffu));
              v[2 * e + 1] = to_float((int16_t)(ww[e] >> 16));
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < kVec; ++e) v[e] = (j + e >= 0 && j + e < L) ? to_float(x[j + e]) : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < kVec; e += 4) *reinterpret_cast<float4*>(xs + i + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
      }
      __syncthreads();
      fir_tile<true>(hp, LdsSamples{xs + shift}, ys, a.up, a.down, a.K, a.Ks, a.tile, base_r, n_valid, n_store, y, a.vec_y != 0);
    } else {
      __syncthreads();                             // the filter is in
      fir_tile<false>(hp, RowSamples<T>{x, j_lo, L}, nullptr, a.up, a.down, a.K, a.Ks, a.tile, base_r, n_valid, n_store, y, false);
    }
  }
}

struct RsStreamArgs {
  float* state;           // [n_streams, cap] rings
  const int32_t* table;   // [n, kTableInts]
  const float* x;         // [n, Ppad] packets (null on a flush)
  const float* filt;
  float* y;               // [n, out_cap]
  int up, down, K, Ks, tile, hp_floats, span_cap, cap, Ppad, out_cap;
};

template <bool STAGE>
__global__ __launch_bounds__(kThreads) void resample_stream_kernel(RsStreamArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hp = lds;
  float* xs = lds + a.hp_floats;
  float* ys = xs + a.span_cap;
  const int row = blockIdx.x;
  const int32_t* t = a.table + row * kTableInts;
  const int slot = t[0], P = t[1], n_out = t[2], ring_pos = t[3], base_q = t[4], base_r0 = t[5];
  float* ring = a.state + (size_t)slot * a.cap;
  const float* pkt = a.x ? a.x + (size_t)row * a.Ppad : nullptr;
  float* yrow = a.y + (size_t)row * a.out_cap;
  if (n_out > 0) stage_filter(hp, a.filt, a.hp_floats);
  for (int k0 = 0; k0 < n_out; k0 += a.tile) {
    const int n_valid = n_out - k0 < a.tile ? n_out - k0 : a.tile;
    const int tq = base_r0 + k0 * a.down;         // < 2^31: checked by the launcher
    const int tile_q = tq / a.up, base_r = tq - tile_q * a.up;
    StreamSamples src{ring, pkt, ring_pos, a.cap, P, base_q + tile_q - (a.K - 1)};
    if (STAGE) {
      const int span = (base_r + (a.tile - 1) * a.down) / a.up + a.K;
      __syncthreads();
      for (int i = threadIdx.x; i < span; i += kThreads) xs[i] = src(i);
      __syncthreads();
      fir_tile<true>(hp, LdsSamples{xs}, ys, a.up, a.down, a.K, a.Ks, a.tile, base_r, n_valid, n_valid, yrow + k0, false);
    } else {
      __syncthreads();
      fir_tile<false>(hp, src, nullptr, a.up, a.down, a.K, a.Ks, a.tile, base_r, n_valid, n_valid, yrow + k0, false);
    }
  }
  // the packet goes behind the history: cells [ring_pos, ring_pos + P) mod cap, disjoint from the K - 1 cells read above
  for (int i = threadIdx.x; i < P; i += kThreads) {
    int r = ring_pos + i;
    if (r >= a.cap) r -= a.cap;
    ring[r] = pkt[i];
  }
}

int allow_lds(size_t lds) {
  if (lds <= 64 * 1024) return 0;
  static bool allowed_on[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  if (!allowed_on[dev]) {
    if (hipFuncSetAttribute((const void*)resample_kernel<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget) != hipSuccess ||
        hipFuncSetAttribute((const void*)resample_kernel<int16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget) != hipSuccess ||
        hipFuncSetAttribute((const void*)resample_stream_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget) != hipSuccess)
      return -1;
    allowed_on[dev] = true;
  }
  return 0;
}

int ring_cap(const RsPlan& p, int max_packet) { return p.K - 1 + max_packet; }

// outputs that are final after N samples, and the length of the whole output
int64_t emitted(int64_t N, const RsPlan& p) {
  const int64_t v = N * p.up - p.half - 1;
  return v < 0 ? 0 : v / p.down + 1;
}
int64_t out_length(int64_t N, const RsPlan& p) { return (N * p.up + p.down - 1) / p.down; }

int check_streams(const RsPlan& p, int n_streams, int max_packet) {
  if (n_streams < 1 || max_packet < 1) return fail(MI355ASR_EINVAL, "resample streams: n_streams = %d, max_packet = %d", n_streams, max_packet);
  if ((int64_t)max_packet * p.up + (int64_t)p.half + p.tile * (int64_t)p.down >= (int64_t)1 << 30)
    return fail(MI355ASR_EINVAL, "resample streams: max_packet = %d x up = %d does not fit the step's 32-bit arithmetic", max_packet, p.up);
  return 0;
}

int stream_out_cap(const RsPlan& p, int max_packet) {
  // a step: E(N + P) - E(N) <= ceil(P up / down) + 1; a flush: ceil(N up / down) - E(N) <= (half + 1) / down + 2
  const int64_t step = ((int64_t)max_packet * p.up + p.down - 1) / p.down + 1;
  const int64_t flush = (p.half + 1) / p.down + 2;
  return (int)std::max(step, flush);
}

}  // namespace

extern "C" {

int mi355asr_resample_plan(int32_t up, int32_t down, int32_t* taps, int32_t* stride, int32_t* tile, int32_t* table_floats) {
  RsPlan p;
  if (int rc = make_plan(up, down, &p)) return rc;
  if (taps) *taps = p.K;
  if (stride) *stride = p.Ks;
  if (tile) *tile = p.tile;
  if (table_floats) *table_floats = p.hp_floats;
  return 0;
}

int mi355asr_resample(const void* x_dev, int32_t dtype, const int32_t* in_len_dev, int32_t B, int64_t Lpad, int32_t up, int32_t down,
                      const float* filt_dev, float* y_dev, int64_t Opad, void* stream) {
  if (!x_dev || !in_len_dev || !filt_dev || !y_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (dtype != MI355ASR_DT_F32 && dtype != MI355ASR_DT_I16) return fail(MI355ASR_EINVAL, "resample: input dtype %d is neither float32 nor int16", dtype);
  if (B < 1 || B > 65535 || Lpad < 1 || Opad < 1 || Lpad > INT32_MAX)
    return fail(MI355ASR_EINVAL, "resample: need 1 <= B <= 65535, 1 <= Lpad < 2^31, Opad >= 1 (got %d, %lld, %lld)", B, (long long)Lpad, (long long)Opad);
  if ((uintptr_t)filt_dev & 15) return fail(MI355ASR_EINVAL, "resample: the filter table must be 16-byte aligned");
  RsPlan p;
  if (int rc = make_plan(up, down, &p)) return rc;
  const int64_t tiles = (Opad + p.tile - 1) / p.tile;
  // several tiles per workgroup once there are plenty of workgroups: the filter is staged once per workgroup
  int64_t tpw = tiles * B / 2048;
  tpw = std::min<int64_t>(std::max<int64_t>(tpw, 1), 16);
  const int64_t gx = (tiles + tpw - 1) / tpw;
  if (gx > INT32_MAX) return fail(MI355ASR_EINVAL, "resample: Opad = %lld gives too many tiles", (long long)Opad);
  const size_t esz = dtype == MI355ASR_DT_F32 ? 4 : 2;
  RsArgs a{};
  a.x = x_dev; a.in_len = in_len_dev; a.filt = filt_dev; a.y = y_dev; a.Lpad = Lpad; a.Opad = Opad; a.tiles = tiles;
  a.up = up; a.down = down; a.half = p.half; a.K = p.K; a.Ks = p.Ks; a.tile = p.tile; a.hp_floats = p.hp_floats; a.span_cap = p.span_cap;
  a.tiles_per_wg = (int)tpw;
  a.vec_x = !((uintptr_t)x_dev & 15) && (Lpad * esz) % 16 == 0;
  a.vec_y = !((uintptr_t)y_dev & 15) && Opad % 4 == 0;
  if (allow_lds(p.lds) != 0) return fail(MI355ASR_EHIP, "resample: %zu bytes of LDS were refused", p.lds);
  const dim3 grid((unsigned)gx, (unsigned)B), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MI355ASR_DT_F32) {
    if (p.staged) hipLaunchKernelGGL((resample_kernel<float, true>), grid, block, p.lds, s, a);
    else hipLaunchKernelGGL((resample_kernel<float, false>), grid, block, p.lds, s, a);
  } else {
    if (p.staged) hipLaunchKernelGGL((resample_kernel<int16_t, true>), grid, block, p.lds, s, a);
    else hipLaunchKernelGGL((resample_kernel<int16_t, false>), grid, block, p.lds, s, a);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_resample_streams_bytes(int32_t up, int32_t down, int32_t n_streams, int32_t max_packet, size_t* state_bytes, size_t* ws_bytes,
                                    int32_t* out_cap) {
  if (!state_bytes || !ws_bytes || !out_cap) return fail(MI355ASR_EINVAL, "null pointer");
  RsPlan p;
  if (int rc = make_plan(up, down, &p)) return rc;
  if (int rc = check_streams(p, n_streams, max_packet)) return rc;
  *state_bytes = (size_t)n_streams * ring_cap(p, max_packet) * sizeof(float);
  *ws_bytes = (size_t)n_streams * kTableInts * sizeof(int32_t);
  *out_cap = stream_out_cap(p, max_packet);
  return 0;
}

int mi355asr_resample_streams_reset(void* state_dev, int32_t up, int32_t down, int32_t n_streams, int32_t max_packet, const int32_t* slots_host,
                                    int32_t n, void* stream) {
  if (!state_dev) return fail(MI355ASR_EINVAL, "null pointer");
  RsPlan p;
  if (int rc = make_plan(up, down, &p)) return rc;
  if (int rc = check_streams(p, n_streams, max_packet)) return rc;
  const size_t slot_bytes = (size_t)ring_cap(p, max_packet) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (!slots_host) {
    HIP_TRY(hipMemsetAsync(state_dev, 0, slot_bytes * n_streams, s));
    return 0;
  }
  if (n < 1) return fail(MI355ASR_EINVAL, "resample streams: reset of %d slots", n);
  for (int i = 0; i < n; ++i)
    if (slots_host[i] < 0 || slots_host[i] >= n_streams)
      return fail(MI355ASR_EINVAL, "resample streams: slot %d out of range 0 .. %d", slots_host[i], n_streams - 1);
  for (int i = 0; i < n; ++i) HIP_TRY(hipMemsetAsync((char*)state_dev + slot_bytes * slots_host[i], 0, slot_bytes, s));
  return 0;
}

int mi355asr_resample_streams_step(void* state_dev, int32_t up, int32_t down, int32_t n_streams, int32_t max_packet, const float* filt_dev,
                                   const int32_t* slots_host, const int64_t* pos_host, const int32_t* n_in_host, int32_t n, int32_t flush,
                                   const float* x_dev, int32_t Ppad, float* y_dev, int32_t out_cap, int32_t* n_out_host, void* ws_dev,
                                   size_t ws_bytes, void* stream) {
  if (!state_dev || !filt_dev || !slots_host || !pos_host || !y_dev || !n_out_host || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (!flush && (!x_dev || !n_in_host)) return fail(MI355ASR_EINVAL, "resample streams: a step needs packets and their lengths");
  if (((uintptr_t)filt_dev & 15) || ((uintptr_t)state_dev & 3)) return fail(MI355ASR_EINVAL, "resample streams: misaligned filter table or state");
  RsPlan p;
  if (int rc = make_plan(up, down, &p)) return rc;
  if (int rc = check_streams(p, n_streams, max_packet)) return rc;
  if (n < 1 || n > n_streams) return fail(MI355ASR_EINVAL, "resample streams: need 1 <= n <= n_streams (got %d)", n);
  if (out_cap < stream_out_cap(p, max_packet)) return fail(MI355ASR_EINVAL, "resample streams: out_cap = %d < %d", out_cap, stream_out_cap(p, max_packet));
  if (ws_bytes < (size_t)n * kTableInts * sizeof(int32_t)) return fail(MI355ASR_EWORKSPACE, "resample streams: workspace too small: %zu bytes", ws_bytes);
  const int cap = ring_cap(p, max_packet);
  std::vector<int32_t> table((size_t)n * kTableInts, 0);
  {
    std::vector<char> seen((size_t)n_streams, 0);
    for (int i = 0; i < n; ++i) {
      const int sl = slots_host[i];
      if (sl < 0 || sl >= n_streams) return fail(MI355ASR_EINVAL, "resample streams: slot %d out of range 0 .. %d", sl, n_streams - 1);
      if (seen[sl]) return fail(MI355ASR_EINVAL, "resample streams: slot %d is named twice in one step", sl);
      seen[sl] = 1;
      const int64_t N0 = pos_host[i];
      const int P = flush ? 0 : n_in_host[i];
      if (N0 < 0 || P < 0 || P > max_packet || P > Ppad || N0 > (INT64_MAX >> 12))
        return fail(MI355ASR_EINVAL, "resample streams: slot %d: position %lld, packet of %d samples (max_packet %d, row pitch %d)", sl,
                    (long long)N0, P, max_packet, Ppad);
      const int64_t k0 = emitted(N0, p);
      const int64_t k1 = flush ? out_length(N0, p) : emitted(N0 + P, p);
      const int64_t c0 = k0 * p.down + p.half;
      int32_t* t = &table[(size_t)i * kTableInts];
      t[0] = sl; t[1] = P; t[2] = (int32_t)(k1 - k0); t[3] = (int32_t)(N0 % cap);
      t[4] = (int32_t)(c0 / p.up - N0);     // jh of the first output relative to the packet's first sample: -(K - 1) < . <= P
      t[5] = (int32_t)(c0 % p.up);
      n_out_host[i] = t[2];
    }
  }
  hipStream_t s = (hipStream_t)stream;
  // the table comes from pageable host memory: the runtime stages it before the call returns, nothing is waited for
  HIP_TRY(hipMemcpyAsync(ws_dev, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  RsStreamArgs a{};
  a.state = (float*)state_dev; a.table = (const int32_t*)ws_dev; a.x = flush ? nullptr : x_dev; a.filt = filt_dev; a.y = y_dev;
  a.up = up; a.down = down; a.K = p.K; a.Ks = p.Ks; a.tile = p.tile; a.hp_floats = p.hp_floats; a.span_cap = p.span_cap; a.cap = cap;
  a.Ppad = Ppad; a.out_cap = out_cap;
  if (allow_lds(p.lds) != 0) return fail(MI355ASR_EHIP, "resample streams: %zu bytes of LDS were refused", p.lds);
  if (p.staged) hipLaunchKernelGGL(resample_stream_kernel<true>, dim3(n), dim3(kThreads), p.lds, s, a);
  else hipLaunchKernelGGL(resample_stream_kernel<false>, dim3(n), dim3(kThreads), p.lds, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
