// Band-limited resampling at any real ratio, one ratio per row (J. O. Smith's interpolation with a tabulated windowed sinc, as
// resampy 0.2's `kaiser_best` runs it) behind mi355asr_sinc_* of include/mi355asr.h.  librosa.effects.pitch_shift is the time
// stretch followed by this at the ratio 2^(-steps / 12): augment.Pitch.
//
// The table is the right half of the filter, win[0 .. 32768] at NT = 512 entries per zero crossing and 64 zero crossings, built
// on the host in float64 and handed in as fp32 in natural order; table_floats = 32772 floats, the last three repeat win[32768],
// so the neighbour difference of the last entry is 0.  For a row of N samples at ratio r, with scale = min(1, r) and
// step = (int)(scale NT), output t is
//     pos = t (1 / r)  (one float64 product),  n = (int)pos,  frac = scale (pos - n),  o = (int)(frac NT),  eta = frac NT - o
//     left :  sum_{i < min(n + 1,     (32769 - o) / step)}  (win[o + i step] + eta (win[o + i step + 1] - win[o + i step])) x[n - i]
//     right:  the same with frac' = scale - frac, over k < min(N - n - 1, (32769 - o') / step) and x[n + k + 1]
// times r when r < 1.  pos, n, o and eta are float64 or integers (an fp32 position is several table entries off from t = 2^17
// on); eta is rounded to fp32 once, and every weight is one fp32 FMA on the fp32 neighbour difference, every product one fp32
// FMA into ONE accumulator: left wing i = 0, 1, ..., then right wing k = 0, 1, ...  No atomics and nothing that depends on the
// batch: a row is the same bits alone, in any batch and in every run.
//
// sinc_kernel: a workgroup of 1024 threads owns tiles of 1024 consecutive outputs of one row, one output per thread.  Per tile the
// input samples its outputs touch (at most 1023 / r + 2 wing + 2, 4 605 at r = 0.25) are staged in LDS, zero outside [0, N): samples
// at or past a row's length are never read.  LDS_TABLE: the whole table (128 KiB) lies in LDS beside them, staged once per
// workgroup with 16-byte loads; a thread's two neighbours come from one ds_read2_b32.  Lanes are outputs, so at one tap the
// wave's addresses are o + i step with o spread over [0, step): distinct banks up to chance, a few ways of conflict.  One
// workgroup per CU (150 KiB), 4 waves per SIMD.  !LDS_TABLE reads the table through the caches instead (it stays in L2): the
// same chain, the same bits; DESIGN.md section 22 has what both measured.  Row, column and sample offsets are 64-bit.
#include "model.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kTile = 1024;               // outputs per tile: one per thread
constexpr int kNT = 512;                  // table entries per zero crossing
constexpr int kTabN = 64 * kNT + 1;       // 32 769 entries
constexpr int kTabFloats = 32772;         // padded to 16 bytes with copies of the last entry
constexpr double kRatioMin = 0.25, kRatioMax = 4.0;
constexpr int kSpanCap = 4672;            // >= 1023 / kRatioMin + 1 + 2 (kTabN / (kNT kRatioMin)), a multiple of 4

struct SincRow {
  double inv, scale;                      // 1 / r, min(1, r)
  int64_t N, valid, cols, off;            // samples; outputs that are computed; columns written (zeros from `valid`); first column
  float gain;                             // r when r < 1, else 1
  int32_t step, K, pad_;                  // (int)(scale NT); taps per wing at most: kTabN / step
};

struct SincArgs {
  const float* x;         // [B, Lpad]
  const SincRow* rows;    // [B]
  const float* table;     // [kTabFloats]
  float* y;               // [B, Opad]
  int64_t Lpad, Opad;
  int tiles_per_wg;
};

int wing_of(double r, int* step_out) {
  const double scale = r < 1.0 ? r : 1.0;
  const int step = (int)(scale * kNT);
  if (step_out) *step_out = step;
  return kTabN / step;
}

bool ratio_ok(double r) { return std::isfinite(r) && r >= kRatioMin && r <= kRatioMax; }

template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void sinc_kernel(SincArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  const float* tab = LDS_TABLE ? lds + kSpanCap : a.table;
  const int b = blockIdx.y;
  const SincRow r = a.rows[b];
  const int64_t tiles = (r.cols + kTile - 1) / kTile;
  const int64_t t_begin = (int64_t)blockIdx.x * a.tiles_per_wg;
  const int64_t t_end = t_begin + a.tiles_per_wg < tiles ? t_begin + a.tiles_per_wg : tiles;
  const float* x = a.x + (int64_t)b * a.Lpad;
  float* y = a.y + (int64_t)b * a.Opad + r.off;
  bool table_in = false;
  for (int64_t tt = t_begin; tt < t_end; ++tt) {
    const int64_t k0 = tt * kTile;
    const int64_t t = k0 + threadIdx.x;
    if (k0 >= r.valid) {                            // nothing of the row here: zeros
      if (t < r.cols) y[t] = 0.0f;
      continue;
    }
    if (LDS_TABLE && !table_in) {
      float* tl = lds + kSpanCap;
      for (int i = threadIdx.x * 4; i < kTabFloats; i += kThreads * 4)
        *reinterpret_cast<float4*>(tl + i) = *reinterpret_cast<const float4*>(a.table + i);
      table_in = true;
    }
    // the samples the tile's outputs touch: n runs over [n_lo, n_hi] (t inv is monotonic), a wing reaches K - 1 to the left of n
    // and K to the right
    const int64_t t_last = (k0 + kTile < r.valid ? k0 + kTile : r.valid) - 1;
    const int64_t n_lo = (int64_t)((double)k0 * r.inv), n_hi = (int64_t)((double)t_last * r.inv);
    const int64_t j_lo = n_lo - (r.K - 1);
    const int64_t want = n_hi + r.K - j_lo + 1;
    const int span = want < kSpanCap ? (int)want : kSpanCap;
    __syncthreads();                                // the previous tile's readers of xs are done
    for (int i = threadIdx.x; i < span; i += kThreads) {
      const int64_t j = j_lo + i;
      xs[i] = (j >= 0 && j < r.N) ? x[j] : 0.0f;
    }
    __syncthreads();
    if (t >= r.cols) continue;
    float acc = 0.0f;
    if (t < r.valid) {
      const double pos = (double)t * r.inv;
      const int64_t n = (int64_t)pos;
      const int base = (int)(n - j_lo);             // xs[base] = x[n]; K - 1 <= base
      double frac = r.scale * (pos - (double)n);
      {
        const double idx = frac * kNT;
        const int o = (int)idx;
        const float eta = (float)(idx - (double)o);
        int cnt = (kTabN - o) / r.step;
        if (n + 1 < cnt) cnt = (int)(n + 1);
        if (base + 1 < cnt) cnt = base + 1;         // never: the span starts K - 1 before n_lo
        const float* w = tab + o;
        const float* xp = xs + base;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
          const float w0 = w[0], w1 = w[1];
          acc = __builtin_fmaf(__builtin_fmaf(eta, w1 - w0, w0), xp[-i], acc);
          w += r.step;
        }
      }
      frac = r.scale - frac;
      {
        const double idx = frac * kNT;
        const int o = (int)idx;
        const float eta = (float)(idx - (double)o);
        int cnt = (kTabN - o) / r.step;
        if (r.N - n - 1 < cnt) cnt = (int)(r.N - n - 1);
        if (span - base - 1 < cnt) cnt = span - base - 1;   // never, unless the span was cut at kSpanCap
        const float* w = tab + o;
        const float* xp = xs + base + 1;
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
          const float w0 = w[0], w1 = w[1];
          acc = __builtin_fmaf(__builtin_fmaf(eta, w1 - w0, w0), xp[k], acc);
          w += r.step;
        }
      }
      acc *= r.gain;
    }
    y[t] = acc;
  }
}

constexpr size_t kLdsTable = (size_t)(kSpanCap + kTabFloats) * sizeof(float);
constexpr size_t kLdsPlain = (size_t)kSpanCap * sizeof(float);

int allow_lds() {
  static bool allowed_on[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  if (!allowed_on[dev]) {
    if (hipFuncSetAttribute((const void*)sinc_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsTable) != hipSuccess) return -1;
    allowed_on[dev] = true;
  }
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_sinc_plan(double ratio, int32_t* tile, int32_t* wing, int32_t* table_floats, double* ratio_min, double* ratio_max) {
  if (tile) *tile = kTile;
  if (table_floats) *table_floats = kTabFloats;
  if (ratio_min) *ratio_min = kRatioMin;
  if (ratio_max) *ratio_max = kRatioMax;
  if (!ratio_ok(ratio)) return fail(MI355ASR_EINVAL, "sinc resample: the ratio %g is outside %g .. %g", ratio, kRatioMin, kRatioMax);
  if (wing) *wing = wing_of(ratio, nullptr);
  return 0;
}

int mi355asr_sinc_workspace_bytes(int32_t B, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535) return fail(MI355ASR_EINVAL, "sinc resample: need 1 <= B <= 65535 (got %d)", B);
  *ws_bytes = (size_t)B * sizeof(SincRow);
  return 0;
}

int mi355asr_sinc_resample(const float* x_dev, int32_t B, int64_t Lpad, const double* ratios_host, const int64_t* len_host,
                           const int64_t* out_len_host, const int64_t* off_host, int64_t* valid_host, const float* table_dev,
                           int32_t table_mode, float* y_dev, int64_t Opad, void* ws_dev, size_t ws_bytes, void* stream) {
  if (!x_dev || !ratios_host || !len_host || !table_dev || !y_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535 || Lpad < 1 || Opad < 1)
    return fail(MI355ASR_EINVAL, "sinc resample: need 1 <= B <= 65535, Lpad >= 1, Opad >= 1 (got %d, %lld, %lld)", B, (long long)Lpad, (long long)Opad);
  if (table_mode != 0 && table_mode != 1) return fail(MI355ASR_EINVAL, "sinc resample: table_mode %d is neither 0 (LDS) nor 1 (caches)", table_mode);
  if (((uintptr_t)table_dev & 15) || ((uintptr_t)ws_dev & 7)) return fail(MI355ASR_EINVAL, "sinc resample: misaligned table or workspace");
  if (ws_bytes < (size_t)B * sizeof(SincRow)) return fail(MI355ASR_EWORKSPACE, "sinc resample: workspace too small: %zu bytes", ws_bytes);
  std::vector<SincRow> rows((size_t)B);
  int64_t tiles_max = 0, tiles_all = 0;
  for (int b = 0; b < B; ++b) {
    const double r = ratios_host[b];
    const int64_t N = len_host[b];
    if (!ratio_ok(r)) return fail(MI355ASR_EINVAL, "sinc resample: row %d: the ratio %g is outside %g .. %g", b, r, kRatioMin, kRatioMax);
    if (N < 0 || N > Lpad) return fail(MI355ASR_EINVAL, "sinc resample: row %d: %lld samples in a row of %lld", b, (long long)N, (long long)Lpad);
    if (N > ((int64_t)1 << 40)) return fail(MI355ASR_EINVAL, "sinc resample: row %d: %lld samples are more than 2^40", b, (long long)N);
    const int64_t out_len = out_len_host ? out_len_host[b] : (int64_t)std::ceil((double)N * r);
    const int64_t off = off_host ? off_host[b] : 0;
    if (out_len < 0 || off < 0 || out_len > Opad || off > Opad - out_len)
      return fail(MI355ASR_EINVAL, "sinc resample: row %d: %lld outputs at column %lld of %lld", b, (long long)out_len, (long long)off, (long long)Opad);
    SincRow& w = rows[b];
    w.inv = 1.0 / r;
    w.scale = r < 1.0 ? r : 1.0;
    w.gain = r < 1.0 ? (float)r : 1.0f;
    w.K = wing_of(r, &w.step);
    w.pad_ = 0;
    w.N = N;
    const int64_t whole = (int64_t)std::floor((double)N * r);
    w.valid = whole < out_len ? whole : out_len;
    w.cols = off_host ? out_len : Opad;           // without offsets the row is zero-filled to Opad
    w.off = off;
    if (valid_host) valid_host[b] = w.valid;
    const int64_t tiles = (w.cols + kTile - 1) / kTile;
    tiles_max = std::max(tiles_max, tiles);
    tiles_all += tiles;
  }
  if (tiles_max == 0) return 0;                   // offsets given and every row empty: nothing to write
  hipStream_t s = (hipStream_t)stream;
  // the rows come from pageable host memory: the runtime stages them before the call returns, nothing is waited for
  HIP_TRY(hipMemcpyAsync(ws_dev, rows.data(), rows.size() * sizeof(SincRow), hipMemcpyHostToDevice, s));
  // several tiles per workgroup once there are plenty of workgroups: the table is staged once per workgroup
  const int64_t tpw = std::min<int64_t>(std::max<int64_t>(tiles_all / 1024, 1), 8);
  const int64_t gx = (tiles_max + tpw - 1) / tpw;
  if (gx > INT32_MAX) return fail(MI355ASR_EINVAL, "sinc resample: Opad = %lld gives too many tiles", (long long)Opad);
  SincArgs a{};
  a.x = x_dev; a.rows = (const SincRow*)ws_dev; a.table = table_dev; a.y = y_dev; a.Lpad = Lpad; a.Opad = Opad; a.tiles_per_wg = (int)tpw;
  const dim3 grid((unsigned)gx, (unsigned)B), block(kThreads);
  if (table_mode == 0) {
    if (allow_lds() != 0) return fail(MI355ASR_EHIP, "sinc resample: %zu bytes of LDS were refused", kLdsTable);
    hipLaunchKernelGGL(sinc_kernel<true>, grid, block, kLdsTable, s, a);
  } else {
    hipLaunchKernelGGL(sinc_kernel<false>, grid, block, kLdsPlain, s, a);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
