// Recursive (IIR) filtering of a ragged batch, and SignalMask, behind mi355asr_sos_ragged and mi355asr_mask_zone of
// include/mi355asr.h: scipy.signal.sosfilt / sosfiltfilt per row (the reference's SignalHz is filtfilt of a 3rd-order Butterworth
// band-stop) with every recursion in float64 on second-order sections.  DESIGN.md section 21.
//
// A row is cut into chunks of kChunk samples at fixed positions of the (odd-extended) row; one lane owns one chunk.  A biquad
// in direct form II transposed is  y = b0 x + z1,  z1' = b1 x - a1 y + z2,  z2' = b2 x - a2 y : per sample a dependent chain of
// two FMAs, so all parallelism is rows x chunks.  One section at a time, three steps:
//   A  sos_pass_kernel (zero run):  every chunk runs the section from the ZERO state and keeps the final state p[c];
//   B  sos_scan_kernel:             one lane per row walks the chunks in filter order, s[c + 1] = M s[c] + p[c], where M is the
//                                   2 x 2 transition of kChunk steps obtained by RUNNING the recursion on the two unit states
//                                   (never by matrix powers: DESIGN.md section 21 has the numbers); s[0] is zi, and the state
//                                   after the last chunk goes to zf;
//   C  sos_pass_kernel (true run):  every chunk runs the section again from its true state s[c] and writes the output.
// Step C of a section and step A of the next one share a launch (the lane runs the next section from zero on the samples it
// has just produced), except where the direction turns in sosfiltfilt.  The 64 lanes of a workgroup own 64 consecutive chunks;
// their samples go through LDS 16 per chunk at a time (rows of 17 doubles: conflict-free 8-byte reads), so global loads and
// stores are runs of 128 bytes.  The intermediate signal lives in ONE float64 buffer of the workspace, updated in place (a
// workgroup reads and writes its own positions only).  Nothing depends on the batch around a row or on timing: no atomics,
// a row is the same bits in every run, in every batch and at every batch position.
//
// mask_zone_kernel: SignalMask.augment element by element, with the reference's own float64 expressions.
#include "common.h"
#include "model.h"

namespace {

constexpr int kChunk = 128;                             // samples per lane; exported by mi355asr_sos_chunk
constexpr int kSub = 16;                                // samples per chunk staged at a time
constexpr int kLanes = 64;                              // chunks per workgroup (one wave)
constexpr int kTile = kLanes * kChunk;                  // positions per workgroup
constexpr int kRowLds = kSub + 1;
constexpr int kScan = 1024;                             // chunk states the scan stages at a time
constexpr int kMaxS = 8;
constexpr int kCoef = 8;                                // doubles per section of the device table: b0 b1 b2 a1 a2 zi0 zi1 -
constexpr int kMaxPad = 1024;                           // the longest edge of sosfiltfilt; the workspace is sized for it

struct SosArgs {
  const void* x;          // [B, Lpad] float or int16
  const int32_t* len;     // [B]
  const double* coef;     // [B or 1, S, kCoef]
  double* buf;            // [B, Next] the intermediate signal
  double* p;              // [B, ncp, 2] zero-run final states of the section in `sb`
  double* sin;            // [B, ncp, 2] true initial states of the section in `sa`
  double* y0;             // [B] first sample of the pass (what zi is scaled by in mode 1)
  const double* zi;       // [B, S, 2] or null (mode 0)
  double* zf;             // [B, S, 2] or null (mode 0)
  const double* noise;    // [B, Npad] or null
  float* y;               // [B, Opad]
  double noise_scale;
  int64_t Lpad, Next, Opad, Npad, ncp;
  int coef_stride;        // 0: shared
  int S, mode, padlen, i16;
  // the launch
  int src_x;              // read the (extended) input, not buf
  int sa, sb;             // sections of the true run and of the zero run (-1: none)
  int rev;                // 1: the backward pass of sosfiltfilt
  int dst;                // 0: none, 1: buf, 2: y (finish: noise, quantise, float32)
  int quantise;
  int first;              // scan: the first section of its pass
};

struct RowGeom {
  int64_t L, N;           // samples, filtered positions (0: the row is copied through or empty)
  int off;                // position of sample 0
};

__device__ __forceinline__ RowGeom row_geom(const SosArgs& a, int b) {
  RowGeom g;
  const int64_t l = a.len[b];
  g.L = l > 0 ? (l < a.Lpad ? l : a.Lpad) : 0;
  g.off = a.mode ? a.padlen : 0;
  g.N = a.mode ? (g.L > a.padlen ? g.L + 2 * (int64_t)a.padlen : 0) : g.L;
  return g;
}

__device__ __forceinline__ double sample(const SosArgs& a, int b, int64_t n) {
  if (a.i16) return (double)reinterpret_cast<const int16_t*>(a.x)[(int64_t)b * a.Lpad + n] * (1.0 / 32768.0);
  return (double)reinterpret_cast<const float*>(a.x)[(int64_t)b * a.Lpad + n];
}

// position pos of the odd extension of the row: 2 x[0] - x[padlen .. 1], the row, 2 x[L - 1] - x[L - 2 .. L - 1 - padlen]
__device__ __forceinline__ double extended(const SosArgs& a, int b, const RowGeom& g, int64_t pos) {
  const int64_t n = pos - g.off;
  if (n < 0) return 2.0 * sample(a, b, 0) - sample(a, b, -n);
  if (n >= g.L) return 2.0 * sample(a, b, g.L - 1) - sample(a, b, 2 * (g.L - 1) - n);
  return sample(a, b, n);
}

__device__ __forceinline__ double quantise16(double v) {
  v = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
  return trunc(v * 32768.0) * (1.0 / 32768.0) + 0.0;    // + 0.0: the reference's integer conversion has no negative zero
}

__global__ __launch_bounds__(kLanes) void sos_pass_kernel(SosArgs a) {
  __shared__ double tile[kLanes * kRowLds];
  const int b = blockIdx.y, lane = threadIdx.x;
  const RowGeom g = row_geom(a, b);
  const int64_t T0 = (int64_t)blockIdx.x * kTile;
  if (a.dst != 2 && T0 >= g.N) return;                  // nothing of the row here
  if (a.dst == 2 && T0 >= g.N) {                        // past the filtered positions: a copied row, or zeros
    float* yrow = a.y + (int64_t)b * a.Opad;
    for (int i = lane; i < kTile; i += kLanes) {
      const int64_t o = T0 + i - g.off;
      if (o < 0 || o >= a.Opad) continue;
      float r = 0.0f;
      if (g.N == 0 && o < g.L) {
        double v = sample(a, b, o);
        if (a.noise) v = __dadd_rn(v, __dmul_rn(a.noise_scale, a.noise[(int64_t)b * a.Npad + o]));
        if (a.quantise) v = quantise16(v);
        r = (float)v;
      }
      yrow[o] = r;
    }
    return;
  }
  const int64_t c = (int64_t)blockIdx.x * kLanes + lane; // this lane's chunk
  const int64_t c0 = c * kChunk;
  const int nc = g.N - c0 >= kChunk ? kChunk : (g.N > c0 ? (int)(g.N - c0) : 0);   // its samples
  double b0 = 0, b1 = 0, b2 = 0, a1 = 0, a2 = 0, z1 = 0, z2 = 0;
  double e0 = 0, e1 = 0, e2 = 0, f1 = 0, f2 = 0, w1 = 0, w2 = 0;
  const double* cf = a.coef + (int64_t)b * a.coef_stride;
  if (a.sa >= 0) {
    const double* q = cf + a.sa * kCoef;
    b0 = q[0]; b1 = q[1]; b2 = q[2]; a1 = q[3]; a2 = q[4];
    if (nc > 0) {
      const double* s = a.sin + ((int64_t)b * a.ncp + c) * 2;
      z1 = s[0]; z2 = s[1];
    }
  }
  if (a.sb >= 0) {
    const double* q = cf + a.sb * kCoef;
    e0 = q[0]; e1 = q[1]; e2 = q[2]; f1 = q[3]; f2 = q[4];
  }
  const double* brow = a.buf + (int64_t)b * a.Next;
  double* wrow = a.buf + (int64_t)b * a.Next;
  float* yrow = a.y + (int64_t)b * a.Opad;
  double* mine = tile + lane * kRowLds;
  for (int step = 0; step < kChunk / kSub; ++step) {
    const int sub = a.rev ? kChunk / kSub - 1 - step : step;
    // stage 16 samples of each of the 64 chunks: 16 lanes read 128 consecutive bytes
#pragma unroll
    for (int j = 0; j < kSub; ++j) {
      const int e = j * kLanes + lane, ch = e >> 4, of = e & (kSub - 1);
      const int64_t pos = T0 + (int64_t)ch * kChunk + sub * kSub + of;
      double v = 0.0;
      if (pos < g.N) v = a.src_x ? extended(a, b, g, pos) : brow[pos];
      tile[ch * kRowLds + of] = v;
    }
    __syncthreads();
    const int cnt = nc - sub * kSub;                    // samples of this lane's chunk in the piece: all 16 when >= 16
    double xr[kSub];
#pragma unroll
    for (int k = 0; k < kSub; ++k) xr[k] = mine[a.rev ? kSub - 1 - k : k];
    if (a.sa >= 0) {
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        if ((a.rev ? kSub - 1 - k : k) < cnt) {
          const double v = xr[k];
          const double yv = __builtin_fma(b0, v, z1);
          z1 = __builtin_fma(-a1, yv, __builtin_fma(b1, v, z2));
          z2 = __builtin_fma(-a2, yv, b2 * v);
          xr[k] = yv;
        }
      }
#pragma unroll
      for (int k = 0; k < kSub; ++k) mine[a.rev ? kSub - 1 - k : k] = xr[k];
    }
    if (a.sb >= 0) {
#pragma unroll
      for (int k = 0; k < kSub; ++k) {
        if ((a.rev ? kSub - 1 - k : k) < cnt) {
          const double v = xr[k];
          const double yv = __builtin_fma(e0, v, w1);
          w1 = __builtin_fma(-f1, yv, __builtin_fma(e1, v, w2));
          w2 = __builtin_fma(-f2, yv, e2 * v);
        }
      }
    }
    __syncthreads();
    if (a.dst) {
#pragma unroll
      for (int j = 0; j < kSub; ++j) {
        const int e = j * kLanes + lane, ch = e >> 4, of = e & (kSub - 1);
        const int64_t pos = T0 + (int64_t)ch * kChunk + sub * kSub + of;
        double v = tile[ch * kRowLds + of];
        if (a.dst == 1) {
          if (pos < g.N) wrow[pos] = v;
        } else {
          const int64_t o = pos - g.off;
          if (o >= 0 && o < a.Opad) {
            float r = 0.0f;
            if (o < g.L && pos < g.N) {
              if (a.noise) v = __dadd_rn(v, __dmul_rn(a.noise_scale, a.noise[(int64_t)b * a.Npad + o]));
              if (a.quantise) v = quantise16(v);
              r = (float)v;
            }
            yrow[o] = r;
          }
        }
      }
      __syncthreads();                                  // the tile is staged again
    }
  }
  if (a.sb >= 0 && nc > 0) {
    double* pp = a.p + ((int64_t)b * a.ncp + c) * 2;
    pp[0] = w1; pp[1] = w2;
  }
}

// one workgroup per row: the true initial state of every chunk of section `sa`, in filter order
__global__ __launch_bounds__(kLanes) void sos_scan_kernel(SosArgs a) {
  __shared__ double sp[2 * kScan];
  const int b = blockIdx.x, lane = threadIdx.x;
  const RowGeom g = row_geom(a, b);
  const double* q = a.coef + (int64_t)b * a.coef_stride + a.sa * kCoef;
  const double a1 = q[3], a2 = q[4];
  double s0 = 0.0, s1 = 0.0;
  if (a.mode) {
    if (g.N == 0) return;                               // copied through or empty: no state
    double first = 0.0;
    if (a.first) {
      first = a.rev ? a.buf[(int64_t)b * a.Next + g.N - 1] : extended(a, b, g, 0);
      if (lane == 0) a.y0[b] = first;
    } else {
      first = a.y0[b];
    }
    s0 = q[5] * first; s1 = q[6] * first;
  } else if (a.zi) {
    s0 = a.zi[((int64_t)b * a.S + a.sa) * 2]; s1 = a.zi[((int64_t)b * a.S + a.sa) * 2 + 1];
  }
  const int64_t nch = (g.N + kChunk - 1) / kChunk;
  if (nch > 0) {
    // the transition of r steps (the short chunk) and of kChunk steps, by running the recursion on the unit states
    const int r = (int)(g.N - (nch - 1) * kChunk);
    double u1 = 1.0, u2 = 0.0, v1 = 0.0, v2 = 1.0;
    double P00 = 1, P01 = 0, P10 = 0, P11 = 1;
    for (int k = 1; k <= kChunk; ++k) {
      const double yu = u1, yv = v1;
      u1 = __builtin_fma(-a1, yu, u2); u2 = -a2 * yu;
      v1 = __builtin_fma(-a1, yv, v2); v2 = -a2 * yv;
      if (k == r) { P00 = u1; P10 = u2; P01 = v1; P11 = v2; }
    }
    const double M00 = u1, M10 = u2, M01 = v1, M11 = v2;
    const double* prow = a.p + (int64_t)b * a.ncp * 2;
    double* srow = a.sin + (int64_t)b * a.ncp * 2;
    // kScan chunks at a time: their zero-run states staged in LDS (whole lines), the walk itself on lane 0 alone -- every step
    // needs the one before it -- leaving each chunk's initial state in the slot its zero-run state came from
    const int64_t kpart = a.rev ? 0 : nch - 1;          // the step that crosses the short chunk
    for (int64_t k0 = 0; k0 < nch; k0 += kScan) {
      const int cnt = nch - k0 < kScan ? (int)(nch - k0) : kScan;
      for (int i = lane; i < cnt; i += kLanes) {        // step k of the walk is chunk k, or nch - 1 - k backward
        const int64_t ch = a.rev ? nch - 1 - (k0 + i) : k0 + i;
        sp[2 * i] = prow[2 * ch]; sp[2 * i + 1] = prow[2 * ch + 1];
      }
      __syncthreads();
      if (lane == 0) {
        for (int i = 0; i < cnt; ++i) {
          const double q0 = sp[2 * i], q1 = sp[2 * i + 1];
          sp[2 * i] = s0; sp[2 * i + 1] = s1;
          double n0, n1;
          if (k0 + i == kpart) {
            n0 = __builtin_fma(P00, s0, __builtin_fma(P01, s1, q0));
            n1 = __builtin_fma(P10, s0, __builtin_fma(P11, s1, q1));
          } else {
            n0 = __builtin_fma(M00, s0, __builtin_fma(M01, s1, q0));
            n1 = __builtin_fma(M10, s0, __builtin_fma(M11, s1, q1));
          }
          s0 = n0; s1 = n1;
        }
      }
      __syncthreads();
      for (int i = lane; i < cnt; i += kLanes) {
        const int64_t ch = a.rev ? nch - 1 - (k0 + i) : k0 + i;
        srow[2 * ch] = sp[2 * i]; srow[2 * ch + 1] = sp[2 * i + 1];
      }
      __syncthreads();
    }
  }
  if (!a.mode && a.zf && lane == 0) {
    a.zf[((int64_t)b * a.S + a.sa) * 2] = s0; a.zf[((int64_t)b * a.S + a.sa) * 2 + 1] = s1;
  }
}

// ---- SignalMask ---------------------------------------------------------------------------------------------------------------------
struct MaskArgs {
  const float* x;         // [B, Lpad]
  const int32_t* len;     // [B]
  const double* u;        // [B, Upad]
  float* y;               // [B, Lpad]
  int64_t Lpad, Upad;
  double zone_lo, zone_hi, mask_ratio;
  int with_noise, quantise;
};

__global__ __launch_bounds__(256) void mask_zone_kernel(MaskArgs a) {
  const int b = blockIdx.y;
  const int64_t l = a.len[b];
  const int64_t L = l > 0 ? (l < a.Lpad ? l : a.Lpad) : 0;
  const int64_t s = (int64_t)((double)L * a.zone_lo), e = (int64_t)((double)L * a.zone_hi);
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.Lpad) return;
  float r = 0.0f;
  if (n < L) {
    double v = (double)a.x[(int64_t)b * a.Lpad + n];
    if (n >= s && n < e && n < L && n - s < a.Upad) {
      const double u = a.u[(int64_t)b * a.Upad + (n - s)];
      const double mask = u < a.mask_ratio ? 0.0 : 1.0;
      v = __dmul_rn(v, mask);
      if (a.with_noise) v = __dadd_rn(v, __dmul_rn(u, mask == 0.0 ? 1.0 : 0.0));
    }
    if (a.quantise) v = quantise16(v);
    r = (float)v;
  }
  a.y[(int64_t)b * a.Lpad + n] = r;
}

struct SosPlan {
  int64_t Next, ncp;
  size_t o_buf, o_p, o_sin, o_coef, o_y0, total;
};

int sos_plan(int32_t B, int64_t Lpad, int32_t S, int32_t mode, int32_t padlen, SosPlan* pl) {
  if (B < 1 || B > 65535 || Lpad < 1 || Lpad > INT32_MAX - 4 * (int64_t)kMaxPad)
    return fail(MI355ASR_EINVAL, "sos: need 1 <= B <= 65535 and 1 <= Lpad < 2^31 - 2^22 (got %d, %lld)", B, (long long)Lpad);
  if (S < 1 || S > kMaxS) return fail(MI355ASR_EINVAL, "sos: %d sections, outside 1 .. %d", S, kMaxS);
  if (mode != 0 && mode != 1) return fail(MI355ASR_EINVAL, "sos: mode %d is neither 0 (sosfilt) nor 1 (sosfiltfilt)", mode);
  if (mode == 1 && (padlen < 0 || padlen > kMaxPad)) return fail(MI355ASR_EINVAL, "sos: padlen = %d is outside 0 .. %d", padlen, kMaxPad);
  const int64_t ext = Lpad + (mode ? 2 * (int64_t)padlen : 0);
  pl->Next = (ext + 15) & ~(int64_t)15;
  pl->ncp = (ext + kChunk - 1) / kChunk;
  size_t o = 0;
  pl->o_buf = o; o += (size_t)B * pl->Next * sizeof(double);
  pl->o_p = o; o += (size_t)B * pl->ncp * 2 * sizeof(double);
  pl->o_sin = o; o += (size_t)B * pl->ncp * 2 * sizeof(double);
  pl->o_coef = o; o += (size_t)B * S * kCoef * sizeof(double);
  pl->o_y0 = o; o += (size_t)B * sizeof(double);
  pl->total = o;
  return 0;
}

}  // namespace

extern "C" {

int32_t mi355asr_sos_chunk(void) { return kChunk; }

int mi355asr_sos_workspace_bytes(int32_t B, int64_t Lpad, int32_t S, int32_t mode, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  SosPlan pl;
  if (int rc = sos_plan(B, Lpad, S, mode, kMaxPad, &pl)) return rc;
  *ws_bytes = pl.total;
  return 0;
}

int mi355asr_sos_ragged(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad, const double* sos_dev,
                        int32_t S, int32_t shared, int32_t mode, int32_t padlen, const double* zi_dev, double* zf_dev,
                        const double* noise_dev, int64_t Npad, double noise_scale, int32_t quantise, float* y_dev, int64_t Opad,
                        void* ws_dev, size_t ws_bytes, void* stream) {
  if (!x_dev || !len_dev || !sos_dev || !y_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (dtype != MI355ASR_DT_F32 && dtype != MI355ASR_DT_I16) return fail(MI355ASR_EINVAL, "sos: input dtype %d is neither float32 nor int16", dtype);
  SosPlan pl;
  if (int rc = sos_plan(B, Lpad, S, mode, padlen, &pl)) return rc;
  if (Opad < 1 || Opad > INT32_MAX) return fail(MI355ASR_EINVAL, "sos: Opad = %lld is outside 1 .. 2^31 - 1", (long long)Opad);
  if (noise_dev && Npad < Lpad) return fail(MI355ASR_EINVAL, "sos: noise of %lld columns does not cover Lpad = %lld", (long long)Npad, (long long)Lpad);
  if (mode == 1 && (zi_dev || zf_dev)) return fail(MI355ASR_EINVAL, "sos: mode 1 (sosfiltfilt) sets its own states: zi_dev and zf_dev must be null");
  if ((uintptr_t)ws_dev & 15) return fail(MI355ASR_EINVAL, "sos: the workspace must be 16-byte aligned");
  SosPlan need;
  if (int rc = sos_plan(B, Lpad, S, mode, kMaxPad, &need)) return rc;
  if (ws_bytes < need.total) return fail(MI355ASR_EWORKSPACE, "sos: workspace too small: %zu bytes, need %zu", ws_bytes, need.total);
  hipStream_t s = (hipStream_t)stream;
  // the sections are read back once: a0 must be 1 (nothing is divided on the device), and sosfilt_zi is computed here
  const int nf = shared ? 1 : B;
  std::vector<double> sos((size_t)nf * S * 6), table((size_t)nf * S * kCoef, 0.0);
  HIP_TRY(hipMemcpyAsync(sos.data(), sos_dev, sos.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int f = 0; f < nf; ++f) {
    double scale = 1.0;
    for (int k = 0; k < S; ++k) {
      const double* c = &sos[((size_t)f * S + k) * 6];
      double* t = &table[((size_t)f * S + k) * kCoef];
      if (!(c[3] == 1.0)) return fail(MI355ASR_EINVAL, "sos: filter %d section %d has a0 = %g: the sections must be normalised to a0 = 1", f, k, c[3]);
      t[0] = c[0]; t[1] = c[1]; t[2] = c[2]; t[3] = c[4]; t[4] = c[5];
      // scipy.signal.sosfilt_zi: lfilter_zi of the section times the DC gain of the sections before it
      const double B0 = c[1] - c[4] * c[0], B1 = c[2] - c[5] * c[0];
      const double z0 = (B0 + B1) / (1.0 + c[4] + c[5]);
      t[5] = scale * z0;
      t[6] = scale * ((1.0 + c[4]) * z0 - B0);
      scale *= (c[0] + c[1] + c[2]) / (1.0 + c[4] + c[5]);
    }
  }
  char* ws = (char*)ws_dev;
  // pageable host memory: the runtime stages the table before the call returns
  HIP_TRY(hipMemcpyAsync(ws + pl.o_coef, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SosArgs a{};
  a.x = x_dev; a.len = len_dev; a.coef = (const double*)(ws + pl.o_coef); a.buf = (double*)(ws + pl.o_buf);
  a.p = (double*)(ws + pl.o_p); a.sin = (double*)(ws + pl.o_sin); a.y0 = (double*)(ws + pl.o_y0);
  a.zi = zi_dev; a.zf = zf_dev; a.noise = noise_dev; a.y = y_dev; a.noise_scale = noise_scale;
  a.Lpad = Lpad; a.Next = pl.Next; a.Opad = Opad; a.Npad = Npad; a.ncp = pl.ncp;
  a.coef_stride = shared ? 0 : S * kCoef;
  a.S = S; a.mode = mode; a.padlen = mode ? padlen : 0; a.i16 = dtype == MI355ASR_DT_I16; a.quantise = quantise != 0;
  const int64_t off = a.padlen;
  const int64_t span = std::max<int64_t>(Lpad + 2 * off, Opad + off);
  const dim3 grid((unsigned)((span + kTile - 1) / kTile), (unsigned)B), block(kLanes);
  auto pass = [&](int src_x, int sa, int sb, int rev, int dst) {
    SosArgs k = a;
    k.src_x = src_x; k.sa = sa; k.sb = sb; k.rev = rev; k.dst = dst;
    hipLaunchKernelGGL(sos_pass_kernel, grid, block, 0, s, k);
  };
  auto scan = [&](int sa, int rev, int first) {
    SosArgs k = a;
    k.sa = sa; k.rev = rev; k.first = first;
    hipLaunchKernelGGL(sos_scan_kernel, dim3((unsigned)B), block, 0, s, k);
  };
  for (int dir = 0; dir <= mode; ++dir) {
    const bool last_pass = dir == mode;
    pass(dir == 0, -1, 0, dir, 0);                      // zero run of the pass's first section
    for (int k = 0; k < S; ++k) {
      scan(k, dir, k == 0);
      const bool last = k == S - 1;
      pass(dir == 0 && k == 0, k, last ? -1 : k + 1, dir, last && last_pass ? 2 : 1);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_mask_zone(const float* x_dev, const int32_t* len_dev, const double* u_dev, int32_t B, int64_t Lpad, int64_t Upad,
                       double zone_lo, double zone_hi, double mask_ratio, int32_t with_noise, int32_t quantise, float* y_dev,
                       void* stream) {
  if (!x_dev || !len_dev || !u_dev || !y_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (B < 1 || B > 65535 || Lpad < 1 || Lpad > INT32_MAX || Upad < 1)
    return fail(MI355ASR_EINVAL, "mask: need 1 <= B <= 65535, 1 <= Lpad < 2^31, Upad >= 1 (got %d, %lld, %lld)", B, (long long)Lpad, (long long)Upad);
  if (!(zone_lo >= 0.0 && zone_lo <= 1.0) || !(zone_hi >= 0.0 && zone_hi <= 1.0))
    return fail(MI355ASR_EINVAL, "mask: the zone (%g, %g) must lie within [0, 1]", zone_lo, zone_hi);
  MaskArgs a{};
  a.x = x_dev; a.len = len_dev; a.u = u_dev; a.y = y_dev; a.Lpad = Lpad; a.Upad = Upad;
  a.zone_lo = zone_lo; a.zone_hi = zone_hi; a.mask_ratio = mask_ratio; a.with_noise = with_noise != 0; a.quantise = quantise != 0;
  hipLaunchKernelGGL(mask_zone_kernel, dim3((unsigned)((Lpad + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
