// Voice-activity detector (the reference's vad.onnx, tf2onnx opset 13) behind mi355asr_vad_* of include/mi355asr.h.
//
// One launch takes waveform samples to one fp32 score per 10 ms frame.  Per frame (80 samples of 8 kHz audio):
//   dense -> dense_1+ReLU -> causal zero pad 4 -> conv1d(k5)+ReLU -> dense_2+ReLU -> LayerNorm(eps 1e-3)
//   -> causal zero pad 4 -> conv1d_1(k5)+ReLU -> dense_3+ReLU -> dense_4 (80 -> 1)
// so a frame depends on itself and the 8 frames before it.  A workgroup owns a tile of kRows LDS rows: kTile output
// frames plus the 8-frame halo before them.  Every 80x80 product (and each conv as K = 5 * 80) is exact fp32 on
// v_mfma_f32_16x16x4_f32; wave w of the five owns output columns 16w .. 16w+15 of every row of the tile, so each weight
// fragment it reads from L2 (pre-packed in fragment order, 1 KiB per wave load) feeds kRows / 16 MFMAs.  Activations
// ping-pong between two LDS buffers; four leading rows of each stay zero so the conv taps of the first rows read zeros.
//
// Speech enhancement (mi355asr_vad_enhance, the online SavedModel's second output): vad_kernel<VadEnhanceArgs> runs one more
// 80x80 layer on dense_3's output, audio_voice_mask (linear: no activation), and writes enhanced = frame * mask for the
// tile's output frames.  The frame samples are re-read from global memory (L2) since the LDS copy has been overwritten
// by then.  The mask multiplies the samples the network saw: with decimate = 2 that is wav[::2] of 16 kHz input, so
// the enhanced output is 8 kHz audio, 80 samples per frame, for either decimation.  vad_kernel<VadArgs> is the
// scores-only kernel, with the arithmetic it had before the variant existed; the enhance variant's score head is the
// same code, so both return the same scores bit for bit.
#include "common.h"
#include "model.h"

namespace {

constexpr int kC = 80;              // channels = samples per frame
constexpr int kRows = 64;           // LDS rows per tile (4 M-tiles of 16)
constexpr int kHalo = 8;            // frames of left context: two causal 5-tap convolutions
constexpr int kTile = kRows - kHalo;
constexpr int kLd = 84;             // LDS row stride (floats): 16-byte aligned, 16 rows land on distinct banks
constexpr int kPadRows = 4;
constexpr int kWaves = kC / 16;     // one 16-column N-tile per wave
constexpr int kThreads = kWaves * 64;

// arena offsets (floats) of the packed weights: six MFMA matrices, their biases, LayerNorm and the 80 -> 1 head
constexpr int kTaps[6] = {1, 1, 5, 1, 5, 1};   // dense, dense_1, conv1d, dense_2, conv1d_1, dense_3
constexpr size_t pack_floats(int taps) { return (size_t)taps * kC * kC; }
constexpr size_t w_off(int layer) {
  size_t o = 0;
  for (int i = 0; i < layer; ++i) o += pack_floats(kTaps[i]);
  return o;
}
constexpr size_t kBiasOff = w_off(6);               // 6 x 80 biases
constexpr size_t kGammaOff = kBiasOff + 6 * kC;
constexpr size_t kBetaOff = kGammaOff + kC;
constexpr size_t kHeadOff = kBetaOff + kC;          // dense_4 kernel [80] then its bias
constexpr size_t kArenaFloats = kHeadOff + kC + 4;
// enhancer handles only: audio_voice_mask packed like the other 80x80 layers, then its bias
constexpr size_t kMaskOff = kArenaFloats;
constexpr size_t kMaskBiasOff = kMaskOff + pack_floats(1);
constexpr size_t kEnhArenaFloats = kMaskBiasOff + kC;
static_assert(kMaskOff % 4 == 0, "fragment loads of the mask layer need 16-byte alignment");

struct VadArgs {
  const float* wav;        // [B, L]
  const int32_t* in_len;   // [B] samples, or null
  float* scores;           // [B, T], or null (enhance only)
  const float* w;          // arena
  int B, L, T, dec, tiles;
};

struct VadEnhanceArgs : VadArgs {
  float* enhanced;         // [B, T * 80]
};

// out[i][16w + c] = act(sum_{tap,k} in[i - (TAPS-1) + tap][k] * W[tap][k][16w + c] + bias), rows i in [0, kRows).
// The fragment k order inside each 16-wide group is k = 16g + 4h + j (lane half h = lane>>4, MFMA step j), so that A
// is one ds_read_b128 per lane and B one 16-byte global load per lane; the sum is still exact fp32 products.
template <int TAPS>
__device__ __forceinline__ void mfma_layer(const float* in, float* out, const f32x4* wp, const float* bias, bool relu,
                                           int zero_rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  constexpr int MT = kRows / 16, G = kC / 16;
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* wpw = wp + (size_t)w * TAPS * G * 64 + lane;
  for (int tap = 0; tap < TAPS; ++tap) {
    f32x4 bv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bv[g] = wpw[(tap * G + g) * 64];
    const float* base = in + (r - (TAPS - 1) + tap) * kLd + 4 * h;
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(base + 16 * m * kLd + 16 * g);
        acc[m] = mfma4(av.x, bv[g].x, acc[m]);
        acc[m] = mfma4(av.y, bv[g].y, acc[m]);
        acc[m] = mfma4(av.z, bv[g].z, acc[m]);
        acc[m] = mfma4(av.w, bv[g].w, acc[m]);
      }
    }
  }
  const int col = 16 * w + r;
  const float bb = bias[col];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 16 * m + 4 * h + j;
      float v = acc[m][j] + bb;
      if (relu) v = fmaxf(v, 0.f);
      out[row * kLd + col] = row < zero_rows ? 0.f : v;
    }
}

// Args = VadArgs: scores only; VadEnhanceArgs: scores (optional) and enhanced frames
template <class Args>
__global__ __launch_bounds__(kThreads) void vad_kernel(Args a) {
  constexpr bool kEnhance = std::is_same<Args, VadEnhanceArgs>::value;
  __shared__ __attribute__((aligned(16))) float lds[2][(kPadRows + kRows) * kLd];
  const int tile = blockIdx.x % a.tiles, b = blockIdx.x / a.tiles;
  int Tb = a.T;
  if (a.in_len) Tb = min(max(a.in_len[b], 0), a.L) / (kC * a.dec);
  const int t0 = tile * kTile;
  if (t0 >= Tb) return;
  float* X = lds[0] + kPadRows * kLd;
  float* Y = lds[1] + kPadRows * kLd;
  const int tid = threadIdx.x;
  for (int i = tid; i < kPadRows * kLd; i += kThreads) { lds[0][i] = 0.f; lds[1][i] = 0.f; }
  // input rows: frame f = t0 - kHalo + i, sample c of it = wav[(f * 80 + c) * dec]; frames outside [0, Tb) are not read
  const float* wrow = a.wav + (size_t)b * a.L;
  for (int i = tid; i < kRows * kC; i += kThreads) {
    const int row = i / kC, c = i - row * kC, f = t0 - kHalo + row;
    X[row * kLd + c] = (f >= 0 && f < Tb) ? wrow[((size_t)f * kC + c) * a.dec] : 0.f;
  }
  __syncthreads();
  // rows of frames before t = 0 enter both convolutions as zero activations (the graph's Pad on the activations)
  const int zr = max(kHalo - t0, 0);
  const f32x4* W = reinterpret_cast<const f32x4*>(a.w);
  const float* bias = a.w + kBiasOff;
  mfma_layer<1>(X, Y, W + w_off(0) / 4, bias + 0 * kC, false, 0);
  __syncthreads();
  mfma_layer<1>(Y, X, W + w_off(1) / 4, bias + 1 * kC, true, zr);
  __syncthreads();
  mfma_layer<5>(X, Y, W + w_off(2) / 4, bias + 2 * kC, true, 0);
  __syncthreads();
  mfma_layer<1>(Y, X, W + w_off(3) / 4, bias + 3 * kC, true, 0);
  __syncthreads();
  // LayerNorm over the 80 channels of each frame, in place (population variance, as the graph's BatchNormalization)
  if (tid < kRows) {
    float* x = X + tid * kLd;
    float s = 0.f;
    for (int c = 0; c < kC; ++c) s += x[c];
    const float mean = s / kC;
    float q = 0.f;
    for (int c = 0; c < kC; ++c) { const float d = x[c] - mean; q = fmaf(d, d, q); }
    const float rs = 1.f / sqrtf(q / kC + kLnEps);
    const bool zero = tid < zr;
    for (int c = 0; c < kC; ++c)
      x[c] = zero ? 0.f : fmaf((x[c] - mean) * rs, a.w[kGammaOff + c], a.w[kBetaOff + c]);
  }
  __syncthreads();
  mfma_layer<5>(X, Y, W + w_off(4) / 4, bias + 4 * kC, true, 0);
  __syncthreads();
  mfma_layer<1>(Y, X, W + w_off(5) / 4, bias + 5 * kC, true, 0);
  __syncthreads();
  if (tid < kTile && (!kEnhance || a.scores)) {
    const int f = t0 + tid;
    if (f < Tb) {
      const float* x = X + (kHalo + tid) * kLd;
      float s = 0.f;
      for (int c = 0; c < kC; ++c) s = fmaf(x[c], a.w[kHeadOff + c], s);
      a.scores[(size_t)b * a.T + f] = s + a.w[kHeadOff + kC];
    }
  }
  if constexpr (kEnhance) {
    // mask = dense_3 @ K + b (no activation) into Y; the head above only reads X, so no barrier between them
    mfma_layer<1>(X, Y, W + kMaskOff / 4, a.w + kMaskBiasOff, false, 0);
    __syncthreads();
    // enhanced[b, f*80 + c] = frame sample * mask for the tile's output frames [t0, t0 + nf): one contiguous span of
    // the output row, stored in thread order; the samples are the ones the input rows read above
    const int nf = min(kTile, Tb - t0);
    float* erow = a.enhanced + (size_t)b * a.T * kC + (size_t)t0 * kC;
    const float* xin = wrow + (size_t)t0 * kC * a.dec;
    for (int i = tid; i < nf * kC; i += kThreads) {
      const int row = i / kC, c = i - row * kC;
      erow[i] = xin[(size_t)i * a.dec] * Y[(kHalo + row) * kLd + c];
    }
  }
}

const char* kDenseNames[4] = {"dense", "dense_1", "dense_2", "dense_3"};

// weights [taps][80 in][80 out] -> fragments [n-tile w][tap][group g][lane][j] = W[tap][16g + 4(lane>>4) + j][16w + (lane&15)]
void pack_layer(const std::vector<float>& w, int taps, float* p) {
  const int G = kC / 16;
  for (int wv = 0; wv < kWaves; ++wv)
    for (int tap = 0; tap < taps; ++tap)
      for (int g = 0; g < G; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * wv + (lane & 15);
            p[((((size_t)wv * taps + tap) * G + g) * 64 + lane) * 4 + j] = w[((size_t)tap * kC + k) * kC + n];
          }
}

int create_vad(const mi355asr_vad_config* cfg, mi355asr_model** out, bool enhance) {
  if (!cfg || !out) return fail(MI355ASR_EINVAL, "null argument");
  if (cfg->dmodel != kC || cfg->frame != kC) return fail(MI355ASR_EINVAL, "VAD: dmodel=%d frame=%d, supported is 80 / 80", cfg->dmodel, cfg->frame);
  if (cfg->decimate != 1 && cfg->decimate != 2) return fail(MI355ASR_EINVAL, "VAD: decimate=%d, must be 1 or 2", cfg->decimate);
  auto* m = new mi355asr_model();
  m->is_vad = true;
  m->vad_enhance = enhance;
  m->vcfg = *cfg;
  std::memset(&m->cfg, 0, sizeof(m->cfg));
  std::memset(&m->dm, 0, sizeof(m->dm));
  auto& ex = m->expected;
  for (const char* n : kDenseNames) {
    ex.push_back({std::string(n) + "/kernel", {kC, kC}});
    ex.push_back({std::string(n) + "/bias", {kC}});
  }
  ex.push_back({"conv1d/kernel", {5, kC, kC}});
  ex.push_back({"conv1d/bias", {kC}});
  ex.push_back({"layer_normalization/gamma", {kC}});
  ex.push_back({"layer_normalization/beta", {kC}});
  ex.push_back({"conv1d_1/kernel", {5, kC, kC}});
  ex.push_back({"conv1d_1/bias", {kC}});
  ex.push_back({"dense_4/kernel", {kC, 1}});
  ex.push_back({"dense_4/bias", {1}});
  if (enhance) {
    ex.push_back({"audio_voice_mask/kernel", {kC, kC}});
    ex.push_back({"audio_voice_mask/bias", {kC}});
  }
  for (const auto& e : ex) m->host[e.name] = HostTensor{};
  *out = m;
  return 0;
}

}  // namespace

namespace mi355 {

int finalize_vad(mi355asr_model* m, hipStream_t s) {
  // the scores-only layout is a prefix of the enhancer's, so mi355asr_vad_forward reads either arena alike
  std::vector<float> arena(m->vad_enhance ? kEnhArenaFloats : kArenaFloats, 0.f);
  const char* mats[6] = {"dense/kernel", "dense_1/kernel", "conv1d/kernel", "dense_2/kernel", "conv1d_1/kernel", "dense_3/kernel"};
  const char* biases[6] = {"dense/bias", "dense_1/bias", "conv1d/bias", "dense_2/bias", "conv1d_1/bias", "dense_3/bias"};
  for (int L = 0; L < 6; ++L) {
    pack_layer(m->host[mats[L]].data, kTaps[L], arena.data() + w_off(L));
    std::memcpy(arena.data() + kBiasOff + L * kC, m->host[biases[L]].data.data(), kC * sizeof(float));
  }
  if (m->vad_enhance) {
    pack_layer(m->host["audio_voice_mask/kernel"].data, 1, arena.data() + kMaskOff);
    std::memcpy(arena.data() + kMaskBiasOff, m->host["audio_voice_mask/bias"].data.data(), kC * sizeof(float));
  }
  std::memcpy(arena.data() + kGammaOff, m->host["layer_normalization/gamma"].data.data(), kC * sizeof(float));
  std::memcpy(arena.data() + kBetaOff, m->host["layer_normalization/beta"].data.data(), kC * sizeof(float));
  std::memcpy(arena.data() + kHeadOff, m->host["dense_4/kernel"].data.data(), kC * sizeof(float));
  arena[kHeadOff + kC] = m->host["dense_4/bias"].data[0];
  if (m->arena) { (void)hipFree(m->arena); m->arena = nullptr; }
  HIP_TRY(hipMalloc((void**)&m->arena, arena.size() * sizeof(float)));
  m->arena_floats = arena.size();
  HIP_TRY(hipMemcpyAsync(m->arena, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (auto& kv : m->host) { kv.second.data.clear(); kv.second.data.shrink_to_fit(); }
  m->finalized = true;
  return 0;
}

}  // namespace mi355

extern "C" {
int mi355asr_vad_create(const mi355asr_vad_config* cfg, mi355asr_model** out) { return create_vad(cfg, out, false); }

int mi355asr_vad_enhancer_create(const mi355asr_vad_config* cfg, mi355asr_model** out) {
  return create_vad(cfg, out, true);
}

int mi355asr_vad_frames(const mi355asr_model* m, int32_t L, int32_t* T) {
  if (!m || !m->is_vad || !T) return fail(MI355ASR_EINVAL, "not a VAD handle / null argument");
  if (L < 0) return fail(MI355ASR_EINVAL, "L=%d must be >= 0", L);
  *T = L / (kC * m->vcfg.decimate);
  return 0;
}

int mi355asr_vad_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes) {
  if (!m || !m->is_vad || !bytes) return fail(MI355ASR_EINVAL, "not a VAD handle / null argument");
  if (B < 1 || L < 0) return fail(MI355ASR_EINVAL, "B must be positive and L >= 0 (got %d, %d)", B, L);
  *bytes = 0;   // the fused kernel keeps every activation in LDS
  return 0;
}

int mi355asr_vad_forward(mi355asr_model* m, const float* wav, int32_t B, int32_t L, const int32_t* in_len,
                         float* scores, void* stream) {
  if (!m || !m->is_vad) return fail(MI355ASR_EINVAL, "not a VAD handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (B < 1 || L < 0) return fail(MI355ASR_EINVAL, "B must be positive and L >= 0 (got %d, %d)", B, L);
  const int dec = m->vcfg.decimate, T = L / (kC * dec);
  if (T == 0) return 0;
  if (!wav || !scores) return fail(MI355ASR_EINVAL, "null argument");
  VadArgs a{wav, in_len, scores, m->arena, B, L, T, dec, ceil_div(T, kTile)};
  const int64_t blocks = (int64_t)B * a.tiles;
  if (blocks > INT32_MAX) return fail(MI355ASR_EINVAL, "B * tiles = %lld exceeds the grid", (long long)blocks);
  hipLaunchKernelGGL(vad_kernel<VadArgs>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch vad_kernel: %s", hipGetErrorString(e));
  return 0;
}

int mi355asr_vad_enhance(mi355asr_model* m, const float* wav, int32_t B, int32_t L, const int32_t* in_len,
                         float* scores, float* enhanced, void* stream) {
  if (!m || !m->is_vad) return fail(MI355ASR_EINVAL, "not a VAD handle");
  if (!m->vad_enhance) return fail(MI355ASR_EINVAL, "VAD handle has no voice-mask head: create it with mi355asr_vad_enhancer_create");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (B < 1 || L < 0) return fail(MI355ASR_EINVAL, "B must be positive and L >= 0 (got %d, %d)", B, L);
  const int dec = m->vcfg.decimate, T = L / (kC * dec);
  if (T == 0) return 0;
  if (!wav || !enhanced) return fail(MI355ASR_EINVAL, "null argument");
  VadEnhanceArgs a;
  static_cast<VadArgs&>(a) = VadArgs{wav, in_len, scores, m->arena, B, L, T, dec, ceil_div(T, kTile)};
  a.enhanced = enhanced;
  const int64_t blocks = (int64_t)B * a.tiles;
  if (blocks > INT32_MAX) return fail(MI355ASR_EINVAL, "B * tiles = %lld exceeds the grid", (long long)blocks);
  hipLaunchKernelGGL(vad_kernel<VadEnhanceArgs>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch vad_kernel (enhance): %s", hipGetErrorString(e));
  return 0;
}
}  // extern "C"
