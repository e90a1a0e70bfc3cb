// Punctuation restorer (the reference's punc.onnx: PuncTransformer.inference) behind mi355asr_punc_* of include/mi355asr.h.
//
// One launch takes a ragged batch of token ids to class probabilities; one workgroup of eight waves owns one sentence and
// walks the whole network over it:
//   x = emb[id] * 8 + pe[t] -> Dense + ELU -> n x { EncoderLayer -> causal Conv1D(k 3) + ReLU -> + x }
//   -> Dense(64 -> 768 -> 64), folded into one 64 x 64 matrix at finalize -> max(n - 1, 1) x EncoderLayer -> Dense + softmax
// Every contraction is exact fp32 on v_mfma_f32_16x16x4_f32.  A 64 x 64 layer gives wave w the output columns 16 (w & 3) ..
// of every second 16-row tile; its weight fragments (pre-packed in fragment order, vad.hip's layout) stay in registers over
// the tiles.  Attention gives wave w head w: scores come out of the MFMA transposed, S^T = K Q^T, so that a lane holds four
// keys of one query -- which is the A fragment of P V with no exchange; column 8 of the V fragment is 1, so the softmax
// denominator is a column of the same accumulator.  Scores are computed twice (row maximum, then exp and P V): nothing of
// size T x T is stored.
// Activations are four [Tp, 64] buffers (row stride kLd) plus the key mask.  A sentence of up to kLdsTokens tokens keeps them in
// LDS; a longer one runs the same code on its region of the caller's workspace (global memory, workgroup barriers between the
// steps).  Which of the two a row takes depends on its own length alone, so a row's result does not depend on its batch.
// punc_heads_kernel (mi355asr_punc_heads) is the same walk compiled with HEADS: where the encoder stack ends it also multiplies
// enc_output by the UNFOLDED to_bert [64, 768] (the trainer's distillation feature; 48 column tiles over the eight waves, straight
// to global memory), and at the end it writes the logits in place of their softmax.  punc_kernel is the HEADS = false instance.
#include <cfloat>

#include "common.h"
#include "model.h"

namespace {

constexpr int kD = 64;                // d_model = enc_embedding_dim = dff
constexpr int kHeads = 8;
constexpr int kDh = kD / kHeads;
constexpr int kLd = 68;               // activation row stride (floats): 16-byte aligned rows
constexpr int kBufs = 4;
constexpr int kWaves = 8;             // one per head; two per 16-column tile of a layer
constexpr int kThreads = kWaves * 64;
constexpr int kMaxTokens = 1024;
constexpr int kMaxClasses = 64;
constexpr float kPuncLnEps = 1e-6f;
constexpr size_t kLdsBudget = 160 * 1024;
constexpr size_t kRowFloats = kBufs * kLd + 1;          // four activation rows and the key's mask term
// the longest sentence in LDS: whole 16-row tiles within the budget
constexpr int kLdsTokens = (int)(kLdsBudget / (kRowFloats * sizeof(float))) / 16 * 16;
static_assert(kLdsTokens == 144, "DESIGN.md section 18 and the header quote this figure");
constexpr size_t act_floats(int Tp) { return (size_t)Tp * kRowFloats; }
static_assert(act_floats(kLdsTokens) * sizeof(float) <= kLdsBudget, "LDS variant exceeds the budget");

// arena (floats): [proj | n_enc layers | n_enc convs | fold | n_map layers | head | embedding | pos_encoding]
constexpr size_t kMat = (size_t)kD * kD;
constexpr size_t kDenseFloats = kMat + kD;                      // packed matrix, bias
constexpr size_t kLayerFloats = 6 * kMat + 6 * kD + 4 * kD;     // wq wk wv wo w1 w2 | their biases | g1 b1 g2 b2
constexpr size_t kLayerBias = 6 * kMat, kLayerLn = 6 * kMat + 6 * kD;
constexpr size_t kConvFloats = 3 * kMat + kD;
// the unfolded to_bert (the distillation feature of mi355asr_punc_heads) lies behind pos_encoding: [to_bert | its bias]
constexpr int kBert = 768;
constexpr size_t kBertFloats = (size_t)kD * kBert + kBert;

struct PuncArgs {
  const int32_t* ids;     // [B, T]
  const int32_t* lens;    // [B] or null
  float* probs;           // [B, T, classes]
  int32_t* cls;           // [B, T] or null
  float* pmax;            // [B, T] or null
  const float* w;         // arena
  float* ws;              // workspace: ws_row floats per sentence (rows longer than kLdsTokens only)
  size_t ws_row;
  size_t o_conv, o_fold, o_map, o_head, o_emb, o_pe;
  int B, T, n_enc, n_map, vocab, classes;
  // the training outputs (punc_heads_kernel); appended, so the inference kernel's arguments keep their places
  float* logits;          // [B, T, classes] or null
  float* feature;         // [B, T, kBert] or null
  size_t o_bert;
};

enum { ACT_NONE, ACT_RELU, ACT_ELU };

// out[i][n] = act(sum_{tap, k} in[i - (TAPS - 1) + tap][k] W[tap][k][n] + bias[n]) (+ res[i][n]) for rows i in [0, Tp); rows
// before 0 read as zeros (the causal pad).  Fragment k order inside a 16-wide group: k = 16 g + 4 h + j (h = lane >> 4, MFMA
// step j), so A is one 16-byte load per lane.  `out` is neither `in` nor, with TAPS > 1, anything `in` aliases.
template <int TAPS, int ACT, bool RES>
DEV void mm64(const float* in, float* out, const float* res, const float* wp, const float* bias, int Tp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4, ct = w & 3;
  constexpr int G = kD / 16;
  const f32x4* wpw = reinterpret_cast<const f32x4*>(wp) + (size_t)ct * TAPS * G * 64 + lane;
  f32x4 bv[TAPS][G];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int g = 0; g < G; ++g) bv[tap][g] = wpw[(tap * G + g) * 64];
  const int col = 16 * ct + r;
  const float bb = bias[col];
  for (int m = w >> 2; m < Tp / 16; m += 2) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int row = 16 * m + r - (TAPS - 1) + tap;
      const bool ok = row >= 0;
      const float* a = in + (ok ? row : 0) * kLd + 4 * h;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        f32x4 av = *reinterpret_cast<const f32x4*>(a + 16 * g);
        if (!ok) av = f32x4{0.f, 0.f, 0.f, 0.f};
        acc = mfma4(av.x, bv[tap][g].x, acc);
        acc = mfma4(av.y, bv[tap][g].y, acc);
        acc = mfma4(av.z, bv[tap][g].z, acc);
        acc = mfma4(av.w, bv[tap][g].w, acc);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int at = (16 * m + 4 * h + j) * kLd + col;
      float v = acc[j] + bb;
      if (ACT == ACT_RELU) v = fmaxf(v, 0.f);
      if (ACT == ACT_ELU) v = v > 0.f ? v : expm1f(v);
      if (RES) v += res[at];
      out[at] = v;
    }
  }
}

// out[i][n] = sum_k in[i][k] W[k][n] + bias[n] for the rows i < len and the kBert columns of to_bert, written to global memory (row
// stride kBert): wave w takes the column tiles w, w + 8, ..., keeps a tile's four weight fragments in registers over the rows
// and adds k in the order mm64 does
DEV void to_bert(const float* in, float* out, const float* wp, const float* bias, int len, int Tp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  constexpr int G = kD / 16;
  for (int ct = w; ct < kBert / 16; ct += kWaves) {
    const f32x4* wpw = reinterpret_cast<const f32x4*>(wp) + (size_t)ct * G * 64 + lane;
    f32x4 bv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bv[g] = wpw[g * 64];
    const int col = 16 * ct + r;
    const float bb = bias[col];
    for (int m = 0; m < Tp / 16; ++m) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* a = in + (16 * m + r) * kLd + 4 * h;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + 16 * g);
        acc = mfma4(av.x, bv[g].x, acc);
        acc = mfma4(av.y, bv[g].y, acc);
        acc = mfma4(av.z, bv[g].z, acc);
        acc = mfma4(av.w, bv[g].w, acc);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * m + 4 * h + j;
        if (row < len) out[(size_t)row * kBert + col] = acc[j] + bb;
      }
    }
  }
}

DEV float sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// LayerNorm over the 64 features of each row, in place; sixteen lanes per row, four features each
DEV void layernorm(float* x, const float* gamma, const float* beta, int Tp) {
  const int sub = threadIdx.x & 15;
  const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * sub), b = *reinterpret_cast<const f32x4*>(beta + 4 * sub);
  for (int row = threadIdx.x >> 4; row < Tp; row += kThreads / 16) {
    f32x4* p = reinterpret_cast<f32x4*>(x + row * kLd + 4 * sub);
    const f32x4 v = *p;
    const float mean = sum16((v.x + v.y) + (v.z + v.w)) * (1.f / kD);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    const float var = sum16((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.f / kD);
    const float rs = 1.f / sqrtf(var + kPuncLnEps);
    *p = f32x4{dx * rs * g.x + b.x, dy * rs * g.y + b.y, dz * rs * g.z + b.z, dw * rs * g.w + b.w};
  }
}

// scores of one 16-key tile against the wave's 16 queries, transposed: s[j] = logit of key 16 kt + 4 h + j for query lane & 15
DEV f32x4 score_tile(const float* K, const float* madd, f32x2 q, int kt, int head, int r, int h) {
  const f32x2 kk = *reinterpret_cast<const f32x2*>(K + (16 * kt + r) * kLd + kDh * head + 2 * h);
  f32x4 s = mfma4(kk.x, q.x, f32x4{0.f, 0.f, 0.f, 0.f});
  s = mfma4(kk.y, q.y, s);
  const f32x4 ma = *reinterpret_cast<const f32x4*>(madd + 16 * kt + 4 * h);
  constexpr float kScale = 0.35355339059327379f;   // 1 / sqrt(8)
  return f32x4{s.x * kScale + ma.x, s.y * kScale + ma.y, s.z * kScale + ma.z, s.w * kScale + ma.w};
}

// ctx = softmax(q k^T / sqrt(8) + mask) v over the keys [0, len), head = wave; written over q
DEV void attention(float* Q, const float* K, const float* V, const float* madd, int len, int Tp) {
  const int lane = threadIdx.x & 63, head = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  const int nkt = (len + 15) / 16;
  for (int qt = 0; qt < Tp / 16; ++qt) {
    // the head's eight features split over the two MFMA steps as k = 2 h + step: one 8-byte load for q and for each key
    const f32x2 q = *reinterpret_cast<const f32x2*>(Q + (16 * qt + r) * kLd + kDh * head + 2 * h);
    float mx = -FLT_MAX;
    for (int kt = 0; kt < nkt; ++kt) {
      const f32x4 s = score_tile(K, madd, q, kt, head, r, h);
      const int key = 16 * kt + 4 * h;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (key + j < len) mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nkt; ++kt) {
      const f32x4 s = score_tile(K, madd, q, kt, head, r, h);
      const int key = 16 * kt + 4 * h;
      const float* vrow = V + key * kLd + kDh * head + (r & 7);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = key + j < len ? expf(s[j] - mx) : 0.f;
        // B[k = key 4 h + j][column r]: the head's value features in columns 0 .. 7, ones in column 8 (the row sum of p)
        const float vb = r == 8 ? 1.f : vrow[j * kLd];
        o = mfma4(p, vb, o);
      }
    }
    // o[j] = sum_key p v of query 16 qt + 4 h + j, feature r; its denominator sits in the lane of column 8
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float l = __shfl(o[j], (lane & 48) | 8);
      if (r < kDh) Q[(16 * qt + 4 * h + j) * kLd + kDh * head + r] = o[j] / l;
    }
  }
}

// one EncoderLayer on the rows in X: out2 lands in Qb; X is left as it was; Kb, Vb are scratch
DEV void encoder_layer(const float* X, float* Qb, float* Kb, float* Vb, const float* madd, const float* wl, int len, int Tp) {
  const float* bias = wl + kLayerBias;
  const float* ln = wl + kLayerLn;
  mm64<1, ACT_NONE, false>(X, Qb, nullptr, wl + 0 * kMat, bias + 0 * kD, Tp);
  mm64<1, ACT_NONE, false>(X, Kb, nullptr, wl + 1 * kMat, bias + 1 * kD, Tp);
  mm64<1, ACT_NONE, false>(X, Vb, nullptr, wl + 2 * kMat, bias + 2 * kD, Tp);
  __syncthreads();
  attention(Qb, Kb, Vb, madd, len, Tp);
  __syncthreads();
  mm64<1, ACT_NONE, true>(Qb, Kb, X, wl + 3 * kMat, bias + 3 * kD, Tp);        // x + ctx Wo + bo
  __syncthreads();
  layernorm(Kb, ln + 0 * kD, ln + 1 * kD, Tp);                                   // out1
  __syncthreads();
  mm64<1, ACT_RELU, false>(Kb, Vb, nullptr, wl + 4 * kMat, bias + 4 * kD, Tp);
  __syncthreads();
  mm64<1, ACT_NONE, true>(Vb, Qb, Kb, wl + 5 * kMat, bias + 5 * kD, Tp);       // out1 + W2 relu(W1 out1)
  __syncthreads();
  layernorm(Qb, ln + 2 * kD, ln + 3 * kD, Tp);                                   // out2
  __syncthreads();
}

// the whole network over one sentence; `act` is LDS or the sentence's workspace region (the address space is inferred per call).
// HEADS: the training outputs in place of the probabilities -- to_bert(enc_output) from the unfolded weights, and the logits the
// softmax would take
template <bool HEADS>
DEV void punc_sentence(const PuncArgs& a, int b, int len, float* act) {
  const int tid = threadIdx.x, sub = tid & 15;
  const int Tp = (len + 15) & ~15;
  const size_t bufsz = (size_t)Tp * kLd;
  float* madd = act + kBufs * bufsz;
  int bx = 0, bk = 1, bq = 2, bv = 3;
  auto buf = [&](int i) { return act + i * bufsz; };
  // x = emb[id] * sqrt(64) + pe[t]; rows past the sentence are zeros (they are never keys, but P V multiplies them by 0)
  const int32_t* ids = a.ids + (size_t)b * a.T;
  for (int t = tid >> 4; t < Tp; t += kThreads / 16) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    float ma = 0.f;
    if (t < len) {
      const int raw = ids[t];
      const int id = min(max(raw, 0), a.vocab - 1);
      const f32x4 e = *reinterpret_cast<const f32x4*>(a.w + a.o_emb + (size_t)id * kD + 4 * sub);
      const f32x4 pe = *reinterpret_cast<const f32x4*>(a.w + a.o_pe + (size_t)t * kD + 4 * sub);
      v = f32x4{e.x * 8.f + pe.x, e.y * 8.f + pe.y, e.z * 8.f + pe.z, e.w * 8.f + pe.w};
      ma = raw == 0 ? -1e9f : 0.f;
    }
    *reinterpret_cast<f32x4*>(buf(bk) + t * kLd + 4 * sub) = v;
    if (sub == 0) madd[t] = ma;
  }
  __syncthreads();
  mm64<1, ACT_ELU, false>(buf(bk), buf(bx), nullptr, a.w, a.w + kMat, Tp);
  __syncthreads();
  for (int i = 0; i < a.n_enc; ++i) {
    encoder_layer(buf(bx), buf(bq), buf(bk), buf(bv), madd, a.w + kDenseFloats + i * kLayerFloats, len, Tp);
    const float* wc = a.w + a.o_conv + i * kConvFloats;
    mm64<3, ACT_RELU, true>(buf(bq), buf(bk), buf(bx), wc, wc + 3 * kMat, Tp);   // relu(conv(out2)) + x
    __syncthreads();
    const int t = bx; bx = bk; bk = t;
  }
  if constexpr (HEADS) {
    // enc_output is read here and by the fold below; neither writes it
    if (a.feature)
      to_bert(buf(bx), a.feature + (size_t)b * a.T * kBert, a.w + a.o_bert, a.w + a.o_bert + (size_t)kD * kBert, len, Tp);
  }
  mm64<1, ACT_NONE, false>(buf(bx), buf(bk), nullptr, a.w + a.o_fold, a.w + a.o_fold + kMat, Tp);
  __syncthreads();
  { const int t = bx; bx = bk; bk = t; }
  for (int i = 0; i < a.n_map; ++i) {
    encoder_layer(buf(bx), buf(bq), buf(bk), buf(bv), madd, a.w + a.o_map + i * kLayerFloats, len, Tp);
    const int t = bx; bx = bq; bq = t;
  }
  mm64<1, ACT_NONE, false>(buf(bx), buf(bk), nullptr, a.w + a.o_head, a.w + a.o_head + kMat, Tp);
  __syncthreads();
  // softmax over the classes, the arg-max of the probabilities as written (the lowest class on a tie) and its value
  const float* lg = buf(bk);
  const int C = a.classes;
  if constexpr (HEADS) {
    if (a.logits) {
      float* out = a.logits + (size_t)b * a.T * C;
      for (int i = tid; i < len * C; i += kThreads) out[i] = lg[(i / C) * kLd + i % C];
    }
    return;
  }
  for (int t = tid >> 4; t < len; t += kThreads / 16) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(lg + t * kLd + 4 * sub);
    float x[4] = {v.x, v.y, v.z, v.w};
    float mx = -FLT_MAX;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * sub + j < C) mx = fmaxf(mx, x[j]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = 4 * sub + j < C ? expf(x[j] - mx) : 0.f;
      s += x[j];
    }
    s = sum16(s);
    float best = -1.f;
    int bi = 0;
    float* prow = a.probs + ((size_t)b * a.T + t) * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = x[j] / s;
      if (4 * sub + j < C) {
        prow[4 * sub + j] = p;
        if (p > best) { best = p; bi = 4 * sub + j; }
      }
    }
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const float ob = __shfl_xor(best, d);
      const int oi = __shfl_xor(bi, d);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (sub == 0) {
      if (a.cls) a.cls[(size_t)b * a.T + t] = bi;
      if (a.pmax) a.pmax[(size_t)b * a.T + t] = best;
    }
  }
}

extern __shared__ __attribute__((aligned(16))) float punc_lds[];

__global__ __launch_bounds__(kThreads) void punc_kernel(PuncArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int len = a.T;
  if (a.lens) len = min(max(a.lens[b], 0), a.T);
  // outputs at or past the sentence's length are zeros
  {
    const size_t row = (size_t)b * a.T;
    float* p = a.probs + (row + len) * a.classes;
    for (int i = tid; i < (a.T - len) * a.classes; i += kThreads) p[i] = 0.f;
    for (int t = len + tid; t < a.T; t += kThreads) {
      if (a.cls) a.cls[row + t] = 0;
      if (a.pmax) a.pmax[row + t] = 0.f;
    }
  }
  if (len == 0) return;
  if (len <= kLdsTokens)
    punc_sentence<false>(a, b, len, punc_lds);
  else
    punc_sentence<false>(a, b, len, a.ws + (size_t)b * a.ws_row);
}

// the same walk with the training outputs (mi355asr_punc_heads): logits and / or the to_bert feature, zeros at and past the length
__global__ __launch_bounds__(kThreads) void punc_heads_kernel(PuncArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int len = a.T;
  if (a.lens) len = min(max(a.lens[b], 0), a.T);
  {
    const size_t row = (size_t)b * a.T + len;
    const size_t rest = (size_t)(a.T - len);
    if (a.logits)
      for (size_t i = tid; i < rest * a.classes; i += kThreads) a.logits[row * a.classes + i] = 0.f;
    if (a.feature)
      for (size_t i = tid; i < rest * kBert; i += kThreads) a.feature[row * kBert + i] = 0.f;
  }
  if (len == 0) return;
  if (len <= kLdsTokens)
    punc_sentence<true>(a, b, len, punc_lds);
  else
    punc_sentence<true>(a, b, len, a.ws + (size_t)b * a.ws_row);
}

// weights [taps][64 in][n_out <= 64 out] -> fragments [column tile][tap][group g][lane][j] = W[tap][16 g + 4 (lane >> 4) + j][16 ct + (lane & 15)],
// columns past n_out zero
void pack_mat(const float* w, int taps, int n_out, float* p) {
  const int G = kD / 16;
  for (int ct = 0; ct < kD / 16; ++ct)
    for (int tap = 0; tap < taps; ++tap)
      for (int g = 0; g < G; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * ct + (lane & 15);
            p[((((size_t)ct * taps + tap) * G + g) * 64 + lane) * 4 + j] = n < n_out ? w[((size_t)tap * kD + k) * n_out + n] : 0.f;
          }
}

// to_bert [64 in][kBert out] -> fragments [column tile][group g][lane][j] = W[16 g + 4 (lane >> 4) + j][16 ct + (lane & 15)]
void pack_bert(const float* w, float* p) {
  const int G = kD / 16;
  for (int ct = 0; ct < kBert / 16; ++ct)
    for (int g = 0; g < G; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * ct + (lane & 15);
          p[(((size_t)ct * G + g) * 64 + lane) * 4 + j] = w[(size_t)k * kBert + n];
        }
}

int map_layers(int num_layers) { return std::max(num_layers - 1, 1); }

void add_dense(std::vector<Expected>& ex, const std::string& n, int in, int out) {
  ex.push_back({n + "/kernel", {in, out}});
  ex.push_back({n + "/bias", {out}});
}

void add_layer(std::vector<Expected>& ex, const std::string& p) {
  for (const char* n : {"/mha/wq", "/mha/wk", "/mha/wv", "/mha/dense", "/ffn/dense_1", "/ffn/dense_2"}) add_dense(ex, p + n, kD, kD);
  for (const char* n : {"/layernorm1", "/layernorm2"}) {
    ex.push_back({p + n + "/gamma", {kD}});
    ex.push_back({p + n + "/beta", {kD}});
  }
}

void pack_enc_layer(mi355asr_model* m, const std::string& p, float* dst) {
  const char* mats[6] = {"/mha/wq", "/mha/wk", "/mha/wv", "/mha/dense", "/ffn/dense_1", "/ffn/dense_2"};
  for (int i = 0; i < 6; ++i) {
    pack_mat(m->host[p + mats[i] + "/kernel"].data.data(), 1, kD, dst + i * kMat);
    std::memcpy(dst + kLayerBias + i * kD, m->host[p + mats[i] + "/bias"].data.data(), kD * sizeof(float));
  }
  const char* lns[4] = {"/layernorm1/gamma", "/layernorm1/beta", "/layernorm2/gamma", "/layernorm2/beta"};
  for (int i = 0; i < 4; ++i) std::memcpy(dst + kLayerLn + i * kD, m->host[p + lns[i]].data.data(), kD * sizeof(float));
}

size_t lds_bytes_for(int T) { return act_floats(std::min((T + 15) & ~15, kLdsTokens)) * sizeof(float); }

// a dynamic LDS request above 64 KB needs the attribute on the kernel, once per device
int allow_lds() {
  static bool allowed_on[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  if (!allowed_on[dev]) {
    for (const void* k : {(const void*)punc_kernel, (const void*)punc_heads_kernel})
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
      }
    allowed_on[dev] = true;
  }
  return 0;
}

size_t ws_row_floats(int T) { return (act_floats((T + 15) & ~15) + 63) & ~(size_t)63; }

}  // namespace

namespace mi355 {

int finalize_punc(mi355asr_model* m, hipStream_t s) {
  const auto& c = m->pcfg;
  const int n_enc = c.num_layers, n_map = map_layers(c.num_layers);
  const size_t o_conv = kDenseFloats + (size_t)n_enc * kLayerFloats, o_fold = o_conv + (size_t)n_enc * kConvFloats,
               o_map = o_fold + kDenseFloats, o_head = o_map + (size_t)n_map * kLayerFloats, o_emb = o_head + kDenseFloats,
               o_pe = o_emb + (size_t)c.vocab * kD, o_bert = o_pe + (size_t)c.pe_input * kD, total = o_bert + kBertFloats;
  std::vector<float> arena(total, 0.f);
  pack_mat(m->host["encoder/dense/kernel"].data.data(), 1, kD, arena.data());
  std::memcpy(arena.data() + kMat, m->host["encoder/dense/bias"].data.data(), kD * sizeof(float));
  for (int i = 0; i < n_enc; ++i) {
    pack_enc_layer(m, "encoder/layer_" + std::to_string(i), arena.data() + kDenseFloats + i * kLayerFloats);
    float* cv = arena.data() + o_conv + i * kConvFloats;
    const std::string p = "encoder/conv_" + std::to_string(i);
    pack_mat(m->host[p + "/kernel"].data.data(), 3, kD, cv);
    std::memcpy(cv + 3 * kMat, m->host[p + "/bias"].data.data(), kD * sizeof(float));
  }
  for (int i = 0; i < n_map; ++i) pack_enc_layer(m, "map/layer_" + std::to_string(i), arena.data() + o_map + i * kLayerFloats);
  {
    // (x W19 + b19) W20 + b20 has no activation between its layers: W = W19 W20 and b = b19 W20 + b20, formed in fp64
    const auto& w19 = m->host["to_bert/kernel"].data; const auto& b19 = m->host["to_bert/bias"].data;
    const auto& w20 = m->host["to_hidden/kernel"].data; const auto& b20 = m->host["to_hidden/bias"].data;
    const int H = 768;
    std::vector<float> w(kMat), bias(kD);
    for (int n = 0; n < kD; ++n) {
      for (int k = 0; k < kD; ++k) {
        double acc = 0.0;
        for (int j = 0; j < H; ++j) acc += (double)w19[(size_t)k * H + j] * (double)w20[(size_t)j * kD + n];
        w[(size_t)k * kD + n] = (float)acc;
      }
      double acc = b20[n];
      for (int j = 0; j < H; ++j) acc += (double)b19[j] * (double)w20[(size_t)j * kD + n];
      bias[n] = (float)acc;
    }
    pack_mat(w.data(), 1, kD, arena.data() + o_fold);
    std::memcpy(arena.data() + o_fold + kMat, bias.data(), kD * sizeof(float));
    // ... and to_bert as it is, for the distillation feature (mi355asr_punc_heads)
    pack_bert(w19.data(), arena.data() + o_bert);
    std::memcpy(arena.data() + o_bert + (size_t)kD * kBert, b19.data(), kBert * sizeof(float));
  }
  pack_mat(m->host["final/kernel"].data.data(), 1, c.classes, arena.data() + o_head);
  std::memcpy(arena.data() + o_head + kMat, m->host["final/bias"].data.data(), c.classes * sizeof(float));
  std::memcpy(arena.data() + o_emb, m->host["embedding"].data.data(), (size_t)c.vocab * kD * sizeof(float));
  std::memcpy(arena.data() + o_pe, m->host["pos_encoding"].data.data(), (size_t)c.pe_input * kD * sizeof(float));
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
int mi355asr_punc_create(const mi355asr_punc_config* cfg, mi355asr_model** out) {
  if (!cfg || !out) return fail(MI355ASR_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->d_model != kD || cfg->enc_embedding_dim != kD || cfg->dff != kD)
    return fail(MI355ASR_EINVAL, "Punc: d_model=%d enc_embedding_dim=%d dff=%d, supported is 64 / 64 / 64", cfg->d_model, cfg->enc_embedding_dim, cfg->dff);
  if (cfg->num_heads != kHeads) return fail(MI355ASR_EINVAL, "Punc: num_heads=%d, supported is 8 heads of 8", cfg->num_heads);
  if (cfg->num_layers < 1 || cfg->num_layers > 6) return fail(MI355ASR_EINVAL, "Punc: num_layers=%d, supported is 1 .. 6", cfg->num_layers);
  if (cfg->classes < 1 || cfg->classes > kMaxClasses) return fail(MI355ASR_EINVAL, "Punc: classes=%d, supported is 1 .. %d", cfg->classes, kMaxClasses);
  if (cfg->vocab < 1 || cfg->vocab > (1 << 24)) return fail(MI355ASR_EINVAL, "Punc: vocab=%d must be in 1 .. 2^24", cfg->vocab);
  if (cfg->pe_input < 1 || cfg->pe_input > kMaxTokens) return fail(MI355ASR_EINVAL, "Punc: pe_input=%d, supported is 1 .. %d", cfg->pe_input, kMaxTokens);
  auto* m = new mi355asr_model();
  m->is_punc = true;
  m->pcfg = *cfg;
  std::memset(&m->cfg, 0, sizeof(m->cfg));
  std::memset(&m->dm, 0, sizeof(m->dm));
  auto& ex = m->expected;
  ex.push_back({"embedding", {cfg->vocab, kD}});
  ex.push_back({"pos_encoding", {cfg->pe_input, kD}});
  add_dense(ex, "encoder/dense", kD, kD);
  for (int i = 0; i < cfg->num_layers; ++i) {
    add_layer(ex, "encoder/layer_" + std::to_string(i));
    ex.push_back({"encoder/conv_" + std::to_string(i) + "/kernel", {3, kD, kD}});
    ex.push_back({"encoder/conv_" + std::to_string(i) + "/bias", {kD}});
  }
  add_dense(ex, "to_bert", kD, 768);
  add_dense(ex, "to_hidden", 768, kD);
  for (int i = 0; i < map_layers(cfg->num_layers); ++i) add_layer(ex, "map/layer_" + std::to_string(i));
  add_dense(ex, "final", kD, cfg->classes);
  for (const auto& e : ex) m->host[e.name] = HostTensor{};
  // the large-LDS attribute, once; a process without a device yet (or at all) gets it at its first forward instead
  (void)allow_lds();
  *out = m;
  return 0;
}

int mi355asr_punc_limits(const mi355asr_model* m, int32_t* lds_tokens, int32_t* max_tokens) {
  if (!m || !m->is_punc) return fail(MI355ASR_EINVAL, "not a Punc handle");
  if (lds_tokens) *lds_tokens = std::min(kLdsTokens, (int)m->pcfg.pe_input);
  if (max_tokens) *max_tokens = m->pcfg.pe_input;
  return 0;
}

int mi355asr_punc_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes) {
  if (!m || !m->is_punc || !bytes) return fail(MI355ASR_EINVAL, "not a Punc handle / null argument");
  if (B < 1 || T < 1) return fail(MI355ASR_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  if (T > m->pcfg.pe_input) return fail(MI355ASR_EINVAL, "T=%d exceeds pe_input=%d", T, m->pcfg.pe_input);
  *bytes = T > kLdsTokens ? (size_t)B * ws_row_floats(T) * sizeof(float) : 0;
  return 0;
}

// the checks and the launch both entry points share; `a` arrives with its output pointers set, heads = punc_heads_kernel
static int punc_launch(mi355asr_model* m, const int32_t* ids, const int32_t* lens, int32_t B, int32_t T, PuncArgs a, bool heads,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (B < 1 || T < 1) return fail(MI355ASR_EINVAL, "B and T must be positive (got %d, %d)", B, T);
  if (T > m->pcfg.pe_input) return fail(MI355ASR_EINVAL, "T=%d exceeds the longest sentence (pe_input=%d)", T, m->pcfg.pe_input);
  if (!ids || (!heads && !a.probs)) return fail(MI355ASR_EINVAL, "null argument");
  size_t need = 0;
  if (int rc = mi355asr_punc_workspace_bytes(m, B, T, &need)) return rc;
  if (need && (!ws || ws_bytes < need)) return fail(MI355ASR_EWORKSPACE, "workspace of %zu bytes, need %zu", ws_bytes, need);
  if (need && ((uintptr_t)ws & 15)) return fail(MI355ASR_EWORKSPACE, "workspace must be 16-byte aligned");
  const size_t lds = lds_bytes_for(T);
  if (lds > 64 * 1024 && allow_lds() != 0) return fail(MI355ASR_EHIP, "%s: cannot raise the dynamic LDS limit to %zu bytes", heads ? "punc_heads_kernel" : "punc_kernel", kLdsBudget);
  const auto& c = m->pcfg;
  a.ids = ids; a.lens = lens; a.w = m->arena;
  a.ws = (float*)ws; a.ws_row = ws_row_floats(T);
  a.n_enc = c.num_layers; a.n_map = map_layers(c.num_layers);
  a.o_conv = kDenseFloats + (size_t)a.n_enc * kLayerFloats;
  a.o_fold = a.o_conv + (size_t)a.n_enc * kConvFloats;
  a.o_map = a.o_fold + kDenseFloats;
  a.o_head = a.o_map + (size_t)a.n_map * kLayerFloats;
  a.o_emb = a.o_head + kDenseFloats;
  a.o_pe = a.o_emb + (size_t)c.vocab * kD;
  a.o_bert = a.o_pe + (size_t)c.pe_input * kD;
  a.B = B; a.T = T; a.vocab = c.vocab; a.classes = c.classes;
  if (heads)
    hipLaunchKernelGGL(punc_heads_kernel, dim3((unsigned)B), dim3(kThreads), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(punc_kernel, dim3((unsigned)B), dim3(kThreads), lds, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch %s: %s", heads ? "punc_heads_kernel" : "punc_kernel", hipGetErrorString(e));
  return 0;
}

int mi355asr_punc_forward(mi355asr_model* m, const int32_t* ids, const int32_t* lens, int32_t B, int32_t T, float* probs,
                          int32_t* cls, float* pmax, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !m->is_punc) return fail(MI355ASR_EINVAL, "not a Punc handle");
  PuncArgs a{};
  a.probs = probs; a.cls = cls; a.pmax = pmax;
  return punc_launch(m, ids, lens, B, T, a, false, ws, ws_bytes, stream);
}

int mi355asr_punc_heads_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes) {
  return mi355asr_punc_workspace_bytes(m, B, T, bytes);
}

int mi355asr_punc_heads(mi355asr_model* m, const int32_t* ids, const int32_t* lens, int32_t B, int32_t T, float* logits, float* feature,
                        void* ws, size_t ws_bytes, void* stream) {
  if (!m || !m->is_punc) return fail(MI355ASR_EINVAL, "not a Punc handle");
  if (!logits && !feature) return fail(MI355ASR_EINVAL, "punc_heads: logits_dev and feature_dev are both null");
  PuncArgs a{};
  a.logits = logits; a.feature = feature;
  return punc_launch(m, ids, lens, B, T, a, true, ws, ws_bytes, stream);
}
}  // extern "C"
