// The punctuation trainer's losses (punc_recover/trainer/punc_trainer.py:93-126) with their gradients with respect to the model's
// two outputs: PuncTrainer.classes_loss and classes_acc behind mi355asr_punc_classes_loss, PuncTrainer.bert_feature_loss behind
// mi355asr_masked_feature_mse (include/mi355asr.h).  Model-independent.
//
// punc_classes_kernel: one workgroup per sentence, a lane owns a token.  The class axis is at most 64 wide (kMaxClasses of
//   punc.hip; the shipped model has a handful of classes), so a token's row is a few dwords that one lane walks three times --
//   maximum and arg-max, the float64 sum of exp(x - max), and on request the gradient -- out of L1; the rows of a wave's 64 tokens
//   are adjacent in memory, so the wave's loads cover whole cache lines between them.  A token with label 0 takes no part and
//   its logits are not read.  The thread adds its tokens t = tid, tid + 256, ... in ascending order, the 64 lanes are added by a
//   fixed butterfly, the four waves as (w0 + w1) + (w2 + w3): five float64 sums (xe m, m, xe m1, m1, hit m) -> loss[b], acc[b].
//   The gradient pass follows in the same launch from the row's own counts and writes every element of [T, C].
// punc_acc_mean_kernel: one wave; the batch mean of acc in float64, lane-strided then the butterfly.  A kernel boundary and not
//   an in-launch hand-off between workgroups: the operand is B floats.
// feature_rows_kernel: one wave per token row (b, t).  Lane l takes the element quads l, l + 64, ... of the row (a quad is the
//   elements 4 q .. 4 q + 3 below F, counted from the row's start, whatever the row's address): one 16-byte load per operand where
//   both rows are 16-byte aligned, dword loads of the same elements otherwise and for the tail -- so the order of the sum does
//   not depend on the alignment.  Squares and counts are float64; the row's value goes to the workspace.  On request the wave
//   reads its row again (6 KB at F = 768: L1 / L2) and writes the gradient, 16 bytes per lane where the gradient row is aligned.
// feature_reduce_kernel: one wave per sentence adds the row values t = lane, lane + 64, ... in ascending order, then the butterfly.
// Nothing depends on timing (no atomics), and a sentence is computed from its own elements alone: a row of a batch equals the row
// alone bit for bit.
#include "common.h"
#include "model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerGroup = kThreads / 64;
constexpr int kMaxClasses = 64;                          // kMaxClasses of punc.hip

struct ClassesArgs {
  const int32_t* labels;   // (b, t) at labels + b ld_lab + t
  const float* x;          // (b, t, c) at x + b ld_b + t ld_t + c
  const float* upstream;   // [B] or null (ones)
  float* loss;             // [B]
  float* acc;              // [B]
  float* grad;             // (b, t, c) at grad + b gld_b + t gld_t + c, or null
  int64_t ld_lab, ld_b, ld_t, gld_b, gld_t;
  int B, Q, T, C;          // Q = min(T, label columns)
};

// max, arg-max (the lowest index on a tie) and the float64 sum of exp(x - max) of one token
DEV void token_stats(const float* row, int C, float* mx, int* am, double* se) {
  float m = row[0];
  int k = 0;
  for (int c = 1; c < C; ++c) {
    const float v = row[c];
    if (v > m) { m = v; k = c; }
  }
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += exp((double)row[c] - (double)m);
  *mx = m; *am = k; *se = s;
}

__global__ __launch_bounds__(kThreads) void punc_classes_kernel(ClassesArgs a) {
  __shared__ double sh[kWavesPerGroup][5];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* lab = a.labels + (int64_t)b * a.ld_lab;
  const float* xb = a.x + (int64_t)b * a.ld_b;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};    // sum xe m, sum m, sum xe m1, sum m1, sum hit m
  for (int t = tid; t < a.Q; t += kThreads) {
    const int y = lab[t];
    if (y == 0) continue;
    double xe = __builtin_nan("");
    bool hit = false;
    if (y > 0 && y < a.C) {
      const float* row = xb + (int64_t)t * a.ld_t;
      float mx; int am; double se;
      token_stats(row, a.C, &mx, &am, &se);
      xe = log(se) + ((double)mx - (double)row[y]);
      hit = am == y;
    }
    s[0] += xe; s[1] += 1.0;
    if (y != 1) { s[2] += xe; s[3] += 1.0; }
    if (hit) s[4] += 1.0;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = wave_sum(s[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) sh[tid >> 6][i] = s[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 5; ++i) s[i] = (sh[0][i] + sh[1][i]) + (sh[2][i] + sh[3][i]);
  const double w_all = 1.0 / (s[1] + 1e-6), w_other = 1.0 / (s[3] + 1e-6);
  if (tid == 0) {
    a.loss[b] = (float)(s[0] * w_all + s[2] * w_other);
    a.acc[b] = (float)(s[4] / s[1]);           // no epsilon, as the reference has none: NaN for a row without a label
  }
  if (!a.grad) return;
  const double up = a.upstream ? (double)a.upstream[b] : 1.0;
  float* gb = a.grad + (int64_t)b * a.gld_b;
  for (int t = tid; t < a.T; t += kThreads) {
    float* g = gb + (int64_t)t * a.gld_t;
    const int y = t < a.Q ? lab[t] : 0;
    if (y <= 0 || y >= a.C) {
      for (int c = 0; c < a.C; ++c) g[c] = 0.f;
      continue;
    }
    const float* row = xb + (int64_t)t * a.ld_t;
    float mx; int am; double se;
    token_stats(row, a.C, &mx, &am, &se);
    const double w = up * (w_all + (y != 1 ? w_other : 0.0));
    const double scale = w / se;
    for (int c = 0; c < a.C; ++c) g[c] = (float)(exp((double)row[c] - (double)mx) * scale - (c == y ? w : 0.0));
  }
}

__global__ __launch_bounds__(64) void punc_acc_mean_kernel(const float* acc, int B, float* mean) {
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) s += (double)acc[b];
  s = wave_sum(s);
  if (threadIdx.x == 0) *mean = (float)(s / (double)B);
}

struct FeatureArgs {
  const float* real;       // (b, t, f) at real + b rld_b + t rld_t + f
  const float* pred;
  const float* upstream;   // [B] or null (ones)
  double* rows;            // [B, T] the row values
  float* grad;             // (b, t, f) at grad + b gld_b + t gld_t + f, t < T2; or null
  int64_t rld_b, rld_t, pld_b, pld_t, gld_b, gld_t;
  int B, T, T2, F;         // T = min(T1, T2)
};

// the quad q of a row: the elements 4 q .. 4 q + 3 below F; one 16-byte load when `wide` and the quad is whole.  Elements at or
// past F read as -10 / 0: masked out
DEV void load_quad(const float* r, const float* p, int q, int F, bool wide, float (&rv)[4], float (&pv)[4]) {
  const int f0 = 4 * q;
  if (wide && f0 + 4 <= F) {
    const f32x4 a = ldg4(r + f0), c = ldg4(p + f0);
    rv[0] = a.x; rv[1] = a.y; rv[2] = a.z; rv[3] = a.w;
    pv[0] = c.x; pv[1] = c.y; pv[2] = c.z; pv[3] = c.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = f0 + j < F;
      rv[j] = in ? r[f0 + j] : -10.f;
      pv[j] = in ? p[f0 + j] : 0.f;
    }
  }
}

__global__ __launch_bounds__(kThreads) void feature_rows_kernel(FeatureArgs a) {
  const int lane = threadIdx.x & 63;
  const int TR = a.grad ? a.T2 : a.T;        // the gradient has the prediction's rows; those at or past T are zeros
  const int64_t row = (int64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (row >= (int64_t)a.B * TR) return;
  const int b = (int)(row / TR), t = (int)(row - (int64_t)b * TR);
  const int F = a.F, nq = (F + 3) / 4;
  float* g = a.grad ? a.grad + (int64_t)b * a.gld_b + (int64_t)t * a.gld_t : nullptr;
  const bool gwide = ((uintptr_t)g & 15) == 0;
  if (t >= a.T) {
    for (int q = lane; q < nq; q += 64) {
      if (gwide && 4 * q + 4 <= F) stg4(g + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});
      else
        for (int f = 4 * q; f < F && f < 4 * q + 4; ++f) g[f] = 0.f;
    }
    return;
  }
  const float* r = a.real + (int64_t)b * a.rld_b + (int64_t)t * a.rld_t;
  const float* p = a.pred + (int64_t)b * a.pld_b + (int64_t)t * a.pld_t;
  const bool wide = (((uintptr_t)r | (uintptr_t)p) & 15) == 0;      // the same in every lane: a wave has one row
  double num = 0.0, cnt = 0.0;
  for (int q = lane; q < nq; q += 64) {
    float rv[4], pv[4];
    load_quad(r, p, q, F, wide, rv, pv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)rv[j] - (double)pv[j];
      if (rv[j] != -10.f) { num += d * d; cnt += 1.0; }
    }
  }
  num = wave_sum(num);
  cnt = wave_sum(cnt);
  const double den = cnt + 1e-6;
  if (lane == 0) a.rows[(int64_t)b * a.T + t] = num / den;
  if (!g) return;
  const double coef = (a.upstream ? (double)a.upstream[b] : 1.0) * 2.0 / (den * (double)a.T);
  for (int q = lane; q < nq; q += 64) {
    float rv[4], pv[4], gv[4];
    load_quad(r, p, q, F, wide, rv, pv);
#pragma unroll
    for (int j = 0; j < 4; ++j) gv[j] = rv[j] != -10.f ? (float)(coef * ((double)pv[j] - (double)rv[j])) : 0.f;
    if (gwide && 4 * q + 4 <= F) stg4(g + 4 * q, f32x4{gv[0], gv[1], gv[2], gv[3]});
    else
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < F) g[4 * q + j] = gv[j];
  }
}

__global__ __launch_bounds__(64) void feature_reduce_kernel(const double* rows, int T, float* out) {
  const int b = blockIdx.x;
  double s = 0.0;
  for (int t = threadIdx.x; t < T; t += 64) s += rows[(int64_t)b * T + t];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[b] = (float)(s / (double)T);
}

size_t feature_ws_bytes(int B, int T) { return align256((size_t)B * T * sizeof(double)); }

}  // namespace

extern "C" {

int mi355asr_punc_classes_loss(const int32_t* labels_dev, int64_t ld_lab, const float* logits_dev, int64_t ld_b, int64_t ld_t,
                               const float* upstream_dev, int32_t B, int32_t Q, int32_t T, int32_t C, float* loss_dev,
                               float* acc_dev, float* acc_mean_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* stream) {
  if (!labels_dev) return fail(MI355ASR_EINVAL, "punc_classes_loss: null pointer labels_dev");
  if (!logits_dev) return fail(MI355ASR_EINVAL, "punc_classes_loss: null pointer logits_dev");
  if (!loss_dev || !acc_dev || !acc_mean_dev) return fail(MI355ASR_EINVAL, "punc_classes_loss: null output pointer (loss_dev, acc_dev, acc_mean_dev)");
  if (C < 1 || C > kMaxClasses) return fail(MI355ASR_EINVAL, "punc_classes_loss: C=%d classes, supported is 1 .. %d", C, kMaxClasses);
  if (B < 1 || Q < 1 || T < 1 || (int64_t)B * T > kMaxExtent32)
    return fail(MI355ASR_EINVAL, "punc_classes_loss: need B, Q, T >= 1 and B * T < 2^31 - 65536 (got %d, %d, %d)", B, Q, T);
  const int Qu = std::min(Q, T);
  if (ld_lab < 0 || ld_b < 0 || (B > 1 && (ld_lab < Qu || ld_b < C)) || (Qu > 1 && ld_t < C))
    return fail(MI355ASR_EINVAL, "punc_classes_loss: the strides ld_lab=%lld, ld_b=%lld, ld_t=%lld let rows overlap (Q'=%d, C=%d)",
                (long long)ld_lab, (long long)ld_b, (long long)ld_t, Qu, C);
  if (grad_dev && ((T > 1 && gld_t < C) || (B > 1 && gld_b < C) || gld_b < 0))
    return fail(MI355ASR_EINVAL, "punc_classes_loss: gld_b=%lld, gld_t=%lld let the gradient rows overlap", (long long)gld_b, (long long)gld_t);
  ClassesArgs a{};
  a.labels = labels_dev; a.x = logits_dev; a.upstream = upstream_dev; a.loss = loss_dev; a.acc = acc_dev; a.grad = grad_dev;
  a.ld_lab = ld_lab; a.ld_b = ld_b; a.ld_t = ld_t; a.gld_b = gld_b; a.gld_t = gld_t;
  a.B = B; a.Q = Qu; a.T = T; a.C = C;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(punc_classes_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(punc_acc_mean_kernel, dim3(1), dim3(64), 0, s, (const float*)acc_dev, (int)B, acc_mean_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_masked_feature_mse_workspace_bytes(int32_t B, int32_t T1, int32_t T2, size_t* bytes) {
  if (!bytes) return fail(MI355ASR_EINVAL, "masked_feature_mse: null pointer bytes");
  if (B < 1 || T1 < 1 || T2 < 1 || (int64_t)B * std::max(T1, T2) > kMaxExtent32)
    return fail(MI355ASR_EINVAL, "masked_feature_mse: need B, T1, T2 >= 1 and B * max(T1, T2) < 2^31 - 65536 (got %d, %d, %d)", B, T1, T2);
  *bytes = feature_ws_bytes(B, std::min(T1, T2));
  return 0;
}

int mi355asr_masked_feature_mse(const float* real_dev, int64_t rld_b, int64_t rld_t, const float* pred_dev, int64_t pld_b,
                                int64_t pld_t, const float* upstream_dev, int32_t B, int32_t T1, int32_t T2, int32_t F,
                                float* out_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* ws_dev, size_t ws_bytes,
                                void* stream) {
  if (!real_dev) return fail(MI355ASR_EINVAL, "masked_feature_mse: null pointer real_dev");
  if (!pred_dev) return fail(MI355ASR_EINVAL, "masked_feature_mse: null pointer pred_dev");
  if (!out_dev) return fail(MI355ASR_EINVAL, "masked_feature_mse: null pointer out_dev");
  size_t need = 0;
  if (int rc = mi355asr_masked_feature_mse_workspace_bytes(B, T1, T2, &need)) return rc;
  if (F < 1) return fail(MI355ASR_EINVAL, "masked_feature_mse: F=%d must be positive", F);
  const int T = std::min(T1, T2);
  if (rld_b < 0 || pld_b < 0 || (T > 1 && (rld_t < F || pld_t < F)) || (B > 1 && (rld_b < F || pld_b < F)))
    return fail(MI355ASR_EINVAL, "masked_feature_mse: the strides (%lld, %lld) of real, (%lld, %lld) of pred let rows of F=%d overlap",
                (long long)rld_b, (long long)rld_t, (long long)pld_b, (long long)pld_t, F);
  if (grad_dev && (gld_b < 0 || (T2 > 1 && gld_t < F) || (B > 1 && gld_b < F)))
    return fail(MI355ASR_EINVAL, "masked_feature_mse: gld_b=%lld, gld_t=%lld let the gradient rows overlap", (long long)gld_b, (long long)gld_t);
  if (!ws_dev || ((uintptr_t)ws_dev & 7)) return fail(MI355ASR_EWORKSPACE, "masked_feature_mse: the workspace is null or not 8-byte aligned");
  if (ws_bytes < need) return fail(MI355ASR_EWORKSPACE, "masked_feature_mse: workspace of %zu bytes, need %zu", ws_bytes, need);
  FeatureArgs a{};
  a.real = real_dev; a.pred = pred_dev; a.upstream = upstream_dev; a.rows = (double*)ws_dev; a.grad = grad_dev;
  a.rld_b = rld_b; a.rld_t = rld_t; a.pld_b = pld_b; a.pld_t = pld_t; a.gld_b = gld_b; a.gld_t = gld_t;
  a.B = B; a.T = T; a.T2 = T2; a.F = F;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * (grad_dev ? T2 : T);
  hipLaunchKernelGGL(feature_rows_kernel, dim3((unsigned)((rows + kWavesPerGroup - 1) / kWavesPerGroup)), dim3(kThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(feature_reduce_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)ws_dev, (int)T, out_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
