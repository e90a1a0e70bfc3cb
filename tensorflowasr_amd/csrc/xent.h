// Softmax cross-entropy kernels (xent.hip) as the host side (api_xent.hip) sees them: argument blocks, the built limits, launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mi355 {

constexpr int kXentThreads = 256;                              // one workgroup per row of V logits
constexpr int kXentSlots = 10;                                 // float4 per thread kept in registers between the passes
constexpr int kXentResidentV = kXentThreads * 4 * kXentSlots;  // 10 240: rows up to here are read once; longer ones again through L2
constexpr int kXentMaxV = 1 << 18;                             // 262 144 classes: 256 float4 per thread, the depth the error bound is stated for
constexpr int64_t kXentMaxRows = (int64_t)1 << 30;             // B * Q: one workgroup each

// Row stage: per (b, t < Q) the loss lse(x) - x[y], the arg-max and, with grad, w * (softmax(x) - onehot(y)).
struct XentRowsArgs {
  const float* x;             // logits, row (b, t) at x + b * ld_b + t * ld_t
  int64_t ld_b, ld_t;
  const int32_t* labels;      // label of (b, t) at labels + b * ld_lab + t
  int32_t ld_lab;
  const float* w;             // [B, Q] per-row weight of the gradient, or nullptr (= 1)
  int32_t B, Q, V;
  float* loss;                // [B, Q]
  int32_t* amax;              // [B, Q] or nullptr
  float* grad;                // row (b, t) at grad + b * gld_b + t * gld_t, or nullptr
  int64_t gld_b, gld_t;
};

// Batch stage: one workgroup; float64 sums in a fixed order.
struct XentBatchArgs {
  const int32_t* labels;      // as above
  int32_t ld_lab;
  int32_t B, Q;
  // weights entry
  const float* upstream;      // [B] or nullptr (= 1)
  float* w;                   // [B, Q]: g_b / Q + G need / (N_need + 1e-6) + G zero / (N_zero + 1e-6), G = sum of g
  // reductions entry
  const float* loss;          // [B, Q]
  const int32_t* amax;        // [B, Q]
  float* mask_loss;           // [B]
  float* acc;                 // scalar
  float* mean;                // scalar
};

void launch_xent_rows(const XentRowsArgs& a, hipStream_t s);
void launch_xent_weights(const XentBatchArgs& a, hipStream_t s);
void launch_xent_reduce(const XentBatchArgs& a, hipStream_t s);

}  // namespace mi355
