// CTC lattice kernels (ctc_lattice.hip) as the host side (api_ctc.hip) sees them: argument blocks, the built limit, launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mi355 {

constexpr int kCtcMaxU = 511;   // label positions per utterance: one thread per (blank, label) pair, 512 threads per workgroup

// Row stage: [B, T, V] -> log q of the U_b labels and of the blank, per frame t < in_len[b].
struct CtcRowArgs {
  const float* x;             // [B, T, V] logits (is_logits) or probabilities
  const int32_t* in_len;      // [B] or nullptr (= T)
  const int32_t* labels;      // [B, U]
  const int32_t* label_len;   // [B]
  float* lp;                  // [B, T, U + 1]: column u < U_b = log q[label u], column U = log q[blank]
  float* stat;                // [B, T, 2] (row maximum, sum of exp) of the logits, or nullptr
  int B, T, V, U, blank, is_logits;
  float log_den;              // logits: log(1 + V * 1e-7), the log of the sum of (p + 1e-7) over a softmax row
};

// Lattice stage: one workgroup per (utterance, direction).
struct CtcLatticeArgs {
  const float* lp;
  const int32_t* in_len;
  const int32_t* labels;
  const int32_t* label_len;
  int B, T, V, U, blank;
  // sum mode
  float* ab;                  // [2, B, T, 2U + 1] normalised log alpha / log beta (beta includes the frame's emission), or nullptr
  double* norm;               // [2, B, T] cumulative normalisers of ab, or nullptr
  double* logp;               // [B]
  int32_t* feasible;          // [B]
  int32_t* chain;             // [B, U]: (next position with the same label + 1) | first occurrence << 16, or nullptr
  float* loss;                // [B]
  // max mode
  uint8_t* bp;                // [B, T, 2U + 1] back-pointers: the step down in state index (0, 1, 2)
  int32_t* path;              // [B, T]
  int32_t* spans;             // [B, U, 2]
  float* score;               // [B]
};

// Gradient stage: d loss / d logits, one workgroup per row.
struct CtcGradArgs {
  const float* x;
  const float* lp;
  const float* stat;
  const float* ab;
  const double* norm;
  const double* logp;
  const int32_t* feasible;
  const int32_t* chain;
  const int32_t* in_len;
  const int32_t* labels;
  const int32_t* label_len;
  float* grad;                // [B, T, V]
  int B, T, V, U, blank;
};

int launch_ctc_rows(const CtcRowArgs& a, hipStream_t s);
int launch_ctc_lattice(const CtcLatticeArgs& a, bool viterbi, int directions, hipStream_t s);
int launch_ctc_grad(const CtcGradArgs& a, hipStream_t s);

}  // namespace mi355
