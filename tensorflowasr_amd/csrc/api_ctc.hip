// CTC loss, its gradient and forced alignment behind the C ABI (kernels: ctc_lattice.hip).  Model-independent, like mi355asr_ctc_greedy.
// Every argument is checked before the first device call; nothing here allocates, copies to the host or waits for the stream.
#include "model.h"
#include "ctc_lattice.h"

namespace mi355 {
namespace {

struct CtcLossPlan {
  size_t lp, stat, logp, feasible, norm, ab, chain, total;
};
CtcLossPlan loss_plan(size_t B, size_t T, size_t U, bool want_grad) {
  CtcLossPlan p{};
  size_t o = 0;
  p.lp = o; o += align256(B * T * (U + 1) * sizeof(float));
  p.stat = o; o += align256(B * T * 2 * sizeof(float));
  p.logp = o; o += align256(B * sizeof(double));
  p.feasible = o; o += align256(B * sizeof(int32_t));
  if (want_grad) {
    p.norm = o; o += align256(2 * B * T * sizeof(double));
    p.ab = o; o += align256(2 * B * T * (2 * U + 1) * sizeof(float));
    p.chain = o; o += align256(B * std::max<size_t>(U, 1) * sizeof(int32_t));
  }
  p.total = o;
  return p;
}

struct CtcAlignPlan {
  size_t lp, bp, total;
};
CtcAlignPlan align_plan(size_t B, size_t T, size_t U) {
  CtcAlignPlan p{};
  p.lp = 0;
  p.bp = align256(B * T * (U + 1) * sizeof(float));
  p.total = p.bp + align256(B * T * (2 * U + 1));
  return p;
}

int ctc_dims_ok(int32_t B, int32_t T, int32_t V, int32_t U) {
  if (B <= 0 || T <= 0 || U < 0) return fail(MI355ASR_EINVAL, "ctc: B and T must be positive and U >= 0 (B=%d T=%d U=%d)", B, T, U);
  if (V < 2) return fail(MI355ASR_EINVAL, "ctc: V=%d, need at least one class and the blank", V);
  if (U > kCtcMaxU) return fail(MI355ASR_EINVAL, "ctc: U=%d label positions, the lattice kernel is built for up to %d", U, kCtcMaxU);
  return 0;
}

}  // namespace
}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355asr_ctc_loss_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t U, int32_t want_grad, size_t* bytes) {
  if (!bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = ctc_dims_ok(B, T, V, U)) return rc;
  *bytes = loss_plan(B, T, U, want_grad != 0).total;
  return 0;
}

int mi355asr_ctc_loss(const float* x, int32_t is_logits, const int32_t* in_len, const int32_t* labels, const int32_t* label_len,
                      int32_t B, int32_t T, int32_t V, int32_t U, int32_t blank, float* loss, float* grad, void* ws,
                      size_t ws_bytes, void* stream) {
  if (int rc = ctc_dims_ok(B, T, V, U)) return rc;
  if (blank < 0 || blank >= V) return fail(MI355ASR_EINVAL, "ctc: blank=%d outside [0, %d)", blank, V);
  if (!loss) return fail(MI355ASR_EINVAL, "ctc_loss: null loss output");
  if (!x || !label_len || (U > 0 && !labels) || !ws) return fail(MI355ASR_EINVAL, "ctc_loss: null pointer");
  if (grad && !is_logits)
    return fail(MI355ASR_EINVAL, "ctc_loss: the gradient is with respect to logits; the probabilities entry returns the loss only");
  const CtcLossPlan p = loss_plan(B, T, U, grad != nullptr);
  if (ws_bytes < p.total) return fail(MI355ASR_EINVAL, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  CtcRowArgs r{};
  r.x = x; r.in_len = in_len; r.labels = labels; r.label_len = label_len;
  r.lp = (float*)(w + p.lp); r.stat = (float*)(w + p.stat);
  r.B = B; r.T = T; r.V = V; r.U = U; r.blank = blank; r.is_logits = is_logits != 0;
  r.log_den = (float)std::log1p((double)V * 1e-7);
  LAUNCH_TRY(launch_ctc_rows(r, s), "ctc rows");
  CtcLatticeArgs l{};
  l.lp = r.lp; l.in_len = in_len; l.labels = labels; l.label_len = label_len;
  l.B = B; l.T = T; l.V = V; l.U = U; l.blank = blank;
  l.logp = (double*)(w + p.logp); l.feasible = (int32_t*)(w + p.feasible); l.loss = loss;
  if (grad) {
    l.ab = (float*)(w + p.ab); l.norm = (double*)(w + p.norm); l.chain = (int32_t*)(w + p.chain);
  }
  LAUNCH_TRY(launch_ctc_lattice(l, false, grad ? 2 : 1, s), "ctc lattice");
  if (grad) {
    CtcGradArgs g{};
    g.x = x; g.lp = r.lp; g.stat = r.stat; g.ab = l.ab; g.norm = l.norm; g.logp = l.logp; g.feasible = l.feasible;
    g.chain = l.chain; g.in_len = in_len; g.labels = labels; g.label_len = label_len; g.grad = grad;
    g.B = B; g.T = T; g.V = V; g.U = U; g.blank = blank;
    LAUNCH_TRY(launch_ctc_grad(g, s), "ctc gradient");
  }
  return 0;
}

int mi355asr_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t U, size_t* bytes) {
  if (!bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = ctc_dims_ok(B, T, V, U)) return rc;
  *bytes = align_plan(B, T, U).total;
  return 0;
}

int mi355asr_ctc_align(const float* x, int32_t is_logits, const int32_t* in_len, const int32_t* labels, const int32_t* label_len,
                       int32_t B, int32_t T, int32_t V, int32_t U, int32_t blank, int32_t* path, int32_t* spans, float* score,
                       void* ws, size_t ws_bytes, void* stream) {
  if (int rc = ctc_dims_ok(B, T, V, U)) return rc;
  if (blank < 0 || blank >= V) return fail(MI355ASR_EINVAL, "ctc: blank=%d outside [0, %d)", blank, V);
  if (!path || !score || (U > 0 && !spans)) return fail(MI355ASR_EINVAL, "ctc_align: null output");
  if (!x || !label_len || (U > 0 && !labels) || !ws) return fail(MI355ASR_EINVAL, "ctc_align: null pointer");
  const CtcAlignPlan p = align_plan(B, T, U);
  if (ws_bytes < p.total) return fail(MI355ASR_EINVAL, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  CtcRowArgs r{};
  r.x = x; r.in_len = in_len; r.labels = labels; r.label_len = label_len;
  r.lp = (float*)(w + p.lp); r.stat = nullptr;
  r.B = B; r.T = T; r.V = V; r.U = U; r.blank = blank; r.is_logits = is_logits != 0;
  r.log_den = (float)std::log1p((double)V * 1e-7);
  LAUNCH_TRY(launch_ctc_rows(r, s), "ctc rows");
  CtcLatticeArgs l{};
  l.lp = r.lp; l.in_len = in_len; l.labels = labels; l.label_len = label_len;
  l.B = B; l.T = T; l.V = V; l.U = U; l.blank = blank;
  l.bp = (uint8_t*)(w + p.bp); l.path = path; l.spans = spans; l.score = score;
  LAUNCH_TRY(launch_ctc_lattice(l, true, 1, s), "ctc alignment");
  return 0;
}

}  // extern "C"
