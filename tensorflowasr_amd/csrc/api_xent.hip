// Softmax cross-entropy, the trainer's mask_loss / translate_acc and their gradient behind the C ABI (kernels: xent.hip).
// Model-independent, like mi355asr_ctc_loss.  Every argument is checked before the first device call; nothing here allocates,
// copies to the host or waits for the stream.
#include "model.h"
#include "xent.h"

namespace mi355 {
namespace {

struct XentPlan {
  size_t loss, amax, w, total;
};
XentPlan xent_plan(size_t B, size_t Q, bool want_grad) {
  XentPlan p{};
  size_t o = 0;
  p.loss = o; o += align256(B * Q * sizeof(float));
  p.amax = o; o += align256(B * Q * sizeof(int32_t));
  p.w = o; o += want_grad ? align256(B * Q * sizeof(float)) : 0;
  p.total = o;
  return p;
}

int xent_sizes_ok(int32_t B, int32_t Q) {
  if (B < 1 || Q < 1) return fail(MI355ASR_EINVAL, "xent: B and Q must be positive (B=%d Q=%d)", B, Q);
  if ((int64_t)B * Q > kXentMaxRows) return fail(MI355ASR_EINVAL, "xent: B * Q = %lld rows, built for up to %lld", (long long)B * Q, (long long)kXentMaxRows);
  return 0;
}

int xent_dims_ok(int32_t B, int32_t Q, int32_t V, int64_t ld_b, int64_t ld_t, int32_t ld_lab, bool has_grad, int64_t gld_b,
                 int64_t gld_t) {
  if (int rc = xent_sizes_ok(B, Q)) return rc;
  if (V < 1 || V > kXentMaxV) return fail(MI355ASR_EINVAL, "xent: V=%d classes, built for 1 .. %d", V, kXentMaxV);
  if (ld_t < V) return fail(MI355ASR_EINVAL, "xent: ld_t=%lld is smaller than V=%d", (long long)ld_t, V);
  if (ld_b < 0) return fail(MI355ASR_EINVAL, "xent: ld_b=%lld is negative", (long long)ld_b);
  if (ld_lab < Q) return fail(MI355ASR_EINVAL, "xent: ld_lab=%d is smaller than Q=%d", ld_lab, Q);
  if (has_grad) {
    if (gld_t < V) return fail(MI355ASR_EINVAL, "xent: gld_t=%lld is smaller than V=%d", (long long)gld_t, V);
    if (B > 1 && gld_b < (int64_t)(Q - 1) * gld_t + V)
      return fail(MI355ASR_EINVAL, "xent: gld_b=%lld lets the gradient rows of two batch entries overlap", (long long)gld_b);
  }
  return 0;
}

}  // namespace
}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355asr_xent_workspace_bytes(int32_t B, int32_t Q, int32_t want_grad, size_t* bytes) {
  if (!bytes) return fail(MI355ASR_EINVAL, "xent: null pointer bytes");
  if (int rc = xent_sizes_ok(B, Q)) return rc;
  *bytes = xent_plan(B, Q, want_grad != 0).total;
  return 0;
}

int mi355asr_xent_rows(const float* x_dev, int64_t ld_b, int64_t ld_t, const int32_t* labels_dev, int32_t ld_lab,
                       const float* weights_dev, int32_t B, int32_t Q, int32_t V, float* loss_dev, int32_t* argmax_dev,
                       float* grad_dev, int64_t gld_b, int64_t gld_t, void* stream) {
  if (!x_dev) return fail(MI355ASR_EINVAL, "xent_rows: null pointer x_dev");
  if (!labels_dev) return fail(MI355ASR_EINVAL, "xent_rows: null pointer labels_dev");
  if (!loss_dev) return fail(MI355ASR_EINVAL, "xent_rows: null pointer loss_dev");
  if (int rc = xent_dims_ok(B, Q, V, ld_b, ld_t, ld_lab, grad_dev != nullptr, gld_b, gld_t)) return rc;
  XentRowsArgs r{};
  r.x = x_dev; r.ld_b = ld_b; r.ld_t = ld_t; r.labels = labels_dev; r.ld_lab = ld_lab; r.w = weights_dev;
  r.B = B; r.Q = Q; r.V = V; r.loss = loss_dev; r.amax = argmax_dev; r.grad = grad_dev; r.gld_b = gld_b; r.gld_t = gld_t;
  launch_xent_rows(r, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mi355asr_mask_loss(const float* x_dev, int64_t ld_b, int64_t ld_t, const int32_t* labels_dev, int32_t ld_lab,
                       const float* upstream_dev, int32_t B, int32_t Q, int32_t V, float* mask_loss_dev, float* acc_dev,
                       float* mean_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* ws_dev, size_t ws_bytes,
                       void* stream) {
  if (!x_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer x_dev");
  if (!labels_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer labels_dev");
  if (!mask_loss_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer mask_loss_dev");
  if (!acc_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer acc_dev");
  if (!mean_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer mean_dev");
  if (!ws_dev) return fail(MI355ASR_EINVAL, "mask_loss: null pointer ws_dev");
  if (int rc = xent_dims_ok(B, Q, V, ld_b, ld_t, ld_lab, grad_dev != nullptr, gld_b, gld_t)) return rc;
  if ((uintptr_t)ws_dev & 7) return fail(MI355ASR_EINVAL, "mask_loss: misaligned workspace ws_dev");
  const XentPlan p = xent_plan(B, Q, grad_dev != nullptr);
  if (ws_bytes < p.total) return fail(MI355ASR_EINVAL, "mask_loss: workspace too small: ws_bytes %zu < %zu bytes", ws_bytes, p.total);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws_dev;
  XentBatchArgs m{};
  m.labels = labels_dev; m.ld_lab = ld_lab; m.B = B; m.Q = Q;
  m.upstream = upstream_dev; m.w = grad_dev ? (float*)(w + p.w) : nullptr;
  m.loss = (float*)(w + p.loss); m.amax = (int32_t*)(w + p.amax);
  m.mask_loss = mask_loss_dev; m.acc = acc_dev; m.mean = mean_dev;
  if (grad_dev) {
    launch_xent_weights(m, s);
    HIP_TRY(hipGetLastError());
  }
  XentRowsArgs r{};
  r.x = x_dev; r.ld_b = ld_b; r.ld_t = ld_t; r.labels = labels_dev; r.ld_lab = ld_lab; r.w = m.w;
  r.B = B; r.Q = Q; r.V = V; r.loss = (float*)(w + p.loss); r.amax = (int32_t*)(w + p.amax);
  r.grad = grad_dev; r.gld_b = gld_b; r.gld_t = gld_t;
  launch_xent_rows(r, s);
  HIP_TRY(hipGetLastError());
  launch_xent_reduce(m, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
