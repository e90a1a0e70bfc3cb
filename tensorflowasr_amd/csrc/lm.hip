// The n-gram language model of the prefix beam search's scorer: packing of the table (lm_table.h), its upload, and the
// verification entry point mi355asr_lm_score (host, or a kernel that runs the device search's own lm_cond).
// replaces: the KenLM model behind externals/ctc_decoders Scorer (scorer.cpp:55-93), character-based mode.
#include <memory>
#include <mutex>

#include "model.h"

struct mi355asr_lm {
  std::vector<LmCell> cells;
  std::vector<int32_t> class_word;
  LmView host{};
  int64_t n_ngrams = 0, n_words = 0;
  // per device: uploaded on first use
  mutable std::mutex mu;
  mutable LmCell* d_cells[64] = {};
  mutable int32_t* d_class_word[64] = {};
};

namespace {

__global__ __launch_bounds__(256) void lm_score_kernel(LmView v, const int32_t* __restrict__ ngrams, int n, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t r[kLmMaxOrder];
#pragma unroll
  for (int k = 0; k < kLmMaxOrder; ++k) r[k] = k < v.order ? ngrams[(size_t)i * v.order + (v.order - 1 - k)] : 0;
  out[i] = lm_cond(v, r);
}

// LM word of every entry of the top-n lists (so that the search prefetches it like the class itself)
__global__ __launch_bounds__(256) void lm_map_kernel(const int32_t* __restrict__ top_idx, size_t n, const int32_t* __restrict__ class_word,
                                                     int n_classes, int32_t* __restrict__ top_w) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int c = top_idx[i];
    top_w[i] = c >= 0 && c < n_classes ? class_word[c] : 0;      // the blank (class n_classes) is never scored
  }
}

}  // namespace

extern "C" {

const LmView* mi355asr_lm_host_view(const mi355asr_lm* lm) { return &lm->host; }
const int32_t* mi355asr_lm_class_word(const mi355asr_lm* lm, int* n_classes) {
  if (n_classes) *n_classes = (int)lm->class_word.size();
  return lm->class_word.data();
}

int mi355asr_lm_device_view(const mi355asr_lm* lm, LmView* view, const int32_t** class_word_dev) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  std::lock_guard<std::mutex> g(lm->mu);
  if (!lm->d_cells[dev]) {
    void *c = nullptr, *w = nullptr;
    const size_t nc = lm->cells.size() * sizeof(LmCell), nw = std::max<size_t>(1, lm->class_word.size()) * sizeof(int32_t);
    if (hipMalloc(&c, nc) != hipSuccess) return -1;
    if (hipMalloc(&w, nw) != hipSuccess) { (void)hipFree(c); return -1; }
    if (hipMemcpy(c, lm->cells.data(), nc, hipMemcpyHostToDevice) != hipSuccess ||
        (!lm->class_word.empty() && hipMemcpy(w, lm->class_word.data(), lm->class_word.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)) {
      (void)hipFree(c); (void)hipFree(w);
      return -1;
    }
    lm->d_cells[dev] = (LmCell*)c;
    lm->d_class_word[dev] = (int32_t*)w;
  }
  *view = lm->host;
  view->cells = lm->d_cells[dev];
  if (class_word_dev) *class_word_dev = lm->d_class_word[dev];
  return 0;
}

int mi355asr_launch_lm_map(const int32_t* top_idx, size_t n, const int32_t* class_word_dev, int n_classes, int32_t* top_w,
                           hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(lm_map_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, top_idx, n, class_word_dev,
                     n_classes, top_w);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int mi355asr_lm_create(int32_t order, const int64_t* counts, const int32_t* words, const float* logp, const float* backoff,
                       const int32_t* class_word, int32_t n_classes, int32_t bos_word, int32_t space_class, mi355asr_lm** out) {
  if (!counts || !words || !logp || !backoff || !out || (n_classes > 0 && !class_word)) return fail(MI355ASR_EINVAL, "null argument");
  if (order < 1 || order > kLmMaxOrder) return fail(MI355ASR_EINVAL, "language model order %d: 1 .. %d are supported", order, kLmMaxOrder);
  int64_t total = 0;
  for (int m = 0; m < order; ++m) {
    if (counts[m] < 0) return fail(MI355ASR_EINVAL, "negative n-gram count");
    total += counts[m];
  }
  const int64_t n_words = counts[0];
  if (n_words < 1 || n_words >= (1ll << 31) || total >= (1ll << 30)) return fail(MI355ASR_EINVAL, "language model: %lld unigrams, %lld n-grams", (long long)n_words, (long long)total);
  if (bos_word < 0 || bos_word > n_words || n_classes < 0 || space_class < -2 || space_class >= n_classes)
    return fail(MI355ASR_EINVAL, "language model: \"<s>\" word %d or space class %d out of range", bos_word, space_class);
  auto lm = std::make_unique<mi355asr_lm>();
  int bits = 0;
  while ((n_words >> bits) != 0) ++bits;
  int lg = 4;
  while ((1ll << lg) < 2 * total) ++lg;
  lm->cells.assign((size_t)1 << lg, LmCell{0, 0.f, 0.f});
  lm->host.cells = lm->cells.data();
  lm->host.shift = 64 - lg;
  lm->host.mask = (uint32_t)((1ull << lg) - 1);
  lm->host.order = order;
  lm->host.bits = bits * order <= 64 ? bits : 0;
  lm->host.bos = bos_word;
  lm->n_ngrams = total;
  lm->n_words = n_words;
  std::vector<char> seen((size_t)n_words + 1, 0);
  const int32_t* w = words;
  int64_t g = 0;
  for (int m = 1; m <= order; ++m) {
    for (int64_t i = 0; i < counts[m - 1]; ++i, w += m, ++g) {
      int32_t r[kLmMaxOrder];
      for (int k = 0; k < m; ++k) {
        r[k] = w[m - 1 - k];
        if (r[k] < 1 || r[k] > n_words) return fail(MI355ASR_EINVAL, "language model: word id %d outside [1, %lld] in %d-gram %lld", r[k], (long long)n_words, m, (long long)i);
      }
      if (m == 1) seen[r[0]] = 1;
      const uint64_t key = lm_key(lm->host, r, m);
      uint32_t s = lm_slot(lm->host, key);
      while (lm->cells[s].key != 0) {
        // packed keys are distinct by construction and hashed keys have to be: the same key twice is a repeated n-gram or a collision
        if (lm->cells[s].key == key) return fail(MI355ASR_EINVAL, "language model: %d-gram %lld has the key of an earlier n-gram (repeated entry, or a 64-bit hash collision)", m, (long long)i);
        s = (s + 1) & lm->host.mask;
      }
      lm->cells[s] = LmCell{key, logp[g], m < order ? backoff[g] : 0.f};
    }
  }
  for (int64_t i = 1; i <= n_words; ++i)
    if (!seen[i]) return fail(MI355ASR_EINVAL, "language model: word %lld has no unigram", (long long)i);
  lm->class_word.assign(class_word, class_word + n_classes);
  for (int c = 0; c < n_classes; ++c)
    if (lm->class_word[c] < 0 || lm->class_word[c] > n_words) return fail(MI355ASR_EINVAL, "class %d maps to word %d outside [0, %lld]", c, lm->class_word[c], (long long)n_words);
  // make_ngram (scorer.cpp:164-194) stops at a space and fills every slot from there backwards with the empty word, which is
  // OOV: a space anywhere among the last `order` tokens makes the n-gram OOV, which is what word 0 does
  if (space_class >= 0) lm->class_word[space_class] = 0;
  *out = lm.release();
  return 0;
}

int mi355asr_lm_destroy(mi355asr_lm* lm) {
  if (!lm) return 0;
  for (int d = 0; d < 64; ++d) {
    if (lm->d_cells[d]) (void)hipFree(lm->d_cells[d]);
    if (lm->d_class_word[d]) (void)hipFree(lm->d_class_word[d]);
  }
  delete lm;
  return 0;
}

int mi355asr_lm_score(const mi355asr_lm* lm, const int32_t* ngrams, int32_t n, float* out, int32_t on_device, void* stream) {
  if (!lm || n < 0 || (n > 0 && (!ngrams || !out))) return fail(MI355ASR_EINVAL, "bad argument");
  if (n == 0) return 0;
  const int order = lm->host.order;
  for (size_t i = 0; i < (size_t)n * order; ++i)
    if (ngrams[i] < 0 || ngrams[i] > lm->n_words) return fail(MI355ASR_EINVAL, "mi355asr_lm_score: word id %d outside [0, %lld]", ngrams[i], (long long)lm->n_words);
  if (!on_device) {
    for (int i = 0; i < n; ++i) {
      int32_t r[kLmMaxOrder] = {0, 0, 0, 0, 0, 0};
      for (int k = 0; k < order; ++k) r[k] = ngrams[(size_t)i * order + (order - 1 - k)];
      out[i] = lm_cond(lm->host, r);
    }
    return 0;
  }
  LmView v;
  if (mi355asr_lm_device_view(lm, &v, nullptr) != 0) return fail(MI355ASR_EHIP, "language model upload failed");
  hipStream_t s = (hipStream_t)stream;
  int32_t* d_in = nullptr;
  float* d_out = nullptr;
  HIP_TRY(hipMalloc((void**)&d_in, (size_t)n * order * sizeof(int32_t)));
  if (hipMalloc((void**)&d_out, (size_t)n * sizeof(float)) != hipSuccess) { (void)hipFree(d_in); return fail(MI355ASR_EHIP, "hipMalloc"); }
  hipError_t e = hipMemcpyAsync(d_in, ngrams, (size_t)n * order * sizeof(int32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(lm_score_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, d_in, n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "mi355asr_lm_score: %s", hipGetErrorString(e));
  return 0;
}

}  // extern "C"
