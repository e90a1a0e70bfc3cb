// CTC prefix beam search behind the C ABI: the one-shot mi355asr_ctc_prefix_beam* entry points (top-n selection on the device, the
// search on the device or on host threads) and the stateful mi355asr_beam_* decoder handle.  Kernels: beam_device.hip; host search: beam.hip.
#include "model.h"

namespace {
// the scorer of a call: lm null = the scorer-less search; otherwise its class map has to cover the V - 1 non-blank classes
int check_scorer(const mi355asr_lm* lm, int V, double alpha, double beta) {
  if (!lm) return 0;
  int n = 0;
  (void)mi355asr_lm_class_word(lm, &n);
  if (n != V - 1) return fail(MI355ASR_EINVAL, "the language model was created for %d classes, the search has %d + blank", n, V - 1);
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(MI355ASR_EINVAL, "alpha and beta must be finite");
  return 0;
}
int prefix_beam_impl(const float* x, int32_t is_logits, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                     int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                     int32_t max_len, const BeamLm* sc, int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp, void* ws,
                     size_t ws_bytes, void* stream);
// what the calling thread's last mi355asr_ctc_prefix_beam / _lm call ran (mi355asr_beam_last_path): written where the search is chosen
thread_local int32_t last_path = 0;
}  // namespace

extern "C" {

int mi355asr_ctc_prefix_beam_lm_host(const float* probs, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                                     int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                     int32_t max_len, const mi355asr_lm* lm, double alpha, double beta, int32_t* ids,
                                     int32_t* lens, float* scores, int32_t* n_hyp) {
  if (!probs || !ids || !lens || !scores || !n_hyp) return fail(MI355ASR_EINVAL, "null pointer");
  if (B <= 0 || T <= 0 || V < 2 || beam_size <= 0 || max_len <= 0 || cutoff_top_n <= 0)
    return fail(MI355ASR_EINVAL, "bad beam-search argument (B=%d T=%d V=%d beam=%d max_len=%d top_n=%d)", B, T, V,
                beam_size, max_len, cutoff_top_n);
  if (int rc = check_scorer(lm, V, alpha, beta)) return rc;
  const BeamLm sc{lm, alpha, beta};
  return mi355asr_beam_host_lm_impl(probs, in_len, B, T, V, beam_size, cutoff_prob, cutoff_top_n, num_threads, max_len, &sc, ids,
                                    lens, scores, n_hyp);
}

int mi355asr_ctc_prefix_beam_lm(const float* x, int32_t is_logits, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                                int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                int32_t max_len, const mi355asr_lm* lm, double alpha, double beta, int32_t* ids, int32_t* lens,
                                float* scores, int32_t* n_hyp, void* ws, size_t ws_bytes, void* stream) {
  if (V >= 2)
    if (int rc = check_scorer(lm, V, alpha, beta)) return rc;
  const BeamLm sc{lm, alpha, beta};
  return prefix_beam_impl(x, is_logits, in_len, B, T, V, beam_size, cutoff_prob, cutoff_top_n, num_threads, max_len, &sc, ids, lens,
                          scores, n_hyp, ws, ws_bytes, stream);
}

int mi355asr_ctc_prefix_beam_lm_workspace_bytes(int32_t B, int32_t T, int32_t cutoff_top_n, int32_t beam_size, int32_t max_len,
                                                size_t* bytes) {
  if (!bytes || B <= 0 || T <= 0 || cutoff_top_n <= 0 || beam_size <= 0 || max_len <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  const size_t need = (size_t)B * T * (std::min(cutoff_top_n, 128) * 12 + 4);     // classes, probabilities, LM words; the blank's probability
  *bytes = ((need + 255) & ~(size_t)255) + mi355asr_beam_device_ws_bytes(B, T, beam_size, max_len);
  return 0;
}

int32_t mi355asr_beam_last_path(void) { return last_path; }

int mi355asr_beam_device_limits(int32_t with_scorer, int32_t* max_classes, int32_t* max_beam, int32_t* max_top_n, int32_t* small_beam) {
  if (!max_classes || !max_beam || !max_top_n || !small_beam) return fail(MI355ASR_EINVAL, "null pointer");
  int v[4];
  mi355asr_beam_device_limit_values(with_scorer != 0, &v[0], &v[1], &v[2], &v[3]);
  *max_classes = v[0]; *max_beam = v[1]; *max_top_n = v[2]; *small_beam = v[3];
  return 0;
}

int mi355asr_ctc_prefix_beam_host(const float* probs, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                                  int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                  int32_t max_len, int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp) {
  if (!probs || !ids || !lens || !scores || !n_hyp) return fail(MI355ASR_EINVAL, "null pointer");
  if (B <= 0 || T <= 0 || V < 2 || beam_size <= 0 || max_len <= 0 || cutoff_top_n <= 0)
    return fail(MI355ASR_EINVAL, "bad beam-search argument (B=%d T=%d V=%d beam=%d max_len=%d top_n=%d)", B, T, V,
                beam_size, max_len, cutoff_top_n);
  return mi355asr_beam_host_impl(probs, in_len, B, T, V, beam_size, cutoff_prob, cutoff_top_n, num_threads, max_len, ids,
                                 lens, scores, n_hyp);
}

int mi355asr_ctc_prefix_beam(const float* x, int32_t is_logits, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                             int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                             int32_t max_len, int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp, void* ws,
                             size_t ws_bytes, void* stream) {
  return prefix_beam_impl(x, is_logits, in_len, B, T, V, beam_size, cutoff_prob, cutoff_top_n, num_threads, max_len, nullptr, ids,
                          lens, scores, n_hyp, ws, ws_bytes, stream);
}
}  // extern "C"

namespace {
int prefix_beam_impl(const float* x, int32_t is_logits, const int32_t* in_len, int32_t B, int32_t T, int32_t V,
                     int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                     int32_t max_len, const BeamLm* sc, int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp, void* ws,
                     size_t ws_bytes, void* stream) {
  const mi355asr_lm* lm = sc ? sc->lm : nullptr;
  if (!x || !ids || !lens || !scores || !n_hyp || !ws) return fail(MI355ASR_EINVAL, "null pointer");
  if (B <= 0 || T <= 0 || V < 2 || beam_size <= 0 || max_len <= 0 || cutoff_top_n <= 0)
    return fail(MI355ASR_EINVAL, "bad beam-search argument");
  if (!(cutoff_prob < 1.0))
    return fail(MI355ASR_EINVAL, "cutoff_prob >= 1 disables pruning in the reference (every class is visited): use "
                "mi355asr_ctc_prefix_beam_host for that mode");
  const int N = std::min(cutoff_top_n, V);
  if (N > 128) return fail(MI355ASR_EINVAL, "cutoff_top_n=%d: the selection kernel supports up to 128", cutoff_top_n);
  const size_t frames = (size_t)B * T;
  // with a scorer: the LM words of the lists and the blank's probability per frame behind the two lists
  const size_t need = frames * N * (sizeof(int32_t) + sizeof(float)) + (lm ? frames * N * sizeof(int32_t) + frames * sizeof(float) : 0);
  if (ws_bytes < need) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  int32_t* d_idx = (int32_t*)ws;
  float* d_p = (float*)((char*)ws + frames * N * sizeof(int32_t));
  int32_t* d_w = lm ? (int32_t*)(d_p + frames * N) : nullptr;
  float* d_blank = lm ? (float*)(d_w + frames * N) : nullptr;
  if (mi355asr_launch_topn(x, (int)frames, V, N, is_logits, d_idx, d_p, d_blank, s) != 0)
    return fail(MI355ASR_EHIP, "top-n kernel launch failed (V=%d, cutoff_top_n=%d)", V, N);
  // MI355ASR_BEAM_DEVICE=0: the prefix search on host threads (beam.hip) instead of the device kernel (beam_device.hip)
  static const bool dev_env = mi355_env("MI355ASR_BEAM_DEVICE", 1) != 0;
  const size_t need_dev = ((need + 255) & ~(size_t)255) + mi355asr_beam_device_ws_bytes(B, T, beam_size, max_len);
  const bool fits = lm ? mi355asr_beam_device_lm_applicable(V, N, beam_size, mi355asr_lm_host_view(lm)->order)
                       : mi355asr_beam_device_applicable(V, N, beam_size);
  if (dev_env && fits && ws_bytes >= need_dev) {
    last_path = lm ? 4 : mi355asr_beam_device_small(N, beam_size) ? 2 : 3;
    char* w = (char*)ws + ((need + 255) & ~(size_t)255);
    BeamDeviceArgs a{};
    a.top_idx = d_idx; a.top_p = d_p; a.B = B; a.T = T; a.V = V; a.N = N; a.beam = beam_size;
    a.cutoff_top_n = cutoff_top_n; a.max_len = max_len; a.cutoff_prob = cutoff_prob;
    int32_t* d_len = nullptr;
    long long* d_prof = nullptr;
    (void)mi355asr_beam_device_carve(w, B, T, beam_size, max_len, &a, &d_len, &d_prof);   // the same layout the size query adds up
    // MI355ASR_BEAM_PROF=1: clock counters of utterance 0's search, printed per call (where a frame's time goes)
    static const bool prof_env = mi355_env("MI355ASR_BEAM_PROF", 0) != 0;
    if (prof_env) {
      a.prof = d_prof;
      HIP_TRY(hipMemsetAsync(a.prof, 0, 16 * sizeof(long long), s));
    }
    // The four results sit next to each other in the workspace (mi355asr_beam_device_carve): ONE copy into a pinned staging buffer of
    // the calling thread, then host copies -- the caller's arrays are pageable (NumPy), and four hipMemcpyAsync into pageable memory are
    // four staged, synchronous copies: ~120 us behind a 2.4 ms search (round 6, kernel trace of config 5); the lengths go up through
    // the same buffer (behind the results' span), so the search is launched without a host-side wait.  The buffer is kept for the
    // thread's lifetime (never freed: at process exit the runtime may be gone before a destructor would run).
    const size_t n_ids = (size_t)B * beam_size * max_len * sizeof(int32_t), n_lens = (size_t)B * beam_size * sizeof(int32_t),
                 n_scores = (size_t)B * beam_size * sizeof(float), n_nh = (size_t)B * sizeof(int32_t);
    const size_t span = (size_t)((const char*)a.n_hyp - (const char*)a.ids) + n_nh, want = span + n_nh + 64;
    static thread_local char* stage = nullptr;
    static thread_local size_t stage_cap = 0;
    if (want > stage_cap) {
      if (stage) (void)hipHostFree(stage);
      stage = nullptr; stage_cap = 0;
      void* q = nullptr;
      if (hipHostMalloc(&q, want + want / 4, hipHostMallocDefault) == hipSuccess) { stage = (char*)q; stage_cap = want + want / 4; }
      else (void)hipGetLastError();
    }
    if (in_len) {
      const void* src = in_len;
      if (stage) { std::memcpy(stage + span, in_len, n_nh); src = stage + span; }
      HIP_TRY(hipMemcpyAsync(d_len, src, n_nh, hipMemcpyHostToDevice, s));
      a.in_len = d_len;
    }
    if (lm) {
      BeamLmDeviceArgs l{};
      const int32_t* d_map = nullptr;
      if (mi355asr_lm_device_view(lm, &l.view, &d_map) != 0) return fail(MI355ASR_EHIP, "language model upload failed");
      if (mi355asr_launch_lm_map(d_idx, frames * N, d_map, V - 1, d_w, s) != 0) return fail(MI355ASR_EHIP, "LM word kernel launch failed");
      l.top_w = d_w; l.blank_p = d_blank; l.alpha = sc->alpha; l.beta = sc->beta;
      if (mi355asr_launch_beam_device_lm(&a, &l, s) != 0) return fail(MI355ASR_EHIP, "device beam search (scorer) launch failed");
    } else if (mi355asr_launch_beam_device(&a, s) != 0) return fail(MI355ASR_EHIP, "device beam search launch failed");
    long long prof[16] = {0};
    if (stage) {
      HIP_TRY(hipMemcpyAsync(stage, a.ids, span, hipMemcpyDeviceToHost, s));
    } else {
      HIP_TRY(hipMemcpyAsync(ids, a.ids, n_ids, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(lens, a.lens, n_lens, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(scores, a.scores, n_scores, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(n_hyp, a.n_hyp, n_nh, hipMemcpyDeviceToHost, s));
    }
    if (a.prof) HIP_TRY(hipMemcpyAsync(prof, a.prof, sizeof(prof), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (stage) {
      std::memcpy(ids, stage, n_ids);
      std::memcpy(lens, stage + ((const char*)a.lens - (const char*)a.ids), n_lens);
      std::memcpy(scores, stage + ((const char*)a.scores - (const char*)a.ids), n_scores);
      std::memcpy(n_hyp, stage + ((const char*)a.n_hyp - (const char*)a.ids), n_nh);
    }
    if (a.prof) {
      const double f = (double)std::max(1ll, prof[8]);
      fprintf(stderr, "[mi355asr] beam %d, utterance 0: %lld frames (%lld redone by the radix path); clocks per frame: entries %.0f, "
              "keys+ranks %.0f, keep %.0f, radix path %.0f (keys %.0f, select %.0f, compaction %.0f); inside the entry phase: thread 0 "
              "%.0f (%.0f up to the parent search), wave 3's candidate list %.0f (%.0f cumulative cut-off)\n", beam_size, prof[8],
              prof[4], prof[0] / f, prof[1] / f, prof[2] / f, prof[3] / f, prof[5] / f, prof[6] / f, prof[7] / f, prof[9] / f, prof[10] / f,
              prof[11] / f, prof[12] / f);
    }
    return 0;
  }
  last_path = 1;
  std::vector<int32_t> h_idx(frames * N);
  std::vector<float> h_p(frames * N);
  HIP_TRY(hipMemcpyAsync(h_idx.data(), d_idx, h_idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_p.data(), d_p, h_p.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  std::vector<float> h_blank(lm ? frames : 0);
  if (lm) HIP_TRY(hipMemcpyAsync(h_blank.data(), d_blank, frames * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return mi355asr_beam_topn_lm_impl(h_idx.data(), h_p.data(), lm ? h_blank.data() : nullptr, in_len, B, T, V, N, beam_size, cutoff_prob,
                                    cutoff_top_n, num_threads, max_len, sc, ids, lens, scores, n_hyp);
}
}  // namespace

extern "C" {

int mi355asr_beam_math_eval(int32_t kind, const float* in_dev, void* out_dev, int32_t n, void* stream) {
  if (!in_dev || !out_dev || n < 0 || kind < 0 || kind > 3) return fail(MI355ASR_EINVAL, "bad argument");
  if (mi355asr_launch_refmath_eval(kind, in_dev, out_dev, n, (hipStream_t)stream) != 0)
    return fail(MI355ASR_EHIP, "refmath kernel launch failed");
  return 0;
}

int mi355asr_ctc_prefix_beam_workspace_bytes(int32_t B, int32_t T, int32_t cutoff_top_n, int32_t beam_size, int32_t max_len,
                                             size_t* bytes) {
  if (!bytes || B <= 0 || T <= 0 || cutoff_top_n <= 0 || beam_size <= 0 || max_len <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  const size_t need = (size_t)B * T * std::min(cutoff_top_n, 128) * 8;
  *bytes = ((need + 255) & ~(size_t)255) + mi355asr_beam_device_ws_bytes(B, T, beam_size, max_len);
  return 0;
}
// ---- stateful BeamDecoder ----------------------------------------------------------------------------------
struct mi355asr_beam { void* st; int V, beam; };
int mi355asr_beam_create(int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, mi355asr_beam** out) {
  if (!out) return fail(MI355ASR_EINVAL, "null argument");
  if (V < 2 || beam_size < 1 || cutoff_top_n < 1 || !(cutoff_prob > 0.0) || cutoff_prob > 1.0)
    return fail(MI355ASR_EINVAL, "beam decoder: need V >= 2, beam_size >= 1, cutoff_top_n >= 1, 0 < cutoff_prob <= 1");
  auto* d = new mi355asr_beam{mi355asr_beam_state_new(V, beam_size, cutoff_prob, cutoff_top_n), V, beam_size};
  *out = d;
  return 0;
}
int mi355asr_beam_create_lm(int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, const mi355asr_lm* lm,
                            double alpha, double beta, mi355asr_beam** out) {
  if (!out) return fail(MI355ASR_EINVAL, "null argument");
  if (V < 2 || beam_size < 1 || cutoff_top_n < 1 || !(cutoff_prob > 0.0) || cutoff_prob > 1.0)
    return fail(MI355ASR_EINVAL, "beam decoder: need V >= 2, beam_size >= 1, cutoff_top_n >= 1, 0 < cutoff_prob <= 1");
  if (int rc = check_scorer(lm, V, alpha, beta)) return rc;
  const BeamLm sc{lm, alpha, beta};
  auto* d = new mi355asr_beam{mi355asr_beam_state_new_lm(V, beam_size, cutoff_prob, cutoff_top_n, &sc), V, beam_size};
  *out = d;
  return 0;
}
int mi355asr_beam_decode(mi355asr_beam* d, const float* probs, int32_t T, int32_t max_len, int32_t* ids, int32_t* lens,
                         float* scores, int32_t* n_hyp) {
  if (!d || !ids || !lens || !scores || !n_hyp || (T > 0 && !probs)) return fail(MI355ASR_EINVAL, "null argument");
  if (T < 0 || max_len < 1) return fail(MI355ASR_EINVAL, "T must be >= 0 and max_len >= 1 (got %d, %d)", T, max_len);
  *n_hyp = mi355asr_beam_state_decode(d->st, probs, T, max_len, ids, lens, scores);
  return 0;
}
int mi355asr_beam_reset(mi355asr_beam* d) {
  if (!d) return fail(MI355ASR_EINVAL, "null argument");
  mi355asr_beam_state_reset(d->st);
  return 0;
}
int mi355asr_beam_destroy(mi355asr_beam* d) {
  if (!d) return 0;
  mi355asr_beam_state_free(d->st);
  delete d;
  return 0;
}
int mi355asr_beam_clone(const mi355asr_beam* d, mi355asr_beam** out) {
  if (!d || !out) return fail(MI355ASR_EINVAL, "null argument");
  *out = new mi355asr_beam{mi355asr_beam_state_clone(d->st), d->V, d->beam};
  return 0;
}

// ---- the device search for many live streams (beam_device.hip STREAM kernels) ----------
namespace {
// what every streams entry point checks first: the search is inside the device limits (no host fallback here)
int check_streams_config(int32_t n_streams, int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t max_frames,
                         const mi355asr_lm* lm) {
  if (n_streams < 1 || V < 2 || beam_size < 1 || cutoff_top_n < 1 || max_frames < 1)
    return fail(MI355ASR_EINVAL, "beam streams: need n_streams >= 1, V >= 2, beam_size >= 1, cutoff_top_n >= 1, max_frames >= 1 (got %d, %d, %d, %d, %d)",
                n_streams, V, beam_size, cutoff_top_n, max_frames);
  if (!(cutoff_prob > 0.0) || !(cutoff_prob < 1.0))
    return fail(MI355ASR_EINVAL, "beam streams: cutoff_prob %g: the device search needs 0 < cutoff_prob < 1 (at 1 the reference visits "
                "every class); use one host mi355asr_beam per stream for that mode", cutoff_prob);
  int lim[4];
  mi355asr_beam_device_limit_values(lm != nullptr, &lim[0], &lim[1], &lim[2], &lim[3]);
  if (V > lim[0]) return fail(MI355ASR_EINVAL, "beam streams: V=%d is above the device search's max_classes=%d", V, lim[0]);
  if (beam_size > lim[1]) return fail(MI355ASR_EINVAL, "beam streams: beam_size=%d is above the device search's max_beam=%d", beam_size, lim[1]);
  if (std::min(cutoff_top_n, V) > lim[2])
    return fail(MI355ASR_EINVAL, "beam streams: cutoff_top_n=%d is above the device search's max_top_n=%d", cutoff_top_n, lim[2]);
  if (lm && !mi355asr_beam_device_lm_applicable(V, std::min(cutoff_top_n, V), beam_size, mi355asr_lm_host_view(lm)->order))
    return fail(MI355ASR_EINVAL, "beam streams: language model order %d is outside the device search", mi355asr_lm_host_view(lm)->order);
  if ((size_t)max_frames * beam_size + 1 > (size_t)0x7fffffff)
    return fail(MI355ASR_EINVAL, "beam streams: max_frames * beam_size = %zu cells do not fit the arena's 31-bit links", (size_t)max_frames * beam_size);
  return 0;
}
// workspace of a step over n streams of T frames: top-n lists (+ LM words, blank probabilities), the slot table
size_t streams_ws(size_t n, size_t T, int N, bool lm, size_t* off_slots) {
  const size_t frames = n * T;
  size_t need = frames * N * (sizeof(int32_t) + sizeof(float)) + (lm ? frames * N * sizeof(int32_t) + frames * sizeof(float) : 0);
  need = (need + 255) & ~(size_t)255;
  if (off_slots) *off_slots = need;
  return need + ((n * sizeof(int32_t) + 255) & ~(size_t)255);
}
}  // namespace

int mi355asr_beam_streams_bytes(int32_t n_streams, int32_t V, int32_t beam_size, int32_t cutoff_top_n, int32_t max_frames,
                                const mi355asr_lm* lm, int32_t T_max, size_t* state_bytes, size_t* ws_bytes) {
  if (!state_bytes || !ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (T_max < 1) return fail(MI355ASR_EINVAL, "beam streams: T_max must be >= 1 (got %d)", T_max);
  if (int rc = check_streams_config(n_streams, V, beam_size, 0.5, cutoff_top_n, max_frames, lm)) return rc;
  *state_bytes = (size_t)n_streams * mi355asr_beam_stream_slot_bytes(beam_size, max_frames, lm != nullptr);
  *ws_bytes = streams_ws((size_t)n_streams, (size_t)T_max, std::min(cutoff_top_n, V), lm != nullptr, nullptr);
  return 0;
}

int mi355asr_beam_streams_reset(void* state_dev, int32_t n_streams, int32_t V, int32_t beam_size, int32_t cutoff_top_n, int32_t max_frames,
                                const mi355asr_lm* lm, const int32_t* slots_host, int32_t n, void* stream) {
  if (!state_dev || ((uintptr_t)state_dev & 15)) return fail(MI355ASR_EINVAL, "beam streams: state_dev must be a 16-byte aligned device pointer");
  if (int rc = check_streams_config(n_streams, V, beam_size, 0.5, cutoff_top_n, max_frames, lm)) return rc;
  if (slots_host) {
    if (n < 1) return fail(MI355ASR_EINVAL, "beam streams: reset of %d slots", n);
    for (int i = 0; i < n; ++i)
      if (slots_host[i] < 0 || slots_host[i] >= n_streams) return fail(MI355ASR_EINVAL, "beam streams: slot %d out of range 0 .. %d", slots_host[i], n_streams - 1);
  }
  if (mi355asr_launch_beam_stream_reset(state_dev, n_streams, beam_size, max_frames, lm != nullptr, lm ? mi355asr_lm_host_view(lm)->bos : 0,
                                        slots_host, n, (hipStream_t)stream) != 0)
    return fail(MI355ASR_EHIP, "beam streams: reset kernel launch failed");
  return 0;
}

int mi355asr_beam_streams_step(void* state_dev, int32_t n_streams, int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n,
                               int32_t max_frames, const mi355asr_lm* lm, double alpha, double beta, const int32_t* slots_host, int32_t n,
                               const float* x_dev, int32_t is_logits, const int32_t* n_commit_dev, const int32_t* n_peek_dev, int32_t T,
                               int32_t n_best, int32_t max_len, const mi355asr_beam_streams_outputs* outs, void* ws_dev, size_t ws_bytes,
                               void* stream) {
  if (!state_dev || !slots_host || !x_dev || !n_commit_dev || !outs || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (!outs->ids || !outs->lens || !outs->scores || !outs->n_hyp || !outs->frames || !outs->status) return fail(MI355ASR_EINVAL, "null output pointer");
  if ((uintptr_t)state_dev & 15) return fail(MI355ASR_EINVAL, "beam streams: state_dev must be 16-byte aligned");
  if (int rc = check_streams_config(n_streams, V, beam_size, cutoff_prob, cutoff_top_n, max_frames, lm)) return rc;
  if (int rc = check_scorer(lm, V, alpha, beta)) return rc;
  if (n < 1 || n > n_streams || T < 1 || max_len < 1) return fail(MI355ASR_EINVAL, "beam streams: need 1 <= n <= n_streams, T >= 1, max_len >= 1 (got %d, %d, %d)", n, T, max_len);
  if (n_best < 1 || n_best > beam_size) return fail(MI355ASR_EINVAL, "beam streams: n_best=%d must be 1 .. beam_size=%d", n_best, beam_size);
  {
    std::vector<char> seen((size_t)n_streams, 0);
    for (int i = 0; i < n; ++i) {
      const int sl = slots_host[i];
      if (sl < 0 || sl >= n_streams) return fail(MI355ASR_EINVAL, "beam streams: slot %d out of range 0 .. %d", sl, n_streams - 1);
      if (seen[sl]) return fail(MI355ASR_EINVAL, "beam streams: slot %d is named twice in one step", sl);
      seen[sl] = 1;
    }
  }
  const int N = std::min(cutoff_top_n, V);
  size_t off_slots = 0;
  const size_t need = streams_ws((size_t)n, (size_t)T, N, lm != nullptr, &off_slots);
  if (ws_bytes < need) return fail(MI355ASR_EWORKSPACE, "beam streams: workspace too small: %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const size_t frames = (size_t)n * T;
  int32_t* d_idx = (int32_t*)ws_dev;
  float* d_p = (float*)((char*)ws_dev + frames * N * sizeof(int32_t));
  int32_t* d_w = lm ? (int32_t*)(d_p + frames * N) : nullptr;
  float* d_blank = lm ? (float*)(d_w + frames * N) : nullptr;
  int32_t* d_slots = (int32_t*)((char*)ws_dev + off_slots);
  // the slot table comes from pageable host memory: the runtime stages it before the call returns, nothing is waited for
  HIP_TRY(hipMemcpyAsync(d_slots, slots_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  // The selection runs over all n * T rows of the padded input; rows past commit + peek are padding whose lists the search never
  // reads (its frame loop and its prefetch end at commit + peek).  topn_kernel / topn_reg_kernel are bounded by V and N whatever a
  // row holds: every loop runs to V, N, 64 or G + min(E, N) <= GT_CAP + EQ_CAP, and every store is behind pg < GT_CAP, pe < EQ_CAP
  // or before < N; lm_map_kernel maps a class outside [0, V - 1) to word 0.
  if (mi355asr_launch_topn(x_dev, (int)frames, V, N, is_logits, d_idx, d_p, d_blank, s) != 0)
    return fail(MI355ASR_EHIP, "top-n kernel launch failed (V=%d, cutoff_top_n=%d)", V, N);
  BeamDeviceArgs a{};
  a.top_idx = d_idx; a.top_p = d_p; a.B = n; a.T = T; a.V = V; a.N = N; a.beam = beam_size;
  a.cutoff_top_n = cutoff_top_n; a.max_len = max_len; a.cutoff_prob = cutoff_prob;
  a.ids = outs->ids; a.lens = outs->lens; a.scores = outs->scores; a.n_hyp = outs->n_hyp;
  BeamStreamArgs sa{};
  sa.state = (char*)state_dev; sa.slot_bytes = mi355asr_beam_stream_slot_bytes(beam_size, max_frames, lm != nullptr);
  sa.slots = d_slots; sa.n_commit = n_commit_dev; sa.n_peek = n_peek_dev; sa.max_frames = max_frames; sa.n_best = n_best;
  sa.frames = outs->frames; sa.status = outs->status;
  int path;
  if (lm) {
    BeamLmDeviceArgs l{};
    const int32_t* d_map = nullptr;
    if (mi355asr_lm_device_view(lm, &l.view, &d_map) != 0) return fail(MI355ASR_EHIP, "language model upload failed");
    if (mi355asr_launch_lm_map(d_idx, frames * N, d_map, V - 1, d_w, s) != 0) return fail(MI355ASR_EHIP, "LM word kernel launch failed");
    l.top_w = d_w; l.blank_p = d_blank; l.alpha = alpha; l.beta = beta;
    path = mi355asr_launch_beam_stream(&a, &l, &sa, s);
  } else {
    path = mi355asr_launch_beam_stream(&a, nullptr, &sa, s);
  }
  if (path < 0) return fail(MI355ASR_EHIP, "beam streams: search kernel launch failed");
  last_path = path;
  return 0;
}
}  // extern "C"
