// internal interface between beam.hip and api.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lm_table.h"

struct mi355asr_lm;
// the scorer of a search (replaces: Scorer* ext_scorer with its alpha / beta); lm null = the scorer-less search
struct BeamLm {
  const mi355asr_lm* lm;
  double alpha, beta;
};

extern "C" {
int mi355asr_beam_host_impl(const float* probs, const int32_t* in_len, int B, int T, int V, int beam_size,
                            double cutoff_prob, int cutoff_top_n, int num_threads, int max_len, int32_t* ids,
                            int32_t* lens, float* scores, int32_t* n_hyp);
int mi355asr_beam_topn_impl(const int32_t* top_idx, const float* top_p, const int32_t* in_len, int B, int T, int V,
                            int N, int beam_size, double cutoff_prob, int cutoff_top_n, int num_threads, int max_len,
                            int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp);
void* mi355asr_beam_state_new(int V, int beam_size, double cutoff_prob, int cutoff_top_n);
void mi355asr_beam_state_free(void* h);
void mi355asr_beam_state_reset(void* h);
int mi355asr_beam_state_decode(void* h, const float* probs, int T, int max_len, int32_t* ids, int32_t* lens, float* scores);
// device prefix search (beam_device.hip): every pointer is a DEVICE pointer
struct BeamDeviceArgs {
  const int32_t* top_idx;   // [B, T, N] classes in descending probability (topn_kernel)
  const float* top_p;       // [B, T, N]
  const int32_t* in_len;    // [B] or null
  int B, T, V, N, beam, cutoff_top_n, max_len;
  double cutoff_prob;
  int32_t* ids;             // [B, beam, max_len] padded with -1
  int32_t* lens;            // [B, beam]
  float* scores;            // [B, beam]
  int32_t* n_hyp;           // [B]
  int2* arena;              // [B, T * beam + 1] back-pointers (parent link, character)
  long long* prof;          // null, or 9 counters of utterance 0 (MI355ASR_BEAM_PROF)
};
bool mi355asr_beam_device_applicable(int V, int N, int beam);
bool mi355asr_beam_device_small(int N, int beam);    // which scorer-less kernel a call gets: one key per thread (true) or the radix path
void mi355asr_beam_device_limit_values(int with_scorer, int* max_classes, int* max_beam, int* max_top_n, int* small_beam);
size_t mi355asr_beam_device_ws_bytes(int B, int T, int beam, int max_len);
// the ONE place that lays the device search's buffers out in its workspace (16-byte aligned segments; ws null: size only):
// fills a->arena / ids / lens / scores / n_hyp, *d_len (staging of in_len) and *prof (9 x int64 counters); returns the bytes used
size_t mi355asr_beam_device_carve(char* ws, int B, int T, int beam, int max_len, BeamDeviceArgs* a, int32_t** d_len, long long** prof);
int mi355asr_launch_beam_device(const BeamDeviceArgs* a, hipStream_t s);
// kind 0 expf(in[i]) -> float, 1 logf -> float, 2 log((double)in[i] + FLT_MIN) -> double, 3 log_sum_exp(in[i], in[n + i]) -> float,
// evaluated by the device search's own routines (refmath.h)
int mi355asr_launch_refmath_eval(int kind, const float* in, void* out, int n, hipStream_t s);
// blank_p_dev (may be null): the probability of class V - 1 per frame, what the scorer's min_cutoff needs
int mi355asr_launch_topn(const float* x_dev, int frames, int V, int N, int is_logits, int32_t* idx_dev, float* p_dev,
                         float* blank_p_dev, hipStream_t s);

// ---- the searches with an n-gram scorer (lm.hip: the table; beam.hip / beam_device.hip: the searches) ----
const LmView* mi355asr_lm_host_view(const mi355asr_lm* lm);
const int32_t* mi355asr_lm_class_word(const mi355asr_lm* lm, int* n_classes);       // class -> LM word (0: OOV), host
// the table and the class map on the current device (uploaded on first use, kept until mi355asr_lm_destroy); 0 on success
int mi355asr_lm_device_view(const mi355asr_lm* lm, LmView* view, const int32_t** class_word_dev);
int mi355asr_beam_host_lm_impl(const float* probs, const int32_t* in_len, int B, int T, int V, int beam_size,
                               double cutoff_prob, int cutoff_top_n, int num_threads, int max_len, const BeamLm* sc,
                               int32_t* ids, int32_t* lens, float* scores, int32_t* n_hyp);
int mi355asr_beam_topn_lm_impl(const int32_t* top_idx, const float* top_p, const float* blank_p, const int32_t* in_len,
                               int B, int T, int V, int N, int beam_size, double cutoff_prob, int cutoff_top_n,
                               int num_threads, int max_len, const BeamLm* sc, int32_t* ids, int32_t* lens, float* scores,
                               int32_t* n_hyp);
void* mi355asr_beam_state_new_lm(int V, int beam_size, double cutoff_prob, int cutoff_top_n, const BeamLm* sc);
// what the device search with a scorer reads besides BeamDeviceArgs (device pointers)
struct BeamLmDeviceArgs {
  LmView view;
  const int32_t* top_w;     // [B, T, N] LM word of top_idx (mi355asr_launch_lm_map)
  const float* blank_p;     // [B, T] probability of the blank
  double alpha, beta;
};
bool mi355asr_beam_device_lm_applicable(int V, int N, int beam, int order);
int mi355asr_launch_lm_map(const int32_t* top_idx, size_t n, const int32_t* class_word_dev, int n_classes, int32_t* top_w,
                           hipStream_t s);
int mi355asr_launch_beam_device_lm(const BeamDeviceArgs* a, const BeamLmDeviceArgs* l, hipStream_t s);
void* mi355asr_beam_state_clone(const void* h);      // a copy of a stateful host decoder, trie and scorer included

// ---- the device search for many live streams (beam_device.hip STREAM) ----
// what a stream call reads besides BeamDeviceArgs (B = streams of the call, T = frames per stream in x; in_len and arena unused;
// ids / lens / scores are [B, n_best, ...]); device pointers
struct BeamStreamArgs {
  char* state;              // [n_streams] slots of slot_bytes
  size_t slot_bytes;
  const int32_t* slots;     // [B] slot of each stream of the call
  const int32_t* n_commit;  // [B] final frames
  const int32_t* n_peek;    // [B] provisional frames behind them, or null
  int max_frames, n_best;
  int32_t* frames;          // [B] frames committed after the call
  int32_t* status;          // [B] 0 ok, 1 over capacity (nothing consumed)
};
size_t mi355asr_beam_stream_slot_bytes(int beam, int max_frames, int with_lm);
int mi355asr_launch_beam_stream_reset(void* state, int n_streams, int beam, int max_frames, int with_lm, int bos, const int32_t* slots_host,
                                      int n, hipStream_t s);
int mi355asr_launch_beam_stream(const BeamDeviceArgs* a, const BeamLmDeviceArgs* l, const BeamStreamArgs* sa, hipStream_t s);
}

// One slot: header int4 (entries, committed frames, 0, 0) | the Beam fields of `beam` entries, in rank order | with a scorer
// lmhist [kLmMaxOrder - 1][beam] and lmterm [beam] | back-pointer arena int2 [max_frames * beam + 1], cell 1 + frame * beam + rank.
// bytes = 16 + beam * (36 + 24 with a scorer), rounded up to 16, + 8 * (max_frames * beam + 1), rounded up to 16.
struct BeamStreamLayout { unsigned id, par, ch, arena_i, score, b, nb, lmhist, lmterm, arena; size_t bytes; };   // beam <= 128: the offsets in front of the arena are small
__host__ __device__ inline BeamStreamLayout beam_stream_layout(int beam, int max_frames, bool with_lm) {
  BeamStreamLayout l;
  const unsigned n = (unsigned)beam;
  l.id = 16; l.par = l.id + 8 * n; l.ch = l.par + 8 * n; l.arena_i = l.ch + 4 * n; l.score = l.arena_i + 4 * n;
  l.b = l.score + 4 * n; l.nb = l.b + 4 * n; l.lmhist = l.nb + 4 * n;
  l.lmterm = l.lmhist + (with_lm ? 4 * (unsigned)(kLmMaxOrder - 1) * n : 0);
  l.arena = (l.lmterm + (with_lm ? 4 * n : 0) + 15) & ~15u;
  l.bytes = ((size_t)l.arena + 8 * ((size_t)max_frames * n + 1) + 15) & ~(size_t)15;
  return l;
}
