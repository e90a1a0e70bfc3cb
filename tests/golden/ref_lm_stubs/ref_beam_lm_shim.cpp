// TEST INFRASTRUCTURE ONLY (see README.md): C ABI around the reference's Scorer, ctc_beam_search_decoder and BeamDecoder
// with ext_scorer set.  Vocabularies and words travel as '\n'-joined UTF-8; hypotheses come back the same way.
#include <cstring>
#include <string>
#include <vector>

#include "ctc_beam_search_decoder.h"
#include "scorer.h"

static std::vector<std::string> split_lines(const char* s) {
  std::vector<std::string> out;
  std::string cur;
  for (const char* p = s; *p; ++p) {
    if (*p == '\n') { out.push_back(cur); cur.clear(); }
    else cur.push_back(*p);
  }
  out.push_back(cur);
  return out;
}
static int emit(const std::vector<std::pair<double, std::string>>& res, double* scores, char* text, int text_cap) {
  std::string all;
  int n = 0;
  for (size_t i = 0; i < res.size(); ++i) {
    scores[n++] = res[i].first;
    if (i) all.push_back('\n');
    all += res[i].second;
  }
  if ((int)all.size() + 1 > text_cap) return -1;
  std::memcpy(text, all.c_str(), all.size() + 1);
  return n;
}
static std::vector<std::vector<double>> rows(const double* probs, int T, int V) {
  std::vector<std::vector<double>> seq(T, std::vector<double>(V));
  for (int t = 0; t < T; ++t)
    for (int v = 0; v < V; ++v) seq[t][v] = probs[(size_t)t * V + v];
  return seq;
}

extern "C" void* ref_scorer_new(double alpha, double beta, const char* lm_path, const char* vocab) {
  return new Scorer(alpha, beta, lm_path, split_lines(vocab));
}
extern "C" void ref_scorer_free(void* s) { delete static_cast<Scorer*>(s); }
extern "C" int ref_scorer_is_character_based(void* s) { return static_cast<Scorer*>(s)->is_character_based() ? 1 : 0; }
extern "C" int ref_scorer_max_order(void* s) { return (int)static_cast<Scorer*>(s)->get_max_order(); }
extern "C" double ref_scorer_cond(void* s, const char* words) { return static_cast<Scorer*>(s)->get_log_cond_prob(split_lines(words)); }
extern "C" double ref_scorer_sent(void* s, const char* words) {
  return static_cast<Scorer*>(s)->get_sent_log_prob(*words ? split_lines(words) : std::vector<std::string>());
}
// vocab: the classes without the blank; probs [T][n_vocab + 1]
extern "C" int ref_lm_beam_search(const double* probs, int T, int V, const char* vocab, int beam_size, double cutoff_prob,
                                  int cutoff_top_n, void* scorer, double* scores, char* text, int text_cap) {
  auto res = ctc_beam_search_decoder(rows(probs, T, V), split_lines(vocab), (size_t)beam_size, cutoff_prob, (size_t)cutoff_top_n,
                                     static_cast<Scorer*>(scorer));
  return emit(res, scores, text, text_cap);
}
// vocab: the classes WITH the blank as the last entry (BeamDecoder's convention)
extern "C" void* ref_lm_decoder_new(const char* vocab, int beam_size, double cutoff_prob, int cutoff_top_n, void* scorer) {
  return new BeamDecoder(split_lines(vocab), (size_t)beam_size, cutoff_prob, (size_t)cutoff_top_n, static_cast<Scorer*>(scorer));
}
extern "C" void ref_lm_decoder_free(void* h) { delete static_cast<BeamDecoder*>(h); }
extern "C" int ref_lm_decoder_decode(void* h, const double* probs, int T, int V, double* scores, char* text, int text_cap) {
  return emit(static_cast<BeamDecoder*>(h)->decode(rows(probs, T, V)), scores, text, text_cap);
}
