// TEST INFRASTRUCTURE ONLY (see README.md): lm::ngram::State = the last order - 1 words, most recent first.
#ifndef GOLDEN_REF_LM_STUB_STATE_HH_
#define GOLDEN_REF_LM_STUB_STATE_HH_
#include "lm/word_index.hh"
namespace lm {
namespace ngram {
struct State {
  WordIndex words[8];
  unsigned char length;
  State() : length(0) {}
};
}  // namespace ngram
}  // namespace lm
#endif
