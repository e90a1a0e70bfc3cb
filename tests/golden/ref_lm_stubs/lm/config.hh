// TEST INFRASTRUCTURE ONLY (see README.md): the one field of lm::ngram::Config that scorer.cpp sets.
#ifndef GOLDEN_REF_LM_STUB_CONFIG_HH_
#define GOLDEN_REF_LM_STUB_CONFIG_HH_
#include "lm/enumerate_vocab.hh"
namespace lm {
namespace ngram {
struct Config {
  EnumerateVocab* enumerate_vocab;
  Config() : enumerate_vocab(nullptr) {}
};
}  // namespace ngram
}  // namespace lm
#endif
