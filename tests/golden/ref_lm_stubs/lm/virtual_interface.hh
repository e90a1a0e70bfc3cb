// TEST INFRASTRUCTURE ONLY (see README.md): lm::base::Model and lm::base::Vocabulary as scorer.cpp uses them.
#ifndef GOLDEN_REF_LM_STUB_VIRTUAL_INTERFACE_HH_
#define GOLDEN_REF_LM_STUB_VIRTUAL_INTERFACE_HH_
#include <string>
#include "lm/word_index.hh"
namespace lm {
namespace base {
class Vocabulary {
public:
  virtual ~Vocabulary() {}
  virtual WordIndex Index(const std::string& word) const = 0;     // 0 = <unk>
};
class Model {
public:
  virtual ~Model() {}
  virtual unsigned char Order() const = 0;
  virtual void NullContextWrite(void* to_state) const = 0;
  virtual float BaseScore(const void* in_state, const WordIndex new_word, void* out_state) const = 0;
  virtual const Vocabulary& BaseVocabulary() const = 0;
};
}  // namespace base
}  // namespace lm
#endif
