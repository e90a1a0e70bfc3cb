// TEST INFRASTRUCTURE ONLY (see README.md): lm::ngram::LoadVirtual as the textbook back-off model over an ARPA file.
// p(w | h) = logp of the longest n-gram (suffix of h, w) in the file, plus the back-off weights of the contexts that were
// backed off from, shortest first, an absent context adding nothing -- accumulated in float, which is how KenLM keeps and
// adds them.  "<unk>" is word 0 whether the file lists it or not; the other words are numbered in file order.
#ifndef GOLDEN_REF_LM_STUB_MODEL_HH_
#define GOLDEN_REF_LM_STUB_MODEL_HH_
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "lm/config.hh"
#include "lm/state.hh"
#include "lm/virtual_interface.hh"

namespace lm {
namespace ngram {

class ArpaBackoffModel : public base::Model, public base::Vocabulary {
public:
  ArpaBackoffModel(const char* path, const Config& config) : order_(0) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    index_["<unk>"] = 0;
    std::vector<std::string> names(1, "<unk>");
    std::string line;
    int cur = 0;
    bool data = false;
    while (std::getline(in, line)) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (line.empty()) continue;
      if (line == "\\data\\") { data = true; continue; }
      if (!data) continue;
      if (line == "\\end\\") break;
      if (line.compare(0, 6, "ngram ") == 0) {
        const int m = std::atoi(line.c_str() + 6);
        if (m > order_) order_ = m;
        continue;
      }
      if (line[0] == '\\') { cur = std::atoi(line.c_str() + 1); continue; }
      std::istringstream ss(line);
      std::vector<std::string> f;
      std::string tok;
      while (ss >> tok) f.push_back(tok);
      if ((int)f.size() < cur + 1) throw std::runtime_error("bad ARPA line: " + line);
      Entry e;
      e.logp = std::strtof(f[0].c_str(), nullptr);
      e.backoff = (int)f.size() > cur + 1 ? std::strtof(f[cur + 1].c_str(), nullptr) : 0.0f;
      std::vector<WordIndex> key;                 // most recent word first
      for (int i = cur; i >= 1; --i) {
        if (cur == 1 && index_.find(f[i]) == index_.end()) {
          index_[f[i]] = (WordIndex)names.size();
          names.push_back(f[i]);
        }
        std::map<std::string, WordIndex>::const_iterator it = index_.find(f[i]);
        if (it == index_.end()) throw std::runtime_error("ARPA n-gram with an unknown word: " + line);
        key.push_back(it->second);
      }
      table_[key] = e;
    }
    if (config.enumerate_vocab)
      for (size_t i = 0; i < names.size(); ++i) config.enumerate_vocab->Add((WordIndex)i, StringPiece(names[i]));
  }
  unsigned char Order() const { return (unsigned char)order_; }
  void NullContextWrite(void* to_state) const { static_cast<State*>(to_state)->length = 0; }
  const base::Vocabulary& BaseVocabulary() const { return *this; }
  WordIndex Index(const std::string& word) const {
    std::map<std::string, WordIndex>::const_iterator it = index_.find(word);
    return it == index_.end() ? 0 : it->second;
  }
  float BaseScore(const void* in_state, const WordIndex word, void* out_state) const {
    const State& in = *static_cast<const State*>(in_state);
    std::vector<WordIndex> key(1, word);
    float p = 0.0f;
    int found = 0;
    for (int n = 1; n <= (int)in.length + 1; ++n) {          // n-gram of n words: the new word and n - 1 of the context
      if (n > 1) key.push_back(in.words[n - 2]);
      std::map<std::vector<WordIndex>, Entry>::const_iterator it = table_.find(key);
      if (it != table_.end()) { p = it->second.logp; found = n; }
    }
    if (found == 0) {                                        // not even a unigram: "<unk>" without an entry
      p = -100.0f;
      found = 1;
    }
    for (int n = found; n <= (int)in.length; ++n) {          // contexts of n words, shortest first
      std::vector<WordIndex> ctx(in.words, in.words + n);
      std::map<std::vector<WordIndex>, Entry>::const_iterator it = table_.find(ctx);
      if (it != table_.end()) p += it->second.backoff;
    }
    State out;
    out.words[0] = word;
    int len = 1;
    for (int i = 0; i < (int)in.length && len < order_ - 1; ++i) out.words[len++] = in.words[i];
    out.length = (unsigned char)(order_ > 1 ? len : 0);
    *static_cast<State*>(out_state) = out;
    return p;
  }

private:
  struct Entry { float logp, backoff; };
  int order_;
  std::map<std::string, WordIndex> index_;
  std::map<std::vector<WordIndex>, Entry> table_;
};

inline base::Model* LoadVirtual(const char* file_name, const Config& config) { return new ArpaBackoffModel(file_name, config); }

}  // namespace ngram
}  // namespace lm
#endif
