// TEST INFRASTRUCTURE ONLY (see README.md): a StringPiece that carries its characters (the oracle's stand-in is empty).
#ifndef ORACLE_REF_STUB_STRING_PIECE_HH_
#define ORACLE_REF_STUB_STRING_PIECE_HH_
#include <cstddef>
#include <string>
class StringPiece {
public:
  StringPiece() : p_(""), n_(0) {}
  StringPiece(const std::string& s) : p_(s.data()), n_(s.size()) {}
  StringPiece(const char* p, std::size_t n) : p_(p), n_(n) {}
  const char* data() const { return p_; }
  std::size_t length() const { return n_; }
private:
  const char* p_;
  std::size_t n_;
};
#endif
