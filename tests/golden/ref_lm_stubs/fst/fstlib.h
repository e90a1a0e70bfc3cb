// TEST INFRASTRUCTURE ONLY (see README.md): the oracle's OpenFST stand-in plus the three calls of Scorer::fill_dictionary,
// which only the word-based mode reaches.
#ifndef GOLDEN_REF_LM_STUB_FSTLIB_H_
#define GOLDEN_REF_LM_STUB_FSTLIB_H_
#include_next "fst/fstlib.h"
namespace fst {
inline void RmEpsilon(StdVectorFst*) { stub_unreachable(); }
inline void Determinize(const StdVectorFst&, StdVectorFst*) { stub_unreachable(); }
inline void Minimize(StdVectorFst*) { stub_unreachable(); }
}  // namespace fst
#endif
