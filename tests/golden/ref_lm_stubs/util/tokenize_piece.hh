// TEST INFRASTRUCTURE ONLY (see README.md): scorer.cpp includes this header and uses nothing from it.
#ifndef GOLDEN_REF_LM_STUB_TOKENIZE_PIECE_HH_
#define GOLDEN_REF_LM_STUB_TOKENIZE_PIECE_HH_
#endif
