// Back-off n-gram language model behind the prefix beam search's scorer (replaces: the KenLM calls of
// externals/ctc_decoders scorer.cpp:74-93, character-based mode): ONE packed table, read by the host search (beam.hip)
// and by the device search (beam_device.hip) through the same functions below, so both evaluate the same float
// arithmetic in the same order.
//
// Words are LM-word ids: 0 = out of vocabulary (a class without an LM word, "<unk>", the space class), 1 .. n_words = the
// unigrams of the ARPA file in file order.  An n-gram (w_1 .. w_m), w_m the predicted word, has the 64-bit key
//   packed mode (bits * order <= 64, bits = width of the largest id):  sum_i w_{m-i} << (bits * i)   -- exact, distinct by
//     construction, never 0 (every id >= 1), and the key of a suffix is a mask of the key of the whole;
//   hashed mode (otherwise): fold of lm_mix over w_m, w_{m-1}, ... -- distinctness of all stored keys is verified when the
//     table is packed (an absent n-gram then matches a stored one with probability n_cells / 2^64 per probe).
// Table: open addressing, linear probing, power-of-two cells at a load factor <= 1/2, cell = (key, logp, back-off) = 16
// bytes = one 128-bit load; key 0 = free.  Written once by mi355asr_lm_create, read-only afterwards.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LM_HD __host__ __device__ __forceinline__
#else
#define LM_HD inline
#endif

constexpr int kLmMaxOrder = 6;
constexpr float kLmOovScore = -1000.0f;   // OOV_SCORE (scorer.h:16)

struct __attribute__((aligned(16))) LmCell {
  uint64_t key;
  float logp, bo;
};

struct LmView {
  const LmCell* cells;
  uint32_t shift;     // 64 - log2(number of cells)
  uint32_t mask;      // number of cells - 1
  int32_t order;      // 1 .. kLmMaxOrder
  int32_t bits;       // > 0: packed keys of `bits` per word; 0: hashed keys
  int32_t bos;        // LM word of "<s>" (0 when the model has none: every padded n-gram is then OOV, as in the reference)
};

LM_HD uint64_t lm_mix(uint64_t h, uint32_t w) {
  const uint64_t z = (h ^ (h >> 29)) * 0x9E3779B97F4A7C15ull + (uint64_t)w;
  return (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull | 1ull;          // never 0
}
LM_HD uint32_t lm_slot(const LmView& v, uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> v.shift); }

// key of the n-gram whose words are r[0] = predicted word, r[1] = the word before it, ... r[m - 1] (host: table packing)
LM_HD uint64_t lm_key(const LmView& v, const int32_t* r, int m) {
  uint64_t k = 0;
  for (int i = 0; i < m; ++i) k = v.bits ? k | ((uint64_t)(uint32_t)r[i] << (v.bits * i)) : lm_mix(k, (uint32_t)r[i]);
  return k;
}

// get_log_cond_prob (scorer.cpp:74-93) of the n-gram r[0] = predicted word, r[1 .. order - 1] = its history backwards
// ("<s>"-padded by the caller): OOV_SCORE when any word is 0; otherwise p = logp of the longest suffix n-gram stored, plus
// the back-off weights of the contexts backed off from, shortest first (an absent context adds nothing), all in float as
// KenLM keeps them.  The 2 * order - 1 first probes are independent loads issued together; a probe that meets another
// key (load factor <= 1/2: rare) walks on.
LM_HD float lm_cond(const LmView& v, const int32_t (&r)[kLmMaxOrder]) {
  const int order = v.order;
  bool oov = false;
#pragma unroll
  for (int i = 0; i < kLmMaxOrder; ++i) oov |= i < order && r[i] == 0;
  if (oov) return kLmOovScore;
  uint64_t ks[kLmMaxOrder], kc[kLmMaxOrder];
  uint64_t s = 0, c = 0;
#pragma unroll
  for (int i = 0; i < kLmMaxOrder; ++i) {
    if (i < order) s = v.bits ? s | ((uint64_t)(uint32_t)r[i] << (v.bits * i)) : lm_mix(s, (uint32_t)r[i]);
    ks[i] = s;
    if (i >= 1 && i < order) c = v.bits ? c | ((uint64_t)(uint32_t)r[i] << (v.bits * (i - 1))) : lm_mix(c, (uint32_t)r[i]);
    kc[i] = c;
  }
  LmCell cs[kLmMaxOrder], cc[kLmMaxOrder];
  uint32_t ss[kLmMaxOrder], sc[kLmMaxOrder];
#pragma unroll
  for (int i = 0; i < kLmMaxOrder; ++i) {
    ss[i] = lm_slot(v, ks[i]);
    sc[i] = lm_slot(v, kc[i]);
    if (i < order) cs[i] = v.cells[ss[i]];
    if (i >= 1 && i < order) cc[i] = v.cells[sc[i]];
  }
  float p = 0.f;
  int found = 0;                  // length of the longest suffix n-gram stored
#pragma unroll
  for (int i = 0; i < kLmMaxOrder; ++i) {
    if (i < order) {
      while (cs[i].key != ks[i] && cs[i].key != 0) { ss[i] = (ss[i] + 1) & v.mask; cs[i] = v.cells[ss[i]]; }
      if (cs[i].key == ks[i]) { p = cs[i].logp; found = i + 1; }
    }
  }
  if (found == 0) return kLmOovScore;          // a word id without a unigram: not produced by mi355asr_lm_create's checks
#pragma unroll
  for (int i = 1; i < kLmMaxOrder; ++i) {
    if (i < order && i >= found) {            // the context of length i = r[1 .. i] was backed off from
      while (cc[i].key != kc[i] && cc[i].key != 0) { sc[i] = (sc[i] + 1) & v.mask; cc[i] = v.cells[sc[i]]; }
      if (cc[i].key == kc[i]) p += cc[i].bo;
    }
  }
  return p;
}
