// fp32 GEMM operands on the bf16 / fp16 matrix pipe: the two operand schemes of the hot path, each primitive once.
//   three terms (TM = 3): x = t0 + t1 + t2 EXACTLY, bf16 terms by truncation; six products (the term pairs with i + j <= 2) through
//     v_mfma_f32_16x16x32_bf16 -- as accurate as an fp32 FMA chain (the dropped pairs are below 2^-24 of a product);
//   two terms (TM = 2): x * s = hi + lo, fp16 terms by rounding (common.h: split_hi_f16 / split_lo_f16), s a power of two that puts
//     the operand's bound near the top of fp16's range; three products through v_mfma_f32_16x16x32_f16.
// A fragment is eight k-slots of one lane, two values per dword, one u32x4_t per term.  Per translation unit (anonymous namespace).
// tests/test_split_f16.py and tests/test_split_bf16.py compare both splits with NumPy on the hardware, bit for bit.
// Kernels whose MFMA interleaving IS their schedule (fused.hip, gemm_ring.hip, leaf.hip: the `ord - p` loops) spell the products out
// themselves; prep_sched.inc / prep2_sched.inc spell the splits out slot by slot.
#pragma once
#include "common.h"

namespace {

struct Split8x3 { u32x4_t t[3]; };           // 8 k-slots x three bf16 terms (or two fp16 terms and an unused third: split_tm)
struct Split8x2 { u32x4_t t[2]; };           // 8 k-slots x (hi, lo) fp16 terms

// exact three-term bf16 split of eight fp32 values (slots 0..3 = lo, 4..7 = hi): x = t0 + t1 + t2, each term the truncated head of
// what is left (v_perm packs the two high halves: (a0 >> 16) | (a1 & 0xffff0000)), the remainders are exact
DEV Split8x3 split8(f32x4 lo, f32x4 hi) {
  float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  Split8x3 f;
#pragma unroll
  for (int term = 0; term < 3; ++term) {
    unsigned d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned a0 = __builtin_bit_cast(unsigned, v[2 * k]), a1 = __builtin_bit_cast(unsigned, v[2 * k + 1]);
      d[k] = __builtin_amdgcn_perm(a1, a0, 0x07060302u);
      if (term < 2) {
        v[2 * k] -= __builtin_bit_cast(float, a0 & 0xffff0000u);
        v[2 * k + 1] -= __builtin_bit_cast(float, a1 & 0xffff0000u);
      }
    }
    f.t[term] = u32x4_t{d[0], d[1], d[2], d[3]};
  }
  return f;
}
// two-term fp16 split of eight values that already carry their power-of-two scale: the three-instruction split of common.h
DEV Split8x2 split8h(f32x4 lo, f32x4 hi) {
  unsigned d0[4], d1[4];
  split8_f16(lo, hi, d0, d1);
  Split8x2 f;
  f.t[0] = u32x4_t{d0[0], d0[1], d0[2], d0[3]};
  f.t[1] = u32x4_t{d1[0], d1[1], d1[2], d1[3]};
  return f;
}
// either scheme in the three-term container, for kernels that are one template over TM (t[2] is zero and unused when TM = 2)
template <int TM>
DEV Split8x3 split_tm(f32x4 lo, f32x4 hi) {
  if constexpr (TM == 2) {
    const Split8x2 h = split8h(lo, hi);
    Split8x3 f;
    f.t[0] = h.t[0];
    f.t[1] = h.t[1];
    f.t[2] = u32x4_t{0u, 0u, 0u, 0u};
    return f;
  } else {
    return split8(lo, hi);
  }
}

// c += A(16 x 32) B(32 x 16) on fragments of one term each
DEV f32x4 mma32(u32x4_t a, u32x4_t b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
DEV f32x4 mma32h(u32x4_t a, u32x4_t b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
template <int TM>
DEV f32x4 mma32_tm(u32x4_t a, u32x4_t b, f32x4 c) {
  if constexpr (TM == 2) return mma32h(a, b, c); else return mma32(a, b, c);
}
// c += A B with both operands split, smallest products first.  TM = 3: the six bf16 term pairs with i + j <= 2 (order 2, then 1,
// then 0); TM = 2: the three fp16 ones, lo x hi, hi x lo, hi x hi.
template <int TM>
DEV f32x4 mma_tm(const u32x4_t (&a)[3], const Split8x3& b, f32x4 c) {
  if constexpr (TM == 2) {
    c = mma32h(a[1], b.t[0], c);
    c = mma32h(a[0], b.t[1], c);
    c = mma32h(a[0], b.t[0], c);
  } else {
    c = mma32(a[2], b.t[0], c);
    c = mma32(a[1], b.t[1], c);
    c = mma32(a[0], b.t[2], c);
    c = mma32(a[1], b.t[0], c);
    c = mma32(a[0], b.t[1], c);
    c = mma32(a[0], b.t[0], c);
  }
  return c;
}

// ---- power-of-two scales of the two-term scheme ---------------------------------------------------------------------------------
// 2^k with bound * 2^k in [2^13, 2^14), k clamped to [-14, KMAX], from the exponent field of `bound` (>= 0; 0 gives 2^KMAX).
// KMAX = 15 where the scale itself is an fp16 operand (the bias slot of the dmodel-144 block kernels); where it only ever multiplies
// fp32 values (fft_stft.hip: 100) nothing ties it to fp16's range and a quiet signal keeps both terms normal.
template <int KMAX>
DEV float pow2_scale(float bound) {
  const int e = (int)((__builtin_bit_cast(unsigned, bound) >> 23) & 255u);          // bound in [2^(e - 127), 2^(e - 126))
  const int k = min(KMAX, max(-14, 140 - e));
  return __builtin_bit_cast(float, (unsigned)(127 + k) << 23);
}
DEV float recip_pow2(float s) {               // 1 / s for a power of two (exact; exponent field 1 .. 253)
  return __builtin_bit_cast(float, 0x7f000000u - __builtin_bit_cast(unsigned, s));
}
// largest magnitude of this lane's token row of 16 N features (the row is spread over the four lanes c, c + 16, c + 32, c + 48)
template <int N>
DEV float row_max(const f32x4 (&xs)[N]) {
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i)
    m = fmaxf(fmaxf(m, fmaxf(fabsf(xs[i].x), fabsf(xs[i].y))), fmaxf(fabsf(xs[i].z), fabsf(xs[i].w)));
  return group_max(m);
}
// largest magnitude of one lane's eight values of a k-step (no reduction over lanes)
DEV float max8(f32x4 a, f32x4 b) {
  return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))), fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
}

}  // namespace
