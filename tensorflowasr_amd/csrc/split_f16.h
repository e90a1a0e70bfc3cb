// Two-term fp16 operand scheme of the dmodel-144 block kernels (fused_pp.hip, fused_ns.hip), on the primitives of mfma_ops.h (split8h,
// pow2_scale<15>, recip_pow2, row_max): the generated activation + split schedule (prep2_sched.inc), a chain's per-token scales and
// the split of a token row into the operands of its k-steps.  Per translation unit (anonymous namespace): included once by each
// kernel file.  See the header of fused_pp.hip for the arithmetic.
#pragma once
#include "block144.h"
#include "common.h"
#include "launch.h"
#include "mfma_ops.h"

namespace {

using Split8 = Split8x2;                     // mfma_ops.h (split8h); the name the generated schedules use

// activation + two-term split of two finished hidden tiles, in slots of <= 2 instructions (prep2_sched.inc).  k1 = -log2 e /
// (unit of the hidden accumulators), ik2 = that unit / (unit of the operand being built): per-lane values
struct Prep2Ctx {
  f32x4 &lo, &hi;
  Split8& out;
  float k1, ik2;
  float ta, tb;
  unsigned hp;
};
using PpPrep = Prep2Ctx;
#include "prep2_sched.inc"

// scales of one chain y += W2 act(W1aug [x ; 1]) for this lane's token (ChainSc: the chain's host-side constants)
struct PpTok { float sx, k1, ik2, s2, inv2; };
DEV PpTok pp_chain_scales(const PpChainSc& c, float xmax) {
  PpTok t;
  t.sx = pow2_scale<15>(xmax);
  const float sh = pow2_scale<15>(fmaf(c.l1, xmax, c.bmax));      // |swish(h)| <= |h| <= l1 max|x| + max|b|
  const float u1 = c.sw1 * t.sx;                                  // unit of the hidden accumulators
  t.k1 = -1.4426950408889634f * recip_pow2(u1);
  t.ik2 = u1 * recip_pow2(sh);
  t.s2 = c.sw2 * sh;                                              // unit of the output accumulators
  t.inv2 = recip_pow2(t.s2);
  return t;
}
// the five split operands of a 16-token tile for the W1 steps, in units of sx; k-slot 144 (the first padding slot of step 4)
// carries 1.0 (= sx in those units): row 144 of the streamed W1 holds the bias
template <int KS>
DEV void split_operand(Split8 (&xf)[KS], const f32x4 (&xs)[KB], int g4, float sx) {
  const f32x4 s4 = splat4(sx);
#pragma unroll
  for (int t = 0; t < KS - 1; ++t) xf[t] = split8h(xs[2 * t] * s4, xs[2 * t + 1] * s4);
  f32x4 oh = splat4(0.f);
  oh.x = g4 == 0 ? sx : 0.0f;
  xf[KS - 1] = split8h(xs[KB - 1] * s4, oh);
}

}  // namespace
