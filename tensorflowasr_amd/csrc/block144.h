// Per-wave scaffolding of the dmodel-144 block kernels (fused.hip, fused_pp.hip, fused_ns.hip): LayerNorm on a wave's register-
// resident token rows with the parameters in LDS, and -- for the kernels whose consumer waves own 16 tokens each (the first two) --
// which tokens a wave owns.  Per translation unit (anonymous namespace).
#pragma once
#include "common.h"
#include "wstream.h"

namespace {

constexpr int D = 144;
constexpr int KB = D / 16;   // 9

struct WaveCtx {
  int lane, g4, t, tok;
  size_t row;
  bool live;
};
// T > 0: utterance-aligned tiling (depthwise conv folded in): workgroup (blockIdx.x, blockIdx.y) = 64-frame chunk blockIdx.x of
// utterance blockIdx.y, so that the conv window of a workgroup never crosses an utterance; T = 0: tokens tiled flat.
// CLAMP_TOK = false leaves `tok` of a lane past the end (flat tiling) as it is: fused.hip's head kernel forms its guarded output
// addresses from it, and its code is kept as it was.
template <bool CLAMP_TOK>
DEV void tok_of(WaveCtx& c, unsigned tid, int M, int T) {
  c.lane = tid & 63;
  c.g4 = (c.lane >> 4) * 4;
  c.t = c.lane & 15;
  const int wv = (int)(tid >> 6);
  if (T > 0) {
    const int f = (blockIdx.x * WAVES_PER_BLOCK + wv) * 16 + c.t;      // frame inside the utterance
    c.live = f < T;
    c.tok = blockIdx.y * T + min(f, T - 1);                             // frames past the end recompute the last one
    c.row = (size_t)c.tok * D;
    return;
  }
  const int wid = blockIdx.x * WAVES_PER_BLOCK + wv;
  c.tok = wid * 16 + c.t;
  c.live = c.tok < M;
  c.row = (size_t)min(c.tok, M - 1) * D;     // waves past the end recompute the last token and store nothing
  if (CLAMP_TOK && !c.live) c.tok = M - 1;
}
template <bool CLAMP_TOK = true>
DEV WaveCtx wave_ctx(int M, int T = 0) {
  WaveCtx c;
  tok_of<CLAMP_TOK>(c, threadIdx.x, M, T);
  return c;
}
// the same, recomputed from an opaque copy of the thread index: long kernels call this again before their stores instead of
// keeping the 64-bit row offset alive across the whole stream (it was the value the register allocator spilled)
template <bool CLAMP_TOK = true>
DEV WaveCtx wave_ctx_fresh(int M, int T = 0) {
  unsigned tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  WaveCtx c;
  tok_of<CLAMP_TOK>(c, tid, M, T);
  return c;
}

// LayerNorm with gamma / beta in LDS
DEV void ln_lds(f32x4 (&xs)[KB], const float* ga, const float* be, int g4, float eps) {
  float mean, rstd;
  ln_stats<KB>(xs, eps, mean, rstd);
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) xs[kb] = (xs[kb] - splat4(mean)) * splat4(rstd) * lds4(ga, kb, g4) + lds4(be, kb, g4);
}

}  // namespace
