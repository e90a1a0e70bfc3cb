// CTC over a [T, 2U+1] lattice: the loss (sum over paths), its gradient with respect to the logits, and the best path (forced
// alignment).  replaces: tf.keras.backend.ctc_batch_cost (asr/trainer/ctc_runners.py:91,133; chunk_conformer_blocks.py:1058-1075,
// 1142-1159), i.e. tf.compat.v1.nn.ctc_loss on log(y_pred + 1e-7) with the blank as the last class.
//
// The class distribution of a frame is q = (p + 1e-7) / sum_k (p_k + 1e-7), p = softmax(z) for the logits entry.  Three stages:
//
//   ctc_rows_kernel     one wave per frame: ONE read of the V-wide row (running maximum and sum of exp per lane, merged across the
//                       wave), then log q of the U_b labels and of the blank gathered into lp [B, T, U+1].  Nothing after it
//                       reads a V-wide row, except the gradient's own pass.
//   ctc_lattice_kernel  one workgroup per (utterance, direction), serial in t.  Thread u owns the states "blank before label u"
//                       (2u) and "label u" (2u+1), so a frame needs ONE value from the neighbour: log alpha of label u-1 (a
//                       cross-lane move in a single wave up to U = 63, a double-buffered LDS slot and one barrier above).
//                       beta is alpha of the reversed problem (labels and frames reversed), so the same code runs both, as the
//                       two workgroups blockIdx.y = 0 / 1, concurrently.  Log domain, f32; after every frame the maximum over
//                       the states is subtracted and added to a double accumulator, so stored values stay within a few units of
//                       0 and alpha + beta - log P does not cancel at losses in the thousands.  The max variant (Viterbi) keeps
//                       one back-pointer byte per (frame, state) and thread 0 walks them back into path and spans.
//   ctc_grad_kernel     one workgroup per frame.  Occupancy of a state = exp(alpha + beta - lp + (norms - log P)); states of
//                       one class are summed along the utterance's "next position with the same label" chain (built once by
//                       the beta workgroup), a fixed order: no floating-point atomics, bit-identical from run to run and
//                       independent of the rest of the batch.  With o_k = occ_k / (p_k + 1e-7) and W = sum_k p_k o_k,
//                       dL/dz_j = p_j (W - o_j) (the q_k / (p_k + 1e-7) terms are the constant 1 / sum(p + 1e-7) and cancel
//                       against sum_k p_k = 1): the row is written as p_j W and the <= U_b + 1 touched classes are rewritten.
//
// Infeasible targets (fewer frames than labels + adjacent repeats), a label outside [0, V) or equal to the blank: loss +inf,
// gradient rows 0, alignment score -inf with path and spans -1.  Frames t >= in_len[b] are never read.
#include "ctc_lattice.h"

#include <cmath>

namespace mi355 {
namespace {

constexpr float kEps = 1e-7f;   // keras.backend.epsilon()

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// butterfly: every lane adds the same pairs in the same order, so all lanes hold the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// The two cross-lane steps of the lattice's serial chain, as DPP moves inside the VALU instead of trips through the LDS crossbar
// (__shfl_*): the maximum over the wave (exact and order-independent, so every lane and every workgroup shape gets the same
// bits) and "the value of the lane below" (lane 0 receives `fill`).
template <int CTRL>
__device__ __forceinline__ float dpp_move(float fill, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = fmaxf(v, dpp_move<0xB1>(v, v));     // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_move<0x4E>(v, v));     // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_move<0x124>(v, v));    // row_ror:4
  v = fmaxf(v, dpp_move<0x128>(v, v));    // row_ror:8: every lane holds the maximum of its row of 16
  const int i = __float_as_int(v);
  return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 0)), __int_as_float(__builtin_amdgcn_readlane(i, 16))),
               fmaxf(__int_as_float(__builtin_amdgcn_readlane(i, 32)), __int_as_float(__builtin_amdgcn_readlane(i, 48))));
}
__device__ __forceinline__ float lane_below(float v, float fill) { return dpp_move<0x138>(fill, v); }   // wave_shr:1

__device__ __forceinline__ float prob_of(float z, float mx, float se) { return expf(z - mx) / se; }

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return m;
  return m + logf(1.f + expf(fminf(a, b) - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return m;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- row stage -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_rows_kernel(CtcRowArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)a.B * a.T) return;
  const int b = (int)(row / a.T), t = (int)(row % a.T);
  const int Tb = a.in_len ? clampi(a.in_len[b], 0, a.T) : a.T;
  if (t >= Tb) return;                                     // frames past the utterance are never read
  const int Ub = clampi(a.label_len[b], 0, a.U);
  const float* x = a.x + (size_t)row * a.V;
  const int V = a.V;
  float mx = 0.f, se = 1.f, log_den = a.log_den;
  if (a.is_logits) {
    float m = -INFINITY, s = 0.f;
    if ((V & 3) == 0) {
      const float4* x4 = reinterpret_cast<const float4*>(x);
      for (int i = lane; i < V / 4; i += 64) {
        const float4 v = x4[i];
        const float nm = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        s = s * expf(m - nm) + ((expf(v.x - nm) + expf(v.y - nm)) + (expf(v.z - nm) + expf(v.w - nm)));
        m = nm;
      }
    } else {
      for (int i = lane; i < V; i += 64) {
        const float v = x[i];
        const float nm = fmaxf(m, v);
        s = s * expf(m - nm) + expf(v - nm);
        m = nm;
      }
    }
    mx = wave_max(m);
    se = wave_sum(m == -INFINITY ? 0.f : s * expf(m - mx));   // a lane without elements (V < 64) holds m = -inf, s = 0
    if (a.stat && lane == 0) {
      a.stat[row * 2] = mx;
      a.stat[row * 2 + 1] = se;
    }
  } else {
    float s = 0.f;
    for (int i = lane; i < V; i += 64) s += x[i];
    s = wave_sum(s);
    log_den = (float)log((double)s + (double)V * 1e-7);
  }
  float* lp = a.lp + (size_t)row * (a.U + 1);
  const int32_t* lab = a.labels + (size_t)b * a.U;
  for (int i = lane; i <= Ub; i += 64) {
    const int cls = i < Ub ? lab[i] : a.blank;
    float v = -INFINITY;                                   // a label outside [0, V): the lattice stage rejects the utterance
    if ((unsigned)cls < (unsigned)V) {
      const float p = a.is_logits ? prob_of(x[cls], mx, se) : x[cls];
      v = logf(p + kEps) - log_den;
    }
    lp[i < Ub ? i : a.U] = v;
  }
}

// ---- lattice stage ---------------------------------------------------------------------------------------------------------
template <bool VITERBI, bool MULTI>
__global__ __launch_bounds__(512) void ctc_lattice_kernel(CtcLatticeArgs a) {
  __shared__ int32_t sh_lab[kCtcMaxU + 1];
  __shared__ float sh_x[2][512];
  __shared__ float sh_m[2][8];
  __shared__ float sh_fin[2];
  __shared__ int sh_cnt[2];
  const int b = blockIdx.x, dir = blockIdx.y, u = threadIdx.x, NT = blockDim.x;
  const int U = a.U, T = a.T, S = 2 * U + 1;
  const int Ub = clampi(a.label_len[b], 0, U);
  const int Tb = a.in_len ? clampi(a.in_len[b], 0, T) : T;
  const int Sb = 2 * Ub + 1;
  const int32_t* lab = a.labels + (size_t)b * U;

  if (u == 0) sh_cnt[0] = sh_cnt[1] = 0;
  for (int i = u; i < Ub; i += NT) sh_lab[i] = lab[i];
  if (VITERBI) {
    for (int i = u; i < T; i += NT) a.path[(size_t)b * T + i] = -1;
    for (int i = u; i < 2 * U; i += NT) a.spans[(size_t)b * 2 * U + i] = -1;
  }
  __syncthreads();
  {
    int bad = 0, rep = 0;
    for (int i = u; i < Ub; i += NT) {
      const int l = sh_lab[i];
      if ((unsigned)l >= (unsigned)a.V || l == a.blank) bad = 1;
      if (i > 0 && l == sh_lab[i - 1]) ++rep;
    }
    if (bad) atomicOr(&sh_cnt[0], 1);
    if (rep) atomicAdd(&sh_cnt[1], rep);
  }
  __syncthreads();
  const bool feasible = !sh_cnt[0] && Tb >= 1 && Tb >= Ub + sh_cnt[1];
  if (!feasible) {
    if (u == 0 && dir == 0) {
      if (VITERBI) {
        a.score[b] = -INFINITY;
      } else {
        a.loss[b] = INFINITY;
        a.logp[b] = -(double)INFINITY;
        a.feasible[b] = 0;
      }
    }
    return;
  }
  if (!VITERBI && dir == 1 && a.chain) {
    // per utterance, once: the next position with the same label, and whether a position is the first of its label
    for (int i = u; i < Ub; i += NT) {
      const int l = sh_lab[i];
      int nxt = -1, first = 1;
      for (int j = i + 1; j < Ub; ++j)
        if (sh_lab[j] == l) { nxt = j; break; }
      for (int j = i - 1; j >= 0; --j)
        if (sh_lab[j] == l) { first = 0; break; }
      a.chain[(size_t)b * U + i] = (nxt + 1) | (first << 16);
    }
  }

  // thread u: blank before label u (state 2u) and label u (state 2u + 1) of the problem as this direction sees it
  const bool has_blank = u <= Ub, has_lab = u < Ub;
  const int ul = dir ? Ub - 1 - u : u;                     // position of "label u" among the utterance's labels
  const bool skip = has_lab && u > 0 && sh_lab[ul] != sh_lab[dir ? ul + 1 : ul - 1];
  const int sB = dir ? Sb - 1 - 2 * u : 2 * u, sL = dir ? Sb - 2 - 2 * u : 2 * u + 1;
  const float* lpu = a.lp + (size_t)b * T * (U + 1);
  const int colL = has_lab ? ul : U;
  auto frame_of = [&](int tt) { return dir ? Tb - 1 - tt : tt; };
  auto load_b = [&](int tt) { return tt < Tb ? lpu[(size_t)frame_of(tt) * (U + 1) + U] : 0.f; };
  auto load_l = [&](int tt) { return (tt < Tb && has_lab) ? lpu[(size_t)frame_of(tt) * (U + 1) + colL] : 0.f; };

  float vb = -INFINITY, vl = -INFINITY;                    // normalised log alpha of the two states
  double csum = 0.0;                                       // what has been subtracted so far
  float b1 = load_b(0), l1 = load_l(0), b2 = load_b(1), l2 = load_l(1), b3 = load_b(2), l3 = load_l(2);
  for (int tt = 0; tt < Tb; ++tt) {
    const float lpb = b1, lpl = l1;
    b1 = b2; l1 = l2; b2 = b3; l2 = l3;
    b3 = load_b(tt + 3); l3 = load_l(tt + 3);              // three frames ahead of the serial chain
    float nb, nl;
    int kb = 0, kl = 0;
    if (tt == 0) {
      nb = (u == 0) ? lpb : -INFINITY;
      nl = (u == 0 && has_lab) ? lpl : -INFINITY;
    } else {
      float left;                                          // label u-1 of the previous frame
      if (MULTI) {
        sh_x[tt & 1][u] = vl;
        __syncthreads();
        left = u > 0 ? sh_x[tt & 1][u - 1] : -INFINITY;
      } else {
        left = lane_below(vl, -INFINITY);
      }
      if (VITERBI) {
        nb = vb; kb = 0;
        if (left > nb) { nb = left; kb = 1; }
        nl = vl; kl = 0;
        if (vb > nl) { nl = vb; kl = 1; }
        if (skip && left > nl) { nl = left; kl = 2; }
      } else {
        nb = lse2(vb, left);
        nl = lse3(vl, vb, skip ? left : -INFINITY);
      }
      nb = has_blank ? nb + lpb : -INFINITY;
      nl = has_lab ? nl + lpl : -INFINITY;
    }
    float m = wave_max_dpp(fmaxf(nb, nl));
    if (MULTI) {
      if ((u & 63) == 0) sh_m[tt & 1][u >> 6] = m;
      __syncthreads();
      m = sh_m[tt & 1][0];
      for (int w = 1; w < (NT >> 6); ++w) m = fmaxf(m, sh_m[tt & 1][w]);
    }
    if (!(m > -INFINITY)) m = 0.f;
    vb = nb - m;
    vl = nl - m;
    csum += (double)m;
    const int t = frame_of(tt);
    if (VITERBI) {
      uint8_t* bp = a.bp + ((size_t)b * T + t) * S;
      if (has_blank) bp[2 * u] = (uint8_t)kb;
      if (has_lab) bp[2 * u + 1] = (uint8_t)kl;
    } else if (a.ab) {
      float* row = a.ab + (((size_t)dir * a.B + b) * T + t) * S;
      if (has_blank) row[sB] = vb;
      if (has_lab) row[sL] = vl;
      if (u == 0) a.norm[((size_t)dir * a.B + b) * T + t] = csum;
    }
  }
  if (dir != 0) return;
  if (u == Ub) sh_fin[0] = vb;
  if (u == Ub - 1) sh_fin[1] = vl;
  if (Ub == 0 && u == 0) sh_fin[1] = -INFINITY;
  __threadfence_block();
  __syncthreads();
  if (u != 0) return;
  if (!VITERBI) {
    const double lp_total = csum + (double)lse2(sh_fin[0], sh_fin[1]);
    a.logp[b] = lp_total;
    a.feasible[b] = 1;
    a.loss[b] = (float)(-lp_total);
    return;
  }
  int s = sh_fin[1] > sh_fin[0] ? 2 * Ub - 1 : 2 * Ub;
  a.score[b] = (float)(csum + (double)fmaxf(sh_fin[0], sh_fin[1]));
  int prev = -1;
  int32_t* path = a.path + (size_t)b * T;
  int32_t* spans = a.spans + (size_t)b * 2 * U;
  for (int t = Tb - 1; t >= 0; --t) {
    if (s & 1) {
      path[t] = sh_lab[s >> 1];
      spans[2 * (s >> 1)] = t;
      if (s != prev) spans[2 * (s >> 1) + 1] = t;
    } else {
      path[t] = a.blank;
    }
    prev = s;
    s -= a.bp[((size_t)b * T + t) * S + s];
  }
}

// ---- gradient stage --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();                                         // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void ctc_grad_kernel(CtcGradArgs a) {
  __shared__ float sh_occ[kCtcMaxU + 1];
  __shared__ float sh_o[kCtcMaxU + 1];
  __shared__ float sh_red[4];
  const long long row = blockIdx.x;
  const int tid = threadIdx.x;
  const int b = (int)(row / a.T), t = (int)(row % a.T);
  const int V = a.V, U = a.U, S = 2 * U + 1;
  const int Tb = a.in_len ? clampi(a.in_len[b], 0, a.T) : a.T;
  float* g = a.grad + (size_t)row * V;
  if (t >= Tb || !a.feasible[b]) {
    for (int j = tid; j < V; j += 256) g[j] = 0.f;
    return;
  }
  const int Ub = clampi(a.label_len[b], 0, U);
  const float* x = a.x + (size_t)row * V;
  const float mx = a.stat[row * 2], se = a.stat[row * 2 + 1];
  const double k = a.norm[(size_t)b * a.T + t] + a.norm[((size_t)a.B + b) * a.T + t] - a.logp[b];
  const float* al = a.ab + (size_t)row * S;
  const float* be = a.ab + ((size_t)a.B * a.T + row) * S;
  const float* lp = a.lp + (size_t)row * (U + 1);
  const int32_t* lab = a.labels + (size_t)b * U;
  const int32_t* chain = a.chain + (size_t)b * U;
  const double lpb = (double)lp[U];
  float part = 0.f;
  for (int u = tid; u <= Ub; u += 256) {
    part += expf((float)((double)al[2 * u] + (double)be[2 * u] - lpb + k));
    if (u < Ub) sh_occ[u] = expf((float)((double)al[2 * u + 1] + (double)be[2 * u + 1] - (double)lp[u] + k));
  }
  const float occ_blank = block_sum256(part, sh_red);      // its barriers also publish sh_occ
  float term = 0.f;
  for (int u = tid; u < Ub; u += 256) {
    const int c = chain[u];
    if (c >> 16) {
      float s = sh_occ[u];
      for (int v = (c & 0xffff) - 1; v >= 0; v = (chain[v] & 0xffff) - 1) s += sh_occ[v];
      const float p = prob_of(x[lab[u]], mx, se);
      const float o = s / (p + kEps);
      sh_o[u] = o;
      term += p * o;
    }
  }
  const float pb = prob_of(x[a.blank], mx, se);
  const float ob = occ_blank / (pb + kEps);
  if (tid == 0) term += pb * ob;
  const float W = block_sum256(term, sh_red);
  if ((V & 3) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* g4 = reinterpret_cast<float4*>(g);
    for (int j = tid; j < V / 4; j += 256) {
      const float4 z = x4[j];
      g4[j] = make_float4(prob_of(z.x, mx, se) * W, prob_of(z.y, mx, se) * W, prob_of(z.z, mx, se) * W, prob_of(z.w, mx, se) * W);
    }
  } else {
    for (int j = tid; j < V; j += 256) g[j] = prob_of(x[j], mx, se) * W;
  }
  __threadfence_block();
  __syncthreads();                                         // the row is written; now the classes the lattice touches
  for (int u = tid; u < Ub; u += 256) {
    if (chain[u] >> 16) {
      const int cls = lab[u];
      g[cls] = prob_of(x[cls], mx, se) * (W - sh_o[u]);
    }
  }
  if (tid == 0) g[a.blank] = pb * (W - ob);
}

}  // namespace

int launch_ctc_rows(const CtcRowArgs& a, hipStream_t s) {
  const long long rows = (long long)a.B * a.T;
  hipLaunchKernelGGL(ctc_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
  return 0;
}

int launch_ctc_lattice(const CtcLatticeArgs& a, bool viterbi, int directions, hipStream_t s) {
  if (a.U > kCtcMaxU) return -1;
  const int nt = ((a.U + 1 + 63) / 64) * 64;
  const dim3 grid(a.B, directions), block(nt);
  if (viterbi) {
    if (nt > 64) hipLaunchKernelGGL((ctc_lattice_kernel<true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ctc_lattice_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (nt > 64) hipLaunchKernelGGL((ctc_lattice_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ctc_lattice_kernel<false, false>), grid, block, 0, s, a);
  }
  return 0;
}

int launch_ctc_grad(const CtcGradArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)((long long)a.B * a.T)), dim3(256), 0, s, a);
  return 0;
}

}  // namespace mi355
