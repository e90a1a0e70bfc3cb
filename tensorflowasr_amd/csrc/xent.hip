// Softmax cross-entropy from logits with its arg-max and its gradient, and the batch reductions of the trainer's mask_loss /
// translate_acc (asr/trainer/ctc_runners.py:63-76, 144) behind mi355asr_xent_rows / mi355asr_mask_loss of include/mi355asr.h.
//
// xent_rows_kernel: one workgroup of 256 threads per row (b, t < Q) of V logits.  Element i belongs to float4 k = i / 4, which is
// slot q = k / 256 of thread k % 256 -- a function of the INDEX alone, never of the row's address, so the order of every sum is
// the same wherever the row lies.  A row whose address is 16-byte aligned is read with one 16-byte load per float4, any other
// row with four 4-byte loads of the same elements; the last, partial float4 is read element by element and nothing at i >= V
// is read.  Rows of up to kXentResidentV = 10 240 classes stay in registers (10 float4 per thread) from the one read to the last
// use; longer rows are read again by the exp-sum pass and by the gradient pass, through L2 (a row is at most 1 MiB).
//   pass 1  m = max, arg-max (the lowest index among equals: (x > best) || (x == best && i < index), the same rule in a thread,
//           across a wave and across the four waves), and x[y] picked out by the thread that owns element y
//   pass 2  e_i = expf(x_i - m) summed per float4 component over the thread's slots in order, then (a0 + a1) + (a2 + a3), then a
//           6-step xor butterfly in the wave, then the four wave sums added in wave order
//   loss    logf(s) + (m - x[y]); a label outside [0, V) gives NaN
//   pass 3  grad_i = (e_i * (w / s)) - (i == y ? w : 0); a label outside [0, V) gives a row of zeros
// No atomics, no workspace, no dependence on anything but the row.
//
// xent_weights_kernel / xent_reduce_kernel: one workgroup of 1 024 threads per call; thread j takes the elements j, j + 1024, ...
// of the [B, Q] plane in order and adds them in float64, the 64 lanes are added by an xor butterfly and the 16 wave sums in wave
// order; the per-row means are one wave per row the same way.
#include "xent.h"

#include <cmath>

#include "common.h"

namespace mi355 {
namespace {

constexpr int kBatchThreads = 1024;

DEV bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the float4 of elements i0 .. i0 + 3 of a row; elements at or past V are never read and come back as -inf
DEV f32x4 load_quad(const float* __restrict__ row, int i0, int V, bool wide) {
  const float ninf = -INFINITY;
  f32x4 v = {ninf, ninf, ninf, ninf};
  if (i0 + 3 < V) {
    if (wide) {
      v = ldg4(row + i0);
    } else {
      v.x = row[i0]; v.y = row[i0 + 1]; v.z = row[i0 + 2]; v.w = row[i0 + 3];
    }
  } else {
    if (i0 < V) v.x = row[i0];
    if (i0 + 1 < V) v.y = row[i0 + 1];
    if (i0 + 2 < V) v.z = row[i0 + 2];
  }
  return v;
}

DEV void store_quad(float* __restrict__ row, int i0, int V, bool wide, f32x4 v) {
  if (i0 + 3 < V) {
    if (wide) {
      stg4(row + i0, v);
    } else {
      row[i0] = v.x; row[i0 + 1] = v.y; row[i0 + 2] = v.z; row[i0 + 3] = v.w;
    }
  } else {
    if (i0 < V) row[i0] = v.x;
    if (i0 + 1 < V) row[i0 + 1] = v.y;
    if (i0 + 2 < V) row[i0 + 2] = v.z;
  }
}

DEV void scan_quad(f32x4 v, int i0, int V, int y, float& bv, int& bi, float& xy, bool& mine) {
  const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + j;
    if (i < V && better(c[j], i, bv, bi)) { bv = c[j]; bi = i; }
    if (i == y) { xy = c[j]; mine = true; }
  }
}

DEV f32x4 exp_quad(f32x4 v, int i0, int V, float m) {
  f32x4 e;
  e.x = i0 < V ? expf(v.x - m) : 0.f;
  e.y = i0 + 1 < V ? expf(v.y - m) : 0.f;
  e.z = i0 + 2 < V ? expf(v.z - m) : 0.f;
  e.w = i0 + 3 < V ? expf(v.w - m) : 0.f;
  return e;
}

DEV f32x4 grad_quad(f32x4 e, int i0, int y, float scale, float w) {
  f32x4 g;
  g.x = e.x * scale - (i0 == y ? w : 0.f);
  g.y = e.y * scale - (i0 + 1 == y ? w : 0.f);
  g.z = e.z * scale - (i0 + 2 == y ? w : 0.f);
  g.w = e.w * scale - (i0 + 3 == y ? w : 0.f);
  return g;
}

template <bool RESIDENT>
__global__ __launch_bounds__(kXentThreads) void xent_rows_kernel(XentRowsArgs a) {
  __shared__ float sh_v[kXentThreads / 64];
  __shared__ int sh_i[kXentThreads / 64];
  __shared__ float sh_s[kXentThreads / 64];
  __shared__ float sh_xy;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)(blockIdx.x / (unsigned)a.Q), t = (int)(blockIdx.x % (unsigned)a.Q);
  const int V = a.V;
  const float* __restrict__ row = a.x + (int64_t)b * a.ld_b + (int64_t)t * a.ld_t;
  const bool wide = ((uintptr_t)row & 15) == 0;
  const int y = a.labels[(int64_t)b * a.ld_lab + t];
  const bool valid = y >= 0 && y < V;
  const int nslots = (((V + 3) >> 2) + kXentThreads - 1) / kXentThreads;   // the same for every thread

  // ---- pass 1: the one read, maximum, arg-max, x[y] -------------------------------------------------------------------------
  f32x4 xs[RESIDENT ? kXentSlots : 1];
  float bv = -INFINITY, xy = 0.f;
  int bi = 0x7fffffff;
  bool mine = false;
  if (RESIDENT) {
    // a slot past the row's last (q >= nslots, the same for the whole workgroup) is skipped by a scalar branch in every pass
#pragma unroll
    for (int q = 0; q < kXentSlots; ++q)
      if (q < nslots) xs[q] = load_quad(row, 4 * (q * kXentThreads + tid), V, wide);
#pragma unroll
    for (int q = 0; q < kXentSlots; ++q)
      if (q < nslots) scan_quad(xs[q], 4 * (q * kXentThreads + tid), V, y, bv, bi, xy, mine);
  } else {
    for (int q = 0; q < nslots; ++q) {
      const int i0 = 4 * (q * kXentThreads + tid);
      scan_quad(load_quad(row, i0, V, wide), i0, V, y, bv, bi, xy, mine);
    }
  }
  if (mine) sh_xy = xy;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { sh_v[wave] = bv; sh_i[wave] = bi; }
  __syncthreads();
  bv = sh_v[0]; bi = sh_i[0];
#pragma unroll
  for (int w = 1; w < kXentThreads / 64; ++w)
    if (better(sh_v[w], sh_i[w], bv, bi)) { bv = sh_v[w]; bi = sh_i[w]; }
  const float m = bv;

  // ---- pass 2: the exponentials and their sum --------------------------------------------------------------------------------
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (RESIDENT) {
#pragma unroll
    for (int q = 0; q < kXentSlots; ++q)
      if (q < nslots) {
        xs[q] = exp_quad(xs[q], 4 * (q * kXentThreads + tid), V, m);
        acc += xs[q];
      }
  } else {
    for (int q = 0; q < nslots; ++q) {
      const int i0 = 4 * (q * kXentThreads + tid);
      acc += exp_quad(load_quad(row, i0, V, wide), i0, V, m);
    }
  }
  float s = (acc.x + acc.y) + (acc.z + acc.w);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) sh_s[wave] = s;
  __syncthreads();
  s = sh_s[0];
#pragma unroll
  for (int w = 1; w < kXentThreads / 64; ++w) s += sh_s[w];

  if (tid == 0) {
    const int64_t o = (int64_t)b * a.Q + t;
    a.loss[o] = valid ? logf(s) + (m - sh_xy) : NAN;
    if (a.amax) a.amax[o] = bi < V ? bi : 0;      // a row with no comparable element (all NaN): class 0
  }
  if (!a.grad) return;

  // ---- pass 3: w * (softmax - onehot) ------------------------------------------------------------------------------------------
  float* __restrict__ grow = a.grad + (int64_t)b * a.gld_b + (int64_t)t * a.gld_t;
  const bool gwide = ((uintptr_t)grow & 15) == 0;
  const float w = a.w ? a.w[(int64_t)b * a.Q + t] : 1.f;
  const float scale = valid ? w / s : 0.f;
  const float wy = valid ? w : 0.f;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (RESIDENT) {
#pragma unroll
    for (int q = 0; q < kXentSlots; ++q) {
      const int i0 = 4 * (q * kXentThreads + tid);
      if (q < nslots) store_quad(grow, i0, V, gwide, valid ? grad_quad(xs[q], i0, y, scale, wy) : zero);
    }
  } else {
    for (int q = 0; q < nslots; ++q) {
      const int i0 = 4 * (q * kXentThreads + tid);
      const f32x4 g = valid ? grad_quad(exp_quad(load_quad(row, i0, V, wide), i0, V, m), i0, y, scale, wy) : zero;
      store_quad(grow, i0, V, gwide, g);
    }
  }
}

// sum over the workgroup in float64: xor butterfly in the wave, then the wave sums in wave order; every thread gets the total
DEV double block_sum(double v, double* sh, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                       // the previous call's readers are done with sh
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  double tot = sh[0];
#pragma unroll
  for (int w = 1; w < kBatchThreads / 64; ++w) tot += sh[w];
  return tot;
}

// need = (label != 0), zero = (label == 0) counted over the [B, Q] plane: exact in float64
DEV double count_need(const XentBatchArgs& a, double* sh, int tid) {
  const int64_t n = (int64_t)a.B * a.Q;
  double c = 0.0;
  for (int64_t i = tid; i < n; i += kBatchThreads) c += a.labels[(i / a.Q) * a.ld_lab + i % a.Q] != 0 ? 1.0 : 0.0;
  return block_sum(c, sh, tid);
}

__global__ __launch_bounds__(kBatchThreads) void xent_weights_kernel(XentBatchArgs a) {
  __shared__ double sh[kBatchThreads / 64];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)a.B * a.Q;
  const double n_need = count_need(a, sh, tid), n_zero = (double)n - n_need;
  double g = 0.0;
  for (int b = tid; b < a.B; b += kBatchThreads) g += a.upstream ? (double)a.upstream[b] : 1.0;
  const double G = block_sum(g, sh, tid);
  const double w_need = G / (n_need + 1e-6), w_zero = G / (n_zero + 1e-6);
  for (int64_t i = tid; i < n; i += kBatchThreads) {
    const int64_t b = i / a.Q;
    const double gb = a.upstream ? (double)a.upstream[b] : 1.0;
    a.w[i] = (float)(gb / a.Q + (a.labels[b * a.ld_lab + i % a.Q] != 0 ? w_need : w_zero));
  }
}

__global__ __launch_bounds__(kBatchThreads) void xent_reduce_kernel(XentBatchArgs a) {
  __shared__ double sh[kBatchThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = (int64_t)a.B * a.Q;
  const double n_need = count_need(a, sh, tid), n_zero = (double)n - n_need;
  double l_need = 0.0, l_zero = 0.0, hit = 0.0;
  for (int64_t i = tid; i < n; i += kBatchThreads) {
    const int32_t y = a.labels[(i / a.Q) * a.ld_lab + i % a.Q];
    const double l = (double)a.loss[i];
    if (y != 0) {
      l_need += l;
      hit += a.amax[i] == y ? 1.0 : 0.0;
    } else {
      l_zero += l;
    }
  }
  l_need = block_sum(l_need, sh, tid);
  l_zero = block_sum(l_zero, sh, tid);
  hit = block_sum(hit, sh, tid);
  const double need_loss = l_need / (n_need + 1e-6), zero_loss = l_zero / (n_zero + 1e-6);
  if (tid == 0) {
    *a.acc = (float)(hit / (n_need + 1e-6));
    *a.mean = (float)((l_need + l_zero) / (double)n);
  }
  for (int b = wave; b < a.B; b += kBatchThreads / 64) {
    double r = 0.0;
    for (int t = lane; t < a.Q; t += 64) r += (double)a.loss[(int64_t)b * a.Q + t];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) r += __shfl_xor(r, off);
    if (lane == 0) a.mask_loss[b] = (float)(r / a.Q + need_loss + zero_loss);
  }
}

}  // namespace

void launch_xent_rows(const XentRowsArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)a.B * a.Q));
  if (a.V <= kXentResidentV) hipLaunchKernelGGL(xent_rows_kernel<true>, grid, dim3(kXentThreads), 0, s, a);
  else hipLaunchKernelGGL(xent_rows_kernel<false>, grid, dim3(kXentThreads), 0, s, a);
}

void launch_xent_weights(const XentBatchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(xent_weights_kernel, dim3(1), dim3(kBatchThreads), 0, s, a);
}

void launch_xent_reduce(const XentBatchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(xent_reduce_kernel, dim3(1), dim3(kBatchThreads), 0, s, a);
}

}  // namespace mi355
