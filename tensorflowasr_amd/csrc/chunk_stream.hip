// Batched ChunkConformer streaming: the steps of one tick that are not row-wise.
//
// Every stream owns a SLOT of the caller's state buffer.  A tick brings n streams; stream i of the tick (slot slots[i]) owns
// rows i * TP .. i * TP + TP - 1 of every activation buffer, of which the first T[i] are real (TP = 4 for the encoder, the
// picker and the helper, win_back + 4 for the text decoder).  The row-wise layers run over all n * TP rows with the library's
// kernels; the kernels here read and write the per-stream state:
//   cs_front_window_kernel  [wav cache ; packet] -> the samples the last chunk_num mel frames need, wav cache update
//   cs_sub_kernel           [sub cache ; mel] for the two VALID convs, sub cache update
//   cs_attn_kernel          band attention of the T[i] new rows over [cached K / V ; new K / V], K / V appended to the cache
//   cs_dwconv_kernel        causal depthwise conv of the T[i] new rows over [cached GLU rows ; new], cache append, counters
//   cs_pick_kernel          phone arg-max -> picked rows, compacted, and the row counts of the helper and the decoder
//   cs_carry_kernel         text decoder input = [rows waiting for right context ; helper output], the new waiting rows
//   cs_reset_kernel         a slot becomes a fresh stream
// The caches hold what the modules COMPUTE from the rows the reference caches (K and V instead of the attention module's input,
// the GLU output instead of the conv module's input): both are functions of one row, so nothing changes in the results and a
// tick projects T rows per block instead of cache + T.  Each cache is a ring: `pos` is where the next row goes, the last
// min(cnt, size) rows before it are the cache.  All predicates on T[i] are uniform per workgroup (one workgroup = one stream).
#include "common.h"
#include "launch.h"

namespace {

constexpr int CS_MAXKEYS = 64;      // keys of one stream and head: one per lane
constexpr int CS_CNT_CAP = 1 << 20; // the row counter saturates (only min(cnt, ring size) is ever used)

DEV int ring_at(int pos, int size, int back) {   // index of the row `back` rows before pos (1 <= back <= size)
  int r = pos - back;
  return r < 0 ? r + size : r;
}

__global__ __launch_bounds__(256) void cs_front_window_kernel(CsFrontArgs a) {
  extern __shared__ float cat[];                 // [2 * Wb]: the stream's cache followed by its packet
  const int i = blockIdx.x, tid = threadIdx.x;
  float* st = a.state + (size_t)a.slots[i] * a.slot_words;
  float* cache = st + a.wav_off;
  const int ns = a.n_samples ? a.n_samples[i] : a.Wb;
  const int Lw = a.Wb + ns;
  for (int j = tid; j < a.Wb; j += 256) cat[j] = cache[j];
  for (int j = tid; j < a.Wb; j += 256) cat[a.Wb + j] = j < ns ? a.packets[(size_t)i * a.Wb + j] : 0.f;
  __syncthreads();
  // valid-mode frames of the Lw-sample buffer: frame f covers samples f hop - (n_dft - 1) .. f hop; the last chunk_num of its
  // F = (Lw - 1) / hop + 1 frames start at sample `first` (negative: the left padding of a stream's first packets is zeros, and
  // so is a fresh stream's cache)
  const int F = (Lw - 1) / a.hop + 1;
  const int first = (F - 1) * a.hop - (a.Lwin - 1);
  float* win = a.window + (size_t)i * a.Lwin;
  for (int j = tid; j < a.Lwin; j += 256) {
    const int sidx = first + j;
    win[j] = (sidx >= 0 && sidx < Lw) ? cat[sidx] : 0.f;
  }
  for (int j = tid; j < a.Wb; j += 256) cache[j] = cat[ns + j];      // the last Wb samples of the buffer
}

__global__ __launch_bounds__(256) void cs_sub_kernel(CsSubArgs a) {
  const int i = blockIdx.x;
  float* cache = a.state + (size_t)a.slots[i] * a.slot_words + a.sub_off;
  const int nc = a.S * a.NM, nm = a.F * a.NM;
  const float* mel = a.mel + (size_t)i * nm;
  float* out = a.new_sub + (size_t)i * (nc + nm);
  for (int e = threadIdx.x; e < nc + nm; e += 256) {
    if (e < nc) {
      out[e] = cache[e];
      cache[e] = mel[nm - nc + e];               // the last S mel rows (the same thread read the element it replaces)
    } else {
      out[e] = mel[e - nc];
    }
  }
}

// one workgroup per stream, one wave per head (four heads: the launcher checks); T[i] is uniform per workgroup, so every barrier is
// reached by all four waves
template <int HS>
__global__ __launch_bounds__(256) void cs_attn_kernel(CsAttnArgs a) {
  __shared__ float vs[4][CS_MAXKEYS][HS];
  __shared__ float ps[4][CS_MAXKEYS];
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int T = min(a.T ? a.T[i] : a.TP, a.TP);
  const int D = a.H * HS;
  float* ctx = a.ctx + (size_t)i * a.TP * D;
  if (T <= 0) {
    for (int e = threadIdx.x; e < a.TP * D; e += 256) ctx[e] = 0.f;
    return;
  }
  float* st = a.state + (size_t)a.slots[i] * a.slot_words;
  const int* meta = reinterpret_cast<const int*>(st + a.meta_off);
  // (the clamps cost nothing and keep a state buffer that was never reset from sending an access out of its slot)
  const int Cm = min(max(meta[0], 0), a.wf), pos = min(max(meta[1], 0), a.wf - 1);
  const int N = Cm + T;
  const int A = min(max(a.A ? a.A[i] : T, 0), T);
  float* kring = st + a.k_off;
  float* vring = st + a.v_off;
  const float* qkv = a.qkv + (size_t)i * a.TP * 3 * D;
  {
    const int h = wave;
    // lane j holds key j of [cache ; new] and stages value row j
    float k[HS];
    const bool have = lane < N;
    {
      const float* kp;
      const float* vp;
      if (lane < Cm) {
        const int r = ring_at(pos, a.wf, Cm - lane);
        kp = kring + (size_t)r * D + h * HS;
        vp = vring + (size_t)r * D + h * HS;
      } else {
        const int t = have ? lane - Cm : 0;
        kp = qkv + (size_t)t * 3 * D + D + h * HS;
        vp = kp + D;
      }
#pragma unroll
      for (int c = 0; c < HS; c += 4) {
        const f32x4 kv = have ? ldg4(kp + c) : splat4(0.f);
        const f32x4 vv = have ? ldg4(vp + c) : splat4(0.f);
        k[c] = kv.x; k[c + 1] = kv.y; k[c + 2] = kv.z; k[c + 3] = kv.w;
        *reinterpret_cast<f32x4*>(&vs[wave][lane][c]) = vv;
      }
    }
    for (int t = 0; t < a.TP; ++t) {
      float* orow = ctx + (size_t)t * D + h * HS;
      if (t >= T) {                                        // padding row (uniform)
        if (lane < HS) orow[lane] = 0.f;
        continue;
      }
      const float* q = qkv + (size_t)t * 3 * D + h * HS;   // already scaled by 1 / sqrt(head size)
      float sdot = 0.f;
#pragma unroll
      for (int c = 0; c < HS; c += 4) {
        const f32x4 qv = ldg4(q + c);
        sdot += (qv.x * k[c] + qv.y * k[c + 1]) + (qv.z * k[c + 2] + qv.w * k[c + 3]);
      }
      // the band of query Cm + t among the N rows of this stream (chunk_conformer_blocks.py:158-176)
      const int iq = Cm + t;
      const int klo = min(max(iq - a.wf, 0), N - a.wb);
      const int khi = max(min(iq + a.wb, N), a.wb);
      const bool vis = have && lane >= klo && lane <= khi;
      float sc = vis ? sdot : -INFINITY;
      float mx = sc;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float p = vis ? __expf(sc - mx) : 0.f;          // the query's own key is always visible: mx is finite
      float sum = p;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
      __syncthreads();                                      // (the previous query's reads of ps are done; vs is staged)
      ps[wave][lane] = p;
      __syncthreads();
      if (lane < HS) {
        float acc = 0.f;
        for (int j = 0; j < N; ++j) acc += ps[wave][j] * vs[wave][j][lane];
        orow[lane] = acc / sum;
      }
    }
    // the first A new rows join the cache: this head's columns of the ring are read and written by this wave alone, and its reads
    // are in registers / LDS by now
    __syncthreads();
    if (lane >= Cm && lane < Cm + A) {
      const int r = (pos + (lane - Cm)) % a.wf;
      float* kp = kring + (size_t)r * D + h * HS;
      float* vp = vring + (size_t)r * D + h * HS;
#pragma unroll
      for (int c = 0; c < HS; c += 4) {
        f32x4 kv = {k[c], k[c + 1], k[c + 2], k[c + 3]};
        stg4(kp + c, kv);
        stg4(vp + c, *reinterpret_cast<const f32x4*>(&vs[wave][lane][c]));
      }
    }
  }
}

__global__ __launch_bounds__(256) void cs_dwconv_kernel(CsDwArgs a) {
  const int i = blockIdx.x;
  const int T = min(a.T ? a.T[i] : a.TP, a.TP);
  const int c4n = a.D / 4;
  float* y = a.y + (size_t)i * a.TP * a.D;
  if (T <= 0) {
    for (int e = threadIdx.x; e < a.TP * a.D; e += 256) y[e] = 0.f;
    return;
  }
  float* st = a.state + (size_t)a.slots[i] * a.slot_words;
  int* meta = reinterpret_cast<int*>(st + a.meta_off);
  const int cnt = max(meta[0], 0), posm = min(max(meta[1], 0), a.wf - 1), pos = min(max(meta[2], 0), a.K - 1);
  const int Cc = min(cnt, a.K);
  const int A = min(max(a.A ? a.A[i] : T, 0), T);
  float* ring = st + a.g_off;
  const float* u = a.u + (size_t)i * a.TP * a.D;
  for (int e = threadIdx.x; e < a.TP * c4n; e += 256) {
    const int t = e / c4n, c4 = (e - t * c4n) * 4;
    f32x4 acc = splat4(0.f);
    if (t < T) {
      // causal: tap j reads row t - (K - 1) + j of the new rows; negative rows are the cache, rows before the stream began are zeros
      for (int j = 0; j < a.K; ++j) {
        const int r = t - (a.K - 1) + j;
        if (r < -Cc) continue;
        const float* up = r < 0 ? ring + (size_t)ring_at(pos, a.K, -r) * a.D : u + (size_t)r * a.D;
        acc += ldg4(up + c4) * ldg4(a.wd + (size_t)j * a.D + c4);
      }
    }
    stg4(y + (size_t)t * a.D + c4, acc);
  }
  __syncthreads();                                         // every read of the ring and of the counters is done
  for (int e = threadIdx.x; e < A * c4n; e += 256) {
    const int t = e / c4n, c4 = (e - t * c4n) * 4;
    stg4(ring + (size_t)((pos + t) % a.K) * a.D + c4, ldg4(u + (size_t)t * a.D + c4));
  }
  if (threadIdx.x == 0) {                                  // this block's attention ran before: the block is done with the counters
    meta[0] = min(cnt + A, CS_CNT_CAP);
    meta[1] = (posm + A) % a.wf;
    meta[2] = (pos + A) % a.K;
  }
}

__global__ __launch_bounds__(256) void cs_pick_kernel(CsPickArgs a) {
  const int i = blockIdx.x;
  const float* st = a.state + (size_t)a.slots[i] * a.slot_words;
  const int carry = min(max(reinterpret_cast<const int*>(st + a.hdr_off)[0], 0), a.wb);
  int n = 0;
  int src[8];                                              // TP <= 8 (checked by the launcher)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    src[t] = -1;
    if (t < a.TP && a.amax[i * a.TP + t] != a.blank) {
      // (src[n] with n a run-time value would go to scratch: write by comparison)
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q == n) src[q] = t;
      ++n;
    }
  }
  const float* hid = a.hidden + (size_t)i * a.TP * a.D;
  float* out = a.picked + (size_t)i * a.TP * a.D;
  for (int e = threadIdx.x; e < a.TP * a.D; e += 256) {
    const int r = e / a.D, c = e - r * a.D;
    int sr = -1;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q == r) sr = src[q];
    out[e] = sr >= 0 ? hid[(size_t)sr * a.D + c] : 0.f;
  }
  if (threadIdx.x == 0) {
    const int td = n > 0 ? carry + n : 0;                  // nothing picked: helper and decoder leave the stream alone
    const int vd = max(td - a.wb, 0);
    a.Th[i] = n; a.Td[i] = td; a.Vd[i] = vd;
    if (a.n_picked) a.n_picked[i] = n;
    if (a.n_valid) a.n_valid[i] = vd;
    if (a.n_unvalid) a.n_unvalid[i] = td - vd;
  }
}

__global__ __launch_bounds__(256) void cs_carry_kernel(CsCarryArgs a) {
  extern __shared__ float rows[];                          // [TPd, D]
  const int i = blockIdx.x;
  const int Td = min(a.Td[i], a.TPd);
  float* out = a.dec_in + (size_t)i * a.TPd * a.D;
  if (Td <= 0) {
    for (int e = threadIdx.x; e < a.TPd * a.D; e += 256) out[e] = 0.f;
    return;
  }
  float* st = a.state + (size_t)a.slots[i] * a.slot_words;
  int* hdr = reinterpret_cast<int*>(st + a.hdr_off);
  float* keep = st + a.carry_off;
  const int carry = min(max(hdr[0], 0), Td);
  const int Vd = min(max(a.Vd[i], 0), Td);
  const float* helped = a.helped + (size_t)i * a.TP * a.D;
  for (int e = threadIdx.x; e < a.TPd * a.D; e += 256) {
    const int r = e / a.D, c = e - r * a.D;
    const float v = r < carry ? keep[e] : (r < Td ? helped[(size_t)(r - carry) * a.D + c] : 0.f);
    rows[e] = v;
    out[e] = v;
  }
  __syncthreads();
  const int left = Td - Vd;                                // min(Td, win_back) rows wait for their right context
  for (int e = threadIdx.x; e < left * a.D; e += 256) keep[e] = rows[Vd * a.D + e];
  if (threadIdx.x == 0) hdr[0] = left;
}

__global__ __launch_bounds__(256) void cs_reset_kernel(CsResetArgs a) {
  const int slot = a.slots ? a.slots[blockIdx.x] : (int)blockIdx.x;
  float* st = a.state + (size_t)slot * a.slot_words;
  for (int e = threadIdx.x; e < a.zero_words; e += 256) st[e] = 0.f;   // wav cache, sub cache, counters (the rings are never read past their counters)
}

}  // namespace

int launch_cs_front_window(const CsFrontArgs& a, hipStream_t s) {
  const size_t lds = (size_t)2 * a.Wb * sizeof(float);
  if (a.n < 1 || lds > 64 * 1024 || a.Lwin < 1) return -1;
  hipLaunchKernelGGL(cs_front_window_kernel, dim3(a.n), dim3(256), lds, s, a);
  return 0;
}
int launch_cs_sub(const CsSubArgs& a, hipStream_t s) {
  if (a.n < 1 || a.S > a.F) return -1;
  hipLaunchKernelGGL(cs_sub_kernel, dim3(a.n), dim3(256), 0, s, a);
  return 0;
}
int launch_cs_attn(int HS, const CsAttnArgs& a, hipStream_t s) {
  if (HS != 36 || a.H != 4 || a.n < 1 || a.wf + a.TP > CS_MAXKEYS || a.wf < a.TP || a.TP < 1) return -1;
  hipLaunchKernelGGL(cs_attn_kernel<36>, dim3(a.n), dim3(256), 0, s, a);
  return 0;
}
int launch_cs_dwconv(const CsDwArgs& a, hipStream_t s) {
  if (a.n < 1 || a.D % 4 || a.K < a.TP) return -1;
  hipLaunchKernelGGL(cs_dwconv_kernel, dim3(a.n), dim3(256), 0, s, a);
  return 0;
}
int launch_cs_pick(const CsPickArgs& a, hipStream_t s) {
  if (a.n < 1 || a.TP > 8) return -1;
  hipLaunchKernelGGL(cs_pick_kernel, dim3(a.n), dim3(256), 0, s, a);
  return 0;
}
int launch_cs_carry(const CsCarryArgs& a, hipStream_t s) {
  const size_t lds = (size_t)a.TPd * a.D * sizeof(float);
  if (a.n < 1 || lds > 64 * 1024) return -1;
  hipLaunchKernelGGL(cs_carry_kernel, dim3(a.n), dim3(256), lds, s, a);
  return 0;
}
int launch_cs_reset(const CsResetArgs& a, hipStream_t s) {
  if (a.n < 1) return -1;
  hipLaunchKernelGGL(cs_reset_kernel, dim3(a.n), dim3(256), 0, s, a);
  return 0;
}
