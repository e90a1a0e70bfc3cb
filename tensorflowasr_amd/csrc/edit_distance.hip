// Ragged edit distance with the (S, D, I) split of utils/xer.py:12-35 behind mi355asr_edit_distance of include/mi355asr.h: for
// each row b the distance of hyp[b, :m_b] against ref[b, :n_b] and the substitution / deletion / insertion counts of the ONE
// optimal alignment the reference's recursion carries:
//     sub = prev[y-1] + (u != v),  del = prev[y] + 1,  ins = curr[y-1] + 1,  best = min(sub, del, ins)
//     take the substitution predecessor if best == sub, else the deletion predecessor if best == del, else the insertion one;
//     row 0 is all insertions, column 0 all deletions.
// Only a mismatching substitution costs 1, so cost == S + D + I in every cell and a cell is one packed 64-bit word in two
// registers: hi = cost << 16 | S, lo = D << 16 | I (every count <= kMaxLen = 16 384 < 2^16, no carry between fields).  A step is
// three adds per candidate at most, three shifts, one v_min3, two compares and the selects.
//
// edit_kernel: one workgroup per pair; thread j owns hypothesis column y = strip * T + 1 + j (T = blockDim.x: kStrip for every
// pair with more than one strip) and walks it down the rows, skewed by its lane: at wave-local step tau lane l is at row
// x = tau - l, so the wave holds one anti-diagonal.  What a lane needs from its left neighbour -- cell (x, y-1), and one step
// later the same value as cell (x-1, y-1), and the reference token u[x-1] -- arrives by DPP wave_shr:1; lane 0 receives the
// boundary column instead (v_readlane of a register that holds 64 boundary rows).  Waves run in phases of 64 steps with one
// barrier per phase: wave w runs its block q = p - 2 w in phase p, two phases behind wave w - 1, whose lane 63 produced the rows
// of block q in its blocks q and q + 1 and left them in an LDS ring of 256 rows (reads of a phase touch rows 64q+1 .. 64q+64,
// writes of the same phase rows 64q+66 .. 64q+129: never the same slot).  The right-hand column of a strip goes to the
// workspace (two buffers, alternating) and is the boundary of wave 0 in the next strip; strip 0 computes its boundary (x
// deletions).  No workgroup waits for another, there are no atomics on global memory, and nothing depends on the batch: a row
// gives the same integers alone, in any batch, at any position, in every run.
//
// The prologue of the same kernel filters both rows into the workspace: the hypothesis is cut before the first `stop` id, then
// the ids of the drop sets are removed (order-preserving compaction: ballot + popcount inside a wave, wave totals through LDS).
// Entries at or past a row's given length are never read.
//
// OPS: every cell's choice (0 match, 1 substitution, 2 deletion, 3 insertion) is kept, 16 rows of a column per 32-bit word
// ([ceil(N / 16)][M] words per pair), and the thread that owns cell (n, m) walks it back after the last barrier; the alignment
// has n + I steps, so it is written from its end and comes out in forward order.
#include "model.h"

namespace {

constexpr int kStrip = 1024;              // columns per strip = threads of a full workgroup
constexpr int kMaxLen = 16384;            // tokens per side: counts fit 16 bits
constexpr int64_t kMaxAlignCells = (int64_t)1 << 24;
constexpr int kRing = 256;                // rows of the LDS boundary ring per wave (>= 129, a power of two)
constexpr int kWaves = kStrip / 64;

struct Cell { uint32_t hi, lo; };         // hi = cost << 16 | S, lo = D << 16 | I

struct DropSet { int32_t n; int32_t id[4]; };

struct EditArgs {
  const int32_t* ref;       // [B, N]
  const int32_t* hyp;       // [B, M]
  const int32_t* ref_len;   // [B] or null
  const int32_t* hyp_len;   // [B] or null
  int32_t N, M;
  DropSet drop_ref, drop_hyp;
  int32_t use_stop, stop;
  int32_t* out;             // [B, 4] distance, S, D, I
  int32_t* lens;            // [B, 2] filtered n, m
  uint8_t* ops;             // [B, N + M] or null
  int32_t* n_ops;           // [B]
  Cell* col;                // [B, 2, N + 1]
  uint32_t* dirs;           // [B, ceil(N / 16), M] (OPS)
  int32_t* uf;              // [B, N] filtered reference
  int32_t* vf;              // [B, M] filtered hypothesis
};

__device__ __forceinline__ uint32_t shr1(uint32_t lane0_value, uint32_t v) {
  // wave_shr:1 -- lane l receives v of lane l - 1; lane 0 has no source and keeps `lane0_value`
  return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0_value, (int)v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ bool dropped(int32_t t, const DropSet& d) {
  bool r = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) r |= (i < d.n) & (t == d.id[i]);
  return r;
}

// order-preserving removal of the drop set from src[0 .. len): -> kept count (the same in every thread)
__device__ int compact(const int32_t* src, int len, const DropSet& d, int32_t* dst, int* wsum) {
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
  int base = 0;
  for (int c = 0; c < len; c += T) {
    const int i = c + tid;
    int32_t t = 0;
    bool keep = false;
    if (i < len) { t = src[i]; keep = !dropped(t, d); }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wsum[w] = __popcll(mask);
    __syncthreads();
    int off = 0, tot = 0;
    for (int j = 0; j < nw; ++j) { const int s = wsum[j]; off += j < w ? s : 0; tot += s; }
    if (keep) dst[base + off + __popcll(mask & ((1ull << lane) - 1ull))] = t;
    base += tot;
    __syncthreads();
  }
  return base;
}

template <bool OPS>
__global__ __launch_bounds__(kStrip) void edit_kernel(EditArgs a) {
  __shared__ Cell ring[kWaves][kRing];
  __shared__ int wsum[kWaves];
  __shared__ int s_stop;
  const int b = blockIdx.x, T = blockDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int N = a.N, M = a.M;
  const int32_t* ref = a.ref + (size_t)b * N;
  const int32_t* hyp = a.hyp + (size_t)b * M;
  int32_t* uf = a.uf + (size_t)b * N;
  int32_t* vf = a.vf + (size_t)b * M;
  Cell* col = a.col + (size_t)b * 2 * (N + 1);

  // ---- filter --------------------------------------------------------------------------------------------------------------
  int n_in = a.ref_len ? a.ref_len[b] : N, m_in = a.hyp_len ? a.hyp_len[b] : M;
  n_in = n_in < 0 ? 0 : (n_in > N ? N : n_in);
  m_in = m_in < 0 ? 0 : (m_in > M ? M : m_in);
  if (a.use_stop) {
    if (tid == 0) s_stop = m_in;
    __syncthreads();
    for (int i = tid; i < m_in; i += T)
      if (hyp[i] == a.stop) atomicMin(&s_stop, i);      // LDS only: the smallest index, whatever the order
    __syncthreads();
    m_in = s_stop;
  }
  const int n = compact(ref, n_in, a.drop_ref, uf, wsum);
  const int m = compact(hyp, m_in, a.drop_hyp, vf, wsum);   // ends in a barrier: uf / vf are visible to the workgroup
  if (tid == 0) { a.lens[2 * b] = n; a.lens[2 * b + 1] = m; }
  if (n == 0 || m == 0) {
    if (tid == 0) {
      int32_t* o = a.out + 4 * (size_t)b;
      o[0] = n + m; o[1] = 0; o[2] = n; o[3] = m;
      if (OPS) {
        uint8_t* ops = a.ops + (size_t)b * ((size_t)N + M);
        for (int i = 0; i < n + m; ++i) ops[i] = n ? 2 : 3;
        a.n_ops[b] = n + m;
      }
    }
    return;
  }

  // ---- the table -----------------------------------------------------------------------------------------------------------
  uint32_t* dirs = OPS ? a.dirs + (size_t)b * ((size_t)((N + 15) >> 4) * M) : nullptr;
  const int NB = (n + 63 + 63) >> 6;                       // blocks of 64 steps: tau = 1 .. n + 63
  const int strips = (m + T - 1) / T;
  Cell out{0, 0};
  for (int s = 0; s < strips; ++s) {
    const int y0 = s * T, y = y0 + 1 + tid;
    const int width = m - y0 < T ? m - y0 : T;
    const int Wv = (width + 63) >> 6;
    const bool last_strip = s == strips - 1;
    const bool colok = y <= m;
    const int32_t v = colok ? vf[y - 1] : 0;
    const Cell* col_in = col + (size_t)(s & 1) * (N + 1);
    Cell* col_out = col + (size_t)((s + 1) & 1) * (N + 1);
    // row 0 is all insertions: cell (0, y) = (cost y, I y); the first `diag` of a lane is cell (0, y - 1)
    out = Cell{(uint32_t)y << 16, (uint32_t)y};
    Cell left{(uint32_t)(y - 1) << 16, (uint32_t)(y - 1)};
    uint32_t ucur = 0, acc = 0;
    const bool producer = w < Wv - 1 || (!last_strip && w == Wv - 1);   // someone reads this wave's last column
    const int P = NB + 2 * (Wv - 1);
    for (int p = 0; p < P; ++p) {
      const int q = p - 2 * w;
      if (w < Wv && q >= 0 && q < NB) {
        // this block's 64 boundary rows and reference tokens: lane l holds row 64 q + 1 + l
        const int xb = 64 * q + 1 + lane;
        Cell bnd;
        if (w > 0) bnd = ring[w][xb & (kRing - 1)];
        else if (s == 0) bnd = Cell{(uint32_t)xb << 16, (uint32_t)xb << 16};
        else bnd = xb <= n ? col_in[xb] : Cell{0, 0};
        const uint32_t ublk = xb <= n ? (uint32_t)uf[xb - 1] : 0u;
        Cell keep{0, 0};
        for (int k = 0; k < 64; ++k) {
          const int x = 64 * q + 1 + k - lane;
          const Cell diag = left;
          left.hi = shr1(__builtin_amdgcn_readlane(bnd.hi, k), out.hi);
          left.lo = shr1(__builtin_amdgcn_readlane(bnd.lo, k), out.lo);
          ucur = shr1(__builtin_amdgcn_readlane(ublk, k), ucur);
          const bool neq = ucur != (uint32_t)v;
          const uint32_t sub_hi = diag.hi + (neq ? 0x10001u : 0u);
          const uint32_t del_hi = out.hi + 0x10000u, del_lo = out.lo + 0x10000u;
          const uint32_t ins_hi = left.hi + 0x10000u, ins_lo = left.lo + 1u;
          const uint32_t cs = sub_hi >> 16, cd = del_hi >> 16, ci = ins_hi >> 16;
          const uint32_t best = min(cs, min(cd, ci));
          const bool take_sub = best == cs, take_del = best == cd;
          const uint32_t nhi = take_sub ? sub_hi : (take_del ? del_hi : ins_hi);
          const uint32_t nlo = take_sub ? diag.lo : (take_del ? del_lo : ins_lo);
          const bool active = colok && (unsigned)(x - 1) < (unsigned)n;
          out.hi = active ? nhi : out.hi;
          out.lo = active ? nlo : out.lo;
          if (OPS) {
            const uint32_t dir = take_sub ? (uint32_t)neq : (take_del ? 2u : 3u);
            const int r = (x - 1) & 15;
            if (active) {
              acc |= dir << (2 * r);
              if (r == 15 || x == n) { dirs[(size_t)((x - 1) >> 4) * M + (y - 1)] = acc; acc = 0; }
            }
          }
          if (producer) {                                  // lane 63 is at row 64 q + 1 + k - 63: lane k keeps it
            const uint32_t h = __builtin_amdgcn_readlane(out.hi, 63), l = __builtin_amdgcn_readlane(out.lo, 63);
            keep.hi = lane == k ? h : keep.hi;
            keep.lo = lane == k ? l : keep.lo;
          }
        }
        if (producer) {
          const int xk = 64 * q + lane - 62;
          if (xk >= 1 && xk <= n) {
            if (w < Wv - 1) ring[w + 1][xk & (kRing - 1)] = keep;
            else col_out[xk] = keep;
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- the result: the thread that owns column m of the last strip holds cell (n, m) -----------------------------------------
  if (tid != (m - 1) - (strips - 1) * T) return;
  const int32_t S = out.hi & 0xffff, D = out.lo >> 16, I = out.lo & 0xffff;
  int32_t* o = a.out + 4 * (size_t)b;
  o[0] = out.hi >> 16; o[1] = S; o[2] = D; o[3] = I;
  if (OPS) {
    uint8_t* ops = a.ops + (size_t)b * ((size_t)N + M);
    int x = n, y = m, pos = n + I - 1;
    while ((x > 0 || y > 0) && pos >= 0) {
      uint32_t d;
      if (x == 0) d = 3;
      else if (y == 0) d = 2;
      else d = (dirs[(size_t)((x - 1) >> 4) * M + (y - 1)] >> (2 * ((x - 1) & 15))) & 3u;
      ops[pos--] = (uint8_t)d;
      if (d != 3) --x;
      if (d != 2) --y;
    }
    a.n_ops[b] = n + I;
  }
}

struct EditLayout { size_t col, dirs, uf, vf, total; };

EditLayout layout_of(int B, int N, int M, bool want_ops) {
  EditLayout l;
  size_t off = 0;
  l.col = off; off += align256((size_t)B * 2 * ((size_t)N + 1) * sizeof(Cell));
  l.dirs = off; off += want_ops ? align256((size_t)B * (size_t)((N + 15) >> 4) * M * sizeof(uint32_t)) : 0;
  l.uf = off; off += align256((size_t)B * N * sizeof(int32_t));
  l.vf = off; off += align256((size_t)B * M * sizeof(int32_t));
  l.total = off;
  return l;
}

int check_shape(int32_t B, int32_t N, int32_t M, int32_t want_ops) {
  if (B < 1 || N < 1 || M < 1) return fail(MI355ASR_EINVAL, "edit distance: need B, max_ref, max_hyp >= 1 (got %d, %d, %d)", B, N, M);
  if (N > kMaxLen || M > kMaxLen)
    return fail(MI355ASR_EINVAL, "edit distance: rows of %d and %d tokens are longer than %d", N, M, kMaxLen);
  if (want_ops && (int64_t)N * M > kMaxAlignCells)
    return fail(MI355ASR_EINVAL, "edit distance: the alignment of %d x %d cells is kept for up to %lld cells per pair", N, M,
                (long long)kMaxAlignCells);
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_edit_distance_workspace_bytes(int32_t B, int32_t max_ref, int32_t max_hyp, int32_t want_ops, size_t* ws_bytes) {
  if (!ws_bytes) return fail(MI355ASR_EINVAL, "null pointer");
  if (int rc = check_shape(B, max_ref, max_hyp, want_ops)) return rc;
  *ws_bytes = layout_of(B, max_ref, max_hyp, want_ops != 0).total;
  return 0;
}

int mi355asr_edit_distance(const int32_t* ref_dev, const int32_t* ref_len_dev, const int32_t* hyp_dev, const int32_t* hyp_len_dev,
                           int32_t B, int32_t max_ref, int32_t max_hyp, const int32_t* drop_ref_host, int32_t n_drop_ref,
                           const int32_t* drop_hyp_host, int32_t n_drop_hyp, int32_t use_stop, int32_t hyp_stop, int32_t* out_dev,
                           int32_t* lens_dev, uint8_t* ops_dev, int32_t* n_ops_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  if (!ref_dev || !hyp_dev || !out_dev || !lens_dev || !ws_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if ((ops_dev == nullptr) != (n_ops_dev == nullptr)) return fail(MI355ASR_EINVAL, "edit distance: ops and n_ops go together");
  const bool want_ops = ops_dev != nullptr;
  if (int rc = check_shape(B, max_ref, max_hyp, want_ops)) return rc;
  if (n_drop_ref < 0 || n_drop_ref > 4 || n_drop_hyp < 0 || n_drop_hyp > 4)
    return fail(MI355ASR_EINVAL, "edit distance: a drop set holds 0 .. 4 ids (got %d and %d)", n_drop_ref, n_drop_hyp);
  if ((n_drop_ref && !drop_ref_host) || (n_drop_hyp && !drop_hyp_host)) return fail(MI355ASR_EINVAL, "null pointer");
  if ((uintptr_t)ws_dev & 7) return fail(MI355ASR_EINVAL, "edit distance: misaligned workspace");
  const EditLayout l = layout_of(B, max_ref, max_hyp, want_ops);
  if (ws_bytes < l.total) return fail(MI355ASR_EWORKSPACE, "edit distance: workspace too small: %zu < %zu bytes", ws_bytes, l.total);
  EditArgs a{};
  a.ref = ref_dev; a.hyp = hyp_dev; a.ref_len = ref_len_dev; a.hyp_len = hyp_len_dev;
  a.N = max_ref; a.M = max_hyp;
  a.drop_ref.n = n_drop_ref; a.drop_hyp.n = n_drop_hyp;
  for (int i = 0; i < n_drop_ref; ++i) a.drop_ref.id[i] = drop_ref_host[i];
  for (int i = 0; i < n_drop_hyp; ++i) a.drop_hyp.id[i] = drop_hyp_host[i];
  a.use_stop = use_stop != 0; a.stop = hyp_stop;
  a.out = out_dev; a.lens = lens_dev; a.ops = ops_dev; a.n_ops = n_ops_dev;
  char* ws = (char*)ws_dev;
  a.col = (Cell*)(ws + l.col); a.dirs = (uint32_t*)(ws + l.dirs); a.uf = (int32_t*)(ws + l.uf); a.vf = (int32_t*)(ws + l.vf);
  const int threads = std::min(kStrip, (max_hyp + 63) / 64 * 64);
  hipStream_t s = (hipStream_t)stream;
  if (want_ops) hipLaunchKernelGGL(edit_kernel<true>, dim3((unsigned)B), dim3(threads), 0, s, a);
  else hipLaunchKernelGGL(edit_kernel<false>, dim3((unsigned)B), dim3(threads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
