// Per-stream encoder histories of a streaming server, kept on the device (mi355asr_stream_append / mi355asr_stream_gather):
// N slots of up to Tcap rows of d floats each, hist [N, Tcap, d], with the rows in use hist_len [N].  A tick appends the
// chunk outputs of the streams that had a chunk due and gathers the histories of the streams that have a decode due into the
// dense [M, Tpad, d] batch the ragged CTC decoder and Translator take.  Plain copy kernels: 16-byte vector loads and stores,
// one launch each; everything that could go wrong (slot range, a slot twice, overflow) is checked on the host copies of the
// slots and lengths before anything is launched.
#include <vector>

#include "common.h"
#include "model.h"

namespace {

// one workgroup per appended slot: rows [hist_len[s], hist_len[s] + Tc) of slot s = chunk[m]; then hist_len[s] += Tc.  The
// slots of a launch are distinct (host check), so no other workgroup reads or writes this slot's length.
__global__ __launch_bounds__(256) void stream_append_kernel(const float* __restrict__ chunk, const int32_t* __restrict__ slot,
                                                            int Tc, int d, float* __restrict__ hist, int32_t* hist_len, int Tcap) {
  const int m = blockIdx.x, s = slot[m];
  const int off = hist_len[s];
  __syncthreads();                                        // every thread has read the length before thread 0 advances it
  if (off + Tc > Tcap) return;                            // (refused on the host; never write past the slot)
  const int n4 = Tc * d / 4;
  const f32x4* src = reinterpret_cast<const f32x4*>(chunk + (size_t)m * Tc * d);
  f32x4* dst = reinterpret_cast<f32x4*>(hist + ((size_t)s * Tcap + off) * d);
  for (int i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) hist_len[s] = off + Tc;
}

// workgroup (x, m): rows [8 x, 8 x + 8) of out[m]: the history of slot[m], behind it the optional tail piece, zeros after that
__global__ __launch_bounds__(256) void stream_gather_kernel(const float* __restrict__ hist, const int32_t* __restrict__ hist_len,
                                                            const int32_t* __restrict__ slot, int Tcap, int d,
                                                            const float* __restrict__ tail, const int32_t* __restrict__ tail_len,
                                                            int Tt, float* __restrict__ out, int32_t* __restrict__ out_len, int Tpad) {
  const int m = blockIdx.y, s = slot[m];
  const int hl = min(hist_len[s], Tcap);
  const int tl = tail && tail_len ? min(max(tail_len[m], 0), Tt) : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_len[m] = min(hl + tl, Tpad);
  const int d4 = d / 4;
  const f32x4* h4 = reinterpret_cast<const f32x4*>(hist + (size_t)s * Tcap * d);
  const f32x4* t4 = tail ? reinterpret_cast<const f32x4*>(tail + (size_t)m * Tt * d) : nullptr;
  f32x4* o4 = reinterpret_cast<f32x4*>(out + (size_t)m * Tpad * d);
  for (int i = threadIdx.x; i < 8 * d4; i += blockDim.x) {
    const int t = blockIdx.x * 8 + i / d4, c = i % d4;
    if (t >= Tpad) break;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t < hl) v = h4[(size_t)t * d4 + c];
    else if (t < hl + tl) v = t4[(size_t)(t - hl) * d4 + c];
    o4[(size_t)t * d4 + c] = v;
  }
}

int check_slots(const int32_t* slot_host, int M, int N) {
  std::vector<char> seen((size_t)N, 0);
  for (int i = 0; i < M; ++i) {
    const int s = slot_host[i];
    if (s < 0 || s >= N) return fail(MI355ASR_EINVAL, "slot[%d] = %d lies outside [0, %d)", i, s, N);
    if (seen[s]) return fail(MI355ASR_EINVAL, "slot %d appears twice", s);
    seen[s] = 1;
  }
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_stream_append(const float* chunk_dev, const int32_t* slot_dev, const int32_t* slot_host, int32_t M, int32_t Tc,
                           int32_t d, float* hist_dev, int32_t* hist_len_dev, int32_t* hist_len_host, int32_t N, int32_t Tcap,
                           void* stream) {
  if (!chunk_dev || !slot_dev || !slot_host || !hist_dev || !hist_len_dev || !hist_len_host) return fail(MI355ASR_EINVAL, "null argument");
  if (M < 1 || Tc < 1 || N < 1 || Tcap < 1 || d < 4 || d % 4 != 0)
    return fail(MI355ASR_EINVAL, "stream_append: need M, Tc, N, Tcap >= 1 and d a multiple of 4 (got %d, %d, %d, %d, %d)", M, Tc, N, Tcap, d);
  if (int rc = check_slots(slot_host, M, N)) return rc;
  for (int i = 0; i < M; ++i) {
    const int s = slot_host[i];
    if (hist_len_host[s] < 0 || hist_len_host[s] + Tc > Tcap)
      return fail(MI355ASR_EINVAL, "stream_append: slot %d holds %d rows, %d more would overflow its %d", s, hist_len_host[s], Tc, Tcap);
  }
  hipLaunchKernelGGL(stream_append_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, chunk_dev, slot_dev, Tc, d, hist_dev, hist_len_dev, Tcap);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch stream append: %s", hipGetErrorString(e));
  for (int i = 0; i < M; ++i) hist_len_host[slot_host[i]] += Tc;
  return 0;
}

int mi355asr_stream_gather(const float* hist_dev, const int32_t* hist_len_dev, const int32_t* hist_len_host, int32_t N, int32_t Tcap,
                           int32_t d, const int32_t* slot_dev, const int32_t* slot_host, int32_t M, const float* tail_dev,
                           const int32_t* tail_len_dev, const int32_t* tail_len_host, int32_t Tc_tail, float* out_dev,
                           int32_t* out_len_dev, int32_t Tpad, void* stream) {
  if (!hist_dev || !hist_len_dev || !hist_len_host || !slot_dev || !slot_host || !out_dev || !out_len_dev) return fail(MI355ASR_EINVAL, "null argument");
  if (M < 1 || N < 1 || Tcap < 1 || Tpad < 1 || d < 4 || d % 4 != 0)
    return fail(MI355ASR_EINVAL, "stream_gather: need M, N, Tcap, Tpad >= 1 and d a multiple of 4 (got %d, %d, %d, %d, %d)", M, N, Tcap, Tpad, d);
  if ((tail_dev != nullptr) != (tail_len_dev != nullptr) || (tail_dev != nullptr) != (tail_len_host != nullptr) || (tail_dev && Tc_tail < 1))
    return fail(MI355ASR_EINVAL, "stream_gather: tail pieces come with their device and host lengths and Tc_tail >= 1");
  if (int rc = check_slots(slot_host, M, N)) return rc;
  for (int i = 0; i < M; ++i) {
    const int tl = tail_len_host ? tail_len_host[i] : 0, hl = hist_len_host[slot_host[i]];
    if (tl < 0 || tl > Tc_tail) return fail(MI355ASR_EINVAL, "stream_gather: tail_len[%d] = %d lies outside [0, %d]", i, tl, Tc_tail);
    if (hl < 0 || hl > Tcap) return fail(MI355ASR_EINVAL, "stream_gather: slot %d holds %d rows of %d", slot_host[i], hl, Tcap);
    if (hl + tl < 1) return fail(MI355ASR_EINVAL, "stream_gather: slot %d has nothing to decode", slot_host[i]);
    if (hl + tl > Tpad) return fail(MI355ASR_EINVAL, "stream_gather: slot %d needs %d rows, Tpad = %d", slot_host[i], hl + tl, Tpad);
  }
  hipLaunchKernelGGL(stream_gather_kernel, dim3((Tpad + 7) / 8, M), dim3(256), 0, (hipStream_t)stream, hist_dev, hist_len_dev, slot_dev,
                     Tcap, d, tail_dev, tail_len_dev, Tc_tail, out_dev, out_len_dev, Tpad);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch stream gather: %s", hipGetErrorString(e));
  return 0;
}

}  // extern "C"
