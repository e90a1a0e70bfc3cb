// ChunkConformer host side (chunk_conformer_blocks.py): offline predict and the streaming entry points with explicit
// caches, behind the mi355asr_chunk_* functions of include/mi355asr.h.
#include "model.h"

namespace {


struct ChunkGeom { int F, T1, T; };

int chunk_geometry(const mi355asr_model* m, int B, int L, ChunkGeom* g) {
  if (B <= 0 || L <= 0) return fail(MI355ASR_EINVAL, "B and L must be positive (B=%d, L=%d)", B, L);
  // 'valid' Spectrogram: the reference left-pads n_dft-1 zeros, then a VALID strided conv (time_frequency.py:106-107)
  g->F = (L - 1) / m->dm.hop + 1;
  // ConvSubsampling(padding='valid'): pad 4 frames in front, VALID 3x3 stride 2, twice (chunk_conformer_blocks.py:60-66)
  g->T1 = (g->F + 4 - 3) / 2 + 1;
  g->T = (g->T1 - 3) / 2 + 1;
  if (g->T < 1) return fail(MI355ASR_EINVAL, "L=%d is too short for the chunk front end", L);
  return 0;
}

struct ChunkPlan : ScratchPlan {
  size_t hid, amax, idx, cnt, logp, pmax, mel, sub, total;
};

ChunkPlan make_chunk_plan(const mi355asr_model* m, int B, int F, int T) {
  const int d = m->cfg.dmodel;
  const size_t M = (size_t)B * T;
  ChunkPlan p;
  Layout lay;
  auto take = [&](size_t floats) { return lay.take(floats); };
  lay.scratch(p, M, d);
  p.hid = take(M * d);
  p.amax = take(M); p.idx = take(M); p.cnt = take(B);
  const int FT = ceil_div(F, 16);
  p.logp = take((size_t)B * F * m->dm.LP);
  p.pmax = take((size_t)B * std::max(FT * m->dm.NCH_dft, F));
  p.mel = take((size_t)B * F * m->cfg.n_mels);
  p.sub = take(M * m->dm.F2 * d);
  // the stacks behind feature_pick run on B * Tp <= M rows: with few picks they take the layer-at-a-time launches (up to
  // MI355ASR_SMALL_M rows), which need the FFN hidden buffer, whatever M is -- without it h4 would alias xa
  const size_t layer_rows = gemm16_for(m, M) ? M : std::min(M, (size_t)std::max(block_switches().small_m, 0L));
  p.h4 = layer_rows ? take(layer_rows * 4 * d) : 0;
  p.total = lay.o;
  return p;
}

// Dense(d->d) [+ blocks] [+ Dense(d->V) with argmax]; input rows at `in`, blocks run in sc.xa
// On return the stack's hidden output is in sc.xa (sc is updated: the blocks ping-pong xa/xb).
// `front` (round 4): a plain layer the caller left to this stack's first block (the chunk front's subsampling Dense: BlockOpts::pre_*
// of the stack's options filled in; `in` is not read then).  A stack's own projection takes the same route when it can.
// len / len_host (ragged batches): the rows of each utterance, on the device and on the host (BlockOpts::t_len of every block)
int run_stack(const mi355asr_model* m, const StackDev& st, const float* in, int B, int T, Scratch& sc,
              float* logits, int32_t* amax, hipStream_t s, const BlockOpts* front = nullptr, const int32_t* len = nullptr,
              const int32_t* len_host = nullptr) {
  const int d = m->cfg.dmodel;
  const int M = B * T;
  BlockOpts first = front ? *front : st.opts;
  BlockOpts rest = st.opts;
  first.t_len = rest.t_len = len;
  first.t_len_host = rest.t_len_host = len_host;
  if (!front && st.proj_wp && st.proj_pp && !st.blocks.empty() && block_takes_pre(m, st.blocks[0], (size_t)M)) {
    first.pre_x = in; first.pre_pp = st.proj_pp; first.pre_sw = st.proj_pp_sw; first.pre_chunks = 1;
  }
  if (first.pre_pp) {
    // (nothing here: the first block below computes the layer in front of it)
  } else if (st.proj_wp) {
    // on its own: the same two-term stream through pp_sublinear_kernel (bit-identical to the folded form), else fp32 MFMA
    if (int rc = run_rows_project(m, st, in, sc.xa, M, s, st.proj_pp && m->cfg.gemm_dtype == 0 && !gemm16_for(m, (size_t)M))) return rc;
  } else if (in != sc.xa) {
    HIP_TRY(hipMemcpyAsync(sc.xa, in, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
  }
  bool ff1_done = false;                    // the tail of block i also runs ff_module_1 + qkv of block i + 1 (model.h)
  for (size_t i = 0; i < st.blocks.size(); ++i) {
    const bool skip = ff1_done;
    int rc = run_block(m, st.blocks[i], i == 0 ? first : rest, sc, B, T, nullptr, s, nullptr,
                       i + 1 < st.blocks.size() ? &st.blocks[i + 1] : nullptr, &ff1_done, skip);
    if (rc) return rc;
  }
  if (st.fc_wp && (logits || amax)) {
    const GemmArgs hd = head_args(st, sc.xa, M, logits, amax);
    // (the q / k / v and context buffers are dead behind the last block: the per-range arg-max pairs of a head split over class
    // ranges, and the arg-max nobody asked for)
    if (int rc = run_class_head(m, hd, HeadLayers::never, sc.qkv, nullptr, reinterpret_cast<int32_t*>(sc.ctx), s)) return rc;
  }
  return 0;
}


// The "valid" Melspectrogram (chunk front): the reference left-pads n_dft - 1 zeros, then a VALID strided conv; log10 only, no
// max-normalisation (chunk_amplitude_to_decibel, backend_keras.py:25-37).  absmax: B words that receive each utterance's largest
// |mel| when the banded mel kernel runs; set to null when it did not (the dense kernel does not produce it).
// pad_left: zeros in front of the first frame (default: the layer's n_dft - 1; the batched streams frame a window they cut themselves)
int run_valid_mel(const mi355asr_model* m, const float* wav, int B, int L, int F, float* logp, float* pmax, float* mel,
                  unsigned** absmax, hipStream_t s, int pad_left = -1, const int32_t* f_len = nullptr) {
  const auto& c = m->cfg;
  if (pad_left < 0) pad_left = c.n_dft - 1;
  const int FT = ceil_div(F, 16);
  if (m->fft_ok) {
    FftStftArgs fa{wav, logp, pmax, m->fft_w1p, m->fft_w2p, m->fft_twc, m->fft_tws, m->fft_win,
                   B, L, F, m->dm.hop, pad_left, m->dm.LP, 0};
    fa.w1s = m->fft_w1s; fa.w2s = m->fft_w2s; fa.w1h = m->fft_w1h; fa.w2h = m->fft_w2h;
    PROF(MI355ASR_K_STFT);
    LAUNCH_TRY(launch_fft_stft(fa, s), "stft (valid, fft)");
  } else {
    StftArgs st{};
    st.wav = wav; st.logp = logp; st.pmax = pmax; st.wp = m->dft_wp;
    st.B = B; st.L = L; st.F = F; st.hop = m->dm.hop; st.pad_left = pad_left; st.n_dft = c.n_dft;
    st.NT = m->dm.NT_dft; st.LP = m->dm.LP; st.nbins = m->dm.nbins; st.FT = FT; st.NCH = m->dm.NCH_dft;
    st.db10 = 0;
    PROF(MI355ASR_K_STFT);
    LAUNCH_TRY(launch_stft(st, s), "stft (valid)");
  }
  MelArgs me{};
  me.logp = logp; me.umax = nullptr; me.mel = mel; me.wp = m->mel_wp;
  me.B = B; me.F = F; me.LP = m->dm.LP; me.nbins = m->dm.nbins; me.KBm = m->dm.KBm; me.NTm = m->dm.NTm;
  me.NM = c.n_mels; me.FT = FT; me.floor_db = 0.f;
  me.f_len = f_len;                 // ragged batches: the utterance's largest |mel| over its own frames
  if (absmax && *absmax) { HIP_TRY(hipMemsetAsync(*absmax, 0, sizeof(unsigned) * (size_t)B, s)); me.absmax = *absmax; }
  { PROF(MI355ASR_K_MEL); LAUNCH_TRY(launch_mel_auto(m, me, s), "mel (valid)"); }
  if (absmax) *absmax = me.absmax;
  return 0;
}

}  // namespace

namespace mi355 {

int finalize_chunk(mi355asr_model* m, hipStream_t s) {
  const auto& cc = m->ccfg;
  ArenaBuilder ab;
  ab.ring_terms = m->cfg.gemm_dtype == 1 ? 1 : 3;
  // round 3: the front runs the split-bf16 subsampling kernels of the offline encoder (the explicit front padding and the
  // VALID geometry are index offsets of the same kernels: subconv.hip reads pt1 / pf1 / pt2 / pf2 / T1 / F1 from its arguments);
  // round 4: and their two-term fp16 forms, conv2's operand scale coming from each utterance's largest |mel| at run time
  const FrontOff fo = pack_front(m, ab, "front/", kNoMelBound);
  const StackOff e = pack_stack(m, ab, "encoder/", "chunk_conformer_block_", cc.enc_num_blocks, false, 0, true);
  const StackOff pk = pack_stack(m, ab, "picker/", "block_", cc.picker_num_blocks, true, cc.picker_num_classes, true);
  const StackOff hp = pack_stack(m, ab, "helper/", "block_", cc.helper_num_blocks, false, 0, true);
  const StackOff dc = pack_stack(m, ab, "decoder/", "block_", cc.decoder_num_blocks, true, cc.decoder_num_classes, true);
  if (int rc = upload_arena(m, ab, s)) return rc;
  const float* base = m->arena;
  resolve_front(m, fo, base);
  resolve_stack(m->c_enc, e, base);
  resolve_stack(m->c_picker, pk, base);
  resolve_stack(m->c_helper, hp, base);
  resolve_stack(m->c_decoder, dc, base);
  m->finalized = true;
  return 0;
}

}  // namespace mi355

namespace {
// =======================================================================================================
// ChunkConformer streaming (single stream, explicit caches; chunk_conformer_blocks.py:72-91, 206-220, 294-310,
// 381-388, 447-458, 530-560, 641-672, 750-770).  The caller owns the caches and trims them (valid / window
// slicing is plain indexing, done in tensorflowasr_amd/models.py as the reference does it in Python).
// =======================================================================================================
struct StreamPlan : ScratchPlan {
  size_t amax, logp, pmax, mel, sub, total;
};
// N = longest [cache ; new] row count of any module, F = mel frames of the wav buffer, Fs = rows of [sub cache ; mel]
StreamPlan make_stream_plan(const mi355asr_model* m, int N, int F, int Fs) {
  const size_t d = m->cfg.dmodel;
  StreamPlan p;
  Layout lay;
  auto take = [&](size_t floats) { return lay.take(floats); };
  lay.scratch(p, N, d);
  p.amax = take(N);
  const int FT = ceil_div(std::max(F, 1), 16);
  p.logp = take((size_t)std::max(F, 1) * m->dm.LP);
  p.pmax = take((size_t)std::max(FT * m->dm.NCH_dft, F));
  p.mel = take((size_t)std::max(F, 1) * m->cfg.n_mels);
  p.sub = take((size_t)std::max(Fs, 1) * m->dm.F2 * d);
  p.total = lay.o;
  return p;
}

// ChunkConformerBlock.stream_call (:381-388) for one stream: x (T rows) in sc.xa -> result in sc.xa, on walk_block_rows (model.h).
// new_mha [Cm+T, d] / new_cnn [Cc+T, d] receive [cache ; module input] (untrimmed).
int run_block_stream(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, Scratch& sc, int T,
                     const float* mha_cache, int Cm, const float* cnn_cache, int Cc, float* new_mha, float* new_cnn,
                     hipStream_t s) {
  const int d = m->cfg.dmodel;
  const size_t row = (size_t)d * 4;
  // [cache ; rows]: what the two layers in front of the token-mixing steps read
  auto concat = [&](float* cat, const float* cache, int C, const float* rows) -> int {
    if (C > 0) HIP_TRY(hipMemcpyAsync(cat, cache, C * row, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(cat + (size_t)C * d, rows, T * row, hipMemcpyDeviceToDevice, s));
    return 0;
  };
  // new_mha = [cache ; xb]; q/k/v of every row of it (the queries are its last T rows, :209-214)
  auto qkv_rows = [&](RowsOf& r) -> int { r = RowsOf{new_mha, Cm + T}; return concat(new_mha, mha_cache, Cm, sc.xb); };
  auto attend = [&]() -> int {
    AttnArgs at = self_attn_args(m, bo, sc.qkv, sc.ctx, 1, T);
    at.q = sc.qkv + (size_t)Cm * 3 * d; at.Tk = Cm + T; at.q_off = Cm;
    PROF(MI355ASR_K_ATTN); LAUNCH_TRY(launch_attention(m->cfg.head_size, at, s), "attention");
    return 0;
  };
  // new_cnn = [cache ; xa]; the conv module runs over all of it, its last T rows are kept (:297-306)
  auto glu_rows = [&](RowsOf& r) -> int { r = RowsOf{new_cnn, Cc + T}; return concat(new_cnn, cnn_cache, Cc, sc.xa); };
  auto depthwise = [&]() -> int {
    PROF(MI355ASR_K_DWCONV); LAUNCH_TRY(launch_dwconv(bo.ksz, dw_args(m, w, bo, sc.u, sc.dw, 1, Cc + T), s), "depthwise conv");
    return 0;
  };
  return walk_block_rows(m, w, bo, sc, T, nullptr, s, qkv_rows, attend, glu_rows, depthwise, (size_t)Cc);
}

// mel frames of a wav buffer / rows after the two VALID stride-2 convs over [sub cache ; last chunk_num mel frames]
void front_stream_shape(const mi355asr_model* m, int Lw, int S, int chunk_num, int* F, int* nf, int* T1, int* T2, int* Tout) {
  *F = (Lw - 1) / m->dm.hop + 1;
  *nf = std::min(*F, chunk_num);
  const int rows = S + *nf;
  *T1 = rows >= 3 ? (rows - 3) / 2 + 1 : 0;
  *T2 = *T1 >= 3 ? (*T1 - 3) / 2 + 1 : 0;
  *Tout = std::min(*T2, chunk_num / m->cfg.reduction_factor);
}

const StackDev* chunk_stack_by_id(const mi355asr_model* m, int id) {
  switch (id) {
    case 0: return &m->c_enc;
    case 1: return &m->c_picker;
    case 2: return &m->c_helper;
    case 3: return &m->c_decoder;
  }
  return nullptr;
}

// the ragged call's workspace: the plan's, then the mel frames and the encoder frames of every utterance (B words each)
size_t chunk_ragged_total(const ChunkPlan& p, int B) { return p.total + 2 * align256((size_t)B * 4); }

// One body for mi355asr_chunk_predict and its ragged form.  ragged: wav_len [B] on the device, utterance b
// being wav[b, :wav_len[b]]; every output row of it equals the call on that utterance alone.  The front, the causal conv and
// every row-wise layer never read past a row's own frames, so the lengths reach four places only: the utterance maximum of the
// mel kernel, the band attention (BlockOpts::t_len: T_b for encoder and picker, the pick counts for helper and decoder),
// feature_pick, and the rows past a length in the outputs.
int chunk_predict(mi355asr_model* m, const float* wav, bool ragged, const int32_t* wav_len, int32_t B, int32_t L,
                  const mi355asr_chunk_outputs* outs, int32_t* n_picked, int32_t* t_pick, void* ws_, size_t ws_bytes, void* stream) {
  if (!m || !m->is_chunk) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (!wav || !outs || !n_picked || !t_pick || !ws_) return fail(MI355ASR_EINVAL, "null argument");
  if (ragged && !wav_len) return fail(MI355ASR_EINVAL, "wav_len: null device pointer");
  // (the block kernels that apply lengths: run_block refuses the others, but only once the front has been launched)
  if (ragged && (m->cfg.gemm_dtype != 0 || use_gemm16(m) || !block_switches().fused))
    return fail(MI355ASR_EINVAL, "ragged ChunkConformer batches: gemm_dtype bf16 / the layer-at-a-time GEMM mode (MI355ASR_GEMM16) / "
                "MI355ASR_FUSED=0: only the fp32 dmodel-144 block kernels apply lengths");
  ChunkGeom g;
  int rc = chunk_geometry(m, B, L, &g);
  if (rc) return rc;
  const ChunkPlan p = make_chunk_plan(m, B, g.F, g.T);
  const size_t need = ragged ? chunk_ragged_total(p, B) : p.total;
  if (ws_bytes < need) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  char* ws = (char*)ws_;
  hipStream_t s = (hipStream_t)stream;
  // ragged: the lengths are device words: read once (this synchronises the stream), held to [2 hop + 1, L] -- at least one encoder frame
  std::vector<int32_t> t_host;
  int32_t *f_len = nullptr, *t_len = nullptr;
  if (ragged) {
    std::vector<int32_t> wl((size_t)B, 0);
    HIP_TRY(hipMemcpyAsync(wl.data(), wav_len, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int lo = 2 * m->dm.hop + 1;
    t_host.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
      if (wl[b] < lo || wl[b] > L) return fail(MI355ASR_EINVAL, "wav_len[%d] = %d lies outside [%d, %d]", b, wl[b], lo, L);
      ChunkGeom gb;
      if ((rc = chunk_geometry(m, 1, wl[b], &gb))) return rc;
      t_host[b] = gb.T;
    }
    f_len = (int32_t*)(ws + p.total);
    t_len = (int32_t*)(ws + p.total + align256((size_t)B * 4));
    LAUNCH_TRY(launch_chunk_ragged_frames(wav_len, B, m->dm.hop, f_len, t_len, s), "ragged frame counts");
  }
  const int32_t* t_len_host = ragged ? t_host.data() : nullptr;
  // rows past an utterance's length get defined values: 0, and -1 for ids
  auto pad_rows = [&](const int32_t* len, int rows, float* x, int n, int32_t* ids) -> int {
    if (len && (x || ids)) LAUNCH_TRY(launch_ragged_rows(len, B, rows, x, n, n, ids, s), "ragged ChunkConformer rows");
    return 0;
  };
  const auto& c = m->cfg;
  const int d = c.dmodel, T = g.T;
  const size_t act = (size_t)B * T * d * 4;
  Scratch sc = make_scratch(p, ws);
  BlockOpts enc_front;
  bool dense_deferred = false;
  // ---- front: valid Melspectrogram + left-padded VALID ConvSubsampling
  {
    float* mel = (float*)(ws + p.mel);
    // round 4: the valid frontend's log10 features have no static bound; the banded mel kernel leaves each utterance's largest
    // |mel| in the first B words of the (by now consumed) per-frame maxima, and the two-term subsampling conv scales by it
    // (round 5: per utterance, not per batch -- a quiet utterance next to a loud one keeps its own 2^-22, and B = 1 == B = N)
    unsigned* melmax = (m->mel_band && m->c2_whalf && m->c1_l1 > 0.f) ? (unsigned*)(ws + p.pmax) : nullptr;
    if ((rc = run_valid_mel(m, wav, B, L, g.F, (float*)(ws + p.logp), (float*)(ws + p.pmax), mel, &melmax, s, -1, f_len))) return rc;
    SubConvArgs sa{};
    sa.mel = mel; sa.out = (float*)(ws + p.sub);
    subconv_weights(m, sa, true);
    static const bool three = mi355_env("MI355ASR_SUBCONV_TERMS", -1) == 3;
    if (melmax && !three) { sa.w2h = m->c2_whalf; sa.h_wscale = m->c2_wscale; sa.h_melmax = melmax; sa.h_l1 = m->c1_l1; sa.h_bmax = m->c1_bmax; sa.c1_wscale = m->c1_wscale; }
    sa.B = B; sa.F = g.F; sa.NM = c.n_mels; sa.T1 = g.T1; sa.F1 = m->dm.F1; sa.T2 = T; sa.F2 = m->dm.F2;
    sa.st1 = 2; sa.pt1 = 4; sa.pf1 = 2; sa.pt2 = 0; sa.pf2 = 0;
    { PROF(MI355ASR_K_SUBCONV); LAUNCH_TRY(launch_subconv(d, sa, s), "conv subsampling (valid)"); }
    const StreamGemmArgs lg = sublinear_args(m, sa.out, sc.xa, B * T);
    // round 4: the Dense rides in the encoder's first ff_module_1 + qkv launch when both run on the two-term stream and
    // nobody asked for the front's output (as encoder_impl in api.hip)
    if (!outs->front_out && !m->c_enc.proj_wp && !m->c_enc.blocks.empty() && m->lin_wsplit && lg.M >= 4096 && m->lin_pp &&
        pp_sublinear_ok(lg, m->lin_pp) && block_takes_pre(m, m->c_enc.blocks[0], (size_t)lg.M)) {
      enc_front = m->c_enc.opts;
      enc_front.pre_x = sa.out; enc_front.pre_pp = m->lin_pp; enc_front.pre_sw = m->lin_pp_sw; enc_front.pre_chunks = m->dm.F2;
      dense_deferred = true;
    } else {
      PROF(MI355ASR_K_SUBLINEAR);
      // the two-term stream (a scale per token and 144-wide chunk), then the split-bf16 ring-DMA Dense, from 4096 rows on,
      // else the fp32-MFMA stream kernel
      if (!(m->lin_wsplit && lg.M >= 4096 && ((m->lin_pp && launch_pp_sublinear(lg, m->lin_pp, m->lin_pp_sw, s) == 0) ||
                                              launch_sublinear_split(lg, m->lin_wsplit, s) == 0)))
        LAUNCH_TRY(launch_stream_gemm(d, lg, s), "subsampling linear");
    }
  }
  if (outs->front_out) {
    HIP_TRY(hipMemcpyAsync(outs->front_out, sc.xa, act, hipMemcpyDeviceToDevice, s));
    if ((rc = pad_rows(t_len, T, outs->front_out, d, nullptr))) return rc;
  }
  // ---- encoder
  rc = run_stack(m, m->c_enc, sc.xa, B, T, sc, nullptr, nullptr, s, dense_deferred ? &enc_front : nullptr, t_len, t_len_host);
  if (rc) return rc;
  if (outs->enc_out) {
    HIP_TRY(hipMemcpyAsync(outs->enc_out, sc.xa, act, hipMemcpyDeviceToDevice, s));
    if ((rc = pad_rows(t_len, T, outs->enc_out, d, nullptr))) return rc;
  }
  // ---- phone picker: logits (optional) + per-frame argmax, hidden = block output
  int32_t* amax = (int32_t*)(ws + p.amax);
  rc = run_stack(m, m->c_picker, sc.xa, B, T, sc, outs->picker_logits, amax, s, nullptr, t_len, t_len_host);
  if (rc) return rc;
  if ((rc = pad_rows(t_len, T, outs->picker_logits, m->ccfg.picker_num_classes, nullptr))) return rc;
  float* hid = (float*)(ws + p.hid);
  HIP_TRY(hipMemcpyAsync(hid, sc.xa, act, hipMemcpyDeviceToDevice, s));
  if (outs->picker_hidden) {
    HIP_TRY(hipMemcpyAsync(outs->picker_hidden, sc.xa, act, hipMemcpyDeviceToDevice, s));
    if ((rc = pad_rows(t_len, T, outs->picker_hidden, d, nullptr))) return rc;
  }
  // ---- feature_pick
  int32_t* idx = (int32_t*)(ws + p.idx);
  int32_t* cnt = (int32_t*)(ws + p.cnt);
  PickArgs pa{amax, idx, cnt, B, T, m->ccfg.picker_num_classes - 1};
  pa.t_len = t_len;                    // ragged: frames past an utterance's own are never picked
  LAUNCH_TRY(launch_pick(pa, s), "feature_pick compaction");
  HIP_TRY(hipMemcpyAsync(n_picked, cnt, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));    // the batch maximum sizes everything downstream (dynamic shape in the reference)
  int Tp = 0;
  for (int b = 0; b < B; ++b) Tp = std::max(Tp, n_picked[b]);
  *t_pick = Tp;
  if (Tp == 0) return 0;               // nothing picked: the reference would build [B, 0, V] logits
  GatherArgs ga{hid, idx, cnt, sc.xa, B, T, Tp, d};
  LAUNCH_TRY(launch_gather(ga, s), "feature_pick gather");
  const size_t actp = (size_t)B * Tp * d * 4;
  if (outs->picked) HIP_TRY(hipMemcpyAsync(outs->picked, sc.xa, actp, hipMemcpyDeviceToDevice, s));
  // ---- context helper, text decoder (ragged: each utterance's pick count is its length; the counts are on the host by now)
  const int32_t* p_len = ragged ? cnt : nullptr;
  const int32_t* p_len_host = ragged ? n_picked : nullptr;
  rc = run_stack(m, m->c_helper, sc.xa, B, Tp, sc, nullptr, nullptr, s, nullptr, p_len, p_len_host);
  if (rc) return rc;
  if (outs->helper_out) {
    HIP_TRY(hipMemcpyAsync(outs->helper_out, sc.xa, actp, hipMemcpyDeviceToDevice, s));
    if ((rc = pad_rows(p_len, Tp, outs->helper_out, d, nullptr))) return rc;
  }
  // (no arg-max unless asked for: the text logits go to top-n / the beam search, and a head without it needs no combine launch)
  rc = run_stack(m, m->c_decoder, sc.xa, B, Tp, sc, outs->text_logits, outs->text_logits ? outs->text_argmax : (outs->text_argmax ? outs->text_argmax : amax), s,
                 nullptr, p_len, p_len_host);
  if (rc) return rc;
  return pad_rows(p_len, Tp, outs->text_logits, m->ccfg.decoder_num_classes, outs->text_argmax);
}


}  // namespace

extern "C" {

int mi355asr_chunk_create(const mi355asr_chunk_config* cfg, mi355asr_model** out) {
  if (!cfg || !out) return fail(MI355ASR_EINVAL, "null argument");
  const auto& c = *cfg;
  if (c.dmodel != 144) return fail(MI355ASR_EINVAL, "ChunkConformer: dmodel=%d, kernels instantiated for 144", c.dmodel);
  if (c.num_heads * c.head_size != c.dmodel || c.head_size != 36)
    return fail(MI355ASR_EINVAL, "ChunkConformer: need num_heads*head_size == dmodel and head_size 36");
  if (c.kernel_size != 32 && c.kernel_size != 5) return fail(MI355ASR_EINVAL, "kernel_size=%d unsupported", c.kernel_size);
  if (c.reduction_factor != 4 || c.n_dft != 1024 || (c.n_mels != 80 && c.n_mels != 128))
    return fail(MI355ASR_EINVAL, "ChunkConformer front: reduction_factor 4, n_dft 1024, n_mels 80|128 only");
  if (c.picker_num_classes < 2 || c.decoder_num_classes < 2) return fail(MI355ASR_EINVAL, "num_classes must be >= 2");
  if (c.enc_win_front < 0 || c.picker_win_front < 0 || c.helper_win_front < 0 || c.decoder_win_front < 0 ||
      c.enc_win_back < 0 || c.picker_win_back < 0 || c.helper_win_back < 0 || c.decoder_win_back < 0)
    return fail(MI355ASR_EINVAL, "window sizes must be non-negative");
  auto* m = new mi355asr_model();
  m->is_chunk = true;
  m->ccfg = c;
  std::memset(&m->cfg, 0, sizeof(m->cfg));
  m->cfg.dmodel = c.dmodel; m->cfg.head_size = c.head_size; m->cfg.num_heads = c.num_heads;
  m->cfg.kernel_size = c.kernel_size; m->cfg.fc_factor = c.fc_factor; m->cfg.reduction_factor = 4;
  m->cfg.n_mels = c.n_mels; m->cfg.sample_rate = c.sample_rate; m->cfg.stride_ms = c.stride_ms; m->cfg.n_dft = c.n_dft;
  Dims& dm = m->dm;
  dm.hop = c.stride_ms * c.sample_rate / 1000;
  if (dm.hop <= 0) { delete m; return fail(MI355ASR_EINVAL, "stride_ms*sample_rate/1000 must be positive"); }
  dm.nbins = c.n_dft / 2 + 1;
  dm.NT_dft = ceil_div(ceil_div(2 * dm.nbins, 16), 13) * 13;
  dm.NCH_dft = dm.NT_dft / 13;
  dm.LP = ceil_div(8 * dm.NT_dft, 16) * 16;
  dm.KBm = ceil_div(ceil_div(dm.nbins, 16), 2) * 2;
  dm.NTm = c.n_mels / 16;
  dm.st1 = 2;
  dm.pf1 = 2; dm.pf2 = 0;                          // tf.pad(..., [2,2]) on the mel axis, then VALID convs
  dm.F1 = (c.n_mels + 4 - 3) / 2 + 1;
  dm.F2 = (dm.F1 - 3) / 2 + 1;
  const int d = c.dmodel;
  auto& ex = m->expected;
  ex.push_back({"front/mel_layer/real_kernels", {c.n_dft, 1, 1, dm.nbins}});
  ex.push_back({"front/mel_layer/imag_kernels", {c.n_dft, 1, 1, dm.nbins}});
  ex.push_back({"front/mel_layer/freq2mel", {dm.nbins, c.n_mels}});
  ex.push_back({"front/conv_subsampling/conv1/kernel", {3, 3, 1, d}});
  ex.push_back({"front/conv_subsampling/conv1/bias", {d}});
  ex.push_back({"front/conv_subsampling/conv2/kernel", {3, 3, d, d}});
  ex.push_back({"front/conv_subsampling/conv2/bias", {d}});
  ex.push_back({"front/conv_subsampling/linear/kernel", {dm.F2 * d, d}});
  ex.push_back({"front/conv_subsampling/linear/bias", {d}});
  add_stack_expected(ex, "encoder/", "chunk_conformer_block_", c.enc_num_blocks, d, c.num_heads, c.head_size, c.kernel_size, false, 0, true);
  add_stack_expected(ex, "picker/", "block_", c.picker_num_blocks, d, c.num_heads, c.head_size, c.kernel_size, true, c.picker_num_classes, true);
  add_stack_expected(ex, "helper/", "block_", c.helper_num_blocks, d, c.num_heads, c.head_size, c.kernel_size, false, 0, true);
  add_stack_expected(ex, "decoder/", "block_", c.decoder_num_blocks, d, c.num_heads, c.head_size, c.kernel_size, true, c.decoder_num_classes, true);
  auto opts = [&](int wf, int wb) { BlockOpts o; o.ksz = c.kernel_size; o.fc = c.fc_factor; o.win_front = wf; o.win_back = wb; o.causal = true; return o; };
  m->c_enc.opts = opts(c.enc_win_front, c.enc_win_back);
  m->c_picker.opts = opts(c.picker_win_front, c.picker_win_back);
  m->c_helper.opts = opts(c.helper_win_front, c.helper_win_back);
  m->c_decoder.opts = opts(c.decoder_win_front, c.decoder_win_back);
  *out = m;
  return 0;
}

int mi355asr_chunk_out_frames(const mi355asr_model* m, int32_t L, int32_t* mel_frames, int32_t* enc_frames) {
  if (!m || !m->is_chunk) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle");
  ChunkGeom g;
  int rc = chunk_geometry(m, 1, L, &g);
  if (rc) return rc;
  if (mel_frames) *mel_frames = g.F;
  if (enc_frames) *enc_frames = g.T;
  return 0;
}

int mi355asr_chunk_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes) {
  if (!m || !m->is_chunk || !bytes) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle / null argument");
  ChunkGeom g;
  int rc = chunk_geometry(m, B, L, &g);
  if (rc) return rc;
  *bytes = make_chunk_plan(m, B, g.F, g.T).total;
  return 0;
}

int mi355asr_chunk_predict(mi355asr_model* m, const float* wav, int32_t B, int32_t L, const mi355asr_chunk_outputs* outs,
                           int32_t* n_picked, int32_t* t_pick, void* ws_, size_t ws_bytes, void* stream) {
  return chunk_predict(m, wav, false, nullptr, B, L, outs, n_picked, t_pick, ws_, ws_bytes, stream);
}

int mi355asr_chunk_predict_ragged(mi355asr_model* m, const float* wav, const int32_t* wav_len, int32_t B, int32_t L,
                                  const mi355asr_chunk_outputs* outs, int32_t* n_picked, int32_t* t_pick, void* ws_,
                                  size_t ws_bytes, void* stream) {
  return chunk_predict(m, wav, true, wav_len, B, L, outs, n_picked, t_pick, ws_, ws_bytes, stream);
}

int mi355asr_chunk_workspace_bytes_ragged(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes) {
  if (!m || !m->is_chunk || !bytes) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle / null argument");
  ChunkGeom g;
  int rc = chunk_geometry(m, B, L, &g);
  if (rc) return rc;
  *bytes = chunk_ragged_total(make_chunk_plan(m, B, g.F, g.T), B);
  return 0;
}

int mi355asr_frame_argmax(const float* x, int32_t M, int32_t V, int32_t* out, void* stream) {
  if (!x || !out) return fail(MI355ASR_EINVAL, "null argument");
  if (M < 0 || V < 1) return fail(MI355ASR_EINVAL, "need M >= 0, V >= 1 (got %d, %d)", M, V);
  LAUNCH_TRY(launch_row_argmax(x, out, M, V, (hipStream_t)stream), "frame argmax");
  return 0;
}

// ---- feature_pick as its own entry point (the streaming path calls it between picker and decoder) --------------------
int mi355asr_feature_pick_count(const float* ctc, int32_t B, int32_t T, int32_t V, int32_t* idx, int32_t* cnt,
                                int32_t* counts_host, void* stream) {
  if ((!ctc && T != 0) || !idx || !cnt || !counts_host) return fail(MI355ASR_EINVAL, "null argument");   // (no frames: nothing to point at)
  if (B < 1 || T < 0 || V < 2) return fail(MI355ASR_EINVAL, "need B >= 1, T >= 0, V >= 2 (got %d, %d, %d)", B, T, V);
  hipStream_t s = (hipStream_t)stream;
  if (T == 0) {
    for (int b = 0; b < B; ++b) counts_host[b] = 0;
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(int32_t), s));
    return 0;
  }
  // the per-frame argmax is written to idx and compacted in place: pick_kernel reads a 64-frame group before it writes,
  // and a kept frame t goes to a slot <= t
  LAUNCH_TRY(launch_row_argmax(ctc, idx, B * T, V, s), "feature_pick argmax");
  PickArgs pa{idx, idx, cnt, B, T, V - 1};
  LAUNCH_TRY(launch_pick(pa, s), "feature_pick compaction");
  HIP_TRY(hipMemcpyAsync(counts_host, cnt, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int mi355asr_feature_pick_gather(const float* hidden, const float* ctc, const int32_t* idx, const int32_t* cnt, int32_t B,
                                 int32_t T, int32_t d, int32_t V, int32_t Tp, float* feat_out, float* ctc_out, void* stream) {
  if (!hidden || !idx || !cnt || !feat_out || (ctc_out && !ctc)) return fail(MI355ASR_EINVAL, "null argument");
  if (B < 1 || T < 0 || Tp < 0 || d < 1 || (ctc_out && V < 1))
    return fail(MI355ASR_EINVAL, "need B >= 1, T, Tp >= 0, d >= 1 (got B=%d T=%d Tp=%d d=%d V=%d)", B, T, Tp, d, V);
  hipStream_t s = (hipStream_t)stream;
  if (Tp == 0) return 0;
  GatherArgs ga{hidden, idx, cnt, feat_out, B, T, Tp, d};
  LAUNCH_TRY(launch_gather(ga, s), "feature_pick gather (hidden)");
  if (ctc_out) {
    GatherArgs gc{ctc, idx, cnt, ctc_out, B, T, Tp, V};
    LAUNCH_TRY(launch_gather(gc, s), "feature_pick gather (ctc)");
  }
  return 0;
}

// ---- ChunkConformer streaming ------------------------------------------------------------------------------
int mi355asr_chunk_front_stream_shape(const mi355asr_model* m, int32_t Lw, int32_t S, int32_t chunk_num, int32_t* nf,
                                      int32_t* t_out) {
  if (!m || !m->is_chunk || !nf || !t_out) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle / null argument");
  if (Lw < 1 || S < 0 || chunk_num < m->cfg.reduction_factor)
    return fail(MI355ASR_EINVAL, "need Lw >= 1, S >= 0, chunk_num >= reduction_factor (got %d, %d, %d)", Lw, S, chunk_num);
  int F, T1, T2;
  front_stream_shape(m, Lw, S, chunk_num, &F, nf, &T1, &T2, t_out);
  return 0;
}

int mi355asr_chunk_stream_workspace_bytes(const mi355asr_model* m, int32_t max_rows, int32_t Lw, int32_t S,
                                          int32_t chunk_num, size_t* bytes) {
  if (!m || !m->is_chunk || !bytes) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle / null argument");
  if (max_rows < 1 || Lw < 1 || S < 0 || chunk_num < 1) return fail(MI355ASR_EINVAL, "bad sizes");
  *bytes = make_stream_plan(m, max_rows, (Lw - 1) / m->dm.hop + 1, S + chunk_num).total;
  return 0;
}

int mi355asr_chunk_front_stream(mi355asr_model* m, const float* wav, int32_t Lw, const float* sub_cache, int32_t S,
                                int32_t chunk_num, float* front_out, float* new_sub, void* ws_, size_t ws_bytes,
                                void* stream) {
  if (!m || !m->is_chunk) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (!wav || !front_out || !new_sub || !ws_ || (S > 0 && !sub_cache)) return fail(MI355ASR_EINVAL, "null argument");
  if (Lw < 1 || S < 0 || chunk_num < m->cfg.reduction_factor)
    return fail(MI355ASR_EINVAL, "need Lw >= 1, S >= 0, chunk_num >= reduction_factor (got %d, %d, %d)", Lw, S, chunk_num);
  const auto& c = m->cfg;
  const int d = c.dmodel;
  int F, nf, T1, T2, Tout;
  front_stream_shape(m, Lw, S, chunk_num, &F, &nf, &T1, &T2, &Tout);
  const StreamPlan p = make_stream_plan(m, std::max(Tout, 1), F, S + nf);
  if (ws_bytes < p.total) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  char* ws = (char*)ws_;
  hipStream_t s = (hipStream_t)stream;
  // valid Melspectrogram of the whole buffer (each call left-pads n_dft-1 zeros, as the layer does), last nf frames
  float* mel = (float*)(ws + p.mel);
  if (int rc = run_valid_mel(m, wav, 1, Lw, F, (float*)(ws + p.logp), (float*)(ws + p.pmax), mel, nullptr, s)) return rc;
  // new_sub = [sub cache ; last nf mel frames]  (ConvSubsampling.stream_call :75)
  const size_t mrow = (size_t)c.n_mels * 4;
  if (S > 0) HIP_TRY(hipMemcpyAsync(new_sub, sub_cache, S * mrow, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(new_sub + (size_t)S * c.n_mels, mel + (size_t)(F - nf) * c.n_mels, nf * mrow,
                         hipMemcpyDeviceToDevice, s));
  if (Tout < 1) return 0;
  // pad 2/2 on the mel axis only, two VALID 3x3 stride-2 convs, last Tout frames, Dense (:77-89)
  SubConvArgs sa{};
  sa.mel = new_sub; sa.out = (float*)(ws + p.sub);
  subconv_weights(m, sa, false);
  sa.B = 1; sa.F = S + nf; sa.NM = c.n_mels; sa.T1 = T1; sa.F1 = m->dm.F1; sa.T2 = T2; sa.F2 = m->dm.F2;
  sa.st1 = 2; sa.pt1 = 0; sa.pf1 = 2; sa.pt2 = 0; sa.pf2 = 0;
  { PROF(MI355ASR_K_SUBCONV); LAUNCH_TRY(launch_subconv(d, sa, s), "conv subsampling (stream)"); }
  const StreamGemmArgs lg = sublinear_args(m, sa.out + (size_t)(T2 - Tout) * m->dm.F2 * d, front_out, Tout);
  { PROF(MI355ASR_K_SUBLINEAR); LAUNCH_TRY(launch_stream_gemm(d, lg, s), "subsampling linear"); }
  return 0;
}

int mi355asr_chunk_stack_stream(mi355asr_model* m, int32_t stack, const float* x, int32_t T, const float* mha_cache,
                                int32_t Cm, const float* cnn_cache, int32_t Cc, float* hidden, float* logits,
                                int32_t* amax, float* new_mha, float* new_cnn, void* ws_, size_t ws_bytes,
                                void* stream) {
  if (!m || !m->is_chunk) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  const StackDev* st = chunk_stack_by_id(m, stack);
  if (!st) return fail(MI355ASR_EINVAL, "stack=%d: 0 encoder, 1 picker, 2 helper, 3 decoder", stack);
  if (!x || !hidden || !new_mha || !new_cnn || !ws_ || (Cm > 0 && !mha_cache) || (Cc > 0 && !cnn_cache))
    return fail(MI355ASR_EINVAL, "null argument");
  if (T < 1 || Cm < 0 || Cc < 0) return fail(MI355ASR_EINVAL, "need T >= 1, Cm >= 0, Cc >= 0 (got %d, %d, %d)", T, Cm, Cc);
  if ((logits || amax) && !st->fc_wp) return fail(MI355ASR_EINVAL, "stack %d has no fully_connected head", stack);
  const int d = m->cfg.dmodel;
  const int N = std::max(Cm, Cc) + T;
  const StreamPlan p = make_stream_plan(m, N, 1, 1);
  if (ws_bytes < p.total) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  char* ws = (char*)ws_;
  hipStream_t s = (hipStream_t)stream;
  Scratch sc = make_scratch(p, ws);
  if (st->proj_wp) {
    if (int rc = run_rows_project(m, *st, x, sc.xa, T, s)) return rc;
  } else {
    HIP_TRY(hipMemcpyAsync(sc.xa, x, (size_t)T * d * 4, hipMemcpyDeviceToDevice, s));
  }
  const size_t nb = st->blocks.size();
  for (size_t i = 0; i < nb; ++i) {
    int rc = run_block_stream(m, st->blocks[i], st->opts, sc, T, mha_cache ? mha_cache + i * (size_t)Cm * d : nullptr, Cm,
                              cnn_cache ? cnn_cache + i * (size_t)Cc * d : nullptr, Cc,
                              new_mha + i * (size_t)(Cm + T) * d, new_cnn + i * (size_t)(Cc + T) * d, s);
    if (rc) return rc;
  }
  HIP_TRY(hipMemcpyAsync(hidden, sc.xa, (size_t)T * d * 4, hipMemcpyDeviceToDevice, s));
  if (st->fc_wp && (logits || amax)) {
    if (int rc = run_rows_head(m, *st, sc.xa, T, logits, amax ? amax : (int32_t*)(ws + p.amax), s)) return rc;
  }
  return 0;
}
}  // extern "C"

// =======================================================================================================
// Batched ChunkConformer streaming: many streams per call, all state on the device (chunk_stream.hip has the
// kernels and the row layout).  Stream b of a tick is picker_stream_predict -> feature_pick ->
// decoder_stream_predict of the single-stream path above on that stream's own caches.
// =======================================================================================================
namespace {

constexpr int kCsChunkNum = 16;   // mel frames per packet (ChunkConformerFront.chunk_num of chunk_conformerS.yml)

// one slot of the state buffer, in 4-byte words: [wav cache | sub cache | counters | waiting decoder rows | per block: K ring, V ring, GLU ring]
struct CsLayout {
  int Wb, S, TP, TPd, wbd, nblk;
  size_t wav, sub, hdr, carry, zero_words, slot_words;
  std::vector<size_t> blk;        // K ring of block j (V ring: + wf d, GLU ring: + 2 wf d); blocks in the order encoder, picker, helper, decoder
  size_t meta(int j) const { return hdr + 4 + 4 * (size_t)j; }
};

// refuses what the batched step does not cover (everything chunk_conformerS.yml ships is covered)
int cs_config_ok(const mi355asr_model* m) {
  if (!m || !m->is_chunk) return fail(MI355ASR_EINVAL, "not a ChunkConformer handle");
  const auto& c = m->ccfg;
  if (c.enc_win_back != 0 || c.picker_win_back != 0 || c.helper_win_back != 0)
    return fail(MI355ASR_EINVAL, "batched streams: encoder / picker / helper win_back must be 0 (got %d, %d, %d)", c.enc_win_back,
                c.picker_win_back, c.helper_win_back);
  if (c.decoder_win_back > 16) return fail(MI355ASR_EINVAL, "batched streams: decoder win_back=%d, at most 16", c.decoder_win_back);
  if (m->cfg.gemm_dtype != 0) return fail(MI355ASR_EINVAL, "batched streams: fp32 (gemm_dtype float32) only");
  const int TP = kCsChunkNum / m->cfg.reduction_factor;
  const int wfs[4] = {c.enc_win_front, c.picker_win_front, c.helper_win_front, c.decoder_win_front};
  for (int i = 0; i < 4; ++i) {
    const int rows = i == 3 ? c.decoder_win_back + TP : TP;
    if (wfs[i] < rows || wfs[i] + rows > 64)
      return fail(MI355ASR_EINVAL, "batched streams: win_front=%d of stack %d: need %d <= win_front <= %d", wfs[i], i, rows, 64 - rows);
  }
  if (c.kernel_size < c.decoder_win_back + TP) return fail(MI355ASR_EINVAL, "batched streams: kernel_size=%d too small", c.kernel_size);
  return 0;
}

CsLayout cs_layout(const mi355asr_model* m) {
  const auto& c = m->ccfg;
  const size_t d = m->cfg.dmodel;
  CsLayout L;
  L.Wb = kCsChunkNum * m->dm.hop;
  L.TP = kCsChunkNum / m->cfg.reduction_factor;
  L.S = L.TP;                                   // init_picker_caches: chunk_num / reduction_factor zero mel rows
  L.wbd = c.decoder_win_back;
  L.TPd = L.wbd + L.TP;
  const int nb[4] = {c.enc_num_blocks, c.picker_num_blocks, c.helper_num_blocks, c.decoder_num_blocks};
  const int wf[4] = {c.enc_win_front, c.picker_win_front, c.helper_win_front, c.decoder_win_front};
  L.nblk = nb[0] + nb[1] + nb[2] + nb[3];
  auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
  size_t o = 0;
  L.wav = o; o = up(o + L.Wb);
  L.sub = o; o = up(o + (size_t)L.S * m->cfg.n_mels);
  L.hdr = o; o = up(o + 4 + 4 * (size_t)L.nblk);
  L.zero_words = o;
  L.carry = o; o = up(o + (size_t)std::max(L.wbd, 1) * d);
  for (int st = 0; st < 4; ++st)
    for (int j = 0; j < nb[st]; ++j) {
      L.blk.push_back(o);
      o = up(o + (2 * (size_t)wf[st] + c.kernel_size) * d);
    }
  L.slot_words = o;
  return L;
}

struct CsPlan : ScratchPlan {
  size_t tab, window, logp, pmax, mel, nsub, sub, hid, amax_p, amax_t, total;
};
CsPlan cs_plan(const mi355asr_model* m, const CsLayout& L, int n) {
  const size_t d = m->cfg.dmodel;
  CsPlan p;
  Layout lay;
  lay.scratch(p, (size_t)n * L.TPd, d);
  p.tab = lay.take((size_t)n * 5);               // slots, packet lengths, helper rows, decoder rows, valid decoder rows
  const int F = kCsChunkNum, FT = ceil_div(F, 16);
  p.window = lay.take((size_t)n * ((F - 1) * m->dm.hop + m->cfg.n_dft));
  p.logp = lay.take((size_t)n * F * m->dm.LP);
  p.pmax = lay.take((size_t)n * std::max(FT * m->dm.NCH_dft, F));
  p.mel = lay.take((size_t)n * F * m->cfg.n_mels);
  p.nsub = lay.take((size_t)n * (L.S + F) * m->cfg.n_mels);
  p.sub = lay.take((size_t)n * L.TP * m->dm.F2 * d);
  p.hid = lay.take((size_t)n * L.TP * d);
  p.amax_p = lay.take((size_t)n * L.TP);
  p.amax_t = lay.take((size_t)n * L.TPd);
  p.total = lay.o;
  return p;
}

size_t cs_state_bytes(const CsLayout& L, int n_streams) { return ((size_t)n_streams * L.slot_words + (size_t)n_streams) * 4; }

// One stack over the n TP padded rows in sc.xa (result there too): walk_block_rows (model.h) on every row, attention and depthwise
// conv per stream on its T[i] real rows against its caches.  blk0 = index of the stack's first block in the state layout.
int cs_run_stack(const mi355asr_model* m, const StackDev& st, const CsLayout& L, int blk0, float* state, const int32_t* slots,
                 int n, int TP, const int32_t* T, const int32_t* A, Scratch& sc, hipStream_t s) {
  const int d = m->cfg.dmodel;
  const BlockOpts& bo = st.opts;
  for (size_t i = 0; i < st.blocks.size(); ++i) {
    const BlockDev& w = st.blocks[i];
    const size_t koff = L.blk[blk0 + i], ring = (size_t)bo.win_front * d, meta = L.meta(blk0 + (int)i);
    auto attend = [&]() -> int {
      CsAttnArgs at{};
      at.qkv = sc.qkv; at.ctx = sc.ctx; at.state = state; at.slot_words = L.slot_words; at.meta_off = meta;
      at.k_off = koff; at.v_off = koff + ring; at.slots = slots; at.T = T; at.A = A;
      at.n = n; at.TP = TP; at.H = m->cfg.num_heads; at.wf = bo.win_front; at.wb = bo.win_back;
      PROF(MI355ASR_K_ATTN); LAUNCH_TRY(launch_cs_attn(m->cfg.head_size, at, s), "stream attention");
      return 0;
    };
    auto depthwise = [&]() -> int {
      CsDwArgs dwa{};
      dwa.u = sc.u; dwa.y = sc.dw; dwa.wd = w.dw_w; dwa.state = state; dwa.slot_words = L.slot_words;
      dwa.meta_off = meta; dwa.g_off = koff + 2 * ring; dwa.slots = slots; dwa.T = T; dwa.A = A;
      dwa.n = n; dwa.TP = TP; dwa.D = d; dwa.K = bo.ksz; dwa.wf = bo.win_front;
      PROF(MI355ASR_K_DWCONV); LAUNCH_TRY(launch_cs_dwconv(dwa, s), "stream depthwise conv");
      return 0;
    };
    if (int rc = walk_block_rows(m, w, bo, sc, n * TP, nullptr, s, own_rows, attend, own_rows, depthwise)) return rc;
  }
  return 0;
}

int cs_common_checks(const mi355asr_model* m, int n_streams) {
  if (int rc = cs_config_ok(m)) return rc;
  if (n_streams < 1) return fail(MI355ASR_EINVAL, "n_streams=%d: need at least one slot", n_streams);
  return 0;
}

// slots_host [n]: in range, each at most once
int cs_check_slots(const int32_t* slots, int n, int n_streams) {
  std::vector<char> seen((size_t)n_streams, 0);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= n_streams) return fail(MI355ASR_EINVAL, "slot %d (entry %d) out of range 0 .. %d", slots[i], i, n_streams - 1);
    if (seen[slots[i]]) return fail(MI355ASR_EINVAL, "slot %d is named twice", slots[i]);
    seen[slots[i]] = 1;
  }
  return 0;
}

}  // namespace

extern "C" {

int mi355asr_chunk_streams_bytes(const mi355asr_model* m, int32_t n_streams, size_t* state_bytes, size_t* ws_bytes) {
  if (int rc = cs_common_checks(m, n_streams)) return rc;
  const CsLayout L = cs_layout(m);
  if (state_bytes) *state_bytes = cs_state_bytes(L, n_streams);
  if (ws_bytes) *ws_bytes = cs_plan(m, L, n_streams).total;      // a tick of n streams needs the plan of n: any n <= n_streams fits
  return 0;
}

int mi355asr_chunk_streams_reset(mi355asr_model* m, void* state_dev, int32_t n_streams, const int32_t* slots_host, int32_t n,
                                 void* stream) {
  if (int rc = cs_common_checks(m, n_streams)) return rc;
  if (!state_dev) return fail(MI355ASR_EINVAL, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const CsLayout L = cs_layout(m);
  CsResetArgs ra{};
  ra.state = (float*)state_dev; ra.slot_words = L.slot_words; ra.zero_words = (int)L.zero_words;
  if (!slots_host) {
    ra.n = n_streams;
  } else {
    if (n < 1) return fail(MI355ASR_EINVAL, "n=%d: need at least one slot", n);
    if (int rc = cs_check_slots(slots_host, n, n_streams)) return rc;
    // the slot table travels in the tail of the state buffer (n_streams words behind the slots)
    int32_t* tab = (int32_t*)state_dev + (size_t)n_streams * L.slot_words;
    m->cs_tab.assign(slots_host, slots_host + n);
    HIP_TRY(hipMemcpyAsync(tab, m->cs_tab.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    ra.slots = tab; ra.n = n;
  }
  LAUNCH_TRY(launch_cs_reset(ra, s), "stream reset");
  return 0;
}

int mi355asr_chunk_streams_step(mi355asr_model* m, void* state_dev, int32_t n_streams, const int32_t* slots_host, int32_t n,
                                const float* packets_dev, const int32_t* n_samples_host,
                                const mi355asr_chunk_streams_outputs* outs, void* ws_, size_t ws_bytes, void* stream) {
  if (int rc = cs_common_checks(m, n_streams)) return rc;
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (!state_dev || !slots_host || !packets_dev || !outs || !ws_) return fail(MI355ASR_EINVAL, "null argument");
  if (n < 1 || n > n_streams) return fail(MI355ASR_EINVAL, "n=%d: need 1 .. n_streams (%d)", n, n_streams);
  if (int rc = cs_check_slots(slots_host, n, n_streams)) return rc;
  const CsLayout L = cs_layout(m);
  if (n_samples_host)
    for (int i = 0; i < n; ++i)
      if (n_samples_host[i] < 1 || n_samples_host[i] > L.Wb)
        return fail(MI355ASR_EINVAL, "n_samples[%d]=%d: need 1 .. %d", i, n_samples_host[i], L.Wb);
  const CsPlan p = cs_plan(m, L, n);
  if (ws_bytes < p.total) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  char* ws = (char*)ws_;
  hipStream_t s = (hipStream_t)stream;
  const auto& c = m->cfg;
  const int d = c.dmodel, TP = L.TP, TPd = L.TPd;
  float* state = (float*)state_dev;
  Scratch sc = make_scratch(p, ws);
  // ---- the tick's tables: slots and packet lengths up, the per-stream row counts are made on the device
  int32_t* tab = (int32_t*)(ws + p.tab);
  int32_t *slots = tab, *nsamp = tab + n, *Th = tab + 2 * n, *Td = tab + 3 * n, *Vd = tab + 4 * n;
  m->cs_tab.assign(slots_host, slots_host + n);
  if (n_samples_host) m->cs_tab.insert(m->cs_tab.end(), n_samples_host, n_samples_host + n);
  HIP_TRY(hipMemcpyAsync(tab, m->cs_tab.data(), m->cs_tab.size() * 4, hipMemcpyHostToDevice, s));
  // ---- front: window of [wav cache ; packet], valid mel, [sub cache ; mel], two VALID convs, Dense
  const int F = kCsChunkNum;
  CsFrontArgs fa{};
  fa.state = state; fa.slot_words = L.slot_words; fa.wav_off = L.wav; fa.slots = slots; fa.packets = packets_dev;
  fa.n_samples = n_samples_host ? nsamp : nullptr; fa.window = (float*)(ws + p.window);
  fa.n = n; fa.Wb = L.Wb; fa.Lwin = (F - 1) * m->dm.hop + c.n_dft; fa.hop = m->dm.hop;
  LAUNCH_TRY(launch_cs_front_window(fa, s), "stream front window");
  float* mel = (float*)(ws + p.mel);
  // the window's frames begin at multiples of hop: the valid framing with nothing padded in front
  if (int rc = run_valid_mel(m, fa.window, n, fa.Lwin, F, (float*)(ws + p.logp), (float*)(ws + p.pmax), mel, nullptr, s, 0)) return rc;
  CsSubArgs su{};
  su.state = state; su.slot_words = L.slot_words; su.sub_off = L.sub; su.slots = slots; su.mel = mel;
  su.new_sub = (float*)(ws + p.nsub); su.n = n; su.S = L.S; su.F = F; su.NM = c.n_mels;
  LAUNCH_TRY(launch_cs_sub(su, s), "stream sub cache");
  const int rows = L.S + F, T1 = (rows - 3) / 2 + 1, T2 = (T1 - 3) / 2 + 1;
  if (T2 != TP) return fail(MI355ASR_EINVAL, "batched streams: the front yields %d rows per packet, expected %d", T2, TP);
  SubConvArgs sa{};
  sa.mel = su.new_sub; sa.out = (float*)(ws + p.sub);
  subconv_weights(m, sa, false);
  sa.B = n; sa.F = rows; sa.NM = c.n_mels; sa.T1 = T1; sa.F1 = m->dm.F1; sa.T2 = T2; sa.F2 = m->dm.F2;
  sa.st1 = 2; sa.pt1 = 0; sa.pf1 = 2; sa.pt2 = 0; sa.pf2 = 0;
  { PROF(MI355ASR_K_SUBCONV); LAUNCH_TRY(launch_subconv(d, sa, s), "conv subsampling (streams)"); }
  const StreamGemmArgs lg = sublinear_args(m, sa.out, sc.xa, n * TP);
  { PROF(MI355ASR_K_SUBLINEAR); LAUNCH_TRY(launch_stream_gemm(d, lg, s), "subsampling linear"); }
  // ---- encoder, phone picker (win_back 0: every row is valid, nothing waits)
  const auto& cc = m->ccfg;
  int blk = 0;
  if (int rc = cs_run_stack(m, m->c_enc, L, blk, state, slots, n, TP, nullptr, nullptr, sc, s)) return rc;
  blk += cc.enc_num_blocks;
  if (int rc = run_rows_project(m, m->c_picker, sc.xa, sc.xa, n * TP, s)) return rc;
  if (int rc = cs_run_stack(m, m->c_picker, L, blk, state, slots, n, TP, nullptr, nullptr, sc, s)) return rc;
  blk += cc.picker_num_blocks;
  int32_t* amax_p = outs->phone_argmax ? outs->phone_argmax : (int32_t*)(ws + p.amax_p);
  if (int rc = run_rows_head(m, m->c_picker, sc.xa, n * TP, outs->phone_logits, amax_p, s)) return rc;
  float* hid = (float*)(ws + p.hid);
  HIP_TRY(hipMemcpyAsync(hid, sc.xa, (size_t)n * TP * d * 4, hipMemcpyDeviceToDevice, s));
  if (outs->picker_hidden) HIP_TRY(hipMemcpyAsync(outs->picker_hidden, sc.xa, (size_t)n * TP * d * 4, hipMemcpyDeviceToDevice, s));
  // ---- feature_pick: the rows the picker did not call blank, and with them the row counts of the second half
  CsPickArgs pa{};
  pa.amax = amax_p; pa.hidden = hid; pa.picked = sc.xa; pa.state = state; pa.slot_words = L.slot_words; pa.hdr_off = L.hdr;
  pa.slots = slots; pa.Th = Th; pa.Td = Td; pa.Vd = Vd;
  pa.n_picked = outs->n_picked; pa.n_valid = outs->n_valid; pa.n_unvalid = outs->n_unvalid;
  pa.n = n; pa.TP = TP; pa.D = d; pa.blank = cc.picker_num_classes - 1; pa.wb = L.wbd;
  LAUNCH_TRY(launch_cs_pick(pa, s), "stream feature_pick");
  // ---- context helper on the picked rows
  if (int rc = cs_run_stack(m, m->c_helper, L, blk, state, slots, n, TP, Th, nullptr, sc, s)) return rc;
  blk += cc.helper_num_blocks;
  // ---- text decoder on [waiting rows ; helper output]; its last win_back rows wait for the next tick
  float* dec_in = sc.xb;                        // (free between two stacks)
  CsCarryArgs ca{};
  ca.helped = sc.xa; ca.dec_in = dec_in; ca.state = state; ca.slot_words = L.slot_words; ca.hdr_off = L.hdr; ca.carry_off = L.carry;
  ca.slots = slots; ca.Td = Td; ca.Vd = Vd; ca.n = n; ca.TP = TP; ca.TPd = TPd; ca.D = d;
  LAUNCH_TRY(launch_cs_carry(ca, s), "stream decoder input");
  if (int rc = run_rows_project(m, m->c_decoder, dec_in, sc.xa, n * TPd, s)) return rc;
  if (int rc = cs_run_stack(m, m->c_decoder, L, blk, state, slots, n, TPd, Td, Vd, sc, s)) return rc;
  int32_t* amax_t = outs->text_argmax ? outs->text_argmax : (int32_t*)(ws + p.amax_t);
  return run_rows_head(m, m->c_decoder, sc.xa, n * TPd, outs->text_logits, amax_t, s);
}

}  // extern "C"
