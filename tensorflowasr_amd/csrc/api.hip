// libmi355asr.so host side: model object, workspace planning and the launch sequences behind the ConformerCTC / CTCDecoder
// entry points of the C ABI declared in include/mi355asr.h.  (Weights: weights.hip; which kernels run a block: block_path.hip.)
#include "common.h"
#include "mfma_ops.h"
#include "model.h"

namespace mi355 {


thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

void same_pad(int n, int k, int s, int* out, int* before) {
  const int o = ceil_div(n, s);
  const int tot = std::max((o - 1) * s + k - n, 0);
  *out = o;
  *before = tot / 2;
}

int launch_mel_auto(const mi355asr_model* m, MelArgs& me, hipStream_t s) {
  if (m->mel_band) {
    me.band = m->mel_band; me.bw = m->mel_bw; me.BW = m->mel_BW;
    if (launch_mel_band(me, s) == 0) return 0;
  }
  me.absmax = nullptr;          // the dense kernel does not produce the run-time maximum: the caller must not rely on it
  return launch_mel(me, s);
}

int launch_gemm16(const mi355asr_model* m, int epi, bool ln, Gemm16Args& g, const float* wp, hipStream_t s) {
  // long batches of dmodel 256 / 512: the same layer with the weights as a slab ring shared by eight waves
  // (gemm_ring.hip): fp32 operands exactly split into three bf16 terms, or one bf16 term in bf16 mode
  // crossover measured with 10 s utterances (tools/model_batch_sweep.py; ms per batch, ring vs per-wave streams):
  // ConformerM B = 4: 3.81 vs 3.10, 8: 4.09 vs 4.26, 16: 4.47 vs 5.19; ConformerL 4: 6.95 vs 6.57, 8: 7.59 vs 9.63, 16: 10.3 vs 18.5
  if ((long)g.M >= ring_min_rows() && !m->ring_of.empty()) {
    const auto it = m->ring_of.find(wp);
    g.wp = wp;
    // round 6, bf16 mode, K = 256, from 8 192 rows: the rows resident in LDS, the column tiles split over the waves (bf16.hip)
    if (it != m->ring_of.end() && m->cfg.gemm_dtype == 1 && launch_gemm256_bf16(epi, ln, g, it->second, s) == 0) return 0;
    if (it != m->ring_of.end() && launch_gemm_ring(epi, ln, g, it->second, m->cfg.gemm_dtype == 1 ? 1 : 3, s) == 0) return 0;
  }
  if (m->cfg.gemm_dtype == 1) { g.wp = m->w16(wp); return launch_gemm16_bf16(epi, ln, g, s); }
  g.wp = wp;
  return launch_gemm16_f32(epi, ln, g, s);
}

// ---- workspace plan (byte offsets, 256-byte aligned) --------------------------------------------------


size_t wavpick_floats(const mi355asr_model* m, int Bp, int Lmax);
constexpr int kWavMinFrames = 3;   // add_wav_info: the fewest encoder frames per input (REFLECT padding by 2, see encoder_impl)

// Bp = number of independent encoder inputs (utterances, or utterances x blocks when streaming),
// F mel frames and T encoder frames per input.
Plan make_plan(const mi355asr_model* m, int Bp, int F, int T) {
  const int d = m->cfg.dmodel;
  const size_t M = (size_t)Bp * T;
  Plan p;
  Layout lay;
  auto take = [&](size_t floats) { return lay.take(floats); };
  lay.scratch(p, M, d);
  // (h4 = 0 aliases xa: safe only because every stack of this plan runs on exactly M rows, so the layer-at-a-time launches run
  // for all of them or for none -- a stage on fewer rows must plan h4 itself, as make_chunk_plan does)
  p.h4 = gemm16_for(m, M) ? take(M * 4 * d) : 0;   // before logp: the block-only entry points size to p.logp
  p.enc = take(M * d);
  p.amax = take(M);
  const int FT = ceil_div(F, 16);
  p.logp = take((size_t)Bp * F * m->dm.LP);
  p.pmax = take((size_t)Bp * std::max(FT * m->dm.NCH_dft, F));
  p.umax = take(Bp);
  p.mel = take((size_t)Bp * F * m->cfg.n_mels);
  p.sub = take(M * m->dm.F2 * d);
  p.wv_floats = wavpick_floats(m, Bp, F * m->dm.hop);      // add_wav_info branch (0 when off); L <= F * hop
  p.wv = p.wv_floats ? take(p.wv_floats) : 0;
  p.total = lay.o;
  return p;
}


int geometry(const mi355asr_model* m, int B, int L, Geometry* g) {
  const auto& c = m->cfg;
  if (B <= 0 || L <= 0) return fail(MI355ASR_EINVAL, "B and L must be positive (B=%d, L=%d)", B, L);
  g->nblk = 1;
  g->Lb = L;
  if (c.chunk_size > 0) {
    if (L % c.chunk_size != 0)
      return fail(MI355ASR_EINVAL, "streaming encoder: L=%d is not a multiple of chunk_size=%d "
                  "(the reference reshapes [B,L,1]->[-1,chunk,1], conformer_blocks.py:585)", L, c.chunk_size);
    g->nblk = L / c.chunk_size;
    g->Lb = c.chunk_size;
  }
  g->Bp = B * g->nblk;
  g->F = ceil_div(g->Lb, m->dm.hop);
  g->T1 = ceil_div(g->F, m->dm.st1);
  g->T = ceil_div(g->T1, 2);
  return 0;
}

// ---- launch sequences ---------------------------------------------------------------------------------

int run_mel(const mi355asr_model* m, const float* wav, int Bp, int Lb, int F, float* logp, float* pmax,
            float* umax, float* mel, hipStream_t s, const int32_t* wav_len = nullptr) {
  const auto& c = m->cfg;
  if (wav_len && (c.mel_layer_type != 0 || !m->fft_ok))
    return fail(MI355ASR_EINVAL, "ragged batches: the Melspectrogram frontend on the FFT STFT only (%s)",
                c.mel_layer_type == 1 ? "LEAF frontend" : c.mel_layer_type == 2 ? "Spectrogram layer" : "dense DFT STFT, stft_mode 0");
  if (c.mel_layer_type == 1) {
    // LEAF: Gabor conv + squared modulus + Gaussian pooling (partials in the log-power scratch), then PCEN + instance norm
    int nf, pl;
    same_pad(Lb, 401, m->dm.hop, &nf, &pl);
    // leaf_terms = 0: fp32 MFMA kernel, tiles of 128 positions; 2 / 3: split-bf16 kernel, tiles of 512 (leaf.hip)
    const int tile = m->leaf_terms ? kLeafSplitTile : 128, nrel = m->leaf_terms ? kLeafSplitSlots : 4;
    const int NH = ceil_div(Lb, tile);
    if (m->leaf_terms) {
      LeafConvArgs la{wav, m->leaf_wsplit, m->leaf_gcoef, logp, m->leaf_p0, m->leaf_p1, Bp, Lb, F, NH, m->dm.hop, pl};
      PROF(MI355ASR_K_STFT);
      LAUNCH_TRY(launch_leaf_conv_pool_split(m->leaf_terms, la, s), "leaf gabor conv (split bf16) + pooling");
    } else {
      LeafConvArgs la{wav, m->leaf_wp, m->leaf_gcoef, logp, m->leaf_p0, m->leaf_p1, Bp, Lb, F, NH, m->dm.hop, pl};
      PROF(MI355ASR_K_STFT);
      LAUNCH_TRY(launch_leaf_conv_pool(la, s), "leaf gabor conv + pooling");
    }
    LeafPcenArgs lp{logp, m->leaf_alpha, m->leaf_delta, m->leaf_root, m->leaf_smooth, m->leaf_gamma, m->leaf_beta, mel,
                    Bp, F, NH, m->dm.hop, pl, tile, nrel};
    { PROF(MI355ASR_K_MEL); LAUNCH_TRY(launch_leaf_pcen_norm(lp, s), "leaf PCEN + instance norm"); }
    return 0;
  }
  const int FT = ceil_div(F, 16);
  int out, before;
  same_pad(Lb, c.n_dft, m->dm.hop, &out, &before);
  StftArgs st{};
  st.wav = wav; st.logp = logp; st.pmax = pmax; st.wp = m->dft_wp;
  st.B = Bp; st.L = Lb; st.F = F; st.hop = m->dm.hop; st.pad_left = before; st.n_dft = c.n_dft;
  st.NT = m->dm.NT_dft; st.LP = m->dm.LP; st.nbins = m->dm.nbins; st.FT = FT; st.NCH = m->dm.NCH_dft;
  st.db10 = 1;
  int npart = FT * m->dm.NCH_dft;
  if (m->fft_ok) {
    FftStftArgs fa{wav, logp, pmax, m->fft_w1p, m->fft_w2p, m->fft_twc, m->fft_tws, m->fft_win,
                   Bp, Lb, F, m->dm.hop, before, m->dm.LP, 1};
    fa.w1s = m->fft_w1s; fa.w2s = m->fft_w2s; fa.w1h = m->fft_w1h; fa.w2h = m->fft_w2h;
    fa.wav_len = wav_len;
    { PROF(MI355ASR_K_STFT); LAUNCH_TRY(launch_fft_stft(fa, s), "stft (fft)"); }
    npart = F;
  } else {
    PROF(MI355ASR_K_STFT);
    LAUNCH_TRY(launch_stft(st, s), "stft");
  }
  UttMaxArgs um{pmax, umax, npart};
  um.wav_len = wav_len; um.hop = m->dm.hop;
  { PROF(MI355ASR_K_UTT_MAX); LAUNCH_TRY(launch_utt_max(um, Bp, s), "utterance max"); }
  MelArgs me{};
  me.logp = logp; me.umax = umax; me.mel = mel; me.wp = m->mel_wp;
  me.B = Bp; me.F = F; me.LP = m->dm.LP; me.nbins = m->dm.nbins; me.KBm = m->dm.KBm; me.NTm = m->dm.NTm;
  me.NM = c.n_mels; me.FT = FT; me.floor_db = -80.0f;
  if (c.mel_layer_type == 2) { PROF(MI355ASR_K_MEL); LAUNCH_TRY(launch_db_norm(me, s), "dB (Spectrogram layer)"); }
  else { PROF(MI355ASR_K_MEL); LAUNCH_TRY(launch_mel_auto(m, me, s), "dB + mel"); }
  return 0;
}

// mel_bounded: the features come from this handle's own frontend (|mel| <= 80 x the filters' L1 norm), which the two-term
// fp16 kernel's operand scale relies on; features handed in by the caller take the three-term bf16 kernel
int run_subsampling(const mi355asr_model* m, const float* mel, int Bp, int F, float* sub, float* out,
                    hipStream_t s, bool mel_bounded, bool* defer_dense, const int32_t* wav_len) {
  if (defer_dense) *defer_dense = false;
  const auto& c = m->cfg;
  const int d = c.dmodel;
  int T1, pt1, T2, pt2;
  same_pad(F, 3, m->dm.st1, &T1, &pt1);
  same_pad(T1, 3, 2, &T2, &pt2);
  SubConvArgs sa{};
  sa.mel = mel; sa.out = sub;
  subconv_weights(m, sa, true);
  static const bool force_half = mi355_env("MI355ASR_SUBCONV_TERMS", -1) == 22;   // 22: also for caller-supplied features (tests)
  if (m->c2_whalf && (mel_bounded || force_half)) { sa.w2h = m->c2_whalf; sa.h_scale = m->c2_hscale; sa.h_wscale = m->c2_wscale; }
  // conv1 on the matrix pipe needs the frontend's own bound on |mel| for its fp16 planes: not for caller-supplied features
  if (sa.w2h && mel_bounded) { sa.c1_mscale = m->c1_mscale; sa.c1_wscale = m->c1_wscale; }
  sa.B = Bp; sa.F = F; sa.NM = c.n_mels; sa.T1 = T1; sa.F1 = m->dm.F1; sa.T2 = T2; sa.F2 = m->dm.F2;
  sa.st1 = m->dm.st1; sa.pt1 = pt1; sa.pf1 = m->dm.pf1; sa.pt2 = pt2; sa.pf2 = m->dm.pf2;
  sa.wav_len = wav_len; sa.hop = m->dm.hop;
  { PROF(MI355ASR_K_SUBCONV); LAUNCH_TRY(launch_subconv(d, sa, s), wav_len ? "conv subsampling of a ragged batch" : "conv subsampling"); }
  if (use_gemm16(m)) {
    Gemm16Args lg{};
    lg.x = sub; lg.ldx = m->dm.F2 * d; lg.bias = m->lin_b; lg.y = out; lg.ldy = d;
    lg.M = Bp * T2; lg.K = m->dm.F2 * d; lg.NT = d / 16; lg.n_valid = d; lg.eps = kLnEps;
    { PROF(MI355ASR_K_SUBLINEAR); LAUNCH_TRY(launch_gemm16(m, E16_BIAS, false, lg, m->lin_wp, s), "subsampling linear"); }
    return 0;
  }
  const StreamGemmArgs lg = sublinear_args(m, sub, out, Bp * T2);
  // MI355ASR_SUBLINEAR_SPLIT: 1 (default) = split-bf16 ring-DMA kernel (fused.hip) from 4096 rows, 2 = for any row
  // count, 0 = the fp32-MFMA stream_gemm_kernel
  static const int lin_split = (int)mi355_env("MI355ASR_SUBLINEAR_SPLIT", 1);
  if (lin_split && m->lin_wsplit && (lg.M >= 4096 || lin_split == 2)) {
    if (defer_dense && m->lin_pp && pp_sublinear_ok(lg, m->lin_pp)) { *defer_dense = true; return 0; }   // the caller folds it into the first block
    PROF(MI355ASR_K_SUBLINEAR);
    // round 4: two fp16 terms with a scale per (token, 144-wide chunk) -- no bound on the operand needed, so caller-supplied
    // features take it too; the three-term kernel behind MI355ASR_PP_SUBLINEAR=0 / MI355ASR_PP=0
    if (m->lin_pp && launch_pp_sublinear(lg, m->lin_pp, m->lin_pp_sw, s) == 0) return 0;
    if (launch_sublinear_split(lg, m->lin_wsplit, s) == 0) return 0;
  }
  {
    PROF(MI355ASR_K_SUBLINEAR);
    // round 6, small batches (the fp32 stream_gemm kernel took 38 us for one utterance): one 16-token tile per workgroup, the 144-wide
    // chunks of a row split over its eight waves, on the two-term fragments of pp_sublinear_kernel (MI355ASR_SUBLINEAR_SPLIT=0: off)
    if (lin_split && m->lin_ns && pp_sublinear_ok(lg, m->lin_pp) && launch_ns1_sublinear(lg, m->lin_ns, m->lin_pp_sw, s) == 0) return 0;
    if (launch_stream_gemm(d, lg, s) == 0) return 0;
  }
  // K = F2 * dmodel that is not a multiple of 32 (the plain Spectrogram layer: F2 = 129): the layer-at-a-time kernel
  Gemm16Args g16{};
  g16.x = sub; g16.ldx = m->dm.F2 * d; g16.bias = m->lin_b; g16.y = out; g16.ldy = d;
  g16.M = Bp * T2; g16.K = m->dm.F2 * d; g16.NT = d / 16; g16.n_valid = d; g16.eps = kLnEps;
  { PROF(MI355ASR_K_SUBLINEAR); LAUNCH_TRY(launch_gemm16(m, E16_BIAS, false, g16, m->lin_wp, s), "subsampling linear"); }
  return 0;
}


int check_ready(const mi355asr_model* m, bool need_encoder = false) {
  if (!m) return fail(MI355ASR_EINVAL, "null model handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  if (m->is_chunk) return fail(MI355ASR_ESTATE, "ChunkConformer handle: use mi355asr_chunk_predict");
  if (m->is_translator) return fail(MI355ASR_ESTATE, "Translator handle: use mi355asr_translator_forward");
  if (m->is_vad) return fail(MI355ASR_ESTATE, "VAD handle: use mi355asr_vad_forward");
  if (m->is_punc) return fail(MI355ASR_ESTATE, "Punc handle: use mi355asr_punc_forward");
  if (need_encoder && !m->cfg.has_encoder) return fail(MI355ASR_ESTATE, "model was created without an encoder (has_encoder=0)");
  return 0;
}


// WavePickModel.get_scales (wav_model.py:132-146): prime factors of hop_size merged down to four strides, descending
std::vector<int> wave_pick_scales(int num) {
  std::vector<int> sc;
  while (num > 1) {
    int i = 2;
    while (i < 100 && num % i != 0) ++i;
    if (i >= 100) return {};
    num /= i;
    sc.push_back(i);
  }
  while (sc.size() > 4) {
    std::vector<int> ns(sc.begin() + 2, sc.end());
    ns.push_back(sc[0] * sc[1]);
    std::sort(ns.begin(), ns.end());
    sc = ns;
  }
  std::reverse(sc.begin(), sc.end());
  return sc;
}

// floats of scratch the add_wav_info branch needs for Bp inputs of at most Lmax samples
size_t wavpick_floats(const mi355asr_model* m, int Bp, int Lmax) {
  if (!m->cfg.add_wav_info || m->wp_stride0 == 0) return 0;
  const size_t T0 = ceil_div(Lmax, m->wp_stride0);
  size_t s1 = 0, t = T0;
  for (const auto& st : m->wp_stages) { t = ceil_div((int)t, st.stride); s1 = std::max(s1, (t + 8) * (size_t)st.c); }
  return (size_t)Bp * ((T0 + 8) * 32 * 2 + 4 * s1) + 1024;
}

// xa[Bp*T, d] += WavePickModel(wav)  (conformer_blocks.py:344-348); every Conv1D is a GEMM over overlapping rows of a
// padded channels-last copy of its input (wavpick.hip)
int run_wavpick(const mi355asr_model* m, const float* wav, int Bp, int Lb, int T, float* xa, float* wv, hipStream_t s) {
  const int d = m->cfg.dmodel;
  const float slope = 0.3f;                          // tf.keras.layers.LeakyReLU() default
  const int T0 = ceil_div(Lb, m->wp_stride0);
  size_t s1 = 0;
  { int t = T0; for (const auto& st : m->wp_stages) { t = ceil_div(t, st.stride); s1 = std::max(s1, (size_t)(t + 8) * st.c); } }
  float* bufA = wv;
  float* bufP = bufA + (size_t)Bp * (T0 + 8) * 32;
  float* bufY = bufP + (size_t)Bp * (T0 + 8) * 32;
  float* bufH = bufY + (size_t)Bp * s1;
  float* bufG = bufH + (size_t)Bp * s1;
  float* bufS = bufG + (size_t)Bp * s1;
  int out0, pl0;
  same_pad(Lb, 7, m->wp_stride0, &out0, &pl0);
  WpSepConvArgs sa{wav, m->wp_dw, m->wp_pw, m->wp_b, bufA, Bp, Lb, T0, m->wp_stride0, pl0, slope};
  LAUNCH_TRY(launch_wp_sepconv(sa, s), "wav_layer separable conv");
  auto conv = [&](const float* xpad, int Tpad, int cin, int k, int stride, int Tout, const float* wp, const float* bias, int cout,
                  float* y, const float* res) -> int {
    Gemm16Args g{};
    g.x = xpad; g.ldx = stride * cin; g.K = k * cin; g.wp = wp; g.bias = bias; g.NT = cout / 16; g.y = y; g.ldy = cout;
    g.M = Bp * Tout; g.n_valid = cout; g.eps = kLnEps; g.scale = 1.0f; g.res = res;
    g.rpb = Tout; g.bstride = (long long)Tpad * cin;
    LAUNCH_TRY(launch_gemm16_f32(res ? E16_RES : E16_BIAS, false, g, s), "wav_layer conv1d");
    return 0;
  };
  const float *cur = bufA, *cur2 = nullptr;
  int Tc = T0, cin = 32;
  for (const auto& st : m->wp_stages) {
    int Tn, lo;
    same_pad(Tc, 3, st.stride, &Tn, &lo);
    const int hi = std::max((Tn - 1) * st.stride + 3 - Tc, 0) - lo;
    WpPadActArgs pz{cur, cur2, bufP, Bp, Tc, cin, lo, hi, 0, 1.0f};
    LAUNCH_TRY(launch_wp_pad_act(pz, s), "wav_layer zero pad");
    int rc = conv(bufP, Tc + lo + hi, cin, 3, st.stride, Tn, st.cw, st.cb, st.c, bufY, nullptr);
    if (rc) return rc;
    // TFResidualStack (wav_model.py:57-104)
    WpPadActArgs pr{bufY, nullptr, bufP, Bp, Tn, st.c, 2, 2, 1, slope};
    LAUNCH_TRY(launch_wp_pad_act(pr, s), "wav_layer reflect pad + LeakyReLU");
    rc = conv(bufP, Tn + 4, st.c, 5, 1, Tn, st.w5, st.b5, st.c, bufH, nullptr);
    if (rc) return rc;
    WpPadActArgs pg{bufH, nullptr, bufG, Bp, Tn, st.c, 0, 0, 0, slope};
    LAUNCH_TRY(launch_wp_pad_act(pg, s), "wav_layer LeakyReLU");
    rc = conv(bufY, Tn, st.c, 1, 1, Tn, st.ws, st.bs, st.c, bufS, nullptr);
    if (rc) return rc;
    rc = conv(bufG, Tn, st.c, 1, 1, Tn, st.w1, st.b1, st.c, bufH, nullptr);
    if (rc) return rc;
    cur = bufS; cur2 = bufH; Tc = Tn; cin = st.c;    // the sum of the two branches is formed by the next padded copy
  }
  if (Tc != T) return fail(MI355ASR_EINVAL, "add_wav_info: the waveform branch yields %d frames, the frontend %d", Tc, T);
  WpPadActArgs pf{cur, cur2, bufP, Bp, Tc, cin, 3, 3, 0, 1.0f};
  LAUNCH_TRY(launch_wp_pad_act(pf, s), "wav_layer zero pad");
  return conv(bufP, Tc + 6, cin, 7, 1, Tc, m->wp_fw, m->wp_fb, d, xa, xa);
}

// the encoder's block stack as stream256_kernel's arguments; false: not its shape (or a ring pack is missing, or switched off)
bool stream256_args(const mi355asr_model* m, int B, int T, const float* x, float* y, S256Args& sa) {
  static const bool on = mi355_env("MI355ASR_STREAM256", 1) != 0;
  const int nb = m->cfg.num_blocks;
  if (!on || m->cfg.gemm_dtype != 1 || m->cfg.dmodel != 256 || m->cfg.num_heads != 4 || m->cfg.head_size != 64 ||
      !stream256_shape_ok(B, T, nb, m->cfg.kernel_size) || (int)m->enc_blocks.size() < nb)
    return false;
  auto ring = [&](const float* wp) -> const void* { const auto it = m->ring_of.find(wp); return it == m->ring_of.end() ? nullptr : it->second; };
  sa.x = x; sa.y = y; sa.B = B; sa.T = T; sa.nblocks = nb; sa.ksz = m->cfg.kernel_size; sa.pad_left = (m->cfg.kernel_size - 1) / 2;
  sa.fc = m->cfg.fc_factor; sa.qscale = 1.0f / std::sqrt((float)m->cfg.head_size); sa.eps = kLnEps;
  for (int i = 0; i < nb; ++i) {
    const BlockDev& w = m->enc_blocks[i];
    S256Block& b = sa.blk[i];
    for (int k = 0; k < 2; ++k) {
      b.ff_ln_g[k] = w.ff_ln_g[k]; b.ff_ln_b[k] = w.ff_ln_b[k]; b.ff_b1[k] = w.ff_b1[k]; b.ff_b2[k] = w.ff_b2[k];
      b.ff_w1[k] = ring(w.ff_w1p[k]); b.ff_w2[k] = ring(w.ff_w2p[k]);
      if (!b.ff_w1[k] || !b.ff_w2[k]) return false;
    }
    b.att_ln_g = w.att_ln_g; b.att_ln_b = w.att_ln_b; b.qkv_b = w.qkv_b; b.out_b = w.out_b;
    b.qkv_w = ring(w.qkv_wp); b.out_w = ring(w.out_wp);
    b.cv_ln_g = w.cv_ln_g; b.cv_ln_b = w.cv_ln_b; b.pw1_b = w.pw1_b; b.dw_w = w.dw_w; b.pc_b1 = w.pc_b1; b.bn_s = w.bn_s; b.bn_t = w.bn_t;
    b.pw2_b = w.pw2_b;
    b.pw1_w = ring(w.pw1_wp); b.pc_w1 = ring(w.pc_w1p); b.pw2_w = ring(w.pw2_wp);
    b.ln_g = w.ln_g; b.ln_b = w.ln_b;
    if (!b.qkv_w || !b.out_w || !b.pw1_w || !b.pc_w1 || !b.pw2_w || w.xq_wp) return false;
  }
  return true;
}

int encoder_impl(mi355asr_model* m, const float* wav, const Geometry& g, const Plan& p, char* ws, float* enc_out,
                 hipStream_t s, const int32_t* wav_len, int32_t* enc_len) {
  // add_wav_info: the residual stacks reflect-pad their input by two rows (wav_model.py:57-104), and tf.pad(..., "REFLECT")
  // is defined for pad < size only -- below three frames the reference has no value, and the padded copies of run_wavpick
  // outgrow their carve.  Refused before anything is launched.
  if (m->cfg.add_wav_info && g.T < kWavMinFrames) {
    const int per = m->dm.hop * m->cfg.reduction_factor;
    return fail(MI355ASR_EINVAL, "add_wav_info: %d samples per %s give %d frames, the waveform branch's reflect padding needs at least "
                "%d (a minimum length of %d samples)", g.Lb, m->cfg.chunk_size > 0 ? "chunk" : "utterance", g.T, kWavMinFrames,
                (kWavMinFrames - 1) * per + 1);
  }
  float* logp = (float*)(ws + p.logp);
  float* mel = (float*)(ws + p.mel);
  int rc = run_mel(m, wav, g.Bp, g.Lb, g.F, logp, (float*)(ws + p.pmax), (float*)(ws + p.umax), mel, s, wav_len);
  if (rc) return rc;
  // ragged batches: the encoder frames of every utterance, into the words of the utterance maxima (read by the mel launch
  // above, free from here on) and the caller's enc_len
  int32_t* t_len = wav_len ? (int32_t*)(ws + p.umax) : nullptr;
  if (wav_len) LAUNCH_TRY(launch_ragged_frames(wav_len, g.Bp, m->dm.hop, m->dm.st1, t_len, enc_len, s), "ragged frame counts");
  Scratch sc = make_scratch(p, ws);
  // round 4: the subsampling Dense rides in the first block's ff_module_1 + qkv launch when both run on the two-term stream
  const int nb = m->cfg.num_blocks;
  bool dense_deferred = false;
  const bool may_defer = nb > 0 && !m->cfg.add_wav_info && block_takes_pre(m, m->enc_blocks[0], (size_t)g.Bp * g.T);
  rc = run_subsampling(m, mel, g.Bp, g.F, (float*)(ws + p.sub), sc.xa, s, true, may_defer ? &dense_deferred : nullptr, wav_len);
  if (rc) return rc;
  if (m->cfg.add_wav_info) {
    rc = run_wavpick(m, wav, g.Bp, g.Lb, g.T, sc.xa, (float*)(ws + p.wv), s);
    if (rc) return rc;
  }
  // round 5: the streaming shapes (bf16 mode, dmodel 256, chunks of <= 16 rows): the whole block stack as ONE launch, one workgroup
  // per chunk (stream256.hip) -- MI355ASR_STREAM256=0: one launch per layer / module as before
  {
    S256Args sa{};
    if (stream256_args(m, g.Bp, g.T, sc.xa, enc_out, sa)) {
      PROF(MI355ASR_K_ENC_STACK);
      if (launch_stream256(sa, s) == 0) {          // -1 (not its shape after all): the per-layer loop below runs instead
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MI355ASR_EHIP, "launch encoder block stack: %s", hipGetErrorString(e));
        return 0;
      }
    }
  }
  bool ff1_done = false;
  for (int i = 0; i < nb; ++i) {
    BlockOpts bo;
    bo.ksz = m->cfg.kernel_size;
    bo.fc = m->cfg.fc_factor;
    bo.t_len = t_len;
    if (i == 0 && dense_deferred) { bo.pre_x = (float*)(ws + p.sub); bo.pre_pp = m->lin_pp; bo.pre_sw = m->lin_pp_sw; bo.pre_chunks = m->dm.F2; }
    const bool skip = ff1_done;
    rc = run_block(m, m->enc_blocks[i], bo, sc, g.Bp, g.T, i == nb - 1 ? enc_out : nullptr, s, nullptr,
                   i + 1 < nb ? &m->enc_blocks[i + 1] : nullptr, &ff1_done, skip);
    if (rc) return rc;
  }
  if (nb == 0) HIP_TRY(hipMemcpyAsync(enc_out, sc.xa, (size_t)g.Bp * g.T * m->cfg.dmodel * 4, hipMemcpyDeviceToDevice, s));
  if (t_len) {
    const int d = m->cfg.dmodel;
    LAUNCH_TRY(launch_ragged_rows(t_len, g.Bp, g.T, enc_out, d, d, nullptr, s), "ragged encoder rows");
  }
  return 0;
}

int ctc_impl(mi355asr_model* m, const float* enc, int B, int T, const Plan& p, char* ws, float* logits,
             int32_t* amax, hipStream_t s, const int32_t* t_len, const int32_t* t_len_host = nullptr) {
  const StackDev& st = m->ctc;
  const int d = m->cfg.dmodel, nb = (int)st.blocks.size();
  // ragged batches: the rows past each utterance's frames get defined values once the head has run
  auto ragged_out = [&]() -> int {
    if (t_len) {
      const int V = st.num_classes;
      LAUNCH_TRY(launch_ragged_rows(t_len, B, T, logits, V, V, amax ? amax : (int32_t*)(ws + p.amax), s), "ragged CTC rows");
    }
    return 0;
  };
  const int M = B * T;
  Scratch sc = make_scratch(p, ws);
  const bool bf16 = gemm16_for(m, M);
  // round 4: the projection rides in the first decoder block's ff_module_1 + qkv launch
  const bool proj_fold = st.proj_pp && nb > 0 && block_takes_pre(m, st.blocks[0], (size_t)M);
  if (proj_fold) {
    // (nothing here: the first block below computes it)
  } else if (bf16) {
    Gemm16Args pr{};
    pr.x = enc; pr.ldx = d; pr.bias = st.proj_b; pr.y = sc.xa; pr.ldy = d;
    pr.M = M; pr.K = d; pr.NT = d / 16; pr.n_valid = d; pr.eps = kLnEps;
    { PROF(MI355ASR_K_CTC_PROJECT); LAUNCH_TRY(launch_gemm16(m, E16_BIAS, false, pr, st.proj_wp, s), "ctc project"); }
  } else {
    // on its own: the same two-term stream through pp_sublinear_kernel (one chunk) -- bit-identical to the folded form --, else fp32 MFMA
    if (int rc = run_rows_project(m, st, enc, sc.xa, M, s, st.proj_pp && m->cfg.gemm_dtype == 0)) return rc;
  }
  // round 4: the class head rides in the last block's tail launch where pp_head_kernel would have run (run_class_head's conditions);
  // the launch does not read hd.x: the block's output never leaves the chip
  const GemmArgs hd = head_args(st, sc.xa, M, logits, amax ? amax : (int32_t*)(ws + p.amax));
  bool head_done = false;
  const auto head_it = (!bf16 && m->cfg.gemm_dtype == 0 && M >= 2048) ? m->head_of.find(st.fc_wp) : m->head_of.end();
  // (no `next` / ff1_done chaining between decoder blocks, unlike encoder_impl and the ChunkConformer's run_stack)
  for (int i = 0; i < nb; ++i) {
    BlockOpts bo = st.opts;
    bo.t_len = t_len;
    bo.t_len_host = t_len_host;
    if (i == 0 && proj_fold) { bo.pre_x = enc; bo.pre_pp = st.proj_pp; bo.pre_sw = st.proj_pp_sw; bo.pre_chunks = 1; }
    if (i == nb - 1 && head_it != m->head_of.end() && head_it->second.pp) {
      bo.head = &hd; bo.head_pp = head_it->second.pp; bo.head_sw = head_it->second.pp_sw; bo.head_groups = head_it->second.groups; bo.head_done = &head_done;
    }
    int rc = run_block(m, st.blocks[i], bo, sc, B, T, nullptr, s);
    if (rc) return rc;
  }
  if (head_done) return ragged_out();
  // (the hidden buffer of the ff modules, M x 4 d floats, planned whenever gemm16_for(m, M), is free here: per-range winners of
  // a layer-at-a-time head split over class ranges)
  GemmArgs h = hd;
  h.x = sc.xa;                                         // (the blocks swap sc.xa / sc.xb)
  if (int rc = run_class_head(m, h, HeadLayers::first, nullptr, sc.h4, h.argmax_out, s)) return rc;
  return ragged_out();                                 // (the class head is row-wise: only the rows past T_b need their values)
}



}  // namespace mi355

// =======================================================================================================
// C ABI
// =======================================================================================================
thread_local int mi355asr_last_scheme = SCHEME_F32;   // launch.h: note_scheme

// mi355asr_test_split_f16: the shared two-term operand split (common.h: split_hi_f16 / split_lo_f16) on an array, pair by pair as the kernels apply it --
// element 2 i goes through the low half (v_fma_mixlo_f16), element 2 i + 1 through the high half (v_fma_mixhi_f16)
__global__ void split_f16_probe_kernel(const float* __restrict__ x, int64_t n, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
  const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const bool two = i + 1 < n;
  const float a = x[i], b = two ? x[i + 1] : 0.f;
  const unsigned h = split_hi_f16(a, b), l = split_lo_f16(h, a, b);
  hi[i] = (uint16_t)(h & 0xffffu);
  lo[i] = (uint16_t)(l & 0xffffu);
  if (two) {
    hi[i + 1] = (uint16_t)(h >> 16);
    lo[i + 1] = (uint16_t)(l >> 16);
  }
}
// mi355asr_test_split_bf16: the shared exact three-term operand split (mfma_ops.h: split8) on an array, pair by pair -- elements
// 2 i and 2 i + 1 are k-slots 0 and 1 of a fragment (the low and the high half of dword 0 of every term)
__global__ void split_bf16_probe_kernel(const float* __restrict__ x, int64_t n, uint16_t* __restrict__ t0, uint16_t* __restrict__ t1,
                                        uint16_t* __restrict__ t2) {
  const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const bool two = i + 1 < n;
  const Split8x3 f = split8(f32x4{x[i], two ? x[i + 1] : 0.f, 0.f, 0.f}, splat4(0.f));
  uint16_t* const out[3] = {t0, t1, t2};
#pragma unroll
  for (int term = 0; term < 3; ++term) {
    out[term][i] = (uint16_t)(f.t[term].x & 0xffffu);
    if (two) out[term][i + 1] = (uint16_t)(f.t[term].x >> 16);
  }
}

extern "C" {

const char* mi355asr_last_error(void) { return g_err; }
const char* mi355asr_version(void) { return "mi355asr 0.1 (gfx950, fp32 operands as fp16 pairs / bf16 triples on the MFMA pipe)"; }

int mi355asr_test_split_f16(const float* x_dev, int64_t n, uint16_t* hi_dev, uint16_t* lo_dev, void* stream) {
  if (!x_dev || !hi_dev || !lo_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (n < 1 || n > (int64_t)1 << 31) return fail(MI355ASR_EINVAL, "test_split_f16: need 1 <= n <= 2^31 (got %lld)", (long long)n);
  const int64_t pairs = (n + 1) / 2;
  hipLaunchKernelGGL(split_f16_probe_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, n, hi_dev, lo_dev);
  return hipGetLastError() == hipSuccess ? MI355ASR_OK : fail(MI355ASR_EHIP, "test_split_f16: launch failed");
}

int mi355asr_test_split_bf16(const float* x_dev, int64_t n, uint16_t* t0_dev, uint16_t* t1_dev, uint16_t* t2_dev, void* stream) {
  if (!x_dev || !t0_dev || !t1_dev || !t2_dev) return fail(MI355ASR_EINVAL, "null pointer");
  if (n < 1 || n > (int64_t)1 << 31) return fail(MI355ASR_EINVAL, "test_split_bf16: need 1 <= n <= 2^31 (got %lld)", (long long)n);
  const int64_t pairs = (n + 1) / 2;
  hipLaunchKernelGGL(split_bf16_probe_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, n, t0_dev, t1_dev,
                     t2_dev);
  return hipGetLastError() == hipSuccess ? MI355ASR_OK : fail(MI355ASR_EHIP, "test_split_bf16: launch failed");
}

int mi355asr_create(const mi355asr_config* cfg, mi355asr_model** out) {
  if (!cfg || !out) return fail(MI355ASR_EINVAL, "null argument");
  mi355asr_config c = *cfg;
  // the plain Spectrogram layer feeds all n_dft / 2 + 1 dB bins to the subsampling convs: from here on they are the
  // "mel" axis of every shape (n_mels of the config is not used by that layer, conformer_blocks.py:318-323)
  if (c.mel_layer_type == 2) c.n_mels = c.n_dft / 2 + 1;
  if (c.dmodel != 144 && (c.dmodel % 128 != 0 || c.dmodel < 128 || c.dmodel > 1024))
    return fail(MI355ASR_EINVAL, "dmodel=%d: supported are 144 (ConformerS), 256 (ConformerM / StreamingS) and other multiples of 128 up to 1024 (512 = ConformerL)", c.dmodel);
  if (c.num_heads * c.head_size != c.dmodel)
    return fail(MI355ASR_EINVAL, "num_heads*head_size (%d*%d) must equal dmodel (%d)", c.num_heads, c.head_size, c.dmodel);
  // round 6: the reference's constructors take any head size / kernel size (conformer_blocks.py:278-294); outside the shipped YAMLs'
  // values (36 / 64, 32 / 5) the block runs on slower general kernels instead of failing (attention_kernel<HS, ...>, dwconv_any_kernel)
  if (!attention_head_size_ok(c.head_size))
    return fail(MI355ASR_EINVAL, "head_size=%d: attention kernels are instantiated for 12, 16, 24, 32, 36, 48, 64, 72 and 128", c.head_size);
  if (c.kernel_size < 1 || c.kernel_size > 1024)
    return fail(MI355ASR_EINVAL, "kernel_size=%d: must be in 1 .. 1024", c.kernel_size);
  if (c.num_classes > 0 && (c.ctc_kernel_size < 1 || c.ctc_kernel_size > 1024))
    return fail(MI355ASR_EINVAL, "ctc_kernel_size=%d: must be in 1 .. 1024", c.ctc_kernel_size);
  if (c.reduction_factor != 2 && c.reduction_factor != 4 && c.reduction_factor != 6 && c.reduction_factor != 8)
    return fail(MI355ASR_EINVAL, "reduction_factor=%d: 2, 4, 6 or 8 (conv1 time stride 1 .. 4)", c.reduction_factor);
  if (c.mel_layer_type < 0 || c.mel_layer_type > 2)
    return fail(MI355ASR_EINVAL, "mel_layer_type=%d: 0 (Melspectrogram), 1 (leaf) or 2 (Spectrogram)", c.mel_layer_type);
  if (c.mel_layer_type == 1 && (c.n_mels != 80 || c.stride_ms * c.sample_rate / 1000 != 160 || c.sample_rate != 16000))
    return fail(MI355ASR_EINVAL, "leaf frontend: instantiated for 80 filters, 16 kHz, 10 ms stride (window 401, hop 160)");
  if (c.gemm_dtype != 0 && c.gemm_dtype != 1) return fail(MI355ASR_EINVAL, "gemm_dtype=%d: 0 (fp32 MFMA) or 1 (bf16 MFMA)", c.gemm_dtype);
  if (c.n_dft != 1024) return fail(MI355ASR_EINVAL, "n_dft=%d: the reference hard-codes 1024 (conformer_blocks.py:312)", c.n_dft);
  if (c.mel_layer_type != 2 && c.n_mels != 80 && c.n_mels != 128)
    return fail(MI355ASR_EINVAL, "n_mels=%d: mel kernel instantiated for 80 and 128", c.n_mels);
  if (c.num_blocks < 0 || c.ctc_num_blocks < 0 || c.chunk_size < 0 || c.num_classes < 0)
    return fail(MI355ASR_EINVAL, "negative count in config");
  auto* m = new mi355asr_model();
  m->cfg = c;
  {
    const int t = (int)mi355_env("MI355ASR_LEAF_TERMS", -1);   // 0 = fp32 MFMA Gabor conv; 2 / 3 = bf16 terms per operand
    if (t == 0 || t == 2 || t == 3) m->leaf_terms = t;
  }
  Dims& dm = m->dm;
  dm.hop = c.stride_ms * c.sample_rate / 1000;
  if (dm.hop <= 0) { delete m; return fail(MI355ASR_EINVAL, "stride_ms*sample_rate/1000 must be positive"); }
  dm.nbins = c.n_dft / 2 + 1;
  dm.NT_dft = ceil_div(2 * dm.nbins, 16);          // 65 tiles of (re,im)-interleaved columns
  dm.NT_dft = ceil_div(dm.NT_dft, 13) * 13;
  dm.NCH_dft = dm.NT_dft / 13;
  dm.LP = ceil_div(8 * dm.NT_dft, 16) * 16;        // log-power row stride (bins), 16-byte aligned rows
  dm.KBm = ceil_div(ceil_div(dm.nbins, 16), 2) * 2;   // sweep_k consumes k-blocks in pairs (zero-padded)
  dm.NTm = c.n_mels / 16;
  dm.st1 = c.reduction_factor / 2;
  same_pad(c.n_mels, 3, 2, &dm.F1, &dm.pf1);
  same_pad(dm.F1, 3, 2, &dm.F2, &dm.pf2);
  const int d = c.dmodel;
  auto& ex = m->expected;
  if (c.has_encoder && c.mel_layer_type == 1) {
    // leaf_audio.frontend.Leaf variables (frontend.py:106-160)
    ex.push_back({"mel_layer/tfbanks_preemp/kernel", {2, 1, 1}});
    ex.push_back({"mel_layer/tfbanks_complex_conv/kernel", {c.n_mels, 2}});
    ex.push_back({"mel_layer/learnable_pooling/kernel", {1, 1, c.n_mels, 1}});
    for (const char* n : {"alpha", "delta", "root"}) ex.push_back({std::string("mel_layer/PCEN/") + n, {c.n_mels}});
    ex.push_back({"mel_layer/PCEN/EMA/smooth", {c.n_mels}});
    ex.push_back({"mel_layer/tfbanks_instancenorm/gamma", {c.n_mels}});
    ex.push_back({"mel_layer/tfbanks_instancenorm/beta", {c.n_mels}});
  }
  if (c.has_encoder) {
    if (c.mel_layer_type != 1) {
    ex.push_back({"mel_layer/real_kernels", {c.n_dft, 1, 1, dm.nbins}});
    ex.push_back({"mel_layer/imag_kernels", {c.n_dft, 1, 1, dm.nbins}});
    if (c.mel_layer_type == 0) ex.push_back({"mel_layer/freq2mel", {dm.nbins, c.n_mels}});
    }
    ex.push_back({"conv_subsampling/conv1/kernel", {3, 3, 1, d}});
    ex.push_back({"conv_subsampling/conv1/bias", {d}});
    ex.push_back({"conv_subsampling/conv2/kernel", {3, 3, d, d}});
    ex.push_back({"conv_subsampling/conv2/bias", {d}});
    ex.push_back({"conv_subsampling/linear/kernel", {dm.F2 * d, d}});
    ex.push_back({"conv_subsampling/linear/bias", {d}});
    for (int i = 0; i < c.num_blocks; ++i)
      add_block_expected(ex, "conformer_block_" + std::to_string(i), d, c.num_heads, c.head_size, c.kernel_size);
  }
  if (c.add_wav_info != 0 && c.add_wav_info != 1) { delete m; return fail(MI355ASR_EINVAL, "add_wav_info=%d: 0 or 1", c.add_wav_info); }
  if (c.has_encoder && c.add_wav_info) {
    // WavePickModel(dmodel, hop_size * reduction_factor) (conformer_blocks.py:329-331, wav_model.py:108-131)
    const std::vector<int> scales = wave_pick_scales(dm.hop * c.reduction_factor);
    if (scales.size() != 4) { delete m; return fail(MI355ASR_EINVAL, "add_wav_info: hop_size*reduction_factor=%d does not factor into four strides", dm.hop * c.reduction_factor); }
    m->wp_stride0 = scales[0];
    ex.push_back({"wav_layer/sep_conv/depthwise_kernel", {7, 1, 1}});
    ex.push_back({"wav_layer/sep_conv/pointwise_kernel", {1, 1, 32}});
    ex.push_back({"wav_layer/sep_conv/bias", {32}});
    int cin = 32;
    for (int i = 1; i < 4; ++i) {
      const int ch = std::min(32 * (i + 1), d);
      mi355asr_model::WavStage st{};
      st.cin = cin; st.c = ch; st.stride = scales[i];
      m->wp_stages.push_back(st);
      const std::string n = std::to_string(i);
      ex.push_back({"wav_layer/conv_" + n + "/kernel", {3, cin, ch}});
      ex.push_back({"wav_layer/conv_" + n + "/bias", {ch}});
      ex.push_back({"wav_layer/res_" + n + "/conv5/kernel", {5, ch, ch}});
      ex.push_back({"wav_layer/res_" + n + "/conv5/bias", {ch}});
      ex.push_back({"wav_layer/res_" + n + "/conv1/kernel", {1, ch, ch}});
      ex.push_back({"wav_layer/res_" + n + "/conv1/bias", {ch}});
      ex.push_back({"wav_layer/res_" + n + "/shortcut/kernel", {1, ch, ch}});
      ex.push_back({"wav_layer/res_" + n + "/shortcut/bias", {ch}});
      cin = ch;
    }
    ex.push_back({"wav_layer/final/kernel", {7, cin, d}});
    ex.push_back({"wav_layer/final/bias", {d}});
  }
  if (c.num_classes > 0)
    add_stack_expected(ex, "", "decoder_conformer_block_", c.ctc_num_blocks, d, c.num_heads, c.head_size, c.ctc_kernel_size, true, c.num_classes, false);
  *out = m;
  return 0;
}

int mi355asr_profile_schemes(const mi355asr_model* m, int32_t* scheme_out, int32_t n) {
  if (!m || !scheme_out || n < MI355ASR_NUM_KERNELS)
    return fail(MI355ASR_EINVAL, "profile_schemes needs an array of at least %d entries", MI355ASR_NUM_KERNELS);
  for (int i = 0; i < MI355ASR_NUM_KERNELS; ++i) scheme_out[i] = m->prof_scheme[i];
  return 0;
}

int mi355asr_profile_enable(mi355asr_model* m, int32_t on) {
  if (!m) return fail(MI355ASR_EINVAL, "null model handle");
  m->prof = on != 0;
  return 0;
}

int mi355asr_profile_read(mi355asr_model* m, double* ms_out, int64_t* count_out, int32_t n, int32_t reset) {
  if (!m || !ms_out || !count_out || n < MI355ASR_NUM_KERNELS)
    return fail(MI355ASR_EINVAL, "profile_read needs arrays of at least %d entries", MI355ASR_NUM_KERNELS);
  for (auto& p : m->ev_pending) {
    HIP_TRY(hipEventSynchronize(p.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p.e0, p.e1));
    m->prof_ms[p.cat] += ms;
    m->prof_cnt[p.cat] += 1;
    m->ev_free.push_back(p.e0);
    m->ev_free.push_back(p.e1);
  }
  m->ev_pending.clear();
  for (int i = 0; i < MI355ASR_NUM_KERNELS; ++i) {
    ms_out[i] = m->prof_ms[i];
    count_out[i] = m->prof_cnt[i];
    if (reset) { m->prof_ms[i] = 0; m->prof_cnt[i] = 0; }
  }
  return 0;
}

int mi355asr_destroy(mi355asr_model* m) {
  if (!m) return 0;
  for (auto& p : m->ev_pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
  for (auto e : m->ev_free) (void)hipEventDestroy(e);
  if (m->arena) (void)hipFree(m->arena);
  if (m->arena16) (void)hipFree(m->arena16);
  delete m;
  return 0;
}

int mi355asr_stft_mode(const mi355asr_model* m) {
  if (!m || !m->finalized || (!m->is_chunk && !m->cfg.has_encoder)) return -1;
  if (!m->is_chunk && m->cfg.mel_layer_type == 1) return -1;     // LEAF frontend: no STFT
  return m->fft_ok ? 1 : 0;
}

}  // extern "C"

// ---- entry points: a solo call is a ragged call without lengths ------------------------------------------------------------
namespace mi355 {
// what the ragged entry points support: the Melspectrogram frontend on the FFT STFT, offline encoder, fp32 mode, dmodel 144
int ragged_config_ok(const mi355asr_model* m) {
  const auto& c = m->cfg;
  const char* why = c.mel_layer_type == 1 ? "the LEAF frontend"
                  : c.mel_layer_type != 0 ? "the Spectrogram layer"
                  : c.chunk_size > 0      ? "the streaming encoder (chunk_size > 0)"
                  : c.add_wav_info        ? "add_wav_info"
                  : c.gemm_dtype != 0     ? "the bf16 GEMM mode"
                  : c.dmodel != 144       ? "dmodel other than 144"
                  : m->dm.st1 != 2        ? "reduction_factor other than 4"
                  : !m->fft_ok            ? "the dense DFT STFT (stft_mode 0)"
                                          : nullptr;
  if (why) return fail(MI355ASR_EINVAL, "ragged batches do not support %s", why);
  // the kernels that apply lengths at dmodel 144: attention_split_kernel (head size 36) and the depthwise conv of 32 taps
  if (c.num_blocks > 0 && c.head_size != 36)
    return fail(MI355ASR_EINVAL, "ragged batches do not support head_size %d: the length-aware attention kernels of dmodel 144 are "
                "instantiated for head_size 36", c.head_size);
  if (c.num_blocks > 0 && c.kernel_size != 32)
    return fail(MI355ASR_EINVAL, "ragged batches do not support kernel_size %d: the depthwise conv kernels that apply lengths take "
                "kernel_size 32", c.kernel_size);
  return 0;
}
// the length-aware attention kernels take more than 16 rows per utterance (queries and keys): checked before anything is launched
int ragged_rows_ok(int T, const char* what) {
  if (T <= 16)
    return fail(MI355ASR_EINVAL, "ragged batches: %s = %d rows per utterance, the length-aware attention kernels need more than 16 "
                "(pad the batch: a row of more than 16 * reduction_factor * hop samples)", what, T);
  return 0;
}
// the ragged CTC decoder / Translator at dmodel 256: 64-dim heads on the layer-at-a-time launches (fp32: the slab-ring packs
// exist, i.e. MI355ASR_GEMM_RING on and the expected rows not set below the ring kernels' crossover; bf16: always)
int ragged_layers256_ok(const mi355asr_model* m, int ksz) {
  if (m->cfg.dmodel != 256 || m->cfg.head_size != 64)
    return fail(MI355ASR_EINVAL, "ragged batches do not support dmodel other than 144, and 256 with 64-dim heads (dmodel %d, head size %d)",
                m->cfg.dmodel, m->cfg.head_size);
  if (ksz != 32)
    return fail(MI355ASR_EINVAL, "ragged batches at dmodel 256 need a ConvModule kernel size of 32: the depthwise conv kernels that "
                "apply lengths (kernel size %d)", ksz);
  if (!use_gemm16(m))
    return fail(MI355ASR_EINVAL, "ragged batches at dmodel 256 need the layer-at-a-time launches: the slab-ring packs are missing "
                "(MI355ASR_GEMM_RING=0, or expected rows below the ring kernels' crossover)");
  return 0;
}
// the lengths are device words: read them once (this synchronises the stream) and check 1 <= len[b] <= hi
int ragged_check_lengths(const int32_t* len_dev, int B, int hi, const char* what, hipStream_t s, std::vector<int32_t>* host) {
  if (!len_dev) return fail(MI355ASR_EINVAL, "%s: null device pointer", what);
  std::vector<int32_t> own;
  std::vector<int32_t>& h = host ? *host : own;
  h.assign((size_t)B, 0);
  HIP_TRY(hipMemcpyAsync(h.data(), len_dev, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b)
    if (h[b] < 1 || h[b] > hi) return fail(MI355ASR_EINVAL, "%s[%d] = %d lies outside [1, %d]", what, b, h[b], hi);
  return 0;
}

// The checks in front of every call that runs the frontend or the encoder on B waveforms of L samples, in the order the
// entry points have always made them; on success the call's geometry and workspace plan.  ragged: also the ragged-only
// checks, wav_len being the lengths the caller handed in.
static int encoder_call_ok(const mi355asr_model* m, bool need_ctc, bool ptrs_ok, int B, int L, size_t ws_bytes, bool ragged,
                           const int32_t* wav_len, hipStream_t s, Geometry* g, Plan* p) {
  int rc = check_ready(m, true);
  if (rc) return rc;
  if (need_ctc && m->cfg.num_classes <= 0) return fail(MI355ASR_ESTATE, "model was created without a CTC head (num_classes=0)");
  if (ragged && (rc = ragged_config_ok(m))) return rc;
  // ... and the CTC decoder's blocks behind the encoder (recognize): the same two kernels
  if (ragged && need_ctc && m->cfg.ctc_num_blocks > 0 && m->cfg.head_size != 36)
    return fail(MI355ASR_EINVAL, "ragged batches do not support head_size %d: the length-aware attention kernels of dmodel 144 are "
                "instantiated for head_size 36", m->cfg.head_size);
  if (ragged && need_ctc && m->cfg.ctc_num_blocks > 0 && m->cfg.ctc_kernel_size != 32)
    return fail(MI355ASR_EINVAL, "ragged batches do not support ctcdecoder_kernel_size %d: the depthwise conv kernels that apply lengths "
                "take kernel_size 32", m->cfg.ctc_kernel_size);
  if (!ptrs_ok) return fail(MI355ASR_EINVAL, "null device pointer");
  if ((rc = geometry(m, B, L, g))) return rc;
  if (ragged && (rc = ragged_rows_ok(g->T, "T(L)"))) return rc;
  *p = make_plan(m, g->Bp, g->F, g->T);
  if (ws_bytes < p->total) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p->total);
  return ragged ? ragged_check_lengths(wav_len, B, L, "wav_len", s) : 0;
}

static int encoder_forward(mi355asr_model* m, const float* wav, bool ragged, const int32_t* wav_len, int B, int L, float* enc_out,
                           int32_t* enc_len, void* ws, size_t ws_bytes, hipStream_t s) {
  Geometry g;
  Plan p;
  if (int rc = encoder_call_ok(m, false, wav && enc_out && ws, B, L, ws_bytes, ragged, wav_len, s, &g, &p)) return rc;
  return encoder_impl(m, wav, g, p, (char*)ws, enc_out, s, wav_len, enc_len);
}

static int ctc_forward(mi355asr_model* m, const float* enc, bool ragged, const int32_t* enc_len, int B, int T, float* logits,
                       int32_t* amax, void* ws, size_t ws_bytes, hipStream_t s) {
  int rc = check_ready(m);
  if (rc) return rc;
  if (m->cfg.num_classes <= 0) return fail(MI355ASR_ESTATE, "model was created without a CTC head (num_classes=0)");
  if (ragged && m->cfg.dmodel == 144 && m->cfg.gemm_dtype != 0)
    return fail(MI355ASR_EINVAL, "ragged batches do not support the bf16 GEMM mode at dmodel 144");
  if (ragged && m->cfg.dmodel != 144 && (rc = ragged_layers256_ok(m, m->cfg.ctc_kernel_size))) return rc;
  if (!enc || !ws || B <= 0 || T <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  if (ragged && (rc = ragged_rows_ok(T, "T"))) return rc;
  const Plan p = make_plan(m, B, 16, T);
  if (ws_bytes < p.logp) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.logp);
  std::vector<int32_t> len_host;
  if (ragged && (rc = ragged_check_lengths(enc_len, B, T, "enc_len", s, &len_host))) return rc;
  return ctc_impl(m, enc, B, T, p, (char*)ws, logits, amax, s, enc_len, ragged ? len_host.data() : nullptr);
}

static int recognize(mi355asr_model* m, const float* wav, bool ragged, const int32_t* wav_len, int B, int L, const int32_t* in_len,
                     int32_t* ids, int32_t* out_len, void* ws, size_t ws_bytes, hipStream_t s) {
  Geometry g;
  Plan p;
  if (int rc = encoder_call_ok(m, true, wav && ids && out_len && ws, B, L, ws_bytes, ragged, wav_len, s, &g, &p)) return rc;
  char* w = (char*)ws;
  float* enc = (float*)(w + p.enc);
  if (int rc = encoder_impl(m, wav, g, p, w, enc, s, wav_len, nullptr)) return rc;
  const int Ttot = g.T * g.nblk;
  const int32_t* t_len = wav_len ? (const int32_t*)(w + p.umax) : nullptr;          // written by encoder_impl
  int32_t* amax = (int32_t*)(w + p.amax);
  if (int rc = ctc_impl(m, enc, B, Ttot, p, w, nullptr, amax, s, t_len)) return rc;
  CollapseArgs ca{amax, in_len, ids, out_len, B, Ttot, m->cfg.num_classes - 1};
  ca.t_len = t_len;
  { PROF(MI355ASR_K_COLLAPSE); LAUNCH_TRY(launch_collapse(ca, s), "ctc collapse"); }
  return 0;
}
}  // namespace mi355

extern "C" {

int mi355asr_out_frames(const mi355asr_model* m, int32_t L, int32_t* mel_frames, int32_t* enc_frames) {
  if (!m) return fail(MI355ASR_EINVAL, "null model handle");
  Geometry g;
  int rc = geometry(m, 1, L, &g);
  if (rc) return rc;
  if (mel_frames) *mel_frames = g.F * g.nblk;
  if (enc_frames) *enc_frames = g.T * g.nblk;
  return 0;
}

int mi355asr_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes) {
  if (!m || !bytes) return fail(MI355ASR_EINVAL, "null argument");
  Geometry g;
  int rc = geometry(m, B, L, &g);
  if (rc) return rc;
  *bytes = make_plan(m, g.Bp, g.F, g.T).total;
  return 0;
}

// (the CTC decoder and a single block use the buffers the plan places in front of the log-power spectrum)
int mi355asr_ctc_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes) {
  if (!m || !bytes || B <= 0 || T <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  *bytes = make_plan(m, B, 16, T).logp;
  return 0;
}

int mi355asr_encoder_forward(mi355asr_model* m, const float* wav, int32_t B, int32_t L, float* enc_out, void* ws,
                             size_t ws_bytes, void* stream) {
  return encoder_forward(m, wav, false, nullptr, B, L, enc_out, nullptr, ws, ws_bytes, (hipStream_t)stream);
}
int mi355asr_encoder_forward_ragged(mi355asr_model* m, const float* wav, const int32_t* wav_len, int32_t B, int32_t L,
                                    float* enc_out, int32_t* enc_len, void* ws, size_t ws_bytes, void* stream) {
  return encoder_forward(m, wav, true, wav_len, B, L, enc_out, enc_len, ws, ws_bytes, (hipStream_t)stream);
}

int mi355asr_ctc_forward(mi355asr_model* m, const float* enc, int32_t B, int32_t T, float* logits, int32_t* amax,
                         void* ws, size_t ws_bytes, void* stream) {
  return ctc_forward(m, enc, false, nullptr, B, T, logits, amax, ws, ws_bytes, (hipStream_t)stream);
}
int mi355asr_ctc_forward_ragged(mi355asr_model* m, const float* enc, const int32_t* enc_len, int32_t B, int32_t T,
                                float* logits, int32_t* amax, void* ws, size_t ws_bytes, void* stream) {
  return ctc_forward(m, enc, true, enc_len, B, T, logits, amax, ws, ws_bytes, (hipStream_t)stream);
}

int mi355asr_recognize(mi355asr_model* m, const float* wav, int32_t B, int32_t L, const int32_t* in_len, int32_t* ids,
                       int32_t* out_len, void* ws, size_t ws_bytes, void* stream) {
  return recognize(m, wav, false, nullptr, B, L, in_len, ids, out_len, ws, ws_bytes, (hipStream_t)stream);
}
int mi355asr_recognize_ragged(mi355asr_model* m, const float* wav, const int32_t* wav_len, int32_t B, int32_t L,
                              const int32_t* in_len, int32_t* ids, int32_t* out_len, void* ws, size_t ws_bytes, void* stream) {
  return recognize(m, wav, true, wav_len, B, L, in_len, ids, out_len, ws, ws_bytes, (hipStream_t)stream);
}

int mi355asr_ctc_greedy(const int32_t* frame_argmax, const int32_t* in_len, int32_t B, int32_t T, int32_t blank,
                        int32_t* ids, int32_t* out_len, void* stream) {
  if (!frame_argmax || !ids || !out_len || B <= 0 || T <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  CollapseArgs ca{frame_argmax, in_len, ids, out_len, B, T, blank};
  LAUNCH_TRY(launch_collapse(ca, (hipStream_t)stream), "ctc collapse");
  return 0;
}

int mi355asr_melspectrogram(mi355asr_model* m, const float* wav, int32_t B, int32_t L, float* mel, void* ws,
                            size_t ws_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  Geometry g;
  Plan p;
  if (int rc = encoder_call_ok(m, false, wav && mel && ws, B, L, ws_bytes, false, nullptr, s, &g, &p)) return rc;
  char* w = (char*)ws;
  return run_mel(m, wav, g.Bp, g.Lb, g.F, (float*)(w + p.logp), (float*)(w + p.pmax), (float*)(w + p.umax), mel, s);
}

int mi355asr_conv_subsampling(mi355asr_model* m, const float* mel, int32_t B, int32_t F, float* out, void* ws,
                              size_t ws_bytes, void* stream) {
  int rc = check_ready(m, true);
  if (rc) return rc;
  if (!mel || !out || !ws || B <= 0 || F <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  const int T = ceil_div(ceil_div(F, m->dm.st1), 2);
  const Plan p = make_plan(m, B, F, T);
  if (ws_bytes < p.total) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.total);
  return run_subsampling(m, mel, B, F, (float*)((char*)ws + p.sub), out, (hipStream_t)stream, false, nullptr, nullptr);
}

int mi355asr_conformer_block(mi355asr_model* m, int32_t stack, int32_t index, const float* x, int32_t B, int32_t T,
                             float* y, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_ready(m);
  if (rc) return rc;
  if (!x || !y || !ws || B <= 0 || T <= 0) return fail(MI355ASR_EINVAL, "bad argument");
  const auto& blocks = stack == 0 ? m->enc_blocks : m->ctc.blocks;
  if (stack < 0 || stack > 1 || index < 0 || index >= (int)blocks.size())
    return fail(MI355ASR_EINVAL, "no block %d in stack %d", index, stack);
  const Plan p = make_plan(m, B, 16, T);
  if (ws_bytes < p.logp) return fail(MI355ASR_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, p.logp);
  hipStream_t s = (hipStream_t)stream;
  Scratch sc = make_scratch(p, (char*)ws);
  HIP_TRY(hipMemcpyAsync(sc.xa, x, (size_t)B * T * m->cfg.dmodel * 4, hipMemcpyDeviceToDevice, s));
  BlockOpts bo;
  bo.ksz = stack == 0 ? m->cfg.kernel_size : m->cfg.ctc_kernel_size;
  bo.fc = stack == 0 ? m->cfg.fc_factor : m->cfg.ctc_fc_factor;
  return run_block(m, blocks[index], bo, sc, B, T, y, s);
}

}  // extern "C"

