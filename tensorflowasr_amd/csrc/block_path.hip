// Which kernels run a Conformer block, its attention and a class head.  This file reads every switch of those paths, once,
// into BlockSwitches, and decides; the launchers in fused*.hip, blocks.hip and attention_split*.hip check only shapes.
// DESIGN.md §3 lists the switches and what each selects.
#include "model.h"

const BlockSwitches& block_switches() {
  static const BlockSwitches w = [] {
    BlockSwitches v;
    v.fused = mi355_env("MI355ASR_FUSED", 1) != 0;                    // 0: dmodel 144 one fp32 launch per layer
    v.gemm16 = mi355_env("MI355ASR_GEMM16", 0) != 0;                  // 1: layer-at-a-time gemm16 kernels for every row count
    v.small_m = mi355_env("MI355ASR_SMALL_M", 48);                    // rows up to which the layer-at-a-time kernels run
    v.pp = mi355_env("MI355ASR_PP", 1) != 0;                          // 0: the three-term loader-wave kernels (fused.hip)
    v.pp_outglu = mi355_env("MI355ASR_PP_OUTGLU", 1) != 0;            // 0: three-term out_glu_ld_kernel
    v.pp_head = mi355_env("MI355ASR_PP_HEAD", 1) != 0;                // 0: three-term head_ld_kernel
    v.pp_dw = mi355_env("MI355ASR_PP_DW", 1) != 0;                    // 0: depthwise conv as its own launch
    v.pp_ogf = mi355_env("MI355ASR_PP_OGF", 1) != 0;                  // 0: out-projection + GLU as its own launch
    v.pp_pre = mi355_env("MI355ASR_PP_PRE", 1) != 0;                  // 0: the layer in front of a block as its own launch
    v.pp_headf = mi355_env("MI355ASR_PP_HEADF", 1) != 0;              // 0: the class head as its own launch
    v.tail_ff1 = mi355_env("MI355ASR_TAIL_FF1", 1) != 0;              // 0: a block's tail and the next ff_module_1 as two launches
    v.head_ring = mi355_env("MI355ASR_HEAD_RING", 1) != 0;            // 0: the fp32-MFMA class head (gemm_rows<EPI_HEAD>)
    v.qkv_head_major = mi355_env("MI355ASR_QKV_HEAD_MAJOR", 1) != 0;  // 0: q / k / v as token-major rows
    v.ns1_max_m = (int)mi355_env("MI355ASR_NS1_MAX_M", 4096);         // rows up to which the fused_ns.hip kernels run
    v.ns1_attn = mi355_env("MI355ASR_NS1_ATTN", 1) != 0;              // 0: a small-batch block's attention as its own launch
    v.attn_split = mi355_env("MI355ASR_ATTN_SPLIT", 1) != 0;          // 0: fp32-MFMA attention_lds_kernel
    v.attn_lds = mi355_env("MI355ASR_ATTN_LDS", 1) != 0;              // 0: online-softmax attention_kernel (K / V from L2)
    v.attn_three = mi355_env("MI355ASR_ATTN_TERMS", -1) == 3;         // 3: three-term attention_split_kernel
    v.attn64_split = mi355_env("MI355ASR_ATTN64_SPLIT", 1) != 0;      // 0: head size 64 on the fp32-MFMA kernels
    v.attn_long = mi355_env("MI355ASR_ATTN_LONG", 1) != 0;            // 0: more than 256 keys on the fp32-MFMA kernels
    v.chain256 = mi355_env("MI355ASR_CHAIN256", 1) != 0;              // 0: bf16 dmodel 256, one launch per dense layer
    return v;
  }();
  return w;
}

// short full-attention utterances: K / V staged in LDS, on the two-term split kernel where the operand bounds are known
AttnChoice choose_attention(int HS, const AttnArgs& a) {
  const BlockSwitches& w = block_switches();
  const bool split_on = w.attn_lds && w.attn_split;
  AttnChoice c;
  if (split_on && attention_split_applicable(HS, a) && (a.Tk <= ATTN_SPLIT_SHORT_KEYS || w.attn_long)) {
    c.terms = !w.attn_three && attention_split_two_term_fits(a) ? 2 : 3;
    if (a.head_major && (c.terms != 2 || a.ldq != HS || a.ldk != HS)) return AttnChoice{};
    c.kernel = a.Tk > ATTN_SPLIT_SHORT_KEYS ? ATTN_SPLIT_LONG : ATTN_SPLIT;
    return c;
  }
  if (a.k_len) {                                      // ragged batches: the split kernels apply key lengths, and at head size 64
    // (token-major rows, full attention) every kernel of the solo call does, each for the utterances it would take alone
    if (HS == 64 && a.win_front < 0 && !a.head_major && a.ldk % 4 == 0 && a.ldq % 4 == 0) c.kernel = ATTN_RAGGED64;
    // band attention (token-major rows, any head size): the online-softmax kernel with the utterance's length as the band's T
    else if (a.win_front >= 0 && !a.head_major && attention_head_size_ok(HS)) { c.kernel = ATTN_ONLINE; c.band_lengths = true; }
    return c;
  }
  if (split_on && w.attn64_split && attention_split64_applicable(HS, a)) {   // round 5: head size 64, bounds known, <= 288 keys
    c.kernel = ATTN_SPLIT64;
    c.terms = 2;
    return c;
  }
  if (a.head_major) return c;                         // head-major q / k / v: attention_split_kernel only
  if (w.attn_lds && attention_lds_applicable(HS, a)) c.kernel = ATTN_LDS;
  else if (attention_head_size_ok(HS)) c.kernel = ATTN_ONLINE;
  return c;
}

// what choose_attention allows a solo call of head size 64 with these operands (the arguments of attn64_class)
int attn64_flags(const AttnArgs& a) {
  const BlockSwitches& w = block_switches();
  int f = 0;
  if (w.attn_lds && w.attn_split && w.attn64_split && a.h2_sq > 0.f && a.h2_sk > 0.f && a.h2_sv > 0.f) f |= ATTN64_F_SPLIT64;
  if (w.attn_lds) f |= ATTN64_F_LDS;
  return f;
}

namespace mi355 {

// a launcher the plan picked declined: the plan and the launcher's shape checks disagree
#define PLANNED(expr, what)                                                                 \
  do {                                                                                      \
    if ((expr) != 0) return fail(MI355ASR_ESTATE, "block plan: the %s launcher declined", what); \
    hipError_t e__ = hipGetLastError();                                                     \
    if (e__ != hipSuccess) return fail(MI355ASR_EHIP, "launch %s: %s", what, hipGetErrorString(e__)); \
  } while (0)

// Layer-at-a-time GEMM family (bf16.hip) instead of the fused / chained fp32 kernels: in bf16 mode, and in fp32 for
// dmodel values those kernels are not instantiated for (e.g. 512 = ConformerL).
bool use_gemm16(const mi355asr_model* m) {
  // dmodel 256 with slab rings (gemm_ring.hip): one launch per dense layer on the split-bf16 pipe beats the fp32 chains
  return block_switches().gemm16 || m->cfg.gemm_dtype == 1 || (m->cfg.dmodel != 144 && m->cfg.dmodel != 256) ||
         (m->cfg.dmodel == 256 && !m->ring_of.empty());
}
// Very few rows (one streaming chunk of 13 frames, the Translator's token stream): the fused kernels give each 16-row tile
// to ONE wave that walks a whole run of layers serially -- a fused launch takes as long for 16 rows as for 16 000 -- and one
// launch per layer with K / column splitting is as fast.  From a few tiles on the fused path wins: round 4 measured ONE
// utterance (ms per recognize(), fused vs layer-at-a-time) 10 s / 250 rows 1.234 vs 1.386, 5 s / 125 rows 1.143 vs 1.263,
// 2 s / 50 rows 1.118 vs 1.224, and B = 2, 3 at 10 s 1.241 / 1.252 vs 1.513 / 1.651 (profiles/r04_batch_sweep.md; the
// round-2 ring kernels had crossed at ~800 rows, which is where this threshold stood until round 4).  MI355ASR_SMALL_M overrides.
bool gemm16_for(const mi355asr_model* m, size_t M) { return use_gemm16(m) || (long)M <= block_switches().small_m; }

bool block_takes_pre(const mi355asr_model* m, const BlockDev& w, size_t M) {
  const BlockSwitches& sw = block_switches();
  return m->cfg.dmodel == 144 && sw.fused && !gemm16_for(m, M) && w.pp_ff1 && w.ff1_slabs && sw.pp && sw.pp_pre;
}

// ---- the arguments of a block's layers and token-mixing steps: every walker below, and those of api_chunk.hip, fill them here
// FFModule i: y = x + fc * FFN(LN(x)), behind ff_module_2 also the block's final LayerNorm
Chain2Args ff_module_args(const BlockDev& w, const BlockOpts& bo, int i, const float* x, float* y, int M, bool block_ln) {
  Chain2Args a{};
  a.x = x; a.res = x; a.y = y;
  a.ln_g = w.ff_ln_g[i]; a.ln_b = w.ff_ln_b[i];
  a.w1p = w.ff_w1p[i]; a.b1 = w.ff_b1[i]; a.w2p = w.ff_w2p[i]; a.b2 = w.ff_b2[i];
  if (block_ln) { a.fln_g = w.ln_g; a.fln_b = w.ln_b; }
  a.scale = bo.fc; a.eps = kLnEps; a.M = M;
  return a;
}
// y = res + pw2( swish( BN( dw Wpc + bpc ) ) ) + b2
Chain2Args conv_tail_args(const BlockDev& w, const float* dw, const float* res, float* y, int M) {
  Chain2Args a{};
  a.x = dw; a.res = res; a.y = y;
  a.w1p = w.pc_w1p; a.b1 = w.pc_b1; a.aff_s = w.bn_s; a.aff_t = w.bn_t; a.w2p = w.pw2_wp; a.b2 = w.pw2_b;
  a.scale = 1.0f; a.eps = kLnEps; a.M = M;
  return a;
}
// a gemm_rows layer of `wide` x dmodel columns of which the first `kept` x dmodel are stored, densely; ln_g: LayerNorm in front
static GemmArgs rows_layer_args(const mi355asr_model* m, const float* x, float* y, const float* wp, const float* bias, int M, int wide,
                                int kept, const float* ln_g = nullptr, const float* ln_b = nullptr, bool qscale = false) {
  const int d = m->cfg.dmodel;
  GemmArgs g{};
  g.x = x; g.y = y; g.ln_g = ln_g; g.ln_b = ln_b; g.wp = wp; g.bias = bias;
  g.M = M; g.NT = wide * d / 16; g.ldy = kept * d; g.n_valid = kept * d; g.eps = kLnEps;
  if (qscale) { g.qscale = 1.0f / std::sqrt((float)m->cfg.head_size); g.qtiles = d / 16; }   // q pre-scaled by 1 / sqrt(hs)
  return g;
}
// qkv = LN(x) Wqkv
GemmArgs qkv_args(const mi355asr_model* m, const BlockDev& w, const float* x, float* qkv, int M) {
  return rows_layer_args(m, x, qkv, w.qkv_wp, w.qkv_b, M, 3, 3, w.att_ln_g, w.att_ln_b, true);
}
// the Translator's RBlock: q = LN(x) Wq  [M, d] ; [k | v] = enc [Wk | Wv]  [B * T_enc, 2 d]  (qkv_b: 3 d zeros, no bias)
GemmArgs cross_q_args(const mi355asr_model* m, const BlockDev& w, const float* x, float* q, int M) {
  return rows_layer_args(m, x, q, w.xq_wp, w.qkv_b, M, 1, 1, w.att_ln_g, w.att_ln_b, true);
}
GemmArgs cross_kv_args(const mi355asr_model* m, const BlockDev& w, const CrossAttn& c, int B) {
  return rows_layer_args(m, c.enc, c.kv, w.xkv_wp, w.qkv_b, B * c.T_enc, 2, 2);
}
// y = res + ctx Wo + bo
GemmArgs attn_out_args(const mi355asr_model* m, const BlockDev& w, const float* ctx, const float* res, float* y, int M) {
  GemmArgs g = rows_layer_args(m, ctx, y, w.out_wp, w.out_b, M, 1, 1);
  g.res = res;
  return g;
}
// u = GLU(LN(x) Wpw1 + b)
GemmArgs glu_args(const mi355asr_model* m, const BlockDev& w, const float* x, float* u, int M) {
  return rows_layer_args(m, x, u, w.pw1_wp, w.pw1_b, M, 2, 1, w.cv_ln_g, w.cv_ln_b);
}
DwArgs dw_args(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, const float* u, float* y, int B, int T) {
  DwArgs a{};
  a.u = u; a.y = y; a.wd = w.dw_w; a.B = B; a.T = T; a.D = m->cfg.dmodel;
  // Keras 'same', stride 1: total k-1, before = (k-1)//2 ; 'causal': all k-1 on the left
  a.pad_left = bo.causal ? bo.ksz - 1 : (bo.ksz - 1) / 2;
  return a;
}
static AttnArgs attn_args_base(const mi355asr_model* m, const BlockOpts& bo, float* ctx, int B, int T) {
  AttnArgs at{};
  at.ctx = ctx; at.B = B; at.Tq = T; at.H = m->cfg.num_heads; at.D = m->cfg.dmodel;
  at.win_front = bo.win_front; at.win_back = bo.win_back;
  return at;
}
AttnArgs self_attn_args(const mi355asr_model* m, const BlockOpts& bo, const float* qkv, float* ctx, int B, int T) {
  const int d = m->cfg.dmodel;
  AttnArgs at = attn_args_base(m, bo, ctx, B, T);
  at.q = qkv; at.k = qkv + d; at.v = qkv + 2 * d; at.ldq = 3 * d; at.ldk = 3 * d; at.Tk = T;
  return at;
}
AttnArgs cross_attn_args(const mi355asr_model* m, const BlockOpts& bo, const float* q, int ldq, const CrossAttn& c, float* ctx, int B, int T) {
  const int d = m->cfg.dmodel;
  AttnArgs at = attn_args_base(m, bo, ctx, B, T);
  at.q = q; at.ldq = ldq; at.k = c.kv; at.v = c.kv + d; at.ldk = 2 * d; at.Tk = c.T_enc;
  return at;
}

// ---- stack-level launches on the rows kernels
int run_rows_project(const mi355asr_model* m, const StackDev& st, const float* x, float* y, int M, hipStream_t s, bool try_pp) {
  const int d = m->cfg.dmodel;
  PROF(MI355ASR_K_CTC_PROJECT);
  if (try_pp) {
    StreamGemmArgs sp{};
    sp.x = x; sp.y = y; sp.M = M; sp.K = d; sp.NT = d / 16; sp.ldy = d; sp.n_valid = d;
    if (launch_pp_sublinear(sp, st.proj_pp, st.proj_pp_sw, s) == 0) return 0;
  }
  LAUNCH_TRY(launch_gemm_rows(d, EPI_BIAS, false, rows_layer_args(m, x, y, st.proj_wp, st.proj_b, M, 1, 1), s), "project");
  return 0;
}
int run_rows_head(const mi355asr_model* m, const StackDev& st, const float* x, int M, float* logits, int32_t* argmax, hipStream_t s) {
  PROF(MI355ASR_K_CTC_HEAD);
  LAUNCH_TRY(launch_gemm_rows(m->cfg.dmodel, EPI_HEAD, false, head_args(st, x, M, logits, argmax), s), "fully_connected");
  return 0;
}
void subconv_weights(const mi355asr_model* m, SubConvArgs& sa, bool split) {
  sa.w1 = m->c1_w; sa.b1 = m->c1_b; sa.w2p = m->c2_wp; sa.b2 = m->c2_b;
  if (split) sa.w2s = m->c2_wsplit;
}
StreamGemmArgs sublinear_args(const mi355asr_model* m, const float* x, float* y, int M) {
  const int d = m->cfg.dmodel;
  StreamGemmArgs lg{};
  lg.x = x; lg.y = y; lg.wp = m->lin_wp; lg.bias = m->lin_b;
  lg.M = M; lg.K = m->dm.F2 * d; lg.NT = d / 16; lg.ldy = d; lg.n_valid = d;
  return lg;
}

// one launch per dense layer (bf16.hip: bf16 or fp32 operands); LayerNorm / softmax / activations / depthwise conv in fp32
static int run_block_layers(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, Scratch& sc, int B, int T,
                            float* out, hipStream_t s, const CrossAttn* cross) {
  const int d = m->cfg.dmodel, hs = m->cfg.head_size, ksz = bo.ksz, M = B * T;
  const float fc = bo.fc;
  auto g16 = [&](const float* x, int ldx, int K, const float* wp, const float* bias, int NT, float* y, int ldy) {
    Gemm16Args g{};
    g.x = x; g.ldx = ldx; g.K = K; g.wp = wp; g.bias = bias; g.NT = NT; g.y = y; g.ldy = ldy;
    g.M = M; g.n_valid = 16 * NT; g.eps = kLnEps; g.scale = 1.0f;
    return g;
  };
  // round 4: bf16 mode, dmodel 256: FFModule and ConvModule tail as ONE launch each (bf16.hip: chain256_bf16_kernel; the
  // hidden activation stays in LDS) -- MI355ASR_CHAIN256=0: one gemm16 / gemm_ring launch per layer
  auto ring = [&](const float* wp) -> const float* { const auto it = m->ring_of.find(wp); return it == m->ring_of.end() ? nullptr : it->second; };
  const float* cr[6] = {ring(w.ff_w1p[0]), ring(w.ff_w2p[0]), ring(w.ff_w1p[1]), ring(w.ff_w2p[1]), ring(w.pc_w1p), ring(w.pw2_wp)};
  const bool chain256 = m->cfg.gemm_dtype == 1 && d == 256 && block_switches().chain256 && !cross && cr[0] && cr[1] && cr[2] && cr[3] && cr[4] && cr[5];
  auto ffn = [&](int i, const float* x, float* y, const float* fg, const float* fb) -> int {
    if (chain256) {
      Chain2Args ca = ff_module_args(w, bo, i, x, y, M, fg != nullptr);
      ca.w1p = cr[2 * i]; ca.w2p = cr[2 * i + 1];
      PROF(MI355ASR_K_FFN); LAUNCH_TRY(launch_chain256_bf16(0, ca, s), "ff module");
      return 0;
    }
    Gemm16Args a1 = g16(x, d, d, w.ff_w1p[i], w.ff_b1[i], 4 * d / 16, sc.h4, 4 * d);
    a1.ln_g = w.ff_ln_g[i]; a1.ln_b = w.ff_ln_b[i];
    { PROF(MI355ASR_K_FFN); LAUNCH_TRY(launch_gemm16(m, E16_SWISH, true, a1, w.ff_w1p[i], s), "ffn1"); }
    Gemm16Args a2 = g16(sc.h4, 4 * d, 4 * d, w.ff_w2p[i], w.ff_b2[i], d / 16, y, d);
    a2.res = x; a2.scale = fc; a2.fln_g = fg; a2.fln_b = fb;
    { PROF(MI355ASR_K_FFN); LAUNCH_TRY(launch_gemm16(m, E16_RES, false, a2, w.ff_w2p[i], s), "ffn2"); }
    return 0;
  };
  int rc = ffn(0, sc.xa, sc.xb, nullptr, nullptr);
  if (rc) return rc;
  AttnArgs at = cross ? cross_attn_args(m, bo, sc.qkv, d, *cross, sc.ctx, B, T) : self_attn_args(m, bo, sc.qkv, sc.ctx, B, T);
  if (cross) {
    // RBlock: q = (LN(xb + PE) Wq) / sqrt(hs) ; [k | v] = enc [Wk | Wv]
    AddPeArgs pa{sc.xb, cross->pe, sc.u, B, T, d};
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_add_pe(pa, s), "positional encoding"); }
    Gemm16Args q = g16(sc.u, d, d, w.xq_wp, w.qkv_b, d / 16, sc.qkv, d);
    q.ln_g = w.att_ln_g; q.ln_b = w.att_ln_b; q.qscale = 1.0f / std::sqrt((float)hs); q.qtiles = d / 16;
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm16(m, E16_QKV, true, q, w.xq_wp, s), "cross-attention query projection"); }
    Gemm16Args kv = g16(cross->enc, d, d, w.xkv_wp, w.qkv_b, 2 * d / 16, cross->kv, 2 * d);
    kv.M = B * cross->T_enc;
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm16(m, E16_BIAS, false, kv, w.xkv_wp, s), "cross-attention key/value projection"); }
  } else {
    Gemm16Args q = g16(sc.xb, d, d, w.qkv_wp, w.qkv_b, 3 * d / 16, sc.qkv, 3 * d);
    q.ln_g = w.att_ln_g; q.ln_b = w.att_ln_b; q.qscale = 1.0f / std::sqrt((float)hs); q.qtiles = d / 16;
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm16(m, E16_QKV, true, q, w.qkv_wp, s), "qkv"); }
    at.h2_sq = w.att_h2[0]; at.h2_sk = w.att_h2[1]; at.h2_sv = w.att_h2[2];      // q / k / v are the block's own projections (0: no bound known)
  }
  if (bo.t_len) {
    at.k_len = cross ? cross->k_len : bo.t_len;
    at.q_len = bo.t_len;                                 // the utterance's own queries: its frames, or its tokens
    at.q_len_host = bo.t_len_host;
    at.k_len_host = cross ? cross->k_len_host : bo.t_len_host;
    if (!at.k_len || !choose_attention(hs, at).applies_lengths())
      return fail(MI355ASR_EINVAL, "ragged batches: no length-aware attention kernel for Tq = %d, Tk = %d", at.Tq, at.Tk);
  }
  { PROF(MI355ASR_K_ATTN); LAUNCH_TRY(launch_attention(hs, at, s), "attention"); }
  Gemm16Args op = g16(sc.ctx, d, d, w.out_wp, w.out_b, d / 16, sc.xa, d);
  op.res = sc.xb;
  { PROF(MI355ASR_K_ATTN_OUT); LAUNCH_TRY(launch_gemm16(m, E16_RES, false, op, w.out_wp, s), "attention out"); }
  Gemm16Args gl = g16(sc.xa, d, d, w.pw1_wp, w.pw1_b, 2 * d / 16, sc.u, d);
  gl.ln_g = w.cv_ln_g; gl.ln_b = w.cv_ln_b; gl.n_valid = d;
  { PROF(MI355ASR_K_PW1_GLU); LAUNCH_TRY(launch_gemm16(m, E16_GLU, true, gl, w.pw1_wp, s), "pw_conv_1 + GLU"); }
  DwArgs dwa = dw_args(m, w, bo, sc.u, sc.dw, B, T);
  dwa.t_len = bo.t_len;
  { PROF(MI355ASR_K_DWCONV); LAUNCH_TRY(launch_dwconv(ksz, dwa, s), "depthwise conv"); }
  if (chain256) {
    Chain2Args ca = conv_tail_args(w, sc.dw, sc.xa, sc.xb, M);
    ca.w1p = cr[4]; ca.w2p = cr[5];
    { PROF(MI355ASR_K_CONV_TAIL); LAUNCH_TRY(launch_chain256_bf16(1, ca, s), "conv module tail"); }
    return ffn(1, sc.xb, out ? out : sc.xa, w.ln_g, w.ln_b);
  }
  Gemm16Args pc = g16(sc.dw, d, d, w.pc_w1p, w.pc_b1, 2 * d / 16, sc.h4, 2 * d);
  pc.aff_s = w.bn_s; pc.aff_t = w.bn_t;
  { PROF(MI355ASR_K_CONV_TAIL); LAUNCH_TRY(launch_gemm16(m, E16_AFFSWISH, false, pc, w.pc_w1p, s), "pointwise + BN + swish"); }
  Gemm16Args p2 = g16(sc.h4, 2 * d, 2 * d, w.pw2_wp, w.pw2_b, d / 16, sc.xb, d);
  p2.res = sc.xa;
  { PROF(MI355ASR_K_CONV_TAIL); LAUNCH_TRY(launch_gemm16(m, E16_RES, false, p2, w.pw2_wp, s), "pw_conv_2"); }
  return ffn(1, sc.xb, out ? out : sc.xa, w.ln_g, w.ln_b);
}

// MI355ASR_FUSED=0 (and the Translator's RBlock under MI355ASR_PP=0): walk_block_rows (model.h) with attention and depthwise
// conv over the B x T rows
static int run_block_rows(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, Scratch& sc, int B, int T,
                          float* out, hipStream_t s, const CrossAttn* cross) {
  const int d = m->cfg.dmodel, hs = m->cfg.head_size, M = B * T;
  auto qkv_rows = [&](RowsOf& r) -> int {
    if (!cross) return 0;
    // q of LN(xb + PE), k / v of the encoder output: made here, the walker's own qkv launch is left out
    AddPeArgs pa{sc.xb, cross->pe, sc.u, B, T, d};
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_add_pe(pa, s), "positional encoding"); }
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm_rows(d, EPI_QKV, true, cross_q_args(m, w, sc.u, sc.qkv, M), s), "cross-attention query projection"); }
    { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm_rows(d, EPI_BIAS, false, cross_kv_args(m, w, *cross, B), s), "cross-attention key/value projection"); }
    r.x = nullptr;
    return 0;
  };
  auto attend = [&]() -> int {
    const AttnArgs at = cross ? cross_attn_args(m, bo, sc.qkv, d, *cross, sc.ctx, B, T) : self_attn_args(m, bo, sc.qkv, sc.ctx, B, T);
    PROF(MI355ASR_K_ATTN); LAUNCH_TRY(launch_attention(hs, at, s), "attention");
    return 0;
  };
  auto depthwise = [&]() -> int {
    // (no t_len: run_block never sends a ragged batch to this walker)
    PROF(MI355ASR_K_DWCONV); LAUNCH_TRY(launch_dwconv(bo.ksz, dw_args(m, w, bo, sc.u, sc.dw, B, T), s), "depthwise conv");
    return 0;
  };
  return walk_block_rows(m, w, bo, sc, M, out, s, qkv_rows, attend, own_rows, depthwise);
}

// What run_block_fused launches for one block, decided before anything is launched.
enum class Ff1Kernel { none, ns1, pp, pp_pre, ld };   // ff_module_1 + qkv (none: the previous block's tail launch ran it)
enum class TailKernel { ns1, pp_og_ff1, pp_og_ff2, pp_og_ff2_head, pp_ff1, pp_ff2, ld_ff1, ld_ff2 };
struct BlockPlan {
  Ff1Kernel ff1 = Ff1Kernel::none;
  AttnChoice attn;
  bool attn_in_ns1 = false;   // the attention runs inside the ns1 out-projection launch (else attn is its own launch)
  bool og_own = false;        // out-projection + GLU as its own launch: og_pp ? pp_out_glu_kernel : out_glu_ld_kernel
  bool og_pp = false;
  bool dw_own = false;        // depthwise conv as its own launch
  bool dw_fold = false;       // ... else in the prologue of the pair-pipelined tail kernel (or of the ns1 tail)
  TailKernel tail = TailKernel::ld_ff2;
  bool next_ff1 = false;      // the tail launch also runs ff_module_1 + qkv of the next block
};

// dmodel 144: token-local runs of layers in one launch each (fused*.hip); attention and the depthwise conv mix tokens
static int run_block_fused(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, Scratch& sc, int B, int T,
                           float* out, hipStream_t s, const CrossAttn* cross, const BlockDev* next, bool* ff1_done, bool skip_ff1) {
  const BlockSwitches& sw = block_switches();
  const int d = m->cfg.dmodel, H = m->cfg.num_heads, hs = m->cfg.head_size, ksz = bo.ksz, M = B * T;
  const float fc = bo.fc, qscale = 1.0f / std::sqrt((float)hs);
  // round 5: q / k / v of a block travel head-major ([B, H, T, 36] planes) whenever their producer is a pair-pipelined kernel and
  // their consumer the two-term attention_split_kernel -- a pure function of the shapes, the switches and the block's weights, so
  // the producer (this block's own ff_module_1 launch, or the previous block's tail) and the consumer agree without a flag
  // being passed between launches.  MI355ASR_QKV_HEAD_MAJOR=0: token-major rows as before.
  auto attn_args = [&](const BlockDev& bw, bool hm) {
    AttnArgs at = self_attn_args(m, bo, sc.qkv, sc.ctx, B, T);
    if (hm) { at.k = sc.qkv + (size_t)M * d; at.v = sc.qkv + 2 * (size_t)M * d; at.ldq = hs; at.ldk = hs; at.head_major = 1; }
    at.h2_sq = bw.att_h2[0]; at.h2_sk = bw.att_h2[1]; at.h2_sv = bw.att_h2[2];      // q / k / v are the block's own projections
    at.k_len = bo.t_len;
    return at;
  };
  auto qkv_head_major = [&](const BlockDev& bw) {
    return sw.qkv_head_major && !cross && sw.pp && choose_attention(hs, attn_args(bw, true)).head_major();
  };
  auto ff1_args = [&](const BlockDev& bw, const float* x0, float* x1) {
    Ff1QkvArgs k1{};
    k1.x0 = x0; k1.x1 = x1; k1.qkv = sc.qkv;
    k1.ff_ln_g = bw.ff_ln_g[0]; k1.ff_ln_b = bw.ff_ln_b[0]; k1.ff_w1p = bw.ff_w1p[0]; k1.ff_b1 = bw.ff_b1[0];
    k1.ff_w2p = bw.ff_w2p[0]; k1.ff_b2 = bw.ff_b2[0];
    k1.att_ln_g = bw.att_ln_g; k1.att_ln_b = bw.att_ln_b; k1.qkv_wp = bw.qkv_wp; k1.qkv_b = bw.qkv_b;
    k1.fc = fc; k1.qscale = qscale; k1.eps = kLnEps; k1.M = M; k1.slabs = bw.ff1_slabs; k1.pp_slabs = bw.pp_ff1; k1.pp_sc = bw.pp_ff1_sc; k1.pp_sw_qkv = bw.pp_sw_qkv;
    k1.ns_w1 = bw.ns_ff1_w1; k1.ns_w2 = bw.ns_ff1_w2; k1.ns_qkv = bw.ns_qkv;
    if (qkv_head_major(bw)) { k1.qkv_T = T; k1.qkv_H = H; }
    return k1;
  };

  // ---- the launches' arguments
  Ff1QkvArgs k1 = ff1_args(w, sc.xa, sc.xb);
  if (bo.pre_pp) { k1.pre_x = bo.pre_x; k1.pre_pp = bo.pre_pp; k1.pre_sw = bo.pre_sw; k1.pre_chunks = bo.pre_chunks; }
  if (cross) { k1.xq_pe = cross->pe; k1.xq_U = T; }
  AttnArgs at = attn_args(w, k1.qkv_T > 0);
  GemmArgs kv{};
  if (cross) {
    // [k | v] = enc [Wk | Wv]  [B * T_enc, 2 d]; q sits at columns 0..143 of the [M, 3 d] rows the ff_module_1 launch wrote
    kv = cross_kv_args(m, w, *cross, B);
    at = cross_attn_args(m, bo, sc.qkv, 3 * d, *cross, sc.ctx, B, T);   // no operand bounds for the encoder's rows: three exact terms
    at.k_len = bo.t_len ? cross->k_len : nullptr;             // ragged batches: the keys are the utterance's encoder frames
  }
  OutGluArgs k2{};
  k2.ctx = sc.ctx; k2.x1 = sc.xb; k2.x2 = sc.xa; k2.u = sc.u;
  k2.out_wp = w.out_wp; k2.out_b = w.out_b; k2.cv_ln_g = w.cv_ln_g; k2.cv_ln_b = w.cv_ln_b;
  k2.pw1_wp = w.pw1_wp; k2.pw1_b = w.pw1_b; k2.eps = kLnEps; k2.M = M;
  k2.og_slabs = w.og_slabs; k2.pp_slabs = w.pp_og; k2.pp_sw_out = w.pp_sw_out; k2.pp_sw_pw1 = w.pp_sw_pw1;
  k2.ns_out = w.ns_out; k2.ns_pw1 = w.ns_pw1;
  DwArgs dwa = dw_args(m, w, bo, sc.u, sc.dw, B, T);
  dwa.t_len = bo.t_len;
  TailFf2Args k4{};
  k4.dw = sc.dw; k4.x2 = sc.xa; k4.y = out ? out : sc.xb;
  k4.pc_w1p = w.pc_w1p; k4.pc_b1 = w.pc_b1; k4.bn_s = w.bn_s; k4.bn_t = w.bn_t; k4.pw2_wp = w.pw2_wp; k4.pw2_b = w.pw2_b;
  k4.ff_ln_g = w.ff_ln_g[1]; k4.ff_ln_b = w.ff_ln_b[1]; k4.ff_w1p = w.ff_w1p[1]; k4.ff_b1 = w.ff_b1[1];
  k4.ff_w2p = w.ff_w2p[1]; k4.ff_b2 = w.ff_b2[1]; k4.ln_g = w.ln_g; k4.ln_b = w.ln_b;
  k4.fc = fc; k4.eps = kLnEps; k4.M = M; k4.slabs = w.tail_slabs; k4.pp_slabs = w.pp_tail; k4.pp_sc[0] = w.pp_tail_sc[0]; k4.pp_sc[1] = w.pp_tail_sc[1];
  k4.ns_cv_w1 = w.ns_cv_w1; k4.ns_cv_w2 = w.ns_cv_w2; k4.ns_ff_w1 = w.ns_ff2_w1; k4.ns_ff_w2 = w.ns_ff2_w2;
  k4.dw_len = bo.t_len;
  TailFf2Args kd = k4;                                         // ... with the depthwise conv in the tail kernel's prologue
  kd.dw_u = sc.u; kd.dw_wd = w.dw_w; kd.dw_T = T; kd.dw_pad = dwa.pad_left;
  const Ff1QkvArgs kn = next ? ff1_args(*next, nullptr, sc.xa) : Ff1QkvArgs{};

  // ---- the plan
  BlockPlan p;
  if (!skip_ff1) {
    if (bo.pre_pp) p.ff1 = Ff1Kernel::pp_pre;                 // (run_block: block_takes_pre)
    // round 6, small batches (up to MI355ASR_NS1_MAX_M rows): one 16-token tile per workgroup (fused_ns.hip)
    else if (sw.pp) p.ff1 = !cross && ns1_rows_ok(M) ? Ff1Kernel::ns1 : Ff1Kernel::pp;
    else p.ff1 = Ff1Kernel::ld;
  }
  p.attn = choose_attention(hs, at);
  // ragged batches: the attention, wherever it runs, must be a kernel that applies key lengths
  if (bo.t_len && !p.attn.applies_lengths())
    return fail(MI355ASR_EINVAL, "ragged batches: no length-aware attention kernel for T = %d (needs T > 16 and the split kernels: "
                "MI355ASR_ATTN_SPLIT / MI355ASR_ATTN_LDS on)", T);
  // round 3: the depthwise conv rides in the prologue of the pair-pipelined tail kernel (no launch, dw never in HBM); round 4:
  // so does out-projection + GLU (x2 and u never in HBM either): the block is attention + one launch
  p.dw_fold = sw.pp && sw.pp_dw && pp_dw_fold_fits(T, ksz);
  const bool og_fold = p.dw_fold && sw.pp_outglu && sw.pp_ogf && pp_og_fold_fits(kd, k2);
  // the block output feeds only the next block's ff_module_1: keep it in registers, write x1 (into the buffer the next block
  // knows as sc.xb after the swap -- this block's x2, which each workgroup has consumed) and qkv
  p.next_ff1 = next && !out && ff1_done && sw.tail_ff1;
  // round 4: the class head behind the CTC decoder's last block rides in the tail launch where pp_head_kernel would have run
  const bool head_fold = og_fold && !p.next_ff1 && bo.head && bo.head_pp && bo.head_done && sw.pp_headf && sw.pp_head && sw.head_ring &&
                         bo.head_groups >= 1 && bo.head->n_valid <= 144 * bo.head_groups;
  // The folded launches (OGF) read x1 from sc.xb, INCLUDING the halo frames of the neighbouring workgroups (the window of the
  // depthwise conv), so nothing in such a launch may write sc.xb: a workgroup that starts after its neighbour has stored the
  // block output there would read y as x1 (grids above one workgroup per CU).  x2 is never materialised in that mode, so sc.xa
  // is free: the block output goes there and the xa/xb swap is skipped.
  TailFf2Args kog = kd;
  if (!out) kog.y = sc.xa;
  // round 6, small batches: the folded block as [attention + out-projection + GLU] -> [depthwise conv + tail (+ the next block's
  // ff_module_1 + qkv)], where the folded pair-pipelined tail would run (its switches), at its own shape rule (16-frame tiles
  // waste little at any length).  x2 / u go to sc.xa / sc.u, which are free in that mode; every workgroup reads and writes its
  // own rows of sc.xa only.  The attention rides in the first launch where the two-term attention_split_kernel would run.
  TailFf2Args kt = p.next_ff1 ? kd : kog;
  if (p.next_ff1) kt.y = nullptr;
  const bool ns1 = sw.pp && sw.pp_outglu && sw.pp_ogf && sw.pp_dw && ksz == 32 && !head_fold && ns1_rows_ok(M) &&
                   ns1_block_ok(kt, p.next_ff1 ? &kn : nullptr, k2);
  if (ns1) {
    p.tail = TailKernel::ns1;
    p.attn_in_ns1 = p.attn.kernel == ATTN_SPLIT && p.attn.terms == 2 && sw.ns1_attn && ns1_attn_fits(hs, at);
  } else {
    p.og_own = !og_fold;
    p.og_pp = sw.pp && sw.pp_outglu;
    p.dw_own = !p.dw_fold;
    if (p.next_ff1) p.tail = og_fold ? TailKernel::pp_og_ff1 : sw.pp ? TailKernel::pp_ff1 : TailKernel::ld_ff1;
    else if (head_fold) p.tail = TailKernel::pp_og_ff2_head;
    else p.tail = og_fold ? TailKernel::pp_og_ff2 : sw.pp ? TailKernel::pp_ff2 : TailKernel::ld_ff2;
  }
  if (!p.attn_in_ns1 && p.attn.kernel == ATTN_NONE) return fail(MI355ASR_EINVAL, "no kernel instantiation for attention");

  // ---- the launches
  if (p.ff1 != Ff1Kernel::none) {
    PROF(MI355ASR_K_FF1_QKV);
    if (p.ff1 == Ff1Kernel::ns1) PLANNED(launch_ns1_ff1_qkv(k1, s), "ff_module_1 + qkv (ns1)");
    else if (p.ff1 == Ff1Kernel::ld) PLANNED(launch_ff1_qkv_ld(k1, s), "ff_module_1 + qkv (ld)");
    else PLANNED(launch_pp_ff1_qkv(k1, s), "ff_module_1 + qkv (pp)");
  }
  if (cross) { PROF(MI355ASR_K_QKV); LAUNCH_TRY(launch_gemm_rows(d, EPI_BIAS, false, kv, s), "cross-attention key/value projection"); }
  if (!p.attn_in_ns1) { PROF(MI355ASR_K_ATTN); PLANNED(launch_attention(hs, at, s), "attention"); }
  if (p.tail == TailKernel::ns1) {
    OutGluArgs kg = k2;
    if (p.attn_in_ns1) {
      kg.attn = 1; kg.aq = at.q; kg.ak = at.k; kg.av = at.v; kg.a_T = at.Tk; kg.a_H = at.H; kg.a_ldq = at.ldq; kg.a_ldk = at.ldk;
      kg.a_head_major = at.head_major; kg.a_sq = at.h2_sq; kg.a_sk = at.h2_sk; kg.a_sv = at.h2_sv; kg.a_klen = at.k_len;
    }
    if (p.next_ff1) {
      { PROF(MI355ASR_K_TAIL_FF1); PLANNED(launch_ns1_og_tail(kt, &kn, kg, s), "small-batch block + next ff_module_1"); }
      *ff1_done = true;
      std::swap(sc.xa, sc.xb);
    } else {
      PROF(MI355ASR_K_TAIL_FF2); PLANNED(launch_ns1_og_tail(kt, nullptr, kg, s), "small-batch block");      // y is in sc.xa (or `out`): no swap
    }
    return 0;
  }
  if (p.og_own) { PROF(MI355ASR_K_OUT_GLU); PLANNED(p.og_pp ? launch_pp_out_glu(k2, s) : launch_out_glu_ld(k2, s), "out-projection + GLU"); }
  if (p.dw_own) { PROF(MI355ASR_K_DWCONV); LAUNCH_TRY(launch_dwconv(ksz, dwa, s), "depthwise conv"); }
  TailFf2Args kf = p.dw_fold ? kd : k4;
  if (p.next_ff1) {
    kf.y = nullptr;
    {
      PROF(MI355ASR_K_TAIL_FF1);
      if (p.tail == TailKernel::pp_og_ff1) PLANNED(launch_pp_og_tail_ff1(kf, kn, k2, s), "out-projection + GLU + conv tail + ff_module_2 + next ff_module_1");
      else if (p.tail == TailKernel::pp_ff1) PLANNED(launch_pp_tail_ff1(kf, kn, s), "conv tail + ff_module_2 + next ff_module_1");
      else PLANNED(launch_tail_ff1_ld(kf, kn, s), "conv tail + ff_module_2 + next ff_module_1 (ld)");
    }
    *ff1_done = true;
    std::swap(sc.xa, sc.xb);
    return 0;
  }
  PROF(MI355ASR_K_TAIL_FF2);
  if (p.tail == TailKernel::pp_og_ff2_head) {
    // the block output itself is stored only if somebody asked for it
    TailFf2Args kh = kog;
    if (!out) kh.y = nullptr;
    kh.head_pp = bo.head_pp; kh.head_sw = bo.head_sw; kh.head_groups = bo.head_groups; kh.head_ldy = bo.head->ldy;
    kh.head_nvalid = bo.head->n_valid; kh.head_y = bo.head->y; kh.head_argmax = bo.head->argmax_out; kh.head_maxval = bo.head->maxval_out;
    PLANNED(launch_pp_og_tail_ff2(kh, k2, s), "block tail + class head");
    *bo.head_done = true;
    return 0;                                          // nothing was stored: the block's input stays where it was
  }
  if (p.tail == TailKernel::pp_og_ff2) {
    PLANNED(launch_pp_og_tail_ff2(kog, k2, s), "out-projection + GLU + conv tail + ff_module_2");
    return 0;                                          // y is in sc.xa (or `out`): no swap
  }
  if (p.tail == TailKernel::pp_ff2) PLANNED(launch_pp_tail_ff2(kf, s), "conv tail + ff_module_2");
  else PLANNED(launch_tail_ff2_ld(kf, s), "conv tail + ff_module_2 (ld)");
  if (!out) std::swap(sc.xa, sc.xb);
  return 0;
}

int run_block(const mi355asr_model* m, const BlockDev& w, const BlockOpts& bo, Scratch& sc, int B, int T, float* out,
              hipStream_t s, const CrossAttn* cross, const BlockDev* next, bool* ff1_done, bool skip_ff1) {
  if (ff1_done) *ff1_done = false;
  const BlockSwitches& sw = block_switches();
  const int d = m->cfg.dmodel, M = B * T;
  if (bo.pre_pp && (cross || skip_ff1 || !block_takes_pre(m, w, (size_t)M)))
    return fail(MI355ASR_ESTATE, "run_block: a layer in front of a block that cannot take it");
  // (ragged batches: the fused kernels, or the layer-at-a-time fp32 launches of at most MI355ASR_SMALL_M rows)
  // (... and dmodel 256 with 64-dim heads on the layer-at-a-time launches, fp32 or bf16: run_block_layers)
  const bool layers256 = d == 256 && m->cfg.head_size == 64 && use_gemm16(m);
  if (bo.t_len && !layers256 && (d != 144 || use_gemm16(m) || (!sw.fused && !gemm16_for(m, M))))
    return fail(MI355ASR_EINVAL, "ragged batches: only the fp32 dmodel-144 block kernels and the layer-at-a-time launches of "
                "dmodel 256 with 64-dim heads apply lengths (dmodel %d%s%s)", d,
                sw.fused ? "" : ", MI355ASR_FUSED=0", use_gemm16(m) ? ", bf16 / layer-at-a-time GEMM mode" : "");
  if (gemm16_for(m, M)) return run_block_layers(m, w, bo, sc, B, T, out, s, cross);
  // round 6: the Translator's RBlock takes the fused kernels too -- its query projection (of LayerNorm(x1 + PE)) rides in the
  // ff_module_1 launch of the pair-pipelined kernel, keys / values come from the encoder output through their own projection
  const bool fused_cross = cross && sw.pp && w.ff1_slabs && w.pp_ff1 && !bo.pre_pp && !skip_ff1 && !next;
  if (bo.t_len && cross && (!fused_cross || !cross->k_len))
    return fail(MI355ASR_EINVAL, "ragged batches: the Translator's cross-attention block needs the fused kernels and encoder lengths");
  if (d == 144 && sw.fused && (!cross || fused_cross)) return run_block_fused(m, w, bo, sc, B, T, out, s, cross, next, ff1_done, skip_ff1);
  return run_block_rows(m, w, bo, sc, B, T, out, s, cross);
}

int run_class_head(const mi355asr_model* m, GemmArgs hd, HeadLayers layers, float* split, float* part, int32_t* amax_scratch,
                   hipStream_t s) {
  const BlockSwitches& sw = block_switches();
  const int d = m->cfg.dmodel, M = hd.M;
  const bool on_layers = layers != HeadLayers::never && gemm16_for(m, (size_t)M);
  enum { NS1, PP_SPLIT, PP, LD, LAYERS, ROWS } k = ROWS;
  int ranges = 1;
  const auto it = m->cfg.gemm_dtype == 0 ? m->head_of.find(hd.wp) : m->head_of.end();
  const bool streams = it != m->head_of.end() && it->second.groups >= 1 && hd.n_valid <= 144 * it->second.groups;
  const bool pp = sw.pp && sw.pp_head && sw.head_ring;   // pp_head_kernel, and ns1_head_kernel standing in for it at few rows
  if (on_layers && layers == HeadLayers::first) k = LAYERS;
  else if (streams && pp && ns1_rows_ok(M)) k = NS1;     // round 6, small batches: one 16-token tile per workgroup
  else if (streams && M >= 2048) {                       // a launch of the ring kernels costs as much for 250 rows as for 16 000
    // few rows and many classes (the Translator's 144 -> 9160 over ~6 000 rows is 93 row workgroups): the column groups split
    // over several workgroups per row tile, the per-range arg-max pairs combined by a second small launch (split: 16 M words)
    const bool wants = hd.argmax_out || hd.maxval_out;
    if (pp && (split || !wants)) ranges = pp_head_ranges(M, it->second.groups);
    if (pp) k = ranges > 1 ? PP_SPLIT : PP;
    else if (sw.head_ring && hd.NT <= 9 * it->second.groups) k = LD;
  }
  if (k == ROWS && on_layers) k = LAYERS;
  if ((k == ROWS || k == LAYERS) && !hd.argmax_out) hd.argmax_out = amax_scratch;   // they store it unconditionally
  PROF(MI355ASR_K_CTC_HEAD);
  switch (k) {
    case NS1: PLANNED(launch_ns1_head(hd, it->second.ns, it->second.pp_sw, it->second.groups, s), "class head (ns1)"); break;
    case PP_SPLIT: PLANNED(launch_pp_head_split(hd, it->second.pp, it->second.pp_sw, it->second.groups, ranges, split, s), "class head (pp, split)"); break;
    case PP: PLANNED(launch_pp_head(hd, it->second.pp, it->second.pp_sw, it->second.groups, s), "class head (pp)"); break;
    case LD: PLANNED(launch_head_ld(hd, it->second.slabs, it->second.groups, s), "class head (ld)"); break;
    case LAYERS: {
      Gemm16Args h16{};
      h16.x = hd.x; h16.ldx = d; h16.bias = hd.bias; h16.y = hd.y; h16.ldy = hd.ldy; h16.M = M; h16.K = d; h16.NT = hd.NT;
      h16.n_valid = hd.n_valid; h16.eps = kLnEps; h16.argmax_out = hd.argmax_out;
      h16.part_max = 8; h16.part_v = part; h16.part_i = reinterpret_cast<int32_t*>(part + (size_t)8 * M);
      LAUNCH_TRY(launch_gemm16(m, E16_HEAD, false, h16, hd.wp, s), "class head");
      break;
    }
    case ROWS: LAUNCH_TRY(launch_gemm_rows(d, EPI_HEAD, false, hd, s), "class head"); break;
  }
  return 0;
}

}  // namespace mi355
