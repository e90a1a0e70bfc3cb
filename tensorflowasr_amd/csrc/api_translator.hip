// Translator host side (conformer_blocks.py:439-566), behind mi355asr_translator_* of include/mi355asr.h.
#include "model.h"

namespace {
// =======================================================================================================
// Translator (conformer_blocks.py:505-548)
// =======================================================================================================
constexpr int kMaxTokens = 2048;   // rows of the positional-encoding table

struct TransPlan : ScratchPlan {
  size_t kv, amax, hsplit, total;
};
TransPlan make_trans_plan(const mi355asr_model* m, int B, int U, int T) {
  const size_t d = m->cfg.dmodel, M = (size_t)B * U;
  TransPlan p;
  Layout lay;
  auto take = [&](size_t floats) { return lay.take(floats); };
  lay.scratch(p, M, d);
  p.kv = take((size_t)B * T * 2 * d); p.amax = take(M);
  p.h4 = gemm16_for(m, M) ? take(M * 4 * d) : 0;   // (every RBlock runs on exactly M = B * U rows: see make_plan in api.hip)
  p.hsplit = take(16 * M);          // per-range (maximum, class) pairs of the class head split over column ranges (up to 8)
  p.total = lay.o;
  return p;
}

}  // namespace

namespace mi355 {

int finalize_translator(mi355asr_model* m, hipStream_t s) {
  const auto& c = m->cfg;
  const auto& tc = m->tcfg;
  const int d = c.dmodel, hs = c.head_size, V = tc.tar_classes;
  ArenaBuilder ab;
  ab.ring_terms = m->cfg.gemm_dtype == 1 ? 1 : 3;
  const size_t o_emb = ab.put(m->host["inp_embedding/embeddings"].data);
  // positional_encoding.py:19-36: pe[pos, 2i] = sin(pos / 10000^(2i/d)), pe[pos, 2i+1] = cos(pos / 10000^(2i/d))
  std::vector<float> pe((size_t)kMaxTokens * d);
  for (int pos = 0; pos < kMaxTokens; ++pos)
    for (int i = 0; i < d; ++i) {
      const double ang = (double)pos / std::pow(10000.0, (double)(2 * (i / 2)) / d);
      pe[(size_t)pos * d + i] = (float)((i & 1) ? std::cos(ang) : std::sin(ang));
    }
  const size_t o_pe = ab.put(pe);
  StackOff so;
  for (int i = 0; i < tc.num_blocks; ++i) {
    const std::string p = "decoder_conformer_block_" + std::to_string(i);
    BlockOff o = pack_block(m, ab, p, d, hs);
    const auto& qk = m->host[p + "/mhsa_module/mha/query_kernel"].data;   // [H, d, hs]
    const auto& kk = m->host[p + "/mhsa_module/mha/key_kernel"].data;
    const auto& vk = m->host[p + "/mhsa_module/mha/value_kernel"].data;
    o.cross = true;
    o.xq_wp = ab.put(pack_p16([&](int i2, int n) { return qk[((size_t)(n / hs) * d + i2) * hs + n % hs]; }, d, d, d / 16));
    o.xkv_wp = ab.put(pack_p16(
        [&](int i2, int n) {
          const int r = n % d;
          const std::vector<float>& w = n < d ? kk : vk;
          return w[((size_t)(r / hs) * d + i2) * hs + r % hs];
        },
        d, 2 * d, 2 * d / 16));
    so.blocks.push_back(o);
  }
  pack_head(m, ab, so, m->host["fully_connected/kernel"].data, m->host["fully_connected/bias"].data, V);
  if (int rc = upload_arena(m, ab, s)) return rc;
  const float* base = m->arena;
  m->t_emb = base + o_emb;
  m->t_pe = base + o_pe;
  resolve_stack(m->t_stack, so, base);
  m->t_stack.opts.ksz = c.kernel_size;
  m->t_stack.opts.fc = c.fc_factor;
  for (auto& kv : m->host) { kv.second.data.clear(); kv.second.data.shrink_to_fit(); }
  m->finalized = true;
  return 0;
}

}  // namespace mi355

extern "C" {
// ---- Translator ----------------------------------------------------------------------------------------
int mi355asr_translator_create(const mi355asr_translator_config* cfg, mi355asr_model** out) {
  if (!cfg || !out) return fail(MI355ASR_EINVAL, "null argument");
  const auto& c = *cfg;
  if (c.dmodel != 144 && (c.dmodel % 128 != 0 || c.dmodel < 128 || c.dmodel > 1024))
    return fail(MI355ASR_EINVAL, "Translator: dmodel=%d, supported are 144 and multiples of 128 up to 1024", c.dmodel);
  if (c.num_heads * c.head_size != c.dmodel || !attention_head_size_ok(c.head_size))
    return fail(MI355ASR_EINVAL, "Translator: need num_heads*head_size == dmodel and a head size of 12, 16, 24, 32, 36, 48, 64, 72 or 128");
  if (c.kernel_size < 1 || c.kernel_size > 1024) return fail(MI355ASR_EINVAL, "kernel_size=%d: must be in 1 .. 1024", c.kernel_size);
  if (c.num_blocks < 1 || c.inp_classes < 1 || c.tar_classes < 2) return fail(MI355ASR_EINVAL, "Translator: bad block / class counts");
  auto* m = new mi355asr_model();
  m->is_translator = true;
  m->tcfg = c;
  std::memset(&m->cfg, 0, sizeof(m->cfg));
  m->cfg.dmodel = c.dmodel; m->cfg.head_size = c.head_size; m->cfg.num_heads = c.num_heads;
  m->cfg.kernel_size = c.kernel_size; m->cfg.fc_factor = c.fc_factor;
  std::memset(&m->dm, 0, sizeof(m->dm));
  const int d = c.dmodel;
  auto& ex = m->expected;
  ex.push_back({"inp_embedding/embeddings", {c.inp_classes, d}});
  for (int i = 0; i < c.num_blocks; ++i)
    add_block_expected(ex, "decoder_conformer_block_" + std::to_string(i), d, c.num_heads, c.head_size, c.kernel_size);
  ex.push_back({"fully_connected/kernel", {d, c.tar_classes}});
  ex.push_back({"fully_connected/bias", {c.tar_classes}});
  for (const auto& e : ex) m->host[e.name] = HostTensor{};
  *out = m;
  return 0;
}

int mi355asr_translator_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t U, int32_t T, size_t* bytes) {
  if (!m || !m->is_translator || !bytes) return fail(MI355ASR_EINVAL, "not a Translator handle / null argument");
  if (B < 1 || U < 1 || T < 1) return fail(MI355ASR_EINVAL, "B, U, T must be positive (got %d, %d, %d)", B, U, T);
  *bytes = make_trans_plan(m, B, U, T).total;
  return 0;
}

}  // extern "C"

// One body for mi355asr_translator_forward and its ragged form.  ragged: token lengths tok_len [B] (rows of ids) and encoder
// lengths enc_len [B] (frames of enc), both on the device
static int translator_forward(mi355asr_model* m, const int32_t* ids, bool ragged, const int32_t* tok_len, const float* enc,
                              const int32_t* enc_len, int32_t B, int32_t U, int32_t T, float* logits, int32_t* amax,
                              void* ws_, size_t ws_bytes, hipStream_t s) {
  if (!m || !m->is_translator) return fail(MI355ASR_EINVAL, "not a Translator handle");
  if (!m->finalized) return fail(MI355ASR_ESTATE, "weights not finalised: call mi355asr_finalize_weights first");
  int rc = 0;
  if (ragged && m->cfg.dmodel != 144 && (rc = ragged_layers256_ok(m, m->tcfg.kernel_size))) return rc;
  if (!ids || !enc || !ws_) return fail(MI355ASR_EINVAL, "null argument");
  if (B < 1 || U < 1 || T < 1) return fail(MI355ASR_EINVAL, "B, U, T must be positive (got %d, %d, %d)", B, U, T);
  if (U > kMaxTokens) return fail(MI355ASR_EINVAL, "U=%d exceeds the positional-encoding table (%d rows)", U, kMaxTokens);
  if (ragged && ((rc = ragged_rows_ok(U, "U")) || (rc = ragged_rows_ok(T, "T")))) return rc;
  const TransPlan p = make_trans_plan(m, B, U, T);
  if (ws_bytes < p.total) return fail(MI355ASR_EINVAL, "workspace too small: %zu < %zu", ws_bytes, p.total);
  std::vector<int32_t> tok_host, enc_host;
  if (ragged && (rc = ragged_check_lengths(tok_len, B, U, "tok_len", s, &tok_host))) return rc;
  if (ragged && (rc = ragged_check_lengths(enc_len, B, T, "enc_len", s, &enc_host))) return rc;
  char* ws = (char*)ws_;
  const int d = m->cfg.dmodel, M = B * U;
  Scratch sc = make_scratch(p, ws);
  EmbedArgs ea{ids, m->t_emb, sc.xa, M, m->tcfg.inp_classes, d};
  LAUNCH_TRY(launch_embed(ea, s), "embedding");
  CrossAttn cr{enc, T, (float*)(ws + p.kv), m->t_pe};
  BlockOpts bo = m->t_stack.opts;
  if (ragged) {
    cr.k_len = enc_len;
    cr.k_len_host = enc_host.data();
    bo.t_len_host = tok_host.data();
    bo.t_len = tok_len;                   // the ConvModule's depthwise conv reads zeros from token row tok_len[b] on
  }
  for (const auto& blk : m->t_stack.blocks)
    if ((rc = run_block(m, blk, bo, sc, B, U, nullptr, s, &cr))) return rc;
  const GemmArgs hd = head_args(m->t_stack, sc.xa, M, logits, amax ? amax : (int32_t*)(ws + p.amax));
  // round 5: from 2048 rows on the class head runs on the two-term stream of pp_head_kernel (or the slab ring), as the CTC decoder's
  // and the ChunkConformer's heads do (144 -> 9160 over 5952 rows: 0.44 ms on the fp32 MFMA kernel)
  float* hsplit = (float*)(ws + p.hsplit);
  if ((rc = run_class_head(m, hd, HeadLayers::after_streams, hsplit, hsplit, hd.argmax_out, s))) return rc;
  // the class head is row-wise: the rows past tok_len[b] get their values afterwards
  const int V = m->tcfg.tar_classes;
  if (ragged) LAUNCH_TRY(launch_ragged_rows(tok_len, B, U, logits, V, V, hd.argmax_out, s), "ragged Translator rows");
  return 0;
}

extern "C" {
int mi355asr_translator_forward(mi355asr_model* m, const int32_t* ids, const float* enc, int32_t B, int32_t U,
                                int32_t T, float* logits, int32_t* amax, void* ws, size_t ws_bytes, void* stream) {
  return translator_forward(m, ids, false, nullptr, enc, nullptr, B, U, T, logits, amax, ws, ws_bytes, (hipStream_t)stream);
}
int mi355asr_translator_forward_ragged(mi355asr_model* m, const int32_t* ids, const int32_t* tok_len, const float* enc,
                                       const int32_t* enc_len, int32_t B, int32_t U, int32_t T, float* logits, int32_t* amax,
                                       void* ws, size_t ws_bytes, void* stream) {
  return translator_forward(m, ids, true, tok_len, enc, enc_len, B, U, T, logits, amax, ws, ws_bytes, (hipStream_t)stream);
}
}  // extern "C"
