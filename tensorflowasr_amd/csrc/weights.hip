// Host tensors -> device arena: the weight-surface ABI (names, shapes, intake), every fragment packer, and the
// packing of fronts, block stacks and class heads shared by the four model kinds.
#include "model.h"

namespace mi355 {

void add_block_expected(std::vector<Expected>& ex, const std::string& p, int d, int H, int hs, int k,
                        bool keras_mha) {
  auto ln = [&](const std::string& q) {
    ex.push_back({q + "/gamma", {d}});
    ex.push_back({q + "/beta", {d}});
  };
  for (const char* ff : {"ff_module_1", "ff_module_2"}) {
    const std::string q = p + "/" + ff;
    ln(q + "/ln");
    ex.push_back({q + "/ffn1/kernel", {d, 4 * d}});
    ex.push_back({q + "/ffn1/bias", {4 * d}});
    ex.push_back({q + "/ffn2/kernel", {4 * d, d}});
    ex.push_back({q + "/ffn2/bias", {d}});
  }
  const std::string m = p + "/mhsa_module";
  ln(m + "/ln");
  if (keras_mha) {   // tf.keras.layers.MultiHeadAttention (chunk_conformer_blocks.py:147): biased q/k/v/out
    for (const char* w : {"query", "key", "value"}) {
      ex.push_back({m + "/mha/" + w + "/kernel", {d, H, hs}});
      ex.push_back({m + "/mha/" + w + "/bias", {H, hs}});
    }
    ex.push_back({m + "/mha/attention_output/kernel", {H, hs, d}});
    ex.push_back({m + "/mha/attention_output/bias", {d}});
  } else {
    ex.push_back({m + "/mha/query_kernel", {H, d, hs}});
    ex.push_back({m + "/mha/key_kernel", {H, d, hs}});
    ex.push_back({m + "/mha/value_kernel", {H, d, hs}});
    ex.push_back({m + "/mha/projection_kernel", {H, hs, d}});
    ex.push_back({m + "/mha/projection_bias", {d}});
  }
  const std::string c = p + "/conv_module";
  ln(c + "/ln");
  ex.push_back({c + "/pw_conv_1/kernel", {1, d, 2 * d}});
  ex.push_back({c + "/pw_conv_1/bias", {2 * d}});
  ex.push_back({c + "/dw_conv/depthwise_kernel", {k, d, 1}});
  ex.push_back({c + "/dw_conv/pointwise_kernel", {1, d, 2 * d}});
  ex.push_back({c + "/dw_conv/bias", {2 * d}});
  ex.push_back({c + "/bn/gamma", {2 * d}});
  ex.push_back({c + "/bn/beta", {2 * d}});
  ex.push_back({c + "/bn/moving_mean", {2 * d}});
  ex.push_back({c + "/bn/moving_variance", {2 * d}});
  ex.push_back({c + "/pw_conv_2/kernel", {1, 2 * d, d}});
  ex.push_back({c + "/pw_conv_2/bias", {d}});
  ln(p + "/ln");
}

// W[k][n] (k < K, n < N) -> P16 fragment order [ceil(K/16)][NTpad][64 lanes][4]
std::vector<float> pack_p16(const std::function<float(int, int)>& f, int K, int N, int NTpad) {
  const int KBT = ceil_div(K, 16);
  std::vector<float> out((size_t)KBT * NTpad * 256, 0.f);
  for (int kb = 0; kb < KBT; ++kb)
    for (int nt = 0; nt < NTpad; ++nt)
      for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, c = lane & 15;
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * kb + 4 * g + j, n = 16 * nt + c;
          if (k < K && n < N) out[(((size_t)kb * NTpad + nt) * 64 + lane) * 4 + j] = f(k, n);
        }
      }
  return out;
}

// ---- operand terms -----------------------------------------------------------------------------------------------------
// v as n bf16 terms: term t = round-to-nearest-even bf16 of what the terms before it left (three hold all 24 significand bits)
static void bf16_terms(float v, int n, uint16_t* out) {
  for (int t = 0; t < n; ++t) {
    uint32_t u; std::memcpy(&u, &v, 4);
    out[t] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    const uint32_t back = (uint32_t)out[t] << 16;
    float hf; std::memcpy(&hf, &back, 4);
    v -= hf;
  }
}
// round-to-nearest-even fp16 of a float (host side of the two-term scheme; subnormals and overflow to infinity included)
uint16_t f16_rne(float v) {
  uint32_t u; std::memcpy(&u, &v, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u >= 0x7f800000u) return (uint16_t)(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);          // rounds to >= 65520: infinity
  if (u < 0x38800000u) {                                             // below 2^-14: subnormal, spacing 2^-24
    float f; std::memcpy(&f, &u, 4);
    const float r = f * 16777216.0f;                                  // exact
    const float q = std::nearbyintf(r);                               // ties to even
    return (uint16_t)(sign | (uint32_t)q);                            // q == 1024 is the smallest normal
  }
  const uint32_t mant = u & 0x7fffffu, exp = (u >> 23) - 112;         // 1 .. 30
  uint32_t h = (exp << 10) | (mant >> 13);
  const uint32_t rem = mant & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;             // carries into the exponent as it should
  return (uint16_t)(sign | h);
}
float f16_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, mnt = h & 1023u;
  float f;
  if (e == 0) f = (float)mnt * 5.9604644775390625e-8f;                // 2^-24
  else if (e == 31) f = mnt ? NAN : INFINITY;
  else { const uint32_t u = ((e + 112) << 23) | (mnt << 13); std::memcpy(&f, &u, 4); }
  uint32_t u; std::memcpy(&u, &f, 4); u |= sign; std::memcpy(&f, &u, 4);
  return f;
}
// largest power of two s with bound * s <= 2^15 (fp16's largest finite value is 65504: a factor of two to spare)
// max_shift: kernels that multiply two or three such scales in fp32 (attention: sq * sk, probabilities * sv) pass 40 and get
// 0 = "no usable bound" (the three-term kernel runs) for degenerate weights instead of a product that overflows to inf
float half_scale_for(double bound, int max_shift) {
  if (!(bound > 0.0) || !std::isfinite(bound)) return 0.f;
  int e; std::frexp(bound, &e);                                       // bound = f 2^e, f in [0.5, 1)
  const int k = 15 - e;
  if (k > max_shift || k < -max_shift) return max_shift < 100 ? 0.f : std::ldexp(1.0f, std::max(-100, std::min(100, k)));
  return std::ldexp(1.0f, k);
}
// v as hi + lo fp16 (two-term scheme)
static void f16_pair(float v, uint16_t* out) {
  out[0] = f16_rne(v);
  out[1] = f16_rne(v - f16_to_float(out[0]));
}

// ---- MFMA fragments ----------------------------------------------------------------------------------------------------
// What a fragment's elements are split into: n bf16 terms of the value, or (f16_scale != 0) hi + lo fp16 of value * f16_scale.
struct Terms { int n; float f16_scale; };
constexpr Terms kBf16x3{3, 0.f};
// nfrag fragments of [terms][64 lanes][8] 16-bit words, element (lane, j) of fragment i = at(i, lane, j); the (k, n) <-> (fragment,
// lane, j) mappings below say which matrix element that is
static std::vector<float> pack_frags(size_t nfrag, Terms terms, const std::function<float(size_t, int, int)>& at) {
  std::vector<uint16_t> frag(nfrag * terms.n * 64 * 8, 0);
  uint16_t t16[3];
  for (size_t i = 0; i < nfrag; ++i)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const float v = at(i, lane, j);
        if (terms.f16_scale != 0.f) f16_pair(v * terms.f16_scale, t16);
        else bf16_terms(v, terms.n, t16);
        for (int t = 0; t < terms.n; ++t) frag[((i * terms.n + t) * 64 + lane) * 8 + j] = t16[t];
      }
  std::vector<float> as_f(frag.size() / 2);
  std::memcpy(as_f.data(), frag.data(), frag.size() * 2);
  return as_f;
}

// W[k][n] -> fragments for v_mfma_f32_16x16x32_bf16 / _f16: [ceil(K/32) steps][N/16 tiles][terms][64 lanes][8],
// lane (r = lane & 15, g = lane >> 4) of tile nt holds, for column 16 nt + r, rows k = 32 step + 16 (j >> 2) + 4 g + (j & 3)
// (the two 16-blocks of a step side by side, as a lane's accumulator-layout float4 pair provides them); zero past K.
static std::vector<float> pack_steps32(const std::function<float(int, int)>& f, int K, int N, Terms terms) {
  const int NT = N / 16;
  return pack_frags((size_t)ceil_div(K, 32) * NT, terms, [&](size_t i, int lane, int j) {
    const int st = (int)(i / NT), nt = (int)(i % NT);
    const int k = 32 * st + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3), n = 16 * nt + (lane & 15);
    return k < K ? f(k, n) : 0.f;
  });
}
// ... as three exact bf16 terms (split-bf16 scheme)
std::vector<float> pack_split32(const std::function<float(int, int)>& f, int K, int N) { return pack_steps32(f, K, N, kBf16x3); }
// ... as TWO fp16 terms of f * scale (two-term scheme)
std::vector<float> pack_half32(const std::function<float(int, int)>& f, int K, int N, float scale) {
  return pack_steps32(f, K, N, Terms{2, scale});
}

// conv2 kernel [3][3][d][d] (HWIO) as fragments for subconv_split_ring_kernel: column chunks of NTc tiles (all
// nine at dmodel 144, eight otherwise).  Steps (subconv.hip): s < 4 KB: channel block cb = s / 4, tap pair p = s % 4 -- lane
// (r = lane & 15, g = lane >> 4) of column tile nt holds, for out channel 16 nt + r, in-channels 16 cb + 4 g + (j & 3) at tap
// 2 p + (j >> 2); then ceil(KB / 2) steps with the NINTH tap of two channel blocks: j < 4 -> block 2 i, j >= 4 -> block
// 2 i + 1 (zero past the last block).
static std::vector<float> pack_conv2(const std::vector<float>& c2, int d, Terms terms) {
  const int KBn = d / 16, steps = KBn * 4 + (KBn + 1) / 2, NTc = d == 144 ? 9 : 8, chunks = KBn / NTc;
  return pack_frags((size_t)chunks * steps * NTc, terms, [&](size_t i, int lane, int j) {
    const int nt = (int)(i % NTc), st = (int)(i / NTc % steps), ch = (int)(i / NTc / steps);
    int cb, q;
    if (st < KBn * 4) { cb = st / 4; q = 2 * (st % 4) + (j >> 2); }
    else { cb = 2 * (st - KBn * 4) + (j >> 2); q = 8; }
    const int cin = 16 * cb + 4 * (lane >> 4) + (j & 3), cout = 16 * (ch * NTc + nt) + (lane & 15);
    return cb < KBn ? c2[((size_t)q * d + cin) * d + cout] : 0.f;
  });
}
std::vector<float> pack_conv2_split(const std::vector<float>& c2, int d) { return pack_conv2(c2, d, kBf16x3); }
// ... as two fp16 terms of kernel * wscale
std::vector<float> pack_conv2_half(const std::vector<float>& c2, int d, float wscale) { return pack_conv2(c2, d, Terms{2, wscale}); }

// LEAF Gabor filters [80 complex filters][K taps] (re / im interleaved: channel 2 f, 2 f + 1) for leaf.hip's split-bf16 conv:
// [13 k-blocks of 32 taps][10 column tiles][terms][64 lanes][8]: lane (r = lane & 15, g = lane >> 4) holds taps
// 32 kb + 8 g + 0..7 of channel 16 nt + r
static std::vector<float> pack_leaf_split(const std::vector<double>& re, const std::vector<double>& im, int K, int terms) {
  return pack_frags((size_t)13 * 10, Terms{terms, 0.f}, [&](size_t i, int lane, int j) {
    const int kb = (int)(i / 10), nt = (int)(i % 10);
    const int tap = 32 * kb + 8 * (lane >> 4) + j, ch = 16 * nt + (lane & 15);
    return tap < K ? (float)((ch & 1) ? im[(size_t)(ch >> 1) * K + tap] : re[(size_t)(ch >> 1) * K + tap]) : 0.f;
  });
}

// Appends the slabs of W (pack_split32 order) to a slab stream: one slab = 9 column tiles of one 32-wide step = 1728
// fragments of 16 bytes, padded to 1792 (SlabStream in fused.hip).  group_major: all steps of tile group 0, then of
// group 1, ... (the order a GEMM swept in column chunks consumes them); else step by step, its groups side by side.
void append_slabs(std::vector<float>& stream, const std::function<float(int, int)>& f, int K, int N, bool group_major) {
  const std::vector<float> sp = pack_split32(f, K, N);
  const int steps = ceil_div(K, 32), NT = N / 16, groups = NT / 9;
  const size_t used = 1728 * 4, stride = 1792 * 4;
  auto put = [&](int st, int gr) {
    const size_t at = stream.size();
    stream.resize(at + stride, 0.f);
    std::memcpy(stream.data() + at, sp.data() + ((size_t)st * NT + 9 * gr) * 192 * 4, used * sizeof(float));
  };
  if (group_major) { for (int gr = 0; gr < groups; ++gr) for (int st = 0; st < steps; ++st) put(st, gr); }
  else { for (int st = 0; st < steps; ++st) for (int gr = 0; gr < groups; ++gr) put(st, gr); }
}
// the subsampling Dense [K, 144] for sublinear_split_kernel: 1728 fragments per 32-wide step, padded to 7 x 256 (4 floats each)
std::vector<float> pack_linear_split(const std::vector<float>& lin, int K, int d) {
  const std::vector<float> sp = pack_split32([&](int k, int n) { return lin[(size_t)k * d + n]; }, K, d);
  const size_t steps = (size_t)ceil_div(K, 32), used = 1728 * 4, stride = 1792 * 4;
  std::vector<float> padded(steps * stride, 0.f);
  for (size_t st = 0; st < steps; ++st) std::memcpy(padded.data() + st * stride, sp.data() + st * used, used * sizeof(float));
  return padded;
}

// ---- pair-pipelined streams (fused_pp.hip; layout tables generated by tools/gen_pp.py) -----------------------------------
#include "pp_layout.inc"
namespace {
// one ring slot: kPpSlot fragments of 1 KB (256 floats) in the order of `lay`; src(desc) = the fragment's 256 floats
void put_pp_slot(std::vector<float>& stream, const PpFragDesc (&lay)[kPpSlot], const std::function<const float*(const PpFragDesc&)>& src) {
  const size_t at = stream.size();
  stream.resize(at + (size_t)kPpSlot * 256, 0.f);
  for (int i = 0; i < kPpSlot; ++i)
    if (lay[i].kind != 0) std::memcpy(stream.data() + at + (size_t)i * 256, src(lay[i]), 256 * sizeof(float));
}
float matrix_scale(const std::function<float(int, int)>& f, int K, int N) {   // power of two: max |f| * s in [2^14, 2^15)
  double mx = 0.0;
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) mx = std::max(mx, std::fabs((double)f(k, n)));
  const float s = half_scale_for(mx);
  return s > 0.f ? s : 1.0f;                  // an all-zero matrix
}
}  // namespace
// Chain y += W2 act(W1aug [x ; 1]) over P = H / 32 hidden pairs, units A, AP, (P - 2) x F, BP, B (2 P ring slots):
// an A fragment = W1aug step a, hidden tile 2 pair + b; a B fragment = W2 step `pair`, column tile a.  Returns the scales the
// two matrices were packed with and the bounds the kernel derives the operand scales from.
PpChainSc append_pp_chain(std::vector<float>& stream, const std::function<float(int, int)>& w1aug, int H, const std::function<float(int, int)>& w2,
                          std::vector<float>* plain1, std::vector<float>* plain2) {
  const int P = H / 32, NT1 = H / 16;
  PpChainSc sc;
  sc.sw1 = matrix_scale(w1aug, 145, H);
  sc.sw2 = matrix_scale(w2, H, 144);
  double l1 = 0.0, bm = 0.0;
  for (int n = 0; n < H; ++n) {
    double sum = 0.0;
    for (int k = 0; k < 144; ++k) sum += std::fabs((double)w1aug(k, n));
    l1 = std::max(l1, sum);
    bm = std::max(bm, std::fabs((double)w1aug(144, n)));
  }
  sc.l1 = (float)(l1 * (1.0 + 1e-6));         // rounded up: the bound has to hold in float
  sc.bmax = (float)(bm * (1.0 + 1e-6));
  const std::vector<float> sp1 = pack_half32(w1aug, 145, H, sc.sw1);      // [5 steps][NT1][2 terms][256]
  const std::vector<float> sp2 = pack_half32(w2, H, 144, sc.sw2);         // [P steps][9][2][256]
  auto fa = [&](int pair, const PpFragDesc& d) { return sp1.data() + (((size_t)d.a * NT1 + 2 * pair + d.b) * 2 + d.term) * 256; };
  auto fb = [&](int pair, const PpFragDesc& d) { return sp2.data() + (((size_t)pair * 9 + d.a) * 2 + d.term) * 256; };
  auto unit = [&](const PpFragDesc (&lay)[kPpSlot], int pa, int pb) {
    put_pp_slot(stream, lay, [&](const PpFragDesc& d) { return d.kind == 1 ? fa(pa, d) : fb(pb, d); });
  };
  unit(kPpLayout_A0, 0, -1);
  unit(kPpLayout_AP0, 1, -1);
  for (int p = 0; p + 2 < P; ++p) { unit(kPpLayout_F0, p + 2, p); unit(kPpLayout_F1, p + 2, p); }
  unit(kPpLayout_BP0, -1, P - 2);
  unit(kPpLayout_B0, -1, P - 1);
  if (plain1) *plain1 = sp1;                  // the same fragments in plain [step][tile][term] order (fused_ns.hip)
  if (plain2) *plain2 = sp2;
  return sc;
}
// A plain layer [145 (row 144 = bias), 144 * groups] in column groups of nine tiles, five S units (ring slots) per group;
// returns the power of two the matrix was packed with
float append_pp_plain(std::vector<float>& stream, const std::function<float(int, int)>& waug, int groups, std::vector<float>* plain) {
  const int NT = 9 * groups;
  const float sw = matrix_scale(waug, 145, 144 * groups);
  const std::vector<float> sp = pack_half32(waug, 145, 144 * groups, sw);
  for (int g = 0; g < groups; ++g)
    for (int st = 0; st < 5; ++st)
      put_pp_slot(stream, kPpLayout_S0, [&](const PpFragDesc& d) { return sp.data() + (((size_t)st * NT + 9 * g + d.a) * 2 + d.term) * 256; });
  if (plain) *plain = sp;
  return sw;
}


// The DFT kernels are model variables (time_frequency.py:62-75 creates them from backend.py:27-69 and a checkpoint
// may overwrite them).  When they are exactly window[n] * (cos, -+sin)(2 pi k n / 1024) the STFT runs as a
// 32 x 32 Cooley-Tukey factorisation (fft_stft.hip); otherwise the dense DFT GEMM stays.  MI355ASR_FFT=0 forces dense.
FftOff pack_fft(ArenaBuilder& ab, const std::vector<float>& re, const std::vector<float>& im, int n_dft, int nb) {
  FftOff o;
  if (mi355_env("MI355ASR_FFT", 1) == 0) return o;
  if (n_dft != 1024 || nb != 513) return o;
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<double> ct(1024), st(1024);
  for (int i = 0; i < 1024; ++i) { ct[i] = std::cos(two_pi * i / 1024.0); st[i] = std::sin(two_pi * i / 1024.0); }
  std::vector<float> win(1024);
  for (int n = 0; n < 1024; ++n) win[n] = re[(size_t)n * nb];   // bin 0: cos = 1
  const double tol = 1e-6;
  bool neg = true, pos = true;   // imag = -w sin (reference) or +w sin: the power spectrum does not care
  for (int n = 0; n < 1024; ++n)
    for (int k = 0; k < nb; ++k) {
      const int a = (int)(((int64_t)k * n) & 1023);
      const double w = win[n];
      if (std::fabs(re[(size_t)n * nb + k] - w * ct[a]) > tol) return o;
      const double iv = im[(size_t)n * nb + k];
      if (std::fabs(iv + w * st[a]) > tol) neg = false;
      if (std::fabs(iv - w * st[a]) > tol) pos = false;
      if (!neg && !pos) return o;
    }
  // stage 1: K = n1 (32), columns [Re k1 (32) | Im k1 (32)] of W32^(n1 k1)
  // stage 1: K = n1 (32), columns [Re k1 (32) | Im k1 (32)] of W32^(n1 k1)
  auto f1 = [&](int k, int n) { const int a = ((k * (n & 31)) & 31) * 32; return (float)(n < 32 ? ct[a] : -st[a]); };
  // stage 2: K = [Re n2 (32) | Im n2 (32)], columns [Re k2 (16) | Im k2 (16)] of W32^(n2 k2)
  auto f2 = [&](int k, int n) {
    const int a = (((k & 31) * (n & 15)) & 31) * 32;
    if (k < 32) return (float)(n < 16 ? ct[a] : -st[a]);
    return (float)(n < 16 ? st[a] : ct[a]);
  };
  o.w1 = ab.put(pack_p16(f1, 32, 64, 4));
  o.w2 = ab.put(pack_p16(f2, 64, 32, 2));
  o.w1s = ab.put(pack_split32(f1, 32, 64));      // the same matrices as exact three-term bf16 fragments (round 3)
  o.w2s = ab.put(pack_split32(f2, 64, 32));
  o.w1h = ab.put(pack_half32(f1, 32, 64, 16384.f));      // two-term scheme: |cos|, |sin| <= 1 times 2^14
  o.w2h = ab.put(pack_half32(f2, 64, 32, 16384.f));
  std::vector<float> tc(1024), ts(1024);
  for (int k1 = 0; k1 < 32; ++k1)
    for (int n2 = 0; n2 < 32; ++n2) { tc[k1 * 32 + n2] = (float)ct[k1 * n2]; ts[k1 * 32 + n2] = (float)st[k1 * n2]; }
  o.twc = ab.put(tc);
  o.tws = ab.put(ts);
  o.win = ab.put(win);
  o.ok = true;
  return o;
}


MelBandOff pack_mel_band(ArenaBuilder& ab, const std::vector<float>& f2m, int nb, int n_mels) {
  MelBandOff o;
  // MI355ASR_MEL_BAND=0: always the dense mel GEMM
  static const bool on = mi355_env("MI355ASR_MEL_BAND", 1) != 0;
  if (!on) return o;
  std::vector<int> band(2 * (size_t)n_mels, 0);
  int bw = 4;
  for (int m = 0; m < n_mels; ++m) {
    int lo = -1, hi = -1;
    for (int k = 0; k < nb; ++k)
      if (f2m[(size_t)k * n_mels + m] != 0.f) { if (lo < 0) lo = k; hi = k; }
    if (lo >= 0) { band[2 * m] = lo; band[2 * m + 1] = hi - lo + 1; bw = std::max(bw, hi - lo + 1); }
  }
  if (bw > 64) return o;
  bw = (bw + 3) & ~3;
  const int lp = ((nb + 15) / 16) * 16;                          // the kernel reads bins [lo, lo + bw) of a row of >= lp floats
  for (int m = 0; m < n_mels; ++m)
    if (band[2 * m] + bw > lp) return o;
  std::vector<float> w((size_t)n_mels * bw, 0.f);
  for (int m = 0; m < n_mels; ++m)
    for (int j = 0; j < band[2 * m + 1]; ++j) w[(size_t)m * bw + j] = f2m[(size_t)(band[2 * m] + j) * n_mels + m];
  std::vector<float> band_f(band.size());
  std::memcpy(band_f.data(), band.data(), band.size() * sizeof(int));   // the arena is a float array: raw bits
  o.band = ab.put(band_f);
  o.bw = ab.put(w);
  o.BW = bw;
  o.ok = true;
  return o;
}
void use_mel_band(mi355asr_model* m, const MelBandOff& o, const float* base) {
  m->mel_band = o.ok ? reinterpret_cast<const int*>(base + o.band) : nullptr;
  m->mel_bw = o.ok ? base + o.bw : nullptr;
  m->mel_BW = o.ok ? o.BW : 0;
}
// Slab ring of gemm_ring.hip: [N / 128 chunks][K / 32 steps][8 column tiles][3 terms][64 lanes][8 bf16]; a GLU layer's
// chunk holds four value tiles and the four gate tiles that go with them.
void put_ring(ArenaBuilder& ab, size_t p16_off, const std::function<float(int, int)>& f, int K, int N, bool glu) {
  if (K % 128 != 0 || N % (glu ? 128 * 2 : 128) != 0) return;
  const int terms = ab.ring_terms;
  const std::vector<float> sp = pack_split32(f, K, N);       // [step][NT][3 terms][64 lanes][8 bf16]
  constexpr size_t TERM = 64 * 8 / 2;                         // floats per (step, column tile, term)
  const int steps = K / 32, NT = N / 16, chunks = NT / 8, half = NT / 2;
  std::vector<float> ring((size_t)chunks * steps * 8 * terms * TERM);
  for (int ch = 0; ch < chunks; ++ch)
    for (int st = 0; st < steps; ++st)
      for (int i = 0; i < 8; ++i) {
        const int tile = glu ? (i < 4 ? 4 * ch + i : half + 4 * ch + (i - 4)) : 8 * ch + i;
        // bf16 mode keeps term 0 only: round-to-nearest-even bf16 of the weight, what the bf16 arena holds as well
        std::memcpy(ring.data() + (((size_t)ch * steps + st) * 8 + i) * terms * TERM, sp.data() + ((size_t)st * NT + tile) * 3 * TERM,
                    terms * TERM * sizeof(float));
      }
  ab.ring_pairs.emplace_back(p16_off, ab.put(ring));
}
// The class head W[K, V] as a slab ring: V padded with zero columns to whole chunks of 128 (the kernel never looks at
// classes >= V).
void put_ring_head(ArenaBuilder& ab, size_t p16_off, const std::function<float(int, int)>& f, int K, int V) {
  if (K % 128 != 0 || V < 1) return;
  put_ring(ab, p16_off, [&](int k, int n) { return n < V ? f(k, n) : 0.f; }, K, ceil_div(V, 128) * 128, false);
}
// MI355ASR_GEMM_RING=0: the dense layers of dmodel 256 / 512 stay on the fp32-MFMA kernels (chain2 / gemm16<PF32>), or
// in bf16 mode on gemm16<PBf16>
// rows from which launch_gemm16 hands a dense layer to the ring kernels (crossover measured below)
long ring_min_rows() {
  static const long v = mi355_env("MI355ASR_RING_MIN_M", 1500);
  return v;
}
bool ring_packs_wanted(const mi355asr_model* m) {
  static const bool on = mi355_env("MI355ASR_GEMM_RING", 1) != 0;
  // (bf16 mode, dmodel 256: chain256_bf16_kernel reads the one-term ring packs at every row count)
  return on && m->cfg.dmodel % 128 == 0 &&
         (m->expected_rows < 0 || m->expected_rows >= ring_min_rows() || (m->cfg.gemm_dtype == 1 && m->cfg.dmodel == 256));
}
void register_rings(mi355asr_model* m, const ArenaBuilder& ab, const float* base) {
  for (const auto& pr : ab.ring_pairs) m->ring_of[base + pr.first] = base + pr.second;
  m->head_of.clear();
  for (const auto& hp : ab.head_pairs) m->head_of[base + hp.p16] = {base + hp.slabs, hp.groups, base + hp.pp, hp.pp_sw, base + hp.ns};
}
void put_head_slabs(ArenaBuilder& ab, size_t p16_off, const std::function<float(int, int)>& f, int d, int V, const float* bias) {
  if (d != 144 || V < 1) return;
  const int groups = ceil_div(ceil_div(V, 16), 9);
  std::vector<float> st;
  append_slabs(st, [&](int k, int n) { return n < V ? f(k, n) : 0.f; }, d, 144 * groups, true);
  const size_t o_st = ab.put(st);
  // the same matrix as the two-term fp16 stream of pp_head_kernel: column groups of nine tiles, five plain ring slots each,
  // the bias in row 144
  std::vector<float> pp, plain;
  const float sw = append_pp_plain(pp, [&](int k, int n) { return n < V ? (k < d ? f(k, n) : bias[n]) : 0.f; }, groups, &plain);
  const size_t o_pp = ab.put(pp);
  ab.head_pairs.push_back({p16_off, o_st, groups, o_pp, sw, ab.put(plain)});
}

using Mat = std::function<float(int, int)>;
// views of a row-major host matrix: all of it, columns from c0 on, rows from r0 on, and [W ; b] (row K = the bias)
static Mat mat(const std::vector<float>& w, int ld) { return [&w, ld](int k, int n) { return w[(size_t)k * ld + n]; }; }
static Mat cols_from(const Mat& f, int c0) { return [f, c0](int k, int n) { return f(k, c0 + n); }; }
static Mat rows_from(const Mat& f, int r0) { return [f, r0](int k, int n) { return f(r0 + k, n); }; }
static Mat with_bias(const Mat& f, int K, const std::vector<float>& b) { return [f, K, &b](int k, int n) { return k < K ? f(k, n) : b[n]; }; }

BlockOff pack_block(mi355asr_model* m, ArenaBuilder& ab, const std::string& p, int d, int hs, bool keras_mha) {
  auto T = [&](const std::string& n) -> const std::vector<float>& { return m->host[n].data; };
  BlockOff o;
  const bool rings = ring_packs_wanted(m);
  // a dense layer W[K, N]: its P16 pack, and its slab ring where the ring kernels may run it
  auto dense = [&](const Mat& f, int K, int N, bool glu = false) {
    const size_t at = ab.put(pack_p16(f, K, N, N / 16));
    if (rings) put_ring(ab, at, f, K, N, glu);
    return at;
  };
  // ---- the block's matrices, each defined once
  const std::string a = p + "/mhsa_module", c = p + "/conv_module";
  const Mat ff_w1[2] = {mat(T(p + "/ff_module_1/ffn1/kernel"), 4 * d), mat(T(p + "/ff_module_2/ffn1/kernel"), 4 * d)};
  const Mat ff_w2[2] = {mat(T(p + "/ff_module_1/ffn2/kernel"), d), mat(T(p + "/ff_module_2/ffn2/kernel"), d)};
  const std::vector<float>* ff_b1[2] = {&T(p + "/ff_module_1/ffn1/bias"), &T(p + "/ff_module_2/ffn1/bias")};
  const auto &qk = T(a + (keras_mha ? "/mha/query/kernel" : "/mha/query_kernel")), &kk_ = T(a + (keras_mha ? "/mha/key/kernel" : "/mha/key_kernel")),
             &vk = T(a + (keras_mha ? "/mha/value/kernel" : "/mha/value_kernel"));
  // q | k | v side by side, column n = which*d + h*hs + o: Keras MHA kernels are [d, H, hs] = [d, d] row-major; the reference's own
  // layer (einsum "BNI,HIO->BNHO") keeps kernel[h][i][o]
  const Mat qkv_at = [&qk, &kk_, &vk, d, hs, keras_mha](int i, int n) {
    const int which = n / d, r = n % d, h = r / hs, oo = r % hs;
    const std::vector<float>& w = which == 0 ? qk : (which == 1 ? kk_ : vk);
    return keras_mha ? w[(size_t)i * d + r] : w[((size_t)h * d + i) * hs + oo];
  };
  std::vector<float> qb(3 * d, 0.f);               // q / k / v bias (zero for the reference's own attention layer)
  if (keras_mha) {
    const auto &bq = T(a + "/mha/query/bias"), &bk = T(a + "/mha/key/bias"), &bv = T(a + "/mha/value/bias");
    for (int i = 0; i < d; ++i) { qb[i] = bq[i]; qb[d + i] = bk[i]; qb[2 * d + i] = bv[i]; }
  }
  const Mat out_w = mat(T(a + (keras_mha ? "/mha/attention_output/kernel" : "/mha/projection_kernel")), d);   // [H, hs, d]: row k = h*hs + i
  const auto& out_b = T(a + (keras_mha ? "/mha/attention_output/bias" : "/mha/projection_bias"));
  const Mat pw1 = mat(T(c + "/pw_conv_1/kernel"), 2 * d), pc = mat(T(c + "/dw_conv/pointwise_kernel"), 2 * d), pw2 = mat(T(c + "/pw_conv_2/kernel"), d);
  const auto &pw1_b = T(c + "/pw_conv_1/bias"), &pc_b = T(c + "/dw_conv/bias");
  std::vector<float> bn_s(2 * d), bn_t(2 * d);     // BatchNorm (inference) folded into scale and shift
  {
    const auto &g = T(c + "/bn/gamma"), &b = T(c + "/bn/beta"), &mu = T(c + "/bn/moving_mean"), &var = T(c + "/bn/moving_variance");
    for (int i = 0; i < 2 * d; ++i) { bn_s[i] = g[i] / std::sqrt(var[i] + kBnEps); bn_t[i] = b[i] - mu[i] * bn_s[i]; }
  }
  // Operand bounds for the two-term attention kernels: a LayerNorm output lies in sqrt(d - 1) |gamma_i| + |beta_i|, so
  // |q_n|, |k_n|, |v_n| <= sum_i |W_in| (sqrt(d - 1) |gamma_i| + |beta_i|) + |b_n| (q times the query scale and log2 e,
  // which the kernel folds into it)
  auto att_bounds = [&](double margin) {
    const auto &lg = T(a + "/ln/gamma"), &lb = T(a + "/ln/beta");
    const double lnb = std::sqrt((double)(d - 1));
    double bnd[3] = {0.0, 0.0, 0.0};
    for (int n = 0; n < 3 * d; ++n) {
      double sum = std::fabs((double)qb[n]);
      for (int i = 0; i < d; ++i) sum += std::fabs((double)qkv_at(i, n)) * (lnb * std::fabs((double)lg[i]) + std::fabs((double)lb[i]));
      bnd[n / d] = std::max(bnd[n / d], sum);
    }
    bnd[0] *= 1.4426950408889634 / std::sqrt((double)hs);
    for (int k = 0; k < 3; ++k) o.att_h2[k] = half_scale_for(bnd[k] * margin, 40);
  };
  // ---- per-layer packs (every dmodel)
  for (int i = 0; i < 2; ++i) {
    const std::string q = p + (i == 0 ? "/ff_module_1" : "/ff_module_2");
    o.ff_ln_g[i] = ab.put(T(q + "/ln/gamma"));
    o.ff_ln_b[i] = ab.put(T(q + "/ln/beta"));
    o.ff_w1p[i] = dense(ff_w1[i], d, 4 * d);
    o.ff_b1[i] = ab.put(*ff_b1[i]);
    o.ff_w2p[i] = dense(ff_w2[i], 4 * d, d);
    o.ff_b2[i] = ab.put(T(q + "/ffn2/bias"));
  }
  o.att_ln_g = ab.put(T(a + "/ln/gamma"));
  o.att_ln_b = ab.put(T(a + "/ln/beta"));
  o.qkv_wp = dense(qkv_at, d, 3 * d);
  o.qkv_b = ab.put(qb);
  o.out_wp = dense(out_w, d, d);
  o.out_b = ab.put(out_b);
  o.cv_ln_g = ab.put(T(c + "/ln/gamma"));
  o.cv_ln_b = ab.put(T(c + "/ln/beta"));
  o.pw1_wp = dense(pw1, d, 2 * d, true);
  o.pw1_b = ab.put(pw1_b);
  o.dw_w = ab.put(T(c + "/dw_conv/depthwise_kernel"));  // [k, d, 1] == [k][d]
  o.pc_w1p = dense(pc, d, 2 * d);
  o.pc_b1 = ab.put(pc_b);
  o.bn_s = ab.put(bn_s);
  o.bn_t = ab.put(bn_t);
  o.pw2_wp = dense(pw2, 2 * d, d);
  o.pw2_b = ab.put(T(c + "/pw_conv_2/bias"));
  o.ln_g = ab.put(T(p + "/ln/gamma"));
  o.ln_b = ab.put(T(p + "/ln/beta"));
  // round 5: operand bounds for the head-size-64 models (attention_split64_kernel): q / k / v of the layer-at-a-time projections.
  // In bf16 mode weights and activations are rounded to bf16 first: each factor grows by at most 2^-8.
  if (d != 144 && d % 64 == 0 && hs == 64) att_bounds(1.01);
  if (d != 144) return o;

  // ---- dmodel 144: the slab streams of the loader-wave kernels (fused.hip), the pair-pipelined ones (fused_pp.hip) and the same
  // two-term fragments in plain order for the N-split kernels (fused_ns.hip: small batches)
  o.split = o.ns = true;
  // fp32 mode: 1.0001 covers the rounding of the bound's own evaluation.  bf16 mode (gemm_dtype 1: the generic per-layer path
  // rounds weights AND activations to bf16 before the projections, each factor growing by up to 2^-8) takes the 1.01 margin of
  // the head-size-64 bounds above, so that bound * scale <= 2^15 holds there too (round-5 advice)
  att_bounds(m->cfg.gemm_dtype == 1 ? 1.01 : 1.0001);
  // a chain W2 act(W1 x + b1) for the loader-wave kernels: per hidden chunk of 144 the five steps of W1[:, chunk] and of W2[chunk, :]
  auto chain_slabs = [&](std::vector<float>& st, const Mat& w1, const Mat& w2, int chunks) {
    for (int ch = 0; ch < chunks; ++ch) {
      append_slabs(st, cols_from(w1, d * ch), d, d, false);
      append_slabs(st, rows_from(w2, d * ch), d, d, false);
    }
  };
  {
    // slab stream of ff1_qkv_ring_kernel: ff_module_1, then q, k, v (five steps each)
    std::vector<float> st;
    chain_slabs(st, ff_w1[0], ff_w2[0], 4);
    append_slabs(st, qkv_at, d, 3 * d, true);
    o.ff1_slabs = ab.put(st);
    // pair-pipelined stream: ff_module_1 as 18 hidden pairs, bias in row 144 of W1; then q, k, v with their bias in row 144
    std::vector<float> pp, n1, n2, nq;
    o.pp_ff1_sc = append_pp_chain(pp, with_bias(ff_w1[0], d, *ff_b1[0]), 4 * d, ff_w2[0], &n1, &n2);
    o.pp_sw_qkv = append_pp_plain(pp, with_bias(qkv_at, d, qb), 3, &nq);
    o.pp_ff1 = ab.put(pp);
    o.ns_ff1_w1 = ab.put(n1); o.ns_ff1_w2 = ab.put(n2); o.ns_qkv = ab.put(nq);
  }
  {
    // slab stream of out_glu_ring_kernel: out-projection (5 slabs), then pw_conv_1 step by step (value | gate)
    std::vector<float> st;
    append_slabs(st, out_w, d, d, false);
    append_slabs(st, pw1, d, 2 * d, false);
    o.og_slabs = ab.put(st);
    // two-term fp16 stream of pp_out_glu_kernel: out projection (one group of nine tiles), then pw_conv_1's value tiles and
    // gate tiles (two groups), five plain ring slots each, the biases in row 144
    std::vector<float> pp, no, np1;
    o.pp_sw_out = append_pp_plain(pp, with_bias(out_w, d, out_b), 1, &no);
    o.pp_sw_pw1 = append_pp_plain(pp, with_bias(pw1, d, pw1_b), 2, &np1);
    o.pp_og = ab.put(pp);
    o.ns_out = ab.put(no); o.ns_pw1 = ab.put(np1);
  }
  {
    // slab stream of tail_ff2_ring_kernel: the conv tail (pointwise 144 -> 288, pw_conv_2 288 -> 144), then FFModule 2 (144 -> 576 -> 144)
    std::vector<float> st;
    chain_slabs(st, pc, pw2, 2);
    chain_slabs(st, ff_w1[1], ff_w2[1], 4);
    o.tail_slabs = ab.put(st);
    // pair-pipelined stream: the conv tail as 9 hidden pairs with the folded BatchNorm in the weights -- column n of the
    // pointwise kernel times scale[n], row 144 = bias[n] * scale[n] + shift[n] (products formed in double, rounded once) --
    // then ff_module_2 as 18 pairs with its bias in row 144
    std::vector<float> pp, c1, c2, n1, n2;
    o.pp_tail_sc[0] = append_pp_chain(pp, [&](int kk, int n) {
      return kk < d ? (float)((double)pc(kk, n) * (double)bn_s[n]) : (float)((double)pc_b[n] * (double)bn_s[n] + (double)bn_t[n]);
    }, 2 * d, pw2, &c1, &c2);
    o.pp_tail_sc[1] = append_pp_chain(pp, with_bias(ff_w1[1], d, *ff_b1[1]), 4 * d, ff_w2[1], &n1, &n2);
    o.pp_tail = ab.put(pp);
    o.ns_cv_w1 = ab.put(c1); o.ns_cv_w2 = ab.put(c2); o.ns_ff2_w1 = ab.put(n1); o.ns_ff2_w2 = ab.put(n2);
  }
  return o;
}

BlockDev resolve(const BlockOff& o, const float* base) {
  BlockDev b;
  if (o.cross) { b.xq_wp = base + o.xq_wp; b.xkv_wp = base + o.xkv_wp; }
  for (int i = 0; i < 2; ++i) {
    b.ff_ln_g[i] = base + o.ff_ln_g[i];
    b.ff_ln_b[i] = base + o.ff_ln_b[i];
    b.ff_w1p[i] = base + o.ff_w1p[i];
    b.ff_b1[i] = base + o.ff_b1[i];
    b.ff_w2p[i] = base + o.ff_w2p[i];
    b.ff_b2[i] = base + o.ff_b2[i];
  }
  b.att_ln_g = base + o.att_ln_g; b.att_ln_b = base + o.att_ln_b;
  b.qkv_wp = base + o.qkv_wp; b.qkv_b = base + o.qkv_b;
  b.out_wp = base + o.out_wp; b.out_b = base + o.out_b;
  b.cv_ln_g = base + o.cv_ln_g; b.cv_ln_b = base + o.cv_ln_b;
  b.pw1_wp = base + o.pw1_wp; b.pw1_b = base + o.pw1_b;
  if (o.split) { b.og_slabs = base + o.og_slabs; b.ff1_slabs = base + o.ff1_slabs; b.tail_slabs = base + o.tail_slabs; b.pp_ff1 = base + o.pp_ff1; b.pp_tail = base + o.pp_tail; b.pp_ff1_sc = o.pp_ff1_sc; b.pp_sw_qkv = o.pp_sw_qkv; b.pp_tail_sc[0] = o.pp_tail_sc[0]; b.pp_tail_sc[1] = o.pp_tail_sc[1]; b.pp_og = base + o.pp_og; b.pp_sw_out = o.pp_sw_out; b.pp_sw_pw1 = o.pp_sw_pw1; }
  if (o.ns) {
    b.ns_ff1_w1 = base + o.ns_ff1_w1; b.ns_ff1_w2 = base + o.ns_ff1_w2; b.ns_qkv = base + o.ns_qkv; b.ns_out = base + o.ns_out; b.ns_pw1 = base + o.ns_pw1;
    b.ns_cv_w1 = base + o.ns_cv_w1; b.ns_cv_w2 = base + o.ns_cv_w2; b.ns_ff2_w1 = base + o.ns_ff2_w1; b.ns_ff2_w2 = base + o.ns_ff2_w2;
  }
  b.att_h2[0] = o.att_h2[0]; b.att_h2[1] = o.att_h2[1]; b.att_h2[2] = o.att_h2[2];
  b.dw_w = base + o.dw_w;
  b.pc_w1p = base + o.pc_w1p; b.pc_b1 = base + o.pc_b1;
  b.bn_s = base + o.bn_s; b.bn_t = base + o.bn_t;
  b.pw2_wp = base + o.pw2_wp; b.pw2_b = base + o.pw2_b;
  b.ln_g = base + o.ln_g; b.ln_b = base + o.ln_b;
  return b;
}

// ---- stacks: Dense(d -> d) [+ blocks] [+ class head] ---------------------------------------------------------------------
void add_stack_expected(std::vector<Expected>& ex, const std::string& prefix, const std::string& blk, int nblocks,
                        int d, int H, int hs, int k, bool project, int num_classes, bool keras_mha) {
  if (project) {
    ex.push_back({prefix + "project/kernel", {d, d}});
    ex.push_back({prefix + "project/bias", {d}});
  }
  for (int i = 0; i < nblocks; ++i) add_block_expected(ex, prefix + blk + std::to_string(i), d, H, hs, k, keras_mha);
  if (num_classes > 0) {
    ex.push_back({prefix + "fully_connected/kernel", {d, num_classes}});
    ex.push_back({prefix + "fully_connected/bias", {num_classes}});
  }
}

// the class head W[d, V], b[V]: P16 pack, slab ring (dmodel 256 / 512), the dmodel-144 streams, the bias padded to whole tiles
void pack_head(mi355asr_model* m, ArenaBuilder& ab, StackOff& so, const std::vector<float>& fc, const std::vector<float>& bias, int V) {
  const int d = m->cfg.dmodel, ct = gemm_ct(d, EPI_HEAD);
  const Mat w = mat(fc, V);
  so.V = V;
  so.NT_fc = ceil_div(ceil_div(V, 16), ct) * ct;
  so.fc_w = ab.put(pack_p16(w, d, V, so.NT_fc));
  if (ring_packs_wanted(m)) put_ring_head(ab, so.fc_w, w, d, V);
  put_head_slabs(ab, so.fc_w, w, d, V, bias.data());
  so.fc_b = ab.put_padded(bias.data(), V, (size_t)so.NT_fc * 16);
}

// weights prefix + {project/*, blk<i>/*, fully_connected/*}; V = 0: no class head
StackOff pack_stack(mi355asr_model* m, ArenaBuilder& ab, const std::string& prefix, const std::string& blk, int nblocks,
                    bool project, int V, bool keras_mha) {
  const int d = m->cfg.dmodel;
  StackOff so;
  so.project = project;
  if (project) {
    const Mat pj = mat(m->host[prefix + "project/kernel"].data, d);
    const auto& pb = m->host[prefix + "project/bias"].data;
    so.proj_w = ab.put(pack_p16(pj, d, d, d / 16));
    // (bf16 mode: the one-term ring of the projection, for gemm256_bf16_kernel at many rows -- config 3's 16 640)
    if (ring_packs_wanted(m) && ab.ring_terms == 1) put_ring(ab, so.proj_w, pj, d, d, false);
    so.proj_b = ab.put(pb);
    if (d == 144) {
      std::vector<float> pp;
      so.proj_pp_sw = append_pp_plain(pp, with_bias(pj, d, pb), 1);
      so.proj_pp = ab.put(pp);
    }
  }
  for (int i = 0; i < nblocks; ++i) so.blocks.push_back(pack_block(m, ab, prefix + blk + std::to_string(i), d, m->cfg.head_size, keras_mha));
  if (V > 0) pack_head(m, ab, so, m->host[prefix + "fully_connected/kernel"].data, m->host[prefix + "fully_connected/bias"].data, V);
  return so;
}

void resolve_stack(StackDev& sd, const StackOff& so, const float* base) {
  sd.blocks.clear();
  for (const auto& o : so.blocks) sd.blocks.push_back(resolve(o, base));
  if (so.project) { sd.proj_wp = base + so.proj_w; sd.proj_b = base + so.proj_b; }
  sd.proj_pp = (so.project && so.proj_pp) ? base + so.proj_pp : nullptr;
  sd.proj_pp_sw = so.proj_pp_sw;
  if (so.V > 0) { sd.fc_wp = base + so.fc_w; sd.fc_b = base + so.fc_b; sd.NT_fc = so.NT_fc; sd.num_classes = so.V; }
}

// ---- front: STFT operands, mel, conv subsampling -------------------------------------------------------------------------
// 80 x the mel filters' largest L1 norm: the dB-normalised frontend's values lie in [-80, 0] (floor_db, relative to the
// utterance maximum); the plain Spectrogram layer hands the dB values on as they are
double db_mel_bound(const mi355asr_model* m, const std::string& prefix) {
  if (m->cfg.mel_layer_type != 0) return 80.0;
  const auto& f2m = m->host.at(prefix + "mel_layer/freq2mel").data;
  double l1 = 0.0;
  for (int mm = 0; mm < m->cfg.n_mels; ++mm) {
    double sum = 0.0;
    for (int k = 0; k < m->dm.nbins; ++k) sum += std::fabs((double)f2m[(size_t)k * m->cfg.n_mels + mm]);
    l1 = std::max(l1, sum);
  }
  return 80.0 * l1;
}

// The front whose weights are prefix + {mel_layer/*, conv_subsampling/*} (the LEAF layer's own variables aside: pack_leaf).
// mel_bound: the static bound on |mel| the two-term fp16 subsampling kernels scale by; kNoMelBound (the "valid" front's log10
// features: the scale is taken from each batch at run time, from the conv1 L1 norm and bias kept here).  lin_plain: also the
// Dense's two-term fragments in plain order.
FrontOff pack_front(mi355asr_model* m, ArenaBuilder& ab, const std::string& prefix, double mel_bound, std::vector<float>* lin_plain) {
  const auto& c = m->cfg;
  const Dims& dm = m->dm;
  const int d = c.dmodel, nb = dm.nbins;
  auto T = [&](const std::string& n) -> const std::vector<float>& { return m->host[prefix + n].data; };
  FrontOff o;
  if (c.mel_layer_type != 1) {
    const auto &re = T("mel_layer/real_kernels"), &im = T("mel_layer/imag_kernels");
    // DFT columns interleaved (re, im) per bin so that power = x^2 + y^2 / z^2 + w^2 inside one lane
    o.dft = ab.put(pack_p16(
        [&](int k, int n) { const int bin = n >> 1; return (n & 1) ? im[(size_t)k * nb + bin] : re[(size_t)k * nb + bin]; },
        c.n_dft, 2 * nb, dm.NT_dft));
    o.fft = pack_fft(ab, re, im, c.n_dft, nb);
    if (c.mel_layer_type == 0) {
      const auto& f2m = T("mel_layer/freq2mel");
      o.mel = ab.put(pack_p16([&](int k, int n) { return k < nb ? f2m[(size_t)k * c.n_mels + n] : 0.f; }, dm.KBm * 16, c.n_mels, dm.NTm));
      o.band = pack_mel_band(ab, f2m, nb, c.n_mels);
    }
  }
  const auto &w1 = T("conv_subsampling/conv1/kernel"), &b1 = T("conv_subsampling/conv1/bias");
  o.c1w = ab.put(w1);                             // [3][3][1][d] == [(i*3+j)*d + c]
  o.c1b = ab.put(b1);
  const auto& c2 = T("conv_subsampling/conv2/kernel");              // [3][3][d][d]
  // K order (c-block, kt, kf, 16): k' = (cb*9 + q)*16 + r  <->  (q = kt*3+kf, c = 16*cb + r)
  o.c2w = ab.put(pack_p16(
      [&](int kp, int n) {
        const int kb = kp / 16, r = kp % 16, cb = kb / 9, q = kb % 9;
        return c2[((size_t)q * d + (16 * cb + r)) * d + n];
      },
      9 * d, d, d / 16));
  o.c2b = ab.put(T("conv_subsampling/conv2/bias"));
  if (d == 144 || d == 256 || d == 512) {
    o.c2s = ab.put(pack_conv2_split(c2, d));       // split-bf16 fragments for subconv_split_ring_kernel
    // Two-term fp16 scheme (subconv.hip): conv2 as hi + lo of kernel * c2_ws; its operand, conv1's output, is bounded by
    // |bias| + |mel| x the filter's L1 norm; conv1 on the matrix pipe (C1M) scales the mel planes and its kernel likewise.
    // LEAF features have no bound.  MI355ASR_SUBCONV_TERMS=3: a front with a static bound does not pack the two-term form (the
    // valid front reads the switch where it takes its scale, at run time).
    static const int terms_env = (int)mi355_env("MI355ASR_SUBCONV_TERMS", 2);
    if (c.mel_layer_type != 1 && (mel_bound < 0.0 || terms_env == 2 || terms_env == 22)) {
      double bx = 0.0, wmax = 0.0, w1max = 0.0, l1max = 0.0, bmax = 0.0;
      for (int ch = 0; ch < d; ++ch) {
        double sum = 0.0;
        for (int t = 0; t < 9; ++t) sum += std::fabs((double)w1[(size_t)t * d + ch]);
        bx = std::max(bx, std::fabs((double)b1[ch]) + mel_bound * sum);
        l1max = std::max(l1max, sum);
        bmax = std::max(bmax, std::fabs((double)b1[ch]));
      }
      for (float v : w1) w1max = std::max(w1max, std::fabs((double)v));
      for (float v : c2) wmax = std::max(wmax, std::fabs((double)v));
      o.c2_ws = half_scale_for(wmax);
      if (mel_bound >= 0.0) { o.c2_hs = half_scale_for(bx); o.c1_ms = half_scale_for(mel_bound * (1.0 + 1e-6)); }
      if (o.c2_ws > 0.f && (mel_bound >= 0.0 ? o.c2_hs > 0.f : l1max > 0.0)) o.c2h = ab.put(pack_conv2_half(c2, d, o.c2_ws));
      if (mel_bound >= 0.0 || o.c2h) {
        o.c1_l1 = (float)(l1max * (1.0 + 1e-6));
        o.c1_bmax = (float)(bmax * (1.0 + 1e-6));
        o.c1_ws = half_scale_for(w1max);
      }
    }
  }
  const auto &lin = T("conv_subsampling/linear/kernel"), &lb = T("conv_subsampling/linear/bias");
  const Mat lw = mat(lin, d);
  o.lw = ab.put(pack_p16(lw, dm.F2 * d, d, d / 16));
  if (ring_packs_wanted(m)) put_ring(ab, o.lw, lw, dm.F2 * d, d, false);
  o.lb = ab.put(lb);
  if (d == 144) {
    // the same kernel for sublinear_split_kernel: 1728 fragments per 32-wide step, padded to 7 x 256 (4 floats each).  The kernel
    // takes K = F2 d that is a multiple of 32 (its launcher checks): F2 = 20 / 32 for 80 / 128 mel filters with either padding;
    // the Spectrogram layer's F2 = 129 is packed and never launched
    o.lws = ab.put(pack_linear_split(lin, dm.F2 * d, d));
    // two-term fp16 stream (pp_sublinear_kernel): chunk f = rows 144 f .. 144 f + 143 of the kernel, the bias in row 144 of chunk 0
    std::vector<float> pp;
    o.lin_pp_sw = append_pp_plain(pp, [&](int k, int n) {
      const int f = n / d, col = n - f * d;
      return k < d ? lin[((size_t)f * d + k) * d + col] : (f == 0 ? lb[col] : 0.f);
    }, dm.F2, lin_plain);
    o.lpp = ab.put(pp);
  }
  return o;
}

void resolve_front(mi355asr_model* m, const FrontOff& o, const float* base) {
  auto at = [&](size_t off) { return off ? base + off : nullptr; };
  const FftOff& fo = o.fft;
  m->dft_wp = base + o.dft; m->mel_wp = base + o.mel;
  m->fft_ok = fo.ok;
  use_mel_band(m, o.band, base);
  m->fft_w1p = base + fo.w1; m->fft_w2p = base + fo.w2; m->fft_twc = base + fo.twc; m->fft_tws = base + fo.tws;
  m->fft_w1s = base + fo.w1s; m->fft_w2s = base + fo.w2s; m->fft_w1h = base + fo.w1h; m->fft_w2h = base + fo.w2h;
  m->fft_win = base + fo.win;
  m->c1_w = base + o.c1w; m->c1_b = base + o.c1b; m->c2_wp = base + o.c2w; m->c2_b = base + o.c2b;
  m->c2_wsplit = at(o.c2s);
  m->c2_whalf = at(o.c2h); m->c2_hscale = o.c2_hs; m->c2_wscale = o.c2_ws;
  m->c1_l1 = o.c1_l1; m->c1_bmax = o.c1_bmax; m->c1_mscale = o.c1_ms; m->c1_wscale = o.c1_ws;
  m->lin_wp = base + o.lw; m->lin_b = base + o.lb;
  m->lin_wsplit = at(o.lws);
  m->lin_pp = at(o.lpp); m->lin_pp_sw = o.lin_pp_sw;
}

// the packed arena onto the device, and the ring / head-stream tables that point into it
int upload_arena(mi355asr_model* m, const ArenaBuilder& ab, hipStream_t s) {
  if (m->arena) { (void)hipFree(m->arena); m->arena = nullptr; }
  HIP_TRY(hipMalloc((void**)&m->arena, ab.buf.size() * sizeof(float)));
  m->arena_floats = ab.buf.size();
  HIP_TRY(hipMemcpyAsync(m->arena, ab.buf.data(), ab.buf.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // ab.buf is freed when the caller returns
  m->ring_of.clear();
  register_rings(m, ab, m->arena);
  return 0;
}



// ---- LEAF frontend (mel_layer_type 1) ------------------------------------------------------------------------------------
struct LeafOff { size_t wp = 0, wsplit = 0, gcoef = 0, alpha = 0, delta = 0, root = 0, smooth = 0, gamma = 0, beta = 0; };
static LeafOff pack_leaf(mi355asr_model* m, ArenaBuilder& ab) {
  // Gabor filters from (center, sigma) with the layer's constraint (convolution.py:137-153, impulse_responses.py:39-64)
  const int K = 401, NF = m->cfg.n_mels;
  const auto& gk = m->host["mel_layer/tfbanks_complex_conv/kernel"].data;
  const double pi = 3.14159265358979323846, s2l2 = std::sqrt(2.0 * std::log(2.0));
  std::vector<double> re((size_t)NF * K), im((size_t)NF * K);
  for (int f = 0; f < NF; ++f) {
    const double mu = std::min(std::max((double)gk[2 * f], 0.0), pi);
    const double sg = std::min(std::max((double)gk[2 * f + 1], 4.0 * s2l2 / pi), K * s2l2 / pi);
    const double den = 1.0 / (std::sqrt(2.0 * pi) * sg);
    for (int t = 0; t < K; ++t) {
      const double tt = t - K / 2, gs = std::exp(-tt * tt / (2.0 * sg * sg));
      re[(size_t)f * K + t] = den * std::cos(mu * tt) * gs;
      im[(size_t)f * K + t] = den * std::sin(mu * tt) * gs;
    }
  }
  LeafOff o;
  o.wp = ab.put(pack_p16([&](int k, int n) { return k < K ? (float)((n & 1) ? im[(size_t)(n >> 1) * K + k] : re[(size_t)(n >> 1) * K + k]) : 0.f; },
                         26 * 16, 2 * NF, 2 * NF / 16));
  o.wsplit = ab.put(pack_leaf_split(re, im, K, m->leaf_terms ? m->leaf_terms : 3));
  const auto& ps = m->host["mel_layer/learnable_pooling/kernel"].data;
  std::vector<float> gc(NF);
  for (int f = 0; f < NF; ++f) {           // impulse_responses.gaussian_lowpass (:103-119), as exp2 coefficients
    const double sg = std::min(std::max((double)ps[f], 2.0 / K), 0.5);
    const double den = sg * 0.5 * (K - 1);
    gc[f] = (float)(-0.5 * 1.4426950408889634 / (den * den));
  }
  o.gcoef = ab.put(gc);
  o.alpha = ab.put(m->host["mel_layer/PCEN/alpha"].data);
  o.delta = ab.put(m->host["mel_layer/PCEN/delta"].data);
  o.root = ab.put(m->host["mel_layer/PCEN/root"].data);
  o.smooth = ab.put(m->host["mel_layer/PCEN/EMA/smooth"].data);
  o.gamma = ab.put(m->host["mel_layer/tfbanks_instancenorm/gamma"].data);
  o.beta = ab.put(m->host["mel_layer/tfbanks_instancenorm/beta"].data);
  const auto& pk = m->host["mel_layer/tfbanks_preemp/kernel"].data;
  m->leaf_p0 = pk[0]; m->leaf_p1 = pk[1];
  return o;
}
static void resolve_leaf(mi355asr_model* m, const LeafOff& o, const float* base) {
  m->leaf_wp = base + o.wp; m->leaf_wsplit = base + o.wsplit; m->leaf_gcoef = base + o.gcoef; m->leaf_alpha = base + o.alpha;
  m->leaf_delta = base + o.delta; m->leaf_root = base + o.root; m->leaf_smooth = base + o.smooth; m->leaf_gamma = base + o.gamma;
  m->leaf_beta = base + o.beta;
}

}  // namespace mi355

extern "C" {

// test hook (not in the public header): the host's fp16 rounding of the two-term scheme's weight packs
void mi355asr_test_f16_rne(const float* in, int32_t n, uint16_t* half_bits, float* back) {
  for (int i = 0; i < n; ++i) { half_bits[i] = f16_rne(in[i]); back[i] = f16_to_float(half_bits[i]); }
}

int mi355asr_set_expected_rows(mi355asr_model* m, int64_t rows) {
  if (!m) return fail(MI355ASR_EINVAL, "null handle");
  if (m->finalized) return fail(MI355ASR_ESTATE, "mi355asr_set_expected_rows must come before mi355asr_finalize_weights");
  m->expected_rows = rows < 0 ? -1 : (long)std::min<int64_t>(rows, 1L << 40);
  return 0;
}
int mi355asr_num_weights(const mi355asr_model* m) { return m ? (int)m->expected.size() : 0; }
const char* mi355asr_weight_name(const mi355asr_model* m, int32_t i) {
  if (!m || i < 0 || i >= (int)m->expected.size()) return nullptr;
  return m->expected[i].name.c_str();
}

int mi355asr_weight_shape(const mi355asr_model* m, int32_t i, int32_t* rank, int64_t* dims, int32_t max_rank) {
  if (!m || !rank || i < 0 || i >= (int)m->expected.size()) return fail(MI355ASR_EINVAL, "weight index %d out of range", i);
  const auto& d = m->expected[i].dims;
  *rank = (int32_t)d.size();
  if ((int)d.size() > max_rank || (!dims && !d.empty())) return fail(MI355ASR_EINVAL, "dims array too small for rank %d", (int)d.size());
  for (size_t k = 0; k < d.size(); ++k) dims[k] = d[k];
  return 0;
}

int mi355asr_load_weight(mi355asr_model* m, const char* name, const float* data, int32_t rank, const int64_t* dims) {
  if (!m || !name || !data || rank < 0 || (rank > 0 && !dims)) return fail(MI355ASR_EINVAL, "null argument");
  const Expected* e = nullptr;
  for (const auto& x : m->expected)
    if (x.name == name) { e = &x; break; }
  if (!e) return fail(MI355ASR_EWEIGHT, "unknown weight '%s' for this configuration", name);
  // compare shapes with singleton axes squeezed (Keras keeps [n_dft,1,1,nb], [1,d,2d], [k,d,1])
  std::vector<int64_t> got, want;
  int64_t n = 1;
  for (int i = 0; i < rank; ++i) { n *= dims[i]; if (dims[i] != 1) got.push_back(dims[i]); }
  for (auto v : e->dims) if (v != 1) want.push_back(v);
  if (got != want || n != e->numel()) {
    std::string gs, ws_;
    for (int i = 0; i < rank; ++i) gs += (i ? "," : "") + std::to_string(dims[i]);
    for (size_t i = 0; i < e->dims.size(); ++i) ws_ += (i ? "," : "") + std::to_string(e->dims[i]);
    return fail(MI355ASR_EWEIGHT, "weight '%s': shape [%s] does not match expected [%s]", name, gs.c_str(), ws_.c_str());
  }
  HostTensor& t = m->host[name];
  t.data.assign(data, data + n);
  t.set = true;
  m->finalized = false;
  return 0;
}

int mi355asr_load_weight_typed(mi355asr_model* m, const char* name, const void* data, int32_t dtype, int32_t rank,
                               const int64_t* dims) {
  if (!data || rank < 0 || (rank > 0 && !dims)) return fail(MI355ASR_EINVAL, "null argument");
  if (dtype == MI355ASR_DT_F32) return mi355asr_load_weight(m, name, (const float*)data, rank, dims);
  int64_t n = 1;
  for (int i = 0; i < rank; ++i) n *= dims[i];
  if (n < 0 || n > ((int64_t)1 << 32)) return fail(MI355ASR_EINVAL, "weight '%s': bad element count", name ? name : "?");
  std::vector<float> v((size_t)n);
  if (dtype == MI355ASR_DT_F64) {
    const double* p = (const double*)data;
    for (int64_t i = 0; i < n; ++i) v[i] = (float)p[i];
  } else if (dtype == MI355ASR_DT_BF16) {
    const uint16_t* p = (const uint16_t*)data;
    for (int64_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)p[i] << 16; std::memcpy(&v[i], &u, 4); }
  } else if (dtype == MI355ASR_DT_F16) {
    const uint16_t* p = (const uint16_t*)data;
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t h = p[i], sign = (h & 0x8000u) << 16, e = (h >> 10) & 31, f = h & 1023;
      uint32_t u;
      if (e == 0) {
        if (f == 0) u = sign;
        else {                                           // subnormal half: normalise
          int sh = 0;
          uint32_t ff = f;
          while (!(ff & 1024)) { ff <<= 1; ++sh; }
          u = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((ff & 1023) << 13);
        }
      } else if (e == 31) u = sign | 0x7f800000u | (f << 13);
      else u = sign | ((e + 112) << 23) | (f << 13);
      std::memcpy(&v[i], &u, 4);
    }
  } else {
    return fail(MI355ASR_EINVAL, "weight '%s': unknown dtype %d", name ? name : "?", dtype);
  }
  return mi355asr_load_weight(m, name, v.data(), rank, dims);
}

int mi355asr_finalize_weights(mi355asr_model* m, void* stream) {
  if (!m) return fail(MI355ASR_EINVAL, "null model handle");
  for (const auto& e : m->expected)
    if (!m->host.count(e.name) || !m->host[e.name].set) return fail(MI355ASR_EWEIGHT, "missing weight '%s'", e.name.c_str());
  hipStream_t s = (hipStream_t)stream;
  if (m->is_chunk) return finalize_chunk(m, s);
  if (m->is_translator) return finalize_translator(m, s);
  if (m->is_vad) return finalize_vad(m, s);
  if (m->is_punc) return finalize_punc(m, s);
  const auto& c = m->cfg;
  const int d = c.dmodel;
  ArenaBuilder ab;
  ab.ring_terms = c.gemm_dtype == 1 ? 1 : 3;
  LeafOff lo;
  FrontOff fo;
  size_t o_lns = 0;
  std::vector<BlockOff> eo;
  if (c.has_encoder) {
    if (c.mel_layer_type == 1) lo = pack_leaf(m, ab);
    std::vector<float> lin_plain;
    fo = pack_front(m, ab, "", c.mel_layer_type == 1 ? kNoMelBound : db_mel_bound(m, ""), &lin_plain);
    if (fo.lpp) o_lns = ab.put(lin_plain);         // (fused_ns.hip: the Dense of small batches)
    for (int i = 0; i < c.num_blocks; ++i) eo.push_back(pack_block(m, ab, "conformer_block_" + std::to_string(i), d, c.head_size));
  }
  struct WavOff { size_t cw, cb, w5, b5, w1, b1, ws, bs; };
  std::vector<WavOff> wo;
  size_t o_wdw = 0, o_wpw = 0, o_wb = 0, o_wfw = 0, o_wfb = 0;
  if (c.has_encoder && c.add_wav_info) {
    // a Conv1D kernel [k, cin, cout] is already the [k*cin, cout] matrix of the GEMM over k overlapping channels-last rows
    auto conv_w = [&](const std::string& name, int K, int N) { return ab.put(pack_p16(mat(m->host[name].data, N), K, N, N / 16)); };
    o_wdw = ab.put(m->host["wav_layer/sep_conv/depthwise_kernel"].data);
    o_wpw = ab.put(m->host["wav_layer/sep_conv/pointwise_kernel"].data);
    o_wb = ab.put(m->host["wav_layer/sep_conv/bias"].data);
    for (size_t i = 0; i < m->wp_stages.size(); ++i) {
      const auto& st = m->wp_stages[i];
      const std::string n = std::to_string(i + 1);
      WavOff w{};
      w.cw = conv_w("wav_layer/conv_" + n + "/kernel", 3 * st.cin, st.c);
      w.cb = ab.put(m->host["wav_layer/conv_" + n + "/bias"].data);
      w.w5 = conv_w("wav_layer/res_" + n + "/conv5/kernel", 5 * st.c, st.c);
      w.b5 = ab.put(m->host["wav_layer/res_" + n + "/conv5/bias"].data);
      w.w1 = conv_w("wav_layer/res_" + n + "/conv1/kernel", st.c, st.c);
      w.b1 = ab.put(m->host["wav_layer/res_" + n + "/conv1/bias"].data);
      w.ws = conv_w("wav_layer/res_" + n + "/shortcut/kernel", st.c, st.c);
      w.bs = ab.put(m->host["wav_layer/res_" + n + "/shortcut/bias"].data);
      wo.push_back(w);
    }
    o_wfw = conv_w("wav_layer/final/kernel", 7 * m->wp_stages.back().c, d);
    o_wfb = ab.put(m->host["wav_layer/final/bias"].data);
  }
  StackOff co;
  if (c.num_classes > 0) co = pack_stack(m, ab, "", "decoder_conformer_block_", c.ctc_num_blocks, true, c.num_classes, false);
  if (int rc = upload_arena(m, ab, s)) return rc;
  const float* base = m->arena;
  if (c.has_encoder) {
    resolve_front(m, fo, base);
    m->lin_ns = o_lns ? base + o_lns : nullptr;
    if (c.mel_layer_type == 1) resolve_leaf(m, lo, base);
  }
  m->wp_dw = base + o_wdw; m->wp_pw = base + o_wpw; m->wp_b = base + o_wb; m->wp_fw = base + o_wfw; m->wp_fb = base + o_wfb;
  for (size_t i = 0; i < wo.size(); ++i) {
    auto& st = m->wp_stages[i];
    st.cw = base + wo[i].cw; st.cb = base + wo[i].cb; st.w5 = base + wo[i].w5; st.b5 = base + wo[i].b5;
    st.w1 = base + wo[i].w1; st.b1 = base + wo[i].b1; st.ws = base + wo[i].ws; st.bs = base + wo[i].bs;
  }
  if (m->arena16) { (void)hipFree(m->arena16); m->arena16 = nullptr; }
  if (c.gemm_dtype == 1) {
    const size_t n16 = (m->arena_floats + 3) & ~(size_t)3;
    HIP_TRY(hipMalloc((void**)&m->arena16, n16 * sizeof(unsigned short)));
    if (launch_to_bf16(m->arena, m->arena16, m->arena_floats & ~(size_t)3, s) != 0) return fail(MI355ASR_EINVAL, "bf16 conversion failed");
    HIP_TRY(hipStreamSynchronize(s));
  }
  m->enc_blocks.clear();
  for (auto& o : eo) m->enc_blocks.push_back(resolve(o, base));
  resolve_stack(m->ctc, co, base);
  m->ctc.opts.ksz = c.ctc_kernel_size;
  m->ctc.opts.fc = c.ctc_fc_factor;
  m->finalized = true;
  return 0;
}

}  // extern "C"
