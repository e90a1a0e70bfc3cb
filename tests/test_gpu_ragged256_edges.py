"""The ragged dmodel-256 calls with 64-dim heads (mi355asr_ctc_forward_ragged, mi355asr_translator_forward_ragged: what the
streaming server runs every tick) with a length ON every boundary of the per-utterance attention classes, against the float64 oracle.

tests/test_gpu_stream_session.py defines a ragged row as the solo call's result and compares GPU calls with GPU calls; a length
predicate that is wrong in both launches passes there.  Here every row of a batch is compared with the oracle run on that
utterance alone, and the padding holds NaN.  attn64_class (csrc/launch.h) sends an utterance of up to 16 keys to
attention_kernel<64, 1>, 17 .. 32 to attention_lds_kernel, 33 .. 288 to attention_split64_kernel and more to attention_kernel<64, 16>
(with MI355ASR_ATTN64_SPLIT=0: attention_lds_kernel up to 272); the Translator's cross-attention has no operand bounds and takes the
online-softmax kernels with key blocks of 16 / 64 / 256 and attention_lds_kernel by (tokens, frames).  The batches of
tests/ragged256_edges.py put lengths on both sides of each of these, once per regime of the dense layers (gemm16 below 1 500 rows,
the slab ring from there, gemm256_bf16_kernel from 8 192 rows in the bf16 mode) and of the depthwise conv (dwconv_kernel<32, 8>
below 2 048 rows, dwconv_tile_kernel<32, 128> from there).  The regime is asserted from mi355asr_profile_schemes where the
schemes differ, else from the row count."""
import ctypes
import os

import numpy as np
import pytest

from helpers import _parity_log, assert_own_argmax, co, maxdiff
from ragged256_edges import (BF16_BATCHES, CTC_BATCHES, DW_TILE_MIN_M, GEMM256_MIN_M, NO_SPLIT_BATCHES, RING_MIN_M, SPLIT64,
                             TR_BATCHES, TR_T, TR_U, last_class, utterance)

pytestmark = pytest.mark.gpu

TOL = 1e-3                     # the project's contract against the float64 oracle
SOLO = 1e-4                    # a row against its solo call where the dense kernels differ, relative to max(1, max|solo|)
MAX_EXCUSED = 0.005            # of a batch's valid frames: arg-max differences the oracle's own margin cannot decide
F32, BF16X3, F16X2, BF16 = 0, 1, 2, 3                    # include/mi355asr.h: MI355ASR_SCHEME_*
DENSE = ("ffn", "qkv", "attn_out", "pw1_glu", "conv_tail")          # the categories launch_gemm16 runs for a block's B * T rows

_STATE = {}
_ORACLE = {}


def _np(t):
    return t.cpu().numpy()


# ---- models and oracles: one of each per module -------------------------------------------------------------------------------
def _ctc(mode):
    """fp32: two blocks, so that one block's padding rows feed the next; bf16: the shipped single block (with two, the float32
    rounding oracle is 1.4e-3 in the mean from the float64 one and the budget below no longer resolves the mode)"""
    if mode not in _STATE:
        from tensorflowasr_amd.models import CTCDecoder
        blocks = 2 if mode == "float32" else 1
        cfg = dict(co.STREAMING_S, ctcdecoder_num_blocks=blocks)
        w = co.ctc_decoder_weights(cfg, 60, seed=3)
        m = CTCDecoder(num_classes=60, dmodel=256, num_blocks=blocks, head_size=64, num_heads=4, kernel_size=32, gemm_dtype=mode)
        m.load_weights(w, by_name=False)
        _STATE[mode] = (m, w, cfg)
    return _STATE[mode]


def _translator():
    if "tr" not in _STATE:
        from tensorflowasr_amd.models import Translator
        cfg = dict(co.STREAMING_S, translator_num_blocks=2, translator_fc_factor=0.5, translator_kernel_size=32)
        w = co.translator_weights(cfg, 60, 100, seed=11)
        t = Translator(60, 100, dmodel=256, num_blocks=2, head_size=64, num_heads=4, kernel_size=32)
        t.load_weights(w, by_name=False)
        _STATE["tr"] = (t, w, cfg)
    return _STATE["tr"]


def _ctc_oracle(n):
    """float64 logits [n, 60] of utterance(n) alone through the two-block decoder"""
    if ("ctc", n) not in _ORACLE:
        _, w, cfg = _ctc("float32")
        _ORACLE["ctc", n] = co.ctc_decoder(utterance(n)[None].astype(np.float64), w, cfg)[0]
    return _ORACLE["ctc", n]


def _bf16_oracles(n):
    """utterance(n) alone through the one-block decoder: (the rounding oracle in float64, the same in float32, the un-rounded
    float64 oracle)"""
    if ("bf16", n) not in _ORACLE:
        from caller_contract_gpu_steps import bf16_oracle
        _, w, cfg = _ctc("bfloat16")
        x = utterance(n)[None]
        r64 = bf16_oracle(lambda: co.ctc_decoder(x.astype(np.float64), w, cfg))[0]
        r32 = bf16_oracle(lambda: co.ctc_decoder(x, w, cfg, dtype=np.float32))[0]
        assert r32.dtype == np.float32 and not co.GEMM_ROUND_BF16
        _ORACLE["bf16", n] = (r64, r32.astype(np.float64), co.ctc_decoder(x.astype(np.float64), w, cfg)[0])
    return _ORACLE["bf16", n]


def _tr_inputs(tl, el):
    """token ids [U] (random valid ids past tl as well) and encoder frames [el, 256] of the pair, seeded by it: a pair has the
    same inputs in every batch"""
    rng = np.random.default_rng(1000 * tl + el)
    return rng.integers(0, 60, size=TR_U).astype(np.int32), rng.standard_normal((el, 256)).astype(np.float32)


def _tr_oracle(tl, el):
    if ("tr", tl, el) not in _ORACLE:
        _, w, cfg = _translator()
        ids, enc = _tr_inputs(tl, el)
        _ORACLE["tr", tl, el] = co.translator(ids[None, :tl], enc[None].astype(np.float64), w, cfg)[0]
    return _ORACLE["tr", tl, el]


# ---- what a call ran -----------------------------------------------------------------------------------------------------------
def _schemes(m):
    """{kernel category: MI355ASR_SCHEME_* of its last launch on this handle}"""
    from tensorflowasr_amd import _lib
    nk = len(_lib.KERNEL_NAMES)
    out = (ctypes.c_int32 * nk)()
    _lib.check(m._h.lib.mi355asr_profile_schemes(m._h.ptr, out, nk))
    return dict(zip(_lib.KERNEL_NAMES, (int(v) for v in out)))


def _assert_ctc_regime(name, sch, Tmax, lens, mode, split64):
    """The operand schemes tell the gemm16 kernels (exact fp32) from the slab ring (three bf16 terms), and the fp32 attention
    kernels from the two-term one where that is the call's last attention launch (launch_attention_ragged64 launches SPLIT64,
    LDS, then the online classes; every batch here holds an online or an LDS utterance, so the category reports fp32).  They
    cannot tell the two depthwise-conv kernels apart, nor gemm256_bf16_kernel from the one-term ring: those follow from the row
    count against the defaults 2 048 and 8 192."""
    M, kind = Tmax * len(lens), name[0]
    assert (M < RING_MIN_M) == (kind == "g") and (M < DW_TILE_MIN_M) == (kind in "gr") and (M >= GEMM256_MIN_M) == (kind == "m"), (name, M)
    if mode == "float32":
        want = F32 if kind == "g" else BF16X3
        assert all(sch[c] == want for c in DENSE), (name, M, want, {c: sch[c] for c in DENSE})
    else:
        assert all(sch[c] == BF16 for c in DENSE), (name, M, {c: sch[c] for c in DENSE})
    last = last_class([(n, n) for n in lens], split64, True)
    assert sch["attention"] == (F16X2 if last == SPLIT64 else F32), (name, last, sch["attention"])
    assert sch["dwconv"] == F32


def _padded_ctc(Tmax, lens):
    from caller_contract_gpu_steps import nan_tail
    x = np.zeros((len(lens), Tmax, 256), np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = utterance(n)
    x = nan_tail(x, lens)
    assert np.isnan(x).sum() == (x.shape[0] * Tmax - sum(lens)) * 256
    return x


def _ctc_call(name, mode, split64=True):
    """the ragged call of one batch -> (logits, arg-max) on the host, after the plain assertions every mode shares: the regime, no
    NaN, rows past each length 0 / -1, the in-kernel arg-max that of the call's own logits"""
    m = _ctc(mode)[0]
    Tmax, lens = CTC_BATCHES[name]
    x = _padded_ctc(Tmax, lens)
    lg, am = m(x, return_argmax=True, lengths=np.array(lens, np.int32))
    sch = _schemes(m)
    lg, am = _np(lg), _np(am)
    _assert_ctc_regime(name, sch, Tmax, lens, mode, split64)
    assert lg.shape == (len(lens), Tmax, 60) and am.shape == (len(lens), Tmax)
    assert not np.isnan(lg).any(), (name, mode)
    for b, n in enumerate(lens):
        assert not lg[b, n:].any() and (am[b, n:] == -1).all(), (name, mode, b, n)
        assert_own_argmax(am[b, :n], lg[b, :n])
    return m, x, lg, am


def _assert_argmax_rule(tag, rows, err):
    """the rule of helpers.assert_frames_and_ids over a whole batch.  rows: [(the call's arg-max [n], oracle logits [n, V])];
    every frame's arg-max is the oracle's unless the oracle's own margin between the two candidates is inside ten times the
    batch's measured logit error; those frames are counted, and at most 0.5 % of the batch's valid frames may be such.
    -> (excused, frames)"""
    frames, excused, decisive = 0, [], []
    for b, (am, ref) in enumerate(rows):
        ra = co.frame_argmax(ref)
        frames += ra.size
        for t in np.flatnonzero(am != ra):
            margin = float(ref[t, ra[t]] - ref[t, am[t]])
            (decisive if margin > 10 * err else excused).append((b, int(t), int(ra[t]), int(am[t]), margin))
    _parity_log({"tag": tag, "frames": frames, "logits_max_abs_err": err, "excused_frames": len(excused), "excused": excused[:20]})
    assert not decisive, "%s: arg-max differs on frames the oracle decides clearly (err %.3g): %s" % (tag, err, decisive[:10])
    assert len(excused) <= MAX_EXCUSED * frames, "%s: too many undecided frames: %d of %d" % (tag, len(excused), frames)
    return len(excused), frames


def _check_ctc_fp32(name, split64=True, solo=False):
    """test a's comparison of one batch; solo: each row also equals its solo call bit for bit -> the line it printed"""
    Tmax, lens = CTC_BATCHES[name]
    m, x, lg, am = _ctc_call(name, "float32", split64)
    worst, at = 0.0, None
    for b, n in enumerate(lens):
        err = maxdiff(lg[b, :n], _ctc_oracle(n))
        assert err < TOL, (name, b, n, err)
        if err >= worst:
            worst, at = err, n
        if solo:
            slg, sam = m(x[b:b + 1, :n], return_argmax=True)
            assert np.array_equal(lg[b, :n], _np(slg)[0]) and np.array_equal(am[b, :n], _np(sam)[0]), (name, b, n)
    excused, frames = _assert_argmax_rule(name, [(am[b, :n], _ctc_oracle(n)) for b, n in enumerate(lens)], worst)
    line = ("%s%s: %d x %d = %d rows, worst |logits - oracle| %.3g at length %d (bound %.3g), %d of %d frames excused%s"
            % (name, "" if split64 else " without the two-term attention", len(lens), Tmax, len(lens) * Tmax, worst, at, TOL, excused,
               frames, ", every row == its solo call" if solo else ""))
    print(line)
    return line


# ---- a. fp32 against the float64 oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CTC_BATCHES))
def test_ctc_edge_lengths_against_the_oracle(name):
    """per row b of the batch: logits[b, :n] within 1e-3 of co.ctc_decoder in float64 on utterance(n) alone; rows past n exactly
    0 / -1 and no NaN anywhere although the padding is NaN; the in-kernel arg-max that of the call's own logits and, over the
    batch, the oracle's on every frame the oracle decides by more than ten times the measured error (at most 0.5 % of the
    frames excused).  The regime is asserted from the operand schemes and the row count; below 1 500 rows every row is also
    its solo call bit for bit."""
    _check_ctc_fp32(name, solo=name[0] == "g")


# ---- b. the same without attention_split64_kernel --------------------------------------------------------------------------------
def no_split_leg():
    """runs in the child process of the test below"""
    assert os.environ.get("MI355ASR_ATTN64_SPLIT") == "0"
    for name in NO_SPLIT_BATCHES:
        print("RESULT " + _check_ctc_fp32(name, split64=False))


def test_ctc_edge_lengths_without_the_two_term_attention():
    """MI355ASR_ATTN64_SPLIT=0 (read once: a fresh child process): 33 .. 272 keys on attention_lds_kernel, more on
    attention_kernel<64, 16>, so 271 | 272 | 273 sit on the LDS / online boundary; g-5x289 and t-12x600 against the oracle as above"""
    import subprocess
    import sys
    code = 'import sys; sys.path.insert(0, "tests"); import test_gpu_ragged256_edges as t; t.no_split_leg()'
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MI355ASR_ATTN64_SPLIT="0"), capture_output=True, text=True,
                         timeout=600, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    print("\n".join(lines))
    assert out.returncode == 0 and len(lines) == len(NO_SPLIT_BATCHES), (out.stdout[-2000:], out.stderr[-3000:])


# ---- c. the bf16 mode against the rounding oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BF16_BATCHES)
def test_ctc_edge_lengths_bf16_against_the_rounding_oracle(name):
    """gemm_dtype = bfloat16, one block.  The reference is co.ctc_decoder in float64 with both operands of every dense layer
    rounded to bf16 (co.GEMM_ROUND_BF16).  The budget is that reference's own float32 error E_ref = |rounding oracle in float64
    - rounding oracle in float32| over all valid elements of the batch, computed here: the GPU's mean error at most 2 x E_ref's
    mean (a stable statistic), its maximum at most 4 x E_ref's maximum (the project's ceiling margin), and it is closer in the mean
    to the rounding oracle than to the un-rounded one -- it really is the bf16 path; 2 x E_ref's mean stays below the mean
    cost of the rounding itself, so the mean bound resolves the mode.  Padding, NaN and the call's own arg-max as in fp32;
    oracle ids are not compared in bf16.
    Measured on the MI355X, GPU against E_ref, mean and max: g-14x100 6.49e-4 / 6.79e-4 and 6.90e-3 / 6.67e-3; r-6x289
    7.29e-4 / 6.38e-4 and 7.04e-3 / 6.99e-3; t-12x600 7.18e-4 / 7.18e-4 and 7.47e-3 / 7.47e-3; m-16x600 7.26e-4 / 6.99e-4 and
    7.19e-3 / 7.47e-3; the GPU's mean distance to the un-rounded oracle is 3.5e-3 in all four."""
    Tmax, lens = CTC_BATCHES[name]
    _, _, lg, _ = _ctc_call(name, "bfloat16")
    got = np.concatenate([lg[b, :n].astype(np.float64) for b, n in enumerate(lens)])
    r64, r32, plain = (np.concatenate([_bf16_oracles(n)[k] for n in lens]) for k in range(3))
    e_ref, e_gpu, e_plain, cost = np.abs(r64 - r32), np.abs(got - r64), np.abs(got - plain), np.abs(r64 - plain)
    print("%s bf16: %d x %d = %d rows; GPU - rounding oracle: mean %.3g (bound 2 x %.3g), max %.3g (bound 4 x %.3g); "
          "GPU - un-rounded oracle: mean %.3g; cost of the rounding: mean %.3g"
          % (name, len(lens), Tmax, len(lens) * Tmax, e_gpu.mean(), e_ref.mean(), e_gpu.max(), e_ref.max(), e_plain.mean(), cost.mean()))
    assert 2 * e_ref.mean() < cost.mean(), "the mean budget does not resolve the bf16 mode"
    assert e_gpu.mean() <= 2 * e_ref.mean(), (name, e_gpu.mean(), e_ref.mean())
    assert e_gpu.max() <= 4 * e_ref.max(), (name, e_gpu.max(), e_ref.max())
    assert e_plain.mean() > e_gpu.mean(), (name, e_plain.mean(), e_gpu.mean())


# ---- d. the Translator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TR_BATCHES))
def test_translator_edges_against_the_oracle(name):
    """U = 48, T = 304; per row: logits[b, :tl] within 1e-3 of co.translator in float64 on the row's own tokens and frames, rows
    past tl 0 / -1, no NaN although the encoder rows past el are NaN (token ids past tl are random valid ids); the arg-max by
    the rule of the CTC test.  x-26 (1 248 token rows: the gemm16 kernels and dwconv_kernel; y-65: the ring and
    dwconv_tile_kernel): each row also within 1e-4 (relative) of its solo call, with the same arg-max."""
    from caller_contract_gpu_steps import nan_tail
    t = _translator()[0]
    pairs = TR_BATCHES[name]
    B = len(pairs)
    tl, el = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    ids, enc = np.zeros((B, TR_U), np.int32), np.zeros((B, TR_T, 256), np.float32)
    for b, (u, e) in enumerate(pairs):
        ids[b], enc[b, :e] = _tr_inputs(u, e)
    enc = nan_tail(enc, el)
    lg, am = t([ids, enc], return_argmax=True, token_lengths=tl, enc_lengths=el)
    sch = _schemes(t)
    lg, am = _np(lg), _np(am)
    # the regime: token rows below / from 1 500 (FFModules on gemm16 / the ring).  The query and key / value projections of the
    # cross-attention hold no ring pack (finalize_translator, csrc/api_translator.hip): the qkv category's last launch, the
    # key / value projection of B x 304 rows, is a gemm16 launch at 7 904 and at 19 760 rows alike.  Cross-attention has no
    # operand bounds: the fp32 kernels
    M = B * TR_U
    assert (M < RING_MIN_M) == (M < DW_TILE_MIN_M) == (name == "x-26") and B * TR_T >= RING_MIN_M
    assert sch["ffn"] == (F32 if name == "x-26" else BF16X3) and sch["qkv"] == F32 and sch["attention"] == F32, (name, sch)
    assert lg.shape == (B, TR_U, 100) and not np.isnan(lg).any()
    worst, at, solo_worst = 0.0, None, 0.0
    for b, (u, e) in enumerate(pairs):
        err = maxdiff(lg[b, :u], _tr_oracle(u, e))
        assert err < TOL, (name, b, u, e, err)
        if err >= worst:
            worst, at = err, (u, e)
        assert not lg[b, u:].any() and (am[b, u:] == -1).all(), (name, b, u, e)
        assert_own_argmax(am[b, :u], lg[b, :u])
        if name == "x-26":
            slg, sam = t([ids[b:b + 1, :u], enc[b:b + 1, :e]], return_argmax=True)
            slg = _np(slg)[0]
            rel = float(np.abs(lg[b, :u] - slg).max()) / max(1.0, float(np.abs(slg).max()))
            assert rel < SOLO, (name, b, u, e, rel)
            assert np.array_equal(am[b, :u], _np(sam)[0]), (name, b, u, e)
            solo_worst = max(solo_worst, rel)
    excused, frames = _assert_argmax_rule(name, [(am[b, :u], _tr_oracle(u, e)) for b, (u, e) in enumerate(pairs)], worst)
    print("translator %s: %d x %d tokens, %d x %d frames, worst |logits - oracle| %.3g at (tokens, frames) %s (bound %.3g), %d of %d "
          "tokens excused%s" % (name, B, TR_U, B, TR_T, worst, at, TOL, excused, frames,
                                ", against solo %.3g relative (bound %.3g)" % (solo_worst, SOLO) if name == "x-26" else ""))
