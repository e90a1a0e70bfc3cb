"""Ragged batches on the MI355X: utterances of different lengths in one call (mi355asr_*_ragged).  Row b must be what the call
without lengths returns for wav[b, :len[b]] alone -- pinned on the reference's own recordings, against solo GPU calls on
synthetic batches, bit for bit against the existing calls when every length is L, and invariant to its neighbours."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, co, encoder_kwargs, maxdiff, small_cfg, waves

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(V=50, num_blocks=2, seed=5, **extra):
    from tensorflowasr_amd.models import ConformerCTC
    cfg = small_cfg(num_blocks)
    w = dict(co.encoder_weights(cfg, seed=seed), **co.ctc_decoder_weights(cfg, V, seed=seed + 1))
    kw = {k: v for k, v in encoder_kwargs(cfg).items() if k != "mel_layer_type"}
    kw.update(extra)
    m = ConformerCTC(V, **kw)
    m.load_weights(w, by_name=False)
    return m


def _pad(items):
    L = max(len(x) for x in items)
    x = np.zeros((len(items), L), np.float32)
    for b, it in enumerate(items):
        x[b, :len(it)] = it
    return x, np.array([len(it) for it in items], np.int32)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_reference_recordings_in_one_call(order):
    """the reference's two recordings (67 263 and 69 456 samples) in one call, both orders: encoder and 50-class logits of each
    utterance within 1e-3 of the reference's code, greedy ids equal to its ctc_decode for both heads, padded rows defined; the
    call without lengths gives the shorter recording different results"""
    from tensorflowasr_amd.models import ConformerCTC
    from test_tf_goldens import _speech_case, _speech_wave, fixture
    fx = fixture("tf_speech.npz")
    cfg, w50, wtr = _speech_case(fx)
    tags = [("bac", "cpp")[i] for i in order]
    items = [_speech_wave(fx, t)[0] for t in tags]
    x, lens = _pad(items)
    assert sorted(lens.tolist()) == [67263, 69456]
    kw = {k: v for k, v in encoder_kwargs(cfg).items() if k != "mel_layer_type"}
    for V, w, lkey, dkey in ((50, w50, "_logits50", "_ctc_decode50"), (1332, wtr, None, "_trained_ctc_decode")):
        m = ConformerCTC(V, **kw)
        m.load_weights(w, by_name=False)
        enc, el = m.encode(x, lengths=lens)
        enc, el = _np(enc), _np(el).tolist()
        lg, am = m.ctc_logits(m.encode(x, lengths=lens)[0], return_argmax=True, lengths=np.array(el, np.int32))
        lg, am = _np(lg), _np(am)
        ids, ol = m.recognize(x, wav_lengths=lens)
        ids, ol = _np(ids), _np(ol)
        for b, t in enumerate(tags):
            T = el[b]
            assert T == fx[t + "_enc"].shape[1]
            assert maxdiff(enc[b:b + 1, :T], fx[t + "_enc"]) < 1e-3
            assert not enc[b, T:].any() and not lg[b, T:].any() and (am[b, T:] == -1).all()
            if lkey:
                assert maxdiff(lg[b:b + 1, :T], fx[t + lkey]) < 1e-3
            assert ids[b, :ol[b]].tolist() == [int(i) for i in fx[t + dkey][0] if i >= 0]
            assert (ids[b, ol[b]:] == -1).all()
        if lkey:
            short = int(np.argmin(lens))
            padded = _np(m.encode(x))[short]
            ref = fx[tags[short] + "_enc"][0]
            assert maxdiff(padded[:ref.shape[0]], ref) > 1e-3


@pytest.mark.parametrize("B,L", [(64, 160000), (12, 64000)])
def test_equal_lengths_bit_identical(B, L):
    """every length = L: the ragged calls return exactly what the existing ones do (64 x 10 s: the pair-pipelined kernels;
    12 x 4 s = 1 200 rows: the small-batch kernels)"""
    m = _model()
    x = waves(B, L, 7).astype(np.float32)
    lens = np.full(B, L, np.int32)
    enc0 = m.encode(x)
    enc1, el = m.encode(x, lengths=lens)
    assert np.array_equal(_np(enc0), _np(enc1))
    assert (_np(el) == enc0.shape[1]).all()
    lg0, am0 = m.ctc_logits(enc0, return_argmax=True)
    lg1, am1 = m.ctc_logits(enc0, return_argmax=True, lengths=_np(el))
    assert np.array_equal(_np(lg0), _np(lg1)) and np.array_equal(_np(am0), _np(am1))
    i0, l0 = m.recognize(x)
    i1, l1 = m.recognize(x, wav_lengths=lens)
    assert np.array_equal(_np(i0), _np(i1)) and np.array_equal(_np(l0), _np(l1))


LENS = [4800, 320000, 48161, 96159, 160000, 33440, 70001, 12345, 250000, 8000, 120321, 27999]


def _ragged_vs_solo(m, lens, seed):
    from tensorflowasr_amd.models import ragged_geometry
    rng = np.random.default_rng(seed)
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    x, ln = _pad(items)
    for b, n in enumerate(ln):
        x[b, n:] = 0.3                                   # whatever the padding holds must not matter
    enc, el = m.encode(x, lengths=ln)
    enc, el = _np(enc), _np(el)
    ids, ol = m.recognize(x, wav_lengths=ln)
    ids, ol = _np(ids), _np(ol)
    for b, it in enumerate(items):
        g = ragged_geometry(len(it))
        assert el[b] == g["T"]
        solo = _np(m.encode(it[None]))[0]
        assert solo.shape[0] == g["T"]
        err = maxdiff(enc[b, :g["T"]], solo) / max(1.0, float(np.abs(solo).max()))
        assert err < 1e-4, (b, len(it), err)
        assert not enc[b, g["T"]:].any()
        si, sl = m.recognize(it[None])
        assert ids[b, :ol[b]].tolist() == _np(si)[0, :_np(sl)[0]].tolist(), (b, len(it))
    return x, ln, enc, ids


def test_ragged_against_solo_calls():
    """0.3 .. 20 s, L mod hop in {0, 1, hop - 1}, odd and even F_b / T1_b, T_b < 16 and > 256, one utterance of exactly L; at
    4 000 rows (8 x 500: the small-batch kernels) and 6 000 (12 x 500: the pair-pipelined ones)"""
    from tensorflowasr_amd.models import ragged_geometry
    g = [ragged_geometry(n) for n in LENS]
    assert {n % 160 for n in LENS} >= {0, 1, 159}
    assert {x["F"] % 2 for x in g} == {0, 1} and {x["T1"] % 2 for x in g} == {0, 1}
    assert min(x["T"] for x in g) < 16 and max(x["T"] for x in g) > 256 and max(LENS) == 320000
    m = _model()
    _ragged_vs_solo(m, LENS[:8], 1)
    _ragged_vs_solo(m, LENS, 2)


def test_ragged_at_shapes_of_the_short_attention_kernel():
    """more than 4 096 rows of at most 256 frames: attention_split_kernel with k_len, and (T = 70, not folded into the tail
    kernel) dwconv_tile_kernel with t_len -- 24 utterances of 0.7 .. 10 s, then 64 of 0.7 .. 2.8 s; and one utterance of 44
    frames (the layer-at-a-time path of very few rows)"""
    from tensorflowasr_amd.models import ragged_geometry
    rng = np.random.default_rng(4)
    m = _model()
    lens = [160000] + rng.integers(10241, 160000, size=23).tolist()
    assert ragged_geometry(max(lens))["T"] == 250 and 24 * 250 > 4096
    _ragged_vs_solo(m, lens, 5)
    lens = [44800] + rng.integers(10241, 44800, size=63).tolist()
    assert ragged_geometry(max(lens))["T"] == 70 and 64 * 70 > 4096
    _ragged_vs_solo(m, lens, 6)
    # at most 48 rows (MI355ASR_SMALL_M): the layer-at-a-time launches, dwconv_kernel with t_len
    _ragged_vs_solo(m, [28000], 7)


def _translator(B_seed=0):
    from tensorflowasr_amd.models import Translator
    t = Translator(inp_classes=60, tar_classes=100, dmodel=144, num_blocks=2, head_size=36, num_heads=4, kernel_size=32)
    t._build(seed=11)
    return t


@pytest.mark.parametrize("B,U,T", [(64, 80, 250), (8, 40, 120)])
def test_translator_equal_lengths_bit_identical(B, U, T):
    """token_lengths = U and enc_lengths = T: exactly the existing call (5 120 rows: the pair-pipelined kernels; 320: small-batch)"""
    import torch
    t = _translator()
    rng = np.random.default_rng(B)
    ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
    enc = rng.standard_normal((B, T, 144)).astype(np.float32)
    lg0, am0 = t([ids, enc], return_argmax=True)
    lg1, am1 = t([ids, enc], return_argmax=True, token_lengths=np.full(B, U, np.int32), enc_lengths=np.full(B, T, np.int32))
    assert np.array_equal(_np(lg0), _np(lg1)) and np.array_equal(_np(am0), _np(am1))
    assert torch.is_tensor(am1)


@pytest.mark.parametrize("B", [6, 64])
def test_translator_ragged_against_solo(B):
    """token rows 1 .. U and encoder frames 20 .. T per utterance: logits within 1e-4 and argmax equal to the solo call on the
    utterance's own rows; rows past its tokens hold 0 / -1"""
    t = _translator()
    rng = np.random.default_rng(B + 1)
    U, T = 90, 250
    tl = rng.integers(1, U + 1, size=B).astype(np.int32)
    el = rng.integers(20, T + 1, size=B).astype(np.int32)
    tl[0], el[0] = U, T
    ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
    enc = rng.standard_normal((B, T, 144)).astype(np.float32)
    for b in range(B):
        enc[b, el[b]:] = 7.0                                # must not reach any row
    lg, am = t([ids, enc], return_argmax=True, token_lengths=tl, enc_lengths=el)
    lg, am = _np(lg), _np(am)
    for b in range(B):
        slg, sam = t([ids[b:b + 1, :tl[b]], enc[b:b + 1, :el[b]]], return_argmax=True)
        slg, sam = _np(slg)[0], _np(sam)[0]
        assert maxdiff(lg[b, :tl[b]], slg) / max(1.0, float(np.abs(slg).max())) < 1e-4, b
        assert np.array_equal(am[b, :tl[b]], sam), b
        assert not lg[b, tl[b]:].any() and (am[b, tl[b]:] == -1).all()


def test_offline_stt_batch_equals_offline_stt_wave(tmp_path):
    """ASR.offline_stt_batch (paths and arrays, several ragged batches) == [offline_stt_wave(w) for w in items]"""
    import wave
    from test_gpu_vad import _asr
    asr = _asr(tmp_path)
    rng = np.random.default_rng(12)
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (16000, 160000, 4800, 57123, 96159, 12000, 200001)]
    pcm = (np.clip(items[1], -1, 1) * 32767).astype("<i2")
    path = str(tmp_path / "u.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    items.append(path)
    want = [asr.offline_stt_wave(asr.speech_featurizer.load_wav(w) if isinstance(w, str) else w) for w in items]
    assert asr.offline_stt_batch(items) == want
    assert asr.offline_stt_batch(items, max_batch_samples=600000) == want
    assert any(p for p, _ in want)


def test_ragged_on_the_pair_pipelined_kernels_only():
    """the same below 4 096 rows with the small-batch kernels switched off (MI355ASR_NS1_MAX_M=0), in a fresh process"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_ragged as t\n"
            "t._ragged_vs_solo(t._model(), t.LENS[:8], 3)\n"
            "print('RAGGED_PP_OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, MI355ASR_NS1_MAX_M="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "RAGGED_PP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_neighbours_do_not_matter():
    """changing or permuting the other utterances leaves row b bit-identical"""
    m = _model()
    rng = np.random.default_rng(9)
    lens = [70001, 160000, 33440, 120321, 8000, 96159]
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    x, ln = _pad(items)
    enc, _ = m.encode(x, lengths=ln)
    enc = _np(enc)
    perm = [3, 0, 5, 1, 4, 2]
    xp, lp = _pad([items[i] for i in perm])
    encp = _np(m.encode(xp, lengths=lp)[0])
    for j, i in enumerate(perm):
        assert np.array_equal(encp[j], enc[i])
    other = [items[0]] + [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in lens[1:]]
    xo, lo = _pad(other)
    assert np.array_equal(_np(m.encode(xo, lengths=lo)[0])[0], enc[0])


def test_errors():
    from tensorflowasr_amd._lib import Mi355AsrError
    m = _model(num_blocks=1)
    x = waves(2, 32000, 3).astype(np.float32)
    for bad in ([0, 32000], [32001, 100], [-5, 20000]):
        with pytest.raises(Mi355AsrError, match="error -1:.*wav_len"):
            m.recognize(x, wav_lengths=np.array(bad, np.int32))
    with pytest.raises(Mi355AsrError, match="error -1:.*enc_len"):
        m.ctc_logits(m.encode(x), lengths=[0, 5])
    # a batch of at most 16 encoder frames per row has no length-aware attention kernel: refused, not run unmasked
    with pytest.raises(Mi355AsrError, match="error -1:.*ragged"):
        m.recognize(waves(2, 8000, 3).astype(np.float32), wav_lengths=np.array([8000, 4000], np.int32))
    from tensorflowasr_amd.models import ConformerCTC
    cfg = small_cfg(1)
    kw = {k: v for k, v in encoder_kwargs(cfg).items() if k != "mel_layer_type"}
    for extra, what in ((dict(mel_layer_type="leaf"), "LEAF"), (dict(add_wav_info=True), "add_wav_info"),
                        (dict(chunk_size=16000), "chunk_size"), (dict(gemm_dtype="bfloat16"), "bf16"),
                        (dict(dmodel=256, head_size=64), "dmodel")):
        mm = ConformerCTC(50, **dict(kw, **extra))
        with pytest.raises(Mi355AsrError, match="error -1:.*%s" % what):
            mm.recognize(x, wav_lengths=np.array([32000, 16000], np.int32))
    t = _translator()
    ids, enc = np.zeros((2, 40), np.int32), np.zeros((2, 60, 144), np.float32)
    for tl, el, what in (([0, 3], [60, 60], "tok_len"), ([40, 41], [60, 60], "tok_len"), ([40, 3], [61, 5], "enc_len")):
        with pytest.raises(Mi355AsrError, match="error -1:.*%s" % what):
            t([ids, enc], return_argmax=True, token_lengths=np.array(tl, np.int32), enc_lengths=np.array(el, np.int32))
    with pytest.raises(Mi355AsrError, match="error -1:.*U = 10"):
        t([ids[:, :10], enc], return_argmax=True, token_lengths=np.array([10, 3], np.int32), enc_lengths=np.array([60, 5], np.int32))
    # a switch that selects a family without lengths: refused (fresh process: the switches are read once)
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, test_gpu_ragged as t\n"
            "from tensorflowasr_amd._lib import Mi355AsrError\n"
            "m = t._model(num_blocks=1)\n"
            "try:\n"
            "    m.recognize(t.waves(2, 32000, 3).astype(np.float32), wav_lengths=np.array([32000, 16000], np.int32))\n"
            "except Mi355AsrError as e:\n"
            "    print('REFUSED', e)\n") % (ROOT, os.path.join(ROOT, "tests"))
    for env in ({"MI355ASR_ATTN_SPLIT": "0"}, {"MI355ASR_FUSED": "0"}, {"MI355ASR_SUBCONV_F32": "1", "MI355ASR_ATTN_LDS": "0"}):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600,
                           cwd=ROOT)
        assert r.returncode == 0 and "REFUSED mi355asr error -1" in r.stdout, (env, r.stdout[-2000:], r.stderr[-3000:])
