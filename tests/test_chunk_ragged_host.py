"""Ragged ChunkConformer batches, the host side: the per-utterance geometry against the shapes the oracle's
front end produces, the two facts on the float64 oracle that motivate the feature, and ChunkASR.offline_stt_batch on a stub runner."""
import numpy as np
import pytest

from chunk_ragged import COMBOS, HOP, L_for, PARITIES, RESIDUES, TOL, geometry_for
from helpers import co


def _front_cfg():
    # the front end alone, on a narrow model: its shapes do not depend on dmodel
    return dict(co.CHUNK_S, dmodel=16, num_heads=1, head_size=16, enc_num_blocks=0, picker_num_blocks=0, helper_num_blocks=0,
                decoder_num_blocks=0, picker_num_classes=4, decoder_num_classes=4)


def test_geometry_equals_the_shapes_of_the_oracle_front():
    """chunk_ragged_geometry(L) == the mel frames and encoder frames co.chunk_front produces, for every L in 321 .. 2000 and a few
    up to 480 000; below 2 hop + 1 samples it refuses"""
    from tensorflowasr_amd.models import chunk_ragged_geometry
    cfg = _front_cfg()
    w = co.chunk_weights(cfg, seed=0)
    rng = np.random.default_rng(0)
    for L in list(range(321, 2001)) + [2560, 16000, 48161, 159999, 160000, 160001, 479999, 480000]:
        mel, front = co.chunk_front(rng.standard_normal((1, L)), w, cfg)
        g = chunk_ragged_geometry(L)
        assert (g["F"], g["T"]) == (mel.shape[1], front.shape[1]), (L, g, mel.shape, front.shape)
        assert g["T1"] == (g["F"] + 4 - 3) // 2 + 1 and g["T"] == (g["T1"] - 3) // 2 + 1
    for L in (0, 1, 160, 320):
        with pytest.raises(ValueError):
            chunk_ragged_geometry(L)
    assert chunk_ragged_geometry(321) == dict(F=3, T1=3, T=1)


def test_length_constructor_hits_the_T_it_names():
    """L_for(T, parity, residue) has exactly T encoder frames, the parities of F and T1 it names and L mod hop == residue, for
    T = 1 .. 100 in all four parities and three residues; no two of them coincide"""
    from tensorflowasr_amd.models import chunk_ragged_geometry
    assert len(COMBOS) == 12 and len(set(COMBOS)) == 12
    seen = set()
    for T in range(1, 101):
        for par in PARITIES:
            for r in RESIDUES:
                L = L_for(T, par, r)
                g = chunk_ragged_geometry(L)
                assert g == geometry_for(T, par), (T, par, r, L, g)
                assert g["F"] % 2 == int(par[0]) and g["T1"] % 2 == int(par[1]) and L % HOP == r
                assert L >= 2 * HOP + 1 and L not in seen
                seen.add(L)
    assert L_for(1, (True, True), 1) == 2 * HOP + 1


# ---- the two facts on the oracle -----------------------------------------------------------------------------------------------
def _three():
    cfg = dict(co.CHUNK_S, enc_num_blocks=1, decoder_num_classes=300)
    w = co.chunk_weights(cfg, seed=3)
    lens = [24000, 16123, 9000]
    x = [co.synth_wave(60 + i, n).astype(np.float64) for i, n in enumerate(lens)]
    return cfg, w, lens, x


def test_oracle_causal_stages_do_not_read_the_padding():
    """junk in the padding of a batch leaves front / enc / picker_hidden / picker_logits of every valid row where the utterance
    alone puts them, to 1e-12 -- and the picker then picks frames of the padding: the batched call decodes junk as speech"""
    cfg, w, lens, x = _three()
    rng = np.random.default_rng(1)
    batch = 3.0 * rng.standard_normal((3, max(lens)))
    for b, xx in enumerate(x):
        batch[b, :len(xx)] = xx
    r = co.chunk_predict(batch, w, cfg)
    for b, xx in enumerate(x):
        solo = co.chunk_predict(xx[None], w, cfg)
        T = solo["front"].shape[1]
        for k in ("front", "enc", "picker_hidden", "picker_logits"):
            assert np.abs(r[k][b, :T] - solo[k][0]).max() < 1e-12, (b, k)
        if T < r["front"].shape[1]:
            keep = r["picker_logits"][b].argmax(-1) != cfg["picker_num_classes"] - 1
            assert keep[T:].any(), "no frame of the padding was picked"


def test_oracle_zero_padded_decoder_differs_from_the_solo_decode():
    """the correct picks of every row, zero-padded to the batch maximum as feature_pick does, then helper and text decoder: the
    logits of the shorter rows differ from their solo decode by more than 100 x TOL, from row count - win_back on and not
    before; the longest row is exact"""
    cfg, w, lens, x = _three()
    hs, fc, wb = cfg["head_size"], cfg["fc_factor"], cfg["decoder_win_back"]
    solos = [co.chunk_predict(xx[None], w, cfg) for xx in x]
    counts = [int(s["counts"][0]) for s in solos]
    assert counts[0] > counts[1] > counts[2] > wb
    Tp = max(counts)
    picked = np.zeros((3, Tp, cfg["dmodel"]))
    for b, s in enumerate(solos):
        picked[b, :counts[b]] = s["picked"][0]
    _, helper = co.chunk_stack(picked, w, "helper", "block_", cfg["helper_num_blocks"], hs, cfg["helper_win_front"], cfg["helper_win_back"], fc, False, False)
    logits, _ = co.chunk_stack(helper, w, "decoder", "block_", cfg["decoder_num_blocks"], hs, cfg["decoder_win_front"], wb, fc, True, True)
    for b, s in enumerate(solos):
        c = counts[b]
        d = np.abs(logits[b, :c] - s["text_logits"][0]).max(-1)
        print("row %d: count %d, max|padded - solo| = %.3g, first differing row %s" % (b, c, d.max(), np.flatnonzero(d > 1e-9)[:1].tolist()))
        if c == Tp:
            assert d.max() < 1e-12
        else:
            assert d.max() > 100 * TOL
            assert d[:c - wb].max() < 1e-12 and d[c - wb] > 1e-9, "the difference does not start at count - win_back"


# ---- ChunkASR.offline_stt_batch on a stub runner --------------------------------------------------------------------------------
class _StubRunner:
    """predict(x, wav_lengths) -> one text frame per utterance whose class says how many samples the row has (in units of 1000),
    and a record of every call"""

    def __init__(self):
        self.calls = []

    def _stream_cfg(self):
        return 16, HOP, 4, None

    def predict(self, x, wav_lengths=None):
        import torch
        x = np.asarray(x)
        self.calls.append((x.copy(), np.asarray(wav_lengths).copy()))
        B = x.shape[0]
        logits = torch.zeros((B, 1, 64))
        for b in range(B):
            logits[b, 0, int(wav_lengths[b]) // 1000] = 1.0
        return logits, np.ones(B, np.int32)


class _StubText:
    num_classes = 64
    decoder_config = {"beam_width": 1}
    scorer = None

    def iextract(self, ids):
        return ["<%d>" % i for i in ids]


class _StubSpeech:
    sample_rate = 16000

    def load_wav(self, path):
        raise AssertionError("no paths in this test")


def _stub_asr():
    from tensorflowasr_amd.chunk_asr import ChunkASR

    class Stub(ChunkASR):
        def __init__(self):
            self.runner, self.text_featurizer, self.speech_featurizer, self.device = _StubRunner(), _StubText(), _StubSpeech(), "cpu"

        def _batch_ids(self, logits, counts):               # the decode kernels need a GPU: the arg-max on the host
            return [[int(logits[b, 0].argmax())] for b in range(logits.shape[0])]
    return Stub()


def test_offline_stt_batch_orders_cuts_and_normalises():
    """texts come back in the caller's order; the items are sorted by length and cut so that no batch holds more than
    max_batch_samples padded samples; every row is the item divided by abs(item.max()) (ChunkASR.load_wav), zero padded, with its
    own length; an item below 2 hop + 1 samples is refused before anything runs"""
    asr = _stub_asr()
    rng = np.random.default_rng(0)
    sizes = [9000, 3000, 12000, 5000, 2000, 7000]
    items = [(0.1 + 0.05 * i) * rng.standard_normal(n).astype(np.float32) for i, n in enumerate(sizes)]
    texts = asr.offline_stt_batch(items, max_batch_samples=20000)
    assert texts == ["<%d>" % (n // 1000) for n in sizes]
    calls = asr.runner.calls
    assert [c[1].tolist() for c in calls] == [[2000, 3000, 5000], [7000, 9000], [12000]]
    for x, lens in calls:
        assert x.shape == (len(lens), int(lens.max())) and x.size <= 20000
        for r, n in enumerate(lens):
            it = items[sizes.index(int(n))]
            assert np.array_equal(x[r, :n], it / np.abs(it.max())) and not x[r, n:].any()
    asr.runner.calls.clear()
    assert asr.offline_stt_batch(items) == texts and len(asr.runner.calls) == 1
    with pytest.raises(ValueError, match="item 1"):
        asr.offline_stt_batch([items[0], items[1][:320]])
