"""Host side of the batched ChunkConformer streams, without a GPU: `ChunkStreamingServer` (packetising, the short last packet,
skips when nothing is picked, slot reuse, the incremental greedy text) over a stepper made of the float64 oracle's single-stream
calls, against `ChunkASR.stream_call`'s loop written with the same oracle calls; and the property of the front end that lets
the batched step treat a fresh stream like any other."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle.conformer_oracle as co
from helpers import pick_bias_for_ragged_counts, waves

W = 2560
CFG = dict(co.CHUNK_S, enc_num_blocks=1, picker_num_classes=30, decoder_num_classes=40)


class Vocab:
    def __init__(self, n, fmt):
        self.num_classes, self.fmt = n, fmt

    def iextract(self, ids):
        return [self.fmt % i for i in ids]


def recogniser():
    """what the server reads of a ChunkASR"""
    return SimpleNamespace(wav_buf_length=W, phone_featurizer=Vocab(CFG["picker_num_classes"], "p%d"),
                           text_featurizer=Vocab(CFG["decoder_num_classes"], "<%d>"),
                           speech_featurizer=SimpleNamespace(sample_rate=16000))


class OracleStepper:
    """open_streams / reset_streams / stream_step of ChunkConformer on the oracle, one stream at a time"""

    def __init__(self, w):
        self.w, self.calls = w, []

    def open_streams(self, n):
        st = SimpleNamespace(n_streams=n, win_back=CFG["decoder_win_back"], pc=[None] * n, dc=[None] * n)
        self.reset_streams(st, range(n))
        return st

    def reset_streams(self, st, slots=None):
        for s in (range(st.n_streams) if slots is None else slots):
            st.pc[s], st.dc[s] = co.chunk_init_picker_caches(CFG), co.chunk_init_decoder_caches(CFG)

    def stream_step(self, st, slots, packets, n_samples=None, want_logits=False):
        self.calls.append(list(slots))
        out = {}
        for s, x in zip(slots, packets):
            vp, _, vh, st.pc[s] = co.chunk_picker_stream_predict(np.asarray(x, np.float64)[None], st.pc[s], self.w, CFG)
            assert vp.shape[1] == 4
            f, cnt = co.feature_pick(vh, vp, CFG["picker_num_classes"] - 1)
            r = {"phone_ids": vp[0].argmax(-1).astype(np.int32), "n_picked": int(cnt[0]), "n_valid": 0, "n_unvalid": 0,
                 "text_ids": np.zeros(0, np.int32)}
            if f.shape[1]:
                vt, unv, st.dc[s] = co.chunk_decoder_stream_predict(f, st.dc[s], self.w, CFG)
                r.update(n_valid=vt.shape[1], n_unvalid=unv.shape[1],
                         text_ids=np.concatenate([vt[0], unv[0]]).argmax(-1).astype(np.int32))
            out[s] = r
        return out


def stream_call_on_the_oracle(a, w, asr):
    """ChunkASR.stream_call's loop (test_chunk_asr.py:60-100) with the oracle's calls; the text is the greedy decode of ALL
    [valid | unvalid] frames after every packet"""
    pc, dc = co.chunk_init_picker_caches(CFG), co.chunk_init_decoder_caches(CFG)
    Vp, Vt = CFG["picker_num_classes"], CFG["decoder_num_classes"]
    valid_txt, valid_ph, unv = np.zeros((1, 0, Vt)), np.zeros((1, 0, Vp)), np.zeros((1, 0, Vt))
    out = []

    def text(logits, blank):
        ids, lens = co.ctc_collapse(logits.argmax(-1), [logits.shape[1]], blank)
        return [int(n) for n in np.clip(ids[0, :lens[0]], 0, None) if n != 0]

    for i in range(99999):
        s, e = i * W, i * W + W
        if s >= len(a):
            break
        vp, _, vh, pc = co.chunk_picker_stream_predict(a[None, s:e].astype(np.float64), pc, w, CFG)
        if vp.shape[1] == 0:
            continue
        f, _ = co.feature_pick(vh, vp, Vp - 1)
        if f.shape[1] != 0:
            vt, unv, dc = co.chunk_decoder_stream_predict(f, dc, w, CFG)
            valid_txt = np.concatenate([valid_txt, vt], 1)
            valid_ph = np.concatenate([valid_ph, vp[:, vp[0].argmax(-1) != Vp - 1]], 1)
        txt = np.concatenate([valid_txt, unv], 1)
        if txt.shape[1] == 0 or valid_ph.shape[1] == 0:
            continue
        out.append((e / 16000, " ".join(asr.phone_featurizer.iextract(text(valid_ph, Vp - 1))),
                    "".join(asr.text_featurizer.iextract(text(txt, Vt - 1)))))
    return out


def gated(n, packets, seed=11):
    x = waves(n, W * packets, 5)
    rng = np.random.default_rng(seed)
    for b in range(n):
        t, is_open = 0, b % 2 == 1
        while t < x.shape[1]:
            seg = int(rng.integers(1600, 6400))
            if not is_open:
                x[b, t:t + seg] *= np.float32(1e-3)
            is_open = not is_open
            t += seg
    return x.astype(np.float32)


def test_server_over_the_oracle_equals_stream_call_per_stream():
    from tensorflowasr_amd.chunk_asr import ChunkStreamingServer
    x = gated(5, 12)
    w = co.chunk_weights(CFG, seed=3)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(CFG, w, x)
    lens = [W * 12 - 333, W * 7 + 1900, W * 9 + 1, W * 4 + 2559, W * 6 + 40]
    audios = [x[k, :lens[k]] for k in range(5)]
    asr = recogniser()
    want = [stream_call_on_the_oracle(a, w, asr) for a in audios]
    assert all(len(t) >= 2 for t in want) and len({t[-1][2] for t in want}) > 1
    stepper = OracleStepper(w)
    srv = ChunkStreamingServer(asr, 4, stepper)
    rng = np.random.default_rng(5)
    opens_at = {0: 0, 1: 0, 2: 2, 3: 3}            # round in which an audio's stream opens; audio 4 waits for a slot to come free
    pos, slot_of, got, reused = {}, {}, {k: [] for k in range(5)}, None
    for rnd in range(200):
        for k, r0 in list(opens_at.items()):
            if r0 == rnd:
                slot_of[k], pos[k] = srv.open(), 0
        msg = {}
        for k in slot_of:
            n = int(rng.choice([200, 1700, 2560, 3000, 6000, 9000]))          # less than a packet ... several at once
            msg[slot_of[k]] = audios[k][pos[k]:pos[k] + n]
            pos[k] += n
        back = srv.send(msg) if msg else {}
        for k in list(slot_of):
            got[k] += back[slot_of[k]]
            if pos[k] >= len(audios[k]):
                got[k] += srv.close(slot_of[k])
                freed = slot_of.pop(k)
                if 4 not in opens_at:
                    opens_at[4], reused = rnd + 1, freed
        if len(pos) == 5 and not slot_of:
            break
    assert len(pos) == 5 and not slot_of and reused is not None
    for k in range(5):
        assert got[k] == want[k], k
    assert any(len(c) > 1 for c in stepper.calls)              # ticks shared by several streams
    assert max(len(c) for c in stepper.calls) <= 4 and all(len(set(c)) == len(c) for c in stepper.calls)
    assert sorted(srv.free) == [0, 1, 2, 3] and not srv.streams
    # a send with several packets' worth takes several ticks inside the same call
    s = srv.open()
    n0 = len(stepper.calls)
    out = srv.send({s: audios[0][:W * 3 + 5]})
    assert len(stepper.calls) == n0 + 3 and out[s] == want[0][:len(out[s])]
    assert [t for t, _, _ in out[s]] == [t for t, _, _ in want[0] if t <= 3 * W / 16000]


def test_a_fresh_stream_is_a_stream_with_a_cache_of_zeros():
    """the front of the batched step is uniform over streams of any age because of this: valid mode left-pads n_dft - 1 zeros
    and the chunk front's dB has no maximum over frames"""
    w = co.chunk_weights(CFG, seed=3)
    x = waves(1, W, 9).astype(np.float64)
    sub = np.zeros((1, 4, 80))
    a, wa, sa = co.chunk_front_stream(x, np.zeros((1, 0)), sub, w, CFG)
    b, wb, sb = co.chunk_front_stream(x, np.zeros((1, W)), sub, w, CFG)
    assert a.shape == b.shape == (1, 4, 144)
    assert np.abs(a - b).max() < 1e-12 and np.abs(sa - sb).max() < 1e-12
    assert np.array_equal(wa, wb[:, -W:]) and wa.shape == (1, W)
    # ... and why a short FIRST packet is not taken: fewer than chunk_num mel frames, fewer rows
    c, _, _ = co.chunk_front_stream(x[:, :1000], np.zeros((1, 0)), sub, w, CFG)
    assert c.shape[1] == 2


class CountingStepper:
    """no model at all: enough for the server's own refusals"""

    def __init__(self):
        self.steps = 0

    def open_streams(self, n):
        return SimpleNamespace(n_streams=n, win_back=8)

    def reset_streams(self, st, slots=None):
        pass

    def stream_step(self, st, slots, packets, n_samples=None, want_logits=False):
        self.steps += 1
        return {s: {"phone_ids": np.full(4, 29, np.int32), "n_picked": 0, "n_valid": 0, "n_unvalid": 0,
                    "text_ids": np.zeros(0, np.int32)} for s in slots}


def test_refusals_of_the_server():
    from tensorflowasr_amd.chunk_asr import ChunkStreamingServer
    stepper = CountingStepper()
    srv = ChunkStreamingServer(recogniser(), 2, stepper)
    a, b = srv.open(), srv.open()
    with pytest.raises(RuntimeError, match="in use"):
        srv.open()                                              # a full server
    full, short = np.zeros(W, np.float32), np.zeros(1000, np.float32)
    with pytest.raises(ValueError, match="first packet"):
        srv.tick({a: short})                                    # a short first packet
    assert stepper.steps == 0
    srv.tick({a: full, b: full})
    srv.tick({a: short})
    with pytest.raises(ValueError, match="short last packet"):
        srv.tick({a: full})                                     # a packet after a short one
    with pytest.raises(ValueError, match="1 .. 2560"):
        srv.tick({b: np.zeros(W + 1, np.float32)})
    assert stepper.steps == 2
    assert srv.close(a) == []
    with pytest.raises(KeyError, match="not open"):
        srv.send({a: full})                                     # a closed slot
    with pytest.raises(KeyError):
        srv.close(a)
    c = srv.open()
    assert c == a                                               # the slot is free again, as a fresh stream
    srv.tick({c: full})
    # a stream that ends before its first full packet cannot be flushed here; its slot is freed all the same
    d = srv.close(b)
    assert d == []
    e = srv.open()
    srv.send({e: short})
    with pytest.raises(ValueError, match="first packet"):
        srv.close(e)
    assert e in srv.free


def test_init_caches_point_to_open_streams():
    """the tuple-of-tensors caches stay the single-stream contract; their refusal names the batched entry"""
    import inspect
    from tensorflowasr_amd import models
    src = inspect.getsource(models.ChunkConformer.init_picker_caches) + inspect.getsource(models.ChunkConformer.init_decoder_caches)
    assert src.count("open_streams") == 2
    g = models.StreamGuard(3, W)
    g.check([0, 2], [W, W])
    g.commit([0, 2], [W, 100])
    with pytest.raises(ValueError, match="short last packet"):
        g.check([2], [W])
    g.reset([2])
    g.check([2], [W])
    with pytest.raises(ValueError, match="out of range"):
        g.check([3], [W])
