"""The stateful beam search for many live streams, without a GPU: `BeamDecoder.fork()` (`mi355asr_beam_clone`), `BeamStreams(host=True)`
(the interface of the device search on one host decoder per slot), `ChunkStreamingServer(beam_width > 1)` over the float64 oracle's
stepper, and the refusals the C entry points make before anything is launched.  Every expected value is the ONE-SHOT host search over
the frames a stream has been given so far (tests/test_host.py and tests/test_beam_lm_host.py pin that search to the reference's decoder):
"the state after k committed frames" is specified by it."""
import ctypes
import json
import os

import numpy as np
import pytest

import test_chunk_streams_host as tcs
from helpers import ROOT, pick_bias_for_ragged_counts
from test_beam_lm_host import ARPA, K, KO, VOCAB, scorer
from tensorflowasr_amd import _lib, ngram
from tensorflowasr_amd.models import BeamDecoder, BeamStreams, beam_device_limits, ctc_prefix_beam_decode

KS = np.load(os.path.join(ROOT, "tests", "golden", "beam_stateful_kat.npz"))


def stateful_cases():
    """the twelve recorded stateful cases -> (name, probs [T, V], beam, cutoff_prob, cutoff_top_n, (model, alpha, beta) or None, pieces)"""
    out = []
    for F, tag in ((K, "lm"), (KO, "orders")):
        for k, m in enumerate(json.loads(str(F["stateful_meta"]))):
            out.append(("%s%d" % (tag, k), F["st_probs_%d" % k], m["beam"], m["cutoff_prob"], m["cutoff_top_n"],
                        (m.get("model", m["order"]), m["alpha"], m["beta"]), list(m["pieces"])))
    for ci in range(4):
        V, beam, ctn, _ = [int(v) for v in KS["c%d_meta" % ci]]
        out.append(("plain%d" % ci, KS["c%d_probs" % ci][0], beam, float(KS["c%d_cp" % ci][0]), ctn, None, [int(v) for v in KS["c%d_pieces" % ci]]))
    return out


def the_scorer(sc):
    if sc is None:
        return None
    model, alpha, beta = sc
    return scorer(int(model) if str(model).isdigit() else model, alpha, beta)


def one_shot(p, beam, cp, ctn, s):
    """the one-shot host search over the frames p -> [(score, ids)], best first (no frames: the root)"""
    if len(p) == 0:
        return [(0.0, [])]
    ids, lens, sc, n = ctc_prefix_beam_decode(np.ascontiguousarray(p)[None], None, beam, cp, ctn, num_threads=1, ext_scorer=s)
    return [(float(sc[0, j]), ids[0, j, :lens[0, j]].tolist()) for j in range(n[0])]


CASES = stateful_cases()


def test_the_fixtures_are_the_twelve_recorded_cases():
    assert len(CASES) == 12 and sum(c[5] is not None for c in CASES) == 8
    assert {c[2] for c in CASES} >= {4, 16, 17, 65, 100} and any(1 in c[6] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fork_looks_ahead_and_leaves_the_original_alone(case):
    _, p, beam, cp, ctn, sc, pieces = case
    s = the_scorer(sc)
    V = p.shape[1]
    rng = np.random.default_rng(len(p) + beam)
    d = BeamDecoder([""] * V, beam, cp, ctn, ext_scorer=s)
    t = 0
    while t < len(p):
        c = min(int(rng.integers(0, 9)), len(p) - t)
        k = min(int(rng.integers(0, 9)), len(p) - t - c)
        got = d.decode_ids(p[t:t + c])
        t += c
        assert got == one_shot(p[:t], beam, cp, ctn, s), (t, "committed")
        f = d.fork()
        assert f.decode_ids(p[t:t + k]) == one_shot(p[:t + k], beam, cp, ctn, s), (t, k, "fork")
        g = f.fork()                                                   # a fork of a fork, and the first fork fed on
        if t + k < len(p):
            assert g.decode_ids(p[t + k:t + k + 1]) == one_shot(p[:t + k + 1], beam, cp, ctn, s)
        # the original, fed on afterwards, is still the search over ITS frames
        assert d.decode_ids(p[:0]) == one_shot(p[:t], beam, cp, ctn, s), (t, "after the fork")
    assert t == len(p)


def test_host_streams_equal_the_one_shot_search_at_every_tick():
    V, beam, cp, ctn = 50, 16, 0.99, 40
    s = scorer(3, 1.2, 0.3)
    rng = np.random.default_rng(21)
    frames = [rng.dirichlet(np.full(V, 0.08), size=200).astype(np.float32) for _ in range(4)]
    bs = BeamStreams(4, V, beam, cp, ctn, ext_scorer=s, max_frames=200, host=True)
    fed = [0] * 4                                                      # committed frames per slot, and where its frames start again
    start = [0] * 4
    peeks = absent = 0
    for tick in range(14):
        slots = [int(v) for v in rng.permutation(4)[:int(rng.integers(1, 5))]]
        absent += len(slots) < 4
        if tick == 6:
            bs.reset([slots[0]])                                       # a mid-way reset: the slot starts over on later frames
            start[slots[0]], fed[slots[0]] = start[slots[0]] + fed[slots[0]], 0
        x = np.full((len(slots), 12, V), np.nan, np.float32)           # rows past commit + peek are padding
        nc = rng.integers(0, 13, len(slots))
        npk = np.array([rng.integers(0, 13 - c) for c in nc])
        for i, sl in enumerate(slots):
            a = start[sl] + fed[sl]
            x[i, :nc[i] + npk[i]] = frames[sl][a:a + nc[i] + npk[i]]
        r = bs.read(bs.step(slots, x, nc, npk, is_logits=False, n_best=3))
        for i, sl in enumerate(slots):
            fed[sl] += int(nc[i])
            want = one_shot(frames[sl][start[sl]:start[sl] + fed[sl] + npk[i]], beam, cp, ctn, s)[:3]
            assert r["status"][i] == 0 and r["frames"][i] == fed[sl] and r["n_hyp"][i] == len(want)
            got = [(float(r["scores"][i, j]), r["ids"][i, j, :r["lens"][i, j]].tolist()) for j in range(len(want))]
            assert got == want, (tick, sl)
            peeks += npk[i] > 0
    assert peeks > 8 and absent > 3 and min(fed) > 5


def test_host_streams_at_capacity():
    V, beam = 12, 4
    rng = np.random.default_rng(2)
    p = rng.dirichlet(np.full(V, 0.3), size=(2, 24)).astype(np.float32)
    bs = BeamStreams(2, V, beam, 0.99, 40, max_frames=20, host=True)
    a = bs.read(bs.step([0, 1], p[:, :12], [12, 5], [0, 3], is_logits=False, n_best=4))
    assert a["frames"].tolist() == [12, 5] and a["status"].tolist() == [0, 0]
    # exactly max_frames is accepted (8 committed), one more frame is not (slot 0: 8 + 1 peek); slot 1 is untouched by that
    b = bs.read(bs.step([0, 1], p[:, 12:21], [8, 4], [1, 0], is_logits=False, n_best=4))
    assert b["status"].tolist() == [1, 0] and b["frames"].tolist() == [12, 9]
    assert [float(v) for v in b["scores"][0]] == [sc for sc, _ in one_shot(p[0, :12], beam, 0.99, 40, None)]        # the unchanged beam
    c = bs.read(bs.step([0, 1], p[:, 12:20], [8, 0], None, is_logits=False, n_best=4))
    assert c["status"].tolist() == [0, 0] and c["frames"].tolist() == [20, 9]
    assert [float(v) for v in c["scores"][0]] == [sc for sc, _ in one_shot(p[0, :20], beam, 0.99, 40, None)]
    assert [float(v) for v in c["scores"][1]] == [sc for sc, _ in one_shot(np.concatenate([p[1, :5], p[1, 12:16]]), beam, 0.99, 40, None)]
    d = bs.read(bs.step([0], p[:1, 20:21], [1], None, is_logits=False, n_best=4))
    assert d["status"].tolist() == [1] and d["frames"].tolist() == [20] and np.array_equal(d["ids"][0], c["ids"][0])
    bs.reset([0])
    e = bs.read(bs.step([0], p[:1, 20:21], [1], None, is_logits=False, n_best=4))
    assert e["status"].tolist() == [0] and e["frames"].tolist() == [1]


# ---- the server over the oracle's stepper ------------------------------------------------------------------------------
def softmax32(z):
    z = np.asarray(z, np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


class BeamOracleStepper(tcs.OracleStepper):
    """the oracle's stepper with the `beam=` of ChunkConformer.stream_step: the text rows of the tick go to the BeamStreams, the
    valid ones as committed frames, the unvalid ones (win_back > 0) as the peek"""

    def stream_step(self, st, slots, packets, n_samples=None, want_logits=False, beam=None):
        co, CFG = tcs.co, tcs.CFG
        self.calls.append(list(slots))
        out, rows = {}, []
        for s, x in zip(slots, packets):
            vp, _, vh, st.pc[s] = co.chunk_picker_stream_predict(np.asarray(x, np.float64)[None], st.pc[s], self.w, CFG)
            f, cnt = co.feature_pick(vh, vp, CFG["picker_num_classes"] - 1)
            r = {"phone_ids": vp[0].argmax(-1).astype(np.int32), "n_picked": int(cnt[0]), "n_valid": 0, "n_unvalid": 0,
                 "text_ids": np.zeros(0, np.int32)}
            lg = np.zeros((0, CFG["decoder_num_classes"]))
            if f.shape[1]:
                vt, unv, st.dc[s] = co.chunk_decoder_stream_predict(f, st.dc[s], self.w, CFG)
                if not st.win_back:
                    unv = unv[:, :0]                                   # (zeros_like(valid): not rows of the decoder)
                lg = np.concatenate([vt[0], unv[0]])
                r.update(n_valid=vt.shape[1], n_unvalid=unv.shape[1], text_ids=lg.argmax(-1).astype(np.int32))
            rows.append(lg)
            out[s] = r
        if beam is not None:
            T = max(1, max(len(lg) for lg in rows))
            x = np.full((len(slots), T, CFG["decoder_num_classes"]), np.nan, np.float32)
            for i, lg in enumerate(rows):
                x[i, :len(lg)] = softmax32(lg)
            nv = [out[s]["n_valid"] for s in slots]
            nu = [out[s]["n_unvalid"] for s in slots]
            b = beam.read(beam.step(slots, x, nv, nu if st.win_back else None, is_logits=False, n_best=1))
            for i, s in enumerate(slots):
                out[s].update(beam_ids=b["ids"][i, 0, :b["lens"][i, 0]].copy(), beam_score=float(b["scores"][i, 0]),
                              beam_status=int(b["status"][i]))
        return out


def beam_stream_call_on_the_oracle(a, w, asr, beam, s):
    """ChunkASR.stream_call's loop with a BeamDecoder of its own in place of the greedy decode of all frames: the valid rows are
    committed, the unvalid rows of the last decoder run are looked at through a fork"""
    co, CFG, W = tcs.co, tcs.CFG, tcs.W
    pc, dc = co.chunk_init_picker_caches(CFG), co.chunk_init_decoder_caches(CFG)
    Vp, Vt = CFG["picker_num_classes"], CFG["decoder_num_classes"]
    dec = BeamDecoder([""] * Vt, beam, 0.99, 40, ext_scorer=s)
    n_txt, n_unv, best, valid_ph, out = 0, 0, [], np.zeros((1, 0, Vp)), []
    for i in range(99999):
        s0, e = i * W, i * W + W
        if s0 >= len(a):
            break
        vp, _, vh, pc = co.chunk_picker_stream_predict(a[None, s0:e].astype(np.float64), pc, w, CFG)
        f, _ = co.feature_pick(vh, vp, Vp - 1)
        if f.shape[1] != 0:
            vt, unv, dc = co.chunk_decoder_stream_predict(f, dc, w, CFG)
            hyp = dec.decode_ids(softmax32(vt[0]))
            if CFG["decoder_win_back"] and unv.shape[1]:
                hyp = dec.fork().decode_ids(softmax32(unv[0]))
            n_txt, n_unv = n_txt + vt.shape[1], unv.shape[1]
            best = [t for t in hyp[0][1] if t != 0]
            valid_ph = np.concatenate([valid_ph, vp[:, vp[0].argmax(-1) != Vp - 1]], 1)
        if n_txt + n_unv == 0 or valid_ph.shape[1] == 0:
            continue
        ids, lens = co.ctc_collapse(valid_ph.argmax(-1), [valid_ph.shape[1]], Vp - 1)
        ph = [int(n) for n in np.clip(ids[0, :lens[0]], 0, None) if n != 0]
        out.append((e / 16000, " ".join(asr.phone_featurizer.iextract(ph)), "".join(asr.text_featurizer.iextract(best))))
    return out


@pytest.mark.parametrize("win_back", [8, 0])
def test_server_with_a_beam_equals_a_decoder_per_stream(win_back, monkeypatch):
    from tensorflowasr_amd.chunk_asr import ChunkStreamingServer
    monkeypatch.setattr(tcs, "CFG", dict(tcs.CFG, decoder_win_back=win_back))
    orig = tcs.co.chunk_decoder_stream_predict

    def decoder_stream_predict(f, caches, w, cfg):                     # win_back 0: the reference's zeros_like(valid) where the oracle says None
        vt, unv, new = orig(f, caches, w, cfg)
        return vt, (np.zeros_like(vt) if unv is None else unv), new
    monkeypatch.setattr(tcs.co, "chunk_decoder_stream_predict", decoder_stream_predict)
    CFG, W = tcs.CFG, tcs.W
    vocab = [" "] + [chr(0x4E00 + 7 * i) for i in range(CFG["decoder_num_classes"] - 2)]
    s = ngram.NGramScorer(0.6, 0.5, ARPA[3], vocab)
    x = tcs.gated(3, 9)
    w = tcs.co.chunk_weights(CFG, seed=3)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(CFG, w, x)
    lens = [W * 9 - 333, W * 5 + 1900, W * 7 + 1]
    audios = [x[k, :lens[k]] for k in range(3)]
    asr = tcs.recogniser()
    want = [beam_stream_call_on_the_oracle(a, w, asr, 4, s) for a in audios]
    greedy = [tcs.stream_call_on_the_oracle(a, w, asr) for a in audios]
    assert all(len(t) >= 2 for t in want) and [len(t) for t in want] == [len(t) for t in greedy]       # when a tuple is emitted does not change
    assert [(t, p) for u in want for t, p, _ in u] == [(t, p) for u in greedy for t, p, _ in u]
    stepper = BeamOracleStepper(w)
    srv = ChunkStreamingServer(asr, 3, stepper, beam_width=4, ext_scorer=s, max_text_frames=400, beam_host=True)
    assert srv.beam.host and srv.beam.beam_size == 4 and srv.beam.cutoff_prob == 0.99
    plain = ChunkStreamingServer(asr, 3, tcs.OracleStepper(w), beam_width=1)                      # the defaults: the parent's server
    assert plain.beam is None
    got, got1 = {k: [] for k in range(3)}, {k: [] for k in range(3)}
    slot_of, pos = {0: srv.open(), 1: srv.open()}, {0: 0, 1: 0, 2: 0}
    slot1 = {k: plain.open() for k in range(3)}
    rng = np.random.default_rng(5)
    for rnd in range(100):
        if rnd == 2:
            slot_of[2] = srv.open()                                    # a staggered start
        msg = {}
        for k in list(slot_of):
            n = int(rng.choice([1700, 2560, 3000, 6000]))
            msg[k] = audios[k][pos[k]:pos[k] + n]
            pos[k] += n
        back = srv.send({slot_of[k]: v for k, v in msg.items()})
        for k in list(slot_of):
            got[k] += back[slot_of[k]]
            if pos[k] >= len(audios[k]):
                got[k] += srv.close(slot_of.pop(k))
        if len(pos) == 3 and not slot_of and rnd >= 2:
            break
    for k in range(3):
        got1[k] = plain.send({slot1[k]: audios[k]})[slot1[k]] + plain.close(slot1[k])
        assert got[k] == want[k], k
        assert got1[k] == greedy[k], k
    assert any(a[2] != b[2] for k in range(3) for a, b in zip(want[k], greedy[k]))                # the beam's text is not the greedy one
    # open() resets the slot's beam: the same audio through a reused slot gives the same tuples
    sl = srv.open()
    assert srv.send({sl: audios[1]})[sl] + srv.close(sl) == want[1]


def test_server_reports_a_full_beam_state_in_the_slots_place():
    from tensorflowasr_amd.chunk_asr import BeamStateOverflow, ChunkStreamingServer

    class Stepper(tcs.CountingStepper):
        def stream_step(self, st, slots, packets, n_samples=None, want_logits=False, beam=None):
            r = super().stream_step(st, slots, packets)
            x = np.full((len(slots), 3, 40), 1 / 40, np.float32)
            b = beam.read(beam.step(slots, x, [3 if s == 0 else 1 for s in slots], None, is_logits=False))
            for i, s in enumerate(slots):
                r[s].update(n_picked=1, n_valid=1, text_ids=np.array([3], np.int32), phone_ids=np.array([1, 29, 29, 29], np.int32),
                            beam_ids=b["ids"][i, 0, :b["lens"][i, 0]], beam_score=0.0, beam_status=int(b["status"][i]))
            return r

    srv = ChunkStreamingServer(tcs.recogniser(), 2, Stepper(), beam_width=2, max_text_frames=4, beam_host=True)
    a, b = srv.open(), srv.open()
    full = np.zeros(tcs.W, np.float32)
    out = srv.tick({a: full, b: full})
    assert all(isinstance(t, tuple) for t in out.values())
    out = srv.tick({a: full, b: full})                                 # slot a: 3 + 3 frames > 4
    assert isinstance(out[a], BeamStateOverflow) and "max_text_frames = 4" in str(out[a]) and isinstance(out[b], tuple)
    with pytest.raises(ValueError, match="beam_width > 1"):
        ChunkStreamingServer(tcs.recogniser(), 2, Stepper(), ext_scorer=object())


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_constructor_names_the_device_limit():
    lim = beam_device_limits(False)
    assert (lim["max_beam"], lim["max_top_n"]) == (128, 40)
    for kw, name in ((dict(beam_size=129), "max_beam = 128"), (dict(cutoff_top_n=41), "max_top_n = 40"),
                     (dict(num_classes=lim["max_classes"] + 1), "max_classes = %d" % lim["max_classes"])):
        args = dict(n_streams=2, num_classes=50, beam_size=4, cutoff_prob=0.99, cutoff_top_n=40)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            BeamStreams(**args)
    with pytest.raises(ValueError, match="cutoff_prob"):
        BeamStreams(2, 50, 4)                                          # the reference's default 1.0 visits every class: host only
    bs = BeamStreams(2, 50, 129, cutoff_top_n=41, max_frames=8, host=True)     # ... which host=True serves
    p = np.random.default_rng(0).dirichlet(np.full(50, 0.1), size=(1, 3)).astype(np.float32)
    r = bs.read(bs.step([1], p, [3], is_logits=False, n_best=129))
    assert r["n_hyp"][0] == len(one_shot(p[0], 129, 1.0, 41, None))
    with pytest.raises(ValueError, match="n_best=130"):
        bs.step([1], p, [0], is_logits=False, n_best=130)
    with pytest.raises(ValueError, match="named twice"):
        bs.step([1, 1], np.concatenate([p, p]), [0, 0], is_logits=False)
    with pytest.raises(ValueError, match="out of range"):
        bs.step([2], p, [0], is_logits=False)


def test_c_entry_points_refuse_before_anything_is_launched():
    lib = _lib.lib()
    sb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    s = scorer(3)
    def r16(v):
        return (v + 15) & ~15
    _lib.check(lib.mi355asr_beam_streams_bytes(64, 50, 10, 40, 1500, s.handle(), 12, ctypes.byref(sb), ctypes.byref(wb)))
    assert sb.value == 64 * r16(r16(16 + 10 * 60) + 8 * (1500 * 10 + 1)) == 64 * 120640
    _lib.check(lib.mi355asr_beam_streams_bytes(64, 50, 10, 40, 1500, None, 12, ctypes.byref(sb), ctypes.byref(wb)))
    assert sb.value == 64 * r16(r16(16 + 10 * 36) + 8 * (1500 * 10 + 1)) == 64 * 120400 and wb.value >= 64 * 12 * 40 * 8
    mem = (ctypes.c_char * 512)()                                      # stands for every device pointer: nothing gets as far as reading one
    ptr = ctypes.c_void_p((ctypes.addressof(mem) + 15) & ~15)
    outs = _lib.BeamStreamsOutputs(**{k: ptr.value for k in BeamStreams.FIELDS})

    def step(V=50, beam=4, cp=0.99, ctn=40, slots=(0, 1), n_best=1, ws=1 << 30, lm=None):
        tab = (ctypes.c_int32 * len(slots))(*slots)
        return lib.mi355asr_beam_streams_step(ptr, 4, V, beam, cp, ctn, 100, lm, 0.0, 0.0, tab, len(slots), ptr, 0, ptr, None, 12, n_best, 20,
                                              ctypes.byref(outs), ptr, ws, None)
    for kw, msg in ((dict(beam=129), "max_beam=128"), (dict(ctn=41), "max_top_n=40"), (dict(V=70000), "max_classes"),
                    (dict(cp=1.0), "cutoff_prob"), (dict(n_best=5), "n_best=5"), (dict(slots=(1, 1)), "named twice"),
                    (dict(slots=(0, 4)), "out of range"), (dict(ws=1000), "workspace too small"),
                    (dict(lm=s.handle(), V=60), "language model was created for")):
        rc = step(**kw)
        assert rc != 0 and msg in lib.mi355asr_last_error().decode(), (kw, lib.mi355asr_last_error())
    assert lib.mi355asr_beam_streams_reset(ptr, 4, 50, 4, 40, 100, None, (ctypes.c_int32 * 1)(4), 1, None) != 0
    assert "out of range" in lib.mi355asr_last_error().decode()
