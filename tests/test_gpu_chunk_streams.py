"""Batched ChunkConformer streaming (mi355asr_chunk_streams_*, ChunkConformer.open_streams / stream_step,
ChunkStreamingServer) on the MI355X.  The standard is the project's: fp32 GPU results within 1e-3 of the float64 oracle
driven ONE STREAM AT A TIME (helpers.stream_oracle), never of another run of the code under test.

Inputs: `helpers.waves` alone gives no ragged picks in a stream (with random weights the picker's blank gap drifts with the
age of the caches), so the audio is gated -- segments of 1600 .. 6400 samples alternately at full and at 1e-3 amplitude -- and
the blank bias is taken from `pick_bias_for_ragged_counts` on the gated batch: every stream then has ticks with 0 .. 4 picks."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle.conformer_oracle as co
from helpers import chunk_config_dict, maxdiff, pick_bias_for_ragged_counts, stream_oracle, waves

pytestmark = pytest.mark.gpu

TOL = 1e-3
W = 2560                                  # wav_buf_length: chunk_num * hop
PACKETS = [30, 24, 18, 12, 20, 14]
SMALL = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=30, decoder_num_classes=40)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def gated_waves(n=6, packets=30, start=5, seed=11):
    x = waves(n, W * packets, start)
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


@functools.lru_cache(maxsize=None)
def small_case():
    """weights, the six audios (the third ends with a short packet) and the oracle's stream of each"""
    x = gated_waves()
    w = co.chunk_weights(SMALL, seed=3)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(SMALL, w, x)
    audios = [x[k, :W * PACKETS[k]] for k in range(6)]
    audios[2] = audios[2][:-1000]
    refs = [oracle_stream(a, w, SMALL) for a in audios]
    return w, audios, refs


def oracle_stream(a, w, cfg):
    n = -(-len(a) // W)
    try:
        ph, hid, txt, unv, _, _, steps = stream_oracle(a[None].astype(np.float64), w, cfg, n, W)
    except ValueError:
        # a stream whose picker never left the blank (short streams at the shipped depth): helpers.stream_oracle has no text
        # to concatenate; the phone side is the same loop
        pc, ph = co.chunk_init_picker_caches(cfg), []
        for i in range(n):
            vp, _, _, pc = co.chunk_picker_stream_predict(a[None, i * W:(i + 1) * W].astype(np.float64), pc, w, cfg)
            ph.append(vp)
        ph = np.concatenate(ph, 1)
        assert (ph[0].argmax(-1) == cfg["picker_num_classes"] - 1).all()
        V = cfg["decoder_num_classes"]
        return dict(ph=ph[0], txt=np.zeros((0, V)), unv=np.zeros((0, V)), steps=[])
    return dict(ph=ph[0], txt=txt[0], unv=unv[0], steps=steps)


def model(cfg, w):
    from tensorflowasr_amd.models import ChunkConformer
    m = ChunkConformer(chunk_config_dict(cfg), cfg["picker_num_classes"], cfg["decoder_num_classes"])
    m.load_weights(w, by_name=False)
    return m


class Track:
    """what one stream returned so far"""

    def __init__(self):
        self.ph, self.txt, self.unv, self.steps, self.picks, self.k = [], [], None, [], [], 0
        self.ph_ids, self.txt_ids, self.unv_ids = [], [], []

    def take(self, r):
        pl = r["phone_logits"].cpu().numpy()
        assert np.array_equal(r["phone_ids"], pl.argmax(-1))             # the kernel's arg-max is that of its own logits
        assert r["n_picked"] == int((r["phone_ids"] != pl.shape[-1] - 1).sum())
        self.ph.append(pl)
        self.ph_ids.append(r["phone_ids"])
        self.picks.append(r["n_picked"])
        if r["n_picked"] > 0:
            tl = r["text_logits"].cpu().numpy()
            assert tl.shape[0] == r["n_valid"] + r["n_unvalid"] and np.array_equal(r["text_ids"], tl.argmax(-1))
            self.txt.append(tl[:r["n_valid"]])
            self.txt_ids.append(r["text_ids"][:r["n_valid"]])
            self.unv, self.unv_ids = tl[r["n_valid"]:], r["text_ids"][r["n_valid"]:]
            self.steps.append((self.k, r["n_valid"]))
        else:
            assert r["n_valid"] == 0 and r["n_unvalid"] == 0 and len(r["text_ids"]) == 0
        self.k += 1

    def against(self, ref, tag):
        assert self.steps == ref["steps"], tag                          # the same picks at every tick
        ph = np.concatenate(self.ph)
        txt = np.concatenate(self.txt) if self.txt else np.zeros_like(ref["txt"])
        unv = self.unv if self.unv is not None else np.zeros_like(ref["unv"])
        assert ph.shape == ref["ph"].shape and txt.shape == ref["txt"].shape and unv.shape == ref["unv"].shape, tag
        e = (maxdiff(ph, ref["ph"]), maxdiff(txt, ref["txt"]), maxdiff(unv, ref["unv"]))
        print("%s: phone %.3g, text %.3g, unvalid %.3g" % ((tag,) + e))
        assert max(e) < TOL, (tag, e)


def run(m, state, plan, audios, n_ticks, want_logits=True):
    """plan: {stream: (slot, first tick, paused ticks)} -> {stream: Track}; a stream sends its next packet at every tick
    from its first on, except the paused ones, until its audio is used up"""
    tracks = {k: Track() for k in plan}
    for tick in range(n_ticks):
        slots, rows, who = [], [], []
        for k, (slot, first, paused) in plan.items():
            t = tracks[k]
            if tick < first or tick in paused or t.k * W >= len(audios[k]):
                continue
            slots.append(slot); rows.append(audios[k][t.k * W:(t.k + 1) * W]); who.append(k)
        if not slots:
            continue
        res = m.stream_step(state, slots, rows, want_logits=want_logits)
        for k, slot in zip(who, slots):
            tracks[k].take(res[slot])
    return tracks


def test_staggered_streams_match_the_oracle(torch_cuda):
    """Six slots; stream k opens at tick 2 k, so one tick holds streams of cache lengths 0, 8, 16, 24, 32 and decoders with
    different numbers of waiting rows; stream 1 pauses for three ticks, stream 2 ends with a short packet, stream 3 (12 packets)
    is the first to end and the sixth audio runs as a new stream in ITS slot."""
    w, audios, refs = small_case()
    m = model(SMALL, w)
    st = m.open_streams(6)
    plan = {k: (k, 2 * k, (8, 9, 10) if k == 1 else ()) for k in range(5)}
    tr = run(m, st, plan, audios, 6 + 12)                 # stream 3 is done at tick 18
    assert tr[3].k == 12 and tr[0].k == 18
    m.reset_streams(st, [3])
    plan2 = dict(plan)
    plan2[5] = (3, 0, ())
    plan2.pop(3)
    tr2 = run_continue(m, st, plan2, audios, tr, 40)
    for k in range(6):
        t = tr2[k]
        assert t.k * W >= len(audios[k]), k
        t.against(refs[k], "stream %d" % k)
    assert any(0 in t.picks for t in tr2.values())        # a tick in which a stream picks nothing (its decoder is left alone)
    assert all(set(t.picks) >= {0, 4} and len(set(t.picks)) >= 4 for t in tr2.values()), [t.picks for t in tr2.values()]


def run_continue(m, state, plan, audios, tracks, n_ticks):
    tr = {k: tracks.get(k, Track()) for k in plan}
    tr.update({k: v for k, v in tracks.items() if k not in plan})
    for tick in range(n_ticks):
        slots, rows, who = [], [], []
        for k, (slot, first, paused) in plan.items():
            t = tr[k]
            if t.k * W >= len(audios[k]):
                continue
            slots.append(slot); rows.append(audios[k][t.k * W:(t.k + 1) * W]); who.append(k)
        if not slots:
            break
        res = m.stream_step(state, slots, rows, want_logits=True)
        for k, slot in zip(who, slots):
            tr[k].take(res[slot])
    return tr


def single_stream(m, a):
    """the existing single-stream calls on one audio -> (picks per packet, phone frame ids, text frame ids valid + last unvalid)"""
    caches, caches2 = m.init_picker_caches(1), m.init_decoder_caches(1)
    picks, ph, txt, unv = [], [], [], None
    for i in range(-(-len(a) // W)):
        vp, _, vh, caches = m.picker_stream_predict(a[None, i * W:(i + 1) * W, None], caches)
        ids = vp.cpu().numpy()[0].argmax(-1)
        ph.append(ids)
        f, _ = m.feature_pick(vh, vp)
        picks.append(f.shape[1])
        if f.shape[1]:
            vt, u, caches2 = m.decoder_stream_predict(f, caches2)
            txt.append(vt.cpu().numpy()[0].argmax(-1))
            unv = u.cpu().numpy()[0].argmax(-1)
    return picks, np.concatenate(ph), np.concatenate(txt + [unv])


def margins(logits):
    s = np.sort(logits, -1)
    return s[..., -1] - s[..., -2]


def test_equal_to_the_single_stream_path(torch_cuda):
    """the same six audios through the single-stream calls: identical picks per tick, identical collapsed phone and text ids.
    A frame whose ORACLE top-2 margin is below 2e-3 (twice the contract) may differ, at most 0.5 % of the frames (the
    project's max_undecided); picks are never excused."""
    w, audios, refs = small_case()
    m = model(SMALL, w)
    st = m.open_streams(6)
    tr = run(m, st, {k: (k, 0, ()) for k in range(6)}, audios, 30)
    total = differ = 0
    for k in range(6):
        picks, ph, txt = single_stream(m, audios[k])
        assert picks == tr[k].picks, k
        bph = np.concatenate(tr[k].ph_ids)
        btxt = np.concatenate(tr[k].txt_ids + [tr[k].unv_ids])
        assert bph.shape == ph.shape and btxt.shape == txt.shape
        for got, want, ref in ((bph, ph, refs[k]["ph"]), (btxt, txt, np.concatenate([refs[k]["txt"], refs[k]["unv"]]))):
            bad = np.flatnonzero(got != want)
            assert all(margins(ref)[bad] < 2e-3), (k, bad, margins(ref)[bad])
            total += got.size; differ += bad.size
            patched = got.copy()
            patched[bad] = want[bad]
            blank = ref.shape[-1] - 1
            a_ids, a_len = co.ctc_collapse(patched[None], [patched.size], blank)
            b_ids, b_len = co.ctc_collapse(want[None], [want.size], blank)
            assert np.array_equal(a_len, b_len) and np.array_equal(a_ids, b_ids)
    print("frames %d, differing on an undecided oracle margin %d" % (total, differ))
    assert differ <= 0.005 * total


def test_a_stream_does_not_depend_on_its_neighbours(torch_cuda):
    """stream 0 over 10 ticks, bit for bit, in two runs that differ in what the other five slots hold: other audio, other
    ages, one of them reset half way; same n per tick and same slot"""
    w, audios, _ = small_case()
    m = model(SMALL, w)

    def one(order, age, reset_at):
        st = m.open_streams(6)
        others = {k: Track() for k in range(1, 6)}
        for k in range(1, 6):                                  # bring the neighbours to different ages first
            for _ in range(age[k - 1]):
                m.stream_step(st, [k], [audios[order[k - 1]][others[k].k * W:(others[k].k + 1) * W]])
                others[k].k += 1
        mine = Track()
        for tick in range(10):
            if tick == reset_at:
                m.reset_streams(st, [4])
                others[4].k = 0
            slots, rows = [0], [audios[0][tick * W:(tick + 1) * W]]
            for k in range(1, 6):
                slots.append(k); rows.append(audios[order[k - 1]][others[k].k * W:(others[k].k + 1) * W])
                others[k].k += 1
            res = m.stream_step(st, slots, rows, want_logits=True)
            mine.take(res[0])
        return mine

    a = one([1, 2, 3, 4, 5], [0, 0, 0, 0, 0], -1)
    b = one([5, 4, 1, 3, 2], [2, 0, 1, 0, 1], 5)
    assert a.steps == b.steps and len(a.txt) > 0
    assert np.array_equal(np.concatenate(a.ph), np.concatenate(b.ph))
    assert np.array_equal(np.concatenate(a.txt), np.concatenate(b.txt)) and np.array_equal(a.unv, b.unv)


def test_streamed_equals_offline(torch_cuda):
    """the point of the cache design: a stream of whole packets gives the offline predict() of the whole signal"""
    w, audios, _ = small_case()
    m = model(SMALL, w)
    st = m.open_streams(2)
    a = audios[0]
    tr = run(m, st, {0: (1, 0, ())}, {0: a}, 30)[0]
    off = m.predict(a[None], stages=True)
    ph, txt = np.concatenate(tr.ph), np.concatenate(tr.txt)
    assert maxdiff(ph, off["picker_logits"].cpu().numpy()[0]) < TOL
    n = txt.shape[0]
    assert n == off["text_logits"].shape[1] - 8
    assert maxdiff(txt, off["text_logits"].cpu().numpy()[0, :n]) < TOL


def test_shipped_configuration_at_serving_size(torch_cuda):
    """chunk_conformerS.yml's dimensions (15 encoder blocks; class counts cut to 226 / 1000 to keep the oracle quick): 64 streams
    of ages 0 .. 15 packets stepped together for 6 ticks; eight sampled streams against the oracle, all 64 sane"""
    cfg = dict(co.CHUNK_S, picker_num_classes=226, decoder_num_classes=1000)
    x = gated_waves(64, 21, 100, seed=12)
    w = co.chunk_weights(cfg, seed=4)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(cfg, w, x[:4])
    m = model(cfg, w)
    st = m.open_streams(64)
    audios = {k: x[k, :W * (6 + k % 16)] for k in range(64)}
    plan = {k: (k, 15 - k % 16, ()) for k in range(64)}      # at tick 15 stream k has heard k % 16 packets; all end at tick 21
    tr = run(m, st, plan, audios, 21)
    for k in range(64):
        t = tr[k]
        assert t.k == 6 + k % 16
        assert all(np.isfinite(p).all() for p in t.ph) and all(np.isfinite(p).all() for p in t.txt)
    ran = 0
    for k in (0, 9, 18, 27, 36, 45, 54, 63):
        tr[k].against(oracle_stream(audios[k], w, cfg), "stream %d (age %d)" % (k, k % 16))
        ran += len(tr[k].steps)
    assert ran > 8                                           # the sample exercises helper and decoder, not the picker alone


def _write_wav(path, x, sr=16000):
    import wave
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _chunk_asr_config(tmp_path, cfg):
    from tensorflowasr_amd.config import load_yaml
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensorflowasr_amd", "configs")
    c = load_yaml(os.path.join(here, "am_data.yml"))
    c.update(load_yaml(os.path.join(here, "chunk_conformerS.yml")))
    c["model_config"]["ChunkConformerEncoder"]["num_blocks"] = cfg["enc_num_blocks"]
    (tmp_path / "phones.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + ["p%d" % i for i in range(26)]) + "\n")
    (tmp_path / "chars.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4e00 + i) for i in range(36)]) + "\n")
    c["inp_config"]["vocabulary"] = str(tmp_path / "phones.txt")
    c["tar_config"]["vocabulary"] = str(tmp_path / "chars.txt")
    c["running_config"]["outdir"] = str(tmp_path / "logs")
    return c


def test_server_end_to_end(torch_cuda, tmp_path):
    """three wav files of lengths that are no multiples of 2560, sent in irregular pieces: per file exactly what
    ChunkASR.stream_call returns for it alone.  (Both run the same kernels' arg-max on fp32 logits that may differ in the last
    bits between a batch of 4 and of 4 n rows: a tuple may differ only where a frame's oracle margin is below 2e-3 -- checked
    by test_equal_to_the_single_stream_path on the same weights; here equality is asserted outright.)"""
    from tensorflowasr_amd.chunk_asr import ChunkASR, ChunkStreamingServer
    cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41)
    asr = ChunkASR(_chunk_asr_config(tmp_path, cfg), load_checkpoint=False)
    x = gated_waves(3, 24, 5)
    lens = [W * 24 - 700, W * 17 + 1234, W * 9 + 77]
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / ("u%d.wav" % k)))
        _write_wav(paths[k], x[k, :lens[k]])
    xq = [asr.load_wav(p) for p in paths]
    w = co.chunk_weights(cfg, seed=3)
    pad = np.stack([np.pad(a, (0, W * 24 - len(a))) for a in xq]).astype(np.float32)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(cfg, w, pad)
    asr.runner.load_weights(w, by_name=False)
    want = [asr.stream_call(p)["streaming"] for p in paths]
    srv = ChunkStreamingServer(asr, 4)
    slots = [srv.open() for _ in range(3)]
    got = {s: [] for s in slots}
    pos = [0, 0, 0]
    rng = np.random.default_rng(3)
    while any(pos[k] < len(xq[k]) for k in range(3)):
        msg = {}
        for k in range(3):
            if pos[k] < len(xq[k]):
                n = int(rng.integers(300, 7000))
                msg[slots[k]] = xq[k][pos[k]:pos[k] + n]
                pos[k] += n
        for s, tuples in srv.send(msg).items():
            got[s] += tuples
    for k in range(3):
        got[slots[k]] += srv.close(slots[k])
        assert len(want[k]) > 3
        assert got[slots[k]] == want[k], k
    assert sorted(srv.free) == [0, 1, 2, 3]


def test_refusals_reach_the_caller_with_their_message(torch_cuda):
    """argument checks of the C entry points, made before anything is launched"""
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.models import ConformerEncoder
    from helpers import encoder_kwargs, small_cfg
    w, audios, _ = small_case()
    m = model(SMALL, w)
    st = m.open_streams(4)
    h, lib = m._h, _lib.lib()
    pk = torch_cuda.zeros((2, W), device=h.device)
    ints = torch_cuda.zeros(64, dtype=torch_cuda.int32, device=h.device)
    outs = _lib.ChunkStreamsOutputs(n_picked=ints.data_ptr())

    def step(handle, slots, ws_bytes=None):
        tab = np.asarray(slots, np.int32)
        return lib.mi355asr_chunk_streams_step(handle, st.buf.data_ptr(), 4, tab.ctypes.data_as(ctypes.c_void_p), len(tab),
                                               pk.data_ptr(), None, ctypes.byref(outs), st.ws.data_ptr(),
                                               st.ws.numel() if ws_bytes is None else ws_bytes,
                                               ctypes.c_void_p(torch_cuda.cuda.current_stream(h.device).cuda_stream))

    def refused(rc, code, word):
        msg = lib.mi355asr_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    refused(step(h.ptr, [1, 1]), -1, "twice")
    refused(step(h.ptr, [0, 4]), -1, "out of range")
    need = ctypes.c_size_t()
    _lib.check(lib.mi355asr_chunk_streams_bytes(h.ptr, 2, None, ctypes.byref(need)))
    n4 = ctypes.c_size_t()
    _lib.check(lib.mi355asr_chunk_streams_bytes(h.ptr, 4, None, ctypes.byref(n4)))
    assert n4.value == st.ws.numel()
    refused(step(h.ptr, [0, 1], need.value - 1), -4, "workspace too small")
    enc = ConformerEncoder(**encoder_kwargs(small_cfg(1)))
    refused(step(enc._h.ptr, [0, 1]), -1, "not a ChunkConformer")
    bad = model(dict(SMALL, enc_win_back=2), co.chunk_weights(dict(SMALL, enc_win_back=2), seed=3))
    with pytest.raises(_lib.Mi355AsrError, match="win_back must be 0"):
        bad.open_streams(2)
    # and the host's own rules (models.StreamGuard)
    with pytest.raises(ValueError, match="twice"):
        m.stream_step(st, [2, 2], [audios[0][:W], audios[0][:W]])
    with pytest.raises(ValueError, match="first packet"):
        m.stream_step(st, [2], [audios[0][:1000]])
    # nothing above touched a stream: slot 0 still gives the oracle's first packet
    r = m.stream_step(st, [0], [audios[0][:W]], want_logits=True)[0]
    vp, _, _, _ = co.chunk_picker_stream_predict(audios[0][None, :W].astype(np.float64), co.chunk_init_picker_caches(SMALL), w, SMALL)
    assert maxdiff(r["phone_logits"].cpu().numpy(), vp[0]) < TOL
