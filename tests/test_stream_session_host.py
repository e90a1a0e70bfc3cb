"""The streaming session's state machine against the reference's, without a GPU: tests/golden/stream_session_ref.json holds
what the reference's stream_asr_session.ASRSession returned on the composed recording with stub models
(tests/golden/make_stream_session_golden.py); the restated StreamingASRSession with the same stubs must reproduce every
event and every recogniser call, and the StreamingASRServer every stream's events."""
import json
import os
import sys

import numpy as np
import pytest

import vad_golden

sys.path.insert(0, vad_golden.GOLDEN)
from make_stream_session_golden import StubRecogniser, StubScorer, packets, stub_punc   # noqa: E402

from tensorflowasr_amd.stream_session import StreamingASRServer, StreamingASRSession, TaskContent   # noqa: E402


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(vad_golden.GOLDEN, "stream_session_ref.json")) as f:
        r = json.load(f)
    assert r["sha256"] == vad_golden.sha256(vad_golden.composed_i16())
    return r


def _run(pk):
    asr = StubRecogniser()
    s = StreamingASRSession(asr, StubScorer(), punc=stub_punc)
    events = [s.send(p) for p in pk]
    events.append(s.final_send())
    return events, asr.calls


@pytest.mark.parametrize("ms,n_events", [("20", 47), ("70", 51)])
def test_session_reproduces_the_reference(ref, ms, n_events):
    """every value send / final_send returns and every extract_feature / decode call, in order"""
    feed = ref["feeds"][ms]
    assert feed["final_send"] == "returned" and feed["n_events"] == n_events
    events, calls = _run(packets(vad_golden.composed_i16(), feed["samples_per_packet"]))
    assert len(events) == len(feed["events"])
    for k, (got, want) in enumerate(zip(events, feed["events"])):
        assert got == want, (k, got, want)
    assert calls == feed["calls"]
    assert sum(e is not None for e in events) == n_events
    assert {e["event_type"] for e in events if e} == {"sentence begin", "inter break", "sentence end"}


def test_feed_of_70_ms_exercises_the_zero_padding_rule(ref):
    """pieces that are not whole chunks reach extract_feature"""
    sizes = {c[1] for c in ref["feeds"]["70"]["calls"] if c[0] == "extract_feature"}
    assert {3360, 7840, 8800, 8960} <= sizes


def test_task_content_defaults():
    tc = TaskContent("s", 0.5, 16000, 5)
    assert tc.chunk_samples == 8000 and tc.wait_sil == 5 and tc.window_samples() == 2400
    assert not tc.feed(np.zeros(320, np.int16).tobytes())          # 0.02 s: no window due yet
    assert tc.frames().shape == (17, 80)
    for _ in range(200):
        tc.feed(np.ones(320, np.int16).tobytes())
    assert tc.window_samples() == 48000 and tc.frames().shape == (300, 80) and tc.frames()[0, 0] == np.float32(1 / 32768)
    tc.feed(np.zeros(100, np.int16).tobytes())
    tc2 = TaskContent("s", 0.5, 16000, 5)
    tc2.feed(np.zeros(100, np.int16).tobytes())
    with pytest.raises(ValueError):
        tc2.frames()                                                # 2 500 samples / 2 is not a whole number of 80-sample frames


def test_server_streams_equal_single_sessions():
    """5 streams fed the recording from different offsets, with gaps: each stream's events are the single session's"""
    x = vad_golden.composed_i16()
    n = 320
    offs = [0, 16000 * 7, 16000 * 13 + 160, 16000 * 21, 16000 * 30]
    feeds = [packets(x[o:o + 16000 * 25], n) for o in offs]
    want = [_run(pk)[0] for pk in feeds]
    assert sum(e is not None for w in want for e in w) > 20
    srv = StreamingASRServer(StubRecogniser(), StubScorer(), len(offs), punc=stub_punc, session="asr")
    got = [[] for _ in offs]
    pos = [0] * len(offs)
    tick = 0
    while any(p < len(f) for p, f in zip(pos, feeds)):
        pk = []
        for i, f in enumerate(feeds):
            skip = (tick + 3 * i) % 7 == 0 or pos[i] >= len(f)      # gaps: a stream without a packet this tick
            pk.append(None if skip else f[pos[i]])
            pos[i] += 0 if skip else 1
        for i, (e, p) in enumerate(zip(srv.send(pk), pk)):
            assert p is not None or e is None
            if p is not None:
                got[i].append(e)
        tick += 1
    for i, e in enumerate(srv.final_send()):
        got[i].append(e)
    for i in range(len(offs)):
        strip = lambda ev: [None if e is None else {k: v for k, v in e.items() if k != "session"} for e in ev]
        assert strip(got[i]) == strip(want[i]), i
        assert all(e["session"] == "asr_%d" % (i + 1) for e in got[i] if e)
