"""Regenerates tests/golden/stream_session_ref.json: the reference's streaming ASRSession (stream_asr_session.py) run with
stub models on the ~60 s composed recording, fed in 20 ms and in 70 ms packets.

    python tests/golden/make_stream_session_golden.py /path/to/reference

Run on a machine that has the reference tree; no test reads that tree.  The reference module is imported by path with stub
modules in place of its models and configuration, so this file holds none of its text:

* scorer (vad.src.vad.VAD): sqrt(mean(x^2)) - 0.01 per 80-sample frame;
* recogniser (asr.src.asr.ASR): extract_feature(wav) returns a [1, T, 1] array with T = 13 frames per started 8 000-sample
  chunk; decode(list) returns "n" + the lengths it was given joined by "+" (five characters or more for two pieces);
* punctuation (punc_recover): appends "." so that the fixture shows where the reference applies it.

Recorded per feed: every value send / final_send returned (None included), the sample counts given to extract_feature and
the history lengths given to decode, in call order."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


class StubScorer:
    def __init__(self, *a, **k):
        pass

    def inference(self, frames):
        x = np.asarray(frames, np.float64)
        return (np.sqrt((x * x).mean(-1)) - 0.01)[..., None]


class StubRecogniser:
    def __init__(self, *a, **k):
        self.calls = []

    def compile(self, *a, **k):
        pass

    def extract_feature(self, wav):
        n = int(np.asarray(wav).reshape(-1).shape[0])
        self.calls.append(["extract_feature", n])
        return np.zeros((1, 13 * -(-n // 8000), 1), np.float32)

    def decode(self, enc_features):
        lens = [int(e.shape[1]) for e in enc_features]
        self.calls.append(["decode", lens])
        return "n" + "+".join(str(n) for n in lens)


def stub_punc(text):
    return text + "."


class StubPunc:
    def __init__(self, *a, **k):
        pass

    def punc_recover(self, text):
        return stub_punc(text)


def packets(samples_i16, n):
    return [samples_i16[i:i + n].tobytes() for i in range(0, len(samples_i16) // n * n, n)]


def load_reference(root):
    stubs = {"asr": {}, "asr.src": {}, "asr.src.asr": {"ASR": StubRecogniser}, "vad": {}, "vad.src": {},
             "vad.src.vad": {"VAD": StubScorer}, "punc_recover": {}, "punc_recover.src": {},
             "punc_recover.src.punc_recover": {"Punc": StubPunc}, "utils": {},
             "utils.user_config": {"UserConfig": lambda *a, **k: None}}
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        if "." not in name or name.count(".") == 1:
            mod.__path__ = []
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("ref_stream_asr_session",
                                                  os.path.join(root, "Inference", "PythonInference", "stream_asr_session.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(session, pk):
    events = [session.send(p) for p in pk]
    try:
        events.append(session.final_send())
        final = "returned"
    except KeyError as e:                       # the reference reads a key that only an answered inter break sets
        final = "KeyError(%s)" % e
    return events, final


def main():
    import vad_golden
    ref = load_reference(sys.argv[1])
    x = vad_golden.composed_i16()
    out = {"sha256": vad_golden.sha256(x), "feeds": {}}
    for ms, n in ((20, 320), (70, 1120)):
        s = ref.ASRSession()
        events, final = run(s, packets(x, n))
        out["feeds"][str(ms)] = {"samples_per_packet": n, "events": events, "final_send": final, "calls": s.asr.calls,
                                 "n_events": sum(e is not None for e in events)}
    with open(os.path.join(HERE, "stream_session_ref.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({k: (v["n_events"], v["final_send"]) for k, v in out["feeds"].items()})


if __name__ == "__main__":
    main()
