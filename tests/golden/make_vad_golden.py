"""Generates the VAD fixtures.  Runs ONLY where the reference checkout exists (nothing at test time reads it).

    python tests/golden/make_vad_golden.py

Outputs (tests/golden/):
  vad.onnx      the reference's trained VAD graph (Inference/PythonInference/vad/models/vad.onnx), byte for byte
  vad_ref.npz   in_test8k               the reference's vad/test.wav (8 kHz), int16 (samples = in / 32768); the other
                                        inputs are rebuilt by tests/vad_golden.py from speech_bac.wav / speech_cpp.wav:
                                        bac, cpp and composed (~60 s, pinned by meta_composed_sha256), 16 kHz
                s32_<name>, s64_<name>  the graph's scores, float32 and float64, executed node by node by
                                        oracle/onnx_mini.run (Relu and Pad supplied here); decimate 2 (wav[::2])
                                        except test8k (decimate 1)
                seg_<name>              [n, 2] segments of the reference's own OfflineVAD.vad on s32_<name>, 16 kHz
                                        buffer of T*160 samples
                syn_scores_<i>, syn_seg_<i>   seeded synthetic score sequences through the same vad()
                rec_in_<i>, rec_out_<i> segment lists through the reference's OfflineVAD.recover
                gate_*                  Session::Parase / VadInference (CppInference asr_session.cpp) executed line by
                                        line in float32 over 0.1 s pushes of the composed recording
The graph's initialisers are not repeated in the npz: tests read them from vad.onnx.
The reference's OfflineVAD class is loaded from offline_asr_session.py with `ast` and executed in place; no source
text is stored.
"""
import ast
import contextlib
import io
import os
import shutil
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import onnx_mini  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vad_golden  # noqa: E402

REF = "/root/reference"
ONNX = REF + "/Inference/PythonInference/vad/models/vad.onnx"
SESSION = REF + "/Inference/PythonInference/offline_asr_session.py"
TEST8K = REF + "/vad/test.wav"
OUT = os.path.join(ROOT, "tests", "golden")


def read_wav(path):
    with wave.open(path) as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(np.float32) / 32768.0


def graph_scores(frames, dtype):
    """vad.onnx on frames [1, T, 80] -> [T] scores, every node through onnx_mini.run except Relu / Pad."""
    nodes, inits, _, _ = onnx_mini.load(ONNX)
    env = {k: (v.astype(dtype) if v.dtype.kind == "f" else v) for k, v in inits.items()}
    env["inputs"] = frames.astype(dtype)
    for nd in nodes:
        if nd.op == "Relu":
            env[nd.outputs[0]] = np.maximum(env[nd.inputs[0]], 0)
        elif nd.op == "Pad":
            p = env[nd.inputs[1]].tolist()
            n = len(p) // 2
            env[nd.outputs[0]] = np.pad(env[nd.inputs[0]], list(zip(p[:n], p[n:])))
        else:
            env[nd.outputs[0]] = onnx_mini.run([nd], env, {}, nd.outputs)[0]
    return env["output_0"].reshape(-1)


def load_offline_vad():
    tree = ast.parse(open(SESSION).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "OfflineVAD"]
    ns = {"np": np}
    exec(compile(ast.Module(body=cls, type_ignores=[]), SESSION, "exec"), ns)
    return ns["OfflineVAD"]


class _Scores:
    def __init__(self, s):
        self.s = s

    def inference(self, data):
        assert data.shape[1] == len(self.s)
        return self.s.reshape(1, -1, 1)


def ref_segments(OfflineVAD, scores):
    v = OfflineVAD(sr=16000)
    v.compile(_Scores(np.asarray(scores, np.float32)))
    with contextlib.redirect_stdout(io.StringIO()):
        r = v.vad(np.zeros(len(scores) * 160, np.float32))
    return np.array(r, np.float64).reshape(-1, 2)


def gate_events(wav):
    """Session::Parase + VadInference, float32 where the C++ is float, over 1600-sample pushes."""
    f32 = np.float32
    wavLength, vad_point, samplerate = f32(0), f32(0), f32(16000)
    sil_times, sound_start, vad_result = 0, 0, False
    buf = np.zeros(0, np.float32)
    events, ran, starts, ends, scores = [], [], [], [], []
    for p in range(len(wav) // 1600):
        x = wav[p * 1600:(p + 1) * 1600]
        wavLength = f32(wavLength + f32(f32(len(x)) / samplerate))
        buf = np.concatenate([buf, x])[-3200:]
        did = bool(float(f32(wavLength - vad_point)) >= 0.1)
        if did:
            need = buf[::2]
            T = len(need) // 80
            out = graph_scores(need[:T * 80].reshape(1, T, 80), np.float32) if T else np.zeros(0, np.float32)
            last = out[-10:] if len(out) >= 10 else np.zeros(0, np.float32)
            scores.append(np.concatenate([last, np.full(10 - len(last), np.nan, np.float32)]))
            vad_result = int(np.sum(last > -0.1)) > 5
            vad_point = wavLength
        ran.append(did)
        ev = 0
        if not sound_start:
            if vad_result:
                sound_start = 1
                starts.append(float(f32(float(wavLength) - 0.2)))
                ev = 1
        else:
            sil_times = sil_times + 1 if not vad_result else 0
            if sil_times == 5:
                ends.append(float(f32(float(wavLength) - 0.2)))
                sound_start, sil_times, ev = 0, 0, 2
        events.append(ev)
    return dict(gate_events=np.array(events, np.int32), gate_ran=np.array(ran, np.bool_),
                gate_scores=np.array(scores, np.float32).reshape(-1, 10), gate_starts=np.array(starts, np.float32),
                gate_ends=np.array(ends, np.float32))


def synthetic(rng):
    """score sequences for every branch of parse / final_parse: no speech, speech from the start, late onset,
    onsets at the 20-frame window edge, sums of exactly 5, exact zeros, partial last blocks, tiny and empty inputs"""
    seqs = [np.zeros(0), -np.ones(7), np.ones(7), np.ones(10), np.ones(25), -np.ones(300), np.ones(300)]
    on = -np.ones(200); on[130:] = 1.0; seqs.append(on)
    five = -np.ones(120); five[15:20] = 0.0; seqs.append(five)              # exactly 5 of 10 at score 0.0
    four = -np.ones(120); four[15:19] = 1.0; seqs.append(four)
    for n in (37, 141, 999, 1203, 2500):
        p = rng.uniform(0.2, 0.8)
        seqs.append(np.where(rng.uniform(size=n) < p, rng.uniform(0, 2, n), -rng.uniform(0, 2, n)))
    for n in (400, 1605, 3001):
        s = -np.ones(n)
        for _ in range(4):
            a = int(rng.integers(0, n)); s[a:a + int(rng.integers(5, 200))] = 0.5
        seqs.append(s)
    seqs.append(np.where(np.arange(500) % 3 == 0, 0.0, -0.0))
    tail = -np.ones(23); tail[10:] = 1.0; seqs.append(tail)                  # onset with a partial last block
    return [np.asarray(s, np.float32) for s in seqs]


def recover_cases(rng):
    cases = [[[0.0, 1.0], [1.05, 2.0]], [[0.0, 1.0], [1.1, 2.0]], [[0.0, 1.0], [1.2, 2.0], [2.25, 3.0]],
             [[0.0, 16.0], [20.0, 21.0]], [[0.0, 30.0], [31.0, 32.0]], [[1.0, 47.3], [47.35, 48.0]],
             [[0.0, 14.0], [14.05, 16.0]], [[0.5, 3.0], [3.05, 9.0], [9.02, 20.0], [25.0, 61.7]]]
    for _ in range(6):
        t, segs = 0.0, []
        for _ in range(int(rng.integers(2, 7))):
            t = round(t + float(rng.choice([0.02, 0.05, 0.3, 2.0])), 3)
            e = round(t + float(rng.uniform(0.2, 33.0)), 3)
            segs.append([t, e]); t = e
        cases.append(segs)
    return cases


def main():
    rng = np.random.default_rng(20261015)
    OfflineVAD = load_offline_vad()
    shutil.copyfile(ONNX, os.path.join(OUT, "vad.onnx"))
    bac, cpp = vad_golden.speech()
    comp = vad_golden.composed_i16()
    out = {"in_test8k": np.round(read_wav(TEST8K) * 32768).astype(np.int16),
           "meta_composed_sha256": np.array(vad_golden.sha256(comp))}
    ins = {"test8k": out["in_test8k"], "bac": bac, "cpp": cpp, "composed": comp}
    for name, i16 in ins.items():
        x = i16.astype(np.float32) / 32768
        d = x if name == "test8k" else x[::2]
        T = len(d) // 80
        fr = d[:T * 80].reshape(1, T, 80)
        out["s32_" + name] = graph_scores(fr, np.float32).astype(np.float32)
        out["s64_" + name] = graph_scores(fr, np.float64).astype(np.float64)
        out["seg_" + name] = ref_segments(OfflineVAD, out["s32_" + name])
        print(name, T, "speech %.0f%%" % (100 * np.mean(out["s32_" + name] >= 0)), out["seg_" + name].tolist())
    for i, s in enumerate(synthetic(rng)):
        out["syn_scores_%d" % i] = s
        out["syn_seg_%d" % i] = ref_segments(OfflineVAD, s)
    for i, c in enumerate(recover_cases(rng)):
        out["rec_in_%d" % i] = np.array(c, np.float64)
        out["rec_out_%d" % i] = np.array(OfflineVAD(sr=16000).recover(c), np.float64).reshape(-1, 2)
    out.update(gate_events(comp.astype(np.float32) / 32768))
    print("gate events:", [(i, int(e)) for i, e in enumerate(out["gate_events"]) if e])
    out["meta_source"] = np.array("vad.onnx + OfflineVAD (offline_asr_session.py) + Session::Parase (asr_session.cpp)")
    out["meta_layout"] = np.array("scores [T]; segments [n,2] seconds rounded to 3 decimals; gate pushes of 1600 samples")
    np.savez_compressed(os.path.join(OUT, "vad_ref.npz"), **out)


if __name__ == "__main__":
    main()
