"""Generates the speech-enhancement fixtures.  Runs ONLY where the reference checkout exists (nothing at test time
reads it).

    python tests/golden/make_enhance_golden.py

Outputs (tests/golden/):
  online_vad_model/saved_model.pb   the reference's vad/online_vad_model/saved_model.pb, byte for byte (its variables
                                    are already stored next to it)
  vad_enhance_ref.npz
    es32_<name>, es64_<name>        scores [T] of the SavedModel's call function, float32 / float64
    ef_<name>                       int32 frame indices kept of the enhanced output (all frames for the short inputs)
    e32_<name>, e64_<name>          enhanced frames [len(ef), 80] (= input frame * voice mask), float32 / float64
        name: composed (tests/vad_golden.py, 16 kHz, decimated: wav[::2]), test8k (vad_ref.npz in_test8k, 8 kHz) and
        the odd lengths of ODD below (prefixes of committed recordings; decimated when 16 kHz)
    ov_scores                       [n, 10] float32: what the reference's vad/online_vad.py asked of `inference`, in
                                    order, when its __main__ ran unmodified over 20 ms packets of test.wav
    ov_windows_sha256               SHA-256 of those n [1, 10, 80] float32 windows, concatenated
    ov_lines                        what that run printed (its events), one entry per line
    meta_*                          SHA-256 of the composed recording and of saved_model.pb, layout notes
The call function (`__inference_online_cnn_vad_layer_call_and_return_conditional_losses_1326`) and `inference` are
executed node by node by tests/tf_graph_mini.py; the reference's online_vad.py is imported with a stub `tensorflow`
module whose `saved_model.load(...).inference` is that interpreter.  No source text is stored.
"""
import contextlib
import hashlib
import io
import os
import runpy
import shutil
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tf_graph_mini  # noqa: E402
import vad_golden  # noqa: E402

REF = "/root/reference"
ONLINE_PY = REF + "/vad/online_vad.py"
MODEL = REF + "/vad/online_vad_model"
OUT = os.path.join(ROOT, "tests", "golden")
SM = os.path.join(OUT, "online_vad_model")
# name -> (source, samples, sample rate); the source is a committed recording
ODD = {"odd_bac": ("bac", 12345, 16000), "odd_cpp_short": ("cpp", 1439, 16000), "odd_test8k": ("test8k", 4037, 8000),
       "odd_test8k_one": ("test8k", 159, 8000)}
STRIDE, HEAD, TAIL = 37, 64, 16


def kept_frames(T):
    if T <= HEAD + TAIL:
        return np.arange(T, dtype=np.int32)
    return np.unique(np.concatenate([np.arange(HEAD), np.arange(0, T, STRIDE), np.arange(T - TAIL, T)])).astype(np.int32)


def sha256_file(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def inputs(ref):
    """name -> (float32 samples, sample rate)"""
    bac, cpp = vad_golden.speech()
    src = {"bac": bac, "cpp": cpp, "test8k": ref["in_test8k"], "composed": vad_golden.composed_i16()}
    out = {"composed": (src["composed"], 16000), "test8k": (src["test8k"], 8000)}
    for name, (s, n, sr) in ODD.items():
        out[name] = (src[s][:n], sr)
    return {k: (v.astype(np.float32) / 32768, sr) for k, (v, sr) in out.items()}


def frames_of(x, sr):
    """[1, T, 80] frames the network reads, T = len(x) // (80 * decimate) as mi355asr_vad_frames counts them"""
    d = x[::2] if sr == 16000 else x
    T = len(x) // (80 * (sr // 8000))
    return d[:T * 80].reshape(1, T, 80)


def online_run(graph):
    """the reference's online_vad.py __main__, unmodified, with `tensorflow` stubbed by the interpreter"""
    calls, windows = [], []

    class _Out:
        def __init__(self, a):
            self.a = a

        def numpy(self):
            return self.a

    class _Loaded:
        def inference(self, x):
            assert x.dtype == np.float32 and x.shape == (1, 10, 80), (x.dtype, x.shape)
            windows.append(np.ascontiguousarray(x))
            s = graph.inference(x)[0]
            calls.append(np.asarray(s, np.float32).reshape(-1))
            return _Out(s)

    def load(path):
        assert sha256_file(os.path.join(path, "saved_model.pb")) == sha256_file(os.path.join(SM, "saved_model.pb"))
        return _Loaded()

    tf = types.ModuleType("tensorflow")
    tf.saved_model = types.SimpleNamespace(load=load)
    saved, cwd = sys.modules.get("tensorflow"), os.getcwd()
    sys.modules["tensorflow"] = tf
    buf = io.StringIO()
    try:
        os.chdir(REF)
        with contextlib.redirect_stdout(buf):
            runpy.run_path(ONLINE_PY, run_name="__main__")
    finally:
        os.chdir(cwd)
        if saved is None:
            del sys.modules["tensorflow"]
        else:
            sys.modules["tensorflow"] = saved
    h = hashlib.sha256()
    for w in windows:
        h.update(w.tobytes())
    return np.stack(calls), h.hexdigest(), buf.getvalue().splitlines()


def main():
    shutil.copyfile(os.path.join(MODEL, "saved_model.pb"), os.path.join(SM, "saved_model.pb"))
    with np.load(os.path.join(OUT, "vad_ref.npz")) as z:
        ref = {k: z[k] for k in z.files}
    g32 = tf_graph_mini.SavedModelGraph(SM, np.float32)
    g64 = tf_graph_mini.SavedModelGraph(SM, np.float64)
    out = {}
    for name, (x, sr) in inputs(ref).items():
        fr = frames_of(x, sr)
        T = fr.shape[1]
        keep = kept_frames(T)
        s32, e32 = g32.call(fr)
        s64, e64 = g64.call(fr)
        out["es32_" + name] = s32.reshape(-1).astype(np.float32)
        out["es64_" + name] = s64.reshape(-1).astype(np.float64)
        out["ef_" + name] = keep
        out["e32_" + name] = e32[0][keep].astype(np.float32)
        out["e64_" + name] = e64[0][keep].astype(np.float64)
        print(name, sr, "T=%d kept %d" % (T, len(keep)))
    out["ov_scores"], out["ov_windows_sha256"], lines = online_run(g32)
    out["ov_windows_sha256"] = np.array(out["ov_windows_sha256"])
    out["ov_lines"] = np.array(lines)
    print("online_vad.py:", len(out["ov_scores"]), "VAD calls;", lines)
    out["meta_composed_sha256"] = np.array(vad_golden.sha256(vad_golden.composed_i16()))
    out["meta_saved_model_sha256"] = np.array(sha256_file(os.path.join(SM, "saved_model.pb")))
    out["meta_layout"] = np.array("enhanced frames [kept, 80] = input frame (8 kHz; wav[::2] of 16 kHz) * voice mask; "
                                  "scores [T]; ov_* from 20 ms packets of test.wav (in_test8k)")
    np.savez_compressed(os.path.join(OUT, "vad_enhance_ref.npz"), **out)


if __name__ == "__main__":
    main()
