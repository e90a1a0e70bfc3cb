"""Speech enhancement (the online VAD's voice-mask head) and the reference's streaming OnlineVAD, host side: the
SavedModel interpreter against vad_ref.npz, the SavedModel weight mapping, a float64 restatement of the enhance path
against tests/golden/vad_enhance_ref.npz (make_enhance_golden.py), OnlineVAD against the reference run's events, the
streaming / batching logic over a NumPy stand-in for the device, and the C ABI surface.  No GPU."""
import os
import re

import numpy as np
import pytest

from tensorflowasr_amd import _lib
from tensorflowasr_amd.vad import MASK_NAMES, ONNX_NAMES, OnlineVAD, OnlineVADBatch, VAD
from test_vad_host import GOLDEN, frames_of, graph_weights, load_ref
import tf_graph_mini
import vad_golden

SAVED_MODEL = os.path.join(GOLDEN, "online_vad_model")
ODD = {"odd_bac": ("bac", 12345, 16000), "odd_cpp_short": ("cpp", 1439, 16000), "odd_test8k": ("test8k", 4037, 8000),
       "odd_test8k_one": ("test8k", 159, 8000)}


def load_enh():
    with np.load(os.path.join(GOLDEN, "vad_enhance_ref.npz")) as z:
        return {k: z[k] for k in z.files}


def enhance_inputs(ref, enh):
    """fixture name -> (float32 samples, sample rate), rebuilt from committed files (see make_enhance_golden.py)"""
    i16 = vad_golden.inputs_i16(ref)
    assert str(enh["meta_composed_sha256"]) == vad_golden.sha256(i16["composed"])
    out = {"composed": (i16["composed"], 16000), "test8k": (i16["test8k"], 8000)}
    for name, (src, n, sr) in ODD.items():
        out[name] = (i16[src][:n], sr)
    return {k: (v.astype(np.float32) / 32768, sr) for k, (v, sr) in out.items()}


def saved_model_weights():
    return VAD(device="cpu").load_saved_model(SAVED_MODEL).weights


def enhance64(frames, w):
    """The online model in float64 as include/mi355asr.h states it: frames [T, 80] -> (scores [T], enhanced [T, 80])."""
    w = {k: v.astype(np.float64) for k, v in w.items()}
    x0 = frames.astype(np.float64)

    def dense(x, n, relu):
        y = x @ w[n + "/kernel"] + w[n + "/bias"]
        return np.maximum(y, 0) if relu else y

    def conv(x, n):
        xp = np.concatenate([np.zeros((4, x.shape[1])), x])
        return np.maximum(sum(xp[t:t + len(x)] @ w[n + "/kernel"][t] for t in range(5)) + w[n + "/bias"], 0)

    x = dense(dense(x0, "dense", False), "dense_1", True)
    x = dense(conv(x, "conv1d"), "dense_2", True)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    x = (x - mu) / np.sqrt(var + np.float64(np.float32(1e-3))) * w["layer_normalization/gamma"] + w["layer_normalization/beta"]
    x = dense(conv(x, "conv1d_1"), "dense_3", True)
    scores = (x @ w["dense_4/kernel"] + w["dense_4/bias"]).reshape(-1)
    return scores, x0 * dense(x, "audio_voice_mask", False)


def input_frames(x, sr):
    """frames [T, 80] the network reads, T = len(x) // (80 * decimate) as mi355asr_vad_frames counts them"""
    d = x[::2] if sr == 16000 else x
    T = len(x) // (80 * (sr // 8000))
    return d[:T * 80].reshape(T, 80)


@pytest.fixture(scope="module")
def ref():
    return load_ref()


@pytest.fixture(scope="module")
def enh():
    return load_enh()


@pytest.fixture(scope="module")
def graph64():
    return tf_graph_mini.SavedModelGraph(SAVED_MODEL, np.float64)


def test_saved_model_fixture_is_pinned(enh):
    import hashlib
    with open(os.path.join(SAVED_MODEL, "saved_model.pb"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == str(enh["meta_saved_model_sha256"])


@pytest.mark.parametrize("name", ["test8k", "bac", "cpp", "composed"])
def test_interpreter_reproduces_the_onnx_graph_scores(ref, graph64, name):
    """the SavedModel walk and its variable binding, checked against vad.onnx's own scores before trusting the mask"""
    fr = frames_of(ref, name)[None]
    g32 = tf_graph_mini.SavedModelGraph(SAVED_MODEL, np.float32)
    for got in (g32.inference(fr)[0], g32.call(fr)[0]):
        want = ref["s32_" + name].astype(np.float64)
        err = np.abs(got.reshape(-1) - want).max() / np.abs(want).max()
        assert err <= 1e-5, (name, err)
    for got in (graph64.inference(fr)[0], graph64.call(fr)[0]):
        want = ref["s64_" + name]
        err = np.abs(got.reshape(-1) - want).max() / np.abs(want).max()
        assert err <= 1e-12, (name, err)


def test_interpreter_binds_every_variable_of_the_call(graph64):
    fd = [f for n, f in graph64.functions.items() if n.endswith("_call_and_return_conditional_losses_1326")][0]
    assert len(fd.args) == 19 and len(fd.outs) == 2
    assert sorted(graph64.names.values()) == sorted("online_cnn_vad/" + n for n in list(ONNX_NAMES) + list(MASK_NAMES))


def test_load_saved_model_maps_names_and_shapes():
    w = saved_model_weights()
    assert set(w) == set(ONNX_NAMES) | set(MASK_NAMES)
    assert w["audio_voice_mask/kernel"].shape == (80, 80) and w["audio_voice_mask/bias"].shape == (80,)
    assert w["conv1d/kernel"].shape == (5, 80, 80) and w["dense_4/kernel"].shape == (80, 1)
    onnx = graph_weights()
    for k in ONNX_NAMES:
        assert w[k].dtype == np.float32 and np.array_equal(w[k], onnx[k]), k
    v = VAD(device="cpu").load_saved_model(SAVED_MODEL)
    assert v.has_mask and not VAD(device="cpu", weights=onnx).has_mask


def test_enhance_without_the_mask_head_is_an_error():
    v = VAD(device="cpu", weights=graph_weights())
    with pytest.raises(_lib.Mi355AsrError, match="voice-mask"):
        v.enhance(np.zeros(1600, np.float32))


@pytest.mark.parametrize("name", ["composed", "test8k"] + sorted(ODD))
def test_float64_restatement_matches_the_graph(ref, enh, name):
    x, sr = enhance_inputs(ref, enh)[name]
    s, e = enhance64(input_frames(x, sr), saved_model_weights())
    keep = enh["ef_" + name]
    scale = max(1.0, float(np.abs(enh["e64_" + name]).max()))
    assert e.shape[0] == len(enh["es64_" + name])
    assert np.abs(e[keep] - enh["e64_" + name]).max() <= 1e-12 * scale, name
    assert np.abs(s - enh["es64_" + name]).max() <= 1e-12 * max(1.0, float(np.abs(s).max())), name
    # the float32 run agrees with the float64 one to float32 accuracy (what the GPU test holds the kernel to)
    assert np.abs(enh["e32_" + name] - enh["e64_" + name]).max() <= 1e-5 * max(1.0, scale)


def _packets(ref):
    x = ref["in_test8k"]
    return [x[i:i + 160].tobytes() for i in range(0, len(x), 160)]


def _run_online(v, packets):
    lines = []
    for p in packets:
        r = v.parse(p)
        if r == 1:
            lines += ["sound end %r" % v.live_result["end_time"], "=" * 22]
        elif r == 0:
            lines.append("sound start %r" % v.live_result["start_time"])
    if v.final_parse() == 1:
        lines += ["sound end %r" % v.live_result["end_time"], "=" * 22]
    return lines


def test_online_vad_reproduces_the_reference_run(ref, enh):
    import hashlib
    scores = list(enh["ov_scores"])
    h = hashlib.sha256()

    def scorer(window):
        assert window.dtype == np.float32 and window.shape == (800,)
        h.update(window.tobytes())
        return scores.pop(0)

    v = OnlineVAD(scorer=scorer)
    lines = _run_online(v, _packets(ref))
    assert not scores, "%d scores left" % len(scores)
    assert h.hexdigest() == str(enh["ov_windows_sha256"])              # the same windows, in the same order
    assert lines == [str(s) for s in enh["ov_lines"]]
    assert v.start_event == 1 and v.end_event == 1


class _NumpyVAD:
    """stand-in for the device VAD: the float64 restatement per row (host checks of the streaming / batching logic)"""
    has_mask = True

    def __init__(self):
        self.w = saved_model_weights()
        self.launches = 0

    def enhance(self, x, lengths=None, sample_rate=16000):
        import torch
        self.launches += 1
        dec = sample_rate // 8000
        B, L = x.shape
        T = L // (80 * dec)
        e, s = np.zeros((B, T * 80)), np.zeros((B, T))
        for b in range(B):
            n = L if lengths is None else min(lengths[b], L)
            tb = n // (80 * dec)
            if tb:
                sb, eb = enhance64(input_frames(x[b, :tb * 80 * dec], sample_rate), self.w)
                s[b, :tb], e[b, :tb * 80] = sb, eb.reshape(-1)
        return torch.from_numpy(e), torch.from_numpy(s)

    def inference(self, frames):
        return np.stack([enhance64(f, self.w)[0] for f in frames])[..., None]


@pytest.mark.parametrize("sr", [16000, 8000])
def test_streaming_logic_equals_offline(ref, sr):
    from tensorflowasr_amd.enhance import StreamingEnhancer
    rng = np.random.default_rng(sr)
    x = ref["in_bac"][:sr * 2].astype(np.float32) / 32768
    xs = [x, x[: len(x) // 3], (rng.standard_normal(sr) * 0.1).astype(np.float32)]
    v = _NumpyVAD()
    se = StreamingEnhancer(v, len(xs), sample_rate=sr)
    got = [([], []) for _ in xs]
    pos = [0] * len(xs)
    while any(p < len(s) for p, s in zip(pos, xs)):
        chunks = []
        for i, s in enumerate(xs):
            n = int(rng.choice([0, 1, 7, 79, 160, 333, 1500, 4000]))
            chunks.append(s[pos[i]:pos[i] + n])
            pos[i] += n
        for i, (e, sc) in enumerate(se.push(chunks)):
            got[i][0].append(e)
            got[i][1].append(sc)
    for i, s in enumerate(xs):
        e_off, s_off = v.enhance(s[None], sample_rate=sr)
        e = np.concatenate(got[i][0])
        assert len(e) == e_off.shape[1]
        assert np.abs(e - e_off.numpy()[0]).max() <= 1e-12
        assert np.abs(np.concatenate(got[i][1]) - s_off.numpy()[0]).max() <= 1e-12


def test_batched_online_vad_equals_single_streams(ref):
    v = _NumpyVAD()
    pk = _packets(ref)[:300]
    single = _run_online(OnlineVAD(v), pk)
    batch = OnlineVADBatch(v, 3)
    offs = [0, 0, 7]                                                    # the third stream starts 7 packets late
    lines = [[] for _ in range(3)]
    for t in range(len(pk) + max(offs)):
        packets = [pk[t - o] if 0 <= t - o < len(pk) else None for o in offs]
        for i, r in enumerate(batch.parse(packets)):
            if r == 1:
                lines[i] += ["sound end %r" % batch[i].live_result["end_time"], "=" * 22]
            elif r == 0:
                lines[i].append("sound start %r" % batch[i].live_result["start_time"])
    for i, r in enumerate(batch.final_parse()):
        if r == 1:
            lines[i] += ["sound end %r" % batch[i].live_result["end_time"], "=" * 22]
    assert single and all(l == single for l in lines)


def test_enhance_exports_in_header_and_signatures():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mi355asr.h")).read()
    for name in ("mi355asr_vad_enhancer_create", "mi355asr_vad_enhance"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mi355asr_vad_enhance"][1]) == 8
