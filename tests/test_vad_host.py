"""VAD host side: the OfflineVAD segmentation and the C++ gate against the reference's own code (recorded in
tests/golden/vad_ref.npz by make_vad_golden.py), the ONNX weight mapping, and a float64 restatement of the network
against the graph's own float64 scores.  No GPU."""
import os

import numpy as np
import pytest

from oracle import onnx_mini
from tensorflowasr_amd.vad import OfflineVAD, VAD, VADGate, segments_from_scores, vad_gate, weights_from_onnx_inits
from vad_golden import inputs_i16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUTS = ("test8k", "bac", "cpp", "composed")


def load_ref():
    """vad_ref.npz plus its inputs (in_<name>, int16), the ones rebuilt from tests/golden/*.wav included"""
    with np.load(os.path.join(GOLDEN, "vad_ref.npz")) as z:
        ref = {k: z[k] for k in z.files}
    ref.update({"in_" + k: v for k, v in inputs_i16(ref).items()})
    return ref


@pytest.fixture(scope="module")
def ref():
    return load_ref()


def graph_inits():
    """the initialisers of tests/golden/vad.onnx as oracle/onnx_mini (a reader independent of the product's) sees them"""
    return onnx_mini.load(os.path.join(GOLDEN, "vad.onnx"))[1]


def graph_weights():
    return weights_from_onnx_inits(graph_inits())


def net64(frames, w):
    """The network as the issue states it, in float64: frames [T, 80] -> scores [T]."""
    w = {k: v.astype(np.float64) for k, v in w.items()}
    dense = lambda x, n, relu: (np.maximum if relu else (lambda a, b: a))(x @ w[n + "/kernel"] + w[n + "/bias"], 0)

    def conv(x, n):
        xp = np.concatenate([np.zeros((4, x.shape[1])), x])          # causal zero pad of the activations
        k = w[n + "/kernel"]                                         # [5, in, out]; tap 4 = current frame
        y = sum(xp[t:t + len(x)] @ k[t] for t in range(5))
        return np.maximum(y + w[n + "/bias"], 0)

    x = frames.astype(np.float64)
    x = dense(x, "dense", False)
    x = dense(x, "dense_1", True)
    x = conv(x, "conv1d")
    x = dense(x, "dense_2", True)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    x = (x - mu) / np.sqrt(var + np.float64(np.float32(1e-3))) * w["layer_normalization/gamma"] + w["layer_normalization/beta"]
    x = conv(x, "conv1d_1")
    x = dense(x, "dense_3", True)
    return (x @ w["dense_4/kernel"] + w["dense_4/bias"]).reshape(-1)


def frames_of(ref, name):
    x = ref["in_" + name].astype(np.float32) / 32768
    d = x if name == "test8k" else x[::2]
    T = len(d) // 80
    return d[:T * 80].reshape(T, 80)


def as_list(a):
    return [[float(s), float(e)] for s, e in np.asarray(a).reshape(-1, 2)]


@pytest.mark.parametrize("name", INPUTS)
def test_segments_of_recordings_equal_the_reference(ref, name):
    s = ref["s32_" + name]
    assert segments_from_scores(s, len(s) * 160, 16000) == as_list(ref["seg_" + name])


def test_segments_of_synthetic_scores_equal_the_reference(ref):
    n = sum(1 for k in ref if k.startswith("syn_scores_"))
    assert n >= 20
    counts = set()
    for i in range(n):
        s = ref["syn_scores_%d" % i]
        got = segments_from_scores(s, len(s) * 160, 16000)
        assert got == as_list(ref["syn_seg_%d" % i]), i
        counts.add(len(got))
    assert counts == {0, 1}          # the reference's offline state machine never closes a segment before the end


def test_recover_equals_the_reference(ref):
    n = sum(1 for k in ref if k.startswith("rec_in_"))
    assert n >= 10
    ov = OfflineVAD(sr=16000)
    for i in range(n):
        assert ov.recover(as_list(ref["rec_in_%d" % i])) == as_list(ref["rec_out_%d" % i]), i


def test_vad_gate_rule():
    assert vad_gate([0.0] * 6 + [-0.1] * 4)
    assert not vad_gate([0.0] * 5 + [-0.1] * 5)           # > -0.1 is strict; more than 5 needed
    assert not vad_gate([1.0] * 9)                        # fewer than 10 frames: the C++ loop does not run
    assert vad_gate([-5.0] * 30 + [1.0] * 6 + [-1.0] * 4)


def test_gate_replays_the_parase_events(ref):
    wav = ref["in_composed"].astype(np.float32) / 32768
    recorded = iter(ref["gate_scores"])
    g = VADGate(scorer=lambda need: next(recorded))
    events, starts, ends = [], [], []
    for p in range(len(wav) // 1600):
        ev = g.push(wav[p * 1600:(p + 1) * 1600])
        events.append(ev)
        if ev == 1:
            starts.append(g.voice_start_times)
        elif ev == 2:
            ends.append(g.voice_end_times)
    assert next(recorded, None) is None                   # the VAD ran exactly as often as in the C++ cadence
    assert events == ref["gate_events"].tolist()
    assert np.array_equal(np.array(starts, np.float32), ref["gate_starts"])
    assert np.array_equal(np.array(ends, np.float32), ref["gate_ends"])
    assert len(starts) >= 5


def test_load_onnx_matches_the_graph_initialisers(ref):
    v = VAD(device="cpu").load_onnx(os.path.join(GOLDEN, "vad.onnx"))
    w = graph_weights()
    assert sorted(v.weights) == sorted(w)
    for k in w:
        assert v.weights[k].dtype == np.float32 and np.array_equal(v.weights[k], w[k]), k
    assert v.weights["conv1d/kernel"].shape == (5, 80, 80) and v.weights["dense_4/kernel"].shape == (80, 1)
    g = graph_inits()["StatefulPartitionedCall/conv1d/conv1d/ExpandDims_1:0"]     # [out, in, 1, 5]
    assert v.weights["conv1d/kernel"][4, 7, 3] == g[3, 7, 0, 4]


@pytest.mark.parametrize("name", INPUTS)
def test_float64_restatement_matches_the_graph(ref, name):
    got = net64(frames_of(ref, name), graph_weights())
    err = float(np.abs(got - ref["s64_" + name]).max())
    assert err < 1e-9, err
