"""CPU tests of the punctuation restorer: the ONNX name map and every transpose (a float64 NumPy restatement on the ABI-named
weights against the graph evaluator's fixture), the positional table, the reference's text rule on stubbed probabilities,
the C ABI's argument checks, the fixture's own sanity, and the sessions' `punc=` hooks.  No kernel is launched here."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import vad_golden
from punc_numpy import punc_probs
from punc_onnx_eval import GOLDEN, Graph, onnx_path

sys.path.insert(0, GOLDEN)
from make_stream_session_golden import StubRecogniser, StubScorer, packets, stub_punc   # noqa: E402

from tensorflowasr_amd import _lib, punc as P   # noqa: E402
from tensorflowasr_amd.checkpoint import read_onnx   # noqa: E402
from tensorflowasr_amd.session import ASRSession   # noqa: E402
from tensorflowasr_amd.stream_session import StreamingASRServer, _Stream   # noqa: E402

MODEL_CONFIG = dict(name="PuncTransformer", num_layers=3, d_model=64, enc_embedding_dim=64, num_heads=8, dff=64, pe_input=1024, rate=0.1)


def config():
    return {"model_config": dict(MODEL_CONFIG),
            "punc_vocab": {"model_type": "LM", "vocabulary": os.path.join(GOLDEN, "punc_tokens_ch.txt"), "blank_at_zero": True, "beam_width": 1},
            "punc_biaodian": {"model_type": "LM", "vocabulary": os.path.join(GOLDEN, "punc_tokens_bd.txt"), "blank_at_zero": True, "beam_width": 1}}


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(GOLDEN, "punc_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def model():
    return P.Punc(config(), device="cpu").load_onnx(onnx_path())


def test_numpy_restatement_on_abi_weights_equals_the_graph(ref, model):
    """pins ONNX_NAMES and every transpose: 1e-12 in float64 on every fixture case"""
    assert set(model.weights) == set(model.weight_names()) and len(model.weights) == 96
    for name in ref["cases"]:
        got = punc_probs(model.weights, ref["ids_" + name])
        err = np.abs(got - ref["p64_" + name]).max()
        assert got.shape == ref["p64_" + name].shape and err <= 1e-12, (name, err)


def test_fixture_covers_the_listed_cases(ref):
    lds = int(ref["lds_tokens"])
    want = {3, 4, 7, 8, 9, 16, 17, 33, 64, 65, lds - 1, lds, lds + 1, 1024}
    assert {len(ref["ids_" + n]) for n in ref["cases"] if n.startswith("rand_")} == want
    texts = [n for n in ref["cases"] if n.startswith("text_")]
    assert len(texts) >= 6
    marked = 0
    for n in texts:
        txt = str(ref["txt_" + n])
        assert 5 <= len(txt) <= 60 and len(ref["ids_" + n]) == len(txt) + 2
        marked += len(ref["out_" + n]) > len(txt)
    assert marked >= 3
    for n in ref["cases"]:
        ids = ref["ids_" + n]
        assert ids[0] == 1 and ids[-1] == 2 and ids[1:-1].min() >= 3 and ids.max() < 5039
        assert ref["p64_" + n].dtype == np.float64 and ref["p32_" + n].dtype == np.float32


def test_fixture_float32_and_float64_decide_alike(ref):
    """the reference's own float32 arithmetic excuses no token: every class and every >= 0.65 decision of p32 is p64's"""
    for n in ref["cases"]:
        p32, p64 = ref["p32_" + n], ref["p64_" + n]
        assert np.array_equal(p32.argmax(-1), p64.argmax(-1)), n
        assert np.array_equal(p32.max(-1) >= 0.65, p64.max(-1) >= 0.65), n
        # ... and the reference alone leaves at most 2 % of a case within 1e-3 of a tie or of the threshold
        top = np.sort(p64, -1)
        near = (top[:, -1] - top[:, -2] < 1e-3) | (np.abs(top[:, -1] - 0.65) < 1e-3)
        assert near.sum() <= 0.02 * len(near), n


def test_fixture_rule_outputs(ref, model):
    """out_<k> is the reference rule on the fixture's own probabilities"""
    for n in (c for c in ref["cases"] if c.startswith("text_")):
        p = ref["p64_" + n][1:-1]
        got = P.apply_rule(str(ref["txt_" + n]), p.argmax(-1), p.max(-1), model.bd_featurizer.vocab_array)
        assert got == ref["out_" + n].tolist(), n


def test_name_map_covers_every_weight_of_the_graph():
    g = Graph()
    _, inits = read_onnx(onnx_path())
    weights = g.weight_initialisers()
    assert len(weights) == 95 and weights == P.graph_weight_names(inits)
    assert set(P.ONNX_NAMES.values()) == set(weights)
    assert len(set(P.ONNX_NAMES.values())) == len(P.ONNX_NAMES) == 95
    extra = dict(inits)
    extra["encoder/unmapped/ReadVariableOp:0"] = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError, match="without an ABI name"):
        P.weights_from_onnx_inits(extra)
    fewer = {k: v for k, v in inits.items() if k != P.ONNX_NAMES["final/bias"]}
    with pytest.raises(ValueError, match="lacks"):
        P.weights_from_onnx_inits(fewer)


def test_load_weights_refuses_an_unset_or_unknown_tensor(model):
    w = dict(model.weights)
    del w["to_bert/bias"]
    with pytest.raises(ValueError, match="to_bert/bias"):
        P.Punc(config(), device="cpu").load_weights(w)
    w = dict(model.weights, bogus=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="bogus"):
        P.Punc(config(), device="cpu").load_weights(w)


def test_pos_encoding_is_the_reference_formula_bit_for_bit(model):
    pe_input, d_model = 1024, 64
    pos, i = np.arange(pe_input)[:, np.newaxis], np.arange(d_model)[np.newaxis, :]
    angle_rads = pos * (1 / np.power(10000, (2 * (i // 2)) / np.float32(d_model)))
    angle_rads[:, 0::2] = np.sin(angle_rads[:, 0::2])
    angle_rads[:, 1::2] = np.cos(angle_rads[:, 1::2])
    want = np.array(angle_rads[np.newaxis, ...], "float32")
    got = P.pos_encoding(pe_input, d_model)
    assert got.dtype == np.float32 and got.tobytes() == want[0].tobytes()
    assert model.pos_encode_inputs.shape == (1, 1024, 64) and model.pos_encode_inputs.tobytes() == want.tobytes()
    assert model.weights["pos_encoding"].tobytes() == want[0].tobytes()


# ---- the text rule on stubbed probabilities ------------------------------------------------------------------------------
class StubbedPunc(P.Punc):
    """`forward` replaced by a table: row t of a sentence gets class `plan[t][0]` with probability `plan[t][1]`"""

    def __init__(self, plan, **kw):
        super().__init__(config(), device="cpu", **kw)
        self.plan, self.launches = plan, 0

    def forward(self, ids, lengths=None, want_decisions=True):
        self.launches += 1
        ids = np.asarray(ids)
        B, T = ids.shape
        C = self.cfg["classes"]
        probs = np.zeros((B, T, C), np.float32)
        for b in range(B):
            for t in range(int(lengths[b])):
                c, p = self.plan.get(t, (0, 1.0))
                probs[b, t] = (1 - p) / (C - 1)
                probs[b, t, c] = p
        return torch.from_numpy(probs), torch.from_numpy(probs.argmax(-1).astype(np.int32)), torch.from_numpy(probs.max(-1))


def test_rule_threshold_argmax_and_vocab_array_offset():
    txt = "今天天气怎么样"
    # row t + 1 belongs to character t (row 0 is <S>)
    p = StubbedPunc({1: (3, 0.6501), 2: (3, 0.6499), 3: (1, 0.99), 4: (0, 0.99), 5: (2, 0.9), 6: (30, 0.7), 0: (5, 0.99), 8: (5, 0.99)})
    bd = p.bd_featurizer
    assert bd.vocab_array[3] == "“" and bd.index_to_token[3] == "，" and bd.vocab_array[2] == "，"
    got = p.punc_recover(txt)
    #     0.6501 marks, 0.6499 does not; classes 0 and 1 never mark; class c yields vocab_array[c], the token of class c + 1;
    #     the rows of <S> (0) and </S> (8) are dropped
    assert got == ["今", "“", "天", "天", "气", "怎", "，", "么", bd.vocab_array[30], "样"]
    assert p(txt) == got and p.launches == 2
    assert p.punc_recover_batch([txt, txt[:3]]) == [got, ["今", "“", "天", "天"]] and p.launches == 3
    # the last class has no vocab_array entry: the reference's IndexError
    with pytest.raises(IndexError):
        StubbedPunc({1: (31, 0.9)}).punc_recover(txt)
    assert p.punc_recover("") == []


def test_unknown_characters_raise_or_skip():
    txt = "今天Ω天气"
    p = StubbedPunc({1: (3, 0.9)})
    with pytest.raises(KeyError):
        p.punc_recover(txt)
    assert p.launches == 0
    q = StubbedPunc({1: (3, 0.9)}, on_unknown="skip")
    assert q.punc_recover(txt) == list(txt) and q.launches == 0
    assert q.punc_recover_batch([txt, "今天"]) == [list(txt), ["今", "“", "天"]] and q.launches == 1
    with pytest.raises(ValueError):
        P.Punc(config(), device="cpu", on_unknown="drop")


def test_encode_wraps_the_text_in_markers(model):
    assert model.encode("今天") == [1] + model.vocab_featurizer.extract("今天") + [2]
    assert model.cfg == dict(d_model=64, enc_embedding_dim=64, num_heads=8, dff=64, num_layers=3, vocab=5039, classes=32, pe_input=1024)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
SHIPPED = dict(d_model=64, enc_embedding_dim=64, num_heads=8, dff=64, num_layers=3, vocab=5039, classes=32, pe_input=1024)


def _create(**over):
    lib = _lib.lib()
    p = ctypes.c_void_p()
    rc = lib.mi355asr_punc_create(ctypes.byref(_lib.PuncConfig(**dict(SHIPPED, **over))), ctypes.byref(p))
    return lib, rc, p


def test_create_accepts_the_shipped_config_and_names_its_weights():
    lib, rc, p = _create()
    assert rc == 0 and p.value
    names = [lib.mi355asr_weight_name(p, i).decode() for i in range(lib.mi355asr_num_weights(p))]
    assert names == P.Punc(config(), device="cpu").weight_names()
    lt, mt = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mi355asr_punc_limits(p, ctypes.byref(lt), ctypes.byref(mt)) == 0
    assert 16 <= lt.value < mt.value == 1024 and lt.value % 16 == 0
    # four activation buffers of 68-float rows and the mask term fit the 160 KiB of LDS at lds_tokens, not one tile later
    assert lt.value * (4 * 68 + 1) * 4 <= 160 * 1024 < (lt.value + 16) * (4 * 68 + 1) * 4
    for n in (1, 6):
        lib2, rc2, p2 = _create(num_layers=n)
        assert rc2 == 0 and lib2.mi355asr_num_weights(p2) == 4 + (n + max(n - 1, 1)) * 16 + 2 * n + 4 + 2
        lib2.mi355asr_destroy(p2)
    lib.mi355asr_destroy(p)


@pytest.mark.parametrize("bad", [dict(d_model=128), dict(dff=256), dict(num_heads=4), dict(num_layers=0), dict(num_layers=7),
                                 dict(classes=65), dict(pe_input=1025), dict(enc_embedding_dim=32), dict(vocab=0)])
def test_create_refuses_unsupported_configs_with_a_message(bad):
    lib, rc, p = _create(**bad)
    assert rc == -1 and not p.value
    msg = lib.mi355asr_last_error().decode()
    assert msg.startswith("Punc:") and len(msg) > 20


def test_workspace_limits_and_state_errors():
    lib, rc, p = _create()
    lt, mt = ctypes.c_int32(), ctypes.c_int32()
    lib.mi355asr_punc_limits(p, ctypes.byref(lt), ctypes.byref(mt))

    def ws(B, T):
        n = ctypes.c_size_t(12345)
        assert lib.mi355asr_punc_workspace_bytes(p, B, T, ctypes.byref(n)) == 0
        return n.value

    Ts = [1, 16, lt.value, lt.value + 1, lt.value + 17, 512, 1024]
    for B in (1, 2, 300):
        sizes = [ws(B, T) for T in Ts]
        assert sizes == sorted(sizes) and sizes[2] == 0 < sizes[3]
        assert all(ws(B, T) <= ws(B + 1, T) for T in Ts)
        # a sentence's region holds its four activation buffers and the mask term
        assert ws(B, 1024) >= B * 1024 * (4 * 68 + 1) * 4 and ws(B, 1024) % 256 == 0
    n = ctypes.c_size_t()
    assert lib.mi355asr_punc_workspace_bytes(p, 1, 1025, ctypes.byref(n)) == -1
    assert lib.mi355asr_punc_workspace_bytes(p, 0, 8, ctypes.byref(n)) == -1
    # forward before finalize: the state error, whatever else is wrong with the call
    assert lib.mi355asr_punc_forward(p, None, None, 1, 8, None, None, None, None, 0, None) == -2
    assert b"finalis" in lib.mi355asr_last_error()
    # the other families' entry points refuse the handle, and this one refuses theirs
    v = ctypes.c_void_p()
    assert lib.mi355asr_vad_create(ctypes.byref(_lib.VadConfig(dmodel=80, frame=80, decimate=2)), ctypes.byref(v)) == 0
    assert lib.mi355asr_punc_forward(v, None, None, 1, 8, None, None, None, None, 0, None) == -1
    assert lib.mi355asr_punc_limits(v, ctypes.byref(lt), ctypes.byref(mt)) == -1
    assert lib.mi355asr_vad_forward(p, None, 1, 160, None, None, None) == -1
    lib.mi355asr_destroy(v)
    lib.mi355asr_destroy(p)


def test_weight_shapes_are_checked():
    lib, rc, p = _create()
    a = np.zeros((64, 3, 64), np.float32)
    dims = (ctypes.c_int64 * 3)(*a.shape)
    assert lib.mi355asr_load_weight(p, b"encoder/conv_0/kernel", a.ctypes.data_as(ctypes.c_void_p), 3, dims) == -3
    dims = (ctypes.c_int64 * 3)(3, 64, 64)
    assert lib.mi355asr_load_weight(p, b"encoder/conv_0/kernel", a.ctypes.data_as(ctypes.c_void_p), 3, dims) == 0
    assert lib.mi355asr_load_weight(p, b"encoder/conv_3/kernel", a.ctypes.data_as(ctypes.c_void_p), 3, dims) == -3
    assert lib.mi355asr_finalize_weights(p, None) == -3 and b"missing weight" in lib.mi355asr_last_error()
    lib.mi355asr_destroy(p)


# ---- sessions ----------------------------------------------------------------------------------------------------------------
class _OneSegmentVad:
    def scores(self, wav):
        return torch.ones((1, len(wav) // 160))


class _TextAsr:
    def __init__(self, text):
        self.text = text

    def offline_stt_wave(self, data):
        return "ph", self.text


def test_asr_session_applies_the_hook_above_five_characters():
    wav = np.zeros(16000 * 2, np.float32)
    calls = []

    def hook(text):
        calls.append(text)
        return list(text) + ["。"]

    for text, want in (("12345", "12345"), ("123456", "123456。"), ("", "")):
        plain = ASRSession(_TextAsr(text), _OneSegmentVad()).send(wav)
        got = ASRSession(_TextAsr(text), _OneSegmentVad(), punc=hook).send(wav)
        assert len(plain) == 1 and plain[0]["best_text"] == text                  # the default: today's output
        assert [{k: v for k, v in r.items() if k != "best_text"} for r in got] == [{k: v for k, v in r.items() if k != "best_text"} for r in plain]
        assert got[0]["best_text"] == want
    assert calls == ["123456"]


def test_stream_rule_is_five_or_more():
    hook = lambda text: list(text) + ["。"]
    st = _Stream("s", 16000, hook)
    assert st._text("1234") == "1234" and st._text("12345") == "12345。"
    assert _Stream("s", 16000, None)._text("123456") == "123456"
    assert st._text("12345", punctuated=["x"]) == "x"


class _BatchHook:
    def __init__(self):
        self.batches, self.singles = [], 0

    def __call__(self, text):
        self.singles += 1
        return stub_punc(text)

    def punc_recover_batch(self, texts):
        self.batches.append(list(texts))
        return [stub_punc(t) for t in texts]


def _serve(punc, feeds):
    srv = StreamingASRServer(StubRecogniser(), StubScorer(), len(feeds), punc=punc, session="asr")
    events, ticks_with_text = [], 0
    for k in range(max(len(f) for f in feeds)):
        ev = srv.send([f[k] if k < len(f) else None for f in feeds])
        ticks_with_text += any(e is not None and len(e.get("best_text", "")) >= 5 for e in ev)
        events.append(ev)
    ev = srv.final_send()
    ticks_with_text += any(e is not None and len(e.get("best_text", "")) >= 5 for e in ev)
    events.append(ev)
    return events, ticks_with_text


def test_server_calls_a_batch_hook_once_per_tick():
    x = vad_golden.composed_i16()
    feeds = [packets(x[o:o + 16000 * 12], 320) for o in (0, 0, 16000 * 7)]      # two streams in step: their texts fall due together
    want, _ = _serve(stub_punc, feeds)
    hook = _BatchHook()
    got, ticks = _serve(hook, feeds)
    assert got == want                                         # the per-text hook's events
    assert sum(e is not None and "best_text" in e for ev in want for e in ev) > 6
    assert hook.singles == 0 and len(hook.batches) == ticks    # one call per tick that has a text due
    assert max(len(b) for b in hook.batches) >= 2 and all(len(t) >= 5 for b in hook.batches for t in b)
    plain, _ = _serve(None, feeds)                             # no hook: the unpunctuated events
    strip = lambda evs: [[None if e is None else {k: (v[:-1] if k == "best_text" and len(v) >= 6 else v) for k, v in e.items()} for e in ev] for ev in evs]
    assert plain == strip(want)
