"""The float64 restatement tests/punc_loss_ref.py of the punctuation trainer's losses, pinned on the host: against the reference's
own PuncTrainer.classes_loss / bert_feature_loss / classes_acc run on the stand-in (tests/golden/punc_loss_ref.npz; float64 to
1e-12 relative, float32 to 2e-6, the line check_recipes.py uses for float32 fixtures), its closed-form gradients against central
differences in float64; the library exports the new entry points and refuses bad arguments before anything is launched."""
import ctypes
import os

import numpy as np
import pytest

import punc_loss_ref as R
from test_punc_host import config

from tensorflowasr_amd import _lib, losses
from tensorflowasr_amd.punc import Punc, lengths_from_ids

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "punc_loss_ref.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_inputs(golden, k):
    B, T, C, T1, T2, seed = (int(v) for v in golden["cases"][k])
    lengths = golden["lengths_%d" % k].tolist()
    lengths = None if lengths == [T] * B else lengths
    logits = R.seeded_logits((B, T, C), seed)
    labels = R.seeded_labels((B, T), C, seed, lengths)
    real, pred = R.seeded_features((B, T1, 768), (B, T2, 768), seed, lengths)
    return labels, logits, real, pred


def close(got, want, rel):
    return np.all(np.abs(np.asarray(got) - want) <= rel * np.abs(want))


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_reproduces_the_reference_run(golden, k):
    labels, logits, real, pred = case_inputs(golden, k)
    for name, a in (("logits", logits), ("labels", labels), ("real", real), ("pred", pred)):
        assert np.sum(a, dtype=np.float64) == golden["sum_%s_%d" % (name, k)], name
    assert (labels == 0).any() and (labels == 1).any() and (labels > 1).any() and (real == -10).any()
    got = {"bd": R.classes_loss(labels, logits), "acc": R.classes_acc(labels, logits)[1], "fm": R.feature_loss(real, pred)}
    for key, value in got.items():
        assert close(value, golden["%s64_%d" % (key, k)], 1e-12), key
        assert close(value, golden["%s32_%d" % (key, k)], 2e-6), key
    assert golden["min_gap"] >= 1e-3


def test_classes_gradient_equals_central_differences():
    B, Q, T, C = 3, 7, 9, 5
    logits = R.seeded_logits((B, T, C), 21).astype(np.float64)
    labels = R.seeded_labels((B, Q), C, 21, [7, 4, 6])
    labels[2, :6] = 1                                         # a row of "no mark" alone: the second term is 0
    labels[0, 1] = C + 3                                      # out of range: a NaN loss for the row, a zero gradient row
    up = np.array([0.7, -1.3, 2.0])
    g = R.classes_grad(labels, logits, up)
    assert np.isnan(R.classes_loss(labels, logits)[0]) and not g[0, 1].any() and not g[:, Q:].any()
    assert not g[:, :Q][labels == 0].any()
    fixed = labels.copy()
    fixed[0, 1] = 2                                           # in range again: finite everywhere
    assert np.array_equal(R.classes_grad(fixed, logits, up)[1:], g[1:])
    h = 1e-6
    num = np.zeros_like(g)
    for idx in np.ndindex(*logits.shape):
        hi, lo = logits.copy(), logits.copy()
        hi[idx] += h
        lo[idx] -= h
        num[idx] = (up * (R.classes_loss(fixed, hi) - R.classes_loss(fixed, lo))).sum() / (2 * h)
    want = R.classes_grad(fixed, logits, up)
    assert np.abs(want).max() > 0.1 and np.abs(want - num).max() <= 1e-8 * np.abs(want).max()
    xe = np.log(np.exp(logits[2, :6]).sum(-1)) - logits[2, :6, 1]
    assert R.classes_loss(labels, logits)[2] == pytest.approx(xe.sum() / (6 + 1e-6), rel=1e-12)


def test_feature_gradient_equals_central_differences():
    real, pred = R.seeded_features((2, 5, 6), (2, 7, 6), 22, [5, 3], scatter=0.2)
    real[1, 0] = -10                                          # a whole token masked inside the sentence
    pred = pred.astype(np.float64)
    up = np.array([1.5, -0.4])
    g = R.feature_grad(real, pred, up)
    assert not g[:, 5:].any() and not g[:, :5][real == -10].any()
    h = 1e-6
    num = np.zeros_like(g)
    for idx in np.ndindex(*pred.shape):
        hi, lo = pred.copy(), pred.copy()
        hi[idx] += h
        lo[idx] -= h
        num[idx] = (up * (R.feature_loss(real, hi) - R.feature_loss(real, lo))).sum() / (2 * h)
    assert np.abs(g).max() > 0.01 and np.abs(g - num).max() <= 1e-8 * np.abs(g).max()
    # a whole sentence masked: loss 0, the padded tokens count in the mean
    real[0] = -10
    assert R.feature_loss(real, pred)[0] == 0.0 and not R.feature_grad(real, pred)[0].any()


def test_train_step_combination():
    labels, logits = R.seeded_labels((2, 6), 4, 23), R.seeded_logits((2, 6, 4), 23)
    real, pred = R.seeded_features((2, 6, 8), (2, 6, 8), 23)
    out = R.punc_losses(labels, real, logits, pred, global_batch_size=8)
    assert out["train_loss"] == pytest.approx((10 * out["feature_map_loss"] + out["bd_loss"]).sum() / 8, rel=1e-15)
    assert np.allclose(out["grad_bd_pred"], R.classes_grad(labels, logits) / 8, rtol=1e-15, atol=0)
    assert np.allclose(out["grad_out_feature"], R.feature_grad(real, pred) * 10 / 8, rtol=1e-15, atol=0)


def test_heads64_is_punc_probs_before_the_softmax():
    from punc_numpy import punc_probs
    from punc_onnx_eval import onnx_path
    punc = Punc(config(), device="cpu").load_onnx(onnx_path())
    ids = R.seeded_ids([11], 11, punc.cfg["vocab"], 3)[0]
    logits, feature = R.heads64(punc.weights, ids)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    assert np.abs(e / e.sum(-1, keepdims=True) - punc_probs(punc.weights, ids)).max() <= 1e-15
    assert logits.shape == (11, punc.cfg["classes"]) and feature.shape == (11, 768)


def test_library_exports_the_new_symbols():
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mi355asr_punc_heads_workspace_bytes", "mi355asr_punc_heads", "mi355asr_punc_classes_loss",
                 "mi355asr_masked_feature_mse_workspace_bytes", "mi355asr_masked_feature_mse"):
        assert name in _lib.SIGNATURES and hasattr(h, name)


P = ctypes.c_void_p(4096)          # a non-null address no call may reach: every case below is refused before a launch
NULL = ctypes.c_void_p()


def refused(rc, code, *words):
    msg = _lib.lib().mi355asr_last_error().decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_classes_loss_refuses_bad_arguments_before_a_launch():
    lib = _lib.lib()
    call = lambda **k: lib.mi355asr_punc_classes_loss(*[k.get(n, d) for n, d in (
        ("labels", P), ("ld_lab", 8), ("logits", P), ("ld_b", 8 * 65), ("ld_t", 65), ("upstream", NULL), ("B", 2), ("Q", 8), ("T", 8),
        ("C", 5), ("loss", P), ("acc", P), ("mean", P), ("grad", NULL), ("gld_b", 0), ("gld_t", 0), ("stream", NULL))])
    refused(call(C=65), -1, "C=65", "64")
    refused(call(C=0), -1, "C=0")
    refused(call(labels=NULL), -1, "labels_dev")
    refused(call(logits=NULL), -1, "logits_dev")
    refused(call(mean=NULL), -1, "null output")
    refused(call(B=0), -1, "B, Q, T")
    refused(call(ld_t=4), -1, "ld_t=4")
    refused(call(ld_lab=7), -1, "ld_lab=7")
    refused(call(grad=P, gld_t=4, gld_b=40), -1, "gld_t=4")
    with pytest.raises(ValueError, match="at most 64"):
        losses.punc_classes_loss(np.zeros((1, 3), np.int32), np.zeros((1, 3, 65), np.float32))
    with pytest.raises(ValueError, match=r"\[B, Q\]"):
        losses.punc_classes_loss(np.zeros((2, 3), np.int32), np.zeros((1, 3, 5), np.float32))
    with pytest.raises(ValueError, match=r"\[B, T, C\]"):
        losses.punc_classes_acc(np.zeros((1, 3), np.int32), np.zeros((3, 5), np.float32))


def test_feature_mse_refuses_bad_arguments_before_a_launch():
    lib = _lib.lib()
    call = lambda **k: lib.mi355asr_masked_feature_mse(*[k.get(n, d) for n, d in (
        ("real", P), ("rld_b", 8 * 768), ("rld_t", 768), ("pred", P), ("pld_b", 8 * 768), ("pld_t", 768), ("upstream", NULL), ("B", 2),
        ("T1", 8), ("T2", 8), ("F", 768), ("out", P), ("grad", NULL), ("gld_b", 0), ("gld_t", 0), ("ws", P), ("ws_bytes", 1 << 20),
        ("stream", NULL))])
    refused(call(real=NULL), -1, "real_dev")
    refused(call(pred=NULL), -1, "pred_dev")
    refused(call(out=NULL), -1, "out_dev")
    refused(call(F=0), -1, "F=0")
    refused(call(T2=0), -1, "T1, T2")
    refused(call(pld_t=767), -1, "overlap")
    refused(call(grad=P, gld_b=8 * 768, gld_t=5), -1, "gld_t=5")
    refused(call(ws=NULL), -4, "workspace")
    refused(call(ws_bytes=8), -4, "need")
    n = ctypes.c_size_t()
    assert lib.mi355asr_masked_feature_mse_workspace_bytes(2, 8, 11, ctypes.byref(n)) == 0 and n.value >= 2 * 8 * 8
    with pytest.raises(ValueError, match="differ in B or F"):
        losses.bert_feature_loss(np.zeros((2, 3, 8), np.float32), np.zeros((2, 3, 9), np.float32))
    with pytest.raises(ValueError, match="differ in B or F"):
        losses.bert_feature_loss(np.zeros((2, 3, 8), np.float32), np.zeros((1, 3, 8), np.float32))


def test_heads_refuses_both_outputs_null_and_an_interior_padding_id():
    lib = _lib.lib()
    h = ctypes.c_void_p()
    cfg = _lib.PuncConfig(d_model=64, enc_embedding_dim=64, num_heads=8, dff=64, num_layers=3, vocab=100, classes=5, pe_input=1024)
    assert lib.mi355asr_punc_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        refused(lib.mi355asr_punc_heads(h, P, NULL, 1, 4, NULL, NULL, NULL, 0, NULL), -1, "both null")
        refused(lib.mi355asr_punc_heads(h, P, NULL, 1, 4, P, NULL, NULL, 0, NULL), -2, "finalise")
        refused(lib.mi355asr_punc_heads(NULL, P, NULL, 1, 4, P, P, NULL, 0, NULL), -1, "Punc handle")
        n = ctypes.c_size_t(7)
        assert lib.mi355asr_punc_heads_workspace_bytes(h, 2, 144, ctypes.byref(n)) == 0 and n.value == 0
        m = ctypes.c_size_t()
        assert lib.mi355asr_punc_heads_workspace_bytes(h, 2, 145, ctypes.byref(n)) == 0
        assert lib.mi355asr_punc_workspace_bytes(h, 2, 145, ctypes.byref(m)) == 0 and n.value == m.value > 0
    finally:
        lib.mi355asr_destroy(h)
    assert lengths_from_ids(np.array([[5, 3, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4]])).tolist() == [2, 0, 4]
    with pytest.raises(ValueError, match="token 1 of row 0"):
        lengths_from_ids(np.array([[5, 0, 3, 0]]))
    with pytest.raises(ValueError, match="neither output"):
        Punc(config(), device="cpu").heads(np.ones((1, 3), np.int32), want_logits=False, want_feature=False)
