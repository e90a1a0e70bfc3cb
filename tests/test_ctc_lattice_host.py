"""CTC loss / gradient / forced alignment, the part that needs no GPU: the C ABI's names and its argument checks (which all come
before the first device call), and the yardsticks of tests/test_gpu_ctc_lattice.py pinned against brute force."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_yardstick as cy
from tensorflowasr_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mi355asr_ctc_loss_workspace_bytes": 6, "mi355asr_ctc_loss": 15, "mi355asr_ctc_align_workspace_bytes": 5,
         "mi355asr_ctc_align": 16}


def test_names_declared_mirrored_and_exported():
    header = open(os.path.join(ROOT, "include", "mi355asr.h")).read()
    h = _lib.lib()
    for name, nargs in NAMES.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/mi355asr.h" % name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(h, name), "%s is not exported by libmi355asr.so" % name
    assert "replaces: tf.keras.backend.ctc_batch_cost" in header and "ctc_runners.py:91,133" in header
    assert "api_ctc.hip" in build.SOURCES and "ctc_lattice.hip" in build.SOURCES


def _loss_args(**kw):
    """a well-formed mi355asr_ctc_loss call on pointers that are never dereferenced (every check precedes the device)"""
    a = dict(x=0x1000, is_logits=1, in_len=0x2000, labels=0x3000, label_len=0x4000, B=2, T=50, V=20, U=5, blank=19,
             loss=0x5000, grad=0x6000, ws=0x7000, ws_bytes=None, stream=None)
    a.update(kw)
    return a


def _call_loss(h, a):
    if a["ws_bytes"] is None:
        n = ctypes.c_size_t()
        assert h.mi355asr_ctc_loss_workspace_bytes(a["B"], a["T"], a["V"], a["U"], int(bool(a["grad"])), ctypes.byref(n)) == 0
        a["ws_bytes"] = n.value
    return h.mi355asr_ctc_loss(a["x"], a["is_logits"], a["in_len"], a["labels"], a["label_len"], a["B"], a["T"], a["V"], a["U"],
                               a["blank"], a["loss"], a["grad"], a["ws"], a["ws_bytes"], a["stream"])


def _call_align(h, a):
    if a["ws_bytes"] is None:
        n = ctypes.c_size_t()
        assert h.mi355asr_ctc_align_workspace_bytes(a["B"], a["T"], a["V"], a["U"], ctypes.byref(n)) == 0
        a["ws_bytes"] = n.value
    return h.mi355asr_ctc_align(a["x"], a["is_logits"], a["in_len"], a["labels"], a["label_len"], a["B"], a["T"], a["V"], a["U"],
                                a["blank"], a["path"], a["spans"], a["score"], a["ws"], a["ws_bytes"], a["stream"])


def _align_args(**kw):
    a = _loss_args()
    del a["loss"], a["grad"]
    a.update(path=0x5000, spans=0x6000, score=0x8000)
    a.update(kw)
    return a


BAD = [("V < 2", dict(V=1, blank=0)), ("blank below 0", dict(blank=-1)), ("blank == V", dict(blank=20)),
       ("workspace too small", dict(ws_bytes=64)), ("null workspace", dict(ws=None))]


@pytest.mark.parametrize("what,kw", BAD + [("null loss", dict(loss=None)),
                                           ("gradient of the probabilities entry", dict(is_logits=0))])
def test_ctc_loss_rejects(what, kw):
    h = _lib.lib()
    a = _loss_args(**kw)
    if what == "V < 2":
        a["ws_bytes"] = 1 << 20
    assert _call_loss(h, a) == -1, what
    assert h.mi355asr_last_error().decode() != "", what


@pytest.mark.parametrize("what,kw", BAD + [("null path", dict(path=None)), ("null spans", dict(spans=None)),
                                           ("null score", dict(score=None))])
def test_ctc_align_rejects(what, kw):
    h = _lib.lib()
    a = _align_args(**kw)
    if what == "V < 2":
        a["ws_bytes"] = 1 << 20
    assert _call_align(h, a) == -1, what
    assert h.mi355asr_last_error().decode() != "", what


def test_built_limit_on_label_positions():
    h = _lib.lib()
    n = ctypes.c_size_t()
    assert h.mi355asr_ctc_loss_workspace_bytes(1, 600, 20, 256, 1, ctypes.byref(n)) == 0 and n.value > 0     # at least 256
    assert h.mi355asr_ctc_align_workspace_bytes(1, 600, 20, 256, ctypes.byref(n)) == 0 and n.value > 0
    for U in (100000,):
        assert h.mi355asr_ctc_loss_workspace_bytes(1, 600, 20, U, 1, ctypes.byref(n)) == -1
        assert "built for up to" in h.mi355asr_last_error().decode()
        assert h.mi355asr_ctc_align_workspace_bytes(1, 600, 20, U, ctypes.byref(n)) == -1
        assert _call_loss(h, _loss_args(U=U, ws_bytes=1 << 30)) == -1
        assert _call_align(h, _align_args(U=U, ws_bytes=1 << 30)) == -1


def test_workspace_grows_with_the_gradient():
    h = _lib.lib()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert h.mi355asr_ctc_loss_workspace_bytes(4, 100, 50, 10, 0, ctypes.byref(a)) == 0
    assert h.mi355asr_ctc_loss_workspace_bytes(4, 100, 50, 10, 1, ctypes.byref(b)) == 0
    assert b.value >= a.value + 2 * 4 * 100 * 21 * 4                  # alpha and beta of every state


def test_wrapper_checks_host_labels():
    """a label equal to the blank or outside [0, V), seen on the host side of the wrapper, is an error before any device work"""
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    z = np.zeros((1, 6, 4), np.float32)
    for bad in ([[0, 3]], [[0, 4]], [[-1, 0]]):
        for fn in (ctc_loss, ctc_forced_align):
            with pytest.raises(_lib.Mi355AsrError, match="label"):
                fn(z, np.array(bad, np.int32))


@pytest.mark.parametrize("i", range(len(cy.TINY)))
def test_yardsticks_equal_brute_force(i):
    """V = 4, T <= 6: the float64 torch chain equals the sum over all V^T paths, the NumPy Viterbi equals the best enumerated
    path -- the two yardsticks of the GPU tests pinned independently of each other (and of the code under test)"""
    labels, T = cy.TINY[i]
    z = cy.tiny_logits(i, T)
    lq = cy.log_q(z)[0].numpy()
    assert abs(np.exp(lq).sum(-1) - 1).max() < 1e-12
    nll, best, best_path, unique = cy.brute_force(lq, labels, 3)
    lab = np.array([labels + [0] * (3 - len(labels))], np.int32)
    loss, grad = cy.torch_chain(z, lab, [T], [len(labels)])
    score, path = cy.viterbi(lq, labels, 3)
    assert abs(loss[0] - nll) <= 1e-12 * max(1.0, abs(nll))
    assert abs(score - best) <= 1e-12 * max(1.0, abs(best))
    assert cy.collapse(path, 3) == labels and abs(cy.path_logprob(lq, path) - best) <= 1e-12 * max(1.0, abs(best))
    if unique:
        assert np.array_equal(path, best_path)
    assert np.isfinite(grad).all() and abs(grad.sum(-1)).max() < 1e-12      # a softmax gradient sums to 0 over the classes


def test_yardstick_infeasible_and_float32():
    z = cy.tiny_logits(50, 3)
    loss, _ = cy.torch_chain(z, np.array([[0, 0]], np.int32), [3], [2], want_grad=False)      # [a, a] needs 3 frames: feasible
    assert np.isfinite(loss[0])
    loss, _ = cy.torch_chain(z, np.array([[0, 0]], np.int32), [2], [2], want_grad=False)      # ... and 2 are too few
    assert np.isinf(loss[0]) and loss[0] > 0
    assert cy.viterbi(cy.log_q(z)[0].numpy()[:2], [0, 0], 3) == (float("-inf"), None)
    z, lab, il, ll = cy.make_case(3, 4, 40, 30, 8, boost=6.0)
    l64, g64 = cy.torch_chain(z, lab, il, ll)
    l32, g32 = cy.torch_chain(z, lab, il, ll, dtype=torch.float32)
    assert np.isfinite(l64).all() and abs(l32 - l64).max() < 1e-3 and abs(g32 - g64).max() < 1e-3
    for b in range(4):
        assert np.all(g64[b, il[b]:] == 0)
