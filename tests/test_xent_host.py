"""Host tests of the Translator-head losses: the float64 restatement (tests/xent_ref.py) against hand-computed cases, against
torch.nn.functional.cross_entropy in float64 and against torch.autograd; the new entry points are declared, mirrored and exported,
and refuse bad arguments before they touch a device.  No kernel is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import xent_ref as xr
from helpers import ROOT
from tensorflowasr_amd import _lib, build

NEW = ("mi355asr_xent_workspace_bytes", "mi355asr_xent_rows", "mi355asr_mask_loss")


def test_hand_computed_batch_of_2x3x4():
    """logits whose softmax is known in closed form: a row of equal logits (loss log 4 whatever the label), a row log([1, 2, 3, 4])
    (p = k / 10) and a row with one logit log 7 over zeros (p = 7 / 10 or 1 / 10)"""
    eq = [0.5, 0.5, 0.5, 0.5]
    ramp = [math.log(k) for k in (1, 2, 3, 4)]
    peak = [0.0, math.log(7.0), 0.0, 0.0]
    logits = np.array([[eq, ramp, peak], [peak, eq, ramp]])
    labels = np.array([[2, 3, 1], [0, 0, 1]])
    loss = np.array([[math.log(4), -math.log(0.4), -math.log(0.7)], [-math.log(0.1), math.log(4), -math.log(0.2)]])
    np.testing.assert_allclose(xr.sparse_xent(logits, labels), loss, rtol=0, atol=1e-14)
    # the four terms of mask_loss: need = label != 0 (4 elements), zero = label == 0 (2 elements)
    row_mean = loss.mean(-1)
    need_loss = (loss[0].sum() + loss[1, 2]) / (4 + 1e-6)
    zero_loss = (loss[1, 0] + loss[1, 1]) / (2 + 1e-6)
    np.testing.assert_allclose(xr.mask_loss(labels, logits), row_mean + need_loss + zero_loss, rtol=0, atol=1e-14)
    # arg-max: row 0 = (0: all equal, 3, 1), row 1 = (1, 0, 3); needed and correct: (0,1) 3 == 3 and (0,2) 1 == 1 and (1,2) 1 != 3
    assert xr.argmax(logits).tolist() == [[0, 3, 1], [1, 0, 3]]
    assert abs(xr.translate_acc(labels, logits) - 2 / (4 + 1e-6)) < 1e-15
    # the min(T, Q) rule: a fourth label column is not used, and neither is a third logits column for two label columns
    wide = np.concatenate([labels, [[3], [3]]], 1)
    np.testing.assert_array_equal(xr.sparse_xent(logits, wide), xr.sparse_xent(logits, labels))
    assert xr.sparse_xent(logits, labels[:, :2]).shape == (2, 2)
    # ctc_acc: per row, over min(width) columns, pad excluded
    acc = xr.ctc_acc(np.array([[4, 5, 6, 0], [7, 0, 0, 0]]), np.array([[4, 9, 6], [7, 7, 7]]))
    np.testing.assert_allclose(acc, [2 / (3 + 1e-6), 1 / (1 + 1e-6)], rtol=0, atol=1e-15)


def test_denominators_without_zero_labels_and_with_only_zero_labels():
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((2, 3, 5))
    none_zero = np.array([[1, 2, 3], [4, 1, 2]])
    loss = xr.sparse_xent(logits, none_zero)
    # no zero label: the zero term is 0 / (0 + 1e-6) = 0, the need term sum / (6 + 1e-6)
    np.testing.assert_allclose(xr.mask_loss(none_zero, logits), loss.mean(-1) + loss.sum() / (6 + 1e-6), rtol=0, atol=1e-14)
    all_zero = np.zeros((2, 3), np.int64)
    loss0 = xr.sparse_xent(logits, all_zero)
    np.testing.assert_allclose(xr.mask_loss(all_zero, logits), loss0.mean(-1) + loss0.sum() / (6 + 1e-6), rtol=0, atol=1e-14)
    assert xr.translate_acc(all_zero, logits) == 0.0          # 0 / 1e-6
    w = xr.mask_loss_weights(all_zero, 3)
    np.testing.assert_allclose(w, np.full((2, 3), 1 / 3 + 2 / (6 + 1e-6)), rtol=0, atol=1e-15)


def test_restatement_against_torch_cross_entropy_in_float64():
    rng = np.random.default_rng(1)
    for B, Q, V in ((2, 3, 1), (3, 2, 7), (2, 4, 1332)):
        x = rng.standard_normal((B, Q, V)) * 3
        y = rng.integers(0, V, (B, Q))
        t = torch.nn.functional.cross_entropy(torch.from_numpy(x).reshape(-1, V), torch.from_numpy(y).reshape(-1), reduction="none")
        np.testing.assert_allclose(xr.sparse_xent(x, y), t.numpy().reshape(B, Q), rtol=0, atol=1e-12)
    # the special values the kernel has to get right, as the restatement states them
    x = np.array([[[1e30, 0.0, -1.0], [-1e30, -2e30, -3e30], [0.0, -np.inf, 1.0], [2.0, 2.0, 2.0]]])
    got = xr.sparse_xent(x, np.array([[0, 0, 1, 2]]))[0]
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == np.inf and abs(got[3] - math.log(3)) < 1e-15
    assert np.isnan(xr.sparse_xent(x, np.array([[-1, 3, 0, 0]]))[0, :2]).all()
    assert (xr.xent_grad(x, np.array([[-1, 3, 0, 0]]))[0, :2] == 0).all()
    assert np.isfinite(xr.xent_grad(x, np.array([[0, 0, 1, 2]]))).all()


def torch_mask_loss(labels, logits):
    """ctc_runners.py:69-76 in torch float64, for autograd"""
    q = min(labels.shape[1], logits.shape[1])
    y, x = labels[:, :q], logits[:, :q]
    loss = torch.nn.functional.cross_entropy(x.reshape(-1, x.shape[-1]), y.reshape(-1), reduction="none").reshape(y.shape)
    need, zero = (y != 0).double(), (y == 0).double()
    return loss.mean(-1) + (loss * need).sum() / (need.sum() + 1e-6) + (loss * zero).sum() / (zero.sum() + 1e-6)


def test_mask_loss_gradient_formula_against_autograd():
    rng = np.random.default_rng(2)
    B, T, Q, V = 3, 5, 4, 11
    x = rng.standard_normal((B, T, V)) * 3
    y = rng.integers(0, 3, (B, Q))
    y[0, 0], y[1, 1] = 0, 5
    up = np.array([0.5, -2.0, 3.25])
    xt = torch.from_numpy(x).requires_grad_(True)
    out = torch_mask_loss(torch.from_numpy(y), xt)
    np.testing.assert_allclose(out.detach().numpy(), xr.mask_loss(y, x), rtol=0, atol=1e-12)
    (out * torch.from_numpy(up)).sum().backward()
    want = xt.grad.numpy()
    got = xr.xent_grad(x, y, xr.mask_loss_weights(y, Q, up))
    np.testing.assert_allclose(got, want[:, :Q], rtol=0, atol=1e-13)
    assert (want[:, Q:] == 0).all()                                 # the columns past the labels take no part


def test_names_declared_mirrored_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355asr.h")).read()
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "api_xent.hip")).read()
    assert "xent.hip" in build.SOURCES and "api_xent.hip" in build.SOURCES and "xent.h" in build.HEADERS
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert hasattr(lib, name) and res is ctypes.c_int and len(args) == len(argtypes), name
        assert re.search(r"^int %s\(" % name, src, re.M), name
        for decl, ct in zip(args, argtypes):
            if "*" in decl:
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, decl)
            elif decl.startswith("size_t"):
                assert ct is ctypes.c_size_t, (name, decl)
            elif decl.startswith("int64_t"):
                assert ct is ctypes.c_int64, (name, decl)
            else:
                assert decl.startswith("int32_t") and ct is ctypes.c_int32, (name, decl)
    from tensorflowasr_amd import losses
    hsrc = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "xent.h")).read()
    assert ("kXentMaxV = 1 << %d;" % int(math.log2(losses.MAX_CLASSES))) in hsrc and losses.MAX_CLASSES >= 65536
    assert "kXentResidentV = kXentThreads * 4 * kXentSlots" in hsrc and "kXentThreads = 256" in hsrc
    assert ("kXentSlots = %d;" % (losses.RESIDENT_CLASSES // 1024)) in hsrc


def test_workspace_formula_and_refusals_before_any_launch():
    """the argument checks come before the first device call, so they run here: fake, never dereferenced pointers"""
    lib = _lib.lib()
    up = lambda n: (n + 255) // 256 * 256
    nb = ctypes.c_size_t(0)
    for B, Q in ((1, 1), (64, 20), (3, 250)):
        for g in (0, 1):
            assert lib.mi355asr_xent_workspace_bytes(B, Q, g, ctypes.byref(nb)) == 0
            assert nb.value == (2 + g) * up(4 * B * Q)
    P = ctypes.c_void_p(4096)
    N = ctypes.c_void_p()

    def refused(rc, word):
        msg = lib.mi355asr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.mi355asr_xent_workspace_bytes(0, 3, 0, ctypes.byref(nb)), "B")
    refused(lib.mi355asr_xent_workspace_bytes(2, -1, 0, ctypes.byref(nb)), "Q")
    refused(lib.mi355asr_xent_workspace_bytes(2, 3, 0, None), "bytes")
    rows = lambda **k: lib.mi355asr_xent_rows(*[k.get(n, d) for n, d in (
        ("x", P), ("ld_b", 60), ("ld_t", 20), ("labels", P), ("ld_lab", 3), ("w", N), ("B", 2), ("Q", 3), ("V", 20), ("loss", P),
        ("amax", N), ("grad", N), ("gld_b", 0), ("gld_t", 0), ("stream", N))])
    refused(rows(x=N), "x_dev")
    refused(rows(labels=N), "labels_dev")
    refused(rows(loss=N), "loss_dev")
    refused(rows(V=0), "V=0")
    refused(rows(V=(1 << 18) + 1, ld_t=1 << 19), "V=")
    refused(rows(ld_t=19), "ld_t")
    refused(rows(ld_b=-1), "ld_b")
    refused(rows(B=-2), "B")
    refused(rows(Q=-3), "Q")
    refused(rows(ld_lab=2), "ld_lab")
    refused(rows(grad=P, gld_b=60, gld_t=19), "gld_t")
    refused(rows(grad=P, gld_b=59, gld_t=20), "gld_b")
    ml = lambda **k: lib.mi355asr_mask_loss(*[k.get(n, d) for n, d in (
        ("x", P), ("ld_b", 60), ("ld_t", 20), ("labels", P), ("ld_lab", 3), ("up", N), ("B", 2), ("Q", 3), ("V", 20), ("out", P),
        ("acc", P), ("mean", P), ("grad", N), ("gld_b", 0), ("gld_t", 0), ("ws", P), ("ws_bytes", 512), ("stream", N))])
    for field, word in (("x", "x_dev"), ("labels", "labels_dev"), ("out", "mask_loss_dev"), ("acc", "acc_dev"), ("mean", "mean_dev"),
                        ("ws", "ws_dev")):
        refused(ml(**{field: N}), word)
    refused(ml(V=0), "V=0")
    refused(ml(ld_t=3), "ld_t")
    refused(ml(B=-1), "B")
    refused(ml(ws_bytes=511), "ws_bytes")
    refused(ml(grad=P, gld_b=60, gld_t=20, ws_bytes=512), "ws_bytes")      # the weights need a third plane
    refused(ml(ws=ctypes.c_void_p(4100)), "ws_dev")
