"""The Translator head's losses and the trainer's evaluation metrics on the GPU: the reference's
`tf.keras.losses.sparse_categorical_crossentropy(labels, logits, from_logits=True)`, `mask_loss`, `translate_acc` and `ctc_acc`
(asr/trainer/ctc_runners.py:48-76, 102, 144-146) with the gradient with respect to the logits (`mi355asr_xent_rows`,
`mi355asr_mask_loss`, csrc/xent.hip).

    loss = sparse_xent(logits, labels)                                   # f32 [B, Q']
    out, grad = mask_loss(labels, logits, return_grad=True)              # f32 [B], d sum(out) / d logits
    acc = translate_acc(labels, logits)                                  # f32 scalar
    accs = ctc_acc(phone_labels, decoded, pad=0)                         # f32 [B]

Everything returned is a device tensor; nothing here copies to the host or waits for the stream."""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 1 << 18           # kXentMaxV of csrc/xent.h
RESIDENT_CLASSES = 10240        # kXentResidentV: rows up to here are read from memory once


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def _device_of(logits, device):
    if device is not None:
        return torch.device(device)
    if torch.is_tensor(logits) and logits.is_cuda:
        return logits.device
    return torch.device("cuda:0")


def _inputs(logits, labels, device=None):
    """-> (x f32 on the device with unit stride over the classes, labels i32 [B, Q] contiguous, B, Q' = min(T, Q), V, device).
    A strided view of the logits (a column slice, a padded class axis) is used in place."""
    dev = _device_of(logits, device)
    if dev.type != "cuda":
        raise _lib.Mi355AsrError("the losses run on the GPU only (got device %s)" % dev)
    x = logits if torch.is_tensor(logits) else torch.from_numpy(np.ascontiguousarray(np.asarray(logits, dtype=np.float32)))
    if x.dim() != 3:
        raise ValueError("logits are [B, T, V] (got shape %s)" % (tuple(x.shape),))
    x = x.to(device=dev, dtype=torch.float32)
    B, T, V = x.shape
    if B < 1 or T < 1 or V < 1:
        raise ValueError("empty logits %s" % (tuple(x.shape),))
    if x.stride(2) != 1 and V > 1 or x.stride(1) < V or x.stride(0) < 0:
        x = x.contiguous()
    y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.int32)))
    if y.dim() != 2 or y.shape[0] != B:
        raise ValueError("labels are [B, Q] with the B of the logits (got %s for %d rows)" % (tuple(y.shape), B))
    y = y.to(device=dev, dtype=torch.int32).contiguous()
    Q = min(T, y.shape[1])
    if Q < 1:
        raise ValueError("no label column")
    return x, y, B, Q, V, dev


def sparse_xent(logits, labels, weights=None, return_grad=False, return_argmax=False):
    """tf.keras.losses.sparse_categorical_crossentropy(labels, logits, from_logits=True): loss[b, t] = logsumexp(logits[b, t]) -
    logits[b, t, labels[b, t]].  logits f32 [B, T, V] (may be a strided view: it is read in place), labels int [B, Q]; the first
    Q' = min(T, Q) columns of both are used, the rule `ctc_acc` applies to its two operands -- TensorFlow raises when T < Q (the
    shapes of labels and logits must agree), so a caller who wants that behaviour checks the widths first.
    -> loss f32 [B, Q'], then with return_grad the gradient f32 [B, Q', V] = weights[b, t] * (softmax - onehot) (weights f32
    [B, Q'], None = ones), then with return_argmax the per-row arg-max i32 [B, Q'] (ties: the lowest index).
    A label outside [0, V) gives loss NaN and a zero gradient row."""
    lib = _lib.lib()
    x, y, B, Q, V, dev = _inputs(logits, labels)
    w = None
    if weights is not None:
        w = weights if torch.is_tensor(weights) else torch.from_numpy(np.asarray(weights, dtype=np.float32))
        w = w.to(device=dev, dtype=torch.float32)[:, :Q].contiguous()
        if tuple(w.shape) != (B, Q):
            raise ValueError("weights are [B, Q'] = [%d, %d] (got %s)" % (B, Q, tuple(w.shape)))
    loss = torch.empty((B, Q), dtype=torch.float32, device=dev)
    amax = torch.empty((B, Q), dtype=torch.int32, device=dev) if return_argmax else None
    grad = torch.empty((B, Q, V), dtype=torch.float32, device=dev) if return_grad else None
    launch_rows(lib, x, y, w, B, Q, V, loss, amax, grad, dev)
    out = (loss,) + ((grad,) if return_grad else ()) + ((amax,) if return_argmax else ())
    return out if len(out) > 1 else loss


def launch_rows(lib, x, y, w, B, Q, V, loss, amax, grad, dev, ld=None, gld=None):
    """The C call on buffers the caller owns (the tests hand in poisoned outputs and their own strides)."""
    ld_b, ld_t = ld if ld is not None else (x.stride(0), x.stride(1))
    gld_b, gld_t = gld if gld is not None else ((grad.stride(0), grad.stride(1)) if grad is not None else (0, 0))
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mi355asr_xent_rows(_p(x), ld_b, ld_t, _p(y), y.stride(0) if y is not None else 0, _p(w), B, Q, V, _p(loss),
                                          _p(amax), _p(grad), gld_b, gld_t, st))


def _mask_loss_call(labels, logits, upstream=None, return_grad=False):
    """one `mi355asr_mask_loss`: -> (mask_loss f32 [B], translate_acc f32 [], mean loss f32 [], gradient [B, T, V] or None)"""
    lib = _lib.lib()
    x, y, B, Q, V, dev = _inputs(logits, labels)
    g = None
    if upstream is not None:
        g = upstream if torch.is_tensor(upstream) else torch.from_numpy(np.asarray(upstream, dtype=np.float32))
        g = g.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if g.numel() != B:
            raise ValueError("upstream holds %d values for %d rows" % (g.numel(), B))
    nbytes = ctypes.c_size_t()
    _lib.check(lib.mi355asr_xent_workspace_bytes(B, Q, int(bool(return_grad)), ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    scal = torch.empty((2,), dtype=torch.float32, device=dev)
    grad = None
    if return_grad:
        T = x.shape[1]
        # the columns t >= Q' of the logits take no part in the loss: their gradient is 0, and the kernel does not touch them
        grad = torch.empty((B, T, V), dtype=torch.float32, device=dev) if T == Q else torch.zeros((B, T, V), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mi355asr_mask_loss(_p(x), x.stride(0), x.stride(1), _p(y), y.stride(0), _p(g), B, Q, V, _p(out), _p(scal[0:1]),
                                          _p(scal[1:2]), _p(grad), grad.stride(0) if return_grad else 0,
                                          grad.stride(1) if return_grad else 0, _p(ws), nbytes.value, st))
    return out, scal[0], scal[1], grad


def mask_loss(labels, logits, return_grad=False, upstream=None):
    """CTCTrainer.mask_loss (ctc_runners.py:69-76): with loss = sparse_xent(logits, labels), need = (labels != 0) and zero =
    (labels == 0) over the used columns,  out[b] = mean_t loss[b, t] + sum(loss * need) / (sum(need) + 1e-6) + sum(loss * zero) /
    (sum(zero) + 1e-6)  -> f32 [B]; the sums are taken in float64 on the device.
    return_grad: also d (sum_b upstream[b] * out[b]) / d logits, f32 with the shape of the logits (upstream f32 [B], None =
    ones): the rows kernel scales softmax - onehot of element (b, t) by g_b / Q' + G * need / (N_need + 1e-6) + G * zero /
    (N_zero + 1e-6), G = sum(upstream); that weight is formed on the device."""
    out, _, _, grad = _mask_loss_call(labels, logits, upstream, return_grad)
    return (out, grad) if return_grad else out


def translate_acc(labels, logits):
    """CTCTrainer.translate_acc (ctc_runners.py:63-68): sum((argmax(logits, -1) == labels) * need) / (sum(need) + 1e-6) over the
    first min(T, Q) columns -> f32 scalar on the device."""
    return _mask_loss_call(labels, logits)[1]


def translate_metrics(labels, logits):
    """What `CTCTrainer._eval_step` hands its `translate_loss` and `translate_acc` metrics, from one pass over the logits:
    -> (the mean of sparse_xent over all B x Q' elements, translate_acc), two f32 scalars on the device."""
    _, acc, mean, _ = _mask_loss_call(labels, logits)
    return mean, acc


def ctc_acc(labels, decoded, pad=0):
    """CTCTrainer.ctc_acc (ctc_runners.py:48-62): over the first min(width) columns of both, per row
    sum((labels == decoded) * (labels != pad)) / (sum(labels != pad) + 1e-6) -> f32 [B].  Plain tensor arithmetic on the device
    the decoded ids are on."""
    d = decoded if torch.is_tensor(decoded) else torch.from_numpy(np.ascontiguousarray(np.asarray(decoded, dtype=np.int32)))
    dev = d.device if d.is_cuda else torch.device("cuda:0")
    y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.int32)))
    d, y = d.to(dev), y.to(dev)
    T = min(d.shape[1], y.shape[1])
    d, y = d[:, :T].to(torch.float32), y[:, :T].to(torch.float32)
    mask = (y != float(pad)).to(torch.float32)
    value = (y == d).to(torch.float32)
    return (value * mask).sum(-1) / (mask.sum(-1) + 1e-6)
