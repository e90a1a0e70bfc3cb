"""The Translator head's losses and the trainer's evaluation metrics on the GPU: the reference's
`tf.keras.losses.sparse_categorical_crossentropy(labels, logits, from_logits=True)`, `mask_loss`, `translate_acc` and `ctc_acc`
(asr/trainer/ctc_runners.py:48-76, 102, 144-146) with the gradient with respect to the logits (`mi355asr_xent_rows`,
`mi355asr_mask_loss`, csrc/xent.hip).

    loss = sparse_xent(logits, labels)                                   # f32 [B, Q']
    out, grad = mask_loss(labels, logits, return_grad=True)              # f32 [B], d sum(out) / d logits
    acc = translate_acc(labels, logits)                                  # f32 scalar
    accs = ctc_acc(phone_labels, decoded, pad=0)                         # f32 [B]

The VAD trainer's losses (vad/trainer/vad_trainer.py, vad/utils/stft.py; `mi355asr_stft_loss`, `mi355asr_vad_mask_stats`,
csrc/stft_loss.hip):

    wav_loss = MultiResolutionSTFTLoss()(wav_label, enhanced)            # f32 scalar, TFMultiResolutionSTFT.call
    wav_loss, grad = MultiResolutionSTFTLoss()(wav_label, enhanced, return_grad=True)
    one, zero = vad_mask_loss(vad_label, logits)                         # VADTrainer.mask_loss
    m = vad_metrics(vad_label, logits)                                   # acc (binary_accuracy), f1, tp, fp, fn, tn

The punctuation trainer's losses (punc_recover/trainer/punc_trainer.py:93-126; `mi355asr_punc_classes_loss`,
`mi355asr_masked_feature_mse`, csrc/punc_loss.hip) on the outputs of `Punc.heads`:

    bd_loss = punc_classes_loss(tar_bd, bd_pred)                         # f32 [B], PuncTrainer.classes_loss
    bd_acc = punc_classes_acc(tar_bd, bd_pred)                           # f32 scalar, PuncTrainer.classes_acc
    feature_map_loss = bert_feature_loss(feature, out_feature)           # f32 [B], PuncTrainer.bert_feature_loss
    out = punc_losses(tar_bd, feature, bd_pred, out_feature, return_grad=True)   # the train step's values and gradients

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


# ---- the VAD trainer's losses ----------------------------------------------------------------------------------------------------------
OLA_TILE = 256                  # kLossOlaTile of csrc/stft_loss.hip: gradient samples per workgroup of the overlap-add
FRAMES_PER_WORKGROUP = 1        # one frame of one row per workgroup of the frame kernel
MAX_RESOLUTIONS = 4
FFT_LENGTHS = (512, 1024, 2048)


def _wave(t, dev, what):
    """[B, L] or the trainer's [B, T, frame] -> f32 [B, L] on the device with unit stride along L (a strided view is used in place)"""
    x = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float32)))
    if x.dim() == 3:
        x = x.reshape(x.shape[0], -1)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s is [B, L] or [B, T, frame] (got shape %s)" % (what, tuple(x.shape)))
    x = x.to(device=dev, dtype=torch.float32)
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _counts(lengths, B, dev):
    if lengths is None:
        return None
    n = lengths if torch.is_tensor(lengths) else torch.from_numpy(np.asarray(lengths, dtype=np.int32))
    n = n.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if n.numel() != B:
        raise ValueError("lengths holds %d values for %d rows" % (n.numel(), B))
    return n


class MultiResolutionSTFTLoss:
    """TFMultiResolutionSTFT of vad/utils/stft.py on the GPU.  Per resolution r = (fft_length, frame_length, frame_step), with
    P, T = tf.signal.stft(prediction), tf.signal.stft(truth) (periodic Hann of frame_length at the start of the FFT frame, no
    centring, F = 1 + (L - frame_length) // step frames) and p = sqrt(|P|^2 + 1e-7) + 1e-6, t likewise:
        sc[b, r]  = ||p_b - t_b||_F / (||p_b||_F + 1e-6)      (the denominator is the PREDICTED magnitude, as the reference has it)
        mag[b, r] = mean over the row's frames and bins of (log p - log t)^2
    The scalar is mean_r(mean_b sc) + mean_r(mean over all valid frames of the batch of (log p - log t)^2): with equal lengths
    exactly TFMultiResolutionSTFT.call(y_true, y_pred).  1 to 4 resolutions, fft_length 512, 1024 or 2048,
    1 <= frame_length <= fft_length, 1 <= frame_step <= frame_length; anything else is a ValueError."""

    def __init__(self, fft_lengths=(1024, 512), frame_lengths=(600, 250), frame_steps=(120, 50), device="cuda:0"):
        fft, fl, st = [int(v) for v in fft_lengths], [int(v) for v in frame_lengths], [int(v) for v in frame_steps]
        if not (len(fft) == len(fl) == len(st)) or not 1 <= len(fft) <= MAX_RESOLUTIONS:
            raise ValueError("1 to %d resolutions, the three lists of equal length (got %d, %d, %d)" % (MAX_RESOLUTIONS, len(fft), len(fl), len(st)))
        for n, l, s in zip(fft, fl, st):
            if n not in FFT_LENGTHS:
                raise ValueError("fft_length %d is not one of %s" % (n, FFT_LENGTHS))
            if not 1 <= l <= n:
                raise ValueError("need 1 <= frame_length <= fft_length (got %d, %d)" % (l, n))
            if not 1 <= s <= l:
                raise ValueError("need 1 <= frame_step <= frame_length (got %d, %d)" % (s, l))
        self.resolutions = list(zip(fft, fl, st))
        self.R = len(fft)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Mi355AsrError("the losses run on the GPU only (got device %s)" % self.device)
        arr = ctypes.c_int32 * self.R
        self._fft, self._fl, self._st = arr(*fft), arr(*fl), arr(*st)

    def _call(self, y_true, y_pred, lengths, w_sc=None, w_mag=None, grad=None):
        """one `mi355asr_stft_loss` on [B, L] device tensors -> (sc, mag, frames); `grad` f32 [B, >= L] is written when given"""
        lib = _lib.lib()
        dev = self.device
        t, p = _wave(y_true, dev, "y_true"), _wave(y_pred, dev, "y_pred")
        if t.shape != p.shape:
            raise ValueError("y_true %s and y_pred %s differ in shape" % (tuple(t.shape), tuple(p.shape)))
        B, L = t.shape
        n = _counts(lengths, B, dev)
        nbytes = ctypes.c_size_t()
        _lib.check(lib.mi355asr_stft_loss_workspace_bytes(B, L, self.R, self._fft, self._fl, self._st, int(grad is not None), ctypes.byref(nbytes)))
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
        sc = torch.empty((B, self.R), dtype=torch.float32, device=dev)
        mag = torch.empty((B, self.R), dtype=torch.float32, device=dev)
        frames = torch.empty((B, self.R), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.mi355asr_stft_loss(_p(t), t.stride(0), _p(p), p.stride(0), _p(n), B, L, self.R, self._fft, self._fl, self._st,
                                              _p(sc), _p(mag), _p(frames), _p(w_sc), _p(w_mag), _p(grad),
                                              grad.stride(0) if grad is not None else 0, _p(ws), nbytes.value, st))
        return sc, mag, frames

    def rows(self, y_true, y_pred, lengths=None):
        """-> sc f32 [B, R], mag f32 [B, R] (NaN for a row without a frame at that resolution, where sc is 0), frames i32 [B, R].
        A row is computed from its own samples below lengths[b] alone."""
        return self._call(y_true, y_pred, lengths)

    def grad_rows(self, y_true, y_pred, w_sc, w_mag, lengths=None, out=None):
        """d / d y_pred of sum_{b, r} (w_sc[b, r] sc[b, r] + w_mag[b, r] mag[b, r]) for caller-given coefficients f32 [B, R]
        -> (sc, mag, frames, grad f32 [B, L]).  Every element of the gradient is written: 0 at and past lengths[b] and where no
        frame reaches.  Where ||p - t|| == 0 the sc term contributes 0 (TensorFlow's gradient is NaN there); a resolution at
        which the row has no frame contributes nothing.  `out`: a caller-owned f32 [B, >= L] buffer with unit stride."""
        dev = self.device
        p = _wave(y_pred, dev, "y_pred")
        B, L = p.shape
        w = [torch.as_tensor(v, dtype=torch.float32, device=dev).reshape(B, self.R).contiguous() for v in (w_sc, w_mag)]
        grad = out if out is not None else torch.empty((B, L), dtype=torch.float32, device=dev)
        sc, mag, frames = self._call(y_true, p, lengths, w[0], w[1], grad)
        return sc, mag, frames, grad[:, :L]

    def _weights(self, frames, upstream):
        f = frames.to(torch.float64)
        B = f.shape[0]
        tot = f.sum(0, keepdim=True)
        w_mag = torch.where(tot > 0, f / (self.R * tot), torch.zeros_like(f))
        w_sc = torch.full_like(f, 1.0 / (self.R * B))
        if upstream is not None:
            u = torch.as_tensor(upstream, dtype=torch.float64, device=f.device).reshape(())
            w_sc, w_mag = w_sc * u, w_mag * u
        return w_sc, w_mag, tot

    def _scalar(self, sc, mag, frames):
        w_sc, w_mag, tot = self._weights(frames, None)
        m = torch.where(frames > 0, mag.to(torch.float64), torch.zeros((), dtype=torch.float64, device=mag.device))
        v = (w_sc * sc.to(torch.float64)).sum() + (w_mag * m).sum()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=mag.device)
        return torch.where((tot > 0).all(), v, nan).to(torch.float32)      # a resolution without any frame: the mean of nothing

    def __call__(self, y_true, y_pred, lengths=None, return_grad=False, upstream=None):
        """-> the reference's scalar (f32, on the device); with return_grad also upstream * d scalar / d y_pred, f32 with the
        [B, L] shape of the flattened input (upstream: a scalar, None = 1).  With ragged `lengths` the mag term of a resolution
        is the mean over all valid frames of the batch: w_mag[b, r] = F[b, r] / (R sum_b F[b, r]), w_sc = 1 / (R B).
        The coefficients depend on the frame counts alone, which follow from the lengths: they are formed on the device before
        the one C call, and nothing waits for the stream."""
        if not return_grad:
            return self._scalar(*self._call(y_true, y_pred, lengths))
        p = _wave(y_pred, self.device, "y_pred")
        B, L = p.shape
        n = _counts(lengths, B, self.device)
        Lb = torch.full((B,), L, dtype=torch.int64, device=self.device) if n is None else n.to(torch.int64).clamp(0, L)
        zero = torch.zeros_like(Lb)
        frames = torch.stack([torch.where(Lb >= fl, 1 + (Lb - fl) // st, zero) for _, fl, st in self.resolutions], 1)
        w_sc, w_mag, _ = self._weights(frames, upstream)
        sc, mag, frames, grad = self.grad_rows(y_true, p, w_sc, w_mag, n)
        return self._scalar(sc, mag, frames), grad


def _mask_stats(labels, logits, lengths, threshold, return_grad):
    lib = _lib.lib()
    dev = _device_of(logits, None)
    if dev.type != "cuda":
        raise _lib.Mi355AsrError("the losses run on the GPU only (got device %s)" % dev)

    def two_d(t, what):
        x = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float32)))
        if x.dim() == 3 and x.shape[2] == 1:
            x = x[:, :, 0]
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("%s is [B, T] or [B, T, 1] (got shape %s)" % (what, tuple(x.shape)))
        x = x.to(device=dev, dtype=torch.float32)
        if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
            x = x.contiguous()
        return x
    z, x = two_d(labels, "labels"), two_d(logits, "logits")
    if z.shape != x.shape:
        raise ValueError("labels %s and logits %s differ in shape" % (tuple(z.shape), tuple(x.shape)))
    B, T = x.shape
    n = _counts(lengths, B, dev)
    sums = torch.empty((4,), dtype=torch.float64, device=dev)
    cnt = torch.empty((4,), dtype=torch.int64, device=dev)
    grad = torch.empty((B, T), dtype=torch.float32, device=dev) if return_grad else None
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mi355asr_vad_mask_stats(_p(z), z.stride(0), _p(x), x.stride(0), _p(n), B, T, float(threshold), _p(sums), _p(cnt),
                                               _p(grad), T, st))
    return sums, cnt, grad


def vad_mask_stats(labels, logits, lengths=None, threshold=0.5, return_grad=False):
    """One launch over labels and logits f32 [B, T] (or [B, T, 1]); frames t >= lengths[b] take no part.
    -> sums f64 [4] = (sum loss*one, sum one, sum loss*zero, sum zero) with loss = max(x, 0) - x z + log1p(exp(-|x|)),
    one = (z == 1), zero = (z == 0); counts i64 [4] = (TP, FP, FN, TN) of the decision logit > threshold against one / zero;
    with return_grad also d (one_loss + zero_loss) / d logits f32 [B, T] (0 past a row's count)."""
    sums, cnt, grad = _mask_stats(labels, logits, lengths, threshold, return_grad)
    return (sums, cnt, grad) if return_grad else (sums, cnt)


def vad_mask_loss(labels, logits, lengths=None, return_grad=False):
    """VADTrainer.mask_loss (vad_trainer.py:42-48): loss = binary_crossentropy(y, logits, from_logits=True),
    one_loss = sum(loss * [y == 1]) / (sum[y == 1] + 1e-6) over the WHOLE batch, zero_loss likewise with [y == 0]
    -> (one_loss, zero_loss) f32 scalars on the device (vad_loss is their sum); with return_grad also
    d (one_loss + zero_loss) / d logits.  The sums are taken in float64 on the device."""
    sums, _, grad = _mask_stats(labels, logits, lengths, 0.5, return_grad)
    one = (sums[0] / (sums[1] + 1e-6)).to(torch.float32)
    zero = (sums[2] / (sums[3] + 1e-6)).to(torch.float32)
    return (one, zero, grad) if return_grad else (one, zero)


def vad_metrics(labels, logits, threshold=0.5, lengths=None):
    """-> dict of device scalars: acc = mean(binary_accuracy(y, logits)) of the trainer, which compares the RAW logit with the
    threshold (logit > 0.5, not the probability); f1 = 2 TP / (2 TP + FP + FN), 0 when that denominator is 0; tp, fp, fn, tn
    (i64).  The reference's VadTester cannot run as written (it reads a config key no config has and calls .result of None), so
    F1 is the ordinary binary F1 from these counts; the reference does not pin it."""
    _, c, _ = _mask_stats(labels, logits, lengths, threshold, False)
    tp, fp, fn, tn = c[0], c[1], c[2], c[3]
    cf = c.to(torch.float64)
    den = 2 * cf[0] + cf[1] + cf[2]
    f1 = torch.where(den > 0, 2 * cf[0] / torch.clamp(den, min=1.0), torch.zeros_like(den))
    return {"acc": ((cf[0] + cf[3]) / cf.sum()).to(torch.float32), "f1": f1.to(torch.float32), "tp": tp, "fp": fp, "fn": fn, "tn": tn}


# ---- the punctuation trainer's losses --------------------------------------------------------------------------------------------------
MAX_PUNC_CLASSES = 64           # kMaxClasses of csrc/punc.hip and csrc/punc_loss.hip
FEATURE_MASK_VALUE = -10.0      # the dataloader's padding of the BERT features


def _as_tensor(t, dtype):
    return t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=dtype)))


def _rows3(t, dev):
    """[B, T, F] -> f32 on the device, used in place when the last axis has unit stride and the rows do not overlap"""
    x = t.to(device=dev, dtype=torch.float32)
    B, T, F = x.shape
    if F > 1 and x.stride(2) != 1 or T > 1 and x.stride(1) < F or B > 1 and x.stride(0) < F or x.stride(0) < 0 or x.stride(1) < 0:
        x = x.contiguous()
    return x


def _upstream(upstream, B, dev):
    if upstream is None:
        return None
    g = _as_tensor(upstream, np.float32).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if g.numel() != B:
        raise ValueError("upstream holds %d values for %d rows" % (g.numel(), B))
    return g


def _punc_classes_call(real, pred, upstream=None, return_grad=False):
    """one `mi355asr_punc_classes_loss` -> (loss f32 [B], acc f32 [B], mean acc f32 [], gradient [B, T, C] or None)"""
    x, y = _as_tensor(pred, np.float32), _as_tensor(real, np.int32)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("pred is [B, T, C], not empty (got shape %s)" % (tuple(x.shape),))
    B, T, C = x.shape
    if C > MAX_PUNC_CLASSES:
        raise ValueError("%d classes: the punctuation losses take at most %d (for a wide class axis see mask_loss)" % (C, MAX_PUNC_CLASSES))
    if y.dim() != 2 or y.shape[0] != B or y.shape[1] < 1:
        raise ValueError("real is [B, Q] with the B of pred and Q >= 1 (got %s for %d rows)" % (tuple(y.shape), B))
    dev = _device_of(x, None)
    if dev.type != "cuda":
        raise _lib.Mi355AsrError("the losses run on the GPU only (got device %s)" % dev)
    lib = _lib.lib()
    x = _rows3(x, dev)
    y = y.to(device=dev, dtype=torch.int32).contiguous()
    g = _upstream(upstream, B, dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    acc = torch.empty((B,), dtype=torch.float32, device=dev)
    mean = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((B, T, C), dtype=torch.float32, device=dev) if return_grad else None
    launch_punc_classes(lib, y, x, g, B, y.shape[1], T, C, loss, acc, mean, grad, dev)
    return loss, acc, mean, grad


def launch_punc_classes(lib, y, x, g, B, Q, T, C, loss, acc, mean, grad, dev):
    """The C call on buffers the caller owns (the tests hand in poisoned outputs and strided views)."""
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mi355asr_punc_classes_loss(_p(y), y.stride(0), _p(x), x.stride(0), x.stride(1), _p(g), B, Q, T, C, _p(loss), _p(acc),
                                                  _p(mean), _p(grad), grad.stride(0) if grad is not None else 0,
                                                  grad.stride(1) if grad is not None else 0, st))


def punc_classes_loss(real, pred, return_grad=False, upstream=None):
    """PuncTrainer.classes_loss (punc_trainer.py:104-115): real int [B, Q] (0 = padding, 1 = no mark), pred f32 [B, T, C <= 64]
    logits (a strided view is read in place); the first Q' = min(T, Q) columns of both are used, the rule `sparse_xent`
    documents.  With xe = sparse_xent, m = (real != 0), m1 = m * (real != 1):
        loss[b] = sum(xe m) / (sum m + 1e-6) + sum(xe m1) / (sum m1 + 1e-6)      -> f32 [B] (the reference keeps a trailing 1)
    return_grad: also d (sum_b upstream[b] loss[b]) / d pred, f32 with the shape of pred (upstream f32 [B], None = ones); zeros for
    t >= Q' and where real == 0.  A label outside [0, C) gives loss NaN and a zero gradient row.  Sums in float64 on the device."""
    loss, _, _, grad = _punc_classes_call(real, pred, upstream, return_grad)
    return (loss, grad) if return_grad else loss


def punc_classes_acc(real, pred):
    """PuncTrainer.classes_acc (punc_trainer.py:118-126): the batch mean of sum((argmax(pred) == real) m) / sum m, m = (real != 0)
    -> f32 scalar.  No epsilon, as the reference has none: a row without a label is NaN and so is the mean.  Ties: lowest index."""
    return _punc_classes_call(real, pred)[2]


def _feature_call(real, pred, upstream=None, return_grad=False):
    r, p = _as_tensor(real, np.float32), _as_tensor(pred, np.float32)
    if r.dim() != 3 or p.dim() != 3 or min(r.shape) < 1 or min(p.shape) < 1:
        raise ValueError("real and pred are [B, T, F], not empty (got shapes %s, %s)" % (tuple(r.shape), tuple(p.shape)))
    if r.shape[0] != p.shape[0] or r.shape[2] != p.shape[2]:
        raise ValueError("real %s and pred %s differ in B or F" % (tuple(r.shape), tuple(p.shape)))
    dev = _device_of(p, None)
    if dev.type != "cuda":
        raise _lib.Mi355AsrError("the losses run on the GPU only (got device %s)" % dev)
    lib = _lib.lib()
    r, p = _rows3(r, dev), _rows3(p, dev)
    B, T1, F = r.shape
    T2 = p.shape[1]
    g = _upstream(upstream, B, dev)
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    grad = torch.empty((B, T2, F), dtype=torch.float32, device=dev) if return_grad else None
    launch_feature_mse(lib, r, p, g, B, T1, T2, F, out, grad, dev)
    return out, grad


def launch_feature_mse(lib, r, p, g, B, T1, T2, F, out, grad, dev):
    """The C call on buffers the caller owns (the tests hand in poisoned outputs, misaligned and strided views)."""
    nbytes = ctypes.c_size_t()
    _lib.check(lib.mi355asr_masked_feature_mse_workspace_bytes(B, T1, T2, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mi355asr_masked_feature_mse(_p(r), r.stride(0), r.stride(1), _p(p), p.stride(0), p.stride(1), _p(g), B, T1, T2, F,
                                                   _p(out), _p(grad), grad.stride(0) if grad is not None else 0,
                                                   grad.stride(1) if grad is not None else 0, _p(ws), nbytes.value, st))


def bert_feature_loss(real, pred, return_grad=False, upstream=None):
    """PuncTrainer.bert_feature_loss (punc_trainer.py:93-102): real f32 [B, T1, F] (the BERT teacher's features, -10 where the
    dataloader padded), pred f32 [B, T2, F] (`Punc.heads`' feature); T = min(T1, T2), k = (real != -10) per element:
        out[b] = mean over t < T of sum_f (real - pred)^2 k / (sum_f k + 1e-6)     -> f32 [B] (the reference keeps a trailing 1)
    Padded tokens count in the mean with 0, as in the reference.  return_grad: also d (sum_b upstream[b] out[b]) / d pred, f32
    [B, T2, F] (upstream f32 [B], None = ones), zero for t >= T and where real == -10.  Strided views are read in place."""
    out, grad = _feature_call(real, pred, upstream, return_grad)
    return (out, grad) if return_grad else out


def punc_losses(tar_bd, feature, bd_pred, out_feature, return_grad=False, global_batch_size=None):
    """What PuncTrainer._train_step forms from the model's two outputs (punc_trainer.py:58-65) -> dict of device tensors:
    bd_loss [B], feature_map_loss [B], bd_acc (scalar) and train_loss = sum(10 feature_map_loss + bd_loss) / global_batch_size
    (tf.nn.compute_average_loss; global_batch_size defaults to B).  return_grad: also grad_bd_pred and grad_out_feature, the
    gradients of train_loss with respect to the two outputs; their upstream coefficients 1 / gbs and 10 / gbs are formed on the
    device."""
    B = int(bd_pred.shape[0])
    gbs = float(B if global_batch_size is None else global_batch_size)
    if not gbs > 0:
        raise ValueError("global_batch_size must be positive (got %r)" % (global_batch_size,))
    up_bd = up_f = None
    if return_grad:
        dev = _device_of(bd_pred, None)
        up_bd = torch.full((B,), 1.0 / gbs, dtype=torch.float32, device=dev)
        up_f = torch.full((B,), 10.0 / gbs, dtype=torch.float32, device=dev)
    bd_loss, _, bd_acc, g_bd = _punc_classes_call(tar_bd, bd_pred, up_bd, return_grad)
    f_loss, g_f = _feature_call(feature, out_feature, up_f, return_grad)
    out = {"bd_loss": bd_loss, "feature_map_loss": f_loss, "bd_acc": bd_acc,
           "train_loss": ((10.0 * f_loss.to(torch.float64) + bd_loss.to(torch.float64)).sum() / gbs).to(torch.float32)}
    if return_grad:
        out["grad_bd_pred"], out["grad_out_feature"] = g_bd, g_f
    return out
