"""Float64 NumPy restatement of the Translator-head losses and the evaluation metrics of the reference's trainer
(asr/trainer/ctc_runners.py:48-76, 144): sparse_categorical_crossentropy(from_logits=True), mask_loss, translate_acc, ctc_acc --
the yardstick of tensorflowasr_amd/losses.py.  Every function takes the first min(T, Q) columns of its two operands."""
import numpy as np

ULP = 2.0 ** -24


def _cut(labels, other):
    labels, other = np.asarray(labels), np.asarray(other)
    q = min(labels.shape[1], other.shape[1])
    return labels[:, :q].astype(np.int64), other[:, :q]


def sparse_xent(logits, labels):
    """loss [B, Q'] = logsumexp(x) - x[y] in float64; a label outside [0, V) gives NaN"""
    y, x = _cut(labels, np.asarray(logits, np.float64))
    V = x.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(-1)
        lse = np.log(np.exp(x - m[..., None]).sum(-1)) + m
        ok = (y >= 0) & (y < V)
        xy = np.take_along_axis(x, np.clip(y, 0, V - 1)[..., None], -1)[..., 0]
        return np.where(ok, (lse - m) + (m - xy), np.nan)


def softmax(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def xent_grad(logits, labels, weights=None):
    """w * (softmax(x) - onehot(y)) [B, Q', V]; a label outside [0, V) gives a zero row"""
    y, x = _cut(labels, np.asarray(logits, np.float64))
    V = x.shape[-1]
    g = softmax(x)
    ok = (y >= 0) & (y < V)
    b, t = np.nonzero(ok)
    g[b, t, y[b, t]] -= 1.0
    g[~ok] = 0.0
    if weights is not None:
        g = g * np.asarray(weights, np.float64)[:, :g.shape[1], None]
    return g


def mask_loss(labels, logits):
    """ctc_runners.py:69-76 -> [B]"""
    y, _ = _cut(labels, np.asarray(logits)[:, :, 0])
    loss = sparse_xent(logits, labels)
    need, zero = (y != 0).astype(np.float64), (y == 0).astype(np.float64)
    need_loss = (loss * need).sum() / (need.sum() + 1e-6)
    zero_loss = (loss * zero).sum() / (zero.sum() + 1e-6)
    return loss.mean(-1) + need_loss + zero_loss


def mask_loss_weights(labels, width, upstream=None):
    """d (sum_b g_b mask_loss_b) / d loss[b, t] = g_b / Q' + G need / (N_need + 1e-6) + G zero / (N_zero + 1e-6) -> [B, Q']"""
    y = np.asarray(labels)[:, :width]
    B, Q = y.shape
    g = np.ones(B) if upstream is None else np.asarray(upstream, np.float64)
    need, zero = (y != 0).astype(np.float64), (y == 0).astype(np.float64)
    return g[:, None] / Q + g.sum() * need / (need.sum() + 1e-6) + g.sum() * zero / (zero.sum() + 1e-6)


def argmax(logits):
    """tf.argmax: the lowest index among equal maxima"""
    return np.argmax(np.asarray(logits), -1)


def translate_acc(labels, logits):
    """ctc_runners.py:63-68 -> scalar"""
    y, pred = _cut(labels, argmax(logits))
    need = (y != 0).astype(np.float64)
    return ((y == pred) * need).sum() / (need.sum() + 1e-6)


def ctc_acc(labels, decoded, pad=0):
    """ctc_runners.py:48-62 -> [B]"""
    y, d = _cut(labels, np.asarray(decoded))
    mask = (y != pad).astype(np.float64)
    return ((y == d) * mask).sum(-1) / (mask.sum(-1) + 1e-6)


def loss_bound(c, logits, labels, loss):
    """c * 2^-24 * (1 + |max x| + |x_y| + |loss|) per element of loss [B, Q'], non-finite terms left out"""
    y, x = _cut(labels, np.asarray(logits, np.float64))
    V = x.shape[-1]
    xy = np.take_along_axis(x, np.clip(y, 0, V - 1)[..., None], -1)[..., 0]
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
    return c * ULP * (1.0 + fin(x.max(-1)) + fin(xy) + fin(loss))
