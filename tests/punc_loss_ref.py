"""TEST INFRASTRUCTURE ONLY.  Float64 NumPy restatement of the punctuation trainer's losses (punc_recover/trainer/punc_trainer.py
classes_loss, classes_acc, bert_feature_loss, lines 93-126) with their gradients in closed form, of what _train_step makes of them,
and of the model's two training outputs (`heads64`, from the pieces of tests/punc_numpy.py: PuncTransformer.call with
training=False returns the logits before the softmax and to_bert's output, punc_transformer.py:285-295).
tests/test_punc_loss_host.py pins it against the reference's own functions run on the stand-in (tests/golden/punc_loss_ref.npz)
and against central differences; the GPU tests compare the kernels with it.  The torch functions are the same arithmetic in
torch ops, in whatever dtype and on whatever device their operands have: the float32 yardstick of the accuracy line and the
composition tools/time_punc_loss.py times."""
import numpy as np

from punc_numpy import _dense, _encoder_layer
from stft_loss_ref import _uniform

MASK_VALUE = -10.0


# ---- seeded inputs: closed formulas of the element index ---------------------------------------------------------------------------
def seeded_logits(shape, seed, scale=6.0):
    """float32 logits of `shape`"""
    return (scale * _uniform(int(np.prod(shape)), 3 * seed)).astype(np.float32).reshape(shape)


def seeded_labels(shape, classes, seed, lengths=None):
    """int32 [B, Q] classes in [0, classes) -- about a quarter 0 (padding inside the row) and a quarter 1 (no mark) when there are
    classes to spare -- and 0 from lengths[b] on"""
    B, Q = shape
    u = _uniform(B * Q, 3 * seed + 1) + 0.5
    y = np.minimum((u * (classes + 2)).astype(np.int64) - 2, classes - 1)
    y = np.where(y < 0, y + 2, y).astype(np.int32).reshape(B, Q) % classes
    if lengths is not None:
        y[np.arange(Q)[None, :] >= np.asarray(lengths)[:, None]] = 0
    return y


def seeded_features(shape_real, shape_pred, seed, lengths=None, scatter=0.04):
    """(real, pred) float32 [B, T1, F], [B, T2, F]: pred a scaled noisy copy of real on the tokens both have; real is -10 on single
    scattered elements (a share `scatter`) and on the whole rows from lengths[b] on"""
    B, T1, F = shape_real
    T2 = shape_pred[1]
    T = max(T1, T2)
    base = 2.0 * _uniform(B * T * F, 3 * seed).reshape(B, T, F)
    noise = _uniform(B * T * F, 3 * seed + 1).reshape(B, T, F)
    hole = _uniform(B * T * F, 3 * seed + 2).reshape(B, T, F) + 0.5 < scatter
    real = np.where(hole, MASK_VALUE, base)[:, :T1].astype(np.float32)
    pred = (0.8 * base + 0.3 * noise)[:, :T2].astype(np.float32)
    if lengths is not None:
        real[np.arange(T1)[None, :] >= np.asarray(lengths)[:, None]] = MASK_VALUE
    return np.ascontiguousarray(real), np.ascontiguousarray(pred)


def seeded_ids(lengths, T, vocab, seed):
    """int32 [B, T] token ids in [1, vocab), 0 from lengths[b] on"""
    B = len(lengths)
    ids = 1 + ((_uniform(B * T, 3 * seed + 2) + 0.5) * (vocab - 1)).astype(np.int64).reshape(B, T) % (vocab - 1)
    ids[np.arange(T)[None, :] >= np.asarray(lengths)[:, None]] = 0
    return ids.astype(np.int32)


# ---- the losses, float64 ----------------------------------------------------------------------------------------------------------
def _xent_parts(real, pred):
    y = np.asarray(real).astype(np.int64)
    x = np.asarray(pred, np.float64)
    Q = min(x.shape[1], y.shape[1])
    y, x = y[:, :Q], x[:, :Q]
    C = x.shape[-1]
    ok = (y >= 0) & (y < C)
    mx = x.max(-1, keepdims=True)
    e = np.exp(x - mx)
    s = e.sum(-1, keepdims=True)
    lse = (mx + np.log(s))[..., 0]
    picked = np.take_along_axis(x, np.clip(y, 0, C - 1)[..., None], -1)[..., 0]
    xe = np.where(ok, lse - picked, np.nan)
    m = y != 0
    m1 = m & (y != 1)
    return y, x, e / s, xe, ok, m, m1


def classes_loss(real, pred):
    """-> float64 [B]: sum(xe m) / (sum m + 1e-6) + sum(xe m1) / (sum m1 + 1e-6); a masked token contributes an exact 0"""
    _, _, _, xe, _, m, m1 = _xent_parts(real, pred)
    return np.where(m, xe, 0.0).sum(-1) / (m.sum(-1) + 1e-6) + np.where(m1, xe, 0.0).sum(-1) / (m1.sum(-1) + 1e-6)


def classes_acc(real, pred):
    """-> (float64 [B], their mean): sum((argmax == label) m) / sum m, no epsilon (0 / 0 = NaN), ties to the lowest index"""
    y, x, _, _, _, m, _ = _xent_parts(real, pred)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = ((x.argmax(-1) == y) & m).sum(-1) / m.sum(-1).astype(np.float64)
    return acc, acc.mean()


def classes_grad(real, pred, upstream=None):
    """d (sum_b upstream[b] loss[b]) / d pred -> float64 with the shape of pred; zero rows for t >= Q', label 0, label out of range"""
    y, x, p, _, ok, m, m1 = _xent_parts(real, pred)
    B, Q, C = x.shape
    up = np.ones(B) if upstream is None else np.asarray(upstream, np.float64).reshape(B)
    w = up[:, None] * (m / (m.sum(-1, keepdims=True) + 1e-6) + m1 / (m1.sum(-1, keepdims=True) + 1e-6)) * ok
    onehot = np.arange(C)[None, None, :] == y[..., None]
    g = np.zeros(np.asarray(pred).shape, np.float64)
    g[:, :Q] = w[..., None] * (p - onehot)
    return g


def feature_loss(real, pred):
    """-> float64 [B]: the mean over t < min(T1, T2) of sum_f (real - pred)^2 k / (sum_f k + 1e-6), k = (real != -10) on the float32
    value"""
    r32 = np.asarray(real, np.float32)
    T = min(r32.shape[1], np.asarray(pred).shape[1])
    k = r32[:, :T] != np.float32(MASK_VALUE)
    d = np.asarray(real, np.float64)[:, :T] - np.asarray(pred, np.float64)[:, :T]
    return (np.where(k, d * d, 0.0).sum(-1) / (k.sum(-1) + 1e-6)).mean(-1)


def feature_grad(real, pred, upstream=None):
    """d (sum_b upstream[b] out[b]) / d pred -> float64 with the shape of pred"""
    r32 = np.asarray(real, np.float32)
    p = np.asarray(pred, np.float64)
    B, T2, F = p.shape
    T = min(r32.shape[1], T2)
    up = np.ones(B) if upstream is None else np.asarray(upstream, np.float64).reshape(B)
    k = r32[:, :T] != np.float32(MASK_VALUE)
    d = p[:, :T] - np.asarray(real, np.float64)[:, :T]
    g = np.zeros(p.shape, np.float64)
    g[:, :T] = up[:, None, None] * 2.0 * np.where(k, d, 0.0) / ((k.sum(-1, keepdims=True) + 1e-6) * T)
    return g


def punc_losses(tar_bd, feature, bd_pred, out_feature, global_batch_size=None):
    """PuncTrainer._train_step's values and the gradients of train_loss with respect to the two outputs, float64"""
    B = np.asarray(bd_pred).shape[0]
    gbs = float(B if global_batch_size is None else global_batch_size)
    bd, fm = classes_loss(tar_bd, bd_pred), feature_loss(feature, out_feature)
    return {"bd_loss": bd, "feature_map_loss": fm, "bd_acc": classes_acc(tar_bd, bd_pred)[1],
            "train_loss": (10.0 * fm + bd).sum() / gbs,
            "grad_bd_pred": classes_grad(tar_bd, bd_pred, np.full(B, 1.0 / gbs)),
            "grad_out_feature": feature_grad(feature, out_feature, np.full(B, 10.0 / gbs))}


# ---- the model's training outputs ---------------------------------------------------------------------------------------------------
def heads64(weights, ids, num_layers=3, dtype=np.float64):
    """ids [T] of one sentence (no padding) -> (logits [T, classes], feature [T, 768]) in `dtype`: punc_numpy.punc_probs up to the
    softmax, with to_bert's output kept"""
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items()}
    ids = np.asarray(ids).reshape(-1)
    T = len(ids)
    d = w["embedding"].shape[1]
    mask_add = (ids == 0).astype(dtype) * dtype(-1e9)
    x = w["embedding"][ids] * np.sqrt(dtype(d)) + w["pos_encoding"][:T]
    x = _dense(w, "encoder/dense", x)
    x = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    for i in range(num_layers):
        plus = x
        x = _encoder_layer(w, "encoder/layer_%d" % i, x, mask_add)
        k = w["encoder/conv_%d/kernel" % i]
        xp = np.concatenate([np.zeros((2, d), dtype), x], 0)
        x = sum(xp[tap:tap + T] @ k[tap] for tap in range(3)) + w["encoder/conv_%d/bias" % i]
        x = np.maximum(x, 0) + plus
    feature = _dense(w, "to_bert", x)
    x = _dense(w, "to_hidden", feature)
    for i in range(max(num_layers - 1, 1)):
        x = _encoder_layer(w, "map/layer_%d" % i, x, mask_add)
    return _dense(w, "final", x), feature


# ---- the same arithmetic in torch ops ------------------------------------------------------------------------------------------------
def torch_classes(real, pred, upstream=None):
    """-> (loss [B], acc [B]) as torch tensors of pred's dtype on pred's device; differentiable in pred"""
    import torch
    Q = min(pred.shape[1], real.shape[1])
    y, x = real[:, :Q].long(), pred[:, :Q]
    xe = torch.logsumexp(x, -1) - x.gather(-1, y.clamp(0, x.shape[-1] - 1)[..., None])[..., 0]
    m = (y != 0).to(x.dtype)
    m1 = m * (y != 1).to(x.dtype)
    loss = (xe * m).sum(-1) / (m.sum(-1) + 1e-6) + (xe * m1).sum(-1) / (m1.sum(-1) + 1e-6)
    acc = ((x.argmax(-1) == y).to(x.dtype) * m).sum(-1) / m.sum(-1)
    return loss, acc


def torch_feature(real, pred):
    """-> out [B] as a torch tensor of pred's dtype; differentiable in pred"""
    T = min(real.shape[1], pred.shape[1])
    r, p = real[:, :T], pred[:, :T]
    k = (r != MASK_VALUE).to(p.dtype)
    return (((r - p) ** 2 * k).sum(-1) / (k.sum(-1) + 1e-6)).mean(-1)
