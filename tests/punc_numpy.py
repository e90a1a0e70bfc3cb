"""TEST INFRASTRUCTURE ONLY.  PuncTransformer.inference restated in NumPy on the ABI-named weights of include/mi355asr.h
(the names `tensorflowasr_amd.punc.Punc.load_onnx` produces), written from punc_recover/models/punc_transformer.py and
independent of the graph evaluator in punc_onnx_eval.py: equality of the two pins the name map and every transpose."""
import numpy as np


def _ln(x, g, b, eps=1e-6):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def _dense(w, p, x):
    return x @ w[p + "/kernel"] + w[p + "/bias"]


def _encoder_layer(w, p, x, mask_add, heads=8):
    T, d = x.shape
    dh = d // heads
    split = lambda a: a.reshape(T, heads, dh).transpose(1, 0, 2)
    q, k, v = (split(_dense(w, "%s/mha/%s" % (p, n), x)) for n in ("wq", "wk", "wv"))
    s = q @ k.transpose(0, 2, 1) / np.sqrt(np.asarray(dh, x.dtype)) + mask_add[None, None, :]
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    a = e / e.sum(-1, keepdims=True)
    ctx = (a @ v).transpose(1, 0, 2).reshape(T, d)
    out1 = _ln(x + _dense(w, p + "/mha/dense", ctx), w[p + "/layernorm1/gamma"], w[p + "/layernorm1/beta"])
    ffn = _dense(w, p + "/ffn/dense_2", np.maximum(_dense(w, p + "/ffn/dense_1", out1), 0))
    return _ln(out1 + ffn, w[p + "/layernorm2/gamma"], w[p + "/layernorm2/beta"])


def punc_probs(weights, ids, num_layers=3, dtype=np.float64):
    """ids [T] of one sentence -> probabilities [T, classes] in `dtype`"""
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
        k = w["encoder/conv_%d/kernel" % i]                       # [3, in, out], tap 2 on the current token
        xp = np.concatenate([np.zeros((2, d), dtype), x], 0)
        x = sum(xp[tap:tap + T] @ k[tap] for tap in range(3)) + w["encoder/conv_%d/bias" % i]
        x = np.maximum(x, 0) + plus
    x = _dense(w, "to_hidden", _dense(w, "to_bert", x))
    for i in range(max(num_layers - 1, 1)):
        x = _encoder_layer(w, "map/layer_%d" % i, x, mask_add)
    z = _dense(w, "final", x)
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)
