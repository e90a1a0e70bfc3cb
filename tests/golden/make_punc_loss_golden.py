"""Records tests/golden/punc_loss_ref.npz: the reference's own PuncTrainer.classes_loss, bert_feature_loss and classes_acc
(punc_recover/trainer/punc_trainer.py:93-126) run on the NumPy stand-in oracle/_tfshim, in float64 (tf.set_wide) and in float32.

Importing the trainer module pulls in the whole training stack, so the three methods are cut out of the file by name (ast) and
executed UNMODIFIED in a namespace that holds the stand-in as `tf`.  The stand-in lacks what they call; it is supplied here, in
this process only (oracle/ is not touched):
  tf.keras.losses.sparse_categorical_crossentropy(y, logits, True)   logsumexp(logits) - logits[y], over the stand-in's arithmetic
  tf.keras.metrics.sparse_categorical_accuracy(y, logits)            float32(argmax(logits) == y)
  tf.cast(x, 1.)    bert_feature_loss names its dtype by the enum value 1 (DT_FLOAT), which TensorFlow's as_dtype accepts

Inputs are closed formulas of the element index (tests/punc_loss_ref.py seeded_*), so the fixture stores results and the inputs'
float64 sums, not the arrays:
  case k of CASES: labels [B, T], logits [B, T, C], BERT features [B, T1, 768], predicted features [B, T2, 768] (TensorFlow's
    sparse cross-entropy wants labels and logits of one width; the feature loss cuts to min(T1, T2) itself)
    -> bd64_k / bd32_k [B], acc64_k / acc32_k, fm64_k / fm32_k [B], sum_logits_k, sum_labels_k, sum_real_k, sum_pred_k
  tester: ids [3, 33] of lengths 17, 9, 33 through tests/punc_loss_ref.py heads64 on the committed punc.onnx weights (rows past
    a length zero, as the kernel writes them), seeded labels and BERT features with -10 past each length
    -> tester_bd64 / 32 [B], tester_acc64 / 32, tester_fm64 / 32 [B], sum_ids, sum_tester_logits, sum_tester_feature
The generator asserts that in float64 every token's two largest logits differ by at least 1e-3 (min_gap records the smallest), so
accuracy and arg-max checks excuse no token.

    python tests/golden/make_punc_loss_golden.py /path/to/TensorflowASR
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_tfshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

# (B, T, C or None for the shipped class count, T1, T2, lengths or None, seed)
CASES = [(3, 20, 5, 22, 20, None, 1), (4, 33, None, 33, 40, [33, 12, 1, 20], 2)]
TESTER_LENGTHS = [17, 9, 33]
TESTER_SEED = 5
GAP = 1e-3


def reference_functions(ref_root, tf):
    path = os.path.join(ref_root, "punc_recover", "trainer", "punc_trainer.py")
    src = open(path).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "PuncTrainer")
    ns = {"tf": tf}
    for fn in cls.body:
        if isinstance(fn, ast.FunctionDef) and fn.name in ("bert_feature_loss", "classes_loss", "classes_acc"):
            exec(textwrap.dedent(ast.get_source_segment(src, fn, padded=True)), ns)
    return ns["classes_loss"], ns["bert_feature_loss"], ns["classes_acc"]


def supply_primitives(tf):
    def sparse_categorical_crossentropy(y_true, y_pred, from_logits=False):
        assert from_logits
        mx = tf.reduce_max(y_pred, -1, True)
        lse = tf.math.log(tf.reduce_sum(tf.exp(y_pred - mx), -1)) + tf.squeeze(mx, -1)
        classes = tf.reshape(tf.range(int(y_pred.shape[-1])), [1, 1, -1])
        onehot = tf.cast(tf.equal(classes, tf.expand_dims(tf.cast(y_true, tf.int32), -1)), y_pred.dtype)
        return lse - tf.reduce_sum(y_pred * onehot, -1)

    def sparse_categorical_accuracy(y_true, y_pred):
        return tf.cast(tf.equal(tf.cast(tf.argmax(y_pred, -1), tf.int32), tf.cast(y_true, tf.int32)), tf.float32)

    plain_cast = tf.cast

    def cast(x, dtype, name=None):
        return plain_cast(x, tf.float32 if isinstance(dtype, float) and dtype == 1.0 else dtype, name)
    tf.cast = cast
    tf.keras.losses = types.SimpleNamespace(sparse_categorical_crossentropy=sparse_categorical_crossentropy)
    tf.keras.metrics = types.SimpleNamespace(sparse_categorical_accuracy=sparse_categorical_accuracy)


def min_gap(logits, used):
    top = np.sort(np.asarray(logits, np.float64), -1)
    return float((top[..., -1] - top[..., -2])[used].min())


def main(ref_root):
    import tensorflow as tf
    import punc_loss_ref as R
    from punc_onnx_eval import onnx_path
    from test_punc_host import config
    from tensorflowasr_amd.checkpoint import read_onnx
    from tensorflowasr_amd.punc import Punc, weights_from_onnx_inits

    supply_primitives(tf)
    classes_loss, bert_feature_loss, classes_acc = reference_functions(ref_root, tf)
    punc = Punc(config(), device="cpu")
    shipped = punc.cfg["classes"]

    def run(labels, logits, real, pred, tag, out, key):
        for wide, w in ((True, "64"), (False, "32")):
            tf.set_wide(wide)
            y, x = tf.constant(labels, dtype=tf.int32), tf.constant(logits, dtype=tf.float32)
            r, p = tf.constant(real, dtype=tf.float32), tf.constant(pred, dtype=tf.float32)
            out["%sbd%s%s" % (tag, w, key)] = np.asarray(classes_loss(None, y, x).numpy(), np.float64).reshape(-1)
            out["%sacc%s%s" % (tag, w, key)] = np.asarray(classes_acc(None, y, x).numpy(), np.float64)
            out["%sfm%s%s" % (tag, w, key)] = np.asarray(bert_feature_loss(None, r, p).numpy(), np.float64).reshape(-1)
        tf.set_wide(False)

    out = {"classes": np.int64(shipped), "cases": np.array([[b, t, c or shipped, t1, t2, s] for b, t, c, t1, t2, _, s in CASES]),
           "tester_lengths": np.array(TESTER_LENGTHS), "tester_seed": np.int64(TESTER_SEED)}
    gaps = []
    for k, (B, T, C, T1, T2, lengths, seed) in enumerate(CASES):
        C = C or shipped
        out["lengths_%d" % k] = np.array(lengths if lengths is not None else [T] * B)
        logits = R.seeded_logits((B, T, C), seed)
        labels = R.seeded_labels((B, T), C, seed, lengths)
        real, pred = R.seeded_features((B, T1, 768), (B, T2, 768), seed, lengths)
        gaps.append(min_gap(logits, np.ones((B, T), bool)))
        run(labels, logits, real, pred, "", out, "_%d" % k)
        for name, a in (("logits", logits), ("labels", labels), ("real", real), ("pred", pred)):
            out["sum_%s_%d" % (name, k)] = np.sum(a, dtype=np.float64)
        print("case", k, out["bd64_%d" % k], out["acc64_%d" % k], out["fm64_%d" % k])

    _, inits = read_onnx(onnx_path())
    weights = weights_from_onnx_inits(inits, punc.cfg["num_layers"])
    weights["pos_encoding"] = punc.pos_encode_inputs[0]
    B, T = len(TESTER_LENGTHS), max(TESTER_LENGTHS)
    ids = R.seeded_ids(TESTER_LENGTHS, T, punc.cfg["vocab"], TESTER_SEED)
    logits, feature = np.zeros((B, T, shipped)), np.zeros((B, T, 768))
    for b, n in enumerate(TESTER_LENGTHS):
        logits[b, :n], feature[b, :n] = R.heads64(weights, ids[b, :n], punc.cfg["num_layers"])
    labels = R.seeded_labels((B, T), shipped, TESTER_SEED, TESTER_LENGTHS)
    real, _ = R.seeded_features((B, T, 768), (B, T, 768), TESTER_SEED, TESTER_LENGTHS)
    gaps.append(min_gap(logits, np.arange(T)[None, :] < np.array(TESTER_LENGTHS)[:, None]))
    run(labels, logits.astype(np.float32), real, feature.astype(np.float32), "tester_", out, "")
    out["sum_ids"] = np.sum(ids, dtype=np.float64)
    out["sum_tester_logits"], out["sum_tester_feature"] = logits.sum(), feature.sum()
    print("tester", out["tester_bd64"], out["tester_acc64"], out["tester_fm64"])
    out["min_gap"] = np.float64(min(gaps))
    assert out["min_gap"] >= GAP, "two largest logits of a token within %g: %s -- choose other seeds" % (GAP, gaps)
    path = os.path.join(HERE, "punc_loss_ref.npz")
    np.savez_compressed(path, **out)
    print("min gap %.3e; wrote punc_loss_ref.npz: %d bytes" % (out["min_gap"], os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
