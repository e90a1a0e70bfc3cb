"""Records tests/golden/stft_loss_ref.npz: the reference's own vad/utils/stft.py (TFMultiResolutionSTFT with its default
resolutions) run unmodified on the NumPy stand-in oracle/_tfshim, in float64 (tf.set_wide) and in float32, on the two seeded
input pairs of tests/stft_loss_ref.py seeded_pair: [2, 30, 80] and [4, 60, 80] (the shipped config's batch size).  The inputs
are a closed formula of the element index, so the fixture stores their float64 sums and not the arrays.

The stand-in lacks two primitives the file calls; they are supplied here, in this process only (oracle/ is not touched):
  tf.norm(x, ord="fro", axis=(-2, -1))   the Frobenius norm over the two axes
  tf.keras.losses.mse                    the stand-in's existing tf.losses.mse (the mean over the last axis)
Per input k: loss64_k / loss32_k (the value call() returns), sc64_k / mag64_k / sc32_k / mag32_k [R] (the batch means of what
each TFSTFT.call returns), sum_true_k / sum_pred_k.

VADTrainer.mask_loss cannot be run as written: the stand-in has no tf.losses.binary_crossentropy and importing
vad/trainer/vad_trainer.py pulls in the whole training stack.  Its five lines are restated below over the stand-in's own tensor
arithmetic with Keras' from_logits formula max(x, 0) - x z + log(1 + exp(-|x|)); mask_one / mask_zero / mask_acc hold the result
on the seeded [2, 30, 1] labels and logits of seeded_mask, float64.

    python tests/golden/make_stft_loss_golden.py /path/to/TensorflowASR
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_tfshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(2, 30, 80), (4, 60, 80)]


def main(ref_root):
    import tensorflow as tf
    from stft_loss_ref import seeded_mask, seeded_pair

    def norm(x, ord="fro", axis=None):
        assert ord == "fro" and tuple(axis) == (-2, -1)
        return tf.sqrt(tf.reduce_sum(tf.square(x), axis=[-2, -1]))
    tf.norm = norm
    tf.keras.losses = types.SimpleNamespace(mse=tf.losses.mse)
    spec = importlib.util.spec_from_file_location("ref_vad_stft", os.path.join(ref_root, "vad", "utils", "stft.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    out = {"shapes": np.array(SHAPES)}
    for k, shape in enumerate(SHAPES):
        y, x = seeded_pair(shape, seed=k)
        out["sum_true_%d" % k], out["sum_pred_%d" % k] = np.sum(y, dtype=np.float64), np.sum(x, dtype=np.float64)
        for wide, tag in ((True, "64"), (False, "32")):
            tf.set_wide(wide)
            m = mod.TFMultiResolutionSTFT(shape[0])
            ty, tx = tf.constant(y, dtype=tf.float32), tf.constant(x, dtype=tf.float32)
            out["loss%s_%d" % (tag, k)] = np.asarray(m.call(ty, tx).numpy(), np.float64)
            ry, rx = tf.reshape(ty, [shape[0], -1]), tf.reshape(tx, [shape[0], -1])
            parts = [f.call([ry, rx]) for f in m.stft_losses]
            out["sc%s_%d" % (tag, k)] = np.array([float(tf.reduce_mean(s).numpy()) for s, _ in parts])
            out["mag%s_%d" % (tag, k)] = np.array([float(tf.reduce_mean(g).numpy()) for _, g in parts])
            print(shape, tag, repr(float(out["loss%s_%d" % (tag, k)])))

    # VADTrainer.mask_loss and tf.metrics.binary_accuracy, restated line for line on the stand-in's tensors
    tf.set_wide(True)
    z, lg = seeded_mask((2, 30, 1), seed=7)
    y, pred = tf.constant(z, dtype=tf.float32), tf.constant(lg, dtype=tf.float32)
    loss = tf.reduce_mean(tf.maximum(pred, 0.) - pred * y + tf.math.log(1. + tf.exp(-tf.abs(pred))), axis=-1)
    one = tf.squeeze(y, -1)
    zero = tf.where(one == 0., 1., 0.)
    one_loss = tf.reduce_sum(loss * one) / (tf.reduce_sum(one) + 1e-6)
    zero_loss = tf.reduce_sum(loss * zero) / (tf.reduce_sum(zero) + 1e-6)
    acc = tf.reduce_mean(tf.cast(tf.equal(y, tf.cast(pred > 0.5, y.dtype)), tf.float32))
    out["mask_one"], out["mask_zero"], out["mask_acc"] = (np.asarray(v.numpy(), np.float64) for v in (one_loss, zero_loss, acc))
    tf.set_wide(False)
    path = os.path.join(HERE, "stft_loss_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote stft_loss_ref.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
