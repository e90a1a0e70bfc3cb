"""Checks of the fixtures against the reference's own Python: they execute code that lives only in the reference checkout, so
they are not part of the test suite (which runs on the repository alone).  Run them after changing a recipe, the stand-in
(oracle/_tfshim) or the Keras-name map, on a machine with the reference checkout:

    REFERENCE_ROOT=/path/to/TensorflowASR python tests/golden/check_recipes.py [check ...]

  ctc_decoder_class   the reference's `CTCDecoder` CLASS (asr/models/conformer_blocks.py:385-438, imported unmodified),
                      executed on the stand-in with the weights of the exported ctc_model.onnx (rebuilt by helpers.ctc_model_onnx),
                      reproduces what the ONNX graph itself computes (tests/golden/ctc_decoder_io.npz) within 1e-4 with
                      identical argmax; building the encoder (13 blocks) and then the CTC decoder the way test_asr.py:26-75
                      does gives the decoder's layers the numbers the exported graph carries (Keras auto-naming)
  tf_fixtures         the committed tests/golden/tf_*.npz are what make_tf_goldens.py produces today (integers and strings
                      exactly, floats to 2e-6 / 1e-12 relative for the float32 / float64 runs)
  config2_b64         the committed tf_config2_b64.npz against a fresh run of make_tf_config2_b64.py on utterances 0 and 63

Every check raises on a mismatch; the script prints one line per check that passed."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REFERENCE_ROOT", "")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import GOLDEN, ctc_model_onnx, golden_ctc_io, golden_ctc_weights, maxdiff  # noqa: E402


def check_ctc_decoder_class():
    sys.path[:0] = [os.path.join(ROOT, "oracle", "_tfshim"), REF]
    import tensorflow as tf
    from tensorflow.keras import _impl
    from asr.models import conformer_blocks as cb
    from tensorflowasr_amd import checkpoint
    assert "standin" in tf.__version__
    tf.set_wide(True)
    _impl.reset_uids()
    # test_asr.py:26-75: encoder first, then the CTC decoder -- the layer numbering of the export depends on it
    enc = cb.ConformerEncoder(dmodel=144, reduction_factor=4, num_blocks=13, head_size=36, num_heads=4, kernel_size=32, fc_factor=0.5,
                              dropout=0.0, add_wav_info=False, sample_rate=16000, n_mels=80, mel_layer_type="Melspectrogram",
                              mel_layer_trainable=False, stride_ms=10)
    ctc = cb.CTCDecoder(num_classes=1332, dmodel=144, num_blocks=1, head_size=36, num_heads=4, kernel_size=32, dropout=0.0, fc_factor=0.5)
    ctc._build()
    names = [v.name for v in ctc.weights]
    # the numbers in the exported graph's scope names (`grep ReadVariableOp` over the initializers)
    with tempfile.TemporaryDirectory() as td:
        _, inits = checkpoint.read_onnx(ctc_model_onnx(td))
    auto = re.compile(r"^(dense|layer_normalization|multi_head_attention|batch_normalization|conv1d|separable_conv1d)_\d+$")
    exported = {p for k in inits for p in k.split("/") if auto.match(p)}
    mine = {p for n in names for p in n.split(":")[0].split("/")[1:-1] if auto.match(p)}
    assert len(exported) == 12 and exported == mine, (sorted(exported - mine), sorted(mine - exported))
    assert {"dense_53", "dense_54", "dense_57", "layer_normalization_65", "layer_normalization_69", "multi_head_attention_13",
            "batch_normalization_13"} <= mine
    assert len(enc.conformer_blocks) == 13
    # the trained weights of the export, through the product's own Keras-name map, into the reference's class
    w = golden_ctc_weights()
    m = checkpoint.keras_names_to_abi(names)
    assert sorted(m.values()) == sorted(w), (sorted(set(w) - set(m.values())), sorted(set(names) - set(m)))
    for v in ctc.weights:
        v.assign(np.asarray(w[m[v.name]], np.float32).reshape(v.shape))
    io = golden_ctc_io()                      # what oracle/onnx_mini.py computed from ctc_model.onnx itself (make_golden.py)
    got = ctc(tf.constant(io["x_a"]), training=False).numpy()
    assert got.shape == io["logits_a"].shape and np.abs(got - io["logits_a"]).max() < 1e-4
    assert np.array_equal(got.argmax(-1), io["logits_a"].argmax(-1))
    got = ctc(tf.constant(io["x_b"]), training=False).numpy()
    assert np.array_equal(got.argmax(-1), io["argmax_b"]) and np.abs(got.max(-1) - io["max_b"]).max() < 1e-4
    assert np.abs(got[:, ::8] - io["logits_b_every8"]).max() < 1e-4
    tf.set_wide(False)


def check_tf_fixtures():
    with tempfile.TemporaryDirectory() as out:
        r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_tf_goldens.py")], capture_output=True, text=True, timeout=1200,
                           cwd=ROOT, env=dict(os.environ, MI355ASR_TF_GOLDEN_OUT=out))
        assert r.returncode == 0, r.stderr[-3000:]
        names = sorted(f for f in os.listdir(GOLDEN) if f.startswith("tf_") and f.endswith(".npz") and f != "tf_config2_b64.npz")
        # (tf_config2_b64.npz has its own recipe, make_tf_config2_b64.py: check_config2_b64)
        assert names == sorted(os.listdir(out)) and len(names) == 11, (names, sorted(os.listdir(out)))
        for n in names:
            a, b = np.load(os.path.join(GOLDEN, n)), np.load(os.path.join(out, n))
            assert sorted(a.files) == sorted(b.files), n
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (n, k)
                if a[k].size == 0:
                    continue
                if a[k].dtype.kind == "f":        # BLAS may sum in another order on another core count: last-digit slack only
                    tol = (1e-12 if a[k].dtype == np.float64 else 2e-6) * max(1.0, float(np.abs(a[k]).max()))
                    assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= tol, (n, k)
                else:
                    assert np.array_equal(a[k], b[k]), (n, k)


def check_config2_b64():
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import make_tf_config2_b64 as m; "
            "r = m.run(utterances=[0, 63]); np.savez(sys.argv[1], **r)" % GOLDEN)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "two.npz")
        r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, timeout=900, cwd=GOLDEN)
        assert r.returncode == 0, r.stderr[-3000:]
        two, fx = np.load(out), np.load(os.path.join(GOLDEN, "tf_config2_b64.npz"))
        for k in two.files:
            a, b = two[k], fx[k][[0, 63]]
            if a.dtype.kind == "f":
                assert maxdiff(a, b) <= 2e-6 * max(1.0, float(np.abs(b).max())), k
            else:
                assert np.array_equal(a, b), k


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "asr", "models")):
        raise SystemExit("set REFERENCE_ROOT to the reference checkout (the directory that holds asr/models)")
    for name in sys.argv[1:] or ["ctc_decoder_class", "tf_fixtures", "config2_b64"]:
        globals()["check_" + name]()
        print("ok:", name, flush=True)
