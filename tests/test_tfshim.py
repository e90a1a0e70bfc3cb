"""Gates on the NumPy stand-in for TensorFlow (oracle/_tfshim) that tests/golden/make_tf_goldens.py runs the reference's own
Python on.  The stand-in is test infrastructure; these tests are what entitles the tf_*.npz fixtures to be called "the
reference's output":

1. reference-held data: keras.backend.ctc_decode (greedy) against the ids the reference's own C++ `ctc_greedy_decoder.h`
   returned for the same batches (tests/golden/standin_greedy_kat.json);
2. every primitive against its torch.nn.functional twin on random data (float64, 1e-10): strided / dilated convolutions
   with TF 'SAME' padding (compared with explicitly padded torch convolutions), depthwise, separable-causal, dense,
   layer / batch / instance normalisation, Keras MultiHeadAttention with a mask (torch scaled_dot_product_attention),
   pooling, embedding, pad modes, FFTs, repeat / roll / band_part / where / dynamic_stitch, scan, while_loop.

The checks that execute the reference's own Python on the stand-in (its CTCDecoder class against the exported ONNX graph,
Keras auto-naming, the fixture recipes) need the reference checkout and live in tests/golden/check_recipes.py."""
import json
import os
import sys

import numpy as np
import pytest

from helpers import GOLDEN, ROOT

SHIM = os.path.join(ROOT, "oracle", "_tfshim")

_PURGE = ("tensorflow", "tensorflow_addons", "librosa", "asr", "leaf_audio", "utils")


@pytest.fixture(scope="module")
def tf():
    """the stand-in on sys.path for this module only; everything it brought in is forgotten afterwards"""
    before = list(sys.path)
    sys.path[:0] = [SHIM]
    for k in [k for k in sys.modules if k.split(".")[0] in _PURGE]:
        del sys.modules[k]
    import tensorflow as tf
    assert "standin" in tf.__version__
    tf.set_wide(True)
    yield tf
    tf.set_wide(False)
    sys.path[:] = before
    for k in [k for k in sys.modules if k.split(".")[0] in _PURGE]:
        del sys.modules[k]


def _fresh_names(tf):
    from tensorflow.keras import _impl
    _impl.reset_uids()


# ---- 1: the stand-in's ctc_decode against the reference's C++ greedy decoder -----------------------------------------
def test_standin_ctc_decode_equals_the_reference_cpp_greedy_decoder(tf):
    """the ids the reference's C++ decoder returned for these batches, on log(p + 1e-7) as test_asr.py:167-185 / asr.py:41-61
    feed it (tests/golden/standin_greedy_kat.json, tests/golden/make_golden.py standin_greedy_kat)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    make_golden = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_golden)
    with open(os.path.join(GOLDEN, "standin_greedy_kat.json")) as f:
        kat = json.load(f)
    cases = list(make_golden.standin_greedy_batches())
    assert sorted(kat) == sorted("%d,%d" % (T, V) for T, V, _, _ in cases)
    for T, V, lens, p in cases:
        dense = tf.keras.backend.ctc_decode(tf.constant(p), lens)[0][0].numpy()
        for b in range(p.shape[0]):
            assert [int(t) for t in dense[b] if t >= 0] == kat["%d,%d" % (T, V)][b], (T, V, b)


# ---- 2: primitives against torch ------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _same(n, k, s, d=1):
    out = -(-n // s)
    tot = max((out - 1) * s + (k - 1) * d + 1 - n, 0)
    return tot // 2, tot - tot // 2


@pytest.mark.parametrize("H,W,kh,kw,sh,sw,padding", [(50, 80, 3, 3, 2, 2, "SAME"), (25, 13, 3, 3, 2, 2, "SAME"), (21, 84, 3, 3, 2, 2, "VALID"),
                                                       (1000, 1, 64, 1, 16, 1, "SAME"), (37, 5, 4, 2, 3, 1, "SAME"), (9, 9, 3, 3, 1, 1, "VALID")])
def test_conv2d_against_torch(tf, H, W, kh, kw, sh, sw, padding):
    import torch.nn.functional as F
    rng = np.random.default_rng(H * W)
    x, w = rng.standard_normal((2, H, W, 3)), rng.standard_normal((kh, kw, 3, 5))
    got = tf.nn.conv2d(tf.constant(x), tf.constant(w), strides=(sh, sw), padding=padding).numpy()
    xt = _t(x).permute(0, 3, 1, 2)
    if padding == "SAME":
        (pt, pb), (pl, pr) = _same(H, kh, sh), _same(W, kw, sw)
        xt = F.pad(xt, (pl, pr, pt, pb))
    ref = F.conv2d(xt, _t(w).permute(3, 2, 0, 1), stride=(sh, sw)).permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-10
    # the Keras layer and keras.backend.conv2d are the same computation
    got2 = tf.keras.backend.conv2d(tf.constant(x), tf.constant(w), strides=(sh, sw), padding=padding.lower(), data_format="channels_last").numpy()
    assert np.array_equal(got, got2)


@pytest.mark.parametrize("T,k,s,d,padding", [(250, 32, 1, 1, "same"), (250, 5, 1, 1, "same"), (13, 5, 1, 1, "same"), (100, 32, 1, 1, "causal"),
                                             (16000, 7, 5, 1, "same"), (400, 3, 4, 1, "same"), (300, 5, 1, 2, "valid"), (64, 1, 1, 1, "same")])
def test_conv1d_and_separable_conv1d_layers_against_torch(tf, T, k, s, d, padding):
    import torch.nn.functional as F
    rng = np.random.default_rng(T + k)
    C, O = 6, 10
    x = rng.standard_normal((2, T, C))
    xt = _t(x).permute(0, 2, 1)
    if padding == "same":
        xt = F.pad(xt, _same(T, k, s, d))
    elif padding == "causal":
        xt = F.pad(xt, (d * (k - 1), 0))
    lay = tf.keras.layers.Conv1D(O, k, strides=s, padding=padding, dilation_rate=d)
    got = lay(tf.constant(x)).numpy()
    W, b = lay.kernel.numpy(), lay.bias.numpy() + 0.25
    lay.bias.assign(b)
    got = lay(tf.constant(x)).numpy()
    ref = F.conv1d(xt, _t(W).permute(2, 1, 0), _t(b), stride=s, dilation=d).permute(0, 2, 1).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-10
    if s == 1 and d == 1:
        sep = tf.keras.layers.SeparableConv1D(O, k, padding=padding, depth_multiplier=1)
        sep(tf.constant(x))
        dk, pk, sb = sep.depthwise_kernel.numpy(), sep.pointwise_kernel.numpy(), rng.standard_normal(O)
        sep.bias.assign(sb)
        got = sep(tf.constant(x)).numpy()
        y = F.conv1d(xt, _t(dk).permute(1, 2, 0), groups=C)                       # [k, C, 1] -> [C, 1, k]
        ref = F.conv1d(y, _t(pk).permute(2, 1, 0), _t(sb)).permute(0, 2, 1).numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-10


def test_depthwise_conv2d_and_conv1d_functions_against_torch(tf):
    import torch.nn.functional as F
    rng = np.random.default_rng(11)
    x, w = rng.standard_normal((2, 1, 1600, 8)), rng.standard_normal((1, 401, 8, 1))
    got = tf.nn.depthwise_conv2d(tf.constant(x), tf.constant(w), strides=(1, 160, 160, 1), padding="SAME").numpy()
    xt = F.pad(_t(x).permute(0, 3, 1, 2), _same(1600, 401, 160))
    ref = F.conv2d(xt, _t(w).permute(2, 3, 0, 1), stride=(1, 160), groups=8).permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape == (2, 1, 10, 8) and np.abs(got - ref).max() < 1e-10
    x1, w1 = rng.standard_normal((2, 3000, 1)), rng.standard_normal((401, 1, 12))
    got = tf.nn.conv1d(tf.constant(x1), tf.constant(w1), stride=1, padding="SAME").numpy()
    ref = F.conv1d(F.pad(_t(x1).permute(0, 2, 1), _same(3000, 401, 1)), _t(w1).permute(2, 1, 0)).permute(0, 2, 1).numpy()
    assert np.abs(got - ref).max() < 1e-10


def test_dense_and_normalisation_layers_against_torch(tf):
    import torch
    import torch.nn.functional as F
    import tensorflow_addons as tfa
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 17, 24))
    d = tf.keras.layers.Dense(40)
    d(tf.constant(x))
    W, b = rng.standard_normal((24, 40)), rng.standard_normal(40)
    d.kernel.assign(W), d.bias.assign(b)
    assert np.abs(d(tf.constant(x)).numpy() - F.linear(_t(x), _t(W).T, _t(b)).numpy()).max() < 1e-10
    ln = tf.keras.layers.LayerNormalization()
    ln(tf.constant(x))
    g, be = rng.standard_normal(24), rng.standard_normal(24)
    ln.gamma.assign(g), ln.beta.assign(be)
    assert ln.epsilon == 1e-3
    assert np.abs(ln(tf.constant(x)).numpy() - F.layer_norm(_t(x), (24,), _t(g), _t(be), eps=1e-3).numpy()).max() < 1e-10
    bn = tf.keras.layers.BatchNormalization()
    bn(tf.constant(x), training=False)
    mu, var = rng.standard_normal(24), rng.random(24) + 0.5
    bn.gamma.assign(g), bn.beta.assign(be), bn.moving_mean.assign(mu), bn.moving_variance.assign(var)
    ref = F.batch_norm(_t(x).permute(0, 2, 1), _t(mu), _t(var), _t(g), _t(be), training=False, eps=1e-3).permute(0, 2, 1).numpy()
    assert np.abs(bn(tf.constant(x), training=False).numpy() - ref).max() < 1e-10
    assert [v.name.rsplit("/", 1)[-1] for v in bn.weights] == ["gamma:0", "beta:0", "moving_mean:0", "moving_variance:0"]
    inn = tfa.layers.InstanceNormalization(axis=2, epsilon=1e-6)
    inn(tf.constant(x))
    inn.gamma.assign(g), inn.beta.assign(be)
    ref = F.instance_norm(_t(x).permute(0, 2, 1), weight=_t(g), bias=_t(be), eps=1e-6).permute(0, 2, 1).numpy()
    assert np.abs(inn(tf.constant(x)).numpy() - ref).max() < 1e-10
    emb = tf.keras.layers.Embedding(30, 8)
    ids = rng.integers(0, 30, (2, 9))
    emb(tf.constant(ids))
    E = rng.standard_normal((30, 8))
    emb.embeddings.assign(E)
    assert np.array_equal(emb(tf.constant(ids)).numpy(), F.embedding(_t(ids), _t(E)).numpy())
    assert np.abs(tf.keras.activations.swish(tf.constant(x)).numpy() - F.silu(_t(x)).numpy()).max() < 1e-12
    assert np.abs(tf.keras.layers.LeakyReLU()(tf.constant(x)).numpy() - F.leaky_relu(_t(x), 0.3).numpy()).max() < 1e-12
    assert np.abs(tf.nn.softmax(tf.constant(x)).numpy() - torch.softmax(_t(x), -1).numpy()).max() < 1e-12
    ap = tf.keras.layers.AveragePooling1D(pool_size=2, strides=2)(tf.constant(x)).numpy()
    assert np.abs(ap - F.avg_pool1d(_t(x).permute(0, 2, 1), 2, 2).permute(0, 2, 1).numpy()).max() < 1e-12


def test_keras_multi_head_attention_with_band_mask_against_torch(tf):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(8)
    B, T, S, D, H, K = 2, 11, 19, 24, 4, 6
    q, kv = rng.standard_normal((B, T, D)), rng.standard_normal((B, S, D))
    mask = rng.random((B, T, S)) > 0.4
    mask[:, :, 0] = True
    mha = tf.keras.layers.MultiHeadAttention(num_heads=H, key_dim=K)
    mha(tf.constant(q), tf.constant(kv))
    ws = {}
    for nm, lay in (("q", mha._query_dense), ("k", mha._key_dense), ("v", mha._value_dense), ("o", mha._output_dense)):
        ws[nm] = (rng.standard_normal(lay.kernel.shape), rng.standard_normal(lay.bias.shape))
        lay.kernel.assign(ws[nm][0]), lay.bias.assign(ws[nm][1])
    assert [v.name for v in mha.weights][:2] == ["multi_head_attention/query/kernel:0", "multi_head_attention/query/bias:0"] or \
        mha.weights[0].name.endswith("/query/kernel:0")
    got = mha(tf.constant(q), tf.constant(kv), attention_mask=tf.constant(mask)).numpy()
    Q = torch.einsum("btd,dhk->bhtk", _t(q), _t(ws["q"][0])) + _t(ws["q"][1])[None, :, None, :]
    Kt = torch.einsum("bsd,dhk->bhsk", _t(kv), _t(ws["k"][0])) + _t(ws["k"][1])[None, :, None, :]
    V = torch.einsum("bsd,dhk->bhsk", _t(kv), _t(ws["v"][0])) + _t(ws["v"][1])[None, :, None, :]
    ctx = F.scaled_dot_product_attention(Q, Kt, V, attn_mask=_t(mask)[:, None])        # scale 1/sqrt(K), -inf where masked
    ref = (torch.einsum("bhtk,hkd->btd", ctx, _t(ws["o"][0])) + _t(ws["o"][1])).numpy()
    assert np.abs(got - ref).max() < 1e-9           # -1e9 adder vs -inf: exp(-1e9) is exactly 0 in both


def test_shape_index_and_control_flow_functions(tf):
    import torch
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 10, 4))
    assert np.array_equal(tf.pad(tf.constant(x), [[0, 0], [2, 1], [0, 0]], "REFLECT").numpy(), np.pad(x, ((0, 0), (2, 1), (0, 0)), mode="reflect"))
    assert np.array_equal(tf.pad(tf.constant(x), [[0, 0], [4, 0], [0, 0]]).numpy(), np.pad(x, ((0, 0), (4, 0), (0, 0))))
    r = np.array([1, 0, 2, 1, 0, 0, 3, 1, 0, 1])
    assert np.array_equal(tf.repeat(tf.constant(x)[0], repeats=tf.constant(r), axis=0).numpy(), torch.repeat_interleave(_t(x[0]), _t(r), 0).numpy())
    assert np.array_equal(tf.roll(tf.constant(x), 3, axis=1).numpy(), torch.roll(_t(x), 3, 1).numpy())
    ones = np.ones((1, 6, 6))
    assert np.array_equal(tf.linalg.band_part(tf.constant(ones), -1, 0).numpy(), torch.tril(_t(ones)).numpy())
    assert np.array_equal(tf.linalg.band_part(tf.constant(ones), 1, 2).numpy(), (torch.triu(_t(ones), -1) * torch.tril(_t(ones), 2)).numpy())
    a, b = tf.split(tf.constant(x), 2, axis=-1)
    assert np.array_equal(a.numpy(), x[..., :2]) and np.array_equal(b.numpy(), x[..., 2:])
    assert tf.where(tf.constant(r) != 0, 1, 0).dtype == tf.int32 and tf.where(tf.constant(r) == 0., 1., 0.).dtype == tf.float32
    assert tf.argmax(tf.constant(x), -1).dtype == tf.int64
    assert np.array_equal(tf.einsum("BNI , HIO -> BNHO", tf.constant(x), tf.constant(np.ones((2, 4, 5)))).numpy(), np.einsum("bni,hio->bnho", x, np.ones((2, 4, 5))))
    st = tf.dynamic_stitch([tf.range(0, 6, delta=2), tf.range(1, 6, delta=2)], [tf.constant(x[:, :3, 0].T), tf.constant(x[:, 3:6, 0].T)]).numpy()
    assert np.array_equal(st[0::2], x[:, :3, 0].T) and np.array_equal(st[1::2], x[:, 3:6, 0].T)
    w = tf.constant(np.full(4, 0.04))
    sc = tf.scan(lambda acc, v: w * v + (1.0 - w) * acc, tf.transpose(tf.constant(x), (1, 0, 2)), initializer=tf.constant(x[:, 0])).numpy()
    acc, ref = x[:, 0], []
    for t in range(10):
        acc = 0.04 * x[:, t] + 0.96 * acc
        ref.append(acc)
    assert np.abs(sc - np.stack(ref)).max() < 1e-12
    i, tot = tf.while_loop(lambda i, s: tf.less(i, 5), lambda i, s: [i + 1, s + tf.cast(i, tf.float32)], [tf.constant(0), tf.constant(0.0)])
    assert int(i) == 5 and float(tot) == 10.0
    s = tf.constant(x).shape
    assert s.as_list() == [3, 10, 4] and s.ndims == 3 and s[:-1] + (7,) == (3, 10, 7) and tf.shape(tf.constant(x))[1].numpy() == 10
    xs = rng.standard_normal((2, 3, 50))
    assert np.abs(tf.signal.rfft(tf.constant(xs), fft_length=[64]).numpy() - torch.fft.rfft(_t(xs), n=64).numpy()).max() < 1e-12
    f = np.fft.rfft(xs, 64)
    assert np.abs(tf.signal.irfft(tf.constant(f)).numpy() - torch.fft.irfft(_t(f)).numpy()).max() < 1e-12


def test_keras_bookkeeping_names_trainable_lists_and_object_graph(tf):
    _fresh_names(tf)
    from tensorflow.keras._impl import to_snake_case

    assert [to_snake_case(n) for n in ("CTCDecoder", "TFResidualStack", "SeparableConv1D", "LeakyReLU", "MultiHeadAttention", "Conv2D",
                                       "StreamingConformerEncoder")] == \
        ["ctc_decoder", "tf_residual_stack", "separable_conv1d", "leaky_re_lu", "multi_head_attention", "conv2d", "streaming_conformer_encoder"]

    class Inner(tf.keras.layers.Layer):
        def __init__(self):
            super().__init__()
            self.d1, self.d2 = tf.keras.layers.Dense(3), tf.keras.layers.Dense(2, name="named")

        def call(self, x, training=False):
            return self.d2(self.d1(x, training=training))

    class Outer(tf.keras.Model):
        def __init__(self):
            super().__init__()
            self.blocks = []
            for _ in range(2):
                self.blocks.append(Inner())
            self.frozen = tf.keras.layers.Dense(2)
            self.frozen.trainable = False
            self.const = tf.keras.backend.variable(np.ones((2, 2)), dtype="float32", name="table")

        def call(self, x):
            for b in self.blocks:
                x = b(x)
            return self.frozen(x)

    m = Outer()
    m(tf.zeros([1, 5, 2]))
    assert [v.name for v in m.trainable_weights] == [                 # a layer's own variables, then its sublayers' (Keras order)
        "table:0",
        "outer/inner/dense/kernel:0", "outer/inner/dense/bias:0", "outer/inner/named/kernel:0", "outer/inner/named/bias:0",
        "outer/inner_1/dense_1/kernel:0", "outer/inner_1/dense_1/bias:0", "outer/inner_1/named/kernel:0", "outer/inner_1/named/bias:0"]
    assert [v.name for v in m.non_trainable_weights] == ["outer/dense_2/kernel:0", "outer/dense_2/bias:0"]
    m.non_trainable_weights.append("ignored")              # appending to the returned list is a no-op, as in Keras
    assert len(m.non_trainable_weights) == 2
    keys = sorted(m._object_graph())
    assert "blocks/1/d2/kernel/.ATTRIBUTES/VARIABLE_VALUE" in keys and "const/.ATTRIBUTES/VARIABLE_VALUE" in keys and len(keys) == 11
