"""TEST INFRASTRUCTURE ONLY.  A NumPy evaluator of the punctuation model's exported graph (tests/golden/punc.onnx.part*,
tf2onnx opset 13), in float64 or float32 throughout.  `oracle.onnx_mini.load` parses the file; the interpreter is here
because `oracle.onnx_mini.run` lacks ten of the graph's operators and casts to fixed dtypes.

    g = Graph(onnx_path())
    probs = g.probs(ids [B, T] int32, np.float64)        # [B, T, 32]; mask and pos_encoding are built as the reference does
"""
import atexit
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import onnx_mini  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_joined = None


def onnx_path():
    """The weights file is committed in parts (each under the repository's file-size limit); they are joined once per process
    into a temporary file, byte for byte the reference's punc.onnx."""
    global _joined
    if _joined is None or not os.path.exists(_joined):
        parts = sorted(f for f in os.listdir(GOLDEN) if f.startswith("punc.onnx.part"))
        assert parts, "tests/golden/punc.onnx.part* missing"
        fd, path = tempfile.mkstemp(prefix="punc_", suffix=".onnx")
        with os.fdopen(fd, "wb") as out:
            for p in parts:
                with open(os.path.join(GOLDEN, p), "rb") as f:
                    out.write(f.read())
        _joined = path
        atexit.register(lambda: os.path.exists(path) and os.remove(path))
    return _joined


def reference_pos_encoding(pe_input=1024, d_model=64):
    """punc_recover.py Punc.get_pos_encoding, verbatim arithmetic -> [pe_input, d_model] float32"""
    pos = np.arange(pe_input)[:, np.newaxis]
    i = np.arange(d_model)[np.newaxis, :]
    angle_rates = 1 / np.power(10000, (2 * (i // 2)) / np.float32(d_model))
    angle_rads = pos * angle_rates
    angle_rads[:, 0::2] = np.sin(angle_rads[:, 0::2])
    angle_rads[:, 1::2] = np.cos(angle_rads[:, 1::2])
    return np.array(angle_rads, "float32")


_NP_OF = {6: np.int32, 7: np.int64, 9: np.bool_}


def _conv(x, w, b, attrs):
    """NCHW x OIHW, unit strides and dilations, explicit pads or VALID"""
    assert attrs.get("strides", [1, 1]) == [1, 1] and attrs.get("dilations", [1, 1]) == [1, 1] and attrs.get("group", 1) == 1
    assert attrs.get("auto_pad", b"NOTSET") in (b"NOTSET", b"VALID")
    p = attrs.get("pads", [0, 0, 0, 0])
    xp = np.pad(x, ((0, 0), (0, 0), (p[0], p[2]), (p[1], p[3])))
    o, c, kh, kw = w.shape
    oh, ow = xp.shape[2] - kh + 1, xp.shape[3] - kw + 1
    y = np.zeros((x.shape[0], o, oh, ow), dtype=x.dtype)
    for i in range(kh):
        for j in range(kw):
            y += np.einsum("nchw,oc->nohw", xp[:, :, i:i + oh, j:j + ow], w[:, :, i, j])
    if b is not None:
        y += b.reshape(1, -1, 1, 1)
    return y


class Graph:
    def __init__(self, path=None):
        self.nodes, self.inits, self.inputs, self.outputs = onnx_mini.load(path or onnx_path())

    def weight_initialisers(self):
        """names of the float initialisers with more than one element: the model's weights"""
        return sorted(k for k, v in self.inits.items() if v.dtype.kind == "f" and v.size > 3)

    def probs(self, ids, dtype=np.float64, pos_encoding=None):
        ids = np.asarray(ids, np.int32)
        pe = reference_pos_encoding() if pos_encoding is None else pos_encoding
        mask = np.array(ids == 0, "float32")[:, np.newaxis, np.newaxis, :]
        feeds = dict(zip(self.inputs, (ids, mask, pe[np.newaxis])))
        return self.run(feeds, dtype)[0]

    def run(self, feeds, dtype):
        f = lambda a: a.astype(dtype) if a.dtype.kind == "f" else a
        env = {k: f(v) for k, v in self.inits.items()}
        env.update({k: f(np.asarray(v)) for k, v in feeds.items()})
        for nd in self.nodes:
            i = [env[n] if n else None for n in nd.inputs]
            a, op = nd.attrs, nd.op
            if op == "Reshape":
                r = i[0].reshape([int(i[0].shape[k]) if s == 0 else int(s) for k, s in enumerate(i[1].tolist())])
            elif op == "Cast":
                r = i[0].astype(dtype if a["to"] in (1, 11) else _NP_OF[a["to"]])
            elif op == "Gather":
                r = np.take(i[0], i[1], axis=a.get("axis", 0))
            elif op == "Shape":
                r = np.array(i[0].shape, dtype=np.int64)
            elif op == "Squeeze":
                r = np.squeeze(i[0], axis=tuple(int(v) for v in i[1].tolist())) if len(i) > 1 else np.squeeze(i[0])
            elif op == "Unsqueeze":
                r = i[0]
                for ax in sorted(int(v) for v in i[1].tolist()):
                    r = np.expand_dims(r, ax)
            elif op == "Add":
                r = i[0] + i[1]
            elif op == "Sub":
                r = i[0] - i[1]
            elif op == "Mul":
                r = i[0] * i[1]
            elif op == "Div":
                r = i[0] / i[1] if i[0].dtype.kind == "f" else i[0] // i[1]
            elif op == "Max":
                r = np.maximum(i[0], i[1])
            elif op == "Sqrt":
                r = np.sqrt(i[0])
            elif op == "Reciprocal":
                r = 1 / i[0]
            elif op == "Relu":
                r = np.maximum(i[0], 0)
            elif op == "Elu":
                al = a.get("alpha", 1.0)
                r = np.where(i[0] > 0, i[0], (al * np.expm1(np.minimum(i[0], 0))).astype(i[0].dtype))
            elif op == "Less":
                r = i[0] < i[1]
            elif op == "Equal":
                r = i[0] == i[1]
            elif op == "And":
                r = np.logical_and(i[0], i[1])
            elif op == "Where":
                r = np.where(i[0], i[1], i[2])
            elif op == "Concat":
                r = np.concatenate(i, axis=a["axis"])
            elif op == "Transpose":
                r = np.transpose(i[0], a["perm"])
            elif op == "MatMul":
                r = np.matmul(i[0], i[1])
            elif op == "GlobalAveragePool":
                r = i[0].mean(axis=tuple(range(2, i[0].ndim)), keepdims=True)
            elif op == "Pad":
                assert a.get("mode", b"constant") == b"constant"
                p = [int(v) for v in i[1].tolist()]
                n = len(p) // 2
                cv = i[2].reshape(()) if len(i) > 2 and i[2] is not None and i[2].size else 0
                r = np.pad(i[0], [(p[k], p[k + n]) for k in range(n)], constant_values=cv)
            elif op == "Slice":
                starts, ends = i[1].tolist(), i[2].tolist()
                axes = i[3].tolist() if len(i) > 3 and i[3] is not None else list(range(len(starts)))
                steps = i[4].tolist() if len(i) > 4 and i[4] is not None else [1] * len(starts)
                sl = [slice(None)] * i[0].ndim
                for s, e, ax, st in zip(starts, ends, axes, steps):
                    sl[ax] = slice(int(s), int(e), int(st))
                r = i[0][tuple(sl)]
            elif op == "Conv":
                r = _conv(i[0], i[1], i[2] if len(i) > 2 else None, a)
            elif op == "Softmax":
                ax = a.get("axis", -1)
                z = i[0] - i[0].max(axis=ax, keepdims=True)
                e = np.exp(z)
                r = e / e.sum(axis=ax, keepdims=True)
            elif op == "Identity":
                r = i[0]
            else:
                raise NotImplementedError(op)
            if isinstance(r, np.ndarray) and r.dtype.kind == "f" and r.dtype != dtype:
                r = r.astype(dtype)
            env[nd.outputs[0]] = r
        return [env[o] for o in self.outputs]
