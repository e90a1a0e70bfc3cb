"""TEST INFRASTRUCTURE ONLY -- a NumPy interpreter for the function library of a TensorFlow SavedModel, just large
enough to run the reference's online VAD (tests/golden/online_vad_model) without TensorFlow.

Wire format facts follow the public TensorFlow protobuf schemas (saved_model.proto, meta_graph.proto, graph.proto,
function.proto, node_def.proto, attr_value.proto, tensor.proto, op_def.proto, saved_object_graph.proto):
  SavedModel.meta_graphs=2; MetaGraphDef.graph_def=2 / object_graph_def=7; GraphDef.library=2;
  FunctionDefLibrary.function=1; FunctionDef.signature=1 (OpDef) / node_def=3 / ret=4 (map);
  OpDef.name=1 / input_arg=2 / output_arg=3; ArgDef.name=1;
  NodeDef.name=1 / op=2 / input=3 / attr=5 (map); AttrValue.list=1 / s=2 / i=3 / f=4 / b=5 / type=6 / tensor=8 / func=10;
  NameAttrList.name=1; TensorProto.dtype=1 / tensor_shape=2 / tensor_content=4 / float_val=5 / int_val=7 / int64_val=10;
  TensorShapeProto.dim=2 (size=1); SavedObjectGraph.nodes=1 / concrete_functions=2 (map);
  SavedObject.children=1 / function=6 / variable=7; SavedFunction.concrete_functions=1;
  SavedConcreteFunction.bound_inputs=2.
Resource arguments of a concrete function are its trailing inputs, bound (in order) to the objects `bound_inputs`
names; the SavedModel's object graph numbers its nodes as the checkpoint's TrackableObjectGraph does, whose attributes
give each variable's checkpoint key (tensorflowasr_amd/tfbundle.py reads those).

    g = SavedModelGraph(path)          # directory with saved_model.pb and variables/
    score, enhanced = g.call(frames)   # the Keras call function: [B, T, 80] -> ([B, T, 1], [B, T, 80])
    score = g.inference(frames)        # the exported `inference` tf.function
"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.onnx_mini import _fields, _packed_varints, _signed  # noqa: E402
from tensorflowasr_amd import tfbundle  # noqa: E402

_DT = {1: np.float32, 2: np.float64, 3: np.int32, 9: np.int64, 10: np.bool_, 20: None}   # 20 = DT_RESOURCE


def _s(v):
    return bytes(v).decode("utf8", "surrogateescape")


def _map_entries(buf):
    k = v = None
    for f, _, x in _fields(buf):
        if f == 1:
            k = _s(x)
        elif f == 2:
            v = x
    return k, v


def _tensor(buf):
    dtype, dims, content, vals = 1, [], None, []
    for f, wt, v in _fields(buf):
        if f == 1:
            dtype = v
        elif f == 2:
            for g, _, d in _fields(v):
                if g == 2:
                    for h, _, sz in _fields(d):
                        if h == 1:
                            dims.append(_signed(sz))
        elif f == 4:
            content = bytes(v)
        elif f == 5:
            vals += list(struct.unpack("<%df" % (len(v) // 4), v)) if wt == 2 else [struct.unpack("<f", v)[0]]
        elif f in (7, 10):
            vals += _packed_varints(v) if wt == 2 else [_signed(v)]
    if dtype not in _DT or _DT[dtype] is None:
        return None                       # strings / resources: never computed on
    dt = _DT[dtype]
    n = int(np.prod(dims)) if dims else 1
    if content is not None:
        a = np.frombuffer(content, dt).copy()
    else:
        a = np.array(vals, dt)
        if a.size == 1 and n != 1:
            a = np.full(n, a[0], dt)
        elif a.size == 0:
            a = np.zeros(n, dt)
    return a.reshape(dims)


def _attr(buf):
    """AttrValue -> python value (list -> list of ints / strings)"""
    for f, wt, v in _fields(buf):
        if f == 1:
            out = []
            for g, gw, x in _fields(v):
                if g == 2:
                    out.append(_s(x))
                elif g == 3:
                    out += _packed_varints(x) if gw == 2 else [_signed(x)]
                elif g == 6:
                    out += _packed_varints(x) if gw == 2 else [x]
            return out
        if f == 2:
            return _s(v)
        if f == 3:
            return _signed(v)
        if f == 4:
            return struct.unpack("<f", v)[0]
        if f in (5, 6):
            return v
        if f == 8:
            return _tensor(v)
        if f == 10:
            for g, _, x in _fields(v):
                if g == 1:
                    return _s(x)
    return None


class Node:
    __slots__ = ("name", "op", "inputs", "attrs")

    def __init__(self, buf):
        self.name, self.op, self.inputs, self.attrs = "", "", [], {}
        for f, _, v in _fields(buf):
            if f == 1:
                self.name = _s(v)
            elif f == 2:
                self.op = _s(v)
            elif f == 3:
                self.inputs.append(_s(v))
            elif f == 5:
                k, a = _map_entries(v)
                self.attrs[k] = _attr(a)


class Function:
    def __init__(self, buf):
        self.name, self.args, self.outs, self.nodes, self.ret = "", [], [], [], {}
        for f, _, v in _fields(buf):
            if f == 1:
                for g, _, x in _fields(v):
                    if g == 1:
                        self.name = _s(x)
                    elif g in (2, 3):
                        nm = [_s(y) for h, _, y in _fields(x) if h == 1][0]
                        (self.args if g == 2 else self.outs).append(nm)
            elif f == 3:
                self.nodes.append(Node(v))
            elif f == 4:
                k, r = _map_entries(v)
                self.ret[k] = _s(r)


class SavedModelGraph:
    def __init__(self, path, dtype=np.float32):
        blob = memoryview(open(os.path.join(path, "saved_model.pb"), "rb").read())
        mg = [v for f, _, v in _fields(blob) if f == 2][0]
        self.functions, self.objects, self.concrete = {}, [], {}
        for f, _, v in _fields(mg):
            if f == 2:
                for g, _, lib in _fields(v):
                    if g == 2:
                        for h, _, fn in _fields(lib):
                            if h == 1:
                                fd = Function(fn)
                                self.functions[fd.name] = fd
            elif f == 7:
                for g, _, x in _fields(v):
                    if g == 1:
                        self.objects.append(self._object(x))
                    elif g == 2:
                        k, c = _map_entries(x)
                        self.concrete[k] = [_signed(b) for h, hw, y in _fields(c) if h == 2
                                            for b in (_packed_varints(y) if hw == 2 else [y])]
        bundle = tfbundle.Bundle(tfbundle.checkpoint_prefix(path))
        self.dtype = dtype
        # object node id -> variable value (checkpoint key of the same node in the TrackableObjectGraph)
        self.values, self.names = {}, {}
        for nid, (_, attrs) in enumerate(bundle.object_graph()):
            for aname, full, ckey in attrs:
                if aname == "VARIABLE_VALUE":
                    self.values[nid] = bundle.tensor(ckey).astype(dtype)
                    self.names[nid] = full

    @staticmethod
    def _object(buf):
        children, fns = {}, []
        for f, _, v in _fields(buf):
            if f == 1:
                nid, name = 0, ""
                for g, _, x in _fields(v):
                    if g == 1:
                        nid = x
                    elif g == 2:
                        name = _s(x)
                children[name] = nid
            elif f == 6:
                fns = [_s(x) for g, _, x in _fields(v) if g == 1]
        return children, fns

    # ---- lookup -----------------------------------------------------------------------------------------------------
    def concrete_for(self, attr, prefix="__inference_"):
        """concrete functions of the root object's tf.function child `attr`"""
        nid = self.objects[0][0][attr]
        return [c for c in self.objects[nid][1] if c.startswith(prefix)]

    def run_concrete(self, name, *inputs):
        """call concrete function `name` with `inputs`, its captured variables bound from the object graph"""
        fd = self.functions[name]
        bound = [self.values[i] for i in self.concrete[name]]
        args = list(inputs) + bound
        assert len(args) == len(fd.args), (name, len(args), len(fd.args))
        return self.run_function(fd, args)

    def call(self, frames):
        """the Keras layer's call function (the one that returns both outputs)"""
        name = [n for n in self.functions if "online_cnn_vad_layer_call_and_return_conditional_losses" in n]
        fd = self.functions[sorted(name)[0]]
        nvar = len(fd.args) - 1
        # its resource arguments are the layer's variables, in the order of the layer's concrete call function
        caller = self._caller_of(fd.name)
        return self.run_function(fd, [np.asarray(frames, self.dtype)] + caller[:nvar])

    def inference(self, frames):
        cf = [c for c in self.concrete_for("inference")]
        return self.run_concrete(cf[0], np.asarray(frames, self.dtype))

    def _caller_of(self, fname):
        """variable values passed to `fname` by the StatefulPartitionedCall in some concrete function"""
        for cname, ids in self.concrete.items():
            if cname not in self.functions or not ids:
                continue
            fd = self.functions[cname]
            for nd in fd.nodes:
                if nd.op in ("StatefulPartitionedCall", "PartitionedCall") and nd.attrs.get("f") == fname:
                    env = {a: None for a in fd.args}
                    nin = len(fd.args) - len(ids)
                    for a, i in zip(fd.args[nin:], ids):
                        env[a] = self.values[i]
                    return [env[i.split(":")[0]] for i in nd.inputs if not i.startswith("^")][1:]
        raise KeyError(fname)

    # ---- interpreter ------------------------------------------------------------------------------------------------
    def run_function(self, fd, args):
        env = dict(zip(fd.args, args))
        outs = {}

        def get(ref):
            parts = ref.split(":")
            if len(parts) == 1:
                return env[parts[0]]
            node, oname, idx = parts[0], parts[1], int(parts[2]) if len(parts) > 2 else 0
            return outs[node][idx]

        pending = list(fd.nodes)
        while pending:
            left = []
            for nd in pending:
                ins = [i for i in nd.inputs if not i.startswith("^")]
                ready = all((i.split(":")[0] in outs) if ":" in i else (i in env) for i in ins)
                ctrl = all(i[1:] in outs for i in nd.inputs if i.startswith("^"))
                if not (ready and ctrl):
                    left.append(nd)
                    continue
                outs[nd.name] = self._op(nd, [get(i) for i in ins])
            assert len(left) < len(pending), "cyclic or unresolved: %s" % [n.name for n in left]
            pending = left
        return tuple(get(fd.ret[o]) for o in fd.outs)

    def _op(self, nd, x):
        op, a = nd.op, nd.attrs
        if op in ("ReadVariableOp", "Identity", "NoOp"):
            return [x[0] if x else None]
        if op == "Const":
            v = a["value"]
            return [v.astype(self.dtype) if v.dtype.kind == "f" else v]
        if op in ("StatefulPartitionedCall", "PartitionedCall"):
            return list(self.run_function(self.functions[a["f"]], x))
        if op == "Shape":
            return [np.array(x[0].shape, np.int32)]
        if op == "GatherV2":
            return [np.take(x[0], x[1], axis=int(x[2]))]
        if op == "Prod":
            return [np.array(np.prod(x[0], axis=tuple(np.atleast_1d(x[1])), keepdims=bool(a.get("keep_dims"))),
                             x[0].dtype)]
        if op == "ConcatV2":
            return [np.concatenate(x[:-1], axis=int(x[-1]))]
        if op == "Pack":
            return [np.stack(x, axis=a.get("axis", 0))]
        if op == "Transpose":
            return [np.transpose(x[0], x[1])]
        if op == "Reshape":
            return [np.reshape(x[0], x[1])]
        if op == "MatMul":
            p, q = x
            p = p.T if a.get("transpose_a") else p
            q = q.T if a.get("transpose_b") else q
            return [p @ q]
        if op == "BiasAdd":
            return [x[0] + x[1]]
        if op in ("Add", "AddV2"):
            return [x[0] + x[1]]
        if op == "Less":
            return [x[0] < x[1]]
        if op == "Sub":
            return [x[0] - x[1]]
        if op == "Mul":
            return [x[0] * x[1]]
        if op == "Relu":
            return [np.maximum(x[0], 0)]
        if op == "Pad":
            return [np.pad(x[0], [tuple(r) for r in x[1]])]
        if op == "ExpandDims":
            return [np.expand_dims(x[0], int(x[1]))]
        if op == "Squeeze":
            dims = a.get("squeeze_dims") or None
            return [np.squeeze(x[0], axis=tuple(dims) if dims else None)]
        if op == "Conv2D":
            return [self._conv2d(x[0], x[1], a)]
        if op == "FusedBatchNormV3":
            # Keras LayerNormalization lowers to this in training form: per-channel batch statistics (population
            # variance) over every axis but the channel one, then scale * x_hat + offset
            xx, scale, offset, mean, var = x
            eps = self.dtype(a.get("epsilon", 1e-4))
            ch = 1 if a.get("data_format", "NHWC") == "NCHW" else 3
            axes = tuple(d for d in range(4) if d != ch)
            shape = [1, 1, 1, 1]
            shape[ch] = -1
            assert a.get("is_training", True), "inference-form batch norm is not used by this graph"
            mean = xx.mean(axis=axes, keepdims=True)
            var = ((xx - mean) ** 2).mean(axis=axes, keepdims=True)
            y = (xx - mean) / np.sqrt(var + eps) * scale.reshape(shape) + offset.reshape(shape)
            return [y.astype(self.dtype), mean.reshape(-1), var.reshape(-1), None, None, None]
        if op == "Fill":
            return [np.full(x[0], x[1])]
        if op == "StridedSlice":
            return [self._strided_slice(x, a)]
        raise NotImplementedError("op %s (%s)" % (op, nd.name))

    @staticmethod
    def _conv2d(x, w, a):
        """NHWC, VALID, strides / dilations 1 (all the graph uses): x [N, H, W, C], w [kh, kw, C, O]"""
        assert a.get("padding") == "VALID", a.get("padding")
        assert all(s == 1 for s in a.get("strides", [1, 1, 1, 1])) and all(d == 1 for d in a.get("dilations", [1, 1, 1, 1]))
        N, H, W_, C = x.shape
        kh, kw, _, O = w.shape
        Ho, Wo = H - kh + 1, W_ - kw + 1
        y = np.zeros((N, Ho, Wo, O), np.result_type(x, w))
        for i in range(kh):
            for j in range(kw):
                y += np.einsum("nhwc,co->nhwo", x[:, i:i + Ho, j:j + Wo, :], w[i, j])
        return y

    @staticmethod
    def _strided_slice(x, a):
        t, begin, end, stride = x
        bm, em, sm = a.get("begin_mask", 0), a.get("end_mask", 0), a.get("shrink_axis_mask", 0)
        assert not a.get("ellipsis_mask", 0) and not a.get("new_axis_mask", 0)
        sl = []
        for d in range(len(begin)):
            if sm >> d & 1:
                sl.append(int(begin[d]))
            else:
                sl.append(slice(None if bm >> d & 1 else int(begin[d]), None if em >> d & 1 else int(end[d]),
                                int(stride[d])))
        return np.asarray(t[tuple(sl)])
