"""Punctuation restoration: the reference's trained `punc.onnx` (PuncTransformer.inference) on the MI355X (punc.hip) and
the rule `Inference/PythonInference/punc_recover/src/punc_recover.py` puts on top of it.

    punc = Punc(config); punc.load_onnx('punc.onnx')
    ''.join(punc.punc_recover('今天天气怎么样'))            # one fused HIP launch per call
    punc.punc_recover_batch([text, ...])                    # ... or per list of texts
    StreamingASRSession(asr, vad, punc=punc)                # an instance is the sessions' `punc=` hook

`config` carries the reference's keys: `model_config` (punc_settings.yml), `punc_vocab` and `punc_biaodian` (data.yml)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .featurizers import TextFeaturizer
from .models import _Handle, _p

THRESHOLD = 0.65
LAYER_DENSES = ("mha/wq", "mha/wk", "mha/wv", "mha/dense", "ffn/dense_1", "ffn/dense_2")


def map_layers(num_layers):
    """PuncTransformer.map_encoders"""
    return max(int(num_layers) - 1, 1)


def onnx_names(num_layers=3):
    """ABI weight name -> tf2onnx initialiser name of a PuncTransformer export.  Keras numbers the Dense layers in creation
    order (projecter, then wq wk wv dense ffn ffn per EncoderLayer, to_bert, to_hidden, the map layers, final), the
    LayerNormalizations two per layer, and scopes the first `num_layers` layers under encoder/.  The Conv1D biases are
    folded constants whose names belong to the shipped export (num_layers 3)."""
    n = int(num_layers)
    k = lambda d: "/dense_%d/Tensordot/ReadVariableOp:0" % d if d else "/dense/Tensordot/ReadVariableOp:0"
    b = lambda d: "/dense_%d/BiasAdd/ReadVariableOp:0" % d if d else "/dense/BiasAdd/ReadVariableOp:0"
    sfx = lambda i: "_%d" % i if i else ""
    names = {"embedding": "encoder/embedding/embedding_lookup/52598:0",
             "encoder/dense/kernel": "encoder" + k(0), "encoder/dense/bias": "encoder" + b(0)}

    def layer(abi, scope, L, first_dense):
        mha = "%sencoder_layer%s/multi_head_attention%s" % (scope, sfx(L), sfx(L))
        seq = "%sencoder_layer%s/sequential%s" % (scope, sfx(L), sfx(L))
        for j, nm in enumerate(LAYER_DENSES):
            base = mha if j < 4 else seq
            names["%s/%s/kernel" % (abi, nm)] = base + k(first_dense + j)
            names["%s/%s/bias" % (abi, nm)] = base + b(first_dense + j)
        for j in (0, 1):
            ln = "%sencoder_layer%s/layer_normalization%s/batchnorm" % (scope, sfx(L), sfx(2 * L + j))
            names["%s/layernorm%d/gamma" % (abi, j + 1)] = ln + "/mul/ReadVariableOp:0"
            names["%s/layernorm%d/beta" % (abi, j + 1)] = ln + "/ReadVariableOp:0"

    conv_bias = {0: "const_fold_opt__797", 1: "const_fold_opt__796", 2: "const_fold_opt__799"}
    for i in range(n):
        layer("encoder/layer_%d" % i, "encoder/", i, 1 + 6 * i)
        names["encoder/conv_%d/kernel" % i] = "encoder/conv1d%s/conv1d/ExpandDims_1:0" % sfx(i)
        if n == 3:
            names["encoder/conv_%d/bias" % i] = conv_bias[i]
    d = 6 * n + 1
    names["to_bert/kernel"], names["to_bert/bias"] = k(d)[1:], b(d)[1:]
    names["to_hidden/kernel"], names["to_hidden/bias"] = k(d + 1)[1:], b(d + 1)[1:]
    for j in range(map_layers(n)):
        layer("map/layer_%d" % j, "", n + j, d + 2 + 6 * j)
    f = d + 2 + 6 * map_layers(n)
    names["final/kernel"] = "time_distributed/dense_%d/MatMul/ReadVariableOp:0" % f
    names["final/bias"] = "time_distributed" + b(f)
    return names


ONNX_NAMES = onnx_names(3)


def graph_weight_names(inits):
    """the initialisers of a graph that are weights: float tensors of more than three elements (the rest are shape and
    mask constants)"""
    return sorted(k for k, v in inits.items() if np.asarray(v).dtype.kind == "f" and np.asarray(v).size > 3)


def weights_from_onnx_inits(inits, num_layers=3):
    """tf2onnx initialisers -> ABI weights: conv kernels [out, in, 1, 3] -> [3, in, out], conv biases [1, 64, 1] -> [64];
    raises if the graph holds a weight the map does not name, or lacks one it names."""
    names = onnx_names(num_layers)
    unmapped = sorted(set(graph_weight_names(inits)) - set(names.values()))
    if unmapped:
        raise ValueError("punc graph: weights without an ABI name: %s" % unmapped)
    missing = sorted(g for g in names.values() if g not in inits)
    if missing:
        raise ValueError("punc graph lacks %s" % missing)
    w = {}
    for abi, g in names.items():
        a = np.asarray(inits[g], np.float32)
        if abi.startswith("encoder/conv_") and abi.endswith("kernel"):
            a = a[:, :, 0, :].transpose(2, 1, 0)
        elif abi.endswith("bias"):
            a = a.reshape(-1)
        w[abi] = np.ascontiguousarray(a)
    return w


def pos_encoding(pe_input, d_model):
    """punc_recover.py Punc.get_pos_encoding, digit for digit: float64 angles with the exponent divided by
    np.float32(d_model), sin on even and cos on odd columns, cast to float32 at the end -> [pe_input, d_model]"""
    pos = np.arange(pe_input)[:, np.newaxis]
    i = np.arange(d_model)[np.newaxis, :]
    angle_rates = 1 / np.power(10000, (2 * (i // 2)) / np.float32(d_model))
    angle_rads = pos * angle_rates
    angle_rads[:, 0::2] = np.sin(angle_rads[:, 0::2])
    angle_rads[:, 1::2] = np.cos(angle_rads[:, 1::2])
    return np.array(angle_rads, "float32")


FEATURE_DIM = 768               # to_bert's width (kBert of csrc/punc.hip)


def lengths_from_ids(ids):
    """PuncTrainer.creat_mask's rule as lengths: ids int [B, T] (array or tensor, any device), 0 = padding -> i32 [B] on the
    ids' device, a row's length one past its last non-zero id.  An id 0 in front of a non-zero id raises ValueError."""
    x = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids)))
    if x.dim() != 2:
        raise ValueError("ids are [B, T] (got shape %s)" % (tuple(x.shape),))
    used = x != 0
    pos = torch.arange(1, x.shape[1] + 1, device=x.device, dtype=torch.int32)
    ln = (used.to(torch.int32) * pos).amax(1) if x.shape[1] else torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
    inner = (~used) & (pos[None, :] <= ln[:, None])
    if bool(inner.any()):
        b, t = (int(v) for v in inner.nonzero()[0])
        raise ValueError("id 0 at token %d of row %d, in front of a non-zero id: padding must follow the sentence" % (t, b))
    return ln.to(torch.int32)


def apply_rule(txt, cls, pmax, vocab_array):
    """punc_recover's loop on the rows of the characters (markers dropped): after character t the mark
    `vocab_array[argmax]` when argmax > 1 and max >= 0.65 -> list"""
    out = []
    for ch, c, p in zip(txt, cls, pmax):
        out.append(ch)
        if c > 1 and p >= THRESHOLD:
            out.append(vocab_array[c])
    return out


class Punc:
    """The reference's Punc (punc_recover/src/punc_recover.py) on libmi355asr.so.

    on_unknown: a character outside the punctuation vocabulary raises KeyError as in the reference ("raise", the default);
    "skip" returns such a text as it came, as a list of its characters, without a launch -- the ASR vocabulary is larger than
    the punctuation one."""

    def __init__(self, config, device="cuda:0", on_unknown="raise", weights=None):
        if on_unknown not in ("raise", "skip"):
            raise ValueError("on_unknown must be 'raise' or 'skip', got %r" % (on_unknown,))
        self.on_unknown = on_unknown
        self.model_config = dict(config["model_config"])
        self.vocab_featurizer = TextFeaturizer(dict(config["punc_vocab"]))
        self.bd_featurizer = TextFeaturizer(dict(config["punc_biaodian"]))
        self.device = torch.device(device)
        mc = self.model_config
        self.cfg = dict(d_model=int(mc["d_model"]), enc_embedding_dim=int(mc["enc_embedding_dim"]), num_heads=int(mc["num_heads"]),
                        dff=int(mc["dff"]), num_layers=int(mc["num_layers"]), vocab=int(self.vocab_featurizer.num_classes),
                        classes=int(self.bd_featurizer.num_classes), pe_input=int(mc["pe_input"]))
        self.pos_encode_inputs = pos_encoding(self.cfg["pe_input"], self.cfg["d_model"])[np.newaxis]
        self._handle_ = None
        if weights is not None:
            self.load_weights(weights)

    # ---- weights ---------------------------------------------------------------------------------------------------------
    def weight_names(self):
        """the ABI names this configuration takes (include/mi355asr.h), `pos_encoding` included"""
        n = ["embedding", "pos_encoding", "encoder/dense/kernel", "encoder/dense/bias"]
        layer = lambda p: ["%s/%s/%s" % (p, d, s) for d in LAYER_DENSES for s in ("kernel", "bias")] + \
            ["%s/layernorm%d/%s" % (p, j, s) for j in (1, 2) for s in ("gamma", "beta")]
        for i in range(self.cfg["num_layers"]):
            n += layer("encoder/layer_%d" % i) + ["encoder/conv_%d/kernel" % i, "encoder/conv_%d/bias" % i]
        n += ["to_bert/kernel", "to_bert/bias", "to_hidden/kernel", "to_hidden/bias"]
        for i in range(map_layers(self.cfg["num_layers"])):
            n += layer("map/layer_%d" % i)
        return n + ["final/kernel", "final/bias"]

    def load_onnx(self, path):
        from .checkpoint import read_onnx
        _, inits = read_onnx(path)
        return self.load_weights(weights_from_onnx_inits(inits, self.cfg["num_layers"]))

    def load_weights(self, weights):
        """dict or .npz of ABI-named tensors; `pos_encoding` defaults to the reference's table.  Raises if a tensor of the
        model is left unset or a name is not the model's."""
        if isinstance(weights, str):
            with np.load(weights) as z:
                weights = {k: z[k] for k in z.files}
        w = {k: np.ascontiguousarray(np.asarray(v, np.float32)) for k, v in weights.items()}
        w.setdefault("pos_encoding", self.pos_encode_inputs[0])
        want = set(self.weight_names())
        if set(w) != want:
            raise ValueError("Punc weights: missing %s, unexpected %s" % (sorted(want - set(w)), sorted(set(w) - want)))
        self.weights = w
        self._handle_ = None
        return self

    def _handle(self):
        if self._handle_ is None:
            if not hasattr(self, "weights"):
                raise _lib.Mi355AsrError("Punc: no weights loaded (load_onnx / load_weights)")
            h = _Handle(_lib.PuncConfig(**self.cfg), self.device, create=_lib.lib().mi355asr_punc_create)
            h.load(self.weights)
            h.finalize()
            lt, mt = ctypes.c_int32(), ctypes.c_int32()
            _lib.check(h.lib.mi355asr_punc_limits(h.ptr, ctypes.byref(lt), ctypes.byref(mt)))
            self.lds_tokens, self.max_tokens = lt.value, mt.value
            self._handle_ = h
        return self._handle_

    # ---- the model ---------------------------------------------------------------------------------------------------------
    def forward(self, ids, lengths=None, want_decisions=True):
        """ids [T] or [B, T] (int; padding past a row's length may be anything in range), lengths [B] or None ->
        (probs [B, T, classes], argmax class [B, T] int32, its probability [B, T]) on the device, one launch.  Everything
        at or past a row's length is 0.  An id outside [0, vocab) is refused here, before any launch."""
        h = self._handle()
        x = h.to_device(ids, dtype=torch.int32)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError("expected ids [T] or [B, T] with T >= 1, got %s" % (tuple(x.shape),))
        B, T = x.shape
        if T > self.max_tokens:
            raise ValueError("%d tokens (markers included) exceed pe_input = %d" % (T, self.max_tokens))
        if B and (int(x.min()) < 0 or int(x.max()) >= self.cfg["vocab"]):
            raise ValueError("token id outside [0, %d)" % self.cfg["vocab"])
        ln = None
        if lengths is not None:
            ln = h.to_device(np.asarray(lengths), dtype=torch.int32)
            if ln.shape != (B,):
                raise ValueError("lengths must be [B]")
        C = self.cfg["classes"]
        probs = torch.empty((B, T, C), dtype=torch.float32, device=h.device)
        cls = torch.empty((B, T), dtype=torch.int32, device=h.device) if want_decisions else None
        pmax = torch.empty((B, T), dtype=torch.float32, device=h.device) if want_decisions else None
        if B:
            n = ctypes.c_size_t()
            _lib.check(h.lib.mi355asr_punc_workspace_bytes(h.ptr, B, T, ctypes.byref(n)))
            ws = h.workspace(n.value) if n.value else None
            with torch.cuda.device(h.device):
                _lib.check(h.lib.mi355asr_punc_forward(h.ptr, _p(x), _p(ln), B, T, _p(probs), _p(cls), _p(pmax), _p(ws), n.value,
                                                       h._stream()))
        return probs, cls, pmax

    def heads(self, ids, lengths=None, want_logits=True, want_feature=True):
        """The model's training outputs, `PuncTransformer.call([inp, mask], training=False)` as PuncTrainer._eval_step runs it:
        -> (logits [B, T, classes], the values `forward` takes its softmax of, and feature [B, T, 768] = to_bert(enc_output),
        the distillation feature) on the device, one launch; the one not wanted is None.  Rows at or past a sentence's length
        are zeros (the reference computes values there; the trainer's losses mask them).
        lengths=None: taken from the ids as the reference's creat_mask does from `ids == 0` -- a row's length is one past its
        last non-zero id; an id 0 in front of a non-zero id is a ValueError (the kernel masks by length, the reference would
        mask that key alone)."""
        if not (want_logits or want_feature):
            raise ValueError("heads: neither output is wanted")
        h = self._handle()
        x = h.to_device(ids, dtype=torch.int32)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError("expected ids [T] or [B, T] with T >= 1, got %s" % (tuple(x.shape),))
        B, T = x.shape
        if T > self.max_tokens:
            raise ValueError("%d tokens (markers included) exceed pe_input = %d" % (T, self.max_tokens))
        if B and (int(x.min()) < 0 or int(x.max()) >= self.cfg["vocab"]):
            raise ValueError("token id outside [0, %d)" % self.cfg["vocab"])
        if lengths is None:
            ln = lengths_from_ids(x)
        else:
            ln = h.to_device(lengths if torch.is_tensor(lengths) else np.asarray(lengths), dtype=torch.int32)
            if ln.shape != (B,):
                raise ValueError("lengths must be [B]")
        C = self.cfg["classes"]
        logits = torch.empty((B, T, C), dtype=torch.float32, device=h.device) if want_logits else None
        feature = torch.empty((B, T, FEATURE_DIM), dtype=torch.float32, device=h.device) if want_feature else None
        if B:
            n = ctypes.c_size_t()
            _lib.check(h.lib.mi355asr_punc_heads_workspace_bytes(h.ptr, B, T, ctypes.byref(n)))
            ws = h.workspace(n.value) if n.value else None
            with torch.cuda.device(h.device):
                _lib.check(h.lib.mi355asr_punc_heads(h.ptr, _p(x), _p(ln), B, T, _p(logits), _p(feature), _p(ws), n.value, h._stream()))
        return logits, feature

    def probs(self, ids, lengths=None):
        """-> device tensor [B, T, classes]"""
        return self.forward(ids, lengths, want_decisions=False)[0]

    # ---- the reference's rule ------------------------------------------------------------------------------------------------
    def encode(self, txt):
        """[<S>] + characters + [</S>]; KeyError on a character outside the punctuation vocabulary"""
        v = self.vocab_featurizer
        return [v.startid()] + v.extract(txt) + [v.endid()]

    def decisions(self, ids_list):
        """token lists -> per list (argmax class, its probability) of every token, one launch for all"""
        if not ids_list:
            return []
        T = max(len(x) for x in ids_list)
        ids = np.zeros((len(ids_list), T), np.int32)
        for r, x in enumerate(ids_list):
            ids[r, :len(x)] = x
        _, cls, pmax = self.forward(ids, [len(x) for x in ids_list])
        cls, pmax = cls.cpu().numpy(), pmax.cpu().numpy()
        return [(cls[r, :len(x)], pmax[r, :len(x)]) for r, x in enumerate(ids_list)]

    def punc_recover_batch(self, texts):
        """`punc_recover` of every text, one launch for all of them -> list of lists"""
        texts = list(texts)
        ids, rows = [], []
        out = [None] * len(texts)
        for i, txt in enumerate(texts):
            try:
                ids.append(self.encode(txt))
                rows.append(i)
            except KeyError:
                if self.on_unknown == "raise":
                    raise
                out[i] = list(txt)
        for i, (cls, pmax) in zip(rows, self.decisions(ids)):
            out[i] = apply_rule(texts[i], cls[1:-1], pmax[1:-1], self.bd_featurizer.vocab_array)
        return out

    def punc_recover(self, txt):
        """The reference's rule exactly: the text between <S> and </S> through the model, the rows of the two markers
        dropped, and after character t the mark `bd_featurizer.vocab_array[argmax]` when argmax > 1 and max >= 0.65 ->
        list of characters and marks.

        The reference indexes `vocab_array`, not `index_to_token`: under `blank_at_zero` the class ids start at 1 but
        `vocab_array` starts at 0, so class c yields the token of class c + 1 (class 2, '</S>', would yield '，', and the
        last class has no entry: IndexError).  That is reproduced; `forward` returns the classes themselves for callers
        that map them differently."""
        return self.punc_recover_batch([txt])[0]

    __call__ = punc_recover
