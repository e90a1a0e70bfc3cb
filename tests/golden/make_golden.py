"""Generates the committed golden fixtures.  Runs ONLY in the build container, where
/root/reference exists (it does not exist on the GPU box; nothing at test time reads it).

  python tests/golden/make_golden.py

Outputs (all under tests/golden/):
  ctc_decoder_weights.npz  trained CTCDecoder weights pulled out of the reference's exported
                           graph Inference/PythonInference/asr/models/offline/ctc_model.onnx,
                           renamed to the Keras layout/names used by oracle/conformer_oracle.py
  ctc_decoder_io.npz       inputs + the logits the reference graph itself produces for them
                           (executed by oracle/onnx_mini.py), used to pin the oracle
  greedy_kat.json          known-answer tests produced by the reference's C++
                           ctc_greedy_decoder.h (compiled by oracle/Makefile into oracle/_ref)
  beam_kat.npz             known-answer tests produced by the reference's scorer-less prefix beam search
                           (externals/ctc_decoders.zip compiled by oracle/Makefile target ref_beam)
  ctc_model_graph.onnx     ctc_model.onnx without the weight payloads that ctc_decoder_weights.npz holds:
                           rebuild_ctc_model() puts them back, byte for byte
  standin_greedy_kat.json  the reference's C++ greedy decoder on the blank-heavy batches of
                           tests/test_tfshim.py::test_standin_ctc_decode_equals_the_reference_cpp_greedy_decoder

  python tests/golden/make_golden.py standin_greedy_kat      (one fixture only: the make_<name> generator)
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import onnx_mini  # noqa: E402

REF = "/root/reference"
ONNX = REF + "/Inference/PythonInference/asr/models/offline/ctc_model.onnx"
OUT = os.path.join(ROOT, "tests", "golden")
H, HS, D = 4, 36, 144


def extract_weights(inits):
    blk = "decoder_conformer_block_0"
    g = lambda n: np.array(inits[n], dtype=np.float32)
    w = {}
    w["project/kernel"] = g("dense_53/Tensordot/ReadVariableOp:0")
    w["project/bias"] = g("dense_53/BiasAdd/ReadVariableOp:0")

    def ln(dst, idx, sub):
        base = "%s/%slayer_normalization_%d" % (blk, sub, idx)
        w[dst + "/gamma"] = g(base + "/mul_3/ReadVariableOp:0")
        w[dst + "/beta"] = g(base + "/add/ReadVariableOp:0")

    ln(blk + "/ff_module_1/ln", 65, "ff_module_1/")
    ln(blk + "/mhsa_module/ln", 66, "mhsa_module/")
    ln(blk + "/conv_module/ln", 67, "conv_module/")
    ln(blk + "/ff_module_2/ln", 68, "ff_module_2/")
    ln(blk + "/ln", 69, "")
    for ff, a, b in (("ff_module_1", 54, 55), ("ff_module_2", 56, 57)):
        w["%s/%s/ffn1/kernel" % (blk, ff)] = g("%s/%s/dense_%d/Tensordot/ReadVariableOp:0" % (blk, ff, a))
        w["%s/%s/ffn1/bias" % (blk, ff)] = g("%s/%s/dense_%d/BiasAdd/ReadVariableOp:0" % (blk, ff, a))
        w["%s/%s/ffn2/kernel" % (blk, ff)] = g("%s/%s/dense_%d/Tensordot/ReadVariableOp:0" % (blk, ff, b))
        w["%s/%s/ffn2/bias" % (blk, ff)] = g("%s/%s/dense_%d/BiasAdd/ReadVariableOp:0" % (blk, ff, b))
    # MHA: tf2onnx folded einsum "BNI,HIO->BNHO" into Gemm(transB=1) with W[h*hs+o, i] = kernel[h,i,o].
    # Roles established by tracing the graph (the Gemm whose output is multiplied by truediv_recip
    # is the query; the one MatMul'ed against it is the key; the remaining one the value).
    m = blk + "/mhsa_module/mha"
    for nm, const in (("query_kernel", "const_fold_opt__9843"), ("key_kernel", "const_fold_opt__9837"),
                      ("value_kernel", "const_fold_opt__9842")):
        w[m + "/" + nm] = np.ascontiguousarray(g(const).reshape(H, HS, D).transpose(0, 2, 1))
    # projection: const [1,1,O,H,I] ; projection_kernel[h,i,o]
    w[m + "/projection_kernel"] = np.ascontiguousarray(g("const_fold_opt__9840")[0, 0].transpose(1, 2, 0))
    w[m + "/projection_bias"] = g(blk + "/mhsa_module/multi_head_attention_13/add/ReadVariableOp:0")
    c = blk + "/conv_module"
    w[c + "/pw_conv_1/kernel"] = np.ascontiguousarray(g(c + "/pw_conv_1/conv1d/ExpandDims_1:0")[:, :, 0, 0].T[None])
    w[c + "/pw_conv_1/bias"] = g("const_fold_opt__9530").reshape(-1)
    w[c + "/dw_conv/depthwise_kernel"] = np.ascontiguousarray(g("const_fold_opt__9512")[:, 0, 0, :].T[:, :, None])
    w[c + "/dw_conv/pointwise_kernel"] = np.ascontiguousarray(g(c + "/dw_conv/ExpandDims_2:0")[:, :, 0, 0].T[None])
    w[c + "/dw_conv/bias"] = g(c + "/dw_conv/BiasAdd/ReadVariableOp:0")
    # BatchNorm arrives folded (mul, shift). Express as Keras params with mean 0, var 1-eps so
    # gamma*(x-0)/sqrt(var+eps)+beta == scale*x+shift.
    scale = g(c + "/batch_normalization_13/batchnorm/mul:0").reshape(-1)
    shift = g("const_fold_opt__9544").reshape(-1)
    w[c + "/bn/gamma"] = scale
    w[c + "/bn/beta"] = shift
    w[c + "/bn/moving_mean"] = np.zeros_like(scale)
    w[c + "/bn/moving_variance"] = np.full_like(scale, 1.0 - 1e-3)
    w[c + "/pw_conv_2/kernel"] = np.ascontiguousarray(g(c + "/pw_conv_2/conv1d/ExpandDims_1:0")[:, :, 0, 0].T[None])
    w[c + "/pw_conv_2/bias"] = g("const_fold_opt__9516").reshape(-1)
    w["fully_connected/kernel"] = g("fully_connected/Tensordot/ReadVariableOp:0")
    w["fully_connected/bias"] = g("fully_connected/BiasAdd/ReadVariableOp:0")
    return w


def make_onnx_fixtures():
    nodes, inits, gin, gout = onnx_mini.load(ONNX)
    w = extract_weights(inits)
    np.savez_compressed(os.path.join(OUT, "ctc_decoder_weights.npz"), **w)
    rng = np.random.default_rng(0)
    xa = rng.standard_normal((2, 50, D)).astype(np.float32)
    xb = (2.0 * rng.standard_normal((1, 250, D))).astype(np.float32)
    ya = onnx_mini.run(nodes, inits, {gin[0]: xa}, gout)[0]
    yb = onnx_mini.run(nodes, inits, {gin[0]: xb}, gout)[0]
    zb = yb.astype(np.float64)
    lse = np.log(np.exp(zb - zb.max(-1, keepdims=True)).sum(-1)) + zb.max(-1)
    np.savez_compressed(os.path.join(OUT, "ctc_decoder_io.npz"),
                        x_a=xa, logits_a=ya.astype(np.float32),
                        x_b=xb, argmax_b=yb.argmax(-1).astype(np.int32),
                        max_b=yb.max(-1).astype(np.float32), lse_b=lse.astype(np.float32),
                        logits_b_every8=yb[:, ::8].astype(np.float32))
    print("onnx fixtures: logits_a", ya.shape, "mean %.3f std %.3f" % (ya.mean(), ya.std()),
          "| blank share b: %.2f" % (yb.argmax(-1) == 1331).mean())


# ---- ctc_model_graph.onnx: the export minus the payload ctc_decoder_weights.npz already holds -----------------------------
# Fields are copied as the file encodes them; only the length prefixes of the edited messages are written anew (minimal varints,
# as protobuf writes them), so stripping and refilling the raw_data of an initializer gives back the original bytes.
def _enc_varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _spans(buf):
    """[(field number, value start, end, start)] of one message, in file order"""
    out, pos = [], 0
    while pos < len(buf):
        start = pos
        key, pos = onnx_mini._varint(buf, pos)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            vs = pos
            _, pos = onnx_mini._varint(buf, pos)
        elif wt == 2:
            ln, vs = onnx_mini._varint(buf, pos)
            pos = vs + ln
        elif wt in (1, 5):
            vs, pos = pos, pos + (8 if wt == 1 else 4)
        else:
            raise ValueError("unsupported wire type %d" % wt)
        out.append((fno, vs, pos, start))
    return out


def _field(fno, payload):
    return _enc_varint(fno << 3 | 2) + _enc_varint(len(payload)) + bytes(payload)


def _tensor_header(buf):
    """TensorProto -> (name, dims, data type, has data)"""
    name, dims, dtype, has = "", [], 1, False
    for fno, vs, e, st in _spans(buf):
        if fno == 1:
            if buf[st] & 7 == 2:
                dims += onnx_mini._packed_varints(buf[vs:e])
            else:
                dims.append(onnx_mini._signed(onnx_mini._varint(buf, vs)[0]))
        elif fno == 2:
            dtype = onnx_mini._varint(buf, vs)[0]
        elif fno == 8:
            name = bytes(buf[vs:e]).decode()
        elif fno in (4, 5, 7, 9, 10, 11):
            has = True
    return name, dims, dtype, has


def _edit_initializers(model, edit):
    """model bytes with every initializer TensorProto replaced by edit(tensor bytes)"""
    model, out = memoryview(model), bytearray()
    for fno, vs, e, st in _spans(model):
        if fno != 7:
            out += model[st:e]
            continue
        graph, g = model[vs:e], bytearray()
        for f2, vs2, e2, st2 in _spans(graph):
            g += _field(5, edit(graph[vs2:e2])) if f2 == 5 else graph[st2:e2]
        out += _field(7, g)
    return bytes(out)


def _weight_sources(shapes):
    """shapes {initializer name: dims} of the initializers to trace -> {weight key: int64 array of 1-based positions in the
    concatenation of those initializers (file order), 0 where the weight element comes from none of them}.  extract_weights
    runs on marker values (each element its position, exact in float32 below 2^24); every other initializer reads as NaN."""
    markers, pos = {}, 1
    for name, dims in shapes.items():
        n = int(np.prod(dims))
        markers[name] = np.arange(pos, pos + n, dtype=np.float64).reshape(dims)
        pos += n
    assert pos < 1 << 24
    return markers, pos - 1


def _trace(markers, others):
    inits = dict(others)
    inits.update(markers)
    out = {}
    for k, v in extract_weights(inits).items():
        v = np.asarray(v, np.float64).ravel()
        ok = np.isfinite(v) & (v >= 1) & (v == np.round(v))
        out[k] = np.where(ok, v, 0).astype(np.int64)
    return out


def rebuild_ctc_model(graph_path, weights):
    """ctc_model_graph.onnx + the CTCDecoder weights (ctc_decoder_weights.npz) -> the bytes of the reference's ctc_model.onnx"""
    with open(graph_path, "rb") as f:
        model = f.read()
    headers = []
    _edit_initializers(model, lambda t: headers.append(_tensor_header(t)) or t)
    empty = {n: d for n, d, dt, has in headers if not has and int(np.prod(d)) > 0}
    assert all(dt == 1 for n, d, dt, has in headers if n in empty), "only float32 payloads are stripped"
    others = {n: np.full(d, np.nan) for n, d, dt, has in headers if n not in empty}
    markers, total = _weight_sources(empty)
    flat = np.full(total + 1, np.nan, np.float32)
    for k, src in _trace(markers, others).items():
        sel = src > 0
        flat[src[sel]] = np.asarray(weights[k], np.float32).ravel()[sel]
    assert not np.isnan(flat[1:]).any(), "a stripped initializer element has no source in the weights"
    payload, pos = {}, 1
    for name, d in empty.items():
        n = int(np.prod(d))
        payload[name] = flat[pos:pos + n].astype("<f4").tobytes()
        pos += n

    def refill(t):
        name = _tensor_header(t)[0]
        if name not in payload:
            return t
        t, out, done = memoryview(t), bytearray(), False
        for fno, vs, e, st in _spans(t):
            if fno > 9 and not done:
                out += _field(9, payload[name])
                done = True
            out += t[st:e]
        return bytes(out) if done else bytes(out) + _field(9, payload[name])
    return _edit_initializers(model, refill)


def make_ctc_model_graph():
    """ctc_model_graph.onnx: the export with the raw_data of every float32 initializer whose elements all reach
    ctc_decoder_weights.npz through extract_weights removed; checked to rebuild byte for byte"""
    import hashlib
    with open(ONNX, "rb") as f:
        model = f.read()
    headers = []
    _edit_initializers(model, lambda t: headers.append(_tensor_header(t)) or t)
    _, inits, _, _ = onnx_mini.load(ONNX)
    floats = {n: d for n, d, dt, has in headers if dt == 1 and has and int(np.prod(d)) > 1}
    markers, total = _weight_sources(floats)
    seen = np.zeros(total + 1, bool)
    for src in _trace(markers, {n: np.full(np.shape(a), np.nan) for n, a in inits.items() if n not in floats}).values():
        seen[src] = True
    strip, pos = set(), 1
    for name, d in floats.items():
        n = int(np.prod(d))
        if seen[pos:pos + n].all():
            strip.add(name)
        pos += n

    def drop(t):
        if _tensor_header(t)[0] not in strip:
            return t
        t = memoryview(t)
        return b"".join(bytes(t[st:e]) for fno, vs, e, st in _spans(t) if fno != 9)
    out = os.path.join(OUT, "ctc_model_graph.onnx")
    with open(out, "wb") as f:
        f.write(_edit_initializers(model, drop))
    w = dict(np.load(os.path.join(OUT, "ctc_decoder_weights.npz")))
    assert rebuild_ctc_model(out, w) == model, "the stripped export does not rebuild byte for byte"
    print("ctc_model_graph.onnx: %d of %d initializers stripped, %d -> %d bytes, sha256 %s" % (
        len(strip), len(headers), len(model), os.path.getsize(out), hashlib.sha256(model).hexdigest()))


def make_greedy_kats():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_ctc_greedy.so"))
    lib.ref_ctc_greedy.restype = ctypes.c_int
    lib.ref_ctc_greedy.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int)]
    rng = np.random.default_rng(7)
    kats = []
    shapes = [(6, 4), (1, 3), (17, 5), (40, 8), (64, 1332), (250, 1332), (3, 2), (12, 6)]
    for T, V in shapes:
        for variant in range(3):
            blank = V - 1
            if variant == 0:        # generic random probabilities
                p = rng.random((T, V)).astype(np.float32)
            elif variant == 1:      # quantised -> many exact ties (first max must win) and repeats
                p = (rng.integers(0, 3, (T, V)) / 2.0).astype(np.float32)
            else:                   # blank-dominated with runs of repeated labels
                ids = np.repeat(rng.integers(0, V, (T + 2) // 3), 3)[:T]
                ids[rng.random(T) < 0.5] = blank
                p = np.full((T, V), 0.01, np.float32)
                p[np.arange(T), ids] = 0.9
            out = (ctypes.c_int * T)()
            n = lib.ref_ctc_greedy(p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), T, V, blank, out)
            kat = {"T": T, "V": V, "blank": blank, "expect": [int(out[i]) for i in range(n)]}
            if V <= 8:
                kat["probs"] = [[float(v) for v in row] for row in p]
            else:               # large cases: store the per-frame argmax instead of the matrix
                kat["frame_argmax"] = [int(v) for v in p.argmax(-1)]
                kat["seeded"] = False
            kats.append(kat)
    # the survey's hand KAT: rows argmax [1,1,3,1,0,tie->0], blank 3 -> [1,1,0]
    p = np.array([[0, 1, 0, 0], [0, .9, 0, 0], [0, 0, 0, 1], [0, 1, 0, 0], [1, 0, 0, 0], [.5, .5, 0, 0]], np.float32)
    out = (ctypes.c_int * 6)()
    n = lib.ref_ctc_greedy(p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 6, 4, 3, out)
    kats.append({"T": 6, "V": 4, "blank": 3, "expect": [int(out[i]) for i in range(n)],
                 "probs": [[float(v) for v in row] for row in p]})
    with open(os.path.join(OUT, "greedy_kat.json"), "w") as f:
        json.dump(kats, f)
    print("greedy KATs:", len(kats), "hand KAT ->", kats[-1]["expect"])


def standin_greedy_batches():
    """(T, V, lens, probabilities (3, T, V) float32) of the stand-in greedy test, in its order; the test rebuilds them from the
    same seed"""
    rng = np.random.default_rng(3)
    for T, V in ((1, 3), (7, 4), (60, 12), (250, 1332)):
        B = 3
        logits = rng.standard_normal((B, T, V)).astype(np.float32) * 3
        logits[:, :, -1] += 2.0                                   # blank-heavy, like a trained CTC model
        logits[0, T // 2] = logits[0, T // 2].max()               # a frame of exact ties: first index wins on both sides
        p = np.exp(logits - logits.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        yield T, V, np.array([T, max(1, T - 2), max(1, T // 2)], np.int32), p


def make_standin_greedy_kat():
    """the reference's C++ greedy decoder on log(p + 1e-7) (test_asr.py:167-185 / asr.py:41-61 feed it that) for every row of
    standin_greedy_batches(): {"T,V": [ids of row 0, row 1, row 2]}"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_ctc_greedy.so"))
    fn = lib.ref_ctc_greedy
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    kat = {}
    for T, V, lens, p in standin_greedy_batches():
        rows = []
        for b in range(p.shape[0]):
            lp = np.ascontiguousarray(np.log(p[b, :lens[b]] + 1e-7), np.float32)
            out = np.zeros(T + 1, np.int32)
            n = fn(lp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(lens[b]), V, V - 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
            rows.append(out[:n].tolist())
        kat["%d,%d" % (T, V)] = rows
    with open(os.path.join(OUT, "standin_greedy_kat.json"), "w") as f:
        json.dump(kat, f)
    print("standin_greedy_kat.json:", {k: [len(r) for r in v] for k, v in kat.items()})


def make_beam_kats():
    """Known-answer tests from the reference's own prefix beam search (scorer-less), oracle/_ref/libref_ctc_beam.so."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref_beam"])
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_ctc_beam.so"))
    lib.ref_ctc_beam_search.restype = ctypes.c_int
    lib.ref_ctc_beam_search.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    rng = np.random.default_rng(11)
    cases = [(6, 4, 3, 1.0, 40, 1.0), (20, 8, 5, 1.0, 40, 1.0), (30, 12, 10, 0.99, 5, 1.0), (50, 30, 8, 0.9, 10, 3.0),
             (40, 60, 20, 1.0, 40, 2.0), (100, 200, 10, 0.999, 40, 4.0), (25, 6, 4, 0.5, 3, 1.0), (15, 5, 100, 1.0, 40, 1.0),
             (1, 7, 4, 1.0, 40, 1.0), (60, 1332, 10, 0.99, 40, 6.0), (250, 1332, 4, 0.999, 40, 8.0)]
    out = {}
    meta = []
    for k, (T, V, beam, cp, tn, temp) in enumerate(cases):
        z = rng.standard_normal((T, V)) * temp
        z[:, -1] += 1.0                                   # blank-leaning, like a CTC model
        p = np.exp(z - z.max(-1, keepdims=True))
        p = (p / p.sum(-1, keepdims=True)).astype(np.float32)   # float32-representable probabilities
        pd = np.ascontiguousarray(p, np.float64)
        sc = (ctypes.c_double * beam)()
        ids = (ctypes.c_int * (beam * T))()
        ln = (ctypes.c_int * beam)()
        n = lib.ref_ctc_beam_search(pd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, V, beam, cp, tn, T, sc, ids, ln)
        e_ids = np.full((n, T), -1, np.int32)
        for i in range(n):
            e_ids[i, :ln[i]] = [ids[i * T + j] for j in range(ln[i])]
        out["probs_%d" % k] = p
        out["ids_%d" % k] = e_ids
        out["lens_%d" % k] = np.array([ln[i] for i in range(n)], np.int32)
        out["scores_%d" % k] = np.array([sc[i] for i in range(n)], np.float64)
        meta.append({"T": T, "V": V, "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "n": n})
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "beam_kat.npz"), **out)
    print("beam KATs:", len(meta), "cases; best of the last:", out["ids_%d" % (len(cases) - 1)][0][:out["lens_%d" % (len(cases) - 1)][0]][:10])


def make_long_beam_kats():
    """The reference's own decoder on LONG inputs (hundreds of frames, scores of -1000 and below, where a float32 ulp is
    1e-4 and hypotheses tie in score all the time): beam_long_kat.npz.  prefix_compare orders by (score, last character)
    only and the reference leaves the rest to std::nth_element over its DFS-ordered vector, so these vectors pin what IS
    specified -- the ranked float32 scores, bit for bit -- and record how many hypotheses coincide beyond that."""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_ctc_beam.so"))
    lib.ref_ctc_beam_search.restype = ctypes.c_int
    lib.ref_ctc_beam_search.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    rng = np.random.default_rng(2024)
    cases = [(500, 120, 10, 0.99, 40, 0.05), (500, 120, 100, 0.99, 40, 1.0), (400, 200, 25, 0.9999, 25, 0.3), (600, 96, 10, 0.99, 40, 2.5)]
    out, meta = {}, []
    for k, (T, V, beam, cp, tn, temp) in enumerate(cases):
        z = rng.standard_normal((T, V)) * temp
        p = np.exp(z - z.max(-1, keepdims=True))
        p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
        pd = np.ascontiguousarray(p, np.float64)
        sc = (ctypes.c_double * beam)()
        ids = (ctypes.c_int * (beam * T))()
        ln = (ctypes.c_int * beam)()
        n = lib.ref_ctc_beam_search(pd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), T, V, beam, cp, tn, T, sc, ids, ln)
        lens = np.array([ln[i] for i in range(n)], np.int32)
        e_ids = np.full((n, int(lens.max()) if n else 0), -1, np.int32)
        for i in range(n):
            e_ids[i, :ln[i]] = [ids[i * T + j] for j in range(ln[i])]
        out["probs_%d" % k] = p
        out["ids_%d" % k] = e_ids
        out["lens_%d" % k] = lens
        out["scores_%d" % k] = np.array([sc[i] for i in range(n)], np.float64)
        meta.append({"T": T, "V": V, "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "n": n})
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "beam_long_kat.npz"), **out)
    print("long beam KATs:", len(meta), "cases")


def make_stateful_beam_kats():
    """The reference's stateful BeamDecoder (ctc_beam_search_decoder.cpp:217-405) fed in pieces, with a reset in
    between: the beam after every decode() call."""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_ctc_beam.so"))
    lib.ref_beam_decoder_new.restype = ctypes.c_void_p
    lib.ref_beam_decoder_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    lib.ref_beam_decoder_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ref_beam_decoder_reset.argtypes = [ctypes.c_void_p]
    lib.ref_beam_decoder_free.argtypes = [ctypes.c_void_p]
    rng = np.random.default_rng(99)
    out = {}
    cases = [(9, 6, 1.0, 40, [5, 1, 7, 4]), (30, 10, 0.99, 8, [13, 12]), (5, 3, 0.9, 3, [1, 1, 1, 1, 9]),
             (1332, 10, 0.99, 40, [20, 11, 19])]
    for ci, (V, beam, cp, ctn, pieces) in enumerate(cases):
        T = sum(pieces)
        sharp = 4.0 if V > 100 else 1.5
        x = rng.standard_normal((2, T, V)) * sharp
        x[..., V - 1] += 2.0                                   # blank-heavy, like a trained CTC model
        p = np.exp(x - x.max(-1, keepdims=True))
        p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
        h = lib.ref_beam_decoder_new(V, beam, cp, ctn)
        res = []
        for u in range(2):                                     # second utterance after reset()
            if u:
                lib.ref_beam_decoder_reset(h)
            o = 0
            for n in pieces:
                pd = np.ascontiguousarray(p[u, o:o + n], np.float64)
                o += n
                sc = np.zeros(beam)
                ids = -np.ones((beam, T), np.int32)
                ln = np.zeros(beam, np.int32)
                k = lib.ref_beam_decoder_decode(h, pd.ctypes.data, n, V, T, sc.ctypes.data, ids.ctypes.data, ln.ctypes.data)
                res.append((k, sc.astype(np.float32), ids, ln))
        lib.ref_beam_decoder_free(h)
        out["c%d_meta" % ci] = np.array([V, beam, ctn, len(pieces)], np.int32)
        out["c%d_cp" % ci] = np.array([cp])
        out["c%d_pieces" % ci] = np.array(pieces, np.int32)
        out["c%d_probs" % ci] = p
        out["c%d_n" % ci] = np.array([r[0] for r in res], np.int32)
        out["c%d_scores" % ci] = np.stack([r[1] for r in res])
        out["c%d_ids" % ci] = np.stack([r[2] for r in res])
        out["c%d_lens" % ci] = np.stack([r[3] for r in res])
    np.savez_compressed(os.path.join(OUT, "beam_stateful_kat.npz"), **out)
    print("beam_stateful_kat.npz:", len(cases), "cases")


def make_wer_kats():
    """(S+I+D)/N and the S / D / I split from the reference's own utils/xer.py (numpy-only, importable here)."""
    from utils import xer
    rng = np.random.default_rng(7)
    kats = []
    for n in range(60):
        lr, lh = int(rng.integers(1, 14)), int(rng.integers(0, 14))
        r = rng.integers(0, 6, lr).tolist()
        h = rng.integers(0, 6, lh).tolist()
        if n % 5 == 0:
            h = list(r)
        if n % 7 == 0 and len(r) > 2:
            h = r[1:] + [9]
        score, s, d, i = xer.wer(r, h)
        kats.append({"r": r, "h": h, "score": score, "s": s, "d": d, "i": i})
    json.dump(kats, open(os.path.join(OUT, "wer_kat.json"), "w"))
    print("wer_kat.json:", len(kats), "cases")


if __name__ == "__main__":
    sys.path.insert(0, REF)
    if len(sys.argv) > 1:
        for name in sys.argv[1:]:
            globals()["make_" + name]()
        sys.exit(0)
    make_wer_kats()
    make_stateful_beam_kats()
    make_onnx_fixtures()
    make_ctc_model_graph()
    make_greedy_kats()
    make_beam_kats()
    make_long_beam_kats()
