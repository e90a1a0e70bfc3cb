"""The GPU steps of tests/test_gpu_caller_contract.py, one per process: `python tests/caller_contract_gpu_steps.py STEP`.

The caller contract of include/mi355asr.h ("Conventions"), pinned entry point by entry point:

  R0  the call on a fresh handle state (no workspace yet, new opaque state) under `fenced(0x00)` (tests/fence.py): every
      workspace, opaque state and output the wrapper allocates holds zeros and sits between two guards
  RF  the same under `fenced(0xFF)`: every float word a NaN, every int32 -1
  RS  no fence: on the same handle first a LARGER call of the same entry point on other data, then the case's call on the
      grown, dirty workspace (stateful families: after their reset, or on a new state object)

and then: (1) everything the wrapper returns, and every raw output tensor the fence recorded, is bit-identical in the three
runs (raw outputs: R0 against RF, over the region the header defines); (2) no guard byte was written, and the workspace was
allocated by the call with exactly the bytes `*_workspace_bytes` answered; (3) R0 is within the family's existing bound of
its existing reference (the float64 oracle at 1e-3, ctc_yardstick.bound, the resampler's bound, net64 at 1e-4, the host
search bit for bit), so the three equal results are anchored to something other than each other.

The stream steps use no fence: they run every family on a side stream behind a long delay and two handles at once, and
compare with the default-stream / sequential result bit for bit.

A step prints what it ran, collects every finding, and exits non-zero if there is one; it is never repeated."""
import ctypes
import os
import sys
import threading
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from fence import fenced                                               # noqa: E402
from helpers import GOLDEN, assert_frames_and_ids, co, encoder_kwargs, maxdiff, small_cfg, waves   # noqa: E402
from tensorflowasr_amd import _lib                                     # noqa: E402

TOL = 1e-3                                                             # the project's contract against the float64 oracle
FINDINGS = []


def finding(msg):
    print("FINDING: " + msg)
    FINDINGS.append(msg)


# ---- the three runs ------------------------------------------------------------------------------------------------------
def flat(r, path="out"):
    """whatever a wrapper returns -> [(path, NumPy array)]; device tensors are copied to the host"""
    if r is None:
        return []
    if torch.is_tensor(r):
        return [(path, r.detach().cpu().contiguous().numpy().copy())]
    if isinstance(r, np.ndarray):
        return [(path, r.copy())]
    if isinstance(r, dict):
        out = []
        for k in sorted(r, key=str):
            if not str(k).startswith("_"):
                out += flat(r[k], "%s[%r]" % (path, k))
        return out
    if isinstance(r, (list, tuple)):
        out = []
        for i, v in enumerate(r):
            out += flat(v, "%s[%d]" % (path, i))
        return out
    if isinstance(r, (int, float, bool, np.integer, np.floating, str)):
        return [(path, np.asarray(r))]
    raise TypeError("%s: %r" % (path, type(r)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8) if a.dtype.kind != "U" else a


def where_differs(a, b):
    """a short description of where two equally shaped arrays differ bit for bit"""
    wa = a.reshape(-1).view("u%d" % a.dtype.itemsize) if a.dtype.kind in "fiu" else a.reshape(-1)
    wb = b.reshape(-1).view("u%d" % b.dtype.itemsize) if b.dtype.kind in "fiu" else b.reshape(-1)
    bad = np.flatnonzero(wa != wb)
    idx = np.unravel_index(bad[[0, -1]], a.shape) if a.ndim else ((0, 0),)
    first, last = tuple(int(i[0]) for i in idx), tuple(int(i[1]) for i in idx)
    return "%d of %d words, first at %s (%r / %r), last at %s" % (len(bad), wa.size, first, a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]], last)


def same(name, what, x, y, tags, defined=None):
    """x, y: [(path, array)] of two runs; defined: {key: boolean mask of the region that is defined}, or a function of x that
    returns one; a key is a substring of the path, or -- raw outputs -- "<index among the raw tensors>: " """
    masks = (defined(x) if callable(defined) else defined) or {}
    if [p for p, _ in x] != [p for p, _ in y]:
        return finding("%s: %s of %s and %s have different structure: %s / %s" % (name, what, tags[0], tags[1], [p for p, _ in x], [p for p, _ in y]))
    for (pa, a), (_, b) in zip(x, y):
        if a.shape != b.shape or a.dtype != b.dtype:
            finding("%s: %s %s: %s %s in %s, %s %s in %s" % (name, what, pa, a.shape, a.dtype, tags[0], b.shape, b.dtype, tags[1]))
            continue
        m = None
        for key, mask in masks.items():
            if pa.startswith(key) if key[0].isdigit() else key in pa:
                m = mask
        if m is not None:
            m = np.broadcast_to(m, a.shape)
            a, b = np.where(m, a, np.zeros((), a.dtype)), np.where(m, b, np.zeros((), b.dtype))
        if a.size and not np.array_equal(bits(a), bits(b)):
            finding("%s: %s %s differs between %s and %s: %s" % (name, what, pa, tags[0], tags[1], where_differs(a, b)))


def snapshot(f):
    """the raw non-workspace tensors a fence handed out, in order, and the sizes of the byte buffers (workspaces, opaque state)"""
    raws = [("%d: %s" % (i, a.site), a.tensor.detach().cpu().numpy().copy())
            for i, a in enumerate(al for al in f.allocations if al.tensor.dtype != torch.uint8)]
    return raws, [int(a.tensor.numel()) for a in f.allocations if a.tensor.dtype == torch.uint8]


def three_runs(name, call, ws_bytes=None, defined=None, raw_defined=None, any_byte_buffers=False):
    """call(stale) -> what the wrapper returns.  stale False: the call must start from a fresh handle state (drop the handle's
    workspace, make new opaque state); stale True: it first makes a larger call of the same entry point on other data, then the
    case's call on the dirty workspace.  ws_bytes: the sizes `*_workspace_bytes` (and `*_bytes` of opaque state) answer for
    the case, each of which must be the numel of a byte buffer the call allocated.  -> R0 (as `flat` gives it)"""
    got = {}
    for tag, fill in (("R0", 0x00), ("RF", 0xFF)):
        with fenced(fill) as f:
            r = call(False)
            torch.cuda.synchronize()
            f.check()
            raws, sizes = snapshot(f)
            got[tag] = (flat(r), raws, sizes)
    rs = call(True)
    torch.cuda.synchronize()
    got["RS"] = (flat(rs), None, None)
    same(name, "returned", got["R0"][0], got["RF"][0], ("R0", "RF"), defined)
    same(name, "returned", got["R0"][0], got["RS"][0], ("R0", "RS"), defined)
    same(name, "raw output", got["R0"][1], got["RF"][1], ("R0", "RF"), raw_defined)
    sizes = got["RF"][2]
    if ws_bytes is not None:
        want = [int(v) for v in (ws_bytes() if callable(ws_bytes) else ws_bytes)]
        left = list(sizes)
        for v in want:
            if v in left:
                left.remove(v)
            else:
                finding("%s: no byte buffer of exactly %d bytes was allocated by the call (allocated: %s)" % (name, v, sizes))
        if left:
            finding("%s: byte buffers %s were allocated beside the ones the size queries answer (%s)" % (name, left, want))
    elif sizes and not any_byte_buffers:
        finding("%s: byte buffers %s allocated, none expected" % (name, sizes))
    nan = [p for p, a in got["RF"][0] if a.dtype.kind == "f" and np.isnan(a).any() and not np.isnan(dict(got["R0"][0])[p]).any()]
    if nan:
        finding("%s: NaN of the 0xFF fill in %s" % (name, nan))
    print("  %-58s R0 = RF = RS over %d returned and %d raw tensors; guards of %d allocations intact; byte buffers %s"
          % (name, len(got["R0"][0]), len(got["R0"][1]), len(got["RF"][1]) + len(sizes), sizes))
    return got["R0"][0]


def first(r0, key="out"):
    for p, a in r0:
        if p == key:
            return a
    raise KeyError("%s not in %s" % (key, [p for p, _ in r0]))


def within(name, got, ref, tol=TOL):
    err = maxdiff(got, ref)
    print("  %-58s max|R0 - reference| = %.3g (bound %.3g)" % (name, err, tol))
    if not err < tol:
        finding("%s: R0 is %.3g from its reference, above %.3g" % (name, err, tol))


def size_t_of(fn, *args):
    n = ctypes.c_size_t()
    _lib.check(fn(*args, ctypes.byref(n)))
    return int(n.value)


def profile_counts(h, fn):
    """launch counts per MI355ASR_K_* category of one call made with profiling on (outside the compared runs)"""
    nk = 20
    ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    _lib.check(h.lib.mi355asr_profile_enable(h.ptr, 1))
    _lib.check(h.lib.mi355asr_profile_read(h.ptr, ms, cnt, nk, 1))
    fn()
    torch.cuda.synchronize()
    _lib.check(h.lib.mi355asr_profile_read(h.ptr, ms, cnt, nk, 1))
    _lib.check(h.lib.mi355asr_profile_enable(h.ptr, 0))
    return [int(c) for c in cnt]


K_FFN, K_ATTN, K_DWCONV, K_FF1_QKV, K_OUT_GLU, K_TAIL_FF2, K_TAIL_FF1, K_ENC_STACK = 5, 7, 10, 15, 16, 17, 18, 19


def nan_tail(x, lens):
    """the rows past each length hold NaN: never read"""
    x = np.array(x, np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    return x


# ---- dmodel 144: ConformerCTC -----------------------------------------------------------------------------------------------
# Regimes (csrc/block_path.hip): rows M = B * T.  M <= 48 (MI355ASR_SMALL_M): run_block_layers, one launch per layer;
# 48 < M <= 4096 (MI355ASR_NS1_MAX_M): the small-batch kernels of fused_ns.hip, the attention inside their first launch up to
# 256 keys (ATTN_SPLIT_SHORT_KEYS), attention_split_long_kernel in a launch of its own above; M > 4096: the pair-pipelined
# kernels of fused_pp.hip with the depthwise conv folded into the tail launch (pp_dw_fold_fits: T >= 64 and little padding).
ENC_SHAPES = [(1, 8000, "13 rows: layer-at-a-time (M <= 48)"),
              (2, 32000, "100 rows: fused_ns, attention inside the launch"),
              (1, 176000, "275 rows and 275 keys: fused_ns, long key-block attention"),
              (17, 160000, "4 250 rows: pair-pipelined fused_pp, folded depthwise conv")]
RAGGED_L, RAGGED_LENS = 48161, [48161, 20001, 33440]                   # one length equals L, one is odd


def conformer_ctc(V=50, seed=5):
    from tensorflowasr_amd.models import ConformerCTC
    cfg = small_cfg(2)
    w = dict(co.encoder_weights(cfg, seed=seed), **co.ctc_decoder_weights(cfg, V, seed=seed + 1))
    m = ConformerCTC(V, **{k: v for k, v in encoder_kwargs(cfg).items() if k != "mel_layer_type"})
    m.load_weights(w, by_name=False)
    return m, w, cfg


def drop_ws(m):
    h = m._h
    h._ws = None
    for k in ("_ids", "_lens"):
        if hasattr(m, k):
            delattr(m, k)


def step_encoder144():
    m, w, cfg = conformer_ctc()
    h = m._h
    for B, L, regime in ENC_SHAPES:
        x = waves(B, L, 7).astype(np.float32)
        big = waves(B + 1, L + 16000, 40).astype(np.float32)
        T = m.out_frames(L)
        print("%d x %d samples, T = %d, %s" % (B, L, T, regime))
        c = profile_counts(h, lambda: m.encode(x))
        M = B * T
        if M <= 48:
            assert c[K_FFN] > 0 and c[K_FF1_QKV] == 0 and c[K_TAIL_FF1] + c[K_TAIL_FF2] == 0, ("layer-at-a-time", c)
        else:
            assert c[K_FFN] == 0 and c[K_FF1_QKV] > 0 and c[K_TAIL_FF1] + c[K_TAIL_FF2] > 0, ("fused", c)
            # the launch counts are the same for fused_ns and fused_pp (both: ff1_qkv, then one tail launch per block): which of
            # the two ran follows from M and MI355ASR_NS1_MAX_M alone.  What the counts do show is the folding: no launch of
            # the depthwise conv or of out-projection + GLU on its own
            print("  launch counts: ff1_qkv %d, attention %d, out_glu %d, dwconv %d, tail_ff1 %d, tail_ff2 %d"
                  % (c[K_FF1_QKV], c[K_ATTN], c[K_OUT_GLU], c[K_DWCONV], c[K_TAIL_FF1], c[K_TAIL_FF2]))
            if M > 4096:
                assert c[K_DWCONV] == 0 and c[K_OUT_GLU] == 0 and c[K_ATTN] > 0, ("folded depthwise conv", c)
            assert (c[K_ATTN] == 0) == (M <= 4096 and T <= 256), ("attention of its own launch", c)
        ws_wave = lambda: [size_t_of(h.lib.mi355asr_workspace_bytes, h.ptr, B, L)]                          # noqa: E731
        ws_frames = lambda: [size_t_of(h.lib.mi355asr_ctc_workspace_bytes, h.ptr, B, T)]                    # noqa: E731

        def recognize(stale):
            drop_ws(m) if not stale else m.recognize(big)
            return m.recognize(x)

        def encode(stale):
            drop_ws(m) if not stale else m.encode(big)
            return m.encode(x)
        r_ids = three_runs("recognize %dx%d" % (B, L), recognize, ws_wave)
        enc = first(three_runs("encode %dx%d" % (B, L), encode, ws_wave))
        enc_big = m.encode(big)

        def logits(stale):
            drop_ws(m) if not stale else m.ctc_logits(enc_big, return_argmax=True)
            return m.ctc_logits(enc, return_argmax=True)
        r_lg = three_runs("ctc_logits(return_argmax) %dx%d" % (B, T), logits, ws_frames)
        # the oracle treats every utterance alone: of a large batch it runs the first, the middle and the last row (as
        # tests/test_gpu_baseline_shapes.py samples its batches); the bit comparisons above cover every row
        rows = list(range(B)) if B <= 4 else [0, B // 2, B - 1]
        enc_ref = co.conformer_encoder(x[rows].astype(np.float64), w, cfg)
        lg_ref = co.ctc_decoder(enc_ref, w, cfg)
        within("encode %dx%d against the float64 oracle" % (B, L), enc[rows], enc_ref)
        within("ctc_logits %dx%d against the float64 oracle" % (B, T), first(r_lg, "out[0]")[rows], lg_ref)
        assert_frames_and_ids(first(r_lg, "out[0]")[rows], first(r_lg, "out[1]")[rows], first(r_ids, "out[0]")[rows], first(r_ids, "out[1]")[rows],
                              lg_ref, [T] * len(rows), m.blank)
    # ---- the ragged entries: rows past each length hold NaN
    B, L = 3, RAGGED_L
    lens = np.array(RAGGED_LENS, np.int32)
    assert lens[0] == L and any(n % 2 for n in lens) and len(set(lens.tolist())) == 3
    x = nan_tail(waves(B, L, 11), lens)
    big = waves(B + 1, L + 16000, 50).astype(np.float32)
    big_lens = np.array([L + 16000, 30000, 12345, 55555], np.int32)
    ws_wave = lambda: [size_t_of(h.lib.mi355asr_workspace_bytes, h.ptr, B, L)]                              # noqa: E731

    def recognize(stale):
        drop_ws(m) if not stale else m.recognize(big, wav_lengths=big_lens)
        return m.recognize(x, wav_lengths=lens)

    def encode(stale):
        drop_ws(m) if not stale else m.encode(big, lengths=big_lens)
        return m.encode(x, lengths=lens)
    print("ragged %d x %d, lengths %s, NaN past each length" % (B, L, lens.tolist()))
    r_ids = three_runs("recognize(wav_lengths) ragged", recognize, ws_wave)
    r_enc = three_runs("encode(lengths) ragged", encode, ws_wave)
    enc, el = first(r_enc, "out[0]"), first(r_enc, "out[1]")
    T = enc.shape[1]
    enc_big, el_big = m.encode(big, lengths=big_lens)

    def logits(stale):
        drop_ws(m) if not stale else m.ctc_logits(enc_big, return_argmax=True, lengths=el_big)
        return m.ctc_logits(enc, return_argmax=True, lengths=el)
    r_lg = three_runs("ctc_logits(lengths) ragged", logits, lambda: [size_t_of(h.lib.mi355asr_ctc_workspace_bytes, h.ptr, B, T)])
    ids, ol = first(r_ids, "out[0]"), first(r_ids, "out[1]")
    for b, n in enumerate(lens):
        e64 = co.conformer_encoder(x[b:b + 1, :n].astype(np.float64), w, cfg)
        l64 = co.ctc_decoder(e64, w, cfg)
        Tb = e64.shape[1]
        assert el[b] == Tb
        within("ragged row %d (%d samples) encoder against the oracle on the row alone" % (b, n), enc[b:b + 1, :Tb], e64)
        within("ragged row %d logits" % b, first(r_lg, "out[0]")[b:b + 1, :Tb], l64)
        assert not enc[b, Tb:].any() and not first(r_lg, "out[0]")[b, Tb:].any() and (first(r_lg, "out[1]")[b, Tb:] == -1).all()
        rid, rlen = co.ctc_collapse(first(r_lg, "out[1]")[b:b + 1, :Tb], [Tb], m.blank)
        assert ol[b] == rlen[0] and np.array_equal(ids[b, :ol[b]], rid[0, :rlen[0]]) and (ids[b, ol[b]:] == -1).all()


def step_offline_stt_batch(tmp):
    """ASR.offline_stt_batch on a ragged batch of three (strings: compared as returned)"""
    import pathlib
    from test_gpu_vad import _asr
    asr = _asr(pathlib.Path(tmp))
    rng = np.random.default_rng(12)
    lens = RAGGED_LENS
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    big = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (70001, 64000, 12000, 33333)]
    models = [v for v in vars(asr).values() if hasattr(v, "_h")]
    assert models, "ASR holds no model with a handle"

    def call(stale):
        if stale:
            asr.offline_stt_batch(big)
        else:
            for mm in models:
                drop_ws(mm)
        return [list(t) for t in asr.offline_stt_batch(items)]
    # (several models behind one call: the workspace sizes are pinned per entry point in the other steps)
    r0 = three_runs("ASR.offline_stt_batch ragged", call, None, any_byte_buffers=True)
    want = flat([list(asr.offline_stt_wave(w)) for w in items])
    assert len(r0) == len(want) and all(pa == pb and np.array_equal(a, b) for (pa, a), (pb, b) in zip(r0, want)), (r0, want)
    print("  offline_stt_batch == [offline_stt_wave(w) for w in items]: %s" % [a.tolist() for _, a in r0])



# ---- dmodel 256, head size 64: CTCDecoder, the streaming encoder -----------------------------------------------------------
# Regimes (launch_gemm16, csrc/api.hip): a dense layer of M = B * T rows runs one gemm16 launch below ring_min_rows() = 1 500
# rows, the split-bf16 slab ring (gemm_ring.hip) from 1 500, and in the bf16 mode from 8 192 rows (MI355ASR_GEMM256_MIN_M) the
# rows-resident kernel of bf16.hip.  All three are reached through launch_gemm16 under the same profile categories, so the
# launch counts of mi355asr_profile_read cannot tell them apart: the regime of a shape follows from its row count alone.
def ctc256(mode, V=60):
    from tensorflowasr_amd.models import CTCDecoder
    cfg = dict(co.STREAMING_S, ctcdecoder_num_blocks=2)
    w = co.ctc_decoder_weights(cfg, V, seed=12)
    m = CTCDecoder(num_classes=V, dmodel=256, num_blocks=2, head_size=64, num_heads=4, kernel_size=32, fc_factor=0.5, gemm_dtype=mode)
    m.load_weights(w, by_name=False)
    return m, w, cfg


def bf16_oracle(fn):
    co.GEMM_ROUND_BF16 = True
    try:
        return fn()
    finally:
        co.GEMM_ROUND_BF16 = False


def against_bf16_oracle(name, got, ref):
    """the suite's bound for the bf16 GEMM mode (tests/test_gpu_parity.py, test_bf16_gemm_mode_against_rounding_oracle_and_fp32):
    against the oracle with both GEMM operands rounded to bf16, logits max < 4e-2 and mean < 3e-3"""
    e = np.abs(got.astype(np.float64) - ref)
    print("  %-58s bf16 rounding oracle: max %.3g (bound 4e-2), mean %.3g (bound 3e-3)" % (name, e.max(), e.mean()))
    if not (e.max() < 4e-2 and e.mean() < 3e-3):
        finding("%s: R0 is max %.3g / mean %.3g from the bf16 rounding oracle" % (name, e.max(), e.mean()))


def step_ctc256():
    rng = np.random.default_rng(1)
    models = {}
    for mode, B, T, regime in (("float32", 2, 40, "80 rows: one gemm16 launch per layer"),
                               ("float32", 6, 260, "1 560 rows: slab ring (>= 1 500)"),
                               ("bfloat16", 32, 260, "8 320 rows: rows-resident bf16 kernel (>= 8 192)")):
        if mode not in models:
            models[mode] = ctc256(mode)
        m, w, cfg = models[mode]
        h = m._h
        print("CTCDecoder 256 %s (%d, %d), %s" % (mode, B, T, regime))
        x = rng.standard_normal((B, T, 256)).astype(np.float32)
        big = rng.standard_normal((B + 1, T + 29, 256)).astype(np.float32)

        def call(stale):
            drop_ws(m) if not stale else m(big, return_argmax=True)
            return m(x, return_argmax=True)
        r = three_runs("CTCDecoder %s (%d, %d)" % (mode, B, T), call, lambda: [size_t_of(h.lib.mi355asr_ctc_workspace_bytes, h.ptr, B, T)])
        lg, am = first(r, "out[0]"), first(r, "out[1]")
        rows = list(range(B)) if B <= 6 else [0, B // 2, B - 1]
        if mode == "float32":
            within("CTCDecoder float32 (%d, %d) against the float64 oracle" % (B, T), lg[rows], co.ctc_decoder(x[rows].astype(np.float64), w, cfg))
        else:
            against_bf16_oracle("CTCDecoder bfloat16 (%d, %d)" % (B, T), lg[rows], bf16_oracle(lambda: co.ctc_decoder(x[rows].astype(np.float64), w, cfg)))
        assert np.array_equal(am, lg.argmax(-1))
    # ---- the ragged form: lengths around the tile and key-block edges, NaN past each length
    m, w, cfg = models["float32"]
    h = m._h
    B, T = 5, 289
    lens = np.array([17, 33, 272, 288, 289], np.int32)
    x = nan_tail(rng.standard_normal((B, T, 256)), lens)
    big = rng.standard_normal((B + 1, T + 30, 256)).astype(np.float32)
    big_lens = np.array([T + 30, 100, 1, 16, 257, 300], np.int32)

    def call(stale):
        drop_ws(m) if not stale else m(big, return_argmax=True, lengths=big_lens)
        return m(x, return_argmax=True, lengths=lens)
    r = three_runs("CTCDecoder float32 ragged (5, 289)", call, lambda: [size_t_of(h.lib.mi355asr_ctc_workspace_bytes, h.ptr, B, T)])
    lg, am = first(r, "out[0]"), first(r, "out[1]")
    for b, n in enumerate(lens):
        within("ragged row %d (%d frames) against the oracle on the row alone" % (b, n), lg[b:b + 1, :n], co.ctc_decoder(x[b:b + 1, :n].astype(np.float64), w, cfg))
        assert not lg[b, n:].any() and (am[b, n:] == -1).all() and np.array_equal(am[b, :n], lg[b, :n].argmax(-1))


def step_stream256():
    """StreamingConformerEncoder, 4 chunks of 8 000 samples: bf16 mode (stream256_kernel, every block of a chunk in one
    workgroup) and fp32"""
    from tensorflowasr_amd.models import StreamingConformerEncoder
    cfg = small_cfg(2, co.STREAMING_S)
    w = co.encoder_weights(cfg, seed=2)
    x = waves(1, 32000, 9).astype(np.float32)
    big = waves(2, 40000, 30).astype(np.float32)
    for mode in ("bfloat16", "float32"):
        e = StreamingConformerEncoder(**dict(encoder_kwargs(cfg), gemm_dtype=mode))
        e.add_chunk_size(8000, 80, 640)
        e.load_weights(w, by_name=False)
        h = e._h
        c = profile_counts(h, lambda: e(x))
        assert (c[K_ENC_STACK] > 0) == (mode == "bfloat16"), (mode, c)

        def call(stale):
            drop_ws(e) if not stale else e(big)
            return e(x)
        r = first(three_runs("StreamingConformerEncoder %s 4 x 8000" % mode, call, lambda: [size_t_of(h.lib.mi355asr_workspace_bytes, h.ptr, 1, 32000)]))
        assert r.shape == (1, 52, 256)
        if mode == "float32":
            within("streaming encoder float32 against the float64 oracle", r, co.streaming_conformer_encoder(x.astype(np.float64), w, cfg, 8000))
        else:
            # tests/test_gpu_parity.py, test_bf16_gemm_mode_against_rounding_oracle_and_fp32: encoder max < 2e-2, mean < 2e-3
            ref = bf16_oracle(lambda: co.streaming_conformer_encoder(x.astype(np.float64), w, cfg, 8000))
            err = np.abs(r - ref)
            print("  streaming encoder bfloat16 against the bf16 rounding oracle: max %.3g (bound 2e-2), mean %.3g (bound 2e-3)" % (err.max(), err.mean()))
            if not (err.max() < 2e-2 and err.mean() < 2e-3):
                finding("streaming encoder bfloat16: max %.3g / mean %.3g from the bf16 rounding oracle" % (err.max(), err.mean()))


# ---- Translator ------------------------------------------------------------------------------------------------------------
def step_translator():
    from tensorflowasr_amd.models import Translator
    rng = np.random.default_rng(3)
    for B, U, T, blocks, ragged in ((2, 7, 30, 1, False), (2, 40, 250, 2, False), (2, 40, 250, 2, True)):
        cfg = dict(co.CONFORMER_S, translator_num_blocks=blocks, translator_fc_factor=0.5, translator_kernel_size=32)
        w = co.translator_weights(cfg, 60, 100, seed=11)
        t = Translator(inp_classes=60, tar_classes=100, dmodel=144, num_blocks=blocks, head_size=36, num_heads=4, kernel_size=32)
        t.load_weights(w, by_name=False)
        h = t._h
        ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
        enc = rng.standard_normal((B, T, 144)).astype(np.float32)
        big_ids = rng.integers(0, 60, size=(B + 1, U + 9)).astype(np.int32)
        big_enc = rng.standard_normal((B + 1, T + 21, 144)).astype(np.float32)
        kw, big_kw = {}, {}
        if ragged:
            tl, el = np.array([17, 40], np.int32), np.array([33, 250], np.int32)
            kw = dict(token_lengths=tl, enc_lengths=el)
            big_kw = dict(token_lengths=np.array([U + 9, 18, 30], np.int32), enc_lengths=np.array([T + 21, 40, 17], np.int32))
            enc = nan_tail(enc, el)
        name = "Translator (%d, %d, %d), %d block%s%s" % (B, U, T, blocks, "s" * (blocks > 1), ", ragged" if ragged else "")

        def call(stale):
            drop_ws(t) if not stale else t([big_ids, big_enc], return_argmax=True, **big_kw)
            return t([ids, enc], return_argmax=True, **kw)
        r = three_runs(name, call, lambda: [size_t_of(h.lib.mi355asr_translator_workspace_bytes, h.ptr, B, U, T)])
        lg, am = first(r, "out[0]"), first(r, "out[1]")
        if not ragged:
            within(name + " against the float64 oracle", lg, co.translator(ids, enc.astype(np.float64), w, cfg))
            assert np.array_equal(am, lg.argmax(-1))
        else:
            for b in range(B):
                ref = co.translator(ids[b:b + 1, :tl[b]], enc[b:b + 1, :el[b]].astype(np.float64), w, cfg)
                within(name + " row %d against the oracle on the row alone" % b, lg[b:b + 1, :tl[b]], ref)
                assert not lg[b, tl[b]:].any() and (am[b, tl[b]:] == -1).all() and np.array_equal(am[b, :tl[b]], lg[b, :tl[b]].argmax(-1))


# ---- LEAF frontend, add_wav_info, plain Spectrogram --------------------------------------------------------------------------
def step_frontends():
    from tensorflowasr_amd.models import ConformerEncoder
    from test_gpu_parity import _leaf_weights
    B, L = 2, 16000
    x = waves(B, L, 60).astype(np.float32)
    big = waves(B + 1, L + 8000, 70).astype(np.float32)
    cfg = small_cfg(2)
    cases = []
    cases.append(("LEAF", dict(mel_layer_type="leaf"), _leaf_weights(cfg, 7), dict(cfg, mel_layer_type="leaf")))
    wa = co.encoder_weights(cfg, seed=21)
    wa.update(co.wave_pick_weights(cfg["dmodel"], 640, seed=22))
    cases.append(("add_wav_info", dict(mel_layer_type="Melspectrogram", add_wav_info=True), wa, dict(cfg, add_wav_info=True)))
    cs = dict(cfg, mel_layer_type="Spectrogram")
    cases.append(("Spectrogram", dict(mel_layer_type="Spectrogram"), co.encoder_weights(cs, seed=9), cs))
    for name, extra, w, ocfg in cases:
        e = ConformerEncoder(**dict(encoder_kwargs(cfg), **extra))
        e.load_weights(w, by_name=False)
        h = e._h

        def call(stale):
            drop_ws(e) if not stale else e(big)
            return e(x)
        r = first(three_runs("ConformerEncoder %s %dx%d" % (name, B, L), call, lambda: [size_t_of(h.lib.mi355asr_workspace_bytes, h.ptr, B, L)]))
        within("ConformerEncoder %s against the float64 oracle" % name, r, co.conformer_encoder(x.astype(np.float64), w, ocfg))

        def mel(stale):
            drop_ws(e) if not stale else e.melspectrogram(big)
            return e.melspectrogram(x)
        three_runs("melspectrogram %s %dx%d" % (name, B, L), mel, lambda: [size_t_of(h.lib.mi355asr_workspace_bytes, h.ptr, B, L)])



# ---- ChunkConformer ---------------------------------------------------------------------------------------------------------
def logged_workspaces(h, call):
    """-> (what call() returns, the workspace sizes the handle must have allocated: every request above the largest so far)"""
    asked, real = [], h.workspace

    def workspace(nbytes):
        asked.append(int(nbytes))
        return real(nbytes)
    h.workspace = workspace
    try:
        r = call()
    finally:
        del h.workspace
    grown, top = [], -1
    for v in asked:
        if v > top:
            grown.append(v)
            top = v
    return r, grown


def chunk_case():
    """the small ChunkConformer of tests/test_gpu_chunk_streams.py on its gated audio (ticks with 0 .. 4 picks)"""
    from helpers import pick_bias_for_ragged_counts
    from test_gpu_chunk_streams import SMALL, W, gated_waves, model
    x = gated_waves()
    w = co.chunk_weights(SMALL, seed=3)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(SMALL, w, x)
    return model(SMALL, w), w, SMALL, x, W


def step_chunk_predict():
    m, w, cfg, x, W = chunk_case()
    h = m._h
    B, L = 2, 24000
    xs, big = x[:2, :L].copy(), x[2:5, :L + 8000].copy()
    _, T = m.out_frames(L)

    def call(stale):
        drop_ws(m) if not stale else m.predict(big, stages=True)
        return m.predict(xs, stages=True)
    # mi355asr_chunk_outputs: picked / helper_out / text_logits / text_argmax have the capacity of T rows per utterance and
    # are written as [B, Tp] blocks; the wrapper returns exactly those blocks, the rest of the raw buffers is masked here
    r_probe = m.predict(xs, stages=True)
    Tp = int(r_probe["text_logits"].shape[1])
    d, V = cfg["dmodel"], cfg["decoder_num_classes"]
    head = lambda width: (np.arange(B * T * width) < B * Tp * width).reshape((B, T, width) if width > 1 else (B, T))   # noqa: E731
    # (raw tensors in the order predict allocates them: text_logits, text_argmax, front, enc, picker_hidden, picked, helper, picker_logits)
    raw = {"0: ": head(V), "1: ": head(1), "5: ": head(d), "6: ": head(d)}
    r = three_runs("ChunkConformer.predict(stages=True) 2x24000", call,
                   lambda: [size_t_of(h.lib.mi355asr_chunk_workspace_bytes, h.ptr, B, L)], raw_defined=raw)
    got = dict((p[len("out['"):-2], a) for p, a in r)
    ref = co.chunk_predict(xs.astype(np.float64), w, cfg)
    assert np.array_equal(got["counts"], ref["counts"]) and 0 < Tp < T, (got["counts"], ref["counts"], Tp, T)
    print("  picked frames per utterance %s of %d, Tp = %d" % (got["counts"].tolist(), T, Tp))
    for k in ("front", "enc", "picker_logits", "picker_hidden", "picked", "helper", "text_logits"):
        assert got[k].shape == ref[k].shape, k
        within("predict stage %s against the float64 oracle" % k, got[k], ref[k])
        print("      per utterance and frame: %s" % np.array2string(np.abs(got[k] - ref[k]).max(-1), precision=1, max_line_width=250))
    assert np.array_equal(got["text_argmax"], got["text_logits"].argmax(-1))



def step_chunk_single_stream():
    """picker_stream_predict -> feature_pick -> decoder_stream_predict over 4 packets, the caches carried by the caller"""
    from helpers import stream_oracle
    m, w, cfg, x, W = chunk_case()
    h = m._h
    ref = None
    for k in range(x.shape[0]):
        try:
            ref = stream_oracle(x[k:k + 1, :4 * W].astype(np.float64), w, cfg, 4, W)
        except ValueError:
            continue
        if ref[2].shape[1] > 0:
            break
    assert ref is not None and ref[2].shape[1] > 0, "no audio with text in its first four packets"
    a, other = x[k, :4 * W], x[(k + 1) % x.shape[0], :8 * W]

    def run(audio):
        caches, caches2, out = m.init_picker_caches(1), m.init_decoder_caches(1), []
        for i in range(len(audio) // W):
            vp, up, vh, caches = m.picker_stream_predict(audio[None, i * W:(i + 1) * W, None], caches)
            f, c = m.feature_pick(vh, vp)
            step = dict(valid_ctc=vp, unvalid_ctc=up, hidden=vh, picked=f, picked_ctc=c)
            if f.shape[1]:
                vt, ut, caches2 = m.decoder_stream_predict(f, caches2)
                step.update(text=vt, unvalid_text=ut)
            out.append(step)
        return dict(steps=out, picker_caches=list(caches), decoder_caches=list(caches2))
    want_ws = []

    def call(stale):
        if stale:
            run(other)
            return run(a)
        drop_ws(m)
        r, grown = logged_workspaces(h, lambda: run(a))
        want_ws[:] = grown
        return r
    # (no mask: feature_pick's kept-frame index list is compared in full -- the arg-max pass writes every entry of it before
    # the compaction moves the kept ones to the front)
    r = three_runs("picker_stream_predict / feature_pick / decoder_stream_predict x 4", call, lambda: want_ws)
    got = dict(r)
    ph = np.concatenate([got["out['steps'][%d]['valid_ctc']" % i] for i in range(4)], 1)
    hid = np.concatenate([got["out['steps'][%d]['hidden']" % i] for i in range(4)], 1)
    txt = np.concatenate([got[k] for k in sorted(got) if k.endswith("['text']")], 1)
    unv = [got[k] for k in sorted(got) if k.endswith("['unvalid_text']")][-1]
    within("single stream phone logits against the float64 oracle", ph, ref[0])
    within("single stream picker hidden", hid, ref[1])
    within("single stream text logits", txt, ref[2])
    within("single stream unvalid text logits", unv, ref[3])
    # feature_pick on no frames (a packet that gave the picker nothing): counts 0, set on the device as well.  idx is [B, 0] in
    # the header; the wrapper's one placeholder column of it (raw tensor 0) is nobody's output
    hid0 = torch.zeros((2, 0, cfg["dmodel"]), device="cuda:0")
    ctc0 = torch.zeros((2, 0, cfg["picker_num_classes"]), device="cuda:0")
    r = three_runs("feature_pick on no frames", lambda stale: m.feature_pick(hid0, ctc0), raw_defined={"0: ": np.zeros((2, 1), bool)})
    assert [a.shape for _, a in r] == [(2, 0, cfg["dmodel"]), (2, 0, cfg["picker_num_classes"])]



def step_chunk_streams():
    """open_streams(4) and stream_step over 12 ticks: a slot reset and reused at tick 6, a stream that ends on a short packet,
    a stream that joins at tick 2; the state buffer poisoned before open_streams' reset"""
    from test_gpu_chunk_streams import Track, oracle_stream
    m, w, cfg, x, W = chunk_case()
    h = m._h
    audios = {0: x[0, :12 * W], 1: x[1, :6 * W], 2: x[2, :8 * W - 1000], 3: x[3, :10 * W], 4: x[4, :6 * W]}
    # stream -> (slot, first tick)
    plan = {0: (0, 0), 1: (1, 0), 2: (2, 0), 3: (3, 2), 4: (1, 6)}

    def ticks(st, tracks=None):
        out, pos = [], {k: 0 for k in plan}
        for tick in range(12):
            if tick == 6:
                m.reset_streams(st, [1])
            slots, rows, who = [], [], []
            for k, (slot, t0) in plan.items():
                if tick >= t0 and pos[k] < len(audios[k]) and not (k == 1 and tick >= 6):
                    slots.append(slot); rows.append(audios[k][pos[k]:pos[k] + W]); who.append(k)
                    pos[k] += W
            res = m.stream_step(st, slots, rows, want_logits=True)
            out.append({"stream %d" % k: res[slot] for k, slot in zip(who, slots)})
            if tracks is not None:
                for k, slot in zip(who, slots):
                    tracks[k].take(res[slot])
        assert all(pos[k] >= len(audios[k]) for k in plan)
        return out
    sizes = (ctypes.c_size_t(), ctypes.c_size_t())
    _lib.check(h.lib.mi355asr_chunk_streams_bytes(h.ptr, 4, ctypes.byref(sizes[0]), ctypes.byref(sizes[1])))
    keep = {}

    def call(stale):
        if stale:                                     # the same state object after other audio, then its reset
            st = keep["st"]
            m.reset_streams(st, None)                 # (slot 2 ended on a short packet)
            for tick in range(5):
                m.stream_step(st, [3, 0, 2, 1], [x[5 - i, (tick + 7) * W:(tick + 8) * W] for i in range(4)], want_logits=True)
            m.reset_streams(st, None)
            return ticks(st)
        drop_ws(m)
        keep["st"] = m.open_streams(4)
        return ticks(keep["st"])
    # (no mask: the padding rows of text_logits / text_argmax past n_valid + n_unvalid are written the same way in every run
    # and are compared with the rest)
    r = three_runs("open_streams(4) + stream_step x 12", call, [sizes[0].value, sizes[1].value])
    tracks = {k: Track() for k in plan}
    st = m.open_streams(4)
    again = flat(ticks(st, tracks))
    same("stream_step x 12", "returned", r, again, ("R0", "a fourth run"))
    picks = sorted({p for t in tracks.values() for p in t.picks})
    assert picks[0] == 0 and picks[-1] == 4, picks
    for k in plan:
        tracks[k].against(oracle_stream(audios[k], w, cfg), "stream %d" % k)
    print("  picks per tick seen: %s" % picks)




# ---- CTC lattice ------------------------------------------------------------------------------------------------------------
def step_lattice():
    import ctc_yardstick as cy
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    from test_gpu_ctc_lattice import case, check_alignment
    c = case("b_boost8")
    B, T, V = c["z"].shape
    U = c["lab"].shape[1]
    bz, bl, bil, bll = cy.make_case(77, B + 1, T + 50, V, U + 10, boost=8.0)
    bad = 4
    for infeasible in (False, True):
        z, lab, il, ll = c["z"], c["lab"].copy(), c["il"].copy(), c["ll"].copy()
        if infeasible:                                   # 10 equal labels need 19 frames (tests/test_gpu_ctc_lattice.py)
            lab[bad, :10] = lab[bad, 0]
            ll[bad], il[bad] = 10, 18
        tag = "b_boost8" + (" with an infeasible row" if infeasible else "")

        def loss(stale):
            if stale:
                ctc_loss(bz, bl, bil, bll, return_grad=True)
            return ctc_loss(z, lab, il, ll, return_grad=True)

        def align(stale):
            if stale:
                ctc_forced_align(bz, bl, bil, bll)
            return ctc_forced_align(z, lab, il, ll)
        lib = _lib.lib()
        r = three_runs("ctc_loss(return_grad=True) " + tag, loss, lambda: [size_t_of(lib.mi355asr_ctc_loss_workspace_bytes, B, T, V, U, 1)])
        got_loss, got_grad = first(r, "out[0]"), first(r, "out[1]")
        ra = three_runs("ctc_forced_align " + tag, align, lambda: [size_t_of(lib.mi355asr_ctc_align_workspace_bytes, B, T, V, U)])
        path, spans, score = first(ra, "out[0]"), first(ra, "out[1]"), first(ra, "out[2]")
        for b in range(B):                               # written zeros, not the fill, past each utterance
            assert np.all(got_grad[b, il[b]:].view(np.int32) == 0) and np.all(path[b, il[b]:] == -1), b
        keep = [b for b in range(B) if not (infeasible and b == bad)]
        e_loss = float(np.abs(got_loss[keep] - c["l64"][keep]).max())
        e_grad = float(np.abs(got_grad[keep] - c["g64"][keep]).max())
        b_loss, b_grad = cy.bound(c["e_loss"], c["l64"]), cy.bound(c["e_grad"], c["g64"])
        print("  %s: loss max|d| %.3g (bound %.3g), gradient max|d| %.3g (bound %.3g)" % (tag, e_loss, b_loss, e_grad, b_grad))
        if not (e_loss <= b_loss and e_grad <= b_grad):
            finding("%s: loss %.3g / gradient %.3g from float64, bounds %.3g / %.3g" % (tag, e_loss, e_grad, b_loss, b_grad))
        if infeasible:
            assert np.isposinf(got_loss[bad]) and np.all(got_grad[bad].view(np.int32) == 0), "the infeasible row's gradient block is written zeros"
            assert np.isneginf(score[bad]) and np.all(path[bad] == -1) and np.all(spans[bad] == -1)
        for b in keep:
            n, u = int(il[b]), int(ll[b])
            check_alignment(cy.log_q(z[b, :n]).numpy(), lab[b, :u], V - 1, path[b, :n], spans[b], float(score[b]), "%s row %d" % (tag, b))


# ---- decoding ---------------------------------------------------------------------------------------------------------------
def step_greedy_argmax():
    from tensorflowasr_amd.models import ctc_greedy_decode, frame_argmax
    rng = np.random.default_rng(3)
    B, T, blank = 9, 333, 6
    fa = rng.integers(0, 7, (B, T)).astype(np.int32)
    fa[4] = blank
    fa[5] = 2
    in_len = np.array([333, 0, 1, 64, 333, 333, 65, 128, 200], np.int32)      # tests/test_gpu_parity.py, test_greedy_ragged_lengths_and_edges
    big = rng.integers(0, 7, (B + 2, T + 100)).astype(np.int32)

    def greedy(stale):
        if stale:
            ctc_greedy_decode(big, None, blank, device="cuda:0")
        return ctc_greedy_decode(fa, in_len, blank, device="cuda:0")
    r = three_runs("ctc_greedy_decode (9, 333) ragged", greedy)
    rid, rlen = co.ctc_collapse(fa, in_len, blank)
    assert np.array_equal(first(r, "out[0]"), rid) and np.array_equal(first(r, "out[1]"), rlen)
    print("  ctc_greedy_decode == the host collapse, ids -1 past each length")
    for V in (277, 1332):
        x = rng.standard_normal((3, 37, V)).astype(np.float32)
        x[0, 0, 5] = x[0, 0, 200] = 9.0                                     # a tie: the first maximum
        bigx = rng.standard_normal((4, 50, V)).astype(np.float32)

        def amax(stale):
            if stale:
                frame_argmax(torch.from_numpy(bigx).cuda())
            return frame_argmax(torch.from_numpy(x).cuda())
        r = first(three_runs("frame_argmax V = %d" % V, amax))
        assert np.array_equal(r, x.argmax(-1)) and r[0, 0] == 5
        print("  frame_argmax V = %d == np.argmax" % V)


def peaky(rng, shape, V, conc=0.08):
    return rng.dirichlet(np.full(V, conc), size=shape).astype(np.float32)


def step_beam():
    """the one-shot device prefix beam search against the host search, bit for bit"""
    from tensorflowasr_amd.models import beam_device_limits, beam_last_path, ctc_prefix_beam_decode
    from test_beam_lm_host import scorer
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    # mi355asr_beam_last_path: 2 the one-key-per-thread kernel (beam <= small_beam and beam * (min(N, beam + 2) + 1) <= 256 with
    # N = min(top-n, V): both beam 10 and beam 4 here), 3 the radix kernel (beam 20: 20 * 23 > 256), 4 the search with a scorer
    lim = beam_device_limits(False)
    for B, T, V, beam, order in ((2, 120, 60, 10, None), (2, 120, 50, 10, 3), (2, 120, 60, 4, None), (2, 120, 60, 20, None)):
        path = 4 if order else (2 if beam <= lim["small_beam"] and beam * (min(40, V, beam + 2) + 1) <= 256 else 3)
        assert path == {10: 2, 4: 2, 20: 3}[beam] or order, (beam, path, lim)
        s = scorer(order, 0.9, 0.2) if order else None               # (the fixture scorer knows 49 classes + blank)
        p = peaky(rng, (B, T), V)
        lens = np.array([T, T - 37], np.int32)
        big = peaky(rng, (B + 1, T + 30), V)
        tag = "ctc_prefix_beam_decode (%d, %d, %d) beam %d%s" % (B, T, V, beam, ", order-%d scorer" % order if order else "")

        def call(stale):
            if stale:
                ctc_prefix_beam_decode(torch.from_numpy(big).cuda(), None, beam, 0.99, 40, ext_scorer=s)
            r = ctc_prefix_beam_decode(torch.from_numpy(p).cuda(), lens, beam, 0.99, 40, ext_scorer=s)
            assert beam_last_path() == path, (tag, beam_last_path(), path)
            return r
        fn = lib.mi355asr_ctc_prefix_beam_lm_workspace_bytes if s else lib.mi355asr_ctc_prefix_beam_workspace_bytes
        r = three_runs(tag, call, lambda: [size_t_of(fn, B, T, 40, beam, T)])
        host = flat(ctc_prefix_beam_decode(p, lens, beam, 0.99, 40, ext_scorer=s, num_threads=2))
        same(tag, "result", r, host, ("R0", "the host search"))
        print("  %s == the host search bit for bit (path %d)" % (tag, path))


def step_beam_streams():
    """BeamStreams(3, ...): the state poisoned before its first reset; 5 steps with n_peek > 0, slot 1 reset midway"""
    from beam_streams_gpu_steps import HostSlots, rows_of, rows_of_host
    from tensorflowasr_amd.models import BeamStreams
    from test_beam_lm_host import scorer
    lib = _lib.lib()
    V, T, mf = 50, 6, 40
    rng = np.random.default_rng(8)
    frames = [peaky(rng, 60, V, c) for c in (0.05, 0.1, 0.3)]
    junk = peaky(rng, (3, 9), V, 0.2)
    plan = [([0, 1, 2], [3, 2, 4], [2, 3, 1]), ([2, 0], [4, 1], [1, 2]), ([1, 0, 2], [3, 3, 0], [3, 1, 2]),
            ([1, 2, 0], [2, 3, 4], [1, 3, 2]), ([0, 1], [2, 4], [4, 1])]                # (slots, n_commit, n_peek) per step
    for order, beam in ((None, 10), (3, 10), (None, 4)):
        s = scorer(order, 0.9, 0.2) if order else None
        tag = "BeamStreams(3, %d, beam %d%s)" % (V, beam, ", order-%d scorer" % order if order else "")
        keep = {}

        def run(bs, host=None):
            fed, out = [0, 0, 0], []
            for i, (slots, nc, npk) in enumerate(plan):
                if i == 3:
                    bs.reset([1])
                    fed[1] = 30                           # other frames for the new stream in slot 1
                    if host:
                        host.d[1].reset()
                x = np.zeros((len(slots), T, V), np.float32)
                x[:] = np.nan                             # rows behind commit + peek are padding and may hold anything
                for j, sl in enumerate(slots):
                    x[j, :nc[j] + npk[j]] = frames[sl][fed[sl]:fed[sl] + nc[j] + npk[j]]
                r = bs.read(bs.step(slots, torch.from_numpy(x).cuda(), nc, npk, is_logits=False, n_best=3, max_len=mf))
                if host:
                    for j, sl in enumerate(slots):
                        assert rows_of(r, j) == rows_of_host(host.step(sl, x[j], nc[j], npk[j]), 3), (tag, i, sl)
                for j, sl in enumerate(slots):
                    fed[sl] += nc[j]
                out.append(r)
            return out

        def call(stale):
            if stale:
                bs = keep["bs"]                           # the same object after other frames, then its reset
                bs.step([0, 1, 2], torch.from_numpy(junk).cuda(), [5, 9, 2], [3, 0, 4], is_logits=False, n_best=3, max_len=mf)
                bs.reset()
            else:
                bs = keep["bs"] = BeamStreams(3, V, beam, 0.99, 40, ext_scorer=s, max_frames=mf)
            return run(bs)
        sb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mi355asr_beam_streams_bytes(3, V, beam, 40, mf, s.handle() if s else None, T, ctypes.byref(sb), ctypes.byref(wb)))
        # mi355asr_beam_streams_outputs: ids are -1 padded and scores -FLT_MAX where there is no hypothesis
        r = three_runs(tag, call, [sb.value, wb.value])
        again = run(BeamStreams(3, V, beam, 0.99, 40, ext_scorer=s, max_frames=mf), HostSlots(3, V, beam, 0.99, 40, s))
        same(tag, "returned", r, flat(again), ("R0", "the run checked against the host decoders"))
        print("  %s == one host BeamDecoder (and its fork) per slot, bit for bit, on 5 steps" % tag)


# ---- VAD and enhancement ------------------------------------------------------------------------------------------------------
def step_vad_enhance():
    from fence import Fence
    from tensorflowasr_amd.vad import VAD
    from test_vad_enhance_host import SAVED_MODEL, enhance64, input_frames, saved_model_weights
    from test_vad_host import graph_weights, net64
    vad = VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx"))
    rng = np.random.default_rng(3)
    lens = [16000 * 3 + 37, 16000, 5 * 160 + 159]                          # tests/test_gpu_vad.py, test_rows_are_independent
    L = max(lens) + 1000
    x = nan_tail(rng.standard_normal((3, L)) * 0.1, lens)
    big = (rng.standard_normal((4, L + 8000)) * 0.1).astype(np.float32)

    def scores(stale):
        if stale:
            vad.scores(big)
        return vad.scores(x, lengths=lens)
    r = first(three_runs("VAD.scores(lengths=)", scores))
    w = graph_weights()
    for b, n in enumerate(lens):
        tb = n // 160
        want = net64(x[b, :tb * 160:2].reshape(tb, 80), w)
        err = float((np.abs(r[b, :tb] - want) / np.maximum(1.0, np.abs(want))).max())
        print("  VAD row %d: %d frames, max scaled error against net64 %.3g (bound 1e-4)" % (b, tb, err))
        if not err <= 1e-4:
            finding("VAD.scores row %d: %.3g from net64" % (b, err))
        assert not r[b, tb:].any()
    # the wrapper zero-fills what mi355asr_vad_forward leaves unwritten ("score entries past its frame count are not written"):
    # the C entry point on a fenced 0xFF output writes the same scores and leaves exactly those entries alone
    h = vad._handle(2)
    f = Fence(0xFF, 4096)
    out = f.allocate(torch.empty, (3, L // 160), torch.float32, "cuda:0", "the C ABI call of step_vad_enhance")
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    _lib.check(h.lib.mi355asr_vad_forward(h.ptr, ctypes.c_void_p(xd.data_ptr()), 3, L, ctypes.c_void_p(ld.data_ptr()), ctypes.c_void_p(out.data_ptr()), h._stream()))
    torch.cuda.synchronize()
    f.check()
    o = out.cpu().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(o[b, :n // 160].view(np.int32), r[b, :n // 160].view(np.int32)) and np.all(o[b, n // 160:].view(np.int32) == -1), b
    print("  mi355asr_vad_forward on a fenced 0xFF output: the same scores, entries past each row's frames untouched, guards intact")
    ev = VAD().load_saved_model(SAVED_MODEL)
    T = 57
    for sr in (16000, 8000):
        dec = sr // 8000
        xe = (rng.standard_normal(T * 80 * dec + 37) * 0.1).astype(np.float32)
        bige = (rng.standard_normal((2, (T + 20) * 80 * dec)) * 0.1).astype(np.float32)

        def enhance(stale):
            if stale:
                ev.enhance(bige, sample_rate=sr)
            return ev.enhance(xe, sample_rate=sr)
        r = three_runs("VAD.enhance T = 57, %d Hz" % sr, enhance)
        e, sc = first(r, "out[0]"), first(r, "out[1]")
        fr = input_frames(xe, sr)
        s64, e64 = enhance64(fr, saved_model_weights())
        from test_gpu_vad_enhance import sample_err
        err, serr = sample_err(e.reshape(-1, 80), e64, fr), float(np.abs(sc[0] - s64).max() / max(1.0, np.abs(s64).max()))
        print("  enhance %d Hz: enhanced worst relative error %.3g (bound 1e-5), scores %.3g (bound 1e-4)" % (sr, err, serr))
        if not (err <= 1e-5 and serr <= 1e-4):
            finding("VAD.enhance %d Hz: %.3g / %.3g from the float64 network" % (sr, err, serr))


# ---- resampling ---------------------------------------------------------------------------------------------------------------
def step_resample():
    from resample_ref import taps_and_gain
    from scipy.signal import resample_poly
    from tensorflowasr_amd.resample import Resampler, StreamResampler, out_length
    rng = np.random.default_rng(9)
    for sr_in, sr_out in ((8000, 16000), (44100, 16000)):
        rs = Resampler(sr_in, sr_out)
        up, down = rs.up, rs.down
        lens = [4417, 2999, 1]
        x = nan_tail(rng.standard_normal((3, max(lens))), lens)
        big = rng.standard_normal((4, max(lens) + 3000)).astype(np.float32)

        def call(stale):
            if stale:
                rs(big)
            return rs(x, lens)
        r = three_runs("Resampler(%d, %d) ragged batch of 3" % (sr_in, sr_out), call)
        y, ol = first(r, "out[0]"), first(r, "out[1]")
        K, A = taps_and_gain(up, down)
        for b, n in enumerate(lens):
            ref = resample_poly(x[b, :n].astype(np.float64), up, down)
            assert ol[b] == len(ref) == out_length(n, up, down) and not y[b, ol[b]:].any(), b
            tol = (K + 2) * 2.0 ** -23 * A * float(np.abs(x[b, :n]).max())      # tests/test_resample_gpu.py: the filter's fp32 bound
            err = float(np.abs(y[b, :ol[b]] - ref).max())
            print("  ratio %d/%d row %d: max|d| against resample_poly %.3g (bound %.3g)" % (up, down, b, err, tol))
            if not err <= tol:
                finding("Resampler %d/%d row %d: %.3g above %.3g" % (up, down, b, err, tol))
    # ---- streams: the state poisoned before its reset
    lib = _lib.lib()
    max_packet = 2000
    one = Resampler(48000, 16000)
    audio = [rng.standard_normal(5000).astype(np.float32) for _ in range(3)]
    sizes = [[1280, 7, 2000, 160], [2000, 160, 1, 1280], [7, 1280, 160, 2000]]
    keep = {}

    def run(srs):
        pos, out = [0, 0, 0], []
        for i in range(4):
            slots = [2, 0, 1] if i % 2 else [0, 1, 2]
            pk = [audio[s][pos[s]:pos[s] + sizes[s][i]] for s in slots]
            y, n_out = srs.step_device(slots, pk)
            out.append(dict(y=y, n_out=n_out))
            for s in slots:
                pos[s] += sizes[s][i]
        out.append(srs.flush([0, 1, 2]))
        return out, pos

    def call(stale):
        if stale:
            srs = keep["srs"]
            srs.step([0, 1, 2], [rng.standard_normal(1999).astype(np.float32) for _ in range(3)])
            srs.reset()
        else:
            srs = keep["srs"] = StreamResampler(3, 48000, 16000, max_packet)
        return run(srs)[0]
    sb, wb, oc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    _lib.check(lib.mi355asr_resample_streams_bytes(1, 3, 3, max_packet, ctypes.byref(sb), ctypes.byref(wb), ctypes.byref(oc)))
    three_runs("StreamResampler(3, 48000, 16000) x 4 steps + flush", call, [sb.value, wb.value])
    srs = StreamResampler(3, 48000, 16000, max_packet)
    out, pos = run(srs)
    got = {s: [] for s in range(3)}
    for i in range(4):
        slots = [2, 0, 1] if i % 2 else [0, 1, 2]
        yh = out[i]["y"].cpu().numpy()
        for j, s in enumerate(slots):
            got[s].append(yh[j, :out[i]["n_out"][j]])
    for s in range(3):
        whole = np.concatenate(got[s] + [out[4][s]])
        ref, _ = one(audio[s][:pos[s]])
        assert np.array_equal(whole.view(np.int32), ref.cpu().numpy()[0, :len(whole)].view(np.int32)) and len(whole) == out_length(pos[s], 1, 3), s
    print("  every stream's concatenated output == Resampler on its concatenated input, bit for bit (itself within the bound above)")


# ---- streaming histories --------------------------------------------------------------------------------------------------
def step_histories():
    from tensorflowasr_amd.stream_session import stream_append, stream_gather
    rng = np.random.default_rng(7)
    N, Tcap, d, Tc = 6, 39, 256, 13                                       # tests/test_gpu_stream_session.py
    hist = torch.zeros((N, Tcap, d), dtype=torch.float32, device="cuda")
    hl = torch.zeros((N,), dtype=torch.int32, device="cuda")
    hl_host = np.zeros(N, np.int32)
    want, wl = np.zeros((N, Tcap, d), np.float32), np.zeros(N, np.int32)
    calls = [(slots, rng.standard_normal((len(slots), Tc, d)).astype(np.float32)) for slots in ([4, 1, 5], [1, 0], [5, 1, 3])]
    for slots, c in calls:
        stream_append(torch.from_numpy(c).cuda(), slots, hist, hl, hl_host)
        for m_, s in enumerate(slots):
            want[s, wl[s]:wl[s] + Tc] = c[m_]
            wl[s] += Tc
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy(), want) and np.array_equal(hl.cpu().numpy(), wl) and np.array_equal(hl_host, wl)

    def append(stale):
        """stream_append has no workspace and allocates nothing through the package (the fence records no allocation): its
        outputs are the caller's history and lengths, here filled with the fence's byte by hand, the lengths then set to 0"""
        fill = 0.0 if stale else float("nan")
        h2 = torch.full((N, Tcap, d), fill, dtype=torch.float32, device="cuda")
        l2, l2h = torch.zeros((N,), dtype=torch.int32, device="cuda"), np.zeros(N, np.int32)
        for slots, c in calls:
            stream_append(torch.from_numpy(c).cuda(), slots, h2, l2, l2h)
        rows = torch.arange(Tcap, device="cuda")[None, :, None] < l2[:, None, None]
        return torch.where(rows, h2, torch.zeros((), device="cuda")), l2, l2h
    r = three_runs("stream_append x 3 on a NaN-filled history", append)
    assert np.array_equal(first(r, "out[0]").view(np.int32), want.view(np.int32)) and np.array_equal(first(r, "out[1]"), wl)
    slots, tl, Tpad = [5, 0, 1, 4], [26, 0, 7, 13], 70
    tails = rng.standard_normal((4, 26, d)).astype(np.float32)
    td = torch.from_numpy(tails).cuda()

    def gather(stale):
        if stale:
            stream_gather(hist, hl, hl_host, [1, 3, 0, 4, 5], Tpad + 20)
        return stream_gather(hist, hl, hl_host, slots, Tpad, td, tl)
    r = three_runs("stream_gather with tails", gather)
    out, ol = first(r, "out[0]"), first(r, "out[1]")
    exp = np.zeros((4, Tpad, d), np.float32)
    for i, s in enumerate(slots):
        exp[i, :wl[s]] = want[s, :wl[s]]
        exp[i, wl[s]:wl[s] + tl[i]] = tails[i, :tl[i]]
    assert np.array_equal(out.view(np.int32), exp.view(np.int32)) and ol.tolist() == [int(wl[s]) + t for s, t in zip(slots, tl)]
    print("  stream_append / stream_gather == NumPy, rows past each length written zeros under the 0xFF fill")



# ---- streams and handles (no fence) -----------------------------------------------------------------------------------------
# The delay: DELAY_MATMULS products of two DELAY_N x DELAY_N fp32 matrices, enqueued on the side stream in front of the input's
# copy.  Sized once on the MI355X: one product takes 7.2 ms (64 of them: 461 ms between two events), so the delay is about
# 170 ms; the longest compared call (open_streams + four stream_steps with their read-backs) takes about 3 ms of host time to
# enqueue and, where it synchronises, to finish: a factor above 50 where 10 is asked.  Every step measures both again and
# asserts the factor of 10.
DELAY_N, DELAY_MATMULS = 8192, 24


class Delay:
    def __init__(self):
        self.a = torch.randn((DELAY_N, DELAY_N), device="cuda:0")
        self.b = torch.empty_like(self.a)
        self.shortest_ms, self.longest_call_ms = float("inf"), 0.0
        torch.cuda.synchronize()

    def enqueue(self):
        for _ in range(DELAY_MATMULS):
            torch.matmul(self.a, self.a, out=self.b)

    def timed(self, e0, e1):
        ms = e0.elapsed_time(e1)
        self.shortest_ms = min(self.shortest_ms, ms)
        return ms

    def conclude(self):
        print("  delay: %d matmuls of %d x %d, shortest %.1f ms between its events; longest compared call: %.2f ms of host time"
              % (DELAY_MATMULS, DELAY_N, DELAY_N, self.shortest_ms, self.longest_call_ms))
        assert self.shortest_ms >= 10.0 * self.longest_call_ms, "delay too short: %.1f ms against calls of %.2f ms" % (self.shortest_ms, self.longest_call_ms)


def control(delay):
    """no library code: a copy enqueued on a pool stream behind the delay has not happened when the null stream reads"""
    side = torch.cuda.Stream()
    x_side = torch.full((1 << 20,), 1.0, device="cuda:0")
    new = torch.full((1 << 20,), 2.0).pin_memory()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record()
        delay.enqueue()
        x_side.copy_(new, non_blocking=True)
        e1.record()
    seen = x_side.clone()                                 # on the default stream, meanwhile
    torch.cuda.current_stream().synchronize()
    early = seen.cpu().numpy()
    side.synchronize()
    late = x_side.cpu().numpy()
    ms = delay.timed(e0, e1)
    assert (late == 2.0).all(), "the copy on the side stream never arrived"
    assert (early == 1.0).all(), "delay too short: the default stream saw the new contents (%d of %d words) after %.1f ms" % (int((early == 2.0).sum()), early.size, ms)
    print("  control: the default stream read the old contents while the side stream's copy waited %.1f ms behind the delay: pool "
          "streams do not wait for the null stream" % ms)


def on_side_stream(delay, name, inputs, warm, call):
    """inputs / warm: {name: NumPy array} of the case and of the warm-up; call(dict of device tensors) -> result.  The device
    buffers hold the warm-up input until the side stream's copy, behind the delay, replaces it: a launch or a copy that went
    to another stream than the one it was given reads the warm-up data (or its own warm-up results) instead."""
    bufs = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in warm.items()}
    pinned = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in inputs.items()}
    assert all(bufs[k].shape == pinned[k].shape and bufs[k].dtype == pinned[k].dtype for k in bufs), name
    flat(call(bufs))                                      # the warm-up, on the default stream
    for k in bufs:
        bufs[k].copy_(pinned[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = call(bufs)
    wall = (time.perf_counter() - t0) * 1e3
    ref = flat(ref)
    delay.longest_call_ms = max(delay.longest_call_ms, wall)
    for k in bufs:                                        # the warm-up input again, and its results in the workspaces
        bufs[k].copy_(torch.from_numpy(np.ascontiguousarray(warm[k])))
    flat(call(bufs))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record()
        delay.enqueue()
        e1.record()
        for k in bufs:
            bufs[k].copy_(pinned[k], non_blocking=True)
        r = call(bufs)
        side.synchronize()
    got = flat(r)
    ms = delay.timed(e0, e1)
    before = len(FINDINGS)
    same(name, "result", ref, got, ("the default stream", "the side stream"))
    print("  %-50s side stream %s default stream; call %.2f ms of host time, delay %.1f ms"
          % (name, "==" if len(FINDINGS) == before else "!=", wall, ms))


def step_side_stream_models():
    from tensorflowasr_amd.models import ConformerEncoder, Translator
    from test_gpu_parity import _leaf_weights
    delay = Delay()
    control(delay)
    m, w, cfg = conformer_ctc()
    x, xw = waves(2, 32000, 7).astype(np.float32), waves(2, 32000, 90).astype(np.float32)
    on_side_stream(delay, "ConformerCTC.recognize 2x32000 (fused_ns)", dict(x=x), dict(x=xw), lambda b: m.recognize(b["x"]))
    on_side_stream(delay, "ConformerCTC.encode + ctc_logits", dict(x=x), dict(x=xw), lambda b: m.ctc_logits(m.encode(b["x"]), return_argmax=True))
    lens = np.array(RAGGED_LENS, np.int32)
    xr, xrw = nan_tail(waves(3, RAGGED_L, 11), lens), waves(3, RAGGED_L, 91).astype(np.float32)
    # (the ragged length check synchronises the stream at entry: it must pass unchanged)
    on_side_stream(delay, "recognize(wav_lengths) ragged", dict(x=xr), dict(x=xrw), lambda b: m.recognize(b["x"], wav_lengths=lens))
    c, wc, _ = ctc256("float32")
    rng = np.random.default_rng(1)
    e, ew = rng.standard_normal((2, 40, 256)).astype(np.float32), rng.standard_normal((2, 40, 256)).astype(np.float32)
    on_side_stream(delay, "CTCDecoder 256 float32 (2, 40)", dict(x=e), dict(x=ew), lambda b: c(b["x"], return_argmax=True))
    t = Translator(inp_classes=60, tar_classes=100, dmodel=144, num_blocks=1, head_size=36, num_heads=4, kernel_size=32)._build(seed=11)
    ids, idw = rng.integers(0, 60, (2, 7)).astype(np.int32), rng.integers(0, 60, (2, 7)).astype(np.int32)
    en, enw = rng.standard_normal((2, 30, 144)).astype(np.float32), rng.standard_normal((2, 30, 144)).astype(np.float32)
    on_side_stream(delay, "Translator (2, 7, 30)", dict(ids=ids, enc=en), dict(ids=idw, enc=enw), lambda b: t([b["ids"], b["enc"]], return_argmax=True))
    scfg = small_cfg(2)
    le = ConformerEncoder(**dict(encoder_kwargs(scfg), mel_layer_type="leaf"))
    le.load_weights(_leaf_weights(scfg, 7), by_name=False)
    xl, xlw = waves(2, 16000, 60).astype(np.float32), waves(2, 16000, 61).astype(np.float32)
    on_side_stream(delay, "ConformerEncoder LEAF 2x16000", dict(x=xl), dict(x=xlw), lambda b: le(b["x"]))
    delay.conclude()


def step_side_stream_chunk():
    delay = Delay()
    control(delay)
    m, w, cfg, x, W = chunk_case()
    # (chunk_predict synchronises its stream in the middle, stream_step reads its integers back: both must pass unchanged)
    on_side_stream(delay, "ChunkConformer.predict(stages=True) 2x24000", dict(x=x[:2, :24000].copy()), dict(x=x[2:4, :24000].copy()),
                   lambda b: m.predict(b["x"], stages=True))

    def streams(b):
        st = m.open_streams(4)
        return [m.stream_step(st, [2, 0, 3, 1], b["x"][:, i * W:(i + 1) * W].contiguous(), want_logits=True) for i in range(4)]
    on_side_stream(delay, "open_streams(4) + stream_step x 4", dict(x=x[:4, :4 * W].copy()), dict(x=x[2:6, 4 * W:8 * W].copy()), streams)

    def single(b):
        caches, out = m.init_picker_caches(1), []
        for i in range(3):
            vp, up, vh, caches = m.picker_stream_predict(b["x"][:, i * W:(i + 1) * W, None], caches)
            out.append((vp, up, vh) + tuple(m.feature_pick(vh, vp)))
        return out
    on_side_stream(delay, "picker_stream_predict + feature_pick x 3", dict(x=x[1:2, :3 * W].copy()), dict(x=x[3:4, :3 * W].copy()), single)
    delay.conclude()


def step_side_stream_decoding():
    import ctc_yardstick as cy
    from tensorflowasr_amd.models import BeamStreams, ctc_forced_align, ctc_greedy_decode, ctc_loss, ctc_prefix_beam_decode, frame_argmax
    from tensorflowasr_amd.resample import Resampler, StreamResampler
    from tensorflowasr_amd.stream_session import stream_append, stream_gather
    from tensorflowasr_amd.vad import VAD
    from test_beam_lm_host import scorer
    from test_vad_enhance_host import SAVED_MODEL
    delay = Delay()
    control(delay)
    rng = np.random.default_rng(21)
    z, lab, il, ll = cy.make_case(13, 8, 250, 1332, 40, boost=8.0)
    zw = cy.make_case(14, 8, 250, 1332, 40, boost=8.0)[0]
    on_side_stream(delay, "ctc_loss(return_grad=True) + ctc_forced_align", dict(z=z), dict(z=zw),
                   lambda b: (ctc_loss(b["z"], lab, il, ll, return_grad=True), ctc_forced_align(b["z"], lab, il, ll)))
    fa, faw = rng.integers(0, 7, (9, 333)).astype(np.int32), rng.integers(0, 7, (9, 333)).astype(np.int32)
    in_len = np.array([333, 0, 1, 64, 333, 333, 65, 128, 200], np.int32)
    lg, lgw = rng.standard_normal((3, 37, 1332)).astype(np.float32), rng.standard_normal((3, 37, 1332)).astype(np.float32)
    on_side_stream(delay, "ctc_greedy_decode + frame_argmax", dict(fa=fa, x=lg), dict(fa=faw, x=lgw),
                   lambda b: (ctc_greedy_decode(b["fa"], in_len, 6), frame_argmax(b["x"])))
    s = scorer(3, 0.9, 0.2)
    p, pw = peaky(rng, (2, 120), 50), peaky(rng, (2, 120), 50)
    # (the one-shot search returns host arrays: it synchronises its stream)
    for sc, tag in ((None, "scorer-less"), (s, "order-3 scorer")):
        on_side_stream(delay, "ctc_prefix_beam_decode (2, 120, 50) beam 10, %s" % tag, dict(p=p), dict(p=pw),
                       lambda b: ctc_prefix_beam_decode(b["p"], None, 10, 0.99, 40, ext_scorer=sc))

        def streams(b):
            bs = BeamStreams(3, 50, 10, 0.99, 40, ext_scorer=sc, max_frames=40)
            out = []
            for i in range(5):
                if i == 3:
                    bs.reset([1])
                out.append(bs.step([2, 0], b["p"][:, 6 * i:6 * i + 6].contiguous(), [4, 3], [2, 1], is_logits=False, n_best=3, max_len=40))
            return [bs.read(r) for r in out]
        on_side_stream(delay, "BeamStreams(3, 50, beam 10) x 5 steps, %s" % tag, dict(p=p), dict(p=pw), streams)
    vad, ev = VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx")), VAD().load_saved_model(SAVED_MODEL)
    lens = [16000 * 3 + 37, 16000, 5 * 160 + 159]
    xv, xvw = (rng.standard_normal((3, lens[0] + 1000)) * 0.1).astype(np.float32), (rng.standard_normal((3, lens[0] + 1000)) * 0.1).astype(np.float32)
    on_side_stream(delay, "VAD.scores(lengths=) + VAD.enhance", dict(x=xv), dict(x=xvw), lambda b: (vad.scores(b["x"], lengths=lens), ev.enhance(b["x"], lengths=lens)))
    rs = Resampler(44100, 16000)
    xr, xrw = rng.standard_normal((3, 4417)).astype(np.float32), rng.standard_normal((3, 4417)).astype(np.float32)
    on_side_stream(delay, "Resampler(44100, 16000) ragged", dict(x=xr), dict(x=xrw), lambda b: rs(b["x"], [4417, 2999, 1]))

    def resample_streams(b):
        srs = StreamResampler(3, 48000, 16000, 2000)
        return [srs.step_device([2, 0, 1], b["x"][:, 1000 * i:1000 * i + 1000].contiguous()) for i in range(4)]
    on_side_stream(delay, "StreamResampler(3, 48000, 16000) x 4 steps", dict(x=xr[:, :4000].copy()), dict(x=xrw[:, :4000].copy()), resample_streams)

    def histories(b):
        hist = torch.zeros((6, 39, 256), dtype=torch.float32, device="cuda")
        hl, hl_host = torch.zeros((6,), dtype=torch.int32, device="cuda"), np.zeros(6, np.int32)
        for i, slots in enumerate(([4, 1, 5], [1, 0], [5, 1, 3])):
            stream_append(b["c"][3 * i:3 * i + len(slots)], slots, hist, hl, hl_host)
        return stream_gather(hist, hl, hl_host, [5, 0, 1, 4], 70, b["t"], [26, 0, 7, 13]), hist, hl
    ch, chw = rng.standard_normal((9, 13, 256)).astype(np.float32), rng.standard_normal((9, 13, 256)).astype(np.float32)
    tl, tlw = rng.standard_normal((4, 26, 256)).astype(np.float32), rng.standard_normal((4, 26, 256)).astype(np.float32)
    on_side_stream(delay, "stream_append x 3 + stream_gather", dict(c=ch, t=tl), dict(c=chw, t=tlw), histories)
    delay.conclude()


def step_two_handles():
    """two handles in flight, each on its own side stream with its own workspace: 20 alternating rounds from one thread, then
    the two loops from two threads (ctypes releases the GIL); every result is the sequential one"""
    from tensorflowasr_amd.models import BeamStreams, ctc_loss
    from test_beam_lm_host import scorer
    rng = np.random.default_rng(31)
    m, _, _ = conformer_ctc()
    c, _, _ = ctc256("bfloat16")
    xs = [torch.from_numpy(waves(2, 32000, 100 + i).astype(np.float32)).cuda() for i in range(4)]
    es = [torch.from_numpy(rng.standard_normal((8, 260, 256)).astype(np.float32)).cuda() for _ in range(4)]
    s = scorer(3, 0.9, 0.2)
    ps = [torch.from_numpy(peaky(rng, (3, 4), 50)).cuda() for _ in range(20)]
    qs = [torch.from_numpy(peaky(rng, (3, 4), 50, 0.2)).cuda() for _ in range(20)]
    jobs = {"ConformerCTC 144 + CTCDecoder 256 bf16": (lambda i, st: m.recognize(xs[i % 4]), lambda i, st: c(es[i % 4], return_argmax=True), None),
            "two BeamStreams sharing one NGramScorer": (lambda i, st: st.step([0, 1, 2], ps[i], [2, 3, 1], [2, 1, 0], is_logits=False, n_best=3, max_len=80),
                                                        lambda i, st: st.step([2, 1, 0], qs[i], [3, 1, 2], [0, 2, 1], is_logits=False, n_best=3, max_len=80),
                                                        lambda: BeamStreams(3, 50, 10, 0.99, 40, ext_scorer=s, max_frames=80))}
    for name, (fa, fb, make) in jobs.items():
        def loop(fn, stream, out, st):
            with torch.cuda.stream(stream):
                for i in range(20):
                    out.append(fn(i, st))

        def states():
            return (make(), make()) if make else (None, None)
        sa, sb = states()
        torch.cuda.synchronize()
        seq_a, seq_b = [], []
        loop(fa, torch.cuda.current_stream(), seq_a, sa)
        torch.cuda.synchronize()
        loop(fb, torch.cuda.current_stream(), seq_b, sb)
        torch.cuda.synchronize()
        want_a, want_b = flat(seq_a), flat(seq_b)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        sa, sb = states()
        torch.cuda.synchronize()
        got_a, got_b = [], []
        for i in range(20):                               # alternately, nothing waited for in between
            with torch.cuda.stream(s1):
                got_a.append(fa(i, sa))
            with torch.cuda.stream(s2):
                got_b.append(fb(i, sb))
        torch.cuda.synchronize()
        same(name, "first handle, alternating", want_a, flat(got_a), ("sequential", "in flight"))
        same(name, "second handle, alternating", want_b, flat(got_b), ("sequential", "in flight"))
        sa, sb = states()
        torch.cuda.synchronize()
        got_a, got_b = [], []
        ta = threading.Thread(target=loop, args=(fa, s1, got_a, sa))
        tb = threading.Thread(target=loop, args=(fb, s2, got_b, sb))
        ta.start(); tb.start(); ta.join(); tb.join()
        torch.cuda.synchronize()
        assert len(got_a) == len(got_b) == 20, "a thread ended early"
        same(name, "first handle, two threads", want_a, flat(got_a), ("sequential", "threaded"))
        same(name, "second handle, two threads", want_b, flat(got_b), ("sequential", "threaded"))
        print("  %s: 20 alternating rounds and 20 rounds in two threads == the sequential results" % name)
    # ---- mi355asr_last_error is thread-local: a refusal in one thread leaves the other thread's message alone
    lib = _lib.lib()
    first_done, second_done, seen = threading.Event(), threading.Event(), {}

    def refused_first():
        try:
            ctc_loss(np.zeros((1, 1200, 8), np.float32), np.zeros((1, 512), np.int32))
        except _lib.Mi355AsrError:
            pass
        seen["own"] = lib.mi355asr_last_error().decode()
        first_done.set()
        second_done.wait(30)
        seen["after"] = lib.mi355asr_last_error().decode()

    def refused_second():
        first_done.wait(30)
        try:
            m.recognize(xs[0], wav_lengths=np.array([0, 32000], np.int32))
        except _lib.Mi355AsrError:
            pass
        seen["other"] = lib.mi355asr_last_error().decode()
        second_done.set()
    t1, t2 = threading.Thread(target=refused_first), threading.Thread(target=refused_second)
    t1.start(); t2.start(); t1.join(); t2.join()
    assert "built for up to" in seen["own"] and "wav_len" in seen["other"] and seen["after"] == seen["own"] != seen["other"], seen
    print("  mi355asr_last_error: %r stayed in its thread after %r in the other" % (seen["own"][:60], seen["other"][:60]))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    t0 = time.time()
    fn = globals()["step_" + name]
    fn(*sys.argv[2:2 + fn.__code__.co_argcount])
    torch.cuda.synchronize()
    print("step %s: %.1f s" % (name, time.time() - t0))
    if FINDINGS:
        print("%d findings:\n  %s" % (len(FINDINGS), "\n  ".join(FINDINGS)))
        sys.exit(1)
    print("step %s ok" % name)
