"""The GPU side of tests/test_gpu_dense_edges.py: the comparisons themselves (the test file calls them in its own process) and the
fresh-process legs (the switches they set are read once per process): python dense_edges_gpu_steps.py <leg> [<out.npz>].
A leg prints `SURFACE ...` lines, writes the raw outputs the parent compares bit for bit, and ends with `step <leg> ok`.

DENSE_EDGES_ORACLE_DIR (set by the test file): oracle results are kept there, so that a leg does not compute again what the parent
already has."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import dense_edges as de  # noqa: E402
from helpers import _parity_log, argmax_mismatch_report, co, encoder_kwargs, small_cfg  # noqa: E402
from surface_yardstick import Ledger  # noqa: E402

_MODELS, _ORACLE = {}, {}


# ---- models and oracles: one of each per process ---------------------------------------------------------------------------------
def model(d, n, V=de.V_DENSE, mode="float32", expected_rows=None):
    key = (d, n, V, mode, expected_rows)
    if key not in _MODELS:
        from tensorflowasr_amd.models import CTCDecoder
        m = CTCDecoder(num_classes=V, dmodel=d, num_blocks=n, head_size=64, num_heads=de.HEADS[d], kernel_size=32, gemm_dtype=mode)
        if expected_rows is not None:
            m._h.set_expected_rows(expected_rows)
        m.load_weights(de.weights(d, n, V), by_name=False)
        _MODELS[key] = m
    return _MODELS[key]


def _kept(name, compute):
    """compute() -> a tuple of arrays, kept in this process and, where the parent named a directory, on disk"""
    if name in _ORACLE:
        return _ORACLE[name]
    path = os.environ.get("DENSE_EDGES_ORACLE_DIR")
    path = os.path.join(path, name + ".npz") if path else None
    if path and os.path.exists(path):
        z = np.load(path)
        _ORACLE[name] = tuple(z["a%d" % i] for i in range(len(z.files)))
    else:
        _ORACLE[name] = tuple(compute())
        if path:
            tmp = "%s.%d.tmp.npz" % (path, os.getpid())
            np.savez(tmp, **{"a%d" % i: a for i, a in enumerate(_ORACLE[name])})
            os.replace(tmp, path)
    return _ORACLE[name]


def oracle(d, n, M, V=de.V_DENSE):
    """(input, float64 logits, the oracle's own float32 logits) of a case"""
    x = de.case_input(d, n, M, V)

    def compute():
        w, cfg = de.weights(d, n, V), de.cfg_for(d, n)
        return co.ctc_decoder(x.astype(np.float64), w, cfg), co.ctc_decoder(x, w, cfg, dtype=np.float32)
    r64, r32 = _kept("f32_d%d_n%d_M%d_V%d" % (d, n, M, V), compute)
    return x, r64, r32


def bf16_oracle(d, n, M):
    """(input, float64 logits with both operands of every dense layer rounded to bf16, the un-rounded float64 logits)"""
    x = de.case_input(d, n, M)

    def compute():
        w, cfg = de.weights(d, n, de.V_DENSE), de.cfg_for(d, n)
        co.GEMM_ROUND_BF16 = True
        try:
            r = co.ctc_decoder(x.astype(np.float64), w, cfg)
        finally:
            co.GEMM_ROUND_BF16 = False
        return (r,)
    return x, _kept("bf16_d%d_n%d_M%d" % (d, n, M), compute)[0], oracle(d, n, M)[1]


# ---- what a call ran -------------------------------------------------------------------------------------------------------------
def schemes(m):
    """{kernel category: MI355ASR_SCHEME_* of its last launch on this handle, -1: never launched}"""
    from tensorflowasr_amd import _lib
    nk = len(_lib.KERNEL_NAMES)
    out = (ctypes.c_int32 * nk)()
    _lib.check(m._h.lib.mi355asr_profile_schemes(m._h.ptr, out, nk))
    return dict(zip(_lib.KERNEL_NAMES, (int(v) for v in out)))


def ring_min_rows():
    return int(os.environ.get("MI355ASR_RING_MIN_M", de.RING_MIN_M))


def assert_family(tag, m, d, n, M, family):
    """family "rings": a handle with slab rings -- gemm16 (exact fp32 products) below ring_min_rows(), gemm_ring_kernel (three bf16
    terms) from there, for the block's five dense categories and the class head; a launcher that declined would leave F32 behind
    (launch_gemm16 falls through to launch_gemm16_f32).  The projection holds a ring pack in the bf16 mode only (pack_stack,
    csrc/weights.hip): in fp32 it is a gemm16 launch at every row count.  "none": no rings on the handle -- the fp32 chains of
    dmodel 256 or gemm16 at dmodel 512, fp32 everywhere.  "bf16": the bf16 mode, one bf16 term everywhere."""
    sch = schemes(m)
    cats = (de.DENSE if n else ()) + de.STACK
    got = {c: sch[c] for c in cats}
    if family == "rings":
        ring = M >= ring_min_rows()
        want = {c: (de.BF16X3 if ring else de.F32) for c in cats}
        want["ctc_project"] = de.F32
    elif family == "none":
        want = {c: de.F32 for c in cats}
    else:
        want = {c: de.BF16 for c in cats}
    assert got == want, "%s: M = %d ran %s, expected %s" % (tag, M, got, want)
    return got


def run_dense_case(led, d, n, M, family, V=de.V_DENSE, expected_rows=None, return_logits=True, fence=None):
    """one call of CTCDecoder(V, d, n blocks) on the case's input against the float64 oracle through the ledger -> (logits, arg-max)"""
    m = model(d, n, V, expected_rows=expected_rows)
    x, r64, r32 = oracle(d, n, M, V)
    tag = "d%d n%d M%d V%d" % (d, n, M, V)
    if fence is not None:
        m._h._ws = None                                  # a workspace of this call's own size, allocated (and poisoned) by the fence
    lg, am = m(x, return_argmax=True, return_logits=return_logits)
    am = am.cpu().numpy()
    lg = lg.cpu().numpy() if return_logits else None
    assert_family(tag, m, d, n, M, family)
    assert am.shape == r64.shape[:2], (tag, am.shape)
    if return_logits:
        led.add(tag, lg, r64, r32)
        led.expect(np.array_equal(am, lg.argmax(-1)), "%s: the head's arg-max is not that of its own logits" % tag)
    # only frames the oracle decides by more than 1e-3 count (helpers.argmax_mismatch_report)
    amax_as_logits = np.zeros(r64.shape, np.float32)
    np.put_along_axis(amax_as_logits, am[..., None].astype(np.int64), 1.0, axis=-1)
    bad = [b for b in argmax_mismatch_report(amax_as_logits, r64) if b[1] > de.MARGIN]
    led.expect(not bad, "%s: arg-max differs on frames the oracle decides by more than 1e-3: %s" % (tag, bad[:10]))
    share = de.undecided_share(r64)
    led.expect(share <= de.MAX_EXCUSED, "%s: %.4f of the frames are undecided, above %.4f" % (tag, share, de.MAX_EXCUSED))
    return lg, am


def run_bf16_case(d, n, M):
    """bf16 mode against the rounding oracle: the project's bounds for logits (max < 4e-2, mean < 3e-3) -> the line it printed"""
    m = model(d, n, mode="bfloat16")
    x, ref, plain = bf16_oracle(d, n, M)
    lg, am = m(x, return_argmax=True)
    lg, am = lg.cpu().numpy(), am.cpu().numpy()
    assert_family("bf16 d%d n%d" % (d, n), m, d, n, M, "bf16")
    assert np.isfinite(lg).all()
    e, ep = np.abs(lg - ref), np.abs(lg - plain)
    line = "SURFACE bf16 d%d n%d M%d: vs rounding oracle max %.3g (bound 4e-2) mean %.3g (bound 3e-3); vs exact oracle mean %.3g" % (d, n, M, e.max(), e.mean(), ep.mean())
    print(line)
    _parity_log({"surface": "bf16", "tag": "d%d n%d M%d" % (d, n, M), "max": float(e.max()), "mean": float(e.mean()), "mean_vs_exact": float(ep.mean())})
    assert e.max() < 4e-2 and e.mean() < 3e-3, line
    assert ep.mean() > e.mean(), "closer to the un-rounded oracle than to the rounding one: not the bf16 path? " + line
    assert np.array_equal(am, lg.argmax(-1)), "the head's arg-max is not that of its own logits"
    return line


# ---- the subsampling conv ------------------------------------------------------------------------------------------------------------
def encoder(d):
    key = ("enc", d)
    if key not in _MODELS:
        from tensorflowasr_amd.models import ConformerEncoder
        cfg = small_cfg(1, co.CONFORMER_M if d == 256 else co.CONFORMER_L)
        w = co.encoder_weights(cfg, seed=3)
        e = ConformerEncoder(**encoder_kwargs(cfg))
        e.load_weights(w, by_name=False)
        _MODELS[key] = (e, w)
    return _MODELS[key]


def subconv_oracle(d, F):
    mel = de.subconv_mel(F)
    w = encoder(d)[1]
    r64, r32 = _kept("subconv_d%d_F%d" % (d, F), lambda: (co.conv_subsampling(mel.astype(np.float64), w), co.conv_subsampling(mel, w)))
    return mel, r64, r32


def run_subconv(led, d, scheme):
    """ConformerEncoder.conv_subsampling at every F of the table against co.conv_subsampling; scheme: what the `subconv` category
    must report (three bf16 terms for caller-supplied features, two fp16 terms under MI355ASR_SUBCONV_TERMS=22) -> {F: output}"""
    e = encoder(d)[0]
    out = {}
    for F in de.SUBCONV_F:
        mel, r64, r32 = subconv_oracle(d, F)
        got = e.conv_subsampling(mel).cpu().numpy()
        sch = schemes(e)["subconv"]
        assert sch == scheme, "d%d F%d: the subsampling conv ran scheme %d, expected %d" % (d, F, sch, scheme)
        assert got.shape == (de.SUBCONV_B, de.subconv_geometry(F)[1], d), (F, got.shape)
        led.add("d%d F%d" % (d, F), got, r64, r32)
        out[F] = got
    return out


# ---- the legs ---------------------------------------------------------------------------------------------------------------------
def leg_ring_off(save):
    """MI355ASR_GEMM_RING=0: no slab rings anywhere -- the fp32 chains (dmodel 256) and gemm16 (512) above the crossover"""
    led = Ledger("ring_off")
    for d in de.DMODELS:
        for n in (0, 1):
            for M in de.RING_OFF_M:
                run_dense_case(led, d, n, M, "none")
    led.close()


def leg_forced(save):
    """MI355ASR_RING_MIN_M=1 and one forced launch shape: the ring at 129 / 257 / 385 rows"""
    assert ring_min_rows() == 1
    led = Ledger("forced[%s]" % ",".join("%s=%s" % (k[len("MI355ASR_RING_"):], v) for k, v in sorted(os.environ.items()) if k.startswith("MI355ASR_RING_") and k != "MI355ASR_RING_MIN_M"))
    for d in de.DMODELS:
        for n in (0, 1):
            for M in de.FORCED_M:
                lg, am = run_dense_case(led, d, n, M, "rings")
                save["d%d_n%d_M%d_lg" % (d, n, M)], save["d%d_n%d_M%d_am" % (d, n, M)] = lg, am
    led.close()


def leg_ranges(save):
    """MI355ASR_RING_MIN_M=1 and a forced number of class ranges: the ring head of 1 332 classes (11 chunks) at 257 and 1 501 rows"""
    assert ring_min_rows() == 1
    led = Ledger("ranges[%s]" % os.environ["MI355ASR_RING_HEAD_RANGES"])
    for M in de.HEAD_M:
        lg, am = run_dense_case(led, 256, 0, M, "rings", V=de.HEAD_RANGES_V)
        _, am0 = run_dense_case(led, 256, 0, M, "rings", V=de.HEAD_RANGES_V, return_logits=False)
        save["M%d_lg" % M], save["M%d_am" % M], save["M%d_am_nologits" % M] = lg, am, am0
    led.close()


def leg_subconv(save):
    led = Ledger("subconv[%s]" % ",".join("%s=%s" % (k[len("MI355ASR_SUBCONV_"):], v) for k, v in sorted(os.environ.items()) if k.startswith("MI355ASR_SUBCONV_")))
    for d in de.DMODELS:
        for F, got in run_subconv(led, d, de.F16X2).items():
            save["d%d_F%d" % (d, F)] = got
    led.close()


if __name__ == "__main__":
    name = sys.argv[1]
    for k, v in de.LEGS[name].items():
        assert os.environ.get(k) == v, "leg %s needs %s=%s" % (name, k, v)
    save = {}
    leg = leg_ring_off if name == "ring_off" else leg_forced if name.startswith("forced_") else leg_ranges if name.startswith("ranges") else leg_subconv
    leg(save)
    if len(sys.argv) > 2 and save:
        np.savez(sys.argv[2], **save)
    print("step %s ok" % name)
