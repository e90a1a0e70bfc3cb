"""The yardstick of tests/test_gpu_constructor_surface.py, none of it the code under test.

Every comparison there is GPU float32 against the float64 oracle on the same inputs, held to
  (1) the project's contract, 1e-3 absolute (BASELINE north star), and
  (2) err <= max(8 * E32, 16 * 2**-23 * max|ref|), E32 being the error of the ORACLE'S OWN float32 run against its float64 run on
      the same inputs, computed at run time: the form of ctc_yardstick.bound with 8 in place of 4.  No number in it comes from the
      GPU build.  Why 8: for the neighbouring comparisons that tests/golden/parity_ceilings.json pins, the errors the GPU build
      recorded are 2.2 - 3.3 x E32 (waveform -> encoder / logits), about 2.6 x (a block on caller tensors), 1.6 - 1.9 x
      (conv_subsampling) and 0.3 - 1.9 x (melspectrogram); eight leaves a factor of at least 2.4 over the worst healthy ratio, and a
      wrong tile, tap or mask is orders of magnitude above it.
Each comparison prints its figures (`SURFACE <tag> err e32 ratio bound`) and logs them (MI355ASR_PARITY_LOG) before anything is
asserted; a test collects its comparisons in a Ledger and asserts them together, so that one run shows every figure."""
import numpy as np

from helpers import _parity_log, maxdiff

TOL = 1e-3
ULP32 = 2.0 ** -23
MULT = 8.0


def bound(e32, ref):
    return max(MULT * float(e32), 16.0 * ULP32 * float(np.max(np.abs(ref))) if np.size(ref) else 0.0)


def e32_of(ref32, ref64):
    """the float32 oracle run against the float64 one; the float32 run must really have been one"""
    assert ref32.dtype == np.float32, "the oracle's float32 run returned %s" % ref32.dtype
    assert ref64.dtype == np.float64 and ref32.shape == ref64.shape
    return float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0


class Ledger:
    def __init__(self, stage):
        self.stage, self.rows, self.failed = stage, [], []

    def add(self, tag, got, ref64, ref32):
        got = np.asarray(got)
        assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
        assert np.isfinite(got).all(), "%s: the GPU result is not finite" % tag
        e32 = e32_of(ref32, ref64)
        err = maxdiff(got, ref64)
        b = bound(e32, ref64)
        ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
        print("SURFACE %s %s err %.4g e32 %.4g ratio %.2f bound %.4g" % (self.stage, tag, err, e32, ratio, b))
        _parity_log({"surface": self.stage, "tag": tag, "err": err, "e32": e32, "ratio": ratio, "bound": b})
        self.rows.append((tag, err, e32, ratio, b))
        if not err < TOL:
            self.failed.append("%s: err %.4g misses the 1e-3 contract" % (tag, err))
        if not err <= b:
            self.failed.append("%s: err %.4g above max(8 x E32 = %.4g, 16 ulp of max|ref|) = %.4g (ratio %.1f)" % (tag, err, MULT * e32, b, ratio))
        return err

    def expect(self, ok, what):
        if not ok:
            self.failed.append(what)

    def close(self):
        if self.rows:
            worst = max(self.rows, key=lambda r: r[3])
            print("SURFACE %s largest ratio %.2f at %s" % (self.stage, worst[3], worst[0]))
        assert not self.failed, "\n".join(self.failed)


# ---- the waveform case both the test file and its fresh-process steps run ----------------------------------------------------
def waveform_case(ledger, tag, dm, H, hs, k, B, L, ctc_k=None, n_oracle=2, V=70, **extra):
    """ConformerCTC(V, one encoder block, the CTC decoder) from the waveform against co.conformer_encoder / co.ctc_decoder on the first
    n_oracle utterances, and the greedy ids as test_conformer_m_and_l_parity checks them.  extra: reduction_factor, n_mels, ..."""
    from helpers import argmax_mismatch_report, co, waves
    from tensorflowasr_amd.models import ConformerCTC
    ctc_k = k if ctc_k is None else ctc_k
    cfg = dict(co.CONFORMER_S, dmodel=dm, num_heads=H, head_size=hs, kernel_size=k, num_blocks=1, ctcdecoder_kernel_size=ctc_k, **extra)
    w = co.encoder_weights(cfg, seed=1)
    w.update(co.ctc_decoder_weights(cfg, V, seed=2))
    m = ConformerCTC(V, dmodel=dm, num_blocks=1, head_size=hs, num_heads=H, kernel_size=k, ctcdecoder_kernel_size=ctc_k, **extra)
    m.load_weights(w, by_name=False)
    x = waves(B, L, 3)
    n = min(n_oracle, B)
    enc = m.encode(x)
    logits, amax = m.ctc_logits(enc, return_argmax=True)
    enc, logits, amax = enc.cpu().numpy(), logits.cpu().numpy(), amax.cpu().numpy()
    enc64 = co.conformer_encoder(x[:n].astype(np.float64), w, cfg)
    log64 = co.ctc_decoder(enc64, w, cfg)
    enc32 = co.conformer_encoder(x[:n], w, cfg, dtype=np.float32)
    log32 = co.ctc_decoder(enc32, w, cfg, dtype=np.float32)
    assert enc.shape[1:] == enc64.shape[1:], (enc.shape, enc64.shape)
    ledger.add(tag + " encoder", enc[:n], enc64, enc32)
    ledger.add(tag + " logits", logits[:n], log64, log32)
    # (into the ledger, not asserted here: the caller's close() shows every figure and every failure of the run together)
    bad = [b for b in argmax_mismatch_report(logits[:n], log64) if b[1] > 1e-3]
    ledger.expect(not bad, "%s: arg-max differs on frames the oracle decides by more than 1e-3: %s" % (tag, bad[:10]))
    ledger.expect((amax == logits.argmax(-1)).all(), "%s: the head's arg-max is not that of its own logits" % tag)
    ids, lens = m.recognize(x)
    rid, rlen = co.ctc_greedy(logits, [logits.shape[1]] * B, V - 1)
    ledger.expect((ids.cpu().numpy() == rid).all() and (lens.cpu().numpy() == rlen).all(), "%s: recognize() ids differ from the greedy collapse of the logits" % tag)
    return enc.shape[1]
