"""Hz and Mask on the MI355X (augment.Hz, augment.Mask, mi355asr_mask_zone) against the reference's own expressions (iir_ref.hz_ref,
mask_ref) and the fixture recorded from its SignalHz and SignalMask (tests/golden/hz_mask_ref.npz).  Hz runs second-order sections
where the reference runs the transfer function, so it is held to 2^-24 |y| + 8 (D + D_ba): D and D_ba are SciPy's own distances
from long-double evaluations of the sections and of the transfer function.  Quantised outputs may differ from the reference's by
one step of 2^-15 on at most 0.1 % of a row's samples.  Mask is exact.

Measured on the MI355X: worst (|y - y_ref| - 2^-24 |y_ref|) / (D + D_ba) = 0.251 for Hz against filtfilt(b, a, x); 0 of 6 970 quantised
samples differ from the quantised reference (and 0 between SciPy's sections and their long-double evaluation)."""
import random

import numpy as np
import pytest
from scipy import signal

import iir_ref as ir
from iir_cases import PADLEN, batch, bits, check_bound, check_quantised, device, filtfilt_refs, poisoned, tf_refs

pytestmark = pytest.mark.gpu


def test_hz_against_the_references_transfer_function_call():
    device()
    from tensorflowasr_amd.augment import Hz
    c = batch()
    hz = Hz()
    y, out_len = hz(c["x"], c["lens"], starts=c["starts"], noise=False)
    y = y.cpu().numpy()
    assert np.array_equal(out_len.cpu().numpy(), c["lens"]) and np.array_equal(hz.last, c["starts"])
    yn = hz(c["x"], c["lens"], starts=c["starts"], noise=c["u"])[0].cpu().numpy()
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        want, D_ba = tf_refs()[b]
        D = filtfilt_refs()[b][1]
        worst = max(worst, check_bound(y[b, :n], np.asarray(want, ir.LD), D, D_ba))
        assert np.array_equal(want + c["us"][b] * 0.001, ir.hz_ref(c["rows"][b], c["starts"][b], c["us"][b]))
        check_bound(yn[b, :n], np.asarray(ir.hz_ref(c["rows"][b], c["starts"][b], c["us"][b]), ir.LD), D, D_ba + 2.0 ** -52)
        assert not y[b, n:].any() and not yn[b, n:].any()
    print("Hz against filtfilt(b, a, x): worst (|y - y_ref| - 2^-24 |y_ref|) / (D + D_ba) = %.3f" % worst)
    # one start for all rows is one shared filter: the same bits as that start per row
    a = hz(c["x"], c["lens"], starts=0.35, noise=False)[0].cpu().numpy()
    b = hz(c["x"], c["lens"], starts=[0.35] * len(c["lens"]), noise=False)[0].cpu().numpy()
    assert np.array_equal(bits(a), bits(b))


def test_hz_quantised_against_the_quantised_reference():
    device()
    from tensorflowasr_amd.augment import Hz
    c = batch()
    y = Hz()(c["x"], c["lens"], starts=c["starts"], noise=c["u"], quantise=True)[0].cpu().numpy()
    total = 0
    for b, n in enumerate(c["lens"]):
        want = ir.quantise(ir.hz_ref(c["rows"][b], c["starts"][b], c["us"][b]))
        # the yardsticks themselves: SciPy's sections and their long-double evaluation quantise alike on these inputs
        own = ir.quantise(signal.sosfiltfilt(c["sos"][b], c["rows"][b], padlen=PADLEN) + c["us"][b] * 0.001) != \
            ir.quantise(np.asarray(filtfilt_refs()[b][0] + ir.LD(0.001) * c["us"][b], np.float64))
        assert own.sum() <= 0.00025 * n, (b, int(own.sum()))
        total += check_quantised(y[b, :n], want)
        assert not y[b, n:].any()
    print("Hz quantised: %d of %d samples differ from the quantised reference" % (total, sum(c["lens"])))


def test_hz_past_the_first_scan_stage():
    """one row whose extended length is SC + 1 positions (1 025 chunks: 17 tiles of the passes, the scan's second stage, the
    short chunk alone in it) at start 0.699 beside one of 6 000 samples at start 0.01, under the bounds above.  Measured on the
    MI355X: worst ratio 1.222 (D_ba, the transfer function's own distance from its long-double evaluation, is of the order of 1e-9 at start 0.699);
    10 of 137 031 quantised samples differ from the quantised reference by one step (allowed: 0.1 % of a row)."""
    device()
    from iir_cases import SC, sections
    from tensorflowasr_amd.augment import Hz
    lens, starts = [SC + 1 - 2 * PADLEN, 6000], [0.699, 0.01]
    rng = np.random.default_rng(41)
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    us = [rng.random(n) for n in lens]
    x, u = poisoned(rows, max(lens) + 7, np.float32), poisoned(us, max(lens) + 7, np.float64)
    hz = Hz()
    y = hz(x, lens, starts=starts, noise=False)[0].cpu().numpy()
    yn = hz(x, lens, starts=starts, noise=u)[0].cpu().numpy()
    yq = hz(x, lens, starts=starts, noise=u, quantise=True)[0].cpu().numpy()
    assert np.isfinite(y).all() and np.isfinite(yn).all() and np.isfinite(yq).all()
    worst = total = 0
    for b, n in enumerate(lens):
        r = rows[b].astype(np.float64)
        ba = signal.butter(3, [starts[b], starts[b] + .3], "bandstop")
        want = signal.filtfilt(*ba, r)
        D_ba = ir.distance(want, ir.filtfilt_ld(*ba, r), r)
        sos = sections(starts[b])
        D = ir.distance(signal.sosfiltfilt(sos, r, padlen=PADLEN), ir.sosfiltfilt_ld(sos, r, PADLEN), r)
        worst = max(worst, check_bound(y[b, :n], np.asarray(want, ir.LD), D, D_ba))
        check_bound(yn[b, :n], np.asarray(ir.hz_ref(r, starts[b], us[b]), ir.LD), D, D_ba + 2.0 ** -52)
        total += check_quantised(yq[b, :n], ir.quantise(ir.hz_ref(r, starts[b], us[b])))
        assert not y[b, n:].any() and not yn[b, n:].any() and not yq[b, n:].any()
    print("Hz past the first scan stage: worst (|y - y_ref| - 2^-24 |y_ref|) / (D + D_ba) = %.3f; %d of %d quantised samples differ"
          % (worst, total, sum(lens)))


def test_hz_returns_short_rows_unchanged_and_draws_when_asked():
    torch = device()
    from tensorflowasr_amd.augment import Hz
    c = batch()
    lens = [21, 1, 0, 22]
    hz = Hz()
    y, out_len = hz(c["x"][:4], lens, starts=c["starts"][:4], noise=False)
    y = y.cpu().numpy()
    assert list(out_len.cpu().numpy()) == lens
    for b in range(3):
        assert np.array_equal(bits(y[b, :lens[b]]), bits(c["x"][b, :lens[b]])) and not y[b, lens[b]:].any()
    assert np.abs(y[3, :22] - c["x"][3, :22]).max() > 1e-3 and not y[3, 22:].any()         # 22 samples are filtered
    # starts and noise drawn: the reference's expression for the start, torch.rand for the noise
    np.random.seed(4)
    torch.manual_seed(4)
    yd = hz(c["x"][4:6], c["lens"][4:6])[0].cpu().numpy()
    np.random.seed(4)
    starts = [float(np.clip(np.random.random(), 0.01, 0.699)) for _ in range(2)]
    assert np.array_equal(hz.last, starts)
    torch.manual_seed(4)
    u = torch.rand((2, c["x"].shape[1]), dtype=torch.float64, device="cuda:0")
    assert np.array_equal(bits(yd), bits(hz(c["x"][4:6], c["lens"][4:6], starts=starts, noise=u)[0].cpu().numpy()))
    assert float(u.min()) >= 0 and float(u.max()) < 1


MASK_LENS = [1, 9, 10, 11, 4001, 300, 0]


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("zone", [(0.0, 1.0), (0.1, 0.9), (0.5, 0.5), (0.9, 0.1)])
def test_mask_is_the_references_expression_bit_for_bit(zone, with_noise):
    device()
    from tensorflowasr_amd.augment import Mask
    rng = np.random.default_rng(13)
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in MASK_LENS]
    rows[4][::7] = 0.0
    rows[4][3::7] = -0.0
    us = [rng.random(n) for n in MASK_LENS]                        # more draws than any zone uses
    x = poisoned(rows, 4009, np.float32)
    u = poisoned(us, 4009, np.float64)
    for ratio in (0.0, 0.3, 1.0):
        m = Mask(zone, ratio, with_noise)
        for quantise in (False, True):
            y, out_len = m(x, MASK_LENS, u=u, quantise=quantise)
            y = y.cpu().numpy()
            assert list(out_len.cpu().numpy()) == MASK_LENS and y.dtype == np.float32 and y.shape == x.shape
            for b, n in enumerate(MASK_LENS):
                s, e = m.span(n)
                want = ir.mask_ref(rows[b], zone, ratio, with_noise, us[b][:max(e - s, 0)])
                if quantise:
                    want = ir.quantise(want)
                assert np.array_equal(bits(y[b, :n]), bits(want.astype(np.float32))), (b, n, ratio, quantise)
                assert not y[b, n:].any()
                if not quantise and n == 4001 and e > s:
                    hit = us[b][:e - s] < ratio            # none at ratio 0, all at ratio 1, about 30 % at 0.3
                    assert hit.mean() == ratio if ratio in (0.0, 1.0) else 0.25 < hit.mean() < 0.35
                    got = y[b, s:e][hit]
                    assert np.array_equal(got, us[b][:e - s][hit].astype(np.float32) if with_noise else np.zeros(hit.sum(), np.float32))
    # a list of per-row draws of exactly e - s values is accepted, and fewer are refused
    m = Mask(zone, 0.3, with_noise)
    spans = [m.span(n) for n in MASK_LENS]
    y2 = m(x, MASK_LENS, u=[us[b][:max(e - s, 0)] for b, (s, e) in enumerate(spans)])[0].cpu().numpy()
    assert np.array_equal(bits(y2), bits(m(x, MASK_LENS, u=u)[0].cpu().numpy()))
    if spans[4][1] > spans[4][0]:
        with pytest.raises(ValueError, match="does not cover"):
            m(x, MASK_LENS, u=u[:, :spans[4][1] - spans[4][0] - 1])


def test_mask_draws_on_the_device_when_no_draws_are_given():
    torch = device()
    from tensorflowasr_amd.augment import Mask
    x = np.full((2, 5000), 0.25, np.float32)
    m = Mask((0.1, 0.9), 0.3, True)
    torch.manual_seed(9)
    y = m(x, [5000, 2000])[0].cpu().numpy()
    torch.manual_seed(9)
    u = torch.rand((2, 5000), dtype=torch.float64, device="cuda:0")
    assert np.array_equal(bits(y), bits(m(x, [5000, 2000], u=u)[0].cpu().numpy()))
    changed = y[0, 500:4500] != 0.25
    assert 0.25 < changed.mean() < 0.35 and not (y[0, :500] != 0.25).any() and not (y[0, 4500:] != 0.25).any()
    assert not y[1, 2000:].any() and not (y[1, 1800:2000] != 0.25).any()


def test_augmentation_process_batch_matches_the_fixture():
    device()
    from test_iir_host import CASES, GOLD, config
    from tensorflowasr_amd.augment import Augmentation
    for key, noise in (("hz", None), ("masking", False), ("masking", True)):
        cfg = config(**{key: True})
        if key == "masking":
            cfg["masking"]["mask_with_noise"] = noise
        aug = Augmentation(cfg, enable=("hz", "masking"))
        for k in CASES:
            random.seed(int(GOLD["seeds"][k]))
            np.random.seed(int(GOLD["seeds"][k]))
            x = GOLD["x%d" % k]
            got = aug.process_batch([x])[0]
            assert got.dtype == np.float32 and got.shape == x.shape
            if key == "hz":
                assert np.random.random() == float(GOLD["hz_next%d" % k])
                check_quantised(got, ir.quantise(GOLD["hz_out%d" % k]))
            else:
                assert np.random.random() == float(GOLD["mask%d_next%d" % (noise, k)])
                assert np.array_equal(bits(got), bits(ir.quantise(GOLD["mask%d_out%d" % (noise, k)]).astype(np.float32)))
    # all rows of a batch in one call each, whichever augmentation a row draws
    aug = Augmentation(config(hz=True, masking=True), enable=("hz", "masking"))
    random.seed(1)
    np.random.seed(1)
    wavs = [GOLD["x%d" % (k % 3)] for k in range(6)]
    drawn = []
    real = aug.draw
    aug.draw = lambda n: drawn.append(real(n)) or drawn[-1]
    out = aug.process_batch(wavs)
    assert {a.key for a, _ in drawn} == {"hz", "masking"}
    for w, (a, d), got in zip(wavs, drawn, out):
        if a.key == "hz":
            check_quantised(got, ir.quantise(ir.hz_ref(w.astype(np.float64), d["start"], d["u"])))
        else:
            want = ir.quantise(ir.mask_ref(w.astype(np.float64), a.zone, a.mask_ratio, a.mask_with_noise, d["u"]))
            assert np.array_equal(bits(got), bits(want.astype(np.float32)))


def test_offline_stt_batch_with_hz(tmp_path):
    from test_gpu_vad import _asr
    from tensorflowasr_amd.augment import Hz
    asr = _asr(tmp_path)
    rng = np.random.default_rng(21)
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (24000, 57123, 33335)]
    np.random.seed(0)
    got = asr.offline_stt_batch(items, augment=Hz())
    assert len(got) == len(items) and all(len(g) == 2 for g in got)
