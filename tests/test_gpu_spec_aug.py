"""spec_aug on the MI355X (mi355asr_spec_aug, augment.SpecAug): against SignalSpecAug restated in float64 (stft_ref.spec_aug) under
the round trip's bound, with centres at the four corners of the spectrum and every window; without centres the plain round trip
bit for bit; short rows passed through; the count limit; int16, repeatability, row independence; the two hooks."""
import ctypes
import functools
import random

import numpy as np
import pytest

import stft_ref as sr
from stft_cases import U24, bits, device, pair_case, signal, worst_ratio
from test_gpu_stft_pair import C_Y

pytestmark = pytest.mark.gpu

GEO = (1024, 800, 160)
# |dy[n]| <= C_Y 2^-24 A[n], the round trip's constant (test_gpu_stft_pair.py): the masked spectrum is bounded by the unmasked one.
# Measured on the MI355X: 0.0464 (windows 0 and 10), 0.0373 (window 1), 0.0459 (513 centres on 1027 frames).


def corners(F, extra=()):
    """(h_, w_) at the four corners of a [513, F] spectrum, and `extra`"""
    return np.array([(0, 0), (512, 0), (0, F - 1), (512, F - 1)] + list(extra), np.int32).reshape(-1, 2) if F else np.zeros((0, 2), np.int32)


def centres_for(lens, rng):
    out = []
    for n in lens:
        F = sr.n_frames(n, 1024, 160)
        extra = [(int(rng.integers(0, 513)), int(rng.integers(0, F))) for _ in range(min(F, 3))]
        out.append(corners(F, extra))
    return out


@functools.lru_cache(maxsize=None)
def aug_case(window):
    device()
    from tensorflowasr_amd.augment import SpecAug
    c = pair_case(1024)
    ce = centres_for(c["lens"], np.random.default_rng(window))
    ce[3] = np.zeros((0, 2), np.int32)                 # a row with frames and no centre
    y, out_len = SpecAug(window=window)(c["x"], c["lens"], centres=ce)
    return ce, y.cpu().numpy(), out_len.cpu().numpy()


@pytest.mark.parametrize("window", [0, 1, 10])
def test_parity_with_centres_at_the_corners(window):
    c = pair_case(1024)
    ce, y, out_len = aug_case(window)
    assert y.dtype == np.float32 and y.shape == c["x"].shape
    worst, changed = 0.0, 0.0
    for b, n in enumerate(c["lens"]):
        want = sr.spec_aug(c["x"][b, :n], ce[b], window)
        assert out_len[b] == len(want) == (160 * (n // 160) if n >= 513 else n), (b, n)
        assert not y[b, len(want):].any(), (b, n)
        if n < 513:
            assert np.array_equal(y[b, :n], c["x"][b, :n]), (b, n)
            continue
        worst = max(worst, worst_ratio(np.abs(y[b, :len(want)] - want), U24 * sr.ola_scale(c["a"][b], *GEO)))
        changed = max(changed, float(np.abs(want - c["x"][b, :len(want)]).max()))
    print("spec_aug window %d: worst ratio %.4f (the masks move samples by up to %.3f)" % (window, worst, changed))
    assert worst <= C_Y
    assert (changed > 0.01) == (window > 0)            # window 0 zeroes nothing, as the reference's empty slices


def test_no_centres_is_the_plain_round_trip_bit_for_bit():
    device()
    from tensorflowasr_amd.augment import SpecAug
    c = pair_case(1024)
    none = [np.zeros((0, 2), np.int32)] * len(c["lens"])
    y, out_len = SpecAug()(c["x"], c["lens"], centres=none)
    y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
    y0, _ = SpecAug(ratio=0)(c["x"], c["lens"])        # nothing drawn
    assert np.array_equal(bits(y0.cpu().numpy()), bits(y))
    for b, n in enumerate(c["lens"]):
        if n >= 513:
            assert out_len[b] == c["out_len"][b]
            assert np.array_equal(bits(y[b, :out_len[b]]), bits(c["y"][b, :out_len[b]])), (b, n)
        else:
            assert out_len[b] == n and np.array_equal(bits(y[b, :n]), bits(c["x"][b, :n])) and not y[b, n:].any(), (b, n)


def test_513_centres_on_a_1027_frame_row():
    device()
    from tensorflowasr_amd.augment import SpecAug
    n = 1026 * 160 + 5
    x = signal(np.random.default_rng(8), n)
    aug = SpecAug(window=10, ratio=0.5)
    assert aug.frames(n) == 1027
    random.seed(3)
    ce = aug.draw(1027)
    assert ce.shape == (513, 2)
    y, out_len = aug(x, None, centres=[ce])
    want = sr.spec_aug(x, ce, 10)
    assert int(out_len[0]) == len(want) == 1026 * 160
    y = y.cpu().numpy()[0]
    worst = worst_ratio(np.abs(y[:len(want)] - want), U24 * sr.ola_scale(sr.frame_l1(x, *GEO), *GEO))
    print("spec_aug 513 centres: worst ratio %.4f" % worst)
    assert worst <= C_Y and not y[len(want):].any()
    # drawn inside the call under the same seed: the same centres, the same bits
    random.seed(3)
    y2, _ = aug(x)
    assert np.array_equal(aug.last[0], ce) and np.array_equal(bits(y2.cpu().numpy()[0]), bits(y))
    # one frame more asks for 514 bins: the reference's random.sample raises, and so does this, naming the row
    with pytest.raises(ValueError, match="row 1"):
        aug(np.zeros((2, 164320), np.float32), [4000, 164320])


def test_514_centres_are_refused_and_nothing_is_launched():
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.zeros((2, 4000), dtype=torch.float32, device="cuda:0")
    ln = torch.tensor([4000, 4000], dtype=torch.int32, device="cuda:0")
    ce = torch.zeros((2, 514, 2), dtype=torch.int32, device="cuda:0")
    y = torch.full((2, 4000), 7.0, dtype=torch.float32, device="cuda:0")
    wb = ctypes.c_size_t()
    assert lib.mi355asr_spec_aug_workspace_bytes(2, 4000, ctypes.byref(wb)) == 0 and wb.value >= 2 * 26 * 800 * 4
    ws = torch.full((wb.value // 4,), 7.0, dtype=torch.float32, device="cuda:0")
    call = lambda counts, window, nbytes: lib.mi355asr_spec_aug(
        p(x), 0, p(ln), 2, 4000, p(ce), 514, p(torch.tensor(counts, dtype=torch.int32, device="cuda:0")), window, p(y), 4000, p(ws),
        nbytes, None)
    assert call([513, 514], 10, wb.value) == -1 and b"row 1 has 514" in lib.mi355asr_last_error()
    assert call([-1, 0], 10, wb.value) == -1
    assert call([0, 0], -1, wb.value) == -1 and b"negative" in lib.mi355asr_last_error()
    assert call([0, 0], 10, wb.value - 16) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((ws == 7.0).all())
    assert call([513, 513], 10, wb.value) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any())


def test_int16_repeats_and_rows_are_independent():
    device()
    from tensorflowasr_amd.augment import SpecAug
    c = pair_case(1024)
    ce, y, out_len = aug_case(10)
    aug = SpecAug(window=10)
    assert np.array_equal(bits(aug(c["x"], c["lens"], centres=ce)[0].cpu().numpy()), bits(y))
    for b, n in enumerate(c["lens"]):
        y1, l1 = aug(c["x"][b, :n], None, centres=[ce[b]])
        assert int(l1[0]) == out_len[b] and np.array_equal(bits(y1.cpu().numpy()[0, :out_len[b]]), bits(y[b, :out_len[b]])), (b, n)
    pcm = np.random.default_rng(5).integers(-32768, 32768, c["x"].shape).astype(np.int16)
    yi, li = aug(pcm, c["lens"], centres=ce)
    yf, lf = aug(pcm.astype(np.float32) / 32768, c["lens"], centres=ce)
    assert np.array_equal(li.cpu().numpy(), lf.cpu().numpy()) and np.array_equal(bits(yi.cpu().numpy()), bits(yf.cpu().numpy()))
    assert float(yi.abs().max()) > 0.5
    # poisoned padding never reaches the output
    xp = np.full((len(c["lens"]), c["x"].shape[1] + 7), np.nan, np.float32)
    for b, n in enumerate(c["lens"]):
        xp[b, :n] = c["x"][b, :n]
    yp = aug(xp, c["lens"], centres=ce)[0].cpu().numpy()
    assert np.isfinite(yp).all() and np.array_equal(bits(yp[:, :y.shape[1]]), bits(y)) and not yp[:, y.shape[1]:].any()


def test_offline_stt_batch_with_spec_aug_at_ratio_0(tmp_path):
    from test_gpu_vad import _asr
    from tensorflowasr_amd.augment import SpecAug
    asr = _asr(tmp_path)
    rng = np.random.default_rng(21)
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (24000, 57123, 33335)]
    got = asr.offline_stt_batch(items, augment=SpecAug(ratio=0))
    assert got == asr.offline_stt_batch([w[:160 * (len(w) // 160)] for w in items]) and any(p for p, _ in got)


def test_augmentation_process_batch_is_its_draws_applied_stage_by_stage():
    device()
    import augment_ref as ar
    from test_stft_ref_host import config
    from tensorflowasr_amd.augment import Augmentation, SpecAug, TimeStretch
    rng = np.random.default_rng(6)
    wavs = [signal(rng, n) for n in (4000, 3000, 1100, 6000, 2500, 1025)]
    aug = Augmentation(config(spec_aug=True, speed=True), enable=("spec_aug", "speed"))
    assert aug.available()
    random.seed(2)
    np.random.seed(2)
    got = aug.process_batch(wavs)
    random.seed(2)
    np.random.seed(2)
    drawn = [aug.draw(len(w)) for w in wavs]
    assert {a.key for a, _ in drawn} == {"spec_aug", "speed"}
    for w, (a, d), y in zip(wavs, drawn, got):
        if a.key == "spec_aug":
            v, n = SpecAug(window=10)(w, None, centres=[d["centres"]])
            assert int(n[0]) == (160 * (len(w) // 160) if len(w) >= 513 else len(w))
        else:
            assert 0.9 <= d["rate"] <= 1.2
            v, n = TimeStretch()(w, None, d["rate"])
            assert int(n[0]) == int(round(len(w) / d["rate"]))
        want = ar.quantise(v.cpu().numpy()[0, :int(n[0])])
        assert y.dtype == np.float32 and np.array_equal(y, want) and np.abs(y).max() > 0.01
    # the reference's shipped configuration: spec_aug alone
    only = Augmentation(config(spec_aug=True), enable=("spec_aug",))
    random.seed(9)
    one = only.process(wavs[0])
    random.seed(9)
    _, d = only.draw(len(wavs[0]))
    v, n = SpecAug(window=10)(wavs[0], None, centres=[d["centres"]])
    assert np.array_equal(one, ar.quantise(v.cpu().numpy()[0, :int(n[0])])) and len(one) == 4000
