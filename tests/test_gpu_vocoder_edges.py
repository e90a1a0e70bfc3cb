"""The phase vocoder on the MI355X at its edges (mi355asr_phase_vocoder, augment.TimeStretch), under test_gpu_time_stretch.py's
bounds and constants, unchanged, against the same float64 oracle (stft_ref.phase_vocoder, stft_ref.time_stretch): both sizes the
library takes, (2048, 2048, 512) and (1024, 800, 160) -- the phase advance per hop 2 pi ((160 k) mod 1024) / 1024 of the second is
compared with something here for the first time --, spectra of 1, 2, 31 and 1 200 frames (a 10 s utterance has 313 at hop 512 and
1 001 at hop 160), rates above the frame count (one output frame: frame 0 of the input), rates whose steps reach an integer only
after rounding (1/3, 0.1), the last output frames, which interpolate against the two zero frames past the end, NaN in the frames
of the buffer past a row's count, one ragged call over all four frame counts, and a second, sharper figure over the last tenth of
the long rows' output frames, where the (t + 1) weight of the bound leaves the most room and the fp32 phase accumulator with its
two-float 2 pi has wrapped the most often.  The stretch end to end on 40 000 and 5 000 samples (79 and 10 frames).  Broadband
noise only (test_gpu_time_stretch.py says why).

Measured on the MI355X (first run; C_V = 16, C_S = 4), worst ratio at (2048, 2048, 512) / (1024, 800, 160):
    1 frame,  rates 0.3, 1.0, 3.0                              1.29, 0.73, 0.73 / 3.10, 0.73, 0.73
    2 frames, rates 0.7, 2.0, 2.5                              3.30, 0.73, 0.73 / 2.89, 0.73, 0.73
    31 frames, rates 1/3, 0.1, 0.7, 1.0000001, 3.0             4.34, 5.92, 3.58, 2.64, 3.62 / 4.35, 5.93, 3.56, 3.04, 2.92
    31 frames, rates 31.0, 40.0 (one frame out)                0.73, 0.73 / 0.73, 0.73
    1 200 frames, rates 0.5, 0.9, 1/3, 1.2, 2.0                3.33, 3.33, 3.94, 2.89, 3.03 / 3.90, 3.84, 4.10, 3.32, 3.20
    the last tenth of those rows' output frames                0.5567 / 0.5119 (C_V_TAIL = 4)
    the stretch, 40 000 samples at 0.9, 1.2, 1/3               0.4801, 0.2700, 0.6461
    the stretch, 5 000 samples at 0.9, 1.2, 2.0                1.4519, 0.4697, 0.3724
(0.73 is the one-frame output: the rounding of |D| cos(angle D), sin(angle D) against D itself.)"""
import functools

import numpy as np
import pytest

import stft_ref as sr
from stft_cases import U24, bits, device, signal, worst_ratio
from test_gpu_time_stretch import C_S, C_V, vocoder

pytestmark = pytest.mark.gpu

GEOS = [(2048, 2048, 512), (1024, 800, 160)]
CASES = {1: [0.3, 1.0, 3.0],
         2: [0.7, 2.0, 2.5],
         31: [1.0 / 3.0, 0.1, 0.7, 1.0000001, 3.0, 31.0, 40.0],
         1200: [0.5, 0.9, 1.0 / 3.0, 1.2, 2.0]}
RAGGED = {1: 0.3, 2: 0.7, 31: 0.1, 1200: 0.9}   # the ragged call: one rate of CASES per frame count
# the worst ratio of the bound above over the last tenth of the output frames of the 1 200-frame rows: four times the value of the
# first run on the MI355X against the float64 oracle, rounded up to a power of two, and never above C_V.  Measured: 0.5567 at
# (2048, 2048, 512) and 0.5119 at (1024, 800, 160), both at rate 2.0 (0.42 to 0.50 at the other rates); over the whole rows the
# same runs give 2.9 to 4.1.
C_V_TAIL = 4.0


@functools.lru_cache(maxsize=None)
def spectrum(geo, F):
    """complex64 [F, bins]: the first F frames of the STFT of noise"""
    n_fft, _, hop = geo
    rng = np.random.default_rng(1000 * F + hop)
    D = sr.stft(signal(rng, max(hop * (F - 1) + 100, n_fft // 2 + 1)), *geo)[:F].astype(np.complex64)
    assert D.shape == (F, n_fft // 2 + 1)
    return D


@functools.lru_cache(maxsize=None)
def oracle(geo, F, rate):
    return sr.phase_vocoder(spectrum(geo, F), rate, geo[2], geo[0])


@functools.lru_cache(maxsize=None)
def case(geo, F):
    """every rate of CASES[F] in one call, each row in a buffer of F + 3 frames whose last three are NaN -> (O, counts)"""
    D = np.concatenate([spectrum(geo, F), np.full((3, geo[0] // 2 + 1), np.nan, np.complex64)])
    rates = CASES[F]
    return vocoder(np.stack([D] * len(rates)), [F] * len(rates), rates, geo)


def ratio(got, want, first=0):
    """worst |got - want| / (2^-23 (t + 1) |want|) over the frames from `first` on"""
    weight = 2.0 ** -23 * np.arange(1, len(want) + 1)[:, None]
    return worst_ratio(np.abs(got - want)[first:], (weight * np.abs(want))[first:])


@pytest.mark.parametrize("F", sorted(CASES))
@pytest.mark.parametrize("geo", GEOS)
def test_vocoder_at_every_frame_count_and_rate(geo, F):
    O, tc = case(geo, F)
    D = spectrum(geo, F)
    assert np.isfinite(O.view(np.float32)).all()          # the NaN frames past the count are never read
    assert O.shape[1] >= int(tc.max()) + 2
    for b, rate in enumerate(CASES[F]):
        want = oracle(geo, F, rate)
        T = len(want)
        assert tc[b] == T == sr.stretch_frames(F, rate) and not O[b, T:].any(), (rate, T)
        worst = ratio(O[b, :T], want)
        print("vocoder %s, %d frames, rate %.7g: %d frames out, worst ratio %.4f" % (geo, F, rate, T, worst))
        assert worst <= C_V, rate
        if rate >= F:                                   # one step, at 0: frame 0 of the input
            assert T == 1 and ratio(O[b, :1], D[:1].astype(np.complex128)) <= C_V, rate
        else:
            assert T > 1


@pytest.mark.parametrize("geo", GEOS)
def test_the_last_tenth_of_the_long_rows(geo):
    O, tc = case(geo, 1200)
    worst = 0.0
    for b, rate in enumerate(CASES[1200]):
        want = oracle(geo, 1200, rate)
        T = len(want)
        r = ratio(O[b, :T], want, first=T - T // 10)
        print("vocoder %s, 1200 frames, rate %.7g: worst ratio over frames %d .. %d: %.4f" % (geo, rate, T - T // 10, T - 1, r))
        worst = max(worst, r)
    print("vocoder %s: worst ratio over the last tenth = %.4f" % (geo, worst))
    assert worst <= C_V_TAIL <= C_V


@pytest.mark.parametrize("geo", GEOS)
def test_ragged_rows_equal_their_solo_calls(geo):
    bins = geo[0] // 2 + 1
    Fs = sorted(RAGGED)
    D = np.full((len(Fs), max(Fs), bins), np.nan, np.complex64)
    for b, F in enumerate(Fs):
        D[b, :F] = spectrum(geo, F)
    rates = [RAGGED[F] for F in Fs]
    O, tc = vocoder(D, Fs, rates, geo)
    assert np.isfinite(O.view(np.float32)).all()
    O2, _ = vocoder(D, Fs, rates, geo)
    assert np.array_equal(bits(O2), bits(O))
    for b, F in enumerate(Fs):
        O1, t1 = case(geo, F)
        k = CASES[F].index(RAGGED[F])
        assert tc[b] == t1[k] and not O[b, tc[b]:].any(), F
        assert np.array_equal(bits(O[b, :tc[b]]), bits(O1[k, :tc[b]])), F


STRETCH_LENS = [40000, 5000]


@pytest.mark.parametrize("rates", [0.9, 1.2, (1.0 / 3.0, 2.0)])
def test_time_stretch_end_to_end_on_a_long_row(rates):
    device()
    from tensorflowasr_amd.augment import TimeStretch
    N_FFT, HOP = 2048, 512
    x = signal(np.random.default_rng(78), (2, max(STRETCH_LENS)))
    ts = TimeStretch()
    y, out_len = ts(x, STRETCH_LENS, rates)
    y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
    per_row = np.broadcast_to(np.asarray(rates, np.float64).reshape(-1), (2,))
    worst = 0.0
    for b, n in enumerate(STRETCH_LENS):
        rate = float(per_row[b])
        want = sr.time_stretch(x[b, :n], rate)
        want_len = int(round(n / rate))
        assert out_len[b] == want_len == len(want) and not y[b, want_len:].any(), (b, n)
        out = sr.phase_vocoder(sr.stft(x[b, :n], N_FFT, N_FFT, HOP), rate, HOP, N_FFT)
        scale = sr.ola_scale(sr.spec_l1(out, N_FFT), N_FFT, N_FFT, HOP, length=want_len, weights=np.arange(1, len(out) + 1))
        r = worst_ratio(np.abs(y[b, :want_len] - want), U24 * scale)
        print("time stretch, %d samples at rate %.4g: %d frames out, worst ratio %.4f" % (n, rate, len(out), r))
        worst = max(worst, r)
    assert worst <= C_S
    y1, l1 = ts(x[0, :STRETCH_LENS[0]], None, float(per_row[0]))
    assert int(l1[0]) == out_len[0] and np.array_equal(bits(y1.cpu().numpy()[0, :out_len[0]]), bits(y[0, :out_len[0]]))
