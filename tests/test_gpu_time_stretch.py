"""The phase vocoder and the time stretch on the MI355X (mi355asr_phase_vocoder, augment.TimeStretch, augment.Speed) against
librosa's restated in float64 (stft_ref.phase_vocoder, stft_ref.time_stretch): the vocoder alone on one uploaded spectrum at every
rate, the stretch end to end on broadband inputs, lengths exactly, repeatability and row independence bit for bit.  No pure tones:
a bin at the float32 rounding floor has no defined phase, which is ill-conditioning of the algorithm and not of a kernel."""
import ctypes
import functools

import numpy as np
import pytest

import stft_ref as sr
from stft_cases import U24, bits, device, signal, worst_ratio

pytestmark = pytest.mark.gpu

N_FFT, HOP, BINS = 2048, 512, 1025
RATES = [0.5, 0.9, 1.0, 1.2, 2.0]
# |d out[k, t]| <= C_V 2^-23 (t + 1) |out[k, t]| (the vocoder alone) and |dy[n]| <= C_S 2^-24 A_s[n] (the stretch; stft_ref.spec_l1
# weighted by t + 1 through stft_ref.ola_scale), against the float64 oracle: four times the worst ratio of the first run on the
# MI355X, rounded up to a power of two.  Measured: vocoder 3.0853 (rate 2.0; 2.87 to 3.05 at the other
# rates), stretch 0.5538 (rate 0.9) and 0.5262 (rate 1.2).  Caps: 64 and 512.
C_V = 16.0
C_S = 4.0


@functools.lru_cache(maxsize=None)
def spectrum():
    """one complex64 spectrum of noise, 31 frames"""
    rng = np.random.default_rng(31)
    return sr.stft(signal(rng, 30 * HOP + 100), N_FFT, N_FFT, HOP).astype(np.complex64)


def vocoder(D, frames, rates, geo=(N_FFT, N_FFT, HOP)):
    """D complex64 [B, Fpad, bins] -> (O [B, Tpad, bins] NumPy, counts); Tpad is two frames more than the longest row's count"""
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    B, BINS = len(D), geo[0] // 2 + 1
    assert D.shape[2] == BINS
    rates = np.ascontiguousarray(rates, np.float64)
    tc = np.array([sr.stretch_frames(F, r) for F, r in zip(frames, rates)], np.int32)
    Tpad = int(tc.max()) + 2
    S = torch.from_numpy(np.ascontiguousarray(D)).to("cuda:0")
    fr = torch.tensor(list(frames), dtype=torch.int32, device="cuda:0")
    O = torch.full((B, Tpad, BINS), 7.0, dtype=torch.complex64, device="cuda:0")
    wb = ctypes.c_size_t()
    _lib.check(lib.mi355asr_phase_vocoder_workspace_bytes(B, ctypes.byref(wb)))
    ws = torch.empty(wb.value // 8, dtype=torch.float64, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.mi355asr_phase_vocoder(p(S), p(fr), B, S.shape[1], *geo, rates.ctypes.data_as(ctypes.c_void_p),
                                          tc.ctypes.data_as(ctypes.c_void_p), p(O), Tpad, p(ws), wb.value, None))
    torch.cuda.synchronize()
    return O.cpu().numpy(), tc


def test_vocoder_alone_at_every_rate():
    D = spectrum()
    assert D.shape == (31, BINS)
    O, tc = vocoder(np.stack([D] * len(RATES)), [31] * len(RATES), RATES)
    for b, rate in enumerate(RATES):
        want = sr.phase_vocoder(D, rate, HOP, N_FFT)
        T = len(want)
        assert tc[b] == T == len(np.arange(0, 31, rate)) and not O[b, T:].any()
        weight = 2.0 ** -23 * np.arange(1, T + 1)[:, None]
        worst = worst_ratio(np.abs(O[b, :T] - want), weight * np.abs(want))
        print("vocoder rate %.1f: %d frames, worst ratio %.4f" % (rate, T, worst))
        assert worst <= C_V <= 64
        if rate == 1.0:                                 # the output is the input, under the same bound
            assert worst_ratio(np.abs(O[b, :T] - D), weight * np.abs(D.astype(np.complex128))) <= C_V
    # the rows were computed as if alone, and the run repeats
    O2, _ = vocoder(np.stack([D] * len(RATES)), [31] * len(RATES), RATES)
    assert np.array_equal(bits(O2), bits(O))
    for b, rate in enumerate(RATES):
        O1, t1 = vocoder(D[None], [31], [rate])
        assert np.array_equal(bits(O1[0, :t1[0]]), bits(O[b, :t1[0]])), rate
    # fewer frames than the buffer holds: the frames past the count are not read
    Dp = np.concatenate([D[:20], np.full((11, BINS), np.nan, np.complex64)])
    O3, t3 = vocoder(Dp[None], [20], [0.9])
    want = sr.phase_vocoder(D[:20], 0.9, HOP, N_FFT)
    assert t3[0] == len(want) and np.isfinite(O3.view(np.float32)).all()
    assert worst_ratio(np.abs(O3[0, :t3[0]] - want), 2.0 ** -23 * np.arange(1, len(want) + 1)[:, None] * np.abs(want)) <= C_V


def test_vocoder_refusals():
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    S = torch.zeros((1, 4, BINS), dtype=torch.complex64, device="cuda:0")
    O = torch.full((1, 8, BINS), 7.0, dtype=torch.complex64, device="cuda:0")
    fr = torch.tensor([4], dtype=torch.int32, device="cuda:0")
    ws = torch.empty(8, dtype=torch.float64, device="cuda:0")
    call = lambda rate, T, geo=(2048, 2048, 512): lib.mi355asr_phase_vocoder(
        p(S), p(fr), 1, 4, *geo, np.array([rate]).ctypes.data_as(ctypes.c_void_p), np.array([T], np.int32).ctypes.data_as(ctypes.c_void_p),
        p(O), 8, p(ws), 64, None)
    assert call(0.0, 4) == -1 and call(-1.0, 4) == -1 and call(float("nan"), 4) == -1 and call(1.0, 9) == -1
    assert call(1.0, 4, (2048, 1024, 512)) == -1
    torch.cuda.synchronize()
    assert bool((O == 7.0).all())
    assert call(1.0, 4) == 0
    torch.cuda.synchronize()
    assert not bool(O.abs().sum() > 0)


def inputs():
    rng = np.random.default_rng(77)
    lens = [5000, 6144, 2561, 1025, 1024, 0]
    x = signal(rng, (len(lens), max(lens)))
    x[1, :3000] *= 1e-4 / 0.3                           # a burst: 1e-4 noise, then 0.3 noise
    return lens, x


@functools.lru_cache(maxsize=None)
def stretch_case(rate):
    device()
    from tensorflowasr_amd.augment import TimeStretch
    lens, x = inputs()
    y, out_len = TimeStretch()(x, lens, rate)
    return lens, x, y.cpu().numpy(), out_len.cpu().numpy()


@pytest.mark.parametrize("rate", [0.9, 1.2])
def test_time_stretch_end_to_end(rate):
    lens, x, y, out_len = stretch_case(rate)
    worst = 0.0
    for b, n in enumerate(lens):
        want_len = int(round(n / rate))
        assert out_len[b] == want_len and not y[b, want_len:].any(), (b, n)
        if n < N_FFT // 2 + 1:                          # no frame (librosa raises there): zeros
            assert not y[b].any()
            continue
        want = sr.time_stretch(x[b, :n], rate)
        assert len(want) == want_len
        out = sr.phase_vocoder(sr.stft(x[b, :n], N_FFT, N_FFT, HOP), rate, HOP, N_FFT)
        scale = sr.ola_scale(sr.spec_l1(out, N_FFT), N_FFT, N_FFT, HOP, length=want_len, weights=np.arange(1, len(out) + 1))
        worst = max(worst, worst_ratio(np.abs(y[b, :want_len] - want), U24 * scale))
    print("time stretch rate %.1f: worst ratio %.4f" % (rate, worst))
    assert worst <= C_S <= 512


def test_time_stretch_rows_are_independent_runs_repeat_and_speed_draws():
    device()
    from tensorflowasr_amd.augment import Speed, TimeStretch
    lens, x, y, out_len = stretch_case(0.9)
    ts = TimeStretch()
    rates = [0.9, 1.2, 0.5, 2.0, 1.0, 0.7]
    ym, lm = ts(x, lens, rates)
    ym, lm = ym.cpu().numpy(), lm.cpu().numpy()
    assert np.array_equal(bits(ts(x, lens, rates)[0].cpu().numpy()), bits(ym))
    assert list(lm) == [int(round(n / r)) for n, r in zip(lens, rates)]
    assert np.array_equal(bits(ym[0, :lm[0]]), bits(y[0, :lm[0]]))
    for b, n in enumerate(lens):
        y1, l1 = ts(x[b, :n], None, rates[b])
        assert int(l1[0]) == lm[b] and np.array_equal(bits(y1.cpu().numpy()[0, :lm[b]]), bits(ym[b, :lm[b]])), (b, n)
    # Speed: SignalSpeed's draw, then the stretch
    sp = Speed("(0.9,1.2)")
    np.random.seed(4)
    ys, ls = sp(x[:2], lens[:2])
    np.random.seed(4)
    drawn = [sp.draw()["rate"] for _ in range(2)]
    yw, lw = ts(x[:2], lens[:2], drawn)
    assert all(0.9 <= r <= 1.2 for r in drawn) and np.array_equal(ls.cpu().numpy(), lw.cpu().numpy())
    assert np.array_equal(bits(ys.cpu().numpy()), bits(yw.cpu().numpy()))
