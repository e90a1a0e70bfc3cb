"""float64 NumPy restatement of librosa 0.9's stft / istft / phase_vocoder / effects.time_stretch and of the reference's
SignalSpecAug (augmentations/augments.py), without librosa: the oracle of the device STFT pair (csrc/stft.hip), and the error
scales its tests measure against.  Spectra are frame-major, [frames, n_fft / 2 + 1] (librosa's layout transposed), as the
device stores them."""
import numpy as np

SIZES = ((1024, 800, 160), (2048, 2048, 512))
TINY = float(np.finfo(np.float32).tiny)


def window(n_fft, win_length):
    """periodic Hann of win_length, zero-padded on both sides to n_fft (scipy get_window(fftbins=True) + librosa pad_center)"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    lpad = (n_fft - win_length) // 2
    return np.pad(w, (lpad, n_fft - win_length - lpad))


def n_frames(n, n_fft, hop):
    """1 + n // hop; 0 for a row too short to reflect-pad (librosa raises there)"""
    return 1 + n // hop if n >= n_fft // 2 + 1 else 0


def frames_of(x, n_fft, win_length, hop):
    """the windowed frames [F, n_fft] of x (float64)"""
    x = np.asarray(x, np.float64)
    F = n_frames(len(x), n_fft, hop)
    if F == 0:
        return np.zeros((0, n_fft))
    xp = np.pad(x, n_fft // 2, mode="reflect")
    idx = hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]
    return xp[idx] * window(n_fft, win_length)[None, :]


def stft(x, n_fft, win_length, hop):
    """-> complex128 [F, n_fft / 2 + 1]"""
    return np.fft.rfft(frames_of(x, n_fft, win_length, hop), axis=1)


def wss(F, n_fft, win_length, hop):
    """librosa.filters.window_sumsquare over F frames: [n_fft + hop (F - 1)]"""
    w2 = window(n_fft, win_length) ** 2
    out = np.zeros(n_fft + hop * max(F - 1, 0))
    for f in range(F):
        out[f * hop:f * hop + n_fft] += w2
    return out


def _ola(frames, n_fft, win_length, hop, length):
    """windowed frames [F, n_fft] -> overlap-added, normalised, centred, `length` samples"""
    F = len(frames)
    if F == 0:
        return np.zeros(0 if length is None else length)
    y = np.zeros(n_fft + hop * (F - 1))
    for f in range(F):
        y[f * hop:f * hop + n_fft] += frames[f]
    s = wss(F, n_fft, win_length, hop)
    nz = s > TINY
    y[nz] /= s[nz]
    y = y[n_fft // 2:]
    n = hop * (F - 1) if length is None else length
    out = np.zeros(n)
    m = min(n, len(y))
    out[:m] = y[:m]
    return out


def istft(S, n_fft, win_length, hop, length=None):
    """S [F, bins] -> hop (F - 1) samples, or `length` (librosa.istft(..., length=): cut, or zero-filled beyond the frames)"""
    S = np.asarray(S, np.complex128)
    return _ola(np.fft.irfft(S, n=n_fft, axis=1) * window(n_fft, win_length)[None, :], n_fft, win_length, hop, length)


def mask(S, centres, win):
    """SignalSpecAug's blocks on a frame-major spectrum: centre (h_, w_) zeroes bins [max(h_ - win, 0), h_ + win) of frames
    [max(w_ - win, 0), w_ + win)"""
    S = np.array(S)
    for h_, w_ in np.asarray(centres, np.int64).reshape(-1, 2):
        S[max(w_ - win, 0):max(w_ + win, 0), max(h_ - win, 0):max(h_ + win, 0)] = 0
    return S


def spec_aug(x, centres, win):
    """SignalSpecAug.augment with its draws given; a row with fewer than 513 samples comes back unchanged"""
    x = np.asarray(x, np.float64)
    if len(x) < 513:
        return x.copy()
    return istft(mask(stft(x, 1024, 800, 160), centres, win), 1024, 800, 160)


def phase_vocoder(D, rate, hop, n_fft):
    """librosa.phase_vocoder on a frame-major D [F, bins] -> [ceil(F / rate), bins]"""
    D = np.asarray(D, np.complex128)
    F, bins = D.shape
    steps = np.arange(0, F, rate, dtype=np.float64)
    out = np.zeros((len(steps), bins), np.complex128)
    phi = np.linspace(0, np.pi * hop, bins)
    acc = np.angle(D[0]) if F else np.zeros(bins)
    Dp = np.concatenate([D, np.zeros((2, bins), np.complex128)])
    for t, step in enumerate(steps):
        c0, c1 = Dp[int(step)], Dp[int(step) + 1]
        alpha = np.mod(step, 1.0)
        out[t] = ((1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)) * np.exp(1j * acc)
        dphase = np.angle(c1) - np.angle(c0) - phi
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        acc = acc + phi + dphase
    return out


def stretch_frames(F, rate):
    return len(np.arange(0, F, rate, dtype=np.float64))


def stretch_len(n, rate):
    return int(round(n / rate))


def time_stretch(x, rate, n_fft=2048, hop=512):
    """librosa.effects.time_stretch -> int(round(len / rate)) samples"""
    x = np.asarray(x, np.float64)
    S = phase_vocoder(stft(x, n_fft, n_fft, hop), rate, hop, n_fft)
    return istft(S, n_fft, n_fft, hop, length=stretch_len(len(x), rate))


# ---- error scales ------------------------------------------------------------------------------------------------------------------
def frame_l1(x, n_fft, win_length, hop):
    """a_f = sum_m |x_f[m] w[m]|: bounds every bin of frame f and every sample of its inverse"""
    return np.abs(frames_of(x, n_fft, win_length, hop)).sum(axis=1)


def ola_scale(a, n_fft, win_length, hop, length=None, weights=None):
    """A[n] = sum_f w[n - f hop] weights[f] a[f] / wss[n], laid out as istft lays its output out"""
    a = np.asarray(a, np.float64)
    if weights is not None:
        a = a * weights
    return _ola(a[:, None] * window(n_fft, win_length)[None, :], n_fft, win_length, hop, length)


def spec_l1(S, n_fft):
    """a_t = (2 / n_fft) sum_k |S[t, k]|: bounds every sample of the inverse of frame t"""
    return (2.0 / n_fft) * np.abs(S).sum(axis=1)
