"""Yardsticks of the recursive filters and of the hz / masking augmentations (NumPy and SciPy only; nothing here touches the
package under test):

    sosfilt_ld, sosfiltfilt_ld   scipy.signal.sosfilt / sosfiltfilt (padtype="odd") evaluated in np.longdouble
    filtfilt_ld                  scipy.signal.filtfilt(b, a, x) -- the reference's transfer-function call -- in np.longdouble
    hz_ref, mask_ref             the reference's SignalHz and SignalMask with the draws handed in
    quantise                     Augmentation.process's clip and truncation to 16 bits
    sosfiltfilt_chunked          a float64 restatement of the device algorithm: one biquad at a time, chunks joined through
                                 2 x 2 transitions obtained by running the recursion (tensorflowasr_amd/csrc/iir.hip)
    filtfilt_chunked_tf          the same idea on the 6th-order transfer-function recursion: kept to show that it FAILS
"""
import numpy as np
from scipy import signal

LD = np.longdouble


def _biquad_ld(c, x, z):
    """one section in direct form II transposed, long double; c = (b0, b1, b2, a0, a1, a2); returns (y, final state)"""
    b0, b1, b2, a0, a1, a2 = [LD(v) for v in c]
    b0, b1, b2, a1, a2 = b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0
    z1, z2 = LD(z[0]), LD(z[1])
    y = np.empty(len(x), LD)
    for n in range(len(x)):
        v = x[n]
        o = b0 * v + z1
        z1 = b1 * v - a1 * o + z2
        z2 = b2 * v - a2 * o
        y[n] = o
    return y, np.array([z1, z2], LD)


def sosfilt_ld(sos, x, zi=None):
    """-> (y, zf [S, 2]) in long double"""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    y = np.asarray(x, LD)
    zf = np.zeros((len(sos), 2), LD)
    for s, c in enumerate(sos):
        y, zf[s] = _biquad_ld(c, y, (0, 0) if zi is None else zi[s])
    return y, zf


def sosfilt_zi_ld(sos):
    """scipy.signal.sosfilt_zi in long double"""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    zi = np.zeros((len(sos), 2), LD)
    scale = LD(1)
    for s, c in enumerate(sos):
        zi[s] = scale * lfilter_zi_ld(c[:3], c[3:])
        scale = scale * (LD(c[0]) + LD(c[1]) + LD(c[2])) / (LD(c[3]) + LD(c[4]) + LD(c[5]))
    return zi


def lfilter_zi_ld(b, a):
    """scipy.signal.lfilter_zi in long double: the state of a step response at rest, by its closed form"""
    b, a = np.asarray(b, LD), np.asarray(a, LD)
    b, a = b / a[0], a / a[0]
    n = max(len(a), len(b))
    a = np.concatenate((a, np.zeros(n - len(a), LD)))
    b = np.concatenate((b, np.zeros(n - len(b), LD)))
    B = b[1:] - a[1:] * b[0]
    zi = np.zeros(n - 1, LD)
    zi[0] = B.sum() / a.sum()                       # the first column of I - companion(a).T sums to sum(a)
    asum, csum = LD(1), LD(0)
    for k in range(1, n - 1):
        asum = asum + a[k]
        csum = csum + b[k] - a[k] * b[0]
        zi[k] = asum * zi[0] - csum
    return zi


def odd_ext(x, n):
    x = np.asarray(x)
    if n < 1:
        return x.copy()
    return np.concatenate((2 * x[0] - x[n:0:-1], x, 2 * x[-1] - x[-2:-n - 2:-1]))


def sosfiltfilt_ld(sos, x, padlen):
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    x = np.asarray(x, LD)
    if len(x) <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    ext = odd_ext(x, padlen)
    zi = sosfilt_zi_ld(sos)
    y, _ = sosfilt_ld(sos, ext, zi * ext[0])
    y, _ = sosfilt_ld(sos, y[::-1], zi * y[-1])
    y = y[::-1]
    return y[padlen:len(y) - padlen] if padlen else y


def _lfilter_ld(b, a, x, z):
    b, a = np.asarray(b, LD), np.asarray(a, LD)
    b, a = b / a[0], a / a[0]
    m = len(a) - 1
    z = np.array(z, LD)
    y = np.empty(len(x), LD)
    for n in range(len(x)):
        v = x[n]
        o = b[0] * v + z[0]
        for k in range(m - 1):
            z[k] = b[k + 1] * v - a[k + 1] * o + z[k + 1]
        z[m - 1] = b[m] * v - a[m] * o
        y[n] = o
    return y, z


def filtfilt_ld(b, a, x):
    """scipy.signal.filtfilt(b, a, x) (padtype="odd", padlen = 3 max(len(a), len(b))) in long double"""
    padlen = 3 * max(len(a), len(b))
    x = np.asarray(x, LD)
    ext = odd_ext(x, padlen)
    zi = lfilter_zi_ld(b, a)
    y, _ = _lfilter_ld(b, a, ext, zi * ext[0])
    y, _ = _lfilter_ld(b, a, y[::-1], zi * y[-1])
    return y[::-1][padlen:-padlen]


def quantise(v):
    """Augmentation.process's last line (the conversion truncates toward zero and knows no negative zero)"""
    return np.array(np.clip(np.asarray(v, np.float64), -1.0, 1.0) * 32768, "int32") / 32768.0


def hz_ref(x, start, u):
    """SignalHz.augment with its two draws handed in: the start and the uniforms"""
    return signal.filtfilt(*signal.butter(3, [start, start + .3], "bandstop"), np.asarray(x, np.float64)) + np.asarray(u, np.float64) * 0.001


def mask_span(n, zone):
    return int(n * zone[0]), int(n * zone[1])


def mask_ref(x, zone, mask_ratio, mask_with_noise, u):
    """SignalMask.augment on float64 data, `u` in place of its np.random.random(e - s)"""
    data = np.array(x, np.float64)
    s, e = mask_span(len(data), zone)
    data_ = data[s:e]
    mask_value = np.asarray(u, np.float64)[:len(data_)]
    mask = np.where(mask_value < mask_ratio, 0.0, 1.0)
    if mask_with_noise:
        value = mask_value * np.where(mask == 0.0, 1.0, 0.0)
        data_ = data_ * mask
        data_ = data_ + value
    else:
        data_ = data_ * mask
    data[s:e] = data_
    return data


# ---- the device algorithm restated in float64 ------------------------------------------------------------------------------------------
def _transition(run, m, steps):
    """the m x m transition of `steps` zero-input samples, by running the recursion on the unit states"""
    M = np.zeros((m, m))
    for j in range(m):
        e = np.zeros(m)
        e[j] = 1.0
        M[:, j] = run(np.zeros(steps), e)[1]
    return M


def chunked_run(run, m, x, zi, C):
    """y of one recursion over x from the state zi, cut into chunks of C: zero-state runs, a sequential walk over their final
    states with the chunk transition, then every chunk again from its true state.  run(seg, z) -> (y, zf)."""
    n = len(x)
    nc = (n + C - 1) // C
    M = _transition(run, m, C)
    p = [run(x[c * C:(c + 1) * C], np.zeros(m))[1] for c in range(nc)]
    s = np.array(zi, np.float64)
    y = np.empty(n)
    for c in range(nc):
        y[c * C:(c + 1) * C] = run(x[c * C:(c + 1) * C], s)[0]
        s = M @ s + p[c]                                # (the short last chunk's exit state is not used)
    return y


def sosfiltfilt_chunked(sos, x, padlen, C):
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    ext = odd_ext(np.asarray(x, np.float64), padlen)
    zi = signal.sosfilt_zi(sos)

    def one_pass(v):
        first = v[0]
        for s in range(len(sos)):
            run = lambda seg, z, s=s: tuple(np.squeeze(r) for r in signal.sosfilt(sos[s:s + 1], seg, zi=np.reshape(z, (1, 2))))
            v = chunked_run(run, 2, v, zi[s] * first, C)
        return v
    y = one_pass(ext)
    y = one_pass(y[::-1].copy())[::-1]
    return y[padlen:len(y) - padlen] if padlen else y


def filtfilt_chunked_tf(b, a, x, C):
    padlen = 3 * max(len(a), len(b))
    ext = odd_ext(np.asarray(x, np.float64), padlen)
    zi = signal.lfilter_zi(b, a)
    run = lambda seg, z: signal.lfilter(b, a, seg, zi=z)
    y = chunked_run(run, len(a) - 1, ext, zi * ext[0], C)
    y = chunked_run(run, len(a) - 1, y[::-1].copy(), zi * y[-1], C)[::-1]
    return y[padlen:-padlen]


def distance(y, y_ld, x):
    """D of a row: max |y - y_ld|, at least 2^-50 max |x|"""
    return max(float(np.abs(np.asarray(y, LD) - y_ld).max()), 2.0 ** -50 * float(np.abs(x).max()))
