"""The tests' own oracle of the band-limited resampler (csrc/sinc_resample.hip, resample.SincResampler) and of augment.Pitch:
J. O. Smith's band-limited interpolation as resampy 0.2 runs it for `kaiser_best`, restated from the published algorithm with NumPy
alone -- the package is not available to compare with, and the four filter constants are quoted from its documentation.  The
algorithm twice in float64 (a scalar loop that reads like the definition, a vectorised form for long rows that also returns the
error scale S1), once in float32 the way a kernel would run it, and pitch_ref on top of stft_ref.time_stretch."""
import math

import numpy as np

import stft_ref as sr

ZEROS, NT = 64, 512
ROLLOFF, BETA = 0.9475937167399596, 14.769656459379492
NW = NT * ZEROS + 1                                     # 32 769 table entries


def table():
    """the right half of the filter, float64"""
    n = NT * ZEROS
    return np.kaiser(2 * n + 1, BETA)[n:] * ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, ZEROS, n + 1))


WIN = table()


def out_length(n, r):
    return int(math.ceil(float(n) * float(r)))


def valid_length(n, r):
    return int(math.floor(float(n) * float(r)))


def resample_scalar(x, r, out_len=None):
    """the definition, one output and one tap at a time"""
    x = np.asarray(x, np.float64)
    N = len(x)
    out_len = out_length(N, r) if out_len is None else int(out_len)
    y = np.zeros(out_len, np.float64)
    scale = min(1.0, r)
    step = int(scale * NT)
    win = WIN * r if r < 1 else WIN
    delta = np.zeros(NW, np.float64)
    delta[:-1] = win[1:] - win[:-1]
    for t in range(min(out_len, valid_length(N, r))):
        pos = t * (1.0 / r)
        n = int(pos)
        frac = scale * (pos - n)
        o = int(frac * NT)
        eta = frac * NT - o
        for i in range(min(n + 1, (NW - o) // step)):
            y[t] += (win[o + i * step] + eta * delta[o + i * step]) * x[n - i]
        frac = scale - frac
        o = int(frac * NT)
        eta = frac * NT - o
        for k in range(min(N - n - 1, (NW - o) // step)):
            y[t] += (win[o + k * step] + eta * delta[o + k * step]) * x[n + k + 1]
    return y


def _wings(N, r, out_len):
    """per output t < valid: (n, [(o, eta, count, first sample, direction)] of the two wings), vectorised over t"""
    scale = min(1.0, r)
    step = int(scale * NT)
    T = min(out_len, valid_length(N, r))
    pos = np.arange(T, dtype=np.float64) * (1.0 / r)
    n = pos.astype(np.int64)
    frac = scale * (pos - n)
    out = []
    for f, limit, first, sign in ((frac, n + 1, n, -1), (scale - frac, N - n - 1, n + 1, 1)):
        idx = f * NT
        o = idx.astype(np.int64)
        out.append((o, idx - o, np.minimum(limit, (NW - o) // step), first, sign))
    return T, step, out


def resample(x, r, out_len=None, weights=False):
    """-> (y float64 [out_len], S1 [out_len] = sum_k |w_k x_k|); weights=True: also a list of (block of outputs, w [block, K],
    sample index [block, K]), one per block and wing (w is 0 past a wing's end), for pushing another signal's bound through the
    same weights: sum_k |w_k| a[n_k] is the sum over the list of (|w| a[index]).sum(1)"""
    x = np.asarray(x, np.float64)
    N = len(x)
    out_len = out_length(N, r) if out_len is None else int(out_len)
    y, s1 = np.zeros(out_len, np.float64), np.zeros(out_len, np.float64)
    T, step, wings = _wings(N, r, out_len)
    win = WIN * r if r < 1 else WIN
    delta = np.zeros(NW, np.float64)
    delta[:-1] = win[1:] - win[:-1]
    kept = []
    k = np.arange(NW // step + 1)[None, :]
    for t0 in range(0, T, 8192):                        # blocks of outputs: [block, K] temporaries
        blk = slice(t0, min(t0 + 8192, T))
        for o, eta, cnt, first, sign in wings:
            m = k < cnt[blk, None]
            j = np.where(m, o[blk, None] + k * step, 0)
            w = np.where(m, win[j] + eta[blk, None] * delta[j], 0.0)
            si = np.where(m, first[blk, None] + sign * k, 0)
            p = w * x[si]
            acc = y[blk]
            for c in range(int(cnt[blk].max())):        # tap after tap, as the scalar loop adds them (a masked tap adds 0)
                acc = acc + p[:, c]
            y[blk] = acc
            s1[blk] += np.abs(p).sum(axis=1)
            if weights:
                kept.append((blk, w, si))
    return (y, s1, kept) if weights else (y, s1)


def resample_f32(x, r, out_len=None):
    """what a kernel computes: the fp32 table, fp32 neighbour differences, position, n, o and eta in float64 (eta rounded to fp32
    once), fp32 FMAs into one accumulator, the left wing first, tap after tap; times fp32(r) at the end when r < 1.  (The FMAs are
    evaluated in float64 and rounded once, which is an FMA for fp32 operands: the products are exact in float64.)"""
    x = np.asarray(x, np.float32)
    N = len(x)
    out_len = out_length(N, r) if out_len is None else int(out_len)
    y = np.zeros(out_len, np.float32)
    T, step, wings = _wings(N, r, out_len)
    win = WIN.astype(np.float32)
    delta = np.zeros(NW, np.float32)
    delta[:-1] = win[1:] - win[:-1]
    if T:
        acc = np.zeros(T, np.float32)
        for o, eta, cnt, first, sign in wings:
            eta = eta.astype(np.float32).astype(np.float64)
            for k in range(int(cnt.max()) if len(cnt) else 0):
                m = k < cnt
                j = np.where(m, o + k * step, 0)
                w = (win[j].astype(np.float64) + eta * delta[j].astype(np.float64)).astype(np.float32)
                xv = x[np.where(m, first + sign * k, 0)].astype(np.float64)
                acc = np.where(m, (w.astype(np.float64) * xv + acc.astype(np.float64)).astype(np.float32), acc)
        if r < 1:
            acc = acc * np.float32(r)
        y[:T] = acc
    return y


MIN_ZONE = 1025


def zone(n, z):
    return int(n * z[0]), int(n * z[1])


def rate_of(steps):
    return 2.0 ** (-float(steps) / 12)


def pitch_ref(x, steps, z):
    """SignalPitch.augment with its draw given, librosa.effects.pitch_shift restated: the zone through stft_ref.time_stretch at
    rate = 2^(-steps / 12), resampled at the ratio `rate` to ceil(len rate) samples, cut or zero-filled to the zone.  A zone of
    fewer than 1025 samples is left as it is (librosa raises there); rate == 1.0 skips the resampler.
    -> (y float64, the stretched zone ys or None)"""
    y = np.asarray(x, np.float64).copy()
    s, e = zone(len(y), z)
    if e - s < MIN_ZONE:
        return y, None
    rate = rate_of(steps)
    ys = sr.time_stretch(y[s:e], rate)
    if rate == 1.0:
        y[s:e] = ys[:e - s]
        return y, ys
    out = np.zeros(e - s, np.float64)
    full = resample(ys, rate)[0]
    m = min(len(full), e - s)
    out[:m] = full[:m]
    y[s:e] = out
    return y, ys
