"""Float64 NumPy restatements of the far-field definitions (include/mi355asr.h): the image-source room
impulse response, the ragged full convolution, SNR mixing and the clip / 16-bit quantisation.  Test infrastructure: the device
kernels of csrc/augment.hip are compared with these, and the bounds of the comparisons are computed here, never from the device."""
import numpy as np


def reflection_coefficients(room, c, reverberation_time):
    """all six beta = sqrt(1 - alpha), alpha = 24 V ln 10 / (c S T); ValueError when alpha > 1"""
    Lx, Ly, Lz = (float(v) for v in room)
    V = Lx * Ly * Lz
    S = 2.0 * (Lx * Lz + Ly * Lz + Lx * Ly)
    alpha = 24.0 * V * np.log(10.0) / (c * S * reverberation_time)
    if alpha > 1.0:
        raise ValueError("alpha = %g > 1" % alpha)
    return [float(np.sqrt(1.0 - alpha))] * 6


def window_taps(fs):
    return 2 * int(np.floor(0.004 * fs + 0.5))


def highpass(h, fs):
    """the generator's 100 Hz high-pass recurrence over h (float64)"""
    W = 2.0 * np.pi * 100.0 / fs
    R1 = np.exp(-W)
    B1, B2, A1 = 2.0 * R1 * np.cos(W), -R1 * R1, -(1.0 + R1)
    out = np.empty(len(h), np.float64)
    y0 = y1 = y2 = 0.0
    for i, v in enumerate(np.asarray(h, np.float64)):
        y2, y1 = y1, y0
        y0 = B1 * y1 + B2 * y2 + v
        out[i] = y0 + A1 * y1 + R1 * y2
    return out


def highpass_abs_gain(nsample, fs):
    """sum of the absolute impulse response of the recurrence over nsample samples: the factor by which an input error can grow"""
    imp = np.zeros(nsample)
    imp[0] = 1.0
    return float(np.abs(highpass(imp, fs)).sum())


def rir(room, source, receiver, c, fs, nsample, reverberation_time=None, beta=None, hp_filter=False):
    """-> (h float64 [nsample], A float64 [nsample]): the response, and A[n] = sum of |gain| over the images whose window covers n
    (before the high-pass filter)"""
    room, source, receiver = (np.asarray(v, np.float64) for v in (room, source, receiver))
    if beta is None:
        beta = reflection_coefficients(room, c, reverberation_time)
    beta = [float(b) for b in beta]
    cTs = c / fs
    Ls, ss, rs = room / cTs, source / cTs, receiver / cTs
    Tw, Fc = window_taps(fs), 0.5
    nd = [int(np.ceil(nsample / (2.0 * Ls[d]))) for d in range(3)]
    m = [np.arange(-n, n + 1) for n in nd]
    mx, my, mz = m[0][:, None, None], m[1][None, :, None], m[2][None, None, :]
    h = np.zeros(nsample)
    A = np.zeros(nsample)
    nn = np.arange(Tw)
    for q in (0, 1):
        dx = (1 - 2 * q) * ss[0] - rs[0] + 2.0 * mx * Ls[0]
        for j in (0, 1):
            dy = (1 - 2 * j) * ss[1] - rs[1] + 2.0 * my * Ls[1]
            for k in (0, 1):
                dz = (1 - 2 * k) * ss[2] - rs[2] + 2.0 * mz * Ls[2]
                dist = np.sqrt(dx * dx + dy * dy + dz * dz)
                fdist = np.floor(dist)
                with np.errstate(divide="ignore", invalid="ignore"):
                    gain = (np.power(beta[0], np.abs(mx - q)) * np.power(beta[1], np.abs(mx))
                            * np.power(beta[2], np.abs(my - j)) * np.power(beta[3], np.abs(my))
                            * np.power(beta[4], np.abs(mz - k)) * np.power(beta[5], np.abs(mz))) / (4.0 * np.pi * dist * cTs)
                keep = fdist < nsample
                d, fd, g = dist[keep], fdist[keep].astype(np.int64), np.broadcast_to(gain, dist.shape)[keep]
                t = (nn - Tw // 2 + 1)[None, :] - (d - fd)[:, None]
                w = 0.5 * (1.0 + np.cos(2.0 * np.pi * t / Tw)) * Fc * np.sinc(Fc * t)      # np.sinc(x) = sin(pi x) / (pi x)
                idx = fd[:, None] - Tw // 2 + 1 + nn[None, :]
                ok = (idx >= 0) & (idx < nsample)
                h += np.bincount(idx[ok], weights=(g[:, None] * w)[ok], minlength=nsample)
                A += np.bincount(idx[ok], weights=np.broadcast_to(np.abs(g)[:, None], idx.shape)[ok], minlength=nsample)
    if hp_filter:
        h = highpass(h, fs)
    return h, A


def fir_full(x, h):
    """-> (y64, bound term sum_k |h[k]| |x[n - k]|) of the full convolution; an empty x gives empty outputs"""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    return np.convolve(x, h), np.convolve(np.abs(x), np.abs(h))


def mix_snr(x, d, snr_db):
    """-> (y64, g64): y = x + g d over len(x) samples, g = sqrt(P_x / 10^(snr_db / 10) / P_d), 0 when either power is 0"""
    x = np.asarray(x, np.float64)
    d = np.asarray(d, np.float64)[:len(x)]
    px, pd = float(np.sum(x * x)), float(np.sum(d * d))
    g = float(np.sqrt(px / 10.0 ** (float(snr_db) / 10.0) / pd)) if px > 0.0 and pd > 0.0 else 0.0
    return x + g * d, g


def quantise(y):
    """Augmentation.process's last step on a float32 array, in float32: np.array(np.clip(y, -1, 1) * 32768, "int32") / 32768"""
    y = np.asarray(y, np.float32)
    return (np.array(np.clip(y, np.float32(-1.0), np.float32(1.0)) * np.float32(32768.0), "int32") / np.float32(32768.0)).astype(np.float32)
