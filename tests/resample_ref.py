"""Float64 NumPy evaluation of the resampling formula the device kernels implement, from
`tensorflowasr_amd.resample.design_filter`; the tests compare it, and the kernels, with scipy.signal.resample_poly."""
import numpy as np

from tensorflowasr_amd.resample import design_filter, out_length

RATIOS = [(2, 1), (1, 2), (1, 3), (160, 441), (320, 441), (640, 441)]


def resample_formula(x, up, down):
    """y[k] = sum_j h[c - j up] x[j], c = k down + half, over 0 <= c - j up < n and 0 <= j < L, in float64"""
    x = np.asarray(x, np.float64)
    h, half = design_filter(up, down)
    n, L = len(h), len(x)
    y = np.zeros(out_length(L, up, down), np.float64)
    for k in range(len(y)):
        c = k * down + half
        j_hi = min(c // up, L - 1)
        j_lo = max(0, -(-(c - n + 1) // up))
        if j_hi >= j_lo:
            j = np.arange(j_lo, j_hi + 1)
            y[k] = np.dot(h[c - j * up], x[j])
    return y


def taps_and_gain(up, down):
    """K = ceil(n / up) taps per output, A = the largest per-phase absolute tap sum of the filter"""
    h, _ = design_filter(up, down)
    K = -(-len(h) // up)
    return K, max(float(np.abs(h[p::up]).sum()) for p in range(up))
