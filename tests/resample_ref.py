"""Float64 NumPy evaluation of the resampling formula the device kernels implement, from
`tensorflowasr_amd.resample.design_filter`; the tests compare it, and the kernels, with scipy.signal.resample_poly.  Below it: the
ratios beyond the shipped rates, and impulse trains with their exact criterion against resample_poly."""
import numpy as np
from scipy.signal import resample_poly

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


# ---- ratios the shipped rates do not reach, and impulse trains that make a sharp test possible at any K -------------------------
# 1/18 is the last ratio whose tile span is staged in LDS and 1/19 the first that is not; 3/61 and 101/640 are unstaged with several
# phases; 147/640 (48 kHz -> 11.025 kHz) and 639/640 are staged close to the budget; 640/1 and 1/640 are the limits
MORE_RATIOS = [(1, 18), (1, 19), (3, 61), (101, 640), (147, 640), (639, 640), (640, 1), (1, 640)]
SMALL_K = [(2, 1), (1, 2), (1, 3), (160, 441), (320, 441), (640, 441), (640, 1), (639, 640)]
LARGE_K = [(1, 18), (1, 19), (1, 20), (3, 61), (101, 640), (147, 640), (1, 640)]


def plan(up, down):
    """the library's plan restated (make_plan of csrc/resample.hip): taps, tile, whether a tile's span is staged, LDS bytes"""
    half = 10 * max(up, down)
    K = -(-(2 * half + 1) // up)
    floats = (up * (K | 1) + 3) & ~3
    unit = 4 * up
    tile = unit * -(-1024 // unit)
    span = ((up - 1) + (tile - 1) * down) // up + K
    staged_bytes = 4 * (floats + ((span + 8 + 8 + 3) & ~3) + tile)
    staged = staged_bytes <= 80 * 1024
    return dict(taps=K, stride=K | 1, table_floats=floats, tile=tile, staged=staged, lds=staged_bytes if staged else 4 * floats)


def filter_gap(up, down):
    """D: the largest absolute difference between design_filter and scipy's firwin(...) * up"""
    from scipy.signal import firwin
    h, half = design_filter(up, down)
    return float(np.abs(h - firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up).max())


def two_tile_length(up, down):
    """an input length that gives more than two output tiles and a ragged end"""
    return ((2 * plan(up, down)["tile"] + 5) * down) // up + 3


def batch_positions(up, down):
    """K + 1 rows of L samples; row b has impulses at b, b + s, b + 2 s, ... (s = K + 1): every position of [0, L) in one row"""
    s = plan(up, down)["taps"] + 1
    L = two_tile_length(up, down)
    return L, [np.arange(b, L, s, dtype=np.int64) for b in range(s)]


def row_positions(up, down):
    """one row: impulses at 0, s, 2 s, ... with s >= K + 1 prime to `down`, and down + 2 or more of them so that the residue classes
    of the first and of the last impulse (which lose their taps before the row's start and past its end) are visited again by an
    impulse in the interior; the last sample is an impulse and L is at least the two-tile length"""
    from math import gcd
    s = plan(up, down)["taps"] + 1
    while gcd(s, down) != 1:
        s += 1
    n = max(down + 2, -(-two_tile_length(up, down) // s) + 1)
    return (n - 1) * s + 1, np.arange(n, dtype=np.int64) * s


def impulse_values(rng, count, pcm=False):
    """+-2^e, e in [-3, 3]; as PCM +-2^e, e in [0, 14], and -32768 now and then (int16 / 32768 is exact)"""
    sign = rng.choice([-1.0, 1.0], count)
    if not pcm:
        return sign * 2.0 ** rng.integers(-3, 4, count)
    v = sign * 2.0 ** rng.integers(0, 15, count)
    v[rng.random(count) < 0.1] = -32768.0
    return v


def impulse_row(L, pos, values, dtype=np.float32):
    x = np.zeros(L, dtype)
    x[pos] = values
    assert np.array_equal(x[pos].astype(np.float64), values)             # exact in the input format
    return x


def impulse_hits(pos, L, up, down):
    """(k, tap) of every (impulse j, output k) pair whose tap index k down + half - j up lies inside the filter"""
    half = 10 * max(up, down)
    pos = np.asarray(pos, np.int64)
    k_lo = np.maximum(0, -(-(pos * up - half) // down))
    k_hi = np.minimum(out_length(L, up, down) - 1, (pos * up + half) // down)
    cnt = np.maximum(0, k_hi - k_lo + 1)
    j = np.repeat(pos, cnt)
    k = np.repeat(k_lo, cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return k, k * down + half - j * up


def impulses_in_window(pos, L, up, down):
    """per output k: how many impulses lie among the K samples x[jh - K + 1 .. jh] of its chain"""
    half, K = 10 * max(up, down), plan(up, down)["taps"]
    jh = (np.arange(out_length(L, up, down), dtype=np.int64) * down + half) // up
    pos = np.sort(np.asarray(pos, np.int64))
    return np.searchsorted(pos, jh, "right") - np.searchsorted(pos, jh - K + 1, "left")


def chain_float32(x, up, down):
    """the kernels' sum in plain float32 NumPy, same tap order m = 0 .. K-1, but the product rounded before it is added (no FMA):
    x [B, L] -> [B, out_length(L)] float32"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    h, half = design_filter(up, down)
    K = plan(up, down)["taps"]
    full = np.zeros(K * up, np.float64)
    full[:len(h)] = h
    hp = np.ascontiguousarray(full.reshape(K, up).T.astype(np.float32))
    L = x.shape[1]
    c = np.arange(out_length(L, up, down), dtype=np.int64) * down + half
    p, jh = c % up, c // up
    xpad = np.zeros((x.shape[0], K - 1 + max(L, int(jh.max()) + 1)), np.float32)
    xpad[:, K - 1:K - 1 + L] = x
    acc = np.zeros((x.shape[0], len(c)), np.float32)
    for m in range(K):
        acc = hp[p, m] * xpad[:, jh - m + K - 1] + acc
    assert acc.dtype == np.float32
    return acc


def check_impulse_rows(up, down, x, positions, y, what, with_e32=True):
    """x [B, L] exact in float64, positions[b] the impulses of row b, y [B, O] float32 what the device returned.  Per output:
    |y - ref| <= 2^-24 |ref| + 8 D (one tap rounded once to fp32; D the gap between design_filter and firwin; 8 the largest amplitude),
    and exactly 0 where, by the positions alone, the output's K samples hold no impulse.  -> the tap indices the rows visited."""
    L = x.shape[1]
    D = filter_gap(up, down)
    assert D <= 1e-12
    assert y.dtype == np.float32 and y.shape == (len(positions), out_length(L, up, down))
    exact = total = 0
    err = e32 = 0.0
    taps = []
    for b, pos in enumerate(positions):
        ref = resample_poly(x[b].astype(np.float64), up, down)
        inside = impulses_in_window(pos, L, up, down)
        assert inside.max(initial=0) <= 1, "the train is too dense for an exact test"
        assert not y[b, inside == 0].any(), (what, b, np.flatnonzero((inside == 0) & (y[b] != 0))[:8])
        d = np.abs(y[b].astype(np.float64) - ref)
        bad = np.flatnonzero(d > 2.0 ** -24 * np.abs(ref) + 8 * D)
        assert not len(bad), (what, b, len(bad), bad[:8], y[b, bad[:8]], ref[bad[:8]])
        exact += int((y[b] == ref.astype(np.float32)).sum())
        total += len(ref)
        err = max(err, float(d.max()))
        if with_e32:
            e32 = max(e32, float(np.abs(chain_float32(x[b], up, down)[0].astype(np.float64) - ref).max()))
        taps.append(impulse_hits(pos, L, up, down)[1])
    p = plan(up, down)
    print("impulses %s %d/%d: K=%d tile=%d %s lds=%d: %d of %d outputs equal float32(ref) exactly; D=%.2g; err/E32=%s"
          % (what, up, down, p["taps"], p["tile"], "staged" if p["staged"] else "unstaged", p["lds"], exact, total, D,
             "%.3f" % (err / e32) if e32 else "n/a"))
    return np.unique(np.concatenate(taps))


def all_taps(up, down):
    return np.arange(20 * max(up, down) + 1)
