"""The batch the GPU tests of the recursive filters and of Hz share, with its references computed once (iir_ref.py): rows around
every chunk edge of the extended signal, per-row band-stops at the five starts, NaN past every row's length; and long_batch():
the same past the first tile of the passes and past the first stage of the scan."""
import functools

import numpy as np
from scipy import signal

import iir_ref as ir

U24 = 2.0 ** -24
PADLEN = 21
STARTS = (0.01, 0.2, 0.35, 0.69, 0.699)


def device():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def chunk():
    from tensorflowasr_amd.iir import SOSFilter
    return SOSFilter.CHUNK


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def lengths():
    """22 and 23 (just above padlen), 64, the extended row at C - 1, C, C + 1 and 2 C, three chunks and a bit, and 6000"""
    C = chunk()
    return [22, 23, 64, C - 43, C - 42, C - 41, 2 * C - 42, 3 * C + 5, 6000]


def sections(start):
    return signal.butter(3, [start, start + 0.3], "bandstop", output="sos")


def poisoned(rows, width, dtype):
    out = np.full((len(rows), width), np.nan, dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """x [9, 6007] float32 (NaN past lens), lens, starts (row b: STARTS[b % 5], so 6000 samples meet 0.69 and, in `shared`,
    0.699), u [9, 6007] float64 uniforms (NaN past lens)"""
    rng = np.random.default_rng(11)
    lens = lengths()
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    us = [rng.random(n) for n in lens]
    starts = [STARTS[b % len(STARTS)] for b in range(len(lens))]
    return {"x": poisoned(rows, max(lens) + 7, np.float32), "lens": lens, "rows": [r.astype(np.float64) for r in rows], "starts": starts,
            "sos": np.stack([sections(s) for s in starts]), "u": poisoned(us, max(lens) + 7, np.float64), "us": us}


@functools.lru_cache(maxsize=None)
def filtfilt_refs(shared_start=None):
    """per row: (y_ld, D) of sosfiltfilt with the row's sections (or those of shared_start)"""
    c = batch()
    out = []
    for b, x in enumerate(c["rows"]):
        sos = sections(shared_start) if shared_start is not None else c["sos"][b]
        y_ld = ir.sosfiltfilt_ld(sos, x, PADLEN)
        out.append((y_ld, ir.distance(signal.sosfiltfilt(sos, x, padlen=PADLEN), y_ld, x)))
    return out


@functools.lru_cache(maxsize=None)
def tf_refs():
    """per row: (hz_ref without noise = scipy's filtfilt(b, a, x), D_ba = max |filtfilt - filtfilt_ld|)"""
    c = batch()
    out = []
    for b, x in enumerate(c["rows"]):
        ba = signal.butter(3, [c["starts"][b], c["starts"][b] + .3], "bandstop")
        y = signal.filtfilt(*ba, x)
        out.append((y, ir.distance(y, ir.filtfilt_ld(*ba, x), x)))
    return out


W = 64 * 128                                    # kLanes * kChunk of iir.hip: the positions of one workgroup of sos_pass_kernel
SC = 1024 * 128                                 # kScan * kChunk of iir.hip: the positions of one stage of sos_scan_kernel
LONG_STARTS = (0.01, 0.699, 0.35)               # SciPy's hardest, worst and easiest band-stop here


def long_lengths(which):
    """samples per row.  "tiles": extended rows (N = L + 2 PADLEN) of W - 1, W, W + 1, 2 W and 2 W + 1 positions, and between
    them rows of 22 and 3 C + 5 samples, which end in tile 0 and are filled in tiles 1 and 2.  "scan": extended rows of SC, SC + 1
    and 2 SC + 5 positions (1024, 1025 and 2049 chunks: one, two and three stages of the scan), and one row of 6000."""
    C, P = chunk(), 2 * PADLEN
    assert W == 64 * C and SC == 1024 * C
    if which == "tiles":
        return [W - 1 - P, 22, W - P, 3 * C + 5, W + 1 - P, 22, 2 * W - P, 3 * C + 5, 2 * W + 1 - P]
    assert which == "scan", which
    return [SC - P, SC + 1 - P, 2 * SC + 5 - P, 6000]


def long_rows(which):
    """the rows of a long batch that leave tile 0"""
    return [b for b, n in enumerate(long_lengths(which)) if n + 2 * PADLEN >= W - 1]


@functools.lru_cache(maxsize=None)
def long_batch(which):
    """batch() past the first tile ("tiles") and past the first scan stage ("scan"): x float32 (NaN past lens), lens, starts (the
    long rows cycle through LONG_STARTS in their order, and so do the short ones), u float64 uniforms (NaN past lens)"""
    rng = np.random.default_rng({"tiles": 17, "scan": 19}[which])
    lens = long_lengths(which)
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    us = [rng.random(n) for n in lens]
    starts, seen = [], [0, 0]
    for n in lens:
        k = int(n + 2 * PADLEN >= W - 1)
        starts.append(LONG_STARTS[seen[k] % 3])
        seen[k] += 1
    return {"x": poisoned(rows, max(lens) + 7, np.float32), "lens": lens, "rows": [r.astype(np.float64) for r in rows], "starts": starts,
            "sos": np.stack([sections(s) for s in starts]), "u": poisoned(us, max(lens) + 7, np.float64), "us": us}


@functools.lru_cache(maxsize=None)
def long_refs(which, shared_start=None):
    """filtfilt_refs() of long_batch(which)"""
    c = long_batch(which)
    out = []
    for b, x in enumerate(c["rows"]):
        sos = sections(shared_start) if shared_start is not None else c["sos"][b]
        y_ld = ir.sosfiltfilt_ld(sos, x, PADLEN)
        out.append((y_ld, ir.distance(signal.sosfiltfilt(sos, x, padlen=PADLEN), y_ld, x)))
    return out


FLIPS = [0, 0]                                 # samples checked / samples whose float32 is not the rounded long-double value


def check_bound(y, y_ld, D, extra=0.0):
    """|y - y_ld| <= 2^-24 |y_ld| + 8 (D + extra) per sample; returns the worst (|y - y_ld| - 2^-24 |y_ld|) / (D + extra), 0 when
    the rounding to float32 covers the error everywhere.  FLIPS counts how often the float64 error moved that rounding."""
    err = np.abs(np.asarray(y, ir.LD) - y_ld)
    over = np.asarray(err - U24 * np.abs(y_ld), np.float64)
    assert over.max() <= 8.0 * (D + extra), (float(over.max()) / (D + extra), D, extra, int(np.argmax(over)))
    FLIPS[0] += len(y_ld)
    FLIPS[1] += int((np.asarray(y, np.float32) != np.asarray(y_ld, np.float64).astype(np.float32)).sum())
    return max(float(over.max()) / (D + extra), 0.0)


def check_quantised(y, want, limit=0.001):
    """every differing sample differs by exactly one step 2^-15, and at most `limit` of the row's samples differ"""
    y, want = np.asarray(y, np.float64), np.asarray(want, np.float64)
    diff = y != want
    assert np.array_equal(np.abs(y[diff] - want[diff]), np.full(int(diff.sum()), 2.0 ** -15)), np.abs(y[diff] - want[diff]).max()
    assert diff.sum() <= limit * len(want), (int(diff.sum()), len(want))
    return int(diff.sum())
