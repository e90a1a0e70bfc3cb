"""Lengths for tests/test_gpu_ragged_edges.py: sample counts that put an utterance's encoder length T exactly where a test wants it,
with every parity of the two sub-sampling convs' SAME padding and every hop residue of the STFT's.

An utterance of L samples has F = ceil(L / 160) mel frames, T1 = ceil(F / 2) conv1 rows and T = ceil(T1 / 2) encoder frames
(models.ragged_geometry).  A combo is (f_odd, t1_odd, r): F odd or even (conv1 pads one row on top or none), T1 odd or even
(the same for conv2), and r = L - 160 (F - 1) in {1, 159, 160}, i.e. L mod hop in {1, 159, 0} (the last STFT frame holds one
sample, all but one, or is full)."""
import itertools

import numpy as np

HOP = 160
COMBOS = list(itertools.product((False, True), (False, True), (1, 159, 160)))          # combo k = COMBOS[k], k = 0 .. 11


def L_for(T, f_odd, t1_odd, r):
    """the sample count whose geometry is exactly (T, T1 = 2T - t1_odd, F = 2 T1 - f_odd) and whose last frame holds r samples"""
    assert T >= 1 and r in (1, HOP - 1, HOP)
    T1 = 2 * T - 1 if t1_odd else 2 * T
    F = 2 * T1 - 1 if f_odd else 2 * T1
    return HOP * (F - 1) + r


def geometry_for(T, f_odd, t1_odd, r):
    T1 = 2 * T - 1 if t1_odd else 2 * T
    return dict(T=T, T1=T1, F=2 * T1 - 1 if f_odd else 2 * T1)


def edge(Tmax, tile=16):
    """{1, 2, 3} + every multiple of the tile and its two neighbours up to Tmax + {Tmax - 1, Tmax}, ascending"""
    s = {1, 2, 3, Tmax - 1, Tmax}
    for k in range(1, Tmax // tile + 2):
        s |= {tile * k - 1, tile * k, tile * k + 1}
    return sorted(t for t in s if 1 <= t <= Tmax)


def with_fill(members, B, Tmax, seed):
    """members, then seeded draws (without repetition) from the lengths 1 .. Tmax that are not in edge(Tmax), up to B entries; the
    draws are a prefix of one seeded permutation, so a larger batch of the same seed extends a smaller one"""
    members = list(members)
    rest = sorted(set(range(1, Tmax + 1)) - set(edge(Tmax)))
    fill = np.random.default_rng(seed).permutation(rest)[:max(B - len(members), 0)]
    return members + [int(t) for t in fill]


def with_combos(Ts):
    """[(T_i, combo (5 i) mod 12)]: 5 and 12 are coprime, so any 12 consecutive utterances hold every combo"""
    return [(int(T), (5 * i) % 12) for i, T in enumerate(Ts)]


def utterance(T, combo):
    """(T, combo) -> 0.1 N(0, 1) noise of L_for(T, combo) samples, seeded by L: the same utterance in every batch"""
    L = L_for(T, *COMBOS[combo])
    return (0.1 * np.random.default_rng(L).standard_normal(L)).astype(np.float32)
