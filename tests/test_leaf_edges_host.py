"""The LEAF frontend's slot arithmetic and the add_wav_info branch's scratch carve on the host (no GPU): tests/leaf_edges.py restates
both from csrc/leaf.hip and csrc/api.hip; here every length is walked through the restatement, and the restatement is held to the
float64 oracle's own geometry."""
import numpy as np

import leaf_edges as le
from helpers import co

_SWEEP = {}


def _sweep():
    """pooling_model for both tiles and every L in 1 .. SWEEP_MAX, computed once: {tile: {L: (problems, used)}}"""
    if not _SWEEP:
        for tile in le.TILES:
            _SWEEP[tile] = {L: le.pooling_model(L, tile) for L in range(1, le.SWEEP_MAX + 1)}
    return _SWEEP


def test_restated_geometry_is_the_oracles():
    """same_pad, F and pl against the oracle's SAME rule, and window_pairs against a direct enumeration"""
    for L in range(1, 1300):
        F, lo, _ = co.same_pad(L, le.KTAPS, le.HOP)
        assert (F, lo) == le.same_pad(L, le.KTAPS, le.HOP)
    for a in range(-2000, 2000):
        assert int(le.cdiv(a, 128)) == int(a / 128) and int(le.cdiv(a, 512)) == int(a / 512)       # C division, towards zero
    for L in (1, 2, 159, 160, 161, 401, 513, 740):
        F, pl = le.same_pad(L, le.KTAPS, le.HOP)
        n, f = le.window_pairs(L, F, pl)
        want = {(i, j) for i in range(L) for j in range(F) if 0 <= i - (le.HOP * j - pl) <= le.KTAPS - 1}
        assert set(zip(n.tolist(), f.tolist())) == want and len(n) == len(want)


def test_slot_arithmetic_is_complete_for_every_length():
    """both tiles, every L in 1 .. 2 * 2560 + 512 (two periods of lcm(512, 160)): every (position, frame) pair inside the pooling
    window lands in exactly one in-range slot of its tile (and of its wave), the gather for the frame visits that tile, and the
    gather reads nothing outside the tiles the conv kernel wrote"""
    assert le.SWEEP_MAX == 2 * 2560 + 512 and set(le.TILES.items()) == {(128, 4), (512, 7)}
    for tile, per_len in _sweep().items():
        assert sorted(per_len) == list(range(1, le.SWEEP_MAX + 1))
        bad = [p for L in per_len for p in per_len[L][0]]
        assert not bad, bad[:10]


def test_slot_model_notices_a_one_off():
    """the sweep is not vacuous: one slot fewer, or a gather window one tile narrower, fails for some length"""
    saved = dict(le.TILES)
    try:
        le.TILES[512], le.TILES[128] = 6, 3
        assert any(le.pooling_model(L, 512)[0] for L in range(1, 2561))
        assert any(le.pooling_model(L, 128)[0] for L in range(1, 2561))
    finally:
        le.TILES.update(saved)
    real = le.gather_range
    try:
        le.gather_range = lambda f, pl, tile, nrel, NH: tuple(np.asarray(v) + d for v, d in zip(real(f, pl, tile, nrel, NH), (1, 0)))
        assert any(le.pooling_model(L, 512)[0] for L in range(1, 2561))
        le.gather_range = lambda f, pl, tile, nrel, NH: tuple(np.asarray(v) + d for v, d in zip(real(f, pl, tile, nrel, NH), (0, -1)))
        assert any(le.pooling_model(L, 128)[0] for L in range(1, 2561))
    finally:
        le.gather_range = real


def test_gpu_lengths_cover_every_slot_and_pad():
    """the GPU length list exercises everything any length can: every slot of a 512-tile, every rel of a wave and of a 128-tile,
    in an interior tile, the first tile, every tile-index residue mod 5 and the partial last tile, and both ends of the left pad"""
    lengths = le.gpu_lengths(default_terms=True)
    assert len(set(lengths)) == len(lengths)
    for part in (le.SHORT, le.TILE_EDGES, le.PAD_RESIDUES, le.COVERAGE, le.FRAME_COUNTS):
        assert set(part) <= set(le.gpu_lengths())                  # the lengths every `terms` runs
    used, pads = le.coverage(le.gpu_lengths())
    reach = {t: set().union(*(u for _, u in per_len.values())) for t, per_len in _sweep().items()}
    all_pads = {le.same_pad(L, le.KTAPS, le.HOP)[1] for L in range(1, le.SWEEP_MAX + 1)}
    # the left pad: (401 - r) / 2 for r = 1 .. 160 samples in the last frame -> 120 (L a multiple of the hop) .. 200 (L = 160 k + 1)
    assert (min(all_pads), max(all_pads)) == (120, 200) and {120, 121, 200} <= pads
    req = le.required_coverage()
    for t in le.TILES:
        assert not le.UNREACHABLE[t] & reach[t]                    # no length in two periods reaches them (the reason: leaf_edges.py)
        assert req[t] - le.UNREACHABLE[t] <= used[t], sorted(req[t] - le.UNREACHABLE[t] - used[t])
        assert reach[t] <= used[t], sorted(reach[t] - used[t])     # ... and nothing else that is reachable is left out
    # a partial last tile is as full as it can be and still be partial, and as empty
    assert {L % 512 for L in lengths} >= {1, 511} and {L % 128 for L in lengths} >= {1, 127}


# ---- add_wav_info ----------------------------------------------------------------------------------------------------------------
CONFIGS = [((8, 5, 4, 4), 144), ((8, 5, 4, 4), 256), ((16, 5, 4, 4), 144), ((16, 5, 4, 4), 256)]


def test_wav_strides_and_floor():
    assert co.wave_pick_scales(640) == [8, 5, 4, 4] and co.wave_pick_scales(1280) == [16, 5, 4, 4]
    assert le.wav_min_length((8, 5, 4, 4)) == 1281 and le.wav_min_length((16, 5, 4, 4)) == 2561
    assert le.wav_stages((8, 5, 4, 4), 144) == [(32, 64, 5), (64, 96, 4), (96, 128, 4)] == le.wav_stages((8, 5, 4, 4), 256)
    # what the floor stands for: np.pad's reflect (the oracle) keeps reflecting below 3 rows, tf.pad REFLECT needs pad < size
    for strides, _ in CONFIGS:
        hopred = int(np.prod(strides))
        for L in range(1, 4001):
            T = -(-L // hopred)
            assert (T >= le.WAV_MIN_FRAMES) == (L >= le.wav_min_length(strides))


def test_wav_scratch_fits_for_every_accepted_length():
    """every write into, and GEMM read from, the six buffers of run_wavpick stays inside what the carve gives the buffer, for
    every accepted L up to 4000, at one row and at an odd batch; the carve itself fits the plan's wavpick_floats(F * hop)"""
    for strides, d in CONFIGS:
        hopred = int(np.prod(strides))
        hop = hopred // 4
        accepted = [L for L in range(1, 4001) if L >= le.wav_min_length(strides)]
        assert accepted and accepted[0] == le.wav_min_length(strides)
        for L in accepted:
            for Bp in (1, 3):
                acc, carved, T = le.wavpick_accesses(strides, d, Bp, L)
                assert T == -(-L // hopred) >= le.WAV_MIN_FRAMES
                over = [(what, buf, n, cap) for what, buf, n, cap in acc if n > cap]
                assert not over, (strides, d, Bp, L, over)
                F = -(-L // hop)
                assert carved <= le.wavpick_floats(strides, d, Bp, F * hop)
        # the oracle's frame count is the restatement's
        for L in (accepted[0], accepted[0] + hopred - 1, 4000):
            assert le.wavpick_accesses(strides, d, 1, L)[2] == -(-L // hopred)


def test_wav_scratch_overflows_below_the_floor():
    """why the floor is not only the reference's: for very short inputs the padded copies outgrow their buffer (the reflect copy
    would write into the buffer it reads) -- every such length lies below the floor"""
    for strides, d in CONFIGS:
        over = [L for L in range(1, le.wav_min_length(strides))
                if any(n > cap for _, _, n, cap in le.wavpick_accesses(strides, d, 1, L)[0])]
        assert over and over == list(range(1, over[-1] + 1))
        assert over[-1] == 19 * strides[0]                   # (T + 6) * 128 > (T0 + 8) * 32 at T = 1: T0 < 20
        what = {w for L in over for w, _, n, cap in le.wavpick_accesses(strides, d, 1, L)[0] if n > cap}
        assert "final zero pad" in what and any(w.endswith("reflect pad") for w in what)
