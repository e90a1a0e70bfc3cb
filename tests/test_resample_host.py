"""CPU tests of tensorflowasr_amd.resample's host functions: the filter design and the resampling formula against scipy, the
output and stream emission counts."""
import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

from resample_ref import RATIOS, resample_formula, taps_and_gain
from tensorflowasr_amd.resample import design_filter, out_length, ratio, stream_emitted


@pytest.mark.parametrize("up,down", RATIOS)
def test_design_filter_equals_scipy_firwin(up, down):
    h, half = design_filter(up, down)
    assert half == 10 * max(up, down) and h.dtype == np.float64 and len(h) == 2 * half + 1
    ref = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert np.abs(h - ref).max() <= 1e-12


@pytest.mark.parametrize("up,down", RATIOS)
def test_formula_and_out_length_equal_scipy_resample_poly(up, down):
    rng = np.random.default_rng(up * 1000 + down)
    for L in (1, 30, 441, 3001):
        x = rng.standard_normal(L)
        ref = resample_poly(x, up, down)
        assert out_length(L, up, down) == len(ref)
        y = resample_formula(x, up, down)
        assert y.shape == ref.shape and np.abs(y - ref).max() <= 1e-12


def test_ratio_reduces_and_refuses_large_ratios():
    assert ratio(8000, 16000) == (2, 1) and ratio(48000, 16000) == (1, 3) and ratio(44100, 16000) == (160, 441)
    assert ratio(11025, 16000) == (640, 441) and ratio(16000, 16000) == (1, 1)
    with pytest.raises(ValueError, match="16001/96000"):
        ratio(96000, 16001)


def test_taps_per_output_of_the_shipped_ratios():
    assert [taps_and_gain(u, d)[0] for u, d in ((2, 1), (1, 3), (160, 441), (320, 441), (640, 441))] == [21, 61, 56, 28, 21]
    for u, d in RATIOS:
        assert 1.0 <= taps_and_gain(u, d)[1] <= 2.25


@pytest.mark.parametrize("up,down", RATIOS)
def test_stream_emission_is_monotone_and_totals_the_output_length(up, down):
    rng = np.random.default_rng(7 * up + down)
    half = 10 * max(up, down)
    for N in (1, 17, 1000, 20001):
        sizes = []
        while sum(sizes) < N:
            sizes.append(int(rng.choice([1, 1, 7, 160, 1280])))
        sizes[-1] -= sum(sizes) - N
        pos, emitted, total = 0, 0, 0
        for p in sizes:
            pos += p
            e = stream_emitted(pos, up, down)
            assert e >= emitted
            # final: the newest sample an emitted output touches has arrived; the next output still waits for one
            assert e == 0 or ((e - 1) * down + half) // up <= pos - 1
            assert (e * down + half) // up >= pos
            total += e - emitted
            emitted = e
        assert emitted <= out_length(N, up, down)
        total += out_length(N, up, down) - emitted          # the flush
        assert total == out_length(N, up, down) == len(resample_poly(np.zeros(N), up, down))


def test_counts_are_exact_far_beyond_32_and_53_bits():
    N = 10 ** 10
    for up, down in RATIOS + [(639, 640)]:
        half = 10 * max(up, down)
        assert out_length(N, up, down) == (N * up + down - 1) // down
        assert stream_emitted(N, up, down) == (N * up - half - 1) // down + 1
        assert isinstance(out_length(N, up, down), int) and isinstance(stream_emitted(N, up, down), int)
    assert out_length(10 ** 17 + 1, 2, 1) == 2 * 10 ** 17 + 2 and stream_emitted(0, 1, 3) == 0


def test_plan_and_stream_sizes_of_the_library():
    """the host half of the C entry points: taps and tile per ratio, the refusal of a ratio above 640, and an output capacity
    per step that no packet or flush can exceed"""
    import ctypes
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    for up, down in RATIOS + [(1, 640), (639, 640)]:
        v = [ctypes.c_int32() for _ in range(4)]
        assert lib.mi355asr_resample_plan(up, down, *[ctypes.byref(c) for c in v]) == 0
        taps, stride, tile, floats = (c.value for c in v)
        assert taps == taps_and_gain(up, down)[0] and stride >= taps and stride % 2 == 1
        assert tile % (4 * up) == 0 and 1024 <= tile < 1024 + 4 * up and floats >= up * stride and floats % 4 == 0
        sb, wb, oc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        max_packet = 1280
        assert lib.mi355asr_resample_streams_bytes(up, down, 3, max_packet, ctypes.byref(sb), ctypes.byref(wb), ctypes.byref(oc)) == 0
        assert sb.value == 3 * 4 * (taps - 1 + max_packet) and wb.value >= 3 * 6 * 4
        for N in (0, 1, 5, 1279, 1280, 99999, 10 ** 10):
            assert stream_emitted(N + max_packet, up, down) - stream_emitted(N, up, down) <= oc.value
            assert out_length(N, up, down) - stream_emitted(N, up, down) <= oc.value
    assert lib.mi355asr_resample_plan(641, 1, None, None, None, None) == -1
    assert b"641/1" in lib.mi355asr_last_error()
    assert lib.mi355asr_resample_plan(1, 0, None, None, None, None) == -1


def test_restated_plan_equals_the_library_and_names_the_staging_boundary():
    """resample_ref.plan (what the GPU tests print and size their inputs by) against mi355asr_resample_plan, and the LDS figures at
    the ratios chosen for them: 1/18 is staged with 80 720 of 81 920 bytes, 1/19 is not; 147/640 is staged with 77 920"""
    import ctypes
    from resample_ref import LARGE_K, MORE_RATIOS, SMALL_K, filter_gap, plan
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    for up, down in sorted(set(RATIOS + MORE_RATIOS + SMALL_K + LARGE_K)):
        v = [ctypes.c_int32() for _ in range(4)]
        assert lib.mi355asr_resample_plan(up, down, *[ctypes.byref(c) for c in v]) == 0
        p = plan(up, down)
        assert [c.value for c in v] == [p["taps"], p["stride"], p["tile"], p["table_floats"]], (up, down)
        assert filter_gap(up, down) <= 1e-12
    assert (plan(1, 18)["staged"], plan(1, 18)["lds"]) == (True, 80720) and not plan(1, 19)["staged"]
    assert (plan(147, 640)["staged"], plan(147, 640)["lds"]) == (True, 77920)
    assert [plan(u, d)["staged"] for u, d in ((3, 61), (101, 640), (1, 640), (640, 1), (640, 441))] == [False, False, False, True, True]
    assert plan(640, 441)["lds"] > 64 * 1024 > plan(640, 1)["lds"]
