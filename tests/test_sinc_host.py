"""The host side of the band-limited resampler and of the pitch augmentation (tensorflowasr_amd/resample.py: SincResampler,
augment.py: Pitch): the tests' oracle sinc_ref.py against itself (scalar and vectorised), against scipy.signal.resample_poly on
band-limited noise and against its own float32 restatement (where the GPU bound C_R comes from), the table, the two DC gains,
Pitch's draw and zone, Augmentation's `unpinned` and the ABI table.  Nothing here has been compared with the resampy or librosa
packages: they are not available.  No GPU."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
from scipy import signal

import sinc_ref as sn
from tensorflowasr_amd import _lib, build, resample
from tensorflowasr_amd.augment import DEVICE_KEYS, KEYS, SIGNAL_KEYS, UNPINNED_KEYS, UNSUPPORTED, Augmentation, Pitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355asr_sinc_plan", "mi355asr_sinc_workspace_bytes", "mi355asr_sinc_resample"]
GPU_RATIOS = [0.25, 2 ** (-3 / 12), 0.9, 0.999, 1.0, 1.0000001, 1.5, 2 ** (3 / 12), 4.0]         # test_gpu_sinc.py's
U24 = 2.0 ** -24


def config(**active):
    """the reference's augments_config as asr/configs/am_data.yml ships it, everything off"""
    cfg = {"noise": {"active": False, "sample_rate": 16000, "SNR": [0, 15], "noises": "./noise"},
           "masking": {"active": False, "zone": "(0.1,0.9)", "mask_ratio": 0.3, "mask_with_noise": False},
           "pitch": {"active": False, "zone": "(0.0,1.0)", "sample_rate": 16000, "factor": "(-1,3)"},
           "speed": {"active": False, "factor": "(0.9,1.2)"},
           "rir": {"active": False, "sample_rate": 16000},
           "hz": {"active": False},
           "vc": {"active": False},
           "spec_aug": {"active": False, "window": 10, "ratio": 0.5}}
    for k, v in active.items():
        cfg[k]["active"] = v
    return cfg


def test_header_signatures_and_sources_agree():
    hdr = open(os.path.join(ROOT, "include", "mi355asr.h")).read()
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "sinc_resample.hip")).read()
    assert "sinc_resample.hip" in build.SOURCES
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\bint(?:32_t)? %s\(([^;]*)\);" % name, hdr)
        assert m, name
        n_args = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r"^int(?:32_t)? %s\(" % name, src, re.M), name
        assert hasattr(lib, name)
    # the plan call needs no device: the constants of the kernel, of resample.py and of the oracle are the same
    p = resample._sinc_plan(lib, 1.0)
    assert p["table_floats"] >= sn.NW and p["table_floats"] % 4 == 0 and p["tile"] >= 64
    assert ("constexpr int kTile = %d;" % p["tile"]) in src and ("constexpr int kTabFloats = %d;" % p["table_floats"]) in src
    assert p["ratio_min"] <= 0.25 and p["ratio_max"] >= 4.0
    assert (resample.SINC_ZEROS, resample.SINC_NT, resample.SINC_ROLLOFF, resample.SINC_BETA) == (sn.ZEROS, sn.NT, sn.ROLLOFF, sn.BETA)
    for r in GPU_RATIOS:
        assert resample._sinc_plan(lib, r)["wing"] == sn.NW // int(min(1.0, r) * sn.NT), r
    for bad in (0.0, -1.0, float("nan"), float("inf"), p["ratio_min"] * 0.999, p["ratio_max"] * 1.001):
        assert lib.mi355asr_sinc_plan(bad, None, None, None, None, None) == -1
        with pytest.raises(ValueError, match="outside the supported 0.25 .. 4"):
            resample._sinc_plan(lib, bad)
    assert np.array_equal(resample.sinc_table(), sn.WIN)
    for n, r in ((0, 1.5), (1, 0.25), (77, 0.9), (3000, 2 ** 0.25), (10, 0.5)):
        assert resample.sinc_out_length(n, r) == sn.out_length(n, r) and resample.sinc_valid_length(n, r) == sn.valid_length(n, r)
    assert resample.sinc_out_length(10, 0.5) == 5 == resample.sinc_valid_length(10, 0.5) and resample.sinc_out_length(77, 0.9) == 70


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.lib()
    wb = ctypes.c_size_t(0)
    assert lib.mi355asr_sinc_workspace_bytes(3, ctypes.byref(wb)) == 0 and wb.value >= 3 * 48
    assert lib.mi355asr_sinc_workspace_bytes(0, ctypes.byref(wb)) == -1
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(None)       # never dereferenced: every call below is refused on its arguments
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(ratio=1.0, n=100, out=100, off=None, B=1, x=one, tab=one, y=one, ws=one, mode=0, Lpad=1000, Opad=1000, nbytes=1 << 20):
        r, ln, ol = np.array([ratio]), np.array([n], np.int64), np.array([out], np.int64)
        of = null if off is None else hp(np.array([off], np.int64))
        return lib.mi355asr_sinc_resample(x, B, Lpad, hp(r), hp(ln), hp(ol), of, null, tab, mode, y, Opad, ws, nbytes, null)
    for kw in (dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=0.2499), dict(ratio=4.001),
               dict(B=0), dict(n=-1), dict(n=1001), dict(out=-1), dict(out=1001), dict(off=-1), dict(off=901), dict(x=null), dict(tab=null),
               dict(y=null), dict(ws=null), dict(tab=ctypes.c_void_p(20)), dict(mode=2), dict(Lpad=0), dict(Opad=0), dict(nbytes=8)):
        assert call(**kw) != 0, kw
        assert lib.mi355asr_last_error()
    assert call(ratio=0.2) == -1 and b"0.2 is outside 0.25 .. 4" in lib.mi355asr_last_error()


@pytest.mark.parametrize("r", [0.25, 0.9, 1.0, 1.19, 4.0])
def test_scalar_and_vectorised_forms_agree(r):
    """to 1e-15 of the row's largest S1 = sum |w_k x_k|: the two forms differ in the order of their sums only"""
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 77, 3000):
        x = rng.standard_normal(n)
        a = sn.resample_scalar(x, r)
        b, s1 = sn.resample(x, r)
        assert len(a) == len(b) == sn.out_length(n, r)
        assert not a[sn.valid_length(n, r):].any() and not b[sn.valid_length(n, r):].any()
        if len(a):
            worst = float(np.abs(a - b).max()) / max(float(s1.max()), 1e-300)
            print("ratio %g, %d samples: scalar - vectorised = %.3g of max S1" % (r, n, worst))
            assert worst <= 1e-15
    # a caller's output length: cut, and zero-filled
    x = rng.standard_normal(77)
    full = sn.resample(x, r)[0]
    assert np.array_equal(sn.resample(x, r, out_len=10)[0], full[:10])
    long = sn.resample(x, r, out_len=len(full) + 5)[0]
    assert np.array_equal(long[:len(full)], full) and not long[len(full):].any()
    assert np.array_equal(sn.resample_scalar(x, r, out_len=len(full) + 5), np.concatenate([sn.resample_scalar(x, r), np.zeros(5)]))


def test_the_table_and_the_dc_gains():
    w = sn.WIN
    assert w.shape == (32769,) == (sn.NW,) and w[0] == sn.ROLLOFF and w.dtype == np.float64
    env = np.abs(w[:-1]).reshape(sn.ZEROS, sn.NT).max(axis=1)           # the largest entry between two zero crossings of the window grid
    assert (np.diff(env) < 0).all() and env[-1] < 1e-7 and abs(w[-1]) < 1e-7
    ones = np.ones(3000)
    for r in (1.0, 1.19, 4.0):                                          # 1 - 3e-8 for r >= 1, on the table's grid
        y = sn.resample(ones, r)[0]
        g = y[len(y) // 2 - 48:len(y) // 2 + 48]                        # from a multiple of 4: every fourth sits on a sample at r = 4
        print("ratio %g: DC gain - 1 = %.3g .. %.3g" % (r, g.min() - 1, g.max() - 1))
        # between the grid's phases the linear interpolation moves it by a few 1e-8: measured -3.3e-8 .. +2.3e-8 at 1.19
        assert np.abs(g[::4 if r == 4.0 else 1] - (1 - 3e-8)).max() < (1e-8 if r != 1.19 else 6e-8)
    y = sn.resample(ones, 0.9)[0]                                       # 1.00058: step = int(0.9 * 512) = 460 and not 460.8
    g = y[len(y) // 2 - 50:len(y) // 2 + 50]
    print("ratio 0.9: DC gain = %.6f .. %.6f" % (g.min(), g.max()))
    # the truncated step samples the filter 0.17 % too densely: up to 1.00058, depending on the output's phase (measured 1.000094 .. 1.000577)
    assert abs(g.max() - 1.00058) < 5e-6 and 1.0 < g.min() < g.max()
    x = np.random.default_rng(0).standard_normal(500)                   # r = 1 is a low-pass at ROLLOFF, not a copy
    y = sn.resample(x, 1.0)[0]
    assert len(y) == 500 and np.abs(y - x)[100:400].max() > 0.01


@pytest.mark.parametrize("up,down", [(9, 10), (6, 5), (1, 2), (2, 1)])
def test_against_resample_poly_on_band_limited_noise(up, down):
    """noise band-limited by resample_poly down 4 and back up: both resamplers are transparent there.  Measured: 6.5e-4 to 8.8e-4
    of max |y| (resample_poly's default Kaiser filter is the cruder of the two)"""
    rng = np.random.default_rng(5)
    x = signal.resample_poly(signal.resample_poly(rng.standard_normal(12000), 1, 4), 4, 1)
    want = signal.resample_poly(x, up, down)
    got = sn.resample(x, up / down)[0]
    n = min(len(want), len(got))
    assert abs(len(want) - len(got)) <= 1 and n > 4400
    err = float(np.abs(got[2000:n - 2000] - want[2000:n - 2000]).max()) / float(np.abs(want).max())
    print("%d/%d: oracle - resample_poly = %.3g of max |y|" % (up, down, err))
    assert err <= 2e-3


@pytest.mark.parametrize("r", GPU_RATIOS)
def test_float32_restatement_stays_within_32_ulp_of_s1(r):
    """|y32 - y64| <= 32 2^-24 S1 per output.  Measured: 9.1 to 14.6 over the nine ratios; test_gpu_sinc.py's C_R = 64 is four
    times the worst, rounded up to a power of two."""
    x = np.random.default_rng(3).standard_normal(6000).astype(np.float32)
    y64, s1 = sn.resample(x, r)
    y32 = sn.resample_f32(x, r)
    assert y32.dtype == np.float32 and len(y32) == len(y64) and (s1[:sn.valid_length(6000, r)] > 0).all()
    m = s1 > 0
    worst = float((np.abs(y32[m] - y64[m]) / (U24 * s1[m])).max())
    print("ratio %.9g: float32 restatement worst ratio %.2f" % (r, worst))
    assert worst <= 32 and not y32[~m].any()


def test_pitch_draw_and_zone():
    p = Pitch("(0.2,0.8)", 16000, "(-1,5)", device="cpu")
    assert p.key == "pitch" and p.zone == (0.2, 0.8) and p.factor == (-1.0, 5.0) and p.sample_rate == 16000
    assert Pitch((0.0, 1.0), factor=(-1, 3), device="cpu").factor == (-1.0, 3.0)
    np.random.seed(9)
    d = p.draw(16000)
    nxt = np.random.random()
    np.random.seed(9)
    scale = 5 - (-1)
    assert d == {"steps": np.random.random() * scale - scale / 2}       # the reference's expression, one call
    assert np.random.random() == nxt and -3 <= d["steps"] <= 3
    # int(n * zone[i]): 0.8 * 9601 = 7680.8, 0.2 * 4000 = 800.0000000000001 -> 800, 0.9 * 10 = 9.000000000000002 -> 9
    assert [p.span(n) for n in (16000, 9601, 4000, 1500, 1, 0)] == [(3200, 12800), (1920, 7680), (800, 3200), (300, 1200), (0, 0), (0, 0)]
    assert [p.span(n) for n in (16000, 9601, 4000, 1500)] == [sn.zone(n, (0.2, 0.8)) for n in (16000, 9601, 4000, 1500)]
    assert Pitch((0.1, 0.9), device="cpu").span(10) == (1, 9) == (int(10 * 0.1), int(10 * 0.9))
    assert Pitch.rate(0) == 1.0 and Pitch.rate(12) == 0.5 and Pitch.rate(-3) == 2.0 ** 0.25 == sn.rate_of(-3)
    with pytest.raises(ValueError, match="zone"):
        Pitch((0.1, 1.2), device="cpu")


def test_augmentation_unpinned():
    assert UNPINNED_KEYS == ("pitch",) and set(UNPINNED_KEYS) <= set(UNSUPPORTED) <= set(KEYS)
    assert not set(UNPINNED_KEYS) & set(DEVICE_KEYS + SIGNAL_KEYS)
    with pytest.raises(NotImplementedError, match="pitch"):             # the default is what it was
        Augmentation(config(pitch=True))
    with pytest.raises(NotImplementedError, match="pitch"):
        Augmentation(config(pitch=True), enable=DEVICE_KEYS + SIGNAL_KEYS)
    a = Augmentation(config(pitch=True), unsupported="skip")
    assert not a.available() and a.skipped == ["pitch"]
    with pytest.raises(ValueError, match="pitch"):
        Augmentation(config(), enable=("pitch",))
    for bad in ("vc", "hz", "nothing"):
        with pytest.raises(ValueError, match="unpinned.*%s" % bad):
            Augmentation(config(), unpinned=(bad,))
    for unpinned in (("pitch",), "pitch"):
        a = Augmentation(config(pitch=True), unpinned=unpinned)
        assert a.available() and a.skipped == [] and [g.key for g in a.augmentations] == ["pitch"]
        g = a.augmentations[0]
        assert isinstance(g, Pitch) and g.zone == (0.0, 1.0) and g.factor == (-1.0, 3.0) and g.sample_rate == 16000
    assert not Augmentation(config(), unpinned=("pitch",)).available()   # the key is off: nothing to run
    a = Augmentation(config(pitch=True, hz=True, vc=True), unpinned=("pitch",), enable=("hz",), unsupported="skip")
    assert sorted(g.key for g in a.augmentations) == ["hz", "pitch"] and a.skipped == ["vc"]
    random.seed(2)
    np.random.seed(2)
    aug, d = Augmentation(config(pitch=True), unpinned=("pitch",)).draw(5000)
    np.random.seed(2)
    assert aug.key == "pitch" and d == {"steps": np.random.random() * 4 - 2}
