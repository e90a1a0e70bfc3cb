"""The host side of the recursive filters and of the hz / masking augmentations (tensorflowasr_amd/iir.py, augment.py): the ABI
table, Augmentation's `enable` with the new keys, the seeded draws and the yardsticks of iir_ref.py against the fixture recorded
from the reference's own SignalHz and SignalMask (tests/golden/make_hz_mask_golden.py), what the library refuses before it
touches a device, and the CPU finding the kernel's structure rests on: a float64 restatement of the chunked scan agrees with a
long-double evaluation one biquad at a time and does NOT on the transfer-function recursion.  No GPU."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
from scipy import signal

import iir_ref as ir
from tensorflowasr_amd import _lib, build
from tensorflowasr_amd.augment import DEVICE_KEYS, KEYS, SIGNAL_KEYS, UNSUPPORTED, Augmentation, Hz, Mask
from tensorflowasr_amd.iir import SOSFilter, default_padlen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355asr_sos_chunk", "mi355asr_sos_workspace_bytes", "mi355asr_sos_ragged", "mi355asr_mask_zone"]
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hz_mask_ref.npz"))
CASES = range(len(GOLD["seeds"]))
ZONE, RATIO = tuple(GOLD["zone"]), float(GOLD["mask_ratio"])


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
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "iir.hip")).read()
    assert "iir.hip" in build.SOURCES
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\bint(?:32_t)? %s\(([^;]*)\);" % name, hdr)
        assert m, name
        n_args = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r"^int(?:32_t)? %s\(" % name, src, re.M), name
        assert hasattr(lib, name)
    C = SOSFilter.CHUNK
    assert C == lib.mi355asr_sos_chunk() and C >= 16 and C % 16 == 0
    assert ("constexpr int kChunk = %d;" % C) in src


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.lib()
    wb = ctypes.c_size_t(0)
    assert lib.mi355asr_sos_workspace_bytes(2, 1000, 3, 1, ctypes.byref(wb)) == 0
    # the float64 intermediate signal of the longest edge, and more
    assert wb.value >= 2 * (1000 + 2 * SOSFilter.MAX_PADLEN) * 8
    for B, L, S, mode in ((0, 1000, 3, 1), (2, 0, 3, 1), (2, 1000, 0, 1), (2, 1000, 9, 0), (2, 1000, 3, 2)):
        assert lib.mi355asr_sos_workspace_bytes(B, L, S, mode, ctypes.byref(wb)) != 0, (B, L, S, mode)
    one = ctypes.c_void_p(16)                 # never dereferenced: every call below is refused on its arguments
    null = ctypes.c_void_p(None)

    def call(x=one, ln=one, sos=one, S=3, mode=1, padlen=21, zi=null, zf=null, y=one, ws=one, dtype=0):
        return lib.mi355asr_sos_ragged(x, dtype, ln, 2, 1000, sos, S, 0, mode, padlen, zi, zf, null, 0, 1.0, 0, y, 1000, ws, 1 << 30, null)
    for kw in (dict(x=null), dict(ln=null), dict(sos=null), dict(y=null), dict(ws=null), dict(S=0), dict(S=9), dict(mode=2), dict(padlen=-1),
               dict(padlen=SOSFilter.MAX_PADLEN + 1), dict(zi=one), dict(zf=one), dict(dtype=1), dict(ws=ctypes.c_void_p(8))):
        assert call(**kw) != 0, kw
        assert lib.mi355asr_last_error()
    assert lib.mi355asr_mask_zone(one, one, one, 2, 100, 100, 0.1, 1.5, 0.3, 1, 0, one, null) != 0
    assert lib.mi355asr_mask_zone(one, one, one, 2, 100, 100, -0.1, 0.5, 0.3, 1, 0, one, null) != 0
    assert lib.mi355asr_mask_zone(null, one, one, 2, 100, 100, 0.1, 0.9, 0.3, 1, 0, one, null) != 0


def test_python_refuses_before_any_launch():
    f = SOSFilter("cpu")                      # nothing below reaches the device
    sos = signal.butter(3, [0.2, 0.5], "bandstop", output="sos")
    assert default_padlen(sos) == 21 == 3 * (2 * 3 + 1 - 0)
    assert default_padlen(signal.butter(3, 0.2, output="sos")) == 3 * (2 * 2 + 1 - 1)          # what sosfiltfilt computes
    with pytest.raises(ValueError, match="row 1.*padlen, which is 21"):
        f.sosfiltfilt(np.zeros((2, 40), np.float32), [40, 21], sos)
    with pytest.raises(ValueError, match="sections"):
        f.sosfilt(np.zeros((1, 40), np.float32), None, np.tile(sos, (3, 1)))
    with pytest.raises(ValueError, match="sos must be"):
        f.sosfilt(np.zeros((2, 40), np.float32), None, np.zeros((3, 3, 6)))
    with pytest.raises(ValueError, match="padlen"):
        f.sosfiltfilt(np.zeros((1, 4000), np.float32), None, sos, padlen=2000)
    with pytest.raises(ValueError, match="zone"):
        Mask((0.1, 1.2))
    assert Mask("(0.1,0.9)").zone == (0.1, 0.9) == Mask((0.1, 0.9)).zone
    with pytest.raises(ValueError, match="starts"):
        Hz("cpu")(np.zeros((1, 100), np.float32), starts=[0.75])
    # the int() truncation of the zone: 0.9 * 10 is 9.000000000000002 in float64, 0.1 * 4001 truncates to 400
    m = Mask((0.1, 0.9))
    assert [m.span(n) for n in (1, 9, 10, 11, 4001)] == [(0, 0), (0, 8), (1, 9), (1, 9), (400, 3600)]
    assert [m.span(n) for n in (1, 9, 10, 11, 4001)] == [ir.mask_span(n, (0.1, 0.9)) for n in (1, 9, 10, 11, 4001)]


def test_augmentation_enable_with_the_signal_keys():
    assert SIGNAL_KEYS == ("hz", "masking") and DEVICE_KEYS == ("spec_aug", "speed")
    assert set(SIGNAL_KEYS) <= set(UNSUPPORTED) <= set(KEYS) and not set(SIGNAL_KEYS) & set(DEVICE_KEYS)
    for key in SIGNAL_KEYS:                   # the default is what it was
        with pytest.raises(NotImplementedError, match=key):
            Augmentation(config(**{key: True}))
        a = Augmentation(config(**{key: True}), unsupported="skip")
        assert not a.available() and a.skipped == [key]
    a = Augmentation(config(hz=True, masking=True), enable=("hz", "masking"))
    assert [g.key for g in a.augmentations] == ["masking", "hz"] and a.skipped == []
    assert isinstance(a.augmentations[0], Mask) and isinstance(a.augmentations[1], Hz)
    assert a.augmentations[0].zone == (0.1, 0.9) and a.augmentations[0].mask_ratio == 0.3 and a.augmentations[0].mask_with_noise is False
    a = Augmentation(config(spec_aug=True, speed=True, hz=True, masking=True), enable=DEVICE_KEYS + SIGNAL_KEYS)
    assert sorted(g.key for g in a.augmentations) == ["hz", "masking", "spec_aug", "speed"]
    with pytest.raises(NotImplementedError, match="hz"):
        Augmentation(config(hz=True, masking=True), enable=("masking",))
    for key in ("pitch", "vc"):
        with pytest.raises(NotImplementedError, match=key):
            Augmentation(config(**{key: True}), enable=DEVICE_KEYS + SIGNAL_KEYS)
        with pytest.raises(ValueError, match=key):
            Augmentation(config(), enable=(key,))


@pytest.mark.parametrize("k", CASES)
def test_draw_order_against_the_reference(k):
    """Hz.draw and Mask.draw make the reference's np.random calls: the same start, the same uniforms (through the outputs they
    give in hz_ref / mask_ref, which are the reference's expressions) and the same amount of generator state"""
    seed, x = int(GOLD["seeds"][k]), GOLD["x%d" % k].astype(np.float64)
    assert list(GOLD["hz_sizes%d" % k]) == [-1, len(x)]
    np.random.seed(seed)
    d = Hz("cpu").draw(len(x))
    assert np.random.random() == float(GOLD["hz_next%d" % k])
    assert d["start"] == float(GOLD["hz_start%d" % k]) and d["u"].shape == (len(x),)
    assert np.array_equal(ir.hz_ref(x, d["start"], d["u"]), GOLD["hz_out%d" % k])
    for noise in (0, 1):
        s, e = ir.mask_span(len(x), ZONE)
        assert list(GOLD["mask%d_sizes%d" % (noise, k)]) == [e - s]
        np.random.seed(seed)
        d = Mask(ZONE, RATIO, bool(noise), device="cpu").draw(len(x))
        assert np.random.random() == float(GOLD["mask%d_next%d" % (noise, k)])
        assert d["u"].shape == (e - s,)
        y = ir.mask_ref(x, ZONE, RATIO, bool(noise), d["u"])
        assert np.array_equal(y, GOLD["mask%d_out%d" % (noise, k)])
        assert np.array_equal(np.signbit(y), np.signbit(GOLD["mask%d_out%d" % (noise, k)]))


def test_augmentation_draw_picks_then_draws():
    a = Augmentation(config(hz=True), enable="hz")
    random.seed(3)
    np.random.seed(3)
    aug, d = a.draw(50)
    np.random.seed(3)
    assert aug.key == "hz" and d["start"] == float(np.clip(np.random.random(), 0.01, 0.699))
    assert np.array_equal(d["u"], np.random.random(50))


def test_long_double_yardsticks_agree_with_scipy():
    rng = np.random.default_rng(7)
    x = (rng.uniform(-1, 1, 500) * 0.5).astype(np.float32).astype(np.float64)
    sos = signal.butter(3, [0.2, 0.5], "bandstop", output="sos")
    b, a = signal.butter(3, [0.2, 0.5], "bandstop")
    assert np.abs(ir.sosfiltfilt_ld(sos, x, 21) - signal.sosfiltfilt(sos, x, padlen=21)).max() < 1e-13
    assert np.abs(ir.filtfilt_ld(b, a, x) - signal.filtfilt(b, a, x)).max() < 1e-12
    zi = rng.standard_normal((3, 2))
    y, zf = signal.sosfilt(sos, x, zi=zi)
    yl, zl = ir.sosfilt_ld(sos, x, zi)
    assert np.abs(yl - y).max() < 1e-13 and np.abs(zl - zf).max() < 1e-13
    assert np.abs(ir.sosfilt_zi_ld(sos) - signal.sosfilt_zi(sos)).max() < 1e-13
    # the two forms are the same filter: the reference's call and the sections agree far below a float32 ulp
    assert np.abs(ir.filtfilt_ld(b, a, x) - ir.sosfiltfilt_ld(sos, x, 21)).max() < 1e-12


X6000 = (np.random.default_rng(1).uniform(-1, 1, 6000) * 0.5).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("start", [0.01, 0.2, 0.699])
def test_chunked_biquad_scan_stays_within_scipys_own_distance(start):
    """measured at chunk 64: 0.76 D, 0.90 D and 0.84 D (D = 2.1e-14, the floor 4.4e-16, 7.3e-13)"""
    sos = signal.butter(3, [start, start + 0.3], "bandstop", output="sos")
    y_ld = ir.sosfiltfilt_ld(sos, X6000, 21)
    D = ir.distance(signal.sosfiltfilt(sos, X6000, padlen=21), y_ld, X6000)
    err = float(np.abs(ir.sosfiltfilt_chunked(sos, X6000, 21, 64) - y_ld).max())
    print("start %g: D = %.3g, chunked scan - long double = %.3g = %.2f D" % (start, D, err, err / D))
    assert err <= 8 * D


@pytest.mark.parametrize("start", [0.01, 0.35, 0.699])
def test_chunked_biquad_scan_meets_the_device_bound_past_a_tile_and_a_scan_stage(start):
    """The float64 restatement at the kernel's chunk (128), rounded to float32 as the device rounds, under the device tests' own
    bound at the extended lengths of tests/test_gpu_iir_tiles.py: the algorithm meets the bound there whatever the kernel does.
    Measured on these rows, worst over the lengths, float64 err / D and max(err - 2^-24 |y_ld|, 0) / D after the rounding: 1.25
    and 0.010 (start 0.01), 0.77 and 0 (0.35), 1.64 (N = W - 1) and 0.739 (N = 2 SC + 5) (0.699); the bound is 8.  The easiest
    start leaves out SC and 2 SC + 5, which keeps the three cases near 10 s."""
    from iir_cases import SC, W, check_bound
    assert W == 64 * SOSFilter.CHUNK and SC == 1024 * SOSFilter.CHUNK
    sos = signal.butter(3, [start, start + 0.3], "bandstop", output="sos")
    rng = np.random.default_rng(29)
    for N in (W - 1, W, W + 1, 2 * W + 1, SC, SC + 1, 2 * SC + 5):
        if start == 0.35 and N in (SC, 2 * SC + 5):
            rng.uniform(-1, 1, N - 42)                  # the later rows keep their draws
            continue
        x = (rng.uniform(-1, 1, N - 42) * 0.5).astype(np.float32).astype(np.float64)
        y_ld = ir.sosfiltfilt_ld(sos, x, 21)
        D = ir.distance(signal.sosfiltfilt(sos, x, padlen=21), y_ld, x)
        y = ir.sosfiltfilt_chunked(sos, x, 21, SOSFilter.CHUNK)
        err = float(np.abs(y - y_ld).max())
        r = check_bound(y.astype(np.float32), y_ld, D)
        print("start %g, N = %d: D = %.3g, float64 err = %.2f D, after rounding to float32: %.3f" % (start, N, D, err / D, r))


def test_chunked_transfer_function_scan_fails():
    """The 6th-order direct-form recursion joined over chunks by its 6 x 6 transition is NOT usable: at start 0.699 the
    transition's entries reach 1.8e4 and the result is 3.7e-6 = 1 494 D away from the long-double evaluation (D = 2.5e-9).  Do not retry
    it without new arithmetic."""
    start = 0.699
    b, a = signal.butter(3, [start, start + 0.3], "bandstop")
    y_ld = ir.filtfilt_ld(b, a, X6000)
    D = ir.distance(signal.filtfilt(b, a, X6000), y_ld, X6000)
    err = float(np.abs(ir.filtfilt_chunked_tf(b, a, X6000, 64) - y_ld).max())
    print("start %g: D = %.3g, chunked transfer-function scan - long double = %.3g = %.0f D" % (start, D, err, err / D))
    assert err > 8 * D and err > 2.0 ** -24
