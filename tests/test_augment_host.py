"""The host side of the far-field simulator (tensorflowasr_amd/augment.py): the ABI table, the reference's Augmentation parsing, the
seeded draws against what the reference's own classes drew (tests/golden/augment_draws.json), and the float64 oracle of
augment_ref.py against scipy and against closed forms.  No GPU."""
import json
import os
import random
import re

import numpy as np
import pytest

import augment_ref as ar
from tensorflowasr_amd import _lib, build
from tensorflowasr_amd.augment import KEYS, UNSUPPORTED, Augmentation, ImageSourceRIR, cut_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "augment_draws.json")))
NEW = ["mi355asr_rir_workspace_bytes", "mi355asr_rir_generate", "mi355asr_fir_ragged", "mi355asr_mix_snr"]


def test_header_signatures_and_sources_agree():
    hdr = open(os.path.join(ROOT, "include", "mi355asr.h")).read()
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "augment.hip")).read()
    assert "augment.hip" in build.SOURCES
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r"^int %s\(" % name, src, re.M), name
    # the limits the Python layer checks are the kernels'
    from tensorflowasr_amd.augment import MAX_TAPS
    assert "constexpr int kFirMaxK = %d;" % MAX_TAPS in src and "constexpr int kRirMaxN = %d;" % MAX_TAPS in src


def config(**active):
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


def bank():
    return [np.full(n, 0.5, np.float32) for n in GOLDEN["bank_lens"]]


def test_augmentation_parsing():
    assert set(KEYS) == set(config()) and set(UNSUPPORTED) == set(KEYS) - {"rir", "noise"}
    a = Augmentation(config())
    assert not a.available() and a["rir"]["sample_rate"] == 16000 and a["nothing"] is None
    with pytest.raises(KeyError, match="echo"):
        Augmentation(dict(config(), echo={"active": False}))
    for key in UNSUPPORTED:
        with pytest.raises(NotImplementedError, match=key):
            Augmentation(config(**{key: True}))
        a = Augmentation(config(**{key: True, "rir": True}), unsupported="skip")
        assert a.available() and [g.key for g in a.augmentations] == ["rir"] and a.skipped == [key]
    cfg = config(rir=True, noise=True)
    a = Augmentation(cfg, noise_bank=bank())
    assert [g.key for g in a.augmentations] == ["noise", "rir"]          # the order of the configuration, as in the reference
    assert cfg["rir"]["active"] is True                                   # the caller's dictionary is left as it was
    with pytest.raises(ValueError):
        Augmentation(config(), unsupported="ignore")
    # the reference's am_data.yml ships with spec_aug active and everything else off
    assert not Augmentation(config(spec_aug=True), unsupported="skip").available()


@pytest.mark.parametrize("seed", GOLDEN["seeds"])
def test_seeded_draws_equal_the_references(seed):
    random.seed(seed)
    np.random.seed(seed)
    rir = Augmentation(config(rir=True)).augmentations[0]
    for want in GOLDEN["rir"][str(seed)]:
        assert rir.draw(8) == want
    random.seed(seed)
    np.random.seed(seed)
    noise = Augmentation(config(noise=True), noise_bank=bank()).augmentations[0]
    assert noise.SNR == GOLDEN["snr"]
    for n, want in zip(GOLDEN["lengths"], GOLDEN["noise"][str(seed)]):
        got = noise.draw(n)
        assert {k: got[k] for k in want} == want and got["segment"].shape == (n,)
    # process(): random.sample picks the augmentation, as in Augmentation.process, then the augmentation draws
    both = Augmentation(config(rir=True, noise=True), noise_bank=bank())
    random.seed(seed)
    np.random.seed(seed)
    picked = random.sample(both.augmentations, 1)[0]
    want = picked.draw(50)
    random.seed(seed)
    np.random.seed(seed)
    aug, got = both.draw(50)
    assert aug is picked and {k: v for k, v in got.items() if k != "segment"} == {k: v for k, v in want.items() if k != "segment"}


def test_noise_segments_follow_the_references_rule():
    rec = np.arange(100, dtype=np.float32)
    highs = []
    seg = cut_noise(rec, 85, lambda high: highs.append(high) or 7)
    assert highs == [200 - 85 - 10] and np.array_equal(seg, np.tile(rec, 2)[7:92])    # 85 + 20 > 100: doubled once
    seg = cut_noise(rec, 80, lambda high: highs.append(high) or 9)
    assert highs[-1] == 100 - 80 - 10 and np.array_equal(seg, rec[9:89])


def test_oracle_convolution_is_scipys():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    for n, k in ((1, 1), (17, 5), (300, 4096), (5000, 33)):
        x, h = rng.standard_normal(n), rng.standard_normal(k)
        y, bound = ar.fir_full(x, h)
        want = signal.convolve(x, h, mode="full")
        assert y.shape == want.shape == (n + k - 1,) and np.allclose(y, want, rtol=0, atol=1e-12 * bound.max())
        assert (bound >= np.abs(y) - 1e-12).all()
    assert ar.fir_full(np.zeros(0), np.ones(3))[0].shape == (0,)


def test_oracle_generator_direct_path_and_refusals():
    room, s, r, c, fs, ns = (5.0, 4.0, 6.0), (1.0, 1.0, 1.0), (2.5, 2.0, 3.0), 340.0, 16000.0, 1024
    h, A = ar.rir(room, s, r, c, fs, ns, beta=[0.0] * 6)
    d = float(np.linalg.norm(np.subtract(s, r)))
    at = d * fs / c
    Tw = ar.window_taps(fs)
    assert Tw == 128
    peak = int(np.argmax(np.abs(h)))
    assert abs(peak - at) <= 1 and abs(h[peak] - 0.5 / (4 * np.pi * d)) < 0.05 * 0.5 / (4 * np.pi * d)   # Fc = 0.5 scales the sinc
    assert not h[:int(at) - Tw // 2].any() and not h[int(at) + Tw // 2 + 1:].any()
    assert np.array_equal(A > 0, np.abs(np.arange(ns) - (np.floor(at) + 0.5)) <= Tw // 2)
    # with reflections the direct path is still there, and the filter removes the mean
    h2, _ = ar.rir(room, s, r, c, fs, ns, reverberation_time=0.4)
    assert abs(h2[peak] - h[peak]) < 1e-3 and np.abs(h2[int(at) + Tw:]).max() > 0
    h3, _ = ar.rir(room, s, r, c, fs, 4096, reverberation_time=0.4, hp_filter=True)
    assert abs(h3.sum()) < 0.1 * np.abs(h3).sum()
    assert ar.highpass_abs_gain(4096, fs) < 3
    # refused by the Python layer, before any library call
    with pytest.raises(ValueError, match="alpha"):
        ImageSourceRIR(16000, room=(5, 4, 6), reverberation_time=0.05)
    with pytest.raises(ValueError, match="alpha"):
        ar.reflection_coefficients((5, 4, 6), 340.0, 0.05)
    gen = ImageSourceRIR(16000)
    assert gen.hp_filter and gen.nsample == 4096 and gen.room == (5.0, 4.0, 6.0) and gen.c == 340.0
    assert np.allclose(gen.beta, ar.reflection_coefficients((5, 4, 6), 340.0, 0.4), rtol=1e-15)
    with pytest.raises(ValueError, match="at the receiver"):
        gen.params([(1, 1, 1), (2, 2, 2)], [(1, 2, 1), (2, 2, 2)])
    with pytest.raises(ValueError, match="outside the room"):
        gen.params([(1, 4.1, 1)], [(1, 2, 1)])
    with pytest.raises(ValueError, match="outside the room"):
        gen.params([(1, 1, 1)], [(-0.1, 2, 1)])
    with pytest.raises(ValueError, match="nsample"):
        ImageSourceRIR(16000, nsample=16385)
    t = gen.params([(1, 1, 1)], [(1, 2, 1)])
    assert t.shape == (1, 20) and list(t[0, :12]) == [5, 4, 6, 1, 1, 1, 1, 2, 1, 340, 16000, 0.4] and list(t[0, 18:]) == [1, 4096]


def test_oracle_mixing_and_quantisation():
    rng = np.random.default_rng(1)
    x, d = rng.standard_normal(1000), rng.standard_normal(1200)
    y, g = ar.mix_snr(x, d, 5.0)
    noise = y - x
    assert abs(10 * np.log10(np.sum(x * x) / np.sum(noise * noise)) - 5.0) < 1e-9
    assert ar.mix_snr(x, np.zeros(1000), 5.0)[1] == 0.0 and ar.mix_snr(np.zeros(10), d, 5.0)[1] == 0.0
    q = ar.quantise(np.array([1.5, -1.5, 0.99999, -0.99999, 3.0e-5, -3.0e-5, 0.25], np.float32))
    assert list(q * 32768) == [32768, -32768, 32767, -32767, 0, 0, 8192]
