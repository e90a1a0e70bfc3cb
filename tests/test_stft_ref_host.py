"""The host side of the STFT pair, spec_aug and the time stretch (tensorflowasr_amd/stft.py, augment.py): the float64 oracle of
stft_ref.py against its own identities, the ABI table, the seeded draws against the reference's expressions written out, and
Augmentation's `enable`.  No GPU."""
import os
import random
import re

import numpy as np
import pytest

import stft_ref as sr
from tensorflowasr_amd import _lib, build
from tensorflowasr_amd.augment import DEVICE_KEYS, KEYS, UNSUPPORTED, Augmentation, SpecAug, Speed
from tensorflowasr_amd.stft import SIZES, STFT, frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355asr_stft_frames", "mi355asr_stft_ragged", "mi355asr_istft_workspace_bytes", "mi355asr_istft_ragged",
       "mi355asr_spec_aug_workspace_bytes", "mi355asr_spec_aug", "mi355asr_phase_vocoder_workspace_bytes", "mi355asr_phase_vocoder"]


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
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "stft.hip")).read()
    assert "stft.hip" in build.SOURCES
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert SIZES == sr.SIZES
    for n_fft, win, hop in SIZES:
        assert "n_fft == %d && win == %d && hop == %d" % (n_fft, win, hop) in src


@pytest.mark.parametrize("n_fft,win,hop", sr.SIZES)
def test_the_oracle_inverts_itself(n_fft, win, hop):
    rng = np.random.default_rng(n_fft)
    for n in (n_fft // 2 + 1, n_fft, 5 * n_fft + 123):
        x = rng.standard_normal(n)
        S = sr.stft(x, n_fft, win, hop)
        F = sr.n_frames(n, n_fft, hop)
        assert S.shape == (F, n_fft // 2 + 1) and F == 1 + n // hop == frames_of(n, n_fft, hop)
        y = sr.istft(S, n_fft, win, hop)
        assert len(y) == hop * (F - 1) and np.abs(y - x[:hop * (F - 1)]).max() <= 1e-12          # measured 3e-16
        # length=: cut, and zero-filled beyond what the frames reach
        assert np.array_equal(sr.istft(S, n_fft, win, hop, length=len(y) - 7), y[:-7])
        z = sr.istft(S, n_fft, win, hop, length=len(y) + 2 * n_fft)
        assert np.array_equal(z[:len(y)], y) and not z[hop * (F - 1) + n_fft // 2:].any()
    assert sr.n_frames(n_fft // 2, n_fft, hop) == 0 == frames_of(n_fft // 2, n_fft, hop) == frames_of(0, n_fft, hop)
    assert sr.stft(np.zeros(n_fft // 2), n_fft, win, hop).shape == (0, n_fft // 2 + 1)
    # the error scales bound what they say they bound
    x = rng.standard_normal(3 * n_fft)
    a = sr.frame_l1(x, n_fft, win, hop)
    assert (np.abs(sr.stft(x, n_fft, win, hop)) <= a[:, None] * (1 + 1e-12)).all()
    assert (np.abs(sr.istft(sr.stft(x, n_fft, win, hop), n_fft, win, hop)) <= sr.ola_scale(a, n_fft, win, hop) * (1 + 1e-9)).all()


def test_the_oracle_window_is_librosas():
    w = sr.window(1024, 800)
    assert len(w) == 1024 and not w[:112].any() and not w[912:].any() and w[112] == 0 and abs(w[512] - 1) < 1e-15
    assert np.allclose(w[112:912], 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(800) / 800), rtol=0, atol=0)
    signal = pytest.importorskip("scipy.signal")
    assert np.allclose(w[112:912], signal.get_window("hann", 800, fftbins=True), rtol=0, atol=1e-15)


def test_time_stretch_at_rate_one_is_the_identity():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(9000)
    y = sr.time_stretch(x, 1.0)
    assert len(y) == 9000 and np.abs(y[:8704] - x[:8704]).max() <= 1e-10                        # measured 7e-12
    for rate in (0.5, 0.9, 1.2, 2.0):
        assert len(sr.time_stretch(x, rate)) == int(round(9000 / rate))
        assert sr.stretch_frames(18, rate) == len(np.arange(0, 18, rate))
    # the vocoder leaves the magnitudes of the frames it lands on exactly
    D = sr.stft(x, 2048, 2048, 512)
    assert np.allclose(np.abs(sr.phase_vocoder(D, 2.0, 512, 2048)), np.abs(D[::2]), rtol=1e-12, atol=0)


def test_spec_aug_oracle_zeroes_the_references_blocks():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(4000)
    S = sr.stft(x, 1024, 800, 160)
    F = len(S)
    ref = S.T.copy()                                            # librosa's layout and the reference's own statement
    for h_, w_ in ((0, 0), (512, F - 1), (100, 7)):
        ref[max(h_ - 10, 0):h_ + 10, max(w_ - 10, 0):w_ + 10] *= 0.0
    got = sr.mask(S, [(0, 0), (512, F - 1), (100, 7)], 10)
    assert np.array_equal(got, ref.T) and (got == 0).sum() == 10 * 10 + 11 * 11 + 20 * 17
    assert np.array_equal(sr.mask(S, [(5, 5)], 0), S) and np.array_equal(sr.mask(S, [], 10), S)
    short = rng.standard_normal(512)
    assert np.array_equal(sr.spec_aug(short, [(1, 1)], 10), short)
    assert len(sr.spec_aug(x, [(100, 7)], 10)) == 160 * (F - 1) == 4000


@pytest.mark.parametrize("seed", [0, 7])
def test_seeded_draws_equal_the_references_expressions(seed):
    aug = SpecAug(window=10, ratio=0.5)
    random.seed(seed)
    got = aug.draw(101)
    random.seed(seed)
    nums = int(101 * 0.5)
    ws = random.sample(list(range(101)), nums)
    hs = random.sample(list(range(513)), nums)
    assert got.shape == (50, 2) and got.dtype == np.int32 and got.tolist() == [[h, w] for h, w in zip(hs, ws)]
    assert SpecAug(ratio=0).draw(101).shape == (0, 2)
    sp = Speed("(0.5,2)")
    np.random.seed(seed)
    rates = [sp.draw()["rate"] for _ in range(20)]
    np.random.seed(seed)
    want = [float(np.clip(np.random.random() * 2, 0.5, 2)) for _ in range(20)]
    assert rates == want and min(rates) == 0.5
    assert Speed((0.9, 1.2)).factor == (0.9, 1.2) == Speed("(0.9,1.2)").factor


def test_augmentation_enable():
    assert DEVICE_KEYS == ("spec_aug", "speed") and set(DEVICE_KEYS) <= set(UNSUPPORTED) <= set(KEYS)
    # the default is what it was
    with pytest.raises(NotImplementedError, match="spec_aug"):
        Augmentation(config(spec_aug=True))
    a = Augmentation(config(spec_aug=True), unsupported="skip")
    assert not a.available() and a.skipped == ["spec_aug"]
    # the reference's shipped configuration, spec_aug alone, is available
    a = Augmentation(config(spec_aug=True), enable=("spec_aug",))
    assert a.available() and [g.key for g in a.augmentations] == ["spec_aug"] and a.skipped == []
    assert a.augmentations[0].window == 10 and a.augmentations[0].ratio == 0.5
    a = Augmentation(config(spec_aug=True, speed=True), enable=("spec_aug", "speed"))
    assert [g.key for g in a.augmentations] == ["speed", "spec_aug"] and a.augmentations[0].factor == (0.9, 1.2)
    with pytest.raises(NotImplementedError, match="speed"):
        Augmentation(config(spec_aug=True, speed=True), enable=("spec_aug",))
    with pytest.raises(NotImplementedError, match="pitch"):
        Augmentation(config(pitch=True), enable=("spec_aug", "speed"))
    with pytest.raises(ValueError, match="pitch"):
        Augmentation(config(), enable=("pitch",))
    # the draws of process(): random.sample picks the augmentation, then it draws
    a = Augmentation(config(spec_aug=True), enable="spec_aug")
    random.seed(5)
    aug, d = a.draw(16000)
    random.seed(5)
    picked = random.sample(a.augmentations, 1)[0]
    ws = random.sample(list(range(101)), 50)
    hs = random.sample(list(range(513)), 50)
    assert aug is picked and d["centres"].tolist() == [[h, w] for h, w in zip(hs, ws)]
    assert a.draw(512)[1]["centres"].shape == (0, 2)           # no frame, nothing drawn


def test_value_errors_fire_before_any_launch():
    # from 164 320 samples int(frames * 0.5) exceeds the 513 bins: the reference's random.sample raises ValueError
    assert int((1 + 164319 // 160) * 0.5) == 513 and int((1 + 164320 // 160) * 0.5) == 514
    a = Augmentation(config(spec_aug=True), enable=("spec_aug",))
    assert len(a.augmentations[0].draw(164319)["centres"]) == 513
    with pytest.raises(ValueError, match="164320"):
        a.augmentations[0].draw(164320)
    with pytest.raises(ValueError):
        SpecAug().draw(1028)
    with pytest.raises(ValueError, match="negative"):
        SpecAug(window=-1)
    for bad in ((1000, 800, 160), (1024, 1024, 256), (2048, 2048, 160), (512, None, None)):
        with pytest.raises(ValueError, match="not one of"):
            STFT(*bad)
    st = STFT(2048)
    assert (st.n_fft, st.win_length, st.hop_length, st.bins) == (2048, 2048, 512, 1025)
    with pytest.raises(ValueError, match="factor"):
        Speed("(0,2)")
