"""Ragged batches on the host (no GPU): the per-utterance geometry the kernels derive from wav_len, and a NumPy restatement of
the masked encoder (tests/ragged_numpy.py) against per-utterance runs of the float64 oracle."""
import numpy as np

from helpers import co, small_cfg, waves
from ragged_numpy import masked_encoder
from tensorflowasr_amd.models import ragged_geometry


def test_geometry_matches_the_oracle_on_unpadded_waves():
    """F_b, pad_left_b, T1_b, the conv pads and T_b for every length 1 .. 3 200 (every residue mod hop, twenty times over)"""
    for L in range(1, 3201):
        g = ragged_geometry(L)
        F, lo, _ = co.same_pad(L, 1024, 160)
        x = np.zeros((1, L))
        assert co.frame_signal(x, 1024, 160).shape[1] == F == g["F"] and lo == g["pad_left"]
        T1, pt1, _ = co.same_pad(F, 3, 2)
        T, pt2, _ = co.same_pad(T1, 3, 2)
        assert (g["T1"], g["pt1"], g["T"], g["pt2"]) == (T1, pt1, T, pt2)
        # TF SAME with k = 3, s = 2: one zero row on top for an odd input, none for an even one
        assert g["pt1"] == F % 2 and g["pt2"] == T1 % 2
        assert -(-(-(-F // 2)) // 2) == g["T"]


def test_geometry_of_a_longer_sweep():
    for L in list(range(9000, 12000, 7)) + [67263, 69456, 160000, 320000]:
        g = ragged_geometry(L)
        mel = co.frame_signal(np.zeros((1, L)), 1024, 160)
        assert mel.shape[1] == g["F"]
        sub = co.conv2d_same(np.zeros((1, g["F"], 80, 1)), np.zeros((3, 3, 1, 1)), np.zeros(1), (2, 2))
        assert sub.shape[1] == g["T1"]
        assert co.conv2d_same(sub, np.zeros((3, 3, 1, 1)), np.zeros(1), (2, 2)).shape[1] == g["T"]


def _case():
    cfg = small_cfg(1)
    w = co.encoder_weights(cfg, seed=3)
    # lengths: L mod 160 in {0, 1, 159}, odd and even F_b and T1_b, one utterance of exactly L
    lens = np.array([5120, 4961, 5279, 3199, 5601])
    L = int(lens.max())
    x = waves(len(lens), L, 40).astype(np.float64)
    for b, n in enumerate(lens):
        x[b, n:] = 0.25 * np.sin(np.arange(L - n))             # non-zero padding: it must not leak into any row
    return cfg, w, lens, x


def test_masked_encoder_equals_per_utterance_oracle():
    cfg, w, lens, x = _case()
    g = [ragged_geometry(int(n)) for n in lens]
    assert {gi["F"] % 2 for gi in g} == {0, 1} and {gi["T1"] % 2 for gi in g} == {0, 1}
    assert {int(n) % 160 for n in lens} >= {0, 1, 159}
    cfg0 = dict(cfg, num_blocks=0)
    sub, Tb = masked_encoder(x, lens, w, cfg0)
    for b, n in enumerate(lens):                               # frontend + subsampling: every rule exact
        solo = co.conformer_encoder(x[b:b + 1, :n], w, cfg0)[0]
        assert np.abs(sub[b, :Tb[b]] - solo).max() <= 1e-12 * np.abs(solo).max()
    enc, Tb = masked_encoder(x, lens, w, cfg)
    assert Tb.tolist() == [gi["T"] for gi in g]
    for b, n in enumerate(lens):
        solo = co.conformer_encoder(x[b:b + 1, :n], w, cfg)[0]
        assert solo.shape[0] == Tb[b]
        # float64 agreement up to summation order: NumPy's contractions over T keys group their partial sums by T, so a
        # ragged row and the solo run round differently (measured: below 1e-9 relative after a block; the masks themselves
        # are exact -- frontend and subsampling agree to the last bit)
        err = np.abs(enc[b, :Tb[b]] - solo).max() / max(1.0, np.abs(solo).max())
        assert err < 1e-8, (b, err)
        assert not enc[b, Tb[b]:].any()


def test_masks_are_necessary():
    """the oracle on the zero-padded batch is NOT what the utterances give alone: every rule above matters"""
    cfg, w, lens, x = _case()
    xz = x.copy()
    for b, n in enumerate(lens):
        xz[b, n:] = 0.0
    padded = co.conformer_encoder(xz, w, cfg)
    enc, Tb = masked_encoder(xz, lens, w, cfg)
    for b, n in enumerate(lens):
        if n == x.shape[1]:
            continue
        assert np.abs(padded[b, :Tb[b]] - enc[b, :Tb[b]]).max() > 1e-3, b
