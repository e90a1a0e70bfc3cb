"""The STFT's two sample-load paths (csrc/fft_stft.hip) against the float64 oracle.

A frame whose 1024 samples all lie inside the utterance ("interior": base >= 0 and base + 1024 <= L with base = f * hop - the
left SAME padding) loads its samples without bounds work; every other frame pads with zeros, sample by sample.  The lengths
here put the boundary between the two everywhere it can sit: no interior frame at all, exactly one (and one sample either side
of that length), a short utterance with edges on both sides, and a ragged batch long enough (more than the kernel's 3072 waves
in frames) that one wave takes an edge frame of one utterance and an interior frame of another."""
import numpy as np
import pytest

from helpers import co, encoder_kwargs, maxdiff, small_cfg, waves

TOL = 1e-3                      # the project's contract against the float64 oracle
HOP, NDFT = 160, 1024
STFT_WAVES = 3072               # fft_stft.hip: launch_fft_stft starts at most this many waves, each looping over frames


def interior_frames(L):
    """the frames of an utterance of L samples that take the unchecked loads"""
    F, before, _ = co.same_pad(L, NDFT, HOP)
    return [f for f in range(F) if f * HOP - before >= 0 and f * HOP - before + NDFT <= L]


def one_interior_length():
    return next(L for L in range(NDFT, 4 * NDFT) if len(interior_frames(L)) == 1)


def test_lengths_sit_where_the_docstring_says():
    L1 = one_interior_length()
    assert interior_frames(800) == [] and len(interior_frames(L1)) == 1 and interior_frames(L1 - 1) == []
    assert len(interior_frames(L1 + 1)) >= 1
    F = co.same_pad(4000, NDFT, HOP)[0]
    n = len(interior_frames(4000))
    assert 0 < n < F and 0 not in interior_frames(4000) and F - 1 not in interior_frames(4000)
    lens, L = RAGGED_LENS, max(RAGGED_LENS)
    Fm = co.same_pad(L, NDFT, HOP)[0]
    assert len(lens) * Fm > STFT_WAVES
    # wave w takes the frames w, w + 3072, ... of the [B, Fm] grid: some wave must hold an interior and a checked frame
    kind = {}
    for b, Lb in enumerate(lens):
        inner = set(interior_frames(Lb))
        for f in range(Fm):
            kind.setdefault((b * Fm + f) % STFT_WAVES, set()).add(f in inner)
    assert sum(len(v) == 2 for v in kind.values()) >= 4


RAGGED_LENS = [132000, 1500, 800, 131999]


@pytest.fixture(scope="module")
def encoder():
    import torch
    from tensorflowasr_amd.models import ConformerEncoder
    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg = small_cfg(1)
    w = co.encoder_weights(cfg, seed=3)
    e = ConformerEncoder(**encoder_kwargs(cfg))
    e.load_weights(w, by_name=False)
    return e, w, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["800", "one-1", "one", "one+1", "4000"])
def test_melspectrogram_edge_and_interior_frames_vs_oracle(encoder, which):
    e, w, _ = encoder
    L1 = one_interior_length()
    L = {"800": 800, "one-1": L1 - 1, "one": L1, "one+1": L1 + 1, "4000": 4000}[which]
    x = waves(3, L, 7)
    got = e.melspectrogram(x).cpu().numpy()
    ref = co.melspectrogram(x.astype(np.float64), w, hop=HOP)
    assert got.shape == ref.shape
    err = maxdiff(got, ref)
    print("melspectrogram L=%d interior=%d of %d frames: max|d| = %.3e" % (L, len(interior_frames(L)), ref.shape[1], err))
    assert err < TOL, (L, err)


@pytest.mark.gpu
def test_ragged_batch_mixes_both_paths_in_one_wave_vs_oracle(encoder):
    """The library has no ragged melspectrogram call, so the ragged frames are checked where they come out: the ragged encoder
    (one block), every row against the oracle run on that utterance alone."""
    e, w, cfg = encoder
    lens = np.array(RAGGED_LENS, np.int32)
    x = waves(len(lens), int(lens.max()), 21)
    for b, Lb in enumerate(lens):
        x[b, Lb:] = np.nan                              # samples past a row's length are never used
    enc, enc_len = e(x, lengths=lens)
    enc, enc_len = enc.cpu().numpy(), enc_len.cpu().numpy()
    for b, Lb in enumerate(lens):
        ref = co.conformer_encoder(x[b:b + 1, :Lb].astype(np.float64), w, cfg)[0]
        assert enc_len[b] == ref.shape[0]
        err = maxdiff(enc[b, :ref.shape[0]], ref)
        print("ragged row %d (%d samples, %d interior frames): max|d| = %.3e" % (b, Lb, len(interior_frames(int(Lb))), err))
        assert err < TOL, (b, err)
        assert not enc[b, ref.shape[0]:].any()
