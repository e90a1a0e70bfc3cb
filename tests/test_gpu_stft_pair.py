"""The ragged STFT / ISTFT pair (csrc/stft.hip, tensorflowasr_amd/stft.py) on the MI355X against the float64 restatement of
stft_ref.py, at (1024, 800, 160) and (2048, 2048, 512): the forward transform bin by bin, the inverse and the round trip sample
by sample, the frame counts and lengths exactly, zeros past them, int16 input, poisoned padding, repeatability and row
independence bit for bit, and the refusal of every other size."""
import ctypes

import numpy as np
import pytest

import stft_ref as sr
from stft_cases import GEO, LENS, OLA_TILE, U24, bits, device, pair_case, signal, worst_ratio

pytestmark = pytest.mark.gpu

# |dS[f, k]| <= C_F 2^-24 a_f and |dy[n]| <= C_Y 2^-24 A[n] (stft_ref.frame_l1, stft_ref.ola_scale), measured against the float64
# oracle: four times the worst ratio of the first run on the MI355X, rounded up to a power of two.
# Measured: forward 0.9608 (1024) and 1.0398 (2048); round trip 0.0464 and 0.0262, the inverse alone 0.0354 and 0.0290, spec_aug
# 0.0464 at the worst.  Caps that hold whatever is measured: 512.
C_F = 8.0
C_Y = 0.25
SIZES = sorted(GEO)


@pytest.mark.parametrize("n_fft", SIZES)
def test_forward_parity_frames_and_zeros(n_fft):
    c = pair_case(n_fft)
    n_fft, win, hop = c["geo"]
    S = c["S"]
    assert S.dtype == np.complex64 and S.shape == (len(c["lens"]), 1 + max(c["lens"]) // hop, n_fft // 2 + 1)
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        F = sr.n_frames(n, n_fft, hop)
        assert c["frames"][b] == F == len(c["ref"][b]), (b, n)
        assert not S[b, F:].any(), (b, n)
        if F:
            worst = max(worst, worst_ratio(np.abs(S[b, :F] - c["ref"][b]), U24 * c["a"][b][:, None] * np.ones((1, S.shape[2]))))
            assert not S[b, :F, 0].imag.any() and not S[b, :F, -1].imag.any()
    print("stft %d forward: worst ratio %.4f" % (n_fft, worst))
    assert worst <= C_F <= 512


@pytest.mark.parametrize("n_fft", SIZES)
def test_round_trip_parity_lengths_and_zeros(n_fft):
    c = pair_case(n_fft)
    n_fft, win, hop = c["geo"]
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        F = sr.n_frames(n, n_fft, hop)
        want_len = hop * (F - 1) if F else 0
        assert c["out_len"][b] == want_len, (b, n)
        assert not c["y"][b, want_len:].any(), (b, n)
        if F:
            want = sr.istft(c["ref"][b], n_fft, win, hop)
            assert np.abs(want - c["x"][b, :want_len]).max() <= 1e-12
            worst = max(worst, worst_ratio(np.abs(c["y"][b, :want_len] - want), U24 * sr.ola_scale(c["a"][b], n_fft, win, hop)))
    print("stft %d round trip: worst ratio %.4f" % (n_fft, worst))
    assert worst <= C_Y <= 512


@pytest.mark.parametrize("n_fft", SIZES)
def test_inverse_of_an_uploaded_spectrum_and_out_lengths(n_fft):
    """the inverse alone, on the oracle's spectrum rounded to complex64, with lengths shorter and longer than the frames reach
    and one sample before, at and after a tile of the overlap-add kernel"""
    device()
    from tensorflowasr_amd.stft import STFT
    n_fft, win, hop = GEO[n_fft]
    rng = np.random.default_rng(n_fft + 1)
    frames = [9, 0, 1, 4, 9, 9, 9, 9]
    natural = hop * 8
    outs = [natural, 300, 700, OLA_TILE - 1, OLA_TILE, OLA_TILE + 1, natural - 77, natural + n_fft]
    x = signal(rng, (len(frames), natural + 10))
    S = np.zeros((len(frames), 9, n_fft // 2 + 1), np.complex64)
    for b, F in enumerate(frames):
        S[b, :F] = sr.stft(x[b], n_fft, win, hop)[:F]
    S[:, :, 0] += 1j                                    # the imaginary parts of bins 0 and n_fft / 2 are ignored, as by irfft
    S[:, :, -1] -= 2j
    st = STFT(n_fft, win, hop)
    y, out_len = st.inverse(S, frames, out_lengths=outs)
    y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
    assert list(out_len) == outs and y.shape == (len(frames), max(outs))
    worst = 0.0
    for b, F in enumerate(frames):
        assert not y[b, outs[b]:].any(), b
        Sb = S[b, :F].astype(np.complex128)
        want = sr.istft(Sb, n_fft, win, hop, length=outs[b])
        scale = sr.ola_scale(sr.frame_l1(x[b], n_fft, win, hop)[:F], n_fft, win, hop, length=outs[b])
        worst = max(worst, worst_ratio(np.abs(y[b, :outs[b]] - want), U24 * scale))
    print("stft %d inverse alone: worst ratio %.4f" % (n_fft, worst))
    assert worst <= C_Y
    # the default length, and a narrower output buffer
    y2, l2 = st.inverse(S, frames)
    assert list(l2.cpu().numpy()) == [hop * (F - 1) if F else 0 for F in frames]
    assert np.array_equal(y2.cpu().numpy()[0], y[0, :natural])
    y3, l3 = st.inverse(S, frames, out_lengths=outs, out_pad=500)
    assert list(l3.cpu().numpy()) == [min(o, 500) for o in outs] and np.array_equal(y3.cpu().numpy(), y[:, :500])


@pytest.mark.parametrize("n_fft", SIZES)
def test_int16_input_and_poisoned_padding(n_fft):
    device()
    from tensorflowasr_amd.stft import STFT
    geo = GEO[n_fft]
    lens = LENS[n_fft]
    pcm = np.random.default_rng(n_fft + 2).integers(-32768, 32768, (len(lens), max(lens))).astype(np.int16)
    pcm[:, :4] = (-32768, 32767, 0, -1)
    st = STFT(*geo)
    Si, fi = st.forward(pcm, lens)
    Sf, ff = st.forward(pcm.astype(np.float32) / 32768, lens)
    assert np.array_equal(fi.cpu().numpy(), ff.cpu().numpy())
    assert np.array_equal(bits(Si.cpu().numpy()), bits(Sf.cpu().numpy())) and float(Si.abs().max()) > 1
    c = pair_case(n_fft)
    xp = np.full((len(lens), max(lens) + 13), np.nan, np.float32)
    for b, n in enumerate(lens):
        xp[b, :n] = c["x"][b, :n]
    Sp, fp = st.forward(xp, lens)
    Sp = Sp.cpu().numpy()
    assert np.isfinite(Sp.view(np.float32)).all() and np.array_equal(fp.cpu().numpy(), c["frames"])
    assert np.array_equal(bits(Sp[:, :c["S"].shape[1]]), bits(c["S"])) and not Sp[:, c["S"].shape[1]:].any()


@pytest.mark.parametrize("n_fft", SIZES)
def test_rows_are_independent_and_runs_repeat(n_fft):
    device()
    from tensorflowasr_amd.stft import STFT
    c = pair_case(n_fft)
    n_fft, win, hop = c["geo"]
    st = STFT(n_fft, win, hop)
    S, frames = st.forward(c["x"], c["lens"])
    y, out_len = st.inverse(S, frames)
    assert np.array_equal(bits(S.cpu().numpy()), bits(c["S"])) and np.array_equal(bits(y.cpu().numpy()), bits(c["y"]))
    for b, n in enumerate(c["lens"]):
        S1, f1 = st.forward(c["x"][b, :n], None)
        F = int(f1[0])
        assert F == c["frames"][b] and np.array_equal(bits(S1.cpu().numpy()[0, :F]), bits(c["S"][b, :F])), (b, n)
        y1, l1 = st.inverse(S1, f1)
        assert int(l1[0]) == c["out_len"][b] and np.array_equal(bits(y1.cpu().numpy()[0, :int(l1[0])]), bits(c["y"][b, :int(l1[0])])), (b, n)


def test_other_sizes_are_refused():
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    x = torch.zeros((1, 4096), dtype=torch.float32, device="cuda:0")
    ln = torch.tensor([4096], dtype=torch.int32, device="cuda:0")
    S = torch.full((1, 40, 1025), 7.0, dtype=torch.complex64, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for geo in ((1024, 1024, 256), (2048, 2048, 160), (512, 512, 128), (1024, 800, 0), (1000, 800, 160)):
        assert lib.mi355asr_stft_ragged(p(x), 0, p(ln), 1, 4096, *geo, p(S), 40, None, None) == -1, geo
        assert b"neither" in lib.mi355asr_last_error()
        wb = ctypes.c_size_t()
        assert lib.mi355asr_istft_workspace_bytes(1, 40, *geo, ctypes.byref(wb)) == -1
        n = ctypes.c_int32()
        assert lib.mi355asr_stft_frames(*geo, 4096, ctypes.byref(n)) == -1
    assert lib.mi355asr_stft_ragged(p(x), 1, p(ln), 1, 4096, 1024, 800, 160, p(S), 40, None, None) == -1      # bf16 input
    torch.cuda.synchronize()
    assert bool((S == 7.0).all())                                                                             # nothing was launched
    n = ctypes.c_int32()
    for geo in GEO.values():
        for samples in (0, geo[0] // 2, geo[0] // 2 + 1, 5000):
            assert lib.mi355asr_stft_frames(*geo, samples, ctypes.byref(n)) == 0 and n.value == sr.n_frames(samples, geo[0], geo[2])
