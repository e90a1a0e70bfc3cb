"""The far-field kernels (csrc/augment.hip, tensorflowasr_amd/augment.py) on the MI355X against the float64 restatements of
augment_ref.py: the ragged FIR under its derived bound, row by row and bit for bit; the image-source generator against the oracle,
its reproducibility and its tolerance; SNR mixing and the 16-bit quantisation; the FarField chain and the offline_stt_batch hook."""
import ctypes
import functools

import numpy as np
import pytest

import augment_ref as ar

pytestmark = pytest.mark.gpu

TILE = 4096                                             # outputs per workgroup of the FIR kernel
FIR_K = [1, 15, 16, 17, 4096, 16384]
# the generator's shapes: (room, c, fs, nsample, T60); sources and receivers per shape below
SMALL = ((3.0, 2.0, 2.5), 340.0, 8000.0, 256, 0.2)
ODD = ((3.0, 2.0, 2.5), 340.0, 8000.0, 251, 0.2)        # nsample not a multiple of 16
DEFAULT = ((5.0, 4.0, 6.0), 340.0, 16000.0, 4096, 0.4)  # SignalRIR's
# C of |dh[n]| <= C 2^-24 A[n]: four times the worst ratio measured on these shapes at the first run on the MI355X (0.2966, the
# small room with the filter off), rounded up to a power of two
RIR_C = 2.0


def device():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def fir_lengths(K):
    base = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3000]
    return base + [n for n in (TILE - K, TILE - K + 1, TILE - K + 2) if n > 0 and n not in base]   # outputs: one tile -1, +0, +1


@functools.lru_cache(maxsize=None)
def fir_case(K):
    """one ragged batch with a filter per row: inputs, the float64 reference and its bound term, what the device returned"""
    device()
    from tensorflowasr_amd.augment import Reverb
    lens = fir_lengths(K)
    rng = np.random.default_rng(1000 + K)
    x = rng.standard_normal((len(lens), max(lens))).astype(np.float32)
    h = (rng.standard_normal((len(lens), K)) * np.exp(-np.arange(K) / (0.3 * K + 1))).astype(np.float32)
    ref = [ar.fir_full(x[b, :n], h[b]) for b, n in enumerate(lens)]
    y, out_len = Reverb()(x, lens, h)
    return lens, x, h, ref, y.cpu().numpy(), out_len.cpu().numpy()


def check_fir(y, out_len, lens, ref, K, what):
    worst = 0.0
    for b, n in enumerate(lens):
        want = n + K - 1 if n else 0
        assert out_len[b] == want == len(ref[b][0]), (what, b)
        assert not y[b, want:].any(), (what, b)
        if n:
            tol = (K + 2) * 2.0 ** -23 * ref[b][1]
            err = np.abs(y[b, :want].astype(np.float64) - ref[b][0])
            assert (err <= tol).all(), (what, b, n, float((err / np.maximum(tol, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("fir %s K=%d: largest error %.4f of its bound" % (what, K, worst))


@pytest.mark.parametrize("K", FIR_K)
def test_fir_parity_per_row_filters(K):
    lens, x, h, ref, y, out_len = fir_case(K)
    assert y.dtype == np.float32 and y.shape == (len(lens), max(lens) + K - 1)
    check_fir(y, out_len, lens, ref, K, "per-row")


@pytest.mark.parametrize("K", FIR_K)
def test_fir_shared_filter_and_int16_input(K):
    from tensorflowasr_amd.augment import Reverb
    lens, x, h, _, _, _ = fir_case(K)
    ref = [ar.fir_full(x[b, :n], h[2]) for b, n in enumerate(lens)]
    y, out_len = Reverb()(x, lens, h[2])
    check_fir(y.cpu().numpy(), out_len.cpu().numpy(), lens, ref, K, "shared")
    pcm = np.random.default_rng(K).integers(-32768, 32768, x.shape).astype(np.int16)
    pcm[:, :4] = (-32768, 32767, 0, -1)
    yi, li = Reverb()(pcm, lens, h)
    yf, lf = Reverb()(pcm.astype(np.float32) / 32768, lens, h)
    assert np.array_equal(li.cpu().numpy(), lf.cpu().numpy())
    assert np.array_equal(yi.cpu().numpy(), yf.cpu().numpy()) and float(yi.abs().max()) > 0.01
    refi = [ar.fir_full(pcm[b, :n].astype(np.float64) / 32768, h[b]) for b, n in enumerate(lens)]
    check_fir(yi.cpu().numpy(), li.cpu().numpy(), lens, refi, K, "int16")
    # rows that do not start on a 16-byte boundary take the scalar loads: the same bits
    yo, _ = Reverb()(pcm[:, :max(lens) - 3].copy(), [min(n, max(lens) - 3) for n in lens], h)
    assert np.array_equal(yo.cpu().numpy()[8, :3000 + K - 1], yi.cpu().numpy()[8, :3000 + K - 1])


@pytest.mark.parametrize("K", FIR_K)
def test_fir_rows_are_independent_and_runs_repeat(K):
    from tensorflowasr_amd.augment import Reverb
    lens, x, h, _, y, out_len = fir_case(K)
    assert np.array_equal(Reverb()(x, lens, h)[0].cpu().numpy(), y)
    for b, n in enumerate(lens):
        alone, alone_len = Reverb()(x[b, :n], None, h[b])
        assert int(alone_len[0]) == out_len[b]
        assert np.array_equal(alone.cpu().numpy()[0, :out_len[b]], y[b, :out_len[b]]), b


@pytest.mark.parametrize("K", [17, 4096])
def test_fir_never_reads_past_a_length_or_past_k(K):
    from tensorflowasr_amd.augment import Reverb
    lens, x, h, _, y, out_len = fir_case(K)
    xp = x.copy()
    for b, n in enumerate(lens):
        xp[b, n:] = np.nan
    hp = np.full((len(lens), K + 5), np.nan, np.float32)
    hp[:, :K] = h
    y2, l2 = Reverb()(xp, lens, hp, taps=K, out_pad=y.shape[1] + 37)
    y2 = y2.cpu().numpy()
    assert np.isfinite(y2).all()
    assert np.array_equal(y2[:, :y.shape[1]], y) and not y2[:, y.shape[1]:].any()
    for b in range(len(lens)):
        assert not y2[b, out_len[b]:].any(), b


def test_fir_refuses_a_filter_above_16384_taps():
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    x = torch.zeros((1, 8), device="cuda:0")
    n = torch.full((1,), 8, dtype=torch.int32, device="cuda:0")
    h = torch.zeros((1, 16385), device="cuda:0")
    y = torch.full((1, 8 + 16384), 7.0, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mi355asr_fir_ragged(p(x), 0, p(n), 1, 8, p(h), 16385, 16385, 0, p(y), y.shape[1], None) == -1
    assert b"16384" in lib.mi355asr_last_error()
    assert lib.mi355asr_fir_ragged(p(x), 0, p(n), 1, 8, p(h), 0, 16385, 0, p(y), y.shape[1], None) == -1
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0                          # nothing was launched
    from tensorflowasr_amd.augment import Reverb
    with pytest.raises(ValueError, match="16385"):
        Reverb()(np.zeros(8, np.float32), None, np.zeros(16385, np.float32))


# ---- the generator -----------------------------------------------------------------------------------------------------------------
GEOMETRIES = {
    "small": (SMALL, [(1.1, 0.7, 1.3), (2.2, 1.5, 0.9)]),
    "odd": (ODD, [(0.4, 1.9, 2.4), (2.9, 0.1, 0.2)]),
    "default": (DEFAULT, [(1.2, 3.1, 4.4), (3.3, 0.4, 2.0)]),
}


@functools.lru_cache(maxsize=None)
def rir_case(name, hp):
    """(oracle h, A, device h) of one shape"""
    device()
    from tensorflowasr_amd.augment import ImageSourceRIR
    (room, c, fs, ns, T), (s, r) = GEOMETRIES[name]
    href, A = ar.rir(room, s, r, c, fs, ns, reverberation_time=T, hp_filter=hp)
    gen = ImageSourceRIR(fs, room=room, reverberation_time=T, nsample=ns, c=c, hp_filter=hp)
    return href, A, gen.generate([s], [r]).cpu().numpy()[0], fs, ns


@pytest.mark.parametrize("name,hp", [("small", False), ("small", True), ("odd", False), ("odd", True), ("default", False), ("default", True)])
def test_generator_against_the_oracle_within_its_tolerance(name, hp):
    """filter off: |dh[n]| <= C 2^-24 A[n], A[n] the sum of |gain| over the images whose window covers n (so a sample no image
    reaches is exactly 0); filter on: the same C against max A times the recurrence's absolute gain.  The measured ratios are printed."""
    href, A, h, fs, ns = rir_case(name, hp)
    assert h.shape == (ns,) and h.dtype == np.float32 and np.isfinite(h).all()
    err = np.abs(h.astype(np.float64) - href)
    if hp:
        scale = np.full(ns, A.max() * ar.highpass_abs_gain(ns, fs))
    else:
        scale = A
        assert not h[A == 0].any()
    ratio = float((err[scale > 0] / (2.0 ** -24 * scale[scale > 0])).max())
    print("rir %s hp=%d: max|h| %.4g, worst |dh| / (2^-24 scale) = %.4f" % (name, hp, float(np.abs(href).max()), ratio))
    assert float(np.abs(href).max()) > 1e-3
    assert ratio <= RIR_C, ratio


def test_generator_is_reproducible_and_independent_of_the_batch():
    device()
    from tensorflowasr_amd.augment import ImageSourceRIR
    room, c, fs, ns, T = SMALL
    rng = np.random.default_rng(3)
    s = rng.uniform(0.05, 0.95, (5, 3)) * room
    r = rng.uniform(0.05, 0.95, (5, 3)) * room
    for hp in (False, True):
        gen = ImageSourceRIR(fs, room=room, reverberation_time=T, nsample=ns, c=c, hp_filter=hp)
        both = gen.generate(s, r).cpu().numpy()
        assert np.array_equal(gen.generate(s, r).cpu().numpy(), both)
        for b in range(5):
            assert np.array_equal(gen.generate(s[b:b + 1], r[b:b + 1]).cpu().numpy()[0], both[b]), (hp, b)
        assert len({both[b].tobytes() for b in range(5)}) == 5
    # zeros past nsample, whatever the buffer held
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    t = np.ascontiguousarray(gen.params(s[:2], r[:2]))
    wb = ctypes.c_size_t()
    assert lib.mi355asr_rir_workspace_bytes(2, ctypes.byref(wb)) == 0
    ws = torch.empty(wb.value // 8, dtype=torch.float64, device="cuda:0")
    h = torch.full((2, ns + 300), float("nan"), device="cuda:0")
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    assert lib.mi355asr_rir_generate(t.ctypes.data_as(ctypes.c_void_p), 2, p(h), ns + 300, p(ws), wb.value, None) == 0
    h = h.cpu().numpy()
    assert np.array_equal(h[:, :ns], both[:2]) and not h[:, ns:].any()
    t[1, 3:6] = t[1, 6:9]                                 # the source at the receiver: refused before any launch
    assert lib.mi355asr_rir_generate(t.ctypes.data_as(ctypes.c_void_p), 2, p(ws), ns, p(ws), wb.value, None) == -1
    assert b"row 1" in lib.mi355asr_last_error()


# ---- mixing ------------------------------------------------------------------------------------------------------------------------
def test_mixing_parity_zero_powers_and_quantisation():
    device()
    from tensorflowasr_amd.augment import AddNoise
    lens = [1, 17, 160000]
    snrs = [-10.0, 0.0, 15.0]
    rng = np.random.default_rng(8)
    x = (0.3 * rng.standard_normal((3, 160000))).astype(np.float32)
    d = rng.standard_normal((3, 160000 + 9)).astype(np.float32)
    mix = AddNoise()
    for snr in snrs:
        y = mix(x, lens, d, snr).cpu().numpy()
        for b, n in enumerate(lens):
            y64, g64 = ar.mix_snr(x[b, :n], d[b, :n], snr)
            tol = 2.0 ** -23 * (np.abs(x[b, :n].astype(np.float64)) + 2 * np.abs(g64 * d[b, :n].astype(np.float64)))
            err = np.abs(y[b, :n].astype(np.float64) - y64)
            assert (err <= tol).all(), (snr, b, float((err / tol).max()))
            assert not y[b, n:].any()
            print("mix snr %+.0f len %d: g %.5g, largest error %.3f of its bound" % (snr, n, g64, float((err / tol).max())))
    # per-row SNRs in one call equal the calls above, row by row
    y = mix(x, lens, d, snrs).cpu().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(y[b], mix(x, lens, d, snrs[b]).cpu().numpy()[b])
    # silent noise, and a silent signal: y = x
    assert np.array_equal(mix(x, lens, np.zeros_like(d), 5.0).cpu().numpy()[2], x[2])
    z = np.zeros_like(x)
    assert not mix(z, lens, d, 5.0).cpu().numpy().any()
    # the quantise flag: the NumPy expression on the unquantised float32 result, bit for bit (values beyond +-1 among them)
    big = (4.0 * x).astype(np.float32)
    plain = mix(big, lens, d, snrs).cpu().numpy()
    q = mix(big, lens, d, snrs, quantise=True).cpu().numpy()
    assert np.abs(plain).max() > 1.5
    for b, n in enumerate(lens):
        assert np.array_equal(q[b, :n], ar.quantise(plain[b, :n])) and not q[b, n:].any()
    edge = np.array([[1.0, -1.0, 0.99999, -0.99999, 3.0e-5, -3.0e-5, 0.5, -2.0]], np.float32)
    assert np.array_equal(mix(edge, None, np.zeros_like(edge), 0.0, quantise=True).cpu().numpy(), ar.quantise(edge))


# ---- the chain and the hook ---------------------------------------------------------------------------------------------------------
def test_farfield_equals_its_three_stages():
    device()
    from tensorflowasr_amd.augment import AddNoise, FarField, ImageSourceRIR, Reverb, cut_noise
    room, c, fs, ns, T = SMALL
    gen = ImageSourceRIR(fs, room=room, reverberation_time=T, nsample=ns, c=c)
    rng = np.random.default_rng(12)
    bank = [rng.standard_normal(700).astype(np.float32), rng.standard_normal(5000).astype(np.float32)]
    lens = [3000, 0, 1234, 17]
    x = (0.2 * rng.standard_normal((4, 3000))).astype(np.float32)
    ff = FarField(gen, noise_bank=bank, snr=(0, 15))
    y, out_len = ff(x, lens, np.random.default_rng(5))
    y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
    assert list(out_len) == [n + ns - 1 if n else 0 for n in lens]
    last = ff.last
    assert all(s != r for s, r in zip(last["sources"], last["receivers"])) and all(0 <= v < 15 for v in last["snr_db"])
    h = gen.generate(last["sources"], last["receivers"])
    rv, rl = Reverb()(x, lens, h)
    d = np.zeros((4, rv.shape[1]), np.float32)
    for b in range(4):
        d[b, :out_len[b]] = cut_noise(bank[last["noise"][b]], int(out_len[b]), lambda high: last["starts"][b])
    want = AddNoise()(rv, rl, d, np.asarray(last["snr_db"], np.float32), quantise=True).cpu().numpy()
    assert np.array_equal(y, want) and np.abs(y).max() > 0.01
    assert np.array_equal(y, ar.quantise(y))


def test_offline_stt_batch_with_an_augmentation(tmp_path):
    from test_gpu_vad import _asr
    from tensorflowasr_amd.augment import FarField
    asr = _asr(tmp_path)
    rng = np.random.default_rng(21)
    items = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (24000, 57123, 33335)]
    plain = asr.offline_stt_batch(items)
    assert asr.offline_stt_batch(items, augment=None) == plain and any(p for p, _ in plain)
    # a one-tap filter and no noise: the transcripts of the quantised waveforms
    ff = FarField(rir=np.ones(1, np.float32), noise_bank=None, quantise=True)
    assert asr.offline_stt_batch(items, augment=ff) == asr.offline_stt_batch([ar.quantise(w) for w in items])


def test_augmentation_process_batch_is_its_draws_applied_stage_by_stage():
    """the reference's class on the device: seeded, every utterance is what its own draws give through the three stages"""
    import random
    device()
    from test_augment_host import config
    from tensorflowasr_amd.augment import AddNoise, Augmentation, ImageSourceRIR, Reverb
    rng = np.random.default_rng(4)
    bank = [rng.standard_normal(900).astype(np.float32), rng.standard_normal(4000).astype(np.float32)]
    wavs = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (800, 1, 2500, 1700, 333, 64)]
    aug = Augmentation(config(rir=True, noise=True), noise_bank=bank)
    random.seed(11)
    np.random.seed(11)
    got = aug.process_batch(wavs)
    random.seed(11)
    np.random.seed(11)
    drawn = [aug.draw(len(w)) for w in wavs]
    assert {a.key for a, _ in drawn} == {"rir", "noise"}
    gen = ImageSourceRIR(16000)
    for w, (a, d), y in zip(wavs, drawn, got):
        if a.key == "rir":
            rv, n = Reverb()(w, None, gen.generate([d["source"]], [d["receiver"]]))
            want = ar.quantise(rv.cpu().numpy()[0, :int(n[0])])
            assert len(y) == len(w) + 4095
        else:
            want = AddNoise()(w, None, d["segment"], float(d["snr_db"]), quantise=True).cpu().numpy()[0]
            assert len(y) == len(w)
        assert y.dtype == np.float32 and np.array_equal(y, want)
    random.seed(11)
    np.random.seed(11)
    one = aug.process(wavs[0])
    assert np.array_equal(one, got[0])
