"""Speech enhancement on the MI355X: vad.hip's enhance variant against the SavedModel's own float32 outputs
(tests/golden/vad_enhance_ref.npz), both decimations, tile cuts and short rows, batch independence, no write past a
row, the streaming enhancer against offline, the batched OnlineVAD, and the C ABI."""
import ctypes
import os

import numpy as np
import pytest

from test_vad_enhance_host import (ODD, SAVED_MODEL, _packets, _run_online, enhance64, enhance_inputs, input_frames,
                                   load_enh, saved_model_weights)
from test_vad_host import GOLDEN, load_ref

pytestmark = pytest.mark.gpu
TILE = 56


@pytest.fixture(scope="module")
def ref():
    return load_ref()


@pytest.fixture(scope="module")
def enh():
    return load_enh()


@pytest.fixture(scope="module")
def vad():
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    from tensorflowasr_amd.vad import VAD
    return VAD().load_saved_model(SAVED_MODEL)


def sample_err(got, want, x):
    """per-sample error of enhanced = x * mask, relative to max(|want|, |x|): the mask's error scaled like the scores'
    check (|d| / max(1, |mask|)); exact zeros of x must stay exact"""
    got, want, x = (np.asarray(a, np.float64) for a in (got, want, x))
    den = np.maximum(np.abs(want), np.abs(x))
    assert np.all(got[den == 0] == 0)
    return float((np.abs(got - want)[den > 0] / den[den > 0]).max()) if np.any(den > 0) else 0.0


@pytest.mark.parametrize("name", ["composed", "test8k"] + sorted(ODD))
def test_enhanced_frames_match_the_saved_model(ref, enh, vad, name):
    x, sr = enhance_inputs(ref, enh)[name]
    e, s = vad.enhance(x, sample_rate=sr)
    e, s = e.cpu().numpy().reshape(-1, 80), s.cpu().numpy().reshape(-1)
    keep = enh["ef_" + name]
    fr = input_frames(x, sr)
    err = sample_err(e[keep], enh["e32_" + name], fr[keep])
    serr = float((np.abs(s - enh["es32_" + name]) / np.maximum(1.0, np.abs(enh["es32_" + name]))).max())
    print("%s: T=%d enhanced worst rel err %.3g, scores %.3g" % (name, len(s), err, serr))
    assert err <= 1e-5 and serr <= 1e-4, (err, serr)


def test_scores_equal_the_onnx_handle_bit_for_bit(ref, vad):
    from tensorflowasr_amd.vad import VAD
    onnx = VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx"))
    x = ref["in_composed"].astype(np.float32) / 32768
    want = onnx.scores(x).cpu().numpy()
    assert np.array_equal(vad.scores(x).cpu().numpy(), want)           # vad_forward on the enhancer handle
    assert np.array_equal(vad.enhance(x)[1].cpu().numpy(), want)        # the enhance kernel's score head
    fr = input_frames(ref["in_test8k"].astype(np.float32) / 32768, 8000)[None]
    assert np.array_equal(vad.inference(fr), onnx.inference(fr))


@pytest.mark.parametrize("T", [1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("sr", [16000, 8000])
def test_tile_cuts_and_short_rows(vad, T, sr):
    dec = sr // 8000
    x = (np.random.default_rng(T * dec).standard_normal(T * 80 * dec + 37) * 0.1).astype(np.float32)
    e, s = vad.enhance(x, sample_rate=sr)
    fr = input_frames(x, sr)
    s64, e64 = enhance64(fr, saved_model_weights())
    assert e.shape == (1, T * 80) and s.shape == (1, T)
    assert sample_err(e.cpu().numpy().reshape(-1, 80), e64, fr) <= 1e-5
    assert np.abs(s.cpu().numpy()[0] - s64).max() <= 1e-4 * max(1.0, np.abs(s64).max())


def test_rows_are_independent_and_nothing_is_written_past_a_row(vad):
    import torch
    from tensorflowasr_amd import _lib
    rng = np.random.default_rng(5)
    lens = [16000 * 3 + 37, 16000, 5 * 160 + 159, 100, 0, 7 * 160]
    L = max(lens) + 1000
    x = (rng.standard_normal((len(lens), L)) * 0.1).astype(np.float32)
    padded = x.copy()
    for b, n in enumerate(lens):
        padded[b, n:] = rng.uniform(-1e30, 1e30, L - n)                    # never read
    h = vad._handle(2)
    T = L // 160
    xd = torch.from_numpy(padded).cuda()
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    sent = -12345.0
    e = torch.full((len(lens), T * 80), sent, device="cuda")
    s = torch.full((len(lens), T), sent, device="cuda")
    _lib.check(h.lib.mi355asr_vad_enhance(h.ptr, ctypes.c_void_p(xd.data_ptr()), len(lens), L,
                                          ctypes.c_void_p(ld.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                          ctypes.c_void_p(e.data_ptr()), h._stream()))
    torch.cuda.synchronize()
    e, s = e.cpu().numpy(), s.cpu().numpy()
    for b, n in enumerate(lens):
        tb = n // 160
        assert np.all(e[b, tb * 80:] == sent) and np.all(s[b, tb:] == sent), b
        if tb:
            e1, s1 = vad.enhance(x[b, :n])
            assert np.array_equal(e[b, :tb * 80], e1.cpu().numpy()[0]), b
            assert np.array_equal(s[b, :tb], s1.cpu().numpy()[0]), b
    # scores_dev = NULL: enhanced only, identical
    e2 = torch.full((len(lens), T * 80), sent, device="cuda")
    _lib.check(h.lib.mi355asr_vad_enhance(h.ptr, ctypes.c_void_p(xd.data_ptr()), len(lens), L,
                                          ctypes.c_void_p(ld.data_ptr()), None, ctypes.c_void_p(e2.data_ptr()),
                                          h._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(e2.cpu().numpy(), e)


def test_decimate_1_equals_decimate_2_on_the_same_samples(vad):
    x = (np.random.default_rng(9).standard_normal(300 * 160) * 0.1).astype(np.float32)
    e2, s2 = vad.enhance(x, sample_rate=16000)
    e1, s1 = vad.enhance(x[::2].copy(), sample_rate=8000)
    assert np.array_equal(e1.cpu().numpy(), e2.cpu().numpy()) and np.array_equal(s1.cpu().numpy(), s2.cpu().numpy())


@pytest.mark.parametrize("sr", [16000, 8000])
def test_streaming_enhancer_equals_offline_bit_for_bit(ref, vad, sr):
    from tensorflowasr_amd.enhance import StreamingEnhancer
    rng = np.random.default_rng(sr + 1)
    comp = ref["in_composed"].astype(np.float32) / 32768
    xs = [comp[:sr * 20], comp[sr * 7: sr * 9 + 13], (rng.standard_normal(sr * 5) * 0.1).astype(np.float32),
          comp[:100]]
    se = StreamingEnhancer(vad, len(xs), sample_rate=sr)
    got = [([], []) for _ in xs]
    pos = [0] * len(xs)
    while any(p < len(s) for p, s in zip(pos, xs)):
        chunks = []
        for i, s in enumerate(xs):
            n = int(rng.choice([0, 1, 80, 159, 160, 1601, 3200, 7777]))
            chunks.append(s[pos[i]:pos[i] + n])
            pos[i] += n
        for i, (e, sc) in enumerate(se.push(chunks)):
            got[i][0].append(e)
            got[i][1].append(sc)
    for i, s in enumerate(xs):
        e_off, s_off = vad.enhance(s, sample_rate=sr)
        assert np.array_equal(np.concatenate(got[i][0]), e_off.cpu().numpy()[0]), i
        assert np.array_equal(np.concatenate(got[i][1]), s_off.cpu().numpy()[0]), i


def test_batched_online_vad_matches_single_stream_and_reference(ref, enh, vad):
    from tensorflowasr_amd.vad import OnlineVAD, OnlineVADBatch
    pk = _packets(ref)
    single = _run_online(OnlineVAD(vad), pk)
    # the reference run's events: device scores agree in sign with the graph's on every window it scored
    assert single == [str(s) for s in enh["ov_lines"]]
    N = 16
    batch = OnlineVADBatch(vad, N)
    lines = [[] for _ in range(N)]
    for p in pk:
        for i, r in enumerate(batch.parse([p] * N)):
            if r == 1:
                lines[i] += ["sound end %r" % batch[i].live_result["end_time"], "=" * 22]
            elif r == 0:
                lines[i].append("sound start %r" % batch[i].live_result["start_time"])
    for i, r in enumerate(batch.final_parse()):
        if r == 1:
            lines[i] += ["sound end %r" % batch[i].live_result["end_time"], "=" * 22]
    assert all(l == single for l in lines)


def test_c_abi_enhance_on_a_scores_only_handle_is_einval(ref):
    import torch
    from tensorflowasr_amd import _lib
    from test_vad_host import graph_weights
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(lib.mi355asr_vad_create(ctypes.byref(_lib.VadConfig(80, 80, 2)), ctypes.byref(h)))
    try:
        for name, a in graph_weights().items():
            a = np.ascontiguousarray(a, np.float32)
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.mi355asr_load_weight(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.ndim, dims))
        _lib.check(lib.mi355asr_finalize_weights(h, None))
        x = torch.zeros((1, 1600), device="cuda")
        out = torch.full((1, 800), 7.0, device="cuda")
        rc = lib.mi355asr_vad_enhance(h, ctypes.c_void_p(x.data_ptr()), 1, 1600, None, None,
                                      ctypes.c_void_p(out.data_ptr()), None)
        assert rc == -1 and b"voice-mask" in lib.mi355asr_last_error()               # MI355ASR_EINVAL
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    finally:
        lib.mi355asr_destroy(h)


def test_c_abi_enhancer_rejects_missing_mask_weights():
    from tensorflowasr_amd import _lib
    from test_vad_host import graph_weights
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(lib.mi355asr_vad_enhancer_create(ctypes.byref(_lib.VadConfig(80, 80, 2)), ctypes.byref(h)))
    try:
        names = {lib.mi355asr_weight_name(h, i).decode() for i in range(lib.mi355asr_num_weights(h))}
        assert names == set(graph_weights()) | {"audio_voice_mask/kernel", "audio_voice_mask/bias"}
        for name, a in graph_weights().items():
            a = np.ascontiguousarray(a, np.float32)
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.mi355asr_load_weight(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.ndim, dims))
        assert lib.mi355asr_finalize_weights(h, None) != 0
    finally:
        lib.mi355asr_destroy(h)
