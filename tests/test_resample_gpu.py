"""The device polyphase resampler (csrc/resample.hip, tensorflowasr_amd/resample.py) on the MI355X: ragged batches against
scipy.signal.resample_poly in float64 within a bound derived from the filter, row isolation, int16 input, streams against the
one-shot call bit for bit, and the entry points that take a sample rate (ASR.offline_stt_batch, ASRSession.send,
ChunkStreamingServer)."""
import functools
import wave

import numpy as np
import pytest
from scipy.signal import resample_poly

from resample_ref import MORE_RATIOS, RATIOS, chain_float32, taps_and_gain
from tensorflowasr_amd.resample import out_length, stream_emitted

pytestmark = pytest.mark.gpu
# 1/20 (401 taps, 20 480 input samples per tile) is a ratio whose input span does not fit in LDS: the kernels read it through the caches
WITH_UNSTAGED = RATIOS + [(1, 20)]
# and the staged / unstaged boundary (1/18, 1/19), unstaged ratios with several phases (3/61, 101/640), staged ones close to the LDS
# budget (147/640, 639/640) and the limits 640/1 and 1/640
ALL_RATIOS = WITH_UNSTAGED + MORE_RATIOS


@functools.lru_cache(maxsize=None)
def resampler(up, down):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tensorflowasr_amd.resample import Resampler
    # any pair of rates in the ratio up / down
    return Resampler(down * 25, up * 25)


def length_for(target, up, down, side):
    """an input length whose output length is `target`, or, where the ratio has no such length (an up-sampler's output lengths
    are multiples of up), the nearest one below (side -1) or above (side +1) it"""
    L = target * down // up
    while out_length(L, up, down) < target:
        L += 1
    if out_length(L, up, down) == target or side > 0:
        return L
    return L - 1


@functools.lru_cache(maxsize=None)
def case(up, down):
    """the ragged batch of the parity and isolation tests, its float64 reference and what the device returned for it"""
    rs = resampler(up, down)
    tile, K = rs.tile, rs.taps
    assert K == taps_and_gain(up, down)[0]
    # two lengths of a few and of some twenty thousand samples, counted at the output where the ratio multiplies them (640/1)
    few, many = (4417, 20001) if up < 4 * down else (-(-4417 * down // up), -(-20001 * down // up))
    in_len = [0, 1, K - 1, few, many, length_for(tile - 1, up, down, -1), length_for(tile, up, down, +1),
              length_for(tile + 1, up, down, +1)]
    assert out_length(in_len[5], up, down) < tile <= out_length(in_len[6], up, down) < out_length(in_len[7], up, down)
    rng = np.random.default_rng(100 * up + down)
    x = rng.standard_normal((len(in_len), max(in_len))).astype(np.float32)
    ref = [resample_poly(x[b, :n].astype(np.float64), up, down) if n else np.zeros(0) for b, n in enumerate(in_len)]
    y, out_len = rs(x, in_len)
    return rs, x, in_len, ref, y.cpu().numpy(), out_len.cpu().numpy()


@pytest.mark.parametrize("up,down", ALL_RATIOS)
def test_parity_with_scipy_within_the_fp32_bound(up, down):
    """|d| <= (K + 2) 2^-23 A max|x|: the filter's rounding to fp32 (2^-24 per tap) and a K-term fp32 accumulation in any order
    (K 2^-24 relative to the sum of absolute terms <= A max|x|), with K taps per output and A the largest per-phase absolute tap
    sum -- both taken from the float64 filter, not from the device's output."""
    rs, x, in_len, ref, y, out_len = case(up, down)
    K, A = taps_and_gain(up, down)
    assert y.dtype == np.float32 and y.shape == (len(in_len), out_length(max(in_len), up, down))
    worst = 0.0
    for b, n in enumerate(in_len):
        assert out_len[b] == len(ref[b]) == out_length(n, up, down), b
        assert not y[b, out_len[b]:].any(), b
        if n:
            tol = (K + 2) * 2.0 ** -23 * A * float(np.abs(x[b, :n]).max())
            err = float(np.abs(y[b, :out_len[b]].astype(np.float64) - ref[b]).max())
            worst = max(worst, err / tol)
            assert err <= tol, (b, n, err, tol)
    # for the record: the error of the same sum in plain float32 NumPy (same tap order, product rounded, then added), on the last row
    b = len(in_len) - 1
    e32 = float(np.abs(chain_float32(x[b, :in_len[b]], up, down)[0].astype(np.float64) - ref[b]).max())
    err = float(np.abs(y[b, :out_len[b]].astype(np.float64) - ref[b]).max())
    print("ratio %d/%d: K=%d A=%.3f tile=%d, largest error %.3f of its bound; last row err / E32 = %.3f"
          % (up, down, K, A, rs.tile, worst, err / e32))


@pytest.mark.parametrize("up,down", ALL_RATIOS)
def test_rows_are_isolated_and_runs_repeat(up, down):
    rs, x, in_len, ref, y, out_len = case(up, down)
    poisoned = x.copy()
    for b, n in enumerate(in_len):
        poisoned[b, n:] = np.nan                       # never read
    y2 = rs(poisoned, in_len)[0].cpu().numpy()
    assert not np.isnan(y2).any()
    assert np.array_equal(y2, y)
    assert np.array_equal(rs(poisoned, in_len)[0].cpu().numpy(), y2)
    for b, n in enumerate(in_len):
        alone, alone_len = rs(x[b, :n])
        assert int(alone_len[0]) == out_len[b]
        assert np.array_equal(alone.cpu().numpy()[0, :out_len[b]], y[b, :out_len[b]]), b


@pytest.mark.parametrize("up,down", ALL_RATIOS)
def test_int16_input_gives_the_bits_of_its_float_conversion(up, down):
    rs = resampler(up, down)
    rng = np.random.default_rng(5)
    in_len = [3001, 1, 0, 2999, rs.taps + 8]
    pcm = rng.integers(-32768, 32768, (len(in_len), 3001)).astype(np.int16)
    if down >= 100 * up:
        pcm[0] = pcm[0] // 2 + 16000                   # thousands of taps average noise away: an offset keeps the output large
    pcm[0, :4] = (-32768, 32767, 0, -1)
    yi, li = rs(pcm, in_len)
    yf, lf = rs(pcm.astype(np.float32) / 32768, in_len)
    assert np.array_equal(li.cpu().numpy(), lf.cpu().numpy())
    assert np.array_equal(yi.cpu().numpy(), yf.cpu().numpy()) and yi.abs().max() > 0.1
    # rows that do not start on a 16-byte boundary take the scalar loads: the same bits
    yo, _ = rs(pcm[:, :2999].copy(), [2999, 1, 0, 2999, rs.taps + 8])
    assert np.array_equal(yo.cpu().numpy()[3], yi.cpu().numpy()[3, :yo.shape[1]])


@pytest.mark.parametrize("up,down", [(2, 1), (1, 3), (160, 441), (1, 20)])
def test_streams_equal_the_one_shot_call_bit_for_bit(up, down):
    from tensorflowasr_amd.resample import StreamResampler
    rs = resampler(up, down)
    max_packet = 2000
    srs = StreamResampler(4, down * 25, up * 25, max_packet)
    rng = np.random.default_rng(9 * up + down)
    sizes = [1, 7, 160, 1280, max_packet]
    slots = [3, 0, 2]
    plans = {s: [sizes[(i + k) % 5] for i in range(11)] + [int(rng.choice(sizes)) for _ in range(4)] for k, s in enumerate(slots)}
    audio = {s: rng.standard_normal(sum(p)).astype(np.float32) for s, p in plans.items()}
    got = {s: [] for s in slots}
    pos = {s: 0 for s in slots}
    nxt = {s: 0 for s in slots}
    restarted = False
    step = 0
    while any(nxt[s] < len(plans[s]) for s in slots):
        # steps name different subsets: every live slot, except one that sits out every third step
        names = [s for k, s in enumerate(slots) if nxt[s] < len(plans[s]) and (step % 3 != k or step % 2)]
        step += 1
        if not names:
            continue
        if step == 8 and not restarted:                 # slot 0 is reset mid-way and starts again from its first sample
            srs.reset([0])
            got[0], pos[0], nxt[0], restarted = [], 0, 0, True
        packets = [audio[s][pos[s]:pos[s] + plans[s][nxt[s]]] for s in names]
        new = srs.step(names, packets)
        for s, p in zip(names, packets):
            want = stream_emitted(pos[s] + len(p), up, down) - stream_emitted(pos[s], up, down)
            assert len(new[s]) == want, (s, pos[s], len(p))
            got[s].append(new[s])
            pos[s] += len(p)
            nxt[s] += 1
    assert restarted
    tails = srs.flush(slots)
    for s in slots:
        one, n = rs(audio[s])
        one = one.cpu().numpy()[0, :int(n[0])]
        mine = np.concatenate(got[s] + [tails[s]])
        assert len(tails[s]) == out_length(pos[s], up, down) - stream_emitted(pos[s], up, down)
        assert mine.shape == one.shape and np.array_equal(mine, one), s
        assert srs.pos[s] == 0                           # flushed slots are fresh again
    with pytest.raises(ValueError, match="twice"):
        srs.step([1, 1], [audio[0][:4], audio[0][:4]])
    with pytest.raises(ValueError, match="out of range"):
        srs.step([4], [audio[0][:4]])
    with pytest.raises(ValueError, match="max_packet"):
        srs.step([1], [np.zeros(max_packet + 1, np.float32)])


def test_refusals_of_the_c_entry_points():
    import ctypes
    import torch
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.resample import Resampler
    assert torch.cuda.is_available()
    lib = _lib.lib()
    v = ctypes.c_int32()
    assert lib.mi355asr_resample_plan(641, 1, ctypes.byref(v), None, None, None) == -1
    assert b"641/1" in lib.mi355asr_last_error()
    with pytest.raises(ValueError, match="16001/96000"):
        Resampler(96000, 16001)
    same = Resampler(16000, 16000)                        # a copy / the int16 conversion
    pcm = np.array([[-32768, 16384, 5, 0]], np.int16)
    y, n = same(pcm, [3])
    assert np.array_equal(y.cpu().numpy(), [[-1.0, 0.5, 5 / 32768, 0.0]]) and int(n[0]) == 3


def test_offline_stt_batch_with_sample_rates(tmp_path):
    """an 8 kHz array, a 48 kHz int16 WAV and a 16 kHz array in one call == the call on the three waveforms resampled outside;
    without sample_rates the call is what it was"""
    from test_gpu_vad import _asr
    from tensorflowasr_amd.resample import Resampler
    asr = _asr(tmp_path)
    rng = np.random.default_rng(21)
    x8 = (0.1 * rng.standard_normal(24000)).astype(np.float32)
    pcm48 = (np.clip(0.1 * rng.standard_normal(100003), -1, 1) * 32767).astype("<i2")
    x16 = (0.1 * rng.standard_normal(57123)).astype(np.float32)
    path = str(tmp_path / "u48.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(48000)
        f.writeframes(pcm48.tobytes())

    def outside(rate, x):
        y, n = Resampler(rate, 16000)(x)
        return y.cpu().numpy()[0, :int(n[0])]
    plain = [outside(8000, x8), outside(48000, pcm48), x16]
    assert [len(p) for p in plain] == [48000, 33335, 57123]
    want = asr.offline_stt_batch(plain)
    assert asr.offline_stt_batch([x8, path, x16], sample_rates=[8000, 48000, None]) == want
    assert asr.offline_stt_batch([x8, pcm48, x16], sample_rates=[8000, 48000, 16000], max_batch_samples=60000) == want
    assert any(p for p, _ in want)
    assert asr.offline_stt_batch(plain, sample_rates=None) == [asr.offline_stt_wave(w) for w in plain] == want
    with pytest.raises(ValueError, match="48000 Hz file"):
        asr.offline_stt_batch([path], sample_rates=[44100])


def test_asr_session_send_with_a_sample_rate(tmp_path):
    from test_gpu_vad import _asr, load_ref
    from tensorflowasr_amd.resample import Resampler
    from tensorflowasr_amd.session import ASRSession
    from tensorflowasr_amd.vad import VAD
    from test_vad_host import GOLDEN
    import os
    s = ASRSession(_asr(tmp_path), VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx")))
    pcm8 = np.ascontiguousarray(load_ref()["in_composed"][::2]).astype(np.int16)
    y, n = Resampler(8000, 16000)(pcm8)
    want = s.send(y.cpu().numpy()[0, :int(n[0])])
    assert len(want) >= 1
    assert s.send(pcm8, sample_rate=8000) == want
    assert s.send(pcm8.astype(np.float32) / 32768, sample_rate=8000) == want


def test_chunk_streaming_server_with_an_input_rate(tmp_path):
    """two 8 kHz streams sent in uneven pieces == a server without input_rate fed, in one piece, the one-shot resampling"""
    import oracle.conformer_oracle as co
    from helpers import pick_bias_for_ragged_counts
    from test_gpu_chunk_streams import W, _chunk_asr_config, gated_waves
    from tensorflowasr_amd.chunk_asr import ChunkASR, ChunkStreamingServer
    from tensorflowasr_amd.resample import Resampler
    cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41)
    asr = ChunkASR(_chunk_asr_config(tmp_path, cfg), load_checkpoint=False)
    x16 = gated_waves(2, 12, 5)
    x8 = [np.ascontiguousarray(x16[0, :W * 12 - 700:2]), np.ascontiguousarray(x16[1, :W * 9 + 1234:2])]
    rs = Resampler(8000, 16000)
    up16 = []
    for a in x8:
        y, n = rs(a)
        up16.append(y.cpu().numpy()[0, :int(n[0])])
    w = co.chunk_weights(cfg, seed=3)
    pad = np.stack([np.pad(a, (0, W * 12 - len(a))) for a in up16]).astype(np.float32)
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(cfg, w, pad)
    asr.runner.load_weights(w, by_name=False)
    ref_srv = ChunkStreamingServer(asr, 2)
    want = []
    for a in up16:
        slot = ref_srv.open()
        want.append(ref_srv.send({slot: a})[slot] + ref_srv.close(slot))
    srv = ChunkStreamingServer(asr, 4, input_rate=8000, max_input_packet=3000)
    slots = [srv.open() for _ in range(2)]
    got = {s: [] for s in slots}
    pos = [0, 0]
    rng = np.random.default_rng(4)
    while any(pos[k] < len(x8[k]) for k in range(2)):
        msg = {}
        for k in range(2):
            if pos[k] < len(x8[k]) and rng.random() < 0.8:
                n = int(rng.choice([1, 37, 160, 1280, 3500]))
                msg[slots[k]] = x8[k][pos[k]:pos[k] + n]
                pos[k] += n
        for s, tuples in srv.send(msg).items():
            got[s] += tuples
    for k in range(2):
        got[slots[k]] += srv.close(slots[k])
        assert len(want[k]) > 3
        assert got[slots[k]] == want[k], k
    assert sorted(srv.free) == [0, 1, 2, 3]
