"""Ragged batches at dmodel 256 with 64-dim heads (the streaming configuration's global CTC decoder and Translator over
per-stream histories), the device-side histories (mi355asr_stream_append / mi355asr_stream_gather) and the batched
streaming server, on the MI355X.

Every comparison but one (named below) is exact (np.array_equal / ==): a ragged row is defined as the solo call's result.
That definition compares GPU calls with GPU calls; the same two entry points meet the float64 oracle (and in the bf16 mode the
rounding oracle), row by row and with a length on every boundary of attn64_class, in tests/test_gpu_ragged256_edges.py.

Which batches can be compared with solo calls bit for bit.  Attention and the depthwise conv are the stages that look across
rows, and in a ragged launch every utterance runs on the attention kernel its solo call takes (attn64_class), so they never
differ.  The dense layers are row-wise, but launch_gemm16 hands them to other kernels by the TOTAL row count of a call: the
slab-ring kernels from 1 500 rows on (MI355ASR_RING_MIN_M), the rows-resident bf16 kernel from 8 192 -- with another
accumulation order, as for any two calls without lengths of different batch sizes.  A solo call has at most 600 rows here, so
the solo comparisons use batches below 1 500 rows (B x T, and B x U for the Translator).  Larger batches (64 x 300, the ring
kernels, dwconv_tile_kernel<32, 128>, several workgroups of queries per utterance) are compared with the call without lengths at
equal lengths, checked for independence from the padding rows, from the order of the utterances and from the padded width (all
exact: the row count stays in the same kernel regime), and in fp32 mode with solo calls to 1e-4 of the largest logit -- the bound
the dmodel-144 ragged tests use for calls whose dense kernels differ (tests/test_gpu_ragged.py)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN

pytestmark = pytest.mark.gpu

LENGTHS = [1, 13, 16, 17, 32, 33, 64, 96, 97, 256, 257, 272, 273, 288, 289, 450, 600]
TMAX = [20, 100, 288, 289, 600]
ROWS = 1499          # below the ring kernels' crossover, see above


def _np(t):
    return t.cpu().numpy()


def _ctc(mode):
    from tensorflowasr_amd.models import CTCDecoder
    m = CTCDecoder(num_classes=60, dmodel=256, num_blocks=2, head_size=64, num_heads=4, kernel_size=32, gemm_dtype=mode)
    return m._build(seed=3)


def _groups(T):
    """the lengths up to T (T itself included) in batches of fewer than 1 500 rows"""
    lens = [n for n in LENGTHS if n < T] + [T]
    B = max(1, ROWS // T)
    return [lens[i:i + B] for i in range(0, len(lens), B)]


@pytest.mark.parametrize("mode", ["float32", "bfloat16"])
def test_ctc_decoder_ragged_rows_equal_solo_calls(mode):
    """row b of logits and arg-max == the call on enc[b:b+1, :T_b] alone, rows past T_b hold 0 / -1; every length = T: the call
    without lengths.  Fails before this change: mi355asr_ctc_forward_ragged refused dmodel 256 and the bf16 mode (EINVAL)."""
    m = _ctc(mode)
    rng = np.random.default_rng(1)
    seen = set()
    for T in TMAX:
        for lens in _groups(T):
            B = len(lens)
            assert B * T <= ROWS
            enc = rng.standard_normal((B, T, 256)).astype(np.float32)
            lg, am = m(enc, return_argmax=True, lengths=np.array(lens, np.int32))
            lg, am = _np(lg), _np(am)
            for b, n in enumerate(lens):
                slg, sam = m(enc[b:b + 1, :n], return_argmax=True)
                d = float(np.abs(lg[b, :n] - _np(slg)[0]).max())
                print("ctc %s T=%d len=%d max|d|=%.3g" % (mode, T, n, d))
                assert np.array_equal(lg[b, :n], _np(slg)[0]), (mode, T, n, d)
                assert np.array_equal(am[b, :n], _np(sam)[0]), (mode, T, n)
                assert not lg[b, n:].any() and (am[b, n:] == -1).all()
                seen.add(n)
        B = max(2, ROWS // T) if T * 2 <= ROWS else 1
        enc = rng.standard_normal((B, T, 256)).astype(np.float32)
        lg0, am0 = m(enc, return_argmax=True)
        lg1, am1 = m(enc, return_argmax=True, lengths=np.full(B, T, np.int32))
        assert np.array_equal(_np(lg0), _np(lg1)) and np.array_equal(_np(am0), _np(am1)), (mode, T)
    assert seen >= {1, 13, 16, 17, 32, 33, 288, 289, 600}


@pytest.mark.parametrize("mode", ["float32", "bfloat16"])
def test_ctc_decoder_large_batch(mode):
    """64 x 300 rows (the slab-ring / rows-resident kernels): every length = T is the call without lengths, and NaN in the rows
    past T_b changes no valid row"""
    m = _ctc(mode)
    rng = np.random.default_rng(2)
    B, T = 64, 300
    enc = rng.standard_normal((B, T, 256)).astype(np.float32)
    lg0, am0 = m(enc, return_argmax=True)
    lg1, am1 = m(enc, return_argmax=True, lengths=np.full(B, T, np.int32))
    assert np.array_equal(_np(lg0), _np(lg1)) and np.array_equal(_np(am0), _np(am1))
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    lens[:6] = [T, 13, 16, 17, 33, 289]
    clean = enc.copy()
    dirty = enc.copy()
    for b in range(B):
        clean[b, lens[b]:] = 0
        dirty[b, lens[b]:] = np.nan
    lgc, amc = m(clean, return_argmax=True, lengths=lens)
    lgd, amd = m(dirty, return_argmax=True, lengths=lens)
    lgc, amc = _np(lgc), _np(amc)
    assert np.isfinite(_np(lgd)).all()
    assert np.array_equal(lgc, _np(lgd)) and np.array_equal(amc, _np(amd))
    # the utterances in another order, and padded to another width (20 480 rows: the same dense kernels): the same rows
    perm = rng.permutation(B)
    lgp, amp = m(clean[perm], return_argmax=True, lengths=lens[perm])
    assert np.array_equal(_np(lgp), lgc[perm]) and np.array_equal(_np(amp), amc[perm])
    wide = np.full((B, T + 20, 256), np.nan, np.float32)
    wide[:, :T] = dirty
    lgw, amw = m(wide, return_argmax=True, lengths=lens)
    assert np.array_equal(_np(lgw)[:, :T], lgc) and np.array_equal(_np(amw)[:, :T], amc)
    if mode == "float32":
        # against solo calls (other dense kernels at 19 200 rows: a tolerance; a wrong bound in a kernel would be O(1))
        for b in list(range(6)) + [int(np.argmin(lens)), int(np.argmax(lens[6:])) + 6, 40, 63]:
            n = int(lens[b])
            solo = _np(m(enc[b:b + 1, :n]))[0]
            err = float(np.abs(lgc[b, :n] - solo).max()) / max(1.0, float(np.abs(solo).max()))
            print("large batch len=%d rel err=%.3g" % (n, err))
            assert err < 1e-4, (b, n, err)


def _translator():
    from tensorflowasr_amd.models import Translator
    t = Translator(inp_classes=60, tar_classes=100, dmodel=256, num_blocks=2, head_size=64, num_heads=4, kernel_size=32)
    return t._build(seed=11)


def test_translator_ragged_rows_equal_solo_calls():
    """token rows 1 .. U and encoder frames 1 .. T per utterance at dmodel 256: logits and arg-max == the solo call on the
    utterance's own rows; equal lengths == the call without lengths; NaN past the encoder frames reaches nothing"""
    t = _translator()
    rng = np.random.default_rng(5)
    U = 40
    toks = [1, 10, 16, 17, 23, 33, 40]
    for T in TMAX:
        for lens in _groups(T):
            B = len(lens)
            assert B * T <= ROWS and B * U <= ROWS
            tl = np.array([toks[(b + T) % len(toks)] for b in range(B)], np.int32)
            ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
            enc = rng.standard_normal((B, T, 256)).astype(np.float32)
            dirty = enc.copy()
            for b, n in enumerate(lens):
                dirty[b, n:] = np.nan
            lg, am = t([ids, dirty], return_argmax=True, token_lengths=tl, enc_lengths=np.array(lens, np.int32))
            lg, am = _np(lg), _np(am)
            for b, n in enumerate(lens):
                slg, sam = t([ids[b:b + 1, :tl[b]], enc[b:b + 1, :n]], return_argmax=True)
                d = float(np.abs(lg[b, :tl[b]] - _np(slg)[0]).max())
                print("translator T=%d enc_len=%d tokens=%d max|d|=%.3g" % (T, n, tl[b], d))
                assert np.array_equal(lg[b, :tl[b]], _np(slg)[0]), (T, n, int(tl[b]), d)
                assert np.array_equal(am[b, :tl[b]], _np(sam)[0]), (T, n, int(tl[b]))
                assert not lg[b, tl[b]:].any() and (am[b, tl[b]:] == -1).all()
        B = max(1, ROWS // T)
        ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
        enc = rng.standard_normal((B, T, 256)).astype(np.float32)
        lg0, am0 = t([ids, enc], return_argmax=True)
        lg1, am1 = t([ids, enc], return_argmax=True, token_lengths=np.full(B, U, np.int32), enc_lengths=np.full(B, T, np.int32))
        assert np.array_equal(_np(lg0), _np(lg1)) and np.array_equal(_np(am0), _np(am1)), T


def test_ragged_still_refuses_what_it_cannot_do():
    from tensorflowasr_amd._lib import Mi355AsrError
    from tensorflowasr_amd.models import CTCDecoder
    m = CTCDecoder(num_classes=60, dmodel=256, num_blocks=1, head_size=32, num_heads=8, kernel_size=32)._build(seed=1)
    with pytest.raises(Mi355AsrError, match="error -1:.*head size 32"):
        m(np.zeros((2, 40, 256), np.float32), return_argmax=True, lengths=[40, 20])
    m = CTCDecoder(num_classes=60, dmodel=256, num_blocks=1, head_size=64, num_heads=4, kernel_size=5)._build(seed=1)
    with pytest.raises(Mi355AsrError, match="error -1:.*kernel size 5"):
        m(np.zeros((2, 40, 256), np.float32), return_argmax=True, lengths=[40, 20])
    m = _ctc("float32")
    with pytest.raises(Mi355AsrError, match="error -1:.*16"):
        m(np.zeros((2, 16, 256), np.float32), return_argmax=True, lengths=[16, 5])


def test_stream_append_and_gather_against_numpy():
    import torch
    from tensorflowasr_amd._lib import Mi355AsrError
    from tensorflowasr_amd.stream_session import stream_append, stream_gather
    rng = np.random.default_rng(7)
    N, Tcap, d, Tc = 6, 39, 256, 13
    hist = torch.zeros((N, Tcap, d), dtype=torch.float32, device="cuda")
    hl = torch.zeros((N,), dtype=torch.int32, device="cuda")
    hl_host = np.zeros(N, np.int32)
    want = np.zeros((N, Tcap, d), np.float32)
    wl = np.zeros(N, np.int32)
    for slots in ([4, 1, 5], [1, 0], [5, 1, 3]):                       # out of order; slot 1 fills up
        c = rng.standard_normal((len(slots), Tc, d)).astype(np.float32)
        stream_append(torch.from_numpy(c).cuda(), slots, hist, hl, hl_host)
        for m_, s in enumerate(slots):
            want[s, wl[s]:wl[s] + Tc] = c[m_]
            wl[s] += Tc
    assert np.array_equal(_np(hist), want) and np.array_equal(_np(hl), wl) and np.array_equal(hl_host, wl)
    with pytest.raises(Mi355AsrError, match="error -1:.*overflow"):
        stream_append(torch.zeros((2, Tc, d), device="cuda"), [0, 1], hist, hl, hl_host)
    with pytest.raises(Mi355AsrError, match="error -1:.*twice"):
        stream_append(torch.zeros((2, Tc, d), device="cuda"), [3, 3], hist, hl, hl_host)
    assert np.array_equal(_np(hist), want) and np.array_equal(_np(hl), wl) and np.array_equal(hl_host, wl)   # nothing was written
    slots = [5, 0, 1, 4]
    tails = rng.standard_normal((4, 26, d)).astype(np.float32)
    tl = [26, 0, 7, 13]
    Tpad = 70
    out, ol = stream_gather(hist, hl, hl_host, slots, Tpad, torch.from_numpy(tails).cuda(), tl)
    exp = np.zeros((4, Tpad, d), np.float32)
    for r, s in enumerate(slots):
        exp[r, :wl[s]] = want[s, :wl[s]]
        exp[r, wl[s]:wl[s] + tl[r]] = tails[r, :tl[r]]
    assert np.array_equal(_np(out), exp) and _np(ol).tolist() == [int(wl[s]) + t for s, t in zip(slots, tl)]
    out, ol = stream_gather(hist, hl, hl_host, [1, 3], 40)
    assert np.array_equal(_np(out)[0, :39], want[1]) and not _np(out)[0, 39:].any() and _np(ol).tolist() == [39, 13]
    with pytest.raises(Mi355AsrError, match="error -1:.*Tpad"):
        stream_gather(hist, hl, hl_host, [1], 38)
    with pytest.raises(Mi355AsrError, match="error -1:.*nothing"):
        stream_gather(hist, hl, hl_host, [2], 17)


def _streaming_asr(tmp_path):
    from tensorflowasr_amd.asr import ASR
    from tensorflowasr_amd.config import load_yaml
    (tmp_path / "phones.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + ["p%d" % i for i in range(56)]) + "\n")
    (tmp_path / "chars.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4e00 + i) for i in range(96)]) + "\n")
    here = os.path.join(os.path.dirname(GOLDEN), "..", "tensorflowasr_amd", "configs")
    cfg = load_yaml(os.path.join(here, "am_data_streaming.yml"))
    cfg.update(load_yaml(os.path.join(here, "Streaming_ConformerS.yml")))
    cfg["model_config"]["num_blocks"] = 2
    cfg["inp_config"]["vocabulary"] = str(tmp_path / "phones.txt")
    cfg["tar_config"]["vocabulary"] = str(tmp_path / "chars.txt")
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    return ASR(cfg, load_checkpoint=False)


def test_server_equals_single_sessions(tmp_path):
    """8 streams at staggered offsets over the composed recording, the real detector and a seeded streaming ASR: every stream's
    events (times and texts) are those of a StreamingASRSession run alone on the same audio, and a sentence-end text is
    ASR.decode of the history ASR.extract_feature produces chunk by chunk"""
    import vad_golden
    from tensorflowasr_amd.stream_session import StreamingASRServer, StreamingASRSession
    from tensorflowasr_amd.vad import VAD
    vad = VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx"))
    asr = _streaming_asr(tmp_path)
    x = vad_golden.composed_i16()
    n = 1600                                                         # 0.1 s packets
    S, span = 8, 16000 * 16
    offs = [16000 * 5 * i + 160 * i for i in range(S)]
    feeds = [[x[o:o + span][k:k + n].tobytes() for k in range(0, span // n * n, n)] for o in offs]
    srv = StreamingASRServer(asr, vad, S, max_history_s=30.)
    got = [[] for _ in range(S)]
    for k in range(len(feeds[0])):
        pk = [f[k] if (k + i) % 11 else None for i, f in enumerate(feeds)]
        for i, e in enumerate(srv.send(pk)):
            if pk[i] is not None:
                got[i].append(e)
        for i, f in enumerate(feeds):                                # the packets a stream skipped arrive on the next tick
            if pk[i] is None:
                got[i].append(srv.send([f[k] if j == i else None for j in range(S)])[i])
    for i, e in enumerate(srv.final_send()):
        got[i].append(e)
    class Recording:
        """the recogniser with a log: the audio of every extract_feature call and, per decode call, which of them it was given"""

        def __init__(self):
            self.audio, self.made, self.decodes = [], {}, []

        def extract_feature(self, wav):
            e = asr.extract_feature(wav)
            self.made[id(e)] = len(self.audio)
            self.audio.append((np.array(wav, np.float32), e))
            return e

        def decode(self, encs):
            text = asr.decode(encs)
            self.decodes.append(([self.made[id(e)] for e in encs], text))
            return text

    n_end, texts = 0, []
    for i, f in enumerate(feeds):
        rec = Recording()
        s = StreamingASRSession(rec, vad, session="asr_%d" % (i + 1))
        want = [s.send(p) for p in f] + [s.final_send()]
        assert got[i] == want, (i, [e for e in got[i] if e], [e for e in want if e])
        ends = [e for e in got[i] if e and e["event_type"] == "sentence end"]
        n_end += len(ends)
        texts += [e["best_text"] for e in got[i] if e and "best_text" in e]
        # the server's sentence-end texts from scratch: extract_feature piece by piece, decode of that history
        by_text = [(idx, t) for idx, t in rec.decodes]
        for e in ends:
            idx = next(idx for idx, t in reversed(by_text) if t == e["best_text"])
            hist = [asr.extract_feature(rec.audio[k][0]) for k in idx]
            assert asr.decode(hist) == e["best_text"], (i, e)
    print("server texts:", texts)
    assert n_end >= 4
    assert any(texts) and len(set(texts)) >= 2, texts
    # a sentence-end text against extract_feature / decode by hand: 2.3 s of speech, four full chunks and a tail
    piece = x[16000 // 2:16000 // 2 + 36800].astype(np.float32) / 32768
    encs = [asr.extract_feature(piece[k:k + 8000]) for k in range(0, 32000, 8000)] + [asr.extract_feature(piece[32000:])]
    assert [int(e.shape[1]) for e in encs] == [13] * 5
    import torch
    lens = np.array([65, 26], np.int32)
    batch = torch.zeros((2, 65, encs[0].shape[2]), device=encs[0].device)
    batch[0] = torch.cat(encs, 1)[0]
    batch[1, :26] = torch.cat(encs[:2], 1)[0]
    texts = asr.decode_batch(batch, torch.from_numpy(lens).to(batch.device))
    assert texts == [asr.decode(encs), asr.decode(encs[:2])]


def test_server_history_overflow_is_per_stream(tmp_path):
    import vad_golden
    from tensorflowasr_amd.stream_session import StreamHistoryOverflow, StreamingASRServer
    from tensorflowasr_amd.vad import VAD
    vad = VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx"))
    asr = _streaming_asr(tmp_path)
    x = vad_golden.composed_i16()
    srv = StreamingASRServer(asr, vad, 2, max_history_s=1.0)         # two chunks per sentence
    a, b = x[8000:], np.zeros(len(x), np.int16)                      # speech / silence
    seen = []
    for k in range(0, 16000 * 6, 1600):
        ev = srv.send([a[k:k + 1600].tobytes(), b[k:k + 1600].tobytes()])
        assert ev[1] is None
        seen.append(ev[0])
    assert any(isinstance(e, StreamHistoryOverflow) for e in seen)
