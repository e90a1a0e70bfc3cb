"""The GPU steps of tests/test_gpu_beam_streams.py, one per process: `python tests/beam_streams_gpu_steps.py STEP [TMPDIR]`.
Every device call asserts that `beam_last_path()` is a stream kernel, and every expected value comes from the host search: a
`BeamDecoder` (and its `fork()` for provisional frames), or `ctc_prefix_beam_decode` made to run the host search on the device's
own top-n lists (path 1, asserted) -- never from another launch of the kernels under test.  Comparisons are exact: n_hyp, the
float scores bit for bit, ids, lens; both searches break ties the same way by construction.  A step prints what it ran and exits
non-zero on the first mismatch; it is never repeated."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
if len(sys.argv) > 1 and sys.argv[1] in ("vocab9160", "server"):
    os.environ["MI355ASR_BEAM_DEVICE"] = "0"                           # the ONE-SHOT calls of these steps run the host search (path 1)

from tensorflowasr_amd import ngram                                    # noqa: E402
from tensorflowasr_amd.models import (BEAM_STREAM_PATHS, BeamDecoder, BeamStreams, beam_device_limits, beam_last_path,   # noqa: E402
                                      ctc_prefix_beam_decode)

GOLDEN = os.path.join(HERE, "golden")
RADIX, SCORER, SMALL = 5, 6, 7                                         # mi355asr_beam_last_path of the stream kernels


def expected_path(V, beam, top_n, with_scorer):
    lim = beam_device_limits(with_scorer)
    N = min(top_n, V)
    if with_scorer:
        return SCORER
    return SMALL if beam <= lim["small_beam"] and beam * (min(N, beam + 2) + 1) <= 256 else RADIX


def dev_step(bs, slots, x, nc, npk, n_best, max_len, what, is_logits=False):
    r = bs.read(bs.step(slots, x, nc, npk, is_logits=is_logits, n_best=n_best, max_len=max_len))
    got, want = beam_last_path(), expected_path(bs.num_classes, bs.beam_size, bs.cutoff_top_n, bs.ext_scorer is not None)
    assert got in BEAM_STREAM_PATHS and got == want, "%s: ran path %d, the dispatch rule says %d" % (what, got, want)
    return r


def rows_of(r, i):
    """slot i of a read result -> [(score bits, ids)] for the n_hyp hypotheses"""
    return [(int(r["scores"][i, j].view(np.int32)), r["ids"][i, j, :r["lens"][i, j]].tolist()) for j in range(r["n_hyp"][i])]


def rows_of_host(hyp, n_best):
    return [(int(np.float32(sc).view(np.int32)), toks) for sc, toks in hyp[:n_best]]


class HostSlots:
    """the expected values: one host BeamDecoder per slot, the peek through fork()"""

    def __init__(self, n, V, beam, cp, ctn, s):
        self.d = [BeamDecoder([""] * V, beam, cp, ctn, ext_scorer=s) for _ in range(n)]
        self.V = V

    def step(self, slot, frames, c, k):
        d = self.d[slot]
        hyp = d.decode_ids(frames[:c])
        return d.fork().decode_ids(frames[c:c + k]) if k else hyp

    def look(self, slot):
        return self.d[slot].decode_ids(np.zeros((0, self.V), np.float32))


def peaky(rng, n, V, conc=0.08):
    return rng.dirichlet(np.full(V, conc), size=n).astype(np.float32)


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def step_fixtures():
    from test_beam_lm_host import _check
    from test_beam_streams_host import CASES, KS, the_scorer
    from test_beam_lm_host import K, KO
    rng = np.random.default_rng(1)
    done = refused = pieces_done = 0
    for ci, (name, probs, beam, cp, ctn, sc, pieces) in enumerate(CASES):
        s = the_scorer(sc)
        V = probs.shape[-1]
        if not cp < 1.0:
            # cutoff_prob 1 visits every class (50 here, the device search takes 40 candidates): refused by name, as the one-shot
            # device search refuses it; test_beam_streams_host.py runs these cases through host=True
            try:
                BeamStreams(3, V, beam, cp, ctn, ext_scorer=s, max_frames=64)
            except ValueError as e:
                assert "cutoff_prob" in str(e)
                refused += 1
                continue
            raise AssertionError("case %s: cutoff_prob %g was not refused" % (name, cp))
        if name.startswith("plain"):
            k = int(name[5:])
            utts = [KS["c%d_probs" % k][u] for u in range(2)]          # two utterances, a reset between them
            rec = lambda call: (KS["c%d_ids" % k][call], KS["c%d_lens" % k][call], KS["c%d_scores" % k][call], int(KS["c%d_n" % k][call]))   # noqa: E731
        else:
            F, k = (K, int(name[2:])) if name.startswith("lm") else (KO, int(name[6:]))
            utts = [probs]
            rec = lambda call: (F["st_ids_%d_%d" % (k, call)], F["st_lens_%d_%d" % (k, call)], F["st_scores_%d_%d" % (k, call)], None)   # noqa: E731
        T_all = sum(pieces)
        bs = BeamStreams(3, V, beam, cp, ctn, ext_scorer=s, max_frames=T_all)
        host = HostSlots(3, V, beam, cp, ctn, s)
        other = [peaky(rng, T_all, V), peaky(rng, T_all, V, 0.5)]
        call = 0
        for u, p in enumerate(utts):
            if u:
                bs.reset([1])
                host.d[1].reset()
            t0, o0 = 0, [0, 0] if u == 0 else o0
            for nt in pieces:
                # the neighbours (slots 0 and 2) take other frames in other piece sizes, with a peek; they stop at capacity
                cn = [int(min(rng.integers(0, 6), T_all - o0[q])) for q in range(2)]
                kn = [int(min(rng.integers(0, 4), T_all - o0[q] - cn[q])) for q in range(2)]
                T = max(nt, cn[0] + kn[0], cn[1] + kn[1], 1)
                x = np.zeros((3, T, V), np.float32)
                x[0, :nt] = p[t0:t0 + nt]
                for q in range(2):
                    x[1 + q, :cn[q] + kn[q]] = other[q][o0[q]:o0[q] + cn[q] + kn[q]]
                r = dev_step(bs, [1, 0, 2], torch.from_numpy(x).cuda(), [nt] + cn, [0] + kn, beam, T_all, "%s piece %d" % (name, call))
                want = host.step(1, x[0], nt, 0)
                assert rows_of(r, 0) == rows_of_host(want, beam), "%s call %d: device != host BeamDecoder" % (name, call)
                for q in range(2):
                    assert rows_of(r, 1 + q) == rows_of_host(host.step(2 * q, x[1 + q], cn[q], kn[q]), beam), (name, call, "neighbour", q)
                    o0[q] += cn[q]
                assert r["status"].tolist() == [0, 0, 0] and r["frames"][0] == t0 + nt
                ref_ids, ref_lens, ref_sc, ref_n = rec(call)
                n = int(r["n_hyp"][0])
                if ref_n is not None:                                  # beam_stateful_kat.npz: as tests/test_host.py reads it
                    assert n == ref_n and np.array_equal(r["scores"][0, :n], ref_sc[:n]), (name, call)
                    for j in range(n):
                        assert r["ids"][0, j, :r["lens"][0, j]].tolist() == ref_ids[j][:int(ref_lens[j])].tolist(), (name, call, j)
                else:
                    _check(r["ids"][0], r["lens"][0], r["scores"][0], n, ref_ids, ref_lens, ref_sc, "%s piece %d" % (name, call), live_only=F is KO)
                t0 += nt
                call += 1
                pieces_done += 1
        done += 1
    assert done + refused == 12 and done >= 9, (done, refused)
    print("device streams == host BeamDecoder == the reference's recorded arrays on %d stateful cases (%d pieces); %d cases with "
          "cutoff_prob 1 refused by name" % (done, pieces_done, refused))


# ---- ticks ---------------------------------------------------------------------------------------------------------------
def step_ticks():
    from test_beam_lm_host import scorer
    V, T = 50, 12
    rng = np.random.default_rng(3)
    frames = [peaky(rng, 110, V, c) for c in (0.05, 0.1, 0.3, 1.0)]
    seen, n_calls = set(), 0
    for model in (None, 3, 6):
        s = scorer(model, 0.9, 0.2) if model else None
        for beam in (1, 4, 16, 17, 128):
            for ctn in (1, 40):
                bs = BeamStreams(5, V, beam, 0.99, ctn, ext_scorer=s, max_frames=120)
                alone = BeamStreams(5, V, beam, 0.99, ctn, ext_scorer=s, max_frames=120)      # every slot stepped in a call of its own
                host = HostSlots(5, V, beam, 0.99, ctn, s)
                fed = [0] * 4
                for tick in range(8):
                    slots = [int(v) for v in rng.permutation(4)[:int(rng.integers(1, 5))]]
                    nc = rng.integers(0, T + 1, len(slots))
                    npk = np.array([rng.integers(0, T + 1 - c) for c in nc])
                    x = np.zeros((len(slots), T, V), np.float32)
                    for i, sl in enumerate(slots):
                        x[i, :nc[i] + npk[i]] = frames[sl][fed[sl]:fed[sl] + nc[i] + npk[i]]
                    xd = torch.from_numpy(x).cuda()
                    what = "ticks model %s beam %d top_n %d tick %d" % (model, beam, ctn, tick)
                    r = dev_step(bs, slots, xd, nc, npk, min(beam, 3), 120, what)
                    seen.add(beam_last_path())
                    for i, sl in enumerate(slots):
                        want = rows_of_host(host.step(sl, x[i], int(nc[i]), int(npk[i])), min(beam, 3))
                        assert rows_of(r, i) == want, "%s slot %d: device != host" % (what, sl)
                        ra = dev_step(alone, [sl], xd[i:i + 1], nc[i:i + 1], npk[i:i + 1], min(beam, 3), 120, what + " alone")
                        for key in BeamStreams.FIELDS:
                            assert np.array_equal(r[key][i], ra[key][0]), "%s slot %d: %s depends on the neighbours" % (what, sl, key)
                        fed[sl] += int(nc[i])
                        assert r["frames"][i] == fed[sl] and r["status"][i] == 0
                    n_calls += 1
    assert seen == {RADIX, SCORER, SMALL}, seen
    print("device streams == host decoders == the same slot stepped alone: %d ticks over beams 1, 4, 16, 17, 128, cutoff_top_n 1 and 40, "
          "no scorer / order 3 / order 6; paths %s" % (n_calls, sorted(seen)))


# ---- peek ----------------------------------------------------------------------------------------------------------------
def step_peek():
    from test_beam_lm_host import scorer
    V, T = 50, 12
    rng = np.random.default_rng(4)
    for model, beam in ((None, 8), (None, 40), (3, 8), (6, 40)):
        s = scorer(model, 0.9, 0.2) if model else None
        p = peaky(rng, 60, V)
        bs = BeamStreams(2, V, beam, 0.99, 40, ext_scorer=s, max_frames=60)
        host = HostSlots(2, V, beam, 0.99, 40, s)
        t = 0
        # (commit, peek): a peek with nothing committed, twice (the second shows the first left nothing); commits with and without a peek
        for j, (c, k) in enumerate(((0, 5), (0, 7), (4, 8), (3, 0), (0, 0), (12, 0), (1, 11), (6, 2))):
            x = np.empty((1, T, V), np.float32)
            x[0, :c + k] = p[t:t + c + k]
            pad = np.array([np.nan, 1e30, -1e30], np.float32)          # rows past commit + peek: padding that may hold anything
            x[0, c + k:] = pad[rng.integers(0, 3, (T - c - k, V))]
            r = dev_step(bs, [1], torch.from_numpy(x).cuda(), [c], [k], beam, 60, "peek model %s beam %d call %d" % (model, beam, j))
            want = rows_of_host(host.step(1, x[0], c, k), beam)
            assert rows_of(r, 0) == want, ("peek", model, beam, j)
            t += c
            assert r["frames"][0] == t and r["status"][0] == 0
            # n_peek = NULL and zero frames: the committed beam, which the peek did not touch
            r0 = dev_step(bs, [1], torch.from_numpy(x).cuda(), [0], None, beam, 60, "look")
            assert rows_of(r0, 0) == rows_of_host(host.look(1), beam), ("the peek left something behind", model, beam, j)
    print("commit + peek == host decoder + fork() on 4 configurations x 8 calls; the committed beam after every peek is the host's; "
          "padding rows of NaN and +-1e30 are never read")


# ---- reset, capacity -----------------------------------------------------------------------------------------------------
def step_reset_capacity():
    V, beam, mf = 12, 16, 20
    rng = np.random.default_rng(2)
    p = peaky(rng, 2 * 30, V, 0.3).reshape(2, 30, V)
    bs = BeamStreams(2, V, beam, 0.99, 40, max_frames=mf)
    # the state again, with a guard behind it: the last slot's arena ends where the state ends
    guard = 256
    big = torch.full((bs.state_bytes + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
    bs.state = big[:bs.state_bytes]
    bs.reset()
    host = HostSlots(2, V, beam, 0.99, 40, None)
    pd = torch.from_numpy(p).cuda()

    def go(slots, lo, hi, nc, npk, what):
        return dev_step(bs, slots, pd[slots, lo:hi].contiguous(), nc, npk, beam, mf, what)
    a = go([0, 1], 0, 12, [12, 5], [0, 3], "first")
    assert rows_of(a, 0) == rows_of_host(host.step(0, p[0, :12], 12, 0), beam) and rows_of(a, 1) == rows_of_host(host.step(1, p[1, :12], 5, 3), beam)
    # slot 1 (the LAST slot): 5 + 15 = exactly max_frames is accepted; slot 0: 12 + 8 + 1 peek is one frame too many
    b = go([0, 1], 12, 27, [8, 15], [1, 0], "capacity")
    assert b["status"].tolist() == [1, 0] and b["frames"].tolist() == [12, 20]
    assert rows_of(b, 0) == rows_of_host(host.look(0), beam), "over capacity: the unchanged beam"
    assert rows_of(b, 1) == rows_of_host(host.step(1, p[1, 12:27], 15, 0), beam)
    c = go([0, 1], 12, 20, [8, 1], None, "after")                      # slot 0 was not touched by the refusal; slot 1 is full now
    assert c["status"].tolist() == [0, 1] and c["frames"].tolist() == [20, 20]
    assert rows_of(c, 0) == rows_of_host(host.step(0, p[0, 12:20], 8, 0), beam) and rows_of(c, 1) == rows_of_host(host.look(1), beam)
    tail = big[bs.state_bytes:].cpu().numpy()
    assert (tail == 0x5A).all(), "the bytes behind the last slot's arena were written"
    slot = bs.state_bytes // 2
    end = ((16 + 36 * beam + 15) & ~15) + 8 * (mf * beam + 1)           # the arena's end inside a slot (mi355asr.h)
    pad = big[:bs.state_bytes].cpu().numpy().reshape(2, slot)[:, end:]
    assert (pad == 0x5A).all(), "the cell past the arena's end was written"
    bs.reset([1])                                                      # a mid-way reset of one slot: slot 0 keeps its beam
    host.d[1].reset()
    d = go([1, 0], 20, 26, [6, 0], [0, 0], "reset")
    assert d["status"].tolist() == [0, 0] and d["frames"].tolist() == [6, 20]
    assert rows_of(d, 0) == rows_of_host(host.step(1, p[1, 20:26], 6, 0), beam) and rows_of(d, 1) == rows_of_host(host.look(0), beam)
    print("max_frames %d, beam %d: exactly max_frames accepted, one frame more gives status 1 with the state and the other slot "
          "untouched; %d guard bytes behind the arena (and %d of slot padding) unchanged; a reset slot starts over" % (mf, beam, guard, pad.shape[1]))


# ---- the text head's shape -----------------------------------------------------------------------------------------------
def one_shot_host(z, lens, beam, s, what):
    """the one-shot call on the same device tensor, made to run the host search on the device's top-n lists"""
    r = ctc_prefix_beam_decode(z, lens, beam, 0.99, 40, is_logits=True, ext_scorer=s, num_threads=16)
    assert beam_last_path() == 1, "%s: the one-shot call ran path %d, not the host search" % (what, beam_last_path())
    return r


def step_vocab9160():
    V, n, Tt, ticks, beam = 9160, 64, 4, 6, 10
    g = torch.Generator(device="cpu").manual_seed(6)
    z = torch.randn((n, Tt * ticks, V), generator=g) * 3.0
    z[..., -1] += 5.0
    z[..., :200] += 2.0                                                # the classes the model knows
    zd = z.cuda()
    m = ngram.read_arpa(os.path.join(GOLDEN, "lm_wide6.arpa"))
    words = [w for w in m.words if len(w) == 1][:2000]
    vocab = words + [chr(0xE000 + i) for i in range(V - 1 - len(words))]
    s = ngram.NGramScorer(0.8, 0.4, os.path.join(GOLDEN, "lm_wide6.arpa"), vocab)
    rng = np.random.default_rng(7)
    for sc in (None, s):
        bs = BeamStreams(n, V, beam, 0.99, 40, ext_scorer=sc, max_frames=Tt * ticks)
        pos = np.zeros(n, np.int64)
        for tick in range(ticks):
            nc = rng.integers(0, Tt + 1, n)
            npk = np.array([rng.integers(0, Tt + 1 - c) for c in nc])
            idx = torch.from_numpy(np.minimum(pos[:, None] + np.arange(Tt)[None], Tt * ticks - 1)).cuda()
            x = torch.gather(zd, 1, idx[:, :, None].expand(n, Tt, V)).contiguous()
            r = dev_step(bs, list(range(n)), x, nc, npk, 1, Tt * ticks, "V 9160 tick %d" % tick, is_logits=True)
            pos += nc
            ids, lens, scores, nh = one_shot_host(zd, (pos + npk).astype(np.int32), beam, sc, "V 9160")
            assert np.array_equal(r["scores"][:, 0].view(np.int32), scores[:, 0].view(np.int32)), ("scores", tick, sc is not None)
            assert np.array_equal(r["lens"][:, 0], lens[:, 0]) and np.array_equal(r["ids"][:, 0], ids[:, 0]), ("ids", tick, sc is not None)
            assert np.array_equal(r["frames"], pos) and not r["status"].any()
        print("64 streams x 6 ticks of logits, V = 9 160, beam 10, %s: every tick == the one-shot host search over the frames so far; "
              "frames per stream %d .. %d" % ("lm_wide6.arpa on the first %d classes" % len(words) if sc is not None else "scorer-less",
                                              pos.min(), pos.max()))


# ---- the server ----------------------------------------------------------------------------------------------------------
class Recording:
    """the recogniser's model behind a server, its stream_step calls counted and, when asked, the text logits of every call kept"""

    def __init__(self, runner, want_logits):
        self.runner, self.want_logits, self.calls, self.logits = runner, want_logits, 0, []
        self._h = runner._h

    def open_streams(self, n):
        return self.runner.open_streams(n)

    def reset_streams(self, st, slots=None):
        return self.runner.reset_streams(st, slots)

    def stream_step(self, st, slots, packets, n_samples=None, want_logits=False, **kw):
        self.calls += 1
        res = self.runner.stream_step(st, slots, packets, n_samples, want_logits=self.want_logits, **kw)
        if self.want_logits:
            self.logits.append({s: (res[s]["text_logits"].clone(), res[s]["n_valid"], res[s]["n_picked"]) for s in slots})
        return res


def step_server(tmp):
    import pathlib
    from helpers import co
    from test_gpu_chunk_streams import _chunk_asr_config
    from tensorflowasr_amd.chunk_asr import ChunkASR, ChunkStreamingServer
    for win_back in (8, 0):
        cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41, decoder_win_back=win_back)
        d = pathlib.Path(tmp) / ("wb%d" % win_back)
        d.mkdir()
        conf = _chunk_asr_config(d, cfg)
        conf["model_config"]["ChunkCTCDecoder"]["win_back"] = win_back     # (the helper builds the shipped YAML: win_back 8)
        chars = ["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4E00 + 7 * i) for i in range(36)]
        with open(conf["tar_config"]["vocabulary"], "w", encoding="utf-8") as f:
            f.write("\n".join(chars) + "\n")
        conf["tar_config"]["lm_config"] = {"lm_path": os.path.join(GOLDEN, "lm_small.arpa"), "alpha": 0.6, "beta": 0.5}
        conf["tar_config"]["beam_width"] = 4
        asr = ChunkASR(conf, load_checkpoint=False)
        asr.runner.load_weights(co.chunk_weights(cfg, seed=3), by_name=False)
        s = asr.text_featurizer.scorer
        assert s is not None and asr.text_featurizer.num_classes == 41
        W = asr.wav_buf_length
        audios = [co.synth_wave(5 + k, length=n).astype(np.float32) for k, n in enumerate((W * 14 - 300, W * 9 + 1000, W * 11 + 7))]
        # ---- every stream alone: stream_step(want_logits=True) behind a greedy server, the text from the host search
        want = []
        for a in audios:
            rec = Recording(asr.runner, True)
            alone = ChunkStreamingServer(asr, 1, rec)
            sl = alone.open()
            valid, unv, tuples = torch.zeros((0, 41), device="cuda:0"), torch.zeros((0, 41), device="cuda:0"), []
            for o in range(0, len(a), W):
                t = alone.tick({sl: a[o:o + W]})[sl]
                lg, nv, npicked = rec.logits[-1][sl]
                if npicked > 0:
                    valid, unv = torch.cat([valid, lg[:nv]]), (lg[nv:] if win_back else lg[:0])
                if t is None:
                    continue
                rows = torch.cat([valid, unv])[None].contiguous()
                best = []
                if rows.shape[1]:
                    ids, lens, _, _ = one_shot_host(rows, None, 4, s, "server, stream alone")
                    best = [int(v) for v in ids[0, 0, :lens[0, 0]] if v != 0]
                tuples.append((t[0], t[1], "".join(asr.text_featurizer.iextract(best))))
            want.append(tuples)
        assert all(len(t) >= 3 for t in want)
        # ---- three staggered streams in one server with the device beam
        rec = Recording(asr.runner, False)
        srv = ChunkStreamingServer(asr, 3, rec, beam_width=4, ext_scorer=s, max_text_frames=256)
        assert not srv.beam.host and srv.win_back == win_back
        before = getattr(asr.runner, "stream_readbacks", 0)
        got, slot_of, pos = {k: [] for k in range(3)}, {}, {k: 0 for k in range(3)}
        rng = np.random.default_rng(8)
        for rnd in range(200):
            for k in range(3):
                if rnd == 2 * k:
                    slot_of[k] = srv.open()
            msg = {}
            for k in slot_of:
                n = int(rng.choice([1700, 2560, 3000, 6000]))
                msg[slot_of[k]] = audios[k][pos[k]:pos[k] + n]
                pos[k] += n
            back = srv.send(msg)
            for k in list(slot_of):
                got[k] += back[slot_of[k]]
                if pos[k] >= len(audios[k]):
                    got[k] += srv.close(slot_of.pop(k))
            if rnd > 4 and not slot_of:
                break
        assert beam_last_path() == SCORER
        for k in range(3):
            assert got[k] == want[k], "win_back %d stream %d:\n%s\n%s" % (win_back, k, got[k], want[k])
        copies = asr.runner.stream_readbacks - before
        assert copies == rec.calls and rec.calls > 14, (copies, rec.calls)       # one device-to-host copy per tick, the beam's results in it
        greedy = ChunkStreamingServer(asr, 1)
        sl = greedy.open()
        g = greedy.send({sl: audios[0]})[sl] + greedy.close(sl)
        print("win_back %d: 3 staggered streams, %d ticks, one read-back each; tuples == each stream alone + the host search; last texts "
              "%r (greedy: %r)" % (win_back, rec.calls, [t[-1][2] for t in want], g[-1][2]))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    fn = globals()["step_" + name]
    fn(*sys.argv[2:3])
    torch.cuda.synchronize()
    print("step %s ok" % name)
