"""Shared pieces of the ragged ChunkConformer tests (tests/test_chunk_ragged_host.py, tests/test_gpu_chunk_ragged.py): the
length constructor, the model configuration, the weights, the batches and the float64 oracle on each utterance alone.

Geometry of the 'valid' chunk front: F = (L - 1) // hop + 1, T1 = (F + 1) // 2 + 1, T = (T1 - 3) // 2 + 1.
An encoder length T has two T1 (2 T + 1 odd, 2 T + 2 even), a T1 has two F (2 T1 - 3 odd, 2 T1 - 2 even), and a frame count F
covers the sample counts (F - 1) hop + 1 .. F hop: L_for names all of them."""
import numpy as np

from helpers import co

HOP = 160
TOL = 1e-3                      # the project's contract against the float64 oracle
MARGIN = 10 * TOL               # the oracle's top-two margin every valid picker frame must have where picks are compared
PARITIES = [(False, False), (False, True), (True, False), (True, True)]      # (F odd, T1 odd)
RESIDUES = [1, 159, 0]                                                       # L mod hop
COMBOS = [(f, t, r) for f, t in PARITIES for r in RESIDUES]


def L_for(T, parity, residue):
    """the sample count with T encoder frames whose F and T1 have the parities (F odd, T1 odd) and L mod hop == residue"""
    f_odd, t1_odd = parity
    T1 = 2 * T + 1 if t1_odd else 2 * T + 2
    F = 2 * T1 - 3 if f_odd else 2 * T1 - 2
    return (F - 1) * HOP + (residue if residue else HOP)


def geometry_for(T, parity):
    f_odd, t1_odd = parity
    T1 = 2 * T + 1 if t1_odd else 2 * T + 2
    return dict(F=2 * T1 - 3 if f_odd else 2 * T1 - 2, T1=T1, T=T)


def config(**kw):
    """the issue's test model: chunk_conformerS with two encoder blocks and 300 text classes"""
    return dict(co.CHUNK_S, enc_num_blocks=2, decoder_num_classes=300, **kw)


def weights(cfg, seed=3, first_bias=0.0, blank_bias=0.0):
    """co.chunk_weights; first_bias: added to the picker's class 0, so that (at 20) the two largest picker logits of every frame
    are class 0 and the blank or the runner-up ~15 below -- the pick decision of a frame then IS its top-two margin, or is far
    from it; blank_bias: the picker's blank"""
    w = co.chunk_weights(cfg, seed=seed, picker_blank_bias=blank_bias)
    w["picker/fully_connected/bias"][0] = first_bias
    return w


def utterance(L, k):
    """utterance k of L samples: the gated sinusoids of co.synth_wave, cut from a longer wave so that a prefix of one length is not
    a prefix of another"""
    return co.synth_wave(700 + k, L + 37 * (k % 5))[37 * (k % 5):][:L].astype(np.float32)


def padded(items, L=None, fill=np.nan):
    """[B, L] batch of the items, the padding of every row holding `fill` -> (x, lengths)"""
    lens = np.array([len(it) for it in items], np.int32)
    x = np.full((len(items), int(L or lens.max())), fill, np.float32)
    for b, it in enumerate(items):
        x[b, :len(it)] = it
    return x, lens


_ALONE = {}


def alone(wav, w, cfg, key):
    """co.chunk_predict on one utterance alone, float64, every stage; computed once per (key, utterance).  An utterance without a
    pick has no helper and decoder input: co.chunk_predict cannot run its [1, 0, d] stacks, so its stages up to feature_pick are
    computed with the same functions and the rest is empty, as the reference's dynamic shapes would have it."""
    k = (key, wav.tobytes())
    if k not in _ALONE:
        x = wav[None].astype(np.float64)
        hs, fc = cfg["head_size"], cfg.get("fc_factor", 0.5)
        r = {}
        r["mel"], r["front"] = co.chunk_front(x, w, cfg)
        _, r["enc"] = co.chunk_stack(r["front"], w, "encoder", "chunk_conformer_block_", cfg["enc_num_blocks"], hs,
                                     cfg["enc_win_front"], cfg["enc_win_back"], fc, False, False)
        r["picker_logits"], r["picker_hidden"] = co.chunk_stack(r["enc"], w, "picker", "block_", cfg["picker_num_blocks"], hs,
                                                               cfg["picker_win_front"], cfg["picker_win_back"], fc, True, True)
        r["picked"], r["counts"] = co.feature_pick(r["picker_hidden"], r["picker_logits"], cfg["picker_num_classes"] - 1)
        if int(r["counts"][0]) == 0:
            r["helper"] = np.zeros((1, 0, cfg["dmodel"]))
            r["text_logits"] = np.zeros((1, 0, cfg["decoder_num_classes"]))
        else:
            r = co.chunk_predict(x, w, cfg)
        _ALONE[k] = r
    return _ALONE[k]


def top_two_margin(logits):
    """the gap between the two largest entries of every row of [..., V] logits"""
    s = np.sort(logits, axis=-1)
    return s[..., -1] - s[..., -2]


def assert_picker_margin(refs):
    """every valid picker frame of every utterance (its oracle run alone) decides its arg-max by at least 10 x TOL: no frame excused"""
    worst = min(float(top_two_margin(r["picker_logits"][0]).min()) for r in refs)
    assert worst >= MARGIN, "the oracle's smallest top-two picker margin is %.3g, below %.3g: choose other seeds" % (worst, MARGIN)
    return worst


# ---- the batches of the edge test: encoder lengths on win_back, win_front, their sum, the 16-row tile and the 64-query workgroup
EDGE_T = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 36, 37, 43, 44, 45, 63, 64, 65, 79, 80]
SMALL_M, NS1_MAX_M = 48, 4096            # the defaults of MI355ASR_SMALL_M and MI355ASR_NS1_MAX_M


def with_combos(Ts, start=0):
    """[(T, parity, residue)]: the combos dealt round the lengths"""
    return [(T,) + (COMBOS[(start + i) % len(COMBOS)][:2], COMBOS[(start + i) % len(COMBOS)][2]) for i, T in enumerate(Ts)]


def fill_lengths(n, Tmax, seed):
    """n lengths of 3 .. Tmax - 1 outside the edge set"""
    rng = np.random.default_rng(seed)
    pool = [t for t in range(3, Tmax) if t not in EDGE_T]
    return [int(t) for t in rng.choice(pool, size=n, replace=n > len(pool))]


def edge_batches():
    """name -> [(T_b, parity, residue)], one batch per block regime of the chunk stacks: rows = B x Tmax up to 48 (layer-at-a-time),
    up to 4096 (fused_ns) and above (fused_pp)"""
    out = {"layers-2x16": with_combos([16, 9]),
           "layers-3x15": with_combos([15, 1, 2], 2),
           "layers-6x8": with_combos([8, 7, 2, 1, 8, 5], 5),
           "ns-21x80": with_combos(EDGE_T[::-1], 1),
           "pp-52x80": with_combos(EDGE_T[::-1] + fill_lengths(31, 80, 80), 3)}
    return out


def batch_items(utts):
    return [utterance(L_for(T, par, r), i) for i, (T, par, r) in enumerate(utts)]


# ---- genuinely ragged picks: rows of one length whose pick counts differ -------------------------------------------------------
RAGGED_T = 48


def ragged_pick_rows():
    """six utterances of one length (48 encoder frames): one nearly silent throughout, one nearly silent for its first three
    quarters, four plain -- with the weights of seed 5 their blank gaps differ enough for ONE blank bias to leave the first
    without a pick and the second with fewer than win_back"""
    L = L_for(RAGGED_T, (True, False), 1)
    rows = []
    for k, mode in enumerate(("quiet", "tail", "", "", "", "")):
        x = utterance(L, 40 + k).copy()
        if mode == "quiet":
            x *= np.float32(1e-3)
        if mode == "tail":
            x[:3 * L // 4] *= np.float32(1e-3)
        rows.append(x)
    return rows


RAGGED_SEED = 5


def ragged_pick_bias(gaps, win_back):
    """gaps[b][t] = (class 0) - (blank at bias 0) of the oracle's picker logits.  The blank bias that leaves one row without a pick,
    one row with 1 .. win_back - 1 picks and every other row with some but not all of its frames, as far from every gap as
    possible -> (bias, its distance from the nearest gap)"""
    allg = np.sort(np.concatenate([np.ravel(g) for g in gaps]))
    best = None
    for lo, hi in zip(allg[:-1], allg[1:]):
        beta = 0.5 * (lo + hi)
        counts = [int((g > beta).sum()) for g in gaps]
        none = [c for c in counts if c == 0]
        few = [c for c in counts if 0 < c < win_back]
        rest = [c for c, g in zip(counts, gaps) if c >= win_back]
        if len(none) == 1 and len(few) >= 1 and rest and all(c < len(g) for c, g in zip(counts, gaps)):
            if best is None or hi - lo > best[1] * 2:
                best = (float(beta), float(hi - lo) / 2)
    assert best is not None, "no blank bias gives the wanted pick counts: choose other seeds"
    return best


def compare_with_oracle(got, lens, refs, cfg, what, stages=("front", "enc", "picker_logits", "picker_hidden", "picked", "helper", "text_logits")):
    """the stages of a ragged predict(stages=True, wav_lengths=lens), as NumPy arrays, against the oracle run on every utterance
    alone: lengths and counts equal, every valid row within TOL, every row past a length exactly 0 (text_argmax -1), nothing
    non-finite.  Prints every figure before it asserts; -> {stage: largest error}"""
    B = len(lens)
    T = np.array([r["front"].shape[1] for r in refs])
    cnt = np.array([int(r["counts"][0]) for r in refs])
    print("%s: T_b %s" % (what, T.tolist()))
    print("%s: counts gpu %s oracle %s" % (what, np.asarray(got["counts"]).tolist(), cnt.tolist()))
    errs, pad_bad, nonfinite = {}, {}, {}
    for k in stages:
        g = np.asarray(got[k])
        n = T if k in ("front", "enc", "picker_logits", "picker_hidden") else cnt
        nonfinite[k] = int((~np.isfinite(g)).sum())
        e, bad = 0.0, 0
        for b in range(B):
            nb = int(n[b])
            if nb:
                e = max(e, float(np.abs(g[b, :nb].astype(np.float64) - refs[b][k][0][:nb]).max()))
            bad += int(np.count_nonzero(g[b, nb:]))
        errs[k], pad_bad[k] = e, bad
        print("%s: %-14s max|gpu - oracle alone| = %.3g   nonzero padding words %d   non-finite %d" % (what, k, e, bad, nonfinite[k]))
    if "enc_lengths" in got:
        assert np.array_equal(np.asarray(got["enc_lengths"]), T), (got["enc_lengths"], T)
    assert np.array_equal(np.asarray(got["counts"]), cnt), (got["counts"], cnt)
    for k in stages:
        assert nonfinite[k] == 0, (what, k, "non-finite values")
        assert errs[k] < TOL, (what, k, errs[k])
        assert pad_bad[k] == 0, (what, k, "rows past the length are not 0")
    if "text_argmax" in got and "text_logits" in stages:
        am, lg = np.asarray(got["text_argmax"]), np.asarray(got["text_logits"])
        for b in range(B):
            c = int(cnt[b])
            assert np.array_equal(am[b, :c], lg[b, :c].argmax(-1)), (what, b, "text_argmax != argmax of the logits")
            assert (am[b, c:] == -1).all(), (what, b, "text_argmax past the count is not -1")
    return errs
