"""The dmodel-144 ragged calls with a length ON every tile, window and key-block boundary, against the float64 oracle.

Every length predicate of the ragged path compares against a per-utterance length inside a tile of 16
frames, a P.V step of 32, a depthwise-conv window of 64 or a key block of 256.  tests/test_gpu_ragged.py draws lengths that sit
mid-tile and compares with solo GPU calls only.  Here the encoder lengths are 1, 2, 3, every multiple of 16 and its two
neighbours, 255 .. 257, 511 .. 513 and the row length itself (tests/ragged_edges.py), in every parity of the SAME paddings and
every hop residue; every utterance is compared with the oracle run on that utterance alone, and the padding holds NaN.
One batch per kernel regime (csrc/block_path.hip), asserted from the launch counts of mi355asr_profile_read."""
import numpy as np
import pytest

from helpers import assert_frames_and_ids, co, maxdiff
from ragged_edges import COMBOS, HOP, L_for, edge, geometry_for, utterance, with_combos, with_fill

TOL = 1e-3                     # the project's contract against the float64 oracle
SOLO = 1e-4                    # ragged row against its solo call, relative to max(1, max|solo|): the bound of tests/test_gpu_ragged.py
SMALL_M, NS1_MAX_M, SHORT_KEYS = 48, 4096, 256     # the defaults of MI355ASR_SMALL_M, MI355ASR_NS1_MAX_M and ATTN_SPLIT_SHORT_KEYS


# ---- 1. the length constructor (host) ------------------------------------------------------------------------------------
def test_length_constructor_hits_the_geometry_it_names():
    """L_for(T, combo) has exactly the T, T1 and F it was built for, for T = 1 .. 530 and all 12 combos, and L mod hop = r mod hop"""
    from tensorflowasr_amd.models import ragged_geometry
    assert len(COMBOS) == 12 and len(set(COMBOS)) == 12
    seen = set()
    for T in range(1, 531):
        for f_odd, t1_odd, r in COMBOS:
            L = L_for(T, f_odd, t1_odd, r)
            g = ragged_geometry(L)
            want = geometry_for(T, f_odd, t1_odd, r)
            assert {k: g[k] for k in ("T", "T1", "F")} == want, (T, f_odd, t1_odd, r, L, g)
            assert g["F"] % 2 == int(f_odd) and g["T1"] % 2 == int(t1_odd) and L % HOP == r % HOP
            assert g["pt1"] == int(f_odd) and g["pt2"] == int(t1_odd)          # one zero row on top exactly when the input is odd
            assert L >= 1 and L not in seen
            seen.add(L)
    assert L_for(1, True, True, 1) == 1


# ---- the batches ---------------------------------------------------------------------------------------------------------
# name -> (Tmax, [(T_b, combo)], the T_b that also get a solo GPU call (None: all))
def _batches():
    out = {}
    for t in (1, 16, 17, 23):
        out["a-24-%d" % t] = (24, with_combos([24, t]), None)
    out["a1-40-17"] = (40, with_combos([17]), None)
    out["b-32x128"] = (128, with_combos(with_fill(edge(128), 32, 128, seed=128)), edge(128))
    out["c-33x128"] = (128, with_combos(with_fill(edge(128), 33, 128, seed=128)), edge(128))
    out["d-52x80"] = (80, with_combos(with_fill(edge(80), 52, 80, seed=80)), edge(80))
    out["e-7x528"] = (528, with_combos([528, 513, 512, 511, 257, 256, 17]), None)
    out["f-14x528"] = (528, with_combos([1, 16, 17, 255, 256, 257, 271, 272, 273, 511, 512, 513, 527, 528]), None)
    out["g-24x40"] = (40, [(T, k) for T in (17, 33) for k in range(12)], None)
    return out


BATCHES = _batches()


def test_batches_hold_the_edges_and_every_combo():
    """the batch table itself: row counts on the regime thresholds, every edge member present, every combo in every batch of 12
    or more, fill lengths outside the edge set and without repetition"""
    rows = {k: len(u) * Tmax for k, (Tmax, u, _) in BATCHES.items()}
    assert rows == {"a-24-1": 48, "a-24-16": 48, "a-24-17": 48, "a-24-23": 48, "a1-40-17": 40, "b-32x128": 4096, "c-33x128": 4224,
                    "d-52x80": 4160, "e-7x528": 3696, "f-14x528": 7392, "g-24x40": 960}
    assert edge(80) == [1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80]
    assert edge(128)[-4:] == [112, 113, 127, 128]
    assert len(edge(128)) == 26 and 129 not in edge(128)
    for name, (Tmax, utts, solo) in BATCHES.items():
        Ts = [t for t, _ in utts]
        assert max(Ts) <= Tmax and min(Ts) >= 1
        assert len(set(utts)) == len(utts)
        if len(utts) >= 12:
            assert {k for _, k in utts} == set(range(12)), name
        if solo is not None:
            assert Ts[:len(solo)] == solo and not set(Ts[len(solo):]) & set(solo) and len(set(Ts)) == len(Ts), name
        L = _row_samples(Tmax, utts)
        assert max(L_for(t, *COMBOS[k]) for t, k in utts) <= L
    # b's utterances are c's first 32: the oracle and solo results are shared
    assert BATCHES["c-33x128"][1][:32] == BATCHES["b-32x128"][1]


def _row_samples(Tmax, utts):
    """the batch is padded to L_for(Tmax, combo 0), the longest sample count of Tmax frames with a one-sample last frame -- or to
    its longest utterance where that is longer"""
    return max([L_for(Tmax, *COMBOS[0])] + [L_for(t, *COMBOS[k]) for t, k in utts])


# ---- shared state: one model, one oracle result and one solo result per utterance --------------------------------------------
_STATE = {}
_ORACLE = {}
_SOLO = {}


def _np(t):
    return t.cpu().numpy()


def _model():
    if "m" not in _STATE:
        from caller_contract_gpu_steps import conformer_ctc
        _STATE["m"] = conformer_ctc()                     # small_cfg(2), V = 50, the seeded oracle weights of test_gpu_ragged._model()
    return _STATE["m"]


def _oracle(wav):
    """float64 encoder output [T, 144] and logits [T, 50] of one utterance alone, computed once per module"""
    key = len(wav)
    if key not in _ORACLE:
        _, w, cfg = _model()
        e = co.conformer_encoder(wav[None].astype(np.float64), w, cfg)
        _ORACLE[key] = (e[0], co.ctc_decoder(e, w, cfg)[0])
    return _ORACLE[key]


def _solo(wav):
    """the calls without lengths on the utterance alone: (enc, logits, ids as a list)"""
    key = len(wav)
    if key not in _SOLO:
        m = _model()[0]
        enc = m.encode(wav[None])
        lg = m.ctc_logits(enc)
        ids, ol = m.recognize(wav[None])
        _SOLO[key] = (_np(enc)[0], _np(lg)[0], _np(ids)[0, :int(_np(ol)[0])].tolist())
    return _SOLO[key]


def _padded(Tmax, utts):
    from caller_contract_gpu_steps import nan_tail
    items = [utterance(t, k) for t, k in utts]
    lens = np.array([len(it) for it in items], np.int32)
    x = np.zeros((len(items), _row_samples(Tmax, utts)), np.float32)
    for b, it in enumerate(items):
        x[b, :len(it)] = it
    x = nan_tail(x, lens)
    assert np.isnan(x).sum() == x.size - int(lens.sum())
    return items, x, lens


def _assert_regime(name, c, B, T):
    """the launch counts of the ragged encoder call say which kernels ran, as far as they can (caller_contract_gpu_steps.
    step_encoder144): K_FFN only on the layer-at-a-time path; on the fused paths an attention launch of its own exactly when the
    rows pass MI355ASR_NS1_MAX_M = 4096 (fused_pp) or the keys pass 256 (attention_split_long_kernel), and no depthwise-conv /
    out-projection launch when the pp block folds the conv.  What they cannot tell is asserted from the row count against the
    defaults 48, 4096 and 256: fused_ns against fused_pp in batch e (both launch attention), and the short against the long
    attention kernel."""
    from caller_contract_gpu_steps import K_ATTN, K_DWCONV, K_FF1_QKV, K_FFN, K_OUT_GLU, K_TAIL_FF1, K_TAIL_FF2
    M = B * T
    if name.startswith("a"):
        assert M <= SMALL_M and c[K_FFN] > 0 and c[K_FF1_QKV] == 0 and c[K_TAIL_FF1] + c[K_TAIL_FF2] == 0, ("layer-at-a-time", M, c)
        return
    assert M > SMALL_M and c[K_FFN] == 0 and c[K_FF1_QKV] > 0 and c[K_TAIL_FF1] + c[K_TAIL_FF2] > 0, ("fused", M, c)
    assert (c[K_ATTN] == 0) == (M <= NS1_MAX_M and T <= SHORT_KEYS), ("attention of its own launch", M, T, c)
    kind = name[0]
    if kind in "bg":                   # fused_ns, ns1_attention inside the first launch
        assert M <= NS1_MAX_M and T <= SHORT_KEYS and c[K_ATTN] == 0, (name, M, c)
    elif kind == "c":                  # fused_pp, depthwise conv folded, short attention kernel
        assert M > NS1_MAX_M and T <= SHORT_KEYS and c[K_ATTN] > 0 and c[K_DWCONV] == 0 and c[K_OUT_GLU] == 0, (name, M, c)
    elif kind == "d":                  # fused_pp, depthwise conv in a launch of its own
        assert M > NS1_MAX_M and T <= SHORT_KEYS and c[K_ATTN] > 0 and c[K_DWCONV] > 0, (name, M, c)
    elif kind == "e":                  # fused_ns rows, long attention in a launch of its own (row count and T only)
        assert M <= NS1_MAX_M and T > SHORT_KEYS and c[K_ATTN] > 0, (name, M, c)
    elif kind == "f":                  # fused_pp, folded depthwise conv over 9 windows, long attention
        assert M > NS1_MAX_M and T > SHORT_KEYS and c[K_ATTN] > 0 and c[K_DWCONV] == 0 and c[K_OUT_GLU] == 0, (name, M, c)
    else:
        raise AssertionError(name)


def _run(name):
    """the three ragged calls of one batch, once per module: everything on the host"""
    if name not in _STATE:
        from caller_contract_gpu_steps import profile_counts
        m = _model()[0]
        Tmax, utts, _ = BATCHES[name]
        items, x, lens = _padded(Tmax, utts)
        assert m.out_frames(x.shape[1]) == Tmax
        counts = profile_counts(m._h, lambda: m.encode(x, lengths=lens))
        enc, el = m.encode(x, lengths=lens)
        lg, am = m.ctc_logits(enc, return_argmax=True, lengths=el)
        ids, ol = m.recognize(x, wav_lengths=lens)
        _STATE[name] = dict(items=items, x=x, lens=lens, counts=counts, enc=_np(enc), el=_np(el), lg=_np(lg), am=_np(am), ids=_np(ids),
                            ol=_np(ol))
    return _STATE[name]


# ---- 2. encoder, logits and ids at edge lengths, in every kernel regime -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_edge_lengths_against_the_oracle(name):
    """per utterance of the batch: enc_lengths == T_b; encoder rows and logits within 1e-3 of the float64 oracle on wav[b, :L_b]
    alone; frame arg-max and recognize(wav_lengths) ids equal to the oracle's (assert_frames_and_ids, at most 0.5 % of the
    utterance's frames excused); rows past T_b exactly 0 / -1 and no NaN anywhere although the wav padding is NaN; edge members
    within 1e-4 (relative) of the solo call with equal ids.  The regime is asserted from the launch counts."""
    Tmax, utts, solo_Ts = BATCHES[name]
    m = _model()[0]
    r = _run(name)
    B = len(utts)
    _assert_regime(name, r["counts"], B, Tmax)
    enc, el, lg, am, ids, ol = (r[k] for k in ("enc", "el", "lg", "am", "ids", "ol"))
    assert enc.shape == (B, Tmax, 144) and lg.shape == (B, Tmax, 50) and am.shape == ids.shape == (B, Tmax)
    assert not np.isnan(enc).any() and not np.isnan(lg).any()
    assert el.tolist() == [t for t, _ in utts]
    worst = dict(enc=0.0, logits=0.0, solo_enc=0.0, solo_logits=0.0)
    for b, ((T, k), wav) in enumerate(zip(utts, r["items"])):
        e64, l64 = _oracle(wav)
        assert e64.shape[0] == T
        err = maxdiff(enc[b, :T], e64)
        assert err < TOL, (name, b, T, k, err)
        worst["enc"] = max(worst["enc"], err)
        lerr, _ = assert_frames_and_ids(lg[b:b + 1, :T], am[b:b + 1, :T], ids[b:b + 1, :T], ol[b:b + 1], l64[None], [T], m.blank,
                                        tag="%s row %d (T %d, combo %d)" % (name, b, T, k))
        worst["logits"] = max(worst["logits"], lerr)
        assert not enc[b, T:].any() and not lg[b, T:].any() and (am[b, T:] == -1).all(), (name, b, T)
        assert 0 <= ol[b] <= T and (ids[b, ol[b]:] == -1).all(), (name, b, T)
        if solo_Ts is None or T in solo_Ts:
            senc, slg, sids = _solo(wav)
            assert senc.shape[0] == T
            for what, got, ref in (("solo_enc", enc[b, :T], senc), ("solo_logits", lg[b, :T], slg)):
                rel = maxdiff(got, ref) / max(1.0, float(np.abs(ref).max()))
                assert rel < SOLO, (name, what, b, T, k, rel)
                worst[what] = max(worst[what], rel)
            assert ids[b, :ol[b]].tolist() == sids, (name, b, T, k)
    print("%s: %d x %d, worst |enc - oracle| %.3g, |logits - oracle| %.3g, against solo %.3g / %.3g (relative)"
          % (name, B, Tmax, worst["enc"], worst["logits"], worst["solo_enc"], worst["solo_logits"]))


# ---- 3. recognize_ragged with in_len ---------------------------------------------------------------------------------------------
def _centred_head_model():
    """the same model with the class head's bias moved by minus the oracle's mean logits of batch b's longest utterance.  With
    the seeded weights every frame of every utterance decides for class 1 (the bias term dominates: the oracle's mean logits
    lead by 1.2, the frames vary by 0.2), so the greedy ids are [1] whatever the collapse does; centred, the frames of an utterance
    spread over all 50 classes with repeats and blanks, and a collapse that stops one frame early or late returns other ids"""
    if "centred" not in _STATE:
        from caller_contract_gpu_steps import conformer_ctc
        Tmax, utts, _ = BATCHES["b-32x128"]
        _, l64 = _oracle(utterance(*[u for u in utts if u[0] == Tmax][0]))
        m, w, _ = conformer_ctc()
        w = dict(w)
        w["fully_connected/bias"] = (w["fully_connected/bias"].astype(np.float64) - l64.mean(0)).astype(np.float32)
        m.load_weights(w, by_name=False)
        _STATE["centred"] = m
    return _STATE["centred"]


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["seeded", "centred"])
def test_recognize_ragged_with_input_length(head):
    """batch b with input_length 1, T_b - 1, T_b, T_b + 5 and Tmax cycled over the rows: the ids are exactly co.ctc_collapse of the
    call's own frame arg-max cut at min(T_b, in_len[b]); from in_len = T_b on the row is the call's without in_len, bit for bit.
    Once with the seeded model of the other tests, whose ids are [1] for every row, and once with its class head centred
    (_centred_head_model), where the rows hold up to T_b ids and every cut changes them."""
    name = "b-32x128"
    Tmax, utts, _ = BATCHES[name]
    r = _run(name)
    if head == "seeded":
        m, am, ids0, ol0 = _model()[0], r["am"], r["ids"], r["ol"]
    else:
        m = _centred_head_model()
        enc, el = m.encode(r["x"], lengths=r["lens"])
        assert np.array_equal(_np(enc), r["enc"])                          # the encoder is the same
        am = _np(m.ctc_logits(enc, return_argmax=True, lengths=el)[1])
        ids0, ol0 = (_np(t) for t in m.recognize(r["x"], wav_lengths=r["lens"]))
        assert len(np.unique(am[am >= 0])) >= 25 and (am == m.blank).any()
    Ts = np.array([T for T, _ in utts])
    il = np.array([(1, T - 1, T, T + 5, Tmax)[b % 5] for b, T in enumerate(Ts)], np.int32)
    assert (il < Ts).any() and (il == Ts).any() and (il > Ts).any()
    ids, ol = (_np(t) for t in m.recognize(r["x"], input_length=il, wav_lengths=r["lens"]))
    cut = 0
    for b, T in enumerate(Ts):
        assert (am[b, T:] == -1).all()
        for got, gl, n in ((ids0, ol0, T), (ids, ol, min(T, int(il[b])))):
            rid, rlen = co.ctc_collapse(am[b:b + 1, :T], [n], m.blank)
            assert gl[b] == rlen[0] and got[b, :gl[b]].tolist() == rid[0, :rlen[0]].tolist() and (got[b, gl[b]:] == -1).all(), (b, T, n)
        if il[b] >= T:
            assert np.array_equal(ids[b], ids0[b]) and ol[b] == ol0[b], (b, T, il[b])
        cut += int(ol[b] < ol0[b])
    if head == "centred":
        assert cut >= 8 and ol0.max() > 64, "the centred head should give long id rows that the cuts shorten"


# ---- 4. Translator at dmodel 144, token and encoder edges ---------------------------------------------------------------------
TOKEN_EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48]
ENC_EDGES = [1, 15, 16, 17, 32, 33, 255, 256, 257, 271, 272]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [30, 90])
def test_translator_token_and_encoder_edges(B):
    """U = 48, T = 272; token lengths cycle through TOKEN_EDGES and encoder lengths through ENC_EDGES with stride 3 (10 and 11
    are coprime to it and to each other: B rows are B different pairs), row 0 is (U, T); encoder rows past enc_len hold NaN, token
    ids past token_len are random valid ids.  30 x 48 = 1 440 rows run the small-batch kernels and 90 x 48 = 4 320 the
    pair-pipelined ones (the row count against MI355ASR_NS1_MAX_M = 4096: the launch counts are the same).  Per row:
    logits[b, :U_b] within 1e-3 of co.translator in float64 on its own tokens and frames and within 1e-4 (relative) of the solo
    call, arg-max equal to the solo call's, rows past U_b 0 / -1, no NaN anywhere."""
    from caller_contract_gpu_steps import nan_tail
    from test_gpu_ragged import _translator
    U, T = 48, 272
    assert (B * U > NS1_MAX_M) == (B == 90)
    t = _translator()
    w = t.get_weights_dict()
    cfg = dict(co.CONFORMER_S, translator_num_blocks=2, translator_fc_factor=0.5, translator_kernel_size=32)
    rng = np.random.default_rng(1000 + B)
    tl = np.array([TOKEN_EDGES[b % 10] for b in range(B)], np.int32)
    el = np.array([ENC_EDGES[(3 * b) % 11] for b in range(B)], np.int32)
    tl[0], el[0] = U, T
    assert set(tl.tolist()) == set(TOKEN_EDGES) and set(el.tolist()) == set(ENC_EDGES)
    assert len({(a, b) for a, b in zip(tl.tolist()[1:], el.tolist()[1:])}) == B - 1
    ids = rng.integers(0, 60, size=(B, U)).astype(np.int32)
    enc = nan_tail(rng.standard_normal((B, T, 144)).astype(np.float32), el)
    lg, am = t([ids, enc], return_argmax=True, token_lengths=tl, enc_lengths=el)
    lg, am = _np(lg), _np(am)
    assert not np.isnan(lg).any()
    worst = [0.0, 0.0]
    for b in range(B):
        Ub, Tb = int(tl[b]), int(el[b])
        ref = co.translator(ids[b:b + 1, :Ub], enc[b:b + 1, :Tb].astype(np.float64), w, cfg)[0]
        err = maxdiff(lg[b, :Ub], ref)
        assert err < TOL, (b, Ub, Tb, err)
        slg, sam = t([ids[b:b + 1, :Ub], enc[b:b + 1, :Tb]], return_argmax=True)
        slg, sam = _np(slg)[0], _np(sam)[0]
        rel = maxdiff(lg[b, :Ub], slg) / max(1.0, float(np.abs(slg).max()))
        assert rel < SOLO, (b, Ub, Tb, rel)
        assert np.array_equal(am[b, :Ub], sam), (b, Ub, Tb)
        assert not lg[b, Ub:].any() and (am[b, Ub:] == -1).all(), (b, Ub, Tb)
        worst = [max(worst[0], err), max(worst[1], rel)]
    print("translator %d x %d x %d: worst |logits - oracle| %.3g, against solo %.3g (relative)" % (B, U, T, worst[0], worst[1]))
