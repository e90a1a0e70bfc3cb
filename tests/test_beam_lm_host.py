"""The n-gram scorer of the CTC prefix beam search on the host: the ARPA reader, `mi355asr_lm_score`, the host search and the
stateful decoder with a scorer against the reference's own decoder (tests/golden/beam_lm_kat.npz: orders 3 and 4, recorded by
tests/golden/make_beam_lm_golden.py from the reference's unmodified sources; tests/golden/beam_lm_orders_kat.npz: orders 1, 2,
5, 6 and an order-6 model too wide for packed table keys, at the beam widths where the device search changes kernels, recorded
by make_beam_lm_orders_golden.py), and the Python surface.  No GPU."""
import ctypes
import gzip
import json
import os
import shutil

import numpy as np
import pytest

import ngram_yardstick as ny
from helpers import ROOT
from tensorflowasr_amd import ngram
from tensorflowasr_amd.models import BeamDecoder, ctc_prefix_beam_decode

GOLDEN = os.path.join(ROOT, "tests", "golden")
K = np.load(os.path.join(GOLDEN, "beam_lm_kat.npz"))
VOCAB = json.loads(str(K["vocabulary"]))
KO = np.load(os.path.join(GOLDEN, "beam_lm_orders_kat.npz"))
assert json.loads(str(KO["vocabulary"])) == VOCAB
ARPA = {3: os.path.join(GOLDEN, "lm_small.arpa"), 4: os.path.join(GOLDEN, "lm_small4.arpa"), 1: os.path.join(GOLDEN, "lm_small1.arpa"),
        2: os.path.join(GOLDEN, "lm_small2.arpa"), 5: os.path.join(GOLDEN, "lm_small5.arpa"), 6: os.path.join(GOLDEN, "lm_small6.arpa"),
        "w6": os.path.join(GOLDEN, "lm_wide6.arpa")}
MODELS = [3, 4, 1, 2, 5, 6, "w6"]                                       # a model's name in the fixtures is str() of these
_scorers = {}


def order_of(model):
    return 6 if model == "w6" else model


def fixture_of(model):
    return K if model in (3, 4) else KO


def scorer(order, alpha=1.0, beta=0.0):
    if order not in _scorers:
        _scorers[order] = ngram.NGramScorer(alpha, beta, ARPA[order], VOCAB)
    s = _scorers[order]
    s.alpha, s.beta = float(alpha), float(beta)
    return s


# ---- ARPA reader -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_arpa_reader_round_trips_the_fixture(model, tmp_path):
    order = order_of(model)
    m = ngram.read_arpa(ARPA[model])
    o, counts, grams = ny.parse_arpa(ARPA[model])                       # the direct parse
    assert m.order == o == order and m.counts == [counts[k] for k in range(1, o + 1)]
    if model == "w6":
        assert len(m.words) >= 2100 and len(m.words).bit_length() * order > 64
    else:
        assert 150 <= len(m.words) <= 250 and sum(m.counts) >= (2000 if model in (3, 4) else len(m.words))
    assert all(c > 0 for c in m.counts)
    for k in range(1, o + 1):
        assert len(grams[k]) == m.counts[k - 1]
        for row, lp, bo in zip(m.ids[k - 1].tolist(), m.logp[k - 1], m.backoff[k - 1]):
            e = grams[k][tuple(m.words[i - 1] for i in row)]
            assert lp == np.float32(e[0]) and bo == np.float32(e[1] or 0.0)
    gz = tmp_path / "lm.arpa.gz"
    with open(ARPA[model], "rb") as f, gzip.open(gz, "wb") as g:
        shutil.copyfileobj(f, g)
    z = ngram.read_arpa(str(gz))
    assert z.words == m.words and z.counts == m.counts
    for k in range(o):
        assert np.array_equal(z.ids[k], m.ids[k]) and np.array_equal(z.logp[k], m.logp[k]) and np.array_equal(z.backoff[k], m.backoff[k])


def test_arpa_reader_refuses_truncated_and_miscounted_files(tmp_path):
    lines = open(ARPA[3], encoding="utf-8").read().split("\n")
    cut = tmp_path / "cut.arpa"
    cut.write_text("\n".join(lines[:len(lines) // 2]), encoding="utf-8")
    with pytest.raises(ngram.ArpaError, match=r"line \d+"):
        ngram.read_arpa(str(cut))
    i = next(j for j, ln in enumerate(lines) if ln.startswith("ngram 2="))
    wrong = list(lines)
    wrong[i] = "ngram 2=%d" % (int(lines[i].split("=")[1]) + 1)
    mis = tmp_path / "mis.arpa"
    mis.write_text("\n".join(wrong), encoding="utf-8")
    with pytest.raises(ngram.ArpaError, match=r"line \d+.*declares"):
        ngram.read_arpa(str(mis))
    j = next(j for j, ln in enumerate(lines) if ln.startswith("\\2-grams")) + 3
    broken = list(lines)
    broken[j] = "not-a-number " + broken[j].split("\t", 1)[1]
    bad = tmp_path / "bad.arpa"
    bad.write_text("\n".join(broken), encoding="utf-8")
    with pytest.raises(ngram.ArpaError, match=r"line %d" % (j + 1)):
        ngram.read_arpa(str(bad))


def test_word_based_model_is_refused(tmp_path):
    p = tmp_path / "words.arpa"
    p.write_text("\\data\\\nngram 1=4\n\n\\1-grams:\n-1.0\t<unk>\n-99\t<s>\n-1.0\t</s>\n-1.0\thello\n\n\\end\\\n", encoding="utf-8")
    with pytest.raises(NotImplementedError, match="dictionary FST"):
        ngram.NGramScorer(1.0, 0.0, str(p), ["h", "e", "l", "o"])


# ---- get_log_cond_prob / mi355asr_lm_score -----------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_lm_score_equals_the_reference_scorer(model):
    order, F = order_of(model), fixture_of(model)
    s = scorer(model)
    q = json.loads(str(F["ngram_queries"]))[str(model)]
    ref = F["cond_%s" % model]
    assert len(ref) == len(q["ngrams"]) >= 200
    assert s.is_character_based() and s.get_max_order() == order and s.get_dict_size() == 0
    assert (ref == -1000.0).any() and (ref != -1000.0).any()
    full = [i for i, g in enumerate(q["ngrams"]) if len(g) == order]
    assert len(full) >= len(ref) - 2
    for g, r in zip(q["ngrams"], ref):
        assert s.get_log_cond_prob(g) == r, g                           # exactly: the float KenLM returns, widened
    ids = np.array([[s.word_id(w) for w in q["ngrams"][i]] for i in full], np.int32)
    lib = s.score_ids(ids)
    assert lib.dtype == np.float32 and np.array_equal(lib.astype(np.float64), ref[full])
    assert len(q["sentences"]) == len(F["sent_%s" % model]) >= 10
    for words, r in zip(q["sentences"], F["sent_%s" % model]):
        assert s.get_sent_log_prob(words) == r, words


@pytest.mark.parametrize("model", MODELS)
def test_lm_score_against_the_float64_yardstick(model):
    order = order_of(model)
    s = scorer(model)
    y = ny.BackoffLM(ARPA[model])
    rng = np.random.default_rng(order + 10 * (model == "w6"))
    n_words = len(s.model.words)
    ids = rng.integers(1, n_words + 1, size=(3000, order)).astype(np.int32)
    seen = np.concatenate([np.pad(s.model.ids[k], ((0, 0), (order - 1 - k, 0)), constant_values=s.bos_word) for k in range(order)])
    ids = np.concatenate([ids, seen[rng.choice(len(seen), min(1500, len(seen)), replace=False)]])
    ids[rng.choice(len(ids), 50, replace=False), rng.integers(order, size=50)] = 0      # OOV somewhere
    got = s.score_ids(ids)
    unk = s.model.word_to_id["<unk>"]
    worst = backed = 0.0
    for row, g in zip(ids.tolist(), got):
        words = ["<oov>" if i in (0, unk) else s.model.words[i - 1] for i in row]
        want, terms = y.cond(words)
        if unk in row:
            continue                                                    # the library takes ids: "<unk>" is word 0 there
        # float32 rounding: each of the k terms is read with a relative error of 2^-24, and each of the k - 1 additions rounds a
        # partial sum that is at most sum|terms| by 2^-24
        margin = len(terms) * sum(abs(t) for t in terms) * 2.0 ** -24
        assert abs(float(g) - want) <= margin, (words, float(g), want, terms)
        worst = max(worst, abs(float(g) - want))
        backed += len(terms) > 1
    print("model %s: %d n-grams, %d backed off, max |lib - float64| = %.3g" % (model, len(ids), backed, worst))
    assert backed > 1000 if order > 1 else backed == 0                   # a unigram model has nothing to back off from


def test_hashed_keys_for_models_too_wide_to_pack():
    """9 000 words at order 5 need 70 bits: the table keys are 64-bit hashes of the ids instead of the ids themselves"""
    chars = [chr(0x4E00 + i) for i in range(9000)]
    m = ngram.synthetic_model(chars, 3000, 3000, seed=3, higher=(2000, 1000))
    s = ngram.NGramScorer(1.0, 0.0, "synthetic", chars[:50], model=m)
    assert m.order == 5 and len(m.words).bit_length() * 5 > 64
    rng = np.random.default_rng(0)
    rows = [np.pad(m.ids[k][:600], ((0, 0), (4 - k, 0)), constant_values=s.bos_word) for k in range(5)]
    ext = m.ids[3][:800]
    rows.append(np.concatenate([rng.integers(4, 9000, (len(ext), 1)).astype(np.int32), ext], 1))      # a 4-gram behind an unseen word
    rows.append(np.concatenate([m.ids[2][:800], rng.integers(4, 9000, (800, 2)).astype(np.int32)], 1))
    ids = np.concatenate(rows)
    got = s.score_ids(ids)
    unk, n = s.model.word_to_id["<unk>"], 0
    for row, g in zip(ids.tolist(), got):
        if unk not in row:                                              # the library takes ids: "<unk>" is word 0 there
            assert s.get_log_cond_prob([m.words[i - 1] for i in row]) == float(g), row
            n += 1
    assert n > 4000


class _LmView(ctypes.Structure):
    """LmView of csrc/lm_table.h"""
    _fields_ = [("cells", ctypes.c_void_p), ("shift", ctypes.c_uint32), ("mask", ctypes.c_uint32), ("order", ctypes.c_int32),
                ("bits", ctypes.c_int32), ("bos", ctypes.c_int32)]


@pytest.mark.parametrize("model", MODELS)
def test_table_key_mode_of_every_fixture_model(model):
    """the wide model's table really is in hashed mode (bits = 0), the others keep their word ids in the key"""
    from tensorflowasr_amd import _lib
    fn = _lib.lib().mi355asr_lm_host_view
    fn.restype, fn.argtypes = ctypes.POINTER(_LmView), [ctypes.c_void_p]
    s = scorer(model)
    v = fn(s.handle()).contents
    n_words = len(s.model.words)
    assert v.order == order_of(model) and v.bos == s.bos_word and v.mask + 1 >= 2 * sum(s.model.counts)
    if model == "w6":
        assert v.bits == 0 and n_words.bit_length() * v.order > 64
    else:
        assert v.bits == n_words.bit_length() and v.bits * v.order <= 64


# ---- the searches ------------------------------------------------------------------------------------------------------
def _check(ids, lens, sc, n, ref_ids, ref_lens, ref_sc, what, live_only=False):
    """scores bit for bit; hypotheses exactly where the reference specifies them (no tied scores), else as test_host.py treats
    beam_long_kat.npz: which of several prefixes of equal score survives is left to std::nth_element there.
    live_only (the orders fixture, whose cutoff_top_n 1 and 2 cases fill the beam with prefixes that lost ALL their probability:
    score -FLT_MAX, every one tied with every other): a rank whose score no other rank shares holds the reference's hypothesis,
    and the nine-tenths overlap is asked of the hypotheses that still have a probability."""
    nn = len(ref_sc)
    assert n == nn, what
    assert np.array_equal(sc[:nn].astype(np.float64), ref_sc), what
    ours = [tuple(ids[j, :lens[j]]) for j in range(nn)]
    ref = [tuple(ref_ids[j, :ref_lens[j]]) for j in range(nn)]
    assert len(set(ours)) == nn, what
    tied = np.array([(ref_sc == v).sum() > 1 for v in ref_sc])
    if not tied.any():
        assert ours == ref and np.array_equal(lens[:nn], ref_lens), what
    if live_only:
        assert all(ours[j] == ref[j] for j in range(nn) if not tied[j]), what
        live = ref_sc > -np.finfo(np.float32).max
        assert len(set(o for o, a in zip(ours, live) if a) & set(r for r, a in zip(ref, live) if a)) >= 0.9 * live.sum(), what
    else:
        assert len(set(ours) & set(ref)) >= 0.9 * nn, what
    return not tied.any()


def test_host_search_reproduces_the_reference_with_a_scorer():
    meta = json.loads(str(K["meta"]))
    assert {m["beam"] for m in meta} >= {1, 4, 16, 100} and {m["cutoff_prob"] for m in meta} == {1.0, 0.99}
    assert {m["cutoff_top_n"] for m in meta} == {8, 40} and {m["order"] for m in meta} == {3, 4}
    assert any(m["alpha"] == 0 for m in meta) and any(m["beta"] < 0 for m in meta) and sum(m["T"] >= 400 for m in meta) >= 3
    exact = 0
    for i, m in enumerate(meta):
        s = scorer(m["order"], m["alpha"], m["beta"])
        ids, lens, sc, n = ctc_prefix_beam_decode(K["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"],
                                                  num_threads=1, ext_scorer=s)
        exact += _check(ids[0], lens[0], sc[0], n[0], K["ids_%d" % i], K["lens_%d" % i], K["scores_%d" % i], "case %d %s" % (i, m))
        if m["differs_from_scorerless"]:
            i0, l0, _, _ = ctc_prefix_beam_decode(K["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], num_threads=1)
            assert tuple(i0[0, 0, :l0[0, 0]]) != tuple(ids[0, 0, :lens[0, 0]]), i
    assert exact >= 10


def _orders_cases(model):
    return [(i, m) for i, m in enumerate(json.loads(str(KO["meta"]))) if m["model"] == str(model)]


def test_orders_fixture_holds_the_cases_it_is_for():
    meta = json.loads(str(KO["meta"]))
    pruned = [m for m in meta if m["cutoff_prob"] < 1.0]
    assert {m["model"] for m in meta} == {"1", "2", "5", "6", "w6"} and {m["order"] for m in meta} == {1, 2, 5, 6}
    assert {m["beam"] for m in pruned} >= {1, 2, 15, 16, 17, 64, 65, 127, 128} and {m["cutoff_top_n"] for m in pruned} >= {1, 2, 15, 40}
    assert sum(m["cutoff_prob"] == 1.0 for m in meta) >= 2 and sum(m["T"] >= 400 and m["order"] == 6 for m in meta) >= 2
    assert any(m["order"] >= 5 and m["longest"] >= 6 for m in meta)      # every age of the history holds a real word somewhere
    for name in ("1", "2", "5", "6", "w6"):
        mine = [m for m in meta if m["model"] == name]
        assert any(m["alpha"] > 0 for m in mine) and any(m["alpha"] == 0 and m["beta"] == 0 for m in mine)
        assert 2 * sum(m["differs_from_scorerless"] for m in mine if m["alpha"] > 0) >= sum(m["alpha"] > 0 for m in mine)
    short = [m for m in meta if m["T"] <= 100]
    assert 3 * sum(not m["tied"] for m in short) >= 2 * len(short)
    assert sorted(m["order"] for m in json.loads(str(KO["stateful_meta"]))) == [1, 2, 5, 6]


@pytest.mark.parametrize("model", [1, 2, 5, 6, "w6"])
def test_host_search_reproduces_the_reference_at_the_other_orders_and_widths(model):
    cases = _orders_cases(model)
    assert len(cases) >= 15
    exact = 0
    for i, m in cases:
        s = scorer(model, m["alpha"], m["beta"])
        assert s.get_max_order() == m["order"] and os.path.basename(ARPA[model]) == m["arpa"]
        ids, lens, sc, n = ctc_prefix_beam_decode(KO["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"],
                                                  num_threads=1, ext_scorer=s)
        exact += _check(ids[0], lens[0], sc[0], n[0], KO["ids_%d" % i], KO["lens_%d" % i], KO["scores_%d" % i], "case %d %s" % (i, m), live_only=True)
        if m["differs_from_scorerless"]:
            i0, l0, _, _ = ctc_prefix_beam_decode(KO["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], num_threads=1)
            assert tuple(i0[0, 0, :l0[0, 0]]) != tuple(ids[0, 0, :lens[0, 0]]), i
    assert 3 * exact >= 2 * len(cases)


def test_stateful_decoder_with_a_scorer_fed_in_pieces():
    _stateful_in_pieces(K)


def test_stateful_decoder_at_orders_1_2_5_6_fed_in_pieces():
    _stateful_in_pieces(KO)


def _stateful_in_pieces(F):
    K = F
    for k, m in enumerate(json.loads(str(K["stateful_meta"]))):
        s = scorer(m["order"], m["alpha"], m["beta"])
        p = K["st_probs_%d" % k]
        d = BeamDecoder(VOCAB + ["<blank>"], m["beam"], m["cutoff_prob"], m["cutoff_top_n"], ext_scorer=s)     # no longer raises
        t0 = 0
        for j, nt in enumerate(m["pieces"]):
            res = d.decode_ids(p[t0:t0 + nt])
            t0 += nt
            ref_sc = K["st_scores_%d_%d" % (k, j)]
            ids = np.full((len(res), max(1, max(len(t) for _, t in res))), -1, np.int32)
            for r, (_, t) in enumerate(res):
                ids[r, :len(t)] = t
            _check(ids, np.array([len(t) for _, t in res], np.int32), np.array([x for x, _ in res], np.float32), len(res),
                   K["st_ids_%d_%d" % (k, j)], K["st_lens_%d_%d" % (k, j)], ref_sc, "stateful %d piece %d" % (k, j), live_only=F is KO)
        one = ctc_prefix_beam_decode(p[None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], num_threads=1, ext_scorer=s)
        assert [x for x, _ in res] == one[2][0, :one[3][0]].tolist()
        assert [t for _, t in res] == [one[0][0, j, :one[1][0, j]].tolist() for j in range(one[3][0])]
        text = d.decode(np.zeros((0, len(VOCAB) + 1), np.float32))
        assert text[0][1] == "".join(VOCAB[t] for t in res[0][1])


def test_ext_scorer_none_is_the_existing_search():
    k = np.load(os.path.join(GOLDEN, "beam_kat.npz"))
    for i, m in enumerate(json.loads(str(k["meta"]))):
        ids, lens, sc, n = ctc_prefix_beam_decode(k["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"],
                                                  num_threads=1, ext_scorer=None)
        assert n[0] == m["n"] and np.array_equal(lens[0, :m["n"]], k["lens_%d" % i]) and np.array_equal(ids[0, :m["n"]], k["ids_%d" % i])
        assert np.array_equal(sc[0, :m["n"]].astype(np.float64), k["scores_%d" % i])


def test_reset_params_takes_effect():
    p = K["probs_3"][None]
    s = scorer(3, 1.2, 0.3)
    a = ctc_prefix_beam_decode(p, None, 16, 0.99, 40, num_threads=1, ext_scorer=s)
    s.reset_params(0.0, 0.0)
    assert (s.alpha, s.beta) == (0.0, 0.0)
    b = ctc_prefix_beam_decode(p, None, 16, 0.99, 40, num_threads=1, ext_scorer=s)
    s.reset_params(1.2, 0.3)
    assert s.alpha == float(np.float32(1.2))                             # scorer.h:63 takes floats
    s.alpha, s.beta = 1.2, 0.3
    c = ctc_prefix_beam_decode(p, None, 16, 0.99, 40, num_threads=1, ext_scorer=s)
    assert not np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a, c))


def test_text_featurizer_builds_the_scorer_from_lm_config(tmp_path):
    from tensorflowasr_amd.featurizers import TextFeaturizer
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join("[SPACE]" if v == " " else v for v in VOCAB) + "\n", encoding="utf-8")
    cfg = {"vocabulary": str(vocab), "blank_at_zero": False, "beam_width": 4,
           "lm_config": {"lm_path": ARPA[3], "alpha": 1.2, "beta": 0.3}}
    tf = TextFeaturizer(cfg)
    assert isinstance(tf.scorer, ngram.NGramScorer) and (tf.scorer.alpha, tf.scorer.beta) == (1.2, 0.3)
    assert tf.scorer.vocabulary == VOCAB and tf.num_classes == len(VOCAB) + 1
    assert TextFeaturizer({"vocabulary": str(vocab), "blank_at_zero": False, "beam_width": 1}).scorer is None
    i = 3
    m = json.loads(str(K["meta"]))[i]
    tf.scorer.alpha, tf.scorer.beta = m["alpha"], m["beta"]
    ids, lens, sc, n = ctc_prefix_beam_decode(K["probs_%d" % i][None], None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"],
                                              num_threads=1, ext_scorer=tf.scorer)
    assert np.array_equal(sc[0, :n[0]].astype(np.float64), K["scores_%d" % i])


def test_make_ngram_keeps_the_space_quirk():
    s = scorer(3)
    a, b = 5, 9
    assert s.make_ngram([a]) == ["<s>", "<s>", VOCAB[a]] and s.make_ngram([b, a, b]) == [VOCAB[b], VOCAB[a], VOCAB[b]]
    assert s.make_ngram([b, 0, a]) == ["", "", VOCAB[a]]                # every slot from the first space backwards is empty
    assert s.get_log_cond_prob(s.make_ngram([b, 0, a])) == ngram.OOV_SCORE
    assert s.get_log_cond_prob(s.make_ngram([b, a])) > -100
