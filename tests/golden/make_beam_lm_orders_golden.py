"""Generator of the n-gram scorer's fixtures at the orders and beam widths beam_lm_kat.npz leaves out: tests/golden/
lm_small1.arpa, lm_small2.arpa, lm_small5.arpa, lm_small6.arpa (orders 1, 2, 5, 6 over the vocabulary of lm_small.arpa),
lm_wide6.arpa (order 6 over 2 100 LM words: 12 bits x 6 words do not fit a 64-bit key, so the library's table is in hashed
mode) and beam_lm_orders_kat.npz.  Run once on a machine with the reference checkout; its outputs are committed.

    REFERENCE_ROOT=/path/to/TensorflowASR python tests/golden/make_beam_lm_orders_golden.py

The corpus, the ARPA writer, the reference build (the reference's unmodified decoder and scorer, compiled in a temporary
directory against tests/golden/ref_lm_stubs) and ref_decode are those of make_beam_lm_golden.py, whose own outputs
(lm_small.arpa, lm_small4.arpa, beam_lm_kat.npz) this script does not touch.  Nothing of the reference and nothing compiled
is written into the tree.  Nothing is written at all unless the cases exercise what they are for (check_cases)."""
import collections
import ctypes
import json
import os
import shutil
import tempfile

import numpy as np

import make_beam_lm_golden as base
from make_beam_lm_golden import ACOUSTIC, CHARS, HERE, LM_WORDS, N_KNOWN, make_probs, ref_decode, unpack

MAX_BYTES = 500 * 1000
# the wide model's words: those of the small models first (so the 40 known acoustic classes keep their words), then 1 900 more
WIDE_WORDS = LM_WORDS + [chr(0x4E00 + 7 * i) for i in range(len(CHARS), len(CHARS) + 1900)]
# model name -> (file, order, sentences of the corpus that are counted); the high orders count few sentences: the files stay small enough to read
MODELS = {"1": ("lm_small1.arpa", 1, 260), "2": ("lm_small2.arpa", 2, 100), "5": ("lm_small5.arpa", 5, 25),
          "6": ("lm_small6.arpa", 6, 20), "w6": ("lm_wide6.arpa", 6, 15)}

# per model: (T, beam, cutoff_prob, cutoff_top_n, alpha, beta, temperature)
TEMPLATE = [
    (12, 16, 0.99, 40, 1.2, 0.3, 2.0), (16, 17, 0.99, 40, 2.5, 0.0, 2.5), (12, 64, 0.99, 40, 1.2, 0.3, 1.5),
    (12, 65, 0.99, 15, 0.05, 1.5, 2.0), (8, 127, 0.99, 40, 0.002, -0.5, 1.5), (8, 128, 0.99, 40, 2.5, 0.3, 2.0),
    (16, 15, 0.99, 15, 1.2, 0.3, 2.5), (16, 2, 0.99, 40, 1.2, 0.3, 2.5), (12, 1, 0.99, 40, 2.5, 0.3, 2.0),
    (10, 16, 0.99, 2, 1.2, 0.3, 1.0), (6, 17, 0.99, 1, 1.2, 0.3, 1.0), (16, 16, 0.99, 40, 0.0, 0.0, 2.0),
    (12, 64, 0.99, 15, 0.0, 0.0, 2.0), (30, 16, 0.99, 40, 1.2, 0.3, 3.0), (6, 128, 0.99, 40, 0.002, 0.3, 1.0),
]
BOOSTED = (6, 128, 0.99, 40, 0.002, 0.3, 1.0)             # this one gets an OOV class and the space made likely in some frames
HOST_ONLY = [(6, 16, 1.0, 40, 1.2, 0.3, 1.5, "1"), (6, 4, 1.0, 15, 2.5, 0.0, 2.0, "5"), (5, 65, 1.0, 40, 1.2, 0.3, 1.5, "w6")]
LONG = [(400, 16, 0.99, 40, 1.2, 0.3, 2.0, "6"), (400, 65, 0.99, 15, 0.5, 0.3, 1.5, "6")]
CASES = [c + (m,) for m in MODELS for c in TEMPLATE] + HOST_ONLY + LONG
# (beam, cutoff_prob, cutoff_top_n, alpha, beta, temperature, model, pieces)
STATEFUL = [
    (4, 1.0, 40, 1.2, 0.3, 1.5, "1", (5, 1, 9, 6)), (16, 0.99, 15, 0.5, -0.5, 2.0, "2", (12, 12, 3)),
    (65, 0.99, 40, 1.2, 0.3, 2.0, "5", (7, 20)), (17, 0.99, 40, 1.2, 0.3, 2.5, "6", (15, 1, 14)),
]
WANT_BEAMS, WANT_TOP_N = {1, 2, 15, 16, 17, 64, 65, 127, 128}, {1, 2, 15, 40}
SHORT = 100


def boost(p):
    """an acoustic class without an LM word, and the space, made likely in the last frame: the scorer then has to score them"""
    q = p.astype(np.float64)
    q[-1, 1 + N_KNOWN + 2] += 0.5                        # late: every token behind an OOV word pays for it again
    q[-1, 0] += 0.6
    q[-1, 1 + N_KNOWN + 5] += 0.3
    return (q / q.sum(-1, keepdims=True)).astype(np.float32)


def write_model(path, name, sents):
    """base.write_arpa lists the words of base.LM_WORDS: the wide model swaps its own list in for the call"""
    _, order, n_sent = MODELS[name]
    saved = base.LM_WORDS
    try:
        if name == "w6":
            base.LM_WORDS = WIDE_WORDS
        n = base.write_arpa(path, sents[:n_sent], order)
    finally:
        base.LM_WORDS = saved
    return n


def assert_closed(path, order):
    """every listed n-gram's prefix and suffix are listed too: then "the longest stored suffix" of the stand-in (and of the
    library) is what KenLM finds, and no back-off context is missing"""
    grams, m = {}, 0
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line.endswith("-grams:"):
                m = int(line[1:-7])
                grams[m] = set()
            elif m and line and not line.startswith("\\"):
                grams[m].add(tuple(line.split()[1:m + 1]))
    assert max(grams) == order and all(grams[k] for k in grams)
    for k in range(2, order + 1):
        for g in grams[k]:
            assert g[:-1] in grams[k - 1] and g[1:] in grams[k - 1], "%s: %s has no prefix or suffix entry" % (path, g)
    return {k: len(v) for k, v in grams.items()}


def queries(rng, name, sents):
    """n-grams for get_log_cond_prob: seen, backed off, "<s>"-padded, OOV, behind a space; and sentences for get_sent_log_prob"""
    o = MODELS[name][1]
    words = WIDE_WORDS if name == "w6" else LM_WORDS
    grams = []
    for sent in sents[:40]:
        toks = ["<s>"] * (o - 1) + sent
        grams += [toks[i:i + o] for i in range(0, len(toks) - o + 1, 3)]
    for _ in range(150):                                   # random words: mostly backed off
        grams.append([words[int(i)] for i in rng.integers(len(words), size=o)])
    for _ in range(60):                                    # a seen history behind a random word, and in front of one
        s = sents[int(rng.integers(len(sents)))]
        grams.append(([words[int(rng.integers(len(words)))]] + (["<s>"] * o + s)[-(o - 1):])[-o:] if o > 1 else [s[0]])
        grams.append(((["<s>"] * o + s[:3])[-(o - 1):] if o > 1 else []) + [words[int(rng.integers(len(words)))]])
    grams += [["<s>"] * (o - 1) + [words[3]], ["<s>"] * o, [words[1]] * (o - 1) + ["</s>"],
              [words[1]] * (o - 1) + [CHARS[N_KNOWN]],                     # an acoustic class without an LM word
              ([CHARS[N_KNOWN + 1]] + [words[2]] * (o - 1))[-max(o, 1):],   # OOV at the far end of the history
              [words[1]] * (o - 1) + ["<unk>"], [""] * (o - 1) + [words[5]],        # what make_ngram leaves behind a space
              ([words[1]] * max(o - 2, 0) + ["", words[4]])[-o:], [words[0], words[1]][:o]]
    grams = [g for g in grams if len(g) == o] + [g for g in grams if len(g) != o]
    sentences = [sent for sent in sents[:12]] + [[], [words[0]], [words[0], CHARS[N_KNOWN]], [words[-1], words[0]]]
    return grams, sentences


def main():
    rng0 = np.random.default_rng(20251017)
    sents = base.make_corpus(rng0)                         # the corpus of lm_small.arpa / lm_small4.arpa
    saved = base.LM_WORDS
    base.LM_WORDS = WIDE_WORDS
    try:
        wide_sents = base.make_corpus(np.random.default_rng(20251018), n_sent=MODELS["w6"][2])
    finally:
        base.LM_WORDS = saved
    rng = np.random.default_rng(20261017)
    staged = tempfile.mkdtemp(prefix="mi355asr_lm_orders_golden_")
    try:
        tmp_arpa = {}
        for name, (fn, order, _) in MODELS.items():
            tmp_arpa[name] = os.path.join(staged, fn)
            n = write_model(tmp_arpa[name], name, wide_sents if name == "w6" else sents)
            size = os.path.getsize(tmp_arpa[name])
            print("%s: order %d, %d n-grams %s, %d bytes" % (fn, order, n, assert_closed(tmp_arpa[name], order), size))
            assert size <= MAX_BYTES, fn
        n_wide = len(WIDE_WORDS) + 3
        assert n_wide >= 2100 and n_wide.bit_length() * 6 > 64, "the wide model would still be packed"
        lib = base.build_reference(staged)
        vocab = "\n".join(ACOUSTIC).encode("utf-8")
        out, meta, flags = {}, [], collections.defaultdict(collections.Counter)

        def scorer(name, alpha, beta):
            s = lib.ref_scorer_new(alpha, beta, tmp_arpa[name].encode(), vocab)
            assert lib.ref_scorer_is_character_based(s) == 1 and lib.ref_scorer_max_order(s) == MODELS[name][1]
            return s

        unknown = set(range(1 + N_KNOWN, len(ACOUSTIC)))
        for k, (T, beam, cp, tn, alpha, beta, temp, name) in enumerate(CASES):
            p = make_probs(np.random.default_rng((20261017, k)), T, temp)      # a stream per case: changing one leaves the others
            if (T, beam, cp, tn, alpha, beta, temp) == BOOSTED:
                p = boost(p)
            s = scorer(name, alpha, beta)
            ids, lens, sc = ref_decode(lib, p, beam, cp, tn, s)
            lib.ref_scorer_free(s)
            ids0, lens0, sc0 = ref_decode(lib, p, beam, cp, tn, None)
            differs = tuple(ids[0, :lens[0]]) != tuple(ids0[0, :lens0[0]])
            fl = flags[name]
            if alpha == 0.0 and beta == 0.0:
                fl["full_beam_pruning"] += int(len(sc) != len(sc0) or not np.array_equal(sc, sc0))
            if alpha > 0:
                fl["alpha_cases"] += 1
                fl["alpha_differs"] += int(differs)
                toks = set(int(t) for i in range(len(lens)) for t in ids[i, :lens[i]])
                fl["oov_scored"] += int(bool(toks & unknown))
                fl["space_scored"] += int(0 in toks)
            fl["six_tokens"] += int(lens.max() >= 6)
            tied = len(set(sc.tolist())) != len(sc)
            flags["all"]["short_cases"] += int(T <= SHORT)
            flags["all"]["short_untied"] += int(T <= SHORT and not tied)
            out["probs_%d" % k], out["ids_%d" % k], out["lens_%d" % k], out["scores_%d" % k] = p, ids, lens, sc
            meta.append({"T": T, "V": p.shape[1], "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "alpha": alpha, "beta": beta,
                         "order": MODELS[name][1], "model": name, "arpa": MODELS[name][0], "n": int(len(sc)), "tied": bool(tied),
                         "differs_from_scorerless": bool(differs), "longest": int(lens.max())})
        print({k: dict(v) for k, v in flags.items()})
        check_cases(flags, meta)

        smeta = []
        for k, (beam, cp, tn, alpha, beta, temp, name, pieces) in enumerate(STATEFUL):
            p = make_probs(rng, sum(pieces), temp)
            s = scorer(name, alpha, beta)
            h = lib.ref_lm_decoder_new(vocab + b"\n<blank>", beam, cp, tn, s)
            t0 = 0
            for j, n_t in enumerate(pieces):
                pd = np.ascontiguousarray(p[t0:t0 + n_t], np.float64)
                t0 += n_t
                sc = (ctypes.c_double * beam)()
                cap = beam * (4 * t0 + 2) + 16
                text = ctypes.create_string_buffer(cap)
                n = lib.ref_lm_decoder_decode(h, pd.ctypes.data_as(ctypes.c_void_p), n_t, p.shape[1], ctypes.cast(sc, ctypes.c_void_p),
                                              ctypes.cast(text, ctypes.c_void_p), cap)
                out["st_ids_%d_%d" % (k, j)], out["st_lens_%d_%d" % (k, j)], out["st_scores_%d_%d" % (k, j)] = unpack(n, sc, text)
            lib.ref_lm_decoder_free(h)
            lib.ref_scorer_free(s)
            out["st_probs_%d" % k] = p
            smeta.append({"V": p.shape[1], "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "alpha": alpha, "beta": beta,
                          "order": MODELS[name][1], "model": name, "arpa": MODELS[name][0], "pieces": list(pieces)})
        assert sorted(m["order"] for m in smeta) == [1, 2, 5, 6]

        cond = {}
        for name in MODELS:
            s = scorer(name, 1.0, 0.0)
            grams, sentences = queries(rng, name, wide_sents if name == "w6" else sents)
            vals = [lib.ref_scorer_cond(s, "\n".join(g).encode("utf-8")) for g in grams]
            svals = [lib.ref_scorer_sent(s, "\n".join(x).encode("utf-8")) for x in sentences]
            lib.ref_scorer_free(s)
            assert any(v == -1000.0 for v in vals) and any(v != -1000.0 for v in vals)
            cond[name] = {"ngrams": grams, "sentences": sentences}
            out["cond_%s" % name] = np.array(vals, np.float64)
            out["sent_%s" % name] = np.array(svals, np.float64)
        out["meta"] = np.array(json.dumps(meta))
        out["stateful_meta"] = np.array(json.dumps(smeta))
        out["vocabulary"] = np.array(json.dumps(ACOUSTIC))
        out["ngram_queries"] = np.array(json.dumps(cond))
        npz = os.path.join(staged, "beam_lm_orders_kat.npz")
        np.savez_compressed(npz, **out)
        print("beam_lm_orders_kat.npz: %d bytes" % os.path.getsize(npz))
        assert os.path.getsize(npz) <= MAX_BYTES
        for name, (fn, _, _) in MODELS.items():
            shutil.copyfile(tmp_arpa[name], os.path.join(HERE, fn))
        shutil.copyfile(npz, os.path.join(HERE, "beam_lm_orders_kat.npz"))
        print("beam LM order KATs:", len(meta), "one-shot,", len(smeta), "stateful")
    finally:
        shutil.rmtree(staged, ignore_errors=True)


def check_cases(flags, meta):
    """the cases must exercise what they are for, or the tests would pass vacuously"""
    for name in MODELS:
        fl = flags[name]
        assert 2 * fl["alpha_differs"] >= fl["alpha_cases"] > 0, "model %s: the scorer changes the best hypothesis in too few cases: %s" % (name, dict(fl))
        assert fl["oov_scored"] >= 1, "model %s: no case scores an OOV class" % name
        assert fl["space_scored"] >= 1, "model %s: no case scores a space" % name
        assert fl["full_beam_pruning"] >= 1, "model %s: no alpha = beta = 0 case differs from the scorer-less run" % name
    assert any(flags[n]["six_tokens"] for n in ("5", "6", "w6")), "no order-5/6 case with a hypothesis of 6 tokens: some history age holds only <s>"
    al = flags["all"]
    assert 3 * al["short_untied"] >= 2 * al["short_cases"], "too many short cases with tied scores (their ids are not pinned): %s" % dict(al)
    pruned = [m for m in meta if m["cutoff_prob"] < 1.0]
    assert {m["beam"] for m in pruned} >= WANT_BEAMS and {m["cutoff_top_n"] for m in pruned} >= WANT_TOP_N
    assert sum(m["cutoff_prob"] == 1.0 for m in meta) >= 2 and sum(m["T"] >= 400 and m["order"] == 6 for m in meta) >= 2
    assert all(5 <= m["T"] <= 60 or m["T"] >= 400 for m in meta)


if __name__ == "__main__":
    main()
