"""Generator of the n-gram scorer's fixtures: tests/golden/lm_small.arpa (order 3), lm_small4.arpa (order 4) and
beam_lm_kat.npz.  Run once on a machine with the reference checkout; its outputs are committed.

    REFERENCE_ROOT=/path/to/TensorflowASR python tests/golden/make_beam_lm_golden.py

What it does:
  * writes the two ARPA models from a seeded synthetic corpus (a Markov chain over ~200 one-character words) with
    absolute discounting of its own;
  * unpacks externals/ctc_decoders.zip to a temporary directory and compiles the reference's own, unmodified
    ctc_beam_search_decoder.cpp, decoder_utils.cpp, path_trie.cpp and scorer.cpp into a temporary shared object, against
    stand-in headers: tests/golden/ref_lm_stubs (a KenLM interface implemented as the textbook back-off model over the ARPA
    file, OpenFST calls that abort) in front of oracle/ref_stubs;
  * records the reference's ranked (score, ids) with ext_scorer set -- one-shot decoder and stateful BeamDecoder fed in
    pieces -- and Scorer::get_log_cond_prob / get_sent_log_prob for a list of n-grams;
  * refuses to write anything unless the cases exercise what they are for (see check_cases).
Nothing of the reference and nothing compiled is written into the tree."""
import collections
import ctypes
import json
import math
import os
import shutil
import subprocess
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REFERENCE_ROOT") or os.environ.get("REF", "")
SOURCES = ["ctc_beam_search_decoder.cpp", "decoder_utils.cpp", "path_trie.cpp", "scorer.cpp"]

# ---- vocabularies: one-character words; class 0 is the space (the reference's word timestamps assume that) -------------
N_KNOWN, N_UNKNOWN, N_LM_ONLY = 40, 8, 157
CHARS = [chr(0x4E00 + 7 * i) for i in range(N_KNOWN + N_UNKNOWN + N_LM_ONLY)]
ACOUSTIC = [" "] + CHARS[:N_KNOWN + N_UNKNOWN]                 # without the blank; the last N_UNKNOWN have no LM word
LM_WORDS = CHARS[:N_KNOWN] + CHARS[N_KNOWN + N_UNKNOWN:]       # 197 characters + <s> </s> <unk> = 200 words


def make_corpus(rng, n_sent=260):
    nxt = {w: rng.choice(N_KNOWN, 3, replace=False) for w in range(len(LM_WORDS))}
    sents = []
    for _ in range(n_sent):
        w = int(rng.integers(N_KNOWN))
        s = [w]
        for _ in range(int(rng.integers(4, 16))):
            r = rng.random()
            if r < 0.75:
                w = int(nxt[w][int(rng.integers(3))])
            elif r < 0.93:
                w = int(rng.integers(N_KNOWN))
            else:
                w = int(rng.integers(N_KNOWN, len(LM_WORDS)))
            s.append(w)
        sents.append([LM_WORDS[i] for i in s])
    return sents


def write_arpa(path, sents, order, discount=0.6):
    """Back-off model with absolute discounting: p(w|h) = (c(hw) - D) / c(h) for seen n-grams, the left-over mass spread over
    the lower order through bo(h).  Unigrams: add-one over the word list, so that every word has one."""
    counts = [collections.Counter() for _ in range(order + 1)]
    for s in sents:
        toks = ["<s>"] + s + ["</s>"]
        for m in range(1, order + 1):
            for i in range(len(toks) - m + 1):
                counts[m][tuple(toks[i:i + m])] += 1
    words = ["<unk>", "<s>", "</s>"] + LM_WORDS
    total = sum(c for (w,), c in counts[1].items() if w != "<s>") + len(words)
    prob = [None, {}]
    for w in words:
        prob[1][(w,)] = -99.0 if w == "<s>" else math.log10((counts[1].get((w,), 0) + 1) / total)
    for m in range(2, order + 1):
        prob.append({g: math.log10((c - discount) / counts[m - 1][g[:-1]]) for g, c in counts[m].items()})
    backoff = [None] + [{} for _ in range(order)]
    for m in range(1, order):
        seen = collections.defaultdict(list)
        for g in prob[m + 1]:
            seen[g[:-1]].append(g)
        for h in prob[m]:
            if h not in seen:
                continue
            hi = sum(10.0 ** prob[m + 1][g] for g in seen[h])
            lo = sum(10.0 ** cond_logp(prob, backoff, g[1:]) for g in seen[h])
            backoff[m][h] = math.log10(max(1.0 - hi, 1e-6) / max(1.0 - lo, 1e-6))
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for m in range(1, order + 1):
            f.write("ngram %d=%d\n" % (m, len(prob[m])))
        for m in range(1, order + 1):
            f.write("\n\\%d-grams:\n" % m)
            keys = list(prob[1]) if m == 1 else sorted(prob[m])
            for g in keys:
                line = "%.6f\t%s" % (prob[m][g], " ".join(g))
                if m < order and g in backoff[m]:
                    line += "\t%.6f" % backoff[m][g]
                f.write(line + "\n")
        f.write("\n\\end\\\n")
    return sum(len(prob[m]) for m in range(1, order + 1))


def cond_logp(prob, backoff, g):
    """float64 back-off probability while the model is being estimated (lower orders are complete when it is called)"""
    if len(g) == 1 or g in prob[len(g)]:
        return prob[len(g)][g]
    return backoff[len(g) - 1].get(g[:-1], 0.0) + cond_logp(prob, backoff, g[1:])


# ---- the reference, compiled in a temporary directory --------------------------------------------------------------------
def build_reference(tmp):
    assert os.path.exists(os.path.join(REF, "externals", "ctc_decoders.zip")), "set REFERENCE_ROOT to the reference checkout"
    with zipfile.ZipFile(os.path.join(REF, "externals", "ctc_decoders.zip")) as z:
        z.extractall(tmp, [n for n in z.namelist() if n.startswith("ctc_decoders/") and not n.startswith("ctc_decoders/.git/")])
    src = os.path.join(tmp, "ctc_decoders")
    stubs = os.path.join(HERE, "ref_lm_stubs")
    have = sorted(os.path.relpath(os.path.join(d, f), os.path.join(ROOT, "oracle", "ref_stubs"))
                  for d, _, fs in os.walk(os.path.join(ROOT, "oracle", "ref_stubs")) for f in fs)
    print("oracle/ref_stubs provides:", ", ".join(have))
    so = os.path.join(tmp, "libref_beam_lm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-w", "-pthread", "-I" + stubs,
                           "-I" + os.path.join(ROOT, "oracle", "ref_stubs"), "-I" + src, "-I" + os.path.join(src, "ThreadPool"),
                           "-o", so, os.path.join(stubs, "ref_beam_lm_shim.cpp")] + [os.path.join(src, s) for s in SOURCES])
    lib = ctypes.CDLL(so)
    D, I, P, S = ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
    lib.ref_scorer_new.restype = P
    lib.ref_scorer_new.argtypes = [D, D, S, S]
    lib.ref_scorer_free.argtypes = [P]
    lib.ref_scorer_is_character_based.argtypes = [P]
    lib.ref_scorer_max_order.argtypes = [P]
    lib.ref_scorer_cond.restype = D
    lib.ref_scorer_cond.argtypes = [P, S]
    lib.ref_scorer_sent.restype = D
    lib.ref_scorer_sent.argtypes = [P, S]
    lib.ref_lm_beam_search.argtypes = [P, I, I, S, I, D, I, P, P, P, I]
    lib.ref_lm_decoder_new.restype = P
    lib.ref_lm_decoder_new.argtypes = [S, I, D, I, P]
    lib.ref_lm_decoder_free.argtypes = [P]
    lib.ref_lm_decoder_decode.argtypes = [P, P, I, I, P, P, I]
    return lib


CLASS_OF = {c: i for i, c in enumerate(ACOUSTIC)}


def unpack(n, scores, text):
    hyps = text.value.decode("utf-8").split("\n") if n else []
    assert len(hyps) == n, (n, len(hyps))
    lens = np.array([len(h) for h in hyps], np.int32)
    ids = np.full((n, int(lens.max()) if n and lens.max() else 1), -1, np.int32)
    for i, h in enumerate(hyps):
        ids[i, :len(h)] = [CLASS_OF[c] for c in h]
    return ids, lens, np.array(scores[:n], np.float64)


def ref_decode(lib, p, beam, cp, tn, scorer):
    T, V = p.shape
    pd = np.ascontiguousarray(p, np.float64)
    sc = (ctypes.c_double * beam)()
    cap = beam * (4 * T + 2) + 16
    text = ctypes.create_string_buffer(cap)
    n = lib.ref_lm_beam_search(pd.ctypes.data_as(ctypes.c_void_p), T, V, "\n".join(ACOUSTIC).encode("utf-8"), beam, cp, tn, scorer,
                               ctypes.cast(sc, ctypes.c_void_p), ctypes.cast(text, ctypes.c_void_p), cap)
    assert n >= 0
    return unpack(n, sc, text)


def make_probs(rng, T, temp):
    V = len(ACOUSTIC) + 1
    z = rng.standard_normal((T, V)) * temp
    z[:, -1] += 1.0                                        # blank-leaning, like a CTC model
    z[:, 0] += 1.2                                         # the space is a likely class too
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


# (T, beam, cutoff_prob, cutoff_top_n, alpha, beta, temperature, model)
CASES = [
    (6, 1, 1.0, 40, 1.2, 0.3, 1.0, 3), (12, 4, 1.0, 40, 1.2, 0.3, 1.5, 3), (20, 4, 0.99, 8, 0.5, 1.5, 2.0, 3),
    (30, 16, 0.99, 40, 1.2, 0.3, 2.0, 3), (30, 16, 1.0, 8, 2.5, 0.0, 2.5, 4), (40, 16, 0.99, 8, 0.0, 0.3, 2.0, 3),
    (40, 16, 0.99, 40, 0.0, -0.5, 2.0, 4), (25, 100, 0.99, 40, 1.2, 0.3, 1.5, 3), (5, 100, 1.0, 40, 0.002, 0.3, 1.0, 4),
    (60, 4, 0.99, 40, 0.5, -0.5, 3.0, 4), (60, 16, 0.99, 40, 2.5, 1.5, 3.0, 3), (48, 100, 0.99, 8, 1.2, 0.3, 2.5, 4),
    (35, 1, 0.99, 40, 1.2, 0.3, 2.5, 4), (40, 16, 0.99, 40, 0.0, 0.0, 2.0, 3), (16, 4, 1.0, 8, 1.2, -0.5, 2.0, 4),
    (500, 16, 0.99, 40, 1.2, 0.3, 2.0, 3), (400, 100, 0.99, 40, 0.5, 0.3, 1.0, 4), (600, 4, 0.99, 8, 1.2, 1.5, 2.5, 3),
]
# (beam, cutoff_prob, cutoff_top_n, alpha, beta, temperature, model, pieces)
STATEFUL = [
    (4, 1.0, 40, 1.2, 0.3, 1.5, 3, (5, 1, 9, 6)), (16, 0.99, 8, 0.5, -0.5, 2.0, 4, (20, 20, 3)),
    (100, 0.99, 40, 1.2, 0.3, 2.0, 3, (7, 30)), (16, 0.99, 40, 0.0, 0.3, 2.5, 4, (25, 25)),
]
SHORT = 100          # most cases up to this many frames must be free of score ties: their ids are then pinned exactly


def main():
    rng = np.random.default_rng(20251017)
    sents = make_corpus(rng)
    arpa = {3: os.path.join(HERE, "lm_small.arpa"), 4: os.path.join(HERE, "lm_small4.arpa")}
    staged = tempfile.mkdtemp(prefix="mi355asr_lm_golden_")
    try:
        tmp_arpa = {o: os.path.join(staged, os.path.basename(p)) for o, p in arpa.items()}
        for o in arpa:
            print("order", o, ":", write_arpa(tmp_arpa[o], sents, o), "n-grams")
        lib = build_reference(staged)
        vocab = "\n".join(ACOUSTIC).encode("utf-8")
        out, meta, flags = {}, [], collections.Counter()

        def scorer(o, alpha, beta):
            s = lib.ref_scorer_new(alpha, beta, tmp_arpa[o].encode(), vocab)
            assert lib.ref_scorer_is_character_based(s) == 1 and lib.ref_scorer_max_order(s) == o
            return s

        unknown = set(range(1 + N_KNOWN, len(ACOUSTIC)))
        for k, (T, beam, cp, tn, alpha, beta, temp, o) in enumerate(CASES):
            p = make_probs(rng, T, temp)
            s = scorer(o, alpha, beta)
            ids, lens, sc = ref_decode(lib, p, beam, cp, tn, s)
            lib.ref_scorer_free(s)
            ids0, lens0, sc0 = ref_decode(lib, p, beam, cp, tn, None)
            best = tuple(ids[0, :lens[0]])
            differs = best != tuple(ids0[0, :lens0[0]])
            if alpha == 0.0 and beta == 0.0:
                # nothing but the scorer path's pruning separates this run from the scorer-less one
                flags["full_beam_pruning"] += int(len(sc) != len(sc0) or not np.array_equal(sc, sc0))
            if alpha > 0:
                flags["alpha_cases"] += 1
                flags["alpha_differs"] += int(differs)
                toks = set(int(t) for i in range(len(lens)) for t in ids[i, :lens[i]])
                flags["oov_scored"] += int(bool(toks & unknown))
                flags["space_scored"] += int(0 in toks)
            tied = len(set(sc.tolist())) != len(sc)
            flags["short_cases"] += int(T <= SHORT)
            flags["short_untied"] += int(T <= SHORT and not tied)
            out["probs_%d" % k], out["ids_%d" % k], out["lens_%d" % k], out["scores_%d" % k] = p, ids, lens, sc
            meta.append({"T": T, "V": p.shape[1], "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "alpha": alpha, "beta": beta,
                         "order": o, "arpa": os.path.basename(arpa[o]), "n": int(len(sc)), "tied": bool(tied), "differs_from_scorerless": bool(differs)})
        check_cases(flags)

        smeta = []
        for k, (beam, cp, tn, alpha, beta, temp, o, pieces) in enumerate(STATEFUL):
            p = make_probs(rng, sum(pieces), temp)
            s = scorer(o, alpha, beta)
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
            smeta.append({"V": p.shape[1], "beam": beam, "cutoff_prob": cp, "cutoff_top_n": tn, "alpha": alpha, "beta": beta, "order": o,
                          "arpa": os.path.basename(arpa[o]), "pieces": list(pieces)})

        # ---- Scorer::get_log_cond_prob / get_sent_log_prob on listed n-grams: seen, backed-off, OOV, "<s>"-padded, space ----
        cond = {}
        for o in arpa:
            s = scorer(o, 1.0, 0.0)
            grams = []
            for sent in sents[:40]:
                toks = ["<s>"] * (o - 1) + sent
                grams += [toks[i:i + o] for i in range(0, len(toks) - o + 1, 3)]
            for _ in range(150):                           # random words: mostly backed off
                grams.append([LM_WORDS[int(i)] for i in rng.integers(len(LM_WORDS), size=o)])
            grams += [["<s>"] * (o - 1) + [LM_WORDS[3]], ["<s>"] * o, [LM_WORDS[1]] * (o - 1) + ["</s>"],
                      [LM_WORDS[1]] * (o - 1) + [CHARS[N_KNOWN]],                  # an acoustic class without an LM word
                      [CHARS[N_KNOWN + 1]] + [LM_WORDS[2]] * (o - 1),              # OOV at the far end of the history
                      [LM_WORDS[1]] * (o - 1) + ["<unk>"], [""] * (o - 1) + [LM_WORDS[5]],      # what make_ngram leaves behind a space
                      [LM_WORDS[1]] * (o - 2) + ["", LM_WORDS[4]], [LM_WORDS[0], LM_WORDS[1]][:o]]
            vals = [lib.ref_scorer_cond(s, "\n".join(g).encode("utf-8")) for g in grams]
            sentences = [sent for sent in sents[:12]] + [[], [LM_WORDS[0]], [LM_WORDS[0], CHARS[N_KNOWN]]]
            svals = [lib.ref_scorer_sent(s, "\n".join(x).encode("utf-8")) for x in sentences]
            lib.ref_scorer_free(s)
            assert any(v == -1000.0 for v in vals) and any(v != -1000.0 for v in vals)
            cond[str(o)] = {"ngrams": grams, "sentences": sentences}
            out["cond_%d" % o] = np.array(vals, np.float64)
            out["sent_%d" % o] = np.array(svals, np.float64)
        out["meta"] = np.array(json.dumps(meta))
        out["stateful_meta"] = np.array(json.dumps(smeta))
        out["vocabulary"] = np.array(json.dumps(ACOUSTIC))
        out["ngram_queries"] = np.array(json.dumps(cond))
        for o in arpa:
            shutil.copyfile(tmp_arpa[o], arpa[o])
        np.savez_compressed(os.path.join(HERE, "beam_lm_kat.npz"), **out)
        print("beam LM KATs:", len(meta), "one-shot,", len(smeta), "stateful;", dict(flags))
    finally:
        shutil.rmtree(staged, ignore_errors=True)


def check_cases(flags):
    """the cases must exercise what they are for, or the tests would pass vacuously"""
    assert 2 * flags["alpha_differs"] >= flags["alpha_cases"] > 0, "the scorer changes the best hypothesis in too few cases: %s" % dict(flags)
    assert flags["full_beam_pruning"] >= 1, "no case reaches the full_beam pruning"
    assert flags["oov_scored"] >= 1, "no case scores an OOV class"
    assert flags["space_scored"] >= 1, "no case scores a space"
    assert 3 * flags["short_untied"] >= 2 * flags["short_cases"], "too many short cases with tied scores (their ids are not pinned)"


if __name__ == "__main__":
    main()
