"""The external scorer of the CTC prefix beam search: a back-off n-gram language model read from an ARPA file, in the
reference's CHARACTER-BASED mode.

replaces: `Scorer(alpha, beta, lm_path, vocab_list)` of externals/ctc_decoders (scorer.h, scorer.cpp, SWIG decoders.i),
where KenLM is called as "log10 p(w | history) of a back-off n-gram model" (scorer.cpp:74-93).  The word-based mode, which
spell-checks prefixes against a dictionary FST built with OpenFST (scorer.cpp:196-230), is not built and is refused.

    scorer = NGramScorer(alpha, beta, "lm.arpa", vocabulary)          # vocabulary: acoustic classes WITHOUT the blank
    ids, lens, scores, n = ctc_prefix_beam_decode(probs, None, 10, ext_scorer=scorer)

Only the standard library and NumPy are needed to read a model; scoring inside a search runs in libmi355asr.so
(`mi355asr_lm_create`: one packed table for the host and the device search)."""
import ctypes
import gzip
import io

import numpy as np

OOV_SCORE = -1000.0                 # scorer.h:16
START_TOKEN, UNK_TOKEN, END_TOKEN = "<s>", "<unk>", "</s>"
MAX_ORDER = 6


class ArpaError(ValueError):
    pass


class ArpaModel:
    """order; counts [order]; words: the unigrams in file order (word id = index + 1, 0 is kept for OOV);
    ids[m - 1] int32 [counts[m - 1], m] word ids w_1 .. w_m; logp[m - 1], backoff[m - 1] float32 (0 where the file has none)."""

    def __init__(self, order, words, ids, logp, backoff):
        self.order, self.words, self.ids, self.logp, self.backoff = order, words, ids, logp, backoff
        self.counts = [len(x) for x in logp]
        self.word_to_id = {w: i + 1 for i, w in enumerate(words)}


def _open_text(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    if magic == b"\x1f\x8b":
        return io.TextIOWrapper(gzip.open(path, "rb"), encoding="utf-8")
    return open(path, "r", encoding="utf-8")


def read_arpa(path):
    """ARPA text (plain or gzip) -> ArpaModel.  Orders 1 .. 6; the \\data\\ counts are checked against what is read; a
    malformed file raises ArpaError with the line number."""
    def bad(no, msg):
        return ArpaError("%s: line %d: %s" % (path, no, msg))

    declared = {}
    sections = {}
    state, cur, no, ended = "head", 0, 0, False
    word_to_id, words = {}, []
    with _open_text(path) as f:
        for no, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if state == "head":
                if line == "\\data\\":
                    state = "data"
                continue                                  # text in front of \data\ is allowed
            if line.startswith("\\"):
                if line == "\\end\\":
                    ended = True
                    break
                if not (line.endswith("-grams:") and line[1:-7].isdigit()):
                    raise bad(no, "unknown section %r" % line)
                m = int(line[1:-7])
                if m != cur + 1 or m not in declared:
                    raise bad(no, "section %r out of sequence or not declared under \\data\\" % line)
                cur, state = m, "grams"
                sections[m] = ([], [], [])
                continue
            if state == "data":
                if not line.startswith("ngram ") or "=" not in line:
                    raise bad(no, "expected 'ngram N=count', got %r" % line)
                k, _, v = line[6:].partition("=")
                try:
                    m, c = int(k), int(v)
                except ValueError:
                    raise bad(no, "expected 'ngram N=count', got %r" % line)
                if m != len(declared) + 1 or c < 0:
                    raise bad(no, "orders must be declared as 1, 2, ... with counts >= 0")
                if m > MAX_ORDER:
                    raise bad(no, "order %d: up to %d are supported" % (m, MAX_ORDER))
                declared[m] = c
                continue
            parts = line.split()
            if len(parts) not in (cur + 1, cur + 2):
                raise bad(no, "a %d-gram line has %d fields" % (cur, len(parts)))
            try:
                lp = float(parts[0])
                bo = float(parts[cur + 1]) if len(parts) == cur + 2 else 0.0
            except ValueError:
                raise bad(no, "probability or back-off is not a number")
            toks = parts[1:cur + 1]
            if cur == 1:
                if toks[0] in word_to_id:
                    raise bad(no, "unigram %r appears twice" % toks[0])
                word_to_id[toks[0]] = len(words) + 1
                words.append(toks[0])
                row = [len(words)]
            else:
                try:
                    row = [word_to_id[t] for t in toks]
                except KeyError as e:
                    raise bad(no, "word %s has no unigram" % e)
            sec = sections[cur]
            sec[0].append(row)
            sec[1].append(lp)
            sec[2].append(bo)
    if not declared:
        raise bad(no, "no \\data\\ section")
    if not ended:
        raise bad(no, "file ends without \\end\\ (truncated?)")
    order = len(declared)
    ids, logp, backoff = [], [], []
    for m in range(1, order + 1):
        rows, lps, bos = sections.get(m, ([], [], []))
        if len(rows) != declared[m]:
            raise bad(no, "\\data\\ declares %d %d-grams, the file holds %d" % (declared[m], m, len(rows)))
        ids.append(np.asarray(rows, np.int32).reshape(-1, m))
        logp.append(np.asarray(lps, np.float32))
        backoff.append(np.asarray(bos, np.float32))
    if declared[1] < 1:
        raise bad(no, "no unigrams")
    return ArpaModel(order, words, ids, logp, backoff)


def synthetic_model(words, n_bigrams, n_trigrams, seed=0, higher=()):
    """A seeded ArpaModel of order 3 (or 3 + len(higher), `higher` giving the counts of the orders above) over `words` (plus <unk>, <s>, </s>) with random n-grams and plausible weights: what the
    timing tool and the GPU tests use where a table of realistic SIZE is wanted and its contents do not matter."""
    rng = np.random.default_rng(seed)
    allw = [UNK_TOKEN, START_TOKEN, END_TOKEN] + list(words)
    n = len(allw)
    ids, logp, bo = [np.arange(1, n + 1, dtype=np.int32).reshape(-1, 1)], [], []
    logp.append((-rng.uniform(1.0, 6.0, n)).astype(np.float32))
    bo.append((-rng.uniform(0.0, 1.5, n)).astype(np.float32))
    order = 3 + len(higher)
    for m, want in enumerate((n_bigrams, n_trigrams) + tuple(higher), 2):
        # words 4 .. n (not <unk>, and "<s>" only in front), distinct rows
        g = rng.integers(4, n + 1, size=(int(want * 1.1) + 8, m)).astype(np.int64)
        g[rng.random(len(g)) < 0.05, 0] = 2
        _, first = np.unique(g, axis=0, return_index=True)
        g = g[np.sort(first)][:want].astype(np.int32)
        ids.append(g)
        logp.append((-rng.uniform(0.05, 4.0, len(g))).astype(np.float32))
        bo.append((-rng.uniform(0.0, 1.0, len(g))).astype(np.float32) if m < order else np.zeros(len(g), np.float32))
    return ArpaModel(order, allw, ids, logp, bo)


def _utf8_len(s):
    return len(s)                                          # get_utf8_str_len counts code points; so does len() of a str


class NGramScorer:
    """`Scorer` of the reference: .alpha, .beta, reset_params, is_character_based, get_max_order, get_dict_size,
    get_log_cond_prob(words), get_sent_log_prob(words).  `vocabulary` is the acoustic vocabulary without the blank.

    Kept from the reference: an acoustic class maps to the LM word with the same string; a class without an LM word, and
    "<unk>", is OOV, and any OOV word in an n-gram makes get_log_cond_prob OOV_SCORE; scores are KenLM's log10 values as
    they are; a " " class is not stepped over by make_ngram in character mode -- every slot from the first space backwards
    is the empty word, so an n-gram with a space among its last max_order tokens scores OOV_SCORE."""

    def __init__(self, alpha, beta, lm_path, vocabulary, model=None):
        """model: an ArpaModel already in memory (lm_path is then only a label)"""
        self.alpha, self.beta = float(alpha), float(beta)
        self.lm_path = lm_path
        self.vocabulary = list(vocabulary)
        self.model = model if model is not None else read_arpa(lm_path)
        special = (START_TOKEN, END_TOKEN, UNK_TOKEN)
        long_words = [w for w in self.model.words if w not in special and _utf8_len(w) > 1]     # scorer.cpp:65-70
        self._character_based = not long_words
        if long_words:
            raise NotImplementedError(
                "%s is a word-based model (e.g. %r): that mode spell-checks prefixes against a dictionary FST built with "
                "OpenFST (scorer.cpp fill_dictionary), which is not part of this build; only character-based models are "
                "supported" % (lm_path, long_words[0]))
        w2i = self.model.word_to_id
        self.class_word = np.asarray([0 if v == UNK_TOKEN else w2i.get(v, 0) for v in self.vocabulary], np.int32)
        self.bos_word = int(w2i.get(START_TOKEN, 0))
        self.space_class = self.vocabulary.index(" ") if " " in self.vocabulary else -2
        self._table = None
        self._ptr = None
        self._lib = None

    # ---- the reference's surface ----
    def reset_params(self, alpha, beta):
        """scorer.h:63 takes floats: the doubles the search reads are float32 values afterwards"""
        self.alpha, self.beta = float(np.float32(alpha)), float(np.float32(beta))

    def is_character_based(self):
        return self._character_based

    def get_max_order(self):
        return self.model.order

    def get_dict_size(self):
        return 0                                           # the dictionary FST's size; a character-based scorer has none

    def word_id(self, word):
        """LM word id as the search sees it: 0 for OOV, "<unk>" and the empty word"""
        return 0 if word == UNK_TOKEN else self.model.word_to_id.get(word, 0)

    def _lookup(self):
        if self._table is None:
            t = {}
            m = self.model
            for k in range(m.order):
                for row, lp, bo in zip(m.ids[k].tolist(), m.logp[k], m.backoff[k]):
                    t[tuple(row)] = (lp, bo)
            self._table = t
        return self._table

    def get_log_cond_prob(self, words):
        """scorer.cpp:74-93: log10 p(words[-1] | the words before it), from the null context; OOV_SCORE if any word is OOV.
        float32 arithmetic as KenLM's: logp of the longest stored suffix, plus the back-offs of the contexts backed off
        from, shortest first; the float widened to a Python float."""
        ids = [self.word_id(w) for w in words]
        if not ids or 0 in ids:
            return OOV_SCORE
        ids = ids[-self.model.order:]
        t = self._lookup()
        found, p = 0, np.float32(0)
        for n in range(1, len(ids) + 1):
            e = t.get(tuple(ids[len(ids) - n:]))
            if e is not None:
                found, p = n, e[0]
        for n in range(found, len(ids)):                   # the context of length n: the n words before the last
            e = t.get(tuple(ids[len(ids) - 1 - n:len(ids) - 1]))
            if e is not None:
                p = np.float32(p + e[1])
        return float(p)

    def get_sent_log_prob(self, words):
        """scorer.cpp:95-120"""
        n = self.model.order
        sent = [START_TOKEN] * (n if not words else n - 1) + list(words) + [END_TOKEN]
        return sum(self.get_log_cond_prob(sent[i:i + n]) for i in range(len(sent) - n + 1))

    def make_ngram(self, token_ids):
        """Scorer::make_ngram (scorer.cpp:164-194) of a prefix given as class ids, character mode -> max_order words"""
        n = self.model.order
        out = []
        toks = list(token_ids)
        while len(out) < n and toks:
            c = toks[-1]
            if c == self.space_class:
                out.append("")                             # get_path_vec stops AT the space and does not move on
                continue
            out.append(self.vocabulary[c])
            toks.pop()
        out += [START_TOKEN] * (n - len(out))
        return out[::-1]

    # ---- the library's side ----
    def handle(self):
        """the `mi355asr_lm` of this model (created on first use)"""
        if self._ptr is None:
            from . import _lib
            lib = _lib.lib()
            m = self.model
            counts = np.asarray(m.counts, np.int64)
            words = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in m.ids]), np.int32)
            logp = np.ascontiguousarray(np.concatenate(m.logp), np.float32)
            bo = np.ascontiguousarray(np.concatenate(m.backoff), np.float32)
            ptr = ctypes.c_void_p()
            vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
            _lib.check(lib.mi355asr_lm_create(m.order, vp(counts), vp(words), vp(logp), vp(bo), vp(self.class_word),
                                              len(self.class_word), self.bos_word, self.space_class, ctypes.byref(ptr)))
            self._lib, self._ptr = lib, ptr
        return self._ptr

    def score_ids(self, ngrams, on_device=False, stream=None):
        """`mi355asr_lm_score`: int32 [n, max_order] LM word ids (0 = OOV, "<s>"-padded) -> float32 [n]"""
        from . import _lib
        g = np.ascontiguousarray(ngrams, np.int32).reshape(-1, self.model.order)
        out = np.empty((g.shape[0],), np.float32)
        ptr = self.handle()
        _lib.check(self._lib.mi355asr_lm_score(ptr, g.ctypes.data_as(ctypes.c_void_p), g.shape[0], out.ctypes.data_as(ctypes.c_void_p),
                                               int(bool(on_device)), ctypes.c_void_p(stream or 0)))
        return out

    def __del__(self):
        try:
            if self._ptr:
                self._lib.mi355asr_lm_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass
