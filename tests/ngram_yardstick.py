"""Yardstick of the n-gram scorer tests, not the code under test: a back-off language model over an ARPA file in plain
Python and float64, with a parser of its own.  Written from the definition of the format -- p(w | h) is the listed
log-probability of (h, w) if the file has it, else back-off(h) + p(w | h without its first word) -- and not from the
library's table (csrc/lm_table.h), the package's reader (tensorflowasr_amd/ngram.py) or the fixture generator's stand-in."""
import gzip

OOV_SCORE = -1000.0


def parse_arpa(path):
    """-> (order, declared counts, {m: {(w_1 .. w_m): (logp, backoff or None)}}), everything as the text gives it"""
    opener = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    counts, grams, m = {}, {}, 0
    with opener(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line in ("\\data\\", "\\end\\"):
                continue
            if line.startswith("ngram "):
                k, v = line[6:].split("=")
                counts[int(k)] = int(v)
            elif line.startswith("\\"):
                m = int(line[1:line.index("-")])
                grams[m] = {}
            else:
                f_ = line.split()
                grams[m][tuple(f_[1:m + 1])] = (float(f_[0]), float(f_[m + 1]) if len(f_) > m + 1 else None)
    return max(counts), counts, grams


class BackoffLM:
    def __init__(self, path):
        self.order, self.counts, self.grams = parse_arpa(path)
        self.words = set(w for (w,) in self.grams[1]) - {"<unk>"}

    def cond(self, words):
        """log10 p(words[-1] | words[:-1]) in float64 -> (value, the terms that were added); OOV_SCORE if a word is unknown"""
        if any(w not in self.words for w in words):
            return OOV_SCORE, [OOV_SCORE]
        return self._p(tuple(words[-self.order:]))

    def _p(self, g):
        e = self.grams[len(g)].get(g)
        if e is not None:
            return e[0], [e[0]]
        ctx = self.grams[len(g) - 1].get(g[:-1])
        bo = ctx[1] if ctx is not None and ctx[1] is not None else 0.0
        p, terms = self._p(g[1:])
        return bo + p, terms + [bo]

    def sentence(self, words):
        n = self.order
        sent = ["<s>"] * (n if not words else n - 1) + list(words) + ["</s>"]
        return sum(self.cond(sent[i:i + n])[0] for i in range(len(sent) - n + 1))
