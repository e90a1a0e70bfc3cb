"""Records tests/golden/wer_edges.npz: the reference's own `levenshtein` (utils/xer.py:12-35, imported as it is; it needs only
NumPy) on pairs at the length, wave, strip and tie-breaking edges of the GPU edit distance (tensorflowasr_amd/scoring.py).

Per case c: the reference row ref[ref_off[c] : ref_off[c + 1]], the hypothesis row hyp[hyp_off[c] : hyp_off[c + 1]] (uint8
ids from alphabets of 2 .. 6 symbols) and expect[c] = (distance, S, D, I) as xer.levenshtein(ref, hyp) returned them.  The
last case is 16 384 x 16 384 over four letters: about two minutes of the reference's Python, once, here.

    python tests/golden/make_wer_edges.py /path/to/TensorflowASR
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STRIP = 1024                      # scoring.EditDistance.STRIP
SHORT = [0, 1, 2, 63, 64, 65, 127, 128, 129]
LONG = [STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1]
MAX_LEN = 16384


def cases():
    rng = np.random.default_rng(20240611)
    out = []

    def rand(n, k):
        return rng.integers(0, k, n).astype(np.uint8)

    def noisy(u, k):
        """u with about a tenth of its tokens replaced, dropped or doubled: a hypothesis close to its reference, many ties"""
        v = []
        for t in u:
            r = rng.random()
            if r < 0.03:
                continue
            v.append(int(rng.integers(0, k)) if r < 0.07 else int(t))
            if r > 0.97:
                v.append(int(rng.integers(0, k)))
        return np.array(v, np.uint8)

    i = 0
    for n in SHORT:
        for m in SHORT:
            k = 2 + i % 5
            i += 1
            out.append(("short_%dx%d" % (n, m), rand(n, k), rand(m, k)))
    for x in LONG:
        k = 2 + i % 5
        i += 1
        out.append(("ref%d_short" % x, rand(x, k), rand(7, k)))
        out.append(("hyp%d_short" % x, rand(7, k), rand(x, k)))
        u = rand(x, k)
        v = noisy(u, k)
        v = np.concatenate([v, rand(max(x - len(v), 0), k)])[:x]
        out.append(("both%d" % x, u, v))
    out.append(("5x3000", rand(5, 3), rand(3000, 3)))
    out.append(("3000x5", rand(3000, 3), rand(5, 3)))
    # the rows with the most ties: identical, fully disjoint, one symbol repeated
    u = rand(200, 4)
    out.append(("identical_200", u, u.copy()))
    u = rand(1100, 5)
    out.append(("identical_1100", u, u.copy()))
    out.append(("disjoint_150x170", rand(150, 3), (rand(170, 3) + 3).astype(np.uint8)))
    out.append(("disjoint_1030x70", rand(1030, 2), (rand(70, 2) + 2).astype(np.uint8)))
    out.append(("repeat_130x67", np.zeros(130, np.uint8), np.zeros(67, np.uint8)))
    out.append(("repeat_67x130", np.zeros(67, np.uint8), np.zeros(130, np.uint8)))
    out.append(("repeat_other_100x100", np.zeros(100, np.uint8), np.ones(100, np.uint8)))
    out.append(("repeat_1100x1030", np.zeros(1100, np.uint8), np.zeros(1030, np.uint8)))
    out.append(("repeat_in_random_300x1025", np.zeros(300, np.uint8), rand(1025, 2)))
    out.append(("max_len", rand(MAX_LEN, 4), rand(MAX_LEN, 4)))
    return out


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_xer", os.path.join(ref_root, "utils", "xer.py"))
    xer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(xer)
    cs = cases()
    expect = []
    for name, u, v in cs:
        cost, (s, d, i) = xer.levenshtein(u.tolist(), v.tolist())
        expect.append((cost, s, d, i))
        print(name, expect[-1], flush=True)
    path = os.path.join(HERE, "wer_edges.npz")
    np.savez_compressed(
        path, names=np.array([c[0] for c in cs]), expect=np.array(expect, np.int32),
        ref=np.concatenate([c[1] for c in cs]), hyp=np.concatenate([c[2] for c in cs]),
        ref_off=np.cumsum([0] + [len(c[1]) for c in cs]).astype(np.int64),
        hyp_off=np.cumsum([0] + [len(c[2]) for c in cs]).astype(np.int64))
    print("wrote wer_edges.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
