"""More GPU steps of tests/test_gpu_beam_lm.py, one per process: `python tests/beam_orders_gpu_steps.py STEP`.  They pin the
device prefix beam search where beam_lm_gpu_steps.py does not reach: language-model orders 1, 2, 5, 6 and hashed table keys,
the beam widths and candidate counts at which the search changes kernels, the redo of the one-key-per-thread kernel, the
class-count limit and max_len below a hypothesis' length.  Every call asserts `beam_last_path()`: all paths return the same
arrays, so an equality that ran the host search twice would prove nothing.  A step prints what it ran and exits non-zero on
the first mismatch; it is never repeated."""
import collections
import json
import os
import re
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tensorflowasr_amd import ngram                                                        # noqa: E402
from tensorflowasr_amd.models import beam_device_limits, beam_last_path, ctc_prefix_beam_decode   # noqa: E402
from beam_lm_gpu_steps import same                                                        # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
ARPA = {"3": "lm_small.arpa", "1": "lm_small1.arpa", "2": "lm_small2.arpa", "5": "lm_small5.arpa", "6": "lm_small6.arpa", "w6": "lm_wide6.arpa"}
SMALL_THREADS = 256          # threads of the one-key-per-thread kernel: one per (entry, candidate) key (include/mi355asr.h)
HOST, SMALL, RADIX, SCORER = 1, 2, 3, 4


def expected_path(V, beam, top_n, with_scorer):
    """the dispatch rule of mi355asr_ctc_prefix_beam*, from the limits the library reports"""
    lim = beam_device_limits(with_scorer)
    N = min(top_n, V)
    if V > lim["max_classes"] or beam > lim["max_beam"] or N > lim["max_top_n"]:
        return HOST
    if with_scorer:
        return SCORER
    return SMALL if beam <= lim["small_beam"] and beam * (min(N, beam + 2) + 1) <= SMALL_THREADS else RADIX


def both(p, pd, lens, beam, cp, top_n, scorer, seen, what, **kw):
    """device call (with its path asserted) and host call on the same probabilities -> equal in everything"""
    dev = ctc_prefix_beam_decode(pd, lens, beam, cp, top_n, ext_scorer=scorer, **kw)
    path = beam_last_path()
    want = expected_path(p.shape[-1], beam, top_n, scorer is not None)
    assert path == want, "%s: ran path %d, the dispatch rule says %d" % (what, path, want)
    host = ctc_prefix_beam_decode(p, lens, beam, cp, top_n, ext_scorer=scorer, num_threads=min(16, p.shape[0]), **kw)
    same(dev, host, what)
    seen[path] += 1
    return dev


def common_batch(V, seed, favoured=None):
    """B = 6, T = 90: peaked rows (the cumulative cut keeps a handful of classes), flat rows (every candidate, closely spaced
    scores), blank-dominated rows, repeated characters; lengths including 0 and 1.  favoured: classes every frame leans to"""
    rng = np.random.default_rng(seed)
    B, T = 6, 90
    z = rng.standard_normal((B, T, V)).astype(np.float32)
    z[0] *= 6.0
    z[1] *= 0.2
    z[2] *= 3.0
    z[2, :, -1] += 8.0
    z[3] *= rng.uniform(0.1, 6.0, (T, 1)).astype(np.float32)
    z[4] *= 2.0
    z[5] *= 4.0
    z[5, ::3, -1] += 6.0
    z[5, 1::3] = z[5, ::3][: z[5, 1::3].shape[0]] + 0.01 * z[5, 1::3]
    if favoured is not None:
        z[:, :, favoured] += 3.0
    p = torch.softmax(torch.from_numpy(z), -1).numpy()
    return p, np.array([T, T, 61, T, 1, 0], np.int32)


def fixture_scorer(name, vocab, alpha=1.0, beta=0.0):
    return ngram.NGramScorer(alpha, beta, os.path.join(GOLDEN, ARPA[name]), vocab)


def dense_model(n_words, order, seed, extra_words=0):
    """`ngram.synthetic_model` over FEW words, so that its random n-grams of every order are met by the hypotheses of a search (over
    a few hundred words no random 5-gram ever is, and the oldest words of the history would decide nothing).  extra_words > 0 puts
    that many unigrams in front of them: the words of the n-grams get ids above 2^11 and the table of an order-6 model hashed keys."""
    words = [chr(0x4E00 + 7 * i) for i in range(n_words)]
    higher = {5: (8000, 40000), 6: (8000, 40000, 150000)}[order]
    m = ngram.synthetic_model(words, 150, 1500, seed=seed, higher=higher)
    if extra_words:
        rng = np.random.default_rng(seed + 1)
        extra = [chr(0x20000 + i) for i in range(extra_words)]
        lift = lambda a: np.where(a >= 4, a + extra_words, a).astype(np.int32)               # noqa: E731
        n = len(m.words) + extra_words
        ids = [np.arange(1, n + 1, dtype=np.int32).reshape(-1, 1)] + [lift(a) for a in m.ids[1:]]
        logp = [np.concatenate([m.logp[0][:3], (-rng.uniform(1.0, 6.0, extra_words)).astype(np.float32), m.logp[0][3:]])] + m.logp[1:]
        bo = [np.concatenate([m.backoff[0][:3], (-rng.uniform(0.0, 1.5, extra_words)).astype(np.float32), m.backoff[0][3:]])] + m.backoff[1:]
        m = ngram.ArpaModel(m.order, m.words[:3] + extra + m.words[3:], ids, logp, bo)
    return words, m


def step_orders():
    K = np.load(os.path.join(GOLDEN, "beam_lm_orders_kat.npz"))
    vocab = json.loads(str(K["vocabulary"]))
    seen = collections.Counter()
    # ---- 1. mi355asr_lm_score on the device
    for name in ("1", "2", "5", "6", "w6"):
        s = fixture_scorer(name, vocab)
        order, n_words = s.model.order, len(s.model.words)
        rng = np.random.default_rng(order)
        ids = rng.integers(0, n_words + 1, size=(20000, order)).astype(np.int32)
        stored = np.concatenate([np.pad(s.model.ids[k], ((0, 0), (order - 1 - k, 0)), constant_values=s.bos_word) for k in range(order)])
        behind = stored.copy()                                        # a stored n-gram behind another first word: backed off once
        behind[:, 0] = rng.integers(1, n_words + 1, len(behind))
        ids = np.concatenate([ids, stored, behind])
        host, dev = s.score_ids(ids), s.score_ids(ids, on_device=True)
        assert np.array_equal(host.view(np.int32), dev.view(np.int32)), (name, np.argwhere(host != dev)[:5])
        print("model %s (order %d, %d words): device mi355asr_lm_score == host on %d n-grams (%d OOV)" %
              (name, order, n_words, len(ids), int((host == -1000).sum())))
    # ---- 2. the fixture cases the device search takes: device == host == the reference's scores
    lim = beam_device_limits(True)
    sc = {name: fixture_scorer(name, vocab) for name in ("1", "2", "5", "6", "w6")}
    done = collections.Counter()
    for i, m in enumerate(json.loads(str(K["meta"]))):
        if not (m["cutoff_prob"] < 1.0 and m["beam"] <= lim["max_beam"] and m["cutoff_top_n"] <= lim["max_top_n"]):
            continue
        s = sc[m["model"]]
        s.alpha, s.beta = m["alpha"], m["beta"]
        p = K["probs_%d" % i][None]
        dev = both(p, torch.from_numpy(p).cuda(), None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], s, seen, "fixture case %d %s" % (i, m))
        assert np.array_equal(dev[2][0, :m["n"]].astype(np.float64), K["scores_%d" % i]), i
        done[m["model"]] += 1
    assert all(done[name] >= 14 for name in sc) and sum(done.values()) >= 75, dict(done)
    print("device search == host search == the reference's scores on the fixture cases per model: %s" % dict(done))
    # ---- 3. the common batch with models whose high orders are met: packed keys at orders 5 and 6, hashed keys at order 6
    p, lens = common_batch(50, 7, favoured=slice(1, 13))             # the frames lean to the 12 classes the dense models know
    pd = torch.from_numpy(p).cuda()
    for order, extra in ((5, 0), (6, 0), (6, 2200)):
        words, m = dense_model(12, order, seed=order, extra_words=extra)
        n_words = len(m.words)
        assert (n_words.bit_length() * order > 64) == bool(extra)
        # 49 classes: a space, the model's 12 words, and 36 classes the model lacks
        s = ngram.NGramScorer(0.5, 0.3, "synthetic", [" "] + words + [chr(0x6000 + i) for i in range(36)], model=m)
        top = set(map(tuple, m.ids[order - 1].tolist()))
        met = 0
        for beam, alpha, beta in ((8, 0.5, 0.3), (100, 0.5, 0.3), (100, 0.0, 0.0)):
            s.alpha, s.beta = alpha, beta
            d = both(p, pd, lens, beam, 0.99, 40, s, seen, "order %d%s beam %d alpha %g" % (order, " hashed" if extra else "", beam, alpha))
            for b in range(p.shape[0]):
                for j in range(d[3][b]):
                    w = [int(s.class_word[c]) for c in d[0][b, j, :d[1][b, j]]]
                    met += sum(tuple(w[q:q + order]) in top for q in range(len(w) - order + 1))
        assert met > 0, "no hypothesis holds an n-gram of the highest order: the oldest words of the history decided nothing"
        print("common batch, order %d, %s keys: device == host at beams 8 and 100; %d highest-order n-grams met in the results" %
              (order, "hashed" if extra else "packed", met))
    assert set(seen) == {SCORER}, dict(seen)
    print("paths seen: %s" % dict(seen))


def step_widths():
    seen = collections.Counter()
    lim = beam_device_limits(False)
    p, lens = common_batch(300, 11)
    pd = torch.from_numpy(p).cuda()
    by_beam = collections.defaultdict(set)
    for beam in (2, 3, 15, 16, 17, 63, 64, 65, 127, 128):
        for top_n in (1, 2, 12, 15, 16, 40):
            for cp in (0.99, 0.9999):
                both(p, pd, lens, beam, cp, top_n, None, seen, "scorer-less beam %d top_n %d cutoff %g" % (beam, top_n, cp))
                by_beam[beam].add(beam_last_path())
    assert SMALL in by_beam[lim["small_beam"]] and by_beam[lim["small_beam"] + 1] == {RADIX}
    assert SMALL in by_beam[15] and SMALL in by_beam[16] and RADIX in by_beam[16] and RADIX in by_beam[17], dict(by_beam)
    assert by_beam[17] == {RADIX} and by_beam[128] == {RADIX} and seen[HOST] == 0
    print("scorer-less: %d calls, device == host; paths per beam: %s" % (sum(seen.values()), {b: sorted(v) for b, v in by_beam.items()}))
    K = np.load(os.path.join(GOLDEN, "beam_lm_orders_kat.npz"))
    vocab = json.loads(str(K["vocabulary"]))
    p50, lens50 = common_batch(50, 12)
    pd50 = torch.from_numpy(p50).cuda()
    n_sc = 0
    for name in ("3", "6"):
        s = fixture_scorer(name, vocab, 0.8, 0.4)
        for beam in (1, 16, 17, 64, 65, 127, 128):
            for top_n in (1, 2, 40):
                both(p50, pd50, lens50, beam, 0.99, top_n, s, seen, "model %s beam %d top_n %d" % (name, beam, top_n))
                n_sc += 1
    assert seen[SCORER] == n_sc == 42
    print("with a scorer (orders 3 and 6): %d calls, device == host, all on path %d" % (n_sc, SCORER))
    # max_len below the hypotheses' lengths: ids cut alike, lens the true lengths
    s = fixture_scorer("6", vocab, 0.8, 0.4)
    for pp, ppd, ll, beam, sc in ((p, pd, lens, 4, None), (p, pd, lens, 40, None), (p50, pd50, lens50, 16, s)):
        d = both(pp, ppd, ll, beam, 0.99, 40, sc, seen, "max_len 3, beam %d" % beam, max_len=3)
        full = ctc_prefix_beam_decode(ppd, ll, beam, 0.99, 40, ext_scorer=sc)
        assert d[0].shape[-1] == 3 and d[1][:, 0].max() > 3 and (d[1] > 3).sum() >= 4, d[1][:, 0]
        assert np.array_equal(d[1], full[1]) and np.array_equal(d[2], full[2]) and np.array_equal(d[0], full[0][:, :, :3])
        print("max_len 3, beam %d%s: device == host, ids are the first 3 of the full result, best lengths %s" %
              (beam, " with a scorer" if sc else "", d[1][:, 0].tolist()))
    print("paths seen: %s" % dict(seen))


def tie_rows(rng, T, V):
    """probabilities in multiples of 1/16: sixteen classes of 1/16 each, or eight of them next to a blank of 8/16"""
    p = np.zeros((T, V), np.float32)
    for t in range(T):
        cls = rng.choice(V - 1, 16, replace=False)
        if t % 3 == 2:
            p[t, cls[:8]] = 1.0 / 16
            p[t, V - 1] = 8.0 / 16
        else:
            p[t, cls] = 1.0 / 16
    return p


def step_redo():
    """the one-key-per-thread kernel looks at the first beam + 2 candidates and has the radix path redo a frame when it cannot
    prove that no later candidate belongs in the beam: equal probabilities at the beam boundary are such frames"""
    os.environ["MI355ASR_BEAM_PROF"] = "1"                            # read once, at the library's first search
    seen = collections.Counter()
    rng = np.random.default_rng(3)
    V, T, beam = 300, 30, 8
    p = np.stack([tie_rows(rng, T, V), tie_rows(rng, T, V)])
    # host-side prediction: a frame with more than beam + 2 candidates whose candidates all score alike cannot be accepted
    predicted = sum(int((p[0, t] > 0).sum() > beam + 2 and len(set(p[0, t][p[0, t] > 0].tolist())) == 1) for t in range(1, T))
    assert predicted > 0
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            both(p, torch.from_numpy(p).cuda(), None, beam, 0.9999, 40, None, seen, "tied rows, beam %d" % beam)
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        err = f.read().decode("utf-8", "replace")
    sys.stderr.write(err)
    found = re.findall(r"beam (\d+), utterance 0: (\d+) frames \((\d+) redone by the radix path\)", err)
    assert len(found) == 1 and int(found[0][0]) == beam and int(found[0][1]) == T, err[-2000:]
    redone = int(found[0][2])
    print("tied rows: %d of %d frames redone by the radix path (the host-side analysis predicted at least %d); device == host" %
          (redone, T, predicted))
    assert seen[SMALL] == 1 and redone > 0
    print("paths seen: %s" % dict(seen))


def limit_probs(rng, V):
    """(2, 16, V): the mass of every frame on about 30 classes, among them V - 2, classes above 32 768, classes above 65 280 where
    V has any, and the blank"""
    B, T = 2, 16
    p = np.full((B, T, V), 1e-9, np.float32)
    for b in range(B):
        for t in range(T):
            cls = set(rng.integers(0, V - 1, 10).tolist()) | set(rng.integers(32769, V - 1, 12).tolist()) | {V - 2, V - 1}
            if V - 2 > 65280:
                cls |= set(rng.integers(65281, V - 1, 6).tolist())
            cls = sorted(cls)
            p[b, t, cls] = rng.uniform(0.2, 1.0, len(cls)).astype(np.float32)
            if t % 4 == 1:
                p[b, t, V - 2] = 3.0                                      # the last character wins some frames, the blank others
            if t % 4 == 3:
                p[b, t, V - 1] = 3.0
    return p / p.sum(-1, keepdims=True, dtype=np.float64).astype(np.float32)


def step_class_limit():
    seen = collections.Counter()
    rng = np.random.default_rng(21)
    for with_scorer in (False, True):
        limit = beam_device_limits(with_scorer)["max_classes"]
        assert limit > 32768
        for V in (limit, limit + 1):
            p = limit_probs(rng, V)
            pd = torch.from_numpy(p).cuda()
            s = None
            if with_scorer:                                            # order 3, hanzi-style: one character per class, a space, 300 classes the model lacks
                chars = [chr(0x20000 + i) for i in range(V - 1)]
                vocab = list(chars)
                vocab[7] = " "
                s = ngram.NGramScorer(0.15, 0.8, "synthetic", vocab, model=ngram.synthetic_model(chars[300:], 20000, 30000, seed=5))
            before = collections.Counter(seen)
            for beam in (8, 40):
                d = both(p, pd, None, beam, 0.999, 40, s, seen, "V %d beam %d%s" % (V, beam, " with a scorer" if s else ""))
                toks = d[0][d[0] >= 0]
                assert (toks == V - 2).any() and (toks > 32768).any() and (V - 2 <= 65280 or (toks > 65280).any())
            ran = sorted((seen - before).keys())
            assert ran == ([HOST] if V > limit else [SCORER] if s else [SMALL, RADIX]), (V, ran)
            print("V = %d (limit %d)%s: beams 8 and 40 ran paths %s and equal the host search" % (V, limit, ", scorer" if s else "", ran))
        # more candidates than the device search takes, one class past the limit: the selection kernel's rounds over a row of this length
        both(p, pd, None, 8, 0.999, 100, s, seen, "V %d top_n 100" % p.shape[-1])
        assert beam_last_path() == HOST
    print("paths seen: %s" % dict(seen))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    globals()["step_" + name]()
    torch.cuda.synchronize()
    print("step %s ok" % name)
