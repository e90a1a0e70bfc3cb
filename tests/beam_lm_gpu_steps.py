"""The GPU steps of tests/test_gpu_beam_lm.py, one per process: `python tests/beam_lm_gpu_steps.py STEP [TMPDIR]`.  A step
prints what it measured and exits non-zero on the first mismatch; it is never repeated."""
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

from tensorflowasr_amd import ngram                                    # noqa: E402
from tensorflowasr_amd.models import beam_last_path, ctc_prefix_beam_decode   # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
ARPA = {3: os.path.join(GOLDEN, "lm_small.arpa"), 4: os.path.join(GOLDEN, "lm_small4.arpa")}
NAMES = ("ids", "lens", "scores", "n_hyp")
PATH_HOST, PATH_SMALL, PATH_RADIX, PATH_SCORER = 1, 2, 3, 4            # mi355asr_beam_last_path


def ran(path, what):
    """the search the last device-side call ran: every path returns the same arrays, so equality alone cannot tell"""
    got = beam_last_path()
    assert got == path, "%s: ran path %d, expected %d" % (what, got, path)
HANZI_CLASSES = 9160                                                   # the ChunkConformer's text head: 9 159 characters + blank


def same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        bad = np.argwhere(np.asarray(x) != np.asarray(y))
        assert bad.size == 0, "%s: %s differ at %s (%d entries)" % (what, name, bad[:3].tolist(), len(bad))


def hanzi_scorer(alpha, beta, n2=150000, n3=350000):
    chars = [chr(0x4E00 + i) for i in range(HANZI_CLASSES - 1)]
    vocab = list(chars)
    vocab[7] = " "                                                     # a space class, and a tail of classes the model lacks
    return ngram.NGramScorer(alpha, beta, "synthetic", vocab, model=ngram.synthetic_model(chars[:-300], n2, n3, seed=5))


def config5_batch(seed, T=500, B=16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn((B, T, HANZI_CLASSES), generator=g) * 3.0
    z[..., -1] += 6.0                                                  # blank-leaning, like a CTC model
    lens = torch.randint(2 * T // 5, T + 1, (B,), generator=g).to(torch.int32)   # ragged: 200 … 500 at the config-5 shape
    lens[B // 5] = T                                                   # one full utterance and one empty one (3 and 5 of 16)
    lens[B // 3] = 0
    return torch.softmax(z, -1), lens.numpy()


def step_lm_score():
    for order in (3, 4):
        K = np.load(os.path.join(GOLDEN, "beam_lm_kat.npz"))
        s = ngram.NGramScorer(1.0, 0.0, ARPA[order], json.loads(str(K["vocabulary"])))
        rng = np.random.default_rng(order)
        n_words = len(s.model.words)
        ids = rng.integers(0, n_words + 1, size=(20000, order)).astype(np.int32)
        seen = np.concatenate([np.pad(s.model.ids[k], ((0, 0), (order - 1 - k, 0)), constant_values=s.bos_word) for k in range(order)])
        ids = np.concatenate([ids, seen])
        host, dev = s.score_ids(ids), s.score_ids(ids, on_device=True)
        assert np.array_equal(host.view(np.int32), dev.view(np.int32)), np.argwhere(host != dev)[:5]
        print("order %d: device mi355asr_lm_score == host on %d n-grams (%d OOV)" % (order, len(ids), int((host == -1000).sum())))
    chars = [chr(0x4E00 + i) for i in range(9000)]                      # order 5 over 9 000 words: hashed keys
    m = ngram.synthetic_model(chars, 30000, 30000, seed=3, higher=(20000, 10000))
    s = ngram.NGramScorer(1.0, 0.0, "synthetic", chars[:50], model=m)
    rng = np.random.default_rng(4)
    ids = np.concatenate([np.pad(m.ids[k], ((0, 0), (4 - k, 0)), constant_values=s.bos_word) for k in range(5)] +
                         [np.concatenate([rng.integers(4, 9000, (20000, 1)).astype(np.int32), m.ids[3]], 1)])
    host, dev = s.score_ids(ids), s.score_ids(ids, on_device=True)
    assert np.array_equal(host.view(np.int32), dev.view(np.int32))
    print("order 5, hashed keys: device == host on %d n-grams" % len(ids))
    s = hanzi_scorer(1.0, 0.0)
    rng = np.random.default_rng(9)
    ids = rng.integers(0, len(s.model.words) + 1, size=(50000, 3)).astype(np.int32)
    ids = np.concatenate([ids, s.model.ids[2][:50000], np.pad(s.model.ids[1][:50000], ((0, 0), (1, 0)), constant_values=s.bos_word)])
    host, dev = s.score_ids(ids), s.score_ids(ids, on_device=True)
    assert np.array_equal(host.view(np.int32), dev.view(np.int32))
    print("hanzi model (%d n-grams): device == host on %d n-grams" % (sum(s.model.counts), len(ids)))


def step_fixtures():
    K = np.load(os.path.join(GOLDEN, "beam_lm_kat.npz"))
    vocab = json.loads(str(K["vocabulary"]))
    sc = {o: ngram.NGramScorer(1.0, 0.0, ARPA[o], vocab) for o in ARPA}
    done = 0
    for i, m in enumerate(json.loads(str(K["meta"]))):
        if not (m["cutoff_prob"] < 1.0 and m["beam"] <= 128 and m["cutoff_top_n"] <= 40):
            continue                                                   # the device entry point takes pruned searches only
        s = sc[m["order"]]
        s.alpha, s.beta = m["alpha"], m["beta"]
        p = K["probs_%d" % i][None]
        host = ctc_prefix_beam_decode(p, None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], num_threads=1, ext_scorer=s)
        dev = ctc_prefix_beam_decode(torch.from_numpy(p).cuda(), None, m["beam"], m["cutoff_prob"], m["cutoff_top_n"], ext_scorer=s)
        ran(PATH_SCORER, "fixture case %d" % i)
        same(dev, host, "fixture case %d %s" % (i, m))
        assert np.array_equal(dev[2][0, :m["n"]].astype(np.float64), K["scores_%d" % i]), i      # and so the reference's scores
        done += 1
    assert done >= 10
    print("device search == host search == the reference's scores on %d fixture cases" % done)


def step_config5():
    probs, lens = config5_batch(1)
    pd = probs.cuda()
    ph = probs.numpy()
    for beam in (10, 100):
        for alpha, beta in ((0.8, 0.4), (0.0, 0.0)):
            s = hanzi_scorer(alpha, beta)
            dev = ctc_prefix_beam_decode(pd, lens, beam, 0.99, 40, ext_scorer=s)
            ran(PATH_SCORER, "config 5 beam %d alpha %g" % (beam, alpha))
            host = ctc_prefix_beam_decode(ph, lens, beam, 0.99, 40, ext_scorer=s, num_threads=16)
            same(dev, host, "config 5 beam %d alpha %g" % (beam, alpha))
            print("config 5 batch, beam %d, alpha %g beta %g: device == host on %d hypotheses; best lengths %s" %
                  (beam, alpha, beta, int(host[3].sum()), host[1][:4, 0].tolist()))
        dev0 = ctc_prefix_beam_decode(pd, lens, beam, 0.99, 40)
        ran(PATH_SMALL if beam == 10 else PATH_RADIX, "config 5 beam %d scorer-less" % beam)
        host0 = ctc_prefix_beam_decode(ph, lens, beam, 0.99, 40, num_threads=16)
        same(dev0, host0, "config 5 beam %d scorer-less" % beam)
        assert not np.array_equal(dev0[2], dev[2])
        print("config 5 batch, beam %d: the scorer-less device search still equals the host search" % beam)


def step_fallback():
    probs, lens = config5_batch(2, T=120, B=4)
    s = hanzi_scorer(0.8, 0.4)
    for beam, topn in ((130, 40), (10, 50)):
        dev = ctc_prefix_beam_decode(probs.cuda(), lens, beam, 0.99, topn, ext_scorer=s)
        ran(PATH_HOST, "fallback beam %d top_n %d" % (beam, topn))
        host = ctc_prefix_beam_decode(probs.numpy(), lens, beam, 0.99, topn, ext_scorer=s, num_threads=4)
        same(dev, host, "fallback beam %d top_n %d" % (beam, topn))
        print("beam %d, cutoff_top_n %d (outside the device search): the call ran the host search and agrees" % (beam, topn))


def _chunk_setup(tmp):
    from helpers import co
    from test_gpu_chunk_streams import _chunk_asr_config
    import pathlib
    cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41)
    conf = _chunk_asr_config(pathlib.Path(tmp), cfg)
    return cfg, conf


def step_pipeline(tmp):
    from helpers import chunk_config_dict, co, waves
    from tensorflowasr_amd.models import ChunkBeamPipeline, ChunkConformer
    cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41)
    m = ChunkConformer(chunk_config_dict(cfg), cfg["picker_num_classes"], cfg["decoder_num_classes"])
    m.load_weights(co.chunk_weights(cfg, seed=3), by_name=False)
    vocab = [" "] + [chr(0x4E00 + 7 * i) for i in range(39)]           # 40 classes, most of them words of the fixture model
    s = ngram.NGramScorer(0.6, 0.5, ARPA[3], vocab)
    x = waves(4, 2560 * 24, 200)
    xs = [x, x[::-1].copy(), x]
    pipe = ChunkBeamPipeline(m, beam_width=10, cutoff_prob=0.99, cutoff_top_n=40, ext_scorer=s)
    outs = [pipe.push(xx) for xx in xs] + [pipe.flush()]
    pipe.close()
    assert outs[0] is None
    for xx, res in zip(xs, outs[1:]):
        lgs, cs = m.predict(xx)
        seq = ctc_prefix_beam_decode(lgs, cs, 10, 0.99, 40, is_logits=True, ext_scorer=s)
        ran(PATH_SCORER, "pipeline, sequential call")
        same(res, seq, "pipeline")
        plain = ctc_prefix_beam_decode(lgs, cs, 10, 0.99, 40, is_logits=True)
        ran(PATH_SMALL, "pipeline, scorer-less call")
    assert not np.array_equal(plain[2], seq[2])
    print("ChunkBeamPipeline with a scorer == the sequential calls on 3 batches; frames per utterance %s" % cs.tolist())


def step_chunk_asr(tmp):
    import wave
    from helpers import co
    from tensorflowasr_amd.chunk_asr import ChunkASR
    cfg, conf = _chunk_setup(tmp)
    conf["tar_config"]["beam_width"] = 4
    chars = ["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4E00 + 7 * i) for i in range(36)]
    with open(conf["tar_config"]["vocabulary"], "w", encoding="utf-8") as f:
        f.write("\n".join(chars) + "\n")
    conf["tar_config"]["lm_config"] = {"lm_path": ARPA[3], "alpha": 0.6, "beta": 0.5}
    asr = ChunkASR(conf, load_checkpoint=False)
    assert asr.text_featurizer.scorer is not None and asr.text_featurizer.num_classes == 41
    asr.runner.load_weights(co.chunk_weights(cfg, seed=3), by_name=False)
    x = co.synth_wave(5, length=2560 * 24)
    path = os.path.join(tmp, "u.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
    text = asr.offline_stt(path)
    logits, _ = asr.runner.predict(asr.load_wav(path).reshape([1, -1, 1]))
    ids, lens, sc, n = ctc_prefix_beam_decode(logits, None, 4, is_logits=True, ext_scorer=asr.text_featurizer.scorer)
    ran(PATH_SCORER, "ChunkASR's search")
    want = "".join(asr.text_featurizer.iextract([int(t) for t in ids[0, 0, :lens[0, 0]] if t != 0]))
    assert text == want, (text, want)
    conf["tar_config"]["beam_width"] = 1
    greedy = ChunkASR(conf, load_checkpoint=False)
    greedy.runner.load_weights(co.chunk_weights(cfg, seed=3), by_name=False)
    print("ChunkASR beam_width 4 + lm_config: %r (%d frames, score %.4f); greedy: %r" % (text, logits.shape[1], sc[0, 0], greedy.offline_stt(path)))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    fn = globals()["step_" + name]
    fn(*sys.argv[2:3])
    torch.cuda.synchronize()
    print("step %s ok" % name)
