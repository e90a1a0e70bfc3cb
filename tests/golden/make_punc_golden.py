"""Writes tests/golden/punc_ref.npz: the committed punctuation graph (punc.onnx.part*, the reference's trained export)
evaluated by tests/punc_onnx_eval.py in float64 (`p64`, the parity reference) and in float32 (`p32`, what the reference's
own float32 run computes up to summation order), on

  rand_<T>   random ids in [3, vocab) between <S> and </S>, T tokens in all, at the kernel's tile and variant edges
  text_<k>   real sentences; `out_<k>` is the reference rule's output on p32 (punc_recover.py: argmax > 1 and max >= 0.65,
             indexing `vocab_array`)

    python tests/golden/make_punc_golden.py

A random draw is kept only if the reference alone leaves at most 2 % of its tokens undecided -- p64 within 1e-3 of a tie between its
two largest classes or of the 0.65 threshold -- since that is all a kernel within 1e-4 of p64 may be excused (tests/test_gpu_punc.py);
a draw that has more is replaced by the generator's next one.

LDS_TOKENS is the kernel's LDS / workspace switch (mi355asr_punc_limits); tests/test_gpu_punc.py checks the fixture has it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from punc_onnx_eval import Graph  # noqa: E402
from tensorflowasr_amd.featurizers import TextFeaturizer  # noqa: E402

LDS_TOKENS = 144
LENGTHS = [3, 4, 7, 8, 9, 16, 17, 33, 64, 65, LDS_TOKENS - 1, LDS_TOKENS, LDS_TOKENS + 1, 1024]
TEXTS = [
    "今天天气怎么样",
    "你好请问你叫什么名字",
    "我们明天去公园玩好不好",
    "他说他不知道这件事情是谁做的",
    "如果明天下雨我们就不去了在家里看电影吧",
    "这个问题很难回答但是我会尽力的",
    "我喜欢吃苹果香蕉和西瓜你呢",
    "请把门关上谢谢",
    "虽然他很累但是他还是坚持把工作做完了然后才回家休息",
    "北京是中国的首都有很多名胜古迹每年都有很多游客来这里参观旅游",
]
THRESHOLD = 0.65
MARGIN, EXCUSED = 1e-3, 0.02


def undecided(p64):
    """tokens whose float64 probabilities are within MARGIN of a tie or of the threshold"""
    top = np.sort(p64, -1)
    return int(((top[:, -1] - top[:, -2] < MARGIN) | (np.abs(top[:, -1] - THRESHOLD) < MARGIN)).sum())


def rule(txt, pred, vocab_array):
    out = []
    for t, b in zip(txt, pred):
        out.append(t)
        if b.argmax() > 1 and b.max() >= THRESHOLD:
            out.append(vocab_array[b.argmax()])
    return out


def decisions_agree(p32, p64):
    return bool(np.array_equal(p32.argmax(-1), p64.argmax(-1)) and np.array_equal(p32.max(-1) >= THRESHOLD, p64.max(-1) >= THRESHOLD))


def main():
    g = Graph()
    ch = TextFeaturizer({"vocabulary": os.path.join(HERE, "punc_tokens_ch.txt"), "blank_at_zero": True})
    bd = TextFeaturizer({"vocabulary": os.path.join(HERE, "punc_tokens_bd.txt"), "blank_at_zero": True})
    rng = np.random.default_rng(20240)
    out = {"lds_tokens": np.int32(LDS_TOKENS)}
    names = []

    def add(name, ids):
        ids = np.asarray(ids, np.int32)
        p64 = g.probs(ids[None], np.float64)[0]
        p32 = g.probs(ids[None], np.float32)[0]
        assert p64.dtype == np.float64 and p32.dtype == np.float32
        assert decisions_agree(p32, p64), "%s: float32 and float64 decide differently; replace it" % name
        out["ids_" + name], out["p64_" + name], out["p32_" + name] = ids, p64, p32
        names.append(name)
        return p32, p64

    for T in LENGTHS:
        while True:
            ids = np.concatenate([[ch.startid()], rng.integers(3, ch.num_classes, T - 2), [ch.endid()]])
            n = undecided(g.probs(ids[None].astype(np.int32), np.float64)[0])
            if n <= EXCUSED * T:
                break
            print("rand_%-5d redrawn: %d of %d tokens undecided in float64" % (T, n, T))
        _, p64 = add("rand_%d" % T, ids)
        print("rand_%-5d max p %.3f, %d undecided" % (T, p64.max(), n))
    marked = 0
    for k, txt in enumerate(TEXTS):
        assert 5 <= len(txt) <= 60
        ids = [ch.startid()] + ch.extract(txt) + [ch.endid()]
        p32, p64 = add("text_%d" % k, ids)
        res = rule(txt, p32[1:-1], bd.vocab_array)
        assert res == rule(txt, p64[1:-1], bd.vocab_array)
        assert undecided(p64) <= EXCUSED * len(ids), "text_%d: replace it" % k
        marked += len(res) > len(txt)
        out["txt_text_%d" % k] = np.array(txt)
        out["out_text_%d" % k] = np.array(res)
        print("text_%d %s" % (k, "".join(res)))
    assert len(TEXTS) >= 6 and marked >= 3, "only %d sentences get a punctuation mark" % marked
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "punc_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
