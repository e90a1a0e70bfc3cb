"""GPU tests of the punctuation restorer (punc.hip behind tensorflowasr_amd.punc.Punc): parity with the reference's exported
graph evaluated in float64 (tests/golden/punc_ref.npz), the decisions the text rule takes, ragged batches in both activation
variants (LDS up to lds_tokens tokens, the workspace beyond), determinism, the C ABI's caller contract on poisoned, fenced
buffers, and the sessions' hook.

Measured on an MI355X, max |probs - p64| per case (bound 1e-4):
  rand_3 3.0e-06  rand_4 3.1e-07  rand_7 5.2e-07  rand_8 6.8e-07  rand_9 5.6e-07  rand_16 1.1e-06  rand_17 3.4e-07  rand_33 1.3e-06
  rand_64 1.2e-06  rand_65 1.3e-06  rand_143 2.1e-06  rand_144 2.7e-06  rand_145 3.2e-06  rand_1024 4.4e-06
  text_0 .. text_9 2.6e-07 .. 1.2e-06; masked keys (id 0 inside a sentence) 8.4e-07.
Tokens excused from the decision check (p64 within 1e-3 of a tie or of 0.65): 1 of 144, 1 of 145, 10 of 1024, none elsewhere."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import vad_golden
from fence import fenced
from punc_numpy import punc_probs
from punc_onnx_eval import GOLDEN, onnx_path
from test_punc_host import _OneSegmentVad, _TextAsr, config

sys.path.insert(0, GOLDEN)
from make_stream_session_golden import StubRecogniser, StubScorer, packets   # noqa: E402

from tensorflowasr_amd import _lib   # noqa: E402
from tensorflowasr_amd.models import _p   # noqa: E402
from tensorflowasr_amd.punc import Punc   # noqa: E402
from tensorflowasr_amd.session import ASRSession   # noqa: E402
from tensorflowasr_amd.stream_session import StreamingASRSession   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the bound test_gpu_vad.py holds the same kind of kernel to
MARGIN = 1e-3       # a decision is held to p64's where p64 is at least this far from a tie and from 0.65
EXCUSED = 0.02


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(GOLDEN, "punc_ref.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def punc():
    return Punc(config()).load_onnx(onnx_path())


def _batch(id_rows, T=None):
    T = T or max(len(r) for r in id_rows)
    ids = np.full((len(id_rows), T), 7, np.int32)          # padding ids are in range and never read as keys
    for r, row in enumerate(id_rows):
        ids[r, :len(row)] = row
    return ids, np.array([len(r) for r in id_rows], np.int32)


@pytest.fixture(scope="module")
def solo(ref, punc):
    """every fixture case run alone, T = its own length: {case: (probs [T, C], cls [T], pmax [T])} on the host"""
    out = {}
    for n in ref["cases"]:
        p, c, m = punc.forward(ref["ids_" + n])
        out[n] = (p[0].cpu().numpy(), c[0].cpu().numpy(), m[0].cpu().numpy())
    return out


def test_limits_are_the_fixtures(ref, punc):
    punc._handle()
    assert punc.lds_tokens == int(ref["lds_tokens"]) and punc.max_tokens == 1024


def test_parity_with_the_reference_graph(ref, solo):
    worst = {}
    for n in ref["cases"]:
        worst[n] = float(np.abs(solo[n][0].astype(np.float64) - ref["p64_" + n]).max())
        print("punc parity %-10s max |p - p64| = %.2e" % (n, worst[n]))
    assert all(np.isfinite(solo[n][0]).all() for n in solo)
    assert max(worst.values()) <= TOL, worst


def test_decisions_equal_the_references(ref, solo):
    for n in ref["cases"]:
        p64, (p, cls, pmax) = ref["p64_" + n], solo[n]
        top = np.sort(p64, -1)
        firm = (top[:, -1] - top[:, -2] >= MARGIN) & (np.abs(top[:, -1] - 0.65) >= MARGIN)
        print("punc decisions %-10s excused %d of %d" % (n, int((~firm).sum()), len(firm)))
        assert (~firm).sum() <= EXCUSED * len(firm), n
        assert np.array_equal(cls[firm], p64.argmax(-1)[firm]), n
        assert np.array_equal((pmax >= 0.65)[firm], (p64.max(-1) >= 0.65)[firm]), n
        # cls / pmax are the arg-max and maximum of the probabilities as written
        assert np.array_equal(cls, p.argmax(-1)) and pmax.tobytes() == p.max(-1).tobytes(), n


def test_real_sentences_get_the_fixtures_punctuation(ref, punc):
    names = [n for n in ref["cases"] if n.startswith("text_")]
    texts = [str(ref["txt_" + n]) for n in names]
    want = [ref["out_" + n].tolist() for n in names]
    assert [punc.punc_recover(t) for t in texts[:3]] == want[:3]
    assert punc.punc_recover_batch(texts) == want
    assert punc(texts[0]) == want[0] and sum(len(w) > len(t) for w, t in zip(want, texts)) >= 3


def _check_rows(ref, solo, names, out, T):
    p, c, m = (t.cpu().numpy() for t in out)
    for r, n in enumerate(names):
        L = len(ref["ids_" + n])
        assert p[r, :L].tobytes() == solo[n][0].tobytes(), (r, n)
        assert c[r, :L].tobytes() == solo[n][1].tobytes() and m[r, :L].tobytes() == solo[n][2].tobytes(), (r, n)
        assert not p[r, L:].any() and not c[r, L:].any() and not m[r, L:].any(), (r, n)


def test_ragged_batch_of_every_length_equals_the_solo_rows(ref, solo, punc):
    """all the listed lengths in one call, both variants side by side: bitwise each row alone; twice: bitwise the same"""
    names = list(ref["cases"])
    ids, lens = _batch([ref["ids_" + n] for n in names])
    assert ids.shape[1] == 1024 and lens.min() == 3
    out = punc.forward(ids, lens)
    _check_rows(ref, solo, names, out, 1024)
    again = punc.forward(ids, lens)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_one_row_in_a_wider_call_equals_the_solo_row(ref, solo, punc):
    """B = 1, T above the row's length: the variant follows the row (lds_tokens: LDS, lds_tokens + 1: workspace), not T"""
    lds = punc.lds_tokens
    for n, T in (("rand_%d" % lds, 1024), ("rand_%d" % (lds + 1), 1024), ("rand_17", lds + 40), ("rand_3", 16)):
        ids, lens = _batch([ref["ids_" + n]], T)
        _check_rows(ref, solo, [n], punc.forward(ids, lens), T)


def test_three_hundred_rows_equal_their_solo_rows(ref, solo, punc):
    """more workgroups than compute units, lengths cycling through every case"""
    cases = list(ref["cases"])
    names = [cases[(5 * r) % len(cases)] for r in range(300)]
    ids, lens = _batch([ref["ids_" + n] for n in names])
    _check_rows(ref, solo, names, punc.forward(ids, lens), ids.shape[1])


def test_masked_and_out_of_range_ids(ref, punc):
    """an id 0 inside a sentence is a masked key (-1e9 on its logits), against the float64 restatement; an id outside the
    table is refused by the Python layer and clamped by the kernel"""
    ids = ref["ids_rand_33"].copy()
    ids[[4, 5, 20]] = 0
    got = punc.probs(ids)[0].cpu().numpy()
    want = punc_probs(punc.weights, ids)
    err = np.abs(got - want).max()
    print("punc masked keys max |p - p64| = %.2e" % err)
    assert err <= TOL
    for bad in (-1, 5039):
        with pytest.raises(ValueError):
            punc.probs(np.array([1, 5, bad, 2]))
    h = punc._handle()
    V = punc.cfg["vocab"]
    over = torch.tensor([[1, 9, V + 5, 2], [1, 9, V - 1, 2], [1, 9, -3, 2]], dtype=torch.int32, device=h.device)
    probs = torch.zeros((3, 4, 32), dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        _lib.check(h.lib.mi355asr_punc_forward(h.ptr, _p(over), None, 3, 4, _p(probs), None, None, None, 0, h._stream()))
    torch.cuda.synchronize()
    assert torch.equal(probs[0], probs[1])
    assert torch.isfinite(probs).all() and torch.allclose(probs.sum(-1), torch.ones(3, 4, device=h.device), atol=1e-5)


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_caller_contract_on_poisoned_fenced_buffers(ref, solo, fill):
    """outputs, ids and the workspace come from fenced allocations holding `fill`: nothing outside probs / cls / pmax and the
    stated workspace bytes is written, the workspace's contents on entry do not matter, a side stream gives the same bits, and
    cls / pmax may be null"""
    lds = int(ref["lds_tokens"])
    names = ["rand_%d" % (lds + 1), "rand_17", "rand_%d" % lds, "rand_3"]
    ids, lens = _batch([ref["ids_" + n] for n in names], lds + 9)
    p = Punc(config()).load_onnx(onnx_path())
    h = p._handle()
    with fenced(fill) as f:
        out = p.forward(ids, lens)
        assert h._ws is not None and h._ws.numel() == 4 * ((((lds + 16) * (4 * 68 + 1) + 63) // 64) * 64) * 4
        only = p.probs(ids, lens)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = p.forward(ids, lens)
        torch.cuda.synchronize()
        f.check()
        assert len(f.allocations) >= 8
    _check_rows(ref, solo, names, out, lds + 9)
    _check_rows(ref, solo, names, on_side, lds + 9)
    assert torch.equal(only, out[0])


def test_too_many_tokens_is_an_error_without_a_launch(punc):
    h = punc._handle()
    T = punc.max_tokens + 1
    ids = torch.ones((1, T), dtype=torch.int32, device=h.device)
    probs = torch.full((1, T, 32), -7.0, dtype=torch.float32, device=h.device)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=h.device)
    rc = h.lib.mi355asr_punc_forward(h.ptr, _p(ids), None, 1, T, _p(probs), None, None, _p(ws), ws.numel(), h._stream())
    assert rc == -1 and b"pe_input" in h.lib.mi355asr_last_error()
    n = ctypes.c_size_t()
    assert h.lib.mi355asr_punc_workspace_bytes(h.ptr, 1, T, ctypes.byref(n)) == -1
    torch.cuda.synchronize()
    assert bool((probs == -7.0).all())
    with pytest.raises(ValueError):
        punc.probs(np.ones(T, np.int32))
    # a workspace smaller than stated is refused too
    T = punc.lds_tokens + 1
    rc = h.lib.mi355asr_punc_forward(h.ptr, _p(ids), None, 1, T, _p(probs), None, None, _p(ws), 1024, h._stream())
    assert rc == -4


class _SentenceRecogniser(StubRecogniser):
    def __init__(self, text):
        super().__init__()
        self.text = text

    def decode(self, enc_features):
        return self.text


def test_sessions_return_the_reference_rules_text(ref, punc):
    txt, want = str(ref["txt_text_1"]), "".join(ref["out_text_1"].tolist())
    assert want != txt
    s = StreamingASRSession(_SentenceRecogniser(txt), StubScorer(), punc=punc)
    texts = []
    for pk in packets(vad_golden.composed_i16()[:16000 * 12], 320):
        e = s.send(pk)
        if e and "best_text" in e:
            texts.append(e["best_text"])
    e = s.final_send()
    if e and "best_text" in e:
        texts.append(e["best_text"])
    assert len(texts) >= 2 and set(texts) == {want}
    off = ASRSession(_TextAsr(txt), _OneSegmentVad(), punc=punc).send(np.zeros(32000, np.float32))
    assert [r["best_text"] for r in off] == [want]
