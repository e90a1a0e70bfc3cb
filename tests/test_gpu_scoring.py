"""The GPU scorer (tensorflowasr_amd/scoring.py, csrc/edit_distance.hip) on the MI355X: exact integers against the fixture
recorded from the reference's utils/xer.py, against answers known by construction, against eval.wer on host-filtered rows;
the alignment replayed; the refusals; and both testers with device scoring against their host loops."""
import ctypes

import numpy as np
import pytest
import torch

from test_scoring_host import edge_cases
from tensorflowasr_amd import _lib
from tensorflowasr_amd.eval import levenshtein, wer

pytestmark = pytest.mark.gpu
POISON = 113                      # fills everything past a row's length: a real id of every fixture alphabet would also do harm


@pytest.fixture(scope="module")
def ed():
    from tensorflowasr_amd.scoring import EditDistance
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    return EditDistance("cuda:0")


def ragged(rows, fill=POISON, width=None):
    out = np.full((len(rows), max(width or 0, max(len(r) for r in rows), 1)), fill, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32)


def run(ed, refs, hyps, **kw):
    (r, rl), (h, hl) = ragged(refs), ragged(hyps)
    return [t.cpu().numpy() for t in ed(r, h, rl, hl, **kw)]


def test_fixture_in_one_batch_reversed_and_one_per_call(ed):
    cases = [c for c in edge_cases() if c[0] != "max_len"]
    refs, hyps = [c[1] for c in cases], [c[2] for c in cases]
    want = np.array([c[3] for c in cases], np.int32)
    want_lens = np.array([[len(u), len(v)] for u, v in zip(refs, hyps)], np.int32)
    out, lens = run(ed, refs, hyps)
    bad = [cases[i][0] for i in np.nonzero((out != want).any(1))[0]]
    assert not bad, (bad, out[(out != want).any(1)], want[(out != want).any(1)])
    assert np.array_equal(lens, want_lens)
    out_r, lens_r = run(ed, refs[::-1], hyps[::-1])
    assert np.array_equal(out_r[::-1], want) and np.array_equal(lens_r[::-1], want_lens)
    for (name, u, v, w), wl in zip(cases, want_lens):
        o, l = run(ed, [u], [v])
        assert tuple(o[0]) == w and tuple(l[0]) == tuple(wl), name


def test_fixture_pair_at_max_len_in_a_call_of_its_own(ed):
    name, u, v, w = edge_cases()[-1]
    assert name == "max_len" and len(u) == len(v) == ed.MAX_LEN
    # no length vectors: the whole row counts
    out, lens = ed(u[None].astype(np.int32), v[None].astype(np.int32))
    assert tuple(out.cpu().numpy()[0]) == w and lens.cpu().tolist() == [[ed.MAX_LEN, ed.MAX_LEN]]


def constructed(n, seed):
    """ref = arange(n); hyp = ref with substitutions by unseen ids, deletions, and insertions of unseen ids, any two edits
    separated by at least three untouched tokens: every reference token is distinct, so the optimal alignment is unique and
    its (S, D, I) are the edits as built."""
    rng = np.random.default_rng(seed)
    ref = np.arange(n, dtype=np.int32)
    hyp, s, d, i, unseen, x = [], 0, 0, 0, n, 0
    while x < n:
        keep = int(rng.integers(3, 30))
        hyp.extend(range(x, min(x + keep, n)))
        x += keep
        if x >= n - 3:
            hyp.extend(range(x, n))
            break
        kind = int(rng.integers(0, 3))
        if kind == 0:
            hyp.append(unseen); unseen += 1; s += 1; x += 1
        elif kind == 1:
            d += 1; x += 1
        elif i < d:                                          # never more insertions than deletions: the hypothesis fits the row limit
            hyp.append(unseen); unseen += 1; i += 1
        else:
            d += 1; x += 1
    return ref, np.array(hyp, np.int32), (s + d + i, s, d, i)


def test_constructed_answers(ed):
    ref, hyp, want = constructed(600, 1)
    assert min(want[1:]) >= 5 and levenshtein(ref.tolist(), hyp.tolist()) == (want[0], want[1:])
    out, _ = run(ed, [ref], [hyp])
    assert tuple(out[0]) == want
    ref, hyp, want = constructed(16384, 2)
    assert min(want[1:]) >= 200 and len(hyp) == 16384 - want[2] + want[3] <= ed.MAX_LEN
    out, lens = run(ed, [ref], [hyp])
    assert tuple(out[0]) == want and lens.tolist() == [[16384, len(hyp)]]


def host_filter(row, drop, stop):
    row = [int(t) for t in row]
    if stop is not None and stop in row:
        row = row[:row.index(stop)]
    return [t for t in row if t not in drop]


@pytest.mark.parametrize("drop_ref,drop_hyp", [((), ()), ((0,), (0,)), ((0, 2, 5, 7), (0, 1, 3, 9))])
def test_filtering(ed, drop_ref, drop_hyp):
    rng = np.random.default_rng(7)
    stop = 1
    refs, hyps = [], []
    for k, (n, m) in enumerate([(40, 37), (5, 90), (130, 129), (64, 65), (1100, 1050), (12, 12), (30, 8), (9, 30)]):
        r, h = rng.integers(2, 10, n), rng.integers(2, 10, m)
        h[rng.integers(0, m, max(m // 6, 1))] = 0            # ids of the drop sets inside the rows
        r[rng.integers(0, n, max(n // 6, 1))] = 0
        refs.append(r); hyps.append(h)
    hyps[0][0] = stop                                        # a stop id at position 0: the hypothesis filters to nothing
    hyps[1][45] = stop; hyps[1][60] = stop                   # in the middle, twice: the first one cuts
    hyps[2][128] = stop                                      # the last token
    hyps[4][1030] = stop                                     # behind the first strip
    refs[5][:] = 0                                           # a reference of dropped ids only (when 0 is dropped)
    hyps[6][:] = [0, 3, 0, 9, 0, 1, 4, 4]                    # dropped ids in front of the stop
    # rows 3 and 7 hold no stop id; padding: copies of a real token, which would change the answer if read
    (r, rl), (h, hl) = ragged(refs, fill=4, width=1200), ragged(hyps, fill=4, width=1111)
    for use_stop in (stop, None, 0):                         # 0: the stop id equals a dropped id
        out, lens = [t.cpu().numpy() for t in ed(r, h, rl, hl, drop_ref=drop_ref, drop_hyp=drop_hyp, hyp_stop=use_stop)]
        for b in range(len(refs)):
            j, i = host_filter(refs[b], drop_ref, None), host_filter(hyps[b], drop_hyp, use_stop)
            assert lens[b].tolist() == [len(j), len(i)], (b, use_stop)
            dist, (s, d, ins) = levenshtein(j, i)
            assert out[b].tolist() == [dist, s, d, ins], (b, use_stop)
            if j:
                assert wer(j, i) == (out[b, 0] / len(j), out[b, 1], out[b, 2], out[b, 3])
            else:
                assert out[b].tolist() == [len(i), 0, 0, len(i)]
            if not i:
                assert out[b].tolist() == [len(j), 0, len(j), 0]
    assert host_filter(hyps[0], drop_hyp, stop) == []


def replay(u, v, ops):
    """ops applied to u must spell v; -> per-code counts"""
    ops = np.asarray(ops)
    x = np.cumsum(ops != 3) - (ops != 3)                     # reference position of every step
    y = np.cumsum(ops != 2) - (ops != 2)                     # hypothesis position of every step
    assert (ops <= 3).all() and (ops != 3).sum() == len(u) and (ops != 2).sum() == len(v)
    assert (u[x[ops == 1]] != v[y[ops == 1]]).all()
    emits = ops != 2                                         # a match copies the reference token, 1 and 3 write the hypothesis's
    spelled = np.where(ops[emits] == 0, np.append(u, 0)[x[emits]], np.append(v, 0)[y[emits]])
    assert np.array_equal(spelled, v)
    return [int((ops == c).sum()) for c in (1, 2, 3)]


def test_alignment_replays_and_counts(ed):
    cases = [c for c in edge_cases() if c[0] != "max_len"]
    small = [c for c in cases if len(c[1]) <= 300 and len(c[2]) <= 300]
    large = [c for c in cases if not (len(c[1]) <= 300 and len(c[2]) <= 300)]
    assert len(small) >= 81 and len(large) >= 12
    for group in (small, large):
        refs, hyps = [c[1] for c in group], [c[2] for c in group]
        assert max(map(len, refs)) * max(map(len, hyps)) <= ed.MAX_ALIGN_CELLS
        out, lens, ops, n_ops = run(ed, refs, hyps, return_ops=True)
        for b, (name, u, v, w) in enumerate(group):
            assert tuple(out[b]) == w, name
            assert n_ops[b] == len(u) + w[3], name
            assert replay(u, v, ops[b, :n_ops[b]]) == list(w[1:]), name


def test_confusion_table_of_a_batch(ed):
    from tensorflowasr_amd.scoring import confusions
    refs = [[4, 5, 6, 7, 8], [4, 5, 6]]
    hyps = [[4, 9, 6, 8, 3], [5, 6, 6]]
    out, lens, ops, n_ops = run(ed, refs, hyps, return_ops=True)
    sub, dele, ins = confusions(refs, hyps, ops, n_ops)
    assert sum(sub.values()) == out[:, 1].sum() and sum(dele.values()) == out[:, 2].sum() and sum(ins.values()) == out[:, 3].sum()
    assert sub.get((5, 9)) == 1


def test_refusals_leave_the_outputs_untouched(ed):
    dev = ed.device

    def attempt(N, M, with_ops, match):
        ref = torch.zeros((1, N), dtype=torch.int32, device=dev)
        hyp = torch.ones((1, M), dtype=torch.int32, device=dev)
        out = torch.full((1, 4), -77, dtype=torch.int32, device=dev)
        lens = torch.full((1, 2), -77, dtype=torch.int32, device=dev)
        ops = torch.full((1, 64), 201, dtype=torch.uint8, device=dev) if with_ops else None
        n_ops = torch.full((1,), -77, dtype=torch.int32, device=dev) if with_ops else None
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        empty = ctypes.c_int32 * 1
        with pytest.raises(_lib.Mi355AsrError, match=match):
            ed.launch(ref, None, hyp, None, empty(), 0, empty(), 0, None, out, lens, ops, n_ops, ws)
        torch.cuda.synchronize()
        assert (out == -77).all() and (lens == -77).all()
        if with_ops:
            assert (ops == 201).all() and (n_ops == -77).all()

    attempt(4097, 4096, True, "cells")                       # above MAX_ALIGN_CELLS with the alignment requested
    attempt(ed.MAX_LEN + 1, 8, False, "longer than")
    attempt(8, ed.MAX_LEN + 1, False, "longer than")
    with pytest.raises(_lib.Mi355AsrError, match="cells"):
        ed(np.zeros((1, 4097), np.int32), np.zeros((1, 4096), np.int32), return_ops=True)
    with pytest.raises(_lib.Mi355AsrError, match="drop set"):
        ed(np.zeros((1, 4), np.int32), np.zeros((1, 4), np.int32), drop_ref=(1, 2, 3, 4, 5))
    # the counts-only path keeps the full MAX_LEN beside a short row, and a batch of several such rows
    out, _ = ed(np.zeros((2, ed.MAX_LEN), np.int32), np.zeros((2, 3), np.int32))
    assert out.cpu().tolist() == [[ed.MAX_LEN - 3, 0, ed.MAX_LEN - 3, 0]] * 2


def test_score_transcripts_equals_wer(ed):
    from tensorflowasr_amd.scoring import score_transcripts
    refs = ["the cat sat on the mat", "abc", ["p1", "p2", "p3"], "x"]
    hyps = ["the cat sat on mat down", "", ["p1", "p3", "p3", "p4"], "x"]
    got = score_transcripts(refs, hyps)
    assert got == [wer(list(r), list(h)) for r, h in zip(refs, hyps)]


def _results_both_ways(make, step_batch):
    res = []
    for device_scoring in (False, True):
        t = make(device_scoring)
        t._eval_step(step_batch)
        t._eval_step(step_batch)                             # the accumulators run over steps
        res.append((t.results(), t))
    return res


def test_am_tester_device_scoring_gives_the_same_results(ed, tmp_path):
    from test_host import _eval_fixture
    from tensorflowasr_amd.eval import AMTester
    cfg = _eval_fixture(tmp_path, False)
    cfg["model_config"]["num_blocks"] = 2
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    rng = np.random.default_rng(11)
    B = 8
    x = np.zeros((B, 20480, 1), np.float32)
    in_len = np.zeros(B, np.int32)
    for b in range(B):
        L = int(rng.integers(9000, 20480))
        w = 0.3 * np.sin(np.arange(L) * (0.01 + 0.004 * b)) + 0.05 * rng.standard_normal(L)
        x[b, :L, 0] = w / np.abs(w).max()
        in_len[b] = L // 640
    ph = rng.integers(4, 24, (B, 9)).astype(np.int32)
    ph_len = rng.integers(3, 10, B).astype(np.int32)
    txt = rng.integers(4, 34, (B, 7)).astype(np.int32)
    for b in range(B):
        ph[b, ph_len[b]:] = 0                                # pad
        k = int(rng.integers(2, 7))
        txt[b, k] = 1; txt[b, k + 1:] = 0                    # </S>, then pad
    batch = (x, in_len, ph, ph_len, txt)
    bias = {}

    def make(device_scoring):
        t = AMTester(cfg, load_checkpoint=False, device_scoring=device_scoring)
        if not bias:                                         # a varied arg-max instead of one constant class
            enc = t.encoder(x, training=False)
            wc = t.ctc_model.get_weights_dict()
            logits, _ = t.ctc_model(enc, training=False, return_argmax=True, return_logits=True)
            bias["ctc"] = (np.asarray(wc["fully_connected/bias"], np.float32) - logits.mean(dim=(0, 1)).cpu().numpy()).astype(np.float32)
        wc = t.ctc_model.get_weights_dict()
        wc["fully_connected/bias"] = bias["ctc"]
        t.ctc_model.load_weights(wc, by_name=False)
        return t

    (host, th), (dev, td) = _results_both_ways(make, batch)
    print("host scoring:", host, "\ndevice scoring:", dev)
    assert host == dev and th.ctc_nums == td.ctc_nums and th.translator_nums == td.translator_nums
    assert th.ctc_nums[0] == 2 * int(ph_len.sum()) and sum(th.ctc_nums[1:]) > 0 and not th.device_scoring and td.device_scoring


def test_chunk_tester_device_scoring_gives_the_same_results(ed, tmp_path):
    from helpers import co
    from test_gpu_parity import _chunk_asr_config
    from tensorflowasr_amd.chunk_asr import ChunkAMTester
    cfg = dict(co.CHUNK_S, enc_num_blocks=2, picker_num_classes=31, decoder_num_classes=41)
    conf = _chunk_asr_config(tmp_path, cfg)
    w = co.chunk_weights(cfg, seed=3)
    B = 8
    xb = np.stack([co.synth_wave(20 + b, length=2560 * 6) for b in range(B)]).astype(np.float32)[..., None]
    rng = np.random.default_rng(5)
    labels = rng.integers(4, 40, (B, 6)).astype(np.int32)
    for b in range(B):
        labels[b, int(rng.integers(2, 7)):] = 0
    batch = (xb, np.full(B, 24, "int32"), None, None, labels, None)
    state = {}

    def make(device_scoring):
        t = ChunkAMTester(conf, load_checkpoint=False, device_scoring=device_scoring)
        t.runner.load_weights(w, by_name=False)
        if not state:                                        # the blank bias at the median gap: about half of the frames picked
            z = t.runner.predict(xb[..., 0], stages=True)["picker_logits"].cpu().numpy()
            gap = np.sort(z[..., :-1].max(-1) - z[..., -1], axis=None)
            state["bias"] = float(w["picker/fully_connected/bias"][-1] + gap[gap.size // 2])
        w2 = dict(w)
        w2["picker/fully_connected/bias"] = np.array(w["picker/fully_connected/bias"], np.float32)
        w2["picker/fully_connected/bias"][-1] = state["bias"]
        t.runner.load_weights(w2, by_name=False)
        return t

    (host, th), (dev, td) = _results_both_ways(make, batch)
    print("host scoring:", host, "\ndevice scoring:", dev)
    assert host == dev and th.ctc_nums == td.ctc_nums
    assert th.ctc_nums[0] == 2 * int((labels != 0).sum()) and sum(th.ctc_nums[1:]) > 0
