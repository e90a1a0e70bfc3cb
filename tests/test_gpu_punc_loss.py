"""The punctuation model's training outputs (Punc.heads, csrc/punc.hip), the punctuation trainer's losses with their gradients
(csrc/punc_loss.hip, tensorflowasr_amd/losses.py) and eval.PuncTester on the MI355X, against the float64 restatement
tests/punc_loss_ref.py.

Accuracy line (the one of tests/test_gpu_stft_loss.py): for each quantity the kernel's largest error against float64 over the case
set is at most 4 x the largest error of the same expression in float32 on the CPU over the same set -- torch float32 for the
losses (loss errors relative to |value64|, gradient errors relative to the row's largest |grad64|), tests/punc_numpy.py's
arithmetic run in float32 for the heads (errors relative to the sentence's largest |value64|); the yardstick's error is asserted
non-zero.
Case sets: heads -- sentences of 3, 16, 17, 143, 144, 145 and 1024 tokens (lds_tokens = 144: the last two keep their activations
in the workspace).  Classes loss -- C in {2, the shipped class count, 64} x Q' in {1, 63, 64, 65, 130} x B in {1, 3}, the logits
two tokens longer than the labels, as long, or three shorter in turn, with an upstream.  Feature loss -- F in {1, 3, 4, 5, 63, 64,
65, 768, 769} x T in {1, 2, 17}, B = 2, the prediction three tokens longer, as long, or two shorter in turn, -10 on scattered
elements and on the rows past a length, with an upstream.
Measured on one MI355X, largest error over the set, kernel / float32 yardstick / ratio (the accuracy tests print them):
  heads logits 8.18e-07 / 8.68e-07 / 0.94, heads feature 9.19e-07 / 5.00e-07 / 1.84;
  classes loss 5.17e-08 / 1.43e-06 / 0.036, its gradient 5.86e-08 / 9.54e-07 / 0.061;
  feature loss 4.97e-08 / 1.77e-07 / 0.28, its gradient 5.18e-08 / 1.36e-07 / 0.38 (the losses are summed in float64 and rounded
  once, so their error is the rounding to float32).
The fixture's inputs against the reference's float32 run: bd_loss within 2.2e-07, feature_map_loss within 9.7e-08 (relative);
PuncTester acc equal, bd_loss |d| 1.3e-06 (line 1.9e-04), feature_map_loss |d| 3.0e-08 (line 3.8e-04); against the float64 restatement on the kernel's own logits and feature bd_loss
2.9e-08 (line 5.8e-06) and feature_map_loss 8.8e-08 (line 8.3e-07), relative."""
import ctypes

import numpy as np
import pytest
import torch

import punc_loss_ref as R
from punc_onnx_eval import onnx_path
from test_punc_host import config
from test_punc_loss_host import GOLDEN, case_inputs

from tensorflowasr_amd import _lib, losses   # noqa: E402
from tensorflowasr_amd.eval import PuncTester   # noqa: E402
from tensorflowasr_amd.models import _p   # noqa: E402
from tensorflowasr_amd.punc import Punc   # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HEAD_LENGTHS = [3, 16, 17, 143, 144, 145, 1024]
CLASS_Q = [1, 63, 64, 65, 130]
FEATURE_F = [1, 3, 4, 5, 63, 64, 65, 768, 769]
FEATURE_T = [1, 2, 17]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def punc(gpu):
    p = Punc(config()).load_onnx(onnx_path())
    p._handle()
    assert p.lds_tokens == 144 and all(n in HEAD_LENGTHS for n in (143, 144, 145, p.max_tokens))
    return p


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def report(name, worst):
    for key, (mine, yard) in worst.items():
        print("%s accuracy %-8s kernel %.3e float32 %.3e ratio %.3f" % (name, key, mine, yard, mine / yard if yard else float("inf")))
    for key, (mine, yard) in worst.items():
        assert yard > 0.0, key
        assert mine <= 4.0 * yard, (key, mine, yard)


# ---- heads ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head_cases(punc):
    """every length once: ids, the float64 and the float32 NumPy outputs, and the kernel's solo run (host arrays)"""
    out = {}
    for i, n in enumerate(HEAD_LENGTHS):
        ids = R.seeded_ids([n], n, punc.cfg["vocab"], 40 + i)[0]
        l64, f64 = R.heads64(punc.weights, ids)
        l32, f32 = R.heads64(punc.weights, ids, dtype=np.float32)
        lg, ft = punc.heads(ids)
        out[n] = dict(ids=ids, l64=l64, f64=f64, l32=l32, f32=f32, lg=lg[0].cpu().numpy(), ft=ft[0].cpu().numpy(), lg_bits=bits(lg[0]), ft_bits=bits(ft[0]))
    return out


def test_heads_accuracy_line(head_cases):
    worst = {"logits": [0.0, 0.0], "feature": [0.0, 0.0]}
    for n, c in head_cases.items():
        assert c["lg"].shape == c["l64"].shape and c["ft"].shape == (n, 768) and np.isfinite(c["lg"]).all() and np.isfinite(c["ft"]).all()
        for key, got, y32, want in (("logits", c["lg"], c["l32"], c["l64"]), ("feature", c["ft"], c["f32"], c["f64"])):
            scale = np.abs(want).max()
            mine, yard = np.abs(got - want).max() / scale, np.abs(y32.astype(np.float64) - want).max() / scale
            print("heads T=%-4d %-7s kernel %.3e numpy-float32 %.3e" % (n, key, mine, yard))
            worst[key][0], worst[key][1] = max(worst[key][0], mine), max(worst[key][1], yard)
    report("heads", worst)


def test_softmax_of_the_logits_is_forward(punc, head_cases):
    for n, c in head_cases.items():
        probs, cls, _ = punc.forward(c["ids"])
        sm = torch.softmax(torch.from_numpy(c["lg"]).to(torch.float64), -1).numpy()
        assert np.abs(sm - probs[0].cpu().numpy()).max() <= 1e-6, n
        assert np.array_equal(c["lg"].argmax(-1), cls[0].cpu().numpy()), n


def raw_heads(punc, ids, lens, want_logits=True, want_feature=True):
    """the C call on poisoned output buffers -> (logits, feature) device tensors [B, T, .]"""
    h = punc._handle()
    x = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(h.device)
    ln = torch.from_numpy(np.asarray(lens, np.int32)).to(h.device)
    B, T = x.shape
    lg = torch.full((B, T, punc.cfg["classes"]), float("nan"), dtype=torch.float32, device=h.device) if want_logits else None
    ft = torch.full((B, T, 768), float("nan"), dtype=torch.float32, device=h.device) if want_feature else None
    n = ctypes.c_size_t()
    _lib.check(h.lib.mi355asr_punc_heads_workspace_bytes(h.ptr, B, T, ctypes.byref(n)))
    ws = h.workspace(n.value) if n.value else None
    with torch.cuda.device(h.device):
        _lib.check(h.lib.mi355asr_punc_heads(h.ptr, _p(x), _p(ln), B, T, _p(lg), _p(ft), _p(ws), n.value, h._stream()))
    return lg, ft


@pytest.mark.parametrize("rows", [[145, 3, 0, 16, 144, 17, 143], [17, 1024, 145]])
def test_ragged_rows_equal_their_solo_bits_and_the_rest_is_zero(punc, head_cases, rows):
    T = max(rows)
    ids = np.full((len(rows), T), 7, np.int32)               # padding ids in range; with explicit lengths they are never read as keys
    for b, n in enumerate(rows):
        if n:
            ids[b, :n] = head_cases[n]["ids"]
    lg, ft = raw_heads(punc, ids, rows)
    for b, n in enumerate(rows):
        if n:
            assert np.array_equal(bits(lg[b, :n]), head_cases[n]["lg_bits"]), (b, n)
            assert np.array_equal(bits(ft[b, :n]), head_cases[n]["ft_bits"]), (b, n)
        assert not bits(lg[b, n:]).any() and not bits(ft[b, n:]).any(), (b, n)
    only_l, none = raw_heads(punc, ids, rows, want_feature=False)
    none2, only_f = raw_heads(punc, ids, rows, want_logits=False)
    assert none is None and none2 is None and np.array_equal(bits(only_l), bits(lg)) and np.array_equal(bits(only_f), bits(ft))


def test_lengths_come_from_the_ids_and_interior_padding_is_refused(punc, head_cases):
    ids = np.zeros((2, 20), np.int32)
    ids[0, :17], ids[1, :3] = head_cases[17]["ids"], head_cases[3]["ids"]
    lg, ft = punc.heads(ids)
    assert np.array_equal(bits(lg[0, :17]), head_cases[17]["lg_bits"]) and np.array_equal(bits(ft[1, :3]), head_cases[3]["ft_bits"])
    assert not bits(lg[0, 17:]).any() and not bits(ft[1, 3:]).any()
    ids[1, 1] = 0
    with pytest.raises(ValueError, match="token 1 of row 1"):
        punc.heads(ids)


def test_forward_is_unchanged_by_heads_on_the_same_handle(punc, head_cases):
    ids = head_cases[145]["ids"]
    fresh = Punc(config()).load_onnx(onnx_path())
    first = [bits(t) for t in fresh.forward(ids)]                 # forward before any heads call on its handle
    other = Punc(config()).load_onnx(onnx_path())
    other.heads(ids)
    after = [bits(t) for t in other.forward(ids)]                 # heads first
    fresh.heads(head_cases[17]["ids"])
    again = [bits(t) for t in fresh.forward(ids)]
    for a, b, c in zip(first, after, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- classes loss -------------------------------------------------------------------------------------------------------------------
def classes_case(C, Q, B, i):
    """labels [B, Ql], logits [B, T, C] with min(T, Ql) = Q: the logits two longer, as long, three shorter in turn"""
    T, Ql = [(Q + 2, Q), (Q, Q), (Q, Q + 3)][i % 3]
    labels = R.seeded_labels((B, Ql), C, 60 + i)
    logits = R.seeded_logits((B, T, C), 60 + i)
    up = (0.5 + np.arange(B) * 0.75).astype(np.float32)
    return labels, logits, up


def expect_acc(acc64):
    """float32(acc) per row and the float64 mean of those float32 values, as the kernel forms it"""
    a32 = np.asarray(acc64).astype(np.float32)
    return a32, np.float32(a32.astype(np.float64).sum() / len(a32))


@pytest.fixture(scope="module")
def classes_accuracy(gpu, punc):
    worst = {"loss": [0.0, 0.0], "grad": [0.0, 0.0]}
    i = 0
    for C in (2, punc.cfg["classes"], 64):
        for Q in CLASS_Q:
            for B in (1, 3):
                labels, logits, up = classes_case(C, Q, B, i)
                i += 1
                l64, g64 = R.classes_loss(labels, logits), R.classes_grad(labels, logits, up)
                a32, m32 = expect_acc(R.classes_acc(labels, logits)[0])
                loss, grad = losses.punc_classes_loss(labels, torch.from_numpy(logits).to(gpu), return_grad=True, upstream=up)
                _, acc, mean, _ = losses._punc_classes_call(labels, logits)
                loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
                assert np.array_equal(acc.cpu().numpy(), a32, equal_nan=True) and np.array_equal(mean.cpu().numpy(), m32, equal_nan=True), (C, Q, B)
                assert float(losses.punc_classes_acc(labels, logits).cpu()) == pytest.approx(float(m32), nan_ok=True, abs=0)
                tx = torch.from_numpy(logits).requires_grad_(True)
                tl, _ = R.torch_classes(torch.from_numpy(labels), tx)
                (tl * torch.from_numpy(up)).sum().backward()
                tl, tg = tl.detach().numpy(), tx.grad.numpy()
                assert grad.shape == logits.shape and np.isfinite(grad).all()
                for b in range(B):
                    if l64[b] == 0.0:
                        assert loss[b] == 0.0
                    else:
                        worst["loss"][0], worst["loss"][1] = max(worst["loss"][0], rel(loss[b], l64[b])), max(worst["loss"][1], rel(tl[b], l64[b]))
                    scale = np.abs(g64[b]).max()
                    if scale == 0.0:
                        assert not grad[b].any()
                    else:
                        worst["grad"][0] = max(worst["grad"][0], np.abs(grad[b] - g64[b]).max() / scale)
                        worst["grad"][1] = max(worst["grad"][1], np.abs(tg[b] - g64[b]).max() / scale)
    return worst


def test_classes_accuracy_line(classes_accuracy):
    report("punc_classes_loss", classes_accuracy)


def run_classes(labels, logits_dev, up, gpu, grad=None):
    """the C call on a logits view and a caller's (poisoned) gradient buffer -> (loss, acc, mean, grad) device tensors"""
    B, T, C = logits_dev.shape
    y = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(gpu)
    g = torch.from_numpy(np.asarray(up, np.float32)).to(gpu) if up is not None else None
    loss, acc = (torch.full((B,), float("nan"), dtype=torch.float32, device=gpu) for _ in range(2))
    mean = torch.full((), float("nan"), dtype=torch.float32, device=gpu)
    if grad is None:
        grad = torch.full((B, T, C), float("nan"), dtype=torch.float32, device=gpu)
    losses.launch_punc_classes(_lib.lib(), y, logits_dev, g, B, y.shape[1], T, C, loss, acc, mean, grad, gpu)
    return loss, acc, mean, grad


def test_classes_special_rows(gpu, punc):
    C, Q, T = punc.cfg["classes"], 65, 67
    labels = R.seeded_labels((4, Q), C, 70)
    logits = R.seeded_logits((4, T, C), 70)
    labels[0] = 0                        # no label at all
    labels[1] = 1                        # "no mark" everywhere: the second term is 0
    labels[2, 5] = C                     # out of range
    labels[2, 6] = -1
    up = np.array([1.0, 2.0, 3.0, 0.25], np.float32)
    loss, acc, mean, grad = (t.cpu().numpy() for t in run_classes(labels, torch.from_numpy(logits).to(gpu), up, gpu))
    l64, g64 = R.classes_loss(labels, logits), R.classes_grad(labels, logits, up)
    assert loss[0] == 0.0 and np.isnan(acc[0]) and np.isnan(mean) and not grad[0].any()
    x = logits[1, :Q].astype(np.float64)
    first_term = (np.log(np.exp(x).sum(-1)) - x[:, 1]).sum() / (Q + 1e-6)
    assert rel(loss[1], first_term) <= 4 * U and rel(loss[1], l64[1]) <= 4 * U
    assert np.isnan(loss[2]) and not grad[2, 5].any() and not grad[2, 6].any() and np.isfinite(grad).all()
    assert rel(loss[3], l64[3]) <= 4 * U
    assert not grad[:, Q:].any() and not grad[:, :Q][labels == 0].any()
    for b in (1, 2, 3):
        assert np.abs(grad[b] - g64[b]).max() <= 4 * U * np.abs(g64[b]).max(), b
    assert np.array_equal(acc[1:], expect_acc(R.classes_acc(labels, logits)[0])[0][1:])


def test_classes_strided_view_poisoned_gradient_and_batch_invariance(gpu, punc):
    C, Q, T, B = punc.cfg["classes"], 130, 133, 3
    labels = R.seeded_labels((B, Q), C, 71)
    logits = R.seeded_logits((B, T, C), 71)
    up = np.array([0.5, 1.5, -2.0], np.float32)
    base = [bits(t) for t in run_classes(labels, torch.from_numpy(logits).to(gpu), up, gpu)]
    # the logits as a view into a larger buffer, the gradient into a larger poisoned buffer
    big = torch.full((B, T + 3, C + 5), float("nan"), dtype=torch.float32, device=gpu)
    big[:, 1:T + 1, 2:2 + C] = torch.from_numpy(logits).to(gpu)
    view = big[:, 1:T + 1, 2:2 + C]
    assert view.stride() == ((T + 3) * (C + 5), C + 5, 1)
    gbig = torch.full((B, T + 1, C + 3), float("nan"), dtype=torch.float32, device=gpu)
    out = run_classes(labels, view, up, gpu, grad=gbig[:, :T, :C])
    for a, t in zip(base, out):
        assert np.array_equal(a, bits(t))
    assert torch.isnan(gbig[:, T:]).all() and torch.isnan(gbig[:, :, C:]).all() and torch.isfinite(gbig[:, :T, :C]).all()
    # every row alone
    for b in range(B):
        solo = run_classes(labels[b:b + 1], torch.from_numpy(logits[b:b + 1]).to(gpu), up[b:b + 1], gpu)
        assert np.array_equal(bits(solo[0]), base[0][b:b + 1]) and np.array_equal(bits(solo[1]), base[1][b:b + 1])
        assert np.array_equal(bits(solo[3]), base[3][b:b + 1])


# ---- feature loss -------------------------------------------------------------------------------------------------------------------
def feature_case(F, T, i, B=2):
    T1, T2 = [(T, T + 3), (T, T), (T + 2, T)][i % 3]
    lengths = [T, max(T - 1, 0)] if i % 2 else None
    real, pred = R.seeded_features((B, T1, F), (B, T2, F), 80 + i, lengths, scatter=0.1)
    up = np.array([1.25, -0.5], np.float32)
    return real, pred, up


@pytest.fixture(scope="module")
def feature_accuracy(gpu):
    worst = {"loss": [0.0, 0.0], "grad": [0.0, 0.0]}
    i = 0
    for F in FEATURE_F:
        for T in FEATURE_T:
            real, pred, up = feature_case(F, T, i)
            i += 1
            v64, g64 = R.feature_loss(real, pred), R.feature_grad(real, pred, up)
            out, grad = losses.bert_feature_loss(real, torch.from_numpy(pred).to(gpu), return_grad=True, upstream=up)
            plain = losses.bert_feature_loss(real, pred)
            assert np.array_equal(bits(plain), bits(out))
            out, grad = out.cpu().numpy(), grad.cpu().numpy()
            tp = torch.from_numpy(pred).requires_grad_(True)
            tv = R.torch_feature(torch.from_numpy(real), tp)
            (tv * torch.from_numpy(up)).sum().backward()
            tv, tg = tv.detach().numpy(), tp.grad.numpy()
            assert grad.shape == pred.shape and np.isfinite(grad).all()
            Tm = min(real.shape[1], pred.shape[1])
            assert not grad[:, Tm:].any() and not grad[:, :Tm][real[:, :Tm] == -10].any()
            for b in range(2):
                if v64[b] == 0.0:
                    assert out[b] == 0.0
                else:
                    worst["loss"][0], worst["loss"][1] = max(worst["loss"][0], rel(out[b], v64[b])), max(worst["loss"][1], rel(tv[b], v64[b]))
                scale = np.abs(g64[b]).max()
                if scale == 0.0:
                    assert not grad[b].any()
                else:
                    worst["grad"][0] = max(worst["grad"][0], np.abs(grad[b] - g64[b]).max() / scale)
                    worst["grad"][1] = max(worst["grad"][1], np.abs(tg[b] - g64[b]).max() / scale)
    return worst


def test_feature_accuracy_line(feature_accuracy):
    report("bert_feature_loss", feature_accuracy)


def run_feature(real_dev, pred_dev, up, gpu, grad=None):
    B, T1, F = real_dev.shape
    T2 = pred_dev.shape[1]
    g = torch.from_numpy(np.asarray(up, np.float32)).to(gpu) if up is not None else None
    out = torch.full((B,), float("nan"), dtype=torch.float32, device=gpu)
    if grad is None:
        grad = torch.full((B, T2, F), float("nan"), dtype=torch.float32, device=gpu)
    losses.launch_feature_mse(_lib.lib(), real_dev, pred_dev, g, B, T1, T2, F, out, grad, gpu)
    return out, grad


@pytest.mark.parametrize("F", [5, 64, 768, 769])
def test_feature_masks_views_and_batch_invariance(gpu, F):
    B, T1, T2 = 3, 17, 19
    real, pred = R.seeded_features((B, T1, F), (B, T2, F), 90, [17, 9, 17], scatter=0.1)
    real[2] = -10                                          # a whole sentence masked: loss 0
    up = np.array([1.0, 3.0, -2.0], np.float32)
    r, p = torch.from_numpy(real).to(gpu), torch.from_numpy(pred).to(gpu)
    out, grad = run_feature(r, p, up, gpu)
    base = bits(out), bits(grad)
    v64, g64 = R.feature_loss(real, pred), R.feature_grad(real, pred, up)
    out, grad = out.cpu().numpy(), grad.cpu().numpy()
    assert out[2] == 0.0 and not grad[2].any() and not grad[:, T1:].any() and not grad[1, 9:].any() and np.isfinite(grad).all()
    assert not grad[:, :T1][real == -10].any()
    for b in (0, 1):
        assert rel(out[b], v64[b]) <= 4 * U and np.abs(grad[b] - g64[b]).max() <= 4 * U * np.abs(g64[b]).max()

    def same(o, g):
        assert np.array_equal(bits(o), base[0]) and np.array_equal(bits(g), base[1])
    # a base pointer off the 16-byte grid: views one float into flat buffers, the gradient likewise
    def shifted(a):
        flat = torch.full((a.numel() + 1,), float("nan"), dtype=torch.float32, device=gpu)
        flat[1:] = a.reshape(-1)
        v = flat[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4
        return v
    gflat = torch.full((B * T2 * F + 1,), float("nan"), dtype=torch.float32, device=gpu)
    same(*run_feature(shifted(r), shifted(p), up, gpu, grad=gflat[1:].view(B, T2, F)))
    assert torch.isnan(gflat[0])
    same(*run_feature(shifted(r), p, up, gpu))
    # strided views: the features inside wider rows and longer sentences, the gradient into a larger poisoned buffer
    rbig = torch.full((B, T1 + 2, F + 5), float("nan"), dtype=torch.float32, device=gpu)
    pbig = torch.full((B, T2 + 1, F + 3), float("nan"), dtype=torch.float32, device=gpu)
    rbig[:, 1:T1 + 1, 2:2 + F], pbig[:, :T2, 3:3 + F] = r, p
    gbig = torch.full((B, T2 + 2, F + 4), float("nan"), dtype=torch.float32, device=gpu)
    same(*run_feature(rbig[:, 1:T1 + 1, 2:2 + F], pbig[:, :T2, 3:3 + F], up, gpu, grad=gbig[:, :T2, :F]))
    assert torch.isnan(gbig[:, T2:]).all() and torch.isnan(gbig[:, :, F:]).all()
    # every row alone
    for b in range(B):
        o, g = run_feature(r[b:b + 1], p[b:b + 1], up[b:b + 1], gpu)
        assert np.array_equal(bits(o), base[0][b:b + 1]) and np.array_equal(bits(g), base[1][b:b + 1])


# ---- the train step's combination and the tester, on the fixture's inputs ------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_punc_losses_on_the_fixture_inputs(gpu, golden, classes_accuracy, feature_accuracy, k):
    """against the reference's float32 run: the kernel's line against float64 (4 x the yardstick) plus the distance of the
    float32 run itself from the float64 run"""
    labels, logits, real, pred = case_inputs(golden, k)
    out = losses.punc_losses(labels, real, torch.from_numpy(logits).to(gpu), pred, return_grad=True, global_batch_size=8)
    want = R.punc_losses(labels, real, logits, pred, global_batch_size=8)
    for key, fix, line in (("bd_loss", "bd", 4 * classes_accuracy["loss"][1]), ("feature_map_loss", "fm", 4 * feature_accuracy["loss"][1])):
        got, w32, w64 = out[key].cpu().numpy(), golden["%s32_%d" % (fix, k)], golden["%s64_%d" % (fix, k)]
        for b in range(len(w32)):
            print("fixture %d %s[%d]: kernel %.9g reference float32 run %.9g rel %.3e line %.3e + %.3e"
                  % (k, key, b, got[b], w32[b], rel(got[b], w32[b]), line, rel(w32[b], w64[b])))
            assert rel(got[b], w32[b]) <= line + rel(w32[b], w64[b])
    # exact up to the rounding of a mean of float32 values (the reference's float32 run adds them in float32)
    assert float(out["bd_acc"].cpu()) == expect_acc(R.classes_acc(labels, logits)[0])[1]
    assert rel(out["bd_acc"].cpu(), golden["acc64_%d" % k]) <= 2 * U and rel(out["bd_acc"].cpu(), golden["acc32_%d" % k]) <= 4 * U
    assert rel(out["train_loss"].cpu(), want["train_loss"]) <= 4 * max(classes_accuracy["loss"][1], feature_accuracy["loss"][1]) + U
    for key, line in (("grad_bd_pred", 4 * classes_accuracy["grad"][1]), ("grad_out_feature", 4 * feature_accuracy["grad"][1])):
        got = out[key].cpu().numpy()
        assert got.shape == want[key].shape
        for b in range(got.shape[0]):
            scale = np.abs(want[key][b]).max()
            assert np.abs(got[b] - want[key][b]).max() <= line * scale, (key, b)


def test_punc_tester_on_the_fixture_inputs(gpu, golden, punc, classes_accuracy, feature_accuracy):
    """acc is exact: the generator asserts a margin of 1e-3 between a token's two largest logits, three orders above the heads'
    error.  The losses: with d_l, d_f the heads' line on this input (4 x the largest error of the NumPy float32 run against float64),
    a token's cross-entropy moves by at most 2 d_l and classes_loss is a sum of two weighted means of it: 4 d_l; an element's
    (real - pred)^2 moves by at most 2 |real - pred| d_f + d_f^2, and the feature loss is a mean of means of it.  Plus the float32
    rounding of the result and the distance of the reference's float32 run from its float64 run."""
    lengths, seed = golden["tester_lengths"].tolist(), int(golden["tester_seed"])
    B, T, C = len(lengths), max(lengths), punc.cfg["classes"]
    ids = R.seeded_ids(lengths, T, punc.cfg["vocab"], seed)
    assert np.sum(ids, dtype=np.float64) == golden["sum_ids"]
    labels = R.seeded_labels((B, T), C, seed, lengths)
    real, _ = R.seeded_features((B, T, 768), (B, T, 768), seed, lengths)
    d_l = d_f = 0.0
    feat64 = np.zeros((B, T, 768))
    for b, n in enumerate(lengths):
        l64, feat64[b, :n] = R.heads64(punc.weights, ids[b, :n])
        l32, f32 = R.heads64(punc.weights, ids[b, :n], dtype=np.float32)
        d_l, d_f = max(d_l, 4 * np.abs(l32 - l64).max()), max(d_f, 4 * np.abs(f32 - feat64[b, :n]).max())
    assert d_l > 0 and d_f > 0
    tester = PuncTester(punc)
    step = tester.update(ids, labels, real)
    res = tester.results()
    assert set(res) == {"acc", "bd_loss", "feature_map_loss"} and res["acc"] == float(step["acc"].cpu())
    assert rel(res["acc"], golden["tester_acc64"]) <= 2 * U and rel(res["acc"], golden["tester_acc32"]) <= 4 * U
    bd32, bd64 = golden["tester_bd32"].mean(), golden["tester_bd64"].mean()
    fm32, fm64 = golden["tester_fm32"].mean(), golden["tester_fm64"].mean()
    used = (real != -10)
    gap = np.abs(np.where(used, real.astype(np.float64) - feat64, 0.0)).max()
    line_bd = 4 * d_l + 4 * U * abs(bd64) + abs(bd32 - bd64)
    line_fm = 2 * gap * d_f + d_f ** 2 + 4 * U * abs(fm64) + abs(fm32 - fm64)
    print("tester: acc %.9g  bd_loss %.9g (float32 run %.9g, |d| %.3e, line %.3e)  feature_map_loss %.9g (float32 run %.9g, |d| %.3e, line %.3e)"
          % (res["acc"], res["bd_loss"], bd32, abs(res["bd_loss"] - bd32), line_bd, res["feature_map_loss"], fm32,
             abs(res["feature_map_loss"] - fm32), line_fm))
    assert abs(res["bd_loss"] - bd32) <= line_bd
    assert abs(res["feature_map_loss"] - fm32) <= line_fm
    # the tighter check, which a wrong mask on a few tokens cannot pass: the float64 restatement on the kernel's OWN two outputs,
    # at the line of the two losses (4 x torch float32's largest error) plus the float32 rounding of the mean over the batch
    logits, feature = (t.cpu().numpy() for t in punc.heads(ids))
    own_bd, own_fm = R.classes_loss(labels, logits).mean(), R.feature_loss(real, feature).mean()
    own_acc = expect_acc(R.classes_acc(labels, logits)[0])[1]
    print("tester on its own outputs: bd_loss rel %.3e (line %.3e)  feature_map_loss rel %.3e (line %.3e)"
          % (rel(res["bd_loss"], own_bd), 4 * classes_accuracy["loss"][1] + 2 * U, rel(res["feature_map_loss"], own_fm),
             4 * feature_accuracy["loss"][1] + 2 * U))
    assert res["acc"] == float(own_acc)
    assert rel(res["bd_loss"], own_bd) <= 4 * classes_accuracy["loss"][1] + 2 * U
    assert rel(res["feature_map_loss"], own_fm) <= 4 * feature_accuracy["loss"][1] + 2 * U
    # without the teacher's features only acc and bd_loss are kept
    t2 = PuncTester(punc)
    s2 = t2.update(ids, labels)
    assert set(s2) == {"acc", "bd_loss"} and np.isnan(t2.results()["feature_map_loss"]) and t2.results()["bd_loss"] == res["bd_loss"]
