"""The float64 restatement tests/stft_loss_ref.py of the VAD trainer's losses, pinned on the host: against the reference's own
vad/utils/stft.py run on the stand-in (tests/golden/stft_loss_ref.npz, float64 to 1e-12 relative and float32 to 2e-6, the line
check_recipes.py uses for float32 fixtures), its analytic gradient against torch float64 autograd of the same graph, the mask
loss and the metrics against a direct loop; and the library exports the new entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import stft_loss_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_loss_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_reproduces_the_reference_run(golden, k):
    shape = tuple(int(v) for v in golden["shapes"][k])
    y, x = R.seeded_pair(shape, seed=k)
    assert np.sum(y, dtype=np.float64) == golden["sum_true_%d" % k] and np.sum(x, dtype=np.float64) == golden["sum_pred_%d" % k]
    sc, mag, frames = R.loss_rows(y.reshape(shape[0], -1), x.reshape(shape[0], -1))
    L = shape[1] * shape[2]
    assert frames.tolist() == [[1 + (L - 600) // 120, 1 + (L - 250) // 50]] * shape[0]
    value = R.scalar(sc, mag, frames)
    for got, key in ((value, "loss"), (sc.mean(0), "sc"), (mag.mean(0), "mag")):
        want64, want32 = golden["%s64_%d" % (key, k)], golden["%s32_%d" % (key, k)]
        assert np.all(np.abs(got - want64) <= 1e-12 * np.abs(want64)), key
        assert np.all(np.abs(got - want32) <= 2e-6 * np.abs(want32)), key


def test_argument_order_the_denominator_is_the_prediction():
    y, x = R.seeded_pair((1, 1200), seed=3)
    sc, _, _ = R.loss_rows(y, 2.0 * x)
    p = R.magnitude(R.spectrum(2.0 * x[0].astype(np.float64), 1024, 600, 120))
    t = R.magnitude(R.spectrum(y[0].astype(np.float64), 1024, 600, 120))
    assert sc[0, 0] == pytest.approx(np.linalg.norm(p - t) / (np.linalg.norm(p) + 1e-6), rel=1e-14)
    assert abs(sc[0, 0] - np.linalg.norm(p - t) / (np.linalg.norm(t) + 1e-6)) > 1e-3


torch_loss = R.torch_loss


@pytest.mark.parametrize("resolutions,lengths", [
    (R.RESOLUTIONS, [2400, 600, 250, 0, 1337]),
    (((2048, 2048, 512),), [4100, 2048]),
    (((512, 7, 3),), [40, 7, 6]),
])
def test_analytic_gradient_equals_autograd(resolutions, lengths):
    B, L = len(lengths), max(lengths) + 3
    y, x = R.seeded_pair((B, L), seed=11)
    value, grad = R.loss_and_grad(y, x, lengths, resolutions)
    ty = torch.tensor(y, dtype=torch.float64)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tv = torch_loss(ty, tx, lengths, resolutions)[0]
    tv.backward()
    assert value == pytest.approx(float(tv.detach()), rel=1e-12)
    ag = tx.grad.numpy()
    for b in range(B):
        scale = np.abs(ag[b]).max()
        assert np.abs(grad[b] - ag[b]).max() <= 1e-9 * scale
        assert np.all(grad[b, lengths[b]:] == 0.0)
    assert np.abs(ag).max() > 0


def test_mask_loss_and_metrics_agree_with_a_loop(golden):
    z, x = R.seeded_mask((2, 30, 1), seed=7)
    one, zero = R.mask_loss(z[..., 0], x[..., 0])
    assert one == pytest.approx(float(golden["mask_one"]), rel=1e-12) and zero == pytest.approx(float(golden["mask_zero"]), rel=1e-12)
    assert R.metrics(z[..., 0], x[..., 0])["acc"] == pytest.approx(float(golden["mask_acc"]), rel=1e-6)
    z, x = R.seeded_mask((3, 50), seed=5)
    x[0, 3], x[1, 0] = 0.5, 80.0
    lengths = [50, 17, 0]
    s = [0.0] * 4
    c = [0] * 4
    for b in range(3):
        for t in range(lengths[b]):
            xv, zv = float(x[b, t]), float(z[b, t])
            l = max(xv, 0.0) - xv * zv + math.log1p(math.exp(-abs(xv)))
            pos = xv > 0.5
            if zv == 1:
                s[0] += l; s[1] += 1; c[0] += pos; c[2] += not pos
            else:
                s[2] += l; s[3] += 1; c[1] += pos; c[3] += not pos
    sums, counts = R.mask_stats(z, x, lengths)
    assert np.allclose(sums, s, rtol=1e-13, atol=0) and counts.tolist() == c
    m = R.metrics(z, x, lengths=lengths)
    assert m["f1"] == pytest.approx(2 * c[0] / (2 * c[0] + c[1] + c[2])) and m["acc"] == pytest.approx((c[0] + c[3]) / sum(c))
    assert R.metrics(np.zeros((1, 4)), -np.ones((1, 4)))["f1"] == 0.0
    # the gradient against autograd of one_loss + zero_loss
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tz = torch.tensor(z, dtype=torch.float64)
    valid = torch.tensor(R._valid(z.shape, lengths))
    l = torch.clamp(tx, min=0) - tx * tz + torch.log1p(torch.exp(-tx.abs()))
    o, zz = valid & (tz == 1), valid & (tz == 0)
    ((l * o).sum() / (o.sum().double() + 1e-6) + (l * zz).sum() / (zz.sum().double() + 1e-6)).backward()
    assert np.abs(R.mask_grad(z, x, lengths) - tx.grad.numpy()).max() <= 1e-14


def test_library_exports_the_new_symbols():
    from tensorflowasr_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mi355asr_stft_loss_workspace_bytes", "mi355asr_stft_loss", "mi355asr_vad_mask_stats"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
