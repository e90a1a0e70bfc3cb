"""Softmax cross-entropy, arg-max, gradient, mask_loss / translate_acc and the tester's trainer metrics on the MI355X
(csrc/xent.hip, tensorflowasr_amd/losses.py) against the float64 restatement tests/xent_ref.py.

Bounds, u = 2^-24, S = ceil(V / 1024) the float4 slots of a thread:
    |loss - loss64|  <=  (16 + S + 3 ln V) u (1 + |max x| + |x_y| + |loss|)
    |grad - grad64|  <=  (20 + S + ln V) u |w|
and, independent of them, over the whole case set the largest loss error is at most 4 x the largest error of torch's float32 CPU
cross_entropy on the same inputs (checked to be non-zero).
Measured on one MI355X over the case set: largest loss error / bound 0.057 (V = 3), largest gradient error / bound 0.070, 0.097
with the mask_loss weights (V = 9 160); largest loss error against float64 1.93e-06 over the whole set and 1.42e-06 over the random
rows, torch's float32 CPU cross_entropy 1.08e-05 on both (its row of 262 144 classes decides it): 0.18 and 0.13 of it, the line
being 4."""
import ctypes
import math

import numpy as np
import pytest
import torch

import xent_ref as xr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLOT = 1024                     # elements per thread x threads: 4 x 256
RESIDENT = 10240                # rows up to here stay in registers
MAXV = 1 << 18
SWEEP = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1332, 2047, 2048, 2049, 9160, RESIDENT - 1, RESIDENT, RESIDENT + 1]


def loss_c(V):
    return 16 + math.ceil(V / SLOT) + 3 * math.log(V)


def grad_c(V):
    return 20 + math.ceil(V / SLOT) + math.log(V)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    from tensorflowasr_amd import losses
    assert (losses.RESIDENT_CLASSES, losses.MAX_CLASSES) == (RESIDENT, MAXV)
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


# ---- the case set -------------------------------------------------------------------------------------------------------------
def special_rows(V, rng):
    """-> x [1, 9, V] float32, labels [1, 9], the arg-max of every row"""
    mid, last = V // 2, V - 1
    x = (rng.standard_normal((9, V)) * 3).astype(np.float32)
    y = rng.integers(0, V, 9)
    x[0] = 0.75; y[0] = V // 3                                    # equal logits: log V
    y[1] = mid; x[1, mid] = -np.inf                               # x[y] = -inf, finite maximum: +inf
    x[2, mid] = 1e30; y[2] = mid                                  # maximum 1e30, at the label
    x[3, last] = 1e30; y[3] = 0                                   # maximum 1e30, elsewhere
    x[4] = -1e30 - np.abs(x[4]) * 1e30; x[4, mid] = -1e30; y[4] = mid       # maximum -1e30, at the label
    x[5] = -1e30 - np.abs(x[5]) * 1e30; x[5, 0] = -1e30; y[5] = last        # maximum -1e30, elsewhere
    x[6, [0, mid, last]] = 50.0                                   # ties: first, middle and last index -> first
    x[7, [mid, last]] = 50.0                                      # ties: middle and last -> middle
    x[8, last] = 50.0                                             # the last index alone
    amax = np.array([0, int(np.argmax(x[1])), mid, last, mid, 0, 0, mid, last])
    return x[None], y[None].astype(np.int32), amax[None]


def build_cases():
    cases = {}
    rng = np.random.default_rng(2024)

    def add(name, V, B, T, Q, pad):
        buf = (rng.standard_normal((B, T, V + pad)) * 3).astype(np.float32)
        if pad:
            buf[:, :, V:] = np.nan                                 # a read past V would poison the row
        if T > Q:
            buf[:, Q:] = np.nan                                    # and so would a read of a column t >= Q'
        cases[name] = dict(V=V, buf=buf, labels=rng.integers(0, V, (B, Q)).astype(np.int32), Q=Q,
                           w=rng.uniform(-2.0, 2.0, (B, Q)).astype(np.float32), random=True)

    for V in SWEEP:
        add("dense-%d" % V, V, 2, 2, 2, 0)                         # odd V: rows at addresses that are not 16-byte aligned
    for V in (5, 65, 1025, 1332, 9160, RESIDENT + 1):
        add("ld_t+3-%d" % V, V, 2, 2, 2, 3)
    for V in (3, 257, 1332, 9160, RESIDENT + 1):
        add("sliced-%d" % V, V, 2, 4, 2, 0)
    add("max-%d" % MAXV, MAXV, 1, 1, 1, 0)
    for V in (5, 1333, RESIDENT + 3):
        x, y, amax = special_rows(V, rng)
        cases["special-%d" % V] = dict(V=V, buf=x, labels=y, Q=9, w=rng.uniform(0.5, 2.0, (1, 9)).astype(np.float32), want_amax=amax,
                                       random=False)
    return cases


CASES = build_cases()
_ran = {}


def run(name):
    """the case on the GPU, once: loss, gradient (weighted), arg-max; with the float64 restatement and torch's float32 CPU loss"""
    if name not in _ran:
        from tensorflowasr_amd.losses import sparse_xent
        c = CASES[name]
        V, Q = c["V"], c["Q"]
        view = torch.from_numpy(c["buf"]).cuda()[:, :, :V]          # ld_t = V + pad, T columns
        loss, grad, amax = sparse_xent(view, c["labels"], weights=c["w"], return_grad=True, return_argmax=True)
        only = sparse_xent(view, c["labels"])
        x = c["buf"][:, :Q, :V]
        l64 = xr.sparse_xent(x, c["labels"])
        l32 = torch.nn.functional.cross_entropy(torch.from_numpy(np.ascontiguousarray(x)).reshape(-1, V),
                                                torch.from_numpy(c["labels"]).long().reshape(-1), reduction="none").numpy().reshape(l64.shape)
        _ran[name] = dict(c, x=x, loss=loss.cpu().numpy(), only=only.cpu().numpy(), grad=grad.cpu().numpy(), amax=amax.cpu().numpy(),
                          l64=l64, l32=l32, g64=xr.xent_grad(x, c["labels"], c["w"]))
    return _ran[name]


def finite_error(got, want):
    """max |got - want| where want is finite; got must equal want wherever want is infinite"""
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf].astype(np.float32)), (got[inf], want[inf])
    return np.abs(got.astype(np.float64) - want)[~inf] if (~inf).any() else np.zeros(1)


@pytest.mark.parametrize("name", list(CASES))
def test_loss_argmax_and_gradient_against_float64(gpu, name):
    r = run(name)
    V = r["V"]
    assert r["loss"].shape == r["l64"].shape and r["grad"].shape == r["g64"].shape
    assert np.array_equal(bits(torch.from_numpy(r["loss"])), bits(torch.from_numpy(r["only"]))), "the loss depends on the gradient pass"
    inf = np.isinf(r["l64"])
    bound = xr.loss_bound(loss_c(V), r["x"], r["labels"], r["l64"])
    err = np.where(inf, 0.0, np.abs(r["loss"].astype(np.float64) - np.where(inf, 0.0, r["l64"])))
    assert np.array_equal(r["loss"][inf], r["l64"][inf].astype(np.float32))
    gerr = np.abs(r["grad"] - r["g64"]).max(-1)
    gbound = grad_c(V) * U * np.abs(r["w"].astype(np.float64))
    print("%s: loss error / bound %.4f, gradient error / bound %.4f" % (name, (err / bound).max(), (gerr / gbound).max()))
    assert (err <= bound).all(), (name, err, bound)
    assert np.isfinite(r["grad"]).all() and (gerr <= gbound).all(), (name, gerr, gbound)
    assert np.array_equal(r["amax"], xr.argmax(r["x"])), name
    if "want_amax" in r:
        assert np.array_equal(r["amax"], r["want_amax"]), name


def test_error_against_torch_float32_over_the_case_set(gpu):
    e_gpu, e_t32, e_gpu_rand, e_t32_rand, ratio_l, ratio_g = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    for name in CASES:
        r = run(name)
        a, b = finite_error(r["loss"], r["l64"]).max(), finite_error(r["l32"], r["l64"]).max()
        e_gpu, e_t32 = max(e_gpu, a), max(e_t32, b)
        if r["random"]:
            e_gpu_rand, e_t32_rand = max(e_gpu_rand, a), max(e_t32_rand, b)
        inf = np.isinf(r["l64"])
        bound = xr.loss_bound(loss_c(r["V"]), r["x"], r["labels"], r["l64"])
        ratio_l = max(ratio_l, (finite_error(r["loss"], r["l64"]) / bound[~inf]).max())
        ratio_g = max(ratio_g, (np.abs(r["grad"] - r["g64"]).max(-1) / (grad_c(r["V"]) * U * np.abs(r["w"]))).max())
    print("whole set: loss max|d| %.3g, torch-float32 %.3g; random rows: %.3g, torch-float32 %.3g; largest error / bound: loss %.4f, "
          "gradient %.4f" % (e_gpu, e_t32, e_gpu_rand, e_t32_rand, ratio_l, ratio_g))
    assert e_t32 > 0 and e_t32_rand > 0, "torch's float32 run has no error on these inputs: the comparison says nothing"
    assert e_gpu <= 4 * e_t32
    assert e_gpu_rand <= 4 * e_t32_rand       # the rows with a maximum of 1e30 decide the line above; this one leaves them out


@pytest.mark.parametrize("V", [5, 1333, RESIDENT + 3])
def test_special_rows(gpu, V):
    r = run("special-%d" % V)
    loss, grad = r["loss"][0], r["grad"][0]
    assert abs(loss[0] - math.log(V)) <= 4 * U * math.log(V)              # equal logits (V is exact as a sum of ones)
    assert loss[1] == np.inf and np.isfinite(grad[1]).all()
    assert np.isfinite(loss[2:6]).all() and loss[2] == 0.0 and loss[4] == 0.0
    assert loss[3] == np.float32(1e30) and loss[5] > 0
    assert np.isfinite(grad).all()
    assert r["amax"][0].tolist() == r["want_amax"][0].tolist()
    one = np.zeros((1, 1, 1), np.float32) + 3.5                           # V = 1: loss 0, gradient 0
    from tensorflowasr_amd.losses import sparse_xent
    l1, g1, a1 = sparse_xent(one, np.zeros((1, 1), np.int32), return_grad=True, return_argmax=True)
    assert l1.item() == 0.0 and g1.item() == 0.0 and a1.item() == 0


def test_invalid_labels_are_nan_with_zero_gradient_and_nothing_else_is_touched(gpu):
    """labels -1 and V inside buffers whose surroundings are poisoned: NaN guard rows before and after the logits, NaN in the
    padding columns and in the columns t >= Q'; 0xFF-filled outputs with guards.  The loss is NaN, the gradient row 0, valid
    rows are right (so no poisoned input was read), and every byte the call does not own keeps its bits."""
    from tensorflowasr_amd import _lib, losses
    B, T, Q, V, PAD, G = 2, 4, 2, 1333, 3, 4096
    rng = np.random.default_rng(5)
    ld_t, ld_b = V + PAD, T * (V + PAD)
    core = np.full((B, T, ld_t), np.nan, np.float32)
    core[:, :Q, :V] = rng.standard_normal((B, Q, V)) * 3
    flat = torch.full((G + B * ld_b + G,), float("nan"), dtype=torch.float32, device=gpu)
    flat[G:G + B * ld_b] = torch.from_numpy(core).reshape(-1).cuda()
    labels = np.full((B, Q + 1), -1, np.int32)
    labels[:, :Q] = rng.integers(0, V, (B, Q))
    labels[0, 0], labels[1, 1] = -1, V
    lab = torch.from_numpy(labels).cuda()
    poison = lambda n, dt: torch.full((n,), -1, dtype=torch.int32, device=gpu).view(dt)
    loss, amax, grad = poison(G + B * Q + G, torch.float32), poison(G + B * Q + G, torch.int32), poison(G + B * ld_b + G, torch.float32)
    before = bits(grad)
    losses.launch_rows(_lib.lib(), flat[G:], lab, None, B, Q, V, loss[G:], amax[G:], grad[G:], gpu, ld=(ld_b, ld_t), gld=(ld_b, ld_t))
    torch.cuda.synchronize()
    for name, t in (("loss", loss), ("argmax", amax)):
        b = bits(t)
        assert (b[:G] == -1).all() and (b[G + B * Q:] == -1).all(), "a guard of %s was written" % name
    got = loss[G:G + B * Q].cpu().numpy().reshape(B, Q)
    want = xr.sparse_xent(core[:, :Q, :V], labels[:, :Q])
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 1]) and np.isnan(want[0, 0]) and np.isnan(want[1, 1])
    ok = ~np.isnan(want)
    assert (np.abs(got - want)[ok] <= xr.loss_bound(loss_c(V), core[:, :Q, :V], labels[:, :Q], want)[ok]).all()
    assert np.array_equal(amax[G:G + B * Q].cpu().numpy().reshape(B, Q), xr.argmax(core[:, :Q, :V]))
    after = bits(grad)
    g = grad[G:G + B * ld_b].cpu().numpy().reshape(B, T, ld_t)
    assert (g[0, 0, :V] == 0).all() and (g[1, 1, :V] == 0).all(), "the gradient row of an invalid label is zero"
    g64 = xr.xent_grad(core[:, :Q, :V], labels[:, :Q])
    assert (np.abs(g[:, :Q, :V] - g64) <= grad_c(V) * U).all()
    owned = np.zeros((B, T, ld_t), bool)
    owned[:, :Q, :V] = True
    keep = np.concatenate([np.ones(G, bool), ~owned.reshape(-1), np.ones(G, bool)])
    assert np.array_equal(after[keep], before[keep]), "a gradient element at t >= Q', past V or in a guard was written"


@pytest.mark.parametrize("V", [1333, 9160, RESIDENT + 3])
def test_a_row_gives_the_same_bits_alone_first_last_and_again(gpu, V):
    from tensorflowasr_amd.losses import sparse_xent
    rng = np.random.default_rng(V)
    row = (rng.standard_normal(V) * 3).astype(np.float32)
    y = int(rng.integers(0, V))
    others = (rng.standard_normal((3, V)) * 3).astype(np.float32)

    def call(x, labels, at):
        out = sparse_xent(x, labels, return_grad=True, return_argmax=True)
        return [bits(o.reshape(-1, o.shape[-1] if o.dim() == 3 else 1)[at]) for o in out]

    alone = call(row.reshape(1, 1, V), np.array([[y]], np.int32), 0)
    again = call(row.reshape(1, 1, V), np.array([[y]], np.int32), 0)
    # odd V: the rows 1, 2 and 3 of a dense batch start 4, 8 and 12 bytes past a 16-byte boundary
    for pos in (0, 1, 2, 3):
        batch = np.insert(others, pos, row, 0)                      # four rows, the row under test first .. last
        labels = np.zeros((batch.shape[0], 1), np.int32)
        labels[pos] = y
        got = call(batch.reshape(-1, 1, V), labels, pos)
        for a, g, what in zip(alone, got, ("loss", "gradient", "arg-max")):
            assert np.array_equal(a, g), "%s of the row differs at position %d of %d" % (what, pos, batch.shape[0])
    for a, g in zip(alone, again):
        assert np.array_equal(a, g)


def test_mask_loss_translate_acc_and_gradient(gpu):
    """mask_loss(return_grad=True) with a non-uniform upstream against torch float64 autograd of the restatement; Q' = min(T, Q)
    on both sides (T > Q: zero gradient columns; T < Q: unused label columns); logits as a strided view"""
    from test_xent_host import torch_mask_loss
    from tensorflowasr_amd.losses import mask_loss, translate_acc, translate_metrics
    rng = np.random.default_rng(11)
    for B, T, Q, V in ((3, 5, 4, 1333), (4, 3, 6, 257), (2, 20, 20, 9160)):
        Qp = min(T, Q)
        buf = (rng.standard_normal((B, T, V + 3)) * 3).astype(np.float32)
        x = buf[:, :, :V]
        y = rng.integers(0, 3, (B, Q)).astype(np.int32) * rng.integers(1, V // 2, (B, Q)).astype(np.int32)
        for b in range(B):                                          # a good share of correct predictions
            y[b, :Qp:2] = np.argmax(x[b, :Qp:2], -1)
        up = rng.uniform(-2.0, 3.0, B).astype(np.float32)
        view = torch.from_numpy(buf).cuda()[:, :, :V]
        out, grad = mask_loss(y, view, return_grad=True, upstream=up)
        plain = mask_loss(y, view)
        acc = translate_acc(y, view)
        mean, acc2 = translate_metrics(y, view)
        xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        o64 = torch_mask_loss(torch.from_numpy(y).long(), xt)
        (o64 * torch.from_numpy(up.astype(np.float64))).sum().backward()
        l64 = xr.sparse_xent(x, y)
        lb = xr.loss_bound(loss_c(V), x, y, l64)
        tol = lb.mean(-1) + 2 * lb.max() + U * np.abs(o64.detach().numpy())
        err = np.abs(out.cpu().numpy() - o64.detach().numpy())
        assert (err <= tol).all(), (err, tol)
        assert np.array_equal(bits(out), bits(plain))
        np.testing.assert_allclose(o64.detach().numpy(), xr.mask_loss(y, x), rtol=0, atol=1e-11)
        w = xr.mask_loss_weights(y, Qp, up)
        g = grad.cpu().numpy()
        assert g.shape == (B, T, V) and (g[:, Qp:] == 0).all()
        gerr = np.abs(g[:, :Qp] - xt.grad.numpy()[:, :Qp]).max(-1)
        print("V=%d: mask_loss error / tolerance %.4f, gradient error / bound %.4f" % (V, (err / tol).max(), (gerr / (grad_c(V) * U * np.abs(w))).max()))
        assert (gerr <= grad_c(V) * U * np.abs(w)).all()
        a64 = xr.translate_acc(y, x)
        assert a64 > 0.2 and abs(acc.item() - a64) <= 2 * U * a64 and bits(acc) == bits(acc2)
        assert abs(mean.item() - l64.mean()) <= lb.mean() + U * abs(l64.mean())


def test_ctc_acc_on_the_device(gpu):
    from tensorflowasr_amd.losses import ctc_acc
    rng = np.random.default_rng(3)
    for P, D in ((6, 4), (4, 4), (3, 7)):
        y = rng.integers(0, 4, (5, P)).astype(np.int32)
        d = rng.integers(0, 4, (5, D)).astype(np.int32)
        y[0] = 0                                                    # a row of pads: 0 / 1e-6
        got = ctc_acc(y, torch.from_numpy(d).cuda(), pad=0)
        want = xr.ctc_acc(y, d)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (5,)
        assert (np.abs(got.cpu().numpy() - want) <= 4 * U * want).all()


def test_refusals_leave_poisoned_outputs_alone(gpu):
    """every EINVAL of the two launching entries with real, poisoned device buffers: -1, a message that names the field, and the
    outputs keep their bits"""
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    B, Q, V = 2, 3, 20
    x = torch.randn((B, Q, V), device=gpu)
    lab = torch.zeros((B, Q), dtype=torch.int32, device=gpu)
    up = torch.ones((B,), device=gpu)
    poison = lambda *s: torch.full(s, -1, dtype=torch.int32, device=gpu)
    loss, amax, grad, out, scal, w, ws = poison(B, Q), poison(B, Q), poison(B, Q, V), poison(B), poison(2), poison(B, Q), poison(192)
    outputs = (loss, amax, grad, out, scal, ws)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def rows(**k):
        a = dict(x=p(x), ld_b=Q * V, ld_t=V, labels=p(lab), ld_lab=Q, w=p(w), B=B, Q=Q, V=V, loss=p(loss), amax=p(amax), grad=p(grad),
                 gld_b=Q * V, gld_t=V)
        a.update(k)
        return lib.mi355asr_xent_rows(a["x"], a["ld_b"], a["ld_t"], a["labels"], a["ld_lab"], a["w"], a["B"], a["Q"], a["V"], a["loss"],
                                      a["amax"], a["grad"], a["gld_b"], a["gld_t"], st)

    def ml(**k):
        a = dict(x=p(x), ld_b=Q * V, ld_t=V, labels=p(lab), ld_lab=Q, up=p(up), B=B, Q=Q, V=V, out=p(out), acc=p(scal[0:1]),
                 mean=p(scal[1:2]), grad=p(grad), gld_b=Q * V, gld_t=V, ws=p(ws), ws_bytes=768)
        a.update(k)
        return lib.mi355asr_mask_loss(a["x"], a["ld_b"], a["ld_t"], a["labels"], a["ld_lab"], a["up"], a["B"], a["Q"], a["V"], a["out"],
                                      a["acc"], a["mean"], a["grad"], a["gld_b"], a["gld_t"], a["ws"], a["ws_bytes"], st)

    null = ctypes.c_void_p()
    tried = [(rows, dict(x=null), "x_dev"), (rows, dict(labels=null), "labels_dev"), (rows, dict(loss=null), "loss_dev"),
             (rows, dict(V=0), "V=0"), (rows, dict(V=MAXV + 1, ld_t=MAXV + 1), "V="), (rows, dict(ld_t=V - 1), "ld_t"),
             (rows, dict(ld_b=-1), "ld_b"), (rows, dict(B=-1), "B="), (rows, dict(Q=-1), "Q="), (rows, dict(B=0), "B="),
             (rows, dict(ld_lab=Q - 1), "ld_lab"), (rows, dict(gld_t=V - 1), "gld_t"), (rows, dict(gld_b=Q * V - 1), "gld_b"),
             (ml, dict(x=null), "x_dev"), (ml, dict(labels=null), "labels_dev"), (ml, dict(out=null), "mask_loss_dev"),
             (ml, dict(acc=null), "acc_dev"), (ml, dict(mean=null), "mean_dev"), (ml, dict(ws=null), "ws_dev"),
             (ml, dict(V=0), "V=0"), (ml, dict(V=MAXV + 1, ld_t=MAXV + 1), "V="), (ml, dict(ld_t=V - 1), "ld_t"),
             (ml, dict(B=-1), "B="), (ml, dict(Q=-1), "Q="), (ml, dict(gld_t=V - 1), "gld_t"), (ml, dict(ws_bytes=767), "ws_bytes")]
    for fn, bad, word in tried:
        rc = fn(**bad)
        msg = lib.mi355asr_last_error().decode()
        assert rc == -1 and word in msg, (bad, rc, msg)
    torch.cuda.synchronize()
    for t in outputs:
        assert (t == -1).all(), "an output was written by a refused call"
    # the same buffers in a good call are written
    assert rows() == 0 and ml() == 0
    torch.cuda.synchronize()
    assert not (loss == -1).any() and not (out == -1).any() and not (scal == -1).any()


# ---- AMTester ----------------------------------------------------------------------------------------------------------------
def _tester(cfg, x, **kw):
    """the synthetic-weight tester of the existing tester tests, its CTC bias shifted so that the greedy decode varies"""
    from tensorflowasr_amd.eval import AMTester
    t = AMTester(cfg, load_checkpoint=False, **kw)
    enc = t.encoder(x, training=False)
    wc = t.ctc_model.get_weights_dict()
    logits0 = t.ctc_model(enc, training=False)
    wc["fully_connected/bias"] = (np.asarray(wc["fully_connected/bias"], np.float32) - logits0.mean(dim=(0, 1)).cpu().numpy()).astype(np.float32)
    t.ctc_model.load_weights(wc, by_name=False)
    return t


def test_am_tester_trainer_metrics(gpu, tmp_path):
    """AMTester(with_trainer_metrics=True): ctc_acc, translate_loss, translate_acc as CTCTrainer._eval_step updates them
    (ctc_runners.py:144-150), against xent_ref on the logits and ids the tester itself produced; three steps whose text labels are
    wider than, as wide as and narrower than the decoded ids (the min(T, Q) rule); SER / CER / S_I_D as with the switch off."""
    from test_host import _eval_fixture
    from tensorflowasr_amd.eval import EvalList
    cfg = _eval_fixture(tmp_path, False)
    cfg["model_config"]["num_blocks"] = 2
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    t = _tester(cfg, _first_features(cfg), with_trainer_metrics=True)
    ds = EvalList(cfg, t.speech_featurizer, t.phone_featurizer, t.text_featurizer, batch_size=3)
    x, in_len, ph, ph_len, txt = ds.eval_data_generator()
    t._eval_step((x, in_len, ph, ph_len, txt))
    width = t.last_trainer_inputs["ctc_decode"].shape[1]
    assert width >= 2, "the decode is too short to have a narrower label"
    V = t.text_featurizer.num_classes
    rng = np.random.default_rng(8)
    batches = []
    for Q in (width + 2, width, width - 1):
        lab = rng.integers(4, V, (3, Q)).astype(np.int32)
        lab[0, Q - 1:] = 1                                          # </S>, then pads
        lab[1, max(Q - 2, 1):] = 0
        batches.append((x, in_len, ph, ph_len, lab))
    for m in t.eval_metrics.values():                              # the probe step does not count
        m.reset_states()
    t.ctc_nums, t.translator_nums = [0, 0, 0, 0], [0, 0, 0, 0]
    t0 = _tester(cfg, x)
    want = {"ctc_acc": [], "translate_loss": [], "translate_acc": []}
    tol_loss = []
    for batch in batches:
        t._eval_step(batch); t.steps += 1
        t0._eval_step(batch); t0.steps += 1
        got = t.last_trainer_inputs
        logits, ids = got["translator_logits"].cpu().numpy(), got["ctc_decode"].cpu().numpy()
        assert logits.shape[1] == ids.shape[1] == width
        l64 = xr.sparse_xent(logits, batch[4])
        assert l64.shape == (3, min(width, batch[4].shape[1])) and np.isfinite(l64).all()
        want["translate_loss"].append(l64.mean())
        tol_loss.append(xr.loss_bound(loss_c(V), logits, batch[4], l64).mean() + U * abs(l64.mean()))
        want["translate_acc"].append(xr.translate_acc(batch[4], logits))
        want["ctc_acc"].extend(xr.ctc_acc(ph, ids, pad=t.text_featurizer.pad))
    r, r0 = t.results(), t0.results()
    print("trainer metrics", {k: r[k] for k in want}, "float64", {k: float(np.mean(v)) for k, v in want.items()})
    assert abs(r["translate_loss"] - np.mean(want["translate_loss"])) <= np.mean(tol_loss)
    assert abs(r["translate_acc"] - np.mean(want["translate_acc"])) <= 4 * U * max(np.mean(want["translate_acc"]), 1e-30)
    assert abs(r["ctc_acc"] - np.mean(want["ctc_acc"])) <= 4 * U * max(np.mean(want["ctc_acc"]), 1e-30)
    assert set(r0) == {"phone_ser", "phone_cer", "txt_ser", "txt_cer", "phone_s_i_d", "trans_s_i_d", "steps"}
    assert set(r) == set(r0) | {"ctc_acc", "translate_loss", "translate_acc"}
    assert all(r0[k] == r[k] for k in r0) and r["steps"] == 3


def _first_features(cfg):
    from tensorflowasr_amd.eval import EvalList
    from tensorflowasr_amd.featurizers import SpeechFeaturizer, TextFeaturizer
    ds = EvalList(cfg, SpeechFeaturizer(cfg["speech_config"]), TextFeaturizer(cfg["inp_config"]), TextFeaturizer(cfg["tar_config"]),
                  batch_size=3)
    return ds.eval_data_generator()[0]
