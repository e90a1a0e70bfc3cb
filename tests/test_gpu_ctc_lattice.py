"""CTC loss, its gradient and forced alignment on the MI355X (csrc/ctc_lattice.hip) against torch.nn.functional.ctc_loss on the
CPU in float64 fed log_softmax(log(softmax(z) + 1e-7)) -- the chain of tf.keras.backend.ctc_batch_cost -- and a float64 NumPy
Viterbi (tests/ctc_yardstick.py; both pinned against brute force in tests/test_ctc_lattice_host.py).

The ceiling on an error against float64 is max(4 x E32, 16 x 2^-23 x max|value|), E32 being the error of torch's own float32
CPU run of the same chain on the same inputs, computed here at run time; each test prints both errors."""
import os

import numpy as np
import pytest
import torch

import ctc_yardstick as cy

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    return torch.device("cuda:0")


_cache = {}


def case(name):
    """the inputs of a case with the float64 yardstick and torch's float32 run of it"""
    if name not in _cache:
        z, lab, il, ll = cy.make_case(**cy.CASES[name])
        l64, g64 = cy.torch_chain(z, lab, il, ll)
        l32, g32 = cy.torch_chain(z, lab, il, ll, dtype=torch.float32)
        _cache[name] = dict(z=z, lab=lab, il=il, ll=ll, l64=l64, g64=g64, e_loss=float(np.abs(l32 - l64).max()),
                            e_grad=float(np.abs(g32 - g64).max()))
    return _cache[name]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("name", list(cy.CASES))
def test_loss_and_gradient_against_float64(gpu, name):
    from tensorflowasr_amd.models import ctc_loss
    c = case(name)
    loss, grad = ctc_loss(c["z"], c["lab"], c["il"], c["ll"], return_grad=True)
    only = ctc_loss(c["z"], c["lab"], c["il"], c["ll"])
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    assert loss.shape == c["l64"].shape and grad.shape == c["g64"].shape and loss.dtype == np.float32
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    e_loss, e_grad = float(np.abs(loss - c["l64"]).max()), float(np.abs(grad - c["g64"]).max())
    b_loss, b_grad = cy.bound(c["e_loss"], c["l64"]), cy.bound(c["e_grad"], c["g64"])
    print("%s: loss max|d| gpu %.3g torch-f32 %.3g bound %.3g (max|loss| %.4g, rel %.3g); grad max|d| gpu %.3g torch-f32 %.3g "
          "bound %.3g (max|grad| %.3g)" % (name, e_loss, c["e_loss"], b_loss, np.abs(c["l64"]).max(),
                                           float((np.abs(loss - c["l64"]) / np.maximum(np.abs(c["l64"]), 1e-30)).max()), e_grad,
                                           c["e_grad"], b_grad, np.abs(c["g64"]).max()))
    assert e_loss <= b_loss and e_grad <= b_grad
    assert np.array_equal(bits(only), loss.view(np.int32))                   # the loss-only call is the same loss
    for b in range(len(c["il"])):
        assert np.all(grad[b, c["il"][b]:] == 0)


def test_infeasible_row(gpu):
    """fewer frames than labels + adjacent repeats: loss +inf, gradient block exactly 0, every other row of the batch bit-identical
    to the same rows computed without it, no NaN anywhere"""
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    c = case("b_boost8")
    z, lab, il, ll = c["z"].copy(), c["lab"].copy(), c["il"].copy(), c["ll"].copy()
    bad = 4
    lab[bad, :10] = lab[bad, 0]                   # 10 equal labels need 19 frames
    ll[bad], il[bad] = 10, 18
    loss, grad = ctc_loss(z, lab, il, ll, return_grad=True)
    keep = [b for b in range(len(il)) if b != bad]
    loss_k, grad_k = ctc_loss(z[keep], lab[keep], il[keep], ll[keep], return_grad=True)
    assert not torch.isnan(loss).any() and not torch.isnan(grad).any()
    assert torch.isinf(loss[bad]) and loss[bad] > 0 and torch.all(grad[bad] == 0)
    assert np.array_equal(bits(loss[keep]), bits(loss_k)) and np.array_equal(bits(grad[keep]), bits(grad_k))
    il2 = il.copy()
    il2[bad] = 19                                 # one frame more and it is feasible
    l2, g2 = ctc_loss(z, lab, il2, ll, return_grad=True)
    one = (z[bad:bad + 1], lab[bad:bad + 1], il2[bad:bad + 1], ll[bad:bad + 1])
    (l64, g64), (l32, g32) = cy.torch_chain(*one), cy.torch_chain(*one, dtype=torch.float32)
    assert torch.isfinite(l2).all() and abs(float(l2[bad]) - l64[0]) <= cy.bound(abs(l32[0] - l64[0]), l64)
    assert np.abs(g2[bad].cpu().numpy() - g64[0]).max() <= cy.bound(np.abs(g32 - g64).max(), g64)
    path, spans, score = ctc_forced_align(z, lab, il, ll)
    assert torch.isinf(score[bad]) and score[bad] < 0 and torch.all(path[bad] == -1) and torch.all(spans[bad] == -1)
    assert not torch.isnan(score).any() and torch.isfinite(score[keep]).all()
    # a label that arrives on the device and is no class at all is answered the same way (the host side cannot see it)
    lab_d = torch.from_numpy(lab).cuda()
    lab_d[3, 0] = z.shape[2] + 5
    l3, g3 = ctc_loss(z, lab_d, torch.from_numpy(il2).cuda(), torch.from_numpy(ll).cuda(), return_grad=True)
    assert torch.isinf(l3[3]) and torch.all(g3[3] == 0) and not torch.isnan(g3).any()
    others = [b for b in range(len(il)) if b != 3]
    assert np.array_equal(bits(l3[others]), bits(l2[others])) and np.array_equal(bits(g3[others]), bits(g2[others]))


@pytest.mark.parametrize("name", ["a_random_scale1", "b_boost12", "d_wide_boost12"])
def test_probabilities_entry(gpu, name):
    """ctc_batch_cost(y_true, softmax(z), input_length [B,1], label_length [B,1]) -> [B,1], the logits entry's loss"""
    from tensorflowasr_amd.models import ctc_batch_cost
    c = case(name)
    p = torch.softmax(torch.from_numpy(c["z"]), -1).numpy()
    got = ctc_batch_cost(c["lab"], p, c["il"][:, None], c["ll"][:, None])
    assert tuple(got.shape) == (len(c["il"]), 1) and got.dtype == torch.float32
    e = float(np.abs(got.cpu().numpy()[:, 0] - c["l64"]).max())
    print("%s: probabilities entry loss max|d| %.3g, bound %.3g" % (name, e, cy.bound(c["e_loss"], c["l64"])))
    assert e <= cy.bound(c["e_loss"], c["l64"])


def test_frames_past_input_length_are_never_read(gpu):
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    c = case("b_boost12")
    z = c["z"].copy()
    loss, grad = ctc_loss(z, c["lab"], c["il"], c["ll"], return_grad=True)
    path, spans, score = ctc_forced_align(z, c["lab"], c["il"], c["ll"])
    rng = np.random.default_rng(0)
    for b, n in enumerate(c["il"]):
        z[b, n:] = rng.uniform(-1e30, 1e30, z[b, n:].shape)
        z[b, n::2] = np.nan
        assert torch.all(grad[b, n:] == 0) and torch.all(path[b, n:] == -1)
    loss2, grad2 = ctc_loss(z, c["lab"], c["il"], c["ll"], return_grad=True)
    path2, spans2, score2 = ctc_forced_align(z, c["lab"], c["il"], c["ll"])
    for a, b in ((loss, loss2), (grad, grad2), (score, score2)):
        assert np.array_equal(bits(a), bits(b))
    assert torch.equal(path, path2) and torch.equal(spans, spans2)


@pytest.mark.parametrize("name", ["a_random_scale4", "c_long_boost10"])
def test_reproducible_and_independent_of_the_batch(gpu, name):
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    c = case(name)
    z, lab, il, ll = c["z"], c["lab"], c["il"], c["ll"]
    B = len(il)
    loss, grad = ctc_loss(z, lab, il, ll, return_grad=True)
    path, spans, score = ctc_forced_align(z, lab, il, ll)
    loss2, grad2 = ctc_loss(z, lab, il, ll, return_grad=True)
    path2, spans2, score2 = ctc_forced_align(z, lab, il, ll)
    assert np.array_equal(bits(loss), bits(loss2)) and np.array_equal(bits(grad), bits(grad2))
    assert torch.equal(path, path2) and torch.equal(spans, spans2) and np.array_equal(bits(score), bits(score2))
    perm = np.roll(np.arange(B), 3)[::-1].copy()                             # another position, other neighbours
    lp, gp = ctc_loss(z[perm], lab[perm], il[perm], ll[perm], return_grad=True)
    pp, sp, cp = ctc_forced_align(z[perm], lab[perm], il[perm], ll[perm])
    assert np.array_equal(bits(lp), bits(loss[perm])) and np.array_equal(bits(gp), bits(grad[perm]))
    assert torch.equal(pp, path[perm]) and torch.equal(sp, spans[perm]) and np.array_equal(bits(cp), bits(score[perm]))
    for b in (0, 1, 2, B - 1):                                                # alone, in its own (smaller) shapes
        n, u = int(il[b]), int(ll[b])
        l1, g1 = ctc_loss(z[b:b + 1, :n], lab[b:b + 1, :u], None, None, return_grad=True)
        p1, s1, c1 = ctc_forced_align(z[b:b + 1, :n], lab[b:b + 1, :u])
        assert np.array_equal(bits(l1), bits(loss[b:b + 1])) and np.array_equal(bits(g1), bits(grad[b:b + 1, :n]))
        assert torch.equal(p1, path[b:b + 1, :n]) and torch.equal(s1, spans[b:b + 1, :u])
        assert np.array_equal(bits(c1), bits(score[b:b + 1]))


def check_alignment(lq64, labels, blank, path, spans, score, what):
    """valid (collapses to the labels, spans are its runs) and optimal to rounding.  score against the float64 sum of log q along
    the path: 16 float32 ulps of the sum, plus 2 ulps of 1 per frame -- a frame's probability p <= 1 is a rounded float32, and its
    logarithm inherits that absolute error"""
    T, U = len(path), len(labels)
    assert cy.collapse(path, blank) == [int(l) for l in labels], what
    runs, prev = [], None
    for t, cls in enumerate(path):
        if cls != blank and cls != prev:
            runs.append([t, t])
        elif cls != blank:
            runs[-1][1] = t
        prev = cls
    assert np.array_equal(np.asarray(spans[:U]).reshape(-1, 2), np.array(runs, np.int64).reshape(-1, 2)), what
    assert np.all(np.asarray(spans[U:]) == -1), what
    flat = np.asarray(spans[:U]).reshape(-1)
    assert np.all(np.diff(flat[1:-1].reshape(-1, 2), axis=1) > 0) if U > 1 else True, what     # end of one < start of the next
    assert np.all(flat[0::2] <= flat[1::2]), what
    along = cy.path_logprob(lq64, path)
    assert abs(score - along) <= 16 * cy.ULP32 * max(abs(along), 1.0) + 2 * cy.ULP32 * T, (what, score, along)
    best64, _ = cy.viterbi(lq64, labels, blank)
    best32, path32 = cy.viterbi(lq64, labels, blank, np.float32)
    d32 = best64 - cy.path_logprob(lq64, path32)
    deficit = best64 - along
    assert deficit >= -1e-9 * max(1.0, abs(best64)), what
    assert deficit <= max(4 * d32, 16 * cy.ULP32 * abs(best64)), (what, deficit, d32)
    return deficit, d32, abs(score - along)


@pytest.mark.parametrize("name", list(cy.CASES))
def test_alignment_is_valid_and_optimal(gpu, name):
    from tensorflowasr_amd.models import ctc_forced_align
    c = case(name)
    V = c["z"].shape[2]
    path, spans, score = ctc_forced_align(c["z"], c["lab"], c["il"], c["ll"])
    assert path.dtype == torch.int32 and spans.dtype == torch.int32 and tuple(spans.shape) == c["lab"].shape + (2,)
    path, spans, score = path.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()
    for b in range(len(c["il"])):
        n, u = int(c["il"][b]), int(c["ll"][b])
        assert np.all(path[b, n:] == -1)
        lq = cy.log_q(c["z"][b, :n]).numpy()
        d, d32, ds = check_alignment(lq, c["lab"][b, :u], V - 1, path[b, :n], spans[b], float(score[b]), "%s row %d" % (name, b))
        print("%s row %d: T %d U %d score %.6g deficit %.3g (float32 Viterbi %.3g) |score - sum along the path| %.3g"
              % (name, b, n, u, score[b], d, d32, ds))
    p2, s2, c2 = ctc_forced_align(torch.softmax(torch.from_numpy(c["z"]), -1).cuda(), c["lab"], c["il"], c["ll"], is_logits=False)
    # the probabilities entry: the same scores up to the roundings of softmax done outside (same budget as above, twice)
    assert np.abs(c2.cpu().numpy() - score).max() <= 2 * (16 * cy.ULP32 * np.abs(score).max() + 2 * cy.ULP32 * c["z"].shape[1])


@pytest.mark.parametrize("i", range(len(cy.TINY)))
def test_brute_force_cases(gpu, i):
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    labels, T = cy.TINY[i]
    z = cy.tiny_logits(i, T)
    lq = cy.log_q(z)[0].numpy()
    nll, best, best_path, unique = cy.brute_force(lq, labels, 3)
    lab = np.array([labels], np.int32).reshape(1, len(labels))
    loss, grad = ctc_loss(z, lab, return_grad=True)
    _, g64 = cy.torch_chain(z, lab, [T], [len(labels)])
    assert abs(float(loss[0]) - nll) <= 1e-5 and np.abs(grad[0].cpu().numpy() - g64[0]).max() <= 1e-5
    path, spans, score = ctc_forced_align(z, lab)
    assert abs(float(score[0]) - best) <= 1e-5
    if unique:
        assert np.array_equal(path[0].cpu().numpy(), best_path)
    # the same utterance padded into wider shapes, another blank: class 1 as the blank of the same distribution
    perm = [0, 3, 2, 1]
    loss_b = ctc_loss(z[..., perm], np.array([[perm[l] for l in labels] + [0, 0]], np.int32), [T], [len(labels)], blank=1)
    assert abs(float(loss_b[0]) - nll) <= 1e-5


def test_long_label_sequences(gpu):
    """256 label positions (several waves per lattice), the built limit, and the 64 / 65 thread boundary"""
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    for U, T in ((256, 600), (63, 150), (64, 150), (511, 1100)):
        z, lab, il, ll = cy.make_case(40 + U, 3, T, 50, U, boost=8.0)
        l64, g64 = cy.torch_chain(z, lab, il, ll)
        l32, g32 = cy.torch_chain(z, lab, il, ll, dtype=torch.float32)
        loss, grad = ctc_loss(z, lab, il, ll, return_grad=True)
        e_l, e_g = np.abs(loss.cpu().numpy() - l64).max(), np.abs(grad.cpu().numpy() - g64).max()
        print("U=%d: loss max|d| %.3g (torch-f32 %.3g), grad max|d| %.3g (torch-f32 %.3g)" % (U, e_l, np.abs(l32 - l64).max(), e_g,
                                                                                             np.abs(g32 - g64).max()))
        assert e_l <= cy.bound(np.abs(l32 - l64).max(), l64) and e_g <= cy.bound(np.abs(g32 - g64).max(), g64)
        path, spans, score = ctc_forced_align(z, lab, il, ll)
        b = 0
        check_alignment(cy.log_q(z[b]).numpy(), lab[b], 49, path[b].cpu().numpy(), spans[b].cpu().numpy(), float(score[b]), "U=%d" % U)
    with pytest.raises(_lib.Mi355AsrError, match="built for up to"):
        ctc_loss(np.zeros((1, 1200, 8), np.float32), np.zeros((1, 512), np.int32))


def _asr(tmp_path):
    from tensorflowasr_amd.asr import ASR
    from tensorflowasr_amd.config import load_yaml
    (tmp_path / "phones.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + ["p%d" % i for i in range(56)]) + "\n")
    (tmp_path / "chars.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4e00 + i) for i in range(96)]) + "\n")
    here = os.path.join(os.path.dirname(GOLDEN), "..", "tensorflowasr_amd", "configs")
    cfg = load_yaml(os.path.join(here, "am_data.yml"))
    cfg.update(load_yaml(os.path.join(here, "conformerS.yml")))
    cfg["model_config"]["num_blocks"] = 2
    cfg["inp_config"]["vocabulary"] = str(tmp_path / "phones.txt")
    cfg["tar_config"]["vocabulary"] = str(tmp_path / "chars.txt")
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    return ASR(cfg, load_checkpoint=False)


def test_asr_align(gpu, tmp_path):
    """ASR.align on the reference recording with a small seeded model: the spans of ctc_forced_align on the utterance's logits,
    times = frames x 0.04 s; the model's own greedy output aligns along the per-frame maxima, so no other labels score higher"""
    from tensorflowasr_amd.models import ctc_forced_align, ctc_greedy_decode
    asr = _asr(tmp_path)
    wav = os.path.join(GOLDEN, "speech_bac.wav")
    data = asr.speech_featurizer.load_wav(wav)
    enc = asr.encoder(np.asarray(data, np.float32).reshape(1, -1, 1), training=False)
    wc = asr.ctc_model.get_weights_dict()
    logits0 = asr.ctc_model(enc, training=False)
    wc["fully_connected/bias"] = (np.asarray(wc["fully_connected/bias"], np.float32)
                                  - logits0.mean(dim=(0, 1)).cpu().numpy()).astype(np.float32)      # a varied arg-max
    asr.ctc_model.load_weights(wc, by_name=False)
    logits, frame_ids = asr.ctc_model(enc, training=False, return_argmax=True)
    V = asr.phone_featurizer.num_classes
    T = logits.shape[1]
    ids, lens = ctc_greedy_decode(frame_ids, None, blank=V - 1)
    n = int(lens[0].item())
    greedy = [int(v) for v in ids[0, :n].cpu().numpy()]
    assert n >= 5
    phones = [asr.phone_featurizer.index_to_token[i] for i in greedy]
    out = asr.align(wav, phones)
    path, spans, score = ctc_forced_align(logits, np.array([greedy], np.int32), blank=V - 1)
    spans = spans[0].cpu().numpy()
    assert [p for p, _, _ in out] == phones and len(out) == n
    for (p, a, b), (f0, f1) in zip(out, spans):
        assert a == f0 * 0.04 and b == (f1 + 1) * 0.04 and 0 <= f0 <= f1 < T
    assert asr.align(data, greedy) == out and asr.last_alignment[0] == float(score[0])
    # greedy labels: the best path is the per-frame arg-max itself
    assert np.array_equal(path[0].cpu().numpy(), frame_ids[0].cpu().numpy())
    lq = cy.log_q(logits[0].cpu().numpy()).numpy()
    assert abs(float(score[0]) - lq.max(-1).sum()) <= 16 * cy.ULP32 * abs(lq.max(-1).sum()) + 1e-4
    for other in (greedy[:-1], greedy[1:], greedy + [greedy[-1] + 1 if greedy[-1] + 2 < V else 4], [g for g in reversed(greedy)]):
        _, _, s = ctc_forced_align(logits, np.array([other], np.int32), blank=V - 1)
        assert float(s[0]) <= float(score[0])
    with pytest.raises(ValueError):
        asr.align(data[:16000], (phones * 10)[:40])                           # 25 frames for 40 labels


def test_am_tester_reports_ctc_loss(gpu, tmp_path):
    """AMTester(with_ctc_loss=True): results()['ctc_loss'] is the mean of ctc_batch_cost over the batch (ctc_runners.py:125-150),
    here against the float64 yardstick on the ORACLE's logits: the loss bound widened by the project's 1e-3 logits contract,
    |d loss| <= 2 T 1e-3 (a logit error e moves log q of a frame by at most 2 e).  Off by default: today's keys."""
    from helpers import co
    from test_host import _eval_fixture
    from tensorflowasr_amd.eval import AMTester, EvalList
    cfg = _eval_fixture(tmp_path, False)
    cfg["model_config"]["num_blocks"] = 2
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    t = AMTester(cfg, load_checkpoint=False, with_ctc_loss=True)
    ds = EvalList(cfg, t.speech_featurizer, t.phone_featurizer, t.text_featurizer, batch_size=3)
    batch = ds.eval_data_generator()
    x, in_len, ph, ph_len, txt = batch
    mc = dict(co.CONFORMER_S, num_blocks=2, translator_num_blocks=2, translator_kernel_size=32, translator_fc_factor=0.5)
    we, wc = t.encoder.get_weights_dict(), t.ctc_model.get_weights_dict()
    for k in ("mel_layer/real_kernels", "mel_layer/imag_kernels"):
        we[k] = we[k].reshape(1024, 513)
    enc = co.conformer_encoder(x[..., 0].astype(np.float64), we, mc)
    logits = co.ctc_decoder(enc, wc, mc)
    T = logits.shape[1]
    l64, _ = cy.torch_chain(logits, ph, np.minimum(in_len, T), ph_len, want_grad=False)
    l32, _ = cy.torch_chain(logits, ph, np.minimum(in_len, T), ph_len, dtype=torch.float32, want_grad=False)
    t.set_datasets([batch])
    t.set_all_steps(1)
    r = t.run()
    tol = cy.bound(np.abs(l32 - l64).max(), l64) + 2 * T * 1e-3
    print("AMTester ctc_loss %.6f, float64 on the oracle logits %.6f, tolerance %.3g" % (r["ctc_loss"], l64.mean(), tol))
    assert np.isfinite(l64).all() and abs(r["ctc_loss"] - l64.mean()) <= tol
    assert set(r) == {"phone_ser", "phone_cer", "txt_ser", "txt_cer", "phone_s_i_d", "trans_s_i_d", "steps", "ctc_loss"}
    t0 = AMTester(cfg, load_checkpoint=False)
    t0.set_datasets([batch])
    t0.set_all_steps(1)
    r0 = t0.run()
    assert set(r0) == {"phone_ser", "phone_cer", "txt_ser", "txt_cer", "phone_s_i_d", "trans_s_i_d", "steps"}
    assert all(r0[k] == r[k] for k in r0)
