"""The multi-resolution STFT loss, its gradient, the VAD mask statistics and VADTester on the MI355X (csrc/stft_loss.hip,
tensorflowasr_amd/losses.py, eval.py) against the float64 restatement tests/stft_loss_ref.py.

Accuracy line: for each of sc, mag, the scalar and the gradient, the largest error over the case set is at most 4 x the largest
error of the same arithmetic in torch float32 on the CPU (unfold x window, torch.fft.rfft, autograd) over the same set; loss errors
relative to |value64|, gradient errors relative to the row's largest |grad64|; torch's error is asserted non-zero.
Case set: single rows of LENGTHS samples (no frame, one frame at one resolution, one at both, the second-frame crossovers, samples
covered by 1 to 5 frames, 48 000, and OLA_TILE - 1, OLA_TILE, OLA_TILE + 1 samples; a workgroup takes one frame, so there is no frame
tile) at the reference's pair of resolutions, at (2048, 2048, 512) alone and at (512, 7, 3) alone.
Measured on one MI355X, largest error over the set, kernel / torch float32 / ratio (test_accuracy_line prints them): sc 3.76e-07 /
2.89e-07 / 1.30, mag 2.33e-06 / 1.07e-06 / 2.19, scalar 9.30e-07 / 4.42e-07 / 2.11, gradient 1.98e-04 / 3.07e-04 / 0.64; the
fixture's two inputs against the reference's float32 run 9.7e-08 and 1.9e-07 (line 1.8e-06); the mask losses 7.9e-08 and 2.3e-08
against the line 8 * 2^-24 * (1 + |value|) = 1.8e-06 and 9.4e-07."""
import ctypes

import numpy as np
import pytest
import torch

import stft_loss_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LENGTHS = [249, 250, 255, 256, 257, 599, 600, 601, 719, 720, 1199, 1200, 2400, 48000]
RES_SETS = {"pair": R.RESOLUTIONS, "2048": ((2048, 2048, 512),), "odd": ((512, 7, 3),)}
EXTRA = {"2048": [2047, 2048, 2559, 2560, 4100], "odd": [6, 7, 9, 10, 40]}
RAGGED = [2400, 600, 250, 0, 1337]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    from tensorflowasr_amd import losses
    assert losses.OLA_TILE == 256 and losses.FRAMES_PER_WORKGROUP == 1
    assert all(n in LENGTHS for n in (losses.OLA_TILE - 1, losses.OLA_TILE, losses.OLA_TILE + 1))
    return torch.device("cuda:0")


def make(name):
    from tensorflowasr_amd import losses
    fft, fl, st = zip(*RES_SETS[name])
    return losses.MultiResolutionSTFTLoss(fft, fl, st)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


@pytest.fixture(scope="module")
def accuracy(gpu):
    """every case once: the kernel's and torch float32's errors against the float64 restatement -> {quantity: [kernel, torch]}"""
    worst = {k: [0.0, 0.0] for k in ("sc", "mag", "scalar", "grad")}
    for name, res in RES_SETS.items():
        fn = make(name)
        for i, L in enumerate(LENGTHS + EXTRA.get(name, [])):
            y, x = R.seeded_pair((1, L), seed=100 + i)
            sc64, mag64, fr64 = R.loss_rows(y, x, None, res)
            v64, g64 = R.loss_and_grad(y, x, None, res)
            value, grad = fn(torch.from_numpy(y).to(gpu), torch.from_numpy(x).to(gpu), return_grad=True)
            sc, mag, frames = fn.rows(y, x)
            sc, mag, value, grad = sc.cpu().numpy(), mag.cpu().numpy(), float(value.cpu()), grad.cpu().numpy()
            assert frames.cpu().numpy().tolist() == fr64.tolist()
            ty, tx = torch.from_numpy(y), torch.from_numpy(x).requires_grad_(True)
            tv, tsc, tmag = R.torch_loss(ty, tx, [L], res)
            if torch.is_tensor(tv):
                tv.backward()
            tg = tx.grad.numpy() if tx.grad is not None else np.zeros_like(x)
            assert np.isfinite(grad).all() and grad.shape == (1, L)
            for r in range(len(res)):
                if fr64[0, r] == 0:
                    assert sc[0, r] == 0.0 and np.isnan(mag[0, r])
                    continue
                for key, got, want, tgot in (("sc", sc, sc64, tsc), ("mag", mag, mag64, tmag)):
                    worst[key][0] = max(worst[key][0], rel(got[0, r], want[0, r]))
                    worst[key][1] = max(worst[key][1], rel(tgot[0][r].detach(), want[0, r]))
            if np.isnan(v64):
                assert np.isnan(value)
            else:
                worst["scalar"][0] = max(worst["scalar"][0], rel(value, v64))
                worst["scalar"][1] = max(worst["scalar"][1], rel(tv.detach(), v64))
            scale = np.abs(g64).max()
            if scale == 0:
                assert not grad.any()
            else:
                worst["grad"][0] = max(worst["grad"][0], np.abs(grad - g64).max() / scale)
                worst["grad"][1] = max(worst["grad"][1], np.abs(tg - g64).max() / scale)
    return worst


def test_accuracy_line(accuracy):
    for key, (mine, yard) in accuracy.items():
        print("stft_loss accuracy %-6s kernel %.3e torch-float32 %.3e ratio %.3f" % (key, mine, yard, mine / yard if yard else float("inf")))
    for key, (mine, yard) in accuracy.items():
        assert yard > 0.0, key
        assert mine <= 4.0 * yard, (key, mine, yard)


@pytest.mark.parametrize("geo,L,res,seed", [((1024, 800, 160), 2400, (1024, 600, 120), 7), ((2048, 2048, 512), 4100, (2048, 2048, 512), 8)])
def test_the_stft_pair_and_the_loss_keep_their_own_tables(gpu, geo, L, res, seed):
    """csrc/stft.hip and csrc/stft_loss.hip build their tables with one builder and upload them through one cache, each under its
    own keys: at the same N the last stage differs by the factor N (the inverse against the transpose) and at 1024 the window
    too (800 centred against 600 at the start).  Both run once before either is checked, so a table served to the wrong user shows
    whichever of the two filled its cache first."""
    import stft_ref as sr
    from stft_cases import U24, signal, worst_ratio
    from test_gpu_stft_pair import C_Y
    from tensorflowasr_amd import losses
    from tensorflowasr_amd.stft import STFT
    n_fft, win, hop = geo
    row = signal(np.random.default_rng(n_fft), (1, L))
    y, x = R.seeded_pair((1, L), seed=seed)
    st = STFT(*geo)
    S, frames = st.forward(row, [L])
    back, out_len = st.inverse(S, frames)
    fn = losses.MultiResolutionSTFTLoss((res[0],), (res[1],), (res[2],))
    _, grad = fn(torch.from_numpy(y).to(gpu), torch.from_numpy(x).to(gpu), return_grad=True)
    # the round trip, as test_gpu_stft_pair.test_round_trip_parity_lengths_and_zeros forms it
    F = sr.n_frames(L, n_fft, hop)
    want_len = hop * (F - 1)
    assert F > 1 and int(frames.cpu()[0]) == F and int(out_len.cpu()[0]) == want_len
    want = sr.istft(sr.stft(row[0], *geo), *geo)
    scale = U24 * sr.ola_scale(sr.frame_l1(row[0], *geo), *geo)
    trip = worst_ratio(np.abs(back.cpu().numpy()[0, :want_len] - want), scale)
    # the gradient, as test_accuracy_line forms it
    g64 = R.loss_and_grad(y, x, None, (res,))[1]
    ty, tx = torch.from_numpy(y), torch.from_numpy(x).requires_grad_(True)
    R.torch_loss(ty, tx, [L], (res,))[0].backward()
    mine = np.abs(grad.cpu().numpy() - g64).max() / np.abs(g64).max()
    yard = np.abs(tx.grad.numpy() - g64).max() / np.abs(g64).max()
    print("tables %d: round trip ratio %.4f (line %.2f), gradient kernel %.3e torch-float32 %.3e" % (n_fft, trip, C_Y, mine, yard))
    assert trip <= C_Y
    assert yard > 0.0 and mine <= 4.0 * yard, (mine, yard)


def test_fixture_inputs_give_the_reference_float32_scalar(gpu, accuracy):
    golden = np.load(R.__file__.replace("stft_loss_ref.py", "golden/stft_loss_ref.npz"))
    fn = make("pair")
    line = 4.0 * accuracy["scalar"][1]
    for k in range(2):
        shape = tuple(int(v) for v in golden["shapes"][k])
        y, x = R.seeded_pair(shape, seed=k)
        got = float(fn(y, x).cpu())                                  # the trainer's [B, T, frame] shape
        want = float(golden["loss32_%d" % k])
        print("fixture %d: kernel %.9g reference float32 run %.9g rel %.3e line %.3e" % (k, got, want, rel(got, want), line))
        assert rel(got, want) <= line


def ragged_buffers(lengths, gpu, seed):
    B, W = len(lengths), max(lengths) + 3
    y, x = R.seeded_pair((B, W), seed=seed)
    for b, n in enumerate(lengths):
        y[b, n:] = np.nan
        x[b, n:] = np.nan
    return y, x


@pytest.mark.parametrize("name", ["pair", "odd"])
def test_ragged_rows_are_bit_identical_and_nothing_past_a_length_is_read(gpu, name):
    fn, res = make(name), RES_SETS[name]
    Rn = len(res)
    y, x = ragged_buffers(RAGGED, gpu, seed=40)
    B, W = y.shape
    rng = np.random.default_rng(5)
    w_sc = (0.1 + rng.random((B, Rn))).astype(np.float32)
    w_mag = (0.1 + rng.random((B, Rn))).astype(np.float32)

    def run(yb, xb, lens, ws, wm):
        out = torch.full((len(lens), xb.shape[1]), float("nan"), dtype=torch.float32, device=gpu)
        sc, mag, frames, grad = fn.grad_rows(yb, xb, ws, wm, lens, out=out)
        return bits(sc), bits(mag), frames.cpu().numpy(), bits(grad), grad.cpu().numpy()
    ty, tx = torch.from_numpy(y).to(gpu), torch.from_numpy(x).to(gpu)
    base = run(ty, tx, RAGGED, w_sc, w_mag)
    sc64, mag64, fr64 = R.loss_rows(np.nan_to_num(y), np.nan_to_num(x), RAGGED, res)
    assert base[2].tolist() == fr64.tolist()
    g = base[4]
    assert np.isfinite(g).all(), "an element of grad was not written, or a sample past a length was read"
    sc, mag = base[0].view(np.float32), base[1].view(np.float32)
    assert np.isfinite(sc).all() and (np.isfinite(mag) == (fr64 > 0)).all()
    for b, n in enumerate(RAGGED):
        reach = max([(F - 1) * st + fl for (_, fl, st), F in zip(res, fr64[b]) if F > 0], default=0)
        assert reach <= n and not g[b, reach:].any() and (bits(torch.from_numpy(g[b, reach:])) == 0).all()
    # a second run, the reversed batch, strided views at an odd offset, and every row alone
    again = run(ty, tx, RAGGED, w_sc, w_mag)
    rev = run(ty.flip(0).contiguous(), tx.flip(0).contiguous(), RAGGED[::-1], w_sc[::-1].copy(), w_mag[::-1].copy())
    wide_y = torch.full((B, W + 6), float("nan"), dtype=torch.float32, device=gpu)
    wide_x = torch.full((B, W + 6), float("nan"), dtype=torch.float32, device=gpu)
    wide_y[:, 1:1 + W], wide_x[:, 3:3 + W] = ty, tx
    view = run(wide_y[:, 1:1 + W], wide_x[:, 3:3 + W], RAGGED, w_sc, w_mag)
    assert wide_y[:, 1:1 + W].data_ptr() % 8 == 4 and wide_x[:, 3:3 + W].data_ptr() % 8 == 4
    for k in range(4):
        assert (again[k] == base[k]).all() and (view[k] == base[k]).all() and (rev[k][::-1] == base[k]).all(), k
    for b, n in enumerate(RAGGED):
        m = max(n, 1)
        alone = run(ty[b:b + 1, :m].contiguous(), tx[b:b + 1, :m].contiguous(), [n], w_sc[b:b + 1], w_mag[b:b + 1])
        for k in range(3):
            assert (alone[k][0] == base[k][b]).all(), (b, k)
        assert (alone[3][0, :n] == base[3][b, :n]).all(), b


def test_equal_and_zero_predictions(gpu):
    fn = make("pair")
    y, _ = R.seeded_pair((2, 2400), seed=9)
    value, grad = fn(y, y.copy(), return_grad=True)
    sc, mag, _ = fn.rows(y, y.copy())
    assert float(value.cpu()) == 0.0 and not sc.cpu().numpy().any() and not mag.cpu().numpy().any()
    g = grad.cpu().numpy()
    assert np.isfinite(g).all() and not g.any()
    value, grad = fn(y, np.zeros_like(y), return_grad=True)
    v64, g64 = R.loss_and_grad(y, np.zeros_like(y))
    assert np.isfinite(float(value.cpu())) and np.isfinite(grad.cpu().numpy()).all()
    assert rel(value.cpu(), v64) <= 1e-5


def test_upstream_scales_the_gradient(gpu):
    fn = make("pair")
    y, x = R.seeded_pair((2, 1337), seed=12)
    v1, g1 = fn(y, x, return_grad=True)
    v2, g2 = fn(y, x, return_grad=True, upstream=2.0)
    v3, g3 = fn(y, x, return_grad=True, upstream=0.3)
    assert float(v1.cpu()) == float(v2.cpu()) == float(v3.cpu())
    g1, g2, g3 = g1.cpu().numpy(), g2.cpu().numpy(), g3.cpu().numpy()
    assert (g2 == 2.0 * g1).all()                                    # a power of two scales every product exactly
    assert np.abs(g3 - 0.3 * g1.astype(np.float64)).max() <= 1e-5 * np.abs(g1).max()
    g64 = R.loss_and_grad(y, x, upstream=0.3)[1]
    assert np.abs(g3 - g64).max() <= 1e-3 * np.abs(g64).max()


def test_unsupported_sizes_raise(gpu):
    from tensorflowasr_amd import _lib, losses
    for args in (((256,), (200,), (50,)), ((1024,), (1025,), (120,)), ((1024,), (600,), (601,)), ((1024,), (0,), (1,)),
                 ((1024,), (600,), (0,)), ((512,) * 5, (250,) * 5, (50,) * 5), ((1024, 512), (600,), (120, 50)), ((), (), ())):
        with pytest.raises(ValueError):
            losses.MultiResolutionSTFTLoss(*args)
    with pytest.raises(ValueError):
        make("pair")(np.zeros((2, 800), np.float32), np.zeros((2, 801), np.float32))
    lib = _lib.lib()
    n = ctypes.c_size_t()
    arr = ctypes.c_int32 * 1
    assert lib.mi355asr_stft_loss_workspace_bytes(1, 800, 1, arr(256), arr(200), arr(50), 0, ctypes.byref(n)) == -1
    assert lib.mi355asr_stft_loss_workspace_bytes(1, 800, 1, arr(512), arr(513), arr(50), 0, ctypes.byref(n)) == -1
    assert lib.mi355asr_stft_loss_workspace_bytes(1, 800, 5, arr(512), arr(250), arr(50), 0, ctypes.byref(n)) == -1
    assert lib.mi355asr_stft_loss_workspace_bytes(1, 800, 1, arr(512), arr(250), arr(50), 0, ctypes.byref(n)) == 0 and n.value > 0


def test_mask_stats(gpu):
    from tensorflowasr_amd import losses
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((3, 50)) * 3).astype(np.float32)
    z = np.zeros((3, 50), np.float32)
    z[0] = 1.0                                                       # all speech; row 1 all silence
    x[0, :6] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), 80.0, -80.0, 0.0, -0.5]
    x[1, 0] = 0.5
    lengths = [50, 1, 0]
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan
        z[b, n:] = np.nan
    sums64, counts64 = R.mask_stats(z, x, lengths)
    tz, tx = torch.from_numpy(z).to(gpu), torch.from_numpy(x).to(gpu)
    sums, counts, grad = losses.vad_mask_stats(tz, tx, lengths, return_grad=True)
    assert counts.cpu().numpy().tolist() == counts64.tolist() and counts64[1] == 0 and counts64[0] + counts64[2] == 50
    assert 0 < counts64[2] < 50                                      # 0.5 itself, -80, 0 and -0.5 are negatives; 80 is not
    assert sums.cpu().numpy()[[1, 3]].tolist() == [50.0, 1.0]
    one, zero, grad2 = losses.vad_mask_loss(tz[:, :, None], tx[:, :, None], lengths, return_grad=True)
    one64, zero64 = R.mask_loss(z, x, lengths)
    for got, want in ((float(one.cpu()), one64), (float(zero.cpu()), zero64)):
        print("mask loss %.9g float64 %.17g err %.3e line %.3e" % (got, want, abs(got - want), 8 * U * (1 + abs(want))))
        assert abs(got - want) <= 8 * U * (1 + abs(want))
    g, g64 = grad.cpu().numpy(), R.mask_grad(z, x, lengths)
    assert np.isfinite(g).all() and not g[1, 1:].any() and not g[2].any()
    assert (np.abs(g - g64) <= 2 * U * np.abs(g64) + 1e-44).all()
    assert (bits(grad2) == bits(grad)).all()
    sums_b, counts_b, grad_b = losses.vad_mask_stats(tz, tx, lengths, return_grad=True)
    assert (sums_b.cpu().numpy().view(np.int64) == sums.cpu().numpy().view(np.int64)).all()
    assert (counts_b == counts).all() and (bits(grad_b) == bits(grad)).all()
    m = losses.vad_metrics(tz, tx, lengths=lengths)
    m64 = R.metrics(z, x, lengths=lengths)
    assert [int(m[k].cpu()) for k in ("tp", "fp", "fn", "tn")] == [m64[k] for k in ("tp", "fp", "fn", "tn")]
    assert float(m["acc"].cpu()) == np.float32(m64["acc"]) and float(m["f1"].cpu()) == np.float32(m64["f1"])
    assert float(losses.vad_metrics(np.zeros((1, 4), np.float32), -np.ones((1, 4), np.float32))["f1"].cpu()) == 0.0


def test_vad_tester(gpu, accuracy):
    import os
    from tensorflowasr_amd.eval import VADTester
    from tensorflowasr_amd.vad import VAD
    vad = VAD().load_saved_model(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "online_vad_model"))
    wav_label, x = R.seeded_pair((2, 40, 80), seed=21)
    vad_label, _ = R.seeded_mask((2, 40, 1), seed=21)
    flat = x.reshape(2, -1)
    before = [bits(t) for t in vad.enhance(flat, sample_rate=8000)]
    tester = VADTester(vad)
    want = {k: [] for k in ("vad_loss", "wav_loss", "vad_acc", "f1")}
    for xb, vb, wb in ((x, vad_label, wav_label), (x[:, ::-1].copy(), vad_label[:, ::-1].copy(), wav_label[:, ::-1].copy())):
        tester.update(xb, vb, wb)
        enhanced, logits = (t.cpu().numpy() for t in vad.enhance(xb.reshape(2, -1), sample_rate=8000))
        one, zero = R.mask_loss(vb[..., 0], logits)
        m = R.metrics(vb[..., 0], logits)
        want["vad_loss"].append(one + zero)
        want["wav_loss"].append(R.loss(wb.reshape(2, -1), enhanced))
        want["vad_acc"].append(m["acc"])
        want["f1"].append(m["f1"])
    got = tester.results()
    want = {k: float(np.mean(v)) for k, v in want.items()}
    print("VADTester", got, want)
    assert rel(got["wav_loss"], want["wav_loss"]) <= 4.0 * accuracy["scalar"][1]
    assert abs(got["vad_loss"] - want["vad_loss"]) <= 2 * 8 * U * (1 + abs(want["vad_loss"])) + U * abs(want["vad_loss"])
    assert abs(got["vad_acc"] - want["vad_acc"]) <= U and abs(got["f1"] - want["f1"]) <= U
    after = [bits(t) for t in vad.enhance(flat, sample_rate=8000)]
    assert all((a == b).all() for a, b in zip(before, after))
