"""The ragged recursive filters on the MI355X (mi355asr_sos_ragged, iir.SOSFilter) against long-double evaluations of
scipy.signal.sosfiltfilt and sosfilt (iir_ref.py): per sample |y - y_ld| <= 2^-24 |y_ld| + 8 D, D = SciPy's own distance from the
long-double result over the row (at least 2^-50 max |x|).  Rows of 22, 23, 64, C - 43, C - 42, C - 41, 2 C - 42, 3 C + 5 and 6000
samples in one batch (C = SOSFilter.CHUNK: the extended rows end at C - 1, C, C + 1 and 2 C), band-stops at the starts 0.01, 0.2,
0.35, 0.69 and 0.699 per row and one shared by all, one and eight sections; NaN past every length; zeros past every length; what
is refused; every row equal to its solo call, to a second run and to itself at another batch position bit for bit; int16; a
stream fed in packets.

Measured on the MI355X: the worst (|y - y_ld| - 2^-24 |y_ld|) / D is 0 in every test of this file -- the final rounding to float32
covers the float64 error at every sample, and the float32 output of the per-row batch is the rounded long-double value at all
6 970 samples.  The final states of sosfilt are float64 and show the recursion's own error: |zf - zf_ld| / max(D, SciPy's
|zf - zf_ld|) is 4.7 at worst (the row of C - 43 samples at start 0.69: 4.3e-14 against SciPy's 7.2e-15), between 0.03 and 0.7 for
the other eight rows; they are held to the same factor 8, for the same reason: two float64 evaluations of the same sections in a
different order."""
import ctypes

import numpy as np
import pytest
from scipy import signal

import iir_ref as ir
from iir_cases import PADLEN, batch, bits, check_bound, chunk, device, filtfilt_refs, poisoned, sections

pytestmark = pytest.mark.gpu


def flt():
    device()
    from tensorflowasr_amd.iir import SOSFilter
    return SOSFilter()


def test_sosfiltfilt_with_a_filter_per_row():
    c = batch()
    y = flt().sosfiltfilt(c["x"], c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    assert y.dtype == np.float32 and y.shape == c["x"].shape and np.isfinite(y).all()
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        y_ld, D = filtfilt_refs()[b]
        worst = max(worst, check_bound(y[b, :n], y_ld, D))
        assert not y[b, n:].any(), (b, n)
    from iir_cases import FLIPS
    print("sosfiltfilt, a filter per row: worst (|y - y_ld| - 2^-24 |y_ld|) / D = %.3f; float32 not the rounded long double: %d of %d"
          % (worst, FLIPS[1], FLIPS[0]))


def test_sosfiltfilt_with_a_shared_filter_and_the_default_padlen():
    c = batch()
    f = flt()
    y = f.sosfiltfilt(c["x"], c["lens"], sections(0.699)).cpu().numpy()          # the default edge of three sections is 21
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        y_ld, D = filtfilt_refs(0.699)[b]
        worst = max(worst, check_bound(y[b, :n], y_ld, D))
        assert not y[b, n:].any(), (b, n)
    print("sosfiltfilt, shared filter at 0.699: worst ratio = %.3f" % worst)
    # [1, S, 6] is the shared filter too, and [B, S, 6] of equal filters gives the same bits
    y1 = f.sosfiltfilt(c["x"], c["lens"], sections(0.699)[None], padlen=PADLEN).cpu().numpy()
    y2 = f.sosfiltfilt(c["x"], c["lens"], np.tile(sections(0.699), (len(c["lens"]), 1, 1)), padlen=PADLEN).cpu().numpy()
    assert np.array_equal(bits(y1), bits(y)) and np.array_equal(bits(y2), bits(y))


@pytest.mark.parametrize("S", [1, 8])
def test_one_and_eight_sections(S):
    C = chunk()
    sos = signal.butter(2, 0.3, output="sos") if S == 1 else signal.butter(8, [0.15, 0.6], "bandpass", output="sos")
    assert sos.shape == (S, 6)
    rng = np.random.default_rng(S)
    lens = [2 * C + 17, 700]
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    x = poisoned(rows, 705, np.float32)
    f = flt()
    from tensorflowasr_amd.iir import default_padlen
    pad = default_padlen(sos)
    y = f.sosfiltfilt(x, lens, sos).cpu().numpy()
    zi = rng.standard_normal((2, S, 2))
    g, zf = f.sosfilt(x, lens, sos, zi=zi)
    g, zf = g.cpu().numpy(), zf.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        r = rows[b].astype(np.float64)
        y_ld = ir.sosfiltfilt_ld(sos, r, pad)
        worst = max(worst, check_bound(y[b, :n], y_ld, ir.distance(signal.sosfiltfilt(sos, r), y_ld, r)))
        g_ld, zf_ld = ir.sosfilt_ld(sos, r, zi[b])
        gs, zs = signal.sosfilt(sos, r, zi=zi[b])
        D = ir.distance(gs, g_ld, r)
        worst = max(worst, check_bound(g[b, :n], g_ld, D))
        Dz = max(D, float(np.abs(zs - zf_ld).max()))
        assert np.abs(zf[b] - zf_ld).max() <= 8 * Dz, (b, float(np.abs(zf[b] - zf_ld).max()), Dz)
        assert not y[b, n:].any() and not g[b, n:].any()
    print("S = %d: worst ratio = %.3f" % (S, worst))


def test_sosfilt_with_states_and_in_packets():
    c = batch()
    C = chunk()
    f = flt()
    B = len(c["lens"])
    rng = np.random.default_rng(3)
    zi = rng.standard_normal((B, 3, 2)) * 0.1
    y, zf = f.sosfilt(c["x"], c["lens"], c["sos"], zi=zi)
    y, zf = y.cpu().numpy(), zf.cpu().numpy()
    y0, zf0 = f.sosfilt(c["x"], c["lens"], c["sos"])
    assert np.isfinite(y).all() and np.isfinite(zf).all()
    worst, refs, zf_lds = 0.0, [], []
    for b, n in enumerate(c["lens"]):
        x = c["rows"][b]
        y_ld, zf_ld = ir.sosfilt_ld(c["sos"][b], x, zi[b])
        ys, zs = signal.sosfilt(c["sos"][b], x, zi=zi[b])
        D = ir.distance(ys, y_ld, x)
        refs.append((y_ld, D))
        worst = max(worst, check_bound(y[b, :n], y_ld, D))
        zf_lds.append((zf_ld, max(D, float(np.abs(zs - zf_ld).max()))))
        print("row %d: |zf - zf_ld| = %.3g, SciPy's %.3g, D = %.3g" % (b, float(np.abs(zf[b] - zf_ld).max()), float(np.abs(zs - zf_ld).max()), D))
        assert np.abs(zf[b] - zf_ld).max() <= 8 * zf_lds[b][1], b
        assert not y[b, n:].any(), (b, n)
        z_ld = ir.sosfilt_ld(c["sos"][b], x)[0]                   # zi = None is the zero state
        check_bound(y0.cpu().numpy()[b, :n], z_ld, ir.distance(signal.sosfilt(c["sos"][b], x), z_ld, x))
    print("sosfilt with zi: worst ratio = %.3f" % worst)
    # the same rows as a stream: packets of 1, 63, C, C + 1 samples and the rest, the state carried from call to call
    cuts = np.cumsum([0, 1, 63, C, C + 1])
    W = c["x"].shape[1]
    state, pieces = zi, []
    for lo, hi in zip(cuts, list(cuts[1:]) + [W]):
        lens = np.clip(np.array(c["lens"]) - lo, 0, hi - lo)
        part, state = f.sosfilt(c["x"][:, lo:hi], lens, c["sos"], zi=state)
        pieces.append(part.cpu().numpy())
    got = np.concatenate(pieces, axis=1)
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        worst = max(worst, check_bound(got[b, :n], *refs[b]))
    # a row that has ended keeps its state through the later packets: the last state is held to the one-shot call's bound
    state = state.cpu().numpy()
    for b in range(B):
        assert np.abs(state[b] - zf_lds[b][0]).max() <= 8 * zf_lds[b][1], b
    print("sosfilt in packets: worst ratio = %.3f" % worst)


def test_noise_is_added_in_float64_and_never_read_past_the_row():
    c = batch()
    y = flt().sosfiltfilt(c["x"], c["lens"], c["sos"], padlen=PADLEN, noise=c["u"], noise_scale=0.001).cpu().numpy()
    assert np.isfinite(y).all()
    for b, n in enumerate(c["lens"]):
        y_ld, D = filtfilt_refs()[b]
        check_bound(y[b, :n], y_ld + ir.LD(0.001) * c["us"][b], D + 2.0 ** -52)   # the product and the sum round once each: two roundings below |y| < 2
        assert not y[b, n:].any()


def test_rows_do_not_depend_on_the_batch_on_the_run_or_on_their_position():
    c = batch()
    f = flt()
    B = len(c["lens"])
    kw = dict(padlen=PADLEN, noise=c["u"], noise_scale=0.001, quantise=True)
    y = f.sosfiltfilt(c["x"], c["lens"], c["sos"], **kw).cpu().numpy()
    assert np.array_equal(bits(f.sosfiltfilt(c["x"], c["lens"], c["sos"], **kw).cpu().numpy()), bits(y))
    order = list(range(B))[::-1]
    yr = f.sosfiltfilt(c["x"][order], [c["lens"][b] for b in order], c["sos"][order], padlen=PADLEN, noise=c["u"][order], noise_scale=0.001,
                       quantise=True).cpu().numpy()
    assert np.array_equal(bits(yr), bits(y[order]))
    g, zf = f.sosfilt(c["x"], c["lens"], c["sos"])
    g, zf = g.cpu().numpy(), zf.cpu().numpy()
    for b, n in enumerate(c["lens"]):
        y1 = f.sosfiltfilt(c["x"][b, :n], None, c["sos"][b], padlen=PADLEN, noise=c["u"][b:b + 1, :n], noise_scale=0.001, quantise=True)
        assert np.array_equal(bits(y1.cpu().numpy()[0]), bits(y[b, :n])), (b, n)
        g1, z1 = f.sosfilt(c["x"][b, :n], None, c["sos"][b])
        assert np.array_equal(bits(g1.cpu().numpy()[0]), bits(g[b, :n])) and np.array_equal(bits(z1.cpu().numpy()[0]), bits(zf[b])), (b, n)


def test_int16_input_is_the_float32_call_on_x_over_32768():
    c = batch()
    f = flt()
    pcm = np.random.default_rng(5).integers(-32768, 32768, c["x"].shape).astype(np.int16)
    a = f.sosfiltfilt(pcm, c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    b = f.sosfiltfilt(pcm.astype(np.float32) / 32768, c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    assert np.array_equal(bits(a), bits(b)) and float(np.abs(a).max()) > 0.5
    a, za = f.sosfilt(pcm, c["lens"], c["sos"])
    b, zb = f.sosfilt(pcm.astype(np.float32) / 32768, c["lens"], c["sos"])
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) and np.array_equal(bits(za.cpu().numpy()), bits(zb.cpu().numpy()))


def test_short_rows_raise_in_python_and_are_copied_by_the_library():
    c = batch()
    f = flt()
    with pytest.raises(ValueError, match="row 2.*greater than padlen, which is 21"):
        f.sosfiltfilt(c["x"][:4], [22, 6000, 21, 23], c["sos"][:4], padlen=PADLEN)
    # the library itself copies such a row through, the finish applied; an empty row gives zeros
    lens = [21, 1, 0, 22]
    y, _ = f._run(c["x"][:4], lens, c["sos"][:4], 1, PADLEN, None, False, None, 1.0, False, short_rows="copy")
    y = y.cpu().numpy()
    for b, n in enumerate(lens[:3]):
        assert np.array_equal(bits(y[b, :n]), bits(c["x"][b, :n])) and not y[b, n:].any(), b
    y_ld = ir.sosfiltfilt_ld(c["sos"][3], c["rows"][3][:22], PADLEN)
    check_bound(y[3, :22], y_ld, ir.distance(signal.sosfiltfilt(c["sos"][3], c["rows"][3][:22], padlen=PADLEN), y_ld, c["rows"][3][:22]))
    yq, _ = f._run(c["x"][:4], lens, c["sos"][:4], 1, PADLEN, None, False, c["u"][:4], 0.001, True, short_rows="copy")
    want = ir.quantise(c["rows"][0][:21] + 0.001 * c["us"][0][:21]).astype(np.float32)
    assert np.array_equal(bits(yq.cpu().numpy()[0, :21]), bits(want))


def test_refusals_leave_the_output_untouched():
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.zeros((2, 4000), dtype=torch.float32, device="cuda:0")
    ln = torch.tensor([4000, 3000], dtype=torch.int32, device="cuda:0")
    y = torch.full((2, 4000), 7.0, dtype=torch.float32, device="cuda:0")
    wb = ctypes.c_size_t()
    assert lib.mi355asr_sos_workspace_bytes(2, 4000, 8, 1, ctypes.byref(wb)) == 0
    ws = torch.empty(wb.value // 8 + 1, dtype=torch.float64, device="cuda:0")
    good = np.tile(sections(0.2), (2, 1, 1))
    bad = good.copy()
    bad[1, 2, 3] = 2.0                         # a0 of the last section of the second filter
    nine = np.tile(sections(0.2), (1, 3, 1))

    def call(sos, S, shared, mode=1, nbytes=wb.value):
        s = torch.from_numpy(np.ascontiguousarray(sos)).to("cuda:0")
        return lib.mi355asr_sos_ragged(p(x), 0, p(ln), 2, 4000, p(s), S, shared, mode, 21, None, None, None, 0, 1.0, 0, p(y), 4000, p(ws),
                                       nbytes, None)
    assert call(bad, 3, 0) == -1 and b"a0 = 2" in lib.mi355asr_last_error()
    assert call(bad[1], 3, 1, mode=0) == -1
    assert call(nine, 9, 1) == -1 and b"9 sections" in lib.mi355asr_last_error()
    assert call(good, 3, 0, nbytes=1024) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call(bad, 3, 1) == 0                # shared: only the first filter is read
    assert call(good, 3, 0) == 0
    torch.cuda.synchronize()
    assert not bool(y.any())                   # the filtered zeros
