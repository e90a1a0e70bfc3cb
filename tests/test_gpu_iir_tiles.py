"""The ragged recursive filters on the MI355X past their first tile: test_gpu_iir.py's checks and bounds, unchanged, on rows that
leave the first workgroup of sos_pass_kernel (W = 64 C = 8 192 positions) and the first stage of sos_scan_kernel (SC = 1 024 C =
131 072 positions), against the same long-double evaluations (iir_ref.py).  iir_cases.long_batch("tiles"): extended rows of W - 1,
W, W + 1, 2 W and 2 W + 1 positions (blockIdx.x = 1 and 2, forward and reverse, the short last chunk in tile 1 and in tile 2) with
rows of 22 and 3 C + 5 samples between them (the fill branch in tiles 1 and 2); long_batch("scan"): SC, SC + 1 and 2 SC + 5
positions (1 024, 1 025 and 2 049 chunks: the second and third stage of the scan, the short chunk alone in a stage, forward and
reverse) beside 6 000 samples.  sosfilt one-shot and in packets that end one before, at and after a tile; rows bit for bit alone,
again and reversed; int16; padlen 0, 127, 128, 129 and 1 024 (the odd extension shorter than, equal to and longer than a chunk,
and the limit); an output more than two tiles wider than the input.

Measured on the MI355X (first run; every figure is held to 8), worst (|y - y_ld| - 2^-24 |y_ld|) / D:
    sosfiltfilt, a filter per row, "tiles" (57 957 samples)        0
    sosfiltfilt, a filter per row, "scan" (530 168 samples)        0.259 (the row of SC + 1 positions at start 0.699), else 0
    sosfiltfilt, one filter at 0.699, "tiles"                      0
    sosfilt with zi, W - 1, W, W + 1, 2 W + 1, SC + 1 samples      0.062 one-shot, 0.067 in packets
    its final states, |zf - zf_ld| / max(D, SciPy's |zf - zf_ld|)  0.125 at worst, one-shot and in packets alike
    padlen 0 / 127 / 128 / 129 / 1 024                             0.649 / 0 / 0 / 0 / 0
    the output two tiles wider, modes 0 and 1                      0
1 084 243 samples are held to the bound in all.  The host restatement of the algorithm at the same lengths
(test_iir_host.py) gives 0.739 at worst."""
import ctypes

import numpy as np
import pytest
from scipy import signal

import iir_ref as ir
from iir_cases import (LONG_STARTS, PADLEN, SC, W, bits, check_bound, chunk, device, long_batch, long_refs, long_rows, poisoned,
                       sections)

pytestmark = pytest.mark.gpu

SEEN = [0]                                      # samples held to check_bound by this file


def flt():
    device()
    from tensorflowasr_amd.iir import SOSFilter
    return SOSFilter()


def bound(y, y_ld, D):
    SEEN[0] += len(y_ld)
    return check_bound(y, y_ld, D)


@pytest.mark.parametrize("which", ["tiles", "scan"])
def test_sosfiltfilt_with_a_filter_per_row(which):
    c = long_batch(which)
    y = flt().sosfiltfilt(c["x"], c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    assert y.dtype == np.float32 and y.shape == c["x"].shape and np.isfinite(y).all()
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        y_ld, D = long_refs(which)[b]
        r = bound(y[b, :n], y_ld, D)
        print("%s row %d: %d samples, start %g, D = %.3g, (|y - y_ld| - 2^-24 |y_ld|) / D = %.3f" % (which, b, n, c["starts"][b], D, r))
        worst = max(worst, r)
        assert not y[b, n:].any(), (b, n)
    print("sosfiltfilt, a filter per row, %s: worst ratio = %.3f over %d samples" % (which, worst, sum(c["lens"])))


def test_sosfiltfilt_with_a_shared_filter():
    c = long_batch("tiles")
    y = flt().sosfiltfilt(c["x"], c["lens"], sections(0.699)).cpu().numpy()
    assert np.isfinite(y).all()
    worst = 0.0
    for b, n in enumerate(c["lens"]):
        y_ld, D = long_refs("tiles", 0.699)[b]
        worst = max(worst, bound(y[b, :n], y_ld, D))
        assert not y[b, n:].any(), (b, n)
    print("sosfiltfilt, shared filter at 0.699, tiles: worst ratio = %.3f" % worst)


def test_sosfilt_with_states_one_shot_and_in_packets_that_end_around_a_tile():
    f = flt()
    lens = [W - 1, W, W + 1, 2 * W + 1, SC + 1]          # mode 0: N = L
    B = len(lens)
    rng = np.random.default_rng(23)
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    x = poisoned(rows, max(lens) + 7, np.float32)
    sos = np.stack([sections(LONG_STARTS[b % 3]) for b in range(B)])
    zi = rng.standard_normal((B, 3, 2)) * 0.1
    y, zf = f.sosfilt(x, lens, sos, zi=zi)
    y, zf = y.cpu().numpy(), zf.cpu().numpy()
    assert np.isfinite(y).all() and np.isfinite(zf).all()
    worst, worst_z, refs, zf_lds = 0.0, 0.0, [], []
    for b, n in enumerate(lens):
        r = rows[b].astype(np.float64)
        y_ld, zf_ld = ir.sosfilt_ld(sos[b], r, zi[b])
        ys, zs = signal.sosfilt(sos[b], r, zi=zi[b])
        D = ir.distance(ys, y_ld, r)
        refs.append((y_ld, D))
        worst = max(worst, bound(y[b, :n], y_ld, D))
        Dz = max(D, float(np.abs(zs - zf_ld).max()))
        zf_lds.append((zf_ld, Dz))
        ez = float(np.abs(zf[b] - zf_ld).max())
        print("row %d (%d samples): |zf - zf_ld| = %.3g, SciPy's %.3g, D = %.3g, ratio %.3f" % (b, n, ez, float(np.abs(zs - zf_ld).max()), D, ez / Dz))
        worst_z = max(worst_z, ez / Dz)
        assert ez <= 8 * Dz, b
        assert not y[b, n:].any(), (b, n)
    print("sosfilt with zi past the first tile: worst ratio = %.3f, worst zf ratio = %.3f" % (worst, worst_z))
    # the same rows as a stream cut at W - 1, W and 2 W + 1: packets end one before, at and after a tile
    cuts = [0, W - 1, W, 2 * W + 1, x.shape[1]]
    state, pieces = zi, []
    for lo, hi in zip(cuts, cuts[1:]):
        part, state = f.sosfilt(x[:, lo:hi], np.clip(np.array(lens) - lo, 0, hi - lo), sos, zi=state)
        pieces.append(part.cpu().numpy())
    got = np.concatenate(pieces, axis=1)
    state = state.cpu().numpy()
    worst = worst_z = 0.0
    for b, n in enumerate(lens):
        worst = max(worst, bound(got[b, :n], *refs[b]))
        ez = float(np.abs(state[b] - zf_lds[b][0]).max())
        worst_z = max(worst_z, ez / zf_lds[b][1])
        assert ez <= 8 * zf_lds[b][1], b
        assert not got[b, n:].any(), (b, n)
    print("sosfilt in packets around a tile: worst ratio = %.3f, worst zf ratio = %.3f" % (worst, worst_z))


def test_rows_do_not_depend_on_the_batch_on_the_run_or_on_their_position():
    f = flt()
    c = long_batch("tiles")
    B = len(c["lens"])
    kw = dict(padlen=PADLEN, noise_scale=0.001, quantise=True)
    y = f.sosfiltfilt(c["x"], c["lens"], c["sos"], noise=c["u"], **kw).cpu().numpy()
    assert np.array_equal(bits(f.sosfiltfilt(c["x"], c["lens"], c["sos"], noise=c["u"], **kw).cpu().numpy()), bits(y))
    order = list(range(B))[::-1]
    yr = f.sosfiltfilt(c["x"][order], [c["lens"][b] for b in order], c["sos"][order], noise=c["u"][order], **kw).cpu().numpy()
    assert np.array_equal(bits(yr), bits(y[order]))
    # quantised, with noise: still the long-double value but for single steps
    from iir_cases import check_quantised
    for b, n in enumerate(c["lens"]):
        check_quantised(y[b, :n], ir.quantise(np.asarray(long_refs("tiles")[b][0] + ir.LD(0.001) * c["us"][b], np.float64)))
    for which in ("tiles", "scan"):
        c = long_batch(which)
        if which == "scan":
            y = f.sosfiltfilt(c["x"], c["lens"], c["sos"], noise=c["u"], **kw).cpu().numpy()
        assert len(long_rows(which)) == (5 if which == "tiles" else 3)
        for b in long_rows(which):
            n = c["lens"][b]
            y1 = f.sosfiltfilt(c["x"][b, :n], None, c["sos"][b], noise=c["u"][b:b + 1, :n], **kw).cpu().numpy()
            assert np.array_equal(bits(y1[0]), bits(y[b, :n])), (which, b, n)


def test_int16_input_is_the_float32_call_on_x_over_32768():
    c = long_batch("tiles")
    f = flt()
    pcm = np.random.default_rng(5).integers(-32768, 32768, c["x"].shape).astype(np.int16)
    a = f.sosfiltfilt(pcm, c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    b = f.sosfiltfilt(pcm.astype(np.float32) / 32768, c["lens"], c["sos"], padlen=PADLEN).cpu().numpy()
    assert np.array_equal(bits(a), bits(b)) and float(np.abs(a).max()) > 0.5
    a, za = f.sosfilt(pcm, c["lens"], c["sos"])
    b, zb = f.sosfilt(pcm.astype(np.float32) / 32768, c["lens"], c["sos"])
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) and np.array_equal(bits(za.cpu().numpy()), bits(zb.cpu().numpy()))


@pytest.mark.parametrize("padlen", [0, 127, 128, 129, 1024])
def test_padlen_edges(padlen):
    """the odd extension one sample shorter than a chunk, a chunk, one sample longer (sample 0 at position 0 of chunk 1 and one
    to either side), none at all and the longest the library takes; rows of padlen + 1 samples (the shortest SciPy filters: every
    sample is mirrored on both sides) and rows whose extension ends at a tile and one position after it"""
    C = chunk()
    assert C == 128
    sos = sections(0.699)
    lens = ([padlen + 1] if padlen else []) + [W - 2 * padlen, W - 2 * padlen + 1]
    rng = np.random.default_rng(100 + padlen)
    rows = [(rng.uniform(-1, 1, n) * 0.5).astype(np.float32) for n in lens]
    y = flt().sosfiltfilt(poisoned(rows, max(lens) + 7, np.float32), lens, sos, padlen=padlen).cpu().numpy()
    assert np.isfinite(y).all()
    worst = 0.0
    for b, n in enumerate(lens):
        r = rows[b].astype(np.float64)
        y_ld = ir.sosfiltfilt_ld(sos, r, padlen)
        D = ir.distance(signal.sosfiltfilt(sos, r, padlen=padlen), y_ld, r)
        worst = max(worst, bound(y[b, :n], y_ld, D))
        assert not y[b, n:].any(), (b, n)
    print("padlen %d, rows of %s samples: worst ratio = %.3f" % (padlen, lens, worst))


def raw(x, lens, sos, mode, padlen, Opad, dtype=0):
    """mi355asr_sos_ragged itself on a shared filter -> (return code, y [B, Opad] NumPy, filled with 7.0 before the call)"""
    torch = device()
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    B, Lpad = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    ln = torch.tensor(list(lens), dtype=torch.int32, device="cuda:0")
    sd = torch.from_numpy(np.ascontiguousarray(sos, np.float64)).to("cuda:0")
    y = torch.full((B, Opad), 7.0, dtype=torch.float32, device="cuda:0")
    wb = ctypes.c_size_t()
    _lib.check(lib.mi355asr_sos_workspace_bytes(B, Lpad, len(sos), mode, ctypes.byref(wb)))
    ws = torch.empty(wb.value // 8 + 1, dtype=torch.float64, device="cuda:0")
    rc = lib.mi355asr_sos_ragged(p(xd), dtype, p(ln), B, Lpad, p(sd), len(sos), 1, mode, padlen, None, None, None, 0, 1.0, 0, p(y), Opad,
                                 p(ws), wb.value, None)
    torch.cuda.synchronize()
    return rc, y.cpu().numpy()


def test_padlen_past_the_limit_is_refused():
    from tensorflowasr_amd.iir import SOSFilter
    assert SOSFilter.MAX_PADLEN == 1024
    x = np.zeros((1, 4000), np.float32)
    with pytest.raises(ValueError, match="padlen = 1025 is outside 0 .. 1024"):
        flt().sosfiltfilt(x, None, sections(0.699), padlen=1025)
    rc, y = raw(x, [4000], sections(0.699), 1, 1025, 4000)
    assert rc == -1 and (y == 7.0).all()
    rc, y = raw(x, [4000], sections(0.699), 1, 1024, 4000)
    assert rc == 0 and not y.any()


@pytest.mark.parametrize("mode", [0, 1])
def test_an_output_more_than_two_tiles_wider_than_the_input(mode):
    """the tiles past the input's width exist for the output alone: zeros from every row's length to Opad (the fill branch two
    and three tiles above a row's end), the samples before them the bits of the call with Opad = Lpad"""
    c = long_batch("tiles")
    x, lens = c["x"][:, :W + 9], [min(n, W + 2) for n in c["lens"]]
    Lpad = x.shape[1]
    Opad = Lpad + 2 * W + 3
    rc0, y0 = raw(x, lens, sections(0.35), mode, PADLEN, Lpad)
    rc1, y1 = raw(x, lens, sections(0.35), mode, PADLEN, Opad)
    assert rc0 == 0 and rc1 == 0 and np.isfinite(y1).all()
    for b, n in enumerate(lens):
        assert not y1[b, n:].any() and not y0[b, n:].any(), (b, n)
        assert np.array_equal(bits(y1[b, :n]), bits(y0[b, :n])) and np.abs(y0[b, :n]).max() > 0.1, (b, n)
    # and the narrow call is the filter: the longest row against the long-double evaluation
    b = int(np.argmax(lens))
    r = x[b, :lens[b]].astype(np.float64)
    if mode:
        y_ld = ir.sosfiltfilt_ld(sections(0.35), r, PADLEN)
        D = ir.distance(signal.sosfiltfilt(sections(0.35), r, padlen=PADLEN), y_ld, r)
    else:
        y_ld = ir.sosfilt_ld(sections(0.35), r)[0]
        D = ir.distance(signal.sosfilt(sections(0.35), r), y_ld, r)
    print("mode %d, Opad = Lpad + 2 W + 3: ratio of the longest row = %.3f" % (mode, bound(y1[b, :lens[b]], y_ld, D)))
    print("samples held to the bound by this file so far: %d" % SEEN[0])
