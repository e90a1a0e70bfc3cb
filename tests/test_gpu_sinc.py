"""The band-limited resampler on the MI355X (mi355asr_sinc_resample, resample.SincResampler) against the tests' float64 restatement
of the published algorithm (sinc_ref.py; not the resampy package, which is not available): every ratio at every length where a
wing, a tile or the row ends, in ONE ragged batch with NaN behind every row and 7.0 in the output buffer; rows of 200 000 samples
(the position arithmetic past t = 2^17); repeatability and row independence bit for bit; the write-at-offset mode; refusals."""
import ctypes
import functools

import numpy as np
import pytest

import sinc_ref as sn
from stft_cases import bits, device, worst_ratio

pytestmark = pytest.mark.gpu

RATIOS = [0.25, 2 ** (-3 / 12), 0.9, 0.999, 1.0, 1.0000001, 1.5, 2 ** (3 / 12), 4.0]
U24 = 2.0 ** -24
# |y - y64| <= C_R 2^-24 S1[t], S1 = sum_k |w_k x_k|: four times the worst ratio of the float32 restatement on the host (14.6,
# test_sinc_host.py), rounded up to a power of two -- not a figure taken from the kernel.  The kernel's own worst ratios on the
# MI355X (printed below), in the order of RATIOS: 16.72, 11.98, 15.16, 15.81, 14.14, 9.18, 11.96, 11.26,
# 13.89; the rows of 200 000 samples 15.50 (ratio 2^(2.999 / 12)) and 15.10 (ratio 0.9).
C_R = 64.0


def noise(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)         # N(0, 1): stft_cases.signal without its 0.3


def wing(r):
    return sn.NW // int(min(1.0, r) * sn.NT)


def resampler(mode=0):
    device()
    from tensorflowasr_amd.resample import SincResampler
    return SincResampler(table_mode=mode)


def short_lengths(r):
    K = wing(r)
    return [0, 1, 2, K - 1, K, K + 1, 2 * K + 1]


def lengths_of(r, tile):
    """the ends of a wing, the input span of one and of two output tiles (each - 1, + 0, + 1), and 6000"""
    n1, n2 = int(np.ceil(tile / r)), int(np.ceil(2 * tile / r))
    return short_lengths(r) + [n1 - 1, n1, n1 + 1, n2 - 1, n2, n2 + 1, 6000]


def run(rs, x, lens, ratios, out_lens=None, offs=None, width=None, fill=7.0):
    """the library call on a prefilled buffer -> (y NumPy [B, width], valid)"""
    import torch
    lens = np.asarray(lens, np.int64)
    ratios = np.ascontiguousarray(ratios, np.float64)
    if out_lens is None:
        out_lens = np.array([sn.out_length(n, r) for n, r in zip(lens, ratios)], np.int64)
    width = int(max(1, np.max(out_lens)) + 3) if width is None else width
    y = torch.full((len(lens), width), fill, dtype=torch.float32, device="cuda:0")
    valid = rs.launch(torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0"), lens, ratios, out_lens, offs, y)
    torch.cuda.synchronize()
    return y.cpu().numpy(), valid


@functools.lru_cache(maxsize=None)
def batch():
    """every ratio and length in one ragged batch: inputs, float64 references (computed once) and the device's result"""
    rs = resampler()
    rng = np.random.default_rng(2024)
    rows = [(r, n) for r in RATIOS for n in lengths_of(r, rs.tile)]
    ratios = np.array([r for r, _ in rows])
    lens = np.array([n for _, n in rows], np.int64)
    x = np.full((len(rows), int(lens.max()) + 5), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = noise(rng, n)
    ref = [sn.resample(x[b, :n], r) for b, (r, n) in enumerate(rows)]
    y, valid = run(rs, x, lens, ratios)
    return {"rs": rs, "rows": rows, "ratios": ratios, "lens": lens, "x": x, "ref": ref, "y": y, "valid": valid}


def check_row(y, y64, s1, n, r):
    """the bound, and the exact parts: zeros where nothing contributes and from floor(n r) to the end of the buffer"""
    out_len, whole = sn.out_length(n, r), sn.valid_length(n, r)
    assert len(y64) == out_len and np.isfinite(y).all()
    assert not y[whole:].any(), (n, r)
    return worst_ratio(np.abs(y[:out_len] - y64), C_R * U24 * s1) * C_R


def test_every_ratio_and_length_in_one_batch():
    c = batch()
    assert c["rs"].tile >= 64 and c["rs"].ratio_min <= 0.25 and c["rs"].ratio_max >= 4.0
    worst = {r: 0.0 for r in RATIOS}
    for b, (r, n) in enumerate(c["rows"]):
        y64, s1 = c["ref"][b]
        assert c["valid"][b] == sn.valid_length(n, r), (r, n)
        worst[r] = max(worst[r], check_row(c["y"][b], y64, s1, n, r))
    for r in RATIOS:
        print("sinc ratio %.9g: wing %d, worst ratio %.3f" % (r, wing(r), worst[r]))
    assert max(worst.values()) <= C_R
    # the Python call: the same bits, exact lengths, its own zero fill
    y, out_len = c["rs"](c["x"], c["lens"], c["ratios"])
    want = [sn.out_length(n, r) for r, n in c["rows"]]
    assert list(out_len.cpu().numpy()) == want and out_len.dtype.is_floating_point is False and y.shape[1] == max(want)
    assert np.array_equal(bits(y.cpu().numpy()), bits(c["y"][:, :max(want)]))
    # a caller's output lengths: cut, and zero-filled; a narrower and a wider buffer
    pick = [b for b, (r, n) in enumerate(c["rows"]) if n == 6000]
    ol = [want[b] + (17 if k % 2 else -17) for k, b in enumerate(pick)]
    y2, l2 = c["rs"](c["x"][pick], c["lens"][pick], c["ratios"][pick], out_lengths=ol, out_pad=max(ol) + 9)
    y2 = y2.cpu().numpy()
    assert list(l2.cpu().numpy()) == ol and y2.shape[1] == max(ol) + 9
    for k, b in enumerate(pick):
        m = min(ol[k], want[b])
        assert np.array_equal(bits(y2[k, :m]), bits(c["y"][b, :m])) and not y2[k, m:].any()
    y3, l3 = c["rs"](c["x"][pick], c["lens"][pick], c["ratios"][pick], out_pad=1000)
    assert y3.shape[1] == 1000 and list(l3.cpu().numpy()) == [1000] * len(pick)
    assert np.array_equal(bits(y3.cpu().numpy()), bits(c["y"][pick, :1000]))


@pytest.mark.parametrize("r", [2 ** (2.999 / 12), 0.9])
def test_long_rows(r):
    """200 000 samples: t passes 2^17, where an fp32 position is several table entries off (orders of magnitude over the bound)"""
    rs = resampler()
    n = 200000
    x = noise(np.random.default_rng(8), (1, n))
    y, valid = run(rs, x, [n], [r])
    y64, s1 = sn.resample(x[0], r)
    assert valid[0] == sn.valid_length(n, r) and len(y64) > 2 ** 17
    worst = check_row(y[0], y64, s1, n, r)
    print("sinc long row, ratio %.9g: %d outputs, worst ratio %.3f" % (r, len(y64), worst))
    assert worst <= C_R


def test_runs_repeat_rows_are_independent_and_both_table_paths_agree():
    c = batch()
    rs = c["rs"]
    y2, _ = run(rs, c["x"], c["lens"], c["ratios"])
    assert np.array_equal(bits(y2), bits(c["y"]))
    y3, _ = run(resampler(1), c["x"], c["lens"], c["ratios"])       # the table through the caches: the same chain
    assert np.array_equal(bits(y3), bits(c["y"]))
    for b, (r, n) in enumerate(c["rows"]):
        if n not in short_lengths(r):
            continue
        y1, _ = run(rs, c["x"][b:b + 1, :max(n, 1)], [n], [r])
        m = sn.out_length(n, r)
        assert np.array_equal(bits(y1[0, :m]), bits(c["y"][b, :m])) and not y1[0, m:].any(), (r, n)


def test_write_at_offset():
    c = batch()
    rs = c["rs"]
    pick = [b for b, (r, n) in enumerate(c["rows"]) if n in (6000, wing(r) + 1)]
    L = 24300
    ol = np.array([sn.out_length(n, r) for r, n in (c["rows"][b] for b in pick)], np.int64)
    assert ol.max() + 255 <= L and len(pick) == 2 * len(RATIOS)
    offs = np.array([(0, 1, 255, L - ol[k])[k % 4] for k in range(len(pick))], np.int64)
    y, _ = run(rs, c["x"][pick], c["lens"][pick], c["ratios"][pick], out_lens=ol, offs=offs, width=L)
    for k, b in enumerate(pick):
        assert np.array_equal(bits(y[k, offs[k]:offs[k] + ol[k]]), bits(c["y"][b, :ol[k]])), (k, c["rows"][b])
        assert (y[k, :offs[k]] == 7.0).all() and (y[k, offs[k] + ol[k]:] == 7.0).all()
    # shorter and longer than the row gives: cut, and zeros up to out_len only
    ol2 = np.where(np.arange(len(pick)) % 2 == 0, ol + 9, np.maximum(ol - 9, 0))
    offs2 = np.minimum(offs, L - ol2)
    y, _ = run(rs, c["x"][pick], c["lens"][pick], c["ratios"][pick], out_lens=ol2, offs=offs2, width=L)
    for k, b in enumerate(pick):
        m = min(ol[k], ol2[k])
        assert np.array_equal(bits(y[k, offs2[k]:offs2[k] + m]), bits(c["y"][b, :m]))
        assert not y[k, offs2[k] + m:offs2[k] + ol2[k]].any()
        assert (y[k, :offs2[k]] == 7.0).all() and (y[k, offs2[k] + ol2[k]:] == 7.0).all()
    # every row empty: nothing is written
    y, _ = run(rs, c["x"][pick], [0] * len(pick), c["ratios"][pick], out_lens=[0] * len(pick), offs=offs, width=L)
    assert (y == 7.0).all()


def test_refusals():
    torch = device()
    from tensorflowasr_amd import _lib
    rs = resampler()
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    x = torch.zeros((2, 1000), dtype=torch.float32, device="cuda:0")
    y = torch.full((2, 4000), 7.0, dtype=torch.float32, device="cuda:0")
    ws = torch.full((64,), 7.0, dtype=torch.float64, device="cuda:0")
    tab = rs.table()

    def call(ratios=(1.0, 1.0), lens=(1000, 500), B=2):
        r, ln = np.array(ratios, np.float64), np.array(lens, np.int64)
        return lib.mi355asr_sinc_resample(p(x), B, 1000, hp(r), hp(ln), None, None, None, p(tab), 0, p(y), 4000, p(ws), 512, None)
    lo, hi = rs.ratio_min, rs.ratio_max
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), lo * (1 - 1e-9), hi * (1 + 1e-9)):
        assert call(ratios=(1.0, bad)) == -1, bad
        assert b"row 1" in lib.mi355asr_last_error() and b"outside 0.25 .. 4" in lib.mi355asr_last_error()
        with pytest.raises(ValueError, match="row 1: the ratio .* is outside the supported 0.25 .. 4"):
            rs(np.zeros((2, 1000), np.float32), None, [1.0, bad])
        with pytest.raises(ValueError, match="outside the supported 0.25 .. 4"):
            rs.wing(bad)
    assert call(B=0) == -1 and call(lens=(1000, -1)) == -1 and call(lens=(1001, 5)) == -1
    with pytest.raises(ValueError, match="empty batch"):
        rs(np.zeros((0, 1000), np.float32))
    with pytest.raises(ValueError, match="lengths"):
        rs(np.zeros((2, 1000), np.float32), [1000, -1])
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((ws == 7.0).all())
    assert call(ratios=(lo, hi)) == 0                                   # the bounds themselves are served
    torch.cuda.synchronize()
    assert not bool((y == 7.0).any()) and not bool(y.abs().sum() > 0)
