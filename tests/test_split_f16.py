"""The two-term fp16 operand split (csrc/common.h: split_hi_f16 / split_lo_f16) on the hardware, bit for bit against NumPy.

Every two-term kernel turns an fp32 operand x (already multiplied by its power-of-two scale) into hi = fp16(x) and
lo = fp16(x - hi), both round-to-nearest-even.  The library forms lo with v_fma_mixlo_f16 / v_fma_mixhi_f16 reading the fp16 hi
in place; mi355asr_test_split_f16 applies exactly that helper to an array and returns the bit patterns.  The input set holds
every exponent from 2^-30 to 2^15, mantissas on and either side of the fp16 rounding ties (of hi and of lo), values whose lo is
an fp16 subnormal or zero, +-0, and the neighbourhood of the largest finite fp16 (where hi rounds to infinity); each value
appears at an even and at an odd position, i.e. goes through the low-half and the high-half instruction."""
import numpy as np
import pytest


def split_inputs():
    """float32 [n], n a few thousand (even), every value once at an even and once at an odd index"""
    vals = []
    # mantissa patterns in units of 2^-23 of the leading bit.  fp16 keeps 10 fraction bits: the hi tie sits at bit 12 (0x1000);
    # lo then keeps the next 11 bits or fewer, so bits 0 .. 2 decide lo's rounding, with its tie at 0x1 / 0x2 / 0x4 patterns.
    mant = [0x000000, 0x000001, 0x7fffff, 0x400000, 0x3fffff, 0x400001,
            0x001000, 0x000fff, 0x001001, 0x003000, 0x002fff, 0x003001,            # hi ties (to even: down, up) and neighbours
            0x7ff000, 0x7fefff, 0x7ff001, 0x7fe000, 0x7fdfff, 0x7fe001,            # hi rounds up into the next binade
            0x000800, 0x0007ff, 0x000801, 0x001800, 0x0017ff, 0x001801,            # lo = half an ulp of hi and neighbours
            0x000002, 0x000003, 0x000004, 0x000005, 0x000006, 0x000007,            # lo's own last bits: ties of the second rounding
            0x001002, 0x001003, 0x000ffd, 0x000ffe, 0x2aaaaa, 0x555555, 0x123456, 0x7edcba]
    for e in range(-30, 16):
        for m in mant:
            bits = np.uint32(((e + 127) << 23) | m)
            v = bits.view(np.float32)
            vals += [v, -v]
    # lo subnormal or zero: x = hi + d with |d| below 2^-14, around fp16 subnormal steps of 2^-24 and their ties
    for hi in (1.0, 0.5, 2.0 ** -3, 2.0 ** -10, 2.0 ** -14, 3.0 * 2.0 ** -16):
        for k in (0, 1, 2, 3, 1023, 1024):
            for frac in (0.0, 0.25, 0.5, 0.75):
                d = (k + frac) * 2.0 ** -24
                vals += [np.float32(hi + d), np.float32(hi - d), np.float32(-(hi + d))]
    vals += [np.float32(0.0), np.float32(-0.0)]
    # the largest finite fp16 (65504): below, on and above the point where hi becomes infinity (65520)
    for v in (65503.0, 65504.0, 65504.004, 65505.0, 65512.0, 65519.0, 65519.996, 65520.0, 65520.004, 65528.0, 65535.0, 65536.0):
        vals += [np.float32(v), np.float32(-v)]
    x = np.array(vals, np.float32)
    x = np.concatenate([x, x[:1], x])          # second copy shifted by one: every value at both parities
    return x[: len(x) // 2 * 2]


def numpy_split(x):
    """(hi, lo) as float16: hi = float16(x), lo = float16(float32(x) - float32(hi))"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x.astype(np.float32) - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def test_numpy_split_is_an_exact_two_term_decomposition():
    """the reference side of the GPU test: x - hi is exact in fp32, |x - hi - lo| <= 2^-22 |x| wherever lo is a normal fp16
    (or zero with an exact remainder), and the set really holds what the docstring lists"""
    x = split_inputs()
    assert 3000 <= x.size <= 20000 and x.size % 2 == 0
    hi, lo = numpy_split(x)
    fin = np.isfinite(hi.astype(np.float64))
    assert (~fin).sum() >= 8 and fin.sum() > 3000                    # the overflow neighbourhood is there, and is small
    x64, hi64, lo64 = x.astype(np.float64)[fin], hi.astype(np.float64)[fin], lo.astype(np.float64)[fin]
    with np.errstate(invalid="ignore"):
        rem32 = x.astype(np.float32) - hi.astype(np.float32)
    assert np.array_equal(rem32[fin].astype(np.float64), x64 - hi64), "x - hi must be exact in fp32"
    normal = np.abs(lo64) >= 2.0 ** -14
    sub = ~normal
    assert normal.sum() > 1000 and sub.sum() > 200 and (lo64 == 0).sum() > 50
    assert np.all(np.abs(x64 - hi64 - lo64)[normal] <= 2.0 ** -22 * np.abs(x64)[normal])
    assert np.all(np.abs(x64 - hi64 - lo64)[sub] <= 2.0 ** -25)     # subnormal lo: half a step of 2^-24, absolute
    for e in range(-30, 16):                                         # every exponent, both signs, both parities
        for s in (1.0, -1.0):
            idx = np.flatnonzero(x == np.float32(s * 2.0 ** e))
            assert (idx % 2 == 0).any() and (idx % 2 == 1).any(), (e, s)
    z = np.flatnonzero(x == 0)
    assert np.signbit(x[z]).any() and (~np.signbit(x[z])).any()


@pytest.mark.gpu
def test_split_on_the_gpu_equals_numpy_bit_for_bit():
    import torch
    from tensorflowasr_amd import _lib
    assert torch.cuda.is_available(), "this test needs the MI355X"
    x = split_inputs()
    hi_ref, lo_ref = numpy_split(x)
    lib = _lib.lib()
    xd = torch.from_numpy(x).cuda()
    hid = torch.full((x.size,), 0x5555, dtype=torch.int16, device="cuda")
    lod = torch.full((x.size,), 0x5555, dtype=torch.int16, device="cuda")
    _lib.check(lib.mi355asr_test_split_f16(xd.data_ptr(), x.size, hid.data_ptr(), lod.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    hi = hid.cpu().numpy().view(np.uint16)
    lo = lod.cpu().numpy().view(np.uint16)
    bad_hi = np.flatnonzero(hi != hi_ref.view(np.uint16))
    bad_lo = np.flatnonzero(lo != lo_ref.view(np.uint16))
    show = lambda idx, got, ref: [(int(i), float(x[i]).hex(), hex(int(got[i])), hex(int(ref.view(np.uint16)[i]))) for i in idx[:8]]
    assert bad_hi.size == 0, ("hi differs at %d of %d" % (bad_hi.size, x.size), show(bad_hi, hi, hi_ref))
    assert bad_lo.size == 0, ("lo differs at %d of %d" % (bad_lo.size, x.size), show(bad_lo, lo, lo_ref))
    # an odd count: the last element is split alone
    n = 4097
    _lib.check(lib.mi355asr_test_split_f16(xd.data_ptr(), n, hid.data_ptr(), lod.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(hid.cpu().numpy().view(np.uint16)[:n], hi_ref.view(np.uint16)[:n])
    assert np.array_equal(lod.cpu().numpy().view(np.uint16)[:n], lo_ref.view(np.uint16)[:n])
