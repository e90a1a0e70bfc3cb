"""The exact three-term bf16 operand split (csrc/mfma_ops.h: split8) on the hardware, bit for bit against NumPy.

Every three-term kernel turns an fp32 operand x into t0 + t1 + t2, each term the truncated high half (a bf16 value) of what the
terms before it left; the subtractions are exact, so nothing is left after three terms and nothing is rounded anywhere: the
comparison has no tolerance.  mi355asr_test_split_bf16 applies exactly that helper to an array and returns the three bit patterns;
the reference is split(x, 3, bf16_trunc) of test_split_arith.py.  The input set: that of the two-term test (test_split_f16.py),
its mantissa patterns again at every tenth exponent from 2^-90 to 2^100, and +-0 -- in that range the smallest non-zero term of
any value is 2^-113 or more, so no term or remainder is an fp32 subnormal and the result does not depend on the denormal mode.
Each value appears at an even and at an odd position, i.e. in the low and in the high half of the packed dword."""
import numpy as np
import pytest

from test_split_arith import bf16_trunc, split
from test_split_f16 import split_inputs


def split3_inputs():
    """float32 [n], n a few thousand (even), every value once at an even and once at an odd index"""
    base = split_inputs()
    mant = np.unique(base[(np.abs(base) >= 1.0) & (np.abs(base) < 2.0)].view(np.uint32) & np.uint32(0x7FFFFF))
    wide = []
    for e in range(-90, 101, 10):
        v = (np.uint32((e + 127) << 23) | mant).view(np.float32)
        wide += [v, -v]
    x = np.concatenate([base[: base.size // 2]] + wide + [np.array([0.0, -0.0], np.float32)]).astype(np.float32)
    x = np.concatenate([x, x[:1], x])          # second copy shifted by one: every value at both parities
    return x[: len(x) // 2 * 2]


def numpy_terms(x):
    """the three terms as bf16 bit patterns (uint16 [3, n]), and the remainder"""
    terms, rest = split(x, 3, bf16_trunc)
    return np.stack([(t.view(np.uint32) >> 16).astype(np.uint16) for t in terms]), terms, rest


def test_numpy_three_term_split_is_exact_on_the_input_set():
    """the reference side of the GPU test: three truncated terms decompose every input exactly, each a bf16 value, and the set
    really holds what the docstring lists"""
    x = split3_inputs()
    assert 3000 <= x.size <= 20000 and x.size % 2 == 0
    assert np.all(np.isfinite(x))
    bits, terms, rest = numpy_terms(x)
    assert np.all(rest == 0)                                               # nothing left after three terms
    total = terms[0].astype(np.float64) + terms[1].astype(np.float64) + terms[2].astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64))
    for t in terms:
        assert np.all((t.view(np.uint32) & 0xFFFF) == 0)                   # every term has a zero low half
    assert np.array_equal((bits.astype(np.uint32) << 16).view(np.float32), np.stack(terms))
    nz = np.concatenate([np.abs(t[t != 0]) for t in terms])
    assert nz.min() >= 2.0 ** -113 and (terms[2] != 0).sum() > 1000       # no subnormal term; the third term is exercised
    for e in list(range(-30, 16)) + list(range(-90, 101, 10)):             # every exponent, both signs, both parities
        for s in (1.0, -1.0):
            idx = np.flatnonzero(x == np.float32(s * 2.0 ** e))
            assert (idx % 2 == 0).any() and (idx % 2 == 1).any(), (e, s)
    z = np.flatnonzero(x == 0)
    for neg in (True, False):
        assert (z[np.signbit(x[z]) == neg] % 2 == 0).any() and (z[np.signbit(x[z]) == neg] % 2 == 1).any()


@pytest.mark.gpu
def test_three_term_split_on_the_gpu_equals_numpy_bit_for_bit():
    import torch
    from tensorflowasr_amd import _lib
    assert torch.cuda.is_available(), "this test needs the MI355X"
    x = split3_inputs()
    ref, _, _ = numpy_terms(x)
    lib = _lib.lib()
    xd = torch.from_numpy(x).cuda()
    td = torch.full((3, x.size), 0x5555, dtype=torch.int16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(n):
        td.fill_(0x5555)
        _lib.check(lib.mi355asr_test_split_bf16(xd.data_ptr(), n, td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), stream))
        torch.cuda.synchronize()
        return td.cpu().numpy().view(np.uint16)

    got = run(x.size)
    for k in range(3):
        bad = np.flatnonzero(got[k] != ref[k])
        show = [(int(i), float(x[i]).hex(), hex(int(got[k][i])), hex(int(ref[k][i]))) for i in bad[:8]]
        assert bad.size == 0, ("term %d differs at %d of %d" % (k, bad.size, x.size), show)
    # an odd count: the last element is split alone, and nothing behind it is written
    n = 4097
    got = run(n)
    assert np.array_equal(got[:, :n], ref[:, :n])
    assert np.all(got[:, n:] == 0x5555)
