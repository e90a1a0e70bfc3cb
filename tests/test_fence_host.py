"""tests/fence.py on CPU tensors: what it hands out, what it catches, and that it leaves nothing patched behind."""
import types

import pytest
import torch

import fence
from fence import GUARD_BYTE, fenced

# a module "of the package": the fence serves only callers whose module name is tensorflowasr_amd[.*]
_SRC = """
import torch
def empty(*a, **k):
    return torch.empty(*a, **k)
def empty_like(t, **k):
    return torch.empty_like(t, **k)
def new_empty(t, *a, **k):
    return t.new_empty(*a, **k)
"""
pkg = types.ModuleType("tensorflowasr_amd._fence_probe")
exec(compile(_SRC, "fence_probe.py", "exec"), pkg.__dict__)


def _originals():
    return torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("guard", [512, 4096])
def test_shapes_dtypes_alignment_and_fill(fill, guard):
    cases = [((3, 5, 7), torch.float32), ((17,), torch.uint8), ((2, 3), torch.int32), ((4, 9), torch.float16),
             ((5,), torch.bfloat16), ((2, 2), torch.float64), ((0,), torch.float32), ((3, 0, 8), torch.int32), ((), torch.float32)]
    with fenced(fill, guard) as f:
        got = []
        for shape, dt in cases:
            got.append(pkg.empty(shape, dtype=dt, device="cpu"))
        got.append(pkg.empty(4, 6, dtype=torch.int32))                   # sizes as separate arguments
        got.append(pkg.empty(size=(2, 5), dtype=torch.float32))
        got.append(pkg.empty(3))                                         # the default dtype
        got.append(pkg.empty_like(torch.zeros((3, 4), dtype=torch.float16)))
        got.append(pkg.empty_like(torch.zeros((3, 4)), dtype=torch.int32))
        got.append(pkg.new_empty(torch.zeros(2, dtype=torch.int32), (6, 2)))
        got.append(pkg.new_empty(torch.zeros(2, dtype=torch.int32), 5, dtype=torch.float32))
        want = cases + [((4, 6), torch.int32), ((2, 5), torch.float32), ((3,), torch.float32), ((3, 4), torch.float16),
                        ((3, 4), torch.int32), ((6, 2), torch.int32), ((5,), torch.float32)]
        assert len(f.allocations) == len(want) == len(got)
        for t, a, (shape, dt) in zip(got, f.allocations, want):
            assert a.tensor is t
            assert tuple(t.shape) == shape and t.dtype == dt and t.device.type == "cpu" and t.is_contiguous(), a.name
            nbytes = t.numel() * t.element_size()
            assert a.backing.dtype == torch.uint8 and a.backing.numel() == 2 * guard + nbytes
            assert t.storage_offset() * t.element_size() == guard and guard % 512 == 0      # the backing's alignment is kept
            if t.numel():                                                # (an empty tensor has no address)
                assert t.data_ptr() - a.backing.data_ptr() == guard and t.data_ptr() % 512 == a.backing.data_ptr() % 512
            assert (a.payload() == fill).all() and a.payload().numel() == nbytes
            for g in a.guards():
                assert g.numel() == guard and (g == GUARD_BYTE).all()
            if fill == 0xFF and t.numel():
                if t.dtype.is_floating_point:
                    assert torch.isnan(t).all(), a.name                 # every float word of 0xFF bytes is a NaN
                elif t.dtype == torch.int32:
                    assert (t == -1).all()
                else:
                    assert (t == 255).all()
            if fill == 0x00:
                assert not t.any()
            assert "fence_probe.py:" in a.site and shape == tuple(a.tensor.shape) and str(shape) in a.name
        f.check()


def test_check_catches_one_byte_before_and_one_after():
    with fenced(0xFF, 512) as f:
        a = pkg.empty((3, 5), dtype=torch.float32)
        b = pkg.empty((7,), dtype=torch.int32)
        z = pkg.empty((0, 4), dtype=torch.float32)
        a.fill_(1.0)
        b.fill_(3)                                                       # writing every payload byte is fine
        f.check()
        ra, rb, rz = f.allocations
        rb.backing[512 - 1] = 0                                           # one byte before b's payload
        with pytest.raises(AssertionError) as e:
            f.check()
        msg = str(e.value)
        assert "before" in msg and "(7,)" in msg and "int32" in msg and "fence_probe.py:" in msg and "bytes 1 .. 1 before" in msg
        rb.backing[512 - 1] = GUARD_BYTE
        f.check()
        ra.backing[512 + 60] = 7                                          # one byte after a's 60 bytes
        with pytest.raises(AssertionError) as e:
            f.check()
        msg = str(e.value)
        assert "after" in msg and "(3, 5)" in msg and "float32" in msg and "bytes 1 .. 1 past" in msg
        ra.backing[512 + 60] = GUARD_BYTE
        ra.backing[512 + 59] = 7                                          # the payload's last byte: not the fence's business
        ra.backing[512] = 7
        f.check()
        rz.backing[512] = 0                                               # an empty payload: the second guard starts at once
        with pytest.raises(AssertionError, match=r"\(0, 4\)"):
            f.check()
        rz.backing[512] = GUARD_BYTE
        ra.backing[-1] = 0                                                # the guards' far ends
        with pytest.raises(AssertionError, match="bytes 512 .. 512 past"):
            f.check()
        ra.backing[-1] = GUARD_BYTE
        ra.backing[0] = 0
        with pytest.raises(AssertionError, match="bytes 512 .. 512 before"):
            f.check()


def test_only_the_package_is_served_and_everything_is_restored():
    before = _originals()
    with fenced(0x00) as f:
        mine = torch.empty((4, 4))                                       # this module is not the package's
        torch.empty_like(mine)
        mine.new_empty((2,))
        assert not f.allocations
        plain = pkg.empty((4,), dtype=torch.float32, pin_memory=False)   # a keyword the fence does not know: torch's own call
        assert not f.allocations and plain.shape == (4,)
        pkg.empty((4,))
        assert len(f.allocations) == 1 and f.guard == 4096
    assert _originals() == before
    assert pkg.empty((4,)).untyped_storage().nbytes() == 16              # plain torch again
    with pytest.raises(RuntimeError, match="boom"):
        with fenced(0xFF):
            pkg.empty((2,))
            raise RuntimeError("boom")
    assert _originals() == before
    with fenced(0x00):                                                   # nested blocks unwind in order
        with fenced(0xFF) as inner:
            assert torch.isnan(pkg.empty((2,))).all() and len(inner.allocations) == 1
    assert _originals() == before


def test_refused_fills_and_guards():
    for fill in (0x7F, 0x5A, 0x01, 256, -1):
        with pytest.raises(ValueError, match="fill"):
            with fenced(fill):
                pass
    for guard in (0, 100, 513, -512):
        with pytest.raises(ValueError, match="guard"):
            with fenced(0x00, guard):
                pass
    assert fence.FILLS == (0x00, 0xFF)
