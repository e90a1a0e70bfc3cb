"""A poisoned, fenced allocator for tests of the C ABI's caller contract (include/mi355asr.h, "Conventions").

    with fenced(0xFF) as f:
        out = model.recognize(wav)          # every torch.empty / empty_like / new_empty the package issues is fenced
        torch.cuda.synchronize()
        f.check()                           # no guard byte was written

While the block is active, every `torch.empty`, `torch.empty_like` and `Tensor.new_empty` called FROM A MODULE OF THE PACKAGE
(`tensorflowasr_amd.*`; any other caller gets torch's own function) is served from a flat uint8 buffer of guard + nbytes + guard
bytes: the payload filled with `fill`, both guards with 0xA5.  The caller gets the inner view with the shape, dtype and device it
asked for, contiguous, aligned as a torch allocation is (guard is a multiple of 512).  Workspaces are therefore exactly as large
as the wrapper asked for, outputs and opaque state hold `fill` where the library left them unwritten, and a write a few rows past
either lands in a guard.  Plain Python: the three names are patched for the duration of the block and restored on exit, also
after an exception.

Fills: 0x00 (the baseline) and 0xFF (every fp32 / fp16 / bf16 word a NaN, every int32 -1: as a length it runs no loop, as an
index it stays next to its buffer).  A fill whose int32 reading is a large positive number is refused: an index read from it
would leave the allocation."""
import contextlib
import sys
import traceback

import torch

PACKAGE = "tensorflowasr_amd"
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF)


class Allocation:
    """one fenced tensor: `backing` (uint8, guard + nbytes + guard), `tensor` (the view handed out), where it was asked for"""

    def __init__(self, backing, tensor, guard, site):
        self.backing, self.tensor, self.guard, self.site = backing, tensor, guard, site
        self.nbytes = tensor.numel() * tensor.element_size()

    @property
    def name(self):
        return "%s %s allocated at %s" % (tuple(self.tensor.shape), str(self.tensor.dtype).replace("torch.", ""), self.site)

    def payload(self):
        return self.backing[self.guard:self.guard + self.nbytes]

    def guards(self):
        return self.backing[:self.guard], self.backing[self.guard + self.nbytes:]


class Fence:
    def __init__(self, fill, guard):
        if fill not in FILLS:
            raise ValueError("fill 0x%02X: only 0x00 and 0xFF (an int32 index read from the fill must stay next to its buffer)" % fill)
        if guard <= 0 or guard % 512:
            raise ValueError("guard %d: a positive multiple of 512 keeps the alignment of a torch allocation" % guard)
        self.fill, self.guard, self.allocations = fill, guard, []

    def allocate(self, real_empty, size, dtype, device, site):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        n = 1
        for s in size:
            n *= int(s)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        backing = real_empty(2 * self.guard + nbytes, dtype=torch.uint8, device=device)
        backing.fill_(GUARD_BYTE)
        backing[self.guard:self.guard + nbytes].fill_(self.fill)
        t = backing[self.guard:self.guard + nbytes].view(dtype).view(tuple(int(s) for s in size))
        a = Allocation(backing, t, self.guard, site)
        self.allocations.append(a)
        return t

    def check(self):
        """every guard byte of every allocation is intact; names the first allocation whose guard is not"""
        for a in self.allocations:
            for side, g in zip(("before", "after"), a.guards()):
                bad = (g != GUARD_BYTE).nonzero()
                if bad.numel():
                    lo, hi = int(bad[0, 0]), int(bad[-1, 0])
                    if side == "before":
                        where = "bytes %d .. %d before its first byte" % (self.guard - hi, self.guard - lo)
                    else:
                        where = "bytes %d .. %d past its last byte" % (lo + 1, hi + 1)
                    raise AssertionError("the guard %s %s was written: %d bytes changed, %s" % (side, a.name, bad.shape[0], where))


def _size_of(args, kwargs):
    if "size" in kwargs:
        return tuple(kwargs.pop("size"))
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(args[0])
    return tuple(args)


def _site(depth=2):
    f = sys._getframe(depth)
    fs = traceback.extract_stack(f, limit=1)[0]
    return "%s:%d in %s" % (fs.filename.rsplit("/", 1)[-1], fs.lineno, fs.name)


def _from_package(depth=2):
    name = sys._getframe(depth).f_globals.get("__name__", "")
    return name == PACKAGE or name.startswith(PACKAGE + ".")


_PLAIN = {"dtype", "device", "size", "requires_grad"}


@contextlib.contextmanager
def fenced(fill, guard=4096):
    fence = Fence(fill, guard)
    real_empty, real_like = torch.empty, torch.empty_like
    had_new = "new_empty" in torch.Tensor.__dict__
    real_new = torch.Tensor.new_empty

    def empty(*args, **kwargs):
        if not _from_package() or set(kwargs) - _PLAIN or kwargs.get("requires_grad"):
            return real_empty(*args, **kwargs)
        kwargs.pop("requires_grad", None)
        size = _size_of(args, kwargs)
        return fence.allocate(real_empty, size, kwargs.get("dtype"), kwargs.get("device"), _site())

    def empty_like(t, **kwargs):
        if not _from_package() or set(kwargs) - _PLAIN or kwargs.get("requires_grad"):
            return real_like(t, **kwargs)
        return fence.allocate(real_empty, tuple(t.shape), kwargs.get("dtype") or t.dtype, kwargs.get("device") or t.device, _site())

    def new_empty(self, *args, **kwargs):
        if not _from_package() or set(kwargs) - _PLAIN or kwargs.get("requires_grad"):
            return real_new(self, *args, **kwargs)
        kwargs.pop("requires_grad", None)
        size = _size_of(args, kwargs)
        return fence.allocate(real_empty, size, kwargs.get("dtype") or self.dtype, kwargs.get("device") or self.device, _site())

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield fence
    finally:
        torch.empty, torch.empty_like = real_empty, real_like
        if had_new:
            torch.Tensor.new_empty = real_new
        else:
            del torch.Tensor.new_empty
