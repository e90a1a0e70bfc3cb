"""Host side of the GPU scorer (tensorflowasr_amd/scoring.py): the recorded fixture against the host restatement of the
reference's recursion, the C ABI's declarations, the refusals that need no launch, and the host helpers.  No kernel runs here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from tensorflowasr_amd import _lib
from tensorflowasr_amd.eval import levenshtein

GOLDEN = os.path.join(ROOT, "tests", "golden")


def edge_cases():
    """[(name, ref u8, hyp u8, (distance, S, D, I))] of tests/golden/wer_edges.npz (make_wer_edges.py)"""
    z = np.load(os.path.join(GOLDEN, "wer_edges.npz"))
    ro, ho = z["ref_off"], z["hyp_off"]
    return [(str(name), z["ref"][ro[c]:ro[c + 1]], z["hyp"][ho[c]:ho[c + 1]], tuple(int(v) for v in z["expect"][c]))
            for c, name in enumerate(z["names"])]


def test_fixture_covers_the_edges_and_agrees_with_the_host_recursion():
    from tensorflowasr_amd.scoring import EditDistance
    cases = edge_cases()
    sizes = {(len(u), len(v)) for _, u, v, _ in cases}
    short = [0, 1, 2, 63, 64, 65, 127, 128, 129]
    assert all((n, m) in sizes for n in short for m in short)
    S = EditDistance.STRIP
    for x in (S - 1, S, S + 1, 2 * S + 1):
        assert (x, x) in sizes and any(n == x and m < 64 for n, m in sizes) and any(m == x and n < 64 for n, m in sizes)
    assert {(5, 3000), (3000, 5), (EditDistance.MAX_LEN, EditDistance.MAX_LEN)} <= sizes
    checked = 0
    for name, u, v, (dist, s, d, i) in cases:
        assert dist == s + d + i, name
        assert abs(len(u) - len(v)) <= dist <= max(len(u), len(v)) and d - i == len(u) - len(v), name
        if len(u) <= 300 and len(v) <= 300:
            assert levenshtein(u.tolist(), v.tolist()) == (dist, (s, d, i)), name
            checked += 1
    assert checked >= 81


def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "mi355asr.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "include/mi355asr.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_ctypes_table_and_argument_counts_agree():
    lib = _lib.lib()
    for name in ("mi355asr_edit_distance_workspace_bytes", "mi355asr_edit_distance"):
        args = _prototype(name)
        res, argtypes = _lib.SIGNATURES[name]
        assert hasattr(lib, name) and res is ctypes.c_int and len(args) == len(argtypes), name
        for decl, ct in zip(args, argtypes):
            if "*" in decl:
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, decl)
            elif decl.startswith("size_t"):
                assert ct is ctypes.c_size_t, (name, decl)
            else:
                assert decl.startswith("int32_t") and ct is ctypes.c_int32, (name, decl)


def test_workspace_formula_and_refusals_before_any_launch():
    from tensorflowasr_amd.scoring import EditDistance
    lib = _lib.lib()
    n = ctypes.c_size_t(12345)

    def up(v):
        return (v + 255) // 256 * 256
    for B, N, M in ((1, 1, 1), (3, 129, 65), (64, 40, 31), (2, 16384, 16384)):
        assert lib.mi355asr_edit_distance_workspace_bytes(B, N, M, 0, ctypes.byref(n)) == 0
        assert n.value == up(16 * B * (N + 1)) + up(4 * B * N) + up(4 * B * M)
    assert lib.mi355asr_edit_distance_workspace_bytes(3, 129, 65, 1, ctypes.byref(n)) == 0
    assert n.value == up(16 * 3 * 130) + up(4 * 3 * 9 * 65) + up(4 * 3 * 129) + up(4 * 3 * 65)
    assert lib.mi355asr_edit_distance_workspace_bytes(1, 4096, 4096, 1, ctypes.byref(n)) == 0      # exactly 2^24 cells
    n.value = 777
    L = EditDistance.MAX_LEN
    for B, N, M, ops in ((1, L + 1, 5, 0), (1, 5, L + 1, 0), (1, 4096, 4097, 1), (0, 5, 5, 0), (1, 0, 5, 0), (1, 5, 0, 0)):
        assert lib.mi355asr_edit_distance_workspace_bytes(B, N, M, ops, ctypes.byref(n)) == -1, (B, N, M, ops)   # MI355ASR_EINVAL
        assert b"edit distance" in lib.mi355asr_last_error() and n.value == 777
    assert 4096 * 4096 == EditDistance.MAX_ALIGN_CELLS and EditDistance.STRIP == 1024 and L == 16384
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "edit_distance.hip")).read()
    assert "kStrip = %d;" % EditDistance.STRIP in src and "kMaxLen = %d;" % L in src
    # null pointers and an over-long drop set never reach a launch either
    assert lib.mi355asr_edit_distance(None, None, None, None, 1, 4, 4, None, 0, None, 0, 0, 0, None, None, None, None, None, 0, None) == -1


def test_testers_default_to_host_scoring():
    from tensorflowasr_amd.chunk_asr import ChunkAMTester
    from tensorflowasr_amd.eval import AMTester
    for cls in (AMTester, ChunkAMTester):
        assert inspect.signature(cls.__init__).parameters["device_scoring"].default is False


def test_host_helpers():
    from tensorflowasr_amd.scoring import EditDistance, confusions, filter_row, score_transcripts
    assert filter_row([5, 0, 7, 1, 9, 0], drop=(0,), stop=1) == [5, 7]
    assert filter_row([1, 2, 3], drop=(), stop=1) == [] and filter_row([4, 2, 4], drop=(4, 9)) == [2]
    assert filter_row([4, 2, 4], drop=(), stop=7) == [4, 2, 4]
    # ref a b c d, hyp a x c c e: match, substitution b -> x, match, substitution d -> c, insertion e
    ref, hyp = [10, 11, 12, 13], [10, 99, 12, 12, 77]
    ops = np.array([0, 1, 0, 1, 3, 255, 255, 255, 255], np.uint8)
    assert confusions(ref, hyp, ops, np.int32(5)) == ({(11, 99): 1, (13, 12): 1}, {}, {77: 1})
    sub, dele, ins = confusions([ref, [1, 2, 3]], [hyp, [3]], np.stack([ops, np.array([2, 2, 0] + [9] * 6, np.uint8)]), np.array([5, 3]))
    assert sub == {(11, 99): 1, (13, 12): 1} and dele == {1: 1, 2: 1} and ins == {77: 1}
    with pytest.raises(ValueError):
        confusions(ref, hyp, ops, np.int32(4))
    with pytest.raises(ZeroDivisionError):
        score_transcripts(["abc", ""], ["abd", "x"])
    assert score_transcripts([], []) == []
    with pytest.raises(_lib.Mi355AsrError):
        EditDistance("cpu")
