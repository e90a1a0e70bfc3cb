"""The tables of tests/dense_edges.py themselves (no GPU): every row count on the edge its comment names, every factorisation the
M it stands for, every leg's environment spelled as the library reads it, and -- from the float64 oracle alone -- at most 0.5 % of
every chosen input's frames with a top-2 margin inside 1e-3."""
import os
import re

import numpy as np
import pytest

import dense_edges as de
from helpers import co

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensorflowasr_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_defaults_of_the_code():
    assert re.search(r'mi355_env\("MI355ASR_RING_MIN_M", %d\)' % de.RING_MIN_M, _src("weights.hip"))
    ring = _src("gemm_ring.hip")
    assert "constexpr int GW = 8, GT = GW * 64;" in ring and "constexpr int GNB = 8;" in ring
    assert "const int r0 = blockIdx.x * (GW * 16 * RT);" in ring                     # 128 or 256 rows per workgroup
    assert de.RING_ROWS == (8 * 16, 8 * 16 * 2) and de.RING_CHUNK == 8 * 16
    # the projection holds a ring pack in the bf16 mode only: what assert_family expects of ctc_project
    assert "if (ring_packs_wanted(m) && ab.ring_terms == 1) put_ring(ab, so.proj_w, pj, d, d, false);" in _src("weights.hip")
    h = open(os.path.join(os.path.dirname(CSRC), "..", "include", "mi355asr.h")).read()
    for name, v in (("F32", de.F32), ("BF16X3", de.BF16X3), ("F16X2", de.F16X2), ("BF16", de.BF16)):
        assert re.search(r"#define MI355ASR_SCHEME_%s %d\b" % (name, v), h)


def test_every_leg_sets_switches_the_library_reads():
    read = set()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".inc")):
            read |= set(re.findall(r'(?:getenv|env_on|mi355_env)\("(MI355ASR_[A-Z0-9_]+)"', _src(f)))
    assert len(de.LEGS) == 1 + len(de.FORCED_SHAPES) + len(de.HEAD_RANGES) + len(de.SUBCONV_LEGS)
    for leg, env in de.LEGS.items():
        assert env and set(env) <= read, (leg, sorted(set(env) - read))
        assert all(isinstance(v, str) and v.isdigit() for v in env.values()), leg
    for leg, env in de.LEGS.items():
        if leg.startswith(("forced_", "ranges")):
            assert env["MI355ASR_RING_MIN_M"] == "1", leg
    assert de.LEGS["ring_off"] == {"MI355ASR_GEMM_RING": "0"}
    shapes = {k: {s[len("MI355ASR_RING_"):]: int(v) for s, v in e.items()} for k, e in de.FORCED_SHAPES.items()}
    assert shapes == {"rt1": {"RT": 1}, "rt2": {"RT": 2}, "slots2": {"SLOTS": 2}, "rt1_cpw2": {"RT": 1, "CPW": 2}, "rt2_cpw8": {"RT": 2, "CPW": 8}}
    # go() declines two row tiles per wave on a two-slot ring: no forced shape asks for both
    assert not any(s.get("RT") == 2 and s.get("SLOTS") == 2 for s in shapes.values())
    assert [int(de.LEGS["ranges%d" % n]["MI355ASR_RING_HEAD_RANGES"]) for n in de.HEAD_RANGES] == [1, 2, 3, 4]
    # MI355ASR_SUBCONV_RT is read by the two-term kernels only: every leg that sets it sends the features there
    for leg, env in de.SUBCONV_LEGS.items():
        assert env["MI355ASR_SUBCONV_TERMS"] == "22", leg
    assert {e.get("MI355ASR_SUBCONV_RT") for e in de.SUBCONV_LEGS.values()} == {None, "1", "2"}


def test_row_counts_sit_on_the_edges():
    assert de.N0_M == tuple(sorted(set(de.N0_M))) and len(de.N0_M) == 25
    for edge in (16, 128, 256, 384, de.RING_MIN_M, 1536, 1792, 2048):
        assert {edge - 1, edge, edge + 1} <= set(de.N0_M), edge
    assert 1 in de.N0_M
    # above the crossover: an edge of both workgroup sizes, of the 128-row one alone (1 792 = 14 x 128 = 7 x 256 is both; 1 536 too)
    assert 1536 % 256 == 0 and 1792 % 256 == 0 and 2048 % 256 == 0 and 1500 % 128 != 0
    for M in de.N0_M:
        if M >= de.RING_MIN_M and M % 128 == 1:
            assert -(-M // 128) * 128 - M == 127                          # one live row in the last workgroup
    assert sorted(de.N1_SHAPES) == [129, 257, 1499, 1500, 1501, 1537, 2049]
    for table in (de.N1_SHAPES, de.FORCED_N1):
        for M, (B, T) in table.items():
            assert B * T == M and T >= 17, (M, B, T)
            # T <= 288 where M allows it: some divisor pair with 17 <= T <= 288 exists
            fits = [t for t in range(17, 289) if M % t == 0]
            assert (T <= 288) == bool(fits), (M, T, fits)
    assert de.N1_SHAPES[1499] == (1, 1499) and all(1499 % k for k in range(2, 39))           # prime
    assert de.N1_SHAPES[1500] == (20, 75) and de.N1_SHAPES[1501] == (19, 79)
    assert [M for M in de.N0_M if M <= de.CHAIN_MAX_M][-1] == 385 and de.EXPECTED_ROWS < de.RING_MIN_M
    assert all(M >= de.RING_MIN_M for M in de.RING_OFF_M) and set(de.RING_OFF_M) <= set(de.N1_SHAPES) and set(de.RING_OFF_M) <= set(de.N0_M)
    # the forced shapes: two, three and four 128-row workgroups (one or two of 256), one row in the last
    assert [(-(-M // 128), M % 128) for M in de.FORCED_M] == [(2, 1), (3, 1), (4, 1)]
    assert [(-(-M // 256), M % 256) for M in de.FORCED_M] == [(1, 129), (2, 1), (2, 129)]
    assert set(de.FORCED_M) <= set(de.N0_M) and set(de.BF16_M) <= set(de.N1_SHAPES)
    assert min(de.BF16_M) < de.RING_MIN_M <= sorted(de.BF16_M)[1]
    assert de.HEADS == {256: 4, 512: 8}


def test_class_counts_sit_on_the_chunk_edges():
    assert de.HEAD_V == (5, 127, 128, 129, 201, 1332) and de.HEAD_M == (257, 1501)
    chunks = {V: -(-V // de.RING_CHUNK) for V in de.HEAD_V}
    assert chunks == {5: 1, 127: 1, 128: 1, 129: 2, 201: 2, 1332: 11}
    assert 201 % 4 != 0 and all(V % 4 == 0 or V in (5, 127, 129, 201) for V in de.HEAD_V)    # ldy & 3: the element-wise stores
    assert min(de.HEAD_M) < de.RING_MIN_M <= max(de.HEAD_M) and [M % 128 for M in de.HEAD_M] == [1, 93]      # a partial last row tile
    # the ranges go() forms at 11 chunks: c = ceil(11 / nr) chunks each, the last one the rest
    for nr, last in ((1, 11), (2, 5), (3, 3), (4, 2)):
        c = -(-11 // nr)
        assert -(-11 // c) == nr and 11 - c * (nr - 1) == last, nr
    assert de.HEAD_RANGES_V == 1332 and de.HEAD_RANGES == (1, 2, 3, 4)


def test_subsampling_lengths_hold_every_padding_parity():
    assert de.SUBCONV_F == (1, 2, 3, 4, 5, 6, 7, 8, 25, 26, 27, 28, 49, 50, 51, 52, 101, 102, 103, 104) and de.SUBCONV_B == 3
    for group in (range(1, 9), range(25, 29), range(49, 53), range(101, 105)):
        par = {(F % 2, de.subconv_geometry(F)[0] % 2) for F in group}
        assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}, list(group)
        assert {de.subconv_geometry(F)[2:] for F in group} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # rows of padding in front
    pos = sorted({20 * de.subconv_geometry(F)[1] for F in de.SUBCONV_F})
    assert pos == [20, 40, 140, 260, 520]
    assert any(p < 128 for p in pos) and any(128 < p < 256 for p in pos) and any(p > 256 for p in pos)
    from ragged_edges import COMBOS, L_for, geometry_for
    for d, cases in de.WAVE_CASES.items():
        assert [T for T, _ in cases] == [17, 33]
    combos = [c for cases in de.WAVE_CASES.values() for _, c in cases]
    assert len(set(combos)) == 4 and all(0 <= c < len(COMBOS) for c in combos)
    assert {COMBOS[c][:2] for c in combos} == {(False, False), (False, True), (True, False), (True, True)}
    for cases in de.WAVE_CASES.values():
        for T, c in cases:
            L = L_for(T, *COMBOS[c])
            F = -(-L // 160)
            assert F == geometry_for(T, *COMBOS[c])["F"] and -(-(-(-F // 2)) // 2) == T


def test_inputs_are_seeded_by_the_case():
    a, b = de.case_input(256, 1, 1501), de.case_input(256, 1, 1501)
    assert a.shape == (19, 79, 256) and a.dtype == np.float32 and np.array_equal(a, b)
    assert de.case_input(512, 0, 2049).shape == (1, 2049, 512)
    assert not np.array_equal(de.case_input(256, 0, 257)[0, :129], de.case_input(256, 0, 129)[0])
    w = de.weights(256, 0, 129)
    assert w["fully_connected/bias"].shape == (129,) and w["fully_connected/bias"].any() and w["project/bias"].any()
    assert len(de.dense_cases()) == len(set(de.dense_cases())) == 2 * (25 + 7 + 1)
    assert len(de.head_cases()) == 12


_W = {}


def _oracle64(d, n, M, V):
    if (d, n, V) not in _W:
        _W[d, n, V] = de.weights(d, n, V)
    return co.ctc_decoder(de.case_input(d, n, M, V).astype(np.float64), _W[d, n, V], de.cfg_for(d, n))


@pytest.mark.parametrize("d", de.DMODELS)
def test_undecided_frames_stay_under_the_cap_for_every_chosen_input(d):
    """the share of frames whose float64 logits leave the arg-max open (top-2 margin <= 1e-3), per case: at most MAX_EXCUSED.  A
    seed that misses is replaced in dense_edges.RESEED; the cap stays."""
    assert de.MAX_EXCUSED == 0.005 and de.MARGIN == 1e-3
    over = []
    cases = [c + (de.V_DENSE,) for c in de.dense_cases() if c[0] == d] + [c for c in de.head_cases() if c[0] == d]
    for dd, n, M, V in cases:
        share = de.undecided_share(_oracle64(dd, n, M, V))
        if share > de.MAX_EXCUSED:
            over.append(((dd, n, M, V), share))
    assert not over, over
