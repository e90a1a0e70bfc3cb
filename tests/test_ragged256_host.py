"""The batch tables of tests/ragged256_edges.py themselves (no GPU): every batch on the side of 1 500 / 2 048 / 8 192 rows its name
says, every attention class of attn64_class (csrc/launch.h) taken, both sides of every class boundary present."""
import os
import re

from ragged256_edges import (BF16_BATCHES, CTC_BATCHES, DW_TILE_MIN_M, ENC_EDGES, GEMM256_MIN_M, LDS, NO_SPLIT_BATCHES, ONLINE1,
                             ONLINE4, ONLINE16, RING_MIN_M, SPLIT64, TOKEN_EDGES, TR_BATCHES, TR_T, TR_U, attn_class, last_class,
                             utterance)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tensorflowasr_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_defaults_of_the_code():
    assert re.search(r'mi355_env\("MI355ASR_RING_MIN_M", %d\)' % RING_MIN_M, _src("weights.hip"))
    assert re.search(r'mi355_env\("MI355ASR_GEMM256_MIN_M", %d\)' % GEMM256_MIN_M, _src("bf16.hip"))
    assert re.search(r"if \(a\.T \* a\.B >= %d\)" % DW_TILE_MIN_M, _src("blocks.hip"))


def test_attn_class_restates_launch_h():
    """the three lines of attn64_class, as they stand in csrc/launch.h, and the restatement at every corner"""
    h = _src("launch.h")
    assert "if ((flags & ATTN64_F_SPLIT64) && tk > 32 && tk <= 288 && tq > 16) return ATTN64_SPLIT64;" in h
    assert "if ((flags & ATTN64_F_LDS) && tk > 16 && tk <= 272 && tq > 16) return ATTN64_LDS;" in h
    assert "return tk <= 16 ? ATTN64_ONLINE1 : tk <= 96 ? ATTN64_ONLINE4 : ATTN64_ONLINE16;" in h
    want = {(17, 16): ONLINE1, (17, 17): LDS, (17, 32): LDS, (17, 33): SPLIT64, (17, 288): SPLIT64, (17, 289): ONLINE16,
            (16, 33): ONLINE4, (16, 96): ONLINE4, (16, 97): ONLINE16, (16, 16): ONLINE1, (1, 600): ONLINE16}
    for (tq, tk), c in want.items():
        assert attn_class(tq, tk, True, True) == c, (tq, tk)
    assert [attn_class(17, tk, False, True) for tk in (33, 272, 273, 288)] == [LDS, LDS, ONLINE16, ONLINE16]
    assert [attn_class(17, tk, False, False) for tk in (16, 17, 96, 97)] == [ONLINE1, ONLINE4, ONLINE4, ONLINE16]
    assert last_class([(40, 40), (20, 20)], True, True) == LDS and last_class([(40, 40), (9, 9)], True, True) == ONLINE1


def test_ctc_batches_hold_every_class_and_boundary():
    rows = {k: Tmax * len(lens) for k, (Tmax, lens) in CTC_BATCHES.items()}
    assert rows == {"g-14x100": 1400, "g-5x289": 1445, "g-2x600": 1200, "r-6x289": 1734, "r-3x600": 1800, "t-30x100": 3000,
                    "t-12x600": 7200, "m-16x600": 9600}
    for name, (Tmax, lens) in CTC_BATCHES.items():
        M = rows[name]
        assert lens[0] == Tmax == max(lens) and min(lens) >= 1 and len(set(lens)) == len(lens), name
        assert Tmax > 16                                                 # ragged_rows_ok: more than 16 rows per utterance
        kind = name[0]
        assert kind in "grtm"
        assert (M < RING_MIN_M) == (kind == "g"), name
        assert (M < DW_TILE_MIN_M) == (kind in "gr"), name
        assert (M >= GEMM256_MIN_M) == (kind == "m"), name
    # every regime meets every class it can: below / from 1 500 rows, and with the tiled depthwise conv
    for kinds in ("g", "r", "tm"):
        lens = sorted({n for k, (_, ln) in CTC_BATCHES.items() if k[0] in kinds for n in ln})
        got = {attn_class(n, n, True, True) for n in lens}
        assert got >= {SPLIT64, ONLINE16}, (kinds, got)
    every = sorted({n for _, ln in CTC_BATCHES.values() for n in ln})
    assert {attn_class(n, n, True, True) for n in every} == {ONLINE1, LDS, SPLIT64, ONLINE16}
    for lo in (16, 32, 288):                                             # ONLINE1 | LDS | SPLIT64 | ONLINE16
        assert lo in every and lo + 1 in every
        assert attn_class(lo, lo, True, True) != attn_class(lo + 1, lo + 1, True, True)
    for kinds in ("g", "tm"):                                            # 16 | 17 and 32 | 33 on both depthwise-conv kernels
        lens = {n for k, (_, ln) in CTC_BATCHES.items() if k[0] in kinds for n in ln}
        assert {16, 17, 32, 33, 288, 289} <= lens, kinds
    # the MI355ASR_ATTN64_SPLIT=0 leg: LDS up to 272 keys, the online-softmax kernel from 273
    for name in NO_SPLIT_BATCHES:
        lens = CTC_BATCHES[name][1]
        assert 272 in lens and 273 in lens, name
        assert attn_class(272, 272, False, True) == LDS and attn_class(273, 273, False, True) == ONLINE16
    assert {271, 272, 273} <= set(CTC_BATCHES["t-12x600"][1])
    assert set(BF16_BATCHES) <= set(CTC_BATCHES) and {k[0] for k in BF16_BATCHES} == set("grtm")
    # the fill of t-30x100: 30 rows, the members first
    t30 = CTC_BATCHES["t-30x100"][1]
    assert len(t30) == 30 and t30[:4] == [100, 1, 2, 3] and {7, 8, 9, 15, 16, 17, 31, 32, 33, 96, 97, 99} <= set(t30[:26])
    assert t30[1:26] == sorted(t30[1:26])
    # the same utterance in every batch
    assert utterance(33).shape == (33, 256) and (utterance(33) == utterance(33)).all() and utterance(33).dtype.name == "float32"
    assert not (utterance(33)[:32] == utterance(32)).all()


def test_translator_batches_hold_every_class_and_boundary():
    assert TR_U == 48 and TR_T == 304 and max(TOKEN_EDGES) == TR_U and max(ENC_EDGES) == TR_T
    rows = {k: TR_U * len(p) for k, p in TR_BATCHES.items()}
    assert rows == {"x-26": 1248, "y-65": 3120}
    assert rows["x-26"] < RING_MIN_M <= 26 * TR_T and rows["x-26"] < DW_TILE_MIN_M        # token rows gemm16, key / value rows on the ring
    assert rows["y-65"] >= RING_MIN_M and rows["y-65"] >= DW_TILE_MIN_M
    for name, pairs in TR_BATCHES.items():
        assert len(set(pairs)) == len(pairs), name                       # no (tokens, frames) pair twice
        assert all(1 <= tl <= TR_U and 1 <= el <= TR_T for tl, el in pairs)
        got = {attn_class(tl, el, False, True) for tl, el in pairs}
        assert got == {ONLINE1, ONLINE4, ONLINE16, LDS}, (name, got)
    x = TR_BATCHES["x-26"]
    assert x[:13] == [(16, e) for e in ENC_EDGES] and x[13:] == [(17, e) for e in ENC_EDGES]
    for tl in (16, 17):
        frames = {el for t, el in x if t == tl}
        assert {16, 17, 96, 97, 272, 273} <= frames
    assert [attn_class(16, e, False, True) for e in (16, 17, 96, 97)] == [ONLINE1, ONLINE4, ONLINE4, ONLINE16]
    assert [attn_class(17, e, False, True) for e in (16, 17, 272, 273)] == [ONLINE1, LDS, LDS, ONLINE16]
    y = TR_BATCHES["y-65"]
    assert y[0] == (TR_U, TR_T) and {t for t, _ in y} == set(TOKEN_EDGES) and {e for _, e in y} == set(ENC_EDGES)
    assert y[1:] == [(TOKEN_EDGES[b % 10], ENC_EDGES[(3 * b) % 13]) for b in range(1, 65)]
