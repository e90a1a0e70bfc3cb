"""Batches for tests/test_gpu_ragged256_edges.py: ragged calls at dmodel 256 with 64-dim heads (the streaming configuration's global
CTC decoder and Translator) whose lengths sit ON every boundary of the per-utterance attention classes, in every regime of the
dense layers and of the depthwise conv.  No GPU here: tests/test_ragged256_host.py asserts these tables.

A dense layer of M = B * Tmax rows runs one gemm16 launch below RING_MIN_M rows, the slab ring of gemm_ring.hip from there on, and
in the bf16 mode gemm256_bf16_kernel from GEMM256_MIN_M rows; the ragged depthwise conv is dwconv_kernel<32, 8> below
DW_TILE_MIN_M rows and dwconv_tile_kernel<32, 128> from there on.  The constants are the code's defaults, not measurements."""
import numpy as np

from ragged_edges import edge

RING_MIN_M = 1500          # MI355ASR_RING_MIN_M (csrc/weights.hip, ring_min_rows)
DW_TILE_MIN_M = 2048       # launch_dwconv (csrc/blocks.hip): B * T from which the LDS-tiled kernel runs
GEMM256_MIN_M = 8192       # MI355ASR_GEMM256_MIN_M (csrc/bf16.hip)

ONLINE1, ONLINE4, ONLINE16, LDS, SPLIT64 = "ONLINE1", "ONLINE4", "ONLINE16", "LDS", "SPLIT64"
LAUNCH_ORDER = [SPLIT64, LDS, ONLINE1, ONLINE4, ONLINE16]          # launch_attention_ragged64 (csrc/blocks.hip)


def attn_class(tq, tk, split64, lds):
    """attn64_class of csrc/launch.h, restated: the attention kernel an utterance of tq queries and tk keys takes at head size 64.
    split64: ATTN64_F_SPLIT64 (the operand bounds are known and MI355ASR_ATTN64_SPLIT is on: self-attention); lds: ATTN64_F_LDS"""
    if split64 and 32 < tk <= 288 and tq > 16:
        return SPLIT64
    if lds and 16 < tk <= 272 and tq > 16:
        return LDS
    return ONLINE1 if tk <= 16 else ONLINE4 if tk <= 96 else ONLINE16


def last_class(pairs, split64, lds):
    """the class of the last attention launch of a ragged call over these (tq, tk) pairs"""
    need = {attn_class(tq, tk, split64, lds) for tq, tk in pairs}
    return [c for c in LAUNCH_ORDER if c in need][-1]


def utterance(n):
    """n frames of N(0, 1) in float32, seeded by n: the same utterance in every batch, one oracle result per length"""
    return np.random.default_rng(n).standard_normal((n, 256)).astype(np.float32)


def _t30():
    """Tmax first, then edge(100) with the neighbours of 8 and of 96, then seeded lengths that are none of these (what
    ragged_edges.with_fill does, over the lengths this batch does not hold yet) up to 30 rows"""
    members = [100] + sorted((set(edge(100)) | {7, 8, 9, 96, 97}) - {100})
    rest = sorted(set(range(1, 101)) - set(members))
    fill = np.random.default_rng(100).permutation(rest)[:30 - len(members)]
    return members + [int(t) for t in fill]


_T12 = [600, 599, 513, 512, 511, 289, 288, 287, 273, 272, 271, 257]

# name -> (Tmax, [lengths]); row 0 is Tmax.  g-: gemm16 kernels, dwconv_kernel<32, 8>; r-: ring kernels, dwconv_kernel;
# t-: ring kernels, dwconv_tile_kernel; m-: at or above GEMM256_MIN_M (the bf16 mode's rows-resident kernel)
CTC_BATCHES = {
    "g-14x100": (100, [100, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 96, 97]),
    "g-5x289": (289, [289, 288, 273, 272, 257]),
    "g-2x600": (600, [600, 513]),
    "r-6x289": (289, [289, 256, 255, 65, 64, 63]),
    "r-3x600": (600, [600, 512, 511]),
    "t-30x100": (100, _t30()),
    "t-12x600": (600, list(_T12)),
    "m-16x600": (600, _T12 + [256, 255, 129, 128]),
}
BF16_BATCHES = ["g-14x100", "r-6x289", "t-12x600", "m-16x600"]
NO_SPLIT_BATCHES = ["g-5x289", "t-12x600"]                      # the MI355ASR_ATTN64_SPLIT=0 leg


# ---- the Translator: U = 48 tokens, T = 304 frames ------------------------------------------------------------------------
TR_U, TR_T = 48, 304
TOKEN_EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48]
ENC_EDGES = [1, 16, 17, 32, 33, 96, 97, 256, 257, 272, 273, 289, 304]


def _x26():
    return [(16, e) for e in ENC_EDGES] + [(17, e) for e in ENC_EDGES]


def _y65():
    # 10 and 13 are coprime and 3 is coprime to 13: 65 rows are 65 different pairs (row 0 replaced by the full row)
    pairs = [(TOKEN_EDGES[b % 10], ENC_EDGES[(3 * b) % 13]) for b in range(65)]
    pairs[0] = (TR_U, TR_T)
    return pairs


# name -> [(token length, encoder length)]
TR_BATCHES = {"x-26": _x26(), "y-65": _y65()}
