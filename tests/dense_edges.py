"""Tables for tests/test_gpu_dense_edges.py: the plain (not ragged) dmodel-256 / 512 dense layers at every row count where a launcher
changes kernel family or a grid gains a partial row tile, the ring class head over the class count, and the subsampling conv
of dmodel 256 / 512 at every padding parity.  No GPU here: tests/test_dense_edges_host.py asserts these tables.

A dense layer of M = B * T rows runs on one of three families (launch_gemm16 in csrc/api.hip, use_gemm16 in csrc/block_path.hip,
ring_packs_wanted / ring_min_rows in csrc/weights.hip): the fp32 chain kernels (dmodel 256 on a handle without slab rings:
set_expected_rows below RING_MIN_M, or MI355ASR_GEMM_RING=0), the per-wave gemm16 kernels (below RING_MIN_M rows; dmodel 512
always when there are no rings) and gemm_ring_kernel (csrc/gemm_ring.hip) from RING_MIN_M rows on, whose workgroups hold 128 or
256 rows.  The constants are the code's defaults, not measurements."""
import numpy as np

from helpers import co

RING_MIN_M = 1500                 # MI355ASR_RING_MIN_M (csrc/weights.hip, ring_min_rows)
RING_ROWS = (128, 256)            # rows per workgroup of gemm_ring_kernel with one / two row tiles per wave
RING_CHUNK = 128                  # classes per column chunk of the ring class head
MAX_EXCUSED = 0.005               # of a case's frames: the oracle's own top-2 margin is within 1e-3 (the arg-max cannot be held there)
MARGIN = 1e-3
F32, BF16X3, F16X2, BF16 = 0, 1, 2, 3                     # include/mi355asr.h: MI355ASR_SCHEME_*
DENSE = ("ffn", "qkv", "attn_out", "pw1_glu", "conv_tail")          # the categories of a block's dense layers
STACK = ("ctc_project", "ctc_head")

DMODELS = (256, 512)
HEADS = {256: 4, 512: 8}          # x 64: ConformerM / ConformerL
V_DENSE = 60

# ---- A. the row counts -------------------------------------------------------------------------------------------------------
# n = 0 (project + head, row-wise, B = 1): the 16-row tile, every 128-row workgroup edge up to three workgroups, the family
# crossover, and the 128- / 256-row edges above it (1 536 = 12 x 128 = 6 x 256, 1 792 = 14 x 128 = 7 x 256, 2 048 = 16 x 128)
N0_M = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1499, 1500, 1501, 1535, 1536, 1537, 1791, 1792, 1793, 2047, 2048,
        2049)
# n = 1 (every epilogue): M -> (B, T), T >= 17 and as short as the divisors of M allow (the oracle's attention is O(T^2))
N1_SHAPES = {129: (3, 43), 257: (1, 257), 1499: (1, 1499), 1500: (20, 75), 1501: (19, 79), 1537: (29, 53), 2049: (3, 683)}
CHAIN_MAX_M = 385                 # the set_expected_rows(300) leg: the fp32 chains at M <= 385
EXPECTED_ROWS = 300
RING_OFF_M = (1500, 2049)         # MI355ASR_GEMM_RING=0
FORCED_M = (129, 257, 385)        # the forced launch shapes: two, three and four 128-row workgroups with one row in the last
FORCED_N1 = {129: (3, 43), 257: (1, 257), 385: (5, 77)}
BF16_M = (257, 1501, 2049)

FORCED_SHAPES = {                 # name -> environment, on top of MI355ASR_RING_MIN_M=1
    "rt1": {"MI355ASR_RING_RT": "1"},
    "rt2": {"MI355ASR_RING_RT": "2"},
    "slots2": {"MI355ASR_RING_SLOTS": "2"},
    "rt1_cpw2": {"MI355ASR_RING_RT": "1", "MI355ASR_RING_CPW": "2"},
    "rt2_cpw8": {"MI355ASR_RING_RT": "2", "MI355ASR_RING_CPW": "8"},
}
FORCE_RING = {"MI355ASR_RING_MIN_M": "1"}

# ---- B. the ring class head ----------------------------------------------------------------------------------------------------
HEAD_V = (5, 127, 128, 129, 201, 1332)
HEAD_M = (257, 1501)
HEAD_RANGES_V = 1332
HEAD_RANGES = (1, 2, 3, 4)

# ---- C. the subsampling conv -----------------------------------------------------------------------------------------------------
SUBCONV_B = 3
SUBCONV_F = tuple(range(1, 9)) + tuple(range(25, 29)) + tuple(range(49, 53)) + tuple(range(101, 105))
SUBCONV_LEGS = {                  # name -> environment (MI355ASR_SUBCONV_RT is read by the two-term kernels only)
    "terms22": {"MI355ASR_SUBCONV_TERMS": "22"},
    "terms22_rt1": {"MI355ASR_SUBCONV_TERMS": "22", "MI355ASR_SUBCONV_RT": "1"},
    "terms22_rt2": {"MI355ASR_SUBCONV_TERMS": "22", "MI355ASR_SUBCONV_RT": "2"},
}
WAVE_CASES = {256: ((17, 3), (33, 8)), 512: ((17, 10), (33, 1))}       # dmodel -> ((T, combo of ragged_edges.COMBOS), ...)

# every leg that runs in a process of its own: name -> environment
LEGS = {"ring_off": {"MI355ASR_GEMM_RING": "0"}}
LEGS.update({"forced_" + k: dict(FORCE_RING, **v) for k, v in FORCED_SHAPES.items()})
LEGS.update({"ranges%d" % n: dict(FORCE_RING, MI355ASR_RING_HEAD_RANGES=str(n)) for n in HEAD_RANGES})
LEGS.update({"subconv_" + k: v for k, v in SUBCONV_LEGS.items()})

# a seed that left more than MAX_EXCUSED of a case's frames undecided is replaced here (the cap stays): case key -> seed bump
RESEED = {(256, 0, 129, 60): 1, (256, 1, 129, 60): 1, (512, 0, 129, 60): 1, (512, 1, 129, 60): 1, (256, 0, 1501, 1332): 5}


def subconv_geometry(F):
    """(T1, T2, rows of SAME padding in front of conv1, of conv2): kernel 3, stride 2, as same_pad in csrc/api.hip"""
    T1 = -(-F // 2)
    T2 = -(-T1 // 2)
    return T1, T2, max((T1 - 1) * 2 + 3 - F, 0) // 2, max((T2 - 1) * 2 + 3 - T1, 0) // 2


def cfg_for(d, n):
    return dict(co.CONFORMER_S, dmodel=d, head_size=64, num_heads=HEADS[d], ctcdecoder_num_blocks=n, ctcdecoder_kernel_size=32)


def weights(d, n, V):
    """co.ctc_decoder_weights with the two biases it leaves at zero drawn as well: a bias read at the wrong column must show"""
    w = co.ctc_decoder_weights(cfg_for(d, n), V, seed=7 * d + 100 * n + V)
    rng = np.random.default_rng(V + d)
    w["project/bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    w["fully_connected/bias"] = (0.1 * rng.standard_normal(V)).astype(np.float32)
    return w


def case_input(d, n, M, V=V_DENSE):
    """the input [B, T, d] of a case, seeded by the case: the same in every leg and every process"""
    B, T = (1, M) if n == 0 else (N1_SHAPES.get(M) or FORCED_N1[M])
    seed = 100000 * n + 17 * d + M + 1000003 * V + 7919 * RESEED.get((d, n, M, V), 0)
    return np.random.default_rng(seed).standard_normal((B, T, d)).astype(np.float32)


def undecided_share(ref64):
    """the share of frames whose float64 logits leave the arg-max open: top-2 margin at most MARGIN"""
    top = np.sort(ref64.reshape(-1, ref64.shape[-1]), axis=-1)
    return float(((top[:, -1] - top[:, -2]) <= MARGIN).mean())


def dense_cases():
    """every (d, n, M) of section A that is compared with the un-rounded oracle"""
    out = []
    for d in DMODELS:
        out += [(d, 0, M) for M in N0_M] + [(d, 1, M) for M in N1_SHAPES]
        out += [(d, n, M) for n in (0, 1) for M in FORCED_M if (d, n, M) not in out]
    return out


def head_cases():
    return [(256, 0, M, V) for V in HEAD_V for M in HEAD_M]


def subconv_mel(F):
    return (-80 * np.random.default_rng(F).random((SUBCONV_B, F, 80))).astype(np.float32)
