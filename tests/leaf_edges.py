"""Case lists for tests/test_gpu_leaf_edges.py, and plain restatements of the index arithmetic of the LEAF frontend (csrc/leaf.hip,
run_mel in csrc/api.hip) and of the scratch carve of the add_wav_info branch (wavpick_floats / run_wavpick in csrc/api.hip).

LEAF.  The Gabor convolution kernels sum |conv|^2 times the Gaussian window into a fixed number of frame slots per tile of
positions -- 4 per 128-tile (fp32 kernel), 4 per wave of 64 positions and 7 per 512-tile (split-bf16 kernel) -- and
leaf_gather_kernel recomputes from the frame which tiles hold a partial sum for it.  `pooling_model(L, tile)` walks every
(position n, frame f) pair whose window weight is not zero, 0 <= n - (hop f - pl) <= 400, through both sides.  Integer division is
C's (towards zero) where an operand can be negative, as in the gather's h_lo.

Waveform branch.  `wavpick_accesses` lists every write into, and every GEMM read from, the six buffers run_wavpick carves out of the
wavpick_floats(...) scratch, with the capacity the carve gives each.

No torch, no GPU."""
import numpy as np

HOP, KTAPS = 160, 401
TILES = {128: 4, 512: 7}                    # positions per workgroup -> frame slots per tile (kLeafSplitTile / kLeafSplitSlots)
WAVE, WAVE_SLOTS = 64, 4                    # the split kernel: positions per wave, frame slots per wave
SWEEP_MAX = 2 * 2560 + 512                  # two periods of lcm(512, 160) and one tile


def cdiv(a, b):
    """C integer division (towards zero) of ints or integer arrays, b > 0"""
    return np.sign(a) * (np.abs(a) // b)


def same_pad(n, k, s):
    """api.hip same_pad: (out, before)"""
    o = -(-n // s)
    return o, max((o - 1) * s + k - n, 0) // 2


def leaf_geometry(L, tile):
    F, pl = same_pad(L, KTAPS, HOP)
    return dict(F=F, pl=pl, NH=-(-L // tile))


def first_frame(n0, pl):
    """fb / fbw / FB of leaf.hip: the first frame slot of the tile (or wave) whose first position is n0"""
    return (n0 + pl) // HOP - 2


def gather_range(f, pl, tile, nrel, NH):
    """leaf_gather_kernel: the tiles h_lo .. h_hi it visits for frame f"""
    h_lo = np.maximum(cdiv(HOP * (f + 3 - nrel) - pl, tile) - 1, 0)
    h_hi = np.minimum(cdiv(HOP * (f + 3) - pl, tile) + 1, NH - 1)
    return h_lo, h_hi


def window_pairs(L, F, pl):
    """every (n, f), n < L, f < F, with 0 <= n - (hop f - pl) <= 400, as two arrays; a position has at most three frames"""
    n = np.arange(L)
    ns, fs = [], []
    for k in range(3):
        f = (n + pl) // HOP - k
        ok = (f >= 0) & (f < F) & (n - (HOP * f - pl) <= KTAPS - 1)
        ns.append(n[ok]); fs.append(f[ok])
    assert not ((((n + pl) // HOP - 3) >= 0) & (n - (HOP * ((n + pl) // HOP - 3) - pl) <= KTAPS - 1)).any()
    return np.concatenate(ns), np.concatenate(fs)


def pooling_model(L, tile):
    """Walk every window pair of an utterance of L samples through the conv kernel's slot arithmetic and the gather's.
    Returns (problems, used): problems a list of strings (empty: the arithmetic is complete for this L), used a set of
    (kind, index, where) -- the slots that hold a non-zero weight -- with kind 'slot' (tile slot) or 'rel' (slot of a wave of
    the split kernel; of the tile for the 128-tile) and where one of 'interior' (any tile but the last), 'last' (the partial
    last tile, L not a multiple of the tile), 'first' (tile 0 where it is not the last) and 'h%5=k' (an interior tile of
    that index residue)."""
    nrel = TILES[tile]
    g = leaf_geometry(L, tile)
    F, pl, NH = g["F"], g["pl"], g["NH"]
    n, f = window_pairs(L, F, pl)
    problems, used = [], set()
    h = n // tile
    slot = f - first_frame(tile * h, pl)
    if ((slot < 0) | (slot >= nrel)).any():
        problems.append("L=%d tile=%d: a pair falls outside its tile's %d slots" % (L, tile, nrel))
    if tile == 512:
        # per wave: rel = f - fbw in [0, 4), and the epilogue maps (wave, rel) to tile slot rel + fbw - FB
        fbw = first_frame(WAVE * (n // WAVE), pl)
        rel = f - fbw
        if ((rel < 0) | (rel >= WAVE_SLOTS)).any():
            problems.append("L=%d: a pair falls outside its wave's %d slots" % (L, WAVE_SLOTS))
        if ((rel + fbw - first_frame(tile * h, pl)) != slot).any():
            problems.append("L=%d: wave slot and tile slot disagree" % L)
    else:
        rel = slot
    # the gather for f visits the pair's tile (its loop runs over distinct tiles: at most once) with this slot in range
    h_lo, h_hi = gather_range(f, pl, tile, nrel, NH)
    if ((h < h_lo) | (h > h_hi)).any():
        bad = np.flatnonzero((h < h_lo) | (h > h_hi))[0]
        problems.append("L=%d tile=%d: the gather for frame %d skips tile %d (visits %d .. %d)" % (L, tile, f[bad], h[bad], h_lo[bad], h_hi[bad]))
    # no slot is read that no tile wrote: every visited (tile, slot) lies in [0, NH) x [0, nrel) -- all of which every tile writes
    ff = np.arange(F)
    lo, hi = gather_range(ff, pl, tile, nrel, NH)
    if (lo < 0).any() or (hi > NH - 1).any():
        problems.append("L=%d tile=%d: the gather leaves the tiles 0 .. %d" % (L, tile, NH - 1))
    # ... and a tile in range whose slot for f is in range but holds no pair contributes an exact zero: nothing to check
    last = (h == NH - 1) & (L % tile != 0)
    interior = h < NH - 1
    groups = [("interior", interior), ("last", last), ("first", interior & (h == 0))]
    groups += [("h%%5=%d" % k, interior & (h % 5 == k)) for k in range(5)]     # tile h + pl mod hop has period 5 in h (both tiles)
    for where, m in groups:
        for s in np.unique(slot[m]):
            used.add(("slot", int(s), where))
        for r in np.unique(rel[m]):
            used.add(("rel", int(r), where))
    return problems, used


# ---- the GPU length list (tests/test_gpu_leaf_edges.py) ---------------------------------------------------------------------------
SHORT = [1, 2, 159, 160, 161, 200, 201, 400, 401, 402]                        # shorter than the window and its half
TILE_EDGES = [127, 128, 129, 511, 512, 513, 1023, 1024, 1025]
PAD_RESIDUES = [2560 + r for r in (0, 1, 79, 80, 81, 159)]
COVERAGE = [740, 2738]          # what the lists above lacked: slot 6 of the first 512-tile, and of an interior tile with h % 5 = 4
FRAME_COUNTS = [3040, 3200, 3360, 20320, 20480, 20481]                         # F = 19, 20, 21, 127, 128, 129
FRAME_COUNTS_DEFAULT_TERMS = [40960, 40961]                                    # F = 256, 257
assert [same_pad(L, KTAPS, HOP)[0] for L in FRAME_COUNTS + FRAME_COUNTS_DEFAULT_TERMS] == [19, 20, 21, 127, 128, 129, 256, 257]


def gpu_lengths(default_terms=False):
    return SHORT + TILE_EDGES + PAD_RESIDUES + COVERAGE + FRAME_COUNTS + (FRAME_COUNTS_DEFAULT_TERMS if default_terms else [])


def required_coverage():
    """{tile: the (kind, index, where) the GPU lengths are asked to exercise}: every slot of a 512-tile, every rel of a wave and of
    a 128-tile, each in an interior tile and in the partial last tile"""
    both = ("interior", "last")
    return {512: {("slot", s, w) for s in range(7) for w in both} | {("rel", r, w) for r in range(4) for w in both},
            128: {("rel", r, w) for r in range(4) for w in both}}


# What no length can exercise.  Slot s of tile h is frame f = (tile h + pl) / hop - 2 + s, and f <= F - 1 with
# hop (F - 1) = L - r (r = 1 .. hop samples in the last frame) needs tile h + pl < L - r + hop (3 - s).  In a partial last tile
# tile h > L - tile, so r + pl - tile < hop (3 - s); r + pl = r + (401 - r) / 2 lies in 201 .. 280, which rules out s = 3 at
# tile 128 (73 < 0) and s = 5, 6 at tile 512 (r + pl < 192, < 32): those frames lie behind the utterance's last one.
UNREACHABLE = {512: {("slot", 5, "last"), ("slot", 6, "last")}, 128: {("rel", 3, "last")}}


def coverage(lengths):
    """{tile: union of pooling_model(L, tile)'s used sets}, and the set of left pads"""
    used = {t: set() for t in TILES}
    for L in lengths:
        for t in TILES:
            used[t] |= pooling_model(L, t)[1]
    return used, {same_pad(L, KTAPS, HOP)[1] for L in lengths}


# ---- add_wav_info: the scratch carve -------------------------------------------------------------------------------------------
WAV_MIN_FRAMES = 3            # tf.pad(..., "REFLECT") by 2 needs at least 3 rows: the library refuses shorter inputs


def wav_stages(strides, dmodel):
    """[(cin, c, stride)] of the three Conv1D + residual-stack stages behind the separable conv"""
    out, cin = [], 32
    for i in range(1, 4):
        c = min(32 * (i + 1), dmodel)
        out.append((cin, c, strides[i]))
        cin = c
    return out


def wav_min_length(strides):
    """the shortest input the library accepts with add_wav_info on: ceil(L / prod(strides)) >= 3"""
    return (WAV_MIN_FRAMES - 1) * int(np.prod(strides)) + 1


def wavpick_floats(strides, dmodel, Bp, Lmax):
    T0 = -(-Lmax // strides[0])
    s1, t = 0, T0
    for _, c, st in wav_stages(strides, dmodel):
        t = -(-t // st)
        s1 = max(s1, (t + 8) * c)
    return Bp * ((T0 + 8) * 32 * 2 + 4 * s1) + 1024


def wavpick_accesses(strides, dmodel, Bp, L):
    """run_wavpick: ([(what, buffer, floats touched from the buffer's start, buffer capacity)], floats carved in all, final T).
    A GEMM reads row (b, t) of a padded copy as k * cin floats from b * Tpad * cin + t * stride * cin."""
    T0 = -(-L // strides[0])
    s1, t = 0, T0
    for _, c, st in wav_stages(strides, dmodel):
        t = -(-t // st)
        s1 = max(s1, (t + 8) * c)
    cap = dict(A=Bp * (T0 + 8) * 32, P=Bp * (T0 + 8) * 32, Y=Bp * s1, H=Bp * s1, G=Bp * s1, S=Bp * s1)
    acc = [("sepconv out", "A", Bp * T0 * 32)]

    def conv(src, Tpad, cin, k, stride, Tout, dst, cout, what):
        acc.append((what + " read", src, (Bp - 1) * Tpad * cin + (Tout - 1) * stride * cin + k * cin))
        acc.append((what + " write", dst, Bp * Tout * cout))

    Tc, cin = T0, 32
    for i, (_, c, st) in enumerate(wav_stages(strides, dmodel), 1):
        Tn, lo = same_pad(Tc, 3, st)
        hi = max((Tn - 1) * st + 3 - Tc, 0) - lo
        acc.append(("stage %d zero pad" % i, "P", Bp * (Tc + lo + hi) * cin))
        conv("P", Tc + lo + hi, cin, 3, st, Tn, "Y", c, "stage %d conv3" % i)
        acc.append(("stage %d reflect pad" % i, "P", Bp * (Tn + 4) * c))
        conv("P", Tn + 4, c, 5, 1, Tn, "H", c, "stage %d conv5" % i)
        acc.append(("stage %d LeakyReLU" % i, "G", Bp * Tn * c))
        conv("Y", Tn, c, 1, 1, Tn, "S", c, "stage %d shortcut" % i)
        conv("G", Tn, c, 1, 1, Tn, "H", c, "stage %d conv1" % i)
        Tc, cin = Tn, c
    acc.append(("final zero pad", "P", Bp * (Tc + 6) * cin))
    acc.append(("final conv read", "P", (Bp - 1) * (Tc + 6) * cin + (Tc - 1) * cin + 7 * cin))
    return [(w, b, n, cap[b]) for w, b, n in acc], sum(cap.values()), Tc


# ---- add_wav_info: the GPU cases -----------------------------------------------------------------------------------------------
WAV_RESIDUES = (0, 1, 7, 8, 9, 39, 40, 41, 159, 160, 161, 639)                 # of the [8, 5, 4, 4] config; x 2 for [16, 5, 4, 4]
WAV_BATCH_EDGES = [(5, 3), (3, 7), (17, 3), (2, 17)]                           # (B, T): 16-row GEMM tiles over several utterances


def wav_lengths(hopred):
    """3 frames' worth + every residue that flips a parity of the four nested SAME pads, scaled to the config's first stride"""
    k = hopred // 640
    return [hopred * 3 + k * r for r in WAV_RESIDUES]
