"""The device resampler where a random-input bound cannot see: impulse trains whose every output is ONE tap of the filter (so the
test is exact at any K and names every tap), the sizes at which its 64-bit arithmetic and its tile loop matter, and streams far from
position 0.  The reference is scipy.signal.resample_poly on the float64 input throughout; rows and streams are compared with the
one-shot call on the row alone bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.signal import resample_poly

from resample_ref import (LARGE_K, SMALL_K, all_taps, batch_positions, check_impulse_rows, impulse_row, impulse_values, plan,
                          row_positions, taps_and_gain)
from tensorflowasr_amd.resample import out_length, stream_emitted

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def resampler(up, down):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from tensorflowasr_amd.resample import Resampler
    rs = Resampler(down * 25, up * 25)
    p = plan(up, down)
    assert (rs.taps, rs.tile) == (p["taps"], p["tile"])
    return rs


def host(y, n):
    return y.cpu().numpy()[:, :n]


@pytest.mark.parametrize("up,down", SMALL_K)
def test_small_k_every_input_position_is_an_impulse_in_some_row(up, down):
    """K + 1 rows, row b with impulses at b, b + (K + 1), ...: every sample of [0, L) (more than two tiles and a ragged end, sample 0
    and sample L - 1 included) is an impulse in exactly one row, so the kernel's whole linear map on that range is pinned"""
    rs = resampler(up, down)
    L, positions = batch_positions(up, down)
    assert sorted(np.concatenate(positions).tolist()) == list(range(L)) and len(positions) == rs.taps + 1
    assert out_length(L, up, down) > 2 * rs.tile and out_length(L, up, down) % rs.tile
    rng = np.random.default_rng(1000 * up + down)
    x = np.stack([impulse_row(L, pos, impulse_values(rng, len(pos))) for pos in positions])
    y, n = rs(x)
    visited = check_impulse_rows(up, down, x, positions, host(y, y.shape[1]), "float32")
    assert np.array_equal(visited, all_taps(up, down))


@functools.lru_cache(maxsize=None)
def long_row(up, down, pcm):
    L, pos = row_positions(up, down)
    rng = np.random.default_rng(77 * up + down + pcm)
    x = impulse_row(L, pos, impulse_values(rng, len(pos), pcm), np.int16 if pcm else np.float32)
    return L, pos, x


@pytest.mark.parametrize("up,down", LARGE_K)
def test_large_k_one_row_visits_every_tap(up, down):
    """one row, impulses K + 1 or more apart at a spacing prime to `down`: at K = 12 801 the random-input bound is five times the
    centre tap, here every output is one tap, exactly"""
    rs = resampler(up, down)
    L, pos, x = long_row(up, down, False)
    assert pos[1] - pos[0] >= rs.taps + 1 and np.gcd(pos[1] - pos[0], down) == 1 and len(pos) >= down
    assert out_length(L, up, down) > 2 * rs.tile
    y, n = rs(x)
    visited = check_impulse_rows(up, down, x[None], [pos], host(y, y.shape[1]), "float32")
    assert np.array_equal(visited, all_taps(up, down))


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (1, 20)])
def test_int16_impulses(up, down):
    """the same trains as PCM: +-2^e, e in [0, 14], and -32768; x / 32768 is exact, so the criterion is the same"""
    rs = resampler(up, down)
    if (up, down) in SMALL_K:
        L, positions = batch_positions(up, down)
        rng = np.random.default_rng(up + down)
        x = np.stack([impulse_row(L, pos, impulse_values(rng, len(pos), True), np.int16) for pos in positions])
    else:
        L, pos, x = long_row(up, down, True)
        x, positions = x[None], [pos]
    assert x.dtype == np.int16 and (x == -32768).any() and (x == 16384).any()
    y, n = rs(x)
    visited = check_impulse_rows(up, down, x.astype(np.float64) / 32768, positions, host(y, y.shape[1]), "int16")
    assert np.array_equal(visited, all_taps(up, down))


# ---- sizes ---------------------------------------------------------------------------------------------------------------------

def test_several_tiles_per_workgroup():
    """2/1, 64 rows of 32768 - 7 b samples: 64 tiles a row, 4096 in all, two per workgroup -- the tile loop, its re-staging barrier
    and a workgroup whose second tile lies past the row's end.  Then four times the width: whole workgroups on zero tiles."""
    up, down = 2, 1
    rs = resampler(up, down)
    B = 64
    lens = [32768 - 7 * b for b in range(B)]
    assert -(-out_length(lens[0], up, down) // rs.tile) * B // 2048 == 2
    rng = np.random.default_rng(64)
    x = rng.standard_normal((B, lens[0])).astype(np.float32)
    y, n = rs(x, lens)
    y, n = y.cpu().numpy(), n.cpu().numpy()
    K, A = taps_and_gain(up, down)
    worst = 0.0
    for b, L in enumerate(lens):
        O = out_length(L, up, down)
        assert int(n[b]) == O and not y[b, O:].any(), b
        ref = resample_poly(x[b, :L].astype(np.float64), up, down)
        tol = (K + 2) * 2.0 ** -23 * A * float(np.abs(x[b, :L]).max())
        err = float(np.abs(y[b, :O] - ref).max())
        worst = max(worst, err / tol)
        assert err <= tol, (b, err, tol)
        alone, _ = rs(x[b, :L])
        assert np.array_equal(alone.cpu().numpy()[0], y[b, :O]), b
    print("2/1 B=64, two tiles per workgroup: largest error %.3f of its bound" % worst)
    wide = 4 * out_length(lens[0], up, down)
    assert min(-(-wide // rs.tile) * B // 2048, 16) == 8
    y4, n4 = rs(x, lens, out_pad=wide)
    y4 = y4.cpu().numpy()
    assert y4.shape == (B, wide) and np.array_equal(n4.cpu().numpy(), n)
    assert np.array_equal(y4[:, :y.shape[1]], y) and not y4[:, y.shape[1]:].any()


def test_k_down_above_2_to_31():
    """640/441, two rows of 3.4 M samples: the last outputs have k down of about 2.17e9.  Row 0 is an impulse train (exact), row 1
    random within the derived bound."""
    up, down = 640, 441
    rs = resampler(up, down)
    L = 3_400_000
    O = out_length(L, up, down)
    assert (O - 1) * down > 2 ** 31 + 10 ** 7
    K, A = taps_and_gain(up, down)
    pos = np.arange(0, L, K + 1, dtype=np.int64)
    assert K + 1 == 22
    rng = np.random.default_rng(2171)
    x = np.stack([impulse_row(L, pos, impulse_values(rng, len(pos))), rng.standard_normal(L).astype(np.float32)])
    y, n = rs(x)
    y = y.cpu().numpy()
    assert n.cpu().numpy().tolist() == [O, O]
    check_impulse_rows(up, down, x[:1], [pos], y[:1], "long row", with_e32=False)
    ref = resample_poly(x[1].astype(np.float64), up, down)
    tol = (K + 2) * 2.0 ** -23 * A * float(np.abs(x[1]).max())
    err = np.abs(y[1] - ref)
    print("640/441, 3.4 M samples: largest error %.3f of its bound, %.3f in the last tile" % (err.max() / tol, err[-rs.tile:].max() / tol))
    assert err.max() <= tol


def live_rows_against_rows_alone(rs, x, lens, live):
    """y of the whole batch: the live rows equal the rows alone bit for bit, every other row is zero"""
    import torch
    y, n = rs(x, lens)
    n = n.cpu().numpy()
    for a in range(0, x.shape[0], 64):
        hi, lo = y[a:a + 64].amax(dim=1).cpu().numpy(), y[a:a + 64].amin(dim=1).cpu().numpy()
        for i in range(len(hi)):
            if a + i in live:
                assert hi[i] > 0.1 and lo[i] < -0.1, a + i
            else:
                assert hi[i] == 0 and lo[i] == 0 and n[a + i] == 0, a + i
    for b in live:
        O = out_length(lens[b], rs.up, rs.down)
        assert n[b] == O
        alone, _ = rs(x[b:b + 1, :lens[b]])
        assert torch.equal(alone[0, :O], y[b, :O]), b
        assert not y[b, O:].any(), b
        del alone
    del y


def test_row_offsets_above_2_to_31_elements_on_the_input_side():
    """1/20, int16, 2049 rows of 2^20 + 8 samples: row 2048 starts 2^31 + 16384 elements in.  Rows 0, 1024 and 2048 are live, every
    other row has length 0 and is never read (it is left uninitialised)."""
    import torch
    rs = resampler(1, 20)
    B, Lpad = 2049, 2 ** 20 + 8
    live = {0: Lpad, 1024: 777_777, 2048: Lpad}
    assert (B - 1) * Lpad > 2 ** 31
    x = torch.empty((B, Lpad), dtype=torch.int16, device="cuda")
    try:
        g = torch.Generator(device="cuda").manual_seed(20)
        for b, n in live.items():
            x[b, :n] = torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        lens = [live.get(b, 0) for b in range(B)]
        live_rows_against_rows_alone(rs, x, lens, live)
    finally:
        rs._keep = None
        del x
        torch.cuda.empty_cache()


def test_row_offsets_above_2_to_31_elements_on_the_output_side():
    """2/1, int16, 1100 rows of 2^20 samples: y is 1100 x 2^21 floats (9.2 GB), row 1099 starts 2.3e9 elements in, and a workgroup
    takes 16 tiles"""
    import torch
    rs = resampler(2, 1)
    B, Lpad = 1100, 2 ** 20
    live = {0: Lpad, 550: 777_777, 1099: Lpad}
    assert (B - 1) * out_length(Lpad, 2, 1) > 2 ** 31 and -(-out_length(Lpad, 2, 1) // rs.tile) * B // 2048 >= 16
    assert B * Lpad * 2 + B * out_length(Lpad, 2, 1) * 4 + 3 * Lpad * 10 < 12e9
    x = torch.empty((B, Lpad), dtype=torch.int16, device="cuda")
    try:
        g = torch.Generator(device="cuda").manual_seed(21)
        for b, n in live.items():
            x[b, :n] = torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        lens = [live.get(b, 0) for b in range(B)]
        live_rows_against_rows_alone(rs, x, lens, live)
    finally:
        rs._keep = None
        del x
        torch.cuda.empty_cache()


def test_the_largest_batch_and_the_refusal_of_one_more():
    from tensorflowasr_amd._lib import Mi355AsrError
    rs = resampler(2, 1)
    rng = np.random.default_rng(65535)
    x = rng.standard_normal((65536, 8)).astype(np.float32)
    y, n = rs(x[:65535])
    y = y.cpu().numpy()
    assert y.shape == (65535, 16) and (n.cpu().numpy() == 16).all()
    for b in (0, 1, 65534):
        assert np.array_equal(rs(x[b])[0].cpu().numpy()[0], y[b]) and np.abs(y[b]).max() > 0, b
    with pytest.raises(Mi355AsrError, match="B <= 65535.*got 65536"):
        rs(x)


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (1, 20)])
def test_out_pad_narrower_and_wider(up, down):
    """narrower than the longest row's output (the n_store < n_valid path offline_stt_batch uses): out_len clamps and the columns are
    the full call's first out_pad columns; wider: zeros.  Widths that are and are not multiples of 4 (16-byte and scalar stores)."""
    rs = resampler(up, down)
    tile = rs.tile
    L = (2 * tile + 300) * down // up
    lens = [L, (tile + 11) * down // up, 5, 0, L - 1]
    rng = np.random.default_rng(3 * up + down)
    x = rng.standard_normal((len(lens), L)).astype(np.float32)
    full, n_full = rs(x, lens)
    full, n_full = full.cpu().numpy(), n_full.cpu().numpy()
    O = full.shape[1]
    assert O == out_length(L, up, down) > 2 * tile
    widths = [517, tile + 37, tile + 40, 2 * tile, O - 1, O + 1, O + 3 - O % 4 + 2, O + 8 - O % 4, O + 2 * tile + 4 - O % 4]
    assert any(w < O and w % 4 for w in widths) and any(w < O and w % 4 == 0 for w in widths)
    assert any(w > O and w % 4 for w in widths) and any(w > O and w % 4 == 0 for w in widths)
    for w in widths:
        y, n = rs(x, lens, out_pad=w)
        y = y.cpu().numpy()
        assert y.shape == (len(lens), w)
        assert np.array_equal(n.cpu().numpy(), np.minimum(n_full, w)), w
        m = min(w, O)
        assert np.array_equal(y[:, :m], full[:, :m]), w
        assert not y[:, m:].any(), w


# ---- streams -------------------------------------------------------------------------------------------------------------------

def stream_resampler(n, up, down, max_packet):
    from tensorflowasr_amd.resample import StreamResampler
    return StreamResampler(n, down * 25, up * 25, max_packet)


@pytest.mark.parametrize("up,down", [(2, 1), (1, 3), (160, 441), (1, 20)])
def test_a_stream_at_2_to_50_equals_the_stream_near_0(up, down):
    """slot 0 starts at 0 and takes m' down zeros (m' = ceil((half + 1) / (up down)): from there on its emitted count is not clamped
    at 0); slot 1 is fresh with its position set to M down, M = 2^50 // down.  Both positions are multiples of `down`, so the same
    packets give the same counts and phases, and, the rings being zero, the same samples -- while the ring positions differ.
    A ring position that is wrong by the same amount at every step would go unseen (the ring has no origin), so slots 2 and 3 start
    just below 2^31 and just below 5 x 2^32 and cross them while the packets arrive: a position cut to 32 bits jumps there."""
    from tensorflowasr_amd._lib import Mi355AsrError
    max_packet = 2000
    srs = stream_resampler(4, up, down, max_packet)
    half = 10 * max(up, down)
    start_a = -(-(half + 1) // (up * down)) * down
    start_b = (2 ** 50 // down) * down
    cap = srs.taps - 1 + max_packet
    assert start_b > 2 ** 49 and start_a % cap != start_b % cap
    fed = 0
    while fed < start_a:
        p = min(max_packet, start_a - fed)
        srs.step([0], [np.zeros(p, np.float32)])
        fed += p
    assert srs.pos == [start_a, 0, 0, 0] and stream_emitted(start_a, up, down) > 0
    starts = [start_a, start_b, (2 ** 31 - 3000) // down * down, (5 * 2 ** 32 - 9000) // down * down]
    assert 2 ** 32 % cap and 2 ** 31 % cap
    srs.pos[1:] = starts[1:]
    rng = np.random.default_rng(50 + up + down)
    total = 0
    for p in [1, 7, 160, 1280, 2000] * 3 + [1999, 3, 2000, 2000]:
        pk = rng.standard_normal(p).astype(np.float32)
        new = srs.step([0, 1, 2, 3], [pk] * 4)
        want = stream_emitted(start_a + total + p, up, down) - stream_emitted(start_a + total, up, down)
        total += p
        for s in (1, 2, 3):
            assert len(new[0]) == len(new[s]) == want, (s, total, p)
            assert np.array_equal(new[0], new[s]), (s, total, p)
        assert srs.pos == [v + total for v in starts]
    assert total > 2 * cap and starts[2] + total > 2 ** 31 + cap and starts[3] + total > 5 * 2 ** 32 + cap      # every ring wrapped
    tails = srs.flush([0, 1, 2, 3])
    for s in (1, 2, 3):
        assert len(tails[0]) == len(tails[s]) > 0 and np.array_equal(tails[0], tails[s]) and np.abs(tails[0]).max() > 0
    srs.pos[1] = 2 ** 51 + 1
    with pytest.raises(Mi355AsrError, match="position %d" % (2 ** 51 + 1)):
        srs.step([1], [np.zeros(4, np.float32)])
    srs.pos[1] = 2 ** 51
    with pytest.raises(Mi355AsrError, match="position %d" % 2 ** 51):
        srs.flush([1])


@pytest.mark.parametrize("up,down,max_packet", [(1, 3, 8000), (160, 441, 8000), (1, 20, 48000), (3, 61, 48000)])
def test_steps_of_several_output_tiles(up, down, max_packet):
    """a full packet emits more than two tiles, on down-samplers and on the unstaged kernel; packets of 1 and 0 samples between"""
    rs = resampler(up, down)
    srs = stream_resampler(3, up, down, max_packet)
    assert stream_emitted(10 ** 6 + max_packet, up, down) - stream_emitted(10 ** 6, up, down) > 2 * rs.tile
    sizes = [max_packet, 1, 0, max_packet, max_packet, 0, 1, 7, max_packet, 0]
    rng = np.random.default_rng(max_packet + up)
    audio = rng.standard_normal(sum(sizes)).astype(np.float32)
    got, pos = [], 0
    for p in sizes:
        new = srs.step([2], [audio[pos:pos + p]])[2]
        assert len(new) == stream_emitted(pos + p, up, down) - stream_emitted(pos, up, down)
        got.append(new)
        pos += p
    got.append(srs.flush([2])[2])
    one, n = rs(audio)
    one = one.cpu().numpy()[0, :int(n[0])]
    mine = np.concatenate(got)
    assert mine.shape == one.shape and np.array_equal(mine, one)


@pytest.mark.parametrize("up,down", [(2, 1), (160, 441), (1, 20)])
def test_device_packets_with_lengths_empty_packets_and_early_flushes(up, down):
    import torch
    rs = resampler(up, down)
    K = rs.taps
    srs = stream_resampler(4, up, down, 1500)
    rng = np.random.default_rng(11 * up + down)
    slots = [3, 1, 0]
    steps = [[1500, 0, 700], [0, 0, 0], [1, 1500, 0], [1200, 333, 1500], [0, 0, 0], [77, 0, 1]]
    audio = {s: rng.standard_normal(sum(st[i] for st in steps)).astype(np.float32) for i, s in enumerate(slots)}
    pos = {s: 0 for s in slots}
    got = {s: [] for s in slots}
    for lens in steps:
        pk = torch.full((len(slots), 1500), float("nan"), device="cuda")            # past a row's length: never read
        for i, s in enumerate(slots):
            pk[i, :lens[i]] = torch.from_numpy(audio[s][pos[s]:pos[s] + lens[i]]).cuda()
        y, counts = srs.step_device(slots, pk, lengths=lens)
        assert y.is_cuda and y.shape == (len(slots), srs.out_cap)
        yh = y.cpu().numpy()
        for i, s in enumerate(slots):
            assert counts[i] == stream_emitted(pos[s] + lens[i], up, down) - stream_emitted(pos[s], up, down), (s, lens)
            got[s].append(yh[i, :counts[i]].copy())
            pos[s] += lens[i]
        if not any(lens):
            assert not counts.any()
    tails = srs.flush(slots)
    for s in slots:
        one, n = rs(audio[s])
        mine = np.concatenate(got[s] + [tails[s]])
        assert not np.isnan(mine).any()
        assert np.array_equal(mine, one.cpu().numpy()[0, :int(n[0])]), s
    # a flush at position 0 gives nothing; at position 1 and K - 2 the whole output of those samples
    assert all(len(v) == 0 for v in srs.flush([0, 1, 2, 3]).values())
    for n_in in (1, K - 2):
        x = rng.standard_normal(n_in).astype(np.float32)
        first = srs.step([2], [x])[2]
        nothing = srs.step([2], [x[:0]])[2]
        tail = srs.flush([2])[2]
        one, n = rs(x)
        assert len(first) == stream_emitted(n_in, up, down) and len(nothing) == 0
        assert len(first) + len(tail) == out_length(n_in, up, down) == int(n[0])
        assert np.array_equal(np.concatenate([first, tail]), one.cpu().numpy()[0, :int(n[0])]), n_in
    with pytest.raises(ValueError, match="lengths"):
        srs.step_device([0, 1], torch.zeros((2, 8), device="cuda"), lengths=[8, 9])


def test_refusals_of_the_stream_entry_points_launch_nothing():
    import torch
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    up, down, n_streams, max_packet = 1, 3, 4, 1280
    srs = stream_resampler(n_streams, up, down, max_packet)
    srs.step([0, 1, 2, 3], [np.ones(100, np.float32)] * 4)          # rings that are not all zero
    torch.cuda.synchronize()
    state0 = srs.state.clone()
    y = torch.full((n_streams, srs.out_cap), 7.0, device="cuda")
    x = torch.ones((n_streams, max_packet + 8), device="cuda")
    # a table that is 16-byte aligned, and the same table 4 bytes further on
    buf = torch.zeros(srs.table.numel() + 8, device="cuda")
    off = (-buf.data_ptr() // 4) % 4
    good = buf[off:off + srs.table.numel()].copy_(srs.table)
    assert good.data_ptr() % 16 == 0
    bad = buf[off + 1:off + 1 + srs.table.numel()]
    slots = np.arange(n_streams, dtype=np.int32)
    pos = np.full(n_streams, 100, np.int64)
    n_out = np.full(n_streams, -5, np.int32)
    P = ctypes.c_void_p

    def step(msg, rc=-1, counted=0, **kw):
        """one call; `counted` leading entries of n_out may be written (the launcher fills the table slot by slot and refuses at the
        first bad slot), every other entry must be untouched"""
        n_out[:] = -5
        a = dict(up=up, down=down, n_streams=n_streams, max_packet=max_packet, filt=good.data_ptr(), slots=slots, n_in=[64] * n_streams,
                 n=n_streams, flush=0, x=x.data_ptr(), Ppad=max_packet + 8, out_cap=srs.out_cap, ws_bytes=srs.ws.numel())
        a.update(kw)
        nin = None if a["n_in"] is None else np.ascontiguousarray(a["n_in"], np.int32)
        got = lib.mi355asr_resample_streams_step(
            P(srs.state.data_ptr()), a["up"], a["down"], a["n_streams"], a["max_packet"], P(a["filt"]), a["slots"].ctypes.data_as(P),
            pos.ctypes.data_as(P), None if nin is None else nin.ctypes.data_as(P), a["n"], a["flush"], None if a["x"] is None else P(a["x"]),
            a["Ppad"], P(y.data_ptr()), a["out_cap"], n_out.ctypes.data_as(P), P(srs.ws.data_ptr()), a["ws_bytes"], None)
        err = lib.mi355asr_last_error().decode()
        assert got == rc and msg in err, (got, err)
        if rc:
            assert (n_out[counted:] == -5).all(), (msg, n_out)

    step("out_cap = %d < %d" % (srs.out_cap - 1, srs.out_cap), out_cap=srs.out_cap - 1)
    step("workspace too small: %d bytes" % (n_streams * 32 - 1), rc=-4, ws_bytes=n_streams * 32 - 1)
    step("need 1 <= n <= n_streams (got 5)", n=n_streams + 1, slots=np.arange(n_streams + 1, dtype=np.int32))
    step("need 1 <= n <= n_streams (got 0)", n=0)
    step("packet of 64 samples (max_packet 1280, row pitch 63)", Ppad=63)
    step("packet of 1281 samples (max_packet 1280, row pitch 1288)", n_in=[1281] * n_streams)
    step("max_packet = %d x up = 1 does not fit the step's 32-bit arithmetic" % 2 ** 30, max_packet=2 ** 30)
    step("misaligned filter table or state", filt=bad.data_ptr())
    step("a step needs packets and their lengths", x=None)
    step("a step needs packets and their lengths", n_in=None)
    step("slot 1 is named twice in one step", counted=2, slots=np.array([0, 1, 1, 2], np.int32))
    step("slot 4 out of range 0 .. 3", counted=2, slots=np.array([0, 1, 4, 2], np.int32))
    sb, wb, oc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    assert lib.mi355asr_resample_streams_bytes(640, 441, 4, 2 ** 21, ctypes.byref(sb), ctypes.byref(wb), ctypes.byref(oc)) == -1
    assert "max_packet = %d x up = 640 does not fit" % 2 ** 21 in lib.mi355asr_last_error().decode()
    assert lib.mi355asr_resample_streams_bytes(640, 441, 0, 1280, ctypes.byref(sb), ctypes.byref(wb), ctypes.byref(oc)) == -1
    assert "n_streams = 0, max_packet = 1280" in lib.mi355asr_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(srs.state, state0) and bool((y == 7.0).all())
    # and the same arguments without a fault are a step
    step("", rc=0)
    torch.cuda.synchronize()
    assert not torch.equal(srs.state, state0) and (n_out == stream_emitted(164, up, down) - stream_emitted(100, up, down)).all()
