"""csrc/resample.hip run as a host program (tools/resample_host_emu: 256 threads per workgroup, LDS as an exact-size heap block)
under the address and undefined-behaviour sanitizers: the kernels' own index arithmetic, staging, FMA chains and the launchers'
stream tables, without a GPU.  Parity with scipy inside the derived bound, rows against rows alone with NaN past every length, int16
against float32, misaligned rows, and a stream against the one-shot call bit for bit -- for a staged down-sampler, a staged
up-sampler with many phases and a ratio that takes the unstaged path.  Then what pins single taps and the launchers' 64-bit table
arithmetic: impulse trains (every output is one tap of the filter, exactly) up to K = 12 801, parity at the staged / unstaged boundary,
at unstaged ratios with several phases and at 640/1, and a stream placed at 2^50 against the same stream near 0."""
import os
import subprocess

import numpy as np
import pytest
from scipy.signal import resample_poly

from resample_ref import all_taps, check_impulse_rows, impulse_row, impulse_values, plan, row_positions, taps_and_gain
from tensorflowasr_amd import resample as R
from tensorflowasr_amd.resample import out_length

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_emu")
    src = open(os.path.join(ROOT, "tensorflowasr_amd", "csrc", "resample.hip")).read()
    a, b = '#include "model.h"', "extern __shared__ __attribute__((aligned(16))) float lds[];"
    assert src.count(a) == 1 and src.count(b) == 2
    (d / "resample_emu.cpp").write_text(src.replace(a, '#include "shim.h"').replace(b, "float* lds = g_lds;"))
    exe = str(d / "emu")
    here = os.path.join(ROOT, "tools", "resample_host_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-pthread", "-I" + here, "-I" + os.path.join(ROOT, "include"), "-I" + str(d),
                           '-DRESAMPLE_SOURCE="resample_emu.cpp"', os.path.join(here, "main.cpp"), "-o", exe])
    return d, exe


def run(emu, *args):
    d, exe = emu
    r = subprocess.run([exe] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def oneshot(emu, up, down, x, lens, misaligned=False):
    d = emu[0]
    x = np.ascontiguousarray(x)
    B, L = x.shape
    O = max(1, out_length(L, up, down))
    x.tofile(str(d / "x.bin"))
    np.asarray(lens, np.int32).tofile(str(d / "l.bin"))
    run(emu, "oneshot", up, down, "t.bin", "x.bin", "i" if x.dtype == np.int16 else "f", B, L, O, "l.bin", "y.bin",
        *(["m"] if misaligned else []))
    return np.fromfile(str(d / "y.bin"), np.float32).reshape(B, O)


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (1, 20)])
def test_kernel_source_on_the_host(emu, up, down):
    d = emu[0]
    p = plan(up, down)
    R._phase_table(up, down, p).tofile(str(d / "t.bin"))
    K, A = taps_and_gain(up, down)
    over_a_tile = (p["tile"] + 1) * down // up + 1
    lens = [0, 1, K - 1, 1501, over_a_tile]
    rng = np.random.default_rng(up + down)
    x = rng.standard_normal((len(lens), max(lens))).astype(np.float32)
    poisoned = x.copy()
    for b, n in enumerate(lens):
        poisoned[b, n:] = np.nan
    y = oneshot(emu, up, down, poisoned, lens)
    assert not np.isnan(y).any()
    for b, n in enumerate(lens):
        ol = out_length(n, up, down)
        assert not y[b, ol:].any()
        if n:
            ref = resample_poly(x[b, :n].astype(np.float64), up, down)
            assert np.abs(y[b, :ol] - ref).max() <= (K + 2) * 2.0 ** -23 * A * np.abs(x[b, :n]).max(), b
            assert np.array_equal(oneshot(emu, up, down, x[b:b + 1, :n], [n])[0, :ol], y[b, :ol]), b
    pcm = rng.integers(-32768, 32768, (2, 1501)).astype(np.int16)
    yi = oneshot(emu, up, down, pcm, [1501, K + 8])
    assert np.array_equal(yi, oneshot(emu, up, down, pcm.astype(np.float32) / 32768, [1501, K + 8]))
    assert np.array_equal(yi, oneshot(emu, up, down, pcm, [1501, K + 8], misaligned=True))
    sizes = [1, 7, 160, 1280, 2000, 1, 1, 7, 333]
    xs = rng.standard_normal(sum(sizes)).astype(np.float32)
    xs.tofile(str(d / "xs.bin"))
    np.asarray(sizes, np.int32).tofile(str(d / "s.bin"))
    run(emu, "stream", up, down, "t.bin", "xs.bin", 2000, "s.bin", "ys.bin")
    ys = np.fromfile(str(d / "ys.bin"), np.float32)
    one = oneshot(emu, up, down, xs[None], [len(xs)])[0, :out_length(len(xs), up, down)]
    assert ys.shape == one.shape and np.array_equal(ys, one)


def table(emu, up, down):
    R._phase_table(up, down, plan(up, down)).tofile(str(emu[0] / "t.bin"))


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (1, 20), (3, 61), (1, 640)])
def test_impulse_train_on_the_host(emu, up, down):
    """one row of impulses K + 1 or more apart that visits every tap: each output is the fp32 tap times +-2^e, or exactly 0"""
    table(emu, up, down)
    L, pos = row_positions(up, down)
    x = impulse_row(L, pos, impulse_values(np.random.default_rng(up + 7 * down), len(pos)))
    y = oneshot(emu, up, down, x[None], [L])
    visited = check_impulse_rows(up, down, x[None], [pos], y, "host emulation", with_e32=False)
    assert np.array_equal(visited, all_taps(up, down))


@pytest.mark.parametrize("up,down", [(1, 18), (1, 19), (3, 61), (101, 640), (640, 1)])
def test_parity_at_ratios_beyond_the_shipped_rates_on_the_host(emu, up, down):
    """1/18 is the last staged ratio (80 720 of 81 920 bytes: an index one past the span would leave the block), 1/19 the first
    unstaged one; 3/61 and 101/640 are unstaged with several phases; 640/1 is the limit"""
    table(emu, up, down)
    K, A = taps_and_gain(up, down)
    lens = [(plan(up, down)["tile"] + 9) * down // up + 1, K - 1, 1]
    rng = np.random.default_rng(31 * up + down)
    x = rng.standard_normal((len(lens), max(lens))).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    y = oneshot(emu, up, down, x, lens)
    assert not np.isnan(y).any()
    for b, n in enumerate(lens):
        ol = out_length(n, up, down)
        ref = resample_poly(x[b, :n].astype(np.float64), up, down)
        assert not y[b, ol:].any()
        assert np.abs(y[b, :ol] - ref).max() <= (K + 2) * 2.0 ** -23 * A * np.abs(x[b, :n]).max(), b


@pytest.mark.parametrize("up,down", [(1, 3), (1, 20)])
def test_a_stream_placed_at_2_to_50_equals_the_stream_near_0(emu, up, down):
    """the launcher's table (ring position, first output's sample and phase) from a 64-bit position: a fresh slot at M down,
    M = 2^50 // down, emits what a stream that took m' down zeros from position 0 emits for the same packets and flush.  The ring
    has no origin, so a ring position that is wrong by the same amount at every step goes unseen: two more streams start just below
    2^31 and just below 5 x 2^32 and cross them while the packets arrive, where a position cut to 32 bits jumps."""
    d = emu[0]
    table(emu, up, down)
    half = 10 * max(up, down)
    start_a = -(-(half + 1) // (up * down)) * down
    start_b = (2 ** 50 // down) * down
    max_packet = 2000
    cap = plan(up, down)["taps"] - 1 + max_packet
    assert start_a % cap != start_b % cap and 2 ** 31 % cap and 2 ** 32 % cap
    sizes = [1, 7, 160, 1280, 2000, 1, 1999, 333]
    rng = np.random.default_rng(up + down)
    xs = rng.standard_normal(sum(sizes)).astype(np.float32)
    np.concatenate([np.zeros(start_a, np.float32), xs]).tofile(str(d / "xa.bin"))
    np.asarray([start_a] + sizes, np.int32).tofile(str(d / "sa.bin"))
    xs.tofile(str(d / "xb.bin"))
    np.asarray(sizes, np.int32).tofile(str(d / "sb.bin"))
    run(emu, "stream", up, down, "t.bin", "xa.bin", max_packet, "sa.bin", "ya.bin")
    ya = np.fromfile(str(d / "ya.bin"), np.float32)
    skip = R.stream_emitted(start_a, up, down)
    assert skip > 0 and not ya[:skip].any()
    for start in (start_b, (2 ** 31 - 3000) // down * down, (5 * 2 ** 32 - 4000) // down * down):
        assert start % down == 0
        run(emu, "stream", up, down, "t.bin", "xb.bin", max_packet, "sb.bin", "yb.bin", start)
        yb = np.fromfile(str(d / "yb.bin"), np.float32)
        assert len(yb) == out_length(start_a + len(xs), up, down) - skip and np.array_equal(ya[skip:], yb) and np.abs(yb).max() > 0.1, start
