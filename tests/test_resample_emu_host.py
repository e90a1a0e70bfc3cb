"""csrc/resample.hip run as a host program (tools/resample_host_emu: 256 threads per workgroup, LDS as an exact-size heap block)
under the address and undefined-behaviour sanitizers: the kernels' own index arithmetic, staging, FMA chains and the launchers'
stream tables, without a GPU.  Parity with scipy inside the derived bound, rows against rows alone with NaN past every length, int16
against float32, misaligned rows, and a stream against the one-shot call bit for bit -- for a staged down-sampler, a staged
up-sampler with many phases and a ratio that takes the unstaged path."""
import os
import subprocess

import numpy as np
import pytest
from scipy.signal import resample_poly

from resample_ref import taps_and_gain
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


def plan(up, down):
    """mi355asr_resample_plan, restated (test_resample_host.py pins the library's values to the same rules)"""
    K = -(-(20 * max(up, down) + 1) // up)
    unit = 4 * up
    return dict(taps=K, stride=K | 1, table_floats=(up * (K | 1) + 3) & ~3, tile=unit * -(-1024 // unit))


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
