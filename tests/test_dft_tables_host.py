"""The host tables of the two-stage MFMA DFT (csrc/dft_tables.h: what stft.hip and stft_loss.hip upload) without a GPU:
tools/dft_tables_dump built under the address and undefined-behaviour sanitizers writes them, and every float32 is compared, bit for
bit, with a restatement of the definitions in the kernel files' header comments -- N = 32 x N2, the twiddles W_N^(k1 n2), the four
stage matrices in the fragment order of v_mfma_f32_16x16x4_f32's A operand, the periodic Hann window and its square."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, window length, window offset, scale of T4): stft.hip's two geometries (centred window, the inverse's 1 / N), then resolutions
# of stft_loss.hip (window at the start, the transpose carries no scale)
CASES = [(1024, 800, 112, 1 / 1024), (2048, 2048, 0, 1 / 2048), (1024, 600, 0, 1.0), (512, 250, 0, 1.0), (512, 7, 0, 1.0)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("dft_tables")
    exe = str(d / "dft_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "dft_tables_dump", "main.cpp"), "-o", exe])
    return d, exe


def cosm(a, b, M):
    return math.cos(2.0 * math.pi * ((a * b) % M) / M)


def sinm(a, b, M):
    return math.sin(2.0 * math.pi * ((a * b) % M) / M)


def pack_frag(T):
    """[M][K] float64 -> float32 in the order [M / 16][K / 4][64]: lane holds row 16 mt + (lane & 15), column 4 ks + (lane >> 4)"""
    M, K = T.shape
    mt, ks, lane = np.meshgrid(np.arange(M // 16), np.arange(K // 4), np.arange(64), indexing="ij")
    return T.astype(np.float32)[16 * mt + (lane & 15), 4 * ks + (lane >> 4)].ravel()


def expected(N, win, offset, scale):
    N2 = N // 32
    H = N2 // 2
    w = np.zeros(N, np.float64)
    for j in range(win):
        w[offset + j] = 0.5 - 0.5 * math.cos(2.0 * math.pi * j / win)
    twc = np.array([[cosm(k1, n2, N) for n2 in range(N2)] for k1 in range(32)])
    tws = np.array([[sinm(k1, n2, N) for n2 in range(N2)] for k1 in range(32)])
    c32 = np.array([[cosm(a, b, 32) for b in range(32)] for a in range(32)])
    s32 = np.array([[sinm(a, b, 32) for b in range(32)] for a in range(32)])
    c2 = np.array([[cosm(a, b, N2) for b in range(N2)] for a in range(N2)])
    s2 = np.array([[sinm(a, b, N2) for b in range(N2)] for a in range(N2)])
    T1 = np.vstack([c32, -s32])                                             # [64][32]: Re | Im of sum_n1 W32^(n1 k1) x
    T2 = np.block([[c2[:H], s2[:H]], [-s2[:H], c2[:H]]])                    # [N2][2 N2]: Re = C Bre + S Bim, Im = -S Bre + C Bim
    T3 = np.block([[c32, -s32], [s32, c32]])                                # [64][64]: Re = C Fre - S Fim, Im = S Fre + C Fim
    T4 = np.hstack([c2 * scale, -s2 * scale])                               # [N2][2 N2]: y = (C Bre - S Bim) scale
    return {"win": w.astype(np.float32), "wsq": (w * w).astype(np.float32), "twc": twc.astype(np.float32).ravel(),
            "tws": tws.astype(np.float32).ravel(), "T1": pack_frag(T1), "T2": pack_frag(T2), "T3": pack_frag(T3), "T4": pack_frag(T4)}


@pytest.mark.parametrize("N,win,offset,scale", CASES)
def test_tables_equal_their_definitions_bit_for_bit(dump, N, win, offset, scale):
    d, exe = dump
    out = str(d / ("t_%d_%d.bin" % (N, win)))
    r = subprocess.run([exe, str(N), str(win), str(offset), repr(float(scale)), out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    head = np.fromfile(out, np.uint64, 9)
    data = np.fromfile(out, np.float32, offset=72)
    want = expected(N, win, offset, scale)
    names = ["win", "wsq", "twc", "tws", "T1", "T2", "T3", "T4"]
    N2 = N // 32
    sizes = [N, N, 32 * N2, 32 * N2, 64 * 32, N2 * 2 * N2, 64 * 64, N2 * 2 * N2]
    assert [int(h) for h in head] == [sum(sizes[:i]) for i in range(9)] and len(data) == sum(sizes)
    for name, at, n in zip(names, head, sizes):
        got = data[int(at):int(at) + n]
        assert want[name].shape == got.shape, name
        differ = np.flatnonzero(got.view(np.uint32) != want[name].view(np.uint32))
        assert differ.size == 0, (name, int(differ[0]), float(got[differ[0]]), float(want[name][differ[0]]))
    # what a table served to the wrong user would show: the window's place and the scale of the last stage
    assert not want["win"][:offset].any() and not want["win"][offset + win:].any()
    assert data[int(head[7])] == np.float32(scale)                          # T4[0][0] = cos(0) scale, lane 0 of the first fragment
