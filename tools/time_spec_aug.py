"""HIP-event timing of spec_aug and the time stretch (csrc/stft.hip) beside what a user would write without them.

    python tools/time_spec_aug.py [--regions 5] [--iters 5] [--json out.json]

The benchmark batch, 64 x 10 s at 16 kHz, the inputs already on the device.  SpecAug at the reference's window 10 and ratio 0.5
(500 centres per row, drawn once and uploaded by every call); its two launches one by one through the plain pair (forward to
memory, inverse from memory: the route that writes and reads the 263 MB spectrum); TimeStretch at rate 0.9 and 1.2 and its three
stages one by one; torch.stft / torch.istft with the same window on the same device as the yardstick of the pair.  3 warm-up calls,
then `regions` timed regions of `iters` back-to-back calls bracketed by events on the launch stream: min / median / max
milliseconds per call.  The DFT stages' FLOP are counted as issued on the matrix pipe (2 M N K per stage product)."""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32_MATRIX_TFLOPS = 157.3


def timed(call, stream, regions, iters):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    per = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            call()
        e1.record(stream)
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / iters)
    per.sort()
    return per[0], float(np.median(per)), per[-1]


def frame_flop(n2):
    """matrix-pipe FLOP of one frame, forward and inverse: the four stage products of csrc/stft.hip"""
    fwd = 2 * 64 * n2 * 32 + 2 * n2 * 32 * 2 * n2
    inv = 2 * 64 * n2 * 64 + 2 * n2 * 32 * 2 * n2
    return fwd, inv


def main():
    import torch
    from tensorflowasr_amd.augment import SpecAug, TimeStretch
    from tensorflowasr_amd.stft import STFT
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    B, L = 64, 160000
    rows = []

    def report(what, t, **more):
        rows.append(dict(what=what, ms_min=t[0], ms_median=t[1], ms_max=t[2], **more))
        print("%-44s min %.4f  median %.4f  max %.4f ms/call  %s"
              % (what, t[0], t[1], t[2], "  ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in more.items())))

    x = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).cuda()
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    aug = SpecAug(window=10, ratio=0.5)
    F = aug.frames(L)
    random.seed(0)
    centres = [aug.draw(F) for _ in range(B)]
    fwd, inv = frame_flop(32)
    t = timed(lambda: aug(x, lens, centres=centres), stream, a.regions, a.iters)
    flop = float(B * F * (fwd + inv))
    report("SpecAug 64 x 10 s, 500 centres per row", t, frames=B * F, gflop=flop / 1e9, tflops_median=flop / (t[1] * 1e-3) / 1e12,
           share_of_f32_matrix_peak=flop / (t[1] * 1e-3) / 1e12 / F32_MATRIX_TFLOPS, workspace_mb=B * F * 800 * 4 / 1e6)
    # the library call alone: the centres already on the device, workspace and output allocated once
    import ctypes
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    table = torch.from_numpy(np.stack(centres).astype(np.int32)).cuda()
    counts = torch.full((B,), table.shape[1], dtype=torch.int32, device="cuda")
    wb = ctypes.c_size_t()
    _lib.check(lib.mi355asr_spec_aug_workspace_bytes(B, L, ctypes.byref(wb)))
    ws = torch.empty(wb.value // 4, dtype=torch.float32, device="cuda")
    yb = torch.empty((B, L), dtype=torch.float32, device="cuda")
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    bare = lambda: _lib.check(lib.mi355asr_spec_aug(p(x), 0, p(lens), B, L, p(table), table.shape[1], p(counts), 10, p(yb), L, p(ws),
                                                    wb.value, ctypes.c_void_p(stream.cuda_stream)))
    tb = timed(bare, stream, a.regions, a.iters)
    report("  mi355asr_spec_aug alone", tb, tflops_median=flop / (tb[1] * 1e-3) / 1e12,
           share_of_f32_matrix_peak=flop / (tb[1] * 1e-3) / 1e12 / F32_MATRIX_TFLOPS, workspace_gbs_median=2 * B * F * 800 * 4 / 1e9 / (tb[1] * 1e-3))
    st = STFT(1024, 800, 160)
    tf = timed(lambda: st.forward(x, lens), stream, a.regions, a.iters)
    S, frames = st.forward(x, lens)
    spectrum_mb = S.numel() * 8 / 1e6
    report("stft 1024 / 800 / 160 to memory", tf, spectrum_mb=spectrum_mb, gbs_median=spectrum_mb / 1e3 / (tf[1] * 1e-3))
    ti = timed(lambda: st.inverse(S, frames, out_pad=L), stream, a.regions, a.iters)
    report("istft 1024 / 800 / 160 from memory", ti, pair_over_spec_aug_alone=(tf[1] + ti[1]) / tb[1])
    win = torch.hann_window(800, periodic=True, device="cuda")

    def torch_pair():
        D = torch.stft(x, 1024, hop_length=160, win_length=800, window=win, center=True, pad_mode="reflect", return_complex=True)
        return torch.istft(D, 1024, hop_length=160, win_length=800, window=win, center=True)
    tt = timed(torch_pair, stream, a.regions, a.iters)
    y, _ = st.inverse(S, frames, out_pad=L)
    yt = torch_pair()
    n = min(y.shape[1], yt.shape[1])
    report("torch.stft + torch.istft, same batch", tt, pair_over_torch=(tf[1] + ti[1]) / tt[1],
           pair_max_err=float((y[:, :n] - x[:, :n]).abs().max()), torch_max_err=float((yt[:, :n] - x[:, :n]).abs().max()))

    ts = TimeStretch()
    fwd2, inv2 = frame_flop(64)
    for rate in (0.9, 1.2):
        t = timed(lambda: ts(x, lens, rate), stream, a.regions, a.iters)
        F2 = 1 + L // 512
        T2 = len(np.arange(0, F2, rate))
        flop = float(B * (F2 * fwd2 + T2 * inv2))
        report("TimeStretch 64 x 10 s, rate %.1f" % rate, t, frames_in=B * F2, frames_out=B * T2, out_samples=int(round(L / rate)),
               gflop=flop / 1e9, tflops_median=flop / (t[1] * 1e-3) / 1e12)
    st2 = ts.stft
    tf2 = timed(lambda: st2.forward(x, lens), stream, a.regions, a.iters)
    report("  stft 2048 / 2048 / 512 to memory", tf2)
    S2, fr2 = st2.forward(x, lens)
    ti2 = timed(lambda: st2.inverse(S2, fr2, out_pad=L), stream, a.regions, a.iters)
    report("  istft 2048 / 2048 / 512 from memory", ti2)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
