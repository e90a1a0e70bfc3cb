"""HIP-event timing of the recursive filters and of the hz / masking augmentations (csrc/iir.hip) beside SciPy on the same host.

    python tools/time_iir.py [--regions 5] [--iters 5] [--json out.json]      (default: profiles/iir_mi355x.json)

The benchmark batch, 64 x 10 s at 16 kHz, inputs, noise and draws already on the device: Hz with one start for all rows (a shared
filter) and with a start per row, the library call alone (sections on the device, workspace and output allocated once), its
mode 0 (sosfilt), and Mask.  3 warm-up calls, then `regions` timed regions of `iters` back-to-back calls bracketed by events on
the launch stream: min / median / max milliseconds per call.  Every mi355asr_sos_ragged call reads its sections back once, so the
call waits for the stream: the event time includes that wait.  scipy.signal.sosfiltfilt runs the same batch on the host once
(one thread).  The bytes are what the passes move: per section and direction one float64 read for the zero run's first launch
and a read and a write for every true run."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


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


def main():
    import torch
    from scipy import signal
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.augment import Hz, Mask
    from tensorflowasr_amd.iir import SOSFilter
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "iir_mi355x.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    B, L, S, PAD = 64, 160000, 3, 21
    C = SOSFilter.CHUNK
    rows = []

    def report(what, t, **more):
        rows.append(dict(what=what, ms_min=t[0], ms_median=t[1], ms_max=t[2], **more))
        print("%-52s min %.4f  median %.4f  max %.4f ms/call  %s"
              % (what, t[0], t[1], t[2], "  ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in more.items())))

    xh = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    u = torch.rand((B, L), dtype=torch.float64, device="cuda")
    starts = np.clip(rng.random(B), 0.01, 0.699)
    N = L + 2 * PAD
    # float64 traffic of mode 1: per direction one read (the first zero run) and S reads and writes (the true runs); the input
    # of the first true run is float32 and the last write is float32; plus the noise
    mb = B * (2 * (1 + 2 * S) * N * 8 - 2 * 4 * N + L * 8) / 1e6
    hz = Hz()
    for what, st in (("Hz 64 x 10 s, one start for all rows", 0.35), ("Hz 64 x 10 s, a start per row", starts)):
        t = timed(lambda: hz(x, lens, starts=st, noise=u, quantise=True), stream, a.regions, a.iters)
        report(what, t, chunk=C, chunks_per_row=-(-N // C), launches=4 * S + 2, traffic_mb=mb, gbs_median=mb / 1e3 / (t[1] * 1e-3),
               share_of_hbm_peak=mb / 1e6 / (t[1] * 1e-3) / HBM_TBS)
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    wb = ctypes.c_size_t()
    _lib.check(lib.mi355asr_sos_workspace_bytes(B, L, S, 1, ctypes.byref(wb)))
    ws = torch.empty(wb.value // 8 + 1, dtype=torch.float64, device="cuda")
    y = torch.empty((B, L), dtype=torch.float32, device="cuda")
    sos = torch.from_numpy(np.stack([Hz.sections(s) for s in starts])).cuda()
    for mode, what in ((1, "  mi355asr_sos_ragged alone, mode 1, per-row filters"), (0, "  mi355asr_sos_ragged alone, mode 0 (sosfilt)")):
        bare = lambda: _lib.check(lib.mi355asr_sos_ragged(p(x), 0, p(lens), B, L, p(sos), S, 0, mode, PAD, None, None, p(u) if mode else None, L,
                                                          0.001, mode, p(y), L, p(ws), wb.value, ctypes.c_void_p(stream.cuda_stream)))
        t = timed(bare, stream, a.regions, a.iters)
        m = mb if mode else B * ((1 + 2 * S) * L * 8 - 2 * 4 * L) / 1e6
        report(what, t, launches=(4 * S + 2) if mode else 2 * S + 1, workspace_mb=wb.value / 1e6, traffic_mb=m, gbs_median=m / 1e3 / (t[1] * 1e-3))
    for noise in (True, False):
        m = Mask("(0.1,0.9)", 0.3, noise)
        t = timed(lambda: m(x, lens, u=u, quantise=True), stream, a.regions, a.iters)
        mm = B * L * (4 + 4 + 0.8 * 8) / 1e6
        report("Mask 64 x 10 s, mask_with_noise=%s" % noise, t, traffic_mb=mm, gbs_median=mm / 1e3 / (t[1] * 1e-3))
    # the host: SciPy on the same batch, one thread, once (the shared filter; per-row filters cost the same per row)
    xd = xh.astype(np.float64)
    sh = Hz.sections(0.35)
    t0 = time.perf_counter()
    yh = signal.sosfiltfilt(sh, xd, axis=-1, padlen=PAD)
    t1 = time.perf_counter()
    b_, a_ = signal.butter(3, [0.35, 0.65], "bandstop")
    signal.filtfilt(b_, a_, xd, axis=-1)
    t2 = time.perf_counter()
    yd = hz(x, lens, starts=0.35, noise=False)[0].cpu().numpy()
    report("scipy.signal.sosfiltfilt, same batch, this host", (1e3 * (t1 - t0),) * 3, filtfilt_ba_ms=1e3 * (t2 - t1),
           max_abs_diff_to_device=float(np.abs(yd - yh).max()))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
