"""HIP-event timing of the band-limited resampler (csrc/sinc_resample.hip) and of the pitch augmentation built on it.

    python tools/time_pitch.py [--regions 5] [--iters 5] [--json out.json]      (default: profiles/pitch_mi355x.json)

The benchmark batch, 64 x 10 s at 16 kHz, inputs already on the device: mi355asr_sinc_resample alone (table, workspace and output
allocated once) at the ratios 0.84, 1.0 and 1.19, with the table in LDS (table_mode 0, what the library uses) and through the
caches (table_mode 1), then augment.Pitch end to end (the gather of the zones, the time stretch -- STFT, phase vocoder, inverse
STFT --, the resampler writing into a copy of the batch) with a step per row, and TimeStretch alone on the same zones.  3 warm-up
calls, then `regions` timed regions of `iters` back-to-back calls bracketed by events on the launch stream: min / median / max
milliseconds per call.  The bytes are what the launch has to move: every input sample read once and every output written once,
fp32; the 128 KiB table stays on the chip.  The taps are the fp32 FMA pairs (weight, product) per output."""
import argparse
import ctypes
import json
import os
import sys

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
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.augment import Pitch, TimeStretch
    from tensorflowasr_amd.resample import SincResampler, sinc_out_length
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pitch_mi355x.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    B, L = 64, 160000
    rows = []

    def report(what, t, **more):
        rows.append(dict(what=what, ms_min=t[0], ms_median=t[1], ms_max=t[2], **more))
        print("%-58s min %.4f  median %.4f  max %.4f ms/call  %s"
              % (what, t[0], t[1], t[2], "  ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in more.items())))

    x = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).cuda()
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    hp = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    wb = ctypes.c_size_t()
    _lib.check(lib.mi355asr_sinc_workspace_bytes(B, ctypes.byref(wb)))
    ws = torch.empty(wb.value // 8, dtype=torch.float64, device="cuda")
    rs = SincResampler()
    tab = rs.table()
    lens = np.full(B, L, np.int64)
    for ratio in (0.84, 1.0, 1.19):
        O = sinc_out_length(L, ratio)
        y = torch.empty((B, O), dtype=torch.float32, device="cuda")
        r = np.full(B, ratio, np.float64)
        ol = np.full(B, O, np.int64)
        wing = rs.wing(ratio)
        for mode, name in ((0, "table in LDS"), (1, "table through the caches")):
            bare = lambda: _lib.check(lib.mi355asr_sinc_resample(p(x), B, L, hp(r), hp(lens), hp(ol), None, None, p(tab), mode, p(y), O, p(ws),
                                                                 wb.value, ctypes.c_void_p(stream.cuda_stream)))
            t = timed(bare, stream, a.regions, a.iters)
            mb = B * (L + O) * 4 / 1e6
            taps = B * O * 2.0 * wing
            report("mi355asr_sinc_resample 64 x 10 s, ratio %.2f, %s" % (ratio, name), t, wing=wing, traffic_mb=mb,
                   gbs_median=mb / 1e3 / (t[1] * 1e-3), share_of_hbm_peak=mb / 1e6 / (t[1] * 1e-3) / HBM_TBS,
                   gtaps_per_s_median=taps / 1e9 / (t[1] * 1e-3))
    steps = rng.uniform(-3, 3, B)
    ln = torch.full((B,), L, dtype=torch.int32, device="cuda")
    pitch = Pitch("(0.2,0.8)")
    t = timed(lambda: pitch(x, ln, steps=steps), stream, a.regions, a.iters)
    report("Pitch 64 x 10 s, zone (0.2, 0.8), a step per row", t)
    t = timed(lambda: pitch(x, ln, steps=steps, quantise=True), stream, a.regions, a.iters)
    report("Pitch 64 x 10 s, the same, quantised", t)
    s, e = pitch.span(L)
    z = x[:, s:e].contiguous()
    zl = torch.full((B,), e - s, dtype=torch.int32, device="cuda")
    rates = np.array([Pitch.rate(v) for v in steps])
    ts = TimeStretch()
    t = timed(lambda: ts(z, zl, rates), stream, a.regions, a.iters)
    report("  TimeStretch alone on the same zones and rates", t)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
