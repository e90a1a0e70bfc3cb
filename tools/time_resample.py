"""HIP-event timing of the device resampler (csrc/resample.hip) beside the host path it replaces.

    python tools/time_resample.py [--regions 7] [--iters 20] [--json out.json]

One-shot kernel: 64 x 10 s of 48 kHz int16 -> 16 kHz and of 8 kHz float32 -> 16 kHz, the inputs already on the device;
5 warm-up calls, then `regions` timed regions of `iters` back-to-back mi355asr_resample calls bracketed by events on the launch
stream; min / median / max milliseconds per call and the achieved GB/s (bytes read + bytes written over the median) against the
6.3 TB/s achievable HBM rate.  Stream step: 64 and 256 slots of 160 ms packets at 8 kHz, the packets on the device
(StreamResampler.step_device: one launch and the upload of the slot table).  Host: the same 64 utterances one after the other
through featurizers._resample (scipy.signal.resample_poly), wall clock."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_TBS = 6.3


def timed(call, stream, regions, iters):
    import torch
    for _ in range(5):
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
    from tensorflowasr_amd import featurizers
    from tensorflowasr_amd.resample import Resampler, StreamResampler, out_length
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    rows = []
    B, sec = 64, 10
    for rate, pcm in ((48000, True), (8000, False)):
        L = rate * sec
        xh = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
        if pcm:
            xh = (np.clip(xh, -1, 1) * 32767).astype(np.int16)
        rs = Resampler(rate, 16000)
        x = torch.from_numpy(xh).cuda()
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        lo, med, hi = timed(lambda: rs(x, lens), stream, a.regions, a.iters)
        O = out_length(L, rs.up, rs.down)
        nbytes = B * (L * xh.itemsize + O * 4)
        t0 = time.perf_counter()
        for b in range(B):
            featurizers._resample(xh[b].astype(np.float32) / 32768 if pcm else xh[b], rate, 16000)
        host_ms = (time.perf_counter() - t0) * 1e3
        # the device path a caller sees: upload of what the caller holds, the launch, until the output is complete
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs(xh, None)
        torch.cuda.synchronize()
        e2e_ms = (time.perf_counter() - t0) * 1e3
        r = dict(what="one-shot", rate=rate, dtype=str(xh.dtype), B=B, seconds=sec, taps=rs.taps, tile=rs.tile, ms_min=lo, ms_median=med,
                 ms_max=hi, bytes=nbytes, gbs_median=nbytes / (med * 1e-3) / 1e9, hbm_share=nbytes / (med * 1e-3) / 1e12 / HBM_TBS,
                 traffic_floor_ms=nbytes / (HBM_TBS * 1e12) * 1e3, host_ms=host_ms, device_with_upload_ms=e2e_ms)
        rows.append(r)
        print("%d x %d s %d Hz %s -> 16 kHz (K=%d): min %.4f  median %.4f  max %.4f ms/call  %.0f GB/s = %.0f%% of %.1f TB/s "
              "(traffic floor %.4f ms); with the upload %.2f ms; host resample_poly x %d: %.1f ms"
              % (B, sec, rate, xh.dtype, rs.taps, lo, med, hi, r["gbs_median"], 100 * r["hbm_share"], HBM_TBS, r["traffic_floor_ms"],
                 e2e_ms, B, host_ms))
        assert med < host_ms, "the device path is not faster than the host path"
    for n in (64, 256):
        P = 8000 * 160 // 1000
        srs = StreamResampler(n, 8000, 16000, P)
        slots = list(range(n))
        packets = (0.1 * torch.randn(n, P, generator=torch.Generator().manual_seed(1))).cuda()
        lo, med, hi = timed(lambda: srs.step_device(slots, packets), stream, a.regions, a.iters)
        t0 = time.perf_counter()
        for _ in range(a.iters):
            srs.step_device(slots, packets)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.iters
        r = dict(what="stream step", slots=n, packet=P, ms_min=lo, ms_median=med, ms_max=hi, wall_ms=wall)
        rows.append(r)
        print("stream step, %d slots x %d samples (160 ms at 8 kHz): min %.4f  median %.4f  max %.4f ms/step on the stream, "
              "%.4f ms wall with the host's packing" % (n, P, lo, med, hi, wall))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
