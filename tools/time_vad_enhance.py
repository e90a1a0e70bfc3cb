"""HIP-event timing of mi355asr_vad_enhance (vad.hip, enhance variant): 60 x 60 s (one hour of 16 kHz audio) and
1 x 10 s, scores and enhanced 8 kHz frames in one launch.

    python tools/time_vad_enhance.py [--regions 7] [--iters 20]

Per shape: 5 warm-up calls, then `regions` timed regions of `iters` back-to-back calls each, bracketed by events on
the launch stream; prints min / median / max milliseconds per call, the achieved rate against the fp32 matrix roof
(155 TFLOP/s; the network with the voice-mask layer is 192 240 FLOP per 10 ms frame, halo recompute not counted) and
the bytes moved (input read twice -- once for the network, once for the product -- plus scores and enhanced frames)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOP_PER_FRAME = 5 * 2 * 80 * 80 + 2 * 2 * 5 * 80 * 80 + 2 * 80 + 80      # dense x4 + mask, conv1d x2, dense_4, product
ROOF_TF = 155.0


def main():
    import torch
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.vad import VAD
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    vad = VAD().load_saved_model(os.path.join(ROOT, "tests", "golden", "online_vad_model"))
    h = vad._handle(2)
    stream = torch.cuda.current_stream()
    rows = []
    for B, sec in ((60, 60), (1, 10)):
        L = sec * 16000
        x = (torch.randn(B, L, generator=torch.Generator().manual_seed(0)) * 0.1).cuda()
        T = L // 160
        scores = torch.empty(B, T, device="cuda")
        enh = torch.empty(B, T * 80, device="cuda")
        call = lambda: _lib.check(h.lib.mi355asr_vad_enhance(h.ptr, ctypes.c_void_p(x.data_ptr()), B, L, None,
                                                             ctypes.c_void_p(scores.data_ptr()),
                                                             ctypes.c_void_p(enh.data_ptr()),
                                                             ctypes.c_void_p(stream.cuda_stream)))
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        per = []
        for _ in range(a.regions):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                call()
            e1.record(stream)
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / a.iters)
        per.sort()
        med = float(np.median(per))
        flop = FLOP_PER_FRAME * B * T
        nbytes = B * T * (2 * 160 * 4 + 4 + 80 * 4)
        r = dict(B=B, seconds=sec, frames=B * T, ms_min=per[0], ms_median=med, ms_max=per[-1],
                 tflops_median=flop / (med * 1e-3) / 1e12, roof_share=flop / (med * 1e-3) / 1e12 / ROOF_TF,
                 floor_ms=flop / (ROOF_TF * 1e12) * 1e3, mbytes=nbytes / 1e6, gbps_median=nbytes / (med * 1e-3) / 1e9)
        rows.append(r)
        print("B=%d x %ds: %d frames  min %.3f  median %.3f  max %.3f ms/call  %.1f TFLOP/s = %.0f%% of %g TF "
              "(roof floor %.3f ms)  %.0f MB moved, %.0f GB/s" % (
                  B, sec, B * T, per[0], med, per[-1], r["tflops_median"], 100 * r["roof_share"], ROOF_TF,
                  r["floor_ms"], r["mbytes"], r["gbps_median"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
