"""HIP-event timing of the ragged entry points (mi355asr_recognize_ragged) on the benchmark's ConformerCTC(S).

    python tools/time_ragged.py [--regions 5] [--iters 10] [--json out.json]

Three regions, each as min / median / max milliseconds per call over `regions` timed regions of `iters` back-to-back
calls bracketed by events on the launch stream (after warm-up):
  equal    64 x 10 s, every length L: mi355asr_recognize against mi355asr_recognize_ragged
  ragged   64 utterances, seeded lengths uniform over 2 .. 15 s: recognize_ragged at [64, Lmax] against the padded
           mi355asr_recognize at [64, Lmax] (same work, wrong results for the shorter rows) and against the per-utterance
           loop (64 recognize calls of [1, L_b])"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, regions, iters):
    import torch
    stream = torch.cuda.current_stream()
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
    return dict(ms_min=per[0], ms_median=float(np.median(per)), ms_max=per[-1])


def main():
    import torch
    from bench import NUM_CLASSES, S_CFG
    from tensorflowasr_amd.models import ConformerCTC
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    m = ConformerCTC(NUM_CLASSES, **S_CFG)
    m._build()
    out = {}
    # (the ragged call reads its lengths back once per call: that synchronisation is inside the timed region)
    B, L = 64, 160000
    x = (torch.randn(B, L, generator=torch.Generator().manual_seed(0)) * 0.1).cuda()
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    out["equal_64x10s"] = dict(recognize=timed(lambda: m.recognize(x, reuse_buffers=True), a.regions, a.iters),
                               recognize_ragged=timed(lambda: m.recognize(x, wav_lengths=lens, reuse_buffers=True),
                                                      a.regions, a.iters))
    rng = np.random.default_rng(1)
    ln = rng.integers(2 * 16000, 15 * 16000 + 1, size=B).astype(np.int32)
    Lmax = int(ln.max())
    xr = (torch.randn(B, Lmax, generator=torch.Generator().manual_seed(1)) * 0.1).cuda()
    lr = torch.from_numpy(ln).cuda()
    solo = [xr[b:b + 1, :int(ln[b])].contiguous() for b in range(B)]

    def loop():
        for b in range(B):
            m.recognize(solo[b], reuse_buffers=False)
    out["uniform_2_15s_64"] = dict(
        Lmax=Lmax, seconds=float(ln.sum()) / 16000,
        recognize_ragged=timed(lambda: m.recognize(xr, wav_lengths=lr, reuse_buffers=True), a.regions, a.iters),
        recognize_padded=timed(lambda: m.recognize(xr, reuse_buffers=True), a.regions, a.iters),
        per_utterance_loop=timed(loop, 3, 1))
    e, r = out["equal_64x10s"], out["uniform_2_15s_64"]
    out["ratios"] = dict(
        equal_ragged_over_recognize=e["recognize_ragged"]["ms_median"] / e["recognize"]["ms_median"],
        ragged_over_padded=r["recognize_ragged"]["ms_median"] / r["recognize_padded"]["ms_median"],
        loop_over_ragged=r["per_utterance_loop"]["ms_median"] / r["recognize_ragged"]["ms_median"])
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
