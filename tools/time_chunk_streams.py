"""HIP-event timing of the batched ChunkConformer streams (ChunkConformer.open_streams / stream_step) on the shipped S
configuration (15 + 1 + 2 + 1 blocks, 277 phone and 9160 text classes; random weights, a picker bias that keeps about half of
the frames).

    python tools/time_chunk_streams.py [--regions 5] [--json profiles/chunk_streams_mi355x.json]
    rocprofv3 --kernel-trace --stats -- python tools/time_chunk_streams.py --trace-shape 64:16:8

Each figure is min / median / max milliseconds per step over `regions` timed regions of enough back-to-back steps to last 0.2 s,
bracketed by events on the launch stream, after warm-up:
  batched[n]       one stream_step over n streams in steady state (caches full, every stream active), n = 1, 16, 64, 256;
                   streams sustained in real time = n * 160 ms / step
  single_x64       the same 64 stream-steps through the single-stream calls (picker_stream_predict -> feature_pick ->
                   decoder_stream_predict) one after the other, alternating with batched[64] in the same process
--trace-shape n:age:steps runs `age` warm-up ticks and `steps` more over n streams and nothing else, for a kernel trace: the
launches per tick are (kernels in the trace - those of the reset) / (age + steps), the same for every n and age."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

W = 2560


def build_model(seed=0):
    from tensorflowasr_amd.config import load_yaml
    from tensorflowasr_amd.models import ChunkConformer
    from tensorflowasr_amd.synthetic import synth_batch
    conf = load_yaml(os.path.join(ROOT, "tensorflowasr_amd", "configs", "chunk_conformerS.yml"))
    m = ChunkConformer(conf, 277, 9160)
    m._build(seed)
    # blank bias at the median of (best non-blank logit - blank logit) over some audio: about half of the frames are kept
    x = synth_batch(0, 4, W * 20)
    z = m.predict(x, stages=True)["picker_logits"].cpu().numpy()
    w = dict(m._weights)
    b = np.array(w["picker/fully_connected/bias"], np.float32)
    b[-1] += float(np.median(z[..., :-1].max(-1) - z[..., -1]))
    w["picker/fully_connected/bias"] = b
    m.load_weights(w, by_name=False)
    return m


def region_timer(regions, budget_ms=200.0):
    import torch

    def timed(call):
        stream = torch.cuda.current_stream()
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); call(); e1.record(stream); e1.synchronize()
        iters = max(1, int(np.ceil(budget_ms / max(e0.elapsed_time(e1), 1e-3))))
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
        return dict(ms_min=per[0], ms_median=float(np.median(per)), ms_max=per[-1], iters=iters)
    return timed


def main():
    import torch
    from tensorflowasr_amd.synthetic import synth_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-shape", default=None, help="n:age:steps")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    m = build_model()
    if a.trace_shape:
        n, age, steps = (int(v) for v in a.trace_shape.split(":"))
        st = m.open_streams(n)
        pk = torch.from_numpy(synth_batch(3, n, W)).cuda()
        for _ in range(age + steps):
            m.stream_step(st, list(range(n)), pk)
        torch.cuda.synchronize()
        print(json.dumps({"trace_shape": dict(streams=n, ticks=age + steps)}))
        return
    timed = region_timer(a.regions)
    out = {"config": "chunk_conformerS.yml, 277 / 9160 classes, fp32", "packet_ms": 160.0, "batched": {}}
    picked = None
    for n in [int(v) for v in a.sizes.split(",")]:
        st = m.open_streams(n)
        audio = torch.from_numpy(synth_batch(7, n, W * 16)).cuda()
        slots = list(range(n))
        for k in range(16):                                    # steady state: every cache full
            r = m.stream_step(st, slots, audio[:, k * W:(k + 1) * W].contiguous())
        pk = audio[:, 15 * W:].contiguous()
        t = timed(lambda: m.stream_step(st, slots, pk))
        t["streams_in_real_time"] = n * 160.0 / t["ms_median"]
        t["picked_per_stream_last_tick"] = float(np.mean([v["n_picked"] for v in r.values()]))
        out["batched"][str(n)] = t
        print("batched", n, t, flush=True)
        if n == 64:
            picked = (st, slots, pk)
    if picked is not None:
        st, slots, pk = picked
        x1 = synth_batch(7, 1, W * 16)
        caches, caches2 = m.init_picker_caches(1), m.init_decoder_caches(1)
        for k in range(16):
            vp, _, vh, caches = m.picker_stream_predict(x1[:, k * W:(k + 1) * W, None], caches)
            f, _ = m.feature_pick(vh, vp)
            if f.shape[1]:
                _, _, caches2 = m.decoder_stream_predict(f, caches2)
        p1 = torch.from_numpy(x1[:, 15 * W:, None]).cuda()

        def single_x64():
            for _ in range(64):
                vp, _, vh, _ = m.picker_stream_predict(p1, caches)      # (the caches are not advanced: every call does a steady-state step)
                f, _ = m.feature_pick(vh, vp)
                if f.shape[1]:
                    m.decoder_stream_predict(f, caches2)

        legs = {"batched_64": [], "single_x64": []}
        for _ in range(3):                                     # the two legs alternating
            legs["batched_64"].append(timed(lambda: m.stream_step(st, slots, pk)))
            legs["single_x64"].append(timed(single_x64))
        bm = float(np.median([t["ms_median"] for t in legs["batched_64"]]))
        sm = float(np.median([t["ms_median"] for t in legs["single_x64"]]))
        out["single_vs_batched_64"] = dict(legs, batched_ms=bm, single_x64_ms=sm, ratio=sm / bm)
        print("single x 64 / batched 64:", sm, bm, sm / bm, flush=True)
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
