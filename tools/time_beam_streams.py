"""Timing of a ChunkConformer streaming tick with and without the stateful device beam search: 1 / 64 / 256
live streams, the text head's 9 160 classes (random weights), beam 10, cutoff_prob 0.99, cutoff_top_n 40, the synthetic 3-gram model
of tools/time_beam_lm.py (about 10^6 n-grams, built in memory from a seed).

    python tools/time_beam_streams.py [--reps 30] [--rounds 2] [--streams 1,64,256] [--json profiles/beam_streams_mi355x.json]
    rocprofv3 --kernel-trace --stats -- python tools/time_beam_streams.py --trace 64

Every leg runs in a fresh process (this script with --leg): 3 warm-up ticks, then `reps` ticks of `ChunkConformer.stream_step` over
all n streams, timed with a host clock around the tick, which ends in the tick's read-back.  The legs are run `rounds` times in
alternation; the median, minimum and maximum of each round are kept.  Legs:
  greedy   a tick as the server runs it without a beam                                                        (a)
  device   the same tick with `beam=BeamStreams(...)`: top-n + LM words + search enqueued behind the decoder   (b)
  host     the tick with want_logits, the text logits copied to the host, one host BeamDecoder per stream
           (commit, fork() for the rows that wait for right context) on 16 threads                            (c)
Nothing is asserted.  What decides whether the device search was worth building is (b) - (a) against (c) - (a) at 64 streams."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
V, BEAM, MAX_FRAMES = 9160, 10, 1500


def setup(n):
    import torch
    import oracle.conformer_oracle as co
    from helpers import chunk_config_dict
    from tensorflowasr_amd.models import ChunkConformer
    cfg = dict(co.CHUNK_S, decoder_num_classes=V)
    m = ChunkConformer(chunk_config_dict(cfg), phone=cfg["picker_num_classes"], txt=V)
    m.load_weights(co.chunk_weights(cfg, seed=0, picker_blank_bias=0.0), by_name=False)
    st = m.open_streams(n)
    g = torch.Generator().manual_seed(1)
    packets = (torch.randn((8, n, st.wav_buf_length), generator=g) * 0.1).cuda()      # a ring of 8 ticks of audio
    return m, st, packets


def softmax32(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def leg(name, n, reps):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from time_beam_lm import scorer
    from tensorflowasr_amd.models import BeamDecoder, BeamStreams
    assert torch.cuda.is_available(), "needs the MI355X"
    m, st, packets = setup(n)
    slots = list(range(n))
    s = scorer() if name != "greedy" else None
    bs = BeamStreams(n, V, BEAM, 0.99, 40, ext_scorer=s, max_frames=MAX_FRAMES) if name == "device" else None
    decs = [BeamDecoder([""] * V, BEAM, 0.99, 40, ext_scorer=s) for _ in range(n)] if name == "host" else None
    pool = ThreadPoolExecutor(16) if name == "host" else None
    frames = [0]

    def one(i, lg, nv, nu):
        hyp = decs[i].decode_ids(softmax32(lg[:nv]))
        return decs[i].fork().decode_ids(softmax32(lg[nv:nv + nu])) if nu else hyp

    def tick(k):
        pk = packets[k % 8]
        if name == "greedy":
            r = m.stream_step(st, slots, pk)
        elif name == "device":
            r = m.stream_step(st, slots, pk, beam=bs)
            assert all(v["beam_status"] == 0 for v in r.values())
        else:
            r = m.stream_step(st, slots, pk, want_logits=True)
            lg = torch.stack([torch.nn.functional.pad(r[i]["text_logits"], (0, 0, 0, st.win_back + 4 - r[i]["text_logits"].shape[0])) for i in slots]).cpu().numpy()
            list(pool.map(lambda i: one(i, lg[i], r[i]["n_valid"], r[i]["n_unvalid"]), slots))
        frames[0] += sum(v["n_valid"] for v in r.values())

    for k in range(3):
        tick(k)
    torch.cuda.synchronize()
    ms = []
    for k in range(reps):
        t0 = time.perf_counter()
        tick(3 + k)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    print(json.dumps({"leg": name, "streams": n, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": ms[0], "ms_max": ms[-1],
                      "text_frames_committed": int(frames[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--streams", default="1,64,256")
    ap.add_argument("--json", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--trace", type=int, default=None, help="streams: five greedy ticks and five ticks with the device beam, nothing else")
    a = ap.parse_args()
    if a.trace is not None:
        import torch
        from time_beam_lm import scorer
        from tensorflowasr_amd.models import BeamStreams
        m, st, packets = setup(a.trace)
        slots = list(range(a.trace))
        bs = BeamStreams(a.trace, V, BEAM, 0.99, 40, ext_scorer=scorer(), max_frames=MAX_FRAMES)
        for k in range(5):
            m.stream_step(st, slots, packets[k])
        for k in range(5):
            m.stream_step(st, slots, packets[k], beam=bs)
        torch.cuda.synchronize()
        print(json.dumps({"trace_streams": a.trace, "ticks_of_each_kind": 5}))
        return
    if a.leg:
        leg(a.leg, a.n, a.reps)
        return
    counts = [int(v) for v in a.streams.split(",")]
    res = []
    for rnd in range(a.rounds):
        for n in counts:
            for name in ("greedy", "device", "host"):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--n", str(n), "--reps", str(a.reps)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
                if r.returncode != 0:                      # a leg that failed is reported and nothing more is started
                    print(json.dumps({"leg": name, "streams": n, "round": rnd, "failed": r.returncode}), flush=True)
                    sys.exit(1)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                d.update(round=rnd)
                res.append(d)
                print(json.dumps(d), flush=True)
    summary = {}
    for n in counts:
        best = {name: min(d["ms_median"] for d in res if d["leg"] == name and d["streams"] == n) for name in ("greedy", "device", "host")}
        summary[str(n)] = dict(best, device_minus_greedy=best["device"] - best["greedy"], host_minus_greedy=best["host"] - best["greedy"])
    out = {"shape": {"V": V, "beam": BEAM, "cutoff_prob": 0.99, "cutoff_top_n": 40, "max_frames": MAX_FRAMES, "order": 3}, "legs": res,
           "summary": summary}
    print(json.dumps(summary))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
