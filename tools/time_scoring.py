"""Wall-clock timing of evaluation scoring: the host loop of the testers (`eval.wer` per pair, what `AMTester._eval_step` runs
without device_scoring) beside one `scoring.EditDistance` call on the GPU.

    python tools/time_scoring.py [--regions 5] [--iters 10] [--skip-host-long] [--json out.json]

Three workloads, ids seeded:
  eval_step   the scoring part of `_eval_step` at 64 utterances with the label lengths of the evaluation fixture of the tests
              (3 phones; 2 characters and the end id), the decoded rows 16 wide with padding behind them: host = copy both id
              streams to the host, strip and `wer` per utterance, twice; device = two calls with drop sets and the stop id, one
              [B, 6] copy each
  pairs_200   64 pairs of 200 x 200 tokens over 40 ids
  long_8192   one pair of 8 192 x 8 192 tokens over 40 ids (the host leg runs once: about half a minute of Python)
Device time is the host clock around `iters` calls that each end in the copy of the results to the host (a caller cannot use
them sooner); 3 warm-up calls; min / median / max over `regions`.  Host time is the host clock around the loop.  No speed is
asserted anywhere; the numbers go to DESIGN.md and README.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(call, regions, iters):
    for _ in range(3):
        call()
    per = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        per.append((time.perf_counter() - t0) * 1e3 / iters)
    per.sort()
    return {"min_ms": per[0], "median_ms": per[len(per) // 2], "max_ms": per[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-host-long", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    from tensorflowasr_amd.eval import wer
    from tensorflowasr_amd.scoring import EditDistance, filter_row
    if not torch.cuda.is_available():
        raise SystemExit("time_scoring.py measures on the GPU; there is none here")
    ed = EditDistance("cuda:0")
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "strip": ed.STRIP}

    # ---- the scoring part of AMTester._eval_step ----
    B, W = 64, 16
    ph_ref = rng.integers(4, 60, (B, 3)).astype(np.int32)
    tx_ref = np.concatenate([rng.integers(4, 100, (B, 2)), np.ones((B, 1))], 1).astype(np.int32)
    ph_hyp = np.zeros((B, W), np.int32)
    tx_hyp = np.zeros((B, W), np.int32)
    for b in range(B):
        n = int(rng.integers(1, 6))
        ph_hyp[b, :n] = rng.integers(4, 60, n)
        n = int(rng.integers(1, 5))
        tx_hyp[b, :n] = rng.integers(4, 100, n)
        tx_hyp[b, n] = 1
    ph_dev, tx_dev = torch.from_numpy(ph_hyp).cuda(), torch.from_numpy(tx_hyp).cuda()

    def host_step():
        p, t = ph_dev.cpu().numpy(), tx_dev.cpu().numpy()
        out = [wer(filter_row(r, (0,)), filter_row(h, (0,))) for h, r in zip(p, ph_ref)]
        return out + [wer(filter_row(r, (0, 1)), filter_row(h, (0, 1), stop=1)) for h, r in zip(t, tx_ref)]

    def device_step():
        a1 = torch.cat(ed(ph_ref, ph_dev, drop_ref=(0,), drop_hyp=(0,)), 1).cpu()
        a2 = torch.cat(ed(tx_ref, tx_dev, drop_ref=(0, 1), drop_hyp=(0, 1), hyp_stop=1), 1).cpu()
        return a1, a2

    h, (d1, d2) = host_step(), device_step()
    assert [list(x[1:]) for x in h] == d1[:, 1:4].tolist() + d2[:, 1:4].tolist(), "device and host scoring disagree"
    res["eval_step"] = {"host": spread(host_step, a.regions, a.iters), "device": spread(device_step, a.regions, a.iters)}

    # ---- 64 pairs of 200 x 200 ----
    r200, h200 = rng.integers(0, 40, (64, 200)).astype(np.int32), rng.integers(0, 40, (64, 200)).astype(np.int32)
    h200_dev = torch.from_numpy(h200).cuda()
    host = lambda: [wer(r.tolist(), h.tolist()) for r, h in zip(r200, h200_dev.cpu().numpy())]       # noqa: E731
    dev = lambda: ed(r200, h200_dev)[0].cpu()                                                          # noqa: E731
    assert [list(x[1:]) for x in host()] == dev()[:, 1:].tolist(), "device and host scoring disagree"
    res["pairs_200"] = {"host": spread(host, max(a.regions // 2, 1), 1), "device": spread(dev, a.regions, a.iters)}

    # ---- one pair of 8192 x 8192 ----
    r8k, h8k = rng.integers(0, 40, (1, 8192)).astype(np.int32), rng.integers(0, 40, (1, 8192)).astype(np.int32)
    h8k_dev = torch.from_numpy(h8k).cuda()
    dev = lambda: ed(r8k, h8k_dev)[0].cpu()                                                            # noqa: E731
    res["long_8192"] = {"device": spread(dev, a.regions, max(a.iters // 5, 1)), "cells": 8192 * 8192}
    if not a.skip_host_long:
        t0 = time.perf_counter()
        w = wer(r8k[0].tolist(), h8k[0].tolist())
        res["long_8192"]["host"] = {"once_ms": (time.perf_counter() - t0) * 1e3}
        assert list(w[1:]) == dev()[0, 1:].tolist(), "device and host scoring disagree"
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
