"""Timing of the CTC prefix beam search with the n-gram scorer at the config-5 search shape (16 utterances, the
ChunkConformer's 9 160 text classes, ragged lengths up to 600 picked frames, cutoff_prob 0.99, cutoff_top_n 40) with a synthetic
3-gram model over the hanzi vocabulary of about 10^6 n-grams, built in memory from a seed.

    python tools/time_beam_lm.py [--reps 15] [--rounds 2] [--parent-lib PATH] [--json profiles/beam_lm_mi355x.json]
    rocprofv3 --kernel-trace --stats -- python tools/time_beam_lm.py --trace 100

Every leg runs in a fresh process (this script with --leg): 3 warm-up calls, then `reps` calls, each a whole
`ctc_prefix_beam_decode` on device logits -- top-n kernel, search, results on the host -- timed with a host clock around the
call, which ends in a stream synchronise.  The legs are run `rounds` times in alternation; per leg the median, minimum and
maximum of each round are kept, so the run-to-run spread stands next to every difference.  Legs, at beam 10 and beam 100:
  plain          scorer-less device search, this build                         (a)
  plain_parent   the same call on another build of the library (--parent-lib)  (a): must not move beyond the spread
  lm_device      scored device search                                          (b) = lm_device / plain: the price of the LM
  lm_host        scored host search on 16 threads, on the device's top-n lists (c) = lm_host / lm_device
Nothing is asserted: the figures go to DESIGN.md section 14."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
V, B, T = 9160, 16, 600
N2, N3 = 300000, 700000


def inputs(seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, T, V), generator=g) * 3.0
    z[..., -1] += 6.0
    lens = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32)
    lens[0] = T
    return z.cuda(), lens.numpy()


def scorer():
    from tensorflowasr_amd import ngram
    chars = [chr(0x4E00 + i) for i in range(V - 1)]
    return ngram.NGramScorer(0.8, 0.4, "synthetic", chars, model=ngram.synthetic_model(chars[:-300], N2, N3, seed=5))


def leg(name, beam, reps):
    """one leg in this process -> a JSON line"""
    import torch
    from tensorflowasr_amd import _lib
    if os.environ.get("MI355ASR_LIB"):                     # another build: bind only the symbols it has
        import ctypes
        h = ctypes.CDLL(os.environ["MI355ASR_LIB"])
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(h, k)}
    from tensorflowasr_amd.models import ctc_prefix_beam_decode
    assert torch.cuda.is_available(), "needs the MI355X"
    z, lens = inputs()
    s = scorer() if name.startswith("lm") else None
    call = lambda: ctc_prefix_beam_decode(z, lens, beam, 0.99, 40, is_logits=True, num_threads=16, ext_scorer=s)   # noqa: E731
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    print(json.dumps({"leg": name, "beam": beam, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": ms[0], "ms_max": ms[-1],
                      "hypotheses": int(out[3].sum()), "best_score_0": float(out[2][0, 0]), "best_len_0": int(out[1][0, 0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--trace", type=int, default=None, help="beam width: five scored device calls and nothing else")
    a = ap.parse_args()
    if a.trace is not None:
        import torch
        from tensorflowasr_amd.models import ctc_prefix_beam_decode
        z, lens = inputs()
        s = scorer()
        for _ in range(5):
            ctc_prefix_beam_decode(z, lens, a.trace, 0.99, 40, is_logits=True, ext_scorer=s)
            ctc_prefix_beam_decode(z, lens, a.trace, 0.99, 40, is_logits=True)
        torch.cuda.synchronize()
        print(json.dumps({"trace_beam": a.trace, "calls_of_each_kind": 5}))
        return
    if a.leg:
        leg(a.leg, a.beam, a.reps)
        return
    legs = [("plain", {}), ("lm_device", {}), ("lm_host", {"MI355ASR_BEAM_DEVICE": "0"})]
    if a.parent_lib:
        legs.insert(1, ("plain_parent", {"MI355ASR_LIB": os.path.abspath(a.parent_lib)}))
    res = []
    for rnd in range(a.rounds):
        for beam in (10, 100):
            for name, env in legs:
                reps = max(3, a.reps // 3) if name == "lm_host" else a.reps
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", name.replace("_parent", ""), "--beam", str(beam), "--reps", str(reps)]
                r = subprocess.run(cmd, env=dict(os.environ, **env), stdout=subprocess.PIPE, text=True, timeout=900)
                if r.returncode != 0:                  # a leg that failed is reported and nothing more is started
                    print(json.dumps({"leg": name, "beam": beam, "round": rnd, "failed": r.returncode}), flush=True)
                    sys.exit(1)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                d.update(leg=name, round=rnd)
                res.append(d)
                print(json.dumps(d), flush=True)
    summary = {}
    for beam in (10, 100):
        med = {name: [d["ms_median"] for d in res if d["leg"] == name and d["beam"] == beam] for name, _ in legs}
        best = {k: min(v) for k, v in med.items()}
        summary[str(beam)] = {"ms_median_per_round": med, "lm_device_over_plain": best["lm_device"] / best["plain"],
                              "lm_host_over_lm_device": best["lm_host"] / best["lm_device"]}
        if "plain_parent" in best:
            summary[str(beam)]["plain_over_parent"] = best["plain"] / best["plain_parent"]
    out = {"shape": {"B": B, "T": T, "V": V, "cutoff_prob": 0.99, "cutoff_top_n": 40, "lm_ngrams": V - 1 - 300 + 3 + N2 + N3, "order": 3},
           "legs": res, "summary": summary}
    print(json.dumps(summary))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
