"""HIP-event timing of mi355asr_punc_forward (punc.hip): B = 1 / 64 / 256 sentences of 20 and 100 tokens, and one of 1024.

    python tools/time_punc.py [--regions 7] [--iters 20] [--json out.json]

Per shape: 5 warm-up calls, then `regions` timed regions of `iters` back-to-back calls each, bracketed by events on the
launch stream; prints min / median / max microseconds per call.  Weights: the trained export under tests/golden, random
ids in [3, vocab) between the markers.  There is no target: the figures are recorded in DESIGN.md section 18 as measured."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from punc_onnx_eval import GOLDEN, onnx_path
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.punc import Punc
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    voc = lambda f: {"vocabulary": os.path.join(GOLDEN, f), "blank_at_zero": True}
    punc = Punc({"model_config": dict(num_layers=3, d_model=64, enc_embedding_dim=64, num_heads=8, dff=64, pe_input=1024),
                 "punc_vocab": voc("punc_tokens_ch.txt"), "punc_biaodian": voc("punc_tokens_bd.txt")}).load_onnx(onnx_path())
    h = punc._handle()
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    rows = []
    for B, T in ((1, 20), (64, 20), (256, 20), (1, 100), (64, 100), (256, 100), (1, 1024)):
        ids = rng.integers(3, punc.cfg["vocab"], (B, T)).astype(np.int32)
        ids[:, 0], ids[:, -1] = 1, 2
        x = torch.from_numpy(ids).cuda()
        probs = torch.empty(B, T, punc.cfg["classes"], device="cuda")
        cls = torch.empty(B, T, dtype=torch.int32, device="cuda")
        pmax = torch.empty(B, T, device="cuda")
        n = ctypes.c_size_t()
        _lib.check(h.lib.mi355asr_punc_workspace_bytes(h.ptr, B, T, ctypes.byref(n)))
        ws = torch.empty(max(n.value, 1), dtype=torch.uint8, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call = lambda: _lib.check(h.lib.mi355asr_punc_forward(h.ptr, p(x), None, B, T, p(probs), p(cls), p(pmax), p(ws), n.value,
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
            per.append(e0.elapsed_time(e1) / a.iters * 1e3)
        per.sort()
        r = dict(B=B, tokens=T, us_min=per[0], us_median=float(np.median(per)), us_max=per[-1],
                 us_per_sentence=float(np.median(per)) / B)
        rows.append(r)
        print("B %4d  T %5d   %9.1f / %9.1f / %9.1f us per call (min / median / max)   %8.2f us per sentence"
              % (B, T, r["us_min"], r["us_median"], r["us_max"], r["us_per_sentence"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
