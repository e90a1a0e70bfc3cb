"""HIP-event timing of the CTC loss, loss + gradient and forced alignment (models.ctc_loss / ctc_forced_align) against
torch.nn.functional.ctc_loss (with log_softmax, and backward for the gradient) on the same GPU -- the only other implementation
there -- and, for context, against the recognise step of the benchmark.

    python tools/time_ctc_loss.py [--regions 5] [--json profiles/ctc_loss_mi355x.json]
    rocprofv3 --kernel-trace --stats -- python tools/time_ctc_loss.py --trace-shape 0

Shapes: 64 x 250 x 1332 with 20..60 labels, 16 x 750 x 9160 with 50..150 labels (seeded; ragged input lengths, one row full).
Each figure is min / median / max milliseconds per call over `regions` timed regions of enough back-to-back calls to last 0.2 s,
bracketed by events on the launch stream, after warm-up.  The calls as timed allocate their outputs and workspace through the
torch caching allocator, as a user's call does.  The row passes have a floor: one read of B x T x V x 4 bytes for the loss and the
alignment, plus one more read and one write for the gradient pass; `floor_fraction` = floor bytes / 6.29 TB/s (the measured copy
rate of the chip) / measured time -- of the whole call, lattice included, so it understates the row kernels.
torch's loss differs in definition (no + 1e-7 chain): it is timed, not compared."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SHAPES = [dict(B=64, T=250, V=1332, U=60, lo=20), dict(B=16, T=750, V=9160, U=150, lo=50)]
HBM_COPY_BYTES_PER_S = 6.29e12
RECOGNIZE_STEP_MS = 1.816          # the benchmark's recognise step


def make(shape, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    B, T, V, U = shape["B"], shape["T"], shape["V"], shape["U"]
    z = torch.randn((B, T, V), generator=g)
    labels = torch.randint(0, V - 1, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(shape["lo"], U + 1, (B,), generator=g, dtype=torch.int32)
    il = torch.randint(max(T // 2, 2 * U), T + 1, (B,), generator=g, dtype=torch.int32)
    il[0], ll[0] = T, U
    return z.cuda(), labels.cuda(), il.cuda(), ll.cuda()


def main():
    import torch
    from time_chunk_streams import region_timer
    from tensorflowasr_amd.models import ctc_forced_align, ctc_loss
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-shape", type=int, default=None, help="index into the shapes: a few calls of each kind, nothing else")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.trace_shape is not None:
        z, lab, il, ll = make(SHAPES[a.trace_shape])
        for _ in range(5):
            ctc_loss(z, lab, il, ll)
            ctc_loss(z, lab, il, ll, return_grad=True)
            ctc_forced_align(z, lab, il, ll)
        torch.cuda.synchronize()
        print(json.dumps({"trace_shape": SHAPES[a.trace_shape], "calls_of_each_kind": 5}))
        return
    timed = region_timer(a.regions)
    out = {"recognize_step_ms": RECOGNIZE_STEP_MS, "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "shapes": []}
    for shape in SHAPES:
        z, lab, il, ll = make(shape)
        B, T, V = shape["B"], shape["T"], shape["V"]
        row_bytes = float(B * T * V * 4)
        il64, ll64, lab64 = il.long(), ll.long(), lab.long()
        zg = z.clone().requires_grad_(True)

        def torch_loss():
            with torch.no_grad():
                return torch.nn.functional.ctc_loss(torch.log_softmax(z, -1).transpose(0, 1), lab64, il64, ll64, blank=V - 1,
                                                    reduction="none")

        def torch_loss_grad():
            zg.grad = None
            l = torch.nn.functional.ctc_loss(torch.log_softmax(zg, -1).transpose(0, 1), lab64, il64, ll64, blank=V - 1,
                                             reduction="none")
            l.sum().backward()
            return zg.grad

        legs = {"loss": (lambda: ctc_loss(z, lab, il, ll), 1.0), "loss_grad": (lambda: ctc_loss(z, lab, il, ll, return_grad=True), 3.0),
                "align": (lambda: ctc_forced_align(z, lab, il, ll), 1.0), "torch_loss": (torch_loss, None),
                "torch_loss_grad": (torch_loss_grad, None)}
        res = {"shape": shape}
        for _ in range(2):                                     # the legs alternating, twice: keep the better median
            for name, (fn, passes) in legs.items():
                t = timed(fn)
                if name not in res or t["ms_median"] < res[name]["ms_median"]:
                    if passes is not None:
                        t["floor_ms"] = passes * row_bytes / HBM_COPY_BYTES_PER_S * 1e3
                        t["floor_fraction"] = t["floor_ms"] / t["ms_median"]
                    t["recognize_steps"] = t["ms_median"] / RECOGNIZE_STEP_MS
                    res[name] = t
        res["torch_over_ours_loss"] = res["torch_loss"]["ms_median"] / res["loss"]["ms_median"]
        res["torch_over_ours_loss_grad"] = res["torch_loss_grad"]["ms_median"] / res["loss_grad"]["ms_median"]
        out["shapes"].append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
