"""HIP-event timing of the softmax cross-entropy (losses.sparse_xent: loss with arg-max, loss with gradient), of mask_loss with and
without its gradient, and of torch.nn.functional.cross_entropy (with and without backward) on the same device tensors.

    python tools/time_xent.py [--regions 5] [--json profiles/xent_mi355x.json]

Shapes: 64 x 20 x 9160 (an evaluation step of the Translator head) and 64 x 250 x 1332.  Each figure is min / median / max
milliseconds per call over `regions` timed regions of enough back-to-back calls to last 0.2 s, bracketed by events on the launch
stream, after three warm-up calls; the legs alternate and the whole round is taken twice, the better median kept (`iters` is the
number of calls per region).  The calls as timed allocate their outputs through the torch caching allocator, as a user's call does.
bytes: the loss reads B x Q x V x 4 bytes once, the gradient writes as many; `hbm_fraction` = bytes / time / 6.29 TB/s, the copy
rate the chip was measured at (its specification says 8 TB/s).  Both inputs (47 MB and 85 MB) fit the 256 MiB Infinity Cache and
are re-read by back-to-back calls, so the rate is a rate from cache, not from HBM; `launch_bound` marks a leg whose time is
within 3 x of an empty launch measured in the same run: that leg measures launch latency, not the kernel.
The clocks are what the device properties and, where it answers, `rocm-smi --showclocks` report after the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SHAPES = [dict(B=64, Q=20, V=9160), dict(B=64, Q=250, V=1332)]
HBM_COPY_BYTES_PER_S = 6.29e12


def clocks():
    import torch
    p = torch.cuda.get_device_properties(0)
    out = {"device": p.name, "max_engine_clock_khz": getattr(p, "clock_rate", None), "max_memory_clock_khz": getattr(p, "memory_clock_rate", None)}
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        cards = json.loads(r.stdout)
        out["rocm_smi_showclocks_card0"] = cards.get("card0", cards)
    except Exception as e:                                  # the tool is optional: the properties above are always there
        out["rocm_smi_showclocks_card0"] = "unavailable: %s" % type(e).__name__
    return out


def main():
    import torch
    from time_chunk_streams import region_timer
    from tensorflowasr_amd.losses import mask_loss, sparse_xent
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    timed = region_timer(a.regions)
    out = {"hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "regions": a.regions, "warmup_calls": 3, "rounds": 2, "region_budget_ms": 200.0,
           "shapes": []}
    one = torch.zeros((1, 1, 8), device="cuda")
    lab1 = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    out["one_row_launch"] = timed(lambda: sparse_xent(one, lab1))          # a one-workgroup call: wrapper + launch latency
    for shape in SHAPES:
        B, Q, V = shape["B"], shape["Q"], shape["V"]
        g = torch.Generator().manual_seed(0)
        x = (torch.randn((B, Q, V), generator=g) * 3).cuda()
        y = torch.randint(0, V, (B, Q), generator=g, dtype=torch.int32)
        y[:, Q // 2:] *= (torch.rand((B, Q - Q // 2), generator=g) < 0.5).int()      # pads, as a text batch has
        y = y.cuda()
        y64 = y.long().reshape(-1)
        xg = x.clone().requires_grad_(True)
        up = torch.rand((B,), generator=g).cuda()
        plane = float(B * Q * V * 4)

        def torch_loss():
            with torch.no_grad():
                return torch.nn.functional.cross_entropy(x.reshape(-1, V), y64, reduction="none")

        def torch_loss_grad():
            xg.grad = None
            torch.nn.functional.cross_entropy(xg.reshape(-1, V), y64, reduction="sum").backward()
            return xg.grad

        legs = {"loss": (lambda: sparse_xent(x, y, return_argmax=True), plane),
                "loss_grad": (lambda: sparse_xent(x, y, return_grad=True, return_argmax=True), 2 * plane),
                "mask_loss": (lambda: mask_loss(y, x), plane),
                "mask_loss_grad": (lambda: mask_loss(y, x, return_grad=True, upstream=up), 2 * plane),
                "torch_loss": (torch_loss, plane), "torch_loss_grad": (torch_loss_grad, 2 * plane)}
        res = {"shape": shape, "input_bytes": plane}
        for _ in range(2):
            for name, (fn, nbytes) in legs.items():
                t = timed(fn)
                if name not in res or t["ms_median"] < res[name]["ms_median"]:
                    t["bytes"] = nbytes
                    t["hbm_fraction"] = nbytes / (t["ms_median"] * 1e-3) / HBM_COPY_BYTES_PER_S
                    t["launch_bound"] = bool(t["ms_median"] < 3 * out["one_row_launch"]["ms_median"])
                    res[name] = t
        res["torch_over_ours_loss"] = res["torch_loss"]["ms_median"] / res["loss"]["ms_median"]
        res["torch_over_ours_loss_grad"] = res["torch_loss_grad"]["ms_median"] / res["loss_grad"]["ms_median"]
        out["shapes"].append(res)
        print(json.dumps(res), flush=True)
    out["clocks"] = clocks()
    print(json.dumps({"one_row_launch": out["one_row_launch"], "clocks": out["clocks"]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
