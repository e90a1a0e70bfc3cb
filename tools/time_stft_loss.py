"""HIP-event timing of the multi-resolution STFT loss (losses.MultiResolutionSTFTLoss: the scalar alone, the scalar with its gradient)
and of the same arithmetic in torch on the same device tensors: unfold x window, torch.fft.rfft, the reference's formula, autograd.

    python tools/time_stft_loss.py [--regions 5] [--json profiles/stft_loss_mi355x.json]

Shapes: 4 x 48 000 (the shipped VAD config: batch 4 of 6 s at 8 kHz) and 64 x 48 000, the reference's two resolutions.  Each figure
is min / median / max milliseconds per call over `regions` timed regions of enough back-to-back calls to last 0.2 s, bracketed by
events on the launch stream, after three warm-up calls; the legs alternate and the whole round is taken twice, the better median
kept.  The calls as timed allocate their workspace and outputs through the torch caching allocator and form the scalar with a few
small torch kernels, as a user's call does.  `launch_bound` marks a leg within 3 x of a one-frame call measured in the same run.
Not timed: ragged batches, (2048, 2048, 512), the mask statistics (one workgroup; a launch), the first call (it builds and uploads
the tables)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SHAPES = [dict(B=4, L=48000), dict(B=64, L=48000)]
RESOLUTIONS = ((1024, 600, 120), (512, 250, 50))


def torch_stft_loss(y, x, windows):
    import torch
    sc_sum, mag_sum = 0.0, 0.0
    for (fft, fl, step), win in zip(RESOLUTIONS, windows):
        P = torch.fft.rfft(x.unfold(1, fl, step) * win, n=fft)
        T = torch.fft.rfft(y.unfold(1, fl, step) * win, n=fft)
        p = torch.sqrt(P.real ** 2 + P.imag ** 2 + 1e-7) + 1e-6
        t = torch.sqrt(T.real ** 2 + T.imag ** 2 + 1e-7) + 1e-6
        sc = torch.sqrt(((p - t) ** 2).sum((1, 2))) / (torch.sqrt((p ** 2).sum((1, 2))) + 1e-6)
        sc_sum = sc_sum + sc.mean()
        mag_sum = mag_sum + ((torch.log(p) - torch.log(t)) ** 2).mean()
    return (sc_sum + mag_sum) / len(RESOLUTIONS)


def main():
    import torch
    from time_chunk_streams import region_timer
    from time_xent import clocks
    from tensorflowasr_amd.losses import MultiResolutionSTFTLoss
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    timed = region_timer(a.regions)
    fn = MultiResolutionSTFTLoss()
    windows = [(0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(fl, dtype=torch.float64) / fl)).float().cuda() for _, fl, _ in RESOLUTIONS]
    out = {"regions": a.regions, "warmup_calls": 3, "rounds": 2, "region_budget_ms": 200.0, "resolutions": RESOLUTIONS, "shapes": []}
    one = torch.randn((1, 600), device="cuda")
    out["one_frame_call"] = timed(lambda: fn(one, one))
    for shape in SHAPES:
        B, L = shape["B"], shape["L"]
        g = torch.Generator().manual_seed(0)
        y = (torch.randn((B, L), generator=g) * 0.1).cuda()
        x = (0.8 * y + 0.02 * torch.randn((B, L), generator=g).cuda()).contiguous()
        xg = x.clone().requires_grad_(True)

        def torch_loss():
            with torch.no_grad():
                return torch_stft_loss(y, x, windows)

        def torch_loss_grad():
            xg.grad = None
            torch_stft_loss(y, xg, windows).backward()
            return xg.grad

        legs = {"loss": lambda: fn(y, x), "loss_grad": lambda: fn(y, x, return_grad=True),
                "torch_loss": torch_loss, "torch_loss_grad": torch_loss_grad}
        res = {"shape": shape, "frames": [1 + (L - fl) // st for _, fl, st in RESOLUTIONS]}
        res["agree"] = abs(float(fn(y, x)) - float(torch_loss())) / abs(float(torch_loss()))
        for _ in range(2):
            for name, leg in legs.items():
                t = timed(leg)
                if name not in res or t["ms_median"] < res[name]["ms_median"]:
                    t["launch_bound"] = bool(t["ms_median"] < 3 * out["one_frame_call"]["ms_median"])
                    res[name] = t
        res["torch_over_ours_loss"] = res["torch_loss"]["ms_median"] / res["loss"]["ms_median"]
        res["torch_over_ours_loss_grad"] = res["torch_loss_grad"]["ms_median"] / res["loss_grad"]["ms_median"]
        out["shapes"].append(res)
        print(json.dumps(res), flush=True)
    out["clocks"] = clocks()
    print(json.dumps({"one_frame_call": out["one_frame_call"], "clocks": out["clocks"]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
