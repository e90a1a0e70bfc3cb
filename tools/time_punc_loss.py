"""HIP-event timing of the punctuation model's training outputs (Punc.heads, against Punc.forward), of the punctuation trainer's losses
with and without their gradients (losses.punc_classes_loss, bert_feature_loss, punc_losses), and of the same arithmetic in torch ops
on the same device tensors (tests/punc_loss_ref.py torch_classes / torch_feature with autograd): what a user would run without them.

    python tools/time_punc_loss.py [--regions 5] [--json profiles/punc_loss_mi355x.json]

Shapes: B = 32 (the reference's data.yml batch size), T = 64 and T = 1024 (pe_input), F = 768, the shipped class count; every
sentence T tokens long.  Each figure is min / median / max milliseconds per call over `regions` timed regions of enough back-to-back
calls to last 0.1 s, bracketed by events on the launch stream, after three warm-up calls.  The calls as timed allocate their
outputs and workspace through the torch caching allocator, as a user's call does.  For the feature loss `hbm_bytes` counts what the
algorithm must move (read real and pred once; with the gradient write it once) and `tb_per_s` is that over the median time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

B, F = 32, 768
LENGTHS = (64, 1024)


def main():
    import torch
    import punc_loss_ref as R
    from punc_onnx_eval import onnx_path
    from test_punc_host import config
    from time_chunk_streams import region_timer
    from time_xent import clocks
    from tensorflowasr_amd import losses
    from tensorflowasr_amd.punc import Punc
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    timed = region_timer(a.regions, budget_ms=100.0)
    punc = Punc(config()).load_onnx(onnx_path())
    C = punc.cfg["classes"]
    out = {"regions": a.regions, "warmup_calls": 3, "region_budget_ms": 100.0, "B": B, "F": F, "classes": C, "shapes": []}
    for T in LENGTHS:
        ids = torch.from_numpy(R.seeded_ids([T] * B, T, punc.cfg["vocab"], 7)).cuda()
        lens = [T] * B                                      # a host list, as Punc.decisions passes it: both calls copy it to the device
        labels = torch.from_numpy(R.seeded_labels((B, T), C, 7)).cuda()
        logits, feature = punc.heads(ids, lens)
        real = torch.from_numpy(R.seeded_features((B, T, F), (B, T, F), 7)[0]).cuda()
        lg, ft = logits.clone().requires_grad_(True), feature.clone().requires_grad_(True)
        labels64 = labels.long()

        def torch_classes():
            with torch.no_grad():
                return R.torch_classes(labels64, logits)

        def torch_classes_grad():
            lg.grad = None
            R.torch_classes(labels64, lg)[0].sum().backward()
            return lg.grad

        def torch_feature():
            with torch.no_grad():
                return R.torch_feature(real, feature)

        def torch_feature_grad():
            ft.grad = None
            R.torch_feature(real, ft).sum().backward()
            return ft.grad

        def torch_losses_grad():
            lg.grad = ft.grad = None
            bd, acc = R.torch_classes(labels64, lg)
            ((10.0 * R.torch_feature(real, ft) + bd).sum() / B).backward()
            return lg.grad, ft.grad, acc.mean()

        legs = {
            "forward": lambda: punc.forward(ids, lens),
            "heads": lambda: punc.heads(ids, lens),
            "heads_logits_only": lambda: punc.heads(ids, lens, want_feature=False),
            "classes_loss": lambda: losses.punc_classes_loss(labels, logits),
            "classes_loss_grad": lambda: losses.punc_classes_loss(labels, logits, return_grad=True),
            "feature_loss": lambda: losses.bert_feature_loss(real, feature),
            "feature_loss_grad": lambda: losses.bert_feature_loss(real, feature, return_grad=True),
            "punc_losses": lambda: losses.punc_losses(labels, real, logits, feature),
            "punc_losses_grad": lambda: losses.punc_losses(labels, real, logits, feature, return_grad=True),
            "torch_classes_loss": torch_classes, "torch_classes_loss_grad": torch_classes_grad,
            "torch_feature_loss": torch_feature, "torch_feature_loss_grad": torch_feature_grad,
            "torch_punc_losses_grad": torch_losses_grad,
        }
        res = {"T": T}
        ours, theirs = losses.punc_losses(labels, real, logits, feature), (torch_classes()[0], torch_feature())
        res["agree_bd_loss"] = float(((ours["bd_loss"] - theirs[0]).abs() / theirs[0].abs()).max())
        res["agree_feature_map_loss"] = float(((ours["feature_map_loss"] - theirs[1]).abs() / theirs[1].abs()).max())
        # forward and heads alternate, twice, the better median kept: their difference is the figure of interest
        for name in ("forward", "heads", "forward", "heads"):
            t = timed(legs[name])
            if name not in res or t["ms_median"] < res[name]["ms_median"]:
                res[name] = t
        for name, leg in legs.items():
            if name not in res:
                res[name] = timed(leg)
        res["heads_over_forward"] = res["heads"]["ms_median"] / res["forward"]["ms_median"]
        res["feature_store_bytes"] = B * T * F * 4
        for k, nbytes in (("feature_loss", 2 * B * T * F * 4), ("feature_loss_grad", 3 * B * T * F * 4)):
            res[k]["hbm_bytes"] = nbytes
            res[k]["tb_per_s"] = nbytes / (res[k]["ms_median"] * 1e-3) / 1e12
        for k in ("classes_loss", "classes_loss_grad", "feature_loss", "feature_loss_grad", "punc_losses_grad"):
            res["torch_over_ours_" + k] = res["torch_" + k]["ms_median"] / res[k]["ms_median"]
        out["shapes"].append(res)
        print(json.dumps(res), flush=True)
    out["clocks"] = clocks()
    print(json.dumps({"clocks": out["clocks"]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
