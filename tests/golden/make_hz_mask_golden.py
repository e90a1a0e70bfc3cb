"""Records tests/golden/hz_mask_ref.npz: the reference's own SignalHz and SignalMask (both mask_with_noise values) run as they
are -- its imports that are not installed (librosa, rir_generator) stubbed in sys.modules as make_augment_golden.py does -- for
the seeds 0 .. 2 on seeded inputs of 22, 1500 and 4000 samples (seed k with input k).  Per case: the input (float32 values,
handed over as float64), the start SignalHz drew, the float64 outputs, how many np.random.random calls were made with which
sizes, and the draw that FOLLOWS the call (np.random.random() right after it), which pins how much of the generator's state the
call consumed.  The uniforms themselves are not stored: np.random.seed(seed) reproduces them, and the outputs pin them.

    python tests/golden/make_hz_mask_golden.py /path/to/TensorflowASR
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [0, 1, 2]
LENGTHS = [22, 1500, 4000]
ZONE, RATIO = "(0.1,0.9)", 0.3


def inputs():
    return [(np.random.default_rng(100 + k).uniform(-1, 1, n) * 0.5).astype(np.float32) for k, n in enumerate(LENGTHS)]


def main(ref_root):
    sys.modules["rir_generator"], sys.modules["librosa"] = types.ModuleType("rir_generator"), types.ModuleType("librosa")
    spec = importlib.util.spec_from_file_location("ref_augments", os.path.join(ref_root, "augmentations", "augments.py"))
    aug = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aug)
    out = {"seeds": np.array(SEEDS), "lengths": np.array(LENGTHS), "zone": np.array(eval(ZONE)), "mask_ratio": np.array(RATIO)}
    real = np.random.random

    def traced(fn, data):
        sizes, scalars = [], []

        def random(size=None):
            sizes.append(-1 if size is None else int(np.prod(size)))
            v = real(size)
            if size is None:
                scalars.append(float(v))
            return v
        np.random.random = random
        try:
            y = fn(data)
        finally:
            np.random.random = real
        return np.asarray(y, np.float64), np.array(sizes), real(), scalars

    for k, (seed, x) in enumerate(zip(SEEDS, inputs())):
        out["x%d" % k] = x
        np.random.seed(seed)
        y, sizes, nxt, scalars = traced(aug.SignalHz().augment, x.astype(np.float64))
        start = float(np.clip(scalars[0], 0.01, 0.699))             # SignalHz's own expression on its own first draw
        out["hz_start%d" % k], out["hz_out%d" % k], out["hz_sizes%d" % k], out["hz_next%d" % k] = np.array(start), y, sizes, np.array(nxt)
        for noise in (0, 1):
            np.random.seed(seed)
            y, sizes, nxt, _ = traced(aug.SignalMask(ZONE, RATIO, bool(noise)).augment, x.astype(np.float64))
            out["mask%d_out%d" % (noise, k)], out["mask%d_sizes%d" % (noise, k)], out["mask%d_next%d" % (noise, k)] = y, sizes, np.array(nxt)
    path = os.path.join(HERE, "hz_mask_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote hz_mask_ref.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
