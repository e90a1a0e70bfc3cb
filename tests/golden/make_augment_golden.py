"""Records tests/golden/augment_draws.json: what the reference's own SignalRIR and SignalNoise draw from `random` and
`np.random` for the seeds 0 .. 3 -- the positions SignalRIR.augment hands to rir_generator.generate, and the recording, start
and SNR SignalNoise.augment draws for a fixed bank and fixed utterance lengths.  The reference's class runs as it is; its
imports that are not installed (librosa, rir_generator) are stubbed in sys.modules, the stubs recording what they are given.

    python tests/golden/make_augment_golden.py /path/to/TensorflowASR
"""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [0, 1, 2, 3]
CALLS = 6                                   # augment() calls per seed
BANK_LENS = [700, 5000, 48000]              # samples of the three noise recordings
LENGTHS = [1, 690, 4985, 16000, 48000, 100003]   # utterance lengths, one per call
SNR = [0, 15]


def main(ref_root):
    calls = []
    rir = types.ModuleType("rir_generator")
    rir.generate = lambda **kw: calls.append(kw) or np.ones((4, 1))
    librosa = types.ModuleType("librosa")
    loaded = []

    def load(path, sr):
        i = int(os.path.basename(path).split(".")[0][1:])
        loaded.append(i)
        return np.zeros(BANK_LENS[i], np.float32) + 0.5, sr
    librosa.load = load
    sys.modules["rir_generator"], sys.modules["librosa"] = rir, librosa
    spec = importlib.util.spec_from_file_location("ref_augments", os.path.join(ref_root, "augmentations", "augments.py"))
    aug = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aug)
    out = {"seeds": SEEDS, "room": [5, 4, 6], "bank_lens": BANK_LENS, "lengths": LENGTHS, "snr": SNR, "rir": {}, "noise": {}}
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "noises.txt")
        with open(lst, "w") as f:
            f.write("".join("n%d.wav\n" % i for i in range(len(BANK_LENS))))
        for seed in SEEDS:
            random.seed(seed)
            np.random.seed(seed)
            del calls[:]
            r = aug.SignalRIR(16000)
            for _ in range(CALLS):
                r.augment(np.zeros(8))
            out["rir"][str(seed)] = [{"receiver": list(kw["r"]), "source": list(kw["s"])} for kw in calls]
            random.seed(seed)
            np.random.seed(seed)
            nz = aug.SignalNoise(16000, SNR, lst)
            real = np.random.randint
            rows = []
            for n in LENGTHS:
                drawn = []
                np.random.randint = lambda *a, **k: drawn.append(int(real(*a, **k))) or drawn[-1]
                try:
                    del loaded[:]
                    nz.augment(np.full(n, 0.25))
                finally:
                    np.random.randint = real
                assert len(drawn) == 3 and loaded == [drawn[0]], (drawn, loaded)
                rows.append({"noise": drawn[0], "start": drawn[1], "snr_db": drawn[2]})
            out["noise"][str(seed)] = rows
    with open(os.path.join(HERE, "augment_draws.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote augment_draws.json")


if __name__ == "__main__":
    main(sys.argv[1])
