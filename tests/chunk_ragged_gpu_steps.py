"""The GPU steps of tests/test_gpu_chunk_ragged.py that need a process of their own, because the switch they set is read once per
process: `python tests/chunk_ragged_gpu_steps.py STEP`.  A step prints what it measured and exits non-zero on the first mismatch;
it is never repeated."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import chunk_ragged as cr                                              # noqa: E402
from helpers import chunk_config_dict                                  # noqa: E402


def model(cfg, w):
    from tensorflowasr_amd.models import ChunkConformer
    m = ChunkConformer(chunk_config_dict(cfg), cfg["picker_num_classes"], cfg["decoder_num_classes"])
    m.load_weights(w, by_name=False)
    return m


def host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def step_band_l2():
    """MI355ASR_ATTN_BAND_LDS=0: attention_kernel<36, 4> with K / V from L2 on the 21 edge lengths, against the oracle alone"""
    assert os.environ.get("MI355ASR_ATTN_BAND_LDS") == "0"
    cfg = cr.config()
    w = cr.weights(cfg, 3, 20.0, -20.0)
    items = cr.batch_items(cr.edge_batches()["ns-21x80"])
    refs = [cr.alone(it, w, cfg, "edge") for it in items]
    cr.assert_picker_margin(refs)
    x, lens = cr.padded(items)
    got = host(model(cfg, w).predict(x, stages=True, wav_lengths=lens))
    cr.compare_with_oracle(got, lens, refs, cfg, "band attention from L2")


def step_gemm16():
    """MI355ASR_GEMM16=1, the layer-at-a-time GEMM family for every row count: the ragged call refuses before anything is launched"""
    assert os.environ.get("MI355ASR_GEMM16") == "1"
    from tensorflowasr_amd import _lib
    cfg = cr.config()
    m = model(cfg, cr.weights(cfg, 3, 20.0, -20.0))
    items = cr.batch_items(cr.edge_batches()["layers-2x16"])
    x, lens = cr.padded(items, fill=0.0)
    try:
        m.predict(x, wav_lengths=lens)
    except _lib.Mi355AsrError as e:
        print("refused:", e)
        assert "error -1" in str(e) and "MI355ASR_GEMM16" in str(e), e
    else:
        raise AssertionError("the ragged call ran in the layer-at-a-time GEMM mode")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    name = sys.argv[1]
    globals()["step_" + name]()
    torch.cuda.synchronize()
    print("step %s ok" % name)
