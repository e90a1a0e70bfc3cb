"""The dmodel-144 block kernels on both of their paths against the float64 oracle, at row counts with a tile remainder.

The small-batch kernels (fused_ns.hip) and the pair-pipelined ones (fused_pp.hip) share the activation + operand-split schedule
(prep2_sched.inc) and the operand split of common.h.  One process per path, because the switches are read once per process:
the defaults (3 x 250 and 3 x 70 rows run on the small-batch kernels) and MI355ASR_SMALL_M=0 MI355ASR_NS1_MAX_M=0 (the
pair-pipelined kernels at any row count).  T = 70 is one full 64-frame tile plus a remainder of 6 rows; T = 250 is the
benchmark's utterance length.  The references are computed once and shared by both processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import co, small_cfg, waves

pytestmark = pytest.mark.gpu
TOL = 1e-3                      # the project's contract against the float64 oracle
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((250, 160000), (70, 44800))          # (encoder frames T, samples L with out_frames(L) = T)

CODE = r'''
import sys, numpy as np
sys.path.insert(0, "tests")
from helpers import co, encoder_kwargs, maxdiff, small_cfg, waves
from tensorflowasr_amd.models import ConformerEncoder
ref = np.load(sys.argv[1])
cfg = small_cfg(2)
w = co.encoder_weights(cfg, seed=3)
e = ConformerEncoder(**encoder_kwargs(cfg)); e.load_weights(w, by_name=False)
for T, L in ((250, 160000), (70, 44800)):
    blk = maxdiff(e.conformer_block(1, ref["x%d" % T]).cpu().numpy(), ref["blk%d" % T])
    got = e(waves(3, L, 11)).cpu().numpy()
    assert got.shape == ref["enc%d" % T].shape, (got.shape, ref["enc%d" % T].shape)
    enc = maxdiff(got, ref["enc%d" % T])
    print("RESULT %d %.3e %.3e" % (T, blk, enc))
'''


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    cfg = small_cfg(2)
    w = co.encoder_weights(cfg, seed=3)
    rng = np.random.default_rng(5)
    out = {}
    for T, L in SHAPES:
        x = rng.standard_normal((3, T, 144)).astype(np.float32)
        out["x%d" % T] = x
        out["blk%d" % T] = co.conformer_block(x.astype(np.float64), w, "conformer_block_1", 36)
        out["enc%d" % T] = co.conformer_encoder(waves(3, L, 11).astype(np.float64), w, cfg)
        assert out["enc%d" % T].shape == (3, T, 144)
    path = str(tmp_path_factory.mktemp("block_paths") / "ref.npz")
    np.savez(path, **out)
    return path


@pytest.mark.parametrize("path", ["small-batch", "pair-pipelined"])
def test_block_and_encoder_vs_oracle_on_each_path(references, path):
    extra = {} if path == "small-batch" else {"MI355ASR_SMALL_M": "0", "MI355ASR_NS1_MAX_M": "0"}
    env = {k: v for k, v in os.environ.items() if k not in ("MI355ASR_SMALL_M", "MI355ASR_NS1_MAX_M")}
    out = subprocess.run([sys.executable, "-c", CODE, references], env=dict(env, **extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert len(lines) == len(SHAPES), (path, out.stdout[-1000:], out.stderr[-2000:])
    for (T, blk, enc), (T_want, _) in zip(lines, SHAPES):
        print("%s T=%s: block max|d| = %s, encoder max|d| = %s" % (path, T, blk, enc))
        assert int(T) == T_want
        assert float(blk) < TOL and float(enc) < TOL, (path, T, blk, enc)
