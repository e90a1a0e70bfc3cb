"""The plain dmodel-256 / 512 paths (ConformerM, ConformerL, the streaming configuration's global CTC decoder) at every row count
where a dense layer changes kernel family or a grid gains a partial row tile, against the float64 oracle.

A dense layer runs on the fp32 chain kernels, on the per-wave gemm16 kernels or on gemm_ring_kernel (csrc/gemm_ring.hip), by the
handle and the row count; inside the ring launcher a cost model picks 128 or 256 rows per workgroup, the column chunks per
workgroup, the ring depth and, for the class head, the number of class ranges.  The tables of tests/dense_edges.py put a row
count on and next to every 128- and 256-row workgroup edge, on 1 499 | 1 500 | 1 501 where a row changes family, and run the
forced launch shapes on grids of two to four row workgroups whose last one holds a single row; the family is asserted from
mi355asr_profile_schemes after every call, so a launcher that declines and falls back fails.  B: the ring class head with 5 ..
1 332 classes (one chunk exactly, one class in a second chunk, an odd row stride, 11 chunks in one to four ranges).  C: the
subsampling conv of dmodel 256 / 512 (column chunks of 128 on the grid) at every parity of both convs' SAME padding and with
T2 x 20 positions on both sides of 128 and 256.

Every fp32 comparison goes through surface_yardstick.Ledger: the 1e-3 contract and max(8 x E32, 16 ulp of max|ref|), E32 being the
oracle's own float32 error on the same input.  Arg-max: only frames the oracle decides by more than 1e-3 count, and at most
0.5 % of a case's frames may be undecided (asserted on the host from the oracle alone, tests/test_dense_edges_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_edges as de
import dense_edges_gpu_steps as steps
from ragged_edges import COMBOS, L_for
from surface_yardstick import Ledger, waveform_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module", autouse=True)
def shared_dir(tmp_path_factory):
    """oracle results (read by the fresh-process legs instead of computing them again) and the raw outputs the legs leave"""
    d = tmp_path_factory.mktemp("dense_edges")
    os.environ["DENSE_EDGES_ORACLE_DIR"] = str(d)
    yield str(d)
    os.environ.pop("DENSE_EDGES_ORACLE_DIR", None)


_fault = []


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(torch_cuda):
    """a HIP error is sticky: once the device has faulted (here, or in a leg's own process) no later test launches anything"""
    assert not _fault, "not started: %s ended with %s" % tuple(_fault[0])
    yield
    try:
        torch_cuda.cuda.synchronize()
    except Exception as e:
        _fault.append(("an earlier test of this file", str(e)[:300]))
        raise


def _run_leg(name, seconds, shared_dir):
    """a leg of dense_edges_gpu_steps.py in a process of its own under its own time limit; one that ends in a signal, an abort or
    its limit is not run again and nothing is started after it -> what it saved"""
    out = os.path.join(shared_dir, "leg_%s.npz" % name)
    cmd = [sys.executable, os.path.join(HERE, "dense_edges_gpu_steps.py"), name, out]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds, env=dict(os.environ, **de.LEGS[name]))
    except subprocess.TimeoutExpired as e:
        _fault.append((name, "its time limit of %d s" % seconds))
        print(e.stdout)
        raise AssertionError("leg %s did not finish in %d s" % (name, seconds))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _fault.append((name, "exit status %d" % r.returncode))
    assert r.returncode == 0, "leg %s: exit status %d\n%s" % (name, r.returncode, r.stdout[-3000:])
    assert "step %s ok" % name in r.stdout
    return dict(np.load(out)) if os.path.exists(out) else {}


def _saved(shared_dir, names):
    """what the named legs saved; a leg that did not run (or failed before saving) fails the comparison"""
    res = {}
    for name in names:
        path = os.path.join(shared_dir, "leg_%s.npz" % name)
        assert os.path.exists(path), "leg %s left no output: run the whole file" % name
        res[name] = dict(np.load(path))
    return res


# ---- A. the dense families over the row count -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", de.DMODELS)
def test_project_and_head_over_the_row_count(d):
    """n = 0: project (E16_BIAS) + head (E16_HEAD) on [1, M, d] at every M of N0_M: gemm16 below 1 500 rows, the ring head from
    there with 12 .. 17 row workgroups of 128, the last one full, short by one and holding one row"""
    led = Ledger("n0")
    for M in de.N0_M:
        steps.run_dense_case(led, d, 0, M, "rings")
    led.close()


@pytest.mark.parametrize("M", list(de.N1_SHAPES))
@pytest.mark.parametrize("d", de.DMODELS)
def test_one_block_with_every_epilogue_over_the_row_count(d, M):
    """n = 1: SWISH, QKV, RES with and without the block LayerNorm, GLU and AFFSWISH next to the projection and the head, on
    [B, T, d] with B x T = M; 1 499 rows on gemm16, 1 500 and 1 501 on the ring"""
    led = Ledger("n1")
    steps.run_dense_case(led, d, 1, M, "rings")
    led.close()


def test_fp32_chains_of_a_handle_without_rings():
    """set_expected_rows(300) at dmodel 256: no slab rings are packed and the dense layers run on the fp32 chains, at M <= 385
    (up to 48 rows, MI355ASR_SMALL_M, such a handle too runs one gemm16 launch per layer: those rows repeat the default handle's)"""
    led = Ledger("chains")
    for M in [M for M in de.N0_M if M <= de.CHAIN_MAX_M]:
        steps.run_dense_case(led, 256, 0, M, "none", expected_rows=de.EXPECTED_ROWS)
    for M in [M for M in de.N1_SHAPES if M <= de.CHAIN_MAX_M]:
        steps.run_dense_case(led, 256, 1, M, "none", expected_rows=de.EXPECTED_ROWS)
    led.close()


def test_without_the_ring_above_the_crossover_in_a_fresh_process(shared_dir):
    """MI355ASR_GEMM_RING=0 at 1 500 and 2 049 rows: the route test_ring_gemm_at_16000_rows_... uses as its reference"""
    _run_leg("ring_off", 300, shared_dir)


@pytest.mark.parametrize("shape", list(de.FORCED_SHAPES))
def test_forced_ring_shapes_on_grids_with_a_partial_last_row_workgroup(shape, shared_dir):
    """MI355ASR_RING_MIN_M=1 with one launch shape forced: 129 / 257 / 385 rows, n = 0 and n = 1, dmodel 256 and 512, each against
    the oracle and on the ring (a declined launch -- go() returns -1 for two row tiles with a two-slot ring -- would report F32)"""
    _run_leg("forced_" + shape, 300, shared_dir)


def test_forced_ring_shapes_are_bit_identical(shared_dir):
    """A row's accumulators see the same k-steps in the same order and the same term order whatever the launch shape: RT only
    adds accumulators (the MFMA loop's innermost index), CPW walks the chunks one after the other with the operand steps
    wrapping to the same values, SLOTS changes only where a slab lies in LDS; the LayerNorm statistics are per row."""
    res = _saved(shared_dir, ["forced_" + k for k in de.FORCED_SHAPES])
    first = res["forced_rt1"]
    assert len(first) == 2 * 2 * 2 * len(de.FORCED_M)
    for name, r in res.items():
        assert sorted(r) == sorted(first), name
        for k in first:
            assert np.array_equal(first[k].view(np.uint32), r[k].view(np.uint32)), (name, k, float(np.abs(first[k] - r[k]).max()))


@pytest.mark.parametrize("M", de.BF16_M)
def test_bf16_mode_against_the_rounding_oracle(M):
    """gemm_dtype = bfloat16, dmodel 256, one block: gemm16 / chain256 at 257 rows, the one-term ring from 1 500"""
    steps.run_bf16_case(256, 1, M)


def test_default_sweep_with_poisoned_workspaces_and_guarded_outputs(torch_cuda):
    """the sweep of the first two tests inside fence.fenced(0xFF): every workspace and output holds NaN before the call and sits
    between guards; the outputs are finite (and within the bound), no guard byte is written -- nothing past row M - 1"""
    from fence import fenced
    led = Ledger("fenced")
    with fenced(0xFF) as f:
        for d in de.DMODELS:
            for M in de.N0_M:
                steps.run_dense_case(led, d, 0, M, "rings", fence=f)
            for M in de.N1_SHAPES:
                steps.run_dense_case(led, d, 1, M, "rings", fence=f)
        torch_cuda.cuda.synchronize()
        assert len(f.allocations) >= 3 * 2 * (len(de.N0_M) + len(de.N1_SHAPES))          # logits, arg-max and a workspace per call
        f.check()
    led.close()


# ---- B. the class head over the class count -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", de.HEAD_V)
def test_class_head_over_the_class_count(V):
    """dmodel 256, n = 0, 257 rows (gemm16 head) and 1 501 rows (ring head, 12 row workgroups, 93 rows in the last): V = 128 is
    one chunk exactly, 129 puts one class in a second chunk, 201 makes the row stride odd (element-wise stores), 1 332 is 11
    chunks in several ranges; with logits and with return_logits=False (the same arg-max, bit for bit)"""
    led = Ledger("head")
    for M in de.HEAD_M:
        _, am = steps.run_dense_case(led, 256, 0, M, "rings", V=V)
        _, am0 = steps.run_dense_case(led, 256, 0, M, "rings", V=V, return_logits=False)
        led.expect(np.array_equal(am, am0), "V%d M%d: the arg-max without logits differs from the one with" % (V, M))
    led.close()


@pytest.mark.parametrize("ranges", de.HEAD_RANGES)
def test_ring_head_of_1332_classes_in_forced_ranges(ranges, shared_dir):
    """MI355ASR_RING_HEAD_RANGES = 1 .. 4 (with 4 the last range holds two chunks) on the ring at 257 and 1 501 rows"""
    _run_leg("ranges%d" % ranges, 300, shared_dir)


def test_ring_head_ranges_are_bit_identical_to_one_range(shared_dir):
    res = _saved(shared_dir, ["ranges%d" % n for n in de.HEAD_RANGES])
    one = res["ranges1"]
    assert len(one) == 3 * len(de.HEAD_M)
    for name, r in res.items():
        for k in one:
            assert np.array_equal(one[k].view(np.uint32), r[k].view(np.uint32)), (name, k)
    for M in de.HEAD_M:
        assert np.array_equal(one["M%d_am" % M], one["M%d_am_nologits" % M])


# ---- C. the subsampling conv at dmodel 256 / 512 --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", de.DMODELS)
def test_conv_subsampling_at_every_padding_parity_and_position_tile_edge(d):
    """caller-supplied features [3, F, 80] in [-80, 0]: the three-term subconv_split_ring_kernel<., d, 8>"""
    led = Ledger("subconv")
    steps.run_subconv(led, d, de.BF16X3)
    led.close()


@pytest.mark.parametrize("leg", list(de.SUBCONV_LEGS))
def test_conv_subsampling_two_term_in_a_fresh_process(leg, shared_dir):
    """MI355ASR_SUBCONV_TERMS=22 sends caller-supplied features through the two-term kernel; with one and with two row tiles per wave"""
    _run_leg("subconv_" + leg, 300, shared_dir)


def test_conv_subsampling_row_tiles_per_wave_are_bit_identical(shared_dir):
    res = _saved(shared_dir, ["subconv_terms22_rt1", "subconv_terms22_rt2", "subconv_terms22"])
    a, b, c = res["subconv_terms22_rt1"], res["subconv_terms22_rt2"], res["subconv_terms22"]
    assert len(a) == len(de.DMODELS) * len(de.SUBCONV_F)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, float(np.abs(a[k] - b[k]).max()))
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k           # (the launcher's own choice is one of the two)


@pytest.mark.parametrize("d,T,combo", [(d, T, c) for d in de.DMODELS for T, c in de.WAVE_CASES[d]])
def test_from_the_waveform_at_17_and_33_frames(d, T, combo):
    led = Ledger("waveform")
    frames = waveform_case(led, "d%d T%d combo%d" % (d, T, combo), d, de.HEADS[d], 64, 32, 2, L_for(T, *COMBOS[combo]))
    assert frames == T
    led.close()
