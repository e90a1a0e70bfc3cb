"""The n-gram scorer of the CTC prefix beam search on the MI355X: the device `mi355asr_lm_score` and the device search with a
scorer against the host search (which tests/test_beam_lm_host.py pins to the reference's own decoder), bit for bit.

Every step (tests/beam_lm_gpu_steps.py, tests/beam_orders_gpu_steps.py) asserts which search each of its calls ran
(`beam_last_path`: the fallback to the host search returns the same arrays) and runs in a process of its own under its own time limit.  A step that ends in a fault,
an abort or its time limit is not run again, and no later step is started on the card: the remaining tests fail at once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_fault = []


def run_step(name, seconds, *args, script="beam_lm_gpu_steps.py"):
    assert not _fault, "not started: step %r ended with %s" % tuple(_fault[0])
    cmd = [sys.executable, os.path.join(HERE, script), name] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as e:
        _fault.append((name, "its time limit of %d s" % seconds))
        print(e.stdout)
        raise AssertionError("step %s did not finish in %d s" % (name, seconds))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _fault.append((name, "exit status %d" % r.returncode))
    assert r.returncode == 0, "step %s: exit status %d\n%s" % (name, r.returncode, r.stdout[-3000:])
    assert "step %s ok" % name in r.stdout


def test_device_lm_score_equals_the_host_bit_for_bit():
    run_step("lm_score", 300)


def test_device_search_equals_the_host_search_on_the_fixture_cases():
    run_step("fixtures", 300)


def test_device_search_on_the_config5_batch_with_and_without_a_scorer():
    run_step("config5", 600)


def test_calls_outside_the_device_limits_run_the_host_search():
    run_step("fallback", 300)


def test_chunk_beam_pipeline_with_a_scorer_equals_the_sequential_calls(tmp_path):
    run_step("pipeline", 300, tmp_path)


def test_chunk_asr_beam_width_4_with_lm_config(tmp_path):
    run_step("chunk_asr", 300, tmp_path)


# ---- tests/beam_orders_gpu_steps.py: orders 1, 2, 5, 6 and hashed keys, the widths where the kernels change, the class limit ----
def test_device_search_at_lm_orders_1_2_5_6_and_with_hashed_table_keys():
    run_step("orders", 300, script="beam_orders_gpu_steps.py")


def test_device_search_at_the_beam_widths_and_candidate_counts_where_the_kernels_change():
    run_step("widths", 300, script="beam_orders_gpu_steps.py")


def test_one_key_per_thread_kernel_has_tied_frames_redone_by_the_radix_path():
    run_step("redo", 120, script="beam_orders_gpu_steps.py")


def test_device_search_at_its_class_limit_and_the_host_search_one_class_above():
    run_step("class_limit", 300, script="beam_orders_gpu_steps.py")
