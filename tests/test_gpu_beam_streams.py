"""The stateful device beam search for many live streams on the MI355X (`mi355asr_beam_streams_*`, `BeamStreams`, the beam of
`ChunkStreamingServer`) against the host search, bit for bit.

Every step (tests/beam_streams_gpu_steps.py) asserts that its device calls ran a stream kernel (`beam_last_path`) and runs in a
process of its own under its own time limit.  A step that ends in a fault, an abort or its time limit is not run again, and no
later step is started on the card: the remaining tests fail at once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_fault = []


def run_step(name, seconds, *args, script="beam_streams_gpu_steps.py"):
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


def test_recorded_stateful_cases_in_their_pieces_among_other_streams():
    run_step("fixtures", 300)


def test_random_ticks_equal_the_host_decoders_and_the_slot_alone():
    run_step("ticks", 300)


def test_peek_equals_the_host_fork_and_leaves_nothing_behind():
    run_step("peek", 300)


def test_reset_and_capacity_with_a_guard_behind_the_arena():
    run_step("reset_capacity", 120)


def test_64_streams_of_the_text_heads_9160_classes():
    run_step("vocab9160", 300)


def test_chunk_streaming_server_with_the_device_beam(tmp_path):
    run_step("server", 600, tmp_path)
