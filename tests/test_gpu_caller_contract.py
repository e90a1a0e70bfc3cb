"""The caller contract of the C ABI (include/mi355asr.h, "Conventions") on the MI355X: caller-owned workspaces, outputs and
opaque state may hold anything on entry, nothing is written outside them, and everything is enqueued on the caller's stream.

Every entry point runs three times -- on zero-filled and on 0xFF-filled fenced allocations (tests/fence.py) and on the dirty,
grown workspace a larger call left behind -- and must return the same bits, leave every guard intact, allocate exactly the
bytes its size query answered and sit within its family's bound of its reference.  The stream steps run every family on a
side stream behind a long delay, and two handles at once from one and from two threads.

Every step (tests/caller_contract_gpu_steps.py) runs in a process of its own under its own time limit.  A step that ends in a
fault, an abort or its time limit is not run again, and no later step is started on the card: the remaining tests fail at once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_fault = []


def run_step(name, seconds, *args):
    assert not _fault, "not started: step %r ended with %s" % tuple(_fault[0])
    cmd = [sys.executable, os.path.join(HERE, "caller_contract_gpu_steps.py"), name] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as e:
        _fault.append((name, "its time limit of %d s" % seconds))
        print(e.stdout)
        raise AssertionError("step %s did not finish in %d s" % (name, seconds))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _fault.append((name, "exit status %d" % r.returncode))
    assert r.returncode == 0, "step %s: exit status %d\n%s" % (name, r.returncode, r.stdout[-4000:])
    assert "step %s ok" % name in r.stdout


# ---- poisoned, fenced buffers ------------------------------------------------------------------------------------------------
def test_conformer_ctc_144_in_every_block_regime_and_ragged():
    run_step("encoder144", 240)


def test_offline_stt_batch_ragged(tmp_path):
    run_step("offline_stt_batch", 120, tmp_path)


def test_ctc_decoder_256_layers_ring_rows_resident_and_ragged():
    run_step("ctc256", 180)


def test_streaming_encoder_256_bf16_and_fp32():
    run_step("stream256", 120)


def test_translator_and_its_ragged_form():
    run_step("translator", 120)


def test_leaf_add_wav_info_and_spectrogram_frontends():
    run_step("frontends", 120)


def test_chunk_conformer_predict_with_stages():
    run_step("chunk_predict", 120)


def test_chunk_conformer_single_stream_calls():
    run_step("chunk_single_stream", 120)


def test_chunk_conformer_batched_streams_on_a_poisoned_state():
    run_step("chunk_streams", 180)


def test_ctc_loss_gradient_and_forced_alignment():
    run_step("lattice", 180)


def test_greedy_decode_and_frame_argmax():
    run_step("greedy_argmax", 120)


def test_device_prefix_beam_search():
    run_step("beam", 120)


def test_beam_streams_on_a_poisoned_state():
    run_step("beam_streams", 120)


def test_vad_scores_and_enhancement():
    run_step("vad_enhance", 120)


def test_resampler_and_stream_resampler_on_a_poisoned_state():
    run_step("resample", 120)


def test_stream_histories():
    run_step("histories", 120)


# ---- streams and handles -----------------------------------------------------------------------------------------------------
def test_side_stream_equals_default_stream_models():
    run_step("side_stream_models", 240)


def test_side_stream_equals_default_stream_chunk_conformer():
    run_step("side_stream_chunk", 240)


def test_side_stream_equals_default_stream_decoding_vad_resampling_histories():
    run_step("side_stream_decoding", 240)


def test_two_handles_in_flight_from_one_and_from_two_threads():
    run_step("two_handles", 240)
