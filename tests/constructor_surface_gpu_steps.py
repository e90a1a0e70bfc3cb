"""The fresh-process legs of tests/test_gpu_constructor_surface.py (the switches they set are read once per process):
python constructor_surface_gpu_steps.py <step>.  A step prints `SURFACE ...` lines and ends with `step <name> ok`."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from surface_yardstick import Ledger, waveform_case  # noqa: E402


def step_ring():
    """dmodel 128 (4 x 32, kernel size 9) and 384 (8 x 48, kernel size 32) from the waveform, under whatever MI355ASR_RING_* /
    MI355ASR_GEMM_RING the parent set"""
    led = Ledger("ring[%s]" % ",".join("%s=%s" % (k[9:], v) for k, v in sorted(os.environ.items()) if k.startswith("MI355ASR_RING_") or k == "MI355ASR_GEMM_RING"))
    waveform_case(led, "128 4x32 k9", 128, 4, 32, 9, 2, 16000)
    waveform_case(led, "384 8x48 k32", 384, 8, 48, 32, 2, 41600)
    led.close()


if __name__ == "__main__":
    name = sys.argv[1]
    {"ring": step_ring}[name]()
    print("step %s ok" % name)
