"""HIP-event timing of the far-field kernels (csrc/augment.hip) beside what a user would write without them.

    python tools/time_augment.py [--regions 5] [--iters 5] [--json out.json]

The benchmark batch, 64 x 10 s at 16 kHz, with SignalRIR's 4096-tap responses.  Each of generation (64 responses of the default
room), convolution (a filter per row) and mixing on its own, the inputs already on the device; the FarField chain as a whole
(its host draws and uploads included, wall clock until the output is complete); the convolution against an FFT convolution
with torch.fft on the same device (rfft of both operands at the full output length, product, irfft -- no overlap, no tuning);
and generation plus convolution against the float64 NumPy oracle of tests/augment_ref.py plus scipy.signal.convolve on the host
(one utterance, times 64).  3 warm-up calls, then `regions` timed regions of `iters` back-to-back calls bracketed by events on
the launch stream: min / median / max milliseconds per call.  The convolution's FLOP are 2 L K per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32_MATRIX_TFLOPS = 157.3


def timed(call, stream, regions, iters):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    per = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            call()
        e1.record(stream)
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / iters)
    per.sort()
    return per[0], float(np.median(per)), per[-1]


def main():
    import torch
    import augment_ref as ar
    from tensorflowasr_amd.augment import AddNoise, FarField, ImageSourceRIR, Reverb
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(0)
    B, L, K, fs = 64, 160000, 4096, 16000
    rows = []

    def report(what, t, **more):
        rows.append(dict(what=what, ms_min=t[0], ms_median=t[1], ms_max=t[2], **more))
        print("%-34s min %.4f  median %.4f  max %.4f ms/call  %s"
              % (what, t[0], t[1], t[2], "  ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in more.items())))

    gen = ImageSourceRIR(fs)
    room = np.asarray(gen.room)
    src = np.round(rng.uniform(0.05, 0.95, (B, 3)) * room, 1)
    rec = np.round(rng.uniform(0.05, 0.95, (B, 3)) * room, 1)
    rec[(src == rec).all(1)] += 0.1
    report("generate 64 x 4096 (hp on)", timed(lambda: gen.generate(src, rec), stream, a.regions, a.iters))
    h = gen.generate(src, rec)
    xh = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    rv = Reverb()
    t = timed(lambda: rv(x, lens, h), stream, a.regions, a.iters)
    flop = 2.0 * B * L * K
    report("convolve 64 x 10 s, K = 4096", t, gflop=flop / 1e9, tflops_median=flop / (t[1] * 1e-3) / 1e12,
           share_of_f32_matrix_peak=flop / (t[1] * 1e-3) / 1e12 / F32_MATRIX_TFLOPS)

    n_fft = L + K - 1

    def fft_conv():
        return torch.fft.irfft(torch.fft.rfft(x, n=n_fft) * torch.fft.rfft(h, n=n_fft), n=n_fft)
    tf = timed(fft_conv, stream, a.regions, a.iters)
    y, _ = rv(x, lens, h)
    yf = fft_conv()
    y64 = np.convolve(xh[0].astype(np.float64), h[0].cpu().numpy().astype(np.float64))
    report("torch.fft convolution, same batch", tf, n_fft=n_fft, kernel_over_fft=t[1] / tf[1],
           fft_max_err=float(np.abs(yf[0].cpu().numpy() - y64).max()), kernel_max_err=float(np.abs(y[0].cpu().numpy() - y64).max()))

    noise = torch.from_numpy(rng.standard_normal((B, n_fft)).astype(np.float32)).cuda()
    snr = rng.integers(0, 15, B).astype(np.float32)
    mix = AddNoise()
    out_len = lens + (K - 1)
    tm = timed(lambda: mix(y, out_len, noise, snr, quantise=True), stream, a.regions, a.iters)
    nbytes = B * n_fft * 4 * 5                          # x and d read twice, y written
    report("mix + quantise 64 x 10.26 s", tm, gbs_median=nbytes / (tm[1] * 1e-3) / 1e9)

    bank = [rng.standard_normal(16000 * s).astype(np.float32) for s in (3, 7, 20)]
    ff = FarField(gen, noise_bank=bank, snr=(0, 15))
    ff(xh, None, np.random.default_rng(1))
    torch.cuda.synchronize()
    walls = []
    for i in range(3):
        t0 = time.perf_counter()
        ff(x, lens, np.random.default_rng(2 + i))
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    report("FarField chain, wall, x on device", (walls[0], walls[1], walls[2]), kernels_sum_ms=rows[0]["ms_median"] + t[1] + tm[1])

    t0 = time.perf_counter()
    h64, _ = ar.rir(gen.room, src[0], rec[0], gen.c, fs, K, reverberation_time=gen.reverberation_time, hp_filter=True)
    t_gen = (time.perf_counter() - t0) * 1e3
    from scipy import signal
    t0 = time.perf_counter()
    signal.convolve(xh[0].astype(np.float64), h64, mode="full")
    t_conv = (time.perf_counter() - t0) * 1e3
    dev = rows[0]["ms_median"] + t[1]
    report("host oracle + scipy, one utterance", (t_gen + t_conv,) * 3, oracle_ms=t_gen, scipy_convolve_ms=t_conv,
           times_64_ms=64 * (t_gen + t_conv), device_generate_plus_convolve_ms=dev, ratio=64 * (t_gen + t_conv) / dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
