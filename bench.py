"""Headline benchmark: audio-frames/s of the ConformerCTC(S) hot path (waveform -> CTC greedy token ids) on
N MI355X GPUs, one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" = one pass of mi355asr_recognize over one batch of 64 synthetic 10-second utterances per GPU that are
already resident in HBM (BASELINE.json configs[1]; weak scaling: 64 utterances per GPU at every N), followed --
when N > 1 -- by the all_gather of the token ids.  1 audio frame = one 10 ms feature hop (am_data.yml:8), so a
10 s utterance is 1000 frames.  Rank 0 prints ONE JSON line.

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned to its caller as DIR/<name>.npy
(float64; the inputs are seeded, so two builds run with the same arguments can be compared output for output).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from tensorflowasr_amd import _lib  # noqa: E402
from tensorflowasr_amd.models import ConformerCTC  # noqa: E402
from tensorflowasr_amd.synthetic import synth_batch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2_f32, 256 CUs @ 2.4 GHz
# Kernels that compute fp32 products as six bf16 MFMAs (operands split into three bf16 terms: subconv.hip, leaf.hip)
# are priced against the dense bf16 MFMA peak (~2.5 PFLOP/s) / 6, in fp32-equivalent (algorithmic) FLOP/s.
PEAK_SPLIT3_TFLOPS = 2500.0 / 6.0
# two-term scheme: fp32 operands as hi + lo fp16 terms, three fp16 MFMAs per product (the fp16 dense peak is the bf16 one)
PEAK_HALF2_TFLOPS = 2500.0 / 3.0


PEAK_BF16_TFLOPS = 2500.0      # dense bf16 / fp16 MFMA (MI355X_MICROARCH.md)
# operand scheme (include/mi355asr.h MI355ASR_SCHEME_*) -> (peak in fp32-equivalent TFLOP/s, what the kernel executes).
# The scheme of every kernel category comes from the LIBRARY (mi355asr_profile_schemes: recorded by the launcher that chose
# the kernel variant), not from this script's reading of the environment.
SCHEME_PEAK = {0: (PEAK_FP32_MFMA_TFLOPS, "fp32 MFMA"),
               1: (PEAK_SPLIT3_TFLOPS, "bf16 MFMA x6 (fp32 operands as three bf16 terms)"),
               2: (PEAK_HALF2_TFLOPS, "fp16 MFMA x3 (fp32 operands as two fp16 terms)"),
               3: (PEAK_BF16_TFLOPS, "bf16 MFMA (operands rounded to bf16)")}
SCHEME_NAME = {0: "f32", 1: "bf16x3", 2: "f16x2", 3: "bf16", -1: "not run"}


def read_schemes(lib, h):
    """{kernel category: MI355ASR_SCHEME_*} of the last launch of each category on this handle"""
    nk = len(_lib.KERNEL_NAMES)
    out = (ctypes.c_int32 * nk)()
    _lib.check(lib.mi355asr_profile_schemes(h.ptr, out, nk))
    return {n: int(out[i]) for i, n in enumerate(_lib.KERNEL_NAMES)}


def kernel_peak(name, schemes):
    return SCHEME_PEAK[max(schemes.get(name, 0), 0)]


PEAK_HBM_GBS = 8000.0

S_CFG = dict(dmodel=144, reduction_factor=4, num_blocks=13, head_size=36, num_heads=4, kernel_size=32,
             fc_factor=0.5, sample_rate=16000, n_mels=80, stride_ms=10, ctcdecoder_num_blocks=1,
             ctcdecoder_kernel_size=32, ctcdecoder_fc_factor=0.5)
NUM_CLASSES = 1332    # pinyin vocabulary 1331 + blank (test_asr.py:180)


def algorithmic_flops(B, L, cfg=S_CFG, V=NUM_CLASSES, stft_mode=0, mel_nnz=None):
    """ALGORITHMIC flops per launch of each kernel category, counted as the reference computes the op
    (1 MAC = 2 flop).  The STFT is priced by what the selected kernel executes: the dense DFT conv
    the reference runs (time_frequency.py:108-115) for stft_mode 0, the two 32-point DFT stages of the 32x32
    Cooley-Tukey kernel for stft_mode 1 (8x fewer flops for the same spectrum -- not credited as dense flops).  The mel
    projection likewise: the banded kernel multiplies the non-zeros of freq2mel only (mel_nnz of 513 x 80)."""
    d, k, H = cfg["dmodel"], cfg["kernel_size"], cfg["num_heads"]
    F = -(-L // 160)
    T1 = -(-F // 2)
    T = -(-T1 // 2)
    F1, F2 = 40, 20
    M = B * T
    return {
        "stft": 2.0 * 2 * B * F * 1024 * 513 if stft_mode == 0 else 2.0 * B * F * (32 * 32 * 64 + 32 * 64 * 32),
        "utt_max": 0.0,
        "mel": 2.0 * B * F * (513 * 80 if mel_nnz is None else mel_nnz),
        "subconv": 2.0 * B * T1 * F1 * d * 9 + 2.0 * B * T * F2 * d * 9 * d,
        "sublinear": 2.0 * M * (F2 * d) * d,
        "ffn": 2.0 * 2 * M * d * 4 * d,
        "qkv": 3 * 2.0 * M * d * d,
        "attention": 2 * 2.0 * B * T * T * d,
        "attn_out": 2.0 * M * d * d,
        "pw1_glu": 2.0 * M * d * 2 * d,
        "dwconv": 2.0 * M * d * k,
        "conv_tail": 2.0 * M * d * 2 * d + 2.0 * M * 2 * d * d,
        "ctc_project": 2.0 * M * d * d,
        "ctc_head": 2.0 * M * d * V,
        "collapse": 0.0,
        # block-level fused kernels (dmodel 144): sums of the layers they contain
        "ff1_qkv": 2.0 * 2 * M * d * 4 * d + 3 * 2.0 * M * d * d,
        "out_glu": 2.0 * M * d * d + 2.0 * M * d * 2 * d,
        # (round 3: the depthwise conv runs in the prologue of the tail kernels -- its flops are theirs now; with
        # MI355ASR_PP_DW=0 it is a launch of its own again and the few per cent are counted twice)
        "tail_ff2": 2.0 * M * d * k + 2.0 * M * d * 2 * d + 2.0 * M * 2 * d * d + 2.0 * 2 * M * d * 4 * d,
        # tail_ff2 of one block + ff1_qkv of the next in one launch
        "tail_ff1": 2.0 * M * d * k + 2.0 * M * d * 2 * d + 2.0 * M * 2 * d * d + 2 * (2.0 * 2 * M * d * 4 * d) + 3 * 2.0 * M * d * d,
    }


def algorithmic_bytes(B, L, cfg=S_CFG, V=NUM_CLASSES):
    """ALGORITHMIC HBM bytes per launch of each kernel category: the fp32 tensors a kernel must read and write once
    (activations in + out, its weights once per launch); SURVEY 8d's stage-fused model, per kernel."""
    d, k = cfg["dmodel"], cfg["kernel_size"]
    F = -(-L // 160)
    T = -(-(-(-F // 2)) // 2)
    M = B * T
    act = 4.0 * M * d
    wb = lambda n: 4.0 * n
    return {
        "stft": 4.0 * B * L + 4.0 * B * F * 528, "mel": 4.0 * B * F * 528 + 4.0 * B * F * 80 + wb(513 * 80),
        "subconv": 4.0 * B * F * 80 + 4.0 * M * 20 * d + wb(9 * d + 9 * d * d), "sublinear": 4.0 * M * 20 * d + act + wb(20 * d * d),
        "ff1_qkv": act + act + 3 * act + wb(8 * d * d + 3 * d * d), "attention": 3 * act + act,
        "out_glu": act + act + act + act + wb(d * d + 2 * d * d), "dwconv": 2 * act + wb(k * d),
        "tail_ff2": 3 * act + wb(4 * d * d + 8 * d * d), "tail_ff1": 2 * act + act + 3 * act + wb(4 * d * d + 16 * d * d + 3 * d * d),
        "ctc_project": 2 * act + wb(d * d),
        "ctc_head": act + 4.0 * M + wb(d * V),
    }


def build_model(device, rank, world, use_dist=False):
    m = ConformerCTC(NUM_CLASSES, device=device, **S_CFG)
    m._build(seed=0)                       # Keras-default random init of the S architecture + DFT/mel constants
    w = m.get_weights_dict()
    golden = os.path.join(ROOT, "tests", "golden", "ctc_decoder_weights.npz")
    if os.path.exists(golden):             # trained CTCDecoder weights exported by the reference
        w.update({k: v for k, v in np.load(golden).items()})
    if use_dist:
        from tensorflowasr_amd.parallel import broadcast_weights
        w = broadcast_weights(w, src=0, device=device)
    m.load_weights(w, by_name=False)
    return m


PUBLISHED_TF2_1CORE = {"value": 1790.0, "unit": "audio-frames/s",
                       "note": "reference README RTF 0.056 on one CPU core (TF2, different hardware): published, not measured here"}


def _oracle_rate(co, x, w, cfg, seconds_budget, max_reps):
    reps, t_total = 0, 0.0
    while reps < 1 or (t_total < seconds_budget and reps < max_reps):
        t0 = time.perf_counter()
        enc = co.conformer_encoder(x, w, cfg, dtype=np.float32)
        logits = co.ctc_decoder(enc, w, cfg, dtype=np.float32)
        co.ctc_greedy(logits, [logits.shape[1]], NUM_CLASSES - 1)
        t_total += time.perf_counter() - t0
        reps += 1
    return 1000.0 * reps / t_total, reps, t_total


def cpu_baseline(seconds_budget=12.0):
    """The NumPy oracle (a port of the reference path; TensorFlow is not installed) timed on this host.  One 10 s utterance at
    a time is a small problem for a BLAS pool: on the 128-core GPU box every core made it SLOWER than one thread (round-4
    review).  So the pool is tried at 1, 8, 32 and all threads and the best is the baseline (`threads_best`); the one-thread
    figure is the one comparable to the README's single-core RTF."""
    from oracle import conformer_oracle as co          # checker only: never on the measured GPU path
    from threadpoolctl import threadpool_info, threadpool_limits
    cores = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    cfg = dict(co.CONFORMER_S)
    w = co.encoder_weights(cfg, seed=0)
    golden = os.path.join(ROOT, "tests", "golden", "ctc_decoder_weights.npz")
    w.update(dict(np.load(golden)) if os.path.exists(golden) else co.ctc_decoder_weights(cfg, NUM_CLASSES))
    x = co.synth_wave(0, 160000)[None]
    tries = sorted({t for t in (1, 8, 32, cores) if t <= cores})
    runs = {}
    for t in tries:
        with threadpool_limits(limits=t):
            v, r, tt = _oracle_rate(co, x, w, cfg, seconds_budget / len(tries), 4)
        runs[t] = {"value": round(v, 1), "threads": t, "sample": "%d x 1 utterance (10 s = 1000 frames), %.1f s" % (r, tt)}
    best = max(runs, key=lambda t: runs[t]["value"])
    one_at_a_time = {"value": runs[best]["value"], "cores": int(best),
                     "sample": "the fp32 NumPy oracle on one 10 s utterance at a time, BLAS pool limited to %s threads in turn (%s); best kept"
                               % (tries, "; ".join("%d: %s" % (t, runs[t]["sample"]) for t in tries))}
    # round-5 review: one utterance at a time does not scale with threads (3 202 -> 3 216 frames/s from 1 to 8 threads on a
    # 128-thread host), so it understates what the host can do.  A batch is embarrassingly parallel over utterances: the second
    # leg shards the benched batch over worker PROCESSES, one BLAS thread each, and the better of the two legs is the baseline.
    try:
        workers = cpu_baseline_workers()
    except Exception as e:                                   # the baseline must not take the bench line down
        workers = {"error": "%s: %s" % (type(e).__name__, e)}
    pick = workers if workers.get("value", 0.0) > one_at_a_time["value"] else one_at_a_time
    return {"value": pick["value"], "unit": "audio-frames/s", "cores": int(pick["cores"]), "kind": "port", "threads_best": int(best),
            "host_threads": int(cores), "sample": pick["sample"],
            "legs": {"one_utterance_at_a_time": one_at_a_time, "worker_processes": workers},
            "by_threads": {str(t): runs[t]["value"] for t in tries},
            "threads1": runs[1], "all_cores": runs[cores],
            "published_tf2_1core": PUBLISHED_TF2_1CORE}


def cpu_baseline_workers(timeout_s=240.0):
    """The benched batch sharded over min(host cores, 64) worker processes (oracle/cpu_worker.py: one BLAS thread each, the fp32
    NumPy oracle from the waveform to the greedy ids).  Timed from the moment every worker is ready (weights built, one warm-up
    utterance done) to the last worker's DONE: start-up is excluded, imbalance is not.  64 utterances when the host has at least
    32 cores, otherwise two per worker (a bounded sample)."""
    import subprocess
    ncpu = os.cpu_count() or 1
    try:
        ncpu = min(ncpu, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    n_workers = max(1, min(ncpu, 64))
    total = 64 if ncpu >= 32 else 2 * n_workers
    worker = os.path.join(ROOT, "oracle", "cpu_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(i), str(n_workers), str(total), "160000", str(NUM_CLASSES)],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
             for i in range(n_workers)]
    deadline = time.time() + timeout_s
    try:
        for p in procs:
            line = p.stdout.readline()
            if not line.startswith("READY") or time.time() > deadline:
                raise RuntimeError("worker did not get ready: %r" % line)
        t0 = time.perf_counter()
        for p in procs:
            p.stdin.write("go\n")
            p.stdin.flush()
        done, busy = 0, 0.0
        for p in procs:
            parts = p.stdout.readline().split()
            if len(parts) != 3 or parts[0] != "DONE":
                raise RuntimeError("worker failed: %r" % parts)
            done += int(parts[1])
            busy += float(parts[2])
        wall = time.perf_counter() - t0
    finally:
        for p in procs:
            try:
                p.stdin.close()
            except Exception:
                pass
            try:
                p.wait(timeout=5)
            except Exception:
                p.kill()
    if done != total:
        raise RuntimeError("workers ran %d of %d utterances" % (done, total))
    return {"value": round(total * 1000.0 / wall, 1), "cores": n_workers, "utterances": total, "wall_s": round(wall, 3),
            "cpu_busy_s": round(busy, 2),
            "sample": "%d of the benched 10 s utterances (1000 frames each) over %d worker processes, one BLAS thread each, fp32 NumPy oracle "
                      "waveform -> greedy ids; %.2f s wall (%.1f s of CPU work), start-up excluded" % (total, n_workers, wall, busy)}


def parity_stamp(model, wav, B, L):
    """The benched batch against the committed fixtures, recorded in the bench line (round-5 review, item 2c): logits of all 64
    utterances against tests/golden/tf_config2_b64.npz -- the REFERENCE'S OWN ConformerEncoder + CTCDecoder + ctc_decode on this
    very batch (tests/golden/make_tf_config2_b64.py; float32 run, and the float64-carried run for the margins) -- on the four
    largest classes of every frame and all classes of every 50th frame; per-frame arg-max; `excused_frames` = frames whose arg-max
    differs from the reference's where the reference's own top-2 margin is within ten times the measured logit error (the rule of
    tests/helpers.assert_frames_and_ids; any other differing frame is `decisive_mismatches`); the greedy ids of recognize() against
    the reference's ctc_decode.  Reads data only (no oracle code); outside every timed region."""
    path = os.path.join(ROOT, "tests", "golden", "tf_config2_b64.npz")
    if not (os.path.exists(path) and B == 64 and L == 160000):
        return None
    g = np.load(path)
    enc = model.encode(wav)
    logits, amax = model.ctc_logits(enc, return_argmax=True)
    ids, lens = model.recognize(wav)
    enc, logits, amax, ids, lens = (t.cpu().numpy() for t in (enc, logits, amax, ids, lens))
    idx, val = g["trained_top4_idx"].astype(np.int64), g["trained_top4_val"].astype(np.float64)
    err = max(float(np.abs(np.take_along_axis(logits, idx, -1) - val).max()),
              float(np.abs(logits[:, ::50].astype(np.float64) - g["trained_logits_every50"]).max()))
    ra = idx[..., 0]
    excused = decisive = 0
    for b, t in np.argwhere(amax != ra):
        pos = np.flatnonzero(idx[b, t] == amax[b, t])
        margin = float(val[b, t, 0] - val[b, t, pos[0]]) if pos.size else float("inf")
        if margin <= 10 * err:
            excused += 1
        else:
            decisive += 1
    ids_equal = bool(np.array_equal(lens, g["trained_lens"]) and np.array_equal(ids, g["trained_ids"]))
    return {"against": "tests/golden/tf_config2_b64.npz: the reference's own model code on this batch (%s)" % str(g["meta_generator"]),
            "frames": int(ra.size), "logits_max_abs_err": err,
            "encoder_max_abs_err_every10": float(np.abs(enc[:, ::10].astype(np.float64) - g["trained_enc_every10"]).max()),
            "excused_frames": excused, "decisive_mismatches": decisive, "greedy_ids_equal_reference_ctc_decode": ids_equal,
            "tokens": int(lens.sum()), "tolerance": 1e-3, "within_tolerance": bool(err < 1e-3 and decisive == 0)}


def length_sweep(model, device, total_s=640.0, lengths=(5.0, 10.0, 15.0, 20.0, 30.0), steps=10):
    """Round-5 review, item 3: no performance cliff past 10.24 s.  The headline model on utterances of 5 / 10 / 15 / 20 / 30 s at (about)
    constant total audio -- B = floor(640 s / length) utterances per step, waveform -> greedy ids, input resident in HBM.  Attention is
    the only part of the path whose work per frame grows with the length (T^2 per utterance); beyond 256 encoder frames it runs in key
    blocks with an online softmax (attention_split_long_kernel)."""
    out = []
    for sec in lengths:
        B, L = max(1, int(total_s / sec)), int(sec * 16000)       # (floor: 43 x 15 s would be 258 workgroups of the block kernels on 256 CUs)
        wav = torch.from_numpy(synth_batch(0, B, L)).to(device)
        model.prepare(B, L)
        t = _timed(lambda: model.recognize(wav, reuse_buffers=True), steps, warmup=3)
        out.append({"seconds": sec, "batch": B, "enc_frames": L // 640, "ms_per_step": round(t * 1e3, 3),
                    "frames_per_s": round(B * (L // 160) / t, 1)})
        del wav
    ref = next(r["frames_per_s"] for r in out if r["seconds"] == 10.0)
    for r in out:
        r["vs_10s"] = round(r["frames_per_s"] / ref, 3)
    return {"what": "ConformerCTC(S), waveform -> greedy ids, ~%g s of audio per step at every length, %d steps each" % (total_s, steps), "by_length": out}


def block_flops(M, B, T, d, k, nblocks):
    """ALGORITHMIC flops per step of the block-level categories of a stack of `nblocks` ConformerBlocks over M = B * T rows"""
    one = {"ffn": 2 * (2.0 * 2 * M * d * 4 * d), "qkv": 3 * 2.0 * M * d * d, "attention": 2 * 2.0 * B * T * T * d,
           "attn_out": 2.0 * M * d * d, "pw1_glu": 2.0 * M * d * 2 * d, "dwconv": 2.0 * M * d * k,
           "conv_tail": 2.0 * M * d * 2 * d + 2.0 * M * 2 * d * d}
    return {n: v * nblocks for n, v in one.items()}


def _read_profile(lib, h, nk, steps):
    ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    _lib.check(lib.mi355asr_profile_read(h.ptr, ms, cnt, nk, 1))
    return {n: (ms[i] / steps, cnt[i] // max(steps, 1)) for i, n in enumerate(_lib.KERNEL_NAMES) if cnt[i]}


def _timed(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def extra_config3(lib, device, steps=20, with_cpu=True):
    """BASELINE.json configs[2]: StreamingConformerCTC (d = 256, 4 blocks, k = 5; CTCDecoder 1 block, k = 32), 64 streaming
    chunks of 0.5 s per step, dense layers with bf16 operands: one encoder pass over the 64 new chunks + the reference's
    "global CTC" over 10 s of history per stream (conformer_blocks.py:574-594, :385-438) + greedy collapse."""
    from tensorflowasr_amd.models import CTCDecoder, StreamingConformerEncoder, ctc_greedy_decode
    B, chunk, hist, d, V = 64, 8000, 20, 256, NUM_CLASSES
    enc = StreamingConformerEncoder(dmodel=d, reduction_factor=4, num_blocks=4, head_size=64, num_heads=4, kernel_size=5,
                                    fc_factor=0.5, sample_rate=16000, n_mels=80, stride_ms=10,
                                    mel_layer_type="Melspectrogram", gemm_dtype="bfloat16", device=device)
    enc.add_chunk_size(chunk, 80, 640)
    enc._build(seed=0)
    ctc = CTCDecoder(num_classes=V, dmodel=d, num_blocks=1, head_size=64, num_heads=4, kernel_size=32, fc_factor=0.5,
                     gemm_dtype="bfloat16", device=device)
    ctc._build(seed=1)
    wav = torch.from_numpy(synth_batch(0, B, chunk)).to(device)
    history = torch.randn(B, hist * 13, d, device=device)

    def step():
        e = enc(wav)
        h = torch.cat([history[:, 13:], e], 1)
        _, amax = ctc(h, return_argmax=True, return_logits=False)      # greedy decode: the class head keeps its running argmax only
        return ctc_greedy_decode(amax, None, blank=V - 1)

    t = _timed(step, steps)
    nk = len(_lib.KERNEL_NAMES)
    for m in (enc, ctc):
        _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 1))
        torch.cuda.synchronize()
        _read_profile(lib, m._h, nk, 1)
    _timed(step, steps, warmup=0)
    pe, pc = _read_profile(lib, enc._h, nk, steps), _read_profile(lib, ctc._h, nk, steps)
    for m in (enc, ctc):
        _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 0))
    sch = {"enc": read_schemes(lib, enc._h), "ctc": read_schemes(lib, ctc._h)}
    # flops per step: encoder over 64 x 13 rows (frontend: 50 mel frames per chunk), CTCDecoder over 64 x 260 rows
    Me, Te, Mc, Tc = B * 13, 13, B * hist * 13, hist * 13
    fe = block_flops(Me, B, Te, d, 5, 4)
    fe["enc_stack"] = sum(fe.values())       # round 5: the four blocks as one launch (stream256.hip)
    fe.update({"stft": 2.0 * B * 50 * (32 * 32 * 64 + 32 * 64 * 32), "subconv": 2.0 * B * 25 * 40 * d * 9 + 2.0 * Me * 20 * d * 9 * d,
               "sublinear": 2.0 * Me * 20 * d * d})
    fc = block_flops(Mc, B, Tc, d, 32, 1)
    fc.update({"ctc_project": 2.0 * Mc * d * d, "ctc_head": 2.0 * Mc * d * V})
    kern = {}
    for tag, prof, fl in (("enc", pe, fe), ("ctc", pc, fc)):
        for n, (ms_step, launches) in prof.items():
            f = fl.get(n, 0.0)
            peak = kernel_peak(n, sch[tag])[0]
            kern[tag + "." + n] = {"launches_per_step": launches, "ms_per_step": round(ms_step, 4), "scheme": SCHEME_NAME[sch[tag].get(n, -1)],
                                   "tflops": round(f / (ms_step * 1e-3) / 1e12, 2) if f else None,
                                   "frac_of_peak": round(f / (ms_step * 1e-3) / 1e12 / peak, 4) if f else None}
    dom = max(kern, key=lambda n: kern[n]["ms_per_step"])
    dpeak = kernel_peak(dom.split(".")[1], sch[dom.split(".")[0]])[0]
    out = {"workload": "StreamingConformerCTC 15M, batch=64 streaming chunks of 0.5 s, bf16 MFMA operands, global CTC over 10 s of history",
           "dtype": "bf16 (GEMM operands; f32 accumulate, LayerNorm, softmax, frontend)", "steps": steps,
           "ms_per_step": round(t * 1e3, 3), "chunks_per_s": round(B / t, 1), "frames_per_s": round(B * 50 / t, 1),
           "rtf_per_stream": round(t / 0.5, 6),
           "roofline": {"bound": "mfma", "kernel": dom, "achieved": kern[dom]["tflops"], "peak": dpeak, "unit": "TFLOP/s",
                        "frac": kern[dom]["frac_of_peak"], "traffic": None,
                        "note": "categories are (handle).(layer kind) summed over their launches of one step; at 832 encoder rows "
                                "the step is launch- and latency-bound (DESIGN.md section 3, bf16 mode)"},
           "kernels": kern}
    if with_cpu:
        from oracle import conformer_oracle as co          # checker only: the CPU baseline leg
        cfg = dict(co.STREAMING_S)
        w = co.encoder_weights(cfg, seed=0)
        w.update(co.ctc_decoder_weights(cfg, V))
        x1 = co.synth_wave(0, chunk)[None]
        h1 = np.random.default_rng(0).standard_normal((1, Tc, d)).astype(np.float32)
        reps, tt = 0, 0.0
        while reps < 1 or (tt < 5.0 and reps < 6):
            t0 = time.perf_counter()
            co.streaming_conformer_encoder(x1, w, cfg, chunk, dtype=np.float32)
            lg = co.ctc_decoder(h1, w, cfg, dtype=np.float32)
            co.ctc_greedy(lg, [lg.shape[1]], V - 1)
            tt += time.perf_counter() - t0
            reps += 1
        out["cpu_baseline"] = {"value": round(50.0 * reps / tt, 1), "unit": "audio-frames/s", "kind": "port",
                               "cores": int(os.cpu_count() or 1),
                               "sample": "%d x (1 stream: one 0.5 s chunk through the encoder + CTCDecoder over 260 history frames), "
                                         "fp32 NumPy oracle, %.1f s total" % (reps, tt)}
    del enc, ctc
    return out


def extra_stt(lib, device, steps=10):
    """What `ASR.offline_stt` computes for a batch (test_asr.py:186-219): waveform -> encoder -> CTCDecoder -> greedy phone ids
    -> Translator([ids, encoder output]) -> text ids (argmax).  64 x 10 s, ConformerCTC(S) + the S Translator (2 RBlocks,
    Embedding(1332 -> 144), Dense(144 -> 9160): conformerS.yml:17-20), random-init weights; the blank bias of the CTC head is set
    so that 76 % of the frames are blank (what the reference's trained ctc_model.onnx does on noise): ~60
    phone tokens per utterance reach the Translator, as in speech.  Reported next to the headline, never as `value`."""
    from tensorflowasr_amd.models import ConformerEncoder, CTCDecoder, Translator, ctc_greedy_decode
    B, L, V, VT = 64, 160000, NUM_CLASSES, 9160
    enc_kw = {k: S_CFG[k] for k in ("dmodel", "reduction_factor", "num_blocks", "head_size", "num_heads", "kernel_size", "fc_factor",
                                    "sample_rate", "n_mels", "stride_ms")}
    enc = ConformerEncoder(mel_layer_type="Melspectrogram", device=device, **enc_kw)
    enc._build(seed=0)
    ctc = CTCDecoder(num_classes=V, dmodel=144, num_blocks=1, head_size=36, num_heads=4, kernel_size=32, fc_factor=0.5, device=device)
    ctc._build(seed=1)
    tr = Translator(inp_classes=V, tar_classes=VT, dmodel=144, num_blocks=2, head_size=36, num_heads=4, kernel_size=32, fc_factor=0.5,
                    device=device)
    tr._build(seed=2)
    wav = torch.from_numpy(synth_batch(0, B, L)).to(device)
    # blank bias: 76 % blank frames
    e0 = enc(wav)
    lg = ctc(e0)
    others = lg[..., :V - 1].max(-1).values
    q = torch.quantile((others - lg[..., V - 1]).flatten().float().cpu(), 0.76).item()
    w = ctc.get_weights_dict()
    w["fully_connected/bias"] = w["fully_connected/bias"].copy()
    w["fully_connected/bias"][V - 1] += q
    ctc.load_weights(w, by_name=False)
    del e0, lg, others

    def step():
        e = enc(wav)
        _, fr = ctc(e, return_argmax=True, return_logits=False)
        ids, lens = ctc_greedy_decode(fr, None, blank=V - 1)
        width = int(lens.max().item())                     # ASR._phone_ids: ctc_decode's dense width (a host sync, as in the reference)
        ph = ids[:, :width].clamp_(min=0).contiguous()
        _, txt = tr([ph, e], return_argmax=True, return_logits=False)      # as ASR.offline_stt: the text ids only
        return ph, lens, txt

    ph, lens, txt = step()
    t = _timed(step, steps)
    nk = len(_lib.KERNEL_NAMES)
    _lib.check(lib.mi355asr_profile_enable(tr._h.ptr, 1))
    torch.cuda.synchronize()
    _read_profile(lib, tr._h, nk, 1)
    _timed(step, steps, warmup=0)
    pt = _read_profile(lib, tr._h, nk, steps)
    _lib.check(lib.mi355asr_profile_enable(tr._h.ptr, 0))
    U = int(ph.shape[1])
    Mt, d, T = B * U, 144, L // 640
    # Translator flops per step (2 RBlocks over B x U rows; cross-attention keys / values from the B x T encoder rows)
    fl = {"ffn": 2 * 2 * (2.0 * 2 * Mt * d * 4 * d), "qkv": 2 * (2.0 * Mt * d * d + 2 * 2.0 * B * T * d * d), "attention": 2 * 2 * 2.0 * B * U * T * d,
          "attn_out": 2 * 2.0 * Mt * d * d, "pw1_glu": 2 * 2.0 * Mt * d * 2 * d, "dwconv": 2 * 2.0 * Mt * d * 32,
          "conv_tail": 2 * (2.0 * Mt * d * 2 * d + 2.0 * Mt * 2 * d * d), "ctc_head": 2.0 * Mt * d * VT}
    sch = read_schemes(lib, tr._h)
    kern = {}
    for n, (ms_step, launches) in pt.items():
        f = fl.get(n, 0.0)
        peak = kernel_peak(n, sch)[0]
        kern[n] = {"launches_per_step": launches, "ms_per_step": round(ms_step, 4), "scheme": SCHEME_NAME[sch.get(n, -1)],
                   "tflops": round(f / (ms_step * 1e-3) / 1e12, 2) if f else None,
                   "frac_of_peak": round(f / (ms_step * 1e-3) / 1e12 / peak, 4) if f else None}
    ms_tr = sum(v["ms_per_step"] for v in kern.values())
    dom = max(kern, key=lambda n: kern[n]["ms_per_step"]) if kern else None
    out = {"workload": "ASR.offline_stt for a batch: 64 x 10 s, encoder + CTCDecoder + greedy ids + Translator (2 RBlocks, 144 -> 9160) -> text ids",
           "steps": steps, "ms_per_step": round(t * 1e3, 3), "frames_per_s": round(B * (L // 160) / t, 1),
           "phone_tokens_per_utt": round(float(lens.float().mean().item()), 1), "translator_rows": Mt, "translator_width": U,
           "ms_translator_kernels": round(ms_tr, 4),
           "roofline": {"bound": "mfma", "kernel": "translator." + dom if dom else None, "achieved": kern[dom]["tflops"] if dom else None,
                        "peak": kernel_peak(dom, sch)[0] if dom else None, "unit": "TFLOP/s", "frac": kern[dom]["frac_of_peak"] if dom else None,
                        "traffic": None},
           "translator_kernels": kern}
    del enc, ctc, tr
    return out


def extra_config5(lib, device, steps=5, with_cpu=True):
    """BASELINE.json configs[4] per GPU: ChunkConformer `predict` (front, 15-block band-attention encoder, phone picker,
    feature_pick, context helper, text decoder: chunk_conformer_blocks.py:815-822) over 16 x 30 s utterances + CTC prefix
    beam search (beam 10, cutoff_top_n 40) of the text logits on the device."""
    from tensorflowasr_amd.config import load_yaml
    from tensorflowasr_amd.models import ChunkConformer, ctc_prefix_beam_decode
    cfg = load_yaml(os.path.join(ROOT, "tensorflowasr_amd", "configs", "chunk_conformerS.yml"))
    Vp, Vt = NUM_CLASSES, 9160
    m = ChunkConformer(cfg, phone=Vp, txt=Vt, device=device)
    m._build(seed=0)
    B, L, d = 16, 480000, 144
    wav = torch.from_numpy(synth_batch(0, B, L)).to(device)
    out = {}

    def predict():
        out["logits"], out["counts"] = m.predict(wav)

    def decode():
        return ctc_prefix_beam_decode(out["logits"], out["counts"], beam_width=10, cutoff_prob=0.99, cutoff_top_n=40, is_logits=True)

    def step():
        predict()
        return decode()

    t = _timed(step, steps)
    tp = min(_timed(predict, steps, warmup=1), _timed(predict, steps, warmup=0))     # (one box measured 4.3 ms in a single region here against 2.4 on every other; its predict + beam total was the usual 5.1)
    # the same work with the beam search of batch n on a second stream while batch n + 1 is predicted
    from tensorflowasr_amd.models import ChunkBeamPipeline
    pipe = ChunkBeamPipeline(m, beam_width=10, cutoff_prob=0.99, cutoff_top_n=40)
    t_pipe = None
    for _ in range(2):                       # best of two regions: one allocator growth (hipMalloc) inside five pushes doubles the figure
        for _ in range(3):
            pipe.push(wav)
        pipe.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.push(wav)
        pipe.flush()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        t_pipe = dt if t_pipe is None else min(t_pipe, dt)
    pipe.close()
    nk = len(_lib.KERNEL_NAMES)
    _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 1))
    torch.cuda.synchronize()
    _read_profile(lib, m._h, nk, 1)
    _timed(predict, steps, warmup=0)
    prof = _read_profile(lib, m._h, nk, steps)
    _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 0))
    sch = read_schemes(lib, m._h)
    T = m.out_frames(L)[1]
    Tp = int(out["logits"].shape[1])
    M, Mp = B * T, B * Tp
    mc = cfg["model_config"]
    nb = {k: mc[n]["num_blocks"] for k, n in (("enc", "ChunkConformerEncoder"), ("pick", "ChunkCTCPicker"),
                                              ("help", "ContextHelper"), ("dec", "ChunkCTCDecoder"))}
    f_tail = lambda rows: 2.0 * rows * d * 2 * d + 2.0 * rows * 2 * d * d + 2.0 * 2 * rows * d * 4 * d      # conv tail + ff_module_2
    f_ff1 = lambda rows: 2.0 * 2 * rows * d * 4 * d + 3 * 2.0 * rows * d * d                               # ff_module_1 + qkv
    # launches of one predict(): a stack of n blocks = 1 x ff1_qkv, (n - 1) x tail_ff1, 1 x tail_ff2
    fl = {"tail_ff1": (nb["enc"] - 1 + nb["pick"] - 1) * (f_tail(M) + f_ff1(M)) + (nb["help"] - 1 + nb["dec"] - 1) * (f_tail(Mp) + f_ff1(Mp)),
          "tail_ff2": 2 * f_tail(M) + 2 * f_tail(Mp), "ff1_qkv": 2 * f_ff1(M) + 2 * f_ff1(Mp),
          "out_glu": (nb["enc"] + nb["pick"]) * 3 * 2.0 * M * d * d + (nb["help"] + nb["dec"]) * 3 * 2.0 * Mp * d * d,
          "ctc_head": 2.0 * M * d * Vp + 2.0 * Mp * d * Vt, "subconv": 2.0 * B * 1501 * 40 * d * 9 + 2.0 * M * 20 * d * 9 * d,
          "sublinear": 2.0 * M * 20 * d * d}
    if "out_glu" not in prof:        # round 4: out-projection + GLU run in the prologue of the tail kernels
        og = lambda rows: 3 * 2.0 * rows * d * d
        fl["tail_ff1"] += (nb["enc"] - 1 + nb["pick"] - 1) * og(M) + (nb["help"] - 1 + nb["dec"] - 1) * og(Mp)
        fl["tail_ff2"] += 2 * og(M) + 2 * og(Mp)
    wf = {k: (mc[n]["win_front"] + mc[n]["win_back"] + 1) for k, n in (("enc", "ChunkConformerEncoder"), ("pick", "ChunkCTCPicker"),
                                                                       ("help", "ContextHelper"), ("dec", "ChunkCTCDecoder"))}
    # band attention (chunk_conformer_blocks.py:158-176): a query sees win_front + win_back + 1 keys
    fl["attention"] = sum(nb[k] * 2 * 2.0 * (M if k in ("enc", "pick") else Mp) * wf[k] * d for k in nb)
    kern = {}
    for n, (ms_step, launches) in prof.items():
        f = fl.get(n, 0.0)
        peak = kernel_peak(n, sch)[0]
        kern[n] = {"launches_per_step": launches, "ms_per_step": round(ms_step, 4), "scheme": SCHEME_NAME[sch.get(n, -1)],
                   "tflops": round(f / (ms_step * 1e-3) / 1e12, 2) if f else None,
                   "frac_of_peak": round(f / (ms_step * 1e-3) / 1e12 / peak, 4) if f else None}
    dom = max(kern, key=lambda n: kern[n]["ms_per_step"])
    res = {"workload": "ChunkConformer 15M + CTC prefix beam (beam 10), 16 x 30 s utterances per GPU (batch=128 over 8 GPUs), fp32",
           "dtype": "f32", "steps": steps, "ms_per_step": round(t * 1e3, 3), "ms_predict": round(tp * 1e3, 3),
           "ms_beam10": round((t - tp) * 1e3, 3), "frames_per_s": round(B * 3000 / t, 1), "picked_frames_max": Tp,
           "pipelined": {"ms_per_step": round(t_pipe * 1e3, 3), "frames_per_s": round(B * 3000 / t_pipe, 1),
                         "how": "beam search of batch n on a second stream (helper thread) while batch n + 1 is predicted (models.ChunkBeamPipeline)"},
           "roofline": {"bound": "mfma", "kernel": dom, "achieved": kern[dom]["tflops"],
                        "peak": round(kernel_peak(dom, sch)[0], 1), "unit": "TFLOP/s",
                        "frac": kern[dom]["frac_of_peak"], "traffic": None,
                        "note": "categories of predict() summed over their launches of one step; the prefix beam search is a latency "
                                "chain (16 utterances x T_pick dependent frames), not a roofline kernel"},
           "kernels": kern}
    if with_cpu:
        from oracle import conformer_oracle as co          # checker only: the CPU baseline leg
        c5 = dict(co.CHUNK_S)
        w5 = co.chunk_weights(c5, seed=0)
        x5 = co.synth_wave(0, L)[None]
        t0 = time.perf_counter()
        co.chunk_predict(x5, w5, c5, dtype=np.float32)
        tt = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(3000.0 / tt, 1), "unit": "audio-frames/s", "kind": "port", "cores": int(os.cpu_count() or 1),
                               "sample": "1 x (one 30 s utterance through chunk_predict, fp32 NumPy oracle; beam search not included), %.1f s" % tt}
    del m
    return res


def config5_main(args, world, rank, device, use_dist):
    """`bench.py --config 5 [--gpus N]`: BASELINE.json configs[4] as its own contract line -- ChunkConformer predict + device
    prefix beam search (beam 10) over 16 x 30 s utterances per GPU (weak scaling: 128 utterances over 8 GPUs), the beams of
    all ranks exchanged with parallel.all_gather_hypotheses.  Same timing rules as the headline line."""
    from tensorflowasr_amd.config import load_yaml
    from tensorflowasr_amd.models import ChunkConformer, ctc_prefix_beam_decode
    dist = None
    if use_dist:
        import torch.distributed as dist
        from tensorflowasr_amd.parallel import all_gather_hypotheses, broadcast_weights
    cfg = load_yaml(os.path.join(ROOT, "tensorflowasr_amd", "configs", "chunk_conformerS.yml"))
    m = ChunkConformer(cfg, phone=NUM_CLASSES, txt=9160, device=device)
    m._build(seed=0)
    if use_dist:
        m.load_weights(broadcast_weights(m.get_weights_dict(), src=0, device=device), by_name=False)
    B, L = 16, 480000
    wav = torch.from_numpy(synth_batch(rank * B, B, L)).to(device)

    last = [None]

    def step():
        logits, counts = m.predict(wav)
        hyp = ctc_prefix_beam_decode(logits, counts, beam_width=10, cutoff_prob=0.99, cutoff_top_n=40, is_logits=True)
        last[0] = all_gather_hypotheses(*hyp, device=device) if use_dist else hyp
        return last[0]

    for _ in range(args.warmup):
        step()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        tt = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, dict(zip(("ids", "lens", "scores", "n_hyp"), last[0])))
    if rank == 0:
        del m
        torch.cuda.empty_cache()
        extra = extra_config5(_lib.lib(), device, steps=max(2, min(args.steps, 5)), with_cpu=(world == 1 and not args.no_cpu_baseline))
        line = {"metric": "audio-frames/sec, ChunkConformer 15M + CTC prefix beam (beam 10), 30 s utts, 16 per MI355X",
                "value": round(world * B * 3000 * args.steps / dt, 1), "unit": "audio-frames/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": extra["workload"], "global_batch": world * B, "samples_per_utt": L,
                           "parallelism": "dp%d" % world, "weights": "random-init (Keras defaults)",
                           "rccl_ranks": (dist.get_world_size() if use_dist else None)},
                "roofline": extra["roofline"], "kernels": extra["kernels"], "ms_predict": extra["ms_predict"],
                "ms_beam10": extra["ms_beam10"]}
        if "cpu_baseline" in extra:
            line["cpu_baseline"] = extra["cpu_baseline"]
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


# The same library with every split-operand kernel on its EXACT-product variant: fp32 operands as three bf16 terms, six MFMAs
# per fragment pair, nothing below 2^-24 of a product dropped (rounds 1-2's arithmetic).  The headline runs two fp16 terms
# where an operand bound is known; this leg puts the price and the numerical difference of that choice in the same line.
EXACT_ENV = {"MI355ASR_PP": "0", "MI355ASR_PP_OUTGLU": "0", "MI355ASR_PP_HEAD": "0", "MI355ASR_SUBCONV_TERMS": "3",
             "MI355ASR_ATTN_TERMS": "3", "MI355ASR_FFT_TERMS": "3"}
LOGIT_SAMPLE = slice(0, None, 8)      # utterances 0, 8, ..., 56 of the batch


def sample_logits(model, wav):
    return model.ctc_logits(model.encode(wav))[LOGIT_SAMPLE].float().cpu().numpy()


def exact_child(args, device):
    """`bench.py --exact-child OUT.npy` (run by exact_products_leg with EXACT_ENV): K steps of the headline step, one JSON line"""
    B, L = args.batch, int(args.seconds * 16000)
    model = build_model(device, 0, 1, False)
    wav = torch.from_numpy(synth_batch(0, B, L)).to(device)
    model.prepare(B, L)
    t = _timed(lambda: model.recognize(wav, reuse_buffers=True), args.steps, warmup=args.warmup)
    np.save(args.exact_child, sample_logits(model, wav))
    sch = read_schemes(_lib.lib(), model._h)
    print(json.dumps({"ms_per_step": round(t * 1e3, 3), "value": round(B * (L // 160) / t, 1),
                      "schemes": {n: SCHEME_NAME[v] for n, v in sch.items() if v >= 0}}), flush=True)


def exact_products_leg(args, model, wav):
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "exact_logits.npy")
        cmd = [sys.executable, os.path.abspath(__file__), "--exact-child", out, "--steps", str(args.steps), "--warmup", str(max(args.warmup, 2)),
               "--batch", str(args.batch), "--seconds", str(args.seconds)]
        r = subprocess.run(cmd, env=dict(os.environ, **EXACT_ENV), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        res = json.loads(r.stdout.strip().splitlines()[-1])
        mine = sample_logits(model, wav)
        theirs = np.load(out)
    res["max_abs_logit_diff_vs_default"] = float(np.abs(mine - theirs).max())
    res["argmax_equal_frames"] = "%d / %d" % (int((mine.argmax(-1) == theirs.argmax(-1)).sum()), mine.shape[0] * mine.shape[1])
    res["unit"] = "audio-frames/s"
    res["env"] = EXACT_ENV
    res["what"] = ("the same step with every split-operand kernel on three exact bf16 terms (six MFMAs per product) instead of two fp16 terms; "
                   "logits of utterances 0, 8, ..., 56 compared with the headline build's")
    return res


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher around it: re-run this command line as N ranks of one node"""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)


def timed_steps(step, pending, n_steps, dist, use_dist, sync, device):
    """EXACTLY n_steps steps between barrier + synchronize on both sides; the MAX over ranks"""
    if use_dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        step()
    while pending:
        pending.pop().wait()
    sync()
    if use_dist:
        dist.barrier()
        sync()
    dt = time.perf_counter() - t0
    if use_dist:
        tt = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt


def repeated_regions(region, steps, min_s, dist, use_dist, device):
    """region() = one K-step timed region (seconds, already the max over ranks).  Regions are repeated until min_s seconds have
    been measured (every rank takes the same decision: rank 0's clock, broadcast).  -> (total seconds, [seconds per region])"""
    times = []
    while True:
        times.append(region())
        go = 1 if sum(times) < min_s and len(times) < 10000 else 0
        if use_dist:
            g = torch.tensor([go], dtype=torch.int32, device=device)
            dist.broadcast(g, src=0)
            go = int(g.item())
        if not go:
            return sum(times), times


def dump_outputs(out_dir, arrays):
    """{name: tensor or array} -> out_dir/<name>.npy in float64 (ids, lengths and float32 scores are all exact in float64)"""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float64))


def region_stats(times, steps):
    per = sorted(t / steps * 1e3 for t in times)
    return {"regions": len(per), "min": round(per[0], 4), "median": round(per[len(per) // 2], 4), "max": round(per[-1], 4)}


def dry_run_gloo(args, world, rank):
    """The multi-rank control flow of main() with no GPU in it: gloo process group, the stand-in recogniser below in place of
    mi355asr_recognize, the same rotating output sets, asynchronous id exchange, barrier / max-over-ranks timing, repeated
    regions and line format.  What it proves: `python bench.py --gpus N` starts N ranks, they rendezvous, every rank sees every
    rank's ids in rank order, and one well-formed line comes out.  It measures nothing."""
    import torch.distributed as dist
    from tensorflowasr_amd.parallel import all_gather_ids
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    device = torch.device("cpu")
    probe = torch.ones(1, dtype=torch.int32)
    dist.all_reduce(probe)
    if int(probe.item()) != world or dist.get_world_size() != args.gpus:
        raise SystemExit("gloo sees %d ranks (all_reduce counted %d), --gpus %d" % (dist.get_world_size(), int(probe.item()), args.gpus))
    B, L = args.batch, int(args.seconds * 16000)
    T = -(-(-(-(-(-L // 160)) // 2)) // 2)
    rot = [(torch.empty((B, T), dtype=torch.int32), torch.empty((B,), dtype=torch.int32)) for _ in range(3)]
    pending, nstep, seen = [], [0], []

    def recognize(out):                                  # ids that name their rank, utterance and step
        ids, lens = out
        ids.fill_(-1)
        ids[:, 0] = rank
        ids[:, 1] = torch.arange(B, dtype=torch.int32) + rank * B
        ids[:, 2] = nstep[0]
        lens.fill_(3)
        return ids, lens

    def step():
        ids, lens = recognize(rot[nstep[0] % 3])
        nstep[0] += 1
        work = all_gather_ids(ids, lens, async_op=True)
        pending.append(work)
        seen.append(work)
        while len(pending) > 2:
            pending.pop(0).wait()
        return work

    for _ in range(args.warmup):
        step()
    while pending:
        pending.pop().wait()
    seen.clear()
    total, times = repeated_regions(lambda: timed_steps(step, pending, args.steps, dist, True, lambda: None, device), args.steps,
                                    min(args.min_timed_s, 0.05), dist, True, device)
    a_ids, a_lens = seen[-1].result()
    ok = bool((a_ids[:, 0] == torch.arange(world, dtype=torch.int32).repeat_interleave(B)).all()
              and (a_ids[:, 1] == torch.arange(world * B, dtype=torch.int32)).all() and (a_lens == 3).all())
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        n = len(times) * args.steps
        print(json.dumps({"metric": "audio-frames/sec/GPU + RTF, ConformerCTC(S) 10s utts, 1/2/4/8 MI355X", "value": round(world * B * (L // 160) * n / total, 1),
                          "unit": "audio-frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(total / n * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "f32", "data": "synthetic", "dry_run": True, "gathered_ids_in_rank_order": bool(flag.item()),
                          "timed_region_s": round(total, 4), "region_ms_per_step": region_stats(times, args.steps),
                          "config": {"workload": "DRY RUN (gloo, stand-in recogniser): launcher + exchange + line format only",
                                     "global_batch": world * B, "parallelism": "dp%d" % world, "rccl_ranks": None,
                                     "backend": "gloo", "ranks": dist.get_world_size()}}), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="utterances per GPU")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-h2d", action="store_true", help="skip the host-buffer (PCIe-inclusive) variant")
    ap.add_argument("--config", type=int, default=2, choices=[2, 5],
                    help="2 (default): the headline ConformerCTC(S) line; 5: ChunkConformer + prefix beam as its own line")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip BASELINE configs 3 (streaming, bf16) and 5 (ChunkConformer + prefix beam) after the headline region")
    ap.add_argument("--no-exact-leg", action="store_true", help="skip the exact-product (three-term) comparison run")
    ap.add_argument("--no-latency-b1", action="store_true", help="skip the one-utterance latency measurement (kernel traces of the headline shape)")
    ap.add_argument("--exact-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="do not record per-kernel HIP events in the timed region (roofline fields become null)")
    ap.add_argument("--min-timed-s", type=float, default=0.0,
                    help="0 (default): the headline region is exactly --steps steps.  > 0: whole K-step regions (each bracketed by "
                         "barrier + synchronize) are repeated until this much time has been measured; ms_per_step = total time / total steps")
    ap.add_argument("--min-warmup-s", type=float, default=1.0,
                    help="after the --warmup steps, untimed K-step regions run until this much time has passed (steady clocks "
                         "before the headline region; 0: none)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned (config 2: ids, lens; config 5: ids, lens, scores, n_hyp) "
                         "as DIR/<name>.npy in float64")
    ap.add_argument("--dry-run-gloo", action="store_true",
                    help="no GPU, no kernels: the launcher, the process group (gloo), the per-step id exchange, the max-over-ranks "
                         "timing and the JSON line with a stand-in recogniser (tests/test_distributed_cpu.py)")
    args = ap.parse_args()

    force_dist = os.environ.get("MI355ASR_BENCH_FORCE_DIST") == "1"
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or force_dist) and not args.exact_child:
        # started as `python bench.py --gpus N` (the driver's form): become the launcher -- one rank per GPU under
        # torch.distributed.run on this node; rank 0 prints the one JSON line on the inherited stdout
        return self_launch(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if args.dry_run_gloo:
        return dry_run_gloo(args, world, rank)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    # MI355ASR_BENCH_FORCE_DIST=1 under `torch.distributed.run --nproc-per-node 1` exercises the RCCL code path
    # (init, barrier, broadcast, all_gather) on a one-GPU box
    use_dist = world > 1 or force_dist
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
        from tensorflowasr_amd.parallel import all_gather_ids
        # RCCL has to see exactly the N ranks the driver asked for, one GPU each: a count of the ranks through the backend itself
        probe = torch.ones(1, dtype=torch.int32, device=device)
        dist.all_reduce(probe)
        if int(probe.item()) != world or dist.get_world_size() != args.gpus:
            raise SystemExit("RCCL sees %d ranks (all_reduce counted %d), --gpus %d" % (dist.get_world_size(), int(probe.item()), args.gpus))

    if args.config == 5:
        return config5_main(args, world, rank, device, use_dist)
    if args.exact_child:
        return exact_child(args, device)
    B, L = args.batch, int(args.seconds * 16000)
    model = build_model(device, rank, world, use_dist)
    wav = torch.from_numpy(synth_batch(rank * B, B, L)).to(device)      # inputs resident in HBM
    T = model.prepare(B, L)
    h = model._h

    pending = []                                                 # RCCL work handles of the batches still in exchange

    # data-parallel runs rotate three output sets: the ids of batch n travel over RCCL (its own stream) while batch
    # n + 1 is recognised into the next set
    # (ids and lengths of a set are two views of one buffer: one collective per batch, parallel.ids_lens_buffer)
    rot = None
    if use_dist:
        from tensorflowasr_amd.parallel import ids_lens_buffer
        rot = [ids_lens_buffer(B, T, device) for _ in range(3)]
    nstep = [0]
    last = [None]                                                # (ids, lens) the latest step returned

    def step():
        if use_dist:
            ids, lens = model.recognize(wav, out=rot[nstep[0] % 3])
            last[0] = ids, lens
            nstep[0] += 1
            if os.environ.get("MI355ASR_BENCH_DEBUG_NO_GATHER") == "1":     # diagnosis only: what the exchange itself costs
                return ids, lens
            # every handle is waited for before the timed region ends; at most two exchanges are left in flight, so a
            # buffer set is never rewritten while its exchange reads it
            work = all_gather_ids(ids, lens, async_op=True)
            pending.append(work)
            while len(pending) > 2:
                pending.pop(0).wait()
            return work
        last[0] = model.recognize(wav, reuse_buffers=True)       # the C-ABI call writes into pre-allocated outputs
        return last[0]

    lib = _lib.lib()
    nk = len(_lib.KERNEL_NAMES)
    ms = (ctypes.c_double * nk)()
    cnt = (ctypes.c_int64 * nk)()

    def timed_region(n_steps):
        return timed_steps(step, pending, n_steps, dist, use_dist, torch.cuda.synchronize, device)

    for _ in range(args.warmup):
        step()
    while pending:
        pending.pop().wait()
    # region 1: the headline number -- exactly K steps, no instrumentation
    _lib.check(lib.mi355asr_profile_enable(h.ptr, 0))
    # untimed K-step regions until --min-warmup-s has passed: a region right after a few warm-up steps runs ~5 % slower than
    # the ones after it (measured: 1.93 against 1.84 ms/step), which is the clock and not the code
    warm_s = sum(repeated_regions(lambda: timed_region(args.steps), args.steps, args.min_warmup_s, dist, use_dist, device)[1]) \
        if args.min_warmup_s > 0 else 0.0
    # --min-timed-s > 0 repeats whole K-step regions until that much time has been measured (K = 20 steps is ~40 ms, less
    # than the box-to-box spread) and reports the spread over the regions next to the mean; by default one region of K steps
    total_s, region_s = repeated_regions(lambda: timed_region(args.steps), args.steps, args.min_timed_s, dist, use_dist, device)
    n_regions = len(region_s)
    elapsed = total_s / n_regions                    # seconds per K-step region (mean over the regions)
    if rank == 0 and args.dump_outputs:              # before anything else reuses the output buffers
        dump_outputs(args.dump_outputs, {"ids": last[0][0], "lens": last[0][1]})
    # region 2: the same K steps again with HIP events recorded on the launch stream around every kernel
    # (costs ~0.9 ms/step of event traffic, which is why it is not the region `value` is computed from)
    elapsed_ev = None
    if not args.no_kernel_events:
        _lib.check(lib.mi355asr_profile_enable(h.ptr, 1))
        torch.cuda.synchronize()
        _lib.check(lib.mi355asr_profile_read(h.ptr, ms, cnt, nk, 1))
        elapsed_ev = timed_region(args.steps)
        _lib.check(lib.mi355asr_profile_read(h.ptr, ms, cnt, nk, 1))
        _lib.check(lib.mi355asr_profile_enable(h.ptr, 0))

    # region 3 (reported separately, never `value`): the batch starts in pinned HOST memory; (a) copy on the launch
    # stream, then recognise; (b) the copy of batch n + 1 on a second stream while batch n is recognised
    h2d = None
    if not args.no_h2d:
        host = torch.from_numpy(synth_batch(rank * B, B, L)).pin_memory()
        dev_bufs = [torch.empty_like(wav), torch.empty_like(wav)]
        n_h = max(args.steps, 1)

        def serial():
            dev_bufs[0].copy_(host, non_blocking=True)
            model.recognize(dev_bufs[0], reuse_buffers=True)

        for _ in range(2):
            serial()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_h):
            serial()
        torch.cuda.synchronize()
        t_serial = (time.perf_counter() - t0) / n_h
        copy_stream = torch.cuda.Stream(device=device)
        main_stream = torch.cuda.current_stream(device)
        ready = [torch.cuda.Event(), torch.cuda.Event()]
        freed = [torch.cuda.Event(), torch.cuda.Event()]

        def overlapped(n):
            with torch.cuda.stream(copy_stream):
                dev_bufs[0].copy_(host, non_blocking=True)
                ready[0].record(copy_stream)
            for i in range(n):
                cur, nxt = i & 1, (i + 1) & 1
                if i + 1 < n:
                    with torch.cuda.stream(copy_stream):
                        if i >= 1:
                            copy_stream.wait_event(freed[nxt])
                        dev_bufs[nxt].copy_(host, non_blocking=True)
                        ready[nxt].record(copy_stream)
                main_stream.wait_event(ready[cur])
                model.recognize(dev_bufs[cur], reuse_buffers=True)
                freed[cur].record(main_stream)

        overlapped(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        overlapped(n_h)
        torch.cuda.synchronize()
        t_over = (time.perf_counter() - t0) / n_h
        h2d = {"bytes_per_step": int(host.numel() * 4),
               "serial": {"ms_per_step": round(t_serial * 1e3, 3), "value": round(B * (L // 160) / t_serial, 1),
                          "how": "pinned host batch -> hipMemcpyAsync on the launch stream -> recognize"},
               "overlapped": {"ms_per_step": round(t_over * 1e3, 3), "value": round(B * (L // 160) / t_over, 1),
                              "how": "copy of batch n+1 on a second stream while batch n is recognised (two device buffers)"},
               "unit": "audio-frames/s per GPU"}

    if rank == 0:
        frames_per_utt = L // 160
        total_frames = world * B * frames_per_utt * args.steps
        value = total_frames / elapsed
        # the banded mel kernel runs unless MI355ASR_MEL_BAND=0 (the default freq2mel has no filter wider than 64 bins)
        mel_nnz = None
        if os.environ.get("MI355ASR_MEL_BAND", "1") != "0":
            from tensorflowasr_amd import frontend_consts
            mel_nnz = int(np.count_nonzero(frontend_consts.freq2mel(16000, 1024, 80)))
        fl = algorithmic_flops(B, L, stft_mode=int(lib.mi355asr_stft_mode(h.ptr)), mel_nnz=mel_nnz)
        ab = algorithmic_bytes(B, L)
        launched = {name for i, name in enumerate(_lib.KERNEL_NAMES) if cnt[i]}
        if "out_glu" not in launched:
            # round 4: out-projection + GLU run in the prologue of the tail kernels (the block is attention + one launch): its
            # flops and its weights are theirs now (the halo rows the prologue recomputes are NOT counted: algorithmic flops)
            for n in ("tail_ff1", "tail_ff2"):
                fl[n] += fl["out_glu"]
                ab[n] += 4.0 * 3 * S_CFG["dmodel"] ** 2
        n_ff1 = max(cnt[_lib.KERNEL_NAMES.index("ff1_qkv")] // args.steps, 1)
        for pre in ("sublinear", "ctc_project"):
            if pre not in launched and "ff1_qkv" in launched:
                # round 4: the subsampling Dense / the CTC projection run in the prologue of the ff1_qkv launch behind them (two
                # such launches per step: the per-launch average carries half of each); x0 is neither written nor read
                fl["ff1_qkv"] += fl[pre] / n_ff1
                ab["ff1_qkv"] += (ab[pre] - 2 * 4.0 * B * (L // 640) * S_CFG["dmodel"]) / n_ff1
        if "ctc_head" not in launched and "tail_ff2" in launched:
            # round 4: the class head runs behind the CTC block's tail (one of the two tail_ff2 launches of a step)
            n_t2 = max(cnt[_lib.KERNEL_NAMES.index("tail_ff2")] // args.steps, 1)
            fl["tail_ff2"] += fl["ctc_head"] / n_t2
            ab["tail_ff2"] += (ab["ctc_head"] - 2 * 4.0 * B * (L // 640) * S_CFG["dmodel"]) / n_t2
        kern = {}
        for i, name in enumerate(_lib.KERNEL_NAMES):
            if cnt[i]:
                avg_ms = ms[i] / cnt[i]
                kern[name] = {"launches_per_step": cnt[i] // args.steps, "avg_ms": round(avg_ms, 4),
                              "share": round(ms[i] / max(sum(ms), 1e-9), 4),
                              "tflops": round(fl[name] / (avg_ms * 1e-3) / 1e12, 2) if fl[name] else None}
        dom = max(kern, key=lambda n: kern[n]["share"]) if kern else None
        achieved = (kern[dom]["tflops"] or 0.0) if dom else 0.0
        schemes = read_schemes(lib, h)           # what the library's launchers chose, per kernel category
        peak, peak_kind = kernel_peak(dom, schemes)
        for n in kern:
            kern[n]["scheme"] = SCHEME_NAME[schemes.get(n, -1)]
            if kern[n]["tflops"]:
                kern[n]["frac_of_peak"] = round(kern[n]["tflops"] / kernel_peak(n, schemes)[0], 4)
        for n in kern:
            if n in ab:
                kern[n]["hbm_gbs"] = round(ab[n] / (kern[n]["avg_ms"] * 1e-3) / 1e9, 1)
                kern[n]["hbm_frac"] = round(kern[n]["hbm_gbs"] / PEAK_HBM_GBS, 4)
        # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the figure comes
        # from separate `rocprofv3 --pmc` passes over this same command (tools/pmc_probe.sh -> profiles/pmc_traffic.json)
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc):
            traffic = json.load(open(pmc)).get(dom)
        step_bytes = B * 27.5e6 * (L / 160000.0) + 38.4e6     # 27.5 MB per 10 s utterance + the weights once
        line = {
            "metric": "audio-frames/sec/GPU + RTF, ConformerCTC(S) 10s utts, 1/2/4/8 MI355X",
            "value": round(value, 1), "unit": "audio-frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "ConformerCTC(S) 10M offline, batch=%d %gs utts per GPU, fp32, waveform->CTC greedy ids"
                                   % (B, args.seconds),
                       "global_batch": world * B, "samples_per_utt": L, "enc_frames": T,
                       "parallelism": "dp%d" % world, "weights": "random-init encoder + reference-exported CTCDecoder",
                       "rccl_ranks": (dist.get_world_size() if use_dist else None), "backend": ("nccl (RCCL)" if use_dist else None)},
            "value_is": "whole-job aggregate over n_gpus (driver contract); the metric's per-GPU rate is frames_per_s_per_gpu",
            "arithmetic": "fp32 values and fp32 accumulation; products on the 16-bit matrix pipe from split fp32 operands -- two fp16 terms of "
                          "power-of-two scaled operands (three MFMAs) where a bound is known, else three exact bf16 terms (six) or the fp32 "
                          "instruction; same measured distance from the fp64 oracle (DESIGN.md section 2, profiles/r03d_parity_excused_frames.jsonl)",
            "frames_per_s_per_gpu": round(value / world, 1),
            "timed_region_s": round(total_s, 4), "timed_steps_total": n_regions * args.steps, "untimed_warmup_s": round(warm_s, 3),
            "region_ms_per_step": region_stats(region_s, args.steps),
            "ms_per_step_with_kernel_events": round(elapsed_ev / args.steps * 1e3, 3) if elapsed_ev else None,
            "rtf": round(elapsed / args.steps / (world * B * args.seconds), 8),
            "roofline": {"bound": "mfma", "kernel": dom, "achieved": achieved, "peak": round(peak, 1),
                         "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
                         "traffic_source": "offline rocprofv3 --pmc passes over this command (profiles/pmc_traffic.json), bytes per launch",
                         "pipe": peak_kind,
                         # last round's line priced this kernel against the six-product bf16 pipe (2500 / 6); kept so that the
                         # two rounds can be compared on one basis -- the kernel now runs three products per fp32 product
                         "frac_vs_six_product_pipe": round(achieved / PEAK_SPLIT3_TFLOPS, 4) if peak == PEAK_HALF2_TFLOPS else None,
                         "algorithmic_bytes": ab.get(dom), "hbm_frac": kern[dom].get("hbm_frac") if dom else None,
                         "step_hbm_frac": round(step_bytes / (elapsed / args.steps) / (PEAK_HBM_GBS * 1e9), 4)},
            "h2d_inclusive": h2d,
            "kernels": kern,
        }
        if os.environ.get("MI355ASR_BENCH_DEBUG_NO_GATHER") == "1":
            line["debug_no_gather"] = True       # the id exchange was removed from the timed step: not a data-parallel measurement
        if world == 1 and not args.no_latency_b1:
            # what a test_asr.py user sees: ONE utterance per call (test_asr.py:186-219), waveform -> greedy ids, resident input
            one = wav[:1].contiguous()
            model.prepare(1, L)
            t1 = _timed(lambda: model.recognize(one, reuse_buffers=True), 50, warmup=5)
            line["latency_b1"] = {"ms": round(t1 * 1e3, 3), "utterance_s": args.seconds, "rtf": round(t1 / args.seconds, 8),
                                  "what": "one %g s utterance per recognize() call, input resident in HBM, 50 calls" % args.seconds}
            model.prepare(B, L)
        if world == 1:
            line["parity"] = parity_stamp(model, wav, B, L)
        if world == 1 and not args.no_extra_configs:
            try:
                line["length_sweep"] = length_sweep(model, device)
            except Exception as e:
                line["length_sweep"] = {"error": "%s: %s" % (type(e).__name__, e)}
            model.prepare(B, L)
        if world == 1 and not args.no_exact_leg:
            line["exact_products"] = exact_products_leg(args, model, wav)
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
        if world == 1 and not args.no_extra_configs:
            # BASELINE.json configs 3 and 5 on the same box, after (never inside) the headline region: their own keys,
            # each with its dominant kernel category against its roofline and a bounded CPU sample of the oracle
            del model
            torch.cuda.empty_cache()
            for key, fn in (("config3", extra_config3), ("config5", extra_config5)):
                try:
                    line[key] = fn(lib, device, with_cpu=not args.no_cpu_baseline)
                except Exception as e:           # the headline line must not die with an extra
                    line[key] = {"error": "%s: %s" % (type(e).__name__, e)}
            try:                                 # the drop-in's whole offline_stt (with the Translator) as its own key
                line["stt_with_translator"] = extra_stt(lib, device)
            except Exception as e:
                line["stt_with_translator"] = {"error": "%s: %s" % (type(e).__name__, e)}
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
