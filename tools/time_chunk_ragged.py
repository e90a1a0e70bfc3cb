"""HIP-event timing of the ragged ChunkConformer predict (mi355asr_chunk_predict_ragged) on config 5's model, 16 x 30 s.

    python tools/time_chunk_ragged.py [--regions 5] [--iters 10] [--json profiles/chunk_ragged_mi355x.json]
    python tools/time_chunk_ragged.py --ab PARENT.so [--json ...]       # plain predict: parent build against this build

Regions, each as min / median / max milliseconds per call over `regions` timed regions of `iters` back-to-back calls bracketed
by events on the launch stream (after warm-up):
  equal    16 x 30 s: predict against predict(wav_lengths = all L)
  ragged   16 utterances, seeded lengths uniform over 5 .. 30 s: the ragged predict at [16, Lmax] against the padded predict at
           that shape (same work, other results for the shorter rows) and against the per-utterance loop (16 predict calls of
           [1, L_b])
  stt      greedy ChunkASR.offline_stt_batch of the 16 utterances against 16 solo decodes in the manner of offline_stt (predict of
           [1, L_b] + frame_argmax + ctc_greedy_decode), wall clock

--ab: plain predict at 16 x 30 s in a process of its own per library (MI355ASR_LIB selects it), interleaved parent, this build,
parent: the parent -> this difference against the parent -> parent difference."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, regions, iters):
    import torch
    stream = torch.cuda.current_stream()
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
    return dict(ms_min=per[0], ms_median=float(np.median(per)), ms_max=per[-1])


def wall(call, n):
    import torch
    call()
    torch.cuda.synchronize()
    per = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    per.sort()
    return dict(ms_min=per[0], ms_median=float(np.median(per)), ms_max=per[-1])


def model():
    from bench import NUM_CLASSES
    from tensorflowasr_amd.config import load_yaml
    from tensorflowasr_amd.models import ChunkConformer
    cfg = load_yaml(os.path.join(ROOT, "tensorflowasr_amd", "configs", "chunk_conformerS.yml"))
    m = ChunkConformer(cfg, phone=NUM_CLASSES, txt=9160)
    m._build(seed=0)
    return m


def ab_child(regions, iters):
    import ctypes
    import torch
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.synthetic import synth_batch
    probe = ctypes.CDLL(_lib.LIB_PATH)                     # an older build lacks the newest entry points: plain predict needs none of them
    for name in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:
        del _lib.SIGNATURES[name]
    m = model()
    wav = torch.from_numpy(synth_batch(0, 16, 480000)).cuda()
    r = timed(lambda: m.predict(wav), regions, iters)
    logits, counts = m.predict(wav)
    r["lib"] = os.path.basename(os.environ.get("MI355ASR_LIB", "this build"))
    r["logits_checksum"] = float(logits.double().abs().sum().item())
    r["counts_sum"] = int(counts.sum())
    print(json.dumps(r))


def ab(parent, regions, iters):
    runs = []
    for lib in (parent, None, parent):
        env = dict(os.environ, CHUNK_RAGGED_AB_CHILD="1")
        if lib:
            env["MI355ASR_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, __file__, "--regions", str(regions), "--iters", str(iters)], env=env, capture_output=True,
                           text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(runs[-1], flush=True)
    a, b, c = (x["ms_median"] for x in runs)
    return dict(parent_first=runs[0], this_build=runs[1], parent_second=runs[2],
                parent_to_this_ms=b - 0.5 * (a + c), parent_to_parent_ms=abs(c - a),
                same_results=runs[0]["logits_checksum"] == runs[1]["logits_checksum"] and runs[0]["counts_sum"] == runs[1]["counts_sum"])


def stt_case(m, waves):
    """a ChunkASR around the model, with stand-in vocabularies of the model's class counts"""
    from tensorflowasr_amd.chunk_asr import ChunkASR

    class Text:
        num_classes, decoder_config, scorer = 9160, {"beam_width": 1}, None

        def iextract(self, ids):
            return [chr(0x4E00 + int(i)) for i in ids]

    class Speech:
        sample_rate = 16000
        load_wav = None                                    # (waveforms only)

    asr = ChunkASR.__new__(ChunkASR)
    asr.runner, asr.text_featurizer, asr.speech_featurizer, asr.device = m, Text(), Speech(), "cuda:0"
    from tensorflowasr_amd.chunk_asr import _ctc_text

    def solo():
        out = []
        for w in waves:
            data = w / np.abs(w.max())
            logits, _ = m.predict(data.reshape([1, -1, 1]))
            out.append("".join(Text().iextract(_ctc_text(logits, 9159))))
        return out
    return (lambda: asr.offline_stt_batch(waves)), solo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--ab", default=None, help="the parent build's libmi355asr.so")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    if os.environ.get("CHUNK_RAGGED_AB_CHILD"):
        return ab_child(a.regions, a.iters)
    out = {}
    if a.json and os.path.exists(a.json):
        with open(a.json) as f:
            out = json.load(f)
    if a.ab:
        out["plain_predict_16x30s_parent_vs_this"] = ab(a.ab, a.regions, a.iters)
    else:
        from tensorflowasr_amd.synthetic import synth_batch
        m = model()
        B, L = 16, 480000
        x = torch.from_numpy(synth_batch(0, B, L)).cuda()
        full = torch.full((B,), L, dtype=torch.int32, device="cuda")
        # (the ragged call reads its lengths back once per call: that synchronisation is inside the timed region)
        out["equal_16x30s"] = dict(predict=timed(lambda: m.predict(x), a.regions, a.iters),
                                   predict_ragged=timed(lambda: m.predict(x, wav_lengths=full), a.regions, a.iters))
        rng = np.random.default_rng(1)
        ln = rng.integers(5 * 16000, 30 * 16000 + 1, size=B).astype(np.int32)
        Lmax = int(ln.max())
        xr = x[:, :Lmax].contiguous()
        lr = torch.from_numpy(ln).cuda()
        solo = [xr[b:b + 1, :int(ln[b])].contiguous() for b in range(B)]

        def loop():
            for b in range(B):
                m.predict(solo[b])
        out["uniform_5_30s_16"] = dict(Lmax=Lmax, seconds=float(ln.sum()) / 16000,
                                       predict_ragged=timed(lambda: m.predict(xr, wav_lengths=lr), a.regions, a.iters),
                                       predict_padded=timed(lambda: m.predict(xr), a.regions, a.iters),
                                       per_utterance_loop=timed(loop, 3, 1))
        waves = [xr[b, :int(ln[b])].cpu().numpy() for b in range(B)]
        batch, one_by_one = stt_case(m, waves)
        out["offline_stt_16"] = dict(offline_stt_batch=wall(batch, 3), solo_decodes=wall(one_by_one, 3))
        e, r, s = out["equal_16x30s"], out["uniform_5_30s_16"], out["offline_stt_16"]
        out["ratios"] = dict(equal_ragged_over_predict=e["predict_ragged"]["ms_median"] / e["predict"]["ms_median"],
                             ragged_over_padded=r["predict_ragged"]["ms_median"] / r["predict_padded"]["ms_median"],
                             loop_over_ragged=r["per_utterance_loop"]["ms_median"] / r["predict_ragged"]["ms_median"],
                             solo_decodes_over_stt_batch=s["solo_decodes"]["ms_median"] / s["offline_stt_batch"]["ms_median"])
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
