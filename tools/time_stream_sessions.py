"""HIP-event timing of the batched streaming decode (tensorflowasr_amd/stream_session.py) on the streaming configuration's
models (StreamingConformerEncoder d = 256, CTCDecoder 1 block, Translator 1 block; random weights).

    python tools/time_stream_sessions.py [--regions 5] [--iters 10] [--gemm-dtype bfloat16] [--json out.json]

Each figure is min / median / max milliseconds per call over `regions` timed regions of `iters` back-to-back calls bracketed by
events on the launch stream (after warm-up):
  config3        configuration 3's step (tests/bench_configs.config3): what a call without lengths costs with this build; run
                 it with the parent's build too, on the same box, to price the length predicate
  decode_64      64 streams with histories uniform over 13 .. 520 frames, all due for a decode: one server tick (stream_gather +
                 ragged CTCDecoder + greedy collapse + ragged Translator), the same 64 decodes one stream at a time with the calls
                 without lengths (ASR.stream_stt's sequence: torch.cat of the chunk outputs, CTCDecoder, collapse, Translator),
                 and the padded call at the batch's shape without lengths (same work, wrong results for the shorter rows)
  tick_64        a realistic tick: 64 streams, 16 with a chunk due (one encoder call + stream_append), 8 with a decode due"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main():
    import torch
    from time_ragged import timed
    from tensorflowasr_amd.models import CTCDecoder, StreamingConformerEncoder, Translator, ctc_greedy_decode
    from tensorflowasr_amd.stream_session import stream_append, stream_gather
    from tensorflowasr_amd.synthetic import synth_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--gemm-dtype", default="bfloat16")
    ap.add_argument("--json", default=None)
    ap.add_argument("--config3-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {}
    import bench_configs
    out["config3"] = [bench_configs.config3(50, a.gemm_dtype)["ms_step_with_global_ctc"] for _ in range(3)]
    if not a.config3_only:
        V, VT, d, F, chunk = 1332, 4000, 256, 13, 8000
        enc = StreamingConformerEncoder(dmodel=d, reduction_factor=4, num_blocks=4, head_size=64, num_heads=4, kernel_size=5,
                                        fc_factor=0.5, sample_rate=16000, n_mels=80, stride_ms=10,
                                        mel_layer_type="Melspectrogram", gemm_dtype=a.gemm_dtype)
        enc.add_chunk_size(chunk, 80, 640)
        enc._build(seed=0)
        ctc = CTCDecoder(num_classes=V, dmodel=d, num_blocks=1, head_size=64, num_heads=4, kernel_size=32, gemm_dtype=a.gemm_dtype)
        ctc._build(seed=1)
        tr = Translator(inp_classes=V, tar_classes=VT, dmodel=d, num_blocks=1, head_size=64, num_heads=4, kernel_size=32)
        tr._build(seed=2)
        N, Tcap = 64, 40 * F
        rng = np.random.default_rng(0)
        n_chunks = rng.integers(1, 41, size=N)
        hist = torch.zeros((N, Tcap, d), device="cuda")
        hl = torch.zeros((N,), dtype=torch.int32, device="cuda")
        hl_host = np.zeros(N, np.int32)
        pieces = [[torch.randn(1, F, d, device="cuda") for _ in range(k)] for k in n_chunks]
        for s, p in enumerate(pieces):
            stream_append(torch.cat(p, 1).contiguous(), [s], hist, hl, hl_host)
        assert (hl_host == n_chunks * F).all()
        Tpad = int(hl_host.max())

        def decode_batch(slots):
            batch, blen = stream_gather(hist, hl, hl_host, slots, max(17, int(hl_host[slots].max())))
            _, fa = ctc(batch, return_argmax=True, return_logits=False, lengths=blen)
            ids, tok = ctc_greedy_decode(fa, blen, blank=V - 1)
            tl = tok.cpu().numpy().astype(np.int32) + 10
            U = max(17, int(tl.max()))
            tokens = torch.zeros((len(slots), U), dtype=torch.int32, device="cuda")
            w = min(U, ids.shape[1])
            tokens[:, :w] = ids[:, :w].clamp(min=0)
            return tr([tokens, batch], return_argmax=True, return_logits=False, token_lengths=torch.from_numpy(tl), enc_lengths=blen)

        def decode_padded():
            batch, _ = stream_gather(hist, hl, hl_host, list(range(N)), Tpad)
            _, fa = ctc(batch, return_argmax=True, return_logits=False)
            ids, tok = ctc_greedy_decode(fa, None, blank=V - 1)
            U = max(17, int(tok.max().item()) + 10)
            tokens = torch.zeros((N, U), dtype=torch.int32, device="cuda")
            w = min(U, ids.shape[1])
            tokens[:, :w] = ids[:, :w].clamp(min=0)
            return tr([tokens, batch], return_argmax=True, return_logits=False)

        def decode_loop():
            for p in pieces:
                e = torch.cat(p, 1)
                _, fa = ctc(e, return_argmax=True, return_logits=False)
                ids, tok = ctc_greedy_decode(fa, None, blank=V - 1)
                n = int(tok[0].item())
                tokens = torch.zeros((1, n + 10), dtype=torch.int32, device="cuda")
                tokens[:, :n] = ids[:, :n].clamp(min=0)
                tr([tokens, e], return_argmax=True, return_logits=False)

        every = list(range(N))
        out["decode_64"] = dict(frames=int(hl_host.sum()), Tpad=Tpad,
                                server_tick=timed(lambda: decode_batch(every), a.regions, a.iters),
                                padded_call=timed(decode_padded, a.regions, a.iters),
                                one_stream_at_a_time=timed(decode_loop, 3, 1))
        r = out["decode_64"]
        r["ragged_over_padded"] = r["server_tick"]["ms_median"] / r["padded_call"]["ms_median"]
        r["loop_over_ragged"] = r["one_stream_at_a_time"]["ms_median"] / r["server_tick"]["ms_median"]
        wav = torch.from_numpy(synth_batch(0, 16, chunk)).cuda()
        chunk_slots = [int(s) for s in np.argsort(hl_host)[:16]]
        decode_slots = [int(s) for s in rng.permutation(N)[:8]]
        keep, keep_dev = hl_host.copy(), hl.clone()

        def tick():
            e = enc(wav)
            stream_append(e, chunk_slots, hist, hl, hl_host)
            decode_batch(decode_slots)
            hl_host[:] = keep                                   # (the timing loop must not fill the histories)
            hl.copy_(keep_dev)

        out["tick_64"] = dict(chunks_due=16, decodes_due=8, tick=timed(tick, a.regions, a.iters))
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
