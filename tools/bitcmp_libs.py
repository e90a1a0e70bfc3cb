"""Bitwise comparison of two builds of the library: `python tools/bitcmp_libs.py LIB_A.so LIB_B.so` runs every host path of the
library once per build, each in its own process (MI355ASR_LIB; "default" = the in-tree build), and prints one JSON line per build
with a SHA-1 of every output and the value of every *_workspace_bytes call; equal lines (the "lib" entry aside) = builds that
compute the same bits from the same workspaces.  The exit status is 1 when two lines differ.

Covered, all on seeded inputs (tensorflowasr_amd.synthetic, the builders of bench.py / tests): ConformerCTC(S) fp32 at 64 x 10 s
(pair-pipelined blocks, deferred Dense, head in the tail launch), 8 x 10 s (small-batch kernels), one utterance of 45 encoder rows
(layer-at-a-time launches) and a ragged batch of 8; the LEAF, Spectrogram and add_wav_info fronts; ConformerM / ConformerL fp32;
config 3 (streaming dmodel 256 in bf16 + the stand-alone CTCDecoder, solo and ragged); ChunkConformer.predict with every stage
output plus streaming steps through picker_stream_predict / decoder_stream_predict; the Translator solo and ragged.

`BITCMP_CHILD=1 python tools/bitcmp_libs.py` is the per-build child on its own (the program to put behind a profiler's `--`)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys


def child():
    import numpy as np
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from bench import build_model
    from helpers import chunk_config_dict
    from oracle import conformer_oracle as co
    from tensorflowasr_amd.models import ChunkConformer, ConformerCTC, CTCDecoder, StreamingConformerEncoder, Translator
    from tensorflowasr_amd.synthetic import synth_batch
    dev = torch.device("cuda", 0)
    out = {"lib": os.path.basename(os.path.dirname(os.environ.get("MI355ASR_LIB", ""))) or "default"}

    def sha(t):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

    def nbytes(h, fn, *args):
        n = ctypes.c_size_t()
        rc = getattr(h.lib, fn)(h.ptr, *args, ctypes.byref(n))
        return n.value if rc == 0 else "error %d" % rc

    def wave(B, L, seed=0):
        return torch.from_numpy(synth_batch(seed, B, L)).to(dev)

    def ctc_model(m, x, lengths=None):
        """recognize, encoder output, logits and arg-max of a ConformerCTC on x (ragged with lengths), and its workspaces"""
        B, L = x.shape
        r = {"ws": nbytes(m._h, "mi355asr_workspace_bytes", B, L), "ws_ctc": nbytes(m._h, "mi355asr_ctc_workspace_bytes", B, m.out_frames(L))}
        ids, lens = m.recognize(x, wav_lengths=lengths)
        enc = m.encode(x, lengths=lengths)
        enc, enc_len = enc if lengths is not None else (enc, None)
        logits, amax = m.ctc_logits(enc, return_argmax=True, lengths=enc_len)
        r.update(ids=sha(ids), lens=sha(lens), enc=sha(enc), logits=sha(logits), argmax=sha(amax))
        if enc_len is not None:
            r["enc_len"] = sha(enc_len)
        return r, enc, ids

    # ---- ConformerCTC(S), fp32: the headline model
    m = build_model(dev, 0, 1)
    out["S_64x10s"], enc64, ids64 = ctc_model(m, wave(64, 160000))
    out["S_8x10s"], enc8, ids8 = ctc_model(m, wave(8, 160000))
    out["S_1x1.8s"], _, _ = ctc_model(m, wave(1, 28800))
    ragged = np.array([160000, 120000, 96000, 150000, 64000, 80000, 112000, 40000], np.int32)
    out["S_ragged8"], _, _ = ctc_model(m, wave(8, 160000), lengths=ragged)
    del m
    # ---- the other fronts and model sizes (random init)
    for name, kw in (("S_leaf", dict(mel_layer_type="leaf")), ("S_spectrogram", dict(mel_layer_type="Spectrogram")),
                     ("S_wavinfo", dict(add_wav_info=True)), ("M", dict(dmodel=256, num_blocks=13, head_size=64, num_heads=4)),
                     ("L", dict(dmodel=512, num_blocks=13, head_size=64, num_heads=8))):
        m = ConformerCTC(1332, **kw)
        m._build()
        out[name + "_8x10s"], _, _ = ctc_model(m, wave(8, 160000))
        del m
        torch.cuda.empty_cache()
    # ---- config 3: streaming dmodel 256 in bf16 and the stand-alone CTCDecoder over 10 s of history, solo and ragged
    enc = StreamingConformerEncoder(dmodel=256, reduction_factor=4, num_blocks=4, head_size=64, num_heads=4, kernel_size=5, fc_factor=0.5,
                                    sample_rate=16000, n_mels=80, stride_ms=10, mel_layer_type="Melspectrogram", gemm_dtype="bfloat16")
    enc.add_chunk_size(8000, 80, 640)
    enc._build(seed=0)
    ctc = CTCDecoder(num_classes=1332, dmodel=256, num_blocks=1, head_size=64, num_heads=4, kernel_size=32, fc_factor=0.5, gemm_dtype="bfloat16")
    ctc._build(seed=1)
    e = enc(wave(64, 8000))
    hist = torch.cat([torch.from_numpy(np.random.RandomState(0).randn(64, 19 * 13, 256).astype(np.float32)).to(dev), e], 1)
    logits, amax = ctc(hist, return_argmax=True)
    hl = (20 * 13 - 3 * (np.arange(64) % 40)).astype(np.int32)
    rl, ra = ctc(hist, return_argmax=True, lengths=hl)
    out["config3"] = {"ws": nbytes(enc._h, "mi355asr_workspace_bytes", 64, 8000), "ws_ctc": nbytes(ctc._h, "mi355asr_ctc_workspace_bytes", 64, 260),
                      "enc": sha(e), "logits": sha(logits), "argmax": sha(amax), "ragged_logits": sha(rl), "ragged_argmax": sha(ra)}
    del enc, ctc
    # ---- ChunkConformer: offline predict with every stage, and the streaming entry points chunk by chunk
    cfg = dict(co.CHUNK_S)
    w = co.chunk_weights(cfg, seed=0, picker_blank_bias=0.0)
    m = ChunkConformer(chunk_config_dict(cfg), phone=cfg["picker_num_classes"], txt=cfg["decoder_num_classes"])
    m.load_weights(w, by_name=False)
    x = wave(4, 160000)
    r = m.predict(x, stages=True)
    out["chunk_predict"] = dict({k: sha(v) for k, v in r.items()}, ws=nbytes(m._h, "mi355asr_chunk_workspace_bytes", 4, 160000))
    logits, counts = m.predict(wave(16, 480000))                # the front's Dense deferred to the encoder's first block
    out["chunk_predict_16x30s"] = {"text_logits": sha(logits), "counts": sha(counts), "ws": nbytes(m._h, "mi355asr_chunk_workspace_bytes", 16, 480000)}
    caches, caches2, st = m.init_picker_caches(1), m.init_decoder_caches(1), {}
    for i in range(4):
        vp, unv, vh, caches = m.picker_stream_predict(x[:1, i * 2560:(i + 1) * 2560, None], caches)
        st["picker%d" % i] = [sha(vp), sha(unv), sha(vh)]
        if vh.shape[1]:
            vt, unv2, caches2 = m.decoder_stream_predict(vh, caches2)
            st["decoder%d" % i] = [sha(vt), sha(unv2)]
    st["caches"] = [sha(c) for c in caches + caches2]
    st["ws"] = nbytes(m._h, "mi355asr_chunk_stream_workspace_bytes", 64, 5120, 4, 16)
    out["chunk_stream"] = st
    del m
    # ---- Translator over the S model's encoder output and phone ids: 64 x 10 s solo (class head split over ranges), 8 ragged
    tr = Translator(inp_classes=1332, tar_classes=9160, dmodel=144, num_blocks=2, head_size=36, num_heads=4, kernel_size=32, fc_factor=0.5)
    tr._build(seed=2)
    ph64, ph8 = ids64[:, :40].clamp(min=0).contiguous(), ids8[:, :40].clamp(min=0).contiguous()
    logits, amax = tr([ph64, enc64], return_argmax=True)
    _, amax_only = tr([ph64, enc64], return_argmax=True, return_logits=False)
    tl, el = np.array([40, 17, 33, 25, 40, 21, 38, 29], np.int32), np.array([250, 100, 180, 240, 64, 125, 200, 90], np.int32)
    rl, ra = tr([ph8, enc8], return_argmax=True, token_lengths=tl, enc_lengths=el)
    out["translator"] = {"ws": nbytes(tr._h, "mi355asr_translator_workspace_bytes", 64, 40, 250), "ws_ragged": nbytes(tr._h, "mi355asr_translator_workspace_bytes", 8, 40, 250),
                         "logits": sha(logits), "argmax": sha(amax), "argmax_only": sha(amax_only), "ragged_logits": sha(rl), "ragged_argmax": sha(ra)}
    torch.cuda.synchronize()
    print(json.dumps(out, sort_keys=True), flush=True)


def main():
    lines = []
    for lib in sys.argv[1:] or ["default"]:
        env = dict(os.environ, BITCMP_CHILD="1")
        if lib != "default":
            env["MI355ASR_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
        line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else None
        print(line or "%s: child failed (exit %d)\n%s" % (lib, r.returncode, r.stderr[-2000:]), flush=True)
        if line is None:
            return 2                                  # nothing more is started after a failed child
        lines.append({k: v for k, v in json.loads(line).items() if k != "lib"})
    same = all(l == lines[0] for l in lines)
    if len(lines) > 1:
        diff = sorted(k for l in lines[1:] for k in l if l[k] != lines[0].get(k))
        print("EQUAL: every hash and every byte count" if same else "DIFFERENT: %s" % ", ".join(diff), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    if os.environ.get("BITCMP_CHILD"):
        child()
    else:
        sys.exit(main())
