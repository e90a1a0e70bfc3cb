"""Ragged ChunkConformer batches on the MI355X: row b of every output of predict(wav_lengths=...) against
the float64 oracle run on wav[b, :L_b] alone, at 1e-3.

The test model is chunk_conformerS with two encoder blocks and 300 text classes.  The picks are driven by the picker's arg-max,
so every test that compares picks first asserts on the CPU that the oracle's top-two margin on every valid picker frame is at
least 10 x TOL; the weights get there by a bias of 20 on the picker's class 0 (chunk_ragged.weights), which leaves class 0 and
the blank as the only candidates of a frame.  Where all frames are to be picked the blank's bias is -20, so that the wav length
sets both the encoder length and the decoder length of a row exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_ragged as cr
from chunk_ragged import HOP, L_for, TOL
from helpers import chunk_config_dict, co

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
STAGES = ("front", "enc", "picker_logits", "picker_hidden", "picked", "helper", "text_logits", "text_argmax")
_STATE = {}


def _host(r):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _case(key):
    """(model, weights, cfg) of one of the three weight sets, made once per module"""
    if key not in _STATE:
        from tensorflowasr_amd.models import ChunkConformer
        if key == "all":                                   # every frame picked
            cfg = cr.config()
            w = cr.weights(cfg, 3, 20.0, -20.0)
        elif key == "wf80":                                # ... with a text decoder of win_front 80
            cfg = cr.config(decoder_win_front=80)
            w = cr.weights(cfg, 3, 20.0, -20.0)
        elif key == "picks":                               # the blank bias from the oracle's gaps: ragged pick counts
            cfg = cr.config()
            w = cr.weights(cfg, cr.RAGGED_SEED, 20.0, 0.0)
            gaps = []
            for x in cr.ragged_pick_rows():
                z = cr.alone(x, w, cfg, "gaps")["picker_logits"][0]
                gaps.append(z[:, 0] - z[:, -1])
            bias, dist = cr.ragged_pick_bias(gaps, cfg["decoder_win_back"])
            print("ragged picks: blank bias %.4f, %.3g from the nearest gap" % (bias, dist))
            assert dist >= cr.MARGIN
            w = cr.weights(cfg, cr.RAGGED_SEED, 20.0, bias)
        m = ChunkConformer(chunk_config_dict(cfg), cfg["picker_num_classes"], cfg["decoder_num_classes"])
        m.load_weights(w, by_name=False)
        _STATE[key] = (m, w, cfg)
    return _STATE[key]


def _edge(name, fill=np.nan):
    """one batch of the edge table: items, NaN-padded batch, lengths, the oracle alone, the ragged call's stages"""
    k = (name, "nan" if fill != fill else fill)
    if k not in _STATE:
        m, w, cfg = _case("all")
        items = cr.batch_items(cr.edge_batches()[name])
        refs = [cr.alone(it, w, cfg, "all") for it in items]
        x, lens = cr.padded(items, fill=fill)
        _STATE[k] = dict(items=items, refs=refs, x=x, lens=lens, got=_host(m.predict(x, stages=True, wav_lengths=lens)))
    return _STATE[k]


def _assert_regime(name, c, M):
    """launch counts of one ragged predict (mi355asr_profile_read): FFN launches of their own only on the layer-at-a-time path;
    on the fused paths the depthwise conv is a launch of its own exactly in the pair-pipelined kernels at 80 frames
    (pp_dw_fold_fits wants little padding to 64), the small-batch kernels of fused_ns.hip run it in their tail launch"""
    from caller_contract_gpu_steps import K_ATTN, K_DWCONV, K_FF1_QKV, K_FFN
    print("%s: %d rows, launch counts %s" % (name, M, c))
    assert c[K_ATTN] > 0                                   # band attention is always a launch of its own
    if name.startswith("layers"):
        assert M <= cr.SMALL_M and c[K_FFN] > 0 and c[K_FF1_QKV] == 0, ("layer-at-a-time", M, c)
    elif name.startswith("ns"):
        assert cr.SMALL_M < M <= cr.NS1_MAX_M and c[K_FFN] == 0 and c[K_FF1_QKV] > 0 and c[K_DWCONV] == 0, ("fused_ns", M, c)
    else:
        assert M > cr.NS1_MAX_M and c[K_FFN] == 0 and c[K_FF1_QKV] > 0 and c[K_DWCONV] > 0, ("fused_pp", M, c)


# ---- 1. edges, all frames picked, one batch per block regime ----------------------------------------------------------------------
def test_edge_table_covers_the_edges_the_parities_and_the_residues():
    b = cr.edge_batches()
    assert sorted(T for T, _, _ in b["ns-21x80"]) == cr.EDGE_T == sorted(T for T, _, _ in b["pp-52x80"][:21])
    assert not set(T for T, _, _ in b["pp-52x80"][21:]) & set(cr.EDGE_T)
    for name in ("ns-21x80", "pp-52x80"):
        assert {(p, r) for _, p, r in b[name]} == {(c[:2], c[2]) for c in cr.COMBOS}
    rows = {k: len(v) * max(T for T, _, _ in v) for k, v in b.items()}
    assert rows == {"layers-2x16": 32, "layers-3x15": 45, "layers-6x8": 48, "ns-21x80": 1680, "pp-52x80": 4160}
    small = {T for k in b if k.startswith("layers") for T, _, _ in b[k]}
    assert {1, 2, 7, 8, 9, 15, 16} <= small


@pytest.mark.parametrize("name", list(cr.edge_batches()))
def test_edge_lengths_against_the_oracle_alone(name):
    """T_b on win_back, win_front, their sum, the 16-row tile and the 64-query workgroup with their neighbours, in the four conv
    parities and three hop residues, NaN in the padding of wav: every stage of every row within 1e-3 of the oracle on the
    utterance alone, counts equal (= T_b), rows past a length exactly 0 / -1, nothing non-finite.  The block regime is asserted
    from the launch counts.  (layers-2x16 is also the <36, 1> launch shape of the band attention: at most 16 keys; the other
    batches run <36, 4, true>, the staged window.)"""
    from caller_contract_gpu_steps import profile_counts
    m, w, cfg = _case("all")
    r = _edge(name)
    cr.assert_picker_margin(r["refs"])
    B, Tmax = len(r["lens"]), max(T for T, _, _ in cr.edge_batches()[name])
    assert m.out_frames(r["x"].shape[1])[1] == Tmax and np.isnan(r["x"]).sum() == r["x"].size - int(r["lens"].sum())
    assert [ref["front"].shape[1] for ref in r["refs"]] == [T for T, _, _ in cr.edge_batches()[name]]
    assert [int(ref["counts"][0]) for ref in r["refs"]] == [T for T, _, _ in cr.edge_batches()[name]]      # every frame picked
    _assert_regime(name, profile_counts(m._h, lambda: m.predict(r["x"], stages=True, wav_lengths=r["lens"])), B * Tmax)
    cr.compare_with_oracle(r["got"], r["lens"], r["refs"], cfg, name)


# ---- 2. the other two launch shapes of the band attention --------------------------------------------------------------------------
def test_band_attention_with_key_blocks_of_256():
    """decoder_win_front = 80 and 100 picked frames in the longest row: the text decoder's sweep spans more than 96 keys, the
    <36, 16> launch shape (this one case needs more than the 80 frames of the other tests)"""
    m, w, cfg = _case("wf80")
    utts = cr.with_combos([100, 97, 96, 45, 9, 1], 4)
    items = cr.batch_items(utts)
    refs = [cr.alone(it, w, cfg, "wf80") for it in items]
    cr.assert_picker_margin(refs)
    assert max(int(r["counts"][0]) for r in refs) > 96 and min(cfg["decoder_win_front"] + cfg["decoder_win_back"] + 31, 100) > 96
    x, lens = cr.padded(items)
    cr.compare_with_oracle(_host(m.predict(x, stages=True, wav_lengths=lens)), lens, refs, cfg, "win_front 80")


def _run_step(name, seconds, env):
    cmd = [sys.executable, os.path.join(HERE, "chunk_ragged_gpu_steps.py"), name]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds, env=dict(os.environ, **env))
    print(r.stdout)
    assert r.returncode == 0, "step %s: exit status %d\n%s" % (name, r.returncode, r.stdout[-4000:])
    assert "step %s ok" % name in r.stdout


def test_band_attention_from_l2_in_a_child_process():
    """MI355ASR_ATTN_BAND_LDS=0 (read once per process): attention_kernel<36, 4> without the staged window"""
    _run_step("band_l2", 120, {"MI355ASR_ATTN_BAND_LDS": "0"})


# ---- 3. genuinely ragged picks -----------------------------------------------------------------------------------------------------
def _picks():
    if "picks-run" not in _STATE:
        m, w, cfg = _case("picks")
        items = cr.ragged_pick_rows()
        refs = [cr.alone(it, w, cfg, "picks") for it in items]
        x, lens = cr.padded(items)
        assert not np.isnan(x).any() and len(set(lens.tolist())) == 1        # an equal-length batch
        _STATE["picks-run"] = dict(items=items, refs=refs, x=x, lens=lens, got=_host(m.predict(x, stages=True, wav_lengths=lens)),
                                   plain=_host(m.predict(x, stages=True)))
    return _STATE["picks-run"]


def test_ragged_pick_counts_against_the_oracle_alone():
    """one row without a pick, one with fewer than win_back, the others with some but not all of their frames: counts, picked,
    helper and text logits equal the oracle alone.  The call WITHOUT lengths on the same batch is more than 10 x TOL from the
    oracle alone on some row: the batch dependence the feature removes."""
    m, w, cfg = _case("picks")
    r = _picks()
    cr.assert_picker_margin(r["refs"])
    counts = [int(ref["counts"][0]) for ref in r["refs"]]
    wb = cfg["decoder_win_back"]
    print("pick counts", counts)
    assert counts.count(0) == 1 and any(0 < c < wb for c in counts) and all(c < cr.RAGGED_T for c in counts)
    cr.compare_with_oracle(r["got"], r["lens"], r["refs"], cfg, "ragged picks")
    assert np.array_equal(r["plain"]["counts"], np.array(counts))
    worst = 0.0
    for b, ref in enumerate(r["refs"]):
        if counts[b]:
            worst = max(worst, float(np.abs(r["plain"]["text_logits"][b, :counts[b]] - ref["text_logits"][0]).max()))
    print("predict without lengths: max|text logits - oracle alone| = %.3g" % worst)
    assert worst > 10 * TOL


# ---- 4. bit-identity ----------------------------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s differs in %d words" % (what, int((a != b).sum()))


def test_padding_content_changes_no_bit():
    """the edge batch with NaN and with zeros behind every utterance: all outputs bit-identical"""
    a, b = _edge("ns-21x80")["got"], _edge("ns-21x80", 0.0)["got"]
    for k in STAGES + ("counts",):
        _same_bits(a[k], b[k], k)


def test_other_rows_change_no_bit_of_a_row():
    """audio and length of every row replaced except the longest (it sets Tp and with it the kernels) and a probe row: the probe
    row's outputs are bit-identical"""
    m, w, cfg = _case("all")
    r = _edge("ns-21x80")
    keep, probe = 0, 5
    assert r["lens"][keep] == r["lens"].max()
    items = list(r["items"])
    for b in range(len(items)):
        if b not in (keep, probe):
            items[b] = cr.utterance(L_for(3 + (7 * b) % 70, cr.PARITIES[b % 4], cr.RESIDUES[b % 3]), 300 + b)
    x, lens = cr.padded(items, L=r["x"].shape[1])
    got = _host(m.predict(x, stages=True, wav_lengths=lens))
    assert got["text_logits"].shape == r["got"]["text_logits"].shape
    for k in STAGES:
        _same_bits(got[k][probe], r["got"][k][probe], k)
        _same_bits(got[k][keep], r["got"][k][keep], k)


def test_all_lengths_equal_to_L_is_the_call_without_lengths_up_to_the_picker():
    """every length = L: front, encoder and picker are bit-identical between predict and the ragged call (the call without
    lengths computes what it did: behind the picks the two differ by design)"""
    r = _picks()
    for k in ("front", "enc", "picker_hidden", "picker_logits", "counts"):
        _same_bits(r["got"][k], r["plain"][k], k)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_row_or_field_and_write_nothing():
    import ctypes
    import torch
    from caller_contract_gpu_steps import conformer_ctc
    from tensorflowasr_amd import _lib
    m, w, cfg = _case("all")
    h = m._h
    B, L = 3, 4000
    T = m.out_frames(L)[1]
    d, V, P = cfg["dmodel"], cfg["decoder_num_classes"], cfg["picker_num_classes"]
    x = torch.zeros((B, L), device=h.device)
    n = ctypes.c_size_t()
    _lib.check(h.lib.mi355asr_chunk_workspace_bytes_ragged(h.ptr, B, L, ctypes.byref(n)))
    plain = ctypes.c_size_t()
    _lib.check(h.lib.mi355asr_chunk_workspace_bytes(h.ptr, B, L, ctypes.byref(plain)))
    assert n.value >= plain.value
    ws = torch.full((n.value,), 0x5A, dtype=torch.uint8, device=h.device)
    SENT = 123.0
    bufs = {k: torch.full((B, T, c), SENT, device=h.device) for k, c in (("front_out", d), ("enc_out", d), ("picker_hidden", d), ("picked", d),
                                                                             ("helper_out", d), ("picker_logits", P), ("text_logits", V))}
    bufs["text_argmax"] = torch.full((B, T), 123, dtype=torch.int32, device=h.device)
    outs = _lib.ChunkOutputs(**{k: v.data_ptr() for k, v in bufs.items()})
    counts = np.full(B, 123, np.int32)
    tp = ctypes.c_int32(123)

    def call(handle, lens):
        wl = torch.tensor(lens, dtype=torch.int32, device=h.device) if lens is not None else None
        with torch.cuda.device(h.device):
            rc = h.lib.mi355asr_chunk_predict_ragged(handle, x.data_ptr(), wl.data_ptr() if wl is not None else None, B, L, ctypes.byref(outs),
                                                     counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tp), ws.data_ptr(), n.value, h._stream())
        torch.cuda.synchronize()
        return rc, h.lib.mi355asr_last_error().decode()

    other = conformer_ctc()[0]
    other.encode(np.zeros((1, 8000), np.float32))                          # (built and finalised)
    cases = [("length 0", h.ptr, [L, 0, L], "wav_len[1]"), ("length L + 1", h.ptr, [L, L, L + 1], "wav_len[2]"),
             ("length 2 hop", h.ptr, [2 * HOP, L, L], "wav_len[0]"), ("null lengths", h.ptr, None, "wav_len"),
             ("a ConformerCTC handle", other._h.ptr, [L, L, L], "ChunkConformer handle")]
    for what, handle, lens, field in cases:
        rc, msg = call(handle, lens)
        print("%s: %d %s" % (what, rc, msg))
        assert rc == -1 and field in msg, (what, rc, msg)                  # MI355ASR_EINVAL
        for k, v in bufs.items():
            assert bool((v == (123 if k == "text_argmax" else SENT)).all()), (what, k, "written")
        assert (counts == 123).all() and tp.value == 123 and bool((ws == 0x5A).all()), (what, "host outputs or workspace written")
    rc, msg = call(h.ptr, [2 * HOP + 1, L, 1000])                          # the shortest length that is taken
    assert rc == 0, msg
    assert counts.tolist() == [1, T, m.out_frames(1000)[1]]


def test_layer_at_a_time_gemm_mode_is_refused_in_a_child_process():
    """MI355ASR_GEMM16=1 (read once per process) puts every block on the GEMM family that bf16 mode uses, which applies no lengths:
    EINVAL before anything is launched.  (A ChunkConformer handle cannot be put into bf16 mode itself: mi355asr_chunk_config has
    no gemm_dtype.)"""
    _run_step("gemm16", 120, {"MI355ASR_GEMM16": "1"})


# ---- 6. the driver surface ------------------------------------------------------------------------------------------------------------
def _asr(tmp_path, beam):
    from beam_lm_gpu_steps import ARPA, _chunk_setup
    from tensorflowasr_amd.chunk_asr import ChunkASR
    cfg, conf = _chunk_setup(str(tmp_path))
    if beam > 1:
        conf["tar_config"]["beam_width"] = beam
        chars = ["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4E00 + 7 * i) for i in range(36)]
        with open(conf["tar_config"]["vocabulary"], "w", encoding="utf-8") as f:
            f.write("\n".join(chars) + "\n")
        conf["tar_config"]["lm_config"] = {"lm_path": ARPA[3], "alpha": 0.6, "beta": 0.5}
    asr = ChunkASR(conf, load_checkpoint=False)
    w = co.chunk_weights(cfg, seed=3)
    x = np.stack([co.synth_wave(5 + i, 2560 * 12) for i in range(2)])
    from helpers import pick_bias_for_ragged_counts
    w["picker/fully_connected/bias"][-1] = pick_bias_for_ragged_counts(cfg, w, x)
    asr.runner.load_weights(w, by_name=False)
    return asr


def _six():
    sizes = [2560 * 12, 2560 * 9 + 77, 2560 * 5 + 1234, 2560 * 11 - 700, 2560 * 3 + 1, 2560 * 7]
    return [(0.5 + 0.1 * i) * co.synth_wave(20 + i, n) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("beam", [1, 4])
def test_offline_stt_batch_equals_one_item_at_a_time(tmp_path, beam):
    """six waveforms of different lengths in one ragged batch, and in two: the texts of the six decoded one at a time (the ragged
    call with B = 1), greedy and with beam_width 4 + tests/golden/lm_small.arpa"""
    asr = _asr(tmp_path, beam)
    assert (asr.text_featurizer.scorer is not None) == (beam > 1)
    items = _six()
    want = [asr.offline_stt_batch([it])[0] for it in items]
    print(want)
    assert any(want)
    assert asr.offline_stt_batch(items) == want
    assert asr.offline_stt_batch(items, max_batch_samples=3 * 2560 * 12) == want


def test_offline_stt_batch_resamples_on_the_device(tmp_path):
    """sample_rates=[8000, None, ...]: what resampling the first item on the host side first gives"""
    from tensorflowasr_amd.resample import Resampler
    asr = _asr(tmp_path, 1)
    items = _six()
    x8 = co.synth_wave(31, 12000).astype(np.float32)
    y, n = Resampler(8000, 16000, device=asr.device)(x8[None], np.array([len(x8)], np.int32))
    y16 = y[0, :int(n[0])].cpu().numpy()
    want = asr.offline_stt_batch([y16] + items[1:])
    got = asr.offline_stt_batch([x8] + items[1:], sample_rates=[8000] + [None] * 5)
    print(got)
    assert got == want and any(got)


def test_beam_pipeline_takes_lengths(tmp_path):
    """ChunkBeamPipeline.push(wav, wav_lengths) + flush(): bit for bit ctc_prefix_beam_decode(logits, counts) on the ragged logits"""
    from tensorflowasr_amd.models import ChunkBeamPipeline, ctc_prefix_beam_decode
    asr = _asr(tmp_path, 4)
    m, s = asr.runner, asr.text_featurizer.scorer
    x, lens = cr.padded(_six()[:4])
    pipe = ChunkBeamPipeline(m, beam_width=4, cutoff_prob=0.99, cutoff_top_n=40, ext_scorer=s)
    assert pipe.push(x, wav_lengths=lens) is None
    res = pipe.flush()
    pipe.close()
    logits, counts = m.predict(x, wav_lengths=lens)
    seq = ctc_prefix_beam_decode(logits, counts, 4, 0.99, 40, is_logits=True, ext_scorer=s)
    for a, b in zip(res, seq):
        _same_bits(np.asarray(a), np.asarray(b), "pipeline")
    assert int(np.asarray(seq[1])[:, 0].max()) > 0
