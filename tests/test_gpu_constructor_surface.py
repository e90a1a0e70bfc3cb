"""Every constructor value outside the shipped configs, on the MI355X: the head sizes, kernel sizes, reduction factors, mel bins,
hops and dmodel values that mi355asr_create / mi355asr_translator_create take and that run on general kernels nobody benchmarks
(attention_kernel<HS, KT>, dwconv_any_kernel, subconv_split_kernel<4, ST1>, the generic subsampling and ring packs of
dmodel % 128 == 0, the 128-bin mel kernels), at the shapes where those kernels change path: across their key blocks and query
workgroups, with taps wholly in the padding, at every remainder of the conv1 stride, at the row counts where a launcher switches
families.

Every comparison is GPU float32 against the float64 oracle on the same inputs and is held to the 1e-3 contract and to
max(8 x E32, 16 ulp of max|ref|), E32 being the oracle's own float32 error measured in the test (tests/surface_yardstick.py).
The comparisons have no entry in tests/golden/parity_ceilings.json: they are logged there, and bounded here.  Models are built once
per configuration and the shapes loop inside a test."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import co, encoder_kwargs, small_cfg, waves
from surface_yardstick import Ledger, waveform_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_models = {}


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_fault = []


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault(torch_cuda):
    """a HIP error is sticky: once the device has faulted (here, or in a step's own process) no later test launches anything"""
    assert not _fault, "not started: %s ended with %s" % tuple(_fault[0])
    yield
    try:
        torch_cuda.cuda.synchronize()
    except Exception as e:
        _fault.append(("an earlier test of this file", str(e)[:300]))
        raise


def _block_model(dm, H, hs, k, gemm_dtype="float32"):
    """ConformerCTC with ONE encoder block (and the CTC decoder the class needs), built once per configuration"""
    key = ("block", dm, H, hs, k, gemm_dtype)
    if key not in _models:
        from tensorflowasr_amd.models import ConformerCTC
        cfg = dict(co.CONFORMER_S, dmodel=dm, num_heads=H, head_size=hs, kernel_size=k, num_blocks=1)
        w = co.encoder_weights(cfg, seed=7)
        w.update(co.ctc_decoder_weights(cfg, 40, seed=8))
        m = ConformerCTC(40, dmodel=dm, num_blocks=1, head_size=hs, num_heads=H, kernel_size=k, gemm_dtype=gemm_dtype)
        m.load_weights(w, by_name=False)
        _models[key] = (m, w, cfg)
    return _models[key]


def _block_refs(x, w, cfg):
    r64 = co.conformer_block(x.astype(np.float64), w, "conformer_block_0", cfg["head_size"], cfg["fc_factor"])
    r32 = co.conformer_block(x, w, "conformer_block_0", cfg["head_size"], cfg["fc_factor"])
    return r64, r32


# ---- 1. every attention instantiation across its own block boundaries ------------------------------------------------------------
ATTN_T = (1, 13, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)


@pytest.mark.parametrize("hs,dm,H", [(12, 144, 12), (16, 144, 9), (16, 256, 16), (24, 144, 6), (32, 256, 8), (32, 128, 4), (48, 144, 3),
                                     (48, 384, 8), (72, 144, 2), (128, 512, 4), (128, 1024, 8)])
def test_attention_instantiations_across_key_blocks_and_query_workgroups(hs, dm, H):
    """attention_kernel<12 / 16 / 24 / 32 / 48, 4> (64-key blocks), <72, 2> (32) and <128, 1> (16) inside one block (kernel size 32) on
    caller tensors [2, T, dmodel]: T around the 16-query tile and the 64-query workgroup, and one, two and four key blocks with the
    last one full, short by one and over by one -- the `alpha` rescale of the online softmax, the prefetch of the next key block
    and a second workgroup along the queries."""
    m, w, cfg = _block_model(dm, H, hs, 32)
    led = Ledger("attention")
    for T in ATTN_T:
        x = np.random.default_rng(1000 * hs + T).standard_normal((2, T, dm)).astype(np.float32)
        r64, r32 = _block_refs(x, w, cfg)
        led.add("hs%d %dx%d T%d" % (hs, dm, H, T), m.conformer_block(0, x).cpu().numpy(), r64, r32)
    led.close()


# ---- 2. every depthwise-conv regime ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dm,H,hs", [(144, 4, 36), (256, 4, 64)])
@pytest.mark.parametrize("k", [1, 2, 3, 6, 31, 33, 64, 255, 256, 1024])
def test_depthwise_conv_kernel_sizes_against_every_length(dm, H, hs, k):
    """dwconv_any_kernel under the tuned attention (head size 36 / 64): kernel sizes even and odd, each with K < T, K = T +- 1 and
    K > 2 T (taps that lie wholly in the padding; even sizes pad (K - 1) // 2 in front), up to the documented 1024."""
    m, w, cfg = _block_model(dm, H, hs, k)
    led = Ledger("dwconv")
    for T in (1, 8, 31, 32, 33, 65):
        x = np.random.default_rng(100 * k + T).standard_normal((2, T, dm)).astype(np.float32)
        r64, r32 = _block_refs(x, w, cfg)
        led.add("%dx%d k%d T%d" % (dm, hs, k, T), m.conformer_block(0, x).cpu().numpy(), r64, r32)
    led.close()


@pytest.mark.parametrize("k", [7, 32])
def test_depthwise_conv_at_the_row_count_where_the_launcher_switches_families(k):
    """launch_dwconv takes the LDS-tiled kernels from 2 048 rows on: B = 33, T = 65 (2 145 rows) at dmodel 144 for kernel size 32
    (dwconv_tile_kernel<32, 144> where a launch of its own runs it) and 7 (still dwconv_any_kernel)."""
    m, w, cfg = _block_model(144, 4, 36, k)
    led = Ledger("dwconv")
    x = np.random.default_rng(k).standard_normal((33, 65, 144)).astype(np.float32)
    r64, r32 = _block_refs(x, w, cfg)
    led.add("144x36 k%d B33 T65" % k, m.conformer_block(0, x).cpu().numpy(), r64, r32)
    led.close()


# ---- 3. the paths a model takes, from the waveform -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dm,H,hs,k,ctc_k,B,L,T", [
    (1, 144, 9, 16, 32, 32, 2, 48160, 76),      # the one-tile-per-workgroup tail with its own attention launch, two key blocks
    (2, 144, 9, 16, 32, 32, 56, 48160, 76),     # 4 256 rows: the pair-pipelined kernels
    (3, 144, 4, 36, 7, 7, 2, 48160, 76),
    (4, 144, 4, 36, 7, 7, 56, 48160, 76),       # 4 256 rows
    (5, 144, 3, 48, 64, 5, 2, 16000, 25),       # K > T; the decoder on another kernel size than the encoder
    (6, 144, 12, 12, 1, 1, 1, 7000, 11),        # the layer-at-a-time path of very few rows
    (7, 128, 4, 32, 9, 9, 2, 16000, None),
    (7, 384, 8, 48, 32, 32, 2, 41600, 65),
    (7, 640, 10, 64, 5, 5, 2, 16000, None),
    (7, 768, 12, 64, 32, 32, 2, 16000, None),
    (7, 896, 7, 128, 3, 3, 1, 16000, None),
    (7, 1024, 8, 128, 33, 33, 1, 41600, None)])
def test_model_paths_from_the_waveform(case, dm, H, hs, k, ctc_k, B, L, T):
    """ConformerCTC(70, one encoder block, the CTC decoder): waveform -> encoder -> logits -> greedy ids.  The oracle runs on the
    first two utterances."""
    led = Ledger("waveform")
    frames = waveform_case(led, "case%d %d %dx%d k%d B%d" % (case, dm, H, hs, k, B), dm, H, hs, k, B, L, ctc_k=ctc_k)
    assert T is None or frames == T, (frames, T)
    led.close()


def _run_step(name, seconds, env):
    """a step of constructor_surface_gpu_steps.py in a process of its own under its own time limit; one that ends in a signal, an
    abort or its limit is not run again and nothing is started after it (tests/test_gpu_beam_streams.py: run_step)"""
    cmd = [sys.executable, os.path.join(HERE, "constructor_surface_gpu_steps.py"), name]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=seconds, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired as e:
        _fault.append((name, "its time limit of %d s" % seconds))
        print(e.stdout)
        raise AssertionError("step %s %s did not finish in %d s" % (name, env, seconds))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _fault.append((name, "exit status %d" % r.returncode))
    assert r.returncode == 0, "step %s %s: exit status %d\n%s" % (name, env, r.returncode, r.stdout[-3000:])
    assert "step %s ok" % name in r.stdout


@pytest.mark.parametrize("env", [{"MI355ASR_RING_MIN_M": "1", "MI355ASR_RING_RT": "1"}, {"MI355ASR_RING_MIN_M": "1", "MI355ASR_RING_RT": "2"},
                                 {"MI355ASR_GEMM_RING": "0"}], ids=["ring_rt1", "ring_rt2", "ring_off"])
def test_ring_kernels_of_dmodel_128_and_384_in_a_fresh_process(env):
    """case 8: the slab-ring kernels forced for a small batch, with one and with two row tiles per wave, and the fp32 kernels they
    replace -- dmodel 128 and 384 as in case 7 (test_ring_gemm_path_of_m_and_l_in_a_subprocess covers 256 and 512)"""
    _run_step("ring", 240, env)


def test_bf16_block_at_dmodel_384_matches_the_rounding_oracle():
    """case 9: one block of dmodel 384 (8 x 48) in bf16 mode on an exact fp32 input [5, 77, 384] against the oracle with both GEMM
    operands rounded to bf16: the bounds of test_bf16_block_matches_rounding_oracle (tie flips: max < 6e-3, mean < 3e-4)."""
    m, w, cfg = _block_model(384, 8, 48, 32, gemm_dtype="bfloat16")
    x = np.random.default_rng(2).standard_normal((5, 77, 384)).astype(np.float32)
    got = m.conformer_block(0, x).cpu().numpy()
    co.GEMM_ROUND_BF16 = True
    try:
        ref = co.conformer_block(x.astype(np.float64), w, "conformer_block_0", 48, cfg["fc_factor"])
    finally:
        co.GEMM_ROUND_BF16 = False
    exact = co.conformer_block(x.astype(np.float64), w, "conformer_block_0", 48, cfg["fc_factor"])
    e = np.abs(got - ref)
    print("SURFACE bf16 384 8x48 [5, 77]: vs rounding oracle max %.3g mean %.3g (vs exact: max %.3g)" % (e.max(), e.mean(), np.abs(got - exact).max()))
    assert e.max() < 6e-3 and e.mean() < 3e-4
    assert np.abs(got - exact).max() > 10 * e.mean()               # it really is the bf16 path


# ---- 4. frontend and subsampling outside 80 bins, hop 160, factor 4 ---------------------------------------------------------------
def _encoder(**over):
    key = ("enc",) + tuple(sorted(over.items()))
    if key not in _models:
        from tensorflowasr_amd.models import ConformerEncoder
        cfg = dict(small_cfg(1), **over)
        w = co.encoder_weights(cfg, seed=3)
        e = ConformerEncoder(**encoder_kwargs(cfg))
        e.load_weights(w, by_name=False)
        _models[key] = (e, w, cfg)
    return _models[key]


@pytest.mark.parametrize("over,hop", [(dict(n_mels=128), 160), (dict(sample_rate=8000), 80), (dict(stride_ms=20), 320)],
                         ids=["n_mels128", "sr8000_hop80", "stride20_hop320"])
def test_melspectrogram_at_128_bins_and_other_hops(over, hop):
    """the 128-bin mel kernels (launch_mel_band sits on its own limit there) and hops of 80 and 320 samples: the lengths of
    test_melspectrogram_parity and L = 50 hop +- 1.  8 x E32 is of the order of the contract here, and the contract binds."""
    e, w, cfg = _encoder(**over)
    led = Ledger("mel")
    for L in (32000, 67263, 1000, 16160, 50 * hop - 1, 50 * hop + 1):
        x = waves(2, L, 5)
        got = e.melspectrogram(x).cpu().numpy()
        assert got.shape == (2, -(-L // hop), cfg["n_mels"])
        led.add("%s L%d" % (",".join("%s=%s" % kv for kv in over.items()), L), got, co.melspectrogram(x.astype(np.float64), w, hop=hop),
                co.melspectrogram(x, w, hop=hop, dtype=np.float32))
    led.close()


def _subsampling(led, e, w, rf, nm, F, tag):
    mel = (-80 * np.random.default_rng(F).random((3, F, nm))).astype(np.float32)
    got = e.conv_subsampling(mel).cpu().numpy()
    st1 = rf // 2
    assert got.shape[1] == -(-(-(-F // st1)) // 2), (F, got.shape)
    led.add("%s F%d" % (tag, F), got, co.conv_subsampling(mel.astype(np.float64), w, reduction_factor=rf),
            co.conv_subsampling(mel, w, reduction_factor=rf))


def test_conv_subsampling_at_128_bins():
    e, w, cfg = _encoder(n_mels=128)
    led = Ledger("subsampling")
    for F in (200, 50, 37, 3):
        _subsampling(led, e, w, 4, 128, F, "n_mels128 rf4")
    led.close()


@pytest.mark.parametrize("dm,H,hs", [(144, 4, 36), (256, 4, 64)])
@pytest.mark.parametrize("rf", [2, 6, 8])
def test_conv_subsampling_at_reduction_factors_other_than_4(rf, dm, H, hs):
    """subconv_split_kernel<4, ST1> (conv1 time stride 1, 3, 4; mel window 2 ST1 + 3 rows): F with every remainder modulo 1, 3 and
    4, odd and even T1, F below the row window, and the frame count ceil(ceil(F / st1) / 2)."""
    e, w, cfg = _encoder(reduction_factor=rf, dmodel=dm, num_heads=H, head_size=hs)
    led = Ledger("subsampling")
    for F in (1, 2, 3, 4, 5, 7, 9, 10, 11, 12, 13, 37, 50, 199, 200, 201, 202):
        _subsampling(led, e, w, rf, 80, F, "rf%d d%d" % (rf, dm))
    led.close()


@pytest.mark.parametrize("rf", [2, 6, 8])
def test_128_bins_from_the_waveform_at_every_reduction_factor(rf):
    led = Ledger("waveform")
    waveform_case(led, "n_mels128 rf%d" % rf, 144, 4, 36, 32, 2, 16000 - 77, reduction_factor=rf, n_mels=128)
    led.close()


# ---- 5. Translator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dm,H,hs,k,shapes", [(144, 3, 48, 7, ((19, 77), (65, 130), (1, 13))), (256, 16, 16, 33, ((19, 77), (65, 130), (1, 13))),
                                              (144, 2, 72, 32, ((17, 33),))])
def test_translator_cross_attention_on_the_general_instantiations(dm, H, hs, k, shapes):
    """Translator(60 -> 75 classes, one RBlock): cross-attention (Tq = U tokens, Tk = T encoder frames) on attention_kernel<48, 4>,
    <16, 4> and <72, 2>, with one and with several key blocks, and the general depthwise conv over the token stream."""
    from tensorflowasr_amd.models import Translator
    cfg = dict(co.CONFORMER_S, dmodel=dm, num_heads=H, head_size=hs, translator_num_blocks=1, translator_kernel_size=k, translator_fc_factor=0.5)
    w = co.translator_weights(cfg, 60, 75, seed=9)
    tr = Translator(inp_classes=60, tar_classes=75, dmodel=dm, num_blocks=1, head_size=hs, num_heads=H, kernel_size=k)
    tr.load_weights(w, by_name=False)
    led = Ledger("translator")
    for U, T in shapes:
        rng = np.random.default_rng(100 * U + T)
        ids = rng.integers(0, 60, (2, U)).astype(np.int32)
        enc = rng.standard_normal((2, T, dm)).astype(np.float32)
        got, amax = tr([ids, enc], return_argmax=True)
        got = got.cpu().numpy()
        led.add("%d %dx%d k%d U%d T%d" % (dm, H, hs, k, U, T), got, co.translator(ids, enc.astype(np.float64), w, cfg),
                co.translator(ids, enc, w, cfg, dtype=np.float32))
        assert (amax.cpu().numpy() == got.argmax(-1)).all()
    led.close()


# ---- 6. streaming encoder ------------------------------------------------------------------------------------------------------------
def test_streaming_encoder_of_13_frame_chunks_on_head_size_32():
    from tensorflowasr_amd.models import StreamingConformerEncoder
    cfg = dict(co.STREAMING_S, dmodel=256, num_heads=8, head_size=32, kernel_size=9, num_blocks=1)
    w = co.encoder_weights(cfg, seed=2)
    e = StreamingConformerEncoder(**encoder_kwargs(cfg))
    e.add_chunk_size(8000, 80, 640)
    e.load_weights(w, by_name=False)
    x = waves(2, 24000, 9)
    got = e(x).cpu().numpy()
    assert got.shape == (2, 39, 256)
    led = Ledger("streaming")
    led.add("256 8x32 k9 chunk 8000", got, co.streaming_conformer_encoder(x.astype(np.float64), w, cfg, 8000),
            co.streaming_conformer_encoder(x, w, cfg, 8000, dtype=np.float32))
    led.close()


# ---- 7. ragged calls on an untuned model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,hs,k,field", [(3, 48, 32, "head_size"), (4, 36, 7, "kernel_size")])
def test_ragged_calls_on_an_untuned_model_are_refused_before_the_frontend(H, hs, k, field):
    """the length-aware kernels of dmodel 144 are those of head size 36 and kernel size 32: ragged_config_ok says so, naming the field,
    before anything is launched (the handle's launch counters stay at zero); the calls without lengths run"""
    from tensorflowasr_amd import _lib
    m, w, cfg = _block_model(144, H, hs, k)
    x = waves(2, 32000, 11)
    lens = np.array([32000, 16000], np.int32)
    lib, nk = _lib.lib(), len(_lib.KERNEL_NAMES)
    ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 1))
    try:
        _lib.check(lib.mi355asr_profile_read(m._h.ptr, ms, cnt, nk, 1))
        with pytest.raises(_lib.Mi355AsrError, match="error -1: ragged batches do not support %s" % field):
            m.recognize(x, wav_lengths=lens)
        with pytest.raises(_lib.Mi355AsrError, match="error -1: ragged batches do not support %s" % field):
            m.encode(x, lengths=lens)
        _lib.check(lib.mi355asr_profile_read(m._h.ptr, ms, cnt, nk, 1))
        launched = {n: int(cnt[i]) for i, n in enumerate(_lib.KERNEL_NAMES) if cnt[i]}
        assert not launched, "a refused ragged call launched %s" % launched
        m.recognize(x)
        _lib.check(lib.mi355asr_profile_read(m._h.ptr, ms, cnt, nk, 1))
        assert cnt[_lib.KERNEL_NAMES.index("stft")] > 0      # ... and the counters do count the frontend
    finally:
        _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 0))


def test_ragged_recognize_with_an_untuned_ctc_decoder_is_refused_before_the_frontend():
    """encoder blocks of head size 36 and kernel size 32, the CTC decoder's block on kernel size 7: recognize(wav_lengths=...) names
    ctcdecoder_kernel_size before anything is launched; the ragged encoder call, which never reaches that block, runs"""
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.models import ConformerCTC
    cfg = dict(co.CONFORMER_S, num_blocks=1, ctcdecoder_kernel_size=7)
    w = co.encoder_weights(cfg, seed=7)
    w.update(co.ctc_decoder_weights(cfg, 40, seed=8))
    m = ConformerCTC(40, num_blocks=1, ctcdecoder_kernel_size=7)
    m.load_weights(w, by_name=False)
    x = waves(2, 32000, 11)
    lens = np.array([32000, 16000], np.int32)
    lib, nk = _lib.lib(), len(_lib.KERNEL_NAMES)
    ms, cnt = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 1))
    try:
        _lib.check(lib.mi355asr_profile_read(m._h.ptr, ms, cnt, nk, 1))
        with pytest.raises(_lib.Mi355AsrError, match="error -1: ragged batches do not support ctcdecoder_kernel_size"):
            m.recognize(x, wav_lengths=lens)
        _lib.check(lib.mi355asr_profile_read(m._h.ptr, ms, cnt, nk, 1))
        assert not any(cnt), "a refused ragged call launched something"
    finally:
        _lib.check(lib.mi355asr_profile_enable(m._h.ptr, 0))
    enc, el = m.encode(x, lengths=lens)
    assert el.cpu().numpy().tolist() == [50, 25] and not enc.cpu().numpy()[1, 25:].any()
