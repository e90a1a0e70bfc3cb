"""The LEAF frontend and the add_wav_info branch at their length, padding and tile edges, against the float64 oracle.

LEAF (csrc/leaf.hip): lengths below the 401-tap window and its half, one sample either side of a 128- and a 512-position tile,
every residue class of the pooling's left pad, the lengths tests/leaf_edges.py adds so that every frame slot of a tile and of a
wave is exercised in the first, an interior and the partial last tile, and the frame counts around the PCEN kernel's 20 thread
rows and 128-frame chunks.  The device must stay within max(the contract bound of test_gpu_parity.test_leaf_frontend_parity for
that MI355ASR_LEAF_TERMS, 4 x E32), E32 being the distance of the oracle run in float32 from the oracle run in float64: at F <= 3
the instance norm divides by a near-zero deviation, which a correct float32 implementation amplifies alike.  Exact statements
(F = 1 gives beta, rows are independent, the streaming reshape, poisoned surroundings, repeatability) have no tolerance.

Waveform branch (csrc/wavpick.hip, run_wavpick): the branch alone as the difference of two block-less encoders against
co.wave_pick_model, through the parity flips of the four nested SAME pads, at the length floor (three frames: below it the call
is refused) and with 16-row GEMM tiles that span several utterances.

Measured on an MI355X (max |device - float64 oracle|; E32 = max |float32 oracle - float64 oracle|):
    case                      L      F   terms 3   terms 2   terms 0   E32
    leaf                      1      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                      2      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    159      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    160      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    161      2   2.1e-05   9.8e-05   2.1e-05   1.0e-06
    leaf                    200      2   1.5e-05   4.2e-04   1.5e-05   6.2e-06
    leaf                    201      2   2.1e-05   3.0e-04   2.1e-05   8.1e-06
    leaf                    400      3   7.1e-06   4.9e-05   3.9e-06   2.1e-06
    leaf                    401      3   3.4e-06   2.8e-04   6.7e-06   5.9e-06
    leaf                    402      3   1.9e-05   8.7e-04   1.9e-05   9.5e-06
    leaf                    127      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    128      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    129      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf                    511      4   4.5e-06   2.3e-04   4.5e-06   4.5e-06
    leaf                    512      4   4.7e-06   1.9e-04   3.7e-06   1.6e-06
    leaf                    513      4   6.6e-06   4.0e-04   6.4e-06   4.4e-06
    leaf                   1023      7   6.8e-06   2.8e-04   4.9e-06   4.2e-06
    leaf                   1024      7   5.0e-06   3.2e-04   5.5e-06   3.7e-06
    leaf                   1025      7   4.4e-06   1.5e-04   5.7e-06   3.3e-06
    leaf                   2560     16   6.5e-06   4.0e-04   6.7e-06   4.5e-06
    leaf                   2561     17   5.0e-06   4.2e-04   4.4e-06   6.3e-06
    leaf                   2639     17   5.2e-06   3.5e-04   5.4e-06   7.4e-06
    leaf                   2640     17   7.6e-06   2.1e-04   8.2e-06   5.8e-06
    leaf                   2641     17   6.6e-06   3.1e-04   6.0e-06   5.5e-06
    leaf                   2719     17   8.6e-06   2.9e-04   7.6e-06   4.3e-06
    leaf                    740      5   6.5e-06   1.6e-04   6.5e-06   4.6e-06
    leaf                   2738     18   5.5e-06   1.7e-04   4.8e-06   5.3e-06
    leaf                   3040     19   7.6e-06   1.7e-04   6.4e-06   4.6e-06
    leaf                   3200     20   8.3e-06   1.8e-04   8.3e-06   5.4e-06
    leaf                   3360     21   5.8e-06   1.8e-04   5.7e-06   3.6e-06
    leaf                  20320    127   5.0e-06   2.8e-04   5.8e-06   5.8e-06
    leaf                  20480    128   6.3e-06   1.5e-04   5.7e-06   4.9e-06
    leaf                  20481    129   6.6e-06   3.2e-04   6.6e-06   7.1e-06
    leaf                  40960    256   6.3e-06      -         -      5.9e-06
    leaf                  40961    257   4.1e-06      -         -      4.2e-06
    leaf row 0 of 3         513      4   6.6e-06   4.0e-04   6.4e-06   4.4e-06
    leaf row 0 of 3        1025      7   4.4e-06   1.5e-04   5.7e-06   3.3e-06
    leaf fenced               1      1   0.0e+00   0.0e+00   0.0e+00   0.0e+00
    leaf fenced             513      4   6.6e-06   4.0e-04   6.4e-06   4.4e-06
    leaf fenced            2561     17   5.0e-06   4.2e-04   4.4e-06   6.3e-06
    leaf silent            2561     17   2.2e-04   2.2e-04   2.2e-04   6.5e-05
    leaf beside silent     2561     17   4.5e-06   8.9e-05   4.5e-06   2.7e-06
    (bounds: 2e-4 / 1e-3 / 1e-3, or 4 x E32 where that is larger -- the silent utterance only: 2.6e-4)
    waveform branch S    13 lengths: max |branch - oracle| 2.3e-07 .. 4.4e-07 (bound 1e-3)
    waveform branch 20ms 13 lengths: max |branch - oracle| 2.5e-07 .. 3.3e-07 (bound 1e-3)
    waveform branch M     4 lengths: max |branch - oracle| 2.0e-07 .. 3.3e-07 (bound 1e-3)
    waveform branch, one row of each batch shape: 2.7e-07 .. 4.1e-07; LEAF + branch at L = 1441: encoder 2.1e-06
"""
import numpy as np
import pytest

import leaf_edges as le
from helpers import co, encoder_kwargs, maxdiff, small_cfg, waves
from test_gpu_parity import _leaf_weights

pytestmark = pytest.mark.gpu
TOL = 1e-3                                    # the project's contract against the float64 oracle
LEAF_BOUND = {"3": 2e-4, "2": TOL, "0": TOL}  # what test_leaf_frontend_parity asserts per MI355ASR_LEAF_TERMS
SEED, WAVE0 = 7, 60                           # _leaf_weights seed, first synth_wave index

_ENC, _REF, _WAV = {}, {}, {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _leaf(terms, monkeypatch):
    """(encoder, weights) with the Gabor conv of `terms`, built once: the library reads MI355ASR_LEAF_TERMS when a handle is made"""
    if terms not in _ENC:
        from tensorflowasr_amd.models import ConformerEncoder
        monkeypatch.setenv("MI355ASR_LEAF_TERMS", terms)
        cfg = small_cfg(1)
        w = _leaf_weights(cfg, SEED, True)
        e = ConformerEncoder(**dict(encoder_kwargs(cfg), mel_layer_type="leaf"))
        e.load_weights(w, by_name=False)
        _ENC[terms] = (e, w)
    return _ENC[terms]


def _wave(L, start=WAVE0, silent=False):
    return np.zeros((1, L), np.float32) if silent else waves(1, L, start)


def _ref(L, start=WAVE0, silent=False):
    """(float64 oracle [F, 80], E32) of one utterance, computed once per module"""
    key = (L, start, silent)
    if key not in _REF:
        w = _leaf_weights(small_cfg(1), SEED, True)
        x = _wave(L, start, silent).astype(np.float64)
        r64 = co.leaf_frontend(x, w)
        r32 = co.leaf_frontend(x, w, dtype=np.float32)
        _REF[key] = (r64[0], float(np.abs(r64 - r32).max()))
    return _REF[key]


def _held(tag, terms, got, L, start=WAVE0, silent=False):
    ref, e32 = _ref(L, start, silent)
    assert got.shape == ref.shape == (-(-L // 160), 80)
    err = maxdiff(got, ref)
    contract = LEAF_BOUND[terms]
    print("%s terms=%s L=%d F=%d: max |gpu - oracle| = %.3g  E32 = %.3g" % (tag, terms, L, ref.shape[0], err, e32))
    assert 4 * e32 <= 100 * contract, "the reference alone is ill conditioned here: choose another waveform seed"
    assert np.isfinite(got).all()
    assert err <= max(contract, 4 * e32), (tag, terms, L, err, e32)
    return err


# ---- LEAF ------------------------------------------------------------------------------------------------------------------------
def _leaf_cases():
    out = [(t, L) for t in ("3", "2", "0") for L in le.gpu_lengths()]
    return out + [("3", L) for L in le.FRAME_COUNTS_DEFAULT_TERMS]


@pytest.mark.parametrize("terms,L", _leaf_cases())
def test_leaf_lengths_against_the_oracle(monkeypatch, terms, L):
    e, w = _leaf(terms, monkeypatch)
    got = e.melspectrogram(_wave(L)).cpu().numpy()
    assert got.shape[0] == 1
    _held("leaf", terms, got[0], L)
    if L <= 160:          # F = 1: the mean of one value is that value, the deviation 0 -- the output is beta, bit for bit
        assert got.shape[1] == 1
        assert np.array_equal(_bits(got[0, 0]), _bits(w["mel_layer/tfbanks_instancenorm/beta"]))


@pytest.mark.parametrize("terms", ["3", "2", "0"])
@pytest.mark.parametrize("L", [513, 1025])
def test_leaf_rows_are_independent(monkeypatch, terms, L):
    e, _ = _leaf(terms, monkeypatch)
    x = waves(3, L, WAVE0)
    got = e.melspectrogram(x).cpu().numpy()
    for b in range(3):
        solo = e.melspectrogram(x[b:b + 1]).cpu().numpy()
        assert np.array_equal(_bits(got[b]), _bits(solo[0])), (terms, L, b)
    _held("leaf row 0 of 3", terms, got[0], L)


def test_leaf_streaming_reshape_is_the_plain_encoder_on_the_chunks():
    """StreamingConformerEncoder (chunk 8000) on 2 x 16000 samples == the plain encoder on the same four 8000-sample rows"""
    from tensorflowasr_amd.models import ConformerEncoder, StreamingConformerEncoder
    cfg = small_cfg(1, co.STREAMING_S)
    w = _leaf_weights(cfg, 8)
    st = StreamingConformerEncoder(**dict(encoder_kwargs(cfg), mel_layer_type="leaf"))
    st.add_chunk_size(8000, 80, 640)
    st.load_weights(w, by_name=False)
    e = ConformerEncoder(**dict(encoder_kwargs(cfg), mel_layer_type="leaf"))
    e.load_weights(w, by_name=False)
    x = waves(2, 16000, 70)
    a = st.melspectrogram(x).cpu().numpy()
    b = e.melspectrogram(x.reshape(4, 8000)).cpu().numpy()
    assert a.shape == b.shape == (4, 50, 80)
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("terms", ["3", "2", "0"])
@pytest.mark.parametrize("L", [1, 513, 2561])
def test_leaf_fenced_and_poisoned(monkeypatch, terms, L):
    """the waveform inside a buffer of NaN words, the workspace and the output fenced and filled with NaN words: a read outside
    [0, L), or of scratch the kernels did not write, would bring a NaN into the pooling.  Twice unfenced: the same bits."""
    import torch
    from fence import fenced
    e, _ = _leaf(terms, monkeypatch)
    x = _wave(L)
    plain = e.melspectrogram(x).cpu().numpy()
    again = e.melspectrogram(x).cpu().numpy()
    assert np.array_equal(_bits(plain), _bits(again))
    pad = 1024                                             # floats of NaN either side: more than the 200 + 416 the staging spans
    e._h._ws = None                                        # the workspace is allocated again, inside the fence
    try:
        with fenced(0xFF) as f:
            buf = f.allocate(torch.empty, (L + 2 * pad,), torch.float32, e._h.device, "the test's waveform")
            assert bool(torch.isnan(buf).all())
            wav = buf[pad:pad + L].view(1, L)
            wav.copy_(torch.from_numpy(x))
            out = e.melspectrogram(wav)
            torch.cuda.synchronize()
            f.check()
            assert len(f.allocations) >= 3                 # waveform, output, workspace
            got = out.cpu().numpy()
            assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + L:]).all())
    finally:
        e._h._ws = None
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(plain)), (terms, L)
    _held("leaf fenced", terms, got[0], L)


@pytest.mark.parametrize("terms", ["3", "2", "0"])
def test_leaf_silent_utterance(monkeypatch, terms):
    """all zeros: every pooled value sits on the 1e-5 floor, PCEN is constant over time and the deviation 0"""
    e, _ = _leaf(terms, monkeypatch)
    L = 2561
    other = _wave(L, WAVE0 + 1)
    x = np.concatenate([_wave(L, silent=True), other])
    got = e.melspectrogram(x).cpu().numpy()
    _held("leaf silent", terms, got[0], L, silent=True)
    _held("leaf beside silent", terms, got[1], L, start=WAVE0 + 1)
    solo = e.melspectrogram(other).cpu().numpy()
    assert np.array_equal(_bits(got[1]), _bits(solo[0]))


# ---- add_wav_info ----------------------------------------------------------------------------------------------------------------
BASES = {"S": None, "20ms": dict(co.CONFORMER_S, stride_ms=20), "M": co.CONFORMER_M}


def _branch_models(base):
    """(with branch, without, weights, dmodel, hop_size * reduction_factor) of a block-less encoder, built once"""
    if base not in _WAV:
        from tensorflowasr_amd.models import ConformerEncoder
        cfg = small_cfg(0, BASES[base])
        hopred = cfg["stride_ms"] * 16 * cfg["reduction_factor"]              # 640 -> strides [8,5,4,4]; 1280 -> [16,5,4,4]
        w = {k: v for k, v in co.encoder_weights(cfg, seed=21).items() if not k.startswith("conformer_block_")}
        w.update(co.wave_pick_weights(cfg["dmodel"], hopred, seed=22))
        ea = ConformerEncoder(**dict(encoder_kwargs(cfg), mel_layer_type="Melspectrogram", add_wav_info=True))
        ea.load_weights(w, by_name=False)
        eb = ConformerEncoder(**dict(encoder_kwargs(cfg), mel_layer_type="Melspectrogram"))
        eb.load_weights({k: v for k, v in w.items() if not k.startswith("wav_layer/")}, by_name=False)
        _WAV[base] = (ea, eb, w, cfg["dmodel"], hopred)
    return _WAV[base]


def _branch_held(tag, base, x, with_branch, without):
    _, _, w, d, hopred = _branch_models(base)
    ref = co.wave_pick_model(x.astype(np.float64), w, d, hopred)
    branch = with_branch.astype(np.float64) - without
    assert branch.shape == ref.shape == (x.shape[0], -(-x.shape[1] // hopred), d)
    assert np.abs(ref).max() > 0.05                       # the branch is not negligible in the sum
    err = maxdiff(branch, ref)
    print("%s %s B=%d L=%d T=%d: max |branch - oracle| = %.3g" % (tag, base, x.shape[0], x.shape[1], ref.shape[1], err))
    assert err < TOL, (tag, base, x.shape, err)


def _wav_cases():
    out = []
    for base in ("S", "20ms", "M"):
        hopred = 1280 if base == "20ms" else 640
        Ls = sorted([2 * hopred + 1] + le.wav_lengths(hopred))        # the floor, then 3 frames' worth + the residues
        if base == "M":
            Ls = Ls[:2] + Ls[-2:]
        out += [(base, L) for L in Ls]
    return out


@pytest.mark.parametrize("base,L", _wav_cases())
def test_wav_branch_length_residues(base, L):
    ea, eb, _, _, hopred = _branch_models(base)
    assert L >= le.wav_min_length(co.wave_pick_scales(hopred))
    x = waves(1, L, 90)
    _branch_held("wav", base, x, ea(x).cpu().numpy(), eb(x).cpu().numpy())


@pytest.mark.parametrize("base", ["S", "20ms", "M"])
def test_wav_branch_refuses_less_than_three_frames(base):
    """one sample below the floor: Mi355AsrError naming add_wav_info and the minimum length, nothing launched -- a sentinel-filled
    output keeps every word; the same encoder without the branch takes the length"""
    import torch
    from tensorflowasr_amd import _lib
    from tensorflowasr_amd.models import _p
    ea, eb, _, d, hopred = _branch_models(base)
    floor = le.wav_min_length(co.wave_pick_scales(hopred))
    assert floor == 2 * hopred + 1
    for L in (floor - 1, hopred, 1):
        x = waves(2, L, 91)
        with pytest.raises(_lib.Mi355AsrError, match=r"add_wav_info.*%d samples" % floor):
            ea(x)
        assert tuple(eb(x).shape) == (2, -(-L // hopred), d)
    h = ea._h
    L = floor - 1
    xd = h.to_device(waves(2, L, 91))
    out = torch.full((2, 2, d), -7.25, dtype=torch.float32, device=h.device)
    ws, n = h.ws_for_wave(2, L)
    with torch.cuda.device(h.device):
        rc = h.lib.mi355asr_encoder_forward(h.ptr, _p(xd), 2, L, _p(out), _p(ws), n, h._stream())
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_lib.Mi355AsrError, match="add_wav_info"):
        _lib.check(rc)
    assert bool((out == -7.25).all())
    x = waves(2, floor, 91)                                # ... and the floor itself runs
    assert tuple(ea(x).shape) == (2, 3, d)


@pytest.mark.parametrize("B,T", le.WAV_BATCH_EDGES)
def test_wav_branch_batch_edges(B, T):
    """B * T rows that are no multiple of 16, 16-row GEMM tiles that span up to six utterances: every row of the batch equals
    its B = 1 run bit for bit, one row is held to the oracle"""
    ea, eb, _, _, hopred = _branch_models("S")
    L = hopred * (T - 1) + 1 if T == 3 else hopred * T - 7
    x = waves(B, L, 92)
    got = ea(x).cpu().numpy()
    assert got.shape[:2] == (B, T) and (B * T) % 16 != 0
    for b in range(B):
        solo = ea(x[b:b + 1]).cpu().numpy()
        assert np.array_equal(_bits(got[b]), _bits(solo[0])), (B, T, b)
    b = B // 2
    _branch_held("wav batch row %d" % b, "S", x[b:b + 1], got[b:b + 1], eb(x[b:b + 1]).cpu().numpy())


def test_wav_branch_with_leaf_near_the_floor():
    """test_add_wav_info_with_leaf_ctc_and_errors's model at L = 1281 + 160: the LEAF and the waveform frame counts agree"""
    from tensorflowasr_amd.models import ConformerCTC
    cfg = small_cfg(1)
    V = 40
    w = _leaf_weights(cfg, 31)
    w.update(co.wave_pick_weights(cfg["dmodel"], 640, seed=32))
    w.update(co.ctc_decoder_weights(cfg, V, seed=33))
    kw = dict(encoder_kwargs(cfg))
    kw.pop("mel_layer_type")
    m = ConformerCTC(V, ctcdecoder_num_blocks=cfg["ctcdecoder_num_blocks"], mel_layer_type="leaf", add_wav_info=True, **kw)
    m.load_weights(w, by_name=False)
    L = 1281 + 160
    x = waves(1, L, 96)
    ref = co.conformer_encoder(x.astype(np.float64), w, dict(cfg, mel_layer_type="leaf", add_wav_info=True))
    enc = m.encode(x).cpu().numpy()
    assert enc.shape == ref.shape == (1, -(-L // 640), cfg["dmodel"]) and ref.shape[1] == 3
    assert co.leaf_frontend(x.astype(np.float64), w).shape[1] == -(-L // 160)
    assert co.wave_pick_model(x.astype(np.float64), w, cfg["dmodel"], 640).shape[1] == 3
    err = maxdiff(enc, ref)
    print("leaf + wav L=%d: max |enc - oracle| = %.3g" % (L, err))
    assert err < TOL
