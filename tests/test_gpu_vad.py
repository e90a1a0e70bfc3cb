"""VAD on the MI355X: vad.hip against the reference graph's own scores (tests/golden/vad_ref.npz), tile shapes,
batch independence, segmentation, ASRSession and the C ABI."""
import ctypes
import os

import numpy as np
import pytest

from test_vad_host import GOLDEN, as_list, frames_of, graph_weights, load_ref, net64

pytestmark = pytest.mark.gpu
TILE = 56          # output frames per workgroup in vad.hip (64 LDS rows minus the 8-frame halo)


@pytest.fixture(scope="module")
def ref():
    return load_ref()


@pytest.fixture(scope="module")
def vad():
    import torch
    assert torch.cuda.is_available(), "needs cuda:0 (MI355X)"
    from tensorflowasr_amd.vad import VAD
    return VAD().load_onnx(os.path.join(GOLDEN, "vad.onnx"))


def close(got, want, what):
    err = np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float(err.max()) <= 1e-4, "%s: max scaled error %.3g" % (what, float(err.max()))
    return float(err.max())


@pytest.mark.parametrize("name", ["test8k", "bac", "cpp", "composed"])
def test_device_scores_match_the_reference_graph(ref, vad, name):
    x = ref["in_" + name].astype(np.float32) / 32768
    if name == "test8k":
        got = vad.inference(frames_of(ref, name)[None]).reshape(-1)
    else:
        got = vad.scores(x).cpu().numpy().reshape(-1)
    want = ref["s32_" + name].astype(np.float64)
    err = float(np.abs(got - want).max())
    e = close(got, want, name)
    sure = np.abs(want) >= 1e-3
    assert np.array_equal(got[sure] >= 0, want[sure] >= 0), name
    print("%s: T=%d max|d|=%.3g scaled=%.3g" % (name, len(want), err, e))


@pytest.mark.parametrize("T", [1, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_tile_boundaries(ref, vad, T):
    w = graph_weights()
    x = (np.random.default_rng(T).standard_normal(T * 160) * 0.1).astype(np.float32)
    got = vad.scores(x).cpu().numpy().reshape(-1)
    close(got, net64(x[::2].reshape(T, 80), w), "T=%d" % T)


def test_one_hour_batch(ref, vad):
    w = graph_weights()
    rng = np.random.default_rng(60)
    x = (rng.standard_normal((60, 60 * 16000)) * rng.uniform(0.01, 0.3, (60, 1))).astype(np.float32)
    got = vad.scores(x).cpu().numpy()
    assert got.shape == (60, 6000)
    for b in (0, 17, 59):
        close(got[b], net64(x[b, ::2].reshape(6000, 80), w), "row %d" % b)


def test_rows_are_independent(vad):
    rng = np.random.default_rng(3)
    lens = [16000 * 3 + 37, 16000, 5 * 160 + 159]
    L = max(lens) + 1000
    x = (rng.standard_normal((3, L)) * 0.1).astype(np.float32)
    padded = x.copy()
    for b, n in enumerate(lens):
        padded[b, n:] = rng.uniform(-1e30, 1e30, L - n)          # garbage past each length: never read
    got = vad.scores(padded, lengths=lens).cpu().numpy()
    for b, n in enumerate(lens):
        one = vad.scores(x[b, :n]).cpu().numpy().reshape(-1)
        assert np.array_equal(got[b, :len(one)], one), b
        assert np.all(got[b, len(one):] == 0)
    # inference on undecimated 8 kHz frames == scores on the same samples taken every second one
    fr = x[0, : 300 * 160: 2].reshape(1, 300, 80)
    assert np.array_equal(vad.inference(fr).reshape(-1), vad.scores(x[0, :300 * 160]).cpu().numpy().reshape(-1))


def test_offline_segments_on_device_scores(ref, vad):
    from tensorflowasr_amd.vad import OfflineVAD
    ov = OfflineVAD(sr=16000)
    ov.compile(vad)
    x = ref["in_composed"].astype(np.float32) / 32768
    assert ov.vad(x[: len(x) // 160 * 160]) == as_list(ref["seg_composed"])


def _asr(tmp_path):
    from tensorflowasr_amd.asr import ASR
    from tensorflowasr_amd.config import load_yaml
    (tmp_path / "phones.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + ["p%d" % i for i in range(56)]) + "\n")
    (tmp_path / "chars.txt").write_text("\n".join(["<S>", "</S>", "[SPACE]", "[UNK]"] + [chr(0x4e00 + i) for i in range(96)]) + "\n")
    here = os.path.join(os.path.dirname(GOLDEN), "..", "tensorflowasr_amd", "configs")
    cfg = load_yaml(os.path.join(here, "am_data.yml"))
    cfg.update(load_yaml(os.path.join(here, "conformerS.yml")))
    cfg["model_config"]["num_blocks"] = 2
    cfg["inp_config"]["vocabulary"] = str(tmp_path / "phones.txt")
    cfg["tar_config"]["vocabulary"] = str(tmp_path / "chars.txt")
    cfg["running_config"]["outdir"] = str(tmp_path / "logs")
    return ASR(cfg, load_checkpoint=False)


def test_asr_session_send(ref, vad, tmp_path):
    from tensorflowasr_amd.session import ASRSession
    asr = _asr(tmp_path)
    s = ASRSession(asr, vad)
    x = ref["in_composed"].astype(np.float32) / 32768
    x = x[: len(x) // 160 * 160]
    out = s.send(x)
    segs = as_list(ref["seg_composed"])
    assert len(out) == len(segs) >= 1
    for i, (r, (a, b)) in enumerate(zip(out, segs)):
        assert set(r) == {"session", "sentence_index", "sentence_begin_time", "best_text", "sentence_end_time"}
        assert r["sentence_index"] == i and r["session"] == "asr_1"
        assert (r["sentence_begin_time"], r["sentence_end_time"]) == (int(a * 1000), int(b * 1000))
        phones, text = asr.offline_stt_wave(x[int(a * 16000):int(b * 16000)])
        assert r["best_text"] == text and s.phones[i] == phones


def test_c_abi_forward_with_null_lengths(ref, vad):
    import torch
    from tensorflowasr_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(lib.mi355asr_vad_create(ctypes.byref(_lib.VadConfig(80, 80, 2)), ctypes.byref(h)))
    try:
        for name, a in graph_weights().items():
            a = np.ascontiguousarray(a, np.float32)
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.mi355asr_load_weight(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.ndim, dims))
        _lib.check(lib.mi355asr_finalize_weights(h, None))
        x = ref["in_bac"].astype(np.float32)[None] / 32768
        L = x.shape[1]
        T = ctypes.c_int32()
        _lib.check(lib.mi355asr_vad_frames(h, L, ctypes.byref(T)))
        assert T.value == L // 160
        n = ctypes.c_size_t(1)
        _lib.check(lib.mi355asr_vad_workspace_bytes(h, 1, L, ctypes.byref(n)))
        assert n.value == 0
        xd = torch.from_numpy(x).cuda()
        out = torch.full((1, T.value), float("nan"), device="cuda")
        _lib.check(lib.mi355asr_vad_forward(h, ctypes.c_void_p(xd.data_ptr()), 1, L, None,
                                            ctypes.c_void_p(out.data_ptr()), None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), vad.scores(x).cpu().numpy())
    finally:
        lib.mi355asr_destroy(h)
