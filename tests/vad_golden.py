"""Inputs of the VAD fixtures (tests/golden/vad_ref.npz), rebuilt from files under tests/golden/ so the npz does not
carry them: the two speech recordings and the ~60 s recording composed from them, digital silence and low-level noise."""
import hashlib
import os
import wave

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def read_wav_i16(path):
    with wave.open(path) as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").copy()


def speech():
    return (read_wav_i16(os.path.join(GOLDEN, "speech_bac.wav")), read_wav_i16(os.path.join(GOLDEN, "speech_cpp.wav")))


def _noise(n, seed):
    """int16 noise in [-33, 33] from a multiplicative hash of the sample index (no RNG stream to depend on)"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(1 << 24)
    u = (i * np.uint64(2654435761) + np.uint64(0x9E3779B9)) % np.uint64(1 << 32)
    return ((u >> np.uint64(8)) % np.uint64(67)).astype(np.int16) - 33


def composed_i16():
    """~60 s at 16 kHz: gaps under 0.1 s, gaps of several seconds, one speech-only span over 15 s, ends mid-speech"""
    bac, cpp = speech()
    sec = lambda s: int(s * 16000)
    zero = lambda s: np.zeros(sec(s), np.int16)
    parts = [_noise(sec(0.5), 1), bac, zero(0.05), cpp, _noise(sec(3.0), 2),
             bac, cpp, bac, cpp,                                   # one speech span over 15 s, no gaps
             zero(5.0), cpp, zero(0.08), bac, _noise(sec(2.0), 3), bac, _noise(sec(0.03), 4), cpp, _noise(sec(4.0), 5),
             bac[: int(len(bac) * 0.6)]]                           # ends mid-speech
    return np.concatenate(parts)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs_i16(ref):
    """name -> int16 samples (x = in / 32768) for every fixture input; test8k is the one stored in the npz"""
    bac, cpp = speech()
    comp = composed_i16()
    assert sha256(comp) == str(ref["meta_composed_sha256"]), "composed recording differs from the one the fixture scored"
    return {"test8k": ref["in_test8k"], "bac": bac, "cpp": cpp, "composed": comp}
