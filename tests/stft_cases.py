"""Shared by the GPU tests of the STFT pair, spec_aug and the time stretch: the ragged batches, their float64 references
(computed once) and what the device returned for them."""
import functools

import numpy as np

import stft_ref as sr

OLA_TILE = 256                                          # outputs per workgroup of the overlap-add kernel
GEO = {1024: (1024, 800, 160), 2048: (2048, 2048, 512)}
# the lengths of the issue, and rows whose output ends one sample before, at and after an overlap-add tile (1280 = 5 tiles = 8
# hops; 2560 = 10 tiles = 5 hops); the -1 / +1 outputs themselves come from out_lengths in the inverse tests
LENS = {1024: [0, 512, 513, 640, 800, 1023, 1024, 1025, 1599, 1600, 1601, 4000, 1279, 1280, 1281],
        2048: [0, 1024, 1025, 2047, 2048, 2049, 5000, 2559, 2560, 2561]}
U24 = 2.0 ** -24


def device():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def signal(rng, shape):
    return (0.3 * rng.standard_normal(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair_case(n_fft):
    """one ragged batch through forward and inverse: inputs, float64 references and scales, device results (NumPy)"""
    device()
    from tensorflowasr_amd.stft import STFT
    geo = GEO[n_fft]
    lens = LENS[n_fft]
    rng = np.random.default_rng(n_fft)
    x = signal(rng, (len(lens), max(lens)))
    ref = [sr.stft(x[b, :n], *geo) for b, n in enumerate(lens)]
    a = [sr.frame_l1(x[b, :n], *geo) for b, n in enumerate(lens)]
    st = STFT(*geo)
    S, frames = st.forward(x, lens)
    y, out_len = st.inverse(S, frames)
    return {"geo": geo, "lens": lens, "x": x, "ref": ref, "a": a, "S": S.cpu().numpy(), "frames": frames.cpu().numpy(),
            "y": y.cpu().numpy(), "out_len": out_len.cpu().numpy()}


def worst_ratio(err, scale):
    """max err / scale over scale > 0; where the scale is 0 the error has to be 0"""
    err, scale = np.asarray(err, np.float64), np.asarray(scale, np.float64)
    assert not err[scale == 0].any()
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)
