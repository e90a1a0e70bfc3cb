"""Recursive (IIR) filters on the device: scipy.signal.sosfilt and scipy.signal.sosfiltfilt for every row of a ragged batch, in
float64 on second-order sections (csrc/iir.hip).  There is no CPU path.

    f = SOSFilter()
    sos = scipy.signal.butter(3, [0.2, 0.5], "bandstop", output="sos")
    y = f.sosfiltfilt(x, lengths, sos)                            # [B, L] float32 on the device, zeros past lengths[b]
    y, zf = f.sosfilt(packet, None, sos, zi=zf)                   # a stream, packet by packet

A row is computed as if it were alone and is the same bits in every run, in every batch and at every batch position: it is cut
into chunks of `SOSFilter.CHUNK` samples at fixed positions."""
import ctypes

import numpy as np


class _Chunk:
    """SOSFilter.CHUNK: the library's chunk length, asked for on first use"""

    def __get__(self, obj, owner):
        from . import _lib
        return int(_lib.lib().mi355asr_sos_chunk())


def default_padlen(sos):
    """scipy.signal.sosfiltfilt's default edge: 3 (2 S + 1 - min(#(sos[:, 2] == 0), #(sos[:, 5] == 0)))"""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    return 3 * (2 * len(sos) + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


class SOSFilter:
    MAX_SECTIONS = 8
    MAX_PADLEN = 1024
    CHUNK = _Chunk()

    def __init__(self, device="cuda:0"):
        self.device = device

    def _sos(self, sos, B):
        import torch
        s = sos.detach().cpu().numpy() if torch.is_tensor(sos) else sos
        s = np.ascontiguousarray(np.asarray(s, np.float64))
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or s.shape[2] != 6 or s.shape[0] not in (1, B):
            raise ValueError("sos must be [S, 6] or [B, S, 6] with B = %d, got %s" % (B, tuple(s.shape)))
        if not 1 <= s.shape[1] <= self.MAX_SECTIONS:
            raise ValueError("%d sections are outside 1 .. %d" % (s.shape[1], self.MAX_SECTIONS))
        return s

    def _run(self, x, lengths, sos, mode, padlen, zi, want_zf, noise, noise_scale, quantise, short_rows="raise"):
        """short_rows="copy": a row of at most padlen samples is copied through by the library instead of raising (Hz)"""
        import torch
        from . import _lib
        from .augment import _lengths, _ptr, _rows, _stream
        lib = _lib.lib()
        x, L = _rows(x, self.device)
        B, W = int(x.shape[0]), int(x.shape[1])
        ln = _lengths(lengths, B, L, self.device)
        s = self._sos(sos, B)
        S, shared = int(s.shape[1]), s.shape[0] == 1
        if mode == 1:
            padlen = max(default_padlen(s[b]) for b in range(s.shape[0])) if padlen is None else int(padlen)
            if not 0 <= padlen <= self.MAX_PADLEN:
                raise ValueError("padlen = %d is outside 0 .. %d" % (padlen, self.MAX_PADLEN))
            lens = ln.cpu().numpy()
            short = np.flatnonzero(lens <= padlen) if short_rows == "raise" else ()
            if len(short):
                raise ValueError("row %d: The length of the input vector x must be greater than padlen, which is %d (the row has %d "
                                 "samples)." % (int(short[0]), padlen, int(lens[short[0]])))
        else:
            padlen = 0
        sd = torch.from_numpy(s).to(self.device)
        zid = zfd = nd = None
        if zi is not None:
            z = zi.detach().to(torch.float64) if torch.is_tensor(zi) else torch.from_numpy(np.ascontiguousarray(np.asarray(zi, np.float64)))
            zid = z.reshape(-1, S, 2).to(self.device).contiguous()
            if zid.shape[0] != B:
                raise ValueError("zi must be [B, S, 2] = [%d, %d, 2], got %s" % (B, S, tuple(z.shape)))
        if want_zf:
            zfd = torch.empty((B, S, 2), dtype=torch.float64, device=self.device)
        if noise is not None:
            nd = noise.to(torch.float64) if torch.is_tensor(noise) else torch.from_numpy(np.ascontiguousarray(np.asarray(noise, np.float64)))
            nd = nd.reshape(B, -1).to(self.device).contiguous()
            if nd.shape[1] < W:
                raise ValueError("noise %s does not cover the batch %s" % (tuple(nd.shape), (B, W)))
        wb = ctypes.c_size_t()
        _lib.check(lib.mi355asr_sos_workspace_bytes(B, W, S, mode, ctypes.byref(wb)))
        ws = torch.empty((wb.value + 7) // 8, dtype=torch.float64, device=self.device)
        y = torch.empty((B, W), dtype=torch.float32, device=self.device)
        null = ctypes.c_void_p(None)
        with torch.cuda.device(self.device):
            _lib.check(lib.mi355asr_sos_ragged(_ptr(x), 4 if x.dtype == torch.int16 else 0, _ptr(ln), B, W, _ptr(sd), S, int(shared), mode,
                                               padlen, _ptr(zid) if zid is not None else null, _ptr(zfd) if zfd is not None else null,
                                               _ptr(nd) if nd is not None else null, int(nd.shape[1]) if nd is not None else 0,
                                               float(noise_scale), int(bool(quantise)), _ptr(y), W, _ptr(ws), wb.value,
                                               _stream(self.device)))
        self._keep = (x, ln, sd, zid, nd, ws)             # inputs of an asynchronous call
        return (y if L else y[:, :0]), zfd

    def sosfilt(self, x, lengths, sos, zi=None):
        """scipy.signal.sosfilt(sos, x, zi=zi) per row.  x [L] or [B, L] float32 or int16 (x / 32768); lengths [B] or None; sos
        [S, 6] (shared) or [B, S, 6]; zi [B, S, 2] float64 or None: the zero state -> (y [B, L] float32 on the device, zeros
        past lengths[b]; zf [B, S, 2] float64 on the device: the state after lengths[b] samples)."""
        return self._run(x, lengths, sos, 0, 0, zi, True, None, 1.0, False)

    def sosfiltfilt(self, x, lengths, sos, padlen=None, noise=None, noise_scale=1.0, quantise=False):
        """scipy.signal.sosfiltfilt(sos, x, padtype="odd", padlen=padlen) per row -> y [B, L] float32 on the device.  padlen
        None: SciPy's default for the sections.  A row with lengths[b] <= padlen raises SciPy's ValueError, naming the row.
        noise [B, >= L] float64: y + noise_scale * noise in float64; quantise: trunc(clip(y, -1, 1) * 32768) / 32768 on the
        float64 value; one rounding to float32."""
        return self._run(x, lengths, sos, 1, padlen, None, False, noise, noise_scale, quantise)[0]
