"""Ragged STFT / ISTFT pair on the device with librosa 0.9 semantics (center=True, pad_mode="reflect", a periodic Hann window of
win_length zero-padded to n_fft): what the reference's augmentations reach through librosa.stft / librosa.istft.  The kernels
are csrc/stft.hip; there is no CPU path.

    st = STFT(1024, 800, 160)                       # SignalSpecAug's sizes; STFT(2048) is librosa's default (time_stretch)
    S, frames = st.forward(x, lengths)              # complex64 [B, Fpad, 513] (librosa's layout transposed), int32 [B]
    y, out_len = st.inverse(S, frames)              # row b: 160 (frames[b] - 1) samples
"""
import ctypes

import numpy as np

SIZES = ((1024, 800, 160), (2048, 2048, 512))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def frames_of(n, n_fft, hop):
    """frames of a row of n samples: 1 + n // hop, 0 below n_fft // 2 + 1 samples"""
    return 1 + int(n) // hop if int(n) >= n_fft // 2 + 1 else 0


class STFT:
    """(n_fft, win_length, hop_length) is (1024, 800, 160) or (2048, 2048, 512), librosa's defaults win_length = n_fft and
    hop_length = win_length // 4 included; anything else is a ValueError."""

    def __init__(self, n_fft, win_length=None, hop_length=None, device="cuda:0"):
        self.n_fft = int(n_fft)
        self.win_length = self.n_fft if win_length is None else int(win_length)
        self.hop_length = self.win_length // 4 if hop_length is None else int(hop_length)
        if (self.n_fft, self.win_length, self.hop_length) not in SIZES:
            raise ValueError("(n_fft, win_length, hop_length) = (%d, %d, %d) is not one of %s"
                             % (self.n_fft, self.win_length, self.hop_length, SIZES))
        self.bins = self.n_fft // 2 + 1
        self.device = device

    def _sizes(self):
        return self.n_fft, self.win_length, self.hop_length

    def forward(self, x, lengths=None):
        """x [L] or [B, L] float32 or int16 (x / 32768); lengths [B] or None -> (S complex64 [B, Fpad, bins] on the device with
        Fpad = max(1, frames of L), frames int32 [B] on the device).  Row b has 1 + lengths[b] // hop frames and zeros after
        them.  Reflect padding needs n_fft // 2 + 1 samples: a shorter row, an empty one included, has 0 frames (librosa
        raises there).  Samples past lengths[b] are never read; a row is computed as if alone."""
        import torch
        from . import _lib
        from .augment import _lengths, _rows
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        Fpad = max(1, frames_of(L, self.n_fft, self.hop_length))
        S = torch.empty((B, Fpad, self.bins), dtype=torch.complex64, device=self.device)
        frames = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mi355asr_stft_ragged(_ptr(x), 4 if x.dtype == torch.int16 else 0, _ptr(ln), B, int(x.shape[1]),
                                                       *self._sizes(), _ptr(S), Fpad, _ptr(frames), _stream(self.device)))
        self._keep = (x, ln)                            # inputs of an asynchronous call
        return S, frames

    def inverse(self, S, frames, out_lengths=None, out_pad=None):
        """S complex64 [B, Fpad, bins] (or [Fpad, bins]), frames [B] -> (y float32 [B, O] on the device, out_len int32 [B] on
        the device).  Row b gets hop (frames[b] - 1) samples, or out_lengths[b] (librosa.istft(..., length=): cut, or
        zero-filled beyond what the frames reach); zeros after them.  O is out_pad, or the longest row."""
        import torch
        from . import _lib
        lib = _lib.lib()
        S = torch.as_tensor(S)
        if S.dim() == 2:
            S = S.reshape(1, *S.shape)
        if S.dim() != 3 or S.shape[2] != self.bins or S.shape[1] < 1:
            raise ValueError("expected a spectrum [B, F >= 1, %d], got %s" % (self.bins, tuple(S.shape)))
        S = S.to(device=self.device, dtype=torch.complex64).contiguous()
        B, Fpad = int(S.shape[0]), int(S.shape[1])
        fr = torch.as_tensor(np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)).reshape(-1)
        fr = fr.to(device=self.device, dtype=torch.int32).clamp(0, Fpad).contiguous()
        if fr.numel() != B:
            raise ValueError("%d rows, %d frame counts" % (B, fr.numel()))
        if out_lengths is None:
            out_len = ((fr - 1).clamp(min=0) * self.hop_length).to(torch.int32)
            ol_ptr = None
        else:
            ol = torch.as_tensor(np.asarray(out_lengths.cpu() if torch.is_tensor(out_lengths) else out_lengths)).reshape(-1)
            out_len = ol.to(device=self.device, dtype=torch.int32).clamp(min=0).contiguous()
            if out_len.numel() != B:
                raise ValueError("%d rows, %d output lengths" % (B, out_len.numel()))
            ol_ptr = _ptr(out_len)
        O = max(1, int(out_len.max().item()) if out_pad is None else int(out_pad))
        asked = out_len                                 # ol_ptr points into it: it lives until the call has been issued
        out_len = out_len.clamp(max=O)
        wb = ctypes.c_size_t()
        _lib.check(lib.mi355asr_istft_workspace_bytes(B, Fpad, *self._sizes(), ctypes.byref(wb)))
        ws = torch.empty(wb.value // 4, dtype=torch.float32, device=self.device)
        y = torch.empty((B, O), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mi355asr_istft_ragged(_ptr(S), _ptr(fr), B, Fpad, *self._sizes(), ol_ptr, _ptr(y), O, _ptr(ws), wb.value,
                                                 _stream(self.device)))
        self._keep = (S, fr, asked, ws)
        return y, out_len
