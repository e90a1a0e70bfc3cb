"""Far-field simulation on the device: what the reference's augmentations/augments.py does on the host with rir_generator,
scipy.signal.convolve and NumPy -- image-source room impulse responses (`ImageSourceRIR`), reverberation of a ragged batch
(`Reverb`), noise at a given SNR (`AddNoise`), the three in a row (`FarField`) and the reference's `Augmentation` class for
its keys `rir` and `noise`.  The kernels are csrc/augment.hip; there is no CPU path.

    rir = ImageSourceRIR(16000)                                   # SignalRIR's room: 5 x 4 x 6 m, T60 0.4 s, 4096 taps
    h = rir.generate(sources, receivers)                          # [B, 4096] float32 on the device
    y, out_len = Reverb()(x, lengths, h)                          # row b: lengths[b] + 4095 samples
    y = AddNoise()(y, out_len, noise, snr_db, quantise=True)

    ff = FarField(rir, noise_bank=[n0, n1], snr=(0, 15))
    y, out_len = ff(x, lengths, np.random.default_rng(0))
    asr.offline_stt_batch(items, augment=ff)                      # what does the model hear in that room at that SNR

The reference's spectral augmentations that need an STFT and its inverse (csrc/stft.hip, stft.py): `SpecAug` is SignalSpecAug,
`TimeStretch` is librosa.effects.time_stretch and `Speed` is SignalSpeed on top of it; `Augmentation(config, enable=("spec_aug",
"speed"))` runs those two keys on the device as well.

    y, out_len = SpecAug(window=10, ratio=0.5)(x, lengths)        # row b: 160 (lengths[b] // 160) samples
    y, out_len = TimeStretch()(x, lengths, rates)                 # row b: int(round(lengths[b] / rates[b])) samples

The two that work on the samples themselves (csrc/iir.hip, iir.py): `Hz` is SignalHz -- a 3rd-order Butterworth band-stop run
forward and backward (scipy.signal.filtfilt) plus a little uniform noise -- and `Mask` is SignalMask; `enable=("hz", "masking")`.

    y, out_len = Hz()(x, lengths, starts=[0.2, 0.5])              # row b: the band [starts[b], starts[b] + 0.3] of Nyquist removed
    y, out_len = Mask("(0.1,0.9)", 0.3)(x, lengths)               # 30 % of the samples of the middle 80 % replaced by noise

`Pitch` is SignalPitch: librosa.effects.pitch_shift on the zone of a row, that is TimeStretch and then a band-limited resampler at
an irrational ratio (csrc/sinc_resample.hip, resample.SincResampler).  The resampler restates the published algorithm behind
resampy's kaiser_best and is pinned against the tests' float64 restatement of it, not against the resampy or librosa packages, so
`Augmentation` runs the key only when asked with `unpinned=("pitch",)`.

    y, out_len = Pitch("(0.2,0.8)")(x, lengths, steps=[-3, 2.5])  # the middle 60 % of row b shifted by steps[b] semitones
"""
import ctypes
import random

import numpy as np

MAX_TAPS = 16384          # the longest filter mi355asr_fir_ragged takes, and the longest response mi355asr_rir_generate writes
UNSUPPORTED = ("masking", "pitch", "speed", "hz", "vc", "spec_aug")     # the reference's other augmentations: off unless enable= / unpinned= name them
KEYS = ("noise", "rir") + UNSUPPORTED


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _rows(x, device, allow_int16=True):
    """x [L] or [B, L], NumPy or tensor -> a contiguous float32 (or int16) tensor [B, max(L, 1)] on the device, and L"""
    import torch
    if isinstance(x, np.ndarray):
        if not (allow_int16 and x.dtype == np.int16):
            x = np.asarray(x, np.float32)
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x, np.float32))
    if not (allow_int16 and x.dtype == torch.int16):
        x = x.to(torch.float32)
    if x.dim() == 1:
        x = x.reshape(1, -1)
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError("expected [L] or [B, L] with B >= 1, got %s" % (tuple(x.shape),))
    L = int(x.shape[1])
    if L == 0:
        x = torch.zeros((x.shape[0], 1), dtype=x.dtype)
    return x.to(device).contiguous(), L


def _lengths(lengths, B, L, device):
    import torch
    if lengths is None:
        return torch.full((B,), L, dtype=torch.int32, device=device)
    ln = lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths))
    ln = ln.reshape(-1).to(device=device, dtype=torch.int32).clamp(0, L).contiguous()
    if ln.numel() != B:
        raise ValueError("%d rows, %d lengths" % (B, ln.numel()))
    return ln


class ImageSourceRIR:
    """Room impulse responses by the image-source method (Habets' rir_generator for an omnidirectional microphone, 3-D, every
    reflection order; DESIGN.md section 19 has the definition -- equality with the PyPI package has not been checked).  The
    defaults are SignalRIR's; `hp_filter` defaults to the package's (on).  Give `beta` (six reflection coefficients, x1 x2 y1
    y2 z1 z2) instead of `reverberation_time` to set the walls directly."""

    def __init__(self, sample_rate, room=(5, 4, 6), reverberation_time=0.4, nsample=4096, c=340, beta=None, hp_filter=True,
                 device="cuda:0"):
        self.sample_rate, self.c = float(sample_rate), float(c)
        self.room = tuple(float(v) for v in room)
        self.nsample, self.hp_filter, self.device = int(nsample), bool(hp_filter), device
        if len(self.room) != 3 or min(self.room) <= 0 or self.sample_rate <= 0 or self.c <= 0:
            raise ValueError("room %s, sample rate %g, sound speed %g: all must be positive" % (self.room, self.sample_rate, self.c))
        if not 1 <= self.nsample <= MAX_TAPS:
            raise ValueError("nsample = %d is outside 1 .. %d" % (self.nsample, MAX_TAPS))
        if beta is not None:
            self.beta, self.reverberation_time = [float(b) for b in beta], 0.0
            if len(self.beta) != 6 or max(abs(b) for b in self.beta) > 1:
                raise ValueError("beta: six reflection coefficients within [-1, 1], got %s" % (beta,))
        else:
            self.reverberation_time = float(reverberation_time)
            Lx, Ly, Lz = self.room
            alpha = 24 * Lx * Ly * Lz * np.log(10.0) / (self.c * 2 * (Lx * Lz + Ly * Lz + Lx * Ly) * self.reverberation_time) \
                if self.reverberation_time > 0 else np.inf
            if alpha > 1:
                raise ValueError("reverberation_time = %g s is too short for the room %s: alpha = %g > 1"
                                 % (self.reverberation_time, self.room, alpha))
            self.beta = [float(np.sqrt(1 - alpha))] * 6

    def params(self, sources, receivers):
        """the [B, 20] float64 table mi355asr_rir_generate takes; ValueError for a position outside the room or a source at
        its receiver"""
        s = np.asarray(sources, np.float64).reshape(-1, 3)
        r = np.asarray(receivers, np.float64).reshape(-1, 3)
        if len(s) != len(r) or not len(s):
            raise ValueError("%d sources, %d receivers" % (len(s), len(r)))
        room = np.asarray(self.room)
        for name, p in (("source", s), ("receiver", r)):
            bad = np.argwhere((p < 0) | (p > room) | ~np.isfinite(p))
            if len(bad):
                raise ValueError("%s %d at %s is outside the room %s" % (name, bad[0][0], tuple(p[bad[0][0]]), self.room))
        same = np.all(s == r, axis=1)
        if same.any():
            raise ValueError("row %d: the source is at the receiver %s" % (int(np.argmax(same)), tuple(s[np.argmax(same)])))
        t = np.zeros((len(s), 20), np.float64)
        t[:, 0:3], t[:, 3:6], t[:, 6:9] = room, s, r
        t[:, 9], t[:, 10], t[:, 11] = self.c, self.sample_rate, self.reverberation_time
        t[:, 12:18] = self.beta
        t[:, 18], t[:, 19] = float(self.hp_filter), self.nsample
        return t

    def generate(self, sources, receivers):
        """sources, receivers [B, 3] in metres -> h [B, nsample] float32 on the device"""
        import torch
        from . import _lib
        lib = _lib.lib()
        t = np.ascontiguousarray(self.params(sources, receivers))
        B = len(t)
        wb = ctypes.c_size_t()
        _lib.check(lib.mi355asr_rir_workspace_bytes(B, ctypes.byref(wb)))
        ws = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        h = torch.empty((B, self.nsample), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mi355asr_rir_generate(t.ctypes.data_as(ctypes.c_void_p), B, _ptr(h), self.nsample, _ptr(ws), wb.value,
                                                 _stream(self.device)))
        self._keep = ws                                 # the table of an asynchronous call
        return h


class Reverb:
    """Full convolution of a ragged batch with one filter per row (or one for all): scipy.signal.convolve(x, h) per row."""

    def __init__(self, device="cuda:0"):
        self.device = device

    def __call__(self, x, lengths, h, out_pad=None, taps=None):
        """x [L] or [B, L] float32 or int16 (x / 32768); lengths [B] or None; h [B, K], or [K] / [1, K] shared by every row
        (taps: use the first `taps` columns of h only) -> (y [B, L + K - 1] float32 on the device, or `out_pad` columns; out_len int32 [B] on the device: lengths + K - 1, 0
        for an empty row).  Row b is computed as if alone; zeros after its out_len[b] samples."""
        import torch
        from . import _lib
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        h, K = _rows(h, self.device, allow_int16=False)
        if taps is not None:
            if not 1 <= int(taps) <= K:
                raise ValueError("taps = %d of a filter of %d columns" % (taps, K))
            K = int(taps)
        if not 1 <= K <= MAX_TAPS:
            raise ValueError("a filter of %d taps is outside 1 .. %d" % (K, MAX_TAPS))
        if h.shape[0] not in (1, B):
            raise ValueError("%d rows, %d filters" % (B, h.shape[0]))
        shared = h.shape[0] == 1
        O = max(1, L + K - 1 if out_pad is None else int(out_pad))
        y = torch.empty((B, O), dtype=torch.float32, device=self.device)
        out_len = torch.where(ln > 0, ln + (K - 1), torch.zeros_like(ln)).clamp(max=O)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mi355asr_fir_ragged(_ptr(x), 4 if x.dtype == torch.int16 else 0, _ptr(ln), B, int(x.shape[1]), _ptr(h),
                                                      K, int(h.shape[1]), int(shared), _ptr(y), O,
                                                      _stream(self.device)))
        self._keep = (x, ln, h)                         # inputs of an asynchronous call
        return y, out_len


class AddNoise:
    """SignalNoise.Add_noise per row, with the powers in float64: y = x + sqrt(P_x / 10^(snr_db / 10) / P_d) d.  A silent
    row or silent noise gives y = x (the reference divides by zero there).  quantise: Augmentation.process's clip and
    truncation to 16 bits."""

    def __init__(self, device="cuda:0"):
        self.device = device

    def __call__(self, x, lengths, noise, snr_db, quantise=False):
        """x [B, L] float32; noise [B, >= L]: lengths[b] samples of row b are used; snr_db a number or [B] -> y [B, L] on the device"""
        import torch
        from . import _lib
        x, L = _rows(x, self.device, allow_int16=False)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        d, D = _rows(noise, self.device, allow_int16=False)
        if d.shape[0] != B or d.shape[1] < x.shape[1]:
            raise ValueError("noise %s does not cover the batch %s" % (tuple(d.shape), tuple(x.shape)))
        snr = torch.as_tensor(np.broadcast_to(np.asarray(snr_db.cpu() if torch.is_tensor(snr_db) else snr_db, np.float32), (B,)).copy())
        snr = snr.to(self.device)
        y = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mi355asr_mix_snr(_ptr(x), _ptr(ln), _ptr(d), _ptr(snr), B, int(x.shape[1]), int(d.shape[1]),
                                                   int(bool(quantise)), _ptr(y), _stream(self.device)))
        self._keep = (x, ln, d, snr)
        return y if L else y[:, :0]


def cut_noise(noise, n, start_draw):
    """SignalNoise.augment's rule: the recording doubled until it is longer than n + 20, then n samples from a drawn start;
    start_draw(high) -> an integer in [0, high) is called once, with high = len(doubled) - n - 10"""
    noise = np.asarray(noise, np.float32).reshape(-1)
    if not len(noise):
        raise ValueError("an empty noise recording")
    while n + 20 > len(noise):
        noise = np.hstack((noise, noise))
    start = int(start_draw(len(noise) - n - 10))
    return noise[start:start + n]


def draw_position(room, draw):
    """SignalRIR.get_num: each coordinate one of the 10 L_d decimetre marks 0, 0.1, ... below L_d; draw(high) -> [0, high)"""
    return [draw(int(d) * 10) / 10.0 for d in room]


class FarField:
    """Reverberation, then noise, then the 16-bit quantisation, on the device; positions, noise segments and SNRs are drawn on
    the host from `rng` (a numpy.random.Generator).  rir: an ImageSourceRIR (a source and a receiver are drawn per row on the
    room's decimetre grid, redrawn when they coincide), a fixed filter (array [K]), or None: no reverberation.  noise_bank: a
    list of 1-D recordings, or None: no noise.  snr: integers are drawn from [snr[0], snr[1]).  The draws of the last call are
    kept in `last`."""

    def __init__(self, rir=None, noise_bank=None, snr=(0, 15), quantise=True, device="cuda:0", seed=0):
        self.rir, self.snr, self.quantise, self.device = rir, (int(snr[0]), int(snr[1])), bool(quantise), device
        self.noise_bank = None if noise_bank is None else [np.asarray(n, np.float32).reshape(-1) for n in noise_bank]
        self.rng = np.random.default_rng(seed)
        self.reverb, self.add_noise = Reverb(device), AddNoise(device)
        self.last = {}

    def __call__(self, x, lengths=None, rng=None):
        """-> (y [B, L'] float32 on the device, out_len int32 [B] on the device)"""
        import torch
        rng = self.rng if rng is None else rng
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        self.last = {}
        if isinstance(self.rir, ImageSourceRIR):
            draw = lambda high: int(rng.integers(0, high))
            rec, src = [], []
            for _ in range(B):
                r = draw_position(self.rir.room, draw)
                s = draw_position(self.rir.room, draw)
                while s == r:
                    s = draw_position(self.rir.room, draw)
                rec.append(r)
                src.append(s)
            self.last.update(sources=src, receivers=rec)
            x, ln = self.reverb(x, ln, self.rir.generate(src, rec))
        elif self.rir is not None:
            x, ln = self.reverb(x, ln, self.rir)
        elif x.dtype != torch.float32:
            x = x.to(torch.float32) / 32768.0
        if self.noise_bank:
            lens = ln.cpu().numpy()
            W = int(x.shape[1])
            d = np.zeros((B, W), np.float32)
            picks, starts, snrs = [], [], []
            for b in range(B):
                picks.append(int(rng.integers(0, len(self.noise_bank))))
                d[b, :lens[b]] = cut_noise(self.noise_bank[picks[-1]], int(lens[b]),
                                           lambda high: starts.append(int(rng.integers(0, high))) or starts[-1])
                snrs.append(int(rng.integers(self.snr[0], self.snr[1])))
            self.last.update(noise=picks, starts=starts, snr_db=snrs)
            x = self.add_noise(x, ln, d, np.asarray(snrs, np.float32), quantise=self.quantise)
        elif self.quantise:
            x = self.add_noise(x, ln, torch.zeros_like(x), 0.0, quantise=True)
        return x, ln


class SpecAug:
    """SignalSpecAug on the device: the STFT at (1024, 800, 160), `int(frames * ratio)` blocks of up to 2 window x 2 window
    bins and frames zeroed around drawn centres, the inverse STFT.  One frame-local pass: the spectrum is never written to
    memory (mi355asr_spec_aug).  The last call's centres are kept in `last`."""
    N_FFT, WIN, HOP, BINS = 1024, 800, 160, 513

    def __init__(self, window=10, ratio=0.5, device="cuda:0"):
        self.window, self.ratio, self.device = int(window), float(ratio), device
        if self.window < 0 or self.ratio < 0:
            raise ValueError("window = %d and ratio = %g must not be negative" % (self.window, self.ratio))
        self.last = []

    def frames(self, n):
        return 1 + int(n) // self.HOP if int(n) >= self.BINS else 0

    def draw(self, n_frames):
        """the reference's two random.sample calls in its order -- the frames, then the bins -- as [nums, 2] pairs (h_, w_);
        ValueError, as there, when int(n_frames * ratio) exceeds the 513 bins (or the frames)"""
        nums = int(n_frames * self.ratio)
        ws = random.sample(list(range(n_frames)), nums)
        hs = random.sample(list(range(self.BINS)), nums)
        return np.array(list(zip(hs, ws)), np.int32).reshape(-1, 2)

    def __call__(self, x, lengths=None, centres=None):
        """x [L] or [B, L] float32 or int16; lengths [B] or None; centres: one [n, 2] array of (h_, w_) per row, or None: drawn
        with `draw` row by row -> (y [B, max(1, L)] float32 on the device, out_len int32 [B] on the device: 160 (len // 160); a row
        with fewer than 513 samples has no frame and comes back unchanged, out_len = len)."""
        import torch
        from . import _lib
        lib = _lib.lib()
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        lens = ln.cpu().numpy()
        if centres is None:
            centres = []
            for b in range(B):
                F = self.frames(lens[b])
                if int(F * self.ratio) > min(self.BINS, F):
                    raise ValueError("row %d: %d frames at ratio %g ask for %d centres, more than the %d bins random.sample can draw"
                                     % (b, F, self.ratio, int(F * self.ratio), self.BINS))
                centres.append(self.draw(F))
        centres = [np.asarray(c, np.int32).reshape(-1, 2) for c in centres]
        if len(centres) != B:
            raise ValueError("%d rows, %d sets of centres" % (B, len(centres)))
        for b, c in enumerate(centres):
            if len(c) > self.BINS:
                raise ValueError("row %d: %d centres, more than the %d bins random.sample can draw" % (b, len(c), self.BINS))
        self.last = centres
        Npad = max(1, max(len(c) for c in centres))
        table = np.zeros((B, Npad, 2), np.int32)
        for b, c in enumerate(centres):
            table[b, :len(c)] = c
        ce = torch.from_numpy(table).to(self.device)
        counts = torch.tensor([len(c) for c in centres], dtype=torch.int32).to(self.device)
        W = int(x.shape[1])
        wb = ctypes.c_size_t()
        _lib.check(lib.mi355asr_spec_aug_workspace_bytes(B, W, ctypes.byref(wb)))
        ws = torch.empty(wb.value // 4, dtype=torch.float32, device=self.device)
        y = torch.empty((B, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mi355asr_spec_aug(_ptr(x), 4 if x.dtype == torch.int16 else 0, _ptr(ln), B, W, _ptr(ce), Npad, _ptr(counts),
                                             self.window, _ptr(y), W, _ptr(ws), wb.value, _stream(self.device)))
        self._keep = (x, ln, ce, counts, ws)
        out_len = torch.where(ln >= self.BINS, (ln // self.HOP) * self.HOP, ln).to(torch.int32)
        return y, out_len


class TimeStretch:
    """librosa.effects.time_stretch (librosa 0.9) per row: the STFT at (2048, 2048, 512), the phase vocoder at the row's rate,
    the inverse STFT cut or zero-filled to int(round(len / rate)) samples.  Three library calls, everything on the device."""
    N_FFT, HOP = 2048, 512

    def __init__(self, device="cuda:0"):
        from .stft import STFT
        self.device = device
        self.stft = STFT(self.N_FFT, device=device)

    def __call__(self, x, lengths, rates):
        """x [L] or [B, L]; lengths [B] or None; rates: a number or [B], each > 0 -> (y [B, O] float32 on the device, out_len
        int32 [B] on the device).  A row with fewer than 1025 samples has no frame (librosa raises there) and gives zeros."""
        import torch
        from . import _lib
        lib = _lib.lib()
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        lens = ln.cpu().numpy()
        rates = np.ascontiguousarray(np.broadcast_to(np.asarray(rates, np.float64).reshape(-1), (B,)))
        if not (rates > 0).all() or not np.isfinite(rates).all():
            raise ValueError("rates must be positive, got %s" % (rates,))
        S, frames = self.stft.forward(x, ln)
        Fh = [1 + int(n) // self.HOP if n >= self.N_FFT // 2 + 1 else 0 for n in lens]
        tc = np.array([len(np.arange(0, F, r, dtype=np.float64)) for F, r in zip(Fh, rates)], np.int32)
        out_len = np.array([int(round(int(n) / r)) for n, r in zip(lens, rates)], np.int32)
        Tpad = max(1, int(tc.max()))
        S2 = torch.empty((B, Tpad, self.stft.bins), dtype=torch.complex64, device=self.device)
        wb = ctypes.c_size_t()
        _lib.check(lib.mi355asr_phase_vocoder_workspace_bytes(B, ctypes.byref(wb)))
        ws = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.mi355asr_phase_vocoder(_ptr(S), _ptr(frames), B, int(S.shape[1]), self.N_FFT, self.N_FFT, self.HOP,
                                                  rates.ctypes.data_as(ctypes.c_void_p), tc.ctypes.data_as(ctypes.c_void_p), _ptr(S2),
                                                  Tpad, _ptr(ws), wb.value, _stream(self.device)))
        self._keep = (S, frames, ws)
        return self.stft.inverse(S2, tc, out_lengths=out_len)


class Speed:
    """SignalSpeed: a rate drawn as np.random.random() * factor[1] clipped to [factor[0], factor[1]], then TimeStretch.  factor is
    a pair or, as in the reference's configuration, its text."""
    key = "speed"

    def __init__(self, factor="(0.5,2)", device="cuda:0"):
        if isinstance(factor, str):
            import ast
            factor = ast.literal_eval(factor)
        self.factor = (float(factor[0]), float(factor[1]))
        if not 0 < self.factor[0] <= self.factor[1]:
            raise ValueError("factor = %s: need 0 < factor[0] <= factor[1]" % (factor,))
        self.device = device
        self._stretch = None

    def draw(self, n=None):
        return {"rate": float(np.clip(np.random.random() * self.factor[1], self.factor[0], self.factor[1]))}

    def __call__(self, x, lengths=None, rates=None):
        """rates None: one draw per row"""
        if self._stretch is None:
            self._stretch = TimeStretch(self.device)
        x, L = _rows(x, self.device)
        if rates is None:
            rates = [self.draw()["rate"] for _ in range(int(x.shape[0]))]
        return self._stretch(x, _lengths(lengths, int(x.shape[0]), L, self.device), rates)


class _SpecAug(SpecAug):
    """SignalSpecAug inside Augmentation: its draws for an utterance of n samples"""
    key = "spec_aug"

    def draw(self, n):
        F = self.frames(n)
        if int(F * self.ratio) > min(self.BINS, F):
            raise ValueError("an utterance of %d samples has %d frames: ratio %g asks for %d centres, more than the %d bins "
                             "random.sample can draw" % (n, F, self.ratio, int(F * self.ratio), self.BINS))
        return {"centres": SpecAug.draw(self, F)}


class Hz:
    """SignalHz on the device: scipy.signal.filtfilt of butter(3, [start, start + 0.3], "bandstop") plus 0.001 times uniform
    noise, per row.  The filter runs as second-order sections in float64 (SOSFilter.sosfiltfilt with padlen = 21, which is
    filtfilt's 3 max(len(a), len(b)); DESIGN.md section 21 has why the transfer-function form cannot be cut into chunks).  A row
    of at most 21 samples, where SciPy raises, comes back unchanged (noise and quantisation still applied), as SpecAug returns a
    row without a frame.  The last call's starts are kept in `last`."""
    key = "hz"
    PADLEN, WIDTH, NOISE = 21, 0.3, 0.001

    def __init__(self, device="cuda:0"):
        from .iir import SOSFilter
        self.device = device
        self.filter = SOSFilter(device)
        self.last = None

    @staticmethod
    def draw_start():
        return float(np.clip(np.random.random(), 0.01, 0.699))

    def draw(self, n):
        """the reference's np.random calls in its order: random() for the start, then random(n) for the noise"""
        start = self.draw_start()
        return {"start": start, "u": np.random.random(int(n))}

    @staticmethod
    def sections(start):
        from scipy import signal            # lazy, as featurizers does: only the filter design needs SciPy
        return signal.butter(3, [start, start + Hz.WIDTH], "bandstop", output="sos")

    def __call__(self, x, lengths=None, starts=None, noise=None, quantise=False):
        """x [L] or [B, L] float32 or int16; lengths [B] or None; starts: one number per row (or one for all), None: drawn per
        row as np.clip(np.random.random(), 0.01, 0.699); noise: [B, L] float64 uniforms (scaled by 0.001 in the kernel), None:
        drawn on the device, False: none -> (y [B, L] float32 on the device, out_len int32 [B] on the device: lengths)"""
        import torch
        x, L = _rows(x, self.device)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        if starts is None:
            starts = [self.draw_start() for _ in range(B)]
        starts = np.broadcast_to(np.asarray(starts, np.float64).reshape(-1), (B,)).copy()
        if not ((starts > 0) & (starts + self.WIDTH < 1)).all():
            raise ValueError("starts must lie in (0, %g), got %s" % (1 - self.WIDTH, starts))
        self.last = starts
        same = bool((starts == starts[0]).all())
        sos = self.sections(starts[0]) if same else np.stack([self.sections(s) for s in starts])
        if noise is None:
            noise = torch.rand((B, int(x.shape[1])), dtype=torch.float64, device=self.device)
        elif noise is False:
            noise = None
        y, _ = self.filter._run(x, ln, sos, 1, self.PADLEN, None, False, noise, self.NOISE, quantise, short_rows="copy")
        return y, ln


class Mask:
    """SignalMask on the device: in the zone [int(len zone[0]), int(len zone[1])) of a row, the samples whose uniform draw u is
    below mask_ratio are replaced by u itself (mask_with_noise) or by 0.  zone is a pair within [0, 1] or, as in the
    reference's configuration, its text."""
    key = "masking"

    def __init__(self, zone="(0.1,0.9)", mask_ratio=0.3, mask_with_noise=True, device="cuda:0"):
        if isinstance(zone, str):
            import ast
            zone = ast.literal_eval(zone)
        self.zone = (float(zone[0]), float(zone[1]))
        if not (0 <= self.zone[0] <= 1 and 0 <= self.zone[1] <= 1):
            raise ValueError("zone = %s must lie within [0, 1]" % (zone,))
        self.mask_ratio, self.mask_with_noise, self.device = float(mask_ratio), bool(mask_with_noise), device

    def span(self, n):
        """(s, e) of a row of n samples: Python's int() of the float64 products; e - s draws are used (none when e <= s)"""
        return int(n * self.zone[0]), int(n * self.zone[1])

    def draw(self, n):
        """the reference's np.random call: random(e - s)"""
        s, e = self.span(n)
        return {"u": np.random.random(max(e - s, 0))}

    def __call__(self, x, lengths=None, u=None, quantise=False):
        """x [L] or [B, L] float32; lengths [B] or None; u: [B, >= e - s] float64 uniforms, or one array per row, None: drawn on
        the device -> (y [B, L] float32 on the device, out_len int32 [B] on the device: lengths)"""
        import torch
        from . import _lib
        x, L = _rows(x, self.device, allow_int16=False)
        B, W = int(x.shape[0]), int(x.shape[1])
        ln = _lengths(lengths, B, L, self.device)
        if u is None:
            u = torch.rand((B, W), dtype=torch.float64, device=self.device)
        elif isinstance(u, (list, tuple)):
            rows = [np.asarray(r, np.float64).reshape(-1) for r in u]
            u = np.zeros((len(rows), max(1, max(len(r) for r in rows))), np.float64)
            for b, r in enumerate(rows):
                u[b, :len(r)] = r
        if not torch.is_tensor(u):
            u = torch.from_numpy(np.ascontiguousarray(np.asarray(u, np.float64)))
        u = u.to(torch.float64).reshape(B, -1) if u.numel() else torch.zeros((B, 1), dtype=torch.float64)
        spans = [self.span(int(n)) for n in ln.cpu().numpy()]
        need = max([e - s for s, e in spans] + [0])
        if u.shape[0] != B or u.shape[1] < need:
            raise ValueError("u %s does not cover the zones of the batch: %d rows, up to %d draws" % (tuple(u.shape), B, need))
        u = u.to(self.device).contiguous()
        y = torch.empty((B, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mi355asr_mask_zone(_ptr(x), _ptr(ln), _ptr(u), B, W, int(u.shape[1]), self.zone[0], self.zone[1],
                                                     self.mask_ratio, int(self.mask_with_noise), int(bool(quantise)), _ptr(y),
                                                     _stream(self.device)))
        self._keep = (x, ln, u)
        return (y if L else y[:, :0]), ln


class Pitch:
    """SignalPitch on the device: librosa.effects.pitch_shift (librosa 0.9) on the zone [int(len zone[0]), int(len zone[1])) of a
    row -- TimeStretch at rate = 2^(-steps / 12), then the band-limited resampler (resample.SincResampler) at the ratio `rate`
    for ceil(len_stretched rate) samples, cut or zero-filled to the zone's length and written over the zone in the same launch.
    Samples outside the zone keep the input's bits.  The resampler follows the published algorithm behind resampy's kaiser_best
    and is pinned against the tests' float64 restatement of it; it has not been compared with the resampy or librosa packages
    (DESIGN.md section 22).  A row whose rate is exactly 1.0 takes the stretched samples as they are (librosa's orig_sr ==
    target_sr shortcut).  A zone of fewer than 1025 samples has no STFT frame: librosa raises there, here the row comes back
    unchanged.  zone and factor are pairs or, as in the reference's configuration, their text.  The last call's steps are kept
    in `last`."""
    key = "pitch"
    MIN_ZONE = 1025

    def __init__(self, zone="(0.2,0.8)", sample_rate=16000, factor="(-1,5)", device="cuda:0"):
        import ast
        if isinstance(zone, str):
            zone = ast.literal_eval(zone)
        if isinstance(factor, str):
            factor = ast.literal_eval(factor)
        self.zone = (float(zone[0]), float(zone[1]))
        self.factor = (float(factor[0]), float(factor[1]))
        if not (0 <= self.zone[0] <= 1 and 0 <= self.zone[1] <= 1):
            raise ValueError("zone = %s must lie within [0, 1]" % (zone,))
        self.sample_rate, self.device = int(sample_rate), device
        self.last = None
        self._stretch = self._sinc = None

    def span(self, n):
        """(s, e) of a row of n samples: Python's int() of the float64 products"""
        return int(n * self.zone[0]), int(n * self.zone[1])

    def draw(self, n=None):
        """the reference's np.random call: one random(), scaled to factor[1] - factor[0] and centred on 0"""
        scale = self.factor[1] - self.factor[0]
        return {"steps": float(np.random.random() * scale - scale / 2)}

    @staticmethod
    def rate(steps):
        """librosa's 2.0 ** (-n_steps / bins_per_octave) with 12 bins per octave"""
        return 2.0 ** (-float(steps) / 12)

    def __call__(self, x, lengths=None, steps=None, quantise=False):
        """x [L] or [B, L] float32; lengths [B] or None; steps: semitones, one number per row (or one for all), None: drawn per
        row -> (y [B, L] float32 on the device, out_len int32 [B] on the device: lengths).  quantise: Augmentation.process's
        clip and truncation to 16 bits, of the whole row."""
        import torch
        from .resample import SincResampler
        if self._stretch is None:
            self._stretch, self._sinc = TimeStretch(self.device), SincResampler(self.device)
        x, L = _rows(x, self.device, allow_int16=False)
        B = int(x.shape[0])
        ln = _lengths(lengths, B, L, self.device)
        lens = ln.cpu().numpy()
        if steps is None:
            steps = [self.draw()["steps"] for _ in range(B)]
        steps = np.broadcast_to(np.asarray(steps, np.float64).reshape(-1), (B,)).copy()
        if not np.isfinite(steps).all():
            raise ValueError("steps must be finite, got %s" % (steps,))
        self.last = steps
        rates = np.array([self.rate(s) for s in steps], np.float64)
        spans = [self.span(int(n)) for n in lens]
        zl = np.array([e - s if e - s >= self.MIN_ZONE else 0 for s, e in spans], np.int64)     # 0: the row is left as it is
        y = x.clone()
        if zl.any():
            self._sinc.ratios(rates[zl > 0], int((zl > 0).sum()))          # a rate outside the resampler's bounds: ValueError
            Z = int(zl.max())
            col = torch.arange(Z, device=self.device)[None, :] + torch.tensor([s for s, _ in spans], device=self.device)[:, None]
            z = torch.gather(x, 1, col.clamp(max=int(x.shape[1]) - 1)).contiguous()
            ys, ls = self._stretch(z, zl.astype(np.int32), rates)
            ls = ls.cpu().numpy().astype(np.int64)
            same = (rates == 1.0) & (zl > 0)
            go = (zl > 0) & ~same
            if go.any():
                self._sinc.launch(ys.contiguous(), np.where(go, ls, 0), np.where(go, rates, 1.0), np.where(go, zl, 0),
                                  np.array([s for s, _ in spans], np.int64), y)
            for b in np.nonzero(same)[0]:
                y[b, spans[b][0]:spans[b][1]] = ys[b, :zl[b]]
        if quantise:
            y = AddNoise(self.device)(y, ln, torch.zeros_like(y), 0.0, quantise=True)
        return (y if L else y[:, :0]), ln


DEVICE_KEYS = ("spec_aug", "speed")      # UNSUPPORTED keys that Augmentation(..., enable=) can run on the device
SIGNAL_KEYS = ("hz", "masking")          # and the two that filter or mask the samples themselves (Hz, Mask)
UNPINNED_KEYS = ("pitch",)               # Augmentation(..., unpinned=): on the device through a filter of the project's own
#                                          restatement of the published algorithm, not pinned to the reference's library (Pitch)


class _RirAug:
    """SignalRIR: its draws (host) and its constants"""
    key = "rir"

    def __init__(self, sample_rate):
        self.sample_rate = sample_rate
        self.room = (5, 4, 6)

    def draw(self, n):
        """the receiver, then the source, as SignalRIR.augment calls get_num; the source is redrawn while it is at the receiver
        (the reference would hand rir_generator a zero distance)"""
        draw = lambda high: random.sample(list(range(high)), 1)[0]
        r = draw_position(self.room, draw)
        s = draw_position(self.room, draw)
        while s == r:
            s = draw_position(self.room, draw)
        return {"receiver": r, "source": s}


class _NoiseAug:
    """SignalNoise: its draws (host) over a bank of recordings"""
    key = "noise"

    def __init__(self, sample_rate=16000, SNR=(-10, 10), noises="", bank=None):
        self.sample_rate, self.SNR = sample_rate, SNR
        if bank is None:
            from .featurizers import read_raw_audio
            with open(noises) as f:
                paths = [ln.strip() for ln in f.readlines()]
            bank = [read_raw_audio(p, sample_rate) for p in paths if p]
        self.bank = [np.asarray(b, np.float32).reshape(-1) for b in bank]

    def draw(self, n):
        """np.random.randint in SignalNoise.augment's order: the recording, the start of the segment, the SNR"""
        pick = int(np.random.randint(0, len(self.bank)))
        start = []
        seg = cut_noise(self.bank[pick], n, lambda high: start.append(int(np.random.randint(0, high))) or start[-1])
        snr = int(np.random.randint(self.SNR[0], self.SNR[1]))
        return {"noise": pick, "start": start[0], "snr_db": snr, "segment": seg}


class Augmentation(dict):
    """The reference's `Augmentation(config["augments_config"])` for its keys `rir` and `noise`, on the device.  An unknown
    key is a KeyError, as there.  An active key among masking, pitch, speed, hz, vc, spec_aug raises NotImplementedError
    naming it; unsupported="skip" drops those keys instead (the shipped am_data.yml has spec_aug active).  process /
    process_batch pick one active augmentation per utterance with random.sample and make the reference's `random` /
    `np.random` calls in its order, so a seeded run draws the reference's positions, segments and SNRs; the one deviation: a
    source drawn at the receiver is drawn again.  noise_bank: recordings to use instead of reading the `noises` list file.
    enable: keys among spec_aug, speed, hz and masking to run on the device as well (SpecAug, Speed, Hz, Mask) instead of
    treating them as unsupported; the default, none, leaves everything above as it is.  unpinned: keys among UNPINNED_KEYS,
    today ("pitch",), to run on the device through a filter that is the project's own restatement of the published algorithm
    and is not pinned to the reference's library (Pitch: the resampler inside librosa's pitch_shift has not been compared with
    the resampy package); without it an active pitch stays unsupported, and enable=("pitch",) stays a ValueError.  vc (TTS
    models) is not built."""

    def __init__(self, config=None, unsupported="raise", noise_bank=None, device="cuda:0", enable=(), unpinned=()):
        if unsupported not in ("raise", "skip"):
            raise ValueError("unsupported must be 'raise' or 'skip', got %r" % (unsupported,))
        enable = (enable,) if isinstance(enable, str) else tuple(enable)
        for key in enable:
            if key not in DEVICE_KEYS + SIGNAL_KEYS:
                raise ValueError("enable: %r is not one of %s" % (key, DEVICE_KEYS + SIGNAL_KEYS))
        unpinned = (unpinned,) if isinstance(unpinned, str) else tuple(unpinned)
        for key in unpinned:
            if key not in UNPINNED_KEYS:
                raise ValueError("unpinned: %r is not one of %s" % (key, UNPINNED_KEYS))
        super().__init__(config or {})
        self.device = device
        self.augmentations = []
        self.skipped = []
        for key, value in self.items():
            if key not in KEYS:
                raise KeyError("No augmentation named: %s\nAvailable augmentations: %s" % (key, list(KEYS)))
            if not value["active"]:
                continue
            kw = {k: v for k, v in value.items() if k != "active"}
            if key in enable:
                cls = {"spec_aug": _SpecAug, "speed": Speed, "hz": Hz, "masking": Mask}[key]
                self.augmentations.append(cls(device=device, **kw))
            elif key in unpinned:
                self.augmentations.append(Pitch(device=device, **kw))
            elif key in UNSUPPORTED:
                if unsupported == "raise":
                    raise NotImplementedError("augmentation '%s' is active and not built here (unsupported='skip' drops it)" % key)
                self.skipped.append(key)
            elif key == "rir":
                self.augmentations.append(_RirAug(**kw))
            else:
                self.augmentations.append(_NoiseAug(bank=noise_bank, **kw))
        self._rirs = {}

    def __missing__(self, key):
        return None

    def available(self):
        return len(self.augmentations) > 0

    def draw(self, n):
        """the host side of process() for an utterance of n samples: (the augmentation picked, its draws)"""
        aug = random.sample(self.augmentations, 1)[0]
        return aug, aug.draw(n)

    def process(self, wav):
        return self.process_batch([wav])[0]

    def process_batch(self, wavs):
        """-> one float32 array per utterance: reverberated (len + 4095 samples), with noise added, with blocks of its spectrum
        zeroed (160 (len // 160) samples), time-stretched (int(round(len / rate)) samples), band-stopped, masked or pitch-shifted
        (len samples); clipped and quantised"""
        import torch
        wavs = [np.asarray(w, np.float32).reshape(-1) for w in wavs]
        drawn = [self.draw(len(w)) for w in wavs]
        out = [None] * len(wavs)
        for key in ("rir", "noise") + DEVICE_KEYS + SIGNAL_KEYS + UNPINNED_KEYS:
            rows = [i for i, (aug, _) in enumerate(drawn) if aug.key == key]
            if not rows:
                continue
            lens = np.array([len(wavs[i]) for i in rows], np.int32)
            x = np.zeros((len(rows), max(1, int(lens.max()))), np.float32)
            for k, i in enumerate(rows):
                x[k, :lens[k]] = wavs[i]
            if key == "rir":
                aug = drawn[rows[0]][0]
                if aug.sample_rate not in self._rirs:
                    self._rirs[aug.sample_rate] = ImageSourceRIR(aug.sample_rate, device=self.device)
                h = self._rirs[aug.sample_rate].generate([drawn[i][1]["source"] for i in rows], [drawn[i][1]["receiver"] for i in rows])
                y, ln = Reverb(self.device)(x, lens, h)
                y = AddNoise(self.device)(y, ln, np.zeros((len(rows), int(y.shape[1])), np.float32), 0.0, quantise=True)
                ln = ln.cpu().numpy()
            elif key in SIGNAL_KEYS:
                aug = drawn[rows[0]][0]
                if key == "hz":
                    u = np.zeros(x.shape, np.float64)
                    for k, i in enumerate(rows):
                        u[k, :lens[k]] = drawn[i][1]["u"]
                    y, ln = aug(x, lens, starts=[drawn[i][1]["start"] for i in rows], noise=u, quantise=True)
                else:
                    y, ln = aug(x, lens, u=[drawn[i][1]["u"] for i in rows], quantise=True)
                ln = ln.cpu().numpy()
            elif key in UNPINNED_KEYS:
                y, ln = drawn[rows[0]][0](x, lens, steps=[drawn[i][1]["steps"] for i in rows], quantise=True)
                ln = ln.cpu().numpy()
            elif key in DEVICE_KEYS:
                aug = drawn[rows[0]][0]
                if key == "spec_aug":
                    y, ln = aug(x, lens, centres=[drawn[i][1]["centres"] for i in rows])
                else:
                    y, ln = aug(x, lens, rates=[drawn[i][1]["rate"] for i in rows])
                y = AddNoise(self.device)(y, ln, torch.zeros_like(y), 0.0, quantise=True)
                ln = ln.cpu().numpy()
            else:
                d = np.zeros_like(x)
                for k, i in enumerate(rows):
                    d[k, :lens[k]] = drawn[i][1]["segment"]
                y = AddNoise(self.device)(x, lens, d, np.array([drawn[i][1]["snr_db"] for i in rows], np.float32), quantise=True)
                ln = lens
            yh = y.cpu().numpy()
            for k, i in enumerate(rows):
                out[i] = yh[k, :ln[k]].copy()
        return out
