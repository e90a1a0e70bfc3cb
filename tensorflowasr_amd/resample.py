"""Polyphase resampling on the device: what `featurizers._resample` (scipy.signal.resample_poly with its defaults) computes on
the host, for ragged batches (`Resampler`) and for many live streams (`StreamResampler`).  The filter is designed here in
float64 with NumPy alone and handed to the kernels of csrc/resample.hip as a phase-major fp32 table; there is no CPU path.

    rs = Resampler(48000, 16000)
    y, out_len = rs(x_int16_or_float32, lengths)          # y [B, Omax] float32 on the device, out_len int32 [B]

    srs = StreamResampler(64, 8000, 16000, max_packet=1280)
    new = srs.step([3, 5], [packet3, packet5])            # {slot: float32 samples that became final}
    tail = srs.flush([3])                                  # the rest, zero-extended; the slot is reset

`SincResampler` is the resampler for ANY real ratio, one ratio per row (csrc/sinc_resample.hip): J. O. Smith's band-limited
interpolation on a tabulated Kaiser-windowed sinc, the algorithm resampy's `kaiser_best` runs inside librosa.effects.pitch_shift.
It follows the published algorithm and is pinned against the tests' float64 restatement of it; it has not been compared with
the resampy or librosa packages, and the four filter constants below are quoted from resampy's documentation.

    y, out_len = SincResampler()(x, lengths, ratios=[2 ** (-3 / 12), 1.19])   # row b: ceil(lengths[b] ratios[b]) samples
"""
import ctypes
from math import gcd

import numpy as np

MAX_RATIO = 640          # max(up, down): the largest filter (12 801 taps, 11.025 kHz -> 16 kHz) the kernels hold in LDS
# the windowed sinc of SincResampler: zero crossings, table entries per crossing, roll-off and Kaiser beta of resampy's kaiser_best
SINC_ZEROS, SINC_NT, SINC_ROLLOFF, SINC_BETA = 64, 512, 0.9475937167399596, 14.769656459379492


def ratio(sr_in, sr_out):
    """-> (up, down) = (sr_out, sr_in) / gcd; ValueError naming the ratio when max(up, down) > MAX_RATIO"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError("sample rates must be positive, got %d -> %d" % (sr_in, sr_out))
    g = gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError("resampling %d -> %d Hz is the ratio %d/%d: max(up, down) must be <= %d"
                         % (sr_in, sr_out, up, down, MAX_RATIO))
    return up, down


def design_filter(up, down):
    """resample_poly's default filter: firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up -> (h float64, half)"""
    up, down = int(up), int(down)
    mr = max(up, down)
    half = 10 * mr
    n = 2 * half + 1
    fc = 1.0 / mr
    h = fc * np.sinc(fc * (np.arange(n, dtype=np.float64) - half)) * np.kaiser(n, 5.0)
    h /= h.sum()
    return h * up, half


def out_length(n, up, down):
    """samples of the output of n input samples: ceil(n up / down) (exact Python integers)"""
    return -(-int(n) * int(up) // int(down))


def stream_emitted(n, up, down):
    """outputs whose taps are all final after n input samples: max(0, floor((n up - half - 1) / down) + 1)"""
    up, down = int(up), int(down)
    return max(0, (int(n) * up - 10 * max(up, down) - 1) // down + 1)


def _plan(lib, up, down):
    from . import _lib
    v = [ctypes.c_int32() for _ in range(4)]
    _lib.check(lib.mi355asr_resample_plan(up, down, *[ctypes.byref(c) for c in v]))
    return dict(zip(("taps", "stride", "tile", "table_floats"), (c.value for c in v)))


def _phase_table(up, down, plan):
    """table[p * stride + m] = float32(h[p + m up]), zero past the filter's end"""
    h, _ = design_filter(up, down)
    K, Ks = plan["taps"], plan["stride"]
    full = np.zeros(K * up, np.float64)
    full[:len(h)] = h
    tab = np.zeros(plan["table_floats"], np.float32)
    tab[:up * Ks].reshape(up, Ks)[:, :K] = full.reshape(K, up).T.astype(np.float32)
    return tab


class _Base:
    def __init__(self, sr_in, sr_out, device):
        import torch
        from . import _lib
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = ratio(sr_in, sr_out)
        self.lib = _lib.lib()
        self.device = torch.device(device)
        self.plan = _plan(self.lib, self.up, self.down)
        self.taps, self.tile = self.plan["taps"], self.plan["tile"]
        self.table = torch.from_numpy(_phase_table(self.up, self.down, self.plan)).to(self.device)

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class Resampler(_Base):
    """One launch per call for a ragged batch; `tile` is the kernel's output tile, `taps` its K = ceil(n / up)."""

    def __init__(self, sr_in, sr_out, device="cuda:0"):
        super().__init__(sr_in, sr_out, device)

    def __call__(self, x, lengths=None, out_pad=None):
        """x [L] or [B, L], float32 or int16, NumPy or tensor; lengths [B] samples per row (None: L each) -> (y [B, Omax] float32
        on the device, out_len int32 [B] on the device).  Row b holds ceil(lengths[b] up / down) samples, computed as if alone,
        and zeros after them; Omax = out_length(L), or `out_pad` columns when given (wider: zeros; narrower: cut)."""
        import torch
        from . import _lib
        if isinstance(x, np.ndarray):
            if x.dtype != np.int16:
                x = np.asarray(x, np.float32)
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, np.float32))
        if x.dtype != torch.int16:
            x = x.to(torch.float32)
        if x.dim() == 1:
            x = x.reshape(1, -1)
        if x.dim() != 2:
            raise ValueError("expected a waveform [L] or [B, L], got %s" % (tuple(x.shape),))
        B, L = int(x.shape[0]), int(x.shape[1])
        if B < 1:
            raise ValueError("an empty batch")
        if lengths is None:
            ln = torch.full((B,), L, dtype=torch.int32, device=self.device)
        else:
            ln = lengths if torch.is_tensor(lengths) else torch.as_tensor(np.asarray(lengths))
            ln = ln.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            if ln.numel() != B:
                raise ValueError("%d rows, %d lengths" % (B, ln.numel()))
        O = max(1, out_length(L, self.up, self.down) if out_pad is None else int(out_pad))
        if L == 0:
            x = torch.zeros((B, 1), dtype=x.dtype)
            ln = torch.zeros_like(ln)
        x = x.to(self.device).contiguous()
        Lp = int(x.shape[1])
        y = torch.empty((B, O), dtype=torch.float32, device=self.device)
        out_len = torch.div(ln.clamp(0, Lp).to(torch.int64) * self.up + (self.down - 1), self.down, rounding_mode="floor")
        out_len = out_len.clamp(max=O).to(torch.int32)
        if self.up == self.down:                      # a copy, or the int16 conversion
            xf = x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x
            w = min(O, Lp)
            y.zero_()
            y[:, :w] = xf[:, :w] * (torch.arange(w, device=self.device)[None, :] < out_len[:, None])
            return y, out_len
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mi355asr_resample(_ptr(x), 4 if x.dtype == torch.int16 else 0, _ptr(ln), B, Lp, self.up, self.down,
                                                  _ptr(self.table), _ptr(y), O, self._stream()))
        self._keep = (x, ln)                          # inputs of an asynchronous call
        return y, out_len


class StreamResampler(_Base):
    """`n_streams` independent live streams, advanced together: one launch per `step` / `flush` whatever the number of slots.
    Positions are Python integers on the host, so a step knows its output counts without asking the device; a slot's
    concatenated outputs equal `Resampler` on its concatenated input bit for bit."""

    def __init__(self, n_streams, sr_in, sr_out, max_packet, device="cuda:0"):
        import torch
        from . import _lib
        super().__init__(sr_in, sr_out, device)
        self.n_streams, self.max_packet = int(n_streams), int(max_packet)
        if self.n_streams < 1 or self.max_packet < 1:
            raise ValueError("n_streams and max_packet must be >= 1")
        self.pos = [0] * self.n_streams
        self.identity = self.up == self.down
        if self.identity:
            return
        sb, wb, oc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
        _lib.check(self.lib.mi355asr_resample_streams_bytes(self.up, self.down, self.n_streams, self.max_packet, ctypes.byref(sb),
                                                            ctypes.byref(wb), ctypes.byref(oc)))
        self.out_cap = oc.value
        self.state = torch.empty(sb.value, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(wb.value, dtype=torch.uint8, device=self.device)
        self.reset()

    def _check(self, slots):
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("a slot is named twice in one step: %s" % (sorted(slots),))
        for s in slots:
            if not 0 <= s < self.n_streams:
                raise ValueError("slot %d out of range 0 .. %d" % (s, self.n_streams - 1))
        return slots

    def reset(self, slots=None):
        """the given slots (None: all) become fresh streams at position 0"""
        from . import _lib
        tab = None if slots is None else self._check(slots)
        for s in (range(self.n_streams) if tab is None else tab):
            self.pos[s] = 0
        if self.identity or (tab is not None and not tab):
            return
        arr = None if tab is None else np.ascontiguousarray(tab, np.int32)
        import torch
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mi355asr_resample_streams_reset(_ptr(self.state), self.up, self.down, self.n_streams, self.max_packet,
                                                                arr.ctypes.data_as(ctypes.c_void_p) if arr is not None else None,
                                                                0 if arr is None else len(arr), self._stream()))

    def _launch(self, slots, lens, x, flush):
        import torch
        from . import _lib
        n = len(slots)
        tab = np.ascontiguousarray(slots, np.int32)
        pos = np.ascontiguousarray([self.pos[s] for s in slots], np.int64)
        nin = np.ascontiguousarray(lens, np.int32)
        n_out = np.zeros(n, np.int32)
        y = torch.zeros((n, self.out_cap), dtype=torch.float32, device=self.device)      # (a step writes n_out[i] samples of row i)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mi355asr_resample_streams_step(
                _ptr(self.state), self.up, self.down, self.n_streams, self.max_packet, _ptr(self.table),
                tab.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p), nin.ctypes.data_as(ctypes.c_void_p), n,
                int(flush), _ptr(x) if x is not None else None, 0 if x is None else int(x.shape[1]), _ptr(y), self.out_cap,
                n_out.ctypes.data_as(ctypes.c_void_p), _ptr(self.ws), self.ws.numel(), self._stream()))
        return y, n_out

    def step_device(self, slots, packets, lengths=None):
        """-> (y [n, out_cap] float32 on the device, counts int32 [n] on the host); row i holds slot slots[i]'s counts[i] new
        samples, zeros behind them.  packets: one 1-D array or tensor per slot, or one float32 tensor [n, P] on the device with `lengths` samples
        per row (None: P each), which is used as it is.  Nothing is waited for."""
        import torch
        slots = self._check(slots)
        if len(packets) != len(slots) or not slots:
            raise ValueError("%d slots, %d packets" % (len(slots), len(packets)))
        if torch.is_tensor(packets) and packets.dim() == 2:
            x = packets.to(device=self.device, dtype=torch.float32).contiguous()
            lens = [int(x.shape[1])] * len(slots) if lengths is None else [int(v) for v in lengths]
            if len(lens) != len(slots) or any(not 0 <= v <= x.shape[1] for v in lens):
                raise ValueError("lengths: one per slot, each within the packet tensor's %d columns" % x.shape[1])
            rows = None
        else:
            rows = [p if torch.is_tensor(p) else np.asarray(p, np.float32).reshape(-1) for p in packets]
            lens = [int(r.numel() if torch.is_tensor(r) else len(r)) for r in rows]
        for s, ln in zip(slots, lens):
            if ln > self.max_packet:
                raise ValueError("slot %d: a packet of %d samples is above max_packet = %d" % (s, ln, self.max_packet))
        P = max(1, max(lens))
        if rows is None:
            pass
        elif all(torch.is_tensor(r) for r in rows):
            x = torch.zeros((len(rows), P), dtype=torch.float32, device=self.device)
            for i, r in enumerate(rows):
                x[i, :lens[i]] = r.reshape(-1).to(device=self.device, dtype=torch.float32)
        else:
            xh = np.zeros((len(rows), P), np.float32)
            for i, r in enumerate(rows):
                xh[i, :lens[i]] = r.cpu().numpy().reshape(-1) if torch.is_tensor(r) else r
            x = torch.from_numpy(xh).to(self.device)
        if self.identity:
            for s, ln in zip(slots, lens):
                self.pos[s] += ln
            return x, np.asarray(lens, np.int32)
        y, n_out = self._launch(slots, lens, x, False)
        for s, ln in zip(slots, lens):
            self.pos[s] += ln
        self._keep = x
        return y, n_out

    def step(self, slots, packets):
        """one launch for all named slots -> {slot: float32 NumPy array of the samples that became final}"""
        slots = [int(s) for s in slots]
        y, n_out = self.step_device(slots, packets)
        yh = y.cpu().numpy()
        return {s: yh[i, :n_out[i]].copy() for i, s in enumerate(slots)}

    def flush(self, slots):
        """-> {slot: the rest of its output up to out_length(samples taken), zero-extended}; the slots are reset"""
        slots = self._check(slots)
        if not slots:
            return {}
        if self.identity:
            out = {s: np.zeros(0, np.float32) for s in slots}
        else:
            y, n_out = self._launch(slots, [0] * len(slots), None, True)
            yh = y.cpu().numpy()
            out = {s: yh[i, :n_out[i]].copy() for i, s in enumerate(slots)}
        self.reset(slots)
        return out


def sinc_table():
    """the right half of the interpolation filter in float64: 32 769 entries, win[0] = SINC_ROLLOFF"""
    n = SINC_NT * SINC_ZEROS
    return np.kaiser(2 * n + 1, SINC_BETA)[n:] * SINC_ROLLOFF * np.sinc(SINC_ROLLOFF * np.linspace(0, SINC_ZEROS, n + 1))


def sinc_out_length(n, r):
    """samples of the output of n input samples at ratio r: ceil(n r), the product in float64"""
    return int(np.ceil(float(int(n)) * float(r)))


def sinc_valid_length(n, r):
    """outputs that are computed: floor(n r); the rest of a longer output is zero (librosa's fix_length)"""
    return int(np.floor(float(int(n)) * float(r)))


def _sinc_plan(lib, ratio=1.0):
    v = [ctypes.c_int32() for _ in range(3)]
    lo, hi = ctypes.c_double(), ctypes.c_double()
    rc = lib.mi355asr_sinc_plan(float(ratio), *[ctypes.byref(c) for c in v], ctypes.byref(lo), ctypes.byref(hi))
    plan = dict(tile=v[0].value, wing=v[1].value, table_floats=v[2].value, ratio_min=lo.value, ratio_max=hi.value)
    if rc != 0:
        raise ValueError("the ratio %r is outside the supported %g .. %g" % (ratio, lo.value, hi.value))
    return plan


class SincResampler:
    """One launch per call for a ragged batch with a ratio per row; `tile` is the kernel's output tile, `ratio_min` and
    `ratio_max` the supported ratios (mi355asr_sinc_plan).  table_mode 1 reads the table through the caches instead of LDS
    (the same bits; for measurements)."""

    def __init__(self, device="cuda:0", table_mode=0):
        import torch
        from . import _lib
        self.lib = _lib.lib()
        self.device = torch.device(device)
        self.table_mode = int(table_mode)
        self.plan = _sinc_plan(self.lib)
        self.tile, self.ratio_min, self.ratio_max = self.plan["tile"], self.plan["ratio_min"], self.plan["ratio_max"]
        self._table = None

    def wing(self, ratio):
        """taps per wing at most at this ratio; ValueError naming the ratio and the bounds"""
        return _sinc_plan(self.lib, ratio)["wing"]

    def ratios(self, ratios, B):
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(ratios, np.float64).reshape(-1), (B,)))
        for b, v in enumerate(r):
            if not (np.isfinite(v) and self.ratio_min <= v <= self.ratio_max):
                raise ValueError("row %d: the ratio %r is outside the supported %g .. %g" % (b, float(v), self.ratio_min, self.ratio_max))
        return r

    def table(self):
        import torch
        if self._table is None:
            tab = np.empty(self.plan["table_floats"], np.float32)
            win = sinc_table().astype(np.float32)
            tab[:len(win)] = win
            tab[len(win):] = win[-1]
            self._table = torch.from_numpy(tab).to(self.device)
        return self._table

    def launch(self, x, lens, ratios, out_lens, offs, y):
        """the library call on prepared arguments: x, y float32 tensors on the device, the rest host arrays -> valid int64 [B]"""
        import torch
        from . import _lib
        B = int(x.shape[0])
        lens = np.ascontiguousarray(lens, np.int64)
        out_lens = np.ascontiguousarray(out_lens, np.int64)
        offs = None if offs is None else np.ascontiguousarray(offs, np.int64)
        valid = np.zeros(B, np.int64)
        wb = ctypes.c_size_t()
        _lib.check(self.lib.mi355asr_sinc_workspace_bytes(B, ctypes.byref(wb)))
        ws = torch.empty(wb.value // 8, dtype=torch.float64, device=self.device)
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mi355asr_sinc_resample(
                _ptr(x), B, int(x.shape[1]), hp(ratios), hp(lens), hp(out_lens), None if offs is None else hp(offs), hp(valid),
                _ptr(self.table()), self.table_mode, _ptr(y), int(y.shape[1]), _ptr(ws), wb.value,
                ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._keep = (x, ws)                          # inputs of an asynchronous call
        return valid

    def __call__(self, x, lengths=None, ratios=1.0, out_lengths=None, out_pad=None):
        """x [L] or [B, L] float32, NumPy or tensor; lengths [B] samples per row (None: L each); ratios: a number or [B], rate_out /
        rate_in per row; out_lengths [B] (None: ceil(lengths ratios)) -> (y [B, Omax] float32 on the device, out_len int32 [B] on
        the device).  Row b holds out_len[b] samples computed as if alone -- those from floor(lengths[b] ratios[b]) on are zero --
        and zeros after them; Omax = the longest out_len, or `out_pad` columns when given (wider: zeros; narrower: cut).  A ratio
        of 1 is a low-pass at SINC_ROLLOFF of Nyquist, not a copy."""
        import torch
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
        elif not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, np.float32))
        x = x.to(torch.float32)
        if x.dim() == 1:
            x = x.reshape(1, -1)
        if x.dim() != 2:
            raise ValueError("expected a waveform [L] or [B, L], got %s" % (tuple(x.shape),))
        B, L = int(x.shape[0]), int(x.shape[1])
        if B < 1:
            raise ValueError("an empty batch")
        if lengths is None:
            lens = np.full(B, L, np.int64)
        else:
            lens = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).reshape(-1).astype(np.int64)
            if len(lens) != B:
                raise ValueError("%d rows, %d lengths" % (B, len(lens)))
            if (lens < 0).any() or (lens > L).any():
                raise ValueError("lengths must lie within 0 .. %d, got %s" % (L, lens))
        r = self.ratios(ratios, B)
        if out_lengths is None:
            out = np.array([sinc_out_length(n, v) for n, v in zip(lens, r)], np.int64)
        else:
            out = np.asarray(out_lengths.cpu() if torch.is_tensor(out_lengths) else out_lengths).reshape(-1).astype(np.int64)
            if len(out) != B or (out < 0).any():
                raise ValueError("out_lengths: one per row and none negative, got %s" % (out,))
        O = max(1, int(out.max()) if out_pad is None else int(out_pad))
        out = np.minimum(out, O)
        if L == 0:
            x = torch.zeros((B, 1), dtype=torch.float32)
        x = x.to(self.device).contiguous()
        y = torch.empty((B, O), dtype=torch.float32, device=self.device)
        self.launch(x, lens, r, out, None, y)
        return y, torch.from_numpy(out.astype(np.int32)).to(self.device)
