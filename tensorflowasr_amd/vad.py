"""Voice-activity detection: the reference's trained `vad.onnx` on the MI355X (vad.hip) and the two segmentation rules
the reference's inference sessions put on top of it.

    vad = VAD(); vad.load_onnx('vad.onnx')
    scores = vad.scores(wav_16k)                       # [B, T] fp32, one per 10 ms frame, one fused HIP launch
    ov = OfflineVAD(sr=16000); ov.compile(vad); ov.vad(wav_16k)   # [[start_s, end_s], ...]

    vad = VAD().load_saved_model('vad/online_vad_model')          # the online model: scores + voice-mask head
    enhanced_8k, scores = vad.enhance(wav_16k)                    # [B, T*80] denoised 8 kHz audio, [B, T]

- `VAD`          Inference/PythonInference/vad/src/vad.py: `inference(frames [B, T, 80]) -> [B, T, 1]`; with the
                 SavedModel's weights also the model's second output, `enhance` (tensorflowasr_amd/enhance.py streams it).
- `OfflineVAD`   offline_asr_session.py OfflineVAD (vad / parse / final_parse / recover), restated with its quirks.
- `OnlineVAD`, `OnlineVADBatch`   vad/online_vad.py OnlineVAD (8 kHz, 20 ms packets), restated with its quirks; the
                 batch form advances many streams with one launch per 100 ms tick.
- `vad_gate`, `VADGate`   CppInference asr_session.cpp Session::VadInference / Session::Parase.
"""
import numpy as np
import torch

from . import _lib
from .models import _Handle, _p

FRAME = 80
# ABI weight name -> (tf2onnx initialiser name, transpose applied to it)
ONNX_NAMES = {
    "dense/kernel": "StatefulPartitionedCall/dense/Tensordot/ReadVariableOp:0",
    "dense/bias": "StatefulPartitionedCall/dense/BiasAdd/ReadVariableOp:0",
    "dense_1/kernel": "StatefulPartitionedCall/dense_1/Tensordot/ReadVariableOp:0",
    "dense_1/bias": "StatefulPartitionedCall/dense_1/BiasAdd/ReadVariableOp:0",
    "conv1d/kernel": "StatefulPartitionedCall/conv1d/conv1d/ExpandDims_1:0",
    "conv1d/bias": "const_fold_opt__154",
    "dense_2/kernel": "StatefulPartitionedCall/dense_2/Tensordot/ReadVariableOp:0",
    "dense_2/bias": "StatefulPartitionedCall/dense_2/BiasAdd/ReadVariableOp:0",
    "layer_normalization/gamma": "StatefulPartitionedCall/layer_normalization/mul_3/ReadVariableOp:0",
    "layer_normalization/beta": "StatefulPartitionedCall/layer_normalization/add/ReadVariableOp:0",
    "conv1d_1/kernel": "StatefulPartitionedCall/conv1d_1/conv1d/ExpandDims_1:0",
    "conv1d_1/bias": "const_fold_opt__153",
    "dense_3/kernel": "StatefulPartitionedCall/dense_3/Tensordot/ReadVariableOp:0",
    "dense_3/bias": "StatefulPartitionedCall/dense_3/BiasAdd/ReadVariableOp:0",
    "dense_4/kernel": "StatefulPartitionedCall/dense_4/Tensordot/ReadVariableOp:0",
    "dense_4/bias": "StatefulPartitionedCall/dense_4/BiasAdd/ReadVariableOp:0",
}


MASK_NAMES = ("audio_voice_mask/kernel", "audio_voice_mask/bias")
SAVED_MODEL_PREFIX = "online_cnn_vad/"


def weights_from_saved_model_variables(variables):
    """{Keras variable name: array} of vad/online_vad_model (tfbundle.Bundle.variables_by_name) -> ABI weights.
    `online_cnn_vad/<layer>/<kernel|bias|gamma|beta>:0` -> `<layer>/<...>`; Keras' conv kernels are already
    [5, in, out] and its dense kernels [in, out], so nothing is transposed."""
    w = {}
    for name, a in variables.items():
        if not name.startswith(SAVED_MODEL_PREFIX):
            raise ValueError("unexpected variable %r in the online VAD model" % name)
        abi = name[len(SAVED_MODEL_PREFIX):].split(":")[0]
        if abi not in ONNX_NAMES and abi not in MASK_NAMES:
            raise ValueError("unexpected variable %r in the online VAD model" % name)
        w[abi] = np.ascontiguousarray(np.asarray(a, np.float32))
    missing = sorted((set(ONNX_NAMES) | set(MASK_NAMES)) - set(w))
    if missing:
        raise ValueError("online VAD model lacks %s" % missing)
    return w


def weights_from_onnx_inits(inits):
    """tf2onnx initialisers -> ABI weights: conv kernels [out, in, 1, 5] -> [5, in, out], biases [1, 80, 1] -> [80]."""
    w = {}
    for abi, g in ONNX_NAMES.items():
        a = np.asarray(inits[g], np.float32)
        if abi.startswith("conv1d") and abi.endswith("kernel"):
            a = a[:, :, 0, :].transpose(2, 1, 0)
        elif abi.endswith("bias"):
            a = a.reshape(-1)
        w[abi] = np.ascontiguousarray(a)
    return w


class VAD:
    """The reference's VAD (vad/src/vad.py) on libmi355asr.so.  `config` is accepted for the reference's signature
    (its running / model settings do not change the graph); `weights` is a dict or .npz of ABI-named tensors."""

    def __init__(self, config=None, weights=None, device="cuda:0"):
        self.config = config
        self.device = torch.device(device)
        self._h = {}
        if weights is not None:
            self.load_weights(weights)

    def load_onnx(self, path):
        from .checkpoint import read_onnx
        _, inits = read_onnx(path)
        self.load_weights(weights_from_onnx_inits(inits))
        return self

    def load_saved_model(self, path):
        """the reference's vad/online_vad_model (a SavedModel directory, or its variables/ prefix): the 16 weights of
        vad.onnx plus the voice-mask head that `enhance` runs.  Only the variables are read (tfbundle); the graph in
        saved_model.pb is what include/mi355asr.h restates."""
        from . import tfbundle
        b = tfbundle.Bundle(tfbundle.checkpoint_prefix(path))
        self.load_weights(weights_from_saved_model_variables(b.variables_by_name()))
        return self

    @property
    def has_mask(self):
        return hasattr(self, "weights") and all(n in self.weights for n in MASK_NAMES)

    def load_weights(self, weights):
        if isinstance(weights, str):
            with np.load(weights) as z:
                weights = {k: z[k] for k in z.files}
        self.weights = {k: np.asarray(v, np.float32) for k, v in weights.items()}
        self._h = {}
        return self

    def _handle(self, decimate):
        h = self._h.get(decimate)
        if h is None:
            if not hasattr(self, "weights"):
                raise _lib.Mi355AsrError("VAD: no weights loaded (load_onnx / load_weights)")
            # weights with the voice-mask head get an enhancer handle: its scores are the scores-only handle's
            create = _lib.lib().mi355asr_vad_enhancer_create if self.has_mask else None
            h = _Handle(_lib.VadConfig(dmodel=FRAME, frame=FRAME, decimate=decimate), self.device, create=create)
            h.load(self.weights)
            h.finalize()
            self._h[decimate] = h
        return h

    def _run(self, x, lengths, decimate):
        h = self._handle(decimate)
        x = h.to_device(x)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError("expected a waveform [L] or [B, L], got %s" % (tuple(x.shape),))
        B, L = x.shape
        T = L // (FRAME * decimate)
        out = torch.zeros((B, T), dtype=torch.float32, device=h.device)
        ln = None if lengths is None else h.to_device(np.asarray(lengths), dtype=torch.int32)
        if B and T:
            with torch.cuda.device(h.device):
                _lib.check(h.lib.mi355asr_vad_forward(h.ptr, _p(x), B, L, _p(ln), _p(out), h._stream()))
        return out

    def enhance(self, wav, lengths=None, sample_rate=16000):
        """the online model's two outputs in one launch: waveform [L] or [B, L] at `sample_rate` (16000: decimated by
        2 in the kernel; 8000: read as it is), `lengths` samples per row -> (enhanced [B, T*80], scores [B, T]).
        `enhanced` is 8 kHz audio whatever the input rate: frame t is the network's input frame (wav[::2] at 16 kHz)
        times the voice mask.  Entries past a row's frame count stay 0.  Needs the mask head (load_saved_model)."""
        if not self.has_mask:
            raise _lib.Mi355AsrError("VAD.enhance: the loaded weights have no voice-mask head (%s); load the online "
                                     "model with load_saved_model -- vad.onnx carries the score head only"
                                     % ", ".join(MASK_NAMES))
        if sample_rate not in (8000, 16000):
            raise ValueError("sample_rate must be 8000 or 16000, got %r" % (sample_rate,))
        decimate = sample_rate // 8000
        h = self._handle(decimate)
        x = h.to_device(wav)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2:
            raise ValueError("expected a waveform [L] or [B, L], got %s" % (tuple(x.shape),))
        B, L = x.shape
        T = L // (FRAME * decimate)
        scores = torch.zeros((B, T), dtype=torch.float32, device=h.device)
        enhanced = torch.zeros((B, T * FRAME), dtype=torch.float32, device=h.device)
        ln = None if lengths is None else h.to_device(np.asarray(lengths), dtype=torch.int32)
        if B and T:
            with torch.cuda.device(h.device):
                _lib.check(h.lib.mi355asr_vad_enhance(h.ptr, _p(x), B, L, _p(ln), _p(scores), _p(enhanced), h._stream()))
        return enhanced, scores

    def scores(self, wav, lengths=None):
        """16 kHz waveform [L] or [B, L] (`lengths`: samples per row) -> scores [B, T], T = L // 160, decimated by 2
        inside the kernel.  Entries past a row's frame count stay 0."""
        return self._run(wav, lengths, 2)

    def inference(self, wav):
        """vad.py VAD.inference: frames [B, T, 80] of 8 kHz samples -> [B, T, 1] (numpy, as onnxruntime returns)."""
        x = np.asarray(wav, np.float32) if not torch.is_tensor(wav) else wav
        B, T, C = x.shape
        if C != FRAME:
            raise ValueError("expected [B, T, 80] frames, got %s" % (tuple(x.shape),))
        return self._run(x.reshape(B, T * FRAME), None, 1).cpu().numpy().reshape(B, T, 1)


# ---- offline segmentation (offline_asr_session.py OfflineVAD) -------------------------------------------------------
class OfflineVAD:
    """offline_asr_session.py OfflineVAD, restated with the reference's behaviour, quirks included:

    - a frame is speech when its score is >= 0.0; the state machine steps in blocks of 10 frames (0.1 s);
    - a start is declared when >= 5 of the newest 10 frames of a 20-frame record are speech, at `wav_length - 0.2`;
    - the end rule (three silent windows -> `wav_length - 3*0.1 + 0.1`) is coded in the reference but cannot fire:
      `parse` only fills `sil_record` while `sound_pick` is set, and nothing sets it.  Once speech starts it runs to
      the end of the recording, where `final_parse` closes it at `wav_length - 0.1` if the 16 kHz buffer holds more
      than 8000 * 0.2 samples.  So `vad` returns no segment or one, and `recover` (merging gaps under 0.1 s,
      splitting spans over 15 s) only runs on lists of two or more -- never from `vad`;
    - boundaries are rounded to 3 decimals.

    One reference quirk is not reproduced: the reference reshapes `wav[::2]` to [1, -1, 80] and so raises unless the
    length is a multiple of 160; here T = L // 160 and the tail is ignored."""

    def __init__(self, min_duration=0.5, sr=8000, recover_thread=0.1, recover_max_duration=15.):
        self.min_duration = min_duration
        self.sample_rate = sr
        self.recover_thread = recover_thread
        self.recover_max_duration = recover_max_duration
        self.sd = None

    def compile(self, sd):
        self.sd = sd

    def vad(self, wav):
        wav = np.asarray(wav, np.float32).reshape(-1)
        s = self.sd.scores(wav).cpu().numpy().reshape(-1)
        return self.segments_from_scores(s, len(wav), self.sample_rate)

    def segments_from_scores(self, scores_1d, wav_len, sample_rate=None):
        """[[start, end], ...] seconds from per-frame scores of a recording of `wav_len` samples (16 kHz buffer)."""
        preds = [1 if v >= 0.0 else 0 for v in np.asarray(scores_1d, np.float32).reshape(-1).tolist()]
        segs = self.parse(preds, wav_len)
        out = [[round(a, 3), round(b, 3)] for a, b in segs]
        if len(out) >= 2:
            out = self.recover(out)
        return out

    def parse(self, vad_preds, wav_len):
        """parse + final_parse: the reference's state machine over 0.1 s blocks -> [(start, end)]"""
        result, live = [], [0.0, 0.0]
        sound_record, sil_record = [], []
        sound_pick = sound_start = sil_times = 0
        data_len = 0
        wav_length = 0
        n = len(vad_preds)
        for i in range(n // 10 + 1):
            s, e = i * 10, i * 10 + 10
            data_len += max(0, min(e * 160, wav_len) - min(s * 160, wav_len))
            pred = vad_preds[s:e]
            if sound_pick:
                sil_record += pred
            else:
                sound_record += pred
            if sound_start:
                if len(sil_record) >= 20:
                    last = sum(sil_record[-10:])
                    if last <= 8 and sil_times == 0:
                        sil_times += 1
                    elif last <= 5 and sil_times >= 1:
                        sil_times += 1
                    else:
                        sil_times = 0
                    sil_record = sil_record[-10:]
                if sil_times == 3:
                    live[1] = wav_length - 3 * 0.1 + 0.1
                    result.append(tuple(live))
                    sil_record, sound_start, sil_times = [], 0, 0
            else:
                if len(sound_record) == 20:
                    if sum(sound_record[-10:]) >= 5.:
                        sound_start = 1
                        sound_record = []
                        live[0] = wav_length - 0.2
                    else:
                        sound_record = sound_record[-10:]
            wav_length += 0.1
        if data_len > int(8000 * 0.2) and sound_start:
            live[1] = wav_length - 0.1
            result.append(tuple(live))
        return result

    def recover(self, results):
        new_results = []
        s, e = results[0]
        for i in range(1, len(results)):
            now = results[i]
            if now[0] - e < self.recover_thread and now[1] - s < self.recover_max_duration:
                e = now[1]
                if i == len(results) - 1:
                    new_results.append([s, e])
            else:
                new_results.append([s, e])
                s, e = now[0], now[1]
                if i == len(results) - 1:
                    new_results.append([s, e])
        out = []
        for s, e in new_results:
            d = e - s
            if d > self.recover_max_duration:
                parts = d // self.recover_max_duration
                if d % self.recover_max_duration != 0:
                    num = d / (parts + 1)
                    parts += 1
                else:
                    num = d / parts
                num = int(num)
                s_ = s
                for i in range(int(parts)):
                    e_ = s_ + num if i != parts - 1 else e
                    out.append([s_, e_])
                    s_ = e_
            else:
                out.append([s, e])
        return out


def segments_from_scores(scores_1d, wav_len, sample_rate=16000):
    """OfflineVAD segmentation of per-frame scores; host only (no GPU)."""
    return OfflineVAD(sr=sample_rate).segments_from_scores(scores_1d, wav_len, sample_rate)


# ---- online segmentation (vad/online_vad.py OnlineVAD) ---------------------------------------------------------------
class OnlineVAD:
    """vad/online_vad.py OnlineVAD: a streaming state machine over 8 kHz int16 packets, restated with the reference's
    behaviour, quirks included:

    - `wav_length` accumulates `len(packet) / 8000` as a Python float (so 20 ms packets drift off multiples of 0.02);
      the VAD runs when `wav_length - vad_point >= 0.1`, on the last 800 samples of a 2 400-sample `voice_data`
      buffer that starts as zeros (float64: the hstack of float64 zeros and the float32 packet), cast to float32;
    - of the 10 scores a run returns, a frame is speech when its score is >= 0.0;
    - start: when the `sound_record` of predictions reaches exactly 20, >= 5 speech frames among its newest 10 declare
      a start at `wav_length - 0.2` (`parse` returns 0, `start_event` = 1); otherwise the record keeps its newest 10;
      the buffered `chunk` restarts from the last 1 600 samples of `voice_data`;
    - end: once speech started, every packet with >= 20 entries in `sil_record` steps `sil_times` (<= 8 speech frames
      of the newest 10 and sil_times == 0 -> 1, also setting end_time = wav_length; <= 5 and == 1 -> 2; <= 2 and
      >= 2 -> +1; otherwise back to 0) and trims the record to 10.  At sil_times == max_sil_wait `parse` returns 1 with
      end_time = `wav_length - max_sil_wait + 0.1`: max_sil_wait is subtracted as seconds, not as 0.1 s steps;
    - `start_event` / `end_event` are set and never cleared; `parse` returns None when nothing happens;
    - `final_parse`: 0 if fewer than 800 samples were buffered since the start, 1 (end_time = wav_length) if more than
      800 and speech is open, None otherwise (exactly 800, or no open speech).

    `scorer(window_800 float32) -> 10 scores` defaults to `vad.inference` on it (decimate 1)."""

    def __init__(self, vad=None, max_sil_wait=3, sr=8000, scorer=None):
        self.scorer = scorer or (lambda x: vad.inference(x.reshape(1, -1, FRAME)).reshape(-1))
        self.max_sil_wait = max_sil_wait
        self.sr = sr
        self.init_params()

    def init_params(self):
        self.chunk = np.array([], "float32")
        self.wav_length = 0
        self.live_result = {"start_time": 0., "end_time": 0., "live_text": "", "decoded_result": []}
        self.vad_point = 0
        self.voice_data = np.zeros(2400)
        self.inter_break = 0
        self.start_event = 0
        self.end_event = 0
        self.send_flag = 0
        self.sil_record = []
        self.sil_times = 0
        self.sound_record = []
        self.sound_start = 0
        self.sound_end = 0

    def window(self):
        """the float32 [800] the VAD scores now"""
        return np.array(self.voice_data[-800:], "float32")

    @staticmethod
    def predictions(scores):
        return np.where(np.asarray(scores).reshape(-1) >= 0., 1, 0).tolist()[-10:]

    def ingest(self, new_data):
        """the part of parse before the VAD call -> whether this packet runs the VAD"""
        new_data = np.array(np.frombuffer(new_data, "int16"), "float32")
        new_data /= 32768
        self.wav_length += len(new_data) / 8000
        if self.sound_start:
            self.chunk = np.concatenate([self.chunk, new_data], 0)
        self.voice_data = np.hstack((self.voice_data, new_data))[-2400:]
        return self.wav_length - self.vad_point >= 0.1

    def advance(self, scores=None):
        """the rest of parse, given the window's scores when `ingest` asked for them"""
        if scores is not None:
            pred = self.predictions(scores)
            if self.sound_start:
                self.sil_record += pred
            else:
                self.sound_record += pred
            self.vad_point = self.wav_length
        if self.sound_start:
            if len(self.sil_record) >= 20:
                last = np.sum(self.sil_record[-10:])
                if last <= 8 and self.sil_times == 0:
                    self.sil_times += 1
                    self.inter_break = 1
                    self.live_result["end_time"] = self.wav_length
                elif last <= 5 and self.sil_times == 1:
                    self.sil_times += 1
                elif last <= 2 and self.sil_times >= 2:
                    self.sil_times += 1
                else:
                    self.sil_times = 0
                self.sil_record = self.sil_record[-10:]
            if self.sil_times == self.max_sil_wait:
                self.sound_end = 1
                self.end_event = 1
                self.live_result["end_time"] = self.wav_length - self.max_sil_wait + 0.1
                self.sil_record = []
                self.sound_start = 0
                self.sil_times = 0
                self.inter_break = 0
                return 1
        else:
            if len(self.sound_record) == 20:
                if np.sum(self.sound_record[-10:]) >= 5.:
                    self.sound_start = 1
                    self.start_event = 1
                    self.sound_record = []
                    self.chunk = self.voice_data[-1600:]
                    self.live_result["start_time"] = self.wav_length - 0.2
                    return 0
                self.sound_record = self.sound_record[-10:]
        return None

    def parse(self, new_data):
        """one int16 packet (bytes) -> 0 (speech started), 1 (speech ended) or None"""
        need = self.ingest(new_data)
        return self.advance(self.scorer(self.window()) if need else None)

    def final_parse(self):
        if len(self.chunk) < 800:
            return 0
        elif len(self.chunk) > 800 and self.sound_start:
            self.send_flag = 1
            self.sound_end = 1
            self.live_result["end_time"] = self.wav_length
            return 1
        return None


class OnlineVADBatch:
    """N independent `OnlineVAD` streams advanced together: `parse(packets)` takes one packet (bytes, or None for no
    packet) per stream and scores every window due this tick with one `vad_forward` of [M, 800] at 8 kHz."""

    def __init__(self, vad, n, max_sil_wait=3, sr=8000):
        self.vad = vad
        self.streams = [OnlineVAD(max_sil_wait=max_sil_wait, sr=sr, scorer=self._unbatched) for _ in range(n)]

    @staticmethod
    def _unbatched(x):
        raise RuntimeError("OnlineVADBatch scores windows in parse")

    def __getitem__(self, i):
        return self.streams[i]

    def __len__(self):
        return len(self.streams)

    def parse(self, packets):
        due = [i for i, (st, p) in enumerate(zip(self.streams, packets)) if p is not None and st.ingest(p)]
        scores = {}
        if due:
            win = np.stack([self.streams[i].window() for i in due])
            s = self.vad.inference(win.reshape(len(due), -1, FRAME)).reshape(len(due), -1)
            scores = dict(zip(due, s))
        return [None if p is None else st.advance(scores.get(i)) for i, (st, p) in enumerate(zip(self.streams, packets))]

    def final_parse(self):
        return [st.final_parse() for st in self.streams]


# ---- streaming gate (CppInference asr_session.cpp) ------------------------------------------------------------------
def vad_gate(scores_last_10):
    """Session::VadInference's rule: more than 5 of the last 10 scores are > -0.1 (fewer than 10 frames: False)."""
    s = np.asarray(scores_last_10, np.float32).reshape(-1)
    if len(s) < 10:
        return False
    return int(np.sum(s[-10:] > -0.1)) > 5


class VADGate:
    """Session::Parase: a 3 200-sample ring of 16 kHz audio, the VAD every 0.1 s of pushed audio, start when the gate
    opens (at wavLength - 0.2 s), end after 5 consecutive closed gates (at wavLength - 0.2 s).  `push` returns 0, 1
    (speech started) or 2 (speech ended) like Parase; times are float32 like the C++ members.  `scorer(buffer_8k)` gives
    the scores of the decimated buffer's frames (default: `vad.inference` on it)."""

    def __init__(self, vad=None, sample_rate=16000, scorer=None):
        self.samplerate = np.float32(sample_rate)
        self.scorer = scorer or (lambda x: vad.inference(x[None, :len(x) // FRAME * FRAME].reshape(1, -1, FRAME)).reshape(-1))
        self.reset()

    def reset(self):
        self.wavLength = np.float32(0)
        self.vad_point = np.float32(0)
        self.sil_times = 0
        self.sound_start = 0
        self.vad_result = False
        self.buffer = np.zeros(0, np.float32)
        self.voice_start_times = np.float32(0)
        self.voice_end_times = np.float32(0)

    def push(self, wav):
        x = np.asarray(wav, np.float32).reshape(-1)
        self.wavLength = np.float32(self.wavLength + np.float32(np.float32(len(x)) / self.samplerate))
        self.buffer = np.concatenate([self.buffer, x])[-3200:]
        if float(np.float32(self.wavLength - self.vad_point)) >= 0.1:
            need = self.buffer[::2]
            out = self.scorer(need) if len(need) >= FRAME else np.zeros(0, np.float32)
            self.vad_result = vad_gate(out)
            self.vad_point = self.wavLength
        if not self.sound_start:
            if self.vad_result:
                self.sound_start = 1
                self.voice_start_times = np.float32(float(self.wavLength) - 0.2)
                return 1
            return 0
        self.sil_times = self.sil_times + 1 if not self.vad_result else 0
        if self.sil_times == 5:
            self.voice_end_times = np.float32(float(self.wavLength) - 0.2)
            self.sound_start = 0
            self.sil_times = 0
            return 2
        return 0
