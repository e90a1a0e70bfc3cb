"""Streaming speech enhancement with the online VAD's voice-mask head (vad.hip, mi355asr_vad_enhance).

    vad = VAD().load_saved_model('vad/online_vad_model')
    se = StreamingEnhancer(vad, n_streams=4, sample_rate=16000)
    for chunks in ...:                              # one array (any length, possibly empty) per stream
        out = se.push(chunks)                       # [(enhanced_8k [k*80], scores [k])] per stream, one launch

A frame's outputs depend on itself and the 8 frames before it (two causal 5-tap convolutions), and the network
zero-pads its activations -- not its input -- before the first frame.  So each stream keeps the last 8 input frames it
has seen and prepends them to its next chunk; the outputs of those frames are recomputed and dropped.  A stream that
has seen fewer than 8 frames prepends all of them, so its window still starts at the stream's first sample.  Every
output frame is therefore computed from exactly the input it has offline, and with the same instruction sequence
(each row of a tile runs the same MFMA chain wherever it sits), so the concatenated output equals
`vad.enhance(whole recording)` bit for bit.  Samples short of a whole frame wait for the next push."""
import numpy as np

from .vad import FRAME

HALO = 8      # frames of left context (vad.hip kHalo)


class StreamingEnhancer:
    def __init__(self, vad, n_streams, sample_rate=16000):
        if sample_rate not in (8000, 16000):
            raise ValueError("sample_rate must be 8000 or 16000, got %r" % (sample_rate,))
        if not vad.has_mask:
            raise ValueError("StreamingEnhancer needs the voice-mask head: load the online model with load_saved_model")
        self.vad = vad
        self.sample_rate = sample_rate
        self.step = FRAME * (sample_rate // 8000)         # input samples per frame
        self.n = n_streams
        self.reset()

    def reset(self):
        # per stream: the input samples not yet emitted as output (up to HALO frames of context, then a partial frame)
        self.keep = [np.zeros(0, np.float32) for _ in range(self.n)]
        self.ctx = [0] * self.n                         # whole frames at the head of keep[i] already emitted

    def push(self, chunks):
        """one chunk of input samples per stream -> [(enhanced 8 kHz [k * 80], scores [k])] per stream, where k is
        the number of whole frames the stream completed; one launch for all streams (none if no stream completes a
        frame)"""
        if len(chunks) != self.n:
            raise ValueError("expected %d chunks, got %d" % (self.n, len(chunks)))
        rows = [np.concatenate([k, np.asarray(c, np.float32).reshape(-1)]) for k, c in zip(self.keep, chunks)]
        lens = [len(r) for r in rows]
        frames = [n // self.step for n in lens]
        out = [(np.zeros(0, np.float32), np.zeros(0, np.float32)) for _ in range(self.n)]
        if any(f > c for f, c in zip(frames, self.ctx)):
            L = max(lens)
            x = np.zeros((self.n, L), np.float32)
            for i, r in enumerate(rows):
                x[i, :len(r)] = r
            enh, sc = self.vad.enhance(x, lengths=lens, sample_rate=self.sample_rate)
            enh, sc = enh.cpu().numpy(), sc.cpu().numpy()
            for i in range(self.n):
                c, f = self.ctx[i], frames[i]
                if f > c:
                    out[i] = (enh[i, c * FRAME:f * FRAME].copy(), sc[i, c:f].copy())
        for i, r in enumerate(rows):
            f = frames[i]
            h = min(f, HALO)
            self.keep[i] = r[(f - h) * self.step:].copy()
            self.ctx[i] = h
        return out
