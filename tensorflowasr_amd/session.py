"""`ASRSession`: offline_asr_session.py ASRSession on the MI355X -- VAD segmentation of a long recording, then one
recognition per segment.

    session = ASRSession(asr, vad)
    for r in session.send('long.wav'):
        print(r['sentence_begin_time'], r['sentence_end_time'], r['best_text'])

Each segment is decoded as its own utterance (`ASR.offline_stt_wave` on the slice): zero-padding segments into one plain
batch would change their results.  `ASR.offline_stt_batch(segments)` decodes segments of different lengths in ragged
batches (mi355asr_*_ragged) with the per-segment results, for callers that batch them.  Punctuation: with `punc=` (a callable
text -> list or string; `tensorflowasr_amd.punc.Punc` is the reference's Punc model on the GPU) a segment's text of more than
5 characters goes through it, the offline reference's test, and the result is joined into `best_text`; the default `None`
leaves `best_text` the Translator's text.  The segmentation is the reference's OfflineVAD (vad.py), including
its behaviour of returning at most one segment, from the first speech onset to the end of the recording."""
import numpy as np

from .featurizers import read_raw_audio
from .vad import OfflineVAD


class ASRSession:
    def __init__(self, asr, vad, session="asr_1", sample_rate=16000, punc=None):
        self.session = session
        self.punc = punc
        self.sample_rate = sample_rate
        self.asr = asr
        self.offline_vad = OfflineVAD(sr=sample_rate)
        self.offline_vad.compile(vad)

    def send(self, wav_path, sample_rate=None):
        """wav path or 1-D array -> [{session, sentence_index, sentence_begin_time, best_text, sentence_end_time}],
        times in integer ms.  Like the reference, every dict carries session 'asr_1'.  Also sets `self.phones`, the
        phone string behind each best_text.

        sample_rate: the rate of the recording when it is not the session's.  The recording (an array, float32 or int16 PCM,
        or a file of that rate) is resampled on the device first (resample.Resampler) and then handled as one at the
        session's rate: the times are those of the resampled recording, which spans the same milliseconds."""
        if sample_rate is not None and int(sample_rate) != int(self.sample_rate):
            from .featurizers import read_wav_native
            from .resample import Resampler
            wav = wav_path
            if not isinstance(wav, np.ndarray):
                wav, file_rate = read_wav_native(wav)
                if file_rate != int(sample_rate):
                    raise ValueError("%s is a %d Hz file, sample_rate says %d" % (wav_path, file_rate, int(sample_rate)))
            wav = wav.reshape(-1)
            cache = self.__dict__.setdefault("_resamplers", {})
            if int(sample_rate) not in cache:
                cache[int(sample_rate)] = Resampler(int(sample_rate), self.sample_rate, device=getattr(self.asr, "device", "cuda:0"))
            y, _ = cache[int(sample_rate)](wav if wav.dtype == np.int16 else wav.astype(np.float32, copy=False))
            wav = y[0].cpu().numpy() if len(wav) else np.zeros(0, np.float32)
        else:
            wav = read_raw_audio(wav_path, self.sample_rate) if not isinstance(wav_path, np.ndarray) else wav_path
        wav = np.asarray(wav, np.float32).reshape(-1)
        wav = wav[:len(wav) // 80 * 80]
        responses, self.phones = [], []
        for idx, (s, e) in enumerate(self.offline_vad.vad(wav)):
            data = wav[int(s * self.sample_rate):int(e * self.sample_rate)]
            phones, text = self.asr.offline_stt_wave(data)
            if self.punc is not None and len(text) > 5:
                text = "".join(self.punc(text))
            self.phones.append(phones)
            responses.append({"session": "asr_1", "sentence_index": idx, "sentence_begin_time": int(s * 1000),
                              "best_text": text, "sentence_end_time": int(e * 1000)})
        return responses
