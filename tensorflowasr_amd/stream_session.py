"""Streaming sessions: the reference's stream_asr_session.py on the MI355X, one stream at a time (`StreamingASRSession`)
and many at once (`StreamingASRServer`).

    session = StreamingASRSession(asr, vad)              # asr: a streaming ASR (am_data.yml streaming: True)
    for packet in packets:                               # bytes of int16 samples at 16 kHz, a multiple of 160 samples
        event = session.send(packet)                     # None, or {'event_type': 'sentence begin' | 'inter break' | 'sentence end', ...}
    event = session.final_send()

    server = StreamingASRServer(asr, vad, n_streams=64, max_history_s=60)
    events = server.send([packet_or_None for each stream])

`TaskContent` is the per-stream state machine, written from the reference's behaviour; the events are compared with the
reference's one by one (tests/golden/stream_session_ref.json), so its quirks are kept:

* a packet is int16 bytes; the clock (seconds) grows by len / rate per packet, in floating point, and every time comes from it;
* the detector sees the last 3 s of audio (`(vad_time + 2) * rate` samples), which start as 2 400 zeros -- 0.15 s, not 3 s --
  so the first windows are short; every `0.1 * vad_time` s the window, decimated by two, is scored in 80-sample frames and
  the last ten decisions (score >= 0) are noted.  A packet must be a multiple of 160 samples or the window does not divide
  into 80-sample frames and the call raises, as in the reference;
* outside a sentence: every second scoring, 5 voiced of the last 10 decisions start a sentence; its audio begins with the last
  0.2 s and its begin time is clock - 0.2;
* inside a sentence: every second scoring the silence ladder moves -- from step 0 on at most 8 voiced of the last 10 (this notes
  an inter break and the end time = clock), from step 1 on at most 5, from step 2 up on at most `end_votes`, anything else
  puts it back to 0; step `wait_sil` ends the sentence with end time = clock - wait_sil * 0.1 + 0.1.  Otherwise a piece is
  due whenever `chunk_seconds` of new audio have come in;
* the begin event is returned before anything else is looked at, and the piece is not trimmed on that packet;
* a due piece is answered as an inter break (encoded, decoded behind the history) when a break is noted and the ladder stands
  at step 1, otherwise it is encoded and joins the history while the break stays noted.  A detector that hovers at 6 .. 8
  voiced of 10 moves the ladder 0, 1, 0, 1, ..., so inter breaks are the most frequent event (25 and 27 against 11 sentences
  in the fixture's two feeds);
* at an inter break or a sentence end the audio since the last piece is encoded and decoded behind the history if it is longer
  than 800 samples; at an inter break it joins the history only if it is a full piece long;
* closing a stream ends a running sentence whose audio is longer than 800 samples (exactly 800: nothing happens);
* the reference's `final_send` looks up a task id that only an answered inter break of the same sentence leaves behind, and
  raises KeyError otherwise; here the sentence-end event is returned (it never carried the id).

Punctuation: the reference passes texts of 5 or more characters through its Punc model.  `punc` is an optional callable
(text -> list or string) applied at the same places -- `tensorflowasr_amd.punc.Punc` is that model on the GPU, and an instance is
the hook; the default leaves the text as it is (as the offline `ASRSession`).  A hook with `punc_recover_batch` (Punc has it) is
called once per server tick with all the texts due, instead of once per text."""
import collections
import enum

import numpy as np


class Phase(enum.Enum):
    IDLE = 0        # between sentences
    SPEECH = 1      # inside a sentence


# what a stream asks of the recogniser after a packet
BEGIN, END, INTER, CHUNK, FINAL = "begin", "end", "inter", "chunk", "final"


class TaskContent:
    """One stream: clock, detector window, decisions, silence ladder, the audio of the running sentence and the encoder
    outputs kept for it (`history`).  `push(packet)` = `feed` + scoring + `step`; `want()` says what the recogniser has to do,
    `settle(action)` takes note that it was done."""

    def __init__(self, session, chunk_seconds, sample_rate=8000, wait_sil=5, vad_time=1, start_votes=5, end_votes=2):
        self.session = session
        self.rate = sample_rate
        self.chunk_samples = chunk_seconds * sample_rate
        self.wait_sil, self.vad_time = wait_sil, vad_time
        self.start_votes, self.end_votes = start_votes, end_votes
        self.detector = None
        self._cap = int((vad_time + 2) * sample_rate)
        self.restart()

    def restart(self):
        """a new stream: the clock and the detector window start over too"""
        self.clock = 0
        self._scored_at = 0
        self._ring = np.zeros(self._cap, np.float32)      # the window, right-aligned
        self._held = 2400
        self.drop_sentence()

    def drop_sentence(self):
        """forget the running sentence, keep the clock and the window"""
        self.phase = Phase.IDLE
        self._votes = collections.deque(maxlen=10)
        self._noted = 0                                   # decisions noted since the last look at them (10 carried over)
        self.ladder = 0
        self.break_noted = False
        self.began = False
        self.due = None                                   # None / "piece" / "end"
        self.begin_s = self.end_s = 0.
        self.history = []
        self._clear_audio()

    def _clear_audio(self):
        self._parts, self._samples, self._mark = [], 0, 0

    # ---- detector -------------------------------------------------------------------------------------------------------
    def window_samples(self):
        return self._held

    def frames(self):
        """what the detector scores: the window decimated by two, [T, 80] float32"""
        return self._ring[self._cap - self._held:][::2].reshape(-1, 80).copy()

    def votes(self, scores):
        v = (np.asarray(scores).reshape(-1) >= 0.).astype(int).tolist()
        return v[-int(10 * self.vad_time):]

    # ---- one packet -----------------------------------------------------------------------------------------------------
    def feed(self, packet):
        """take the packet in; True when the window is due for scoring (pass `votes(scores of frames())` to `step`)"""
        x = np.frombuffer(packet, "<i2").astype(np.float32) / np.float32(32768)
        n = len(x)
        self.clock += n / self.rate
        if self.phase is Phase.SPEECH:
            self._parts.append(x)
            self._samples += n
        if n >= self._cap:
            self._ring[:] = x[n - self._cap:]
        elif n:
            self._ring[:-n] = self._ring[n:]
            self._ring[-n:] = x
        self._held = min(self._cap, self._held + n)
        return self.clock - self._scored_at >= 0.1 * self.vad_time

    def step(self, votes=None):
        if votes is not None:
            self._votes.extend(votes)
            self._noted += len(votes)
            self._scored_at = self.clock
        if self.phase is Phase.SPEECH:
            self._step_speech()
        elif self._noted == 20:
            if sum(self._votes) >= self.start_votes:
                self.phase, self.began = Phase.SPEECH, True
                self._votes.clear()
                self._noted = 0
                lead = self._ring[self._cap - min(self._held, int(self.rate * 0.2)):].copy()
                self._parts, self._samples = [lead], len(lead)
                self.begin_s = self.clock - 0.2
            else:
                self._noted = 10

    def _step_speech(self):
        if self._noted >= 20:
            voiced = sum(self._votes)
            limit = 8 if self.ladder == 0 else 5 if self.ladder == 1 else self.end_votes
            if voiced > limit:
                self.ladder = 0
            else:
                if self.ladder == 0:
                    self.break_noted = True
                    self.end_s = self.clock
                self.ladder += 1
            self._noted = 10
        fresh = self._samples - self._mark
        if self.ladder == self.wait_sil:
            self.end_s = self.clock - self.wait_sil * 0.1 + 0.1
            self.phase = Phase.IDLE
            self._votes.clear()
            self._noted = 0
            self.ladder = 0
            self.break_noted = False
            self.due = "end"
        elif fresh >= self.chunk_samples:
            self.due = "piece"
            self._mark = self._samples
        elif fresh == 0:
            self.due = None

    def push(self, packet):
        self.step(self.votes(self.detector.inference(self.frames()[None])) if self.feed(packet) else None)

    def close(self):
        """the stream is over: a running sentence with more than 800 samples of audio ends now"""
        if self.phase is Phase.SPEECH and self._samples > 800:
            self.due = "end"
            self.end_s = self.clock

    # ---- the recogniser's side ----------------------------------------------------------------------------------------------
    def audio(self):
        return np.concatenate(self._parts) if self._parts else np.zeros(0, np.float32)

    def want(self, closing=False):
        """(action, audio): audio = the float32 piece to encode, None when there is nothing to encode"""
        if closing:
            if self.due is None:
                return None, None
            a = self.audio()
            return FINAL, (a if len(a) > 800 else None)
        if self.began:
            return BEGIN, None
        if self.due is None:
            return None, None
        a = self.audio()
        tail = a if len(a) > 800 else None
        if self.due == "end":
            return END, tail
        if self.break_noted and self.ladder == 1:
            return INTER, tail
        return CHUNK, a

    def joins_history(self, action, audio):
        return action == CHUNK or (action == INTER and audio is not None and len(audio) >= self.chunk_samples)

    def settle(self, action):
        if action == BEGIN:
            self.began = False
            return
        if action in (END, FINAL):
            self.phase = Phase.IDLE
            self.begin_s = self.end_s = 0.
            self.history = []
            self._clear_audio()
        elif action == INTER:
            self.break_noted = False
        if action is not None:
            self.due = None
        if self._samples >= self.chunk_samples:          # a full piece has been used up
            self._clear_audio()


class _Stream:
    """a TaskContent plus what the session adds: sentence numbering, punctuation and the event dictionaries; split into
    `plan` and `finish` so that a server can run the recogniser for many streams in between"""

    def __init__(self, session, sample_rate, punc):
        self.session = session
        self.punc = punc
        self.task_content = TaskContent(session, 0.5, sample_rate, 5)
        self.sentence_id = 0

    def plan(self, closing=False):
        if closing:
            self.task_content.close()
        return self.task_content.want(closing)

    def wants_punc(self, text):
        return self.punc is not None and text is not None and len(text) >= 5

    def _text(self, text, punctuated=None):
        if punctuated is not None:           # the server ran the hook for this text already (one call per tick)
            text = punctuated
        elif self.wants_punc(text):
            text = self.punc(text)
        return "".join(text)

    def finish(self, action, text=None, closing=False, punctuated=None):
        tc = self.task_content
        resp = None
        if action == BEGIN:
            resp = dict(session=self.session, event_type="sentence begin", sentence_index=int(self.sentence_id),
                        sentence_begin_time=int(tc.clock * 1000 - 200))
        elif action in (END, FINAL):
            resp = dict(session=self.session, event_type="sentence end", sentence_index=int(self.sentence_id),
                        sentence_begin_time=int(tc.begin_s * 1000), best_text=str(self._text(text, punctuated)),
                        sentence_end_time=int(tc.end_s * 1000))
            self.sentence_id += 1
        elif action == INTER:
            resp = dict(session=self.session, event_type="inter break", sentence_begin_time=int(tc.begin_s * 1000),
                        sentence_end_time=int(tc.end_s * 1000), best_text=str(self._text(text, punctuated)))
        tc.settle(action)
        if closing:
            tc.restart()
        return resp


class StreamingASRSession:
    """stream_asr_session.py ASRSession: `send(bytes)` / `final_send()` return None or the reference's event dict.
    asr: `extract_feature(wav) -> enc` and `decode([enc, ...]) -> text` (tensorflowasr_amd.asr.ASR with a streaming
    encoder); vad: `inference([1, T, 80]) -> scores` (tensorflowasr_amd.vad.VAD)."""

    def __init__(self, asr, vad, session="asr_1", sample_rate=16000, punc=None):
        self.session = session
        self.sample_rate = sample_rate
        self.asr = asr
        self._s = _Stream(session, sample_rate, punc)
        self.task_content = self._s.task_content
        self.task_content.detector = vad

    @property
    def sentence_id(self):
        return self._s.sentence_id

    def _recognise(self, action, audio):
        tc = self.task_content
        if action == CHUNK:
            tc.history = tc.history + [self.asr.extract_feature(audio)]
            return None
        if action not in (END, INTER, FINAL):
            return None
        if audio is None:
            return self.asr.decode(tc.history)
        enc = self.asr.extract_feature(audio)
        text = self.asr.decode(tc.history + [enc])
        if tc.joins_history(action, audio):
            tc.history = tc.history + [enc]
        return text

    def send(self, audio_data):
        self.task_content.push(audio_data)
        action, audio = self._s.plan()
        return self._s.finish(action, self._recognise(action, audio))

    def final_send(self):
        action, audio = self._s.plan(closing=True)
        return self._s.finish(action, self._recognise(action, audio), closing=True)


# ---- device plumbing of the server -----------------------------------------------------------------------------------
def stream_append(chunks, slots, hist, hist_len, hist_len_host):
    """mi355asr_stream_append: chunks [M, Tc, d] (device) go behind the histories of `slots` (list of ints) in hist
    [N, Tcap, d]; hist_len (device int32 [N]) and hist_len_host (numpy int32 [N]) advance by Tc"""
    import ctypes
    import torch
    from . import _lib
    M, Tc, d = chunks.shape
    N, Tcap, _ = hist.shape
    sh = np.ascontiguousarray(slots, np.int32)
    sd = torch.from_numpy(sh).to(hist.device)
    with torch.cuda.device(hist.device):
        st = ctypes.c_void_p(torch.cuda.current_stream(hist.device).cuda_stream)
        _lib.check(_lib.lib().mi355asr_stream_append(
            ctypes.c_void_p(chunks.data_ptr()), ctypes.c_void_p(sd.data_ptr()), sh.ctypes.data_as(ctypes.c_void_p), M, Tc, d,
            ctypes.c_void_p(hist.data_ptr()), ctypes.c_void_p(hist_len.data_ptr()), hist_len_host.ctypes.data_as(ctypes.c_void_p),
            N, Tcap, st))


def stream_gather(hist, hist_len, hist_len_host, slots, Tpad, tails=None, tail_len=None):
    """mi355asr_stream_gather: the histories of `slots` as a dense batch -> (out [M, Tpad, d], out_len int32 [M]), both on the
    device.  tails [M, Tt, d] with tail_len (ints, 0 = none): pieces placed behind the histories without being stored."""
    import ctypes
    import torch
    from . import _lib
    N, Tcap, d = hist.shape
    sh = np.ascontiguousarray(slots, np.int32)
    M = len(sh)
    sd = torch.from_numpy(sh).to(hist.device)
    out = torch.empty((M, Tpad, d), dtype=torch.float32, device=hist.device)
    out_len = torch.empty((M,), dtype=torch.int32, device=hist.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()
    th = td = None
    if tails is not None:
        th = np.ascontiguousarray(tail_len, np.int32)
        td = torch.from_numpy(th).to(hist.device)
    with torch.cuda.device(hist.device):
        st = ctypes.c_void_p(torch.cuda.current_stream(hist.device).cuda_stream)
        _lib.check(_lib.lib().mi355asr_stream_gather(
            p(hist), p(hist_len), hist_len_host.ctypes.data_as(ctypes.c_void_p), N, Tcap, d, p(sd), sh.ctypes.data_as(ctypes.c_void_p), M,
            p(tails), p(td), th.ctypes.data_as(ctypes.c_void_p) if th is not None else ctypes.c_void_p(),
            int(tails.shape[1]) if tails is not None else 0, p(out), p(out_len), Tpad, st))
    return out, out_len


class StreamHistoryOverflow(RuntimeError):
    """a stream's sentence has outgrown max_history_s; the stream has been reset"""


class _HostRecogniser:
    """the server's recogniser for objects that only have extract_feature / decode (stubs): one call per stream"""

    def __init__(self, asr):
        self.asr = asr

    def run(self, state, encode, decode):
        enc = {i: self.asr.extract_feature(audio) for i, audio, _ in encode}
        texts = {}
        for i, with_tail in decode:
            texts[i] = self.asr.decode(state[i] + ([enc[i]] if with_tail else []))
        for i, _, joins in encode:
            if joins:
                state[i] = state[i] + [enc[i]]
        return texts


class StreamingASRServer:
    """N streams advanced together.  `send(packets)`: one packet (bytes) or None per stream -> one event or None per stream.
    Per tick: the VAD windows due are scored in one `vad.inference` per window length (every stream older than 3 s has the
    same one); the pieces due -- chunks, and the tails of the decodes due -- go through the streaming encoder in one call
    and behind their histories with `stream_append` (one launch per piece size in chunks); the decodes due are gathered
    (`stream_gather`, tails that do not join a history included) and run through one ragged CTCDecoder call, one greedy
    collapse and one ragged Translator call.  A stream whose history would pass max_history_s (counting the pieces that join
    it) gets a `StreamHistoryOverflow` in its place of the result list, returned, not raised, so that the other streams go on;
    nothing is launched for it, its sentence is dropped without an end event, and its clock and sentence numbering go on, so
    the next sentence's times stay those of the stream."""

    def __init__(self, asr, vad, n_streams, max_history_s=60., session="asr", sample_rate=16000, punc=None):
        self.asr, self.vad, self.n = asr, vad, int(n_streams)
        self.sample_rate = sample_rate
        self.punc = punc
        self.streams = [_Stream("%s_%d" % (session, i + 1), sample_rate, punc) for i in range(self.n)]
        self.device_path = hasattr(asr, "encoder") and hasattr(asr, "ctc_model") and hasattr(asr, "translator")
        self.max_history_s = float(max_history_s)
        if self.device_path:
            import torch
            self.chunk = int(asr.chunk)
            self.frames = int(asr.encoder._h.out_frames(self.chunk)[1])
            self.Tcap = self.frames * max(1, int(np.ceil(self.max_history_s * sample_rate / self.chunk)))
            d = asr.model_config["dmodel"]
            dev = asr.encoder._h.device
            self.hist = torch.zeros((self.n, self.Tcap, d), dtype=torch.float32, device=dev)
            self.hist_len = torch.zeros((self.n,), dtype=torch.int32, device=dev)
            self.hist_len_host = np.zeros(self.n, np.int32)
        else:
            self._host = _HostRecogniser(asr)
            self.state = [[] for _ in range(self.n)]

    def __len__(self):
        return self.n

    # ---- VAD: all windows due, grouped by length ----------------------------------------------------------------------
    def _score(self, due):
        groups = {}
        for i in due:
            w = self.streams[i].task_content.frames()
            groups.setdefault(w.shape[0], []).append((i, w))
        preds = {}
        for items in groups.values():
            s = np.asarray(self.vad.inference(np.stack([w for _, w in items])))
            s = s.reshape(len(items), -1)
            for (i, _), row in zip(items, s):
                preds[i] = self.streams[i].task_content.votes(row)
        return preds

    def _reset_history(self, i):
        if self.device_path:
            if self.hist_len_host[i]:
                self.hist_len_host[i] = 0
                self.hist_len[i] = 0
        else:
            self.state[i] = []

    def _chunks_of(self, audio):
        return -(-len(audio) // self.chunk)

    # ---- the recogniser for one tick ------------------------------------------------------------------------------------
    def _run_device(self, encode, decode):
        """encode: [(stream, audio, joins_history)], decode: [(stream, with_tail)] -> {stream: text}"""
        import torch
        asr = self.asr
        enc_of = {}
        if encode:
            n = [self._chunks_of(a) for _, a, _ in encode]
            x = np.zeros((sum(n), self.chunk), np.float32)           # a piece is zero-padded to whole chunks (ASR.extract_feature)
            r = 0
            for (_, a, _), k in zip(encode, n):
                x[r:r + k].reshape(-1)[:len(a)] = a
                r += k
            enc = asr.encoder.inference(x.reshape(len(x), -1, 1))        # [chunks, frames, d]: every chunk on its own
            r = 0
            for (i, _, _), k in zip(encode, n):
                enc_of[i] = enc[r:r + k].reshape(1, k * self.frames, -1)
                r += k
            by_size = {}
            for (i, _, joins), k in zip(encode, n):
                if joins:
                    by_size.setdefault(k, []).append(i)
            for k, idx in by_size.items():
                stream_append(torch.cat([enc_of[i] for i in idx], 0).contiguous(), idx, self.hist, self.hist_len, self.hist_len_host)
        if not decode:
            return {}
        idx = [i for i, _ in decode]
        joined = {i for i, _, j in encode if j}
        tl = [int(enc_of[i].shape[1]) if with_tail and i not in joined else 0 for i, with_tail in decode]
        tails = None
        if any(tl):
            tails = torch.zeros((len(idx), max(tl), self.hist.shape[2]), dtype=torch.float32, device=self.hist.device)
            for r, (i, t) in enumerate(zip(idx, tl)):
                if t:
                    tails[r, :t] = enc_of[i][0]
        lens = self.hist_len_host[idx] + np.array(tl, np.int32)
        Tpad = max(17, int(lens.max()))
        batch, blen = stream_gather(self.hist, self.hist_len, self.hist_len_host, idx, Tpad, tails, tl if tails is not None else None)
        return dict(zip(idx, asr.decode_batch(batch, blen, lens)))

    def _recognise(self, encode, decode):
        if self.device_path:
            return self._run_device(encode, decode)
        return self._host.run(self.state, encode, decode)

    def _history_after(self, i, action, audio):
        if not self.device_path:
            return 0
        joins = audio is not None and self.streams[i].task_content.joins_history(action, audio)
        add = self._chunks_of(audio) * self.frames if joins else 0      # (a tail that does not join is not stored)
        return int(self.hist_len_host[i]) + add

    def _tick(self, plans, finish):
        out = [None] * self.n
        encode, decode, live = [], [], {}
        for i, (action, audio) in plans.items():
            st = self.streams[i]
            if action in (END, INTER, CHUNK, FINAL) and self.device_path and self._history_after(i, action, audio) > self.Tcap:
                out[i] = StreamHistoryOverflow("stream %d: more than max_history_s = %g s of speech in one sentence" % (i, self.max_history_s))
                st.task_content.drop_sentence()
                self._reset_history(i)
                continue
            live[i] = action
            if audio is not None and action is not None and action != BEGIN:
                encode.append((i, audio, st.task_content.joins_history(action, audio)))
            if action in (END, INTER, FINAL):
                decode.append((i, audio is not None))
        texts = self._recognise(encode, decode) if (encode or decode) else {}
        punctuated = {}
        if hasattr(self.punc, "punc_recover_batch"):
            # every text this tick's events carry, through the hook in one call (a hook without the batch form runs per text)
            due = [i for i, action in live.items() if action in (END, INTER, FINAL) and self.streams[i].wants_punc(texts.get(i))]
            if due:
                punctuated = dict(zip(due, self.punc.punc_recover_batch([texts[i] for i in due])))
        for i, action in live.items():
            out[i] = finish(self.streams[i], action, texts.get(i), punctuated.get(i))
            if action in (END, FINAL):
                self._reset_history(i)
        return out

    def send(self, packets):
        if len(packets) != self.n:
            raise ValueError("%d packets for %d streams" % (len(packets), self.n))
        tcs = [s.task_content for s in self.streams]
        due = [i for i, p in enumerate(packets) if p is not None and tcs[i].feed(p)]
        preds = self._score(due) if due else {}
        plans = {}
        for i, p in enumerate(packets):
            if p is not None:
                tcs[i].step(preds.get(i))
                plans[i] = self.streams[i].plan()
        return self._tick(plans, lambda st, action, text, punctuated: st.finish(action, text, punctuated=punctuated))

    def final_send(self, streams=None):
        """end the given streams (default: all) -> one event or None per stream of the server (None for the others)"""
        idx = range(self.n) if streams is None else ([streams] if isinstance(streams, int) else streams)
        plans = {i: self.streams[i].plan(closing=True) for i in idx}
        out = self._tick(plans, lambda st, action, text, punctuated: st.finish(action, text, closing=True, punctuated=punctuated))
        for i in idx:
            self._reset_history(i)
        return out
