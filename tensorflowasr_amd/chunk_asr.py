"""`ChunkASR` and `ChunkAMTester`: the recogniser of the reference's test_chunk_asr.py (:21-139) and the evaluation loop
of asr/tester/chunk_tester.py (:14-80) for the ChunkConformer, on the MI355X model of this package.

    from tensorflowasr_amd.config import UserConfig
    from tensorflowasr_amd.chunk_asr import ChunkASR
    asr = ChunkASR(UserConfig('configs/am_data.yml', 'configs/chunk_conformerS.yml'))
    for t, phones, text in asr.stream_call('utt.wav')["streaming"]: ...

Same construction as the reference (`ChunkConformer(config, phone_num_classes, text_num_classes)`, weights from the newest
TensorFlow checkpoint under `<outdir>/all-ckpt`, test_chunk_asr.py:36-43), same streaming loop: `wav_buf_length` samples
per call -> picker_stream_predict -> feature_pick -> decoder_stream_predict, greedy CTC decode of [valid | unvalid] text
logits after every call, and the offline `predict` of the whole utterance for comparison.  Every tensor operation between
the waveform and the token ids runs in libmi355asr.so."""
import logging
import os

import numpy as np
import torch

from .eval import _Mean, update_from_device_scores, wer
from .featurizers import SpeechFeaturizer, TextFeaturizer
from .models import ChunkConformer, ctc_greedy_decode, frame_argmax


def _ctc_text(logits, blank):
    """softmax + tf.keras.backend.ctc_decode(greedy) + clip (test_chunk_asr.py:88-100): [1, T, V] logits -> id list without
    zeros.  The argmax of softmax(x) is the argmax of x; the blank is the last class."""
    if logits.shape[1] == 0:
        return []
    ids, lens = ctc_greedy_decode(frame_argmax(logits), None, blank=blank)
    row = ids[0, :int(lens[0].item())].clamp(min=0).cpu().numpy()
    return [int(n) for n in row if n != 0]


class ChunkASR:
    def __init__(self, config, device="cuda:0", load_checkpoint=True):
        self.running_config = config["running_config"]
        self.speech_config = config["speech_config"]
        self.model_config = config["model_config"]
        self.opt_config = config["optimizer_config"] if "optimizer_config" in config else None
        self.phone_featurizer = TextFeaturizer(config["inp_config"])
        self.text_featurizer = TextFeaturizer(config["tar_config"])
        self.speech_featurizer = SpeechFeaturizer(self.speech_config)
        self.config = config
        self.device = device
        self.compile(load_checkpoint)

    # test_chunk_asr.py:35-45
    def compile(self, load_checkpoint=True):
        self.runner = ChunkConformer(self.config, self.phone_featurizer.num_classes, self.text_featurizer.num_classes,
                                     device=self.device)
        self.runner._build()
        if load_checkpoint:
            from .checkpoint import latest_tf_checkpoint
            path = latest_tf_checkpoint(os.path.join(self.running_config["outdir"], "all-ckpt"))
            self.runner.load_weights(path)
            logging.info("ChunkConformer load at %s", path)
        chunk_num, hop, _, _ = self.runner._stream_cfg()
        self.wav_buf_length = chunk_num * hop          # ChunkConformerFront.wav_buf_length (chunk_conformer_blocks.py:419)

    def load_wav(self, wav_path):
        data = self.speech_featurizer.load_wav(wav_path)
        return data / np.abs(data.max())               # test_chunk_asr.py:49 (sic: abs of the max, not max of the abs)

    def offline_stt(self, wav_path):
        """runner.predict on the whole utterance + greedy CTC decode (test_chunk_asr.py:56, 124-137) -> text; with
        `beam_width` > 1 in the text vocabulary's config, the prefix beam search (and its `lm_config` scorer) instead"""
        data = self.load_wav(wav_path)
        logits, _ = self.runner.predict(data.reshape([1, -1, 1]))
        beam = int(self.text_featurizer.decoder_config.get("beam_width", 1) or 1)
        if beam > 1:
            return "".join(self.text_featurizer.iextract(self._beam_text(logits, beam)))
        return "".join(self.text_featurizer.iextract(_ctc_text(logits, self.text_featurizer.num_classes - 1)))

    def _beam_text(self, logits, beam):
        """beam_width > 1: the best hypothesis of the prefix beam search on the text logits, with the vocabulary's scorer
        (lm_config) if it has one -> id list without zeros, as _ctc_text returns"""
        from .models import ctc_prefix_beam_decode
        if logits.shape[1] == 0:
            return []
        ids, lens, _, _ = ctc_prefix_beam_decode(logits, None, beam, is_logits=True, ext_scorer=self.text_featurizer.scorer)
        return [int(n) for n in ids[0, 0, :int(lens[0, 0])] if n != 0]

    def _resampler(self, rate):
        """the device resampler from `rate` to the model's rate (one per rate, kept)"""
        from .resample import Resampler
        cache = self.__dict__.setdefault("_resamplers", {})
        if rate not in cache:
            cache[rate] = Resampler(rate, self.speech_featurizer.sample_rate, device=self.device)
        return cache[rate]

    def _batch_ids(self, logits, counts):
        """the text ids of every row of a ragged batch's text logits [B, Tp, V], row b over its first counts[b] frames:
        greedy (frame_argmax + ctc_greedy_decode), or with `beam_width` > 1 in the text vocabulary's config the prefix beam
        search with the vocabulary's scorer -> B id lists without zeros, as _ctc_text / _beam_text return for one row"""
        B = logits.shape[0]
        if logits.shape[1] == 0:
            return [[] for _ in range(B)]
        in_len = torch.as_tensor(np.asarray(counts, np.int32), device=logits.device)
        beam = int(self.text_featurizer.decoder_config.get("beam_width", 1) or 1)
        if beam > 1:
            from .models import ctc_prefix_beam_decode
            ids, lens, _, _ = ctc_prefix_beam_decode(logits, in_len, beam, is_logits=True, ext_scorer=self.text_featurizer.scorer)
            return [[int(n) for n in ids[b, 0, :int(lens[b, 0])] if n != 0] for b in range(B)]
        ids, lens = ctc_greedy_decode(frame_argmax(logits), in_len, blank=self.text_featurizer.num_classes - 1)
        ids, lens = ids.clamp(min=0).cpu().numpy(), lens.cpu().numpy()
        return [[int(n) for n in ids[b, :int(lens[b])] if n != 0] for b in range(B)]

    def offline_stt_batch(self, items, max_batch_samples=None, sample_rates=None):
        """offline_stt for every item of a list -- paths or 1-D waveforms -- in ragged batches: ONE ragged `predict` per batch
        (mi355asr_chunk_predict_ragged), each row computed as if alone, then the greedy decode (or the prefix beam search) of
        every row over its own counts[b] text frames.  Returns the texts in the order of `items`.  Every item is normalised as
        `load_wav` does (data / abs(data.max())), the items are sorted by length and cut into batches of at most
        max_batch_samples padded samples (None: one batch).  sample_rates: as ASR.offline_stt_batch -- an item with a rate is
        resampled on the device (resample.Resampler) and normalised there, over its own samples."""
        from .asr import batch_items, batch_rows, cut_batches
        model_rate = int(self.speech_featurizer.sample_rate)
        waves, rates = batch_items(items, sample_rates, self.speech_featurizer.load_wav, model_rate)
        own = lambda i: rates is None or rates[i] is None
        waves = [w / np.abs(w.max()) if own(i) and len(w) else w for i, w in enumerate(waves)]
        n16, batches = cut_batches(waves, rates, model_rate, max_batch_samples)
        hop = int(self.runner._stream_cfg()[1])
        for i, n in enumerate(n16):
            if n < 2 * hop + 1:
                raise ValueError("item %d has %d samples at the model's rate: the chunk front end needs at least %d" % (i, n, 2 * hop + 1))
        out = [None] * len(waves)
        for idx in batches:
            lens = np.array([n16[i] for i in idx], np.int32)
            x = batch_rows(waves, rates, idx, lens, int(lens.max()), self._resampler, self.device)
            if isinstance(x, torch.Tensor):                    # the resampled rows: normalised where they are
                for r, i in enumerate(idx):
                    if not own(i):
                        row = x[r, :int(lens[r])]
                        x[r, :int(lens[r])] = row / row.max().abs()
            logits, counts = self.runner.predict(x, wav_lengths=lens)
            for r, ids in enumerate(self._batch_ids(logits, counts)):
                out[idx[r]] = "".join(self.text_featurizer.iextract(ids))
        return out

    def stream_call(self, wav_path, verbose=False):
        """test_chunk_asr.py:47-139 -> {"streaming": [(seconds_heard, phones, text), ...], "offline": text}"""
        r = self.runner
        data = self.load_wav(wav_path)
        dev = r._h.device
        caches, caches2 = r.init_picker_caches(1), r.init_decoder_caches(1)
        Vt, Vp = self.text_featurizer.num_classes, self.phone_featurizer.num_classes
        valid_txt_outs = torch.zeros((1, 0, Vt), device=dev)
        valid_phone_outs = torch.zeros((1, 0, Vp), device=dev)
        unvalid_txt_outs = torch.zeros((1, 0, Vt), device=dev)
        out = []
        for i in range(99999):
            s = i * self.wav_buf_length
            e = s + self.wav_buf_length
            if s >= len(data):
                break
            input_wav = data[int(s):int(e)].reshape([1, -1, 1])
            valid_phone_out, _, valid_hidden_out, caches = r.picker_stream_predict(input_wav, caches)
            if valid_phone_out.shape[1] == 0:
                continue
            feature_outputs, picked_phone_out = r.feature_pick(valid_hidden_out, valid_phone_out)
            if feature_outputs.shape[1] != 0:
                valid_ctc_out, unvalid_txt_outs, caches2 = r.decoder_stream_predict(feature_outputs, caches2)
                valid_txt_outs = torch.cat([valid_txt_outs, valid_ctc_out], 1)
                valid_phone_outs = torch.cat([valid_phone_outs, picked_phone_out], 1)
            txt_output = torch.cat([valid_txt_outs, unvalid_txt_outs], 1)
            if txt_output.shape[1] == 0 or valid_phone_outs.shape[1] == 0:
                continue
            text = self.text_featurizer.iextract(_ctc_text(txt_output, Vt - 1))
            phone = self.phone_featurizer.iextract(_ctc_text(valid_phone_outs, Vp - 1))
            out.append((e / self.speech_featurizer.sample_rate, " ".join(phone), "".join(text)))
            if verbose:
                print("time:", out[-1][0])
                print("streaming phone out:", phone)
                print("streaming texts out:", text)
        offline = self.offline_stt(wav_path)
        if verbose:
            print("offline texts out:", offline)
        return {"streaming": out, "offline": offline}

    stt = offline_stt


class ChunkAMTester(ChunkASR):
    """asr/tester/chunk_tester.py: `runner.predict(features)` -> softmax -> greedy ctc_decode over all picked frames ->
    SER / CER of the text ids with the S / I / D accumulators.  Batches are the 6-tuples of the reference's chunk loader
    (features, input_length, phone_labels, phone_label_length, tar_label, tar_label_length); 5-tuples of EvalList work too."""

    def __init__(self, config, device="cuda:0", load_checkpoint=True, device_scoring=False):
        self.eval_metrics = {"ser": _Mean(), "cer": _Mean()}
        self.ctc_nums = [0, 0, 0, 0]
        self.steps, self.all_steps = 0, 0
        self.eval_datasets = None
        super().__init__(config, device=device, load_checkpoint=load_checkpoint)
        self.device_scoring = bool(device_scoring)      # True: scoring.EditDistance, one call per batch (same results())
        if self.device_scoring:
            from .scoring import EditDistance
            self.scorer = EditDistance(device)

    def set_all_steps(self, all_steps):
        self.all_steps = all_steps

    def set_datasets(self, evaldataset):
        self.eval_datasets = evaldataset

    def _eval_step(self, batch):
        features, tar_label = batch[0], batch[4]
        logits, _ = self.runner.predict(features)
        B, Tp, V = logits.shape
        pad = self.text_featurizer.pad
        if self.device_scoring:
            refs = np.asarray(tar_label).reshape(B, -1)
            if Tp == 0:
                ids = torch.zeros((B, 0), dtype=torch.int32, device=logits.device)
            else:
                ids, lens = ctc_greedy_decode(frame_argmax(logits), None, blank=V - 1)
                ids = ids[:, :max(int(lens.max().item()), 1)].clamp(min=0)
            update_from_device_scores(self.scorer(refs, ids, drop_ref=(pad,), drop_hyp=(pad,)), self.ctc_nums,
                                      self.eval_metrics["ser"], self.eval_metrics["cer"])
            return
        if Tp == 0:
            hyps = [[] for _ in range(B)]
        else:
            # new_inp_length = ones * ctc_output.shape[1] (chunk_tester.py:40): every picked row, zero padding included
            ids, lens = ctc_greedy_decode(frame_argmax(logits), None, blank=V - 1)
            ids = ids.clamp(min=0).cpu().numpy()
            hyps = [ids[b, :max(int(lens.max().item()), 1)].tolist() for b in range(B)]
        for hyp, ref in zip(hyps, np.asarray(tar_label)):
            i = [int(t) for t in hyp if int(t) != pad]
            j = [int(t) for t in np.asarray(ref).flatten() if int(t) != pad]
            _, ws, wd, wi = wer(j, i)
            self.ctc_nums[0] += len(j); self.ctc_nums[1] += ws; self.ctc_nums[2] += wi; self.ctc_nums[3] += wd
            self.eval_metrics["ser"].update_state(0 if i == j else 1)
            self.eval_metrics["cer"].reset_states()
            self.eval_metrics["cer"].update_state(sum(self.ctc_nums[1:]) / (self.ctc_nums[0] + 1e-6))

    def results(self):
        r = {k: v.result() for k, v in self.eval_metrics.items()}
        r["s_i_d"] = "{}_{}_{}".format(*self.ctc_nums[1:])
        r["steps"] = self.steps
        return r

    def run(self):
        if self.eval_datasets is None:
            raise RuntimeError("call set_datasets(...) first")
        for batch in self.eval_datasets:
            self._eval_step(batch)
            self.steps += 1
            logging.info("[Eval] [Step %d] %s", self.steps, self.results())
            if self.all_steps and self.steps >= self.all_steps:
                break
        return self.results()


class _Greedy:
    """greedy CTC text of a growing frame sequence, kept as integers on the host: merge repeated frames, drop the blank
    (tf.keras.backend.ctc_decode), then drop id 0 as `_ctc_text` does."""

    def __init__(self, blank):
        self.blank, self.prev, self.ids = blank, None, []

    def feed(self, frames):
        for f in frames:
            f = int(f)
            if f != self.prev and f != self.blank:
                self.ids.append(f)
            self.prev = f
        return self

    def fork(self):
        g = _Greedy(self.blank)
        g.prev, g.ids = self.prev, list(self.ids)
        return g

    def text(self):
        return [n for n in self.ids if n != 0]


class _Stream:
    def __init__(self, phone_blank, text_blank):
        self.buf = np.zeros(0, np.float32)
        self.packets = 0
        self.phones = _Greedy(phone_blank)      # over the picked (non-blank) phone frames of every packet so far
        self.n_phone_frames = 0
        self.valid = _Greedy(text_blank)        # over the final text frames
        self.n_valid = 0
        self.unvalid = []                       # the text frames that still wait for right context (of the last decoder run)
        self.beam_ids = []                      # beam_width > 1: the best hypothesis after the last decoder run


class BeamStateOverflow(RuntimeError):
    """a stream's text has more frames than the server's beam state holds (`max_text_frames`)"""


class ChunkStreamingServer:
    """Many live ChunkConformer streams on one GPU: `ChunkASR.stream_call`'s loop for every caller at once.

        srv = ChunkStreamingServer(chunk_asr, 64)
        slot = srv.open()
        for t, phones, text in srv.send({slot: samples})[slot]: ...      # any number of samples per call
        tail = srv.close(slot)                                            # the rest as the short last packet

    `send` cuts what arrives into packets of `wav_buf_length` samples and runs ONE `stream_step` per tick over all streams
    that have a full packet; the tuples are those `stream_call` appends, one per packet completed.  The per-frame argmax
    comes from the head kernels; each stream's greedy text is continued on the host from its frame ids instead of being
    decoded again from all logits.  `stepper` (default: the recogniser's model) is anything with `open_streams`,
    `reset_streams` and `stream_step` of `ChunkConformer`.

    `beam_width` > 1: a tuple's text is the best hypothesis of the prefix beam search (with `ext_scorer`, an n-gram scorer)
    over the stream's final text frames plus, as a peek, the frames that still wait for right context -- `ChunkASR._beam_text`
    (cutoff_prob 0.99, cutoff_top_n 40) on the rows the greedy text reads, kept on the device by a `BeamStreams` of
    `max_text_frames` frames per stream and stepped inside the tick.  With a text decoder of win_back 0
    the reference's unvalid part is zeros_like(valid logits): rows that only ever add id 0 to a greedy text, where it is dropped.
    They are not fed to the search: the text is the committed beam's best.  A stream that outgrows `max_text_frames` gets a
    `BeamStateOverflow` in the place of its tuple -- returned, not raised, as `StreamingASRServer` does for its history, so
    that the other streams go on; `open()` resets a slot's beam with the rest of its state.

    `input_rate` (e.g. 8000): `send` takes samples at that rate and resamples them to the model's on the device, one
    `resample.StreamResampler` step per call for all streams named in it; the tuples are those of a server fed
    the one-shot resampling of each stream's audio."""

    def __init__(self, chunk_asr, n_streams, stepper=None, beam_width=1, ext_scorer=None, max_text_frames=1500, beam_host=False,
                 input_rate=None, max_input_packet=None):
        from .models import StreamGuard
        self.asr = chunk_asr
        self.stepper = stepper if stepper is not None else chunk_asr.runner
        self.n_streams = int(n_streams)
        self.wav_buf_length = int(chunk_asr.wav_buf_length)
        self.state = self.stepper.open_streams(self.n_streams)
        self.guard = StreamGuard(self.n_streams, self.wav_buf_length)
        self.streams = {}
        self.free = list(range(self.n_streams - 1, -1, -1))
        self.win_back = int(getattr(self.state, "win_back", 0))
        self.beam = None
        if int(beam_width) > 1:
            from .models import BeamStreams
            kw = {} if beam_host else {"device": getattr(self.stepper, "_h").device}
            self.beam = BeamStreams(self.n_streams, chunk_asr.text_featurizer.num_classes, int(beam_width), 0.99, 40, ext_scorer,
                                    max_frames=int(max_text_frames), host=bool(beam_host), **kw)
        elif ext_scorer is not None:
            raise ValueError("ext_scorer needs beam_width > 1: the greedy text has no use for a scorer")
        # callers at another rate: one StreamResampler slot per stream slot, stepped once per send for every stream named in it
        self.resampler = None
        model_rate = int(chunk_asr.speech_featurizer.sample_rate)
        if input_rate is not None and int(input_rate) != model_rate:
            from .resample import StreamResampler
            self.input_rate = int(input_rate)
            # the longest piece one step takes (longer ones are cut): one second of input unless told otherwise
            self.max_input_packet = int(max_input_packet or self.input_rate)
            dev = getattr(getattr(self.stepper, "_h", None), "device", None) or getattr(chunk_asr, "device", "cuda:0")
            self.resampler = StreamResampler(self.n_streams, self.input_rate, model_rate, self.max_input_packet, device=dev)

    def open(self):
        if not self.free:
            raise RuntimeError("all %d stream slots are in use" % self.n_streams)
        slot = self.free.pop()
        self.stepper.reset_streams(self.state, [slot])
        self.guard.reset([slot])
        if self.beam is not None:
            self.beam.reset([slot])
        if self.resampler is not None:
            self.resampler.reset([slot])
        self.streams[slot] = _Stream(self.asr.phone_featurizer.num_classes - 1, self.asr.text_featurizer.num_classes - 1)
        return slot

    def _stream(self, slot):
        if slot not in self.streams:
            raise KeyError("slot %r is not open" % (slot,))
        return self.streams[slot]

    def tick(self, packets):
        """{slot: one packet} -> {slot: tuple or None}: one `stream_step` over these streams."""
        slots = sorted(packets)
        rows = [np.asarray(packets[s], np.float32).reshape(-1) for s in slots]
        for s in slots:
            self._stream(s)
        lens = [len(r) for r in rows]
        self.guard.check(slots, lens)
        if self.beam is not None:
            res = self.stepper.stream_step(self.state, slots, rows, beam=self.beam)
        else:
            res = self.stepper.stream_step(self.state, slots, rows)
        self.guard.commit(slots, lens)
        out, full = {}, []
        sr = self.asr.speech_featurizer.sample_rate
        for s in slots:
            st, r = self.streams[s], res[s]
            st.packets += 1
            if r["n_picked"] > 0:                                   # the decoder ran (stream_call: feature_outputs.shape[1] != 0)
                blank = st.phones.blank
                picked = [f for f in r["phone_ids"] if int(f) != blank]
                st.phones.feed(picked)
                st.n_phone_frames += len(picked)
                nv = r["n_valid"]
                st.valid.feed(r["text_ids"][:nv])
                st.n_valid += nv
                # (win_back 0: the reference returns zeros_like(valid logits) as the unvalid part -- nv frames of class 0)
                st.unvalid = list(r["text_ids"][nv:]) if self.win_back else [0] * nv
                if self.beam is not None:
                    if r["beam_status"] != 0:
                        full.append(s)
                    st.beam_ids = [int(t) for t in r["beam_ids"] if t != 0]
            out[s] = None
            if st.n_valid + len(st.unvalid) == 0 or st.n_phone_frames == 0:
                continue
            ids = st.beam_ids if self.beam is not None else st.valid.fork().feed(st.unvalid).text()
            text = self.asr.text_featurizer.iextract(ids)
            phone = self.asr.phone_featurizer.iextract(st.phones.text())
            out[s] = (st.packets * self.wav_buf_length / sr, " ".join(phone), "".join(text))
        for s in full:                          # in the slot's place, returned and not raised: the other streams go on
            out[s] = BeamStateOverflow("slot %d: more than max_text_frames = %d text frames in one stream (its search consumed "
                                       "nothing of this tick); close and reopen it" % (s, self.beam.max_frames))
        return out

    def send(self, audio):
        """{slot: float samples of any length} -> {slot: [(seconds_heard, phones, text), ...]}.  The samples are at the model's
        rate, or at the server's `input_rate`: then everything that arrived in this call goes through ONE resampler step for all
        its slots (a piece above max_input_packet: one step per max_input_packet samples) and what that emits joins the buffers."""
        out = {}
        if self.resampler is not None:
            audio = self._resampled(audio)
        for s, x in audio.items():
            st = self._stream(s)
            st.buf = np.concatenate([st.buf, np.asarray(x, np.float32).reshape(-1)])
            out[s] = []
        W = self.wav_buf_length
        while True:
            ready = {s: st.buf[:W] for s, st in self.streams.items() if len(st.buf) >= W}
            if not ready:
                break
            for s in ready:
                self.streams[s].buf = self.streams[s].buf[W:]
            for s, t in self.tick(ready).items():
                if t is not None:
                    out.setdefault(s, []).append(t)
        return out

    def _resampled(self, audio):
        """{slot: samples at input_rate} -> {slot: the samples at the model's rate that became final}"""
        rows = {s: np.asarray(x, np.float32).reshape(-1) for s, x in audio.items()}
        for s in rows:
            self._stream(s)
        out = {s: [] for s in rows}
        M, off = self.max_input_packet, 0
        while True:
            part = {s: x[off:off + M] for s, x in rows.items() if len(x) > off}
            if not part:
                break
            slots = sorted(part)
            for s, y in self.resampler.step(slots, [part[s] for s in slots]).items():
                out[s].append(y)
            off += M
        return {s: np.concatenate(v) if v else np.zeros(0, np.float32) for s, v in out.items()}

    def close(self, slot):
        """the buffered tail as the stream's short last packet -> its tuples; the slot is free afterwards.  With an input_rate
        the slot's resampler is flushed first: the outputs that waited for samples after the stream's end."""
        st = self._stream(slot)
        try:
            out = []
            if self.resampler is not None:
                st.buf = np.concatenate([st.buf, self.resampler.flush([slot])[slot]])
                W = self.wav_buf_length
                while len(st.buf) >= W:                  # the flush can complete a packet
                    pkt, st.buf = st.buf[:W], st.buf[W:]
                    t = self.tick({slot: pkt})[slot]
                    if t is not None:
                        out.append(t)
            if len(st.buf):
                t = self.tick({slot: st.buf})[slot]
                if t is not None:
                    out.append(t)
            return out
        finally:
            del self.streams[slot]
            self.free.append(slot)
