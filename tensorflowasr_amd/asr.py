"""`ASR`: the recogniser object of the reference's test_asr.py (:14-220), on the MI355X models of this package.

    from tensorflowasr_amd.config import UserConfig
    from tensorflowasr_amd.asr import ASR
    asr = ASR(UserConfig('configs/am_data.yml', 'configs/conformerS.yml'))
    phones, text = asr.stt('utt.wav')

Same construction (featurizers from `inp_config` / `tar_config` / `speech_config`, encoder / CTCDecoder / Translator
from `model_config`), same checkpoint directory convention (`<outdir>/{encoder,ctc_decoder,translator}-ckpt/
model_<step>.<ext>`, highest step wins; the reference's Keras `.h5` files, TensorFlow checkpoints and `.npz` files of
Keras-layout tensors are all read directly -- checkpoint.latest_checkpoint), same
outputs (`' '.join(phones), ''.join(text)`).  Everything between the waveform and the token ids runs through
libmi355asr.so; there is no CPU path."""
import logging
import os
import time

import numpy as np

from .featurizers import SpeechFeaturizer, TextFeaturizer
from .models import ConformerEncoder, CTCDecoder, StreamingConformerEncoder, Translator, ctc_forced_align, ctc_greedy_decode


def batch_items(items, sample_rates, load_wav, model_rate):
    """The items of an offline_stt_batch call (paths or 1-D waveforms) as 1-D arrays, and their rates: None (all at the model's
    rate), or per item None / the rate it will be resampled from on the device.  A path with a rate is read at the file's
    own rate, which has to be the stated one; an unsupported ratio is refused here, before anything runs."""
    if sample_rates is None:
        return [np.asarray(load_wav(w) if isinstance(w, (str, os.PathLike)) else w, np.float32).reshape(-1) for w in items], None
    from .featurizers import read_wav_native
    from .resample import ratio
    if len(sample_rates) != len(items):
        raise ValueError("%d items, %d sample rates" % (len(items), len(sample_rates)))
    waves, rates = [], []
    for w, r in zip(items, sample_rates):
        r = None if r is None or int(r) == model_rate else int(r)
        if isinstance(w, (str, os.PathLike)):
            if r is None:
                w = load_wav(w)
            else:
                path = w
                w, file_rate = read_wav_native(path)
                if file_rate != r:
                    raise ValueError("%s is a %d Hz file, sample_rates says %d" % (path, file_rate, r))
        w = np.asarray(w).reshape(-1)
        if r is None or w.dtype != np.int16:
            w = w.astype(np.float32, copy=False)
        if r is not None:
            ratio(r, model_rate)                       # an unsupported ratio: before anything runs
        waves.append(w)
        rates.append(r)
    return waves, rates


def cut_batches(waves, rates, model_rate, max_batch_samples, min_L=0):
    """Ragged batches of a list of waveforms: sorted by length (similar lengths together: less padding) and cut so that no
    batch holds more than max_batch_samples padded samples (B x its longest row, at least min_L; None: one batch).
    -> (n16: every item's samples at the model's rate -- its length, or the length of its resampled output; the batches as
    lists of item indices)"""
    from .resample import out_length, ratio
    n16 = [len(w) if rates is None or rates[i] is None else out_length(len(w), *ratio(rates[i], model_rate))
           for i, w in enumerate(waves)]
    order = sorted(range(len(waves)), key=lambda i: n16[i])
    batches, cur = [], []
    for i in order:
        L = max(min_L, max([n16[j] for j in cur] + [n16[i]]))
        if cur and max_batch_samples is not None and (len(cur) + 1) * L > max_batch_samples:
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return n16, batches


def batch_rows(waves, rates, idx, lens, W, resampler_for, device):
    """The [len(idx), W] batch of the items idx, zero padded: a host array when every row is at the model's rate, else a device
    tensor whose rows with a rate were resampled there -- one launch of resampler_for(rate) per distinct rate, the rows going
    into the tensor without passing over the host."""
    import torch
    x = np.zeros((len(idx), W), np.float32)
    groups = {}                                     # rate -> the rows of the batch to resample from it
    for r, i in enumerate(idx):
        if rates is None or rates[i] is None:
            x[r, :lens[r]] = waves[i]
        else:
            groups.setdefault(rates[i], []).append(r)
    if groups:
        x = torch.from_numpy(x).to(device)
        for rate, rows in sorted(groups.items()):
            src = [waves[idx[r]] for r in rows]
            n_in = np.array([len(w) for w in src], np.int32)
            # int16 PCM goes up as it is (the kernel converts, x / 32768) unless the rate's rows are mixed
            pcm = all(w.dtype == np.int16 for w in src)
            xin = np.zeros((len(rows), max(1, int(n_in.max()))), np.int16 if pcm else np.float32)
            for k, w in enumerate(src):
                xin[k, :len(w)] = w if pcm or w.dtype != np.int16 else w.astype(np.float32) / 32768.0
            y, _ = resampler_for(rate)(xin, n_in, out_pad=W)       # one launch per distinct rate
            x[torch.as_tensor(rows, device=x.device)] = y
    return x


class ASR:
    def __init__(self, config, device="cuda:0", load_checkpoint=True, verbose=False):
        self.running_config = config["running_config"]
        self.speech_config = config["speech_config"]
        self.model_config = config["model_config"]
        self.opt_config = config["optimizer_config"] if "optimizer_config" in config else None
        self.phone_featurizer = TextFeaturizer(config["inp_config"])
        self.text_featurizer = TextFeaturizer(config["tar_config"])
        self.speech_featurizer = SpeechFeaturizer(self.speech_config)
        self.chunk = self.speech_config["sample_rate"] * self.speech_config["streaming_bucket"]
        self.device = device
        self.verbose = verbose
        self.timings = {}
        self.compile(load_checkpoint)

    # test_asr.py:26-93
    def compile(self, load_checkpoint=True):
        mc, sc = self.model_config, self.speech_config
        enc_kw = dict(dmodel=mc["dmodel"], reduction_factor=mc["reduction_factor"], num_blocks=mc["num_blocks"],
                      head_size=mc["head_size"], num_heads=mc["num_heads"], kernel_size=mc["kernel_size"],
                      fc_factor=mc["fc_factor"], dropout=mc["dropout"], add_wav_info=sc["add_wav_info"],
                      sample_rate=sc["sample_rate"], n_mels=sc["num_feature_bins"],
                      mel_layer_type=sc["mel_layer_type"], mel_layer_trainable=sc["mel_layer_trainable"],
                      stride_ms=sc["stride_ms"], device=self.device)
        if not sc["streaming"]:
            self.encoder = ConformerEncoder(name="conformer_encoder", **enc_kw)
        else:
            assert "Streaming" in mc["name"], "am_data.yml set streaming=True,But model.yml is OfflineCTC"
            self.encoder = StreamingConformerEncoder(name="stream_conformer_encoder", **enc_kw)
            self.encoder.add_chunk_size(
                chunk_size=int(sc["streaming_bucket"] * sc["sample_rate"]), mel_size=sc["num_feature_bins"],
                hop_size=int(sc["stride_ms"] * sc["sample_rate"] // 1000) * mc["reduction_factor"])
            self.encoder.set_inference_func()
        self.ctc_model = CTCDecoder(num_classes=self.phone_featurizer.num_classes, dmodel=mc["dmodel"],
                                    num_blocks=mc["ctcdecoder_num_blocks"], head_size=mc["head_size"],
                                    num_heads=mc["num_heads"], kernel_size=mc["ctcdecoder_kernel_size"],
                                    dropout=mc["ctcdecoder_dropout"], fc_factor=mc["ctcdecoder_fc_factor"],
                                    device=self.device)
        self.translator = Translator(inp_classes=self.phone_featurizer.num_classes,
                                     tar_classes=self.text_featurizer.num_classes, dmodel=mc["dmodel"],
                                     num_blocks=mc["translator_num_blocks"], head_size=mc["head_size"],
                                     num_heads=mc["num_heads"], kernel_size=mc["translator_kernel_size"],
                                     dropout=mc["translator_dropout"], fc_factor=mc["translator_fc_factor"],
                                     device=self.device)
        self.encoder._build()
        self.ctc_model._build()
        self.translator._build()
        self.translator.set_inference_func()
        if load_checkpoint:
            self.load_checkpoint()
        if self.verbose:
            self.encoder.summary(line_length=100)
            self.ctc_model.summary(line_length=100)
            self.translator.summary(line_length=100)

    # test_asr.py:95-114
    @staticmethod
    def _latest(checkpoint_dir):
        from .checkpoint import latest_checkpoint
        return latest_checkpoint(checkpoint_dir)

    def load_checkpoint(self):
        for sub, model, by_name in (("encoder-ckpt", self.encoder, True), ("ctc_decoder-ckpt", self.ctc_model, False),
                                    ("translator-ckpt", self.translator, False)):
            path = self._latest(os.path.join(self.running_config["outdir"], sub))
            model.load_weights(path, by_name=by_name)
            logging.info("%s load at %s", sub.replace("-ckpt", ""), path)

    # ---- decoding helpers --------------------------------------------------------------------------------
    def _phone_ids(self, enc_outputs):
        """softmax + tf.keras.backend.ctc_decode(greedy) + clip(-1 -> 0) (test_asr.py:196-200): per-frame argmax
        inside the CTC head kernel, merge/blank-drop on the device."""
        _, frame_ids = self.ctc_model(enc_outputs, training=False, return_argmax=True, return_logits=False)
        # tf.keras.backend.ctc_decode: the blank is the LAST class (num_classes - 1), independent of `blank_at_zero`
        ids, lens = ctc_greedy_decode(frame_ids, None, blank=self.phone_featurizer.num_classes - 1)
        # ctc_decode's dense output is as wide as the longest decoded sequence of the batch, padded with -1; the
        # width matters: the Translator has no mask, padded positions reach their neighbours through its ConvModule
        width = int(lens.max().item())
        return ids[:, :width].clamp_(min=0).contiguous(), lens

    def _finish(self, ctc_decode_row, translator_row):
        ctc_result = [int(n) for n in ctc_decode_row if n != 0]
        txt_result = []
        for n in translator_row:
            n = int(n)
            if n != 0:
                txt_result.append(n)
            if n == self.text_featurizer.endid():
                break
        phone = self.phone_featurizer.iextract(ctc_result)
        txt = self.text_featurizer.iextract(txt_result)
        return " ".join(phone), "".join(txt)

    # test_asr.py:186-219
    def offline_stt(self, wav_path):
        return self.offline_stt_wave(self.speech_featurizer.load_wav(wav_path))

    def offline_stt_wave(self, data):
        """offline_stt on an in-memory 1-D waveform at the model's sample rate (one utterance)."""
        input_wav = np.asarray(data, np.float32).reshape([1, -1, 1])
        t0 = time.time()
        enc_outputs = self.encoder(input_wav, training=False)
        ctc_decode, _ = self._phone_ids(enc_outputs)
        _, translator_out = self.translator([ctc_decode, enc_outputs], training=False, return_argmax=True, return_logits=False)
        ctc_row, txt_row = ctc_decode[0].cpu().numpy(), translator_out[0].cpu().numpy()
        self.timings["offline_stt"] = time.time() - t0
        return self._finish(ctc_row, txt_row)

    def align(self, wav_or_path, phones):
        """When each phone was spoken: encoder -> CTC logits -> forced alignment (models.ctc_forced_align) of `phones` (a
        space-separated string, or a list of tokens or of ids) to the utterance.  -> [(phone, start_s, end_s), ...]: start_s =
        first frame x the frame period, end_s = (last frame + 1) x the frame period, the period being reduction_factor x
        stride_ms (40 ms for the shipped configurations).  Raises ValueError when the utterance has too few frames for them.
        The score of the alignment and its frames are kept in self.last_alignment (score, spans [U, 2])."""
        data = self.speech_featurizer.load_wav(wav_or_path) if isinstance(wav_or_path, (str, os.PathLike)) else wav_or_path
        tokens = phones.split() if isinstance(phones, str) else list(phones)
        ids = [int(t) if isinstance(t, (int, np.integer)) else self.phone_featurizer.token_to_index[t] for t in tokens]
        enc_outputs = self.encoder(np.asarray(data, np.float32).reshape([1, -1, 1]), training=False)
        logits = self.ctc_model(enc_outputs, training=False)
        # the blank is the LAST class, as tf.keras.backend.ctc_decode and ctc_batch_cost have it (see _phone_ids)
        _, spans, score = ctc_forced_align(logits, np.asarray([ids], np.int32).reshape(1, len(ids)),
                                           blank=self.phone_featurizer.num_classes - 1)
        spans, score = spans[0].cpu().numpy(), float(score[0].item())
        if not np.isfinite(score):
            raise ValueError("%d phones cannot be aligned to %d frames" % (len(ids), logits.shape[1]))
        self.last_alignment = (score, spans)
        period = self.model_config["reduction_factor"] * self.speech_config["stride_ms"] / 1000.0
        return [(self.phone_featurizer.index_to_token[i], float(a) * period, float(b + 1) * period)
                for i, (a, b) in zip(ids, spans)]

    def _resampler(self, rate):
        """the device resampler from `rate` to the model's rate (one per rate, kept)"""
        from .resample import Resampler
        cache = self.__dict__.setdefault("_resamplers", {})
        if rate not in cache:
            cache[rate] = Resampler(rate, self.speech_config["sample_rate"], device=self.device)
        return cache[rate]

    def offline_stt_batch(self, items, max_batch_samples=None, sample_rates=None, augment=None):
        """offline_stt_wave for every item of a list -- paths or 1-D waveforms -- in ragged batches: one encoder, CTC and
        Translator call per batch (mi355asr_*_ragged), each row computed as if alone.  Returns [(phones, text), ...] in the
        order of `items`, what [offline_stt_wave(w) for w in items] returns.  max_batch_samples bounds B x Lmax of a batch
        (the workspace grows with it, counted in samples at the model's rate); None: one batch.  Offline Melspectrogram encoders
        of dmodel 144 only.

        sample_rates: one rate per item, None for an item that is at the model's rate already (the default for all).  An
        array item with a rate (float32, or int16 PCM) is resampled on the device from that rate; a path item with a rate is
        read at the file's own rate (featurizers.read_wav_native), which has to be the stated one, and resampled on the
        device.  Items of one rate in one batch share one resampler launch (resample.Resampler), and the resampled rows go
        into the batch's device tensor without passing over the host.

        augment: a callable (x [B, W], lengths int32 [B]) -> (y [B, W'] float32 on the device, out_len int32 [B] on the device),
        such as an augment.FarField: applied to every batch on the device, after loading and resampling and before the
        encoder, which then sees out_len[b] samples of row b.  None (the default): nothing is applied."""
        waves, rates = batch_items(items, sample_rates, self.speech_featurizer.load_wav, int(self.speech_config["sample_rate"]))
        return self._stt_batch(waves, rates, max_batch_samples, augment)

    def _stt_batch(self, waves, rates, max_batch_samples, augment=None):
        """offline_stt_batch on 1-D arrays; rates: None, or per item None / the rate it is resampled from on the device"""
        import torch
        mc, sc = self.model_config, self.speech_config
        # the length-aware attention kernels need more than 16 rows per utterance: pad the batch's L (and U) beyond that
        min_L = 16 * mc["reduction_factor"] * int(sc["stride_ms"] * sc["sample_rate"] // 1000) + 1
        out = [None] * len(waves)
        n16, batches = cut_batches(waves, rates, int(sc["sample_rate"]), max_batch_samples, min_L)
        blank = self.phone_featurizer.num_classes - 1
        for idx in batches:
            lens = np.array([n16[i] for i in idx], np.int32)
            x = batch_rows(waves, rates, idx, lens, max(min_L, int(lens.max())), self._resampler, self.device)
            if augment is not None:
                x, out_len = augment(x, lens)
                lens = out_len.cpu().numpy().astype(np.int32)
                if x.shape[1] < min_L:
                    x = torch.nn.functional.pad(x, (0, min_L - x.shape[1]))
            enc, enc_len = self.encoder(x, training=False, lengths=lens)
            _, frame_ids = self.ctc_model(enc, training=False, return_argmax=True, return_logits=False, lengths=enc_len)
            ids, tok = ctc_greedy_decode(frame_ids, enc_len, blank=blank)
            tok_h = tok.cpu().numpy()
            U = max(17, int(tok_h.max()))
            ids = ids[:, :U].clamp_(min=0).contiguous()
            # an utterance with nothing decoded gives an empty Translator row alone; here it rides along as one token
            _, tr = self.translator([ids, enc], training=False, return_argmax=True, return_logits=False,
                                    token_lengths=torch.from_numpy(np.maximum(tok_h, 1).astype(np.int32)), enc_lengths=enc_len)
            ids_h, tr_h = ids.cpu().numpy(), tr.cpu().numpy()
            for r, i in enumerate(idx):
                n = int(tok_h[r])
                out[i] = self._finish(ids_h[r, :n], tr_h[r, :n])
        return out

    # test_asr.py:116-164
    def stream_stt(self, wav_path):
        import torch
        data = self.speech_featurizer.load_wav(wav_path)
        enc_outputs, ctc_row, txt_row = None, [], []
        for i in range(9999):
            s = i * self.chunk
            e = s + self.chunk
            if s >= len(data):
                break
            input_wav = data[int(s):int(e)]
            if len(input_wav) < int(self.chunk):      # the reference's tf.function pads nothing and would fail on a
                input_wav = np.pad(input_wav, (0, int(self.chunk) - len(input_wav)))   # short tail: zero-pad it
            enc_output = self.encoder.inference(input_wav.reshape([1, -1, 1]))
            enc_outputs = enc_output if enc_outputs is None else torch.cat((enc_outputs, enc_output), 1)
            ctc_decode, _ = self._phone_ids(enc_outputs)           # global CTC over everything heard so far
            ctc_row = ctc_decode[0].cpu().numpy()
            ctc_result = [int(n) for n in ctc_row if n != 0] + [0] * 10
            _, tr = self.translator([np.array([ctc_result], "int32"), enc_outputs], return_argmax=True, return_logits=False)
            txt_row = tr[0].cpu().numpy()
        return self._finish(ctc_row, txt_row)

    # ---- Inference/PythonInference/asr/src/asr.py: the two calls of the streaming session ---------------------------
    def extract_feature(self, wav):
        """the streaming encoder on a piece of audio -> enc [1, T, dmodel] on the device.  A piece that is not a whole
        number of chunks is zero-padded to one, the rule stream_stt uses for its last piece (the reference's ONNX encoder
        takes any length, its TF function does not)."""
        wav = np.asarray(wav, np.float32).reshape(-1)
        chunk = int(self.chunk)
        n = max(1, -(-len(wav) // chunk))
        if len(wav) < n * chunk:
            wav = np.pad(wav, (0, n * chunk - len(wav)))
        return self.encoder.inference(wav.reshape([1, -1, 1]))

    def _text_of(self, translator_row):
        out = []
        for n in translator_row:
            n = int(n)
            if n == self.text_featurizer.endid():
                break
            if n != 0:
                out.append(n)
        return "".join(self.text_featurizer.iextract(out))

    def decode(self, enc_features):
        """the encoder outputs of a sentence so far -> text: global CTC decoder over all of them, greedy collapse, ten zero
        tokens appended, Translator, text up to the end id"""
        import torch
        if not len(enc_features):
            return ""
        enc = enc_features[0] if len(enc_features) == 1 else torch.cat(list(enc_features), 1)
        _, frame_ids = self.ctc_model(enc, training=False, return_argmax=True, return_logits=False)
        ids, lens = ctc_greedy_decode(frame_ids, None, blank=self.phone_featurizer.num_classes - 1)
        n = int(lens[0].item())
        tokens = torch.zeros((1, n + 10), dtype=torch.int32, device=ids.device)
        tokens[:, :n] = ids[:, :n].clamp(min=0)
        _, tr = self.translator([tokens, enc], training=False, return_argmax=True, return_logits=False)
        return self._text_of(tr[0].cpu().numpy())

    def decode_batch(self, enc, enc_lengths, enc_lengths_host=None):
        """decode() for a ragged batch: enc [M, T, dmodel] (T >= 17) holding enc_lengths[b] frames per row (int32 on the device)
        -> [text]: one ragged CTCDecoder call, one greedy collapse, one ragged Translator call"""
        import torch
        _, frame_ids = self.ctc_model(enc, training=False, return_argmax=True, return_logits=False, lengths=enc_lengths)
        ids, tok = ctc_greedy_decode(frame_ids, enc_lengths, blank=self.phone_featurizer.num_classes - 1)
        tl = tok.cpu().numpy().astype(np.int32) + 10
        U = max(17, int(tl.max()))
        tokens = torch.zeros((enc.shape[0], U), dtype=torch.int32, device=ids.device)
        w = min(U, ids.shape[1])
        tokens[:, :w] = ids[:, :w].clamp(min=0)           # the collapse pads with -1: zeros, the ten appended ones among them
        _, tr = self.translator([tokens, enc], training=False, return_argmax=True, return_logits=False,
                                token_lengths=torch.from_numpy(tl), enc_lengths=enc_lengths)
        tr = tr.cpu().numpy()
        return [self._text_of(tr[b, :tl[b]]) for b in range(enc.shape[0])]

    def stt(self, wav_path):
        if self.speech_config["streaming"]:
            return self.stream_stt(wav_path)
        return self.offline_stt(wav_path)

    # test_asr.py:166-185 (host-side equivalents the reference keeps next to the TF path)
    @staticmethod
    def remove_blank(labels, blank=0):
        new_labels, previous = [], None
        for l in labels:
            if l != previous:
                new_labels.append(l)
                previous = l
        return [l for l in new_labels if l != blank]

    def greedy_decode(self, y, blank=1331):
        return self.remove_blank(np.argmax(y, axis=1), blank)
