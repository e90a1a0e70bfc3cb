"""Batch evaluation harness: the reference's `AMTester` (asr/tester/am_tester.py:13-183, base_tester.py:19-95),
its list-file eval loader conventions (asr/dataloaders/am_dataloader.py:118-227) and its error-rate arithmetic
(utils/xer.py:12-36, 211-220), on the MI355X models of this package.

    tester = AMTester(UserConfig(data_yml, model_yml))
    tester.set_datasets(EvalList(config, tester.speech_featurizer, tester.phone_featurizer, tester.text_featurizer))
    metrics = tester.run()      # {'phone_ser', 'phone_cer', 'txt_ser', 'txt_cer', 'phone_s_i_d', 'trans_s_i_d', ...}

List file lines are `wav_path<TAB>text` as in the reference; the phone labels come from `text_to_vocab(text)`
(the reference uses pypinyin, am_dataloader.py:69-79 -- pass your own callable) or from an optional third
tab-separated column of space-separated phone tokens."""
import logging
import os

import numpy as np

from .asr import ASR
from .models import ctc_greedy_decode, ctc_loss


# ---- utils/xer.py ---------------------------------------------------------------------------------------------
def levenshtein(u, v):
    """Edit distance of `v` (hypothesis) against `u` (reference) with the (SUB, DEL, INS) counts of one optimal
    alignment.  Tie-breaking as utils/xer.py:12-36: a substitution/match step is preferred over a deletion, a
    deletion over an insertion -- the S/I/D split (not the distance) depends on it."""
    n, m = len(u), len(v)
    cost = list(range(m + 1))
    ops = [(0, 0, j) for j in range(m + 1)]
    for x in range(1, n + 1):
        new_cost = [x] + [0] * m
        new_ops = [(0, x, 0)] + [None] * m
        ux = u[x - 1]
        for y in range(1, m + 1):
            neq = int(ux != v[y - 1])
            c_sub, c_del, c_ins = cost[y - 1] + neq, cost[y] + 1, new_cost[y - 1] + 1
            best = min(c_sub, c_del, c_ins)
            new_cost[y] = best
            if best == c_sub:
                s, d, i = ops[y - 1]
                new_ops[y] = (s + neq, d, i)
            elif best == c_del:
                s, d, i = ops[y]
                new_ops[y] = (s, d + 1, i)
            else:
                s, d, i = new_ops[y - 1]
                new_ops[y] = (s, d, i + 1)
        cost, ops = new_cost, new_ops
    return cost[m], ops[m]


def wer(r, h):
    """utils/xer.py:211-220: ((S+I+D)/N, S, D, I) for reference `r`, hypothesis `h` (sequences of tokens/ids)."""
    _, (s, d, i) = levenshtein(r, h)
    return (s + i + d) / len(r), s, d, i


class _Mean:
    """tf.keras.metrics.Mean: running mean of the values given to update_state."""

    def __init__(self):
        self.reset_states()

    def reset_states(self):
        self.total, self.count = 0.0, 0

    def update_state(self, v):
        self.total += float(v)
        self.count += 1

    def result(self):
        return self.total / self.count if self.count else 0.0


def update_from_device_scores(scored, nums, ser, cer):
    """`scored` = (result i32 [B, 4], lengths i32 [B, 2]) of scoring.EditDistance: what the host loops of the testers do with
    `wer` per utterance -- nums = [n, s, i, d] accumulators, `ser` 1 for a non-zero distance, `cer` the running rate -- in
    utterance order.  An empty reference raises ZeroDivisionError, as `wer` does."""
    import torch
    for dist, s, d, i, n, _ in torch.cat(scored, 1).cpu().tolist():
        if n == 0:
            raise ZeroDivisionError("division by zero: empty reference")
        nums[0] += n; nums[1] += s; nums[2] += i; nums[3] += d
        ser.update_state(1 if dist else 0)
        cer.reset_states()
        cer.update_state(sum(nums[1:]) / (nums[0] + 1e-6))


# ---- asr/dataloaders/am_dataloader.py:118-227 (eval half) -----------------------------------------------------
class EvalList:
    """Iterates a test list in batches the way `AM_DataLoader.eval_data_generator` builds them:
    skip unreadable / shorter than 400 samples / longer than `wav_max_duration`; offline: peak-normalise
    `x / max|x|`, `in_len = len // (reduction * hop)`, zero-pad to the batch maximum; streaming: raw samples, padded
    to the next multiple of the block, `in_len` counted in whole blocks (13 frames each at 0.5 s)."""

    def __init__(self, config, speech_featurizer, phone_featurizer, text_featurizer, test_list=None,
                 text_to_vocab=None, batch_size=None):
        self.speech_config = config["speech_config"]
        self.speech_featurizer, self.phone_featurizer, self.text_featurizer = speech_featurizer, phone_featurizer, text_featurizer
        self.batch = batch_size or config["running_config"]["batch_size"]
        self.streaming = self.speech_config["streaming"]
        self.chunk = int(self.speech_config["sample_rate"] * self.speech_config["streaming_bucket"])
        self.text_to_vocab = text_to_vocab
        path = test_list or self.speech_config["eval_list"]
        with open(path, encoding="utf-8") as f:
            self.test_list = [l.strip() for l in f.readlines() if l.strip() != ""]
        self.test_offset = 0

    def eval_per_epoch_steps(self):
        return len(self.test_list) // self.batch

    @staticmethod
    def only_chinese(word):
        return "".join(ch for ch in word if "一" <= ch <= "鿿")

    @staticmethod
    def check_valid(txt, vocab_list):
        if len(txt) == 0:
            return False
        for n in txt:
            if n not in vocab_list:
                return n
        return True

    def _phones_of(self, fields, txt):
        if len(fields) > 2:
            return fields[2].split()
        if self.text_to_vocab is None:
            raise ValueError("list line has no phone column and no text_to_vocab callable was given "
                             "(the reference derives phones with pypinyin, which this image does not ship)")
        return self.text_to_vocab(txt)

    def eval_data_generator(self):
        sc = self.speech_config
        reduce = sc["reduction_factor"] * (self.speech_featurizer.sample_rate / 1000) * sc["stride_ms"]
        feats, input_length, phones, phones_length, txts = [], [], [], [], []
        max_input = 0
        for _ in range(self.batch * 10):
            line = self.test_list[self.test_offset]
            self.test_offset += 1
            if self.test_offset > len(self.test_list) - 1:
                self.test_offset = 0
            fields = line.strip().split("\t")
            wp, txt = fields[0], fields[1]
            try:
                data = self.speech_featurizer.load_wav(wp)
            except Exception:
                logging.info("%s load data failed,skip", wp)
                continue
            if len(data) < 400:
                continue
            if len(data) > self.speech_featurizer.sample_rate * sc["wav_max_duration"]:
                logging.info("%s duration out of wav_max_duration(%s),skip", wp, sc["wav_max_duration"])
                continue
            if sc.get("only_chinese"):
                txt = self.only_chinese(txt)
            if not self.streaming:
                feat = data / np.abs(data).max()
                in_len = len(feat) // reduce
            else:
                feat = data
                in_len = len(feat) // self.chunk + (1 if len(feat) % self.chunk != 0 else 0)
                chunk_times = self.chunk // reduce + (1 if self.chunk % reduce != 0 else 0)
                in_len *= chunk_times
            py = self._phones_of(fields, txt)
            if self.check_valid(py, self.phone_featurizer.vocab_array) is not True:
                logging.info(" %s phones not all in tokens,continue", txt)
                continue
            if self.check_valid(txt, self.text_featurizer.vocab_array) is not True:
                logging.info(" %s text not all in tokens,continue", txt)
                continue
            phone_feature = self.phone_featurizer.extract(py)
            text_feature = self.text_featurizer.extract(list(txt)) + [self.text_featurizer.endid()]
            if in_len < len(phone_feature):
                logging.info("%s feature length < phone length,continue", wp)
                continue
            max_input = max(max_input, len(feat))
            feats.append(feat)
            input_length.append(in_len)
            phones.append(phone_feature)
            txts.append(text_feature)
            phones_length.append(len(phone_feature))
            if len(feats) == self.batch:
                break
        if not feats:
            raise RuntimeError("no usable utterance in the evaluation list")
        if self.streaming:
            # am_dataloader.py:198-209 rounds max_input up to the next block boundary TWICE (before each of its two
            # pad_signal calls), so every streaming batch carries one extra all-zero block; the CTCDecoder and the
            # Translator attend over all frames without a mask, so that block is part of the reference's numbers
            max_input = max_input // self.chunk * self.chunk + self.chunk
            max_input = max_input // self.chunk * self.chunk + self.chunk
            chunk_times = self.chunk // reduce + (1 if self.chunk % reduce != 0 else 0)
            input_length = np.clip(input_length, 0, (max_input // self.chunk) * chunk_times)
        x = self.speech_featurizer.pad_signal(feats, max_input)[..., None]

        def pad(seqs, value):
            out = np.full((len(seqs), max(len(s) for s in seqs)), value, np.int32)
            for i, s in enumerate(seqs):
                out[i, :len(s)] = s
            return out
        return (x.astype(np.float32), np.array(input_length, "int32"), pad(phones, self.phone_featurizer.pad),
                np.array(phones_length, "int32"), pad(txts, self.text_featurizer.pad))

    def __iter__(self):
        while True:
            yield self.eval_data_generator()


# ---- asr/tester/am_tester.py ----------------------------------------------------------------------------------
class AMTester(ASR):
    """`AMTester(config)`: same models / checkpoints as `ASR`, evaluated over batches
    `(features [B,L,1], input_length [B], phone_labels [B,P], phone_label_length [B], text_labels [B,Q])`.
    with_ctc_loss=True adds the `ctc_loss` metric of CTCTrainer._eval_step (asr/trainer/ctc_runners.py:125-150): the mean of
    tf.keras.backend.ctc_batch_cost(phone_labels, softmax(logits), input_length, phone_label_length) over the utterances.
    with_trainer_metrics=True adds the other three numbers of that step, updated as it updates them: `ctc_acc` (one value per
    utterance), `translate_loss` (the mean of the cross-entropy of the Translator logits over all B x min(U, Q) elements) and
    `translate_acc` (one scalar per step) -- from the logits of the one Translator call the step makes (losses.py); the inputs
    of the last step are kept in `last_trainer_inputs`.  The decoded ids and their scoring are the same either way."""

    def __init__(self, config, device="cuda:0", load_checkpoint=True, with_ctc_loss=False, device_scoring=False,
                 with_trainer_metrics=False):
        self.config = config
        self.with_ctc_loss = bool(with_ctc_loss)
        self.with_trainer_metrics = bool(with_trainer_metrics)
        self.device_scoring = bool(device_scoring)      # True: scoring.EditDistance, one call per id stream (same results())
        self.eval_metrics = {k: _Mean() for k in ("phone_ser", "phone_cer", "txt_ser", "txt_cer")}
        if self.with_ctc_loss:
            self.eval_metrics["ctc_loss"] = _Mean()
        if self.with_trainer_metrics:
            self.eval_metrics.update((k, _Mean()) for k in ("ctc_acc", "translate_loss", "translate_acc"))
        self.last_trainer_inputs = None
        self.ctc_nums = [0, 0, 0, 0]          # n, s, i, d
        self.translator_nums = [0, 0, 0, 0]
        self.steps, self.all_steps = 0, 0
        self.eval_datasets = None
        super().__init__(config, device=device, load_checkpoint=load_checkpoint)
        if self.device_scoring:
            from .scoring import EditDistance
            self.scorer = EditDistance(device)
        self.output_file_path = os.path.join(self.running_config["outdir"], "test.tsv")

    def set_all_steps(self, all_steps):
        self.all_steps = all_steps

    def set_datasets(self, evaldataset):
        self.eval_datasets = evaldataset

    def finished(self):
        return self.steps >= self.all_steps

    @staticmethod
    def _strip(seq, values):
        return [int(t) for t in seq if int(t) not in values]

    def _eval_step(self, batch):
        """am_tester.py:34-89."""
        features, input_length, phone_labels, phone_label_length, tar_label = batch
        enc_output = self.encoder(features, training=False)
        logits, frame_ids = self.ctc_model(enc_output, training=False, return_argmax=True, return_logits=self.with_ctc_loss)
        if self.with_ctc_loss:
            # ctc_batch_cost on softmax(logits): the logits entry of the loss takes the softmax inside its row kernel
            for v in ctc_loss(logits, phone_labels, input_length, phone_label_length).cpu().numpy():
                self.eval_metrics["ctc_loss"].update_state(v)
        # tf.keras.backend.ctc_decode treats the LAST class as the blank whatever `blank_at_zero` says (am_tester.py:38-40)
        ids, lens = ctc_greedy_decode(frame_ids, input_length, blank=self.phone_featurizer.num_classes - 1)
        ctc_decode = ids[:, :max(int(lens.max().item()), 1)].clamp_(min=0).contiguous()
        translator_logits, translator_out = self.translator([ctc_decode, enc_output], training=False, return_argmax=True,
                                                            return_logits=self.with_trainer_metrics)
        if self.with_trainer_metrics:
            self._trainer_metrics(phone_labels, ctc_decode, tar_label, translator_logits)
        pad = self.phone_featurizer.pad
        tpad, tend = self.text_featurizer.pad, self.text_featurizer.endid()
        if self.device_scoring:
            self._score_on_device(ctc_decode, phone_labels, (pad,), None, self.ctc_nums, "phone_ser", "phone_cer")
            self._score_on_device(translator_out, tar_label, (tpad, tend), 1, self.translator_nums, "txt_ser", "txt_cer")
            return
        ctc_decode, translator_out = ctc_decode.cpu().numpy(), translator_out.cpu().numpy()
        for hyp, ref in zip(ctc_decode, np.asarray(phone_labels)):
            i, j = self._strip(hyp, (pad,)), self._strip(ref, (pad,))
            _, ws, wd, wi = wer(j, i)
            self.ctc_nums[0] += len(j); self.ctc_nums[1] += ws; self.ctc_nums[2] += wi; self.ctc_nums[3] += wd
            self.eval_metrics["phone_ser"].update_state(0 if i == j else 1)
            self.eval_metrics["phone_cer"].reset_states()
            self.eval_metrics["phone_cer"].update_state(sum(self.ctc_nums[1:]) / (self.ctc_nums[0] + 1e-6))
        for hyp, ref in zip(translator_out, np.asarray(tar_label)):
            hyp = [int(t) for t in hyp]
            if 1 in hyp:
                hyp = hyp[:hyp.index(1)]
            i, j = self._strip(hyp, (tpad, tend)), self._strip(ref, (tpad, tend))
            _, ws, wd, wi = wer(j, i)
            self.translator_nums[0] += len(j); self.translator_nums[1] += ws
            self.translator_nums[2] += wi; self.translator_nums[3] += wd
            self.eval_metrics["txt_ser"].update_state(0 if i == j else 1)
            self.eval_metrics["txt_cer"].reset_states()
            self.eval_metrics["txt_cer"].update_state(sum(self.translator_nums[1:]) / (self.translator_nums[0] + 1e-6))

    def _trainer_metrics(self, phone_labels, ctc_decode, tar_label, translator_logits):
        """ctc_runners.py:144-150: ctc_acc masks with the TEXT featurizer's pad, as the reference does."""
        from .losses import ctc_acc, translate_metrics
        mean, acc = translate_metrics(tar_label, translator_logits)
        accs = ctc_acc(phone_labels, ctc_decode, pad=self.text_featurizer.pad)
        self.last_trainer_inputs = dict(phone_labels=phone_labels, ctc_decode=ctc_decode, tar_label=tar_label,
                                        translator_logits=translator_logits)
        for v in accs.cpu().numpy():
            self.eval_metrics["ctc_acc"].update_state(v)
        self.eval_metrics["translate_loss"].update_state(mean.item())
        self.eval_metrics["translate_acc"].update_state(acc.item())

    def _score_on_device(self, hyp, ref, drop, stop, nums, ser, cer):
        """One scoring call for an id stream whose hypotheses stay on the device; the accumulators and metrics are then updated
        in utterance order from one [B, 6] copy, as the host loop of _eval_step updates them."""
        update_from_device_scores(self.scorer(ref, hyp, drop_ref=drop, drop_hyp=drop, hyp_stop=stop), nums,
                                  self.eval_metrics[ser], self.eval_metrics[cer])

    def results(self):
        r = {k: v.result() for k, v in self.eval_metrics.items()}
        r["phone_s_i_d"] = "{}_{}_{}".format(*self.ctc_nums[1:])
        r["trans_s_i_d"] = "{}_{}_{}".format(*self.translator_nums[1:])
        r["steps"] = self.steps
        return r

    def _eval_batches(self):
        for batch in self.eval_datasets:
            self._eval_step(batch)
            self.steps += 1
            logging.info("[Eval] [Step %d] %s", self.steps, self.results())
            if self.finished():
                break

    def run(self):
        if self.eval_datasets is None:
            raise RuntimeError("call set_datasets(...) first")
        if not self.all_steps:
            self.set_all_steps(max(self.eval_datasets.eval_per_epoch_steps(), 1)
                               if hasattr(self.eval_datasets, "eval_per_epoch_steps") else 1)
        self._eval_batches()
        return self.results()


class VADTester:
    """What `VADTrainer._eval_step` (vad/trainer/vad_trainer.py:76-84) keeps for the online VAD model, on the GPU: per step
    vad_loss = one_loss + zero_loss of mask_loss on the speech logits, wav_loss = the multi-resolution STFT loss between the
    clean waveform and the voice-mask head's output, vad_acc = binary_accuracy (the raw logit against the threshold), plus the
    binary F1 from the same counts.  The reference's own VadTester cannot run as written (it reads
    running_config['voice_thread'], which no config has, and calls .result of None), so F1 is the ordinary
    2 TP / (2 TP + FP + FN) and the reference does not pin it.

        tester = VADTester(VAD().load_saved_model(path))
        for x, vad_label, wav_label in batches:          # [B, T, 80], [B, T, 1], [B, T, 80] at 8 kHz, as the dataloader yields
            tester.update(x, vad_label, wav_label)
        tester.results()                                  # {'vad_loss', 'wav_loss', 'vad_acc', 'f1'}: the means over the steps

    The step values stay on the device; `results` is the one place that copies to the host."""

    def __init__(self, vad, threshold=0.5, stft_loss=None):
        from . import losses
        self.vad = vad
        self.threshold = float(threshold)
        self.stft_loss = stft_loss if stft_loss is not None else losses.MultiResolutionSTFTLoss(device=vad.device)
        self._losses = losses
        self.reset()

    def reset(self):
        self._steps = {"vad_loss": [], "wav_loss": [], "vad_acc": [], "f1": []}

    def update(self, x, vad_label, wav_label, lengths=None):
        """x [B, T, 80] noisy 8 kHz frames, vad_label [B, T, 1] (or [B, T]) in {0, 1}, wav_label [B, T, 80] clean frames;
        `lengths`: valid frames per row (None: all T).  -> this step's values as device scalars."""
        import torch
        xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        if xt.dim() != 3:
            raise ValueError("x is [B, T, 80] (got shape %s)" % (tuple(xt.shape),))
        B, T, frame = xt.shape
        samples = None if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(B) * frame
        enhanced, logits = self.vad.enhance(xt.reshape(B, T * frame), lengths=samples, sample_rate=8000)
        one, zero = self._losses.vad_mask_loss(vad_label, logits, lengths=lengths)
        m = self._losses.vad_metrics(vad_label, logits, threshold=self.threshold, lengths=lengths)
        wav = self.stft_loss(wav_label, enhanced, lengths=samples)
        step = {"vad_loss": one + zero, "wav_loss": wav, "vad_acc": m["acc"], "f1": m["f1"]}
        for k, v in step.items():
            self._steps[k].append(v)
        return step

    def results(self):
        import torch
        return {k: float(torch.stack(v).to(torch.float64).mean().item()) if v else float("nan") for k, v in self._steps.items()}


class PuncTester:
    """The reference's PuncTester (punc_recover/tester/punc_tester.py) and the eval half of PuncTrainer
    (punc_recover/trainer/punc_trainer.py:77-90) for the punctuation model, on the GPU: per step acc = classes_acc (the one metric
    the reference's tester keeps; the trainer calls it bd_acc), bd_loss = the batch mean of classes_loss, and, when the BERT
    teacher's features are given, feature_map_loss = the batch mean of bert_feature_loss.

        tester = PuncTester(Punc(config).load_onnx(path))
        for ids, labels, features in batches:            # [B, T] ids (0 = padding), [B, T] classes, [B, T, 768] or None
            tester.update(ids, labels, features)
        tester.results()                                  # {'acc', 'bd_loss', 'feature_map_loss'}: the means over the steps

    One `Punc.heads` launch per step.  `heads` checks the ids on the host before it launches (their range, and that no 0 stands in
    front of a non-zero id), which waits for the stream as `Punc.forward` does; the step values themselves stay on the device until
    `results` copies them."""

    def __init__(self, punc):
        from . import losses
        self.punc = punc
        self._losses = losses
        self.reset()

    def reset(self):
        self._steps = {"acc": [], "bd_loss": [], "feature_map_loss": []}

    def update(self, ids, labels, features=None):
        """ids int [B, T] with 0 as padding behind each sentence (the lengths follow from it, as creat_mask has it), labels int
        [B, Q], features f32 [B, T1, 768] or None -> this step's values as device scalars."""
        logits, feature = self.punc.heads(ids, want_feature=features is not None)
        loss, _, acc, _ = self._losses._punc_classes_call(labels, logits)
        step = {"acc": acc, "bd_loss": loss.mean()}
        if features is not None:
            step["feature_map_loss"] = self._losses.bert_feature_loss(features, feature).mean()
        for k, v in step.items():
            self._steps[k].append(v)
        return step

    def results(self):
        import torch
        return {k: float(torch.stack(v).to(torch.float64).mean().item()) if v else float("nan") for k, v in self._steps.items()}
