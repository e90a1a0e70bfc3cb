"""Scoring of evaluation batches on the GPU: the reference's `levenshtein` / `wer` (utils/xer.py:12-35, 211-220) for a ragged
batch in one launch (`mi355asr_edit_distance`, csrc/edit_distance.hip), with the filtering `AMTester._eval_step` does in front
of it (am_tester.py:34-89: cut the hypothesis at the first stop id, strip pad / end ids from both sides).

    ed = EditDistance("cuda:0")
    res, lens = ed(ref_ids, hyp_ids, drop_ref=(pad,), drop_hyp=(pad,))     # i32 [B, 4] (distance, S, D, I), i32 [B, 2] (n, m)
    score_transcripts(["the cat sat"], ["the cat sat down"])               # [(rate, S, D, I)] as eval.wer

The (S, D, I) split is that of the one optimal alignment the reference's recursion carries (a substitution / match step before
a deletion, a deletion before an insertion); eval.levenshtein is the host restatement it is tested against."""
import ctypes

import numpy as np
import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def filter_row(row, drop=(), stop=None):
    """What the kernel's prologue does to one row, on the host: cut before the first `stop`, then remove the ids of `drop`."""
    row = [int(t) for t in row]
    if stop is not None and int(stop) in row:
        row = row[:row.index(int(stop))]
    drop = set(int(d) for d in drop)
    return [t for t in row if t not in drop]


class EditDistance:
    """`EditDistance(device)(ref, hyp, ...)`: rows are i32 [B, N] / [B, M] host arrays or device tensors, lengths i32 [B] or
    None (the whole row counts; entries at or past a row's length are never read).  Returns device tensors."""

    STRIP = 1024                    # hypothesis columns per strip (one per thread of the workgroup that owns the pair)
    MAX_LEN = 16384                 # tokens per row: the counts are kept in 16 bits
    MAX_ALIGN_CELLS = 1 << 24       # return_ops: N * M cells at most (2 bits per cell, 4 MiB per pair)

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.Mi355AsrError("EditDistance runs on the GPU only (got device %s)" % device)
        self._lib = _lib.lib()

    def _rows(self, x):
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32)))
        if x.dim() != 2:
            raise ValueError("rows are [B, width] (got shape %s)" % (tuple(x.shape),))
        x = x.to(device=self.device, dtype=torch.int32).contiguous()
        return x

    def _lengths(self, v, B):
        if v is None:
            return None
        if not torch.is_tensor(v):
            v = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.int32)))
        v = v.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        if v.numel() != B:
            raise ValueError("%d lengths for %d rows" % (v.numel(), B))
        return v

    def __call__(self, ref, hyp, ref_lengths=None, hyp_lengths=None, drop_ref=(), drop_hyp=(), hyp_stop=None, return_ops=False):
        """-> (result i32 [B, 4] = (distance, S, D, I), lengths i32 [B, 2] = filtered (n, m)); with return_ops also
        (ops u8 [B, N + M], n_ops i32 [B]): ops[b, :n_ops[b]] is the alignment in forward order, 0 match, 1 substitution,
        2 deletion, 3 insertion."""
        ref, hyp = self._rows(ref), self._rows(hyp)
        B = ref.shape[0]
        if hyp.shape[0] != B or B < 1:
            raise ValueError("ref and hyp need the same, non-zero number of rows (got %d and %d)" % (B, hyp.shape[0]))
        ref_lengths, hyp_lengths = self._lengths(ref_lengths, B), self._lengths(hyp_lengths, B)
        # a batch whose rows are all empty on one side: one column that no length reaches
        if ref.shape[1] == 0:
            ref, ref_lengths = torch.zeros((B, 1), dtype=torch.int32, device=self.device), torch.zeros(B, dtype=torch.int32, device=self.device)
        if hyp.shape[1] == 0:
            hyp, hyp_lengths = torch.zeros((B, 1), dtype=torch.int32, device=self.device), torch.zeros(B, dtype=torch.int32, device=self.device)
        N, M = ref.shape[1], hyp.shape[1]
        drop_ref, drop_hyp = [int(d) for d in drop_ref], [int(d) for d in drop_hyp]
        dr = (ctypes.c_int32 * max(len(drop_ref), 1))(*drop_ref)
        dh = (ctypes.c_int32 * max(len(drop_hyp), 1))(*drop_hyp)
        lib = self._lib
        nbytes = ctypes.c_size_t()
        _lib.check(lib.mi355asr_edit_distance_workspace_bytes(B, N, M, int(bool(return_ops)), ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        out = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        lens = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        ops = torch.empty((B, N + M), dtype=torch.uint8, device=self.device) if return_ops else None
        n_ops = torch.empty((B,), dtype=torch.int32, device=self.device) if return_ops else None
        self.launch(ref, ref_lengths, hyp, hyp_lengths, dr, len(drop_ref), dh, len(drop_hyp), hyp_stop, out, lens, ops, n_ops, ws)
        return (out, lens, ops, n_ops) if return_ops else (out, lens)

    def launch(self, ref, ref_lengths, hyp, hyp_lengths, dr, n_dr, dh, n_dh, hyp_stop, out, lens, ops, n_ops, ws):
        """The C call on buffers the caller owns (the tests hand in poisoned outputs)."""
        with torch.cuda.device(self.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(self._lib.mi355asr_edit_distance(
                _p(ref), _p(ref_lengths), _p(hyp), _p(hyp_lengths), ref.shape[0], ref.shape[1], hyp.shape[1], dr, n_dr, dh, n_dh,
                int(hyp_stop is not None), int(hyp_stop) if hyp_stop is not None else 0, _p(out), _p(lens), _p(ops), _p(n_ops),
                _p(ws), ws.numel(), st))


def _pad_rows(rows):
    out = np.zeros((len(rows), max(max((len(r) for r in rows), default=0), 1)), np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32)


def score_transcripts(refs, hyps, device="cuda:0"):
    """`eval.wer` for lists of token lists or strings (a string is its characters): -> [((S + D + I) / N, S, D, I)] per pair,
    in one GPU call.  An empty reference raises ZeroDivisionError, as `wer` does."""
    refs, hyps = [list(r) for r in refs], [list(h) for h in hyps]
    if len(refs) != len(hyps):
        raise ValueError("%d references for %d hypotheses" % (len(refs), len(hyps)))
    if any(len(r) == 0 for r in refs):
        raise ZeroDivisionError("division by zero: empty reference")
    if not refs:
        return []
    vocab = {}
    ids = [[[vocab.setdefault(t, len(vocab)) for t in row] for row in side] for side in (refs, hyps)]
    (r, rl), (h, hl) = _pad_rows(ids[0]), _pad_rows(ids[1])
    out, _ = EditDistance(device)(r, h, rl, hl)
    return [((s + d + i) / len(ref), s, d, i) for ref, (_, s, d, i) in zip(refs, out.cpu().tolist())]


def confusions(ref, hyp, ops, n_ops):
    """The alignment as the table an evaluator prints.  ref / hyp: the FILTERED rows the alignment refers to (`filter_row`), one
    pair or a batch of them; ops / n_ops as EditDistance returns them (host arrays or tensors).
    -> (substitutions {(ref_id, hyp_id): count}, deletions {ref_id: count}, insertions {hyp_id: count}), summed over the batch."""
    ops = ops.cpu().numpy() if torch.is_tensor(ops) else np.asarray(ops)
    n_ops = n_ops.cpu().numpy() if torch.is_tensor(n_ops) else np.asarray(n_ops)
    if n_ops.ndim == 0:
        ref, hyp, ops, n_ops = [ref], [hyp], ops.reshape(1, -1), n_ops.reshape(1)
    sub, dele, ins = {}, {}, {}
    for r, h, o, k in zip(ref, hyp, ops, n_ops):
        x = y = 0
        for code in o[:int(k)].tolist():
            if code == 0:
                x, y = x + 1, y + 1
            elif code == 1:
                key = (int(r[x]), int(h[y]))
                sub[key] = sub.get(key, 0) + 1
                x, y = x + 1, y + 1
            elif code == 2:
                dele[int(r[x])] = dele.get(int(r[x]), 0) + 1
                x += 1
            else:
                ins[int(h[y])] = ins.get(int(h[y]), 0) + 1
                y += 1
        if x != len(r) or y != len(h):
            raise ValueError("the alignment covers %d x %d tokens of a %d x %d pair" % (x, y, len(r), len(h)))
    return sub, dele, ins
