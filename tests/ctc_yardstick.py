"""Yardsticks of the CTC lattice tests, none of them the code under test:
  torch_chain    torch.nn.functional.ctc_loss on the CPU, fed log_softmax(log(softmax(z) + 1e-7)) -- the chain of
                 tf.keras.backend.ctc_batch_cost -- in float64 (the yardstick) or float32 (the scale of float32 error);
                 autograd gives the gradient with respect to z
  log_q          the class distribution the lattice runs over, as log-probabilities
  viterbi        the max-plus pass over the lattice in NumPy, in a chosen dtype
  brute_force    every one of the V^T paths of a tiny case
and the seeded cases both test files use."""
import itertools

import numpy as np
import torch

EPS = 1e-7
ULP32 = 2.0 ** -23


def log_q(z, dtype=torch.float64, is_logits=True):
    z = (z if torch.is_tensor(z) else torch.as_tensor(np.asarray(z))).to(dtype)
    p = torch.softmax(z, -1) if is_logits else z
    return torch.log_softmax(torch.log(p + EPS), -1)


def torch_chain(z, labels, input_length, label_length, dtype=torch.float64, want_grad=True, blank=None):
    """-> (loss [B], d sum(loss) / d z [B,T,V] or None), NumPy, in `dtype`"""
    z = torch.as_tensor(np.asarray(z)).to(dtype).clone().requires_grad_(want_grad)
    B, T, V = z.shape
    lq = log_q(z, dtype)
    il = torch.as_tensor(np.asarray(input_length).reshape(-1), dtype=torch.long)
    ll = torch.as_tensor(np.asarray(label_length).reshape(-1), dtype=torch.long)
    tg = torch.as_tensor(np.asarray(labels), dtype=torch.long).reshape(B, -1)
    if tg.shape[1] == 0:
        tg = torch.zeros((B, 1), dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(lq.transpose(0, 1), tg, il, ll, blank=V - 1 if blank is None else blank, reduction="none")
    grad = None
    if want_grad:
        loss.sum().backward()
        grad = z.grad.numpy()
    return loss.detach().numpy(), grad


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def viterbi(lq, labels, blank, dtype=np.float64):
    """lq [T, V] log-probabilities, labels [U] -> (score, path [T]) of the best alignment; (-inf, None) when there is none.
    Ties: the lower predecessor state wins (any best path is a valid answer)."""
    lq = np.asarray(lq).astype(dtype)
    T = lq.shape[0]
    ext = [blank]
    for l in labels:
        ext += [int(l), blank]
    S = len(ext)
    ninf = dtype(-np.inf)
    a = np.full(S, ninf, dtype)
    a[0] = lq[0, ext[0]]
    if S > 1:
        a[1] = lq[0, ext[1]]
    bp = np.zeros((T, S), np.int32)
    for t in range(1, T):
        n = np.full(S, ninf, dtype)
        for s in range(S):
            best, k = a[s], 0
            if s >= 1 and a[s - 1] > best:
                best, k = a[s - 1], 1
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] and a[s - 2] > best:
                best, k = a[s - 2], 2
            n[s] = dtype(best + lq[t, ext[s]])
            bp[t, s] = k
        a = n
    s = S - 1
    if S > 1 and a[S - 2] > a[S - 1]:
        s = S - 2
    score = a[s]
    if not np.isfinite(score):
        return float("-inf"), None
    path = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = ext[s]
        s -= bp[t, s]
    return float(score), path


def path_logprob(lq64, path):
    return float(np.sum(np.asarray(lq64, np.float64)[np.arange(len(path)), np.asarray(path)]))


def brute_force(lq, labels, blank):
    """lq [T, V] -> (-log sum over the paths that collapse to `labels`, best such path's log-probability, that path,
    whether the best is unique); (inf, -inf, None, True) when no path does"""
    lq = np.asarray(lq, np.float64)
    T, V = lq.shape
    want = [int(l) for l in labels]
    total, best, best_path, n_best = 0.0, -np.inf, None, 0
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) != want:
            continue
        lp = float(sum(lq[t, c] for t, c in enumerate(path)))
        total += np.exp(lp)
        if lp > best + 1e-12:
            best, best_path, n_best = lp, np.array(path), 1
        elif abs(lp - best) <= 1e-12:
            n_best += 1
    if best_path is None:
        return np.inf, -np.inf, None, True
    return -np.log(total), best, best_path, n_best == 1


def bound(err32, values):
    """the ceiling on the GPU's error against float64: 4 x the error of torch's own float32 run of the chain (this project's
    convention for recorded-error ceilings), with a floor of 16 float32 ulps at the tensor's scale"""
    return max(4.0 * float(err32), 16.0 * ULP32 * float(np.max(np.abs(values))))


# ---- the seeded cases ------------------------------------------------------------------------------------------------------
def make_case(seed, B, T, V, U, scale=1.0, boost=0.0):
    """logits [B,T,V] f32, labels [B,U] i32, input lengths and label lengths [B]: ragged, row 0 with T frames and U labels,
    row 1 with no labels, row 2 with all labels equal (and frames enough for the blanks between them)"""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn((B, T, V), generator=g) * scale).numpy().astype(np.float32)
    labels = torch.randint(0, V - 1, (B, U), generator=g).numpy().astype(np.int32)
    il = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g).numpy().astype(np.int32)
    ll = torch.randint(max(U // 4, 1), U + 1, (B,), generator=g).numpy().astype(np.int32)
    il[0], ll[0] = T, U
    ll[1] = 0
    labels[2, :] = labels[2, 0]
    ll[2] = min(int(ll[2]), int(il[2]) // 3)
    for b in range(B):                                        # keep every row feasible: frames >= labels + adjacent repeats
        n = int(ll[b])
        rep = int(np.sum(labels[b, 1:n] == labels[b, :n - 1])) if n > 1 else 0
        assert il[b] >= n + rep, (b, il[b], n, rep)
    if boost:
        for b in range(B):
            ext = [V - 1]
            for l in labels[b, :ll[b]]:
                ext += [int(l), V - 1]
            tb = int(il[b])
            for t in range(tb):
                z[b, t, ext[t * len(ext) // tb]] += boost
    return z, labels, il, ll


CASES = {
    "a_random_scale1": dict(seed=11, B=8, T=250, V=1332, U=40, scale=1.0),
    "a_random_scale4": dict(seed=12, B=8, T=250, V=1332, U=40, scale=4.0),
    "b_boost8": dict(seed=13, B=8, T=250, V=1332, U=40, boost=8.0),
    "b_boost12": dict(seed=14, B=8, T=250, V=1332, U=40, boost=12.0),
    "c_long_boost10": dict(seed=15, B=4, T=750, V=1332, U=100, boost=10.0),
    "d_wide_boost12": dict(seed=16, B=4, T=120, V=9160, U=30, boost=12.0),
}

# (V = 4, blank = 3): [a], [a, a], [a, b, a], []
TINY = [([0], 3), ([0, 0], 4), ([0, 1, 0], 6), ([], 3), ([1, 1], 5), ([0, 1, 0], 3)]


def tiny_logits(i, T, V=4):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn((1, T, V), generator=g) * 2).numpy().astype(np.float32)
