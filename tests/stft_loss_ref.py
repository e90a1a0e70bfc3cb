"""Float64 NumPy restatement of the VAD trainer's losses (vad/utils/stft.py TFMultiResolutionSTFT, vad/trainer/vad_trainer.py
mask_loss / binary_accuracy) and of what tensorflowasr_amd.losses adds to them: ragged rows, the analytic gradient with respect
to the predicted waveform, the F1 counts.  tests/test_stft_loss_host.py pins it against the reference's own file run on the
stand-in (tests/golden/stft_loss_ref.npz) and against torch float64 autograd; the GPU tests compare the kernels with it.

tf.signal.stft: frame f holds the samples f*step .. f*step + frame_length - 1 times a periodic Hann window of frame_length,
zero-padded at the end to fft_length; F = 1 + (L - frame_length) // step frames, 0 when L < frame_length.
TFSTFT.call unpacks `x, y = inputs` from `[y, x]`, so the spectral convergence is ||p - t|| / (||p|| + 1e-6) with p the
PREDICTED magnitude."""
import numpy as np

RESOLUTIONS = ((1024, 600, 120), (512, 250, 50))          # (fft_length, frame_length, frame_step) of the reference


def _uniform(n, seed):
    """n float64 in [-0.5, 0.5): an integer hash of the element index (no generator whose stream a library may change)"""
    h = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(1000003) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return (h >> np.uint64(11)).astype(np.float64) / float(1 << 53) - 0.5


def seeded_pair(shape, seed):
    """(truth, prediction) float32 of `shape`: a two-tone signal plus noise, and a scaled, differently noisy copy of it"""
    n = int(np.prod(shape))
    i = np.arange(n)
    clean = 0.3 * np.sin(2 * np.pi * 0.031 * i) + 0.2 * np.sin(2 * np.pi * 0.173 * i + 1.0) + 0.1 * _uniform(n, 2 * seed)
    pred = 0.8 * clean + 0.15 * _uniform(n, 2 * seed + 1)
    return clean.astype(np.float32).reshape(shape), pred.astype(np.float32).reshape(shape)


def seeded_mask(shape, seed):
    """(labels in {0, 1}, logits) float32 of `shape`"""
    n = int(np.prod(shape))
    z = (_uniform(n, 2 * seed) > 0.1).astype(np.float32)
    x = (6.0 * _uniform(n, 2 * seed + 1) + 2.0 * (z - 0.5)).astype(np.float32)
    return z.reshape(shape), x.reshape(shape)


def n_frames(L, frame_length, step):
    return 1 + (L - frame_length) // step if L >= frame_length else 0


def window(frame_length):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(frame_length) / frame_length)


def spectrum(x, fft, fl, step):
    """x float64 [L] -> complex [F, fft/2 + 1]"""
    F = n_frames(len(x), fl, step)
    idx = np.arange(F)[:, None] * step + np.arange(fl)[None, :]
    return np.fft.rfft(np.asarray(x, np.float64)[idx] * window(fl), n=fft, axis=-1)


def magnitude(X):
    return np.sqrt(np.abs(X) ** 2 + 1e-7) + 1e-6


def _lengths(y, lengths):
    B, L = y.shape
    return [L] * B if lengths is None else [int(min(max(v, 0), L)) for v in lengths]


def loss_rows(y_true, y_pred, lengths=None, resolutions=RESOLUTIONS):
    """-> sc f64 [B, R], mag f64 [B, R] (the row's own mean over frames x bins; NaN without a frame), frames i64 [B, R]"""
    y_true, y_pred = np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64)
    B = y_true.shape[0]
    lens = _lengths(y_true, lengths)
    R = len(resolutions)
    sc, mag, frames = np.zeros((B, R)), np.full((B, R), np.nan), np.zeros((B, R), np.int64)
    for b in range(B):
        for r, (fft, fl, step) in enumerate(resolutions):
            F = n_frames(lens[b], fl, step)
            frames[b, r] = F
            if F == 0:
                continue
            p = magnitude(spectrum(y_pred[b, :lens[b]], fft, fl, step))
            t = magnitude(spectrum(y_true[b, :lens[b]], fft, fl, step))
            sc[b, r] = np.sqrt(np.sum((p - t) ** 2)) / (np.sqrt(np.sum(p ** 2)) + 1e-6)
            mag[b, r] = np.mean((np.log(p) - np.log(t)) ** 2)
    return sc, mag, frames


def weights(frames, upstream=1.0):
    """the coefficients of sc[b, r] and mag[b, r] in the scalar: w_sc = 1 / (R B), w_mag = F[b, r] / (R sum_b F[b, r])"""
    frames = np.asarray(frames, np.float64)
    B, R = frames.shape
    tot = frames.sum(0, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        w_mag = frames / (R * tot)
    return np.full((B, R), upstream / (R * B)), w_mag * upstream


def scalar(sc, mag, frames):
    """mean_r(mean_b sc) + mean_r(the mean of (log p - log t)^2 over all valid frames of the batch); with equal lengths this is
    TFMultiResolutionSTFT.call.  A resolution without any frame gives NaN (TensorFlow's mean of nothing)."""
    w_sc, w_mag = weights(frames)
    m = np.where(np.asarray(frames) > 0, mag, 0.0)
    return float(np.sum(w_sc * sc) + np.sum(w_mag * m))


def loss(y_true, y_pred, lengths=None, resolutions=RESOLUTIONS):
    return scalar(*loss_rows(y_true, y_pred, lengths, resolutions))


def grad_rows(y_true, y_pred, w_sc, w_mag, lengths=None, resolutions=RESOLUTIONS):
    """d / d y_pred of sum_{b, r} (w_sc[b, r] sc[b, r] + w_mag[b, r] mag[b, r]) -> f64 [B, L].  Where ||p - t|| == 0 the spectral
    convergence term contributes 0 (TensorFlow gives NaN there); a resolution without a frame contributes nothing."""
    y_true, y_pred = np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64)
    B, L = y_true.shape
    lens = _lengths(y_true, lengths)
    g = np.zeros((B, L))
    for b in range(B):
        for r, (fft, fl, step) in enumerate(resolutions):
            F = n_frames(lens[b], fl, step)
            if F == 0:
                continue
            P = spectrum(y_pred[b, :lens[b]], fft, fl, step)
            s = np.sqrt(np.abs(P) ** 2 + 1e-7)
            p = s + 1e-6
            t = magnitude(spectrum(y_true[b, :lens[b]], fft, fl, step))
            D, Np = np.sqrt(np.sum((p - t) ** 2)), np.sqrt(np.sum(p ** 2))
            dp = w_mag[b, r] * 2.0 * (np.log(p) - np.log(t)) / (p * F * p.shape[1])
            if D > 0:
                dp = dp + w_sc[b, r] * ((p - t) / (D * (Np + 1e-6)) - D * p / (Np * (Np + 1e-6) ** 2))
            G = dp / s * P                                            # dL / d Re X + i dL / d Im X
            G[:, 1:-1] *= 0.5                                         # irfft doubles the inner bins; it ignores Im at the two ends
            xw = np.fft.irfft(G, n=fft, axis=-1)[:, :fl] * fft * window(fl)
            for f in range(F):
                g[b, f * step:f * step + fl] += xw[f]
    return g


def loss_and_grad(y_true, y_pred, lengths=None, resolutions=RESOLUTIONS, upstream=1.0):
    sc, mag, frames = loss_rows(y_true, y_pred, lengths, resolutions)
    w_sc, w_mag = weights(frames, upstream)
    return scalar(sc, mag, frames), grad_rows(y_true, y_pred, w_sc, np.nan_to_num(w_mag), lengths, resolutions)


# ---- VADTrainer.mask_loss, binary_accuracy, F1 --------------------------------------------------------------------------------------
def _valid(shape, lengths):
    B, T = shape
    cnt = [T] * B if lengths is None else [int(min(max(v, 0), T)) for v in lengths]
    return np.arange(T)[None, :] < np.asarray(cnt)[:, None]


def bce(labels, logits):
    x, z = np.asarray(logits, np.float64), np.asarray(labels, np.float64)
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def mask_stats(labels, logits, lengths=None, threshold=0.5):
    """labels, logits [B, T] -> (sums f64 [4]: sum loss*one, sum one, sum loss*zero, sum zero; counts i64 [4]: TP, FP, FN, TN of
    the decision float32(logit) > float32(threshold)) over the frames t < lengths[b]"""
    z = np.asarray(labels, np.float32)
    v = _valid(z.shape, lengths)
    x = np.where(v, np.asarray(logits, np.float32), np.float32(0))
    z = np.where(v, z, np.float32(-1))
    l = bce(z, x)
    one, zero = v & (z == 1), v & (z == 0)
    pos = x > np.float32(threshold)
    sums = np.array([l[one].sum(), one.sum(), l[zero].sum(), zero.sum()], np.float64)
    counts = np.array([(one & pos).sum(), (zero & pos).sum(), (one & ~pos).sum(), (zero & ~pos).sum()], np.int64)
    return sums, counts


def mask_loss(labels, logits, lengths=None):
    s, _ = mask_stats(labels, logits, lengths)
    return s[0] / (s[1] + 1e-6), s[2] / (s[3] + 1e-6)


def mask_grad(labels, logits, lengths=None):
    """d (one_loss + zero_loss) / d logits, 0 past a row's count"""
    z = np.asarray(labels, np.float32)
    v = _valid(z.shape, lengths)
    x = np.where(v, np.asarray(logits, np.float64), 0.0)
    z = np.where(v, z, np.float32(-1))
    s, _ = mask_stats(labels, logits, lengths)
    w = np.where(z == 1, 1.0 / (s[1] + 1e-6), np.where(z == 0, 1.0 / (s[3] + 1e-6), 0.0))
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return np.where(v, (sig - z) * w, 0.0)


def metrics(labels, logits, threshold=0.5, lengths=None):
    _, c = mask_stats(labels, logits, lengths, threshold)
    tp, fp, fn, tn = (int(v) for v in c)
    n = tp + fp + fn + tn
    den = 2 * tp + fp + fn
    return {"acc": (tp + tn) / n if n else float("nan"), "f1": 2 * tp / den if den else 0.0, "tp": tp, "fp": fp, "fn": fn, "tn": tn}


# ---- the same arithmetic in torch (the accuracy yardstick in float32, the autograd check in float64) -----------------------------------
def torch_loss(y, x, lengths, resolutions=RESOLUTIONS):
    """y, x torch [B, L] of one dtype: unfold x window, torch.fft.rfft, the reference's arithmetic, ragged rows as above
    -> (scalar, sc [B][R], mag [B][R]) as tensors (None where the row has no frame); the scalar leaves out a resolution without
    any frame, so that its gradient stays defined"""
    import math
    import torch
    B, R_ = y.shape[0], len(resolutions)
    total = 0.0
    sc = [[None] * R_ for _ in range(B)]
    mag = [[None] * R_ for _ in range(B)]
    for r, (fft, fl, step) in enumerate(resolutions):
        n = torch.arange(fl, dtype=torch.float64)
        win = (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / fl)).to(x.dtype)
        num, cnt = 0.0, 0
        for b in range(B):
            L = int(lengths[b])
            if L < fl:
                continue
            P = torch.fft.rfft(x[b, :L].unfold(0, fl, step) * win, n=fft)
            T = torch.fft.rfft(y[b, :L].unfold(0, fl, step) * win, n=fft)
            p = torch.sqrt(P.real ** 2 + P.imag ** 2 + 1e-7) + 1e-6
            t = torch.sqrt(T.real ** 2 + T.imag ** 2 + 1e-7) + 1e-6
            sc[b][r] = torch.sqrt(((p - t) ** 2).sum()) / (torch.sqrt((p ** 2).sum()) + 1e-6)
            d2 = ((torch.log(p) - torch.log(t)) ** 2).sum()
            mag[b][r] = d2 / p.numel()
            total = total + sc[b][r] / (R_ * B)
            num = num + d2
            cnt += p.numel()
        if cnt:
            total = total + num / cnt / R_
    return total, sc, mag
