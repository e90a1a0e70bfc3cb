"""A NumPy restatement of the encoder on a RAGGED batch (include/mi355asr.h, "Ragged batches"): padded audio [B, L] plus
lengths, every per-utterance rule written as a mask on the padded arrays -- the specification the length-aware kernels
implement.  Test code only; tests/test_ragged_host.py holds it to per-utterance runs of the float64 oracle."""
import numpy as np

from helpers import co


def masked_encoder(wav, lens, w, cfg, hop=160, n_dft=1024):
    wav = np.asarray(wav, np.float64)
    B, L = wav.shape
    F, _, _ = co.same_pad(L, n_dft, hop)
    st1 = cfg.get("reduction_factor", 4) // 2
    # STFT: utterance b framed with its own SAME padding; samples at or past lens[b] read as zero
    fr = np.zeros((B, F, n_dft))
    Fb = np.zeros(B, np.int64)
    for b in range(B):
        Fb[b], lo, _ = co.same_pad(int(lens[b]), n_dft, hop)
        x = np.zeros(lo + F * hop + n_dft)
        x[lo:lo + lens[b]] = wav[b, :lens[b]]
        fr[b] = x[np.arange(F)[:, None] * hop + np.arange(n_dft)[None, :]]
    re, im = fr @ w["mel_layer/real_kernels"].astype(np.float64), fr @ w["mel_layer/imag_kernels"].astype(np.float64)
    p = re * re + im * im
    log_spec = 10.0 * np.log(np.maximum(p, 1e-10)) / np.log(10).astype(np.float32).astype(np.float64)
    # dB maximum over the utterance's own F_b frames only
    fvalid = np.arange(F)[None, :] < Fb[:, None]
    mx = np.where(fvalid[..., None], log_spec, -np.inf).reshape(B, -1).max(axis=1)
    db = np.maximum(log_spec - mx[:, None, None], -80.0)
    mel = db @ w["mel_layer/freq2mel"].astype(np.float64)

    def conv_same_ragged(x, n_in, k, bias, st):
        """Conv2D 'same' in time with each utterance's own top padding (from its own n_in rows); rows >= n_in read 0"""
        Bx, H, W, C = x.shape
        oh = -(-H // st)
        n_out = np.zeros(Bx, np.int64)
        kh, kw, _, O = k.shape
        ow, pl, pr = co.same_pad(W, kw, 2)
        y = np.zeros((Bx, oh, ow, O))
        for b in range(Bx):
            n_out[b], pt, _ = co.same_pad(int(n_in[b]), kh, st)
            xb = np.where((np.arange(H) < n_in[b])[:, None, None], x[b], 0.0)
            xp = np.zeros((pt + oh * st + kh, W + pl + pr, C))
            xp[pt:pt + H, pl:pl + W] = xb
            for i in range(kh):
                for j in range(kw):
                    y[b] += xp[i:i + oh * st:st, j:j + ow * 2:2, :] @ k[i, j].astype(np.float64)
        return y + bias.astype(np.float64), n_out

    pre = "conv_subsampling"
    x, T1b = conv_same_ragged(mel[..., None], Fb, w[pre + "/conv1/kernel"], w[pre + "/conv1/bias"], st1)
    x = np.maximum(x, 0)
    x, Tb = conv_same_ragged(x, T1b, w[pre + "/conv2/kernel"], w[pre + "/conv2/bias"], 2)
    x = np.maximum(x, 0)
    Bx, T, Fo, C = x.shape
    x = x.reshape(Bx, T, Fo * C) @ w[pre + "/linear/kernel"].astype(np.float64) + w[pre + "/linear/bias"].astype(np.float64)
    tvalid = np.arange(T)[None, :] < Tb[:, None]
    for i in range(cfg["num_blocks"]):
        x = masked_block(x, tvalid, w, "conformer_block_%d" % i, cfg["head_size"], cfg.get("fc_factor", 0.5))
    return np.where(tvalid[..., None], x, 0.0), Tb


def masked_block(x, tvalid, w, p, head_size, fc_factor):
    """ConformerBlock with attention keys t >= T_b excluded and the depthwise conv reading zeros from row T_b on"""
    x = co.ff_module(x, w, p + "/ff_module_1", fc_factor)
    q = p + "/mhsa_module"
    y = co.layer_norm(x, w[q + "/ln/gamma"], w[q + "/ln/beta"])
    mask = tvalid[:, None, None, :].astype(np.float64)            # [B, 1 (heads), 1 (queries), keys]
    x = x + co.mha(y, y, w, q + "/mha", head_size, mask=mask)
    c = p + "/conv_module"
    y = co.layer_norm(x, w[c + "/ln/gamma"], w[c + "/ln/beta"])
    y = co._dense(y, w[c + "/pw_conv_1/kernel"][0]) + w[c + "/pw_conv_1/bias"]
    d = y.shape[-1] // 2
    y = y[..., :d] * co.sigmoid(y[..., d:])
    y = np.where(tvalid[..., None], y, 0.0)                      # the GLU output past the utterance is its padding
    y = co.depthwise_conv1d_same(y, w[c + "/dw_conv/depthwise_kernel"])
    y = co._dense(y, w[c + "/dw_conv/pointwise_kernel"][0]) + w[c + "/dw_conv/bias"]
    y = (y - w[c + "/bn/moving_mean"]) / np.sqrt(w[c + "/bn/moving_variance"] + co.BN_EPS) * w[c + "/bn/gamma"] + w[c + "/bn/beta"]
    y = co._dense(co.swish(y), w[c + "/pw_conv_2/kernel"][0]) + w[c + "/pw_conv_2/bias"]
    x = x + y
    x = co.ff_module(x, w, p + "/ff_module_2", fc_factor)
    return co.layer_norm(x, w[p + "/ln/gamma"], w[p + "/ln/beta"])
