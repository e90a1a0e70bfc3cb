/* mi355asr.h -- C ABI of libmi355asr.so: the MI355X (gfx950) Conformer-CTC hot path of
 * Z-yq/TensorflowASR (encoder + CTCDecoder + CTC greedy decode) behind plain pointers and sizes.
 *
 * The reference has no FFI for this path: it is Keras `Model` objects called from Python
 * (test_asr.py:186-219) and, in deployment, ONNX sessions called from C++
 * (Inference/CppInference/onnx/src/core/asr_session.cpp:77-123).  Each entry point below names the
 * reference interface it stands in for.  INTEGRATION.md shows the ctypes stub (Python reference)
 * and the C++ `ASR::Session` patch a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MI355ASR_E* code on failure;
 *     mi355asr_last_error() returns a thread-local message for the last failure on this thread
 *   - `*_dev` pointers are DEVICE pointers owned by the caller (e.g. torch-ROCm tensors);
 *     host pointers are marked `_host`
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is enqueued
 *     asynchronously on it; nothing synchronises the device
 *   - nothing is enqueued on any stream but `stream` -- no launch, no copy, no memset -- so a call made on a stream that
 *     does not synchronise with the null stream sees its inputs as that stream left them (an entry that names a
 *     synchronisation below waits for `stream` alone)
 *   - a workspace (`ws_dev`, `ws_bytes` from the matching *_workspace_bytes) may hold anything on entry: no call reads a
 *     workspace word it has not written itself; on exit its contents are unspecified.  No byte outside
 *     [ws_dev, ws_dev + ws_bytes), the output tensors and, for the stateful families, the state buffer is written
 *   - an opaque state buffer (chunk streams, beam streams, resample streams) needs nothing but its `reset`, whatever it held
 *     before: rings and arenas are never read past their counters
 *   - an output is written in full, padding included (0, -1 or -FLT_MAX as its entry says), except where an entry says that
 *     a region is not written: mi355asr_vad_forward / mi355asr_vad_enhance past a row's frame count, the capacity of the
 *     mi355asr_chunk_outputs buffers behind their [B, Tp] blocks, and y_dev of mi355asr_resample_streams_step past
 *     n_out_host[i]
 *     (tests/test_gpu_caller_contract.py holds every entry point to these points on poisoned, fenced buffers)
 *   - a handle is not re-entrant: one in-flight call per handle (the reference's C++ Session has the
 *     same contract, asr_session.h keeps mutable buffers); distinct handles are independent: they may be in flight at the
 *     same time on different streams, from one thread or from several
 *   - values and accumulation are fp32 everywhere, matching the reference's dtype.  Products are formed by the fp32 matrix
 *     instruction (v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain) or, in the large dmodel-144 kernels, on the 16-bit
 *     matrix pipe from SPLIT fp32 operands: three bf16 terms each, exact (six v_mfma_f32_16x16x32_bf16 per product group,
 *     the dropped term pairs below 2^-24 of a product), or -- where an operand bound is known: the handle's own weights,
 *     its LayerNorm outputs, its frontend's dB range, a row maximum measured in the kernel -- two fp16 terms of the operand
 *     times a power of two (hi + lo, round-to-nearest: 2^-22 relative; three v_mfma_f32_16x16x32_f16 per product group).
 *     Both sit at the same measured distance from the fp64 oracle as the fp32 instruction; stage
 *     calls on caller-supplied tensors always take the exact three-term or fp32 kernels.
 *     gemm_dtype = 1 is the separate, lossy bf16 mode (operands rounded to bf16).
 */
#ifndef MI355ASR_H
#define MI355ASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355ASR_OK 0
#define MI355ASR_EINVAL -1   /* bad argument / unsupported configuration */
#define MI355ASR_ESTATE -2   /* call order (weights not finalised, ...) */
#define MI355ASR_EWEIGHT -3  /* unknown / missing / mis-shaped weight */
#define MI355ASR_EWORKSPACE -4
#define MI355ASR_EHIP -5     /* HIP runtime error */

typedef struct mi355asr_model mi355asr_model;

/* Constructor arguments of ConformerEncoder / StreamingConformerEncoder / CTCDecoder
 * (asr/models/conformer_blocks.py:278-294, 386-395, 568-572; values from the YAML files under asr/configs/). */
typedef struct {
  int32_t dmodel;            /* model_config.dmodel                       144 | 256            */
  int32_t num_blocks;        /* model_config.num_blocks                   13  | 4              */
  int32_t head_size;         /* model_config.head_size                    36  | 64   (tuned); 12, 16, 24, 32, 48, 72, 128 run on a general kernel */
  int32_t num_heads;         /* model_config.num_heads                    4                    */
  int32_t kernel_size;       /* model_config.kernel_size                  32  | 5    (tuned); any other size 1 .. 1024 runs on a general kernel   */
  float   fc_factor;         /* model_config.fc_factor                    0.5                  */
  int32_t reduction_factor;  /* model_config.reduction_factor             4          (2, 4, 6 or 8; the tuned kernels are the ones for 4)          */
  int32_t n_mels;            /* speech_config.num_feature_bins            80                   */
  int32_t sample_rate;       /* speech_config.sample_rate                 16000                */
  int32_t stride_ms;         /* speech_config.stride_ms                   10                   */
  int32_t n_dft;             /* hard-coded 1024 in conformer_blocks.py:312                     */
  int32_t chunk_size;        /* StreamingConformerEncoder.add_chunk_size (samples); 0 = offline */
  int32_t has_encoder;       /* 1: handle owns a ConformerEncoder; 0: CTCDecoder-only handle  */
  int32_t num_classes;       /* CTCDecoder num_classes (blank = num_classes-1); 0 = no CTC head */
  int32_t ctc_num_blocks;    /* model_config.ctcdecoder_num_blocks        1                    */
  int32_t ctc_kernel_size;   /* model_config.ctcdecoder_kernel_size       32                   */
  float   ctc_fc_factor;     /* model_config.ctcdecoder_fc_factor         0.5                  */
  int32_t gemm_dtype;        /* 0: fp32 values, fp32-accurate products everywhere (see the header comment; default)
                              * 1: bf16 MFMA for the dense layers -- bf16 GEMM inputs, fp32 accumulation, fp32
                              *    LayerNorm / softmax / activations / frontend (BASELINE config 3)               */
  int32_t mel_layer_type;    /* speech_config.mel_layer_type: 0 = 'Melspectrogram' (default), 1 = 'leaf' (LEAF frontend,
                              *    leaf_audio/frontend.py: Gabor filters + Gaussian pooling + PCEN + instance norm;
                              *    needs n_mels 80, stride_ms 10 at 16 kHz), 2 = 'Spectrogram' (any other value in the
                              *    reference, conformer_blocks.py:318-323: the n_dft/2+1 = 513 dB bins without the mel
                              *    matrix; n_mels is ignored and no freq2mel tensor exists)                        */
  int32_t add_wav_info;      /* speech_config.add_wav_info: 1 adds WavePickModel(waveform) (asr/models/wav_model.py:108-146)
                              *    to the subsampled features (conformer_blocks.py:344-348); needs L % hop_size == 0.
                              *    Calls that run the encoder need at least 3 encoder frames per input (L > 2 * hop_size *
                              *    reduction_factor samples, per chunk when streaming): the branch reflect-pads by two
                              *    frames, which the reference defines for longer inputs only -- else MI355ASR_EINVAL */
} mi355asr_config;

const char* mi355asr_last_error(void);
const char* mi355asr_version(void);
/* Test hook: the two-term fp16 operand split every two-term kernel applies (hi = fp16(x), lo = fp16(x - hi), both round to
 * nearest even) on x_dev f32 [n], as bit patterns: hi_dev, lo_dev u16 [n].  Elements are split in pairs (2 i, 2 i + 1) as
 * the kernels do, so even and odd positions take the two halves of the packed instructions.  Asynchronous on `stream`. */
int mi355asr_test_split_f16(const float* x_dev, int64_t n, uint16_t* hi_dev, uint16_t* lo_dev, void* stream);
/* Test hook: the exact three-term bf16 operand split every three-term kernel applies (each term the truncated high half of what
 * the terms before it left: x = t0 + t1 + t2) on x_dev f32 [n], as bit patterns: t0_dev, t1_dev, t2_dev u16 [n].  Elements are
 * split in pairs (2 i, 2 i + 1) as the kernels pack them; an odd n splits the last element alone.  Asynchronous on `stream`. */
int mi355asr_test_split_bf16(const float* x_dev, int64_t n, uint16_t* t0_dev, uint16_t* t1_dev, uint16_t* t2_dev, void* stream);

/* replaces: ConformerEncoder(...)/CTCDecoder(...) construction, test_asr.py:28-75 */
int mi355asr_create(const mi355asr_config* cfg, mi355asr_model** out);
int mi355asr_destroy(mi355asr_model* m);

/* replaces: model.load_weights(path[, by_name=True]), test_asr.py:95-114.  `name` is the Keras-layout
 * tensor name (see DESIGN.md "weight names"), data is host fp32 in the Keras layout of that tensor.
 * May be called again after finalisation to overwrite a tensor (then finalise again). */
int mi355asr_load_weight(mi355asr_model* m, const char* name, const float* data_host, int32_t rank,
                         const int64_t* dims);
/* the same for checkpoints that store other element types (`load_weights(handle, name, host_ptr, dtype, rank,
 * dims)`): the tensor is converted to fp32 on the host.  bf16 / fp16 are the raw 16-bit patterns. */
#define MI355ASR_DT_F32 0
#define MI355ASR_DT_F16 1
#define MI355ASR_DT_BF16 2
#define MI355ASR_DT_F64 3
#define MI355ASR_DT_I16 4   /* mi355asr_resample and mi355asr_fir_ragged input only */
int mi355asr_load_weight_typed(mi355asr_model* m, const char* name, const void* data_host, int32_t dtype, int32_t rank,
                               const int64_t* dims);
/* number of tensors the configuration expects / name of the i-th one (so loaders can iterate) */
int mi355asr_num_weights(const mi355asr_model* m);
const char* mi355asr_weight_name(const mi355asr_model* m, int32_t i);
/* replaces: iterating model.weights / model.summary() after _build() (test_asr.py:85-93): Keras-layout shape of the
 * i-th tensor, *rank and dims[0..*rank); a non-Python caller sizes its buffers with it (examples/asr_session.cpp). */
int mi355asr_weight_shape(const mi355asr_model* m, int32_t i, int32_t* rank, int64_t* dims, int32_t max_rank);
/* replaces: model._build() (test_asr.py:85-87): checks every tensor is present, packs the matrices into
 * MFMA fragment order, folds BatchNorm into (scale, shift), uploads to HBM. */
int mi355asr_finalize_weights(mi355asr_model* m, void* stream);
/* optional, before mi355asr_finalize_weights: the most rows (batch x encoder frames) one call will bring.  Handles of
 * dmodel 256 / 512 pack every dense layer a second time as a split-bf16 slab ring for batches of >= 1500 rows (1.5 x the
 * dense weights' bytes, and their packing time); a handle that will only see single utterances or streaming chunks says
 * so here and keeps the per-wave kernels (and, at dmodel 256, the fused chains).  rows < 0 = unknown (the default: pack). */
int mi355asr_set_expected_rows(mi355asr_model* m, int64_t rows);
/* which STFT kernel mi355asr_finalize_weights selected: 1 = 32x32 Cooley-Tukey on the matrix cores (the loaded
 * mel_layer/{real,imag}_kernels are window[n]*exp(-2*pi*i*k*n/1024), as backend.py:27-69 builds them), 0 = dense DFT
 * GEMM with the kernels as loaded (a checkpoint changed them), -1 = no frontend / not finalized. */
int mi355asr_stft_mode(const mi355asr_model* m);

/* shape helpers: mel frames F = ceil(L/hop), encoder frames T = ceil(ceil(F/2)/2) per block of L samples */
int mi355asr_out_frames(const mi355asr_model* m, int32_t L, int32_t* mel_frames, int32_t* enc_frames);
/* bytes of caller-provided device scratch needed by any forward call on [B, L] */
int mi355asr_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes);
/* same for the calls that start from encoder frames (ctc_forward, conformer_block): [B, T, dmodel] */
int mi355asr_ctc_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes);

/* replaces: encoder(wav, training=False) / encoder.inference(wav)  (conformer_blocks.py:343-378, 574-594);
 *           ASR::Session::EncoderInference (asr_session.cpp:77-98), ONNX "inputs" -> "Identity:0".
 * wav_dev f32 [B, L] (the reference's trailing channel dim of 1 dropped) -> enc_out_dev f32 [B, T_total, dmodel]
 * with T_total = (L/chunk_size)*T(chunk_size) when chunk_size>0 else T(L). */
int mi355asr_encoder_forward(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L, float* enc_out_dev,
                             void* ws_dev, size_t ws_bytes, void* stream);

/* replaces: ctc_model(enc, training=False) (conformer_blocks.py:419-424); ASR::Session::CTCInference
 * (asr_session.cpp:100-123), ONNX "inputs" [B,T,d] -> "Identity:0" [B,T,V].
 * logits_dev (f32 [B,T,V]) and frame_argmax_dev (i32 [B,T]) may each be NULL.  The argmax is the one
 * tf.keras.backend.ctc_decode / ctc_greedy_decoder.h:9-20 take per frame (first maximum wins). */
int mi355asr_ctc_forward(mi355asr_model* m, const float* enc_dev, int32_t B, int32_t T, float* logits_dev,
                         int32_t* frame_argmax_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* replaces: tf.keras.backend.ctc_decode(probs, input_length)[0][0] greedy (test_asr.py:196-200) and
 * ctc_greedy_decoder(probs, blank_id, vocab) (ctc_greedy_decoder.h:5-44): merge repeated, drop blank,
 * dense output padded with -1.  in_len_dev may be NULL (= T for every utterance). Model-independent. */
int mi355asr_ctc_greedy(const int32_t* frame_argmax_dev, const int32_t* in_len_dev, int32_t B, int32_t T,
                        int32_t blank, int32_t* ids_dev, int32_t* out_len_dev, void* stream);

/* replaces: tf.keras.backend.ctc_batch_cost(y_true, y_pred, input_length, label_length) of CTCTrainer._train_step /
 * _eval_step (asr/trainer/ctc_runners.py:91,133) and ChunkConformer.train_step / test_step
 * (chunk_conformer_blocks.py:1058-1075, 1142-1159): tf.compat.v1.nn.ctc_loss on log(y_pred + 1e-7), which applies a
 * softmax to its inputs, so a frame's class distribution is q = (p + 1e-7) / sum_k (p_k + 1e-7); repeats merged;
 * loss_b = -log sum_paths prod_t q[b, t, pi_t] over the frames t < in_len[b] and the labels labels[b, :label_len[b]].
 * Model-independent.  x_dev f32 [B, T, V]: probabilities (is_logits = 0, ctc_batch_cost's own argument; loss only, a
 * non-NULL grad_dev is rejected) or logits (p = softmax(x); grad_dev, if given, receives d loss_b / d x through the
 * whole chain softmax -> + 1e-7 -> log -> log-softmax -> CTC, rows t >= in_len[b] are 0).  in_len_dev i32 [B] may be
 * NULL (= T); labels_dev i32 [B, U]; label_len_dev i32 [B] (0 is legal: the all-blank path); `blank` is an argument (the
 * reference's is V - 1).  loss_dev f32 [B].
 * Not the reference's behaviour, on purpose: a target that no path of in_len[b] frames can emit (in_len < label_len +
 * adjacent repeats; also a label outside [0, V) or equal to the blank) makes TensorFlow raise; here loss = +inf and
 * the utterance's gradient rows are 0, with no NaN anywhere.
 * Returns -1 with a message, launching nothing, for V < 2, blank outside [0, V), U above the built limit (511), a
 * workspace smaller than mi355asr_ctc_loss_workspace_bytes says, and NULL outputs.  No allocation, no host
 * synchronisation; the result of a row is bit-identical from run to run and whatever else is in the batch. */
int mi355asr_ctc_loss_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t U, int32_t want_grad, size_t* bytes);
int mi355asr_ctc_loss(const float* x_dev, int32_t is_logits, const int32_t* in_len_dev, const int32_t* labels_dev,
                      const int32_t* label_len_dev, int32_t B, int32_t T, int32_t V, int32_t U, int32_t blank,
                      float* loss_dev, float* grad_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Forced alignment: the max-plus (Viterbi) pass over the lattice that mi355asr_ctc_loss sums over -- the token times
 * ASR.offline_stt (test_asr.py:186-200) does not return.  Arguments as for mi355asr_ctc_loss.
 * path_dev i32 [B, T]: the class of every frame on the best path (-1 at t >= in_len[b]); spans_dev i32 [B, U, 2]: first
 * and last frame of each label (-1 for unused entries); score_dev f32 [B]: log of the best path's probability under q.
 * An infeasible target: score -inf, path and spans -1. */
int mi355asr_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t U, size_t* bytes);
int mi355asr_ctc_align(const float* x_dev, int32_t is_logits, const int32_t* in_len_dev, const int32_t* labels_dev,
                       const int32_t* label_len_dev, int32_t B, int32_t T, int32_t V, int32_t U, int32_t blank,
                       int32_t* path_dev, int32_t* spans_dev, float* score_dev, void* ws_dev, size_t ws_bytes,
                       void* stream);

/* replaces: tf.keras.losses.sparse_categorical_crossentropy(labels, logits, from_logits=True), tf.argmax(logits, -1) and the
 * mask_loss / translate_acc of CTCTrainer (asr/trainer/ctc_runners.py:63-76, 102, 144-146), with d / d logits.
 * Model-independent.  The logits row of (b, t), t < Q, is the V floats at x_dev + b * ld_b + t * ld_t (elements, not bytes), so
 * a column slice logits[:, :Q] of a [B, T, V] tensor is ld_b = T * V, ld_t = V; ld_t >= V need not be a multiple of 4, rows
 * that are not 16-byte aligned are read with narrower loads, and no element past V of a row or at t >= Q is read or written.
 * labels_dev i32: the label of (b, t) at labels_dev + b * ld_lab + t.
 * The rows entry: loss_dev f32 [B, Q] = logsumexp(x) - x[label]; argmax_dev i32 [B, Q] (may be NULL), ties to the lowest
 * index; grad_dev (may be NULL; row (b, t) at grad_dev + b * gld_b + t * gld_t) = w * (softmax(x) - onehot(label)), w =
 * weights_dev[b * Q + t] or 1 for NULL.  A label outside [0, V): loss NaN, arg-max as usual, gradient row 0 (TensorFlow raises
 * on the CPU and returns NaN on a GPU).  x[label] = -inf with a finite maximum: loss +inf, gradient finite.
 * The mask-loss entry runs the rows entry into its workspace and reduces in float64, one workgroup, in a fixed order, with
 * need = (label != 0), zero = (label == 0):
 *   mask_loss_dev f32 [B] = mean_t loss[b, t] + sum(loss need) / (sum(need) + 1e-6) + sum(loss zero) / (sum(zero) + 1e-6)
 *   acc_dev f32 [1]       = sum((argmax == label) need) / (sum(need) + 1e-6)                        (translate_acc)
 *   mean_dev f32 [1]      = the mean of loss over all B * Q elements                    (what the translate_loss metric keeps)
 *   grad_dev (may be NULL) = d (sum_b upstream_dev[b] * mask_loss[b]) / d x; upstream_dev f32 [B], NULL = ones; it is read
 *   only when grad_dev is given
 * Returns -1 with a message that names the field, launching nothing and writing nothing, for a NULL required pointer, B or Q
 * below 1, V outside 1 .. 262144, ld_t < V, ld_b < 0, ld_lab < Q, gld_t < V, gradient rows of two batch entries that would
 * overlap, and a workspace smaller than the workspace entry says (B, Q, want_grad).  No allocation, no host synchronisation,
 * no atomics; the results of a row are bit-identical from run to run, wherever the row lies and whatever else is in the batch. */
int mi355asr_xent_workspace_bytes(int32_t B, int32_t Q, int32_t want_grad, size_t* bytes);
int mi355asr_xent_rows(const float* x_dev, int64_t ld_b, int64_t ld_t, const int32_t* labels_dev, int32_t ld_lab,
                       const float* weights_dev, int32_t B, int32_t Q, int32_t V, float* loss_dev, int32_t* argmax_dev,
                       float* grad_dev, int64_t gld_b, int64_t gld_t, void* stream);
int mi355asr_mask_loss(const float* x_dev, int64_t ld_b, int64_t ld_t, const int32_t* labels_dev, int32_t ld_lab,
                       const float* upstream_dev, int32_t B, int32_t Q, int32_t V, float* mask_loss_dev, float* acc_dev,
                       float* mean_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* ws_dev, size_t ws_bytes,
                       void* stream);

/* replaces: TFMultiResolutionSTFT.call of vad/utils/stft.py (the wav_loss of VADTrainer) with d / d prediction, and the sums
 * behind VADTrainer.mask_loss, tf.metrics.binary_accuracy and a binary F1 (vad/trainer/vad_trainer.py:42-48, 76-84).
 * Model-independent.  Row b of the truth is the Lpad floats at truth_dev + b * ld_truth, of the prediction at pred_dev +
 * b * ld_pred (elements; unit stride along the row, rows need not be aligned); len_dev i32 [B] (NULL: every row has Lpad
 * samples) is clamped to 0 .. Lpad and no sample at or past it is read.  Resolution r of R (1 .. 4; host arrays) is
 * (fft_lengths[r] in {512, 1024, 2048}, 1 <= frame_lengths[r] <= fft_lengths[r], 1 <= frame_steps[r] <= frame_lengths[r]) with
 * tf.signal.stft semantics: frame f is the samples f * step .. f * step + frame_length - 1 times a periodic Hann window of
 * frame_length, zero-padded at the end to fft_length; F = 1 + (len - frame_length) / step frames, 0 when len < frame_length.
 * With p = sqrt(|P|^2 + 1e-7) + 1e-6 of the prediction and t of the truth (formed in float64 from fp32 spectra; both DFT stages
 * on v_mfma_f32_16x16x4_f32 with float64-computed tables):
 *   sc_dev f32 [B, R]     = ||p - t||_F / (||p||_F + 1e-6) over the row's frames and bins; 0 for a row without a frame
 *   mag_dev f32 [B, R]    = the row's mean of (log p - log t)^2; NaN for a row without a frame
 *   frames_dev i32 [B, R] = F
 *   grad_dev (may be NULL; row b at grad_dev + b * ld_grad, Lpad elements, every one written) =
 *     d / d prediction of sum_{b, r} (w_sc_dev[b * R + r] * sc[b, r] + w_mag_dev[b * R + r] * mag[b, r]); 0 at and past len and
 *     where no frame reaches.  Where ||p - t|| == 0 the sc term contributes 0 (TensorFlow's gradient is NaN there); a resolution
 *     at which the row has no frame contributes nothing.  The spectra are recomputed for the gradient, not stored.
 * Frame sums, row sums and p, t, log are float64; sums have a fixed order (no atomics): a row's outputs are bit-identical from run
 * to run, wherever the row lies and whatever else is in the batch.  The tables of a (device, fft_length, frame_length) are built
 * and uploaded on first use (that call allocates and copies); afterwards no allocation and no host synchronisation.
 * Returns -1 with a message, launching nothing, for a NULL required pointer, R outside 1 .. 4, an unsupported size, B outside
 * 1 .. 65535, Lpad outside 1 .. 2^31 - 65537, a row stride below Lpad when B > 1, grad_dev without both weight arrays, a workspace
 * that is not 16-byte aligned; -4 for a workspace smaller than the workspace entry says (same B, Lpad, resolutions, want_grad).
 *
 * mi355asr_vad_mask_stats: one launch (one workgroup) over labels and logits f32, element (b, t) at labels_dev + b * ld_lab + t and
 * logits_dev + b * ld_x + t, t < counts_dev[b] (i32 [B], NULL: T; clamped to 0 .. T; nothing at or past it is read).  With
 * loss = max(x, 0) - x z + log1p(exp(-|x|)), one = (z == 1), zero = (z == 0), float64 / int64 sums in a fixed order:
 *   sums_dev f64 [4]       = sum loss * one, sum one, sum loss * zero, sum zero      (mask_loss: [0] / ([1] + 1e-6), [2] / ([3] + 1e-6))
 *   counts_out_dev i64 [4] = TP, FP, FN, TN of the decision x > threshold (the raw logit, as binary_accuracy has it)
 *   grad_dev (may be NULL; row b at grad_dev + b * ld_grad) = d (one_loss + zero_loss) / d x, 0 from counts_dev[b] on. */
int mi355asr_stft_loss_workspace_bytes(int32_t B, int64_t Lpad, int32_t R, const int32_t* fft_lengths, const int32_t* frame_lengths,
                                       const int32_t* frame_steps, int32_t want_grad, size_t* bytes);
int mi355asr_stft_loss(const float* truth_dev, int64_t ld_truth, const float* pred_dev, int64_t ld_pred, const int32_t* len_dev,
                       int32_t B, int64_t Lpad, int32_t R, const int32_t* fft_lengths, const int32_t* frame_lengths,
                       const int32_t* frame_steps, float* sc_dev, float* mag_dev, int32_t* frames_dev, const float* w_sc_dev,
                       const float* w_mag_dev, float* grad_dev, int64_t ld_grad, void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_vad_mask_stats(const float* labels_dev, int64_t ld_lab, const float* logits_dev, int64_t ld_x, const int32_t* counts_dev,
                            int32_t B, int32_t T, float threshold, double* sums_dev, int64_t* counts_out_dev, float* grad_dev,
                            int64_t ld_grad, void* stream);

/* replaces: ctc_beam_search_decoder_batch(probs_split, vocabulary, beam_size, num_processes, cutoff_prob,
 * cutoff_top_n, ext_scorer = nullptr) of externals/ctc_decoders (ctc_beam_search_decoder.cpp:18-187, 426-459;
 * SWIG entry decoders.i) -- the CTC prefix beam search without a scorer (with one: mi355asr_ctc_prefix_beam_lm* below).  Blank = class V-1, vocabulary = classes
 * 0..V-2 (as the reference assigns blank_id = vocabulary.size()).  Token ids are returned instead of the
 * concatenated vocabulary strings.  Outputs are HOST buffers: ids i32 [B, beam, max_len] (-1 padded, hypotheses
 * best first), lens i32 [B, beam], scores f32 [B, beam] (log prob), n_hyp i32 [B] (number of valid hypotheses).
 * Reference quirk kept: with cutoff_prob == 1.0 no class is pruned, whatever cutoff_top_n says
 * (decoder_utils.cpp:18-31).
 *   _host : probs_host f32 [B, T, V] on the host; everything runs on the CPU threads (model-independent helper,
 *           also what the unit tests pin against the reference's own decoder).
 *   device: x_dev f32 [B, T, V] logits (is_logits != 0: softmax is fused into the selection kernel) or
 *           probabilities; the per-frame top-cutoff_top_n selection runs on the GPU, the prefix search on
 *           prefix search on the device as well (beam_device.hip: one workgroup per utterance, the beam in LDS; beam_size
 *           <= 128, cutoff_top_n <= 40, ws_dev of mi355asr_ctc_prefix_beam_workspace_bytes) or, failing those, on
 *           `num_threads` host threads.  Needs cutoff_prob < 1 and cutoff_top_n <= 128 (otherwise use _host).
 *           Synchronises `stream` (the results are host arrays).
 *           ws_dev: at least B*T*cutoff_top_n*8 bytes (host search); mi355asr_ctc_prefix_beam_workspace_bytes for the
 *           device search. */
int mi355asr_ctc_prefix_beam_host(const float* probs_host, const int32_t* in_len_host, int32_t B, int32_t T, int32_t V,
                                  int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                  int32_t max_len, int32_t* ids_host, int32_t* lens_host, float* scores_host,
                                  int32_t* n_hyp_host);
int mi355asr_ctc_prefix_beam(const float* x_dev, int32_t is_logits, const int32_t* in_len_host, int32_t B, int32_t T,
                             int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n,
                             int32_t num_threads, int32_t max_len, int32_t* ids_host, int32_t* lens_host,
                             float* scores_host, int32_t* n_hyp_host, void* ws_dev, size_t ws_bytes, void* stream);

/* The score arithmetic of the device prefix search, exposed for verification.  The reference's scores are defined by the
 * C library it is compiled against: log_sum_exp<float> = logf(expf(x - m) + expf(y - m)) + m (zip:ctc_decoders/
 * decoder_utils.h:41-49) and (float)log((double)p + FLT_MIN) (ctc_beam_search_decoder.cpp:57-59); the device search
 * evaluates glibc's own algorithms (csrc/refmath.h).  kind 0: out f32[i] = expf(in[i]), in [-17.5, 0];
 * 1: out f32[i] = logf(in[i]), in [1, 2]; 2: out f64[i] = log((double)in[i] + FLT_MIN), in [0, 1];
 * 3: out f32[i] = log_sum_exp(in[i], in[n + i]) (in holds 2 n values).  Device pointers. */
/* Which search the last mi355asr_ctc_prefix_beam / mi355asr_ctc_prefix_beam_lm call of the CALLING THREAD ran: 0 none yet;
 * 1 the host search on the device's top-n lists (outside the device search's limits, a workspace below
 * mi355asr_ctc_prefix_beam*_workspace_bytes, or MI355ASR_BEAM_DEVICE=0); 2 the device search's one-key-per-thread kernel;
 * 3 its radix kernel; 4 the device search with a scorer; 5, 6, 7: mi355asr_beam_streams_step (below).  All of them return the same arrays, so this is the only way to
 * tell them apart; it is set on the host from the conditions that choose the launch.
 * mi355asr_beam_device_limits: the limits those conditions use -- the device search serves V <= max_classes, beam_size <=
 * max_beam, min(cutoff_top_n, V) <= max_top_n; without a scorer the one-key-per-thread kernel runs when beam_size <=
 * small_beam and beam_size * (min(N, beam_size + 2) + 1) <= 256 with N = min(cutoff_top_n, V) (small_beam is 0 with one). */
int32_t mi355asr_beam_last_path(void);
int mi355asr_beam_device_limits(int32_t with_scorer, int32_t* max_classes, int32_t* max_beam, int32_t* max_top_n,
                                int32_t* small_beam);

int mi355asr_beam_math_eval(int32_t kind, const float* in_dev, void* out_dev, int32_t n, void* stream);

/* Stateful prefix beam search for streaming recognition.
 * replaces: class BeamDecoder (zip:ctc_decoders/ctc_beam_search_decoder.h: BeamDecoder(vocabulary, beam_size,
 * cutoff_prob, cutoff_top_n, ext_scorer = nullptr), .decode(probs_seq), .reset(); .cpp:217-405).  decode() consumes
 * T more frames, continuing from the prefix trie the previous calls left, and returns the current beam (best
 * first) -- feeding an utterance in pieces gives the result of feeding it whole.  As in the reference class, the
 * vocabulary INCLUDES the blank as its last entry: probs rows have V = num_classes entries, blank = V-1 (:238-240).
 * Host-side (the trie search is branchy integer work); probs_host f32 [T, V]; outputs as in
 * mi355asr_ctc_prefix_beam_host for one utterance: ids i32 [beam, max_len], lens i32 [beam], scores f32 [beam]. */
int mi355asr_ctc_prefix_beam_workspace_bytes(int32_t B, int32_t T, int32_t cutoff_top_n, int32_t beam_size, int32_t max_len,
                                             size_t* bytes);

typedef struct mi355asr_beam mi355asr_beam;
int mi355asr_beam_create(int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, mi355asr_beam** out);
int mi355asr_beam_decode(mi355asr_beam* d, const float* probs_host, int32_t T, int32_t max_len, int32_t* ids_host,
                         int32_t* lens_host, float* scores_host, int32_t* n_hyp_host);
int mi355asr_beam_reset(mi355asr_beam* d);
int mi355asr_beam_destroy(mi355asr_beam* d);
/* a copy of the decoder as it stands (trie, frame count, scorer reference): feeding the copy leaves the original untouched --
 * how a caller looks at provisional frames */
int mi355asr_beam_clone(const mi355asr_beam* d, mi355asr_beam** out);

/* The external scorer of the prefix beam search: a back-off n-gram language model in CHARACTER-BASED mode.
 * replaces: Scorer(alpha, beta, lm_path, vocab_list) of externals/ctc_decoders (scorer.h, scorer.cpp; KenLM behind
 * get_log_cond_prob, scorer.cpp:74-93) as ctc_beam_search_decoder.cpp:64-73, 84-86, 111-128 use it.  The word-based mode
 * (a dictionary FST over OpenFST) is not built.  The ARPA file is read by the caller (tensorflowasr_amd/ngram.py); the
 * library takes the model as LM-word ids: 0 = out of vocabulary, 1 .. counts[0] = the unigrams.
 *   mi355asr_lm_create: order 1 .. 6; counts i64 [order]; words i32 = for m = 1 .. order, counts[m-1] n-grams of m ids each
 *     (w_1 .. w_m, w_m the predicted word); logp / backoff f32, one per n-gram in the same sequence (log10, as KenLM keeps
 *     them; the back-off of the highest order is ignored); class_word i32 [n_classes]: acoustic class -> LM word, 0 for a
 *     class the model does not know (and for "<unk>"); bos_word: the id of "<s>" (0: none); space_class: the " " class or
 *     -2 -- make_ngram stops at a space and leaves empty words behind it (scorer.cpp:164-194), so a space among the last
 *     `order` tokens scores OOV_SCORE, which is what mapping it to word 0 does.  The n-grams are packed once into one
 *     open-addressed table keyed by 64 bits of the ids (csrc/lm_table.h; a repeated key is MI355ASR_EINVAL), shared by the
 *     host and the device search, uploaded to a device on first use and read-only afterwards.
 *   mi355asr_lm_score: for verification (as mi355asr_beam_math_eval): out[i] = get_log_cond_prob of the i-th of n n-grams
 *     (i32 [n, order], w_1 .. w_order, "<s>"-padded by the caller, 0 = OOV) as the float KenLM returns: OOV_SCORE = -1000 when
 *     any word is OOV, else logp of the longest stored suffix + the back-offs of the contexts backed off from, shortest
 *     first, added in float.  HOST pointers; on_device != 0 evaluates them in a kernel with the device search's own routine.
 *   mi355asr_ctc_prefix_beam_lm_host / _lm / mi355asr_beam_create_lm: the three searches above with (lm, alpha, beta):
 *     float score = (float)(cond * alpha); log_p += score; log_p += beta (float += double) for every new or re-reached
 *     prefix, log10 values used as they are; the per-frame min_cutoff / full_beam pruning of the scorer path; the returned
 *     scores include the LM terms.  lm NULL is the scorer-less search.  lm must have n_classes = V - 1.  The device search
 *     serves beam_size <= 128, cutoff_top_n <= 40, order <= 6 (ws_dev of mi355asr_ctc_prefix_beam_lm_workspace_bytes);
 *     anything else, or MI355ASR_BEAM_DEVICE=0, runs the host search on the device's top-n lists. */
typedef struct mi355asr_lm mi355asr_lm;
int mi355asr_lm_create(int32_t order, const int64_t* counts, const int32_t* words, const float* logp, const float* backoff,
                       const int32_t* class_word, int32_t n_classes, int32_t bos_word, int32_t space_class, mi355asr_lm** out);
int mi355asr_lm_destroy(mi355asr_lm* lm);
int mi355asr_lm_score(const mi355asr_lm* lm, const int32_t* ngrams_host, int32_t n, float* out_host, int32_t on_device,
                      void* stream);
int mi355asr_ctc_prefix_beam_lm_host(const float* probs_host, const int32_t* in_len_host, int32_t B, int32_t T, int32_t V,
                                     int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                     int32_t max_len, const mi355asr_lm* lm, double alpha, double beta, int32_t* ids_host,
                                     int32_t* lens_host, float* scores_host, int32_t* n_hyp_host);
int mi355asr_ctc_prefix_beam_lm(const float* x_dev, int32_t is_logits, const int32_t* in_len_host, int32_t B, int32_t T,
                                int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, int32_t num_threads,
                                int32_t max_len, const mi355asr_lm* lm, double alpha, double beta, int32_t* ids_host,
                                int32_t* lens_host, float* scores_host, int32_t* n_hyp_host, void* ws_dev, size_t ws_bytes,
                                void* stream);
int mi355asr_ctc_prefix_beam_lm_workspace_bytes(int32_t B, int32_t T, int32_t cutoff_top_n, int32_t beam_size, int32_t max_len,
                                                size_t* bytes);
int mi355asr_beam_create_lm(int32_t V, int32_t beam_size, double cutoff_prob, int32_t cutoff_top_n, const mi355asr_lm* lm,
                            double alpha, double beta, mi355asr_beam** out);

/* encoder + CTCDecoder + greedy in one call: wav [B,L] -> ids i32 [B,T_total] (-1 padded), out_len i32 [B].
 * This is the timed region of bench.py (offline_stt steps 3-5, test_asr.py:191-198). */
int mi355asr_recognize(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L, const int32_t* in_len_dev,
                       int32_t* ids_dev, int32_t* out_len_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- Ragged batches: utterances of different lengths in one call ----------------------------------------------
 * wav_dev f32 [B, L] holds utterance b in its first wav_len[b] samples (the rest of the row is never read); wav_len_dev i32 [B]
 * on the device, 1 <= wav_len[b] <= L.  Row b of every output equals what the call without lengths returns for
 * wav[b, :wav_len[b]] alone: the STFT frames each utterance with its own TF 'SAME' padding, the dB maximum covers its own
 * frames, the subsampling convs pad by its own lengths, attention sees only its T_b = ceil(ceil(ceil(wav_len[b] / hop) / 2) / 2)
 * frames and the depthwise conv reads zeros past them.  Rows t >= T_b are written as defined values: encoder output 0, logits 0,
 * frame argmax -1; ids are -1 padded as usual.  Workspace: that of [B, L] (mi355asr_workspace_bytes; ctc: ctc_workspace_bytes).
 * Each call reads the lengths back to check them (synchronises `stream` once, at entry).
 * Supported: the Melspectrogram frontend on the FFT STFT (mi355asr_stft_mode 1), chunk_size 0, add_wav_info 0, gemm_dtype 0,
 * dmodel 144, reduction_factor 4, head_size 36 and kernel_size 32 wherever the model has blocks (recognize_ragged: also
 * ctcdecoder_kernel_size 32), more than 16 encoder frames in a row of L samples (pad L when every utterance is shorter), and
 * the default kernel switches; anything else returns MI355ASR_EINVAL with a message (mi355asr_last_error), checked before any
 * launch except for kernel switches, which are checked where the block reaches them.
 * ctc_forward_ragged and translator_forward_ragged also take dmodel 256 with 64-dim heads and a ConvModule kernel size of 32, in fp32 and (the CTC decoder) in the
 * bf16 GEMM mode (the streaming configuration's global CTC decoder over per-stream histories): every utterance's attention runs
 * on the kernel its solo call takes.  encoder_forward_ragged and recognize_ragged do not.
 *   encoder_forward_ragged: enc_out_dev f32 [B, T(L), dmodel]; enc_len_dev i32 [B] receives T_b (may be NULL)
 *   ctc_forward_ragged:     enc_dev [B, T, dmodel] with enc_len_dev i32 [B] (1 <= enc_len[b] <= T) frames per utterance
 *   recognize_ragged:       the greedy collapse of utterance b stops at min(T_b, in_len[b]) (in_len_dev may be NULL) */
int mi355asr_encoder_forward_ragged(mi355asr_model* m, const float* wav_dev, const int32_t* wav_len_dev, int32_t B, int32_t L,
                                    float* enc_out_dev, int32_t* enc_len_dev, void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_ctc_forward_ragged(mi355asr_model* m, const float* enc_dev, const int32_t* enc_len_dev, int32_t B, int32_t T,
                                float* logits_dev, int32_t* frame_argmax_dev, void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_recognize_ragged(mi355asr_model* m, const float* wav_dev, const int32_t* wav_len_dev, int32_t B, int32_t L,
                              const int32_t* in_len_dev, int32_t* ids_dev, int32_t* out_len_dev, void* ws_dev, size_t ws_bytes,
                              void* stream);

/* ---- Streaming server: per-stream encoder histories on the device ---------------------------------------------
 * hist_dev f32 [N, Tcap, d] holds hist_len[s] rows of slot s; the lengths live on the device (hist_len_dev i32 [N]) and in a
 * host copy the caller keeps (hist_len_host), on which every check is made before anything is launched.  slot_dev / slot_host:
 * the M distinct slots of the call, on the device and on the host.
 *   stream_append: chunk_dev f32 [M, Tc, d] goes behind row hist_len[slot[m]] of slot[m]; both copies of the lengths advance
 *                  by Tc.  MI355ASR_EINVAL when a slot lies outside [0, N), appears twice or would overflow Tcap.
 *   stream_gather: out_dev f32 [M, Tpad, d] receives the history of slot[m], behind it the first tail_len[m] rows of
 *                  tail_dev f32 [M, Tc_tail, d] (all three tail arguments NULL: none; tail_len 0: none for that row; the tail
 *                  is not stored), zeros after that; out_len_dev i32 [M] the row counts.  Tpad >= every count; the ragged CTC
 *                  call wants Tpad >= 17.  One launch each. */
int mi355asr_stream_append(const float* chunk_dev, const int32_t* slot_dev, const int32_t* slot_host, int32_t M, int32_t Tc,
                           int32_t d, float* hist_dev, int32_t* hist_len_dev, int32_t* hist_len_host, int32_t N, int32_t Tcap,
                           void* stream);
int mi355asr_stream_gather(const float* hist_dev, const int32_t* hist_len_dev, const int32_t* hist_len_host, int32_t N,
                           int32_t Tcap, int32_t d, const int32_t* slot_dev, const int32_t* slot_host, int32_t M,
                           const float* tail_dev, const int32_t* tail_len_dev, const int32_t* tail_len_host, int32_t Tc_tail,
                           float* out_dev, int32_t* out_len_dev, int32_t Tpad, void* stream);

/* Stage-level entry points (same kernels the calls above run; exposed so that the parity tests can
 * localise a mismatch to one reference layer):
 *   melspectrogram   Melspectrogram.call (time_frequency.py:173-189): wav [B,L] -> mel [B,F,n_mels]
 *   conv_subsampling ConvSubsampling.call (conformer_blocks.py:90-96): mel [B,F,n_mels] -> [B,T,d]
 *   conformer_block  ConformerBlock.call (conformer_blocks.py:259-265) of block `index` of the encoder
 *                    (stack 0) or the CTCDecoder (stack 1): x [B,T,d] -> y [B,T,d] */
int mi355asr_melspectrogram(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L, float* mel_dev,
                            void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_conv_subsampling(mi355asr_model* m, const float* mel_dev, int32_t B, int32_t F, float* out_dev,
                              void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_conformer_block(mi355asr_model* m, int32_t stack, int32_t index, const float* x_dev, int32_t B,
                             int32_t T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- ChunkConformer (asr/models/chunk_conformer_blocks.py:775-822, offline `predict`) ---------------------------
 * front (valid-padded Melspectrogram + left-padded VALID ConvSubsampling, :400-445, :23-70) -> ChunkConformerEncoder
 * (band attention [i-win_front, i+win_back], causal depthwise conv, :142-398, :462-560) -> phone_picker
 * (ChunkCTCDecoder :571-637) -> feature_pick (keep frames whose phone argmax is not the blank, :913-999) ->
 * ContextHelper (:679-770) -> text ChunkCTCDecoder -> logits [B, T_pick, num_classes].
 * Values from asr/configs/chunk_conformerS.yml.  All sub-models share dmodel / heads / kernel size here. */
typedef struct {
  int32_t dmodel, head_size, num_heads, kernel_size;      /* 144, 36, 4, 32                                 */
  float   fc_factor;                                      /* 0.5                                            */
  int32_t n_mels, sample_rate, stride_ms, n_dft;          /* 80, 16000, 10, 1024                            */
  int32_t reduction_factor;                               /* 4                                              */
  int32_t enc_num_blocks, enc_win_front, enc_win_back;    /* 15, 36, 0                                      */
  int32_t picker_num_classes, picker_num_blocks, picker_win_front, picker_win_back;   /* phone+1, 1, 36, 0 */
  int32_t helper_num_blocks, helper_win_front, helper_win_back;                       /* 2, 36, 0          */
  int32_t decoder_num_classes, decoder_num_blocks, decoder_win_front, decoder_win_back; /* txt+1, 1, 36, 8 */
} mi355asr_chunk_config;

/* optional DEVICE outputs of mi355asr_chunk_predict (NULL = not wanted).  Frame-major fp32 unless noted;
 * T = encoder frames of the utterances, Tp = max over the batch of picked frames (returned on the host).  The four buffers
 * with a capacity receive a dense [B, Tp, ...] block at their start; the rest of the capacity is not written. */
typedef struct {
  float*   front_out;       /* [B, T, d]                    ChunkConformerFront.call                      */
  float*   enc_out;         /* [B, T, d]                    ChunkConformerEncoder.call                    */
  float*   picker_logits;   /* [B, T, picker_num_classes]   phone_picker(...)[0]                          */
  float*   picker_hidden;   /* [B, T, d]                    phone_picker(...)[1]                          */
  float*   picked;          /* [B, >=Tp, d] (capacity B*T*d) feature_pick(...)[0], zero padded            */
  float*   helper_out;      /* [B, >=Tp, d] (capacity B*T*d) helper(picked)                               */
  float*   text_logits;     /* [B, Tp, decoder_num_classes] (capacity B*T*V) ChunkConformer.predict       */
  int32_t* text_argmax;     /* i32 [B, Tp] (capacity B*T)   per-frame argmax of text_logits               */
} mi355asr_chunk_outputs;

/* replaces: ChunkConformer(config, phone, txt) construction (test_chunk_asr.py:40-55).  The handle takes
 * weights through mi355asr_load_weight / mi355asr_finalize_weights like the other models (names: DESIGN.md). */
int mi355asr_chunk_create(const mi355asr_chunk_config* cfg, mi355asr_model** out);
int mi355asr_chunk_out_frames(const mi355asr_model* m, int32_t L, int32_t* mel_frames, int32_t* enc_frames);
int mi355asr_chunk_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes);
/* replaces: ChunkConformer.predict(x) (chunk_conformer_blocks.py:815-822).  wav_dev f32 [B, L].
 * n_picked_host i32 [B] and t_pick_host i32 [1] are HOST outputs (the picked-frame counts size the second half of
 * the network, so the call synchronises `stream` once in the middle, as the reference's dynamic shapes do). */
int mi355asr_chunk_predict(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L,
                           const mi355asr_chunk_outputs* outs, int32_t* n_picked_host, int32_t* t_pick_host,
                           void* ws_dev, size_t ws_bytes, void* stream);
/* Ragged ChunkConformer batches: utterance b is wav_dev[b, :wav_len_dev[b]] (i32 [B] on the device,
 * 2 hop + 1 <= wav_len[b] <= L; what lies behind it in the row is never read into a result -- it may hold anything).  Row b of
 * every output equals the call on that utterance alone: the band attention of every stack takes the utterance's own length
 * (T_b = chunk_out_frames(wav_len[b]) for encoder and picker, its pick count for helper and decoder), frames past T_b are never
 * picked, and n_picked_host[b] is the valid length of its text logits.  Rows past T_b of front_out / enc_out / picker_logits /
 * picker_hidden and rows past n_picked[b] of picked / helper_out / text_logits are 0, text_argmax is -1 there.  The lengths
 * are read back at entry (one more synchronisation of `stream`).  EINVAL, before anything is launched: a length outside
 * its range (the message names the row), a null wav_len_dev, a handle that is not a ChunkConformer, bf16 GEMM mode.
 * Workspace: mi355asr_chunk_workspace_bytes_ragged(B, L). */
int mi355asr_chunk_workspace_bytes_ragged(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes);
int mi355asr_chunk_predict_ragged(mi355asr_model* m, const float* wav_dev, const int32_t* wav_len_dev, int32_t B, int32_t L,
                                  const mi355asr_chunk_outputs* outs, int32_t* n_picked_host, int32_t* t_pick_host,
                                  void* ws_dev, size_t ws_bytes, void* stream);

/* per-frame argmax of given logits or probabilities, f32 [M, V] -> i32 [M], first maximum wins: the decision step of
 * tf.keras.backend.ctc_decode(greedy) when the logits come from outside a head kernel (the streaming ChunkConformer path
 * concatenates logits of several calls, test_chunk_asr.py:84-96); feed the result to mi355asr_ctc_greedy. */
int mi355asr_frame_argmax(const float* x_dev, int32_t M, int32_t V, int32_t* out_dev, void* stream);

/* replaces: ChunkConformer.feature_pick(encoder_hidden_states, ctc_outs[, max_T]) (chunk_conformer_blocks.py:913-999), the
 * "length regulator" between the phone picker and the text decoder of the streaming path (test_chunk_asr.py:72-75): keep
 * the frames whose phone argmax is not the blank (class V - 1), compacted per utterance, zero padded to the batch maximum.
 * Handle-free, two calls because the batch maximum sizes the outputs (a dynamic shape in the reference):
 *   _count:  ctc_dev f32 [B, T, V] -> idx_dev i32 [B, T] (kept frame indices), cnt_dev i32 [B], counts_host i32 [B];
 *            synchronises the stream once to return the counts
 *   _gather: hidden_dev f32 [B, T, d], ctc_dev -> feat_out_dev f32 [B, Tp, d], ctc_out_dev f32 [B, Tp, V] (or NULL)
 *            for any Tp >= max(counts) (max_T of the reference) */
int mi355asr_feature_pick_count(const float* ctc_dev, int32_t B, int32_t T, int32_t V, int32_t* idx_dev, int32_t* cnt_dev,
                                int32_t* counts_host, void* stream);
int mi355asr_feature_pick_gather(const float* hidden_dev, const float* ctc_dev, const int32_t* idx_dev,
                                 const int32_t* cnt_dev, int32_t B, int32_t T, int32_t d, int32_t V, int32_t Tp,
                                 float* feat_out_dev, float* ctc_out_dev, void* stream);

/* ---- ChunkConformer streaming: one stream, explicit caches ------------------------------------------
 * replaces the pieces of ChunkConformer.picker_stream_predict / decoder_stream_predict (chunk_conformer_blocks.py:
 * 824-866, ONNX form :868-898).  The caller owns every cache tensor and does the slicing the reference does in
 * Python (valid / unvalid split by win_back, caches cut to the last win_front / kernel_size rows, dec_inp carry);
 * tensorflowasr_amd.models.ChunkConformer.{init_picker_caches, picker_stream_predict, init_decoder_caches,
 * decoder_stream_predict, feature_pick} is that code.  All tensors are device f32, row-major, batch 1.
 *
 * front_stream: ChunkConformerFront.stream_call (:447-458) + ConvSubsampling.stream_call (:72-91).
 *   wav_dev [Lw] = [front_wav_cache ; new samples]; sub_cache_dev [S, n_mels]
 *   -> new_sub_dev [S + nf, n_mels] = [sub cache ; last nf mel frames], front_out_dev [t_out, d]
 *   (nf = min(mel frames of the buffer, chunk_num), t_out = min(frames after the two stride-2 convs, chunk_num /
 *   reduction_factor): mi355asr_chunk_front_stream_shape).
 * stack_stream: ChunkConformerEncoder (stack 0) / phone picker ChunkCTCDecoder (1) / ContextHelper (2) / text
 *   ChunkCTCDecoder (3) .stream_call (:530-560, 641-672, 750-770) up to (not including) the valid/unvalid slicing:
 *   x_dev [T, d] (picker / decoder: dec_inp rows followed by the new rows; `project` is applied inside),
 *   mha_cache_dev [num_blocks, Cm, d], cnn_cache_dev [num_blocks, Cc, d]
 *   -> hidden_dev [T, d] (block-stack output), logits_dev [T, num_classes] / argmax_dev i32 [T] (stacks 1, 3; NULL =
 *   not wanted), new_mha_dev [num_blocks, Cm + T, d], new_cnn_dev [num_blocks, Cc + T, d] = [cache ; module input]
 *   per block, untrimmed.  Band attention is evaluated with the queries as the last T rows of the Cm + T keys. */
int mi355asr_chunk_front_stream_shape(const mi355asr_model* m, int32_t Lw, int32_t S, int32_t chunk_num, int32_t* nf,
                                      int32_t* t_out);
/* max_rows = largest (cache rows + T) of any stack_stream call; Lw, S, chunk_num as for front_stream */
int mi355asr_chunk_stream_workspace_bytes(const mi355asr_model* m, int32_t max_rows, int32_t Lw, int32_t S,
                                          int32_t chunk_num, size_t* bytes);
int mi355asr_chunk_front_stream(mi355asr_model* m, const float* wav_dev, int32_t Lw, const float* sub_cache_dev,
                                int32_t S, int32_t chunk_num, float* front_out_dev, float* new_sub_dev, void* ws_dev,
                                size_t ws_bytes, void* stream);
int mi355asr_chunk_stack_stream(mi355asr_model* m, int32_t stack, const float* x_dev, int32_t T,
                                const float* mha_cache_dev, int32_t Cm, const float* cnn_cache_dev, int32_t Cc,
                                float* hidden_dev, float* logits_dev, int32_t* argmax_dev, float* new_mha_dev,
                                float* new_cnn_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- ChunkConformer streaming: many streams per call, state on the device --------------------------------------
 * One call advances every stream that has a packet by that packet; stream b's results are those of the single-stream
 * calls above (picker_stream_predict -> feature_pick -> decoder_stream_predict) on its own audio, whatever else shares
 * the call.  A stream lives in a SLOT (0 .. n_streams - 1) of an opaque state buffer the caller allocates on the device;
 * between calls everything a stream needs stays there (wav and sub caches, per block the projected keys / values and
 * the GLU rows of the last win_front / kernel_size frames, the decoder rows that wait for right context).
 * A packet is wav_buf_length = 16 * hop samples; a stream's LAST packet may be shorter (n_samples_host), its first may
 * not.  Supported: what chunk_conformerS.yml ships -- chunk_num 16, win_back 0 for encoder / picker / helper, win_back
 * <= 16 for the text decoder, fp32; anything else is MI355ASR_EINVAL before anything is launched, as are a slot out of
 * range or named twice and a packet length outside 1 .. wav_buf_length.  The step makes no host synchronisation: its
 * integer results are device arrays the caller reads back with one copy.
 * Outputs (device, NULL = not wanted), n = streams of the call, TPd = decoder win_back + 4: */
typedef struct {
  int32_t* phone_argmax;    /* i32 [n, 4]        per-frame argmax of the phone picker                               */
  int32_t* n_picked;        /* i32 [n]           frames of the call the picker did not call blank                   */
  int32_t* text_argmax;     /* i32 [n, TPd]      per-frame argmax of the text decoder: valid rows, then unvalid     */
  int32_t* n_valid;         /* i32 [n]           text rows that are final (0 when nothing was picked)               */
  int32_t* n_unvalid;       /* i32 [n]           text rows that will be run again with more right context           */
  float*   phone_logits;    /* f32 [n, 4, picker_num_classes]                                                       */
  float*   text_logits;     /* f32 [n, TPd, decoder_num_classes]  rows past n_valid + n_unvalid are padding         */
  float*   picker_hidden;   /* f32 [n, 4, d]                                                                        */
} mi355asr_chunk_streams_outputs;
/* bytes of the state buffer for n_streams slots and of the workspace of a step over up to n_streams streams */
int mi355asr_chunk_streams_bytes(const mi355asr_model* m, int32_t n_streams, size_t* state_bytes, size_t* ws_bytes);
/* the n slots of slots_host (NULL: all n_streams) become fresh streams; a new state buffer is reset as a whole first */
int mi355asr_chunk_streams_reset(mi355asr_model* m, void* state_dev, int32_t n_streams, const int32_t* slots_host,
                                 int32_t n, void* stream);
/* packets_dev f32 [n, wav_buf_length] (row i: the packet of slot slots_host[i], the rest of a short one is ignored);
 * n_samples_host i32 [n] or NULL (every packet full) */
int mi355asr_chunk_streams_step(mi355asr_model* m, void* state_dev, int32_t n_streams, const int32_t* slots_host,
                                int32_t n, const float* packets_dev, const int32_t* n_samples_host,
                                const mi355asr_chunk_streams_outputs* outs, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- prefix beam search for many live streams, state on the device ---------------------------------------------
 * The stateful search of the mi355asr_beam handle, with or without a scorer, for n_streams streams at once, a few frames per call:
 * stream b's result after k committed frames is that of the one-shot search over those k frames, whatever else shares the
 * call.  A stream lives in a SLOT of a state buffer the caller allocates on the device: its beam in rank order, with a
 * scorer every entry's LM history and own LM term, and a back-pointer arena of max_frames * beam_size + 1 cells
 * (bytes per slot: 16 + beam_size * 36 (60 with a scorer) rounded up to 16, + 8 * (max_frames * beam_size + 1) rounded up
 * to 16).  A new state buffer is reset as a whole first.
 * A step gives stream i = slot slots_host[i] the rows x_dev[i, 0 .. n_commit_dev[i]) as FINAL frames, followed by
 * n_peek_dev[i] PROVISIONAL frames (NULL: none): the reported beam is the one after all of them, the state keeps the beam
 * after the final ones only -- a peek leaves no trace (what the text decoder's "unvalid" rows need: they are run again with
 * more right context).  Both counts are DEVICE arrays, clamped to 0 .. T and 0 .. T - n_commit; rows behind them are padding
 * and may hold anything.  A stream whose committed + commit + peek frames exceed max_frames consumes nothing, keeps its
 * state, reports its unchanged beam and status 1 (decided on the device; a reset makes the slot usable again).
 * There is NO host fallback: a configuration outside mi355asr_beam_device_limits (for the scorer or scorer-less search), a
 * cutoff_prob outside (0, 1), a slot out of range or named twice, n_best outside 1 .. beam_size or a workspace below
 * mi355asr_beam_streams_bytes is MI355ASR_EINVAL / MI355ASR_EWORKSPACE before anything is launched.  The step makes no host
 * synchronisation (a scorer is uploaded to the device once, on its first use); mi355asr_beam_last_path reports 5 (radix
 * kernel), 6 (with a scorer) or 7 (one key per thread: beam_size <= small_beam, scorer-less) for it.
 * Outputs (device), n = streams of the call: */
typedef struct {
  int32_t* ids;             /* i32 [n, n_best, max_len]  best first, padded with -1, cut at max_len                   */
  int32_t* lens;            /* i32 [n, n_best]           full lengths                                                 */
  float*   scores;          /* f32 [n, n_best]           -FLT_MAX where there is no hypothesis                        */
  int32_t* n_hyp;           /* i32 [n]                   min(entries of the beam, n_best)                             */
  int32_t* frames;          /* i32 [n]                   frames committed after the call                              */
  int32_t* status;          /* i32 [n]                   0 ok, 1 over capacity                                        */
} mi355asr_beam_streams_outputs;
/* bytes of the state for n_streams slots and of the workspace of a step over up to n_streams streams of up to T_max rows */
int mi355asr_beam_streams_bytes(int32_t n_streams, int32_t V, int32_t beam_size, int32_t cutoff_top_n, int32_t max_frames,
                                const mi355asr_lm* lm_or_null, int32_t T_max, size_t* state_bytes, size_t* ws_bytes);
/* the n slots of slots_host (NULL: all n_streams) become fresh streams */
int mi355asr_beam_streams_reset(void* state_dev, int32_t n_streams, int32_t V, int32_t beam_size, int32_t cutoff_top_n,
                                int32_t max_frames, const mi355asr_lm* lm_or_null, const int32_t* slots_host, int32_t n,
                                void* stream);
/* x_dev f32 [n, T, V] probabilities, or logits with is_logits (blank = class V - 1) */
int mi355asr_beam_streams_step(void* state_dev, int32_t n_streams, int32_t V, int32_t beam_size, double cutoff_prob,
                               int32_t cutoff_top_n, int32_t max_frames, const mi355asr_lm* lm_or_null, double alpha,
                               double beta, const int32_t* slots_host, int32_t n, const float* x_dev, int32_t is_logits,
                               const int32_t* n_commit_dev, const int32_t* n_peek_dev, int32_t T, int32_t n_best,
                               int32_t max_len, const mi355asr_beam_streams_outputs* outs, void* ws_dev, size_t ws_bytes,
                               void* stream);

/* ---- Translator: phoneme ids + encoder output -> text logits -------------------------------
 * replaces: Translator(inp_classes, tar_classes, dmodel, num_blocks, head_size, num_heads, kernel_size, dropout,
 * fc_factor) (test_asr.py:76-84; conformer_blocks.py:505-548): Embedding(inp_classes -> d) -> num_blocks x RBlock
 * (FFModule -> cross-attention with q = LN(x + sinusoid PE), k = v = encoder output -> ConvModule -> FFModule -> LN)
 * -> Dense(d -> tar_classes).  Weight names: inp_embedding/embeddings, decoder_conformer_block_<i>/... (as the
 * ConformerBlock), fully_connected/{kernel,bias}. */
typedef struct {
  int32_t dmodel, num_blocks, head_size, num_heads, kernel_size;
  float   fc_factor;
  int32_t inp_classes, tar_classes;
} mi355asr_translator_config;
int mi355asr_translator_create(const mi355asr_translator_config* cfg, mi355asr_model** out);
/* U = token positions per utterance (padded CTC output), T = encoder frames per utterance */
int mi355asr_translator_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t U, int32_t T, size_t* bytes);
/* replaces: translator([ctc_decode, enc_outputs], training=False) and tf.argmax(., -1) (test_asr.py:202-203,
 * streaming :149-150).  ids_dev i32 [B, U] (values clamped to [0, inp_classes)), enc_dev f32 [B, T, d];
 * logits_dev f32 [B, U, tar_classes] or NULL, argmax_dev i32 [B, U] or NULL (first maximum wins). */
int mi355asr_translator_forward(mi355asr_model* m, const int32_t* ids_dev, const float* enc_dev, int32_t B,
                                int32_t U, int32_t T, float* logits_dev, int32_t* argmax_dev, void* ws_dev,
                                size_t ws_bytes, void* stream);
/* ragged batches (see "Ragged batches" above): utterance b has tok_len_dev[b] tokens (1 <= tok_len[b] <= U; the solo call's
 * width is its own decoded length) and enc_len_dev[b] encoder frames (1 <= enc_len[b] <= T); both i32 [B] on the device.
 * Cross-attention keys past enc_len[b] are excluded, the ConvModule reads zeros from token row tok_len[b] on, and rows past
 * tok_len[b] hold logits 0 / argmax -1.  Row b equals mi355asr_translator_forward on ids[b, :tok_len[b]] and
 * enc[b, :enc_len[b]].  dmodel 144; U > 16 and T > 16 (pad both); workspace of mi355asr_translator_workspace_bytes(B, U, T). */
int mi355asr_translator_forward_ragged(mi355asr_model* m, const int32_t* ids_dev, const int32_t* tok_len_dev,
                                       const float* enc_dev, const int32_t* enc_len_dev, int32_t B, int32_t U, int32_t T,
                                       float* logits_dev, int32_t* argmax_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- Voice-activity detector: waveform -> one score per 10 ms frame ------------------------------------------
 * replaces: VAD.inference on Inference/PythonInference/vad/models/vad.onnx (offline_asr_session.py OfflineVAD.vad,
 * CppInference asr_session.cpp Session::VadInference).  A frame is 80 samples of 8 kHz audio; decimate = 2 takes
 * every second sample of 16 kHz input in the kernel (wav[::2]), decimate = 1 reads 8 kHz input as it is.
 * Network per frame: dense -> dense_1 + ReLU -> conv1d (k 5, causal zero pad on the activations) + ReLU ->
 * dense_2 + ReLU -> LayerNorm (eps 1e-3) -> conv1d_1 (k 5, causal) + ReLU -> dense_3 + ReLU -> dense_4; a frame
 * depends on itself and the 8 frames before it.  Speech: score >= 0 (offline session) or > -0.1 (C++ gate).
 * Weight names and layouts (fp32, tf2onnx graph names):
 *   dense/kernel, dense_1/kernel, dense_2/kernel, dense_3/kernel  [80 in, 80 out]   + <name>/bias [80]
 *   conv1d/kernel, conv1d_1/kernel  [5 taps, 80 in, 80 out] (tap 4 is the current frame) + <name>/bias [80]
 *   layer_normalization/gamma, layer_normalization/beta  [80]
 *   dense_4/kernel [80, 1], dense_4/bias [1]
 * load with mi355asr_load_weight, then mi355asr_finalize_weights; mi355asr_destroy frees the handle. */
typedef struct {
  int32_t dmodel;     /* 80 */
  int32_t frame;      /* 80 samples (after decimation) per frame */
  int32_t decimate;   /* 1 or 2 */
} mi355asr_vad_config;
int mi355asr_vad_create(const mi355asr_vad_config* cfg, mi355asr_model** out);
/* T = floor(L / (80 * decimate)) frames for L input samples */
int mi355asr_vad_frames(const mi355asr_model* m, int32_t L, int32_t* T);
/* always 0 today (every activation stays on chip); kept so a caller can size a workspace if that changes */
int mi355asr_vad_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t L, size_t* bytes);
/* wav_dev f32 [B, L]; in_len_dev i32 [B] samples per row or NULL (every row has L); scores_dev f32 [B, T] with
 * T = mi355asr_vad_frames(L).  Row b gets floor(min(in_len[b], L) / (80 * decimate)) scores; samples past a row's
 * length are never read and score entries past its frame count are not written. */
int mi355asr_vad_forward(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L, const int32_t* in_len_dev,
                         float* scores_dev, void* stream);

/* ---- Speech enhancement from the online VAD's voice-mask head ------------------------------------------------
 * replaces: the second output of vad/online_vad_model (the SavedModel's online_cnn_vad call): after dense_3 + ReLU,
 * mask = dense_3 @ audio_voice_mask/kernel + audio_voice_mask/bias (linear, no activation), enhanced = frame * mask.
 * An enhancer handle takes the 16 weights above plus
 *   audio_voice_mask/kernel [80 in, 80 out], audio_voice_mask/bias [80]
 * (tensorflowasr_amd/vad.py VAD.load_saved_model maps the SavedModel's variables to these names).
 * mi355asr_vad_forward works on an enhancer handle and returns the same scores as on a scores-only one. */
int mi355asr_vad_enhancer_create(const mi355asr_vad_config* cfg, mi355asr_model** out);
/* One launch: scores and enhanced frames.  wav_dev / in_len_dev as mi355asr_vad_forward; scores_dev f32 [B, T] or
 * NULL (not written); enhanced_dev f32 [B, T * 80] with T = mi355asr_vad_frames(L).  The mask multiplies the samples
 * the network reads, so the enhanced output is 8 kHz audio, 80 samples per frame, whatever the decimation: with
 * decimate = 2 it is the enhanced wav[::2] of 16 kHz input (resampling back to 16 kHz is the caller's).  Row b gets
 * floor(min(in_len[b], L) / (80 * decimate)) * 80 samples; nothing past that is written.  MI355ASR_EINVAL on a
 * handle from mi355asr_vad_create. */
int mi355asr_vad_enhance(mi355asr_model* m, const float* wav_dev, int32_t B, int32_t L, const int32_t* in_len_dev,
                         float* scores_dev, float* enhanced_dev, void* stream);

/* ---- Punctuation restoration: token ids -> class probabilities per token --------------------------------------
 * replaces: Punc.punc_recover's onnxruntime session on Inference/PythonInference/punc_recover/models/punc.onnx
 * (PuncTransformer.inference of punc_recover/models/punc_transformer.py).  Per sentence of T ids (<S> first, </S> last):
 *   x = embedding[id] * sqrt(d_model) + pos_encoding[:T];  x = ELU(x W + b)
 *   num_layers times: x = x + ReLU(causal Conv1D k=3 (EncoderLayer(x)))
 *   x = (x W19 + b19) W20 + b20 (64 -> 768 -> 64, no activation between);  max(num_layers - 1, 1) more EncoderLayers
 *   probs = softmax(x Wf + bf)
 * EncoderLayer (post-LN, eps 1e-6): out1 = LN1(x + dense(MHA(x))), out2 = LN2(out1 + W2 relu(W1 out1)); 8 heads of 8, logits
 * scaled by 1 / sqrt(8), -1e9 added at a key whose id is 0.  One launch per ragged batch, one workgroup per sentence.
 * Weight names (fp32, Keras layouts; <L> = encoder/layer_<i>, i < num_layers, or map/layer_<i>, i < max(num_layers - 1, 1)):
 *   embedding [vocab, 64], pos_encoding [pe_input, 64], encoder/dense/{kernel [64, 64], bias [64]}
 *   <L>/mha/{wq,wk,wv,dense}/{kernel [64, 64], bias [64]}, <L>/ffn/{dense_1,dense_2}/{kernel [64, 64], bias [64]}
 *   <L>/layernorm1/{gamma,beta} [64], <L>/layernorm2/{gamma,beta} [64]
 *   encoder/conv_<i>/kernel [3 taps, 64 in, 64 out] (tap 2 is the current token), encoder/conv_<i>/bias [64]
 *   to_bert/kernel [64, 768], to_bert/bias [768], to_hidden/kernel [768, 64], to_hidden/bias [64]
 *   final/kernel [64, classes], final/bias [classes]
 * load with mi355asr_load_weight, then mi355asr_finalize_weights; mi355asr_destroy frees the handle. */
typedef struct {
  int32_t d_model;             /* 64 */
  int32_t enc_embedding_dim;   /* 64 */
  int32_t num_heads;           /* 8 */
  int32_t dff;                 /* 64 */
  int32_t num_layers;          /* 1 .. 6 */
  int32_t vocab;               /* rows of the embedding table */
  int32_t classes;             /* <= 64 */
  int32_t pe_input;            /* rows of pos_encoding, <= 1024: the longest sentence */
} mi355asr_punc_config;
int mi355asr_punc_create(const mi355asr_punc_config* cfg, mi355asr_model** out);
/* lds_tokens: the longest sentence whose activations stay in LDS; max_tokens = pe_input: the longest sentence at all */
int mi355asr_punc_limits(const mi355asr_model* m, int32_t* lds_tokens, int32_t* max_tokens);
/* 0 for T <= lds_tokens; beyond that one activation region per sentence */
int mi355asr_punc_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes);
/* ids_dev i32 [B, T]; len_dev i32 [B] tokens per row (clamped to [0, T]) or NULL (every row has T); probs_dev f32
 * [B, T, classes]; cls_dev i32 [B, T] (arg-max class, the lowest on a tie) and pmax_dev f32 [B, T] (its probability), either may
 * be NULL.  Row b is computed as if it were alone: ids at or past len[b] are never keys, and every output at or past len[b] is
 * written as 0.  An id outside [0, vocab) is clamped into the table.  A row of more than lds_tokens tokens keeps its
 * activations in the workspace, whatever T and B are.  T > max_tokens is MI355ASR_EINVAL before anything is launched. */
int mi355asr_punc_forward(mi355asr_model* m, const int32_t* ids_dev, const int32_t* len_dev, int32_t B, int32_t T,
                          float* probs_dev, int32_t* cls_dev, float* pmax_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* The model's training outputs: PuncTransformer.call([inp, mask], training=False) as PuncTrainer._eval_step runs it (no dropout).
 * ids_dev, len_dev, B, T, the workspace and the limits as in mi355asr_punc_forward (the workspace entry returns the same size).
 *   logits_dev f32 [B, T, classes] (may be NULL): bd_output, the values mi355asr_punc_forward takes its softmax of; they go
 *     through the folded 64 x 64 matrix as inference does.
 *   feature_dev f32 [B, T, 768] (may be NULL): bert_out = to_bert(enc_output) from the unfolded to_bert/kernel [64, 768] and its
 *     bias, exact fp32 on the MFMA.
 * At least one of the two is non-NULL (else MI355ASR_EINVAL, before anything is launched).  Rows at or past len[b] are written as
 * zeros (the reference computes values there; every loss below masks them).  A row's result depends on its own length alone.
 * mi355asr_punc_forward on the same handle is not affected: same kernel, same bits as before. */
int mi355asr_punc_heads_workspace_bytes(const mi355asr_model* m, int32_t B, int32_t T, size_t* bytes);
int mi355asr_punc_heads(mi355asr_model* m, const int32_t* ids_dev, const int32_t* len_dev, int32_t B, int32_t T,
                        float* logits_dev, float* feature_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* replaces: PuncTrainer.classes_loss, classes_acc and bert_feature_loss (punc_recover/trainer/punc_trainer.py:93-126) with the
 * gradients with respect to the model's two outputs.  Model-independent (csrc/punc_loss.hip).
 *
 * mi355asr_punc_classes_loss: label (b, t) at labels_dev + b * ld_lab + t (i32, Q columns), logit (b, t, c) at logits_dev +
 * b * ld_b + t * ld_t + c (f32, T tokens, C <= 64 classes, unit stride over c).  The first Q' = min(T, Q) columns of both are
 * used.  With xe = logsumexp(logits) - logits[label], m = (label != 0), m1 = m * (label != 1), N = sum m, N1 = sum m1:
 *   loss_dev f32 [B]    = sum(xe m) / (N + 1e-6) + sum(xe m1) / (N1 + 1e-6)
 *   acc_dev f32 [B]     = sum((argmax == label) m) / N -- no epsilon, as the reference has none: NaN for a row without a label;
 *                         ties go to the lowest index
 *   acc_mean_dev f32 [1] = the mean of acc_dev over the batch (classes_acc)
 *   grad_dev (may be NULL; (b, t, c) at grad_dev + b * gld_b + t * gld_t + c, every element of [B, T, C] written) =
 *     upstream[b] * (m / (N + 1e-6) + m1 / (N1 + 1e-6)) * (softmax - onehot); upstream_dev f32 [B] or NULL (ones); zeros for
 *     t >= Q', where label == 0 and where the label is outside [0, C) (there the loss is NaN, as in mi355asr_xent_rows).
 * The logits of a token whose label is 0 are not read.  One launch (one workgroup per row, a lane per token; the lane walks its
 * token's row twice for the loss and once more for the gradient, out of L1), then a one-wave launch for the batch mean.  C > 64 is MI355ASR_EINVAL.
 *
 * mi355asr_masked_feature_mse: real (b, t, f) at real_dev + b * rld_b + t * rld_t + f (T1 tokens), pred likewise with pld_b,
 * pld_t (T2 tokens); F >= 1 features with unit stride, rows need not be aligned (aligned rows are read 16 bytes per lane).
 * T = min(T1, T2), k = (real != -10) per element (an exact float compare), cnt = sum_f k:
 *   out_dev f32 [B] = mean over t < T of sum_f (real - pred)^2 k / (cnt + 1e-6); a token without an unmasked element counts in
 *     the mean with 0, as in the reference
 *   grad_dev (may be NULL; (b, t, f) at grad_dev + b * gld_b + t * gld_t + f, every element of [B, T2, F] written) =
 *     upstream[b] * 2 (pred - real) k / ((cnt + 1e-6) T); 0 for t >= T and where real == -10.
 * ws_dev: mi355asr_masked_feature_mse_workspace_bytes(B, T1, T2) bytes, 8-byte aligned (the row values, float64).
 * Both: every sum is float64 in a fixed order without atomics; a row of a batch gives the bits it gives alone.  No allocation,
 * no host synchronisation.  -1 with a message, launching nothing, for a NULL required pointer, a size below 1, B * T >= 2^31 -
 * 65536 or strides that let rows overlap; -4 for a workspace that is too small. */
int mi355asr_punc_classes_loss(const int32_t* labels_dev, int64_t ld_lab, const float* logits_dev, int64_t ld_b, int64_t ld_t,
                               const float* upstream_dev, int32_t B, int32_t Q, int32_t T, int32_t C, float* loss_dev,
                               float* acc_dev, float* acc_mean_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* stream);
int mi355asr_masked_feature_mse_workspace_bytes(int32_t B, int32_t T1, int32_t T2, size_t* bytes);
int mi355asr_masked_feature_mse(const float* real_dev, int64_t rld_b, int64_t rld_t, const float* pred_dev, int64_t pld_b,
                                int64_t pld_t, const float* upstream_dev, int32_t B, int32_t T1, int32_t T2, int32_t F,
                                float* out_dev, float* grad_dev, int64_t gld_b, int64_t gld_t, void* ws_dev, size_t ws_bytes,
                                void* stream);

/* ---- Polyphase resampling (scipy.signal.resample_poly, default Kaiser filter) ------------------------------------
 * replaces: the host resampling of utils/speech_featurizers.py read_raw_audio (librosa.load at another rate).
 * A ratio up / down (sr_out / sr_in in lowest terms, max(up, down) <= 640; anything else is MI355ASR_EINVAL naming it) has
 * half = 10 max(up, down) and a filter h of 2 half + 1 taps that the CALLER designs (tensorflowasr_amd/resample.py
 * design_filter) and hands over as a 16-byte aligned fp32 device table in phase-major order:
 *   table[p * stride + m] = h[p + m * up] for p < up, m < taps, where p + m * up < 2 half + 1; 0 elsewhere,
 * table_floats floats in all; taps, stride, table_floats and the kernel's output tile come from mi355asr_resample_plan.
 * Output k of a row of L samples is sum_m table[p][m] x[jh - m] with c = k down + half, p = c mod up, jh = c div up and
 * x = 0 outside [0, L): one fp32 FMA chain over m = 0 .. taps - 1, the same in every entry point below. */
int mi355asr_resample_plan(int32_t up, int32_t down, int32_t* taps, int32_t* stride, int32_t* tile, int32_t* table_floats);
/* x_dev [B, Lpad] of dtype MI355ASR_DT_F32 or MI355ASR_DT_I16 (converted as x / 32768, exact: the same bits as the
 * float input); in_len_dev i32 [B] samples per row (clamped to [0, Lpad]); y_dev f32 [B, Opad].  Row b gets
 * ceil(in_len[b] up / down) outputs, computed as if the row were alone; samples at or past in_len[b] are never read;
 * columns past the row's output length (or all of Opad, if that is smaller) are written as 0.  Asynchronous on `stream`. */
int mi355asr_resample(const void* x_dev, int32_t dtype, const int32_t* in_len_dev, int32_t B, int64_t Lpad, int32_t up,
                      int32_t down, const float* filt_dev, float* y_dev, int64_t Opad, void* stream);
/* Many live streams, one launch per step.  state_dev (state_bytes, caller-owned) holds per slot a ring of
 * taps - 1 + max_packet samples; a stream's position (samples taken so far, 64-bit) is the CALLER's: pos_host[i] for the
 * slot slots_host[i].  After N samples a stream has emitted E(N) = max(0, floor((N up - half - 1) / down) + 1) outputs,
 * those whose taps are all final, so a step over a packet of n_in_host[i] <= max_packet samples (x_dev f32 [n, Ppad])
 * writes E(N + n_in) - E(N) outputs to row i of y_dev f32 [n, out_cap] (the rest of the row is not written) and that
 * count to n_out_host[i]; with
 * flush != 0 (x_dev, n_in_host unused) it writes the rest up to ceil(N up / down), zero-extended, after which the slot
 * must be reset.  Concatenated, a stream's outputs equal mi355asr_resample of its concatenated input bit for bit.
 * reset: slots_host NULL = every slot.  A slot out of range or named twice, a packet above max_packet or Ppad, an
 * out_cap below the one mi355asr_resample_streams_bytes returns, or a workspace below ws_bytes is MI355ASR_EINVAL /
 * MI355ASR_EWORKSPACE before anything is launched.  No call waits for the device. */
int mi355asr_resample_streams_bytes(int32_t up, int32_t down, int32_t n_streams, int32_t max_packet, size_t* state_bytes,
                                    size_t* ws_bytes, int32_t* out_cap);
int mi355asr_resample_streams_reset(void* state_dev, int32_t up, int32_t down, int32_t n_streams, int32_t max_packet,
                                    const int32_t* slots_host, int32_t n, void* stream);
int mi355asr_resample_streams_step(void* state_dev, int32_t up, int32_t down, int32_t n_streams, int32_t max_packet,
                                   const float* filt_dev, const int32_t* slots_host, const int64_t* pos_host,
                                   const int32_t* n_in_host, int32_t n, int32_t flush, const float* x_dev, int32_t Ppad,
                                   float* y_dev, int32_t out_cap, int32_t* n_out_host, void* ws_dev, size_t ws_bytes,
                                   void* stream);

/* ---- Far-field simulation: image-source room impulse responses, reverberation, noise at a given SNR ----------------
 * replaces: augmentations/augments.py -- SignalRIR (rir_generator.generate + scipy.signal.convolve), SignalNoise.Add_noise
 * and the clip / 16-bit quantisation of Augmentation.process.  Stateless, like mi355asr_resample.
 *
 * mi355asr_rir_generate: B impulse responses by the image-source method (Habets' rir_generator: omnidirectional
 * microphone, 3-D, unlimited reflection order; DESIGN.md section 19 spells the definition out).  params_host is f64
 * [B, 20], copied by the call: room L[3], source s[3], receiver r[3] in metres; sound speed c (m/s); sample rate fs;
 * reverberation_time in seconds (> 0: all six reflection coefficients are sqrt(1 - alpha), alpha = 24 V ln 10 / (c S T);
 * <= 0: the six coefficients that follow are used); beta[6] in the order x1 x2 y1 y2 z1 z2; hp_filter (0 or 1); nsample.
 * h_dev f32 [B, Kpad]: row b holds its nsample samples and zeros after them.  Distances, fractional delays, the gains and
 * the sums are float64; a row is the same bits in every run and in every batch (no atomics: each output sample adds its
 * images in image order).  ws_dev holds the call's device table (mi355asr_rir_workspace_bytes, 8-byte aligned).
 * One generator launch for all B rows, followed by one launch of the float64 high-pass recurrence when a row asks for it.
 * Refused as MI355ASR_EINVAL before anything is launched: nsample outside 1 .. min(16384, Kpad); a position outside
 * [0, L]; the source at the receiver; alpha > 1; |beta| > 1; a window 2 round(0.004 fs) above 1024 taps; more than 255
 * images per side on an axis (ceil(nsample / (2 L fs / c))). */
int mi355asr_rir_workspace_bytes(int32_t B, size_t* ws_bytes);
int mi355asr_rir_generate(const double* params_host, int32_t B, float* h_dev, int32_t Kpad, void* ws_dev, size_t ws_bytes,
                          void* stream);
/* Full convolution of a ragged batch: x_dev [B, Lpad] of dtype MI355ASR_DT_F32 or MI355ASR_DT_I16 (converted as x / 32768),
 * in_len_dev i32 [B] (clamped to [0, Lpad]), h_dev f32 [B, Kpad] -- or [1, Kpad], one filter for every row, when
 * shared_filter != 0 -- of which K taps (1 .. 16384) are used, y_dev f32 [B, Opad].  Row b gets in_len[b] + K - 1 outputs
 * (scipy.signal.convolve(x, h, mode="full")), a row of length 0 none; columns past the row's output length (or all of
 * Opad, if that is smaller) are written as 0.  Samples at or past in_len[b] and taps at or past K are never read.  A row
 * is computed as if it were alone.  Exact fp32 products summed in fp32 (v_mfma_f32_16x16x4_f32):
 * |y[n] - y64[n]| <= (K + 2) 2^-23 sum_k |h[k]| |x[n - k]|.  Asynchronous on `stream`. */
int mi355asr_fir_ragged(const void* x_dev, int32_t dtype, const int32_t* in_len_dev, int32_t B, int64_t Lpad,
                        const float* h_dev, int32_t K, int64_t Kpad, int32_t shared_filter, float* y_dev, int64_t Opad,
                        void* stream);
/* y = x + g d per row, g = float32(sqrt(P_x / 10^(snr_db / 10) / P_d)) with P_x = sum x^2, P_d = sum d^2 over the row's
 * len[b] samples (clamped to [0, Lpad]), both in float64: x_dev f32 [B, Lpad], d_dev f32 [B, Dpad] (Dpad >= Lpad; len[b]
 * samples of a row are read), snr_db_dev f32 [B], y_dev f32 [B, Lpad] (zeros past len[b]; may be x_dev).  P_x == 0 or
 * P_d == 0 gives g = 0, y = x (the reference divides by zero there).  quantise != 0 applies Augmentation.process's last
 * step, trunc(clamp(y, -1, 1) * 32768) / 32768 (truncation toward zero, exact in fp32).  Before quantisation
 * |y - y64| <= 2^-23 (|x| + 2 |g64 d|).  One launch, asynchronous on `stream`. */
int mi355asr_mix_snr(const float* x_dev, const int32_t* len_dev, const float* d_dev, const float* snr_db_dev, int32_t B,
                     int64_t Lpad, int64_t Dpad, int32_t quantise, float* y_dev, void* stream);

/* ---- Ragged STFT / ISTFT pair, spec_aug and the phase vocoder ---------------------------------------------------------
 * replaces: librosa.stft / librosa.istft / librosa.phase_vocoder (librosa 0.9: center=True, pad_mode="reflect", a periodic
 * Hann window of win_length zero-padded on both sides to n_fft) as augmentations/augments.py calls them in SignalSpecAug and,
 * through librosa.effects.time_stretch, in SignalSpeed.  Stateless.  (n_fft, win_length, hop) is (1024, 800, 160) or
 * (2048, 2048, 512); anything else is MI355ASR_EINVAL.  Both DFT stages of both directions run on v_mfma_f32_16x16x4_f32 with
 * stage matrices computed in float64; the overlap-add is owner-computes in ascending frame order; there are no atomics: a
 * row is the same bits in every run and in every batch.  The tables of a size are uploaded to the current device on the
 * first call that uses it (one hipMalloc and one blocking copy) and kept for the life of the process.  DESIGN.md section 20.
 *
 * mi355asr_stft_frames: frames of a row of n_samples: 1 + n_samples / hop, or 0 when n_samples < n_fft / 2 + 1 (reflect
 * padding needs that many; librosa raises there).
 * mi355asr_stft_ragged: x_dev [B, Lpad] of dtype MI355ASR_DT_F32 or MI355ASR_DT_I16 (x / 32768), len_dev i32 [B] (clamped
 * to [0, Lpad]) -> S_dev complex64 [B, Fpad, n_fft / 2 + 1] interleaved, frame-major (librosa's layout transposed); frames
 * at or past the row's count are zeros; a row with more than Fpad frames is cut at Fpad.  frames_dev i32 [B] (may be null)
 * receives the counts.  Samples at or past len[b] are never read.  One launch.
 * mi355asr_istft_ragged: S_dev as above with frames_dev i32 [B] -> y_dev f32 [B, Opad]: irfft of each frame (1 / n_fft
 * included), times the window, overlap-added, divided by the window's sum of squares where that exceeds tiny(float32), the
 * first n_fft / 2 samples dropped.  Row b gets out_len_dev[b] samples (librosa.istft(..., length=); zeros where no frame
 * reaches) or, with out_len_dev null, hop (frames[b] - 1); zeros after them.  The imaginary parts of bins 0 and n_fft / 2 are
 * ignored.  ws_dev (16-byte aligned) holds the windowed frames, B Fpad win_length floats.  Two launches.
 * mi355asr_spec_aug: SignalSpecAug at (1024, 800, 160) without the spectrum in memory: every frame goes forward, has the
 * bins [max(h_ - window, 0), h_ + window) zeroed for every centre (h_, w_) of its row with max(w_ - window, 0) <= frame <
 * w_ + window, and comes back, on chip; its windowed samples go to ws_dev and are overlap-added by a second launch.
 * centres_dev i32 [B, Npad, 2] holds (h_, w_) pairs, counts_dev i32 [B] how many of a row's are used.  y_dev f32 [B, Opad]:
 * row b gets 160 (len[b] / 160) samples; a row with fewer than 513 samples is copied through (len[b] samples).  With no
 * centres the result is that of stft_ragged followed by istft_ragged, bit for bit.  The counts are read back before anything
 * is launched (the call waits for `stream` once): a count above 513 (the reference's random.sample raises there) or above
 * Npad, or a negative window, is MI355ASR_EINVAL.
 * mi355asr_phase_vocoder: librosa.phase_vocoder on S_dev / frames_dev: row b is resampled in time by rates_host[b]
 * (float64; the time steps t * rate are float64) into out_frames_host[b] <= Tpad frames of O_dev complex64 [B, Tpad,
 * n_fft / 2 + 1]; zeros after them.  The expected phase advance is reduced modulo 2 pi in float64 on the host and the
 * accumulated phase is kept in [-pi, pi].  Both host arrays are copied by the call into ws_dev.  One launch. */
int mi355asr_stft_frames(int32_t n_fft, int32_t win_length, int32_t hop, int64_t n_samples, int32_t* frames);
int mi355asr_stft_ragged(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad, int32_t n_fft,
                         int32_t win_length, int32_t hop, float* S_dev, int32_t Fpad, int32_t* frames_dev, void* stream);
int mi355asr_istft_workspace_bytes(int32_t B, int32_t Fpad, int32_t n_fft, int32_t win_length, int32_t hop, size_t* ws_bytes);
int mi355asr_istft_ragged(const float* S_dev, const int32_t* frames_dev, int32_t B, int32_t Fpad, int32_t n_fft,
                          int32_t win_length, int32_t hop, const int32_t* out_len_dev, float* y_dev, int64_t Opad,
                          void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_spec_aug_workspace_bytes(int32_t B, int64_t Lpad, size_t* ws_bytes);
int mi355asr_spec_aug(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad,
                      const int32_t* centres_dev, int32_t Npad, const int32_t* counts_dev, int32_t window, float* y_dev,
                      int64_t Opad, void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_phase_vocoder_workspace_bytes(int32_t B, size_t* ws_bytes);
int mi355asr_phase_vocoder(const float* S_dev, const int32_t* frames_dev, int32_t B, int32_t Fpad, int32_t n_fft,
                           int32_t win_length, int32_t hop, const double* rates_host, const int32_t* out_frames_host,
                           float* O_dev, int32_t Tpad, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- Ragged recursive (IIR) filters on second-order sections, and SignalMask -------------------------------------------
 * replaces: scipy.signal.sosfilt / scipy.signal.sosfiltfilt per row, and with them augmentations/augments.py's SignalHz
 * (scipy.signal.filtfilt of a 3rd-order Butterworth band-stop, plus uniform noise) and SignalMask.  Stateless.
 *
 * mi355asr_sos_ragged: x_dev [B, Lpad] of dtype MI355ASR_DT_F32 or MI355ASR_DT_I16 (x / 32768), len_dev i32 [B] (clamped to
 * [0, Lpad]); sos_dev f64 [B, S, 6] -- or [1, S, 6], one filter for every row, when shared != 0 -- in SciPy's layout
 * (b0 b1 b2 a0 a1 a2), 1 <= S <= 8; y_dev f32 [B, Opad].
 *   mode 0: sosfilt(sos, x, zi=zi) per row.  zi_dev f64 [B, S, 2] (null: the zero state); zf_dev f64 [B, S, 2] (may be
 *   null) receives the final state, which is zi for an empty row.  padlen is ignored.
 *   mode 1: sosfiltfilt(sos, x, padtype="odd", padlen=padlen) per row, 0 <= padlen <= 1024: the odd extension (2 x[0] -
 *   x[padlen .. 1], the row, the mirrored tail) is built inside the kernels; each pass starts from sosfilt_zi(sos) times
 *   its first sample; forward, reversed, forward, reversed, the edges stripped.  zi_dev and zf_dev must be null
 *   (MI355ASR_EINVAL otherwise).  A row with 0 < len <= padlen (SciPy raises there) is copied through, with the finish
 *   below applied.
 * The finish of a row: noise_dev f64 [B, Npad] (Npad >= Lpad), when not null, is added as y + noise_scale * noise in
 * float64 (product and sum each rounded once); quantise != 0 applies trunc(clamp(y, -1, 1) * 32768) / 32768 to the
 * float64 value; the result is rounded to float32 once.  Columns at or past len[b] (up to Opad) are written as 0.
 * Samples and noise at or past len[b] are never read.
 * All recursion arithmetic is float64 in direct form II transposed, one section at a time.  A row is cut into chunks of
 * mi355asr_sos_chunk() samples at fixed positions of the extended row; a chunk's initial state comes from a sequential
 * walk over the chunks' zero-state results with the chunk's 2 x 2 transition, itself obtained by running the recursion.
 * No atomics: a row is the same bits in every run, in every batch and at every batch position.  Against a long-double
 * evaluation y_ld of the same sections: |y - y_ld| <= 2^-24 |y_ld| + 8 D per sample, D = max |scipy - y_ld| over the row
 * (at least 2^-50 max |x|); DESIGN.md section 21 has what was measured.
 * The sections are read back before anything is launched (the call waits for `stream` once): a0 != 1 in any section is
 * MI355ASR_EINVAL, as are S outside 1 .. 8, a null required pointer and padlen outside 0 .. 1024; y_dev is not touched
 * then.  ws_dev (16-byte aligned, mi355asr_sos_workspace_bytes) holds the float64 intermediate signal and the chunk
 * states.  Launches: 2 S + 1 in mode 0, 4 S + 2 in mode 1.
 *
 * mi355asr_mask_zone: SignalMask.augment per row: s = (int)(len zone_lo), e = (int)(len zone_hi) (float64 products,
 * truncated; 0 <= zone <= 1); for s <= n < e with u = u_dev[b, n - s] (f64 [B, Upad]; Upad must cover e - s, a sample
 * whose n - s is at or past Upad is left as it is): y = x m + (with_noise ? u (1 - m) : 0) in float64 with m = u <
 * mask_ratio ? 0 : 1 -- the reference's expressions, so u where masked (0 without noise) and x elsewhere; outside the
 * zone y = x.  Then the optional quantisation as above, one rounding to float32, zeros past len[b].  Exact: equal to the
 * NumPy expressions bit for bit.  One launch. */
int32_t mi355asr_sos_chunk(void);
int mi355asr_sos_workspace_bytes(int32_t B, int64_t Lpad, int32_t S, int32_t mode, size_t* ws_bytes);
int mi355asr_sos_ragged(const void* x_dev, int32_t dtype, const int32_t* len_dev, int32_t B, int64_t Lpad,
                        const double* sos_dev, int32_t S, int32_t shared, int32_t mode, int32_t padlen,
                        const double* zi_dev, double* zf_dev, const double* noise_dev, int64_t Npad, double noise_scale,
                        int32_t quantise, float* y_dev, int64_t Opad, void* ws_dev, size_t ws_bytes, void* stream);
int mi355asr_mask_zone(const float* x_dev, const int32_t* len_dev, const double* u_dev, int32_t B, int64_t Lpad,
                       int64_t Upad, double zone_lo, double zone_hi, double mask_ratio, int32_t with_noise,
                       int32_t quantise, float* y_dev, void* stream);

/* ---- Band-limited resampling at any real ratio, one ratio per row ----------------------------------------------------------
 * replaces: resampy.resample(x, sr_in, sr_out, filter="kaiser_best") per row as librosa.effects.pitch_shift calls it, with
 * librosa's fix_length behind it.  It follows the published algorithm (J. O. Smith's band-limited interpolation on a tabulated
 * Kaiser-windowed sinc: 64 zero crossings, 512 entries per crossing, linear interpolation between entries); it has NOT been
 * compared with the resampy or librosa packages, and the filter's four constants are quoted from resampy's documentation.
 * Stateless.
 *
 * mi355asr_sinc_plan: tile = outputs per workgroup tile; wing = taps per wing at most at `ratio`, 32769 / (int)(min(1, ratio)
 * 512); table_floats = floats of the table (32 772: win[0 .. 32768] in natural order, then three copies of win[32768]);
 * ratio_min, ratio_max = the supported ratios, both inclusive (0.25 and 4).  tile, table_floats and the bounds are written
 * whatever `ratio` is; a ratio that is not finite or outside the bounds is MI355ASR_EINVAL and leaves *wing alone.
 *
 * mi355asr_sinc_resample: x_dev f32 [B, Lpad]; on the host: ratios f64 [B] (sr_out / sr_in), len i64 [B] (0 .. Lpad),
 * out_len i64 [B] (null: ceil(len ratio), the product in float64), off i64 [B] (may be null), valid i64 [B] (may be null:
 * receives min(floor(len ratio), out_len), the outputs that are computed).  y_dev f32 [B, Opad].  With s = min(1, ratio)
 * and step = (int)(512 s), output t < valid of a row is, with pos = t (1 / ratio) in float64, n = (int)pos, f = s (pos - n):
 *     sum_{i < min(n + 1, (32769 - o) / step)} w(o + i step) x[n - i],  o = (int)(512 f), w(j) = win[j] + (512 f - o) (win[j + 1] - win[j])
 *   + the same with f' = s - f over k < min(len - n - 1, (32769 - o') / step) and x[n + k + 1],
 * times ratio when ratio < 1.  pos, n, o and 512 f - o are float64 or integers; weights, products and the sum are fp32 FMAs in
 * that order into one accumulator: a row is the same bits alone, in any batch and in every run.  Outputs valid <= t <
 * out_len are 0 (fix_length).  off null: row b holds its out_len[b] outputs from column 0 and zeros up to Opad.  off given:
 * row b writes y[b, off[b] .. off[b] + out_len[b]) and nothing else of the row.  Samples at or past len[b] are never read.
 * table_mode 0 keeps the table in LDS (one 1024-thread workgroup of 150 KiB per CU), 1 reads it through the caches: the
 * same bits.  Against the float64 evaluation y64 of the same sums: |y - y64| <= 64 2^-24 sum_k |w_k x_k| per output.
 * Refused as MI355ASR_EINVAL before anything is launched or copied: B outside 1 .. 65535, Lpad or Opad < 1, a ratio that is
 * not finite or outside the bounds (named with the bounds), a length outside 0 .. Lpad, out_len < 0, off < 0 or off +
 * out_len > Opad, a null required pointer, a table that is not 16-byte aligned.  ws_dev (8-byte aligned,
 * mi355asr_sinc_workspace_bytes) receives the per-row parameters.  One launch, nothing is waited for. */
int mi355asr_sinc_plan(double ratio, int32_t* tile, int32_t* wing, int32_t* table_floats, double* ratio_min, double* ratio_max);
int mi355asr_sinc_workspace_bytes(int32_t B, size_t* ws_bytes);
int mi355asr_sinc_resample(const float* x_dev, int32_t B, int64_t Lpad, const double* ratios_host, const int64_t* len_host,
                           const int64_t* out_len_host, const int64_t* off_host, int64_t* valid_host, const float* table_dev,
                           int32_t table_mode, float* y_dev, int64_t Opad, void* ws_dev, size_t ws_bytes, void* stream);

/* ---- Ragged edit distance with the substitution / deletion / insertion split -------------------------------------------------
 * replaces: utils/xer.py:12-35 (`levenshtein`) and :211-220 (`wer`) per hypothesis / label pair, with the filtering
 * am_tester.py:34-89 does in front of it.  Stateless.
 *
 * ref_dev i32 [B, max_ref], hyp_dev i32 [B, max_hyp]; ref_len_dev / hyp_len_dev i32 [B] on the device, clamped to the row
 * width, null: the whole row counts.  Entries at or past a row's length are never read.  Per row, in this order: the
 * hypothesis is cut before the first hyp_stop (use_stop != 0); the ids of drop_hyp_host[0 .. n_drop_hyp) are removed from the
 * hypothesis and those of drop_ref_host[0 .. n_drop_ref) from the reference (host arrays of 0 .. 4 ids, read before the call
 * returns).  With u the n filtered reference tokens and v the m filtered hypothesis tokens the table is
 *     sub = prev[y-1] + (u != v), del = prev[y] + 1, ins = curr[y-1] + 1, best = min(sub, del, ins); the counts of a cell are
 *     those of the substitution predecessor if best == sub, else of the deletion predecessor if best == del, else of the
 *     insertion predecessor, plus the step; row 0 is all insertions, column 0 all deletions
 * and out_dev i32 [B, 4] receives (distance, S, D, I) of cell (n, m): n == 0 gives (m, 0, 0, m), m == 0 gives (n, 0, n, 0).
 * lens_dev i32 [B, 2] receives (n, m).  Integers: a row gives the same result alone, in any batch, at any position and in
 * every run.  ops_dev u8 [B, max_ref + max_hyp] and n_ops_dev i32 [B] (both or neither): the alignment behind the counts,
 * n_ops = n + I codes in forward order, 0 match, 1 substitution, 2 deletion, 3 insertion; the rest of the row is not written.
 * Refused as MI355ASR_EINVAL before anything is launched, outputs untouched: B, max_ref or max_hyp < 1; max_ref or max_hyp
 * above 16 384 (the counts are kept in 16 bits); with ops, max_ref * max_hyp above 2^24 cells; a drop set of more than 4 ids;
 * a null required pointer; a workspace that is not 8-byte aligned.  The workspace (mi355asr_edit_distance_workspace_bytes, each
 * part rounded up to 256 bytes) holds 16 B (max_ref + 1) bytes of strip boundary columns, 4 B (max_ref + max_hyp) bytes of
 * filtered rows and, with ops, 4 B ceil(max_ref / 16) max_hyp bytes of per-cell choices.  One launch, one workgroup per row,
 * nothing is waited for. */
int mi355asr_edit_distance_workspace_bytes(int32_t B, int32_t max_ref, int32_t max_hyp, int32_t want_ops, size_t* ws_bytes);
int mi355asr_edit_distance(const int32_t* ref_dev, const int32_t* ref_len_dev, const int32_t* hyp_dev, const int32_t* hyp_len_dev,
                           int32_t B, int32_t max_ref, int32_t max_hyp, const int32_t* drop_ref_host, int32_t n_drop_ref,
                           const int32_t* drop_hyp_host, int32_t n_drop_hyp, int32_t use_stop, int32_t hyp_stop, int32_t* out_dev,
                           int32_t* lens_dev, uint8_t* ops_dev, int32_t* n_ops_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream around each kernel (off by default).
 * profile_read waits for the recorded events, then returns accumulated milliseconds and launch counts per
 * kernel category below (arrays of at least MI355ASR_NUM_KERNELS); reset != 0 clears the accumulators.
 * bench.py uses this for the live `roofline.achieved` figure. */
#define MI355ASR_K_STFT 0         /* stft_kernel          Spectrogram conv2d x2 + power + log           */
#define MI355ASR_K_UTT_MAX 1      /* utt_max_kernel       per-sample max of the dB spectrogram          */
#define MI355ASR_K_MEL 2          /* mel_kernel           (dB-max).clamp(-80) @ freq2mel                */
#define MI355ASR_K_SUBCONV 3      /* subconv_kernel       Conv2D+ReLU -> Conv2D+ReLU (fused)            */
#define MI355ASR_K_SUBLINEAR 4    /* stream_gemm_kernel   Dense(F2*d -> d)                              */
#define MI355ASR_K_FFN 5          /* chain2_kernel mode 0 FFModule (+ block LayerNorm on the 2nd one)   */
#define MI355ASR_K_QKV 6          /* gemm_rows EPI_QKV    LN + q/k/v projections                        */
#define MI355ASR_K_ATTN 7         /* attention_kernel     softmax(q k^T) v                              */
#define MI355ASR_K_ATTN_OUT 8     /* gemm_rows EPI_RESIDUAL out-projection + residual                   */
#define MI355ASR_K_PW1_GLU 9      /* gemm_rows EPI_GLU    LN + pw_conv_1 + GLU                          */
#define MI355ASR_K_DWCONV 10      /* dwconv_kernel        depthwise conv                                */
#define MI355ASR_K_CONV_TAIL 11   /* chain2_kernel mode 1 pointwise + BN + swish + pw_conv_2 + residual */
#define MI355ASR_K_CTC_PROJECT 12 /* gemm_rows EPI_BIAS   CTCDecoder.project                            */
#define MI355ASR_K_CTC_HEAD 13    /* gemm_rows EPI_HEAD   fully_connected + per-frame argmax            */
#define MI355ASR_K_COLLAPSE 14    /* collapse_kernel      greedy merge/blank-drop                       */
#define MI355ASR_K_FF1_QKV 15     /* ff1_qkv_kernel       FFModule 1 + LN + q/k/v projections (fused, dmodel 144)     */
#define MI355ASR_K_OUT_GLU 16     /* out_glu_kernel       out-projection + residual + LN + pw_conv_1 + GLU (fused)    */
#define MI355ASR_K_TAIL_FF2 17    /* tail_ff2_kernel      ConvModule tail + FFModule 2 + block LayerNorm (fused)      */
#define MI355ASR_K_TAIL_FF1 18    /* tail_ff1_ld_kernel   tail_ff2 of block i + ff1_qkv of block i + 1 in one launch  */
#define MI355ASR_K_ENC_STACK 19   /* stream256_kernel     every ConformerBlock of the streaming encoder, one workgroup per chunk (bf16 mode) */
#define MI355ASR_NUM_KERNELS 20
int mi355asr_profile_enable(mi355asr_model* m, int32_t on);
/* Which arithmetic the LAST launch of each kernel category used (recorded whether or not timing is enabled; -1: the category
 * has not run on this handle).  Several kernels exist for most categories -- chosen by dmodel, row count, whether an operand
 * bound is known, and the MI355ASR_* experiment switches -- and they run on different pipes; whoever prices a kernel against
 * a roofline (bench.py) asks the library instead of re-deriving the choice. */
#define MI355ASR_SCHEME_F32 0     /* exact fp32 products: v_mfma_f32_16x16x4_f32 / fp32 VALU                           */
#define MI355ASR_SCHEME_BF16X3 1  /* fp32 operands as three bf16 terms, six bf16 MFMAs per fragment pair (exact to 2^-24) */
#define MI355ASR_SCHEME_F16X2 2   /* fp32 operands as two fp16 terms, three fp16 MFMAs per fragment pair (2^-22 of the bound) */
#define MI355ASR_SCHEME_BF16 3    /* operands rounded to bf16 (gemm_dtype = 1)                                         */
int mi355asr_profile_schemes(const mi355asr_model* m, int32_t* scheme_out, int32_t n);
int mi355asr_profile_read(mi355asr_model* m, double* ms_out, int64_t* count_out, int32_t n, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* MI355ASR_H */
