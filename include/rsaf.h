/*
 * rsaf.h — C ABI of librsaf.so (gfx950 / MI355X).
 *
 * The reference (ayushpradhan-dev/robust-speech-analysis-framework) is pure Python and has no
 * FFI/plugin registry; its hot path is reached through four Python callables and one nn.Module
 * (SURVEY.md §8b).  This header is the boundary a maintainer binds (ctypes) to
 * replace the third-party back-ends those callables drive.  Each entry point cites the reference
 * interface it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls enqueue work and
 *     return without synchronising unless stated otherwise;
 *   - return value: RSAF_OK (0) or an RSAF_ERR_* code; rsaf_last_error() gives the message of the
 *     calling thread's last failure; no exception crosses the boundary;
 *   - the caller owns every buffer; workspaces are sized with the matching *_workspace_bytes call;
 *   - plain C types only (no torch types).
 */
#ifndef RSAF_H
#define RSAF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSAF_OK 0
#define RSAF_ERR_ARG 1      /* bad argument / unsupported shape */
#define RSAF_ERR_HIP 2      /* a HIP runtime call failed */
#define RSAF_ERR_WORKSPACE 3 /* workspace too small */

#define RSAF_ABI_VERSION 7   /* 7: rsaf_gemm_f16x3 / rsaf_split_f16x2 / rsaf_f16x2_row_scales replace the bf16x6 entries (two fp16 planes with power-of-two row scales, three MFMA products).  6: params_host[18] of rsaf_mshds_pitch (per-depth Chebyshev tables behind sinc_cheb).  4: clip_info rows carry the sound's x1 / xmax (48 bytes); rsaf_resample_praat restates Sound_upsample for a rate ratio of 2.  5: the openSMILE-style chain is float64 end to end (lld / cand / functionals buffers are double) */

typedef void* rsaf_stream_t;

/* ---- library ------------------------------------------------------------------------------- */
int rsaf_abi_version(void);
const char* rsaf_last_error(void);
/* Upload the per-device constant tables (Hamming window, FFT twiddles, mel bank, DCT, ...).
 * Synchronous; called lazily by the first rsaf_smile_* call on a device otherwise. */
int rsaf_init_device(int device);

/* Per-kernel timing with HIP events on the launch stream (bench.py roofline object).
 * begin: start collecting; end: synchronise the recorded events and copy up to `cap` records.
 * A record accumulates all launches of one kernel family. */
typedef struct {
    char name[48];
    int64_t launches;
    double ms;        /* summed event time */
    double flops;     /* algorithmic FLOPs summed over launches (0 for byte-bound kernels) */
    double bytes;     /* algorithmic bytes summed over launches */
} rsaf_prof_record;
int rsaf_prof_begin(void);
int rsaf_prof_end(rsaf_prof_record* records_host, int cap, int* n_records_host);

/* ---- openSMILE-style chain ---------------------------------------------------------------------
 * Replaces the per-file SMILExtract subprocess of src/opensmile_extractor.py:62-75 driven by
 * Androids.conf:73-368 (cFramer .. cFunctionals), at the FILE'S OWN sample rate: cFramer's sizes are
 * seconds (Androids.conf:73-78) and SMILExtract analyses the file as it is.  Layout: all clips of a
 * batch (one sample rate per call) are concatenated in `wav` (float32 in [-1,1), mono); clip c occupies
 * samples [clip_off[c], clip_off[c+1]).  rsaf_smile_geometry gives frame = round(0.025 fs), hop =
 * round(0.010 fs) (floor(x + 0.5)) and the FFT length (next power of two: 256 / 512 / 1024 / 2048).
 * Frames: n_frames(n) = n < frame ? 0 : (n-frame)/hop + 1, frame_off is their exclusive prefix sum.
 * LLDs are written contour-major: lld[i * total_frames + frame_off[c] + t], i in [0, RSAF_SMILE_NLLD).
 * The whole chain computes, stores and hands over FLOAT64 (ABI 5): its decisions (peak enhancement, candidate ranking,
 * Viterbi path, jitter lags, roll-off crossings, maxPos / minPos) then coincide with the float64 CPU restatement. */
#define RSAF_SMILE_FRAME 400   /* at 16 kHz */
#define RSAF_SMILE_HOP 160     /* at 16 kHz */
#define RSAF_SMILE_NLLD 38
#define RSAF_SMILE_NFEAT 912
#define RSAF_SMILE_NCAND 6
int rsaf_smile_geometry(int sample_rate, int* frame_host, int* hop_host, int* nfft_host);
int64_t rsaf_smile_n_frames(int64_t n_samples, int sample_rate);
/* Androids.conf:73-186,258-280: framer, pre-emphasis, Hamming, FFT magnitude, mel/MFCC, RMS energy, ZCR,
 * intensity/loudness, 16 spectral descriptors (32 LLD rows), and cSpecScale + cPitchShs: per frame the
 * NCAND best sub-harmonic-summation candidates as (f0 Hz, voicing) double pairs, best score first, zeros in
 * empty slots -> cand[frame][NCAND][2] (caller-owned, 96 bytes per frame).  The six remaining LLD rows
 * (F0final, voicingFinalUnclipped, jitterLocal, jitterDDP, shimmerLocal, logHNR) are filled by
 * rsaf_smile_pitch_track.  octave_spectrum (may be NULL): the cSpecScale output ('hps' level of the config),
 * [total_frames][nfft/2 + 1] float64. */
int rsaf_smile_lld_batch(const float* wav, const int64_t* clip_off, const int64_t* frame_off,
                         int n_clips, int64_t max_clip_frames, int64_t total_frames, int sample_rate,
                         double* lld, double* cand, double* octave_spectrum, rsaf_stream_t stream);
/* Androids.conf:190-255: cPitchSmootherViterbi (fixed lag 30 frames) over the candidates, cValbasedSelector
 * (pitch zeroed where pcm_RMSenergy < 0.001: reads LLD row 0), cPitchJitter (waveform-matched periods on `wav`
 * driven by F0final) -> LLD rows 14, 15, 18..21.  back_workspace: 8 bytes per frame.
 * rsaf_smile_workspace_bytes(total_frames) covers cand + back_workspace when carved from one buffer. */
int64_t rsaf_smile_workspace_bytes(int64_t total_frames);
int rsaf_smile_pitch_track(const float* wav, const int64_t* clip_off, const int64_t* frame_off, int n_clips,
                           int64_t total_frames, int sample_rate, const double* cand, void* back_workspace,
                           double* lld, rsaf_stream_t stream);
/* Androids.conf:284-368 (sma3, delta regression W=2, 12 functionals).  window_frames = 0: statistics over the
 * whole clip; > 0: over the first window_frames frames of the full-length contours (the literal reading of
 * frameSize=0.025 / frameStep=0 at :355-356 keeps row 0 of a 3-frame-window output; see oracle/smile_oracle.py).
 * out: [n_clips, RSAF_SMILE_NFEAT] float64 in cCsvSink column order. */
int rsaf_smile_functionals(const double* lld, const int64_t* frame_off, int n_clips,
                           int64_t total_frames, int window_frames, double* out, rsaf_stream_t stream);

/* ---- exact-fp32 MFMA GEMM building block ---------------------------------------------------------
 * C[z][m][n] = act(alpha * sum_k A[z][m][k] * B[z](k,n) + bias[n] + R[z][m][n]).
 * Replaces the stock PyTorch ops the reference dispatches for every dense contraction of the path:
 * nn.Linear / nn.Conv1d inside transformers' Wav2Vec2Model (src/foundation_model_extractor.py:115)
 * and nn.Conv1d / the LSTM input projections of CNNLSTM (src/models.py:49-62,145-152).
 * B is [N,K] (b_kn = 0, K contiguous) or [K,N] (b_kn = 1).  z = z1*nz2 + z2 with the element strides
 * strides8_host = {sA1,sA2,sB1,sB2,sC1,sC2,sR1,sR2} (host array, may be NULL = all zero).
 * a_pad_k > 0: k=3/pad=1 convolution over a channels-last sequence read in place (A points one
 * row before the sequence, lda = Cin, K = 3*Cin, a_pad_k = Cin).  act: 0 none, 1 GELU(erf), 2 SiLU.
 * Requirements: A, B 16-byte aligned; lda, ldb, A/B strides multiples of 4; K % 4 == 0 (b_kn = 0)
 * or N % 4 == 0 (b_kn = 1); nz <= 65535.  Only the logical operand elements reach a result: the padding
 * between K and lda (ldb) and past N in a row of B, R or C may hold anything, NaN included, and is not written. */
int rsaf_gemm_f32(const float* A, const float* B, float* C, const float* bias, const float* R,
                  int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr,
                  int nz, int nz2, const int64_t* strides8_host, int a_pad_k, int act, float alpha,
                  int b_kn, rsaf_stream_t stream);

/* ---- fp32-accurate GEMM on the fp16 matrix pipe: two-way operand splits, three products --------------------------
 * The same contraction and call sites as above (nn.Linear / nn.Conv1d inside Wav2Vec2Model,
 * src/foundation_model_extractor.py:115), from three v_mfma_f32_32x32x16_f16 products per term (csrc/gemm_f16x3.hip):
 * every operand row is multiplied by a power of two `scale[r]` that puts its largest magnitude into [2^14, 2^15) and
 * split into two fp16 planes, x * scale = hi + lo (11 + 11 significand bits); a b = (a_h b_h + a_h b_l + a_l b_h) /
 * (s_a s_b), fp32 accumulation.  Error against float64: at or below that of an fp32 FMA chain.
 *   rsaf_f16x2_row_scales: scale[r] from the exact maximum of row r of src[rows][K] (row stride ld); norm2 (may be NULL)
 *     receives the rows' Euclidean norms (the Cauchy-Schwarz bound a producer needs for a GEMM OUTPUT's scale).
 *   rsaf_split_f16x2: src * scale[r * scale_stride] -> planes (fp16 bit patterns, plane_stride elements apart), row-major
 *     [rows][K] or (panels != 0) k16 panels: element (r, k) at (k / 16) * (rows * 16) + r * 16 + k % 16.
 *   rsaf_gemm_f16x3: C (fp32, row stride ldc) and / or C_planes (the next GEMM's A, scaled by c_scale[m * c_scale_stride],
 *     which must keep |x| * c_scale below 65504), either may be NULL; a_scale[m * a_scale_stride], b_scale[n]: the scales
 *     the planes were built with; amax_out (may be NULL): atomicMax of the bit pattern of max |x| over everything
 *     written (zero it first).  Supported, ten combinations: {act 0, C} {act 0, C, R} {act 0, C_planes}
 *     {act 0, C, C_planes} {act 1, C} {act 2, C} {act 1, C, R} {act 2, C, R} {act 1, C_planes} {act 2, C_planes}; anything
 *     else (a residual without C, an activation with both outputs, no output) is an argument error.
 *     K % 16 == 0, N % 16 == 0.                                                                                    */
int rsaf_f16x2_row_scales(const float* src, int64_t rows, int K, int64_t ld, float* scale, float* norm2,
                          rsaf_stream_t stream);
int rsaf_split_f16x2(const float* src, int64_t rows, int K, int64_t ld, const float* scale, int scale_stride,
                     uint16_t* planes, int64_t plane_stride, int panels, rsaf_stream_t stream);
int rsaf_gemm_f16x3(const uint16_t* A_planes, int64_t a_plane_stride, const float* a_scale, int a_scale_stride,
                    const uint16_t* B_planes, int64_t b_plane_stride, const float* b_scale, float* C,
                    uint16_t* C_planes, int64_t c_plane_stride, const float* c_scale, int c_scale_stride,
                    uint32_t* amax_out, const float* bias, const float* R, int M, int N, int K, int64_t lda, int64_t ldb,
                    int64_t ldc, int64_t ldr, int act, float alpha, int a_panels, int b_panels, int c_panels,
                    rsaf_stream_t stream);

/* ---- CNN-LSTM-with-attention classifier forward ----------------------------------------------------
 * Replaces CNNLSTM.forward (src/models.py:161-193) in eval mode: x[B,T,input_dim] float32 ->
 * logits[B,num_classes].  Zero-padded frames are processed like any other frame (the reference's
 * collate_fn pads without a mask, src/dl_cv_strategies.py:81-84).
 * `weights`: one float32 device blob with eval-mode BatchNorm folded into the convolutions,
 * conv kernels stored tap-major ([Cout][tap*Cin + ci]), LSTM biases summed (b_ih + b_hh) and both
 * directions concatenated ([fwd 4H | reverse 4H] rows, gate order i,f,g,o).  Segment offsets (in
 * floats, 16-byte aligned) come from rsaf_cnnlstm_weight_offsets in this order:
 *   w1 b1 wsc bsc w2 b2 w3 b3 w4 b4  {wih_l bih_l whh_l} x lstm_layers  watt batt wfc bfc
 * (wsc/bsc = -1 when input_dim == channels: identity shortcut).
 * act: 1 = gelu, 2 = silu.  hidden must be 64 or 128, T >= 2, B <= 65535.                       */
int64_t rsaf_cnnlstm_weight_floats(int input_dim, int channels, int hidden, int num_classes, int lstm_layers);
int rsaf_cnnlstm_weight_offsets(int input_dim, int channels, int hidden, int num_classes, int lstm_layers,
                                int64_t* offsets_host, int cap, int* n_host);
int64_t rsaf_cnnlstm_workspace_bytes(int B, int T, int input_dim, int channels, int hidden, int lstm_layers);
int rsaf_cnnlstm_forward(const float* x, int B, int T, int input_dim, int channels, int hidden,
                         int num_classes, int lstm_layers, int act, const float* weights,
                         void* workspace, int64_t workspace_bytes, float* logits, rsaf_stream_t stream);
/* The same forward with the intermediate tensors the reference's sub-modules return copied out (any pointer may
 * be NULL): res1_out [B][T][C] = res_block1 output (src/models.py:175, channels-last), res2_out [B][T/2][C] =
 * res_block2 output (:178), lstm_out [B][T/2][2H] = nn.LSTM output (:184), pooled_out [B][2H] =
 * AttentionPooling output (:187). */
int rsaf_cnnlstm_forward_stages(const float* x, int B, int T, int input_dim, int channels, int hidden,
                                int num_classes, int lstm_layers, int act, const float* weights, void* workspace,
                                int64_t workspace_bytes, float* logits, float* res1_out, float* res2_out,
                                float* lstm_out, float* pooled_out, rsaf_stream_t stream);
/* ResidualBlock.forward (src/models.py:64-76) in eval mode on a channels-last sequence: x [B][T][Cin] ->
 * y [B][T][Cout] = act(BN2(conv2(act(BN1(conv1(x))))) + shortcut(x)), k = 3 / pad 1 / stride 1.  BatchNorm folded
 * into tap-major weights ([Cout][tap*Cin + ci]) as in the blob of rsaf_cnnlstm_forward; wsc/bsc = folded
 * conv1x1+BN shortcut, both NULL for the identity shortcut (Cin == Cout). */
int64_t rsaf_cnn_resblock_workspace_bytes(int B, int T, int out_channels);
int rsaf_cnn_resblock_forward(const float* x, int B, int T, int in_channels, int out_channels, int act,
                              const float* w1, const float* b1, const float* wsc, const float* bsc,
                              const float* w2, const float* b2, void* workspace, int64_t workspace_bytes,
                              float* y, rsaf_stream_t stream);
/* AttentionPooling.forward (src/models.py:94-107): seq [B][T][features] -> pooled [B][features] =
 * sum_t softmax_t(seq . watt + batt) * seq; features = 128 or 256. */
int rsaf_attnpool_forward(const float* seq, int B, int T, int features, const float* watt, const float* batt,
                          float* pooled, rsaf_stream_t stream);

/* ---- CNN-LSTM training step: forward in training mode + backward -------------------------------------
 * Replaces `out = model(seq)` under model.train() and the model part of `loss.backward()` in the reference's
 * training loops (src/dl_cv_strategies.py:118-125,241-243; module: src/models.py:64-76,161-193): BatchNorm1d on
 * batch statistics (biased variance over B*T rows; zero-padded frames count), dropout by caller-supplied masks
 * (float32 0 or 1/(1-p), NULL = no dropout): mask_block1 [B][T][C], mask_block2 [B][T/2][C],
 * mask_lstm_host = HOST array of lstm_layers-1 DEVICE pointers [B][T/2][2H] (or NULL), mask_fc [B][2H].
 * `params` / `grads`: float32 device blobs, segment offsets (floats) from rsaf_cnnlstm_train_param_offsets in
 * this order (conv kernels tap-major [Cout][tap][Cin]; g/be = BatchNorm weight/bias; b_l = b_ih + b_hh, both
 * directions stacked [fwd 4H | reverse 4H], gate order i,f,g,o):
 *   w1 b1 g1 be1  wsc bsc gsc besc  w2 b2 g2 be2  w3 b3 g3 be3  w4 b4 g4 be4  {wih_l b_l whh_l} x layers
 *   watt batt wfc bfc                                  (the four shortcut entries are -1 when input_dim == channels)
 * The gradient of b_l is the gradient of both b_ih and b_hh.
 * `saved` (rsaf_cnnlstm_train_saved_floats) carries the activations from forward to backward; `scratch`
 * (rsaf_cnnlstm_train_scratch_floats) may be reused between calls.  bn_stats_out (optional, device): [5][3][C]
 * mean / biased variance / rstd of bn1, shortcut BN, bn2 of block 1 and bn1, bn2 of block 2, for the caller's
 * running-statistics update.  backward consumes `saved` (the gates are overwritten): one backward per forward. */
int64_t rsaf_cnnlstm_train_param_floats(int input_dim, int channels, int hidden, int num_classes, int lstm_layers);
int rsaf_cnnlstm_train_param_offsets(int input_dim, int channels, int hidden, int num_classes, int lstm_layers,
                                     int64_t* offsets_host, int cap, int* n_host);
int64_t rsaf_cnnlstm_train_saved_floats(int B, int T, int input_dim, int channels, int hidden, int lstm_layers);
int64_t rsaf_cnnlstm_train_scratch_floats(int B, int T, int input_dim, int channels, int hidden, int lstm_layers);
int rsaf_cnnlstm_train_forward(const float* x, int B, int T, int input_dim, int channels, int hidden,
                               int num_classes, int lstm_layers, int act, const float* params,
                               const float* mask_block1, const float* mask_block2,
                               const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                               int64_t saved_floats, float* scratch, int64_t scratch_floats, float* logits,
                               float* bn_stats_out, rsaf_stream_t stream);
int rsaf_cnnlstm_train_backward(const float* x, int B, int T, int input_dim, int channels, int hidden,
                                int num_classes, int lstm_layers, int act, const float* params,
                                const float* mask_block1, const float* mask_block2,
                                const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                                int64_t saved_floats, float* scratch, int64_t scratch_floats,
                                const float* dlogits, float* grads, rsaf_stream_t stream);

/* ---- Group training step: K independent replicas of one architecture in one call -----------------------
 * The reference trains models of identical architecture and hyper-parameters on different data one after another
 * (the inner folds of an Optuna trial, src/dl_cv_strategies.py:224-251; the folds of :399-422).  A group call runs
 * the step above for K such replicas (own weights, own batch of own shape B x T, own masks) on one stream, with the
 * LSTM recurrences of all replicas in ONE launch per layer and pass; everything else runs per replica.  The results
 * are those of K single calls, bit for bit.  Every field of an item means what the argument of the same name means
 * above; sizes per item from rsaf_cnnlstm_train_saved_floats / _scratch_floats / _param_floats.  Each replica needs
 * its own `scratch` (stages of different replicas interleave).  forward reads x .. bn_stats_out, backward x ..
 * scratch_floats, dlogits and grads.  All checks of the single entries apply per item, plus 1 <= K <=
 * RSAF_CNNLSTM_GROUP_MAX and no two items overlapping in saved, scratch, logits (forward) or grads (backward); they
 * all run before the first launch, and rsaf_last_error() names the item.  A group in which a batch exceeds the
 * 4-row recurrence threshold (RSAF_LSTM_SMALL_MAX, default 1 024) runs that recurrence per replica. */
#define RSAF_CNNLSTM_GROUP_MAX 16
typedef struct {
    const float* x;
    int B, T;
    const float* params;
    const float* mask_block1;
    const float* mask_block2;
    const float* const* mask_lstm_host;
    const float* mask_fc;
    float* saved;
    int64_t saved_floats;
    float* scratch;
    int64_t scratch_floats;
    float* logits;                 /* forward */
    float* bn_stats_out;           /* forward, optional */
    const float* dlogits;          /* backward */
    float* grads;                  /* backward */
} rsaf_cnnlstm_train_item;
int rsaf_cnnlstm_train_group_max(void);
int rsaf_cnnlstm_train_forward_group(const rsaf_cnnlstm_train_item* items_host, int K, int input_dim, int channels,
                                     int hidden, int num_classes, int lstm_layers, int act, rsaf_stream_t stream);
int rsaf_cnnlstm_train_backward_group(const rsaf_cnnlstm_train_item* items_host, int K, int input_dim, int channels,
                                      int hidden, int num_classes, int lstm_layers, int act, rsaf_stream_t stream);

/* ---- Rest of the training step: cross-entropy, Adam and BatchNorm running statistics, one launch per group ------
 * What the reference's loop does around the model (src/dl_cv_strategies.py:122-125,236-248): nn.CrossEntropyLoss()
 * with its defaults on the logits, torch.optim.Adam(model.parameters()).step(), and nn.BatchNorm1d's update of its
 * running statistics.  Each entry takes K <= RSAF_CNNLSTM_GROUP_MAX items (host array) and issues ONE launch.
 *
 * rsaf_ce_loss_group: loss_out[0] = mean over the B rows of (logsumexp(logits[b]) - logits[b][labels[b]]), computed
 * with the row maximum subtracted; dlogits_out [B][nc] = (softmax - onehot) / B, or NULL (validation passes: the
 * loss alone, same bits).  Any num_classes >= 2.  A label outside [0, num_classes) makes the item's loss NaN and is
 * never used as an index. */
typedef struct {
    const float* logits;           /* [B][num_classes] */
    const int64_t* labels;         /* [B] */
    int B;
    float* loss_out;               /* one float */
    float* dlogits_out;            /* [B][num_classes] or NULL */
} rsaf_ce_loss_item;
int rsaf_ce_loss_group(const rsaf_ce_loss_item* items_host, int K, int num_classes, rsaf_stream_t stream);

/* rsaf_cnnlstm_adam_group: the published Adam update (bias-corrected moments, eps outside the square root, no weight
 * decay, no amsgrad) of K replicas of one architecture, on the parameters in their natural torch layouts.
 * The parameters of a replica are numbered in blob order, rsaf_cnnlstm_adam_param_count() of them:
 *   per convolution (five, or four when input_dim == channels): weight [Cout][Cin][k], bias, BN weight, BN bias;
 *   per LSTM layer: weight_ih, weight_ih_reverse, bias_ih, bias_hh, bias_ih_reverse, bias_hh_reverse, weight_hh,
 *   weight_hh_reverse;  then attention weight, attention bias, fc weight, fc bias.
 * `table`: DEVICE array of device pointers, [3][P] = parameter, exp_avg, exp_avg_sq of every parameter (float32,
 * contiguous; entries of skipped parameters are not read), or [4][P] with the gradients in the parameters' layouts
 * as fourth row when `grads` is NULL.  Otherwise `grads` is a gradient blob as rsaf_cnnlstm_train_backward_group
 * wrote it: the conv kernels are read tap-major, and b_ih and b_hh of a direction both receive the gradient of
 * their sum.  Bit i of `skip` leaves parameter i and its moments as they are (requires_grad = False, or no gradient).
 * lr, betas, eps and the 1-based `step` of the bias corrections are per item.  Items must not share parameters or
 * moments.
 *
 * rsaf_cnnlstm_pack_params_group: params = the blob of rsaf_cnnlstm_train_forward, written from the parameters where
 * they live (row 0 of `table`): conv kernels tap-major, b_ih + b_hh summed.  The padding floats between segments are
 * not written.  One launch at the head of a step replaces the host-side packing, and since the blob is rebuilt from
 * the parameters every step, no edit of them (load_state_dict, an in-place change, also one through `.data` that no
 * version counter sees) can leave it stale. */
typedef struct {
    const float* grads;            /* gradient blob, or NULL: gradients from the table's fourth row */
    const void* const* table;      /* device array [3][P] or [4][P] of device pointers */
    uint64_t skip;
    double lr, beta1, beta2, eps;
    int64_t step;
} rsaf_cnnlstm_adam_item;
typedef struct {
    const void* const* table;      /* device array [>= 1][P] of device pointers: row 0 = the parameters */
    float* params;                 /* parameter blob, written */
} rsaf_cnnlstm_pack_item;
int rsaf_cnnlstm_pack_params_group(const rsaf_cnnlstm_pack_item* items_host, int K, int input_dim, int channels,
                                   int hidden, int num_classes, int lstm_layers, rsaf_stream_t stream);
int rsaf_cnnlstm_adam_param_count(int input_dim, int channels, int hidden, int num_classes, int lstm_layers);
int rsaf_cnnlstm_adam_group(const rsaf_cnnlstm_adam_item* items_host, int K, int input_dim, int channels, int hidden,
                            int num_classes, int lstm_layers, rsaf_stream_t stream);

/* ---- Class weights and gradient-norm clipping in the fused step --------------------------------------------------
 * nn.CrossEntropyLoss(weight = w) and clip_grad_norm_(model.parameters(), max_norm) between backward and step, on data
 * the step already holds on the device.  New entries beside the ones above, which keep their code and their bits.
 * Checks of all three, before any launch, rsaf_last_error() naming the item: 1 <= K <= RSAF_CNNLSTM_GROUP_MAX, the
 * pointers that are not marked optional, and no two ranges that the items of the call write overlapping.
 *
 * rsaf_ce_loss_weighted_group: rsaf_ce_loss_group with per-item class weights (reduction "mean"):
 *   loss_out[0]    = sum_b w[y_b] nll_b / sum_b w[y_b],  nll_b = logsumexp(logits[b]) - logits[b][y_b] (row maximum subtracted)
 *   dlogits_out[b] = w[y_b] (softmax(logits[b]) - onehot(y_b)) / sum_b w[y_b]
 * One launch, one workgroup per item, rows in double by one lane each, both sums by the fixed tree of
 * rsaf_ce_loss_group.  A class of weight 0 is allowed; sum_b w[y_b] = 0 gives a NaN loss, as torch does.  A label
 * outside [0, num_classes) makes the item's loss (and that row of dlogits_out) NaN and indexes neither the row nor w.
 * An item with class_weight == NULL returns the bits of rsaf_ce_loss_group.  num_classes >= 2. */
typedef struct {
    const float* logits;           /* [B][num_classes] */
    const int64_t* labels;         /* [B] */
    int B;
    float* loss_out;               /* one float */
    float* dlogits_out;            /* [B][num_classes] or NULL */
    const float* class_weight;     /* [num_classes] device floats, or NULL: the unweighted mean */
} rsaf_ce_loss_weighted_item;
int rsaf_ce_loss_weighted_group(const rsaf_ce_loss_weighted_item* items_host, int K, int num_classes, rsaf_stream_t stream);

/* rsaf_cnnlstm_grad_norm_group: norm_out[0] = sqrt(sum_p ||g_p||^2) over the PARAMETERS of the numbering above whose
 * bit in `skip` is clear, and scale_out[0] = min(1, max_norm / (norm + 1e-6)): what clip_grad_norm_ (2-norm) multiplies
 * the gradients by.  The gradients come from `grads` / `table` exactly as in rsaf_cnnlstm_adam_item.  With a gradient
 * blob, b_ih and b_hh of a direction both receive the gradient of the one segment of their sum, so that segment counts
 * twice with both live, once with one of them skipped and not at all with both skipped; the padding floats between
 * segments are never read, and the tap-major image of a conv kernel is a permutation.  The sum runs over the segments
 * and workgroups of rsaf_cnnlstm_adam_group: each workgroup sums the squares of its <= 1024 floats in double through a
 * fixed tree into one of the item's `partials`, a second launch adds the partials in a fixed order, and norm and scale
 * are rounded to float once.  No floating-point atomics: the results do not depend on K, on the item's position or on
 * scheduling.  max_norm > 0 and not NaN; +inf gives scale 1 with the norm still reported, and a zero gradient gives
 * scale 1.  `partials`: 8-byte aligned, at least rsaf_cnnlstm_grad_norm_partials() doubles (-1: unsupported
 * dimensions), scratch.  Two launches per call.
 *
 * rsaf_cnnlstm_adam_scaled_group: rsaf_cnnlstm_adam_group on g * grad_scale[0] (the product rounded once in double);
 * grad_scale is read on the device, so nothing waits for the norm.  NULL means 1, and a scale of exactly 1.0f leaves
 * the update of rsaf_cnnlstm_adam_group bit for bit.  One launch. */
typedef struct {
    const float* grads;            /* gradient blob, or NULL: gradients from the table's fourth row */
    const void* const* table;      /* device array [4][P] of device pointers (read only when grads is NULL) */
    uint64_t skip;
    double max_norm;
    double* partials;              /* scratch, partials_count doubles */
    int64_t partials_count;
    float* norm_out;               /* one float */
    float* scale_out;              /* one float */
} rsaf_cnnlstm_grad_norm_item;
typedef struct {
    const float* grads;
    const void* const* table;
    uint64_t skip;
    double lr, beta1, beta2, eps;
    int64_t step;
    const float* grad_scale;       /* one device float, or NULL: 1 */
} rsaf_cnnlstm_adam_scaled_item;
int64_t rsaf_cnnlstm_grad_norm_partials(int input_dim, int channels, int hidden, int num_classes, int lstm_layers);
int rsaf_cnnlstm_grad_norm_group(const rsaf_cnnlstm_grad_norm_item* items_host, int K, int input_dim, int channels,
                                 int hidden, int num_classes, int lstm_layers, rsaf_stream_t stream);
int rsaf_cnnlstm_adam_scaled_group(const rsaf_cnnlstm_adam_scaled_item* items_host, int K, int input_dim, int channels,
                                   int hidden, int num_classes, int lstm_layers, rsaf_stream_t stream);

/* rsaf_bn_running_stats_group: running = (1 - momentum) * running + momentum * batch value for the five BatchNorm
 * layers of a replica, from the [5][3][C] statistics of the step (bn_stats_out above); the batch variance is scaled
 * by `unbias[i]` = n / (n - 1), n the rows that layer saw.  A layer whose running_mean is NULL is left out (no
 * shortcut BatchNorm when input_dim == channels; track_running_stats = False). */
typedef struct {
    const float* stats;            /* [5][3][C] */
    float* running_mean[5];
    float* running_var[5];
    double momentum[5];
    double unbias[5];
} rsaf_bn_running_item;
int rsaf_bn_running_stats_group(const rsaf_bn_running_item* items_host, int K, int channels, rsaf_stream_t stream);

/* ---- Dropout masks of a group training step from a counter-based generator, one launch per group ----------------
 * Every mask element is a pure function of (seed, step, slot, element index): no generator state lives on the device,
 * a mask does not depend on what else drew random numbers, and K replicas drawn in one call, one by one or in any order
 * receive the same masks.  The masks are what rsaf_cnnlstm_train_forward reads: float32, 0 or 1 / (1 - p).
 *
 * The generator is the published Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key
 * schedule constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds.  The mapping, which any host
 * can restate:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (j, slot, step & 0xffffffff, step >> 32),  j = e >> 2 the block of flat element index e
 *   element e takes output word e & 3 of its block
 *   thr     = (uint32) floor(p * 2^32), computed in double; the element is kept iff word >= thr
 *   a kept element holds 1.0f / (float)(1.0 - p) (the subtraction in double, then the cast, then a float division),
 *   every other element 0.0f; a slot with p >= 1 is all zeros.
 * Slots (the element index is the flat index of the layout):
 *   0 = res_block1 [B][T][C], 1 = res_block2 [B][T/2][C], 2 = fc [B][2H],
 *   3 + l = LSTM inter-layer mask l [B][T/2][2H], l <= 2 (lstm_layers <= 4).
 *
 * rsaf_dropout_masks_group writes all drawn slots of K <= RSAF_CNNLSTM_GROUP_MAX items in ONE launch.  A slot with
 * p <= 0 is not drawn: its pointer must be NULL (the training entries take NULL for "no mask").  No float at or beyond
 * mask + n is written.  Checked before the launch, rsaf_last_error() naming item and slot: K in range; 0 <= n <= 2^32;
 * p not NaN; a non-NULL slot has n >= 1, p > 0 and a 16-byte aligned pointer; no two drawn ranges of the call overlap.
 * A call in which nothing is drawn returns RSAF_OK without a launch. */
#define RSAF_DROPOUT_SLOTS 6
typedef struct {
    uint64_t seed, step;
    float* mask[RSAF_DROPOUT_SLOTS];    /* NULL = slot not drawn */
    int64_t n[RSAF_DROPOUT_SLOTS];      /* elements */
    double p[RSAF_DROPOUT_SLOTS];
} rsaf_dropout_item;
int rsaf_dropout_masks_group(const rsaf_dropout_item* items_host, int K, rsaf_stream_t stream);

/* ---- Group inference forward: K independent eval-mode forwards of one architecture in one call -----------------
 * The other half of the reference's loops: the validation pass of every epoch (src/dl_cv_strategies.py:131-139) and
 * _eval_model (:183-194).  No weight changes between the batches of such a pass, so every batch of every model is an
 * independent forward.  A group call runs rsaf_cnnlstm_forward for K of them (own batch of own shape B x T, own
 * workspace, own logits) on one stream, with the LSTM recurrences of all items in ONE launch per layer and the
 * attention pooling + classifier of all items in ONE launch; everything else runs per item.  The logits are those of
 * K single calls, bit for bit.  Every field means what the argument of the same name means in rsaf_cnnlstm_forward;
 * workspace size per item from rsaf_cnnlstm_workspace_bytes.  Items may share `weights` (several batches of one
 * model): the fp16 plane pairs of the weights are then prepared once, in the workspace of the first item that carries
 * the blob, and the later items read them there.  All checks of the single entry apply per item (with B >= 1), plus
 * 1 <= K <= RSAF_CNNLSTM_GROUP_MAX and no two items overlapping in workspace or logits; they all run before the first
 * launch, and rsaf_last_error() names the item.  An item whose batch exceeds the 4-row recurrence threshold
 * (RSAF_LSTM_SMALL_MAX, default 1 024) has its recurrences launched on its own. */
typedef struct {
    const float* x;
    int B, T;
    const float* weights;
    void* workspace;
    int64_t workspace_bytes;
    float* logits;
} rsaf_cnnlstm_forward_item;
int rsaf_cnnlstm_forward_group(const rsaf_cnnlstm_forward_item* items_host, int K, int input_dim, int channels,
                               int hidden, int num_classes, int lstm_layers, int act, rsaf_stream_t stream);

/* ---- Mixed groups: K replicas of different architecture in one call ---------------------------------------------
 * The reference's hyper-parameter search (src/dl_cv_strategies.py:216-251) trains three inner folds per trial, and
 * cnn_out_channels, lstm_hidden_dim and the activation change from trial to trial: a group of one architecture holds
 * three replicas.  A mixed group holds K <= RSAF_CNNLSTM_GROUP_MAX replicas that share input_dim, num_classes and
 * lstm_layers; item k has channels, hidden (64 or 128) and act of arch_host[k] (several trials in flight side by side).
 * The three entries below do what rsaf_cnnlstm_train_forward_group, _backward_group and rsaf_cnnlstm_forward_group do,
 * item k with its own architecture: ONE launch per LSTM layer and pass still carries the recurrences of all items,
 * whatever their hidden size, and ONE launch the heads of all items of the inference forward.  Per item the arithmetic
 * is that of the single entries, so every result equals, bit for bit, what the same items give through the single
 * entries or through one group call per architecture; with all arch_host[k] equal it is what the group entry gives.
 *
 * The recurrence launches use 512-thread workgroups.  A hidden = 128 item runs as in the group entries (one workgroup
 * per 4-row tile and direction).  The workgroup of a hidden = 64 item runs BOTH directions of its tile, waves 0-3 the
 * forward and waves 4-7 the reverse direction, each half with LDS buffers of its own; both halves loop over the same
 * T, so they take the same barriers, and the second-direction workgroups of such an item leave whole.  The rule the
 * kernels keep: all eight waves of a workgroup either leave before the first LDS access or barrier, or take every
 * barrier of the loop; no workgroup has some waves returned while others wait at a barrier.
 *
 * Checks, all before the first launch, rsaf_last_error() naming the item: 1 <= K <= RSAF_CNNLSTM_GROUP_MAX; items_host
 * and arch_host non-NULL; the dims of every item as in the single entries; every per-item check of the group entries
 * with the item's own architecture (sizes from rsaf_cnnlstm_train_saved_floats / _scratch_floats / _param_floats /
 * rsaf_cnnlstm_workspace_bytes for that architecture), where a buffer smaller than the item's architecture needs
 * (typically one sized for another item's) is RSAF_ERR_ARG; no two items overlapping as in the group entries.  In the
 * inference entry, items that share `weights` must share an architecture (RSAF_ERR_ARG otherwise); the fp16 plane
 * pairs are prepared once per distinct blob as in rsaf_cnnlstm_forward_group.  An item whose batch exceeds the 4-row
 * recurrence threshold (RSAF_LSTM_SMALL_MAX) has its recurrences launched on its own; the others stay grouped.
 *
 * Around the model: rsaf_ce_loss_group and rsaf_dropout_masks_group know no architecture and take the whole mixed
 * group in one launch.  rsaf_cnnlstm_pack_params_group, rsaf_cnnlstm_adam_group and rsaf_bn_running_stats_group carry
 * the segment table of ONE architecture in their kernel arguments (six tables do not fit), so a mixed group calls each
 * of them once per distinct architecture: a few element-wise launches in place of one. */
typedef struct {
    int channels, hidden, act;
} rsaf_cnnlstm_arch;
int rsaf_cnnlstm_train_forward_group_mixed(const rsaf_cnnlstm_train_item* items_host, const rsaf_cnnlstm_arch* arch_host,
                                           int K, int input_dim, int num_classes, int lstm_layers,
                                           rsaf_stream_t stream);
int rsaf_cnnlstm_train_backward_group_mixed(const rsaf_cnnlstm_train_item* items_host,
                                            const rsaf_cnnlstm_arch* arch_host, int K, int input_dim, int num_classes,
                                            int lstm_layers, rsaf_stream_t stream);
int rsaf_cnnlstm_forward_group_mixed(const rsaf_cnnlstm_forward_item* items_host, const rsaf_cnnlstm_arch* arch_host,
                                     int K, int input_dim, int num_classes, int lstm_layers, rsaf_stream_t stream);

/* ---- Input gradient of the training step ----------------------------------------------------------------------
 * What `loss.backward()` leaves in `x.grad` when a trainable module sits in front of the classifier (a mix of encoder
 * layers, a projection, a perturbation of the embeddings).  The entries below are rsaf_cnnlstm_train_backward,
 * _backward_group and _backward_group_mixed with three more operands; the plain entries keep their code and their bits.
 *   dx [B][T][input_dim] float32, written (not accumulated) in every row: zero-padded frames and the odd last frame
 *   carry gradient too, since nothing is masked.  With dy_c1 / dy_sc the gradients at the outputs of res_block1.conv1
 *   and of the shortcut convolution (behind their BatchNorm backward) and dz1 the gradient at the block's sum:
 *     dx[b,t,:] = sum_tap dy_c1[b, t-tap+1, :] . W1[:, :, tap] + dy_sc[b,t,:] . Wsc     (input_dim != channels)
 *     dx        = (the convolution term) + dz1                                          (identity shortcut)
 *   dx_scratch: rsaf_cnnlstm_train_dx_scratch_floats(input_dim, channels) floats (host only; -1 for bad dims), the
 *   tap-flipped weights of the data-gradient GEMM.  `scratch` and `saved` keep the sizes of the plain entries.
 * dx == NULL (an item, or the single entry): that replica wants none and runs exactly the launches of the plain entry;
 * dx_scratch is then not read.  With dx, three launches are added per replica (two with the identity shortcut): the 1x1
 * data-gradient GEMM of the shortcut, the flip of W1 and the k = 3 data-gradient GEMM whose epilogue adds the shortcut
 * term.  The parameter gradients are the same bits with and without dx, and the recurrences of a group stay one launch
 * per layer and pass.  Checks on top of those of the plain entries, all before the first launch, rsaf_last_error()
 * naming the item: dx needs dx_scratch (RSAF_ERR_ARG); a short dx_scratch is RSAF_ERR_WORKSPACE; dx and dx_scratch
 * share no float with each other, with x, saved, scratch or grads of their item, or with saved, scratch, grads, dx or
 * dx_scratch of another item (RSAF_ERR_ARG). */
int64_t rsaf_cnnlstm_train_dx_scratch_floats(int input_dim, int channels);
int rsaf_cnnlstm_train_backward_dx(const float* x, int B, int T, int input_dim, int channels, int hidden,
                                   int num_classes, int lstm_layers, int act, const float* params,
                                   const float* mask_block1, const float* mask_block2,
                                   const float* const* mask_lstm_host, const float* mask_fc, float* saved,
                                   int64_t saved_floats, float* scratch, int64_t scratch_floats,
                                   const float* dlogits, float* grads, float* dx, float* dx_scratch,
                                   int64_t dx_scratch_floats, rsaf_stream_t stream);
typedef struct {
    const float* x;
    int B, T;
    const float* params;
    const float* mask_block1;
    const float* mask_block2;
    const float* const* mask_lstm_host;
    const float* mask_fc;
    float* saved;
    int64_t saved_floats;
    float* scratch;
    int64_t scratch_floats;
    float* logits;                 /* not read: the item is a backward item */
    float* bn_stats_out;           /* not read */
    const float* dlogits;
    float* grads;
    float* dx;                     /* [B][T][input_dim], or NULL: no input gradient for this replica */
    float* dx_scratch;             /* rsaf_cnnlstm_train_dx_scratch_floats floats; not read when dx is NULL */
    int64_t dx_scratch_floats;
} rsaf_cnnlstm_train_dx_item;
int rsaf_cnnlstm_train_backward_group_dx(const rsaf_cnnlstm_train_dx_item* items_host, int K, int input_dim, int channels,
                                         int hidden, int num_classes, int lstm_layers, int act, rsaf_stream_t stream);
int rsaf_cnnlstm_train_backward_group_mixed_dx(const rsaf_cnnlstm_train_dx_item* items_host,
                                               const rsaf_cnnlstm_arch* arch_host, int K, int input_dim,
                                               int num_classes, int lstm_layers, rsaf_stream_t stream);

/* ---- Learned mix of encoder layers ---------------------------------------------------------------------------
 * x[b,t,:] = sum_l p[l] h[b,l,t,:] over the L hidden-state layers of a padded batch h [B][L][T][D] (what
 * rsaf_w2v2_forward_ragged_hidden returns per file, stacked), p [L] device floats: the softmax of the learned weights,
 * which with its Jacobian stays with the caller (two tiny ops on [L]).  1 <= L <= RSAF_LAYER_MIX_MAX, D % 4 == 0,
 * B * T * D < 2^40; h, x and dx 16-byte aligned.
 * rsaf_layer_mix_forward: one launch; every workgroup walks its chunks of (b, t, d) once (float4, grid stride) and loops
 * over l, so x is written once and h read once.
 * rsaf_layer_mix_backward: dp_out[l] = sum_{b,t,d} h[b,l,t,d] dx[b,t,d].  The (b, t, d) range is cut into parts whose
 * number depends on the shape alone (csrc/layer_mix_layout.h); a part reads dx once for all L layers, accumulates its L
 * sums in double and writes them to `partials` ([parts][L] doubles, rsaf_layer_mix_partials(B, L, T, D) of them: host
 * only, -1 for bad dims); a second launch adds the parts in ascending order.  No atomics: the same bits on every call.
 * A short `partials` (partials_count, in doubles) is RSAF_ERR_WORKSPACE. */
#define RSAF_LAYER_MIX_MAX 32
int rsaf_layer_mix_forward(const float* h, int B, int L, int T, int D, const float* p, float* x, rsaf_stream_t stream);
int64_t rsaf_layer_mix_partials(int B, int L, int T, int D);
int rsaf_layer_mix_backward(const float* h, const float* dx, int B, int L, int T, int D, double* partials,
                            int64_t partials_count, float* dp_out, rsaf_stream_t stream);

/* ---- Wav2Vec2 frame embeddings for a batch of equal-length chunks -----------------------------------
 * Replaces, per chunk, `processor(chunk).input_values` + `Wav2Vec2Model(...)(input_values)
 * .last_hidden_state` (src/foundation_model_extractor.py:113-116; third-party transformers
 * modeling_wav2vec2.py / feature_extraction_wav2vec2.py:95), fp32 end to end.
 * Chunk i covers samples [chunk_start[i], chunk_start[i] + chunk_len) of `wav` (chunk_start: device
 * int64 array).  out: float32 rows of `hidden` floats; chunk i's T = rsaf_w2v2_frames(chunk_len) frames go
 * to rows out_row_start[i] .. +T (device int64 array; lets the caller lay chunks out in the
 * reference's np.vstack order, src/foundation_model_extractor.py:124) or, when out_row_start is
 * NULL, to rows i*T .. (i+1)*T.
 * `weights`: one float32 device blob; segment offsets (floats, 16-byte aligned) from
 * rsaf_w2v2_weight_offsets in this order:
 *   conv0[C][10] gn_gamma gn_beta conv1..conv6 ([C][tap*C+ci]) fp_ln_g fp_ln_b fp_w[H][C] fp_b
 *   pos_w ([G][C/G][tap*(H/G)+ci], weight norm folded) pos_b enc_ln_g enc_ln_b
 *   per layer: wqkv[3H][H] bqkv wo bo ln1_g ln1_b w1[I][H] b1 w2[H][I] b2 ln2_g ln2_b
 * Feature encoder geometry is wav2vec2's (kernels 10,3,3,3,3,2,2 / strides 5,2,2,2,2,2,2, GroupNorm
 * on layer 0, no conv bias, post-LN encoder).  n_chunks * max(heads, pos_groups) <= 65535.        */
int rsaf_w2v2_frames(int chunk_len);
int64_t rsaf_w2v2_weight_floats(int conv_dim, int hidden, int layers, int heads, int intermediate,
                                int pos_kernel, int pos_groups);
int rsaf_w2v2_weight_offsets(int conv_dim, int hidden, int layers, int heads, int intermediate,
                             int pos_kernel, int pos_groups, int64_t* offsets_host, int cap, int* n_host);
int64_t rsaf_w2v2_workspace_bytes(int n_chunks, int chunk_len, int conv_dim, int hidden, int layers,
                                  int heads, int intermediate, int pos_kernel, int pos_groups);
int rsaf_w2v2_forward(const float* wav, const int64_t* chunk_start, int n_chunks, int chunk_len,
                      int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                      int pos_groups, float layer_norm_eps, const float* weights, void* workspace,
                      int64_t workspace_bytes, float* out, const int64_t* out_row_start,
                      rsaf_stream_t stream);
/* The same forward for windows of DIFFERENT lengths in one call (the reference's loop ends every file in a tail window of
 * its own length, src/foundation_model_extractor.py:103-108): chunk i has chunk_len[i] samples (device int32 array) and
 * T_i = rsaf_w2v2_frames(chunk_len[i]) frames, written to rows out_row_start[i] .. +T_i (or packed, window after window,
 * when out_row_start is NULL).  chunk_len_host: the same lengths on the host (launch geometry); they must be
 * NON-INCREASING.  Every window is normalised, GroupNorm-ed, zero-padded (positional conv) and attended over its own
 * frames only: the values are those of the per-window call.  That holds for window lengths of any mix: where the lengths
 * of a call span frame counts at which the forward changes kernels (256 and 512 frames), the call is run as consecutive
 * sub-calls, one per run of windows that share their kernels, in the same workspace and on the same stream.           */
int64_t rsaf_w2v2_workspace_bytes_ragged(const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers,
                                         int heads, int intermediate, int pos_kernel, int pos_groups);
int rsaf_w2v2_forward_ragged(const float* wav, const int64_t* chunk_start, const int* chunk_len,
                             const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers, int heads,
                             int intermediate, int pos_kernel, int pos_groups, float layer_norm_eps,
                             const float* weights, void* workspace, int64_t workspace_bytes, float* out,
                             const int64_t* out_row_start, rsaf_stream_t stream);
/* Forward variants of the large Wav2Vec2 checkpoints (wav2vec2-large-lv60, -large-robust, XLSR-53, XLS-R 300M): the _ex entry
 * points take `flags`, an OR of the bits below; with flags == 0 they are the entry points above (same weight layout, same
 * workspace, same output bits).  The HF config switch behind each bit:
 *   RSAF_W2V2_LAYER_FEAT_NORM  feat_extract_norm="layer": every conv layer is conv -> LayerNorm over the C channels of each
 *                              frame (eps 1e-5, nn.LayerNorm's default, not layer_norm_eps) -> GELU; no GroupNorm
 *   RSAF_W2V2_CONV_BIAS        conv_bias=True: the 7 feature-encoder convolutions add a bias
 *   RSAF_W2V2_PRE_LN           do_stable_layer_norm=True: h = x + pos_conv(x) without a LayerNorm; per layer
 *                              h += attn(LN1(h)); h += FFN(LN2(h)) (LN1 = layers.l.layer_norm, LN2 = final_layer_norm);
 *                              encoder.layer_norm once after the last layer
 *   RSAF_W2V2_NO_INPUT_NORM    preprocessor do_normalize=False: the windows go into conv0 without zero-mean / unit variance
 * Weight segments appended after the last layer (rsaf_w2v2_weight_offsets_ex lists one offset per C-float row of them):
 *   CONV_BIAS:        cbias[7][C] (conv layer i's bias)
 *   LAYER_FEAT_NORM:  cln[7][2][C] ({gamma, beta} of conv layer i's LayerNorm; layer 0's lives here, the GroupNorm slots
 *                     gn_gamma / gn_beta are unused)
 * Weight floats, offsets and workspace bytes depend on the flags: size every buffer with the _ex calls.
 *
 * The HuBERT and WavLM families are two more variants of the same forward:
 *   RSAF_W2V2_NO_FEAT_PROJ_LN  HubertConfig.feat_proj_layer_norm=False: the feature projection reads the conv output as it is
 *                              (feature_projection.layer_norm does not exist; its two weight slots are unused).  Not with
 *                              RSAF_W2V2_LAYER_FEAT_NORM (RSAF_ERR_ARG): no published geometry pairs them
 *   RSAF_W2V2_REL_POS_BIAS     WavLM's gated relative position bias: scores = q.k / sqrt(hd) + gate[q][head] * tab[head][k - q]
 *                              with gate = a * (b * gru_rel_pos_const[head] - 1) + 2, a = sigmoid(x_in[q, head] . ga + ba),
 *                              b = sigmoid(x_in[q, head] . gb + bb); x_in = the rows the q/k/v projection reads; ga / gb = the
 *                              sums of rows 0..3 / 4..7 of gru_rel_pos_linear.weight, ba / bb those of its bias
 * Their weight segments follow the ones above (REL_POS_BIAS only):
 *   per layer, four offsets:  ga[hd], gb[hd], {ba, bb}, gru_rel_pos_const[heads]
 *   once, one offset:         tab[heads][2 RSAF_W2V2_REL_SPAN - 1], tab[h][d + RSAF_W2V2_REL_SPAN - 1] =
 *                             rel_attn_embed[bucket(d)][h] for |d| < RSAF_W2V2_REL_SPAN; the kernels clamp d to that range,
 *                             which is exact when max_bucket_distance < RSAF_W2V2_REL_SPAN (bucket() is constant beyond it).
 *                             The packer builds it with transformers' sequence of torch operations
 * The gates take rows x heads floats of workspace per call.
 *
 * data2vec-audio is one more variant: Wav2Vec2's forward with another positional embedding.
 *   RSAF_W2V2_POS_CONV_STACK   the positional embedding is a stack of D grouped convolutions instead of one weight-normed
 *                              convolution: p_0 = x (the projected features of one window), and for i = 0..D-1
 *                                  p_{i+1} = GELU( LN( conv1d_i(p_i) ) ),      h = encoder.layer_norm(x + p_D)
 *                              conv1d_i: hidden -> hidden channels in pos_groups groups, pos_kernel taps (1..64, odd or even),
 *                              zero padding pos_kernel / 2 on both sides of the WINDOW and, for an even kernel, the last
 *                              output frame dropped: frame t reads frames t - K/2 .. t - K/2 + K - 1.  With bias, without
 *                              weight norm.  LN: LayerNorm over the hidden channels of a frame WITHOUT weight or bias, eps
 *                              1e-5 whatever layer_norm_eps is (nn.LayerNorm's default).  The depth D (1..15) travels in
 *                              bits 12..15 of flags (D << RSAF_W2V2_POS_DEPTH_SHIFT).  RSAF_ERR_ARG before any launch: the
 *                              flag without depth bits, depth bits without the flag, the flag without
 *                              RSAF_W2V2_LAYER_FEAT_NORM, or with RSAF_W2V2_PRE_LN, RSAF_W2V2_REL_POS_BIAS or
 *                              RSAF_W2V2_NO_FEAT_PROJ_LN
 * Weight blob: layer 0's kernel ([hidden][tap * cg + ci], cg = hidden / pos_groups: the layout of the single convolution)
 * and bias sit in the pos_conv_w / pos_conv_b slots; layers 1..D-1 are appended after every segment above, and
 * rsaf_w2v2_weight_offsets_ex lists them last, {weight, bias} per layer.  The workspace grows by the fp16 planes and row
 * scales of those D - 1 kernels; the stack's rows live in buffers the single convolution uses.                       */
#define RSAF_W2V2_LAYER_FEAT_NORM 1
#define RSAF_W2V2_CONV_BIAS 2
#define RSAF_W2V2_PRE_LN 4
#define RSAF_W2V2_NO_INPUT_NORM 8
#define RSAF_W2V2_NO_FEAT_PROJ_LN 32 /* (bit 16 stays an unknown bit: RSAF_ERR_ARG, as callers of ABI 7 were promised) */
#define RSAF_W2V2_REL_POS_BIAS 64
#define RSAF_W2V2_POS_CONV_STACK 256 /* (bit 128 stays an unknown bit) */
#define RSAF_W2V2_POS_DEPTH_SHIFT 12
#define RSAF_W2V2_POS_DEPTH_MASK 0xF000
#define RSAF_W2V2_REL_SPAN 1024
int64_t rsaf_w2v2_weight_floats_ex(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                   int pos_groups, int flags);
int rsaf_w2v2_weight_offsets_ex(int conv_dim, int hidden, int layers, int heads, int intermediate, int pos_kernel,
                                int pos_groups, int flags, int64_t* offsets_host, int cap, int* n_host);
int64_t rsaf_w2v2_workspace_bytes_ragged_ex(const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers,
                                            int heads, int intermediate, int pos_kernel, int pos_groups, int flags);
int rsaf_w2v2_forward_ragged_ex(const float* wav, const int64_t* chunk_start, const int* chunk_len,
                                const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers, int heads,
                                int intermediate, int pos_kernel, int pos_groups, float layer_norm_eps, int flags,
                                const float* weights, void* workspace, int64_t workspace_bytes, float* out,
                                const int64_t* out_row_start, rsaf_stream_t stream);
/* rsaf_w2v2_forward_ragged_ex that also writes encoder hidden states: transformers'
 * Wav2Vec2Model(..., output_hidden_states=True).hidden_states[k], k = 0..layers (layers + 1 of them, hidden_states[layers] ==
 * `out` bit for bit).  hidden_index_host: n_hidden STRICTLY INCREASING indices in [0, layers] on the host; state
 * hidden_index_host[j] goes to hidden_out + j * hidden_plane_floats, in the row layout of `out` (rows out_row_start[i] .. +T_i,
 * or packed).  hidden_out 16-byte aligned, hidden_plane_floats a multiple of 4 and at least the call's frames x hidden.
 * What each state is (RSAF_W2V2_PRE_LN clear / set):
 *   k = 0            encoder.layer_norm(x + pos_conv(x))      /  x + pos_conv(x), not normalised
 *   0 < k < layers   output of layer k - 1 (final_layer_norm) /  residual stream after layer k - 1, not normalised
 *   k = layers       last_hidden_state (= out)
 * Each state is written by the LayerNorm launch that already reads or writes it: no extra launch, no extra workspace
 * (size it with rsaf_w2v2_workspace_bytes_ragged_ex).  Bad indices return RSAF_ERR_ARG before any launch; n_hidden == 0 is
 * rsaf_w2v2_forward_ragged_ex (same kernels, same bits).                                                               */
int rsaf_w2v2_forward_ragged_hidden(const float* wav, const int64_t* chunk_start, const int* chunk_len,
                                    const int* chunk_len_host, int n_chunks, int conv_dim, int hidden, int layers, int heads,
                                    int intermediate, int pos_kernel, int pos_groups, float layer_norm_eps, int flags,
                                    const float* weights, void* workspace, int64_t workspace_bytes, float* out,
                                    const int64_t* out_row_start, const int* hidden_index_host, int n_hidden,
                                    float* hidden_out, int64_t hidden_plane_floats, rsaf_stream_t stream);

/* ---- Praat-style analyses behind the MSHDS features (float64) ---------------------------------------
 * Replace the parselmouth/Praat calls of src/mshds_extractor.py: To Intensity (:41,198), To Pitch
 * (ac) (:104,143,178,270,355), To Harmonicity (cc) (:36,221), to_spectrogram + spectrum moments
 * (:356-369) and the statistics taken from them (:144-160,179-180,199-202,222,370-373).
 * `clip_info`: device array of n_clips records {int64 sample_off; int64 frame_off; double t1;
 * int32 n_samples; int32 n_frames; double x1; double xmax} (48 bytes) describing, for THIS analysis, where each clip's
 * samples start in `wav`, where its frames start in the per-frame output buffers, the time of its
 * first frame and its frame count (Praat's Sampled_shortTermAnalysis grid, computed by the host), and the
 * sound's own time axis as Praat's Sound object carries it: x1 = time of the first sample (dx / 2 for a sound read
 * from a file), [0, xmax] = its time domain (n dx for a file; after the Sound_resample of
 * src/mshds_extractor.py:418-419 the ORIGINAL duration, with the new grid centred in it).
 * Window tables (`window`, `window_r` = normalised autocorrelation of the window, `twiddle`) are
 * device float64 arrays prepared by the host.  All outputs are float64.                          */
int rsaf_mshds_frameout_doubles(void);   /* doubles per frame record: intensity, ncand, freq[16], strength[16] */
int rsaf_mshds_clip_peak(const float* wav, const void* clip_info, int n_clips, double* gpeak, rsaf_stream_t stream);
/* db_out[frame]; stats_out[clip][2] = {energy-mean dB, max/min of parabolic extrema} */
int rsaf_mshds_intensity(const float* wav, const void* clip_info, int n_clips, int max_frames,
                         const double* window, int half_window, double time_step, int subtract_mean,
                         double* db_out, double* stats_out, rsaf_stream_t stream);
/* params_host[18] = {dt, min_pitch, ceiling, voicing_thr, octave_cost, silence_thr, octave_jump_cost,
 *   voiced_unvoiced_cost, nsamp_window, nsamp_period, min_lag, max_lag, brent_ixmax, max_candidates,
 *   refine_depth, is_cc, dt_window, table_mode (0 | 1 | 2, see sinc_cheb)}.  sel_freq / sel_strength: the path finder's choice per frame.
 * stats_out[clip][8] = {n(f != 0), mean, population sd, mean after |z| <= 2, n voiced, mean Hz,
 *   sd in semitones (n-1), n after filter}.
 * sinc_cheb (may be NULL): [2 * refine_depth][16] Chebyshev coefficients on frac in [0, 1] of the sinc-interpolation
 *   weights of tap offsets -(depth-1) .. depth (mshds.sinc_cheb_table); with it the Brent refinement evaluates a
 *   16-term polynomial per step instead of the 2*depth-term sum whenever no candidate's depth is clipped.  With
 *   params_host[17] = 1 the table is followed by the tables of the clipped depths e = 1 .. refine_depth - 1
 *   ([2 e][16] each, depth e at offset 2 * refine_depth * 16 + 16 e (e - 1) doubles): candidates whose depth the array
 *   ends clip to e >= 3 (cross-correlation passes) then take the polynomial form too (ABI 6).
 *   With params_host[17] = 2 (single-threshold cross-correlation analyses; the harmonicity pass: depth 700) sinc_cheb holds
 *   ONE TABLE PER CELL instead (mshds.sinc_cell_tables): cells b = brent_ixmax + lag_lo - 1 .. brent_ixmax + lag_hi
 *   (lag_lo = max(min_lag, 2), lag_hi = min(max_lag, brent_ixmax) - 1), each [ntap_pad][16] with ntap_pad = max_lag + 1
 *   rounded up to a multiple of 4: row m = the sum of the rows of the cell's own depth min(depth, b + 1, RN - b - 1) that
 *   meet lag +m and lag -m of the symmetric correlation array; the coefficients of every cell of the batch are then built
 *   by a per-cell GEMM on the fp64 matrix pipe, clipped depths included (pitch_cell_coef_kernel).
 * workspace: per frame the correlation row (between the correlation kernel - fp64 FFT auto- / cross-correlation, one wave
 *   per frame - and the candidate kernel), the Chebyshev coefficient blocks of two candidate lists (2 x 4 KB) and a 128-byte
 *   record (between the candidate kernel and the refinement kernels: the Brent search runs one candidate per lane in its own
 *   kernel); at least rsaf_mshds_pitch_workspace_bytes_per_clip bytes, the clips are processed in groups of
 *   floor(workspace_bytes / that).  Environment RSAF_PITCH_INKERNEL=1: refinement inside the candidate kernel (the form
 *   before round 4; the tests' A/B reference). */
int64_t rsaf_mshds_pitch_workspace_bytes_per_clip(int max_frames, const double* params_host);
int rsaf_mshds_pitch(const float* wav, const void* clip_info, int n_clips, int max_frames, const double* gpeak,
                     const double* window, const double* window_r, const double* params_host,
                     void* frame_out, unsigned char* psi, int* end_state, double* sel_freq, double* sel_strength,
                     double* stats_out, const double* sinc_cheb, void* workspace, int64_t workspace_bytes,
                     rsaf_stream_t stream);
/* The same analysis for two voicing thresholds at once (src/mshds_extractor.py:178 and :270 differ in nothing
 * else): one frame kernel computes the correlation and refines the union of the two candidate lists, the path
 * finder runs per threshold.  The *2 outputs have the shapes of their first-threshold counterparts. */
int rsaf_mshds_pitch_dual(const float* wav, const void* clip_info, int n_clips, int max_frames, const double* gpeak,
                          const double* window, const double* window_r, const double* params_host,
                          void* frame_out, unsigned char* psi, int* end_state, double* sel_freq, double* sel_strength,
                          double* stats_out, double voicing_threshold2, void* frame_out2, unsigned char* psi2,
                          int* end_state2, double* sel_freq2, double* sel_strength2, double* stats_out2,
                          const double* sinc_cheb, void* workspace, int64_t workspace_bytes, rsaf_stream_t stream);
/* _speechrate (src/mshds_extractor.py:11-125) from the 50 Hz / 16 ms intensity contour (rsaf_mshds_intensity)
 * and the 4-candidate pitch pass of :104.  out[clip][5] = Speaking_Rate, Articulation_Rate,
 * Phonation_Ratio, Pause_Rate, Mean_Pause_Dur.  workspace: n_clips * workspace_doubles(max_frames). */
int64_t rsaf_mshds_speechrate_workspace_doubles(int max_frames);
int rsaf_mshds_speechrate(const double* intensity_db, const void* clip_info, int n_clips, int max_frames,
                          double intensity_dt, const double* sel_freq, const void* pitch_clip_info,
                          double pitch_dt, double pitch_ceiling, double* workspace, double* out,
                          rsaf_stream_t stream);
/* _measureFormants (src/mshds_extractor.py:303-338): To Formant (burg) 5 ms / 5 formants / 5 kHz / 25 ms /
 * 50 Hz on a 10 kHz resampling of the clip, To Pitch (cc) (rsaf_mshds_pitch, is_cc), To PointProcess (cc),
 * then F1,B1,F2,B2 linearly interpolated at every pulse -> mean and sample SD.
 * resample_info: device array of {int64 sample_off; int64 out_off; double pos0; double x1o; int32 n_in;
 * int32 n_out; int32 table; int32 pad} (48 bytes).  The 10 kHz resampling is Praat's Sound_resample(10000, 500):
 * `lowpassed` = the clips after rsaf_praat_lowpass_batch (same layout as wav, float64); tables: [n_tables][5][table_stride]
 * float64 NUM_interpolate_sinc weights at full depth (tap k < 2*depth+1 belongs to input base + k - depth; zeros up to
 * table_stride >= rsaf_mshds_resample10k_table_stride(depth)); phase_base:
 * [n_tables][5] int32 = floor(pos0 + 1.6 r) (output m = 5q + r reads input 8q + base); outputs whose depth Praat
 * clips at the ends of the sound are evaluated directly.
 * frames_out: per frame {double f[5]; double b[5]} (NaN padded); pulses: [n_clips][max_pulses] times (unsorted);
 * stats out[clip][8] = mean/SD of F1, B1, F2, B2 in the reference's column order. */
int rsaf_mshds_resample10k_table_stride(int depth);
int rsaf_mshds_resample10k(const double* lowpassed, const void* resample_info, int n_clips, int max_out,
                           const double* tables, int table_stride, const int* phase_base, int depth, double* out,
                           rsaf_stream_t stream);
int rsaf_mshds_formants(const double* y10, const void* resample_info, const void* clip_info, int n_clips,
                        int max_frames, const double* window, int nsamp_window, double time_step, double dx_out,
                        double preemph_factor, void* frames_out, rsaf_stream_t stream);
/* pulses[clip][max_pulses] in ascending time, n_pulses[clip]; workspace sized by
 * rsaf_mshds_pulses_workspace_bytes (stretch table and per-stretch pulse slots). */
int64_t rsaf_mshds_pulses_workspace_bytes(int n_clips, int max_frames, double pitch_dt, double pitch_ceiling);
int rsaf_mshds_pulses(const float* wav, const void* pitch_clip_info, int n_clips, int max_frames, const double* sel_freq,
                      double pitch_dt, double pitch_ceiling, void* workspace, int64_t workspace_bytes, double* pulses,
                      int max_pulses, int* n_pulses, rsaf_stream_t stream);
/* Ltas (pitch-corrected) 0-5000 Hz in 100 Hz bands from the time-sorted pulses of rsaf_mshds_pulses, then
 * "Get slope" (50-1000 vs 1000-4000 Hz, dB) and the slope of the robust line fit over 100-5000 Hz:
 * out[clip][2] = {Spectral_Slope, Spectral_Tilt}, NaN where Praat raises.
 * Replaces call(snd, "To Ltas (pitch-corrected)...") + "Get slope" + "Report spectral tilt",
 * src/mshds_extractor.py:239-249.  clip_info rows need sample_off and n_samples only. */
int rsaf_mshds_ltas_slope_tilt(const float* wav, const void* clip_info, int n_clips, const double* pulses,
                               int max_pulses, const int* n_pulses, double shortest_period, double longest_period,
                               double max_period_factor, double* out, rsaf_stream_t stream);
/* Mean cepstral peak prominence (CPPS) of the voiced stretches: out[clip], NaN when no stretch exceeds 4 dB or
 * Praat would raise.  Voiced intervals from the time-sorted pulses ("To TextGrid (vuv)" 0.02 0.1, times rounded
 * to 6 decimals like "Down to Table"), each extracted, resampled to 10 kHz as Sound_resample (10000, 50) does it (FFT
 * low-pass of the extracted part over its own power of two, NUM_interpolate_sinc), "To PowerCepstrogram" 60 0.002 5000 50,
 * "Get CPPS" no 0.01 0.001 60 330 0.05 parabolic 0.001 0 Straight Robust.
 * Replaces src/mshds_extractor.py:272-297.  Workspaces (caller-owned, per clip): seg_table
 * [max_seg][rsaf_mshds_cpp_seg_doubles()] doubles, hdr [4] ints = {intervals, 1 if the clip failed, frames in all,
 * resampled samples in all} (csrc/mshds_cpp_layout.h: Seg, ClipHdr), resampled [cap_res], cepstrogram
 * [cap_frames][513], cpp_frames [cap_frames] doubles, lp_work [cap_work] complex doubles (cap_work >= longest clip +
 * 2000 max_seg covers every case); lowpassed: float64 scratch for the samples wav[lp_origin ...] of the clips of this
 * call (sample s of the batch at lowpassed[s - lp_origin]); lg_max = log2 of the first power of two >= longest clip +
 * 2000.  window1000 = the 1000-point Gaussian window of Sound_createGaussian, twiddle1024[k] = (cos, -sin)(2 pi k / 1024),
 * k < 512. */
int rsaf_mshds_cpp_seg_doubles(void);
int rsaf_mshds_cpp(const float* wav, const void* clip_info, int n_clips, const double* pulses, int max_pulses,
                   const int* n_pulses, const double* window1000, const double* twiddle1024, int max_seg, int cap_res,
                   int cap_frames, void* seg_table, int* hdr, double* resampled, double* cepstrogram, double* cpp_frames,
                   double* lowpassed, int64_t lp_origin, void* lp_work, int64_t cap_work, int lg_max, double* out,
                   rsaf_stream_t stream);
int rsaf_mshds_formant_stats(const void* frames, const void* clip_info, int n_clips, double time_step,
                             const double* pulses, int max_pulses, const int* n_pulses, double* out,
                             rsaf_stream_t stream);
int rsaf_mshds_hnr_mean(const double* sel_freq, const double* sel_strength, const void* clip_info, int n_clips,
                        double* out, rsaf_stream_t stream);
/* moments[frame][5] = {gate, CoG, SD, skewness, kurtosis}; stats_out[clip][4] = means over gated frames */
int rsaf_mshds_spectral_moments(const float* wav, const void* clip_info, const void* pitch_clip_info, int n_clips,
                                int max_frames, const double* sel_freq, double pitch_dt, double ceiling,
                                const double* window, const double* twiddle, int nsamp_window, int nfft,
                                int nbins, double time_step, double freq_step, double* moments,
                                double* stats_out, rsaf_stream_t stream);

/* ---- sample-rate conversion in front of the extractors ---------------------------------- */
/* Interleaved little-endian integer PCM (1 = unsigned 8 bit, 2, 3, 4 bytes per sample) -> float32 in [-1, 1),
 * channel mean in float32.  Replaces torchaudio.load + waveform.mean(dim=0), src/foundation_model_extractor.py:87-91
 * (and the mono conversion of parselmouth.Sound / cWaveSource monoMixdown). */
int rsaf_pcm_to_mono_f32(const void* pcm, int sample_width, int n_channels, int64_t n_frames, float* out,
                         rsaf_stream_t stream);
/* torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff
 * 0.99): out[i * n_phase + p] = sum_k taps[p][k] * in[i * orig + tap_start[p] + k] (zero outside the input), with
 * orig/new already divided by their gcd, n_phase = new, n_out = ceil(new * n_in / orig).  The host builds the
 * taps (resample.sinc_hann_taps).  Replaces src/foundation_model_extractor.py:93-94. */
int rsaf_resample_sinc_hann(const float* in, int64_t n_in, const float* taps, const int* tap_start, int n_phase, int orig,
                            int taps_per_phase, float* out, int64_t n_out, rsaf_stream_t stream);
/* Praat Sound.resample(fs_out, precision) as Praat does it (published Sound_resample): when the rate goes down, a
 * brick-wall low-pass of the whole sound by a real FFT over the first power of two >= n_in + 2000 samples (bins from
 * floor(fs_out / fs_in * nfft) in Praat's packed order cleared), then NUM_interpolate_sinc(precision) on the new sample
 * grid centred in the old time domain; n_out = round(n_in / fs_in * fs_out).  `work`: device scratch of at least
 * rsaf_resample_praat_work_bytes(...) bytes (0 when the rate goes up: may be NULL).  Sounds of up to 2^24 - 2000
 * samples.  Not restated: the special case of a ratio of exactly 2 (Sound_upsample), which takes the general branch.
 * Replaces snd.resample(16000, 50), src/mshds_extractor.py:419. */
int64_t rsaf_resample_praat_work_bytes(int64_t n_in, double fs_in, double fs_out);
/* The low-pass step alone over a batch of sounds (the 10 kHz resampling inside To Formant (burg)): sigs = device array of
 * {int64 in_off; int64 out_off; int64 work_off; int32 n; int32 lg} (32 bytes): n float samples at in + in_off ->
 * n float64 samples at out + out_off, through 2^(lg-1) complex numbers at work + work_off (2^lg = first power of two
 * >= n + 2000, 11 <= lg <= lg_max <= 24); upfactor = new rate * old sample period < 1; work_complex = complex numbers
 * in `work`. */
/* Longest sound (samples) the whole-sound FFT low-pass takes: 2^26 - 2000 (25 min at 44.1 kHz, 69 min at 16 kHz); the
 * transform runs as two LDS passes of at most 8192 x 4096 complex points.  Longer input: rsaf_resample_praat /
 * rsaf_praat_lowpass_batch return RSAF_ERR_ARG; the MSHDS drop-in then gives NaN for the formant columns of that clip only
 * (16 kHz input) or the reference's per-file NaN row (other rates). */
int64_t rsaf_praat_lowpass_max_samples(void);
int rsaf_praat_lowpass_batch(const float* in, const void* sigs, int n_sigs, int lg_max, double upfactor, void* work,
                             int64_t work_complex, double* out, rsaf_stream_t stream);
int rsaf_resample_praat(const float* in, int64_t n_in, double fs_in, double fs_out, int precision, float* out,
                        int64_t n_out, void* work, int64_t work_bytes, rsaf_stream_t stream);

/* ---- session aggregation and batch assembly behind the extractors ---------------------- */
/* out[seg][col][2] = {mean, sample standard deviation (n-1)} over the rows row_index[seg_off[seg] .. seg_off[seg+1])
 * of rows[.][ld], NaN skipped, NaN when fewer than 1 / 2 values remain.
 * Replaces merged_df.groupby('unique_participant_id').agg(['mean', 'std']), src/utils.py:49. */
int rsaf_segment_mean_std(const double* rows, int64_t ld, const int* row_index, const int* seg_off, int n_seg, int width,
                          double* out, rsaf_stream_t stream);
/* out[plane][seg][col] = mean over rows seg_off[seg] .. seg_off[seg+1] (device int64, n_seg + 1 entries) of
 * rows[plane * plane_floats + row * ld + col], float32 in and out, summed in fp64 in row order (deterministic); NaN for an empty
 * segment.  Pools n_planes Wav2Vec2 hidden states per file at once: np.mean(sequence, axis=0),
 * src/foundation_model_extractor.py:160. */
int rsaf_rows_segment_mean_f32(const float* rows, int64_t ld, int64_t plane_floats, int n_planes, const int64_t* seg_off,
                               int n_seg, int width, float* out, rsaf_stream_t stream);
/* dst[r][0..width) = src[src_row[r]][0..width), zeros where src_row[r] < 0.
 * Replaces np.vstack(participant_sequences), src/utils.py:96, and the zero padding of collate_fn,
 * src/dl_cv_strategies.py:81-84. */
int rsaf_gather_rows_f32(const float* src, int64_t ld_src, const int64_t* src_row, int64_t n_rows, int width, float* dst,
                         int64_t ld_dst, rsaf_stream_t stream);

/* ---- Device-resident training data: the padded batches of K loader steps in ONE launch --------------------------------
 * The sequences of a data set live back to back in one float32 arena [arena_rows][width] on the device; a batch is B
 * members, member b being the row_count[b] frames from arena row row_start[b] on (both arrays on the device).
 *   out[b][t] = arena[row_start[b] + t]  for t < min(row_count[b], T),  zeros for every other t
 * (collate_fn's pad_sequence(batch_first = True, padding_value = 0), src/dl_cv_strategies.py:81-84, T the longest
 * member).  The kernel writes the zeros itself: no memset, no index array.  A member of 0 (or fewer) frames is a
 * block of zeros.  An arena row outside [0, arena_rows) is never read: it gives a zero row.  With the four label
 * fields, label_out[b] = label_src[label_index[b]], and -1 where label_index[b] is outside [0, label_count) (never read).
 * 16-byte loads and stores where width % 4 == 0 and `arena` and `out` are 16-byte aligned, dwords otherwise; element
 * offsets are 64-bit.  The items travel by value in the kernel arguments; each has its own B and T.
 * Checks, all before the launch, rsaf_last_error() naming the item: 1 <= K <= RSAF_CNNLSTM_GROUP_MAX, width >= 1,
 * B >= 1, T >= 1, B * T * width < 2^40, no NULL among arena, row_start, row_count and out, the four label fields
 * given together or not at all, no two `out` / `label_out` ranges of the call overlapping; and the call fits one grid
 * (fewer than 2^31 workgroups of 256 float4 or float elements over all items).
 * `frames`: the frames the item copies, sum of min(row_count[b], T), as the host knows them; it only sizes the bytes
 * of the profiling family "train_collate" (floats read + written); negative: counted as B * T. */
typedef struct {
    const float* arena;            /* device [arena_rows][width] */
    int64_t arena_rows;
    const int64_t* row_start;      /* device [B] */
    const int32_t* row_count;      /* device [B] */
    int B, T;
    float* out;                    /* device [B][T][width], written in full */
    const int64_t* label_src;      /* device [label_count], or NULL with the other three */
    int64_t label_count;
    const int64_t* label_index;    /* device [B] */
    int64_t* label_out;            /* device [B] */
    int64_t frames;
} rsaf_collate_item;
int rsaf_collate_pad_group(const rsaf_collate_item* items_host, int K, int width, rsaf_stream_t stream);

/* ---- Augmentations inside the collate launch, from a counter-based generator -----------------------------------------
 * rsaf_collate_augment_group is rsaf_collate_pad_group with a pipeline of up to RSAF_AUGMENT_MAX augmentation ops per
 * item, applied in order to every member BEFORE it is padded (the reference's SequenceDataset applies `transform` per
 * item, src/dl_cv_strategies.py:19-62, and collate_fn pads afterwards): the padding stays +0.0 under every pipeline.
 * Every augmented value is a pure function of (seed, epoch, sample, op, element): no generator state lives on the
 * device, and a member gets the same bits in any batch, at any T, in any group and on either store path.  No op changes
 * the number of frames.
 *
 * The generator is the Philox4x32-10 of the dropout masks (above).  key = (seed & 0xffffffff, seed >> 32).  Member b is
 * sequence sample_id[b] (its index in the store, < 2^32).  Op number s (0-based) of the pipeline uses two streams:
 *   parameter block: counter = (0, 0x100 + 2 s, sample_id, epoch)            -> words w0 .. w3
 *   element blocks : counter = (j, 0x100 + 2 s + 1, sample_id, epoch), j = e >> 2, for the flat index e = t * width + d of
 *                    the element in the member's own [frames][width] layout (so e does not depend on the batch)
 * The op fires iff `always` != 0 or w0 < fire_threshold; the host sets always = (p >= 1) and fire_threshold =
 * floor(p * 2^32) otherwise.  u(w) = (w >> 8) * 2^-24.  What a firing op does, by `kind`:
 *   0 Scale          x <- x * f, f = (float)(a + (b - a) * u(w1)): difference, product and sum in double, each rounded,
 *                    not fused; one rounding to float; the product with x in float
 *   1 GaussianNoise  x <- fmaf(amp, z[e], x), amp formed like f from w1.  The element block j with words (A, B, C, D)
 *                    gives four normals by Box-Muller in float: u1 = ((A >> 8) + 1) * 2^-24 (in (0, 1]),
 *                    u2 = (B >> 8) * 2^-24, r = sqrt(-2 ln u1), z[4j] = r cos(2 pi u2), z[4j+1] = r sin(2 pi u2); the pair
 *                    (C, D) gives z[4j+2] and z[4j+3] in the same way
 *   2 TimeMask       n = the member's own number of frames (row_count[b], not T): lo = floor(n * a), hi = floor(n * b) in
 *                    double, len = lo + (((uint64) w1 * (hi - lo + 1)) >> 32), start = ((uint64) w2 * (n - len + 1)) >> 32;
 *                    frames [start, start + len) become +0.0
 *   3 FeatureMask    the same with n = width: columns [start, start + len) of every frame become +0.0
 * Everything but z is integer or single-rounded arithmetic and is the same bits in any restatement; z comes from the
 * accurate logf, sqrtf and sincospif (no fast intrinsics) and is within 2^-17 of the exact value.
 *
 * `ops` is the op table on the device (the kernel reads it through uniform loads), `ops_host` the same n_ops entries in
 * host memory: the entry checks those and never reads device memory.  An item with n_ops = 0 is a plain collate item
 * (ops, ops_host and sample_id may be NULL) and gets the bits of rsaf_collate_pad_group.
 * Checks, all before the launch, rsaf_last_error() naming the item and, where there is one, the op: everything
 * rsaf_collate_pad_group checks; 0 <= n_ops <= RSAF_AUGMENT_MAX; with n_ops > 0: ops, ops_host and sample_id not NULL,
 * every kind known, a and b finite, epoch < 2^32 and T * width < 2^34 (element blocks are counted in 32 bits).
 * Profiling family: "train_collate_augment", bytes as for "train_collate". */
#define RSAF_AUGMENT_MAX 8
typedef struct {
    int kind;                      /* 0 Scale, 1 GaussianNoise, 2 TimeMask, 3 FeatureMask */
    uint32_t fire_threshold;       /* floor(p * 2^32) */
    int always;                    /* p >= 1 */
    double a, b;                   /* min and max of the factor, the amplitude or the band part */
} rsaf_augment_op;
typedef struct {
    /* the fields of rsaf_collate_item, in its order */
    const float* arena;
    int64_t arena_rows;
    const int64_t* row_start;
    const int32_t* row_count;
    int B, T;
    float* out;
    const int64_t* label_src;
    int64_t label_count;
    const int64_t* label_index;
    int64_t* label_out;
    int64_t frames;
    /* the pipeline */
    const rsaf_augment_op* ops;       /* device [n_ops] */
    const rsaf_augment_op* ops_host;  /* host [n_ops], the same values */
    int n_ops;
    uint64_t seed;
    uint64_t epoch;                /* < 2^32 */
    const int64_t* sample_id;      /* device [B]: the members' sequence indices in the store */
} rsaf_collate_augment_item;
int rsaf_collate_augment_group(const rsaf_collate_augment_item* items_host, int K, int width, rsaf_stream_t stream);

/* ---- The layer mix inside the collate launch: resident layer stacks ----------------------------------------------------
 * A store of layer stacks keeps sequence i, [L][T_i][width] as rsaf_w2v2_forward_ragged_hidden returns it per file, as
 * L * T_i consecutive arena rows, layer-major: frame t of layer l is arena row row_start + l * T_i + t, row_start the
 * first row of the block.  width % 4 == 0; arena, out and dx 16-byte aligned.  The padded stack [B][L][T][width] of a
 * batch, L + 1 times the size of the batch the classifier reads, never exists.
 *
 * rsaf_collate_mix_group: ONE launch for K <= RSAF_CNNLSTM_GROUP_MAX items of one width, each with its own B, T, L and p:
 *   out[b][t][:] = sum_l p[l] arena[row_start[b] + l * T_b + t][:]   for t < min(T_b, T),  T_b = row_count[b]
 *   +0.0 everywhere else, written by the kernel (no memset, no index array)
 * A member whose block [row_start[b], row_start[b] + L * T_b) does not lie wholly inside [0, arena_rows) is never read and
 * comes out as zeros; a member of 0 (or fewer) frames is a block of zeros.  Per position: a = p[0] v_0, then a += p[l] v_l,
 * float32, l ascending (the one inline function of csrc/layer_mix_layout.h that rsaf_layer_mix_forward calls too), so the
 * batch has the bits of rsaf_layer_mix_forward on the zero-padded stack.  The labels are those of rsaf_collate_item.
 * Grid: the workgroups of all items back to back, each one chunk of consecutive float4 of one member's `out`; the loads
 * of four layers are issued before their adds.
 * Checks, all before the launch, rsaf_last_error() naming the item: everything rsaf_collate_pad_group checks,
 * 1 <= L <= RSAF_LAYER_MIX_MAX, width a positive multiple of 4, p not NULL, arena and out 16-byte aligned,
 * B * T * width < 2^40.  Profiling family "train_collate_mix", bytes 4 * (L * frames * width + B * T * width).
 *
 * rsaf_collate_mix_backward_group: dp_out[l] = sum over the frames that exist of arena[...] . dx[b][t][:], for K items in
 * TWO launches: one over the parts of all items, one final sum with one wave per (item, l).  Partition and summation
 * order are those of rsaf_layer_mix_backward for the padded shape (B, L, T, width) (csrc/layer_mix_layout.h); a position
 * whose frame does not exist is skipped, neither the arena nor dx is read there.  A product of two floats is exact in
 * double and a skipped term is an exact +-0 added to a sum that starts at +0.0, so dp_out has the bits of
 * rsaf_layer_mix_backward on the zero-padded stack.  No atomics: the same bits on every call, at any K.  `partials`:
 * 8-byte aligned scratch of at least rsaf_layer_mix_partials(B, L, T, width) doubles, RSAF_ERR_WORKSPACE when shorter.
 * Checks as above (dx, partials and dp_out for out; no labels); no two `partials` / `dp_out` ranges of a call overlap.
 * Profiling family "train_collate_mix_backward", bytes 4 * ((L + 1) * frames * width). */
typedef struct {
    const float* arena;            /* device [arena_rows][width] */
    int64_t arena_rows;
    const int64_t* row_start;      /* device [B]: first arena row of the member's block */
    const int32_t* row_count;      /* device [B]: the member's frames T_b */
    int B, T, L;
    const float* p;                /* device [L] */
    float* out;                    /* device [B][T][width], written in full */
    const int64_t* label_src;      /* the four label fields of rsaf_collate_item: all or none */
    int64_t label_count;
    const int64_t* label_index;
    int64_t* label_out;
    int64_t frames;                /* sum of min(T_b, T), as the host knows it; negative: counted as B * T */
} rsaf_collate_mix_item;
int rsaf_collate_mix_group(const rsaf_collate_mix_item* items_host, int K, int width, rsaf_stream_t stream);
typedef struct {
    const float* arena;
    int64_t arena_rows;
    const int64_t* row_start;
    const int32_t* row_count;
    int B, T, L;
    const float* dx;               /* device [B][T][width] */
    double* partials;              /* scratch, partials_count doubles */
    int64_t partials_count;
    float* dp_out;                 /* device [L] */
    int64_t frames;
} rsaf_collate_mix_backward_item;
int rsaf_collate_mix_backward_group(const rsaf_collate_mix_backward_item* items_host, int K, int width, rsaf_stream_t stream);

/* rsaf_layer_mix_adam_group: the step of the L mix weights of K items in ONE launch, one wave per item.
 * mode RSAF_LAYER_MIX_FROM_DP: the gradient is the softmax Jacobian applied to dp in double,
 *     dw_l = p_l (dp_l - sum_j p_j dp_j), the sum by the xor butterfly over the lanes, dw_l rounded to float once
 *     (written to dw_out where that is not NULL);
 * mode RSAF_LAYER_MIX_FROM_DW: the gradient is dw as given (the `.grad` of the weights).
 * Then the published Adam update of rsaf_cnnlstm_adam_group (the same arithmetic: moments and update in double from the
 * float operands, each rounded to float once; bias-corrected, eps outside the square root, no weight decay) on w,
 * exp_avg, exp_avg_sq (device [L] each) with the item's lr, betas, eps and 1-based step, and
 *     p_next_l = (float)(exp(w_l - max_j w_j) / sum_j exp(w_j - max_j w_j))      of the NEW w, in double, rounded once.
 * mode RSAF_LAYER_MIX_SOFTMAX_ONLY: p_next from w as it stands; nothing else is read or written.
 * L = 1 gives dw = 0 exactly and leaves w bit for bit.  Checks before the launch: 1 <= K <= RSAF_CNNLSTM_GROUP_MAX,
 * 1 <= L <= RSAF_LAYER_MIX_MAX, a known mode, the pointers the mode reads or writes, and for the two stepping modes
 * step >= 1, 0 <= beta < 1, eps >= 0, lr >= 0.  Profiling family "layer_mix_adam".
 *
 * Launch census of a group step of K <= RSAF_CNNLSTM_GROUP_MAX replicas with a learned mix each (cnnlstm_mix_train_step_group),
 * on top of the launches of the fused step above (packing, dropout masks, forward, loss, backward through the _dx entries, Adam,
 * running statistics), whatever K: 1 x rsaf_collate_mix_group (it replaces the step's rsaf_collate_pad_group), 2 launches of
 * rsaf_collate_mix_backward_group, 1 x rsaf_layer_mix_adam_group, which leaves the p of the next step; a softmax-only launch of
 * the same entry only where weights were changed from outside since the last step.  No launch reads or writes a [B][L][T][width]
 * tensor. */
#define RSAF_LAYER_MIX_FROM_DP 0
#define RSAF_LAYER_MIX_FROM_DW 1
#define RSAF_LAYER_MIX_SOFTMAX_ONLY 2
typedef struct {
    int L, mode;
    const float* p;                /* device [L], FROM_DP */
    const float* dp;               /* device [L], FROM_DP */
    const float* dw;               /* device [L], FROM_DW */
    float* dw_out;                 /* device [L] or NULL, FROM_DP */
    float* w;                      /* device [L] */
    float* exp_avg;
    float* exp_avg_sq;
    float* p_next;                 /* device [L] */
    double lr, beta1, beta2, eps;
    int64_t step;
} rsaf_layer_mix_adam_item;
int rsaf_layer_mix_adam_group(const rsaf_layer_mix_adam_item* items_host, int K, rsaf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSAF_H */
