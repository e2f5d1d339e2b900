/*
 * tcresnet_hip.h -- C ABI of the MI355X-native (gfx950) TC-ResNet keyword-spotting hot path.
 *
 * The reference (hyperconnect/TC-ResNet, TF 1.13 graph code) has no FFI/plugin boundary for this
 * path: every number is produced by TensorFlow ops reached from a handful of Python call sites.
 * Each entry point below replaces the TF ops behind one of those call sites (cited per function,
 * paths relative to the reference tree).  The Python host package (tc-resnet_amd/) binds this
 * header with ctypes and exposes the reference's own class/argument names on top of it.
 *
 * Conventions
 *   - every function returns 0 on success, a negative tcr_status otherwise; tcr_last_error()
 *     returns a thread-local message.  Nothing throws, nothing allocates device memory:
 *     all device buffers (including workspaces) are caller-owned, contiguous float32.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, asynchronously.
 *   - activations are planar per utterance with a zero halo on the time axis:
 *       act[b][c][TCR_HALO + t],  row length Tp = T + 2*TCR_HALO  (tcr_padded_len(T)).
 *     The halo implements TF "SAME" zero padding without per-tap bounds checks.
 *   - conv weights keep the reference checkpoint layout [k][Cin][Cout] (= TF HWIO [k,1,Cin,Cout]).
 */
#ifndef TCRESNET_HIP_H
#define TCRESNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCR_ABI_VERSION 3
#define TCR_HALO 4
#define TCR_MAX_BLOCKS 16

typedef enum tcr_status {
    TCR_OK = 0,
    TCR_ERR_ARG = -1,          /* invalid argument / unsupported configuration */
    TCR_ERR_HIP = -2,          /* a HIP call or kernel launch failed */
    TCR_ERR_WORKSPACE = -3     /* workspace too small */
} tcr_status;

int tcr_abi_version(void);
const char* tcr_last_error(void);
static inline int tcr_padded_len(int t) { return t + 2 * TCR_HALO; }

/* ------------------------------------------------------------------------------------------ */
/* Front-end: MFCC / log-mel (datasets/preprocessors.py:54-96,183-194; window/stride samples   */
/* from factory/audio_nets.py:62-64; flags from datasets/audio_data_wrapper.py:61-110).        */
/* ------------------------------------------------------------------------------------------ */
typedef struct tcr_frontend_cfg {
    int32_t sample_rate;        /* --sample_rate 16000 */
    int32_t n_samples;          /* sample_rate * clip_duration_ms / 1000 */
    int32_t win;                /* window_size_samples  */
    int32_t hop;                /* window_stride_samples */
    int32_t nfft;               /* out: enclosing power of two of win (tf.contrib.signal.stft) */
    int32_t n_frames;           /* out: 1 + (n_samples - win) / hop (signal.frame, pad_end=False) */
    int32_t n_mel;              /* --num_mel_bins (64) */
    int32_t n_coef;             /* --num_mfccs for mfcc; ignored (== n_mel) for log-mel */
    float lower_hz;             /* --lower_edge_hertz 80 */
    float upper_hz;             /* --upper_edge_hertz 7600 */
    int32_t method;             /* 0 = mfcc (power spectrum + DCT-II), 1 = log_mel_spectrogram (magnitude),
                                 * 2 = deploy-path mfcc: contrib_audio.audio_spectrogram + contrib_audio.mfcc op semantics
                                 *     (datasets/preprocessors.py:98-124,196-203): magnitude-weighted mel filterbank of the op,
                                 *     log(max(x, 1e-12)), the same sqrt(2/N) DCT-II */
} tcr_frontend_cfg;

/* Fills nfft / n_frames and validates the configuration. */
int tcr_frontend_resolve(tcr_frontend_cfg* cfg);
/* Size in bytes of the constant tables (Hann window, FFT twiddles, HTK mel slopes, DCT-II). */
size_t tcr_frontend_plan_bytes(const tcr_frontend_cfg* cfg);
/* Builds the tables in HOST memory (computed in float64, stored float32); the caller uploads
 * them once to a device buffer of the same size and passes that pointer to tcr_frontend_fwd. */
int tcr_frontend_plan_init(const tcr_frontend_cfg* cfg, void* host_plan);
/* Dense [n_bins][n_mel] mel matrix / [n_mel][n_coef] DCT matrix reconstructed from a plan
 * (host side; for tests and for exporting the constants). */
int tcr_frontend_plan_mel_matrix(const tcr_frontend_cfg* cfg, const void* host_plan, float* out);
int tcr_frontend_plan_dct_matrix(const tcr_frontend_cfg* cfg, const void* host_plan, float* out);

/* wav [batch][n_samples] -> feat [batch][n_coef][Tp] (halo zeroed), Tp = tcr_padded_len(n_frames).
 * Replaces tf.contrib.signal.stft / linear_to_mel_weight_matrix / tensordot / log /
 * mfccs_from_log_mel_spectrograms (datasets/preprocessors.py:68-94,191-193). */
int tcr_frontend_fwd(const tcr_frontend_cfg* cfg, const void* plan_dev, const float* wav, int batch,
                     float* feat, void* stream);
/* The same with a per-call launch hint: `rounds` > 0 fixes the packed kernels' rounds of frames per persistent-workgroup chunk
 * (clamped to what the kernel supports; 0 = the launcher's cost model, i.e. tcr_frontend_fwd).  A caller that runs the front-end
 * next to other kernels (tcresnet_amd.pipeline) passes its own measured choice here instead of flipping the process-wide
 * TCR_TUNE_FRONTEND knob around the launch.  Results do not depend on it. */
int tcr_frontend_fwd_rounds(const tcr_frontend_cfg* cfg, const void* plan_dev, const float* wav, int batch,
                            float* feat, int rounds, void* stream);

/* "no_preprocessing" (datasets/preprocessors.py:45-49): re-layout a reference-shaped feature
 * tensor [batch][T][F] into the planar halo layout [batch][F][Tp], and back. */
int tcr_features_to_planar(const float* ntf, int batch, int t, int f, float* planar, void* stream);
int tcr_features_from_planar(const float* planar, int batch, int t, int f, float* ntf, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Network: TC-ResNet (audio_nets/tc_resnet.py:6-70, arg scope :102-123)                       */
/* ------------------------------------------------------------------------------------------ */
typedef struct tcr_tcresnet_cfg {
    char scope[32];                 /* "TCResNet8" / "TCResNet14": TF variable scope (tc_resnet.py:57,65) */
    int32_t in_channels;            /* MFCC coefficients (become channels, tc_resnet.py:17) */
    int32_t t_in;                   /* number of frames L */
    int32_t num_classes;
    int32_t n_blocks;
    int32_t channels[TCR_MAX_BLOCKS + 1];   /* n_channels after width_multiplier (tc_resnet.py:59-60) */
    float bn_decay;                 /* 0.997 (tc_resnet.py:107) */
    float bn_eps;                   /* 0.001 (slim.batch_norm default) */
} tcr_tcresnet_cfg;

typedef struct tcr_net tcr_net;     /* opaque, host-only (no device allocations) */

int tcr_tcresnet_create(const tcr_tcresnet_cfg* cfg, tcr_net** out);
void tcr_net_destroy(tcr_net* net);

/* Parameter arena layout.  Trainables live in ONE flat float32 arena (so that the optimiser step
 * and the data-parallel gradient all-reduce are one call each): all conv/fc weights first
 * (these are the L2-regularised variables of factory/audio_nets.py:175-180), then BN gamma/beta.
 * Moving statistics live in a second arena.  Offsets are in floats. */
typedef enum tcr_tensor_kind {
    TCR_WEIGHT = 0, TCR_GAMMA = 1, TCR_BETA = 2, TCR_MOVING_MEAN = 3, TCR_MOVING_VAR = 4
} tcr_tensor_kind;

typedef struct tcr_tensor_info {
    char name[96];          /* TF variable name, e.g. "TCResNet8/block0/conv0_0/BatchNorm/gamma" */
    int32_t kind;           /* tcr_tensor_kind */
    int32_t arena;          /* 0 = trainable arena, 1 = moving-stat arena */
    int64_t offset;         /* floats */
    int64_t size;           /* floats */
    int32_t shape[4];       /* TF shape, e.g. [9,1,16,24] */
    int32_t rank;
} tcr_tensor_info;

int64_t tcr_net_param_floats(const tcr_net* net);      /* trainable arena size (padded) */
int64_t tcr_net_decay_floats(const tcr_net* net);      /* prefix of the arena that is L2-regularised */
int64_t tcr_net_stat_floats(const tcr_net* net);       /* moving-stat arena size */
int tcr_net_num_tensors(const tcr_net* net);
int tcr_net_tensor_info(const tcr_net* net, int index, tcr_tensor_info* out);
int tcr_net_out_frames(const tcr_net* net);            /* L' after the last block */
int tcr_net_feat_channels(const tcr_net* net);         /* channels into fc */

/* Workspace size for a batch; train != 0 includes saved activations and gradient scratch. */
size_t tcr_net_workspace_bytes(const tcr_net* net, int batch, int train);

/* Eval-mode forward (is_training=False: BN uses moving stats, dropout off):
 * tc_resnet() + slim.softmax (audio_nets/tc_resnet.py:6-54, factory/audio_nets.py:147-156),
 * i.e. what Base.run_inference fetches (helper/base.py:86-104).
 * feat [batch][Cin][Tp]; logits/probs [batch][num_classes]; ranges [batch][2] (may be NULL). */
int tcr_net_forward_infer(const tcr_net* net, const float* params, const float* stats, const float* feat,
                          int batch, void* workspace, size_t workspace_bytes,
                          float* logits, float* probs, float* ranges, void* stream);

/* Deployable ("frozen") form of the network (factory/audio_nets.py:87-125 build_deployable_model + freeze.py:16-49
 * convert_variables_to_constants): eval-mode BN folded into per-channel (scale, shift) constants.
 *   tcr_net_frozen_floats   size of the constant table;
 *   tcr_net_fold_bn         params + moving stats -> the table (what a frozen export stores next to the conv weights);
 *   tcr_net_forward_frozen  eval forward from (conv weights in `params`, table): no variable is read, the BN entries of
 *                           `params` and the moving statistics are not needed.  Bitwise tcr_net_forward_infer.
 * Layout of the table (tcr_net_frozen_floats floats, every caller sizes it by that call): per BN unit scale[c_pad], shift[c_pad]
 * (offsets and contents as ever); rounded up to 4 floats; a header of 4 words {flag, image floats, 0, 0}; the WEIGHT IMAGE: every
 * conv layer's weights in the order a lane of the fused eval kernel reads its matrix fragments,
 *   [layer, forward order][row tile m][tap j][c4 / 4][lane 0..63][width],
 * c4 the channel quad, width = 4 (the last group of a tap: C4 % 4 when that is not 0, C4 = Cin / 4), lane = 16 q + r holding
 * W[j][4 c4 + q][min(16 m + r, Cout - 1)] -- one 16-byte load per lane for four channel quads of a tap where the kernel took four
 * 4-byte loads at scattered rows.  (Networks with a layer of Cin % 4 != 0 have no image: the table ends behind the header.)
 *   tcr_net_fold_bn         writes scale / shift and CLEARS the flag: with the flag clear every call that takes the table reads the conv
 *                           weights from `params`, exactly as before the image existed;
 *   tcr_net_fold_weights    writes the image from `params` and SETS the flag (table on a 16-byte boundary).  With the flag set, the
 *                           kernels that know the image (TCResNet8-1.0 at 49 frames in groups of 8, the benchmark's shape) take their CONV
 *                           WEIGHTS FROM THE TABLE, not from `params`: after changing a conv weight the caller must fold again (or
 *                           clear the flag with tcr_net_fold_bn).  fc / fc2 and every other kernel keep reading `params`.
 * A call whose plan sizes the image differently from the kernel it selects is refused (TCR_ERR_ARG). */
int64_t tcr_net_frozen_floats(const tcr_net* net);
int tcr_net_fold_bn(const tcr_net* net, const float* params, const float* stats, float* frozen_ss, void* stream);
int tcr_net_fold_weights(const tcr_net* net, const float* params, float* frozen_ss, void* stream);
int tcr_net_forward_frozen(const tcr_net* net, const float* params, const float* frozen_ss, const float* feat,
                           int batch, void* workspace, size_t workspace_bytes,
                           float* logits, float* probs, float* ranges, void* stream);

/* The whole eval path of one batch in ONE call: waveform -> MFCC -> (BN fold when `refold` != 0) -> network -> softmax, i.e.
 * model.build(wavs, labels, is_training=False) + session.run(outputs) of the reference (factory/audio_nets.py:41-60,
 * datasets/preprocessors.py:183-194, audio_nets/tc_resnet.py:6-54, helper/base.py:86-104).  Same kernels and results as
 * tcr_frontend_fwd + tcr_net_fold_bn + tcr_net_forward_frozen; it exists for small batches, where three host calls cost more than
 * the kernels (B <= 64: ~70 us -> the kernels' own time).
 * feat: caller-owned scratch for the features, [batch][n_coef][n_frames + 2 * TCR_HALO] floats; frozen_ss: the folded table
 * (tcr_net_frozen_floats), its scale / shift rewritten and its weight-image flag cleared when `refold` is non-zero (stats may be NULL
 * otherwise). */
int tcr_forward_waveform(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                         const float* stats, float* frozen_ss, int refold, const float* wav, int batch, float* feat,
                         void* workspace, size_t workspace_bytes, float* logits, float* probs, float* ranges, void* stream);

/* Train-mode forward (is_training=True): batch-statistics BN with moving-stat update
 * (decay, Bessel-corrected variance), inverted dropout after the global pool, softmax,
 * mean cross-entropy (factory/audio_nets.py:161-173).  Saves what backward needs in `workspace`.
 *   labels      [batch][num_classes] one-hot float (datasets/audio_data_wrapper.py:114-118)
 *   keep_prob   --dropout_keep_prob; the mask for sample i, channel c is a pure function of
 *               (seed, sample_offset + i, c) so that a sharded batch draws the same mask
 *   loss_out    device float[2]: {sum over the batch of -sum_k y log softmax, unused}
 *   global_batch  divisor of the mean loss / of dlogits (== batch on one GPU) */
int tcr_net_forward_train(const tcr_net* net, const float* params, float* stats, const float* feat,
                          const float* labels, int batch, int global_batch, float keep_prob,
                          uint64_t seed, int64_t sample_offset, float label_smoothing,
                          void* workspace, size_t workspace_bytes,
                          float* logits, float* probs, float* loss_out, void* stream);

/* Backward of the model loss wrt every trainable (tf.gradients inside
 * slim.learning.create_train_op, helper/trainer.py:205-211).  Must follow a forward_train on
 * the same workspace.  grads: arena-shaped, overwritten.  The L2 term is NOT added here
 * (it is folded into tcr_sgd_momentum_step / reported by tcr_l2_loss). */
int tcr_net_backward(const tcr_net* net, const float* params, const float* feat, int batch,
                     void* workspace, size_t workspace_bytes, float* grads, void* stream);

/* Cross-replica (sync) BN.  forward_train / backward can be run stage by stage: stage s ends right
 * after the per-channel partial sums of its BN layer ({sum y, sum y^2} forward, {sum dz, sum dz*xhat}
 * backward; 2*C float64 values, the per-workgroup partial rows added up in the fixed order the unstaged
 * path uses) have been written to a contiguous device buffer, which the host all-reduces (sum) across
 * replicas before calling stage s+1.  Statistics then span global_batch, exactly as in the single-device
 * reference; with one replica the staged run is bitwise the unstaged one.  Stages 0 .. tcr_net_num_stages()-1; the last stage
 * has no hand-off.  See DESIGN.md "Data parallel". */
int tcr_net_num_stages(const tcr_net* net, int backward);
int tcr_net_stage_sums(const tcr_net* net, int backward, int stage, void* workspace, int batch,
                       double** sums_dev, int64_t* n_doubles);
int tcr_net_forward_train_stage(const tcr_net* net, const float* params, float* stats, const float* feat,
                                const float* labels, int batch, int global_batch, float keep_prob,
                                uint64_t seed, int64_t sample_offset, float label_smoothing,
                                void* workspace, size_t workspace_bytes,
                                float* logits, float* probs, float* loss_out, int stage, void* stream);
int tcr_net_backward_stage(const tcr_net* net, const float* params, const float* feat, int batch, int global_batch,
                           void* workspace, size_t workspace_bytes, float* grads, int stage, void* stream);

/* The same hand-off by DEPENDENCY LEVEL (round 3): the units whose statistics become available together are handed over at once --
 * forward: conv0 | per block (down, conv_a) | conv_b; backward: per block, last first, (conv_b, down) | conv_a; then conv0 -- so a
 * training step needs 2 x (1 + 2 x blocks) all-reduces instead of 2 x (BN units): TCResNet8 14 instead of 20, TCResNet14 26 instead
 * of 32.  Levels 0 .. tcr_net_num_levels() - 1; after every level but the last the caller all-reduces (sum) the *n_doubles float64
 * values at *sums_dev (tcr_net_level_sums).  One replica: bitwise the unstaged run. */
int tcr_net_num_levels(const tcr_net* net, int backward);
int tcr_net_level_sums(const tcr_net* net, int backward, int level, void* workspace, int batch, double** sums_dev, int64_t* n_doubles);
int tcr_net_forward_train_level(const tcr_net* net, const float* params, float* stats, const float* feat, const float* labels, int batch,
                                int global_batch, float keep_prob, uint64_t seed, int64_t sample_offset, float label_smoothing,
                                void* workspace, size_t workspace_bytes, float* logits, float* probs, float* loss_out, int level, void* stream);
int tcr_net_backward_level(const tcr_net* net, const float* params, const float* feat, int batch, int global_batch,
                           void* workspace, size_t workspace_bytes, float* grads, int level, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Network: DS-CNN S / M / L (audio_nets/ds_cnn.py:19-118), the depthwise-separable baseline     */
/* ------------------------------------------------------------------------------------------ */
/* Limits.  tcr_dscnn_create refuses (TCR_ERR_ARG, tcr_last_error names the limit): h_in, w_in < 1; num_classes outside 1 .. 46
 * (the head's num_classes + 2 <= 48); depth not a positive multiple of 4; n_separable outside 1 .. 8; conv1_kh outside 1 .. 16;
 * conv1_kw != 4; a stride outside {1, 2}.  Everything create accepts runs eval (tcr_dscnn_forward_infer) at any batch.
 * TRAINING has two further limits, both of conv_1's filter gradient: conv1_kh <= 12 (kh x 4 taps in a 48-tap tile) and
 * w_in * (h_in + 8) <= 3072 floats (four copies of an utterance's padded feature map in 48 KB of LDS: 98 frames x 40 coefficients
 * do not train, 98 x 28 and 49 x 40 do).  A net beyond them is refused by the first training call -- tcr_dscnn_train_workspace_bytes
 * returns 0, tcr_dscnn_forward_train[_stage] returns TCR_ERR_ARG -- with the limit in tcr_last_error and nothing launched or
 * written; tcr_dscnn_backward is never the first to object. */
typedef struct tcr_dscnn_cfg {
    int32_t h_in;                   /* frames (49 for 40/20 ms) */
    int32_t w_in;                   /* MFCC coefficients (--num_mfccs 10) */
    int32_t num_classes;            /* 1 .. 46 */
    int32_t depth;                  /* 64 / 172 / 276 (ds_cnn.py:20,29,37); any positive multiple of 4 */
    int32_t n_separable;            /* 4 / 4 / 5 separable blocks; 1 .. 8 */
    int32_t conv1_kh, conv1_kw;     /* 10 x 4; kh 1 .. 16 (training: <= 12), kw 4 */
    int32_t conv1_sh, conv1_sw;     /* (2,2) S; (2,1) M, L; each 1 or 2 */
    int32_t ds1_sh, ds1_sw;         /* stride of conv_ds_1: (1,1) S; (2,2) M, L; each 1 or 2 */
    float bn_decay;                 /* 0.96 (ds_cnn.py:107) */
    float bn_eps;                   /* 0.001 */
} tcr_dscnn_cfg;

typedef struct tcr_dscnn tcr_dscnn;

int tcr_dscnn_create(const tcr_dscnn_cfg* cfg, tcr_dscnn** out);
void tcr_dscnn_destroy(tcr_dscnn* net);
int64_t tcr_dscnn_param_floats(const tcr_dscnn* net);   /* weights, biases, BN beta (no gamma: scale=False) */
int64_t tcr_dscnn_stat_floats(const tcr_dscnn* net);
int tcr_dscnn_num_tensors(const tcr_dscnn* net);
int tcr_dscnn_tensor_info(const tcr_dscnn* net, int index, tcr_tensor_info* out);   /* names: "DSCNN/conv_ds_1/pointwise_conv/weights", ... */
size_t tcr_dscnn_workspace_bytes(const tcr_dscnn* net, int batch);
/* Eval-mode forward: feat = front-end output [batch][w_in][tcr_padded_len(h_in)] (num_mfccs = w_in);
 * logits / probs [batch][num_classes].  DSCNN() + slim.softmax (ds_cnn.py:89-101, factory/audio_nets.py:147-156). */
int tcr_dscnn_forward_infer(const tcr_dscnn* net, const float* params, const float* stats, const float* feat,
                            int batch, void* workspace, size_t workspace_bytes, float* logits, float* probs, void* stream);

/* Train-mode forward of DSCNN() (is_training=True: batch statistics, moving averages updated with decay 0.96 --
 * DSCNN_arg_scope, ds_cnn.py:104-118) + softmax cross-entropy (factory/audio_nets.py:161-173); no dropout is applied
 * in the graph (ds_cnn.py:89-101).  Arguments as tcr_net_forward_train; the workspace keeps what backward needs. */
size_t tcr_dscnn_train_workspace_bytes(const tcr_dscnn* net, int batch);      /* 0: bad argument, or a net past the training limits above */
int tcr_dscnn_forward_train(const tcr_dscnn* net, const float* params, float* stats, const float* feat, const float* labels,
                            int batch, int global_batch, float label_smoothing, void* workspace, size_t workspace_bytes,
                            float* logits, float* probs, float* loss_out, void* stream);
/* Gradient of the model loss wrt every trainable of the arena (tf.gradients inside slim.learning.create_train_op,
 * helper/trainer.py:205-211; the reference trains DS-CNN with Adam -> tcr_adam_step).  The conv / depthwise /
 * pointwise biases feed a train-mode BN, so their gradient is identically zero and is written as 0. */
int tcr_dscnn_backward(const tcr_dscnn* net, const float* params, const float* feat, int batch,
                       void* workspace, size_t workspace_bytes, float* grads, void* stream);
/* Cross-replica (sync) BN for DS-CNN, as tcr_net_*_stage: stage u of the forward ends with unit u's {sum y, sum y^2} (2*C float64) in
 * the hand-off buffer, stage k of the backward with {sum dz, sum dz*xhat} of unit (units-1-k); the host all-reduces them between stages.
 * tcr_dscnn_num_stages() stages each way; with one replica the staged run is bitwise the unstaged one. */
/* Where a training forward left the post-BN+ReLU activation of BN unit `unit` (0 = conv_1, then depthwise / pointwise of every
 * separable block) inside the caller's training workspace: [batch][channels][padded] floats at float offset *offset, the `positions`
 * values of a plane behind a TCR_HALO-float halo.  The reference's `endpoints` of ds_cnn.py:46-62,104-118; used by the parity tests
 * to take the float64 oracle's gradient on the kernels' side of ReLU inputs within round-off of zero. */
int tcr_dscnn_num_units(const tcr_dscnn* net);
int tcr_dscnn_unit_output(const tcr_dscnn* net, int unit, int batch, int64_t* offset, int* channels, int* positions, int* padded);
/* The default training path never writes that activation (its consumers apply BN + ReLU to the unit's raw conv output as they read it,
 * TCR_TUNE_DS_TRAIN): this call computes it from the raw output and the batch statistics the last training forward left in the workspace,
 * into the slot tcr_dscnn_unit_output() names.  Replaces nothing in the reference (test / inspection hook for `endpoints`). */
int tcr_dscnn_materialize_unit(const tcr_dscnn* net, int unit, int batch, void* workspace, size_t workspace_bytes, void* stream);
/* Test hook, host arithmetic only: how the depthwise filter gradient splits `batch` utterances of `positions` output positions into
 * chunks, and whether its plain kernel may split a chunk's flattened index with the float reciprocal (exact below 2^22) or divides. */
int tcr_dscnn_dw_wgrad_plan(int batch, int positions, int* chunks, int* utt_per_block, int* fast_divide);
int tcr_dscnn_num_stages(const tcr_dscnn* net);
int tcr_dscnn_stage_sums(const tcr_dscnn* net, int backward, int stage, void* workspace, int batch, double** sums_dev, int64_t* n_doubles);
int tcr_dscnn_forward_train_stage(const tcr_dscnn* net, const float* params, float* stats, const float* feat, const float* labels,
                                  int batch, int global_batch, float label_smoothing, void* workspace, size_t workspace_bytes,
                                  float* logits, float* probs, float* loss_out, int stage, void* stream);
int tcr_dscnn_backward_stage(const tcr_dscnn* net, const float* params, const float* feat, int batch, int global_batch,
                             void* workspace, size_t workspace_bytes, float* grads, int stage, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Generic 2-D layer graph: the other model families behind the factory        */
/*   ResNet2D8 / ResNet2D8Pool (audio_nets/tc_resnet.py:14-15,23-24,73-99),                       */
/*   Res8 / Res8Narrow / Res15 / Res15Narrow (audio_nets/res.py:6-123),                           */
/*   KWSModel architectures (audio_nets/kws.py:15-63).                                            */
/* ------------------------------------------------------------------------------------------ */
/* The host describes the topology node by node, as the reference's Python builds its TF graph; every builder returns the
 * node id (>= 0) or a negative tcr_status.  Input id -1 is the network input [batch][c][h*w + 2*TCR_HALO] (planar, the
 * plane at offset TCR_HALO).  Variables live in one trainable arena (all variables whose TF name lacks "BatchNorm" first:
 * the L2-regularised set of factory/audio_nets.py:175-180) and one moving-statistics arena, under the names given here. */
typedef struct tcr_g2d tcr_g2d;
int tcr_g2d_create(const char* scope, int h, int w, int c, tcr_g2d** out);
void tcr_g2d_destroy(tcr_g2d* g);
/* slim.conv2d / tf.nn.conv2d (+ bias, + ReLU): kernel kh x kw, stride, dilation `rate` (audio_nets/res.py:11-16), SAME
 * (valid_padding = 0) or VALID padding; weights HWIO under `weights_name`, bias under `biases_name` (NULL / "": none).
 * A fully connected layer over a flattened [h][w][c] activation is the VALID conv with kh = h, kw = w. */
int tcr_g2d_conv(tcr_g2d* g, int in, int kh, int kw, int cout, int sh, int sw, int dh, int dw, int valid_padding, int relu,
                 const char* weights_name, const char* biases_name);
/* tf.nn.depthwise_conv2d with channel multiplier 1 -- slim.separable_conv2d(num_outputs=None, depth_multiplier=1) -- (+ bias, + ReLU):
 * one kh x kw filter per channel, output channels = input channels C; no other multiplier is offered.  Window, padding and output
 * size are exactly tcr_g2d_conv's (SAME pads with the extra element on the high side; dilation needs stride 1).  Weights
 * [kh][kw][C][1] under `weights_name`, bias [C] under `biases_name` (NULL / "": none); both sit in the decayed arena by the name rule
 * of every other variable.  With in(o, t) = o * stride + t * rate - pad_lo per dimension and positions outside the plane reading 0:
 *   forward            y[n][c][oy][ox]  = act(bias[c] + sum_{i,j} x[n][c][in(oy, i)][in(ox, j)] * W[i][j][c])
 *   data gradient      dx[n][c][iy][ix] += sum_{i,j} dy[n][c][(iy + pt - i*dh) / sh][(ix + pl - j*dw) / sw] * W[i][j][c]   (exact divisions only)
 *   filter gradient    dW[i][j][c]      = sum_{n,oy,ox} x[n][c][in(oy, i)][in(ox, j)] * dy[n][c][oy][ox]
 * Each forward output is one fused-multiply-add chain over the taps in (i, then j) order, so its bits do not depend on how the plane
 * is tiled; the filter gradient is summed per utterance chunk and the chunks in a fixed order (no atomics): repeated runs give the
 * same bits.  Operand pointers need 4-byte alignment only.  Refused at construction (message in tcr_last_error): kh * kw > 1024 taps;
 * min((kh - 1) * dh + 1, h) * w > 4096 floats (the rows one output row reads must fit one staged tile -- the plane's HEIGHT is not
 * limited); a kernel that does not fit the input under VALID padding; dilation together with a stride. */
int tcr_g2d_depthwise_conv(tcr_g2d* g, int in, int kh, int kw, int sh, int sw, int dh, int dw, int valid_padding, int relu,
                           const char* weights_name, const char* biases_name);
/* slim.batch_norm(fused): optional beta (center) / gamma (scale), optional ReLU; variables `<prefix>/gamma|beta|moving_*`. */
int tcr_g2d_batch_norm(tcr_g2d* g, int in, int center, int scale, int relu, float decay, float eps, const char* prefix);
/* slim.avg_pool2d / tf.nn.max_pool; kh <= 0: the window is the whole plane (global pool). */
int tcr_g2d_pool(tcr_g2d* g, int in, int is_max, int kh, int kw, int sh, int sw, int valid_padding);
int tcr_g2d_add(tcr_g2d* g, int a, int b, int relu);                 /* net += layer_in [; relu] */
int tcr_g2d_dropout(tcr_g2d* g, int in, float keep_prob);            /* tf.nn.dropout / slim.dropout; identity in eval mode */
/* SVDF layer of KWSModel --architecture low_latency_svdf (audio_nets/kws.py:490-680, training graph): after the frequency filters (a
 * 1 x F VALID conv) `time_filter` applies one filter of the plane's length per channel (tf.matmul with weights_time [filters, T], :604-612),
 * `group_sum` adds the `rank` filters of a unit, the bias and the ReLU (:613-628). */
int tcr_g2d_time_filter(tcr_g2d* g, int in, const char* weights_name);
int tcr_g2d_group_sum(tcr_g2d* g, int in, int group, int relu, const char* biases_name);
int tcr_g2d_node_shape(const tcr_g2d* g, int node, int* c, int* h, int* w);
/* A node's activation inside the workspace of a forward call at (batch, train): [batch][C][plane_floats], the H*W values of a
 * plane start `halo` floats in.  What the reference exposes as `endpoints` (audio_nets/res.py:66, tc_resnet.py:95). */
int tcr_g2d_node_output(const tcr_g2d* g, int node, int batch, int train, int64_t* offset_floats, int64_t* plane_floats, int* halo);
int tcr_g2d_finalize(tcr_g2d* g, int logits_node);                   /* logits node: [num_classes] x 1 x 1 */
int64_t tcr_g2d_param_floats(const tcr_g2d* g);
int64_t tcr_g2d_decay_floats(const tcr_g2d* g);
int64_t tcr_g2d_stat_floats(const tcr_g2d* g);
int tcr_g2d_num_tensors(const tcr_g2d* g);
int tcr_g2d_num_classes(const tcr_g2d* g);
int tcr_g2d_tensor_info(const tcr_g2d* g, int index, tcr_tensor_info* out);
size_t tcr_g2d_workspace_bytes(const tcr_g2d* g, int batch, int train);
/* front-end output [batch][f][tcr_padded_len(t)] -> the [t x f] single-channel plane these networks read ([N, T, F, 1]) */
int tcr_g2d_input_from_features(const float* feat, int batch, int t, int f, float* plane, void* stream);
/* eval forward + softmax; train forward (batch statistics, dropout keyed by (seed, node, sample), mean cross-entropy:
 * arguments as tcr_net_forward_train); backward of the model loss wrt every trainable (same seed / sample_offset). */
int tcr_g2d_forward_infer(const tcr_g2d* g, const float* params, const float* stats, const float* x, int batch,
                          void* workspace, size_t workspace_bytes, float* logits, float* probs, void* stream);
int tcr_g2d_forward_train(const tcr_g2d* g, const float* params, float* stats, const float* x, const float* labels, int batch,
                          int global_batch, uint64_t seed, int64_t sample_offset, float label_smoothing, void* workspace,
                          size_t workspace_bytes, float* logits, float* probs, float* loss_out, void* stream);
int tcr_g2d_backward(const tcr_g2d* g, const float* params, const float* x, int batch, uint64_t seed, int64_t sample_offset,
                     void* workspace, size_t workspace_bytes, float* grads, void* stream);
/* Cross-replica BN for the graph engine (round 3): the forward / backward stop behind every BN node's statistics (graph order / reverse
 * graph order), the caller all-reduces the 2 x C float64 sums (tcr_g2d_stage_sums) and runs the next stage; stages
 * 0 .. tcr_g2d_num_stages() - 1 (= BN nodes + 1).  One replica: bitwise the unstaged run. */
int tcr_g2d_num_stages(const tcr_g2d* g);
int tcr_g2d_stage_sums(const tcr_g2d* g, int backward, int stage, void* workspace, int batch, double** sums_dev, int64_t* n_doubles);
int tcr_g2d_forward_train_stage(const tcr_g2d* g, const float* params, float* stats, const float* x, const float* labels, int batch,
                                int global_batch, uint64_t seed, int64_t sample_offset, float label_smoothing, void* workspace,
                                size_t workspace_bytes, float* logits, float* probs, float* loss_out, int stage, void* stream);
int tcr_g2d_backward_stage(const tcr_g2d* g, const float* params, const float* x, int batch, int global_batch, uint64_t seed,
                           int64_t sample_offset, void* workspace, size_t workspace_bytes, float* grads, int stage, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Optimiser (helper/trainer.py:171-197) and L2 (factory/audio_nets.py:175-182)                */
/* ------------------------------------------------------------------------------------------ */
/* tf.train.MomentumOptimizer, use_nesterov=False:  g' = g*grad_scale + wd*w (first n_decay floats)
 * a <- mu*a + g' ; w <- w - lr*a. */
int tcr_sgd_momentum_step(float* params, const float* grads, float* momentum, int64_t n, int64_t n_decay,
                          float lr, float mu, float weight_decay, float grad_scale, void* stream);
/* tf.train.AdamOptimizer (beta1 .9, beta2 .999, eps 1e-8 defaults); t = 1-based step. */
int tcr_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t n_decay,
                  float lr, float beta1, float beta2, float eps, int64_t t, float weight_decay,
                  float grad_scale, void* stream);
/* tf.train.RMSPropOptimizer (decay .9, momentum 0, eps 1e-10 defaults; helper/trainer.py:186-188):
 * ms <- decay*ms + (1-decay)*g'^2 ; mom <- momentum*mom + lr*g'/sqrt(ms + eps) ; w <- w - mom.  The `ms` slot starts at one. */
int tcr_rmsprop_step(float* params, const float* grads, float* ms, float* mom, int64_t n, int64_t n_decay,
                     float lr, float decay, float momentum, float eps, float weight_decay, float grad_scale, void* stream);
/* tf.train.ExponentialMovingAverage(decay).apply(variables_to_train) (helper/trainer.py:213-217):
 * shadow <- shadow - (1 - decay) * (shadow - params), over the trainable arena. */
int tcr_ema_step(float* shadow, const float* params, int64_t n, float decay, void* stream);
/* out[0] = weight_decay * sum_{i<n_decay} 0.5*w_i^2 (device float). */
int tcr_l2_loss(const float* params, int64_t n_decay, float weight_decay, float* out, void* stream);
/* Batch SUM of the softmax cross-entropy of logits rows [batch][num_classes] against one-hot (optionally smoothed) labels: the model
 * loss of an evaluation build (tf.losses.softmax_cross_entropy, factory/audio_nets.py:161-173) times the batch. */
int tcr_xent_loss_sum(const float* logits, const float* labels, int batch, int num_classes, float label_smoothing,
                      float* loss_utt, float* loss_sum, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Input stage: PCM decode + crop/pad + time shift + background mix            */
/* ------------------------------------------------------------------------------------------ */
/* Batched device form of contrib_audio.decode_wav(desired_samples) + _shift_audio + _mix_background
 * (datasets/augmentation_factory.py:30-211; mapped per element by AudioDataWrapper._parse_function,
 * datasets/audio_data_wrapper.py:37-58).  The random draws of the reference's graph are inputs:
 *   pcm        int16 pool holding every clip (mono, already at sample_rate);
 *   clip_off   [batch] first sample of each utterance's clip in the pool;
 *   clip_len   [batch] decoded samples of the clip (0 = the empty filename of a "silent" sample); longer clips are
 *              cropped, shorter ones zero-padded to desired_samples (decode_wav).  NULL: every clip has desired_samples;
 *   shift      [batch] time_shift_amount in samples, + delays the audio (zero fill, _shift_audio :104-141); NULL: 0;
 *   background int16 pool of the background-noise recordings; bg_off [batch] first sample of the random crop;
 *   bg_vol     [batch] background_volume (0 = not mixed: not read); NULL: no mixing at all;
 *   out        [batch][desired_samples] float32 = clip(background / 32768 * bg_vol + foreground, -1, 1)  (:92-95).
 * One IEEE multiply and one IEEE add per sample, like tf.multiply / tf.add: results are bit-exact. */
int tcr_augment_fwd(const int16_t* pcm, const int64_t* clip_off, const int32_t* clip_len, const int32_t* shift,
                    const int16_t* background, const int64_t* bg_off, const float* bg_vol, int batch,
                    int desired_samples, float* out, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Streaming detection: S concurrent audio streams, k new frames per stream and step.          */
/* ------------------------------------------------------------------------------------------ */
/* Each stream conceptually carries audio = zeros(n_samples) ++ every sample pushed since its last reset.  A step appends k * hop
 * samples to every stream; afterwards, for every stream:
 *   - its window (the first S * n_coef * (T + 2*TCR_HALO) floats of `state`, planar [S][n_coef][Tp], halo zero) is bitwise
 *     tcr_frontend_fwd (default knobs) of audio[-n_samples:] -- only the k new frames are computed (the window's columns k..T-1
 *     move to 0..T-k-1; the new ones come from frontend_pk3's arithmetic), nothing accumulates;
 *   - logits / probs [S][num_classes] are bitwise tcr_net_forward_frozen of the S windows at batch S with `frozen_ss`;
 *   - the detector (per stream: a ring of the last W = average_steps probability vectors, count = min(steps since reset, W),
 *     prev_label = -1, prev_step, a step counter n):
 *       smoothed = (sum of the ring's vectors, oldest to newest, float32) * (1.0f / count);
 *       count < min_count: top = -1, score = 0, is_new = 0;
 *       else top = argmax(smoothed) (lowest index on ties), score = smoothed[top],
 *            is_new = score > threshold && top != prev_label && (prev_label == -1 || n - prev_step > suppression_steps),
 *            and when is_new: prev_label = top, prev_step = n;
 *       then n += 1.
 * reset (uint8 [S], may be NULL): the marked streams return to the initial state -- audio, window, ring, detector -- BEFORE this
 * step's samples are appended.  Streams are independent.
 * Configurations: the front-end's n_coef x T must be the net's input; 1 <= k <= T; the front-end must be one frontend_pk3_kernel
 * covers (mfcc / log-mel; the float64 deploy path, method 2, and windows pk3 declines are refused: no other kernel gives the
 * offline features bitwise).  State and workspace are caller-owned device memory of the sizes below (0: invalid arguments, see
 * tcr_last_error); tcr_stream_init fills the state (every stream = a silent clip) and must run once before the first step; the
 * state belongs to one (cfg, net, n_streams, k, det) and the same values must be passed to every step.  tcr_stream_scan (below,
 * after tcr_scan) advances the same state by many steps in one call, bitwise these steps. */
typedef struct tcr_detect_cfg {
    int32_t average_steps;      /* W: probability vectors averaged (average_window_ms / step) */
    int32_t min_count;          /* 1..W: no result before this many vectors since the reset */
    int32_t suppression_steps;  /* a new detection needs more than this many steps since the last one (unless the first) */
    float threshold;            /* the smoothed score must exceed it */
} tcr_detect_cfg;

size_t tcr_stream_state_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int n_streams, int k, const tcr_detect_cfg* det);
size_t tcr_stream_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int n_streams, int k);
int tcr_stream_init(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, int n_streams, int k,
                    const tcr_detect_cfg* det, void* state, void* workspace, size_t ws_bytes, void* stream);
/* One step, one host call: stage / shift, front-end (k frames per stream), network, detector.  samples [S][k * hop] float32;
 * smoothed [S][num_classes], top / score / is_new [S]. */
int tcr_stream_step(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                    const float* frozen_ss, int n_streams, int k, const tcr_detect_cfg* det, const float* samples,
                    const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits, float* probs,
                    float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream);

/* Offline scanning: every step of N signals of equal length L (samples [N][L] float32, L a positive multiple of k * hop) in one
 * call.  For signal n and step i = 0 .. L / (k * hop) - 1, logits / probs / smoothed [N][steps][num_classes] and top / score /
 * is_new [N][steps] are bitwise what a fresh stream (tcr_stream_init, then steps without resets) returns from its (i + 1)-th step
 * when fed signal n k * hop samples at a time, with the same cfg, frozen_ss, k and det: the window of step i is frames
 * [(i + 1) k, (i + 1) k + T) of the signal with n_samples zeros in front, and the detector rule is tcr_stream_step's.
 * Configurations: those tcr_stream_* accept (the same refusals, the same messages).  The workspace does not depend on L:
 * tcr_scan_workspace_bytes sizes one for chunks of up to max_windows windows (0: invalid arguments, see tcr_last_error), and
 * tcr_scan runs the largest chunks the bytes passed hold (TCR_ERR_WORKSPACE below one window).  Outputs are caller-owned device
 * memory sized by L; everything is enqueued on `stream`.  Every signal starts from a silent clip: to scan a recording in pieces,
 * or to continue a stream, use tcr_stream_scan, which starts from and updates a stream state. */
size_t tcr_scan_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int k, int max_windows);
int tcr_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params, const float* frozen_ss,
             int n_signals, int64_t n_samples, int k, const tcr_detect_cfg* det, const float* samples /* [N][L] */,
             void* workspace, size_t ws_bytes, float* logits, float* probs, float* smoothed /* [N][steps][C] */,
             int32_t* top, float* score, int32_t* is_new /* [N][steps] */, void* stream);

/* m = n_samples / (k * hop) steps of tcr_stream_step for every stream, in one call, at tcr_scan's throughput.  samples [S][n_samples]
 * float32 (n_samples a positive multiple of k * hop); reset [S] uint8 or NULL, applied before the first step only (as
 * tcr_stream_step applies it); state: a tcr_stream_state_bytes region from tcr_stream_init / _step / _scan with the same (cfg, net,
 * S, k, det).  logits / probs / smoothed [S][m][C], top / score / is_new [S][m]: step i of stream s is bitwise what the (i + 1)-th
 * of m tcr_stream_step calls returns; afterwards `state` is what those m calls leave: the window, the tail, the five detector
 * integers and the ring slots of the last min(count, W) vectors bitwise (the other ring slots are never read).  workspace:
 * tcr_scan_workspace_bytes(cfg, net, k, max_windows) bytes (TCR_ERR_WORKSPACE below one window).  Precondition: every stream's
 * step counter stays below 2^31 (n + m < 2^31 steps since its reset).  Configurations and refusals: tcr_stream_step's.  Calls of
 * tcr_stream_step and tcr_stream_scan may be mixed on one state in any order; everything is enqueued on `stream`. */
int tcr_stream_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                    const float* frozen_ss, int n_streams, int64_t n_samples, int k, const tcr_detect_cfg* det,
                    const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes,
                    float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream);

/* The detection entries above for every model family: each _m twin takes a model reference in place of (net, params, frozen_ss)
 * and is otherwise the entry it is named after (arguments, layouts, refusals, bitwise contracts).  The window stays the planar
 * front-end output [n_coef][T + 2*TCR_HALO] in the state whatever the family; the network call is
 *   TCR_FAMILY_TCRESNET  tcr_net_forward_frozen(handle, params, aux = the folded table of tcr_net_fold_bn, windows);
 *   TCR_FAMILY_DSCNN     tcr_dscnn_forward_infer(handle, params, aux = the moving statistics, windows): w_in = n_coef, h_in = T;
 *   TCR_FAMILY_G2D       tcr_g2d_forward_infer(handle, params, aux = the moving statistics, planes): a finalized graph of a
 *                        single-channel h = T frames x w = n_coef input; the windows are laid out as tcr_g2d_input_from_features
 *                        lays them out (a pure copy).
 * So logits / probs of a step are bitwise that call on the S windows at batch S (DS-CNN: S <= 65535 * 16, the batch range of one
 * kernel path; tcr_scan_m keeps its launches in it).  DS-CNN and 2-D graphs fold their BN inside every call: in-place updates to
 * params / aux are seen by the next one.  A state belongs to one (cfg, model, n_streams, k, det), as above.  Refused, with a
 * message: an unknown family, a null handle, a graph that is not finalized, a front-end that does not yield the input shape,
 * more than 256 classes.  The entries without _m are these with a TCR_FAMILY_TCRESNET reference. */
#define TCR_FAMILY_TCRESNET 0
#define TCR_FAMILY_DSCNN 1
#define TCR_FAMILY_G2D 2
typedef struct tcr_model_ref {
    int family;                 /* TCR_FAMILY_* */
    const void* handle;         /* tcr_net* / tcr_dscnn* / finalized tcr_g2d* */
    const float* params;        /* the trainable arena */
    const float* aux;           /* TC-ResNet: frozen_ss (tcr_net_fold_bn); DS-CNN, 2-D graph: the moving-statistics arena */
} tcr_model_ref;

size_t tcr_stream_state_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k, const tcr_detect_cfg* det);
size_t tcr_stream_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k);
int tcr_stream_init_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                      const tcr_detect_cfg* det, void* state, void* workspace, size_t ws_bytes, void* stream);
int tcr_stream_step_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                      const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                      size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                      void* stream);
size_t tcr_scan_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows);
int tcr_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals, int64_t n_samples, int k,
               const tcr_detect_cfg* det, const float* samples, void* workspace, size_t ws_bytes, float* logits, float* probs,
               float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream);
int tcr_stream_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int64_t n_samples,
                      int k, const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                      size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                      void* stream);

/* Detection sweep: tcr_stream_step's suppression rule for T thresholds at once, with the detections scored against labelled events.
 * top int32 / score float32 [N][steps] are what tcr_scan writes (or streaming steps stacked over steps).  For every signal n and
 * threshold t, starting from prev_label = -1, prev_step = 0, the steps i = 0 .. valid_steps[n] - 1 are walked in order:
 *     is_new = top >= 0 && score > thresholds[t] && top != prev_label && (prev_label == -1 || i - prev_step > suppression_steps),
 *     and when is_new: prev_label = top, prev_step = i.
 * So at thresholds[t] the steps that fire are exactly those a tcr_scan with det->threshold = thresholds[t] (and the same
 * suppression_steps) marks in is_new.  valid_steps [N] (NULL: all steps) ends each signal's walk early (clamped to 0..steps); the
 * rule is causal, so this is the walk of the signal cut there.  Steps whose top is outside 0 .. num_classes - 1 never fire.
 * Events, per signal sorted by step: CSR event_offsets [N + 1] into event_first / event_last (int64, an inclusive step range) and
 * event_label (int32).  Precondition: within a signal, event_first[j + 1] > event_last[j] (disjoint, in order); when it is broken
 * the counts are unspecified (the call stays memory-safe).  A detection at step i with label c is a hit when an event j with
 * first <= i <= last has label c and no earlier detection hit j, a duplicate when one did; every other detection is a false accept
 * (one inside another label's event too).  Events labelled outside 0 .. num_classes - 1 are never hit.
 * Outputs, caller-owned device memory: detections / hits / duplicates int32 [N][T][num_classes] (per detection label); false
 * accepts = detections - hits - duplicates, misses = events - hits.  event_offsets NULL: no events (hits and duplicates may then
 * be NULL; when given they are zeroed).  fired uint8 [T][N][steps] (NULL: not written) is 1 at the steps that fire, 0 elsewhere.
 * Every pointer is device memory; everything is enqueued on `stream`.  Refused (TCR_ERR_ARG, tcr_last_error): null top / score /
 * thresholds / detections, events without their arrays or hits / duplicates, N, T, steps or num_classes <= 0, num_classes > 256,
 * suppression_steps < 0, N x steps or N x T x num_classes >= 2^31. */
int tcr_detect_sweep(int n_signals, int64_t steps, int num_classes, const int32_t* top, const float* score,
                     const int64_t* valid_steps, int32_t suppression_steps, int n_thresholds, const float* thresholds,
                     const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last,
                     const int32_t* event_label, int32_t* detections, int32_t* hits, int32_t* duplicates,
                     uint8_t* fired, void* stream);

/* Ragged scanning: tcr_scan_m over N signals of different lengths in one call, packed one after the other.  Signal n is
 * samples[sample_offsets[n] .. sample_offsets[n + 1]) (float32, device); sample_offsets is a HOST array [N + 1] that starts at 0
 * and does not decrease, every length a multiple of k * hop (0 allowed: a signal without steps has no rows).  Step i of signal n is
 * packed row sample_offsets[n] / (k * hop) + i of logits / probs / smoothed [total_steps][num_classes] and top / score / is_new
 * [total_steps] (all positions int64).  Contract: signal n's rows are bitwise what tcr_scan_m returns for that signal alone
 * (n_signals = 1; the same cfg, model, k and det; a fresh start from one clip of silence) -- whatever the workspace's size, the
 * group size the call picks and the other signals of the call.  The smoothing of a signal's first steps and its suppression walk
 * never read another signal's rows.  The model is a tcr_model_ref of any family (TC-ResNet: TCR_FAMILY_TCRESNET with aux =
 * frozen_ss), so there is one entry.
 * Workspace: tcr_scan_ragged_workspace_bytes = the offset tables of max_signals signals (2 (max_signals + 1) int64, rounded up to
 * 256 bytes: step and group offsets, uploaded by the call) + tcr_scan_workspace_bytes_m(cfg, model, k, max_windows).  The call
 * places the tables of its n_signals at the front and runs the largest chunks the rest holds, so max_signals and max_windows only
 * size the bytes.  The tables are copied from the host on `stream` and the call waits for that copy before it launches (the stream's
 * earlier work included): sample_offsets may be freed when it returns; the call cannot be captured into a graph.  Everything else is
 * enqueued on `stream`.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): null arguments, n_signals <= 0, more signals than the workspace's
 * tables hold, sample_offsets[0] != 0, decreasing offsets, a length that is not a multiple of k * hop, total_steps == 0,
 * total_steps x num_classes >= 2^31, and everything tcr_scan_m refuses, with its messages.  TCR_ERR_WORKSPACE when the bytes behind
 * the tables are below one window. */
size_t tcr_scan_ragged_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows,
                                       int max_signals);
int tcr_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals,
                    const int64_t* sample_offsets /* HOST [N + 1] */, int k, const tcr_detect_cfg* det,
                    const float* samples /* device, packed */, void* workspace, size_t ws_bytes, float* logits, float* probs,
                    float* smoothed /* [total_steps][C] */, int32_t* top, float* score, int32_t* is_new /* [total_steps] */,
                    void* stream);

/* Ragged many-step pushes: tcr_stream_scan_m with a step count of its own for every stream.  Stream s advances by
 * m_s = (sample_offsets[s + 1] - sample_offsets[s]) / (k * hop) >= 0 steps; samples, sample_offsets (HOST [S + 1], from 0, not
 * decreasing, every length a multiple of k * hop) and the six outputs are packed as tcr_scan_ragged packs them: step i of stream s
 * is row sample_offsets[s] / (k * hop) + i.  reset [S] uint8 or NULL; state: the region tcr_stream_init_m made for (cfg, model, S, k,
 * det); workspace: tcr_scan_ragged_workspace_bytes(cfg, model, k, max_windows, max_signals >= n_streams) bytes.
 * Contract: stream s's rows, and the state it is left in (window, tail, the five integers and the ring slots of the last
 * min(count, W) vectors), are bitwise what m_s calls of tcr_stream_step_m produce for that stream, the reset applied before the
 * first of them; a call with the same m_s for every stream is bitwise tcr_stream_scan_m.  A stream with m_s == 0 is untouched: its
 * window, tail, ring and integers are byte for byte what they were, and reset[s] != 0 is IGNORED for it (no step, no reset: pass
 * the flag again with the call that brings the stream's next step).  Calls of tcr_stream_step, tcr_stream_scan and
 * tcr_stream_scan_ragged may be mixed on one state in any order.  The offset tables are uploaded as tcr_scan_ragged uploads them
 * (host copy on `stream`, then a wait), so the call cannot be captured into a graph; everything else is enqueued on `stream`.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched and the state is untouched): everything tcr_scan_ragged refuses except
 * that a stream without steps is allowed, everything tcr_stream_scan_m refuses, a call without any step (total_steps == 0), and
 * more streams than the workspace's tables hold.  TCR_ERR_WORKSPACE when the bytes behind the tables are below one window.
 * tcr_stream_scan_ragged is the entry with a TCR_FAMILY_TCRESNET reference built from (net, params, frozen_ss). */
int tcr_stream_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                           const float* frozen_ss, int n_streams, const int64_t* sample_offsets /* HOST [S + 1] */, int k,
                           const tcr_detect_cfg* det, const float* samples /* device, packed */, const uint8_t* reset, void* state,
                           void* workspace, size_t ws_bytes, float* logits, float* probs, float* smoothed /* [total_steps][C] */,
                           int32_t* top, float* score, int32_t* is_new /* [total_steps] */, void* stream);
int tcr_stream_scan_ragged_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams,
                             const int64_t* sample_offsets /* HOST [S + 1] */, int k, const tcr_detect_cfg* det,
                             const float* samples /* device, packed */, const uint8_t* reset, void* state, void* workspace,
                             size_t ws_bytes, float* logits, float* probs, float* smoothed /* [total_steps][C] */, int32_t* top,
                             float* score, int32_t* is_new /* [total_steps] */, void* stream);

/* tcr_detect_sweep over a ragged scan: top / score are packed [total_steps] and signal n's steps are rows step_offsets[n] ..
 * step_offsets[n + 1] - 1 (DEVICE int64 [N + 1], from 0, non-decreasing: a precondition, the host does not read it).  The rule is
 * tcr_detect_sweep's, walked over each signal's own rows from prev_label = -1; events stay CSR per signal, in steps relative to the
 * signal's first step.  For every n and t the counts equal tcr_detect_sweep on the zero-padded dense layout with valid_steps[n] =
 * the signal's steps.  fired uint8 [T][total_steps] (NULL: not written) is zeroed and set by the kernel.  Refusals: those of
 * tcr_detect_sweep that do not need the step counts, and a null step_offsets. */
int tcr_detect_sweep_ragged(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int num_classes, const int32_t* top,
                            const float* score, int32_t suppression_steps, int n_thresholds, const float* thresholds,
                            const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last,
                            const int32_t* event_label, int32_t* detections, int32_t* hits, int32_t* duplicates,
                            uint8_t* fired /* [T][total_steps] or NULL */, void* stream);

/* Detector tuning from one scan.  logits / probs of a scan do not depend on det, so the detector tail can be run again on the probs a
 * scan wrote, with any other det, without the front-end and the network.
 *
 * tcr_detect_redetect: probs [N][steps][num_classes] (what tcr_scan / tcr_scan_m wrote, with any det) -> smoothed [N][steps][C] (NULL:
 * not written), top / score / is_new [N][steps]: for every signal bitwise what tcr_scan_m writes for it with this det (the rule of
 * tcr_stream_step above, from a fresh detector).  tcr_detect_redetect_ragged: the same over packed probs [total_steps][C] with signal
 * n's steps in rows step_offsets[n] .. step_offsets[n + 1] - 1 (DEVICE int64 [N + 1], from 0, non-decreasing, step_offsets[N] ==
 * total_steps: preconditions, the host does not read the table): bitwise tcr_scan_ragged's outputs; a signal's first steps never read
 * the signal before it.  Both only enqueue kernels on `stream` -- no copy, no wait -- so, unlike tcr_scan_ragged, they can be captured
 * into a graph.  Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): null probs / det / top / score / is_new (ragged:
 * step_offsets), N, steps (ragged: total_steps) or num_classes <= 0, num_classes > 256, average_steps < 1, min_count outside
 * 1..average_steps, suppression_steps < 0, N x steps x num_classes >= 2^31. */
int tcr_detect_redetect(int n_signals, int64_t steps, int num_classes, const float* probs /* [N][steps][C] */,
                        const tcr_detect_cfg* det, float* smoothed /* [N][steps][C] or NULL */, int32_t* top, float* score,
                        int32_t* is_new, void* stream);
int tcr_detect_redetect_ragged(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int num_classes,
                               const float* probs /* packed [total_steps][C] */, const tcr_detect_cfg* det, float* smoothed,
                               int32_t* top, float* score, int32_t* is_new, void* stream);

/* The detector grid: J points (average_steps, min_count, suppression_steps) x T thresholds from one scan's probs, in one call.  For
 * point j the slice [j] of detections / hits / duplicates int32 [J][N][T][num_classes] equals tcr_detect_sweep (step_offsets != NULL:
 * tcr_detect_sweep_ragged) over the top / score of a scan of the same audio with det = {points[j], any threshold} -- the same
 * thresholds, events (in steps: they do not depend on the point) and valid_steps.  Dense: probs [N][steps][C], total_steps = N x
 * steps, valid_steps [N] or NULL.  Ragged: probs packed [total_steps][C], step_offsets a DEVICE table as above, `steps` ignored,
 * valid_steps NULL.  `points` is a HOST array, read before the call returns; every other pointer is device memory.  There is no
 * `fired` output (J x T x steps bytes): the detections of one point are tcr_detect_redetect plus tcr_detect_sweep.
 * How: the points are reduced to their distinct (average_steps, min_count) pairs.  One kernel stages tiles of TCR_GRID_TILE steps (and
 * the average_steps - 1 rows in front of them) in LDS and writes top / score for every pair into workspace rows, smoothing once per
 * distinct average_steps; then tcr_detect_sweep's kernel runs once per point over its pair's rows.  The staged tile holds
 * (TCR_GRID_TILE + W - 1) x num_classes floats in 63 KB of LDS, so it takes average_steps up to  W_max = 16128 / num_classes - 255
 * (num_classes 12: 1089; 3: 5121; 36: 193; none from 63 classes on); pairs above W_max are smoothed by tcr_detect_redetect's kernel,
 * one launch each, into the same rows (the same results, each row read average_steps times from memory instead).
 * Workspace: tcr_detect_grid_workspace_bytes(total_steps, n_points) holds the rows of n_points pairs (0: invalid arguments), which
 * is enough for any grid of n_points points; with fewer bytes the pairs run in batches that fit, the counts are the same, and below
 * tcr_detect_grid_workspace_bytes(total_steps, 1) the call returns TCR_ERR_WORKSPACE.  Everything is enqueued on `stream`.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): everything tcr_detect_sweep refuses (ragged: tcr_detect_sweep_ragged),
 * everything tcr_detect_redetect refuses, for every point; null points or workspace, n_points <= 0, J x N x T x num_classes >= 2^31,
 * valid_steps together with step_offsets, and (dense) total_steps != N x steps. */
#define TCR_GRID_TILE 256
typedef struct tcr_detect_point {
    int32_t average_steps, min_count, suppression_steps;
} tcr_detect_point;
size_t tcr_detect_grid_workspace_bytes(int64_t total_steps, int n_points);
int tcr_detect_grid(int n_signals, int64_t steps /* dense; ignored when step_offsets != NULL */,
                    const int64_t* step_offsets /* DEVICE [N + 1] or NULL */, int64_t total_steps, int num_classes,
                    const float* probs, const int64_t* valid_steps /* dense only, or NULL */, int n_points,
                    const tcr_detect_point* points /* HOST */, int n_thresholds, const float* thresholds,
                    const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last,
                    const int32_t* event_label, int32_t* detections, int32_t* hits,
                    int32_t* duplicates /* [J][N][T][C] */, void* workspace, size_t ws_bytes, void* stream);

/* Sparse scans: tcr_scan_ragged's logits / probs for a chosen subset of its packed steps, at the cost of that subset -- the second
 * stage of a cascade, or a new checkpoint rescored only around labelled events.  cfg, plan_dev, model, n_signals, sample_offsets (HOST
 * [N + 1]), k and samples are tcr_scan_ragged's; selected is a HOST array of n_selected packed step indices (row numbers of
 * tcr_scan_ragged's outputs), strictly increasing.  Contract: row b of logits / probs [n_selected][num_classes] (compact, in
 * `selected`'s order) is bitwise row selected[b] of tcr_scan_ragged's logits / probs for the same arguments -- a fresh signal with one
 * clip of silence in front, for every model family, whatever max_windows, the group size the call picks and the other selected
 * steps.  No detector runs: there is no det and no smoothed / top / score / is_new (merge the rows into a full scan's probs and run
 * tcr_detect_redetect_ragged).
 * Cost: the steps are cut into groups of G steps exactly as tcr_scan_ragged cuts them, but only the groups that hold a selected step
 * are staged and run through the front-end (a group is one row of G k + T - k frames; G: the fewest frames summed over those groups),
 * and the network runs at the batch of the selected steps only and writes the caller's rows itself.
 * Workspace: tcr_scan_steps_workspace_bytes = the tables of max_signals signals and max_selected steps ((max_signals + 1 + 3
 * max_selected) int64, rounded up to 256 bytes: the step offsets, selected, every selected step's front-end row and every row's
 * first step) + tcr_scan_workspace_bytes_m(cfg, model, k, max_windows); it does not depend on the signals' length.  The host builds
 * the tables, copies them on `stream` and waits for that copy before it launches, as tcr_scan_ragged does: sample_offsets and selected
 * may be freed when the call returns, and the call cannot be captured into a graph.  Everything else is enqueued on `stream`.
 * n_selected == 0 returns TCR_OK and launches nothing (samples / logits / probs may then be NULL).
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): everything tcr_scan_ragged refuses (except what concerns det and its
 * four detector outputs), n_selected < 0, more signals and selected steps than the workspace's tables hold, null selected with
 * n_selected > 0, a selected step outside 0 .. total_steps - 1 or not above the one before it.  TCR_ERR_WORKSPACE when the bytes behind
 * the tables are below one window.
 * tcr_scan_steps_plan: what a call with these arguments and ws_bytes would run, from the host alone (the same refusals; nothing is
 * launched): plan[0] = G, plan[1] = the front-end rows staged, plan[2] = the frames of a row, plan[3] = the rows of a chunk (all 0
 * when n_selected == 0). */
size_t tcr_scan_steps_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows,
                                      int max_signals, int64_t max_selected);
int tcr_scan_steps(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals,
                   const int64_t* sample_offsets /* HOST [N + 1] */, int k, const int64_t* selected /* HOST [n_selected] */,
                   int64_t n_selected, const float* samples /* device, packed */, void* workspace, size_t ws_bytes,
                   float* logits, float* probs /* [n_selected][C] */, void* stream);
int tcr_scan_steps_plan(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_signals,
                        const int64_t* sample_offsets /* HOST [N + 1] */, int k, const int64_t* selected /* HOST */,
                        int64_t n_selected, size_t ws_bytes, int64_t* plan /* HOST [4] */);

/* Step selection: which steps of a scan a second stage should look at.  values [total_steps][num_classes] are a ragged scan's probs
 * or smoothed (a dense scan's with step_offsets[n] = n x steps), step_offsets a DEVICE table as tcr_detect_redetect_ragged takes it
 * (from 0, non-decreasing, step_offsets[N] == total_steps: preconditions).  Step p is FLAGGED when some class c with class_mask[c] !=
 * 0 has values[p][c] >= enter (a float32 compare: a NaN value never flags), and SELECTED when a flagged step p' of the same signal
 * has  p - pad_after <= p' <= p + pad_before  -- pad_before steps in front of every flag and pad_after behind it, never across a
 * signal's ends.  selected (DEVICE int64, room for total_steps) receives the selected packed steps in increasing order, n_selected
 * (DEVICE [1]) their number, mask (DEVICE [total_steps] or NULL) 1 at the selected steps and 0 elsewhere.  enter = -inf selects every
 * step (whose masked values are not all NaN), +inf none: n_selected = 0 is a valid result.  No floating-point arithmetic: the output
 * is exact.  Prefix sums over the packed steps in kernels of their own (no workgroup waits for another); the cost is linear in
 * total_steps and independent of the pads.  Everything is enqueued on `stream` -- no copy, no wait.
 * Workspace: tcr_scan_select_workspace_bytes(total_steps) (0: total_steps outside 1 .. 2^31 - 1); TCR_ERR_WORKSPACE below it.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): null step_offsets / values / class_mask / workspace / selected /
 * n_selected, N or total_steps <= 0, num_classes outside 1 .. 256, total_steps x num_classes >= 2^31, NaN enter, a negative pad. */
size_t tcr_scan_select_workspace_bytes(int64_t total_steps);
int tcr_scan_select(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int num_classes,
                    const float* values /* [total_steps][C] */, const uint8_t* class_mask /* DEVICE [C] */, float enter,
                    int pad_before, int pad_after, void* workspace, size_t ws_bytes, int64_t* selected /* DEVICE */,
                    int64_t* n_selected /* DEVICE [1] */, uint8_t* mask /* [total_steps] or NULL */, void* stream);

/* Streaming cascades: the causal cascade -- tcr_scan_select at pad_before = 0, a second model on the selected steps, its detector
 * over the merged posteriors -- carried from step to step over S concurrent streams.  A stream cannot be rescored before its flag,
 * so pad_before is 0 by definition: at a flag the detector's average mixes first-stage rows from before it with second-stage rows
 * from it on.  Per step: the first detector's tcr_stream_step_m (unchanged, its own state), tcr_stream_select over its probs or
 * smoothed, a read-back of n_selected by the host (one small copy and wait per step: a cascade step cannot be captured into a
 * graph), then tcr_stream_step_selected_m of the second detector with the first one's logits / probs as fill rows.  The steps
 * stacked over time are bitwise the cascade scan of the whole signals at pad_before = 0.
 *
 * tcr_stream_select: values [S][num_classes] are the first stage's probs or smoothed of this step.  Stream s is FLAGGED when some
 * class c with class_mask[c] != 0 has values[s][c] >= enter (a float32 compare: a NaN never flags), and SELECTED when it was flagged
 * at this step or at one of the pad_after steps before it since its last reset.  The carried state is since [S] int32 (DEVICE): the
 * steps since the stream's last flag, saturating, INT32_MAX = never; tcr_stream_select_init sets every entry to never, and reset [S]
 * uint8 (or NULL) sets a stream's entry to never BEFORE the step, as tcr_stream_step applies resets.  selected (DEVICE int64, room
 * for S) receives the selected stream indices in increasing order, n_selected (DEVICE [1]) their number, mask (DEVICE [S] or NULL) 1
 * at the selected streams and 0 elsewhere.  enter = -inf selects every stream whose masked values are not all NaN, +inf none.  No
 * floating-point arithmetic beyond the compare; the order comes from prefix sums in kernels of their own (no atomics, no workgroup
 * waits for another).  Everything is enqueued on `stream` -- no copy, no wait.
 * Workspace: tcr_stream_select_workspace_bytes(S) (0: S <= 0); TCR_ERR_WORKSPACE below it.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): null values / class_mask / since / workspace / selected / n_selected,
 * S <= 0, num_classes outside 1 .. 256, NaN enter, a negative pad_after.
 *
 * tcr_stream_step_selected_m: a step of tcr_stream_step_m (the same arguments up to ws_bytes, the same outputs) on an ordinary
 * tcr_stream_init_m state, in which the network runs only on the n_selected (HOST) streams of selected (DEVICE int64, strictly
 * increasing, in 0 .. S - 1: preconditions), at batch n_selected, on their windows gathered into the workspace.  For any selection
 * the stage / shift and the front-end run for all S streams, so the window and the tail of every stream are bitwise what
 * tcr_stream_step_m leaves; a selected stream's logits / probs row is bitwise that step's row (a window's result does not depend on
 * its batch); every other stream's row is its row of fill_logits / fill_probs [S][num_classes], bit for bit; and the detector
 * (tcr_stream_step's rule, the ring and the five integers of this state) runs over the merged probs of all S streams.  With all S
 * streams selected the call is bitwise tcr_stream_step_m, for the six outputs and every byte of `state` (the fill rows may then be
 * NULL); with n_selected == 0 no gather and no network kernel is launched.  Calls of tcr_stream_step_m, tcr_stream_scan_m and
 * tcr_stream_step_selected_m may be mixed on one state in any order.  Fill rows that alias the outputs are undefined.
 * Workspace: tcr_stream_selected_workspace_bytes_m (the staging rows, the gathered windows, the compact rows and the network at
 * batch S; 0: invalid arguments); TCR_ERR_WORKSPACE below it.  Everything is enqueued on `stream`.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): everything tcr_stream_step_m refuses, n_selected outside 0 .. S, null
 * selected with n_selected > 0, null fill rows with n_selected < S. */
int tcr_stream_select_init(int n_streams, int32_t* since /* DEVICE [S] */, void* stream);
size_t tcr_stream_select_workspace_bytes(int n_streams);
int tcr_stream_select(int n_streams, int num_classes, const float* values /* [S][C] */, const uint8_t* class_mask /* DEVICE [C] */,
                      float enter, int pad_after, const uint8_t* reset /* [S] or NULL */, int32_t* since /* [S] */, void* workspace,
                      size_t ws_bytes, int64_t* selected /* DEVICE [S] */, int64_t* n_selected /* DEVICE [1] */,
                      uint8_t* mask /* [S] or NULL */, void* stream);
size_t tcr_stream_selected_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k);
int tcr_stream_step_selected_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                               const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                               size_t ws_bytes, const int64_t* selected /* DEVICE */, int64_t n_selected /* HOST */,
                               const float* fill_logits, const float* fill_probs /* [S][C]; NULL allowed when n_selected == S */,
                               float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                               void* stream);

/* Hard-example mining: the windows a scan got wrong, the best of them, and their audio.  All layouts are the ragged ones: step_offsets
 * is a DEVICE table as tcr_detect_redetect_ragged takes it (a dense scan: step_offsets[n] = n x steps); every pointer is device memory
 * unless marked HOST; everything is enqueued on `stream` -- no copy, no wait -- and every result is deterministic: the tables are
 * written by prefix sums in kernels of their own (no workgroup waits for another, no position comes from an atomic).
 * Workspace of the first three: tcr_mine_workspace_bytes(n_items, ranked) with n_items = total_steps (tcr_mine_detections),
 * total_steps x num_classes (tcr_mine_peaks), both with ranked = 0 (a byte per item and the tiles' sums), or n_cand with ranked = 1
 * (tcr_mine_select: four more bytes per candidate, the ranks of the ties); 0 when n_items is outside 1 .. 2^31 - 1;
 * TCR_ERR_WORKSPACE below it.
 *
 * tcr_mine_detections: a scan's detections classified against events.  top / score / is_new [total_steps] are a scan's or a
 * redetect's; the events are tcr_detect_sweep_ragged's CSR (event_offsets int32 [N + 1], inclusive step ranges relative to the
 * signal's first step, sorted and disjoint within a signal: preconditions) and n_events their number, event_offsets[N].  A CANDIDATE
 * is a step with is_new != 0 and 0 <= top < num_classes.  The candidates are written in increasing packed step: cand_step int64,
 * cand_label int32 (top), cand_value float32 (score), cand_kind uint8 (0 false accept, 1 hit, 2 duplicate), cand_event int32 (the CSR
 * index of the event whose range covers the step, whatever its label; -1: none), each with room for total_steps; n_cand (int64 [1])
 * their number.  event_hit int64 [n_events]: the packed step of the detection that hit the event, -1 for a miss.  The rule is
 * tcr_detect_sweep's: a detection is a hit when an event of its label covers it and no earlier detection hit that event, a
 * duplicate when one did, a false accept otherwise -- evaluated without the walk: the hit of event e is the first candidate in e's
 * range whose label is e's.  Per signal and label the kinds' counts equal tcr_detect_sweep_ragged's detections - hits - duplicates,
 * hits and duplicates at the threshold that produced is_new.  event_offsets NULL: every candidate is kind 0 with cand_event -1 and
 * event_hit is not written.  No floating-point arithmetic.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): a null step_offsets / top / score / is_new / workspace / candidate table
 * / n_cand, N or total_steps <= 0, num_classes outside 1 .. 256, total_steps x num_classes >= 2^31, event_offsets without event_first
 * / event_last / event_label, n_events < 0, n_events > 0 with a null event_hit. */
size_t tcr_mine_workspace_bytes(int64_t n_items, int ranked);
int tcr_mine_detections(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int num_classes,
                        const int32_t* top, const float* score, const int32_t* is_new, const int32_t* event_offsets /* or NULL */,
                        const int64_t* event_first, const int64_t* event_last, const int32_t* event_label, int n_events,
                        void* workspace, size_t ws_bytes, int64_t* cand_step, int32_t* cand_label, float* cand_value,
                        uint8_t* cand_kind, int32_t* cand_event, int64_t* n_cand /* DEVICE [1] */,
                        int64_t* event_hit /* [n_events] */, void* stream);

/* tcr_mine_peaks: near misses, independent of any threshold.  values [total_steps][num_classes] are a scan's probs or smoothed.
 * The pair (p, c) with class_mask[c] != 0 is a candidate when  values[p][c] >= floor  (float32 compares: a NaN never is), p lies in no
 * exclusion range of its signal (exclude_offsets int32 [N + 1] / exclude_first / exclude_last int64: CSR per signal of inclusive step
 * ranges relative to the signal's first step, sorted and disjoint, whatever label; NULL: none),  values[p][c] > values[q][c]  for
 * every q in [p - R, p) and  values[p][c] >= values[q][c]  for every q in (p, p + R], q over the steps of p's own signal only and NaN
 * neighbours ignored: on a plateau the lowest step wins.  The candidates go to cand_step / cand_label / cand_value in (packed step,
 * class) order, the first `capacity` of them; n_cand is their true number whatever the capacity, so a caller can retry with room.
 * How: a workgroup stages a tile of TCR_MINE_TILE steps and R steps on each side in LDS and takes every window's maximum from
 * running maxima over blocks of R steps, at a cost per element that does not depend on R.  The staged steps take 8 bytes per class
 * of a chunk and 4 more in 63 KB of LDS, the classes going through in chunks when they do not fit at once, so the radius is bounded
 * by one class a chunk:  R <= TCR_MINE_RADIUS_MAX = (64512 / 12 - TCR_MINE_TILE) / 2 = 2560  whatever num_classes (all 12 classes at
 * once up to R = 194).
 * Refused (TCR_ERR_ARG): a null step_offsets / values / class_mask / workspace / n_cand, N or total_steps <= 0, num_classes outside
 * 1 .. 256, total_steps x num_classes >= 2^31, a NaN floor, radius outside 1 .. TCR_MINE_RADIUS_MAX, capacity < 0, capacity > 0 with a
 * null table, exclude_offsets without exclude_first / exclude_last. */
#define TCR_MINE_TILE 256
#define TCR_MINE_RADIUS_MAX 2560
int tcr_mine_peaks(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int num_classes,
                   const float* values /* [total_steps][C] */, const uint8_t* class_mask /* [C] */, float floor, int radius,
                   const int32_t* exclude_offsets /* [N + 1] or NULL */, const int64_t* exclude_first, const int64_t* exclude_last,
                   void* workspace, size_t ws_bytes, int64_t capacity, int64_t* cand_step, int32_t* cand_label, float* cand_value,
                   int64_t* n_cand /* DEVICE [1] */, void* stream);

/* tcr_mine_select: the k best of n_cand candidates, exact.  A candidate is eligible when cand_kind is NULL or bit cand_kind[j] of
 * kind_mask is set.  Order: the larger cand_value first (a float32 compare, -0 equal to +0; NaNs by their bit image, positive ones
 * above +inf, negative ones below -inf), then the lower index.  picked (int64, room for min(k, n_cand)) receives the indices of the
 * first min(k, eligible) candidates of that order, in INCREASING index order; n_picked (int64 [1]) their number.  A radix select
 * over the order-preserving integer image of the values (four histogram passes find the k-th key), then one compaction of
 * everything above that key and the lowest-index ties at it: no sort, no floating-point arithmetic.  k == 0, n_cand == 0 or nothing
 * eligible: n_picked = 0 (with k == 0 or n_cand == 0 only n_picked is touched, and value / workspace / picked may be NULL).
 * Refused (TCR_ERR_ARG): a null n_picked, n_cand outside 0 .. 2^31 - 1, k < 0, a null cand_value / workspace / picked. */
int tcr_mine_select(int64_t n_cand, const float* cand_value, const uint8_t* cand_kind /* [n_cand] or NULL */, uint32_t kind_mask,
                    int64_t k, void* workspace, size_t ws_bytes, int64_t* picked, int64_t* n_picked /* DEVICE [1] */, void* stream);

/* tcr_mine_gather: the clips.  samples: packed float32, signal n's samples at sample_offsets[n] .. sample_offsets[n + 1] - 1 (DEVICE
 * int64 [N + 1]).  Clip i is n_samples samples of signal clip_signal[i] (int32 [n_clips]) from its sample clip_first[i] (int64,
 * relative to the signal's start; it may be negative or run past the signal's end).  out float32 [n_clips][n_samples] (or NULL):
 * bitwise the signal's samples, zeros outside the signal -- a neighbouring signal is never read; a clip_signal outside 0 .. N - 1
 * gives a clip of zeros.  out_pcm int16 [n_clips][n_samples] (or NULL):  clamp(rint(x * 32768), -32768, 32767)  with ties to even and
 * NaN -> 0, which inverts the int16 decode v / 32768 exactly.  16-byte stores (int16: 8-byte) at the row's aligned elements, fed by
 * aligned 16-byte loads whatever clip_first; single elements at a row's unaligned ends and next to a signal's ends.  n_clips == 0: a
 * successful no-op.
 * Refused (TCR_ERR_ARG): out and out_pcm both NULL, N or n_samples <= 0, n_clips < 0, a null sample_offsets / samples / clip_signal /
 * clip_first, more than 2^31 workgroups' worth of clips. */
int tcr_mine_gather(int n_signals, const int64_t* sample_offsets /* DEVICE [N + 1] */, const float* samples, int64_t n_clips,
                    const int32_t* clip_signal, const int64_t* clip_first, int n_samples, float* out /* or NULL */,
                    int16_t* out_pcm /* or NULL */, void* stream);

/* Composing labelled test recordings: dataset clips pasted at known times onto looping background noise, written straight into the
 * packed layout tcr_scan_ragged and tcr_mine_gather take, from the int16 pools of the training input stage (tcr_augment_fwd's).
 * Every pointer is device memory; everything is enqueued on `stream` -- no copy, no wait.
 *
 * tcr_pcm_energy: sumsq[j] (int64 [n_clips]) = the sum of v * v over the clip_len[j] (int64) int16 samples from pcm[clip_off[j]]
 * (int64) on.  Integer arithmetic, exact: the result does not depend on the launch shape, the order of the additions or the
 * device.  clip_len[j] <= 0 gives 0.  One launch for the whole table, thousands of one-second clips and minute-long recordings
 * alike: the pool is read with 16-byte loads at a clip's aligned elements, a long clip is shared out over several workgroups in
 * groups of 16384 samples, and every group's sum is added to the table (zeroed first, on `stream`) by one 64-bit integer atomic.
 * n_clips == 0: a successful no-op.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched): n_clips < 0, a null pcm / clip_off / clip_len / sumsq, more than 2^31
 * workgroups' worth of clips. */
int tcr_pcm_energy(const int16_t* pcm, const int64_t* clip_off, const int64_t* clip_len, int64_t n_clips, int64_t* sumsq, void* stream);

/* tcr_compose: N = n_signals recordings; recording n is the packed samples sample_offsets[n] .. sample_offsets[n + 1] - 1 (int64
 * [N + 1], from 0, non-decreasing; total_samples == sample_offsets[N], which the host knows: preconditions).
 * Foreground: place_offsets (int32 [N + 1]) is a CSR over the placements; placement j of recording n puts the place_len[j] (int32)
 * samples from pcm[place_clip_off[j]] (int64) on at the recording's samples place_first[j] .. place_first[j] + place_len[j] - 1,
 * scaled by place_gain[j] (float32).  place_first (int64) may be negative or run past the recording's end: the part outside the
 * recording is dropped, a neighbouring recording is never written or read.  Preconditions: within a recording the placements are
 * sorted by place_first and disjoint, place_first[j] + place_len[j] <= place_first[j + 1] (touching is allowed; place_len[j] == 0
 * is allowed and places nothing); gains and volumes are finite.
 * Background: recording n loops the bg_len[n] (int64, >= 1) samples from bg[bg_off[n]] (int64) on, starting bg_phase[n] (int64,
 * 0 <= phase < bg_len[n]) samples in: at its sample i the background is bg[bg_off[n] + (bg_phase[n] + i) mod bg_len[n]], times
 * bg_vol[n] (float32 [N]).  bg_vol NULL: no background anywhere (bg, bg_off, bg_len and bg_phase are not read); bg_vol[n] == 0:
 * recording n's background is not read.
 * Per sample i of recording n, in float32, never contracted into an fma -- tcr_augment_fwd's operations in its order:
 *     fg  = (float)pcm[place_clip_off[j] + i - place_first[j]] * (1 / 32768.f) * place_gain[j]   if placement j covers i, else 0.f
 *     out = bg_vol[n] != 0 ? clip(((float)bgsample * (1 / 32768.f)) * bg_vol[n] + fg, -1, 1)  :  clip(fg, -1, 1)
 * out (float32 [total_samples], or NULL): that value.  out_pcm (int16 [total_samples], or NULL): tcr_mine_gather's rounding of it,
 * clamp(rint(x * 32768), -32768, 32767) with ties to even.
 * How: the packed samples are cut into tiles of TCR_COMPOSE_TILE, a few consecutive ones per workgroup, so the work is proportional to
 * total_samples whatever the recordings' lengths, and every store but the last of the total is a 16-byte one (out_pcm: 8-byte).  The recordings a tile touches,
 * each one's first placement that reaches the tile and its background phase at the tile's first sample (the one 64-bit modulo per
 * tile and recording) are wave-uniform: binary searches through scalar loads, carried forward from tile to tile within a workgroup.  The lanes walk the placements that intersect the
 * tile and find the background sample by a compare against the loop's wrap point (bg_len >= TCR_COMPOSE_TILE) or a 32-bit modulo.
 * total_samples == 0: a successful no-op.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, nothing written): out and out_pcm both NULL, N <= 0, total_samples < 0,
 * a null sample_offsets / pcm / place_offsets / place_clip_off / place_len / place_first / place_gain, bg_vol without bg / bg_off /
 * bg_len / bg_phase, an out that is not 16-byte aligned or an out_pcm that is not 8-byte aligned, more than 2^31 tiles. */
#define TCR_COMPOSE_TILE 2048
int tcr_compose(int n_signals, const int64_t* sample_offsets /* DEVICE [N + 1] */, int64_t total_samples, const int16_t* pcm,
                const int32_t* place_offsets /* [N + 1] */, const int64_t* place_clip_off, const int32_t* place_len,
                const int64_t* place_first, const float* place_gain, const int16_t* bg /* or NULL */, const int64_t* bg_off,
                const int64_t* bg_len, const int64_t* bg_phase, const float* bg_vol /* [N] or NULL */, float* out /* or NULL */,
                int16_t* out_pcm /* or NULL */, void* stream);

/* Reverberation: every clip of a table convolved with a room impulse response out of a bank, so that a corpus can vary the room
 * as tcr_compose varies the noise.  Every pointer is device memory; everything is enqueued on `stream` -- no copy, no wait.
 *
 * tcr_reverb: n_clips inputs; clip j is the n = in_len[j] (int64) samples from in[in_off[j]] (int64) on -- in_format 1: int16,
 * decoded as (float)v * (1 / 32768.f), exact; in_format 0: float32, finite (precondition).  The bank: response r is the
 * L = ir_len[r] (int32) float32 taps h[0 .. L - 1] from ir[ir_off[r]] (int64) on, finite, 1 <= L <= TCR_REVERB_TAPS_MAX; clip j
 * uses r = clip_ir[j] (int32).  Clip j writes the m = out_off[j + 1] - out_off[j] outputs out_off[j] .. of the packed output
 * (out_off int64 [n_clips + 1], from 0, non-decreasing); any m >= 0 is allowed, outputs at or beyond n + L - 1 are 0.  Output i:
 *     y[i] = the fmaf chain from 0.f over the input index jj ascending, jj = max(0, i - L + 1) .. min(i, n - 1):
 *            acc = fmaf(h[i - jj], x[jj], acc)
 * one chain per output, one rounding per product: the k-ordered chain of v_mfma_f32_16x16x4_f32.  A zero-padded term
 * fmaf(0, finite, acc) leaves acc's bits alone, so a sample's bits do not depend on the tile, the launch, the clip's neighbours or
 * where the clip and the response lie in their buffers.
 * out (float32, packed, or NULL): y.  out_pcm (int16, packed, or NULL): tcr_mine_gather's rounding of y,
 * clamp(rint(y * 32768), -32768, 32767) with ties to even -- the response [1.0f] reproduces an int16 clip byte for byte.
 * tile_off (int64 [n_clips + 1]): the prefix sums of ceil(m_j / TCR_REVERB_TILE) from 0, total_tiles == tile_off[n_clips], which
 * the host knows (a precondition, like tcr_compose's total_samples).  in_samples and ir_floats are the element counts of `in` and
 * `ir`: no load touches anything outside them, whatever the tables hold.
 * Preconditions (the Python layer checks them): 0 <= clip_ir[j] < the bank's size, 1 <= ir_len[r] <= TCR_REVERB_TAPS_MAX, clips
 * inside in[0 .. in_samples) and responses inside ir[0 .. ir_floats), out / out_pcm of out_off[n_clips] elements.
 * How: one launch, one workgroup per tile of TCR_REVERB_TILE outputs, which finds its clip by a binary search of tile_off through
 * scalar loads, so the work is proportional to the tiles and one-second clips and a ten-minute recording go in the same call.  The
 * convolution is a product with a banded Toeplitz matrix on the exact-f32 matrix core, the k loop over the input index ascending in
 * stages of TCR_REVERB_STAGE input samples staged through LDS; stages and 16-sample groups that hold only padding are skipped, so
 * the cost is about outputs x min(L, n + TCR_REVERB_TILE) multiply-adds.  Stores at a clip's ends are element-wise.
 * n_clips == 0 or total_tiles == 0: a successful no-op.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, nothing written): out and out_pcm both NULL, n_clips < 0, a null in /
 * in_off / in_len / ir / ir_off / ir_len / clip_ir / out_off / tile_off, an in_format other than 0 and 1, an out or ir that is not
 * 4-byte aligned (out_pcm: 2-byte; in: its element), a negative total_tiles / in_samples / ir_floats, 2^31 tiles or clips or more. */
#define TCR_REVERB_TILE 4096
#define TCR_REVERB_STAGE 1024
#define TCR_REVERB_TAPS_MAX 16384
int tcr_reverb(int64_t n_clips, const void* in, int in_format, int64_t in_samples, const int64_t* in_off, const int64_t* in_len,
               const float* ir, int64_t ir_floats, const int64_t* ir_off, const int32_t* ir_len, const int32_t* clip_ir,
               const int64_t* out_off /* [n_clips + 1] */, const int64_t* tile_off /* [n_clips + 1] */, int64_t total_tiles,
               float* out /* or NULL */, int16_t* out_pcm /* or NULL */, void* stream);

/* Phrase detection: multi-word phrases ("go left", "stop ... no") scored from a scan's word posteriors, as a transform of posteriors --
 * values [steps][num_classes] in, out [steps][P + 1] phrase posteriors out, the last column a background class -- so that
 * tcr_detect_redetect, tcr_detect_sweep(_ragged), tcr_detect_grid and tcr_mine_* apply to phrases unchanged with num_classes = P + 1.
 * The background does for phrases what _silence_ does for words: it is on top when no phrase scores, so the detector's
 * top != prev_label rule lets the same phrase fire again later.
 * values: float32 per signal, a scan's or a redetect's smoothed (probs is allowed).  Precondition: finite values in [0, 1]; outside
 * that range the results are unspecified, the call stays memory-safe.  Phrase q is the classes phrase_words[phrase_offsets[q] ..
 * phrase_offsets[q + 1] - 1] = c_1 .. c_n, 1 <= n <= TCR_PHRASE_MAX_WORDS, repeats allowed.  For step i of a signal (counted from the
 * signal's first step) and w = window_steps let h = max(0, i - w + 1), and f(a, b) the float32 product a * b (TCR_PHRASE_PRODUCT) or
 * fminf(a, b) (TCR_PHRASE_MIN):
 *   ordered = 1:  conf_q[i] = max over h <= t_1 <= t_2 <= .. <= t_n <= i of f(..f(f(v[t_1][c_1], v[t_2][c_2]), v[t_3][c_3]).., v[t_n][c_n]),
 *                 the fold running left to right, evaluated as the DP  E_1(t) = max(E_1(t - 1), v[t][c_1]),
 *                 E_m(t) = max(E_m(t - 1), f(E_{m-1}(t), v[t][c_m]))  over t = h .. i with m ascending inside each t, started afresh for
 *                 every i: conf_q[i] = E_n(i).  Both are the same bits, because float32 multiply and min are monotone in each
 *                 non-negative argument; the product is not re-associated.
 *   ordered = 0:  conf_q[i] = the fold over m = 1 .. n, in this order, of  max over h <= t <= i of v[t][c_m]  (Chen et al. 2014).
 *   out[i][q] = conf_q[i] for q < P,  out[i][P] = 1.0f - max over q of conf_q[i].
 * A signal's first steps never read another signal's rows.  No normalisation (an n-th root) is applied: with TCR_PHRASE_PRODUCT a
 * per-word confidence p corresponds to a threshold of p^n; TCR_PHRASE_MIN keeps thresholds on the single-word scale.
 * How: a workgroup per tile of TCR_PHRASE_TILE steps of one signal stages the tile's rows and the up to w - 1 rows in front of them
 * in LDS, the U distinct word classes only, one column after the other; a lane per step then walks its window with the DP state in
 * registers.  (TCR_PHRASE_TILE + w - 1) x U floats stay within 64 KB, which bounds the window:
 * tcr_phrase_window_max(U) = 16384 / U - 255 (U = 4: 3841, U = 12: 1110; below 1 -- no window at all -- from U = 65 on, and for
 * U < 1).  There is no path above the limit.  phrase_offsets / phrase_words are HOST tables, read before the call returns (they
 * travel as kernel arguments); every other pointer is device memory.  The entries only enqueue a kernel on `stream` -- no copy, no
 * wait -- so they can be captured into a graph like tcr_detect_redetect.  The ragged form takes step_offsets as
 * tcr_detect_redetect_ragged does (DEVICE int64 [N + 1], from 0, non-decreasing, step_offsets[N] == total_steps: preconditions).
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, out is not written): a null step_offsets (ragged) / values /
 * phrase_offsets / phrase_words / cfg / out, N, steps (dense), total_steps (ragged) or num_classes <= 0, n_phrases outside
 * 1 .. TCR_PHRASE_MAX, phrase_offsets that do not start at 0 or decrease, a phrase of 0 or more than TCR_PHRASE_MAX_WORDS words, a word
 * outside 0 .. num_classes - 1, window_steps < 1 or above tcr_phrase_window_max(U) for the U distinct word classes of the call,
 * ordered outside 0 / 1, an unknown combine, steps in all x (P + 1) or x num_classes >= 2^31. */
#define TCR_PHRASE_MAX_WORDS 8
#define TCR_PHRASE_MAX 64               /* phrases per call */
#define TCR_PHRASE_TILE 256
enum { TCR_PHRASE_PRODUCT = 0, TCR_PHRASE_MIN = 1 };
typedef struct tcr_phrase_cfg {
    int32_t window_steps, ordered, combine;
} tcr_phrase_cfg;
int tcr_phrase_window_max(int n_distinct_classes);      /* largest window_steps the staged kernel takes; < 1: none */
int tcr_phrase_scores(int n_signals, int64_t steps, int num_classes, const float* values /* [N][steps][C] */, int n_phrases,
                      const int32_t* phrase_offsets /* HOST [P + 1] */, const int32_t* phrase_words /* HOST */,
                      const tcr_phrase_cfg* cfg, float* out /* [N][steps][P + 1] */, void* stream);
int tcr_phrase_scores_ragged(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int num_classes,
                             const float* values /* packed [total_steps][C] */, int n_phrases, const int32_t* phrase_offsets /* HOST */,
                             const int32_t* phrase_words /* HOST */, const tcr_phrase_cfg* cfg, float* out /* [total_steps][P + 1] */,
                             void* stream);

/* Streaming phrase detection: tcr_phrase_scores and the detector over its posteriors with the phrase window and the detector carried
 * across calls, for S live streams (what tcr_stream_step / tcr_stream_scan / tcr_stream_scan_ragged wrote in smoothed or probs goes
 * in as it comes).  State is caller-owned device memory of tcr_phrase_stream_state_bytes (0: invalid arguments, see tcr_last_error),
 * filled by tcr_phrase_stream_init (every stream: no rows seen, prev_label = -1); it belongs to one (n_streams, num_classes, phrase
 * tables, cfg), and the same values must be passed to every push.
 * tcr_phrase_stream_push: values [S][steps][num_classes], `steps` new rows for every stream -> post [S][steps][P + 1], top / score /
 * is_new [S][steps].  tcr_phrase_stream_push_ragged: stream s brings m_s = step_offsets[s + 1] - step_offsets[s] >= 0 rows, values and
 * the four outputs packed [total_steps][..] with stream s's rows at step_offsets[s] .. (DEVICE int64 [S + 1], from 0, non-decreasing,
 * step_offsets[S] == total_steps: preconditions, the host does not read the table).
 * Contract: for stream s let R_s be all rows pushed to it since its init or last reset, in order.  The post rows a call writes for s
 * are bitwise the corresponding (last) rows of tcr_phrase_scores(1, len(R_s), ..) over R_s -- the float32 operations and their order
 * are the ones fixed above, evaluated over the same rows oldest first -- and top / score / is_new are bitwise tcr_detect_redetect
 * over those posteriors with `det` (num_classes = P + 1): the rule of tcr_stream_step at average_steps = min_count = 1, with n,
 * prev_label and prev_step carried.  So any way of cutting a stream into pushes gives the outputs of one whole scan, and after a call
 * the state is what any other split of the same rows leaves; dense, ragged and one-step (steps = 1) calls mix freely on one state.
 * reset [S] uint8 or NULL: reset[s] != 0 returns stream s to the initial state before its first row of this call.  In a ragged call
 * a stream with m_s == 0 is untouched -- its state is byte for byte what it was -- and reset[s] is IGNORED for it (pass the flag again
 * with the call that brings the stream's next row).  Streams are independent.  Precondition: fewer than 2^31 rows per stream since
 * its reset.
 * State: the detector integers [5][S] int32 as tcr_stream_step keeps them (head, count, prev_label, prev_step, n; at one vector per
 * decision head stays 0 and count 1, and n is the rows the stream has seen), rounded up to 256 bytes, then a ring of the last w - 1
 * rows, the U distinct word classes only, planar over the streams: float32 [w - 1][U][S], row r of a stream (counted from its
 * reset) in slot r mod (w - 1).  A call writes only the slots of its new rows (the last w - 1 of them), in a launch of its own behind
 * every reader of the old rows.
 * How: a call that brings at most 4 rows per stream on average (a server's one-step pushes) runs a lane per row, phrases dealt to the
 * waves of a workgroup, every window walked from the ring and `values` in global memory -- consecutive lanes are consecutive streams,
 * so a dense one-step push reads consecutive addresses; a larger call (a recording in chunks) runs tcr_phrase_scores' tile kernel with
 * the up to w - 1 rows in front of a stream's first tile staged from the ring.  The window limit stays tcr_phrase_window_max(U).
 * Like the entries above these only enqueue kernels on `stream` (tcr_phrase_stream_init: a memset and a kernel) -- no copy, no wait,
 * the phrase tables travel as kernel arguments -- so they can be captured into a graph.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, the state and the outputs are untouched): everything tcr_phrase_scores
 * refuses (n_streams for N); a null state, det, post, top, score or is_new, a null step_offsets (ragged); det->average_steps != 1 or
 * det->min_count != 1; det->suppression_steps < 0; n_streams <= 0; steps (ragged: total_steps) <= 0; steps in all x (P + 1) or
 * x num_classes >= 2^31. */
size_t tcr_phrase_stream_state_bytes(int n_streams, int num_classes, int n_phrases, const int32_t* phrase_offsets /* HOST [P + 1] */,
                                     const int32_t* phrase_words /* HOST */, const tcr_phrase_cfg* cfg);
int tcr_phrase_stream_init(int n_streams, int num_classes, int n_phrases, const int32_t* phrase_offsets /* HOST */,
                           const int32_t* phrase_words /* HOST */, const tcr_phrase_cfg* cfg, void* state, void* stream);
int tcr_phrase_stream_push(int n_streams, int64_t steps, int num_classes, const float* values /* [S][steps][C] */, int n_phrases,
                           const int32_t* phrase_offsets /* HOST */, const int32_t* phrase_words /* HOST */, const tcr_phrase_cfg* cfg,
                           const tcr_detect_cfg* det, const uint8_t* reset /* [S] or NULL */, void* state,
                           float* post /* [S][steps][P + 1] */, int32_t* top, float* score, int32_t* is_new /* [S][steps] */,
                           void* stream);
int tcr_phrase_stream_push_ragged(int n_streams, const int64_t* step_offsets /* DEVICE [S + 1] */, int64_t total_steps,
                                  int num_classes, const float* values /* packed [total_steps][C] */, int n_phrases,
                                  const int32_t* phrase_offsets /* HOST */, const int32_t* phrase_words /* HOST */,
                                  const tcr_phrase_cfg* cfg, const tcr_detect_cfg* det, const uint8_t* reset /* [S] or NULL */,
                                  void* state, float* post /* [total_steps][P + 1] */, int32_t* top, float* score,
                                  int32_t* is_new /* [total_steps] */, void* stream);

/* Enrolled keywords (template matching): keywords the model was not trained on, detected by query-by-example -- the feature rows of a
 * few recorded examples are kept as templates and matched against the running rows by subsequence dynamic time warping.  Like the
 * phrase entries this is a transform of posteriors: values [steps][F] float32 feature rows in (a scan's smoothed or probs with
 * F = num_classes; any other float32 rows of F <= TCR_DTW_MAX_FEATURES columns), out [steps][K + 1] posteriors over K keywords and a
 * background class out, and lengths [steps][K] int32 (or NULL), so that tcr_detect_redetect, tcr_detect_sweep(_ragged),
 * tcr_detect_grid and tcr_mine_* apply to enrolled keywords unchanged with num_classes = K + 1.
 * The score.  Every operation is float32, evaluated as written, no multiply-add fused.  Template q has L_q frames T[j][f] (templates:
 * DEVICE, packed [total_frames][F], template q's frames at frame_offsets[q] .. frame_offsets[q + 1] - 1).  A signal's rows are
 * v_t[f], t counted from the signal's first step (a stream: from its init or last reset).
 *   local distance:  d(j, t) = a_{F-1},  a_0 = |T[j][0] - v_t[0]|,  a_f = a_{f-1} + |T[j][f] - v_t[f]|, f ascending (no multiply).
 *   before a signal's first row:  D[j] = +inf, n[j] = 0 for every j.
 *   step t, for every j from the previous column D', n' only, three candidates in priority order:
 *     1. diag: (D'[j-1], n'[j-1]) if j >= 1, else (0, 0) -- the free start: a path may begin at any step;
 *     2. stay: (D'[j], n'[j]);
 *     3. skip: (D'[j-2], n'[j-2]) if j >= 2, (0, 0) if j == 1, (+inf, 0) if j == 0;
 *     best = diag; if stay.D < best.D: best = stay; if skip.D < best.D: best = skip (strict: ties keep the earlier candidate);
 *     D[j] = d(j, t) + best.D,  n[j] = min(best.n, INT32_MAX - 1) + 1.
 *   per template:  cost_q(t) = D[L_q - 1], len_q(t) = n[L_q - 1] (the steps on the best path: the match spans t - len + 1 .. t);
 *     conf_q(t) = fmaxf(1 - cost_q(t) * scale[q], 0), and 0 instead if cfg.max_steps > 0 and len_q(t) > cfg.max_steps (+inf costs give
 *     0 by the same expression).  scale: HOST float32 [Q], every entry finite and > 0 (0.5 / L_q maps the mean total variation of
 *     probability rows onto [0, 1]).
 *   per keyword:  keyword k owns templates keyword_offsets[k] .. keyword_offsets[k + 1] - 1 (at least one).  out[t][k] = the maximum of
 *     their conf in ascending template order with strict > (the first maximum wins), lengths[t][k] = the winning template's len,
 *     out[t][K] = 1 - max_k out[t][k] (the background: what it is for phrases).
 * A signal's first steps never read another signal's rows or state.  For values outside [0, 1] or non-finite ones the results are
 * unspecified, the call stays memory-safe.  The cost is summed per step and normalised by L through scale, so it prefers short paths:
 * that is what lengths and max_steps are for.
 * How: one wave per (signal, keyword) walks the keyword's templates one after the other over the signal's rows; a lane owns
 * ceil(L / 64) <= 4 consecutive frames with D and n in registers and its template frames in LDS, the rows come through an LDS tile
 * fetched one tile ahead, and the neighbour's last two (D, n) pairs are handed over by two shuffles a step.  A second small kernel
 * writes the background.  The walk is sequential in t: the parallelism of a call is N x K waves (a single long recording with one
 * keyword runs on one wave).  Limits: Q <= TCR_DTW_MAX_TEMPLATES, F <= TCR_DTW_MAX_FEATURES, L_q <= tcr_dtw_frames_max(F) =
 * min(256, 4096 / F) (256 up to F = 16, 64 at F = 64; 0 for F outside 1 .. 64); there is no path above them.  frame_offsets,
 * keyword_offsets and scale are HOST tables, read before the call returns (they travel as kernel arguments); every other pointer is
 * device memory.  The entries only enqueue kernels on `stream` -- no copy, no wait -- so they can be captured into a graph.  The
 * ragged form takes step_offsets as tcr_detect_redetect_ragged does (DEVICE int64 [N + 1], from 0, non-decreasing, step_offsets[N]
 * == total_steps: preconditions).
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, out and lengths are not written): a null step_offsets (ragged) / values
 * / templates / frame_offsets / keyword_offsets / scale / cfg / out; N, steps (dense), total_steps (ragged) or n_features <= 0;
 * n_features above TCR_DTW_MAX_FEATURES; n_templates outside 1 .. TCR_DTW_MAX_TEMPLATES; n_keywords outside 1 .. n_templates; offsets
 * that do not start at 0 or decrease; keyword_offsets that does not end at n_templates; a keyword without a template; a template of 0
 * or more than tcr_dtw_frames_max(n_features) frames; a scale <= 0 or non-finite; max_steps < 0; steps in all x (K + 1) or x
 * n_features >= 2^31. */
#define TCR_DTW_MAX_TEMPLATES 64
#define TCR_DTW_MAX_FEATURES 64
typedef struct tcr_dtw_cfg {
    int32_t max_steps;          /* > 0: a match of more steps scores 0; 0: no limit */
} tcr_dtw_cfg;
int tcr_dtw_frames_max(int n_features);                 /* the largest template, in frames; 0: n_features outside 1 .. 64 */
int tcr_dtw_scores(int n_signals, int64_t steps, int n_features, const float* values /* [N][steps][F] */, int n_templates,
                   const float* templates /* DEVICE [total_frames][F] */, const int32_t* frame_offsets /* HOST [Q + 1] */, int n_keywords,
                   const int32_t* keyword_offsets /* HOST [K + 1] */, const float* scale /* HOST [Q] */, const tcr_dtw_cfg* cfg,
                   float* out /* [N][steps][K + 1] */, int32_t* lengths /* [N][steps][K] or NULL */, void* stream);
int tcr_dtw_scores_ragged(int n_signals, const int64_t* step_offsets /* DEVICE [N + 1] */, int64_t total_steps, int n_features,
                          const float* values /* packed [total_steps][F] */, int n_templates, const float* templates /* DEVICE */,
                          const int32_t* frame_offsets /* HOST */, int n_keywords, const int32_t* keyword_offsets /* HOST */,
                          const float* scale /* HOST */, const tcr_dtw_cfg* cfg, float* out /* [total_steps][K + 1] */,
                          int32_t* lengths /* [total_steps][K] or NULL */, void* stream);

/* Streaming template matching: tcr_dtw_scores and the detector over its posteriors with the DTW column and the detector carried across
 * calls, for S live streams -- the tcr_phrase_stream_* entries' arguments and meaning, with the template tables for the phrase tables
 * and `lengths` ([..][K] int32 or NULL) next to post.  State is caller-owned device memory of tcr_dtw_stream_state_bytes (0: invalid
 * arguments, see tcr_last_error), filled by tcr_dtw_stream_init (every stream: the initial column, no rows seen, prev_label = -1);
 * it belongs to one (n_streams, n_features, tables, cfg), and the same values must be passed to every push.
 * Contract: for stream s let R_s be all rows pushed to it since its init or last reset, in order.  The post and lengths rows a call
 * writes for s are bitwise the corresponding (last) rows of tcr_dtw_scores(1, len(R_s), ..) over R_s, and top / score / is_new are
 * bitwise tcr_detect_redetect over those posteriors with `det` (num_classes = K + 1, average_steps = min_count = 1), with n,
 * prev_label and prev_step carried.  The recurrence reads the previous column only, so any way of cutting a stream into pushes gives
 * the outputs of one whole scan, a one-step push costs one step, and dense, ragged and one-step calls mix freely on one state.
 * reset [S] uint8 or NULL: reset[s] != 0 returns stream s to the initial state before its first row of this call.  In a ragged call a
 * stream with m_s == 0 is untouched -- its state is byte for byte what it was -- and reset[s] is IGNORED for it (pass the flag again
 * with the call that brings the stream's next row).  Streams are independent.  Precondition: fewer than 2^31 rows per stream since
 * its reset.
 * State (opaque to callers; for the record): the detector integers [5][S] int32 as tcr_stream_step keeps them, rounded up to 256
 * bytes, then D float32 and n int32, each [total_frames x S]: template q's block at frame_offsets[q] x S, stream s's L_q values at
 * s x L_q inside it.  tcr_dtw_stream_state_bytes = that rounding + 8 x total_frames x S.
 * A push is tcr_dtw_scores' two kernels on the carried columns, then detect_smooth_kernel at one vector per decision and
 * scan_suppress_kernel; tcr_dtw_stream_init is a memset and a kernel.  No copy, no wait: the entries can be captured into a graph.
 * Refused (TCR_ERR_ARG, tcr_last_error; nothing is launched, the state and the outputs are untouched): everything tcr_dtw_scores
 * refuses (n_streams for N; lengths may be NULL); a null state, det, post, top, score or is_new; det->average_steps != 1 or
 * det->min_count != 1; det->suppression_steps < 0. */
size_t tcr_dtw_stream_state_bytes(int n_streams, int n_features, int n_templates, const float* templates /* DEVICE */,
                                  const int32_t* frame_offsets /* HOST [Q + 1] */, int n_keywords, const int32_t* keyword_offsets /* HOST */,
                                  const float* scale /* HOST [Q] */, const tcr_dtw_cfg* cfg);
int tcr_dtw_stream_init(int n_streams, int n_features, int n_templates, const float* templates /* DEVICE */,
                        const int32_t* frame_offsets /* HOST */, int n_keywords, const int32_t* keyword_offsets /* HOST */,
                        const float* scale /* HOST */, const tcr_dtw_cfg* cfg, void* state, void* stream);
int tcr_dtw_stream_push(int n_streams, int64_t steps, int n_features, const float* values /* [S][steps][F] */, int n_templates,
                        const float* templates /* DEVICE */, const int32_t* frame_offsets /* HOST */, int n_keywords,
                        const int32_t* keyword_offsets /* HOST */, const float* scale /* HOST */, const tcr_dtw_cfg* cfg,
                        const tcr_detect_cfg* det, const uint8_t* reset /* [S] or NULL */, void* state,
                        float* post /* [S][steps][K + 1] */, int32_t* lengths /* [S][steps][K] or NULL */, int32_t* top, float* score,
                        int32_t* is_new /* [S][steps] */, void* stream);
int tcr_dtw_stream_push_ragged(int n_streams, const int64_t* step_offsets /* DEVICE [S + 1] */, int64_t total_steps, int n_features,
                               const float* values /* packed [total_steps][F] */, int n_templates, const float* templates /* DEVICE */,
                               const int32_t* frame_offsets /* HOST */, int n_keywords, const int32_t* keyword_offsets /* HOST */,
                               const float* scale /* HOST */, const tcr_dtw_cfg* cfg, const tcr_detect_cfg* det,
                               const uint8_t* reset /* [S] or NULL */, void* state, float* post /* [total_steps][K + 1] */,
                               int32_t* lengths /* [total_steps][K] or NULL */, int32_t* top, float* score,
                               int32_t* is_new /* [total_steps] */, void* stream);

/* Capturing detections' audio on live streams: a recorder next to a streaming detector (tcr_stream_step / tcr_stream_scan / _ragged,
 * tcr_phrase_stream_push*, a cascade: anything that writes top / score / is_new per stream and row) that hands back, for each of the
 * detector's detections, the clip DetectionStage.mine's gather (tcr_mine_gather) cuts from the whole recording -- bitwise, however
 * the stream is cut into pushes, although the audio is gone once pushed.
 * Definition.  A stream's RECORDING is every sample pushed to it since its init or last reset; row i is its i-th step of step_samples
 * samples.  Row i is a TRIGGER when is_new[i] != 0 and, with a class mask, 0 <= top[i] < num_classes and class_mask[top[i]] != 0.  The
 * CLIP of trigger row i is
 *     recording[(i + 1) * step_samples + lead - n_samples  ..  (i + 1) * step_samples + lead)
 * with zeros outside the recording; lead (samples) may have either sign.  With  D = max(0, ceil(lead / step_samples))  the clip of row
 * i is EMITTED by the call that brings the stream's row i + D, the first row after which all the clip's samples have been heard; with
 * lead <= 0 that is the trigger's own call.
 * Why a ring of  H = n_samples + max(0, -lead)  samples suffices: in the call that emits it a clip ends at or after the end of the
 * call's first row minus max(0, -lead) samples ((i + 1 - r0) step + lead with i + D >= r0 and D step >= lead > (D - 1) step), so it
 * starts less than H samples before the call's first sample; everything later is in the call itself.
 * State (caller-owned device memory of tcr_capture_state_bytes, 16-byte aligned, zeroed by tcr_capture_init: no rows heard, nothing
 * pending; it belongs to one (n_streams, step_samples, n_samples, lead)): per stream {int64 rows heard, int32 ring slot of the next
 * sample, int32 0} [S], rounded up to 256 bytes; the triggers of every stream's last D rows, oldest first -- int32 flag [S][D],
 * int32 label [S][D], float32 score [S][D] -- rounded up to 256 bytes; the ring float32 [S][R], R = H rounded up to 4, sample t of
 * the recording in slot t mod R.  In all  S (16 + 12 D + 4 R)  bytes and the rounding: 4096 streams at one second of 16 kHz audio are
 * 262 MB.  After a call the state is what any other split of the same rows leaves.
 * tcr_capture_push: samples [S][steps * step_samples], top / score / is_new [S][steps], `steps` new rows for every stream.
 * tcr_capture_push_ragged: stream s brings m_s = step_offsets[s + 1] - step_offsets[s] >= 0 rows (DEVICE int64 [S + 1], from 0,
 * non-decreasing, step_offsets[S] == total_steps: preconditions, the host does not read the table), samples [total_steps *
 * step_samples] and the three row arrays [total_steps] packed in stream order.  A stream with m_s == 0 keeps every byte of its
 * state, and reset[s] is IGNORED for it (pass the flag again with the call that brings its next row).
 * reset [S] uint8 or NULL: reset[s] != 0 applies before the stream's first row of the call: its pending triggers are dropped, earlier
 * audio reads as zeros, rows count from 0 again.
 * Outputs, in (stream, row) order: clip_stream int32, clip_step int64 (the trigger's row, counted from the reset), clip_label int32
 * (top), clip_score float32 [capacity]; out float32 [capacity][n_samples] and / or out_pcm int16 [capacity][n_samples] (either may be
 * NULL; the int16 rounding is tcr_mine_gather's own function); n_clips int32 [2]: the clips written, then the clips due.  When more
 * than `capacity` clips are due the first `capacity` of that order are written and the rest are DROPPED (n_clips[1] tells); this is
 * not an error.  Rows of the outputs past n_clips[0] are not touched.
 * tcr_capture_flush: emits the pending clips -- the triggers among the last D rows -- of the streams with mask[s] != 0 (NULL: all),
 * audio not yet heard reading as zeros (what mining gives for a detection near a recording's end), and clears those triggers, so a
 * stream that goes on does not emit them again; ring and row count stay.  With lead <= 0 nothing is ever pending (n_clips = 0, 0).
 * Workspace: tcr_capture_workspace_bytes(total_rows) for a push of total_rows rows in all (dense: S * steps), S * D for a flush; 16-byte
 * aligned; a larger one serves smaller calls.
 * How: a flag per row (row j emits the trigger of row j - D, from the call or the carried tail), tcr_scan_select's ordered compaction
 * into the table, a gather of min(capacity, rows) workgroup rows that exits on the device-side count and reads each clip from the ring
 * (at most two wrapped stretches) and the call's samples with tcr_mine_gather's 16-byte row code, then the append of the call's last R
 * samples per stream (16-byte stores when step_samples is a multiple of 4 and samples is 16-byte aligned, single floats otherwise).
 * Only kernels are enqueued on `stream` (tcr_capture_init: a memset) -- no copy, no wait, nothing read back: the calls can be captured
 * into a graph.  Precondition: fewer than 2^63 / step_samples rows per stream since its reset.
 * Refused (TCR_ERR_ARG; tcr_capture_state_bytes / _workspace_bytes return 0): n_streams, step_samples or n_samples <= 0; step_samples,
 * n_samples or |lead| above 2^28; a state of 10^15 bytes or more (size overflow); total_rows outside 1 .. 2^31 - 1; steps (ragged:
 * total_steps) <= 0; 2^40 or more samples in a call; a null or misaligned state or workspace; a null samples, top, score, is_new,
 * n_clips, step_offsets (ragged); a class mask with num_classes <= 0; capacity outside 0 .. 2^31 - 1, or null tables with capacity
 * > 0.  TCR_ERR_WORKSPACE: a workspace smaller than tcr_capture_workspace_bytes of the call's rows. */
size_t tcr_capture_state_bytes(int n_streams, int step_samples, int n_samples, int lead);
size_t tcr_capture_workspace_bytes(int64_t total_rows);
int tcr_capture_init(int n_streams, int step_samples, int n_samples, int lead, void* state, void* stream);
int tcr_capture_push(int n_streams, int64_t steps, int step_samples, int n_samples, int lead,
                     const float* samples /* [S][steps * step_samples] */, const int32_t* top, const float* score,
                     const int32_t* is_new /* [S][steps] */, const uint8_t* class_mask /* [num_classes] or NULL */, int num_classes,
                     const uint8_t* reset /* [S] or NULL */, void* state, void* workspace, size_t ws_bytes, int64_t capacity,
                     float* out /* [capacity][n_samples] or NULL */, int16_t* out_pcm /* or NULL */, int32_t* clip_stream,
                     int64_t* clip_step, int32_t* clip_label, float* clip_score, int32_t* n_clips /* DEVICE [2] */, void* stream);
int tcr_capture_push_ragged(int n_streams, const int64_t* step_offsets /* DEVICE [S + 1] */, int64_t total_steps, int step_samples,
                            int n_samples, int lead, const float* samples /* packed */, const int32_t* top, const float* score,
                            const int32_t* is_new /* [total_steps] */, const uint8_t* class_mask /* [num_classes] or NULL */,
                            int num_classes, const uint8_t* reset /* [S] or NULL */, void* state, void* workspace, size_t ws_bytes,
                            int64_t capacity, float* out, int16_t* out_pcm, int32_t* clip_stream, int64_t* clip_step,
                            int32_t* clip_label, float* clip_score, int32_t* n_clips /* DEVICE [2] */, void* stream);
int tcr_capture_flush(int n_streams, const uint8_t* mask /* [S] or NULL: all */, int step_samples, int n_samples, int lead, void* state,
                      void* workspace, size_t ws_bytes, int64_t capacity, float* out, int16_t* out_pcm, int32_t* clip_stream,
                      int64_t* clip_step, int32_t* clip_label, float* clip_score, int32_t* n_clips /* DEVICE [2] */, void* stream);

/* Sample-rate conversion: a rational-ratio polyphase FIR in front of the detectors (which take float32 at the model's rate).
 * in_rate -> out_rate, g = gcd: up = L = out_rate / g, down = M = in_rate / g; taps = P per phase (even, or 1); table float32
 * [up][taps], designed on the host (tcresnet_amd.resampling.design_table: windowed sinc, fc = rolloff / max(1, M / L), Kaiser
 * window over zero_crossings * max(1, M / L) input samples each side, every phase row divided by its sum: unit DC gain).
 * Output j >= 0 (global index, int64):
 *     n_j = floor(j M / L),  phi_j = (j M) mod L,  lead = P / 2 - 1 (0 when P == 1),
 *     y[j] = sum over p = 0 .. P - 1, in this order, as one fmaf chain starting from 0:  table[phi_j][p] * x[n_j - lead + p].
 * x[i] is the decoded input at global index i: float32 as is, int16 as (float)v * (1.0f / 32768.0f) (exact); x[i] = 0 for every i
 * outside the span the caller passed, so the start of a signal, its end and a final flush need no special case.  A signal of n_in
 * samples has ceil(n_in L / M) outputs.  The order of the chain is part of the contract: a sample's value does not depend on the
 * tile, the chunk or the call that computed it, so converting a range of outputs in pieces is bitwise converting it at once.  With
 * up = down = taps = 1 and the table {1.0f} the result is bitwise the decoded input.  Positions are 64-bit on host and device
 * (j M passes 2^32 within an hour of 44.1 kHz audio).
 * Live audio: keep the last `taps` input samples of each stream next to the new ones in one buffer, call tcr_resample with the
 * buffer's global index as in_first and the outputs whose span (tcr_resample_span) has arrived; at the end call once more for the
 * remaining outputs up to ceil(n_total L / M) - 1: the future reads as zeros. */
typedef struct {
    int32_t up, down, taps;
    int32_t in_format;          /* 0 float32, 1 int16 */
    int32_t in_step;            /* elements between consecutive samples of a row: the channel count of interleaved PCM (channel 0 is read) */
} tcr_resample_cfg;
/* in: S rows; row s starts at in + s * in_pitch elements and holds n_in samples (in_step elements apart), the first of which has
 * global index in_first (which may be negative).  out[s * out_pitch + (j - out_first)] = y[j] for j in [out_first, out_first + n_out).
 * table: device float32 [up][taps].  Stateless; nothing is read outside the rows, nothing written outside out's n_out columns.
 * Every pointer is device memory; the launch is enqueued on `stream`.  n_out == 0 or S == 0: a successful no-op.  Refused
 * (TCR_ERR_ARG, tcr_last_error, no launch): null pointers, up / down / taps < 1, odd taps other than 1, unknown in_format,
 * in_step < 1, negative counts, in_pitch < (n_in - 1) in_step + 1, out_pitch < n_out, positions past 2^61 / down, and what a
 * workgroup cannot stage: taps > 6143 (a table row), or, with G = min(up, 32, 6144 / (taps | 1)) rows per workgroup,
 * taps + ceil(G down / up) + 1 > 14336 (the input samples of one row group: e.g. down > 14333 at up = 1, taps = 2); with n_out > 0
 * and S > 0 also up > 65535 G (more row groups than one launch covers). */
int tcr_resample(const tcr_resample_cfg* cfg, const float* table, int n_streams, const void* in, int64_t in_pitch, int64_t in_first,
                 int64_t n_in, int64_t out_first, int64_t n_out, float* out, int64_t out_pitch, void* stream);
/* The input span [first, first + n) that outputs [out_first, out_first + n_out) read: first = floor(out_first M / L) - lead,
 * first + n - 1 = floor((out_first + n_out - 1) M / L) - lead + taps - 1 (n = 0 when n_out == 0).  Host arithmetic only. */
int tcr_resample_span(const tcr_resample_cfg* cfg, int64_t out_first, int64_t n_out, int64_t* first, int64_t* n);

/* ------------------------------------------------------------------------------------------ */
/* Instrumentation                                                                             */
/* ------------------------------------------------------------------------------------------ */
/* Name of the n-th kernel family in this library (NULL past the end); used by bench.py to match
 * rocprofv3 kernel-trace rows. */
const char* tcr_kernel_name(int index);

/* Process-wide kernel-selection knobs for A/B measurements (defaults = 0 = the tuned choice). */
enum { TCR_TUNE_CONV_PATH = 0,   /* 0 auto: implicit-GEMM MFMA conv where the shape fits, 1: scalar-fed VALU conv, 2: as 0 */
       TCR_TUNE_FRONTEND = 1,    /* 0 / 5: packed-FP32 kernel (default); 1..4: scalar-FP32 kernel, variant (v-1): bit0 wave-local phase ordering, bit1 sample prefetch */
       TCR_TUNE_CONV_B = 2,      /* MFMA conv activations: 0 straight from global/L1 (default), 1 via an LDS image; 3: wide 1x1 convs on the register-fed kernel instead of the LDS-tiled one, DS-CNN conv_1 not fused with the first depthwise layer */
       TCR_TUNE_NET_FUSED = 3,   /* eval forward: 0 one fused LDS-resident kernel for the whole net (default; layers of the flagship shapes run compile-time-specialised), 1 per-layer kernels, 2 fused with the features copied to LDS, 3 fused, generic layer walk only, 4 the round-2 static-shape layer, 5 the static kernel with four 16-position tiles per job in block 0's layers instead of two (round 5 experiment: bitwise, no faster), 7 fused without the bank-aligned utterance strides (A/B arm); the static kernels' nine-tap layers (round 6): 0 work dealt in 16-position units, as even over the waves as units allow, + a whole tap of weight lookahead in the layers of <= 32 input channels (TCResNet14-1.5: <= 48) (default), 8 jobs of two tiles dealt round-robin (rounds 3-5), 9 units without the lookahead; TCResNet8-1.0's kernel, conv0_1 (block 0's nine-tap layer of 24 input channels): 0 a row tile's whole weight set resident in registers across a wave's run of units, requested in front of the phase's barrier (default at 49 frames), 10 the round-6 walk (default at 98 frames, where the resident form measured no faster), 11 the resident walk at either frame count (all bitwise); groups of 8 utterances at 49 frames (12 classes, 8 waves): 0 the TIME-MAJOR plan (default) -- positions ordered 8 * frame + utterance, LDS rows [channel][frame + 4 + 4 halo frames][8 utterances] with a channel pitch of 16 (mod 32) floats where a stride-1 layer reads them and 8 (mod 32) where a stride-2 layer does (rows no convolution reads: no halo, no pad), so a 16-position tile is two frames of every utterance and the taps that would multiply only SAME-padding zeros for both frames are not issued (conv0_1's resident walk stays whole), jobs dealt by live-tap count, weight fragments by 16-byte loads out of the frozen table's weight image where the table carries one (13: the time-major plan with the 4-byte loads from `params` whatever the table carries, A/B arm, bitwise); bitwise unless a weight is not finite (Inf * 0 no longer enters the edge outputs) --, 12 the utterance-major walk on those groups too (A/B arm; what every other group size, the 98-frame kernel and TCResNet14-1.5 run) */
       TCR_TUNE_FUSED_GROUP = 4, /* utterances per workgroup group of the fused kernel (0: largest that fits 64 KB of LDS) */
       TCR_TUNE_FUSED_WAVES = 5, /* fused kernel: waves per workgroup (4, 8, 16) + 100 * weight-ring depth (4, 8, 16); 0: default */
       TCR_TUNE_CONV_KSPLIT = 6, /* train-mode conv / data-gradient: waves sharing one 32-position group's reduction (0 auto, 1, 2, 4) */
       TCR_TUNE_WGRAD_STREAM = 7,/* backward: 0 weight-gradient kernels on the library's internal streams (one set per device and process; default), 1 everything on the caller's stream, 2: as 0 with the TC-ResNet shortcut units (BN backward, data and filter gradient) on the second internal stream instead of behind the other units' filter gradients (measured: -1 % at 49 frames, +7 % for TCResNet8 at 98); 3: lazy backward with one stream fork per block instead of one per BN unit (measured slower: +3 %) */
       TCR_TUNE_TRAIN_FWD = 8,   /* train-mode forward: 0 group-resident phases (train_fused.hip; BN affine / ReLU / residual applied while the next conv stages its input, statistics from the conv epilogue), 1 per-layer kernels (conv -> statistics -> finalize -> normalise), 2: as 0 with the head walking the block output's rows for its pooling instead of starting from the sums over time the closing phase leaves (round 6; bitwise the same) */
       TCR_TUNE_TRAIN_BWD = 9,   /* TC-ResNet backward: 0 "lazy" BN backward (bwd_lazy.hip: dy never written -- the data-gradient kernel applies BN backward while it stages a group of utterances into LDS, runs every stride phase and the block's shortcut conv from that image and leaves the next unit's sums from its epilogue; the filter-gradient kernels compute dy where they load it; default for nets of <= 48 channels, where it measured faster; 3: for every net it covers), 1 the group-resident phases of round 2 (train_fused_bwd.hip), 2 the per-layer chain (reduce -> finalize + bn_bwd_apply -> data gradient per phase; the default until round 3) */
       TCR_TUNE_PHASE_CFG = 10,  /* training phases: waves per workgroup * 100 + utterances per group (0: default) */
       TCR_TUNE_BWD_BN_FUSED = 11, /* BN backward: 0 finalize folded into the apply pass (one launch, ~512 workgroups; round 6: for every layer width -- rounds 3-5: <= 48 channels, 1024 workgroups), 1 finalize + apply kernels, >= 2: folded, that many workgroups aimed at */
       TCR_TUNE_BWD_MASK = 12,   /* BN backward: 0 a unit's own ReLU mask recomputed from its raw conv output ([fmaf(y, scale, shift) > 0], bitwise the activation's; default), 1 read back from the stored activation, 2: as 0 with the scalar (one element per thread) elementwise BN kernels instead of the 16-byte ones (bitwise the same), 3: also the scalar per-channel reduction kernel (another summation order), 4: the 16-byte reduction kernel also where its grid would be small (tests), 5: as 0 with the lazy backward's last block reduced by two launches (conv_b's unit, then the shortcut's reading the masked gradient back) instead of one two-unit pass (round 6; bitwise the same rows) */
       TCR_TUNE_FE_GRID = 13,    /* front-end: cap on the number of persistent workgroups (0: two per CU). 256 = one per CU, which leaves half of every CU's LDS and registers to a co-resident network kernel on another stream */
       TCR_TUNE_FUSED_GRID = 14, /* fused eval network: cap on the number of persistent workgroups (0: as many as the LDS allows per CU) */
       TCR_TUNE_DS_TRAIN = 15,   /* DS-CNN training: 0 normalised activations never materialised where every consumer has the form (172 / 276-channel nets): consumers apply BN + ReLU to the raw conv outputs, batch statistics and backward sums come from conv / data-gradient epilogues (default); 1 the materialising path (statistics reduce -> finalize -> normalise, backward reduce); 2: as 0, but every unit's BN backward by a bn_bwd_apply pass (default 0: conv_1's filter gradient computes dy where it reads it); 3: as 0, the depthwise units' kernels too; 4: as 0, and the pointwise units' data-gradient kernel applies the BN backward while staging and writes dy for the filter gradient instead of a bn_bwd_apply pass (measured slower) */
       TCR_TUNE_WGRAD_TILES = 16, /* 9-tap filter gradients (16-byte-load kernel): output-channel tiles per launch (0: default 2 since round 6, 3 before; a layer of more tiles is split into launches that share one slab) */
       TCR_TUNE_DOWN_DGRAD = 17,  /* TC-ResNet backward, a block's 1x1 shortcut conv: 0 its data gradient runs early on the side stream and writes the block-input gradient first, conv_a's adds onto it (default for nets of <= 48 channels and, since round 6, for wider nets from 64 frames up, where it measured faster; 2: for every net); 1 conv_a's first, the shortcut's added behind it on the main stream (bitwise the same sums: one addition, commuted) */
       TCR_TUNE_BWD_LAZY_CFG = 18, /* lazy backward geometry: utterances per group + 100 * waves per job (0: cost model) + 10000 * (out channels * 10 + layers) to address one kernel of the net */
       TCR_TUNE_PHASE_STATIC = 19, /* training forward phases of TCResNet8-1.0 / TCResNet14-1.5 at 49 / 98 frames: 0 compile-time-shaped kernels, utterance stride in LDS padded to the bank pattern (default); bit 0: generic layer walk; bit 1: unpadded stride; bit 2: the phases' staging one element at a time with its coefficients gathered from global memory (rounds 2-5) instead of float4 accesses + an LDS coefficient table (round 6) (A/B arms, all bitwise) */
       TCR_TUNE_WGRAD_WAVES = 20, /* on-the-fly 9-tap filter gradients: waves per workgroup (0: policy; 4, 8, 12, 16) */
       TCR_TUNE_WGRAD_LDS = 21,  /* first conv's filter gradient: 0 the LDS-staged nine-wave kernel (default), 1 the 16-byte-load kernel; per-layer chain, round 6 A/B arms (bitwise the default): 2 the first conv's dy written by an apply pass instead of built where the filter gradient loads it, 3 every layer's split-K slabs summed in one pass at the step's end instead of the first half of the units early */
       TCR_TUNE_LAZY_STAGE = 22, /* lazy backward: 0 the group's rows staged with 16-byte loads (default), 1 a dword gather per interior element (bitwise the same) */
       TCR_TUNE_FE_KERNEL = 23,  /* packed-FP32 front-end: 0 the three-waves-per-SIMD kernel (frontend_pk3.hip: wave-local LDS regions, <= 168 registers; default), 1 the two-waves kernel of rounds 2-4 (frontend_pk.hip; also what filterbanks with more work items than the unrolled trips fall back to). Bitwise the same features. */
       TCR_TUNE_FE_STAGGER = 24, /* three-waves front-end: one-off start-up delay of (workgroup generation * 4 + wave) * value * 64 cycles that de-phases the twelve waves of a CU (0: none) */
       TCR_TUNE_PW_WGRAD = 25,   /* wide pointwise (DS-CNN 172 / 276 channels) filter gradient: 0 the register-staged kernel (two 4-wave workgroups per CU; on 13 x 5 maps its unrolled form with fixed staging roles, round 5; default), 1 the DMA-staged kernel (global_load_lds into two LDS buffers, one 12-wave workgroup per CU, three split-K wave groups; measured 2 % slower), 2 the register-staged kernel's run-time-shape form on every map (rounds 4-5; bitwise the default) */
       TCR_TUNE_DEPLOY_F32 = 26, /* deploy-path MFCC (method 2): 0 the float64 kernel (one workgroup per frame; TF's ops compute in double; default), 1 the float32 throughput kernels with the op's filterbank / log floor (rounds 3-4: up to 0.5 off on noise-free tones, where the empty bands are pure round-off) */
       TCR_TUNE_NET_SMALL = 27,  /* eval network, TCResNet8-1.0 at 49 frames, batches of <= 64 utterances: 0 the small-batch kernel (one utterance per 8-wave workgroup, each phase's weights DMA-copied into LDS one phase ahead; default), 1 the throughput kernel at one utterance per group (rounds 2-4).  Bitwise the same outputs. */
       TCR_TUNE_PW_POS = 28,     /* wide pointwise convs (DS-CNN-L, 276 channels; forward, data gradient): 0 the nine-tile kernel built for <= 128 registers = four waves per SIMD, its weight chunks copied global -> LDS by the DMA path and its LDS fragment reads one step ahead of the MFMAs (default since round 5), 1 the unconstrained build of rounds 3-4 (92 VGPRs + 72 AGPRs, three waves per SIMD, register-staged weights), 2 the <= 128-register build with register-staged weights.  Bitwise the same results. */
       TCR_TUNE_BN_APPLY = 29,   /* BN-backward apply passes: 0 four float4 per thread and operand, per-channel coefficients staged in LDS (large tensors, DS-CNN: default since round 5; the finalize-folded pass of the TC-ResNet chain, bn_bwd_apply_fused_kernel: round 6), 1 the one-float4-per-thread loops of rounds 2-5.  Bitwise the same dy. */
       TCR_TUNE_DW_DGRAD = 30,   /* DS-CNN depthwise data gradient, stride-1 units on 13 x 5 maps: 0 the row kernel (dz / raw / dx blocks of 16 planes as contiguous float4 through LDS, one lane per map row; default since round 5), 1 the zero-padded-image kernel of rounds 2-4.  Bitwise the same dx and backward sums. */
       TCR_TUNE_DW_WGRAD = 31,   /* DS-CNN depthwise filter gradient, stride-1 units on 13 x 5 maps: 0 the row kernel (a wave owns four channels, their x / dz planes as contiguous float4 through wave-private LDS; default since round 5), 1 the gather kernel of rounds 2-4 (another summation order: equal to rounding). */
       TCR_TUNE_DW_FWD = 32,     /* DS-CNN depthwise conv (eval and training forward), stride-1 layers on 13 x 5 maps: 0 the row kernels (x / y blocks of 16 planes as contiguous float4 through LDS; also the global pooling's block-copy kernel and the row-per-lane stencil of the fused conv_1 + depthwise eval kernel; default since round 5), 1 the zero-padded-image kernels of rounds 2-4.  Bitwise the same outputs and statistics. */
       TCR_TUNE_WGRAD_PIPE = 33, /* 16-byte-load filter gradients (conv_wgrad_mfma4_kernel): 0 software-pipelined -- the operands of a wave's NEXT trip (the next 16 / 8 positions, or the next utterance's first) are requested before the current trip's MFMAs, two register sets alternating (round 6; bitwise the old kernel: same trips, same order; default), 1 every trip loads, waits, multiplies (rounds 3-5) */
       TCR_TUNE_COMPOSE_RUN = 34, /* tcr_compose: tiles of TCR_COMPOSE_TILE packed samples a workgroup composes one after the other, the recording and placement positions carried from tile to tile (0: default 4; 1: every tile finds them by binary search).  Bitwise the same output. */
       TCR_TUNE_COUNT = 35 };
int tcr_tune(int knob, int value);

/* Host-side view of how the fused eval kernel's resident-weight layers deal their work (no launch): the run of wave `wave` of `nw` in a
 * layer of `nrt` row tiles (16 output channels) x `nt16` column tiles (16 positions).  out3 = {row tile, first column, end column}: the
 * wave's units are (row tile, c) for first <= c < end, all in ONE row tile.  0, or -1 on bad arguments (nw not a multiple of nrt). */
int tcr_fused_deal_run(int nrt, int nt16, int nw, int wave, int* out3);

/* Host-side view of the fused eval kernel's TIME-MAJOR plan (TCR_TUNE_NET_FUSED, arm 0 / 12), no launch.
 * tcr_fused_tm_taps: the taps of a (k, stride, SAME padding pad_lo) layer over `tin` frames that read a real input frame for output
 *   tile `tile` (frames 2 * tile, 2 * tile + 1): out2 = {first, last}; the other taps are skipped for that tile.  0, or -1.
 * tcr_fused_tm_deal: the jobs of wave `wave` of `nw` in such a layer of `cin` -> `cout` channels, written to jobs[0 .. return value)
 *   (cap >= 8) as  row tile | first column tile << 4 | two tiles << 10 | first tap << 11 | last tap << 15;  *mfma (may be NULL): matrix
 *   instructions the layer issues per group of 8 utterances.  -1 on bad arguments or a layer the table does not hold.
 * tcr_net_fused_plan: what tcr_net_forward_infer would launch for `batch` utterances under the current knobs: out = {time-major,
 *   utterances per group, waves per workgroup, LDS bytes per workgroup, workgroups per CU, layers L, then per layer: floats per
 *   utterance (time-major: per channel) of its output / input / shortcut rows, stride of the layer that reads its output (0: none)}.
 *   Returns the ints written (6 + 4 L <= cap), 0 when the fused kernel does not take this net, -1 on bad arguments. */
int tcr_fused_tm_taps(int k, int stride, int tin, int pad_lo, int tile, int* out2);
int tcr_fused_tm_deal(int k, int stride, int cin, int cout, int tin, int pad_lo, int nw, int wave, unsigned* jobs, int cap, int* mfma);
int tcr_net_fused_plan(const tcr_net* net, int batch, int* out, int cap);

/* The library's internal streams (hipStream_t), one set per device and process.  HIP multiplexes streams onto a few hardware queues
 * and streams that share a queue serialise; the set is chosen on first use -- candidates are probed -- so that streams 0, 1, 2 and
 * `caller_stream` (the stream the host launches on; it is synchronised a few times by that first call) run concurrently, and stream 3
 * runs concurrently with `caller_stream` and stream 2.  0 / 1: the backward's filter gradients, used internally.  2: for the host's
 * input stage (the next batch's front-end next to a training step: the reference's tf.data prefetch, datasets/data_wrapper_base.py:70-76).
 * 3: for the network of a two-stream inference pipeline whose front-end runs on 2.  NULL on failure or idx outside 0..3. */
void* tcr_internal_stream(int idx, void* caller_stream);

#ifdef __cplusplus
}
#endif
#endif /* TCRESNET_HIP_H */
