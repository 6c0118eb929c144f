/*
 * alphapig_hip.h -- C ABI of libalphapig_hip.so: the batched policy-value evaluator on
 * hand-written gfx950 (MI355X / CDNA4) HIP kernels.
 *
 * Plain C: pointers and sizes only.  "dev" pointers are device (HBM) addresses, "host"
 * pointers ordinary or pinned host memory.  One engine = one device + one HIP stream; an
 * engine is not thread-safe.  int-returning calls return >= 0 on success, a negative
 * APZ_E_* code on failure (text: apz_last_error()).  No exceptions cross the boundary.
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   PolicyValueNet.__init__ / create_policy_value_predict / set_params
 *                                   policy_value_net_mxnet.py:21-38, :214-230
 *   network graph (stem, residual blocks, heads)      policy_value_net_mxnet.py:70-102
 *                                                     policy_value_net_mxnet_simple.py:68-92
 *   PolicyValueNet.policy_value (batched forward)     policy_value_net_mxnet.py:232-242
 *   PolicyValueNet.policy_value_fn (H2D, forward, D2H) policy_value_net_mxnet.py:261-280
 *   Board.current_state (plane encoding, done on device from compact codes) game.py:68-94
 *   TrainPipeline.get_equi_data (8-fold dihedral augmentation) train_mxnet.py:115-135
 *   SoftmaxActivation of the policy head (over all cells; opt-in over the empty cells only:
 *   apz_set_legal_policy, apz_pv_loss_legal)          policy_value_net_mxnet.py:90
 */
#ifndef ALPHAPIG_HIP_H
#define ALPHAPIG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APZ_OK 0
#define APZ_E_ARG (-1)
#define APZ_E_HIP (-2)       /* a HIP runtime call failed                        */
#define APZ_E_STATE (-3)     /* e.g. forward before weights were loaded           */
#define APZ_E_UNSUPPORTED (-4)

#define APZ_NET_RESNET 0     /* policy_value_net_mxnet.py        */
#define APZ_NET_SIMPLE 1     /* policy_value_net_mxnet_simple.py */

/* kernel classes for apz_kernel_time_ms (framed engines, see apz_create: APZ_K_STEM includes the framing kernel and the
 * stem's clear, APZ_K_TRUNK the clears behind the trunk convolutions, counted with their layers) */
#define APZ_K_STEM 0
#define APZ_K_TRUNK 1
#define APZ_K_HEAD_CONV 2
#define APZ_K_HEAD_FC 3
#define APZ_K_ENCODE 4
#define APZ_K_FORWARD 5   /* one whole forward (stem .. value head): EVERY forward while profiling is on, not only the sampled ones */
#define APZ_K_COUNT 6

typedef struct apz_engine apz_engine;

typedef struct apz_config {
    int32_t height;     /* board_height                                                 */
    int32_t width;      /* board_width                                                  */
    int32_t c_in;       /* input planes: 9 (channelnum, policy_value_net_mxnet.py:24) or 4 */
    int32_t n_filter;   /* trunk width (resnet), policy_value_net_mxnet.py:21           */
    int32_t n_blocks;   /* residual blocks (resnet)                                     */
    int32_t net_kind;   /* APZ_NET_*                                                    */
    int32_t max_batch;  /* largest n accepted by forward calls                          */
    int32_t device;     /* HIP device ordinal                                           */
} apz_config;

const char *apz_last_error(void);
int apz_version(void);
int apz_device_count(void);

/* Boards: 15x15 and 8x8 (either net, 64 / 128 / 256 filters) have kernels of their own.  Every other square board of side
 * S in 6 .. 14 except 10 is a "framed" engine (csrc/frame15.h): the residual net with 128 filters, c_in 9 or 4, computed by the 15x15
 * trunk kernels on a 15x15 frame that holds the board in its top-left S x S window; the off-board cells of every
 * activation are zeroed after each layer, so the results are those of the S x S net.  Every interface below speaks S x S
 * (planes [n][c_in][S][S], codes of stride (S*S + 1 + 15) / 16 * 16, S*S probabilities); all inference entry points, the
 * arithmetics, apz_set_trunk_uniform, the activation exponents and the HIP-graph replay work as at 15x15.  The training
 * entry points (apz_conv3x3_fwd, apz_wino_*, apz_layout_convert, ...) stay 15x15 / 8x8 only; the training step of a
 * framed board runs on a 15x15 engine through them and the apz_*_frame entry points below, which take the side explicitly.
 * APZ_E_UNSUPPORTED (NULL, message in apz_last_error): non-square boards, S < 6, S > 15, 10x10, and at a framed size the simple net
 * or 64 / 256 filters. */
apz_engine *apz_create(const apz_config *cfg);
void apz_destroy(apz_engine *e);

/* Parameter table (MXNet names, policy_value_loss.json): name and element count. */
int apz_param_count(apz_engine *e);
const char *apz_param_name(apz_engine *e, int i);
int64_t apz_param_size(apz_engine *e, int i);
/* Load RAW parameters (conv weight/bias, BN gamma/beta/moving stats, FC weight/bias) from
 * host float32 arrays; every table entry must be supplied.  BatchNorm (eps 1e-3,
 * fix_gamma semantics per layer) is folded into conv weights/biases inside.
 * Synchronous: drains the engine's stream, copies the tensors into an engine-owned staging buffer in device memory, folds
 * and packs them there with the kernels apz_load_weights_dev runs (csrc/weights_pack.h: one implementation, the same
 * bits from both), and returns when the weights are in place.  The first call allocates the packed buffers and the
 * staging buffer for the engine's configuration (apz_set_trunk_arith comes before it); later calls allocate nothing. */
int apz_load_weights(apz_engine *e, const char *const *names, const float *const *host_ptrs,
                     const int64_t *sizes, int n);

/* Batched forward on the engine's stream, asynchronous.  planes_dev [n][c_in][H][W] f32.
 * probs_dev [n][H*W], values_dev [n]; logits_dev / vlogits_dev (pre-softmax / pre-tanh)
 * may be NULL. */
int apz_forward(apz_engine *e, const void *planes_dev, int n, void *probs_dev, void *values_dev,
                void *logits_dev, void *vlogits_dev);
/* Host-buffer convenience (H2D, forward, D2H, sync): policy_value / policy_value_fn path. */
int apz_forward_host(apz_engine *e, const float *planes_host, int n, float *probs_host,
                     float *values_host);
/* Self-play path: compact position codes (include/alphapig_host.h, apzh_code_stride bytes
 * per leaf) H2D, planes encoded on device, forward, D2H, sync. */
int apz_forward_codes_host(apz_engine *e, const uint8_t *codes_host, int n, float *probs_host,
                           float *values_host);
/* Asynchronous halves of the same, for overlapping host tree work with the GPU: buffers
 * must be pinned (apz_host_alloc) and stay valid until apz_sync() returns. */
int apz_forward_codes_async(apz_engine *e, const uint8_t *codes_pinned, int n, float *probs_pinned,
                            float *values_pinned);
/* Stream-ordered queue of up to APZ_MAX_SLOTS batches on the engine's ONE stream: submit copies
 * the codes into the slot's pinned buffer and enqueues H2D, encode, forward, D2H and an event;
 * wait blocks on that event and copies the slot's results out.  A second batch submitted while
 * the first runs starts the moment the first one's last kernel ends (no host round trip in
 * between).  submit calls are serialised by an internal lock; different slots may be submitted
 * and waited from different host threads.  A batch is answered with the weights installed when it
 * was submitted, whatever is installed before the wait (tests/test_gpu_weight_versions.py), with one
 * exception: an APZ_ARITH_F16X2 batch that overflowed is repeated by apz_wait on the exact-fp32 kernel
 * with the weights installed at the time of the WAIT, not those it was submitted under. */
#define APZ_MAX_SLOTS 4
int apz_submit_codes(apz_engine *e, int slot, const uint8_t *codes_host, int n);
int apz_wait(apz_engine *e, int slot, float *probs_host, float *values_host);
void *apz_host_alloc(int64_t bytes);   /* pinned host memory */
void apz_host_free(void *p);

/* codes_dev [n][stride] u8 -> planes_dev [n][n_planes][H][W] f32 (n_planes 9 or 4). */
int apz_encode_planes(apz_engine *e, const void *codes_dev, int n, int n_planes, void *planes_dev);
/* 8-fold dihedral augmentation, reference order r1, r1f, r2, r2f, r3, r3f, id, idf:
 * planes_dev [n][c][H][W], pi_dev [n][H*W] -> planes_out_dev [n*8][c][H][W], pi_out_dev [n*8][H*W]. */
int apz_augment8(apz_engine *e, const void *planes_dev, const void *pi_dev, int n, int c,
                 void *planes_out_dev, void *pi_out_dev);

/* Root move sampling on the GPU (opt-in; NOT bit-compatible with the reference's NumPy stream):
 * visits_host [g][H*W] int32 with -1 where the root has no child; pi_host [g][H*W] gets
 * softmax(log(visits+1e-10)/temp) (mcts_alphaZero.py:152-155), moves_host[g] a draw from
 * (1-eps)*pi + eps*Dirichlet(alpha) (:198-201).  Deterministic in (seed, step, game index).
 * Accuracy of pi: within 1e-6 absolute of that softmax evaluated in float64, at every temperature and however close the
 * leading children are (the kernel works from v / v_max with v - v_max taken in integers), on condition that every
 * visit count is below 2^24 (counts convert to float exactly).  A child without visits beside a visited one gets the
 * reference's weight (below 1e-10 at temp <= 1); a row whose children all have 0 visits is uniform over them.
 * A row without any child (all -1): pi all zero, move -1, nothing non-finite; the other rows are unaffected. */
int apz_sample_moves_host(apz_engine *e, const int32_t *visits_host, int g, float temp, float alpha,
                          float eps, uint64_t seed, uint64_t step, float *pi_host, int32_t *moves_host);
/* The same with one caller-chosen 64-bit key per row instead of (step, row): the draw of row i depends on
 * (seed, keys_host[i]) only.  The self-play engine passes (global game index << 20 | ply), so a game's noise is
 * reproducible whatever batch, rank or step it is sampled in (the reference's per-game reproducibility comes from
 * np.random.seed before a game, mcts_alphaZero.py:198-201).  keys_host == NULL: as apz_sample_moves_host. */
int apz_sample_moves_keyed_host(apz_engine *e, const int32_t *visits_host, int g, float temp, float alpha,
                                float eps, uint64_t seed, uint64_t step, const uint64_t *keys_host,
                                float *pi_host, int32_t *moves_host);

/* ---- training-side convolution primitives (hand-written forward, data- and
 * weight-gradient of the 3x3 convolutions, callable on caller-owned dense NCHW float32 device
 * tensors, e.g. from a torch.autograd.Function).  `stream` = the hipStream_t to launch on (NULL is
 * the null stream, which is what torch.cuda.current_stream().cuda_stream reports by default);
 * APZ_ENGINE_STREAM selects the engine's own stream.  The training entry points share per-engine scratch buffers: calls on
 * one stream are ordered by it, and a call on a DIFFERENT stream than the previous one is ordered (event + stream wait)
 * behind everything that was queued on the previous stream -- one engine never works on two streams at once.
 * Supported: boards 15x15 and 8x8; packed C_out in {64, 128, 256}.
 *   apz_conv3x3_pack   w_dev [cout][cin][3][3] -> wpk_dev (apz_conv3x3_packed_size floats);
 *                      transpose_flip=1 packs the weights of the data-gradient convolution
 *                      dX = conv(dY, W'), W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]
 *   apz_conv3x3_fwd    y = conv(x, wpk) (+ bias_dev if not NULL) (ReLU if relu); channels are
 *                      those of the PACKED convolution (cin_p inputs, cout_p outputs)
 *   apz_conv3x3_wgrad  dw_dev [cout][cin][3][3] = sum_b x_b (*) dy_b (overwritten) */
#define APZ_ENGINE_STREAM ((void *)(intptr_t)-1)
int64_t apz_conv3x3_packed_size(int cin_p, int cout_p);
int apz_conv3x3_pack(apz_engine *e, const void *w_dev, int cin, int cout, int transpose_flip,
                     void *wpk_dev, void *stream);
int apz_conv3x3_fwd(apz_engine *e, const void *x_dev, const void *wpk_dev, const void *bias_dev,
                    void *y_dev, int n, int cin_p, int cout_p, int relu, void *stream);
/* The forward convolution on the fp16 matrix pipe with two-term operands (csrc/conv15_split.h; 15x15 boards, cin a multiple
 * of 64, cout a multiple of 16, APZ_E_UNSUPPORTED otherwise): y = conv(x, w) (+ bias_dev if not NULL) (+ resid_dev if not
 * NULL) (ReLU if relu) on dense tensors x [n][cin][15][15], y / resid [n][cout][15][15]; w_dev = the raw fp32 weights
 * [cout][cin][3][3], split and packed into engine scratch by the evaluator's packing kernel in front of the launch.
 * flag_dev: a device word the kernel sets to 1 -- never clears -- when a sum in front of the ReLU is not finite (an input
 * beyond 65 504 in magnitude). */
int apz_conv15h_fwd(apz_engine *e, const void *x_dev, const void *w_dev, const void *bias_dev,
                    const void *resid_dev, void *y_dev, int n, int cin, int cout, int relu,
                    void *flag_dev, void *stream);
/* The training step of the generic 15x15 nets on the same kernel (HipTrainer(trunk_arith="f16x2") on nets without the
 * padded-row trunk; csrc/conv15_split.h).  Dense tensors, C_in and C_out multiples of 64.
 *   apz_conv15h_packed_size  floats of one orientation's packed weights of a cin -> cout layer (9 cin cout); beside them an
 *                            orientation has bias8h = [its output channels: bias][as many: 1 / S] floats.
 *   apz_conv15h_pack_many    one launch for the step's `count` layers, both orientations each.  table_host: `count` entries
 *                            of struct apz_conv15h_pack_entry, 56 bytes each, read before the call returns.  Orientation 0 = the forward
 *                            (bit for bit what apz_conv15h_fwd packs per call), orientation 1 = the data gradient
 *                            (W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx], bias zero); the per-channel scale S is taken over
 *                            the orientation's own output channel.  flag_dev (NULL: none): a 32-bit word zeroed by the launch.
 *   apz_conv15h_fwd_packed   y = conv(x) + bias (+ resid_dev; NULL: none), no ReLU, on orientation 0 of a packed layer; a
 *                            non-finite sum sets *flag_dev = 1.
 *   apz_conv15h_dgrad        dx [n][c_dx][15][15] = conv(dy [n][c_dy][15][15], W') (+ add_dev; NULL: none) on orientation 1
 *                            of a packed layer (pk / bias8h of c_dy -> c_dx).  dymax_dev: dymax_count >= 1 partial maxima of
 *                            |dy| (apz_bn_bwd_max's dxmax) -- the launch scales dy by 2^a with the maximum in [2^7, 2^8)
 *                            before the fp16 split, as apz_wino3h_conv_dgrad does (NaN entries are ignored, a zero maximum
 *                            gives a = 0); flag_dev as above, also set when an entry of dymax_dev is +inf. */
typedef struct apz_conv15h_pack_entry {
    const float *w;             /* [cout][cin][3][3] fp32, device */
    const float *bias;          /* [cout], device; NULL: zero */
    void *pk[2];                /* apz_conv15h_packed_size(cin, cout) floats each, device, 16-byte aligned */
    float *bias8h[2];           /* [2 cout] and [2 cin] floats, device */
    int cin, cout;
} apz_conv15h_pack_entry;
int64_t apz_conv15h_packed_size(int cin, int cout);
int apz_conv15h_pack_many(apz_engine *e, const void *table_host, int count, void *flag_dev, void *stream);
int apz_conv15h_fwd_packed(apz_engine *e, const void *x_dev, const void *pk_dev, const void *bias8h_dev,
                           const void *resid_dev, void *y_dev, int n, int cin, int cout, void *flag_dev, void *stream);
int apz_conv15h_dgrad(apz_engine *e, const void *dy_dev, const void *pk_dev, const void *bias8h_dev, const void *add_dev,
                      void *dx_dev, int n, int c_dy, int c_dx, const void *dymax_dev, int dymax_count, void *flag_dev,
                      void *stream);
/* activation layouts of the training primitives: dense NCHW, or the trunk's padded rows [n][C][15][16]
 * (15x15 boards; pad column zero) in which the self-play kernels keep their activations */
#define APZ_LAYOUT_DENSE 0
#define APZ_LAYOUT_ROWS16 1
int apz_conv3x3_wgrad(apz_engine *e, const void *x_dev, const void *dy_dev, void *dw_dev, int n,
                      int cin, int cout, int layout, void *stream);
/* The same forward / data-gradient convolution for the trunk shape (128 -> 128 channels, 15x15) on the
 * fused Winograd F(4x4,3x3) kernel of the self-play path (csrc/trunk15_wino3.h, csrc/wino_common.h):
 *   apz_wino_pack   w_dev [128][128][3][3] -> upk_dev (apz_wino_packed_size floats), U = G g G^T in fp32
 *                   on the device; transpose_flip as in apz_conv3x3_pack
 *   apz_wino_conv   y = conv(x, upk) + bias_dev (NULL: none) (ReLU if relu), x / y dense [n][128][15][15]
 *                   (copied to / from the kernel's padded-row layout in engine-owned scratch) */
int64_t apz_wino_packed_size(void);
int apz_wino_pack(apz_engine *e, const void *w_dev, int transpose_flip, void *upk_dev, void *stream);
/* ... of `count` layers whose weights lie back to back (w_dev [count][128][128][3][3]) in both orientations, one launch:
 * upk_dev [count][2][apz_wino_packed_size()] (forward, data gradient).  A training step packs every trunk layer twice
 * (policy_value_net_mxnet.py:282-299: the weights change with every optimiser step). */
int apz_wino_pack_many(apz_engine *e, const void *w_dev, int count, void *upk_dev, void *stream);
int apz_wino_conv(apz_engine *e, const void *x_dev, const void *upk_dev, const void *bias_dev,
                  void *y_dev, int n, int relu, int layout, void *stream);
/* ... + resid_dev (padded-row layout only; NULL: none) before the ReLU: the data gradient of a residual block's first
 * convolution meets the skip gradient inside the kernel's epilogue (trunk15_wino3.h) */
int apz_wino_conv_add(apz_engine *e, const void *x_dev, const void *upk_dev, const void *bias_dev,
                      const void *resid_dev, void *y_dev, int n, int relu, int layout, void *stream);
/* The training forward of a trunk layer (policy_value_net_mxnet.py:41-56: Convolution, then BatchNorm): y = conv(x, upk)
 * + bias in the padded-row layout, and stats_dev [128][n][2] doubles = per (channel, board) the sum and the sum of
 * squares of the board's 225 outputs, taken in the kernel's epilogue.  apz_bn_fwd_stats = apz_bn_fwd that takes its
 * batch statistics from such a buffer (stats_dev NULL: computes them itself) instead of a pass over x.  mask_dev (NULL:
 * not wanted; padded-row layout): n * C * 60 bytes, bit e of byte i = [element 4 i + e of y > 0] -- apz_bn_bwd reads the
 * ReLU decisions from it instead of from the 16-times-larger y. */
int apz_wino_conv_stats(apz_engine *e, const void *x_dev, const void *upk_dev, const void *bias_dev, void *y_dev,
                        void *stats_dev, int n, void *stream);
/* The training step's trunk on the f16x2 kernel (trunk15_wino3h16.h; HipTrainer(trunk_arith="f16x2")).
 *   apz_wino3h_pack_many   w_dev [count][128][128][3][3] fp32, b_dev [count][128] (NULL: zero) -> upk_dev
 *                          [count][2][apz_wino3h_packed_size() floats] and bias_dev [count][2][256] floats (forward, data
 *                          gradient), U in double, no BatchNorm fold: per output channel S = 2^k, U S as two fp16 terms,
 *                          bias = [128 biases (the data gradient's: 0)][128 x 1 / S].  flag_dev (NULL: none): a 32-bit
 *                          word zeroed by this launch.
 *   apz_wino3h_conv_stats  apz_wino_conv_stats' contract (y [n][128][15][16] = conv + bias, stats_dev double [128][n][2])
 *                          on the f16x2 kernel; a non-finite output sets *flag_dev = 1 (the step is then repeated on the
 *                          exact kernels).
 *   apz_wino3h_conv_dgrad  dx = conv(dy, W') (+ add_dev; NULL: none), every tensor [n][128][15][16]; dymax_dev: dymax_count
 *                          partial maxima of |dy| (apz_bn_bwd_max's dxmax) -- the launch scales dy by 2^a with the maximum
 *                          in [2^7, 2^8) before the fp16 split (-64 <= a <= 110: maxima down to 1e-31 reach that
 *                          window; NaN entries are ignored); flag_dev as above, also set when an entry of dymax_dev
 *                          is +inf.
 *   apz_bn_bwd_max         apz_bn_bwd (padded rows, or dense 15x15 tensors) + dxmax_dev [apz_bn_bwd_splits(n, C, layout)][C] floats: max |dx|
 *                          per batch split and channel (NULL: apz_bn_bwd's launches and bits).
 *   apz_adam_step_unless   apz_adam_step, skipped on the device when the 32-bit word at skip_dev is not zero. */
int64_t apz_wino3h_packed_size(void);
int apz_wino3h_pack_many(apz_engine *e, const void *w_dev, const void *b_dev, int count, void *upk_dev, void *bias_dev,
                         void *flag_dev, void *stream);
int apz_wino3h_conv_stats(apz_engine *e, const void *x_dev, const void *upk_dev, const void *bias_dev, void *y_dev,
                          void *stats_dev, int n, void *flag_dev, void *stream);
int apz_wino3h_conv_dgrad(apz_engine *e, const void *dy_dev, const void *upk_dev, const void *bias_dev, const void *add_dev,
                          void *dx_dev, int n, const void *dymax_dev, int dymax_count, void *flag_dev, void *stream);
int apz_bn_fwd_stats(apz_engine *e, const void *x_dev, const void *resid_dev, const void *gamma_dev,
                     const void *beta_dev, void *run_mean_dev, void *run_var_dev, void *y_dev, void *mean_dev,
                     void *invstd_dev, const void *stats_dev, void *mask_dev, int n, int C, int layout, int relu,
                     float momentum, float eps, void *stream);
/* Training-mode BatchNorm (+ residual) (+ ReLU), the reference's BatchNorm(eps = 1e-3) between the trunk's
 * convolutions (policy_value_net_mxnet.py:41-102), over n x C planes in `layout`:
 *   apz_bn_fwd  y = act((x - mean_c) * invstd_c * gamma_c + beta_c (+ resid)); batch statistics (biased
 *               variance) written to mean_dev / invstd_dev [C] for the backward pass; run_mean / run_var
 *               (may be NULL) updated as run = (1 - momentum) * run + momentum * batch (unbiased variance);
 *               gamma_dev NULL = 1 (the reference's fix_gamma layers)
 *   apz_bn_bwd  dz = dy (* [out > 0] with relu: from out_dev, or from mask_dev when given -- then out_dev may be NULL);
 *               dbeta = sum dz; dgamma = sum dz * xhat;
 *               dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M); dres = dz (NULL: not wanted);
 *               dxsum_dev (NULL: not wanted): [apz_bn_bwd_splits(n, C, layout)][dxsum_ld] floats, dxsum_ld >= C;
 *               row s, column c gets the sum of channel c's dx over the boards of batch split s.  The column
 *               sums (apz_colsum) are the bias gradient of the convolution that produced x; a caller with
 *               several layers gives each its own C columns of one matrix and adds them all in one launch.
 * Channel sums: double precision, per (channel, batch split) partials (no atomics) that every consumer workgroup
 * adds in a fixed order (csrc/conv_train.h; the padded-row passes: csrc/bn_frame.h) -- two launches per call, the same bits
 * on every run.  The training entry points share per-engine scratch: calls on one engine must be ordered by ONE stream at a
 * time.
 *   apz_colsum  out[j] = scale * sum_i in[i][j] over rows x cols floats, fixed order (double accumulation) */
int apz_bn_fwd(apz_engine *e, const void *x_dev, const void *resid_dev, const void *gamma_dev,
               const void *beta_dev, void *run_mean_dev, void *run_var_dev, void *y_dev, void *mean_dev,
               void *invstd_dev, int n, int C, int layout, int relu, float momentum, float eps, void *stream);
/* Weight gradient of the trunk shape (128 -> 128, 15x15) through the Winograd domain (csrc/wgrad_wino3.h; 3.6x fewer
 * MFMAs than apz_conv3x3_wgrad): x_dev / dy_dev in the padded-row layout [n][128][15][16], dw_dev [128][128][3][3]
 * overwritten. */
int apz_wgrad_wino(apz_engine *e, const void *x_dev, const void *dy_dev, void *dw_dev, int n, void *stream);
/* The same weight gradient with the per-position products on the fp16 matrix pipe (csrc/wgrad_wino3h.h): both
 * transformed operands as two fp16 terms (hi + lo, round to nearest even), fp32 accumulation, the same slice scratch
 * and finish kernel as apz_wgrad_wino, the same bits on every run.
 *   scale     dymax_dev: dymax_count >= 1 floats whose largest magnitude is max |dy| (what apz_bn_bwd_max leaves in
 *             dxmax_dev; as apz_wino3h_conv_dgrad).  The launch multiplies dy by 2^a, a chosen on the device so that
 *             max |dy| 2^a lies in [2^6, 2^7): the transformed gradient stays below 225 * 2^7 = 28 800 < 65 504 and
 *             cannot overflow on finite input; a = 0 for an all-zero dy, -64 <= a <= 110; 2^-a is applied to the result.
 *   overflow  the transformed activations are not scaled (|V| <= 100 max |x|).  The 32-bit word at flag_dev (may be
 *             NULL) is set to 1 when a partial result is not finite, an activation exceeds 655 (where that bound
 *             leaves the fp16 range) or an entry of dymax_dev is +inf; the call never clears it, and dw_dev of a
 *             call that sets it is unspecified. */
int apz_wgrad_wino_f16x2(apz_engine *e, const void *x_dev, const void *dy_dev, void *dw_dev, int n,
                         const void *dymax_dev, int dymax_count, void *flag_dev, void *stream);
/* One optimiser step of the reference's Adam (policy_value_net_mxnet.py:198-205: rescale_grad = 1/batch_size,
 * wd on *_weight / *_gamma) over ntensors device tensors in ONE launch.  table_host: ntensors entries
 * { float *w; const float *g; float *m; float *v; int64 n; float wd; int32 pad; } (48 bytes) in HOST memory;
 * g = g * rescale + wd * w; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g*g; w -= lr_t * m / (sqrt(v) + eps),
 * lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) computed by the caller. */
int apz_adam_step(apz_engine *e, const void *table_host, int ntensors, float lr_t, float b1, float b2,
                  float eps, float rescale, void *stream);
int apz_bn_bwd(apz_engine *e, const void *dy_dev, const void *x_dev, const void *out_dev, const void *mask_dev,
               const void *gamma_dev, const void *mean_dev, const void *invstd_dev, void *dx_dev,
               void *dres_dev, void *dgamma_dev, void *dbeta_dev, void *dxsum_dev, int dxsum_ld, int n, int C,
               int layout, int relu, void *stream);
int apz_bn_bwd_max(apz_engine *e, const void *dy_dev, const void *x_dev, const void *out_dev, const void *mask_dev,
                   const void *gamma_dev, const void *mean_dev, const void *invstd_dev, void *dx_dev, void *dres_dev,
                   void *dgamma_dev, void *dbeta_dev, void *dxsum_dev, int dxsum_ld, void *dxmax_dev, int n, int C,
                   int layout, int relu, void *stream);
int apz_adam_step_unless(apz_engine *e, const void *table_host, int ntensors, float lr_t, float b1, float b2,
                         float eps, float rescale, const void *skip_dev, void *stream);
/* The guarded optimiser step (csrc/grad_guard.h; HipTrainer(step_guard=True, clip_norm=...)): the global norm of the
 * gradients in the Adam table, global-norm clipping and a refusal of non-finite steps, decided on the device.
 *   apz_grad_norm          two launches over the table's g tensors (w, m, v are not read): per-workgroup sums of squares in
 *                          double (no atomics, a fixed order: the same bits on every run and for every alignment of g), then
 *                          one workgroup that writes the 16-byte record at record_dev (16-byte aligned).  The order, for a
 *                          reader who wants the bits: grid (32, ntensors) x 256 threads; thread j of workgroup b of tensor t
 *                          adds the squares of elements 4 q .. 4 q + 3, q = 256 b + j, + 8192, ..., in index order; the
 *                          workgroup's 256 sums go through a 64-lane shuffle tree (offsets 32, 16, .., 1) and the four
 *                          wave sums are added in wave order; the fold adds tensor t's 32 workgroup sums in index order
 *                          and then the ntensors tensor sums in index order (two levels, not one chain over all 32 *
 *                          ntensors partials).  The record:
 *                            { float norm; float rescale_eff; uint32 skip; uint32 why; }
 *                          norm = sqrt(sum g^2) * rescale (the float64 value rounded once);
 *                          why: bit 1  a gradient element is not finite
 *                               bit 2  one of the three floats at loss3_dev (NULL: not looked at) is not finite
 *                               bit 4  the 32-bit word at skip_in_dev (NULL: none; the f16x2 overflow word) is not zero
 *                               bit 8  clip > 0 and norm, finite in double, does not fit a finite float
 *                          skip = (why != 0);
 *                          rescale_eff = rescale when clip <= 0 or norm <= clip, else the fp32 product
 *                          rescale * (float)(clip / norm): the gradient scaled to norm `clip`.
 *   apz_adam_step_guarded  the same two launches and then apz_adam_step with rescale_eff in place of rescale -- nothing is
 *                          updated when skip is set.  A step that neither clips nor skips has apz_adam_step's bits.
 * Arguments are checked as apz_adam_step's; no stream synchronisation. */
int apz_grad_norm(apz_engine *e, const void *table_host, int ntensors, float rescale, float clip, const void *loss3_dev,
                  const void *skip_in_dev, void *record_dev, void *stream);
int apz_adam_step_guarded(apz_engine *e, const void *table_host, int ntensors, float lr_t, float b1, float b2, float eps,
                          float rescale, float clip, const void *loss3_dev, const void *skip_in_dev, void *record_dev,
                          void *stream);
/* The trainer's averaged weights (csrc/ema.h; HipTrainer(ema_decay=...)): one launch over ntensors pairs of device tensors,
 * grid (32, ntensors) x 256 like apz_adam_step.  table_host: ntensors entries { float *s; const float *w; int64 n; }
 * (24 bytes) in HOST memory -- s the shadow (the average), w the weight, n floats each.  Per element, for a reader who
 * wants the bits:
 *     d = w - s;  p = c * d;  s = s + p      three float32 operations, each rounded to nearest even on its own
 * never a fused multiply-add (the kernel is compiled with floating-point contraction off, by pragma and by the build's
 * -ffp-contract=off): the NumPy float32 expression s + c * (w - s) gives the same bits.  w == s leaves the value as
 * it is (w - s = +0).  Only s is written, element by element: s and w may start anywhere on the float grid.
 * skip_a_dev / skip_b_dev (each may be NULL): 32-bit device words; when either is not zero at the time the launch runs,
 * nothing is written (the f16x2 overflow word, or the skip word at byte 8 of apz_grad_norm's record -- the launch queued
 * behind an Adam launch skips exactly when that one did).  Arguments are checked as apz_adam_step's and the table travels
 * the same way, except that ntensors = 0 is accepted and launches nothing; no stream synchronisation. */
int apz_ema_update(apz_engine *e, const void *table_host, int ntensors, float c, const void *skip_a_dev,
                   const void *skip_b_dev, void *stream);
int apz_bn_bwd_splits(apz_engine *e, int n, int C, int layout);
int apz_colsum(apz_engine *e, const void *in_dev, void *out_dev, int rows, int cols, float scale, void *stream);

/* ---- heads and loss of the training graph (policy_value_net_mxnet.py:85-102, :173-193), csrc/heads_train.h.
 * All tensors float32 on the device; `layout` as above for the trunk-side tensors (x, dx); y / dy dense.
 *   apz_conv1x1_fwd / _bwd   the 1x1 head convolutions conv3_1_1 (C -> 4) and conv3_2_1 (C -> 2): y = W x + b;
 *                            dx (NULL: not wanted), dW [CO][C], db [CO] (NULL: not wanted); sums over the batch are
 *                            taken in index order (no float atomics)
 *   apz_fc_fwd / _bwd        FullyConnected: y[n][N] = x[n][K] W[N][K]^T + b; dx, dW, db (each may be NULL): one
 *                            fp32-MFMA GEMM kernel with operand strides
 *   apz_dropout              y = x * mask / keep, mask = [hash(seed, step, index) < keep]: the same call with dy gives
 *                            the backward pass (the mask is regenerated, not stored)
 *   apz_pv_loss              p = softmax(logits), v = tanh(vlogit); loss3 = (mean (z - v)^2, mean -sum pi log p,
 *                            mean -sum p log p); dlogits = (p sum(pi) - pi) / n, dvlogit = 2 (v - z)(1 - v^2) / n;
 *                            probs / values = p, v.  Every output pointer may be NULL.
 *   apz_layout_convert       dense [planes][15][15] <-> padded rows [planes][15][16]
 *   apz_bias_grad            db[c] = sum over boards and cells of dy[n][c][.] (the bias gradient of a convolution;
 *                            pad cells of a padded-row gradient are zero), fixed summation order
 *   apz_add                  y += x (count floats): the meeting point of the trunk and skip gradients
 * conv1x1_bwd: dx gets zero pad cells; accumulate_dx != 0 adds to what dx already holds (second head). */
/* apz_load_weights for tensors that already live in device memory (policy_value_net_mxnet.py:295-297: after an
 * optimiser step the new parameters go into the predict modules): the fold and pack kernels of apz_load_weights,
 * queued on `stream` without a copy and without a host synchronisation; forwards queued afterwards use the new weights.
 * Same name / size table, same checks and same resulting bits as apz_load_weights; the engine must have been loaded once
 * from the host (that call allocates the buffers this one fills). */
int apz_load_weights_dev(apz_engine *e, const char *const *names, const void *const *dev_ptrs, const int64_t *sizes,
                         int n, void *stream);
/* Device replay buffer (alphapig_amd/replay.py, csrc/replay.h): the ring keeps what the self-play exchange delivers --
 * codes_dev [capacity][code stride] u8, pi_dev [capacity][H*W] f32, z_dev [capacity] f32, one slot per tuple -- and a
 * mini-batch is gathered on the device.  entries_host [n] i32: slot * 8 + symmetry (the order of apz_augment8).
 * Sample j gets planes_out_dev [j][n_planes][H][W] = the planes apz_encode_planes writes for its slot, permuted like row
 * `symmetry` of apz_augment8; pi_out_dev [j][H*W] = that row's pi; z_out_dev [j] = z[slot] -- the same bits.  Queued on
 * `stream` (the entry words are copied in stream order; entries_host need not outlive the call).  APZ_E_UNSUPPORTED on a
 * non-square board; APZ_E_ARG for n_planes other than 9 / 4 or any entry outside [0, 8 * capacity), before anything is
 * copied or launched; n == 0 is APZ_OK. */
int apz_replay_gather(apz_engine *e, const void *codes_dev, const void *pi_dev, const void *z_dev, int64_t capacity,
                      const int32_t *entries_host, int n, int n_planes, void *planes_out_dev, void *pi_out_dev,
                      void *z_out_dev, void *stream);
/* apz_forward_host on planes that already live in device memory: the engine's stream is ordered behind everything queued
 * on `after_stream` so far (APZ_ENGINE_STREAM: nothing to wait for), runs the same forward and copies probs / values to
 * the host.  Same bits as apz_forward_host on the same planes; returns with the engine's stream drained. */
int apz_forward_dev_host(apz_engine *e, const void *planes_dev, int n, float *probs_host, float *values_host,
                         void *after_stream);
int apz_conv1x1_fwd(apz_engine *e, const void *x_dev, const void *w_dev, const void *bias_dev, void *y_dev, int n,
                    int C, int CO, int layout, void *stream);
int apz_conv1x1_bwd(apz_engine *e, const void *x_dev, const void *w_dev, const void *dy_dev, void *dx_dev,
                    void *dw_dev, void *db_dev, int n, int C, int CO, int layout, int accumulate_dx, void *stream);
/* ... of two 1x1 convolutions that share their input (the reference's two heads, policy_value_net_mxnet.py:85-96):
 * dx = W1^T dy1 + W2^T dy2 in one pass over x and dx; dw_dev [CO1 + CO2][C]: the first head's rows, then the second's. */
int apz_conv1x1_bwd2(apz_engine *e, const void *x_dev, const void *w1_dev, const void *dy1_dev, int CO1,
                     const void *w2_dev, const void *dy2_dev, int CO2, void *dx_dev, void *dw_dev, int n, int C,
                     int layout, int accumulate_dx, void *stream);
int apz_bias_grad(apz_engine *e, const void *dy_dev, void *db_dev, int n, int C, int layout, void *stream);
int apz_add(apz_engine *e, void *y_dev, const void *x_dev, int64_t count, void *stream);
int apz_fc_fwd(apz_engine *e, const void *x_dev, const void *w_dev, const void *bias_dev, void *y_dev, int n, int K,
               int N, void *stream);
int apz_fc_bwd(apz_engine *e, const void *x_dev, const void *w_dev, const void *dy_dev, void *dx_dev, void *dw_dev,
               void *db_dev, int n, int K, int N, void *stream);
int apz_dropout(apz_engine *e, const void *x_dev, void *y_dev, int64_t count, float keep, uint64_t seed,
                uint64_t step, void *stream);
int apz_pv_loss(apz_engine *e, const void *logits_dev, const void *vlogit_dev, const void *pi_dev, const void *z_dev,
                int n, void *loss3_dev, void *dlogits_dev, void *dvlogit_dev, void *probs_dev, void *values_dev,
                void *stream);
/* apz_pv_loss over the EMPTY cells of every board (the training side of apz_set_legal_policy; csrc/heads_train.h).
 * occ_dev [n][H*W] u8 in move order: byte m != 0 where move m is occupied (apz_occupancy_planes).  With E the empty cells
 * of a row: p = softmax of the logits over E (the maximum over E only), policy loss -sum_E pi log p, entropy -sum_E p log p,
 * dlogits = (p sum_E(pi) - pi) / n on E; probs and dlogits are exactly +0 on the occupied cells, and a row without an empty
 * cell has policy loss 0, entropy 0 and all-zero probs / dlogits.  An occupied cell is left out by selection: whatever its
 * logit holds (NaN, inf, the row's maximum) changes no output bit.  The kernel keeps the unmasked kernel's ownership of
 * cells by lanes and its reduction trees: with occ_dev all zero every output has apz_pv_loss's bits.  Value terms unchanged. */
int apz_pv_loss_legal(apz_engine *e, const void *logits_dev, const void *vlogit_dev, const void *pi_dev,
                      const void *z_dev, const void *occ_dev, int n, void *loss3_dev, void *dlogits_dev,
                      void *dvlogit_dev, void *probs_dev, void *values_dev, void *stream);
/* planes_dev [n][c_in][H][W] f32 (the planes of apz_encode_planes: top row first) -> occ_dev [n][H*W] u8 in move order
 * (m = h*W + w, bottom row first: the order of the position codes and of pi): 1 where cell (H-1-h, w) of the "all own
 * stones" or of the "all opponent stones" plane is non-zero -- planes 6 and 7 for c_in = 9, planes 0 and 1 for c_in = 4 --
 * else 0.  Any board size (the engine's own is not looked at); queued on `stream`. */
int apz_occupancy_planes(apz_engine *e, const void *planes_dev, int n, int c_in, int H, int W, void *occ_dev,
                         void *stream);
int apz_layout_convert(apz_engine *e, const void *src_dev, void *dst_dev, int64_t planes, int to_rows16, void *stream);

/* ---- the training step on framed boards (csrc/bn_frame.h, csrc/frame15.h): a board of side S in 6 .. 14 (not 8, not 10)
 * is the top-left S x S window of the 15x15 frame, and the trunk runs on the 15x15 kernels above (apz_wino_conv_add,
 * apz_wgrad_wino), which compute exactly the S x S convolution and its gradients provided the off-board cells of every
 * tensor they READ are zero.  They write whole planes, so the mask sits in the BatchNorm passes.  Every entry point here
 * takes `side` explicitly and runs on a 15x15 engine (APZ_E_UNSUPPORTED on another, and for a side other than 6, 7, 9,
 * 11, 12, 13, 14 or 15).  side = 15 returns the bits of the plain padded-row entry points.
 *   apz_bn_fwd_frame         apz_bn_fwd_stats (padded-row layout only, statistics always by a pass of its own) over the
 *                            on-board cells: count n * side * side (batch variance, and the unbiased factor of run_var);
 *                            off-board cells of x and resid may hold anything, NaN and inf included (they are selected
 *                            away, never multiplied); every off-board cell of y is exactly +0 and every off-board bit of
 *                            mask_dev 0.
 *   apz_bn_bwd_frame         apz_bn_bwd_max with the same mask: dy and xhat are selected before they are summed, count
 *                            n * side * side, off-board dx and dres exactly +0, dxsum / dxmax from the masked values.
 *   apz_frame_planes_dev     dense [planes][side][side] -> dense [planes][15][15], off-board cells zero.
 *   apz_conv1x1_fwd_frame    apz_conv1x1_fwd on the window of a padded-row x: y dense [n][CO][side][side].
 *   apz_conv1x1_bwd2_frame   apz_conv1x1_bwd2 with dy1 / dy2 dense [n][CO][side][side], x and dx padded rows: rows
 *                            0 .. side - 1 of dx are written (columns side .. 15 zero), rows side .. 14 are left as they
 *                            were -- apz_bn_bwd_frame, which reads dx next, masks them. */
int apz_bn_fwd_frame(apz_engine *e, const void *x_dev, const void *resid_dev, const void *gamma_dev,
                     const void *beta_dev, void *run_mean_dev, void *run_var_dev, void *y_dev, void *mean_dev,
                     void *invstd_dev, void *mask_dev, int n, int C, int layout, int relu, float momentum, float eps,
                     int side, void *stream);
int apz_bn_bwd_frame(apz_engine *e, const void *dy_dev, const void *x_dev, const void *out_dev, const void *mask_dev,
                     const void *gamma_dev, const void *mean_dev, const void *invstd_dev, void *dx_dev, void *dres_dev,
                     void *dgamma_dev, void *dbeta_dev, void *dxsum_dev, int dxsum_ld, void *dxmax_dev, int n, int C,
                     int layout, int relu, int side, void *stream);
int apz_frame_planes_dev(apz_engine *e, const void *src_dev, void *dst_dev, int64_t planes, int side, void *stream);
int apz_conv1x1_fwd_frame(apz_engine *e, const void *x_dev, const void *w_dev, const void *bias_dev, void *y_dev, int n,
                          int C, int CO, int side, void *stream);
int apz_conv1x1_bwd2_frame(apz_engine *e, const void *x_dev, const void *w1_dev, const void *dy1_dev, int CO1,
                           const void *w2_dev, const void *dy2_dev, int CO2, void *dx_dev, void *dw_dev, int n, int C,
                           int side, int accumulate_dx, void *stream);

int apz_sync(apz_engine *e);
void *apz_stream(apz_engine *e);
void *apz_device_alloc(apz_engine *e, int64_t bytes);
void apz_device_free(apz_engine *e, void *p);
int apz_memcpy_h2d(apz_engine *e, void *dst_dev, const void *src_host, int64_t bytes);
int apz_memcpy_d2h(apz_engine *e, void *dst_host, const void *src_dev, int64_t bytes);

/* ---- measurement / test hooks ---------------------------------------------------------- */
/* Time conv layer `layer` (0 = stem, 1.. = trunk convs in graph order) alone at batch n on
 * synthetic resident inputs: `warmup` untimed + `iters` timed launches bracketed by HIP
 * events on the engine stream; ms_out[0] = average milliseconds per launch. */
int apz_conv3x3_bench(apz_engine *e, int layer, int n, int iters, int warmup, float *ms_out);
/* After a forward of batch n: copy the output activation of conv layer `layer`
 * ([n][C_out][H][W]) to host (per-layer parity tests). */
int apz_layer_io(apz_engine *e, int layer, float *host_out, int64_t count);
/* TEST HOOK, engines with padded-row activations (the 128-filter residual net at 15x15 and at framed sizes): the same for
 * the raw activation [n][C_out][15][16], count = n * C_out * 240.  On a framed engine every cell outside the S x S window
 * of every layer but the last is exactly +0 (csrc/frame15.h); the last layer's off-board cells hold whatever the
 * convolution left there (the heads read on-board cells only). */
int apz_layer_frame(apz_engine *e, int layer, float *host_out, int64_t count);
/* Per-kernel-class HIP-event timing over subsequent forwards: on = 1 times every forward,
 * on = k > 1 every k-th forward (the event records cost a few us per kernel, so sampled timing
 * keeps the measured run undisturbed); then read out[0] = total ms, out[1] = timed launches
 * (resolved at apz_sync). */
/* on != 0: apz_submit_codes replays the launch sequence of a small batch (<= 64 boards) as a HIP graph from the third
 * submission of a (slot, batch size) pair on (results unchanged: the same kernels with the same arguments).  Default: off
 * -- measured slower than the plain launches on ROCm 7.2 (profiles/r04_graph_ab.log). */
int apz_set_forward_graphs(apz_engine *e, int on);
/* Dihedral leaf symmetry of the entry points that forward position codes for a caller (apz_forward_codes_host,
 * apz_forward_codes_async, apz_submit_codes / apz_wait, the exact repeat of an overflowed batch included); csrc/leaf_sym.h.
 * The net is trained on all eight dihedral images of every position (apz_augment8, apz_replay_gather); by default it is
 * evaluated in one orientation.  Image k of a code row, k = 0 .. 7 in apz_augment8's order (6 = identity): the code row of
 * that image of the position.  If the net answers q_k on image k, the position's policy is probs[perm_p[k][p]] = q_k[p]
 * (perm_p: the pi table of apz_augment8) and its value is unchanged: "folding back".
 *   APZ_SYM_NONE   (default) the engine launches exactly what it launched before this call existed.
 *   APZ_SYM_KEYED  every board is evaluated on ONE image, k = key(seed, its H*W + 1 code bytes) (apz_leaf_symmetry_keys),
 *                  and folded back: one forward of n boards plus two short launches.  The answer stays a function of
 *                  (weights, seed, position): not of the batch, the row, the slot, the game or the rank.
 *   APZ_SYM_MEAN8  board b becomes rows 8b .. 8b + 7 of ONE forward of 8 n boards (image k in row 8b + k); probs[m] =
 *                  0.125f * (((((((u_0 + u_1) + u_2) + u_3) + u_4) + u_5) + u_6) + u_7) with u_k the folded policy of image k,
 *                  plain fp32 adds in that order, the value likewise from the eight tanh outputs: equivariant by
 *                  construction.  Needs 8 n <= max_batch (else APZ_E_ARG, the message says so), and the arithmetic a batch
 *                  gets (apz_set_trunk_arith, apz_set_trunk_uniform) is that of 8 n boards: five positions are a 40-board
 *                  forward.
 * Timed in the APZ_K_ENCODE class.  Takes effect from the next forward; HIP graphs are dropped and captured again.
 * The planes entry points, apz_forward_dev_host, calibration, apz_prewarm, apz_layer_io and apz_conv3x3_bench are not
 * concerned (after a forward under APZ_SYM_MEAN8, apz_layer_io speaks of its 8 n image rows).
 * APZ_E_ARG for another mode, APZ_E_STATE while a slot is in flight, APZ_E_UNSUPPORTED on a non-square board. */
#define APZ_SYM_NONE 0
#define APZ_SYM_KEYED 1
#define APZ_SYM_MEAN8 2
int apz_set_leaf_symmetry(apz_engine *e, int mode, uint64_t seed);
int apz_get_leaf_symmetry(apz_engine *e, int *mode, uint64_t *seed);
/* The image index APZ_SYM_KEYED uses for each of n code rows (codes_host [n][stride], hw = H*W < stride), with
 *   fmix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33
 *   t_i = fmix64(seed + 0x9E3779B97F4A7C15 * (256 * i + byte_i + 1))   i = 0 .. hw, all mod 2^64
 *   k   = fmix64(seed ^ (sum_i t_i mod 2^64)) >> 61
 * -> k_out [n], each 0 .. 7.  Takes no engine and needs no GPU: the function the kernel runs, compiled for the host. */
int apz_leaf_symmetry_keys(const uint8_t *codes_host, int n, int hw, int stride, uint64_t seed, uint8_t *k_out);
/* Legal-move policy (default off: the reference's softmax over all H*W cells, policy_value_net_mxnet.py:90, and the engine
 * launches exactly what it launched before this call existed).  on != 0: every entry point that returns probs -- planes and
 * codes forms, host, device and async, apz_submit_codes / apz_wait with the exact repeat of an overflowed batch,
 * apz_forward_dev_host, HIP-graph replay -- takes the policy softmax over the EMPTY cells E of each board:
 *   probs[m] = exp(l_m - max_E l) / sum_E exp(l - max_E l) on E, exactly +0 on occupied cells,
 * so the priors of a search node sum to 1 over its legal moves.  Move m = h*W + w is occupied where code byte m != 0 (codes
 * entry points: the head reads the forward's own code rows in place) or where apz_occupancy_planes says so (planes entry
 * points: staged by one short launch in front of the head).  Under a leaf symmetry the mask is that of the image the forward
 * reads, so the folded answer is zero on the position's own occupied cells, under APZ_SYM_MEAN8 as well.  Occupied cells
 * are left out by selection, never by arithmetic: a NaN, an inf or the row's largest logit there changes no output bit; a
 * row without an empty cell is all zeros.  The masked heads (csrc/heads.h, csrc/conv8_small.h) keep the unmasked heads'
 * ownership of cells by lanes and their reduction trees: a board with no stone gets the switch-off bits, and a row's bits
 * depend on neither the batch nor the grid.  Values, logits_dev and vlogits_dev of apz_forward are untouched.
 * Engine state: apz_load_weights and apz_load_weights_dev keep it; HIP graphs are dropped and captured again.
 * APZ_E_STATE while a slot is in flight.  apz_get_legal_policy: 0 / 1. */
int apz_set_legal_policy(apz_engine *e, int on);
int apz_get_legal_policy(apz_engine *e);
int apz_set_profiling(apz_engine *e, int on);
/* TEST HOOK.  The 15x15 / 128-filter residual net has two trunk convolution kernels: the fused F(4x4,3x3) Winograd kernel
 * (default, csrc/trunk15_wino3.h) and the direct convolution (csrc/trunk15_ring.h) that the tests use as the in-tree
 * cross-check of the former (exact fp32 FMA chains, no transform).  Takes effect from the next forward. */
/* Arithmetic of the 128 -> 128 trunk convolutions of the 15x15 residual net (policy_value_net_mxnet.py:77-83), to be
 * chosen BEFORE apz_load_weights.  APZ_ARITH_F32 (default): exact fp32 products on the fp32 matrix pipe -- the bits the
 * parity tests rest on.  APZ_ARITH_BF16X3: batches of more than 32 boards run csrc/trunk15_wino3b.h -- every fp32 operand
 * as three bf16 terms, six bf16 products per fp32 product, fp32 accumulation: fp32-accurate (tests/
 * test_gpu_winograd_numerics.py), different low-order bits.  APZ_ARITH_F16X2 (round 6): batches of more than 32 boards run
 * csrc/trunk15_wino3h.h -- every fp32 operand as two fp16 terms (weights times a per-channel power of two), three products
 * per fp32 product on the fp16 matrix pipe, fp32 accumulation: the same accuracy class, 1.5x the exact kernel's speed.
 * An activation beyond the fp16 range (|x| > ~655) shows as a non-finite output; the kernel raises a word and the entry
 * point that collects the forward (apz_wait, apz_forward_host, apz_forward_codes_host, apz_forward, apz_forward_codes_async
 * -- the last two then return with the stream drained) repeats it on the exact-fp32 kernel: results are always finite-
 * checked, never silently wrong.  apz_trunk_overflows: how many forwards were repeated.
 * 8x8 boards (policy_value_net_mxnet_simple.py:68-92 and the 8x8 residual nets): APZ_ARITH_F16X2 runs every 3x3 convolution
 * with a multiple of 64 input channels on csrc/conv8_split.h (the same two-term split, no Winograd transform: activations up
 * to 65 504 are in range) for EVERY batch size, the first layer on conv8_kernel; same overflow word, same repeat.
 * Every other 15x15 net (the simple net, the residual nets of 64 and 256 filters; default APZ_ARITH_F32): APZ_ARITH_F16X2
 * runs every 3x3 convolution with a multiple of 64 input channels on csrc/conv15_split.h -- conv8_split.h's arithmetic and
 * weights on dense 15x15 planes, for EVERY batch size, a board's bits independent of the batch; the other layers on the
 * fp32 generic kernel (csrc/conv3x3_mfma.h), which also runs the repeat of a forward that raised the overflow word.  No
 * activation exponents there; apz_set_trunk_uniform does nothing.
 * APZ_ARITH_BF16X3 exists for the 15x15 / 128-filter net only (APZ_E_UNSUPPORTED elsewhere). */
#define APZ_ARITH_F32 0
#define APZ_ARITH_BF16X3 1
#define APZ_ARITH_F16X2 2
int apz_set_trunk_arith(apz_engine *e, int arith);
/* Batch-size independence of the APZ_ARITH_F16X2 trunk (15x15 / 128-filter residual net).  By default a batch of more than
 * 32 boards runs the two-term fp16 kernel (csrc/trunk15_wino3h16.h) and a batch of <= 32 boards the exact-fp32 small-batch
 * kernel (csrc/trunk15_wino3s.h): a position's low-order bits depend on how many boards share its forward.  on != 0
 * (default off; takes effect from the next forward): batches of <= 32 boards run csrc/trunk15_wino3hs.h instead -- the
 * small-batch form of the f16x2 kernel, held to BIT equality with the batched kernel for every board (tests/
 * test_gpu_trunk_f16x2_small.py), with the same weights, overflow word and static exponents (a layer with exponent 0 runs
 * the unscaled form, as in the batched dispatch).  A board's result then depends on its planes, the weights and the
 * exponents only, whatever the batch.  A forward that raises the overflow word is repeated on the exact-fp32 kernel for the
 * WHOLE batch (for batches of more than 32 boards that is so with or without this call): the independence holds for forwards
 * that do not overflow.  The exact repeat, calibration, apz_prewarm, apz_conv3x3_bench and apz_layer_io follow the same
 * route as a forward of that n; APZ_TRUNK_WINOGRAD_BATCHED (test hook) still forces the batched form.  HIP graphs
 * (apz_set_forward_graphs) capture the new kernel like any other: every launch of a capture carries its own epoch.
 * An engine on which this call is never made launches exactly the kernels it launched before the call existed.
 * Returns APZ_OK and does nothing for APZ_ARITH_F32 and for 8x8 boards (already uniform: one kernel family for every batch
 * size); APZ_E_UNSUPPORTED, with the reason in apz_last_error, for APZ_ARITH_BF16X3 and for an engine created under
 * APZ_F16X2_K8=1 (no small-batch form of those kernels). */
int apz_set_trunk_uniform(apz_engine *e, int on);
long apz_trunk_overflows(apz_engine *e);
/* Static per-layer activation exponents of the APZ_ARITH_F16X2 trunk kernel (15x15 / 128-filter residual net, batches of
 * more than 32 boards; csrc/trunk15_wino3h16.h, WINO3H16_PLAIN_SCALED).  Unscaled, the two-term split holds activations
 * between 2^-3 (below it the lo term is a subnormal fp16 number with an absolute 2^-25 error) and ~655 (above it the
 * transformed tile overflows and the forward is repeated on the exact kernel -- every time).  With exponent a the kernel
 * multiplies the input of trunk convolution l by 2^a before the transform and folds 2^-a into the channel's 1 / S: both
 * exact, so the layer computes the same function with its window moved.  Activations in device memory stay unscaled fp32.
 *   a[count], count = 2 * n_blocks, graph order (convA1, convB1, convA2, ...); all 0 by default, and a layer with
 *   exponent 0 runs the unscaled kernel: an engine on which none of these calls is made behaves exactly as before.
 * The exponents are engine state: apz_load_weights and apz_load_weights_dev keep them.  They are STATIC -- changed only by
 * the calls below -- so a board's bits do not depend on its batch; a changed exponent changes the low-order bits of that
 * layer (same accuracy class).  set: |a| <= 100, additionally clamped so that 2^-a / S[co] stays a normal float for every
 * output channel of the layer as loaded (get returns the values in force; apz_load_weights clamps again, the device-side
 * refresh does not look).  APZ_E_UNSUPPORTED, with the reason in apz_last_error, for another arithmetic than APZ_ARITH_F16X2,
 * for an engine created under APZ_F16X2_K8=1 and for 8x8 boards (csrc/conv8_split.h is in range up to 65 504 already). */
int apz_set_trunk_act_exponents(apz_engine *e, const int *a, int count);
int apz_get_trunk_act_exponents(apz_engine *e, int *a, int count);
/* Calibration: one forward of the given batch (planes_host as for apz_forward_host, codes_host as for
 * apz_forward_codes_host) on the exact-fp32 kernels, measuring m_l = max |input of trunk convolution l| (csrc/act_max.h),
 * then a_l = 4 - floor(log2 m_l): m_l 2^a in [2^4, 2^5), 20x headroom below the overflow bound for positions that were not in
 * the batch (derivation: ACT_WINDOW_LOG2 in csrc/trunk15_wino3h16.h); a_l = 0 for m_l = 0.  layer_max_out (may be NULL)
 * receives the `count` maxima.  A maximum that is not finite: error, all exponents unchanged.  The maxima are taken behind
 * the ReLU, which hides a NaN, so the call then runs the batch once on the f16x2 kernel with the new exponents: if that
 * raises the overflow word (a layer is not finite in exact fp32 either) the call fails and the exponents are unchanged.
 * Synchronous; does not count as an overflow; the forwards' results are discarded. */
int apz_calibrate_trunk_planes(apz_engine *e, const float *planes_host, int n, float *layer_max_out, int count);
int apz_calibrate_trunk_codes(apz_engine *e, const uint8_t *codes_host, int n, float *layer_max_out, int count);
/* on != 0 (default off): the exact repeat of an overflowed forward (in the collecting entry points listed above) also
 * measures the maxima and sets a_l = min(a_l, 4 - floor(log2 m_l)) -- exponents only ever go down, and stay as they are if
 * a maximum is not finite.  apz_trunk_overflows counts that forward; the next forward of the same batch runs on the f16x2
 * kernel without a repeat.  apz_prewarm, apz_conv3x3_bench and apz_layer_io never adjust exponents (apz_conv3x3_bench on a
 * trunk layer runs the form the layer's current exponent selects). */
int apz_set_act_scale_auto(apz_engine *e, int on);
#define APZ_TRUNK_DIRECT 0
#define APZ_TRUNK_WINOGRAD 3            /* default: batches of <= 32 boards take the small-batch form (csrc/trunk15_wino3s.h) */
#define APZ_TRUNK_WINOGRAD_BATCHED 4    /* ... the batched form for every batch size (the tests hold the two forms to bit equality) */
#define APZ_TRUNK_WINOGRAD_NO_QUARTER 5 /* ... the batched form with 64-channel work items only (no 32-channel items for few-pair batches) */
int apz_test_select_trunk(apz_engine *e, int kind);
int apz_kernel_time_ms(apz_engine *e, int kernel_class, float *out2);
/* Enqueue `iters` forwards of n empty boards on the engine's stream and return without waiting (apz_sync waits).
 * GPU-only warm-up for measurements: clocks, the runtime's event / signal pools, instruction caches.  The results go
 * to the engine's device buffers and are never read; pending submissions are not disturbed (same stream, in order). */
int apz_prewarm(apz_engine *e, int n, int iters);

#ifdef __cplusplus
}
#endif
#endif
