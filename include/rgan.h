/*
 * rgan.h — C-ABI of the MI355X (gfx950) RelativisticGAN training core.
 *
 * The reference has no FFI of its own: its hot path is the module-level PyTorch
 * training loop of code/GAN_losses_iter.py (GLI).  Each entry point below replaces
 * the PyTorch op(s) that loop reaches, cited per function.
 *
 * Conventions:
 *   - plain device pointers (fp32 unless stated) and sizes; no torch types;
 *   - the caller allocates every output and every workspace; kernels never allocate;
 *   - return 0 on success, a hipError_t-compatible code otherwise
 *     (RGAN_EINVAL = invalid descriptor / sizes, checked on the host before launch);
 *   - every launch goes on `stream` (hipStream_t passed as void*); no host syncs, so
 *     every entry point is hipGraph-capturable.
 */
#ifndef RGAN_H
#define RGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGAN_EINVAL 1001

/* ABI revision.  2: rgan_adam_packed takes step = device float[2] (step[1] is the
 * call's uint32 arrival ticket, zero before the first call); revision 1 took float[1].
 * 3: adds rgan_conv_wgrad_rows.  4: adds rgan_bn_segment_apply and rgan_bn_backward_sums_apply.
 * rgan_diffaug_workspace, rgan_diffaug, rgan_ema_update, rgan_diffaug_p, rgan_ada_update,
 * rgan_ada_adjust, rgan_lecam, rgan_lecam_finish, rgan_diffaug_geo_workspace and rgan_diffaug_geo
 * are additive within revision 4 (nothing else changed), and so are rgan_sort_segments with its
 * _tile and _ws_bytes, the rgan_swd_ entry points and the nearest-image entry points
 * (rgan_nn_row_bytes, _pack_u8, _topk_splits, _topk_ws_bytes, _topk, _covered). */
#define RGAN_ABI_VERSION 4

/* Activation codes fused into epilogues (GLI:345,370,388,417,437,450; SELU GLI:338). */
enum {
  RGAN_ACT_NONE = 0, RGAN_ACT_RELU = 1, RGAN_ACT_LRELU = 2, RGAN_ACT_TANH = 3,
  RGAN_ACT_SIGMOID = 4, RGAN_ACT_SELU = 5
};

/* One 2-D convolution as the reference's torch.nn.Conv2d / ConvTranspose2d sees it.
 * "x" is the op's input image, "y" its output.  Element strides are given for
 * (batch, channel, h, w) so NCHW (reference layout) and NHWC (internal layout,
 * torch channels_last) tensors are both accepted.  Weights are in torch layout:
 * Conv2d [cout][cin][kh][kw], ConvTranspose2d [cin][cout][kh][kw], contiguous. */
typedef struct RganConv {
  int batch;
  int cin, hin, win;
  int cout, hout, wout;
  int kh, kw, stride, pad;
  int transposed;          /* 0: Conv2d, 1: ConvTranspose2d */
  long long xs[4];         /* x strides (b, c, h, w) in elements */
  long long ys[4];         /* y strides (b, c, h, w) in elements */
} RganConv;

/* Workspace bytes needed by rgan_conv_{fwd,dgrad,wgrad}; `which` = 0 fwd, 1 dgrad, 2 wgrad
 * (wgrad's includes the bias-gradient reduction scratch);
 * `prepacked` != 0: the caller passes packed weights (no packing scratch).  0 = unsupported. */
size_t rgan_conv_workspace(const RganConv* d, int which, int prepacked);

/* Kernel-ready weight layout for which = 0 (fwd) or 1 (dgrad): [phases][N][K] floats for
 * the implicit GEMMs (k contiguous: the B operand's LDS rows), [4][Cin][16] for the narrow
 * (<= 4 output channel) transposed conv.  Packing is separated so callers can cache it per weight version (weights change
 * only at the optimizer step, but each net is run 2-4 times per iteration).
 * rgan_conv_pack_floats returns 0 when the op reads the torch layout directly (narrow
 * 4x4 convs with <= 4 input channels) -- or when the descriptor is unsupported, which
 * rgan_conv_workspace reports separately (0). */
size_t rgan_conv_pack_floats(const RganConv* d, int which);
int rgan_conv_pack(const RganConv* d, int which, const float* w, float* packed, void* stream);
/* n packs at once (the stale layouts of a net after its optimizer step, torch.optim's
 * step at GLI:659/712 being what moved them): entry i = rgan_conv_pack(d[i], which[i], w[i],
 * packed[i]); the tiled layouts share one launch per 16, others get their own. */
int rgan_conv_pack_batch(int n, const RganConv* const* d, const int* which, const float* const* w,
                         float* const* packed, void* stream);

/* y = act(conv(x, w) * (*wscale) + bias).  Replaces Conv2d/ConvTranspose2d.forward
 * (GLI:336,361,387,410,428,448; arch 1 GLI:202-223,260-302) fused with the
 * following activation when no BatchNorm sits between them.  wpacked: nullable
 * rgan_conv_pack(which=0) output (then w may be NULL).  wscale: nullable device scalar
 * (spectral norm's 1/sigma, torch/nn/utils/spectral_norm.py:115-116), applied to the
 * accumulator in the epilogue.  A stride-1 pad-0 ConvTranspose2d over a 1x1 map (the 1x1 -> k x k
 * expansion) takes no bias: with one, rgan_conv_fwd and rgan_conv_fwd_bn return RGAN_EINVAL before
 * any launch (rgan_conv_workspace cannot say so: it does not see the bias). */
int rgan_conv_fwd(const RganConv* d, const float* x, const float* w, const float* wpacked,
                  const float* wscale, const float* bias, float* y, int act, float act_alpha,
                  void* ws, size_t ws_bytes, void* stream);

/* Conv2d/ConvTranspose2d.forward feeding a train-mode BatchNorm2d (GLI:361-366,387-391,
 * 428-433): y = conv(x, w) * (*wscale) + bias, and -- when the GEMM's vector epilogue
 * or its split-K reduce covers the layer -- the BatchNorm batch statistics of y as per-64-row
 * segment moments bn_part[S][2][C] = (sum y, sum y^2) in double, computed from the finished
 * tile in LDS or from the reduced rows in registers (no re-read of y).
 * S = rgan_conv_bn_segments(d, segs) (0: the epilogue cannot, use rgan_bn_stats); `segs`
 * equal batch segments are kept apart (the batched D(x)/D(G(z)) call: segment k's rows are
 * segments [k*S/segs, (k+1)*S/segs)).  *fused (host int) = 1 when bn_part was written.
 * Merge with rgan_bn_segment_stats. */
long long rgan_conv_bn_segments(const RganConv* d, int segs);
int rgan_conv_fwd_bn(const RganConv* d, const float* x, const float* w, const float* wpacked,
                     const float* wscale, const float* bias, float* y, void* ws, size_t ws_bytes,
                     double* bn_part, long long part_segments, int segs, int* fused, void* stream);

/* dx = d conv / d x applied to dy  (aten convolution_backward, grad_input). */
int rgan_conv_dgrad(const RganConv* d, const float* dy, const float* w, const float* wpacked,
                    const float* wscale, float* dx, void* ws, size_t ws_bytes, void* stream);

/* Post-op for the layer that PRODUCED a GEMM's output operand, applied where the output
 * value is final (the GEMM epilogue or its split-K reduce) instead of a separate pass over
 * it.  `x` has the output's element strides (same shape).
 *   mode 1 (activation backward, aten's threshold/leaky_relu/tanh backward of GLI:345,370,
 *          417 behind the conv's data gradient): out = v * act'(x), x = the producer's
 *          activation output;
 *   mode 2 (BatchNorm2d backward sums, the first half of aten native_batch_norm_backward,
 *          GLI:341-345/366-370/433-437): out = g = v * act'(x * al + be), x = the producer's
 *          BatchNorm input y, al = gamma * invstd, be = beta - mean * al from stats[k] of the
 *          output row's batch segment k (nseg equal segments of every phase's rows), and
 *          part[S][2][C] = (sum g, sum g (y - mean)) per 64-row segment in double, S =
 *          rgan_conv_post_segments(...); finish with rgan_bn_backward_parts. */
typedef struct RganPost {
  int mode;                /* 1 or 2 */
  int act;                 /* RGAN_ACT_* of the producer */
  float alpha;
  int nseg;                /* mode 2: batch segments with their own statistics (1 or 2) */
  const float* x;          /* activation output (mode 1) / BatchNorm input y (mode 2) */
  const float* stats;      /* mode 2: [nseg][2C] (mean, invstd) */
  const float* gamma;      /* mode 2: nullable */
  const float* beta;       /* mode 2: nullable */
  double* part;            /* mode 2: [part_segments][2][C] */
  long long part_segments;
} RganPost;

/* rgan_conv_fwd (which = 0, act none, no bias) or rgan_conv_dgrad (which = 1) with a
 * producer post-op.  *fused (host int) = 1 when the post-op was applied (else `out` holds
 * the plain result and the caller runs the separate pass).  rgan_conv_post_segments: S for
 * mode 2 (0: this GEMM cannot emit the sums) and (nullable *phases) the phase-major blocks
 * the S segments come in (4 for a k4 s2 p1 Conv2d data gradient, else 1). */
long long rgan_conv_post_segments(const RganConv* d, int which, int mode, int nseg, int* phases);
int rgan_conv_post(const RganConv* d, int which, const float* in, const float* w, const float* wpacked,
                   const float* wscale, float* out, void* ws, size_t ws_bytes, const RganPost* post,
                   int* fused, void* stream);

/* G's first layer on its 1x1 input (GLI:334-345: ConvTranspose2d(z, Cout, 4, 1, 0) + train-
 * mode BatchNorm2d + activation) in one launch: y[b][t][c] = sum_ci z[b][ci] W[ci][c][t]
 * (t = 4 kh + kw; y, a NHWC [B][4][4][Cout]), the BatchNorm batch statistics of each channel
 * over its B x 16 values (exact two-pass, double), running statistics + num_batches_tracked
 * updated as torch does, stats = (mean, invstd) [2][Cout], a = act(BN(y)).  z [B][Cin]
 * contiguous, 16-B aligned; B in {32, 64} (the batch sizes of BASELINE's configs); Cin (z size)
 * in {64, 128}; Cout % 16 == 0 (other shapes run the GEMM + BatchNorm entry points).
 * rgan_g1_wgrad: its weight gradient dW[ci][c][t] (+)= sum_b z[b][ci] dy[b][t][c] (dy NHWC). */
int rgan_g1_fwd_bn(const float* z, int B, int Cin, const float* w, int Cout, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                   long long* num_batches_tracked, int act, float act_alpha, float* y, float* a, float* stats,
                   void* stream);
int rgan_g1_wgrad(const float* z, int B, int Cin, const float* dy, int Cout, float* dw, int accumulate,
                  void* stream);

/* dw = d conv / d w applied to dy (aten convolution_backward, grad_weight), written
 * in torch weight layout; dbias (nullable) = per-output-channel sum of dy.
 * accumulate != 0: dw += ..., dbias += ... (autograd's gradient accumulation into an
 * existing .grad, GLI:605/624/658's repeated backward calls, done in the GEMM's epilogue
 * instead of a separate add pass). */
int rgan_conv_wgrad(const RganConv* d, const float* x, const float* dy, float* dw, float* dbias,
                    int accumulate, void* ws, size_t ws_bytes, void* stream);
/* The same with dbias summed over the pixel rows p >= dbias_row0 only (p = (b, h, w) in
 * order; 0 <= dbias_row0 < batch*hout*wout): the WGAN-GP double backward's weight gradient
 * runs one GEMM over [adjoint; forward] row pairs while the bias gradient is the forward
 * half's alone.  rgan_conv_wgrad(...) == rgan_conv_wgrad_rows(..., 0, ...). */
int rgan_conv_wgrad_rows(const RganConv* d, const float* x, const float* dy, float* dw, float* dbias,
                         long long dbias_row0, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- --NN_conv blocks: Upsample(scale_factor=2, nearest) + Conv2d(k3, s1, p1) ----
 * (GLI:351-356 middle, GLI:377-382 end).  conv3x3(up2(x), W) equals a k4 s2 p1
 * ConvTranspose2d of x with the folded weight Wt = A W A^T per 3x3 slice
 * (A = [[0,0,1],[0,1,1],[1,1,0],[1,0,0]]), so the layer runs as rgan_conv_* with
 * transposed = 1, k = 4, stride 2, pad 1 on Wt.
 * rgan_nn_fold_weight: W [cout][cin][3][3] -> Wt [cin][cout][4][4] (16-byte aligned).
 * rgan_nn_unfold_grad: the adjoint, dWt [cin][cout][4][4] -> dW [cout][cin][3][3]
 * (the Conv2d weight gradient, aten convolution_backward grad_weight). */
int rgan_nn_fold_weight(const float* w, int cout, int cin, float* wt, void* stream);
int rgan_nn_unfold_grad(const float* dwt, int cout, int cin, float* dw, void* stream);

/* ---- image layers (k4 s2 p1 with <= 4 image channels: GLI:404 D start, GLI:386 G end) ----
 * rgan_patches_k4s2: patch matrix of an image [B][C][H][W] (element strides b,c,h,w; C <= 4,
 * H, W even) on the half-size grid: X[(b, i, j)][4 t + c] = img[b][c][2i-1+kh][2j-1+kw],
 * t = 4 kh + kw, zero outside the image and for c >= C; X is [B*(H/2)*(W/2)][64] floats,
 * 16-byte aligned.  Every image-layer GEMM then runs as a 1x1 rgan_conv_* over X.
 * rgan_patch_weight: W1[o][4 t + c] = w[o*row_stride + c*channel_stride + t] (rows x 64).
 * rgan_unpatch_grad: dw[o][c][t] = g1[o*row_stride + (4 t + c)*col_stride] (rows x C x 16). */
int rgan_patches_k4s2(const float* img, int batch, int channels, int height, int width,
                      const long long* strides, float* patches, void* stream);
int rgan_patch_weight(const float* w, int rows, int channels, long long row_stride, long long channel_stride,
                      float* w1, void* stream);
int rgan_unpatch_grad(const float* g1, int rows, int channels, long long row_stride, long long col_stride,
                      float* dw, int accumulate, void* stream);

/* ---- image export (GLI:563-565 sample grid, GLI:759-768 extra FID images) ----
 * torchvision.utils.save_image's float -> uint8 step on the device: t = x*scale + shift;
 * optional normalize with range = device float[2] {min, max} of the batch
 * (make_grid(normalize=True): t = (clamp(t, lo, hi) - lo) / max(hi - lo, 1e-5)); then
 * u8 = trunc(clamp(t*255 + 0.5, 0, 255)).  x: [B][C][H][W] with element strides
 * strides[4]; grid = 0: out [B][H][W][C] (one image per file, padding 0);
 * grid = 1: make_grid layout [Hg][Wg][C], nrow tiles per row, `padding` pixels of 0.
 * rgan_minmax: out2 = {min, max} of x[0..n) (ws: rgan_minmax_ws_bytes). */
/* Real-image batch (GLI:173-177 + ToTensor/Normalize GLI:160-166): out[b] = (u8 / 255 - 0.5)
 * / 0.5 of images[idx[b]], images = decoded uint8 [N][per] resident on the device
 * (per = C*S*S, a multiple of 4; out 16-byte aligned). */
int rgan_gather_images_u8(const unsigned char* images, const long long* idx, int batch, long long per,
                          float* out, void* stream);
size_t rgan_minmax_ws_bytes(long long n);
int rgan_minmax(const float* x, long long n, float* out2, void* ws, void* stream);
int rgan_images_to_u8(const float* x, int B, int C, int H, int W, const long long* strides,
                      float scale, float shift, const float* range, int grid, int nrow, int padding,
                      unsigned char* out, void* stream);

/* ---- BatchNorm2d, train mode (GLI:341,366,433; arch 1 GLI:204-218,262-297) ----
 * Tensors are [batch*h*w][C] with element strides (sp = pixel stride, sc = channel
 * stride); P = batch*h*w.  stats = float[2*C] workspace slot receiving (mean, invstd).
 * Running stats follow torch: r = (1-m) r + m * stat, unbiased var for running_var;
 * num_batches_tracked (int64, nullable) += 1.  `partial` workspace: rgan_bn_partial_bytes. */
size_t rgan_bn_partial_bytes(long long P, int C);
int rgan_bn_stats(const float* y, long long P, int C, long long sp, long long sc,
                  float eps, float momentum, float* running_mean, float* running_var,
                  long long* num_batches_tracked, float* stats, void* partial, void* stream);
/* rgan_conv_fwd_bn's segment moments [s0, s1) -> stats + running stats (moments == NULL),
 * or this rank's (count, mean, M2) double[3*C] for SyncBN (moments != NULL, as
 * rgan_bn_moments).  Chan merges in a fixed order (deterministic). */
int rgan_bn_segment_stats(const double* part, long long s0, long long s1, int C, int seg_rows,
                          float eps, float momentum, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float* stats, double* moments, void* stream);
/* The batched D pass's two calls (GLI:580-605 run D(x) then D(x_fake)) in one launch each:
 * segment stats of the nseg (1 or 2) equal halves of segments [s0, s1) -> stats[nseg][2C],
 * running statistics updated in call order; and the normalisation + activation of y's nseg
 * equal row ranges with their stats rows (dense NHWC y and a, P % nseg == 0). */
int rgan_bn_segment_stats_n(const double* part, long long s0, long long s1, int nseg, int C, int seg_rows,
                            float eps, float momentum, float* running_mean, float* running_var,
                            long long* num_batches_tracked, float* stats, void* stream);
int rgan_bn_apply_segments(const float* y, long long P, int C, int nseg, const float* stats, const float* gamma,
                           const float* beta, int act, float act_alpha, float* a, void* stream);
/* Both of the above in one call (ABI 4): stats[nseg][2C] of y's nseg equal row ranges from
 * rgan_conv_fwd_bn's segment sums part[S][2][C] (P == S * seg_rows), running statistics in call
 * order, and a = act(BN(y)).  A small layer (S / nseg <= 64 segments) runs as ONE launch whose
 * blocks each merge their channels' segment sums in the same fixed order; a larger one as
 * rgan_bn_segment_stats_n + rgan_bn_apply_segments.  Dense NHWC y and a, 16-byte aligned. */
int rgan_bn_segment_apply(const double* part, long long S, int nseg, int seg_rows, const float* y, long long P,
                          int C, float eps, float momentum, float* running_mean, float* running_var,
                          long long* num_batches_tracked, const float* gamma, const float* beta, int act,
                          float act_alpha, float* stats, float* a, void* stream);
/* a = act(gamma * (y - mean) * invstd + beta)  (torch's alpha/beta form) */
int rgan_bn_apply(const float* y, long long P, int C, long long sp, long long sc,
                  const float* stats, const float* gamma, const float* beta,
                  int act, float act_alpha, float* a, long long asp, long long asc, void* stream);
/* Staged form for data parallelism (SyncBN): local moments (count, mean, M2) as
 * double[3][C]; the caller gathers them from all ranks into [nranks][3][C] and merges
 * in rank order with rgan_bn_finalize (Chan's parallel variance; deterministic). */
int rgan_bn_moments(const float* y, long long P, int C, long long sp, long long sc,
                    double* moments, void* partial, void* stream);
int rgan_bn_finalize(const double* moments, int nranks, int C, float eps, float momentum,
                     float* running_mean, float* running_var, long long* num_batches_tracked,
                     float* stats, void* stream);
/* The batched D pass's two calls' BatchNorm backward (GLI:605/624/644 through each call's
 * BatchNorm) in three launches instead of six: dy of y's nseg (1 or 2) equal row ranges, each
 * with its stats row [nseg][2C] and its own sums; dgamma / dbeta = the segments' sum.  Dense
 * NHWC da, y, dy; partial >= nseg * rgan_bn_partial_bytes(P / nseg, C). */
int rgan_bn_backward_segments(const float* da, const float* y, long long P, int C, int nseg, const float* stats,
                              const float* gamma, const float* beta, int act, float act_alpha, float* dy,
                              float* dgamma, float* dbeta, void* partial, void* stream);
/* The rest of the BatchNorm backward after a GEMM's post-op wrote g = da * act' and the
 * segment sums (rgan_conv_post mode 2): merge part[S][2][C] (phases phase-major blocks of
 * S / phases segments, each split into nseg batch segments) into sums[nseg][2][C] (caller's
 * scratch), then dy = al (g - sum_g / Pk - (y - mean) invstd^2 sum_gx / Pk) per batch segment,
 * dgamma / dbeta = the segments' sum (nullable).  Dense NHWC g, y, dy. */
int rgan_bn_backward_parts(const float* g, const float* y, long long P, int C, int nseg, const float* stats,
                           const float* gamma, const float* beta, const double* part, long long S, int phases,
                           float* dy, float* dgamma, float* dbeta, double* sums, void* stream);
/* The staged backward's sums and apply in one call (ABI 4; one process or per-shard BN): writes
 * sums[2][C] = (sum g, sum g (y - mean)), g = da * act' (the WGAN-GP engine keeps them for the
 * double backward), dy = BN-backward(g) + add (add nullable), dgamma / dbeta written or, with
 * accumulate_affine, added into (nullable).  Dense NHWC da, y, dy, add; add may be dy itself
 * (added in place).  P <= 2048 rows and C >= 1024 (C % 16 == 0): one launch; otherwise
 * rgan_bn_backward_sums + rgan_bn_backward_apply_ex.  partial: rgan_bn_partial_bytes(P, C). */
int rgan_bn_backward_sums_apply(const float* da, const float* y, long long P, int C, const float* stats,
                                const float* gamma, const float* beta, int act, float act_alpha, const float* add,
                                float* dy, float* dgamma, float* dbeta, int accumulate_affine, double* sums,
                                void* partial, void* stream);
/* Backward through act(BN(y)): given da, produce dy, dgamma, dbeta. */
int rgan_bn_backward(const float* da, long long dsp, long long dsc,
                     const float* y, long long P, int C, long long sp, long long sc,
                     const float* stats, const float* gamma, const float* beta,
                     int act, float act_alpha, float* dy, long long ysp, long long ysc,
                     float* dgamma, float* dbeta, void* partial, void* stream);
/* Staged backward: local sums double[2][C] = (sum g, sum g*(y-mean)), g = da*act'; the
 * caller all-reduces them over ranks, then apply with the global pixel count P_global.
 * All BN sums accumulate in double (torch's CPU kernel does too): the backward sums can
 * cancel almost completely and a float accumulator leaves a coherent error in dy. */
int rgan_bn_backward_sums(const float* da, long long dsp, long long dsc, const float* y,
                          long long P, int C, long long sp, long long sc, const float* stats,
                          const float* gamma, const float* beta, int act, float act_alpha,
                          double* sums, void* partial, void* stream);
int rgan_bn_backward_apply(const float* da, long long dsp, long long dsc, const float* y,
                           long long P, int C, long long sp, long long sc, const float* stats,
                           const float* gamma, const float* beta, int act, float act_alpha,
                           const double* sums, long long P_global, float* dy, long long ysp,
                           long long ysc, float* dgamma, float* dbeta, void* stream);

/* rgan_bn_backward_apply plus: add (nullable, y's strides) is added to dy, and
 * accumulate_affine != 0 adds dgamma/dbeta into the given buffers (the batched D
 * step's two BN calls, the WGAN-GP double backward's second-order terms). */
int rgan_bn_backward_apply_ex(const float* da, long long dsp, long long dsc, const float* y,
                              long long P, int C, long long sp, long long sc, const float* stats,
                              const float* gamma, const float* beta, int act, float act_alpha,
                              const double* sums, long long P_global, const float* add, float* dy,
                              long long ysp, long long ysc, float* dgamma, float* dbeta,
                              int accumulate_affine, void* stream);

/* ---- WGAN-GP double backward (GLI:655 create_graph=True, differentiated by GLI:658) ----
 * Layer act(BN(y)) with batch statistics `stats`, whose create-graph backward took dh
 * (the upstream gradient) to dy = BNback(dh act'(z)) with first-order sums
 * first_sums = (sum e, sum e (y - mean)) [2C] (rgan_bn_backward_sums, global).  Given
 * a = dP/d(dy) (all [P][C] with strides sp, sc):
 *   rgan_bn_dd_sums stage 1: sums[3][C] = (sum a, sum a xhat, sum a e);
 *                   stage 2 (only for act'' != 0: tanh, sigmoid, SELU; needs the global
 *                   stage-1 sums): sums[2][C] = (sum t, sum t xhat);
 *   rgan_bn_dd_apply: adj_dh = dP/d(dh) (nullable), ydir = the direct dP/dy of the
 *                   double backward, dgamma2/dbeta2 (nullable, accumulate_affine: +=)
 *                   its gamma/beta terms (from the *_local sums when given: under
 *                   SyncBN the gradient all-reduce sums them over ranks).
 * Cross-rank: the caller all-reduces first_sums and each stage's sums (SyncBN) and
 * passes the global pixel count P_global.  partial: rgan_bn_dd_partial_bytes. */
size_t rgan_bn_dd_partial_bytes(long long P, int C);
int rgan_bn_dd_sums(const float* a, const float* y, const float* dh, long long P, int C,
                    long long sp, long long sc, const float* stats, const float* gamma,
                    const float* beta, int act, float act_alpha, int stage, const double* stage1,
                    long long P_global, double* sums, void* partial, void* stream);
int rgan_bn_dd_apply(const float* a, const float* y, const float* dh, long long P, int C,
                     long long sp, long long sc, const float* stats, const float* gamma,
                     const float* beta, int act, float act_alpha, const double* first_sums,
                     const double* stage1, const double* stage2, const double* stage1_local,
                     const double* stage2_local, long long P_global, float* adj_dh, float* ydir,
                     float* dgamma2, float* dbeta2, int accumulate_affine, void* stream);
/* Without BatchNorm (dy = dh act'(y), act_out = act(y)): adj_dh = a act'(y),
 * ydir = a dh act''(y); either output nullable. */
int rgan_act_dd(const float* a, const float* act_out, const float* dh, long long n, int act,
                float act_alpha, float* adj_dh, float* ydir, void* stream);

/* ---- elementwise ---- */
/* dx = da * act'(a) where a = act(x) is the saved activation output. */
int rgan_act_backward(const float* da, const float* a, long long n, int act, float act_alpha,
                      float* dx, void* stream);
/* dx = da * act'(a) + add (add nullable, same layout) */
int rgan_act_backward_ex(const float* da, const float* a, const float* add, long long n, int act,
                         float act_alpha, float* dx, void* stream);
/* out[n] (+)= sum over pixels of t (per channel; bias gradient), strided like bn;
 * accumulate != 0 adds into out (gradient accumulation, no separate add pass).
 * partial: rgan_bn_partial_bytes(P, C) of scratch (fixed-order two-level sum). */
int rgan_channel_sum(const float* t, long long P, int C, long long sp, long long sc,
                     float* out, int accumulate, void* partial, void* stream);

/* dgamma (+)= (float)(sums[1][c] * invstd[c]), dbeta (+)= (float)sums[0][c] (accumulate != 0:
 * added) from [2][C] BatchNorm backward sums (rgan_bn_backward_sums) and stats [mean; invstd]:
 * the affine gradients from a rank's LOCAL sums under SyncBN, where the normalisation uses the
 * all-reduced ones (either output nullable). */
int rgan_bn_affine_grads(const double* sums, const float* stats, int C, float* dgamma, float* dbeta,
                         int accumulate, void* stream);

/* ---- loss heads (GLI:481-484, 592-644, 686-709) ----
 * kind = --loss_D (1..8); side 0 = D-real (heads 1-4) / D (heads 5-8), 1 = D-fake
 * (heads 1-4), 2 = G.  r, f: [n] (either nullable per head).  loss: device float[1];
 * dr, df: [n] gradients of loss w.r.t. r and f (nullable).  n <= 65536.  The per-element
 * terms are fp32.  The loss sums of heads 1-4 (whose gradients depend on no sum) are
 * accumulated in double and rounded once; heads 5-8 sum in fp32. */
int rgan_loss_head(int kind, int side, const float* r, const float* f, int n,
                   float* loss, float* dr, float* df, void* stream);
/* Heads 1-4, D side as ONE launch: loss3 = {errD_real, errD_fake, errD_real + errD_fake}
 * and both gradients (nullable) -- the batched D step's pair of losses. */
int rgan_loss_head_pair(int kind, const float* r, const float* f, int n, float* loss3, float* dr,
                        float* df, void* stream);
/* Heads 5-8, G side, on the G step's batched output y = [D(G(z)); D(x)] (2n values): loss
 * and dy[0..n) = d loss / d D(G(z)), dy[n..2n) = 0 (D(x) is a no-grad forward, GLI:681),
 * in one launch. */
int rgan_loss_head_joint(int kind, const float* y, int n, float* loss, float* dy, void* stream);
/* Distributed form: the three phases of the same head with the cross-rank sums done by
 * the caller between them.  phase 0: sums[0..1] = (sum r, sum f) local;
 * phase 1: given global means in gsum[0..1] (sum r, sum f over n_global), sums[0..3] =
 * local (sum a, sum b, sum a', sum b'); phase 2: loss and grads from global gsum[0..5]. */
int rgan_loss_head_dist(int kind, int side, int phase, const float* r, const float* f, int n,
                        int n_global, const float* gsum, float* sums, float* loss,
                        float* dr, float* df, void* stream);
/* out = in * (*scale) (device scalar), used to apply an upstream gradient. */
int rgan_scale(const float* in, const float* scale, long long n, float* out, void* stream);

/* ---- WGAN-GP (GLI:646-658) ---- */
/* xb[b] = x[b]*u[b] + xf[b]*(1-u[b]) over per-sample blocks of `per` elements. */
int rgan_gp_interp(const float* x, const float* xf, const float* u, int batch, long long per,
                   float* xb, void* stream);
/* norms[b] = ||g_b||_2 ; loss = lam * mean_b (norms-1)^2 over n_global samples. */
int rgan_gp_penalty(const float* g, int batch, long long per, float lam, int n_global,
                    float* norms, float* loss, void* stream);
/* dg = (*gscale) * lam * 2 (norm_b - 1)/n_global * g_b / norm_b (0 where norm_b == 0). */
int rgan_gp_penalty_backward(const float* g, const float* norms, int batch, long long per,
                             float lam, int n_global, const float* gscale, float* dg,
                             void* stream);

/* ---- zero-centred gradient penalties R1 / R2 (--rgan_r1, --rgan_r2; not in the reference) ----
 * g: [batch][per] gradient image of D at the penalised point, contiguous.  batch <= 65535
 * (the forward's grid puts the sample index in its y dimension), n_global >= batch.
 * Forward: sq[b] = ||g_b||_2^2 and loss[0] = gamma / 2 * (sum_b sq[b]) / n_global, as a
 * two-stage sum in a fixed order (no atomics, no counters: two calls give the same bits):
 * stage 1 splits every sample over enough blocks to fill the chip, stage 2 adds each
 * sample's partials and then the samples in index order, in double.  16-byte loads when
 * per % 4 == 0 and g is 16-byte aligned; any per and any 4-byte alignment otherwise.
 * ws: rgan_gp_zc_workspace(batch, per) bytes (0 for arguments the calls reject). */
size_t rgan_gp_zc_workspace(int batch, long long per);
int rgan_gp_zc_penalty(const float* g, int batch, long long per, float gamma, int n_global,
                       float* sq, float* loss, void* ws, void* stream);
/* dg = (gscale ? *gscale : 1) * gamma / n_global * g.  gscale (nullable) is a device
 * scalar read by the kernel, so a captured call follows it.  dg may be g itself (each
 * element is read, then written); a partial overlap is not supported.  16-byte accesses
 * when per % 4 == 0 and both g and dg are 16-byte aligned. */
int rgan_gp_zc_penalty_backward(const float* g, int batch, long long per, float gamma,
                                int n_global, const float* gscale, float* dg, void* stream);

/* ---- spectral norm (torch/nn/utils/spectral_norm.py:62-139; GLI call sites 334-446) ----
 * W viewed as [rows][cols]; element (r, c) sits at r*rs + (c / lo)*hs + (c % lo).
 * Conv2d weight (dim 0): rs = cin*kk, hs = kk, lo = kk.  ConvTranspose2d (dim 1, the
 * permute(1,0,2,3) view): rs = kk, hs = cout*kk, lo = kk.
 * One power iteration: v = normalize(W^T u), u = normalize(W v), sigma = u.(W v);
 * writes u, v in place and inv_sigma[0] = 1/sigma.  do_iter = 0 only recomputes sigma.
 * ws: rgan_spectral_ws_bytes(rows, cols). */
size_t rgan_spectral_ws_bytes(int rows, int cols);
int rgan_spectral_power(const float* W, int rows, int cols, long long rs, long long hs, int lo,
                        float eps, float* u, float* v, float* inv_sigma, int do_iter,
                        void* ws, void* stream);
/* All spectral layers of one net call in FOUR launches (instead of four per layer):
 * each layer gets one power iteration exactly as rgan_spectral_power(do_iter=1).
 * n <= 16 layers; every sum in a fixed order (no cross-block hand-off, no counters); ws:
 * rgan_spectral_batch_ws_bytes(n, layers). */
typedef struct RganSnLayer {
  const float* W;
  int rows, cols, lo;
  long long rs, hs;
  float* u;                /* updated in place (the module's weight_u / weight_v buffers) */
  float* v;
  float* u_copy;           /* nullable: the new u, v also written here (the call's own copy,
                              torch spectral_norm's u.clone() / v.clone(), spectral_norm.py:112-114) */
  float* v_copy;
  float* inv_sigma;
} RganSnLayer;
size_t rgan_spectral_batch_ws_bytes(int n, const RganSnLayer* layers);
int rgan_spectral_power_batch(int n, const RganSnLayer* layers, float eps, void* ws, void* stream);
/* dW_orig = dW_eff/sigma - (<dW_eff, W_orig>/sigma^2) u v^T (u, v constants); ws >= 2 KiB. */
int rgan_spectral_backward(const float* W, const float* dWeff, int rows, int cols,
                           long long rs, long long hs, int lo, const float* u, const float* v,
                           const float* inv_sigma, float* dW, int accumulate, void* ws, void* stream);

/* ---- Adam (torch/optim/adam.py:347-547, _single_tensor_adam semantics) ----
 * Updates `ntensors` tensors (any count; launched in chunks).  hyper = device double[8]:
 * {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} (doubles, as torch keeps them in
 * Python floats); step = device float[1], incremented once per call before use, like
 * state['step'].  Pointer arrays are host arrays of device pointers. */
int rgan_adam(int ntensors, float* const* params, const float* const* grads,
              float* const* exp_avg, float* const* exp_avg_sq, const long long* numel,
              const double* hyper, float* step, void* stream);
/* step[0] += 1 (the bump rgan_adam / rgan_adam_packed issue before the update). */
int rgan_adam_step_inc(float* step, void* stream);
/* rgan_adam that also writes the cached GEMM layouts of the weights it updates (what
 * rgan_conv_pack(d, which, w, packed) would produce from the new values), instead of a
 * repack pass reading every weight again after the step.  packs[i].tensor indexes the
 * params arrays; layouts the Adam kernel cannot write (non-contiguous weights, generic
 * packs) are repacked by their own launch after it, so every listed layout is current
 * when the call's work completes.  step = device float[2]: step[0] the count (as rgan_adam),
 * step[1] the call's arrival ticket (a uint32, 0 before the first call; left 0). */
typedef struct RganAdamPack {
  int tensor;
  int which;               /* 0 forward layout, 1 data-gradient layout (rgan_conv_pack) */
  const RganConv* d;       /* the descriptor the layout was packed for */
  float* packed;           /* rgan_conv_pack_floats(d, which) floats */
} RganAdamPack;
int rgan_adam_packed(int ntensors, float* const* params, const float* const* grads,
                     float* const* exp_avg, float* const* exp_avg_sq, const long long* numel,
                     const double* hyper, float* step, int npacks, const RganAdamPack* packs,
                     void* stream);
/* hyper[0] *= gamma (ExponentialLR.step, GLI:533-534,713-714). */
int rgan_lr_decay(double* hyper, double gamma, void* stream);

/* ---- data movement ---- */
/* out[b] = images[idx[b]] for per-image blocks of `per` floats (the real-batch draw,
 * GLI:176-178, 581-583, on a dataset resident in HBM). */
int rgan_gather_images(const float* images, const long long* idx, int batch, long long per,
                       float* out, void* stream);

/* ---- differentiable augmentation of D's inputs (--rgan_diffaug; no reference counterpart) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * One random colour / translation / cutout transform per sample, for every image D sees, and
 * its adjoint for the gradient that flows back to G.  x, y: [batch][channels][h][w] contiguous;
 * u: [batch][8] uniforms in [0, 1), columns 0..6 used (7 reserved).  policy: bit 1 colour,
 * bit 2 translation, bit 4 cutout; a disabled part takes its identity value.
 *   colour:      beta = u0 - 1/2, sat = 2 u1, con = u2 + 1/2 (identity 0, 1, 1);
 *                col(x)[c,i,j] = con (sat (x[c,i,j] - m_ij) + m_ij - mu) + mu + beta,
 *                m_ij = mean_c x[:,i,j], mu = mean_{c,i,j} x
 *   translation: R = floor(h/8 + 1/2), tx = min(floor(u3 (2R + 1)), 2R) - R; ty from u4 and w;
 *                sources outside the image read 0
 *   cutout:      K = floor(h/2 + 1/2), o = min(floor(u5 (h + 1 - K mod 2)), h - K mod 2), rows
 *                [o - floor(K/2), o - floor(K/2) + K - 1] of the output are 0; columns from u6, w
 *   adjoint = 0: y[c,i,j] = col(x)[c,i+tx,j+ty], or 0 inside the box / for a source outside
 *   adjoint != 0 (x is dy, y is dx): g = dy moved back (0 where nothing arrives), then
 *                dx = con (sat g + (1 - sat) mean_c g) + (1 - con) mean_{c,i,j} g
 * The sample mean is a two-stage sum through ws (rgan_diffaug_workspace floats, only written
 * with the colour bit) added in a fixed order: no atomics, two calls give the same bits.
 * Without the colour bit every output is a copied input value or 0.  y must not alias x.
 * 16-byte loads and stores when w % 4 == 0 and x, y are 16-byte aligned; any w, alignment and
 * channel count otherwise.  batch <= 65535, channels*h*w < 2^31. */
size_t rgan_diffaug_workspace(int batch, int channels, int h, int w);
int rgan_diffaug(const float* x, const float* u, int batch, int channels, int h, int w, int policy,
                 int adjoint, float* ws, float* y, void* stream);

/* ---- the same transform, each group applied with probability p (--rgan_aug_p, --rgan_ada_target) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * gate: [batch][4] uniforms in [0, 1); columns 0, 1, 2 gate colour, translation and cutout of
 * the sample (3 reserved).  p: one device double, read by the kernels at run time, so a call
 * captured in a HIP graph follows a p written between replays (rgan_ada_update moves it).
 * Group g of sample b is applied iff policy has its bit and gate[b][g] < (float)*p (strict:
 * p = 0 opens nothing, p = 1 everything; a NaN p opens nothing).  With m_b = policy restricted to
 * sample b's open groups, sample b's output equals bit for bit rgan_diffaug's for that sample
 * alone with policy m_b: the kernels are rgan_diffaug's own, compiled with the gate test, and the
 * split of the sample sum is unchanged.  So m_b = 0 copies the sample, and a sample whose colour
 * gate is closed is a pure move (the colour map with identity parameters would round); its
 * reduction blocks return before loading anything.  Workspace: rgan_diffaug_workspace.
 * Arguments as rgan_diffaug, plus gate and p non-null. */
int rgan_diffaug_p(const float* x, const float* u, const float* gate, const double* p, int batch,
                   int channels, int h, int w, int policy, int adjoint, float* ws, float* y,
                   void* stream);

/* ---- geometric groups of the same transform: x-flip, quarter turns, warp (--rgan_diffaug) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * policy in [0, 63]: bits 1, 2, 4 as rgan_diffaug, bit 8 xflip, bit 16 rot90 (needs h == w),
 * bit 32 warp.  v: [batch][8] uniforms in [0, 1): v0 flip, v1 quarter turns, v2 zoom, v3 angle,
 * v4..v6 the gates of xflip / rot90 / warp (read only with gate and p, which also gate colour /
 * translation / cutout as rgan_diffaug_p does), v7 reserved.  A cleared or closed group takes
 * its identity value.
 *   flip  = v0 >= 1/2                       torch.flip(., (3,))
 *   k     = min(floor(4 v1), 3)             torch.rot90(., k, (2, 3))
 *   s     = 2^((v2 - 1/2) / 2), theta = (2 v3 - 1) pi   (derived in double)
 *   y = cutout( translate( Warp( Rot90^k( Flip( col(x) ) ) ) ) ), the colour means those of x and
 *   the box tested at the output position.  With ci = (h-1)/2, cj = (w-1)/2, di = i + tx - ci,
 *   dj = j + ty - cj:
 *     r = ci + ( cos(theta) di + sin(theta) dj) / s,  c = cj + (-sin(theta) di + cos(theta) dj) / s
 *     Warp(z)[i,j] = sum over the four lattice neighbours q of (r, c) inside the image of
 *                    max(0, 1 - |r - q_r|) max(0, 1 - |c - q_c|) z[q]
 * Coordinates are computed in double.  A sample whose warp is closed, cleared or the identity
 * (v2 = v3 = 1/2) is moved by whole pixels: without the colour bit its outputs are copied inputs
 * or +0.0, with it the arithmetic is rgan_diffaug's.  adjoint != 0: the exact transpose of the
 * linear part, gathered over the at most 4 x 4 outputs that read a source pixel, in a fixed
 * order: no atomics, two calls give the same bits.  gate and p: both null (ungated) or both
 * non-null; exactly one null is RGAN_EINVAL, as are bit 16 with h != w and a policy outside
 * [0, 63].  With bits 8, 16, 32 clear the call is rgan_diffaug / rgan_diffaug_p (v unread).
 * Sizes, aliasing and workspace as rgan_diffaug (rgan_diffaug_geo_workspace floats). */
size_t rgan_diffaug_geo_workspace(int batch, int channels, int h, int w);
int rgan_diffaug_geo(const float* x, const float* u, const float* v, const float* gate, const double* p,
                     int batch, int channels, int h, int w, int policy, int adjoint, float* ws, float* y,
                     void* stream);

/* ---- adaptive augmentation probability (--rgan_ada_target; no reference counterpart) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * state = device double[4] {p, S, N, calls}; hyper = device double[4] {target, interval,
 * images_per_unit_p, reserved}.  Both are read on the device at run time: a captured call keeps
 * counting across graph replays and follows a hyper-parameter written between them.
 * rgan_ada_update: the rank statistic of one D step over rows i < n of the two output vectors,
 *   S += #(y_real[i] > y_fake[i]) - #(y_real[i] < y_fake[i]);  N += n
 * (a tie or a comparison with a NaN counts 0).  One launch of one block; the integer counts are
 * added in a fixed order without atomics, and S, N are integers held exactly in double, so shards
 * of a batch add exactly in any order.  With adjust != 0 the same launch then does what
 * rgan_ada_adjust does:
 *   calls += 1;  if (calls mod interval == 0 and N > 0) {
 *     r = S / N;  p = clamp(p + sgn(r - target) N / images_per_unit_p, 0, 1)  (sgn(0) = 0);  S = N = 0 }
 * all in double.  Null pointers and n <= 0 are refused (RGAN_EINVAL) without a launch. */
int rgan_ada_update(const float* y_real, const float* y_fake, int n, const double* hyper,
                    double* state, int adjust, void* stream);
int rgan_ada_adjust(const double* hyper, double* state, void* stream);

/* ---- LeCam regularisation of D (--rgan_lecam; Tseng et al., CVPR 2021; no reference counterpart) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * state = device double[4] {a_real, a_fake, calls, 0}; hyper = device double[4] {lambda, beta, start,
 * reserved}.  Both are read on the device at run time: a captured call keeps moving the anchors
 * across graph replays and follows a hyper-parameter written between them.
 * rgan_lecam, over rows i < n of D's outputs on this rank's real and generated batch (n_global = the
 * rows of all ranks, n on one rank; N below):
 *   w = calls >= start ? lambda : 0                                  (calls as the call finds it)
 *   L = w [ (1/N) sum (y_real[i] - a_fake)^2 + (1/N) sum (y_fake[i] - a_real)^2 ]
 *   dy_real[i] = (float)(2 w / N (y_real[i] - a_fake));  dy_fake[i] = (float)(2 w / N (y_fake[i] - a_real))
 * (the anchors are constants of the call; w == 0: L and both gradients are exact zeros, the launch
 * is the same).  mode 0 then moves the anchors on the batch means m_r = sum y_real / N, m_f =
 * sum y_fake / N and writes out[0] = L, out[1..3] = 0:
 *   calls == 0: a_real = m_r, a_fake = m_f;  else a = beta a + (1 - beta) m;   calls += 1
 * mode 1 (data parallel) leaves state alone and writes out = {sum y_real, sum y_fake,
 * sum (y_real - a_fake)^2, sum (y_fake - a_real)^2} of this rank's rows; the caller adds the ranks'
 * sums and rgan_lecam_finish forms L (into loss[0], which may be sums) and moves the anchors as
 * mode 0 does.  Either side may be absent (null y, and then a null dy): its part of L, its gradient
 * and the move of its own anchor (a_real for y_real) are left out, and calls += 1 goes with the
 * fake side, so a real-only call followed by a fake-only call counts one step (sides of
 * rgan_lecam_finish: 1 real, 2 fake, 3 both).  A dy may be null (no gradient wanted).  y and dy need
 * 4-byte alignment only.  All sums and the anchor arithmetic are double, one block adds in a fixed
 * order without atomics (two calls on the same inputs give the same bits), and a gradient element
 * is rounded once, from double to fp32.  Refused (RGAN_EINVAL) without a launch: n <= 0,
 * n_global < n, both y null, a dy given for an absent side, null hyper / state / out / sums / loss,
 * a mode other than 0 / 1, sides outside 1..3. */
int rgan_lecam(const float* y_real, const float* y_fake, int n, int n_global, const double* hyper,
               double* state, float* dy_real, float* dy_fake, double* out, int mode, void* stream);
int rgan_lecam_finish(const double* sums, int n_global, int sides, const double* hyper,
                      double* state, double* loss, void* stream);

/* ---- exponential moving average of G's weights (--rgan_ema_G; no reference counterpart) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * One call, over ntensors pairs (avg[j], params[j]) of numel[j] floats each:
 *   count[0] += 1;  t = count[0];
 *   beta_t = warmup ? min(beta, (1 + t) / (10 + t)) : beta          (double; the TF num_updates ramp)
 *   w = (float)(1 - beta_t);  avg = avg + w (params - avg)          (fp32, every element)
 * rounded as torch.lerp rounds: fma(w, params - avg, avg) for w < 1/2, fma(w - 1, params - avg,
 * params) otherwise, so w = 1 stores params itself.  hyper = device double[2] {beta, warmup (0 | 1)};
 * count = device float[1].  Both are read on the device at run time: a call captured in a HIP
 * graph follows the counter across replays, and a beta written into hyper between replays.
 * avg, params, numel: host arrays of device pointers / sizes (numel[j] >= 0).  params is only
 * read.  float4 accesses where avg[j] and params[j] are both 16-byte aligned, one float per lane
 * for other tensors and for a tail of numel[j] % 4.  12 B/element of HBM traffic.  Launches: the
 * one-thread count bump (rgan_adam_step_inc), then one per 48 tensors.  ntensors = 0: success,
 * nothing launched, count unchanged. */
int rgan_ema_update(int ntensors, float* const* avg, const float* const* params,
                    const long long* numel, const double* hyper, float* count, void* stream);

/* ---- live launch timing (bench.py roofline) ----
 * rgan_profile_begin(capacity): bracket each subsequent conv GEMM launch with HIP events
 * on its stream (up to `capacity` launches).  rgan_profile_end: wait, stop, return
 * summed GEMM time, summed algorithmic FLOPs (2*B*Cin*Cout*k*k*pixels per conv op) and
 * the launch count.  rgan_profile_kernel(i = 0, 1, ... until it returns RGAN_EINVAL): the same per kernel symbol. */
int rgan_profile_begin(int capacity);
int rgan_profile_end(double* total_ms, double* total_flops, long long* launches);
int rgan_profile_kernel(int idx, char* name, int name_len, double* ms, double* flops, long long* n);

/* GEMM arithmetic of the FAST 128x128 forward and data-gradient GEMMs (Conv and ConvT; the
 * weight gradients stay on the fp32 MFMA): 0 = fp32 MFMA (default),
 * 1 = fp32 emulated on the bf16 MFMA (each operand split exactly into three bf16 pieces,
 * the six products down to 2^-16 relative accumulated in fp32: per-product error <= 2^-23
 * relative, the fp32 rounding scale).  Also settable at load by RGAN_EMU_BF16X6=1.  Read
 * at launch time (a captured graph keeps the kernels it captured).  Returns the previous
 * setting, or -1 for a value other than 0 / 1.  No reference counterpart (an MI355X
 * arithmetic option; the reference computes fp32 on the CPU). */
int rgan_set_gemm_emulation(int on);

/* Library self-description: number of exported compute entry points, version string
 * (ends in "abi<RGAN_ABI_VERSION>"; rgan_abi_version() returns the number). */
int rgan_abi_version(void);
const char* rgan_version(void);

/* Device sampling (--rgan_rng device; replaces the draws of GLI:176,608,630,648-649,674):
 * Philox-4x32-10 keyed by `seed` at the device counter *counter, which the call advances
 * on the stream by the numbers it used (graph-replay safe).
 * rgan_rng_fill: out[0..n) ~ N(0, 1) (kind 0, Box-Muller) or U[0, 1) (kind 1).
 * rgan_rng_choice: n <= 4096 distinct indices of [0, N) (numpy.random.choice(N, n,
 * replace=False)'s distribution; Floyd's algorithm on one wave), int64.
 *
 * The stream (pinned bit for bit by tests/test_rng_gpu.py against tests/rng_ref.py): counter
 * value c yields the four 32-bit words w0..w3 = Philox-4x32-10(counter words (c lo, c hi, 0, 0),
 * key (seed lo, seed hi)); c runs modulo 2^64.
 *   fill, with base = *counter at the call: element 4q+i comes from counter base+q.
 *     kind 1: out[4q+i] = (w_i >> 8) 2^-24, a multiple of 2^-24 in [0, 1 - 2^-24]: never 1.
 *     kind 0: with U(w) = ((w >> 8) + 1) 2^-24 in (0, 1] (the logarithm never sees 0):
 *             out[4q] = r0 cos(2 pi U(w1)), out[4q+1] = r0 sin(2 pi U(w1)), r0 = sqrt(-2 ln U(w0));
 *             out[4q+2], out[4q+3] the same with w2 for the radius and w3 for the angle.
 *             |out| <= sqrt(48 ln 2) ~ 5.768 (U = 2^-24); U = 1 gives a pair of zeros.
 *     The call advances *counter by ceil(n / 4); a tail (n % 4 != 0) drops the last quad's
 *     unused elements.
 *   choice, with base = *counter: an integer below m from one counter's words is
 *     (((w1 << 32) | w0) m) >> 64.  Floyd: step s = 0..n-1 has j = N-n+s and t below j+1 from
 *     counter base+s; it picks t, or j if t is already picked.  Then a Fisher-Yates pass over the
 *     picks: for s = n-1 .. 1 swap positions s and k, k below s+1 from counter base+n+s.
 *     The call advances *counter by 2 n.
 * A refused call (RGAN_EINVAL: a null pointer, n < 0, kind other than 0 / 1, N <= 0, n > N,
 * n > 4096) and n = 0 (returns 0) launch nothing, write nothing and leave *counter unchanged. */
int rgan_rng_fill(float* out, long long n, int kind, unsigned long long seed, unsigned long long* counter,
                  void* stream);
int rgan_rng_choice(long long* out, int N, int n, unsigned long long seed, unsigned long long* counter,
                    void* stream);

/* ---- segmented key sort (csrc/sort.hip; the sliced Wasserstein metric's; no reference counterpart) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * rgan_sort_segments: nseg contiguous segments of len fp32 keys each, in[s len .. (s + 1) len), each
 * sorted ascending into out; keys only.  Order: the total order of the bit patterns, key(u) =
 * u ^ (u >> 31 ? 0xffffffff : 0x80000000) compared unsigned, so -0 < +0 and NaN patterns sort by
 * their bits (negative ones first, positive ones last); out holds the input's own bit patterns.
 * A least-significant-digit radix sort of 4 passes x 8 bits over tiles of rgan_sort_segments_tile()
 * keys (one block each): per pass a histogram per tile, one exclusive scan over (digit, tile) per
 * segment, and a stable scatter whose ranks come from wave ballots and scans, never from the order
 * in which atomics arrive: equal inputs give equal bits, run after run.  The passes go in -> tmp ->
 * out -> tmp -> out: tmp holds nseg len floats and is scratch; out may be in (in is read by the
 * first pass only), tmp may be neither.  in, out, tmp need 4-byte alignment only.  ws: at least
 * rgan_sort_segments_ws_bytes(nseg, len) bytes (256 uint32 per tile), 4-byte aligned.
 * Limits: nseg >= 1, len >= 1, nseg len < 2^31.  Anything else, a null pointer, tmp == in or out, or
 * a short ws is refused (RGAN_EINVAL) without a launch; the ws_bytes function answers 0 then. */
int rgan_sort_segments_tile(void);
size_t rgan_sort_segments_ws_bytes(int nseg, int len);
int rgan_sort_segments(const float* in, float* out, float* tmp, int nseg, int len, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- sliced Wasserstein distance over Laplacian-pyramid patches (csrc/swd.hip; --rgan_swd_every,
 * python -m relativisticgan_amd.evaluate; Karras et al., ICLR 2018, section 5; the reference's
 * quality metric is FID, code/fid.py, which needs a downloaded network) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * Images are planar fp32 [N][C][S][S] with values 0..255, 1 <= C <= 4.  Every entry point refuses
 * (RGAN_EINVAL, nothing launched) a null pointer, a size <= 0 and what its own lines add.
 *
 * rgan_swd_load_u8: out[n][c][y][x] = in[n s0 + c s1 + y s2 + x s3], strides = host long long[4] in
 * elements, each >= 0 (CHW datasets and the HWC output of rgan_images_to_u8 alike).
 *
 * rgan_swd_pyr_down: out [N][C][S/2][S/2] = the even rows and columns of in filtered with the 5x5
 * binomial [1 4 6 4 1]/16 x [1 4 6 4 1]/16, the border mirrored without repeating the edge
 * (-1 -> 1, -2 -> 2, S -> S - 2, S + 1 -> S - 3).  S a power of two >= 32; out must not be in.
 * rgan_swd_laplace: out = fine - up(coarse), fine and out [N][C][S][S], coarse [N][C][S/2][S/2]:
 * up puts coarse on the even positions of a zero image of side S, applies the same filter with the
 * same mirror rule to that image and multiplies by 4; the zero image is never formed.  out may be
 * fine (a thread reads only its own element of fine); it must not be coarse.  S as for pyr_down.
 * Both add their taps in double, rows then columns ascending, and round once to fp32.
 *
 * rgan_swd_positions: pos[i] = 3 + floor(u[i] (side - 6)) for i < n, u in [0, 1) as rgan_rng_fill
 * kind 1 draws it (a multiple of 2^-24: the product is formed exactly in integers; u outside
 * [0, 1) is clamped), so 3 <= pos <= side - 4.  side >= 7.
 *
 * rgan_swd_descriptors: for image n < N and patch p < P with centre (y, x) = pos[(n P + p) 2 + {0, 1}]
 * (int32; clamped to [3, S - 4], so no read leaves the image), row m = n P + p of desc [N P][K],
 * K = 49 C: desc[m][49 c + 7 dy + dx] = img[n][c][y + dy - 3][x + dx - 3], and part[n][c] = double
 * {sum, sum of squares} of the row values of channel c (part: N C 2 doubles).  S >= 7,
 * N P < 2^31.  One block per image; the sums are added in a fixed order.
 * rgan_swd_normalize: over M rows of desc and the nparts images' part (M 49 values per channel):
 * stats[c] = double {mean, population standard deviation} (stats: C 2 doubles), then in place
 * desc = (float)(((double)desc - mean) / std), each element rounded once.  A channel whose std is 0
 * becomes zeros.  The sums are finished by one block in a fixed order: equal inputs, equal bits.
 * rgan_swd_stats_ws_bytes(nparts, C): bytes of part followed by stats (0 for bad sizes).
 *
 * rgan_swd_unit_columns: dirs [K][D] in place, column d divided by its L2 norm (sum of squares in
 * double over ascending k, one rounding per element); a zero column stays.  K <= 196, D <= 512.
 * rgan_swd_project: proj[d][m] = sum_k desc[m][k] dirs[k][d], proj [D][M] (a direction's values
 * contiguous: the segments rgan_sort_segments takes).  fp32, one fused multiply-add per k in
 * ascending k from 0, through LDS tiles of 64 rows x 64 directions x 49 k.  M D < 2^31, K <= 196,
 * D <= 512.
 *
 * rgan_swd_l1: out[0] = sum_i |a[i] - b[i]| over n < 2^31 floats, in double: per-thread strided sums,
 * a block's threads, then the blocks, all in an order fixed by n.  ws: rgan_swd_l1_ws_bytes(n). */
int rgan_swd_load_u8(const uint8_t* in, int N, int C, int S, const long long* strides, float* out,
                     void* stream);
int rgan_swd_pyr_down(const float* in, int N, int C, int S, float* out, void* stream);
int rgan_swd_laplace(const float* fine, const float* coarse, int N, int C, int S, float* out,
                     void* stream);
int rgan_swd_positions(const float* u, long long n, int side, int* pos, void* stream);
size_t rgan_swd_stats_ws_bytes(int nparts, int C);
int rgan_swd_descriptors(const float* img, int N, int C, int S, int P, const int* pos, float* desc,
                         double* part, void* stream);
int rgan_swd_normalize(float* desc, long long M, int C, const double* part, int nparts,
                       double* stats, void* stream);
int rgan_swd_unit_columns(float* dirs, int K, int D, void* stream);
int rgan_swd_project(const float* desc, const float* dirs, int M, int K, int D, float* proj,
                     void* stream);
size_t rgan_swd_l1_ws_bytes(long long n);
int rgan_swd_l1(const float* a, const float* b, long long n, double* out, void* ws, size_t ws_bytes,
                void* stream);

/* ---- nearest training images and k-NN precision / recall in pixel space (csrc/nn.hip;
 * --rgan_nn_every, evaluate --rgan_nn; Kynkaanniemi et al., NeurIPS 2019; no counterpart in the
 * reference) ----
 * (additive within ABI revision 4: no existing entry point changed)
 * All arithmetic is integer and exact: equal inputs give equal outputs whatever the tiling or the
 * number of parts.  Every entry point refuses (RGAN_EINVAL, nothing launched) a null pointer, a size
 * < 1 and what its own lines add.
 *
 * A descriptor row is row_bytes int8: D = C s s values in (c, y, x) order, then zeros up to the next
 * multiple of 64.  rgan_nn_row_bytes(C, s) is that size, or 0 for what is refused: C outside 1..4,
 * s not in {8, 16, 32, 64}, or more than RGAN_NN_MAX_ROW_BYTES = 12288 bytes (so that a squared
 * distance, at most 255^2 12288 = 799 027 200, and every norm and dot product fit int32).
 *
 * rgan_nn_pack_u8: image n < N of in (uint8, element (n, c, y, x) at n s0 + c s1 + y s2 + x s3,
 * strides = host long long[4], each >= 0: CHW sets and HWC bytes alike) -> desc[n][row_bytes] and
 * norm[n].  With f = S / s (S % s == 0, 1 <= f <= 32) a descriptor value is
 * (sum of the f x f box + f f / 2) / (f f) - 128, the box mean with halves rounded up, shifted into
 * int8; norm[n] = the sum of the squared shifted values.  The pad bytes are written as 0.
 *
 * rgan_nn_topk: for query row q < Q of a (norms na) the k (1..8) nearest of the R rows of b (norms
 * nb): the k smallest keys (uint64(d2) << 32) | r, d2 = na[q] + nb[r] - 2 a[q].b[r], over the r
 * with r - q != self_offset (RGAN_NN_NO_SELF excludes nothing; self_offset = lo is leave-one-out
 * when a is rows lo.. of b).  dist[q][j], idx[q][j] ascend in j, ties by the smaller r; when fewer
 * than k rows remain the tail is dist = INT32_MAX, idx = -1.  a and b are 16-byte aligned, row_bytes
 * a multiple of 64 and <= 12288.  The rows of b are cut into nsplit contiguous parts (part p is
 * rows [p R / nsplit, (p + 1) R / nsplit); 0 = rgan_nn_topk_splits(Q, R), at most 4096), a block
 * takes 128 queries and one part and writes its k best keys to ws, and a second kernel merges the
 * parts; keys are distinct, so the result is the same for every nsplit.  ws: 8-byte aligned,
 * rgan_nn_topk_ws_bytes(Q, R, k, nsplit) bytes (0 for refused sizes; Q nsplit k must fit int).
 * The products come from v_mfma_i32_32x32x32_i8 over LDS tiles of 128 rows x 128 bytes.
 *
 * rgan_nn_covered: flag[q] = 1 when some r with r - q != self_offset has d2(q, r) <= radius[r],
 * else 0 (flag is zeroed on the stream first, then blocks that found one store 1: the same GEMM
 * body with another epilogue). */
#define RGAN_NN_MAX_ROW_BYTES 12288
#define RGAN_NN_NO_SELF (-0x7fffffffffffffffLL - 1)
size_t rgan_nn_row_bytes(int C, int s);
int rgan_nn_pack_u8(const uint8_t* in, int N, int C, int S, const long long* strides, int s,
                    int8_t* desc, int* norm, void* stream);
int rgan_nn_topk_splits(int Q, int R);
size_t rgan_nn_topk_ws_bytes(int Q, int R, int k, int nsplit);
int rgan_nn_topk(const int8_t* a, const int* na, int Q, const int8_t* b, const int* nb, int R,
                 int row_bytes, int k, long long self_offset, int nsplit, int* dist, int* idx, void* ws,
                 size_t ws_bytes, void* stream);
int rgan_nn_covered(const int8_t* a, const int* na, int Q, const int8_t* b, const int* nb,
                    const int* radius, int R, int row_bytes, long long self_offset, int* flag,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
