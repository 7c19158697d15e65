/*
 * ggan.h -- C ABI of libggan.so, the MI355X (gfx950) kernels behind the tflib.ops operator API
 * of zhenxuan00/graphical-gan.
 *
 * Boundary: the reference's Python operator constructors
 *   tflib/ops/conv2d.py:20 Conv2D, tflib/ops/deconv2d.py:20 Deconv2D, tflib/ops/linear.py:24 Linear,
 *   tflib/ops/batchnorm.py:6 Batchnorm, tflib/objs/gan_inference.py:28-119,307-358 objectives
 * hand their arithmetic to TensorFlow kernels (tf.nn.conv2d, tf.nn.conv2d_transpose, tf.matmul,
 * tf.nn.fused_batch_norm, tf.nn.sigmoid_cross_entropy_with_logits, AdamOptimizer, tf.gradients).
 * Each entry point below replaces one of those TF kernels (cited per function).
 *
 * Conventions
 *   - all tensors are dense fp32 in device memory; activations NCHW; the caller owns every buffer;
 *   - Conv2D filters HWIO [k][k][Cin][Cout]; Deconv2D filters [k][k][Cout][Cin] (reference layouts);
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*), allocates
 *     nothing, keeps no state between calls and is hipGraph-capturable;
 *   - `ws` is caller-provided scratch of at least ggan_*_workspace() bytes (may be NULL when 0).  Its first
 *     GGAN_WS_RESERVED bytes hold arrival counters of in-kernel split-K combines: the caller zeroes them ONCE when it
 *     allocates the workspace, every kernel leaves them zero; calls sharing a workspace must be stream-ordered;
 *   - return value 0 = ok, negative = error; ggan_last_error() gives the message (thread-local).
 */
#ifndef GGAN_H
#define GGAN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ggan_stream_t; /* hipStream_t */
#define GGAN_WS_RESERVED 16384

/* activation codes for fused epilogues and ggan_act_* */
enum { GGAN_ACT_NONE = 0, GGAN_ACT_LRELU = 1, GGAN_ACT_RELU = 2, GGAN_ACT_TANH = 3, GGAN_ACT_SIGMOID = 4 };

/* The ABI's version: changes whenever a struct layout or an entry point's meaning changes (500: ggan_conv_geom carries the launch plan,
 * ggan_prof_rec the grid; 600: a profiler record is one problem SHAPE -- (kernel, grid, flop per launch) --, ggan_noise_fill_steps is
 * gone; 700: ggan_gmm_posterior_assign / ggan_cluster_accuracy, the test-set pass; 800: ggan_gmm_latent_st_fwd / _bwd, the
 * straight-through MODE_K values).  A binding compares it with the header it was
 * written against before the first call. */
#define GGAN_ABI_VERSION 800
int ggan_version(void);
const char* ggan_last_error(void);
/* ---- convolution geometry ------------------------------------------------------------------
 * A strided cross-correlation y[N,Co,Ho,Wo] = conv(x[N,Ci,H,W], w[k,k,Ci,Co]) with explicit
 * top/left padding (TF 'SAME' puts the extra row/col at the bottom/right -- SURVEY.md A.1; the
 * caller computes pad_t/pad_l = pad_total/2, bottom/right padding is implied by Ho/Wo). */
typedef struct {
    int N, Ci, H, W;      /* the LARGE-spatial tensor (conv input / deconv output)  */
    int Co, Ho, Wo;       /* the SMALL-spatial tensor (conv output / deconv input)  */
    int k, stride, pad_t, pad_l;
    /* The launch plan travels with the call (round 4: these were process-wide setters; the library keeps no mutable state besides the
     * guarded profiler table and the caches of plan-time tables, so calls from several threads / streams do not interfere):
     *   plan_wgs         workgroups the forward / data-gradient launch plans for (tile size, split-K); 0 = default (200,
     *                    about one per CU: right for a launch that has the chip to itself).  A caller running TWO conv chains side
     *                    by side on two streams asks for ~128, so that each launch leaves CUs to the other chain.
     *   plan_wgs_filter  the same for the filter-gradient launch (0 = 256 split-K workgroups)
     *   plan_flags       GGAN_PLAN_PLAIN: the plain one-thread-per-output kernels (debug cross-check) */
    int plan_wgs, plan_wgs_filter, plan_flags;
} ggan_conv_geom;
#define GGAN_PLAN_PLAIN 1

/* tf.nn.conv2d(NCHW) + tf.nn.bias_add (tflib/ops/conv2d.py:106-120).  bias may be NULL.
 * act/alpha: optional fused pointwise epilogue (GGAN_ACT_NONE for reference behaviour). */
size_t ggan_conv2d_workspace(const ggan_conv_geom* g);
int ggan_conv2d_fwd(const ggan_conv_geom* g, const float* x, const float* w, const float* bias,
                    float* y, int act, float alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* Conv2DBackpropInput: gx[N,Ci,H,W] from gy[N,Co,Ho,Wo] (what tf.gradients derives from conv2d.py:106).
 * bias (len Ci, may be NULL) / act are a fused epilogue used by the Deconv2D forward. */
int ggan_conv2d_bwd_data(const ggan_conv_geom* g, const float* gy, const float* w, const float* bias,
                         float* gx, int act, float alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* Conv2DBackpropFilter: gw[k,k,Ci,Co]; gbias[Co] = sum over N,Ho,Wo of gy (BiasAddGrad), may be NULL. */
int ggan_conv2d_bwd_filter(const ggan_conv_geom* g, const float* x, const float* gy, float* gw,
                           float* gbias, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* Backward of a FUSED conv+bias+activation layer: the two gradients above computed from gy[i]*act'(y[i]) where y is the
 * layer's saved output, with the activation derivative applied while gy is staged (no separate pointwise pass and no
 * intermediate tensor) and the bias gradient produced by the filter-gradient kernel from the tiles it stages anyway. */
int ggan_conv2d_bwd_data_act(const ggan_conv_geom* g, const float* gy, const float* y, int y_act, float y_alpha,
                             const float* w, float* gx, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_conv2d_bwd_filter_act(const ggan_conv_geom* g, const float* x, const float* gy, const float* y, int y_act,
                               float y_alpha, float* gw, float* gbias, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* Filter gradient left as its split-K partial slabs, for a consumer that sums them anyway (ggan_pack_parts): saves the
 * reduce launch.  part[s*stride + i], s < *n_parts, i < 25*Ci*Co is slab s of gw; with_bias != 0 appends the Co
 * bias-gradient partials to every slab (i in [25*Ci*Co, 25*Ci*Co+Co)).  part_cap (floats) bounds the number of slabs.
 * Returns 1 when the geometry is not covered by the MFMA kernel (nothing written; use ggan_conv2d_bwd_filter_act). */
int ggan_conv2d_bwd_filter_parts(const ggan_conv_geom* g, const float* x, const float* gy, const float* y, int y_act,
                                 float y_alpha, int with_bias, float* part, size_t part_cap, int* n_parts,
                                 size_t* stride, ggan_stream_t stream);

/* tf.nn.conv2d_transpose + bias_add (tflib/ops/deconv2d.py:101-114) computed natively in NCHW (the two
 * layout transposes at :91/:116 are mathematically no-ops).  g describes the forward conv whose
 * input-gradient this is: x_small[N,Co,Ho,Wo] -> y_big[N,Ci,H,W]; w is the Deconv2D filter
 * [k,k,out=Ci,in=Co], which is bit-for-bit the HWIO filter of that forward conv. */
int ggan_deconv2d_fwd(const ggan_conv_geom* g, const float* x_small, const float* w, const float* bias,
                      float* y_big, int act, float alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_deconv2d_bwd_data(const ggan_conv_geom* g, const float* gy_big, const float* w, float* gx_small,
                           void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_deconv2d_bwd_filter(const ggan_conv_geom* g, const float* gy_big, const float* x_small, float* gw,
                             float* gbias /* [Ci], sum of gy_big */, void* ws, size_t ws_bytes,
                             ggan_stream_t stream);

/* Linear backward with the following activation's derivative folded into the operand load, so g' = g * act'(y) is never
 * written (replaces tf.matmul's MatMul gradients + the script's tf.maximum/LeakyReLU gradient + BiasAddGrad,
 * tflib/ops/linear.py:133-146).  x[M,K] layer input, w[K,N], y[M,N] the layer's activated output, g[M,N] = dL/dy.
 *   ggan_linear_bwd_data_act:   dx[M,K] = g' w^T
 *   ggan_linear_bwd_weight_act: dw[K,N] = x^T g',  db[N] = column sums of g' (db may be NULL) */
int ggan_linear_bwd_data_act(int M, int N, int K, const float* g, const float* y, int y_act, float y_alpha,
                             const float* w, float* dx, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_linear_bwd_weight_act(int M, int N, int K, const float* x, const float* g, const float* y, int y_act,
                               float y_alpha, float* dw, float* db, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* ggan_gemm with "concatenated" operands that are never concatenated (the critic's Linear on [conv features | z features],
 * gan_inference_cifar10.py:246-248 tf.concat + Linear, and its two gradients):
 *   A2 != NULL: op(A) = [A | A2] side by side along the SECOND stored dimension of A (k when ta == 0, m when ta == 1); the
 *               first a_split columns come from A (leading dimension a_split), the rest from A2 (leading dimension whole -
 *               a_split); a_split a multiple of 64 (of 16 where the product is one the skinny kernel takes) reads both in place, any
 *               other 0 < a_split < whole is staged side by side at
 *               the end of the workspace by one pointwise launch in front of the product (the mixture scripts' Linear on [z | k]
 *               with DIM_LATENT = 8, gmgan_inference_cifar10.py:74,236-237): the workspace must hold that matrix.
 *   C2 != NULL: output columns [0, c_split) go to C (leading dimension c_split), [c_split, N) to C2 (leading dimension N -
 *               c_split); no bias / activation / column sums with a split output.  c_split a multiple of 64 stores directly,
 *               any other 0 < c_split < N is dealt out of the workspace by one pointwise launch behind the product.  Not both
 *               A2 and C2 where either split is off the grid.
 *   colsum_b (may be NULL; tb == 0 only): column sums of B, as ggan_gemm_colsum. */
int ggan_gemm_split(int ta, int tb, int M, int N, int K, const float* A, const float* A2, int a_split, const float* B,
                    const float* bias, float* C, float* C2, int c_split, float* colsum_b, int act, float alpha, void* ws,
                    size_t ws_bytes, ggan_stream_t stream);

/* The state-space scripts' transition operator unrolled over a sequence, as ONE scan per direction
 * (/root/reference/ssgan_inference_moving_mnist.py:98-114 ImplicitOperator, :134-141 DynamicGenerator; 'res_w' variant:
 * ssgan_inference_chairs.py): z_{t+1} = Linear_out(lrelu(Linear_1(lrelu(Linear_in([z_t | eps]))))) + z_t   (zw == NULL)
 *                                      ... + z_t zw + b_zw                                                 (zw != NULL)
 * for t = 0 .. T-1 (T = LEN-1), one workgroup per sequence.  H (DIM_OP) must be 256, dl, dt <= 16.
 *   forward : zs[B, T+1, dl] (zs[:, 0] = z0), h1 / h2 [T, B, H] = the two hidden activations (kept for the backward).
 *   backward: from g_zs[B, T+1, dl] = d cost / d zs: the masked hidden-layer gradients G1, G2 [T, B, H], the gradient at every
 *             operator output Go[T, B, dl], the operator inputs Xin[T, B, dl+dt], d_z0[B, dl], d_eps[B, dt] (may be NULL).  The
 *             weight gradients are products over all T*B rows: dW_in = Xin^T G1, dW_1 = h1^T G2, dW_out = h2^T Go,
 *             dZW = Xin[:, :dl]^T Go, biases = column sums (ggan_gemm_colsum). */
int ggan_dyn_scan_fwd(int B, int T, int dl, int dt, int H, const float* z0, const float* eps, const float* w_in, const float* b_in,
                      const float* w_1, const float* b_1, const float* w_out, const float* b_out, const float* zw, const float* b_zw,
                      float alpha, float* zs, float* h1, float* h2, ggan_stream_t stream);
int ggan_dyn_scan_bwd(int B, int T, int dl, int dt, int H, const float* g_zs, const float* zs, const float* eps, const float* h1,
                      const float* h2, const float* w_in, const float* w_1, const float* w_out, const float* zw, float alpha, float* G1,
                      float* G2, float* Go, float* Xin, float* d_z0, float* d_eps, ggan_stream_t stream);

/* The tail of a critic as ONE op: Linear ([a1 | a2] -> H) + LeakyReLU(alpha) + Linear (H -> 1).
 * Replaces, for the joint critic, tf.concat + lib.ops.linear.Linear('Discriminator.zx1') + LeakyReLU +
 * lib.ops.linear.Linear('Discriminator.Output') (/root/reference/gan_inference_cifar10.py:246-254,
 * gmgan_inference_cifar10.py:294-300) and, with a2 == NULL, 'Discriminator.Hyper3' + 'Discriminator.HyperOutput'
 * (gmgan_inference_cifar10.py:288-291) and the state-space critics' last two layers.
 *   forward:  h[M,H] = lrelu([a1|a2] w + b) (kept: the backward's activation reference), logits[M] = h w_out + b_out.
 *             a1 [M,K1], a2 [M,K2] (NULL when K2 == 0; K1 a multiple of 64 otherwise), w [K1+K2,H], b [H], w_out [H], b_out [1].
 *   backward: from g[M] = d cost / d logits: gh[M,H] = g w_out^T * lrelu'(h) (caller-owned scratch), d_wout[H], d_bout[1],
 *             d_w[K1+K2,H], d_b[H], d_a1[M,K1], d_a2[M,K2]; every output pointer may be NULL (not wanted), d_b needs d_w,
 *             d_a2 goes with d_a1.  Launches: one head kernel + one grouped product launch.  g == NULL: gh (and d_wout / d_bout,
 *             which are then ignored here) were produced by ggan_bce_head_bwd -- only the products are launched. */
int ggan_critic_head_fwd(int M, int K1, int K2, int H, const float* a1, const float* a2, const float* w, const float* b,
                         const float* w_out, const float* b_out, float alpha, float* h, float* logits, void* ws, size_t ws_bytes,
                         ggan_stream_t stream);
int ggan_critic_head_bwd(int M, int K1, int K2, int H, const float* g, const float* a1, const float* a2, const float* w, const float* h,
                         const float* w_out, float alpha, float* gh, float* d_a1, float* d_a2, float* d_w, float* d_b, float* d_wout,
                         float* d_bout, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* The same head when its caller knows BEFORE it runs that its logits feed one sigmoid-cross-entropy cost
 * (/root/reference/tflib/objs/gan_inference.py:104-117: cost = sum_k w_k * reduce_mean(sigmoid_cross_entropy_with_logits(rows of term k,
 * label z_k)); terms = 1..4 consecutive row ranges covering the M logits): the gradient of that cost for a unit upstream gradient is
 * row-local, so the forward's tail launch also leaves g[M] = d cost / d logits and gh[M,H] = g w_out^T * lrelu'(h), and the backward's
 * product launch carries, as extra workgroups, what needs all rows: loss[0] (bit-identical to ggan_bce_logits_multi_fwd on the same
 * terms), d_wout[H] = h^T g, d_bout[1] = sum g.  One launch less per step on the chain  tail product -> logits -> cost -> head backward ->
 * products  than ggan_critic_head_fwd + ggan_bce_head_bwd + ggan_critic_head_bwd(g = NULL); same values bit for bit.  H <= 2048.
 * kind 0: sigmoid cross-entropy terms; kind 1: plain means (the Wasserstein costs of gan_inference.py:4-45, sum_k w_k * reduce_mean(rows of term k);
 * labels unused).  ext (backward only, may be NULL): ext[k] != NULL makes term k a value read THERE (term_rows[k] floats) instead of a row range -- the
 * one-element gradient penalty that a wali-gp critic cost adds (gan_inference_cifar10.py:365); such a term only enters loss[0].  The cost's value is
 * bit-identical to ggan_bce_logits_multi_fwd / ggan_mean_multi_fwd_grad on the same terms. */
int ggan_critic_head_fwd_bce(int M, int K1, int K2, int H, const float* a1, const float* a2, const float* w, const float* b,
                             const float* w_out, const float* b_out, float alpha, float* h, float* logits, int kind, int nterms,
                             const int* term_rows, const float* labels, const float* weights, float* g, float* gh, void* ws,
                             size_t ws_bytes, ggan_stream_t stream);
int ggan_critic_head_bwd_tail(int M, int K1, int K2, int H, const float* a1, const float* a2, const float* w, const float* h,
                              const float* w_out, float alpha, const float* gh, float* d_a1, float* d_a2, float* d_w, float* d_b,
                              float* d_wout, float* d_bout, const float* logits, const float* g, int kind, int nterms, const int* term_rows,
                              const float* labels, const float* weights, const float* const* ext, float* loss, void* ws, size_t ws_bytes,
                              ggan_stream_t stream);

/* ---- dense -------------------------------------------------------------------------------
 * C[M,N] = op(A) * op(B) (+ bias[N]) (+act), row-major, ta/tb = 1 reads the operand transposed
 * (A stored [K,M] / B stored [N,K]).  tf.matmul + bias_add of tflib/ops/linear.py:133-146 is
 * (ta=0,tb=0); its gradients are (0,1) for dX = dY*W^T and (1,0) for dW = X^T*dY. */
size_t ggan_gemm_workspace(int M, int N, int K);
int ggan_gemm(int ta, int tb, int M, int N, int K, const float* A, const float* B, const float* bias,
              float* C, int act, float alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* Same, plus colsum_b[n] = sum_k op(B)[k][n] from the B tiles the kernel stages anyway (tb must be 0): dW = X^T dY and
 * db = sum_rows dY of the Linear backward in ONE launch. */
int ggan_gemm_colsum(int ta, int M, int N, int K, const float* A, const float* B, float* C, float* colsum_b,
                     void* ws, size_t ws_bytes, ggan_stream_t stream);
/* out[c] = sum_r x[r,c] over a [rows,cols] matrix (BiasAddGrad of Linear). */
int ggan_colsum(const float* x, float* out, int rows, int cols, ggan_stream_t stream);
/* the same sum for tall matrices (Conv3D bias gradients: 10^5..10^6 rows): row slabs + a fixed-order second stage; ws = scratch */
int ggan_colsum_tall(const float* x, float* out, int rows, int cols, void* ws, size_t ws_bytes, ggan_stream_t stream);
/* out[c] = sum_{n,hw} x[n,c,hw] (BiasAddGrad NCHW).  ws: optional scratch (>= 4 KiB * C) enabling a chip-wide
 * two-stage reduction; with ws == NULL one workgroup per channel is used. */
int ggan_chansum(const float* x, float* out, int N, int C, int HW, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* ---- batch normalisation, training mode, batch statistics, biased variance -------------------
 * tf.nn.fused_batch_norm(NCHW, eps) (tflib/ops/batchnorm.py:29-30) for HW>1 and the
 * tf.nn.moments + tf.nn.batch_normalization branch (:74-87) as the HW=1 case over [N,C].
 * save_mean/save_invstd: [C] each, written by fwd and consumed by bwd. */
int ggan_bn_fwd_train(const float* x, const float* scale, const float* offset, float* y,
                      float* save_mean, float* save_invstd, int N, int C, int HW, float eps,
                      int act, float alpha, ggan_stream_t stream);
int ggan_bn_bwd(const float* x, const float* gy, const float* scale, const float* save_mean,
                const float* save_invstd, float* gx, float* gscale, float* goffset,
                int N, int C, int HW, ggan_stream_t stream);
/* same, with the activation fused into the forward (ggan_bn_fwd_train act != NONE) differentiated on load: gy is
 * dL/d(activated output y); no separate ggan_act_bwd pass.  gx_chansum (may be NULL; HW > 1 only) receives
 * sum_{n,h,w} gx per channel = the BiasAddGrad of the layer that feeds this BatchNorm, from the values in registers. */
int ggan_bn_bwd_act(const float* x, const float* gy, const float* y, int y_act, float y_alpha, const float* scale,
                    const float* save_mean, const float* save_invstd, float* gx, float* gscale, float* goffset,
                    float* gx_chansum, int N, int C, int HW, ggan_stream_t stream);

/* y = conv2d(x, w) * act'(yref), act' the derivative of the activation (ref_act, ref_alpha) that produced yref, taken at yref (as
 * ggan_act_bwd does): ggan_conv2d_fwd followed by ggan_act_bwd in one launch.  This is the backward of ggan_conv2d_bwd_data_act with
 * respect to its gy operand -- what the gradient-penalty pass of MODE wali-gp differentiates through (gan_inference_cifar10.py:353-364:
 * tf.gradients of a cost that contains tf.gradients(disc_hat, [x_hat])).  Returns 1, having launched nothing, where no kernel fuses
 * the mask for this geometry (filters other than 5x5 stride 2, split-K launches): the caller composes the two calls. */
int ggan_conv2d_fwd_masked(const ggan_conv_geom* g, const float* x, const float* w, float* y, const float* yref, int ref_act,
                           float ref_alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* Linear + Batchnorm([0]) + activation in one launch: the head of every Generator of the image scripts
 * (gan_inference_cifar10.py:134-138: Linear 'Generator.Input' -> Batchnorm 'Generator.BN1' over the batch axis -> relu).
 * x [M,K], w [K,N], b [N] (may be NULL); h [M,N] = x @ w + b (BatchNorm's input, kept for its backward), y [M,N] =
 * act(scale * (h - mean) * invstd + offset) with the batch statistics of the M rows, save_mean / save_invstd [N] as
 * ggan_bn_fwd_train leaves them (the backward is ggan_bn_bwd_act followed by the Linear layer's gradients).  Returns 1 when the
 * shape is not covered (M > 128 or not a multiple of 16, K > 256 or not a multiple of 4, N not a multiple of 32): nothing
 * written, use ggan_gemm + ggan_bn_fwd_train. */
int ggan_linear_bn_rows_fwd(const float* x, const float* w, const float* b, const float* scale, const float* offset, float* h,
                            float* y, float* save_mean, float* save_invstd, int M, int K, int N, float eps, int act,
                            float alpha, ggan_stream_t stream);
/* The backward of that head where its input needs no gradient (the generators' input is noise): ggan_bn_bwd_act over the rows + the
 * weight-gradient product x^T gh + its column sums in ONE launch (the last two launches of the Generator's backward chain, in front of
 * the step's pack + Adam launch).  gy [M,N] = d cost / d y, h / y / save_mean / save_invstd as the forward left them (y: the activation
 * reference, NULL for act == NONE); dw [K,N], db [N] (may be NULL), dscale [N], doffset [N].  Returns 1 when the shape is not covered
 * (K in {64, 128, 256}, M <= 128 in 16 equal row groups, N a multiple of 32): the caller composes ggan_bn_bwd_act + ggan_gemm_colsum. */
int ggan_linear_bn_rows_bwd(const float* x, const float* gy, const float* h, const float* y, const float* scale, const float* save_mean,
                            const float* save_invstd, float* dw, float* db, float* dscale, float* doffset, int M, int K, int N, int act,
                            float alpha, ggan_stream_t stream);

/* Second derivative of ggan_bn_bwd_act w.r.t. its inputs, for objectives that differentiate a network containing BatchNorm twice
 * (MODE vegan-wgan-gp: the gradient penalty on the latent critic, gan_inference_cifar10.py:305-317 with BN_FLAG = True).  h =
 * dL/d(gx).  Outputs: ggy = dL/d(gy), gx2 = dL/d(x) (all of it: through the batch statistics too), gscale2 = dL/d(scale).  The
 * fused activation must be piecewise linear (lrelu / relu / none). */
int ggan_bn_bwd_bwd(const float* x, const float* gy, const float* y, int y_act, float y_alpha, const float* h, const float* scale,
                    const float* save_mean, const float* save_invstd, float* ggy, float* gx2, float* gscale2, int N, int C, int HW,
                    ggan_stream_t stream);

/* Row-grouped training-mode BatchNorm over the whole chip (the state-space critics' [fake; real] batches, the 3dcnn critic's NDHWC
 * volumes read as [rows, C], the frame generators' [B*LEN, C, H, W] maps).  x [N, C, HW] (HW = 1: rows x channels); the leading
 * dimension is cut into `groups` equal contiguous parts, each normalised with its OWN batch statistics (biased variance, merged from
 * per-slab (count, mean, M2) by Chan's formula); scale / offset [C] are shared.  save_mean / save_invstd: [groups, C].  Three launches,
 * no atomics, fixed summation order (bit-identical run to run).  ws: the caller's workspace (GGAN_WS_RESERVED bytes skipped; needs
 * 12 * groups * C * (slabs + 1) bytes after it, a few hundred KB at most).  act: NONE / LRELU / RELU epilogue, as ggan_bn_fwd_train. */
int ggan_bn_split_fwd_train(const float* x, const float* scale, const float* offset, float* y, float* save_mean, float* save_invstd,
                            int N, int C, int HW, int groups, float eps, int act, float alpha, void* ws, size_t ws_bytes,
                            ggan_stream_t stream);
/* Its backward.  gy = dL/d(activated output); the activation (NONE / LRELU / RELU) is differentiated on load at the affine output
 * recomputed from x (no forward output kept).  gscale / goffset [C] (may be NULL: then neither is computed) are summed over all groups.
 * gx is written for the leading gx_groups groups only (0..groups; the rest is left untouched and, when gscale and goffset are NULL,
 * the trailing groups' gy is not read).  gx_chansum (may be NULL; HW > 1 only): sum of gx per channel over the written groups = the
 * bias gradient of the layer that feeds this BatchNorm. */
int ggan_bn_split_bwd_act(const float* x, const float* gy, int act, float alpha, const float* scale, const float* offset,
                          const float* save_mean, const float* save_invstd, float* gx, float* gscale, float* goffset,
                          float* gx_chansum, int N, int C, int HW, int groups, int gx_groups, void* ws, size_t ws_bytes,
                          ggan_stream_t stream);

/* Cross-replica ("sync") BatchNorm, SURVEY.md 8(e): statistics over the GLOBAL batch of `world` equal-sized replicas.  The
 * reference has no multi-GPU path; this is the mode under which N GPUs x B/N reproduce 1 GPU x B.  The host all-gathers the
 * 2*C floats each *_stats call produces ([2][C]: forward (mean, M2), backward (sum g, sum g*xhat)) into [world][2][C] and hands
 * them to the *_apply call, which merges them in rank order (bit-identical on every replica).  gscale / goffset are this
 * replica's own sums: the gradient exchange averages them with the other parameter gradients.  No second derivative. */
int ggan_bn_sync_stats(const float* x, float* stats, int N, int C, int HW, ggan_stream_t stream);
int ggan_bn_sync_apply(const float* x, const float* stats, int world, const float* scale, const float* offset, float* y,
                       float* save_mean, float* save_invstd, int N, int C, int HW, float eps, int act, float alpha,
                       ggan_stream_t stream);
int ggan_bn_sync_bwd_stats(const float* x, const float* gy, const float* y, int y_act, float y_alpha, const float* save_mean,
                           const float* save_invstd, float* sums, int N, int C, int HW, ggan_stream_t stream);
int ggan_bn_sync_bwd_apply(const float* x, const float* gy, const float* y, int y_act, float y_alpha, const float* scale,
                           const float* save_mean, const float* save_invstd, const float* sums, int world, int rank, float* gx,
                           float* gscale, float* goffset, int N, int C, int HW, ggan_stream_t stream);

/* ---- pointwise -------------------------------------------------------------------------------
 * LeakyReLU = tf.maximum(alpha*x, x) (gmgan_inference_cifar10.py:122-123), tf.nn.relu, tf.tanh,
 * tf.nn.sigmoid.  bwd takes the forward INPUT for lrelu/relu and the forward OUTPUT for
 * tanh/sigmoid in `ref`. */
int ggan_act_fwd(const float* x, float* y, size_t n, int act, float alpha, ggan_stream_t stream);
int ggan_act_bwd(const float* gy, const float* ref, float* gx, size_t n, int act, float alpha,
                 ggan_stream_t stream);
/* ggan_act_bwd that also emits the bias gradient of the layer as partial slabs: gx = gy * act'(ref) over [N, C, HW] and
 * parts[s*C + c] = sum of gx over channel c of the s-th image range, s < *n_parts (<= parts_cap / C); the slabs are summed by
 * ggan_pack_parts (stride C).  One launch for what tf.nn.bias_add's BiasAddGrad and the activation's gradient op are in the
 * backward of Deconv2D / Conv2D + activation (tflib/ops/deconv2d.py:110-116 followed by tf.nn.relu / tanh in the scripts). */
int ggan_act_bwd_chansum(const float* gy, const float* ref, float* gx, float* parts, int parts_cap, int* n_parts, int N, int C, int HW,
                         int act, float alpha, ggan_stream_t stream);
/* y = x + bias broadcast: NCHW bias[C] (HW>1) or [rows,C] (HW=1).  tf.nn.bias_add. */
int ggan_bias_add(const float* x, const float* bias, float* y, int N, int C, int HW, ggan_stream_t stream);
/* real_x = mul*(float(int32)/div - .5) (+ noise) (gmgan_inference_cifar10.py:342; face :242-243). */
int ggan_cast_scale_i32(const int32_t* x, const float* noise /* may be NULL */, float* y, size_t n,
                        float div, float mul, ggan_stream_t stream);
/* The same op reading its minibatch from a device-resident ring of `nslots` pre-staged minibatches of n int32 each: slot
 * (*ctr_a + *ctr_b + offset) mod nslots (either counter may be NULL).  The counters are device integers that other launches of
 * the step advance (the optimizers' step counts), so a replayed HIP graph walks the ring without a host-side copy of the next
 * minibatch into a staging buffer -- what the feed_dict of session.run is to the reference (gan_inference_cifar10.py:392-401),
 * with the data already in HBM. */
int ggan_cast_scale_ring_i32(const int32_t* ring, int nslots, const int32_t* ctr_a, const int32_t* ctr_b, int offset,
                             const float* noise /* may be NULL */, float* y, size_t n, float div, float mul, ggan_stream_t stream);
/* ggan_cast_scale_ring_i32 and the ggan_conv2d_fwd that reads its result, in ONE launch: real_x = 2*((tf.cast(real_x_int, tf.float32)/255.)-.5)
 * in front of lib.ops.conv2d.Conv2D('Extractor.1', 3, DIM, 5, ., stride=2) (/root/reference/gan_inference_cifar10.py:342,155-157).  The
 * scaled image x_out [N,Ci,H,W] is still written (the critic's input and the layer's filter gradient read it).  Returns 1 without
 * launching where the geometry is outside the thin-channel forward kernel (Ci <= 4, Co 32 | 64, k 5, stride 2): issue the two calls. */
int ggan_conv2d_fwd_cast_ring(const ggan_conv_geom* g, const int32_t* ring, int nslots, const int32_t* ctr_a, const int32_t* ctr_b, int offset,
                              const float* noise /* may be NULL */, float div, float mul, float* x_out, const float* w,
                              const float* bias /* may be NULL */, float* y, int act, float alpha, ggan_stream_t stream);
/* out[B,D] = k[B,K] mu[K,D] + noise[B,D] in one pointwise launch: HyperGenerator of the gmgan scripts, tf.add(tf.matmul(tf.cast(hyper_k,
 * tf.float32), com_mu), hyper_noise) (/root/reference/gmgan_inference_cifar10.py:150-153).  D a multiple of 4, buffers 16-byte aligned. */
int ggan_mix_mean(const float* k, const float* mu, const float* noise, float* out, int B, int K, int D, ggan_stream_t stream);
/* out = a*x + b*y (+c) elementwise (interpolates, residuals). */
int ggan_axpby(const float* x, const float* y, float* out, size_t n, float a, float b, float c,
               ggan_stream_t stream);
/* out[r,:] = x[r,:] + alpha[r]*(y[r,:]-x[r,:])  (gan_inference_cifar10.py:358-361). */
int ggan_row_lerp(const float* x, const float* y, const float* alpha, float* out, int rows, int cols,
                  ggan_stream_t stream);

/* ---- losses ----------------------------------------------------------------------------------
 * loss[0] = weight * mean_i( max(x,0) - x*z + log1p(exp(-|x|)) ), z = label (0 or 1)
 * (tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean, tflib/objs/gan_inference.py:85-101).
 * accumulate != 0 adds into loss[0] instead of overwriting. */
int ggan_bce_logits_fwd(const float* x, float label, float weight, float* loss, int n, int accumulate,
                        ggan_stream_t stream);
/* gx[i] = gloss[0]*weight*(sigmoid(x[i]) - z)/n */
int ggan_bce_logits_bwd(const float* x, float label, float weight, const float* gloss, float* gx, int n,
                        ggan_stream_t stream);
/* every term of one cost in a single launch: loss = sum_i weights[i] * mean(bce(xs[i], labels[i])), terms added in index
 * order (same result as one ggan_bce_logits_fwd per term with accumulate); the backward writes gxs[i] for every term. */
#define GGAN_BCE_MAX 16
int ggan_bce_logits_multi_fwd(const float* const* xs, const float* labels, const float* weights, const int* ns,
                              int count, float* loss, ggan_stream_t stream);
/* ggan_bce_logits_multi_fwd_grad AND the head kernel of ggan_critic_head_bwd in one launch, for a cost whose logits are the output
 * of ONE critic head (the terms xs[i] are consecutive row ranges of its logits[M], in order): loss and the unit-seed gradients gxs as
 * above, plus gh[M,H] = g w_out^T * lrelu'(h), d_wout[H] = h^T g, d_bout = sum g (d_wout / d_bout may be NULL) from the head's kept
 * activation h (gan_inference_cifar10.py:246-254 + tflib/objs/gan_inference.py:104-117).  M <= GGAN_HEAD_BCE_MAX_ROWS.  The products of
 * the head's backward follow with ggan_critic_head_bwd(g = NULL: gh is given). */
#define GGAN_HEAD_BCE_MAX_ROWS 2048
int ggan_bce_head_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count, float* loss,
                      float* const* gxs, int M, int H, const float* h, const float* w_out, float alpha, float* gh, float* d_wout,
                      float* d_bout, ggan_stream_t stream);
/* the same for a cost over the logits of up to GGAN_BCE_HEADS heads (the mixture scripts: joint critic + mixture critic,
 * gmgan_inference_cifar10.py:282-301): head a owns the next head_terms[a] terms; all arrays indexed by head (host arrays). */
#define GGAN_BCE_HEADS 2
int ggan_bce_heads_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count, float* loss,
                       float* const* gxs, int nheads, const int* head_terms, const int* Ms, const int* Hs, const float* const* hs,
                       const float* const* w_outs, const float* alphas, float* const* ghs, float* const* d_wouts /* entries may be NULL */,
                       float* const* d_bouts /* entries may be NULL */, ggan_stream_t stream);
int ggan_bce_logits_multi_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns,
                              int count, const float* gloss, float* const* gxs, ggan_stream_t stream);
/* forward AND the gradients for an upstream gradient of exactly 1 in one launch: gxs[i][j] = weights[i]*(sigmoid(x)-z)/n, bit for
 * bit what ggan_bce_logits_multi_bwd writes for gloss[0] == 1.  The cost of a train op is differentiated with a unit seed
 * (tf.gradients(cost, var_list), gan_inference.py:108-117), so the backward launch of the cost disappears from the step. */
int ggan_bce_logits_multi_fwd_grad(const float* const* xs, const float* labels, const float* weights, const int* ns,
                                   int count, float* loss, float* const* gxs, ggan_stream_t stream);
/* loss[0] (+)= weight*mean(x); bwd gx[i] = gloss[0]*weight/n  (wali_gp, gan_inference.py:29-30). */
int ggan_mean_fwd(const float* x, float weight, float* loss, int n, int accumulate, ggan_stream_t stream);
int ggan_mean_bwd(const float* gloss, float weight, float* gx, int n, ggan_stream_t stream);
/* every term of a Wasserstein cost in one launch: loss = sum_i weights[i]*mean(xs[i]) (terms added in index order, as
 * ggan_mean_fwd with accumulate), and -- gxs non-NULL -- the gradients for an upstream gradient of exactly 1,
 * gxs[i][:] = weights[i]/ns[i] (what ggan_mean_bwd writes for gloss[0] == 1).  count <= GGAN_BCE_MAX. */
int ggan_mean_multi_fwd_grad(const float* const* xs, const float* weights, const int* ns, int count, float* loss,
                             float* const* gxs /* may be NULL */, ggan_stream_t stream);

/* Conv3D of the '3dcnn' sequence critic (tflib/ops/conv3d.py:6-51: tf.nn.conv3d, data NDHWC [N,L,H,W,C], filter [fl,fs,fs,in,out],
 * strides (stride_len, stride, stride), SAME padding; ssgan_inference_moving_mnist.py:352-405).  The filter is already the [K, Co]
 * operand of a GEMM (K = fl*fs*fs*in, ordered (dl,dh,dw,ci)), so the layer is ggan_im2col3d followed by ggan_gemm (bias / activation in
 * its epilogue); the filter gradient is ggan_gemm(col^T, gy) and the data gradient ggan_col2im3d(ggan_gemm(gy, W^T)).
 * dims10 = {N, L, H, W, Ci, Co, fl, fs, stride_len, stride} (host array).
 *   col [N*Lo*Ho*Wo, K]: col[(n,ol,oh,ow)][(dl,dh,dw,ci)] = x[n, ol*sl+dl-pl, oh*s+dh-ph, ow*s+dw-pw, ci], 0 in the padding
 *   ggan_col2im3d is its adjoint (a gather: deterministic). */
int ggan_conv3d_out_shape(const int* dims10, int* lo_ho_wo);
int ggan_im2col3d(const int* dims10, const float* x, float* col, ggan_stream_t stream);
int ggan_col2im3d(const int* dims10, const float* col, float* gx, ggan_stream_t stream);
/* The same three products as implicit GEMMs (no patch matrix: the gathered operand is addressed in place, csrc/conv3d.hip):
 *   ggan_conv3d_fwd    y  = act(conv3d(x, w) + bias)                       (tflib/ops/conv3d.py:33-48)
 *   ggan_conv3d_wgrad  gw = d/dw  for an upstream gradient gy [N,Lo,Ho,Wo,Co] (already multiplied by act'(y))
 *   ggan_conv3d_dgrad  gx = d/dx  (one product per residue class of the input voxels, all classes in one launch)
 * ggan_conv3d_igemm_ok(dims10, kind) (kind 0 fwd, 1 filter grad, 2 data grad) returns 1 when the geometry is covered (Co % 4 == 0,
 * 32-bit sizes, every (row or column index) x (extent it is divided by) below 2^32 -- a volume 4096 wide with more than 256 output
 * rows of that width is not; data grad: Ci % 4 == 0, Ci >= 16, strides <= 2); the callers keep ggan_im2col3d / ggan_col2im3d + ggan_gemm for the
 * rest.  Operands 16-byte aligned; ws as for ggan_gemm (split of the reduction when the tile grid is small). */
int ggan_conv3d_igemm_ok(const int* dims10, int kind);
int ggan_conv3d_fwd(const int* dims10, const float* x, const float* w, const float* bias /* may be NULL */, float* y, int act,
                    float alpha, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_conv3d_wgrad(const int* dims10, const float* x, const float* gy, float* gw, void* ws, size_t ws_bytes,
                      ggan_stream_t stream);
int ggan_conv3d_dgrad(const int* dims10, const float* gy, const float* w, float* gx, ggan_stream_t stream);

/* Biased MMD^2 with a mixture of RBF kernels between two sets of codes X[m,d], Y[n,d] (MODE vegan-mmd:
 * tflib/objs/mmd.py:20-71 mix_rbf_mmd2(q_z, p_z, sigmas, wts, biased=True)): k(a,b) = sum_s wt_s exp(-||a-b||^2 / (2 sigma_s^2)),
 * out = mean k(X,X) + mean k(Y,Y) - 2 mean k(X,Y).  sigmas / wts are HOST arrays (wts may be NULL = all 1), ns <= 8, m + n <= 512.
 * row_scratch: m + n floats of device scratch.  Backward: gout = dL/d(out) (device scalar), dX / dY may be NULL. */
int ggan_mix_rbf_mmd2_fwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                          float* out, float* row_scratch, ggan_stream_t stream);
int ggan_mix_rbf_mmd2_bwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                          const float* gout, float* dX, float* dY, ggan_stream_t stream);
/* The unbiased estimator (tflib/objs/mmd.py:53-61, _mmd2 with biased=False) at the same sizes and with the same arguments: the diagonals of
 * the same-set blocks are left out and those blocks are averaged over m (m - 1) and n (n - 1) ordered pairs; m, n >= 2. */
int ggan_mix_rbf_mmd2_unbiased_fwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                                   float* out, float* row_scratch, ggan_stream_t stream);
int ggan_mix_rbf_mmd2_unbiased_bwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                                   const float* gout, float* dX, float* dY, ggan_stream_t stream);

/* The three pairwise kernel sums behind both MMD^2 estimators, at set sizes (tflib/objs/mmd.py:20-67: _mix_rbf_kernel's three Gram
 * matrices and _mmd2's sums, never materialised here): X[m,d], Y[n,d] row-major device fp32, any d >= 1, 1 <= m, n <= 131072, X == Y allowed;
 * sigmas / wts HOST arrays (wts may be NULL = all 1), ns <= 8.  sums3 (device, 3 doubles):
 *   [0] S_xx = sum_{i != j} k(x_i, x_j)   [1] S_yy = sum_{i != j} k(y_i, y_j)   [2] S_xy = sum_{i, j} k(x_i, y_j)
 * with k as above.  The reference's diagonal is the constant sum(wts) (mmd.py:52-54), so
 *   biased   = (S_xx + m sum(wts)) / m^2 + (S_yy + n sum(wts)) / n^2 - 2 S_xy / (m n)
 *   unbiased = S_xx / (m (m - 1)) + S_yy / (n (n - 1)) - 2 S_xy / (m n).
 * Gram tiles on the fp32 MFMA, distances / exponentials / sums in the tiles' epilogue; per-workgroup partials added in a fixed order in
 * double (no atomics: repeated calls give the same bits).  ws: ggan_mix_rbf_sums_workspace(m, n) bytes of 16-byte aligned device scratch
 * (linear in m + n; 0 = sizes out of range), all of it scratch -- no arrival counters.  Forward only. */
size_t ggan_mix_rbf_sums_workspace(int m, int n);
int ggan_mix_rbf_sums(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                      double* sums3, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* k-NN balls of row sets: the two primitives behind improved precision / recall (Kynkaanniemi et al. 2019, "Improved Precision and Recall
 * Metric for Assessing Generative Models") and density / coverage (Naeem et al. 2020, "Reliable Fidelity and Diversity Metrics for
 * Generative Models") -- evaluate.Evaluator.prdc_scores, functional.prdc.  Squared Euclidean distances D throughout, as
 * max(|a|^2 + |b|^2 - 2 a.b, 0) from fp32-MFMA Gram tiles; row-major device fp32, any d >= 1, 1 <= rows <= 131072.
 *   ggan_knn_radii:   r2[i] = the k-th smallest of { D(z_i, z_l) : l != i }, 1 <= k <= 8, k <= n - 1.  Row i itself is left out by INDEX,
 *                     a duplicate of it counts (a multiset order statistic: three equal rows have a k = 2 radius of 0).
 *   ggan_ball_counts: cnt[a] = #{ j : D(a_a, b_j) <= rB2[j] } (inclusive), min2[a] = min_j D(a_a, b_j), for the m rows of A against the n
 *                     rows of B with their squared radii rB2[n].
 * With X the real set (m rows), Y the generated one (n rows), rX = radii(X), rY = radii(Y), (cy, .) = ball_counts(Y, X, rX) and
 * (cx, mx) = ball_counts(X, Y, rY): precision = mean(cy > 0), density = sum(cy) / (k n), recall = mean(cx > 0), coverage = mean(mx <= rX).
 * ws: ggan_*_workspace bytes of 16-byte aligned device scratch (0 = arguments out of range), all of it scratch.  Per-row lists, integer
 * counts and minima only -- no floating-point atomics: repeated calls give the same bits.  Forward only. */
size_t ggan_knn_radii_workspace(int n, int k);
int ggan_knn_radii(const float* Z, int n, int d, int k, float* r2, void* ws, size_t ws_bytes, ggan_stream_t stream);
size_t ggan_ball_counts_workspace(int m, int n);
int ggan_ball_counts(const float* A, const float* B, int m, int n, int d, const float* rB2, int* cnt, float* min2, void* ws,
                     size_t ws_bytes, ggan_stream_t stream);

/* Labelled neighbour lists across two row sets: the primitive behind the k-NN accuracy of the codes (evaluate.Evaluator.knn_scores,
 * functional.knn_lists / knn_vote / knn_accuracy).  Q[m,d] queries, C[n,d] candidates, row-major device fp32, Q == C allowed, any d >= 1,
 * 1 <= m, n <= 131072; D(i,j) = max(|q_i|^2 + |c_j|^2 - 2 q_i.c_j, 0) from the Gram tiles of ggan_knn_radii.
 *   ggan_knn_lists: idx[i, 0..k) (int32 [m,k]) = the k candidates smallest under the TOTAL order (D(i,j), j), ascending: a tie in distance
 *                   goes to the lower candidate index, whatever the launch shape, so the result is unique.  d2 [m,k] (may be NULL) their
 *                   distances.  skip_diag != 0 (needs m == n) leaves out candidate j == i by INDEX; a duplicate of row i still counts.
 *                   1 <= k <= GGAN_KNN_MAX_K, k <= n - (skip_diag ? 1 : 0).  ws: ggan_knn_lists_workspace(m, n, k) bytes of 16-byte
 *                   aligned device scratch (0 = arguments out of range).  No floating-point atomics: repeated calls give the same bits.
 *   ggan_knn_vote:  pred[i] = the label that occurs most often among labels_c[idx[i, 0..k)], the SMALLEST such label on a tied vote: a
 *                   function of the label multiset, not of the order in the list.  Every idx value must index labels_c.  labels_q
 *                   (may be NULL) the queries' own labels: correct[0] += #{i : pred[i] == labels_q[i]} and
 *                   confusion[labels_q[i] * classes + pred[i]] += 1 (int32 [classes, classes], classes <= 1024; a pair with a label
 *                   outside 0 .. classes-1 is not counted); either may be NULL, the caller zeroes them.  Integer adds only.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
#define GGAN_KNN_MAX_K 8
size_t ggan_knn_lists_workspace(int m, int n, int k);
int ggan_knn_lists(const float* Q, const float* C, int m, int n, int d, int k, int skip_diag, int32_t* idx, float* d2, void* ws,
                   size_t ws_bytes, ggan_stream_t stream);
int ggan_knn_vote(const int32_t* idx, const int32_t* labels_c, const int32_t* labels_q, int m, int k, int classes, int32_t* pred,
                  int32_t* correct, int32_t* confusion, ggan_stream_t stream);

/* Parzen-window log-sums across two row sets: the primitive behind the Gaussian Parzen-window log-likelihood of held-out rows under a
 * kernel density fitted to generated ones (evaluate.Evaluator.parzen_scores, functional.parzen_lse / parzen_ll).  Q[m,d] queries, S[n,d]
 * samples, row-major device fp32, Q == S allowed, any d >= 1, 1 <= m, n <= 131072; D(i,j) = max(|q_i|^2 + |s_j|^2 - 2 q_i.s_j, 0) from the
 * Gram tiles of ggan_knn_radii; no row is left out.
 *   ggan_parzen_lse: lse[s, i] (fp32 [ns,m]) = log sum_j exp(-D(i,j) / (2 sigmas[s]^2)) for the ns bandwidths of the HOST array sigmas,
 *                    1 <= ns <= GGAN_PARZEN_MAX_SIGMAS, every one finite and positive.  The sums are carried shifted by the row's
 *                    running minimum distance (one minimum serves all bandwidths), so the result is finite for every finite input;
 *                    where only the nearest sample survives in fp32 it is -D_min / (2 sigma^2).  One pass over the Gram tiles.
 *                    ws: ggan_parzen_lse_workspace(m, n, ns) bytes of 16-byte aligned device scratch, linear in m + n (times ns)
 *                    (0 = arguments out of range).  Partial sums are combined in a fixed order, no floating-point atomics: repeated
 *                    calls give the same bits, and a bandwidth's value does not depend on the others in the call.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
#define GGAN_PARZEN_MAX_SIGMAS 16
size_t ggan_parzen_lse_workspace(int m, int n, int ns);
int ggan_parzen_lse(const float* Q, const float* S, int m, int n, int d, const float* sigmas /*host*/, int ns,
                    float* lse /*device [ns, m]*/, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* Reconstruction fidelity of image pairs: per-image mean squared error and mean structural similarity (Wang, Bovik, Sheikh, Simoncelli
 * 2004) of A[i] against B[i] (evaluate.Evaluator.rec_scores / SequenceEvaluator.rec_scores, functional.ssim_pairs).  A, B: row-major device
 * fp32 [n, c*h*w], channel-major planes -- the layout of [B, OUTPUT_DIM] rows and of [B, LEN, OUTPUT_DIM] with n = B*LEN --, A == B allowed;
 * 1 <= n <= 131072, 1 <= c <= 4, 11 <= h, w <= 64.  The pixel of input X in unit scale is u = scale_x * x + shift_x (tanh range: 0.5, 0.5;
 * sigmoid range: 1, 0; data in 0..255: 1/255, 0): the rescaling is in the formula, the data stay as the nets see them.
 *   mse[i]  = mean over c*h*w of (ua - ub)^2
 *   ssim[i] = mean over the c channels and the (h-10)*(w-10) valid window positions of
 *             ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = 0.01^2, C2 = 0.03^2 (data range 1),
 *             mx, my, sxx, syy, sxy the means, population variances and covariance under the separable 11x11 Gaussian window of
 *             sigma 1.5, normalised to sum 1 (scikit-image structural_similarity(gaussian_weights=True, sigma=1.5,
 *             use_sample_covariance=False), cropped by 5 on every side).  The second moments are taken of values CENTRED by each plane's
 *             mean, so that E[x^2] - mx^2 does not cancel on bright flat regions.
 * ws: ggan_ssim_pairs_workspace(n, c, h, w) bytes of 4-byte aligned device scratch (0 = arguments out of range): the per-plane sums, which a
 * second launch combines over the c planes of an image in index order.  Sums are reduced in a fixed order, no floating-point atomics:
 * repeated calls give the same bits, and an image's values depend neither on its neighbours nor on n.  Arguments out of range, a null
 * pointer or a short workspace return a negative code before any device work.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
size_t ggan_ssim_pairs_workspace(int n, int c, int h, int w);
int ggan_ssim_pairs(const float* A, const float* B, int n, int c, int h, int w, float scale_a, float shift_a, float scale_b, float shift_b,
                    float* mse /*[n]*/, float* ssim /*[n]*/, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* Least-squares linear probe: a ridge-regularised least-squares classifier on standardised rows, fitted in closed form
 * (evaluate.Evaluator.probe_scores, functional.lsq_probe_fit / lsq_probe_predict).  Z[n,d] row-major device fp32, y int32 labels in
 * [0, classes), 1 <= d <= GGAN_PROBE_MAX_DIM, 1 <= classes <= GGAN_PROBE_MAX_CLASSES, rows <= 131072 (the fit: n >= 2).
 *   ggan_probe_moments: mean[j] = mean_i z_ij, inv_std[j] = 1 / sqrt(mean_i (z_ij - mean_j)^2) -- 0 for a constant column, which so drops
 *                       out --, counts[c] = #{i : y_i == c}.  Two passes over the rows, the column sums in fp64 per block of
 *                       GGAN_PROBE_ROW_BLOCK rows and over the blocks in block order; the second pass centres with the fp64 mean.
 *                       status[0] is WRITTEN: GGAN_PROBE_BAD_LABEL if a label lies outside [0, classes) (it is never used as an index and
 *                       counted nowhere), GGAN_PROBE_NONFINITE if a mean or a variance is not finite, else 0.
 *   ggan_probe_normal:  G[d,d] = Zs^T Zs / n and R[d,classes] with R[:, c] = (1/n) sum_{i: y_i = c} zs_i, zs_i = (z_i - mean) * inv_std
 *                       formed in fp32 on the fly: neither Zs nor a one-hot label matrix exists in memory.  A block of GGAN_PROBE_ROW_BLOCK
 *                       rows is summed in fp32 in row order (v_mfma_f32_32x32x2_f32, d padded to a multiple of 32; instance t = ceil(d / 32)),
 *                       the block partials in fp64 in block order.
 *   ggan_probe_solve:   W[d,classes] = (G + ridge I)^-1 R by a Cholesky factorisation in fp64 in one workgroup's LDS, rounded once to
 *                       fp32; bias[c] = counts[c] / n.  ridge > 0.  status[0] |= GGAN_PROBE_NONFINITE for a non-finite entry of G or R,
 *                       GGAN_PROBE_BAD_PIVOT for a pivot that is not positive; W is then filled with NaN.
 *   ggan_probe_predict: pred[i] = argmax_c bias[c] + sum_j ((z_ij - mean_j) * inv_std_j) W[j,c], the LOWEST class on a tie (pred may be
 *                       NULL); with labels y and correct: correct[0] = #{i : pred[i] == y_i}, which the entry zeroes first (integer adds).
 * ws: ggan_probe_*_workspace(n, d, classes) bytes of 16-byte aligned device scratch (0 = arguments out of range).  No floating-point
 * atomics, every sum in a fixed order: repeated calls give the same bits.  Arguments out of range, a null pointer or a short workspace
 * return a negative code before any device work.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
#define GGAN_PROBE_MAX_DIM 128
#define GGAN_PROBE_MAX_CLASSES 32
#define GGAN_PROBE_ROW_BLOCK 256
#define GGAN_PROBE_BAD_LABEL 1
#define GGAN_PROBE_NONFINITE 2
#define GGAN_PROBE_BAD_PIVOT 4
size_t ggan_probe_moments_workspace(int n, int d, int classes);
int ggan_probe_moments(const float* Z, const int32_t* y, int n, int d, int classes, float* mean, float* inv_std, int32_t* counts,
                       int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);
size_t ggan_probe_normal_workspace(int n, int d, int classes);
int ggan_probe_normal(const float* Z, const int32_t* y, int n, int d, int classes, const float* mean, const float* inv_std, float* G,
                      float* R, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_probe_solve(const float* G, const float* R, const int32_t* counts, int n, int d, int classes, float ridge, float* W, float* bias,
                     int32_t* status, ggan_stream_t stream);
int ggan_probe_predict(const float* Z, const int32_t* y, int m, int d, int classes, const float* mean, const float* inv_std,
                       const float* W, const float* bias, int32_t* pred, int32_t* correct, ggan_stream_t stream);

/* The wide twin of the probe chain: the same classifier, the same status bits, 1 <= d <= GGAN_WPROBE_MAX_DIM (pixels, the Extractor's top
 * activations: functional.lsq_probe_fit_wide / lsq_probe_predict_wide, Evaluator.probe_scores with PROBE_WIDE).  classes, rows, n and ridge
 * as above; G[d,d], R[d,classes] and the factor are device fp64 (8-byte aligned).  The summation orders:
 *   ggan_wprobe_moments: as ggan_probe_moments for any d: a column's sum in fp64 in row order per block of GGAN_PROBE_ROW_BLOCK rows, the
 *                        blocks in block order.  status[0] is WRITTEN.
 *   ggan_wprobe_normal:  G and R in fp64.  One workgroup owns a pair (ti >= tj) of GGAN_WPROBE_TILE-column tiles and walks all row blocks:
 *                        a block of GGAN_PROBE_ROW_BLOCK rows in fp32 in row order (v_mfma_f32_32x32x2_f32, the rows standardised as they
 *                        are staged, columns past d as zeros), the blocks in fp64 in block order, / n.  No partial exists in memory; the
 *                        upper triangle is the mirrored store of the lower: G is exactly symmetric.
 *   ggan_wprobe_factor:  L L^T = G + ridge I in place on the lower triangle of G (the upper is left as it is), fp64, right-looking in
 *                        panels of GGAN_WPROBE_PANEL columns: the diagonal block column by column in one workgroup's LDS, the panel
 *                        below solved against it a row per thread, the trailing tiles updated by v_mfma_f64_16x16x4_f64.  No host
 *                        synchronisation.  status[0] |= GGAN_PROBE_BAD_PIVOT for a pivot that is not positive (the factorisation goes on
 *                        from a harmless one), GGAN_PROBE_NONFINITE for a non-finite entry.
 *   ggan_wprobe_solve:   W = L^-T L^-1 R: one workgroup per right-hand side, a blocked sweep in steps of GGAN_WPROBE_PANEL rows, fp64,
 *                        rounded once to fp32; bias[c] = counts[c] / n.  W is all NaN when status[0] carries GGAN_PROBE_NONFINITE or
 *                        GGAN_PROBE_BAD_PIVOT (raised by any launch before, or here by a non-finite entry of R).
 *   ggan_wprobe_predict: as ggan_probe_predict; a score is one fmaf chain in fp32 per chunk of GGAN_WPROBE_CHUNK columns (from the bias in
 *                        the first chunk), the chunks added in fp64 in chunk order; for d <= GGAN_WPROBE_CHUNK it is ggan_probe_predict's.
 * ws: ggan_wprobe_moments_workspace(n, d, classes) bytes of 16-byte aligned device scratch (0 = arguments out of range); the other entries
 * need none.  No floating-point atomics: repeated calls give the same bits.  Arguments out of range, a null or misaligned pointer or a
 * short workspace return a negative code before any device work.  Forward only.  Added without a version change. */
#define GGAN_WPROBE_MAX_DIM 4096
#define GGAN_WPROBE_TILE 64
#define GGAN_WPROBE_PANEL 64
#define GGAN_WPROBE_CHUNK 128
size_t ggan_wprobe_moments_workspace(int n, int d, int classes);
int ggan_wprobe_moments(const float* Z, const int32_t* y, int n, int d, int classes, float* mean, float* inv_std, int32_t* counts,
                        int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_wprobe_normal(const float* Z, const int32_t* y, int n, int d, int classes, const float* mean, const float* inv_std, double* G,
                       double* R, ggan_stream_t stream);
int ggan_wprobe_factor(double* G, int d, float ridge, int32_t* status, ggan_stream_t stream);
int ggan_wprobe_solve(const double* L, const double* R, const int32_t* counts, int n, int d, int classes, float* W, float* bias,
                      int32_t* status, ggan_stream_t stream);
int ggan_wprobe_predict(const float* Z, const int32_t* y, int m, int d, int classes, const float* mean, const float* inv_std,
                        const float* W, const float* bias, int32_t* pred, int32_t* correct, ggan_stream_t stream);

/* Frechet distance between Gaussians fitted to two row sets, |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) -- the "FD" of FID
 * (evaluate.Evaluator.frechet_scores, functional.frechet_moments / frechet_distance).  It stands in for the one number about samples the
 * reference publishes, tflib/inception_score.py (which needs a download), on the sets the reference draws as pictures in
 * gan_inference_cifar10.py:381-391; the features are the codes, or a fixed random projection of the pixels, not Inception's.
 *   ggan_frechet_moments:  mean[d] and cov[d,d] (divisor n - 1) of the device fp32 rows X[n,d], 2 <= n <= 131072, 1 <= d <=
 *                          GGAN_FRECHET_MAX_DIM, both in fp64.  The mean from fp64 sums per block of GGAN_PROBE_ROW_BLOCK rows, added in block
 *                          order; the covariance from rows centred by that fp64 mean (never E[x^2] - mean^2): a block's products are summed
 *                          in fp32 in row order (v_mfma_f32_32x32x2_f32, d padded to a multiple of 32; instance t = ceil(d / 32)), the block
 *                          partials in fp64 in block order, and the result is NOT rounded to fp32.  status[0] is WRITTEN:
 *                          GGAN_FRECHET_NONFINITE if a mean or an entry is not finite, else 0.
 *   ggan_frechet_distance: out[4] = { fd, |mu1 - mu2|^2, tr S1 + tr S2, 2 tr (S1 S2)^(1/2) } from device fp64 moments, in one workgroup, all
 *                          fp64: a diagonally pivoted Cholesky factorisation of S1 that tolerates a semi-definite matrix (once the largest
 *                          remaining pivot is at or below d eps tr S1 the remaining columns are zero), M = L^T S2 L, the eigenvalues of M by
 *                          two-sided Jacobi rotations in round-robin ordering, sum sqrt(max(lambda, 0)).  fd is NOT clipped at 0.  status[0]
 *                          is WRITTEN: GGAN_FRECHET_NONFINITE for a non-finite input (out is then NaN), GGAN_FRECHET_NOT_CONVERGED if the
 *                          off-diagonal norm of M is above 1e-14 of its Frobenius norm at the start after the fixed cap of sweeps, else 0.
 * ws: ggan_frechet_*_workspace(...) bytes of 16-byte aligned device scratch (0 = arguments out of range).  No floating-point atomics,
 * every sum in a fixed order: repeated calls give the same bits.  Arguments out of range, a null pointer or a short workspace return a
 * negative code before any device work.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
#define GGAN_FRECHET_MAX_DIM 128
#define GGAN_FRECHET_NONFINITE 1
#define GGAN_FRECHET_NOT_CONVERGED 2
size_t ggan_frechet_moments_workspace(int n, int d);
int ggan_frechet_moments(const float* X, int n, int d, double* mean, double* cov, int32_t* status, void* ws, size_t ws_bytes,
                         ggan_stream_t stream);
size_t ggan_frechet_distance_workspace(int d);
int ggan_frechet_distance(const double* mean1, const double* cov1, const double* mean2, const double* cov2, int d, double* out,
                          int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);

/* Sliced Wasserstein distance between two row sets, already projected onto L directions: PX[m,L] and PY[n,L] (device fp32, row-major;
 * direction l is column l, stride L; no alignment is assumed and L need be no multiple of anything), 1 <= m, n <= GGAN_SWD_MAX_ROWS,
 * 1 <= L <= GGAN_SWD_MAX_DIRS, p = 1 or 2 (evaluate.Evaluator.swd_scores, functional.sliced_wasserstein_projected / sliced_wasserstein).
 * Like the Frechet entries it stands in for the one number about samples the reference publishes, tflib/inception_score.py (which needs a
 * download): it compares the whole distributions in the full pixel space, with no kernel width, no Gaussian fit and no column cap.
 *   per[L]  (fp64) W_p^p(l) = the integral over t in (0, 1) of |F_a^-1(t) - F_b^-1(t)|^p between the empirical measures of column l of PX
 *           (mass 1/m a point) and of PY (mass 1/n a point): both columns sorted by a bitonic network in LDS (padded with +inf to a power of
 *           two), then, with point i of a owning [i n, (i+1) n) and point j of b owning [j m, (j+1) m) in units of 1/(m n), the sum over the
 *           overlapping pairs of (the integer overlap) |a_i - b_j|^p, over m n.  Equal sizes give mean_i |a_i - b_i|^p.  The differences of
 *           fp32 keys are exact in fp64; power, weights and sums are fp64, summed in an order fixed by sorted position.
 *   out[2]  (fp64) { (mean_l per[l])^(1/p), (max_l per[l])^(1/p) }: the sliced distance, and the largest distance over the given directions
 *           (a lower bound of the max-sliced distance).
 *   status[0] is WRITTEN: GGAN_SWD_NONFINITE if a value of PX or PY is NaN or +-inf -- per and out are then NaN, never a fault --, else 0.
 * ws: ggan_swd_workspace(m, n, L) bytes of 16-byte aligned device scratch, 4 L (m + n) rounded up (the transposed columns; 0 = arguments
 * out of range).  No floating-point atomics: the result depends on the multiset of each column only -- rows of PX or of PY permuted give the
 * same bits, as do repeated calls.  Arguments out of range, a null pointer, a misaligned fp64 output or a short or misaligned workspace
 * return a negative code before any device work.
 * Forward only.  Added without a version change: no existing entry point or struct is touched. */
#define GGAN_SWD_MAX_ROWS 16384
#define GGAN_SWD_MAX_DIRS 4096
#define GGAN_SWD_NONFINITE 1
size_t ggan_swd_workspace(int m, int n, int L);
int ggan_swd(const float* PX, const float* PY, int m, int n, int L, int p, double* per, double* out, int32_t* status, void* ws,
             size_t ws_bytes, ggan_stream_t stream);

/* A classifier's loss and the score of its posteriors (functional.SoftmaxXent / softmax_xent / class_score, classifier.ImageClassifier).
 * Both read device fp32 logits [rows, classes] row-major, 2 <= classes <= GGAN_CLS_MAX_CLASSES; one wavefront takes a row and one lane a
 * class.  fp32 inside a row (the maximum and the sum of exp(x - max) by a fixed butterfly over the wave, expf and logf at their accurate
 * forms), fp64 across rows (a wave's rows in row order, a workgroup's waves in wave order, the workgroups' partials by one finishing
 * workgroup in a fixed order).  No floating-point atomics: repeated calls give the same bits.
 *   ggan_softmax_xent_fwd_grad: tf.nn.softmax_cross_entropy_with_logits with one-hot labels, averaged over the rows (the reference's only use,
 *                       gmgan_inference_cifar10.py:392,402, is commented out; the library had no categorical cross-entropy), with its gradient
 *                       in the same launch.  labels int32 [B], 1 <= B <= 65536.
 *                       loss[0] = mean_b (log sum_c exp(x_bc - max_b) - (x_b,label - max_b)); dlogits[B,classes] = (softmax(x_b) - onehot) / B;
 *                       hits[0] = the rows whose argmax is their label, the LOWEST class on a tie; status[0] is WRITTEN: GGAN_CLS_BAD_LABEL if a
 *                       label lies outside [0, classes) (it is never an index: the row's one-hot is empty), GGAN_CLS_NONFINITE for a logit that
 *                       is NaN or +-inf, else 0.  With a status loss[0] is NaN; every row of dlogits is written all the same.
 *   ggan_class_score:   tflib/inception_score.py:47-53 from logits instead of posteriors (the frozen Inception graph of :56-90 is a download; the
 *                       caller brings its own classifier): split s of `splits` covers the rows [s N / splits, (s + 1) N / splits) in integer
 *                       division (:49), 1 <= splits <= GGAN_CLS_MAX_SPLITS, splits <= N <= 1048576, and
 *                       scores[s] = exp(mean_i sum_c p_ic (log p_ic - log pbar_c)), pbar = mean_i p_i, computed as exp(H(pbar) - mean_i H(p_i))
 *                       from sum_i sum_c p_ic log p_ic and the column sums sum_i p_ic of ONE sweep: log p is the log-softmax
 *                       (x - max) - log sum exp(x - max), never the log of a probability, and pbar log pbar is 0 at pbar = 0 -- where the
 *                       reference's np.log(part) (:50) turns an underflowed posterior into NaN, this stays finite.
 *                       stats[4] = { mean_s scores (:53), the population std over the splits (np.std, :53), mean_i H(p_i) over all rows,
 *                       H of the marginal over all rows }.  status[0] is WRITTEN: GGAN_CLS_NONFINITE for a logit that is NaN or +-inf -- scores
 *                       and stats are then all NaN --, else 0.  A workgroup of the sweep takes GGAN_CLS_ROW_BLOCK rows of one split.
 * ws: ggan_softmax_xent_workspace(B, classes) / ggan_class_score_workspace(N, classes, splits) bytes of 16-byte aligned device scratch (0 =
 * arguments out of range).  Arguments out of range, a null pointer or a short or misaligned workspace return a negative code before any
 * device work.
 * Added without a version change: no existing entry point or struct is touched. */
#define GGAN_CLS_MAX_CLASSES 64
#define GGAN_CLS_MAX_SPLITS 64
#define GGAN_CLS_ROW_BLOCK 256
#define GGAN_CLS_BAD_LABEL 1
#define GGAN_CLS_NONFINITE 2
size_t ggan_softmax_xent_workspace(int B, int classes);
int ggan_softmax_xent_fwd_grad(const float* logits, const int32_t* labels, int B, int classes, float* loss, float* dlogits, int32_t* hits,
                               int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);
size_t ggan_class_score_workspace(int N, int classes, int splits);
int ggan_class_score(const float* logits, int N, int classes, int splits, float* scores, float* stats, int32_t* status, void* ws,
                     size_t ws_bytes, ggan_stream_t stream);

/* k-means fitted on the device, and the two scores read off a fitted partition (functional.kmeans_* / bin_test / cluster_scores,
 * evaluate.Evaluator.kmeans_scores).  Nothing of this exists in the reference.  Rows X [n, d] and centres C [k, d] are device fp32,
 * row-major, 1 <= n <= 131072, any d >= 1 (a width that is no multiple of 4 or a base that is not 16-byte aligned takes the scalar
 * loads of the sweep), 1 <= k <= GGAN_KMEANS_MAX_K.  Squared Euclidean distances in float32 Gram form |x|^2 + |c|^2 - 2 x.c clamped at 0.
 * No floating-point atomics, no result depends on the launch shape: repeated calls give the same bits.  No host synchronisation inside.
 *   ggan_kmeans_seed    k-means++ from k uniforms u [k] (device fp64, in [0, 1), drawn by the caller): centre 0 is row floor(u[0] n);
 *                       centre t the first row, in row order, whose running fp64 sum of mind exceeds u[t] * total, mind[r] the smallest
 *                       distance of row r to the centres chosen so far; a total of 0 (every row coincides with a centre): row
 *                       floor(u[t] n).  centres [k, d] = the rows, idx int32 [k] their indices.  The picked index stays on the device.
 *   ggan_kmeans_pick    that pick alone, for a given mind float32 [n] and one uniform u[0]: idx[0].
 *   ggan_kmeans_assign  assign int32 [n] = the nearest centre, a tie in distance to the LOWER centre index; dist float32 [n] that distance;
 *                       inertia (may be NULL) = the sum of dist in fp64, a fixed order; prev (may be NULL; may BE assign) an earlier
 *                       assignment: moved[0] is WRITTEN, the rows whose centre changed (all n without prev; moved may be NULL without
 *                       prev); counts (may be NULL) int32 [k]: counts[c] += the rows assigned to c -- ADDED, the caller zeroes them, so that
 *                       slabs of one set accumulate.  status[0] is WRITTEN: GGAN_KMEANS_NONFINITE if the squared norm of a row or of a
 *                       centre, or a distance, is NaN or +-inf (the assignment is then still an index below k, and nothing faults), else 0.
 *   ggan_kmeans_update  centres[c] = the mean of the rows with assign == c, counts int32 [k] WRITTEN; an empty cluster keeps the centre it
 *                       had (centres are in / out).  Blocks of GGAN_KMEANS_ROW_BLOCK rows are summed in fp32 in row order, the blocks in
 *                       fp64 in block order.  An assignment outside [0, k) belongs to no cluster.
 *   ggan_kmeans_fit     seed, then `iters` times (assign, update), then a final assign; 0 <= iters <= GGAN_KMEANS_MAX_ITERS, a fixed count:
 *                       inertia double [iters + 1] and moved int32 [iters + 1] are those of every assign (moved[0] = n), moved[iters] == 0
 *                       says it converged; counts are those of the final assignment; status as ggan_kmeans_assign, over all of them.
 *   ggan_bin_test       NDB (Richardson & Weiss 2018) of two histograms int32 [k]: out[0] = the bins whose two-proportion z statistic
 *                       |p1 - p2| / se, se = sqrt(P (1 - P) (1/N1 + 1/N2)), exceeds z_threshold (a bin with se == 0 does not differ),
 *                       out[1] = out[0] / k, out[2] = the Jensen-Shannon divergence of the two histograms in nats, 0 log 0 = 0; fp64, one
 *                       workgroup, sums in bin order.  An empty histogram gives NaN.
 *   ggan_cluster_scores assign, labels int32 [n] -> table int32 [k, classes] (WRITTEN, integer atomics), out[0] = purity = the sum over
 *                       clusters of the largest cell over n, out[1] = NMI = I(U; V) / ((H(U) + H(V)) / 2), 1 when both entropies are 0;
 *                       1 <= classes <= GGAN_KMEANS_MAX_CLASSES.  status[0] is WRITTEN: GGAN_KMEANS_BAD_INDEX for a label outside
 *                       [0, classes) or an assignment outside [0, k) (never an index; out is then NaN), else 0.
 * ws: ggan_kmeans_workspace(n, d, k) bytes of 16-byte aligned device scratch, the same for seed, assign, update and fit (0 = arguments out
 * of range); its largest part, the update's block partials, is ceil(n / GGAN_KMEANS_ROW_BLOCK) k d floats.  Arguments out of range, a null
 * pointer or a short or misaligned workspace return a negative code before any device work.
 * Added without a version change: no existing entry point or struct is touched. */
#define GGAN_KMEANS_MAX_K 128
#define GGAN_KMEANS_MAX_CLASSES 32
#define GGAN_KMEANS_ROW_BLOCK 512
#define GGAN_KMEANS_MAX_ITERS 1000
#define GGAN_KMEANS_NONFINITE 1
#define GGAN_KMEANS_BAD_INDEX 2
size_t ggan_kmeans_workspace(int n, int d, int k);
int ggan_kmeans_seed(const float* X, int n, int d, int k, const double* u, float* centres, int32_t* idx, void* ws, size_t ws_bytes,
                     ggan_stream_t stream);
int ggan_kmeans_pick(const float* mind, int n, const double* u, int32_t* idx, ggan_stream_t stream);
int ggan_kmeans_assign(const float* X, const float* C, int n, int d, int k, const int32_t* prev, int32_t* assign, float* dist, double* inertia,
                       int32_t* moved, int32_t* counts, int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_kmeans_update(const float* X, const int32_t* assign, int n, int d, int k, float* centres, int32_t* counts, void* ws, size_t ws_bytes,
                       ggan_stream_t stream);
int ggan_kmeans_fit(const float* X, int n, int d, int k, int iters, const double* u, float* centres, int32_t* idx, int32_t* assign,
                    int32_t* counts, double* inertia, int32_t* moved, int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_bin_test(const int32_t* counts_ref, const int32_t* counts_test, int k, double z_threshold, double* out, ggan_stream_t stream);
int ggan_cluster_scores(const int32_t* assign, const int32_t* labels, int n, int k, int classes, int32_t* table, double* out, int32_t* status,
                        ggan_stream_t stream);

/* Stochastic encoder head, TYPE_Q = 'learn_std' (gan_inference_cifar10.py:173-188): std = exp(log_std), z = mean + eps * std; the backward
 * takes the gradients arriving at z and at std (either may be NULL). */
int ggan_reparam_fwd(const float* mean, const float* log_std, const float* eps, float* z, float* std_out, size_t n, ggan_stream_t stream);
int ggan_reparam_bwd(const float* gz, const float* gstd, const float* eps, const float* std_in, float* gmean, float* glog_std, size_t n,
                     ggan_stream_t stream);

/* tflib/objs/kl_aggregated.py:46-74 (MODE vegan-kl / vegan-ikl / vegan-jsd): Monte-Carlo divergence between the aggregated posterior -- the
 * equal-weight mixture of the minibatch's nx diagonal Gaussians (mu, sd: [nx, d]) -- and the N(0, I) prior (gan_inference_cifar10.py:269-270).
 * kind 0: KL(q||p) on nz samples of q (k_onehot [nz, nx] one-hot component draws, eps_q [nz, d]; z = k @ mu + (k @ sd) * eps, :6-16);
 * kind 1: KL(p||q) on the nz prior samples z_p [nz, d]; kind 2: JSD on both sets, the mixture m built from the nx components and n_coms
 * copies of the prior term (:31-44).  out: device scalar.  Z [ns, d], A [ns, nx], Bv [ns], T [ns] (ns = nz, or 2 nz for kind 2) are
 * caller-owned buffers the forward fills and the backward reads; W [ns, nx] and GZ [nz, d] are backward scratch.  gout: device scalar. */
int ggan_agg_div_fwd(int kind, const float* mu, const float* sd, const float* k_onehot, const float* eps_q, const float* z_p, int nx, int nz,
                     int d, int n_coms, float* out, float* Z, float* A, float* Bv, float* T, ggan_stream_t stream);
int ggan_agg_div_bwd(int kind, const float* mu, const float* sd, const float* k_onehot, const float* eps_q, int nx, int nz, int d, int n_coms,
                     const float* Z, const float* A, const float* Bv, const float* gout, float* W, float* GZ, float* gmu, float* gsd,
                     ggan_stream_t stream);

/* All the noise of one session.run in one launch: up to GGAN_NOISE_MAX device tensors, each filled with kind 0 = a + b*N(0,1),
 * 1 = uniform on (a, b) for a = 0 and on [a, b] otherwise (the draw u lies in [2^-25, 1 - 2^-24]; a + (b - a) u may round onto an end when
 * a != 0), 2 = one-hot rows of width `widths[i]` with a uniformly drawn index (the prior's k ~ Cat(1/K)).  Replaces
 * tf.random_normal / tf.random_uniform / Categorical.sample + one_hot of the scripts (gmgan_inference_cifar10.py:115-120,344-346;
 * gan_inference_cifar10.py:353-357).  state = {seed, draw number, arrival counter} (3 x uint64 in DEVICE memory, arrival counter
 * zero): Philox4x32-10 keyed by the seed; the draw number is advanced on the device, so a captured HIP graph yields new noise on
 * every replay.  Same seed + draw number => same values on every box. */
#define GGAN_NOISE_MAX 16
int ggan_noise_fill(float* const* dsts, const size_t* sizes, const int* kinds, const float* a, const float* b, const int* widths,
                    int count, uint64_t* state, ggan_stream_t stream);
/* Mixture-of-Gaussians latent glue of the gmgan scripts (HyperExtractor, gmgan_inference_cifar10.py:156-173 with MODE_K =
 * 'CONCRETE'): logits[b,j] = -.5*||z_b - mu_j||^2 + log_pi and k[b,:] = softmax((logits[b,:] + gumbel(u[b,:])) / temp), gumbel(u) =
 * -log(-log(u + 1e-20) + 1e-20) (:117-120).  One launch instead of the dozen [B,K] / [B,K,D] pointwise ops of the TF graph.
 * logits may be NULL (not fetched).  Backward: g_logits / g_k are dL/dlogits, dL/dk (either may be NULL); dz / dmu may be NULL.
 * K, B <= 256. */
int ggan_gmm_latent_fwd(const float* z, const float* mu, const float* gumbel_u, float* logits, float* k, int B, int K, int D,
                        float log_pi, float temp, ggan_stream_t stream);
int ggan_gmm_latent_bwd(const float* z, const float* mu, const float* k, const float* g_logits, const float* g_k, float* dz,
                        float* dmu, int B, int K, int D, float temp, ggan_stream_t stream);
/* The straight-through MODE_K values of HyperExtractor (gmgan_inference_cifar10.py:164-171, the same lines in the mnist / svhn
 * scripts), replacing its softmax / argmax / one_hot / stop_gradient ops with one launch per direction; logits as above.
 *   GGAN_MODE_K_STC (MODE_K = 'STRAIGHT_THROUGHT_CONCRETE', :164-167): soft[b,:] = s = the CONCRETE softmax of (logits + gumbel(u)) / temp,
 *     h = one_hot(argmax_j s[b,j]), k = (h - s) + s.  The argmax runs over the float32 s, the first index on a tie.
 *   GGAN_MODE_K_ST (MODE_K = 'STRAIGHT_THROUGHT', :169-171): h = one_hot(argmax_j logits[b,j]), k = (h - logits) + logits; gumbel_u,
 *     soft and temp are not read (the script draws no noise and defines no TEMP in this mode).
 *   k is TF's float32 stop_gradient(h - v) + v, a subtraction then an addition: 0 where h = 0, fl(fl(1 - v) + v) at the argmax.
 * Backward (mode as in the forward): STC is ggan_gmm_latent_bwd on soft (the gradient flows through the softmax, not through h);
 * ST passes g_k to the logits unchanged, dlogits = g_logits + g_k (soft, temp not read).  NULL rules and K, B <= 256 as above. */
enum { GGAN_MODE_K_CONCRETE = 0, GGAN_MODE_K_STC = 1, GGAN_MODE_K_ST = 2 };
int ggan_gmm_latent_st_fwd(const float* z, const float* mu, const float* gumbel_u, float* logits, float* k, float* soft, int B, int K,
                           int D, float log_pi, float temp, int mode, ggan_stream_t stream);
int ggan_gmm_latent_st_bwd(const float* z, const float* mu, const float* soft, const float* g_logits, const float* g_k, float* dz,
                           float* dmu, int B, int K, int D, float temp, int mode, ggan_stream_t stream);
/* The test-set pass of the gmgan scripts (gmgan_inference_mnist.py:338 q_k_probs = tf.nn.softmax(q_k_logits), :511-529 the clustering
 * accuracy), one launch per minibatch of B rows that are rows row0 .. row0+B-1 of the test set:
 *   logits[b,j] = -.5*||z_b - mu_j||^2 + log_pi  (summed as ggan_gmm_latent_fwd sums them: the same bits), p = softmax(logits) with no
 *   Gumbel noise and no temperature; probs[b,:] = p (probs: [B,K] of THIS launch, may be NULL); assign[row0+b] = argmax_j p (first index
 *   on a tie, np.argmax(prob_c, axis=1)); colbest[j] = max over every row seen of (float bits of p[b,j]) << 32 | (0xFFFFFFFF - row):
 *   the running column argmax, lowest row on a tie (np.argmax(prob_c, axis=0)).  The caller zeroes colbest at the start of a pass.
 *   K <= GGAN_POSTERIOR_MAX_K, any B.
 * ggan_cluster_accuracy then propagates labels and counts: label_of[j] = labels[0xFFFFFFFF - (colbest[j] & 0xFFFFFFFF)],
 *   correct[0] = #{b < N : label_of[assign[b]] == labels[b]} (:518-528; a component no row is assigned to keeps its label and never
 *   matches; a column whose probabilities all underflowed to 0 decodes to row 0, as np.argmax does). */
#define GGAN_POSTERIOR_MAX_K 8192
int ggan_gmm_posterior_assign(const float* z, const float* mu, float log_pi, int B, int K, int D, int row0, float* probs,
                              int32_t* assign, uint64_t* colbest, ggan_stream_t stream);
int ggan_cluster_accuracy(const int32_t* assign, const int32_t* labels, const uint64_t* colbest, int N, int K, int32_t* correct,
                          ggan_stream_t stream);
/* The frame sheets of the state-space scripts' video passes (ssgan_inference_moving_mnist.py:568-618 vis / generate_video /
 * reconstruct_video / disentangle), one launch per sheet, each pixel read once:
 *   gen  [n, LEN, C, H, W] generated frames in [-1, 1]: q = trunc(((x + 1) * a) * b), each product rounded to float32 on its own;
 *   data [n, LEN, C*H*W] sequences as the feed holds them (real_x_unit): q = trunc(x * d); q clamped to 0..255.
 *   Sources: gen alone, data alone, or both with interleave != 0 (sheet row 2i = data i, row 2i + 1 = generated i);
 *   rows = n, or 2n when interleaved.
 *   sheet [rows*H, LEN*W, C] bytes: save_images(x, size=(rows, LEN)), row r the LEN frames of sequence r;
 *   gif   [LEN, nh*H, nw*W] palette indices: frame t tiles sequence r at cell (r / nw, r % nw), nh * nw = rows; the index is the grey byte
 *   (C = 1) or 36 r6 + 6 g6 + b6 of the 6x6x6 colour cube, r6 = (5 r + 127) / 255 in integers (C = 3).
 * C is 1 or 3, W a multiple of 4, gen / data 16-byte aligned, sheet / gif 4-byte aligned.  Added without a version change: no existing
 * entry point or struct is touched. */
int ggan_video_sheet_u8(const float* gen, const float* data, uint8_t* sheet, uint8_t* gif, int n, int rows, int LEN, int C, int H, int W,
                        int nh, int nw, int interleave, float a, float b, float d, ggan_stream_t stream);

/* ---- t-SNE: the latent-space pictures of the MNIST scripts (gan_inference_mnist.py:472-480, gmgan_inference_mnist.py:533-551:
 * TSNE().fit_transform on the host).  van der Maaten's algorithm with the schedule of that TSNE(); the repulsive term is summed exactly
 * over all pairs (no Barnes-Hut tree) and there is no early stop.  No float atomics: the same input gives the same bits on every run.
 * Added without a version change: no existing entry point or struct is touched.
 *   ggan_tsne_sqnorms     norms[i] = |x_i|^2, x [N, D].
 *   ggan_tsne_neighbours  rows row0 .. row0+rows-1: dots [rows, N] (scratch) = X_blk X^T through ggan_gemm (ws as there), turned in place
 *                         into d_ij = max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0); idx / dist [N, K]: the K nearest j != i of each row of the
 *                         block, ascending in (distance, index): a tie in distance goes to the lower index.  2 <= K + 1 <= N, K <= 128.
 *   ggan_tsne_affinities  sklearn's _binary_search_perplexity, one row each: at most `steps` bisection steps on beta from 1, until the
 *                         entropy of p_j|i = exp(-beta d_ij) / sum is log(perplexity) within tol.  Each row of dist is ascending (as ggan_tsne_neighbours writes it): the distances are taken relative to
 *                         dist[i][0], which changes neither p nor the entropy and needs no floor on the sum; p_cond [N, K], beta [N]: the value
 *                         p_cond was formed with.  0 < perplexity < N.
 *   ggan_tsne_symmetrise  P = (P + P^T) / 2N as a CSR: ptr [N + 1], col / val [2 N K].  Row i: its K neighbours in their order, then
 *                         every j whose list holds i, ascending; a j in both relations carries its whole value in the first group and
 *                         0 in the second.  ptr[N] = 2 N K.  scratch: 2 N + N K ints.
 *   ggan_tsne_gradient    at the embedding y [N, 2]: attr[i] = sum_j P_ij q_ij (y_i - y_j), rep[i] = sum_j q_ij^2 (y_i - y_j),
 *                         z[0] = sum_{i != j} q_ij, q_ij = 1 / (1 + |y_i - y_j|^2).  The j range is cut into `splits` (1 .. 64)
 *                         parts, one per workgroup; part: 2 N splits floats, zblk: splits * ceil(N / 256) floats, added in a fixed order.
 *   ggan_tsne_kl          kl[0] = sum_ij P_ij log(P_ij Z / q_ij) (klrow: N floats of scratch).
 *   ggan_tsne_iterate     iterations it0 .. it1-1: grad = 4 (e attr - rep / Z); gains + 0.2 where grad and velocity disagree in sign,
 *                         x 0.8 otherwise, floored at min_gain; vel = m vel - learning_rate gain grad; y += vel.  e = early_exaggeration
 *                         and m = momentum0 while it < exploration_iters, then 1 and momentum1.  Positions alternate between ya (read
 *                         first) and yb: the result is in ya after an even number of iterations, in yb after an odd one. */
#define GGAN_TSNE_MAX_K 128
#define GGAN_TSNE_MAX_SPLITS 64
int ggan_tsne_sqnorms(const float* x, int N, int D, float* norms, ggan_stream_t stream);
int ggan_tsne_neighbours(const float* x, const float* norms, int N, int D, int row0, int rows, int K, float* dots, int32_t* idx, float* dist,
                         void* ws, size_t ws_bytes, ggan_stream_t stream);
int ggan_tsne_affinities(const float* dist, int N, int K, float perplexity, int steps, float tol, float* p_cond, float* beta,
                         ggan_stream_t stream);
int ggan_tsne_symmetrise(const int32_t* idx, const float* p_cond, int N, int K, int* ptr, int32_t* col, float* val, int* scratch,
                         ggan_stream_t stream);
int ggan_tsne_gradient(const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits, float* part, float* zblk,
                       float* attr, float* rep, float* z, ggan_stream_t stream);
int ggan_tsne_kl(const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits, float* part, float* zblk,
                 float* klrow, float* kl, ggan_stream_t stream);
int ggan_tsne_iterate(const int* ptr, const int32_t* col, const float* val, float* ya, float* yb, float* vel, float* gains, int N, int splits,
                      float* part, float* zblk, int it0, int it1, int exploration_iters, float early_exaggeration, float momentum0,
                      float momentum1, float learning_rate, float min_gain, ggan_stream_t stream);

/* reconstruction distances of tflib/utils/distance.py:3-17 (`distance(x, y, 'l1'|'l2')` = reduce_mean(|x-y|^p)), used by the
 * alice / local_epce / vegan objectives as rec_penalty: out[0] (+)= weight * mean(|x-y|^p), p = 1 | 2; the backward writes
 * gx and/or gy (either may be NULL). */
int ggan_dist_fwd(const float* x, const float* y, float* out, size_t n, int p, float weight, int accumulate,
                  ggan_stream_t stream);
int ggan_dist_bwd(const float* x, const float* y, const float* gout, float* gx, float* gy, size_t n, int p,
                  float weight, ggan_stream_t stream);
/* slopes[b] = sqrt(sum_j g[b,j]^2); pen[0] = lam*mean_b((slopes-1)^2)  (gan_inference_cifar10.py:363-364).
 * bwd: gg[b,j] = gpen[0]*lam*2*(slopes[b]-1)/B * g[b,j]/slopes[b]. */
int ggan_gp_penalty_fwd(const float* g, float* slopes, float* pen, int B, int D, float lam,
                        ggan_stream_t stream);
int ggan_gp_penalty_bwd(const float* g, const float* slopes, const float* gpen, float* gg, int B, int D,
                        float lam, ggan_stream_t stream);
/* ggan_gp_penalty_fwd together with ggan_gp_penalty_bwd for a unit upstream gradient (gg_unit = d pen / d g) in one launch -- the
 * penalty enters the critic cost with weight 1 (gan_inference_cifar10.py:365), so that IS its upstream gradient.  arrive: one int32,
 * zero before the first call, left zero (the last workgroup forms the penalty: fixed order, deterministic). */
int ggan_gp_penalty_fwd_grad(const float* g, float* slopes, float* pen, float* gg_unit, int32_t* arrive, int B, int D, float lam,
                             ggan_stream_t stream);
/* The critic tail Linear([a1 | a2] -> H) -> LeakyReLU(alpha) -> Linear(H -> 1) differentiated w.r.t. its input, as the penalty pass needs it
 * (tf.gradients(Discriminator(x_hat, z_hat), [x_hat]), gan_inference_cifar10.py:362), between the two large products:
 * gpre[n, j] = (u ? u[n] : 1) * w_out[j] * (h[n, j] > 0 ? 1 : alpha) -- u[M] the upstream gradient of the logits (NULL: ones), h[M, H]
 * the hidden layer (pre- or post-activation: only its sign is read).  The bits of the K = 1 product u w_out^T followed by ggan_act_bwd.
 * Any M, H >= 1; 16-byte accesses when H is a multiple of 4 and the buffers are 16-byte aligned. */
int ggan_head_seed_fwd(int M, int H, const float* u /* may be NULL */, const float* h, const float* w_out, float alpha, float* gpre,
                       ggan_stream_t stream);

/* ---- optimiser --------------------------------------------------------------------------------
 * tf.train.AdamOptimizer step over a flat parameter buffer (tflib/objs/gan_inference.py:108-117;
 * SURVEY.md A.5): t = *step + 1; m,v EMA; lr_t = lr*sqrt(1-b2^t)/(1-b1^t); theta -= lr_t*m/(sqrt(v)+eps).
 * `step` lives in device memory so that a captured graph advances it: the kernel reads it and
 * ggan_adam_advance increments it afterwards.  grad_scale multiplies g first (1/world for DP). */
int ggan_adam_step(float* theta, const float* g, float* m, float* v, size_t n, const int32_t* step,
                   float lr, float beta1, float beta2, float eps, float grad_scale, ggan_stream_t stream);
int ggan_adam_advance(int32_t* step, ggan_stream_t stream);

/* tf.train.RMSPropOptimizer step over a flat buffer (decay 0.9, momentum 0, eps 1e-10 are TF's defaults), followed by the
 * weight clipping of the `wali` objective (tflib/objs/gan_inference.py:4-26: tf.clip_by_value(var, -.01, .01) on the critic);
 * pass clip_lo = -INFINITY, clip_hi = INFINITY for no clipping.  ms is initialised to 1.0 by TF. */
int ggan_rmsprop_step(float* theta, const float* g, float* ms, size_t n, float lr, float decay, float eps,
                      float grad_scale, float clip_lo, float clip_hi, ggan_stream_t stream);
/* Adam step whose counter was already advanced: *step holds THIS update's ordinal t (>= 1), e.g. incremented by the
 * ggan_pack_parts launch of the same optimizer step (its `bump` argument) -- no separate ggan_adam_advance launch. */
int ggan_adam_step_counted(float* theta, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr,
                           float beta1, float beta2, float eps, float grad_scale, ggan_stream_t stream);
/* Exponential moving average of a flat weight buffer, for sampling and evaluation only.  NO call site in the reference (it
 * keeps no average); the semantics are those TensorFlow 1 documents for tf.train.ExponentialMovingAverage(decay, num_updates):
 *     d_t = min(decay, (1 + t) / (10 + t));   shadow -= (1 - d_t) * (shadow - theta)
 * in fp32, in place.  t = step[0] is read on the device and must already hold the ordinal (1, 2, ...) of the update just applied:
 * its state after ggan_adam_step_counted, after ggan_pack_adam, and after the pack launch of an RMSProp step.  theta is only
 * read.  decay in [0, 1); shadow and theta are distinct 16-byte aligned buffers of n floats. */
int ggan_ema_step(float* shadow, const float* theta, size_t n, const int32_t* step, float decay, ggan_stream_t stream);
/* Exchanges the contents of two non-overlapping 16-byte aligned fp32 buffers in one pass (no scratch): how the averaged weights
 * visit the live parameter storage for an evaluation and leave it again, bit for bit. */
int ggan_swap(float* a, float* b, size_t n, ggan_stream_t stream);
/* gather up to GGAN_PACK_MAX scattered tensors into one flat buffer (gradient bucket for RCCL). */
#define GGAN_PACK_MAX 64
int ggan_pack(const float* const* srcs, const size_t* sizes, const size_t* offsets, int count,
              float* flat, ggan_stream_t stream);
/* same, where source i is the sum of parts[i] slabs strides[i] floats apart (summed in slab order: deterministic);
 * bump (may be NULL): an int32 incremented once by this launch. */
int ggan_pack_parts(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts,
                    const size_t* strides, int count, float* flat, int32_t* bump, ggan_stream_t stream);
/* ggan_pack_parts with an optional SECOND contribution per tensor (srcs2[i] may be NULL; parts2 / strides2 as parts / strides):
 * flat[off_i ..] = sum of the slabs of srcs[i] (zeros if NULL) + sum of the slabs of srcs2[i].  A parameter that two passes of one
 * step reach (the critic's main pass and its gradient-penalty pass, gan_inference_cifar10.py:351-366) gets its two gradient
 * contributions summed here instead of by an addition launch per parameter. */
int ggan_pack_parts2(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts, const size_t* strides,
                     const float* const* srcs2, const int* parts2, const size_t* strides2, int count, float* flat, int32_t* bump,
                     ggan_stream_t stream);
/* ggan_pack_parts2 followed by ggan_adam_step_counted in ONE launch (single-replica optimizer steps: nothing happens to the packed
 * gradient between the two; tf.train.AdamOptimizer.minimize = compute_gradients + apply_gradients, gan_inference_cifar10.py:376-380).
 * The summed gradient is still written to `flat`; theta / m / v are the optimizer's flat buffers with the same offsets.  Every
 * workgroup uses step[0] + 1 as the update's ordinal and the last one to finish advances step[0]; `arrive` is
 * GGAN_PACK_ARRIVE_INTS int32 of device memory (arrival counters) that are zero before the call and are left zero.  Same
 * arithmetic, in the same order, as the two launches.  arrive == NULL: the launch applies PART of an update (a subset of the
 * tensors) and leaves step[0] alone -- the launch that completes the update, ordered behind it, passes the counters.
 * flat, theta, m and v must be 16-byte aligned (refused otherwise, as ggan_adam_step refuses them): the kernel picks its 16-byte
 * accesses from flat + offset and the sources and applies them to theta, m and v at the same offset.  The project's own caller
 * (optim.py: AdamOptimizer's g, theta, m, v) always passes whole, fresh torch allocations, which are aligned. */
#define GGAN_PACK_ARRIVE_STRIDE 1024
#define GGAN_PACK_ARRIVE_INTS (33 * GGAN_PACK_ARRIVE_STRIDE)
int ggan_pack_adam(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts, const size_t* strides,
                   const float* const* srcs2 /* may be NULL */, const int* parts2, const size_t* strides2, int count, float* flat,
                   float* theta, float* m, float* v, int32_t* step, int32_t* arrive, float lr, float beta1, float beta2, float eps,
                   float grad_scale, ggan_stream_t stream);

/* ---- per-kernel timing (bench.py roofline leg) -----------------------------------------------
 * When enabled every launch is bracketed by hipEvents on its own stream.  ggan_prof_report
 * synchronises, then writes up to `cap` records -- one per (kernel, work-items per launch, algorithmic flop per launch): a kernel launched
 * on two problem shapes is two records even where the two launches have the same grid, so that per-launch figures are never averages
 * over different problems -- and returns their number.  `flops` / `launches` is the record's flop per launch (its key). */
typedef struct { char name[48]; double total_ms; long launches; double flops; double bytes; long grid; } ggan_prof_rec;   /* one record per (kernel, grid = work-items per launch = rocprofv3's Grid_Size, flop per launch) */
int ggan_prof_enable(int on);
int ggan_prof_reset(void);
int ggan_prof_report(ggan_prof_rec* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* GGAN_H */
