/*
 * slk.h — C-ABI of the MI355X-native split-CNN step (libslk.so, gfx950).
 *
 * The reference (eliasandronicou/split-learning-k8s) has no native code and no FFI: every op of its
 * hot path is a torch CPU call made by src/model_def.py, src/client_part.py and src/server_part.py.
 * Each entry point below replaces one (or a fused group) of those calls; the reference call site is
 * cited next to each declaration. The Python host layer (split-learning-k8s_amd/splitcnn/_lib.py)
 * binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions (all entry points):
 *   - Plain pointers to DEVICE memory, sizes as int, the HIP stream as `void*` (hipStream_t).
 *   - Every buffer, including workspaces, is allocated by the caller. The library never allocates,
 *     frees or synchronises, so every call is safe inside HIP-graph capture.
 *   - Return value: 0 on success, otherwise a hipError_t code (1 = hipErrorInvalidValue for bad
 *     arguments). slk_error_string() turns it into text. Nothing throws across the ABI.
 *   - Stateless and reentrant; ordering comes only from the caller's stream.
 *   - Layouts are the reference's logical NCHW layouts (torch contiguous):
 *       x      f32 [B,1,28,28]      client input           (client_part.py:110,114)
 *       act    f32 [B,32,26,26]     cut-layer activations  (client_part.py:114,118)
 *       pooled f32 [B,64,12,12]     = flatten [B,9216], index c*144+h*12+w (model_def.py:20-21,26-27)
 *       code   u8  [B,64,12,12]     max-pool argmax in its 2x2 window, row-major 0..3, first max wins;
 *                                   4 = pooled value <= 0 (ReLU blocks the gradient)
 *       logits f32 [B,10]; labels i64 [B]
 *       W1 f32[32,1,3,3] b1[32]  W2 f32[64,32,3,3] b2[64]  W3 f32[10,9216] b3[10]  (model_def.py:8,18,22)
 *   - Flat parameter blocks (what the fused SGD updates in one launch):
 *       client: [W1 (288) | b1 (32)]                     = SLK_CLIENT_NPARAM floats
 *       server: [W2 (18432) | b2 (64) | W3 (92160) | b3 (10)] = SLK_SERVER_NPARAM floats
 *   - Tensors, parameters, accumulators and every non-conv2 kernel are fp32 (the reference's dtype).
 *     conv2's products come in two forms: the f32 MFMA (Winograd slk_conv2_*, direct slk_conv2_*_direct)
 *     and "x3" (slk_conv2_*_x3*, the default fused step's): each f32 operand is scaled by an exact power
 *     of two and split into f16 hi + lo, and a product is hi*hi + hi*lo + lo*hi on the f16 MFMA with
 *     f32 accumulation (per-product error <= ~7e-7 relative; tested against fp64 at the f32 path's bars).
 *     Weight-gradient reductions use per-workgroup slabs summed in a fixed order, so every result is
 *     run-to-run bit-stable.
 */
#ifndef SLK_H
#define SLK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLK_ABI_VERSION 1

#define SLK_CLIENT_NPARAM 320
#define SLK_SERVER_NPARAM 110666
#define SLK_OFF_W2 0
#define SLK_OFF_B2 18432
#define SLK_OFF_W3 18496
#define SLK_OFF_B3 110656

int slk_abi_version(void);
const char* slk_error_string(int err);
/* Hex sha256 of the sources this library was compiled from (the csrc .hip and .h files, include/slk.h);
 * splitcnn/_lib.py refuses a library whose id differs from the tree's. */
const char* slk_build_id(void);

/* ---------------------------------------------------------------- NaN and +-inf
 * What every entry of the convolution path (client stage, server stage, the x3 and K5 forms) does with a non-finite
 * operand. It DEVIATES from torch in clause 2: torch's relu and max_pool2d return NaN for a NaN, these kernels +0.
 * tests/nonfinite_ref.py states the rule in float64, tests/test_nonfinite_k2_gpu.py holds every K2 entry to it.
 *
 * 1. Arithmetic is IEEE. A non-finite operand of a product propagates into every accumulator the product is summed
 *    into (0 x NaN = NaN, 0 x inf = NaN), except under clause 4.
 * 2. ReLU and max-pool are selects. ReLU is v > 0 ? v : +0. The pooled value is the maximum of the window's values that
 *    compare greater than 0, else +0 with code 4 (CODE_NONE). A NaN or -inf pre-activation gives +0; a +inf is kept
 *    and its code is its index. A code byte is always 0, 1, 2, 3 or 4. NOT torch: a NaN weight, bias or input pixel
 *    is erased here and the logged loss stays finite where the reference logs NaN (README, "NaN and +-inf").
 *    The x3 forwards scan a window from its FIRST raw accumulator with a strict > (csrc/slk_x3.hip pool_piece): a NaN
 *    in that position gives +0 / code 4 for the window, a NaN in another position is skipped.
 * 3. Scaling maxima ignore NaN (fmaxf): slk_row_amax, the fused maxima of slk_fc_dgrad_amax / slk_fc_backward /
 *    slk_fc_xent_amax, conv1_cut_bound of slk_conv1_fwd_amax / slk_conv1_fwd_x3, the x3sa forward's own maximum. An
 *    infinite maximum gives scale exponent 0 (csrc/slk_x3.hip x3_exp). An x3 kernel then splits a +-inf operand into
 *    (+-inf, inf - inf = NaN), so every output it reaches is NaN before clause 2 applies, and the weight gradients'
 *    launch-wide scale moves for every sample; the f32 forms (Winograd, direct) keep +-inf, except that Winograd's
 *    transforms (B^T d B, G g G^T, A^T m A: csrc/slk_wino.hip) meet inf - inf and may turn it into NaN inside the
 *    2 x 2 tiles (all nine taps of a weight gradient) the infinity reaches.
 * 4. Products that are never formed. A pooled gradient exists only where a code routes it. The 2:4-sparse weight
 *    gradients (slk_conv2_wgrad_x3s, the K5 weight gradients) skip exact zeros of dY: a non-finite activation that
 *    meets only exact zeros of dY may or may not make its column non-finite. Staged zero padding IS multiplied: a
 *    poisoned weight of a dgrad or of a padded (K5) forward may reach every pixel of its channel's planes, and a
 *    poisoned gradient at a border pixel every tap of its channel in the K5 weight gradients.
 * 5. Masks are selects. A gradient at a position whose ReLU bit or routing code excludes it is +0 whatever came in
 *    (the Winograd dgrad expands a window with a bit-mask AND, so its cut gradient is non-finite exactly where the
 *    direct kernel's is; the Winograd wgrad drops a blocked window's value before its table multiply).
 * 6. Samples are independent in every entry whose output has a batch dimension: another sample's NaN or inf changes
 *    no bit of a clean sample's output. Slabs the poisoned sample does not feed are unchanged.
 * 7. Heads, optimizers, EMA, both codecs and the loaders keep the contracts stated at their declarations. The K5
 *    head's dropout is a select ((keep bit) ? d * keep_scale : 0, csrc/slk_wide_head.hip): a DROPPED NaN or inf feature
 *    is 0 (torch's Dropout multiplies by the mask and keeps a NaN), a kept one is an ordinary operand of clause 1.
 *    The cut noise (slk_cut_noise, "Cut noise" below) has no special case: a NaN element makes its sample's s2, coef
 *    and every clipped element NaN, an infinite s2 gives coef = 0 (then 0 x inf = NaN at an infinite element), and
 *    without a clip a non-finite element stays its own; no other sample is touched. The MX cut records ("MX cut
 *    records" below) poison by BLOCK, not by sample: a non-finite element makes its 32-element block's scale byte 0xFF
 *    and the block 32 NaNs on the other side, the sample's other 511 blocks are unchanged (the FP8 records poison the
 *    whole sample); the head then poisons that sample's logits as for any NaN feature it keeps.
 * The supported check is Python's GraphedTrainer.check_finite() (parameters, optimizer state, averaged blocks). */

/* ---------------------------------------------------------------- client stage (ModelPartA) */

/* act = conv2d(x, W1, b1) > 0 ? conv2d(x, W1, b1) : +0, stride 1, no padding: torch's relu except for a NaN
 * pre-activation, which gives +0 (clause 2 above).
 * Replaces ModelPartA.forward (src/model_def.py:11-12) as called at src/client_part.py:114 on finite operands. */
int slk_conv1_fwd(const float* x, const float* W1, const float* b1, float* act, int B, void* stream);

/* slk_conv1_fwd that also writes act_amax[b], the per-sample scale value of the x3 conv2 kernels: since
 * round 5 the bound max_c (sum_k |W1[c][k]| * max|x[b]| + max(b1[c], 0)) >= max(act[b]) (one float expression,
 * slk_common.h conv1_cut_bound; the same value slk_conv1_fwd_x3 emits), so the 354 MB cut is never re-read
 * and no writer needs a pass over its outputs before splitting them. */
int slk_conv1_fwd_amax(const float* x, const float* W1, const float* b1, float* act, float* act_amax, int B,
                       void* stream);

/* Client backward: relu-bwd mask (act > 0) applied to the cut gradient, then conv1 weight/bias
 * gradient. No input gradient (the data needs none). Writes per-group partial slabs
 * [slk_conv1_wgrad_nslab(B)][320] into `slabs`; reduce them with slk_sgd_from_slabs or
 * slk_reduce_slabs. Replaces `activations.backward(server_grads)` (src/client_part.py:132). */
int slk_conv1_wgrad(const float* x, const float* act, const float* cut_grad, float* slabs, int B,
                    void* stream);
int slk_conv1_wgrad_nslab(int B);
/* Same result as slk_conv1_wgrad, with the ReLU mask recomputed from x, W1, b1 in slk_conv1_fwd's
 * exact FMA order (act > 0 <=> conv1(x) > 0, bit-identically) instead of read from `act`: 89.6 KB of
 * HBM traffic per sample instead of 176 KB. W1/b1 must be the forward's weights (they are inside a
 * split step: the client's SGD follows its backward, client_part.py:132-133). */
int slk_conv1_wgrad_remask(const float* x, const float* W1, const float* b1, const float* cut_grad, float* slabs,
                           int B, void* stream);

/* ---------------------------------------------------------------- server stage (ModelPartB) */

/* pooled = maxpool2(relu(conv2d(act, W2, b2))) and its argmax code, fused (Winograd F(2x2,3x3) on
 * the f32 MFMA: one transformed 2x2 output tile = one pool window). Replaces ModelPartB.forward lines
 * src/model_def.py:25-27 as called at src/server_part.py:48 on finite operands; relu and maxpool2 are clause 2's
 * selects ("NaN and +-inf" above: a NaN pre-activation is dropped, not propagated as torch does). */
int slk_conv2_fwd_pool(const float* act, const float* W2, const float* b2, float* pooled,
                       uint8_t* code, int B, void* stream);
/* The same op as a direct implicit GEMM (f32 MFMA, k-ordered fma chains); kept as the A/B and
 * cross-check path. */
int slk_conv2_fwd_pool_direct(const float* act, const float* W2, const float* b2, float* pooled,
                              uint8_t* code, int B, void* stream);

/* logits = pooled @ W3^T + b3.  Replaces model_def.py:28 (fc1). */
int slk_fc_fwd(const float* pooled, const float* W3, const float* b3, float* logits, int B,
               void* stream);

/* Cross-entropy (mean reduction, hard labels, no label smoothing: slk_xent_soft_fwd_bwd has both) forward+backward
 * from logits:
 * loss_i[b] = logsumexp(z_b) - z_b[y_b];  dlogits = (softmax(z) - onehot(y)) * grad_scale.
 * grad_scale = 1/B reproduces nn.CrossEntropyLoss()'s mean (src/server_part.py:16,49,51).
 * An out-of-range label writes NaN loss/dlogits for that row and sets *err_flag (may be NULL). */
int slk_xent_fwd_bwd(const float* logits, const int64_t* labels, float* loss_i, float* dlogits,
                     float grad_scale, int* err_flag, int B, void* stream);

/* slk_fc_fwd + slk_xent_fwd_bwd in one launch (the cross-entropy of a workgroup's 16 samples from the logits it
 * just reduced, in LDS): the same logits, loss_i and dlogits bit for bit. src/server_part.py:48-49 + the CE part
 * of :51. */
int slk_fc_logits_xent(const float* pooled, const float* W3, const float* b3, const int64_t* labels, float* logits,
                       float* loss_i, float* dlogits, float grad_scale, int* err_flag, int B, void* stream);

/* dpooled = dlogits @ W3 (fc1 input gradient). Replaces the fc1 part of loss.backward()
 * (src/server_part.py:51). */
int slk_fc_dgrad(const float* dlogits, const float* W3, float* dpooled, int B, void* stream);
/* slk_fc_dgrad that also writes dp_amax[b] = max |dpooled[b]|: the split head of the x3 step (logits,
 * cross-entropy, fc1 weight gradient while pooled is still in the Infinity Cache, then this). */
int slk_fc_dgrad_amax(const float* dlogits, const float* W3, float* dpooled, float* dp_amax, int B, void* stream);

/* Fused server head: fc1 forward, cross-entropy forward+backward and fc1 input gradient in one
 * launch (pooled is read from HBM once for the logits and once, L2-hot, for nothing else).
 * Outputs logits, loss_i, dlogits, dpooled. Replaces server_part.py:48(fc1 part),49,51(fc1 part). */
int slk_fc_xent(const float* pooled, const float* W3, const float* b3, const int64_t* labels,
                float* logits, float* loss_i, float* dlogits, float* dpooled, float grad_scale,
                int* err_flag, int B, void* stream);

/* slk_fc_xent that also writes dp_amax[b] = max |dpooled[b]| (the x3 conv2 backward kernels' scales). */
int slk_fc_xent_amax(const float* pooled, const float* W3, const float* b3, const int64_t* labels, float* logits,
                     float* loss_i, float* dlogits, float* dpooled, float* dp_amax, float grad_scale, int* err_flag,
                     int B, void* stream);

/* ---- soft targets: label smoothing and mixed labels (the soft forms of the four cross-entropy entries)
 * A target stays one int64 per sample. A MIXED LABEL packs two classes and a weight:
 *   y = a | (b << 8) | ((int64)float_bits(wb) << 32)       a, b in [0, 10); bits 16-31 zero; wb an f32 in [0, 1]
 * wb is the weight of class b, 1 - wb that of class a. A plain label a < 10 is the case b = 0, wb = 0, so every
 * hard-label tensor is a valid mixed label; one with wb != 0 is >= 2^32, which the hard-label entries above flag as
 * out of range. With smoothing eps in [0, 1] (by value: a captured graph keeps it) and C = 10 the row's target is
 *   t_j = (1 - eps) * ((j == a ? 1 - wb : 0) + (j == b ? wb : 0)) + eps / C
 *   loss_i = logsumexp(z) - sum_j t_j z_j;   dlogits_j = (softmax(z)_j - t_j) * grad_scale
 * i.e. torch.nn.functional.cross_entropy(z, probs, label_smoothing=eps) for the two-class probability target, and
 * nn.CrossEntropyLoss(label_smoothing=eps) on class indices when wb = 0. In float32, operation by operation (fl = one
 * rounding; lse = m + logf(se) and expf(z_j - lse) exactly as in the hard-label entries):
 *   wa = fl(1 - wb);  keep = fl(1 - eps);  flat = fl(eps / 10)                      (IEEE subtraction / division)
 *   u_j = (j == a ? wa : 0) + (j == b ? wb : 0)                                    (selects, then one addition)
 *   t_j = fmaf(keep, u_j, flat)
 *   S = 0;  for j = 0..9 ascending:  if (t_j != 0) S = fmaf(t_j, z_j, S)            (t_j == 0 contributes nothing,
 *                                                                                    also at z_j = -inf)
 *   loss_i = fl(lse - S);   dlogits_j = fl(fl(expf(z_j - lse) - t_j) * grad_scale)
 * With eps = 0 and plain labels t is exactly one-hot and S = z_a, so every soft entry writes bit for bit what its
 * hard-label twin writes (on -inf logits off the label too). A target is malformed when a >= 10, b >= 10, a bit of
 * 16-31 is set, y < 0, or wb is NaN or outside [0, 1]: it sets *err_flag (may be NULL) and that row's loss_i and
 * dlogits are NaN, other rows unaffected — as an out-of-range label in the hard entries. smoothing outside [0, 1]
 * or NaN returns the invalid-argument status without a launch. Evaluation (slk_fc_eval, slk_eval_logits) stays the
 * plain cross-entropy on plain labels, as a model.eval() loop reports it. */

/* slk_xent_fwd_bwd with soft targets. */
int slk_xent_soft_fwd_bwd(const float* logits, const int64_t* labels, float* loss_i, float* dlogits, float grad_scale,
                          float smoothing, int* err_flag, int B, void* stream);
/* slk_fc_logits_xent with soft targets: the same logits (bitwise), then the soft loss_i and dlogits. The default K2
 * step's head when the trainer is built with loss=SoftCrossEntropy(...). */
int slk_fc_logits_xent_soft(const float* pooled, const float* W3, const float* b3, const int64_t* labels,
                            float* logits, float* loss_i, float* dlogits, float grad_scale, float smoothing,
                            int* err_flag, int B, void* stream);
/* slk_fc_xent / slk_fc_xent_amax with soft targets in one entry: dp_amax may be NULL (then it is not written). */
int slk_fc_xent_soft(const float* pooled, const float* W3, const float* b3, const int64_t* labels, float* logits,
                     float* loss_i, float* dlogits, float* dpooled, float* dp_amax, float grad_scale, float smoothing,
                     int* err_flag, int B, void* stream);

/* fc1 weight/bias gradient partials: slabs [slk_fc_wgrad_nslab(B)][92170] laid out as
 * [dW3 (10*9216) | db3 (10)], i.e. the tail of the server flat block. */
int slk_fc_wgrad(const float* dlogits, const float* pooled, float* slabs, int B, void* stream);
int slk_fc_wgrad_nslab(int B);

/* slk_fc_dgrad_amax + slk_fc_wgrad in ONE launch whose blocks take one of the two jobs from their index (each
 * kind keeps its own partition, so neither waits for the other): the default K2 step's fc1 backward. Every output bit for bit what the two entries write for the same inputs:
 *   dpooled[b][k] = the ten-term fmaf chain from 0 over the classes in ascending order, fmaf(dlogits[b][j], W3[j][k], .)
 *   dp_amax[b]    = max_k |dpooled[b][k]|                       (a maximum: no order)
 *   slabs[s]      = [dW3 | db3] of slice s of the batch, slk_fc_wgrad_nslab(B) slices in slk_fc_wgrad's order: each
 *                   dW3[j][k] the fmaf chain from 0 over the slice's samples in ascending order, db3[j] their plain
 *                   sum in the same order. */
int slk_fc_backward(const float* dlogits, const float* W3, const float* pooled, float* dpooled, float* dp_amax,
                    float* slabs, int B, void* stream);

/* Cut-layer gradient: cut_grad = conv2 input gradient of maxpool/relu-masked dpooled
 * (uses `code` from slk_conv2_fwd_pool). This is `client_activations.grad` of
 * src/server_part.py:45,51,57. Winograd F(2x2,3x3) on the f32 MFMA; the routed conv2 output
 * gradient is expanded per transform tile in registers (never materialised). */
int slk_conv2_dgrad(const float* dpooled, const uint8_t* code, const float* W2, float* cut_grad,
                    int B, void* stream);
/* The same op as a direct implicit GEMM (A/B and cross-check path). */
int slk_conv2_dgrad_direct(const float* dpooled, const uint8_t* code, const float* W2, float* cut_grad,
                           int B, void* stream);

/* conv2 weight/bias gradient partials: slabs [slk_conv2_wgrad_nslab(B)][18496] laid out as
 * [dW2 (64*288) | db2 (64)], i.e. the head of the server flat block; their fixed-order sum is the
 * gradient. Winograd F(2x2,3x3) filter gradient on the f32 MFMA (G^T dU G applied per slab). */
int slk_conv2_wgrad(const float* act, const float* dpooled, const uint8_t* code, float* slabs,
                    int B, void* stream);
int slk_conv2_wgrad_nslab(int B);
/* The same op as a direct implicit GEMM (A/B and cross-check path), with its own slab count. */
int slk_conv2_wgrad_direct(const float* act, const float* dpooled, const uint8_t* code, float* slabs,
                           int B, void* stream);
int slk_conv2_wgrad_direct_nslab(int B);

/* ---------------------------------------------------------------- conv2 on the f16 MFMA, fp32-grade ("x3")
 * The same ops as slk_conv2_fwd_pool / _dgrad / _wgrad, computed as direct implicit GEMMs whose f32
 * operands are split after an exact power-of-two scale into f16 hi + lo, each product formed by three
 * v_mfma_f32_16x16x32_f16 (hi*hi + hi*lo + lo*hi) into an f32 accumulator: per-product relative error
 * <= ~7e-7 (csrc/slk_x3.hip). Operand scales: weights per launch (from max|W2|), data per sample from a
 * caller-supplied per-sample max |.| (slk_row_amax, or a producer that emits it); the arrays must bound
 * their rows (a too-small bound overflows f16 to inf). Replace the same reference lines as the f32 ops.
 * Non-finite operands (clause 3 above): NaN never enters a scale; a +-inf operand of any x3 entry becomes NaN in every
 * output it reaches (forwards: then +0 / code 4 by clause 2), where the f32 forms would pass +inf on. */

/* amax[r] = max_i |x[r*n + i]| for r < rows (NaNs ignored). */
int slk_row_amax(const float* x, int rows, int n, float* amax, void* stream);
/* slk_conv2_fwd_pool on the x3 path; act_amax[B] = per-sample max |act| (model_def.py:25-27). */
int slk_conv2_fwd_pool_x3(const float* act, const float* act_amax, const float* W2, const float* b2, float* pooled,
                          uint8_t* code, int B, void* stream);
/* slk_conv2_dgrad on the x3 path; dp_amax[B] = per-sample max |dpooled| (server_part.py:45,51,57). */
int slk_conv2_dgrad_x3(const float* dpooled, const float* dp_amax, const uint8_t* code, const float* W2,
                       float* cut_grad, int B, void* stream);
/* slk_conv2_wgrad on the x3 path: slabs [slk_conv2_wgrad_x3_nslab(B)][18496] = [dW2 | db2] partials
 * (fixed-order sum = the gradient). The reduction spans samples (server_part.py:51), so every product
 * carries one scale: the input keeps its sample's scale (from act_amax) and that sample's dY is scaled
 * to compensate (launch maxima of act_amax / dp_amax); db2 is summed in f32. */
int slk_conv2_wgrad_x3(const float* act, const float* act_amax, const float* dpooled, const float* dp_amax,
                       const uint8_t* code, float* slabs, int B, void* stream);
int slk_conv2_wgrad_x3_nslab(int B);
/* The forward that also writes its split f16 input images (act16, slk_conv2_act16_bytes(B) bytes; each
 * sample at its own scale from act_amax) and the wgrad that moves them by LDS-DMA instead of loading and
 * splitting act: the wgrad's input staging becomes a copy. Same results as slk_conv2_wgrad_x3 (bitwise:
 * the same scales, the same f16 values).
 * slk_conv2_wgrad_x3s refuses (invalid value) a batch whose K share would span more samples than its LDS scale
 * table holds: B >= 2,883,243, whose act16 images and pooled gradient alone exceed the device's memory. */
int slk_conv2_fwd_pool_x3s(const float* act, const float* act_amax, const float* W2, const float* b2, float* pooled,
                           uint8_t* code, uint16_t* act16, int B, void* stream);
int slk_conv2_wgrad_x3s(const uint16_t* act16, const float* act_amax, const float* dpooled, const float* dp_amax,
                        const uint8_t* code, float* slabs, int B, void* stream);
/* Which kernel slk_conv2_wgrad_x3s runs: always 2 = on the 2:4-sparse f16 MFMA (v_smfmac_f32_16x16x64_f16:
 * the max-pool routing leaves at most 2 nonzeros of dY in every 4 consecutive output pixels of a row starting at
 * a multiple of 4, so half the dense x3 products are never issued; clause 4 above: a non-finite activation that meets
 * only skipped zeros of dY does not reach its column). 1 (the dense x3 kernel) and 0 (the round-4
 * kernel) named forms that are no longer built. Measurement only (bench.py prices the executed products against
 * the matching peak). */
int slk_conv2_wgrad_x3_form(void);
/* slk_conv2_fwd_pool_x3s with the per-sample max |act| computed inside the forward (written to act_amax,
 * the values slk_row_amax gives) instead of read: the drop-in module path has no separate pass over the cut.
 * act 16-byte aligned. Replaces the row_amax + forward pair behind ModelPartB.forward (src/model_def.py:25-26). */
/* Measurement only: the device's sustained dense f16 MFMA rate (v_mfma_f32_16x16x32_f16, 6 independent chains
 * per wave, 2 waves per SIMD, varied operands). out: slk_mfma_probe_blocks() * 256 floats; FLOPs per launch =
 * slk_mfma_probe_blocks() * 4 * iters * 6 * 16384. bench.py prices the kernels against it beside the nominal peak. */
int slk_mfma_probe_blocks(void);
int slk_mfma_probe(float* out, int iters, void* stream);
int slk_conv2_fwd_pool_x3sa(const float* act, float* act_amax, const float* W2, const float* b2, float* pooled,
                            uint8_t* code, uint16_t* act16, int B, void* stream);
/* act16 layout: per sample an h plane then an l plane, each [26 x 26 pixels][32 ci] f16 with 64-B pixels
 * (8-channel chunk c8 at slot c8 ^ (x & 2)): B x 86,528 bytes. */
int64_t slk_conv2_act16_bytes(int B);

/* The client's conv1 + ReLU (replaces slk_conv1_fwd_amax inside a fused step, src/client_part.py:114)
 * writing the x3 server operand directly: act_amax (the bound of slk_conv1_fwd_amax) and the act16 images
 * (bit-identical to those slk_conv2_fwd_pool_x3s writes from the f32 act with that act_amax), plus the f32
 * act when act != NULL — one pass per (pixel, 8-channel) item. The server forward then reads the
 * images (slk_conv2_fwd_pool_x3i: same pooled / code as slk_conv2_fwd_pool_x3 on the f32 act, bitwise)
 * and so does the wgrad (slk_conv2_wgrad_x3s). relu_bits (optional, slk_relu_bits_bytes(B) bytes, 16-byte
 * aligned): the ReLU mask act > 0 of every cut element, 1 bit each (per sample [4 channel groups cg][169]
 * u32, bit 4 (c & 7) + u of word (c >> 3, t) = act[c][4 t + u] > 0), which slk_conv2_dgrad_x3_c1w consumes. */
int slk_conv1_fwd_x3(const float* x, const float* W1, const float* b1, float* act, float* act_amax, uint16_t* act16,
                     uint32_t* relu_bits, int B, void* stream);
int64_t slk_relu_bits_bytes(int B);
int slk_conv2_fwd_pool_x3i(const uint16_t* act16, const float* act_amax, const float* W2, const float* b2,
                           float* pooled, uint8_t* code, int B, void* stream);

/* slk_conv2_fwd_pool_x3i without the routing codes (pooled only, bitwise the same pooled): the forward of an
 * evaluation pass, which has no backward to route (model_def.py:25-27 under model.eval()). */
int slk_conv2_fwd_pool_x3p(const uint16_t* act16, const float* act_amax, const float* W2, const float* b2,
                           float* pooled, int B, void* stream);

/* The x3 dgrad with the client's backward fused (src/server_part.py:51 -> src/client_part.py:132 in one
 * launch, for the single-GPU step): the cut gradient is not written; each workgroup applies the client's
 * ReLU mask (relu_bits from slk_conv1_fwd_x3) and writes one slab [dW1 c*9+tap (288) | db1 c (32)] of the
 * client gradient (slk_conv2_dgrad_x3_c1w_nslab(B) slabs, reduced by slk_sgd_from_slabs). */
int slk_conv2_dgrad_x3_c1w(const float* dpooled, const float* dp_amax, const uint8_t* code, const float* W2,
                           const float* x, const uint32_t* relu_bits, float* client_slabs, int B, void* stream);
int slk_conv2_dgrad_x3_c1w_nslab(int B);

/* ---------------------------------------------------------------- evaluation / prediction
 * The reference builds a test split (src/client_part.py:52,73) and never evaluates on it; these entries are the
 * forward-only pass a user's `model.eval(); out = model(x); criterion(out, y); out.argmax(1)` loop needs, with the
 * metrics summed on the device (no host sync per batch). pred is i64 [B]: argmax of the sample's logits, the first
 * maximum on exact ties, a NaN logit counting as the maximum (numpy.argmax). */

/* The fc head in evaluation mode: slk_fc_logits_xent's logits stage (bitwise its logits), then loss_i =
 * logsumexp(z) - z[y] (bitwise its loss_i) and pred; no dlogits. logits may be NULL (not stored). labels may be
 * NULL (predict only): loss_i is then not written and err_flag not touched. A label outside [0, 10) sets *err_flag
 * (may be NULL) and gives loss_i = NaN. Replaces model_def.py:28 + the criterion of server_part.py:49 in eval. */
int slk_fc_eval(const float* pooled, const float* W3, const float* b3, const int64_t* labels, float* logits,
                float* loss_i, int64_t* pred, int* err_flag, int B, void* stream);

/* The same loss_i / pred stage (bit for bit) for logits f32 [B,10] already in memory: slk_wide_head_fwd's, the
 * drop-in modules', the U-shaped head's. labels / loss_i / err_flag as in slk_fc_eval. */
int slk_eval_logits(const float* logits, const int64_t* labels, int B, float* loss_i, int64_t* pred, int* err_flag,
                    void* stream);

/* Adds one batch to the metric accumulator `acc`: 104 x 8 bytes of device memory (8-byte aligned), zeroed by the
 * caller before the first batch, updated by one workgroup per launch with plain read-modify-writes (launches on
 * one stream are ordered; do not update one accumulator from two streams at once):
 *   acc[0]                   i64  n           samples seen
 *   acc[1]                   i64  correct     pred == label
 *   acc[2]                   i64  bad_labels  labels outside [0, 10)
 *   acc[3]                   f64  loss_sum    sum of loss_i (float64, fixed order: a function of the inputs and B)
 *   acc[4 + 10 label + pred] i64  confusion counts
 * A sample with an out-of-range label counts in n and bad_labels only. Replaces the host-side
 * `correct += (pred == y).sum().item(); loss += ...item()` of an evaluation loop. */
int slk_eval_accumulate(const float* loss_i, const int64_t* pred, const int64_t* labels, int B, int64_t* acc,
                        void* stream);
#define SLK_EVAL_ACC_WORDS 104

/* ---------------------------------------------------------------- reductions / optimizer */

/* out[i] = (accumulate ? out[i] : 0) + sum_{s=0}^{nslab-1} slabs[s*n + i]  (fixed slab order).
 * accumulate = 1 sums micro-batches into one gradient (pipeline topologies).
 * Summation order (this and SGD from slabs): nslab <= 16 -> slabs in ascending order per column;
 * 16 < nslab <= 64 -> 4 partial sums over slabs w, w+4, w+8, ... (w = 0..3) added in w order; nslab > 64 ->
 * 16 partial sums over slabs w, w+16, ... added in w order (Adam from slabs: the same three forms). Each is
 * a fixed function of (slabs, nslab): bit-stable run to run, but results from different forms are not
 * bitwise comparable. Where the prior out[i] of accumulate = 1 enters, in float32: the ascending form adds
 * it last, out = out + (((s0 + s1) + s2) + ...); the 4- and 16-partial forms start their chain of partials
 * at it, out = (((out + p0) + p1) + p2) + ... (tests/test_reduce_order_gpu.py pins all of this bit for bit). */
int slk_reduce_slabs(const float* slabs, int nslab, int n, float* out, int accumulate, void* stream);

/* Fused deterministic slab reduction + SGD (lr, no momentum, no weight decay):
 * g = sum_s slabs[s*n+i]; grad[i] = g (if grad != NULL); param[i] -= lr * g.
 * Replaces optimizer.step() of optim.SGD(lr=0.01) (client_part.py:17,133; server_part.py:15,52). */
int slk_sgd_from_slabs(float* param, float* grad, const float* slabs, int nslab, int n, float lr,
                       void* stream);

/* param[i] -= lr * grad[i]  (flat multi-tensor SGD; torch.optim.SGD semantics, momentum 0). */
int slk_sgd(float* param, const float* grad, int n, float lr, void* stream);

/* out[0] = scale * sum(values[0..n))  (fixed-order reduction). With values = per-sample losses and
 * scale = 1/B this is nn.CrossEntropyLoss()'s mean (src/server_part.py:49). */
int slk_loss_sum(const float* values, int n, float scale, float* out, void* stream);

/* Loss log ring: ring[*counter % capacity] = scale * sum(values[0..n)); ++*counter (one device
 * thread). This is the device-side replacement of mlflow.log_metric("loss", loss.item(), step)
 * (src/server_part.py:55): the slot comes from device memory, so a captured HIP graph logs every
 * replay into a new slot, and the host flushes the ring every N steps instead of syncing per step. */
int slk_loss_log(const float* values, int n, float scale, float* ring, int capacity, int* counter,
                 void* stream);

/* Every optimizer step of one split step in ONE launch: for each segment s < nseg (<= 4),
 * slk_sgd_from_slabs(params[s], grads ? grads[s] : NULL, slabs[s], nslab[s], n[s], lr), and, when
 * loss_values != NULL, slk_loss_log(loss_values, loss_n, loss_scale, ring, capacity, counter) —
 * bit-identical to those separate launches. Replaces the server's optimizer.step() + log_metric
 * (src/server_part.py:52,55) and the client's optimizer.step() (src/client_part.py:133) at the end
 * of a fused split step. The pointer/size arrays are host memory. A segment with params[s] == NULL
 * (and grads[s] != NULL) only reduces: grads[s] = sum of its slabs (the data-parallel replica fills
 * its all-reduce bucket this way: several slk_reduce_slabs in one launch). */
int slk_sgd_multi_from_slabs(float* const* params, float* const* grads, const float* const* slabs,
                             const int* nslab, const int* n, int nseg, float lr, const float* loss_values,
                             int loss_n, float loss_scale, float* ring, int capacity, int* counter,
                             void* stream);

/* torch.optim.SGD(lr, momentum, dampening, nesterov, weight_decay) fused with the slab reduction, the rate
 * read on the device: lr = lr_table[clamp(*step, 0, lr_len - 1)], where *step is the number of optimizer
 * steps this stage has completed (advance it with slk_tick after the launch). A constant rate is a table of
 * length 1, a torch.optim.lr_scheduler schedule a table of its per-step values (the last one holds past the
 * end); no host value is baked into a captured HIP graph. Valid counter values are 0 <= *step <= 2^31 - 2: the
 * Adam-type entries form t = *step + 1 as an int, so *step = 2^31 - 1 (INT_MAX) is outside the contract of every
 * entry that takes `step`, and slk_tick must not be asked to advance a counter past 2^31 - 2. Per element, g = sum_s slabs[s*n+i] (the three
 * summation forms of slk_reduce_slabs); grad[i] = g (if grad != NULL, before weight decay); then
 *   g += weight_decay * p                                         (weight_decay != 0)
 *   buf = (*step == 0) ? g : momentum * buf + (1 - dampening) * g  (momentum != 0; buf may be NULL otherwise)
 *   g = nesterov ? g + momentum * buf : buf
 *   p -= lr * g.
 * With momentum 0, weight_decay 0 and a one-entry table the result is bitwise slk_sgd_from_slabs'.
 * Replaces optimizer.step() (client_part.py:133, server_part.py:52) for any torch.optim.SGD recipe and
 * scheduler.step() of torch.optim.lr_scheduler.*. */
int slk_sgdm_from_slabs(float* param, float* grad, float* buf, const float* slabs, int nslab, int n,
                        const float* lr_table, int lr_len, const int* step, float momentum, float dampening,
                        float weight_decay, int nesterov, void* stream);

/* slk_sgdm_from_slabs over nseg (<= 4) segments, one buf per segment, plus slk_loss_log when
 * loss_values != NULL, in ONE launch — bit-identical to the separate launches (the momentum form of
 * slk_sgd_multi_from_slabs; every segment needs a param). The pointer/size arrays are host memory. */
int slk_sgdm_multi_from_slabs(float* const* params, float* const* grads, float* const* bufs,
                              const float* const* slabs, const int* nslab, const int* n, int nseg,
                              const float* lr_table, int lr_len, const int* step, float momentum, float dampening,
                              float weight_decay, int nesterov, const float* loss_values, int loss_n,
                              float loss_scale, float* ring, int capacity, int* counter, void* stream);

/* Global-norm gradient clipping, torch.nn.utils.clip_grad_norm_(params, max_norm) (L2, error_if_nonfinite =
 * False) in front of slk_sgdm_* / slk_adamw_*, per GROUP of segments (a group = one stage = one torch
 * optimizer's parameters). The whole norm must be known before the first parameter moves, so the fused
 * reduce + step is two launches, both without atomics and bit-reproducible:
 *   1. slk_reduce_sqnorm_multi   grads[s] = sum of slabs[s] and one partial of sum g^2 per block;
 *   2. slk_sgdm_clip_multi / slk_adamw_clip_multi   every block sums its group's partials, forms
 *      norm = sqrt(sum), coef = max_norm / (norm + 1e-6) clamped from above at 1, and steps from coef * g.
 * Layout shared by both passes (host arrays of nseg <= 4 entries): group[s] in [0, ngroup), group[0] = 0,
 * group[s] = group[s-1] or group[s-1] + 1, the last one ngroup - 1. Segment s owns
 * slk_reduce_sqnorm_nblk(n[s], nslab[s]) consecutive floats of partials[group[s]], after those of the earlier
 * segments of its group (so each group's buffer holds the sum of its segments' counts, and nothing behind
 * that is written). Both passes must be given the same nslab, n and group. */

/* Blocks (= partials) of one segment in pass 1: ceil(n / 1024) for nslab <= 16, ceil(n / 256) for nslab <= 64,
 * else ceil(n / 64) — the three forms of slk_reduce_slabs; 0 when n or nslab is 0. */
int slk_reduce_sqnorm_nblk(int n, int nslab);

/* Pass 1. Per segment: grads[s][i] = sum_k slabs[s][k*n+i] in the form of slk_reduce_slabs for nslab[s]
 * (bitwise the grad slk_sgdm_from_slabs / slk_adamw_from_slabs write), and block blk of the segment writes
 * partial[blk] = sum over its columns of g*g in this float32 order: the thread that holds the finished sum
 * of a column squares it (one rounding); every other thread of the 1024 holds 0 — columns past n, and the
 * threads that only sum slabs: in the 256-column form the columns belong to threads 0..255 (waves 0..3), in
 * the 64-column form to wave 0, in the 1024-column form thread = column. Inside each of the 16 waves the 64
 * values are added as a balanced tree over neighbouring lanes (lane pairs, then 4, 8, 16, 32, 64 lanes); then
 * the 16 wave sums are added in ascending wave order, ((w0 + w1) + w2) + ... . With grads[s] == slabs[s]
 * (nslab[s] must be 1) the gradient block already holds the sum — after slk_reduce_slabs(accumulate) or an
 * all-reduce — and is only read. When loss_values != NULL one more block runs slk_loss_log, as in
 * slk_sgdm_multi_from_slabs. */
int slk_reduce_sqnorm_multi(float* const* grads, const float* const* slabs, const int* nslab, const int* n,
                            const int* group, int nseg, float* const* partials, int ngroup,
                            const float* loss_values, int loss_n, float loss_scale, float* ring, int capacity,
                            int* counter, void* stream);

/* Pass 2 for torch.optim.SGD. Every block (1024 elements of one segment) first sums the np partials of its
 * group: thread j (0..1023) adds partials j, j + 1024, j + 2048, ... in ascending order starting from 0; the
 * 1024 values are then added exactly as in pass 1 (the tree inside each wave, the 16 waves ascending). The
 * order depends on that group's partials alone, so a group's total is the same bits in every block and in any
 * launch, whatever shares it. Then, in float32, norm = sqrt(total), coef = *max_norm / (norm + 1e-6f),
 * coef = coef > 1 ? 1 : coef (a NaN norm keeps a NaN coef, as torch.clamp; an infinite one gives 0 and
 * inf * 0 = NaN parameters; a zero one gives 1), and slk_sgdm_from_slabs' arithmetic runs on
 * fl(coef * grads[s][i]) — clipping before weight decay. grads is only read: it keeps the UNCLIPPED reduced
 * gradient (the clipped one is coef * grads). The group's first block writes norm_out[g][0] = norm,
 * norm_out[g][1] = coef. max_norm is device memory (so is the rate): a captured HIP graph follows both.
 * *max_norm = inf gives coef = 1, bitwise slk_sgdm_multi_from_slabs. The caller ticks `step`. */
int slk_sgdm_clip_multi(float* const* params, const float* const* grads, float* const* bufs, const int* nslab,
                        const int* n, const int* group, int nseg, const float* const* partials,
                        float* const* norm_out, int ngroup, const float* max_norm, const float* lr_table,
                        int lr_len, const int* step, float momentum, float dampening, float weight_decay,
                        int nesterov, void* stream);

/* MNIST batch from the HBM-resident u8 dataset (replaces DataLoader(batch_size=64, shuffle=True)
 * over torchvision MNIST + ToTensor + Normalize((0.1307,),(0.3081,)), src/client_part.py:61-64,98):
 * x[s] = ((float)images[idx[s]] / 255 - mean) / std as f32 [B,1,28,28], y[s] = labels[idx[s]] (i64).
 * images: [n_images][784] u8 (4-byte aligned); x 16-byte aligned. An idx outside [0, n_images)
 * sets *err_flag (if non-null) and reads image 0. Bit-identical to the torchvision transform. */
int slk_mnist_batch(const uint8_t* images, const uint8_t* labels, int n_images, const int64_t* idx,
                    int B, float mean, float std, float* x, int64_t* y, int* err_flag, void* stream);

/* Training batch with augmentation from an HBM-resident u8 dataset images [n_images][C][H][W] (4-byte aligned)
 * and labels [n_images], one launch: for b < B and i = idx[b], torchvision's
 *   RandomCrop(H, padding=pad, fill 0) -> RandomHorizontalFlip(0.5) -> ToTensor() -> Normalize(mean[C], std[C])
 * as x f32 [B,C,H,W] (16-byte aligned) and y[b] = labels[i] (i64). With the sample's draws dy, dx in [0, 2*pad]
 * and flip in {0, 1}:
 *   xs = (flip ? W-1-xo : xo) + dx - pad;  ys = yo + dy - pad
 *   p  = (0 <= xs < W && 0 <= ys < H) ? images[i][c][ys][xs] : 0        (u8: the padding is in pixel space)
 *   x[b][c][yo][xo] = ((float)p / 255.0f - mean[c]) / std[c]            (f32, IEEE division, as slk_mnist_batch)
 * so a padded pixel is (0 - mean[c]) / std[c], not 0. The draws are a counter-based hash of the DATASET index,
 * not of the batch position b (all uint32 arithmetic, lowbias32 as in the K5 dropout mask):
 *   e  = (uint32)i * 0x9E3779B1 + epoch * 0x85EBCA77 + seed * 0xC2B2AE3D
 *   h0 = lowbias32(e);  h1 = lowbias32(h0 + 0x9E3779B9);  h2 = lowbias32(h1 + 0x9E3779B9)
 *   dy = ((uint64)h0 * (2*pad+1)) >> 32;  dx = ((uint64)h1 * (2*pad+1)) >> 32;  flip = flip_enabled ? h2 >> 31 : 0
 * so a sample's augmentation in an epoch does not depend on batch size, shuffle order or a ragged last batch.
 * The same distribution as torchvision's transforms from another random stream. pad = 0, flip_enabled = 0 is
 * plain gather + normalise (evaluation), bitwise slk_mnist_batch for (1,28,28).
 * (C,H,W) is (3,32,32) or (1,28,28); anything else, pad outside [0, 8], a null or misaligned pointer returns the
 * invalid-argument status without a launch; B == 0 returns 0. mean and std are HOST arrays of C floats, read
 * during the call and passed by value (like seed, epoch, pad, flip_enabled: a captured graph would keep them).
 * An idx outside [0, n_images) sets *err_flag (if non-null) and reads image 0 with image 0's draws. No byte
 * outside the dataset is ever addressed. */
int slk_image_batch(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                    const int64_t* idx, int B, const float* mean, const float* std, int pad, int flip_enabled,
                    uint32_t seed, uint32_t epoch, float* x, int64_t* y, int* err_flag, void* stream);

/* slk_image_batch with CutMix (Yun et al. 2019 with lam ~ Beta(1, 1), the paper's setting), one launch, the same two
 * shapes. For batch position s, i = idx[s] is the primary sample and i2 = idx2[s] (i64 [B]) its partner. Both get
 * their own crop and flip draws exactly as in slk_image_batch (h0..h2 of their own dataset index). The box comes
 * from the PRIMARY sample's hash chain, continued, all in integers (64-bit products):
 *   h3..h7 = lowbias32(previous + 0x9E3779B9), after h2
 *   apply  = (uint64)h3 < (uint64)(prob * 4294967296.0)         (the threshold is computed once on the host in double)
 *   side   = max((h4 * H) >> 32, (h5 * H) >> 32)                 (the max of two uniforms has density 2r: the law of
 *                                                                 sqrt(1 - lam) for lam ~ U(0, 1))
 *   cy = (h6 * H) >> 32;  cx = (h7 * W) >> 32
 *   y1 = clip(cy - side/2, 0, H);  y2 = clip(cy + side/2, 0, H)   (integer halves, as the paper's rand_bbox)
 *   x1 = clip(cx - side/2, 0, W);  x2 = clip(cx + side/2, 0, W)
 *   area = apply ? (y2 - y1) * (x2 - x1) : 0;   wb = (float)area / (float)(H * W)          (IEEE division)
 * Output pixel (c, yo, xo) is, for y1 <= yo < y2 and x1 <= xo < x2 (and apply), the u8 pixel sample i2 would have
 * at (c, yo, xo) under i2's own crop and flip, otherwise sample i's; then the same ToTensor / Normalize arithmetic.
 * y[s] = labels[i] | labels[i2] << 8 | (int64)float_bits(wb) << 32 (a mixed label, "soft targets" above); an
 * unapplied or empty box gives the plain label labels[i]. The box is keyed on (dataset index, epoch, seed) like the
 * crop, so it does not depend on batch size or order; only the partner does. prob = 0 gives bit for bit
 * slk_image_batch's x and plain labels; idx2 = idx gives its x and labels with a == b. prob outside [0, 1] or NaN
 * returns the invalid-argument status, as do slk_image_batch's own bad arguments and a null idx2. An idx2 outside
 * [0, n_images) behaves like an idx outside it (flag, then row 0 with row 0's draws). No byte outside the dataset
 * is ever addressed, for either source. Other Beta parameters and MixUp (a float blend) are slk_image_batch_blend's,
 * below; this entry keeps its bits. */
int slk_image_batch_mix(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                        const int64_t* idx, const int64_t* idx2, int B, const float* mean, const float* std, int pad,
                        int flip_enabled, uint32_t seed, uint32_t epoch, double prob, float* x, int64_t* y,
                        int* err_flag, void* stream);

/* slk_image_batch_mix with lam ~ Beta(alpha, alpha) from a quantile table, and MixUp (Zhang et al. 2018), chosen per
 * sample, one launch, the same two shapes. The arguments are slk_image_batch_mix's, plus two DEVICE tables of 1024
 * entries each, either of which may be NULL (not both), and switch_prob:
 *   cut_table[k] = min(floor(sqrt(1 - q_k) * 2^32), 2^32 - 1)     the box side ratio of CutMix, as a 32-bit fraction
 *   lam_table[k] = (float)q_k                                      the partner's weight of MixUp
 * with q_k the quantile of Beta(alpha, alpha) at (k + 0.5) / 1024 (splitcnn.loss.beta_quantiles builds them; each
 * table may have its own alpha). Primary i = idx[s] and partner i2 = idx2[s] get their own crop and flip draws
 * h0..h2 exactly as in slk_image_batch. The primary's chain is continued, h3..h7 = lowbias32(previous + 0x9E3779B9):
 *   apply = (uint64)h3 < (uint64)(prob * 4294967296.0)             (the samples slk_image_batch_mix would pick)
 *   cut   = both tables given ? (uint64)h4 < (uint64)(switch_prob * 4294967296.0) : (cut_table != NULL)
 *   k     = h5 >> 22                                               (table index, 0..1023)
 *   cy    = (h6 * H) >> 32;  cx = (h7 * W) >> 32                   (as in slk_image_batch_mix)
 * CutMix sample (apply && cut): side = ((uint64)cut_table[k] * H) >> 32; from side / 2 on, the box, the selection on
 * the u8 pixels, wb = area / (H * W) and the label are slk_image_batch_mix's.
 * MixUp sample (apply && !cut): wb = lam_table[k]. For every output pixel, pa and pb are the u8 pixels samples i and
 * i2 would show there, each under its own crop and flip (padding is 0 in pixel space). In float32, every operation
 * rounded on its own:
 *   fa = (float)pa / 255.0f;  fb = (float)pb / 255.0f;  om = 1.0f - wb
 *   f  = fadd_rn(fmul_rn(om, fa), fmul_rn(wb, fb))                 (two products and a sum, NOT an fma)
 *   x  = (f - mean[c]) / std[c]
 * and y[s] = wb > 0 ? labels[i] | labels[i2] << 8 | (int64)float_bits(wb) << 32 : labels[i]. wb = 0 (or a denormal)
 * gives bit for bit sample i's plain image, wb = 1 sample i2's. The blend is made BEFORE Normalize, on the ToTensor
 * values, and is neither fa + wb (fb - fa) nor a contracted form: those round differently.
 * Unapplied sample: slk_image_batch's bits and the plain label. prob = 0 is bitwise slk_image_batch. With only
 * cut_table given, a sample's apply, cy, cx equal slk_image_batch_mix's at the same (index, epoch, seed, prob).
 * One lam per SAMPLE out of 1024 values (timm's mode="elem" on a quantile table), not one per batch.
 * Both tables NULL, a misaligned table, prob or switch_prob outside [0, 1] or NaN, and every bad argument of
 * slk_image_batch_mix return the invalid-argument status without a launch; B == 0 returns 0. An idx / idx2 outside
 * [0, n_images) sets the flag and reads row 0 with row 0's draws. No byte outside the dataset is ever addressed, for
 * either source. The tables are only read and their values are not validated: a lam_table entry outside [0, 1]
 * reaches the soft heads' target check like any malformed label. */
int slk_image_batch_blend(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                          const int64_t* idx, const int64_t* idx2, int B, const float* mean, const float* std, int pad,
                          int flip_enabled, uint32_t seed, uint32_t epoch, double prob, const uint32_t* cut_table,
                          const float* lam_table, double switch_prob, float* x, int64_t* y, int* err_flag,
                          void* stream);


/* ================================================================ lossless cut-exchange codec (K3 / K4)
 * The multi-GPU topologies move the cut over RCCL instead of the reference's pickled HTTP body
 * (src/client_part.py:117-125 activations out, src/server_part.py:57-58 gradient back). The cut is a
 * ReLU output (about half zeros), so a micro-batch of n elements travels as mask (ceil(n/32) uint32
 * words: bit set where the element's bit pattern is nonzero) + the set elements in order, and the cut
 * gradient as its values at the same set positions only (the client applies its own ReLU mask, a subset
 * of the set bits, before using the gradient; the left-out positions never reach a result). Blocks of
 * 2048 elements: counts/offsets hold slk_cut_blocks(n) ints, total one int (the number of set bits).
 *   encode : mask, per-block counts, exclusive offsets, total, and the packed values of x;
 *   offsets: counts, offsets, total from a received mask;
 *   pack   : the values of x at the mask's set positions (the gradient direction);
 *   unpack : x = the values scattered to the set positions, zeros elsewhere. */
int slk_cut_blocks(int64_t n);
int slk_cut_encode(const float* x, int64_t n, uint32_t* mask, int* counts, int* offsets, int* total, float* vals,
                   void* stream);
int slk_cut_offsets(const uint32_t* mask, int64_t n, int* counts, int* offsets, int* total, void* stream);
int slk_cut_pack(const float* x, int64_t n, const uint32_t* mask, const int* offsets, float* vals, void* stream);
int slk_cut_unpack(const float* vals, int64_t n, const uint32_t* mask, const int* offsets, float* x, void* stream);
/* Fused consumers of a received micro-batch (the K3 / K4 server; each replaces an unpack or a pack pass over
 * the dense f32 cut, src/server_part.py:39-45 and :57-58):
 *   ranks      : ranks[w] (ceil(n/32) ints) = the vals index of mask word w's first set element
 *                (offsets of the block + the set bits of its earlier words), from slk_cut_offsets' offsets;
 *   unpack_x3  : the x3 input images of B samples (slk_conv2_act16_bytes(B) bytes, each sample at the scale
 *                of act_amax[b]) straight from mask + vals + ranks: the images slk_conv1_fwd_x3 would have
 *                written from the same cut (bit for bit), no dense f32 cut;
 *   dgrad_pack : slk_conv2_dgrad_x3 writing the cut gradient packed (values at the mask's set positions, at
 *                their ranks) — what slk_cut_pack would extract from its dense output. */
int slk_cut_ranks(const uint32_t* mask, int64_t n, const int* offsets, int* ranks, void* stream);
int slk_cut_unpack_x3(const float* vals, const uint32_t* mask, const int* ranks, const float* act_amax, int B,
                      uint16_t* act16, void* stream);
int slk_conv2_dgrad_x3_pack(const float* dpooled, const float* dp_amax, const uint8_t* code, const float* W2,
                            const uint32_t* mask, const int* ranks, float* vals, int B, void* stream);
/* The same over the np parts of one server chunk (one part per client, each n elements / part_b samples) in
 * one launch per pass: `parts` is a device table of pointers (uint64 each) —
 *   offsets_ranks_parts: [np][5] = (mask, counts, offsets, total, ranks): count + scan + ranks of every part;
 *   unpack_x3_parts    : [B / part_b][3] = (vals, mask, ranks); sample b reads part b / part_b;
 *   dgrad_x3_pack_parts: [B / part_b][3] = (mask, ranks, vals). */
int slk_cut_offsets_ranks_parts(const uint64_t* parts, int np, int64_t n, void* stream);
int slk_cut_unpack_x3_parts(const uint64_t* parts, int part_b, const float* act_amax, int B, uint16_t* act16,
                            void* stream);
int slk_conv2_dgrad_x3_pack_parts(const float* dpooled, const float* dp_amax, const uint8_t* code, const float* W2,
                                  const uint64_t* parts, int part_b, int B, void* stream);

/* ================================================================ widened split CNN (BASELINE config 5)
 * The reference has no such model: these entry points run the north star's
 * widened config — client conv1 3->64 (32x32) + ReLU, conv2 64->128 + ReLU + pool, conv3 128->256 +
 * ReLU + pool (the cut, [B,256,8,8]); server Dropout(0.25) + Linear(16384,10) + cross-entropy; Adam —
 * behind the same step contract (client_part.py:110-138 <-> server_part.py:25-58). Oracle:
 * oracle/wide_step.py. Activations are bf16 in the "C8" layout [B][C/8][H][W][8] (8 channels of one
 * pixel = one 16-byte chunk); routing codes are u8 in the same layout (0..3 = argmax position in the
 * 2x2 window, first max wins; 4 = ReLU-blocked). Weight masters are f32 in torch layout; the MFMA
 * convolutions read bf16 shadows built by slk_wide_shadows:
 *   w2f [tap][ci/8][co][8] (128x64)   w2d [8-tap][co/8][ci][8]
 *   w3f [co/128][tap][ci/8][co%128][8] (256x128)   w3d [8-tap][co/8][ci][8]
 * Client flat block: [W1 1728 | b1 64 | W2 73728 | b2 128 | W3 294912 | b3 256]; server: [Wf | bf]. */
#define SLK_WIDE_CLIENT_NPARAM 370816
#define SLK_WIDE_SERVER_NPARAM 163850

/* a1 = bf16(relu(conv1(bf16(x)) + b1)), x f32 NCHW [B,3,32,32]; one bf16 MFMA K-step (K = 27 -> 32);
 * w1b [64][32] bf16 from slk_wide_shadows. a1bits (may be NULL): the ReLU word of every pixel, [B][1024]
 * u64, bit c = (a1[c] > 0) — what slk_wide_conv2_dgrad masks with (8 KB a sample instead of a1's 128 KB). */
int slk_wide_conv1_fwd(const float* x, const uint16_t* w1b, const float* b1, uint16_t* a1, uint64_t* a1bits, int B,
                       void* stream);
/* The same ReLU words from a stored a1 (callers that hold a1 but not its words). */
int slk_wide_relu_bits(const uint16_t* a1, uint64_t* a1bits, int B, void* stream);
/* p2, code2 = pool(relu(conv2(a1) + b2)) — bf16 MFMA implicit GEMM, f32 accumulation. */
int slk_wide_conv2_fwd(const uint16_t* a1, const uint16_t* w2f, const float* b2, uint16_t* p2, uint8_t* code2,
                       int B, void* stream);
/* cut, code3 = pool(relu(conv3(p2) + b3)). The cut is what the client sends (client_part.py:117-125). */
int slk_wide_conv3_fwd(const uint16_t* p2, const uint16_t* w3f, const float* b3, uint16_t* cut, uint8_t* code3,
                       int B, void* stream);
/* Server: dropout (hash of seed, *step, b0 + sample, feature; keep iff hash >= keep_threshold, kept values
 * scaled by keep_scale), fc forward, cross-entropy forward+backward (dlogits scaled by grad_scale), the
 * cut gradient dcut = keep * keep_scale * dlogits @ Wf (bf16, C8) and the fc weight-gradient slabs
 * [slk_wide_head_nslab(B)][163850] = [dWf (torch layout) | dbf]. wf8 = slk_wide_fc_shadow(Wf);
 * work = slk_wide_head_work(B) floats of scratch (the step's dropout bits); b0 = global index of sample 0 (micro-batches and
 * SplitFed slices of one step draw the dropout mask of the concatenated batch). Replaces
 * server_part.py:48-51 + the cut-gradient return (:57) for the widened model. */
int slk_wide_head(const uint16_t* cut, const float* wf8, const float* bf, const int64_t* labels, const int* step,
                  unsigned seed, unsigned keep_threshold, float keep_scale, float grad_scale, float* logits,
                  float* loss_i, float* dlogits, uint16_t* dcut, float* slabs, float* work, int* err_flag, int b0,
                  int B, void* stream);
int slk_wide_head_nslab(int B);
int slk_wide_head_work(int B);
/* slk_wide_head with soft targets (mixed labels and `smoothing`: "soft targets" above, the same float32 expression
 * and the same malformed-target rule): the same dropout, logits, dcut, slabs and work; dcut and the slabs are what
 * slk_wide_head_bwd writes from this entry's dlogits, bit for bit. */
int slk_wide_head_soft(const uint16_t* cut, const float* wf8, const float* bf, const int64_t* labels, const int* step,
                       unsigned seed, unsigned keep_threshold, float keep_scale, float grad_scale, float smoothing,
                       float* logits, float* loss_i, float* dlogits, uint16_t* dcut, float* slabs, float* work,
                       int* err_flag, int b0, int B, void* stream);
/* slk_wide_head split at the loss, for the module path (WideModelPartB.forward -> criterion ->
 * loss.backward(), server_part.py:48-51): _fwd writes the logits (dropout + fc, the same kernel and
 * sum order as slk_wide_head, so bit-identical logits); _bwd takes dlogits from any loss and writes dcut and the fc slabs
 * exactly as slk_wide_head's last stage. */
int slk_wide_head_fwd(const uint16_t* cut, const float* wf8, const float* bf, const int* step, unsigned seed,
                      unsigned keep_threshold, float keep_scale, float* logits, int b0, int B, void* stream);
int slk_wide_head_bwd(const uint16_t* cut, const float* wf8, const float* dlogits, const int* step, unsigned seed,
                      unsigned keep_threshold, float keep_scale, uint16_t* dcut, float* slabs, int b0, int B,
                      void* stream);
/* Client backward (activations.backward(grads), client_part.py:132), with no unpooled gradient ever
 * stored: conv3's wgrad and dgrad apply conv3's max-pool backward (code3) to the POOLED cut gradient
 * dcut while staging it; conv3 wgrad slabs [nslab][294912 + 256]; dp2 = conv3 dgrad = the gradient of
 * p2 at its own 16 x 16 resolution (bf16, C8); conv2's dgrad and wgrad apply conv2's max-pool backward
 * (code2) to dp2 the same way; conv2 wgrad slabs [nslab][73728 + 128]; da1m = conv2 dgrad masked by
 * a1 > 0 (its ReLU words a1bits, slk_wide_conv1_fwd); conv1 wgrad slabs [nslab][1728 + 64] (bf16(x) operand). Slabs are [dW (torch layout) | db],
 * reduced in fixed order. */
int slk_wide_conv3_wgrad(const uint16_t* dcut, const uint8_t* code3, const uint16_t* p2, float* slabs, int B,
                         void* stream);
int slk_wide_conv3_wgrad_nslab(int B);
int slk_wide_conv3_dgrad(const uint16_t* dcut, const uint8_t* code3, const uint16_t* w3d, uint16_t* dp2, int B,
                         void* stream);
int slk_wide_conv2_wgrad(const uint16_t* dp2, const uint8_t* code2, const uint16_t* a1, float* slabs, int B,
                         void* stream);
int slk_wide_conv2_wgrad_nslab(int B);
/* Always 1: the K5 weight gradients run on the 2:4-sparse bf16 MFMA (the max-pool-routed dC); 0 named the dense
 * form, which is no longer built. */
int slk_wide_wgrad_form(void);
int slk_wide_conv2_dgrad(const uint16_t* dp2, const uint8_t* code2, const uint16_t* w2d, const uint64_t* a1bits,
                         uint16_t* da1m, int B, void* stream);
int slk_wide_conv1_wgrad(const float* x, const uint16_t* da1m, float* slabs, int B, void* stream);
int slk_wide_conv1_wgrad_nslab(int B);

/* Fixed-order slab reduction + torch.optim.Adam step (amsgrad off, no weight decay) on n floats:
 * t = *step + 1; grad (if non-null) receives the reduced gradient. Replaces optimizer.step() for the
 * widened config (the north star's "fused SGD/Adam"). */
int slk_adam_from_slabs(float* param, float* grad, float* m, float* v, const float* slabs, int nslab, int n,
                        float lr, float beta1, float beta2, float eps, const int* step, void* stream);

/* slk_adam_from_slabs over nseg (<= 4) parameter segments, each with its own slab set, in ONE launch
 * (bit-identical to the separate launches); grads may be NULL or hold NULL entries. The pointer and
 * size arrays are host memory. Replaces the per-parameter loop of the client's optimizer.step()
 * (torch.optim.Adam) for the widened model (src/client_part.py:133's call site). */
int slk_adam_multi_from_slabs(float* const* params, float* const* grads, float* const* m, float* const* v,
                              const float* const* slabs, const int* nslab, const int* n, int nseg, float lr,
                              float beta1, float beta2, float eps, const int* step, void* stream);

/* slk_adam_from_slabs with the rate read on the device (lr = lr_table[clamp(*step, 0, lr_len - 1)], as
 * slk_sgdm_from_slabs) and weight decay: decoupled = 1 is torch.optim.AdamW (p *= 1 - lr * weight_decay
 * before the update), decoupled = 0 is torch.optim.Adam(weight_decay=...) (g += weight_decay * p before the
 * moments). grad (if non-null) receives the reduced gradient before weight decay. With weight_decay 0 and a
 * one-entry table the result is bitwise slk_adam_from_slabs'. */
int slk_adamw_from_slabs(float* param, float* grad, float* m, float* v, const float* slabs, int nslab, int n,
                         const float* lr_table, int lr_len, const int* step, float beta1, float beta2, float eps,
                         float weight_decay, int decoupled, void* stream);
/* slk_adamw_from_slabs over nseg (<= 4) segments in ONE launch (bit-identical to the separate launches). */
int slk_adamw_multi_from_slabs(float* const* params, float* const* grads, float* const* m, float* const* v,
                               const float* const* slabs, const int* nslab, const int* n, int nseg,
                               const float* lr_table, int lr_len, const int* step, float beta1, float beta2,
                               float eps, float weight_decay, int decoupled, void* stream);
/* slk_sgdm_clip_multi with torch.optim.AdamW / Adam(weight_decay) in place of SGD: slk_adamw_from_slabs'
 * arithmetic on coef * grads[s][i] (clipping before either weight decay), after slk_reduce_sqnorm_multi over the
 * same segments. Arguments, groups, orders and outputs as slk_sgdm_clip_multi. */
int slk_adamw_clip_multi(float* const* params, const float* const* grads, float* const* m, float* const* v,
                         const int* nslab, const int* n, const int* group, int nseg, const float* const* partials,
                         float* const* norm_out, int ngroup, const float* max_norm, const float* lr_table,
                         int lr_len, const int* step, float beta1, float beta2, float eps, float weight_decay,
                         int decoupled, void* stream);
/* Layer-wise trust ratios: LARS (You, Gitman, Ginsburg 2017) on slk_sgdm_*'s arithmetic and LAMB (You et al.
 * 2019, algorithm 2) on slk_adamw_*'s. A TENSOR is one weight or one bias; a segment is one [W | b] pair:
 * elements [0, nw[s]) are the weight tensor, [nw[s], n[s]) the bias (nw = n: no bias; 0 <= nw <= n). Each
 * tensor's step is scaled by a ratio of two of its own L2 norms, which must exist before its first element
 * moves, so the fused reduce + step is two launches, both without atomics and bit-reproducible:
 *   LARS  1. slk_reduce_tnorm_multi   2. slk_lars_multi
 *   LAMB  1. slk_lamb_moments_multi   2. slk_lamb_multi
 * Segments, groups (a group = one stage), nslab, n and group are those of the clip launches above; both passes
 * must be given the same nslab, n, nw and group. Partials: block blk (< slk_reduce_sqnorm_nblk(n[s], nslab[s]))
 * of segment s owns the FOUR floats [x2_W, p2_W, x2_b, p2_b] at partials[group[s]][4 * (off + blk)], off the
 * block count of the group's earlier segments; a group's buffer holds 4 * (the sum of its segments' counts)
 * floats, 16-byte aligned. x is the reduced gradient g (LARS) or the update direction u (LAMB), p the parameter
 * before the step. trust_out[g] is f32 [2 * (segments of group g)][3]: rows 2k and 2k + 1 are
 * [w_norm, x_norm, ratio] of the weight and of the bias of the group's k-th segment, written by pass 2 (the
 * row of an empty tensor is not written). With exclude_bias != 0 a bias tensor runs at ratio = 1 and weight
 * decay 0 (its row reports the norms and ratio 1).
 *
 * Pass 1, float32 order. grads[s][i] = the fixed-order slab sum (bitwise slk_sgdm_from_slabs' /
 * slk_adamw_from_slabs'; grads[s] == slabs[s] with nslab 1: read in place, nothing written). The thread that
 * owns column i forms x2 = fl(x * x) and p2 = fl(p * p), each rounded on its own, and holds them in the weight
 * pair (i < nw) or the bias pair of its four values, the other pair 0 (a select: a NaN stays in its tensor);
 * every other thread holds four zeros (the owners are the threads slk_reduce_sqnorm_multi names). Each of the
 * four values is then summed over the block exactly as slk_reduce_sqnorm_multi's partial (the tree inside each
 * wave, the 16 waves ascending) and thread 0 writes the four sums. A block that straddles nw contributes to
 * both tensors. LAMB's owner first moves the moments with slk_adamw_from_slabs' expressions at weight decay 0,
 *   m = m + (1 - b1)(g - m);  v = v * b2 + g * g * (1 - b2)   (stored),
 * and forms, with t = *step + 1 and the bias corrections in double rounded to float32 as slk_adamw_from_slabs,
 *   denom = sqrt(v) / (float)sqrt(1 - b2^t) + eps;  c = fl(m / denom);
 *   u = fl(c * (float)(1 / (1 - b1^t))) + fl(wd * p)   (each product rounded on its own; wd = 0: the first).
 *
 * Pass 2: thread = element, 1024 per block. Every block sums its SEGMENT's partials, per component: thread j
 * adds partials j, j + 1024, ... ascending from 0, then the block sum as in pass 1 — a fixed function of the
 * segment's own partials, whatever shares the launch. w_norm = sqrt(sum p2), x_norm = sqrt(sum x2), then
 *   LARS  ratio = (w_norm > 0 && g_norm > 0) ? fl(trust_coef * w_norm) / ((g_norm + fl(wd * w_norm)) + eps) : 1
 *         d = fl(ratio * (g + fl(wd * p)))   (wd = 0: fl(ratio * g))
 *         then slk_sgdm_from_slabs' momentum / dampening / Nesterov arithmetic on d at weight decay 0:
 *         p -= lr * (that). An excluded bias has d = g: bitwise slk_sgdm_multi_from_slabs at weight decay 0.
 *   LAMB  ratio = (w_norm > 0 && u_norm > 0) ? w_norm / u_norm : 1
 *         u recomputed from the stored m, v and the unmodified p (pass 1's expression, the same bits),
 *         p = p - fl(fl(lr * ratio) * u).
 *         An excluded bias, and a tensor with w_norm == 0 (every p is 0: ratio 1 and no decay term), take the
 *         same update in slk_adamw_from_slabs' own expression p + (-(float)(lr / (1 - b1^t))) * (m / denom):
 *         bitwise slk_adamw_multi_from_slabs at weight decay 0.
 * A NaN norm fails both compares (ratio 1); the rate is lr_table[min(*step, lr_len - 1)]; the caller ticks
 * `step` after pass 2. When loss_values != NULL pass 1 runs one more block, slk_loss_log. */
int slk_reduce_tnorm_multi(float* const* grads, const float* const* params, const float* const* slabs,
                           const int* nslab, const int* n, const int* nw, const int* group, int nseg,
                           float* const* partials, int ngroup, const float* loss_values, int loss_n,
                           float loss_scale, float* ring, int capacity, int* counter, void* stream);
int slk_lars_multi(float* const* params, const float* const* grads, float* const* bufs, const int* nslab,
                   const int* n, const int* nw, const int* group, int nseg, const float* const* partials,
                   float* const* trust_out, int ngroup, const float* lr_table, int lr_len, const int* step,
                   float momentum, float dampening, float weight_decay, int nesterov, float trust_coef, float eps,
                   int exclude_bias, void* stream);
int slk_lamb_moments_multi(float* const* grads, const float* const* params, float* const* m, float* const* v,
                           const float* const* slabs, const int* nslab, const int* n, const int* nw,
                           const int* group, int nseg, float* const* partials, int ngroup, const int* step,
                           float beta1, float beta2, float eps, float weight_decay, int exclude_bias,
                           const float* loss_values, int loss_n, float loss_scale, float* ring, int capacity,
                           int* counter, void* stream);
int slk_lamb_multi(float* const* params, float* const* m, float* const* v, const int* nslab, const int* n,
                   const int* nw, const int* group, int nseg, const float* const* partials,
                   float* const* trust_out, int ngroup, const float* lr_table, int lr_len, const int* step,
                   float beta1, float beta2, float eps, float weight_decay, int exclude_bias, void* stream);
/* Exponential moving average of the parameters, after the step's optimizer launches and before the tick of
 * `step`: nseg (1 .. SLK_EMA_MAXSEG) segments (e[s], p[s], n[s]) move in ONE launch, e in place, p only read. The
 * pointer and size arrays are host memory (read at the call, so the launch is safe inside a stream capture);
 * `decay` (f32[1]) and `step` (i32[1], the optimizer steps completed BEFORE this one) are device memory read by
 * the kernel, so a captured graph follows both; `start` (>= 0) and `warmup` (0 / 1) travel by value and a captured
 * graph keeps them. With k = *step and t = k - start:
 *   t <  0:  e[i] = p[i]                 a copy of the bits (NaN payloads and -0.0 included)
 *   t >= 0:  n  = t + 1                  (an integer in [1, 2^31])
 *            nf = (float)n               round to nearest even; exact up to 2^24, above that nf is the nearest
 *                                        float32 (spacing 2, 4, ... 128), still non-decreasing in n
 *            w  = fl(fl(1 + nf) / fl(10 + nf))    correctly rounded division; w < 1 until n is about 1.5e8, then 1
 *            d  = warmup ? (w < *decay ? w : *decay) : *decay     (TensorFlow's / torch_ema's num_updates form;
 *                                        once w >= *decay — at the latest when w rounds to 1 — d is *decay for good)
 *            omd = fl(1 - d)
 *            e[i] = fma(omd, fl(p[i] - e[i]), e[i])   the difference rounded on its own, the product and the sum
 *                                        fused: one rounding (torch's AveragedModel lerp e + (1 - d)(p - e))
 * NaN and +-inf in p[i] propagate into e[i] by this arithmetic alone and reach no other element. Every element
 * is read and written by exactly one thread, without atomics; its result depends on e[i], p[i], *decay, *step,
 * start and warmup only — not on the grid, the segment's place in the launch or the pointers' alignment. e[s] and
 * p[s] need 4-byte alignment; where both have the same 16-byte phase the body moves as 16-byte vectors behind a
 * scalar head, otherwise the segment moves by scalars. n[s] = 0 is legal (its pointers may then be NULL).
 * Refused with hipErrorInvalidValue, nothing launched: a NULL argument or segment pointer (n[s] > 0), nseg outside
 * [1, SLK_EMA_MAXSEG], n[s] < 0, start < 0, a pointer not 4-byte aligned, e[s] == p[s] or any overlap of the two
 * blocks of a segment. */
#define SLK_EMA_MAXSEG 8
int slk_ema_multi(float* const* e, const float* const* p, const int* n, int nseg, const float* decay,
                  const int* step, int start, int warmup, void* stream);
/* FP8 cut records (csrc/slk_cut8.hip): an opt-in, lossy wire format of the K5 cut and of its gradient. A sample
 * is the 16,384 contiguous bf16 elements of one cut [256,8,8] (C8 layout in memory; the codec is elementwise, so
 * the layout does not matter) or of one cut-gradient row. fmt 0 = "e4m3" (OCP e4m3fn, F_MAX 448), fmt 1 = "e5m2"
 * (OCP e5m2, F_MAX 57344); the convention is e4m3 forward, e5m2 backward.
 * Record: one sample becomes 16,400 bytes (16 x 1025), records contiguous: u8 [n, 16400], so a slice of samples
 * is a slice of bytes. The base pointer must be 16-byte aligned.
 *   bytes 0..3   int32 e, little endian          bytes 8..15      zero
 *   bytes 4..7   uint32 fmt                      bytes 16..16399  payload, byte i = the fp8 code of element i
 * Encode: amax = max |x_i| over the sample. amax == 0: e = 0; otherwise e is the smallest integer with
 * amax * 2^-e <= F_MAX, clamped below at -100. y_i = x_i * 2^-e (an exact float32 product of a bf16 value and a
 * power of two) is converted to fp8 round-to-nearest-even; |y_i| <= F_MAX by construction, so nothing saturates
 * and neither format's NaN or inf codes are produced; a result of zero keeps the sign of x_i. A sample with any
 * non-finite element is poisoned: e = 0x7FFFFFFF and an all-zero payload.
 * Decode: x^_i = fp8_to_f32(payload_i) * 2^e written as bf16 — exact: at most 4 significant bits, and e >= -100
 * keeps it a normal bf16 — with one exception at the top of bf16's range: where the product of a finite code is
 * 2^128 or more it is written as the largest finite bf16 of its sign (0x7F7F / 0xFF7F), never as inf. An encoder
 * produces such a code only for a sample whose amax lies in bf16's top binade and rounds up past it (amax =
 * 255 * 2^120 becomes 256 * 2^120 in e4m3); saturating there is nearer to x than the bound below asks and keeps
 * the idempotence. A poisoned record decodes to 16,384 bf16 NaNs (0x7FC0). A record is malformed if its
 * fmt word is not `fmt`, bytes 8..15 are not zero, or e is outside [-100, 127] and not the poison value: it
 * decodes to NaNs as well and sets err_flag[0] = 1 (a plain store; nobody clears it). NaN and inf codes inside a
 * received payload convert and propagate (a NaN code of either sign gives 0x7FC0).
 * Error: |x - x^| <= max(|x| * 2^-(m+1), 2^e * 2^(emin-m-1)), (m, emin) = (3, -6) for e4m3 and (2, -14) for
 * e5m2. decode(encode(.)) is idempotent in decoded bits (the records may differ: e drops by one where the
 * rounded amax falls onto F_MAX / 2).
 * slk_cut8_roundtrip is bitwise decode(encode(x)) in one launch with no record in memory; out may equal x.
 * One block per sample; every output byte is written by exactly one thread, without atomics. n == 0 launches
 * nothing and returns 0; n < 0, fmt outside {0, 1}, a NULL pointer or a pointer that is not 16-byte aligned
 * (err_flag: 4-byte) is refused with hipErrorInvalidValue before any launch. */
int slk_cut8_encode(const void* x_bf16, int n, int fmt, void* rec, void* stream);
int slk_cut8_decode(const void* rec, int n, int fmt, void* out_bf16, int* err_flag, void* stream);
int slk_cut8_roundtrip(const void* x_bf16, int n, int fmt, void* out_bf16, void* stream);
int64_t slk_cut8_record_bytes(void); /* 16400 */
/* FP8 cut records: stochastic rounding. The record format, e, poisoning, the decode and the saturation at the top of
 * bf16's range are those above; a record written here is an ordinary record for slk_cut8_decode. Only the conversion
 * of y_i = x_i * 2^-e changes: each element goes to one of its two neighbouring codes, with probabilities that make
 * the expectation equal to y_i.
 * The random word (all uint32 arithmetic, lowbias32 as in the K5 dropout mask): with g = row0 + the sample's row in
 * the launch, t = *step (a device int32[1] the kernel reads and never writes; a captured graph follows it) and i the
 * element's index 0..16383,
 *   base = lowbias32(g * 0x9E3779B1 + t * 0x85EBCA77 + seed * 0xC2B2AE3D + (fmt + 1) * 0x27D4EB2F)
 *   r_i  = lowbias32(base + i * 0x9E3779B1)
 * so a slice of rows encoded with its own row0 gives the rows of the whole launch.
 * The rounding: |y| = sig * 2^q with the integer sig < 256 of the bf16 value; p = floor(log2 |y|), pe = max(p, emin),
 * and the target's quantum is 2^s units of sig, s = pe - m - q. For s <= 0 the value is representable and the code
 * is the nearest-rounding code. Otherwise k = sig >> s, rem = sig - (k << s), and the magnitude code is k + up with
 * the exponent field (pe - emin) << m added on, so a carry lands in the exponent by the addition; the sign is
 * copied, and a zero result keeps the sign of x_i. With nb = 23 - m (20 for e4m3, 21 for e5m2) and R = r_i >> (32 - nb),
 *   T = rem << (nb - s) for s <= nb, rem >> (s - nb) above;   up = (R + T) >> nb   (the carry out of nb bits)
 * — the mapping of gfx950's v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32 (they add r's top nb bits to the float32 fraction
 * bits they discard), which the kernels use; cut8::encode_one_sr (csrc/slk_cut8.h) is this rule in integer C++ and
 * the specification. rem = 0 never rounds up; for s <= nb exactly rem * 2^(nb - s) of the 2^nb values of R round up,
 * P(up) = rem / 2^s; for s > nb (a result more than nb - 8 binades below the smallest subnormal's) the count is
 * floor(rem * 2^(nb - s)), a downward bias below 2^-nb of one quantum. |y| <= F_MAX and F_MAX is representable, so
 * nothing saturates and no NaN or inf code is produced.
 * Error: |x - x^| < max(|x| * 2^-m, 2^e * 2^(emin-m)), strict, twice the nearest bound. A value that nearest
 * rounding reproduces is reproduced for every r: roundtrip_sr(roundtrip(x)) == roundtrip(x) bit for bit, except for
 * the saturated 0x7F7F / 0xFF7F at the top of bf16's range, which is no multiple of a quantum and goes to either of
 * its neighbours (the upper one saturates again).
 * slk_cut8_roundtrip_sr is bitwise decode(encode_sr(x)); out may equal x. Poisoned and all-zero samples, the launch
 * shape and the refusals are those of slk_cut8_encode / slk_cut8_roundtrip; also refused: a NULL step or one that is
 * not 4-byte aligned, and row0 < 0. */
int slk_cut8_encode_sr(const void* x_bf16, int n, int fmt, void* rec, uint32_t seed, const int* step, int row0,
                       void* stream);
int slk_cut8_roundtrip_sr(const void* x_bf16, int n, int fmt, void* out_bf16, uint32_t seed, const int* step, int row0,
                          void* stream);
/* MX cut records (csrc/slk_cutmx.hip): an opt-in, lossy, block-scaled wire format of the K5 cut and of its gradient
 * after the OCP Microscaling formats — one E8M0 power-of-two scale per 32 elements and narrow element codes — where
 * the FP8 records above have one scale per sample. A sample is the 16,384 contiguous bf16 elements of one cut or
 * cut-gradient row, as in the FP8 records; a block is 32 consecutive elements of the row as stored, 512 blocks a
 * sample (the codec is elementwise in memory order, so the C8 layout does not matter).
 * Element formats: fmt 0 = "e2m1" (OCP FP4: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; F_MAX = 6, m = 1, emin = 0; no
 * NaN or inf code; the code is sign << 3 | exp << 1 | man), fmt 1 = "e4m3" (OCP e4m3fn, exactly the FP8 records'
 * format 0: F_MAX = 448, m = 3, emin = -6).
 * Per-block scale: a block with a non-finite element is poisoned: scale byte 0xFF (E8M0's NaN) and all-zero codes.
 * Otherwise amax = max |x_i| over the block; e = 0 if amax == 0, else e is the smallest integer with
 * amax * 2^-e <= F_MAX, clamped below at -100 (the FP8 records' clamp, for the same reason: no product ever depends
 * on float32 subnormal handling). The scale byte is e + 127. Nothing saturates — a deliberate deviation from the
 * OCP v1.0 suggestion e = floor(log2 amax) - emax_elem, which clips the values between F_MAX * 2^e and 2^(e+1) times
 * the element format's top binade; the record is still a valid MX block, since any E8M0 scale is — and this keeps the
 * FP8 records' error bound per block: |x - x^| <= max(|x| * 2^-(m+1), 2^e * 2^(emin-m-1)).
 * Codes: each code is x_i * 2^-e (an exact float32 product) rounded to nearest even; a zero result keeps the sign of
 * x_i (e2m1 has a -0 code, 0x8).
 * Record: u8 [n, R], records contiguous, the base 16-byte aligned; R = 8,720 (e2m1) or 16,912 (e4m3), both multiples
 * of 16, so a slice of samples is an aligned slice of bytes.
 *   bytes 0..15     header: uint32 words, little endian: word 0 = 32 (the block length), word 1 = 0x10 + fmt,
 *                   words 2 and 3 = 0. The format words are disjoint from the FP8 records' (0, 1), so each decoder
 *                   reports the other's record as malformed.
 *   bytes 16..527   512 scale bytes, one per block, in block order
 *   bytes 528..     payload. e2m1: 8,192 bytes, element 2i in bits 0..3 of byte i, element 2i + 1 in bits 4..7.
 *                   e4m3: 16,384 bytes, one per element.
 * Decode: x^_i = value(code_i) * 2^e written as bf16 — exact (at most four significant bits, and e >= -100 keeps it
 * a normal bf16) — with the FP8 records' one exception at the top of bf16's range: a finite code whose product is at
 * or past 2^128 (amax = 255 * 2^120 rounds to 4 * 2^126 in e2m1, to 256 * 2^120 in e4m3) is written as the largest
 * finite bf16 of its sign. decode(encode(.)) is idempotent in decoded bits and finite inputs stay finite. A poisoned
 * block decodes to 32 NaNs (0x7FC0): a non-finite element poisons its block, not its sample. Malformed records: a
 * wrong header word decodes the whole sample to NaNs and stores err_flag[0] = 1; a scale byte below 27 (e < -100)
 * decodes that block to 32 NaNs and stores err_flag[0] = 1, the other blocks decode as usual (a plain store; nobody
 * clears it). An e4m3 NaN code inside a received payload propagates as 0x7FC0.
 * slk_cutmx_roundtrip is bitwise decode(encode(x)) in one launch with no record in memory; out may equal x.
 * Order inside a training step (wide.WideTrainer(cut_codec=codec.MxCut(...))): the cut noise if any,
 * slk_cutmx_roundtrip in the forward format, the head, slk_cutmx_roundtrip in the backward format in place, the
 * clip's slk_cut_scale_rows if any, the client's backward.
 * One workgroup of 256 threads per sample, a thread owning two whole blocks: each input byte is read once with
 * 16-byte loads, every output byte is written by exactly one thread (the scale bytes of four lanes as one word),
 * without atomics, LDS or barriers. cutmx::* in csrc/slk_cutmx.h is this rule in integer C++ that also compiles for
 * the host. n == 0 launches nothing and returns 0; n < 0, fmt outside {0, 1}, a NULL pointer or a pointer that is
 * not 16-byte aligned (err_flag: 4-byte) is refused with hipErrorInvalidValue before any launch. */
int slk_cutmx_encode(const void* x_bf16, int n, int fmt, void* rec, void* stream);
int slk_cutmx_decode(const void* rec, int n, int fmt, void* out_bf16, int* err_flag, void* stream);
int slk_cutmx_roundtrip(const void* x_bf16, int n, int fmt, void* out_bf16, void* stream);
int64_t slk_cutmx_record_bytes(int fmt); /* 8720 / 16912; -1 for another fmt */
/* Cut noise (csrc/slk_cut_noise.hip): an opt-in defence of the K5 cut against model inversion — a per-sample norm
 * bound, then additive noise from a 1,024-entry table. An experiment's tool, not a certified mechanism: no epsilon
 * is claimed. A sample is the 16,384 contiguous bf16 elements of one cut row, as in the FP8 records. All float
 * arithmetic is float32 and EVERY operation is rounded on its own (fl(.) below): no fma contraction anywhere.
 * Clip (only where max_norm is not NULL; max_norm is a device f32[1], so a captured graph follows it):
 *   s2 = sum x_i^2 in one fixed order. Thread t of 256 holds elements [16 (256 j + t), +16), j = 0..3, and adds
 *        fl(x_i * x_i) one at a time from 0, j ascending, then the element ascending. Inside each wave of 64 the xor
 *        butterfly a = a + shfl_xor(a, o) runs for o = 32, 16, 8, 4, 2, 1; the four waves' sums w0..w3 (threads
 *        64 w .. 64 w + 63) combine as (w0 + w1) + (w2 + w3).
 *   norm = sqrt(s2);  coef = *max_norm / (norm + 1e-6f), replaced by 1 where it compares greater than 1
 *        (slk_clip_coef's formulation); the square root and the division are correctly rounded.
 *        *max_norm = inf gives coef = 1 for a finite norm. stats[row] = (norm, coef), f32 pairs, where stats is given.
 *   c_i = fl(coef * x_i).      Without max_norm nothing is reduced, stats is not written and c_i = x_i exactly.
 * Draw (only where scale is not NULL; scale is a device f32[1]). All uint32 arithmetic, lowbias32 as in the K5
 * dropout mask; g = row0 + the sample's row in the launch, t = *step (a device int32[1] read as uint32 and never
 * written; a captured graph follows it), i the element's index 0..16383:
 *   base = lowbias32(g * 0x9E3779B1 + t * 0x85EBCA77 + seed * 0xC2B2AE3D + 3 * 0x27D4EB2F)    (cut8 uses 1 and 2)
 *   r    = lowbias32(base + i * 0x9E3779B1);     r2 = lowbias32(r + 0x9E3779B9)
 *   neg  = r >> 31;    k = (r >> 21) & 1023;     G = clz(r2), 32 for r2 = 0
 *   a    = fl(fl(tail * (float)G) + table[k]);   n = fl(*scale * a), its sign bit flipped where neg
 *   y_i  = bf16_rne(fl(c_i + n))
 * so a slice of rows launched with its own row0 gives the rows of the whole launch. table is a device f32[1024]
 * (16-byte aligned; its values are not validated), tail a by-value float. Without scale, y_i = bf16_rne(c_i) and
 * table, tail, seed, step and row0 are not read.
 * The two laws the Python side builds (splitcnn/privacy.py):
 *   Laplace(b):   -ln U = G ln 2 + (-ln U'), G geometric, U' uniform on (1/2, 1), so tail = f32(ln 2), table[k] =
 *                 f32(-log1p(-(k + 0.5) / 2048)), *scale = b: exact in distribution up to the 1,024 strata of U'; the
 *                 magnitude ends at about 32 ln 2 b, a cut of probability 2^-32 per element.
 *   Gaussian(s):  tail = 0, table[k] = the half-normal quantile at (k + 0.5) / 1024, *scale = s: 2,048 values, the
 *                 support ends at 3.487 s and the table's variance is 0.99936.
 * NaN and +-inf follow IEEE with no special case ("NaN and +-inf" clause 7): a NaN result is a quiet NaN of
 * unspecified sign and payload.
 * Backward (slk_cut_scale_rows): the noise is additive and the clip coefficient is treated as a CONSTANT (detached,
 * as the FP8 codec is straight-through), so the client back-propagates out_i = bf16_rne(fl(coef_row * x_i)) with
 * coef_row = stats[row][1] — a deviation from differentiating through the norm, which would add a term along x. A
 * coef of 1 leaves every finite element's bits.
 * One block of 256 threads per sample; the sample is read once and held in registers; the table is staged once per
 * block in LDS; every output element and every stats pair is written by exactly one thread with ordinary vector
 * stores, without atomics. out may equal x. n == 0 launches nothing and returns 0. Refused with
 * hipErrorInvalidValue before any launch: n < 0, row0 < 0, a NULL x / out (or stats for slk_cut_scale_rows), x or
 * out not 16-byte aligned, stats not 8-byte aligned, max_norm or scale not 4-byte aligned, and with scale a NULL or
 * misaligned table (16 bytes) or step (4 bytes). stats may be NULL in slk_cut_noise (the pairs are then not kept). */
int slk_cut_noise(const void* x_bf16, int n, const float* table, float tail, const float* scale,
                  const float* max_norm, uint32_t seed, const int* step, int row0, void* out_bf16, float* stats,
                  void* stream);
int slk_cut_scale_rows(const void* x_bf16, int n, const float* stats, void* out_bf16, void* stream);
/* Rebuild the bf16 weight shadows from the f32 masters: w1b [64][32] (W1 rows, k >= 27 zero) and the
 * MFMA layouts of W2 [128,64,3,3] and W3 [256,128,3,3]. */
int slk_wide_shadows(const float* W1, const float* W2, const float* W3, uint16_t* w1b, uint16_t* w2f, uint16_t* w2d,
                     uint16_t* w3f, uint16_t* w3d, void* stream);
/* wf8[j][(plane*64+pix)*8+k] = Wf[j][(plane*8+k)*64+pix]: the fc weight in the cut's C8 order. */
int slk_wide_fc_shadow(const float* wf, float* wf8, void* stream);
/* ++*counter on the device (the per-stage step counter a captured HIP graph advances). A step counter stays in
 * [0, 2^31 - 2] (see slk_sgdm_from_slabs): ticking one that already holds 2^31 - 2 leaves it at INT_MAX, which no
 * optimizer entry accepts, and one more tick overflows the int. */
int slk_tick(int* counter, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLK_H */
