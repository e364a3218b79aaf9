/*
 * rpn_hip.h -- C ABI of librpn_hip.so: the MI355X (gfx950) Region Proposal Network
 * forward / proposal path.
 *
 * The reference (FurkanOM/tf-rpn) is pure Python on TensorFlow 2.0 and has no FFI of
 * its own; the boundary it offers is a handful of Python call signatures.  Every entry
 * point below names the reference interface (file:line under /root/reference) it
 * replaces; tf_rpn_amd/ binds them with ctypes under the reference's own function
 * names (INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - all `d_` pointers are DEVICE pointers (hipMalloc / torch.cuda storage), float32,
 *     row-major, box order [y1, x1, y2, x2]; the caller allocates every output.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call
 *     is asynchronous on that stream and never synchronises the device.
 *   - return value: 0 on success, a negative rpn_status otherwise; rpn_last_error()
 *     returns a thread-local human-readable message for the last failure.
 *   - there is NO CPU fallback: without a HIP device every compute call fails with
 *     RPN_ERR_NO_DEVICE.
 *
 * Environment knobs of the library (read once per process).  These are ALL the names the
 * shipped library reads (tests/test_host.py compares this list with the binary's strings);
 * every setting computes the same arithmetic contract -- integer / index outputs bit-exact,
 * floats within the documented bound -- they select between implementations:
 *   RPN_KNOB RPN_B1_FUSE     (1)  VGG16 block 1 as one launch under f16x3; 0: two kernels
 *   RPN_KNOB RPN_HEAD_SPLITK (1)  rpn_reg | rpn_cls on the split-K head kernel; 0: generic f32 implicit GEMM
 *   RPN_KNOB RPN_KSPLIT      (1)  rpn_conv (split-precision modes) as a K tree: four fixed leaves of K, value (l0 + l1) +
 *                                 (l2 + l3) at every batch size, computed by 1, 2 or 4 workgroups per tile as the grid
 *                                 allows (same bits); 0: one accumulation chain, one workgroup per tile
 *   RPN_KNOB RPN_S16_DYN     (0)  1: dynamic tile queue in the persistent split-precision conv kernel
 *   RPN_KNOB RPN_S16_C64     (0)  1: block1_conv2 on the persistent kernel's 64-wide tiles
 *   RPN_KNOB RPN_NMS_LINEAR  (1)  NMS band selection from the linear score histogram; 0: radix select +
 *                                 bitonic sort only; 2: histogram select, sorted the old way
 *   RPN_KNOB RPN_NMS_CLUSTER (0 = automatic)  workgroups per (image, class) that share the NMS band selection
 *                                 when few images have many anchors; 1: always one workgroup
 *   RPN_KNOB RPN_NMS_PRUNE   (1)  NMS candidates meet only the selected boxes whose AREA allows the IoU threshold
 *                                 (area-ordered copy of the selected list); 0: the whole list
 *   RPN_KNOB RPN_MN_FUSE     (1)  MobileNetV2: one launch per inverted-residual block; 0: layer by layer
 *   RPN_KNOB RPN_MN_X3       (1)  MobileNetV2 under f16x3: 16-bit MFMA GEMMs inside the fused blocks; 0: f32 MFMA
 * Kernel / tile selection switches for A/B timing and the timing experiments whose results are
 * wrong on purpose (RPN_NMS_STOP, RPN_IOU_EXP, RPN_SPLIT_*, RPN_IOU_*, ...) exist only in a
 * laboratory build (`make -C tf_rpn_amd/csrc lab` -> librpn_hip_lab.so, -DRPN_LAB); the product
 * library does not contain their names.
 */
#ifndef RPN_HIP_H
#define RPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPN_ABI_VERSION 1

typedef enum rpn_status {
    RPN_OK = 0,
    RPN_ERR_INVALID = -1,      /* bad argument (shape, null pointer, unsupported size) */
    RPN_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime error */
    RPN_ERR_WORKSPACE = -3,    /* workspace too small */
    RPN_ERR_UNSUPPORTED = -4   /* configuration outside the implemented range */
} rpn_status;

typedef enum rpn_backbone { RPN_BACKBONE_VGG16 = 0, RPN_BACKBONE_MOBILENET_V2 = 1 } rpn_backbone;

/* arithmetic of the conv stack.  F32: exact float32 MFMA (v_mfma_f32_32x32x2_f32), bit-for-bit
 * an ordered fmaf chain.  BF16X3 / F16X3: in the 3x3 stride-1 layers every float32 operand is carried
 * as hi + lo 16-bit halves (bfloat16 / float16) and each product is formed as
 * hi*hi + hi*lo + lo*hi on the 16-bit MFMA with float32 accumulation (product error ~2^-16 / ~2^-21
 * relative; measured against the 1e-4 parity bound in tests/, never assumed).  F16X3 requires
 * |activation| < 65504.  All other layers stay on the float32 kernels. */
typedef enum rpn_precision { RPN_PRECISION_F32 = 0, RPN_PRECISION_BF16X3 = 1, RPN_PRECISION_F16X3 = 2,
                             RPN_PRECISION_F32W = 3 /* float32 Winograd for the 3x3 stride-1 convs -- F(4x4,3x3) where its tiles
                                                       fill the chip, F(2x2,3x3) otherwise, chosen per model handle: float32
                                                       operands and accumulation, 1/4 / 1/2.25 of the multiply-adds, another
                                                       summation order (1e-4 contract; measured 3e-6 ... 6e-6 on the heads) */
} rpn_precision;

int rpn_abi_version(void);
const char *rpn_last_error(void);
/* number of visible HIP devices (0 when there is none); never fails */
int rpn_device_count(void);
/* Stream diagnostic: enqueue ONE wave on `stream` that sleeps for `microseconds` (0 .. 10000) of the device's real-time counter.
 * HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4); two streams that share a queue run one behind
 * the other.  The predictor loop (predictor.py:46-60 restated with the NMS of batch k beside the convs of batch k + 1) needs its
 * two streams on DIFFERENT queues: spin both and compare the elapsed time (tf_rpn_amd/predictor.py: _streams_overlap). */
int rpn_stream_spin(void *stream, int microseconds);

/* ------------------------------------------------------------------------------------
 * generate_anchors(hyper_params) -> (A,4)            utils/bbox_utils.py:23-46 (+ :3-21)
 *   A = feature_map_shape^2 * n_ratios * n_scales, flat index (y*F + x)*K + k,
 *   k = scale_idx*n_ratios + ratio_idx.  ratios / scales are the python floats of
 *   hyper_params["anchor_ratios"/"anchor_scales"] (HOST arrays of double).
 * ---------------------------------------------------------------------------------- */
int rpn_generate_anchors(double img_size, int feature_map_shape, const double *ratios, int n_ratios,
                         const double *scales, int n_scales, float *d_anchors, void *stream);

/* ------------------------------------------------------------------------------------
 * get_bboxes_from_deltas(anchors, deltas) -> (B,A,4)          utils/bbox_utils.py:72-96
 *   fused with the caller's `rpn_bbox_deltas *= variances`       predictor.py:55
 *   d_anchors is (A,4) when anchors_batched == 0 (the predictor.py:56 call shape), else (B,A,4).
 *   variances: HOST pointer to 4 floats, or NULL for no scaling.
 * ---------------------------------------------------------------------------------- */
int rpn_decode(const float *d_anchors, int anchors_batched, const float *d_deltas, const float *variances,
               int B, int A, float *d_boxes, void *stream);

/* get_deltas_from_bboxes(bboxes, gt_boxes) -> (B,A,4)        utils/bbox_utils.py:98-124 */
int rpn_encode(const float *d_bboxes, int bboxes_batched, const float *d_gt_boxes, int B, int A,
               float *d_deltas, void *stream);

/* normalize_bboxes / denormalize_bboxes(bboxes, height, width)     utils/bbox_utils.py:152-166 / :168-182
 *   nboxes boxes of 4 floats; denormalize != 0 multiplies and rounds half-to-even (tf.round), else divides */
int rpn_scale_boxes(const float *d_boxes, long long nboxes, float height, float width, int denormalize,
                    float *d_out, void *stream);

/* ------------------------------------------------------------------------------------
 * generate_iou_map(bboxes, gt_boxes) -> (B,A,G)              utils/bbox_utils.py:126-150
 *   d_bboxes is (A,4) when bboxes_batched == 0 (the utils/train_utils.py:106 call shape).
 * ---------------------------------------------------------------------------------- */
int rpn_iou_map(const float *d_bboxes, int bboxes_batched, int A, const float *d_gt_boxes, int B, int G,
                float *d_iou, void *stream);

/* ------------------------------------------------------------------------------------
 * non_max_suppression(pred_bboxes, pred_labels, **kwargs)      utils/bbox_utils.py:48-70
 *   == tf.image.combined_non_max_suppression (TF 2.0.0 kernel semantics).
 *   d_boxes (B,N,q,4) with q in {1,C}; d_scores (B,N,C).
 *   Outputs (M = max_total; the pad_per_class rule is applied by the caller):
 *   d_out_boxes (B,M,4), d_out_scores (B,M), d_out_classes (B,M) float32,
 *   d_out_valid (B) int32, and -- not returned by TF, for parity checks -- d_out_idx (B,M)
 *   int32 box indices (-1 padded; may be NULL).
 *   d_workspace: rpn_nms_workspace_bytes(...) bytes of device scratch (may be NULL if 0).  For C > 1 the
 *   staging part is REQUIRED (RPN_ERR_WORKSPACE otherwise).  For few (image, class) pairs with many
 *   candidates (<= 32 pairs, N >= 16384) the size also covers the "cluster" scratch with which several
 *   workgroups per pair share the passes over the scores; a call that passes less (or NULL) still
 *   succeeds with identical results on one workgroup per pair.  rpn_decode_nms takes the same scratch:
 *   rpn_nms_workspace_bytes(B, A, 1, max_total, max_total).
 * ---------------------------------------------------------------------------------- */
size_t rpn_nms_workspace_bytes(int B, int N, int C, int max_per_class, int max_total);
int rpn_combined_nms(const float *d_boxes, const float *d_scores, int B, int N, int q, int C,
                     int max_per_class, int max_total, float iou_threshold, float score_threshold,
                     int clip_boxes, float *d_out_boxes, float *d_out_scores, float *d_out_classes,
                     int32_t *d_out_idx, int32_t *d_out_valid, void *d_workspace, size_t workspace_bytes,
                     void *stream);

/* ------------------------------------------------------------------------------------
 * predictor.py:52-56 + NMS in one launch sequence: (reg,cls) head outputs -> proposals.
 *   d_deltas (B,A,4) raw head output, d_scores (B,A) objectness, d_anchors (A,4);
 *   boxes are decoded lazily inside the NMS kernel (never materialised in HBM).
 * ---------------------------------------------------------------------------------- */
int rpn_decode_nms(const float *d_anchors, const float *d_deltas, const float *variances,
                   const float *d_scores, int B, int A, int max_total, float iou_threshold,
                   float score_threshold, int clip_boxes, float *d_out_boxes, float *d_out_scores,
                   int32_t *d_out_idx, int32_t *d_out_valid, void *d_workspace, size_t workspace_bytes,
                   void *stream);

/* ------------------------------------------------------------------------------------
 * The proposal layer's filters in front of the NMS (Faster R-CNN's proposal layer: decode and clip, drop boxes smaller than
 * min_size, keep the pre_nms_topN best scored, NMS, keep post_nms_topN).  No reference counterpart.  rpn_decode_nms does the
 * decode, the NMS and the last cut; this entry does the two filters between them, as a MASK over the scores:
 *     rpn_proposal_filter(scores -> masked);  rpn_decode_nms(masked, the same score_threshold and clip_boxes)
 * is the proposal layer.  float32 throughout; image b's outputs depend on image b alone.
 *   d_scores (B,A) objectness; d_deltas (B,A,4) raw head output and d_anchors (A,4), read only with use_min_size (both may be
 *   NULL otherwise: nothing is decoded); variances: HOST pointer to 4 floats, or NULL for no scaling.
 * Anchor i of image b is a CANDIDATE iff
 *   scores[b,i] > score_threshold   (strict; a NaN score is never a candidate: rpn_decode_nms's own rule), and
 *   with use_min_size != 0: box = what rpn_decode returns for the anchor, bit for bit (get_bboxes_from_deltas on
 *   deltas * variances), each coordinate clipped to [0, 1] (v < 0 ? 0 : v > 1 ? 1 : v) iff clip_boxes != 0;
 *     (box.y2 - box.y1) >= min_h && (box.x2 - box.x1) >= min_w,   each difference one float32 subtraction.
 *   A NaN side fails the test (a NaN or infinite delta, for instance).  A side exactly equal to the minimum passes.
 * Candidates are ranked by score descending as floats compare (-0.0 ties with +0.0, +inf is first), ties to the lower index:
 * the NMS's own order.  With pre_nms_topn > 0 the first pre_nms_topn candidates of that order are KEPT, exactly that many
 * when there are more (a tie across the cut is split by index, never rounded up to a bin); with pre_nms_topn <= 0 every
 * candidate is kept.
 * Outputs: d_masked_scores (B,A) = scores[b,i], bit for bit, where kept and -inf elsewhere (-inf is never > score_threshold);
 *   it must not overlap d_scores.  d_kept (B,) int32 = the number of kept anchors, or NULL.
 * One launch of one workgroup per image on `stream`; no host synchronisation, no floating-point atomics: the same bits on every
 * run.  d_workspace: rpn_proposal_filter_workspace_bytes(B, A) bytes (currently 0: the output row is the passes' staging buffer;
 * may be NULL then).  RPN_ERR_INVALID before any device use for negative sizes, A > 2^30, a NULL pointer that is needed,
 * overlapping score buffers, and with use_min_size a min_h or min_w that is negative or NaN.
 * ---------------------------------------------------------------------------------- */
size_t rpn_proposal_filter_workspace_bytes(int B, int A);
int rpn_proposal_filter(const float *d_anchors, const float *d_deltas, const float *variances, const float *d_scores, int B, int A,
                        int pre_nms_topn, int use_min_size, float min_h, float min_w, float score_threshold, int clip_boxes,
                        float *d_masked_scores, int32_t *d_kept, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * calculate_rpn_actual_outputs(anchors, gt_boxes, gt_labels, hyper_params)   utils/train_utils.py:84-144
 *   (+ randomly_select_xyz_mask :50-65) -- the consumer of generate_iou_map; the (B,A,G) map is never written.
 *   d_gt_labels (B,G) int32, -1 = padding.  d_random_pos / d_random_neg (B,A) int32 >= 1 replace the two
 *   tf.random.uniform draws (priority order: larger first, ties lower index).  variances: HOST pointer, 4 floats.
 *   Outputs: d_bbox_deltas (B,A,4) = encoded deltas / variances (zero for non-positive anchors),
 *   d_bbox_labels (B,A) float32 in {1, 0, -1} (caller views it as (B,F,F,K)).
 * ---------------------------------------------------------------------------------- */
size_t rpn_targets_workspace_bytes(int B, int A, int G);
int rpn_rpn_targets(const float *d_anchors, const float *d_gt_boxes, const int32_t *d_gt_labels, int B, int A, int G,
                    int total_pos, int total_neg, const float *variances, const int32_t *d_random_pos,
                    const int32_t *d_random_neg, float *d_bbox_deltas, float *d_bbox_labels, void *d_workspace,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * preprocessing(image_data, final_height, final_width)            utils/data_utils.py:25-28
 *   one image: uint8 (H,W,3) -> float32 (out_h,out_w,3) in [0,1]: tf.image.convert_image_dtype (x * 1/255),
 *   tf.image.resize (bilinear, half-pixel centres, no antialias), optional tf.image.flip_left_right
 *   (flip_horizontally, utils/data_utils.py:63).  d_out may point into a (B,out_h,out_w,3) batch.
 * ---------------------------------------------------------------------------------- */
int rpn_preprocess_image(const unsigned char *d_img_u8, int H, int W, int out_h, int out_w, int flip,
                         float *d_out, void *stream);

/* ------------------------------------------------------------------------------------
 * get_model(hyper_params) -> rpn_model            models/rpn_vgg16.py:6-22,
 *                                                 models/rpn_mobilenet_v2.py:6-22
 * rpn_model.predict_on_batch(imgs) -> [reg, cls]  predictor.py:50
 *   The handle owns the packed device weights and the activation workspace.
 *   Weights are addressed by the Keras layer names the reference's
 *   load_weights(by_name=True) uses (predictor.py:44): "block1_conv1" ... "rpn_conv",
 *   "rpn_cls", "rpn_reg"; MobileNetV2: "Conv1", "bn_Conv1", "block_3_depthwise_BN", ...
 * ---------------------------------------------------------------------------------- */
typedef struct rpn_model rpn_model;

int rpn_model_create(int backbone, int img_size, int anchor_count, int precision, int max_batch,
                     rpn_model **out);
void rpn_model_destroy(rpn_model *m);
/* feature-map side F (31 for vgg16@500, 32 for mobilenet_v2@500) and head widths */
int rpn_model_feature_map_shape(const rpn_model *m);
/* number of weight-carrying layers, and the i-th layer's name / kernel shape (R,S,Cin,Cout) /
 * kind: 0 conv+bias, 1 conv (no bias) followed by BatchNorm, 2 depthwise conv followed by BatchNorm */
int rpn_model_num_layers(const rpn_model *m);
int rpn_model_layer_info(const rpn_model *m, int i, char *name, int name_len, int shape[4], int *kind);
/* Keras name of the BatchNormalization layer that follows layer i ("" when there is none) */
int rpn_model_layer_bn_name(const rpn_model *m, int i, char *name, int name_len);
/* device memory the handle needs (packed weights; activation arena for max_batch images) */
int rpn_model_memory_bytes(const rpn_model *m, size_t *weights, size_t *arena);
/* keep every intermediate activation alive (unique arena offsets) so that rpn_model_get_activation can
 * read any layer after a forward pass; must be called before the first set_layer / forward */
int rpn_model_keep_activations(rpn_model *m, int keep);
/* HOST pointers: kernel HWIO float32 (depthwise: (R,S,C,1)); bias (Cout) or NULL;
 * bn = {gamma, beta, moving_mean, moving_variance} each (Cout) or NULL (folded on the host, eps 1e-3) */
int rpn_model_set_layer(rpn_model *m, const char *name, const float *kernel, const float *bias,
                        const float *bn_gamma, const float *bn_beta, const float *bn_mean,
                        const float *bn_var);
/* d_imgs (B,img,img,3) NHWC float32 in [0,1] (utils/data_utils.py:25-26);
 * d_reg (B,F,F,4K), d_cls (B,F,F,K) -- the reference's output order is [reg, cls]
 * (models/rpn_vgg16.py:21).
 * A handle owns ONE activation arena and one set of inter-workgroup scratch (K-split partials and tickets): the forwards
 * of a handle must be ordered on one stream (or by events); for concurrent forwards on several streams create one handle
 * per stream (the reference's Keras model is not re-entrant either).
 * Batch invariance: an image's outputs are bit-identical at every batch size B <= max_batch OF ONE HANDLE (split factors follow
 * the grid, summation trees are fixed).  Two handles created with different max_batch may choose different weight packings
 * (MobileNetV2 under F16X3: block 3's chunk size follows the grid at max_batch) and then agree within the float bound, not
 * bit for bit. */
int rpn_model_forward(rpn_model *m, const float *d_imgs, int B, float *d_reg, float *d_cls, void *stream);
/* Sticky status flags of the forwards run so far (no reference counterpart: TF computes in float32 throughout).
 * RPN_STATUS_F16_RANGE: under RPN_PRECISION_F16X3 some activation did not fit float16 (|x| > 65504 or non-finite) when
 * it was written in split form -- outputs of that forward are invalid (use BF16X3 or F32 for such weights).  The flag
 * is raised on the device by the kernel that hits it; a forward never reads it back (no host synchronisation on the
 * hot path).  This call copies the word to the host (synchronising on `stream`) and clears it when `reset` != 0. */
#define RPN_STATUS_F16_RANGE 1u
int rpn_model_status(rpn_model *m, unsigned *flags, int reset, void *stream);
/* debug / test hook: copy the activation of layer `name` (NHWC float32) into d_out */
int rpn_model_get_activation(rpn_model *m, const char *name, float *d_out, size_t out_bytes, int shape[4],
                             void *stream);
/* debug / test hook: which form of the head (rpn_reg | rpn_cls) a forward of B images on this handle runs.  Host arithmetic
 * only, nothing is launched; the forward takes its choice from the same functions.
 *   info[0]  RPN_HEAD_ROUTE_SPLITK (rpn_head_splitk<NB>) or RPN_HEAD_ROUTE_F32 (the float32 implicit GEMM: 5K > 96 or RPN_HEAD_SPLITK=0)
 *   info[1]  NB = ceil(5K / 16), the kernel's 16-column blocks               (0 on the float32 route)
 *   info[2]  pixels per workgroup: 32, 16, or 4 (at most 1024 pixels in slabs) (0 on the float32 route)
 *   info[3]  partial-sum slabs of rpn_conv that the head adds: 1, 2 or 4     (1 on the float32 route)
 * RPN_ERR_INVALID for B outside [1, max_batch]. */
#define RPN_HEAD_ROUTE_SPLITK 0
#define RPN_HEAD_ROUTE_F32 1
int rpn_model_head_launch_info(const rpn_model *m, int B, int info[4]);
/* debug / test hook: run the ops of the handle's own graph up to the one that writes tensor `name` -- at the handle's precision, on
 * its production (fused) graph, no rpn_model_keep_activations needed -- and copy that tensor's first B images into d_out as NHWC
 * float32 (rpn_model_get_activation(m, name, NULL, 0, shape, NULL) gives H, W, C).  A fused MobileNetV2 block's tensor carries the name
 * of its projection, "block_<k>_project"; the stem block (Conv1 + expanded_conv) writes "expanded_conv_project".  Only the layers of
 * those ops need weights.  RPN_ERR_INVALID for B outside [1, max_batch], for a name no op of this graph writes, and for a tensor the
 * graph never holds as such (a conv whose 2 x 2 max-pool runs in its epilogue; rpn_conv where the head adds its split-K slabs). */
int rpn_model_forward_to(rpn_model *m, const char *name, const float *d_imgs, int B, float *d_out, void *stream);
/* debug / test hook: which form of the fused MobileNetV2 block that writes tensor `name` a forward of B images on this handle
 * runs.  Host arithmetic only, nothing is launched; the launchers take their choice from the same functions.
 *   info[0]  RPN_IR_ROUTE_*: the kernel family.  F16X3 decides per HANDLE (grid at max_batch) between ir_block_x3 and
 *            ir_block_hrx3 for blocks 4 and 5; the float32 precisions decide per CALL between ir_block and ir_block_hr for block 3
 *            (512 tiles at B), two kernels that add the same chunks in the same order
 *   info[1]  expanded channels per chunk (F16X3 block 3: per handle, 48 up to 512 tiles at max_batch, 16 above)
 *   info[2]  K-split factor: workgroups per tile, 1 | 2 | 3 | 4 | 6 (always 1 on the float32 routes); follows the grid at B, every
 *            factor adds the same tree
 *   info[3]  tiles over the B images (4 x 8 output pixels; RPN_IR_ROUTE_STEM: 8 x 16)
 * RPN_ERR_INVALID for B outside [1, max_batch], for a name no op writes, and for an op that is not a fused block. */
#define RPN_IR_ROUTE_IR_BLOCK 0
#define RPN_IR_ROUTE_IR_BLOCK_HR 1
#define RPN_IR_ROUTE_IR_BLOCK_X3 2
#define RPN_IR_ROUTE_IR_BLOCK_HRX3 3
#define RPN_IR_ROUTE_STEM 4
int rpn_model_ir_launch_info(const rpn_model *m, const char *name, int B, int info[4]);
/* debug / test hook: which form of the split-precision (BF16X3 / F16X3) op that writes tensor `name` a forward of B images on this
 * handle runs.  Host arithmetic only, nothing is launched, no device is needed; the launchers take their choice from the same
 * functions.  A pooled tensor ("block2_pool") whose 2 x 2 max-pool runs in a conv's epilogue is written by that conv.
 *   info[0]  RPN_CONV_ROUTE_*: the kernel family.  The route is the HANDLE's; between the two conv3x3_split16 families and their
 *            tile widths the launcher decides per CALL, from the grid at B
 *   info[1]  channels per tile: 64 or 128 (the first layer: its Cout; RPN_CONV_ROUTE_MAXPOOL_SPLIT: 0)
 *   info[2]  1 when the 2 x 2 max-pool runs in this kernel's epilogue, else 0
 *   info[3]  K form: 0 one accumulation chain; 1 the K tree inside one workgroup (rpn_conv in front of the slab-adding head);
 *            2 | 4 the K tree split over that many workgroups per tile (the head adds the slabs)
 * RPN_ERR_INVALID for B outside [1, max_batch], for a name no op writes, and for an op that is not on a split route (a float32
 * kernel, the head). */
#define RPN_CONV_ROUTE_VGG_BLOCK1 0    /* block1_conv1 + block1_conv2 + block1_pool in one launch (F16X3) */
#define RPN_CONV_ROUTE_FIRST_LAYER 1   /* the Cin = 3 kernels writing SPLIT16 (BF16X3: float32 arithmetic; F16X3: the 16-bit MFMA) */
#define RPN_CONV_ROUTE_SPLIT 2         /* conv3x3_split, 32x32x16 MFMA */
#define RPN_CONV_ROUTE_SPLIT16_REG 3   /* conv3x3_split16, 16x16x32 MFMA, register-staged */
#define RPN_CONV_ROUTE_SPLIT16_DMA 4   /* conv3x3_split16, persistent LDS-DMA form */
#define RPN_CONV_ROUTE_MAXPOOL_SPLIT 5 /* the un-fused 2 x 2 max-pool on SPLIT16 */
int rpn_model_conv_launch_info(const rpn_model *m, const char *name, int B, int info[4]);
/* algorithmic FLOPs (2*MACs) of one image through the conv stack */
double rpn_model_flops_per_image(const rpn_model *m);
/* per-op timing with HIP events recorded on the caller's stream around every launch of a forward:
 * keep the events of the last n_forwards forwards (0 = off), run forwards, then read the mean elapsed
 * milliseconds of each op over the kept forwards.
 * rpn_model_op_info names op i, the kernel that runs it and its algorithmic FLOPs / HBM bytes per image.  The kernel name is the
 * one a forward of max_batch images runs: a conv3x3_split16 layer picks its form (register-staged or LDS-DMA, 64 or 128 channels
 * wide) from the grid of each CALL, so a smaller batch may run another one -- rpn_model_conv_launch_info(m, name, B, ..) says which.
 * Every form gives the same bits (the batch invariance of rpn_model_forward). */
int rpn_model_set_profiling(rpn_model *m, int n_forwards);
/* time only the ops with mask[i] != 0 (n = rpn_model_num_ops; NULL: every op); untimed ops read back as 0 ms */
int rpn_model_set_profiling_mask(rpn_model *m, const unsigned char *mask, int n);
/* with a mask: time ONE marked op per forward, round robin (2 events per forward); rpn_model_get_profile then averages
   each op over the forwards in which it was the one timed */
int rpn_model_set_profiling_rotate(rpn_model *m, int on);
/* arithmetic of op i's matrix work: an rpn_precision value (RPN_PRECISION_F32 for the float32-MFMA / vector-ALU kernels,
 * the model's split precision for the kernels that form each product from three 16-bit MFMAs); -1 for a bad index.
 * A 2x2 max-pool that runs inside the previous conv's epilogue is reported by rpn_model_op_info with the kernel name
 * "fused:maxpool_split" and zero bytes: it is not a launch. */
int rpn_model_op_arith(const rpn_model *m, int i);
int rpn_model_num_ops(const rpn_model *m);
int rpn_model_op_info(const rpn_model *m, int i, char *name, int name_len, char *kernel, int kernel_len,
                      double *flops_per_image, double *bytes_per_image);
int rpn_model_get_profile(rpn_model *m, float *ms, int n, int *n_forwards);

/* ------------------------------------------------------------------------------------
 * Training of the RPN head on a FROZEN backbone                   trainer.py:54-69
 *   The reference fine-tunes the whole Keras model (its base model is trainable); rpn_head_trainer_create trains rpn_conv,
 *   rpn_reg and rpn_cls only (rpn_model_trainer_create below adds backbone layers).  The loss and Adam forms are TF 2.0.0's,
 *   restated from its sources as recalled (tf_rpn_amd/csrc/train_kernels.hip, with the kernels; the trainer that runs them is
 *   tf_rpn_amd/csrc/trainer.hip).  Every reduction has a fixed order and
 *   there are no floating-point atomics: a call is bit-identical from run to run.
 *
 * reg_loss(y_true, y_pred) + cls_loss(y_true, y_pred)      utils/train_utils.py:164-185, :146-162
 *   d_reg_true (B,A,4) bbox_deltas, d_reg_pred (B,F,F,4K) = (B,A,4); d_cls_true (B,A) labels in {1, 0, -1},
 *   d_cls_pred (B,A) probabilities.  d_losses <- [reg_loss, cls_loss]:
 *     reg: Huber (delta 1) per element, summed over the 4 coordinates, over the anchors whose true deltas are not all
 *          zero, / max(1, n_pos);
 *     cls: keras BinaryCrossentropy on probabilities (clip to [1e-7, 1 - 1e-7], log(. + 1e-7)) averaged over every
 *          entry of the batch with label != -1; NaN when there is none (its gradient is then zero).
 *   d_grad_reg (B,A,4) / d_grad_cls (B,A) (each may be NULL): the gradients of the two losses with respect to d_reg_pred
 *   and d_cls_pred (d/dp; zero where the clip is active).  d_ws: rpn_rpn_losses_workspace_bytes(B, A) bytes.
 * ---------------------------------------------------------------------------------- */
size_t rpn_rpn_losses_workspace_bytes(int B, int A);
int rpn_rpn_losses(const float *d_reg_true, const float *d_reg_pred, const float *d_cls_true, const float *d_cls_pred,
                   int B, int A, float *d_losses, float *d_grad_reg, float *d_grad_cls, void *d_ws, size_t ws_bytes,
                   void *stream);
/* weight gradient of a 3x3 stride-1 'same' conv (the backward of rpn_conv's Conv2D, models/rpn_vgg16.py:18), single-layer entry
 * like rpn_conv2d: d_x (B,H,W,Cin), d_dy (B,H,W,Cout) -> d_dw (3,3,Cin,Cout) HWIO with
 * dw[r][s][ci][co] = sum_{b,y,x} x[b][y+r-1][x+s-1][ci] dy[b][y][x][co] (zero padding), d_db (Cout) = sum of dy, or NULL.
 * Exact float32 products on the float32 MFMA, float32 sums over four fixed ranges of pixels added as (l0 + l1) + (l2 + l3).
 * Cin, Cout multiples of 4.  d_ws: rpn_conv3x3_wgrad_workspace_bytes(...) bytes. */
size_t rpn_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int rpn_conv3x3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw,
                      float *d_db, void *d_ws, size_t ws_bytes, void *stream);
/* rpn_model.compile(optimizer=Adam, loss=[reg_loss, cls_loss]) + train_on_batch / test_on_batch      trainer.py:54-56, :64-69
 *   The trainer holds float32 master weights of the three head layers, Adam's m and v (zero at creation) and the step
 *   count t (applied steps only); sizes come from the model handle (Cin 512 / 576, F, K, max_batch).  It borrows the
 *   handle: the backbone runs on the handle's ops at the handle's precision, so the handle must outlive the trainer and
 *   its activation arena is overwritten by a step.  The head runs in exact float32 from the master weights whatever the
 *   handle's precision; the handle's own head weights are NOT changed by a step (copy them with get_layer + set_layer).
 *   set_layer / get_layer: HOST arrays, kernel HWIO + bias, names "rpn_conv" | "rpn_reg" | "rpn_cls" (any other name is
 *   RPN_ERR_INVALID: the backbone is frozen); get_layer synchronises `stream`.  bias is NULL for the bias-less MobileNetV2 convs of
 *   a trainer made by rpn_model_trainer_create, and only for them.
 *   step: d_imgs (B,img,img,3), d_bbox_deltas (B,A,4), d_bbox_labels (B,F,F,K); d_losses <- [reg + cls, reg, cls] computed
 *   with the weights before the update (Keras train_on_batch order).  update = 0: losses only (test_on_batch, t unchanged);
 *   update = 1: backward + one Adam step (t += 1; alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t) on the device, no host
 *   synchronisation).  steps: t.  outputs: the (reg, cls) head outputs of the last step, whose batch was B. */
typedef struct rpn_head_trainer rpn_head_trainer;
int rpn_head_trainer_create(rpn_model *m, rpn_head_trainer **out);
void rpn_head_trainer_destroy(rpn_head_trainer *t);
int rpn_head_trainer_set_layer(rpn_head_trainer *t, const char *name, const float *kernel, const float *bias);
int rpn_head_trainer_get_layer(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream);
/* the gradient of the total loss with respect to a head layer at the last update step (HOST kernel HWIO + bias) */
int rpn_head_trainer_get_gradient(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream);
int rpn_head_trainer_step(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                          const float *d_bbox_labels, int update, float lr, float beta_1, float beta_2, float epsilon,
                          float *d_losses, void *stream);
long long rpn_head_trainer_steps(const rpn_head_trainer *t);
int rpn_head_trainer_outputs(rpn_head_trainer *t, float *d_reg, float *d_cls, int B, void *stream);
/* A step in two halves, for a caller that trains a second stage on the feature tap (joint Faster R-CNN training: the backbone gets the
 * RPN's gradient plus the second stage's).  rpn_head_trainer_step(update) IS rpn_head_trainer_forward(train = update) followed, when
 * update = 1, by rpn_head_trainer_backward(d_feature_grad = NULL): the same launches in the same order on the same buffers, the same
 * bits.
 *   forward: the forward pass and the losses, d_losses <- [reg + cls, reg, cls]; train = 1 also keeps the loss gradients and, on
 *     MobileNetV2, runs BatchNorm with the batch statistics and updates the moving statistics HERE (as the first half of an update step
 *     does); train = 0 is an evaluation (moving statistics, nothing kept).  train = 1 leaves the forward PENDING on the trainer; train = 0
 *     leaves nothing pending.  A new forward replaces a pending one (on MobileNetV2 the moving statistics have then been updated twice);
 *     set_layer / set_bn drop it.  rpn_head_trainer_outputs works after either kind of forward.
 *   feature: the float32 feature tap (B,F,F,Cin) of the last forward of either kind -- block5_conv3 after its ReLU / block_13_expand
 *     after its ReLU6 -- copied to d_out.  On a trainer with a trained backbone span this is the trainer's own exact-float32 tensor from
 *     the master weights (BatchNorm in batch-statistics mode after train = 1), not the inference handle's; on a frozen-backbone trainer
 *     it is the handle's features as the head trainer reads them.
 *   backward: the second half -- head backward, backbone backward, ONE Adam launch (t += 1 here, and only here).  d_feature_grad
 *     (B,F,F,Cin) or NULL: dL2/dfeat of a loss the caller computed from `feature`'s tensor; it is read in place (no copy, no extra
 *     pass, no atomics) by the epilogue of the first 3x3 dgrad, where it is added to the RPN's gradient at the tap BEFORE the tap's
 *     activation mask: VGG16 (dgrad + g2) [feat > 0]; MobileNetV2: the BatchNorm backward that follows masks the sum with ReLU6's
 *     [0 < y < 6].  The gradients of rpn_conv, rpn_reg and rpn_cls do not depend on it.  It must stay valid until the stream has run
 *     the call.  Requires a pending forward (train = 1) on this trainer with the same d_imgs pointer and the same B, else
 *     RPN_ERR_INVALID; the pending forward is consumed.  On a frozen-backbone trainer (rpn_head_trainer_create, train_from = NULL) a
 *     non-NULL d_feature_grad is RPN_ERR_INVALID -- nothing below the tap trains -- rather than being dropped. */
int rpn_head_trainer_forward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                             const float *d_bbox_labels, int train, float *d_losses, void *stream);
int rpn_head_trainer_feature(rpn_head_trainer *t, float *d_out, int B, void *stream);
int rpn_head_trainer_backward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_feature_grad,
                              float lr, float beta_1, float beta_2, float epsilon, void *stream);
/* the same trainer with the VGG16 backbone trained from `train_from` ("block1_conv1" .. "block5_conv3") upward: the reference's
 * trainable Keras base model (models/rpn_vgg16.py:16-21) when train_from = "block1_conv1".  NULL: rpn_head_trainer_create.
 * set_layer takes every VGG16 conv as well (all 13 must be set before a step): convs below train_from are frozen constants, outside
 * Adam's buffer (get_layer returns them, get_gradient fails).  A step runs the whole VGG16 forward in exact float32 from the
 * trainer's own weights (not the handle's ops), then the backward down to train_from; Adam updates head and trained convs in one
 * launch.  Device memory (at the first step) is sized by max_batch and the trained span.
 * On a MobileNetV2 handle train_from is "block_7_expand" .. "block_12_expand" (the first layer of an inverted-residual block) or
 * "block_13_expand": that layer and every layer above it -- the stride-1 blocks at the feature map's own resolution -- train with the
 * head; any other name (a VGG16 conv, a layer inside a block, a layer below block_7_expand) is RPN_ERR_INVALID.  The layers below
 * train_from stay frozen and run on the handle's ops at the handle's precision, BatchNorm folded (inference mode).  The trained
 * layers run in exact float32 from the trainer's unfolded parameters: on an update step BatchNorm normalises with the batch mean and
 * the biased batch variance over (B, F, F) (eps 1e-3) and updates the moving statistics in the same step, moving = moving * 0.999 +
 * batch * 0.001, the variance with Bessel's correction N / (N - 1) (TF 2.0's fused BatchNorm as recalled); on an evaluation step
 * (update = 0) it normalises with the moving statistics and changes nothing.  Per trained conv Adam updates the kernel, gamma and
 * beta (same flat buffer, one launch); the moving statistics are state.  These convs have no bias: set_layer / get_layer /
 * get_gradient take bias = NULL for them, and the three calls below carry the BatchNorm of a trained conv, named by the conv or by
 * its BatchNorm layer ("<conv>_BN"): HOST arrays of Cout floats; every trained conv and BatchNorm must be set before a step. */
int rpn_model_trainer_create(rpn_model *m, const char *train_from, rpn_head_trainer **out);
/* the trainer that trains EVERY layer of the model, as the reference's trainer.py does (its Keras base model is trainable).  VGG16:
 * rpn_model_trainer_create(m, "block1_conv1", out).  MobileNetV2: all 40 convs -- Conv1 (BatchNorm "bn_Conv1"), expanded_conv_depthwise,
 * expanded_conv_project, block_1_expand .. block_12_project, block_13_expand -- each with its BatchNorm, and the head; there is no frozen
 * prefix (the span's input is the image batch), every layer runs at its own resolution in exact float32 as described above, and
 * set_layer / set_bn / get_* take all 40 names.  rpn_model_trainer_create keeps refusing names below block_7_expand. */
int rpn_model_trainer_create_full(rpn_model *m, rpn_head_trainer **out);
int rpn_head_trainer_set_bn(rpn_head_trainer *t, const char *name, const float *gamma, const float *beta, const float *mean,
                            const float *var);
int rpn_head_trainer_get_bn(rpn_head_trainer *t, const char *name, float *gamma, float *beta, float *mean, float *var, void *stream);
/* the gradients of gamma and beta at the last update step */
int rpn_head_trainer_get_bn_gradient(rpn_head_trainer *t, const char *name, float *dgamma, float *dbeta, void *stream);

/* backward of MobileNetV2's stride-1 blocks, single-layer entries (float32; float64 partial sums inside the BatchNorm reductions; no
 * floating-point atomics, every reduction a fixed tree chosen from the shape alone: bit-identical from run to run).  P = B H W pixels
 * of an NHWC tensor; channel counts are multiples of 4, and every device pointer (the workspace included) is 16-byte aligned: the
 * kernels move four channels at a time (RPN_ERR_INVALID otherwise).
 * rpn_batchnorm_train_forward: d_x (P,C) -> d_mean, d_var (C): the batch mean and biased variance; d_y (P,C) = gamma (x - mean) /
 *   sqrt(var + eps) + beta, then min(max(., 0), 6) when relu6 = 1; d_moving_mean / d_moving_var (both or neither) are updated as
 *   moving * momentum + batch * (1 - momentum), the variance with Bessel's correction.  d_ws: rpn_batchnorm_workspace_bytes(P, C).
 * rpn_batchnorm_train_backward: with dy' = d_dy [0 < y < 6] when relu6 = 1 (TF's Relu6Grad; y recomputed from d_x), else d_dy:
 *   d_dbeta = sum dy', d_dgamma = sum dy' xhat, d_dx = gamma / sqrt(var + eps) (dy' - dbeta / P - xhat dgamma / P).  d_mean / d_var:
 *   what the forward returned.  d_dx may be d_dy.  Same workspace.
 * rpn_conv1x1_wgrad: d_x (P,Cin), d_dy (P,Cout) -> d_dw (Cin,Cout) = x^T dy on the float32 MFMA, the pixels in a power-of-two number of
 *   fixed ranges summed in a fixed tree.  d_ws: rpn_conv1x1_wgrad_workspace_bytes(...) bytes (0: none needed, d_ws may be NULL).
 * rpn_conv1x1_dgrad: d_dx (P,Cin) = d_dy (P,Cout) d_w^T (d_w (Cin,Cout)) on the float32 MFMA, + d_add (P,Cin) when non-NULL (the
 *   gradient that reaches a residual block's input beside its expand conv).
 * rpn_dwconv3x3_dgrad / _wgrad: depthwise 3x3 stride-1 'same', d_w (3,3,C): dx[b][y][x][c] = sum_{r,s} dy[b][y+1-r][x+1-s][c]
 *   w[r][s][c]; dw[r][s][c] = sum_{b,y,x} x[b][y+r-1][x+s-1][c] dy[b][y][x][c].  d_ws: rpn_dwconv3x3_wgrad_workspace_bytes(...). */
size_t rpn_batchnorm_workspace_bytes(long long P, int C);
int rpn_batchnorm_train_forward(const float *d_x, long long P, int C, const float *d_gamma, const float *d_beta, int relu6, float eps,
                                float momentum, float *d_y, float *d_mean, float *d_var, float *d_moving_mean, float *d_moving_var,
                                void *d_ws, size_t ws_bytes, void *stream);
int rpn_batchnorm_train_backward(const float *d_x, const float *d_dy, long long P, int C, const float *d_gamma, const float *d_beta,
                                 const float *d_mean, const float *d_var, int relu6, float eps, float *d_dx, float *d_dgamma,
                                 float *d_dbeta, void *d_ws, size_t ws_bytes, void *stream);
size_t rpn_conv1x1_wgrad_workspace_bytes(long long P, int Cin, int Cout);
int rpn_conv1x1_wgrad(const float *d_x, const float *d_dy, long long P, int Cin, int Cout, float *d_dw, void *d_ws, size_t ws_bytes,
                      void *stream);
int rpn_conv1x1_dgrad(const float *d_dy, const float *d_w, const float *d_add, long long P, int Cin, int Cout, float *d_dx, void *stream);
int rpn_dwconv3x3_dgrad(const float *d_dy, const float *d_w, int B, int H, int W, int C, float *d_dx, void *stream);
size_t rpn_dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C);
int rpn_dwconv3x3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int C, float *d_dw, void *d_ws, size_t ws_bytes,
                        void *stream);

/* backward of MobileNetV2's stride-2 layers, single-layer entries (same conventions: float32, each output written once, no atomics,
 * fixed trees, C % 4 == 0, 16-byte aligned pointers).  The padding is Keras' ZeroPadding2D(correct_pad(3)) followed by a 'valid'
 * stride-2 conv, per spatial dim of n input pixels: before = n % 2 (even side 0, odd side 1), after = 1, out = (n + before + 1 - 3) /
 * 2 + 1; pt / pl are `before` of H / W, OH / OW the two output sides.
 * rpn_dwconv3x3_s2_dgrad: d_dy (B,OH,OW,C), d_w (3,3,C) -> d_dx (B,H,W,C): dx[b][y][x][c] = sum_{r,s} dy[b][(y+pt-r)/2][(x+pl-s)/2][c]
 *   w[r][s][c] over the taps where both quotients are exact and in range; every element is written (zeros where no output reads).
 * rpn_dwconv3x3_s2_wgrad: d_x (B,H,W,C), d_dy (B,OH,OW,C) -> d_dw (3,3,C): dw[r][s][c] = sum_{b,oy,ox} x[b][2oy+r-pt][2ox+s-pl][c]
 *   dy[b][oy][ox][c].  d_ws: rpn_dwconv3x3_s2_wgrad_workspace_bytes(B, H, W, C) (the INPUT's shape).
 * rpn_conv3x3_s2_cin3_wgrad: the stem (Conv1), d_x (B,H,W,3) the image batch, d_dy (B,OH,OW,Cout) -> d_dw (3,3,3,Cout): dw[r][s][ci][co] =
 *   sum_{b,oy,ox} x[b][2oy+r-pt][2ox+s-pl][ci] dy[b][oy][ox][co]; the pixels in up to 256 fixed ranges added in a fixed two-level tree.
 *   d_ws: rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, H, W, Cout).  (The stem needs no data gradient.) */
int rpn_dwconv3x3_s2_dgrad(const float *d_dy, const float *d_w, int B, int H, int W, int C, float *d_dx, void *stream);
size_t rpn_dwconv3x3_s2_wgrad_workspace_bytes(int B, int H, int W, int C);
int rpn_dwconv3x3_s2_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int C, float *d_dw, void *d_ws, size_t ws_bytes,
                           void *stream);
size_t rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(int B, int H, int W, int Cout);
int rpn_conv3x3_s2_cin3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int Cout, float *d_dw, void *d_ws,
                              size_t ws_bytes, void *stream);

/* backward of the VGG16 backbone, single-layer entries (float32; no floating-point atomics: bit-identical from run to run)
 * rpn_conv3x3_dgrad: input gradient of a 3x3 stride-1 'same' conv, d_dx (B,H,W,Cin) = conv_transpose(d_dy (B,H,W,Cout), d_w HWIO),
 *   i.e. dx[b][y][x][ci] = sum_{r,s,co} dy[b][y+1-r][x+1-s][co] w[r][s][ci][co] (zero outside); with d_mask (B,H,W,Cin) non-NULL
 *   only the entries where mask > 0 are kept (the ReLU of the layer's input), the others are 0.  Cin % 4 == 0, Cout % 16 == 0.
 *   d_ws: rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout) bytes.
 * rpn_conv3x3_dgrad_add: the same with an addend d_add (B,H,W,Cin), non-NULL and 4-byte aligned, in the epilogue: d_dx = mask > 0 ?
 *   fl32(dgrad + add) : 0 (without mask: fl32(dgrad + add)) -- the gradient that reaches the same tensor by another path, added before
 *   the mask, in the same pass, each output written once.  Same validation, workspace and tile choice (rpn_conv3x3_dgrad_tile_n).
 *   d_add == d_dx is allowed: each element is read and then written by the same lane.
 * rpn_maxpool2x2_backward: MaxPooling2D(2, 2) 'valid' backward fused with the ReLU mask of the pooled tensor: d_y (B,H,W,C) the
 *   pool's input, d_dpool (B,H/2,W/2,C) -> d_dy_out (B,H,W,C): each window's gradient at its first maximum (row-major, replaced only
 *   by a strictly greater value) when that maximum is > 0; every other entry, the rows / columns no window covers included, is 0.
 *   C % 4 == 0, H, W >= 2.
 * rpn_conv3x3_wgrad_wide: weight and bias gradient at backbone shapes, as rpn_conv3x3_wgrad computes them but with Cin = 3 accepted
 *   and d_db required: the pixels are split into a power-of-two number of fixed ranges chosen from (B, H, W, Cin, Cout) alone,
 *   summed in a fixed pairwise tree; db is one more row of the same GEMM.  Cin 3 or a multiple of 4, Cout % 4 == 0.
 *   d_ws: rpn_conv3x3_wgrad_wide_workspace_bytes(...) bytes. */
size_t rpn_conv3x3_dgrad_workspace_bytes(int Cin, int Cout);
/* the input-channel width (128 | 64) of the workgroup tile rpn_conv3x3_dgrad runs on for a shape, chosen from the shape alone (the
 * bits are the same either way); 0 for a bad shape.  Host only. */
int rpn_conv3x3_dgrad_tile_n(int B, int H, int W, int Cin);
int rpn_conv3x3_dgrad(const float *d_dy, const float *d_w, const float *d_mask, int B, int H, int W, int Cin, int Cout, float *d_dx,
                      void *d_ws, size_t ws_bytes, void *stream);
int rpn_conv3x3_dgrad_add(const float *d_dy, const float *d_w, const float *d_mask, const float *d_add, int B, int H, int W, int Cin,
                          int Cout, float *d_dx, void *d_ws, size_t ws_bytes, void *stream);
int rpn_maxpool2x2_backward(const float *d_y, const float *d_dpool, int B, int H, int W, int C, float *d_dy_out, void *stream);
size_t rpn_conv3x3_wgrad_wide_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int rpn_conv3x3_wgrad_wide(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw, float *d_db,
                           void *d_ws, size_t ws_bytes, void *stream);

/* Training the backbone's backward in split float16 (rpn_head_trainer_set_backward_precision on a VGG16 trainer).  The trainer's
 * forward stays exact float32, so the kept activations, the ReLU masks, the pool maxima and the losses are bit for bit those of the
 * float32 step; the head's three layers (rpn_conv's weight gradient included), block1_conv1's weight gradient (Cin = 3: 37 GEMM rows),
 * the max-pool backward and Adam stay float32 as well.  Every other 3x3 product of the backbone's backward -- each input gradient,
 * the first one from rpn_conv's dS with its feature_grad addend included, and each weight + bias gradient -- runs on
 * v_mfma_f32_16x16x32_f16 under the contract of "Training the head in split float16" below, applied to the implicit GEMMs:
 *   Operands: an activation x enters as hi = f16(x), lo = f16(x - hi), round-to-nearest-even, unscaled; |x| > 65504 or a non-finite
 *     value raises RPN_STATUS_F16_RANGE.  A gradient tensor dY enters as the split of dY * 2^t, ONE t per gradient tensor, t = 12 - e
 *     with max|dY| = m 2^e, m in [0.5, 1), clamped to [-116, 100], NaNs skipped, 0 for an all-zero tensor; the SAME t serves the weight
 *     gradient and the input gradient that read the same dY.  A kernel w enters as the split of w * 2^s, one s per layer over its
 *     whole HWIO kernel (the forward rule of the head: 12 - e clamped to [-100, 24]).  Both maxima are found on the device (an integer
 *     atomicMax on the bits), with no host round trip and no synchronisation.  Each product is lo*hi, hi*lo, hi*hi in that order per
 *     step of 32 of the reduction, float32 accumulation inside the MFMA; lo*lo is dropped.  A non-finite gradient raises the flag, a
 *     finite one of any magnitude does not.
 *   dx (P x Cin) = 2^-(t + s) (im2col'(2^t dY) (P x 9 Cout)) (2^s W'), W'[r][s][co][ci] = W[2-r][2-s][ci][co], packed once per layer per
 *     step into a hi / lo image.  The reduction runs over k = (3 r + s) Cout + co in steps of 32 from 0 (the tail of 9 Cout as zeros):
 *     its order follows from the shape alone, is the same at both tile widths (128 x 128 | 128 x 64, chosen from the shape alone:
 *     rpn_conv3x3_dgrad_x3_tile_n), and a pixel's result reads no other pixel's tile -- the same bits at B = 1 and inside a batch
 *     whenever t is the same.  Epilogue: dx = mask > 0 ? fl32(acc * 2^a * 2^b + add) : 0, a + b = -(t + s) in halves of the same sign
 *     (two exact factors, as the head's d_in); add and mask are optional, add == dx is allowed, every element is written once.
 *   dW (9 Cin x Cout) = 2^-t (im2col(X)^T (2^t dY)), the reduction over the pixels: the leaves of rpn_conv3x3_wgrad_wide (fixed
 *     ranges of pixels chosen from the shape alone), each walked in steps of 32 pixels from its start with its tail as zeros and
 *     multiplied by 2^-t, then added in the float32 path's fixed pairwise tree.  db is one more row of the same GEMM, a row of ones
 *     (hi = 1, lo = 0): db = 2^-t sum (hi + lo)(2^t dY) in the same leaves and tree.
 *   No floating-point atomics: bit-identical from run to run.
 *   rpn_head_trainer_set_backward_precision: RPN_PRECISION_F32 (the default: exactly the float32 launches, bit for bit) or
 *     RPN_PRECISION_F16X3; BF16X3 and F32W are RPN_ERR_UNSUPPORTED, F16X3 on a head-only or a MobileNetV2 trainer is
 *     RPN_ERR_UNSUPPORTED, any other value RPN_ERR_INVALID.  It needs no device and keeps the weights, Adam's moments and the step
 *     count.  rpn_head_trainer_backward_precision reports it.  A VGG16 trainer allocates the image and the max / scale words with its
 *     other buffers, whatever the precision: rpn_head_trainer_backward_x3_bytes bytes (9.4 MB for VGG16's 512 x 512 layers; 0 for a
 *     trainer without a VGG16 span).
 *   rpn_head_trainer_status: the sticky RPN_STATUS_F16_RANGE of the backward's products (0 before the first step); reset = 1 clears
 *     it; synchronises `stream`.
 *   rpn_conv3x3_dgrad_x3 / rpn_conv3x3_wgrad_wide_x3: the two products on their own, TEST AND TIMING ENTRIES like rpn_conv3x3_dgrad /
 *     rpn_conv3x3_wgrad_wide (same shapes and tensors; d_mask, d_add as rpn_conv3x3_dgrad_add, either may be NULL).  Each call finds t
 *     (and s) itself; neither allocates nor synchronises.  d_ws: *_workspace_bytes(...) bytes, 16-byte aligned -- the packed image or
 *     the leaf slabs, plus 256 bytes of max / scale words.  d_dy, d_x 16-byte aligned; d_w 4-byte aligned (a 16-byte aligned d_w is
 *     read with wider loads: the same bits).  d_status: a device word that receives
 *     RPN_STATUS_F16_RANGE, or NULL.  dgrad: Cin % 4 == 0, Cout % 16 == 0.  wgrad: Cin % 4 == 0 (Cin = 3 is RPN_ERR_UNSUPPORTED:
 *     block1_conv1 stays on rpn_conv3x3_wgrad_wide), Cout % 4 == 0, B H W < 2^31 - 64.
 *   rpn_conv3x3_dgrad_x3_tile_n: A TEST HOOK like rpn_conv3x3_dgrad_tile_n -- the input-channel width (128 | 64) of the tile
 *     rpn_conv3x3_dgrad_x3 runs a shape on, 0 for a bad shape; host only. */
int rpn_head_trainer_set_backward_precision(rpn_head_trainer *t, int precision);
int rpn_head_trainer_backward_precision(const rpn_head_trainer *t);
size_t rpn_head_trainer_backward_x3_bytes(const rpn_head_trainer *t);
int rpn_head_trainer_status(rpn_head_trainer *t, unsigned *flags, int reset, void *stream);
size_t rpn_conv3x3_dgrad_x3_workspace_bytes(int Cin, int Cout);
int rpn_conv3x3_dgrad_x3_tile_n(int B, int H, int W, int Cin);
int rpn_conv3x3_dgrad_x3(const float *d_dy, const float *d_w, const float *d_mask, const float *d_add, int B, int H, int W, int Cin,
                         int Cout, float *d_dx, unsigned *d_status, void *d_ws, size_t ws_bytes, void *stream);
size_t rpn_conv3x3_wgrad_wide_x3_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int rpn_conv3x3_wgrad_wide_x3(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw, float *d_db,
                              unsigned *d_status, void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * single conv layer, for kernel-level parity tests and micro-benchmarks.
 *   x (B,H,W,Cin) NHWC, w HWIO (device), bias (Cout, device, may be NULL).
 *   pad_t / pad_l: zero rows/cols added before the first row/col; OH/OW given by the caller.
 *   act: 0 linear, 1 relu, 2 sigmoid, 3 relu6.
 * ---------------------------------------------------------------------------------- */
int rpn_conv2d(const float *d_x, int B, int H, int W, int Cin, const float *d_w, const float *d_bias,
               int R, int S, int Cout, int stride, int pad_t, int pad_l, int OH, int OW, int act,
               int precision, float *d_out, void *stream);
int rpn_maxpool2x2(const float *d_x, int B, int H, int W, int C, float *d_out, void *stream);
/* depthwise 3x3 (MobileNetV2): d_w (3,3,C), d_bias (C) or NULL, C % 4 == 0 */
int rpn_dwconv3x3(const float *d_x, int B, int H, int W, int C, const float *d_w, const float *d_bias,
                  int stride, int pad_t, int pad_l, int OH, int OW, int act, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------
 * RoI pooling of a feature map under proposals (no reference counterpart: the operator between the RPN and a Faster R-CNN
 * detection head, tf.image.crop_and_resize(feature_map, rois, box_indices, (ph, pw)), bilinear, extrapolation value 0).
 *   d_x (B,H,W,C) NHWC float32, d_rois (B,R,4) normalised [y1,x1,y2,x2], d_out (B,R,ph,pw,C); RoI r of image b samples image b.
 *   d_valid (B,) int32 or NULL: rows r >= valid[b] are written as zeros (what rpn_decode_nms / rpn_combined_nms return).
 *   float32, every operation rounded on its own:
 *     hs = (y2 - y1) * (H - 1) / (ph - 1), in_y(i) = y1 * (H - 1) + i * hs   (ph == 1: in_y = 0.5 * (y1 + y2) * (H - 1)), same in x;
 *     in_y < 0, in_y > H - 1, in_x < 0, in_x > W - 1 or NaN: the sample is 0 in every channel; else t = floor(in_y), b = ceil(in_y),
 *     ly = in_y - t, l = floor(in_x), r = ceil(in_x), lx = in_x - l, top = x[t,l] + (x[t,r] - x[t,l]) * lx, bot likewise on row b,
 *     out = top + (bot - top) * ly.
 *   A box side clipped to exactly 1.0 can round the LAST sample's coordinate just above H - 1 in float32; that sample is then 0
 *   (TensorFlow evaluates the same expression).
 * rpn_roi_pool_backward: d_dx (B,H,W,C) = the adjoint of rpn_roi_pool applied to d_dy (B,R,ph,pw,C): every sample adds dy times its
 *   four corner weights; extrapolated samples and rows beyond valid add nothing.  Writes every element of d_dx.  A gather in
 *   (r, i, j) order without floating-point atomics: bit-identical from run to run, and image b's dx depends on image b alone.
 *   There is no gradient with respect to the boxes.
 * rpn_model_roi_pool: rpn_roi_pool of the feature tap (block5_conv3 / block_13_expand) where the handle's last forward left it --
 *   float32, or the hi / lo 16-bit split form under BF16X3 / F16X3, no float32 copy -- bit-identical to rpn_roi_pool applied to
 *   rpn_model_get_activation of that tap.  Ordered on `stream` like a forward; fails before the first forward and for
 *   B > max_batch.
 * C % 4 == 0; pointers 16-byte aligned; B, R, ph, pw, H, W >= 1.
 * ---------------------------------------------------------------------------------- */
int rpn_roi_pool(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw, const int *d_valid,
                 float *d_out, void *stream);
int rpn_roi_pool_backward(const float *d_dy, const float *d_rois, const int *d_valid, int B, int H, int W, int C, int R, int ph,
                          int pw, float *d_dx, void *stream);
int rpn_model_roi_pool(rpn_model *m, const float *d_rois, int B, int R, int ph, int pw, const int *d_valid, float *d_out,
                       void *stream);

/* ------------------------------------------------------------------------------------
 * RoI Align (no reference counterpart; the pooling operator of Mask R-CNN and of every Faster R-CNN since): every output bin is
 * the average of s x s bilinear samples spread evenly over the bin, in pixel-centre coordinates.  The arithmetic is Detectron2's
 * aligned=True form as this project restates it; torchvision is not a dependency and bit parity with torchvision.ops.roi_align
 * is NOT pinned -- the pinned oracle is the float32 restatement of tests/test_roi_align_host.py.  Beside rpn_roi_pool, which keeps
 * its bits.
 *   d_x (B,H,W,C) NHWC float32, d_rois (B,R,4) normalised [y1,x1,y2,x2], d_out (B,R,ph,pw,C); RoI r of image b samples image b.
 *   s = sampling_ratio, 1..4.  (extent_y, extent_x) = (Sy, Sx): the image's height and width measured in feature pixels, float32,
 *   finite and > 0: (H, W) maps the box [0,1] onto the whole map; a stride-16 backbone on 500 pixels has exactly 500 / 16 = 31.25.
 *   d_valid (B,) int32 or NULL: rows r >= valid[b] are written as zeros.
 *   float32, every operation rounded on its own, in exactly this order (y axis; x likewise with x1, x2, Sx, pw, W):
 *     start = y1 * Sy - 0.5;  end = y2 * Sy - 0.5;  bin = (end - start) / (float)ph;  step = bin / (float)s    (no clamp of the size)
 *     sample k (0 <= k < s) of bin i:  y = (start + (float)i * bin) + ((float)k + 0.5) * step
 *     ok = y >= -1 && y <= (float)H                                     (false for NaN)
 *     if (y < 0) y = 0;  lo = (int)y;  if (lo >= H - 1) { lo = hi = H - 1; y = (float)lo; } else hi = lo + 1;
 *     l = y - (float)lo;  h = 1 - l
 *   sample (ky, kx) = ((hy*hx * x[lo_y,lo_x] + hy*lx * x[lo_y,hi_x]) + ly*hx * x[hi_y,lo_x]) + ly*lx * x[hi_y,hi_x]
 *     (the four weights are rounded products, each term a rounded product, added left to right)
 *   acc = +0;  for ky in 0..s-1, for kx in 0..s-1: if (ok_y(ky) && ok_x(kx)) acc = acc + sample(ky, kx);
 *   out[b,r,i,j,c] = acc / (float)(s * s)                  (a sample that is not ok adds nothing, but still counts in s * s)
 *   Unlike rpn_roi_pool the result is continuous in the box: for a box inside [0, 1] at the default extent every sample lies in
 *   [-0.5, H - 0.5], a whole half pixel away from the ok thresholds -1 and H, so no rounding of a coordinate can switch a sample
 *   off (there is no "last sample rounds past H - 1" case), and a coordinate that rounds across a pixel centre moves weight l ~ 0
 *   from one neighbour to the other.
 * rpn_roi_align_backward: d_dx (B,H,W,C) = the adjoint with respect to the feature map, applied to d_dy (B,R,ph,pw,C).  Writes
 *   every element of d_dx.  A gather without floating-point atomics, bit-identical from run to run; image b's dx depends on image
 *   b's RoIs, valid count and dy alone.  The weights are separable:
 *     Ay(i, py) = +0, then for k in 0..s-1 with ok(k): Ay = Ay + w_k,  w_k = (lo == py ? h : 0) + (hi == py ? l : 0);  Ax(j, px) likewise
 *     acc = +0;  for r < valid[b], i, j in that order, where Ay(i, py) != 0 and Ax(j, px) != 0:
 *         acc[c] = acc[c] + dy[b,r,i,j,c] * (Ay(i, py) * Ax(j, px))
 *     dx[b,py,px,c] = acc[c] / (float)(s * s)
 *   There is no gradient with respect to the boxes.
 * rpn_model_roi_align: rpn_roi_align of the feature tap where the handle's last forward left it -- float32, or the hi / lo 16-bit
 *   split form under BF16X3 / F16X3, no float32 copy -- bit-identical to rpn_roi_align applied to rpn_model_get_activation of that
 *   tap.  Ordered on `stream` like a forward; fails before the first forward and for B > max_batch.
 * C % 4 == 0; pointers 16-byte aligned; B, R, ph, pw, H, W >= 1; RPN_ERR_INVALID for sampling_ratio outside 1..4 and for an extent
 * that is not finite and > 0, before any device use.
 * ---------------------------------------------------------------------------------- */
int rpn_roi_align(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw, int sampling_ratio,
                  float extent_y, float extent_x, const int *d_valid, float *d_out, void *stream);
int rpn_roi_align_backward(const float *d_dy, const float *d_rois, const int *d_valid, int B, int H, int W, int C, int R, int ph,
                           int pw, int sampling_ratio, float extent_y, float extent_x, float *d_dx, void *stream);
int rpn_model_roi_align(rpn_model *m, const float *d_rois, int B, int R, int ph, int pw, int sampling_ratio, float extent_y,
                        float extent_x, const int *d_valid, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------
 * RoI max pooling (no reference counterpart; Fast R-CNN's RoIPool, the pooling of the VGG16 Faster R-CNN recipe): every output bin
 * is the MAXIMUM over a quantised block of feature pixels.  The arithmetic is Caffe's ROIPooling / torchvision.ops.roi_pool on this
 * project's normalised boxes; neither is a dependency and parity with them is NOT pinned -- where they differ from each other or
 * from this text, this text is the contract, and the pinned oracle is its restatement in tests/test_roi_max_host.py.  Beside
 * rpn_roi_pool and rpn_roi_align, which keep their bits.
 *   d_x (B,H,W,C) NHWC float32, d_rois (B,R,4) normalised [y1,x1,y2,x2], d_out (B,R,ph,pw,C) float32, d_argmax (B,R,ph,pw,C) int32
 *   or NULL (then it is not written: inference); RoI r of image b pools image b.  d_valid (B,) int32 or NULL.
 *   (extent_y, extent_x) = (Sy, Sx): the box scale in feature pixels, float32, finite and > 0.  (H - 1, W - 1) makes the box
 *   [0,0,1,1] exactly the pixels 0 .. H - 1, the convention of rpn_roi_pool (and NOT rpn_roi_align's (H, W), which measures
 *   pixel cells, not pixel centres); a stride-16 backbone on 500 pixels has exactly 500 / 16 = 31.25.
 *   float32, every operation rounded on its own, per axis (y shown; x likewise with x1, x2, Sx, pw, W):
 *     a = y1 * Sy;  e = y2 * Sy.  If any of the box's four products is NaN the RoI is DEAD.  Otherwise each product is clamped to
 *     [-2^20, 2^20];  p1 = (int)roundf(a);  p2 = (int)roundf(e)   (half away from zero);  n = max(p2 - p1 + 1, 1)  (a flipped or
 *     zero-size box is one pixel wide);  bin = (float)n / (float)ph
 *     bin i covers the pixel rows [hs, he):  hs = min(max((int)floorf((float)i * bin) + p1, 0), H)
 *                                            he = min(max((int)ceilf((float)(i + 1) * bin) + p1, 0), H)
 *   A bin with he <= hs or we <= ws is EMPTY: its output is +0.0 in every channel and its argmax -1.  A non-empty bin scans its
 *   pixels in (row, column) order: m = the first pixel's value, idx = its y * W + x; a later pixel v replaces them iff
 *   v > m || v != v  (torch.max_pool2d's rule: the first maximum wins a tie, a NaN in the bin reaches the output).
 *   out = m, a bit-exact copy of an input value (the sign of zero kept); argmax = idx.
 *   Rows r >= valid[b] and dead RoIs: every output +0.0, every argmax -1.
 *   So: an all-negative bin gives its negative maximum, not 0; an all -inf bin gives -inf; on a post-ReLU map most ties are
 *   between zeros and the bin's first pixel wins them; bins overlap (he(i) can exceed hs(i + 1)), and when the RoI is smaller than
 *   the grid (n < ph) one pixel lies in several bins of the same RoI.
 * rpn_roi_max_pool_backward: d_dx[b,y,x,c] = the sum of d_dy[b,r,i,j,c] over the (r, i, j) with d_argmax[b,r,i,j,c] == y * W + x,
 *   accumulated in float32 in (r, i, j) order from +0.0, r < valid[b], dead RoIs skipped.  Writes every element of d_dx.  A gather
 *   without floating-point atomics, bit-identical from run to run; image b's dx depends on image b's RoIs, valid count, argmax
 *   and dy alone.  d_argmax must be what the forward wrote for these boxes, extent and valid (the bins a pixel can lie in are
 *   recomputed from the boxes; an argmax entry is only ever compared, never used as an address).  No gradient with respect to
 *   the boxes.
 * rpn_model_roi_max_pool: rpn_roi_max_pool of the feature tap where the handle's last forward left it -- float32, or the hi / lo
 *   16-bit split form under BF16X3 / F16X3, no float32 copy -- bit-identical to rpn_roi_max_pool applied to
 *   rpn_model_get_activation of that tap.  Ordered on `stream` like a forward; fails before the first forward and for B > max_batch.
 * C % 4 == 0; pointers 16-byte aligned; B, R, ph, pw, H, W >= 1; RPN_ERR_INVALID for an extent that is not finite and > 0, before
 * any device use.
 * ---------------------------------------------------------------------------------- */
int rpn_roi_max_pool(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw, float extent_y,
                     float extent_x, const int *d_valid, float *d_out, int32_t *d_argmax /* may be NULL */, void *stream);
int rpn_roi_max_pool_backward(const float *d_dy, const int32_t *d_argmax, const float *d_rois, const int *d_valid, int B, int H, int W,
                              int C, int R, int ph, int pw, float extent_y, float extent_x, float *d_dx, void *stream);
int rpn_model_roi_max_pool(rpn_model *m, const float *d_rois, int B, int R, int ph, int pw, float extent_y, float extent_x,
                           const int *d_valid, float *d_out, int32_t *d_argmax, void *stream);

/* ------------------------------------------------------------------------------------
 * Second stage around RoI pooling: targets, losses, detections (no reference counterpart: the reference stops at the proposals;
 * thresholds and sampling rule are this project's choice).  The counterparts of rpn_rpn_targets / rpn_rpn_losses / rpn_decode_nms.
 * Everything on `stream`, no host synchronisation, no floating-point atomics: bit-identical from run to run.
 *
 * rpn_roi_targets: which proposal trains on which ground-truth box.
 *   d_rois (B,R,4) normalised [y1,x1,y2,x2]; d_valid (B,) int32 or NULL: rows r >= valid[b] are padding (what rpn_decode_nms
 *   returns); d_gt_boxes (B,G,4); d_gt_labels (B,G) int32: a gt row is valid iff its label is >= 1 (0 is background, padding is -1);
 *   variances: HOST pointer, 4 floats; d_random_pos / d_random_neg (B,R) int32 >= 1: the sampling priorities.
 *   float32, every operation rounded on its own, the arithmetic of generate_iou_map / get_deltas_from_bboxes.  Per live row:
 *     best = 0, arg = none; for valid gt g in index order: iou = IoU(roi, gt[g]); if (iou > best) { best = iou; arg = g; }
 *   (strict: the first maximum wins, a NaN never wins, an IoU of 0 never sets arg).
 *   Positive candidates: live rows with best > pos_iou; the total_pos of highest random_pos priority are kept, ties to the lower
 *   index.  Negative candidates: live rows not kept as positives with neg_lo <= best < neg_hi; total_pos + total_neg - n_pos_kept
 *   of them are kept by random_neg the same way (the batch fills up with negatives, as the RPN targets do).
 *   d_roi_labels (B,R) int32: the matched gt's label for a kept positive, 0 for a kept negative, -1 otherwise (padding included).
 *   d_roi_deltas (B,R,4): encode(roi, gt[arg]) / variances for a kept positive, exactly +0.0 everywhere else.
 *   B, R, G >= 1, G <= 2048, 0 <= neg_lo <= neg_hi, pos_iou >= 0; d_workspace: rpn_roi_targets_workspace_bytes(B, R, G) bytes.
 *   One launch, one workgroup per image; the (B,R,G) IoU map is never written.
 *
 * rpn_roi_sample_targets: the proposal-target layer: rpn_roi_targets' assignment over the proposals PLUS the gt boxes, and only the
 * sampled RoIs handed on, as a dense (B,S) batch that the pools, the detection head and rpn_roi_losses take as it is.
 *   d_rois, d_valid, d_gt_boxes, d_gt_labels, variances, the counts and the thresholds: as rpn_roi_targets takes them.  add_gt: 0 or
 *   not 0.  N = add_gt ? R + G : R.  d_random_pos / d_random_neg (B,N) int32 >= 1.  S must equal total_pos + total_neg and be >= 1.
 *   Candidates of image b: candidate i < R is RoI i, live iff i < clamp(valid[b], 0, R); candidate R + g is gt box g, live iff add_gt
 *   and gt_labels[b,g] >= 1.  A candidate that is not live is never selected.
 *   Per live candidate, in float32 with every operation rounded on its own (generate_iou_map):
 *     best = 0, arg = none; for valid gt g in index order: iou = IoU(box, gt[g]); if (iou > best) { best = iou; arg = g; }
 *   (strict: the first maximum wins, a NaN never wins).  A gt candidate meets itself at IoU exactly 1 unless it is degenerate: a
 *   zero-area or NaN box has IoU 0 or NaN with everything, itself included.
 *   Positive candidates: live, best > pos_iou; the total_pos of highest random_pos priority are kept, ties to the lower candidate
 *   index.  Negative candidates: live, not kept as positives, neg_lo <= best < neg_hi; total_pos + total_neg - n_pos of them are kept
 *   by random_neg the same way.  With add_gt == 0 the kept sets are rpn_roi_targets' for the same priorities.
 *   Output rows of image b, in this order: the kept positives in ascending candidate index, the kept negatives in ascending
 *   candidate index, then padding up to S.
 *     d_out_rois (B,S,4): the candidate's box, a bit-exact copy; d_out_labels (B,S) int32: the matched gt's label, 0 for a negative;
 *     d_out_deltas (B,S,4): encode(box, gt[arg]) / variances for a positive, exactly +0.0 for a negative;
 *     d_out_index (B,S) int32: the candidate index (>= R: gt box index - R); d_out_counts (B,2) int32: [n_sampled, n_pos].
 *     Padding rows s >= n_sampled: box and deltas +0.0, label -1, index -1.  Every element of all five is written on every call.
 *   n_sampled is what rpn_roi_pool / rpn_roi_align / rpn_roi_max_pool / rpn_roi_decode_scores take as d_valid.
 *   B, R >= 1, 1 <= G <= 2048, thresholds as above; d_workspace: rpn_roi_sample_targets_workspace_bytes(B, R, G, add_gt) bytes.
 *   One launch, one workgroup per image; the row of a kept candidate comes from an ordered workgroup scan: no atomics on global
 *   memory, no memset, the IoU map is never written.  d_out_rois and d_out_deltas 16-byte aligned.
 *
 * rpn_roi_losses: the detection head's two losses and, optionally, their gradients.
 *   d_cls_logits (B,R,C) LOGITS (not probabilities); d_reg_pred (B,R,4C) class-specific boxes; d_roi_labels (B,R) int32;
 *   d_roi_deltas (B,R,4).  A row whose label is outside [0, C) is ignored by both losses and never indexes memory.
 *     cls_loss = sum over kept rows of (logsumexp(logits) - logits[label]) / max(1, n_kept)
 *     reg_loss = sum over rows with label >= 1 of sum_k huber_1(pred[4 label + k] - delta[k]) / max(1, n_pos),
 *                huber_1(e) = 0.5 q^2 + (|e| - q), q = min(|e|, 1)
 *   d_losses = [reg_loss, cls_loss] (the order of rpn_rpn_losses).  With no kept row / no positive row the loss is 0 and its
 *   gradient all zeros: NO NaN -- on purpose unlike rpn_rpn_losses, whose cls_loss is Keras' mean of an empty tensor.
 *   d_grad_logits (B,R,C) or NULL: (softmax - onehot) / n_kept on kept rows, 0 elsewhere.  d_grad_reg (B,R,4C) or NULL:
 *   clamp(pred - delta, -1, 1) / n_pos on the four entries of the labelled class of positive rows, 0 elsewhere.  Each is the
 *   gradient of its own loss and is written in full.  Sums in float64, per-thread partials then a fixed tree.
 *   d_workspace: rpn_roi_losses_workspace_bytes(B, R, C) bytes.
 *
 * rpn_roi_decode_scores: head outputs -> what rpn_combined_nms takes (q == C).
 *   d_boxes (B,R,C,4): boxes[b,r,c] = decode(rois[b,r], reg_pred[b,r,c] * variances), bit-identical to rpn_decode on the expanded
 *   tensors; not clipped; every row is decoded.  d_scores (B,R,C): softmax(logits[b,r])[c] for c >= 1 on a live row; exactly 0 for
 *   background (c == 0) and for rows r >= valid[b] -- run the NMS with a score threshold above 0.  variances: HOST pointer.
 * d_rois, d_gt_boxes, d_roi_deltas, d_reg_pred, d_grad_reg, d_boxes 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
size_t rpn_roi_targets_workspace_bytes(int B, int R, int G);
int rpn_roi_targets(const float *d_rois, const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels, int B, int R,
                    int G, int total_pos, int total_neg, float pos_iou, float neg_lo, float neg_hi, const float *variances,
                    const int32_t *d_random_pos, const int32_t *d_random_neg, float *d_roi_deltas, int32_t *d_roi_labels,
                    void *d_workspace, size_t workspace_bytes, void *stream);
size_t rpn_roi_sample_targets_workspace_bytes(int B, int R, int G, int add_gt);
int rpn_roi_sample_targets(const float *d_rois, const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels, int B,
                           int R, int G, int add_gt, int total_pos, int total_neg, float pos_iou, float neg_lo, float neg_hi,
                           const float *variances, const int32_t *d_random_pos, const int32_t *d_random_neg, int S,
                           float *d_out_rois, int32_t *d_out_labels, float *d_out_deltas, int32_t *d_out_index,
                           int32_t *d_out_counts, void *d_workspace, size_t workspace_bytes, void *stream);
size_t rpn_roi_losses_workspace_bytes(int B, int R, int C);
int rpn_roi_losses(const float *d_cls_logits, const float *d_reg_pred, const int32_t *d_roi_labels, const float *d_roi_deltas, int B,
                   int R, int C, float *d_losses, float *d_grad_logits, float *d_grad_reg, void *d_workspace, size_t workspace_bytes,
                   void *stream);
int rpn_roi_decode_scores(const float *d_rois, const int32_t *d_valid, const float *d_reg_pred, const float *d_cls_logits,
                          const float *variances, int B, int R, int C, float *d_boxes, float *d_scores, void *stream);

/* ------------------------------------------------------------------------------------
 * Soft-NMS (Bodla et al. 2017, "Improving Object Detection With One Line of Code"; TensorFlow's soft_nms_sigma) in place of
 * rpn_combined_nms behind rpn_roi_decode_scores: overlapping boxes have their scores decayed instead of being deleted.  No
 * reference counterpart.  d_boxes (B,N,q,4) with q in {1,C} and d_scores (B,N,C) as for rpn_combined_nms.
 *
 * Per image b and class c (class 0 is a class like any other here; rpn_roi_decode_scores gives it score 0), in float32:
 *   thr = score_threshold >= 0 (a decay would RAISE a negative score).  A row n is a candidate iff scores[b,n,c] > thr (strict: a
 *   NaN score never qualifies); cur[n] starts as that score.  While a candidate is live and fewer than max_per_class are selected:
 *     m = the live candidate of highest cur, ties to the lower row index; emit (m, cur[m]); m is no longer live;
 *     for every live n, with iou = the NMS-internal IoU of rpn_combined_nms (canonical corners, 0 when either area is <= 0,
 *     inter / (area_m + area_n - inter), one rounding per operation) of box m and box n:
 *       RPN_SOFT_NMS_LINEAR:    iou > iou_threshold:  cur[n] = fl(cur[n] * fl(1 - iou))
 *       RPN_SOFT_NMS_GAUSSIAN:  iou > iou_threshold:  n is removed (TensorFlow's hard cut; a removal, not a product with 0)
 *                               else iou > 0:         cur[n] = fl(cur[n] * expf(fl(fl(iou * iou) * k))),  k = (float)(-1.0 / (double)sigma)
 *       every other case (a NaN iou, iou <= 0, a linear iou <= iou_threshold) leaves cur[n] unchanged;
 *     n stays live iff cur[n] > thr.
 *   iou_threshold = 1 with RPN_SOFT_NMS_GAUSSIAN is the paper's pure Gaussian; sigma = +inf (k = -0.0, every weight exactly 1) is
 *   rpn_combined_nms at the same iou_threshold, bit for bit.  TensorFlow's soft_nms_sigma = s_tf is sigma = 2 s_tf here (TF
 *   multiplies iou^2 by -0.5 / s_tf).
 *   The emitted scores of a class are non-increasing.  The classes' lists of an image are merged by (emitted score descending,
 *   class ascending, selection rank ascending), cut to max_total and padded with zeros.
 * Outputs (M = max_total): d_out_boxes (B,M,4), clipped to [0,1] iff clip_boxes (the IoUs see the unclipped boxes);
 *   d_out_scores (B,M) the DECAYED scores; d_out_classes (B,M) float32 or NULL; d_out_idx (B,M) int32 rows, -1 padded, or NULL;
 *   d_out_valid (B) int32.
 * Determinism: no floating-point atomics, fixed orders -- the same bits on every run, and image b's result depends on image b alone.
 * Limits, refused with RPN_ERR_INVALID before any launch: N <= 4096 (the second stage has R <= 2000; the candidates of a pair
 *   live in LDS, 96 + 28 N bytes); C * min(max_per_class, N) <= 16384 (the merge keeps every staged score in LDS); sigma > 0
 *   (+inf allowed); iou_threshold >= 0; score_threshold >= 0; method one of the two below.
 * d_workspace: rpn_soft_nms_workspace_bytes(...) bytes, REQUIRED (RPN_ERR_WORKSPACE otherwise): per (image, class) the selected
 *   rows and their decayed scores.  Two launches: one workgroup per (image, class), then one per image.
 * ---------------------------------------------------------------------------------- */
typedef enum rpn_soft_nms_method { RPN_SOFT_NMS_LINEAR = 0, RPN_SOFT_NMS_GAUSSIAN = 1 } rpn_soft_nms_method;
size_t rpn_soft_nms_workspace_bytes(int B, int N, int C, int max_per_class, int max_total);
int rpn_soft_nms(const float *d_boxes, const float *d_scores, int B, int N, int q, int C, int max_per_class, int max_total,
                 int method, float iou_threshold, float sigma, float score_threshold, int clip_boxes, float *d_out_boxes,
                 float *d_out_scores, float *d_out_classes, int32_t *d_out_idx, int32_t *d_out_valid, void *d_workspace,
                 size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Detection head: the fully-connected second stage on the RoI features (no reference counterpart: the reference stops at the
 * proposals; the architecture -- two ReLU layers and a class-specific box regressor, the Fast R-CNN head -- is this project's choice,
 * as the thresholds of rpn_roi_targets are).
 *   pooled (B,R,ph,pw,Cf), what rpn_roi_pool writes, read as x (M = B R, K1 = ph pw Cf): Keras' Flatten of NHWC, index (i pw + j) Cf + c
 *   fc1: h1 = relu(x  W1 + b1)    W1 (K1, H1)   Keras Dense layout, (in, out) row-major
 *   fc2: h2 = relu(h1 W2 + b2)    W2 (H1, H2)
 *   cls: logits = h2 Wc + bc      Wc (H2, C)    -> d_logits (M, C)    LOGITS: what rpn_roi_losses / rpn_roi_decode_scores take
 *   reg: deltas = h2 Wr + br      Wr (H2, 4C)   -> d_deltas (M, 4C)   class-specific
 *   Cf, H1, H2 multiples of 4; C >= 2.  Dropout after h1 and h2 is off by default (rate 0) and counter-based ("Dropout" below): it
 *   keeps the run-to-run bit identity of every training entry point.
 * Arithmetic: exact float32 on v_mfma_f32_32x32x2_f32.  Forward: every output element is ONE fmaf chain in k order over the whole
 *   of K starting from +0, then + bias, then max(., 0) where there is a ReLU; no split of K.  A row's result depends on that row
 *   of the input and on the weights alone: the same RoI features give the same bits at any M and beside any other rows.
 *   Backward: dW = in^T dZ and d_in = dZ W^T as rpn_conv1x1_wgrad / rpn_conv1x1_dgrad compute them (cls and reg as one matrix padded
 *   to a multiple of 4 columns), db = the column sums of dZ (chunks of 64 rows in order, then the chunks in order), the ReLU mask
 *   [h > 0] applied to d_h1 / d_h2 in place.  No floating-point atomics, every sum in a fixed order chosen from the shapes alone:
 *   bit-identical from run to run.  Adam is the head trainer's (TF 2.0 ApplyAdam, alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t)
 *   on the device), ONE launch over one flat buffer holding all eight tensors.
 * The object owns all its device memory -- weights, and with trainable = 1 their gradients, Adam's m and v (zero at creation) and
 *   the backward's buffers -- allocated at the first call that needs the device; create, memory_bytes and every argument check run
 *   without one.  trainable = 0 (the inference head) holds the weights and the two hidden activations, which a forward overwrites,
 *   and nothing else: memory_bytes reports weights (x 4 when trainable) and workspace separately.
 *   set_layer / get_layer / get_gradient: HOST arrays, kernel (in, out) + bias (out), names "fc1" | "fc2" | "cls" | "reg"; every
 *   layer must be set before a forward.  get_* synchronise `stream`; nothing else synchronises.
 *   forward: M <= max_rows rows.  keep = 1 (trainable heads only) leaves the hidden activations for ONE use, the backward of that
 *     forward: the head keeps one forward at a time.  Any later forward (kept or not) replaces it, set_layer and adam_step drop it
 *     (the weights it was made with are gone); a forward with keep = 0 leaves nothing to go back through.
 *   backward: d_pooled is the kept forward's input again -- the SAME pointer and M (it is not copied; its contents must not have
 *     changed); anything else, or no kept forward, is RPN_ERR_INVALID: a backward never reads another forward's activations.  (A
 *     second kept forward of the same buffer cannot be told from the first by this check; models.DetectionHead counts calls.)
 *     d_grad_logits (M, C) and d_grad_deltas (M, 4C) are what rpn_roi_losses writes.  The eight parameter gradients REPLACE the
 *     stored ones (get_gradient): they do not accumulate over calls.  d_grad_pooled (M, K1) or NULL: the gradient with respect to
 *     the pooled features, what rpn_roi_pool_backward takes -- NULL skips that product.
 *   adam_step: one update from the stored gradients; t += 1 (rpn_det_head_steps).
 *   Sizes one launch can grid: K1, H1, H2 <= 65535 * 64, max_rows <= 65535 * 64 (create), M <= 65535 * 128 (rpn_fc_forward);
 *   beyond them RPN_ERR_INVALID.  Every argument and state check (unset layers included) comes before the first device call.
 * rpn_fc_forward: the forward product on its own, d_out (M, N) = act(d_a (M, K) d_w (K, N; leading dimension ldw) + d_bias (N) or
 *   NULL), relu = 1: max(., 0).  K % 4 == 0, ldw % 4 == 0, ldw >= N (N itself is free: pad the rows of d_w); M free.
 * d_pooled, d_grad_pooled, d_a, d_w 16-byte aligned.
 *
 * The inference head in split float16 (RPN_PRECISION_F16X3; rpn_det_head_create_ex, rpn_fc_forward_x3).  For one layer
 * out = act(x W + b), on v_mfma_f32_16x16x32_f16:
 *   Input split: every float32 input x enters as hi = f16(x), lo = f16(x - hi), both round-to-nearest-even and unscaled (float16
 *     subnormals are kept), whether x is a pooled feature or a hidden activation: h1 and h2 travel as float32 and are split by the
 *     layer that reads them.
 *   Weight split: every weight w enters as the same split of w * 2^s, ONE s per layer (fc1, fc2, cls, reg each have their own):
 *     s = 12 - e clamped to [-100, 24] where max|w| = m 2^e, m in [0.5, 1), over that layer's kernel (0 for an all-zero kernel) --
 *     the rule of the split convolutions.  The epilogue multiplies the accumulator by 2^-s (exact) before the bias.
 *   Product: hi*hi + hi*lo + lo*hi with float32 accumulation inside the MFMA; lo*lo is dropped.  Then + bias and max(., 0), float32.
 *   Order: K is walked in steps of 32 from 0; in each step the accumulator takes lo*hi, hi*lo, hi*hi in that order.  Nothing depends
 *     on M, there is no split of K and no floating-point atomic: a row's result depends on that row, the weights and the bias only,
 *     the same bits at M = 1 and M = 2400, beside any other rows, on every run.  K tails inside a step of 32 enter as zeros.
 *   Range: an input with |x| > 65504 or a non-finite one (pooled features, h1, h2) raises RPN_STATUS_F16_RANGE in a device word the
 *     head owns (rpn_det_head_status: sticky, never read back by a forward; exactly 65504 does not raise it).  The outputs of such a
 *     forward are invalid: use the float32 head for such features.  A float32 head always reports 0.
 *   Sizes: K % 4 == 0, N and M free, as for the float32 product.
 *   Memory: an F16X3 head keeps its float32 weights (get_layer round-trips bit for bit) AND their packed split image, written on the
 *     device by set_layer from the float32 copy: one 128-byte record of hi and lo halves per column and 32 rows of K, the same
 *     bytes per weight as float32.  The image mirrors the float32 layout, so memory_bytes reports weights as TWICE the float32
 *     head's when every layer's K is a multiple of 32 (0.96 GB at 25 088 x 4096) and the rows up to the next multiple of 32 more
 *     otherwise; the workspace is the same.
 *   rpn_det_head_create_ex: `precision` RPN_PRECISION_F32 (= rpn_det_head_create) or RPN_PRECISION_F16X3.  F16X3 with trainable = 1,
 *     BF16X3 and F32W are RPN_ERR_UNSUPPORTED: training stays exact float32.  backward, adam_step and get_gradient fail on an F16X3
 *     head as on any trainable = 0 head.
 *   rpn_det_head_forward_layer: ONE hidden layer of the head, "fc1" or "fc2", at the head's precision on the caller's buffers,
 *     d_out (M, H) = relu(d_in (M, K) W + b) -- what a forward launches for that layer (a timing / test hook).
 *   rpn_fc_forward_x3: the split product on its own.  d_w is the float32 (K, ldw) matrix ON THE DEVICE; s is taken over its columns
 *     [0, N).  A test entry like rpn_conv2d: every call finds max|w|, allocates, packs and synchronises.  d_status: a device word
 *     that receives RPN_STATUS_F16_RANGE, or NULL.
 *
 * Training the head in split float16 (rpn_det_head_set_train_precision on a trainable = 1 head, which is created in float32).  The
 * master weights, the gradients, the bias sums and Adam stay float32; every PRODUCT runs on v_mfma_f32_16x16x32_f16:
 *   Forward: every forward of such a head that is NOT kept, and every kept forward at dropout rate 0, is the contract above,
 *     unchanged -- the same image, the same s per layer, the same kernel -- so its outputs are bit for bit those of an F16X3
 *     inference head holding the same weights.  (A kept forward at rate > 0 drops its hidden activations: "Dropout" below.)
 *   Gradient split: an output gradient dZ (M, N) enters every product as the hi / lo split (round-to-nearest-even, as above) of
 *     dZ * 2^t, ONE t per gradient tensor: dz (the cls | reg pair side by side, one t over its 5 C real columns), d_h2, d_h1.
 *     t = 12 - e where max|dZ| = m 2^e, m in [0.5, 1), over the M live rows and the real columns; 0 for an all-zero tensor; NaNs are
 *     skipped by the maximum.  t is clamped to [-116, 100]: -116 is what the largest finite float32 gives, so every finite
 *     gradient is brought into float16's range.  The maximum is found on the device (an integer atomicMax on the bits: order-
 *     independent), with no host round trip.
 *   dW = in^T dZ: `in` enters unscaled, with the very split the forward applied to it; dZ as above; the accumulator is multiplied by
 *     2^-t (exact).  The reduction runs over the M rows.
 *   d_in = dZ W^T: dZ as above; W as the split of W * 2^s, s by the forward's rule over the matrix this product sees -- fc1's and
 *     fc2's own s, and for the pair ONE s over cls | reg together (the forward's two scales cannot be factored out of one
 *     reduction).  W is read from the float32 master weights and split on the fly: there is no transposed image.  The accumulator is
 *     multiplied by 2^-(t + s) as TWO exact multiplications, by 2^a and then 2^b with a = -(t + s) / 2 truncated and b = -(t + s) - a
 *     (2^-(t + s) may leave float32's range as one factor; 2^-t alone may overflow an accumulator that 2^-s brings back, so the
 *     halves have the same sign: whatever order of 2^-t and 2^-s stays in range gives these bits).  The reduction runs over the N
 *     real columns.
 *   Product and order: hi*hi + hi*lo + lo*hi, lo*lo dropped, float32 accumulation inside the MFMA.  The reduction index is walked in
 *     steps of 32 from 0, in each step lo*hi, hi*lo, hi*hi; it is never split (2400 rows: 75 steps) and there is no floating-point
 *     atomic.  Reduction tails enter as zeros; M and N need not be multiples of 4 or 32; the padding columns N .. ld - 1 of dZ and W
 *     are read and dropped.  A row of d_in reads that row of dZ, W and the two shifts alone: the same bits at M = 1 and in a batch
 *     whenever the row alone and the batch give the same t (a row that holds an entry of the batch maximum's binade does).
 *   Everything else as in float32: db = the float32 column sums of dZ; the ReLU mask is [h > 0] on the kept activation (now the
 *     split forward's), applied in the epilogue of the d_in product; gradients are stored float32; Adam is ONE launch on the master
 *     weights.  Bit-identical from run to run.
 *   Repack: adam_step refreshes the image and every s on the device from the master weights, by the rule above, without a
 *     synchronisation; set_layer marks the image stale and the next forward refreshes it the same way.  The forward reads its 2^-s
 *     from device memory.
 *   Range: a non-finite gradient raises RPN_STATUS_F16_RANGE (rpn_det_head_status); a finite one of any magnitude does not.  Inputs
 *     and activations raise it as in the forward.
 *   rpn_det_head_set_train_precision: RPN_PRECISION_F32 (the default: exactly the float32 kernels) or RPN_PRECISION_F16X3; BF16X3 and
 *     F32W are RPN_ERR_UNSUPPORTED, a trainable = 0 head or any other value RPN_ERR_INVALID.  It drops a kept forward, keeps the
 *     weights, Adam's moments and the step count, and needs no device: the image is allocated at the next call that needs the device.
 *     rpn_det_head_train_precision reports it.  (rpn_det_head_create_ex(trainable = 1, F16X3) stays RPN_ERR_UNSUPPORTED.)
 *   Memory: from the first set_train_precision(F16X3) on, memory_bytes reports weights as w, g, m, v AND the image -- FIVE times the
 *     float32 inference head's when every layer's K is a multiple of 32 (2.4 GB at 25 088 x 4096 x 4096), the rows up to the next
 *     multiple of 32 more otherwise.  Going back to F32 keeps the image, and the report keeps saying so.
 *   rpn_fc_wgrad_x3 / rpn_fc_dgrad_x3: the two products on their own.  TEST ENTRIES like rpn_fc_forward_x3: every call finds the
 *     maxima, allocates and synchronises.  wgrad: d_out (K, N; leading dimension ldo >= N) = d_a (M, K)^T d_dz (M, N; leading
 *     dimension ldz); the columns N .. ldo - 1 of d_out are not written.  dgrad: d_out (M, K) = d_dz (M, N; ldz) d_w (K, N; ldw)^T,
 *     times [d_h > 0] when d_h (M, K) is given; s is taken over the K x N real entries of d_w.  K % 4 == 0 (wgrad), ldz % 4 == 0,
 *     ldw % 4 == 0, d_a, d_dz, d_w 16-byte aligned; M and N free.  d_status as for rpn_fc_forward_x3.
 *
 * Dropout after the two hidden layers of a trainable head (rpn_det_head_set_dropout; the default rate is 0, at which every kernel,
 * launch and bit is what it is without this section).  Seeded and counter-based: the mask is a function of indices alone, there is
 * no generator state and no mask tensor, and the backward evaluates no random number.
 *   Generator: Philox4x32-10 as in Random123 and cuRAND.  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9,
 *     0xBB67AE85; ten rounds, the key bumped between rounds; one round maps (c0, c1, c2, c3), (k0, k1) to
 *     (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).  Known answers (counter / key -> output):
 *       0 0 0 0 / 0 0                                          -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *       ffffffff x 4 / ffffffff x 2                            -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *       243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   Which word belongs to which element: hidden layer l (0: fc1's output, 1: fc2's), flat row m = b R + r of the call, column n, the
 *     head's dropout call number t.  Counter (n, m >> 2, l, t mod 2^32), key (seed & 0xffffffff, seed >> 32), the element's word is
 *     output word m & 3.  (Both forward kernels' accumulator layouts give a thread four consecutive rows of one column starting at
 *     a multiple of 4: one evaluation serves four stores.)
 *   Mask and value: thr = min(llround(rate 2^32), 2^32 - 1), computed on the host in double.  An element is KEPT iff word >= thr, an
 *     unsigned integer compare with no float conversion (a word equal to thr is kept).  scale = (float)(1.0 / (1.0 - rate)), a
 *     double division rounded once.  The stored hidden activation is fl32(max(z, 0) * scale) where kept and exactly +0.0 where
 *     dropped: Keras' Dropout / tf.nn.dropout, x * 1/(1 - rate) * mask.
 *   When it applies: only on a forward whose activations are kept for a backward -- rpn_det_head_forward(keep = 1) on a trainable
 *     head with rate > 0.  It is the identity in every other forward (keep = 0, rpn_det_head_forward_layer, any inference head), and
 *     those do not advance t: validation runs with keep = 0.  t starts at 0 and increases by one per forward that applied dropout;
 *     both hidden layers of that forward use the same t.
 *   Backward: the stored activation is zero where the element was dropped, and scale >= 1 cannot take a positive value to zero, so
 *     [a_stored > 0] is exactly [z > 0] AND kept.  The backward of a dropped layer is the backward above with one more factor:
 *     d_pre = [a_stored > 0] ? fl32(d * scale) : 0, d being what the input-gradient product writes without dropout; in F16X3 the
 *     factor comes after the two exact powers of two.  dW = in^T dZ reads the stored (dropped, scaled) activation: the correct
 *     operand, unchanged.
 *   What stays guaranteed: no floating-point atomics and fixed summation orders; the same bits on every run for the same (weights,
 *     input, seed, t); the mask of flat row m is the same whether the call is shaped (1, 74) or (2, 37); at the same (seed, t) the
 *     float32 head and the head that trains in F16X3 use the identical mask; at rate == 0 the dropout kernels (new kernels under
 *     their own names) are never launched and no extra multiply happens.
 *   rpn_det_head_set_dropout: 0 <= rate < 1 and finite, and a trainable = 1 head, otherwise RPN_ERR_INVALID.  Needs no device, drops
 *     a kept forward, leaves t alone.  rpn_det_head_dropout_state reports rate, seed and t (the call number the NEXT dropped forward
 *     will use); rpn_det_head_set_dropout_calls sets t, for resuming a run or repeating a call (trainable heads; it leaves a kept
 *     forward alone, whose backward does not read t).
 *   rpn_det_head_get_activation: copies the kept forward's stored hidden activation, "fc1" (M, H1) or "fc2" (M, H2), to d_out on the
 *     device; RPN_ERR_INVALID for any other name or when no forward of M rows is kept.  It is what lets a caller see the mask.
 *   rpn_dropout_forward: the contract's mask and scale on any tensor, d_out (M, N) = keep ? fl32(d_x * scale) : +0, no ReLU, out of
 *     place, M and N free; `calls` is t, `layer` is l (>= 0).  rate as for set_dropout.
 * ---------------------------------------------------------------------------------- */
typedef struct rpn_det_head rpn_det_head;
int rpn_det_head_set_dropout(rpn_det_head *h, double rate, unsigned long long seed);
int rpn_det_head_dropout_state(const rpn_det_head *h, double *rate, unsigned long long *seed, unsigned long long *calls);
int rpn_det_head_set_dropout_calls(rpn_det_head *h, unsigned long long calls);
int rpn_det_head_get_activation(rpn_det_head *h, const char *name, float *d_out, int M, void *stream);
int rpn_dropout_forward(const float *d_x, int M, int N, double rate, unsigned long long seed, unsigned calls, int layer, float *d_out,
                        void *stream);
int rpn_det_head_set_train_precision(rpn_det_head *h, int precision);
int rpn_det_head_train_precision(const rpn_det_head *h);
int rpn_fc_wgrad_x3(const float *d_a, const float *d_dz, int M, int K, int N, int ldz, int ldo, float *d_out, unsigned *d_status,
                    void *stream);
int rpn_fc_dgrad_x3(const float *d_dz, const float *d_w, int M, int K, int N, int ldz, int ldw, const float *d_h, float *d_out,
                    unsigned *d_status, void *stream);
int rpn_det_head_create(int ph, int pw, int Cf, int H1, int H2, int C, int max_rows, int trainable, rpn_det_head **out);
int rpn_det_head_create_ex(int ph, int pw, int Cf, int H1, int H2, int C, int max_rows, int trainable, int precision,
                           rpn_det_head **out);
int rpn_det_head_status(rpn_det_head *h, unsigned *flags, int reset, void *stream);
int rpn_det_head_forward_layer(rpn_det_head *h, const char *name, const float *d_in, int M, float *d_out, void *stream);
int rpn_fc_forward_x3(const float *d_a, const float *d_w, const float *d_bias, int M, int K, int N, int ldw, int relu, float *d_out,
                      unsigned *d_status, void *stream);
void rpn_det_head_destroy(rpn_det_head *h);
int rpn_det_head_memory_bytes(const rpn_det_head *h, size_t *weights, size_t *workspace);
int rpn_det_head_set_layer(rpn_det_head *h, const char *name, const float *kernel, const float *bias);
int rpn_det_head_get_layer(rpn_det_head *h, const char *name, float *kernel, float *bias, void *stream);
int rpn_det_head_get_gradient(rpn_det_head *h, const char *name, float *kernel, float *bias, void *stream);
int rpn_det_head_forward(rpn_det_head *h, const float *d_pooled, int M, int keep, float *d_logits, float *d_deltas, void *stream);
int rpn_det_head_backward(rpn_det_head *h, const float *d_pooled, int M, const float *d_grad_logits, const float *d_grad_deltas,
                          float *d_grad_pooled, void *stream);
int rpn_det_head_adam_step(rpn_det_head *h, float lr, float beta_1, float beta_2, float epsilon, void *stream);
long long rpn_det_head_steps(const rpn_det_head *h);
int rpn_fc_forward(const float *d_a, const float *d_w, const float *d_bias, int M, int K, int N, int ldw, int relu, float *d_out,
                   void *stream);

/* ------------------------------------------------------------------------------------
 * Optimizers: SGD momentum, L2 weight decay, clipping by the global norm, and the optimizer's state
 *   (tf_rpn_amd/csrc/optim_kernels.hip; no reference counterpart: its trainer.py compiles with Adam(1e-5) and nothing else).
 *   Both handles -- rpn_head_trainer and a trainable rpn_det_head -- start as they always were: Adam, no decay, no clip norm, and
 *   in that configuration a step launches exactly what it launched before these entries existed (adam_kernel, no norm pass).
 *
 * set_optimizer(kind, momentum, nesterov, weight_decay, global_clipnorm)
 *   kind: RPN_OPT_ADAM or RPN_OPT_SGD.  momentum in [0, 1) (SGD's; Adam ignores it), nesterov 0 | 1, weight_decay >= 0 and
 *   global_clipnorm >= 0, both finite, 0 = off.  A bad value is RPN_ERR_INVALID with a message, before any device work.  The step
 *   entries (rpn_head_trainer_step / _backward, rpn_det_head_adam_step) keep their arguments: under SGD beta_1, beta_2 and epsilon
 *   are ignored and lr is SGD's.  SWITCHING kind ZEROES m, v AND THE STEP COUNT; setting the same kind again keeps them.
 *   Drops a pending / kept forward.
 *
 * One step over the flat buffer of everything the handle trains, per element, float32, EVERY OPERATION ROUNDED ON ITS OWN:
 *     g1 = g * c                         c: the clip scale below; g itself when no clip norm is configured
 *     g2 = g1 + weight_decay * w         on a DECAYED element; g1 elsewhere
 *     SGD  (Keras / TF 2.0 ApplyKerasMomentum, restated as recalled):  a = momentum * a - lr * g2;  w += a
 *          nesterov: w += momentum * a - lr * g2 with the new a.  momentum = 0 runs the same formula.  a lives in slot 0 (m); slot 1
 *          (v) is not touched.
 *     Adam (ApplyAdam): the arithmetic of the default step on g2; alpha in double on the device from t.
 *   So the clip acts on the LOSS gradient alone -- what get_gradient returns -- and the decay is added after the clip: Caffe's
 *   order, and py-faster-rcnn's.  (The decay is L2, inside the gradient; not AdamW's decoupled form.)
 *   DECAYED elements are the kernels only: never a bias, a BatchNorm's gamma or beta, the bias row of the trainer's fused
 *   513 x 5K head matrix, an alignment gap or a padding column of the detection head's cls | reg pair.  The set is a sorted table
 *   of [begin, end) index ranges derived from the handle's layout and uploaded once (decay_ranges reads it: up to `cap` pairs
 *   into `ranges`, which may be NULL; returns the number of pairs, or -1 for a null handle).  Gaps and padding hold w = 0 and g = 0 and stay exactly zero under every rule.
 *
 * The global norm (global_clipnorm = C > 0 only): S = sum g[i]^2 over the whole gradient buffer in float64 (a float32 square is
 *   exact there), per-workgroup partials in a fixed order and one finishing workgroup; the grid, and with it the order, depends on
 *   the buffer's size alone: the same bits on every run, no floating-point atomics.  The finishing workgroup writes S and
 *   c = sqrt(S) > C ? (float)(C / sqrt(S)) : exactly 1.0f to device memory, where the update reads c: NOTHING IS READ BACK BY A STEP.
 *   A NON-FINITE S (a NaN or an infinite gradient) GIVES c = NaN AND THE STEP CARRIES IT INTO EVERY WEIGHT, as
 *   tf.clip_by_global_norm does: clipping bounds a large step, it does not hide a broken one.
 *   grad_norm: *norm = sqrt(S), the pre-clip global norm, and *scale = c of the last applied step; synchronises `stream`.
 *   RPN_ERR_INVALID when no clip norm is configured or no step has run under it.
 *
 * The optimizer's state, HOST arrays in get_layer's layout: slot 0 is m (Adam's first moment / SGD's accumulator), slot 1 is v.
 *   get_slot / set_slot: kernel + bias of a trained layer (bias NULL for a trained MobileNetV2 conv, and only for it);
 *   get_bn_slot / set_bn_slot: gamma + beta of a trained MobileNetV2 BatchNorm.  A frozen or unknown layer and a slot other than
 *   0 or 1 are RPN_ERR_INVALID.  These entries need the device (the state lives there only).  set_* drops a pending / kept forward,
 *   as set_layer does.  set_steps sets the step count t (>= 0) that Adam's alpha and the next step's number follow.  To resume a
 *   run: create, set_optimizer, set_layer ..., set_slot ..., set_steps.
 *
 * The two kernels on caller buffers (tests, scripts/optimizer_bench.py); every pointer a device pointer:
 *   rpn_grad_sq_norm: d_g (n) float32, 16-byte aligned -> *d_S, *d_scale as above with C = clipnorm (0: the scale is 1).  d_ws:
 *     rpn_grad_sq_norm_workspace_bytes(n) bytes.
 *   rpn_optimizer_apply: one step t (from 1) of `kind` on w, g, m, v (n floats each, 16-byte aligned; d_v may be NULL under SGD).
 *     d_decay_ranges: n_ranges sorted, disjoint, non-empty [begin, end) pairs inside [0, n), 16-byte aligned (the caller's to get
 *     right: the values are only ever compared with element indices); d_scale: the device float c, or NULL for none.  kind = RPN_OPT_ADAM without ranges (or with weight_decay = 0) and without d_scale IS the default
 *     step: it launches adam_kernel.
 * ---------------------------------------------------------------------------------- */
#define RPN_OPT_ADAM 0
#define RPN_OPT_SGD 1
int rpn_head_trainer_set_optimizer(rpn_head_trainer *t, int kind, float momentum, int nesterov, float weight_decay, float global_clipnorm);
int rpn_det_head_set_optimizer(rpn_det_head *h, int kind, float momentum, int nesterov, float weight_decay, float global_clipnorm);
int rpn_head_trainer_grad_norm(rpn_head_trainer *t, double *norm, float *scale, void *stream);
int rpn_det_head_grad_norm(rpn_det_head *h, double *norm, float *scale, void *stream);
int rpn_head_trainer_decay_ranges(const rpn_head_trainer *t, long long *ranges, int cap);
int rpn_det_head_decay_ranges(const rpn_det_head *h, long long *ranges, int cap);
int rpn_head_trainer_get_slot(rpn_head_trainer *t, const char *name, int slot, float *kernel, float *bias, void *stream);
int rpn_head_trainer_set_slot(rpn_head_trainer *t, const char *name, int slot, const float *kernel, const float *bias);
int rpn_head_trainer_get_bn_slot(rpn_head_trainer *t, const char *name, int slot, float *gamma, float *beta, void *stream);
int rpn_head_trainer_set_bn_slot(rpn_head_trainer *t, const char *name, int slot, const float *gamma, const float *beta);
int rpn_det_head_get_slot(rpn_det_head *h, const char *name, int slot, float *kernel, float *bias, void *stream);
int rpn_det_head_set_slot(rpn_det_head *h, const char *name, int slot, const float *kernel, const float *bias);
int rpn_head_trainer_set_steps(rpn_head_trainer *t, long long steps);
int rpn_det_head_set_steps(rpn_det_head *h, long long steps);
size_t rpn_grad_sq_norm_workspace_bytes(long long n);
int rpn_grad_sq_norm(const float *d_g, long long n, float clipnorm, double *d_S, float *d_scale, void *d_ws, size_t ws_bytes, void *stream);
int rpn_optimizer_apply(int kind, float *d_w, const float *d_g, float *d_m, float *d_v, long long n, const long long *d_decay_ranges,
                        int n_ranges, long long t, float lr, float beta_1, float beta_2, float epsilon, float momentum, int nesterov,
                        float weight_decay, const float *d_scale, void *stream);

/* ------------------------------------------------------------------------------------
 * Evaluation: PASCAL VOC average precision of the detections and the recall of the proposals, accumulated on the device (no
 * reference counterpart: its training script stops at val_loss).  The rules are VOCdevkit's VOCevaldet; where the devkit is loose
 * the choice is THIS PROJECT'S and is marked (*).  update / update_proposals enqueue on `stream` and return: no copy to the host,
 * no stream or device synchronisation.  No floating-point atomics; every float64 sum has an order fixed by the counts alone, so
 * result gives the same bits on every run.
 *
 * create: C classes (0 is background), room for max_images images of M detection rows each; iou_threshold in (0, 1]; top_k (n_k)
 *   and recall_iou (n_t): HOST arrays, the cut-offs (>= 1) and IoU thresholds (in (0, 1]) of the proposal recall, at most 8 each.
 *   2 <= C <= 65535, 1 <= M <= 4096, max_images * M <= 2^30.  All device memory -- the records, the two halves of the sort
 *   workspace, the counters: 24 bytes per record in all -- is ONE allocation owned by the handle, made at creation (without a
 *   device, where create, memory_bytes and every argument check still work: by the first call that finds one).
 * update: one batch.  d_boxes (B,M,4) [y1,x1,y2,x2], d_scores (B,M), d_classes (B,M) float32 and d_valid (B,) int32 as
 *   rpn_combined_nms returns them; d_gt_boxes (B,G,4); d_gt_labels (B,G) int32; d_gt_difficult (B,G) bytes or NULL (all zeros);
 *   1 <= G <= 2048; M is the handle's.  d_flags (B,M) int32 or NULL: 1 TP / 0 FP / -1 not counted, for every row.
 *   Live detections: row m of image b counts iff m < valid[b], its class is an integer in [1, C) and its score is finite and > 0.
 *     Every other row is dropped and never indexes memory.
 *   Ground truth: a row counts iff its label is >= 1 (0 is background, -1 padding, as rpn_roi_targets).
 *   Matching, for a live detection of class c: jmax = the gt of label c in the same image of highest IoU -- float32
 *     generate_iou_map arithmetic, every operation rounded on its own -- the FIRST on ties (*), a NaN never wins, difficult gts
 *     included; jmax does not depend on which gts are taken.
 *       no gt of that class, or iou < iou_threshold                          -> FP
 *       iou >= iou_threshold (>=, as the devkit) and the gt is difficult     -> ignored: in neither count, does not take the gt
 *       iou >= iou_threshold, not difficult, and FIRST in (score descending, m ascending (*)) order among the detections of the
 *         image with the same jmax and iou >= iou_threshold                  -> TP;  any later one -> FP
 *   npos[c] = counted, non-difficult gts of label c (labels >= C are not counted); ndet[c] = TP + FP records.
 *   Slot of a row = (images before this batch + b) * M + m.  images + B > max_images or a bad size: RPN_ERR_INVALID, nothing
 *   is enqueued, nothing changes.
 * result: per class, the TP / FP records ordered by score descending, ties to the lower slot (*) (a stable sort); at rank i
 *     precision = tp_i / (tp_i + fp_i) on cumulative counts, divided in float64; recall = tp_i / npos.
 *   d_ap (C,)   all-point (VOC2010+): (sum over TP records t of pmax(t)) / npos, pmax(t) = the maximum precision at any rank >= t's.
 *   d_ap11 (C,) 11-point (VOC2007): the mean over k = 0..10 of the maximum precision among ranks with 10 tp_i >= k npos, 0 if there
 *     is none -- compared IN INTEGERS (*): it does not reproduce the np.arange(0, 1.1, 0.1) rounding of the common Python port.
 *   npos == 0: both NaN (index 0 always); npos > 0 and no records: both 0.  The mean over classes is left to the caller.
 *   d_npos, d_ndet (C,) int32.  d_recall (n_k,n_t) float64 = hits / n_gt, NaN when n_gt == 0; d_n_gt: one long long.  Any output
 *   may be NULL (d_ap and d_ap11 together).  Device pointers; result synchronises nothing either.  It may be called any number
 *   of times, between updates too.
 * update_proposals: the RPN alone.  d_rois (B,R,4), d_valid (B,) or NULL.  For every counted, non-difficult gt (any label >= 1),
 *   every cut-off k and threshold t: a hit iff the maximum over r < min(k, valid[b]) of IoU(roi r, gt) is >= t (no RoI: no hit);
 *   hits[k,t] and n_gt accumulate.  Independent of update's image count.
 * pr_curve: class c's ranking, c in [1, C): the first min(n, cap) records' score, TP flag and slot; *d_n = n = ndet[c].
 * reset: counters and the image count to zero, on `stream`.  images: detection images counted so far (a host counter).
 * d_boxes, d_gt_boxes, d_rois 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct rpn_evaluator rpn_evaluator;
int rpn_evaluator_create(int C, int max_images, int M, float iou_threshold, const int *top_k, int n_k, const float *recall_iou,
                         int n_t, rpn_evaluator **out);
void rpn_evaluator_destroy(rpn_evaluator *e);
int rpn_evaluator_memory_bytes(const rpn_evaluator *e, size_t *bytes);
int rpn_evaluator_reset(rpn_evaluator *e, void *stream);
int rpn_evaluator_images(const rpn_evaluator *e);
int rpn_evaluator_update(rpn_evaluator *e, const float *d_boxes, const float *d_scores, const float *d_classes,
                         const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels,
                         const unsigned char *d_gt_difficult, int B, int G, int32_t *d_flags, void *stream);
int rpn_evaluator_update_proposals(rpn_evaluator *e, const float *d_rois, const int32_t *d_valid, int R, const float *d_gt_boxes,
                                   const int32_t *d_gt_labels, const unsigned char *d_gt_difficult, int B, int G, void *stream);
int rpn_evaluator_result(rpn_evaluator *e, double *d_ap, double *d_ap11, int32_t *d_npos, int32_t *d_ndet, double *d_recall,
                         long long *d_n_gt, void *stream);
int rpn_evaluator_pr_curve(rpn_evaluator *e, int c, float *d_scores, int32_t *d_tp, int32_t *d_slots, int cap, int32_t *d_n,
                           void *stream);

/* ------------------------------------------------------------------------------------
 * Evaluation, COCO style: AP over several IoU thresholds and object sizes, AR at several numbers of detections, accumulated on the
 * device.  A second handle beside rpn_evaluator, which keeps its rules.  The rules are pycocotools' COCOeval in bbox mode AS
 * RECALLED (pycocotools is not a dependency and parity with it is not pinned); where a rule is THIS PROJECT'S choice it is marked
 * (*).  update enqueues on `stream` and returns: no copy to the host, no synchronisation.  No floating-point atomics; every float64
 * sum has an order fixed by the counts alone, so result gives the same bits on every run.
 *
 * create: C, max_images, M with rpn_evaluator_create's limits (2 <= C <= 65535, 1 <= M <= 4096, max_images * M <= 2^30).  HOST arrays:
 *   iou_thresholds (T), 1 <= T <= 10, each in (0, 1]; NULL: the ten float32 values nearest to the doubles 0.5 + 0.05 i.
 *   area_ranges (A,2) of [lo, hi] in pixels^2, 1 <= A <= 4, 0 <= lo <= hi, finite; NULL: [0, 1e10], [0, 32^2], [32^2, 96^2],
 *     [96^2, 1e10].  Index 0 is "all" by convention only.
 *   max_dets (K), 1 <= K <= 4, strictly ascending, 1 <= max_dets[0], max_dets[K-1] <= M; NULL: (1, 10, 100).
 *   height, width: the default image size in float32, finite and > 0.  Boxes are normalised [y1, x1, y2, x2].
 *   All device memory -- 20 bytes of record (score, class and rank, 2 bits per (a, t)) and the two 8-byte halves of the sort
 *   workspace: 36 bytes per detection row of max_images * M in all, plus the counters -- is ONE allocation owned by the handle, made
 *   at creation (without a device, where create, memory_bytes and every argument check still work: by the first call that finds one).
 * update: one batch.  The detection inputs are exactly rpn_evaluator_update's; d_gt_boxes (B,G,4), d_gt_labels (B,G) int32,
 *   d_gt_difficult (B,G) bytes or NULL; 1 <= G <= 2048.  d_image_sizes (B,2) float32 [height, width] or NULL (the handle's size).
 *   Live detections: row m of image b counts iff m < valid[b], its class is an integer in [1, C) and its score is finite and > 0.
 *     Every other row is dropped and never indexes memory.
 *   Ground truth: a row counts iff its label is >= 1 (labels >= C are not counted).
 *   IoU: float32 generate_iou_map arithmetic, every operation rounded on its own.  A NaN IoU never matches (*).
 *   Pixel area of a box = fl32(fl32((y2 - y1) * height) * fl32((x2 - x1) * width)), every operation rounded on its own (*):
 *     pycocotools reads an `area` field, a box-only dataset has only the box.
 *   Per (image b, class c): D = the live detections of class c in (score descending, m ascending) order, cut to the first
 *     max_dets[K-1]; a detection's position in D is its RANK; rows beyond the cut are counted nowhere.  ndet[c] counts the ranked rows.
 *   Per area range a, a gt of label c is IGNORED iff it is difficult or its area is < lo_a or > hi_a (both ends inclusive: a 32 x 32
 *     box is small and medium).  npig[c, a] counts the others.
 *   Matching per (b, c, a, t) with its own `taken` set, the detections of D in order.  Among the untaken, non-ignored gts with
 *     iou >= thr_t the match is the one of highest IoU, the LAST in input order on ties (*) (pycocotools' `if ious[d,g] < iou:
 *     continue`; rpn_evaluator takes the first); if there is none, the same rule among the untaken ignored gts.  A matched gt is
 *     taken, an ignored one too; there are no crowd boxes, every gt matches at most once.
 *       matched to a non-ignored gt                                      -> TP (1)
 *       matched to an ignored gt                                         -> ignored (-1)
 *       unmatched, the detection's own area outside [lo_a, hi_a]         -> ignored (-1)
 *       unmatched otherwise                                              -> FP (0)
 *   d_flags (B,M,A,T) int8 or NULL: 1 / 0 / -1, and -2 for a row that is not counted (not live, or beyond the cut).
 *   Slot of a row = (images before this batch + b) * M + m.  images + B > max_images or a bad size: RPN_ERR_INVALID, nothing is
 *   enqueued, nothing changes.
 * result: per class, the ranked rows ordered by score descending, ties to the lower slot (a stable sort: rpn_evaluator's ranking).
 *   For (c, a, t) and cut-off k: walk the rows with rank < max_dets[k], skip those whose flag at (a, t) is -1, accumulate tp_i, fp_i.
 *   d_ar (C,A,T,K) = tp_total / npig[c, a], one float64 division.
 *   d_ap (C,A,T), at the last cut-off: prec_i = tp_i / (fl64(tp_i + fp_i) + 2^-52) (np.spacing(1)), made non-increasing from the
 *     right; for q = 0..100, p_q = the precision at the first rank with 100 tp_i >= q npig, compared IN INTEGERS (*), 0 if there is
 *     none; ap = (sum of p_q) / 101 in float64.
 *   npig == 0: ap and ar NaN (class 0 always); npig > 0 and no rows: 0.  d_npig (C,A), d_ndet (C,) int32.  Device pointers, any may
 *   be NULL; result synchronises nothing and may be called any number of times, between updates too.
 * reset: counters and the image count to zero, on `stream`.  images: images counted so far (a host counter).
 * d_boxes, d_gt_boxes 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct rpn_coco_evaluator rpn_coco_evaluator;
int rpn_coco_evaluator_create(int C, int max_images, int M, const float *iou_thresholds, int T, const float *area_ranges, int A,
                              const int *max_dets, int K, float height, float width, rpn_coco_evaluator **out);
void rpn_coco_evaluator_destroy(rpn_coco_evaluator *e);
int rpn_coco_evaluator_memory_bytes(const rpn_coco_evaluator *e, size_t *bytes);
int rpn_coco_evaluator_reset(rpn_coco_evaluator *e, void *stream);
int rpn_coco_evaluator_images(const rpn_coco_evaluator *e);
int rpn_coco_evaluator_update(rpn_coco_evaluator *e, const float *d_boxes, const float *d_scores, const float *d_classes,
                              const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels,
                              const unsigned char *d_gt_difficult, const float *d_image_sizes, int B, int G, signed char *d_flags,
                              void *stream);
int rpn_coco_evaluator_result(rpn_coco_evaluator *e, double *d_ap, double *d_ar, int32_t *d_npig, int32_t *d_ndet, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RPN_HIP_H */
