// det_head.h -- host-side interface of the detection head's own kernels (det_head_kernels.hip; internal to librpn_hip.so): the
// fully-connected forward GEMM on the float32 MFMA and the two small element-wise kernels of the head's backward.  The weight and
// input gradients run on train_mnv2.h's launch_conv1x1_wgrad / launch_conv1x1_dgrad, the bias gradients on train_head.h's
// launch_colsum and the update on train_head.h's launch_adam.  Those kernels are float32, write each output once and use no atomics.
// The inference head's split-float16 forward (det_head_x3_kernels.hip) is declared below them: no floating-point atomics either
// (its range flag is an atomicOr on a status word, the max|.| scans an integer atomicMax), and neither have the two backward products
// of a head trained in split float16 (rpn_det_head_set_train_precision), declared last.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dropout.h"

namespace rpn {

// out (M, N) = act(a (M, K) row-major . w (K, N) row-major with leading dimension ldw + bias (N) or nothing); relu != 0: max(., 0).
// K % 4 == 0, ldw % 4 == 0, ldw >= N (the columns N .. ldw - 1 of w are read and dropped), a and w 16-byte aligned; M, N free.
// Columns [0, split) go to out0 (M, split), columns [split, N) to out1 (M, N - split): two contiguous tensors from one product
// (split == N: out0 alone, out1 unused).  Every element is one k-ordered fmaf chain over the whole of K from +0, the bias added after
// it: a row's bits depend on that row of a, on w and on bias alone.
hipError_t launch_fc_forward(const float *a, const float *w, const float *bias, int M, int K, int N, int ldw, int relu, int split,
                             float *out0, float *out1, hipStream_t s);

// ---- the same product in split float16 (det_head_x3_kernels.hip; arithmetic contract in include/rpn_hip.h) ----------------------------
// Packed image of a (K, ld) float32 matrix times 2^shift: [ceil(K / 32)][ld][8 pieces of 16 bytes] -- for column n and 32 rows of K
// the logical pieces are hi k 0-7, hi k 8-15, hi k 16-23, hi k 24-31, lo k 0-7, ..., lo k 24-31 (float16), piece p stored at slot
// p ^ (n / 2 % 8): the kernel's LDS image, copied as it is.  Rows beyond K are zeros.  The same bytes per weight as float32.
inline size_t fc_x3_packed_bytes(int K, int ld) { return (size_t)((K + 31) / 32) * (size_t)ld * 128; }

// packs columns [c0, c0 + ncols) of w (K, ld; float32 on the device) into `packed`; the other columns of the image are left alone.
// dmul (device memory) non-null: the multiplier 2^shift is read from there and `shift` is ignored
hipError_t launch_fc_pack_x3(const float *w, int K, int ld, int c0, int ncols, int shift, void *packed, hipStream_t s,
                             const float *dmul = nullptr);

// *out_bits = max over rows < K, columns < N of the bits of |w| (non-negative floats order as their bits; NaNs are skipped);
// *out_bits must be zero before the call
hipError_t launch_fc_absmax(const float *w, int K, int N, int ld, unsigned *out_bits, hipStream_t s);

// out = act(scale * (a . packed) + bias), `scale` = scale0 for columns < split and scale1 for the others (2^-shift of the packing);
// the rest as launch_fc_forward, ld % 4 == 0 being the image's column count.  status: the float16 range flag, or null.
hipError_t launch_fc_forward_x3(const float *a, const void *packed, const float *bias, int M, int K, int N, int ld, int relu, int split,
                                float scale0, float scale1, float *out0, float *out1, unsigned *status, hipStream_t s,
                                const float *dscale0 = nullptr, const float *dscale1 = nullptr);   // non-null: the scales, from device memory

// ---- the backward products of a head trained in split float16 (arithmetic contract in include/rpn_hip.h) --------------------------------
// A scale pair in device memory is {2^s, 2^-s}.  scales[2 i], scales[2 i + 1], i < n, from bits[i] (what launch_fc_absmax leaves): s =
// 12 - e clamped to [-100, 24] (weights, split_weight_shift's rule) or to [-116, 100] (`gradient`), s = 0 for a zero maximum; with
// joint_a >= 0 pair n is taken from the larger of bits[joint_a] and bits[joint_b] (cls | reg as one matrix).
hipError_t launch_fc_scales_x3(const unsigned *bits, int n, int joint_a, int joint_b, bool gradient, float *scales, hipStream_t s);

// out (K, N; leading dimension ldo) = a (M, K)^T dz (M, N; leading dimension ldz): a unscaled, dz as the split of dz * gscale[0], the
// accumulator times gscale[1].  K % 4 == 0, ldz % 4 == 0, a and dz 16-byte aligned; the columns N .. ldz - 1 of dz are read and
// dropped, the columns N .. ldo - 1 of out are not written.  M is walked in steps of 32 from 0, never split.
hipError_t launch_fc_wgrad_x3(const float *a, const float *dz, int M, int K, int N, int ldz, int ldo, const float *gscale, float *out,
                              unsigned *status, hipStream_t s);

// out (M, K) = dz (M, N; ldz) w (K, N; ldw)^T [h > 0] (h (M, K) or null): dz as the split of dz * gscale[0], w as the split of
// w * wscale[0], the accumulator times gscale[1] * wscale[1] (as two exact factors of the same sign).  ldz % 4 == 0, ldw % 4 == 0, dz and w 16-byte aligned.
hipError_t launch_fc_dgrad_x3(const float *dz, const float *w, const float *h, int M, int K, int N, int ldz, int ldw, const float *gscale,
                              const float *wscale, float *out, unsigned *status, hipStream_t s);

// dz (M, npad) = [grad_logits (M, C) | grad_deltas (M, 4 C) | zeros]: the gradient of the padded cls | reg product
hipError_t launch_pack_pair_grad(const float *grad_logits, const float *grad_deltas, int M, int C, int npad, float *dz, hipStream_t s);

// g (n floats, n % 4 == 0) <- g [h > 0], in place: the ReLU of the layer whose output h is
hipError_t launch_relu_mask(float *g, const float *h, long long n, hipStream_t s);

// ---- dropout after a hidden layer (dropout.h; contract in include/rpn_hip.h) -------------------------------------------------------------
// New kernels under their own names: the kernels above are launched exactly as before whenever no dropout applies.
// out (M, N) = keep ? fl32(max(a . w + bias, 0) * scale) : +0 -- launch_fc_forward with relu = 1 and split = N, dropped
hipError_t launch_fc_forward_dropout(const float *a, const float *w, const float *bias, int M, int K, int N, int ldw,
                                     const DropoutArgs &drop, float *out, hipStream_t s);

// the same in split float16 with the scale in device memory (a training head's): launch_fc_forward_x3 with relu = 1 and split = N
hipError_t launch_fc_forward_x3_dropout(const float *a, const void *packed, const float *bias, int M, int K, int N, int ld,
                                        const float *dscale, const DropoutArgs &drop, float *out, unsigned *status, hipStream_t s);

// g <- h > 0 ? fl32(g * scale) : 0, in place: the backward of a dropped layer whose STORED (dropped, scaled) output h is
hipError_t launch_relu_scale_mask(float *g, const float *h, long long n, float scale, hipStream_t s);

// launch_fc_dgrad_x3 with the dropped layer's factor after the two exact ones: out = h > 0 ? fl32(acc f1 f2 * scale) : 0 (h non-null)
hipError_t launch_fc_dgrad_x3_dropout(const float *dz, const float *w, const float *h, int M, int K, int N, int ldz, int ldw,
                                      const float *gscale, const float *wscale, float scale, float *out, unsigned *status, hipStream_t s);

// out (M, N) = keep ? fl32(x * scale) : +0, out of place; M and N free
hipError_t launch_dropout_forward(const float *x, int M, int N, const DropoutArgs &drop, float *out, hipStream_t s);

}  // namespace rpn
