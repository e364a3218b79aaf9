// det_head.h -- host-side interface of the detection head's own kernels (det_head_kernels.hip; internal to librpn_hip.so): the
// fully-connected forward GEMM on the float32 MFMA and the two small element-wise kernels of the head's backward.  The weight and
// input gradients run on train_mnv2.h's launch_conv1x1_wgrad / launch_conv1x1_dgrad, the bias gradients on train_head.h's
// launch_colsum and the update on train_head.h's launch_adam.  Every kernel is float32, writes each output once and uses no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rpn {

// out (M, N) = act(a (M, K) row-major . w (K, N) row-major with leading dimension ldw + bias (N) or nothing); relu != 0: max(., 0).
// K % 4 == 0, ldw % 4 == 0, ldw >= N (the columns N .. ldw - 1 of w are read and dropped), a and w 16-byte aligned; M, N free.
// Columns [0, split) go to out0 (M, split), columns [split, N) to out1 (M, N - split): two contiguous tensors from one product
// (split == N: out0 alone, out1 unused).  Every element is one k-ordered fmaf chain over the whole of K from +0, the bias added after
// it: a row's bits depend on that row of a, on w and on bias alone.
hipError_t launch_fc_forward(const float *a, const float *w, const float *bias, int M, int K, int N, int ldw, int relu, int split,
                             float *out0, float *out1, hipStream_t s);

// dz (M, npad) = [grad_logits (M, C) | grad_deltas (M, 4 C) | zeros]: the gradient of the padded cls | reg product
hipError_t launch_pack_pair_grad(const float *grad_logits, const float *grad_deltas, int M, int C, int npad, float *dz, hipStream_t s);

// g (n floats, n % 4 == 0) <- g [h > 0], in place: the ReLU of the layer whose output h is
hipError_t launch_relu_mask(float *g, const float *h, long long n, hipStream_t s);

}  // namespace rpn
