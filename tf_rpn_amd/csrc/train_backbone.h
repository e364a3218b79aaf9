// train_backbone.h -- host-side interface of the VGG16 backbone backward kernels (train_backbone_kernels.hip; internal to
// librpn_hip.so).  Every kernel is float32, writes each output once, and uses no floating-point atomics.  launch_wgrad_wide runs the
// 3x3 weight-gradient kernel of train_kernels.hip (train_head.h: launch_wgrad_slabs); the helpers the training kernel files share are
// in train_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rpn {

// dgrad of a 3x3 stride-1 'same' conv: dx (B,H,W,Cin) = conv_transpose(dy (B,H,W,Cout), w HWIO), then dx += add when add is given
// (same shape as dx; it may be dx), then dx *= [mask > 0] when mask is given.  wt: 9 Cout Cin floats of device scratch that receive
// the flipped, transposed weights W'[r][s][co][ci] = W[2-r][2-s][ci][co].  Cin % 4 == 0, Cout % 16 == 0.
hipError_t launch_conv3x3_dgrad(const float *dy, const float *w_hwio, const float *mask, const float *add, int B, int H, int W, int Cin,
                                int Cout, float *wt, float *dx, hipStream_t s);
// whether the dgrad runs on the 128 x 128 tile (else 128 x 64): chosen from the shape alone, the bits are the same either way
bool conv3x3_dgrad_wide_tile(int B, int H, int W, int Cin);

// MaxPooling2D(2, 2) 'valid' backward with the ReLU mask of the pooled tensor fused in: dy (B,H,W,C) gets dpool (B,H/2,W/2,C) at
// the first maximum of each window (row-major, replaced only by a strictly greater value) when that maximum is > 0, 0 elsewhere
// (rows / columns no window covers included).  C % 4 == 0.
hipError_t launch_maxpool2x2_backward(const float *y, const float *dpool, int B, int H, int W, int C, float *dy, hipStream_t s);

// weight + bias gradient of a 3x3 stride-1 'same' conv at backbone shapes: x (B,H,W,cin_x) -- cin_x = Cin rounded up to 4; the
// extra channels, if any, must be 0 -- and dy (B,H,W,Cout) -> dw (3,3,Cin,Cout) HWIO, db (Cout).  The pixels are split into
// wgrad_wide_leaves(...) fixed ranges (a power of two, from the shape alone) that are summed in a fixed pairwise tree; db is one
// more row of the same GEMM (a row of ones: conv3x3_wgrad_f32_kernel<true>).  part: wgrad_wide_ws_floats(...) floats of device scratch.
int wgrad_wide_leaves(int B, int H, int W, int Cin, int Cout);
size_t wgrad_wide_ws_floats(int B, int H, int W, int Cin, int Cout);
hipError_t launch_wgrad_wide(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, float *part, float *dw, float *db,
                             hipStream_t s);

// (P, 3) -> (P, 4) with a zero fourth channel: the first layer's input as wgrad_wide reads it
hipError_t launch_pad_channels3to4(const float *x, long long P, float *out, hipStream_t s);

}  // namespace rpn
