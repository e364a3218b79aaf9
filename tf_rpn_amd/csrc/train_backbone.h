// train_backbone.h -- host-side interface of the VGG16 backbone backward kernels (train_backbone_kernels.hip: float32;
// train_backbone_x3_kernels.hip: the two 3x3 products in split float16; internal to librpn_hip.so).  Every kernel writes each output
// once and uses no floating-point atomics.  launch_wgrad_wide runs the
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

// the sum of the L leaf slabs of (9 cin_x + 1) x Cout floats in part, slab i with slab i + half down the fixed pairwise tree, ->
// dw (3,3,Cin,Cout) without the padded channels and db (Cout) from row 9 cin_x: the second half of launch_wgrad_wide, which the
// split-float16 weight gradient below shares
hipError_t launch_wgrad_wide_sum(float *part, int L, int cin_x, int Cin, int Cout, float *dw, float *db, hipStream_t s);

// ---- the same two products in split float16 (train_backbone_x3_kernels.hip; contract in include/rpn_hip.h) ---------------------------
// A scale pair in device memory is {2^e, 2^-e}.  launch_scale_x3: max|x| over n floats (any 4-byte aligned x: float4 loads when x is
// 16-byte aligned and n % 4 == 0, scalar ones otherwise -- the maximum is the same) into *bits
// (zeroed here) and its pair into scale[0 .. 1] by the head's rule (launch_fc_scales_x3: gradient -> t in [-116, 100], else the
// weights' s), all on the stream.
hipError_t launch_scale_x3(const float *x, long long n, bool gradient, unsigned *bits, float *scale, hipStream_t s);
// dgrad: gscale = the pair of dy's t (launch_scale_x3 over dy; the weight gradient that reads the same dy takes the same pair);
// image: dgrad_x3_image_bytes(Cin, Cout) bytes that receive the flipped, transposed, split 2^s W'; wbits / wscale: one word and one
// pair that receive max|w| and s.  add / mask as launch_conv3x3_dgrad; status (or null) receives RPN_STATUS_F16_RANGE.  dy must be
// 16-byte aligned; w_hwio needs 4-byte alignment only (the trainer's master kernels follow the head's 5 K columns in one flat buffer):
// the scan and the packing read an unaligned w with scalar loads.
size_t dgrad_x3_image_bytes(int Cin, int Cout);
bool conv3x3_dgrad_x3_wide_tile(int B, int H, int W, int Cin);
hipError_t launch_conv3x3_dgrad_x3(const float *dy, const float *w_hwio, const float *mask, const float *add, int B, int H, int W, int Cin,
                                   int Cout, const float *gscale, void *image, unsigned *wbits, float *wscale, float *dx, unsigned *status,
                                   hipStream_t s);
// wgrad: Cin % 4 == 0; the leaves, the slab layout (part: wgrad_wide_ws_floats(...) floats) and the tree are launch_wgrad_wide's; db
// is the GEMM's row of ones
hipError_t launch_wgrad_wide_x3(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, const float *gscale, float *part,
                                float *dw, float *db, unsigned *status, hipStream_t s);

// (P, 3) -> (P, 4) with a zero fourth channel: the first layer's input as wgrad_wide reads it
hipError_t launch_pad_channels3to4(const float *x, long long P, float *out, hipStream_t s);

}  // namespace rpn
