// train_mnv2.h -- host-side interface of the MobileNetV2 backward kernels (train_mnv2_kernels.hip; internal to librpn_hip.so):
// training-mode BatchNorm, the 1x1 conv backward on the float32 MFMA, the depthwise 3x3 backward (stride 1 and stride 2) and the
// stem's weight gradient.  The two depthwise strides are instances of one kernel pair; the fixed 32-leaf tree (tree_sum32), the
// lane-sum epilogue of the per-channel weight gradients and the other shared helpers are in train_common.h.  Every kernel is
// float32 (float64 partial sums inside the BatchNorm reductions), writes each output once and uses no floating-point atomics; every
// reduction is a fixed number of leaves, chosen from the shape alone, added in a fixed tree.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rpn {

// leaves of a per-channel reduction over P pixels (BatchNorm statistics / backward sums, depthwise weight gradient): a power of
// two <= 32 from P alone
int mn_reduce_leaves(long long P);

// ---- BatchNorm over the P = B H W pixels of a (P, C) NHWC tensor, C % 4 == 0 ---------------------------------------------------
// part: bn_part_doubles(P, C) doubles of device scratch
size_t bn_part_doubles(long long P, int C);
// batch mean, biased batch variance and rstd = 1 / sqrt(var + eps) of x -> mean, var, rstd (C each); with mmean / mvar non-null the
// moving statistics are updated in the same launch: moving = moving * momentum + batch * (1 - momentum), the variance with
// Bessel's correction P / (P - 1)
hipError_t launch_bn_train_stats(const float *x, long long P, int C, float eps, float momentum, double *part, float *mean, float *var,
                                 float *rstd, float *mmean, float *mvar, hipStream_t s);
// rstd = 1 / sqrt(var + eps) in the same form (inference mode: var = the moving variance; the single-layer backward entry)
hipError_t launch_bn_rstd(const float *var, int C, float eps, float *rstd, hipStream_t s);
// y = act(gamma (x - mean) rstd + beta) (+ res); relu6 != 0: min(max(., 0), 6)
hipError_t launch_bn_apply(const float *x, long long P, int C, const float *mean, const float *rstd, const float *gamma,
                           const float *beta, int relu6, const float *res, float *y, hipStream_t s);
// dy' = dy [0 < y < 6] (relu6; y recomputed from x as launch_bn_apply computes it) or dy; dbeta = sum dy', dgamma = sum dy' xhat,
// dx = gamma rstd (dy' - dbeta / P - xhat dgamma / P).  Two passes over the tensor.  dx may be dy.
hipError_t launch_bn_backward(const float *x, const float *dy, long long P, int C, const float *mean, const float *rstd,
                              const float *gamma, const float *beta, int relu6, double *part, float *dgamma, float *dbeta, float *dx,
                              hipStream_t s);

// ---- 1x1 conv backward on v_mfma_f32_32x32x2_f32: x (P, Cin), dy (P, Cout), w (Cin, Cout); Cin, Cout multiples of 4 --------------
// dw (Cin, Cout) = x^T dy: the pixels in conv1x1_wgrad_leaves(...) fixed ranges (a power of two <= 32 from the shape alone) summed in
// a fixed tree.  part: conv1x1_wgrad_ws_floats(...) floats (0 when there is one leaf).
int conv1x1_wgrad_leaves(long long P, int Cin, int Cout);
size_t conv1x1_wgrad_ws_floats(long long P, int Cin, int Cout);
hipError_t launch_conv1x1_wgrad(const float *x, const float *dy, long long P, int Cin, int Cout, float *part, float *dw, hipStream_t s);
// dx (P, Cin) = dy w^T (+ add (P, Cin): the gradient that reaches a residual block's input beside its expand conv)
hipError_t launch_conv1x1_dgrad(const float *dy, const float *w, const float *add, long long P, int Cin, int Cout, float *dx,
                                hipStream_t s);

// ---- depthwise 3x3 stride-1 'same' backward: x, dy (B, H, W, C), w (3, 3, C); C % 4 == 0 ------------------------------------------
// dx[b][y][x][c] = sum_{r,s} dy[b][y+1-r][x+1-s][c] w[r][s][c] (the depthwise conv with flipped taps)
hipError_t launch_dwconv3x3_dgrad(const float *dy, const float *w, int B, int H, int W, int C, float *dx, hipStream_t s);
// dw[r][s][c] = sum_{b,y,x} x[b][y+r-1][x+s-1][c] dy[b][y][x][c]; part: dwconv3x3_wgrad_ws_floats(...) floats
size_t dwconv3x3_wgrad_ws_floats(long long P, int C);
hipError_t launch_dwconv3x3_wgrad(const float *x, const float *dy, int B, int H, int W, int C, float *part, float *dw, hipStream_t s);

// ---- the stride-2 layers: Keras ZeroPadding2D(correct_pad(3)) + a 3x3 stride-2 'valid' conv ----------------------------------------
// one spatial dim of n input pixels: pad before = n % 2 (even: 0, odd: 1), pad after = 1, out = (n + before + 1 - 3) / 2 + 1
inline void mn_s2_geom(int n, int *pad_before, int *out)
{
    *pad_before = n % 2;
    *out = (n + *pad_before + 1 - 3) / 2 + 1;
}
// depthwise, x (B, H, W, C), dy (B, OH, OW, C), w (3, 3, C), C % 4 == 0:
// dx[b][y][x][c] = sum_{r,s} dy[b][(y+pt-r)/2][(x+pl-s)/2][c] w[r][s][c] over the taps where both quotients are exact and in range;
// every dx element is written
hipError_t launch_dwconv3x3_s2_dgrad(const float *dy, const float *w, int B, int H, int W, int C, float *dx, hipStream_t s);
// dw[r][s][c] = sum_{b,oy,ox} x[b][2oy+r-pt][2ox+s-pl][c] dy[b][oy][ox][c]; mn_reduce_leaves(B OH OW) leaves;
// part: dwconv3x3_s2_wgrad_ws_floats(...) floats
size_t dwconv3x3_s2_wgrad_ws_floats(int B, int H, int W, int C);
hipError_t launch_dwconv3x3_s2_wgrad(const float *x, const float *dy, int B, int H, int W, int C, float *part, float *dw, hipStream_t s);
// the stem (Conv1), x (B, H, W, 3), dy (B, OH, OW, Cout), Cout % 4 == 0: dw (3, 3, 3, Cout)[r][s][ci][co] = sum_{b,oy,ox}
// x[b][2oy+r-pt][2ox+s-pl][ci] dy[b][oy][ox][co] over stem_wgrad_leaves(B OH OW) leaves (a power of two <= 256 from the pixel count
// alone) added in a fixed two-level tree; part: conv3x3_s2_cin3_wgrad_ws_floats(...) floats.  x is read element-wise (no alignment).
int stem_wgrad_leaves(long long P);
size_t conv3x3_s2_cin3_wgrad_ws_floats(int B, int H, int W, int Cout);
hipError_t launch_conv3x3_s2_cin3_wgrad(const float *x, const float *dy, int B, int H, int W, int Cout, float *part, float *dw,
                                        hipStream_t s);

}  // namespace rpn
