// x3_tile.h -- the device helpers the split-float16 GEMM kernels share (det_head_x3_kernels.hip: the detection head's forward and
// backward products; train_backbone_x3_kernels.hip: the VGG16 backbone's backward products): the hi / lo split of eight floats with
// its range probe, the v_mfma_f32_16x16x32_f16 wrapper, the workgroup tile and one step of 32 of the reduction from the LDS records.
// Arithmetic contract in include/rpn_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rpn {

using x3_f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using x3_f32x4 = __attribute__((ext_vector_type(4))) float;

// 8 floats -> the 16-byte piece of their hi halves and the piece of their lo halves (x - hi), round-to-nearest-even, unscaled:
// split_conv.h's split_piece<true>, both pieces at once.  `status` (may be null) receives RPN_STATUS_F16_RANGE when a
// value does not fit float16 (|x| > 65504 or non-finite); fmaxf drops NaNs, so x * 0 accumulates to NaN for any NaN / inf.
__device__ __forceinline__ void split8_x3(const float (&x)[8], uint4 &hi, uint4 &lo, unsigned *status)
{
    if (status) {
        const float m = fmaxf(fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))),
                              fmaxf(fmaxf(fabsf(x[4]), fabsf(x[5])), fmaxf(fabsf(x[6]), fabsf(x[7]))));
        float nan_probe = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) nan_probe = fmaf(x[k], 0.0f, nan_probe);
        if (!(m <= 65504.0f) || nan_probe != 0.0f) atomicOr(status, 1u /* RPN_STATUS_F16_RANGE */);
    }
    x3_f16x8 h, l;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        h[k] = (_Float16)x[k];
        l[k] = (_Float16)(x[k] - (float)h[k]);
    }
    hi = __builtin_bit_cast(uint4, h);
    lo = __builtin_bit_cast(uint4, l);
}

__device__ __forceinline__ x3_f32x4 mfma_x3(uint4 a, uint4 b, x3_f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(x3_f16x8, a), __builtin_bit_cast(x3_f16x8, b), c, 0, 0, 0);
}

// The workgroup tile: 128 x 128 outputs, four waves of 64 x 64 = 4 x 4 MFMA blocks of 16 x 16, the reduction in steps of 32 = one
// MFMA depth.  LDS records: a row's (column's) 32 reduction values as four hi and four lo 16-byte pieces in 128 bytes, piece p at
// slot p ^ (row / 2 % 8).
constexpr int kX3BM = 128, kX3BN = 128, kX3BK = 32;

// One step of 32 of the reduction from the LDS records of a 128 x (32 NJ) tile: wave (wm, wn) owns 4 x NJ MFMA blocks, rows
// wm * 64 + 16 i + lane % 16 of As, columns wn * 16 NJ + 16 j + lane % 16 of Bs.  Fragments (row / column = lane % 16, k octet =
// lane / 16) are single ds_read_b128s; each accumulator takes lo*hi, hi*lo, hi*hi in that order.
template <int NJ>
__device__ __forceinline__ void x3_mma_step_n(const uint4 *__restrict__ As, const uint4 *__restrict__ Bs, x3_f32x4 (&acc)[4][NJ], int wm,
                                              int wn, int l16, int q)
{
    uint4 ah[4], al[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wm * 64 + 16 * i + l16, sw = (r >> 1) & 7;
        ah[i] = As[r * 8 + (q ^ sw)];
        al[i] = As[r * 8 + ((4 + q) ^ sw)];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = wn * 16 * NJ + 16 * j + l16, sw = (c >> 1) & 7;
        const uint4 bh = Bs[c * 8 + (q ^ sw)], bl = Bs[c * 8 + ((4 + q) ^ sw)];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(al[i], bh, acc[i][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(ah[i], bl, acc[i][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(ah[i], bh, acc[i][j]);
    }
}

// the 128 x 128 tile's step: the forward's fragment reads and MFMA order
__device__ __forceinline__ void x3_mma_step(const uint4 *__restrict__ As, const uint4 *__restrict__ Bs, x3_f32x4 (&acc)[4][4], int wm,
                                            int wn, int l16, int q)
{
    x3_mma_step_n<4>(As, Bs, acc, wm, wn, l16, q);
}

// acc * 2^-(t + s) as two exact factors 2^a 2^b, a + b = -(t + s) in halves of the same sign, from the device's {2^t, 2^-t} and
// {2^s, 2^-s} pairs: 2^-(t + s) may leave float32's range as one factor, and 2^-t alone may overflow an accumulator that 2^-s
// brings back (a huge gradient, small weights)
__device__ __forceinline__ void x3_unscale_factors(float inv_t, float inv_s, float &f1, float &f2)
{
    const int ex = (int)((__float_as_uint(inv_t) >> 23) & 0xffu) + (int)((__float_as_uint(inv_s) >> 23) & 0xffu) - 254;
    const int ea = ex / 2, eb = ex - ea;
    f1 = __uint_as_float((unsigned)(ea + 127) << 23);
    f2 = __uint_as_float((unsigned)(eb + 127) << 23);
}

}  // namespace rpn
