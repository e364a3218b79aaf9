// train_common.h -- what the training kernel files (train_kernels.hip, train_backbone_kernels.hip, train_mnv2_kernels.hip) share:
// the 1-D grid rule, the MFMA accumulator type, the tile of the 3x3 weight-gradient kernel, the fixed 32-leaf tree and the
// lane-sum epilogue of the per-channel weight gradients.  (a256, the workspace rounding, is in rpn_common.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace rpn {

// workgroups of 256 threads for a grid-stride loop over n items, at most cap of them (the cap changes speed only)
inline int grid_1d(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap)); }

// one 32x32 block of v_mfma_f32_32x32x2_f32 results: element e of a lane is row 8 (e / 4) + 4 (lane / 32) + e % 4, column lane % 32
using f32x16t = __attribute__((ext_vector_type(16))) float;

// conv3x3_wgrad_f32_kernel (train_kernels.hip): a 128 x 128 tile of dW per workgroup, K slices of 16 pixels; LDS row stride 160: the
// two half-waves of a fragment read hit disjoint banks
constexpr int kWgBM = 128, kWgBN = 128, kWgBK = 16, kWgLd = 160;

constexpr int kMaxLeaves = 32;

// sum of `leaves` (a power of two <= 32) values stride apart, in a fixed tree: absent leaves are zeros, which change no bit
template <class T>
__device__ inline T tree_sum32(const T *p, size_t stride, int leaves)
{
    T v[kMaxLeaves];
#pragma unroll
    for (int i = 0; i < kMaxLeaves; ++i) v[i] = i < leaves ? p[(size_t)i * stride] : T(0);
#pragma unroll
    for (int w = kMaxLeaves / 2; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) v[i] = v[i] + v[i + w];
    return v[0];
}

// The end of a per-channel weight-gradient workgroup of QUADS channel quads x LANES pixel lanes (256 threads; thread = lane rl, quad
// q): every thread stores its nine float4 sums to red[lane][row][QUADS * 4 channels of tile `tile`], barrier, then each (row, channel)
// adds its LANES values in lane order and is stored once, to rows[row * C + ch].  The caller puts a barrier between two calls.
template <int QUADS, int LANES>
__device__ __forceinline__ void lane_sum_store(float (&red)[LANES][9 * QUADS * 4], const float4 *acc, int q, int rl, int tile, int C,
                                               float *__restrict__ rows)
{
    constexpr int TC = QUADS * 4;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        red[rl][t * TC + 4 * q + 0] = acc[t].x;
        red[rl][t * TC + 4 * q + 1] = acc[t].y;
        red[rl][t * TC + 4 * q + 2] = acc[t].z;
        red[rl][t * TC + 4 * q + 3] = acc[t].w;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 9 * TC; o += 256) {
        const int t = o / TC, ch = tile * TC + (o % TC);
        float a = 0.0f;
        for (int l = 0; l < LANES; ++l) a += red[l][o];
        if (ch < C) rows[(size_t)t * C + ch] = a;
    }
}

}  // namespace rpn
