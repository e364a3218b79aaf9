// det_head_x3_kernels.hip -- the detection head's forward product in split float16 (RPN_PRECISION_F16X3; contract in
// include/rpn_hip.h, host interface in det_head.h): the GEMM on v_mfma_f32_16x16x32_f16, the device-side weight packing and the
// max|w| scan of the test entry.  The head object and the ABI live in det_head_kernels.hip.
#include <cstdint>

#include "det_head.h"

namespace rpn {

using x3_f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using x3_f32x4 = __attribute__((ext_vector_type(4))) float;

// 8 floats -> the 16-byte piece of their hi halves and the piece of their lo halves (x - hi), round-to-nearest-even, unscaled:
// conv_split_kernels.hip's split_piece<true>, both pieces at once.  `status` (may be null) receives RPN_STATUS_F16_RANGE when a
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

// ---- forward GEMM on v_mfma_f32_16x16x32_f16 -----------------------------------------------------------------------------------------
// out (M x N) = act(scale * (A (M x K float32, K contiguous) . W) + bias), W the packed image of det_head.h.
// Workgroup: a 128 x 128 tile, four waves of 64 x 64 = 4 x 4 MFMA blocks of 16 x 16 (sixteen accumulators of 4 registers).  K in
// steps of 32 = one MFMA depth, staged global -> registers -> LDS, double buffered with one barrier per step.
//   A: a thread loads 8 consecutive floats of a row (two float4), splits them (the range probe sits here) and writes the hi piece
//      and the lo piece into the row's 128-byte record -- the layout of the weight image: 8 pieces per row, piece p at slot
//      p ^ (row / 2 % 8).
//   W: the 128 columns of a step are 16 KB contiguous in the image (guarded by column < ld): four 16-byte copies per thread.
//   Fragments (A row / B column = lane % 16, k octet = lane / 16) are single ds_read_b128s; a read is served in groups of sixteen
//   lanes holding sixteen consecutive rows, eight with octet g and eight with g ^ 1, and the XOR puts those on sixteen different
//   16-byte slots of the 256-byte bank row.
// 2 x (16 + 16) KB = 64 KB of LDS: two workgroups per CU.
// Each accumulator takes, per step in k order, lo*hi, hi*lo, hi*hi: the order over K follows from K alone and a row's result reads
// that row of A only.  Rows / columns beyond the matrix and k beyond K enter as zeros; stores are scalar and guarded, columns < split
// to out0, the others to out1.
constexpr int kX3BM = 128, kX3BN = 128, kX3BK = 32;

__global__ void __launch_bounds__(256) fc_forward_x3_kernel(const float *__restrict__ A, const uint4 *__restrict__ Wp,
                                                           const float *__restrict__ bias, int M, int K, int N, int ld, int relu,
                                                           int split, float scale0, float scale1, float *__restrict__ out0,
                                                           float *__restrict__ out1, unsigned *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint4 As[2][kX3BM * 8];
    __shared__ __attribute__((aligned(16))) uint4 Bs[2][kX3BN * 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM;
    const int nsteps = (K + kX3BK - 1) / kX3BK;
    const int ar = tid >> 2, ao = tid & 3;                       // A: rows ar, ar + 64; k octet ao
    float4 ra[2][2];
    uint4 rb[4];
    auto load_global = [&](int step) {
        const int ka = step * kX3BK + 8 * ao;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = m0 + ar + 64 * i;
            ra[i][0] = ra[i][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row < M) {
                const float *src = A + (size_t)row * K + ka;
                if (ka < K) ra[i][0] = *reinterpret_cast<const float4 *>(src);
                if (ka + 4 < K) ra[i][1] = *reinterpret_cast<const float4 *>(src + 4);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, col = n0 + (idx >> 3);
            rb[i] = make_uint4(0u, 0u, 0u, 0u);
            if (col < ld) rb[i] = Wp[((size_t)step * ld + col) * 8 + (idx & 7)];
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float xs[8] = {ra[i][0].x, ra[i][0].y, ra[i][0].z, ra[i][0].w, ra[i][1].x, ra[i][1].y, ra[i][1].z, ra[i][1].w};
            uint4 hi, lo;
            split8_x3(xs, hi, lo, status);
            const int r = ar + 64 * i, sw = (r >> 1) & 7;
            As[buf][r * 8 + (ao ^ sw)] = hi;
            As[buf][r * 8 + ((4 + ao) ^ sw)] = lo;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[buf][tid + 256 * i] = rb[i];
    };
    x3_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

    load_global(0);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global(step + 1);
        uint4 ah[4], al[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wm * 64 + 16 * i + l16, sw = (r >> 1) & 7;
            ah[i] = As[cur][r * 8 + (q ^ sw)];
            al[i] = As[cur][r * 8 + ((4 + q) ^ sw)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = wn * 64 + 16 * j + l16, sw = (c >> 1) & 7;
            const uint4 bh = Bs[cur][c * 8 + (q ^ sw)], bl = Bs[cur][c * 8 + ((4 + q) ^ sw)];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(al[i], bh, acc[i][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(ah[i], bl, acc[i][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x3(ah[i], bh, acc[i][j]);
        }
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator element e of block (i, j): row 16 i + 4 (lane / 16) + e, column 16 j + lane % 16
    const int n1 = N - split;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + 16 * j + l16;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.0f;
        const float sc = col < split ? scale0 : scale1;
        float *dst = col < split ? out0 + col : out1 + (col - split);
        const int ldo = col < split ? split : n1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm * 64 + 16 * i + 4 * q + e;
                if (row < M) {
                    float v = acc[i][j][e] * sc;
                    if (bias) v += bv;
                    if (relu) v = fmaxf(v, 0.0f);
                    dst[(size_t)row * ldo] = v;
                }
            }
    }
}

// one thread per 16-byte piece; the column runs fastest, so a wave reads 64 consecutive floats of each of its 8 rows of w
__global__ void __launch_bounds__(256) fc_pack_x3_kernel(const float *__restrict__ w, int K, int ld, int c0, int ncols, float mul,
                                                        long long total, uint4 *__restrict__ packed)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / ncols;
        const int col = c0 + (int)(i - t * ncols), p = (int)(t & 7);
        const long long chunk = t >> 3;
        const bool lo = p >= 4;
        x3_f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long k = chunk * 32 + 8 * (p & 3) + j;
            const float x = k < K ? w[(size_t)k * ld + col] * mul : 0.0f;
            const _Float16 h = (_Float16)x;
            v[j] = lo ? (_Float16)(x - (float)h) : h;
        }
        packed[((size_t)chunk * ld + col) * 8 + (p ^ ((col >> 1) & 7))] = __builtin_bit_cast(uint4, v);
    }
}

__global__ void __launch_bounds__(256) fc_absmax_kernel(const float *__restrict__ w, long long total, int N, int ld,
                                                       unsigned *__restrict__ out_bits)
{
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long k = i / N;
        const float v = fabsf(w[(size_t)k * ld + (size_t)(i - k * N)]);
        if (v > m) m = v;                                         // (a NaN never compares greater)
    }
    if (m > 0.0f) atomicMax(out_bits, __float_as_uint(m));
}

static int grid_x3(long long items)
{
    const long long g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

hipError_t launch_fc_pack_x3(const float *w, int K, int ld, int c0, int ncols, int shift, void *packed, hipStream_t s)
{
    const long long total = (long long)((K + 31) / 32) * 8 * ncols;
    hipLaunchKernelGGL(fc_pack_x3_kernel, dim3(grid_x3(total)), dim3(256), 0, s, w, K, ld, c0, ncols, ldexpf(1.0f, shift), total,
                       reinterpret_cast<uint4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_fc_absmax(const float *w, int K, int N, int ld, unsigned *out_bits, hipStream_t s)
{
    const long long total = (long long)K * N;
    hipLaunchKernelGGL(fc_absmax_kernel, dim3(grid_x3(total)), dim3(256), 0, s, w, total, N, ld, out_bits);
    return hipGetLastError();
}

hipError_t launch_fc_forward_x3(const float *a, const void *packed, const float *bias, int M, int K, int N, int ld, int relu, int split,
                                float scale0, float scale1, float *out0, float *out1, unsigned *status, hipStream_t s)
{
    hipLaunchKernelGGL(fc_forward_x3_kernel, dim3((N + kX3BN - 1) / kX3BN, (M + kX3BM - 1) / kX3BM), dim3(256), 0, s, a,
                       reinterpret_cast<const uint4 *>(packed), bias, M, K, N, ld, relu, split, scale0, scale1, out0, out1, status);
    return hipGetLastError();
}

}  // namespace rpn
