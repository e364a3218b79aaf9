// det_head_x3_kernels.hip -- the detection head's products in split float16 (RPN_PRECISION_F16X3; contract in include/rpn_hip.h,
// host interface in det_head.h): the forward GEMM on v_mfma_f32_16x16x32_f16, the device-side weight packing and max|.| scan, and
// for a head that TRAINS in split float16 the two backward GEMMs (fc_wgrad_x3_kernel "TN", fc_dgrad_x3_kernel "NT") and the kernel
// that turns maxima into power-of-two scales on the device.  The head object and the ABI live in det_head_kernels.hip; the device
// helpers shared with the backbone's split-float16 backward (split, MFMA wrapper, tile, one reduction step) in x3_tile.h.
#include <cstdint>

#include "det_head.h"
#include "x3_tile.h"

namespace rpn {

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
// the main loop shared by fc_forward_x3_kernel and fc_forward_x3_dropout_kernel: acc <- the workgroup's tile of A . W (unscaled).
// The thread's indices come from the kernel, which needs them again in its epilogue.
__device__ __forceinline__ void fc_forward_x3_mainloop(const float *__restrict__ A, const uint4 *__restrict__ Wp, int M, int K, int ld,
                                                       unsigned *__restrict__ status, const int tid, const int wm, const int wn,
                                                       const int l16, const int q, const int n0, const int m0, x3_f32x4 (&acc)[4][4])
{
    __shared__ __attribute__((aligned(16))) uint4 As[2][kX3BM * 8];
    __shared__ __attribute__((aligned(16))) uint4 Bs[2][kX3BN * 8];
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
}

__global__ void __launch_bounds__(256) fc_forward_x3_kernel(const float *__restrict__ A, const uint4 *__restrict__ Wp,
                                                           const float *__restrict__ bias, int M, int K, int N, int ld, int relu,
                                                           int split, float scale0, float scale1,
                                                           const float *__restrict__ dscale0, const float *__restrict__ dscale1,
                                                           float *__restrict__ out0, float *__restrict__ out1,
                                                           unsigned *__restrict__ status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM;
    x3_f32x4 acc[4][4];
    fc_forward_x3_mainloop(A, Wp, M, K, ld, status, tid, wm, wn, l16, q, n0, m0, acc);
    // accumulator element e of block (i, j): row 16 i + 4 (lane / 16) + e, column 16 j + lane % 16
    // (a training head's scales live in device memory: they follow the weights without a host round trip)
    if (dscale0) scale0 = *dscale0, scale1 = *dscale1;
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

// The same product for a hidden layer of a training head that is dropped (dropout.h; contract in include/rpn_hip.h): out (M x N) =
// keep ? fl32(max(acc * *dscale + bias, 0) * scale) : +0, the 2^-s read from device memory.  Block (i, j)'s four elements are four
// consecutive rows of one column starting at a multiple of 4: one generator evaluation (counter (column, row / 4, layer, t)) per
// block, made inside the store loop.
__global__ void __launch_bounds__(256) fc_forward_x3_dropout_kernel(const float *__restrict__ A, const uint4 *__restrict__ Wp,
                                                                   const float *__restrict__ bias, int M, int K, int N, int ld,
                                                                   const float *__restrict__ dscale, DropoutArgs drop,
                                                                   float *__restrict__ out, unsigned *__restrict__ status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM;
    x3_f32x4 acc[4][4];
    fc_forward_x3_mainloop(A, Wp, M, K, ld, status, tid, wm, wn, l16, q, n0, m0, acc);
    const float sc = *dscale;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + 16 * j + l16;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row0 = m0 + wm * 64 + 16 * i + 4 * q;
            if (row0 >= M) continue;
            const unsigned keep = dropout_keep4(drop, (unsigned)col, (unsigned)row0 >> 2);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (row0 + e < M) {
                    float v = acc[i][j][e] * sc;
                    if (bias) v += bv;
                    out[(size_t)(row0 + e) * N + col] = keep >> e & 1u ? fmaxf(v, 0.0f) * drop.scale : 0.0f;
                }
        }
    }
}

// one thread per 16-byte piece; the column runs fastest, so a wave reads 64 consecutive floats of each of its 8 rows of w
__global__ void __launch_bounds__(256) fc_pack_x3_kernel(const float *__restrict__ w, int K, int ld, int c0, int ncols, float mul,
                                                        const float *__restrict__ dmul, long long total,
                                                        uint4 *__restrict__ packed)
{
    if (dmul) mul = *dmul;                                        // (a training head: 2^shift from device memory)
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

// ---- the backward products of a head trained in split float16 ------------------------------------------------------------------------
// Both keep the forward's tile (128 x 128 x 32, four waves of 4 x 4 MFMA blocks), its LDS records (a row's 32 reduction values as
// four hi and four lo 16-byte pieces, piece p at slot p ^ (row / 2 % 8)), its double buffer with one barrier per step and its order
// inside a step (lo*hi, hi*lo, hi*hi); they differ in how the two operands reach the records.

// scales[2 i] = 2^s, scales[2 i + 1] = 2^-s from the bits of a maximum: s = 12 - e clamped to [lo, hi], max = m 2^e, m in [0.5, 1);
// s = 0 for a maximum of zero.  Entry n (when joint_a >= 0) is taken from the larger of bits[joint_a] and bits[joint_b].
__global__ void __launch_bounds__(64) fc_scales_x3_kernel(const unsigned *__restrict__ bits, int n, int joint_a, int joint_b, int lo, int hi,
                                    float *__restrict__ scales)
{
    const int i = threadIdx.x;
    if (i > n || (i == n && joint_a < 0)) return;
    unsigned b = 0;
    if (i < n) b = bits[i];
    else b = bits[joint_a] > bits[joint_b] ? bits[joint_a] : bits[joint_b];
    int s = 0;
    if (b >= 0x7f800000u) s = lo;                                 // an infinite maximum: the split raises the range flag
    else if (b > 0u) {
        int e = 0;
        (void)frexpf(__uint_as_float(b), &e);
        s = 12 - e;
        s = s < lo ? lo : s > hi ? hi : s;
    }
    scales[2 * i] = ldexpf(1.0f, s);
    scales[2 * i + 1] = ldexpf(1.0f, -s);
}

// "TN": out (K x N, leading dimension ldo) = 2^-t * (A^T (2^t DZ)), A (M x K) and DZ (M x N, leading dimension ldz) float32 with the
// reduction index M STRIDED in both.  Tile rows are columns of A, tile columns are columns of DZ.  Threads 0-127 stage A, 128-255 DZ:
// a thread loads eight rows (one octet of the step's 32) of one column quad as float4s -- 32 lanes read 512 contiguous bytes of a
// row -- and then holds, per column, the 8 reduction-consecutive values of one piece: the transposition happens in registers, the
// split (range probe included) per piece, and the two pieces go to that column's record.  gscale: {2^t, 2^-t} in device memory.
// Rows beyond M enter as zeros (a zero step adds +0 to every accumulator); columns >= N of DZ are read and dropped.
__global__ void __launch_bounds__(256) fc_wgrad_x3_kernel(const float *__restrict__ A, const float *__restrict__ DZ, int M, int K, int N,
                                                         int ldz, int ldo, const float *__restrict__ gscale, float *__restrict__ out,
                                                         unsigned *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint4 S[2][2][kX3BM * 8];     // [buffer][operand][record pieces]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * kX3BN, k0 = blockIdx.y * kX3BM;
    const int nsteps = (M + kX3BK - 1) / kX3BK;
    const int half = tid >> 7, cq = tid & 31, o = (tid >> 5) & 3;          // operand (wave-uniform), column quad, octet of the step
    const float *src = half ? DZ : A;
    const int ld = half ? ldz : K, lim = half ? N : K, c0 = (half ? n0 : k0) + 4 * cq;
    const float mul = half ? gscale[0] : 1.0f;
    float4 r[8];
    auto load_global = [&](int step) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = step * kX3BK + 8 * o + j;
            r[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < M && c0 < ld) r[j] = *reinterpret_cast<const float4 *>(src + (size_t)m * ld + c0);
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float xs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = c == 0 ? r[j].x : c == 1 ? r[j].y : c == 2 ? r[j].z : r[j].w;
                xs[j] = c0 + c < lim ? v * mul : 0.0f;
            }
            uint4 hi, lo;
            split8_x3(xs, hi, lo, status);
            const int row = 4 * cq + c, sw = (row >> 1) & 7;
            S[buf][half][row * 8 + (o ^ sw)] = hi;
            S[buf][half][row * 8 + ((4 + o) ^ sw)] = lo;
        }
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
        x3_mma_step(S[cur][0], S[cur][1], acc, wm, wn, l16, q);
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    const float inv = gscale[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + 16 * j + l16;
        if (col >= N) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = k0 + wm * 64 + 16 * i + 4 * q + e;
                if (row < K) out[(size_t)row * ldo + col] = acc[i][j][e] * inv;
            }
    }
}

// "NT": out (M x K) = 2^-(t + s) ((2^t DZ) (2^s W)^T) [h > 0], DZ (M x N, leading dimension ldz) and W (K x N, leading dimension
// ldw) float32 with the reduction index N CONTIGUOUS in both: either operand is staged as the forward stages its A -- a thread loads
// 8 consecutive floats of a row, splits them and writes the two pieces -- W from the master weights, no transposed image.  The range
// probe sits on DZ.  Columns >= N of both are read (inside ld) and dropped.  gscale {2^t, 2^-t}, wscale {2^s, 2^-s}: device memory.
// A row's result reads that row of DZ, W and the two scales only.
// the main loop shared by fc_dgrad_x3_kernel and fc_dgrad_x3_dropout_kernel: acc <- the workgroup's tile of (2^t DZ) (2^s W)^T
__device__ __forceinline__ void fc_dgrad_x3_mainloop(const float *__restrict__ DZ, const float *__restrict__ W, int M, int K, int N,
                                                     int ldz, int ldw, const float *__restrict__ gscale,
                                                     const float *__restrict__ wscale, unsigned *__restrict__ status, const int tid,
                                                     const int wm, const int wn, const int l16, const int q, const int k0,
                                                     const int m0, x3_f32x4 (&acc)[4][4])
{
    __shared__ __attribute__((aligned(16))) uint4 S[2][2][kX3BM * 8];
    const int nsteps = (N + kX3BK - 1) / kX3BK;
    const int ar = tid >> 2, ao = tid & 3;                       // rows ar, ar + 64 of either operand; octet ao of the step
    const float gmul = gscale[0], wmul = wscale[0];
    float4 ra[2][2], rb[2][2];
    auto load_global = [&](int step) {
        const int n = step * kX3BK + 8 * ao;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[i][0] = ra[i][1] = rb[i][0] = rb[i][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int row = m0 + ar + 64 * i, wrow = k0 + ar + 64 * i;
            if (row < M) {
                const float *p = DZ + (size_t)row * ldz + n;
                if (n < ldz) ra[i][0] = *reinterpret_cast<const float4 *>(p);
                if (n + 4 < ldz) ra[i][1] = *reinterpret_cast<const float4 *>(p + 4);
            }
            if (wrow < K) {
                const float *p = W + (size_t)wrow * ldw + n;
                if (n < ldw) rb[i][0] = *reinterpret_cast<const float4 *>(p);
                if (n + 4 < ldw) rb[i][1] = *reinterpret_cast<const float4 *>(p + 4);
            }
        }
    };
    auto store_lds = [&](int buf, int step) {
        const int n = step * kX3BK + 8 * ao;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float va[8] = {ra[i][0].x, ra[i][0].y, ra[i][0].z, ra[i][0].w, ra[i][1].x, ra[i][1].y, ra[i][1].z, ra[i][1].w};
            const float vb[8] = {rb[i][0].x, rb[i][0].y, rb[i][0].z, rb[i][0].w, rb[i][1].x, rb[i][1].y, rb[i][1].z, rb[i][1].w};
            float xa[8], xb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                xa[k] = n + k < N ? va[k] * gmul : 0.0f;
                xb[k] = n + k < N ? vb[k] * wmul : 0.0f;
            }
            uint4 hi, lo;
            const int r = ar + 64 * i, sw = (r >> 1) & 7;
            split8_x3(xa, hi, lo, status);
            S[buf][0][r * 8 + (ao ^ sw)] = hi;
            S[buf][0][r * 8 + ((4 + ao) ^ sw)] = lo;
            split8_x3(xb, hi, lo, nullptr);
            S[buf][1][r * 8 + (ao ^ sw)] = hi;
            S[buf][1][r * 8 + ((4 + ao) ^ sw)] = lo;
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

    load_global(0);
    store_lds(0, 0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global(step + 1);
        x3_mma_step(S[cur][0], S[cur][1], acc, wm, wn, l16, q);
        if (more) store_lds(cur ^ 1, step + 1);
        __syncthreads();
        cur ^= 1;
    }
}

__global__ void __launch_bounds__(256) fc_dgrad_x3_kernel(const float *__restrict__ DZ, const float *__restrict__ W,
                                                         const float *__restrict__ H, int M, int K, int N, int ldz, int ldw,
                                                         const float *__restrict__ gscale, const float *__restrict__ wscale,
                                                         float *__restrict__ out, unsigned *__restrict__ status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int k0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM;
    x3_f32x4 acc[4][4];
    fc_dgrad_x3_mainloop(DZ, W, M, K, N, ldz, ldw, gscale, wscale, status, tid, wm, wn, l16, q, k0, m0, acc);
    // acc * 2^-(t + s) as two exact multiplications (x3_unscale_factors, x3_tile.h)
    float f1, f2;
    x3_unscale_factors(gscale[1], wscale[1], f1, f2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = k0 + wn * 64 + 16 * j + l16;
        if (col >= K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm * 64 + 16 * i + 4 * q + e;
                if (row < M) {
                    float v = acc[i][j][e] * f1 * f2;
                    if (H) v = H[(size_t)row * K + col] > 0.0f ? v : 0.0f;
                    out[(size_t)row * K + col] = v;
                }
            }
    }
}

// the input gradient of a DROPPED layer: out = H > 0 ? fl32(acc f1 f2 * scale) : 0, H the stored (dropped, scaled) activation -- the
// factor 1 / (1 - rate) after the two exact powers of two; no generator runs here
__global__ void __launch_bounds__(256) fc_dgrad_x3_dropout_kernel(const float *__restrict__ DZ, const float *__restrict__ W,
                                                                 const float *__restrict__ H, int M, int K, int N, int ldz, int ldw,
                                                                 const float *__restrict__ gscale, const float *__restrict__ wscale,
                                                                 float scale, float *__restrict__ out, unsigned *__restrict__ status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int k0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM;
    x3_f32x4 acc[4][4];
    fc_dgrad_x3_mainloop(DZ, W, M, K, N, ldz, ldw, gscale, wscale, status, tid, wm, wn, l16, q, k0, m0, acc);
    // acc * 2^-(t + s) as two exact multiplications (x3_unscale_factors, x3_tile.h)
    float f1, f2;
    x3_unscale_factors(gscale[1], wscale[1], f1, f2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = k0 + wn * 64 + 16 * j + l16;
        if (col >= K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm * 64 + 16 * i + 4 * q + e;
                if (row < M) out[(size_t)row * K + col] = H[(size_t)row * K + col] > 0.0f ? acc[i][j][e] * f1 * f2 * scale : 0.0f;
            }
    }
}

static int grid_x3(long long items)
{
    const long long g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

hipError_t launch_fc_pack_x3(const float *w, int K, int ld, int c0, int ncols, int shift, void *packed, hipStream_t s, const float *dmul)
{
    const long long total = (long long)((K + 31) / 32) * 8 * ncols;
    hipLaunchKernelGGL(fc_pack_x3_kernel, dim3(grid_x3(total)), dim3(256), 0, s, w, K, ld, c0, ncols, ldexpf(1.0f, shift), dmul, total,
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
                                float scale0, float scale1, float *out0, float *out1, unsigned *status, hipStream_t s,
                                const float *dscale0, const float *dscale1)
{
    hipLaunchKernelGGL(fc_forward_x3_kernel, dim3((N + kX3BN - 1) / kX3BN, (M + kX3BM - 1) / kX3BM), dim3(256), 0, s, a,
                       reinterpret_cast<const uint4 *>(packed), bias, M, K, N, ld, relu, split, scale0, scale1, dscale0, dscale1, out0, out1,
                       status);
    return hipGetLastError();
}

hipError_t launch_fc_scales_x3(const unsigned *bits, int n, int joint_a, int joint_b, bool gradient, float *scales, hipStream_t s)
{
    hipLaunchKernelGGL(fc_scales_x3_kernel, dim3(1), dim3(64), 0, s, bits, n, joint_a, joint_b, gradient ? -116 : -100, gradient ? 100 : 24,
                       scales);
    return hipGetLastError();
}

hipError_t launch_fc_wgrad_x3(const float *a, const float *dz, int M, int K, int N, int ldz, int ldo, const float *gscale, float *out,
                              unsigned *status, hipStream_t s)
{
    hipLaunchKernelGGL(fc_wgrad_x3_kernel, dim3((N + kX3BN - 1) / kX3BN, (K + kX3BM - 1) / kX3BM), dim3(256), 0, s, a, dz, M, K, N, ldz, ldo,
                       gscale, out, status);
    return hipGetLastError();
}

hipError_t launch_fc_dgrad_x3(const float *dz, const float *w, const float *h, int M, int K, int N, int ldz, int ldw, const float *gscale,
                              const float *wscale, float *out, unsigned *status, hipStream_t s)
{
    hipLaunchKernelGGL(fc_dgrad_x3_kernel, dim3((K + kX3BN - 1) / kX3BN, (M + kX3BM - 1) / kX3BM), dim3(256), 0, s, dz, w, h, M, K, N, ldz,
                       ldw, gscale, wscale, out, status);
    return hipGetLastError();
}

hipError_t launch_fc_forward_x3_dropout(const float *a, const void *packed, const float *bias, int M, int K, int N, int ld,
                                        const float *dscale, const DropoutArgs &drop, float *out, unsigned *status, hipStream_t s)
{
    hipLaunchKernelGGL(fc_forward_x3_dropout_kernel, dim3((N + kX3BN - 1) / kX3BN, (M + kX3BM - 1) / kX3BM), dim3(256), 0, s, a,
                       reinterpret_cast<const uint4 *>(packed), bias, M, K, N, ld, dscale, drop, out, status);
    return hipGetLastError();
}

hipError_t launch_fc_dgrad_x3_dropout(const float *dz, const float *w, const float *h, int M, int K, int N, int ldz, int ldw,
                                      const float *gscale, const float *wscale, float scale, float *out, unsigned *status, hipStream_t s)
{
    hipLaunchKernelGGL(fc_dgrad_x3_dropout_kernel, dim3((K + kX3BN - 1) / kX3BN, (M + kX3BM - 1) / kX3BM), dim3(256), 0, s, dz, w, h, M, K,
                       N, ldz, ldw, gscale, wscale, scale, out, status);
    return hipGetLastError();
}

}  // namespace rpn
