// train_mnv2_kernels.hip -- backward of MobileNetV2 (Conv1, expanded_conv, block_1 .. block_12, block_13_expand): BatchNorm in
// training mode, the 1x1 convs on the float32 MFMA, the depthwise 3x3 convs (stride 1 'same'; stride 2 behind Keras' correct_pad) and
// the stem's weight gradient.  The trainer that strings them together is in trainer.hip (mn_forward / mn_backward).  tree_sum32, the
// lane-sum epilogue of the per-channel weight gradients (lane_sum_store) and the helpers shared with the other training kernel files
// are in train_common.h.
//
// BatchNorm form (TF 2.0's fused BatchNorm, restated as recalled -- nothing here can run TF): over the N = B H W pixels of a channel,
//   mean = sum x / N, var = sum (x - mean)^2 / N (biased), xhat = (x - mean) / sqrt(var + eps), y = gamma xhat + beta;
//   moving_mean = moving_mean * momentum + mean * (1 - momentum), moving_var likewise with var N / (N - 1) (Bessel);
//   backward: dbeta = sum dy, dgamma = sum dy xhat, dx = gamma / sqrt(var + eps) (dy - dbeta / N - xhat dgamma / N).
// Keras MobileNetV2: eps 1e-3, momentum 0.999.  The ReLU6 that follows is fused: forward min(max(y, 0), 6), backward dy [0 < y < 6]
// (TF's Relu6Grad, strict on both sides), y recomputed from the kept conv output by the very expression of the forward.
//
// Reductions: the pixels are cut into a power-of-two number of leaves chosen from the shape alone; a leaf is summed in a fixed order
// (16 row lanes per workgroup, each over its rows in order, then the lanes in order), the leaves in a fixed tree.  The BatchNorm sums
// are carried in float64 (sum and sum of squares: var = E[x^2] - mean^2 is formed in float64, where a channel of mean 100 and spread
// 0.1 still keeps 10 significant digits).  No floating-point atomics, no scratch memory.
#include <algorithm>
#include <cstdint>

#include "rpn_common.h"
#include "train_common.h"
#include "train_mnv2.h"

namespace rpn {

constexpr int kRedQuads = 16, kRedLanes = 16;   // a reduction workgroup: 16 channel quads x 16 row lanes
constexpr int kGridCap = 4096;                  // workgroups of this file's grid-stride kernels

int mn_reduce_leaves(long long P)
{
    int L = 1;
    while (L < kMaxLeaves && P / (2 * L) >= 16) L *= 2;
    return L;
}

__device__ inline float bn_rstd_of(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }
// the forward's value of one element: xhat, then y before the activation
__device__ inline float bn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ inline float bn_y(float xhat, float gamma, float beta) { return fmaf(xhat, gamma, beta); }

// ---- BatchNorm statistics ------------------------------------------------------------------------------------------------------
// part[leaf][0][C] = sum x, part[leaf][1][C] = sum x^2 over the leaf's pixels, float64.  grid (ceil(C / 64), leaves).
__global__ void __launch_bounds__(256) bn_stats_partial_kernel(const float *__restrict__ x, long long P, int C, int leaves,
                                                              double *__restrict__ part)
{
    __shared__ double red[kRedLanes][2 * kRedQuads * 4];
    const int q = threadIdx.x & (kRedQuads - 1), rl = threadIdx.x / kRedQuads;
    const int C4 = C / 4, cq = blockIdx.x * kRedQuads + q, leaf = blockIdx.y;
    const long long pbeg = P * leaf / leaves, pend = P * (leaf + 1) / leaves;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
    if (cq < C4) {
        for (long long p = pbeg + rl; p < pend; p += kRedLanes) {
            const float4 v = reinterpret_cast<const float4 *>(x)[p * C4 + cq];
            const double d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[j] += d[j];
                ss[j] = fma(d[j], d[j], ss[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[rl][4 * q + j] = s[j];
        red[rl][kRedQuads * 4 + 4 * q + j] = ss[j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * kRedQuads * 4) {
        const int which = threadIdx.x / (kRedQuads * 4), ch = blockIdx.x * kRedQuads * 4 + (threadIdx.x % (kRedQuads * 4));
        double a = 0.0;
        for (int r = 0; r < kRedLanes; ++r) a += red[r][threadIdx.x];
        if (ch < C) part[((size_t)leaf * 2 + which) * C + ch] = a;
    }
}

__global__ void __launch_bounds__(256) bn_stats_finish_kernel(const double *__restrict__ part, int leaves, int C, long long P, float eps,
                                                             float momentum, float *__restrict__ mean, float *__restrict__ var,
                                                             float *__restrict__ rstd, float *__restrict__ mmean, float *__restrict__ mvar)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double s = tree_sum32<double>(part + c, (size_t)2 * C, leaves);
    const double ss = tree_sum32<double>(part + C + c, (size_t)2 * C, leaves);
    const double n = (double)P, m = s / n, v = fmax(0.0, ss / n - m * m);
    const float mf = (float)m, vf = (float)v;
    mean[c] = mf;
    var[c] = vf;
    rstd[c] = bn_rstd_of(vf, eps);
    if (mmean) {
        const float unbiased = (float)(P > 1 ? v * n / (n - 1.0) : v);
        mmean[c] = mmean[c] * momentum + mf * (1.0f - momentum);
        mvar[c] = mvar[c] * momentum + unbiased * (1.0f - momentum);
    }
}

__global__ void __launch_bounds__(256) bn_rstd_kernel(const float *__restrict__ var, int C, float eps, float *__restrict__ rstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) rstd[c] = bn_rstd_of(var[c], eps);
}

// ---- BatchNorm apply (+ ReLU6, + residual): one pass, a float4 of channels per lane ------------------------------------------
__global__ void __launch_bounds__(256) bn_apply_kernel(const float4 *__restrict__ x, long long total4, int C4, const float4 *__restrict__ mean,
                                                      const float4 *__restrict__ rstd, const float4 *__restrict__ gamma,
                                                      const float4 *__restrict__ beta, int relu6, const float4 *__restrict__ res,
                                                      float4 *__restrict__ y)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const float4 v = x[i], m = mean[c], r = rstd[c], g = gamma[c], b = beta[c];
        float o[4] = {bn_y(bn_xhat(v.x, m.x, r.x), g.x, b.x), bn_y(bn_xhat(v.y, m.y, r.y), g.y, b.y),
                      bn_y(bn_xhat(v.z, m.z, r.z), g.z, b.z), bn_y(bn_xhat(v.w, m.w, r.w), g.w, b.w)};
        if (relu6) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(o[j], 0.0f), 6.0f);
        }
        if (res) {
            const float4 e = res[i];
            o[0] += e.x; o[1] += e.y; o[2] += e.z; o[3] += e.w;
        }
        y[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- BatchNorm backward, pass 1: part[leaf][0][C] = sum dy', part[leaf][1][C] = sum dy' xhat (float64) ------------------------
__global__ void __launch_bounds__(256) bn_bwd_partial_kernel(const float *__restrict__ x, const float *__restrict__ dy, long long P, int C,
                                                            const float4 *__restrict__ mean, const float4 *__restrict__ rstd,
                                                            const float4 *__restrict__ gamma, const float4 *__restrict__ beta, int relu6,
                                                            int leaves, double *__restrict__ part)
{
    __shared__ double red[kRedLanes][2 * kRedQuads * 4];
    const int q = threadIdx.x & (kRedQuads - 1), rl = threadIdx.x / kRedQuads;
    const int C4 = C / 4, cq = blockIdx.x * kRedQuads + q, leaf = blockIdx.y;
    const long long pbeg = P * leaf / leaves, pend = P * (leaf + 1) / leaves;
    double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
    if (cq < C4) {
        const float4 m4 = mean[cq], r4 = rstd[cq], g4 = gamma[cq], b4 = beta[cq];
        const float m[4] = {m4.x, m4.y, m4.z, m4.w}, r[4] = {r4.x, r4.y, r4.z, r4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w},
                    b[4] = {b4.x, b4.y, b4.z, b4.w};
        for (long long p = pbeg + rl; p < pend; p += kRedLanes) {
            const float4 v4 = reinterpret_cast<const float4 *>(x)[p * C4 + cq], d4 = reinterpret_cast<const float4 *>(dy)[p * C4 + cq];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = bn_xhat(v[j], m[j], r[j]), yv = bn_y(xh, g[j], b[j]);
                const float dj = (!relu6 || (yv > 0.0f && yv < 6.0f)) ? d[j] : 0.0f;
                sb[j] += (double)dj;
                sg[j] = fma((double)dj, (double)xh, sg[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[rl][4 * q + j] = sb[j];
        red[rl][kRedQuads * 4 + 4 * q + j] = sg[j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * kRedQuads * 4) {
        const int which = threadIdx.x / (kRedQuads * 4), ch = blockIdx.x * kRedQuads * 4 + (threadIdx.x % (kRedQuads * 4));
        double a = 0.0;
        for (int r = 0; r < kRedLanes; ++r) a += red[r][threadIdx.x];
        if (ch < C) part[((size_t)leaf * 2 + which) * C + ch] = a;
    }
}

__global__ void __launch_bounds__(256) bn_bwd_finish_kernel(const double *__restrict__ part, int leaves, int C, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    dbeta[c] = (float)tree_sum32<double>(part + c, (size_t)2 * C, leaves);
    dgamma[c] = (float)tree_sum32<double>(part + C + c, (size_t)2 * C, leaves);
}

// ---- BatchNorm backward, pass 2: dx = gamma rstd (dy' - dbeta / N - xhat dgamma / N) -------------------------------------------
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float4 *__restrict__ x, const float4 *dy, long long total4, int C4,
                                                          const float4 *__restrict__ mean, const float4 *__restrict__ rstd,
                                                          const float4 *__restrict__ gamma, const float4 *__restrict__ beta,
                                                          const float4 *__restrict__ dgamma, const float4 *__restrict__ dbeta, float inv_n,
                                                          int relu6, float4 *dx)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const float4 v4 = x[i], d4 = dy[i], m4 = mean[c], r4 = rstd[c], g4 = gamma[c], b4 = beta[c], dg4 = dgamma[c], db4 = dbeta[c];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w},
                    r[4] = {r4.x, r4.y, r4.z, r4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w},
                    dg[4] = {dg4.x, dg4.y, dg4.z, dg4.w}, db[4] = {db4.x, db4.y, db4.z, db4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = bn_xhat(v[j], m[j], r[j]), yv = bn_y(xh, g[j], b[j]);
            const float dj = (!relu6 || (yv > 0.0f && yv < 6.0f)) ? d[j] : 0.0f;
            o[j] = g[j] * r[j] * (dj - db[j] * inv_n - xh * (dg[j] * inv_n));
        }
        dx[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

size_t bn_part_doubles(long long P, int C) { return (size_t)mn_reduce_leaves(P) * 2 * C; }

hipError_t launch_bn_train_stats(const float *x, long long P, int C, float eps, float momentum, double *part, float *mean, float *var,
                                 float *rstd, float *mmean, float *mvar, hipStream_t s)
{
    const int leaves = mn_reduce_leaves(P);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((C + 63) / 64, leaves), dim3(256), 0, s, x, P, C, leaves, part);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, leaves, C, P, eps, momentum, mean, var, rstd,
                       mmean, mvar);
    return hipGetLastError();
}

hipError_t launch_bn_rstd(const float *var, int C, float eps, float *rstd, hipStream_t s)
{
    hipLaunchKernelGGL(bn_rstd_kernel, dim3((C + 255) / 256), dim3(256), 0, s, var, C, eps, rstd);
    return hipGetLastError();
}

hipError_t launch_bn_apply(const float *x, long long P, int C, const float *mean, const float *rstd, const float *gamma,
                           const float *beta, int relu6, const float *res, float *y, hipStream_t s)
{
    const long long total4 = P * (C / 4);
    auto f4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_1d(total4, kGridCap)), dim3(256), 0, s, f4(x), total4, C / 4, f4(mean), f4(rstd), f4(gamma),
                       f4(beta), relu6, f4(res), reinterpret_cast<float4 *>(y));
    return hipGetLastError();
}

hipError_t launch_bn_backward(const float *x, const float *dy, long long P, int C, const float *mean, const float *rstd,
                              const float *gamma, const float *beta, int relu6, double *part, float *dgamma, float *dbeta, float *dx,
                              hipStream_t s)
{
    const int leaves = mn_reduce_leaves(P);
    const long long total4 = P * (C / 4);
    auto f4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((C + 63) / 64, leaves), dim3(256), 0, s, x, dy, P, C, f4(mean), f4(rstd), f4(gamma),
                       f4(beta), relu6, leaves, part);
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, leaves, C, dgamma, dbeta);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_1d(total4, kGridCap)), dim3(256), 0, s, f4(x), f4(dy), total4, C / 4, f4(mean), f4(rstd),
                       f4(gamma), f4(beta), f4(dgamma), f4(dbeta), (float)(1.0 / (double)P), relu6, reinterpret_cast<float4 *>(dx));
    return hipGetLastError();
}

// ---- 1x1 conv backward: one GEMM kernel on v_mfma_f32_32x32x2_f32 -------------------------------------------------------------------
// C (M x N) = sum_k A(m, k) B(k, n) over k in leaf blockIdx.z of `leaves` fixed ranges of K.
//   KCONTIG = false (weight gradient: A = x (P, Cin), B = dy (P, Cout), K = the pixels): A[k][m], B[k][n], a K slice of either is a
//     contiguous run of channels per pixel;
//   KCONTIG = true (input gradient: A = dy (P, Cout), B = w (Cin, Cout), K = Cout): A[m][k], B[n][k], rows run along K and are
//     transposed on their way into LDS.
// Workgroup: a 64 x 64 tile, four waves of 32 x 32 (one MFMA block each); K slices of 16 staged global -> registers -> LDS, double
// buffered with one barrier per slice, as conv3x3_wgrad_f32_kernel stages its operands.  Each leaf writes its own slab of `out`
// (out + leaf M N); `add` (M x N, leaves == 1 only) is added in the epilogue.  M, N, the row lengths and K (KCONTIG) are multiples of 4.
constexpr int kGmT = 64, kGmK = 16, kGmLd = 96;   // LDS row stride 96: the two half-waves of a fragment read hit disjoint banks

template <bool KCONTIG>
__global__ void __launch_bounds__(256) gemm1x1_f32_kernel(const float *__restrict__ A, const float *__restrict__ Bm, int M, int N, long long K,
                                                         int lda, int ldb, int leaves, const float *__restrict__ add, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float As[2][kGmK][kGmLd];
    __shared__ __attribute__((aligned(16))) float Bs[2][kGmK][kGmLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * kGmT, m0 = blockIdx.y * kGmT, leaf = blockIdx.z;
    const long long kbeg = K * leaf / leaves, kend = K * (leaf + 1) / leaves;
    const int nsteps = (int)((kend - kbeg + kGmK - 1) / kGmK);
    // loader.  !KCONTIG: thread -> (K row kr of the slice, channel quad q).  KCONTIG: thread -> (tile row r, K quad kq)
    const int kr = tid >> 4, q = tid & 15, r = tid >> 2, kq = tid & 3;
    float4 ra, rb;
    auto load_global = [&](long long k0) {
        ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!KCONTIG) {
            const long long k = k0 + kr;
            if (k < kend) {
                if (m0 + 4 * q < M) ra = *reinterpret_cast<const float4 *>(A + (size_t)k * lda + m0 + 4 * q);
                if (n0 + 4 * q < N) rb = *reinterpret_cast<const float4 *>(Bm + (size_t)k * ldb + n0 + 4 * q);
            }
        } else {
            const long long k = k0 + 4 * kq;
            if (k < kend) {
                if (m0 + r < M) ra = *reinterpret_cast<const float4 *>(A + (size_t)(m0 + r) * lda + k);
                if (n0 + r < N) rb = *reinterpret_cast<const float4 *>(Bm + (size_t)(n0 + r) * ldb + k);
            }
        }
    };
    auto store_lds = [&](int buf) {
        if (!KCONTIG) {
            *reinterpret_cast<float4 *>(&As[buf][kr][4 * q]) = ra;
            *reinterpret_cast<float4 *>(&Bs[buf][kr][4 * q]) = rb;
        } else {
            As[buf][4 * kq + 0][r] = ra.x; As[buf][4 * kq + 1][r] = ra.y; As[buf][4 * kq + 2][r] = ra.z; As[buf][4 * kq + 3][r] = ra.w;
            Bs[buf][4 * kq + 0][r] = rb.x; Bs[buf][4 * kq + 1][r] = rb.y; Bs[buf][4 * kq + 2][r] = rb.z; Bs[buf][4 * kq + 3][r] = rb.w;
        }
    };
    f32x16t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const int am = wm * 32 + (lane & 31), bn = wn * 32 + (lane & 31), kh = lane >> 5;

    load_global(kbeg);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global(kbeg + (long long)(step + 1) * kGmK);
#pragma unroll
        for (int kk = 0; kk < kGmK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[cur][2 * kk + kh][am], Bs[cur][2 * kk + kh][bn], acc, 0, 0, 0);
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator element e: row 8 (e / 4) + 4 kh + e % 4, column lane % 32
    const int col = n0 + bn;
    if (col >= N) return;
    float *slab = out + (size_t)leaf * M * N;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 32 + 8 * (e >> 2) + 4 * kh + (e & 3);
        if (row < M) {
            const size_t o = (size_t)row * N + col;
            slab[o] = add ? acc[e] + add[o] : acc[e];
        }
    }
}

// out[j] = the fixed tree over the `leaves` (a power of two <= 32 GROUPS) slabs of len floats: tree_sum32 over each group of 32, then
// the groups pairwise, neighbours first: ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)) at GROUPS = 8 (an absent group is a
// zero).  GROUPS = 1 is tree_sum32 alone -- the 32-leaf reductions must not run through a wider form: adding the absent groups'
// zeros would turn a sum of -0.0 into +0.0.
template <int GROUPS>
__global__ void __launch_bounds__(256) slab_tree_kernel(const float *__restrict__ part, long long len, int leaves, float *__restrict__ out)
{
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < len; j += (long long)gridDim.x * 256) {
        float v[GROUPS];
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int n = leaves - g * kMaxLeaves;
            v[g] = n > 0 ? tree_sum32<float>(part + (size_t)g * kMaxLeaves * len + j, (size_t)len, n < kMaxLeaves ? n : kMaxLeaves) : 0.0f;
        }
#pragma unroll
        for (int n = GROUPS; n > 1; n >>= 1)
#pragma unroll
            for (int i = 0; i < n / 2; ++i) v[i] = v[2 * i] + v[2 * i + 1];
        out[j] = v[0];
    }
}

int conv1x1_wgrad_leaves(long long P, int Cin, int Cout)
{
    const long long tiles = (long long)((Cin + kGmT - 1) / kGmT) * ((Cout + kGmT - 1) / kGmT);
    int L = 1;
    while (L < kMaxLeaves && P / (2 * L) >= 64 && tiles * L < 512) L *= 2;
    return L;
}

size_t conv1x1_wgrad_ws_floats(long long P, int Cin, int Cout)
{
    const int L = conv1x1_wgrad_leaves(P, Cin, Cout);
    return L > 1 ? (size_t)L * Cin * Cout : 0;
}

hipError_t launch_conv1x1_wgrad(const float *x, const float *dy, long long P, int Cin, int Cout, float *part, float *dw, hipStream_t s)
{
    const int L = conv1x1_wgrad_leaves(P, Cin, Cout);
    hipLaunchKernelGGL(gemm1x1_f32_kernel<false>, dim3((Cout + kGmT - 1) / kGmT, (Cin + kGmT - 1) / kGmT, L), dim3(256), 0, s, x, dy, Cin, Cout,
                       P, Cin, Cout, L, (const float *)nullptr, L > 1 ? part : dw);
    if (L > 1) {
        const long long len = (long long)Cin * Cout;
        hipLaunchKernelGGL(slab_tree_kernel<1>, dim3(grid_1d(len, kGridCap)), dim3(256), 0, s, part, len, L, dw);
    }
    return hipGetLastError();
}

hipError_t launch_conv1x1_dgrad(const float *dy, const float *w, const float *add, long long P, int Cin, int Cout, float *dx,
                                hipStream_t s)
{
    hipLaunchKernelGGL(gemm1x1_f32_kernel<true>, dim3((Cin + kGmT - 1) / kGmT, (unsigned)((P + kGmT - 1) / kGmT), 1), dim3(256), 0, s, dy, w,
                       (int)P, Cin, (long long)Cout, Cout, Cout, 1, add, dx);
    return hipGetLastError();
}

// ---- depthwise 3x3 backward, stride 1 ('same') and stride 2 (block_1, block_3, block_6 and block_13's depthwise; Keras
// ZeroPadding2D(correct_pad) + 'valid') --------------------------------------------------------------------------------------------------
// The forward reads x[STRIDE oy + r - pt][STRIDE ox + s - pl] for output (oy, ox).  Stride 1 is pt = pl = 1, OH = H, OW = W (folded in
// at compile time); stride 2 has pt = H % 2, pl = W % 2 (mn_s2_geom).
// dgrad: input pixel (y, x) is read by output ((y + pt - r) / STRIDE, (x + pl - s) / STRIDE) where both are exact and in range: the
// depthwise conv of dy with the taps flipped at stride 1, at most 2 x 2 taps at stride 2.  Every dx element is written once (pixels
// no output reads get zeros); a float4 of channels per lane, as dwconv3x3_kernel.
template <int STRIDE>
__global__ void __launch_bounds__(256) dwconv3x3_dgrad_kernel(const float4 *__restrict__ dy, const float4 *__restrict__ w, int H, int W,
                                                             int OH_, int OW_, int pt_, int pl_, int C4, long long total,
                                                             float4 *__restrict__ dx)
{
    const int OH = STRIDE == 1 ? H : OH_, OW = STRIDE == 1 ? W : OW_, pt = STRIDE == 1 ? 1 : pt_, pl = STRIDE == 1 ? 1 : pl_;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        long long t = i / C4;
        const int ix = (int)(t % W);
        t /= W;
        const int iy = (int)(t % H);
        const long long b = t / H;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ny = iy + pt - r;
            if (ny < 0 || (STRIDE == 2 && (ny & 1)) || ny / STRIDE >= OH) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int nx = ix + pl - s;
                if (nx < 0 || (STRIDE == 2 && (nx & 1)) || nx / STRIDE >= OW) continue;
                const float4 v = dy[((b * OH + ny / STRIDE) * OW + nx / STRIDE) * C4 + c];
                const float4 k = w[(r * 3 + s) * C4 + c];
                acc.x = fmaf(v.x, k.x, acc.x);
                acc.y = fmaf(v.y, k.y, acc.y);
                acc.z = fmaf(v.z, k.z, acc.z);
                acc.w = fmaf(v.w, k.w, acc.w);
            }
        }
        dx[i] = acc;
    }
}

// wgrad: part[leaf][9][C] = the nine per-channel sums over the leaf's OUTPUT pixels.  grid (ceil(C / (4 QUADS)), leaves); a workgroup
// is QUADS channel quads x LANES pixel lanes: 16 x 16 at stride 1; 8 x 32 at stride 2 (those layers have 96 .. 576 channels and up to
// 125 000 output pixels: narrower channel tiles give the grid three times the workgroups of the 64-channel tile at the same leaf
// count).  The nine taps of a lane's four channels stay in registers; a lane takes its pixels in order, and a leaf is summed lane by
// lane in order (lane_sum_store).
constexpr int kS2Quads = 8, kS2Lanes = 32;

template <int STRIDE, int QUADS, int LANES>
__global__ void __launch_bounds__(256) dwconv3x3_wgrad_partial_kernel(const float4 *__restrict__ x, const float4 *__restrict__ dy, int B,
                                                                     int H, int W, int OH_, int OW_, int pt_, int pl_, int C, int leaves,
                                                                     float *__restrict__ part)
{
    static_assert(QUADS * LANES == 256, "a workgroup of 256 threads");
    __shared__ float red[LANES][9 * QUADS * 4];
    const int OH = STRIDE == 1 ? H : OH_, OW = STRIDE == 1 ? W : OW_, pt = STRIDE == 1 ? 1 : pt_, pl = STRIDE == 1 ? 1 : pl_;
    const int q = threadIdx.x & (QUADS - 1), rl = threadIdx.x / QUADS;
    const int C4 = C / 4, cq = blockIdx.x * QUADS + q, leaf = blockIdx.y;
    const long long P = (long long)B * OH * OW, pbeg = P * leaf / leaves, pend = P * (leaf + 1) / leaves;
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cq < C4) {
        for (long long p = pbeg + rl; p < pend; p += LANES) {
            const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
            const long long b = p / ((long long)OW * OH);
            const float4 d = dy[p * C4 + cq];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int iy = STRIDE * oy + r - pt;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int ix = STRIDE * ox + s - pl;
                    if (ix < 0 || ix >= W) continue;
                    const float4 v = x[((b * H + iy) * W + ix) * C4 + cq];
                    float4 &a = acc[r * 3 + s];
                    a.x = fmaf(v.x, d.x, a.x);
                    a.y = fmaf(v.y, d.y, a.y);
                    a.z = fmaf(v.z, d.z, a.z);
                    a.w = fmaf(v.w, d.w, a.w);
                }
            }
        }
    }
    lane_sum_store<QUADS, LANES>(red, acc, q, rl, blockIdx.x, C, part + (size_t)leaf * 9 * C);
}

hipError_t launch_dwconv3x3_dgrad(const float *dy, const float *w, int B, int H, int W, int C, float *dx, hipStream_t s)
{
    const long long total = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(dwconv3x3_dgrad_kernel<1>, dim3(grid_1d(total, kGridCap)), dim3(256), 0, s, reinterpret_cast<const float4 *>(dy),
                       reinterpret_cast<const float4 *>(w), H, W, H, W, 1, 1, C / 4, total, reinterpret_cast<float4 *>(dx));
    return hipGetLastError();
}

size_t dwconv3x3_wgrad_ws_floats(long long P, int C) { return (size_t)mn_reduce_leaves(P) * 9 * C; }

hipError_t launch_dwconv3x3_wgrad(const float *x, const float *dy, int B, int H, int W, int C, float *part, float *dw, hipStream_t s)
{
    const int leaves = mn_reduce_leaves((long long)B * H * W);
    hipLaunchKernelGGL((dwconv3x3_wgrad_partial_kernel<1, kRedQuads, kRedLanes>), dim3((C + 63) / 64, leaves), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(x), reinterpret_cast<const float4 *>(dy), B, H, W, H, W, 1, 1, C, leaves, part);
    hipLaunchKernelGGL(slab_tree_kernel<1>, dim3(grid_1d(9LL * C, kGridCap)), dim3(256), 0, s, part, 9LL * C, leaves, dw);
    return hipGetLastError();
}

hipError_t launch_dwconv3x3_s2_dgrad(const float *dy, const float *w, int B, int H, int W, int C, float *dx, hipStream_t s)
{
    int pt, pl, OH, OW;
    mn_s2_geom(H, &pt, &OH);
    mn_s2_geom(W, &pl, &OW);
    const long long total = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(dwconv3x3_dgrad_kernel<2>, dim3(grid_1d(total, kGridCap)), dim3(256), 0, s, reinterpret_cast<const float4 *>(dy),
                       reinterpret_cast<const float4 *>(w), H, W, OH, OW, pt, pl, C / 4, total, reinterpret_cast<float4 *>(dx));
    return hipGetLastError();
}

size_t dwconv3x3_s2_wgrad_ws_floats(int B, int H, int W, int C)
{
    int pt, pl, OH, OW;
    mn_s2_geom(H, &pt, &OH);
    mn_s2_geom(W, &pl, &OW);
    return (size_t)mn_reduce_leaves((long long)B * OH * OW) * 9 * C;
}

hipError_t launch_dwconv3x3_s2_wgrad(const float *x, const float *dy, int B, int H, int W, int C, float *part, float *dw, hipStream_t s)
{
    int pt, pl, OH, OW;
    mn_s2_geom(H, &pt, &OH);
    mn_s2_geom(W, &pl, &OW);
    const int leaves = mn_reduce_leaves((long long)B * OH * OW);
    hipLaunchKernelGGL((dwconv3x3_wgrad_partial_kernel<2, kS2Quads, kS2Lanes>), dim3((C + kS2Quads * 4 - 1) / (kS2Quads * 4), leaves),
                       dim3(256), 0, s, reinterpret_cast<const float4 *>(x), reinterpret_cast<const float4 *>(dy), B, H, W, OH, OW, pt, pl,
                       C, leaves, part);
    hipLaunchKernelGGL(slab_tree_kernel<1>, dim3(grid_1d(9LL * C, kGridCap)), dim3(256), 0, s, part, 9LL * C, leaves, dw);
    return hipGetLastError();
}

// ---- the stem's weight gradient: 3x3 stride-2 conv from the 3-channel image (Conv1; same padding rule) -------------------------------
// dw[r][s][ci][co] = sum over the B OH OW output pixels of x[b][2 oy + r - pt][2 ox + s - pl][ci] dy[b][oy][ox][co]: 27 Cout outputs,
// each a sum over every pixel (500 000 at batch 8, 500 x 500), so the reduction tree is the kernel.  The pixels are cut into
// stem_wgrad_leaves(P) leaves (a power of two <= 256 from P alone: 32 leaves would leave 7/8 of the device idle); a leaf is one
// workgroup per 32 output channels, 8 channel quads x 32 pixel lanes, a lane keeping its 27 taps x 4 channels in registers (dy read
// once as a float4, the 27 image values of the pixel's window shared by the 8 quads through the cache).  The lanes are summed in order
// through LDS, one filter row at a time (lane_sum_store); the leaves in a fixed tree (slab_tree_kernel<8>): tree_sum32 over each group
// of 32, then the (up to 8) groups pairwise.
constexpr int kStemMaxLeaves = 256;

int stem_wgrad_leaves(long long P)
{
    int L = 1;
    while (L < kStemMaxLeaves && P / (2 * L) >= 64) L *= 2;
    return L;
}

__global__ void __launch_bounds__(256) conv3x3_s2_cin3_wgrad_partial_kernel(const float *__restrict__ x, const float4 *__restrict__ dy, int B,
                                                                           int H, int W, int OH, int OW, int pt, int pl, int Cout,
                                                                           int leaves, float *__restrict__ part)
{
    __shared__ float red[kS2Lanes][9 * kS2Quads * 4];
    const int q = threadIdx.x & (kS2Quads - 1), rl = threadIdx.x / kS2Quads;
    const int C4 = Cout / 4, cq = blockIdx.x * kS2Quads + q, leaf = blockIdx.y;
    const long long P = (long long)B * OH * OW, pbeg = P * leaf / leaves, pend = P * (leaf + 1) / leaves;
    float4 acc[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cq < C4) {
        for (long long p = pbeg + rl; p < pend; p += kS2Lanes) {
            const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
            const long long b = p / ((long long)OW * OH);
            const float4 d = dy[p * C4 + cq];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int iy = 2 * oy + r - pt;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int ix = 2 * ox + s - pl;
                    if (ix < 0 || ix >= W) continue;
                    const float *xp = x + ((b * H + iy) * W + ix) * 3;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const float v = xp[ci];
                        float4 &a = acc[(r * 3 + s) * 3 + ci];
                        a.x = fmaf(v, d.x, a.x);
                        a.y = fmaf(v, d.y, a.y);
                        a.z = fmaf(v, d.z, a.z);
                        a.w = fmaf(v, d.w, a.w);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {                   // red[lane][(s, ci)][32 channels of the tile], one filter row per pass
        if (r) __syncthreads();
        lane_sum_store<kS2Quads, kS2Lanes>(red, acc + r * 9, q, rl, blockIdx.x, Cout, part + ((size_t)leaf * 27 + r * 9) * Cout);
    }
}

size_t conv3x3_s2_cin3_wgrad_ws_floats(int B, int H, int W, int Cout)
{
    int pt, pl, OH, OW;
    mn_s2_geom(H, &pt, &OH);
    mn_s2_geom(W, &pl, &OW);
    return (size_t)stem_wgrad_leaves((long long)B * OH * OW) * 27 * Cout;
}

hipError_t launch_conv3x3_s2_cin3_wgrad(const float *x, const float *dy, int B, int H, int W, int Cout, float *part, float *dw,
                                        hipStream_t s)
{
    int pt, pl, OH, OW;
    mn_s2_geom(H, &pt, &OH);
    mn_s2_geom(W, &pl, &OW);
    const int leaves = stem_wgrad_leaves((long long)B * OH * OW);
    hipLaunchKernelGGL(conv3x3_s2_cin3_wgrad_partial_kernel, dim3((Cout + kS2Quads * 4 - 1) / (kS2Quads * 4), leaves), dim3(256), 0, s, x,
                       reinterpret_cast<const float4 *>(dy), B, H, W, OH, OW, pt, pl, Cout, leaves, part);
    hipLaunchKernelGGL(slab_tree_kernel<kStemMaxLeaves / kMaxLeaves>, dim3(grid_1d(27LL * Cout, kGridCap)), dim3(256), 0, s, part, 27LL * Cout, leaves, dw);
    return hipGetLastError();
}

}  // namespace rpn

using namespace rpn;

// ---- C ABI: single-layer entries ---------------------------------------------------------------------------------------------------
// the kernels read and write their tensors as float4
template <typename... T> static bool al16(const T *...p) { return ((... | (uintptr_t)p) & 15) == 0; }
#define MN_ALIGNED(what, ...) RPN_REQUIRE(al16(__VA_ARGS__), what ": every device pointer must be 16-byte aligned")

static bool pc_ok(long long P, int C) { return P >= 1 && P <= (1ll << 31) && C >= 4 && C % 4 == 0 && C <= (1 << 16); }
static size_t bn_ws_bytes(long long P, int C) { return a256(bn_part_doubles(P, C) * sizeof(double)) + a256((size_t)C * sizeof(float)); }

extern "C" size_t rpn_batchnorm_workspace_bytes(long long P, int C) { return pc_ok(P, C) ? bn_ws_bytes(P, C) : 0; }

extern "C" int rpn_batchnorm_train_forward(const float *d_x, long long P, int C, const float *d_gamma, const float *d_beta, int relu6,
                                           float eps, float momentum, float *d_y, float *d_mean, float *d_var, float *d_moving_mean,
                                           float *d_moving_var, void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_gamma && d_beta && d_y && d_mean && d_var, "rpn_batchnorm_train_forward: null pointer");
    RPN_REQUIRE(pc_ok(P, C), "rpn_batchnorm_train_forward: bad shape (P %lld, C %d: C must be a multiple of 4)", P, C);
    RPN_REQUIRE((d_moving_mean == nullptr) == (d_moving_var == nullptr), "rpn_batchnorm_train_forward: moving mean and variance go together");
    MN_ALIGNED("rpn_batchnorm_train_forward", d_x, d_gamma, d_beta, d_y, d_mean, d_var, d_moving_mean, d_moving_var, (const char *)d_ws);
    RPN_REQUIRE(relu6 == 0 || relu6 == 1, "rpn_batchnorm_train_forward: relu6 must be 0 or 1");
    RPN_REQUIRE(eps > 0.0f && momentum >= 0.0f && momentum <= 1.0f, "rpn_batchnorm_train_forward: bad eps / momentum");
    if (!d_ws || ws_bytes < bn_ws_bytes(P, C))
        return fail(RPN_ERR_WORKSPACE, "rpn_batchnorm_train_forward: %zu bytes of workspace needed", bn_ws_bytes(P, C));
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    double *part = reinterpret_cast<double *>(d_ws);
    float *rstd = reinterpret_cast<float *>((char *)d_ws + a256(bn_part_doubles(P, C) * sizeof(double)));
    hipError_t e = launch_bn_train_stats(d_x, P, C, eps, momentum, part, d_mean, d_var, rstd, d_moving_mean, d_moving_var, s);
    if (e == hipSuccess) e = launch_bn_apply(d_x, P, C, d_mean, rstd, d_gamma, d_beta, relu6, nullptr, d_y, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_batchnorm_train_forward: %s", hipGetErrorString(e));
}

extern "C" int rpn_batchnorm_train_backward(const float *d_x, const float *d_dy, long long P, int C, const float *d_gamma,
                                            const float *d_beta, const float *d_mean, const float *d_var, int relu6, float eps, float *d_dx,
                                            float *d_dgamma, float *d_dbeta, void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_gamma && d_beta && d_mean && d_var && d_dx && d_dgamma && d_dbeta, "rpn_batchnorm_train_backward: null pointer");
    RPN_REQUIRE(pc_ok(P, C), "rpn_batchnorm_train_backward: bad shape (P %lld, C %d: C must be a multiple of 4)", P, C);
    RPN_REQUIRE(relu6 == 0 || relu6 == 1, "rpn_batchnorm_train_backward: relu6 must be 0 or 1");
    MN_ALIGNED("rpn_batchnorm_train_backward", d_x, d_dy, d_gamma, d_beta, d_mean, d_var, d_dx, d_dgamma, d_dbeta, (const char *)d_ws);
    RPN_REQUIRE(eps > 0.0f, "rpn_batchnorm_train_backward: bad eps");
    if (!d_ws || ws_bytes < bn_ws_bytes(P, C))
        return fail(RPN_ERR_WORKSPACE, "rpn_batchnorm_train_backward: %zu bytes of workspace needed", bn_ws_bytes(P, C));
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    double *part = reinterpret_cast<double *>(d_ws);
    float *rstd = reinterpret_cast<float *>((char *)d_ws + a256(bn_part_doubles(P, C) * sizeof(double)));
    hipError_t e = launch_bn_rstd(d_var, C, eps, rstd, s);
    if (e == hipSuccess) e = launch_bn_backward(d_x, d_dy, P, C, d_mean, rstd, d_gamma, d_beta, relu6, part, d_dgamma, d_dbeta, d_dx, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_batchnorm_train_backward: %s", hipGetErrorString(e));
}

static bool gemm_ok(long long P, int Cin, int Cout)
{
    return P >= 1 && P <= (1ll << 21) && Cin >= 4 && Cout >= 4 && Cin % 4 == 0 && Cout % 4 == 0 && Cin <= 4096 && Cout <= 4096;
}

extern "C" size_t rpn_conv1x1_wgrad_workspace_bytes(long long P, int Cin, int Cout)
{
    return gemm_ok(P, Cin, Cout) ? a256(conv1x1_wgrad_ws_floats(P, Cin, Cout) * sizeof(float)) : 0;
}

extern "C" int rpn_conv1x1_wgrad(const float *d_x, const float *d_dy, long long P, int Cin, int Cout, float *d_dw, void *d_ws, size_t ws_bytes,
                                 void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw, "rpn_conv1x1_wgrad: null pointer");
    RPN_REQUIRE(gemm_ok(P, Cin, Cout), "rpn_conv1x1_wgrad: bad shape (P %lld, Cin %d, Cout %d: channels must be multiples of 4)", P, Cin, Cout);
    MN_ALIGNED("rpn_conv1x1_wgrad", d_x, d_dy, d_dw, (const char *)d_ws);
    const size_t need = rpn_conv1x1_wgrad_workspace_bytes(P, Cin, Cout);
    if (need && (!d_ws || ws_bytes < need)) return fail(RPN_ERR_WORKSPACE, "rpn_conv1x1_wgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_conv1x1_wgrad(d_x, d_dy, P, Cin, Cout, reinterpret_cast<float *>(d_ws), d_dw, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv1x1_wgrad: %s", hipGetErrorString(e));
}

extern "C" int rpn_conv1x1_dgrad(const float *d_dy, const float *d_w, const float *d_add, long long P, int Cin, int Cout, float *d_dx,
                                 void *stream)
{
    RPN_REQUIRE(d_dy && d_w && d_dx, "rpn_conv1x1_dgrad: null pointer");
    RPN_REQUIRE(gemm_ok(P, Cin, Cout), "rpn_conv1x1_dgrad: bad shape (P %lld, Cin %d, Cout %d: channels must be multiples of 4)", P, Cin, Cout);
    MN_ALIGNED("rpn_conv1x1_dgrad", d_dy, d_w, d_add, d_dx);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_conv1x1_dgrad(d_dy, d_w, d_add, P, Cin, Cout, d_dx, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv1x1_dgrad: %s", hipGetErrorString(e));
}

static bool dw_ok(int B, int H, int W, int C)
{
    return B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && C <= (1 << 16) && (long long)B * H * W <= (1ll << 31);
}

extern "C" int rpn_dwconv3x3_dgrad(const float *d_dy, const float *d_w, int B, int H, int W, int C, float *d_dx, void *stream)
{
    RPN_REQUIRE(d_dy && d_w && d_dx, "rpn_dwconv3x3_dgrad: null pointer");
    RPN_REQUIRE(dw_ok(B, H, W, C), "rpn_dwconv3x3_dgrad: bad shape (C must be a multiple of 4)");
    MN_ALIGNED("rpn_dwconv3x3_dgrad", d_dy, d_w, d_dx);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_dwconv3x3_dgrad(d_dy, d_w, B, H, W, C, d_dx, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_dwconv3x3_dgrad: %s", hipGetErrorString(e));
}

extern "C" size_t rpn_dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C)
{
    return dw_ok(B, H, W, C) ? a256(dwconv3x3_wgrad_ws_floats((long long)B * H * W, C) * sizeof(float)) : 0;
}

extern "C" int rpn_dwconv3x3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int C, float *d_dw, void *d_ws, size_t ws_bytes,
                                   void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw, "rpn_dwconv3x3_wgrad: null pointer");
    RPN_REQUIRE(dw_ok(B, H, W, C), "rpn_dwconv3x3_wgrad: bad shape (C must be a multiple of 4)");
    MN_ALIGNED("rpn_dwconv3x3_wgrad", d_x, d_dy, d_dw, (const char *)d_ws);
    const size_t need = rpn_dwconv3x3_wgrad_workspace_bytes(B, H, W, C);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_dwconv3x3_wgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_dwconv3x3_wgrad(d_x, d_dy, B, H, W, C, reinterpret_cast<float *>(d_ws), d_dw, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_dwconv3x3_wgrad: %s", hipGetErrorString(e));
}

extern "C" int rpn_dwconv3x3_s2_dgrad(const float *d_dy, const float *d_w, int B, int H, int W, int C, float *d_dx, void *stream)
{
    RPN_REQUIRE(d_dy && d_w && d_dx, "rpn_dwconv3x3_s2_dgrad: null pointer");
    RPN_REQUIRE(dw_ok(B, H, W, C), "rpn_dwconv3x3_s2_dgrad: bad shape (C must be a multiple of 4)");
    MN_ALIGNED("rpn_dwconv3x3_s2_dgrad", d_dy, d_w, d_dx);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_dwconv3x3_s2_dgrad(d_dy, d_w, B, H, W, C, d_dx, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_dwconv3x3_s2_dgrad: %s", hipGetErrorString(e));
}

extern "C" size_t rpn_dwconv3x3_s2_wgrad_workspace_bytes(int B, int H, int W, int C)
{
    return dw_ok(B, H, W, C) ? a256(dwconv3x3_s2_wgrad_ws_floats(B, H, W, C) * sizeof(float)) : 0;
}

extern "C" int rpn_dwconv3x3_s2_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int C, float *d_dw, void *d_ws,
                                      size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw, "rpn_dwconv3x3_s2_wgrad: null pointer");
    RPN_REQUIRE(dw_ok(B, H, W, C), "rpn_dwconv3x3_s2_wgrad: bad shape (C must be a multiple of 4)");
    MN_ALIGNED("rpn_dwconv3x3_s2_wgrad", d_x, d_dy, d_dw, (const char *)d_ws);
    const size_t need = rpn_dwconv3x3_s2_wgrad_workspace_bytes(B, H, W, C);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_dwconv3x3_s2_wgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_dwconv3x3_s2_wgrad(d_x, d_dy, B, H, W, C, reinterpret_cast<float *>(d_ws), d_dw, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_dwconv3x3_s2_wgrad: %s", hipGetErrorString(e));
}

extern "C" size_t rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(int B, int H, int W, int Cout)
{
    return dw_ok(B, H, W, Cout) ? a256(conv3x3_s2_cin3_wgrad_ws_floats(B, H, W, Cout) * sizeof(float)) : 0;
}

extern "C" int rpn_conv3x3_s2_cin3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int Cout, float *d_dw, void *d_ws,
                                         size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw, "rpn_conv3x3_s2_cin3_wgrad: null pointer");
    RPN_REQUIRE(dw_ok(B, H, W, Cout), "rpn_conv3x3_s2_cin3_wgrad: bad shape (Cout must be a multiple of 4)");
    MN_ALIGNED("rpn_conv3x3_s2_cin3_wgrad", d_x, d_dy, d_dw, (const char *)d_ws);
    const size_t need = rpn_conv3x3_s2_cin3_wgrad_workspace_bytes(B, H, W, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_conv3x3_s2_cin3_wgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_conv3x3_s2_cin3_wgrad(d_x, d_dy, B, H, W, Cout, reinterpret_cast<float *>(d_ws), d_dw, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv3x3_s2_cin3_wgrad: %s", hipGetErrorString(e));
}
