// train_kernels.hip -- the kernels of the RPN head's training step, the counterpart of the reference's trainer.py:54-69 (compile with
// Adam(1e-5) and loss=[reg_loss, cls_loss], then fit): the two losses and their gradients, the backward of the fused 1x1 head, the
// 3x3 weight gradient of rpn_conv, column sums and Adam, each with its host launcher (train_head.h), and the two stand-alone entries
// rpn_rpn_losses and rpn_conv3x3_wgrad.  The trainer that strings them together -- and the backbones' backward kernels of
// train_backbone_kernels.hip / train_mnv2_kernels.hip behind them -- is trainer.hip.  The 3x3 weight-gradient MFMA kernel here is the
// only one: the VGG16 backbone's wgrad (train_backbone_kernels.hip) runs its other instance through launch_wgrad_slabs.  What the
// three kernel files share (grid rule, accumulator type, the wgrad tile, the fixed trees) is in train_common.h.  Of a step these
// kernels compute
//   losses + their gradients (one pass, fixed-order reductions)
//   dZ = [dreg | dcls * p (1 - p)] (P,5K);  dW_head = S^T dZ, db_head = sum dZ;  dS = (dZ W_head^T) * [S > 0]
//   dW_conv = 3x3 weight gradient of X and dS on the float32 MFMA (split K, fixed tree), db_conv = sum dS
//   Adam over every trained tensor in one launch
// No floating-point atomics anywhere: every sum has a fixed order, so a step is bit-identical from run to run.
//
// Loss and optimizer forms (TF 2.0.0, restated from its sources as recalled -- nothing here can run TF):
//   cls_loss (utils/train_utils.py:146-162): keras BinaryCrossentropy on probabilities (backend.binary_crossentropy with
//     from_logits=False): p' = clip(p, 1e-7, 1 - 1e-7), bce = -(t log(p' + 1e-7) + (1 - t) log(1 - p' + 1e-7)), mean over the kept
//     entries (y_true != -1) of the whole batch; NaN when nothing is kept.  The gradient is zero where the clip is active.
//   reg_loss (utils/train_utils.py:164-185): Huber (delta 1) per element -- TF 2.0's huber_loss has no mean over the last axis --
//     summed over the 4 coordinates, masked by "any y_true coordinate != 0", summed, divided by max(1, n_pos).
//   Adam (training_ops ApplyAdam): alpha = lr sqrt(1 - b2^t) / (1 - b1^t); m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2);
//     w -= alpha m / (sqrt(v) + eps), t = the number of applied steps.
//   BatchNorm in training mode (the fused BatchNorm kernels; MobileNetV2 span, train_mnv2_kernels.hip): normalise with the batch mean
//     and the biased batch variance over (B, H, W), eps 1e-3; moving = moving * momentum + batch * (1 - momentum) with momentum 0.999,
//     the variance with Bessel's correction N / (N - 1); Relu6Grad keeps dy where 0 < y < 6, strict on both sides.
#include <algorithm>
#include <cmath>

#include "rpn_common.h"
#include "train_common.h"
#include "train_head.h"

namespace rpn {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 512;
constexpr int kChunkRows = 64;          // rows per partial of the column sums / the head weight gradient
constexpr int kLeaves = 4;              // K leaves of the head's 3x3 weight gradient: the value is (l0 + l1) + (l2 + l3) at every grid
constexpr int kGridCap = 2048;          // workgroups of this file's grid-stride kernels
constexpr float kClipLo = 1e-7f, kClipHi = 1.0f - 1e-7f;   // keras epsilon() and 1 - epsilon() as float32 constants
constexpr double kLogEps = (double)1e-7f;

static int loss_blocks(long long n) { return (int)std::min<long long>((n + kLossThreads - 1) / kLossThreads, kLossMaxBlocks); }

// ---- losses: pass 1 ---------------------------------------------------------------------------------------------------
// Per element of (B, A): the Huber sum of the 4 coordinates (counted when any true coordinate is non-zero) and the BCE of the
// kept labels, both in float64; the UNSCALED gradients (clip(pred - true, -1, 1) * mask, d bce / d p) go to graw_*; the block's
// partial sums (reg, cls, n_pos, n_valid) go to part[block] after a fixed LDS tree.
__global__ void __launch_bounds__(kLossThreads) rpn_loss_kernel(const float4 *__restrict__ reg_true, const float4 *__restrict__ reg_pred,
                                                              const float *__restrict__ cls_true, const float *__restrict__ cls_pred,
                                                              long long n, float4 *__restrict__ graw_reg, float *__restrict__ graw_cls,
                                                              double4 *__restrict__ part)
{
    double reg = 0.0, cls = 0.0, npos = 0.0, nval = 0.0;
    for (long long i = (long long)blockIdx.x * kLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kLossThreads) {
        const float4 t = reg_true[i], p = reg_pred[i];
        const bool pos = t.x != 0.0f || t.y != 0.0f || t.z != 0.0f || t.w != 0.0f;
        const double d[4] = {(double)p.x - t.x, (double)p.y - t.y, (double)p.z - t.z, (double)p.w - t.w};
        double h = 0.0;
        float g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double a = fabs(d[c]), q = fmin(a, 1.0);
            h += 0.5 * q * q + (a - q);
            g[c] = pos ? (float)fmax(-1.0, fmin(1.0, d[c])) : 0.0f;
        }
        if (pos) { reg += h; npos += 1.0; }
        if (graw_reg) graw_reg[i] = make_float4(g[0], g[1], g[2], g[3]);
        const float y = cls_true[i];
        float gc = 0.0f;
        if (y != -1.0f) {
            const float pr = cls_pred[i];
            const double pc = (double)fminf(fmaxf(pr, kClipLo), kClipHi), yd = y;
            cls -= yd * log(pc + kLogEps) + (1.0 - yd) * log(1.0 - pc + kLogEps);
            nval += 1.0;
            if (pr >= kClipLo && pr <= kClipHi) gc = (float)(-(yd / (pc + kLogEps)) + (1.0 - yd) / (1.0 - pc + kLogEps));
        }
        if (graw_cls) graw_cls[i] = gc;
    }
    __shared__ double4 red[kLossThreads];
    red[threadIdx.x] = make_double4(reg, cls, npos, nval);
    __syncthreads();
    for (int w = kLossThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double4 a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = make_double4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ---- losses: pass 2 (one workgroup) -- the partials in a fixed tree, the two losses and the gradient scales -----------------
// out: [reg, cls] or, with_total, [reg + cls, reg, cls]; scale = {1 / max(1, n_pos), n_valid ? 1 / n_valid : 0}
__global__ void __launch_bounds__(kLossThreads) rpn_loss_finish_kernel(const double4 *__restrict__ part, int nparts, float *__restrict__ out,
                                                                     int with_total, float *__restrict__ scale)
{
    __shared__ double4 red[kLossThreads];
    double4 s = make_double4(0.0, 0.0, 0.0, 0.0);
    for (int i = threadIdx.x; i < nparts; i += kLossThreads) {
        const double4 a = part[i];
        s = make_double4(s.x + a.x, s.y + a.y, s.z + a.z, s.w + a.w);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kLossThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double4 a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = make_double4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double4 t = red[0];
        const float reg = (float)(t.x / fmax(1.0, t.z));
        const float cls = t.w > 0.0 ? (float)(t.y / t.w) : __builtin_nanf("");    // mean of an empty tensor
        if (with_total) { out[0] = reg + cls; out[1] = reg; out[2] = cls; }
        else { out[0] = reg; out[1] = cls; }
        scale[0] = (float)(1.0 / fmax(1.0, t.z));
        scale[1] = t.w > 0.0 ? (float)(1.0 / t.w) : 0.0f;
    }
}

__global__ void __launch_bounds__(256) rpn_loss_scale_kernel(float *__restrict__ g_reg, float *__restrict__ g_cls, long long n,
                                                           const float *__restrict__ scale)
{
    const float sr = scale[0], sc = scale[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (g_reg) {
#pragma unroll
            for (int c = 0; c < 4; ++c) g_reg[4 * i + c] *= sr;
        }
        if (g_cls) g_cls[i] *= sc;
    }
}

// ---- head backward ------------------------------------------------------------------------------------------------------
// dZ (P, 5K) = [graw_reg * s_reg | graw_cls * s_cls * p (1 - p)] (the sigmoid of the cls columns folded in here)
__global__ void __launch_bounds__(256) head_dz_kernel(const float *__restrict__ graw_reg, const float *__restrict__ graw_cls,
                                                    const float *__restrict__ cls, const float *__restrict__ scale, long long P, int K,
                                                    float *__restrict__ dz)
{
    const int nc = 5 * K;
    const float sr = scale[0], sc = scale[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P * nc; i += (long long)gridDim.x * 256) {
        const long long row = i / nc;
        const int c = (int)(i - row * nc);
        float v;
        if (c < 4 * K) {
            v = graw_reg[row * 4 * K + c] * sr;
        } else {
            const float p = cls[row * K + c - 4 * K];
            v = graw_cls[row * K + c - 4 * K] * sc * (p * (1.0f - p));
        }
        dz[i] = v;
    }
}

// partial of dW_head = S^T dZ (rows 0 .. 511) and db_head = sum dZ (row 512) over the kChunkRows rows of chunk blockIdx.x:
// part[chunk][513][nc].  Thread t owns input channels t and t + 256; rows in order.
template <int NC>
__global__ void __launch_bounds__(256) head_wgrad_kernel(const float *__restrict__ S, const float *__restrict__ dz, long long P,
                                                       float *__restrict__ part)
{
    __shared__ float zs[kChunkRows][NC];
    const long long r0 = (long long)blockIdx.x * kChunkRows;
    const int rows = (int)std::min<long long>(kChunkRows, P - r0);
    for (int i = threadIdx.x; i < rows * NC; i += 256) zs[i / NC][i % NC] = dz[r0 * NC + i];
    __syncthreads();
    float acc0[NC], acc1[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc0[c] = acc1[c] = 0.0f;
    for (int r = 0; r < rows; ++r) {
        const float s0 = S[(r0 + r) * 512 + threadIdx.x], s1 = S[(r0 + r) * 512 + threadIdx.x + 256];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            acc0[c] = fmaf(s0, zs[r][c], acc0[c]);
            acc1[c] = fmaf(s1, zs[r][c], acc1[c]);
        }
    }
    float *dst = part + (size_t)blockIdx.x * 513 * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        dst[threadIdx.x * NC + c] = acc0[c];
        dst[(threadIdx.x + 256) * NC + c] = acc1[c];
    }
    if (threadIdx.x < NC) {
        float b = 0.0f;
        for (int r = 0; r < rows; ++r) b += zs[r][threadIdx.x];
        dst[512 * NC + threadIdx.x] = b;
    }
}

// dS (P, 512) = (dZ W_head^T) * [S > 0]; w_head (512, NC) row-major.  16 rows per workgroup of 512 threads, thread t: channel t.
template <int NC>
__global__ void __launch_bounds__(512) head_dgrad_kernel(const float *__restrict__ S, const float *__restrict__ dz,
                                                       const float *__restrict__ w_head, long long P, float *__restrict__ dS)
{
    constexpr int RB = 16;
    __shared__ float zs[RB][NC];
    const long long r0 = (long long)blockIdx.x * RB;
    const int rows = (int)std::min<long long>(RB, P - r0);
    for (int i = threadIdx.x; i < rows * NC; i += 512) zs[i / NC][i % NC] = dz[r0 * NC + i];
    __syncthreads();
    float w[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = w_head[threadIdx.x * NC + c];
#pragma unroll 1
    for (int r = 0; r < rows; ++r) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) a = fmaf(zs[r][c], w[c], a);
        const long long o = (r0 + r) * 512 + threadIdx.x;
        dS[o] = S[o] > 0.0f ? a : 0.0f;
    }
}

// column sums of x (rows, C) over chunks of kChunkRows rows, rows in order: part[chunk][C]
__global__ void __launch_bounds__(256) colsum_partial_kernel(const float *__restrict__ x, long long rows, int C, float *__restrict__ part)
{
    const long long r0 = (long long)blockIdx.x * kChunkRows;
    const int nr = (int)std::min<long long>(kChunkRows, rows - r0);
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.0f;
        for (int r = 0; r < nr; ++r) s += x[(r0 + r) * C + c];
        part[(size_t)blockIdx.x * C + c] = s;
    }
}

// out[j] = sum over the chunks, in chunk order, of part[chunk][j]
__global__ void __launch_bounds__(256) reduce_chunks_kernel(const float *__restrict__ part, int nchunks, long long len, float *__restrict__ out)
{
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < len; j += (long long)gridDim.x * 256) {
        float s = 0.0f;
        for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * len + j];
        out[j] = s;
    }
}

// ---- 3x3 stride-1 'same' weight gradient on the float32 MFMA -----------------------------------------------------------------
// dW[r][s][ci][co] = sum_{b,y,x} X[b][y+r-1][x+s-1][ci] * dY[b][y][x][co] (zero padding): a GEMM C (M x N) = A^T B with
// M = 9 Cin (row m = (3 r + s) Cin + ci), N = Cout, K = the P = B H W pixels; both operands are pixel-major (A^T[p][m] is a
// shifted row of X, B[p][n] a row of dY), so a K slice of either is a contiguous run of channels per pixel.
// With ONES the GEMM has one more row, M1 = M + 1: row 9 Cin is a row of ones, which yields db = sum dY.
// Workgroup: a 128 x 128 tile of C (train_common.h) over ONE of `leaves` fixed ranges of pixels (leaf l = blockIdx.z:
// [l P / leaves, (l + 1) P / leaves)); four waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x2_f32 blocks).  K slices of 16 pixels are
// staged global -> registers -> LDS (double-buffered, one barrier per slice, the next slice's loads in flight under the current
// slice's MFMAs), as conv_igemm_f32 stages its operands.  Each leaf's tile goes to its own slab of M1 x Cout floats; the callers
// add the slabs, each in its own fixed order: the head (launch_wgrad, 4 leaves) as (l0 + l1) + (l2 + l3) in wgrad_reduce_kernel,
// the VGG16 backbone (launch_wgrad_wide, train_backbone_kernels.hip) slab i with slab i + half.  The leaves do not depend on the
// grid: the same bits at every launch.
template <bool ONES>
__global__ void __launch_bounds__(256) conv3x3_wgrad_f32_kernel(const float *__restrict__ X, const float *__restrict__ dY, int B, int H,
                                                              int W, int Cin, int Cout, int leaves, float *__restrict__ part)
{
    __shared__ float As[2][kWgBK][kWgLd];
    __shared__ float Bs[2][kWgBK][kWgLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = 9 * Cin, M1 = M + (ONES ? 1 : 0), n0 = blockIdx.x * kWgBN, m0 = blockIdx.y * kWgBM, leaf = blockIdx.z;
    const long long P = (long long)B * H * W;
    const long long pbeg = P * leaf / leaves, pend = P * (leaf + 1) / leaves;
    const int nsteps = (int)((pend - pbeg + kWgBK - 1) / kWgBK);

    // loader: thread -> (pixel row kr and kr + 8 of the slice, 4-channel quad q); the same (tap, ci) / n for every slice
    const int kr = tid >> 5, q = tid & 31;
    const int m = m0 + 4 * q, n = n0 + 4 * q;
    const bool m_ok = m < M, ones = ONES && m == M, n_ok = n < Cout;
    const int tap = m_ok ? m / Cin : 0, ci = m_ok ? m - tap * Cin : 0;
    const int dr = tap / 3 - 1, ds = tap % 3 - 1;
    // pixel coordinates of this thread's two rows at the current slice, advanced by 16 pixels per slice
    int pb[2], py[2], px[2];
    long long pp[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        pp[u] = pbeg + kr + 8 * u;
        const long long hw = (long long)H * W;
        pb[u] = (int)(pp[u] / hw);
        const int rem = (int)(pp[u] - (long long)pb[u] * hw);
        py[u] = rem / W;
        px[u] = rem - py[u] * W;
    }
    float4 ra[2], rb[2];
    auto load_global = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            ra[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            rb[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (pp[u] < pend) {
                const int yy = py[u] + dr, xx = px[u] + ds;
                if (m_ok && yy >= 0 && yy < H && xx >= 0 && xx < W)
                    ra[u] = *reinterpret_cast<const float4 *>(X + (((size_t)pb[u] * H + yy) * W + xx) * Cin + ci);
                if (ones) ra[u].x = 1.0f;
                if (n_ok) rb[u] = *reinterpret_cast<const float4 *>(dY + (size_t)pp[u] * Cout + n);
            }
        }
    };
    auto advance = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pp[u] += kWgBK;
            px[u] += kWgBK;
            while (px[u] >= W) {
                px[u] -= W;
                if (++py[u] == H) { py[u] = 0; ++pb[u]; }
            }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            *reinterpret_cast<float4 *>(&As[buf][kr + 8 * u][4 * q]) = ra[u];
            *reinterpret_cast<float4 *>(&Bs[buf][kr + 8 * u][4 * q]) = rb[u];
        }
    };

    f32x16t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int am = wm * 64 + (lane & 31), bn = wn * 64 + (lane & 31), kh = lane >> 5;

    load_global();
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) {
            advance();
            load_global();
        }
#pragma unroll
        for (int kk = 0; kk < kWgBK / 2; ++kk) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = As[cur][2 * kk + kh][am + 32 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[cur][2 * kk + kh][bn + 32 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator element e of block (i, j): row 8 (e / 4) + 4 kh + e % 4, column lane % 32
    float *slab = part + (size_t)leaf * M1 * Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + 32 * j + (lane & 31);
            if (col >= Cout) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + 32 * i + 8 * (e >> 2) + 4 * kh + (e & 3);
                if (row < M1) slab[(size_t)row * Cout + col] = acc[i][j][e];
            }
        }
}

// dW = (l0 + l1) + (l2 + l3) over the four leaf slabs of len floats each
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float *__restrict__ part, long long len, float *__restrict__ dw)
{
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < len; j += (long long)gridDim.x * 256)
        dw[j] = (part[j] + part[len + j]) + (part[2 * len + j] + part[3 * len + j]);
}

// ---- Adam (ApplyAdam) over one flat float32 buffer holding every trained tensor ------------------------------------------------
__global__ void __launch_bounds__(256) adam_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ mom,
                                                 float *__restrict__ vel, long long n, long long t, float lr, float b1, float b2, float eps)
{
    const float alpha = (float)((double)lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t)));
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i];
        const float mi = mom[i] + (gi - mom[i]) * (1.0f - b1);
        const float vi = vel[i] + (gi * gi - vel[i]) * (1.0f - b2);
        mom[i] = mi;
        vel[i] = vi;
        w[i] -= alpha * mi / (sqrtf(vi) + eps);
    }
}

// ---- host launchers ----------------------------------------------------------------------------------------------------------
size_t losses_ws_bytes(long long n) { return a256((size_t)loss_blocks(n) * sizeof(double4)) + 256; }

// pass 1 + pass 2; the gradient scales land at the end of the workspace (losses_scale)
float *losses_scale(void *ws, long long n) { return reinterpret_cast<float *>((char *)ws + a256((size_t)loss_blocks(n) * sizeof(double4))); }

hipError_t launch_losses(const float *reg_true, const float *reg_pred, const float *cls_true, const float *cls_pred, long long n,
                         float *graw_reg, float *graw_cls, float *out, int with_total, void *ws, hipStream_t s)
{
    const int nb = loss_blocks(n);
    double4 *part = reinterpret_cast<double4 *>(ws);
    hipLaunchKernelGGL(rpn_loss_kernel, dim3(nb), dim3(kLossThreads), 0, s, reinterpret_cast<const float4 *>(reg_true),
                       reinterpret_cast<const float4 *>(reg_pred), cls_true, cls_pred, n, reinterpret_cast<float4 *>(graw_reg),
                       graw_cls, part);
    hipLaunchKernelGGL(rpn_loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, s, part, nb, out, with_total, losses_scale(ws, n));
    return hipGetLastError();
}

size_t colsum_ws_floats(long long rows, int C) { return (size_t)((rows + kChunkRows - 1) / kChunkRows) * C; }

hipError_t launch_colsum(const float *x, long long rows, int C, float *part, float *out, hipStream_t s)
{
    const int nchunks = (int)((rows + kChunkRows - 1) / kChunkRows);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nchunks), dim3(256), 0, s, x, rows, C, part);
    hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_1d(C, kGridCap)), dim3(256), 0, s, part, nchunks, (long long)C, out);
    return hipGetLastError();
}

size_t wgrad_ws_floats(int Cin, int Cout) { return (size_t)kLeaves * 9 * Cin * Cout; }

void launch_wgrad_slabs(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, int leaves, bool ones, float *part,
                        hipStream_t s)
{
    const dim3 grid((Cout + kWgBN - 1) / kWgBN, (9 * Cin + (ones ? 1 : 0) + kWgBM - 1) / kWgBM, leaves);
    if (ones)
        hipLaunchKernelGGL(conv3x3_wgrad_f32_kernel<true>, grid, dim3(256), 0, s, x, dy, B, H, W, Cin, Cout, leaves, part);
    else
        hipLaunchKernelGGL(conv3x3_wgrad_f32_kernel<false>, grid, dim3(256), 0, s, x, dy, B, H, W, Cin, Cout, leaves, part);
}

hipError_t launch_wgrad(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, float *part, float *dw, hipStream_t s)
{
    launch_wgrad_slabs(x, dy, B, H, W, Cin, Cout, kLeaves, false, part, s);
    const long long len = 9LL * Cin * Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_1d(len, kGridCap)), dim3(256), 0, s, part, len, dw);
    return hipGetLastError();
}

size_t head_backward_ws_floats(long long P, int nc) { return (size_t)((P + kChunkRows - 1) / kChunkRows) * 513 * nc; }

hipError_t launch_head_backward(const float *graw_reg, const float *graw_cls, const float *cls, const float *scale, const float *S,
                                const float *w_head, long long P, int K, float *dz, float *part, float *dw_head, float *dS,
                                bool *supported, hipStream_t s)
{
    const int nc = 5 * K;
    hipLaunchKernelGGL(head_dz_kernel, dim3(grid_1d(P * nc, kGridCap)), dim3(256), 0, s, graw_reg, graw_cls, cls, scale, P, K, dz);
    const int chunks = (int)((P + kChunkRows - 1) / kChunkRows);
    const int dgrid = (int)((P + 15) / 16);
    *supported = true;
    // head_{w,d}grad are instantiated for the anchor counts of the reference's configurations (5 K = 45: 3 ratios x 3 scales)
    // and the other small tables up to K = 12
    switch (nc) {
#define RPN_HEAD_NC(NCV)                                                                                                    \
    case NCV:                                                                                                               \
        hipLaunchKernelGGL(head_wgrad_kernel<NCV>, dim3(chunks), dim3(256), 0, s, S, dz, P, part);                          \
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_1d(513 * NCV, kGridCap)), dim3(256), 0, s, part, chunks, 513LL * NCV, dw_head); \
        hipLaunchKernelGGL(head_dgrad_kernel<NCV>, dim3(dgrid), dim3(512), 0, s, S, dz, w_head, P, dS);                     \
        break;
        RPN_HEAD_NC(5) RPN_HEAD_NC(10) RPN_HEAD_NC(15) RPN_HEAD_NC(20) RPN_HEAD_NC(25) RPN_HEAD_NC(30) RPN_HEAD_NC(35)
        RPN_HEAD_NC(40) RPN_HEAD_NC(45) RPN_HEAD_NC(50) RPN_HEAD_NC(55) RPN_HEAD_NC(60)
#undef RPN_HEAD_NC
        default: *supported = false;
    }
    return hipGetLastError();
}

hipError_t launch_adam(float *w, const float *g, float *m, float *v, long long n, long long t, float lr, float b1, float b2, float eps,
                       hipStream_t s)
{
    hipLaunchKernelGGL(adam_kernel, dim3(grid_1d(n, kGridCap)), dim3(256), 0, s, w, g, m, v, n, t, lr, b1, b2, eps);
    return hipGetLastError();
}

}  // namespace rpn

using namespace rpn;

// ---- C ABI: losses -----------------------------------------------------------------------------------------------------------
extern "C" size_t rpn_rpn_losses_workspace_bytes(int B, int A)
{
    if (B < 1 || A < 1) return 0;
    return losses_ws_bytes((long long)B * A);
}

extern "C" int rpn_rpn_losses(const float *d_reg_true, const float *d_reg_pred, const float *d_cls_true, const float *d_cls_pred, int B,
                              int A, float *d_losses, float *d_grad_reg, float *d_grad_cls, void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_reg_true && d_reg_pred && d_cls_true && d_cls_pred && d_losses, "rpn_rpn_losses: null pointer");
    RPN_REQUIRE(B >= 1 && A >= 1, "rpn_rpn_losses: bad shape B=%d A=%d", B, A);
    const long long n = (long long)B * A;
    if (!d_ws || ws_bytes < losses_ws_bytes(n))
        return fail(RPN_ERR_WORKSPACE, "rpn_rpn_losses: %zu bytes of workspace needed", losses_ws_bytes(n));
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    hipError_t e = launch_losses(d_reg_true, d_reg_pred, d_cls_true, d_cls_pred, n, d_grad_reg, d_grad_cls, d_losses, 0, d_ws, s);
    if (e == hipSuccess && (d_grad_reg || d_grad_cls)) {
        hipLaunchKernelGGL(rpn_loss_scale_kernel, dim3(grid_1d(n, kGridCap)), dim3(256), 0, s, d_grad_reg, d_grad_cls, n, losses_scale(d_ws, n));
        e = hipGetLastError();
    }
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_rpn_losses: %s", hipGetErrorString(e));
}

// ---- C ABI: single-layer weight gradient -------------------------------------------------------------------------------------
extern "C" size_t rpn_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout)
{
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return 0;
    return a256(wgrad_ws_floats(Cin, Cout) * sizeof(float)) + a256(colsum_ws_floats((long long)B * H * W, Cout) * sizeof(float));
}

extern "C" int rpn_conv3x3_wgrad(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw, float *d_db,
                                 void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw, "rpn_conv3x3_wgrad: null pointer");
    RPN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 4 && Cout >= 4, "rpn_conv3x3_wgrad: bad shape");
    RPN_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0, "rpn_conv3x3_wgrad: Cin and Cout must be multiples of 4");
    RPN_REQUIRE((long long)9 * Cin * Cout <= (1ll << 30) && (long long)H * W <= (1 << 30), "rpn_conv3x3_wgrad: layer too large");
    const size_t need = rpn_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_conv3x3_wgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    float *part = reinterpret_cast<float *>(d_ws);
    hipError_t e = launch_wgrad(d_x, d_dy, B, H, W, Cin, Cout, part, d_dw, s);
    if (e == hipSuccess && d_db)
        e = launch_colsum(d_dy, (long long)B * H * W, Cout, part + a256(wgrad_ws_floats(Cin, Cout) * sizeof(float)) / sizeof(float), d_db, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv3x3_wgrad: %s", hipGetErrorString(e));
}
