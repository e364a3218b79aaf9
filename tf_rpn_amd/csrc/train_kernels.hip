// train_kernels.hip -- training of the RPN head (rpn_conv, rpn_cls, rpn_reg) on a frozen backbone: the counterpart of the
// reference's trainer.py:54-69 (compile with Adam(1e-5) and loss=[reg_loss, cls_loss], then fit).
//
// rpn_head_trainer_create trains the head on a frozen backbone; rpn_model_trainer_create also trains the VGG16 convs from a given one
// up (the reference's Keras base model is trainable): the step then runs the whole VGG16 forward in exact float32 from the trainer's
// weights (backbone_forward) and, after the head's backward below, the backbone's (backbone_backward; kernels in
// train_backbone_kernels.hip).  On a MobileNetV2 handle it trains the stride-16 blocks from a given expand conv up (block_7 ..
// block_12, block_13_expand) with BatchNorm in training mode: the layers below run frozen on the handle's ops (BatchNorm folded),
// the trained ones in exact float32 from the trainer's unfolded parameters (mn_forward / mn_backward; kernels and the recalled
// BatchNorm form in train_mnv2_kernels.hip).  The head-only step is
//   backbone (the handle's own ops and precision) -> X (B,F,F,Cin) float32
//   rpn_conv (exact float32, ReLU) -> S (P,512), P = B F F;  fused 1x1 head -> reg (P,4K) linear | cls (P,K) sigmoid
//   losses + their gradients (one pass, fixed-order reductions)
//   dZ = [dreg | dcls * p (1 - p)] (P,5K);  dW_head = S^T dZ, db_head = sum dZ;  dS = (dZ W_head^T) * [S > 0]
//   dW_conv = 3x3 weight gradient of X and dS on the float32 MFMA (split K, fixed tree), db_conv = sum dS
//   Adam over the six parameter tensors in one launch
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
#include <cstring>
#include <string>
#include <vector>

#include "conv_kernels.h"
#include "rpn_common.h"
#include "train_backbone.h"
#include "train_mnv2.h"

namespace rpn {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 512;
constexpr int kChunkRows = 64;          // rows per partial of the column sums / the head weight gradient
constexpr int kLeaves = 4;              // K leaves of the 3x3 weight gradient: the value is (l0 + l1) + (l2 + l3) at every grid
constexpr float kClipLo = 1e-7f, kClipHi = 1.0f - 1e-7f;   // keras epsilon() and 1 - epsilon() as float32 constants
constexpr double kLogEps = (double)1e-7f;

static size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }
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
// Workgroup: a 128 x 128 tile of C over ONE of kLeaves fixed ranges of pixels (leaf l: [l P / 4, (l + 1) P / 4)); four waves of
// 64 x 64 (2 x 2 v_mfma_f32_32x32x2_f32 blocks).  K slices of 16 pixels are staged global -> registers -> LDS (double-buffered,
// one barrier per slice, the next slice's loads in flight under the current slice's MFMAs), as conv_igemm_f32 stages its
// operands.  Each leaf's tile goes to its own slab of the workspace; wgrad_reduce_kernel adds (l0 + l1) + (l2 + l3).  The
// leaves do not depend on the grid: the same bits at every launch.
constexpr int kWgBM = 128, kWgBN = 128, kWgBK = 16, kWgLd = 160;   // LDS row stride: the two half-waves of a fragment read hit disjoint banks

using f32x16w = __attribute__((ext_vector_type(16))) float;

__global__ void __launch_bounds__(256) conv3x3_wgrad_f32_kernel(const float *__restrict__ X, const float *__restrict__ dY, int B, int H,
                                                              int W, int Cin, int Cout, float *__restrict__ part)
{
    __shared__ float As[2][kWgBK][kWgLd];
    __shared__ float Bs[2][kWgBK][kWgLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = 9 * Cin, n0 = blockIdx.x * kWgBN, m0 = blockIdx.y * kWgBM, leaf = blockIdx.z;
    const long long P = (long long)B * H * W;
    const long long pbeg = P * leaf / kLeaves, pend = P * (leaf + 1) / kLeaves;
    const int nsteps = (int)((pend - pbeg + kWgBK - 1) / kWgBK);

    // loader: thread -> (pixel row kr and kr + 8 of the slice, 4-channel quad q); the same (tap, ci) / n for every slice
    const int kr = tid >> 5, q = tid & 31;
    const int m = m0 + 4 * q, n = n0 + 4 * q;
    const bool m_ok = m < M, n_ok = n < Cout;
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

    f32x16w acc[2][2];
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
    float *slab = part + (size_t)leaf * M * Cout;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + 32 * j + (lane & 31);
            if (col >= Cout) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + 32 * i + 8 * (e >> 2) + 4 * kh + (e & 3);
                if (row < M) slab[(size_t)row * Cout + col] = acc[i][j][e];
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

static int grid_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 2048)); }

// ---- host launchers ----------------------------------------------------------------------------------------------------------
static size_t losses_ws_bytes(long long n) { return a256((size_t)loss_blocks(n) * sizeof(double4)) + 256; }

// pass 1 + pass 2; the gradient scales land at the end of the workspace (losses_scale)
static float *losses_scale(void *ws, long long n) { return reinterpret_cast<float *>((char *)ws + a256((size_t)loss_blocks(n) * sizeof(double4))); }

static hipError_t launch_losses(const float *reg_true, const float *reg_pred, const float *cls_true, const float *cls_pred, long long n,
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

static size_t colsum_ws_floats(long long rows, int C) { return (size_t)((rows + kChunkRows - 1) / kChunkRows) * C; }

static hipError_t launch_colsum(const float *x, long long rows, int C, float *part, float *out, hipStream_t s)
{
    const int nchunks = (int)((rows + kChunkRows - 1) / kChunkRows);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nchunks), dim3(256), 0, s, x, rows, C, part);
    hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_for(C)), dim3(256), 0, s, part, nchunks, (long long)C, out);
    return hipGetLastError();
}

static size_t wgrad_ws_floats(int Cin, int Cout) { return (size_t)kLeaves * 9 * Cin * Cout; }

static hipError_t launch_wgrad(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, float *part, float *dw, hipStream_t s)
{
    const int M = 9 * Cin;
    hipLaunchKernelGGL(conv3x3_wgrad_f32_kernel, dim3((Cout + kWgBN - 1) / kWgBN, (M + kWgBM - 1) / kWgBM, kLeaves), dim3(256), 0, s, x,
                       dy, B, H, W, Cin, Cout, part);
    const long long len = (long long)M * Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for(len)), dim3(256), 0, s, part, len, dw);
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
        hipLaunchKernelGGL(rpn_loss_scale_kernel, dim3(grid_for(n)), dim3(256), 0, s, d_grad_reg, d_grad_cls, n, losses_scale(d_ws, n));
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

// ---- C ABI: the head trainer -------------------------------------------------------------------------------------------------
constexpr int kMnMax = 40;                      // MobileNetV2's convs up to block_13_expand (mn_table())
struct rpn_head_trainer {
    rpn_model *m = nullptr;
    int cin = 0, F = 0, K = 0, max_batch = 0, nc = 0;
    // master weights, flat: [rpn_conv kernel (3,3,cin,512) | rpn_conv bias | head kernel (512, 5K): rpn_reg columns, then rpn_cls |
    // head bias (5K)] -- gradients, Adam's m and v in the same layout
    size_t off_ck = 0, off_cb = 0, off_hk = 0, off_hb = 0, n = 0;
    std::vector<float> host_w;                  // the master weights until the first step moves them to the device
    bool loaded[3] = {false, false, false};     // rpn_conv, rpn_reg, rpn_cls
    long long t = 0;                            // applied Adam steps
    int last_B = 0;
    int pending_B = 0;                          // the batch of a forward(train = 1) whose backward has not run yet; 0: none
    const float *pending_imgs = nullptr;        // ... and its d_imgs
    const float *d_tap = nullptr;               // the feature tap of the last forward (d_feat, or the VGG16 span's block5_conv3 output)
    float *d_w = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr;
    float *d_pconv = nullptr, *d_phead = nullptr;
    float *d_feat = nullptr, *d_S = nullptr, *d_reg = nullptr, *d_cls = nullptr, *d_graw = nullptr, *d_dz = nullptr, *d_dS = nullptr;
    float *d_part = nullptr;
    void *d_lws = nullptr;
    PackedShape ps_conv{}, ps_head{};
    // ---- the VGG16 backbone (rpn_model_trainer_create; train_kernels.hip: backbone_*) ----
    // bb_from: the first trained conv (index into kVgg), -1 on a head-only trainer.  Trained convs bb_from .. 12 follow the head in
    // the flat buffers (kernel HWIO, then bias, at off_bk / off_bb); the frozen ones live in host_frozen / d_frozen at the same offsets.
    int bb_from = -1, img = 0;
    int hs[13] = {};                             // spatial side of each conv's input and output
    size_t off_bk[13] = {}, off_bb[13] = {};
    bool bb_loaded[13] = {};
    std::vector<float> host_frozen;
    PackedShape ps_bb[13]{};
    float *d_frozen = nullptr, *d_pack = nullptr, *d_wt = nullptr, *d_wpart = nullptr, *d_img4 = nullptr;
    float *d_act[13] = {}, *d_pool[13] = {}, *d_ping[2] = {}, *d_grad[2] = {};
    // ---- MobileNetV2 (rpn_model_trainer_create / _create_full on a MobileNetV2 handle; mn_*) ----
    // mn_from: the first trained layer (index into mn_table(): an expand conv of the stride-16 span, or 0 = Conv1: the whole model),
    // -1: none.  A trained layer's kernel, gamma and beta follow the head in the flat buffers (off_mk / off_mg / off_mb); its moving
    // mean | variance are state outside Adam's buffer (host_bn / d_bn at off_ms); d_bstat holds the statistics a step normalised with
    // (mean | var | rstd at off_bs).  mn_hin / mn_hout: the spatial side of each layer's input and output.
    int mn_from = -1;
    std::string mn_x0;                           // the handle's tensor below the span: the frozen prefix ends there (none from Conv1)
    int mn_hin[kMnMax] = {}, mn_hout[kMnMax] = {};
    size_t off_mk[kMnMax] = {}, off_mg[kMnMax] = {}, off_mb[kMnMax] = {}, off_ms[kMnMax] = {}, off_bs[kMnMax] = {};
    bool mn_loaded[kMnMax] = {}, mn_bn_loaded[kMnMax] = {};
    std::vector<float> host_bn;
    PackedShape ps_mn[kMnMax]{};
    float *d_bn = nullptr, *d_bstat = nullptr, *d_x0 = nullptr, *d_mpack = nullptr, *d_mwpart = nullptr;
    double *d_mpart = nullptr;
    float *d_mz[kMnMax] = {}, *d_my[kMnMax] = {}, *d_mgr[2] = {}, *d_mt[3] = {};
};

namespace {

const char *kHeadLayers[3] = {"rpn_conv", "rpn_reg", "rpn_cls"};

int layer_index(const char *name)
{
    for (int i = 0; i < 3; ++i)
        if (!strcmp(name, kHeadLayers[i])) return i;
    return -1;
}

// the 13 convs of VGG16 (models/rpn_vgg16.py: keras.applications.VGG16 up to block5_conv3), each 3x3 'same' + ReLU;
// pool: MaxPooling2D(2, 2) 'valid' after the conv
struct VggConv {
    const char *name;
    int cin, cout;
    bool pool;
};
const VggConv kVgg[13] = {{"block1_conv1", 3, 64, false},    {"block1_conv2", 64, 64, true},    {"block2_conv1", 64, 128, false},
                          {"block2_conv2", 128, 128, true},  {"block3_conv1", 128, 256, false}, {"block3_conv2", 256, 256, false},
                          {"block3_conv3", 256, 256, true},  {"block4_conv1", 256, 512, false}, {"block4_conv2", 512, 512, false},
                          {"block4_conv3", 512, 512, true},  {"block5_conv1", 512, 512, false}, {"block5_conv2", 512, 512, false},
                          {"block5_conv3", 512, 512, false}};

int vgg_index(const char *name)
{
    for (int i = 0; i < 13; ++i)
        if (!strcmp(name, kVgg[i].name)) return i;
    return -1;
}

size_t vgg_kernel_floats(int i) { return (size_t)9 * kVgg[i].cin * kVgg[i].cout; }
// a backbone conv's kernel and bias on the device: the master weights when trained, the frozen constants otherwise
const float *vgg_w(const rpn_head_trainer *t, int i) { return (i >= t->bb_from ? t->d_w : t->d_frozen) + t->off_bk[i]; }
const float *vgg_b(const rpn_head_trainer *t, int i) { return (i >= t->bb_from ? t->d_w : t->d_frozen) + t->off_bb[i]; }
// a forward tensor the backward reads: conv i's ReLU output and its pooled form, from the input of the first trained conv upward
bool vgg_kept(const rpn_head_trainer *t, int i) { return i >= t->bb_from - 1; }
size_t vgg_act_floats(const rpn_head_trainer *t, int i) { return (size_t)t->max_batch * t->hs[i] * t->hs[i] * kVgg[i].cout; }
size_t vgg_pool_floats(const rpn_head_trainer *t, int i) { return (size_t)t->max_batch * (t->hs[i] / 2) * (t->hs[i] / 2) * kVgg[i].cout; }

size_t trainer_part_floats(const rpn_head_trainer *t)
{
    const long long P = (long long)t->max_batch * t->F * t->F;
    const size_t chunks = (size_t)((P + kChunkRows - 1) / kChunkRows);
    return std::max(std::max(chunks * 513 * t->nc, wgrad_ws_floats(t->cin, 512)), colsum_ws_floats(P, 512));
}

// the backbone's buffers, sized by max_batch and the trained span (about 3.5 GB at batch 8, 500 x 500, from block1_conv1)
int backbone_device(rpn_head_trainer *t)
{
    size_t pack = 0, ping = 0, grad = 0, wpart = 0;
    for (int i = 0; i < 13; ++i) {
        if (i > 0) pack = std::max(pack, t->ps_bb[i].floats());
        if (!vgg_kept(t, i)) ping = std::max(ping, std::max(vgg_act_floats(t, i), kVgg[i].pool ? vgg_pool_floats(t, i) : 0));
        if (i >= t->bb_from) {
            grad = std::max(grad, vgg_act_floats(t, i));
            wpart = std::max(wpart, wgrad_wide_ws_floats(t->max_batch, t->hs[i], t->hs[i], kVgg[i].cin, kVgg[i].cout));
        }
    }
    RPN_HIP_CHECK(hipMalloc(&t->d_frozen, std::max<size_t>(1, t->host_frozen.size()) * sizeof(float)));
    if (!t->host_frozen.empty())
        RPN_HIP_CHECK(hipMemcpy(t->d_frozen, t->host_frozen.data(), t->host_frozen.size() * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(hipMalloc(&t->d_pack, pack * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_wt, (size_t)9 * 512 * 512 * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_wpart, wpart * sizeof(float)));
    for (int u = 0; u < 2; ++u) {
        RPN_HIP_CHECK(hipMalloc(&t->d_grad[u], grad * sizeof(float)));
        if (ping) RPN_HIP_CHECK(hipMalloc(&t->d_ping[u], ping * sizeof(float)));
    }
    if (t->bb_from == 0) RPN_HIP_CHECK(hipMalloc(&t->d_img4, (size_t)t->max_batch * t->img * t->img * 4 * sizeof(float)));
    for (int i = 0; i < 13; ++i) {
        if (!vgg_kept(t, i)) continue;
        RPN_HIP_CHECK(hipMalloc(&t->d_act[i], vgg_act_floats(t, i) * sizeof(float)));
        if (kVgg[i].pool) RPN_HIP_CHECK(hipMalloc(&t->d_pool[i], vgg_pool_floats(t, i) * sizeof(float)));
    }
    return RPN_OK;
}

// ---- MobileNetV2: the stem and the inverted-residual blocks, each layer at its own resolution ---------------------------------------
// kind 0: 1x1 expand + BatchNorm + ReLU6, 1: depthwise 3x3 + BatchNorm + ReLU6 (stride 1 'same', or stride 2 behind Keras'
// correct_pad: mn_s2_geom), 2: 1x1 project + BatchNorm (linear) (+ the block's input when res), 3: the stem Conv1, a 3x3 stride-2
// conv from the 3-channel image + BatchNorm + ReLU6 (same padding rule).  No conv has a bias.  Keras names; the BatchNorm layer of
// conv X is "X_BN", Conv1's is "bn_Conv1".  expanded_conv has no expand conv.
constexpr int kMnLayers = kMnMax;
constexpr int kMnSpan = 21;                     // block_7_expand: the first layer at the feature map's own resolution (stride 16)
constexpr float kMnBnEps = 1e-3f, kMnBnMomentum = 0.999f;      // keras.applications.MobileNetV2
struct MnConv {
    std::string name, bn;
    int kind, cin, cout, stride;
    bool res;
};
const std::vector<MnConv> &mn_table()
{
    static const std::vector<MnConv> tab = [] {
        std::vector<MnConv> v;
        // (cin, cout, stride) of block_1 .. block_12 (keras.applications.MobileNetV2, alpha 1; expansion 6)
        const int blk[12][3] = {{16, 24, 2}, {24, 24, 1}, {24, 32, 2}, {32, 32, 1}, {32, 32, 1}, {32, 64, 2},
                                {64, 64, 1}, {64, 64, 1}, {64, 64, 1}, {64, 96, 1}, {96, 96, 1}, {96, 96, 1}};
        v.push_back({"Conv1", "bn_Conv1", 3, 3, 32, 2, false});
        v.push_back({"expanded_conv_depthwise", "expanded_conv_depthwise_BN", 1, 32, 32, 1, false});
        v.push_back({"expanded_conv_project", "expanded_conv_project_BN", 2, 32, 16, 1, false});
        for (int b = 0; b < 12; ++b) {
            const std::string pre = "block_" + std::to_string(b + 1) + "_";
            const int cin = blk[b][0], cout = blk[b][1], stride = blk[b][2];
            v.push_back({pre + "expand", pre + "expand_BN", 0, cin, 6 * cin, 1, false});
            v.push_back({pre + "depthwise", pre + "depthwise_BN", 1, 6 * cin, 6 * cin, stride, false});
            v.push_back({pre + "project", pre + "project_BN", 2, 6 * cin, cout, 1, cin == cout && stride == 1});
        }
        v.push_back({"block_13_expand", "block_13_expand_BN", 0, 96, 576, 1, false});
        return v;
    }();
    return tab;
}

// index of conv `name`, or of the conv whose BatchNorm layer is `name` (with_bn: "<conv>_BN" or the layer's Keras name)
int mn_index(const char *name, bool with_bn = false)
{
    const std::vector<MnConv> &tab = mn_table();
    for (int i = 0; i < kMnLayers; ++i)
        if (tab[i].name == name || (with_bn && (tab[i].name + "_BN" == name || tab[i].bn == name))) return i;
    return -1;
}

size_t mn_kernel_floats(int i)
{
    const MnConv &l = mn_table()[i];
    return l.kind == 1 ? (size_t)9 * l.cout : (l.kind == 3 ? (size_t)27 * l.cout : (size_t)l.cin * l.cout);
}

// pixels per image of layer i's input / output
size_t mn_pin(const rpn_head_trainer *t, int i) { return (size_t)t->mn_hin[i] * t->mn_hin[i]; }
size_t mn_pout(const rpn_head_trainer *t, int i) { return (size_t)t->mn_hout[i] * t->mn_hout[i]; }

// the span's buffers, sized by max_batch and the trained layers: per trained conv its output z (kept for the BatchNorm backward)
// and the normalised, activated tensor y (the next layer's input; the last one is d_feat)
// Every per-layer buffer is sized by that layer's own pixel count; the gradient buffers by the largest tensor they carry (mn_backward):
// d_mgr the block inputs, d_mt[0] the project outputs, d_mt[1 / 2] the expanded tensors (block_1_expand's 250 x 250 x 96 per image at
// 500 x 500) -- never less than the stride-16 span needs (F x F x 96 / 576: rpn_conv's input gradient lands in d_mt[1]).
int mn_device(rpn_head_trainer *t)
{
    const std::vector<MnConv> &tab = mn_table();
    const size_t B = (size_t)t->max_batch, PF = B * t->F * t->F;
    size_t pack = 0, wpart = 0, bstat = 0, part = bn_part_doubles((long long)PF, 576), gr = PF * 96, t0 = PF * 96, t12 = PF * 576;
    for (int i = t->mn_from; i < kMnLayers; ++i) {
        const MnConv &l = tab[i];
        const size_t Pi = B * mn_pin(t, i), Po = B * mn_pout(t, i);
        if (l.kind == 0 || l.kind == 2) pack = std::max(pack, t->ps_mn[i].floats());
        if (l.kind == 1)
            wpart = std::max(wpart, l.stride == 2 ? dwconv3x3_s2_wgrad_ws_floats((int)B, t->mn_hin[i], t->mn_hin[i], l.cout)
                                                  : dwconv3x3_wgrad_ws_floats((long long)Po, l.cout));
        else if (l.kind == 3)
            wpart = std::max(wpart, conv3x3_s2_cin3_wgrad_ws_floats((int)B, t->mn_hin[i], t->mn_hin[i], l.cout));
        else
            wpart = std::max(wpart, conv1x1_wgrad_ws_floats((long long)Po, l.cin, l.cout));
        part = std::max(part, bn_part_doubles((long long)Po, l.cout));
        if (l.kind == 0) gr = std::max(gr, Pi * l.cin);
        if (l.kind == 2) t0 = std::max(t0, Po * l.cout);
        if (l.kind != 3) t12 = std::max(t12, std::max(Pi * l.cin, l.kind == 2 ? (size_t)0 : Po * l.cout));
        else t12 = std::max(t12, Po * l.cout);
        bstat = t->off_bs[i] + (size_t)3 * l.cout;
        RPN_HIP_CHECK(hipMalloc(&t->d_mz[i], Po * l.cout * sizeof(float)));
        if (i < kMnLayers - 1) RPN_HIP_CHECK(hipMalloc(&t->d_my[i], Po * l.cout * sizeof(float)));
    }
    if (t->mn_from > 0) RPN_HIP_CHECK(hipMalloc(&t->d_x0, PF * tab[t->mn_from].cin * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mpack, std::max<size_t>(1, pack) * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mwpart, std::max<size_t>(1, wpart) * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mpart, part * sizeof(double)));
    RPN_HIP_CHECK(hipMalloc(&t->d_bstat, bstat * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_bn, t->host_bn.size() * sizeof(float)));
    RPN_HIP_CHECK(hipMemcpy(t->d_bn, t->host_bn.data(), t->host_bn.size() * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(hipMalloc(&t->d_wt, (size_t)9 * 512 * 576 * sizeof(float)));
    for (int u = 0; u < 2; ++u) RPN_HIP_CHECK(hipMalloc(&t->d_mgr[u], gr * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mt[0], t0 * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mt[1], t12 * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_mt[2], t12 * sizeof(float)));
    return RPN_OK;
}

// every device buffer of the trainer freed and its pointer reset (destroy, or a failed first-step allocation)
void trainer_free(rpn_head_trainer *t)
{
    float *mn[] = {t->d_bn, t->d_bstat, t->d_x0, t->d_mpack, t->d_mwpart, t->d_mgr[0], t->d_mgr[1], t->d_mt[0], t->d_mt[1], t->d_mt[2]};
    for (float *p : mn)
        if (p) (void)hipFree(p);
    if (t->d_mpart) (void)hipFree(t->d_mpart);
    for (int i = 0; i < kMnLayers; ++i) {
        if (t->d_mz[i]) (void)hipFree(t->d_mz[i]);
        if (t->d_my[i] && i < kMnLayers - 1) (void)hipFree(t->d_my[i]);           // (the last one is d_feat)
        t->d_mz[i] = t->d_my[i] = nullptr;
    }
    t->d_bn = t->d_bstat = t->d_x0 = t->d_mpack = t->d_mwpart = t->d_mgr[0] = t->d_mgr[1] = t->d_mt[0] = t->d_mt[1] = t->d_mt[2] = nullptr;
    t->d_mpart = nullptr;
    float *bufs[] = {t->d_w, t->d_g, t->d_m, t->d_v, t->d_pconv, t->d_phead, t->d_feat, t->d_S, t->d_reg, t->d_cls, t->d_graw, t->d_dz,
                     t->d_dS, t->d_part};
    for (float *p : bufs)
        if (p) (void)hipFree(p);
    if (t->d_lws) (void)hipFree(t->d_lws);
    t->d_w = t->d_g = t->d_m = t->d_v = t->d_pconv = t->d_phead = t->d_feat = t->d_S = t->d_reg = t->d_cls = nullptr;
    t->d_graw = t->d_dz = t->d_dS = t->d_part = nullptr;
    t->d_lws = nullptr;
    float *bb[] = {t->d_frozen, t->d_pack, t->d_wt, t->d_wpart, t->d_img4, t->d_ping[0], t->d_ping[1], t->d_grad[0], t->d_grad[1]};
    for (float *p : bb)
        if (p) (void)hipFree(p);
    for (int i = 0; i < 13; ++i) {
        if (t->d_act[i]) (void)hipFree(t->d_act[i]);
        if (t->d_pool[i]) (void)hipFree(t->d_pool[i]);
        t->d_act[i] = t->d_pool[i] = nullptr;
    }
    t->d_frozen = t->d_pack = t->d_wt = t->d_wpart = t->d_img4 = nullptr;
    t->d_ping[0] = t->d_ping[1] = t->d_grad[0] = t->d_grad[1] = nullptr;
}

int trainer_alloc(rpn_head_trainer *t)
{
    if (t->bb_from >= 0) {
        const int st = backbone_device(t);
        if (st != RPN_OK) return st;
    }
    if (t->mn_from >= 0) {
        const int st = mn_device(t);
        if (st != RPN_OK) return st;
    }
    const size_t P = (size_t)t->max_batch * t->F * t->F;
    float **bufs[] = {&t->d_w, &t->d_g, &t->d_m, &t->d_v, &t->d_pconv, &t->d_phead, &t->d_feat, &t->d_S, &t->d_reg, &t->d_cls,
                      &t->d_graw, &t->d_dz, &t->d_dS, &t->d_part};
    const size_t floats[] = {t->n, t->n, t->n, t->n, t->ps_conv.floats(), t->ps_head.floats(), P * t->cin, P * 512, P * 4 * t->K,
                             P * t->K, P * 5 * t->K, P * t->nc, P * 512, trainer_part_floats(t)};
    for (size_t i = 0; i < sizeof(floats) / sizeof(floats[0]); ++i) RPN_HIP_CHECK(hipMalloc(bufs[i], floats[i] * sizeof(float)));
    RPN_HIP_CHECK(hipMalloc(&t->d_lws, losses_ws_bytes((long long)P * t->K)));
    RPN_HIP_CHECK(hipMemcpy(t->d_w, t->host_w.data(), t->n * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(hipMemset(t->d_g, 0, t->n * sizeof(float)));       // no kernel writes the padding in front of an aligned slice
    RPN_HIP_CHECK(hipMemset(t->d_m, 0, t->n * sizeof(float)));
    RPN_HIP_CHECK(hipMemset(t->d_v, 0, t->n * sizeof(float)));
    return RPN_OK;
}

// all device buffers at the first step; d_w is set only when every allocation and upload succeeded (a failure frees what was
// allocated, so a later step starts over instead of running on a half-built trainer)
int trainer_device(rpn_head_trainer *t)
{
    if (!have_device()) return RPN_ERR_NO_DEVICE;
    if (t->d_w) return RPN_OK;
    const int st = trainer_alloc(t);
    if (st != RPN_OK) trainer_free(t);
    return st;
}

// The whole VGG16 forward in exact float32 from the trainer's weights (the frozen prefix included), keeping what the backward
// reads -> the block5_conv3 output (B, F, F, 512).  Weights are packed on the device at every step: the trained ones move.
hipError_t backbone_forward(rpn_head_trainer *t, const float *d_imgs, int B, hipStream_t s, const float **feat)
{
    const float *in = d_imgs;
    int ping = 0;
    auto next = [&](float *kept) -> float * {
        if (kept) return kept;
        float *p = t->d_ping[ping];
        ping ^= 1;
        return p;
    };
    if (t->bb_from == 0) {
        const hipError_t e = launch_pad_channels3to4(d_imgs, (long long)B * t->img * t->img, t->d_img4, s);
        if (e != hipSuccess) return e;
    }
    for (int i = 0; i < 13; ++i) {
        const int H = t->hs[i];
        float *out = next(t->d_act[i]);
        hipError_t e;
        if (i == 0) {
            e = launch_conv_cin3(in, vgg_w(t, 0), vgg_b(t, 0), out, B, H, H, H, H, kVgg[0].cout, 1, 1, 1, ACT_RELU, 0, false, s);
        } else {
            pack_weights_device(t->ps_bb[i], vgg_w(t, i), t->d_pack, s);
            ConvArgs a{};
            a.x = in; a.w = t->d_pack; a.bias = vgg_b(t, i); a.residual = nullptr;
            a.out = out; a.out2 = nullptr;
            a.B = B; a.H = H; a.W = H; a.Cin = kVgg[i].cin; a.OH = H; a.OW = H; a.Cout = kVgg[i].cout;
            a.R = 3; a.S = 3; a.stride = 1; a.pad_t = 1; a.pad_l = 1; a.ps = t->ps_bb[i];
            a.act = ACT_RELU; a.act2 = ACT_LINEAR; a.split = kVgg[i].cout; a.ld1 = kVgg[i].cout; a.ld2 = 0;
            e = launch_conv_f32(a, s);
        }
        if (e != hipSuccess) return e;
        in = out;
        if (kVgg[i].pool) {
            float *po = next(t->d_pool[i]);
            e = launch_maxpool2x2(in, B, H, H, kVgg[i].cout, po, s);
            if (e != hipSuccess) return e;
            in = po;
        }
    }
    *feat = in;
    return hipSuccess;
}

// From dS (rpn_conv's pre-activation gradient) down to the first trained conv: dgrad (+ the ReLU mask of its input) or dgrad + the
// max-pool backward (+ the mask of the pooled conv) between layers, the weight and bias gradient of each trained conv.  add (B,F,F,cin)
// or NULL: a second stage's gradient with respect to the tap (the post-ReLU block5_conv3 output); it joins the RPN's gradient in the
// first dgrad's epilogue, before block5_conv3's ReLU mask: (dgrad + add) [feat > 0].
hipError_t backbone_backward(rpn_head_trainer *t, int B, const float *add, hipStream_t s)
{
    float *g = t->d_grad[0], *h = t->d_grad[1];
    const int F = t->hs[12];
    hipError_t e = launch_conv3x3_dgrad(t->d_dS, t->d_w + t->off_ck, t->d_act[12], add, B, F, F, t->cin, 512, t->d_wt, g, s);
    for (int i = 12; i >= t->bb_from && e == hipSuccess; --i) {
        const int H = t->hs[i];
        const float *x = i == 0 ? t->d_img4 : (kVgg[i - 1].pool ? t->d_pool[i - 1] : t->d_act[i - 1]);
        e = launch_wgrad_wide(x, g, B, H, H, kVgg[i].cin, kVgg[i].cout, t->d_wpart, t->d_g + t->off_bk[i], t->d_g + t->off_bb[i], s);
        if (e != hipSuccess || i == t->bb_from) break;
        if (kVgg[i - 1].pool) {
            e = launch_conv3x3_dgrad(g, vgg_w(t, i), nullptr, nullptr, B, H, H, kVgg[i].cin, kVgg[i].cout, t->d_wt, h, s);
            if (e == hipSuccess) e = launch_maxpool2x2_backward(t->d_act[i - 1], h, B, t->hs[i - 1], t->hs[i - 1], kVgg[i - 1].cout, g, s);
        } else {
            e = launch_conv3x3_dgrad(g, vgg_w(t, i), t->d_act[i - 1], nullptr, B, H, H, kVgg[i].cin, kVgg[i].cout, t->d_wt, h, s);
            std::swap(g, h);
        }
    }
    return e;
}

// The span's forward in exact float32 from the trainer's unfolded parameters, on top of the frozen prefix (the handle's ops up to
// mn_x0; from Conv1 there is none: the span's input is the image batch).  train: BatchNorm normalises with the batch statistics and
// updates the moving ones; else with the moving statistics (inference mode, nothing updated).  Every conv output z and every layer
// output y is kept.  -> the block_13_expand output in d_feat.
int mn_forward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, bool train, hipStream_t s)
{
    const std::vector<MnConv> &tab = mn_table();
    if (t->mn_from > 0) {
        const int e0 = model_features_at(t->m, t->mn_x0.c_str(), d_imgs, B, t->d_x0, s);
        if (e0 != RPN_OK) return e0;
    }
    t->d_my[kMnLayers - 1] = t->d_feat;
    for (int i = t->mn_from; i < kMnLayers; ++i) {
        const MnConv &l = tab[i];
        const int H = t->mn_hin[i], F = t->mn_hout[i];
        const long long P = (long long)B * F * F;
        const float *in = i == t->mn_from ? (i == 0 ? d_imgs : t->d_x0) : t->d_my[i - 1];
        const float *w = t->d_w + t->off_mk[i];
        hipError_t e;
        if (l.kind == 1) {
            const int pad = l.stride == 2 ? H % 2 : 1;
            e = launch_dwconv3x3(in, B, H, H, l.cout, w, nullptr, l.stride, pad, pad, F, F, ACT_LINEAR, t->d_mz[i], s);
        } else if (l.kind == 3) {
            e = launch_conv_cin3(in, w, nullptr, t->d_mz[i], B, H, H, F, F, l.cout, 2, H % 2, H % 2, ACT_LINEAR, 0, false, s);
        } else {
            pack_weights_device(t->ps_mn[i], w, t->d_mpack, s);
            ConvArgs a{};
            a.x = in; a.w = t->d_mpack; a.bias = nullptr; a.residual = nullptr;
            a.out = t->d_mz[i]; a.out2 = nullptr;
            a.B = B; a.H = F; a.W = F; a.Cin = l.cin; a.OH = F; a.OW = F; a.Cout = l.cout;
            a.R = 1; a.S = 1; a.stride = 1; a.pad_t = 0; a.pad_l = 0; a.ps = t->ps_mn[i];
            a.act = ACT_LINEAR; a.act2 = ACT_LINEAR; a.split = l.cout; a.ld1 = l.cout; a.ld2 = 0;
            e = launch_conv_f32(a, s);
        }
        float *mean = t->d_bstat + t->off_bs[i], *var = mean + l.cout, *rstd = var + l.cout;
        float *mmean = t->d_bn + t->off_ms[i], *mvar = mmean + l.cout;
        if (e == hipSuccess) {
            if (train) {
                e = launch_bn_train_stats(t->d_mz[i], P, l.cout, kMnBnEps, kMnBnMomentum, t->d_mpart, mean, var, rstd, mmean, mvar, s);
            } else {
                e = hipMemcpyAsync(mean, mmean, (size_t)2 * l.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess) e = launch_bn_rstd(mvar, l.cout, kMnBnEps, rstd, s);
            }
        }
        const float *res = (l.kind == 2 && l.res) ? (i - 2 == t->mn_from ? t->d_x0 : t->d_my[i - 3]) : nullptr;
        if (e == hipSuccess)
            e = launch_bn_apply(t->d_mz[i], P, l.cout, mean, rstd, t->d_w + t->off_mg[i], t->d_w + t->off_mb[i], l.kind != 2, res, t->d_my[i], s);
        if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s: %s", what, l.name.c_str(), hipGetErrorString(e));
    }
    return RPN_OK;
}

// From dS (rpn_conv's pre-activation gradient) down to the first trained layer.  g: the gradient of the current layer's output.  A
// residual block's output gradient stays in d_mgr[a] until the block's expand dgrad adds it to what that conv sends to the block's
// input (the dgrad's epilogue: no atomics, no extra pass).  add (B,F,F,cin) or NULL: a second stage's gradient with respect to the
// tap (block_13_expand after its ReLU6); it joins the RPN's gradient in the first dgrad's epilogue, and the BatchNorm backward that
// follows applies the ReLU6 mask to the sum.
hipError_t mn_backward(rpn_head_trainer *t, const float *d_imgs, int B, const float *add, hipStream_t s)
{
    const std::vector<MnConv> &tab = mn_table();
    float *g = t->d_mt[1];
    const float *gres = nullptr;
    int a = 1;
    hipError_t e = launch_conv3x3_dgrad(t->d_dS, t->d_w + t->off_ck, nullptr, add, B, t->F, t->F, t->cin, 512, t->d_wt, g, s);
    for (int i = kMnLayers - 1; i >= t->mn_from && e == hipSuccess; --i) {
        const MnConv &l = tab[i];
        const int H = t->mn_hin[i], F = t->mn_hout[i];
        const long long P = (long long)B * F * F;
        const float *in = i == t->mn_from ? (i == 0 ? d_imgs : t->d_x0) : t->d_my[i - 1];
        const float *w = t->d_w + t->off_mk[i];
        const float *mean = t->d_bstat + t->off_bs[i], *rstd = mean + 2 * l.cout;
        float *dz = g;
        if (l.kind == 2) {
            if (l.res) gres = g;
            dz = t->d_mt[0];
        }
        e = launch_bn_backward(t->d_mz[i], g, P, l.cout, mean, rstd, t->d_w + t->off_mg[i], t->d_w + t->off_mb[i], l.kind != 2, t->d_mpart,
                               t->d_g + t->off_mg[i], t->d_g + t->off_mb[i], dz, s);
        if (e != hipSuccess) break;
        if (l.kind == 3) {                      // the stem: its input is the image, so there is no data gradient
            e = launch_conv3x3_s2_cin3_wgrad(in, dz, B, H, H, l.cout, t->d_mwpart, t->d_g + t->off_mk[i], s);
            break;
        }
        if (l.kind == 1) {
            float *dx = dz == t->d_mt[1] ? t->d_mt[2] : t->d_mt[1];
            if (l.stride == 2) {
                e = launch_dwconv3x3_s2_wgrad(in, dz, B, H, H, l.cout, t->d_mwpart, t->d_g + t->off_mk[i], s);
                if (e == hipSuccess) e = launch_dwconv3x3_s2_dgrad(dz, w, B, H, H, l.cout, dx, s);
            } else {
                e = launch_dwconv3x3_wgrad(in, dz, B, F, F, l.cout, t->d_mwpart, t->d_g + t->off_mk[i], s);
                if (e == hipSuccess) e = launch_dwconv3x3_dgrad(dz, w, B, F, F, l.cout, dx, s);
            }
            g = dx;
            continue;
        }
        e = launch_conv1x1_wgrad(in, dz, P, l.cin, l.cout, t->d_mwpart, t->d_g + t->off_mk[i], s);
        if (e != hipSuccess || i == t->mn_from) break;
        if (l.kind == 2) {
            g = t->d_mt[1];
            e = launch_conv1x1_dgrad(dz, w, nullptr, P, l.cin, l.cout, g, s);
        } else {
            float *dx = t->d_mgr[a ^ 1];
            e = launch_conv1x1_dgrad(dz, w, gres, P, l.cin, l.cout, dx, s);
            a ^= 1;
            g = dx;
            gres = nullptr;
        }
    }
    return e;
}

}  // namespace

extern "C" int rpn_head_trainer_create(rpn_model *m, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_head_trainer_create: null argument");
    int cin, F, K, mb;
    model_train_dims(m, &cin, &F, &K, &mb);
    RPN_REQUIRE(cin % 4 == 0 && 5 * K <= 64 && K >= 1, "rpn_head_trainer_create: unsupported head (Cin %d, K %d)", cin, K);
    rpn_head_trainer *t = new rpn_head_trainer();
    t->m = m; t->cin = cin; t->F = F; t->K = K; t->max_batch = mb; t->nc = 5 * K;
    t->off_ck = 0;
    t->off_cb = (size_t)9 * cin * 512;
    t->off_hk = t->off_cb + 512;
    t->off_hb = t->off_hk + (size_t)512 * t->nc;
    t->n = t->off_hb + t->nc;
    t->host_w.assign(t->n, 0.0f);
    t->ps_conv = packed_shape(3, 3, cin, 512);
    t->ps_head = packed_shape(1, 1, 512, t->nc);
    *out = t;
    return RPN_OK;
}

// the MobileNetV2 trainer from layer `from` of mn_table() up: an expand conv of the stride-16 span, or 0 (Conv1: the whole model)
static int mn_trainer_create(rpn_model *m, int from, int img, const char *what, rpn_head_trainer **out)
{
    const std::vector<MnConv> &tab = mn_table();
    rpn_head_trainer *t = nullptr;
    const int st = rpn_head_trainer_create(m, &t);
    if (st != RPN_OK) return st;
    for (int i = 0, h = img; i < kMnLayers; ++i) {          // each layer's own resolution, from the image down
        t->mn_hin[i] = h;
        if (tab[i].stride == 2) {
            int pad;
            mn_s2_geom(h, &pad, &h);
        }
        t->mn_hout[i] = h;
    }
    bool ok = t->cin == 576 && t->mn_hout[kMnLayers - 1] == t->F && t->F >= 1;
    if (from > 0) {
        t->mn_x0 = tab[from - 1].name;
        int h = 0, w = 0, c = 0;
        ok = ok && model_tensor_shape(m, t->mn_x0.c_str(), &h, &w, &c) == RPN_OK && h == t->F && w == t->F && c == tab[from].cin;
    } else {
        ok = ok && (long long)t->max_batch * t->mn_hout[0] * t->mn_hout[0] <= (1ll << 21);       // the 1x1 GEMMs' row count (gemm_ok)
    }
    if (!ok) {
        rpn_head_trainer_destroy(t);
        return fail(RPN_ERR_UNSUPPORTED, "%s: unexpected MobileNetV2 graph below '%s'", what, tab[from].name.c_str());
    }
    t->img = img;
    t->mn_from = from;
    size_t state = 0, bstat = 0;
    for (int i = from; i < kMnLayers; ++i) {
        t->off_mk[i] = (t->n + 3) & ~(size_t)3;     // the kernels read these slices as float4 (every slice's length is a multiple of 4)
        t->off_mg[i] = t->off_mk[i] + mn_kernel_floats(i);
        t->off_mb[i] = t->off_mg[i] + tab[i].cout;
        t->n = t->off_mb[i] + tab[i].cout;
        t->off_ms[i] = state;
        state += (size_t)2 * tab[i].cout;
        t->off_bs[i] = bstat;
        bstat += (size_t)3 * tab[i].cout;
        if (tab[i].kind == 0 || tab[i].kind == 2) t->ps_mn[i] = packed_shape(1, 1, tab[i].cin, tab[i].cout);
    }
    t->host_w.assign(t->n, 0.0f);
    t->host_bn.assign(state, 0.0f);
    *out = t;
    return RPN_OK;
}

extern "C" int rpn_model_trainer_create_full(rpn_model *m, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_model_trainer_create_full: null argument");
    int backbone, img;
    model_train_backbone(m, &backbone, &img);
    if (backbone == RPN_BACKBONE_MOBILENET_V2) return mn_trainer_create(m, 0, img, "rpn_model_trainer_create_full", out);
    RPN_REQUIRE(backbone == RPN_BACKBONE_VGG16, "rpn_model_trainer_create_full: unknown backbone %d", backbone);
    return rpn_model_trainer_create(m, kVgg[0].name, out);
}

extern "C" int rpn_model_trainer_create(rpn_model *m, const char *train_from, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_model_trainer_create: null argument");
    if (!train_from) return rpn_head_trainer_create(m, out);
    int backbone, img;
    model_train_backbone(m, &backbone, &img);
    if (backbone == RPN_BACKBONE_MOBILENET_V2) {
        const std::vector<MnConv> &tab = mn_table();
        const int from = mn_index(train_from);
        RPN_REQUIRE(from >= kMnSpan && tab[from].kind == 0,
                    "rpn_model_trainer_create: '%s' does not start a trainable span of MobileNetV2: accepted are block_7_expand .. "
                    "block_12_expand and block_13_expand (that layer and every layer above it train with the head); otherwise this "
                    "backbone trains its head only -- the layer is a VGG16 conv, is not the first layer of a block, or lies below "
                    "block_7_expand (rpn_model_trainer_create_full trains the whole model)", train_from);
        return mn_trainer_create(m, from, img, "rpn_model_trainer_create", out);
    }
    RPN_REQUIRE(backbone == RPN_BACKBONE_VGG16, "rpn_model_trainer_create: unknown backbone %d", backbone);
    const int from = vgg_index(train_from);
    RPN_REQUIRE(from >= 0, "rpn_model_trainer_create: '%s' is not a VGG16 conv (block1_conv1 .. block5_conv3)", train_from);
    int hs[13];
    for (int i = 0, h = img; i < 13; ++i) {
        hs[i] = h;
        if (kVgg[i].pool) h /= 2;
    }
    rpn_head_trainer *t = nullptr;
    const int st = rpn_head_trainer_create(m, &t);
    if (st != RPN_OK) return st;
    if (t->cin != 512 || t->F != hs[12] || hs[12] < 1) {
        rpn_head_trainer_destroy(t);
        return fail(RPN_ERR_UNSUPPORTED, "rpn_model_trainer_create: unexpected VGG16 graph (features %d, F %d)", t->cin, t->F);
    }
    t->bb_from = from;
    t->img = img;
    size_t frozen = 0;
    for (int i = 0; i < 13; ++i) {
        t->hs[i] = hs[i];
        size_t &off = i >= from ? t->n : frozen;
        t->off_bk[i] = off;
        t->off_bb[i] = off + vgg_kernel_floats(i);
        off = t->off_bb[i] + kVgg[i].cout;
        if (i > 0) t->ps_bb[i] = packed_shape(3, 3, kVgg[i].cin, kVgg[i].cout);
    }
    t->host_w.assign(t->n, 0.0f);
    t->host_frozen.assign(frozen, 0.0f);
    *out = t;
    return RPN_OK;
}

extern "C" void rpn_head_trainer_destroy(rpn_head_trainer *t)
{
    if (!t) return;
    trainer_free(t);
    delete t;
}

extern "C" int rpn_head_trainer_set_layer(rpn_head_trainer *t, const char *name, const float *kernel, const float *bias)
{
    RPN_REQUIRE(t && name && kernel, "rpn_head_trainer_set_layer: null argument");
    t->pending_B = 0;                           // new parameters: a pending forward no longer matches them
    const int mi = t->mn_from >= 0 ? mn_index(name) : -1;
    if (mi >= 0) {
        // a MobileNetV2 conv of the span: the kernel alone (these convs have no bias; rpn_head_trainer_set_bn carries the BatchNorm)
        RPN_REQUIRE(mi >= t->mn_from, "rpn_head_trainer_set_layer: '%s' is frozen (training starts at %s): it runs on the model handle", name,
                    mn_table()[t->mn_from].name.c_str());
        RPN_REQUIRE(!bias, "rpn_head_trainer_set_layer: '%s' has no bias (pass NULL)", name);
        if (t->d_w) RPN_HIP_CHECK(hipMemcpy(t->host_w.data(), t->d_w, t->n * sizeof(float), hipMemcpyDeviceToHost));
        memcpy(&t->host_w[t->off_mk[mi]], kernel, mn_kernel_floats(mi) * sizeof(float));
        if (t->d_w) RPN_HIP_CHECK(hipMemcpy(t->d_w, t->host_w.data(), t->n * sizeof(float), hipMemcpyHostToDevice));
        t->mn_loaded[mi] = true;
        return RPN_OK;
    }
    RPN_REQUIRE(bias, "rpn_head_trainer_set_layer: null argument");
    const int li = layer_index(name);
    const int bi = t->bb_from >= 0 ? vgg_index(name) : -1;
    RPN_REQUIRE(li >= 0 || bi >= 0, "rpn_head_trainer_set_layer: '%s' is not trained (the backbone is frozen: rpn_conv, rpn_reg, rpn_cls only)",
                name);
    if (bi >= 0) {
        // a trained conv: its slices of the master weights; a frozen one: the constants
        const bool trained = bi >= t->bb_from;
        std::vector<float> &w = trained ? t->host_w : t->host_frozen;
        float *dev = trained ? t->d_w : t->d_frozen;
        if (dev && trained) RPN_HIP_CHECK(hipMemcpy(w.data(), dev, w.size() * sizeof(float), hipMemcpyDeviceToHost));
        memcpy(&w[t->off_bk[bi]], kernel, vgg_kernel_floats(bi) * sizeof(float));
        memcpy(&w[t->off_bb[bi]], bias, kVgg[bi].cout * sizeof(float));
        if (dev) RPN_HIP_CHECK(hipMemcpy(dev, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        t->bb_loaded[bi] = true;
        return RPN_OK;
    }
    // the layer's slices of the flat master buffer: (offset, row length, row stride, rows) for the kernel, then the bias
    std::vector<float> &w = t->host_w;
    if (t->d_w) RPN_HIP_CHECK(hipMemcpy(w.data(), t->d_w, t->n * sizeof(float), hipMemcpyDeviceToHost));
    if (li == 0) {
        memcpy(&w[t->off_ck], kernel, (size_t)9 * t->cin * 512 * sizeof(float));
        memcpy(&w[t->off_cb], bias, 512 * sizeof(float));
    } else {
        const int col = li == 1 ? 0 : 4 * t->K, width = li == 1 ? 4 * t->K : t->K;
        for (int k = 0; k < 512; ++k) memcpy(&w[t->off_hk + (size_t)k * t->nc + col], kernel + (size_t)k * width, width * sizeof(float));
        memcpy(&w[t->off_hb + col], bias, width * sizeof(float));
    }
    if (t->d_w) RPN_HIP_CHECK(hipMemcpy(t->d_w, w.data(), t->n * sizeof(float), hipMemcpyHostToDevice));
    t->loaded[li] = true;
    return RPN_OK;
}

// a head layer's slices of the master weights (grad == 0) or of the last step's gradient (grad == 1) -> HOST kernel / bias
static int trainer_read(rpn_head_trainer *t, const char *what, const char *name, float *kernel, float *bias, int grad, void *stream)
{
    RPN_REQUIRE(t && name && kernel, "%s: null argument", what);
    const int mi = t->mn_from >= 0 ? mn_index(name) : -1;
    if (mi >= 0) {
        RPN_REQUIRE(mi >= t->mn_from, "%s: layer '%s' is frozen (training starts at %s): it runs on the model handle", what, name,
                    mn_table()[t->mn_from].name.c_str());
        RPN_REQUIRE(!bias, "%s: '%s' has no bias (pass NULL)", what, name);
        RPN_REQUIRE(t->mn_loaded[mi], "%s: layer '%s' was never set", what, name);
        RPN_REQUIRE(!grad || t->t > 0, "%s: no update step has run", what);
        if (t->d_w) {
            RPN_HIP_CHECK(hipMemcpyAsync(kernel, (grad ? t->d_g : t->d_w) + t->off_mk[mi], mn_kernel_floats(mi) * sizeof(float),
                                         hipMemcpyDeviceToHost, as_stream(stream)));
            RPN_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
        } else {
            memcpy(kernel, &t->host_w[t->off_mk[mi]], mn_kernel_floats(mi) * sizeof(float));
        }
        return RPN_OK;
    }
    const int li = layer_index(name);
    const int bi = t->bb_from >= 0 ? vgg_index(name) : -1;
    if (li < 0 && bi < 0 && t->mn_from >= 0) {     // a layer of the model below the span, or no layer of it at all
        RPN_REQUIRE(model_has_layer(t->m, name), "%s: the model has no layer named '%s'", what, name);
        return fail(RPN_ERR_INVALID, "%s: '%s' is frozen (training starts at %s): it runs on the model handle", what, name,
                    mn_table()[t->mn_from].name.c_str());
    }
    RPN_REQUIRE(bias, "%s: null argument", what);
    RPN_REQUIRE(li >= 0 || bi >= 0, "%s: '%s' is not trained (rpn_conv, rpn_reg, rpn_cls)", what, name);
    RPN_REQUIRE(li >= 0 ? t->loaded[li] : t->bb_loaded[bi], "%s: layer '%s' was never set", what, name);
    RPN_REQUIRE(!grad || bi < 0 || bi >= t->bb_from, "%s: layer '%s' is frozen (training starts at %s): it has no gradient", what, name,
                bi >= 0 ? kVgg[std::max(t->bb_from, 0)].name : "");
    RPN_REQUIRE(!grad || t->t > 0, "%s: no update step has run", what);
    if (bi >= 0 && bi < t->bb_from) {           // a frozen conv: its constants
        memcpy(kernel, &t->host_frozen[t->off_bk[bi]], vgg_kernel_floats(bi) * sizeof(float));
        memcpy(bias, &t->host_frozen[t->off_bb[bi]], kVgg[bi].cout * sizeof(float));
        return RPN_OK;
    }
    std::vector<float> gbuf;
    if (grad) gbuf.resize(t->n);
    std::vector<float> &w = grad ? gbuf : t->host_w;
    if (t->d_w) {
        RPN_HIP_CHECK(hipMemcpyAsync(w.data(), grad ? t->d_g : t->d_w, t->n * sizeof(float), hipMemcpyDeviceToHost, as_stream(stream)));
        RPN_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
    }
    if (bi >= 0) {
        memcpy(kernel, &w[t->off_bk[bi]], vgg_kernel_floats(bi) * sizeof(float));
        memcpy(bias, &w[t->off_bb[bi]], kVgg[bi].cout * sizeof(float));
    } else if (li == 0) {
        memcpy(kernel, &w[t->off_ck], (size_t)9 * t->cin * 512 * sizeof(float));
        memcpy(bias, &w[t->off_cb], 512 * sizeof(float));
    } else {
        const int col = li == 1 ? 0 : 4 * t->K, width = li == 1 ? 4 * t->K : t->K;
        for (int k = 0; k < 512; ++k) memcpy(kernel + (size_t)k * width, &w[t->off_hk + (size_t)k * t->nc + col], width * sizeof(float));
        memcpy(bias, &w[t->off_hb + col], width * sizeof(float));
    }
    return RPN_OK;
}

extern "C" int rpn_head_trainer_get_layer(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream)
{
    return trainer_read(t, "rpn_head_trainer_get_layer", name, kernel, bias, 0, stream);
}

extern "C" int rpn_head_trainer_get_gradient(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream)
{
    return trainer_read(t, "rpn_head_trainer_get_gradient", name, kernel, bias, 1, stream);
}

// ---- the BatchNorm of a trained MobileNetV2 conv (named by the conv or by its BatchNorm layer, "<conv>_BN") --------------------------
extern "C" int rpn_head_trainer_set_bn(rpn_head_trainer *t, const char *name, const float *gamma, const float *beta, const float *mean,
                                       const float *var)
{
    RPN_REQUIRE(t && name && gamma && beta && mean && var, "rpn_head_trainer_set_bn: null argument");
    t->pending_B = 0;                           // new parameters: a pending forward no longer matches them
    const int mi = t->mn_from >= 0 ? mn_index(name, true) : -1;
    RPN_REQUIRE(mi >= 0, "rpn_head_trainer_set_bn: '%s' is not a BatchNorm this trainer trains", name);
    RPN_REQUIRE(mi >= t->mn_from, "rpn_head_trainer_set_bn: '%s' is frozen (training starts at %s): it runs on the model handle", name,
                mn_table()[t->mn_from].name.c_str());
    const size_t C = (size_t)mn_table()[mi].cout;
    if (t->d_w) {
        RPN_HIP_CHECK(hipMemcpy(t->host_w.data(), t->d_w, t->n * sizeof(float), hipMemcpyDeviceToHost));
        RPN_HIP_CHECK(hipMemcpy(t->host_bn.data(), t->d_bn, t->host_bn.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    memcpy(&t->host_w[t->off_mg[mi]], gamma, C * sizeof(float));
    memcpy(&t->host_w[t->off_mb[mi]], beta, C * sizeof(float));
    memcpy(&t->host_bn[t->off_ms[mi]], mean, C * sizeof(float));
    memcpy(&t->host_bn[t->off_ms[mi] + C], var, C * sizeof(float));
    if (t->d_w) {
        RPN_HIP_CHECK(hipMemcpy(t->d_w, t->host_w.data(), t->n * sizeof(float), hipMemcpyHostToDevice));
        RPN_HIP_CHECK(hipMemcpy(t->d_bn, t->host_bn.data(), t->host_bn.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    t->mn_bn_loaded[mi] = true;
    return RPN_OK;
}

// gamma, beta (grad: their gradients at the last update step) and, !grad, the moving mean / variance -> HOST arrays
static int trainer_read_bn(rpn_head_trainer *t, const char *what, const char *name, float *a, float *b, float *mean, float *var, int grad,
                           void *stream)
{
    RPN_REQUIRE(t && name && a && b && (grad || (mean && var)), "%s: null argument", what);
    const int mi = t->mn_from >= 0 ? mn_index(name, true) : -1;
    RPN_REQUIRE(mi >= 0, "%s: '%s' is not a BatchNorm this trainer trains", what, name);
    RPN_REQUIRE(mi >= t->mn_from, "%s: '%s' is frozen (training starts at %s): it runs on the model handle", what, name,
                mn_table()[t->mn_from].name.c_str());
    RPN_REQUIRE(t->mn_bn_loaded[mi], "%s: BatchNorm '%s' was never set", what, name);
    RPN_REQUIRE(!grad || t->t > 0, "%s: no update step has run", what);
    const size_t C = (size_t)mn_table()[mi].cout;
    if (t->d_w) {
        hipStream_t s = as_stream(stream);
        const float *src = grad ? t->d_g : t->d_w;
        RPN_HIP_CHECK(hipMemcpyAsync(a, src + t->off_mg[mi], C * sizeof(float), hipMemcpyDeviceToHost, s));
        RPN_HIP_CHECK(hipMemcpyAsync(b, src + t->off_mb[mi], C * sizeof(float), hipMemcpyDeviceToHost, s));
        if (!grad) {
            RPN_HIP_CHECK(hipMemcpyAsync(mean, t->d_bn + t->off_ms[mi], C * sizeof(float), hipMemcpyDeviceToHost, s));
            RPN_HIP_CHECK(hipMemcpyAsync(var, t->d_bn + t->off_ms[mi] + C, C * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        RPN_HIP_CHECK(hipStreamSynchronize(s));
        return RPN_OK;
    }
    memcpy(a, &t->host_w[t->off_mg[mi]], C * sizeof(float));
    memcpy(b, &t->host_w[t->off_mb[mi]], C * sizeof(float));
    memcpy(mean, &t->host_bn[t->off_ms[mi]], C * sizeof(float));
    memcpy(var, &t->host_bn[t->off_ms[mi] + C], C * sizeof(float));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_get_bn(rpn_head_trainer *t, const char *name, float *gamma, float *beta, float *mean, float *var, void *stream)
{
    return trainer_read_bn(t, "rpn_head_trainer_get_bn", name, gamma, beta, mean, var, 0, stream);
}

extern "C" int rpn_head_trainer_get_bn_gradient(rpn_head_trainer *t, const char *name, float *dgamma, float *dbeta, void *stream)
{
    return trainer_read_bn(t, "rpn_head_trainer_get_bn_gradient", name, dgamma, dbeta, nullptr, nullptr, 1, stream);
}

// ---- a step in two halves: forward + losses (+ the loss gradients), then head backward, backbone backward and Adam ------------------
// `what` names the public entry in the messages.  rpn_head_trainer_step = both halves back to back: the same launches in the same
// order on the same buffers as the closed call it was.
static int trainer_check_forward(const rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_bbox_deltas,
                                 const float *d_bbox_labels, const float *d_losses)
{
    RPN_REQUIRE(t && d_imgs && d_bbox_deltas && d_bbox_labels && d_losses, "%s: null argument", what);
    RPN_REQUIRE(B >= 1 && B <= t->max_batch, "%s: batch %d outside [1, %d]", what, B, t->max_batch);
    return RPN_OK;
}

static int trainer_check_adam(const char *what, float lr, float beta_1, float beta_2, float epsilon)
{
    RPN_REQUIRE(std::isfinite(lr) && lr >= 0.0f && beta_1 >= 0.0f && beta_1 < 1.0f && beta_2 >= 0.0f && beta_2 < 1.0f &&
                    std::isfinite(epsilon) && epsilon >= 0.0f,
                "%s: bad Adam hyper-parameters", what);
    return RPN_OK;
}

static int trainer_check_loaded(const rpn_head_trainer *t, const char *what)
{
    for (int i = 0; i < 3; ++i) RPN_REQUIRE(t->loaded[i], "%s: layer '%s' was never set", what, kHeadLayers[i]);
    if (t->bb_from >= 0)
        for (int i = 0; i < 13; ++i) RPN_REQUIRE(t->bb_loaded[i], "%s: layer '%s' was never set", what, kVgg[i].name);
    for (int i = std::max(t->mn_from, 0); t->mn_from >= 0 && i < kMnLayers; ++i)
        RPN_REQUIRE(t->mn_loaded[i] && t->mn_bn_loaded[i], "%s: layer '%s' or its BatchNorm was never set", what,
                    mn_table()[i].name.c_str());
    return RPN_OK;
}

// the arguments are checked by the caller
static int trainer_forward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_bbox_deltas,
                           const float *d_bbox_labels, int train, float *d_losses, void *stream)
{
    t->pending_B = 0;                           // whatever happens below, the buffers of an earlier forward are being overwritten:
    t->pending_imgs = nullptr;                  // nothing is pending, and feature / outputs have nothing to return until this one is done
    t->last_B = 0;
    t->d_tap = nullptr;
    const int st = trainer_device(t);
    if (st != RPN_OK) return st;
    hipStream_t s = as_stream(stream);
    const int F = t->F, K = t->K, nc = t->nc;
    const long long P = (long long)B * F * F;
    const float *feat = t->d_feat;
    if (t->bb_from >= 0) {
        // a trained backbone: the whole VGG16 in exact float32 from the trainer's weights
        const hipError_t eb = backbone_forward(t, d_imgs, B, s, &feat);
        if (eb != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: backbone: %s", what, hipGetErrorString(eb));
    } else if (t->mn_from >= 0) {
        // a trained MobileNetV2 span: BatchNorm in training mode on an update step, in inference mode on an evaluation
        const int e0 = mn_forward(t, what, d_imgs, B, train != 0, s);
        if (e0 != RPN_OK) return e0;
    } else {
        const int e0 = model_features(t->m, d_imgs, B, t->d_feat, s);
        if (e0 != RPN_OK) return e0;
    }
    // head forward in exact float32 from the master weights
    pack_weights_device(t->ps_conv, t->d_w + t->off_ck, t->d_pconv, s);
    pack_weights_device(t->ps_head, t->d_w + t->off_hk, t->d_phead, s);
    ConvArgs a{};
    a.x = feat; a.w = t->d_pconv; a.bias = t->d_w + t->off_cb; a.residual = nullptr;
    a.out = t->d_S; a.out2 = nullptr;
    a.B = B; a.H = F; a.W = F; a.Cin = t->cin; a.OH = F; a.OW = F; a.Cout = 512;
    a.R = 3; a.S = 3; a.stride = 1; a.pad_t = 1; a.pad_l = 1; a.ps = t->ps_conv;
    a.act = ACT_RELU; a.act2 = ACT_LINEAR; a.split = 512; a.ld1 = 512; a.ld2 = 0;
    hipError_t e = launch_conv_f32(a, s);
    if (e == hipSuccess) {
        ConvArgs h{};
        h.x = t->d_S; h.w = t->d_phead; h.bias = t->d_w + t->off_hb; h.residual = nullptr;
        h.out = t->d_reg; h.ld1 = 4 * K; h.act = ACT_LINEAR; h.split = 4 * K;
        h.out2 = t->d_cls; h.ld2 = K; h.act2 = ACT_SIGMOID;
        h.B = B; h.H = F; h.W = F; h.Cin = 512; h.OH = F; h.OW = F; h.Cout = nc;
        h.R = 1; h.S = 1; h.stride = 1; h.pad_t = 0; h.pad_l = 0; h.ps = t->ps_head;
        e = launch_conv_f32(h, s);
    }
    float *graw_reg = t->d_graw, *graw_cls = t->d_graw + P * 4 * K;
    const long long n = P * K;                  // (B, A) with A = F F K
    if (e == hipSuccess)
        e = launch_losses(d_bbox_deltas, t->d_reg, d_bbox_labels, t->d_cls, n, train ? graw_reg : nullptr, train ? graw_cls : nullptr,
                          d_losses, 1, t->d_lws, s);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
    t->last_B = B;
    t->d_tap = feat;
    if (train) {
        t->pending_B = B;
        t->pending_imgs = d_imgs;
    }
    return RPN_OK;
}

// the pending forward's B and d_imgs and the Adam parameters are checked by the caller
static int trainer_backward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_feature_grad, float lr,
                            float beta_1, float beta_2, float epsilon, void *stream)
{
    hipStream_t s = as_stream(stream);
    const int F = t->F, K = t->K, nc = t->nc;
    const long long P = (long long)B * F * F;
    const long long n = P * K;
    float *graw_reg = t->d_graw, *graw_cls = t->d_graw + P * 4 * K;
    t->pending_B = 0;                           // consumed, whatever happens below
    t->pending_imgs = nullptr;
    hipLaunchKernelGGL(head_dz_kernel, dim3(grid_for(P * nc)), dim3(256), 0, s, graw_reg, graw_cls, t->d_cls, losses_scale(t->d_lws, n), P, K,
                       t->d_dz);
    const int chunks = (int)((P + kChunkRows - 1) / kChunkRows);
    const int dgrid = (int)((P + 15) / 16);
    // head_{w,d}grad are instantiated for the anchor counts of the reference's configurations (5 K = 45: 3 ratios x 3 scales)
    // and the other small tables up to K = 12
    switch (nc) {
#define RPN_HEAD_NC(NCV)                                                                                                          \
    case NCV:                                                                                                                     \
        hipLaunchKernelGGL(head_wgrad_kernel<NCV>, dim3(chunks), dim3(256), 0, s, t->d_S, t->d_dz, P, t->d_part);                \
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_for(513 * NCV)), dim3(256), 0, s, t->d_part, chunks, 513LL * NCV,      \
                           t->d_g + t->off_hk);                                                                                   \
        hipLaunchKernelGGL(head_dgrad_kernel<NCV>, dim3(dgrid), dim3(512), 0, s, t->d_S, t->d_dz, t->d_w + t->off_hk, P, t->d_dS); \
        break;
        RPN_HEAD_NC(5) RPN_HEAD_NC(10) RPN_HEAD_NC(15) RPN_HEAD_NC(20) RPN_HEAD_NC(25) RPN_HEAD_NC(30) RPN_HEAD_NC(35)
        RPN_HEAD_NC(40) RPN_HEAD_NC(45) RPN_HEAD_NC(50) RPN_HEAD_NC(55) RPN_HEAD_NC(60)
#undef RPN_HEAD_NC
        default: return fail(RPN_ERR_UNSUPPORTED, "%s: %d anchors per position", what, K);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_wgrad(t->d_tap, t->d_dS, B, F, F, t->cin, 512, t->d_part, t->d_g + t->off_ck, s);
    if (e == hipSuccess) e = launch_colsum(t->d_dS, P, 512, t->d_part, t->d_g + t->off_cb, s);
    if (e == hipSuccess && t->bb_from >= 0) e = backbone_backward(t, B, d_feature_grad, s);
    if (e == hipSuccess && t->mn_from >= 0) e = mn_backward(t, d_imgs, B, d_feature_grad, s);
    if (e == hipSuccess) {
        ++t->t;
        hipLaunchKernelGGL(adam_kernel, dim3(grid_for((long long)t->n)), dim3(256), 0, s, t->d_w, t->d_g, t->d_m, t->d_v, (long long)t->n,
                           t->t, lr, beta_1, beta_2, epsilon);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_step(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                                     const float *d_bbox_labels, int update, float lr, float beta_1, float beta_2, float epsilon,
                                     float *d_losses, void *stream)
{
    const char *what = "rpn_head_trainer_step";
    int st = trainer_check_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, d_losses);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(update == 0 || update == 1, "rpn_head_trainer_step: update must be 0 or 1");
    if (update && (st = trainer_check_adam(what, lr, beta_1, beta_2, epsilon)) != RPN_OK) return st;
    if ((st = trainer_check_loaded(t, what)) != RPN_OK) return st;
    st = trainer_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, update, d_losses, stream);
    if (st != RPN_OK || !update) return st;
    return trainer_backward(t, what, d_imgs, B, nullptr, lr, beta_1, beta_2, epsilon, stream);
}

extern "C" int rpn_head_trainer_forward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                                        const float *d_bbox_labels, int train, float *d_losses, void *stream)
{
    const char *what = "rpn_head_trainer_forward";
    int st = trainer_check_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, d_losses);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(train == 0 || train == 1, "rpn_head_trainer_forward: train must be 0 or 1");
    if ((st = trainer_check_loaded(t, what)) != RPN_OK) return st;
    return trainer_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, train, d_losses, stream);
}

extern "C" int rpn_head_trainer_feature(rpn_head_trainer *t, float *d_out, int B, void *stream)
{
    RPN_REQUIRE(t && d_out, "rpn_head_trainer_feature: null argument");
    RPN_REQUIRE(B >= 1 && B == t->last_B && t->d_tap, "rpn_head_trainer_feature: batch %d, the last forward ran %d images", B, t->last_B);
    RPN_REQUIRE_DEVICE();
    RPN_HIP_CHECK(hipMemcpyAsync(d_out, t->d_tap, (size_t)B * t->F * t->F * t->cin * sizeof(float), hipMemcpyDeviceToDevice,
                                 as_stream(stream)));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_backward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_feature_grad, float lr,
                                         float beta_1, float beta_2, float epsilon, void *stream)
{
    const char *what = "rpn_head_trainer_backward";
    RPN_REQUIRE(t, "rpn_head_trainer_backward: null argument");
    RPN_REQUIRE(!d_feature_grad || t->bb_from >= 0 || t->mn_from >= 0,
                "rpn_head_trainer_backward: d_feature_grad given to a trainer with a frozen backbone: nothing below the feature tap trains "
                "(create the trainer with rpn_model_trainer_create and a train_from layer)");
    RPN_REQUIRE(d_imgs, "rpn_head_trainer_backward: null argument");
    const int st = trainer_check_adam(what, lr, beta_1, beta_2, epsilon);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(t->pending_B > 0, "rpn_head_trainer_backward: no pending rpn_head_trainer_forward with train = 1 on this trainer");
    RPN_REQUIRE(B == t->pending_B, "rpn_head_trainer_backward: batch %d, the pending forward ran %d images", B, t->pending_B);
    RPN_REQUIRE(d_imgs == t->pending_imgs, "rpn_head_trainer_backward: d_imgs is not the pending forward's image batch");
    RPN_REQUIRE(((uintptr_t)d_feature_grad & 3) == 0, "rpn_head_trainer_backward: d_feature_grad must be 4-byte aligned");
    return trainer_backward(t, what, d_imgs, B, d_feature_grad, lr, beta_1, beta_2, epsilon, stream);
}

extern "C" long long rpn_head_trainer_steps(const rpn_head_trainer *t) { return t ? t->t : -1; }

extern "C" int rpn_head_trainer_outputs(rpn_head_trainer *t, float *d_reg, float *d_cls, int B, void *stream)
{
    RPN_REQUIRE(t && d_reg && d_cls, "rpn_head_trainer_outputs: null argument");
    RPN_REQUIRE(B >= 1 && B == t->last_B, "rpn_head_trainer_outputs: batch %d, the last step ran %d images", B, t->last_B);
    RPN_REQUIRE_DEVICE();
    const size_t P = (size_t)B * t->F * t->F;
    RPN_HIP_CHECK(hipMemcpyAsync(d_reg, t->d_reg, P * 4 * t->K * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    RPN_HIP_CHECK(hipMemcpyAsync(d_cls, t->d_cls, P * t->K * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return RPN_OK;
}
