// det_head_kernels.hip -- the detection head: two fully-connected ReLU layers on the flattened RoI features and the cls | reg output
// pair (rpn_det_head_*, rpn_fc_forward; contract in include/rpn_hip.h).  New here: the forward GEMM (fc_forward_f32_kernel) and two
// small element-wise kernels; the split-float16 forward of the inference head (RPN_PRECISION_F16X3) has its kernels in
// det_head_x3_kernels.hip and its host side here.  The backward reuses the 1x1-conv backward GEMMs (train_mnv2.h), the column sums and Adam
// (train_head.h) unchanged; after each input-gradient GEMM one in-place pass applies the ReLU mask (launch_relu_mask).  A trainable
// head switched to split float16 (rpn_det_head_set_train_precision) runs the split forward and det_head_x3_kernels.hip's two backward
// GEMMs instead, keeps the packed image beside its float32 master weights and refreshes it on the device (head_repack).
// Dropout after the two hidden layers (dropout.h; rpn_det_head_set_dropout, rpn_dropout_forward) has kernels of its own, launched
// only by a kept forward at rate > 0 and by that forward's backward: fc_forward_f32_dropout_kernel, relu_scale_mask_kernel,
// dropout_forward_kernel here, the two split-float16 variants in det_head_x3_kernels.hip.
#include <cstdint>
#include <cstring>
#include <vector>

#include "conv_kernels.h"
#include "det_head.h"
#include "rpn_common.h"
#include "train_common.h"
#include "train_head.h"
#include "train_mnv2.h"

namespace rpn {

static constexpr int kGridCap = 4096;          // workgroups of this file's grid-stride kernels

// ---- forward GEMM on v_mfma_f32_32x32x2_f32 ------------------------------------------------------------------------------------------
// out (M x N) = act(A (M x K, K contiguous) W (K x N, N contiguous, leading dimension ldw) + bias).
// Workgroup: a 128 x 128 tile, four waves of 64 x 64 = 2 x 2 MFMA blocks of 32 x 32 (four independent accumulators per wave: the
// 64-cycle dependent latency of the instruction is covered inside one wave).  K slices of 32 are staged global -> registers -> LDS,
// double buffered with one barrier per slice, the next slice's loads in flight under this slice's 64 MFMAs per wave.
//   A: a thread loads float4s along K (rows tid / 8 + 32 i, K quad tid % 8) and stores them transposed, As[k][m ^ 4 (k / 4 % 8)]:
//      ds_write_b32 banks are (address / 4) % 32 per 32-lane half; a half holds 8 K quads x 4 consecutive rows, and the XOR sends
//      quad q of row 4 g + r to bank 4 (g ^ q) + r -- 32 different banks.  The XOR permutes columns inside an aligned group of 32,
//      so a fragment read (32 consecutive rows of one k per half-wave) stays conflict free, and k / 4 % 8 of the k = 2 kk + lane / 32
//      a lane reads at step kk is kk / 2 % 8: the same for the whole wave.
//   W: float4s along N (K rows tid / 32 + 8 i, column quad tid % 32), stored as they are: a half-wave writes one whole row.
// 2 x 32 x (128 + 128) floats = 64 KB of LDS: two workgroups per CU.
// Each accumulator element is one fmaf chain in k order over the whole of K (no split of K, no partial tiles added later); slices
// beyond K and rows / columns beyond the matrix enter as zeros.  Row m's result reads row m of A only.
// M, N and K tails are guarded; stores are scalar and guarded (N need not be a multiple of 4), columns < split to out0, the others
// to out1.
constexpr int kFcBM = 128, kFcBN = 128, kFcBK = 32;
// grid.y holds the row tiles of the forward (128 rows) and of launch_conv1x1_dgrad (64 rows), and the input-channel tiles of
// launch_conv1x1_wgrad (64 channels): what one launch can cover
constexpr long long kMaxGridY = 65535;
constexpr long long kFcMaxRows = kMaxGridY * kFcBM, kHeadMaxRows = kMaxGridY * 64, kHeadMaxWidth = kMaxGridY * 64;

// the main loop shared by fc_forward_f32_kernel and fc_forward_f32_dropout_kernel: acc <- the workgroup's tile of A W.  The thread's
// indices come from the kernel, which needs them again in its epilogue.
__device__ __forceinline__ void fc_forward_f32_mainloop(const float *__restrict__ A, const float *__restrict__ W, int M, int K, int ldw,
                                                        const int tid, const int wm, const int wn, const int l32, const int kh,
                                                        const int n0, const int m0, f32x16t (&acc)[2][2])
{
    __shared__ __attribute__((aligned(16))) float As[2][kFcBK][kFcBM];
    __shared__ __attribute__((aligned(16))) float Bs[2][kFcBK][kFcBN];
    const int nsteps = (K + kFcBK - 1) / kFcBK;
    const int ar = tid >> 3, akq = tid & 7, bk = tid >> 5, bq = tid & 31;
    float4 ra[4], rb[4];
    auto load_global = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            rb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int row = m0 + ar + 32 * i, ka = k0 + 4 * akq;
            if (row < M && ka < K) ra[i] = *reinterpret_cast<const float4 *>(A + (size_t)row * K + ka);
            const int kb = k0 + bk + 8 * i, col = n0 + 4 * bq;
            if (kb < K && col < ldw) rb[i] = *reinterpret_cast<const float4 *>(W + (size_t)kb * ldw + col);
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = (ar + 32 * i) ^ (4 * akq);
            As[buf][4 * akq + 0][m] = ra[i].x;
            As[buf][4 * akq + 1][m] = ra[i].y;
            As[buf][4 * akq + 2][m] = ra[i].z;
            As[buf][4 * akq + 3][m] = ra[i].w;
            *reinterpret_cast<float4 *>(&Bs[buf][bk + 8 * i][4 * bq]) = rb[i];
        }
    };
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    load_global(0);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global((step + 1) * kFcBK);
#pragma unroll
        for (int kk = 0; kk < kFcBK / 2; ++kk) {
            const int k = 2 * kk + kh, sw = 4 * ((kk >> 1) & 7);
            const float a0 = As[cur][k][(wm * 64 + l32) ^ sw], a1 = As[cur][k][(wm * 64 + 32 + l32) ^ sw];
            const float b0 = Bs[cur][k][wn * 64 + l32], b1 = Bs[cur][k][wn * 64 + 32 + l32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
}

__global__ void __launch_bounds__(256) fc_forward_f32_kernel(const float *__restrict__ A, const float *__restrict__ W,
                                                            const float *__restrict__ bias, int M, int K, int N, int ldw, int relu,
                                                            int split, float *__restrict__ out0, float *__restrict__ out1)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, kh = lane >> 5;
    const int n0 = blockIdx.x * kFcBN, m0 = blockIdx.y * kFcBM;
    f32x16t acc[2][2];
    fc_forward_f32_mainloop(A, W, M, K, ldw, tid, wm, wn, l32, kh, n0, m0, acc);
    // accumulator element e: row 8 (e / 4) + 4 kh + e % 4, column lane % 32
    const int n1 = N - split;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + 32 * j + l32;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.0f;
        float *dst = col < split ? out0 + col : out1 + (col - split);
        const int ld = col < split ? split : n1;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + 32 * i + 8 * (e >> 2) + 4 * kh + (e & 3);
                if (row < M) {
                    float v = bias ? acc[i][j][e] + bv : acc[i][j][e];
                    if (relu) v = fmaxf(v, 0.0f);
                    dst[(size_t)row * ld] = v;
                }
            }
    }
}

// The same product for a hidden layer that is dropped (dropout.h; contract in include/rpn_hip.h): out (M x N) =
// keep ? fl32(max(A W + bias, 0) * scale) : +0.  An accumulator's elements 4 g .. 4 g + 3 are four consecutive rows of one column
// starting at a multiple of 4, so one generator evaluation (counter (column, row / 4, layer, t)) serves four stores; it is made
// inside the store loop, one group at a time, so that its state lives beside the 64 accumulators without scratch.
__global__ void __launch_bounds__(256) fc_forward_f32_dropout_kernel(const float *__restrict__ A, const float *__restrict__ W,
                                                                    const float *__restrict__ bias, int M, int K, int N, int ldw,
                                                                    DropoutArgs drop, float *__restrict__ out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, kh = lane >> 5;
    const int n0 = blockIdx.x * kFcBN, m0 = blockIdx.y * kFcBM;
    f32x16t acc[2][2];
    fc_forward_f32_mainloop(A, W, M, K, ldw, tid, wm, wn, l32, kh, n0, m0, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + 32 * j + l32;
        if (col >= N) continue;
        const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row0 = m0 + wm * 64 + 32 * i + 8 * g + 4 * kh;
                if (row0 >= M) continue;
                const unsigned keep = dropout_keep4(drop, (unsigned)col, (unsigned)row0 >> 2);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (row0 + r < M) {
                        const float z = bias ? acc[i][j][4 * g + r] + bv : acc[i][j][4 * g + r];
                        out[(size_t)(row0 + r) * N + col] = keep >> r & 1u ? fmaxf(z, 0.0f) * drop.scale : 0.0f;
                    }
            }
    }
}

// out (M x N) = keep ? fl32(x * scale) : +0, out of place: the contract's mask and scale on any tensor.  One thread per four rows of
// one column (one generator evaluation), the column running fastest: a wave reads and writes 256 contiguous bytes of each row.
__global__ void __launch_bounds__(256) dropout_forward_kernel(const float *__restrict__ x, int M, int N, long long total, DropoutArgs drop,
                                                             float *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long mq = i / N;
        const int n = (int)(i - mq * N);
        const unsigned keep = dropout_keep4(drop, (unsigned)n, (unsigned)mq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = 4 * mq + r;
            if (row < M) out[row * N + n] = keep >> r & 1u ? x[row * N + n] * drop.scale : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(256) pack_pair_grad_kernel(const float *__restrict__ gl, const float *__restrict__ gd, long long total,
                                                            int C, int npad, float *__restrict__ dz)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / npad;
        const int j = (int)(i - m * npad);
        dz[i] = j < C ? gl[m * C + j] : j < 5 * C ? gd[m * 4 * C + (j - C)] : 0.0f;
    }
}

__global__ void __launch_bounds__(256) relu_mask_kernel(float4 *__restrict__ g, const float4 *__restrict__ h, long long n4)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 v = g[i];
        const float4 a = h[i];
        v.x = a.x > 0.0f ? v.x : 0.0f;
        v.y = a.y > 0.0f ? v.y : 0.0f;
        v.z = a.z > 0.0f ? v.z : 0.0f;
        v.w = a.w > 0.0f ? v.w : 0.0f;
        g[i] = v;
    }
}

// the mask of a DROPPED layer: g <- a > 0 ? fl32(g * scale) : 0.  The stored activation a is zero where the element was dropped and
// positive where it was kept and z > 0 (scale >= 1 cannot take a positive value to zero), so no generator runs in the backward.
__global__ void __launch_bounds__(256) relu_scale_mask_kernel(float4 *__restrict__ g, const float4 *__restrict__ h, long long n4,
                                                             float scale)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 v = g[i];
        const float4 a = h[i];
        v.x = a.x > 0.0f ? v.x * scale : 0.0f;
        v.y = a.y > 0.0f ? v.y * scale : 0.0f;
        v.z = a.z > 0.0f ? v.z * scale : 0.0f;
        v.w = a.w > 0.0f ? v.w * scale : 0.0f;
        g[i] = v;
    }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

hipError_t launch_fc_forward(const float *a, const float *w, const float *bias, int M, int K, int N, int ldw, int relu, int split,
                             float *out0, float *out1, hipStream_t s)
{
    hipLaunchKernelGGL(fc_forward_f32_kernel, dim3((N + kFcBN - 1) / kFcBN, (M + kFcBM - 1) / kFcBM), dim3(256), 0, s, a, w, bias, M, K, N,
                       ldw, relu, split, out0, out1);
    return hipGetLastError();
}

hipError_t launch_pack_pair_grad(const float *grad_logits, const float *grad_deltas, int M, int C, int npad, float *dz, hipStream_t s)
{
    const long long total = (long long)M * npad;
    hipLaunchKernelGGL(pack_pair_grad_kernel, dim3(grid_1d(total, kGridCap)), dim3(256), 0, s, grad_logits, grad_deltas, total, C, npad, dz);
    return hipGetLastError();
}

hipError_t launch_relu_mask(float *g, const float *h, long long n, hipStream_t s)
{
    hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_1d(n / 4, kGridCap)), dim3(256), 0, s, reinterpret_cast<float4 *>(g),
                       reinterpret_cast<const float4 *>(h), n / 4);
    return hipGetLastError();
}

hipError_t launch_fc_forward_dropout(const float *a, const float *w, const float *bias, int M, int K, int N, int ldw,
                                     const DropoutArgs &drop, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(fc_forward_f32_dropout_kernel, dim3((N + kFcBN - 1) / kFcBN, (M + kFcBM - 1) / kFcBM), dim3(256), 0, s, a, w, bias,
                       M, K, N, ldw, drop, out);
    return hipGetLastError();
}

hipError_t launch_relu_scale_mask(float *g, const float *h, long long n, float scale, hipStream_t s)
{
    hipLaunchKernelGGL(relu_scale_mask_kernel, dim3(grid_1d(n / 4, kGridCap)), dim3(256), 0, s, reinterpret_cast<float4 *>(g),
                       reinterpret_cast<const float4 *>(h), n / 4, scale);
    return hipGetLastError();
}

hipError_t launch_dropout_forward(const float *x, int M, int N, const DropoutArgs &drop, float *out, hipStream_t s)
{
    const long long total = (long long)((M + 3) / 4) * N;
    hipLaunchKernelGGL(dropout_forward_kernel, dim3(grid_1d(total, kGridCap)), dim3(256), 0, s, x, M, N, total, drop, out);
    return hipGetLastError();
}

}  // namespace rpn

// ---- the head object -------------------------------------------------------------------------------------------------------------------
// One flat parameter buffer w of n floats: W1 (K1, H1) | b1 (H1) | W2 (H1, H2) | b2 (H2) | Wp (H2, npad) | bp (npad), where Wp / bp
// hold the cls | reg pair side by side, columns [0, C) cls, [C, 5 C) reg, [5 C, npad) zeros, npad = 5 C rounded up to 4.  A trainable
// head has g, m and v of the same layout (the padding's gradient is zero, so Adam leaves it zero).  Device memory is allocated at the
// first call that needs it; create itself touches no device.
struct rpn_det_head {
    int ph, pw, cf, h1, h2, c, max_rows, trainable;
    int k1, npad;
    size_t off[6], n;            // W1, b1, W2, b2, Wp, bp; the total
    size_t part_floats;          // reduction scratch of the backward (weight-gradient slabs or column-sum chunks, whichever is larger)
    float *w = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
    float *a1 = nullptr, *a2 = nullptr;                       // the two hidden activations (max_rows, H1) / (max_rows, H2)
    float *dz = nullptr, *d1 = nullptr, *d2 = nullptr, *part = nullptr;
    unsigned loaded = 0;         // bit per layer: fc1, fc2, cls, reg
    int kept_rows = 0;           // rows of the forward whose activations the backward may read; 0: none
    const float *kept_pooled = nullptr;   // ... and that forward's input: the backward must be handed the same tensor
    long long t = 0;
    // RPN_PRECISION_F16X3 (inference heads only): beside w, the packed split image of the three weight matrices.  It mirrors w's layout
    // -- W1 | (b1) | W2 | (b2) | Wp | (bp), every matrix with its rows rounded up to 32 and the bias slots unused -- so that it is as
    // large as w when every K is a multiple of 32.  shift[i]: layer i's power-of-two pre-scale; status: the float16 range flag.
    int precision = RPN_PRECISION_F32;
    unsigned char *wx = nullptr;
    unsigned *status = nullptr;
    size_t xoff[3] = {0, 0, 0}, xbytes = 0;   // byte offsets of W1, W2, Wp in wx; its size
    int shift[4] = {0, 0, 0, 0};
    // A trainable head whose products run in split float16 (rpn_det_head_set_train_precision): the same image beside the float32 master
    // weights, refreshed ON THE DEVICE (head_repack) after every change of w, and every scale in device memory.  xmeta, 64 words:
    // [0, 7) the bits of max|.| of fc1, fc2, cls, reg, dz, d2, d1; from word 8 the pairs {2^s, 2^-s} of fc1, fc2, cls, reg, cls | reg as
    // one matrix, dz, d2, d1.  x_stale: w has changed since the image was written.
    int train_precision = RPN_PRECISION_F32;
    unsigned *xmeta = nullptr;
    bool x_stale = false;
    // Dropout after the two hidden layers (rpn_det_head_set_dropout; trainable heads): host state only.  drop_calls is the call
    // number t of the NEXT dropped forward; kept_dropped: the kept forward applied dropout (at drop_rate: set_dropout drops it).
    double drop_rate = 0.0;
    unsigned long long drop_seed = 0, drop_calls = 0;
    bool kept_dropped = false;
    // The update rule (rpn_det_head_set_optimizer; default: Adam alone = launch_adam)
    rpn::OptimConfig opt;
    rpn::OptimDevice optdev;
};

namespace {
using namespace rpn;

const char *const kLayerNames[4] = {"fc1", "fc2", "cls", "reg"};

int layer_index(const char *name)
{
    for (int i = 0; name && i < 4; ++i)
        if (!strcmp(name, kLayerNames[i])) return i;
    return -1;
}

// where layer i's kernel and bias live inside a buffer of the parameter layout: rows x cols floats at leading dimension ld
struct LayerView {
    size_t kernel, bias;
    int rows, cols, ld;
};

LayerView layer_view(const rpn_det_head *h, int i)
{
    switch (i) {
    case 0: return {h->off[0], h->off[1], h->k1, h->h1, h->h1};
    case 1: return {h->off[2], h->off[3], h->h1, h->h2, h->h2};
    case 2: return {h->off[4], h->off[5], h->h2, h->c, h->npad};
    default: return {h->off[4] + (size_t)h->c, h->off[5] + (size_t)h->c, h->h2, 4 * h->c, h->npad};
    }
}

size_t head_workspace_bytes(const rpn_det_head *h)
{
    const size_t R = (size_t)h->max_rows;
    size_t b = a256(R * h->h1 * sizeof(float)) + a256(R * h->h2 * sizeof(float));
    if (h->trainable)
        b += a256(R * h->npad * sizeof(float)) + a256(R * h->h1 * sizeof(float)) + a256(R * h->h2 * sizeof(float)) +
             a256(h->part_floats * sizeof(float));
    return b;
}

void head_free(rpn_det_head *h)
{
    for (float **p : {&h->w, &h->g, &h->m, &h->v, &h->a1, &h->a2, &h->dz, &h->d1, &h->d2, &h->part}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (h->wx) (void)hipFree(h->wx);
    if (h->status) (void)hipFree(h->status);
    if (h->xmeta) (void)hipFree(h->xmeta);
    h->wx = nullptr, h->status = nullptr, h->xmeta = nullptr;
    optim_free(&h->optdev);
    h->loaded = 0;               // the weights went with the buffers
    h->kept_rows = 0;
}

// the head's device memory, once; zeros everywhere (the padding columns of the pair stay zero for ever)
int head_ensure_image(rpn_det_head *h);

int head_ensure_device(rpn_det_head *h)
{
    if (h->w) return head_ensure_image(h);
    RPN_REQUIRE_DEVICE();
    const size_t R = (size_t)h->max_rows;
    struct { float **p; size_t n; bool zero; } bufs[] = {
        {&h->w, h->n, true}, {&h->a1, R * h->h1, false}, {&h->a2, R * h->h2, false},
        {&h->g, h->trainable ? h->n : 0, true}, {&h->m, h->trainable ? h->n : 0, true}, {&h->v, h->trainable ? h->n : 0, true},
        {&h->dz, h->trainable ? R * h->npad : 0, false}, {&h->d1, h->trainable ? R * h->h1 : 0, false},
        {&h->d2, h->trainable ? R * h->h2 : 0, false}, {&h->part, h->trainable ? h->part_floats : 0, false}};
    for (auto &b : bufs) {
        if (!b.n) continue;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(b.p), b.n * sizeof(float));
        if (e == hipSuccess && b.zero) e = hipMemset(*b.p, 0, b.n * sizeof(float));
        if (e != hipSuccess) {
            head_free(h);
            return fail(RPN_ERR_NO_DEVICE, "rpn_det_head: device allocation of %zu bytes failed: %s", b.n * sizeof(float),
                        hipGetErrorString(e));
        }
    }
    return head_ensure_image(h);
}

// the packed image, the status word and (trainable heads) the scale block, once a precision asks for them; a trainable head's image
// starts stale: whatever w holds by then is packed by the next call that reads the image
int head_ensure_image(rpn_det_head *h)
{
    if (!h->xbytes || h->wx) return RPN_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->wx), h->xbytes);
    if (e == hipSuccess) e = hipMemset(h->wx, 0, h->xbytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->status), sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(h->status, 0, sizeof(unsigned));
    if (e == hipSuccess && h->trainable) e = hipMalloc(reinterpret_cast<void **>(&h->xmeta), 64 * sizeof(unsigned));
    if (e == hipSuccess && h->trainable) e = hipMemset(h->xmeta, 0, 64 * sizeof(unsigned));
    if (e != hipSuccess) {
        head_free(h);
        return fail(RPN_ERR_NO_DEVICE, "rpn_det_head: device allocation of %zu bytes failed: %s", h->xbytes, hipGetErrorString(e));
    }
    h->x_stale = h->trainable != 0;
    return RPN_OK;
}

// byte offsets and size of the packed image (host state only)
void head_size_image(rpn_det_head *h)
{
    const size_t xs[6] = {fc_x3_packed_bytes(h->k1, h->h1), (size_t)h->h1 * sizeof(float), fc_x3_packed_bytes(h->h1, h->h2),
                          (size_t)h->h2 * sizeof(float), fc_x3_packed_bytes(h->h2, h->npad), (size_t)h->npad * sizeof(float)};
    h->xbytes = 0;
    for (int i = 0; i < 6; ++i) {
        if (i % 2 == 0) h->xoff[i / 2] = h->xbytes;
        h->xbytes += xs[i];
    }
}

float *head_scales(const rpn_det_head *h, int pair) { return reinterpret_cast<float *>(h->xmeta + 8) + 2 * pair; }

// kernel / bias of layer `name` between HOST arrays and the buffer `base` (the weights or their gradient)
int head_copy_layer(rpn_det_head *h, float *base, const char *name, float *kernel, float *bias, bool to_device, hipStream_t s)
{
    const LayerView lv = layer_view(h, layer_index(name));
    const size_t wbytes = (size_t)lv.cols * sizeof(float);
    if (to_device) {
        RPN_HIP_CHECK(hipMemcpy2D(base + lv.kernel, (size_t)lv.ld * sizeof(float), kernel, wbytes, wbytes, lv.rows, hipMemcpyHostToDevice));
        RPN_HIP_CHECK(hipMemcpy(base + lv.bias, bias, wbytes, hipMemcpyHostToDevice));
    } else {
        RPN_HIP_CHECK(hipMemcpy2DAsync(kernel, wbytes, base + lv.kernel, (size_t)lv.ld * sizeof(float), wbytes, lv.rows,
                                       hipMemcpyDeviceToHost, s));
        RPN_HIP_CHECK(hipMemcpyAsync(bias, base + lv.bias, wbytes, hipMemcpyDeviceToHost, s));
        RPN_HIP_CHECK(hipStreamSynchronize(s));
    }
    return RPN_OK;
}

// F16X3: layer i's pre-scale from the host kernel, then its columns of the packed image from the float32 copy on the device
int head_pack_layer(rpn_det_head *h, int i, const float *kernel)
{
    const LayerView lv = layer_view(h, i);
    const int mat = i < 2 ? i : 2;                               // cls and reg share the pair's matrix: columns [0, C) and [C, 5 C)
    h->shift[i] = split_weight_shift(kernel, (size_t)lv.rows * lv.cols, true);
    RPN_HIP_CHECK(launch_fc_pack_x3(h->w + h->off[2 * mat], lv.rows, lv.ld, i == 3 ? h->c : 0, lv.cols, h->shift[i], h->wx + h->xoff[mat],
                                    nullptr));
    RPN_HIP_CHECK(hipStreamSynchronize(nullptr));
    return RPN_OK;
}

// A training head's image and scales from its master weights, all on the device and without a synchronisation: max|w| per layer,
// the shifts by the inference head's rule (plus the pair's joint one, for the input gradient), then fc_pack_x3_kernel per layer.
hipError_t head_repack(rpn_det_head *h, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(h->xmeta, 0, 4 * sizeof(unsigned), s);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        const LayerView lv = layer_view(h, i);
        e = launch_fc_absmax(h->w + lv.kernel, lv.rows, lv.cols, lv.ld, h->xmeta + i, s);
    }
    if (e == hipSuccess) e = launch_fc_scales_x3(h->xmeta, 4, 2, 3, false, head_scales(h, 0), s);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        const LayerView lv = layer_view(h, i);
        const int mat = i < 2 ? i : 2;
        e = launch_fc_pack_x3(h->w + h->off[2 * mat], lv.rows, lv.ld, i == 3 ? h->c : 0, lv.cols, 0, h->wx + h->xoff[mat], s, head_scales(h, i));
    }
    if (e == hipSuccess) h->x_stale = false;
    return e;
}

bool head_trains_x3(const rpn_det_head *h) { return h->train_precision == RPN_PRECISION_F16X3; }

// The decayed elements of the parameter layout, as sorted disjoint [begin, end) pairs: W1, W2 and the real columns [0, 5 C) of every
// row of Wp -- one range per row when the pair is padded (npad > 5 C), so that no bias and no padding column is ever decayed.
std::vector<long long> head_decay_ranges(const rpn_det_head *h)
{
    std::vector<long long> out;
    auto add = [&](size_t b, size_t e) { out.push_back((long long)b), out.push_back((long long)e); };
    add(h->off[0], h->off[0] + (size_t)h->k1 * h->h1);
    add(h->off[2], h->off[2] + (size_t)h->h1 * h->h2);
    if (h->npad == 5 * h->c) {
        add(h->off[4], h->off[4] + (size_t)h->h2 * h->npad);
    } else {
        for (int r = 0; r < h->h2; ++r) add(h->off[4] + (size_t)r * h->npad, h->off[4] + (size_t)r * h->npad + 5 * (size_t)h->c);
    }
    return out;
}

// before a training head's image is read
hipError_t head_fresh_image(rpn_det_head *h, hipStream_t s) { return head_trains_x3(h) && h->x_stale ? head_repack(h, s) : hipSuccess; }

// one product of the head at its precision: layer 0 (fc1), 1 (fc2) or 2 (the cls | reg pair; out0 / out1); `dropped`: a hidden
// layer of a kept forward at rate > 0 -- the dropout variants, launched in no other case
hipError_t head_launch_layer(rpn_det_head *h, int mat, const float *in, int M, float *out0, float *out1, hipStream_t s,
                             bool dropped = false)
{
    const int K = mat == 0 ? h->k1 : mat == 1 ? h->h1 : h->h2, N = mat == 0 ? h->h1 : mat == 1 ? h->h2 : 5 * h->c;
    const int ld = mat == 2 ? h->npad : N, relu = mat == 2 ? 0 : 1, split = mat == 2 ? h->c : N;
    const float *w = h->w + h->off[2 * mat], *b = h->w + h->off[2 * mat + 1];
    if (dropped) {
        const DropoutArgs drop = make_dropout_args(h->drop_rate, h->drop_seed, h->drop_calls, mat);
        if (head_trains_x3(h))
            return launch_fc_forward_x3_dropout(in, h->wx + h->xoff[mat], b, M, K, N, ld, head_scales(h, mat) + 1, drop, out0, h->status, s);
        return launch_fc_forward_dropout(in, w, b, M, K, N, ld, drop, out0, s);
    }
    if (head_trains_x3(h))
        return launch_fc_forward_x3(in, h->wx + h->xoff[mat], b, M, K, N, ld, relu, split, 1.0f, 1.0f, out0, out1, h->status, s,
                                    head_scales(h, mat) + 1, head_scales(h, mat == 2 ? 3 : mat) + 1);
    if (h->precision != RPN_PRECISION_F16X3) return launch_fc_forward(in, w, b, M, K, N, ld, relu, split, out0, out1, s);
    return launch_fc_forward_x3(in, h->wx + h->xoff[mat], b, M, K, N, ld, relu, split, ldexpf(1.0f, -h->shift[mat]),
                                ldexpf(1.0f, -h->shift[mat == 2 ? 3 : mat]), out0, out1, h->status, s);
}

}  // namespace

extern "C" int rpn_det_head_create(int ph, int pw, int Cf, int H1, int H2, int C, int max_rows, int trainable, rpn_det_head **out)
{
    return rpn_det_head_create_ex(ph, pw, Cf, H1, H2, C, max_rows, trainable, RPN_PRECISION_F32, out);
}

extern "C" int rpn_det_head_create_ex(int ph, int pw, int Cf, int H1, int H2, int C, int max_rows, int trainable, int precision,
                                      rpn_det_head **out)
{
    const char *who = "rpn_det_head_create_ex";
    RPN_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    RPN_REQUIRE(ph >= 1 && pw >= 1, "%s: pooling size %d x %d", who, ph, pw);
    RPN_REQUIRE(Cf >= 4 && Cf % 4 == 0, "%s: Cf = %d must be a positive multiple of 4", who, Cf);
    RPN_REQUIRE(H1 >= 4 && H1 % 4 == 0 && H2 >= 4 && H2 % 4 == 0, "%s: H1 = %d and H2 = %d must be positive multiples of 4", who, H1, H2);
    RPN_REQUIRE(C >= 2 && C <= (1 << 20), "%s: C = %d labels (background included) must be >= 2", who, C);
    RPN_REQUIRE(max_rows >= 1, "%s: max_rows = %d", who, max_rows);
    RPN_REQUIRE(trainable == 0 || trainable == 1, "%s: trainable must be 0 or 1", who);
    const long long k1 = (long long)ph * pw * Cf;
    const int npad = (5 * C + 3) / 4 * 4;
    RPN_REQUIRE(k1 <= kHeadMaxWidth && H1 <= kHeadMaxWidth && H2 <= kHeadMaxWidth,
                "%s: %d x %d x %d = %lld features, H1 = %d, H2 = %d: a layer's input may be at most %lld wide (one weight-gradient launch)", who,
                ph, pw, Cf, k1, H1, H2, kHeadMaxWidth);
    RPN_REQUIRE(max_rows <= kHeadMaxRows, "%s: max_rows = %d, at most %lld rows fit one input-gradient launch", who, max_rows, kHeadMaxRows);
    RPN_REQUIRE(precision == RPN_PRECISION_F32 || precision == RPN_PRECISION_BF16X3 || precision == RPN_PRECISION_F16X3 ||
                    precision == RPN_PRECISION_F32W, "%s: precision = %d is no rpn_precision value", who, precision);
    if (precision == RPN_PRECISION_BF16X3 || precision == RPN_PRECISION_F32W)
        return fail(RPN_ERR_UNSUPPORTED, "%s: the head computes in RPN_PRECISION_F32 or RPN_PRECISION_F16X3, not in precision %d", who, precision);
    if (precision == RPN_PRECISION_F16X3 && trainable)
        return fail(RPN_ERR_UNSUPPORTED, "%s: RPN_PRECISION_F16X3 is the inference head's (trainable = 0): training stays exact float32", who);
    rpn_det_head *h = new rpn_det_head();
    h->precision = precision;
    h->ph = ph, h->pw = pw, h->cf = Cf, h->h1 = H1, h->h2 = H2, h->c = C, h->max_rows = max_rows, h->trainable = trainable;
    h->k1 = (int)k1, h->npad = npad;
    const size_t sizes[6] = {(size_t)k1 * H1, (size_t)H1, (size_t)H1 * H2, (size_t)H2, (size_t)H2 * npad, (size_t)npad};
    h->n = 0;
    for (int i = 0; i < 6; ++i) {
        h->off[i] = h->n;
        h->n += sizes[i];
    }
    if (precision == RPN_PRECISION_F16X3) head_size_image(h);
    const long long R = max_rows;
    h->part_floats = std::max({conv1x1_wgrad_ws_floats(R, h->k1, H1), conv1x1_wgrad_ws_floats(R, H1, H2), conv1x1_wgrad_ws_floats(R, H2, npad),
                               colsum_ws_floats(R, H1), colsum_ws_floats(R, H2), colsum_ws_floats(R, npad)});
    *out = h;
    return RPN_OK;
}

extern "C" void rpn_det_head_destroy(rpn_det_head *h)
{
    if (!h) return;
    head_free(h);
    delete h;
}

extern "C" int rpn_det_head_memory_bytes(const rpn_det_head *h, size_t *weights, size_t *workspace)
{
    RPN_REQUIRE(h && weights && workspace, "rpn_det_head_memory_bytes: null pointer");
    *weights = h->n * sizeof(float) * (h->trainable ? 4 : 1) + h->xbytes;
    *workspace = head_workspace_bytes(h);
    return RPN_OK;
}

extern "C" int rpn_det_head_set_layer(rpn_det_head *h, const char *name, const float *kernel, const float *bias)
{
    const char *who = "rpn_det_head_set_layer";
    RPN_REQUIRE(h && name && kernel && bias, "%s: null pointer", who);
    const int i = layer_index(name);
    RPN_REQUIRE(i >= 0, "%s: unknown layer '%s' (fc1, fc2, cls, reg)", who, name);
    int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    h->kept_rows = 0;            // a kept forward was made with the weights this call replaces
    st = head_copy_layer(h, h->w, name, const_cast<float *>(kernel), const_cast<float *>(bias), true, nullptr);
    if (st == RPN_OK && h->precision == RPN_PRECISION_F16X3) st = head_pack_layer(h, i, kernel);
    h->x_stale = true;           // (a training head's image follows at the next call that reads it)
    if (st == RPN_OK) h->loaded |= 1u << i;
    return st;
}

extern "C" int rpn_det_head_get_layer(rpn_det_head *h, const char *name, float *kernel, float *bias, void *stream)
{
    const char *who = "rpn_det_head_get_layer";
    RPN_REQUIRE(h && name && kernel && bias, "%s: null pointer", who);
    const int i = layer_index(name);
    RPN_REQUIRE(i >= 0, "%s: unknown layer '%s' (fc1, fc2, cls, reg)", who, name);
    RPN_REQUIRE(h->loaded >> i & 1u, "%s: layer '%s' was never set", who, name);
    return head_copy_layer(h, h->w, name, kernel, bias, false, as_stream(stream));
}

extern "C" int rpn_det_head_get_gradient(rpn_det_head *h, const char *name, float *kernel, float *bias, void *stream)
{
    const char *who = "rpn_det_head_get_gradient";
    RPN_REQUIRE(h && name && kernel && bias, "%s: null pointer", who);
    const int i = layer_index(name);
    RPN_REQUIRE(i >= 0, "%s: unknown layer '%s' (fc1, fc2, cls, reg)", who, name);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    return head_copy_layer(h, h->g, name, kernel, bias, false, as_stream(stream));
}

extern "C" long long rpn_det_head_steps(const rpn_det_head *h) { return h ? h->t : 0; }

extern "C" int rpn_det_head_set_train_precision(rpn_det_head *h, int precision)
{
    const char *who = "rpn_det_head_set_train_precision";
    RPN_REQUIRE(h, "%s: null head", who);
    RPN_REQUIRE(precision == RPN_PRECISION_F32 || precision == RPN_PRECISION_BF16X3 || precision == RPN_PRECISION_F16X3 ||
                    precision == RPN_PRECISION_F32W, "%s: precision = %d is no rpn_precision value", who, precision);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    if (precision == RPN_PRECISION_BF16X3 || precision == RPN_PRECISION_F32W)
        return fail(RPN_ERR_UNSUPPORTED, "%s: a head trains in RPN_PRECISION_F32 or RPN_PRECISION_F16X3, not in precision %d", who, precision);
    h->kept_rows = 0;            // a kept forward was made at the other precision
    h->train_precision = precision;
    if (precision == RPN_PRECISION_F16X3 && !h->xbytes) head_size_image(h);   // (allocated by the next call that needs the device)
    return RPN_OK;
}

extern "C" int rpn_det_head_train_precision(const rpn_det_head *h) { return h ? h->train_precision : RPN_PRECISION_F32; }

extern "C" int rpn_det_head_set_dropout(rpn_det_head *h, double rate, unsigned long long seed)
{
    const char *who = "rpn_det_head_set_dropout";
    RPN_REQUIRE(h, "%s: null head", who);
    RPN_REQUIRE(rate >= 0.0 && rate < 1.0, "%s: rate = %g must be finite and in [0, 1)", who, rate);      // (a NaN fails both compares)
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0 (dropout applies to kept forwards only)", who);
    h->kept_rows = 0;            // a kept forward was made at the other rate or seed
    h->drop_rate = rate, h->drop_seed = seed;
    return RPN_OK;
}

extern "C" int rpn_det_head_dropout_state(const rpn_det_head *h, double *rate, unsigned long long *seed, unsigned long long *calls)
{
    RPN_REQUIRE(h && rate && seed && calls, "rpn_det_head_dropout_state: null pointer");
    *rate = h->drop_rate, *seed = h->drop_seed, *calls = h->drop_calls;
    return RPN_OK;
}

extern "C" int rpn_det_head_set_dropout_calls(rpn_det_head *h, unsigned long long calls)
{
    const char *who = "rpn_det_head_set_dropout_calls";
    RPN_REQUIRE(h, "%s: null head", who);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    h->drop_calls = calls;       // (a kept forward stays: its backward reads the stored activations, not t)
    return RPN_OK;
}

extern "C" int rpn_det_head_get_activation(rpn_det_head *h, const char *name, float *d_out, int M, void *stream)
{
    const char *who = "rpn_det_head_get_activation";
    RPN_REQUIRE(h && name && d_out, "%s: null pointer", who);
    const int i = layer_index(name);
    RPN_REQUIRE(i == 0 || i == 1, "%s: layer '%s' is not a hidden layer (fc1, fc2)", who, name);
    RPN_REQUIRE(M >= 1 && h->kept_rows == M, "%s: no kept forward of %d rows (the kept forward, if any, had %d rows)", who, M, h->kept_rows);
    const size_t bytes = (size_t)M * (i == 0 ? h->h1 : h->h2) * sizeof(float);
    RPN_HIP_CHECK(hipMemcpyAsync(d_out, i == 0 ? h->a1 : h->a2, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return RPN_OK;
}

extern "C" int rpn_dropout_forward(const float *d_x, int M, int N, double rate, unsigned long long seed, unsigned calls, int layer,
                                   float *d_out, void *stream)
{
    const char *who = "rpn_dropout_forward";
    RPN_REQUIRE(d_x && d_out, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && N >= 1, "%s: M = %d, N = %d", who, M, N);
    RPN_REQUIRE(rate >= 0.0 && rate < 1.0, "%s: rate = %g must be finite and in [0, 1)", who, rate);
    RPN_REQUIRE(layer >= 0, "%s: layer = %d", who, layer);
    RPN_REQUIRE(d_x != d_out, "%s: the kernel is out of place", who);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_dropout_forward(d_x, M, N, make_dropout_args(rate, seed, calls, layer), d_out, as_stream(stream));
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_det_head_forward(rpn_det_head *h, const float *d_pooled, int M, int keep, float *d_logits, float *d_deltas,
                                    void *stream)
{
    const char *who = "rpn_det_head_forward";
    RPN_REQUIRE(h && d_pooled && d_logits && d_deltas, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && M <= h->max_rows, "%s: M = %d rows, the head was created for 1 .. %d", who, M, h->max_rows);
    RPN_REQUIRE(keep == 0 || (keep == 1 && h->trainable), "%s: keep = %d on a head created with trainable = %d", who, keep, h->trainable);
    RPN_REQUIRE(aligned16(d_pooled), "%s: the pooled features must be 16-byte aligned", who);
    RPN_REQUIRE(h->loaded == 15u, "%s: set_layer has not been called for every layer (fc1, fc2, cls, reg)", who);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    const hipStream_t s = as_stream(stream);
    h->kept_rows = 0;                    // the activations of an earlier forward are overwritten from here on
    const bool dropped = keep && h->drop_rate > 0.0;     // dropout is the identity in every forward that is not kept
    hipError_t e = head_fresh_image(h, s);
    if (e == hipSuccess) e = head_launch_layer(h, 0, d_pooled, M, h->a1, nullptr, s, dropped);
    if (e == hipSuccess) e = head_launch_layer(h, 1, h->a1, M, h->a2, nullptr, s, dropped);
    if (e == hipSuccess) e = head_launch_layer(h, 2, h->a2, M, d_logits, d_deltas, s);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    if (keep) h->kept_rows = M, h->kept_pooled = d_pooled, h->kept_dropped = dropped;
    if (dropped) h->drop_calls += 1;                     // both hidden layers of this forward used the same t
    return RPN_OK;
}

extern "C" int rpn_det_head_forward_layer(rpn_det_head *h, const char *name, const float *d_in, int M, float *d_out, void *stream)
{
    const char *who = "rpn_det_head_forward_layer";
    RPN_REQUIRE(h && name && d_in && d_out, "%s: null pointer", who);
    const int i = layer_index(name);
    RPN_REQUIRE(i == 0 || i == 1, "%s: layer '%s' is not a hidden layer (fc1, fc2)", who, name);
    RPN_REQUIRE(M >= 1 && M <= kFcMaxRows, "%s: M = %d (1 .. %lld)", who, M, kFcMaxRows);
    RPN_REQUIRE(aligned16(d_in), "%s: the input must be 16-byte aligned", who);
    RPN_REQUIRE(h->loaded >> i & 1u, "%s: layer '%s' was never set", who, name);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    hipError_t e = head_fresh_image(h, as_stream(stream));
    if (e == hipSuccess) e = head_launch_layer(h, i, d_in, M, d_out, nullptr, as_stream(stream));
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_det_head_status(rpn_det_head *h, unsigned *flags, int reset, void *stream)
{
    RPN_REQUIRE(h && flags, "rpn_det_head_status: null pointer");
    *flags = 0;
    if (!h->status) return RPN_OK;           // a float32 head, or an F16X3 head that has not touched the device yet
    const hipStream_t s = as_stream(stream);
    RPN_HIP_CHECK(hipMemcpyAsync(flags, h->status, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (reset) RPN_HIP_CHECK(hipMemsetAsync(h->status, 0, sizeof(unsigned), s));
    RPN_HIP_CHECK(hipStreamSynchronize(s));
    return RPN_OK;
}

extern "C" int rpn_det_head_backward(rpn_det_head *h, const float *d_pooled, int M, const float *d_grad_logits,
                                     const float *d_grad_deltas, float *d_grad_pooled, void *stream)
{
    const char *who = "rpn_det_head_backward";
    RPN_REQUIRE(h && d_pooled && d_grad_logits && d_grad_deltas, "%s: null pointer", who);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    RPN_REQUIRE(M >= 1 && M <= h->max_rows, "%s: M = %d rows, the head was created for 1 .. %d", who, M, h->max_rows);
    RPN_REQUIRE(h->kept_rows == M && h->kept_pooled == d_pooled,
                "%s: no kept forward of these %d rows (the kept forward, if any, had %d rows; any later forward, set_layer or adam_step "
                "replaces or drops it)", who, M, h->kept_rows);
    RPN_REQUIRE(aligned16(d_pooled) && aligned16(d_grad_pooled), "%s: the pooled features and their gradient must be 16-byte aligned", who);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    const hipStream_t s = as_stream(stream);
    const int K1 = h->k1, H1 = h->h1, H2 = h->h2, NP = h->npad;
    float *w = h->w, *g = h->g;
    // a dropped kept forward: each hidden layer's mask also carries the factor 1 / (1 - rate); the stored activations are zero
    // where an element was dropped, so the mask needs no generator
    const bool dropped = h->kept_dropped;
    const float dscale = make_dropout_args(h->drop_rate, 0, 0, 0).scale;
    if (head_trains_x3(h)) {
        // the same chain in split float16: each gradient tensor's max|.| (over its M rows and real columns) gives its shift, on the
        // device; the ReLU mask sits in the input-gradient product's epilogue; the bias sums stay float32
        const int NC = 5 * h->c;
        const float *sdz = head_scales(h, 5), *sd2 = head_scales(h, 6), *sd1 = head_scales(h, 7);
        auto shift_of = [&](const float *t, int cols, int ld, int slot) {
            hipError_t r = launch_fc_absmax(t, M, cols, ld, h->xmeta + 4 + slot, s);
            if (r == hipSuccess) r = launch_fc_scales_x3(h->xmeta + 4 + slot, 1, -1, -1, true, head_scales(h, 5 + slot), s);
            return r;
        };
        hipError_t e = hipMemsetAsync(h->xmeta + 4, 0, 3 * sizeof(unsigned), s);
        if (e == hipSuccess) e = launch_pack_pair_grad(d_grad_logits, d_grad_deltas, M, h->c, NP, h->dz, s);
        if (e == hipSuccess) e = shift_of(h->dz, NC, NP, 0);
        if (e == hipSuccess) e = launch_fc_wgrad_x3(h->a2, h->dz, M, H2, NC, NP, NP, sdz, g + h->off[4], h->status, s);
        if (e == hipSuccess) e = launch_colsum(h->dz, M, NP, h->part, g + h->off[5], s);
        if (e == hipSuccess)
            e = dropped ? launch_fc_dgrad_x3_dropout(h->dz, w + h->off[4], h->a2, M, H2, NC, NP, NP, sdz, head_scales(h, 4), dscale, h->d2, h->status, s)
                        : launch_fc_dgrad_x3(h->dz, w + h->off[4], h->a2, M, H2, NC, NP, NP, sdz, head_scales(h, 4), h->d2, h->status, s);
        if (e == hipSuccess) e = shift_of(h->d2, H2, H2, 1);
        if (e == hipSuccess) e = launch_fc_wgrad_x3(h->a1, h->d2, M, H1, H2, H2, H2, sd2, g + h->off[2], h->status, s);
        if (e == hipSuccess) e = launch_colsum(h->d2, M, H2, h->part, g + h->off[3], s);
        if (e == hipSuccess)
            e = dropped ? launch_fc_dgrad_x3_dropout(h->d2, w + h->off[2], h->a1, M, H1, H2, H2, H2, sd2, head_scales(h, 1), dscale, h->d1, h->status, s)
                        : launch_fc_dgrad_x3(h->d2, w + h->off[2], h->a1, M, H1, H2, H2, H2, sd2, head_scales(h, 1), h->d1, h->status, s);
        if (e == hipSuccess) e = shift_of(h->d1, H1, H1, 2);
        if (e == hipSuccess) e = launch_fc_wgrad_x3(d_pooled, h->d1, M, K1, H1, H1, H1, sd1, g + h->off[0], h->status, s);
        if (e == hipSuccess) e = launch_colsum(h->d1, M, H1, h->part, g + h->off[1], s);
        if (e == hipSuccess && d_grad_pooled)
            e = launch_fc_dgrad_x3(h->d1, w + h->off[0], nullptr, M, K1, H1, H1, H1, sd1, head_scales(h, 0), d_grad_pooled, h->status, s);
        if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
        return RPN_OK;
    }
    // the pair: dz = [grad_logits | grad_deltas | 0]; dWp = a2^T dz, dbp = sum dz, d2 = (dz Wp^T) [a2 > 0]
    hipError_t e = launch_pack_pair_grad(d_grad_logits, d_grad_deltas, M, h->c, NP, h->dz, s);
    if (e == hipSuccess) e = launch_conv1x1_wgrad(h->a2, h->dz, M, H2, NP, h->part, g + h->off[4], s);
    if (e == hipSuccess) e = launch_colsum(h->dz, M, NP, h->part, g + h->off[5], s);
    if (e == hipSuccess) e = launch_conv1x1_dgrad(h->dz, w + h->off[4], nullptr, M, H2, NP, h->d2, s);
    if (e == hipSuccess) e = dropped ? launch_relu_scale_mask(h->d2, h->a2, (long long)M * H2, dscale, s) : launch_relu_mask(h->d2, h->a2, (long long)M * H2, s);
    // fc2: dW2 = a1^T d2, db2 = sum d2, d1 = (d2 W2^T) [a1 > 0]
    if (e == hipSuccess) e = launch_conv1x1_wgrad(h->a1, h->d2, M, H1, H2, h->part, g + h->off[2], s);
    if (e == hipSuccess) e = launch_colsum(h->d2, M, H2, h->part, g + h->off[3], s);
    if (e == hipSuccess) e = launch_conv1x1_dgrad(h->d2, w + h->off[2], nullptr, M, H1, H2, h->d1, s);
    if (e == hipSuccess) e = dropped ? launch_relu_scale_mask(h->d1, h->a1, (long long)M * H1, dscale, s) : launch_relu_mask(h->d1, h->a1, (long long)M * H1, s);
    // fc1: dW1 = pooled^T d1, db1 = sum d1, grad_pooled = d1 W1^T when asked for
    if (e == hipSuccess) e = launch_conv1x1_wgrad(d_pooled, h->d1, M, K1, H1, h->part, g + h->off[0], s);
    if (e == hipSuccess) e = launch_colsum(h->d1, M, H1, h->part, g + h->off[1], s);
    if (e == hipSuccess && d_grad_pooled) e = launch_conv1x1_dgrad(h->d1, w + h->off[0], nullptr, M, K1, H1, d_grad_pooled, s);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_det_head_adam_step(rpn_det_head *h, float lr, float beta_1, float beta_2, float epsilon, void *stream)
{
    const char *who = "rpn_det_head_adam_step";
    RPN_REQUIRE(h, "%s: null head", who);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    RPN_REQUIRE(h->opt.kind == RPN_OPT_SGD || (beta_1 >= 0.0f && beta_1 < 1.0f && beta_2 >= 0.0f && beta_2 < 1.0f && epsilon > 0.0f),
                "%s: beta_1 = %g, beta_2 = %g, epsilon = %g", who, (double)beta_1, (double)beta_2, (double)epsilon);
    RPN_REQUIRE(h->loaded == 15u, "%s: set_layer has not been called for every layer (fc1, fc2, cls, reg)", who);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    h->kept_rows = 0;            // a kept forward was made with the weights this step changes
    hipError_t e = hipSuccess;
    if (h->opt.is_default()) {
        e = launch_adam(h->w, h->g, h->m, h->v, (long long)h->n, h->t + 1, lr, beta_1, beta_2, epsilon, as_stream(stream));
    } else {                     // another rule, a decay or a clip norm (under SGD beta_1, beta_2 and epsilon are ignored, lr is SGD's)
        const std::vector<long long> ranges = h->optdev.buf ? std::vector<long long>() : head_decay_ranges(h);
        const int so = optim_step(who, h->opt, &h->optdev, ranges.data(), (int)(ranges.size() / 2), h->w, h->g, h->m, h->v, (long long)h->n,
                                  h->t + 1, lr, beta_1, beta_2, epsilon, as_stream(stream));
        if (so != RPN_OK) return so;
    }
    h->x_stale = true;
    if (e == hipSuccess) e = head_fresh_image(h, as_stream(stream));          // split float16: repacked here, without a synchronisation
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    h->t += 1;
    return RPN_OK;
}

// ---- C ABI: the update rule and the optimizer's state (include/rpn_hip.h, "Optimizers") -------------------------------------------------
extern "C" int rpn_det_head_set_optimizer(rpn_det_head *h, int kind, float momentum, int nesterov, float weight_decay, float global_clipnorm)
{
    const char *who = "rpn_det_head_set_optimizer";
    RPN_REQUIRE(h, "%s: null head", who);
    const int st = optim_check_config(who, kind, momentum, nesterov, weight_decay, global_clipnorm);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0", who);
    h->kept_rows = 0;
    if (kind != h->opt.kind) {   // the other rule's m and v mean nothing to this one
        if (h->m) {
            RPN_HIP_CHECK(hipMemset(h->m, 0, h->n * sizeof(float)));
            RPN_HIP_CHECK(hipMemset(h->v, 0, h->n * sizeof(float)));
        }
        h->t = 0;
    }
    h->opt.kind = kind, h->opt.momentum = momentum, h->opt.nesterov = nesterov, h->opt.weight_decay = weight_decay;
    h->opt.clipnorm = global_clipnorm;
    h->optdev.stepped = false;
    return RPN_OK;
}

extern "C" int rpn_det_head_grad_norm(rpn_det_head *h, double *norm, float *scale, void *stream)
{
    RPN_REQUIRE(h, "rpn_det_head_grad_norm: null head");
    return optim_grad_norm("rpn_det_head_grad_norm", h->opt, h->optdev, norm, scale, as_stream(stream));
}

extern "C" int rpn_det_head_decay_ranges(const rpn_det_head *h, long long *ranges, int cap)
{
    if (!h) return -1;
    const std::vector<long long> r = head_decay_ranges(h);
    const int n = (int)(r.size() / 2);
    for (int i = 0; ranges && i < std::min(n, cap); ++i) ranges[2 * i] = r[2 * i], ranges[2 * i + 1] = r[2 * i + 1];
    return n;
}

static int head_slot_access(rpn_det_head *h, const char *who, const char *name, int slot, float *kernel, float *bias, bool write, void *stream)
{
    RPN_REQUIRE(h && name && kernel && bias, "%s: null pointer", who);
    RPN_REQUIRE(layer_index(name) >= 0, "%s: unknown layer '%s' (fc1, fc2, cls, reg)", who, name);
    RPN_REQUIRE(slot == 0 || slot == 1, "%s: slot %d (0: m, 1: v)", who, slot);
    RPN_REQUIRE(h->trainable, "%s: the head was created with trainable = 0: it has no optimizer state", who);
    const int st = head_ensure_device(h);
    if (st != RPN_OK) return st;
    if (write) h->kept_rows = 0;
    return head_copy_layer(h, slot == 0 ? h->m : h->v, name, kernel, bias, write, as_stream(stream));
}

extern "C" int rpn_det_head_get_slot(rpn_det_head *h, const char *name, int slot, float *kernel, float *bias, void *stream)
{
    return head_slot_access(h, "rpn_det_head_get_slot", name, slot, kernel, bias, false, stream);
}

extern "C" int rpn_det_head_set_slot(rpn_det_head *h, const char *name, int slot, const float *kernel, const float *bias)
{
    return head_slot_access(h, "rpn_det_head_set_slot", name, slot, const_cast<float *>(kernel), const_cast<float *>(bias), true, nullptr);
}

extern "C" int rpn_det_head_set_steps(rpn_det_head *h, long long steps)
{
    RPN_REQUIRE(h && steps >= 0, "rpn_det_head_set_steps: null head or steps = %lld < 0", steps);
    RPN_REQUIRE(h->trainable, "rpn_det_head_set_steps: the head was created with trainable = 0");
    h->kept_rows = 0;
    h->t = steps;
    return RPN_OK;
}

extern "C" int rpn_fc_forward(const float *d_a, const float *d_w, const float *d_bias, int M, int K, int N, int ldw, int relu,
                              float *d_out, void *stream)
{
    const char *who = "rpn_fc_forward";
    RPN_REQUIRE(d_a && d_w && d_out, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && M <= kFcMaxRows && N >= 1, "%s: M = %d (1 .. %lld), N = %d", who, M, kFcMaxRows, N);
    RPN_REQUIRE(K >= 4 && K % 4 == 0, "%s: K = %d must be a positive multiple of 4", who, K);
    RPN_REQUIRE(ldw >= N && ldw % 4 == 0, "%s: ldw = %d must be a multiple of 4 and >= N = %d", who, ldw, N);
    RPN_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    RPN_REQUIRE(aligned16(d_a) && aligned16(d_w), "%s: a and w must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_fc_forward(d_a, d_w, d_bias, M, K, N, ldw, relu, N, d_out, nullptr, as_stream(stream));
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_fc_forward_x3(const float *d_a, const float *d_w, const float *d_bias, int M, int K, int N, int ldw, int relu,
                                 float *d_out, unsigned *d_status, void *stream)
{
    const char *who = "rpn_fc_forward_x3";
    RPN_REQUIRE(d_a && d_w && d_out, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && M <= kFcMaxRows && N >= 1, "%s: M = %d (1 .. %lld), N = %d", who, M, kFcMaxRows, N);
    RPN_REQUIRE(K >= 4 && K % 4 == 0, "%s: K = %d must be a positive multiple of 4", who, K);
    RPN_REQUIRE(ldw >= N && ldw % 4 == 0, "%s: ldw = %d must be a multiple of 4 and >= N = %d", who, ldw, N);
    RPN_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    RPN_REQUIRE(aligned16(d_a) && aligned16(d_w), "%s: a and w must be 16-byte aligned", who);
    RPN_REQUIRE((reinterpret_cast<uintptr_t>(d_status) & 3u) == 0, "%s: the status word must be 4-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const hipStream_t s = as_stream(stream);
    // a test entry: max|w| over the columns [0, N), the packed image and the product, with a host round trip in between
    const size_t pbytes = fc_x3_packed_bytes(K, ldw);
    unsigned char *buf = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&buf), a256(pbytes) + 256);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: device allocation of %zu bytes failed: %s", who, pbytes, hipGetErrorString(e));
    unsigned *d_max = reinterpret_cast<unsigned *>(buf + a256(pbytes));
    float mx = 0.0f;
    e = hipMemsetAsync(d_max, 0, sizeof(unsigned), s);
    if (e == hipSuccess) e = launch_fc_absmax(d_w, K, N, ldw, d_max, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&mx, d_max, sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const int shift = split_weight_shift(&mx, 1, true);
    if (e == hipSuccess) e = launch_fc_pack_x3(d_w, K, ldw, 0, ldw, shift, buf, s);
    const float scale = ldexpf(1.0f, -shift);
    if (e == hipSuccess) e = launch_fc_forward_x3(d_a, buf, d_bias, M, K, N, ldw, relu, N, scale, scale, d_out, nullptr, d_status, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

namespace {

// the scale block of a test entry: the maximum's bits at word 0, pairs from word 8
hipError_t entry_scales(const float *t, int rows, int cols, int ld, bool gradient, unsigned *meta, int slot, hipStream_t s)
{
    hipError_t e = launch_fc_absmax(t, rows, cols, ld, meta + slot, s);
    if (e == hipSuccess) e = launch_fc_scales_x3(meta + slot, 1, -1, -1, gradient, reinterpret_cast<float *>(meta + 8) + 2 * slot, s);
    return e;
}

}  // namespace

extern "C" int rpn_fc_wgrad_x3(const float *d_a, const float *d_dz, int M, int K, int N, int ldz, int ldo, float *d_out,
                               unsigned *d_status, void *stream)
{
    const char *who = "rpn_fc_wgrad_x3";
    RPN_REQUIRE(d_a && d_dz && d_out, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && N >= 1, "%s: M = %d, N = %d", who, M, N);
    RPN_REQUIRE(K >= 4 && K % 4 == 0 && K <= kFcMaxRows, "%s: K = %d must be a positive multiple of 4 (at most %lld)", who, K, kFcMaxRows);
    RPN_REQUIRE(ldz >= N && ldz % 4 == 0, "%s: ldz = %d must be a multiple of 4 and >= N = %d", who, ldz, N);
    RPN_REQUIRE(ldo >= N, "%s: ldo = %d must be >= N = %d", who, ldo, N);
    RPN_REQUIRE(aligned16(d_a) && aligned16(d_dz), "%s: a and dz must be 16-byte aligned", who);
    RPN_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_status) & 3u) == 0,
                "%s: out and the status word must be 4-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const hipStream_t s = as_stream(stream);
    unsigned *meta = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&meta), 64 * sizeof(unsigned));
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: device allocation failed: %s", who, hipGetErrorString(e));
    e = hipMemsetAsync(meta, 0, 64 * sizeof(unsigned), s);
    if (e == hipSuccess) e = entry_scales(d_dz, M, N, ldz, true, meta, 0, s);
    if (e == hipSuccess) e = launch_fc_wgrad_x3(d_a, d_dz, M, K, N, ldz, ldo, reinterpret_cast<float *>(meta + 8), d_out, d_status, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(meta);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_fc_dgrad_x3(const float *d_dz, const float *d_w, int M, int K, int N, int ldz, int ldw, const float *d_h, float *d_out,
                               unsigned *d_status, void *stream)
{
    const char *who = "rpn_fc_dgrad_x3";
    RPN_REQUIRE(d_dz && d_w && d_out, "%s: null pointer", who);
    RPN_REQUIRE(M >= 1 && M <= kFcMaxRows && K >= 1 && N >= 1, "%s: M = %d (1 .. %lld), K = %d, N = %d", who, M, kFcMaxRows, K, N);
    RPN_REQUIRE(ldz >= N && ldz % 4 == 0 && ldw >= N && ldw % 4 == 0, "%s: ldz = %d and ldw = %d must be multiples of 4 and >= N = %d", who,
                ldz, ldw, N);
    RPN_REQUIRE(aligned16(d_dz) && aligned16(d_w), "%s: dz and w must be 16-byte aligned", who);
    RPN_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_h) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(d_status) & 3u) == 0, "%s: out, h and the status word must be 4-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const hipStream_t s = as_stream(stream);
    unsigned *meta = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&meta), 64 * sizeof(unsigned));
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: device allocation failed: %s", who, hipGetErrorString(e));
    float *sc = reinterpret_cast<float *>(meta + 8);
    e = hipMemsetAsync(meta, 0, 64 * sizeof(unsigned), s);
    if (e == hipSuccess) e = entry_scales(d_dz, M, N, ldz, true, meta, 0, s);
    if (e == hipSuccess) e = entry_scales(d_w, K, N, ldw, false, meta, 1, s);
    if (e == hipSuccess) e = launch_fc_dgrad_x3(d_dz, d_w, d_h, M, K, N, ldz, ldw, sc, sc + 2, d_out, d_status, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(meta);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RPN_OK;
}
