// train_backbone_kernels.hip -- the backward pass of the VGG16 backbone (reference models/rpn_vgg16.py:16-21: the Keras base model is
// trainable, trainer.py:54-69 compiles and fits all of it): 3x3 input gradients (dgrad), 3x3 weight + bias gradients at backbone
// shapes (wgrad_wide) and the MaxPooling2D(2, 2) backward.  The training step that chains them lives in trainer.hip.  The wgrad's MFMA
// kernel is conv3x3_wgrad_f32_kernel<true> of train_kernels.hip (launch_wgrad_slabs, train_head.h): here are its leaf rule and its
// slab tree.  The helpers shared with the other training kernel files are in train_common.h.
//
// Gradient forms (TF 2.0.0, restated from its sources as recalled -- nothing here can run TF):
//   ReluGrad(grad, op.outputs[0]):  dY * [Y > 0], Y the ReLU OUTPUT (nn_grad.py _ReluGrad).
//   MaxPoolGrad on the CPU (maxpooling_op.cc, SpatialMaxPoolWithArgMaxHelper): each window's gradient goes to its first maximum in
//     row-major window order -- a later value replaces it only when strictly greater; inputs no window covers get 0.
//   Conv2DBackpropInput of a stride-1 'same' 3x3 conv: the forward conv of dY with W'[r][s][co][ci] = W[2-r][2-s][ci][co].
//   Conv2DBackpropFilter: dW[r][s][ci][co] = sum_{b,y,x} X[b][y+r-1][x+s-1][ci] dY[b][y][x][co];  BiasAddGrad: db = sum dY.
// No floating-point atomics: every sum has a fixed order, so the bits do not depend on the device or the run.
#include <algorithm>

#include "rpn_common.h"
#include "train_backbone.h"
#include "train_common.h"
#include "train_head.h"

namespace rpn {

constexpr int kGridCap = 4096;          // workgroups of this file's grid-stride kernels

// ---- dgrad: dX (P x Cin) = A (P x 9 Cout) Wt (9 Cout x Cin) on v_mfma_f32_32x32x2_f32 -----------------------------------------
// A[p][tap Cout + co] = dY[b][y + r - 1][x + s - 1][co] (tap = 3 r + s, zero outside the image), Wt[tap Cout + co][ci] =
// W[8 - tap][ci][co] (dgrad_weights_kernel).  Workgroup: 128 pixels x 64 WN input channels, four waves of 64 x 32 WN; K slices of 16
// (one tap, 16 output channels: Cout % 16 == 0) staged global -> registers -> LDS, double-buffered with one barrier per slice, as
// conv3x3_wgrad_f32_kernel stages its operands.  The K order of every output is the same at every tile width: the same bits.
// Epilogue: + add[o] when given (a gradient that reaches the same tensor by another path, read in place: same lane, same address as
// the store, read before it, and dX carries no __restrict__ there, so add may be dX itself), then the ReLU mask of the layer's input (mask > 0), when given.
// The add is chosen at compile time (ADD): conv3x3_dgrad_f32_kernel is the body without it, conv3x3_dgrad_add_f32_kernel with it.
constexpr int kDgBM = 128, kDgBK = 16, kDgLdA = 160;   // A rows of 160 floats: the two half-waves of a fragment read hit disjoint banks

// dX is __restrict__ in the plain kernel only: with ADD the addend may BE dX (in place), so neither pointer may promise the other away
template <bool ADD> struct DgradOut { using type = float *__restrict__; };
template <> struct DgradOut<true> { using type = float *; };

template <int WN, bool ADD>
__device__ __forceinline__ void conv3x3_dgrad_f32_body(const float *__restrict__ dY, const float *__restrict__ Wt,
                                                       const float *__restrict__ mask, const float *add, int B, int H, int W, int Cin,
                                                       int Cout, typename DgradOut<ADD>::type dX)
{
    constexpr int BN = 64 * WN, LDB = WN == 2 ? 160 : 96, QPR = BN / 4, RPP = 256 / QPR;   // quads per B row, B rows per pass
    __shared__ float As[2][kDgBK][kDgLdA];
    __shared__ float Bs[2][kDgBK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l32 = lane & 31, kh = lane >> 5;
    const long long P = (long long)B * H * W;
    const long long m0 = (long long)blockIdx.x * kDgBM;
    const int n0 = blockIdx.y * BN;
    const int nsteps = 9 * Cout / kDgBK;

    // A loader: pixel ai of the tile, channels 8 ah .. 8 ah + 7 of the slice
    const int ai = tid >> 1, ah = tid & 1;
    const long long ap = m0 + ai;
    const bool a_ok = ap < P;
    int ab = 0, ay = 0, ax = 0;
    if (a_ok) {
        const long long hw = (long long)H * W;
        ab = (int)(ap / hw);
        const int rem = (int)(ap - (long long)ab * hw);
        ay = rem / W;
        ax = rem - ay * W;
    }
    // B loader: rows bk + RPP u of the slice, 4-channel quad bq
    const int bq = tid % QPR, bk = tid / QPR, bn = n0 + 4 * bq;
    const bool b_ok = bn < Cin;
    float4 ra[2], rb[WN];
    auto load_global = [&](int step) {
        const int k0 = step * kDgBK, tap = k0 / Cout, co = k0 - tap * Cout + 8 * ah;
        const int yy = ay + tap / 3 - 1, xx = ax + tap % 3 - 1;
        ra[0] = ra[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a_ok && yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const float4 *src = reinterpret_cast<const float4 *>(dY + (((size_t)ab * H + yy) * W + xx) * Cout + co);
            ra[0] = src[0];
            ra[1] = src[1];
        }
#pragma unroll
        for (int u = 0; u < WN; ++u)
            rb[u] = b_ok ? *reinterpret_cast<const float4 *>(Wt + (size_t)(k0 + bk + RPP * u) * Cin + bn) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    auto store_lds = [&](int buf) {
        const int r = 8 * ah;
        As[buf][r + 0][ai] = ra[0].x; As[buf][r + 1][ai] = ra[0].y; As[buf][r + 2][ai] = ra[0].z; As[buf][r + 3][ai] = ra[0].w;
        As[buf][r + 4][ai] = ra[1].x; As[buf][r + 5][ai] = ra[1].y; As[buf][r + 6][ai] = ra[1].z; As[buf][r + 7][ai] = ra[1].w;
#pragma unroll
        for (int u = 0; u < WN; ++u) *reinterpret_cast<float4 *>(&Bs[buf][bk + RPP * u][4 * bq]) = rb[u];
    };

    f32x16t acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int am = wm * 64 + l32, bnl = wn * 32 * WN + l32;

    load_global(0);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global(step + 1);
#pragma unroll
        for (int kk = 0; kk < kDgBK / 2; ++kk) {
            float av[2], bv[WN];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = As[cur][2 * kk + kh][am + 32 * i];
#pragma unroll
            for (int j = 0; j < WN; ++j) bv[j] = Bs[cur][2 * kk + kh][bnl + 32 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator element e of block (i, j): pixel row 8 (e / 4) + 4 kh + e % 4, channel column lane % 32
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int col = n0 + bnl + 32 * j;
            if (col >= Cin) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long p = m0 + wm * 64 + 32 * i + 8 * (e >> 2) + 4 * kh + (e & 3);
                if (p >= P) continue;
                const size_t o = (size_t)p * Cin + col;
                float v = acc[i][j][e];
                if (ADD) v += add[o];
                if (mask && !(mask[o] > 0.0f)) v = 0.0f;
                dX[o] = v;
            }
        }
}

template <int WN>
__global__ void __launch_bounds__(256) conv3x3_dgrad_f32_kernel(const float *__restrict__ dY, const float *__restrict__ Wt,
                                                              const float *__restrict__ mask, int B, int H, int W, int Cin, int Cout,
                                                              float *__restrict__ dX)
{
    conv3x3_dgrad_f32_body<WN, false>(dY, Wt, mask, nullptr, B, H, W, Cin, Cout, dX);
}

// the same tile with the addend in the epilogue: a kernel of its own, so that the plain one keeps its code and its registers
template <int WN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) conv3x3_dgrad_add_f32_kernel(const float *__restrict__ dY, const float *__restrict__ Wt,
                                                                  const float *__restrict__ mask, const float *add, int B, int H, int W,
                                                                  int Cin, int Cout, float *dX)
{
    conv3x3_dgrad_f32_body<WN, true>(dY, Wt, mask, add, B, H, W, Cin, Cout, dX);
}

// Wt[tap Cout + co][ci] = W[8 - tap][ci][co]
__global__ void __launch_bounds__(256) dgrad_weights_kernel(const float *__restrict__ w, int Cin, int Cout, float *__restrict__ wt)
{
    const long long n = 9LL * Cin * Cout;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        const long long rest = i / Cin;
        const int co = (int)(rest % Cout), tap = (int)(rest / Cout);
        wt[i] = w[((size_t)(8 - tap) * Cin + ci) * Cout + co];
    }
}

bool conv3x3_dgrad_wide_tile(int B, int H, int W, int Cin)
{
    const long long mt = ((long long)B * H * W + kDgBM - 1) / kDgBM;
    return Cin >= 128 && mt * ((Cin + 127) / 128) >= 512;      // 128 x 128 tiles only when they still give two per CU of 256
}

hipError_t launch_conv3x3_dgrad(const float *dy, const float *w_hwio, const float *mask, const float *add, int B, int H, int W, int Cin,
                                int Cout, float *wt, float *dx, hipStream_t s)
{
    hipLaunchKernelGGL(dgrad_weights_kernel, dim3(grid_1d(9LL * Cin * Cout, kGridCap)), dim3(256), 0, s, w_hwio, Cin, Cout, wt);
    const unsigned mt = (unsigned)(((long long)B * H * W + kDgBM - 1) / kDgBM);
    const bool wide = conv3x3_dgrad_wide_tile(B, H, W, Cin);
    const dim3 grid(mt, wide ? (Cin + 127) / 128 : (Cin + 63) / 64);
    if (wide && add)
        hipLaunchKernelGGL(conv3x3_dgrad_add_f32_kernel<2>, grid, dim3(256), 0, s, dy, wt, mask, add, B, H, W, Cin, Cout, dx);
    else if (wide)
        hipLaunchKernelGGL(conv3x3_dgrad_f32_kernel<2>, grid, dim3(256), 0, s, dy, wt, mask, B, H, W, Cin, Cout, dx);
    else if (add)
        hipLaunchKernelGGL(conv3x3_dgrad_add_f32_kernel<1>, grid, dim3(256), 0, s, dy, wt, mask, add, B, H, W, Cin, Cout, dx);
    else
        hipLaunchKernelGGL(conv3x3_dgrad_f32_kernel<1>, grid, dim3(256), 0, s, dy, wt, mask, B, H, W, Cin, Cout, dx);
    return hipGetLastError();
}

// ---- MaxPooling2D(2, 2) 'valid' backward + the ReLU mask of the pooled tensor -----------------------------------------------
// One thread per 4 channels of one input position: every element of dy is written once (no memset).
__global__ void __launch_bounds__(256) maxpool2x2_backward_kernel(const float *__restrict__ y, const float *__restrict__ dpool, int B, int H,
                                                                int W, int C, float *__restrict__ dy)
{
    const int C4 = C >> 2, OH = H >> 1, OW = W >> 1;
    const long long n = (long long)B * H * W * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const long long pix = i / C4;
        const int x = (int)(pix % W);
        const long long r = pix / W;
        const int yy = (int)(r % H), b = (int)(r / H);
        const int py = yy >> 1, px = x >> 1;
        float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (py < OH && px < OW) {
            const float *base = y + (((size_t)b * H + 2 * py) * W + 2 * px) * C + c;
            float4 v[4];
            v[0] = *reinterpret_cast<const float4 *>(base);
            v[1] = *reinterpret_cast<const float4 *>(base + C);
            v[2] = *reinterpret_cast<const float4 *>(base + (size_t)W * C);
            v[3] = *reinterpret_cast<const float4 *>(base + (size_t)W * C + C);
            const float4 g = *reinterpret_cast<const float4 *>(dpool + (((size_t)b * OH + py) * OW + px) * C + c);
            const int own = 2 * (yy & 1) + (x & 1);
            float res[4];
            const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float w0 = v[0][k], w1 = v[1][k], w2 = v[2][k], w3 = v[3][k];
                int arg = 0;
                float best = w0;
                if (w1 > best) { best = w1; arg = 1; }
                if (w2 > best) { best = w2; arg = 2; }
                if (w3 > best) { best = w3; arg = 3; }
                res[k] = (arg == own && best > 0.0f) ? gv[k] : 0.0f;
            }
            out = make_float4(res[0], res[1], res[2], res[3]);
        }
        *reinterpret_cast<float4 *>(dy + (size_t)pix * C + c) = out;
    }
}

hipError_t launch_maxpool2x2_backward(const float *y, const float *dpool, int B, int H, int W, int C, float *dy, hipStream_t s)
{
    hipLaunchKernelGGL(maxpool2x2_backward_kernel, dim3(grid_1d((long long)B * H * W * (C / 4), kGridCap)), dim3(256), 0, s, y, dpool, B, H, W, C, dy);
    return hipGetLastError();
}

// ---- wgrad at backbone shapes ---------------------------------------------------------------------------------------------------
// C (M1 x Cout) = A^T B over the pixels, M1 = 9 Cin + 1, on conv3x3_wgrad_f32_kernel<true> (train_kernels.hip): rows 0 .. 9 Cin - 1
// the weight gradient (row (3 r + s) Cin + ci), row 9 Cin a row of ones (-> db).  Leaf l of wgrad_wide_leaves(...) takes pixels
// [l P / leaves, (l + 1) P / leaves) and writes its own slab; wgrad_tree_kernel / wgrad_wide_finish_kernel add the slabs pairwise.

// one level of the fixed tree: slab i += slab i + half, i < half
__global__ void __launch_bounds__(256) wgrad_tree_kernel(float *__restrict__ part, long long len, int half)
{
    const long long n = (long long)half * len;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) part[j] = part[j] + part[n + j];
}

// the last level (slab 0 + slab 1, or slab 0 alone) -> dw (3,3,Cin,Cout) without the padded channels, db (Cout) from row 9 cin_x
__global__ void __launch_bounds__(256) wgrad_wide_finish_kernel(const float *__restrict__ part, int two, int cin_x, int Cin, int Cout,
                                                              float *__restrict__ dw, float *__restrict__ db)
{
    const long long len = (9LL * cin_x + 1) * Cout;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < len; j += (long long)gridDim.x * 256) {
        const float v = two ? part[j] + part[len + j] : part[j];
        const int row = (int)(j / Cout), co = (int)(j - (long long)row * Cout);
        if (row == 9 * cin_x) {
            db[co] = v;
        } else {
            const int tap = row / cin_x, ci = row - tap * cin_x;
            if (ci < Cin) dw[((size_t)tap * Cin + ci) * Cout + co] = v;
        }
    }
}

int wgrad_wide_leaves(int B, int H, int W, int Cin, int Cout)
{
    const int cin_x = (Cin + 3) & ~3;
    const long long tiles = (long long)((Cout + kWgBN - 1) / kWgBN) * ((9 * cin_x + 1 + kWgBM - 1) / kWgBM);
    const long long P = (long long)B * H * W;
    int L = 1;                                     // 1024 workgroups (four per CU of 256) or >= 512 pixels per leaf
    while (L < 1024 && tiles * L < 1024 && P / (2 * L) >= 512) L *= 2;
    return L;
}

size_t wgrad_wide_ws_floats(int B, int H, int W, int Cin, int Cout)
{
    const int cin_x = (Cin + 3) & ~3;
    return (size_t)wgrad_wide_leaves(B, H, W, Cin, Cout) * (9 * (size_t)cin_x + 1) * Cout;
}

hipError_t launch_wgrad_wide_sum(float *part, int L, int cin_x, int Cin, int Cout, float *dw, float *db, hipStream_t s)
{
    const long long len = (9LL * cin_x + 1) * Cout;
    for (int half = L / 2; half >= 2; half /= 2)
        hipLaunchKernelGGL(wgrad_tree_kernel, dim3(grid_1d(half * len, kGridCap)), dim3(256), 0, s, part, len, half);
    hipLaunchKernelGGL(wgrad_wide_finish_kernel, dim3(grid_1d(len, kGridCap)), dim3(256), 0, s, part, L >= 2 ? 1 : 0, cin_x, Cin, Cout, dw, db);
    return hipGetLastError();
}

hipError_t launch_wgrad_wide(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, float *part, float *dw, float *db,
                             hipStream_t s)
{
    const int cin_x = (Cin + 3) & ~3, L = wgrad_wide_leaves(B, H, W, Cin, Cout);
    launch_wgrad_slabs(x, dy, B, H, W, cin_x, Cout, L, true, part, s);
    return launch_wgrad_wide_sum(part, L, cin_x, Cin, Cout, dw, db, s);
}

__global__ void __launch_bounds__(256) pad_channels3to4_kernel(const float *__restrict__ x, long long P, float *__restrict__ out)
{
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256)
        *reinterpret_cast<float4 *>(out + 4 * p) = make_float4(x[3 * p], x[3 * p + 1], x[3 * p + 2], 0.0f);
}

hipError_t launch_pad_channels3to4(const float *x, long long P, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(pad_channels3to4_kernel, dim3(grid_1d(P, kGridCap)), dim3(256), 0, s, x, P, out);
    return hipGetLastError();
}

}  // namespace rpn

using namespace rpn;

// ---- C ABI: single-layer entries -----------------------------------------------------------------------------------------------
extern "C" size_t rpn_conv3x3_dgrad_workspace_bytes(int Cin, int Cout)
{
    if (Cin < 1 || Cout < 1) return 0;
    return a256((size_t)9 * Cin * Cout * sizeof(float));
}

extern "C" int rpn_conv3x3_dgrad(const float *d_dy, const float *d_w, const float *d_mask, int B, int H, int W, int Cin, int Cout,
                                 float *d_dx, void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_dy && d_w && d_dx, "rpn_conv3x3_dgrad: null pointer");
    RPN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 4 && Cout >= 16, "rpn_conv3x3_dgrad: bad shape");
    RPN_REQUIRE(Cin % 4 == 0 && Cout % 16 == 0, "rpn_conv3x3_dgrad: Cin must be a multiple of 4 and Cout of 16");
    RPN_REQUIRE((long long)9 * Cin * Cout <= (1ll << 30) && (long long)H * W <= (1 << 30) && (long long)B * H * W <= (1ll << 36),
                "rpn_conv3x3_dgrad: layer too large");
    const size_t need = rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_conv3x3_dgrad: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_conv3x3_dgrad(d_dy, d_w, d_mask, nullptr, B, H, W, Cin, Cout, reinterpret_cast<float *>(d_ws), d_dx,
                                              as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv3x3_dgrad: %s", hipGetErrorString(e));
}

extern "C" int rpn_conv3x3_dgrad_add(const float *d_dy, const float *d_w, const float *d_mask, const float *d_add, int B, int H, int W,
                                     int Cin, int Cout, float *d_dx, void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_dy && d_w && d_add && d_dx, "rpn_conv3x3_dgrad_add: null pointer");
    RPN_REQUIRE(((uintptr_t)d_add & 3) == 0, "rpn_conv3x3_dgrad_add: d_add must be 4-byte aligned");
    RPN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 4 && Cout >= 16, "rpn_conv3x3_dgrad_add: bad shape");
    RPN_REQUIRE(Cin % 4 == 0 && Cout % 16 == 0, "rpn_conv3x3_dgrad_add: Cin must be a multiple of 4 and Cout of 16");
    RPN_REQUIRE((long long)9 * Cin * Cout <= (1ll << 30) && (long long)H * W <= (1 << 30) && (long long)B * H * W <= (1ll << 36),
                "rpn_conv3x3_dgrad_add: layer too large");
    const size_t need = rpn_conv3x3_dgrad_workspace_bytes(Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_conv3x3_dgrad_add: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_conv3x3_dgrad(d_dy, d_w, d_mask, d_add, B, H, W, Cin, Cout, reinterpret_cast<float *>(d_ws), d_dx,
                                              as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv3x3_dgrad_add: %s", hipGetErrorString(e));
}

extern "C" int rpn_conv3x3_dgrad_tile_n(int B, int H, int W, int Cin)
{
    if (B < 1 || H < 1 || W < 1 || Cin < 4) return 0;
    return conv3x3_dgrad_wide_tile(B, H, W, Cin) ? 128 : 64;
}

extern "C" int rpn_maxpool2x2_backward(const float *d_y, const float *d_dpool, int B, int H, int W, int C, float *d_dy, void *stream)
{
    RPN_REQUIRE(d_y && d_dpool && d_dy, "rpn_maxpool2x2_backward: null pointer");
    RPN_REQUIRE(B >= 1 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0, "rpn_maxpool2x2_backward: bad shape (H, W >= 2, C a multiple of 4)");
    RPN_REQUIRE((long long)H * W <= (1 << 30), "rpn_maxpool2x2_backward: layer too large");
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_maxpool2x2_backward(d_y, d_dpool, B, H, W, C, d_dy, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_maxpool2x2_backward: %s", hipGetErrorString(e));
}

static bool wgrad_wide_shape_ok(int B, int H, int W, int Cin, int Cout)
{
    return B >= 1 && H >= 1 && W >= 1 && (Cin == 3 || (Cin >= 4 && Cin % 4 == 0)) && Cout >= 4 && Cout % 4 == 0;
}

extern "C" size_t rpn_conv3x3_wgrad_wide_workspace_bytes(int B, int H, int W, int Cin, int Cout)
{
    if (!wgrad_wide_shape_ok(B, H, W, Cin, Cout)) return 0;
    const size_t pad = Cin == 3 ? a256((size_t)B * H * W * 4 * sizeof(float)) : 0;
    return a256(wgrad_wide_ws_floats(B, H, W, Cin, Cout) * sizeof(float)) + pad;
}

extern "C" int rpn_conv3x3_wgrad_wide(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw, float *d_db,
                                      void *d_ws, size_t ws_bytes, void *stream)
{
    RPN_REQUIRE(d_x && d_dy && d_dw && d_db, "rpn_conv3x3_wgrad_wide: null pointer");
    RPN_REQUIRE(wgrad_wide_shape_ok(B, H, W, Cin, Cout), "rpn_conv3x3_wgrad_wide: bad shape (Cin 3 or a multiple of 4, Cout a multiple of 4)");
    RPN_REQUIRE((long long)9 * Cin * Cout <= (1ll << 30) && (long long)H * W <= (1 << 30) && (long long)B * H * W <= (1ll << 36),
                "rpn_conv3x3_wgrad_wide: layer too large");
    const size_t need = rpn_conv3x3_wgrad_wide_workspace_bytes(B, H, W, Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "rpn_conv3x3_wgrad_wide: %zu bytes of workspace needed", need);
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    float *part = reinterpret_cast<float *>(d_ws);
    const float *x = d_x;
    hipError_t e = hipSuccess;
    if (Cin == 3) {
        float *x4 = part + a256(wgrad_wide_ws_floats(B, H, W, Cin, Cout) * sizeof(float)) / sizeof(float);
        e = launch_pad_channels3to4(d_x, (long long)B * H * W, x4, s);
        x = x4;
    }
    if (e == hipSuccess) e = launch_wgrad_wide(x, d_dy, B, H, W, Cin, Cout, part, d_dw, d_db, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "rpn_conv3x3_wgrad_wide: %s", hipGetErrorString(e));
}
