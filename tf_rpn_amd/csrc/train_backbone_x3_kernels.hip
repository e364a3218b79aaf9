// train_backbone_x3_kernels.hip -- the backward products of the VGG16 backbone in split float16 (RPN_PRECISION_F16X3 as a trainer's
// backward precision; contract in include/rpn_hip.h, "Training the backbone's backward in split float16"): the 3x3 input gradient
// (conv3x3_dgrad_x3_kernel) and the 3x3 weight + bias gradient (conv3x3_wgrad_x3_kernel) on v_mfma_f32_16x16x32_f16, the device-side
// max scan of a gradient tensor or a kernel, and the flip + transpose + split of a layer's kernel into the dgrad's packed image.
// They are the implicit GEMMs of train_backbone_kernels.hip (dgrad) and train_kernels.hip (wgrad) on the tile, the LDS records, the
// double buffer and the step order of the detection head's backward (det_head_x3_kernels.hip; shared device helpers in x3_tile.h).
// Host interface in train_backbone.h.  No floating-point atomics, every output written once: the same bits on every run.
#include <cstdint>

#include "det_head.h"
#include "rpn_common.h"
#include "train_backbone.h"
#include "train_common.h"
#include "x3_tile.h"

namespace rpn {

constexpr int kX3GridCap = 2048;        // workgroups of this file's grid-stride kernels

// max|x| over n4 float4s as the bits of a non-negative float, joined by an integer atomicMax (order-independent): a NaN never
// compares greater and is skipped, an infinity wins.  One atomic per wave.
__global__ void __launch_bounds__(256) conv_absmax_x3_kernel(const float4 *__restrict__ x, long long n4, unsigned *__restrict__ out_bits)
{
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = x[i];
        const float a[4] = {fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (a[k] > m) m = a[k];
    }
    unsigned b = __float_as_uint(m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)b, off);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b > 0u) atomicMax(out_bits, b);
}

// the same over n floats with 4-byte alignment only (a kernel slice of the trainer's flat master buffer: the slices follow the
// head's 5 K columns and are not 16-byte aligned); the maximum does not depend on the order, so both forms give the same bits
__global__ void __launch_bounds__(256) conv_absmax1_x3_kernel(const float *__restrict__ x, long long n, unsigned *__restrict__ out_bits)
{
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float a = fabsf(x[i]);
        if (a > m) m = a;
    }
    unsigned b = __float_as_uint(m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)b, off);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b > 0u) atomicMax(out_bits, b);
}

// ---- the dgrad's weight image ----------------------------------------------------------------------------------------------------------
// W'[k][ci] = 2^s W[8 - tap][ci][co], k = tap Cout + co, as the head's packed image (fc_pack_x3_kernel): chunk k / 32 holds, per
// column ci, a 128-byte record of four hi and four lo pieces, piece p at slot p ^ (ci / 2 % 8); k >= 9 Cout enters as zeros.  One
// thread per (ci, octet of k): 8 consecutive co of one tap are 32 contiguous bytes of w, and both pieces of them are written here.
// VEC: w is 16-byte aligned and the octet is read as two float4s (an octet starts at a multiple of 8 floats of w); otherwise -- the
// trainer's master kernels are only 4-byte aligned -- as eight scalar loads.  The values, and so the image, are the same.
template <bool VEC>
__global__ void __launch_bounds__(256) dgrad_pack_x3_kernel(const float *__restrict__ w, int Cin, int Cout, const float *__restrict__ wscale,
                                                           uint4 *__restrict__ packed)
{
    const int noct = (9 * Cout + kX3BK - 1) / kX3BK * 4;
    const long long total = (long long)Cin * noct;
    const float mul = wscale[0];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i / noct), oct = (int)(i - (long long)ci * noct), k = 8 * oct;
        float xs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (k < 9 * Cout) {
            const int tap = k / Cout, co = k - tap * Cout;
            const float *src = w + ((size_t)(8 - tap) * Cin + ci) * Cout + co;
            if (VEC) {
                const float4 a = reinterpret_cast<const float4 *>(src)[0], b = reinterpret_cast<const float4 *>(src)[1];
                xs[0] = a.x * mul; xs[1] = a.y * mul; xs[2] = a.z * mul; xs[3] = a.w * mul;
                xs[4] = b.x * mul; xs[5] = b.y * mul; xs[6] = b.z * mul; xs[7] = b.w * mul;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xs[j] = src[j] * mul;
            }
        }
        uint4 hi, lo;
        split8_x3(xs, hi, lo, nullptr);
        const int chunk = oct >> 2, p = oct & 3, sw = (ci >> 1) & 7;
        uint4 *rec = packed + ((size_t)chunk * Cin + ci) * 8;
        rec[p ^ sw] = hi;
        rec[(4 + p) ^ sw] = lo;
    }
}

// ---- dgrad: dX (P x Cin) = 2^-(t + s) (A (P x 9 Cout) W' (9 Cout x Cin)) ------------------------------------------------------------------
// A[p][tap Cout + co] = 2^t dY[b][y + r - 1][x + s - 1][co] (tap = 3 r + s, zero outside the image).  Workgroup: 128 pixels x 32 NJ
// input channels (NJ = 4 | 2), four waves of 64 x 16 NJ; the reduction in steps of 32 (Cout % 16 == 0: an octet of k never leaves its
// tap, a step may), staged global -> registers -> LDS, double buffered with one barrier per step.
//   A: a thread loads 8 consecutive channels of one shifted pixel of dY (two float4), multiplies by 2^t, splits them (the range
//      probe sits here) and writes the two pieces into the pixel's record, as the head's forward stages its A.
//   W': the columns of a step are contiguous in the image (guarded by column < Cin): NJ 16-byte copies per thread.
// 2 x (16 + 4 NJ) KB of LDS.  Every accumulator takes, per step in k order, lo*hi, hi*lo, hi*hi: the order over (tap, co) follows from
// the shape alone, is the same at either tile width, and a pixel's result reads no other pixel's tile.
// Epilogue: v = acc * 2^a * 2^b (x3_unscale_factors), then fl32(v + add[o]) when add is given (read before the store by the same
// lane: add may be dX, so neither pointer is __restrict__), then 0 where mask <= 0 when mask is given.
template <int NJ>
__global__ void __launch_bounds__(256) conv3x3_dgrad_x3_kernel(const float *__restrict__ dY, const uint4 *__restrict__ Wp,
                                                              const float *__restrict__ mask, const float *add, int B, int H, int W,
                                                              int Cin, int Cout, const float *__restrict__ gscale,
                                                              const float *__restrict__ wscale, float *dX, unsigned *__restrict__ status)
{
    constexpr int BN = 32 * NJ;
    __shared__ __attribute__((aligned(16))) uint4 As[2][kX3BM * 8];
    __shared__ __attribute__((aligned(16))) uint4 Bs[2][BN * 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const long long P = (long long)B * H * W, m0 = (long long)blockIdx.x * kX3BM;
    const int n0 = blockIdx.y * BN, K = 9 * Cout;
    const int nsteps = (K + kX3BK - 1) / kX3BK;
    const int ar = tid >> 2, ao = tid & 3;                       // A: pixels ar, ar + 64 of the tile; k octet ao
    const float gmul = gscale[0];
    bool a_ok[2];
    int ab[2], ay[2], ax[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long ap = m0 + ar + 64 * i;
        a_ok[i] = ap < P;
        ab[i] = ay[i] = ax[i] = 0;
        if (a_ok[i]) {
            const long long hw = (long long)H * W;
            ab[i] = (int)(ap / hw);
            const int rem = (int)(ap - (long long)ab[i] * hw);
            ay[i] = rem / W;
            ax[i] = rem - ay[i] * W;
        }
    }
    float4 ra[2][2];
    uint4 rb[NJ];
    auto load_global = [&](int step) {
        const int k = step * kX3BK + 8 * ao;
        const int tap = k / Cout, co = k - tap * Cout, dr = tap / 3 - 1, ds = tap % 3 - 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[i][0] = ra[i][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int yy = ay[i] + dr, xx = ax[i] + ds;
            if (a_ok[i] && k < K && yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const float4 *src = reinterpret_cast<const float4 *>(dY + (((size_t)ab[i] * H + yy) * W + xx) * Cout + co);
                ra[i][0] = src[0];
                ra[i][1] = src[1];
            }
        }
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int idx = tid + 256 * u, col = n0 + (idx >> 3);
            rb[u] = make_uint4(0u, 0u, 0u, 0u);
            if (col < Cin) rb[u] = Wp[((size_t)step * Cin + col) * 8 + (idx & 7)];
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float xs[8] = {ra[i][0].x * gmul, ra[i][0].y * gmul, ra[i][0].z * gmul, ra[i][0].w * gmul,
                                 ra[i][1].x * gmul, ra[i][1].y * gmul, ra[i][1].z * gmul, ra[i][1].w * gmul};
            uint4 hi, lo;
            split8_x3(xs, hi, lo, status);
            const int r = ar + 64 * i, sw = (r >> 1) & 7;
            As[buf][r * 8 + (ao ^ sw)] = hi;
            As[buf][r * 8 + ((4 + ao) ^ sw)] = lo;
        }
#pragma unroll
        for (int u = 0; u < NJ; ++u) Bs[buf][tid + 256 * u] = rb[u];
    };
    x3_f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;

    load_global(0);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        if (more) load_global(step + 1);
        x3_mma_step_n<NJ>(As[cur], Bs[cur], acc, wm, wn, l16, q);
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator element e of block (i, j): pixel row 16 i + 4 (lane / 16) + e, channel column 16 j + lane % 16
    float f1, f2;
    x3_unscale_factors(gscale[1], wscale[1], f1, f2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = n0 + wn * 16 * NJ + 16 * j + l16;
        if (col >= Cin) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long p = m0 + wm * 64 + 16 * i + 4 * q + e;
                if (p >= P) continue;
                const size_t o = (size_t)p * Cin + col;
                float v = acc[i][j][e] * f1 * f2;
                if (add) v = __fadd_rn(v, add[o]);
                if (mask && !(mask[o] > 0.0f)) v = 0.0f;
                dX[o] = v;
            }
    }
}

// ---- wgrad: slab (M1 x Cout) = 2^-t (A^T (2^t dY)) over one leaf's pixels ---------------------------------------------------------------
// Rows m = (3 r + s) Cin + ci are shifted columns of X (zero outside the image), row 9 Cin a row of ones (-> db = the sum of dY, formed
// by the same split product: hi = 1, lo = 0), columns are the output channels; leaf l = blockIdx.z takes the pixels
// [l P / leaves, (l + 1) P / leaves) in steps of 32 from its start, tails as zeros, and writes its own slab.  Staging is the head's
// "TN" form (fc_wgrad_x3_kernel): the reduction index (the pixel) is strided in both operands; threads 0-127 stage X, 128-255 dY; a
// thread loads one channel quad of the 8 pixels of one octet as float4s and then holds, per channel, the 8 pixel-consecutive values
// of one piece: the transposition happens in registers, the split (range probe included, on X and on 2^t dY) per piece.
__global__ void __launch_bounds__(256) conv3x3_wgrad_x3_kernel(const float *__restrict__ X, const float *__restrict__ dY, int B, int H, int W,
                                                              int Cin, int Cout, int leaves, const float *__restrict__ gscale,
                                                              float *__restrict__ part, unsigned *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint4 S[2][2][kX3BM * 8];     // [buffer][operand][record pieces]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l16 = lane & 15, q = lane >> 4;
    const int M = 9 * Cin, M1 = M + 1, n0 = blockIdx.x * kX3BN, m0 = blockIdx.y * kX3BM, leaf = blockIdx.z;
    const long long P = (long long)B * H * W;
    const int pbeg = (int)(P * leaf / leaves), pend = (int)(P * (leaf + 1) / leaves), hw = H * W;
    const int nsteps = (pend - pbeg + kX3BK - 1) / kX3BK;
    const int half = tid >> 7, cq = tid & 31, o = (tid >> 5) & 3;          // operand (wave-uniform), channel quad, octet of the step
    const int c0 = (half ? n0 : m0) + 4 * cq;
    const bool c_ok = half ? c0 < Cout : c0 < M, ones = !half && c0 == M;
    const int tap = c_ok && !half ? c0 / Cin : 0, ci = c_ok && !half ? c0 - tap * Cin : 0;
    const int dr = tap / 3 - 1, ds = tap % 3 - 1;
    const float mul = half ? gscale[0] : 1.0f;
    float4 r[8];
    // the image coordinates of this thread's first pixel of the current step, advanced by 32 pixels per step (the steps are loaded
    // in order); a shifted pixel's address is linear in the pixel index: X + (p + dr W + ds) Cin + ci
    int y0 = 0, x0 = 0;
    if (!half) {
        const int rem = (pbeg + 8 * o) % hw;
        y0 = rem / W;
        x0 = rem - y0 * W;
    }
    const long long shift = (long long)dr * W + ds;
    auto load_global = [&](int step) {
        const int p0 = pbeg + step * kX3BK + 8 * o;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (half) {
            const float *src = dY + (size_t)p0 * Cout + c0;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c_ok && p0 + j < pend) r[j] = *reinterpret_cast<const float4 *>(src + (size_t)j * Cout);
        } else {
            int y = y0, x = x0;
            const long long off = ((long long)p0 + shift) * Cin + ci;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (p0 + j < pend) {
                    const int yy = y + dr, xx = x + ds;
                    if (c_ok && yy >= 0 && yy < H && xx >= 0 && xx < W)
                        r[j] = *reinterpret_cast<const float4 *>(X + (off + (long long)j * Cin));
                    if (ones) r[j].x = 1.0f;
                }
                if (++x == W) {
                    x = 0;
                    if (++y == H) y = 0;
                }
            }
            x0 += kX3BK;
            while (x0 >= W) {
                x0 -= W;
                if (++y0 == H) y0 = 0;
            }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float xs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xs[j] = (c == 0 ? r[j].x : c == 1 ? r[j].y : c == 2 ? r[j].z : r[j].w) * mul;
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
    float *slab = part + (size_t)leaf * M1 * Cout;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + 16 * j + l16;
        if (col >= Cout) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wm * 64 + 16 * i + 4 * q + e;
                if (row < M1) slab[(size_t)row * Cout + col] = acc[i][j][e] * inv;
            }
    }
}

// ---- host launchers ----------------------------------------------------------------------------------------------------------------------
hipError_t launch_scale_x3(const float *x, long long n, bool gradient, unsigned *bits, float *scale, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    if ((reinterpret_cast<uintptr_t>(x) & 15u) == 0 && n % 4 == 0)
        hipLaunchKernelGGL(conv_absmax_x3_kernel, dim3(grid_1d(n / 4, kX3GridCap)), dim3(256), 0, s, reinterpret_cast<const float4 *>(x), n / 4, bits);
    else
        hipLaunchKernelGGL(conv_absmax1_x3_kernel, dim3(grid_1d(n, kX3GridCap)), dim3(256), 0, s, x, n, bits);
    return launch_fc_scales_x3(bits, 1, -1, -1, gradient, scale, s);
}

size_t dgrad_x3_image_bytes(int Cin, int Cout) { return (size_t)((9 * Cout + kX3BK - 1) / kX3BK) * (size_t)Cin * 128; }

bool conv3x3_dgrad_x3_wide_tile(int B, int H, int W, int Cin)
{
    const long long mt = ((long long)B * H * W + kX3BM - 1) / kX3BM;
    return (Cin - 1) % 128 >= 64 && mt * ((Cin + 127) / 128) >= 256;      // the last 128 columns more than half used, one tile per CU of 256
}

hipError_t launch_conv3x3_dgrad_x3(const float *dy, const float *w_hwio, const float *mask, const float *add, int B, int H, int W, int Cin,
                                   int Cout, const float *gscale, void *image, unsigned *wbits, float *wscale, float *dx, unsigned *status,
                                   hipStream_t s)
{
    hipError_t e = launch_scale_x3(w_hwio, 9LL * Cin * Cout, false, wbits, wscale, s);
    if (e != hipSuccess) return e;
    uint4 *img = reinterpret_cast<uint4 *>(image);
    const long long pieces = (long long)Cin * ((9 * Cout + kX3BK - 1) / kX3BK * 4);
    if ((reinterpret_cast<uintptr_t>(w_hwio) & 15u) == 0)
        hipLaunchKernelGGL(dgrad_pack_x3_kernel<true>, dim3(grid_1d(pieces, kX3GridCap)), dim3(256), 0, s, w_hwio, Cin, Cout, wscale, img);
    else
        hipLaunchKernelGGL(dgrad_pack_x3_kernel<false>, dim3(grid_1d(pieces, kX3GridCap)), dim3(256), 0, s, w_hwio, Cin, Cout, wscale, img);
    const unsigned mt = (unsigned)(((long long)B * H * W + kX3BM - 1) / kX3BM);
    if (conv3x3_dgrad_x3_wide_tile(B, H, W, Cin))
        hipLaunchKernelGGL(conv3x3_dgrad_x3_kernel<4>, dim3(mt, (Cin + 127) / 128), dim3(256), 0, s, dy, img, mask, add, B, H, W, Cin, Cout,
                           gscale, wscale, dx, status);
    else
        hipLaunchKernelGGL(conv3x3_dgrad_x3_kernel<2>, dim3(mt, (Cin + 63) / 64), dim3(256), 0, s, dy, img, mask, add, B, H, W, Cin, Cout,
                           gscale, wscale, dx, status);
    return hipGetLastError();
}

hipError_t launch_wgrad_wide_x3(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, const float *gscale, float *part,
                                float *dw, float *db, unsigned *status, hipStream_t s)
{
    const int L = wgrad_wide_leaves(B, H, W, Cin, Cout);
    const dim3 grid((Cout + kX3BN - 1) / kX3BN, (9 * Cin + 1 + kX3BM - 1) / kX3BM, L);
    hipLaunchKernelGGL(conv3x3_wgrad_x3_kernel, grid, dim3(256), 0, s, x, dy, B, H, W, Cin, Cout, L, gscale, part, status);
    return launch_wgrad_wide_sum(part, L, Cin, Cin, Cout, dw, db, s);
}

}  // namespace rpn

using namespace rpn;

// ---- C ABI: single-layer entries (the workspace ends with 256 bytes of max / scale words: the maxima's bits at words 0 (dy) and 1
// (w), the pairs {2^t, 2^-t} and {2^s, 2^-s} from word 8) -------------------------------------------------------------------------------
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

extern "C" size_t rpn_conv3x3_dgrad_x3_workspace_bytes(int Cin, int Cout)
{
    if (Cin < 4 || Cout < 16 || Cin % 4 || Cout % 16 || (long long)9 * Cin * Cout > (1ll << 30)) return 0;
    return a256(dgrad_x3_image_bytes(Cin, Cout)) + 256;
}

extern "C" int rpn_conv3x3_dgrad_x3_tile_n(int B, int H, int W, int Cin)
{
    if (B < 1 || H < 1 || W < 1 || Cin < 4) return 0;
    return conv3x3_dgrad_x3_wide_tile(B, H, W, Cin) ? 128 : 64;
}

extern "C" int rpn_conv3x3_dgrad_x3(const float *d_dy, const float *d_w, const float *d_mask, const float *d_add, int B, int H, int W,
                                    int Cin, int Cout, float *d_dx, unsigned *d_status, void *d_ws, size_t ws_bytes, void *stream)
{
    const char *who = "rpn_conv3x3_dgrad_x3";
    RPN_REQUIRE(d_dy && d_w && d_dx, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 4 && Cout >= 16, "%s: bad shape", who);
    RPN_REQUIRE(Cin % 4 == 0 && Cout % 16 == 0, "%s: Cin must be a multiple of 4 and Cout of 16", who);
    RPN_REQUIRE((long long)9 * Cin * Cout <= (1ll << 30) && (long long)H * W <= (1 << 30) && (long long)B * H * W <= (1ll << 36),
                "%s: layer too large", who);
    RPN_REQUIRE(aligned16(d_dy) && aligned16(d_ws), "%s: dy and the workspace must be 16-byte aligned", who);
    RPN_REQUIRE(aligned4(d_w) && aligned4(d_dx) && aligned4(d_mask) && aligned4(d_add) && aligned4(d_status),
                "%s: w, dx, mask, add and the status word must be 4-byte aligned", who);
    const size_t need = rpn_conv3x3_dgrad_x3_workspace_bytes(Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "%s: %zu bytes of workspace needed", who, need);
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    unsigned *meta = reinterpret_cast<unsigned *>((char *)d_ws + need - 256);
    float *sc = reinterpret_cast<float *>(meta + 8);
    hipError_t e = launch_scale_x3(d_dy, (long long)B * H * W * Cout, true, meta, sc, s);
    if (e == hipSuccess)
        e = launch_conv3x3_dgrad_x3(d_dy, d_w, d_mask, d_add, B, H, W, Cin, Cout, sc, d_ws, meta + 1, sc + 2, d_dx, d_status, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
}

static bool wgrad_x3_shape_ok(int B, int H, int W, int Cin, int Cout)
{
    return B >= 1 && H >= 1 && W >= 1 && Cin >= 4 && Cout >= 4 && Cout % 4 == 0 && (long long)9 * Cin * Cout <= (1ll << 30) &&
           (long long)B * H * W < (1ll << 31) - 64;
}

extern "C" size_t rpn_conv3x3_wgrad_wide_x3_workspace_bytes(int B, int H, int W, int Cin, int Cout)
{
    if (!wgrad_x3_shape_ok(B, H, W, Cin, Cout) || Cin % 4) return 0;
    return a256(wgrad_wide_ws_floats(B, H, W, Cin, Cout) * sizeof(float)) + 256;
}

extern "C" int rpn_conv3x3_wgrad_wide_x3(const float *d_x, const float *d_dy, int B, int H, int W, int Cin, int Cout, float *d_dw,
                                         float *d_db, unsigned *d_status, void *d_ws, size_t ws_bytes, void *stream)
{
    const char *who = "rpn_conv3x3_wgrad_wide_x3";
    RPN_REQUIRE(d_x && d_dy && d_dw && d_db, "%s: null pointer", who);
    if (Cin == 3)
        return fail(RPN_ERR_UNSUPPORTED, "%s: Cin = 3 (block1_conv1) stays on the float32 kernel: rpn_conv3x3_wgrad_wide", who);
    RPN_REQUIRE(Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0, "%s: bad shape (Cin and Cout multiples of 4)", who);
    RPN_REQUIRE(wgrad_x3_shape_ok(B, H, W, Cin, Cout), "%s: bad shape, or layer too large", who);
    RPN_REQUIRE(aligned16(d_x) && aligned16(d_dy) && aligned16(d_ws), "%s: x, dy and the workspace must be 16-byte aligned", who);
    RPN_REQUIRE(aligned4(d_dw) && aligned4(d_db) && aligned4(d_status), "%s: dw, db and the status word must be 4-byte aligned", who);
    const size_t need = rpn_conv3x3_wgrad_wide_x3_workspace_bytes(B, H, W, Cin, Cout);
    if (!d_ws || ws_bytes < need) return fail(RPN_ERR_WORKSPACE, "%s: %zu bytes of workspace needed", who, need);
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    unsigned *meta = reinterpret_cast<unsigned *>((char *)d_ws + need - 256);
    float *sc = reinterpret_cast<float *>(meta + 8);
    hipError_t e = launch_scale_x3(d_dy, (long long)B * H * W * Cout, true, meta, sc, s);
    if (e == hipSuccess) e = launch_wgrad_wide_x3(d_x, d_dy, B, H, W, Cin, Cout, sc, reinterpret_cast<float *>(d_ws), d_dw, d_db, d_status, s);
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
}
