// conv_cin3_kernels.hip -- the first layer (Cin = 3, 3x3: VGG16 block1_conv1, MobileNetV2 Conv1), three kernels:
//   conv_cin3_mfma_kernel      split-precision modes, on the 16-bit matrix cores (K = 27 padded to one 16x16x32 step)
//   conv_cin3_kernel           direct convolution on the vector ALU, float32 or SPLIT16 output
//   conv_cin3_f32_mfma_kernel  float32 graphs, on the float32 matrix pipe
// with the MFMA form's weight packer and the two launchers.  (VGG16's f16x3 headline runs this layer inside vgg_block1:
// conv_split_kernels.hip.)
#include "split_conv.h"

namespace rpn {

// ---- first layer on the matrix cores (split-precision modes) ---------------------------------------------------
// Cin = 3, 3x3: K = 27 is padded to 32 = ONE v_mfma_f32_16x16x32 step.  Workgroup = 8 x 32 output pixels x Cout
// (Cout = 16 * NTILES <= 64), 4 waves, each 2 rows.  The float32 input patch is staged in LDS; every lane gathers
// the 8 patch values of its (pixel, k-group) from LDS and splits them into hi / lo halves on the fly (the A
// fragment of the im2col matrix, never materialised); the pre-split weights are read from LDS once and stay in
// registers.  3 MFMAs per (16 px x 16 ch) tile.  ~4x fewer vector-ALU instructions per output than the direct
// kernel, so the layer becomes bound by its 4*Cout bytes per pixel of output.
template <bool F16, bool OUT_SPLIT, int STRIDE, int NTILES>
__global__ void __launch_bounds__(256)
conv_cin3_mfma_kernel(const float *__restrict__ x, const uint4 *__restrict__ w /* [Cout_pad][8 pieces] */,
                      const float *__restrict__ bias, void *__restrict__ out, int B, int H, int W, int OH, int OW,
                      int pad_t, int pad_l, int act, float out_scale, int tiles_x, int tiles_y, unsigned *status)
{
    constexpr int COUT = 16 * NTILES;
    constexpr int PR = 7 * STRIDE + 3, PC = 31 * STRIDE + 3;            // input patch rows / columns
    constexpr int PATCH = PR * PC * 3;
    constexpr int STAGE_LD = COUT + kStagePad;
    __shared__ __attribute__((aligned(16))) float patch[(PATCH + 3) / 4 * 4];
    __shared__ uint4 wl[COUT * 8];
    __shared__ __attribute__((aligned(16))) float stage_all[4 * 32 * STAGE_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kg = lane >> 4;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    const int img = t / tiles_y;
    const int oy0 = ty * 8, ox0 = tx * 32;
    const int iy0 = oy0 * STRIDE - pad_t, ix0 = ox0 * STRIDE - pad_l;
    const float *ximg = x + (size_t)img * H * W * 3;

    for (int e = tid; e < PATCH; e += 256) {                             // patch rows are contiguous in the image
        const int pr = e / (PC * 3), rem = e - pr * (PC * 3);
        const int iy = iy0 + pr, ix = ix0 + rem / 3;
        patch[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? ximg[((size_t)iy * W + ix) * 3 + rem % 3] : 0.0f;
    }
    for (int e = tid; e < COUT * 8; e += 256) {
        const int n = e >> 3, pc = e & 7;
        reinterpret_cast<u32x4 *>(wl)[n * 8 + (pc ^ ((n >> 1) & 7))] = reinterpret_cast<const u32x4 *>(w)[e];
    }
    // k = 8 kg + j = (r * 3 + s) * 3 + c  ->  offset inside the patch relative to the pixel's top-left input
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * kg + j;
        koff[j] = k < 27 ? (k / 9) * (PC * 3) + (k % 9) : -1;
    }
    __syncthreads();

    u32x4 bhi[NTILES], blo[NTILES];
#pragma unroll
    for (int j = 0; j < NTILES; ++j) {
        const int n = j * 16 + lr;
        const int idx = n * 8 + (kg ^ ((n >> 1) & 7));
        bhi[j] = reinterpret_cast<const u32x4 *>(wl)[idx];
        blo[j] = reinterpret_cast<const u32x4 *>(wl)[idx ^ 4];
    }
    f32x4 acc[4][NTILES];                                                // [row i * 2 + half][N tile]
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int prow = (2 * wave + (m >> 1)) * STRIDE, pcol = (16 * (m & 1) + lr) * STRIDE;
        const int base = (prow * PC + pcol) * 3;
        float xs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[j] = koff[j] >= 0 ? patch[base + koff[j]] : 0.0f;
        const u32x4 ahi = __builtin_bit_cast(u32x4, split_piece<F16>(xs, false));
        const u32x4 alo = __builtin_bit_cast(u32x4, split_piece<F16>(xs, true));
#pragma unroll
        for (int j = 0; j < NTILES; ++j) {
            f32x4 c = f32x4{0.f, 0.f, 0.f, 0.f};
            c = mfma16<F16>(alo, bhi[j], c);
            c = mfma16<F16>(ahi, blo[j], c);
            acc[m][j] = mfma16<F16>(ahi, bhi[j], c);
        }
    }

    float *stage = stage_all + wave * (32 * STAGE_LD);
    float bias_v[NTILES];
#pragma unroll
    for (int j = 0; j < NTILES; ++j) bias_v[j] = bias ? bias[j * 16 + lr] : 0.0f;
    const float act_lo = act == ACT_LINEAR ? -INFINITY : 0.0f;
    const float act_hi = act == ACT_RELU6 ? 6.0f : INFINITY;
    constexpr int PPX = COUT / 4;                                        // 16-byte pieces per pixel (both formats)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int j = 0; j < NTILES; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    stage[(16 * hf + 4 * kg + r) * STAGE_LD + j * 16 + lr] =
                        fminf(fmaxf(acc[i * 2 + hf][j][r] * out_scale + bias_v[j], act_lo), act_hi);
        __syncthreads();
        const int oy = oy0 + 2 * wave + i;
        if (oy < OH) {
            for (int e = lane; e < 32 * PPX; e += 64) {
                const int px = e / PPX, q = e - px * PPX;
                const int ox = ox0 + px;
                if (ox >= OW) continue;
                const size_t pix = ((size_t)img * OH + oy) * OW + ox;
                if constexpr (OUT_SPLIT) {
                    const int cl = q >> 2, pc = q & 3;
                    float xs[8];
                    const float *src = &stage[px * STAGE_LD + cl * 16 + (pc >> 1) * 8];
                    const float4 v0 = *reinterpret_cast<const float4 *>(src);
                    const float4 v1 = *reinterpret_cast<const float4 *>(src + 4);
                    xs[0] = v0.x; xs[1] = v0.y; xs[2] = v0.z; xs[3] = v0.w;
                    xs[4] = v1.x; xs[5] = v1.y; xs[6] = v1.z; xs[7] = v1.w;
                    reinterpret_cast<uint4 *>(out)[pix * PPX + q] = split_piece<F16>(xs, (pc & 1) != 0, status);
                } else {
                    reinterpret_cast<float4 *>(out)[pix * PPX + q] =
                        *reinterpret_cast<const float4 *>(&stage[px * STAGE_LD + 4 * q]);
                }
            }
        }
        __syncthreads();
    }
}

// weights of the MFMA first layer: HWIO (3,3,3,Cout) -> [cout_pad][8 pieces] (k = (r*3+s)*3+c, zero for k >= 27)
void pack_weights_cin3_mfma_host(const float *hwio, const float *scale, int Cout, int cout_pad, bool f16, int shift,
                                 unsigned short *dst /* [cout_pad][64] */)
{
    const float mul = ldexpf(1.0f, shift);
    memset(dst, 0, (size_t)cout_pad * 64 * sizeof(unsigned short));
    for (int k = 0; k < 27; ++k)
        for (int n = 0; n < Cout; ++n) {
            float v = hwio[(size_t)k * Cout + n];
            if (scale) v *= scale[n];
            v *= mul;
            unsigned short hi, lo;
            split_halves_host(v, f16, hi, lo);
            unsigned short *rec = dst + (size_t)n * 64;
            rec[(k >> 3) * 8 + (k & 7)] = hi;
            rec[(4 + (k >> 3)) * 8 + (k & 7)] = lo;
        }
}

hipError_t launch_conv_cin3_mfma(const float *x, const void *w, const float *bias, void *out, int B, int H, int W,
                                 int OH, int OW, int Cout, int stride, int pad_t, int pad_l, int act, float out_scale,
                                 int out_fmt, bool f16, hipStream_t s)
{
    if ((Cout != 32 && Cout != 64) || (stride != 1 && stride != 2) || act == ACT_SIGMOID) return hipErrorInvalidValue;
    const int tiles_x = (OW + 31) / 32, tiles_y = (OH + 7) / 8;
    const long long nblocks = (long long)tiles_x * tiles_y * B;
    if (nblocks <= 0 || nblocks > 0x7fffffffll) return hipErrorInvalidValue;
#define RPN_C3M(F16_, SPLIT_, STRIDE_, NT_)                                                                          \
    hipLaunchKernelGGL((conv_cin3_mfma_kernel<F16_, SPLIT_, STRIDE_, NT_>), dim3((unsigned)nblocks), dim3(256), 0, s, x, \
                       (const uint4 *)w, bias, out, B, H, W, OH, OW, pad_t, pad_l, act, out_scale, tiles_x, tiles_y, range_status())
#define RPN_C3M_FMT(F16_, STRIDE_, NT_) \
    { if (out_fmt) RPN_C3M(F16_, true, STRIDE_, NT_); else RPN_C3M(F16_, false, STRIDE_, NT_); }
#define RPN_C3M_ST(F16_, NT_) \
    { if (stride == 1) RPN_C3M_FMT(F16_, 1, NT_) else RPN_C3M_FMT(F16_, 2, NT_) }
    if (f16) { if (Cout == 64) RPN_C3M_ST(true, 4) else RPN_C3M_ST(true, 2) }
    else     { if (Cout == 64) RPN_C3M_ST(false, 4) else RPN_C3M_ST(false, 2) }
#undef RPN_C3M_ST
#undef RPN_C3M_FMT
#undef RPN_C3M
    return hipGetLastError();
}

// ---- first layer: Cin = 3, 3x3, stride 1 or 2 (VGG16 block1_conv1, MobileNetV2 Conv1) -------------
// K = 27 is too short for the matrix cores to pay off (the gather dominates), so this is a direct
// convolution on the vector ALU: one thread = 2 horizontally adjacent output pixels x 16 output
// channels, weights broadcast from LDS (27 x Cout floats), 864 FMAs per thread.  The output is written
// either as float32 NHWC or directly as SPLIT16 records (one 64-byte record per thread and pixel), which
// removes the separate float32 -> SPLIT16 pass in front of the split-precision layers.
// HBM-bound in principle (12 B read + 4*Cout B written per pixel); VALU-bound in practice.
struct __attribute__((packed, aligned(4))) F4u {      // float4 at 4-byte alignment (still one global_load_dwordx4)
    float x, y, z, w;
};

// WCG (Cout <= 64): the channel group is WAVE-uniform (wave w of the block = group w % CG, a lane = a pixel pair), so the 16 weights of
// a tap are a scalar load (s_load_dwordx16 from `w`, scalar-cache hits) and feed the FMAs as SGPR operands, two channels per
// v_pk_fma_f32.  With a lane-dependent group every tap cost four 16-byte LDS reads per lane: 4 KB per wave for 32 FMAs -- the LDS
// pipe, shared by the CU's four SIMDs, was exactly as busy as the vector ALUs, and the layer ran at half its store rate.
template <bool F16, bool OUT_SPLIT, int STRIDE, bool WCG = false>
__global__ void __launch_bounds__(256)
conv_cin3_kernel(const float *__restrict__ x, const float *__restrict__ w /* (27, Cout) */,
                 const float *__restrict__ bias, void *__restrict__ out, int B, int H, int W, int OH, int OW,
                 int Cout, int stride, int pad_t, int pad_l, int act, long long npairs, unsigned *status)
{
    extern __shared__ __attribute__((aligned(16))) float wl[];       // [27][Cout] + bias[Cout], then the stage
    const int CG = Cout >> 4;
    uint4 *stage = reinterpret_cast<uint4 *>(WCG ? wl : wl + 28 * Cout);   // [2 * 256 / CG pixels][4 * CG pieces] (WCG: no weights in LDS)
    if constexpr (!WCG) {
        for (int i = threadIdx.x; i < 27 * Cout; i += 256) wl[i] = w[i];
        for (int i = threadIdx.x; i < Cout; i += 256) wl[27 * Cout + i] = bias ? bias[i] : 0.0f;
        __syncthreads();
    }
    // index math in 32 bits with ONE division per block (the host checks npairs < 2^31): 64-bit div/mod per
    // thread and per stored piece used to double this kernel's VALU instruction count
    const int PW = (OW + 1) >> 1;                                     // pixel pairs per output row
    const int pairs_per_block = 256 / CG;
    const unsigned pair0 = blockIdx.x * (unsigned)pairs_per_block;
    const unsigned row0 = pair0 / (unsigned)PW;                       // flattened (img, oy) row of the block's first pair
    const int x0 = (int)(pair0 - row0 * (unsigned)PW);
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int cg = WCG ? wv % CG : (int)threadIdx.x % CG;
    const int pairl = WCG ? ((int)threadIdx.x & 63) + 64 * (wv / CG) : (int)threadIdx.x / CG;
    const bool live = pair0 + (unsigned)pairl < (unsigned)npairs;
    int px2 = x0 + pairl;
    unsigned rowf = row0;
    while (px2 >= PW) {                                               // at most pairs_per_block / PW + 1 turns
        px2 -= PW;
        ++rowf;
    }
    const int img = (int)(rowf / (unsigned)OH);
    const int oy = (int)(rowf - (unsigned)img * (unsigned)OH);
    const int ox = 2 * px2;
    (void)stride;

    using f2 = __attribute__((ext_vector_type(2))) float;
    f2 acc[2][8];                                                     // channel pairs: one v_pk_fma_f32 = two FMAs (same chains, same bits)
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        if constexpr (WCG) acc[0][n] = bias ? f2{bias[cg * 16 + 2 * n], bias[cg * 16 + 2 * n + 1]} : f2{0.0f, 0.0f};
        else acc[0][n] = f2{wl[27 * Cout + cg * 16 + 2 * n], wl[27 * Cout + cg * 16 + 2 * n + 1]};
        acc[1][n] = acc[0][n];
    }
    if (live) {
        // per filter row: the 2 output pixels read (STRIDE + 3) consecutive input pixels = 12 or 15 contiguous
        // floats; interior threads fetch them as 4 wide loads, border threads element by element with zero fill
        const float *ximg = x + (size_t)img * H * W * 3;
        const int c0 = ox * STRIDE - pad_l;                              // first input column of the window
        // WCG: the three rows' windows are requested together (one memory latency per thread instead of three; the rolled loop's
        // registers are not what limits residency there -- the staging LDS is)
        float win3[WCG ? 3 : 1][16];
        if constexpr (WCG) {
            const int iy0 = oy * STRIDE - pad_t;
            if (iy0 >= 0 && iy0 + 2 < H && c0 >= 0 && c0 * 3 + 16 <= W * 3) {      // ONE decision for the three rows: twelve loads in flight
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const F4u *src = reinterpret_cast<const F4u *>(ximg + ((size_t)(iy0 + r) * W + c0) * 3);
#pragma unroll
                    for (int v4 = 0; v4 < 4; ++v4) {
                        const F4u v = src[v4];
                        win3[r][4 * v4] = v.x; win3[r][4 * v4 + 1] = v.y; win3[r][4 * v4 + 2] = v.z; win3[r][4 * v4 + 3] = v.w;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int iy = iy0 + r;
                    const bool row_ok = iy >= 0 && iy < H;
#pragma unroll
                    for (int j = 0; j < 15; ++j) {
                        const int col = c0 + j / 3;
                        const bool v = row_ok && col >= 0 && col < W && j < 3 * (STRIDE + 3);
                        win3[r][j] = v ? ximg[((size_t)iy * W + col) * 3 + j % 3] : 0.0f;
                    }
                    win3[r][15] = 0.0f;
                }
            }
        }
#pragma unroll(WCG ? 3 : 1)
        for (int r = 0; r < 3; ++r) {                                    // (!WCG) rolled: keeps registers low
            const int iy = oy * STRIDE + r - pad_t;
            const bool row_ok = iy >= 0 && iy < H;
            float win[16];
            if constexpr (WCG) {
#pragma unroll
                for (int j = 0; j < 16; ++j) win[j] = win3[r][j];
            } else if (row_ok && c0 >= 0 && c0 * 3 + 16 <= W * 3) {
                const F4u *src = reinterpret_cast<const F4u *>(ximg + ((size_t)iy * W + c0) * 3);
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const F4u v = src[v4];
                    win[4 * v4] = v.x; win[4 * v4 + 1] = v.y; win[4 * v4 + 2] = v.z; win[4 * v4 + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 15; ++j) {
                    const int col = c0 + j / 3;
                    const bool v = row_ok && col >= 0 && col < W && j < 3 * (STRIDE + 3);
                    win[j] = v ? ximg[((size_t)iy * W + col) * 3 + j % 3] : 0.0f;
                }
                win[15] = 0.0f;
            }
#pragma unroll
            for (int sc = 0; sc < 9; ++sc) {                             // (tap column s, channel c) = (sc / 3, sc % 3)
                const float4 *wk = WCG ? reinterpret_cast<const float4 *>(w + (r * 9 + sc) * Cout + cg * 16)      // (uniform: scalar loads)
                                       : reinterpret_cast<const float4 *>(&wl[(r * 9 + sc) * Cout + cg * 16]);
                const float4 w0 = wk[0], w1 = wk[1], w2 = wk[2], w3 = wk[3];
                const f2 ws[8] = {{w0.x, w0.y}, {w0.z, w0.w}, {w1.x, w1.y}, {w1.z, w1.w},
                                  {w2.x, w2.y}, {w2.z, w2.w}, {w3.x, w3.y}, {w3.z, w3.w}};
                const float in0 = win[sc], in1 = win[sc + 3 * STRIDE];    // pixel p reads column p*STRIDE + s
                const f2 i0 = {in0, in0}, i1 = {in1, in1};
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    acc[0][n] = __builtin_elementwise_fma(i0, ws[n], acc[0][n]);
                    acc[1][n] = __builtin_elementwise_fma(i1, ws[n], acc[1][n]);
                }
            }
        }
    }
    // stage this thread's 2 x 4 pieces, block-local layout [pixel = 2*pairl + p][piece = 4*cg + k]
    // activation as a branch-free clamp (linear / relu / relu6 only; the host rejects sigmoid for this kernel)
    const float act_lo = act == ACT_LINEAR ? -INFINITY : 0.0f;
    const float act_hi = act == ACT_RELU6 ? 6.0f : INFINITY;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float v[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = fminf(fmaxf(acc[p][n >> 1][n & 1], act_lo), act_hi);
        // WCG: a wave's lanes are pixel PAIRS, 2 * ppp pieces = a multiple of 512 bytes apart -- every lane of a store on the same
        // four banks; the piece index inside a pixel is XOR-swizzled by the pair index (undone by the block-linear reader below)
        uint4 *dst = stage + (2 * pairl + p) * (4 * CG);
        const int q0 = 4 * cg, sw = WCG ? (pairl & (4 * CG - 1) & 7) : 0;
        if constexpr (OUT_SPLIT) {
            const float lo8[8] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
            const float hi8[8] = {v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15]};
            dst[(q0 + 0) ^ sw] = split_piece<F16>(lo8, false, status);
            dst[(q0 + 1) ^ sw] = split_piece<F16>(lo8, true);
            dst[(q0 + 2) ^ sw] = split_piece<F16>(hi8, false, status);
            dst[(q0 + 3) ^ sw] = split_piece<F16>(hi8, true);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                dst[(q0 + k) ^ sw] = make_uint4(__float_as_uint(v[4 * k]), __float_as_uint(v[4 * k + 1]),
                                                __float_as_uint(v[4 * k + 2]), __float_as_uint(v[4 * k + 3]));
        }
    }
    __syncthreads();
    // block-linear stores: consecutive lanes write consecutive 16-byte pieces (1 KB per wave instruction);
    // both layouts (SPLIT16 records, float32 NHWC) are 4*CG pieces per pixel in the same order
    const int ppp = 4 * CG;                                           // pieces per pixel
    const int total = 2 * pairs_per_block * ppp;                      // = 2048
    uint4 *gout = reinterpret_cast<uint4 *>(out);
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / ppp, q = e - pl * ppp;
        if (pair0 + (unsigned)(pl >> 1) >= (unsigned)npairs) continue;
        int gx2 = x0 + (pl >> 1);
        unsigned grow = row0;
        while (gx2 >= PW) {
            gx2 -= PW;
            ++grow;
        }
        const int gox = 2 * gx2 + (pl & 1);
        if (gox >= OW) continue;
        gout[((size_t)grow * OW + gox) * ppp + q] = stage[WCG ? pl * ppp + (q ^ ((pl >> 1) & (ppp - 1) & 7)) : e];
    }
}

// ---- first layer of the float32 graphs on the float32 matrix pipe (round 6): Cin = 3, 3x3, stride 1, 'same', Cout = 64 --------
// VGG16 block1_conv1 in the f32 / f32w precisions.  The vector-ALU kernel above needs 432 packed FMAs + a staged store per thread and
// ran at 0.154 ms (batch 8, 500 x 500); a kernel that ONLY writes the layer's 512 MB takes 0.092 ms with 32 waves per CU and 0.12 ms
// with 8 (scripts/micro/store_rate.hip, store_overlap.hip).  This one: 0.139 ms.
// The 27 taps are ONE K = 28 reduction of v_mfma_f32_16x16x4_f32 (twice the vector ALU's FMA rate): the WEIGHTS are the A operand
// (rows = 16 output channels), a 16-pixel run of an output row is the B operand (columns), so that a lane's four accumulators are four
// CONSECUTIVE channels of one pixel -- a 16-byte store, four lanes complete 64 contiguous bytes, no transpose through LDS.  K index
// e = 9 r + 3 s + c (filter row, filter column, input channel) = the (27, Cout) weight order; for a fixed r the nine (s, c) values of a
// pixel are nine CONSECUTIVE floats of input row y + r - 1 starting at 3 (x - 1).  Bias first, then k ascending: the order of the
// vector-ALU kernel's chain.
// A first form read the B operand straight from global memory (one dword per lane and K step) and the weights per wave: 72 narrow
// load instructions per wave, and the texture-address path alone took 0.076 ms of its 0.166.
// So: PERSISTENT workgroups (the 28 + 16 weight / bias registers are loaded once per workgroup, not per tile), a tile = 8 output rows x
// 64 pixels (a wave = rows wv and wv + 4), its 10 x 66-pixel input patch staged through LDS by 8 coalesced dword loads per thread
// (requested one tile ahead, double-buffered: ONE barrier per tile), the B operand read from there (ds_read_b32, conflict-free: lanes
// 12 bytes apart).  The float32 MFMA executes on the vector ALU's lanes, so every other instruction of the tile loop is MFMA time
// as well: the tile's coordinates advance incrementally (two divisions per tile were ~90 scalar instructions), interior tiles
// have their tile offset in the loads' SCALAR offset (no per-lane address arithmetic), ReLU is one integer max.
// Reference op: Conv2D(64, (3, 3), padding="same", activation="relu") = VGG16 block1_conv1 behind /root/reference/rpn.py:26-33.
constexpr int kC3Rows = 8;                          // output rows per tile
constexpr int kC3PatchRow = 200;                    // floats per staged patch row (198 used).  (The B-operand reads are 2-way bank-conflicted by
                                                    // construction -- four K lanes per pixel on a 3-float pixel stride cannot tile 64 banks; rocprofv3: 45 % of
                                                    // this kernel's LDS cycles, which are < 1 % of its time.  A 201-float row changed nothing.)
constexpr int kC3Stage = ((kC3Rows + 2) * 198 + 255) / 256;            // staging loads per thread (8)
constexpr int kC3PatchFloats = (kC3Stage * 256 / 198 + 1) * kC3PatchRow;   // 10 rows + the row that takes the idle threads' writes
struct C3Tile {
    int img, by, bx;
};
template <bool RELU>
__global__ void __launch_bounds__(256, 2)       // (<= 256 registers: the accumulators stay in the VGPR file, no v_accvgpr copies)
conv_cin3_f32_mfma_kernel(const float *__restrict__ x, const float *__restrict__ w /* (27, 64) */, const float *__restrict__ bias,
                          float *__restrict__ out, int H, int W, int tiles_x, int tiles_y, int n_tiles)
{
    __shared__ float patch[2][kC3PatchFloats];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = lane & 15, kq = lane >> 4;
    constexpr unsigned kOob = 0x80000000u;
    float aw[7][4];                                                      // A: W[channel 16 nb + (lane & 15)][k = 4 kk + kq]
#pragma unroll
    for (int kk = 0; kk < 7; ++kk) {
        const int k = 4 * kk + kq;                                       // (k = 27, the padding: row 26 read, zero kept)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const float v = w[(k < 27 ? k : 26) * 64 + nb * 16 + px];
            aw[kk][nb] = k < 27 ? v : 0.0f;
        }
    }
    f32x4 bv[4];                                                         // the lane's channels 16 nb + 4 kq + (0..3)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) bv[nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (bias) {                                                          // (the caller's pointer: 4-byte alignment only)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[nb][i] = bias[nb * 16 + 4 * kq + i];
    }
    int rd[7];                                                           // B: patch[row wv + 4 h + r][3 (16 mb + px) + t] of k = 9 r + t, floats
#pragma unroll
    for (int kk = 0; kk < 7; ++kk) {
        const int e = 4 * kk + kq < 27 ? 4 * kk + kq : 26, r = e / 9, t = e - 9 * r;   // (k = 27: any address, its weight is 0 -- but finite data: row 26's)
        rd[kk] = (wv + r) * kC3PatchRow + 3 * px + t;
    }
    // staging: element i = tid + 256 it of the 10 x 198 patch (row r = i / 198, float j of the row: column x0 - 1 + j / 3)
    int st_lds[kC3Stage];
    unsigned st_off[kC3Stage];                                           // byte offset from the patch's first float; out of range for the idle threads
#pragma unroll
    for (int it = 0; it < kC3Stage; ++it) {
        const int i = tid + 256 * it, r = i / 198, j = i - 198 * r;
        st_lds[it] = r * kC3PatchRow + j;
        st_off[it] = r < kC3Rows + 2 ? (unsigned)((r * W * 3 + j) * 4) : kOob;
    }
    const int tiles_xy = tiles_x * tiles_y;
    // tile t = (img, by, bx); a workgroup's tiles are gridDim.x apart: the step as (d_img, d_by, d_bx), added with carries
    const int g = (int)gridDim.x, d_img = g / tiles_xy, d_by = (g - d_img * tiles_xy) / tiles_x, d_bx = g - d_img * tiles_xy - d_by * tiles_x;
    auto advance = [&](C3Tile t) {
        t.bx += d_bx;
        if (t.bx >= tiles_x) {
            t.bx -= tiles_x;
            ++t.by;
        }
        t.by += d_by;
        if (t.by >= tiles_y) {
            t.by -= tiles_y;
            ++t.img;
        }
        t.img += d_img;
        return t;
    };
    float pre[kC3Stage];
    auto request = [&](C3Tile t) {                                       // the tile's patch -> registers (zero outside the image)
        const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x) + (size_t)t.img * H * W * 3, (short)0,
                                                                               H * W * 12, 0x00020000);
        if (t.by >= 1 && t.by * kC3Rows + kC3Rows + 1 <= H && t.bx >= 1 && t.bx * 192 + 195 <= 3 * W) {   // (uniform) all inside the image:
            const int tbase = (((t.by * kC3Rows - 1) * W * 3) + t.bx * 192 - 3) * 4;   // no vector ALU work -- the tile in the SCALAR offset
#pragma unroll
            for (int it = 0; it < kC3Stage; ++it)
                pre[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(in_rs, st_off[it], tbase, 0));
        } else {
#pragma unroll
            for (int it = 0; it < kC3Stage; ++it) {
                const int i = tid + 256 * it, r = i / 198, j = i - 198 * r;
                const int iy = t.by * kC3Rows - 1 + r, fx = t.bx * 192 - 3 + j;
                const bool ok = r < kC3Rows + 2 && iy >= 0 && iy < H && fx >= 0 && fx < 3 * W;
                pre[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(in_rs, ok ? (unsigned)((iy * W * 3 + fx) * 4) : kOob, 0, 0));
            }
        }
    };
    auto deposit = [&](int buf) {
#pragma unroll
        for (int it = 0; it < kC3Stage; ++it) patch[buf][st_lds[it]] = pre[it];
    };
    const unsigned st_out = (unsigned)((px * 64 + 4 * kq) * 4);          // the lane's bytes from the tile row's first output
    int tile = blockIdx.x, buf = 0;
    C3Tile cur;
    cur.img = tile / tiles_xy;
    cur.by = (tile - cur.img * tiles_xy) / tiles_x;
    cur.bx = tile - cur.img * tiles_xy - cur.by * tiles_x;
    if (tile < n_tiles) {
        request(cur);
        deposit(0);
    }
    __syncthreads();
    // The loop body is STRAIGHT-LINE (a row past the image's end computes on zeros and stores out of range; the last tile requests an
    // out-of-range patch): the vector-memory counter is in order, so "the next patch has arrived" is `s_waitcnt vmcnt(32)` -- the 32
    // stores issued behind the request may still be in flight -- and hipcc can only count that far when no branch lies between.  With the
    // stores in a branch the wait became vmcnt(4): every tile waited for its own stores' acknowledgements.
    for (; tile < n_tiles; tile += g, buf ^= 1) {
        const bool more = tile + g < n_tiles;
        C3Tile nxt = advance(cur);
        if (!more) nxt.by = -0x100000;                                   // (every row out of the image: eight loads that fetch nothing)
        const int x0 = cur.bx * 64;
        const bool whole = x0 + 64 <= W;
        const __amdgpu_buffer_rsrc_t out_rs = __builtin_amdgcn_make_buffer_rsrc(out + (size_t)cur.img * H * W * 64, (short)0, H * W * 256,
                                                                                0x00020000);
        float pin[4][7];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int kk = 0; kk < 7; ++kk) pin[mb][kk] = patch[buf][rd[kk] + mb * 48];
        request(nxt);                                                    // (in flight across the tile's MFMAs)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int y = cur.by * kC3Rows + wv + 4 * h;
            const bool row = y < H;                                      // (uniform)
            const int tb = (y * W + x0) * 256;                           // (scalar) the tile row's first output, bytes into the image
            if (h == 1) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int kk = 0; kk < 7; ++kk) pin[mb][kk] = patch[buf][4 * kC3PatchRow + rd[kk] + mb * 48];
            }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                f32x4 acc[4];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) acc[nb] = bv[nb];
#pragma unroll
                for (int kk = 0; kk < 7; ++kk)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[kk][nb], pin[mb][kk], acc[nb], 0, 0, 0);
                if constexpr (RELU) {
                    // max(x, 0) on the BITS (v_max_i32: one instruction; fmaxf is a canonicalising v_max v, v, v + the max).  Negative floats
                    // are negative integers -> +0; -0.0 -> +0; a NaN with the sign bit clear stays a NaN (as in the reference's ReLU), with
                    // it set -> 0.
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float f = acc[nb][i];                  // (a VALUE: __builtin_bit_cast of the vector-element lvalue read element 0 four times)
                            acc[nb][i] = __int_as_float(__builtin_elementwise_max(__float_as_int(f), 0));
                        }
                }
                // The tile offset goes into the VECTOR offset (one v_add per 16 pixels), the scalar offset is the constant 0.  Behind a
                // 16-byte store whose scalar offset is a REGISTER hipcc leaves NO wait state before a vector instruction that overwrites the
                // store's data registers (its hazard table knows the hazard for a constant offset only), and gfx950 needs one:
                // `buffer_store_dwordx4 v[18:21], v26, s[12:15], s54 offen` + `v_add_u32 v18, 0x1000, v120` stored the LDS address in
                // element 0 of lanes 12-15 of every 16, differently from run to run (scripts/micro/store_hazard.hip measures it: 0.5 % of
                // the stores with no wait state, none with one; dword stores are not affected).  scripts/isa_store_hazard.py scans the
                // library's assembly for the pattern.
                const unsigned vo = (row && (whole || x0 + 16 * mb + px < W)) ? st_out + (unsigned)(tb + mb * 4096) : kOob;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[nb]), out_rs, vo + (unsigned)(nb * 64), 0, 0);
            }
        }
        deposit(buf ^ 1);                                                // (the other buffer: every wave left it at the last barrier)
        cur = nxt;
        __syncthreads();
    }
}

bool conv_cin3_uses_f32_mfma(int B, int H, int W, int OH, int OW, int Cout, int stride, int pad_t, int pad_l, int act, int out_fmt)
{
    // (laboratory knob 0 = the vector-ALU kernel; same contract)
    static const int f32_mfma = RPN_LAB_KNOB("RPN_CIN3_F32_MFMA", 1);
    return f32_mfma && out_fmt == 0 && Cout == 64 && stride == 1 && pad_t == 1 && pad_l == 1 && OH == H && OW == W &&
           (act == ACT_RELU || act == ACT_LINEAR) && (long long)H * W * 256 < 0x7fffffffll && B > 0 && H > 0 && W > 0 &&
           (long long)((W + 63) / 64) * ((H + 7) / 8) * B < 0x7fffffffll;            // (the tile count: 32-bit in the kernel)
}

// w: (27, Cout) float32 = HWIO flattened (BatchNorm scale already folded); out_fmt: 0 float32 NHWC, 1 SPLIT16
hipError_t launch_conv_cin3(const float *x, const float *w, const float *bias, void *out, int B, int H, int W,
                            int OH, int OW, int Cout, int stride, int pad_t, int pad_l, int act, int out_fmt, bool f16,
                            hipStream_t s)
{
    if (Cout % 16 != 0 || Cout > 256 || 256 % (Cout / 16) != 0 || act == ACT_SIGMOID) return hipErrorInvalidValue;
    if (conv_cin3_uses_f32_mfma(B, H, W, OH, OW, Cout, stride, pad_t, pad_l, act, out_fmt)) {
        const int tiles_x = (W + 63) / 64, tiles_y = (H + kC3Rows - 1) / kC3Rows;
        const long long n_tiles = (long long)tiles_x * tiles_y * B;
        if (n_tiles >= 0x7fffffffll) return hipErrorInvalidValue;
        int dev = 0, n_cus = 0;                                          // persistent: 3 workgroups per CU (<= 168 registers) of the CURRENT device
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n_cus < 1)
            n_cus = 256;
        const dim3 grid((unsigned)(n_tiles < 3ll * n_cus ? n_tiles : 3ll * n_cus));
        if (act == ACT_RELU)
            hipLaunchKernelGGL(conv_cin3_f32_mfma_kernel<true>, grid, dim3(256), 0, s, x, w, bias, static_cast<float *>(out), H, W,
                               tiles_x, tiles_y, (int)n_tiles);
        else
            hipLaunchKernelGGL(conv_cin3_f32_mfma_kernel<false>, grid, dim3(256), 0, s, x, w, bias, static_cast<float *>(out), H, W,
                               tiles_x, tiles_y, (int)n_tiles);
        return hipGetLastError();
    }
    const long long npairs = (long long)B * OH * ((OW + 1) / 2);
    const long long threads = npairs * (Cout / 16);
    if (threads <= 0) return hipSuccess;
    if (npairs >= 0x7fffffffll || threads / 256 >= 0x7fffffffll) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    const bool wcg = Cout <= 64 && 4 % (Cout / 16) == 0;            // 1, 2 or 4 channel groups: one per wave (conv_cin3_kernel)
    const size_t lds = (wcg ? 0 : (size_t)28 * Cout * sizeof(float)) + (size_t)2048 * 16;   // (weights + bias) + staged records
#define RPN_CIN3(F16_, SPLIT_, STRIDE_)                                                                       \
    do {                                                                                                      \
        if (wcg)                                                                                              \
            hipLaunchKernelGGL((conv_cin3_kernel<F16_, SPLIT_, STRIDE_, true>), dim3(grid), dim3(256), lds, s, x, w, bias, out, B, \
                               H, W, OH, OW, Cout, stride, pad_t, pad_l, act, npairs, range_status());         \
        else                                                                                                  \
            hipLaunchKernelGGL((conv_cin3_kernel<F16_, SPLIT_, STRIDE_, false>), dim3(grid), dim3(256), lds, s, x, w, bias, out, B, \
                               H, W, OH, OW, Cout, stride, pad_t, pad_l, act, npairs, range_status());         \
    } while (0)
    if (stride != 1 && stride != 2) return hipErrorInvalidValue;
    if (out_fmt == 0) {
        if (stride == 1) RPN_CIN3(false, false, 1); else RPN_CIN3(false, false, 2);
    } else if (f16) {
        if (stride == 1) RPN_CIN3(true, true, 1); else RPN_CIN3(true, true, 2);
    } else {
        if (stride == 1) RPN_CIN3(false, true, 1); else RPN_CIN3(false, true, 2);
    }
#undef RPN_CIN3
    return hipGetLastError();
}

}  // namespace rpn
