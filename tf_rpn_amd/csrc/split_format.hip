// split_format.hip -- the SPLIT16 format outside the convolutions (conv_split_kernels.hip describes the format): the kernels
// that convert float32 NHWC to and from it and max-pool it, the float16 range-status word, and the host's weight packers.
#include "split_conv.h"

namespace rpn {

// ---- float32 NHWC <-> SPLIT16 ---------------------------------------------------------------
template <bool F16>
__global__ void __launch_bounds__(256)
f32_to_split_kernel(const float *__restrict__ x, long long npieces, uint4 *__restrict__ out, unsigned *status)
{
    // piece p: pixel-major; 4 pieces per 16 channels; piece (g*2 + lo) covers channels 8g..8g+7
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npieces; p += (long long)gridDim.x * 256) {
        const long long rec = p >> 2;                 // (pixel, chunk) record
        const int pc = (int)(p & 3);
        const float *src = x + rec * 16 + (pc >> 1) * 8;
        const float4 v0 = *reinterpret_cast<const float4 *>(src);
        const float4 v1 = *reinterpret_cast<const float4 *>(src + 4);
        const float xs[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        out[p] = split_piece<F16>(xs, (pc & 1) != 0, status);
    }
}

template <bool F16>
__global__ void __launch_bounds__(256)
split_to_f32_kernel(const uint4 *__restrict__ x, long long nhalf, float *__restrict__ out)
{
    // one thread per 8 channels: pieces (2g, 2g+1) -> 8 floats
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < nhalf; p += (long long)gridDim.x * 256) {
        const uint4 hi = x[2 * p], lo = x[2 * p + 1];
        const unsigned h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
        float o[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = join<F16>((unsigned short)(h[k] & 0xffffu), (unsigned short)(l[k] & 0xffffu));
            o[2 * k + 1] = join<F16>((unsigned short)(h[k] >> 16), (unsigned short)(l[k] >> 16));
        }
        float4 *dst = reinterpret_cast<float4 *>(out + p * 8);
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
}

// MaxPooling2D(2,2) 'valid' on SPLIT16: compare hi+lo, keep the winner's (hi, lo) pair
template <bool F16>
__global__ void __launch_bounds__(256)
maxpool_split_kernel(const uint4 *__restrict__ x, int H, int W, int G, int OH, int OW, long long total,
                     uint4 *__restrict__ out)
{
    // G = C/8 groups of 8 channels per pixel; thread = one (pixel, group): reads pieces (2g, 2g+1)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int g = (int)(i % G);
        long long t = i / G;
        const int ox = (int)(t % OW);
        t /= OW;
        const int oy = (int)(t % OH);
        const long long b = t / OH;
        unsigned bh[4] = {0, 0, 0, 0}, bl[4] = {0, 0, 0, 0};
        float best[8];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const size_t pix = ((size_t)b * H + 2 * oy + dy) * W + 2 * ox + dx;
                const uint4 hi = x[(pix * G + g) * 2], lo = x[(pix * G + g) * 2 + 1];
                const unsigned h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned short hs = (unsigned short)((k & 1) ? (h[k >> 1] >> 16) : (h[k >> 1] & 0xffffu));
                    const unsigned short ls = (unsigned short)((k & 1) ? (l[k >> 1] >> 16) : (l[k >> 1] & 0xffffu));
                    const float v = join<F16>(hs, ls);
                    if ((dy == 0 && dx == 0) || v > best[k]) {
                        best[k] = v;
                        const unsigned sh = (k & 1) ? 16u : 0u;
                        const unsigned m = 0xffffu << sh;
                        bh[k >> 1] = (bh[k >> 1] & ~m) | ((unsigned)hs << sh);
                        bl[k >> 1] = (bl[k >> 1] & ~m) | ((unsigned)ls << sh);
                    }
                }
            }
        const size_t opix = ((size_t)b * OH + oy) * OW + ox;
        out[(opix * G + g) * 2] = make_uint4(bh[0], bh[1], bh[2], bh[3]);
        out[(opix * G + g) * 2 + 1] = make_uint4(bl[0], bl[1], bl[2], bl[3]);
    }
}

// ---- host side -------------------------------------------------------------------------------
// Device word that the kernels launched from this thread flag float16 range violations into (rpn_model_forward sets
// it to the model's status word around its launches; null = no reporting).
static thread_local unsigned *t_range_status = nullptr;
void set_range_status(unsigned *p) { t_range_status = p; }
unsigned *range_status() { return t_range_status; }

static inline unsigned short f32_to_bf16_rne(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static inline float bf16_to_f32(unsigned short h)
{
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

void split_halves_host(float v, bool f16, unsigned short &hi, unsigned short &lo)
{
    if (f16) {
        const _Float16 h = (_Float16)v;
        const _Float16 l = (_Float16)(v - (float)h);
        memcpy(&hi, &h, 2);
        memcpy(&lo, &l, 2);
    } else {
        hi = f32_to_bf16_rne(v);
        lo = f32_to_bf16_rne(v - bf16_to_f32(hi));
    }
}

int split_weight_shift(const float *hwio, size_t count, bool f16)
{
    if (!f16) return 0;
    float mx = 0.0f;
    for (size_t i = 0; i < count; ++i) {
        const float v = hwio[i] < 0 ? -hwio[i] : hwio[i];
        if (v > mx) mx = v;
    }
    if (!(mx > 0.0f)) return 0;
    int e = 0;
    (void)frexpf(mx, &e);                       // mx = m * 2^e, m in [0.5, 1)
    int s = 12 - e;                             // largest weight lands in [2^11, 2^12): far from fp16 overflow
    if (s < -100) s = -100;                     // negative: weights beyond the float16 range are scaled DOWN (their hi
    if (s > 24) s = 24;                         // halves would be inf), the epilogue's 2^-s restores the magnitude
    return s;
}

// HWIO (3,3,Cin,Cout) float32 (multiplied by `scale[n]` if given, and by 2^shift) -> [Cin/K][9][cout_pad][2 K halves]: one record
// per K-channel slice, tap and output channel, of 8-channel pieces.  K = 16 (32x32x16 kernels; the SPLIT16 activation record):
// pieces hi k0-7, lo k0-7, hi k8-15, lo k8-15.  K = 32 ("split32", 16x16x32 kernels): pieces hi k0-7 .. hi k24-31, lo k0-7 .. --
// stored as the kernels' LDS image, piece p of channel n at p ^ ((n >> 1) & 7).
static void pack_weights_split_records(const float *hwio, const float *scale, int Cin, int Cout, int cout_pad, bool f16,
                                       int shift, int K, unsigned short *dst)
{
    const int chunks = Cin / K, rec_len = 2 * K;
    const float mul = ldexpf(1.0f, shift);
    memset(dst, 0, (size_t)9 * chunks * cout_pad * rec_len * sizeof(unsigned short));
    for (int t = 0; t < 9; ++t)
        for (int c = 0; c < Cin; ++c)
            for (int n = 0; n < Cout; ++n) {
                float v = hwio[((size_t)t * Cin + c) * Cout + n];
                if (scale) v *= scale[n];
                v *= mul;
                unsigned short hi, lo;
                split_halves_host(v, f16, hi, lo);
                const int chunk = c / K, g = (c % K) >> 3, k = c & 7;
                unsigned short *rec = dst + (((size_t)chunk * 9 + t) * cout_pad + n) * rec_len;
                const int hi_piece = K == 16 ? 2 * g : g, lo_piece = K == 16 ? 2 * g + 1 : 4 + g;
                const int swz = K == 16 ? 0 : (n >> 1) & 7;
                rec[(hi_piece ^ swz) * 8 + k] = hi;
                rec[(lo_piece ^ swz) * 8 + k] = lo;
            }
}

void pack_weights_split_host(const float *hwio, const float *scale, int Cin, int Cout, int cout_pad, bool f16,
                             int shift, unsigned short *dst /* [Cin/16][9][cout_pad][32] */)
{
    pack_weights_split_records(hwio, scale, Cin, Cout, cout_pad, f16, shift, 16, dst);
}

// "split32" packing for the 16x16x32-MFMA kernel: [Cin/32][9][cout_pad][8 pieces = hi k0-7, hi k8-15, hi k16-23,
// hi k24-31, lo k0-7, ...] (128 bytes per output channel, tap and 32-channel slice)
void pack_weights_split32_host(const float *hwio, const float *scale, int Cin, int Cout, int cout_pad, bool f16,
                               int shift, unsigned short *dst /* [Cin/32][9][cout_pad][64] */)
{
    pack_weights_split_records(hwio, scale, Cin, Cout, cout_pad, f16, shift, 32, dst);
}

static int grid_cap(long long items)
{
    long long g = (items + 255) / 256;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    return (int)g;
}

hipError_t launch_f32_to_split(const float *x, long long npix, int C, bool f16, void *out, hipStream_t s)
{
    if (C % 16 != 0) return hipErrorInvalidValue;
    const long long pieces = npix * (C / 16) * 4;
    if (pieces == 0) return hipSuccess;
    with_bool(f16, [&](auto F16) { hipLaunchKernelGGL(f32_to_split_kernel<F16()>, dim3(grid_cap(pieces)), dim3(256), 0, s, x, pieces, (uint4 *)out, range_status()); });
    return hipGetLastError();
}

hipError_t launch_split_to_f32(const void *x, long long npix, int C, bool f16, float *out, hipStream_t s)
{
    if (C % 16 != 0) return hipErrorInvalidValue;
    const long long halves = npix * (C / 8);
    if (halves == 0) return hipSuccess;
    with_bool(f16, [&](auto F16) { hipLaunchKernelGGL(split_to_f32_kernel<F16()>, dim3(grid_cap(halves)), dim3(256), 0, s, (const uint4 *)x, halves, out); });
    return hipGetLastError();
}

hipError_t launch_maxpool_split(const void *x, int B, int H, int W, int C, bool f16, void *out, hipStream_t s)
{
    if (C % 16 != 0) return hipErrorInvalidValue;
    const int OH = H / 2, OW = W / 2, G = C / 8;
    const long long total = (long long)B * OH * OW * G;
    if (total == 0) return hipSuccess;
    with_bool(f16, [&](auto F16) { hipLaunchKernelGGL(maxpool_split_kernel<F16()>, dim3(grid_cap(total)), dim3(256), 0, s, (const uint4 *)x, H, W, G, OH, OW, total, (uint4 *)out); });
    return hipGetLastError();
}

}  // namespace rpn
