// split_conv.h -- what the split-precision ("x3 split") kernel files share: the device helpers of the SPLIT16 format and of
// the 16-bit MFMA tiles, the kernels' argument block, and the host's XCD tile grid.  Included by conv_split_kernels.hip,
// conv_split16_kernels.hip, conv_cin3_kernels.hip and split_format.hip only; it is NOT an interface (that is conv_kernels.h).
#pragma once
#include "conv_kernels.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

// The next slice's global loads are issued at the TOP of a barrier interval so that a whole interval of MFMAs hides
// their latency.  Left alone the scheduler sinks them to the end of the interval, right in front of the barrier whose
// far side stores them to LDS (measured in the ISA), exposing the full memory latency every interval: pin them.
#ifndef RPN_PIN
#define RPN_PIN 1
#endif
#if RPN_PIN
#define RPN_PIN_LOADS() __builtin_amdgcn_sched_barrier(0)
#else
#define RPN_PIN_LOADS() ((void)0)
#endif

namespace rpn {

// The epilogue's staging area is private to a wave: lanes exchange data through it, other waves never touch it, and
// a wave's LDS instructions execute in order -- so the exchange needs a wave-level fence, not a workgroup barrier
// (which would make every wave wait for the slowest one twice per output row).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// (workgroups are 64 * NW threads; NW = 4 or 8)
constexpr int TWS = 32;                 // tile width in pixels = one MFMA M-block
constexpr int HW = TWS + 2;             // halo width
constexpr int kStagePad = 4;            // floats of padding per staged row (keeps 16-byte alignment)

template <bool F16> struct Half;
template <> struct Half<false> {
    using vec = bf16x8;
    using elem = __bf16;
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
    }
};
template <> struct Half<true> {
    using vec = f16x8;
    using elem = _Float16;
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    }
};

// 8 floats -> one 16-byte piece: the hi halves, or the lo halves (x - hi)
// `status` (may be null): device word that receives RPN_STATUS_F16_RANGE when an activation does not fit float16
// (|x| > 65504, or non-finite): its hi half would become inf and every later layer silently garbage (ReLU turns the
// resulting NaNs into zeros).  Checked once per piece, by the lane that produces the hi halves; bf16 halves have
// float32's range.
template <bool F16>
__device__ __forceinline__ uint4 split_piece(const float (&x)[8], bool lo, unsigned *status = nullptr)
{
    using E = typename Half<F16>::elem;
    typename Half<F16>::vec v;
    if constexpr (F16) {
        if (status && !lo) {
            const float m = fmaxf(fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3]))),
                                  fmaxf(fmaxf(fabsf(x[4]), fabsf(x[5])), fmaxf(fabsf(x[6]), fabsf(x[7]))));
            float nan_probe = 0.0f;                           // fmaxf drops NaNs: x * 0 accumulates to NaN for any NaN / inf
#pragma unroll
            for (int k = 0; k < 8; ++k) nan_probe = fmaf(x[k], 0.0f, nan_probe);
            if (!(m <= 65504.0f) || nan_probe != 0.0f) atomicOr(status, 1u /* RPN_STATUS_F16_RANGE */);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const E h = (E)x[k];
        v[k] = lo ? (E)(x[k] - (float)h) : h;
    }
    return __builtin_bit_cast(uint4, v);
}

template <bool F16>
__device__ __forceinline__ float join(unsigned short hi, unsigned short lo)
{
    using E = typename Half<F16>::elem;
    return (float)__builtin_bit_cast(E, hi) + (float)__builtin_bit_cast(E, lo);
}

// v_mfma_f32_16x16x32: A row = lane & 15, k = 8 * (lane >> 4) .. + 7; B column = lane & 15, same k; C/D column = lane & 15,
// row = 4 * (lane >> 4) + reg
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <bool F16>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c)
{
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// XOR swizzle of the eight 16-byte pieces of halo pixel hx (16x16x32 kernels): physical slot = logical piece ^ halo_swz(hx).
// A fragment read (ds_read_b128) is served in four groups of sixteen lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
// same + 32 (MI355X_MICROARCH.md, LDS) -- i.e. sixteen consecutive pixels, eight of them with k-group g and eight with g ^ 1, and
// the tap's column shift s3 = 0, 1, 2 moves that window by a pixel.  With hx & 6 the sixteen pieces of every group fall on sixteen
// different 16-byte bank groups for all three shifts and both 16-pixel halves (exhaustive check and search:
// scripts/lds_swizzle_search.py).  (Rounds 1-5 used (hx >> 1) & 7, which is conflict-free for s3 = 0 only: the taps with
// s3 = 1, 2 paid 2-way conflicts on half of their groups -- the 24-31 % SQ_LDS_BANK_CONFLICT share of profiles/r05_f16x3_pmc.txt;
// round 6: 0.0-0.8 %, profiles/r06_f16x3_pmc.txt.)
__device__ __forceinline__ int halo_swz(int hx) { return hx & 6; }

__device__ __forceinline__ int xcd_remap_s(int bid, int nwg)
{
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

struct SplitConvArgs {
    const uint4 *x;       // SPLIT16 input  [B][H][W][Cin/16][4]
    const uint4 *w;       // split weights  [Cin/16][9][cout_pad][4]
    const float *bias;    // (Cout) float32, may be null
    void *out;            // SPLIT16 [B][H][W][Cout/16][4]  or float32 NHWC [B][H][W][Cout]
    int B, H, W, Cin, Cout, cout_pad;
    float out_scale;      // 2^-s when the weights were pre-scaled by 2^s
    int act, out_f32;
    unsigned *sched;      // persistent kernel: 17 zero-initialised counters (per XCD label: tile queue, exits; labels done), or null
    unsigned *status;     // float16 range flag of the owning model (split_piece), or null
    // B1 instantiation only (VGG16 block 1 in one launch: block1_conv1 computed into the halo tile, x unused):
    const float *img;     // float32 NHWC image (B, H, W, 3)
    const uint4 *w1;      // first-layer weights [64][8 pieces] (pack_weights_cin3_mfma_host)
    const float *b1;      // first-layer bias (64)
    float scale1;         // 2^-s of the pre-scaled first-layer weights
    // conv3x3_split16_kernel only: split-K over gridDim.y workgroups per tile.  Workgroup y accumulates the 32-channel
    // slices [y * chunks / gridDim.y, (y + 1) * chunks / gridDim.y) and writes its RAW partial sums (x out_scale; no bias,
    // no activation) as float32 NHWC to slab y of `out` (slab_floats apart); the consumer adds the slabs.
    long long slab_floats;
    // K TREE (rpn_conv, whose consumer -- the RPN head -- can add partial-sum slabs): the 32-channel slices are cut into FOUR
    // fixed leaves at slices k * slices / 4, k = 0 .. 4 (18 slices: 4 5 4 5), each leaf is one accumulation chain, and the layer's
    // value is (l0 + l1) + (l2 + l3) -- whoever adds: one workgroup inside its tile loop (conv3x3_split16_dma_kernel<.., 64,
    // true>, any batch), two workgroups writing l0 + l1 and l2 + l3 as slabs, or four writing one leaf each, the head adding
    // them in that order.  The same bits at every split factor, so the factor may follow the batch size.
    int ktree;
};

// Host side of the kernels' XCD-aware tile order (conv3x3_split_kernel has the why; xcd_remap_s / TileWalk decode it): TH x 32 px
// by BN channel tiles, the 8 XCD labels as an XN x XM grid over (N-tiles, M-tiles), `slots` tiles per label with both tile counts
// rounded up to that grid.  A one-shot launch has 8 * slots workgroups; each launcher keeps its own limit on that number.
struct SplitGrid {
    int tiles_x, tiles_y, n_tiles, XN, XM;
    long long m_tiles, slots;
    bool valid;                          // m_tiles > 0
};
inline SplitGrid split_grid(int B, int H, int W, int Cout, int TH, int BN)
{
    SplitGrid g;
    g.tiles_x = (W + TWS - 1) / TWS; g.tiles_y = (H + TH - 1) / TH; g.n_tiles = (Cout + BN - 1) / BN;
    g.m_tiles = (long long)g.tiles_x * g.tiles_y * B;
    g.XN = g.n_tiles >= 8 ? 8 : (g.n_tiles >= 4 ? 4 : (g.n_tiles >= 2 ? 2 : 1)); g.XM = 8 / g.XN;
    g.slots = (long long)((g.n_tiles + g.XN - 1) / g.XN) * ((g.m_tiles + g.XM - 1) / g.XM);
    g.valid = g.m_tiles > 0;
    return g;
}

// A run-time bool as a template argument: with_bool(f16, [&](auto F16) { hipLaunchKernelGGL((kernel<F16()>), ...); }).
// Only the instantiations that f names are emitted, so a launcher nests one call per bool that really varies.
template <class F>
inline auto with_bool(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// float32 -> the (hi, lo) 16-bit halves of a packed weight, float16 or bfloat16 (split_format.hip)
void split_halves_host(float v, bool f16, unsigned short &hi, unsigned short &lo);

}  // namespace rpn
