// dropout.h -- the counter-based dropout of the detection head (contract in include/rpn_hip.h, "Dropout"): Philox4x32-10 as in
// Random123 / cuRAND, the threshold rule and the device helper that returns the four keep bits of one generator evaluation.  The
// mask of an element is a function of (seed, call number, layer, row, column) alone: no generator state, no mask tensor, the same
// bits for every tile shape, kernel form and precision.  Shared by the two forward GEMM variants (det_head_kernels.hip,
// det_head_x3_kernels.hip) and the stand-alone element-wise kernel behind rpn_dropout_forward.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace rpn {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // the round multipliers
constexpr unsigned kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // the key increments

// what a kernel needs to drop one layer of one call: the key (seed's low and high word), counter words 2 and 3 (layer, call number
// mod 2^32), the threshold and the scale 1 / (1 - rate)
struct DropoutArgs {
    unsigned k0, k1, layer, t, thr;
    float scale;
};

// one round: (c0, c1, c2, c3), (k0, k1) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
__host__ __device__ __forceinline__ void philox_round(unsigned c[4], unsigned k0, unsigned k1)
{
    const unsigned long long p0 = (unsigned long long)kPhiloxM0 * c[0], p1 = (unsigned long long)kPhiloxM1 * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (unsigned)p1, c[3] = (unsigned)p0;
    c[0] = n0, c[2] = n2;
}

// ten rounds, the key bumped between rounds; c is replaced by the four output words
__host__ __device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) k0 += kPhiloxW0, k1 += kPhiloxW1;
        philox_round(c, k0, k1);
    }
}

// bit i: the element of row 4 mq + i, column n is KEPT (its word, output word i of counter (n, mq, layer, t), is >= thr: an unsigned
// compare, a word equal to the threshold is kept)
__device__ __forceinline__ unsigned dropout_keep4(const DropoutArgs &d, unsigned n, unsigned mq)
{
    unsigned c[4] = {n, mq, d.layer, d.t};
    philox4x32_10(c, d.k0, d.k1);
    return (c[0] >= d.thr ? 1u : 0u) | (c[1] >= d.thr ? 2u : 0u) | (c[2] >= d.thr ? 4u : 0u) | (c[3] >= d.thr ? 8u : 0u);
}

// host side: thr = min(llround(rate 2^32), 2^32 - 1) and scale = (float)(1.0 / (1.0 - rate)), both from double; 0 <= rate < 1
inline DropoutArgs make_dropout_args(double rate, unsigned long long seed, unsigned long long calls, int layer)
{
    const long long r = std::llround(rate * 4294967296.0);
    DropoutArgs d;
    d.k0 = (unsigned)(seed & 0xffffffffull), d.k1 = (unsigned)(seed >> 32);
    d.layer = (unsigned)layer, d.t = (unsigned)(calls & 0xffffffffull);
    d.thr = r > 0xffffffffll ? 0xffffffffu : (unsigned)r;
    d.scale = (float)(1.0 / (1.0 - rate));
    return d;
}

}  // namespace rpn
