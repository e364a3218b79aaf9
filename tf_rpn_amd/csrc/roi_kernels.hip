// roi_kernels.hip -- RoI pooling of a feature map under normalised boxes, and its gradient with respect to the feature map.
//
// No reference counterpart: the reference stops at the proposals.  The operator is what TensorFlow Faster R-CNN implementations
// put between the proposals and the detection head, tf.image.crop_and_resize(feature_map, rois, box_indices, pooling_size) with
// method "bilinear" and extrapolation value 0, with box_indices fixed to "RoI r of image b samples image b".
//
// Contract (float32 throughout, every operation rounded on its own: this file is compiled with -ffp-contract=off, like the box
// math, so that the result is bit-identical to a float32 restatement on the host):
//   x (B,H,W,C) NHWC, rois (B,R,4) normalised [y1,x1,y2,x2], out (B,R,ph,pw,C)
//   hs = (y2 - y1) * (H - 1) / (ph - 1);  in_y(i) = y1 * (H - 1) + i * hs            (ph > 1)
//                                         in_y    = 0.5 * (y1 + y2) * (H - 1)        (ph == 1);   the same in x with W, pw
//   a sample with in_y < 0, in_y > H - 1, in_x < 0, in_x > W - 1 or a NaN coordinate is 0 in every channel; otherwise
//   t = floor(in_y), b = ceil(in_y), ly = in_y - t, l = floor(in_x), r = ceil(in_x), lx = in_x - l,
//   top = x[t,l] + (x[t,r] - x[t,l]) * lx, bot likewise on row b, out = top + (bot - top) * ly
//   with `valid` (B,) the rows r >= valid[b] are zeros (NMS pads its output with all-zero boxes, which would all sample pixel (0,0)).
// Edge behaviour that follows from the float32 expression and is part of the contract (TensorFlow computes the same one): a box
// clipped to exactly 1.0 can round in_y of its LAST sample just above H - 1 (y1 * (H - 1) + (ph - 1) * hs is not y2 * (H - 1) in
// float32), and that sample is then 0.  On edge-touching random boxes about 1 % of the samples do this; none does in float64.
//
// Backward: dx = the adjoint of the forward (each sample adds dy times its four corner weights), as a GATHER -- no float atomics,
// so two runs give the same bits, and image b's dx is a function of image b's rois, valid count and dy alone.
//
// RoI Align (roi_align_kernel, roi_align_backward_kernel, below the pooling kernels) is the second operator of this file: every
// output bin is the average of s x s bilinear samples spread over the bin, in pixel-centre coordinates (Detectron2's aligned=True
// form; include/rpn_hip.h states the arithmetic operation by operation).  Same layout, same launch shape, same rules: float32,
// every operation rounded on its own, the backward a gather in (r, i, j) order.
//
// RoI max pooling (roi_max_pool_kernel, roi_max_pool_backward_kernel) is the third: Fast R-CNN's RoIPool, every output bin the
// maximum over a quantised block of feature pixels, with the pixel it came from kept as an argmax for the backward, which is
// again a gather in (r, i, j) order.  include/rpn_hip.h states the quantisation operation by operation.
#include <cmath>
#include <cstdint>

#include "roi_kernels.h"
#include "rpn_common.h"

namespace rpn {

constexpr int kRoiWaves = 4;             // waves per forward workgroup
constexpr int kRoiSamplesPerWave = 4;    // consecutive samples (i, j) of one RoI per wave
constexpr int kRoiSampleTile = kRoiWaves * kRoiSamplesPerWave;   // samples per forward workgroup
constexpr int kRoiChannelTile = 64 * 4;  // channels one wave covers per pass (16 bytes per lane)

// input coordinate of sample k of n along an axis of `size` pixels under the box side [c1, c2]; ok = false when it extrapolates
__device__ __forceinline__ float roi_coord(float c1, float c2, int n, int k, int size, bool *ok)
{
    const float span = (float)(size - 1);
    float in;
    if (n > 1) {
        const float scale = (c2 - c1) * span / (float)(n - 1);
        in = c1 * span + (float)k * scale;
    } else {
        in = 0.5f * (c1 + c2) * span;
    }
    *ok = in >= 0.0f && in <= span;      // (false for NaN)
    return in;
}

// the weight pixel `pos` of that axis has in sample k: (1 - frac) as the floor pixel plus frac as the ceil pixel, 0 when the
// sample does not touch it or extrapolates
__device__ __forceinline__ float roi_axis_weight(float c1, float c2, int n, int k, int size, int pos)
{
    bool ok;
    const float in = roi_coord(c1, c2, n, k, size, &ok);
    if (!ok) return 0.0f;
    const float lo = floorf(in), frac = in - lo;
    float w = 0.0f;
    if ((int)lo == pos) w = 1.0f - frac;
    if ((int)ceilf(in) == pos) w += frac;
    return w;
}

__device__ __forceinline__ float roi_half_to_f32(unsigned short h, bool f16)
{
    return f16 ? (float)__builtin_bit_cast(_Float16, h) : __builtin_bit_cast(float, (unsigned)h << 16);
}

// channels c .. c + 3 (c % 4 == 0) of pixel `pix`
template <int SRC>
__device__ __forceinline__ float4 roi_load4(const void *x, long long pix, int C, int c)
{
    if constexpr (SRC == ROI_SRC_F32) {
        return *reinterpret_cast<const float4 *>(static_cast<const float *>(x) + pix * C + c);
    } else {
        // SPLIT16: per pixel and 8 channels one 16-byte piece of hi halves, then one of lo halves; value = hi + lo (join<>)
        constexpr bool F16 = SRC == ROI_SRC_SPLIT_F16;
        const char *p = static_cast<const char *>(x) + ((pix * (C >> 3) + (c >> 3)) * 32 + (c & 4) * 2);
        const uint2 hi = *reinterpret_cast<const uint2 *>(p), lo = *reinterpret_cast<const uint2 *>(p + 16);
        float4 v;
        v.x = roi_half_to_f32((unsigned short)(hi.x & 0xffffu), F16) + roi_half_to_f32((unsigned short)(lo.x & 0xffffu), F16);
        v.y = roi_half_to_f32((unsigned short)(hi.x >> 16), F16) + roi_half_to_f32((unsigned short)(lo.x >> 16), F16);
        v.z = roi_half_to_f32((unsigned short)(hi.y & 0xffffu), F16) + roi_half_to_f32((unsigned short)(lo.y & 0xffffu), F16);
        v.w = roi_half_to_f32((unsigned short)(hi.y >> 16), F16) + roi_half_to_f32((unsigned short)(lo.y >> 16), F16);
        return v;
    }
}

__device__ __forceinline__ float4 roi_lerp(float4 a, float4 b, float t)
{
    return make_float4(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t, a.w + (b.w - a.w) * t);
}

// Forward.  Store-bound: B R ph pw C floats written, each sample's four corner pixels read (the feature map stays in cache).
// Workgroup (roi, sample tile): blockIdx.x = b R + r, blockIdx.y = tile of kRoiSampleTile samples; a wave owns
// kRoiSamplesPerWave consecutive samples.  Per sample the coordinates, corner addresses and weights are wave-uniform (computed
// once, from scalars); the lanes run over the channels, 16 bytes each, so every store instruction writes 1 KiB of one output row.
template <int SRC>
__global__ void __launch_bounds__(64 * kRoiWaves)
roi_pool_kernel(const void *__restrict__ x, int H, int W, int C, const float *__restrict__ rois, int R, int ph, int pw,
                const int *__restrict__ valid, float *__restrict__ out)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long roi = blockIdx.x;
    const int b = (int)(roi / R), r = (int)(roi - (long long)b * R);
    const int nsamp = ph * pw;
    const bool live = valid == nullptr || r < valid[b];
    const float *box = rois + roi * 4;
    const float y1 = box[0], x1 = box[1], y2 = box[2], x2 = box[3];
#pragma unroll
    for (int k = 0; k < kRoiSamplesPerWave; ++k) {
        const int q = (int)blockIdx.y * kRoiSampleTile + wave * kRoiSamplesPerWave + k;
        if (q >= nsamp) break;
        const int i = q / pw, j = q - i * pw;
        bool oky, okx;
        const float in_y = roi_coord(y1, y2, ph, i, H, &oky), in_x = roi_coord(x1, x2, pw, j, W, &okx);
        const bool ok = live && oky && okx;
        float ly = 0.0f, lx = 0.0f;
        long long tl = 0, tr = 0, bl = 0, br = 0;
        if (ok) {
            const float fy = floorf(in_y), fx = floorf(in_x);
            ly = in_y - fy;
            lx = in_x - fx;
            const long long row_t = ((long long)b * H + (int)fy) * W, row_b = ((long long)b * H + (int)ceilf(in_y)) * W;
            const int cl = (int)fx, cr = (int)ceilf(in_x);
            tl = row_t + cl; tr = row_t + cr; bl = row_b + cl; br = row_b + cr;
        }
        float *o = out + (roi * nsamp + q) * C;
        for (int c = lane * 4; c < C; c += kRoiChannelTile) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) {
                const float4 vtl = roi_load4<SRC>(x, tl, C, c), vtr = roi_load4<SRC>(x, tr, C, c);
                const float4 vbl = roi_load4<SRC>(x, bl, C, c), vbr = roi_load4<SRC>(x, br, C, c);
                v = roi_lerp(roi_lerp(vtl, vtr, lx), roi_lerp(vbl, vbr, lx), ly);
            }
            *reinterpret_cast<float4 *>(o + c) = v;
        }
    }
}

__device__ __forceinline__ float roi_lane_value(float v, int src_lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src_lane));
}

// Backward, as a gather: one wave per (feature-map pixel, tile of kRoiChannelTile channels), lanes over the channels.  The wave
// walks its image's RoIs in index order, 64 at a time: each lane tests ONE RoI (does any sample row touch pixel row y, any sample
// column pixel column x), the ballot lists the RoIs that do; for each of those, in order, the lanes compute the row weights of the
// ph sample rows (one per lane) and the column weights of the pw sample columns, and the non-zero (i, j) pairs are accumulated in
// (r, i, j) order.  Everything that decides WHAT is added is wave-uniform, the order is fixed, and nothing of another image is read.
__global__ void __launch_bounds__(64)
roi_pool_backward_kernel(const float *__restrict__ dy, const float *__restrict__ rois, const int *__restrict__ valid, int H, int W,
                         int C, int R, int ph, int pw, int ctiles, float *__restrict__ dx)
{
    const int lane = threadIdx.x;
    const long long pix = blockIdx.x / (unsigned)ctiles;
    const int ct = (int)(blockIdx.x - (unsigned)pix * (unsigned)ctiles);
    const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
    const int c = ct * kRoiChannelTile + lane * 4;
    const bool active = c < C;
    int nr = R;
    if (valid) nr = min(max(valid[b], 0), R);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int r0 = 0; r0 < nr; r0 += 64) {
        const int r = r0 + lane;
        float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool hit = false;
        if (r < nr) {
            box = *reinterpret_cast<const float4 *>(rois + ((long long)b * R + r) * 4);
            bool hy = false, hx = false;
            for (int i = 0; i < ph; ++i) hy = hy || roi_axis_weight(box.x, box.z, ph, i, H, py) != 0.0f;
            if (hy)
                for (int j = 0; j < pw; ++j) hx = hx || roi_axis_weight(box.y, box.w, pw, j, W, px) != 0.0f;
            hit = hy && hx;
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {
            const int k = __builtin_ctzll(hits);
            hits &= hits - 1;
            const float y1 = roi_lane_value(box.x, k), x1 = roi_lane_value(box.y, k);
            const float y2 = roi_lane_value(box.z, k), x2 = roi_lane_value(box.w, k);
            const long long roi = (long long)b * R + (r0 + k);
            for (int i0 = 0; i0 < ph; i0 += 64) {
                const float wy = i0 + lane < ph ? roi_axis_weight(y1, y2, ph, i0 + lane, H, py) : 0.0f;
                unsigned long long rows = __ballot(wy != 0.0f);
                while (rows) {
                    const int li = __builtin_ctzll(rows);
                    rows &= rows - 1;
                    const float wyi = roi_lane_value(wy, li);
                    const long long row = (roi * ph + (i0 + li)) * pw;
                    for (int j0 = 0; j0 < pw; j0 += 64) {
                        const float wx = j0 + lane < pw ? roi_axis_weight(x1, x2, pw, j0 + lane, W, px) : 0.0f;
                        unsigned long long cols = __ballot(wx != 0.0f);
                        while (cols) {
                            const int lj = __builtin_ctzll(cols);
                            cols &= cols - 1;
                            const float w = wyi * roi_lane_value(wx, lj);
                            if (active) {
                                const float4 g = *reinterpret_cast<const float4 *>(dy + (row + (j0 + lj)) * C + c);
                                acc.x += g.x * w; acc.y += g.y * w; acc.z += g.z * w; acc.w += g.w * w;
                            }
                        }
                    }
                }
            }
        }
    }
    if (active) *reinterpret_cast<float4 *>(dx + pix * C + c) = acc;
}

// ---- RoI Align ------------------------------------------------------------------------------------------------------------------
// one axis of a box in feature pixels: first bin's start, bin size, distance between two samples of a bin
struct RoiAlignAxis {
    float start, bin, step;
};

__device__ __forceinline__ RoiAlignAxis roi_align_axis(float c1, float c2, float extent, int n, int s)
{
    const float start = c1 * extent - 0.5f, end = c2 * extent - 0.5f;
    const float bin = (end - start) / (float)n;
    return {start, bin, bin / (float)s};
}

// coordinate of sample k of bin i
__device__ __forceinline__ float roi_align_coord(const RoiAlignAxis &a, int i, int k)
{
    return (a.start + (float)i * a.bin) + ((float)k + 0.5f) * a.step;
}

// the two pixels a sample at `y` reads along an axis of `size` pixels and the weight `l` of the second (the first has 1 - l);
// false when the sample is further than one pixel outside (or NaN): it then contributes nothing
__device__ __forceinline__ bool roi_align_corners(float y, int size, int *lo, int *hi, float *l)
{
    *lo = *hi = 0;
    *l = 0.0f;
    if (!(y >= -1.0f && y <= (float)size)) return false;
    if (y < 0.0f) y = 0.0f;
    int p = (int)y;
    if (p >= size - 1) {
        p = size - 1;
        *hi = p;
        y = (float)p;
    } else {
        *hi = p + 1;
    }
    *lo = p;
    *l = y - (float)p;
    return true;
}

// A(i, pos): the weight pixel `pos` of that axis has in bin i, summed over the bin's s samples in order
__device__ __forceinline__ float roi_align_axis_weight(const RoiAlignAxis &a, int i, int s, int size, int pos)
{
    float sum = 0.0f;
    for (int k = 0; k < s; ++k) {
        int lo, hi;
        float l;
        if (!roi_align_corners(roi_align_coord(a, i, k), size, &lo, &hi, &l)) continue;
        float w = 0.0f;
        if (lo == pos) w = 1.0f - l;
        if (hi == pos) w += l;
        sum += w;
    }
    return sum;
}

constexpr int kRoiAlignMaxSamples = 4;   // sampling_ratio <= 4: the sample columns of a bin are kept in registers

// Forward.  The launch shape of roi_pool_kernel: workgroup (roi, tile of kRoiSampleTile bins), a wave owns kRoiSamplesPerWave
// consecutive bins, the lanes run over the channels, 16 bytes each, one float4 store per output.  The s x s samples of a bin are
// accumulated in registers; a bin's s sample columns (pixels and weights) are computed once per bin, its sample rows once per
// channel pass; all of that is wave-uniform.  4 s^2 corner loads per store.
template <int SRC>
__global__ void __launch_bounds__(64 * kRoiWaves)
roi_align_kernel(const void *__restrict__ x, int H, int W, int C, const float *__restrict__ rois, int R, int ph, int pw, int s,
                 float extent_y, float extent_x, const int *__restrict__ valid, float *__restrict__ out)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long roi = blockIdx.x;
    const int b = (int)(roi / R), r = (int)(roi - (long long)b * R);
    const int nbins = ph * pw;
    const bool live = valid == nullptr || r < valid[b];
    const float *box = rois + roi * 4;
    const RoiAlignAxis ay = roi_align_axis(box[0], box[2], extent_y, ph, s), ax = roi_align_axis(box[1], box[3], extent_x, pw, s);
    const float count = (float)(s * s);
#pragma unroll
    for (int k = 0; k < kRoiSamplesPerWave; ++k) {
        const int q = (int)blockIdx.y * kRoiSampleTile + wave * kRoiSamplesPerWave + k;
        if (q >= nbins) break;
        const int i = q / pw, j = q - i * pw;
        int xlo[kRoiAlignMaxSamples], xhi[kRoiAlignMaxSamples];
        float lx[kRoiAlignMaxSamples];
        bool okx[kRoiAlignMaxSamples];
#pragma unroll
        for (int kx = 0; kx < kRoiAlignMaxSamples; ++kx)
            okx[kx] = roi_align_corners(roi_align_coord(ax, j, kx), W, &xlo[kx], &xhi[kx], &lx[kx]) && kx < s && live;
        float *o = out + (roi * nbins + q) * C;
        for (int c = lane * 4; c < C; c += kRoiChannelTile) {
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int ky = 0; ky < s; ++ky) {
                int ylo, yhi;
                float ly;
                if (!roi_align_corners(roi_align_coord(ay, i, ky), H, &ylo, &yhi, &ly)) continue;
                const float hy = 1.0f - ly;
                const long long row_lo = ((long long)b * H + ylo) * W, row_hi = ((long long)b * H + yhi) * W;
#pragma unroll
                for (int kx = 0; kx < kRoiAlignMaxSamples; ++kx) {
                    if (!okx[kx]) continue;
                    const float hx = 1.0f - lx[kx];
                    const float w1 = hy * hx, w2 = hy * lx[kx], w3 = ly * hx, w4 = ly * lx[kx];
                    const float4 v1 = roi_load4<SRC>(x, row_lo + xlo[kx], C, c), v2 = roi_load4<SRC>(x, row_lo + xhi[kx], C, c);
                    const float4 v3 = roi_load4<SRC>(x, row_hi + xlo[kx], C, c), v4 = roi_load4<SRC>(x, row_hi + xhi[kx], C, c);
                    acc.x += ((w1 * v1.x + w2 * v2.x) + w3 * v3.x) + w4 * v4.x;
                    acc.y += ((w1 * v1.y + w2 * v2.y) + w3 * v3.y) + w4 * v4.y;
                    acc.z += ((w1 * v1.z + w2 * v2.z) + w3 * v3.z) + w4 * v4.z;
                    acc.w += ((w1 * v1.w + w2 * v2.w) + w3 * v3.w) + w4 * v4.w;
                }
            }
            *reinterpret_cast<float4 *>(o + c) = make_float4(acc.x / count, acc.y / count, acc.z / count, acc.w / count);
        }
    }
}

// Backward, the gather of roi_pool_backward_kernel with separable bin weights: one wave per (feature-map pixel, tile of
// kRoiChannelTile channels).  The wave walks its image's RoIs in index order, 64 at a time: each lane tests ONE RoI (has any bin
// row a weight on pixel row y, any bin column on pixel column x), the ballot lists the RoIs that do; for each of those, in order,
// the lanes compute Ay(i, py) of the ph bin rows (one per lane) and Ax(j, px) of the pw bin columns, and the non-zero (i, j) pairs
// are accumulated in (r, i, j) order: acc += dy * (Ay * Ax); dx = acc / (s * s).
__global__ void __launch_bounds__(64)
roi_align_backward_kernel(const float *__restrict__ dy, const float *__restrict__ rois, const int *__restrict__ valid, int H, int W,
                          int C, int R, int ph, int pw, int s, float extent_y, float extent_x, int ctiles, float *__restrict__ dx)
{
    const int lane = threadIdx.x;
    const long long pix = blockIdx.x / (unsigned)ctiles;
    const int ct = (int)(blockIdx.x - (unsigned)pix * (unsigned)ctiles);
    const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
    const int c = ct * kRoiChannelTile + lane * 4;
    const bool active = c < C;
    int nr = R;
    if (valid) nr = min(max(valid[b], 0), R);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int r0 = 0; r0 < nr; r0 += 64) {
        const int r = r0 + lane;
        float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool hit = false;
        if (r < nr) {
            box = *reinterpret_cast<const float4 *>(rois + ((long long)b * R + r) * 4);
            const RoiAlignAxis ay = roi_align_axis(box.x, box.z, extent_y, ph, s), ax = roi_align_axis(box.y, box.w, extent_x, pw, s);
            bool hy = false, hx = false;
            for (int i = 0; i < ph; ++i) hy = hy || roi_align_axis_weight(ay, i, s, H, py) != 0.0f;
            if (hy)
                for (int j = 0; j < pw; ++j) hx = hx || roi_align_axis_weight(ax, j, s, W, px) != 0.0f;
            hit = hy && hx;
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {
            const int k = __builtin_ctzll(hits);
            hits &= hits - 1;
            const RoiAlignAxis ay = roi_align_axis(roi_lane_value(box.x, k), roi_lane_value(box.z, k), extent_y, ph, s);
            const RoiAlignAxis ax = roi_align_axis(roi_lane_value(box.y, k), roi_lane_value(box.w, k), extent_x, pw, s);
            const long long roi = (long long)b * R + (r0 + k);
            for (int i0 = 0; i0 < ph; i0 += 64) {
                const float wy = i0 + lane < ph ? roi_align_axis_weight(ay, i0 + lane, s, H, py) : 0.0f;
                unsigned long long rows = __ballot(wy != 0.0f);
                while (rows) {
                    const int li = __builtin_ctzll(rows);
                    rows &= rows - 1;
                    const float wyi = roi_lane_value(wy, li);
                    const long long row = (roi * ph + (i0 + li)) * pw;
                    for (int j0 = 0; j0 < pw; j0 += 64) {
                        const float wx = j0 + lane < pw ? roi_align_axis_weight(ax, j0 + lane, s, W, px) : 0.0f;
                        unsigned long long cols = __ballot(wx != 0.0f);
                        while (cols) {
                            const int lj = __builtin_ctzll(cols);
                            cols &= cols - 1;
                            const float w = wyi * roi_lane_value(wx, lj);
                            if (active) {
                                const float4 g = *reinterpret_cast<const float4 *>(dy + (row + (j0 + lj)) * C + c);
                                acc.x += g.x * w; acc.y += g.y * w; acc.z += g.z * w; acc.w += g.w * w;
                            }
                        }
                    }
                }
            }
        }
    }
    const float count = (float)(s * s);
    if (active) *reinterpret_cast<float4 *>(dx + pix * C + c) = make_float4(acc.x / count, acc.y / count, acc.z / count, acc.w / count);
}

// ---- RoI max pooling ------------------------------------------------------------------------------------------------------------
// one axis of a box in whole feature pixels: first pixel and bin size (include/rpn_hip.h states the arithmetic)
struct RoiMaxAxis {
    int p1;
    float bin;
};

constexpr float kRoiMaxClamp = 1048576.0f;   // 2^20: the products are clamped here before they are rounded to int

// false when a product is NaN (the RoI is dead)
__device__ __forceinline__ bool roi_max_axis(float c1, float c2, float extent, int n, RoiMaxAxis *a)
{
    float s = c1 * extent, e = c2 * extent;
    const bool ok = s == s && e == e;
    s = fminf(fmaxf(s, -kRoiMaxClamp), kRoiMaxClamp);
    e = fminf(fmaxf(e, -kRoiMaxClamp), kRoiMaxClamp);
    const int p1 = ok ? (int)roundf(s) : 0, p2 = ok ? (int)roundf(e) : 0;
    a->p1 = p1;
    a->bin = (float)max(p2 - p1 + 1, 1) / (float)n;
    return ok;
}

// pixels [*lo, *hi) of bin i along an axis of `size` pixels; empty when *hi <= *lo
__device__ __forceinline__ void roi_max_bin(const RoiMaxAxis &a, int i, int size, int *lo, int *hi)
{
    *lo = min(max((int)floorf((float)i * a.bin) + a.p1, 0), size);
    *hi = min(max((int)ceilf((float)(i + 1) * a.bin) + a.p1, 0), size);
}

__device__ __forceinline__ void roi_max_take(float v, int p, float *m, int *idx)
{
    if (v > *m || v != v) {
        *m = v;
        *idx = p;
    }
}

// Forward.  The launch shape of roi_pool_kernel: workgroup (roi, tile of kRoiSampleTile bins), a wave owns kRoiSamplesPerWave
// consecutive bins, the lanes run over the channels, 16 bytes each: one float4 store of the maximum per pass and, when `argmax`
// is not null, one int4 store of the pixel y W + x it was taken from.  A bin's limits are wave-uniform and computed once per
// bin; its pixels are scanned in (row, column) order, the first maximum wins and a NaN is taken (torch.max_pool2d's rule).
// (he - hs)(we - ws) pixel loads per store: about 20 for a box that covers the 31 x 31 map at 7 x 7.
template <int SRC>
__global__ void __launch_bounds__(64 * kRoiWaves)
roi_max_pool_kernel(const void *__restrict__ x, int H, int W, int C, const float *__restrict__ rois, int R, int ph, int pw,
                    float extent_y, float extent_x, const int *__restrict__ valid, float *__restrict__ out, int *__restrict__ argmax)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long roi = blockIdx.x;
    const int b = (int)(roi / R), r = (int)(roi - (long long)b * R);
    const int nbins = ph * pw;
    const float *box = rois + roi * 4;
    RoiMaxAxis ay, ax;
    const bool oky = roi_max_axis(box[0], box[2], extent_y, ph, &ay), okx = roi_max_axis(box[1], box[3], extent_x, pw, &ax);
    const bool live = (valid == nullptr || r < valid[b]) && oky && okx;
    const long long image = (long long)b * H * W;
#pragma unroll
    for (int k = 0; k < kRoiSamplesPerWave; ++k) {
        const int q = (int)blockIdx.y * kRoiSampleTile + wave * kRoiSamplesPerWave + k;
        if (q >= nbins) break;
        const int i = q / pw, j = q - i * pw;
        int hs, he, ws, we;
        roi_max_bin(ay, i, H, &hs, &he);
        roi_max_bin(ax, j, W, &ws, &we);
        const bool ok = live && he > hs && we > ws;
        const long long o = (roi * nbins + q) * C;
        for (int c = lane * 4; c < C; c += kRoiChannelTile) {
            float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int4 idx = make_int4(-1, -1, -1, -1);
            if (ok) {
                const int first = hs * W + ws;
                m = roi_load4<SRC>(x, image + first, C, c);
                idx = make_int4(first, first, first, first);
                for (int y = hs; y < he; ++y)
                    for (int xx = y == hs ? ws + 1 : ws; xx < we; ++xx) {
                        const int p = y * W + xx;
                        const float4 v = roi_load4<SRC>(x, image + p, C, c);
                        roi_max_take(v.x, p, &m.x, &idx.x);
                        roi_max_take(v.y, p, &m.y, &idx.y);
                        roi_max_take(v.z, p, &m.z, &idx.z);
                        roi_max_take(v.w, p, &m.w, &idx.w);
                    }
            }
            *reinterpret_cast<float4 *>(out + o + c) = m;
            if (argmax) *reinterpret_cast<int4 *>(argmax + o + c) = idx;
        }
    }
}

// Backward, the gather of roi_pool_backward_kernel: one wave per (feature-map pixel, tile of kRoiChannelTile channels).  The wave
// walks its image's RoIs in index order, 64 at a time: each lane tests ONE RoI (live, and the pixel inside the pixels its bins
// cover, [hs(0), he(ph - 1)) x [ws(0), we(pw - 1))), the ballot lists the RoIs that pass; for each of those, in order, the lanes
// test the ph bin rows (one per lane) and the pw bin columns for containing the pixel -- bins overlap, so up to two per axis do
// when bin >= 1 and up to all of them otherwise -- and for each (i, j), in order, the lanes load argmax and dy of their four
// channels and add dy where the argmax is this pixel.  What is added is decided per channel, the order is fixed.
__global__ void __launch_bounds__(64)
roi_max_pool_backward_kernel(const float *__restrict__ dy, const int *__restrict__ argmax, const float *__restrict__ rois,
                             const int *__restrict__ valid, int H, int W, int C, int R, int ph, int pw, float extent_y, float extent_x,
                             int ctiles, float *__restrict__ dx)
{
    const int lane = threadIdx.x;
    const long long pix = blockIdx.x / (unsigned)ctiles;
    const int ct = (int)(blockIdx.x - (unsigned)pix * (unsigned)ctiles);
    const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
    const int p = py * W + px;
    const int c = ct * kRoiChannelTile + lane * 4;
    const bool active = c < C;
    int nr = R;
    if (valid) nr = min(max(valid[b], 0), R);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int r0 = 0; r0 < nr; r0 += 64) {
        const int r = r0 + lane;
        float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool hit = false;
        if (r < nr) {
            box = *reinterpret_cast<const float4 *>(rois + ((long long)b * R + r) * 4);
            RoiMaxAxis ay, ax;
            if (roi_max_axis(box.x, box.z, extent_y, ph, &ay) && roi_max_axis(box.y, box.w, extent_x, pw, &ax)) {
                int lo, hi, unused;
                roi_max_bin(ay, 0, H, &lo, &unused);
                roi_max_bin(ay, ph - 1, H, &unused, &hi);
                hit = py >= lo && py < hi;
                roi_max_bin(ax, 0, W, &lo, &unused);
                roi_max_bin(ax, pw - 1, W, &unused, &hi);
                hit = hit && px >= lo && px < hi;
            }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {
            const int k = __builtin_ctzll(hits);
            hits &= hits - 1;
            RoiMaxAxis ay, ax;
            roi_max_axis(roi_lane_value(box.x, k), roi_lane_value(box.z, k), extent_y, ph, &ay);
            roi_max_axis(roi_lane_value(box.y, k), roi_lane_value(box.w, k), extent_x, pw, &ax);
            const long long roi = (long long)b * R + (r0 + k);
            for (int i0 = 0; i0 < ph; i0 += 64) {
                int lo = 0, hi = 0;
                if (i0 + lane < ph) roi_max_bin(ay, i0 + lane, H, &lo, &hi);
                unsigned long long rows = __ballot(py >= lo && py < hi);
                while (rows) {
                    const int li = __builtin_ctzll(rows);
                    rows &= rows - 1;
                    const long long row = (roi * ph + (i0 + li)) * pw;
                    for (int j0 = 0; j0 < pw; j0 += 64) {
                        lo = hi = 0;
                        if (j0 + lane < pw) roi_max_bin(ax, j0 + lane, W, &lo, &hi);
                        unsigned long long cols = __ballot(px >= lo && px < hi);
                        while (cols) {
                            const int lj = __builtin_ctzll(cols);
                            cols &= cols - 1;
                            if (active) {
                                const long long at = (row + (j0 + lj)) * C + c;
                                const int4 a = *reinterpret_cast<const int4 *>(argmax + at);
                                const float4 g = *reinterpret_cast<const float4 *>(dy + at);
                                if (a.x == p) acc.x += g.x;
                                if (a.y == p) acc.y += g.y;
                                if (a.z == p) acc.z += g.z;
                                if (a.w == p) acc.w += g.w;
                            }
                        }
                    }
                }
            }
        }
    }
    if (active) *reinterpret_cast<float4 *>(dx + pix * C + c) = acc;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the checks every entry shares; B R and B H W ctiles are grid dimensions, ph pw / kRoiSampleTile is one
static int roi_check(const char *who, int B, int H, int W, int C, int R, int ph, int pw)
{
    RPN_REQUIRE(B >= 1 && R >= 1 && ph >= 1 && pw >= 1, "%s: B, R and the pooling size must be >= 1 (got %d, %d, %d x %d)", who, B, R,
                ph, pw);
    RPN_REQUIRE(H >= 1 && W >= 1, "%s: feature map %d x %d", who, H, W);
    RPN_REQUIRE(C >= 4 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", who, C);
    RPN_REQUIRE((long long)B * R < (1ll << 31), "%s: B * R = %lld RoIs do not fit one launch", who, (long long)B * R);
    RPN_REQUIRE((long long)ph * pw <= 65535ll * kRoiSampleTile, "%s: pooling size %d x %d is beyond one launch", who, ph, pw);
    RPN_REQUIRE((long long)B * H * W * ((C + kRoiChannelTile - 1) / kRoiChannelTile) < (1ll << 31),
                "%s: the feature map (%d, %d, %d, %d) is beyond one launch", who, B, H, W, C);
    return RPN_OK;
}

int roi_pool_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                     int pw, const int *d_valid, float *d_out, hipStream_t s)
{
    RPN_REQUIRE(d_x && d_rois && d_out, "%s: null pointer", who);
    const int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(src == ROI_SRC_F32 || C % 8 == 0, "%s: a split-form feature map needs C %% 8 == 0 (got %d)", who, C);
    RPN_REQUIRE(aligned16(d_x) && aligned16(d_out), "%s: the feature map and the output must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const dim3 grid((unsigned)((long long)B * R), (unsigned)((ph * pw + kRoiSampleTile - 1) / kRoiSampleTile)), block(64 * kRoiWaves);
    if (src == ROI_SRC_F32)
        hipLaunchKernelGGL(roi_pool_kernel<ROI_SRC_F32>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, d_valid, d_out);
    else if (src == ROI_SRC_SPLIT_BF16)
        hipLaunchKernelGGL(roi_pool_kernel<ROI_SRC_SPLIT_BF16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, d_valid, d_out);
    else
        hipLaunchKernelGGL(roi_pool_kernel<ROI_SRC_SPLIT_F16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, d_valid, d_out);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

// sampling_ratio and extent: checked with the geometry, before any device use
static int roi_align_check(const char *who, int s, float extent_y, float extent_x)
{
    RPN_REQUIRE(s >= 1 && s <= kRoiAlignMaxSamples, "%s: sampling_ratio %d outside [1, %d]", who, s, kRoiAlignMaxSamples);
    RPN_REQUIRE(std::isfinite(extent_y) && std::isfinite(extent_x) && extent_y > 0.0f && extent_x > 0.0f,
                "%s: the extent must be finite and > 0 (got %g x %g)", who, (double)extent_y, (double)extent_x);
    return RPN_OK;
}

int roi_align_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                      int pw, int sampling_ratio, float extent_y, float extent_x, const int *d_valid, float *d_out, hipStream_t s)
{
    RPN_REQUIRE(d_x && d_rois && d_out, "%s: null pointer", who);
    int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st == RPN_OK) st = roi_align_check(who, sampling_ratio, extent_y, extent_x);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(src == ROI_SRC_F32 || C % 8 == 0, "%s: a split-form feature map needs C %% 8 == 0 (got %d)", who, C);
    RPN_REQUIRE(aligned16(d_x) && aligned16(d_out), "%s: the feature map and the output must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const dim3 grid((unsigned)((long long)B * R), (unsigned)((ph * pw + kRoiSampleTile - 1) / kRoiSampleTile)), block(64 * kRoiWaves);
    if (src == ROI_SRC_F32)
        hipLaunchKernelGGL(roi_align_kernel<ROI_SRC_F32>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, sampling_ratio, extent_y,
                           extent_x, d_valid, d_out);
    else if (src == ROI_SRC_SPLIT_BF16)
        hipLaunchKernelGGL(roi_align_kernel<ROI_SRC_SPLIT_BF16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, sampling_ratio,
                           extent_y, extent_x, d_valid, d_out);
    else
        hipLaunchKernelGGL(roi_align_kernel<ROI_SRC_SPLIT_F16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, sampling_ratio,
                           extent_y, extent_x, d_valid, d_out);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

static int roi_extent_check(const char *who, float extent_y, float extent_x)
{
    RPN_REQUIRE(std::isfinite(extent_y) && std::isfinite(extent_x) && extent_y > 0.0f && extent_x > 0.0f,
                "%s: the extent must be finite and > 0 (got %g x %g)", who, (double)extent_y, (double)extent_x);
    return RPN_OK;
}

int roi_max_pool_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                         int pw, float extent_y, float extent_x, const int *d_valid, float *d_out, int32_t *d_argmax, hipStream_t s)
{
    RPN_REQUIRE(d_x && d_rois && d_out, "%s: null pointer", who);
    int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st == RPN_OK) st = roi_extent_check(who, extent_y, extent_x);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(src == ROI_SRC_F32 || C % 8 == 0, "%s: a split-form feature map needs C %% 8 == 0 (got %d)", who, C);
    RPN_REQUIRE(aligned16(d_x) && aligned16(d_out) && aligned16(d_argmax),
                "%s: the feature map, the output and the argmax must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const dim3 grid((unsigned)((long long)B * R), (unsigned)((ph * pw + kRoiSampleTile - 1) / kRoiSampleTile)), block(64 * kRoiWaves);
    if (src == ROI_SRC_F32)
        hipLaunchKernelGGL(roi_max_pool_kernel<ROI_SRC_F32>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, extent_y, extent_x,
                           d_valid, d_out, d_argmax);
    else if (src == ROI_SRC_SPLIT_BF16)
        hipLaunchKernelGGL(roi_max_pool_kernel<ROI_SRC_SPLIT_BF16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, extent_y,
                           extent_x, d_valid, d_out, d_argmax);
    else
        hipLaunchKernelGGL(roi_max_pool_kernel<ROI_SRC_SPLIT_F16>, grid, block, 0, s, d_x, H, W, C, d_rois, R, ph, pw, extent_y,
                           extent_x, d_valid, d_out, d_argmax);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

}  // namespace rpn

using namespace rpn;

extern "C" int rpn_roi_pool(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw,
                            const int *d_valid, float *d_out, void *stream)
{
    return roi_pool_forward("rpn_roi_pool", d_x, ROI_SRC_F32, B, H, W, C, d_rois, R, ph, pw, d_valid, d_out, as_stream(stream));
}

extern "C" int rpn_roi_pool_backward(const float *d_dy, const float *d_rois, const int *d_valid, int B, int H, int W, int C, int R,
                                     int ph, int pw, float *d_dx, void *stream)
{
    const char *who = "rpn_roi_pool_backward";
    RPN_REQUIRE(d_dy && d_rois && d_dx, "%s: null pointer", who);
    const int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(aligned16(d_dy) && aligned16(d_dx) && aligned16(d_rois), "%s: dy, dx and rois must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const int ctiles = (C + kRoiChannelTile - 1) / kRoiChannelTile;
    hipLaunchKernelGGL(roi_pool_backward_kernel, dim3((unsigned)((long long)B * H * W * ctiles)), dim3(64), 0, as_stream(stream), d_dy,
                       d_rois, d_valid, H, W, C, R, ph, pw, ctiles, d_dx);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" int rpn_roi_align(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw,
                             int sampling_ratio, float extent_y, float extent_x, const int *d_valid, float *d_out, void *stream)
{
    return roi_align_forward("rpn_roi_align", d_x, ROI_SRC_F32, B, H, W, C, d_rois, R, ph, pw, sampling_ratio, extent_y, extent_x,
                             d_valid, d_out, as_stream(stream));
}

extern "C" int rpn_roi_align_backward(const float *d_dy, const float *d_rois, const int *d_valid, int B, int H, int W, int C, int R,
                                      int ph, int pw, int sampling_ratio, float extent_y, float extent_x, float *d_dx, void *stream)
{
    const char *who = "rpn_roi_align_backward";
    RPN_REQUIRE(d_dy && d_rois && d_dx, "%s: null pointer", who);
    int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st == RPN_OK) st = roi_align_check(who, sampling_ratio, extent_y, extent_x);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(aligned16(d_dy) && aligned16(d_dx) && aligned16(d_rois), "%s: dy, dx and rois must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const int ctiles = (C + kRoiChannelTile - 1) / kRoiChannelTile;
    hipLaunchKernelGGL(roi_align_backward_kernel, dim3((unsigned)((long long)B * H * W * ctiles)), dim3(64), 0, as_stream(stream), d_dy,
                       d_rois, d_valid, H, W, C, R, ph, pw, sampling_ratio, extent_y, extent_x, ctiles, d_dx);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" int rpn_roi_max_pool(const float *d_x, int B, int H, int W, int C, const float *d_rois, int R, int ph, int pw,
                                float extent_y, float extent_x, const int *d_valid, float *d_out, int32_t *d_argmax, void *stream)
{
    return roi_max_pool_forward("rpn_roi_max_pool", d_x, ROI_SRC_F32, B, H, W, C, d_rois, R, ph, pw, extent_y, extent_x, d_valid, d_out,
                                d_argmax, as_stream(stream));
}

extern "C" int rpn_roi_max_pool_backward(const float *d_dy, const int32_t *d_argmax, const float *d_rois, const int *d_valid, int B,
                                         int H, int W, int C, int R, int ph, int pw, float extent_y, float extent_x, float *d_dx,
                                         void *stream)
{
    const char *who = "rpn_roi_max_pool_backward";
    RPN_REQUIRE(d_dy && d_argmax && d_rois && d_dx, "%s: null pointer", who);
    int st = roi_check(who, B, H, W, C, R, ph, pw);
    if (st == RPN_OK) st = roi_extent_check(who, extent_y, extent_x);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(aligned16(d_dy) && aligned16(d_argmax) && aligned16(d_dx) && aligned16(d_rois),
                "%s: dy, argmax, dx and rois must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const int ctiles = (C + kRoiChannelTile - 1) / kRoiChannelTile;
    hipLaunchKernelGGL(roi_max_pool_backward_kernel, dim3((unsigned)((long long)B * H * W * ctiles)), dim3(64), 0, as_stream(stream),
                       d_dy, d_argmax, d_rois, d_valid, H, W, C, R, ph, pw, extent_y, extent_x, ctiles, d_dx);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}
