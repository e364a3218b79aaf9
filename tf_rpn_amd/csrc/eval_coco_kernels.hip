// eval_coco_kernels.hip -- COCO-style scoring of the detections on the device: AP over several IoU thresholds and area ranges, AR at
// several cut-offs (rpn_coco_evaluator_*; the contract is written out in include/rpn_hip.h).  A second handle beside rpn_evaluator
// (eval_kernels.hip), which keeps its rules.
//
// No reference counterpart.  The rules are pycocotools' COCOeval in bbox mode without crowd boxes; the header marks this project's
// own choices.
//
//   coco_match_kernel : one 1024-thread workgroup per image, ~153 KB of LDS.
//                       (1) the gts, sorted by (label, input index) with a bitonic sort of 64-bit keys in LDS, then staged in that
//                           order: box, label << 1 | difficult, pixel area (24 bytes each) -- a class's gts are one run, in input order;
//                       (2) the rows, sorted by (class, score descending, m ascending) the same way; the class segments and every
//                           row's segment from one scan of the sorted keys;
//                       (3) the greedy chains, one per (class segment, area range, threshold).  A class with ng <= 32 gts takes
//                           W = pow2(ng) lanes per chain, so a wave runs 64 / W chains of a segment side by side (lane = chain * W
//                           + gt); with more gts a chain has the wave and gt lane + 64 j is bit j of the lane's `taken` /
//                           `ignored` words.  The (segment, group of chains) items go to the 16 waves round robin.  The
//                           detections come 64 at a time (one global load per lane, then lane broadcasts); every lane computes
//                           the IoU of its gt and two group maxima (DPP), of (non-ignored, IoU bits) and of the index, pick the
//                           match: the later index wins a tie.  The chain is cut at max_dets[K-1] steps.  2 bits per (a, t) and
//                           row go to LDS with integer atomics;
//                       (4) one record per row: (score, class << 12 | rank; 0 = not counted) and 12 bytes of flags, vector stores;
//                           npig / ndet with integer atomics.
//                       HBM per image: 28 M + 21 G read, 20 M (+ A T M flags) written.
//   coco_rank_kernel  : one workgroup per class: compaction in slot order and the stable radix sort of eval_sort.h, shared with
//                       eval_class_kernel.  HBM per class: 8 n_records read; 16 n_c per sort pass.
//   coco_curve_kernel : one workgroup per (class, area range, threshold).  Pass 1 counts TP at every cut-off and FP; pass 2 walks the
//                       ranking backwards in tiles (cumulative counts from the totals, a workgroup scan per tile), precision in
//                       float64, its reverse running maximum, and the 101-point sum in closed form: the j-th TP stands for the
//                       recall points q with 100 (j - 1) < q npig <= 100 j (and q = 0 for j = 1).  Per-thread partials in tile order,
//                       then a fixed LDS tree.  HBM per workgroup: 2 x 16 n_c gathered.
// No floating-point atomics, every float64 sum in an order fixed by the counts alone.  Compiled with -ffp-contract=off: the IoU is
// generate_iou_map's (bbox_core.h) and the pixel areas round after every operation.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>

#include "bbox_core.h"
#include "eval_sort.h"
#include "rpn_common.h"

namespace rpn {

constexpr int kCoMaxG = 2048;
constexpr int kCoMaxM = 4096;
constexpr int kCoMaxC = 65535;
constexpr int kCoMaxT = 10, kCoMaxA = 4, kCoMaxK = 4;
constexpr int kCoFlagWords = 3;                         // 2 bits per (a, t): at most 80 of 96
constexpr unsigned long long kCoPad = ~0ull;            // a sort key beyond the input
constexpr unsigned kCoNoClass = 0xFFFFu;                // the class field of a row that is not live (C <= 65535: never a class)

struct CocoConfig {
    int T, A, K;
    float thr[kCoMaxT];
    float lo[kCoMaxA], hi[kCoMaxA];
    int max_dets[kCoMaxK];
};

struct CocoMatchArgs {
    const float *boxes, *scores, *classes;
    const int *valid;
    const float *gt;
    const int *labels;
    const unsigned char *difficult;
    const float *sizes;            // (B,2) [height, width] or null
    float height, width;
    int M, G, C;
    CocoConfig cfg;
    long long slot0;
    int2 *rec;                     // (score bits, class << 12 | rank; 0 = not counted)
    unsigned *recflags;            // 3 words per slot
    int *npig, *ndet;              // (C,A), (C,)
    signed char *flags;            // (B,M,A,T) or null
};

// ascending bitonic sort of keys[0, n), n a power of two >= 2, by the whole workgroup
__device__ __forceinline__ void co_bitonic(unsigned long long *keys, int n)
{
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = threadIdx.x; idx < (n >> 1); idx += kEvThreads) {
                const int i = 2 * idx - (idx & (j - 1)), l = i + j;
                const unsigned long long x = keys[i], y = keys[l];
                const bool up = (i & k) == 0;
                if ((x > y) == up) {
                    keys[i] = y;
                    keys[l] = x;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int co_pow2(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ float co_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// The maximum of v over every group of `width` consecutive lanes (a power of two, the same in the whole wave), in every lane of the
// group: an xor butterfly -- DPP inside the rows of 16 (the two quad permutations; once the quads agree the half-row mirror is the
// exchange of quads and the row mirror that of half-rows), ds_bpermute across rows.  Every lane of the wave must be active.
__device__ __forceinline__ unsigned co_group_umax(unsigned v, int width)
{
    if (width >= 2) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));       // quad_perm [1,0,3,2]
    if (width >= 4) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));       // quad_perm [2,3,0,1]
    if (width >= 8) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));      // row_half_mirror
    if (width >= 16) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));     // row_mirror
    if (width >= 32) v = max(v, (unsigned)__shfl_xor((int)v, 16, 64));
    if (width >= 64) v = max(v, (unsigned)__shfl_xor((int)v, 32, 64));
    return v;
}

__device__ __forceinline__ float co_pixel_area(const Box &b, float height, float width)
{
    const float h = (b.y2 - b.y1) * height, w = (b.x2 - b.x1) * width;
    return h * w;
}

__global__ void __launch_bounds__(kEvThreads)
coco_match_kernel(CocoMatchArgs p)
{
    __shared__ __attribute__((aligned(16))) float gts[4 * kCoMaxG];
    __shared__ int gcode[kCoMaxG];                          // label << 1 | difficult, sorted; INT_MAX beyond the counted gts
    __shared__ float gpix[kCoMaxG];
    __shared__ unsigned long long keys[kCoMaxM];
    __shared__ unsigned fl[kCoFlagWords * kCoMaxM];         // by sorted position
    __shared__ unsigned short segs[kCoMaxM + 1];
    __shared__ unsigned short seg_g0[kCoMaxM], seg_ng[kCoMaxM];     // the gt run of every segment's class
    __shared__ float cfg_thr[kCoMaxT], cfg_lo[kCoMaxA], cfg_hi[kCoMaxA];
    __shared__ int wsum[kEvWaves];
    __shared__ int n_live_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
    const int M = p.M, G = p.G, C = p.C;
    const int T = p.cfg.T, A = p.cfg.A, AT = A * T;
    const int cut = p.cfg.max_dets[p.cfg.K - 1];
    const float height = p.sizes ? p.sizes[2 * (size_t)b] : p.height, width = p.sizes ? p.sizes[2 * (size_t)b + 1] : p.width;

    // (1) the gts, by (label, input index)
    const int NG = co_pow2(G);
    for (int g = tid; g < NG; g += kEvThreads) {
        unsigned long long key = kCoPad;
        if (g < G) {
            const int lab = p.labels[(size_t)b * G + g];
            if (lab >= 1 && lab < C) key = ((unsigned long long)lab << 12) | (unsigned long long)g;
        }
        keys[g] = key;
    }
    __syncthreads();
    co_bitonic(keys, NG);
    for (int i = tid; i < G; i += kEvThreads) {
        const unsigned long long key = keys[i];
        int code = 0x7FFFFFFF;
        if (key != kCoPad) {
            const int gi = (int)(key & 0xFFFull);
            const int lab = (int)(key >> 12);
            const int diff = p.difficult ? (p.difficult[(size_t)b * G + gi] != 0) : 0;
            const Box gb = load_box(p.gt + 4 * ((size_t)b * G + gi));
            const float pix = co_pixel_area(gb, height, width);
            store_box(gts + 4 * i, gb);
            gpix[i] = pix;
            code = (int)(((unsigned)lab << 1) | (unsigned)diff);
            for (int a = 0; a < A; ++a)
                if (!diff && !(pix < p.cfg.lo[a]) && !(pix > p.cfg.hi[a])) atomicAdd(&p.npig[lab * A + a], 1);
        }
        gcode[i] = code;
    }
    __syncthreads();                                        // (keys are reused below)

    // (2) the rows, by (class, score descending, m ascending); rows that are not live keep their m behind every class
    const int NM = co_pow2(M);
    const int live = min(max(p.valid[b], 0), M);
    for (int m = tid; m < NM; m += kEvThreads) {
        unsigned long long key = kCoPad;
        if (m < M) {
            const size_t row = (size_t)b * M + m;
            const float s = p.scores[row], cf = p.classes[row];
            key = ((unsigned long long)kCoNoClass << 44) | (0xFFFFFFFFull << 12) | (unsigned long long)m;
            if (m < live && cf >= 1.0f && cf < (float)C && s > 0.0f && s < INFINITY) {
                const int c = (int)cf;
                if ((float)c == cf) key = ((unsigned long long)c << 44) | ((unsigned long long)(~orderable(s)) << 12) | (unsigned long long)m;
            }
        }
        keys[m] = key;
    }
    for (int i = tid; i < kCoFlagWords * NM; i += kEvThreads) fl[i] = 0u;
    if (tid == 0) n_live_s = NM;
    __syncthreads();
    co_bitonic(keys, NM);
    // segments: a head wherever the class changes; every live key then carries its segment in place of its score
    int nseg = 0;
    for (int i0 = 0; i0 < NM; i0 += kEvThreads) {
        const int i = i0 + tid;
        const unsigned long long key = i < NM ? keys[i] : kCoPad;
        const unsigned cls = (unsigned)(key >> 44);         // 0xFFFFF for a pad
        const bool is_live = cls < kCoNoClass;
        bool prev_live = false;
        unsigned prev_cls = 0u;
        if (i > 0 && i < NM) {
            prev_cls = (unsigned)(keys[i - 1] >> 44);
            prev_live = prev_cls < kCoNoClass;
        }
        const bool head = is_live && (i == 0 || prev_cls != cls);
        if (i < NM && !is_live && (i == 0 || prev_live)) n_live_s = i;
        int total;
        const int excl = block_scan(head ? 1 : 0, wsum, &total);        // (two barriers: every neighbour is read before any key is rewritten)
        if (is_live) {
            const int s = nseg + excl + (head ? 1 : 0) - 1;
            if (head) segs[s] = (unsigned short)i;
            keys[i] = ((unsigned long long)cls << 44) | ((unsigned long long)s << 12) | (key & 0xFFFull);
        }
        nseg += total;
        __syncthreads();
    }
    if (tid == 0) segs[nseg] = (unsigned short)n_live_s;
    __syncthreads();

    // (3) the chains.  The gt run of every segment first, a thread per segment.
    for (int sg = tid; sg < nseg; sg += kEvThreads) {
        const int c = (int)(keys[segs[sg]] >> 44);
        int l = 0, r = G;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if ((gcode[mid] >> 1) < c) l = mid + 1; else r = mid;
        }
        const int first = l;
        r = G;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if ((gcode[mid] >> 1) <= c) l = mid + 1; else r = mid;
        }
        seg_g0[sg] = (unsigned short)first;
        seg_ng[sg] = (unsigned short)(l - first);
    }
    if (tid < kCoMaxT) cfg_thr[tid] = tid < T ? p.cfg.thr[tid] : INFINITY;
    if (tid < kCoMaxA) {
        cfg_lo[tid] = tid < A ? p.cfg.lo[tid] : 0.0f;
        cfg_hi[tid] = tid < A ? p.cfg.hi[tid] : 0.0f;
    }
    __syncthreads();
    // A class with ng <= 32 gts needs W = pow2(ng) lanes per chain, so a wave runs P = 64 / W of the segment's A T chains side by
    // side: lane = chain * W + gt.  With more gts a chain has the whole wave and gt lane + 64 j is bit j of the lane's words.  The
    // (segment, group of P chains) items are dealt to the waves round robin in that order.
    int dealt = 0;
    for (int s = 0; s < nseg; ++s) {
        const int ng = seg_ng[s];
        int W = 1;
        while (W < ng && W < 64) W <<= 1;
        const int P = 64 / W, groups = (AT + P - 1) / P;
        const int mine_first = ((w - dealt) % kEvWaves + kEvWaves) % kEvWaves;      // this wave's first group of the segment
        dealt += groups;
        if (mine_first >= groups) continue;
        const int p0 = segs[s], p1 = min((int)segs[s + 1], p0 + cut);
        const int g0 = seg_g0[s];
        const int strides = W < 64 ? 1 : (ng + 63) >> 6;    // <= 32
        const int gl0 = lane & (W - 1), sub = lane / W;
        Box gfirst = Box{0.0f, 0.0f, 0.0f, 0.0f};
        float gfirst_area = 0.0f;
        if (gl0 < ng) {
            gfirst = load_box(gts + 4 * (g0 + gl0));
            gfirst_area = box_area_plain(gfirst);
        }
        const bool one_chunk = p1 - p0 <= 64;
        Box mine = Box{0.0f, 0.0f, 0.0f, 0.0f};
        float mypix = 0.0f;
        if (one_chunk && p0 + lane < p1) {
            mine = load_box(p.boxes + 4 * ((size_t)b * M + (int)(keys[p0 + lane] & 0xFFFull)));
            mypix = co_pixel_area(mine, height, width);
        }
        for (int gi = mine_first; gi < groups; gi += kEvWaves) {
            const int at = gi * P + sub;                    // this lane's chain
            const bool chain = at < AT;
            const int a = chain ? at / T : 0, t = chain ? at - a * T : 0;
            const float thr = chain ? cfg_thr[t] : INFINITY, lo = cfg_lo[a], hi = cfg_hi[a];
            unsigned taken = chain ? 0u : ~0u, ign = 0u;     // (a lane without a chain matches nothing)
            for (int j = 0; j < strides; ++j) {
                const int g = g0 + gl0 + 64 * j;
                if (gl0 + 64 * j < ng) {
                    const float pix = gpix[g];
                    if ((gcode[g] & 1) || pix < lo || pix > hi) ign |= 1u << j;
                } else {
                    taken |= 1u << j;                       // no gt here
                }
            }
            const int bit = 2 * at, word = bit >> 5, sh = bit & 31;
            for (int d0 = p0; d0 < p1; d0 += 64) {
                if (!one_chunk && d0 + lane < p1) {
                    mine = load_box(p.boxes + 4 * ((size_t)b * M + (int)(keys[d0 + lane] & 0xFFFull)));
                    mypix = co_pixel_area(mine, height, width);
                }
                const int cnt = min(64, p1 - d0);
                for (int i = 0; i < cnt; ++i) {
                    const Box d = Box{co_bcast(mine.y1, i), co_bcast(mine.x1, i), co_bcast(mine.y2, i), co_bcast(mine.x2, i)};
                    const float dpix = co_bcast(mypix, i);
                    const float darea = box_area_plain(d);
                    // this lane's best: (non-ignored << 31 | IoU bits), 0 = none, and its index in the run; the later gt wins a tie
                    unsigned best = 0u;
                    int best_gl = 0;
                    for (int j = 0; j < strides; ++j) {
                        if ((taken >> j) & 1u) continue;
                        const int gl = gl0 + 64 * j;
                        Box gb = gfirst;
                        float garea = gfirst_area;
                        if (j > 0) {
                            gb = load_box(gts + 4 * (g0 + gl));
                            garea = box_area_plain(gb);
                        }
                        const float iou = iou_map_pair(d, darea, gb, garea);
                        if (iou >= thr) {                   // a NaN never matches; thr > 0, so the bits order as the values
                            const unsigned key = ((((ign >> j) & 1u) ^ 1u) << 31) | __float_as_uint(iou);
                            if (key >= best) {
                                best = key;
                                best_gl = gl;
                            }
                        }
                    }
                    const unsigned top = co_group_umax(best, W);
                    const int win = (int)co_group_umax(best == top && top != 0u ? (unsigned)best_gl + 1u : 0u, W) - 1;
                    unsigned code;                          // 0 FP, 1 TP, 2 ignored
                    if (top != 0u) {
                        if ((win & 63) == gl0) taken |= 1u << (win >> 6);
                        code = (top >> 31) ? 1u : 2u;
                    } else {
                        code = (dpix < lo || dpix > hi) ? 2u : 0u;
                    }
                    if (chain && gl0 == 0 && code) atomicOr(&fl[kCoFlagWords * (d0 + i) + word], code << sh);
                }
            }
        }
    }
    __syncthreads();

    // (4) one record per row
    for (int i = tid; i < NM; i += kEvThreads) {
        const unsigned long long key = keys[i];
        if (key == kCoPad) continue;
        const int m = (int)(key & 0xFFFull);
        const unsigned cls = (unsigned)(key >> 44);
        const size_t row = (size_t)b * M + m;
        const long long slot = p.slot0 + (long long)row;
        int head = 0;
        unsigned f0 = 0u, f1 = 0u, f2 = 0u;
        if (cls < kCoNoClass) {
            const int s = (int)((key >> 12) & 0xFFFull);
            const int rank = i - (int)segs[s];
            if (rank < cut) {
                head = (int)((cls << 12) | (unsigned)rank);
                f0 = fl[kCoFlagWords * i];
                f1 = fl[kCoFlagWords * i + 1];
                f2 = fl[kCoFlagWords * i + 2];
                if (rank == 0) atomicAdd(&p.ndet[cls], min((int)segs[s + 1] - (int)segs[s], cut));
            }
        }
        p.rec[slot] = make_int2(__float_as_int(p.scores[row]), head);
        p.recflags[kCoFlagWords * slot] = f0;
        p.recflags[kCoFlagWords * slot + 1] = f1;
        p.recflags[kCoFlagWords * slot + 2] = f2;
        if (p.flags) {
            signed char *out = p.flags + row * (size_t)AT;
            for (int at = 0; at < AT; ++at) {
                const unsigned wd = (2 * at) >> 5 == 0 ? f0 : ((2 * at) >> 5 == 1 ? f1 : f2);
                const unsigned code = (wd >> ((2 * at) & 31)) & 3u;
                out[at] = head == 0 ? (signed char)-2 : (code == 2u ? (signed char)-1 : (signed char)code);
            }
        }
    }
}

// ---- per-class ranking ----------------------------------------------------------------------------------------------------------
struct CocoRankArgs {
    const int2 *rec;
    long long n_rec;
    const int *ndet;
    uint2 *buf[2];                 // ping-pong workspace: (key, slot)
    int *parity;
};

__global__ void __launch_bounds__(kEvThreads)
coco_rank_kernel(CocoRankArgs p)
{
    __shared__ EvSortLds sort_lds;
    const int c = blockIdx.x;
    const int n = p.ndet[c];
    long long off = 0;
    for (int i = 0; i < c; ++i) off += p.ndet[i];
    uint2 *cur = p.buf[0] + off, *alt = p.buf[1] + off;
    ev_compact(
        p.rec, p.n_rec, cur, n, sort_lds.wsum, [c](const int2 &r) { return r.y != 0 && (int)((unsigned)r.y >> 12) == c; },
        [](const int2 &r, long long slot) { return make_uint2(~orderable(__int_as_float(r.x)), (unsigned)slot); });
    const int par = ev_radix_sort(cur, alt, n, sort_lds);
    if (threadIdx.x == 0) p.parity[c] = par;
}

// ---- curves -------------------------------------------------------------------------------------------------------------------
struct CocoCurveArgs {
    const int2 *rec;
    const unsigned *recflags;
    const int *npig, *ndet, *parity;
    const uint2 *buf[2];
    CocoConfig cfg;
    double *ap, *ar;               // (C,A,T), (C,A,T,K) or null
};

__global__ void __launch_bounds__(kEvThreads)
coco_curve_kernel(CocoCurveArgs p)
{
    __shared__ int wsum[kEvWaves];
    __shared__ int cnt[kCoMaxK + 1];
    __shared__ double wmax[kEvWaves];
    __shared__ double red[kEvThreads];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int T = p.cfg.T, A = p.cfg.A, K = p.cfg.K;
    const int c = blockIdx.x, a = blockIdx.y / T, t = blockIdx.y - a * T;
    const int npig = p.npig[c * A + a];
    const size_t o_ap = ((size_t)c * A + a) * T + t;
    if (c == 0 || npig <= 0) {
        if (tid == 0 && p.ap) p.ap[o_ap] = NAN;
        if (tid < K && p.ar) p.ar[o_ap * K + tid] = NAN;
        return;
    }
    const int n = p.ndet[c];
    long long off = 0;
    for (int i = 0; i < c; ++i) off += p.ndet[i];
    const uint2 *src = (p.parity[c] ? p.buf[1] : p.buf[0]) + off;
    const int bit = 2 * (a * T + t), word = bit >> 5, sh = bit & 31;

    // pass 1: TP at every cut-off, FP at the last
    if (tid <= kCoMaxK) cnt[tid] = 0;
    __syncthreads();
    {
        int tp[kCoMaxK] = {0, 0, 0, 0}, fp = 0;
        for (int i = tid; i < n; i += kEvThreads) {
            const unsigned slot = src[i].y;
            const int rank = p.rec[slot].y & 0xFFF;
            const unsigned code = (p.recflags[(size_t)kCoFlagWords * slot + word] >> sh) & 3u;
#pragma unroll
            for (int k = 0; k < kCoMaxK; ++k)
                if (k < K && code == 1u && rank < p.cfg.max_dets[k]) ++tp[k];
            if (code == 0u) ++fp;
        }
#pragma unroll
        for (int k = 0; k < kCoMaxK; ++k)
            if (tp[k]) atomicAdd(&cnt[k], tp[k]);
        if (fp) atomicAdd(&cnt[kCoMaxK], fp);
    }
    __syncthreads();
    if (tid < K && p.ar) p.ar[o_ap * K + tid] = (double)cnt[tid] / (double)npig;
    if (!p.ap) return;

    // pass 2: backwards over the ranking.  Every ranked row is inside the last cut-off.
    int rem_tp = cnt[K - 1], rem_fp = cnt[kCoMaxK];         // TP / FP at or before the end of the current tile
    double acc = 0.0, carry = 0.0;
    const int ntiles = (n + kEvThreads - 1) / kEvThreads;
    for (int tile = ntiles - 1; tile >= 0; --tile) {
        const int i = tile * kEvThreads + tid;
        unsigned code = 2u;
        if (i < n) code = (p.recflags[(size_t)kCoFlagWords * src[i].y + word] >> sh) & 3u;
        const int is_tp = code == 1u, is_fp = code == 0u;
        int tot_tp, tot_fp;
        const int ex_tp = block_scan(is_tp, wsum, &tot_tp);
        const int ex_fp = block_scan(is_fp, wsum, &tot_fp);
        const int tpi = rem_tp - tot_tp + ex_tp + is_tp, fpi = rem_fp - tot_fp + ex_fp + is_fp;
        rem_tp -= tot_tp;
        rem_fp -= tot_fp;
        double pm = code != 2u ? (double)tpi / ((double)(tpi + fpi) + 0x1p-52) : 0.0;      // an ignored row is not on the curve
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_down(pm, o, 64);
            if (lane + o < 64) pm = fmax(pm, v);
        }
        if (lane == 0) wmax[w] = pm;
        __syncthreads();
        double later = carry, all = carry;
#pragma unroll
        for (int k = 0; k < kEvWaves; ++k) {
            const double v = wmax[k];
            if (k > w) later = fmax(later, v);
            all = fmax(all, v);
        }
        pm = fmax(pm, later);
        carry = all;
        if (is_tp) {
            const long long j = tpi;
            const long long q = (100 * j) / npig - (100 * (j - 1)) / npig + (j == 1 ? 1 : 0);
            acc += pm * (double)q;
        }
        __syncthreads();
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kEvThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) p.ap[o_ap] = red[0] / 101.0;
}

__global__ void __launch_bounds__(256)
coco_finish_kernel(const int *__restrict__ npig, const int *__restrict__ ndet, int C, int A, int *__restrict__ out_npig,
                   int *__restrict__ out_ndet)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < C * A; i += gridDim.x * 256) {
        if (out_npig) out_npig[i] = npig[i];
        if (out_ndet && i < C) out_ndet[i] = ndet[i];
    }
}

static bool co_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace rpn

using namespace rpn;

struct rpn_coco_evaluator {
    int C = 0, max_images = 0, M = 0;
    CocoConfig cfg = {};
    float height = 0.0f, width = 0.0f;
    int images = 0;
    // one allocation, made at creation
    unsigned char *d_mem = nullptr;
    size_t bytes = 0, counter_bytes = 0;
    int2 *rec = nullptr;
    unsigned *recflags = nullptr;
    uint2 *buf[2] = {nullptr, nullptr};
    unsigned char *counters = nullptr;     // everything reset() clears, contiguous
    int *npig = nullptr, *ndet = nullptr, *parity = nullptr;
};

// the section offsets of the handle's one allocation; returns its size
static size_t co_layout(rpn_coco_evaluator *e)
{
    const size_t n = (size_t)e->max_images * e->M;
    size_t o = 0;
    const size_t o_rec = o;
    o += a256(n * sizeof(int2));
    const size_t o_fl = o;
    o += a256(n * kCoFlagWords * sizeof(unsigned));
    const size_t o_b0 = o;
    o += a256(n * sizeof(uint2));
    const size_t o_b1 = o;
    o += a256(n * sizeof(uint2));
    const size_t o_cnt = o;
    const size_t o_npig = o;
    o += a256((size_t)e->C * kCoMaxA * 4);
    const size_t o_ndet = o;
    o += a256((size_t)e->C * 4);
    const size_t o_par = o;
    o += a256((size_t)e->C * 4);
    e->counter_bytes = o - o_cnt;
    if (e->d_mem) {
        unsigned char *m = e->d_mem;
        e->rec = reinterpret_cast<int2 *>(m + o_rec);
        e->recflags = reinterpret_cast<unsigned *>(m + o_fl);
        e->buf[0] = reinterpret_cast<uint2 *>(m + o_b0);
        e->buf[1] = reinterpret_cast<uint2 *>(m + o_b1);
        e->counters = m + o_cnt;
        e->npig = reinterpret_cast<int *>(m + o_npig);
        e->ndet = reinterpret_cast<int *>(m + o_ndet);
        e->parity = reinterpret_cast<int *>(m + o_par);
    }
    return o;
}

// Without a device at creation (argument checks and memory_bytes still work) the memory is allocated by the first call that finds one.
static int co_ensure(rpn_coco_evaluator *e)
{
    if (e->d_mem) return RPN_OK;
    RPN_REQUIRE_DEVICE();
    RPN_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&e->d_mem), e->bytes));
    co_layout(e);
    RPN_HIP_CHECK(hipMemset(e->counters, 0, e->counter_bytes));
    RPN_HIP_CHECK(hipDeviceSynchronize());
    return RPN_OK;
}

extern "C" int rpn_coco_evaluator_create(int C, int max_images, int M, const float *iou_thresholds, int T, const float *area_ranges,
                                         int A, const int *max_dets, int K, float height, float width, rpn_coco_evaluator **out)
{
    const char *who = "rpn_coco_evaluator_create";
    RPN_REQUIRE(out, "%s: null pointer", who);
    *out = nullptr;
    RPN_REQUIRE(C >= 2 && C <= kCoMaxC, "%s: C = %d, must be in [2, %d]", who, C, kCoMaxC);
    RPN_REQUIRE(max_images >= 1 && M >= 1 && M <= kCoMaxM, "%s: max_images = %d, M = %d (1 <= M <= %d)", who, max_images, M, kCoMaxM);
    RPN_REQUIRE((long long)max_images * M <= (1ll << 30), "%s: max_images * M = %lld records, at most 2^30", who,
                (long long)max_images * M);
    RPN_REQUIRE(height > 0.0f && height < INFINITY && width > 0.0f && width < INFINITY, "%s: image size %g x %g, must be finite and > 0",
                who, (double)height, (double)width);
    CocoConfig cfg = {};
    if (iou_thresholds) {
        RPN_REQUIRE(T >= 1 && T <= kCoMaxT, "%s: %d IoU thresholds, must be in [1, %d]", who, T, kCoMaxT);
        for (int i = 0; i < T; ++i) {
            RPN_REQUIRE(iou_thresholds[i] > 0.0f && iou_thresholds[i] <= 1.0f, "%s: iou_thresholds[%d] = %g, must be in (0, 1]", who, i,
                        (double)iou_thresholds[i]);
            cfg.thr[i] = iou_thresholds[i];
        }
        cfg.T = T;
    } else {
        cfg.T = 10;
        for (int i = 0; i < 10; ++i) cfg.thr[i] = (float)(0.5 + 0.05 * i);
    }
    if (area_ranges) {
        RPN_REQUIRE(A >= 1 && A <= kCoMaxA, "%s: %d area ranges, must be in [1, %d]", who, A, kCoMaxA);
        for (int i = 0; i < A; ++i) {
            const float lo = area_ranges[2 * i], hi = area_ranges[2 * i + 1];
            RPN_REQUIRE(lo >= 0.0f && lo <= hi && hi < INFINITY, "%s: area range %d = [%g, %g], must be finite with 0 <= lo <= hi", who, i,
                        (double)lo, (double)hi);
            cfg.lo[i] = lo;
            cfg.hi[i] = hi;
        }
        cfg.A = A;
    } else {
        const float d[8] = {0.0f, 1e10f, 0.0f, 1024.0f, 1024.0f, 9216.0f, 9216.0f, 1e10f};
        cfg.A = 4;
        for (int i = 0; i < 4; ++i) {
            cfg.lo[i] = d[2 * i];
            cfg.hi[i] = d[2 * i + 1];
        }
    }
    if (max_dets) {
        RPN_REQUIRE(K >= 1 && K <= kCoMaxK, "%s: %d cut-offs in max_dets, must be in [1, %d]", who, K, kCoMaxK);
        for (int i = 0; i < K; ++i) {
            RPN_REQUIRE(max_dets[i] >= 1 && (i == 0 || max_dets[i] > max_dets[i - 1]), "%s: max_dets must be >= 1 and strictly ascending",
                        who);
            cfg.max_dets[i] = max_dets[i];
        }
        cfg.K = K;
    } else {
        cfg.K = 3;
        cfg.max_dets[0] = 1;
        cfg.max_dets[1] = 10;
        cfg.max_dets[2] = 100;
    }
    RPN_REQUIRE(cfg.max_dets[cfg.K - 1] <= M, "%s: max_dets[%d] = %d > M = %d", who, cfg.K - 1, cfg.max_dets[cfg.K - 1], M);
    rpn_coco_evaluator *e = new (std::nothrow) rpn_coco_evaluator();
    RPN_REQUIRE(e, "%s: out of host memory", who);
    e->C = C; e->max_images = max_images; e->M = M; e->cfg = cfg; e->height = height; e->width = width;
    e->bytes = co_layout(e);
    if (rpn_device_count() >= 1) {
        const int st = co_ensure(e);
        if (st != RPN_OK) {
            delete e;
            return st;
        }
    }
    *out = e;
    return RPN_OK;
}

extern "C" void rpn_coco_evaluator_destroy(rpn_coco_evaluator *e)
{
    if (!e) return;
    if (e->d_mem) (void)hipFree(e->d_mem);
    delete e;
}

extern "C" int rpn_coco_evaluator_memory_bytes(const rpn_coco_evaluator *e, size_t *bytes)
{
    RPN_REQUIRE(e && bytes, "rpn_coco_evaluator_memory_bytes: null pointer");
    *bytes = e->bytes;
    return RPN_OK;
}

extern "C" int rpn_coco_evaluator_images(const rpn_coco_evaluator *e) { return e ? e->images : 0; }

extern "C" int rpn_coco_evaluator_reset(rpn_coco_evaluator *e, void *stream)
{
    RPN_REQUIRE(e, "rpn_coco_evaluator_reset: null pointer");
    const int st = co_ensure(e);
    if (st != RPN_OK) return st;
    RPN_HIP_CHECK(hipMemsetAsync(e->counters, 0, e->counter_bytes, as_stream(stream)));
    e->images = 0;
    return RPN_OK;
}

extern "C" int rpn_coco_evaluator_update(rpn_coco_evaluator *e, const float *d_boxes, const float *d_scores, const float *d_classes,
                                         const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels,
                                         const unsigned char *d_gt_difficult, const float *d_image_sizes, int B, int G,
                                         signed char *d_flags, void *stream)
{
    const char *who = "rpn_coco_evaluator_update";
    RPN_REQUIRE(e && d_boxes && d_scores && d_classes && d_valid && d_gt_boxes && d_gt_labels, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && G >= 1, "%s: B and G must be >= 1 (got %d, %d)", who, B, G);
    RPN_REQUIRE(G <= kCoMaxG, "%s: G = %d > %d", who, G, kCoMaxG);
    RPN_REQUIRE((long long)e->images + B <= e->max_images, "%s: %d images seen + %d > max_images = %d", who, e->images, B, e->max_images);
    RPN_REQUIRE(co_aligned16(d_boxes) && co_aligned16(d_gt_boxes), "%s: boxes and gt boxes must be 16-byte aligned", who);
    const int st = co_ensure(e);
    if (st != RPN_OK) return st;
    CocoMatchArgs p{};
    p.boxes = d_boxes; p.scores = d_scores; p.classes = d_classes; p.valid = d_valid;
    p.gt = d_gt_boxes; p.labels = d_gt_labels; p.difficult = d_gt_difficult; p.sizes = d_image_sizes;
    p.height = e->height; p.width = e->width;
    p.M = e->M; p.G = G; p.C = e->C; p.cfg = e->cfg;
    p.slot0 = (long long)e->images * e->M;
    p.rec = e->rec; p.recflags = e->recflags; p.npig = e->npig; p.ndet = e->ndet; p.flags = d_flags;
    hipLaunchKernelGGL(coco_match_kernel, dim3(B), dim3(kEvThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    e->images += B;
    return RPN_OK;
}

extern "C" int rpn_coco_evaluator_result(rpn_coco_evaluator *e, double *d_ap, double *d_ar, int32_t *d_npig, int32_t *d_ndet, void *stream)
{
    const char *who = "rpn_coco_evaluator_result";
    RPN_REQUIRE(e, "%s: null pointer", who);
    int st = co_ensure(e);
    if (st != RPN_OK) return st;
    hipStream_t s = as_stream(stream);
    if (d_ap || d_ar) {
        CocoRankArgs r{};
        r.rec = e->rec;
        r.n_rec = (long long)e->images * e->M;
        r.ndet = e->ndet;
        r.buf[0] = e->buf[0]; r.buf[1] = e->buf[1];
        r.parity = e->parity;
        hipLaunchKernelGGL(coco_rank_kernel, dim3(e->C), dim3(kEvThreads), 0, s, r);
        RPN_CHECK_LAUNCH();
        CocoCurveArgs p{};
        p.rec = e->rec; p.recflags = e->recflags; p.npig = e->npig; p.ndet = e->ndet; p.parity = e->parity;
        p.buf[0] = e->buf[0]; p.buf[1] = e->buf[1];
        p.cfg = e->cfg; p.ap = d_ap; p.ar = d_ar;
        hipLaunchKernelGGL(coco_curve_kernel, dim3(e->C, e->cfg.A * e->cfg.T), dim3(kEvThreads), 0, s, p);
        RPN_CHECK_LAUNCH();
    }
    if (d_npig || d_ndet) {
        const int grid = std::max(1, std::min((e->C * e->cfg.A + 255) / 256, 1024));
        hipLaunchKernelGGL(coco_finish_kernel, dim3(grid), dim3(256), 0, s, e->npig, e->ndet, e->C, e->cfg.A, d_npig, d_ndet);
        RPN_CHECK_LAUNCH();
    }
    return RPN_OK;
}
