// eval_kernels.hip -- the detection metric on the device: PASCAL VOC average precision of the detections and the recall of the
// proposals (rpn_evaluator_*; the contract is written out in include/rpn_hip.h).
//
// No reference counterpart: the reference's training script stops at val_loss.  The matching rule is VOCdevkit's VOCevaldet; where
// the devkit is loose (ties, the 11-point comparison) the choice is this project's and the header states it.
//
//   eval_match_kernel   : one 1024-thread workgroup per image.  The gt boxes, their (label, difficult) codes and one 64-bit claim
//                         word per gt sit in LDS (56 KB at G = 2048); every thread owns up to four detection rows (m = tid + 1024 u,
//                         M <= 4096) and keeps each row's best IoU / first argmax among the gts of its class in registers.  A row that
//                         reaches the threshold on a non-difficult gt posts (~orderable(score) << 12 | m) with an LDS atomic minimum
//                         on that gt's claim word: after the barrier the row whose key is still there is the true positive.  Each
//                         row's (score, class << 1 | tp) record goes to its slot of the handle's record buffer with one 8-byte vector
//                         store (0 in the second word: not counted); npos / ndet with integer atomics.
//                         HBM per image: 28 M + 21 G read, 8 M (+ 4 M flags) written.
//   eval_recall_kernel  : one 256-thread workgroup per image, a thread per gt: the running maximum IoU over the RoIs in order (the
//                         RoI address is the same in every lane: one scalar load), read at the cut-offs in ascending order.
//                         HBM per image: 16 min(max k, valid) + 21 G read; <= 64 integer atomics per workgroup.
//   eval_class_kernel   : one 1024-thread workgroup per class ((1) and (2) are eval_sort.h's, shared with eval_coco_kernels.hip).
//                         (1) the class's live records, compacted in slot order into the
//                         workspace as (~orderable(score), slot << 1 | tp) pairs (eight records per thread, a workgroup scan of the
//                         counts, no atomics); (2) a stable LSD radix sort, four 8-bit passes over a ping-pong pair -- all four
//                         histograms from one read, a pass whose digit is the same in every key is skipped, tiles of 4096 keys, ranks
//                         inside a tile from wave ballots and per-wave digit counts, so equal keys keep slot order;
//                         (3) an inclusive scan of the TP flags written over the keys, then a reverse max-scan of the float64
//                         precisions with the AP sums: per-thread partials in tile order, then a fixed LDS tree.
//                         HBM per class: 8 n_records read in (1); 16 n_c per sort pass; 24 n_c in (3).  O(n passes), no rank counting.
//   eval_finish_kernel  : counters -> recall (float64), npos, ndet.     eval_curve_kernel: one class's ranking -> (score, tp, slot).
// No floating-point atomics anywhere, every float64 sum in an order fixed by the counts alone: result() gives the same bits on every
// run.  Compiled with -ffp-contract=off: the IoU is generate_iou_map's (bbox_core.h), bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>

#include "bbox_core.h"
#include "eval_sort.h"
#include "rpn_common.h"

namespace rpn {

constexpr int kEvMaxG = 2048;              // as rpn_roi_targets
constexpr int kEvMaxM = 4096;
constexpr int kEvMaxCut = 8;               // cut-offs and thresholds of the proposal recall
constexpr int kEvMaxC = 65535;
constexpr int kEvRows = kEvMaxM / kEvThreads;              // detection rows per thread of the match kernel
constexpr int kEvRecallThreads = 256;

// ---- matching ---------------------------------------------------------------------------------------------------------------
struct EvalMatchArgs {
    const float *boxes;            // (B,M,4)
    const float *scores;           // (B,M)
    const float *classes;          // (B,M) float32, as the NMS returns them
    const int *valid;              // (B,)
    const float *gt;               // (B,G,4)
    const int *labels;             // (B,G)
    const unsigned char *difficult;   // (B,G) or null
    int M, G, C;
    float thr;
    long long slot0;               // images before this batch * M
    int2 *rec;                     // records: (score bits, class << 1 | tp; 0 = not counted)
    int *npos, *ndet;              // (C,)
    int *flags;                    // (B,M) or null
};

__global__ void __launch_bounds__(kEvThreads)
eval_match_kernel(EvalMatchArgs p)
{
    __shared__ __attribute__((aligned(16))) float gts[4 * kEvMaxG];
    __shared__ int gcode[kEvMaxG];                          // label << 1 | difficult; 0 = not a gt
    __shared__ unsigned long long claim[kEvMaxG];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int M = p.M, G = p.G, C = p.C;
    const float *gt = p.gt + 4 * (size_t)b * G;
    for (int g = tid; g < G; g += kEvThreads) {
        const int lab = p.labels[(size_t)b * G + g];
        const int diff = p.difficult ? (p.difficult[(size_t)b * G + g] != 0) : 0;
        store_box(gts + 4 * g, load_box(gt + 4 * (size_t)g));
        gcode[g] = lab >= 1 ? (int)(((unsigned)lab << 1) | (unsigned)diff) : 0;
        claim[g] = ~0ull;
        if (lab >= 1 && lab < C && !diff) atomicAdd(&p.npos[lab], 1);
    }
    __syncthreads();
    const int live = min(max(p.valid[b], 0), M);

    float score[kEvRows];
    int cls[kEvRows], jmax[kEvRows];                        // cls 0: dropped; jmax -1: false positive, -2: ignored (difficult gt)
#pragma unroll
    for (int u = 0; u < kEvRows; ++u) {
        const int m = tid + u * kEvThreads;
        score[u] = 0.0f;
        cls[u] = 0;
        jmax[u] = -1;
        if (m >= M) continue;
        const size_t row = (size_t)b * M + m;
        const float s = p.scores[row], cf = p.classes[row];
        score[u] = s;
        if (m >= live || !(cf >= 1.0f && cf < (float)C) || !(s > 0.0f && s < INFINITY)) continue;
        const int c = (int)cf;
        if ((float)c != cf) continue;
        cls[u] = c;
        const Box d = load_box(p.boxes + 4 * row);
        const float darea = box_area_plain(d);
        float best = -INFINITY;
        int j = -1;
        for (int g = 0; g < G; ++g) {
            if ((gcode[g] >> 1) != c) continue;
            const Box gb = load_box(gts + 4 * g);
            const float iou = iou_map_pair(d, darea, gb, box_area_plain(gb));
            if (iou > best) {                               // strict: the first maximum wins, a NaN never does
                best = iou;
                j = g;
            }
        }
        if (j >= 0 && best >= p.thr) {
            if (gcode[j] & 1) {
                jmax[u] = -2;
            } else {
                jmax[u] = j;
                atomicMin(&claim[j], ((unsigned long long)(~orderable(s)) << 12) | (unsigned long long)m);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kEvRows; ++u) {
        const int m = tid + u * kEvThreads;
        if (m >= M) continue;
        int flag = -1;
        if (cls[u] > 0 && jmax[u] != -2) {
            flag = 0;
            if (jmax[u] >= 0 && claim[jmax[u]] == (((unsigned long long)(~orderable(score[u])) << 12) | (unsigned long long)m)) flag = 1;
        }
        const size_t row = (size_t)b * M + m;
        p.rec[p.slot0 + (long long)row] = make_int2(__float_as_int(score[u]), flag < 0 ? 0 : ((cls[u] << 1) | flag));
        if (p.flags) p.flags[row] = flag;
        if (flag >= 0) atomicAdd(&p.ndet[cls[u]], 1);
    }
}

// ---- proposal recall --------------------------------------------------------------------------------------------------------
struct EvalRecallArgs {
    const float *rois;             // (B,R,4)
    const int *valid;              // (B,) or null
    const float *gt;
    const int *labels;
    const unsigned char *difficult;
    int R, G, n_k, n_t;
    int ks[kEvMaxCut];             // cut-offs, ascending
    int kidx[kEvMaxCut];           // their rows in the caller's order
    float thr[kEvMaxCut];
    unsigned long long *hits;      // (n_k, n_t)
    unsigned long long *n_gt;
};

__global__ void __launch_bounds__(kEvRecallThreads)
eval_recall_kernel(EvalRecallArgs p)
{
    __shared__ unsigned cnt[kEvMaxCut * kEvMaxCut + 1];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int R = p.R, G = p.G;
    if (tid <= kEvMaxCut * kEvMaxCut) cnt[tid] = 0u;
    __syncthreads();
    int live = R;
    if (p.valid) live = min(max(p.valid[b], 0), R);
    const float *rois = p.rois + 4 * (size_t)b * R;
    for (int g = tid; g < G; g += kEvRecallThreads) {
        const size_t gi = (size_t)b * G + g;
        if (p.labels[gi] < 1 || (p.difficult && p.difficult[gi] != 0)) continue;
        atomicAdd(&cnt[kEvMaxCut * kEvMaxCut], 1u);
        const Box gb = load_box(p.gt + 4 * gi);
        const float garea = box_area_plain(gb);
        float best = -INFINITY;                             // the maximum of no RoI reaches no threshold
        int r = 0;
        for (int i = 0; i < p.n_k; ++i) {
            const int lim = min(p.ks[i], live);
            for (; r < lim; ++r) {
                const Box rb = load_box(rois + 4 * (size_t)r);
                const float iou = iou_map_pair(rb, box_area_plain(rb), gb, garea);
                if (iou > best) best = iou;                 // a NaN never raises it
            }
            for (int t = 0; t < p.n_t; ++t)
                if (best >= p.thr[t]) atomicAdd(&cnt[p.kidx[i] * kEvMaxCut + t], 1u);
        }
    }
    __syncthreads();
    if (tid < kEvMaxCut * kEvMaxCut) {
        const int i = tid / kEvMaxCut, t = tid % kEvMaxCut;
        if (i < p.n_k && t < p.n_t && cnt[tid]) atomicAdd(&p.hits[i * p.n_t + t], (unsigned long long)cnt[tid]);
    } else if (tid == kEvMaxCut * kEvMaxCut && cnt[tid]) {
        atomicAdd(p.n_gt, (unsigned long long)cnt[tid]);
    }
}

// ---- per-class ranking and average precision --------------------------------------------------------------------------------
struct EvalClassArgs {
    const int2 *rec;
    long long n_rec;               // images * M
    const int *npos, *ndet;
    int c0;                        // class of workgroup 0
    uint2 *buf[2];                 // ping-pong workspace: (key, slot << 1 | tp), later (cumulative tp, slot << 1 | tp)
    int *parity;                   // (C,) which of the two holds class c's ranking
    double *ap, *ap11;             // (C,) or null
};

__global__ void __launch_bounds__(kEvThreads)
eval_class_kernel(EvalClassArgs p)
{
    __shared__ EvSortLds sort_lds;
    __shared__ double wmax[kEvWaves];
    __shared__ double p11[11];
    __shared__ double red[kEvThreads];
    int *const wsum = sort_lds.wsum;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = p.c0 + blockIdx.x;
    const int n = p.ndet[c], npos = p.npos[c];
    long long off = 0;
    for (int i = 0; i < c; ++i) off += p.ndet[i];

    // (1) this class's live records, in slot order, as (~orderable(score), slot << 1 | tp)
    uint2 *cur = p.buf[0] + off, *alt = p.buf[1] + off;
    ev_compact(
        p.rec, p.n_rec, cur, n, wsum, [c](const int2 &r) { return r.y != 0 && (r.y >> 1) == c; },
        [](const int2 &r, long long slot) {
            return make_uint2(~orderable(__int_as_float(r.x)), ((unsigned)slot << 1) | (unsigned)(r.y & 1));
        });
    // (2) stable LSD radix sort by the key, ascending: score descending, ties in slot order
    const int par = ev_radix_sort(cur, alt, n, sort_lds);
    if (tid == 0) p.parity[c] = par;
    if (!p.ap) return;

    // (3) cumulative TP over the ranking (written over the keys), then precision's reverse maximum and the two sums
    {
        int run = 0;
        for (int i0 = 0; i0 < n; i0 += kEvThreads) {
            const int i = i0 + tid;
            const bool tp = i < n && (cur[i].y & 1u);
            int total;
            const int excl = block_scan(tp ? 1 : 0, wsum, &total);
            if (i < n) cur[i].x = (unsigned)(run + excl + (tp ? 1 : 0));
            run += total;
        }
    }
    if (tid < 11) p11[tid] = 0.0;
    __syncthreads();
    double acc = 0.0, carry = 0.0;                           // carry: the maximum precision at every later rank (precisions are >= 0)
    const int ntiles = (n + kEvThreads - 1) / kEvThreads;
    for (int t = ntiles - 1; t >= 0; --t) {
        const int i = t * kEvThreads + tid;
        const bool valid = i < n;
        uint2 kv = make_uint2(0u, 0u);
        if (valid) kv = cur[i];
        const int tpc = (int)kv.x, tp = (int)(kv.y & 1u);
        double pm = valid ? (double)tpc / (double)(i + 1) : 0.0;
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
        if (valid) {
            if (tp) acc += pm;
            const long long now = 10ll * tpc, before = 10ll * (tpc - tp);
            for (int k = 0; k <= 10; ++k) {                 // the first rank with 10 tp >= k npos: the maximum from there on
                const long long need = (long long)k * npos;
                if (now >= need && (i == 0 || before < need)) p11[k] = pm;
            }
        }
        __syncthreads();
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kEvThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        double a = NAN, a11 = NAN;
        if (npos > 0) {
            a = red[0] / (double)npos;
            double s11 = 0.0;
            for (int k = 0; k <= 10; ++k) s11 += p11[k];
            a11 = s11 / 11.0;
        }
        p.ap[c] = a;
        p.ap11[c] = a11;
    }
}

__global__ void __launch_bounds__(256)
eval_finish_kernel(const int *__restrict__ npos, const int *__restrict__ ndet, int C, const unsigned long long *__restrict__ hits,
                   const unsigned long long *__restrict__ n_gt, int n_cut, int *__restrict__ out_npos, int *__restrict__ out_ndet,
                   double *__restrict__ out_recall, long long *__restrict__ out_n_gt)
{
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) {
        if (out_npos) out_npos[c] = npos[c];
        if (out_ndet) out_ndet[c] = ndet[c];
    }
    const unsigned long long ng = *n_gt;
    if (out_recall && tid < n_cut) out_recall[tid] = ng ? (double)hits[tid] / (double)ng : (double)NAN;
    if (out_n_gt && tid == 0) *out_n_gt = (long long)ng;
}

__global__ void __launch_bounds__(256)
eval_curve_kernel(const int2 *__restrict__ rec, const uint2 *__restrict__ buf0, const uint2 *__restrict__ buf1,
                  const int *__restrict__ parity, const int *__restrict__ ndet, int c, int cap, float *__restrict__ scores,
                  int *__restrict__ tp, int *__restrict__ slots, int *__restrict__ out_n)
{
    long long off = 0;
    for (int i = 0; i < c; ++i) off += ndet[i];
    const int n = ndet[c];
    const uint2 *src = (parity[c] ? buf1 : buf0) + off;
    const int lim = min(n, cap);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < lim; i += gridDim.x * 256) {
        const unsigned pay = src[i].y;
        const int slot = (int)(pay >> 1);
        scores[i] = __int_as_float(rec[slot].x);
        tp[i] = (int)(pay & 1u);
        slots[i] = slot;
    }
    if (out_n && blockIdx.x == 0 && threadIdx.x == 0) *out_n = n;
}

static bool ev_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace rpn

using namespace rpn;

struct rpn_evaluator {
    int C = 0, max_images = 0, M = 0;
    float thr = 0.5f;
    int n_k = 0, n_t = 0;
    int ks[kEvMaxCut] = {}, kidx[kEvMaxCut] = {};
    float rthr[kEvMaxCut] = {};
    int images = 0;
    // one allocation, made at creation
    unsigned char *d_mem = nullptr;
    size_t bytes = 0, counter_bytes = 0;
    int2 *rec = nullptr;
    uint2 *buf[2] = {nullptr, nullptr};
    unsigned char *counters = nullptr;     // everything reset() clears, contiguous
    int *npos = nullptr, *ndet = nullptr, *parity = nullptr;
    unsigned long long *hits = nullptr, *n_gt = nullptr;
};

// the section offsets of the handle's one allocation; returns its size
static size_t ev_layout(rpn_evaluator *e)
{
    const size_t n = (size_t)e->max_images * e->M;
    size_t o = 0;
    const size_t o_rec = o;
    o += a256(n * sizeof(int2));
    const size_t o_b0 = o;
    o += a256(n * sizeof(uint2));
    const size_t o_b1 = o;
    o += a256(n * sizeof(uint2));
    const size_t o_cnt = o;
    const size_t o_npos = o;
    o += a256((size_t)e->C * 4);
    const size_t o_ndet = o;
    o += a256((size_t)e->C * 4);
    const size_t o_par = o;
    o += a256((size_t)e->C * 4);
    const size_t o_hits = o;
    o += a256((size_t)(kEvMaxCut * kEvMaxCut + 1) * 8);
    e->counter_bytes = o - o_cnt;
    if (e->d_mem) {
        unsigned char *m = e->d_mem;
        e->rec = reinterpret_cast<int2 *>(m + o_rec);
        e->buf[0] = reinterpret_cast<uint2 *>(m + o_b0);
        e->buf[1] = reinterpret_cast<uint2 *>(m + o_b1);
        e->counters = m + o_cnt;
        e->npos = reinterpret_cast<int *>(m + o_npos);
        e->ndet = reinterpret_cast<int *>(m + o_ndet);
        e->parity = reinterpret_cast<int *>(m + o_par);
        e->hits = reinterpret_cast<unsigned long long *>(m + o_hits);
        e->n_gt = e->hits + kEvMaxCut * kEvMaxCut;
    }
    return o;
}

// Without a device at creation (argument checks and memory_bytes still work) the memory is allocated by the first call that finds one.
static int ev_ensure(rpn_evaluator *e)
{
    if (e->d_mem) return RPN_OK;
    RPN_REQUIRE_DEVICE();
    RPN_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&e->d_mem), e->bytes));
    ev_layout(e);
    // (once, at creation: the counters are zero before any stream, blocking or not, can touch them)
    RPN_HIP_CHECK(hipMemset(e->counters, 0, e->counter_bytes));
    RPN_HIP_CHECK(hipDeviceSynchronize());
    return RPN_OK;
}

extern "C" int rpn_evaluator_create(int C, int max_images, int M, float iou_threshold, const int *top_k, int n_k,
                                    const float *recall_iou, int n_t, rpn_evaluator **out)
{
    const char *who = "rpn_evaluator_create";
    RPN_REQUIRE(out, "%s: null pointer", who);
    *out = nullptr;
    RPN_REQUIRE(C >= 2 && C <= kEvMaxC, "%s: C = %d, must be in [2, %d]", who, C, kEvMaxC);
    RPN_REQUIRE(max_images >= 1 && M >= 1 && M <= kEvMaxM, "%s: max_images = %d, M = %d (1 <= M <= %d)", who, max_images, M, kEvMaxM);
    RPN_REQUIRE((long long)max_images * M <= (1ll << 30), "%s: max_images * M = %lld records, at most 2^30", who,
                (long long)max_images * M);
    RPN_REQUIRE(iou_threshold > 0.0f && iou_threshold <= 1.0f, "%s: iou_threshold = %g, must be in (0, 1]", who, (double)iou_threshold);
    RPN_REQUIRE(n_k >= 0 && n_k <= kEvMaxCut && n_t >= 0 && n_t <= kEvMaxCut, "%s: %d cut-offs and %d thresholds, at most %d each", who,
                n_k, n_t, kEvMaxCut);
    RPN_REQUIRE((n_k == 0 || top_k) && (n_t == 0 || recall_iou), "%s: null pointer", who);
    for (int i = 0; i < n_k; ++i) RPN_REQUIRE(top_k[i] >= 1, "%s: top_k[%d] = %d, must be >= 1", who, i, top_k[i]);
    for (int i = 0; i < n_t; ++i)
        RPN_REQUIRE(recall_iou[i] > 0.0f && recall_iou[i] <= 1.0f, "%s: recall_iou[%d] = %g, must be in (0, 1]", who, i,
                    (double)recall_iou[i]);
    rpn_evaluator *e = new (std::nothrow) rpn_evaluator();
    RPN_REQUIRE(e, "%s: out of host memory", who);
    e->C = C; e->max_images = max_images; e->M = M; e->thr = iou_threshold; e->n_k = n_k; e->n_t = n_t;
    for (int i = 0; i < n_k; ++i) e->kidx[i] = i;
    std::stable_sort(e->kidx, e->kidx + n_k, [&](int a, int b) { return top_k[a] < top_k[b]; });
    for (int i = 0; i < n_k; ++i) e->ks[i] = top_k[e->kidx[i]];
    for (int i = 0; i < n_t; ++i) e->rthr[i] = recall_iou[i];
    e->bytes = ev_layout(e);
    if (rpn_device_count() >= 1) {
        const int st = ev_ensure(e);
        if (st != RPN_OK) {
            delete e;
            return st;
        }
    }
    *out = e;
    return RPN_OK;
}

extern "C" void rpn_evaluator_destroy(rpn_evaluator *e)
{
    if (!e) return;
    if (e->d_mem) (void)hipFree(e->d_mem);
    delete e;
}

extern "C" int rpn_evaluator_memory_bytes(const rpn_evaluator *e, size_t *bytes)
{
    RPN_REQUIRE(e && bytes, "rpn_evaluator_memory_bytes: null pointer");
    *bytes = e->bytes;
    return RPN_OK;
}

extern "C" int rpn_evaluator_images(const rpn_evaluator *e) { return e ? e->images : 0; }

extern "C" int rpn_evaluator_reset(rpn_evaluator *e, void *stream)
{
    RPN_REQUIRE(e, "rpn_evaluator_reset: null pointer");
    const int st = ev_ensure(e);
    if (st != RPN_OK) return st;
    RPN_HIP_CHECK(hipMemsetAsync(e->counters, 0, e->counter_bytes, as_stream(stream)));
    e->images = 0;
    return RPN_OK;
}

extern "C" int rpn_evaluator_update(rpn_evaluator *e, const float *d_boxes, const float *d_scores, const float *d_classes,
                                    const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels,
                                    const unsigned char *d_gt_difficult, int B, int G, int32_t *d_flags, void *stream)
{
    const char *who = "rpn_evaluator_update";
    RPN_REQUIRE(e && d_boxes && d_scores && d_classes && d_valid && d_gt_boxes && d_gt_labels, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && G >= 1, "%s: B and G must be >= 1 (got %d, %d)", who, B, G);
    RPN_REQUIRE(G <= kEvMaxG, "%s: G = %d > %d", who, G, kEvMaxG);
    RPN_REQUIRE((long long)e->images + B <= e->max_images, "%s: %d images seen + %d > max_images = %d", who, e->images, B, e->max_images);
    RPN_REQUIRE(ev_aligned16(d_boxes) && ev_aligned16(d_gt_boxes), "%s: boxes and gt boxes must be 16-byte aligned", who);
    const int st = ev_ensure(e);
    if (st != RPN_OK) return st;
    EvalMatchArgs p{};
    p.boxes = d_boxes; p.scores = d_scores; p.classes = d_classes; p.valid = d_valid;
    p.gt = d_gt_boxes; p.labels = d_gt_labels; p.difficult = d_gt_difficult;
    p.M = e->M; p.G = G; p.C = e->C; p.thr = e->thr;
    p.slot0 = (long long)e->images * e->M;
    p.rec = e->rec; p.npos = e->npos; p.ndet = e->ndet; p.flags = d_flags;
    hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(kEvThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    e->images += B;
    return RPN_OK;
}

extern "C" int rpn_evaluator_update_proposals(rpn_evaluator *e, const float *d_rois, const int32_t *d_valid, int R,
                                              const float *d_gt_boxes, const int32_t *d_gt_labels,
                                              const unsigned char *d_gt_difficult, int B, int G, void *stream)
{
    const char *who = "rpn_evaluator_update_proposals";
    RPN_REQUIRE(e && d_rois && d_gt_boxes && d_gt_labels, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && R >= 1 && G >= 1, "%s: B, R and G must be >= 1 (got %d, %d, %d)", who, B, R, G);
    RPN_REQUIRE(G <= kEvMaxG, "%s: G = %d > %d", who, G, kEvMaxG);
    RPN_REQUIRE((long long)B * R < (1ll << 29), "%s: B * R = %lld RoIs do not fit one launch", who, (long long)B * R);
    RPN_REQUIRE(ev_aligned16(d_rois) && ev_aligned16(d_gt_boxes), "%s: rois and gt boxes must be 16-byte aligned", who);
    const int st = ev_ensure(e);
    if (st != RPN_OK) return st;
    EvalRecallArgs p{};
    p.rois = d_rois; p.valid = d_valid; p.gt = d_gt_boxes; p.labels = d_gt_labels; p.difficult = d_gt_difficult;
    p.R = R; p.G = G; p.n_k = e->n_k; p.n_t = e->n_t;
    for (int i = 0; i < kEvMaxCut; ++i) {
        p.ks[i] = e->ks[i];
        p.kidx[i] = e->kidx[i];
        p.thr[i] = e->rthr[i];
    }
    p.hits = e->hits; p.n_gt = e->n_gt;
    hipLaunchKernelGGL(eval_recall_kernel, dim3(B), dim3(kEvRecallThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

// the ranking of classes [c0, c0 + nc) into the workspace, with their APs when d_ap is given
static int ev_rank(rpn_evaluator *e, int c0, int nc, double *d_ap, double *d_ap11, hipStream_t s)
{
    EvalClassArgs p{};
    p.rec = e->rec;
    p.n_rec = (long long)e->images * e->M;
    p.npos = e->npos; p.ndet = e->ndet; p.c0 = c0;
    p.buf[0] = e->buf[0]; p.buf[1] = e->buf[1];
    p.parity = e->parity; p.ap = d_ap; p.ap11 = d_ap11;
    hipLaunchKernelGGL(eval_class_kernel, dim3(nc), dim3(kEvThreads), 0, s, p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" int rpn_evaluator_result(rpn_evaluator *e, double *d_ap, double *d_ap11, int32_t *d_npos, int32_t *d_ndet, double *d_recall,
                                    long long *d_n_gt, void *stream)
{
    const char *who = "rpn_evaluator_result";
    RPN_REQUIRE(e, "%s: null pointer", who);
    RPN_REQUIRE((d_ap != nullptr) == (d_ap11 != nullptr), "%s: d_ap and d_ap11 go together", who);
    int st = ev_ensure(e);
    if (st != RPN_OK) return st;
    hipStream_t s = as_stream(stream);
    if (d_ap) {
        st = ev_rank(e, 0, e->C, d_ap, d_ap11, s);
        if (st != RPN_OK) return st;
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(256), 0, s, e->npos, e->ndet, e->C, e->hits, e->n_gt, e->n_k * e->n_t, d_npos,
                       d_ndet, d_recall, d_n_gt);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" int rpn_evaluator_pr_curve(rpn_evaluator *e, int c, float *d_scores, int32_t *d_tp, int32_t *d_slots, int cap, int32_t *d_n,
                                      void *stream)
{
    const char *who = "rpn_evaluator_pr_curve";
    RPN_REQUIRE(e && d_scores && d_tp && d_slots, "%s: null pointer", who);
    RPN_REQUIRE(c >= 1 && c < e->C, "%s: class %d outside [1, %d)", who, c, e->C);
    RPN_REQUIRE(cap >= 0, "%s: cap = %d", who, cap);
    int st = ev_ensure(e);
    if (st != RPN_OK) return st;
    hipStream_t s = as_stream(stream);
    st = ev_rank(e, c, 1, nullptr, nullptr, s);
    if (st != RPN_OK) return st;
    const int grid = std::max(1, std::min((cap + 255) / 256, 1024));
    hipLaunchKernelGGL(eval_curve_kernel, dim3(grid), dim3(256), 0, s, e->rec, e->buf[0], e->buf[1], e->parity, e->ndet, c, cap, d_scores,
                       d_tp, d_slots, d_n);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}
