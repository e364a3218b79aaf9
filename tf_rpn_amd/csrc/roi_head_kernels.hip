// roi_head_kernels.hip -- what a Faster R-CNN second stage needs around RoI pooling: which proposal trains on which ground-truth
// box (rpn_roi_targets), the detection head's two losses with their gradients (rpn_roi_losses), and head outputs -> per-class boxes
// and scores in front of the NMS (rpn_roi_decode_scores).  The second-stage counterparts of rpn_rpn_targets / rpn_rpn_losses /
// rpn_decode_nms.
//
// No reference counterpart: the reference stops at the proposals.  The thresholds and the sampling rule are this project's choice
// (the usual Faster R-CNN ones: IoU above 0.5 positive, [0.1, 0.5) negative, a fixed batch per image filled up with negatives), the
// box arithmetic is the reference's (bbox_core.h), and the subsampling is the one of its RPN targets (target_kernels.hip): exact top-K
// by an explicit random priority, ties to the lower index.
//
//   roi_target_kernel     : one 1024-thread workgroup per image.  The gt boxes, their areas and their validity are staged in LDS
//                           (1024 at a time); every thread walks its RoIs (r = tid, tid + 1024, ...) with max IoU / first argmax
//                           in registers and writes them to the (B,R) workspace; two radix selects (positives, then negatives) and
//                           the output pass follow in the same workgroup.  The (B,R,G) IoU map is never written; no memset, no
//                           atomics on global memory.
//                           HBM: 16 R + 20 G read, 8 R written and re-read (workspace, L2-resident), 8 R priorities read, 20 R
//                           written, per image.
//   roi_sample_kernel     : the proposal-target layer (rpn_roi_sample_targets): the same workgroup, matching pass and two selects
//                           over N = R (+ G with add_gt) candidates -- the RoIs, then the gt boxes themselves -- and, in place of
//                           the (B,R) output pass, an ordered workgroup scan (chunks of 1024 with a running offset; ballot +
//                           popcount inside a wave, 16 wave totals in LDS) that gives every kept candidate its row of a dense
//                           (B,S) batch: positives first, then negatives, each in ascending candidate index; the padding rows
//                           and the counts are written by the same kernel.  No atomics on global memory, no memset.
//                           HBM: 16 N + 20 G read, 8 N written and re-read (workspace, L2-resident), 8 N priorities read, 16 S
//                           kept boxes re-read, 40 S + 8 written, per image.
//   roi_loss_kernel       : one thread per RoI row: max, sum of exp and the cross-entropy of kept rows, the Huber sum of positive
//                           rows, all in float64; per-row (max, 1 / sum) to the workspace; block partials after a fixed LDS tree.
//   roi_loss_finish_kernel: the partials in a fixed tree -> [reg_loss, cls_loss] and the two gradient scales.
//   roi_loss_grad_kernel  : elementwise over (B R, C): grad_logits = (softmax - onehot) * scale, and the float4 of grad_reg that
//                           belongs to (row, class).  Both tensors written in full.
//                           HBM: 20 C + 20 read per row by the first kernel, 20 C read and 20 C written per row by the last.
//   roi_decode_scores_kernel : a workgroup per 64 rows: the rows' softmax statistics into LDS, then lanes over (row, class): one
//                           float4 of deltas in, one float4 box and one score out.  HBM: 20 C + 16 read, 20 C written per row.
// No floating-point atomics: every reduction has a fixed order, so every entry is bit-identical from run to run.  Compiled with
// -ffp-contract=off (same arithmetic as generate_iou_map / get_deltas_from_bboxes / get_bboxes_from_deltas).
#include <algorithm>
#include <cstdint>

#include "bbox_core.h"
#include "radix_select.h"
#include "rpn_common.h"

namespace rpn {

constexpr int kRoiTgtThreads = 1024;
constexpr int kRoiGtChunk = 1024;          // gt boxes staged in LDS at a time (one per thread)

struct RoiTargetArgs {
    const float *rois;        // (B,R,4)
    const int *valid;         // (B,) or null
    const float *gt;          // (B,G,4)
    const int *labels;        // (B,G), >= 1 = a gt box
    const int *rand_pos;      // (B,R) >= 1
    const int *rand_neg;      // (B,R) >= 1
    int R, G;
    int total_pos, total_neg;
    float var[4];
    float pos_iou, neg_lo, neg_hi;
    float *out_deltas;        // (B,R,4)
    int *out_labels;          // (B,R)
    // workspace
    float *best;              // (B,R) max IoU over the valid gt boxes (0 when none overlaps)
    int *arg;                 // (B,R) first argmax, -1 = none
};

__global__ void __launch_bounds__(kRoiTgtThreads)
roi_target_kernel(RoiTargetArgs p)
{
    __shared__ unsigned hist[kRsHistWords];
    __shared__ int ctl[8];
    __shared__ __attribute__((aligned(16))) float gts[4 * kRoiGtChunk];
    __shared__ float garea[kRoiGtChunk];
    __shared__ int gok[kRoiGtChunk];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int R = p.R, G = p.G;
    const float *rois = p.rois + 4 * (size_t)b * R;
    const float *gt = p.gt + 4 * (size_t)b * G;
    const int *glab = p.labels + (size_t)b * G;
    float *best = p.best + (size_t)b * R;
    int *arg = p.arg + (size_t)b * R;
    const int *rpos = p.rand_pos + (size_t)b * R, *rneg = p.rand_neg + (size_t)b * R;
    int live = R;                                           // rows r >= live are padding
    if (p.valid) live = min(max(p.valid[b], 0), R);

    // max IoU / first argmax of every live row over the valid gt boxes, in gt order
    for (int g0 = 0; g0 < G; g0 += kRoiGtChunk) {
        const int ng = min(kRoiGtChunk, G - g0);
        if (g0) __syncthreads();                            // the previous chunk has been read
        if (tid < ng) {
            const Box g = load_box(gt + 4 * (size_t)(g0 + tid));
            store_box(gts + 4 * tid, g);
            garea[tid] = box_area_plain(g);
            gok[tid] = glab[g0 + tid] >= 1;
        }
        __syncthreads();
        for (int r = tid; r < live; r += kRoiTgtThreads) {
            const Box bb = load_box(rois + 4 * (size_t)r);
            const float barea = box_area_plain(bb);
            float bi = 0.0f;
            int ai = -1;
            if (g0) { bi = best[r]; ai = arg[r]; }          // (this thread's own earlier writes)
            for (int g = 0; g < ng; ++g) {
                if (!gok[g]) continue;                      // workgroup-uniform
                const float iou = iou_map_pair(bb, barea, load_box(gts + 4 * g), garea[g]);
                if (iou > bi) {                             // strict: the first maximum wins, a NaN never does
                    bi = iou;
                    ai = g0 + g;
                }
            }
            best[r] = bi;
            arg[r] = ai;
        }
    }
    __syncthreads();

    auto key_pos = [&](int i) -> unsigned long long {
        const bool m = best[i] > p.pos_iou;
        return m ? (((unsigned long long)(unsigned)rpos[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
    };
    int pos_count = 0;
    unsigned long long thr_pos = 0ull;
    if (p.total_pos > 0)
        thr_pos = radix_select<kRoiTgtThreads>(key_pos, live, ~0ull, p.total_pos, p.total_pos, hist, ctl, &pos_count);
    if (thr_pos == 0ull) pos_count = 0;
    auto is_pos = [&](int i) -> bool {
        const unsigned long long k = key_pos(i);
        return thr_pos != 0ull && k != 0ull && k >= thr_pos;
    };
    const int neg_want = p.total_pos + p.total_neg - pos_count;          // the batch fills up with negatives
    auto key_neg = [&](int i) -> unsigned long long {
        const float v = best[i];
        const bool m = v >= p.neg_lo && v < p.neg_hi && !is_pos(i);
        return m ? (((unsigned long long)(unsigned)rneg[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
    };
    int neg_count = 0;
    unsigned long long thr_neg = 0ull;
    if (neg_want > 0) thr_neg = radix_select<kRoiTgtThreads>(key_neg, live, ~0ull, neg_want, neg_want, hist, ctl, &neg_count);

    for (int i = tid; i < R; i += kRoiTgtThreads) {
        int lab = -1;
        float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < live) {
            if (is_pos(i)) {
                const int a = arg[i];                       // best > pos_iou >= 0: some gt set it
                lab = glab[a];
                d = encode_box(load_box(rois + 4 * (size_t)i), load_box(gt + 4 * (size_t)a));
                d.x = d.x / p.var[0];
                d.y = d.y / p.var[1];
                d.z = d.z / p.var[2];
                d.w = d.w / p.var[3];
            } else {
                const unsigned long long kn = key_neg(i);
                if (thr_neg != 0ull && kn != 0ull && kn >= thr_neg) lab = 0;
            }
        }
        p.out_labels[(size_t)b * R + i] = lab;
        *reinterpret_cast<float4 *>(p.out_deltas + 4 * ((size_t)b * R + i)) = d;
    }
}

// ---- sampled targets: the proposal-target layer ------------------------------------------------------------------------------
struct RoiSampleArgs {
    const float *rois;        // (B,R,4)
    const int *valid;         // (B,) or null
    const float *gt;          // (B,G,4)
    const int *labels;        // (B,G), >= 1 = a gt box
    const int *rand_pos;      // (B,N) >= 1
    const int *rand_neg;      // (B,N) >= 1
    int R, G, N, S;           // N = add_gt ? R + G : R candidates, S = total_pos + total_neg output rows
    int add_gt;
    int total_pos, total_neg;
    float var[4];
    float pos_iou, neg_lo, neg_hi;
    float *out_rois;          // (B,S,4)
    float *out_deltas;        // (B,S,4)
    int *out_labels;          // (B,S)
    int *out_index;           // (B,S)
    int *out_counts;          // (B,2)
    // workspace
    float *best;              // (B,N) max IoU over the valid gt boxes (0 when none overlaps, NaN for a candidate that is not live)
    int *arg;                 // (B,N) first argmax, -1 = none
};

// roi_target_kernel's matching and selection over the N candidates (RoIs, then the gt boxes), then the kept candidates written as a
// dense batch.  The matching loop and the two selects are roi_target_kernel's, statement for statement (that kernel is left as it
// was); what differs is where a candidate's box comes from, how a dead candidate is kept out, and the output pass.
__global__ void __launch_bounds__(kRoiTgtThreads)
roi_sample_kernel(RoiSampleArgs p)
{
    __shared__ unsigned hist[kRsHistWords];
    __shared__ int ctl[8];
    __shared__ __attribute__((aligned(16))) float gts[4 * kRoiGtChunk];
    __shared__ float garea[kRoiGtChunk];
    __shared__ int gok[kRoiGtChunk];
    __shared__ int wsum[2][kRoiTgtThreads / 64];            // the scan's wave totals, two chunks in flight
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int R = p.R, G = p.G, N = p.N, S = p.S;
    const float *rois = p.rois + 4 * (size_t)b * R;
    const float *gt = p.gt + 4 * (size_t)b * G;
    const int *glab = p.labels + (size_t)b * G;
    float *best = p.best + (size_t)b * N;
    int *arg = p.arg + (size_t)b * N;
    const int *rpos = p.rand_pos + (size_t)b * N, *rneg = p.rand_neg + (size_t)b * N;
    int live = R;                                           // RoI rows r >= live are padding
    if (p.valid) live = min(max(p.valid[b], 0), R);
    const int n = p.add_gt ? N : live;                      // candidates i >= n are dead and never looked at
    auto box_of = [&](int i) -> const float * { return i < R ? rois + 4 * (size_t)i : gt + 4 * (size_t)(i - R); };

    // max IoU / first argmax of every live candidate over the valid gt boxes, in gt order.  A dead candidate (a padding RoI in front
    // of the gt candidates, a gt row that is no gt) gets best = NaN: a NaN is above no threshold and inside no interval, so neither
    // select below can take it; a live candidate's best starts at 0 and is only replaced by a larger IoU, so it is never NaN.
    for (int g0 = 0; g0 < G; g0 += kRoiGtChunk) {
        const int ng = min(kRoiGtChunk, G - g0);
        if (g0) __syncthreads();                            // the previous chunk has been read
        if (tid < ng) {
            const Box g = load_box(gt + 4 * (size_t)(g0 + tid));
            store_box(gts + 4 * tid, g);
            garea[tid] = box_area_plain(g);
            gok[tid] = glab[g0 + tid] >= 1;
        }
        __syncthreads();
        for (int i = tid; i < n; i += kRoiTgtThreads) {
            const bool alive = i < R ? i < live : glab[i - R] >= 1;
            if (!alive) {
                best[i] = __builtin_nanf("");
                arg[i] = -1;
                continue;
            }
            const Box bb = load_box(box_of(i));
            const float barea = box_area_plain(bb);
            float bi = 0.0f;
            int ai = -1;
            if (g0) { bi = best[i]; ai = arg[i]; }          // (this thread's own earlier writes)
            for (int g = 0; g < ng; ++g) {
                if (!gok[g]) continue;                      // workgroup-uniform
                const float iou = iou_map_pair(bb, barea, load_box(gts + 4 * g), garea[g]);
                if (iou > bi) {                             // strict: the first maximum wins, a NaN never does
                    bi = iou;
                    ai = g0 + g;
                }
            }
            best[i] = bi;
            arg[i] = ai;
        }
    }
    __syncthreads();

    auto key_pos = [&](int i) -> unsigned long long {
        const bool m = best[i] > p.pos_iou;
        return m ? (((unsigned long long)(unsigned)rpos[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
    };
    int pos_count = 0;
    unsigned long long thr_pos = 0ull;
    if (p.total_pos > 0)
        thr_pos = radix_select<kRoiTgtThreads>(key_pos, n, ~0ull, p.total_pos, p.total_pos, hist, ctl, &pos_count);
    if (thr_pos == 0ull) pos_count = 0;
    auto is_pos = [&](int i) -> bool {
        const unsigned long long k = key_pos(i);
        return thr_pos != 0ull && k != 0ull && k >= thr_pos;
    };
    const int neg_want = p.total_pos + p.total_neg - pos_count;          // the batch fills up with negatives
    auto key_neg = [&](int i) -> unsigned long long {
        const float v = best[i];
        const bool m = v >= p.neg_lo && v < p.neg_hi && !is_pos(i);
        return m ? (((unsigned long long)(unsigned)rneg[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i)) : 0ull;
    };
    int neg_count = 0;
    unsigned long long thr_neg = 0ull;
    if (neg_want > 0) thr_neg = radix_select<kRoiTgtThreads>(key_neg, n, ~0ull, neg_want, neg_want, hist, ctl, &neg_count);
    if (thr_neg == 0ull) neg_count = 0;
    auto is_neg = [&](int i) -> bool {
        const unsigned long long k = key_neg(i);
        return thr_neg != 0ull && k != 0ull && k >= thr_neg;
    };

    float *orois = p.out_rois + 4 * (size_t)b * S, *odeltas = p.out_deltas + 4 * (size_t)b * S;
    int *olabels = p.out_labels + (size_t)b * S, *oindex = p.out_index + (size_t)b * S;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int lane = tid & 63, wave = tid >> 6;
    int turn = 0;                                           // which half of wsum the next chunk uses
    // Ordered compaction: the candidates in chunks of 1024 with a running offset; inside a chunk a kept candidate's row is the
    // number of kept candidates in front of it: the lanes below it in its wave (ballot + popcount, the wave scan of a 0/1 flag) plus
    // the totals of the waves below (16 partials in LDS).  One barrier per chunk: consecutive chunks alternate between the halves
    // of wsum, and a wave can be at most one chunk ahead of the slowest.
    auto compact = [&](auto kept, bool positive, int row0) {
        int run = row0;
        for (int c0 = 0; c0 < n; c0 += kRoiTgtThreads, turn ^= 1) {
            const int i = c0 + tid;
            const bool k = i < n && kept(i);
            const unsigned long long mask = __ballot(k);
            if (lane == 0) wsum[turn][wave] = __popcll(mask);
            __syncthreads();
            int below = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kRoiTgtThreads / 64; ++w) {
                const int t = wsum[turn][w];
                below += w < wave ? t : 0;
                total += t;
            }
            const int s = run + below + __popcll(mask & ((1ull << lane) - 1ull));
            if (k && s < S) {                               // (s < S always: the selects keep at most S; a guard, not a path)
                const float4 box = *reinterpret_cast<const float4 *>(box_of(i));
                int lab = 0;
                float4 d = zero4;
                if (positive) {
                    const int a = arg[i];                   // best > pos_iou >= 0: some gt set it
                    lab = glab[a];
                    d = encode_box(Box{box.x, box.y, box.z, box.w}, load_box(gt + 4 * (size_t)a));
                    d.x = d.x / p.var[0];
                    d.y = d.y / p.var[1];
                    d.z = d.z / p.var[2];
                    d.w = d.w / p.var[3];
                }
                *reinterpret_cast<float4 *>(orois + 4 * (size_t)s) = box;
                *reinterpret_cast<float4 *>(odeltas + 4 * (size_t)s) = d;
                olabels[s] = lab;
                oindex[s] = i;
            }
            run += total;
        }
    };
    compact(is_pos, true, 0);
    compact(is_neg, false, pos_count);
    const int n_sampled = pos_count + neg_count;
    for (int s = n_sampled + tid; s < S; s += kRoiTgtThreads) {          // padding rows
        *reinterpret_cast<float4 *>(orois + 4 * (size_t)s) = zero4;
        *reinterpret_cast<float4 *>(odeltas + 4 * (size_t)s) = zero4;
        olabels[s] = -1;
        oindex[s] = -1;
    }
    if (tid == 0) {
        p.out_counts[2 * b] = n_sampled;
        p.out_counts[2 * b + 1] = pos_count;
    }
}

// ---- losses -----------------------------------------------------------------------------------------------------------------
constexpr int kRoiLossThreads = 256;
constexpr int kRoiLossMaxBlocks = 512;

__device__ __forceinline__ double4 roi_block_sum(double4 v, double4 *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kRoiLossThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double4 a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = make_double4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        __syncthreads();
    }
    return red[0];
}

// rowstat[row] = (max logit, 1 / sum exp(logit - max)); part[block] = (reg sum, cls sum, n_pos, n_kept)
__global__ void __launch_bounds__(kRoiLossThreads)
roi_loss_kernel(const float *__restrict__ logits, const float *__restrict__ reg_pred, const int *__restrict__ labels,
                const float4 *__restrict__ deltas, long long n, int C, float2 *__restrict__ rowstat, double4 *__restrict__ part)
{
    __shared__ double4 red[kRoiLossThreads];
    double reg = 0.0, cls = 0.0, npos = 0.0, nkept = 0.0;
    for (long long i = (long long)blockIdx.x * kRoiLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kRoiLossThreads) {
        const int lab = labels[i];
        const bool kept = lab >= 0 && lab < C;               // anything else is ignored and never indexes memory
        if (!kept && !rowstat) continue;
        const float *l = logits + i * C;
        float m = l[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += exp((double)l[c] - (double)m);
        if (rowstat) rowstat[i] = make_float2(m, (float)(1.0 / s));
        if (!kept) continue;
        cls += ((double)m + log(s)) - (double)l[lab];
        nkept += 1.0;
        if (lab >= 1) {
            const float4 p = *reinterpret_cast<const float4 *>(reg_pred + (i * C + lab) * 4), t = deltas[i];
            const double d[4] = {(double)p.x - t.x, (double)p.y - t.y, (double)p.z - t.z, (double)p.w - t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double a = fabs(d[k]), q = fmin(a, 1.0);
                reg += 0.5 * q * q + (a - q);
            }
            npos += 1.0;
        }
    }
    const double4 t = roi_block_sum(make_double4(reg, cls, npos, nkept), red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// out = [reg_loss, cls_loss]; scale = {1 / max(1, n_pos), 1 / max(1, n_kept)}.  An empty sum is 0, so is its loss: no NaN.
__global__ void __launch_bounds__(kRoiLossThreads)
roi_loss_finish_kernel(const double4 *__restrict__ part, int nparts, float *__restrict__ out, float *__restrict__ scale)
{
    __shared__ double4 red[kRoiLossThreads];
    double4 s = make_double4(0.0, 0.0, 0.0, 0.0);
    for (int i = threadIdx.x; i < nparts; i += kRoiLossThreads) {
        const double4 a = part[i];
        s = make_double4(s.x + a.x, s.y + a.y, s.z + a.z, s.w + a.w);
    }
    const double4 t = roi_block_sum(s, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(t.x / fmax(1.0, t.z));
        out[1] = (float)(t.y / fmax(1.0, t.w));
        scale[0] = (float)(1.0 / fmax(1.0, t.z));
        scale[1] = (float)(1.0 / fmax(1.0, t.w));
    }
}

// one element per (row, class): its grad_logits value and its float4 of grad_reg
__global__ void __launch_bounds__(256)
roi_loss_grad_kernel(const float *__restrict__ logits, const float *__restrict__ reg_pred, const int *__restrict__ labels,
                     const float4 *__restrict__ deltas, long long n, int C, const float2 *__restrict__ rowstat,
                     const float *__restrict__ scale, float *__restrict__ g_logits, float4 *__restrict__ g_reg)
{
    const float sr = scale[0], sc = scale[1];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n * C; e += (long long)gridDim.x * 256) {
        const long long row = e / C;
        const int c = (int)(e - row * C);
        const int lab = labels[row];
        const bool kept = lab >= 0 && lab < C;
        if (g_logits) {
            float g = 0.0f;
            if (kept) {
                const float2 st = rowstat[row];
                g = (expf(logits[e] - st.x) * st.y - (c == lab ? 1.0f : 0.0f)) * sc;
            }
            g_logits[e] = g;
        }
        if (g_reg) {
            float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (kept && lab >= 1 && c == lab) {
                const float4 p = *reinterpret_cast<const float4 *>(reg_pred + e * 4), t = deltas[row];
                g.x = fmaxf(-1.0f, fminf(1.0f, p.x - t.x)) * sr;
                g.y = fmaxf(-1.0f, fminf(1.0f, p.y - t.y)) * sr;
                g.z = fmaxf(-1.0f, fminf(1.0f, p.z - t.z)) * sr;
                g.w = fmaxf(-1.0f, fminf(1.0f, p.w - t.w)) * sr;
            }
            g_reg[e] = g;
        }
    }
}

// ---- head outputs -> per-class boxes and scores -----------------------------------------------------------------------------
constexpr int kRoiDecRows = 64;            // rows per workgroup

struct RoiVar {
    float v[4];
};

__global__ void __launch_bounds__(256)
roi_decode_scores_kernel(const float *__restrict__ rois, const int *__restrict__ valid, const float4 *__restrict__ reg_pred,
                         const float *__restrict__ logits, RoiVar var, long long n, int R, int C, float4 *__restrict__ boxes,
                         float *__restrict__ scores)
{
    __shared__ float2 stat[kRoiDecRows];                    // (max, 1 / sum exp), (0, 0) for a padding row
    const long long row0 = (long long)blockIdx.x * kRoiDecRows;
    const int nrows = (int)min((long long)kRoiDecRows, n - row0);
    if ((int)threadIdx.x < nrows) {
        const long long row = row0 + threadIdx.x;
        const int b = (int)(row / R), r = (int)(row - (long long)b * R);
        float2 st = make_float2(0.0f, 0.0f);
        if (!valid || r < valid[b]) {
            const float *l = logits + row * C;
            float m = l[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += exp((double)l[c] - (double)m);
            st = make_float2(m, (float)(1.0 / s));
        }
        stat[threadIdx.x] = st;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nrows * C; e += 256) {
        const int lr = e / C, c = e - lr * C;
        const long long row = row0 + lr, i = row * C + c;
        const float4 d = reg_pred[i];
        store_box(reinterpret_cast<float *>(boxes + i),
                  decode_box(load_box(rois + 4 * row), d.x * var.v[0], d.y * var.v[1], d.z * var.v[2], d.w * var.v[3]));
        const float2 st = stat[lr];
        // background and padding rows: exactly 0 (st.y == 0 marks a padding row; a live row's 1 / sum is at least 1 / C)
        scores[i] = (c >= 1 && st.y != 0.0f) ? expf(logits[i] - st.x) * st.y : 0.0f;
    }
}

static bool rh_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static int roi_loss_blocks(long long n)
{
    return (int)std::max<long long>(1, std::min<long long>((n + kRoiLossThreads - 1) / kRoiLossThreads, kRoiLossMaxBlocks));
}

}  // namespace rpn

using namespace rpn;

extern "C" size_t rpn_roi_targets_workspace_bytes(int B, int R, int G)
{
    if (B <= 0 || R <= 0 || G <= 0) return 0;
    return 2 * a256((size_t)B * R * 4);
}

extern "C" int rpn_roi_targets(const float *d_rois, const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels, int B,
                               int R, int G, int total_pos, int total_neg, float pos_iou, float neg_lo, float neg_hi,
                               const float *variances, const int32_t *d_random_pos, const int32_t *d_random_neg, float *d_roi_deltas,
                               int32_t *d_roi_labels, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "rpn_roi_targets";
    RPN_REQUIRE(d_rois && d_gt_boxes && d_gt_labels && variances && d_random_pos && d_random_neg && d_roi_deltas && d_roi_labels,
                "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && R >= 1 && G >= 1, "%s: B, R and G must be >= 1 (got %d, %d, %d)", who, B, R, G);
    RPN_REQUIRE(G <= 2048, "%s: G = %d > 2048", who, G);
    RPN_REQUIRE((long long)B * R < (1ll << 31), "%s: B * R = %lld RoIs do not fit one launch", who, (long long)B * R);
    RPN_REQUIRE(total_pos >= 0 && total_neg >= 0 && (long long)total_pos + total_neg < (1ll << 31),
                "%s: total_pos = %d, total_neg = %d", who, total_pos, total_neg);
    RPN_REQUIRE(neg_lo >= 0.0f && neg_lo <= neg_hi && pos_iou >= 0.0f,
                "%s: thresholds need 0 <= neg_lo <= neg_hi and pos_iou >= 0 (got neg_lo %g, neg_hi %g, pos_iou %g)", who, (double)neg_lo,
                (double)neg_hi, (double)pos_iou);
    RPN_REQUIRE(rh_aligned16(d_rois) && rh_aligned16(d_gt_boxes) && rh_aligned16(d_roi_deltas),
                "%s: rois, gt boxes and deltas must be 16-byte aligned", who);
    const size_t need = rpn_roi_targets_workspace_bytes(B, R, G);
    if (!d_workspace || workspace_bytes < need)
        return fail(RPN_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    RPN_REQUIRE_DEVICE();
    RoiTargetArgs p{};
    p.rois = d_rois; p.valid = d_valid; p.gt = d_gt_boxes; p.labels = d_gt_labels;
    p.rand_pos = d_random_pos; p.rand_neg = d_random_neg;
    p.R = R; p.G = G; p.total_pos = total_pos; p.total_neg = total_neg;
    for (int i = 0; i < 4; ++i) p.var[i] = variances[i];
    p.pos_iou = pos_iou; p.neg_lo = neg_lo; p.neg_hi = neg_hi;
    p.out_deltas = d_roi_deltas; p.out_labels = d_roi_labels;
    p.best = reinterpret_cast<float *>(d_workspace);
    p.arg = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(d_workspace) + a256((size_t)B * R * 4));
    hipLaunchKernelGGL(roi_target_kernel, dim3(B), dim3(kRoiTgtThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" size_t rpn_roi_sample_targets_workspace_bytes(int B, int R, int G, int add_gt)
{
    if (B <= 0 || R <= 0 || G <= 0) return 0;
    return 2 * a256((size_t)B * ((size_t)R + (add_gt ? G : 0)) * 4);
}

extern "C" int rpn_roi_sample_targets(const float *d_rois, const int32_t *d_valid, const float *d_gt_boxes, const int32_t *d_gt_labels,
                                      int B, int R, int G, int add_gt, int total_pos, int total_neg, float pos_iou, float neg_lo,
                                      float neg_hi, const float *variances, const int32_t *d_random_pos, const int32_t *d_random_neg,
                                      int S, float *d_out_rois, int32_t *d_out_labels, float *d_out_deltas, int32_t *d_out_index,
                                      int32_t *d_out_counts, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "rpn_roi_sample_targets";
    RPN_REQUIRE(d_rois && d_gt_boxes && d_gt_labels && variances && d_random_pos && d_random_neg && d_out_rois && d_out_labels &&
                    d_out_deltas && d_out_index && d_out_counts,
                "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && R >= 1 && G >= 1, "%s: B, R and G must be >= 1 (got %d, %d, %d)", who, B, R, G);
    RPN_REQUIRE(G <= 2048, "%s: G = %d > 2048", who, G);
    const long long N = (long long)R + (add_gt ? G : 0);
    RPN_REQUIRE((long long)B * N < (1ll << 31), "%s: B * N = %lld candidates do not fit one launch", who, (long long)B * N);
    RPN_REQUIRE(total_pos >= 0 && total_neg >= 0 && (long long)total_pos + total_neg < (1ll << 31),
                "%s: total_pos = %d, total_neg = %d", who, total_pos, total_neg);
    RPN_REQUIRE(S >= 1 && (long long)S == (long long)total_pos + total_neg, "%s: S = %d must be total_pos + total_neg = %lld and >= 1",
                who, S, (long long)total_pos + total_neg);
    RPN_REQUIRE((long long)B * S < (1ll << 31), "%s: B * S = %lld rows do not fit one launch", who, (long long)B * S);
    RPN_REQUIRE(neg_lo >= 0.0f && neg_lo <= neg_hi && pos_iou >= 0.0f,
                "%s: thresholds need 0 <= neg_lo <= neg_hi and pos_iou >= 0 (got neg_lo %g, neg_hi %g, pos_iou %g)", who, (double)neg_lo,
                (double)neg_hi, (double)pos_iou);
    RPN_REQUIRE(rh_aligned16(d_rois) && rh_aligned16(d_gt_boxes) && rh_aligned16(d_out_rois) && rh_aligned16(d_out_deltas),
                "%s: rois, gt boxes, out_rois and out_deltas must be 16-byte aligned", who);
    const size_t need = rpn_roi_sample_targets_workspace_bytes(B, R, G, add_gt);
    if (!d_workspace || workspace_bytes < need)
        return fail(RPN_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    RPN_REQUIRE_DEVICE();
    RoiSampleArgs p{};
    p.rois = d_rois; p.valid = d_valid; p.gt = d_gt_boxes; p.labels = d_gt_labels;
    p.rand_pos = d_random_pos; p.rand_neg = d_random_neg;
    p.R = R; p.G = G; p.N = (int)N; p.S = S; p.add_gt = add_gt ? 1 : 0; p.total_pos = total_pos; p.total_neg = total_neg;
    for (int i = 0; i < 4; ++i) p.var[i] = variances[i];
    p.pos_iou = pos_iou; p.neg_lo = neg_lo; p.neg_hi = neg_hi;
    p.out_rois = d_out_rois; p.out_deltas = d_out_deltas; p.out_labels = d_out_labels; p.out_index = d_out_index;
    p.out_counts = d_out_counts;
    p.best = reinterpret_cast<float *>(d_workspace);
    p.arg = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(d_workspace) + a256((size_t)B * N * 4));
    hipLaunchKernelGGL(roi_sample_kernel, dim3(B), dim3(kRoiTgtThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}

extern "C" size_t rpn_roi_losses_workspace_bytes(int B, int R, int C)
{
    if (B <= 0 || R <= 0 || C <= 0) return 0;
    const long long n = (long long)B * R;
    return a256((size_t)roi_loss_blocks(n) * sizeof(double4)) + 256 + a256((size_t)n * sizeof(float2));
}

extern "C" int rpn_roi_losses(const float *d_cls_logits, const float *d_reg_pred, const int32_t *d_roi_labels, const float *d_roi_deltas,
                              int B, int R, int C, float *d_losses, float *d_grad_logits, float *d_grad_reg, void *d_workspace,
                              size_t workspace_bytes, void *stream)
{
    const char *who = "rpn_roi_losses";
    RPN_REQUIRE(d_cls_logits && d_reg_pred && d_roi_labels && d_roi_deltas && d_losses, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && R >= 1 && C >= 1, "%s: B, R and C must be >= 1 (got %d, %d, %d)", who, B, R, C);
    RPN_REQUIRE((long long)B * R < (1ll << 31), "%s: B * R = %lld rows do not fit one launch", who, (long long)B * R);
    RPN_REQUIRE(rh_aligned16(d_reg_pred) && rh_aligned16(d_roi_deltas) && rh_aligned16(d_grad_reg),
                "%s: reg_pred, roi_deltas and grad_reg must be 16-byte aligned", who);
    const size_t need = rpn_roi_losses_workspace_bytes(B, R, C);
    if (!d_workspace || workspace_bytes < need)
        return fail(RPN_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    RPN_REQUIRE_DEVICE();
    hipStream_t s = as_stream(stream);
    const long long n = (long long)B * R;
    const int nb = roi_loss_blocks(n);
    unsigned char *ws = reinterpret_cast<unsigned char *>(d_workspace);
    double4 *part = reinterpret_cast<double4 *>(ws);
    float *scale = reinterpret_cast<float *>(ws + a256((size_t)nb * sizeof(double4)));
    float2 *rowstat = reinterpret_cast<float2 *>(ws + a256((size_t)nb * sizeof(double4)) + 256);
    const float4 *deltas = reinterpret_cast<const float4 *>(d_roi_deltas);
    hipLaunchKernelGGL(roi_loss_kernel, dim3(nb), dim3(kRoiLossThreads), 0, s, d_cls_logits, d_reg_pred, d_roi_labels, deltas, n, C,
                       d_grad_logits ? rowstat : nullptr, part);
    RPN_CHECK_LAUNCH();
    hipLaunchKernelGGL(roi_loss_finish_kernel, dim3(1), dim3(kRoiLossThreads), 0, s, part, nb, d_losses, scale);
    RPN_CHECK_LAUNCH();
    if (d_grad_logits || d_grad_reg) {
        const int grid = (int)std::max<long long>(1, std::min<long long>((n * C + 255) / 256, 4096));
        hipLaunchKernelGGL(roi_loss_grad_kernel, dim3(grid), dim3(256), 0, s, d_cls_logits, d_reg_pred, d_roi_labels, deltas, n, C, rowstat,
                           scale, d_grad_logits, reinterpret_cast<float4 *>(d_grad_reg));
        RPN_CHECK_LAUNCH();
    }
    return RPN_OK;
}

extern "C" int rpn_roi_decode_scores(const float *d_rois, const int32_t *d_valid, const float *d_reg_pred, const float *d_cls_logits,
                                     const float *variances, int B, int R, int C, float *d_boxes, float *d_scores, void *stream)
{
    const char *who = "rpn_roi_decode_scores";
    RPN_REQUIRE(d_rois && d_reg_pred && d_cls_logits && variances && d_boxes && d_scores, "%s: null pointer", who);
    RPN_REQUIRE(B >= 1 && R >= 1 && C >= 1, "%s: B, R and C must be >= 1 (got %d, %d, %d)", who, B, R, C);
    RPN_REQUIRE((long long)B * R < (1ll << 31), "%s: B * R = %lld rows do not fit one launch", who, (long long)B * R);
    RPN_REQUIRE(rh_aligned16(d_rois) && rh_aligned16(d_reg_pred) && rh_aligned16(d_boxes),
                "%s: rois, reg_pred and boxes must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const long long n = (long long)B * R;
    RoiVar var;
    for (int i = 0; i < 4; ++i) var.v[i] = variances[i];
    hipLaunchKernelGGL(roi_decode_scores_kernel, dim3((unsigned)((n + kRoiDecRows - 1) / kRoiDecRows)), dim3(256), 0, as_stream(stream),
                       d_rois, d_valid, reinterpret_cast<const float4 *>(d_reg_pred), d_cls_logits, var, n, R, C,
                       reinterpret_cast<float4 *>(d_boxes), d_scores);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}
