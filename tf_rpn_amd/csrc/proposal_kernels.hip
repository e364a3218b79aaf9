// proposal_kernels.hip -- the RPN proposal layer's filters in front of the NMS (contract: include/rpn_hip.h, rpn_proposal_filter):
// the minimum box size and the exact pre-NMS top-N, written as a MASK over the scores.  A dropped anchor's score becomes -inf,
// which rpn_decode_nms never takes for a candidate, so the tuned NMS kernel runs unchanged behind this pre-pass.
//
// One 1024-thread workgroup per image (images are independent; at most 61440 anchors each), three steps on the image's row:
//   mark   : score -> masked score (the score itself, or -inf when it fails the threshold or, with the size test, when its decoded
//            box is too small), candidates counted with integer adds (wave shuffle, one LDS atomic per wave).  The decode is
//            rpn_decode's: bbox_core.h's decode_box on deltas * variances, this file compiled with -ffp-contract=off like the
//            other box kernels.  It happens here ONCE; the passes below read 4 bytes per anchor and never call expf again.
//   select : only when more candidates than pre_nms_topn survive: radix_select.h on the NMS's own key, orderable(score) << 32 |
//            ~index, with cap == target (exact, as the RPN-target kernel uses it).  Up to six passes over the masked row (11-bit
//            digits of a 64-bit key); distinct scores need three or four, a cut inside a run of ties needs all six.
//   cut    : candidates whose key is below the selected one are overwritten with -inf.
// The masked OUTPUT row is the staging buffer of the passes (it is L2-resident: 240 KB per image at most), so the entry needs no
// workspace.  A thread reads back only elements it wrote itself (every loop walks i = tid + k * 1024).
// Bytes per image: mark reads 4 A (+ 32 A with the size test: anchors and deltas) and writes 4 A; each select pass reads 4 A;
// cut reads 4 A and writes 4 bytes per dropped candidate.  No floating-point atomics, no data-dependent order: same bits every run.
#include "bbox_core.h"
#include "radix_select.h"
#include "rpn_common.h"

#include <cmath>
#include <cstdint>

namespace rpn {

constexpr int kPfThreads = 1024;

struct ProposalFilterArgs {
    const float *anchors;     // (A,4); unused without the size test
    const float *deltas;      // (B,A,4); unused without the size test
    const float *scores;      // (B,A)
    float var[4];
    int var_enabled;
    int A;
    int topn;                 // <= 0: no cut
    float min_h, min_w;
    float score_thr;
    int clip;
    float *masked;            // (B,A)
    int *kept;                // (B,) or null
};

// the NMS's candidate key (nms_kernels.hip, make_key): 0 for a score that is not > thr (NaN included), else score order first,
// lower index first among equal scores
__device__ __forceinline__ unsigned long long proposal_key(float s, float thr, int i)
{
    if (!(s > thr)) return 0ull;
    return ((unsigned long long)orderable(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

template <bool MINSIZE>
__global__ void __launch_bounds__(kPfThreads)
proposal_filter_kernel(ProposalFilterArgs p)
{
    __shared__ unsigned hist[kRsHistWords];
    __shared__ int ctl[4];
    __shared__ int cand_total;
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x, A = p.A;
    const float *__restrict__ sc = p.scores + (size_t)b * A;
    float *mk = p.masked + (size_t)b * A;
    const float ninf = -INFINITY;
    if (tid == 0) cand_total = 0;
    __syncthreads();

    // ---- mark: 4 anchors per thread and trip, their loads issued together
    int cnt = 0;
    for (int base = tid; base < A; base += 4 * kPfThreads) {
        float s[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kPfThreads;
            s[u] = i < A ? sc[i] : ninf;
            ok[u] = s[u] > p.score_thr;                       // strict; false for NaN and for the padding lanes
        }
        if constexpr (MINSIZE) {
            Box an[4];
            float4 d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(base + u * kPfThreads, A - 1);          // padding lanes re-read the last anchor, result unused
                an[u] = load_box(p.anchors + 4 * (size_t)j);
                d[u] = *reinterpret_cast<const float4 *>(p.deltas + 4 * ((size_t)b * A + j));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float dy = d[u].x, dx = d[u].y, dh = d[u].z, dw = d[u].w;
                if (p.var_enabled) {
                    dy = dy * p.var[0];
                    dx = dx * p.var[1];
                    dh = dh * p.var[2];
                    dw = dw * p.var[3];
                }
                Box bx = decode_box(an[u], dy, dx, dh, dw);
                if (p.clip) {
                    bx.y1 = clip01(bx.y1);
                    bx.x1 = clip01(bx.x1);
                    bx.y2 = clip01(bx.y2);
                    bx.x2 = clip01(bx.x2);
                }
                const float h = bx.y2 - bx.y1, w = bx.x2 - bx.x1;
                ok[u] = ok[u] && h >= p.min_h && w >= p.min_w;            // a NaN side fails
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kPfThreads;
            if (i < A) mk[i] = ok[u] ? s[u] : ninf;
            cnt += ok[u] ? 1 : 0;
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0 && cnt != 0) atomicAdd(&cand_total, cnt);
    __syncthreads();
    int kept = cand_total;

    // ---- select + cut (workgroup-uniform condition)
    if (p.topn > 0 && kept > p.topn) {
        const float thr = p.score_thr;
        int count = 0;
        const unsigned long long kthr = radix_select<kPfThreads>([&](int i) { return proposal_key(mk[i], thr, i); }, A, ~0ull,
                                                                 p.topn, p.topn, hist, ctl, &count);
        for (int base = tid; base < A; base += 8 * kPfThreads) {
            float sb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * kPfThreads;
                sb[u] = i < A ? mk[i] : ninf;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * kPfThreads;
                const unsigned long long key = proposal_key(sb[u], thr, i);
                if (key != 0ull && key < kthr) mk[i] = ninf;              // (key != 0 implies i < A)
            }
        }
        kept = count;
    }
    if (tid == 0 && p.kept) p.kept[b] = kept;
}

}  // namespace rpn

using namespace rpn;

extern "C" size_t rpn_proposal_filter_workspace_bytes(int B, int A)
{
    (void)B;
    (void)A;
    return 0;       // the masked-score output row doubles as the staging buffer of the passes
}

extern "C" int rpn_proposal_filter(const float *d_anchors, const float *d_deltas, const float *variances, const float *d_scores,
                                   int B, int A, int pre_nms_topn, int use_min_size, float min_h, float min_w,
                                   float score_threshold, int clip_boxes, float *d_masked_scores, int32_t *d_kept,
                                   void *d_workspace, size_t workspace_bytes, void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    RPN_REQUIRE(B >= 0 && A >= 0, "rpn_proposal_filter: negative size");
    RPN_REQUIRE(A <= (1 << 30), "rpn_proposal_filter: %d anchors per image > 2^30", A);
    if (use_min_size)
        RPN_REQUIRE(min_h >= 0.0f && min_w >= 0.0f, "rpn_proposal_filter: min_size must be >= 0 and not NaN (min_h=%g, min_w=%g)",
                    (double)min_h, (double)min_w);
    if (B == 0) return RPN_OK;
    if (A > 0) {
        RPN_REQUIRE(d_scores && d_masked_scores, "rpn_proposal_filter: null score pointer");
        RPN_REQUIRE(!use_min_size || (d_anchors && d_deltas), "rpn_proposal_filter: the size test needs anchors and deltas");
        const uintptr_t bytes = (uintptr_t)B * (uintptr_t)A * sizeof(float);
        const uintptr_t in = (uintptr_t)d_scores, out = (uintptr_t)d_masked_scores;
        RPN_REQUIRE(out + bytes <= in || in + bytes <= out, "rpn_proposal_filter: d_masked_scores must not alias d_scores");
    } else if (!d_kept) {
        return RPN_OK;
    }
    RPN_REQUIRE_DEVICE();
    ProposalFilterArgs p{};
    p.anchors = d_anchors;
    p.deltas = d_deltas;
    p.scores = d_scores;
    if (variances) {
        for (int i = 0; i < 4; ++i) p.var[i] = variances[i];
        p.var_enabled = 1;
    }
    p.A = A;
    p.topn = pre_nms_topn;
    p.min_h = min_h;
    p.min_w = min_w;
    p.score_thr = score_threshold;
    p.clip = clip_boxes ? 1 : 0;
    p.masked = d_masked_scores;
    p.kept = d_kept;
    if (use_min_size && A > 0)
        hipLaunchKernelGGL(proposal_filter_kernel<true>, dim3((unsigned)B), dim3(kPfThreads), 0, as_stream(stream), p);
    else
        hipLaunchKernelGGL(proposal_filter_kernel<false>, dim3((unsigned)B), dim3(kPfThreads), 0, as_stream(stream), p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}
