// soft_nms_kernels.hip -- Soft-NMS (Bodla et al. 2017; TensorFlow's soft_nms_sigma) for the second stage's detections.
//
// The contract is stated in include/rpn_hip.h (rpn_soft_nms).  Two launches:
//
//   soft_select_kernel<METHOD>   one 256-thread workgroup per (image, class) pair.  The candidates (score > thr) are compacted into
//                                LDS in ascending row order (ballot + ordered scan, one barrier per 256 rows), then the greedy
//                                loop runs: every thread decays its strided share of the live candidates against the box just
//                                selected and, in the same sweep, keeps the best (score, row) it saw; a wave reduction and one
//                                exchange through LDS elect the next box.  A thread only ever writes the scores of its own
//                                candidates, so the exchange (double-buffered) is the only barrier of a selection.
//   soft_join_kernel             one workgroup per image merges the C per-class lists of (row, decayed score).  Every list is
//                                non-increasing, so an entry's place in the merged order is its own rank plus, per foreign
//                                list, a count found by binary search -- no sort.
//
// No floating-point atomics, fixed orders: the same bits on every run, and an image's result depends on that image alone.
// Compiled with -ffp-contract=off: the IoU is bbox_core.h's nms_iou, the decay one rounding per operation.
#include "bbox_core.h"
#include "rpn_common.h"

#include <cmath>
#include <mutex>

namespace rpn {
namespace {

constexpr int kSoftThreads = 256;
constexpr int kSoftWaves = kSoftThreads / 64;
constexpr int kSoftMaxN = 4096;            // candidates of a pair live in LDS: 96 + 28 N bytes
constexpr int kSoftMaxEntries = 16384;     // C * min(max_per_class, N): the join keeps every staged score in LDS
constexpr size_t kSoftHeader = 96;         // u64 best[2][kSoftWaves] | int count[2][kSoftWaves]

struct SoftArgs {
    const float *boxes;      // (B,N,q,4)
    const float *scores;     // (B,N,C)
    int B, N, q, C;
    int max_sel;             // per class
    int max_total;
    int clip;
    float iou_thr, k, score_thr;
    float *out_boxes, *out_scores, *out_classes;
    int *out_idx, *out_valid;
    int *stage_idx;          // (B,C,max_sel) selected rows
    float *stage_score;      // (B,C,max_sel) their decayed scores
    int *stage_cnt;          // (B,C)
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <int METHOD>
__global__ void __launch_bounds__(kSoftThreads)
soft_select_kernel(SoftArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = p.N, C = p.C;
    unsigned long long *wbest = reinterpret_cast<unsigned long long *>(smem);
    int *wcnt = reinterpret_cast<int *>(smem + 8 * 2 * kSoftWaves);
    float4 *cb = reinterpret_cast<float4 *>(smem + kSoftHeader);     // canonical corners
    float *area = reinterpret_cast<float *>(cb + N);
    float *cur = area + N;
    int *row = reinterpret_cast<int *>(cur + N);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x;
    const int b = pair / C, c = pair - b * C;
    const float thr = p.score_thr;

    // ---- candidates into LDS, ascending row order
    int ncand = 0;
    for (int n0 = 0, it = 0; n0 < N; n0 += kSoftThreads, ++it) {
        const int n = n0 + tid;
        float s = 0.0f;
        if (n < N) s = p.scores[((size_t)b * N + n) * C + c];
        const bool take = n < N && s > thr;                          // strict: a NaN score never qualifies
        const unsigned long long mask = __ballot(take);
        int *wc = wcnt + (it & 1) * kSoftWaves;
        if (lane == 0) wc[wave] = __popcll(mask);
        __syncthreads();
        int off = ncand, total = 0;
#pragma unroll
        for (int w = 0; w < kSoftWaves; ++w) {
            const int v = wc[w];
            off += w < wave ? v : 0;
            total += v;
        }
        if (take) {
            const int i = off + __popcll(mask & ((1ull << lane) - 1ull));
            const CBox cx = canonical(load_box(p.boxes + 4 * (((size_t)b * N + n) * p.q + (p.q == 1 ? 0 : c))));
            cb[i] = make_float4(cx.ymin, cx.xmin, cx.ymax, cx.xmax);
            area[i] = cx.area;
            cur[i] = s;
            row[i] = n;
        }
        ncand += total;
    }
    if (ncand == 0) {
        if (tid == 0) p.stage_cnt[pair] = 0;
        return;
    }
    __syncthreads();

    // ---- the greedy loop: decay against the last selected box and elect the next one in one sweep
    const size_t stage = (size_t)pair * p.max_sel;
    CBox bm{};
    bool have = false;
    int nsel = 0;
    for (;;) {
        unsigned long long best = 0ull;
        for (int i = tid; i < ncand; i += kSoftThreads) {
            float s = cur[i];
            if (!(s > thr)) continue;                                // selected, removed or decayed away
            if (have) {
                const float4 v = cb[i];
                const CBox bn{v.x, v.y, v.z, v.w, area[i]};
                const float iou = nms_iou(bm, bn);
                if (METHOD == RPN_SOFT_NMS_LINEAR) {
                    if (iou > p.iou_thr) s = s * (1.0f - iou);
                } else {
                    if (iou > p.iou_thr)
                        s = -1.0f;                                   // TensorFlow's hard cut: a removal
                    else if (iou > 0.0f)
                        s = s * expf((iou * iou) * p.k);
                }
                cur[i] = s;
            }
            if (s > thr) {
                // positive floats order as their bits; candidates are in row order, so the lower index is the lower row
                const unsigned long long key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
                best = key > best ? key : best;
            }
        }
        best = wave_max_u64(best);
        unsigned long long *wb = wbest + (nsel & 1) * kSoftWaves;
        if (lane == 0) wb[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kSoftWaves; ++w) {
            const unsigned long long o = wb[w];
            best = o > best ? o : best;
        }
        if (best == 0ull) break;                                     // nothing live (uniform: every thread reads the same four)
        const int m = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
        if (tid == 0) {
            p.stage_idx[stage + nsel] = row[m];
            p.stage_score[stage + nsel] = __uint_as_float((unsigned)(best >> 32));
        }
        if (++nsel >= p.max_sel) break;
        if ((m & (kSoftThreads - 1)) == tid) cur[m] = -1.0f;         // its owner takes it out
        const float4 v = cb[m];
        bm = CBox{v.x, v.y, v.z, v.w, area[m]};
        have = true;
    }
    if (tid == 0) p.stage_cnt[pair] = nsel;
}

// entries of the non-increasing list s[0 .. n) that come before a foreign entry of score v: >= v when the list's class is the
// lower one (STRICT == false), > v otherwise
template <bool STRICT>
__device__ __forceinline__ int count_before(const float *s, int n, float v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool before = STRICT ? s[mid] > v : s[mid] >= v;
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kSoftThreads)
soft_join_kernel(SoftArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = p.C, max_sel = p.max_sel, N = p.N, M = p.max_total;
    float *sc = reinterpret_cast<float *>(smem);                     // [C][max_sel]
    int *cnt = reinterpret_cast<int *>(sc + (size_t)C * max_sel);    // [C]
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int E = C * max_sel;
    for (int c = tid; c < C; c += kSoftThreads) cnt[c] = p.stage_cnt[(size_t)b * C + c];
    __syncthreads();
    for (int e = tid; e < E; e += kSoftThreads) {
        const int c = e / max_sel, r = e - c * max_sel;
        sc[e] = r < cnt[c] ? p.stage_score[((size_t)b * C + c) * max_sel + r] : 0.0f;
    }
    __syncthreads();
    int total = 0;
    for (int c = 0; c < C; ++c) total += cnt[c];
    const int nvalid = total < M ? total : M;
    for (int e = tid; e < E; e += kSoftThreads) {
        const int c = e / max_sel, r = e - c * max_sel;
        if (r >= cnt[c]) continue;
        const float s = sc[e];
        int rank = r;
        for (int f = 0; f < c && rank < M; ++f) rank += count_before<false>(sc + (size_t)f * max_sel, cnt[f], s);
        for (int f = c + 1; f < C && rank < M; ++f) rank += count_before<true>(sc + (size_t)f * max_sel, cnt[f], s);
        if (rank >= M) continue;
        const size_t o = (size_t)b * M + rank;
        const int idx = p.stage_idx[((size_t)b * C + c) * max_sel + r];
        Box bx = load_box(p.boxes + 4 * (((size_t)b * N + idx) * p.q + (p.q == 1 ? 0 : c)));
        if (p.clip) {
            bx.y1 = clip01(bx.y1);
            bx.x1 = clip01(bx.x1);
            bx.y2 = clip01(bx.y2);
            bx.x2 = clip01(bx.x2);
        }
        store_box(p.out_boxes + 4 * o, bx);
        p.out_scores[o] = s;
        if (p.out_classes) p.out_classes[o] = (float)c;
        if (p.out_idx) p.out_idx[o] = idx;
    }
    for (int r = nvalid + tid; r < M; r += kSoftThreads) {
        const size_t o = (size_t)b * M + r;
        store_box(p.out_boxes + 4 * o, Box{0.0f, 0.0f, 0.0f, 0.0f});
        p.out_scores[o] = 0.0f;
        if (p.out_classes) p.out_classes[o] = 0.0f;
        if (p.out_idx) p.out_idx[o] = -1;
    }
    if (tid == 0) p.out_valid[b] = nvalid;
}

// a launch above the default 64 KB of dynamic LDS needs the function's ceiling raised; once per (device, size) is enough
struct LdsCeiling {
    std::mutex mu;
    size_t have[16] = {};
    hipError_t raise(const void *fn, size_t bytes)
    {
        if (bytes <= 64 * 1024) return hipSuccess;
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= 0 && dev < 16 && have[dev] >= bytes) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess && dev >= 0 && dev < 16) have[dev] = bytes;
        return e;
    }
};

int soft_max_sel(int N, int max_per_class)
{
    const int m = max_per_class < N ? max_per_class : N;
    return m < 1 ? 1 : m;
}

size_t soft_stage_bytes(int B, int C, int max_sel) { return a256((size_t)B * C * max_sel * sizeof(int)); }

}  // namespace
}  // namespace rpn

using namespace rpn;

extern "C" size_t rpn_soft_nms_workspace_bytes(int B, int N, int C, int max_per_class, int max_total)
{
    (void)max_total;
    if (B <= 0 || C < 1 || N < 0 || max_per_class < 0) return 0;
    const int max_sel = soft_max_sel(N, max_per_class);
    return 2 * soft_stage_bytes(B, C, max_sel) + a256((size_t)B * C * sizeof(int));
}

extern "C" int rpn_soft_nms(const float *d_boxes, const float *d_scores, int B, int N, int q, int C, int max_per_class,
                            int max_total, int method, float iou_threshold, float sigma, float score_threshold, int clip_boxes,
                            float *d_out_boxes, float *d_out_scores, float *d_out_classes, int32_t *d_out_idx,
                            int32_t *d_out_valid, void *d_workspace, size_t workspace_bytes, void *stream)
{
    RPN_REQUIRE(B >= 0 && N >= 0 && C >= 1, "rpn_soft_nms: bad sizes B=%d N=%d C=%d", B, N, C);
    RPN_REQUIRE(q == 1 || q == C, "rpn_soft_nms: q must be 1 or C (q=%d, C=%d)", q, C);
    RPN_REQUIRE(max_per_class >= 0 && max_total >= 0, "rpn_soft_nms: negative output size");
    RPN_REQUIRE(method == RPN_SOFT_NMS_LINEAR || method == RPN_SOFT_NMS_GAUSSIAN, "rpn_soft_nms: unknown method %d", method);
    RPN_REQUIRE(iou_threshold >= 0.0f, "rpn_soft_nms: iou_threshold must be >= 0, got %g", (double)iou_threshold);
    RPN_REQUIRE(sigma > 0.0f, "rpn_soft_nms: sigma must be > 0, got %g", (double)sigma);
    RPN_REQUIRE(score_threshold >= 0.0f, "rpn_soft_nms: score_threshold must be >= 0 (a decay would raise a negative score), got %g",
                (double)score_threshold);
    RPN_REQUIRE(N <= kSoftMaxN, "rpn_soft_nms: N = %d is above the limit of %d boxes per image", N, kSoftMaxN);
    const int max_sel = soft_max_sel(N, max_per_class);
    RPN_REQUIRE((long long)C * max_sel <= kSoftMaxEntries, "rpn_soft_nms: C * min(max_per_class, N) = %lld is above the limit of %d",
                (long long)C * max_sel, kSoftMaxEntries);
    if (B == 0 || max_total == 0) return RPN_OK;
    RPN_REQUIRE(d_out_boxes && d_out_scores && d_out_valid, "rpn_soft_nms: null output pointer");
    RPN_REQUIRE(N == 0 || (d_boxes && d_scores), "rpn_soft_nms: null input pointer");
    RPN_REQUIRE_DEVICE();
    const size_t need = rpn_soft_nms_workspace_bytes(B, N, C, max_per_class, max_total);
    if (!d_workspace || workspace_bytes < need)
        return fail(RPN_ERR_WORKSPACE, "rpn_soft_nms: workspace of %zu bytes needed, %zu given", need, workspace_bytes);

    SoftArgs p{};
    p.boxes = d_boxes;
    p.scores = d_scores;
    p.B = B; p.N = N; p.q = q; p.C = C;
    p.max_sel = max_sel;
    p.max_total = max_total;
    p.clip = clip_boxes;
    p.iou_thr = iou_threshold;
    p.k = (float)(-1.0 / (double)sigma);
    p.score_thr = (max_per_class == 0) ? INFINITY : score_threshold;      // nothing can be selected
    p.out_boxes = d_out_boxes; p.out_scores = d_out_scores; p.out_classes = d_out_classes;
    p.out_idx = d_out_idx; p.out_valid = d_out_valid;
    unsigned char *ws = reinterpret_cast<unsigned char *>(d_workspace);
    const size_t stage = soft_stage_bytes(B, C, max_sel);
    p.stage_idx = reinterpret_cast<int *>(ws);
    p.stage_score = reinterpret_cast<float *>(ws + stage);
    p.stage_cnt = reinterpret_cast<int *>(ws + 2 * stage);

    hipStream_t s = as_stream(stream);
    auto select = method == RPN_SOFT_NMS_LINEAR ? soft_select_kernel<RPN_SOFT_NMS_LINEAR> : soft_select_kernel<RPN_SOFT_NMS_GAUSSIAN>;
    const size_t lds_select = kSoftHeader + (size_t)28 * N;             // sized by N, not by the limit
    {
        static LdsCeiling ceiling[2];
        RPN_HIP_CHECK(ceiling[method].raise(reinterpret_cast<const void *>(select), lds_select));
    }
    hipLaunchKernelGGL(select, dim3(B * C), dim3(kSoftThreads), lds_select, s, p);
    RPN_CHECK_LAUNCH();
    const size_t lds_join = (size_t)4 * C * max_sel + (size_t)4 * C;
    {
        static LdsCeiling ceiling;
        RPN_HIP_CHECK(ceiling.raise(reinterpret_cast<const void *>(soft_join_kernel), lds_join));
    }
    hipLaunchKernelGGL(soft_join_kernel, dim3(B), dim3(kSoftThreads), lds_join, s, p);
    RPN_CHECK_LAUNCH();
    return RPN_OK;
}
