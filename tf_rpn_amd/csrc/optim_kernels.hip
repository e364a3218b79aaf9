// optim_kernels.hip -- what the trainers' update can do beyond plain Adam (train_kernels.hip's adam_kernel, which stays the default
// step of both handles): the global squared norm of the gradient buffer, and one update kernel per rule -- SGD with (Nesterov)
// momentum, or Adam -- with L2 weight decay on the kernels and clipping by the global norm.  The contract is in train_head.h and
// include/rpn_hip.h ("Optimizers").
//
// This file is compiled with -ffp-contract=off: every float32 operation below rounds on its own, so the SGD step is bit for bit its
// numpy restatement.  adam_kernel is compiled with contraction on, and the compiler fuses exactly two of its operations (g g - v and
// the multiply-add into v); adam_update spells those two as fmaf so that both kernels give the same bits on the same input.
//
// Both kernels are memory-bound ("Optimizers"): 16-byte loads and stores, a grid-stride loop over float4s, up to
// 2048 workgroups of 256.  No floating-point atomics: the norm's partials are added in an order that depends on n alone.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "rpn_common.h"
#include "train_common.h"
#include "train_head.h"

namespace rpn {

constexpr int kOptThreads = 256;
constexpr int kOptMaxBlocks = 2048;             // 8 workgroups per CU of the 256
constexpr size_t kOptHeadBytes = 256;           // S at byte 0, c at byte 8 of the update's device block

static int opt_blocks(long long n)
{
    const long long nv = (n + 3) / 4;
    return (int)std::max<long long>(1, std::min<long long>((nv + kOptThreads - 1) / kOptThreads, kOptMaxBlocks));
}

// ---- the squared norm: pass 1 ---------------------------------------------------------------------------------------------------
// Thread k of the grid adds the squares of the float4s k, k + T, k + 2 T .. (T threads in all), each x, y, z, w in order, in float64;
// the block's 256 sums meet in a fixed LDS tree.  The last float4 may be partial: it is read element by element.
__global__ void __launch_bounds__(kOptThreads) grad_sq_norm_kernel(const float *__restrict__ g, long long n, double *__restrict__ part)
{
    const long long nv = (n + 3) >> 2;
    double acc = 0.0;
    for (long long q = (long long)blockIdx.x * kOptThreads + threadIdx.x; q < nv; q += (long long)gridDim.x * kOptThreads) {
        const long long i0 = q << 2;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i0 + 4 <= n) {
            const float4 f = *reinterpret_cast<const float4 *>(g + i0);
            x[0] = f.x, x[1] = f.y, x[2] = f.z, x[3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) x[j] = g[i0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
    }
    __shared__ double red[kOptThreads];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kOptThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ---- the squared norm: pass 2 (one workgroup) -- the partials in a fixed tree, S and the clip scale -------------------------------
__global__ void __launch_bounds__(kOptThreads) grad_sq_norm_finish_kernel(const double *__restrict__ part, int nparts, float clipnorm,
                                                                        double *__restrict__ S, float *__restrict__ scale)
{
    __shared__ double red[kOptThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kOptThreads) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kOptThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double sum = red[0], norm = sqrt(sum);
        float c = 1.0f;
        if (!(sum <= 1.7976931348623157e308)) c = __builtin_nanf("");      // NaN or infinity: the step carries it into every weight
        else if (clipnorm > 0.0f && norm > (double)clipnorm) c = (float)((double)clipnorm / norm);
        S[0] = sum;
        scale[0] = c;
    }
}

// ---- the update -------------------------------------------------------------------------------------------------------------------
struct OptimArgs {
    float *w;
    const float *g;
    float *m, *v;
    long long n;
    const long long *ranges;                    // device: sorted, disjoint [begin, end) pairs -- the decayed elements
    int n_ranges;
    const float *scale;                         // device: the clip scale, or null
    long long t;
    float lr, b1, b2, eps, mu, wd;
    int nesterov;
};

// adam_kernel's arithmetic, operation for operation (see the head of this file)
__device__ __forceinline__ void adam_update(float &w, float g, float &m, float &v, float alpha, float omb1, float omb2, float eps)
{
    const float mi = m + (g - m) * omb1;
    const float vi = fmaf(omb2, fmaf(g, g, -v), v);
    m = mi;
    v = vi;
    w = w - alpha * mi / (sqrtf(vi) + eps);
}

__device__ __forceinline__ void sgd_update(float &w, float g, float &a, float lr, float mu, bool nesterov)
{
    const float step = lr * g;
    const float ai = mu * a - step;
    a = ai;
    w = nesterov ? w + (mu * ai - step) : w + ai;
}

// Each thread takes whole float4s at a growing index, so it follows the sorted range table with a cursor: a binary search when the
// cursor's range ends below the float4, single steps inside it.  A range may begin and end anywhere.
template <int KIND>
__global__ void __launch_bounds__(kOptThreads) optim_apply_kernel(OptimArgs a)
{
    const float c = a.scale ? a.scale[0] : 1.0f;
    float alpha = 0.0f;
    if (KIND == RPN_OPT_ADAM)
        alpha = (float)((double)a.lr * sqrt(1.0 - pow((double)a.b2, (double)a.t)) / (1.0 - pow((double)a.b1, (double)a.t)));
    const float omb1 = 1.0f - a.b1, omb2 = 1.0f - a.b2;
    const long long nv = (a.n + 3) >> 2;
    const int nr = a.n_ranges;
    int r = 0;
    long long rb = 0, re = 0;
    if (nr > 0) rb = a.ranges[0], re = a.ranges[1];
    for (long long q = (long long)blockIdx.x * kOptThreads + threadIdx.x; q < nv; q += (long long)gridDim.x * kOptThreads) {
        const long long i0 = q << 2;
        const bool full = i0 + 4 <= a.n;
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (full) {
            const float4 fw = *reinterpret_cast<const float4 *>(a.w + i0), fg = *reinterpret_cast<const float4 *>(a.g + i0);
            const float4 fm = *reinterpret_cast<const float4 *>(a.m + i0);
            w[0] = fw.x, w[1] = fw.y, w[2] = fw.z, w[3] = fw.w;
            g[0] = fg.x, g[1] = fg.y, g[2] = fg.z, g[3] = fg.w;
            m[0] = fm.x, m[1] = fm.y, m[2] = fm.z, m[3] = fm.w;
            if (KIND == RPN_OPT_ADAM) {
                const float4 fv = *reinterpret_cast<const float4 *>(a.v + i0);
                v[0] = fv.x, v[1] = fv.y, v[2] = fv.z, v[3] = fv.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= a.n) continue;
                w[j] = a.w[i0 + j], g[j] = a.g[i0 + j], m[j] = a.m[i0 + j];
                if (KIND == RPN_OPT_ADAM) v[j] = a.v[i0 + j];
            }
        }
        if (r < nr && re <= i0) {               // the first range that ends above i0
            int lo = r + 1, hi = nr;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a.ranges[2 * mid + 1] <= i0) lo = mid + 1;
                else hi = mid;
            }
            r = lo;
            if (r < nr) rb = a.ranges[2 * r], re = a.ranges[2 * r + 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j;
            while (r < nr && re <= i) {
                ++r;
                if (r < nr) rb = a.ranges[2 * r], re = a.ranges[2 * r + 1];
            }
            const bool decayed = r < nr && i >= rb;
            const float g1 = a.scale ? g[j] * c : g[j];
            const float g2 = decayed ? g1 + a.wd * w[j] : g1;
            if (KIND == RPN_OPT_ADAM) adam_update(w[j], g2, m[j], v[j], alpha, omb1, omb2, a.eps);
            else sgd_update(w[j], g2, m[j], a.lr, a.mu, a.nesterov != 0);
        }
        if (full) {
            *reinterpret_cast<float4 *>(a.w + i0) = make_float4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<float4 *>(a.m + i0) = make_float4(m[0], m[1], m[2], m[3]);
            if (KIND == RPN_OPT_ADAM) *reinterpret_cast<float4 *>(a.v + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= a.n) continue;
                a.w[i0 + j] = w[j], a.m[i0 + j] = m[j];
                if (KIND == RPN_OPT_ADAM) a.v[i0 + j] = v[j];
            }
        }
    }
}

// ---- host launchers -----------------------------------------------------------------------------------------------------------------
size_t grad_norm_ws_bytes(long long n) { return a256((size_t)opt_blocks(n) * sizeof(double)); }

hipError_t launch_grad_sq_norm(const float *g, long long n, float clipnorm, double *part, double *S, float *scale, hipStream_t s)
{
    const int nb = opt_blocks(n);
    hipLaunchKernelGGL(grad_sq_norm_kernel, dim3(nb), dim3(kOptThreads), 0, s, g, n, part);
    hipLaunchKernelGGL(grad_sq_norm_finish_kernel, dim3(1), dim3(kOptThreads), 0, s, part, nb, clipnorm, S, scale);
    return hipGetLastError();
}

static hipError_t launch_optim_apply(int kind, const OptimArgs &a, hipStream_t s)
{
    const dim3 grid(opt_blocks(a.n)), block(kOptThreads);
    if (kind == RPN_OPT_SGD) hipLaunchKernelGGL(optim_apply_kernel<RPN_OPT_SGD>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(optim_apply_kernel<RPN_OPT_ADAM>, grid, block, 0, s, a);
    return hipGetLastError();
}

int optim_check_config(const char *who, int kind, float momentum, int nesterov, float weight_decay, float clipnorm)
{
    RPN_REQUIRE(kind == RPN_OPT_ADAM || kind == RPN_OPT_SGD, "%s: kind = %d is neither RPN_OPT_ADAM (0) nor RPN_OPT_SGD (1)", who, kind);
    RPN_REQUIRE(momentum >= 0.0f && momentum < 1.0f, "%s: momentum = %g must lie in [0, 1)", who, (double)momentum);      // (a NaN fails both)
    RPN_REQUIRE(nesterov == 0 || nesterov == 1, "%s: nesterov must be 0 or 1", who);
    RPN_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.0f, "%s: weight_decay = %g must be finite and >= 0", who,
                (double)weight_decay);
    RPN_REQUIRE(std::isfinite(clipnorm) && clipnorm >= 0.0f, "%s: global_clipnorm = %g must be finite and >= 0 (0: off)", who,
                (double)clipnorm);
    return RPN_OK;
}

void optim_free(OptimDevice *d)
{
    if (d->buf) (void)hipFree(d->buf);
    *d = OptimDevice{};
}

static double *optim_S(const OptimDevice &d) { return reinterpret_cast<double *>(d.buf); }
static float *optim_scale(const OptimDevice &d) { return reinterpret_cast<float *>(d.buf + 8); }

int optim_step(const char *who, const OptimConfig &cfg, OptimDevice *d, const long long *ranges, int n_ranges, float *w, const float *g,
               float *m, float *v, long long n, long long t, float lr, float b1, float b2, float eps, hipStream_t s)
{
    const size_t part_bytes = grad_norm_ws_bytes(n);
    if (!d->buf) {                              // once: the block, and the range table behind the partials
        const size_t table = (size_t)n_ranges * 2 * sizeof(long long);
        RPN_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d->buf), kOptHeadBytes + part_bytes + std::max<size_t>(table, 16)));
        hipError_t e = hipMemset(d->buf, 0, kOptHeadBytes);
        if (e == hipSuccess && table) e = hipMemcpy(d->buf + kOptHeadBytes + part_bytes, ranges, table, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            optim_free(d);
            return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
        }
        d->n_ranges = n_ranges;
    }
    const bool clip = cfg.clipnorm > 0.0f, decay = cfg.weight_decay > 0.0f;
    hipError_t e = hipSuccess;
    if (clip) e = launch_grad_sq_norm(g, n, cfg.clipnorm, reinterpret_cast<double *>(d->buf + kOptHeadBytes), optim_S(*d), optim_scale(*d), s);
    OptimArgs a{};
    a.w = w, a.g = g, a.m = m, a.v = v, a.n = n;
    a.ranges = reinterpret_cast<const long long *>(d->buf + kOptHeadBytes + part_bytes);
    a.n_ranges = decay ? d->n_ranges : 0;
    a.scale = clip ? optim_scale(*d) : nullptr;
    a.t = t, a.lr = lr, a.b1 = b1, a.b2 = b2, a.eps = eps, a.mu = cfg.momentum, a.wd = cfg.weight_decay, a.nesterov = cfg.nesterov;
    if (e == hipSuccess) e = launch_optim_apply(cfg.kind, a, s);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    if (clip) d->stepped = true;
    return RPN_OK;
}

int optim_grad_norm(const char *who, const OptimConfig &cfg, const OptimDevice &d, double *norm, float *scale, hipStream_t s)
{
    RPN_REQUIRE(norm && scale, "%s: null argument", who);
    RPN_REQUIRE(cfg.clipnorm > 0.0f, "%s: no clip norm is configured (set_optimizer's global_clipnorm): no norm is computed", who);
    RPN_REQUIRE(d.buf && d.stepped, "%s: no update step has run under this clip norm", who);
    double S = 0.0;
    RPN_HIP_CHECK(hipMemcpyAsync(&S, optim_S(d), sizeof(double), hipMemcpyDeviceToHost, s));
    RPN_HIP_CHECK(hipMemcpyAsync(scale, optim_scale(d), sizeof(float), hipMemcpyDeviceToHost, s));
    RPN_HIP_CHECK(hipStreamSynchronize(s));
    *norm = std::sqrt(S);
    return RPN_OK;
}

}  // namespace rpn

using namespace rpn;

// ---- C ABI: the two kernels on caller buffers ---------------------------------------------------------------------------------------------
static bool aligned16p(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" size_t rpn_grad_sq_norm_workspace_bytes(long long n) { return n >= 1 ? grad_norm_ws_bytes(n) : 0; }

extern "C" int rpn_grad_sq_norm(const float *d_g, long long n, float clipnorm, double *d_S, float *d_scale, void *d_ws, size_t ws_bytes,
                                void *stream)
{
    const char *who = "rpn_grad_sq_norm";
    RPN_REQUIRE(d_g && d_S && d_scale, "%s: null pointer", who);
    RPN_REQUIRE(n >= 1, "%s: n = %lld", who, n);
    RPN_REQUIRE(std::isfinite(clipnorm) && clipnorm >= 0.0f, "%s: clipnorm = %g must be finite and >= 0 (0: off)", who, (double)clipnorm);
    RPN_REQUIRE(aligned16p(d_g), "%s: the buffer must be 16-byte aligned", who);
    RPN_REQUIRE((reinterpret_cast<uintptr_t>(d_S) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d_scale) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(d_ws) & 7u) == 0, "%s: S and the workspace must be 8-byte aligned, scale 4-byte aligned", who);
    if (!d_ws || ws_bytes < grad_norm_ws_bytes(n)) return fail(RPN_ERR_WORKSPACE, "%s: %zu bytes of workspace needed", who, grad_norm_ws_bytes(n));
    RPN_REQUIRE_DEVICE();
    const hipError_t e = launch_grad_sq_norm(d_g, n, clipnorm, reinterpret_cast<double *>(d_ws), d_S, d_scale, as_stream(stream));
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
}

extern "C" int rpn_optimizer_apply(int kind, float *d_w, const float *d_g, float *d_m, float *d_v, long long n, const long long *d_decay_ranges,
                                   int n_ranges, long long t, float lr, float beta_1, float beta_2, float epsilon, float momentum,
                                   int nesterov, float weight_decay, const float *d_scale, void *stream)
{
    const char *who = "rpn_optimizer_apply";
    const int st = optim_check_config(who, kind, momentum, nesterov, weight_decay, 0.0f);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(d_w && d_g && d_m && (d_v || kind == RPN_OPT_SGD), "%s: null pointer", who);
    RPN_REQUIRE(n >= 1 && t >= 1, "%s: n = %lld, t = %lld (the number of this step, from 1)", who, n, t);
    RPN_REQUIRE(std::isfinite(lr) && lr >= 0.0f, "%s: lr = %g", who, (double)lr);
    RPN_REQUIRE(kind == RPN_OPT_SGD || (beta_1 >= 0.0f && beta_1 < 1.0f && beta_2 >= 0.0f && beta_2 < 1.0f && std::isfinite(epsilon) && epsilon >= 0.0f),
                "%s: bad Adam hyper-parameters", who);
    RPN_REQUIRE(aligned16p(d_w) && aligned16p(d_g) && aligned16p(d_m) && aligned16p(d_v), "%s: w, g, m and v must be 16-byte aligned", who);
    RPN_REQUIRE((reinterpret_cast<uintptr_t>(d_scale) & 3u) == 0, "%s: the scale must be 4-byte aligned", who);
    RPN_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || d_decay_ranges), "%s: n_ranges = %d", who, n_ranges);
    RPN_REQUIRE(aligned16p(d_decay_ranges), "%s: the range table must be 16-byte aligned", who);
    RPN_REQUIRE_DEVICE();
    const hipStream_t s = as_stream(stream);
    const bool decay = n_ranges > 0 && weight_decay > 0.0f;
    hipError_t e;
    if (kind == RPN_OPT_ADAM && !d_scale && !decay) {        // today's step
        e = launch_adam(d_w, d_g, d_m, d_v, n, t, lr, beta_1, beta_2, epsilon, s);
    } else {
        // (the table's values are compared with element indices and never used as one: a table that is not sorted decays the wrong
        // elements and touches no other memory)
        OptimArgs a{};
        a.w = d_w, a.g = d_g, a.m = d_m, a.v = d_v, a.n = n, a.scale = d_scale;
        a.ranges = decay ? d_decay_ranges : nullptr, a.n_ranges = decay ? n_ranges : 0;
        a.t = t, a.lr = lr, a.b1 = beta_1, a.b2 = beta_2, a.eps = epsilon, a.mu = momentum, a.wd = weight_decay, a.nesterov = nesterov;
        e = launch_optim_apply(kind, a, s);
    }
    return e == hipSuccess ? RPN_OK : fail(RPN_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
}
