// eval_sort.h -- what the two evaluators' ranking kernels share (eval_kernels.hip: eval_class_kernel; eval_coco_kernels.hip:
// coco_rank_kernel): the workgroup scan, the compaction of one class's records in slot order and the stable LSD radix sort of
// (key, payload) pairs.  One 1024-thread workgroup; every function is called by all of its threads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rpn {

constexpr int kEvThreads = 1024;
constexpr int kEvWaves = kEvThreads / 64;
constexpr int kEvSortItems = 4;                         // keys per thread and tile of the sort passes
constexpr int kEvSortTile = kEvThreads * kEvSortItems;
constexpr int kEvScanItems = 8;                         // records per thread and tile of the compaction

// the LDS of ev_compact and ev_radix_sort
struct EvSortLds {
    int hist[4][256];
    int base[256];
    int wcnt[kEvWaves][256];
    int wsum[kEvWaves];
    int skip;
};

// lanes of this wave whose 8-bit digit equals mine (invalid lanes match nobody)
__device__ __forceinline__ unsigned long long wave_match8(unsigned d, bool valid)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool on = (d >> bit) & 1u;
        const unsigned long long m = __ballot(on);
        peers &= on ? m : ~m;
    }
    return peers;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// exclusive prefix of a per-thread count over the workgroup, in thread order; *total = the workgroup's sum.  wsum: kEvWaves ints of LDS.
__device__ __forceinline__ int block_scan(int v, int *wsum, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kEvWaves; ++i) {
        const int s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// The records of one class, in slot order, into cur[0, n): kEvScanItems consecutive records per thread (64 bytes, four 16-byte loads
// in flight per lane), so thread order then item order is slot order.  take(record) says whether the record is the class's;
// pair(record, slot) is what goes into the workspace.  No atomics.
template <class Take, class Pair>
__device__ __forceinline__ void ev_compact(const int2 *rec, long long n_rec, uint2 *cur, int n, int *wsum, Take take, Pair pair)
{
    const int tid = threadIdx.x;
    int run = 0;
    for (long long s0 = 0; s0 < n_rec; s0 += (long long)kEvThreads * kEvScanItems) {
        const long long first = s0 + (long long)tid * kEvScanItems;
        int2 r[kEvScanItems];
        if (first + kEvScanItems <= n_rec) {
            const int4 *q = reinterpret_cast<const int4 *>(rec + first);       // 64-byte aligned: the buffer is, first % 8 == 0
#pragma unroll
            for (int u = 0; u < kEvScanItems / 2; ++u) {
                const int4 v = q[u];
                r[2 * u] = make_int2(v.x, v.y);
                r[2 * u + 1] = make_int2(v.z, v.w);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kEvScanItems; ++u) r[u] = first + u < n_rec ? rec[first + u] : make_int2(0, 0);
        }
        unsigned mine = 0u;
#pragma unroll
        for (int u = 0; u < kEvScanItems; ++u)
            if (take(r[u])) mine |= 1u << u;
        int total;
        int pos = run + block_scan(__popc(mine), wsum, &total);
        // (pos < n always: ndet counts exactly these records; the test keeps a torn counter from writing past the segment)
#pragma unroll
        for (int u = 0; u < kEvScanItems; ++u) {
            if (((mine >> u) & 1u) && pos < n) {
                cur[pos] = pair(r[u], first + u);
                ++pos;
            }
        }
        run += total;
    }
}

// A stable LSD radix sort of cur[0, n) by .x, ascending, four 8-bit passes over the ping-pong pair (cur, alt): all four histograms
// from one read, a pass whose digit is the same in every key is skipped, tiles of kEvSortTile keys, ranks inside a tile from wave
// ballots and per-wave digit counts, so equal keys keep their order.  Returns the number of passes taken modulo 2; cur then points
// at the sorted half.
__device__ __forceinline__ int ev_radix_sort(uint2 *&cur, uint2 *&alt, int n, EvSortLds &L)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < 4 * 256; i += kEvThreads) (&L.hist[0][0])[i] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kEvThreads) {
        const int i = i0 + tid;
        const bool valid = i < n;
        const unsigned key = valid ? cur[i].x : 0u;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const unsigned d = (key >> (8 * ps)) & 255u;
            const unsigned long long peers = wave_match8(d, valid);
            if (valid && (peers & lanes_below(lane)) == 0ull) atomicAdd(&L.hist[ps][d], __popcll(peers));
        }
    }
    __syncthreads();
    int par = 0;
    for (int ps = 0; ps < 4; ++ps) {
        if (tid == 0) L.skip = 0;
        __syncthreads();
        if (tid < 256 && L.hist[ps][tid] == n) L.skip = 1;      // every key has this digit: the pass would be the identity
        // exclusive scan of the 256 bins -> where each digit's run starts
        int incl = tid < 256 ? L.hist[ps][tid] : 0;
        const int mine = incl;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) L.wsum[w] = incl;
        __syncthreads();
        if (tid < 256) {
            int b0 = 0;
            for (int i = 0; i < w; ++i) b0 += L.wsum[i];
            L.base[tid] = b0 + incl - mine;
        }
        const bool skipped = L.skip != 0;
        __syncthreads();
        if (skipped || n == 0) continue;
        // tiles of kEvSortTile keys; wave w owns kEvSortItems runs of 64 consecutive keys, so (wave, round, lane) order is key order
        for (int i0 = 0; i0 < n; i0 += kEvSortTile) {
            uint2 kv[kEvSortItems];
            int rank[kEvSortItems];
            const int first = i0 + w * (64 * kEvSortItems) + lane;
#pragma unroll
            for (int u = 0; u < kEvSortItems; ++u) {
                kv[u] = make_uint2(0u, 0u);
                if (first + 64 * u < n) kv[u] = cur[first + 64 * u];
            }
            for (int k = tid; k < kEvWaves * 256; k += kEvThreads) (&L.wcnt[0][0])[k] = 0;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kEvSortItems; ++u) {
                const bool valid = first + 64 * u < n;
                const unsigned d = (kv[u].x >> (8 * ps)) & 255u;
                const unsigned long long peers = wave_match8(d, valid);
                const int r = __popcll(peers & lanes_below(lane));
                const int before = L.wcnt[w][d];                // this wave's keys of digit d in its earlier rounds
                rank[u] = before + r;
                __builtin_amdgcn_wave_barrier();                // every peer has read the count before the first of them raises it
                if (valid && r == 0) L.wcnt[w][d] = before + __popcll(peers);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
            if (tid < 256) {                                // this tile's keys of digit `tid`, wave by wave
                int run = L.base[tid];
                for (int k = 0; k < kEvWaves; ++k) {
                    const int t = L.wcnt[k][tid];
                    L.wcnt[k][tid] = run;
                    run += t;
                }
                L.base[tid] = run;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kEvSortItems; ++u)
                if (first + 64 * u < n) alt[L.wcnt[w][(kv[u].x >> (8 * ps)) & 255u] + rank[u]] = kv[u];
            __syncthreads();
        }
        uint2 *t = cur;
        cur = alt;
        alt = t;
        par ^= 1;
    }
    return par;
}

}  // namespace rpn
