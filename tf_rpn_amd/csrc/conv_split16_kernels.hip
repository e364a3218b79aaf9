// conv_split16_kernels.hip -- the x3-split 3x3 convolution (conv_split_kernels.hip has the arithmetic and the SPLIT16 layout)
// on the 16x16x32 MFMA, 32-channel slices, weights in "split32" packing:
//   conv3x3_split16_kernel      register-staged                                             (odd slice counts, small grids, split-K)
//   conv3x3_split16_dma_kernel  LDS-DMA staging, one barrier per tap, persistent workgroups whose tap stream runs on across
//                               tiles: the dominant kernel of the headline step              (11 of VGG16's 13 3x3 layers)
// then their launchers and launch predicates.  DESIGN.md 4.1 has the measurements that chose between the families.
#include "split_conv.h"

#include <mutex>
#include <unordered_map>

// Debug build only (-DRPN_STAMP, scripts/stamp_probe.py): in-kernel cycle stamps of the 16x16x32 kernel's phases.
#ifdef RPN_STAMP
__device__ unsigned long long g_rpn_stamps[8192 * 32];
#define RPN_STAMP_AT(k)                                                                                    \
    do {                                                                                                   \
        if (threadIdx.x == 0 && blockIdx.x < 8192 && (k) < 32)                                             \
            g_rpn_stamps[blockIdx.x * 32 + (k)] = __builtin_readcyclecounter();                            \
    } while (0)
#define RPN_STAMP_VAL(k, v)                                                                                \
    do {                                                                                                   \
        if (threadIdx.x == 0 && blockIdx.x < 8192) g_rpn_stamps[blockIdx.x * 32 + (k)] = (v);             \
    } while (0)
extern "C" int rpn_debug_read_stamps(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rpn_stamps), (size_t)n * 8);
}
// HW_ID of every wave of the first 64 workgroups (which waves of a workgroup share a SIMD): [workgroup][wave]
__device__ unsigned g_rpn_wave_hwid[64 * 16];
#define RPN_STAMP_WAVE_HWID()                                                                              \
    do {                                                                                                   \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 64)                                                    \
            g_rpn_wave_hwid[blockIdx.x * 16 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_getreg((31 << 11) | 4); \
    } while (0)
extern "C" int rpn_debug_read_wave_hwid(unsigned *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rpn_wave_hwid), (size_t)n * 4);
}
#else
#define RPN_STAMP_WAVE_HWID() ((void)0)
#define RPN_STAMP_AT(k) ((void)0)
#define RPN_STAMP_VAL(k, v) ((void)0)
#endif

namespace rpn {

// ---- 16x16x32-MFMA variant -----------------------------------------------------------------------------
// Same algorithm on v_mfma_f32_16x16x32_{f16,bf16}: on MI355X the chip holds a higher clock on this MFMA shape
// than on 32x32x16 under load, so equal cycles per flop turn into more flops per second.  K = 32 per MFMA, so the
// K-slice is 32 channels: 8 x 32 px x 128 ch tile, 8 waves (512 threads, each 64 px x 64 ch = 4 x 4 MFMA tiles),
// one workgroup per CU (136 KB LDS: two halo buffers of 340 px x 128 B, one weight buffer of 3 taps x 128 x 128 B).
// LDS rows hold 8 pieces [hi k0-7, hi k8-15, hi k16-23, hi k24-31, lo ...] XOR-swizzled by halo_swz(column)
// (resp. (n >> 1) & 7 for the weight rows, whose reads are never shifted): every ds_read_b128 fragment read is conflict-free.  Weights use the "split32" packing
// [Cin/32][9][cout_pad][128 B] in that piece order; activations stay SPLIT16 in HBM (pieces re-ordered on staging).

// Timing experiment only (-DRPN_NOSTORE): every epilogue store of a lane goes to one 16-byte slot per lane, so the
// instruction stream is unchanged but no output traffic reaches HBM.
#ifdef RPN_NOSTORE
#define RPN_STORE_INDEX(i) ((i) & 63)
#else
#define RPN_STORE_INDEX(i) (i)
#endif

// Epilogue shared by the 16x16x32 kernels: scale + bias + activation (+ fused 2x2 max-pool), transposed through a
// wave-private LDS staging area, 16-byte stores (C/D of the 16x16 MFMA: column = lane & 15, row = 4 * (lane >> 4) + reg).
// The caller guarantees that no wave still reads (and no DMA still writes) the pipeline buffers the area overlays.
template <bool F16, bool POOL, int RW, int NW, int NJ = 4>
__device__ __forceinline__ void split16_epilogue(f32x4 (&acc)[RW * 2][NJ], float *lds_f, const SplitConvArgs &a, int img,
                                                 int oy0, int ox0, int n0, int wave, int wm, int wn, int lane,
                                                 int stamp_base = -1 /* -DRPN_STAMP builds: first of 4 stamp slots */)
{
    (void)stamp_base;
    // the lane index as an opaque value: the epilogue's lane arithmetic (e / PP, e % PP, staging addresses) is otherwise
    // loop-invariant in the persistent kernel's tile loop, gets hoisted in front of it and is carried through the tap loop
    // in registers the 256-VGPR kernel does not have (5 were spilled to scratch)
    asm volatile("" : "+v"(lane));
    constexpr int MT = RW * 2;
    constexpr int CW = 16 * NJ;                        // channels per wave
    constexpr int STAGE_LD = CW + kStagePad;
    constexpr int PP = CW / 4;                         // 16-byte pieces (or float4s) per pixel
    const int lr = lane & 15, kg = lane >> 4;
    // ---- epilogue (as in the 32x32 kernel; C/D of the 16x16 MFMA: column = lane & 15, row = 4 * (lane >> 4) + reg) --
    float *stage = lds_f + wave * (32 * STAGE_LD);
    float bias_v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wn * CW + j * 16 + lr;
        bias_v[j] = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;
    }
    const float act_lo = a.act == ACT_LINEAR ? -INFINITY : 0.0f;
    const float act_hi = a.act == ACT_RELU6 ? 6.0f : INFINITY;
    const int cout_chunks = a.Cout >> 4;
    const int nbase = n0 + wn * CW;
    // Stores (round 6): one buffer per output ROW SEGMENT [oxb, OWo) of the image -- a pixel past the right edge is past the buffer's
    // end and the hardware drops it, a lane whose channels lie beyond Cout carries an out-of-range offset -- so a round is two LDS
    // reads, the hi / lo split and ONE buffer store whose 32-bit offset advances by a constant: no branch, no 64-bit index
    // arithmetic, no integer multiply.  (Rounds 1-5 recomputed (((img * OH + oy) * OW + ox) * chunks + n / 16) * 4 + pc in 64 bits
    // and branched on ox < OW && n < Cout in every round: ~100 v_mul_lo_u32 / v_lshl_add_u64 / v_mad_u64_u32 and 92 exec branches per
    // tile and thread -- a third of the epilogue's 2 600 vector instructions.)
    const int pix_bytes = a.out_f32 ? a.Cout * 4 : cout_chunks * 64;       // bytes per output pixel
    constexpr int PXR = 64 / PP;                                          // pixels per round of 64 lanes
    const int px_l = lane / PP, q_l = lane % PP;
    auto store_stage = [&](int npx_log2, int oy, int oxb, int OHo, int OWo) {
        if (oy >= OHo) return;
        const int rounds = (PP << npx_log2) >> 6;
        const long long row_off = (((long long)img * OHo + oy) * OWo + oxb) * (long long)pix_bytes;
        const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char *>(a.out) + row_off, (short)0,
                                                                              (OWo - oxb) * pix_bytes, 0x00020000);
        if (a.out_f32) {
            const int n = nbase + 4 * q_l;
            unsigned voff = n < a.Cout ? (unsigned)(px_l * pix_bytes + n * 4) : 0x80000000u;
#pragma unroll
            for (int rd = 0; rd < rounds; ++rd) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(&stage[(rd * PXR + px_l) * STAGE_LD + 4 * q_l]);
#ifdef RPN_NOSTORE
                __builtin_amdgcn_raw_buffer_store_b128(v, ors, (unsigned)(lane * 16), 0, 0);
#else
                __builtin_amdgcn_raw_buffer_store_b128(v, ors, voff, 0, 0);
#endif
                voff += (unsigned)(PXR * pix_bytes);
            }
        } else {
            // a lane owns EIGHT channels of a pixel and writes their hi piece and their lo piece -- 32 contiguous bytes of the pixel's
            // SPLIT16 record -- from one read of the eight floats: 8 conversions to 16 bits, 8 back, 8 subtractions, 8 conversions
            // per 32 bytes.  (Rounds 1-5: a lane per 16-byte piece, hi or lo by lane parity -- both computed, one selected (8
            // v_cndmask), the same eight floats read by two lanes: 40 vector instructions and two LDS reads per 16 bytes.)
            constexpr int LPP = CW / 8;                                   // lanes per pixel: 8 | 4
            constexpr int PXR2 = 64 / LPP;                                // pixels per round: 8 | 16
            const int px2 = lane / LPP, q2 = lane % LPP;
            const int cl = q2 >> 1, hf = q2 & 1;                          // 16-channel slice of the wave's channels, its half
            const int n = nbase + cl * 16;
            unsigned voff = n < a.Cout ? (unsigned)(px2 * pix_bytes + (n >> 4) * 64 + hf * 32) : 0x80000000u;
            const int rounds2 = (1 << npx_log2) / PXR2;
#pragma unroll
            for (int rd = 0; rd < rounds2; ++rd) {
                float xs[8];
                const float *src = &stage[(rd * PXR2 + px2) * STAGE_LD + cl * 16 + hf * 8];
                const float4 v0 = *reinterpret_cast<const float4 *>(src);
                const float4 v1 = *reinterpret_cast<const float4 *>(src + 4);
                xs[0] = v0.x; xs[1] = v0.y; xs[2] = v0.z; xs[3] = v0.w;
                xs[4] = v1.x; xs[5] = v1.y; xs[6] = v1.z; xs[7] = v1.w;
                const u32x4 hi = __builtin_bit_cast(u32x4, split_piece<F16>(xs, false, a.status));
                const u32x4 lo = __builtin_bit_cast(u32x4, split_piece<F16>(xs, true, nullptr));
#ifdef RPN_NOSTORE
                __builtin_amdgcn_raw_buffer_store_b128(hi, ors, (unsigned)(lane * 32), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, ors, (unsigned)(lane * 32 + 16), 0, 0);
#else
                __builtin_amdgcn_raw_buffer_store_b128(hi, ors, voff, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, ors, voff + 16u, 0, 0);
#endif
                voff += (unsigned)(PXR2 * pix_bytes);
            }
        }
    };

    if constexpr (POOL) {
        const int OHo = a.H >> 1, OWo = a.W >> 1;     // RW == 2: rows (2wm, 2wm+1) are one pooling row pair
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r2 = 0; r2 < 2; ++r2) {
                    const float v0 = fmaxf(acc[hf][j][2 * r2], acc[hf][j][2 * r2 + 1]);            // row i = 0
                    const float v1 = fmaxf(acc[(MT - 2) + hf][j][2 * r2], acc[(MT - 2) + hf][j][2 * r2 + 1]);    // row i = 1
                    const int px2 = 8 * hf + 2 * kg + r2;                                          // pooled column 0..15
                    stage[px2 * STAGE_LD + j * 16 + lr] = fminf(fmaxf(fmaxf(v0, v1) * a.out_scale + bias_v[j], act_lo), act_hi);
                }
        wave_sync();
        store_stage(4, (oy0 + 2 * wm) >> 1, ox0 >> 1, OHo, OWo);
    } else {
#pragma unroll
        for (int i = 0; i < RW; ++i) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int px = 16 * hf + 4 * kg + r;
                        stage[px * STAGE_LD + j * 16 + lr] =
                            fminf(fmaxf(acc[i * 2 + hf][j][r] * a.out_scale + bias_v[j], act_lo), act_hi);
                    }
            wave_sync();
            if (stamp_base >= 0) RPN_STAMP_AT(stamp_base + 2 * i);
            store_stage(5, oy0 + RW * wm + i, ox0, a.H, a.W);
            wave_sync();
            if (stamp_base >= 0) RPN_STAMP_AT(stamp_base + 2 * i + 1);
        }
    }
}

// TH: tile rows (8 | 4); WN: waves along N (2 -> 128 channels, 1 -> 64); NW: waves (8 | 4).  Each wave owns
// RW = TH / (NW / WN) rows of 32 pixels x 64 channels.  <8,2,8>: one 136 KB workgroup per CU (large layers);
// <4,1,4>: 77 KB, two workgroups per CU (small feature maps).
template <int TH, int WN, int NW, bool F16, bool POOL>
__global__ void __launch_bounds__(64 * NW, NW == 8 ? 2 : 2)
conv3x3_split16_kernel(SplitConvArgs a, int tiles_x, int tiles_y, int n_tiles)
{
    constexpr int NT = 64 * NW, BN = 64 * WN;
    constexpr int WM = NW / WN, RW = TH / WM;          // rows of 32 pixels per wave
    constexpr int MT = RW * 2;                         // 16-pixel MFMA tiles per wave along M
    constexpr int HP = (TH + 2) * HW;                 // halo pixels
    constexpr int PPP = 8;                            // 16-byte pieces per 32-channel row
    constexpr int ABUF = HP * PPP + 8;                // + dummy slot for idle lanes
    constexpr int A_PIECES = HP * PPP;
    constexpr int A_ROUNDS = (A_PIECES + NT - 1) / NT;
    constexpr int A_RPS = (A_ROUNDS + 2) / 3, A_SLOTS = 3 * A_RPS;
    constexpr int B_PIECES = 3 * BN * PPP;            // one filter row of 32-channel weight rows
    constexpr int B_ROUNDS = B_PIECES / NT;
    constexpr int STAGE_LD = 64 + kStagePad;
    constexpr int LDS_PIPE = 2 * ABUF + B_PIECES;
    constexpr int LDS_STAGE = (NW * 32 * STAGE_LD * 4 + 15) / 16;
    constexpr int LDS_UINT4 = LDS_PIPE > LDS_STAGE ? LDS_PIPE : LDS_STAGE;
    static_assert(RW * WM == TH && RW >= 1 && B_PIECES % NT == 0 && (!POOL || RW == 2), "tile shape");

    __shared__ uint4 lds[LDS_UINT4];
    u32x4 *As = reinterpret_cast<u32x4 *>(lds);
    u32x4 *Bs = reinterpret_cast<u32x4 *>(lds) + 2 * ABUF;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;         // rows [RW*wm, +RW), channels [64wn, +64)
    const int lr = lane & 15, kg = lane >> 4;         // fragment row / k-group (8 channels) of this lane

    int nt, mt;
    {
        const int m_tiles = tiles_x * tiles_y * a.B;
        const int XN = n_tiles >= 8 ? 8 : (n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1)), XM = 8 / XN;
        const int NTl = (n_tiles + XN - 1) / XN;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        nt = (slot % NTl) * XN + (xcd % XN);
        mt = (slot / NTl) * XM + (xcd / XN);
        if (nt >= n_tiles || mt >= m_tiles) return;
    }
    const int tx = mt % tiles_x;
    mt /= tiles_x;
    const int ty = mt % tiles_y;
    const int img = mt / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TWS, n0 = nt * BN;
    RPN_STAMP_AT(0);
    RPN_STAMP_VAL(1, ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                         (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4));       // XCC_ID, HW_ID

    const int all_chunks = a.Cin >> 5;                // 32-channel slices
    int c_begin = (int)((long long)blockIdx.y * all_chunks / gridDim.y);        // split-K: this workgroup's slices
    int chunks = (int)((long long)(blockIdx.y + 1) * all_chunks / gridDim.y);   // (one past its last slice)
    int c_fold = -1;                                  // K tree, two leaves per workgroup: the first slice of the second leaf
    constexpr bool KT = TH == 4 && NW == 4 && !POOL;   // (the instantiation the K-tree launcher uses; the others have no registers for it)
    if (KT && a.ktree) {                              // (gridDim.y = 2 or 4: the launcher sends an unsplit tree layer elsewhere)
        const int per = 4 / (int)gridDim.y, l0 = (int)blockIdx.y * per;
        c_begin = ktree_cut(all_chunks, l0);
        chunks = ktree_cut(all_chunks, l0 + per);
        if (per == 2) c_fold = ktree_cut(all_chunks, l0 + 1);
    }
    const int steps = chunks * 3;
    const size_t in_pix_stride = (size_t)(a.Cin >> 4) * 4;
    const uint4 *__restrict__ xin = a.x + (size_t)img * a.H * a.W * in_pix_stride;

    constexpr unsigned kOob = 0x80000000u;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(xin), (short)0, (int)((size_t)a.H * a.W * in_pix_stride * 16), 0x00020000);
    unsigned a_goff[A_SLOTS];
    int a_loff[A_SLOTS];
#pragma unroll
    for (int R = 0; R < A_SLOTS; ++R) {
        const int e = R * NT + tid;
        const int pix = e >> 3, q = e & 7;            // q: piece of the pixel's 128-byte (2 x SPLIT16 record) slice
        const int hy = pix / HW, hx = pix - hy * HW;
        const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
        const bool piece = e < A_PIECES;
        const bool inimg = piece && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const int kgq = (q >> 2) * 2 + ((q >> 1) & 1), lo = q & 1;     // SPLIT16 record order -> (k-group, lo)
        a_loff[R] = piece ? (pix * PPP + ((lo * 4 + kgq) ^ halo_swz(hx))) : HP * PPP;
        a_goff[R] = inimg ? (unsigned)((((size_t)iy * a.W + ix) * in_pix_stride + q) * 16) : kOob;
    }
    u32x4 b_reg[B_ROUNDS];
    u32x4 a_reg[A_RPS];
#define RPN16_LOAD_B(STEP)                                                                                   \
    {                                                                                                        \
        const u32x4 *src_ = reinterpret_cast<const u32x4 *>(a.w) + ((size_t)(STEP) * 3 * a.cout_pad + n0) * PPP; \
        _Pragma("unroll") for (int i_ = 0; i_ < B_ROUNDS; ++i_) {                                            \
            const int e_ = tid + i_ * NT;                                                                    \
            const int t_ = e_ / (BN * PPP), rem_ = e_ - t_ * (BN * PPP);                                     \
            b_reg[i_] = src_[(size_t)t_ * a.cout_pad * PPP + rem_];                                          \
        }                                                                                                    \
    }
#define RPN16_STORE_B()                                                                                      \
    {                                                                                                        \
        _Pragma("unroll") for (int i_ = 0; i_ < B_ROUNDS; ++i_) {                                            \
            const int e_ = tid + i_ * NT;                                                                    \
            const int t_ = e_ / (BN * PPP), rem_ = e_ - t_ * (BN * PPP);                                     \
            Bs[t_ * BN * PPP + rem_] = b_reg[i_];       /* the packed weights already are the swizzled image */ \
        }                                                                                                    \
    }
#define RPN16_LOAD_A(CHUNK, R) \
    __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, a_goff[R], (CHUNK) * 128, 0))

    f32x4 acc[MT][4];                                 // [M-tile = row i * 2 + half][N-tile j]
    f32x4 leaf0[KT ? MT : 1][KT ? 4 : 1];            // (K tree: the finished first leaf of this workgroup's pair)
    (void)leaf0;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (KT) leaf0[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    int a_off[3][2];                                  // [tap column s][16-px half]: lane-constant
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int hx = 16 * hf + lr + s3;
            a_off[s3][hf] = hx * PPP + (kg ^ halo_swz(hx));
        }
    int b_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = wn * 64 + j * 16 + lr;
        b_off[j] = n * PPP + (kg ^ ((n >> 1) & 7));
    }

#pragma unroll
    for (int R = 0; R < A_SLOTS; ++R) As[a_loff[R]] = RPN16_LOAD_A(c_begin, R);
    RPN16_LOAD_B(3 * c_begin);
    RPN16_STORE_B();
    __syncthreads();
    RPN_STAMP_AT(2);

    int abuf = 0;
#pragma unroll 1
    for (int chunk = c_begin; chunk < chunks; ++chunk) {
        const int next_chunk = chunk + 1 < chunks ? chunk + 1 : chunk;
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            const int step = chunk * 3 + row;
            RPN16_LOAD_B(step + 1 < steps ? step + 1 : step);
#pragma unroll
            for (int q = 0; q < A_RPS; ++q) a_reg[q] = RPN16_LOAD_A(next_chunk, row * A_RPS + q);
            RPN_PIN_LOADS();

            const u32x4 *arow = As + (abuf * ABUF + (RW * wm + row) * HW * PPP);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                u32x4 ahi[MT], alo[MT], bhi[4], blo[4];
#pragma unroll
                for (int m = 0; m < MT; ++m) {            // m = i * 2 + half
                    const int idx = (m >> 1) * HW * PPP + a_off[s][m & 1];
                    ahi[m] = arow[idx];
                    alo[m] = arow[idx ^ 4];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bhi[j] = Bs[s * BN * PPP + b_off[j]];
                    blo[j] = Bs[s * BN * PPP + (b_off[j] ^ 4)];
                }
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[m][j] = mfma16<F16>(alo[m], bhi[j], acc[m][j]);
                        acc[m][j] = mfma16<F16>(ahi[m], blo[j], acc[m][j]);
                        acc[m][j] = mfma16<F16>(ahi[m], bhi[j], acc[m][j]);
                    }
            }
            __syncthreads();                              // every wave is done reading the weight buffer
            RPN16_STORE_B();
#pragma unroll
            for (int q = 0; q < A_RPS; ++q) As[(abuf ^ 1) * ABUF + a_loff[row * A_RPS + q]] = a_reg[q];
            __syncthreads();
        }
        abuf ^= 1;
        RPN_STAMP_AT(4 + chunk);
        if constexpr (KT) {
            if (chunk + 1 == c_fold) {                // K tree: the first leaf is complete
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        leaf0[m][j] = acc[m][j];
                        acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
            }
        }
    }
    if constexpr (KT) {
        if (c_fold >= 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][j] = leaf0[m][j] + acc[m][j];
        }
    }
#undef RPN16_LOAD_B
#undef RPN16_STORE_B
#undef RPN16_LOAD_A

    if (gridDim.y > 1) {                              // split-K: raw partial sums to this workgroup's slab
        SplitConvArgs ar = a;
        ar.bias = nullptr;
        ar.act = ACT_LINEAR;
        ar.out_f32 = 1;
        ar.out = reinterpret_cast<float *>(a.out) + (size_t)blockIdx.y * a.slab_floats;
        split16_epilogue<F16, POOL, RW, NW>(acc, reinterpret_cast<float *>(lds), ar, img, oy0, ox0, n0, wave, wm, wn, lane);
    } else {
        split16_epilogue<F16, POOL, RW, NW>(acc, reinterpret_cast<float *>(lds), a, img, oy0, ox0, n0, wave, wm, wn, lane);
    }
    RPN_STAMP_AT(3);
}

// ---- 16x16x32-MFMA variant: persistent workgroups, LDS-DMA pipeline ----------------------------------------------
// Same tile (8 x 32 px x 128 ch, 8 waves), same LDS images and the same products accumulated in the same order as
// conv3x3_split16_kernel<8, 2, 8>, with the staging pipeline and the tile loop rebuilt from in-kernel cycle stamps
// (scripts/stamp_probe.py) of that kernel: 18.7k cycles per 32-channel slice against 13.8k of MFMA issue, and 13k
// cycles per tile of prologue + epilogue + dispatch gap that nothing overlapped (one workgroup per CU).
//   * `buffer_load ... lds` (global -> LDS, no registers, no ds_write): one barrier per TAP and no exposed store phase
//     (before: 62 KB of ds_write_b128 at ~79 B/clk/CU between the two barriers of every filter row).  The weights of
//     tap t+3 are DMA'd into a 3-slot ring while tap t computes; the halo tile of the next slice in 6 pieces per wave
//     during taps 0..5 of the current slice (other halo buffer).  A wave issues them in the MIDDLE of its interval, behind
//     MFMAs, not at the head where all eight waves stood in front of their first MFMA together ("Issue sites" in the kernel).
//   * the MFMA fragments of tap t+1 are read into a second register set during tap t (one read behind each of the 16
//     chain-head MFMAs), so the matrix pipe does not wait for LDS behind a barrier.
//   * persistent workgroups (one per CU) walk the tiles of their XCD: the tap stream simply continues into the next
//     tile (its halo tile and first weights are DMA'd during the last slice of the current one), so there is no
//     prologue and no dispatch gap between tiles.
//   * the epilogue stages through halo buffer 1 + the LDS left over (dead until the next tile's first interval refills
//     them), one workgroup barrier per tile.  (Tried and dropped: swapped MFMA operands -- weights as A, pixels as B, so
//     that a lane's 4 accumulator registers are 4 consecutive CHANNELS of one pixel -- with 8-byte stores straight from
//     registers: 9.8k against 6.5k cycles per tile, the store issue became the limit.)
// Hazards, by the rule "read a DMA'd buffer one interval after the wait that retires it":
//   RAW  weights(t+2) (issued in interval t-1) are retired by the counted vmcnt at the end of interval t (which leaves
//        only interval t's own DMAs in flight), then the barrier; read in interval t+1.  Halo pieces likewise (issued in
//        intervals 0..5, first read in interval 8).
//   WAR  the ring slot of tap t+3 is the slot of tap t, whose fragments were read in interval t-1 and retired by the
//        lgkmcnt(0) in front of that interval's barrier.  The other halo buffer was last read in interval 7 of the
//        previous slice.
// (Tried: a 6-slot ring at 64 channels per tile -- weights four intervals ahead -- and the halo pieces two per tap behind
// the weights of taps 0..2 so that the in-order counter gives them two intervals to land: no gain on any layer, the DMA
// latency is already covered.)
// The weights in HBM are already the swizzled LDS image ("split32" packing), so their DMA is a linear copy; the halo
// tile's swizzle is applied on the per-lane SOURCE address (the LDS side of a DMA is lane-linear).  Out-of-image halo
// pixels are out-of-range buffer offsets: the DMA writes zeros for them (checked: scripts/micro/dma_oob.hip).
// Needs an even number of 32-channel slices (the body is unrolled over two slices = 18 taps so that register sets,
// halo buffers and ring slots are all compile-time) and an input tensor below 2 GiB (32-bit buffer offsets).
#ifndef RPN_DMA_SCHED
#define RPN_DMA_SCHED 1
#endif
#define RPN_LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))

// Tile schedule of a persistent workgroup: blockIdx & 7 labels the XCD; an XCD owns n-tiles (xcd % XN) + XN * k and
// walks its slots.  next(): first real tile at or after `slot` (slots past the edge of the XN x XM ownership grid are
// skipped); -1: none.  Tiles are 8 rows x 32 pixels x bn channels.
struct TileWalk {
    int n_tiles, m_tiles, tiles_x, tiles_y, XN, XM, NTl, n_slots, xcd, slot_stride, bn;
    // tile of slot `slot` of this XCD label; false: the slot lies past the edge of the XN x XM ownership grid
    __device__ __forceinline__ bool decode(int slot, int &img, int &oy0, int &ox0, int &n0) const
    {
        const int nt = (slot % NTl) * XN + (xcd % XN);
        int mt = (slot / NTl) * XM + (xcd / XN);
        if (nt >= n_tiles || mt >= m_tiles) return false;
        const int tx = mt % tiles_x;
        mt /= tiles_x;
        const int ty = mt % tiles_y;
        img = mt / tiles_y;
        oy0 = ty * 8; ox0 = tx * TWS; n0 = nt * bn;
        return true;
    }
    // static schedule: first real tile at or after `slot`, stepping by the number of workgroups of this label; -1: none
    __device__ __forceinline__ int next(int slot, int &img, int &oy0, int &ox0, int &n0) const
    {
        for (; slot < n_slots; slot += slot_stride)
            if (decode(slot, img, oy0, ox0, n0)) return slot;
        return -1;
    }
    // dynamic schedule (one thread): given a ticket drawn from the label's queue, draw on until it names a real tile;
    // >= n_slots: the queue is exhausted
    // (the queue hands out the slots after the first `slot_stride`: those are every workgroup's statically assigned
    // first tile, so that a launch with one tile per workgroup cannot leave workgroups empty-handed)
    __device__ __forceinline__ int settle(int ticket, unsigned *queue) const
    {
        int img, oy0, ox0, n0, slot = ticket + slot_stride;
        while (slot < n_slots && !decode(slot, img, oy0, ox0, n0)) slot = (int)atomicAdd(queue, 1u) + slot_stride;
        return slot;
    }
};

// Byte offset (inside the SPLIT16 input tensor) of the 16-byte piece that lane `lane` of halo wave-instruction
// k = j * NW + wave DMAs: LDS piece e = 64 k + lane = halo pixel * 8 + physical slot; the LDS image's XOR swizzle is applied
// here, on the source side.  Out-of-image pixels and the padding lanes get an out-of-range offset (the DMA writes zeros).
template <int NW, int A_INSTR, int A_PIECES>
__device__ __forceinline__ unsigned halo_source_offset(int j, int wave, int lane, int im, int y0, int x0, int H, int W,
                                                       int in_pix_stride)
{
    int ln = lane;
    asm volatile("" : "+v"(ln));                      // opaque: keeps the lane-constant parts from being hoisted
    int k = j * NW + wave;                            // out of the tap loop into long-lived registers
    if (k >= A_INSTR) k -= A_INSTR;                   // surplus instructions of the last round re-fetch pieces 0, 1, ...
    const int e = k * 64 + ln;
    const int pix = e >> 3, ps = e & 7;
    const int hy = pix / HW, hx = pix - hy * HW;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool in = e < A_PIECES && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const int lg = ps ^ halo_swz(hx);              // logical piece: lo * 4 + k-group
    const int q = (((lg & 3) >> 1) << 2) | ((lg & 1) << 1) | (lg >> 2);   // its place in the slice's SPLIT16 records
    return in ? (unsigned)((((im * H + iy) * W + ix) * in_pix_stride + q) * 16) : 0x80000000u;
}

template <bool F16, bool POOL, int BN, bool KTREE = false>
__global__ void __launch_bounds__(512, 2)
conv3x3_split16_dma_kernel(SplitConvArgs a, int tiles_x, int tiles_y, int n_tiles)
{
    static_assert(!KTREE || (BN == 64 && !POOL), "K tree: the 64-wide tile has the registers for two more accumulator sets");
    constexpr int TH = 8, NW = 8, WN = 2, RW = 2, MT = 4, PPP = 8;
    constexpr int NJ = BN / (16 * WN);                 // 16-channel MFMA tiles per wave: 4 (BN = 128) or 2 (BN = 64)
    constexpr int B_PER_WAVE = BN * PPP / 64 / NW;     // weight DMA instructions per wave and tap: 2 or 1
    constexpr int HP = (TH + 2) * HW;                  // 340 halo pixels
    constexpr int A_INSTR = (HP * PPP + 63) / 64;      // 43 wave-instructions (1 KB each) per halo tile
    constexpr int ABUF = A_INSTR * 64;                 // pieces per halo buffer (the tail of the last KB is padding)
    constexpr int A_PER_WAVE = (A_INSTR + NW - 1) / NW;   // 6 (the 5 surplus ones of the last round duplicate pieces 0..4)
    constexpr int BSLOT = BN * PPP;                    // pieces per ring slot (one tap: 16 KB)
    // LDS map (16-byte pieces): halo buffer 0 | weight ring | 1 KB scratch (tile queue) | halo buffer 1 | spare.  At the end of a tile halo
    // buffer 1 is dead (an even number of slices), so buffer 1 + spare is the epilogue's staging area: 8 waves x 32 px x
    // 68 floats = 69632 bytes = exactly what is left of the CU's 160 KB.
    constexpr int B_AT = ABUF, DUMP = B_AT + 3 * BSLOT, A1_AT = DUMP + 64;
    constexpr int STAGE_PIECES = NW * 32 * (16 * NJ + kStagePad) * 4 / 16;
    constexpr int LDS_UINT4 = A1_AT + (ABUF > STAGE_PIECES ? ABUF : STAGE_PIECES);
    static_assert(A_PER_WAVE <= 9 && RW * (NW / WN) == TH && MT == 2 * RW && LDS_UINT4 * 16 <= 160 * 1024 &&
                      (BN == 128 || BN == 64), "tile shape");

    __shared__ uint4 lds[LDS_UINT4];
    u32x4 *As = reinterpret_cast<u32x4 *>(lds);       // halo buffer b at As + b * A1_AT
    u32x4 *Bs = reinterpret_cast<u32x4 *>(lds) + B_AT;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lr = lane & 15, kg = lane >> 4;

    // tile schedule: blockIdx & 7 labels the XCD; an XCD owns n-tiles (xcd % XN) + XN * k and walks its slots
    const int m_tiles = tiles_x * tiles_y * a.B;
    const int XN = n_tiles >= 8 ? 8 : (n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1)), XM = 8 / XN;
    const int NTl = (n_tiles + XN - 1) / XN, MTl = (m_tiles + XM - 1) / XM;
    const int xcd = blockIdx.x & 7;
    const int slot_stride = gridDim.x >> 3;
    const TileWalk walk{n_tiles, m_tiles, tiles_x, tiles_y, XN, XM, NTl, NTl * MTl, xcd, slot_stride, BN};
#define next_tile(SLOT, IMG, OY0, OX0, N0) walk.next((SLOT), (IMG), (OY0), (OX0), (N0))

    const int all_chunks = a.Cin >> 5;                // 32-channel slices (even)
    // K tree split two ways (gridDim.y == 2; launch_conv3x3_split16_ksplit on grids of 65 .. 128 tiles): workgroup y walks the
    // slices [cb, cb + chunks) = leaves 2y, 2y + 1 (ktree_cut's middle cut is even: whole slice pairs) and writes the RAW sum of
    // its two leaves to slab y (the host passes no bias, a linear activation, float32 output); the RPN head adds the slabs
    int cb = 0, chunks = all_chunks;
    if constexpr (KTREE) {
        if (gridDim.y == 2) {
            const int mid = ktree_cut(all_chunks, 2);
            cb = blockIdx.y ? mid : 0;
            chunks = blockIdx.y ? all_chunks - mid : mid;
            a.out = reinterpret_cast<float *>(a.out) + (size_t)blockIdx.y * a.slab_floats;
        }
    }
    const int total_taps = chunks * 9, tap0 = cb * 9;
    const int in_pix_stride = (a.Cin >> 4) * 4;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(a.x), (short)0, (int)((size_t)a.B * a.H * a.W * in_pix_stride * 16), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(a.w), (short)0, (int)((size_t)all_chunks * 9 * a.cout_pad * 128), 0x00020000);
    const int w_tap_bytes = a.cout_pad * 128;

    // halo DMA: wave-instruction k = j * 8 + wave fills LDS pieces [64k, 64k + 64); piece e = pixel * 8 + physical slot.
    // The six source offsets of a tile's halo (a_goff) are computed once per tile: in the prologue, and for the next tile at tap 9
    // of the last slice, at the halo piece's issue site (RPN_DMA_HALO: behind MFMA 4 NJ of half 1; ~25 VALU operations each).
#define halo_goff(J, IM, Y0, X0) halo_source_offset<NW, A_INSTR, HP * PPP>((J), wave, lane, (IM), (Y0), (X0), a.H, a.W, in_pix_stride)
    const unsigned b_voff = (unsigned)(((B_PER_WAVE * wave) * 64 + lane) * 16);   // this wave's share of a tap's weights

    // (WV: the wave's index -- `wave`, or an opaque copy of it where the LDS address is to be computed at the DMA and not kept
    // in a scalar register of its own through the kernel: 15 such addresses otherwise)
#define RPN_DMA_A(J, GOFF, SOFF, BUF, WV)                                                                         \
    {                                                                                                             \
        const int k0_ = (J) * NW + (WV), k_ = k0_ < A_INSTR ? k0_ : k0_ - A_INSTR;   /* surplus: a duplicate */         \
        u32x4 *dst_ = As + (BUF) * A1_AT + k_ * 64;                                                               \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, RPN_LDS_PTR(dst_), 16, (GOFF), (SOFF), 0, 0);             \
    }
#define RPN_DMA_B1(SOFF, SLOT, PIECE, WV)    /* piece PIECE (0 | 1) of this wave's share of a tap's weights */      \
    {                                                                                                             \
        u32x4 *dst_ = Bs + (SLOT) * BSLOT + (B_PER_WAVE * (WV)) * 64;                                             \
        /* the instruction offset advances BOTH the global and the LDS address */                                \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, RPN_LDS_PTR(dst_), 16, b_voff, (SOFF), (PIECE) * 1024, 0); \
    }
#define RPN_DMA_B(SOFF, SLOT)                                                                                     \
    {                                                                                                             \
        RPN_DMA_B1(SOFF, SLOT, 0, wave);                                                                          \
        if constexpr (B_PER_WAVE == 2) RPN_DMA_B1(SOFF, SLOT, 1, wave);                                           \
    }

    int a_off[3][2];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int hx = 16 * hf + lr + s3;
            a_off[s3][hf] = hx * PPP + (kg ^ halo_swz(hx));
        }
    int b_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = wn * (16 * NJ) + j * 16 + lr;
        b_off[j] = n * PPP + (kg ^ ((n >> 1) & 7));
    }

    // Tile schedule.  Static: workgroup w of a label takes slots w, w + stride, ...  Dynamic (a.sched != null): only the
    // first tile is w; every further tile is drawn from a queue shared by the label's workgroups -- the ticket is drawn
    // (one atomic, not waited for) when a tile starts and turned into the next tile at taps 4..6, in time for the last
    // slice's look-ahead DMAs -- so that a CU that starts late or shares its time (another stream's kernel holding LDS:
    // the NMS, an RCCL kernel) takes fewer tiles instead of stalling a fixed share of the layer.
    const bool dyn = a.sched != nullptr;
    int *tile_q = reinterpret_cast<int *>(lds + DUMP);           // [tile parity]: the slot drawn for the next tile
    int img = 0, oy0 = 0, ox0 = 0, n0 = 0;
    int cur;
    if (dyn) {
        cur = blockIdx.x >> 3;
        if (!walk.decode(cur, img, oy0, ox0, n0)) {              // first slot on the ownership grid's padding (rare)
            if (tid == 0) tile_q[0] = walk.settle((int)atomicAdd(a.sched + xcd, 1u), a.sched + xcd);
            __syncthreads();
            cur = __builtin_amdgcn_readfirstlane(tile_q[0]);
            __syncthreads();
            if (cur >= walk.n_slots || !walk.decode(cur, img, oy0, ox0, n0)) cur = -1;
        }
    } else {
        cur = next_tile(blockIdx.x >> 3, img, oy0, ox0, n0);
    }
    // Every workgroup counts itself out, the last one re-arms the counters for the next launch on this stream.  Two
    // levels (per label, then one count of finished labels): 256 workgroups finishing together on ONE counter cost
    // ~6 us per launch in same-address atomics.
#define RPN_SCHED_EXIT()                                                                                          \
    if (dyn && tid == 0) {                                                                                        \
        __threadfence();                                                                                          \
        if (atomicAdd(a.sched + 8 + xcd, 1u) == (gridDim.x >> 3) - 1 && atomicAdd(a.sched + 16, 1u) == 7) {       \
            _Pragma("unroll") for (int i_ = 0; i_ < 17; ++i_) a.sched[i_] = 0u;                                   \
        }                                                                                                         \
    }
    if (cur < 0) {
        RPN_SCHED_EXIT();
        return;
    }
    RPN_STAMP_AT(0);
    RPN_STAMP_VAL(1, ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                         (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4));       // XCC_ID, HW_ID
    RPN_STAMP_WAVE_HWID();

    // Issue sites of the tap loop's DMAs.  The pieces of an interval may be issued anywhere between its two barriers: the ring slot
    // of tap t+3 was last read in interval t-1 and nobody reads the other halo buffer during the slice (hazards above); the counted
    // wait at the interval's end stays exact as long as every wave issues the interval's pieces in front of it.  At the head of the
    // interval, where all eight waves issued them at once in front of their first MFMA, they cost ~180 cycles per wave and tap.  Now
    // the head holds the first fragment read and the first MFMA only:
    //   weights (1 or 2 pieces) behind the 2 NJ chain-head MFMAs of half 0 (RPN_DMA_WEIGHTS),
    //   the halo piece (taps 0..5) behind MFMA 4 NJ of half 1 (RPN_DMA_HALO; the 128-wide tile has no fragment read left there).
    // The scalar address arithmetic sits at the sites, too: each site is a scheduling region of its own (sched_barrier), entered
    // through a scalar branch on `gt >= 0`, which always holds.  The branch is there for the register allocator: with the 18 taps
    // in ONE basic block and the sites inside it, hipcc spilled 160-184 VGPRs to scratch (and scratch loads share vmcnt with the
    // DMAs); cut into blocks at the sites the kernel needs fewer registers than before (224 against 249 at 128 wide).  The LDS
    // addresses are computed at the site from an opaque copy of the wave's index: hoisted, they held 15 scalar registers.
    // All of this rests on hipcc not proving `gt >= 0` (gt starts at 3 and only loses total_taps after gaining as many).  A compiler
    // that folds the branch brings the spills back: tests/test_host.py::test_kernel_register_budgets (no scratch, <= 256 VGPRs, the
    // SGPR spill budgets) is the guard, and the fix is then another condition the compiler cannot see through.
#ifdef RPN_EXP_NO_DMA
#define RPN_TAP_DMA_B1(SOFF, SLOT, PIECE, WV) ((void)(SOFF))
#define RPN_TAP_DMA_A(J, GOFF, SOFF, BUF, WV) ((void)(GOFF))
#else
#define RPN_TAP_DMA_B1 RPN_DMA_B1
#define RPN_TAP_DMA_A RPN_DMA_A
#endif
#define RPN_DMA_WEIGHTS()   /* weights of tap t+3: this tile's, or the first taps of the next tile (or a harmless re-load) */  \
    {                                                                                                              \
        int wv_ = wave;                                                                                            \
        asm volatile("" : "+s"(wv_));                                                                              \
        if (gt >= 0) {                                                                                             \
            int tap_ = gt, nb_ = n0;                                                                               \
            if (gt >= total_taps) {                                                                                \
                if (nxt >= 0) { tap_ = gt - total_taps; nb_ = nn0; }                                               \
                else tap_ = total_taps - 1;                                                                        \
            }                                                                                                      \
            const int soff_ = (tap0 + tap_) * w_tap_bytes + nb_ * (PPP * 16);                                      \
            RPN_TAP_DMA_B1(soff_, s9 % 3, 0, wv_);                                                                 \
            if constexpr (B_PER_WAVE == 2) RPN_TAP_DMA_B1(soff_, s9 % 3, 1, wv_);                                  \
        }                                                                                                          \
    }
#define RPN_DMA_HALO()      /* halo piece s9 of the next slice: this tile's, or slice 0 of the next tile */                 \
    {                                                                                                              \
        int wv_ = wave;                                                                                            \
        asm volatile("" : "+s"(wv_));                                                                              \
        if (T == 9 && nxt >= 0 && pair == (chunks >> 1) - 1) {    /* last slice of the tile: from here on the halo */ \
            _Pragma("unroll") for (int j = 0; j < A_PER_WAVE; ++j) a_goff[j] = halo_goff(j, nimg, noy0, nox0);     /* of the NEXT tile */ \
        }                                                                                                          \
        if (s9 < A_PER_WAVE && gt >= 0) {                                                                          \
            const int nc_ = 2 * pair + c2 + 1;                                                                     \
            RPN_TAP_DMA_A(s9, a_goff[s9], (cb + (nc_ < chunks ? nc_ : (nxt >= 0 ? 0 : chunks - 1))) * 128, (c2 + 1) & 1, wv_); \
        }                                                                                                          \
    }
    // sched_group_barrier pipelines of the segments between the sites (0x100: one ds_read, 0x008: MFMAs); a pipeline takes its
    // instructions from the code ABOVE it in its region, so each stands at the end of its segment
#if RPN_DMA_SCHED
#define RPN_SCHED_CUT() __builtin_amdgcn_sched_barrier(0)
#define RPN_G_RM(NR, NM)                                                                                           \
    _Pragma("unroll") for (int q_ = 0; q_ < (NR); ++q_) {                                                          \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                         \
        __builtin_amdgcn_sched_group_barrier(0x008, (NM), 0);                                                      \
    }
#define RPN_G00()       /* half 0, MFMAs [0, 2 NJ): a read of row 1's pixels behind each of the first four */       \
    {                                                                                                              \
        RPN_G_RM(4, 1);                                                                                            \
        if constexpr (2 * NJ - 4 > 0) __builtin_amdgcn_sched_group_barrier(0x008, 2 * NJ - 4, 0);                  \
    }
#define RPN_GM() __builtin_amdgcn_sched_group_barrier(0x008, 4 * NJ, 0)     /* half 0, MFMAs [2 NJ, 6 NJ): bare */
#define RPN_G10()       /* half 1, MFMAs [0, 4 NJ): the next tap's weights, a read per MFMA, then its row-0 pixels, one per two */ \
    {                                                                                                              \
        RPN_G_RM(2 * NJ, 1);                                                                                       \
        RPN_G_RM((NJ < 4 ? NJ : 4), 2);                                                                            \
        if constexpr (NJ > 4) __builtin_amdgcn_sched_group_barrier(0x008, 2 * (NJ - 4), 0);                        \
    }
#define RPN_G12()       /* half 1, MFMAs [4 NJ, 6 NJ): the rest of those reads (NJ < 4) */                           \
    {                                                                                                              \
        RPN_G_RM((NJ < 4 ? 4 - NJ : 0), 2);                                                                        \
        if constexpr (NJ - (NJ < 4 ? 4 - NJ : 0) > 0)                                                              \
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * (NJ - (NJ < 4 ? 4 - NJ : 0)), 0);                      \
    }
#else
#define RPN_SCHED_CUT() ((void)0)
#define RPN_G00() ((void)0)
#define RPN_GM() ((void)0)
#define RPN_G10() ((void)0)
#define RPN_G12() ((void)0)
#endif

    // Fragment registers.  The interval of a tap is worked in two halves (the wave's first / second pixel row) so that
    // only the weight fragments are double-buffered: fx0 / fx1 hold [hi, lo] of the two 16-pixel tiles of row 0 / 1.
    //   half 0: MFMAs of row 0 (fx0, fw[cur]); reads: fx1 of THIS tap
    //   half 1: MFMAs of row 1 (fx1, fw[cur]); reads: fw[next] and fx0 of the NEXT tap
    u32x4 fx0[4], fx1[4], fw[2][2 * NJ];                   // fx: [16-px half * 2 + (0 hi | 1 lo)];  fw: [set][j * 2 + (0 hi | 1 lo)]
#define RPN_X_ADDR(BUF, ROW, S, I, II)   /* row I of the wave, element II = half * 2 + lohi */                       \
    (As[(BUF) * A1_AT + (RW * wm + (ROW) + (I)) * HW * PPP + (a_off[S][(II) >> 1] ^ (((II) & 1) ? 4 : 0))])
#define RPN_W_ADDR(S, II)                /* element II = j * 2 + lohi */                                           \
    (Bs[(S) * BSLOT + (b_off[(II) >> 1] ^ (((II) & 1) ? 4 : 0))])

    // ---- prologue (first tile only): halo tile of slice 0, weights of taps 0..2, first fragments of tap 0 -------
    unsigned a_goff[A_PER_WAVE];                       // halo source offsets of the tile whose halo is being fetched
#pragma unroll
    for (int j = 0; j < A_PER_WAVE; ++j) a_goff[j] = halo_goff(j, img, oy0, ox0);
#pragma unroll
    for (int j = 0; j < A_PER_WAVE; ++j) RPN_DMA_A(j, a_goff[j], cb * 128, 0, wave);
#pragma unroll
    for (int t = 0; t < 3; ++t) RPN_DMA_B((tap0 + t) * w_tap_bytes + n0 * (PPP * 16), t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 2 * NJ; ++i) fw[0][i] = RPN_W_ADDR(0, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) fx0[i] = RPN_X_ADDR(0, 0, 0, 0, i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                      // ring slot 0 may now be overwritten (tap 3)

    int gt = 3;                                        // next tap to DMA, counted from the current tile's tap 0
    int tile_no = 0;
    for (;;) {
        int nimg = 0, noy0 = 0, nox0 = 0, nn0 = 0;
        int nxt = -1;
        unsigned ticket = 0;
        if (dyn) {
            if (tid == 0) ticket = atomicAdd(a.sched + xcd, 1u);     // for the next tile; resolved at taps 4..6 below
        } else {
            nxt = next_tile(cur + slot_stride, nimg, noy0, nox0, nn0);
        }
        f32x4 acc[MT][NJ];
        f32x4 t01[KTREE ? MT : 1][KTREE ? NJ : 1], t23[KTREE ? MT : 1][KTREE ? NJ : 1];     // K tree (SplitConvArgs::ktree): l0 + l1, l2
        (void)t01; (void)t23;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
        for (int pair = 0; pair < (chunks >> 1); ++pair) {
#pragma unroll
            for (int T = 0; T < 18; ++T) {            // tap T of this pair of slices; everything below is static in T
                const int c2 = T / 9, s9 = T % 9;
                const int CS = T & 1, CB = c2 & 1, CR = s9 / 3, CC = s9 % 3;                       // this tap
                const int NS = (T + 1) & 1, NB = ((T + 1) / 9) & 1, NR = ((T + 1) % 9) / 3, NC = ((T + 1) % 9) % 3;   // next
                if (dyn && pair == 0) {     // (nothing before tap 9 of the last slice needs to know the next tile)
                    if (T == 4 && tid == 0) tile_q[tile_no & 1] = walk.settle((int)ticket, a.sched + xcd);
                    if (T == 6) {           // two barriers later
                        const int sl = __builtin_amdgcn_readfirstlane(tile_q[tile_no & 1]);
                        nxt = (sl < walk.n_slots && walk.decode(sl, nimg, noy0, nox0, nn0)) ? sl : -1;
                    }
                }
                // ---- half 0: row 0.  Program order = intended issue order: a fragment read behind each of the first MFMAs
#pragma unroll
                for (int i = 0; i < 2 * NJ; ++i) {    // chain heads (x lo * w hi) of tiles (m = i / NJ, j = i % NJ)
#ifndef RPN_EXP_NO_LDSREAD
                    if (i < 4) fx1[i] = RPN_X_ADDR(CB, CR, CC, 1, i);
#endif
                    acc[i / NJ][i % NJ] = mfma16<F16>(fx0[2 * (i / NJ) + 1], fw[CS][2 * (i % NJ)], acc[i / NJ][i % NJ]);
                }
                RPN_G00();
                RPN_SCHED_CUT();
                RPN_DMA_WEIGHTS();
                RPN_SCHED_CUT();
#pragma unroll
                for (int i = 0; i < 2 * NJ; ++i) {
                    acc[i / NJ][i % NJ] = mfma16<F16>(fx0[2 * (i / NJ)], fw[CS][2 * (i % NJ) + 1], acc[i / NJ][i % NJ]);   // x hi * w lo
                    acc[i / NJ][i % NJ] = mfma16<F16>(fx0[2 * (i / NJ)], fw[CS][2 * (i % NJ)], acc[i / NJ][i % NJ]);       // x hi * w hi
                }
                RPN_GM();
                RPN_SCHED_CUT();
                // ---- half 1: row 1; the next tap's weights and row-0 pixels arrive meanwhile
#pragma unroll
                for (int i = 0; i < 2 * NJ; ++i) {
#ifndef RPN_EXP_NO_LDSREAD
                    fw[NS][i] = RPN_W_ADDR(NC, i);
#else
                    fw[NS][i] = fw[CS][i];
#endif
                    acc[2 + i / NJ][i % NJ] = mfma16<F16>(fx1[2 * (i / NJ) + 1], fw[CS][2 * (i % NJ)], acc[2 + i / NJ][i % NJ]);
                }
#pragma unroll
                for (int i = 0; i < 2 * NJ; ++i) {
                    if (i == NJ) {
                        RPN_G10();
                        RPN_SCHED_CUT();
                        RPN_DMA_HALO();
                        RPN_SCHED_CUT();
                    }
#ifndef RPN_EXP_NO_LDSREAD
                    if (i < 4) fx0[i] = RPN_X_ADDR(NB, NR, NC, 0, i);
#endif
                    acc[2 + i / NJ][i % NJ] = mfma16<F16>(fx1[2 * (i / NJ)], fw[CS][2 * (i % NJ) + 1], acc[2 + i / NJ][i % NJ]);
                    acc[2 + i / NJ][i % NJ] = mfma16<F16>(fx1[2 * (i / NJ)], fw[CS][2 * (i % NJ)], acc[2 + i / NJ][i % NJ]);
                }
                RPN_G12();
                RPN_SCHED_CUT();                       // (register-only MFMAs would otherwise sink below the barrier)
                ++gt;
                // Leave exactly this interval's own DMAs in flight.  Not in a tile's first interval: what it needs (tap 2) was
                // retired by the vmcnt(0) in front of the previous tile's epilogue (or by the prologue), and the in-order
                // counter would otherwise make the wave wait for that epilogue's global stores -- all 256 workgroups
                // finish their tiles together, so those stores are a burst (stamps: 12.9k cycles of epilogue in steady
                // state against 6.5k on a workgroup's first tile).  The stores now have two intervals to drain.
#ifdef RPN_EXP_HALF_BARRIERS                /* timing experiment only (results are wrong): a barrier every second tap */
                if ((T & 1) == 0) continue;
#endif
                if (T == 0 && pair == 0) {
                } else if constexpr (B_PER_WAVE == 2) {
                    if (s9 < A_PER_WAVE) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                } else {
                    if (s9 < A_PER_WAVE) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
#if RPN_DMA_SCHED
                __builtin_amdgcn_sched_barrier(0);
#endif
                if (s9 == 8 && tile_no == 1) RPN_STAMP_AT(4 + 2 * pair + c2);   // (second tile: steady state)
                if constexpr (KTREE) {      // a leaf ends behind slice k * slices / 4 (slices >= 8: every leaf has two or more)
                    if (s9 == 8) {          // (tap 8's MFMAs are all issued above; tap 9's fragments are in registers already)
                        const int done = cb + 2 * pair + c2 + 1;     // slices of the LAYER finished
                        const bool e0 = done == ktree_cut(all_chunks, 1), e1 = done == ktree_cut(all_chunks, 2),
                                   e2 = done == ktree_cut(all_chunks, 3);
                        if (e0 || e1 || e2) {
#pragma unroll
                            for (int m = 0; m < MT; ++m)
#pragma unroll
                                for (int j = 0; j < NJ; ++j) {
                                    if (e0) t01[m][j] = acc[m][j];
                                    else if (e1) t01[m][j] = t01[m][j] + acc[m][j];
                                    else t23[m][j] = acc[m][j];
                                    acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                                }
                        }
                    }
                }
            }
        }
        if constexpr (KTREE) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if (gridDim.y == 2) acc[m][j] = blockIdx.y == 0 ? t01[m][j] : t23[m][j] + acc[m][j];   // l0 + l1 | l2 + l3
                    else acc[m][j] = t01[m][j] + (t23[m][j] + acc[m][j]);
                }
        }
        // The first fragments of the next tile's tap 0 are already in registers and its DMAs are in flight (halo buffer 0,
        // the weight ring): the epilogue stages through halo buffer 1 + the spare LDS, both dead until the next tile's
        // first interval starts to refill buffer 1 -- hence one workgroup barrier per tile.
        if (tile_no < 2) RPN_STAMP_AT(20 + 6 * tile_no);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last interval's weight DMAs (issued a whole interval ago)
        if (tile_no < 2) RPN_STAMP_AT(21 + 6 * tile_no);
#ifdef RPN_EXP_NO_EPILOGUE                  /* timing experiment only: the accumulators are kept alive, nothing is written */
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(acc[m][j]));
#elif defined(RPN_STAMP)
        split16_epilogue<F16, POOL, RW, NW, NJ>(acc, reinterpret_cast<float *>(lds + A1_AT), a, img, oy0, ox0, n0, wave, wm, wn, lane,
                                                tile_no < 2 ? 22 + 6 * tile_no : -1);
#else
        split16_epilogue<F16, POOL, RW, NW, NJ>(acc, reinterpret_cast<float *>(lds + A1_AT), a, img, oy0, ox0, n0, wave, wm, wn, lane);
#endif
        if (tile_no == 1) RPN_STAMP_AT(3);
        if (nxt < 0) break;
        __builtin_amdgcn_s_barrier();
        if (tile_no == 0) RPN_STAMP_AT(2);
        cur = nxt; img = nimg; oy0 = noy0; ox0 = nox0; n0 = nn0;
        gt -= total_taps;
        ++tile_no;
    }
#undef RPN_X_ADDR
#undef RPN_W_ADDR
#undef next_tile
#undef halo_goff
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped tail DMAs still target this workgroup's LDS
    RPN_SCHED_EXIT();
#undef RPN_SCHED_EXIT
#undef RPN_DMA_A
#undef RPN_DMA_B
#undef RPN_DMA_B1
#undef RPN_TAP_DMA_B1
#undef RPN_TAP_DMA_A
#undef RPN_DMA_WEIGHTS
#undef RPN_DMA_HALO
#undef RPN_SCHED_CUT
#undef RPN_G_RM
#undef RPN_G00
#undef RPN_GM
#undef RPN_G10
#undef RPN_G12
}

// 16x16x32-MFMA kernel (weights in "split32" packing).  Needs Cin % 32 == 0 and cout_pad % 128 == 0.
// Tile-queue counters of the persistent kernel's dynamic schedule: 17 unsigned per stream (launches on one stream are
// serialised and every launch leaves them zero), allocated and zeroed at the stream's first launch.  Null = static tile
// schedule: the default.  RPN_S16_DYN=1 turns the dynamic schedule on (not under stream capture at a stream's first
// launch, where nothing may be allocated).  Measured on VGG16, batch 8: alone on the GPU the dynamic schedule costs 2 %
// (2760 vs 2814 images/s: a device-scope atomic takes microseconds on this multi-XCD part, and the in-order vmcnt makes
// the drawing wave wait for it one interval later); it pays when another stream's kernel holds CUs during a persistent
// layer (block1_conv2 on this kernel beside the overlapped NMS: 2800 vs 2737 images/s with the static schedule).
static unsigned *sched_counters(hipStream_t s)
{
    static const int dyn = RPN_KNOB("RPN_S16_DYN", 0);
    if (!dyn) return nullptr;
    static std::mutex mu;
    static std::unordered_map<hipStream_t, unsigned *> pool;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find(s);
    if (it != pool.end()) return it->second;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
    unsigned *p = nullptr;
    if (hipMalloc(&p, 128) != hipSuccess || hipMemset(p, 0, 128) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    pool[s] = p;
    return p;
}

const char *conv3x3_split16_variant(int B, int H, int W, int Cin, int Cout, int cout_pad, bool pool)
{
    if (Cin % 32 != 0 || Cout % 16 != 0 || cout_pad % 64 != 0 || cout_pad < Cout) return nullptr;
    static const int dma_mode = RPN_LAB_KNOB("RPN_S16_DMA", 1);
    const long long big_blocks = (long long)((W + 31) / 32) * ((H + 7) / 8) * B * ((Cout + 127) / 128);
    const bool dma_ok = dma_mode && Cin % 64 == 0 && (long long)B * H * W * Cin * 4 < 0x7fffffffll &&
                        (long long)(Cin / 32) * 9 * cout_pad * 128 < 0x7fffffffll;
    // a grid of at most half the CUs (batch-1 feature maps: the layer's time is ONE tile's walk through K): the 4 x 32 x 64
    // register-staged tiles give twice the workgroups (measured at 32 x 32 x 576 -> 512, batch 1: 0.067 vs 0.076 ms)
    const long long blocks64 = (long long)((W + 31) / 32) * ((H + 7) / 8) * B * ((Cout + 63) / 64);
    if (dma_ok && !pool && cout_pad % 128 == 0 && blocks64 <= 128) return "reg,64";
    if (dma_ok) return (cout_pad % 128 != 0 || big_blocks < 256) ? "dma,64" : "dma,128";
    if (cout_pad % 128 != 0) return nullptr;
    return (big_blocks < 256 && !pool) ? "reg,64" : "reg,128";
}

hipError_t launch_conv3x3_split16(const void *x, const void *w, const float *bias, void *out, int B, int H, int W,
                                  int Cin, int Cout, int cout_pad, float out_scale, int act, bool out_f32, bool f16,
                                  bool pool, hipStream_t s, bool ktree)
{
    if (Cin % 32 != 0 || Cout % 16 != 0 || cout_pad % 64 != 0 || act == ACT_SIGMOID) return hipErrorInvalidValue;
    if (ktree && (pool || !conv3x3_split16_ktree_ok(B, H, W, Cin, Cout, cout_pad))) return hipErrorInvalidValue;
    SplitConvArgs a{};
    a.status = range_status();
    a.x = (const uint4 *)x; a.w = (const uint4 *)w; a.bias = bias; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.cout_pad = cout_pad;
    a.out_scale = out_scale; a.act = act; a.out_f32 = out_f32 ? 1 : 0;
    const char *variant = conv3x3_split16_launch_variant(B, H, W, Cin, Cout, cout_pad, pool, ktree);
    if (!variant) return hipErrorInvalidValue;
    a.ktree = ktree ? 1 : 0;
    const long long big_blocks = (long long)((W + 31) / 32) * ((H + 7) / 8) * B * ((Cout + 127) / 128);
    if (variant[0] == 'd') {
        // Persistent LDS-DMA kernel: 8 x 32 px tiles, 128 channels wide -- or 64 wide where that is all there is
        // (Cout <= 64) or where 128-wide tiles would leave CUs without a tile (the 31 x 31 layers).  One workgroup per
        // CU (8 per XCD label at least), each walks the slots of its XCD label.
        const int BN = variant[4] == '6' ? 64 : 128;
        const SplitGrid g = split_grid(B, H, W, Cout, 8, BN);
        if (!g.valid || g.slots > 0x0fffffffll) return hipErrorInvalidValue;
        static const int n_cus = [] {
            int dev = 0, n = 0;
            if (hipGetDevice(&dev) != hipSuccess ||
                hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8)
                n = 256;
            return n;
        }();
        const dim3 pgrid(8u * (unsigned)(g.slots < n_cus / 8 ? g.slots : n_cus / 8));
        a.sched = sched_counters(s);
        with_bool(f16, [&](auto F16) {
            if (ktree)                      // the whole K tree inside the tile loop (SplitConvArgs::ktree)
                hipLaunchKernelGGL((conv3x3_split16_dma_kernel<F16(), false, 64, true>), pgrid, dim3(512), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
            else with_bool(pool, [&](auto POOL) {
                if (BN == 128) hipLaunchKernelGGL((conv3x3_split16_dma_kernel<F16(), POOL(), 128>), pgrid, dim3(512), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
                else hipLaunchKernelGGL((conv3x3_split16_dma_kernel<F16(), POOL(), 64>), pgrid, dim3(512), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
            });
        });
        return hipGetLastError();
    }
    // Register-staged kernels (an odd number of 32-channel slices, or RPN_S16_DMA=0).  Large grids: 8 x 32 px x 128 ch
    // tiles, one 8-wave workgroup per CU; small feature maps (no pooling there): 4 x 32 px x 64 ch tiles, 4 waves, two
    // workgroups per CU.
    const bool small = big_blocks < 256 && !pool;
    const SplitGrid g = split_grid(B, H, W, Cout, small ? 4 : 8, small ? 64 : 128);
    const long long nblocks = 8 * g.slots;
    if (!g.valid || nblocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblocks);
    with_bool(f16, [&](auto F16) {
        if (small) hipLaunchKernelGGL((conv3x3_split16_kernel<4, 1, 4, F16(), false>), grid, dim3(256), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
        else with_bool(pool, [&](auto POOL) {
            hipLaunchKernelGGL((conv3x3_split16_kernel<8, 2, 8, F16(), POOL()>), grid, dim3(512), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
        });
    });
    return hipGetLastError();
}

// Split-K factor for a 3x3 layer whose only consumer can add partial-sum slabs (rpn_conv -> the RPN head): grids of at
// most a quarter / half of the CUs (batch-1 feature maps) are cut 4 / 2 ways along K so that the layer's time is no longer
// one workgroup's walk through all of K.  1: no split.
// Whether a 3x3 layer feeding the slab-adding head runs as a K TREE (SplitConvArgs::ktree) -- at EVERY batch size up to
// B, so that the split factor may follow the grid size without changing bits: needs the persistent 64-wide kernel for the
// unsplit case (and its 2 GiB / even-slice limits) and at least one slice pair per leaf.  RPN_KSPLIT=0: one accumulation
// chain at every batch size (the layer's time at batch 1 is then one workgroup's walk through all of K).
bool conv3x3_split16_ktree_ok(int B, int H, int W, int Cin, int Cout, int cout_pad)
{
    static const int on = RPN_KNOB("RPN_KSPLIT", 1);
    return on && Cin % 64 == 0 && Cin >= 256 && Cout % 16 == 0 && cout_pad % 128 == 0 && cout_pad >= Cout &&
           (long long)B * H * W * Cin * 4 < 0x7fffffffll && (long long)(Cin / 32) * 9 * cout_pad * 128 < 0x7fffffffll;
}

bool conv3x3_split16_ksplit_dma(int B, int H, int W, int Cin, int Cout, int cout_pad)
{
    static const int on = RPN_LAB_KNOB("RPN_KSPLIT_DMA", 1);
    const char *v = conv3x3_split16_variant(B, H, W, Cin, Cout, cout_pad, false);
    if (!on || !v || strcmp(v, "reg,64") != 0) return false;           // (the small-grid case of a DMA-capable layer)
    const long long blocks64 = (long long)((W + 31) / 32) * ((H + 7) / 8) * B * ((Cout + 63) / 64);
    const int chunks = Cin / 32, mid = ktree_cut(chunks, 2);
    // the launcher's one-round grid: 2 x 8 x slots workgroups with slots <= 16 (launch_conv3x3_split16_ksplit's split_grid, so
    // the predicate never says yes to a grid the launcher refuses)
    const long long slots = split_grid(B, H, W, Cout, 8, 64).slots;
    return blocks64 > 64 && blocks64 <= 128 && slots <= 16 && mid >= 2 && (chunks - mid) >= 2 && (chunks - mid) % 2 == 0;
}

int conv3x3_split16_ksplit(int B, int H, int W, int Cin, int Cout, int cout_pad)
{
    if (conv3x3_split16_ksplit_dma(B, H, W, Cin, Cout, cout_pad)) return 2;
    // (a K-tree layer only -- the caller checks conv3x3_split16_ktree_ok at its largest batch)  MobileNetV2 500 x 500, one
    // image: 0.292 -> 0.259 ms per step; 1024 x 1024: 0.395 -> 0.377.
    const char *v = conv3x3_split16_variant(B, H, W, Cin, Cout, cout_pad, false);
    if (!v || strcmp(v, "reg,64") != 0) return 1;
    const long long blocks = (long long)((W + 31) / 32) * ((H + 3) / 4) * B * ((Cout + 63) / 64);
    return blocks <= 128 ? 4 : (blocks <= 256 ? 2 : 1);           // (2 workgroups of this kernel fit a CU: 512 slots)
}

// The split-K form of launch_conv3x3_split16 (4 x 32 x 64 register-staged tiles): out = ksplit float32 NHWC slabs of
// (B,H,W,Cout), slab_floats apart, holding RAW partial sums (no bias, no activation).
hipError_t launch_conv3x3_split16_ksplit(const void *x, const void *w, float *out, long long slab_floats, int B, int H, int W,
                                         int Cin, int Cout, int cout_pad, float out_scale, bool f16, int ksplit, hipStream_t s)
{
    if ((ksplit != 2 && ksplit != 4) || !conv3x3_split16_ktree_ok(B, H, W, Cin, Cout, cout_pad)) return hipErrorInvalidValue;
    SplitConvArgs a{};
    a.status = nullptr;
    a.ktree = 1;
    a.x = (const uint4 *)x; a.w = (const uint4 *)w; a.bias = nullptr; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.cout_pad = cout_pad;
    a.out_scale = out_scale; a.act = ACT_LINEAR; a.out_f32 = 1; a.slab_floats = slab_floats;
    if (ksplit == 2 && conv3x3_split16_ksplit_dma(B, H, W, Cin, Cout, cout_pad)) {
        // the persistent LDS-DMA kernel, two workgroups per 8 x 32 x 64 tile (static schedule: the two halves of a tile must not
        // share a tile queue); every workgroup has exactly one tile on these grids
        const SplitGrid g = split_grid(B, H, W, Cout, 8, 64);
        if (!g.valid || g.slots > 16) return hipErrorInvalidValue;        // 2 x 8 x slots workgroups: one tile each, one round
        const dim3 pgrid(8u * (unsigned)g.slots, 2);
        a.sched = nullptr;
        with_bool(f16, [&](auto F16) {
            hipLaunchKernelGGL((conv3x3_split16_dma_kernel<F16(), false, 64, true>), pgrid, dim3(512), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
        });
        return hipGetLastError();
    }
    const SplitGrid g = split_grid(B, H, W, Cout, 4, 64);
    const long long nblocks = 8 * g.slots;
    if (!g.valid || nblocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblocks, (unsigned)ksplit);
    with_bool(f16, [&](auto F16) {
        hipLaunchKernelGGL((conv3x3_split16_kernel<4, 1, 4, F16(), false>), grid, dim3(256), 0, s, a, g.tiles_x, g.tiles_y, g.n_tiles);
    });
    return hipGetLastError();
}

}  // namespace rpn
