// conv_split_kernels.hip -- 3x3 / stride-1 / 'same' convolution on the 16-bit matrix cores with
// float32-grade accuracy ("x3 split"), for gfx950 (MI355X).
//
// Why: the exact-f32 MFMA tops out at 157 TFLOP/s, i.e. ~1000 images/s for VGG16+RPN at 500x500
// (SURVEY.md H1); the 16-bit MFMA is 16x faster.  Every float32 operand x is carried as two
// 16-bit halves hi = rn16(x), lo = rn16(x - hi), and each product is formed as
//        a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi          (3 MFMAs, float32 accumulation)
// dropping only a_lo*b_lo.  With bfloat16 halves the product error is ~2^-16 relative, with
// float16 halves ~2^-21 (weights are pre-scaled by a power of two so their low halves stay
// normal); the error is measured against a CPU float64 reference in tests/, never assumed.
//
// Layouts ("SPLIT16"): activations [B][H][W][C/16][64 B], one 64-byte record per pixel and
// 16-channel slice = {hi[0:8], lo[0:8], hi[8:16], lo[8:16]} as four 16-byte pieces; weights
// [C/16][tap][cout_pad][64 B] with the same record per output channel.  A 16-byte piece is
// exactly one lane's A (or B) fragment of v_mfma_f32_32x32x16_{bf16,f16}.
//
// Kernel: implicit GEMM, M = TH x 32 output pixels of one image, N = 64 or 128 output
// channels, K walked as (16-channel slice) x (9 taps).  Per slice the (TH+2) x 34 input halo is
// staged in LDS ONCE and re-read by all 9 taps at shifted addresses (the im2col matrix never
// exists); per tap only the BN x 64 B weight tile is streamed.  Both are double-buffered through
// registers (global loads for step s+1 are issued before the MFMAs of step s), one barrier per
// tap.  LDS records are XOR-swizzled by (row >> 2) & 3 so that every ds_read_b128 fragment
// read is bank-conflict free.  Epilogue: bias + activation, then the tile is transposed
// through LDS so each lane stores whole 16-byte pieces (256 contiguous bytes per pixel).
//
// Roofline: MFMA-bound; 3 MFMAs per algorithmic product, so the algorithmic peak is
// (dense 16-bit MFMA peak, 2.5 PFLOP/s) / 3.
//
// Three kernel families share that design (DESIGN.md 4.1 has the measurements that chose between them):
//   conv3x3_split_kernel        32x32x16 MFMA, 16-channel slices, register-staged: THIS FILE  (Cin = 64 -> 64: block1_conv2,
//                               and vgg_block1, its B1 instantiation)
//   conv3x3_split16_kernel      16x16x32 MFMA, 32-channel slices, register-staged             (conv_split16_kernels.hip)
//   conv3x3_split16_dma_kernel  16x16x32 MFMA, LDS-DMA staging, persistent workgroups         (conv_split16_kernels.hip)
// The first-layer kernels are in conv_cin3_kernels.hip, the SPLIT16 format kernels and the weight packers in split_format.hip,
// and what all four files share (device helpers, SplitConvArgs, the host's tile grid) in split_conv.h.
#include "split_conv.h"

namespace rpn {

// TH: tile height (4 or 8 rows of 32 pixels); WN: waves along N (2 -> BN = 128, 1 -> BN = 64).
// One barrier interval ("step") = one 16-channel slice x one FILTER ROW (3 taps): 3 x MI x NI x 3 MFMAs per
// wave between barriers, and the LDS fragment reads of tap s+1 overlap the MFMAs of tap s.
// BBUF: weight-tile buffers in LDS (2 = double buffered, one barrier per step; 1 = single buffered with a
// second barrier, used where two buffers would not leave room for two workgroups per CU).
//
// B1 (VGG16 block 1 in ONE launch: block1_conv1 -> block1_conv2 -> block1_pool, models/rpn_vgg16.py:16): the input is
// the float32 image, and the halo tile of each 16-channel slice of block1_conv1's output is COMPUTED into LDS instead of
// being staged from HBM -- the 64-channel full-resolution tensor (512 MB at batch 8: written once, read 1.1 times) never
// exists.  Per tile the (TH+4) x 36 x 3 image patch is staged once; every wave builds the im2col operand (K = 27 -> 32)
// of its share of the 340 halo pixels once, as hi/lo fragments in registers (B operand of v_mfma_16x16x32, so that a
// lane's 4 results are 4 consecutive CHANNELS of one pixel = one 8-byte run of the pixel's LDS record), and per slice
// multiplies them with that slice's 16 x 32 weight fragment: 3 MFMAs + bias/ReLU/split + 2 ds_write_b64 per 16 pixels,
// two such blocks per barrier interval, written to the halo buffer the loop is not reading.  Halo pixels outside the
// image are zeros (block1_conv2 pads block1_conv1's OUTPUT).  +8 % MFMA work on block1_conv2 (halo recompute included).
template <int TH, int WN, int BBUF, int NW, bool F16, bool POOL, bool B1 = false>
__global__ void __launch_bounds__(64 * NW, NW / 2)
conv3x3_split_kernel(SplitConvArgs a, int tiles_x, int tiles_y, int n_tiles)
{
    constexpr int NT = 64 * NW;              // threads per workgroup (NW = 4 or 8 waves)
    constexpr int WM = NW / WN;              // waves along M
    constexpr int MI = TH / WM;              // 32-pixel rows per wave
    constexpr int NI = 2;                    // 32-channel blocks per wave
    constexpr int BN = WN * NI * 32;
    constexpr int HP = (TH + 2) * HW;        // halo pixels
    constexpr int A_PIECES = HP * 4;
    constexpr int A_ROUNDS = (A_PIECES + NT - 1) / NT;
    constexpr int A_RPS = (A_ROUNDS + 2) / 3;                         // halo rounds issued per step
    constexpr int B_PIECES = 3 * BN * 4;                              // one filter row of weight records
    constexpr int B_ROUNDS = B_PIECES / NT;
    static_assert(MI * WM == TH && B_PIECES % NT == 0, "tile shape");
    constexpr int STAGE_LD = 64 + kStagePad;                         // floats per staged row
    constexpr int ABUF = HP * 4 + 4;                                 // one halo buffer + a dummy slot for idle lanes
    constexpr int PW = TWS + 4;                                      // B1: image patch columns (halo of the halo)
    constexpr int PATCH_F = B1 ? (TH + 4) * PW * 3 : 0;              // B1: floats of the image patch
    static_assert(!B1 || (WN == 1 && POOL && BBUF == 2), "B1: the 64 -> 64 pooled instantiations only");
    constexpr int LDS_PIPE = 2 * ABUF + BBUF * B_PIECES;             // uint4 units
    constexpr int LDS_STAGE = (NW * 32 * STAGE_LD * 4 + 15) / 16;    // uint4 units (NW waves x 32 rows)
    constexpr int LDS_UINT4 = (LDS_PIPE > LDS_STAGE ? LDS_PIPE : LDS_STAGE) + (PATCH_F + 3) / 4;

    __shared__ uint4 lds[LDS_UINT4];
    // native vector type for everything staged: struct copies of HIP's uint4 lower to memcpy, which keeps the
    // staging registers in scratch memory across a barrier
    u32x4 *As = reinterpret_cast<u32x4 *>(lds);               // [2][ABUF]
    u32x4 *Bs = reinterpret_cast<u32x4 *>(lds) + 2 * ABUF;    // [BBUF][3][BN][4]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lm = lane & 31, kh = lane >> 5;

    // XCD-aware tile order (speed only): hardware deals workgroup ids round-robin over the 8 XCDs, so
    // blockIdx % 8 labels the XCD.  The 8 XCDs form an XN x XM grid; XCD (xn, xm) owns the N-tiles
    // nt = xn (mod XN) and the M-tiles mt = xm (mod XM), so the weight slice it streams (K x BN x |nt set|,
    // 1.2-2.4 MB for the 512-channel layers) stays resident in its private 4 MB L2 instead of all
    // 9.4 MB of weights passing through every L2.  Workgroups past the padded grid exit at once.
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

    const int chunks = a.Cin >> 4;
    const int steps = chunks * 3;
    const size_t in_pix_stride = (size_t)chunks * 4;                     // uint4 per input pixel
    const uint4 *__restrict__ xin = B1 ? nullptr : a.x + (size_t)img * a.H * a.W * in_pix_stride;

    // ---- global -> register staging: every per-thread address is loop-invariant ----------------------
    // Halo pieces go through a raw buffer descriptor over THIS image: an out-of-image piece gets an offset
    // beyond num_records and the hardware range check returns zeros (no branch, no exec masking); the
    // 16-channel slice is selected by the scalar offset.  Weight pieces are plain global loads at
    // (uniform tile base) + (loop-invariant per-thread offset); cout_pad is a multiple of BN, no bounds check.
    constexpr int A_SLOTS = 3 * A_RPS;                                 // halo rounds per slice (some may be empty)
    constexpr unsigned kOob = 0x80000000u;                            // > any per-image tensor size (< 2 GiB)
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(xin), (short)0, (int)((size_t)a.H * a.W * in_pix_stride * 16), 0x00020000);
    unsigned a_goff[A_SLOTS];          // byte offset of this thread's piece of slice 0 (or kOob)
    int a_loff[A_SLOTS];               // uint4 index inside one halo buffer (dummy slot HP*4 when unused)
#pragma unroll
    for (int R = 0; R < (B1 ? 0 : A_SLOTS); ++R) {
        const int e = R * NT + tid;
        const int pix = e >> 2, pc = e & 3;
        const int hy = pix / HW, hx = pix - hy * HW;
        const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
        const bool piece = e < A_PIECES;
        const bool inimg = piece && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        a_loff[R] = piece ? (pix * 4 + (pc ^ ((hx >> 2) & 3))) : HP * 4;
        a_goff[R] = inimg ? (unsigned)((((size_t)iy * a.W + ix) * in_pix_stride + pc) * 16) : kOob;
    }
    u32x4 b_reg[B_ROUNDS];
    u32x4 a_reg[A_RPS];
    // (written as macros, not lambdas: a by-reference capture keeps the staging arrays in scratch memory)
#define RPN_LOAD_B(STEP)                                                                               \
    {                                                                                                  \
        const u32x4 *src_ = reinterpret_cast<const u32x4 *>(a.w) + ((size_t)(STEP) * 3 * a.cout_pad + n0) * 4;   \
        _Pragma("unroll") for (int i_ = 0; i_ < B_ROUNDS; ++i_) {                                      \
            const int e_ = tid + i_ * NT;                                                              \
            const int t_ = e_ / (BN * 4), rem_ = e_ - t_ * (BN * 4);          /* powers of two */      \
            b_reg[i_] = src_[(size_t)t_ * a.cout_pad * 4 + rem_];                                      \
        }                                                                                              \
    }
#define RPN_STORE_B(BUF)                                                                               \
    {                                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < B_ROUNDS; ++i_) {                                      \
            const int e_ = tid + i_ * NT;                                                              \
            const int t_ = e_ / (BN * 4), rem_ = e_ - t_ * (BN * 4);                                   \
            const int n_ = rem_ >> 2, pc_ = rem_ & 3;                                                  \
            Bs[(((BUF) * 3 + t_) * BN + n_) * 4 + (pc_ ^ ((n_ >> 2) & 3))] = b_reg[i_];                \
        }                                                                                              \
    }
#define RPN_LOAD_A(CHUNK, R) \
    __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, a_goff[R], (CHUNK) * 64, 0))

    // ---- B1: first-layer state (all dead code otherwise) ------------------------------------------------------
    constexpr int NBLK = (HP + 15) / 16;                              // 16-pixel blocks of the halo tile
    constexpr int QB = B1 ? (NBLK + NW - 1) / NW : 1;                 // blocks per wave: block = wave + NW * q
    constexpr int QPS = (QB + 2) / 3;                                 // blocks computed per barrier interval
    float *patchf = reinterpret_cast<float *>(lds + (LDS_PIPE > LDS_STAGE ? LDS_PIPE : LDS_STAGE));
    const int lr = lane & 15, kg = lane >> 4;
    u32x4 phi[QB], plo[QB];            // im2col fragments (8 of the 32 k of pixel lr): hi / lo halves
    int pdst[QB];                      // byte offset of this lane's 8-byte run inside a halo buffer (no pixel: the dummy slot)
    float b1_max = 0.0f;               // largest first-layer activation this lane produced (float16 range check)
    unsigned pin = 0;                  // bit q: the pixel is inside the image
    u32x4 w1hi = {0, 0, 0, 0}, w1lo = {0, 0, 0, 0};
    f32x4 b1v = {0.f, 0.f, 0.f, 0.f};
    (void)patchf; (void)lr; (void)kg; (void)pin; (void)phi; (void)plo; (void)pdst; (void)w1hi; (void)w1lo; (void)b1v;
    (void)b1_max;
#define RPN_B1_LOADW(CHUNK)                                                                            \
    {                                                                                                  \
        const u32x4 *w1_ = reinterpret_cast<const u32x4 *>(a.w1) + ((CHUNK) * 16 + lr) * 8 + kg;       \
        w1hi = w1_[0];                                                                                 \
        w1lo = w1_[4];                                                                                 \
        b1v = *reinterpret_cast<const f32x4 *>(a.b1 + (CHUNK) * 16 + 4 * kg);                          \
    }
    // block Q of the slice whose weights are in w1hi / w1lo -> halo buffer BUF.  Branch-free, so that the scheduler may
    // place this work among the tap MFMAs of the interval: lanes without a pixel (the tail of the last block, the
    // blocks past it) store to the buffer's dummy slot, and the float16 range check is one max per block, tested once
    // at the end of the kernel.
#define RPN_B1_BLOCK(Q, BUF)                                                                           \
    {                                                                                                  \
        f32x4 c_ = {0.f, 0.f, 0.f, 0.f};                                                               \
        c_ = mfma16<F16>(w1lo, phi[Q], c_);                                                            \
        c_ = mfma16<F16>(w1hi, plo[Q], c_);                                                            \
        c_ = mfma16<F16>(w1hi, phi[Q], c_);                                                            \
        using E_ = typename Half<F16>::elem;                                                           \
        using h4_ = __attribute__((ext_vector_type(4))) E_;                                            \
        const bool in_ = (pin >> (Q)) & 1u;                                                            \
        h4_ hv_, lv_;                                                                                  \
        _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                             \
            float v_ = fmaxf(c_[r_] * a.scale1 + b1v[r_], 0.0f);                                       \
            v_ = in_ ? v_ : 0.0f;                                                                      \
            b1_max = fmaxf(b1_max, v_);                                                                \
            const E_ h_ = (E_)v_;                                                                      \
            hv_[r_] = h_;                                                                              \
            lv_[r_] = (E_)(v_ - (float)h_);                                                            \
        }                                                                                              \
        char *d_ = reinterpret_cast<char *>(As + (BUF) * ABUF);                                        \
        *reinterpret_cast<uint2 *>(d_ + pdst[Q]) = __builtin_bit_cast(uint2, hv_);                     \
        *reinterpret_cast<uint2 *>(d_ + (pdst[Q] ^ 16)) = __builtin_bit_cast(uint2, lv_);              \
    }
    if constexpr (B1) {
        // image patch: rows oy0 - 2 .. oy0 + TH + 1, columns ox0 - 2 .. ox0 + 33, zero outside the image
        const float *ximg = a.img + (size_t)img * a.H * a.W * 3;
        for (int e = tid; e < PATCH_F; e += NT) {
            const int pr = e / (PW * 3), rem = e - pr * (PW * 3);
            const int iy = oy0 - 2 + pr, ix = ox0 - 2 + rem / 3;
            patchf[e] = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? ximg[((size_t)iy * a.W + ix) * 3 + rem % 3] : 0.0f;
        }
    }

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // fragment addresses: A depends on the lane and the tap column s only (column swizzle), B on the lane only
    int a_off[3];
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) a_off[s3] = (lm + s3) * 4 + ((2 * kh) ^ (((lm + s3) >> 2) & 3));
    int b_off[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = wn * (NI * 32) + j * 32 + lm;
        b_off[j] = n * 4 + ((2 * kh) ^ ((n >> 2) & 3));
    }

    // ---- prologue: halo of slice 0, weights of step 0 -------------------------------------------
    if constexpr (B1) {
        RPN_LOAD_B(0);
        RPN_B1_LOADW(0);
        RPN_STORE_B(0);
        __syncthreads();                                   // the patch is complete
        // k = 8 kg + j = (r * 3 + s) * 3 + c  ->  offset inside the patch relative to the pixel's top-left input
        int koff[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * kg + j;
            koff[j] = k < 27 ? (k / 9) * (PW * 3) + (k % 9) : -1;
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int p = (wave + NW * q) * 16 + lr;
            const bool valid = p < HP;
            const int pp = valid ? p : HP - 1;
            const int hy = pp / HW, hx = pp - hy * HW;
            const int base = (hy * PW + hx) * 3;
            float xs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) xs[j] = koff[j] >= 0 ? patchf[base + koff[j]] : 0.0f;
            phi[q] = __builtin_bit_cast(u32x4, split_piece<F16>(xs, false));
            plo[q] = __builtin_bit_cast(u32x4, split_piece<F16>(xs, true));
            const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) pin |= 1u << q;
            // channels 4 kg .. 4 kg + 3 of the slice: hi piece 2 * (kg >> 1), its half (kg & 1); lo piece = hi piece ^ 1
            pdst[q] = valid ? (pp * 4 + ((2 * (kg >> 1)) ^ ((hx >> 2) & 3))) * 16 + (kg & 1) * 8 : HP * 4 * 16 + (kg & 1) * 8;
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) RPN_B1_BLOCK(q, 0);
    } else {
#pragma unroll
        for (int R = 0; R < A_SLOTS; ++R) As[a_loff[R]] = RPN_LOAD_A(0, R);
        RPN_LOAD_B(0);
        RPN_STORE_B(0);
    }
    __syncthreads();

    int abuf = 0, bbuf = 0;
#pragma unroll 1
    for (int chunk = 0; chunk < chunks; ++chunk) {
        // the prefetch past the last slice / step is clamped to the last one: its data lands in the idle
        // buffers and is never read, which keeps the loop free of branches
        const int next_chunk = chunk + 1 < chunks ? chunk + 1 : chunk;
#pragma unroll
        for (int row = 0; row < 3; ++row) {              // unrolled: halo slot indices are compile-time
            const int step = chunk * 3 + row;
            RPN_LOAD_B(step + 1 < steps ? step + 1 : step);
            if constexpr (B1) {
                if (row == 0) RPN_B1_LOADW(next_chunk);      // first-layer weights of the slice computed below
            } else {
#pragma unroll
                for (int q = 0; q < A_RPS; ++q) a_reg[q] = RPN_LOAD_A(next_chunk, row * A_RPS + q);
            }
            if constexpr (NW == 4) RPN_PIN_LOADS();          // (the 8-wave variant has 128 VGPRs: pinned, it spills)

            const u32x4 *arow = As + (abuf * ABUF + (wm * MI + row) * HW * 4);
#pragma unroll
            for (int s = 0; s < 3; ++s) {                    // the 3 taps of filter row `row`
                u32x4 ahi[MI], alo[MI], bhi[NI], blo[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) {               // a_off[s] is lane-constant; i * HW * 4 is an immediate
                    ahi[i] = arow[i * HW * 4 + a_off[s]];
                    alo[i] = arow[i * HW * 4 + (a_off[s] ^ 1)];
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    bhi[j] = Bs[(bbuf * 3 + s) * BN * 4 + b_off[j]];
                    blo[j] = Bs[(bbuf * 3 + s) * BN * 4 + (b_off[j] ^ 1)];
                }
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        acc[i][j] = Half<F16>::mfma(alo[i], bhi[j], acc[i][j]);
                        acc[i][j] = Half<F16>::mfma(ahi[i], blo[j], acc[i][j]);
                        acc[i][j] = Half<F16>::mfma(ahi[i], bhi[j], acc[i][j]);
                    }
            }

            if (BBUF == 1) __syncthreads();              // every wave is done reading the single weight buffer
            RPN_STORE_B(BBUF == 2 ? (bbuf ^ 1) : 0);
            if constexpr (B1) {
                // the next slice's halo tile: QPS blocks per interval (in the last slice: that slice's own tile once more,
                // into the idle buffer -- cheaper than a branch that would fence this work off from the MFMAs)
#pragma unroll
                for (int q = row * QPS; q < (row + 1) * QPS && q < QB; ++q) RPN_B1_BLOCK(q, abuf ^ 1);
            } else {
#pragma unroll
                for (int q = 0; q < A_RPS; ++q) As[(abuf ^ 1) * ABUF + a_loff[row * A_RPS + q]] = a_reg[q];
            }
            __syncthreads();
            if (BBUF == 2) bbuf ^= 1;
        }
        abuf ^= 1;
    }

#undef RPN_LOAD_B
#undef RPN_STORE_B
#undef RPN_LOAD_A
#undef RPN_B1_LOADW
#undef RPN_B1_BLOCK
    if constexpr (B1 && F16) {
        if (a.status && !(b1_max <= 65504.0f)) atomicOr(a.status, 1u /* RPN_STATUS_F16_RANGE */);
    }
    // ---- epilogue: scale + bias + activation (+ fused 2x2 max-pool), transpose through LDS, 16-byte stores --
    float *stage = reinterpret_cast<float *>(lds) + wave * (32 * STAGE_LD);
    float bias_v[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int n = n0 + wn * (NI * 32) + j * 32 + lm;
        bias_v[j] = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;
    }
    // activation as a branch-free clamp: linear / relu / relu6 (the launcher rejects sigmoid)
    const float act_lo = a.act == ACT_LINEAR ? -INFINITY : 0.0f;
    const float act_hi = a.act == ACT_RELU6 ? 6.0f : INFINITY;
    const int cout_chunks = a.Cout >> 4;
    const int nbase = n0 + wn * (NI * 32);                             // first channel of this wave's 64
    // write NPX staged pixels x 64 channels of output row `oy` (output image OHo x OWo, first column oxb): one buffer per row
    // segment [oxb, OWo), a lane owns eight channels of a pixel and writes their hi and lo pieces (split16_epilogue has the why)
    const int pix_bytes = a.out_f32 ? a.Cout * 4 : cout_chunks * 64;
    auto store_stage = [&](int npx_log2, int oy, int oxb, int OHo, int OWo) {
        if (oy >= OHo) return;
        const long long row_off = (((long long)img * OHo + oy) * OWo + oxb) * (long long)pix_bytes;
        const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char *>(a.out) + row_off, (short)0,
                                                                              (OWo - oxb) * pix_bytes, 0x00020000);
        if (a.out_f32) {
            const int rounds = (16 << npx_log2) >> 6;                  // (npx * 16 float4s) / 64 lanes
            const int px_l = lane >> 4, q_l = lane & 15;
            const int n = nbase + 4 * q_l;
            unsigned voff = n < a.Cout ? (unsigned)(px_l * pix_bytes + n * 4) : 0x80000000u;
#pragma unroll
            for (int rd = 0; rd < rounds; ++rd) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(&stage[(rd * 4 + px_l) * STAGE_LD + 4 * q_l]);
                __builtin_amdgcn_raw_buffer_store_b128(v, ors, voff, 0, 0);
                voff += (unsigned)(4 * pix_bytes);
            }
        } else {
            const int rounds2 = (8 << npx_log2) >> 6;                  // (npx * 8 lanes) / 64
            const int px2 = lane >> 3, q2 = lane & 7;
            const int cl = q2 >> 1, hf = q2 & 1;
            const int n = nbase + cl * 16;
            unsigned voff = n < a.Cout ? (unsigned)(px2 * pix_bytes + (n >> 4) * 64 + hf * 32) : 0x80000000u;
#pragma unroll
            for (int rd = 0; rd < rounds2; ++rd) {
                float xs[8];
                const float *src = &stage[(rd * 8 + px2) * STAGE_LD + cl * 16 + hf * 8];
                const float4 v0 = *reinterpret_cast<const float4 *>(src);
                const float4 v1 = *reinterpret_cast<const float4 *>(src + 4);
                xs[0] = v0.x; xs[1] = v0.y; xs[2] = v0.z; xs[3] = v0.w;
                xs[4] = v1.x; xs[5] = v1.y; xs[6] = v1.z; xs[7] = v1.w;
                const u32x4 hi = __builtin_bit_cast(u32x4, split_piece<F16>(xs, false, a.status));
                const u32x4 lo = __builtin_bit_cast(u32x4, split_piece<F16>(xs, true, nullptr));
                __builtin_amdgcn_raw_buffer_store_b128(hi, ors, voff, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(lo, ors, voff + 16u, 0, 0);
                voff += (unsigned)(8 * pix_bytes);
            }
        }
    };

    if constexpr (POOL) {
        // MaxPooling2D(2,2) 'valid' fused: the 2x2 window of output pixel (y,x) is rows (2y, 2y+1) -- two
        // M-blocks of this wave -- and accumulator registers (2e', 2e'+1) of one lane, so the max is lane-local.
        // max commutes with the monotone bias + activation, which are applied once afterwards.
        static_assert(!POOL || (MI % 2 == 0), "pooling needs an even number of rows per wave");
        const int OHo = a.H >> 1, OWo = a.W >> 1;
#pragma unroll
        for (int ip = 0; ip < MI / 2; ++ip) {
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int e2 = 0; e2 < 8; ++e2) {
                    const float v0 = fmaxf(acc[2 * ip][j][2 * e2], acc[2 * ip][j][2 * e2 + 1]);
                    const float v1 = fmaxf(acc[2 * ip + 1][j][2 * e2], acc[2 * ip + 1][j][2 * e2 + 1]);
                    const int m2 = (e2 & 1) + 4 * (e2 >> 1) + 2 * kh;             // pooled column 0..15
                    stage[m2 * STAGE_LD + j * 32 + lm] = fminf(fmaxf(fmaxf(v0, v1) * a.out_scale + bias_v[j], act_lo), act_hi);
                }
            wave_sync();
            store_stage(4, (oy0 + wm * MI + 2 * ip) >> 1, ox0 >> 1, OHo, OWo);
            wave_sync();
        }
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i) {             // fully unrolled: acc[] must be indexed statically
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = (e & 3) + 8 * (e >> 2) + 4 * kh;
                    stage[m * STAGE_LD + j * 32 + lm] = fminf(fmaxf(acc[i][j][e] * a.out_scale + bias_v[j], act_lo), act_hi);
                }
            wave_sync();
            store_stage(5, oy0 + wm * MI + i, ox0, a.H, a.W);
            wave_sync();
        }
    }
}

template <int TH, int WN, int BBUF, bool F16, bool POOL, int NW = 4>
static hipError_t launch_split_variant(const SplitConvArgs &a, hipStream_t s)
{
    // grid padded to 8 x ceil(n_tiles / XN) x ceil(m_tiles / XM): see the XCD-aware tile order in the kernel
    const SplitGrid g = split_grid(a.B, a.H, a.W, a.Cout, TH, WN * 64);
    const long long nblocks = 8 * g.slots;
    if (!g.valid || nblocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL((conv3x3_split_kernel<TH, WN, BBUF, NW, F16, POOL>), dim3((unsigned)nblocks), dim3(64 * NW), 0,
                       s, a, g.tiles_x, g.tiles_y, g.n_tiles);
    return hipGetLastError();
}

// laboratory knobs (-DRPN_LAB builds only; speed only, never results): RPN_SPLIT_TILE = 82 | 81 | 42 | 41 forces a tile shape,
// RPN_SPLIT_BBUF = 1 | 2 the number of weight buffers.  The instantiations that only RPN_SPLIT_BBUF, RPN_SPLIT_WAVES and
// RPN_SPLIT_SMALL reach are compiled into the laboratory library alone.

// 10 * tile rows + 64-channel columns of the 32x32x16 kernel's tile for a layer: 81 | 82 | 42 | 41 (launch_split_tiles launches it;
// rpn_model_conv_launch_info reports its width)
int conv3x3_split_tile(int B, int H, int W, int Cout, bool pool)
{
    static const int force_tile = RPN_LAB_KNOB("RPN_SPLIT_TILE", 0);
    const long long mt8 = (long long)((W + 31) / 32) * ((H + 7) / 8) * B;
    const long long mt4 = (long long)((W + 31) / 32) * ((H + 3) / 4) * B;
    const int nt128 = (Cout + 127) / 128;
    int tile;
    if (Cout <= 64) tile = 81;
    else if (mt8 * nt128 >= 512) tile = 82;
    else if (mt4 * nt128 >= 512 || pool) tile = 42;
    else tile = 41;
    if (force_tile && Cout > 64 && !(pool && force_tile == 41)) tile = force_tile;
    return tile;
}

template <bool F16, bool POOL>
static hipError_t launch_split_tiles(const SplitConvArgs &a, hipStream_t s)
{
    // tile choice: 64-wide N tiles for Cout <= 64; shorter / narrower tiles when the grid would not put
    // two workgroups on each of the 256 CUs
    const int tile = conv3x3_split_tile(a.B, a.H, a.W, a.Cout, POOL);
    // default buffers: two wherever LDS still admits two workgroups per CU (<= 80 KB)
    int bbuf = (tile == 82) ? 1 : 2;
#ifdef RPN_LAB
    static const int force_bbuf = RPN_LAB_KNOB("RPN_SPLIT_BBUF", 0);
    if (force_bbuf) bbuf = force_bbuf;
    if (tile == 82 && bbuf == 2) bbuf = 1;                   // 92 KB: one workgroup per CU, not offered
    static const int force_waves = RPN_LAB_KNOB("RPN_SPLIT_WAVES", 0);        // 8: 512-thread workgroups on the 8x32 x 128 tile
    if (tile == 82 && force_waves == 8) return launch_split_variant<8, 2, 1, F16, POOL, 8>(a, s);
    // experiment (RPN_SPLIT_SMALL=2): 128 px x 128 ch tiles shared by 8 waves for small feature maps.  Measured on
    // 31x31x512, batch 8: 0.137 ms vs 0.126 ms for the default 4-wave 128 x 64 tiles, so it stays off.
    static const int small_mode = RPN_LAB_KNOB("RPN_SPLIT_SMALL", 0);
    if constexpr (!POOL) {
        const long long mt4 = (long long)((a.W + 31) / 32) * ((a.H + 3) / 4) * a.B;
        const int nt128 = (a.Cout + 127) / 128;
        if (tile == 41 && small_mode == 2 && mt4 * nt128 >= 256) return launch_split_variant<4, 2, 2, F16, false, 8>(a, s);
    }
#endif
    switch (tile * 10 + bbuf) {
        case 821: return launch_split_variant<8, 2, 1, F16, POOL>(a, s);
        case 812: return launch_split_variant<8, 1, 2, F16, POOL>(a, s);
        case 422: return launch_split_variant<4, 2, 2, F16, POOL>(a, s);
        case 412: if constexpr (!POOL) return launch_split_variant<4, 1, 2, F16, false>(a, s); else break;
#ifdef RPN_LAB
        case 811: return launch_split_variant<8, 1, 1, F16, POOL>(a, s);
        case 421: return launch_split_variant<4, 2, 1, F16, POOL>(a, s);
        case 411: if constexpr (!POOL) return launch_split_variant<4, 1, 1, F16, false>(a, s); else break;
#endif
        default: break;
    }
    return hipErrorInvalidValue;
}

// 3x3 stride-1 'same' conv on SPLIT16 input (optionally followed by a fused 2x2 'valid' max-pool).
// x: SPLIT16 (B,H,W,Cin), w: split records, out: SPLIT16 or f32 NHWC of (B,H,W,Cout) or, pooled, (B,H/2,W/2,Cout).
hipError_t launch_conv3x3_split(const void *x, const void *w, const float *bias, void *out, int B, int H, int W,
                                int Cin, int Cout, int cout_pad, float out_scale, int act, bool out_f32, bool f16,
                                bool pool, hipStream_t s, bool ktree)
{
    if (ktree) return hipErrorInvalidValue;           // (the parameter only keeps the two launchers' signatures equal)
    if (Cin % 16 != 0 || Cout % 16 != 0 || cout_pad % 64 != 0 || act == ACT_SIGMOID) return hipErrorInvalidValue;
    SplitConvArgs a{};
    a.status = range_status();
    a.x = (const uint4 *)x; a.w = (const uint4 *)w; a.bias = bias; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.cout_pad = cout_pad;
    a.out_scale = out_scale; a.act = act; a.out_f32 = out_f32 ? 1 : 0;
    return with_bool(f16, [&](auto F16) {
        return with_bool(pool, [&](auto POOL) { return launch_split_tiles<F16(), POOL()>(a, s); });
    });
}

// VGG16 block 1 in one launch: block1_conv1 (3 -> 64) + ReLU -> block1_conv2 (64 -> 64) + ReLU -> 2x2 max-pool
// (models/rpn_vgg16.py:16, keras-applications VGG16).  img: float32 NHWC (B,H,W,3); w1: pack_weights_cin3_mfma_host
// records of block1_conv1; w2: pack_weights_split_host records of block1_conv2; out: SPLIT16 (B,H/2,W/2,64).
hipError_t launch_vgg_block1(const float *img, const void *w1, const float *b1, float scale1, const void *w2,
                             const float *b2, float scale2, void *out, int B, int H, int W, bool f16, hipStream_t s)
{
    if (B < 1 || H < 2 || W < 2) return hipErrorInvalidValue;
    SplitConvArgs a{};
    a.status = range_status();
    a.x = nullptr; a.w = (const uint4 *)w2; a.bias = b2; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = 64; a.Cout = 64; a.cout_pad = 64;
    a.out_scale = scale2; a.act = ACT_RELU; a.out_f32 = 0;
    a.img = img; a.w1 = (const uint4 *)w1; a.b1 = b1; a.scale1 = scale1;
    const SplitGrid g = split_grid(B, H, W, 64, 8, 64);             // n_tiles = 1: XN = 1, XM = 8 (the kernel's tile order)
    const long long nblocks = 8 * g.slots;
    if (nblocks > 0x7fffffffll) return hipErrorInvalidValue;
    with_bool(f16, [&](auto F16) {
        hipLaunchKernelGGL((conv3x3_split_kernel<8, 1, 2, 4, F16(), true, true>), dim3((unsigned)nblocks), dim3(256), 0, s, a,
                           g.tiles_x, g.tiles_y, g.n_tiles);
    });
    return hipGetLastError();
}

}  // namespace rpn
