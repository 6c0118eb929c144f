// Weight gradient of the trunk convolution (128 -> 128, 15x15) through the Winograd F(4x4,3x3) domain, the per-position
// products on the fp16 matrix pipe with two-term operands.  gfx950 only.
//
// The mathematics, the decomposition and the epilogue are wgrad_wino3.h's: dg = G^T [ sum over boards and tiles of
// dM (.) V ] G with V = B^T d B and dM = A dY A^T; one workgroup (512 threads, one per CU) owns 32 output x 32 input channels
// with all 36 positions; a half board is 64 planes x 8 tiles = ONE (plane, tile) PAIR PER THREAD, transformed in fp32
// registers from patch rows that come straight from global memory a half board ahead; two operand sets, one barrier per
// half board; 8 spx batch slices whose partial dg go to the scratch tensor that wgrad_wino_finish_kernel adds in slice
// order.  The summation order is fixed by (n, launch shape): the same bits on every run.
//
// What changes -- the product.  Every transformed value v is split into two fp16 terms, hi = fp16(v) and lo = fp16(v - hi)
// (v_cvt_pk_f16_f32 + v_fma_mixlo/hi_f16, both round to nearest even), and dU[pos][co][ci] += dM[pos][co][tile] V[pos][ci][tile]
// runs as v_mfma_f32_16x16x32_f16 with fp32 accumulation.
//
// k packing -- the choice.  The contraction index is the tile and a half board has 8 of them; k = 32 is four times that, so
// the four term products ride in k:   A = [Mh | Mh | Ml | Ml]  (m = co),   B = [Vh | Vl | Vh | Vl]  (n = ci)
// -- lane (q, j) of the MFMA holds k = 8 q .. 8 q + 7, i.e. the 8 tiles of term q >> 1 of dM and of term q & 1 of V for channel
// j.  ONE MFMA per (position, 16 co, 16 ci, half board) forms hi.hi + hi.lo + lo.hi (+ lo.lo, free): 18 MFMAs of 16 cycles per
// wave and half instead of 36 fp32 MFMAs of 32.  The other candidate (per board two MFMAs on word-packed {hi, lo} operands)
// contracts a whole board per MFMA pair: a second half board's operands resident, which the LDS does not hold.  The operand
// arrays are [position 36][term 2][channel 32][tile 8] fp16: a lane's fragment is the 16 contiguous bytes of one (position,
// term, channel), the 16 channels of a group are 256 contiguous bytes = one bank row, and the two terms lie 512 bytes apart:
// every 16-lane group of a ds_read_b128 (MI355X LDS: {0-3, 12-15, 20-27}, ...) takes 16 distinct 16-byte slots (B) or the same
// 256 bytes twice (A: q and q + 1 read one term, identical addresses broadcast): conflict-free without a swizzle, 27
// ds_read_b128 per wave and half (the fp32 kernel: 54 ds_read_b32 -- the same LDS cycles).  A hi / lo pair takes the 4 bytes
// of the fp32 value: 144 KiB for the two sets as before, and the epilogue's 148.5 KiB.
//
// What it costs, and why the trainer does not use it (profiles/r08_wgrad_f16x2.md).  The transform writes its two terms as
// 16-bit stores (ds_write_b16 / _d16_hi from the packed pairs of two positions; a wave's 64 lanes write 128 contiguous
// bytes): 72 stores per thread and half board instead of 36, and an LDS store costs its 4 cycles of address + data transfer
// whatever its width.  Measured: the MFMA phase falls to 0.4 - 0.5 of the exact kernel's, the transform grows by more than
// that, and the kernel takes 140 against 132 us at 512 boards and 39.2 against 36.5 us at 128.  The phases stay apart
// (transform, barrier, MFMAs) as in wgrad_wino3.h: issuing the MFMAs inside the next half board's transform was measured
// slower still (152 us) and is not kept.  The kernel is reachable through apz_wgrad_wino_f16x2 and
// hipconv.conv3x3_wgrad_f16x2 only.
//
// Range.  dM: A has a largest absolute row sum of 15, |dM| <= 225 max |dy|.  The gradients of a mean loss sit far below the
// fp16 normal range, so dy is multiplied by 2^a on the way in, a chosen on the device from `dymax` (`dymax_n` partial
// maxima of |dy|, what apz_bn_bwd_max leaves; every workgroup folds them: max is exact in any order, no atomics) such that
// max |dy| 2^a lies in [2^6, 2^7): 225 * 128 = 28 800 < 65 504 -- the dM side cannot overflow on finite input whose maxima
// are true -- and 21 binades below the maximum are still normal fp16.  a = 0 for an all-zero dy, -64 <= a <= 110; 2^-a is
// applied to the partial dg in the epilogue (exact: a power of two).  V: |V| <= 100 max |x|, not scaled, as in the forward.  The
// 32-bit word at `flag` is set (a plain vector store; never cleared here) when a partial dg is not finite -- an fp16 term that
// is +-inf makes every accumulator it feeds +-inf or NaN -- and also when an activation exceeds 65 504 / 100, where the
// bound above no longer keeps V inside fp16 (sufficient, not necessary: a single outlier only reaches 25 |x|).  The result
// of a launch that sets the word is unspecified.
// Lower end: a lo term below the fp16 normal range carries an ABSOLUTE error of up to 2^-25, so
// activations far below 2^-3 lose relative accuracy, exactly as in the f16x2 forward.  Not guarded.
#pragma once
#include <hip/hip_runtime.h>

#include "wgrad_wino3.h"
#include "wino_f16x2.h"

namespace apz {

struct WgradWino3H {
    static constexpr int C = 128, CO_B = 32, CI_B = 32, BLOCKS = (C / CO_B) * (C / CI_B);   // 16 channel blocks
    static constexpr int GPLANE = 240;
    static constexpr int TERM_BYTES = 32 * 16, POS_BYTES = 2 * TERM_BYTES;                  // [term][channel 32][tile 8] fp16
    static constexpr int OP_BYTES = 36 * POS_BYTES, SET_BYTES = 2 * OP_BYTES;               // V or dM of a half board; (V, dM)
    static constexpr int MAIN_BYTES = 2 * SET_BYTES;                                        // 147 456
    static constexpr int EPI_CS = WgradWino3::EPI_CS, EPI_PST = WgradWino3::EPI_PST;        // epilogue staging as wgrad_wino3.h
    static constexpr int EPI_BYTES = 36 * EPI_PST * 4;                                      // 152 064
    static constexpr int LDS_BYTES = EPI_BYTES > MAIN_BYTES + 32 ? EPI_BYTES : MAIN_BYTES + 32;
    static constexpr int THREADS = 512;
    static constexpr float X_LIMIT = 655.f;                                                 // 100 |x| stays below 65 504
};
static_assert(WgradWino3H::LDS_BYTES <= 160 * 1024, "LDS");

// a with m 2^a in [2^6, 2^7); 0 for m = 0; clamped to [-64, 110] (as wino3h16_dgrad_exponent: maxima down to 1e-31 reach
// the window; m = +inf sets the overflow word)
__device__ __forceinline__ int wgw3h_exponent(float m) {
    if (!(m > 0.f)) return 0;
    const int e = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 255u);   // m in [2^(e-127), 2^(e-126)) (e = 0: subnormal)
    const int a = 133 - e;
    return a < -64 ? -64 : (a > 110 ? 110 : a);
}

// the two terms of v0 (position p) and v1 (position p + 1) of this thread's (channel, tile): dst points at the hi term of
// position p
__device__ __forceinline__ void wgw3h_emit2(char* dst, float v0, float v1) {
    // (as asm: left to the compiler, the conversions of values that come out of an FMA are folded into v_fma_mix pairs -- three
    // instructions and a move instead of one)
    unsigned hu;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hu) : "v"(v0), "v"(v1));
    const unsigned lu = f16x2_split_lo(hu, v0, v1);
    using T = WgradWino3H;
    *reinterpret_cast<unsigned short*>(dst) = (unsigned short)hu;
    *reinterpret_cast<unsigned short*>(dst + T::POS_BYTES) = (unsigned short)(hu >> 16);
    *reinterpret_cast<unsigned short*>(dst + T::TERM_BYTES) = (unsigned short)lu;
    *reinterpret_cast<unsigned short*>(dst + T::POS_BYTES + T::TERM_BYTES) = (unsigned short)(lu >> 16);
}

#ifdef APZ_WGW3_STAMPS
// measurement builds: cycles per wave of workgroup 0 in (0) loop overhead, (2) transform, (3) barrier, (4) MFMA phase,
// (5) epilogue (slot 1 is unused, as in wgrad_wino3.h)
__device__ unsigned long long apz_wgw3h_stamps[8][6];
#endif

// x, dy: padded-row layout [n][128][15][16].  scratch, grid, slices and BUF: as wgrad_wino3_kernel.  dymax: dymax_n >= 1
// partial maxima of |dy|.  flag: the overflow word (may be null).
template <bool BUF = false>
__global__ __launch_bounds__(512) void wgrad_wino3h_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           float* __restrict__ scratch, int n, int spx,
                                                           const float* __restrict__ dymax, int dymax_n,
                                                           unsigned* __restrict__ flag) {
    using T = WgradWino3H;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* ldsb = reinterpret_cast<char*>(lds);        // two operand sets: V [36][2 terms][32 ch][8 tiles], dM likewise

    const int wg_k = blockIdx.x >> 3;
    const int blk = wg_k % T::BLOCKS, cob = blk >> 2, cib = blk & 3;
    const int slice = (blockIdx.x & 7) * spx + wg_k / T::BLOCKS, slices = 8 * spx;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, j = lane & 15;

    // ---- the scale of dy: 2^a from the partial maxima (the eight wave maxima meet behind the operand sets)
    float sc, isc;
    bool max_inf;                                     // a partial maximum is +inf: no scale fits, the result is void
    {
        float m = 0.f;
        for (int i = tid; i < dymax_n; i += T::THREADS) m = fmaxf(m, fabsf(dymax[i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float* wm = lds + T::MAIN_BYTES / 4;
        if (lane == 0) wm[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 8; w++) m = fmaxf(m, wm[w]);
        __syncthreads();                              // (the epilogue's staging area covers wm)
        const int a = __builtin_amdgcn_readfirstlane(wgw3h_exponent(m));
        max_inf = !(m <= 3.4028234664e38f);
        f16x2_pow2_pair(a, sc, isc);
    }

    // ---- MFMA roles: wave = (position group pg: positions 9 pg .. 9 pg + 8) x (output-channel group cc)
    const int pg = wave & 3, cc = wave >> 2;
    f32x4 acc[9][2];
#pragma unroll
    for (int p = 0; p < 9; p++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[p][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment addresses within an operand array, position 9 pg: A = dM term q >> 1 of output channel 16 cc + j, B = V term
    // q & 1 of input channels j and 16 + j
    const int a_off = pg * 9 * T::POS_BYTES + (q >> 1) * T::TERM_BYTES + (cc * 16 + j) * 16;
    const int b_off = pg * 9 * T::POS_BYTES + (q & 1) * T::TERM_BYTES + j * 16;

    // ---- transform roles (as wgrad_wino3_kernel): wave w < 4: input planes 8 w .. 8 w + 7 of the block's 32; wave w >= 4:
    // gradient planes 8 (w - 4) .. + 7.  Lane = (plane pl, tile row tr of the half, tile column ttx): a tile row is a quad.
    const bool grad = wave >= 4;
    const int ttx = lane & 3, tr = (lane >> 2) & 1, pl = lane >> 3;
    const int ch = (wave & 3) * 8 + pl;                             // channel of the block's 32
    const int tile = tr * 4 + ttx;                                  // tile of the half = k within a term
    const int w_off = ch * 16 + tile * 2;                           // bytes within a (position, term)
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(grad ? dy : x), 0, (unsigned)n * T::C * T::GPLANE * 4u, 0x00020000);
    const unsigned plane_off = (unsigned)(((grad ? cob * T::CO_B : cib * T::CI_B) + ch) * T::GPLANE + 4 * ttx) * 4u;
    const float* plane0 = grad ? dy + ((size_t)cob * T::CO_B + ch) * T::GPLANE + 4 * ttx : x + ((size_t)cib * T::CI_B + ch) * T::GPLANE + 4 * ttx;

    const int nboards = slice < n ? (n - slice + slices - 1) / slices : 0;
    const int total = nboards * 2;                    // half boards of this workgroup's stream
    // rows off the board: a per-lane offset past any legal num_records (see wgrad_wino3.h; n <= 32768 boards)
    constexpr unsigned OOB = 0xF8000000u;
    f32x4 nx[6];
    auto prefetch = [&](int u) {
        const int uu = u < total ? u : total - 1;     // (past the end: a harmless repeat)
        const int b = slice + (uu >> 1) * slices, trow = 2 * (uu & 1) + tr;
        const float* pb = plane0 + (size_t)b * T::C * T::GPLANE;
        const unsigned soff = (unsigned)b * (unsigned)(T::C * T::GPLANE * 4);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (grad && i >= 4) break;
            const int R = grad ? 4 * trow + i : 4 * trow - 1 + i;
            const bool in = R >= 0 && R <= 14;
            if constexpr (BUF) {
                nx[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, in ? plane_off + (unsigned)R * 64u : OOB, soff, 0));
            } else {
                nx[i] = *reinterpret_cast<const f32x4*>(pb + (in ? R : 0) * 16);
                if (!in) nx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    float xmax = 0.f;                                 // largest |activation| among this thread's own tiles
#ifdef APZ_WGW3_STAMPS
    unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long st_t = __builtin_readcyclecounter();
#endif

    // ---- the MFMAs of one half board from operand set `ops`: step p = position 9 pg + p, operands one step ahead
    f16x8 fa, fb0, fb1;
    auto fetch = [&](const char* ops, int p, f16x8& a_, f16x8& b0_, f16x8& b1_) {
        a_ = *reinterpret_cast<const f16x8*>(ops + T::OP_BYTES + a_off + p * T::POS_BYTES);
        b0_ = *reinterpret_cast<const f16x8*>(ops + b_off + p * T::POS_BYTES);
        b1_ = *reinterpret_cast<const f16x8*>(ops + b_off + p * T::POS_BYTES + 256);
    };
    auto mma_step = [&](const char* ops, int p) {
        f16x8 na = fa, nb0 = fb0, nb1 = fb1;
        if (p + 1 < 9) fetch(ops, p + 1, na, nb0, nb1);
        acc[p][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb0, acc[p][0], 0, 0, 0);
        acc[p][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb1, acc[p][1], 0, 0, 0);
        fa = na;
        fb0 = nb0;
        fb1 = nb1;
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- the transform of half board v (rows in nx) into operand set `ops`
    auto transform = [&](int v, char* ops) {
        if (!grad) {
            // ---- V = B^T d B of (input channel ch, tile (trow, ttx)): the 6 x 6 patch, rows first
            float xr[6][6];
#pragma unroll
            for (int i = 0; i < 6; i++) {             // patch row i, columns -1 .. 4
                const f32x4 c03 = nx[i];
                xr[i][0] = wgw_quad_neighbour<false>(c03[3], ttx);
                xr[i][1] = c03[0];
                xr[i][2] = c03[1];
                xr[i][3] = c03[2];
                xr[i][4] = c03[3];
                xr[i][5] = wgw_quad_neighbour<true>(c03[0], ttx);
            }
#pragma unroll
            for (int i = 1; i < 5; i++)               // the tile's own rows (the halo rows are other tiles' own)
                xmax = fmaxf(fmaxf(xmax, fmaxf(fabsf(nx[i][0]), fabsf(nx[i][1]))), fmaxf(fabsf(nx[i][2]), fabsf(nx[i][3])));
            prefetch(v + 1);                          // in flight during the barrier and this half's MFMAs
            float y[6][6];                            // y = B^T d (rows 0 / 5, 1 / 2, 3 / 4 share their partial sums)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                y[0][k] = __builtin_fmaf(4.f, xr[0][k], __builtin_fmaf(-5.f, xr[2][k], xr[4][k]));
                y[5][k] = __builtin_fmaf(4.f, xr[1][k], __builtin_fmaf(-5.f, xr[3][k], xr[5][k]));
                const float a = __builtin_fmaf(-4.f, xr[2][k], xr[4][k]), b = __builtin_fmaf(-4.f, xr[1][k], xr[3][k]);
                y[1][k] = a + b;
                y[2][k] = a - b;
                const float cdiff = xr[4][k] - xr[2][k], d = xr[3][k] - xr[1][k];
                y[3][k] = __builtin_fmaf(2.f, d, cdiff);
                y[4][k] = __builtin_fmaf(-2.f, d, cdiff);
            }
            char* dst = ops + w_off;
#pragma unroll
            for (int ir = 0; ir < 6; ir++) {
                const float* vv = y[ir];
                const float a = __builtin_fmaf(-4.f, vv[2], vv[4]), b = __builtin_fmaf(-4.f, vv[1], vv[3]);
                const float cdiff = vv[4] - vv[2], d = vv[3] - vv[1];
                float o[6];
                o[0] = __builtin_fmaf(4.f, vv[0], __builtin_fmaf(-5.f, vv[2], vv[4]));
                o[1] = a + b;
                o[2] = a - b;
                o[3] = __builtin_fmaf(2.f, d, cdiff);
                o[4] = __builtin_fmaf(-2.f, d, cdiff);
                o[5] = __builtin_fmaf(4.f, vv[1], __builtin_fmaf(-5.f, vv[3], vv[5]));
#pragma unroll
                for (int k = 0; k < 6; k += 2) wgw3h_emit2(dst + (ir * 6 + k) * T::POS_BYTES, o[k], o[k + 1]);
            }
        } else {
            // ---- dM = A (2^a dY) A^T of (output channel ch, tile (trow, ttx)): 4 x 4 -> 6 x 6
            const f32x4 d0 = nx[0] * sc, d1 = nx[1] * sc, d2 = nx[2] * sc, d3 = nx[3] * sc;   // exact: a power of two
            prefetch(v + 1);
            f32x4 m[6];
            m[0] = d0;
            m[5] = d3;
            {
                const f32x4 s02 = d0 + d2, s13 = d1 + d3;
                m[1] = s02 + s13;
                m[2] = s02 - s13;
                const f32x4 sv = d0 + 4.f * d2, tv = 2.f * d1 + 8.f * d3;
                m[3] = sv + tv;
                m[4] = sv - tv;
            }
            char* dst = ops + T::OP_BYTES + w_off;
#pragma unroll
            for (int ir = 0; ir < 6; ir++) {
                const f32x4 w = m[ir];
                const float s02 = w[0] + w[2], s13 = w[1] + w[3];
                const float sv = __builtin_fmaf(4.f, w[2], w[0]), tv = __builtin_fmaf(8.f, w[3], 2.f * w[1]);
                float o[6];
                o[0] = w[0];
                o[1] = s02 + s13;
                o[2] = s02 - s13;
                o[3] = sv + tv;
                o[4] = sv - tv;
                o[5] = w[3];
#pragma unroll
                for (int k = 0; k < 6; k += 2) wgw3h_emit2(dst + (ir * 6 + k) * T::POS_BYTES, o[k], o[k + 1]);
            }
        }
    };
    if (total > 0) prefetch(0);
    for (int u = 0; u < total; u++) {
        char* ops = ldsb + (u & 1) * T::SET_BYTES;
        WGW3_STAMP(0)
        transform(u, ops);
#ifdef APZ_WGW3_STAMPS
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
        WGW3_STAMP(2)
        // the half's operand arrays are complete -- and everybody is past the previous half's MFMAs, whose operand set the
        // NEXT transform overwrites: one barrier per half board
        __syncthreads();
        WGW3_STAMP(3)
        fetch(ops, 0, fa, fb0, fb1);
#pragma unroll
        for (int p = 0; p < 9; p++) mma_step(ops, p);
        WGW3_STAMP(4)
    }
    __syncthreads();                                  // the last half's operand reads are done
    // ---- partial dg of this slice and channel block (as wgrad_wino3_kernel): accumulator (p, b), lane (q, j), register r
    // holds dU at pos = 9 pg + p, co = 32 cob + 16 cc + 4 q + r, ci = 32 cib + 16 b + j; times 2^-a on the way out
    constexpr int CS = T::EPI_CS, PST = T::EPI_PST;
    float* du = lds;
    float* outw = scratch + (size_t)slice * WgradWino::SCRATCH_FLOATS_PER_SLICE;
    const float G[6][3] = {{0.25f, 0.f, 0.f},           {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                           {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
#pragma unroll
    for (int p = 0; p < 9; p++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) du[(pg * 9 + p) * PST + (cc * 16 + 4 * q + r) * CS + b * 16 + j] = acc[p][b][r];
    __syncthreads();
    float chk = 0.f;                                  // NaN as soon as one output is +-inf or NaN
#pragma unroll
    for (int e0 = 0; e0 < 1024; e0 += T::THREADS) {
        const int e = e0 + tid, col = e >> 5, cil = e & 31;
        float u[36];
#pragma unroll
        for (int p = 0; p < 36; p++) u[p] = du[p * PST + col * CS + cil];
        float tt[3][6];                              // tt[x][k] = sum_i G[i][x] dU[i][k]
#pragma unroll
        for (int x3 = 0; x3 < 3; x3++)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                float v = 0.f;
#pragma unroll
                for (int i6 = 0; i6 < 6; i6++) v += G[i6][x3] * u[i6 * 6 + k];
                tt[x3][k] = v;
            }
        float* d = outw + ((size_t)(cob * T::CO_B + col) * T::C + cib * T::CI_B + cil) * 9;
#pragma unroll
        for (int x3 = 0; x3 < 3; x3++)
#pragma unroll
            for (int y3 = 0; y3 < 3; y3++) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 6; k++) v += tt[x3][k] * G[k][y3];
                v *= isc;
                d[x3 * 3 + y3] = v;
                chk = __builtin_fmaf(v, 0.f, chk);
            }
    }
    if ((chk != chk || xmax > T::X_LIMIT || max_inf) && flag) *reinterpret_cast<volatile unsigned*>(flag) = 1u;
#ifdef APZ_WGW3_STAMPS
    WGW3_STAMP(5)
    if (blockIdx.x == 0 && lane == 0)
        for (int k = 0; k < 6; k++) apz_wgw3h_stamps[wave][k] = st_acc[k];
#endif
}

}  // namespace apz
