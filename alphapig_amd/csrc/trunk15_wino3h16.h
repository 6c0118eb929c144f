// Trunk 3x3 convolution (128 -> 128 channels, 15x15 board) + folded BN + (residual) + ReLU: trunk15_wino3h.h's fused
// F(4x4,3x3) Winograd convolution on the fp16 matrix pipe with two-term operands, K loop repacked (round 7).  gfx950 only.
//
// What stays: the arithmetic (x = hi + lo, two fp16 terms, weights times S[co] = 2^k, 1 / S[co] in the bias FMA, activations
// unscaled, the overflow word), the work item (board pair x 64 output channels x 36 positions), the grid and duo scheme, eight
// waves = (32-channel half, 3x3 position block) with 144 accumulators each, and the epilogue (its arithmetic is the shared
// wino_out_row, wino_sum4 and wino_nonfinite of wino_common.h in both kernels).
//
// What changes -- the K packing.  trunk15_wino3h.h contracts k = 16 as 8 channels x the two WEIGHT terms (A = [Whi | Wlo],
// B = [Vt | Vt]): four products per 8 channels, lo.lo included, and both lane halves of a B fragment read the same 16 bytes.
// Here k = 16 is 16 channels of ONE term, and a chunk of 16 input channels takes three MFMAs per (position, 32 output channels):
//     H . Vlo  +  L . Vhi  +  H . Vhi        (H = [Whi ch 0-7 | Whi ch 8-15], L = the same of Wlo, V likewise)
// -- the three products the accuracy argument rests on (|error| <= 2^-22 relative per operand); lo.lo is dropped.  Per wave and
// 16 input channels: 27 MFMAs instead of 36, 18 V fragment reads instead of 36, one chunk barrier instead of two; the weight
// bytes are the same (two 1 KB units per position).
//
// LDS.  A 16-channel V buffer is 36 x 2 terms x 32 columns x 16 ch x 2 B = 72 KiB; two of them are 144 KiB of the 160, and the
// raw input tiles no longer fit beside them.  So they are not staged: every thread owns one (board, channel, tile) of a chunk
// -- 2 x 16 x 16 = 512 -- and buffer-loads the tile's 4 x 4 pixels into 16 registers a chunk ahead (the twin workgroup of the
// duo scheme reads the same planes: L2).  A board's 16 tiles are one 16-lane DPP row, so the halo rows -1 and 4 of the patch
// are row_shr:4 / row_shl:4 of the neighbouring tiles' rows 3 and 0 (zero across the board edge by bound_ctrl), and the halo
// columns come from the quad neighbours' column-pass inputs as in trunk15_wino3h.h.  Each thread transforms the whole 6 x 6
// patch of its channel (the old kernel: half of it, for 8 channels).
//
// Layouts.  in / resid / out: rows16 [n][128][15][16] (col 15 == 0).  V (LDS): [pos 36][term 2 (hi, lo)][col 32][half 2][8 ch]
// fp16, col = board * 16 + tile, and the channel half stored at half ^ (col >> 3 & 1): a B fragment (lane: col = lane & 31,
// channels 8 (lane >> 5) .. + 7) is ONE ds_read_b128 with no bank conflict (unswizzled, the 32-byte column stride puts two lanes
// of every b128 lane group on one bank quad), and the transform's ds_write_b32 of 32 lanes fall on 16 banks (2-way: free).
// upk: [cog 4][block 4][chunk 8][position 9][unit 2 (H, L)][half 2][co 32][8 ch] fp16.  bias: [128 bias][128 1/S].
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "wino_f16x2.h"

namespace apz {

struct Wino3H16 {
    static constexpr int C = 128, CK = 16, NCHUNK = C / CK;            // 8 chunks of 16 input channels
    static constexpr int GPLANE = 240;
    static constexpr int VTERM = 32 * 32, VPOS = 2 * VTERM, V_BYTES = 36 * VPOS;   // 1024, 2048, 73728 bytes
    static constexpr int UNIT = 2 * 32 * 16;                           // bytes of one weight unit (H or L of a position): 1024
    static constexpr size_t UPK_BYTES = (size_t)4 * 4 * NCHUNK * 9 * 2 * UNIT;     // 2.36 MB per layer (as Wino3H)
    static constexpr int BIAS_FLOATS = 256;                            // [bias 128][1 / S 128]
    // epilogue: M and the store staging alias the two V buffers
    static constexpr int MQ_FLOATS = 36 * 16 * 32;                     // 73728 bytes
    static constexpr int SROW = 20, SPLANE = 16 * SROW;                // staging plane: 16 rows x 20 floats
    static constexpr int STG_FLOATS = 8 * 4 * SPLANE;                  // 8 waves x 4 planes (40 KiB)
    static constexpr int LDS_BYTES = 2 * V_BYTES;                      // 147456
    static_assert((MQ_FLOATS + STG_FLOATS) * 4 <= LDS_BYTES, "the epilogue area fits over V");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    // byte offset of element (co, ci, pos, term) in the packed weights
    __host__ __device__ static size_t upk_offset(int co, int ci, int pos, int term) {
        const int i = pos / 6, k = pos % 6, ri = i / 3, ki = k / 3, p9 = 3 * (i % 3) + (k % 3);
        const int cog = co >> 5, r = co & 31, chunk = ci >> 4, half = (ci >> 3) & 1, w = 2 * ri + ki;
        return ((((size_t)(cog * 4 + w) * NCHUNK + chunk) * 9 + p9) * 2 + term) * UNIT + half * 512 + r * 16 + (ci & 7) * 2;
    }
};

#ifdef APZ_WINO3H_STAMPS
__device__ unsigned long long apz_wino3h16_stamps[4 * 8 * 12];   // [workgroup 4][wave 8][phase 12]
#endif

#ifndef APZH16_RING
#define APZH16_RING 3        /* positions (H + L: 8 registers each) of the weight ring; RING - 1 in flight.  Must divide 18 */
#endif
#ifndef APZH16_RAW_SLOT
#define APZH16_RAW_SLOT 4    /* the MFMA slot whose end requests the raw tiles of the chunk after next */
#endif

// FORM: WINO3H16_PLAIN is the self-play kernel (aux unused).  The training step's two forms, RELU false for both:
//   WINO3H16_STATS  the forward in front of a BatchNorm: bias only, no residual; `aux` receives per (output channel, board)
//                   the sum and the sum of squares of the board's 225 outputs as double [128][n][2], the contract of
//                   trunk15_wino3_kernel<..., STATS = true> (bn_fwd(stats=...) consumes either).  A board's 225 values: the
//                   lane's 4x4 tile row by row, its four rows, then the 16 tiles of the board (one DPP row) -- a fixed fp32
//                   tree whatever the launch shape or the board's place in the batch.
//   WINO3H16_DGRAD  the data gradient (flipped, transposed weights; bias zero; RESID adds the skip gradient).  Its input is
//                   not O(1): the gradients of a mean loss sit far below the fp16 normal range, where the lo term of the
//                   split is subnormal and carries an ABSOLUTE error of up to 2^-25.  So the launch
//                   scales its input by 2^a, chosen on the device: `aux` holds `aux_n` partial maxima of |input| (bn_bwd's
//                   dxmax, one per channel and batch split), every workgroup folds them (max: exact, any order), and a puts
//                   the maximum into [2^7, 2^8) -- |V| <= 100 max <= 25 600 stays below the fp16 limit, and 22 binades
//                   below the maximum are still normal fp16.  The raw tile values are multiplied by 2^a before the
//                   transform, 2^-a goes into the 1 / S of the bias FMA.  2^a and 2^-a are normal floats for
//                   -64 <= a <= 110; the product 2^-a / S = 2^-(a + k) (S = 2^k from f16x2_scale_for, k about 18 for
//                   weights of this net, clamped to 100) is an fp32 subnormal from a + k = 127 on, and exact there only
//                   because this library is built with fp32 denormals enabled (the compiler's default for gfx950;
//                   no flush-to-zero flag in build.py) and while a + k <= 149.  A maximum of 1e-30 has a = 107: 2^-125
//                   at k = 18.  A partial maximum of +inf sets the overflow word.
//   WINO3H16_PLAIN_SCALED  the self-play kernel with a STATIC input scale (RELU true): `aux_n` is not a count but the
//                   layer's exponent a, |a| <= ACT_EXP_MAX, chosen on the host (a calibration forward, or the response to
//                   an overflow) and the same for every launch until the host changes it -- so a board's bits depend on a,
//                   never on the other boards of its batch.  As in DGRAD the raw tiles are multiplied by 2^a before the
//                   transform and 2^-a goes into the 1 / S of the bias FMA (both exact); no `aux` folding, no barrier in
//                   front of the first item.  Bias, residual, ReLU, the non-finite check and the overflow word are
//                   WINO3H16_PLAIN's.  The host keeps 2^-a / S a normal float (apz_set_trunk_act_exponents clamps a), and it
//                   launches WINO3H16_PLAIN itself for a = 0.
enum { WINO3H16_PLAIN = 0, WINO3H16_STATS = 1, WINO3H16_DGRAD = 2, WINO3H16_PLAIN_SCALED = 3 };

// WINO3H16_PLAIN_SCALED: where the host puts a layer's calibration maximum m = max |input|, and why.  The split is proven
// for max |x| 2^a < 655 (|V| <= 100 max |x| must stay below the fp16 limit 65 504).  DGRAD's window [2^7, 2^8) fits a scale
// taken from the EXACT maximum of the tensor the launch reads.  A static exponent is taken from one calibration batch and
// then meets positions that were not in it, so the window sits three binades lower: a = ACT_WINDOW_LOG2 - floor(log2 m)
// puts m 2^a into [2^4, 2^5) -- at least 655 / 32 = 20 times headroom above the calibration maximum, and the lo term of
// the split stays a normal fp16 number (full 22-bit operands) for inputs down to 2^4 2^-7 = 2^-3 after scaling, 7 binades
// below the maximum (unscaled, that floor of 2^-3 is absolute: DESIGN.md section 4).
constexpr int ACT_WINDOW_LOG2 = 4;
constexpr int ACT_EXP_MAX = 100;          // |a| <= 100: 2^a and 2^-a are normal floats

// a with m 2^a in [2^ACT_WINDOW_LOG2, 2^(ACT_WINDOW_LOG2 + 1)); 0 for m == 0; clamped to |a| <= ACT_EXP_MAX.  m finite, >= 0.
inline int act_exponent_for(float m) {
    if (!(m > 0.f)) return 0;
    int ex;
    std::frexp((double)m, &ex);           // m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1 (subnormal floats included)
    const int a = ACT_WINDOW_LOG2 - (ex - 1);
    return a < -ACT_EXP_MAX ? -ACT_EXP_MAX : (a > ACT_EXP_MAX ? ACT_EXP_MAX : a);
}

// a with max |x| 2^a in [2^7, 2^8); 0 for max 0 (as f16x2_scale_for(0)); clamped to [-64, 110]: 2^110 and 2^-110 are
// normal floats, and maxima down to 2^-103 (1e-31) still reach the window.  (A maximum of +inf -- the launch sets the
// overflow word for it -- gives -64.)
__device__ __forceinline__ int wino3h16_dgrad_exponent(float m) {
    if (!(m > 0.f)) return 0;
    const int e = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 255u);   // m in [2^(e-127), 2^(e-126)) (e = 0: subnormal)
    const int a = 134 - e;
    return a < -64 ? -64 : (a > 110 ? 110 : a);
}

template <bool RESID, bool RELU = true, int FORM = WINO3H16_PLAIN>
__global__ __launch_bounds__(512) void trunk15_wino3h16_kernel(const float* __restrict__ in, const void* __restrict__ upk,
                                                               const float* __restrict__ bias, const float* __restrict__ resid,
                                                               float* __restrict__ out, int n, unsigned* __restrict__ flag,
                                                               void* __restrict__ aux, int aux_n) {
    using T = Wino3H16;
    constexpr bool STATS = FORM == WINO3H16_STATS, DGRAD = FORM == WINO3H16_DGRAD, SCALED = FORM == WINO3H16_PLAIN_SCALED;
    static_assert(FORM == WINO3H16_PLAIN || SCALED || !RELU, "the training forms have no ReLU");
    static_assert(!SCALED || RELU, "the scaled form is a self-play form");
    static_assert(!STATS || !RESID, "STATS: bias only");
#ifdef APZ_WINO3H_STAMPS
    // phases as trunk15_wino3h.h: 0 item prologue, 1 chunk barrier waits, 2 chunk bodies, 3 staging + stores, 4 epilogue first
    // barriers, 5 item start, 6 s_memrealtime ticks, 7 total, 8 M write + residual, 9 gather + output transform, 10 second barriers
    unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_t = __builtin_readcyclecounter();
    const unsigned long long st_t0 = st_t, st_r0 = __builtin_amdgcn_s_memrealtime();
#define APZH16_STAMP(ph_)                                             \
    {                                                                 \
        const unsigned long long now_ = __builtin_readcyclecounter(); \
        st_acc[ph_] += now_ - st_t;                                   \
        st_t = now_;                                                  \
    }
#else
#define APZH16_STAMP(ph_)
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* vbase = reinterpret_cast<char*>(lds);                           // [2][V_BYTES]
    float* mq = lds;                                                      // epilogue: M[pos 36][co 16][col 32] (over V)
    float* stg = mq + T::MQ_FLOATS;                                       // epilogue: [wave 8][plane 4][16 x 20]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const WinoItems items(n, (int)gridDim.x, (int)blockIdx.x);   // (board pair, channel half) per item
    const int nitems = items.nitems;
    if (items.np == 0) return;

    // DGRAD: the input scale 2^a and 2^-a from the partial maxima (the eight wave maxima pass through V[0], which the first
    // item's transform writes only behind its barrier)
    float xsc = 1.f, xisc = 1.f;
    bool aux_inf = false;                             // DGRAD: a partial maximum is +inf -- no scale fits, the result is void
    if constexpr (DGRAD) {
        const float* pm = static_cast<const float*>(aux);
        float m = 0.f;
        for (int i = tid; i < aux_n; i += 512) m = fmaxf(m, fabsf(pm[i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (lane == 0) lds[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 8; w++) m = fmaxf(m, lds[w]);
        const int a = __builtin_amdgcn_readfirstlane(wino3h16_dgrad_exponent(m));
        aux_inf = !(m <= 3.4028234664e38f);
        f16x2_pow2_pair(a, xsc, xisc);
    }
    if constexpr (SCALED) f16x2_pow2_pair(aux_n, xsc, xisc);   // the host's exponent: a kernel argument, the same in every wave

    const unsigned plane_b = T::GPLANE * 4;
    const unsigned act_bytes = rows16_bytes(n);
    const __amdgpu_buffer_rsrc_t r_in = wino_rsrc(in, act_bytes), r_res = wino_rsrc(RESID ? resid : in, act_bytes);
    const __amdgpu_buffer_rsrc_t r_out = wino_rsrc(out, act_bytes), r_u = wino_rsrc(upk, (unsigned)T::UPK_BYTES);
    const __amdgpu_buffer_rsrc_t r_st = wino_rsrc(STATS ? aux : out, STATS ? (unsigned)n * T::C * 16u : 0u);

    // ---- transform role: board tb, channels 4 cq .. 4 cq + 3 of the chunk; the lane roles (tile, channel pair cpl, channel
    // parity e) and the transform's passes are wino_f16x2.h's.
    const int tb = wave & 1, cq = wave >> 1;
    const int ttx = lane & 3, tty = (lane >> 2) & 3, tile = lane & 15, cpl = (lane >> 4) & 1, e = lane >> 5;
    const int chl = 4 * cq + 2 * cpl + e;                          // channel of the chunk (0..15)
    const int cpair = 2 * cq + cpl;                                // channel pair (0..7): V half cpair >> 2, dword cpair & 3
    const int vcol = tb * 16 + tile;
    // bytes in a V term: column vcol, swizzled half, dword of the pair; lanes of the even channel write positions k = 0..2 of a
    // row, lanes of the odd channel k = 3..5
    const int tv_off = vcol * 32 + (((cpair >> 2) ^ ((vcol >> 3) & 1)) * 16) + (cpair & 3) * 4 + e * 3 * T::VPOS;
    const unsigned col16_mask = ttx == 3 ? 0u : 0xffffffffu;       // column 16 does not exist
    const float c4l = ttx == 0 ? 0.f : 4.f;                        // column -1 of the first tile column is the zero border
    // raw tile rows: the lane part of the address (channel within the wave's four, tile); row 15 (tile row 3, its row 3) is
    // out of range (0x80000000: the load returns zeros)
    const unsigned raw_vo = (unsigned)(2 * cpl + e) * plane_b + (unsigned)(tty * 4 * 16 + ttx * 4) * 4;
    const unsigned raw_vo3 = tty == 3 ? 0x80000000u : raw_vo + 3u * 64u;
    f32x4 raw[4];
    auto raw_load = [&](int t, int c) {                            // chunk c of item t -> raw
        const int bdp = 2 * items.pair(t) + tb;
        const int bd = bdp < n ? bdp : n - 1;
        const unsigned so = (unsigned)(bd * T::C + c * T::CK + 4 * cq) * plane_b;
#pragma unroll
        for (int r = 0; r < 3; r++) raw[r] = bload(r_in, raw_vo + (unsigned)r * 64u, so);
        raw[3] = bload(r_in, raw_vo3, so);
    };

    f32x2 tt[6][2];                                // vertical-pass results: rows 0..5, column pairs (0, 1), (2, 3)
    float oo[6];
    // (one-line lambdas, not direct calls: the compiler then simplifies each before it inlines it, which keeps the kernel's
    // instruction schedule)
    auto vpass = [&](int kc) { f16x2_vpass(raw, kc, tt); };
    auto col_pass = [&](int j) { f16x2_col_pass(tt, j, c4l, col16_mask, oo); };
    auto exchange = [&]() { f16x2_exchange(oo); };
    // (even channel's value, odd channel's value) of one position -> its hi and lo words in V
    auto emit = [&](char* vp, float ev, float od) {
        unsigned hu, lu;
        f16x2_split(ev, od, hu, lu);
        *reinterpret_cast<unsigned*>(vp) = hu;
        *reinterpret_cast<unsigned*>(vp + T::VTERM) = lu;
    };
    // The transform of one chunk (raw -> V[vpar]) in 27 slices, three per MFMA slot: 0, 1 the vertical pass (raw is free
    // behind it), 2 nothing, then per row j = 0..5: column pass, exchange, positions k = 0, 1, position k = 2
    auto tslice = [&](int vpar, auto KK) {
        constexpr int K = decltype(KK)::value;
        char* vp = vbase + vpar * T::V_BYTES + tv_off;
        if constexpr ((DGRAD || SCALED) && K == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) raw[r] *= xsc;      // exact: a power of two
        }
        if constexpr (K < 2) vpass(K);
        else if constexpr (K >= 3) {
            constexpr int j = (K - 3) / 4, part = (K - 3) % 4;
            if constexpr (part == 0) col_pass(j);
            else if constexpr (part == 1) exchange();
            else if constexpr (part == 2) {
                emit(vp + (j * 6 + 0) * T::VPOS, oo[0], oo[3]);
                emit(vp + (j * 6 + 1) * T::VPOS, oo[1], oo[4]);
            } else emit(vp + (j * 6 + 2) * T::VPOS, oo[2], oo[5]);
        }
    };
    auto transform = [&](int vpar) {
#define APZH16_TS(k) tslice(vpar, std::integral_constant<int, k>{});
        APZH16_TS(0) APZH16_TS(1) APZH16_TS(2) APZH16_TS(3) APZH16_TS(4) APZH16_TS(5) APZH16_TS(6) APZH16_TS(7) APZH16_TS(8)
        APZH16_TS(9) APZH16_TS(10) APZH16_TS(11) APZH16_TS(12) APZH16_TS(13) APZH16_TS(14) APZH16_TS(15) APZH16_TS(16)
        APZH16_TS(17) APZH16_TS(18) APZH16_TS(19) APZH16_TS(20) APZH16_TS(21) APZH16_TS(22) APZH16_TS(23) APZH16_TS(24)
        APZH16_TS(25) APZH16_TS(26)
#undef APZH16_TS
    };

    // ---- MFMA role: 32-channel half cc of the item's 64, position block (ri, ki)
    const int cc = wave >> 2, ri = (wave >> 1) & 1, ki = wave & 1, blk = wave & 3;
    const int r31 = lane & 31, hh = lane >> 5;
    const unsigned a_vo = lane * 16;                  // a unit: lanes 0-31 channels 0-7 of their output channel, 32-63 channels 8-15
    const int wpos0 = 18 * ri + 3 * ki;               // first position of this wave's block
    auto pos_off = [](int p9) { return (6 * (p9 / 3) + (p9 % 3)) * T::VPOS; };   // position p9 of the block, relative to wpos0

    // weight stream: the 18 units (position p9, H / L) of a chunk are contiguous, 144 per item and wave; a load is base +
    // (u / 4) * 4096 as the scalar offset + (u % 4) * 1024 as the immediate (u = 2 p9 + term)
    static constexpr int RING = APZH16_RING;
    static_assert(18 % RING == 0 && RING >= 2, "ring slots must tile two chunks");
    f16x8 ah[RING], al[RING];
    auto unit_base = [&](int t, int c) {
        const int cog = 2 * items.half(t) + cc;
        return (unsigned)(((cog * 4 + blk) * T::NCHUNK + c) * 18) * T::UNIT;
    };
    unsigned ub_cur = 0, ub_nxt = 0;
    auto unit_pair_at = [&](unsigned base, int p9, int slot) {
        const int u = 2 * p9;
        ah[slot] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_u, a_vo + (unsigned)(u & 3) * T::UNIT,
                                                                                  base + (unsigned)(u >> 2) * 4u * T::UNIT, 0));
        al[slot] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_u, a_vo + (unsigned)((u + 1) & 3) * T::UNIT,
                                                                                  base + (unsigned)((u + 1) >> 2) * 4u * T::UNIT, 0));
    };
    // position p9 (0 .. 8 + RING - 1) counted from the start of the current chunk
    auto unit_load = [&](int p9, int slot) {
        if (p9 < 9) unit_pair_at(ub_cur, p9, slot);
        else unit_pair_at(ub_nxt, p9 - 9, slot);
    };

    unsigned nonfinite = aux_inf ? 1u : 0u;           // any pre-ReLU output of this thread that is not a finite number

    ub_cur = ub_nxt = unit_base(0, 0);
#pragma unroll
    for (int u = 0; u < RING - 1; u++) unit_load(u, u);
    raw_load(0, 0);
    // the later-dispatched half of the workgroup (waves 4..7, the SIMD partners of 0..3) loses every issue arbitration by age
    // (MI355X_MICROARCH.md, "Two waves per SIMD", item 4): one static priority raise evens it out
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);

    for (int t = 0; t < nitems; t++) {
        const int h = items.half(t);
        const int bd0 = 2 * items.pair(t);
        const bool two = bd0 + 1 < n;
        // ---- item prologue: raw holds chunk 0 (requested in front of the loop / in the last epilogue step): V[0]
        __syncthreads();                              // the previous item's M / staging (over V) consumed
        APZH16_STAMP(5)
        transform(0);
        raw_load(t, 1);
        f32x16h acc[9];
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[p][v] = 0.f;
        APZH16_STAMP(0)

        // ---- chunk loop.  Chunk c: [barrier] MFMAs over V[c & 1]: 9 slots = the wave's 9 positions, each 3 MFMAs + three
        // slices of the transform of raw (= chunk c + 1) -> V[(c + 1) & 1] + the refill of the weight ring slot freed by the
        // previous slot; behind slot APZH16_RAW_SLOT (the vertical pass long done) raw <- chunk c + 2.
        f16x8 bfr[2];
        auto chunk = [&](int c, auto PAR, auto XF, auto LD) {
            constexpr int par = decltype(PAR)::value;
            constexpr bool xf = decltype(XF)::value, ld = decltype(LD)::value;
            __syncthreads();                          // V[par] complete; V[1 - par] free
            APZH16_STAMP(1)
            ub_cur = ub_nxt;
            ub_nxt = c + 1 < T::NCHUNK ? ub_cur + 18u * T::UNIT : (t + 1 < nitems ? unit_base(t + 1, 0) : ub_cur + 18u * T::UNIT);
            const char* vp = vbase + par * T::V_BYTES;
            // per-lane fragment offset from an opaque copy of the lane id (see trunk15_wino3h.h)
            int le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(le));
            const int fcol = le & 31;
            const int b_hi = wpos0 * T::VPOS + fcol * 32 + ((((le >> 5) & 1) ^ ((fcol >> 3) & 1)) * 16);   // B = Vhi, 16 channels
            const int b_lo = b_hi + T::VTERM;                                                                // B = Vlo
            bfr[0] = *reinterpret_cast<const f16x8*>(vp + b_hi);
            bfr[1] = *reinterpret_cast<const f16x8*>(vp + b_lo);
#define APZH16_SLOT(k)                                                                                                   \
            {                                                                                                            \
                constexpr int p9 = (k), slot = (par * 9 + (k)) % RING;                                                   \
                /* the small products first: H . Vlo, L . Vhi, then H . Vhi; every V fragment is re-read for the next    \
                   position right behind the last MFMA that uses it */                                                   \
                acc[p9] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[slot], bfr[1], acc[p9], 0, 0, 0);                    \
                if (p9 + 1 < 9) bfr[1] = *reinterpret_cast<const f16x8*>(vp + b_lo + pos_off(p9 + 1));                   \
                acc[p9] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[slot], bfr[0], acc[p9], 0, 0, 0);                    \
                acc[p9] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[slot], bfr[0], acc[p9], 0, 0, 0);                    \
                if (p9 + 1 < 9) bfr[0] = *reinterpret_cast<const f16x8*>(vp + b_hi + pos_off(p9 + 1));                   \
                if (xf) {                                                                                                \
                    tslice(1 - par, std::integral_constant<int, 3 * (k)>{});                                             \
                    tslice(1 - par, std::integral_constant<int, 3 * (k) + 1>{});                                         \
                    tslice(1 - par, std::integral_constant<int, 3 * (k) + 2>{});                                         \
                }                                                                                                        \
                if ((k) == APZH16_RAW_SLOT && ld) raw_load(t, c + 2);                                                    \
                /* position k + RING - 1 goes into the ring slot of position k - 1, whose MFMAs are done */             \
                unit_load((k) + RING - 1, (par * 9 + (k) + RING - 1) % RING);                                            \
                __builtin_amdgcn_sched_barrier(0);                                                                       \
            }
            APZH16_SLOT(0) APZH16_SLOT(1) APZH16_SLOT(2) APZH16_SLOT(3) APZH16_SLOT(4) APZH16_SLOT(5) APZH16_SLOT(6) APZH16_SLOT(7) APZH16_SLOT(8)
#undef APZH16_SLOT
            APZH16_STAMP(2)
        };
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        using Y = std::true_type;
        using N = std::false_type;
        for (int c = 0; c < T::NCHUNK - 2; c += 2) {
            chunk(c, P0{}, Y{}, Y{});
            chunk(c + 1, P1{}, Y{}, Y{});
        }
        chunk(T::NCHUNK - 2, P0{}, Y{}, N{});         // transforms the last chunk; nothing left to load
        chunk(T::NCHUNK - 1, P1{}, N{}, N{});         // MFMAs only

        // ---- epilogue.  Four steps of 16 output channels = channels 8 s .. 8 s + 7 of BOTH 32-channel
        // halves.  Layout of the 32 x 32 tile: lane (col = lane & 31, hh = lane >> 5), register v: channel (v & 3) + 8 (v >> 2) +
        // 4 hh.  M row (of 16) = 8 cc + channel - 8 s.
        const int cosel = lane >> 5;               // gather role: M row 2 wave + cosel of the step's 16, column lane & 31
        const int col = lane & 31, gbd = col >> 4, gtile = col & 15;
        const int gty = gtile >> 2, gtx = gtile & 3;
        float* sw = stg + wave * (4 * T::SPLANE);
        const int s_lin = (lane >> 2) * T::SROW + (lane & 3) * 4;
        const unsigned ep_vo = lane < 60 ? lane * 16 : 0x80000000u;
        auto row_chan = [&](int s, int row) { return (2 * h + (row >> 3)) * 32 + 8 * s + (row & 7); };
        f32x4 rs[4];
        auto resid_request = [&](int s) {
#pragma unroll
            for (int pl = 0; pl < 4; pl++) {
                const int bdp = bd0 + (pl & 1);
                const int bd = bdp < n ? bdp : n - 1;
                rs[pl] = bload(r_res, ep_vo, (unsigned)(bd * T::C + row_chan(s, 2 * wave + (pl >> 1))) * plane_b);
            }
        };
        if (RESID) resid_request(0);
        auto ep_step = [&](auto S_) {
            constexpr int s = decltype(S_)::value;
            __syncthreads();                       // MFMAs over V done (s = 0) / M and staging of the previous step consumed
            APZH16_STAMP(4)
            {
                float* mw = mq + wpos0 * 512 + (8 * cc + 4 * hh) * 32 + r31;
#pragma unroll
                for (int p9 = 0; p9 < 9; p9++)
#pragma unroll
                    for (int e4 = 0; e4 < 4; e4++) mw[(6 * (p9 / 3) + p9 % 3) * 512 + e4 * 32] = acc[p9][4 * s + e4];
            }
            if (RESID) {
#pragma unroll
                for (int pl = 0; pl < 4; pl++) *reinterpret_cast<f32x4*>(sw + pl * T::SPLANE + s_lin) = rs[pl];
            }
            // the accumulators are spent: the next item's first raw tiles
            if (s == 3 && t + 1 < nitems) raw_load(t + 1, 0);
            APZH16_STAMP(8)
            __syncthreads();                       // M complete
            APZH16_STAMP(10)
            {
                const int co16 = 2 * wave + cosel;
                const float* mp = mq + co16 * 32 + col;
                float hrow[6][4];                   // the k-direction transform of every row
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    float m[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) m[k] = mp[(6 * i + k) * 512];
                    wino_out_row(m[0], m[1], m[2], m[3], m[4], m[5], hrow[i][0], hrow[i][1], hrow[i][2], hrow[i][3]);
                }
                if (RESID && s + 1 < 4) resid_request(s + 1);
                const int ch = row_chan(s, co16);
                const float bv = bias[ch];
                const float is = (DGRAD || SCALED) ? bias[128 + ch] * xisc : bias[128 + ch];   // 1 / S of the channel (a power of two)
                float* sp = sw + (cosel * 2 + gbd) * T::SPLANE + (4 * gty) * T::SROW + 4 * gtx;
                f32x4 y[4];
#pragma unroll
                for (int ee = 0; ee < 4; ee++) {
                    float o0, o1, o2, o3;
                    wino_out_row(hrow[0][ee], hrow[1][ee], hrow[2][ee], hrow[3][ee], hrow[4][ee], hrow[5][ee], o0, o1, o2, o3);
                    y[0][ee] = o0, y[1][ee] = o1, y[2][ee] = o2, y[3][ee] = o3;
                }
                float chk = 0.f;
                float r1[4], r2[4];                  // STATS: the row sums of the tile
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    f32x4 v;
#pragma unroll
                    for (int ee = 0; ee < 4; ee++) v[ee] = __builtin_fmaf(y[a][ee], is, bv);
                    if (RESID) v += *reinterpret_cast<const f32x4*>(sp + a * T::SROW);   // (wave-private: written above by this wave)
                    chk += wino_sum4(v);
#pragma unroll
                    for (int ee = 0; ee < 4; ee++) v[ee] = RELU ? fmaxf(v[ee], 0.f) : v[ee];
                    if (gtx == 3) v[3] = 0.f;      // column 15 is the halo column of the rows16 layout
                    *reinterpret_cast<f32x4*>(sp + a * T::SROW) = v;
                    if constexpr (STATS) {
                        r1[a] = (v[0] + v[1]) + (v[2] + v[3]);
                        r2[a] = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                    }
                }
                nonfinite |= wino_nonfinite(chk) ? 1u : 0u;
                if constexpr (STATS) {
                    if (gty == 3) r1[3] = 0.f, r2[3] = 0.f;          // board row 15 does not exist
                    // the 16 tiles of this (channel, board) are one DPP row: lanes 16 (2 cosel + gbd) .. + 15
                    const double d1 = (double)wino3_row16_sum((r1[0] + r1[1]) + (r1[2] + r1[3]));
                    const double d2 = (double)wino3_row16_sum((r2[0] + r2[1]) + (r2[2] + r2[3]));
                    const bool mine = gtile == 0 && (gbd == 0 || two);
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    const unsigned so = (unsigned)(ch * n + bd0 + gbd) * 16u;
                    bstore(r_st, mine ? so : 0x80000000u, 0u, __builtin_bit_cast(f32x4, f64x2{d1, d2}));
                }
            }
            APZH16_STAMP(9)
            wave_lds_fence();
#pragma unroll
            for (int pl = 0; pl < 4; pl++) {
                const f32x4 pv = *reinterpret_cast<const f32x4*>(sw + pl * T::SPLANE + s_lin);
                const unsigned vo = ((pl & 1) == 0 || two) ? ep_vo : 0x80000000u;   // the missing second board of an odd batch
                bstore(r_out, vo, (unsigned)((bd0 + (pl & 1)) * T::C + row_chan(s, 2 * wave + (pl >> 1))) * plane_b, pv);
            }
            APZH16_STAMP(3)
        };
        ep_step(std::integral_constant<int, 0>{});
        ep_step(std::integral_constant<int, 1>{});
        ep_step(std::integral_constant<int, 2>{});
        ep_step(std::integral_constant<int, 3>{});
    }
    // (a plain store: every writer writes the same 1, and the word may live in pinned host memory)
    if (nonfinite && flag) *reinterpret_cast<volatile unsigned*>(flag) = 1u;
#ifdef APZ_WINO3H_STAMPS
    st_acc[7] = __builtin_readcyclecounter() - st_t0;
    st_acc[6] = __builtin_amdgcn_s_memrealtime() - st_r0;
    if (lane == 0 && blockIdx.x < 4)
        for (int i = 0; i < 12; i++) apz_wino3h16_stamps[(blockIdx.x * 8 + wave) * 12 + i] = st_acc[i];
#endif
#undef APZH16_STAMP
}

}  // namespace apz
