// Trunk 3x3 convolution (128 -> 128 channels, 15x15 board) + folded BN + (residual) + ReLU as a fused F(4x4,3x3)
// Winograd convolution whose 36 per-position GEMMs run on the FP16 matrix pipe at fp32-level accuracy: every fp32 operand
// is split into TWO fp16 terms (x = hi + lo, 11 significant bits each, both rounded to nearest even: |x - hi - lo| <=
// 2^-22 |x| while lo is a normal fp16 number, <= 2^-25 absolute below that) and a product is the three term products
// hi.hi + hi.lo + lo.hi (+ lo.lo, which rides along for free), accumulated in fp32 by the MFMA.  gfx950 only.
// Successor of trunk15_wino3b.h (three bf16 terms, six products): half the matrix instructions, a third fewer weight
// bytes, a third fewer LDS fragment reads and half the split's vector instructions (round 6; profiles/r06_wino3h.md).
//
// Range.  fp16 holds 6.1e-5 .. 65504 in normal numbers, so both operands are placed by powers of two:
//   * weights: U = G g G^T of output channel co is multiplied by S[co] = 2^k chosen by the packer (weights_pack.h,
//     f16x2_scale_for) so that max |U S| sits in [2^13, 2^14); the epilogue multiplies by 1 / S[co] (exact) inside the bias FMA.
//   * activations: V = B^T d B is NOT scaled.  |V| <= 100 max|d|: post-ReLU activations up to 655 are representable;
//     values below 2^-3 keep an absolute error of 2^-25.  An input that does overflow gives +-inf / NaN in the
//     accumulators; the epilogue checks every pre-ReLU value (a NaN would otherwise be clamped to 0 silently) and raises
//     `flag[0]`, on which the engine repeats the forward on the exact-fp32 kernel (apz_engine.hip).
//
// Shape: trunk15_wino3b.h's, unchanged (read its header for the measured reasons) -- work item = (board pair, 64 output
// channels, all 36 positions); eight waves, two per SIMD; wave = (32-channel half, 3x3 position block) with 9 x 16 = 144
// accumulator registers; 16 chunks of 8 input channels per item, one barrier per chunk; raw planes by LDS-DMA, the input
// transform B^T d B (fp32 VALU) by all 512 threads in 18 slices between the MFMAs; weights straight from L2 into a
// register ring.  What changed:
//   * K packing.  One v_mfma_f32_32x32x16_f16 contracts k = 16 = 8 channels x 2 weight terms:
//         A = [Whi | Wlo] (lanes 0-31 hold k = 0-7, lanes 32-63 k = 8-15), B = [Vt | Vt] for t = lo, then t = hi:
//     two MFMAs per (position, 32 output channels, 8 input channels) instead of three, ONE 16-byte weight load per lane
//     and unit (1 KB per wave, fully coalesced; 4 bytes per weight as in the fp32 kernel), two V fragments per position.
//   * The split: hi = v_cvt_pk_f16_f32 of (even channel's value, odd channel's), lo = v_fma_mixlo / mixhi_f16 of the exact
//     remainders: 3 vector instructions per position and channel pair (bf16 x 3: 11); the two channels of a pair meet by
//     ONE v_permlane16_swap_b32 per value pair (DPP: two selects and a move); the transform itself on column pairs (v_pk).
//
// Layouts.  in / resid / out: rows16 [n][128][15][16] (col 15 == 0).  raw (LDS): as Wino3B.  V (LDS): [pos 36][term 2]
// [col 32][8 ch] fp16, col = board * 16 + tile: a B fragment is ONE conflict-free ds_read_b128 (both lane halves read the
// same 16 bytes).  upk: [cog 4][block 4][chunk 16][position 9][term 2][co 32][8 ch] fp16.  bias: [128 bias][128 1/S].
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wino_f16x2.h"

namespace apz {

struct Wino3H {
    static constexpr int C = 128, CK = 8, NCHUNK = C / CK;             // 16 chunks of 8 input channels
    static constexpr int GPLANE = 240;
    // raw input tile: as Wino3B (planes as in HBM + two zero rows behind each; plane stride 272 floats)
    static constexpr int RROW = 16, RPS = 17 * RROW, RFRONT = 32;
    static constexpr int RAW_FLOATS = RFRONT + 2 * CK * RPS + 32;      // 4416 floats (17.3 KiB)
    static constexpr int VTERM = 32 * 16, VPOS = 2 * VTERM, V_BYTES = 36 * VPOS;   // 512, 1024, 36864 bytes
    static constexpr int MAIN_BYTES = 2 * RAW_FLOATS * 4 + 2 * V_BYTES; // 109056
    static constexpr int UNIT = 2 * 32 * 16;                           // bytes of one (cog, block, chunk, position): 1024
    static constexpr size_t UPK_BYTES = (size_t)4 * 4 * NCHUNK * 9 * UNIT;         // 2.36 MB per layer
    static constexpr int BIAS_FLOATS = 256;                            // [bias 128][1 / S 128]
    // epilogue: M and the store staging alias the two V buffers (and what lies behind them); the raw tiles stay untouched
    static constexpr int MQ_FLOATS = 36 * 16 * 32;                     // 73728 bytes at the V base
    static constexpr int SROW = 20, SPLANE = 16 * SROW;                // staging plane: 16 rows x 20 floats
    static constexpr int STG_FLOATS = 8 * 4 * SPLANE;                  // 8 waves x 4 planes (40 KiB)
    static constexpr int LDS_BYTES = 2 * RAW_FLOATS * 4 + (MQ_FLOATS + STG_FLOATS) * 4;   // 150016
    static_assert(LDS_BYTES >= MAIN_BYTES, "epilogue area covers V");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    // byte offset of element (co, ci, pos, term) in the packed weights
    __host__ __device__ static size_t upk_offset(int co, int ci, int pos, int term) {
        const int i = pos / 6, k = pos % 6, ri = i / 3, ki = k / 3, p9 = 3 * (i % 3) + (k % 3);
        const int cog = co >> 5, r = co & 31, chunk = ci >> 3, w = 2 * ri + ki;
        const int ch = ci & 7;
        return ((((size_t)(cog * 4 + w) * NCHUNK + chunk) * 9 + p9) * 2 + term) * VTERM + r * 16 + ch * 2;
    }
};

#ifdef APZ_WINO3H_STAMPS
__device__ unsigned long long apz_wino3h_stamps[4 * 8 * 12];   // [workgroup 4][wave 8][phase 12]
#endif

#ifndef APZH_RING
#define APZH_RING 6          /* weight units in registers (RING - 1 in flight); 6 or 9 */
#endif

template <bool RESID, bool RELU = true>
__global__ __launch_bounds__(512) void trunk15_wino3h_kernel(const float* __restrict__ in, const void* __restrict__ upk,
                                                             const float* __restrict__ bias, const float* __restrict__ resid,
                                                             float* __restrict__ out, int n, unsigned* __restrict__ flag) {
    using T = Wino3H;
#ifdef APZ_WINO3H_STAMPS
    // phases: 0 item prologue (transform), 1 chunk barrier waits, 2 chunk bodies, 3 epilogue work, 4 epilogue barrier waits,
    // 5 item start (wait for the first planes + barrier), 6 = s_memrealtime ticks (100 MHz) of the whole wave, 7 total;
    // epilogue detail: 4 = waits at a step's first barrier, 8 = M write + residual, 10 = waits at the second barrier, 9 = gather +
    // output transform, 3 = staging + stores
    unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_t = __builtin_readcyclecounter();
    const unsigned long long st_t0 = st_t, st_r0 = __builtin_amdgcn_s_memrealtime();
#define APZH_STAMP(ph_)                                               \
    {                                                                 \
        const unsigned long long now_ = __builtin_readcyclecounter(); \
        st_acc[ph_] += now_ - st_t;                                   \
        st_t = now_;                                                  \
    }
#else
#define APZH_STAMP(ph_)
#endif
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* rawb = lds;                                                    // [2][RAW_FLOATS]
    char* vbase = reinterpret_cast<char*>(lds + 2 * T::RAW_FLOATS);       // [2][V_BYTES]
    float* mq = lds + 2 * T::RAW_FLOATS;                                  // epilogue: M[pos 36][co 16][col 32] (over V)
    float* stg = mq + T::MQ_FLOATS;                                       // epilogue: [wave 8][plane 4][16 x 20]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const WinoItems items(n, (int)gridDim.x, (int)blockIdx.x);   // (board pair, channel half) per item
    const int nitems = items.nitems;
    if (items.np == 0) return;

    const unsigned plane_b = T::GPLANE * 4;
    const unsigned act_bytes = rows16_bytes(n);
    const __amdgpu_buffer_rsrc_t r_res = wino_rsrc(RESID ? resid : in, act_bytes), r_out = wino_rsrc(out, act_bytes);
    const __amdgpu_buffer_rsrc_t r_u = wino_rsrc(upk, (unsigned)T::UPK_BYTES);

    // ---- staging role: wave w brings planes w (board 0) and w + 8 (board 1) of a chunk into LDS by LDS-DMA
    // (buffer_load_dwordx4 ... lds; lanes 60..63 out of range: row 15 of the tile stays zero).  Inline assembly: hipcc's
    // wait-count insertion does not see these loads.  They need no wait of their own: a plane requested in slot 1 of a
    // chunk is older than the weight loads issued behind it, whose data the MFMAs of a later slot wait for -- vector memory
    // operations complete in order -- and the tile is first read behind the next chunk's barrier.
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)rawb;   // LDS byte address of rawb
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    const unsigned long long in_a = (unsigned long long)in;
    const i32x4_ dma_rsrc = {(int)(unsigned)(in_a & 0xffffffffull), (int)(unsigned)((in_a >> 32) & 0xffffull), (int)act_bytes, 0x00020000};
    const unsigned dma_vo = lane < 60 ? lane * 16 : 0x80000000u;
    auto raw_dma = [&](int t, int c, int par) {       // chunk c (clamped) of item t -> raw[par]
        c = c < T::NCHUNK ? c : T::NCHUNK - 1;
        const int bd0_ = 2 * items.pair(t);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int plane = 8 * j + wave;           // board j, channel `wave`
            const int bdp = bd0_ + j;
            const int bd = bdp < n ? bdp : n - 1;
            const unsigned so = (unsigned)(bd * T::C + c * T::CK + wave) * plane_b;
            const unsigned dst = lds0 + (unsigned)(par * T::RAW_FLOATS + T::RFRONT + plane * T::RPS) * 4;
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(dma_vo), "s"(dma_rsrc), "s"(dst), "s"(so) : "memory");
        }
    };

    // ---- MFMA role: 32-channel half cc of the item's 64, position block (ri, ki)
    const int cc = wave >> 2, ri = (wave >> 1) & 1, ki = wave & 1, blk = wave & 3;
    const int r31 = lane & 31, hh = lane >> 5;
    const unsigned a_vo = lane * 16;                  // A = [Whi | Wlo]: lanes 0-31 the hi terms of their channel, 32-63 the lo terms
    const int wpos0 = 18 * ri + 3 * ki;               // first position of this wave's block
    auto pos_off = [](int p9) { return (6 * (p9 / 3) + (p9 % 3)) * T::VPOS; };   // position p9 of the block, relative to wpos0

    // weight stream: unit index of this wave = (item t * 16 + chunk c) * 9 + p9
    static constexpr int RING = APZH_RING;
    static_assert(RING == 6 || RING == 9 || RING == 18, "ring slots must tile two chunks");
    f16x8 af[RING];
    // byte offset of unit (t, c, 0).  The units of an item are contiguous (144 x 1 KB per wave), so a chunk body needs two
    // uniform bases -- this chunk's and the next one's (which may belong to the next item) -- and every load is base +
    // (p9 / 4) * 4096 as the scalar offset + (p9 % 4) * 1024 as the instruction's immediate: ~6 scalar instructions per chunk
    // instead of five per load.  Behind the last chunk of the last item the "next" base just runs on (unused data; the buffer
    // descriptor bounds it).
    auto unit_base = [&](int t, int c) {
        const int cog = 2 * items.half(t) + cc;
        return (unsigned)(((cog * 4 + blk) * T::NCHUNK + c) * 9) * T::UNIT;
    };
    unsigned ub_cur = 0, ub_nxt = 0;                  // bases of the chunk being multiplied and of the one after it
    auto unit_load_at = [&](unsigned base, int p9, int slot) {
#if defined(APZH_ABL_W) && APZH_ABL_W == 2   /* measurement build: every weight load reads the same (L1-resident) unit */
        af[slot] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_u, a_vo, (unsigned)(cc * 4 + blk) * T::UNIT + 0u * (base + p9), 0));
#else
        af[slot] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_u, a_vo + (unsigned)(p9 & 3) * T::UNIT,
                                                                                  base + (unsigned)(p9 >> 2) * 4u * T::UNIT, 0));
#endif
    };
    // unit p9 (0 .. 8 + RING - 1) counted from the start of the current chunk
    auto unit_load = [&](int p9, int slot) {
        if (p9 < 9) unit_load_at(ub_cur, p9, slot);
        else unit_load_at(ub_nxt, p9 - 9, slot);
    };

    auto af_keep = [&](int s_) { asm volatile("" ::"v"(af[s_])); };   // (measurement builds)
    (void)af_keep;
    unsigned nonfinite = 0;                           // any pre-ReLU output of this thread that is not a finite number

    // Everything that depends on the row half of the transform role is instantiated twice (wave-uniform branch below)
    auto run = [&](auto PH) {
        constexpr int ph = decltype(PH)::value;
        // ---- transform role: board tb, row half ph, channels 4 ch4 .. 4 ch4 + 3.  lane -> (tile column ttx = bits 0-1, tile
        // row tty = bits 2 and 5, pair cpl = bit 3, channel parity e = bit 4): the two channels of a pair sit 16 lanes apart
        // (v_permlane16_swap_b32 exchanges them, below), and every 16-lane group a ds_read_b128 is served in ({0-3,12-15,
        // 20-27}, {4-11,16-19,28-31}, the same + 32) holds all sixteen (channel of four, ttx): with the plane stride of 272
        // floats (68 bank quads = 4 mod 16; a tile row is 16 quads) its reads fall on sixteen different bank quads.
        const int tb = wave & 1, ch4 = wave >> 2;
        const int ttx = lane & 3, cpl = (lane >> 3) & 1, e = (lane >> 4) & 1;
        const int tty = 2 * (lane >> 5) + ((lane >> 2) & 1);
        const int tile = 4 * tty + ttx, chl = 4 * ch4 + 2 * cpl + e;          // channel of the chunk (0..7)
        const int tr_off = T::RFRONT + (tb * 8 + chl) * T::RPS + (4 * tty - 1 + ph) * T::RROW + 4 * ttx;
        const unsigned col16_mask = ttx == 3 ? 0u : 0xffffffffu;   // column 16 does not exist: the word there is column 0 of the next row
        // bytes: column tb * 16 + tile, dword = channel pair (low half: the even channel); lanes of the even channel pack
        // positions k = 0..2 of a row, lanes of the odd channel k = 3..5
        const int tv_off = tb * 256 + tile * 16 + (2 * ch4 + cpl) * 4 + e * 3 * T::VPOS;
        // All of the transform runs on column PAIRS (v_pk_* instructions: vector instruction slots, not flops, are what the
        // chunk loop is short of -- profiles/r06_wino3h.md): pair 0 = columns (0, 1), 1 = (2, 3), 2 = the halo (-1, 4).
        f32x2 xr[5][2];                                // five patch rows: the two centre pairs
        f32x2 tt[3][3];                                // row-pass results (rows 3 ph .. 3 ph + 2) of the three column pairs
        float oo[6];
        // the patch rows come out of LDS one MFMA slot before the row pass uses them (slice 0 only issues the reads: an
        // in-order wave that waits for an LDS round trip right behind its reads cannot issue its next MFMAs meanwhile)
        float xhl[5], xhr[5];                          // the halo columns (-1 and 4) of the five patch rows
#ifndef APZH_HALO_DPP
#define APZH_HALO_DPP 2      /* the halo columns (-1 and 4) from the neighbouring tile lanes by DPP; 0: two LDS reads per row, 4-way bank
                                conflicted (36 % of the kernel's LDS cycles): 65.1 / 68.7 us instead of 62.0 / 65.6 (profiles/r06_wino3h.md) */
#endif
        const unsigned col0_mask = ttx == 0 ? 0u : 0xffffffffu;    // (APZH_HALO_DPP) column -1 of the first tile column is the zero border
        const float c4l = ttx == 0 ? 0.f : 4.f;                    // (APZH_HALO_DPP == 2) ... as the coefficient its only use carries
        auto row_load = [&](const float* rp) {
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const f32x4 c03 = *reinterpret_cast<const f32x4*>(rp + i * T::RROW);
                xr[i][0] = f32x2{c03[0], c03[1]};
                xr[i][1] = f32x2{c03[2], c03[3]};
                if (!APZH_HALO_DPP) {
                    xhl[i] = rp[i * T::RROW - 1];
                    xhr[i] = rp[i * T::RROW + 4];
                }
            }
        };
        auto row_pass = [&]() {
            f32x2 xh[5];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                if (APZH_HALO_DPP == 2) {
                    xh[i] = f32x2{0.f, 0.f};              // (unused: the halo columns are taken from the row-pass RESULTS below)
                } else if (APZH_HALO_DPP) {
                    // the four tile columns of a tile row are the four lanes of a quad: column -1 = column 3 of the lane below,
                    // column 4 = column 0 of the lane above (quad_perm [0,0,1,2] / [1,2,3,3]); the border lanes are masked
                    // (scalar copies first: hipcc 7.2 takes element 0 when __builtin_bit_cast is applied to a vector element directly)
                    const float c3 = xr[i][1][1], c0 = xr[i][0][0];
                    const int l = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c3), 0x90, 0xF, 0xF, true);
                    const int r = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c0), 0xF9, 0xF, 0xF, true);
                    xh[i] = f32x2{__builtin_bit_cast(float, (unsigned)l & col0_mask), __builtin_bit_cast(float, (unsigned)r & col16_mask)};
                } else {
                    xh[i] = f32x2{xhl[i], __builtin_bit_cast(float, __builtin_bit_cast(unsigned, xhr[i]) & col16_mask)};   // (no branch)
                }
            }
#pragma unroll
            for (int kc = 0; kc < (APZH_HALO_DPP == 2 ? 2 : 3); kc++) {
                f32x2 x[5];
#pragma unroll
                for (int i = 0; i < 5; i++) x[i] = kc < 2 ? xr[i][kc] : xh[i];
                if (ph == 0) {                         // x = patch rows 0..4: y0 = 4x0 - 5x2 + x4, y1/y2 = (x4 - 4x2) +- (x3 - 4x1)
                    const f32x2 a = fma2(-4.f, x[2], x[4]), b = fma2(-4.f, x[1], x[3]);
                    tt[0][kc] = fma2(4.f, x[0], fma2(-5.f, x[2], x[4]));
                    tt[1][kc] = a + b;
                    tt[2][kc] = a - b;
                } else {                               // z = patch rows 1..5: y3/y4 = (z3 - z1) +- 2(z2 - z0), y5 = 4z0 - 5z2 + z4
                    const f32x2 c = x[3] - x[1], d = x[2] - x[0];
                    tt[0][kc] = fma2(2.f, d, c);
                    tt[1][kc] = fma2(-2.f, d, c);
                    tt[2][kc] = fma2(4.f, x[0], fma2(-5.f, x[2], x[4]));
                }
            }
            if (APZH_HALO_DPP == 2) {
                // The row pass works on columns, and a tile's halo columns ARE columns of its neighbours: column -1 = column 3 of
                // the tile to the left (its pair 1, element 1), column 4 = column 0 of the tile to the right (pair 0, element 0), and
                // the four tile columns of a tile row are the four lanes of a quad -- so the halo pair of every row-pass result
                // comes from the neighbouring lanes' results (quad_perm [0,0,1,2] / [1,2,3,3]; the same operations on the same
                // words: the same bits) instead of from a row pass of its own: 6 moves instead of 10 moves, 10 selects and 5 - 6
                // packed operations per chunk.  Border lanes: the left one is zeroed by its coefficient in col_pass (c4l), the
                // right one by a mask here.  (scalar copies first: hipcc 7.2 takes element 0 when __builtin_bit_cast is applied to
                // a vector element directly)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float c3 = tt[j][1][1], c0 = tt[j][0][0];
                    const int l = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c3), 0x90, 0xF, 0xF, true);
                    const int r = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c0), 0xF9, 0xF, 0xF, true);
                    tt[j][2] = f32x2{__builtin_bit_cast(float, l), __builtin_bit_cast(float, (unsigned)r & col16_mask)};
                }
            }
        };
        // B^T over the columns of one row: v = (v1, v2), (v3, v4), (v0, v5) -> o[0..5]
        auto col_pass = [&](const f32x2* t, float* o) {
            const f32x2 ab = fma2(-4.f, t[0], t[1]);   // (b, a) = (v3 - 4 v1, v4 - 4 v2)
            const f32x2 dc = t[1] - t[0];              // (d, c) = (v3 - v1, v4 - v2)
            o[0] = __builtin_fmaf(APZH_HALO_DPP == 2 ? c4l : 4.f, t[2][0], __builtin_fmaf(-5.f, t[0][1], t[1][1]));
            o[3] = __builtin_fmaf(2.f, dc[0], dc[1]);
            o[1] = ab[1] + ab[0];
            o[4] = __builtin_fmaf(-2.f, dc[0], dc[1]);
            o[2] = ab[1] - ab[0];
            o[5] = __builtin_fmaf(4.f, t[0][0], __builtin_fmaf(-5.f, t[1][0], t[2][1]));
        };
        // The six values of a row: lanes of the even channel keep o[0..2] and hand o[3..5] to their pair partner (16 lanes
        // up), lanes of the odd channel the other way round.  v_permlane16_swap_b32 a, b swaps a's odd 16-lane rows with b's
        // even ones: afterwards (o[k], o[k + 3]) is (even channel's value, odd channel's value) of position k in the even
        // channel's lanes and of position k + 3 in the odd channel's -- one instruction per value pair where DPP needed two
        // selects and a move.  (gfx950 wants two wait states between a vector write of an operand and the swap: s_nop 1.)
        auto exchange = [&](float* o) {
            asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %3\n\tv_permlane16_swap_b32 %1, %4\n\tv_permlane16_swap_b32 %2, %5"
                : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]));
        };
        // (even channel's value, odd channel's value) of one position -> its hi and lo words in V
        auto emit = [&](char* vp, float ev, float od) {
            unsigned hu, lu;
            f16x2_split(ev, od, hu, lu);
            *reinterpret_cast<unsigned*>(vp) = hu;
            *reinterpret_cast<unsigned*>(vp + T::VTERM) = lu;
        };
#ifndef APZH_EMIT2
#define APZH_EMIT2 0
#endif
        // (APZH_EMIT2) two positions at once: f16x2_split's two v_fma_mixlo / v_fma_mixhi pairs interleaved in ONE asm statement, so that no wait state is needed between a
        // register's low-half write and its high-half write
        auto emit2 = [&](char* vp0, float ev0, float od0, char* vp1, float ev1, float od1) {
            typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
            const f16x2_ h0 = {(_Float16)ev0, (_Float16)od0}, h1 = {(_Float16)ev1, (_Float16)od1};
            const unsigned hu0 = __builtin_bit_cast(unsigned, h0), hu1 = __builtin_bit_cast(unsigned, h1);
            unsigned lu0, lu1;
            asm("v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
                "v_fma_mixlo_f16 %1, %3, -1.0, %5 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
                "v_fma_mixhi_f16 %0, %2, -1.0, %6 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
                "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                : "=&v"(lu0), "=&v"(lu1) : "v"(hu0), "v"(hu1), "v"(ev0), "v"(ev1), "v"(od0), "v"(od1));
            *reinterpret_cast<unsigned*>(vp0) = hu0;
            *reinterpret_cast<unsigned*>(vp0 + T::VTERM) = lu0;
            *reinterpret_cast<unsigned*>(vp1) = hu1;
            *reinterpret_cast<unsigned*>(vp1 + T::VTERM) = lu1;
        };
        // The transform of one chunk (raw[rpar] -> V[vpar], this thread's channel, rows 3 ph .. 3 ph + 2) in 18 slices, two
        // per MFMA slot of a chunk body
        auto tslice = [&](int rpar, int vpar, auto KK) {
            constexpr int K = decltype(KK)::value;
            const float* rp = rawb + rpar * T::RAW_FLOATS + tr_off;
            char* vp = vbase + vpar * T::V_BYTES + tv_off;
            if constexpr (K == 0) row_load(rp);
            else if constexpr (K == 2) row_pass();
            else if constexpr (K >= 3 && K < 18) {
                constexpr int ii = (K - 3) / 5, part = (K - 3) % 5;
                if constexpr (part == 0) col_pass(tt[ii], oo);
                else if constexpr (part == 1) exchange(oo);
                else if (APZH_EMIT2) {
                    if constexpr (part == 2)
                        emit2(vp + ((3 * ph + ii) * 6 + 0) * T::VPOS, oo[0], oo[3], vp + ((3 * ph + ii) * 6 + 1) * T::VPOS, oo[1], oo[4]);
                    else if constexpr (part == 3)
                        emit(vp + ((3 * ph + ii) * 6 + 2) * T::VPOS, oo[2], oo[5]);
                } else {
                    constexpr int k = part - 2;
                    emit(vp + ((3 * ph + ii) * 6 + k) * T::VPOS, oo[k], oo[k + 3]);
                }
            }
        };
#define APZH_ALL18(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16) F(17)
        auto transform = [&](int rpar, int vpar) {
#define APZH_TS(k) tslice(rpar, vpar, std::integral_constant<int, k>{});
            APZH_ALL18(APZH_TS)
#undef APZH_TS
        };

        // zero halo rows of both raw buffers (the DMA never touches them), once
        for (int i = tid * 4; i < 2 * T::RAW_FLOATS; i += 2048) *reinterpret_cast<f32x4*>(&lds[i]) = f32x4{0.f, 0.f, 0.f, 0.f};
        // the first RING - 1 weight units (the first chunk body takes its base from ub_nxt)
        ub_cur = ub_nxt = unit_base(0, 0);
#pragma unroll
        for (int u = 0; u < RING - 1; u++) unit_load(u, u);
        __syncthreads();
        raw_dma(0, 0, 0);                              // the first item's first two chunks (later items: from the epilogue before)
        raw_dma(0, 1, 1);

        for (int t = 0; t < nitems; t++) {
            const int h = items.half(t);
            const int bd0 = 2 * items.pair(t);
            const bool two = bd0 + 1 < n;
            // ---- item prologue: raw(0), raw(1) have been requested; V[0] = transform(raw(0))
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            APZH_STAMP(5)
            transform(0, 0);
            f32x16h acc[9];
#pragma unroll
            for (int p = 0; p < 9; p++)
#pragma unroll
                for (int v = 0; v < 16; v++) acc[p][v] = 0.f;
            APZH_STAMP(0)

            // ---- chunk loop.  Iteration c: [barrier] DMA of raw(c+2) -> raw[c & 1] (read last by the transform of iteration
            // c - 1); transform of raw[(c+1) & 1] -> V[(c+1) & 1]; MFMAs over V[c & 1]: 9 slots = the wave's 9 positions,
            // each slot 2 MFMAs + two slices of the transform + the refill of the weight ring slot freed by the previous slot.
            // (measurement builds of tools/wino3h_bench.hip: the chunk body without its transform / weight loads / fragment reads)
#ifndef APZH_ABL_T
#define APZH_ABL_T 0
#endif
#ifndef APZH_ABL_W
#define APZH_ABL_W 0
#endif
#ifndef APZH_ABL_D
#define APZH_ABL_D 0      /* no LDS-DMA of the next chunks' planes inside the chunk loop (stale tiles: timing only) */
#endif
#ifndef APZH_ABL_B
#define APZH_ABL_B 0
#endif
#ifndef APZH_ABL_M
#define APZH_ABL_M 0      /* no MFMAs in the chunk loop */
#endif
#ifndef APZH_ABL_S
#define APZH_ABL_S 0      /* no barrier at the top of a chunk (races: timing only) */
#endif
#if APZH_ABL_M
#define APZH_MFMA_NONE(a_, b_, c_) asm volatile("" ::"v"(a_), "v"(b_))
#endif
#if APZH_ABL_W == 3           /* the weight ring keeps streaming, the MFMAs read one fixed unit: no per-slot wait for a load */
#define APZH_AF(slot_) af_fixed
#define APZH_AF_KEEP(slot_) af_keep(slot_);
#else
#define APZH_AF(slot_) af[slot_]
#define APZH_AF_KEEP(slot_)
#endif
#define APZH_MFMA_REAL(a_, b_, c_) c_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_, b_, c_, 0, 0, 0)
#if APZH_ABL_M == 1
#define APZH_MFMA_LO APZH_MFMA_NONE
#define APZH_MFMA_HI APZH_MFMA_NONE
#elif APZH_ABL_M == 2         /* one MFMA per slot */
#define APZH_MFMA_LO APZH_MFMA_NONE
#define APZH_MFMA_HI APZH_MFMA_REAL
#else
#define APZH_MFMA_LO APZH_MFMA_REAL
#define APZH_MFMA_HI APZH_MFMA_REAL
#endif
#if APZH_ABL_T == 1
#define APZH_TSLICE(k)
#elif APZH_ABL_T == 2       /* the transform's work twice (same results): is there slack for vector instructions? */
#define APZH_TSLICE(k) tslice(1 - par, 1 - par, std::integral_constant<int, (k)>{}); tslice(1 - par, 1 - par, std::integral_constant<int, (k)>{});
#else
#define APZH_TSLICE(k) tslice(1 - par, 1 - par, std::integral_constant<int, (k)>{});
#endif
#if APZH_ABL_W == 1
#define APZH_ULOAD(k)
#else
#define APZH_ULOAD(k) unit_load((k) + RING - 1, (par * 9 + (k) + RING - 1) % RING);
#endif
#ifndef APZH_PRIO
#define APZH_PRIO 1
#endif
#if APZH_PRIO
            // the later-dispatched half of the workgroup (waves 4..7, the SIMD partners of 0..3) loses every issue
            // arbitration by age (MI355X_MICROARCH.md, "Two waves per SIMD", item 4): one static priority raise evens it out
            if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
            f16x8 bfr[2];
#if APZH_ABL_W == 3
            f16x8 af_fixed = af[0];
            asm volatile("" : "+v"(af_fixed));
#endif
            auto chunk = [&](int c, auto PAR) {
                constexpr int par = decltype(PAR)::value;
#ifndef APZH_ADDR_EARLY
#define APZH_ADDR_EARLY 0
#endif
                int le_early = 0;
                if (APZH_ADDR_EARLY) {                // the fragment offset in front of the barrier instead of behind it
                    le_early = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    asm volatile("" : "+v"(le_early));
                    le_early = wpos0 * T::VPOS + (le_early & 31) * 16;
                    asm volatile("" : "+v"(le_early));
                }
                if (!APZH_ABL_S) __syncthreads();     // V[par] and raw[1 - par] complete; V[1 - par] and raw[par] free
                APZH_STAMP(1)
                ub_cur = ub_nxt;                      // (chunk 0 of item 0: set in front of the loop)
                ub_nxt = c + 1 < T::NCHUNK ? ub_cur + 9u * T::UNIT : (t + 1 < nitems ? unit_base(t + 1, 0) : ub_cur + 9u * T::UNIT);
                const char* vp = vbase + par * T::V_BYTES;
                // per-lane fragment offset rebuilt from an opaque copy of the lane id (kept live across the kernel it is
                // what hipcc spills, and every scratch reload is followed by vmcnt(0): a full drain of the weight ring)
                int le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                asm volatile("" : "+v"(le));
                const int b_hi = APZH_ADDR_EARLY ? le_early : wpos0 * T::VPOS + (le & 31) * 16;   // B = [Vhi | Vhi]
                const int b_lo = b_hi + T::VTERM;                                    // B = [Vlo | Vlo]
#ifndef APZH_BDEDUP
#define APZH_BDEDUP 0
#endif
#if APZH_BDEDUP
                // ONE read per position: lanes 0-31 fetch the lo term, lanes 32-63 the hi term; the two fragments [Vlo | Vlo] and
                // [Vhi | Vhi] are made in registers (v_permlane32_swap_b32: lanes 32-63 of the first operand <-> lanes 0-31 of the second)
                const int b_mix = b_hi + ((le & 32) ? 0 : T::VTERM);
                u32x4 bmix = *reinterpret_cast<const u32x4*>(vp + b_mix);
                auto bsplit = [&]() {
                    u32x4 lo4 = bmix, hi4 = bmix;
                    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %1, %5\n\t"
                                 "v_permlane32_swap_b32 %2, %6\n\tv_permlane32_swap_b32 %3, %7\n\ts_nop 1"
                                 : "+v"(lo4[0]), "+v"(lo4[1]), "+v"(lo4[2]), "+v"(lo4[3]), "+v"(hi4[0]), "+v"(hi4[1]), "+v"(hi4[2]), "+v"(hi4[3]));
                    bfr[1] = __builtin_bit_cast(f16x8, lo4);
                    bfr[0] = __builtin_bit_cast(f16x8, hi4);
                };
                bsplit();
#else
                bfr[0] = *reinterpret_cast<const f16x8*>(vp + b_hi);
                bfr[1] = *reinterpret_cast<const f16x8*>(vp + b_lo);
#endif
#if APZH_BDEDUP
#define APZH_BREAD_LO(p9)
#define APZH_BREAD_HI(p9) if (p9 + 1 < 9 && !APZH_ABL_B) bmix = *reinterpret_cast<const u32x4*>(vp + b_mix + pos_off(p9 + 1));
#define APZH_BSPLIT(p9) if (p9 + 1 < 9 && !APZH_ABL_B) bsplit();
#else
#define APZH_BREAD_LO(p9) if (p9 + 1 < 9 && !APZH_ABL_B) bfr[1] = *reinterpret_cast<const f16x8*>(vp + b_lo + pos_off(p9 + 1));
#define APZH_BREAD_HI(p9) if (p9 + 1 < 9 && !APZH_ABL_B) bfr[0] = *reinterpret_cast<const f16x8*>(vp + b_hi + pos_off(p9 + 1));
#define APZH_BSPLIT(p9)
#endif
#define APZH_SLOT(k)                                                                                                     \
                {                                                                                                        \
                    constexpr int p9 = (k), slot = (par * 9 + (k)) % RING;                                               \
                    /* the small products first: (Whi + Wlo) . Vlo, then (Whi + Wlo) . Vhi; every V fragment is re-read   \
                       for the next position right behind the MFMA that uses it */                                        \
                    APZH_MFMA_LO(APZH_AF(slot), bfr[1], acc[p9]);                                                        \
                    APZH_BREAD_LO(p9)                                                                                    \
                    APZH_MFMA_HI(APZH_AF(slot), bfr[0], acc[p9]);                                                        \
                    APZH_BREAD_HI(p9)                                                                                    \
                    if ((k) == 1 && !APZH_ABL_D) raw_dma(t, c + 2, par);                                                 \
                    APZH_TSLICE(2 * (k))                                                                                 \
                    APZH_TSLICE(2 * (k) + 1)                                                                             \
                    /* unit k + RING - 1 goes into the ring slot of unit k - 1, whose MFMAs are done */                 \
                    APZH_ULOAD(k)                                                                                        \
                    APZH_BSPLIT(p9)                                                                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                   \
                }
                APZH_SLOT(0) APZH_SLOT(1) APZH_SLOT(2) APZH_SLOT(3) APZH_SLOT(4) APZH_SLOT(5) APZH_SLOT(6) APZH_SLOT(7) APZH_SLOT(8)
#undef APZH_SLOT
#undef APZH_BREAD_LO
#undef APZH_BREAD_HI
#undef APZH_BSPLIT
                APZH_AF_KEEP(0) APZH_AF_KEEP(1) APZH_AF_KEEP(2) APZH_AF_KEEP(3) APZH_AF_KEEP(4) APZH_AF_KEEP(5)
                APZH_STAMP(2)
            };
            for (int c = 0; c < T::NCHUNK; c += 2) {
                chunk(c, std::integral_constant<int, 0>{});
                chunk(c + 1, std::integral_constant<int, 1>{});
            }

            // ---- epilogue: four steps of 16 output channels = channels 8 s .. 8 s + 7 of BOTH 32-channel halves, so that
            // all eight waves move accumulators in every step (a step of one half left four waves idle while the other four
            // wrote 72 values each: profiles/r06_wino3h.md).  Layout of the 32 x 32 tile: lane (col = lane & 31, hh =
            // lane >> 5), register v: channel (v & 3) + 8 (v >> 2) + 4 hh -- registers 4 s .. 4 s + 3 are channels 8 s +
            // (0..3) + 4 hh.  M row (of 16) = 8 cc + channel - 8 s.
            const int cosel = lane >> 5;               // gather role: M row 2 wave + cosel of the step's 16, column lane & 31
            const int col = lane & 31, gbd = col >> 4, gtile = col & 15;
            const int gty = gtile >> 2, gtx = gtile & 3;
            float* sw = stg + wave * (4 * T::SPLANE);
            const int s_lin = (lane >> 2) * T::SROW + (lane & 3) * 4;
            const unsigned ep_vo = lane < 60 ? lane * 16 : 0x80000000u;
            // output channel of M row `row` in step s
            auto row_chan = [&](int s, int row) { return (2 * h + (row >> 3)) * 32 + 8 * s + (row & 7); };
            // residual planes of this wave (its 2 M rows x 2 boards), requested a step ahead of their use
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
                APZH_STAMP(4)
                if (s == 0 && t + 1 < nitems) {        // the raw tiles are free: the next item's first two chunks
                    raw_dma(t + 1, 0, 0);
                    raw_dma(t + 1, 1, 1);
                }
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
                APZH_STAMP(8)
                __syncthreads();                       // M complete
                APZH_STAMP(10)
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
                    // the next step's residual planes: behind the gather (their registers are free now), in front of this
                    // step's stores (vmcnt counts in issue order: the wait for them must not include those stores)
                    if (RESID && s + 1 < 4) resid_request(s + 1);
                    const int ch = row_chan(s, co16);
                    const float bv = bias[ch];
                    const float is = bias[128 + ch];                     // 1 / S of the channel (a power of two)
                    float* sp = sw + (cosel * 2 + gbd) * T::SPLANE + (4 * gty) * T::SROW + 4 * gtx;
                    f32x4 y[4];
#pragma unroll
                    for (int ee = 0; ee < 4; ee++) {
                        float o0, o1, o2, o3;
                        wino_out_row(hrow[0][ee], hrow[1][ee], hrow[2][ee], hrow[3][ee], hrow[4][ee], hrow[5][ee], o0, o1, o2, o3);
                        y[0][ee] = o0, y[1][ee] = o1, y[2][ee] = o2, y[3][ee] = o3;
                    }
#ifndef APZH_CHK4
#define APZH_CHK4 0      /* 1: the non-finite check on the four corner outputs of a tile only (see below) instead of all sixteen: 13 vector
                            instructions fewer per step, no measurable change (profiles/r06_wino3h_micro_ab.log: the epilogue waits on
                            barriers and LDS round trips, not on its vector instructions) -- so the plain form stays */
#endif
                    // Non-finite check.  y[a][e] sums M[i][k] over i in rows(a), k in rows(e) with rows(0) = 0..4, rows(1) = rows(2) =
                    // 1..4, rows(3) = 1..5 (the non-zero columns of A^T): the four corners y[0][0], y[0][3], y[3][0], y[3][3] together
                    // contain every one of the 36 M[i][k], and a NaN or an infinity in a sum stays non-finite -- so the corners'
                    // sum is non-finite whenever any accumulator of the tile is (3 additions per step instead of 16).
                    float chk = APZH_CHK4 ? (y[0][0] + y[0][3]) + (y[3][0] + y[3][3]) : 0.f;
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        f32x4 v;
#pragma unroll
                        for (int ee = 0; ee < 4; ee++) v[ee] = __builtin_fmaf(y[a][ee], is, bv);
                        if (RESID) v += *reinterpret_cast<const f32x4*>(sp + a * T::SROW);   // (wave-private: written above by this wave)
                        if (!APZH_CHK4) chk += wino_sum4(v);
#pragma unroll
                        for (int ee = 0; ee < 4; ee++) v[ee] = RELU ? fmaxf(v[ee], 0.f) : v[ee];
                        if (gtx == 3) v[3] = 0.f;      // column 15 is the halo column of the rows16 layout
                        *reinterpret_cast<f32x4*>(sp + a * T::SROW) = v;   // (same lane, same addresses as the residual it read)
                    }
                    nonfinite |= wino_nonfinite(chk) ? 1u : 0u;
                }
                APZH_STAMP(9)
                wave_lds_fence();
#pragma unroll
                for (int pl = 0; pl < 4; pl++) {
                    const f32x4 pv = *reinterpret_cast<const f32x4*>(sw + pl * T::SPLANE + s_lin);
                    const unsigned vo = ((pl & 1) == 0 || two) ? ep_vo : 0x80000000u;   // the missing second board of an odd batch
#if defined(APZH_ABL_ST) && APZH_ABL_ST     /* measurement build: no output stores (how much of the epilogue is the HBM burst?) */
                    asm volatile("" ::"v"(pv), "v"(vo));
#else
                    bstore(r_out, vo, (unsigned)((bd0 + (pl & 1)) * T::C + row_chan(s, 2 * wave + (pl >> 1))) * plane_b, pv);
#endif
                }
                APZH_STAMP(3)
            };
            ep_step(std::integral_constant<int, 0>{});
            ep_step(std::integral_constant<int, 1>{});
            ep_step(std::integral_constant<int, 2>{});
            ep_step(std::integral_constant<int, 3>{});
            // (the next item's prologue starts with a barrier: M / staging are consumed before its transform writes V)
        }
    };
    if (((wave >> 1) & 1) == 0)
        run(std::integral_constant<int, 0>{});
    else
        run(std::integral_constant<int, 1>{});
    // (a plain store: every writer writes the same 1, and the word may live in pinned host memory)
    if (nonfinite && flag) *reinterpret_cast<volatile unsigned*>(flag) = 1u;
#ifdef APZ_WINO3H_STAMPS
    st_acc[7] = __builtin_readcyclecounter() - st_t0;
    st_acc[6] = __builtin_amdgcn_s_memrealtime() - st_r0;
    if (lane == 0 && blockIdx.x < 4)
        for (int i = 0; i < 12; i++) apz_wino3h_stamps[(blockIdx.x * 8 + wave) * 12 + i] = st_acc[i];
#endif
}

}  // namespace apz
