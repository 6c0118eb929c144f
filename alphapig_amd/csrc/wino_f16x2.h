// Shared pieces of the kernels that run fp32 products on the fp16 matrix pipe with two-term operands (x = hi + lo, both
// rounded to nearest even): trunk15_wino3h.h, trunk15_wino3h16.h, trunk15_wino3hs.h, conv8_split.h, wgrad_wino3h.h and the
// packers of their weights.  gfx950 only.  One copy each of: the channel scale and the host-side split and packer, the power-
// of-two pair of a scale exponent, the device-side split, and the input transform on column pairs of trunk15_wino3h16.h and
// its small-batch twin trunk15_wino3hs.h -- whose bit contract rests on the two running the same operations.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "wino_common.h"

namespace apz {

typedef float f32x16h __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- weights: the channel scale, the split, the host packer

// the power of two that puts m = max |U| of an output channel into [2^13, 2^14) (m == 0: 1)
__host__ __device__ inline float f16x2_scale_for(double m) {
    if (!(m > 0.0)) return 1.f;
    int e;
    frexp(m, &e);                                                  // m = f 2^e, f in [0.5, 1)
    int k = 14 - e;
    k = k < -100 ? -100 : (k > 100 ? 100 : k);
    return (float)ldexp(1.0, k);
}

// x -> the bits of hi = fp16(x) and lo = fp16(x - hi), the remainder formed in double
__host__ __device__ inline void f16x2_split(double x, unsigned short& hb, unsigned short& lb) {
    const _Float16 hi = (_Float16)(float)x;
    const _Float16 lo = (_Float16)(float)(x - (double)(float)hi);
    hb = __builtin_bit_cast(unsigned short, hi);
    lb = __builtin_bit_cast(unsigned short, lo);
}

// Host packing: U[pos][co][ci] (double) -> a trunk kernel's fp16 x 2 layout + the per-channel inverse scales.
// `u_of(co, ci, pos)` returns the value.  inv_scale: 128 floats (goes behind the 128 biases).  L: the layout (Wino3H of
// trunk15_wino3h.h or Wino3H16 of trunk15_wino3h16.h: the same terms and scales, another order).
template <class L, class F>
inline void wino3h_pack_host(F u_of, std::vector<uint16_t>& out, float* inv_scale) {
    out.assign(L::UPK_BYTES / 2, 0);
    for (int co = 0; co < 128; co++) {
        double m = 0;
        for (int ci = 0; ci < 128; ci++)
            for (int pos = 0; pos < 36; pos++) m = std::max(m, std::fabs((double)u_of(co, ci, pos)));
        const float S = f16x2_scale_for(m);
        inv_scale[co] = 1.f / S;
        for (int ci = 0; ci < 128; ci++)
            for (int pos = 0; pos < 36; pos++)
                f16x2_split((double)u_of(co, ci, pos) * (double)S, out[L::upk_offset(co, ci, pos, 0) / 2],
                            out[L::upk_offset(co, ci, pos, 1) / 2]);
    }
}

// ---- activations

// 2^a and 2^-a (normal floats for |a| <= 126): an input scale and what undoes it, both exact
__device__ __forceinline__ void f16x2_pow2_pair(int a, float& p, float& ip) {
    p = __builtin_bit_cast(float, (unsigned)(127 + a) << 23);
    ip = __builtin_bit_cast(float, (unsigned)(127 - a) << 23);
}

// The lo word of a split pair: hu = the packed fp16 (ev, od); returns the packed fp16 of the remainders ev - hi, od - hi,
// which v_fma_mix forms exactly in fp32 before it rounds.
__device__ __forceinline__ unsigned f16x2_split_lo(unsigned hu, float ev, float od) {
    unsigned lu;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lu) : "v"(hu), "v"(ev));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu) : "v"(hu), "v"(od));
    return lu;
}
// (ev, od) -- in the trunk kernels the even and the odd channel's value of one position -> hu = both rounded to fp16
// (v_cvt_pk_f16_f32), lu = the remainders.  Where the words go is the caller's business: the V layouts differ.
__device__ __forceinline__ void f16x2_split(float ev, float od, unsigned& hu, unsigned& lu) {
    typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
    const f16x2_ h2 = {(_Float16)ev, (_Float16)od};
    hu = __builtin_bit_cast(unsigned, h2);
    lu = f16x2_split_lo(hu, ev, od);
}

// ---- Input transform V = B^T d B of trunk15_wino3h16_kernel and trunk15_wino3hs_kernel, one 6 x 6 patch per lane.
// Lane roles: tile = lane bits 0-3 (tile column ttx = bits 0-1, tile row tty = bits 2-3), channel pair = bit 4, channel
// parity = bit 5.  So a board's 16 tiles are one 16-lane DPP row (the halo rows come from row_shr / row_shl by 4 lanes), the
// tile columns of a tile row are a quad (the halo columns: quad_perm), and the two channels of a pair sit 32 lanes apart
// (v_permlane32_swap_b32 exchanges them).  raw[r] = row r of the lane's own 4 x 4 tile.

// B^T over the rows of the patch (x0 = row -1 .. x5 = row 4), on the column pair kc (0: columns 0, 1; 1: columns 2, 3):
// tt[0..5][kc].  Rows -1 and 4 are row 3 of the tile above and row 0 of the tile below (zero beyond the board: bound_ctrl).
__device__ __forceinline__ void f16x2_vpass(const f32x4 (&raw)[4], int kc, f32x2 (&tt)[6][2]) {
    f32x2 x[6];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const float r3 = raw[3][2 * kc + j], r0 = raw[0][2 * kc + j];
        x[0][j] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r3), 0x114, 0xF, 0xF, true));   // row_shr:4
        x[5][j] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r0), 0x104, 0xF, 0xF, true));   // row_shl:4
    }
#pragma unroll
    for (int r = 0; r < 4; r++) x[r + 1] = f32x2{raw[r][2 * kc], raw[r][2 * kc + 1]};
    const f32x2 a = fma2(-4.f, x[2], x[4]), b = fma2(-4.f, x[1], x[3]);
    const f32x2 c = x[4] - x[2], d = x[3] - x[1];
    tt[0][kc] = fma2(4.f, x[0], fma2(-5.f, x[2], x[4]));
    tt[1][kc] = a + b;
    tt[2][kc] = a - b;
    tt[3][kc] = fma2(2.f, d, c);
    tt[4][kc] = fma2(-2.f, d, c);
    tt[5][kc] = fma2(4.f, x[1], fma2(-5.f, x[3], x[5]));
}
// B^T over the columns of row j: the halo columns (-1 and 4) are the quad neighbours' columns 3 and 0 of the same row
// (quad_perm [0,0,1,2] / [1,2,3,3]); v = (v1, v2), (v3, v4), (v0, v5) -> oo[0..5].  The borders of the board: c4l = 0 instead
// of 4 in the first tile column (column -1 is the zero border, as the coefficient its only use carries), col16_mask = 0
// instead of all ones in the last (column 16 does not exist).
__device__ __forceinline__ void f16x2_col_pass(const f32x2 (&tt)[6][2], int j, float c4l, unsigned col16_mask, float (&oo)[6]) {
    const float c3 = tt[j][1][1], c0 = tt[j][0][0];
    const int l = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c3), 0x90, 0xF, 0xF, true);
    const int r = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, c0), 0xF9, 0xF, 0xF, true);
    const float v0 = __builtin_bit_cast(float, l), v5 = __builtin_bit_cast(float, (unsigned)r & col16_mask);
    const f32x2 ab = fma2(-4.f, tt[j][0], tt[j][1]);   // (b, a) = (v3 - 4 v1, v4 - 4 v2)
    const f32x2 dc = tt[j][1] - tt[j][0];              // (d, c) = (v3 - v1, v4 - v2)
    oo[0] = __builtin_fmaf(c4l, v0, __builtin_fmaf(-5.f, tt[j][0][1], tt[j][1][1]));
    oo[3] = __builtin_fmaf(2.f, dc[0], dc[1]);
    oo[1] = ab[1] + ab[0];
    oo[4] = __builtin_fmaf(-2.f, dc[0], dc[1]);
    oo[2] = ab[1] - ab[0];
    oo[5] = __builtin_fmaf(4.f, tt[j][0][0], __builtin_fmaf(-5.f, tt[j][1][0], v5));
}
// Lanes of the even channel keep oo[0..2] and hand oo[3..5] to their pair partner (32 lanes up), lanes of the odd channel
// the other way round: afterwards (oo[k], oo[k + 3]) = (even channel's value, odd channel's value) of position k in the even
// channel's lanes and of position k + 3 in the odd channel's.  (two wait states after a vector write of an operand)
__device__ __forceinline__ void f16x2_exchange(float (&oo)[6]) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %3\n\tv_permlane32_swap_b32 %1, %4\n\tv_permlane32_swap_b32 %2, %5"
        : "+v"(oo[0]), "+v"(oo[1]), "+v"(oo[2]), "+v"(oo[3]), "+v"(oo[4]), "+v"(oo[5]));
}

}  // namespace apz
