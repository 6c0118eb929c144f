// Shared pieces of the Winograd F(4x4,3x3) trunk kernels (trunk15_wino3*.h, wgrad_wino3*.h) for gfx950: vector types, the
// packed FMA, the wavefront-scope LDS fence, the packed-weight geometry, the work-item schedule of the batched kernels, the
// raw-buffer helpers for rows16 activations, the output transform's row formula and the epilogue tail of the split-operand
// kernels.  What belongs to the fp16 two-term split alone is in wino_f16x2.h.
#pragma once
#include <hip/hip_runtime.h>

#include "conv3x3_mfma.h"

namespace apz {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Transformed weights U = G g G^T of one 128 -> 128 layer, packed per MFMA A fragment:
// [cot 8][row half 2][c4 32][lane 64][20] -- lane (q = lane>>4, j = lane&15) holds U[row 3*half + ii][k] at index
// 6*ii + k of co = cot*16 + j, ci = c4*4 + q (18 values + 2 pad: four 16-byte loads + one 8-byte load per k-step).
struct WinoPack {
    static constexpr int UROW = 20;                    // floats per lane and k-step
    static constexpr size_t UPK_FLOATS = (size_t)8 * 2 * 32 * 64 * UROW;   // per layer (2.6 MB)
};

// The same values for the small-batch kernel (trunk15_wino3s.h), whose MFMA wave w owns positions 9 w .. 9 w + 8:
// [cot 8][w 4][c4 32][piece 3][lane 64][4] -- value m = 4 piece + e of the wave's nine (pad: 0), so that one k-step of a
// wave is three fully coalesced 1 KB loads (from the layout above it was nine loads touching forty 128-byte lines each).
struct WinoPackSmall {
    static constexpr int STEP = 3 * 64 * 4;            // floats per (cot, w, c4)
    static constexpr size_t UPK_FLOATS = (size_t)8 * 4 * 32 * STEP;   // per layer (3.1 MB)
    __host__ __device__ static size_t index(int co, int ci, int pos) {
        const int cot = co >> 4, jj = co & 15, c4 = ci >> 2, qq = ci & 3, w = pos / 9, m = pos % 9;
        return ((((size_t)(cot * 4 + w) * 32 + c4) * 3 + (m >> 2)) * 64 + (qq * 16 + jj)) * 4 + (m & 3);
    }
};

__device__ __forceinline__ f32x2 fma2(const float a, const f32x2 b, const f32x2 c) {   // a*b + c (v_pk_fma_f32)
    return __builtin_elementwise_fma(f32x2{a, a}, b, c);
}

// ---- Work items of the batched trunk kernels with two channel halves per board pair (trunk15_wino3b.h, _wino3h.h,
// _wino3h16.h; trunk15_wino3.h restates the mapping because its QUARTER form has four parts).  An item = (board pair,
// channel half).  Grids that are a multiple of 16 run in "duo" mode: two workgroups that the dispatcher (observed: round-
// robin over the 8 XCDs) places on the same XCD take the two channel halves of the SAME pairs at the same time, so that the
// second read of a pair's input planes is an L2 hit instead of a second trip over the fabric.  Placement changes only
// speed: any other grid (and any other placement) computes the same thing.
//   duo:   block b -> XCD group c = b % 8, i = b / 8; duo d = (i / 2) * 8 + c takes pairs d, d + G / 2, ...; half i & 1.
//   plain: block b takes pairs b, b + G, ... and both halves of each.
// Built from (n, gridDim.x, blockIdx.x).
struct WinoItems {
    bool duo;
    int pair0, pstride, h_fix;
    int np;                                            // board pairs of this workgroup (0: nothing to do, return before any barrier)
    int nitems;
    __device__ __forceinline__ WinoItems(int n, int G_, int b_) {
        const int npairs = (n + 1) >> 1;
        duo = (G_ & 15) == 0;
        pair0 = duo ? ((b_ >> 4) * 8 + (b_ & 7)) : b_;
        pstride = duo ? (G_ >> 1) : G_;
        h_fix = (b_ >> 3) & 1;                         // duo mode: this workgroup's channel half
        np = pair0 < npairs ? (npairs - pair0 + pstride - 1) / pstride : 0;
        nitems = duo ? np : 2 * np;
    }
    __device__ __forceinline__ int pair(int t) const { return pair0 + (duo ? t : (t >> 1)) * pstride; }
    __device__ __forceinline__ int half(int t) const { return duo ? h_fix : (t & 1); }
};

// ---- Global memory through raw buffer instructions: descriptor (SGPRs) + per-lane 32-bit offset + wave-uniform SGPR
// offset.  No 64-bit per-lane addresses (registers, VALU), and lanes that must not take part (60..63 of a 960-byte plane) get
// an offset beyond the buffer (0x80000000): their loads return 0, their stores are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wino_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
// bytes of n boards of rows16 activations [n][128][15][16] (launchers keep this below 2^31)
__device__ __forceinline__ unsigned rows16_bytes(int n) { return (unsigned)n * 128 * (240 * 4); }
__device__ __forceinline__ f32x4 bload(const __amdgpu_buffer_rsrc_t& r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
// Stores keep soffset = 0 and add the uniform part into the per-lane offset.  With an SGPR soffset hipcc (ROCm 7.2)
// emits no wait state between a 128-bit buffer store and a VALU write of its data registers (LLVM's hazard
// recognizer exempts that form), and on gfx950 the store then picks up the NEW value of the last dword in some
// lanes (found the hard way: one element per 4x4 tile of every 16th channel wrong, and only in some builds).
__device__ __forceinline__ void bstore(const __amdgpu_buffer_rsrc_t& r, unsigned voff, unsigned soff, const f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff + soff, 0, 0);
}

// ---- Output transform A^T of one row of six: o0 = m0+m1+m2+m3+m4, o1 = (m1-m2) + 2(m3-m4), o2 = (m1+m2) + 4(m3+m4),
// o3 = (m1-m2) + 8(m3-m4) + m5.  Y = A^T M A applies it to the six rows of M (k direction) and then, per column, to the six
// row results (each column's six through the same function).  The order of the additions is part of the kernels' bit
// contract.
__device__ __forceinline__ void wino_out_row(float m0, float m1, float m2, float m3, float m4, float m5, float& o0, float& o1,
                                             float& o2, float& o3) {
    const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
    o0 = (m0 + s12) + s34;
    o1 = __builtin_fmaf(2.f, d34, d12);
    o2 = __builtin_fmaf(4.f, s34, s12);
    o3 = __builtin_fmaf(8.f, d34, d12) + m5;
}

// ---- The non-finite check of the split-operand kernels' epilogue: chk gathers wino_sum4 of the PRE-ReLU rows of a tile (a NaN
// would otherwise be clamped to 0 silently); an overflow of the split shows as +-inf / NaN there and wino_nonfinite(chk) is
// true.  (The rest of the tail -- v = fma(y, 1 / S, bias), the residual, the ReLU, the zero of column 15 -- stays in the
// kernels: moved into functions, each of these changed the instruction schedule of trunk15_wino3h16_kernel or
// trunk15_wino3hs_kernel.)
__device__ __forceinline__ float wino_sum4(const f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ bool wino_nonfinite(float chk) { return (chk - chk) != 0.f; }   // 0 for every finite sum; NaN != 0 is true

// ---- The sum over the 16 lanes of a DPP row (STATS forms: the 16 tiles of a board), a fixed tree of DPP adds
template <int CTRL>
__device__ __forceinline__ float wino3_dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wino3_row16_sum(float v) {
    v = wino3_dpp_add<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v = wino3_dpp_add<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v = wino3_dpp_add<0x141>(v);      // row_half_mirror: the other quad of the 8
    return wino3_dpp_add<0x140>(v);   // row_mirror: the other 8 of the 16
}

// Lanes of ONE wave exchange data through LDS (write in one layout, read in another).  The LDS executes a
// wave's instructions in order, so no s_barrier is needed -- but the compiler reasons per thread and may move
// a lane's read above its own (provably different-address) write.  This pins the order for the compiler.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace apz
