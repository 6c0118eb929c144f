// Small-batch form of trunk15_wino3h16_kernel (trunk 3x3 convolution 128 -> 128 at 15x15 + folded BN (+ residual) + ReLU as
// a fused F(4x4,3x3) Winograd convolution on the fp16 matrix pipe with two-term operands) for 1 .. 32 boards.  gfx950 only.
//
// Why: with trunk_arith = f16x2 a batch of more than 32 boards runs trunk15_wino3h16_kernel and a smaller one the exact fp32
// trunk15_wino3s_kernel, so a position's low-order bits depend on how many boards share its forward.  This kernel gives the
// small batches the batched kernel's bits (apz_set_trunk_uniform); the batched kernel itself would put one board on two of
// the 256 CUs.
//
// SAME BITS as trunk15_wino3h16_kernel<RESID, true, WINO3H16_PLAIN / WINO3H16_PLAIN_SCALED> for every output element of every
// board.  SHARED with that kernel -- one function each, so this part of the contract holds by construction:
//   input transform  f16x2_pow2_pair (SCALED: raw *= 2^a), f16x2_vpass, f16x2_col_pass, f16x2_exchange, f16x2_split of
//                    wino_f16x2.h, with the same lane roles (a board's 16 tiles = one DPP row, the tile columns of a row = a
//                    quad, a channel pair 32 lanes apart);
//   output formulas  wino_out_row for the k direction of every row, wino_sum4 for a row of the check sum and
//                    wino_nonfinite for its test (wino_common.h).
// Still RESTATED here operation for operation, and held to the batched kernel by the bit-equality tests alone:
//   accumulation     per (position, 32 output channels): acc = 0, then for the chunks of 16 input channels in ascending
//                    order  mfma(H, Vlo), mfma(L, Vhi), mfma(H, Vhi)  with v_mfma_f32_32x32x16_f16, channels 0-7 of the
//                    chunk in lanes 0-31 and 8-15 in lanes 32-63.  A column of the 32 is (board, tile); a column's result
//                    does not depend on the others, so a lone board's 16 columns carry the batched kernel's values (the
//                    other 16 columns repeat them and are dropped).  The contraction is never split;
//   row halves       the rows combine as in trunk15_wino3s.h -- the lower half hands over (h0 + s12, d12, s12), the upper
//                    (s34, d34, h5), which are exactly the intermediates of wino_out_row over the six row results, and
//                    y[0..3] is finished from them;
//   tail             v = fma(y, 1 / S (2^-a), bias) + residual, ReLU, column 15 zeroed;
//   check tree       chk runs over the same 16 values of a (channel, tile), rows in the same order (row 15 included, its
//                    residual 0); the word is raised by a plain store.
// Same inputs: rows16 activations, the packed weights upk3h and bias3h of the batched kernel, the overflow word, the layer's
// static exponent.
//
// Work item = workgroup (board, 32 output channels cog, row half): 8 workgroups per board, 512 threads.  One item is one
// board: the 256 (channel, tile) units of a 16-channel chunk are half the workgroup, so a STEP is two chunks (wave parity =
// chunk of the step) and the K loop is four steps with one barrier each.  Per step every thread transforms the three rows
// of its half of one (channel, tile) patch into V[step & 1] while waves 0..5 = (row jj of the half, column block ki) run the
// 2 x 3 x 3 MFMAs of the step before.  Waves 6 and 7 run the same instruction stream on weights read out of range (zeros,
// no traffic) and write nothing: every global load stays unconditional and in ONE code path, so that the compiler's vmcnt
// bookkeeping is exact (trunk15_wino3s.h on what a load behind a wave-role branch costs).  Load distance: the raw tiles of a
// step are requested two steps (four chunks) ahead, a step's weights (12 units of 1 KB per wave) one step ahead.
//
// The two row halves of a (board, cog) meet through the in-launch reduction of trunk15_wino3s.h: 12 floats per (channel,
// tile) into a global slab, every wave drains its stores, one lane issues an agent-scope release and exchanges the launch's
// epoch into the pair's ticket word; the workgroup that gets the epoch back is second: agent-scope acquire, read the other
// slab, finish.  Slabs and words are this kernel's own.  Blocks b and b + 8 are the two halves (same XCD as dispatched
// today: speed only).
//
// Layouts.  V (LDS): [buffer 2][chunk of the step 2][pos 18][term 2 (hi, lo)][tile 16][half 2][8 ch] fp16, the channel half
// stored at half ^ (tile >> 3 & 1) as in trunk15_wino3h16.h.  M (over V buffer 0): [pos 18][co 32][tile 16] fp32.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "trunk15_wino3h16.h"
#include "trunk15_wino3s.h"

namespace apz {

struct Wino3HS {
    static constexpr int C = 128, CK = 16, NSTEP = 4;                  // a step = two chunks of 16 input channels
    static constexpr int GPLANE = 240;
    static constexpr int VTERM = 16 * 32, VPOS = 2 * VTERM, VKC = 18 * VPOS, V_BYTES = 2 * VKC;   // 512, 1024, 18432, 36864
    static constexpr int UNIT = Wino3H16::UNIT;
    static constexpr int M_FLOATS = 18 * 32 * 16;
    static constexpr int LDS_BYTES = 2 * V_BYTES + 16;                 // + the ticket flag
    static constexpr int SLAB_FLOATS = 12 * 512;                       // row partials of one (board, cog, half)
    static constexpr int MAX_BOARDS = Wino3S::MAX_BOARDS;
    static size_t slab_floats() { return (size_t)MAX_BOARDS * 4 * 2 * SLAB_FLOATS; }
    static size_t counters() { return (size_t)MAX_BOARDS * 4; }
    static int grid(int n) { return ((n + 1) >> 1) * 16; }
    static_assert(M_FLOATS * 4 <= V_BYTES, "M fits over one V buffer");
    static_assert(NSTEP * 2 * CK == C, "steps");
};

template <bool RESID, bool SCALED>
__global__ __launch_bounds__(512) void trunk15_wino3hs_kernel(const float* __restrict__ in, const void* __restrict__ upk,
                                                              const float* __restrict__ bias, const float* __restrict__ resid,
                                                              float* __restrict__ out, int n, unsigned* __restrict__ flag,
                                                              int act_exp, float* __restrict__ slabs,
                                                              unsigned* __restrict__ tickets, unsigned epoch) {
    using T = Wino3HS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* vbase = reinterpret_cast<char*>(lds);                           // [2][V_BYTES]
    float* mq = lds;                                                      // epilogue: M (over V buffer 0)
    unsigned* lflag = reinterpret_cast<unsigned*>(vbase + 2 * T::V_BYTES);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b_ = (int)blockIdx.x;
    const int bd = 2 * (b_ >> 4) + ((b_ >> 2) & 1), half = (b_ >> 3) & 1, cog = b_ & 3;
    if (bd >= n) return;                              // (uniform) the missing second board of an odd batch

    float xsc = 1.f, xisc = 1.f;
    if constexpr (SCALED) f16x2_pow2_pair(act_exp, xsc, xisc);   // the host's exponent: the same in every launch of the layer

    const unsigned plane_b = T::GPLANE * 4;
    const __amdgpu_buffer_rsrc_t r_in = wino_rsrc(in, rows16_bytes(n)), r_u = wino_rsrc(upk, (unsigned)Wino3H16::UPK_BYTES);

    // ---- transform role: trunk15_wino3h16_kernel's (lane roles: wino_f16x2.h), with the wave parity naming the chunk of the
    // step instead of the board
    const int kcw = wave & 1, cq = wave >> 1;
    const int ttx = lane & 3, tty = (lane >> 2) & 3, tile = lane & 15, cpl = (lane >> 4) & 1, e = lane >> 5;
    const int cpair = 2 * cq + cpl;                                // channel pair (0..7): V half cpair >> 2, dword cpair & 3
    const int tv_off = kcw * T::VKC + tile * 32 + (((cpair >> 2) ^ ((tile >> 3) & 1)) * 16) + (cpair & 3) * 4 + e * 3 * T::VPOS;
    const unsigned col16_mask = ttx == 3 ? 0u : 0xffffffffu;       // column 16 does not exist
    const float c4l = ttx == 0 ? 0.f : 4.f;                        // column -1 of the first tile column is the zero border
    const unsigned raw_vo = (unsigned)(2 * cpl + e) * plane_b + (unsigned)(tty * 4 * 16 + ttx * 4) * 4;
    const unsigned raw_vo3 = tty == 3 ? 0x80000000u : raw_vo + 3u * 64u;   // row 15 is out of range: the load returns zeros
    f32x4 rawr[2][4];                                              // ring: step & 1
    auto raw_load = [&](auto S_) {
        constexpr int s = decltype(S_)::value;
        const unsigned so = (unsigned)(bd * T::C + (2 * s) * T::CK + kcw * T::CK + 4 * cq) * plane_b;
#pragma unroll
        for (int r = 0; r < 3; r++) rawr[s & 1][r] = bload(r_in, raw_vo + (unsigned)r * 64u, so);
        rawr[s & 1][3] = bload(r_in, raw_vo3, so);
    };

    f32x2 tt[6][2];                                // vertical-pass results: rows 0..5, column pairs (0, 1), (2, 3)
    float oo[6];
    // (a one-line lambda, not a direct call: the compiler then simplifies it before it inlines it, which keeps the SCALED
    // kernels' instruction schedule)
    auto vpass = [&](const f32x4 (&raw)[4], int kc) { f16x2_vpass(raw, kc, tt); };
    // (even channel's value, odd channel's value) of one position -> its hi and lo words in V
    auto emit = [&](char* vp, float ev, float od) {
        unsigned hu, lu;
        f16x2_split(ev, od, hu, lu);
        *reinterpret_cast<unsigned*>(vp) = hu;
        *reinterpret_cast<unsigned*>(vp + T::VTERM) = lu;
    };
    auto trow = [&](char* vp, int j, int jj) {         // patch row j = row jj of this half
        f16x2_col_pass(tt, j, c4l, col16_mask, oo);
        f16x2_exchange(oo);
        emit(vp + (jj * 6 + 0) * T::VPOS, oo[0], oo[3]);
        emit(vp + (jj * 6 + 1) * T::VPOS, oo[1], oo[4]);
        emit(vp + (jj * 6 + 2) * T::VPOS, oo[2], oo[5]);
    };
    auto transform = [&](auto S_) {                    // raw of step s -> V[s & 1]
        constexpr int s = decltype(S_)::value;
        f32x4(&raw)[4] = rawr[s & 1];
        if constexpr (SCALED) {
#pragma unroll
            for (int r = 0; r < 4; r++) raw[r] *= xsc;      // exact: a power of two
        }
        vpass(raw, 0);
        vpass(raw, 1);
        char* vp = vbase + (s & 1) * T::V_BYTES + tv_off;
        if (half == 0) {
            trow(vp, 0, 0);
            trow(vp, 1, 1);
            trow(vp, 2, 2);
        } else {
            trow(vp, 3, 0);
            trow(vp, 4, 1);
            trow(vp, 5, 2);
        }
    };

    // ---- MFMA role: wave (jj, ki) = positions (row 3 half + jj, columns 3 ki .. 3 ki + 2) x the 32 output channels of cog.
    // A step's units of the wave: [chunk 2][position 3][H, L], 6 KB contiguous per chunk in upk's block 2 half + ki.
    const bool mfma_wave = wave < 6;
    const int jj = mfma_wave ? wave >> 1 : 2, ki = wave & 1;
    const unsigned a_vo = mfma_wave ? (unsigned)lane * 16u : 0x80000000u;   // a unit: lanes 0-31 channels 0-7, 32-63 channels 8-15
    const unsigned u_base = (unsigned)(((cog * 4 + 2 * half + ki) * Wino3H16::NCHUNK) * 18 + 6 * jj) * T::UNIT;
    f16x8 wr[2][12];                                   // ring: step & 1; [chunk of the step][position][H, L]
    auto unit_load = [&](auto S_) {
        constexpr int s = decltype(S_)::value;
#pragma unroll
        for (int kc = 0; kc < 2; kc++)
#pragma unroll
            for (int u = 0; u < 6; u++)
                wr[s & 1][kc * 6 + u] = __builtin_bit_cast(
                    f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_u, a_vo, u_base + (unsigned)((2 * s + kc) * 18 + u) * T::UNIT, 0));
    };
    f32x16h acc[3];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int v = 0; v < 16; v++) acc[p][v] = 0.f;
    // B fragment of a position: column = lane & 15 (lanes 16-31 repeat 0-15), channels 8 (lane >> 5) .. + 7: one ds_read_b128
    const int b_off = (jj * 6 + 3 * ki) * T::VPOS + (lane & 15) * 32 + ((((lane >> 5) & 1) ^ ((lane >> 3) & 1)) * 16);
    auto mfmas = [&](auto S_) {
        constexpr int s = decltype(S_)::value;
#pragma unroll
        for (int kc = 0; kc < 2; kc++) {               // chunks 2 s, 2 s + 1: ascending
            const char* vp = vbase + (s & 1) * T::V_BYTES + kc * T::VKC + b_off;
#pragma unroll
            for (int kk = 0; kk < 3; kk++) {
                const f16x8 bh = *reinterpret_cast<const f16x8*>(vp + kk * T::VPOS);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(vp + kk * T::VPOS + T::VTERM);
                const f16x8 ah = wr[s & 1][kc * 6 + 2 * kk], al = wr[s & 1][kc * 6 + 2 * kk + 1];
                acc[kk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[kk], 0, 0, 0);
                acc[kk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[kk], 0, 0, 0);
                acc[kk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[kk], 0, 0, 0);
            }
        }
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    raw_load(I0{});
    raw_load(I1{});
    unit_load(I0{});
    transform(I0{});
    raw_load(I2{});
    // step s: [barrier: V[s & 1] complete, V[(s + 1) & 1] free] weights of step s + 1, transform of step s + 1, raw tiles of
    // step s + 3, MFMAs of step s
    __syncthreads();
    unit_load(I1{});
    transform(I1{});
    raw_load(I3{});
    mfmas(I0{});
    __syncthreads();
    unit_load(I2{});
    transform(I2{});
    mfmas(I1{});
    __syncthreads();
    unit_load(I3{});
    transform(I3{});
    mfmas(I2{});
    __syncthreads();
    mfmas(I3{});

    // ---- epilogue, part 1: M[pos 18][co 32][tile 16] through LDS (V buffer 0: last read in step 2, behind a barrier)
    if (mfma_wave && (lane & 16) == 0) {
        float* mw = mq + (jj * 6 + 3 * ki) * 512 + (4 * (lane >> 5)) * 16 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < 3; kk++)
#pragma unroll
            for (int v = 0; v < 16; v++) mw[kk * 512 + ((v & 3) + 8 * (v >> 2)) * 16] = acc[kk][v];
    }
    const int ec = tid >> 4, et = tid & 15, ety = et >> 2, etx = et & 3;
    const int ch = cog * 32 + ec;
    const size_t plane = ((size_t)bd * T::C + ch) * T::GPLANE;
    const int po = (4 * ety) * 16 + 4 * etx;    // this thread's patch inside the plane (row a: + 16 a)
    __syncthreads();
    float own[3][4];                            // half 0: (h0 + s12, d12, s12); half 1: (s34, d34, h5); per column e
    {
        const float* mp = mq + ec * 16 + et;
        float hh[3][4];
#pragma unroll
        for (int i = 0; i < 3; i++) {           // the k-direction transform of row 3 half + i (the batched kernel's hrow)
            float m[6];
#pragma unroll
            for (int k = 0; k < 6; k++) m[k] = mp[(6 * i + k) * 512];
            wino_out_row(m[0], m[1], m[2], m[3], m[4], m[5], hh[i][0], hh[i][1], hh[i][2], hh[i][3]);
        }
#pragma unroll
        for (int ee = 0; ee < 4; ee++) {
            if (half == 0) {
                const float s12 = hh[1][ee] + hh[2][ee];
                own[0][ee] = hh[0][ee] + s12;
                own[1][ee] = hh[1][ee] - hh[2][ee];
                own[2][ee] = s12;
            } else {
                own[0][ee] = hh[0][ee] + hh[1][ee];
                own[1][ee] = hh[0][ee] - hh[1][ee];
                own[2][ee] = hh[2][ee];
            }
        }
    }
    // ---- part 2: publish the partial, draw a ticket; the pair's second arriver combines (trunk15_wino3s.h)
    const int pairi = bd * 4 + cog;
    {
        f32x4* slab = reinterpret_cast<f32x4*>(slabs + ((size_t)pairi * 2 + half) * T::SLAB_FLOATS) + tid * 3;
#pragma unroll
        for (int v = 0; v < 3; v++) slab[v] = f32x4{own[v][0], own[v][1], own[v][2], own[v][3]};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // every wave: its slab stores have left
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (keep: the fence's own wait can be dropped by the compiler)
        const unsigned old = __hip_atomic_exchange(tickets + pairi, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned second = old == epoch ? 1u : 0u;         // the other half of this launch has been here
        if (second) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *lflag = second;
    }
    __syncthreads();
    if (*lflag == 0u) return;                   // first arriver of the pair: done (uniform)
    float other[3][4];
    {
        const f32x4* slab = reinterpret_cast<const f32x4*>(slabs + ((size_t)pairi * 2 + (half ^ 1)) * T::SLAB_FLOATS) + tid * 3;
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const f32x4 t4 = slab[v];
            other[v][0] = t4[0]; other[v][1] = t4[1]; other[v][2] = t4[2]; other[v][3] = t4[3];
        }
    }
    f32x4 rs[4];
    if (RESID) {                                // (row 15 does not exist: the batched kernel reads zeros for it)
#pragma unroll
        for (int a = 0; a < 4; a++)
            rs[a] = (4 * ety + a < 15) ? *reinterpret_cast<const f32x4*>(resid + plane + po + 16 * a) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float bv = bias[ch];
    const float is = SCALED ? bias[128 + ch] * xisc : bias[128 + ch];   // 1 / S of the channel (a power of two)
    f32x4 y[4];
#pragma unroll
    for (int ee = 0; ee < 4; ee++) {
        const float lo0 = half == 0 ? own[0][ee] : other[0][ee], d12 = half == 0 ? own[1][ee] : other[1][ee],
                    s12 = half == 0 ? own[2][ee] : other[2][ee];
        const float s34 = half == 0 ? other[0][ee] : own[0][ee], d34 = half == 0 ? other[1][ee] : own[1][ee],
                    h5 = half == 0 ? other[2][ee] : own[2][ee];
        y[0][ee] = lo0 + s34;                                  // (hrow0 + s12) + s34
        y[1][ee] = __builtin_fmaf(2.f, d34, d12);
        y[2][ee] = __builtin_fmaf(4.f, s34, s12);
        y[3][ee] = __builtin_fmaf(8.f, d34, d12) + h5;
    }
    float chk = 0.f;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        f32x4 v;
#pragma unroll
        for (int ee = 0; ee < 4; ee++) v[ee] = __builtin_fmaf(y[a][ee], is, bv);
        if (RESID) v += rs[a];
        chk += wino_sum4(v);
#pragma unroll
        for (int ee = 0; ee < 4; ee++) v[ee] = fmaxf(v[ee], 0.f);
        if (etx == 3) v[3] = 0.f;               // column 15 is the halo column of the rows16 layout
        if (4 * ety + a < 15) *reinterpret_cast<f32x4*>(out + plane + po + 16 * a) = v;
    }
    // (a plain store: every writer writes the same 1, and the word may live in pinned host memory)
    if (wino_nonfinite(chk) && flag) *reinterpret_cast<volatile unsigned*>(flag) = 1u;
}

}  // namespace apz
