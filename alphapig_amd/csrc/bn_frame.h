// Padded-row BatchNorm, whole board or framed: the four passes of the training step on the trunk's layout
// [n][C][15][16] (plane = 60 float4), each one kernel body on a compile-time board policy.
//
//  bn_stats_rows_kernel        per-(channel, split) sums of x and x^2
//  bn_apply_rows_kernel        y = act(x sc + shift (+ resid)) and the ReLU byte mask
//  bn_bwd_reduce_rows_kernel   per-(channel, split) sums of dz and dz xhat
//  bn_bwd_apply_rows_kernel    dx and dres; dxsum / dxmax per split
//
// 16-byte accesses, no per-element index division; a workgroup walks four boards per trip (4 x 60 of its 256 threads), and
// a thread owns one float4 index k of a plane for the whole launch (row k >> 2, columns 4 (k & 3) .. + 3).
//
// Board15 is the 15x15 board: the pad elements are zero on input, so they add nothing to any sum, and are written back
// as zero (the pad-column rule (k & 3) == 3); nothing else is selected.  The policy is empty: one argument byte nobody reads.
//
// BoardFrame is a board of side S < 15 on the 15x15 trunk kernels (csrc/frame15.h).  The trunk's convolutions and their
// data gradients write whole 15x15 planes, so every tensor a BatchNorm pass reads may hold anything in its off-board cells
// (bias-and-neighbour values after a convolution; uninitialised memory, NaN and inf included, in the rows the heads'
// backward pass never writes).  What a convolution READS must be zero there.  The mask therefore sits in these four
// passes and nowhere else:
//
//  statistics       sums over on-board cells only (the caller's count is n S S)
//  apply            y and the ReLU byte mask: off-board cells exactly +0 / bit 0
//  backward reduce  dz and xhat selected before they are summed (relu = 0 has no ReLU bit to hide behind)
//  backward apply   dx and dres: off-board cells exactly +0; dxsum / dxmax from the masked values
//
// Masking is by selection (keep ? v : 0), never by multiplication: 0 * NaN is NaN.  A thread's mask is four bits computed
// once: bit e = [row < S and 4 (k & 3) + e < S].  S = 15 gives the pad-column rule, and with it Board15's bits: the
// operation order within a thread, the block_sum_256 / channel_sums tree, the grid and the 16-byte accesses are the same.
// S is a runtime argument: one code object per kernel serves every size.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_train.h"

namespace apz {

// bit e: element e of float4 k of a padded-row plane lies on the S x S board
__device__ __forceinline__ unsigned frame_keep_bits(int k, int S) {
    const int row = k >> 2, col = (k & 3) * 4;
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) bits |= (unsigned)(row < S && col + e < S) << e;
    return bits;
}

__device__ __forceinline__ f32x4 frame_select(f32x4 v, unsigned keep) {
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = (keep >> e) & 1u ? v[e] : 0.f;
    return v;
}

struct Board15 {
    static constexpr bool FRAME = false;
    __device__ __forceinline__ unsigned keep_bits(int) const { return 0; }      // (not looked at)
};
struct BoardFrame {
    static constexpr bool FRAME = true;
    int S;                                   // the board's side
    __device__ __forceinline__ unsigned keep_bits(int k) const { return frame_keep_bits(k, S); }
};

// what a pass reads before it sums: the framed board's cells only (Board15: the pad elements are zero already)
template <class B>
__device__ __forceinline__ f32x4 rows_read(f32x4 v, unsigned keep) {
    if constexpr (B::FRAME) return frame_select(v, keep);
    return v;
}

// what a pass writes: off the board (the pad column included) exactly +0
template <class B>
__device__ __forceinline__ f32x4 rows_written(f32x4 v, unsigned keep, int k) {
    if constexpr (B::FRAME) return frame_select(v, keep);
    if ((k & 3) == 3) v[3] = 0.f;            // the pad column (60 float4 per plane: 4 per row)
    return v;
}

template <class B>
__global__ __launch_bounds__(256) void bn_stats_rows_kernel(const float* __restrict__ x, double* __restrict__ part, int n, int C,
                                                            B board) {
    __shared__ double sh[4];
    const int c = blockIdx.x, t = threadIdx.x, sub = t / 60, k = t - sub * 60;   // 4 boards per trip, 60 float4 each
    const unsigned keep = board.keep_bits(k);
    double s1 = 0.0, s2 = 0.0;
    if (sub < 4)
        for (int b = blockIdx.y * 4 + sub; b < n; b += gridDim.y * 4) {
            const f32x4 v = rows_read<B>(reinterpret_cast<const f32x4*>(x + ((size_t)b * C + c) * 240)[k], keep);
            // squares and sums in double, as bn_stats_kernel: an fp32 (v0^2 + v1^2) + ... loses (1 + mean^2 / var) ulps of the
            // variance to the cancellation in sum x^2 / M - mean^2 (the kernel is bound by its loads)
            const double d0 = v[0], d1 = v[1], d2 = v[2], d3 = v[3];
            s1 += (d0 + d1) + (d2 + d3);
            s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    s1 = block_sum_256(s1, sh);
    s2 = block_sum_256(s2, sh);
    if (t == 0) {
        part[2 * ((size_t)c * gridDim.y + blockIdx.y)] = s1;
        part[2 * ((size_t)c * gridDim.y + blockIdx.y) + 1] = s2;
    }
}

template <class B>
__global__ __launch_bounds__(256) void bn_apply_rows_kernel(const float* __restrict__ x, const float* __restrict__ resid,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const double* __restrict__ part, int psplits, BnFinal fin,
                                                            float* __restrict__ y, unsigned char* __restrict__ mask, int n,
                                                            int C, int relu, B board) {
    __shared__ double sh[4];
    const int c = blockIdx.x, t = threadIdx.x, sub = t / 60, k = t - sub * 60;
    float m, is;
    channel_stats(part, c, psplits, sh, fin, m, is);
    const float sc = is * (gamma ? gamma[c] : 1.f), shf = beta[c] - m * sc;
    if (sub >= 4) return;
    const unsigned keep = board.keep_bits(k);
    for (int b = blockIdx.y * 4 + sub; b < n; b += gridDim.y * 4) {
        const size_t o = ((size_t)b * C + c) * 60 + k;
        f32x4 a = reinterpret_cast<const f32x4*>(x)[o];
        a = a * sc + shf;
        if (resid) a += reinterpret_cast<const f32x4*>(resid)[o];
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; e++) a[e] = fmaxf(a[e], 0.f);
        }
        a = rows_written<B>(a, keep, k);
        reinterpret_cast<f32x4*>(y)[o] = a;
        // the ReLU decisions of these four elements for the backward pass: one byte per 16 bytes of y (bn_bwd_* then read
        // 3.9 MB instead of the 63 MB output tensor per 512-board layer, twice)
        if (mask) mask[o] = (unsigned char)((a[0] > 0.f) | ((a[1] > 0.f) << 1) | ((a[2] > 0.f) << 2) | ((a[3] > 0.f) << 3));
    }
}

// dz of one float4: dy behind the ReLU decision (the byte mask, else the forward output), then behind the board mask; and
// the float4 of x beside it -> xv.  Board15 issues both loads in front of the ReLU branch, BoardFrame loads x behind the
// selection: the order each kernel has always had, kept so that its device code stays what was measured.
template <class B>
__device__ __forceinline__ f32x4 rows_dz(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ out,
                                         const unsigned char* __restrict__ mask, size_t o, int relu, unsigned keep, f32x4& xv) {
    f32x4 g = reinterpret_cast<const f32x4*>(dy)[o];
    if constexpr (!B::FRAME) xv = reinterpret_cast<const f32x4*>(x)[o];
    if (relu && mask) {
        const unsigned bits = mask[o];
#pragma unroll
        for (int e = 0; e < 4; e++) g[e] = (bits >> e) & 1u ? g[e] : 0.f;
    } else if (relu) {
        const f32x4 ov = reinterpret_cast<const f32x4*>(out)[o];
#pragma unroll
        for (int e = 0; e < 4; e++) g[e] = ov[e] > 0.f ? g[e] : 0.f;
    }
    g = rows_read<B>(g, keep);
    if constexpr (B::FRAME) xv = reinterpret_cast<const f32x4*>(x)[o];
    return g;
}

// xhat of element e as the backward sums take it: off the framed board 0 (0 * NaN is NaN: x is selected too)
template <class B>
__device__ __forceinline__ float rows_xhat(float x, float m, float is, unsigned keep, int e) {
    if constexpr (B::FRAME) return (keep >> e) & 1u ? (x - m) * is : 0.f;
    return (x - m) * is;
}

template <class B>
__global__ __launch_bounds__(256) void bn_bwd_reduce_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ out, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, double* __restrict__ part,
                                                                 const unsigned char* __restrict__ mask, int n, int C, int relu,
                                                                 B board) {
    __shared__ double sh[4];
    const int c = blockIdx.x, t = threadIdx.x, sub = t / 60, k = t - sub * 60;
    const unsigned keep = board.keep_bits(k);
    const float m = mean[c], is = invstd[c];
    double s1 = 0.0, s2 = 0.0;
    if (sub < 4)
        for (int b = blockIdx.y * 4 + sub; b < n; b += gridDim.y * 4) {
            const size_t o = ((size_t)b * C + c) * 60 + k;
            f32x4 xv;
            const f32x4 g = rows_dz<B>(dy, x, out, mask, o, relu, keep, xv);
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                a1 += g[e];
                a2 += g[e] * rows_xhat<B>(xv[e], m, is, keep, e);
            }
            s1 += a1;
            s2 += a2;
        }
    s1 = block_sum_256(s1, sh);
    s2 = block_sum_256(s2, sh);
    if (t == 0) {
        part[2 * ((size_t)c * gridDim.y + blockIdx.y)] = s1;
        part[2 * ((size_t)c * gridDim.y + blockIdx.y) + 1] = s2;
    }
}

template <class B>
__global__ __launch_bounds__(256) void bn_bwd_apply_rows_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ out, const float* __restrict__ gamma,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const double* __restrict__ part, int psplits,
                                                                float* __restrict__ dx, float* __restrict__ dres,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ dxsum, int dxsum_ld,
                                                                const unsigned char* __restrict__ mask, int n, int C, int relu,
                                                                double M, float* __restrict__ dxmax, B board) {
    __shared__ double sh[4];
    const int c = blockIdx.x, t = threadIdx.x, sub = t / 60, k = t - sub * 60;
    const unsigned keep = board.keep_bits(k);
    double s1, s2;
    channel_sums(part, c, psplits, sh, s1, s2);
    if (blockIdx.y == 0 && t == 0) {
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
    }
    const float m = mean[c], is = invstd[c], k0 = (float)(s1 / M), k1 = (float)(s2 / M);
    const float gi = (gamma ? gamma[c] : 1.f) * is;
    double ds = 0.0;
    float dm = 0.f;
    if (sub < 4)
        for (int b = blockIdx.y * 4 + sub; b < n; b += gridDim.y * 4) {
            const size_t o = ((size_t)b * C + c) * 60 + k;
            f32x4 xv;
            f32x4 g = rows_dz<B>(dy, x, out, mask, o, relu, keep, xv);
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; e++) r[e] = gi * (g[e] - k0 - (xv[e] - m) * is * k1);
            r = rows_written<B>(r, keep, k);     // gradients do not flow back over the board's edge
            g = rows_written<B>(g, keep, k);     // (BoardFrame: selected in rows_dz already)
            reinterpret_cast<f32x4*>(dx)[o] = r;
            if (dres) reinterpret_cast<f32x4*>(dres)[o] = g;
            ds += (double)((r[0] + r[1]) + (r[2] + r[3]));
            if (dxmax) dm = fmaxf(dm, fmaxf(fmaxf(fabsf(r[0]), fabsf(r[1])), fmaxf(fabsf(r[2]), fabsf(r[3]))));
        }
    if (dxsum) {
        ds = block_sum_256(ds, sh);
        if (t == 0) dxsum[(size_t)blockIdx.y * dxsum_ld + c] = (float)ds;
    }
    if (dxmax) {   // [split][C]: max |dx| of this workgroup (the input scale of trunk15_wino3h16_train_kernel's data gradient)
        dm = block_max_256(dm, reinterpret_cast<float*>(sh));
        if (t == 0) dxmax[(size_t)blockIdx.y * C + c] = dm;
    }
}

}  // namespace apz
