// Dihedral leaf symmetry of the evaluator (apz_set_leaf_symmetry): the forward sees an IMAGE of every position and the
// caller gets the answer folded back, so that nothing outside these two kernels knows about it.
//
// Position codes and pi are bottom-row-first, so both move with perm_p (the pi table of apz_augment8, reference order r1,
// r1f, r2, r2f, r3, r3f, id, idf; k = 6 is the identity):
//   image k of a code row    codes_k[p] = codes[perm_p[k][p]] for p < HW, byte HW (the colour) copied, pad bytes 0 -- the
//                            code row of get_equi_data's k-th image: encode(codes_k) == encode(codes)[:, perm_s[k]]
//   fold back                the net answers q_k on image k; the position's policy is probs[perm_p[k][p]] = q_k[p], i.e.
//                            probs[m] = q_k[inv_p[k][m]] with inv_p[k] the inverse permutation; the value is unchanged
//   APZ_SYM_KEYED            every board on ONE image, k = leaf_sym_key(seed, its HW + 1 bytes): a function of the seed and
//                            the position only, not of the batch, the row or the launch
//   APZ_SYM_MEAN8            board b becomes rows 8b .. 8b + 7 (image k in row 8b + k) of one forward of 8n boards;
//                            probs[m] = 0.125f * (((((((u_0 + u_1) + u_2) + u_3) + u_4) + u_5) + u_6) + u_7), u_k the folded
//                            policy of image k: plain fp32 adds in k order (the translation unit is compiled with
//                            -ffp-contract=off: no fma); the value likewise from the eight tanh outputs
//
//  sym_expand_kernel<MEAN8>  one wavefront per board: the source row ONCE with 16-byte loads into LDS (in the slot path the
//                            source is pinned host memory over PCIe), the key by an exact 64-bit wave sum, the image row(s)
//                            gathered from LDS and stored as whole dwords, k as one byte per board
//  sym_fold_kernel<MEAN8>    head outputs of the images -> the caller's [n][HW] probs and [n] values.  The gather form: every
//                            destination row is stored contiguously and completely (in the slot path it is device-mapped
//                            pinned memory: scattered loads from L2 are cheap, scattered stores over PCIe are not)
// Both: no atomics, every output byte written by exactly one lane, nothing read that the launch did not get as input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace apz {

__host__ __device__ inline uint64_t leaf_sym_fmix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// The key of a code row: t_i = fmix64(seed + 0x9E3779B97F4A7C15 (256 i + byte_i + 1)) for i = 0 .. hw, all mod 2^64, and
// k = fmix64(seed ^ sum_i t_i) >> 61.  The sum is order-free, so the terms may be spread over any number of parties: a
// party takes i = first, first + step, ... and `total` turns its partial sum into the sum over all parties.  The host takes
// every term itself (first 0, step 1, total = identity), a wavefront one lane per party (first = lane, step 64, total =
// leaf_sym_wave_sum) -- the arithmetic is this one function either way.
template <class Total>
__host__ __device__ inline int leaf_sym_key(uint64_t seed, const unsigned char* row, int hw, int first, int step, Total total) {
    uint64_t part = 0;
    for (int i = first; i <= hw; i += step)
        part += leaf_sym_fmix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(256 * i + (int)row[i] + 1));
    return (int)(leaf_sym_fmix64(seed ^ total(part)) >> 61);
}

struct LeafSym {
    static constexpr int WAVES = 4, THREADS = 64 * WAVES;   // boards per workgroup of sym_expand_kernel
    static constexpr int MAX_STRIDE = 256;                   // >= the code stride of the largest board (15x15: 240)
    static int expand_grid(int n) { return (n + WAVES - 1) / WAVES; }
};

// exact sum over the 64 lanes of a wavefront, the same value in every lane (butterfly on the two 32-bit halves)
__device__ inline uint64_t leaf_sym_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// codes [n][stride] -> out [n (MEAN8: 8 n)][stride], k_out [n].  stride: a multiple of 16, <= LeafSym::MAX_STRIDE; both
// code buffers 16-byte aligned.  perm_p [8][hw].  Grid: LeafSym::expand_grid(n) workgroups of LeafSym::THREADS.
template <bool MEAN8>
__global__ __launch_bounds__(LeafSym::THREADS) void sym_expand_kernel(const unsigned char* __restrict__ codes,
                                                                      const int* __restrict__ perm_p,
                                                                      unsigned char* __restrict__ out,
                                                                      unsigned char* __restrict__ k_out, int n, int hw,
                                                                      int stride, uint64_t seed) {
    __shared__ uint4 rows[LeafSym::WAVES][LeafSym::MAX_STRIDE / 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * LeafSym::WAVES + wave;
    const bool live = b < n;                                  // (a wave without a board still meets the barrier)
    if (live && lane < stride / 16) rows[wave][lane] = ((const uint4*)(codes + (size_t)b * stride))[lane];
    __syncthreads();
    if (!live) return;
    const unsigned char* row = (const unsigned char*)rows[wave];
    const int key = leaf_sym_key(seed, row, hw, lane, 64, [](uint64_t part) { return leaf_sym_wave_sum(part); });
    if (lane == 0) k_out[b] = (unsigned char)key;
    const int dwords = stride / 4;
    const int images = MEAN8 ? 8 : 1;
    for (int i = lane; i < images * dwords; i += 64) {
        const int img = i / dwords, d = i - img * dwords;
        const int k = MEAN8 ? img : key;
        const int* pk = perm_p + k * hw;
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = 4 * d + j;
            const unsigned byte = p < hw ? row[pk[p]] : (p == hw ? row[hw] : 0u);
            word |= byte << (8 * j);
        }
        ((unsigned*)(out + ((size_t)b * images + img) * stride))[d] = word;
    }
}

// q [n (MEAN8: 8 n)][hw], v [n (MEAN8: 8 n)]: the head's outputs on the rows sym_expand_kernel wrote; k_in [n] its keys
// (not read under MEAN8); inv_p [8][hw]: inv_p[k][perm_p[k][p]] = p.  -> probs [n][hw], values [n].  Grid-stride over
// (board, cell), the cell fastest.
template <bool MEAN8>
__global__ __launch_bounds__(256) void sym_fold_kernel(const float* __restrict__ q, const float* __restrict__ v,
                                                       const unsigned char* __restrict__ k_in, const int* __restrict__ inv_p,
                                                       float* __restrict__ probs, float* __restrict__ values, int n, int hw) {
    const long total = (long)n * hw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw), m = (int)(i - (long)b * hw);
        if (MEAN8) {
            const float* qb = q + (size_t)b * 8 * hw;
            float s = qb[inv_p[m]];
#pragma unroll
            for (int k = 1; k < 8; k++) s = s + qb[(size_t)k * hw + inv_p[k * hw + m]];
            probs[i] = 0.125f * s;
            if (m == 0) {
                const float* vb = v + (size_t)b * 8;
                float t = vb[0];
#pragma unroll
                for (int k = 1; k < 8; k++) t = t + vb[k];
                values[b] = 0.125f * t;
            }
        } else {
            const int k = k_in[b] & 7;
            probs[i] = q[(size_t)b * hw + inv_p[k * hw + m]];
            if (m == 0) values[b] = v[b];
        }
    }
}

}  // namespace apz
