// The optimiser step's guard: the global norm of the step's gradients, global-norm clipping and a refusal of non-finite
// steps, all on the device (apz_grad_norm / apz_adam_step_guarded; HipTrainer(step_guard=True, clip_norm=...)).
//
//  grad_sumsq_kernel         grid (32, ntensors) x 256 over the Adam tensor table -- the Adam launch's own fixed shape, so no
//                            bit depends on the number of CUs.  Workgroup (b, t) walks its grid-stride share of tensor t's
//                            gradient, squares every element in double (a float squared is exact there) and adds; the block
//                            goes through block_sum_256's fixed tree.  Out, by ordinary stores (no atomics): one double and
//                            one "saw a non-finite element" word per workgroup, at index 32 t + b.
//  grad_guard_fold_kernel    ONE workgroup: tensor t's 32 partials added in index order by one thread, the tensor sums then
//                            added in index order by thread 0 (a fixed order, whatever ran first); norm = sqrt(total) *
//                            rescale; the verdict as one 16-byte GuardRecord.
//  adam_step_guarded_kernel  returns when the record says skip, else conv_train.h's adam_step_body with the record's
//                            rescale_eff as its `rescale`.  The clip travels INSIDE that argument: a step that neither clips
//                            nor skips has rescale_eff == rescale bit for bit and is adam_step_kernel's step by construction,
//                            whatever the compiler contracts inside the body (a factor multiplied in beside `rescale` would
//                            round differently under fused multiply-adds).
//
// Which thread adds which element never depends on where the tensor starts: a thread owns LOGICAL quads (elements 4 q .. 4 q
// + 3 of the tensor) and adds them in index order.  A tensor that starts h = 1 .. 3 floats past a 16-byte boundary is read
// through the aligned 16-byte vectors around each quad (two per quad; the neighbour's is a cache hit); the vectors that
// straddle the tensor's first and last element -- the head and the tail -- are read element by element, so nothing outside
// [g, g + n) is touched, and missing elements count as +0, which changes neither a sum nor the non-finite word.  The same
// values in differently aligned storage therefore give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conv_train.h"

namespace apz {

struct GuardRecord {        // 16 bytes, 16-byte aligned; include/alphapig_hip.h documents it
    float norm;             // sqrt(sum g^2) * rescale: the norm of the gradient Adam sees (before weight decay)
    float rescale_eff;      // what adam_step_body gets as `rescale`
    unsigned skip;          // why != 0
    unsigned why;           // GUARD_* bits
};
enum : unsigned { GUARD_GRAD = 1u, GUARD_LOSS = 2u, GUARD_SKIP_IN = 4u, GUARD_NORM = 8u };
constexpr int GUARD_SPLITS = 32;        // gridDim.x of grad_sumsq_kernel = partials per tensor

__device__ __forceinline__ bool guard_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// aligned vector j of the 16-byte grid the tensor sits on (a = g - h floats): logical elements 4 j - h .. 4 j - h + 3
__device__ __forceinline__ f32x4 guard_vec(const float* __restrict__ g, long long n, int h, long long j) {
    const long long lo = 4 * j - h;
    if (lo >= 0 && lo + 4 <= n) return *reinterpret_cast<const f32x4*>(g + lo);     // (g + lo = a + 4 j: 16-byte aligned)
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (lo + k >= 0 && lo + k < n) ? g[lo + k] : 0.f;
    return v;
}

template <int H>
__device__ __forceinline__ void guard_walk(const float* __restrict__ g, long long n, double& s, unsigned& bad) {
    const long long quads = (n + 3) / 4;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
        const f32x4 a = guard_vec(g, n, H, q);
        f32x4 x = a;
        if (H != 0) {
            const f32x4 b = guard_vec(g, n, H, q + 1);
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = (k + H < 4) ? a[(k + H) & 3] : b[(k + H) & 3];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            bad |= (unsigned)guard_nonfinite(x[k]);
            s += (double)x[k] * (double)x[k];
        }
    }
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamTensor* __restrict__ tab, double* __restrict__ part,
                                                         unsigned* __restrict__ bad_out) {
    __shared__ double sh[4];
    __shared__ unsigned shbad[4];
    const AdamTensor T = tab[blockIdx.y];
    double s = 0.0;
    unsigned bad = 0;
    switch ((int)((reinterpret_cast<uintptr_t>(T.g) >> 2) & 3)) {      // floats past a 16-byte boundary: uniform
        case 0: guard_walk<0>(T.g, T.n, s, bad); break;
        case 1: guard_walk<1>(T.g, T.n, s, bad); break;
        case 2: guard_walk<2>(T.g, T.n, s, bad); break;
        default: guard_walk<3>(T.g, T.n, s, bad); break;
    }
    const bool wave_bad = __any((int)bad);
    if ((threadIdx.x & 63) == 0) shbad[threadIdx.x >> 6] = wave_bad;
    s = block_sum_256(s, sh);           // (its barriers order shbad as well)
    if (threadIdx.x == 0) {
        const size_t o = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[o] = s;
        bad_out[o] = shbad[0] | shbad[1] | shbad[2] | shbad[3];
    }
}

// count = ntensors partial groups of GUARD_SPLITS.  loss3 / skip_in may be NULL.  One workgroup of 256.
__global__ __launch_bounds__(256) void grad_guard_fold_kernel(const double* __restrict__ part, const unsigned* __restrict__ bad,
                                                              int ntensors, float rescale, float clip,
                                                              const float* __restrict__ loss3, const unsigned* __restrict__ skip_in,
                                                              GuardRecord* __restrict__ rec) {
    __shared__ double tsum[256];
    __shared__ unsigned shbad[4];
    double total = 0.0;
    unsigned any_bad = 0;
    for (int t0 = 0; t0 < ntensors; t0 += 256) {        // (uniform trip count: the barriers below are safe)
        const int t = t0 + threadIdx.x;
        double s = 0.0;
        if (t < ntensors) {
#pragma unroll
            for (int k = 0; k < GUARD_SPLITS; k++) {
                s += part[(size_t)t * GUARD_SPLITS + k];
                any_bad |= bad[(size_t)t * GUARD_SPLITS + k];
            }
        }
        __syncthreads();
        tsum[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(256, ntensors - t0);
            for (int k = 0; k < m; k++) total += tsum[k];
        }
    }
    const bool wave_bad = __any((int)(any_bad != 0));
    if ((threadIdx.x & 63) == 0) shbad[threadIdx.x >> 6] = wave_bad;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double norm = sqrt(total) * (double)rescale;
    unsigned why = 0;
    if ((shbad[0] | shbad[1] | shbad[2] | shbad[3]) || !(fabs(total) <= 1.79769313486231570815e308)) why |= GUARD_GRAD;
    if (loss3 && (guard_nonfinite(loss3[0]) || guard_nonfinite(loss3[1]) || guard_nonfinite(loss3[2]))) why |= GUARD_LOSS;
    if (skip_in && *reinterpret_cast<const volatile unsigned*>(skip_in)) why |= GUARD_SKIP_IN;
    const float normf = (float)norm;
    if (clip > 0.f && !(why & GUARD_GRAD) && guard_nonfinite(normf)) why |= GUARD_NORM;
    float eff = rescale;
    if (clip > 0.f && !(norm <= (double)clip)) eff = rescale * (float)((double)clip / norm);
    union {
        GuardRecord r;
        uint4 v;
    } out;
    out.r.norm = normf;
    out.r.rescale_eff = eff;
    out.r.skip = why != 0;
    out.r.why = why;
    *reinterpret_cast<uint4*>(rec) = out.v;      // one 16-byte vector store
}

__global__ __launch_bounds__(256) void adam_step_guarded_kernel(const AdamTensor* __restrict__ tab, float lr_t, float b1, float b2,
                                                                float eps, const GuardRecord* __restrict__ rec) {
    if (*reinterpret_cast<const volatile unsigned*>(&rec->skip)) return;
    adam_step_body(tab, lr_t, b1, b2, eps, rec->rescale_eff);
}

}  // namespace apz
