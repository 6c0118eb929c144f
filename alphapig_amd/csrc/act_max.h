// max |x| of an activation tensor in the trunk's rows16 layout [n][128][15][16] (pad column zero: it cannot raise a maximum).
// gfx950.  Feeds the static activation exponents of the f16x2 trunk kernel (trunk15_wino3h16.h, WINO3H16_PLAIN_SCALED): it
// runs in a calibration forward and in the exact repeat of an overflowed forward, never in the steady state.
//
// One pass over HBM: every thread takes 16-byte loads in a grid-stride loop, a wave folds its 64 maxima with
// shuffles, the four waves of a workgroup meet in LDS, and thread 0 writes ONE partial per workgroup with an ordinary
// store.  No atomics: the host folds the `gridDim.x` partials.  A maximum is exact in any order, so the result does not
// depend on the grid.  fmaxf ignores a NaN operand (a NaN activation does not show here; the f16x2 kernel's own overflow
// word reports it); +inf survives every fold and is reported as such.
#pragma once
#include <hip/hip_runtime.h>

#include "conv3x3_mfma.h"

namespace apz {

struct ActMax {
    static constexpr int THREADS = 256;
    static constexpr int MAX_PARTS = 512;         // partials per tensor: two workgroups per CU of an MI355X
    // workgroups for `n4` 16-byte elements: at least four loads per thread before another workgroup is worth its launch
    static int grid_for(long n4) {
        const long g = (n4 + 4L * THREADS - 1) / (4L * THREADS);
        return (int)(g < 1 ? 1 : (g > MAX_PARTS ? MAX_PARTS : g));
    }
};

// x: n4 x 16 bytes (16-byte aligned); part[gridDim.x]
__global__ __launch_bounds__(ActMax::THREADS) void act_absmax_kernel(const float* __restrict__ x, long n4,
                                                                     float* __restrict__ part) {
    __shared__ float wmax[ActMax::THREADS / 64];
    const f32x4* p = reinterpret_cast<const f32x4*>(x);
    const long stride = (long)gridDim.x * ActMax::THREADS;
    float m = 0.f;
#pragma unroll 4
    for (long i = (long)blockIdx.x * ActMax::THREADS + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = p[i];                                             // global_load_dwordx4
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < ActMax::THREADS / 64; w++) m = fmaxf(m, wmax[w]);
        part[blockIdx.x] = m;
    }
}

}  // namespace apz
