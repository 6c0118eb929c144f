// Wavefront-wide max and sum for gfx950 (64 lanes): a butterfly of five xor shuffles, so every lane ends with the result and
// the order of the operations is fixed -- the bits do not depend on the batch or on the launch shape.
#pragma once
#include <hip/hip_runtime.h>

namespace apz {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace apz
