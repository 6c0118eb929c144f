// The trainer's averaged weights (apz_ema_update; HipTrainer(ema_decay=...)): an exponential moving average of every
// parameter tensor -- BatchNorm moving statistics and pinned gammas included -- kept in a shadow copy on the device and
// moved by ONE launch queued directly behind each Adam launch, under that Adam launch's skip rule.
//
//  ema_update_kernel   grid (32, ntensors) x 256 over a table of { shadow, weight, n } -- the Adam launch's own fixed shape.
//                      Workgroup (b, t) walks its grid-stride share of tensor t:  s = s + c * (w - s), the subtraction, the
//                      product and the sum each rounded on its own (never a fused multiply-add), so that the NumPy float32
//                      expression s + c * (w - s) gives the same bits.  What keeps the compiler from contracting them is
//                      `#pragma clang fp contract(off)` in the kernel and -ffp-contract=off on the build line
//                      (alphapig_amd/build.py, tools/device_code_diff.py) -- NOT the __f*_rn spellings, which this
//                      toolchain's headers define as plain +, * and - and which only say what is meant;
//                      tests/test_gpu_ema.py compares the bits.  w == s gives w - s = +0 and leaves the value as it
//                      is: a pinned gamma stays exactly 1.  Element accesses only: a tensor may start anywhere on the float
//                      grid and nothing outside [s, s + n) is written.  No atomics and no scratch.
//                      skip_a / skip_b (each may be NULL): device words; when either is not zero at the time the launch
//                      runs, every workgroup returns before its first store -- the f16x2 overflow word, or the `skip` word
//                      of the guard's record, read the way adam_step_unless_kernel reads its word.
#pragma once
#include <hip/hip_runtime.h>

namespace apz {

struct EmaTensor {      // 24 bytes; include/alphapig_hip.h documents it
    float* s;           // the shadow (the average): read and written
    const float* w;     // the weight: read
    long long n;
};

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaTensor* __restrict__ tab, float c,
                                                         const unsigned* __restrict__ skip_a,
                                                         const unsigned* __restrict__ skip_b) {
#pragma clang fp contract(off)
    if (skip_a && *reinterpret_cast<const volatile unsigned*>(skip_a)) return;
    if (skip_b && *reinterpret_cast<const volatile unsigned*>(skip_b)) return;
    const EmaTensor T = tab[blockIdx.y];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < T.n; i += (long long)gridDim.x * blockDim.x) {
        const float s = T.s[i];
        T.s[i] = __fadd_rn(s, __fmul_rn(c, __fsub_rn(T.w[i], s)));
    }
}

}  // namespace apz
