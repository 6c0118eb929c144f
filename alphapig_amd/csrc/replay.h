// Mini-batch gather of the device replay buffer (alphapig_amd/replay.py: DeviceReplayBuffer): position codes, pi and z
// stay in device memory as the self-play exchange delivers them (one ring slot per tuple, un-augmented), and a sampled
// mini-batch is decoded and rotated where the trainer reads it -- nothing goes through the host.
#pragma once
#include <hip/hip_runtime.h>

namespace apz {

// entries [n] i32: slot * 8 + symmetry.  For sample j:
//   planes_out[j][c][p] = P[c][perm_s[k][p]]   with P = the planes encode_planes_kernel (heads.h) writes for code row `slot`
//   pi_out[j][p]        = pi[slot][perm_p[k][p]]
//   z_out[j]            = z[slot]
// -- every bit of apz_encode_planes followed by row k of apz_augment8.  P is never materialised: P's cell q (planes are
// top-row-first) is code byte (H - 1 - q / W) * W + q % W (codes and pi are bottom-row-first: encode_planes_kernel's `o`
// read backwards), so a thread reads the ONE code byte of its source cell and writes all NP planes of its output cell.
// Grid-stride over (sample, cell), the cell fastest: the stores to each plane are contiguous.  The host side has
// checked 0 <= entry < 8 * capacity (apz_replay_gather).
__global__ void replay_gather_kernel(const unsigned char* __restrict__ codes, const float* __restrict__ pi,
                                     const float* __restrict__ z, const int* __restrict__ entries,
                                     const int* __restrict__ perm_s, const int* __restrict__ perm_p,
                                     float* __restrict__ planes_out, float* __restrict__ pi_out, float* __restrict__ z_out,
                                     int n, int H, int W, int stride, int NP) {
    const int HW = H * W;
    const long total = (long)n * HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / HW), p = (int)(i - (long)j * HW);
        const int ent = entries[j];
        const size_t s = (size_t)(ent >> 3);
        const int k = ent & 7;
        const int q = perm_s[k * HW + p];
        const int r = q / W, w = q - r * W;
        const int m = (H - 1 - r) * W + w;
        const unsigned char* cb = codes + s * stride;
        const int code = cb[m];
        const float colour = cb[HW] ? 1.f : 0.f;
        const int opp = code >= 5, age = (code - 1) & 3;
        float* pb = planes_out + (size_t)j * NP * HW;
        if (NP == 9) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const float on = (code && t <= age) ? 1.f : 0.f;
                pb[(6 - 2 * t) * HW + p] = opp ? 0.f : on;
                pb[(7 - 2 * t) * HW + p] = opp ? on : 0.f;
            }
            pb[8 * HW + p] = colour;
        } else {
            pb[0 * HW + p] = (code && !opp) ? 1.f : 0.f;
            pb[1 * HW + p] = (code && opp) ? 1.f : 0.f;
            pb[2 * HW + p] = (code && age == 0) ? 1.f : 0.f;
            pb[3 * HW + p] = colour;
        }
        pi_out[(size_t)j * HW + p] = pi[s * HW + perm_p[k * HW + p]];
        if (p == 0) z_out[j] = z[s];
    }
}

}  // namespace apz
