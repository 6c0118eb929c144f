// BatchNorm folding and weight packing, the one implementation: every evaluator weight goes through these kernels
// (double arithmetic, rounded once).  apz_load_weights stages the host tensors in device memory and runs them;
// apz_load_weights_dev runs them on tensors that already live there -- the trainer's after an optimiser step
// (policy_value_net_mxnet.py:295-297: the reference copies the new parameters into its predict modules after every
// step), a few tens of microseconds.  The kernels write the value slots of a layout only: the pad slots (taps 9..11 of
// the [12] forms, 18..19 of upk2's [20], what WinoPackSmall::index leaves out) are zero from the allocation
// (apz_engine.hip, alloc_packed).  gfx950.
#pragma once
#include "trunk15_wino3b.h"
#include "trunk15_wino3h16.h"
#include "wino_f16x2.h"
#include <hip/hip_runtime.h>

namespace apz {

// scale[o] = gamma[o] / sqrt(var[o] + eps) (gamma == nullptr: 1), shift[o] = (bias[o] - mean[o]) * scale[o] + beta[o]
__global__ void fold_bn_kernel(const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ mean, const float* __restrict__ var, double* __restrict__ scale,
                               double* __restrict__ shift, float* __restrict__ bias_out, int cout, double eps) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= cout) return;
    const double g = gamma ? (double)gamma[o] : 1.0;
    const double s = g / sqrt((double)var[o] + eps);
    const double sh = ((double)bias[o] - (double)mean[o]) * s + (double)beta[o];
    scale[o] = s;
    shift[o] = sh;
    if (bias_out) bias_out[o] = (float)sh;
}

// direct-convolution fragments: X4 ? [cot][c4][lane][12] : [cot][c4][tap][lane]; element = w[co][ci][tap] * scale[co]
__global__ void pack_direct_kernel(const float* __restrict__ w, const double* __restrict__ scale, float* __restrict__ pk, int cin,
                                   int n4, int ncot, int x4) {
    const int total = ncot * n4 * 9 * 64;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int lane = i & 63, tap = (i >> 6) % 9, c4 = (i / (64 * 9)) % n4, cot = i / (64 * 9 * n4);
        const int co = cot * 16 + (lane & 15), ci = c4 * 4 + (lane >> 4);
        float v = 0.f;
        if (ci < cin) v = (float)((double)w[((size_t)co * cin + ci) * 9 + tap] * scale[co]);
        if (x4)
            pk[(((size_t)cot * n4 + c4) * 64 + lane) * 12 + tap] = v;
        else
            pk[(((size_t)cot * n4 + c4) * 9 + tap) * 64 + lane] = v;
    }
}

// the 3x3 kernel (co, ci) of the 128 -> 128 trunk shape with the BatchNorm scale folded in
__device__ __forceinline__ void folded_kernel(const float* __restrict__ w, const double* __restrict__ scale, int co, int ci,
                                              double (&g)[3][3]) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g[a][b] = (double)w[((size_t)co * 128 + ci) * 9 + a * 3 + b] * scale[co];
}

// F(4x4,3x3) Winograd weights of one 3x3 kernel g: u[6i+k] = (G g G^T)[i][k] in double (t = G g first, then t G^T) -- the
// one copy every packer below rounds from
__device__ __forceinline__ void wino_u_of(const double (&g)[3][3], double (&u)[36]) {
    const double G[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double t[6][3];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int b = 0; b < 3; b++) t[i][b] = G[i][0] * g[0][b] + G[i][1] * g[1][b] + G[i][2] * g[2][b];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k < 6; k++) u[6 * i + k] = t[i][0] * G[k][0] + t[i][1] * G[k][1] + t[i][2] * G[k][2];
}

// U of the folded 128 -> 128 trunk layer, rounded once, in trunk15_wino3.h's layout (wino_common.h: [cot 8][row half 2]
// [c4 32][lane 64][20]) and, up3s != NULL, in trunk15_wino3s.h's (WinoPackSmall).  One thread per (co, ci).
__global__ void pack_wino_folded_kernel(const float* __restrict__ w, const double* __restrict__ scale, float* __restrict__ up2,
                                        float* __restrict__ up3s) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 128 * 128) return;
    const int co = idx >> 7, ci = idx & 127;
    double g[3][3], u[36];
    folded_kernel(w, scale, co, ci, g);
    wino_u_of(g, u);
    const int cot = co >> 4, jj = co & 15;
    const int qq = ci & 3, c4 = ci >> 2;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int pass = i / 3;
            up2[((((size_t)cot * 2 + pass) * 32 + c4) * 64 + (qq * 16 + jj)) * 20 + (i - 3 * pass) * 6 + k] = (float)u[6 * i + k];
            if (up3s) up3s[WinoPackSmall::index(co, ci, 6 * i + k)] = (float)u[6 * i + k];
        }
}

// The same U as three bf16 terms for trunk15_wino3b.h (Wino3B::upk_offset): round to nearest even, remainders in double.
__global__ void pack_wino3b_folded_kernel(const float* __restrict__ w, const double* __restrict__ scale, unsigned short* __restrict__ up) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 128 * 128) return;
    const int co = idx >> 7, ci = idx & 127;
    double g[3][3], u[36];
    folded_kernel(w, scale, co, ci, g);
    wino_u_of(g, u);
#pragma unroll
    for (int pos = 0; pos < 36; pos++) {
        double rem = u[pos];
#pragma unroll
        for (int term = 0; term < 3; term++) {
            unsigned b = __builtin_bit_cast(unsigned, (float)rem);
            if ((b & 0x7f800000u) != 0x7f800000u) b += 0x7fffu + ((b >> 16) & 1u);
            b &= 0xffff0000u;
            up[Wino3B::upk_offset(co, ci, pos, term) / 2] = (unsigned short)(b >> 16);
            rem -= (double)__builtin_bit_cast(float, b);
        }
    }
}

// The U of kernel g (one output channel co, thread = input channel ci of a 128-thread workgroup) for the fp16 x 2 kernels:
// max |U| of the channel over the workgroup, S = f16x2_scale_for(max), U S as two fp16 terms (both round to nearest even,
// the remainder in double) at L::upk_offset; bias3h[co] = bias, bias3h[128 + co] = 1 / S
template <class L>
__device__ __forceinline__ void pack_wino3h_channel(const double (&g)[3][3], int co, int ci, double bias, unsigned short* __restrict__ up,
                                                    float* __restrict__ bias3h) {
    double u[36];
    wino_u_of(g, u);
    double m = 0.0;
#pragma unroll
    for (int pos = 0; pos < 36; pos++) m = fmax(m, fabs(u[pos]));
    __shared__ double red[128];
    red[ci] = m;
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (ci < s) red[ci] = fmax(red[ci], red[ci + s]);
        __syncthreads();
    }
    const float S = f16x2_scale_for(red[0]);
    if (ci == 0) {
        bias3h[co] = (float)bias;
        bias3h[128 + co] = 1.f / S;
    }
#pragma unroll
    for (int pos = 0; pos < 36; pos++) {
        unsigned short hb, lb;
        f16x2_split(u[pos] * (double)S, hb, lb);
        up[L::upk_offset(co, ci, pos, 0) / 2] = hb;
        up[L::upk_offset(co, ci, pos, 1) / 2] = lb;
    }
}

// The same U for trunk15_wino3h.h: one workgroup per output channel (thread = input channel), the BatchNorm folded in
// (L = Wino3H, or Wino3H16 of trunk15_wino3h16.h); bias3h = [128 folded biases][128 x 1 / S].  Launch: grid 128, block 128.
template <class L>
__global__ void pack_wino3h_folded_kernel(const float* __restrict__ w, const double* __restrict__ scale, const double* __restrict__ shift,
                                          unsigned short* __restrict__ up, float* __restrict__ bias3h) {
    const int co = blockIdx.x, ci = threadIdx.x;
    double g[3][3];
    folded_kernel(w, scale, co, ci, g);
    pack_wino3h_channel<L>(g, co, ci, shift[co], up, bias3h);
}

// The training step's weights for trunk15_wino3h16_train_kernel, no BatchNorm fold: `count` layers whose fp32 weights sit
// back to back ([count][128][128][3][3]), each for the forward (bias b[layer], may be NULL: zero) and the data gradient
// (W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx], bias zero; S per output channel of W', i.e. per input channel of the forward),
// in one launch: up [count][2][UPK_BYTES], bias3h [count][2][256].  flag (may be NULL) is zeroed: the overflow word of the
// step these weights serve.  Launch: grid (128, 2 count), block 128.
__global__ void pack_wino3h16_many_kernel(const float* __restrict__ w, const float* __restrict__ b, unsigned short* __restrict__ up,
                                          float* __restrict__ bias3h, unsigned* __restrict__ flag) {
    const int co = blockIdx.x, ci = threadIdx.x, layer = blockIdx.y >> 1, flip = blockIdx.y & 1;
    const float* wl = w + (size_t)layer * (128 * 128 * 9);
    double g[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            g[a][c] = flip ? (double)wl[((size_t)ci * 128 + co) * 9 + (2 - a) * 3 + (2 - c)] : (double)wl[((size_t)co * 128 + ci) * 9 + a * 3 + c];
    const double bias = (!flip && b) ? (double)b[(size_t)layer * 128 + co] : 0.0;
    pack_wino3h_channel<Wino3H16>(g, co, ci, bias, up + (size_t)blockIdx.y * (Wino3H16::UPK_BYTES / 2),
                                  bias3h + (size_t)blockIdx.y * Wino3H16::BIAS_FLOATS);
    if (flag && blockIdx.x == 0 && blockIdx.y == 0 && ci == 0) *flag = 0u;
}

// heads: rows [row0, row0 + rows) of the [6][C] matrix of both 1x1 convolutions, and their folded biases
__global__ void pack_head_conv_kernel(const float* __restrict__ w, const double* __restrict__ scale, const double* __restrict__ shift,
                                      float* __restrict__ w6, float* __restrict__ b6, int rows, int row0, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * C) {
        const int o = i / C;
        w6[(size_t)row0 * C + i] = (float)((double)w[i] * scale[o]);
    }
    if (i < rows) b6[row0 + i] = (float)shift[i];
}

// policy FullyConnected [hw][4 hw] -> head_fc_kernel's [tile][trip of 8 k-steps][lane][8] (zero past hw outputs / KS steps)
__global__ void pack_fc_kernel(const float* __restrict__ wfc, float* __restrict__ pk, int hw, int ntile, int KG) {
    const int K = 4 * hw, KS = hw;
    const long total = (long)ntile * KG * 64 * 8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int u = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const long r = i >> 9;
        const int trip = (int)(r % KG), nt = (int)(r / KG);
        const int s = trip * 8 + u, o = nt * 16 + (lane & 15), k = 4 * s + (lane >> 4);
        pk[i] = (s < KS && o < hw) ? wfc[(size_t)o * K + k] : 0.f;
    }
}

}  // namespace apz
