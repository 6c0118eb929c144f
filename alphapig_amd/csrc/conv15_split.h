// 15x15 boards: 3x3 convolution + folded BatchNorm (+ residual) + ReLU on dense activations [n][C][225] on the FP16 matrix
// pipe at fp32-level accuracy -- every fp32 operand as two fp16 terms (x = hi + lo, both rounded to nearest even), fp32
// accumulation.  The 15x15 sibling of conv8h_kernel (conv8_split.h: the arithmetic, the weight layout and its packer are
// that file's; trunk15_wino3h.h's header has the error bound and the overflow word; the shared code: wino_f16x2.h) for the
// nets that have no Winograd trunk: the simple net, the residual nets of 64 and 256 filters.  gfx950 only.
//
// Work item = (board, 16 output channels); the four waves of a workgroup split the contraction (wave w: input channels
// [w C_in / 4, (w + 1) C_in / 4), in sub-chunks of 16), no workgroup barrier in the main loop, the four partial sums meet
// once in LDS and are added in wave order: a board's bits depend on nothing but the board.  C_in a multiple of 64, C_out
// of 16; there is no transform in front of the split, so inputs up to 65 504 are in range.
//   K = 32 = 16 input channels x the two WEIGHT terms: A = [Whi | Wlo], B = [X | X] for X = lo, then hi (conv8_split.h).
//   A pixel tile of B is one board row: 16 pixels, the sixteenth is padding -- its sums are junk that no thread reads.
//   15 tiles x f32x4 = 60 accumulator registers.
//   LDS tile of a wave, per term: [17 rows -1 .. 15][18 cells -1 .. 16][16 ch] fp16, a cell = one pixel's 16 channels =
//   32 bytes, row stride 576 bytes.  A B fragment is 16 consecutive cells = 512 contiguous bytes: the 16-lane groups a
//   ds_read_b128 is served in cover all 64 banks exactly once, whatever the row stride.  A tile row's fragment serves the
//   three (output row, ky) pairs that meet in it: 3 kx x 17 rows x 2 terms = 102 reads for 270 MFMAs per sub-chunk.
//   Rows -1 and 15 and cells -1, 15 and 16 are zero and nothing in the main loop writes them.
//   Staging: lane = pixel, four passes of 64 (the last: 33 lanes); per pass 16 coalesced dword loads (one per channel)
//   through a buffer descriptor of the board (a lane beyond the board's last plane reads 0, never memory), 8
//   v_cvt_pk_f16_f32 + 16 v_fma_mix, four ds_write_b128 under the lane's own `pixel < 225`.
//   Reduction: every wave writes its 16 x 240 partial sums over its OWN tile area (so the workgroup's 78 336 bytes are
//   all there is: two workgroups per CU), the 256 threads add the four areas in wave order for the 16 x 225 real pixels
//   -- dense planes are 900 bytes, not 16-byte aligned: dword accesses, consecutive threads on consecutive addresses -- and
//   every wave zeroes its area again for the next item.
// Overflow: a non-finite pre-ReLU sum raises flag[0] (a plain vector store); the engine repeats the forward on the fp32
// generic kernel (apz_engine.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "conv8_split.h"
#include "trunk15_wino3h16.h"

namespace apz {

struct Conv15H {
    static constexpr int HW = 225, W = 15;
    static constexpr int CELL = 32, RSB = 18 * CELL;            // bytes: a pixel's 16 channels, a tile row (cells -1 .. 16)
    static constexpr int TERM_BYTES = 17 * RSB;                 // rows -1 .. 15: 9 792
    static constexpr int WAVE_BYTES = 2 * TERM_BYTES;           // hi tile, lo tile
    static constexpr int RED_CS = 244;                          // channel stride of a wave's partial sums (15 x 16 pixels + 4)
    static constexpr int LDS_BYTES = 4 * WAVE_BYTES;            // 78 336: two workgroups per CU
    static_assert(16 * RED_CS * 4 <= WAVE_BYTES, "a wave's partial sums fit its own tile area");
    static_assert(TERM_BYTES % 16 == 0, "the zeroing loop and the staging stores: whole 16-byte slots");
    static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
    static constexpr int PASSES = 4;                            // staging passes of 64 pixels
    static bool supports(int cin, int cout) { return Conv8H::supports(cin, cout); }
    // persistent over items, two workgroups per CU
    static long grid_for(long items, int num_cu) { return items < 2L * num_cu ? items : 2L * num_cu; }
};

// The operator form (apz_conv15h_fwd) has no BatchNorm to fold: pack_conv8h_kernel's scale = 1, shift = the bias (null: 0)
__global__ void conv15h_plain_fold_kernel(const float* __restrict__ bias, double* __restrict__ scale, double* __restrict__ shift,
                                          int cout) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co < cout) {
        scale[co] = 1.0;
        shift[co] = bias ? (double)bias[co] : 0.0;
    }
}

// The training step's data-gradient form (HipTrainer(trunk_arith="f16x2") on the generic 15x15 nets; apz_conv15h_dgrad): the
// same convolution on the flipped, transposed weights (pack_conv15h_many_kernel's second orientation: bias zero), RESID adds
// the skip gradient.  Its input is the gradient of a mean loss, far below 2^-3, where the lo term of the split is subnormal
// and carries an ABSOLUTE error of up to 2^-25.  So the launch scales its input by 2^a, chosen on the
// device exactly as trunk15_wino3h16_kernel<..., WINO3H16_DGRAD> does: `dymax` holds `dymax_n` partial maxima of |input|
// (bn_bwd's dxmax, one per batch split and channel), every workgroup folds them (max: exact in any order; NaN entries are
// ignored), wino3h16_dgrad_exponent puts the maximum into [2^7, 2^8), the staged values are multiplied by 2^a in front of the
// split and 2^-a goes into the 1 / S of the bias FMA (both exact; 2^-a / S may be an fp32 subnormal: this library is built
// with fp32 denormals on).  A +inf maximum raises flag[0]; a zero maximum gives a = 0 and dx = exactly `resid`, or +0.
enum { CONV15H_PLAIN = 0, CONV15H_DGRAD = 1 };

// in: dense [n][cin][225] floats; out / resid: dense [n][cout][225]; pk: Conv8H layout; bias8h: [cout bias][cout 1/S].
// FORM CONV15H_PLAIN (the evaluator's kernel, and with relu = 0 the training step's forward: apz_conv15h_fwd_packed) takes no
// further argument; CONV15H_DGRAD takes (const float* dymax, int dymax_n) behind `flag` and relu = 0: in = dy [n][cin = C of
// dy][225], out = dx, resid = the skip gradient.
template <bool RESID, int FORM = CONV15H_PLAIN, class... AUX>
__global__ __launch_bounds__(256, 2) void conv15h_kernel(const float* __restrict__ in, const void* __restrict__ pk,
                                                         const float* __restrict__ bias8h, const float* __restrict__ resid,
                                                         float* __restrict__ out, int n, int cin, int cout, int relu,
                                                         unsigned* __restrict__ flag, AUX... aux) {
    static_assert(sizeof...(AUX) == (FORM == CONV15H_DGRAD ? 2 : 0), "CONV15H_DGRAD: (dymax, dymax_n); CONV15H_PLAIN: nothing");
    using T = Conv15H;
    extern __shared__ __attribute__((aligned(16))) char lds15[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = lane >> 4, j = lane & 15;
    char* tile = lds15 + wave * T::WAVE_BYTES;                  // [term 2][17 rows][18 cells][16 ch] fp16
    float* red_own = reinterpret_cast<float*>(tile);            // ... and, behind the main loop, [co 16][RED_CS] partial sums

    auto zero_tile = [&]() {       // border cells are never written with anything else in the main loop
        for (int i = lane * 16; i < T::WAVE_BYTES; i += 1024) *reinterpret_cast<f32x4*>(tile + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // DGRAD: the input scale 2^a and 2^-a from the partial maxima (the four wave maxima pass through the first words of the
    // tile memory, which is zeroed only behind the second barrier)
    float xsc = 1.f, xisc = 1.f;
    bool max_inf = false;                           // DGRAD: a partial maximum is +inf -- no scale fits, the result is void
    if constexpr (FORM == CONV15H_DGRAD) {
        const float* dymax;
        int dymax_n;
        [&](const float* p, int c) { dymax = p, dymax_n = c; }(aux...);
        float m = 0.f;
        for (int i = tid; i < dymax_n; i += 256) m = fmaxf(m, fabsf(dymax[i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float* wm = reinterpret_cast<float*>(lds15);
        if (lane == 0) wm[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
        __syncthreads();
        const int a = __builtin_amdgcn_readfirstlane(wino3h16_dgrad_exponent(m));
        max_inf = !(m <= 3.4028234664e38f);
        f16x2_pow2_pair(a, xsc, xisc);
    }
    zero_tile();
    wave_lds_fence();

    const int ncot = cout >> 4, nitems = n * ncot;
    const int nsub_all = cin >> 4, nsub = nsub_all >> 2;        // sub-chunks of 16 channels: in the layer, of this wave
    const int s_lo = wave * nsub;
    // staging role: pass q, lane -> pixel p = 64 q + lane -> cell (p / 15 + 1, p % 15 + 1); ok bit q: p < 225
    int st_cell[T::PASSES];
#pragma unroll
    for (int q = 0; q < T::PASSES; q++) {
        const int p = 64 * q + lane;
        st_cell[q] = (p / T::W + 1) * T::RSB + (p % T::W + 1) * T::CELL;
    }
    const bool st_last = 64 * (T::PASSES - 1) + lane < T::HW;   // the last pass: 33 of 64 lanes
    // B fragment of lane (pixel j of a board row, k group kg): channels 8 (kg & 1) .. + 7
    const int brd = j * T::CELL + (kg & 1) * 16;
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(pk), 0, (unsigned)Conv8H::pk_bytes(cin, cout), 0x00020000);
    const unsigned board_bytes = (unsigned)cin * T::HW * 4u;
    unsigned nonfinite = max_inf ? 1u : 0u;

    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int b = item / ncot, cot = item - b * ncot;
        // the board's input planes: a lane past the last one (pass 3 of the board's last channel) reads 0
        const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in + (size_t)b * cin * T::HW), 0, board_bytes, 0x00020000);
        f32x4 acc[15];
#pragma unroll
        for (int t = 0; t < 15; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float pre[T::PASSES][16];
        auto fetch = [&](int s) {                   // sub-chunk s of this wave: one dword per channel, pass and lane (a pixel)
            const unsigned ch0 = (unsigned)(16 * (s_lo + s)) * (T::HW * 4u);
#pragma unroll
            for (int q = 0; q < T::PASSES; q++)
#pragma unroll
                for (int u = 0; u < 16; u++)
                    pre[q][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_in, (64 * q + lane) * 4, ch0 + u * (T::HW * 4u), 0));
        };
        auto stash = [&]() {                        // split and store: the pixel's 16 channels, hi cell and lo cell
#pragma unroll
            for (int q = 0; q < T::PASSES; q++) {
                u32x4 h[2], l[2];
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    unsigned hu, lu;
                    if constexpr (FORM == CONV15H_DGRAD)
                        f16x2_split(pre[q][2 * m] * xsc, pre[q][2 * m + 1] * xsc, hu, lu);
                    else
                        f16x2_split(pre[q][2 * m], pre[q][2 * m + 1], hu, lu);
                    h[m >> 2][m & 3] = hu;
                    l[m >> 2][m & 3] = lu;
                }
                if (q + 1 < T::PASSES || st_last) {
                    *reinterpret_cast<u32x4*>(tile + st_cell[q]) = h[0];
                    *reinterpret_cast<u32x4*>(tile + st_cell[q] + 16) = h[1];
                    *reinterpret_cast<u32x4*>(tile + T::TERM_BYTES + st_cell[q]) = l[0];
                    *reinterpret_cast<u32x4*>(tile + T::TERM_BYTES + st_cell[q] + 16) = l[1];
                }
            }
        };
        typedef f16x8 WFrag[9];
        WFrag wA, wB;
        auto wload = [&](WFrag& dst, int s) {       // the nine taps of sub-chunk s: one coalesced 1 KB load each
            const unsigned so = (unsigned)((cot * nsub_all + s_lo + s) * 9) * Conv8H::UNIT;
#pragma unroll
            for (int tap = 0; tap < 9; tap++)
                dst[tap] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, lane * 16 + (tap & 3) * Conv8H::UNIT,
                                                                                          so + (unsigned)(tap >> 2) * 4u * Conv8H::UNIT, 0));
        };
        // Tile row R (board row R - 1) and column shift kx: one fragment per term, used by output rows R, R - 1, R - 2 with
        // ky = 0, 1, 2.  The order of the products of an output element is this loop nest's and nothing else's.
        auto compute = [&](const WFrag& w) {
#pragma unroll
            for (int R = 0; R < 17; R++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    const char* bp = tile + brd + R * T::RSB + kx * T::CELL;
                    const f16x8 blo = *reinterpret_cast<const f16x8*>(bp + T::TERM_BYTES);
                    const f16x8 bhi = *reinterpret_cast<const f16x8*>(bp);
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
                        if (R - ky >= 0 && R - ky < 15)
                            acc[R - ky] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ky * 3 + kx], blo, acc[R - ky], 0, 0, 0);
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
                        if (R - ky >= 0 && R - ky < 15)
                            acc[R - ky] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ky * 3 + kx], bhi, acc[R - ky], 0, 0, 0);
                }
        };
        auto turn = [&](const WFrag& w, WFrag& wnext, int s) {     // sub-chunk s from `w`; s + 1 prepared
            if (s + 1 < nsub) {
                fetch(s + 1);
                wload(wnext, s + 1);
            }
            compute(w);
            if (s + 1 < nsub) {
                wave_lds_fence();                   // this wave's reads of the tile are done
                stash();
                wave_lds_fence();
            }
        };
        wload(wA, 0);
        fetch(0);
        stash();
        wave_lds_fence();
        for (int s = 0; s < nsub; s += 2) {
            turn(wA, wB, s);
            if (s + 1 < nsub) turn(wB, wA, s + 1);
        }
        // ---- the four partial sums meet: wave's area [co 16][RED_CS]; lane (kg, j) reg r = co 4 kg + r, pixel 16 t + j
        // (j = 15: the padding pixel's junk, which stays in LDS)
        wave_lds_fence();                           // this wave's reads of its tile are done
#pragma unroll
        for (int t = 0; t < 15; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) red_own[(4 * kg + r) * T::RED_CS + 16 * t + j] = acc[t][r];
        __syncthreads();
        for (int i = tid; i < 16 * T::HW; i += 256) {           // i = co 225 + pixel: consecutive threads, consecutive addresses
            const int co = i / T::HW, p = i - co * T::HW;
            const int y = p / T::W, x = p - y * T::W;
            const float* rp = reinterpret_cast<const float*>(lds15) + co * T::RED_CS + 16 * y + x;
            float sum = rp[0] + rp[T::WAVE_BYTES / 4];
            sum = sum + rp[2 * (T::WAVE_BYTES / 4)];
            sum = sum + rp[3 * (T::WAVE_BYTES / 4)];
            if constexpr (FORM == CONV15H_DGRAD)
                sum = __builtin_fmaf(sum, bias8h[cout + cot * 16 + co] * xisc, bias8h[cot * 16 + co]);
            else
                sum = __builtin_fmaf(sum, bias8h[cout + cot * 16 + co], bias8h[cot * 16 + co]);
            const size_t o = ((size_t)b * cout + cot * 16) * T::HW + i;
            if (RESID) sum = sum + resid[o];
            nonfinite |= ((sum - sum) != 0.f) ? 1u : 0u;        // an overflow of the fp16 split shows as +-inf / NaN here
            if (relu) sum = fmaxf(sum, 0.f);
            out[o] = sum;
        }
        __syncthreads();                            // the reduction's reads are done
        zero_tile();
        wave_lds_fence();
    }
    if (nonfinite && flag) *reinterpret_cast<volatile unsigned*>(flag) = 1u;
}

// The training step's weights, one launch per step: `count` layers of any eligible shape, each in both orientations.
//   orientation 0 (forward)        out channel = co, in channel = ci, tap = ky 3 + kx, bias = the layer's (null: 0) -- bit for
//                                  bit what conv15h_plain_fold_kernel + pack_conv8h_kernel leave
//   orientation 1 (data gradient)  W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]: out channel = ci, in channel = co, bias 0
// S = f16x2_scale_for(max |w|) over the ORIENTATION's own output channel.  Grid (max channels of any layer, 2 count), block
// 256: workgroup (oc, 2 l + o) packs output channel oc of orientation o of layer l, or leaves at once.  flag (may be null)
// is zeroed: the overflow word of the step these weights serve.
struct Conv15HPackEntry {
    const float* w;             // [cout][cin][3][3]
    const float* bias;          // [cout], or null
    unsigned short* pk[2];      // Conv8H layout of (cin -> cout), of (cout -> cin)
    float* bias8h[2];           // [2 cout], [2 cin]
    int cin, cout;
};
__global__ __launch_bounds__(256) void pack_conv15h_many_kernel(const Conv15HPackEntry* __restrict__ tab,
                                                                unsigned* __restrict__ flag) {
    const Conv15HPackEntry E = tab[blockIdx.y >> 1];
    const int flip = blockIdx.y & 1, oc = blockIdx.x, tid = threadIdx.x;
    if (flag && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *flag = 0u;
    const int noc = flip ? E.cin : E.cout, nic = flip ? E.cout : E.cin;
    if (oc >= noc) return;
    auto at = [&](int ic, int tap) -> double {
        return flip ? (double)E.w[((size_t)ic * E.cin + oc) * 9 + (8 - tap)] : (double)E.w[((size_t)oc * E.cin + ic) * 9 + tap];
    };
    double m = 0.0;
    for (int ic = tid; ic < nic; ic += 256)
#pragma unroll
        for (int tap = 0; tap < 9; tap++) m = fmax(m, fabs(at(ic, tap)));
    __shared__ double red[256];
    red[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float S = f16x2_scale_for(red[0]);
    float* b8 = E.bias8h[flip];
    if (tid == 0) {
        b8[oc] = (!flip && E.bias) ? E.bias[oc] : 0.f;
        b8[noc + oc] = 1.f / S;
    }
    unsigned short* pk = E.pk[flip];
    for (int ic = tid; ic < nic; ic += 256)
#pragma unroll
        for (int tap = 0; tap < 9; tap++)
            f16x2_split(at(ic, tap) * (double)S, pk[Conv8H::pk_index(oc, ic, tap, 0, nic)], pk[Conv8H::pk_index(oc, ic, tap, 1, nic)]);
}

}  // namespace apz
