// Square boards of side S < 15 on the 15x15 trunk kernels ("framed" engines, S = 6 .. 14 except 8 and 10).
//
// A board of side S is a 15x15 frame whose cells outside the top-left S x S window are not there: plane row r is frame
// row r, plane column c is frame column c.  A 3x3 convolution with zero padding on the S x S board equals the same
// convolution on the frame, cropped, provided the off-board cells of its INPUT are zero.  The trunk kernels work on
// rows16 tensors [n][128][15][16] and write whole planes, so every layer leaves bias-and-neighbour values in the
// off-board cells; frame_clear_kernel zeroes them before the next layer reads them.
//
// The invariant: after every layer but the last (whose consumers, the heads, read on-board cells only), every
// off-board cell of the activation is exactly +0.  A board's outputs, the f16x2 overflow word and the maxima a
// calibration measures are therefore functions of on-board data and weights only -- not of what the buffers held
// before, nor of the board's place in the batch.
//
// The overflow word gains no new cause: the f16x2 kernels raise it for a non-finite pre-ReLU output, which takes an
// input beyond the fp16 range.  Off-board inputs are zero, and an off-board output is the bias plus a sum over fewer
// (on-board) neighbours than an on-board cell has: finite whenever the on-board ones are.
//
//  frame_encode_kernel   position codes [n][code_stride(S)] -> framed planes [n][NP][15][15]; on-board values are those
//                        of encode_planes_kernel (heads.h) at that size, every off-board cell of every plane is zero --
//                        the colour plane included ("all ones" must not leak past the board's edge)
//  frame_planes_kernel   dense planes [n][NP][S][S] (the planes entry points) -> the same framed layout
//  frame_clear_kernel    zeroes the off-board cells of a rows16 tensor: rows S..14 whole, columns S..15 of rows 0..S-1.
//                        Write-only, no atomics, idempotent; 16-byte stores except for the piece the board's edge cuts.
// S is a runtime argument: one code object per kernel serves every size.
#pragma once
#include <hip/hip_runtime.h>

#include "conv3x3_mfma.h"

namespace apz {

struct Frame15 {
    static constexpr int SIDE = 15, CELLS = 225;     // the frame of the planes
    static constexpr int GROW = 16, GPLANE = 240;    // rows16 activations (Trunk15::GROW / GPLANE)
    // 8x8 has kernels of its own.  10x10 stays refused as it always was: tests/test_gpu_net.py holds the evaluator to
    // refusing that board (its example of an unsupported size); nothing in the kernels sets it apart -- `s != 10` and
    // that case go together.
    static constexpr bool framed_side(int s) { return s >= 6 && s <= 14 && s != 8 && s != 10; }
    // off-board work items of one rows16 plane: 16-byte pieces of rows S..14, then the pieces of rows 0..S-1 at or
    // beyond column S (the first of them cut by the edge when S is no multiple of 4)
    static constexpr int pieces_per_row(int s) { return 4 - s / 4; }
    static constexpr int clear_items(int s) { return (SIDE - s) * 4 + s * pieces_per_row(s); }
};

static_assert(Frame15::clear_items(6) == 54 && Frame15::clear_items(7) <= 64 && Frame15::clear_items(14) == 18,
              "frame_clear_kernel: one lane per off-board work item of a plane (the count falls as S grows)");

__global__ __launch_bounds__(256) void frame_encode_kernel(const unsigned char* __restrict__ codes, float* __restrict__ planes,
                                                           int n, int S, int stride, int NP) {
    constexpr int CELLS = Frame15::CELLS;
    const long total = (long)n * CELLS;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / CELLS), m = (int)(i - (long)b * CELLS);
        const int r = m / 15, c = m - r * 15;
        const bool on_board = r < S && c < S;
        const unsigned char* cb = codes + (size_t)b * stride;
        // frame row r is plane row r: the vertical flip of game.py:94 puts board row S - 1 - r there
        const int code = on_board ? cb[(S - 1 - r) * S + c] : 0;
        const float colour = (on_board && cb[S * S]) ? 1.f : 0.f;
        float* pb = planes + (size_t)b * NP * CELLS + m;
        const int opp = code >= 5, age = (code - 1) & 3;
        if (NP == 9) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float on = (code && k <= age) ? 1.f : 0.f;
                pb[(6 - 2 * k) * CELLS] = opp ? 0.f : on;
                pb[(7 - 2 * k) * CELLS] = opp ? on : 0.f;
            }
            pb[8 * CELLS] = colour;
        } else {
            pb[0 * CELLS] = (code && !opp) ? 1.f : 0.f;
            pb[1 * CELLS] = (code && opp) ? 1.f : 0.f;
            pb[2 * CELLS] = (code && age == 0) ? 1.f : 0.f;
            pb[3 * CELLS] = colour;
        }
    }
}

// planes_in [nplanes][S][S] -> planes_out [nplanes][15][15]
__global__ __launch_bounds__(256) void frame_planes_kernel(const float* __restrict__ planes_in, float* __restrict__ planes_out,
                                                           long nplanes, int S) {
    constexpr int CELLS = Frame15::CELLS;
    const long total = nplanes * CELLS;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long p = i / CELLS;
        const int m = (int)(i - p * CELLS);
        const int r = m / 15, c = m - r * 15;
        planes_out[i] = (r < S && c < S) ? planes_in[p * (S * S) + r * S + c] : 0.f;
    }
}

// act [nplanes][15][16].  One wavefront per plane, lane = work item (at most 54 of them, at S = 6), 32-bit index arithmetic.
// A row of a rows16 plane is one 64-byte line and every row has off-board cells (rows 0..S-1 from column S on, S <= 14), so
// the pass touches every line of the tensor: measured at 512 boards it costs 13 - 18 us per layer, about what writing the
// whole 63 MB would, whatever the index arithmetic (profiles/r16_frame_boards.md).  A mask fused into the trunk kernels'
// epilogues would remove it; this pass then stays as its cross-check.
__global__ __launch_bounds__(256) void frame_clear_kernel(float* __restrict__ act, long nplanes, int S) {
    const int above = (Frame15::SIDE - S) * 4, ppr = Frame15::pieces_per_row(S), items = Frame15::clear_items(S);
    const int it = threadIdx.x & 63;
    if (it >= items) return;
    for (long p = blockIdx.x * 4L + (threadIdx.x >> 6); p < nplanes; p += gridDim.x * 4L) {
        int row, piece;
        if (it < above) {                       // rows S..14: all four pieces
            row = S + (it >> 2);
            piece = it & 3;
        } else {                                // rows 0..S-1: the pieces that reach column S or beyond
            const int k = it - above;
            row = k / ppr;
            piece = S / 4 + (k - row * ppr);
        }
        float* dst = act + p * Frame15::GPLANE + row * Frame15::GROW + piece * 4;
        if (row >= S || piece * 4 >= S) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {                                // the piece the board's right edge cuts: its on-board columns stay
            for (int c = S - piece * 4; c < 4; c++) dst[c] = 0.f;
        }
    }
}

}  // namespace apz
