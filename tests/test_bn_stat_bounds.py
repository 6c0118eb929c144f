"""The error envelope of the BatchNorm statistics that the trunk convolutions leave in their epilogue (trunk15_wino3_kernel
<STATS>, WINO3H16_STATS): per board a fixed fp32 tree over the 225 values and their squares, double sums across boards.

The bars (u = 2^-24, r = |mean| / std of the channel) come from the arithmetic: the tree has at most 8 additions over a
term and one product rounding per square, and a sum of squares has no cancellation, so |d var| <= 25 u (std^2 + mean^2);
with invstd = (var + eps)^-1/2 that is |d invstd| / invstd <= 12.5 u (1 + r^2) (+ 2 u: the final roundings), and
|d mean| <= 9 u sqrt(std^2 + mean^2).  This module holds the bars (tests/test_gpu_bn_offset.py asserts them of the
kernels) and checks on the CPU that a numpy restatement of the tree stays inside them over the offset ladder."""
import numpy as np
import pytest

U = 2.0 ** -24
LADDER = (0, 3, 10, 30, 100)
SIGMAS = (0.05, 1.0, 20.0)
EPS = float(np.float32(1e-3))      # the operator takes a float


def ref_stats(x64):
    """x64 [n][C][15][15] float64 -> (mean, biased variance) per channel, two passes"""
    m = x64.mean(axis=(0, 2, 3))
    v = ((x64 - m[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
    return m, v


def own_pass_bars(mean, var, eps=EPS):
    """-> (relative bar of invstd, absolute bar of mean, absolute bar of var) for a statistics pass that squares and adds
    in double: flat in r.  (var: the invstd bar read backwards, d var = 2 (var + eps) d invstd / invstd.)"""
    rel = np.full_like(mean, 4 * U)
    return rel, 2 * U * np.abs(mean) + 1e-30, 2 * rel * (var + eps)


def epilogue_bars(mean, var, eps=EPS):
    """the same three for the per-board fp32 tree"""
    r2 = mean * mean / var
    return (12.5 * (1 + r2) + 2) * U, 9 * U * np.sqrt(var + mean * mean), 25 * U * (var + mean * mean)


def board_tree_f32(x):
    """x [..., 15, 15] float32 -> the board sums of the convolution epilogue in float32: a lane's 4x4 tile row by row
    ((v0 + v1) + (v2 + v3)), its four rows the same way, then the board's 16 tiles as a butterfly; row and column 15 are zero"""
    p = np.zeros(x.shape[:-2] + (16, 16), dtype=np.float32)
    p[..., :15, :15] = x
    t = p.reshape(x.shape[:-2] + (4, 4, 4, 4))                    # [tile row][row in tile][tile col][col in tile]
    rows = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])      # [ty][a][tx]
    tiles = (rows[..., 0, :] + rows[..., 1, :]) + (rows[..., 2, :] + rows[..., 3, :])   # [ty][tx]
    s = tiles.reshape(x.shape[:-2] + (16,))
    for half in (8, 4, 2, 1):
        s = s[..., :half] + s[..., half:2 * half]
    assert s.dtype == np.float32
    return s[..., 0]


def emulated_stats(x):
    """x [n][C][15][15] float32 -> (mean, biased var) float64 as bn_apply derives them from the per-board sums"""
    M = x.shape[0] * 225.0
    s1 = board_tree_f32(x).astype(np.float64).sum(axis=0)
    s2 = board_tree_f32(x * x).astype(np.float64).sum(axis=0)
    m = s1 / M
    return m, np.maximum(s2 / M - m * m, 0.0)


def offset_channels(rs, n, c, r):
    """x[:, ch] = sigma_ch (randn + r), sigma cycling through SIGMAS -> float32 [n][c][15][15]"""
    sig = np.array([SIGMAS[i % 3] for i in range(c)], dtype=np.float64)
    return (sig[None, :, None, None] * (rs.standard_normal((n, c, 15, 15)) + r)).astype(np.float32)


@pytest.mark.parametrize("r", LADDER)
def test_the_per_board_fp32_tree_stays_inside_the_epilogue_bar(r):
    worst = [0.0, 0.0, 0.0]
    for seed in range(20):
        x = offset_channels(np.random.RandomState(1000 * r + seed), 9, 6, r)
        m64, v64 = ref_stats(x.astype(np.float64))
        m, v = emulated_stats(x)
        rel_bar, mean_bar, var_bar = epilogue_bars(m64, v64)
        i64 = 1.0 / np.sqrt(v64 + EPS)
        invstd = (1.0 / np.sqrt(v + EPS)).astype(np.float32).astype(np.float64)
        mean = m.astype(np.float32).astype(np.float64)
        ratios = (np.abs(invstd - i64) / i64 / rel_bar, np.abs(mean - m64) / mean_bar, np.abs(v - v64) / var_bar)
        worst = [max(w, float(q.max())) for w, q in zip(worst, ratios)]
    print("r = %g: worst error / bar  invstd %.3f  mean %.3f  var %.3f" % ((r,) + tuple(worst)))
    assert max(worst) <= 1.0, worst
