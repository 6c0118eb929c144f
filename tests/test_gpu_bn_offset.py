"""Training-mode BatchNorm on channels with an offset: x[:, c] = sigma_c (randn + r), r = |mean| / std up to 100, on the four
routes to the statistics -- bn_stats_kernel (dense), bn_stats_rows_kernel (padded rows), and the epilogues of the two trunk
convolutions (conv3x3_fwd_stats, conv3x3_fwd_stats_f16x2), where the convolution's bias makes the offset.  Float64 reference
on the CPU from the same float32 tensors; the bars are tests/test_bn_stat_bounds.py's (derived from the arithmetic, u = 2^-24):
flat in r for the routes that square and add in double, (12.5 (1 + r^2) + 2) u of invstd for the per-board fp32 trees.
Up to r = 3 (what the net shows at initialisation) y, dx, dgamma, dbeta, dres keep test_bn_forward_backward's bars unchanged;
beyond, y, dx and dgamma get the first-order propagation of the permitted statistics error through xhat = (x - mean) invstd
on top (_propagation), and the float64 backward pass takes the kernel's own ReLU decisions (an activation within the permitted
error of zero may land on either side).  Backward pass up to r = 30.  Each case prints its worst error / bar."""
import numpy as np
import pytest

from test_bn_stat_bounds import EPS, LADDER, SIGMAS, U, epilogue_bars, offset_channels, own_pass_bars, ref_stats

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

MOM = 0.1


def _pad16(a):
    return F.pad(torch.as_tensor(a), (0, 1)).contiguous()


def _bc(v):
    return v[None, :, None, None]


def _cmax(a):
    return np.abs(a).max(axis=(0, 2, 3))


def _propagation(xhat, ga, i64, rel_bar, mean_bar, dz, dgamma, dx, M):
    """What a statistics error of (rel_bar of invstd, mean_bar of mean) may do to y and dx, to first order, per channel:
    |d xhat| <= mean_bar invstd + max |xhat| rel_bar;  y = gamma xhat + ...: |d y| <= |gamma| |d xhat|;
    dx = gamma invstd (dz - k0 - xhat k1), k1 = mean(dz xhat): |d k1| <= |d xhat| mean |dz|."""
    dxh = mean_bar * i64 + _cmax(xhat) * rel_bar
    prop_y = np.abs(ga) * dxh
    if dz is None:
        return prop_y, None
    k1 = np.abs(dgamma) / M
    prop_dx = rel_bar * _cmax(dx) + np.abs(ga) * i64 * (dxh * k1 + _cmax(xhat) * dxh * np.abs(dz).mean(axis=(0, 2, 3)))
    return prop_y, prop_dx


def _run(x, layout, bars, r, g, stats=None, label=""):
    """x: float32 CPU tensor [n][c][15][15] (dense values) or, with stats, the convolution's padded-row device output.
    BatchNorm + residual + ReLU forward and backward on the kernels against float64; -> worst error / bar of (invstd, mean)."""
    from alphapig_amd import hipconv
    if stats is None:
        xc = (_pad16(x) if layout == 1 else x).cuda()
        x64 = x.double().numpy()
    else:
        xc = x
        x64 = x[..., :15].double().cpu().numpy()
    n, c = x64.shape[:2]
    M = n * 225.0
    res = torch.randn(n, c, 15, 15, generator=g)
    ga = torch.rand(c, generator=g) + 0.5
    be = torch.randn(c, generator=g) * 0.2
    dy = torch.randn(n, c, 15, 15, generator=g)
    pad = _pad16 if layout == 1 else (lambda t: t)
    cut = (lambda t: t[..., :15]) if layout == 1 else (lambda t: t)
    rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
    rc, dyc, gc, bc = pad(res).cuda(), pad(dy).cuda(), ga.cuda(), be.cuda()
    y, mean, invstd = hipconv.bn_fwd(xc, gc, bc, rm, rv, rc, True, layout, MOM, EPS, stats=stats)
    back = r <= 30
    if back:
        dx, dres, dgamma, dbeta = hipconv.bn_bwd(dyc, xc, y, gc, mean, invstd, True, True, layout)
    torch.cuda.synchronize()
    host = lambda t: t.double().cpu().numpy()

    # ---- statistics
    m64, v64 = ref_stats(x64)
    i64 = 1.0 / np.sqrt(v64 + EPS)
    rel_bar, mean_bar, var_bar = bars(m64, v64)
    e_i = np.abs(host(invstd) - i64) / i64 / rel_bar
    e_m = np.abs(host(mean) - m64) / mean_bar
    print("%s r = %g: worst error / bar  invstd %.3f  mean %.3f" % (label, r, e_i.max(), e_m.max()))
    assert e_i.max() <= 1.0, (r, float(e_i.max()), int(e_i.argmax()))
    assert e_m.max() <= 1.0, (r, float(e_m.max()), int(e_m.argmax()))
    # moving statistics after one update from (0, 1): the same bars times the momentum, and the update's own float32
    # arithmetic (momentum and 1 - momentum as floats; two products and a sum: 3 u of the terms)
    mom, keep = float(np.float32(MOM)), float(np.float32(1) - np.float32(MOM))
    unb = v64 * M / (M - 1.0)
    rm64, rv64 = mom * m64, keep * 1.0 + mom * unb
    assert np.all(np.abs(host(rm) - rm64) <= mom * mean_bar + 3 * U * np.abs(rm64))
    assert np.all(np.abs(host(rv) - rv64) <= mom * var_bar * M / (M - 1.0) + 3 * U * (keep + mom * unb))

    # ---- y
    ga64, be64 = ga.double().numpy(), be.double().numpy()
    xhat = (x64 - _bc(m64)) * _bc(i64)
    y64 = np.maximum(_bc(ga64) * xhat + _bc(be64) + res.double().numpy(), 0.0)
    yk = host(cut(y))
    if layout == 1:
        assert float(y[..., 15].abs().max()) == 0.0
    if back:
        mask = (y64 > 0) if r <= 3 else (yk > 0)
        dz = dy.double().numpy() * mask
        dbeta64 = dz.sum(axis=(0, 2, 3))
        dgamma64 = (dz * xhat).sum(axis=(0, 2, 3))
        dx64 = _bc(ga64 * i64) * (dz - _bc(dbeta64 / M) - xhat * _bc(dgamma64 / M))
    prop_y, prop_dx = _propagation(xhat, ga64, i64, rel_bar, mean_bar, dz if back else None, dgamma64 if back else None,
                                   dx64 if back else None, M)
    if r <= 3:
        prop_y = np.zeros_like(prop_y)
        prop_dx = np.zeros_like(prop_y)
    elif layout == 1:        # bn_apply_rows_kernel folds the shift: y = x sc + (beta - mean sc)
        fold = 2 * U * np.abs(ga64) * np.abs(m64) / np.sqrt(v64)
        prop_y = prop_y + fold
        prop_dx = None if prop_dx is None else prop_dx + fold
    over = lambda a, b, prop: float((np.abs(a - b) - _bc(prop)).max())
    assert over(yk, y64, prop_y) < 1e-5 * (np.abs(y64).max() + 1e-3)
    if not back:
        return float(e_i.max()), float(e_m.max())

    # ---- backward
    if layout == 1:
        assert float(dx[..., 15].abs().max()) == 0.0
    close = lambda a, b, t: float(np.abs(a - b).max()) < t * (float(np.abs(b).max()) + 1e-3)
    assert over(host(cut(dx)), dx64, prop_dx) < 1e-4 * (np.abs(dx64).max() + 1e-3)
    assert close(host(dbeta), dbeta64, 1e-5)
    # dgamma = sum dz xhat sees the statistics error too: xhat' = xhat (1 + rho) - d mean invstd, so beyond r = 3
    # |d dgamma| <= rel_bar |dgamma| + mean_bar invstd |dbeta| on top of the existing bar (dbeta and dres do not depend on them)
    prop_dg = np.zeros_like(dgamma64) if r <= 3 else rel_bar * np.abs(dgamma64) + mean_bar * i64 * np.abs(dbeta64)
    assert float((np.abs(host(dgamma) - dgamma64) - prop_dg).max()) < 1e-5 * (float(np.abs(dgamma64).max()) + 1e-3)
    assert close(host(cut(dres)), dz, 1e-6)
    return float(e_i.max()), float(e_m.max())


@pytest.mark.parametrize("r", LADDER)
@pytest.mark.parametrize("layout,n,c", [(0, 7, 128), (0, 7, 4), (1, 9, 128)])
def test_own_statistics_pass(layout, n, c, r):
    """bn_stats_kernel / bn_stats_rows_kernel (9 boards: three splits, the last trip of four boards holds one): sums and
    squares in double, so invstd to 4 u and the mean to 2 u whatever the offset."""
    from alphapig_amd import hipconv
    x = torch.from_numpy(offset_channels(np.random.RandomState(100 * r + 10 * layout + c), n, c, r))
    if layout == 1:
        assert hipconv.bn_bwd_splits(_pad16(x).cuda(), layout) > 1
    g = torch.Generator().manual_seed(500 + r + c + layout)
    _run(x, layout, own_pass_bars, r, g, label="own pass, layout %d, c %d," % (layout, c))


@pytest.fixture(scope="module")
def conv_problem():
    """x, w (output channel co scaled by sigma_co) and, from a first float64 pass, the standard deviation of every output
    channel without bias"""
    g = torch.Generator().manual_seed(77)
    n = 9
    x = torch.randn(n, 128, 15, 15, generator=g)
    sig = torch.tensor([SIGMAS[i % 3] for i in range(128)])
    w = (torch.randn(128, 128, 3, 3, generator=g) / 34.0 * sig[:, None, None, None]).float()
    y0 = F.conv2d(x.double(), w.double(), None, padding=1)
    return x, w, y0.std(dim=(0, 2, 3), unbiased=False).float()


@pytest.mark.parametrize("r", LADDER)
@pytest.mark.parametrize("route", ["f32", "f16x2"])
def test_statistics_from_the_convolution_epilogue(conv_problem, route, r):
    """bias b_c = r std_c: the convolution's output has the offset, its epilogue the per-board fp32 sums; BatchNorm from them
    against float64 statistics of the kernel's own y."""
    from alphapig_amd import hipconv
    x, w, std = conv_problem
    b = (std * float(r)).float()
    xc, wc, bc = _pad16(x).cuda(), w.cuda(), b.cuda()
    if route == "f32":
        y, st = hipconv.conv3x3_fwd_stats(xc, wc, bc)
    else:
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        u, bb = hipconv.wino3h_pack_many(wc[None].contiguous(), bc[None].contiguous())
        y, st = hipconv.conv3x3_fwd_stats_f16x2(xc, u[0, 0], bb[0, 0], flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
    g = torch.Generator().manual_seed(900 + r)
    _run(y, 1, epilogue_bars, r, g, stats=st, label="epilogue %s," % route)
