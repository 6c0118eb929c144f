"""The host paths that the whole-board and the framed training operators share (apz_engine.hip: one padded-row BatchNorm
path, one 1x1 forward and one paired backward on a geometry value): every pair of entry points that must launch the same
kernels on the same geometry gives the same bytes, and every refusal keeps its code and its text."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DENSE, R = 0, 1          # hipconv.DENSE, hipconv.ROWS16
E_ARG, E_UNSUPPORTED = -1, -4
BAD = "bad argument"
SIDE = "%s: side must be 6, 7, 9, 11, 12, 13, 14 or 15"


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def _rows(n, c, g):
    """padded rows [n][c][15][16], the pad column zero"""
    x = torch.randn(n, c, 15, 16, generator=g) * 1.3 + 0.2
    x[..., 15] = 0
    return x.cuda()


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("n", [1, 5])
def test_conv1x1_forward_side_15_is_the_plain_call(n):
    from alphapig_amd import hipconv
    g = torch.Generator().manual_seed(410 + n)
    x = _rows(n, 128, g)
    for co in (4, 2):
        w, b = (torch.randn(co, 128, 1, 1, generator=g) / 11).cuda(), torch.randn(co, generator=g).cuda()
        plain, framed = hipconv.conv1x1_fwd(x, w, b, R), hipconv.conv1x1_fwd(x, w, b, R, side=15)
        torch.cuda.synchronize()
        assert tuple(plain.shape) == (n, co, 15, 15) and _same(plain, framed), co


@pytest.mark.parametrize("n", [1, 5])
def test_conv1x1_pair_backward_side_15_is_the_plain_call(n):
    from alphapig_amd import hipconv
    g = torch.Generator().manual_seed(420 + n)
    x = _rows(n, 128, g)
    w1, w2 = (torch.randn(4, 128, 1, 1, generator=g) / 11).cuda(), (torch.randn(2, 128, 1, 1, generator=g) / 11).cuda()
    dy1, dy2 = torch.randn(n, 4, 15, 15, generator=g).cuda(), torch.randn(n, 2, 15, 15, generator=g).cuda()
    plain = hipconv.conv1x1_bwd_pair(x, w1, dy1, w2, dy2, R)
    framed = hipconv.conv1x1_bwd_pair(x, w1, dy1, w2, dy2, R, side=15)
    torch.cuda.synchronize()
    assert _same(plain[0][..., :15, :], framed[0][..., :15, :])           # dx: rows 0 .. 14 of every plane
    for i, name in ((1, "dw1"), (2, "db1"), (3, "dw2"), (4, "db2")):
        assert _same(plain[i], framed[i]), name


def _bn_case(n, layout, g):
    """-> (board, c, x, resid, dy, gamma, beta): the dense layout on an 8x8 engine with 64 channels"""
    if layout == R:
        board, c = (15, 15), 128
        x, r, dy = _rows(n, c, g), _rows(n, c, g), _rows(n, c, g)
    else:
        board, c = (8, 8), 64
        x, r, dy = (torch.randn(n, c, 8, 8, generator=g).cuda() for _ in range(3))
    return board, c, x, r, dy, (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.2).cuda()


@pytest.mark.parametrize("layout", [R, DENSE])
@pytest.mark.parametrize("n", [1, 5])
def test_bn_forward_wrapper_is_the_stats_entry_without_stats_and_mask(n, layout):
    from alphapig_amd import hipconv
    board, c, x, r, _, ga, be = _bn_case(n, layout, torch.Generator().manual_seed(430 + 2 * n + layout))
    L, hnd, stream = hipconv._ctx(x, board)
    outs = []
    for stats_entry in (False, True):
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
        y, mean, invstd = torch.empty_like(x), torch.empty(c).cuda(), torch.empty(c).cuda()
        head = (hnd, _p(x), _p(r), _p(ga), _p(be), _p(rm), _p(rv), _p(y), _p(mean), _p(invstd))
        tail = (n, c, layout, 1, 0.1, 1e-3, stream)
        rc = L.apz_bn_fwd_stats(*head, None, None, *tail) if stats_entry else L.apz_bn_fwd(*head, *tail)
        assert rc == 0, L.apz_last_error().decode()
        torch.cuda.synchronize()
        outs.append((y, mean, invstd, rm, rv))
    for i, (a, b) in enumerate(zip(*outs)):
        assert _same(a, b), i


@pytest.mark.parametrize("layout", [R, DENSE])
@pytest.mark.parametrize("n", [1, 5])
def test_bn_backward_wrapper_is_the_max_entry_without_dxmax(n, layout):
    from alphapig_amd import hipconv
    board, c, x, r, dy, ga, be = _bn_case(n, layout, torch.Generator().manual_seed(440 + 2 * n + layout))
    y, mean, invstd = hipconv.bn_fwd(x, ga, be, None, None, r, True, layout, 0.1, 1e-3)
    L, hnd, stream = hipconv._ctx(x, board)
    splits = hipconv.bn_bwd_splits(x, layout)
    outs = []
    for max_entry in (False, True):
        dx, dres = torch.empty_like(x), torch.empty_like(x)
        dgamma, dbeta, dxsum = torch.empty(c).cuda(), torch.empty(c).cuda(), torch.zeros(splits, c).cuda()
        head = (hnd, _p(dy), _p(x), _p(y), None, _p(ga), _p(mean), _p(invstd), _p(dx), _p(dres), _p(dgamma), _p(dbeta), _p(dxsum), c)
        tail = (n, c, layout, 1, stream)
        rc = L.apz_bn_bwd_max(*head, None, *tail) if max_entry else L.apz_bn_bwd(*head, *tail)
        assert rc == 0, L.apz_last_error().decode()
        torch.cuda.synchronize()
        outs.append((dx, dres, dgamma, dbeta, dxsum))
    for i, (a, b) in enumerate(zip(*outs)):
        assert _same(a, b), i


def test_refusals_keep_their_codes_and_texts():
    """The strings are those of the commit in front of the shared host paths"""
    from alphapig_amd import hipconv
    n, c = 2, 128
    x = torch.zeros(n, c, 15, 16).cuda()
    v = torch.zeros(c).cuda()                   # beta, mean, invstd, gamma ...
    w = torch.zeros(4, c).cuda()
    d = torch.zeros(n, 4, 15, 15).cuda()
    L, hnd, stream = hipconv._ctx(x, (15, 15))
    X, V, W, D = _p(x), _p(v), _p(w), _p(d)

    def bn_fwd_frame(x_ptr, layout, side):
        return L.apz_bn_fwd_frame(hnd, x_ptr, None, None, V, None, None, X, V, V, None, n, c, layout, 1, 0.1, 1e-3, side, stream)

    def bn_bwd_frame(x_ptr, layout, side):
        return L.apz_bn_bwd_frame(hnd, X, x_ptr, X, None, None, V, V, X, None, V, V, None, 0, None, n, c, layout, 1, side, stream)

    def conv1x1_fwd_frame(x_ptr, layout, side):
        return L.apz_conv1x1_fwd_frame(hnd, x_ptr, W, None, D, n, c, 4, side, stream)

    def conv1x1_bwd2_frame(x_ptr, layout, side):
        return L.apz_conv1x1_bwd2_frame(hnd, x_ptr, W, D, 4, None, None, 0, X, W, n, c, side, 0, stream)

    def refused(rc, code, text):
        assert rc == code and L.apz_last_error().decode() == text, (rc, L.apz_last_error().decode(), text)

    for call in (bn_fwd_frame, bn_bwd_frame, conv1x1_fwd_frame, conv1x1_bwd2_frame):
        for side in (5, 8, 10, 16):
            refused(call(X, R, side), E_UNSUPPORTED, SIDE % call.__name__)
        refused(call(None, R, 9), E_ARG, BAD)                                # a null x
    refused(bn_fwd_frame(X, DENSE, 9), E_UNSUPPORTED, "bn_fwd_frame: padded-row layout only")
    refused(bn_bwd_frame(X, DENSE, 9), E_UNSUPPORTED, "bn_bwd_frame: padded-row layout only")
    # ... and the plain entries beside them
    refused(L.apz_bn_fwd_stats(hnd, None, None, None, V, None, None, X, V, V, None, None, n, c, R, 1, 0.1, 1e-3, stream), E_ARG, BAD)
    refused(L.apz_bn_bwd_max(hnd, X, None, X, None, None, V, V, X, None, V, V, None, 0, None, n, c, R, 1, stream), E_ARG, BAD)
    refused(L.apz_conv1x1_fwd(hnd, None, W, None, D, n, c, 4, R, stream), E_ARG, BAD)
    refused(L.apz_conv1x1_bwd2(hnd, None, W, D, 4, None, None, 0, X, W, n, c, R, 0, stream), E_ARG, BAD)
    mask = torch.zeros(n, c, 60, dtype=torch.uint8).cuda()
    d8 = torch.zeros(n, c, 8, 8).cuda()
    L8, hnd8, stream8 = hipconv._ctx(d8, (8, 8))
    refused(L8.apz_bn_fwd_stats(hnd8, _p(d8), None, None, V, None, None, _p(d8), V, V, None, _p(mask), n, c, DENSE, 1, 0.1, 1e-3,
                                stream8), E_UNSUPPORTED, "bn_fwd_stats: padded-row layout only")
    refused(L8.apz_bn_bwd_max(hnd8, _p(d8), _p(d8), _p(d8), None, None, V, V, _p(d8), None, V, V, None, 0, V, n, c, DENSE, 1,
                              stream8), E_UNSUPPORTED, "bn_bwd_max: padded-row layout only")
    refused(L8.apz_conv1x1_fwd(hnd8, _p(d8), W, None, D, n, c, 4, R, stream8), E_UNSUPPORTED, "padded-row layout: 15x15 boards only")
    torch.cuda.synchronize()
