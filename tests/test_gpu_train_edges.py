"""The training operators on the tensors a training step really hands them, beside the unit normals of the other modules:
constant and dead channels through BatchNorm, all-zero gradients and single boards through the f16x2 training forms, and
the overflow word of those forms at the operator level -- non-finite inputs, understated or non-finite maxima, a word that
stays set until wino3h_pack_many clears it, and Adam's skip.  Float64 references on the CPU from the same float32 tensors,
at the bars of test_gpu_train.py / test_gpu_train_f16x2.py / test_gpu_wgrad_f16x2.py.  Non-finite floats are data here:
no launch faults."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

U = 2.0 ** -24
EPS = float(np.float32(1e-3))      # the operators take a float


def _rows16(t):
    return F.pad(t, (0, 1)).contiguous()


def _flag(v=0):
    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _word(flag):
    torch.cuda.synchronize()
    return int(flag.item())


def _pack(w, b=None, flag=None):
    from alphapig_amd import hipconv
    return hipconv.wino3h_pack_many(w[None].contiguous(), None if b is None else b[None].contiguous(), flag=flag)


def _dymax(dy):
    return dy.abs().amax(dim=(0, 2, 3)).reshape(1, 128).contiguous()      # what bn_bwd's dxmax holds: partial maxima


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


class _Layer:
    """One trunk layer and n boards: weights, bias, x, dy, the skip gradient; float64 results on demand"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.n = n
        self.w = (torch.randn(128, 128, 3, 3, generator=g) / 34).cuda()
        self.b = torch.randn(128, generator=g).cuda()
        self.x = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
        self.xr = torch.relu(self.x)                                       # the weight gradient's activations
        self.dy = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
        self.add = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
        self.fwd_pack = _pack(self.w, self.b)
        self.bwd_pack = _pack(self.w)

    def y64(self, x):
        return F.conv2d(x[..., :15].double().cpu(), self.w.double().cpu(), self.b.double().cpu(), padding=1)

    def dx64(self, dy, add=None):
        r = F.conv_transpose2d(dy[..., :15].double().cpu(), self.w.double().cpu(), padding=1)
        return r if add is None else r + add[..., :15].double().cpu()

    @staticmethod
    def dw64(x, dy):
        w64 = torch.zeros(128, 128, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x[..., :15].double().cpu(), w64, None, padding=1).backward(dy[..., :15].double().cpu())
        return w64.grad

    # the three operators, each -> result(s) with the word it was given
    def fwd(self, x, flag):
        from alphapig_amd import hipconv
        u, bb = self.fwd_pack
        return hipconv.conv3x3_fwd_stats_f16x2(x, u[0, 0], bb[0, 0], flag)

    def dgrad(self, dy, dymax, flag, add=None):
        from alphapig_amd import hipconv
        u, bb = self.bwd_pack
        return hipconv.conv3x3_dgrad_f16x2(dy, u[0, 1], bb[0, 1], dymax, flag, add=add)

    def wgrad(self, x, dy, dymax, flag):
        from alphapig_amd import hipconv
        return hipconv.conv3x3_wgrad_f16x2(x, dy, dymax, flag)

    # the bars of the f16x2 test modules, against the exact kernel's own error on the same data
    def fwd_in_bar(self, y, x):
        from alphapig_amd import hipconv
        ref = self.y64(x)
        e16, e32 = _rel(y[..., :15], ref), _rel(hipconv.conv3x3_fwd(x, self.w, self.b, hipconv.ROWS16)[..., :15], ref)
        return e16 < max(4 * e32, 1e-5), (e16, e32)

    def dgrad_in_bar(self, dx, dy, add=None):
        from alphapig_amd import hipconv
        ref = self.dx64(dy, add)
        e16, e32 = _rel(dx[..., :15], ref), _rel(hipconv.conv3x3_dgrad(dy, self.w, hipconv.ROWS16, add=add)[..., :15], ref)
        return e16 <= 2 * max(e32, 4e-6), (e16, e32)

    def wgrad_in_bar(self, dw, x, dy):
        from alphapig_amd import hipconv
        ref = self.dw64(x, dy)
        e16, e32 = _rel(dw, ref), _rel(hipconv.conv3x3_wgrad(x, dy, hipconv.ROWS16), ref)
        return e16 < 1e-4 and e16 <= max(4 * e32, 1e-5), (e16, e32)


@pytest.fixture(scope="module")
def layer3():
    return _Layer(3, 31)


# ---- B1: constant channels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_constant_channels(layout):
    """Channel 3 is 0 everywhere, channel 7 is 3.5 (variance exactly 0: invstd = 1 / sqrt(eps), y = beta), channel 11 is
    constant on every board but differs between boards.  On padded rows bn_apply_rows_kernel folds the shift,
    y = x sc + (beta - mean sc): y = beta up to the two roundings of mean sc (2 u |gamma| |mean| invstd); dense: exactly.
    ((x - mean) sc + beta there would give exactly beta too, as the dense kernel does; not chosen: it would change the bits
    of every padded-row BatchNorm output for one more operation per element.)"""
    from alphapig_amd import hipconv
    n, c = 5, 128
    g = torch.Generator().manual_seed(61 + layout)
    x = torch.randn(n, c, 15, 15, generator=g)
    x[:, 3] = 0.0
    x[:, 7] = 3.5
    x[:, 11] = (torch.arange(n).float() * 0.75 - 1.0)[:, None, None]
    ga = torch.rand(c, generator=g) + 0.5
    be = torch.randn(c, generator=g) * 0.2
    dy = torch.randn(n, c, 15, 15, generator=g)
    pad = _rows16 if layout == 1 else (lambda t: t)
    cut = (lambda t: t[..., :15]) if layout == 1 else (lambda t: t)
    xc, dyc, gc, bc = pad(x).cuda(), pad(dy).cuda(), ga.cuda(), be.cuda()
    y, mean, invstd = hipconv.bn_fwd(xc, gc, bc, None, None, None, False, layout, 0.1, EPS)
    dx, _, dgamma, dbeta = hipconv.bn_bwd(dyc, xc, y, gc, mean, invstd, False, False, layout)
    torch.cuda.synchronize()
    assert float(mean[3]) == 0.0 and float(mean[7]) == 3.5
    i0 = 1.0 / np.sqrt(EPS)
    for ch in (3, 7):
        assert abs(float(invstd[ch]) - i0) <= 2 * U * i0
        slack = 2 * U * float(ga[ch]) * abs(float(mean[ch])) * i0 if layout == 1 else 0.0
        assert float((cut(y)[:, ch].cpu() - be[ch]).abs().max()) <= slack, ch
    # everything against float64 at test_bn_forward_backward's bars
    x64 = x.double().requires_grad_(True)
    ga64, be64 = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    y64 = F.batch_norm(x64, None, None, ga64, be64, training=True, eps=EPS)
    y64.backward(dy.double())
    close = lambda a, b, t: float((a.cpu().double() - b).abs().max()) < t * (float(b.abs().max()) + 1e-3)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(y).all())
    assert close(cut(y), y64.detach(), 1e-5)
    assert close(cut(dx), x64.grad, 1e-4)
    assert close(dbeta, be64.grad, 1e-5) and close(dgamma, ga64.grad, 1e-5)
    assert close(mean, x.double().mean(dim=(0, 2, 3)), 1e-6)
    if layout == 1:
        assert float(y[..., 15].abs().max()) == 0.0 and float(dx[..., 15].abs().max()) == 0.0


# ---- B2: a ReLU that is dead on the whole batch ------------------------------------------------------------------------
def test_dead_relu_channels():
    """beta = -50 on four channels: their mask bytes are zero, and dx, dres, dgamma, dbeta, the dxsum and the dxmax columns
    are exactly 0; the other channels as in test_bn_bwd_leaves_the_maxima."""
    from alphapig_amd import hipconv
    n, dead = 9, [0, 5, 64, 127]
    g = torch.Generator().manual_seed(7)
    x = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
    dy = (_rows16(torch.randn(n, 128, 15, 15, generator=g)) * 1e-4).cuda()
    ga = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
    be = torch.zeros(128)
    be[dead] = -50.0
    be = be.cuda()
    R = hipconv.ROWS16
    y, m, i, k = hipconv.bn_fwd(x, ga, be, None, None, None, True, R, 0.1, EPS, want_mask=True)
    splits = hipconv.bn_bwd_splits(x, R)
    assert splits > 1
    dmax = torch.full((splits, 128), 7.0, device="cuda")
    dsum = torch.full((splits, 128), 7.0, device="cuda")
    d0 = hipconv.bn_bwd(dy, x, None, ga, m, i, True, True, R, mask=k)
    d1 = hipconv.bn_bwd(dy, x, None, ga, m, i, True, True, R, mask=k, dxmax=dmax, dxsum=dsum)
    torch.cuda.synchronize()
    dx, dres, dgamma, dbeta = d1
    assert float(y[:, dead].abs().max()) == 0.0 and int(k[:, dead].max()) == 0
    for t in (dx[:, dead], dres[:, dead], dgamma[dead], dbeta[dead], dsum[:, dead], dmax[:, dead]):
        assert float(t.abs().max()) == 0.0
    live = [c for c in range(128) if c not in dead]
    assert int(k[:, live].max()) > 0
    assert torch.equal(d0[0], dx) and torch.equal(d0[1], dres)
    assert torch.equal(dmax.amax(dim=0), dx.abs().amax(dim=(0, 2, 3)))
    assert float(dmax[:, live].amax(dim=0).min()) > 0.0
    ref = dx.double().sum(dim=(0, 2, 3))
    assert float((hipconv.colsum(dsum).double() - ref).abs().max()) < 1e-6 * float(dx.abs().sum(dim=(0, 2, 3)).max())


# ---- B3: gradients that are exactly zero ------------------------------------------------------------------------------
def test_all_zero_gradient(layer3):
    L = layer3
    zero, zmax = torch.zeros_like(L.dy), torch.zeros((2, 128), device="cuda")
    flag = _flag()
    dx = L.dgrad(zero, zmax, flag)
    dxa = L.dgrad(zero, zmax, flag, add=L.add)
    dw = L.wgrad(L.xr, zero, zmax, flag)
    assert _word(flag) == 0
    assert float(dx.abs().max()) == 0.0 and torch.equal(dxa, L.add) and float(dw.abs().max()) == 0.0


def test_one_tiny_gradient_element(layer3):
    """dy zero except one element of 1e-30, true maxima: the device-chosen scale lifts it into the fp16 range, in the data
    gradient and in the weight gradient"""
    L = layer3
    dy = torch.zeros_like(L.dy)
    dy[2, 77, 6, 9] = 1e-30
    flag = _flag()
    dx = L.dgrad(dy, _dymax(dy), flag)
    dxa = L.dgrad(dy, _dymax(dy), flag, add=L.add)
    assert _word(flag) == 0
    ok, e = L.dgrad_in_bar(dx, dy)
    print("dgrad, one 1e-30 element: f16x2 %.3g, f32 %.3g of max |dx64|" % e)
    assert ok, e
    assert float((dxa - L.add - dx).abs().max()) <= 2 * U * float(L.add.abs().max())
    assert float(dx[..., 15].abs().max()) == 0.0
    flag = _flag()
    dw = L.wgrad(L.xr, dy, _dymax(dy), flag)
    assert _word(flag) == 0
    ok, e = L.wgrad_in_bar(dw, L.xr, dy)
    print("wgrad, one 1e-30 element: f16x2 %.3g, f32 %.3g of max |dw64|" % e)
    assert ok, e


# ---- B4: one board, two boards ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_single_boards(n):
    """The missing second board of the pair: forward with statistics and data gradient against float64, complete statistics
    rows, and the bits of the same boards in a launch of five; bn_fwd(stats=) at n = 1 (moving variance: 225 / 224)."""
    from alphapig_amd import hipconv
    L = _Layer(5, 45)
    flag = _flag()
    y5, st5 = L.fwd(L.x, flag)
    dx5 = L.dgrad(L.dy, _dymax(L.dy), flag, add=L.add)
    x, dy, add = L.x[5 - n:].contiguous(), L.dy[5 - n:].contiguous(), L.add[5 - n:].contiguous()
    y, st = L.fwd(x, flag)
    dx = L.dgrad(dy, _dymax(L.dy), flag, add=add)        # the same maxima: the same scale, so the same bits
    dx_own = L.dgrad(dy, _dymax(dy), flag)
    assert _word(flag) == 0
    assert tuple(st.shape) == (128, n, 2) and bool(torch.isfinite(st).all())
    assert torch.equal(y, y5[5 - n:]) and torch.equal(st, st5[:, 5 - n:]) and torch.equal(dx, dx5[5 - n:])
    ok, e = L.fwd_in_bar(y, x)
    assert ok, e
    ok, e = L.dgrad_in_bar(dx, dy, add)
    assert ok, e
    ok, e = L.dgrad_in_bar(dx_own, dy)
    assert ok, e
    yy = y[..., :15].double()
    s1, s2 = yy.sum(dim=(2, 3)).t(), (yy * yy).sum(dim=(2, 3)).t()
    assert float((st[..., 0] - s1).abs().max()) < 1e-5 * float(yy.abs().sum(dim=(2, 3)).max())
    assert float((st[..., 1] - s2).abs().max()) < 1e-5 * float(s2.max())
    for t in (y, dx, dx_own):
        assert float(t[..., 15].abs().max()) == 0.0
    # BatchNorm from the statistics
    be = torch.zeros(128, device="cuda")
    rm, rv = torch.zeros(128, device="cuda"), torch.ones(128, device="cuda")
    a, mean, invstd = hipconv.bn_fwd(y, None, be, rm, rv, None, True, hipconv.ROWS16, 0.1, EPS, stats=st)
    torch.cuda.synchronize()
    M = n * 225.0
    m64 = yy.mean(dim=(0, 2, 3)).cpu()
    v64 = yy.var(dim=(0, 2, 3), unbiased=False).cpu()
    close = lambda got, ref, t: float((got.cpu().double() - ref).abs().max()) < t * (float(ref.abs().max()) + 1e-3)
    assert close(mean, m64, 1e-5) and close(invstd, 1.0 / torch.sqrt(v64 + EPS), 1e-5)
    assert close(rm, 0.1 * m64, 1e-5) and close(rv, 0.9 + 0.1 * v64 * M / (M - 1.0), 1e-5)
    assert float((rv.cpu().double() - (0.9 + 0.1 * v64)).abs().max()) > 1e-4      # ... and not the biased variance


# ---- C: the overflow word ---------------------------------------------------------------------------------------------
POISON = [float("inf"), float("nan")]


@pytest.mark.parametrize("board", [0, 2])
def test_forward_word(layer3, board):
    L = layer3
    for v in POISON + [7e4]:
        hot = L.x.clone()
        hot[board, 19, 7, 3] = v
        flag = _flag()
        L.fwd(hot, flag)
        assert _word(flag) != 0, v
    big = (L.x * (300.0 / float(L.x.abs().max()))).contiguous()            # max |x| = 300: inside the range
    flag = _flag()
    y, _ = L.fwd(big, flag)
    assert _word(flag) == 0
    ok, e = L.fwd_in_bar(y, big)
    assert ok, e


@pytest.mark.parametrize("board", [0, 2])
def test_data_gradient_word(layer3, board):
    """the maxima are those of the clean gradient: the poisoned element is what they did not see"""
    L = layer3
    for v in POISON + [7e4]:
        hot = L.dy.clone()
        hot[board, 19, 7, 3] = v
        flag = _flag()
        L.dgrad(hot, _dymax(L.dy), flag)
        assert _word(flag) != 0, v
    hot = L.dy.clone()
    hot[board, 19, 7, 3] = float("inf")
    flag = _flag()
    L.dgrad(hot, _dymax(hot), flag)                                         # ... and those that did
    assert _word(flag) != 0


@pytest.mark.parametrize("board", [0, 2])
def test_weight_gradient_word(layer3, board):
    L = layer3
    for v in POISON + [700.0]:
        hot = L.xr.clone()
        hot[board, 19, 7, 3] = v
        flag = _flag()
        L.wgrad(hot, L.dy, _dymax(L.dy), flag)
        assert _word(flag) != 0, v
    for v in POISON:
        hot = L.dy.clone()
        hot[board, 19, 7, 3] = v
        flag = _flag()
        L.wgrad(L.xr, hot, _dymax(L.dy), flag)
        assert _word(flag) != 0, v
    warm = L.xr.clone()
    warm[board, 19, 7, 3] = 600.0                                           # inside the range
    flag = _flag()
    dw = L.wgrad(warm, L.dy, _dymax(L.dy), flag)
    assert _word(flag) == 0
    ok, e = L.wgrad_in_bar(dw, warm, L.dy)
    assert ok, e


@pytest.mark.parametrize("k", [1, 4, 8, 12, 20])
def test_understated_maxima(layer3, k):
    """dymax too small by 2^-k: the launch scales too far up.  Either the word is set, or the result is as good as with the
    true maxima -- never a wrong result behind a clean word."""
    L = layer3
    low = _dymax(L.dy) * 2.0 ** -k
    flag = _flag()
    dx = L.dgrad(L.dy, low, flag, add=L.add)
    if _word(flag) == 0:
        ok, e = L.dgrad_in_bar(dx, L.dy, L.add)
        assert ok, (k, e)
    flag = _flag()
    dw = L.wgrad(L.xr, L.dy, low, flag)
    if _word(flag) == 0:
        ok, e = L.wgrad_in_bar(dw, L.xr, L.dy)
        assert ok, (k, e)


def test_non_finite_maxima(layer3):
    """A NaN among the partial maxima is ignored (the same bits); +inf sets the word or leaves a result within the bar."""
    L = layer3
    true = _dymax(L.dy).repeat(2, 1).contiguous()
    flag = _flag()
    dx, dw = L.dgrad(L.dy, true, flag), L.wgrad(L.xr, L.dy, true, flag)
    for at in ((0, 0), (1, 127)):
        bad = true.clone()
        bad[at] = float("nan")
        assert torch.equal(L.dgrad(L.dy, bad, flag), dx) and torch.equal(L.wgrad(L.xr, L.dy, bad, flag), dw)
    assert _word(flag) == 0
    bad = true.clone()
    bad[1, 5] = float("inf")
    flag = _flag()
    dxi = L.dgrad(L.dy, bad, flag)
    if _word(flag) == 0:
        ok, e = L.dgrad_in_bar(dxi, L.dy)
        assert ok, e
    flag = _flag()
    dwi = L.wgrad(L.xr, L.dy, bad, flag)
    if _word(flag) == 0:
        ok, e = L.wgrad_in_bar(dwi, L.xr, L.dy)
        assert ok, e


def test_the_word_stays_until_the_pack_clears_it(layer3):
    from alphapig_amd import hipconv
    L = layer3
    flag = _flag()
    hot = L.x.clone()
    hot[1, 2, 3, 4] = float("inf")
    L.fwd(hot, flag)
    assert _word(flag) != 0
    L.fwd(L.x, flag)
    assert _word(flag) != 0
    L.dgrad(L.dy, _dymax(L.dy), flag)
    assert _word(flag) != 0
    L.wgrad(L.xr, L.dy, _dymax(L.dy), flag)
    assert _word(flag) != 0
    # Adam with the word set: nothing moves
    g = torch.Generator().manual_seed(3)
    w, gr, m, v = (torch.randn(1000, generator=g).cuda() for _ in range(4))
    v = v.abs()
    before = [t.clone() for t in (w, m, v)]
    hipconv.adam_step([(w, gr, m, v, 1e-4)], 1e-3, 0.9, 0.999, 1e-8, 1.0 / 64, w.device, skip=flag)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((w, m, v), before))
    # the next step's pack clears it, and packs what a call without the word packs
    u, bb = _pack(L.w, L.b, flag=flag)
    assert _word(flag) == 0
    assert torch.equal(u, L.fwd_pack[0]) and torch.equal(bb, L.fwd_pack[1])
    hipconv.adam_step([(w, gr, m, v, 1e-4)], 1e-3, 0.9, 0.999, 1e-8, 1.0 / 64, w.device, skip=flag)
    torch.cuda.synchronize()
    assert not torch.equal(w, before[0])
