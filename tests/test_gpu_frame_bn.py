"""The framed padded-row BatchNorm kernels (csrc/bn_frame.h: hipconv.bn_fwd / bn_bwd with side=S) and the framed 1x1
head entry points, operator by operator: against torch float64 autograd on the S x S crop at the bars of
test_gpu_train.py::test_bn_forward_backward, off-board outputs exactly +0, the same bits whatever the off-board inputs
hold (NaN and inf included), the existing kernels' bits at S = 15, and the same bits on a second call."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

R = 1          # hipconv.ROWS16
# (relu, residual, gamma): each switch on and off, relu = 0 with and without a residual (no ReLU bit hides dy there)
FLAGS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]


def _on_board(S):
    on = torch.zeros(15, 16, dtype=torch.bool)
    on[:S, :S] = True
    return on


def _poison(shape):
    """NaN, +inf, -inf and 1e30 in turn"""
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30])
    return vals[torch.arange(int(np.prod(shape))) % 4].reshape(shape)


def _frame(t, S, poison):
    """[n][C][S][S] -> padded rows [n][C][15][16] on the device, the off-board cells zero or poisoned"""
    n, c = t.shape[:2]
    out = _poison((n, c, 15, 16)) if poison else torch.zeros(n, c, 15, 16)
    out[..., :S, :S] = t
    return out.contiguous().cuda()


def _words(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and bool((_words(a.float() if a.dtype == torch.uint8 else a) ==
                                                                _words(b.float() if b.dtype == torch.uint8 else b)).all())


def _run(S, x, r, dy, ga, be, relu, resid, gamma, poison, use_mask=True):
    """forward + backward on the framed kernels -> every output, in a fixed order"""
    from alphapig_amd import hipconv
    c = x.shape[1]
    xc, dyc = _frame(x, S, poison), _frame(dy, S, poison)
    rc = _frame(r, S, poison) if resid else None
    gc, bc = (ga.cuda() if gamma else None), be.cuda()
    rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
    y, mean, invstd, mask = hipconv.bn_fwd(xc, gc, bc, rm, rv, rc, relu, R, 0.1, 1e-3, want_mask=True, side=S)
    splits = hipconv.bn_bwd_splits(xc, R, side=S)
    dxsum = torch.full((splits, c), 7.0, device="cuda")
    dxmax = torch.full((splits, c), 7.0, device="cuda")
    dx, dres, dgamma, dbeta = hipconv.bn_bwd(dyc, xc, None if use_mask else y, gc, mean, invstd, relu, resid, R, dxsum=dxsum,
                                             mask=mask if use_mask else None, dxmax=dxmax, side=S)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, mask=mask, run_mean=rm, run_var=rv, dx=dx, dres=dres, dgamma=dgamma,
                dbeta=dbeta, dxsum=dxsum, dxmax=dxmax)


@pytest.mark.parametrize("S,n,c", list(itertools.product([6, 7, 9, 12, 13, 14], [1, 5, 9], [3, 128])))
def test_framed_bn_forward_backward(S, n, c):
    g = torch.Generator().manual_seed(1000 * S + 10 * n + c)
    x = torch.randn(n, c, S, S, generator=g) * 1.7 + 0.3
    r = torch.randn(n, c, S, S, generator=g)
    ga = torch.rand(c, generator=g) + 0.5
    be = torch.randn(c, generator=g) * 0.2
    dy = torch.randn(n, c, S, S, generator=g)
    on = _on_board(S).cuda()
    close = lambda a, b, t: float((a.cpu().double() - b).abs().max()) < t * (float(b.abs().max()) + 1e-3)
    for relu, resid, gamma in FLAGS:
        x64, r64 = x.double().requires_grad_(True), r.double().requires_grad_(True)
        ga64, be64 = ga.double().requires_grad_(gamma), be.double().requires_grad_(True)
        rm64, rv64 = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
        y64 = F.batch_norm(x64, rm64, rv64, ga64 if gamma else torch.ones(c, dtype=torch.float64), be64, training=True,
                           momentum=0.1, eps=1e-3)
        if resid:
            y64 = y64 + r64
        if relu:
            y64 = torch.relu(y64)
        y64.backward(dy.double())
        clean = _run(S, x, r, dy, ga, be, relu, resid, gamma, poison=False)
        dirty = _run(S, x, r, dy, ga, be, relu, resid, gamma, poison=True)
        again = _run(S, x, r, dy, ga, be, relu, resid, gamma, poison=True)
        by_y = _run(S, x, r, dy, ga, be, relu, resid, gamma, poison=True, use_mask=False)     # ReLU decisions read from y
        tag = (relu, resid, gamma)
        # accuracy on the board
        cut = lambda t: t[..., :S, :S]
        assert close(cut(clean["y"]), y64.detach(), 1e-5), tag
        assert close(cut(clean["dx"]), x64.grad, 1e-4), tag
        assert close(clean["dbeta"], be64.grad, 1e-5), tag
        if gamma:
            assert close(clean["dgamma"], ga64.grad, 1e-5), tag
        if resid:
            assert close(cut(clean["dres"]), r64.grad, 1e-6), tag
        else:
            assert clean["dres"] is None
        assert close(clean["run_mean"], rm64, 1e-5) and close(clean["run_var"], rv64, 1e-5), tag
        assert close(clean["mean"], x.double().mean(dim=(0, 2, 3)), 1e-5), tag
        for out in (clean, dirty):
            # off the board: exactly +0 (the word, not the value: -0 and NaN would both slip through a comparison with 0.0)
            for k in ("y", "dx") + (("dres",) if resid else ()):
                assert int((_words(out[k])[..., ~on] != 0).sum()) == 0, (tag, k)
            bits = torch.stack([(out["mask"] >> e) & 1 for e in range(4)], dim=-1).reshape(n, c, 15, 16).bool()
            assert not bool(bits[..., ~on].any()), tag
            assert torch.equal(bits, out["y"] > 0), tag
            assert bool(torch.isfinite(out["dxsum"]).all()) and bool(torch.isfinite(out["dxmax"]).all()), tag
        # whatever the off-board inputs hold, and on every call: the same bits
        for k in clean:
            assert _same_bits(clean[k], dirty[k]), (tag, k, "poison")
            assert _same_bits(dirty[k], again[k]), (tag, k, "second call")
            assert _same_bits(dirty[k], by_y[k]), (tag, k, "ReLU decisions from y")
        # dxsum / dxmax are those of the masked dx
        ref_sum = clean["dx"].double().sum(dim=(2, 3))
        assert float((clean["dxsum"].double().sum(dim=0) - ref_sum.sum(dim=0)).abs().max()) <= 1e-6 * float(
            clean["dx"].abs().sum(dim=(0, 2, 3)).max()) + 1e-12, tag
        assert torch.equal(clean["dxmax"].max(dim=0).values, clean["dx"].abs().amax(dim=(0, 2, 3))), tag


@pytest.mark.parametrize("n", [5, 9])
def test_side_15_returns_the_existing_kernels_bits(n):
    """side=15 is the pad-column rule of the plain padded-row kernels: the same bits as that path with its own statistics pass"""
    from alphapig_amd import hipconv
    c, S = 128, 15
    g = torch.Generator().manual_seed(77 + n)
    x = torch.randn(n, c, S, S, generator=g) * 1.7 + 0.3
    r = torch.randn(n, c, S, S, generator=g)
    dy = torch.randn(n, c, S, S, generator=g)
    ga, be = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    xc, rcc, dyc = _frame(x, S, False), _frame(r, S, False), _frame(dy, S, False)
    for relu, resid, gamma in FLAGS:
        outs = []
        for side in (None, 15):
            kw = {} if side is None else {"side": side}
            gc, rc = (ga.cuda() if gamma else None), (rcc if resid else None)
            rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
            y, mean, invstd, mask = hipconv.bn_fwd(xc, gc, be.cuda(), rm, rv, rc, relu, R, 0.1, 1e-3, want_mask=True, **kw)
            splits = hipconv.bn_bwd_splits(xc, R, **kw)
            dxsum, dxmax = torch.zeros(splits, c).cuda(), torch.zeros(splits, c).cuda()
            res = hipconv.bn_bwd(dyc, xc, None, gc, mean, invstd, relu, resid, R, dxsum=dxsum, mask=mask, dxmax=dxmax, **kw)
            res_y = hipconv.bn_bwd(dyc, xc, y, gc, mean, invstd, relu, resid, R, **kw)
            torch.cuda.synchronize()
            outs.append((y, mean, invstd, mask, rm, rv, dxsum, dxmax) + tuple(res) + tuple(res_y))
        for i, (a, b) in enumerate(zip(*outs)):
            assert _same_bits(a, b), ((relu, resid, gamma), i)


def test_side_is_checked():
    from alphapig_amd import hipconv
    x = torch.zeros(2, 3, 15, 16).cuda()
    be = torch.zeros(3).cuda()
    for side in (5, 8, 10, 16):
        with pytest.raises(RuntimeError, match="side"):
            hipconv.bn_fwd(x, None, be, None, None, None, True, R, 0.1, 1e-3, side=side)
    with pytest.raises(ValueError, match="padded-row"):
        hipconv.bn_fwd(torch.zeros(2, 3, 15, 15).cuda(), None, be, None, None, None, True, 0, 0.1, 1e-3, side=9)
    with pytest.raises(RuntimeError, match="side"):
        hipconv.frame_planes(torch.zeros(2, 3, 10, 10).cuda())


def test_frame_planes():
    from alphapig_amd import hipconv
    x = torch.randn(5, 9, 9, 9)
    y = hipconv.frame_planes(x.cuda())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (5, 9, 15, 15) and torch.equal(y[..., :9, :9].cpu(), x)
    y[..., :9, :9] = 0
    assert int((_words(y) != 0).sum()) == 0


def tol(ref, rel=2e-5):
    return rel * float(ref.detach().abs().max()) + 1e-6


def err(got, ref):
    return float((got.detach().cpu().double() - ref.detach()).abs().max())


def test_framed_heads_forward_and_pair_backward():
    """The 1x1 head convolutions on the S x S window of a padded-row trunk output whose off-board cells hold anything, at the
    bars of test_gpu_train.py::test_head_conv1x1_forward_backward"""
    from alphapig_amd import hipconv
    S, n, c = 9, 5, 128
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, c, S, S, generator=g)
    w1, w2 = torch.randn(4, c, 1, 1, generator=g) / float(np.sqrt(c)), torch.randn(2, c, 1, 1, generator=g) / float(np.sqrt(c))
    b1, b2 = torch.randn(4, generator=g), torch.randn(2, generator=g)
    dy1, dy2 = torch.randn(n, 4, S, S, generator=g), torch.randn(n, 2, S, S, generator=g)
    x64 = x.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    y1, y2 = F.conv2d(x64, p64[0], p64[1]), F.conv2d(x64, p64[2], p64[3])
    ((y1 * dy1.double()).sum() + (y2 * dy2.double()).sum()).backward()
    xc = _frame(x, S, poison=True)
    for w, b, y64 in ((w1, b1, y1), (w2, b2, y2)):
        y = hipconv.conv1x1_fwd(xc, w.cuda(), b.cuda(), R, side=S)
        assert tuple(y.shape) == tuple(y64.shape) and err(y, y64) < tol(y64)
    dx, dw1, db1, dw2, db2 = hipconv.conv1x1_bwd_pair(xc, w1.cuda(), dy1.cuda(), w2.cuda(), dy2.cuda(), R, side=S)
    torch.cuda.synchronize()
    assert err(dx[..., :S, :S], x64.grad) < tol(x64.grad)
    assert int((_words(dx[..., :S, S:]) != 0).sum()) == 0           # the written rows' own off-board columns: zero
    for got, ref in ((dw1, p64[0]), (db1, p64[1]), (dw2, p64[2]), (db2, p64[3])):
        assert err(got, ref.grad) < 5 * tol(ref.grad)
    # rows S .. 14 of dx are left to bn_bwd(side=S): whatever they hold there, the same bits come out
    be = torch.zeros(c).cuda()
    yb, mean, invstd = hipconv.bn_fwd(xc, None, be, None, None, None, True, R, 0.1, 1e-3, side=S)
    a = hipconv.bn_bwd(dx, xc, yb, None, mean, invstd, True, False, R, side=S)[0]
    dx[..., S:, :] = float("nan")
    b = hipconv.bn_bwd(dx, xc, yb, None, mean, invstd, True, False, R, side=S)[0]
    torch.cuda.synchronize()
    assert _same_bits(a, b) and bool(torch.isfinite(a).all())


def test_dense_operators_run_at_a_framed_size():
    """Behind the framed 1x1 convolutions the heads are dense [n][C][S][S]: the head BatchNorms, the loss, FullyConnected and
    Dropout already run at such a size (an S x S helper engine whose dense kernels take H and W at run time)"""
    from alphapig_amd import hipconv
    S, n = 9, 5
    g = torch.Generator().manual_seed(8)
    close = lambda a, b, t: float((a.cpu().double() - b).abs().max()) < t * (float(b.abs().max()) + 1e-3)
    for c in (4, 2):
        x, dy, be = torch.randn(n, c, S, S, generator=g) + 0.2, torch.randn(n, c, S, S, generator=g), torch.randn(c, generator=g) * 0.2
        x64, be64 = x.double().requires_grad_(True), be.double().requires_grad_(True)
        y64 = torch.relu(F.batch_norm(x64, None, None, torch.ones(c, dtype=torch.float64), be64, training=True, eps=1e-3))
        y64.backward(dy.double())
        y, mean, invstd = hipconv.bn_fwd(x.cuda(), None, be.cuda(), None, None, None, True, 0, 0.1, 1e-3)
        dx, _, _, dbeta = hipconv.bn_bwd(dy.cuda(), x.cuda(), y, None, mean, invstd, True, False, 0)
        torch.cuda.synchronize()
        assert close(y, y64.detach(), 1e-5) and close(dx, x64.grad, 1e-4) and close(dbeta, be64.grad, 1e-5)
    hw = S * S
    logits, u = torch.randn(n, hw, generator=g) * 3, torch.randn(n, generator=g)
    pi = torch.softmax(torch.randn(n, hw, generator=g), dim=1)
    z = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0])
    l64, u64 = logits.double().requires_grad_(True), u.double().requires_grad_(True)
    logp = F.log_softmax(l64, dim=1)
    vl, pl = ((z.double() - torch.tanh(u64)) ** 2).mean(), (-(logp * pi.double()).sum(dim=1)).mean()
    (vl + pl).backward()
    vl, pl = vl.detach(), pl.detach()
    out = hipconv.pv_loss(logits.cuda(), u.cuda(), pi.cuda(), z.cuda(), grads=True)
    l3 = out["loss3"].cpu().double()
    assert abs(float(l3[0] - vl)) < 1e-5 * (1 + float(vl)) and abs(float(l3[1] - pl)) < 1e-5 * (1 + float(pl))
    assert err(out["dlogits"], l64.grad) < tol(l64.grad, 1e-4) and err(out["dvlogit"], u64.grad) < tol(u64.grad, 1e-4)
    xin, w, b = torch.randn(n, 4 * hw, generator=g), torch.randn(hw, 4 * hw, generator=g) / 18, torch.randn(hw, generator=g)
    assert err(hipconv.fc_fwd(xin.cuda(), w.cuda(), b.cuda()), xin.double() @ w.double().t() + b.double()) < 1e-4
    d = hipconv.dropout(xin.cuda(), 0.5, 3, 1)
    assert torch.equal(d, hipconv.dropout(xin.cuda(), 0.5, 3, 1)) and torch.equal(d[d != 0], (xin.cuda() * 2)[d != 0])
