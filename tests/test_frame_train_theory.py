"""Where the board mask of the framed training step has to sit (csrc/bn_frame.h; DESIGN.md, "Boards smaller than 15x15"),
as a float64 experiment on the CPU.

The framed graph: a stem, one residual block and a linear loss on the 15x15 frame, the S x S board in its top-left
window.  Every whole-plane operator of the product (the trunk convolutions, their data gradients, the heads' input
gradient) is followed by junk of 1e3 written into the off-board cells -- more than those kernels really leave there.  The
mask sits in the four BatchNorm passes only: statistics over on-board cells with the count n S S, the forward apply pass,
the backward reduce pass, and the output of the backward apply pass.  Compared with autograd on the plain S x S board.

With the masks every gradient agrees to rounding; without the statistics mask, without the forward apply mask or without
the backward output mask some gradient is off by more than a percent of its scale."""
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

EPS, JUNK, N, C, CIN = 1e-3, 1e3, 3, 8, 4
SIDES = [6, 7, 9, 12, 14]
ALL_MASKS = dict(stats=True, apply=True, bwd_out=True)


def _problem(S):
    g = torch.Generator().manual_seed(100 + S)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    p = {"w0": rnd(C, CIN, 3, 3) / 6, "b0": rnd(C), "be0": rnd(C) * 0.2,
         "wA": rnd(C, C, 3, 3) / 8, "bA": rnd(C), "gA": torch.rand(C, generator=g, dtype=torch.float64) + 0.5, "beA": rnd(C) * 0.2,
         "wB": rnd(C, C, 3, 3) / 8, "bB": rnd(C), "gB": torch.rand(C, generator=g, dtype=torch.float64) + 0.5, "beB": rnd(C) * 0.2}
    x = (torch.rand(N, CIN, S, S, generator=g) > 0.6).double()
    G = rnd(N, C, S, S)                       # the linear loss: sum(out * G)
    return p, x, G


def _autograd(S):
    p, x, G = _problem(S)
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ones = torch.ones(C, dtype=torch.float64)
    bn = lambda y, ga, be: F.batch_norm(y, None, None, ga, be, training=True, eps=EPS)
    a = torch.relu(bn(F.conv2d(x, p["w0"], p["b0"], padding=1), ones, p["be0"]))
    h = torch.relu(bn(F.conv2d(a, p["wA"], p["bA"], padding=1), p["gA"], p["beA"]))
    out = torch.relu(bn(F.conv2d(h, p["wB"], p["bB"], padding=1), p["gB"], p["beB"]) + a)
    (out * G).sum().backward()
    return {k: v.grad for k, v in p.items()}


class _Framed(object):
    """The same graph on the frame, forward and backward written out as the trainer runs them"""

    def __init__(self, S, masks):
        self.S, self.m = S, masks
        self.on = torch.zeros(15, 15, dtype=torch.bool)
        self.on[:S, :S] = True
        self.M = float(N * S * S)

    def junk(self, t):              # what a whole-plane kernel leaves off the board
        return torch.where(self.on, t, torch.full_like(t, JUNK))

    def sel(self, t, on=True):
        return torch.where(self.on, t, torch.zeros_like(t)) if on else t

    def bn_fwd(self, x, gamma, beta, resid=None):
        xs = self.sel(x, self.m["stats"])
        mean = xs.sum(dim=(0, 2, 3)) / self.M
        var = (xs * xs).sum(dim=(0, 2, 3)) / self.M - mean * mean
        invstd = 1.0 / torch.sqrt(var + EPS)
        bc = lambda v: v.view(1, -1, 1, 1)
        y = (x - bc(mean)) * bc(invstd) * bc(gamma) + bc(beta)
        if resid is not None:
            y = y + resid
        return self.sel(torch.relu(y), self.m["apply"]), mean, invstd

    def bn_bwd(self, dy, x, y, gamma, mean, invstd):
        bc = lambda v: v.view(1, -1, 1, 1)
        dz = dy * (y > 0)
        xhat = (x - bc(mean)) * bc(invstd)
        dzs, xhs = self.sel(dz), self.sel(xhat)                 # the reduce pass selects both, in every variant
        dbeta, dgamma = dzs.sum(dim=(0, 2, 3)), (dzs * xhs).sum(dim=(0, 2, 3))
        dx = bc(gamma * invstd) * (dz - bc(dbeta) / self.M - xhat * bc(dgamma) / self.M)
        return self.sel(dx, self.m["bwd_out"]), self.sel(dz, self.m["bwd_out"]), dgamma, dbeta

    def grads(self):
        S = self.S
        p, x, G = _problem(S)
        ones = torch.ones(C, dtype=torch.float64)
        conv = lambda t, w, b: self.junk(F.conv2d(t, w, b, padding=1))
        dgrad = lambda dy, w: self.junk(torch.nn.grad.conv2d_input(dy.shape[:1] + w.shape[1:2] + dy.shape[2:], w, dy, padding=1))
        wgrad = lambda t, dy, w: torch.nn.grad.conv2d_weight(t, w.shape, dy, padding=1)
        xf = torch.zeros(N, CIN, 15, 15, dtype=torch.float64)
        xf[..., :S, :S] = x
        y0 = conv(xf, p["w0"], p["b0"])
        a, m0, i0 = self.bn_fwd(y0, ones, p["be0"])
        yA = conv(a, p["wA"], p["bA"])
        h, mA, iA = self.bn_fwd(yA, p["gA"], p["beA"])
        yB = conv(h, p["wB"], p["bB"])
        out, mB, iB = self.bn_fwd(yB, p["gB"], p["beB"], a)
        d_out = torch.full((N, C, 15, 15), JUNK, dtype=torch.float64)       # the heads' input gradient: the window only
        d_out[..., :S, :S] = G
        g = {}
        dyB, dskip, g["gB"], g["beB"] = self.bn_bwd(d_out, yB, out, p["gB"], mB, iB)
        g["wB"], g["bB"] = wgrad(h, dyB, p["wB"]), dyB.sum(dim=(0, 2, 3))
        dh = dgrad(dyB, p["wB"])
        dyA, _, g["gA"], g["beA"] = self.bn_bwd(dh, yA, h, p["gA"], mA, iA)
        g["wA"], g["bA"] = wgrad(a, dyA, p["wA"]), dyA.sum(dim=(0, 2, 3))
        da = self.junk(dgrad(dyA, p["wA"]) + dskip)
        dy0, _, _, g["be0"] = self.bn_bwd(da, y0, a, ones, m0, i0)
        g["w0"], g["b0"] = wgrad(xf, dy0, p["w0"]), dy0.sum(dim=(0, 2, 3))
        return g


def _worst(got, ref):
    """max over the gradients of |got - ref| / scale; a convolution bias in front of a BatchNorm has the true gradient
    zero, so it is held to the scale of its weight's gradient"""
    worst = 0.0
    for k, r in ref.items():
        scale = float(ref["w" + k[1:]].abs().max()) if k in ("b0", "bA", "bB") else float(r.abs().max())
        worst = max(worst, float((got[k] - r).abs().max()) / scale)
    return worst


@pytest.fixture(scope="module")
def reference():
    return {S: _autograd(S) for S in SIDES}


@pytest.mark.parametrize("S", SIDES)
def test_masks_in_the_four_batchnorm_passes_suffice(S, reference):
    got = _Framed(S, ALL_MASKS).grads()
    assert set(got) == set(reference[S])
    assert _worst(got, reference[S]) < 1e-12


@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("without", ["stats", "apply", "bwd_out"])
def test_each_mask_is_needed(S, without, reference):
    got = _Framed(S, dict(ALL_MASKS, **{without: False})).grads()
    assert _worst(got, reference[S]) > 1e-2
