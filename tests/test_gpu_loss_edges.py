"""apz_pv_loss (pv_loss_kernel, csrc/heads_train.h) against float64 log_softmax / tanh and their gradients on the same
float32 inputs, where a trained net puts it: peaked and exactly one-hot policies, logits offset by +-1e4, one-hot targets
on the most and on the least likely cell, empty targets, draws, and value logits from 1e-20 to far past where tanhf
saturates.  The bars, the input families and the float64 reference come from tests/test_head_loss_bounds.py (which checks
on the CPU that a float32 restatement of the kernel keeps 4x room inside them); a workgroup is four samples, so
n = 1, 3, 5 are its tails."""
import numpy as np
import pytest

import test_head_loss_bounds as hb

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("loss3", "dlogits", "dvlogit", "probs", "values")


def run(args, outputs_only=False):
    from alphapig_amd import hipconv
    dev = [torch.from_numpy(a).cuda() for a in args]
    out = hipconv.pv_loss(dev[0], dev[1], outputs=True) if outputs_only else hipconv.pv_loss(*dev, grads=True, outputs=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_the_float64_reference_is_autograd():
    """the analytic gradients of hb.pv_loss64 are torch's float64 autograd of the same loss (CPU arithmetic only)"""
    F = torch.nn.functional
    logits, u, pi, z = (torch.from_numpy(a).double() for a in hb.loss_batch("randn30", "dirichlet", 5, 64, 3))
    logits.requires_grad_(True)
    u.requires_grad_(True)
    logp = F.log_softmax(logits, dim=1)
    (((z - torch.tanh(u)) ** 2).mean() + (-(logp * pi).sum(dim=1)).mean()).backward()
    ref = hb.pv_loss64(logits.detach().numpy(), u.detach().numpy(), pi.numpy(), z.numpy())
    np.testing.assert_allclose(ref["dlogits"], logits.grad.numpy(), rtol=1e-12, atol=1e-300)
    # autograd forms 1 - tanh^2 with the cancellation (2e-16 absolute), the reference takes 1 / cosh^2
    np.testing.assert_allclose(ref["dvlogit"], u.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["probs"], logp.exp().detach().numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("hw", [225, 64])
@pytest.mark.parametrize("n", [1, 3, 5, 37])
def test_loss_head_inside_its_bars_on_every_family(n, hw):
    worst = {}
    for combo, lf, tf in hb.loss_combos():
        args = hb.loss_batch(lf, tf, n, hw, combo)
        bars, ref = hb.pv_loss_bars(*args)
        got = run(args)
        for k in KEYS:
            assert np.isfinite(got[k]).all(), (lf, tf, k)
            worst[(lf, k)] = max(worst.get((lf, k), 0.0), hb.ratio(got[k], ref[k], bars[k]))
        assert got["loss3"][2] >= 0, (lf, tf)
        assert (np.abs(got["values"]) <= 1).all(), (lf, tf)
        assert (got["dvlogit"][np.abs(got["values"]) == 1] == 0).all(), (lf, tf)     # tanhf returned +-1: exactly no gradient
        empty = ~args[2].any(axis=1)                                                 # an all-zero pi row
        assert (got["dlogits"][empty] == 0).all(), (lf, tf)
        only = run(args, outputs_only=True)
        assert set(only) == {"probs", "values"}
        assert np.array_equal(only["probs"], got["probs"]) and np.array_equal(only["values"], got["values"])
    for lf in hb.LOGIT_FAMILIES:
        print("n %d hw %d %-10s kernel / bar: %s" % (n, hw, lf, "  ".join("%s %.3f" % (k, worst[(lf, k)]) for k in KEYS)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


@pytest.mark.parametrize("hw", [225, 64])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_one_hot_policies_have_exactly_zero_entropy_and_empty_targets_no_cross_entropy(n, hw):
    args = hb.one_hot_batch(n, hw)
    got = run(args)
    assert np.isfinite(got["loss3"]).all()
    assert got["loss3"][2] == 0                                   # 0 x finite in every cell, never 0 x inf
    assert ((got["probs"] == 1).sum(axis=1) == 1).all() and ((got["probs"] == 0).sum(axis=1) == hw - 1).all()
    bars, ref = hb.pv_loss_bars(*args)
    for k in KEYS:
        assert np.isfinite(got[k]).all() and hb.ratio(got[k], ref[k], bars[k]) <= 1.0, k
    # empty targets only: cross-entropy exactly 0, no policy gradient
    logits, u, pi, z = args
    got = run((logits, u, np.zeros_like(pi), z))
    assert got["loss3"][1] == 0 and not got["dlogits"].any()
