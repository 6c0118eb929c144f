"""The inference heads' softmax and tanh at peaked policies and saturated values, on both head paths: 15x15 boards
(head_fc_kernel<1, true> + head_softmax_value_kernel, csrc/heads.h) and 8x8 boards (head8_kernel, csrc/conv8_small.h,
the one-launch head every 8x8 engine runs; head_fc_kernel<1>'s fused tail has no board size that reaches it).

A freshly initialised net has logits of a few tenths.  The FullyConnected layers are linear in their parameters, so
fc_3_1_1 / fc_3_2_1 scaled by f scale the logits and the value logit by f: f = 30 gives a peaked policy, f = 1000 a
one-hot one and |value logit| up to 1500.  Two separate checks, so that a softmax error cannot hide behind the GEMM's:
  * logits / value logits against oracle/net_ref.py in float64 on the scaled float32 parameters, to LOGIT_ATOL * f
    (the suite's 1e-4 carried through the linear layer);
  * probs against the float64 softmax of THE KERNEL'S OWN float32 logits, values against the float64 tanh of its own
    value logit, at the bars of tests/test_head_loss_bounds.py.
n = 1, 5, 17, 37: the tail of the 4-board softmax workgroup, of the 16-board FullyConnected tile, and both."""
import numpy as np
import pytest

import test_head_loss_bounds as hb
from alphapig_amd import weights
from oracle import net_ref
from test_gpu_net import LOGIT_ATOL, random_positions

pytestmark = pytest.mark.gpu

FACTORS = (1, 30, 1000)
NMAX = 37
# seeds chosen with the float64 oracle alone: no row's top-two logit gap is within 2 * LOGIT_ATOL (0 % of the rows are left
# out of the argmax check; the test asserts < 10 %); at f = 1000, 8 of the 37 15x15 rows (3 of the first 5) and all 8x8
# rows are exactly one-hot in float32, and the value logits are 390 .. 1115 and 440 .. 500 (12 .. 33 at f = 30 on 15x15)
NETS = {"split15": dict(kind="resnet", side=15, blocks=1, init=("resnet", 15, 15, 9, 1, 128), seed=5, planes_seed=500),
        "head8": dict(kind="simple", side=8, blocks=0, init=("simple", 8, 8, 9), seed=10, planes_seed=502)}
HEAD_PARAMS = ("fc_3_1_1_weight", "fc_3_1_1_bias", "fc_3_2_1_weight", "fc_3_2_1_bias")


def scaled(prm, f):
    out = dict(prm)
    for k in HEAD_PARAMS:
        out[k] = np.asarray(prm[k], dtype=np.float32) * np.float32(f)
    return out


@pytest.fixture(scope="module")
def heads():
    """-> get(name, f): (net with the scaled parameters loaded, planes, float64 oracle outputs of the scaled parameters);
    one engine per path, one oracle run per (path, f)"""
    from alphapig_amd.policy_value_net import PolicyValueNet
    nets, cache = {}, {}

    def get(name, f):
        cfg = NETS[name]
        if name not in nets:
            prm = weights.init_params(*cfg["init"], seed=cfg["seed"], style="bench")
            if cfg["kind"] == "resnet":
                net = PolicyValueNet(15, 15, batch_size=64, n_blocks=1, n_filter=128, model_params=prm)
            else:
                net = PolicyValueNet(8, 8, batch_size=64, model_params=prm, net_kind="simple")
            nets[name] = [net, prm, random_positions(NMAX, cfg["side"], seed=cfg["planes_seed"])[1], None]
        net, prm, planes, loaded = nets[name]
        if (name, f) not in cache:
            cache[(name, f)] = net_ref.forward(scaled(prm, f), planes, cfg["kind"], cfg["blocks"] or 10, np.float64)
        if loaded != f:
            net.set_params(scaled(prm, f))
            nets[name][3] = f
        return net, planes, cache[(name, f)]

    yield get
    for net, *_ in nets.values():
        net.close()


@pytest.mark.parametrize("n", [1, 5, 17, 37])
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("name", sorted(NETS))
def test_softmax_and_tanh_of_scaled_heads(heads, name, f, n):
    net, planes, oracle = heads(name, f)
    planes = planes[:n]
    o_logits, o_vlog = oracle[0][:n], oracle[2][:n, 0]
    logits, probs, vlog, vals = net.forward_with_logits(planes)
    for a in (logits, probs, vlog, vals):
        assert np.isfinite(a).all()
    # 1. the linear layers
    bar = LOGIT_ATOL * f
    e_l, e_v = np.abs(logits - o_logits).max(), np.abs(vlog - o_vlog).max()
    # 2. softmax / tanh of the kernel's own logits
    p_bar, sum_bar = hb.softmax_bar(logits)
    q_p = hb.ratio(probs, hb.softmax64(logits)[0], p_bar)
    q_s = hb.ratio(probs.astype(np.float64).sum(axis=1), 1.0, sum_bar)
    q_v = hb.ratio(vals, np.tanh(vlog.astype(np.float64)), hb.tanh_bar(vlog))
    top = np.sort(o_logits, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * bar
    print("%s f %g n %d: logits %.2e value logit %.2e (bar %.0e)  error / bar: probs %.3f row sum %.3f values %.3f  "
          "max p %.6f  max |value logit| %.1f  rows left out of the argmax check %.0f %%" % (
              name, f, n, e_l, e_v, bar, q_p, q_s, q_v, probs.max(), np.abs(vlog).max(), 100 * (1 - clear.mean())))
    assert e_l <= bar and e_v <= bar
    assert q_p <= 1.0 and q_s <= 1.0 and q_v <= 1.0
    assert (np.abs(vals) <= 1).all()
    assert 1 - clear.mean() < 0.10
    np.testing.assert_array_equal(probs.argmax(axis=1)[clear], o_logits.argmax(axis=1)[clear])
    if f == 1000:                       # the policy is one-hot wherever the kernel's own logits say so
        gap = np.sort(logits.astype(np.float64), axis=1)
        hot = gap[:, -1] - gap[:, -2] > hb.ONE_HOT_GAP
        assert hot.any() or n == 1
        assert (probs[hot].max(axis=1) == 1).all() and ((probs[hot] == 0).sum(axis=1) == probs.shape[1] - 1).all()
    p2, v2 = net.forward_planes(planes)
    np.testing.assert_array_equal(p2, probs)
    np.testing.assert_array_equal(v2, vals)
