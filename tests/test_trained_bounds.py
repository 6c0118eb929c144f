"""The bars of tests/test_gpu_trained_weights.py, tried on the CPU: a bar that plain float32 arithmetic cannot meet is a
wrong bar.  Forty optimiser steps of tests/torch_trainer.py (float32) on the committed episodes, then the inference graph
with PyTorch's float32 library operators against the float64 oracle on the evaluation positions: every error stays within
a TENTH of its bar -- per layer, per output channel (against (1e-4 / 3) * max(1, A_c), A_c from |x| * |folded w| + |shift|),
logits, value logit, probabilities and values -- and channels the oracle calls dead are exactly 0.  (On 300-step weights
the layer errors were 0.005 to 0.008 of the bar.)  Also: the pieces of tests/trained_nets.py that need no GPU."""
import numpy as np
import pytest

import trained_nets as tn


def test_fixture_tuples_and_held_out_positions():
    states, pis, zs, pos = tn.fixture_tuples(15)
    assert states.shape == (2224, 9, 15, 15) and pis.shape == (2224, 225) and zs.shape == (2224,)
    assert np.abs(pis.sum(axis=1) - 1).max() < 1e-3 and set(np.unique(zs)) <= {-1.0, 0.0, 1.0}
    s8 = tn.fixture_tuples(8)
    assert s8[0].shape == (160, 9, 8, 8)
    for side, n in ((15, 40), (8, 36)):
        planes = tn.eval_positions(side)
        assert planes.shape == (n, 9, side, side) and set(np.unique(planes)) <= {0.0, 1.0}
        assert len({p.tobytes() for p in planes}) == n
        # no evaluation position is an image of a position a training batch can draw
        st, _, _, pos = tn.fixture_tuples(side)
        pool = {st[i].tobytes() for i in np.flatnonzero(~np.isin(pos, tn.held_out(side)))}
        assert not pool & {p.tobytes() for p in planes[2:]}


@pytest.mark.parametrize("kind,side,blocks", [("resnet", 15, 3), ("simple", 8, 0)])
def test_float32_meets_a_tenth_of_every_bar_on_trained_weights(kind, side, blocks):
    import torch
    prm, losses = tn.trained_params_cpu(kind, side, blocks, 40)
    assert np.isfinite(losses).all() and np.mean(losses[-10:]) < losses[0]
    planes = tn.eval_positions(side)
    ref = tn.Reference(prm, planes, kind, blocks)
    got = tn.torch_forward_layers(prm, planes, kind, blocks, torch.float32)
    rec, bad = ref.check_heads(got[:4])
    worst = {k: v for k, v in rec.items() if k.endswith("_over_bar")}
    for l, a in enumerate(got[4]):
        r, b = ref.check_layer(l, a)
        bad += b
        worst["layer%d" % l] = r["err_over_bar"]
        worst["layer%d_chan" % l] = r["chan_err_over_bar"]
    print(kind, side, {k: "%.4f" % v for k, v in worst.items()})
    assert not bad, bad
    assert max(worst.values()) < 0.1, worst
