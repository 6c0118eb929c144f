"""The user-visible property of PolicyValueNet(uniform_trunk=True): with trunk_arith "f16x2" on the 15x15 / 128-filter net a
self-play game depends on its seed only, not on how many games share a forward.  36 games played 36 at a time (batches of 36
boards -- the batched f16x2 kernel -- shrinking through the 32-board threshold to the tail) and 4 at a time (always the
small-batch kernel, csrc/trunk15_wino3hs.h) give identical moves, pi and z for every game index."""
import numpy as np
import pytest

from alphapig_amd import weights
from alphapig_amd.selfplay import SelfPlayEngine

pytestmark = pytest.mark.gpu


def _play(prm, concurrent):
    from alphapig_amd.policy_value_net import PolicyValueNet
    net = PolicyValueNet(15, 15, batch_size=64, n_blocks=2, n_filter=128, model_params=prm, trunk_arith="f16x2",
                         uniform_trunk=True)
    eng = SelfPlayEngine(net, 15, 15, 5, n_games=concurrent, n_playout=8, base_seed=123, pipeline=1)
    try:
        eps = eng.play_games(36)
        assert net.trunk_overflows() == 0
        return eps
    finally:
        eng.close()
        net.close()


def test_a_game_does_not_depend_on_the_number_of_concurrent_games():
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=9, style="bench")
    wide, narrow = _play(prm, 36), _play(prm, 4)
    assert len(wide) == 36 and len(narrow) == 36
    for a, b in zip(wide, narrow):
        assert a.index == b.index
        np.testing.assert_array_equal(a.moves, b.moves)
        np.testing.assert_array_equal(np.asarray(a.pis), np.asarray(b.pis))
        np.testing.assert_array_equal(np.asarray(a.zs), np.asarray(b.zs))
