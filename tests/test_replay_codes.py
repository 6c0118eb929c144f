"""replay.planes_to_codes is the inverse of TreePool.codes_to_planes: on the planes the reference itself produced
(tests/golden/planes.npz) and on the codes of a scripted game."""
import os

import numpy as np
import pytest

from alphapig_amd.game import Board
from alphapig_amd.replay import CompactReplayBuffer, planes_to_codes
from alphapig_amd.treepool import TreePool


def test_planes_of_the_reference_survive_the_round_trip(golden_dir):
    g = np.load(os.path.join(golden_dir, "planes.npz"))
    pools = {}
    seen = 0
    for k in range(int(g["n_cases"])):
        w, n_in_row = int(g["c%d_meta" % k][0]), int(g["c%d_meta" % k][1])
        pool = pools.setdefault(w, TreePool(w, w, n_in_row, n_games=1, n_playout=1))
        for key, c_in in (("c%d_planes" % k, 9), ("c%d_planes4" % k, 4)):
            p = g[key].astype(np.float32)[None]
            codes = planes_to_codes(p)
            assert codes.dtype == np.uint8 and codes.shape == (1, pool.code_stride)
            np.testing.assert_array_equal(pool.codes_to_planes(codes, c_in), p)
            seen += 1
    assert seen >= 2
    for pool in pools.values():
        pool.close()


def test_codes_of_a_scripted_game_survive_the_round_trip():
    pool = TreePool(15, 15, 5, n_games=1, n_playout=1)
    b = Board(width=15, height=15, n_in_row=5)
    b.init_board(0)
    codes = []
    for m in np.random.RandomState(3).permutation(225)[:30]:
        codes.append(b.position_codes())
        b.do_move(int(m))
    codes.append(b.position_codes())
    codes = np.stack(codes)
    # empty and all four ages (the player to move placed the stones of odd age, so 1 + age is even and 5 + age odd)
    assert set(int(c) for c in np.unique(codes[:, :225])) == {0, 2, 4, 5, 7, 8}
    assert set(int(c) for c in codes[:, 225]) == {0, 1}
    np.testing.assert_array_equal(planes_to_codes(pool.codes_to_planes(codes, 9)), codes)
    # ... and every code value a row can carry, wherever it stands
    rs = np.random.RandomState(4)
    anyc = np.zeros((6, pool.code_stride), np.uint8)
    anyc[:, :225] = rs.randint(0, 9, (6, 225))
    anyc[:, 225] = np.arange(6) % 2
    np.testing.assert_array_equal(planes_to_codes(pool.codes_to_planes(anyc, 9)), anyc)
    pool.close()


def test_extend_planes_stores_the_codes_and_refuses_other_planes():
    b = Board(width=8, height=8, n_in_row=4)
    b.init_board(1)
    states = []
    for m in (27, 28, 35, 36, 20):
        b.do_move(m)
        states.append(np.ascontiguousarray(b.current_state(), dtype=np.float32))
    buf = CompactReplayBuffer(64, 8, 8, 9)
    pis = np.full((5, 64), 1.0 / 64, np.float32)
    buf.extend_planes(np.stack(states), pis, [1.0, -1.0, 1.0, -1.0, 1.0])
    assert len(buf) == 40
    s, p, z = buf.entry(6 + 8 * 4)                       # the identity image of the last tuple
    np.testing.assert_array_equal(s, states[4])
    assert z == 1.0
    bad = np.stack(states)
    bad[0, 6] = bad[0, 7] = 1.0                          # own and opponent stones on the same cells
    with pytest.raises(ValueError):
        buf.extend_planes(bad, pis, np.zeros(5))
