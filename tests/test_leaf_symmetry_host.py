"""Dihedral leaf symmetry, the parts that need no GPU: the key function against a numpy restatement of its formula, the
facts about the permutation tables the kernels rest on (csrc/leaf_sym.h), the binding's refusals and the pipeline's
configuration keys (stand-in evaluator and trainer, tests/_pipeline_worker.py)."""
import numpy as np
import pytest

from _pipeline_worker import TiltNet, TiltTrainer
from alphapig_amd import checkpoint
from alphapig_amd.augment import dihedral_tables, get_equi_data, leaf_symmetry_keys
from alphapig_amd.pipeline import TrainPipeline
from alphapig_amd.treepool import TreePool

U = np.uint64
SIDES = (6, 8, 9, 15)
SEEDS = (0, 1, 77, 2 ** 63 + 5, 2 ** 64 - 1)


def _fmix64(x):
    x = x.copy()
    x ^= x >> U(33)
    x *= U(0xff51afd7ed558ccd)
    x ^= x >> U(33)
    x *= U(0xc4ceb9fe1a85ec53)
    x ^= x >> U(33)
    return x


def keys_restated(codes, hw, seed):
    """the formula of include/alphapig_hip.h (apz_leaf_symmetry_keys) in numpy uint64 arithmetic (wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        i = np.arange(hw + 1, dtype=U)[None, :]
        t = _fmix64(U(seed) + U(0x9E3779B97F4A7C15) * (U(256) * i + codes[:, :hw + 1].astype(U) + U(1)))
        return (_fmix64(U(seed) ^ t.sum(axis=1, dtype=U)) >> U(61)).astype(np.uint8)


def _stride(hw):
    return (hw + 1 + 15) // 16 * 16


def random_rows(side, n, rs):
    hw = side * side
    c = np.zeros((n, _stride(hw)), np.uint8)
    c[:, :hw] = rs.randint(0, 9, (n, hw)) * (rs.rand(n, hw) < rs.rand(n, 1))        # from nearly empty to nearly full
    c[:, hw] = rs.randint(0, 2, n)
    return c


@pytest.mark.parametrize("side", SIDES)
def test_keys_are_the_formula(side):
    hw = side * side
    rs = np.random.RandomState(side)
    rows = random_rows(side, 2000, rs)
    empty = np.zeros((2, _stride(hw)), np.uint8)
    empty[1, hw] = 1                                        # the empty board, either colour to move
    base = random_rows(side, 1, rs)
    one_byte = np.repeat(base, hw + 1, axis=0)              # rows that differ from `base` in exactly one byte
    for p in range(hw + 1):
        one_byte[p, p] = (one_byte[p, p] + 1) % (9 if p < hw else 2)
    seen = set()
    for seed in SEEDS:
        for codes in (rows, empty, base, one_byte):
            want = keys_restated(codes, hw, seed)
            assert want.max() <= 7
            np.testing.assert_array_equal(leaf_symmetry_keys(codes, seed), want)
        want = keys_restated(rows, hw, seed)
        assert set(want.tolist()) == set(range(8))          # every k occurs (on the restatement first)
        assert set(leaf_symmetry_keys(rows, seed).tolist()) == set(range(8))
        seen.add(tuple(want[:64].tolist()))
        # a one-byte change moves the key like a fresh draw would, not stuck on the base row's k: hw + 1 >= 37 draws from
        # eight values show fewer than four of them with probability below 1e-9
        assert len(set(keys_restated(one_byte, hw, seed).tolist())) >= 4
    assert len(seen) == len(SEEDS)                          # the seed matters
    # pad bytes are not part of the key
    padded = rows.copy()
    padded[:, hw + 1:] = 255
    np.testing.assert_array_equal(leaf_symmetry_keys(padded, 77), keys_restated(rows, hw, 77))
    assert leaf_symmetry_keys(rows[:0], 5).shape == (0,)


def test_keys_refuse_what_names_no_board():
    with pytest.raises(ValueError):
        leaf_symmetry_keys(np.zeros((3, 16), np.uint8), 0)          # boards of side 1 .. 3 share this stride
    with pytest.raises(ValueError):
        leaf_symmetry_keys(np.zeros(240, np.uint8), 0)
    with pytest.raises(ValueError):
        leaf_symmetry_keys(np.zeros((3, 240), np.uint8), 0, hw=240)  # the colour byte would lie outside the row
    assert leaf_symmetry_keys(np.zeros((3, 16), np.uint8), 0, hw=9).shape == (3,)


def image_rows(codes, side, k):
    """image k of every code row, as csrc/leaf_sym.h defines it"""
    hw = side * side
    pp = dihedral_tables(side)[1]
    out = np.zeros_like(codes)
    out[:, :hw] = codes[:, pp[k]]
    out[:, hw] = codes[:, hw]
    return out


@pytest.mark.parametrize("side", SIDES)
def test_table_facts(side):
    hw = side * side
    ps, pp = dihedral_tables(side)
    ident = np.arange(hw)
    np.testing.assert_array_equal(pp[6], ident)
    np.testing.assert_array_equal(ps[6], ident)
    rows = [tuple(r) for r in pp]
    assert len(set(rows)) == 8 and all(sorted(r) == list(range(hw)) for r in rows)
    for a in range(8):                                      # closed under composition, every inverse a table row
        inv = np.empty(hw, np.int64)
        inv[pp[a]] = ident
        assert tuple(inv) in rows
        for b in range(8):
            assert tuple(pp[a][pp[b]]) in rows
    # a code row's image is the code row of get_equi_data's k-th image: encode(codes_k) == encode(codes)[:, perm_s[k]]
    pool = TreePool(side, side, min(side, 5), n_games=1, n_playout=2)
    try:
        codes = random_rows(side, 6, np.random.RandomState(100 + side))
        codes[0, :hw] = 0                                   # the empty board
        codes[1, :hw] = 0
        codes[1, 0] = 1                                     # a lone corner stone
        for c_in in (9, 4):
            planes = pool.codes_to_planes(codes, c_in)
            equi = get_equi_data([(planes[i], np.arange(hw, dtype=np.float64), 0.0) for i in range(len(codes))], side, side)
            for k in range(8):
                got = pool.codes_to_planes(image_rows(codes, side, k), c_in)
                np.testing.assert_array_equal(got.reshape(len(codes), c_in, hw), planes.reshape(len(codes), c_in, hw)[:, :, ps[k]])
                for i in range(len(codes)):
                    np.testing.assert_array_equal(got[i], equi[8 * i + k][0])
                    # folding back: image k's pi is pi[perm_p[k]], so probs[perm_p[k][p]] = q_k[p] restores the position's
                    folded = np.empty(hw)
                    folded[pp[k]] = equi[8 * i + k][1]
                    np.testing.assert_array_equal(folded, np.arange(hw))
    finally:
        pool.close()


def test_the_binding_refuses_bad_modes_before_it_looks_for_a_gpu(monkeypatch):
    from alphapig_amd import _native, policy_value_net
    from alphapig_amd.policy_value_net import LanedEvaluator, PolicyValueNet, check_leaf_symmetry

    def no_library():
        raise AssertionError("a bad mode must be refused before the native library is touched")
    monkeypatch.setattr(_native, "hip", no_library)
    for bad in ("mean", "MEAN8", "", None, 3, True):
        with pytest.raises(ValueError, match="leaf_symmetry"):
            PolicyValueNet(15, 15, batch_size=4, n_blocks=1, leaf_symmetry=bad)
        with pytest.raises(ValueError):
            check_leaf_symmetry(bad)
    assert policy_value_net.LEAF_SYMMETRIES == {"none": 0, "keyed": 1, "mean8": 2}

    class Lane(object):
        n_slots, batchsize, hw, code_stride = 3, 4, 225, 240

        def __init__(self):
            self.calls = []

        def set_leaf_symmetry(self, mode, seed=None):
            self.calls.append((mode, seed))
    net = PolicyValueNet.__new__(PolicyValueNet)              # the setter of a net that was never created: no engine to reach
    with pytest.raises(ValueError, match="leaf_symmetry"):
        net.set_leaf_symmetry("keyed8")
    lanes = LanedEvaluator([Lane(), Lane(), Lane()])
    with pytest.raises(ValueError):
        lanes.set_leaf_symmetry("bogus", 1)
    assert all(ln.calls == [] for ln in lanes.lanes)
    lanes.set_leaf_symmetry("keyed", 9)
    assert all(ln.calls == [("keyed", 9)] for ln in lanes.lanes)  # every lane


def test_abi_constants_and_symbols():
    import os
    import re
    from alphapig_amd import _native
    hdr = open(os.path.join(os.path.dirname(_native.PKG), "include", "alphapig_hip.h")).read()
    for name, val in (("APZ_SYM_NONE", 0), ("APZ_SYM_KEYED", 1), ("APZ_SYM_MEAN8", 2), ("APZ_K_COUNT", 6)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr)
    for sym in ("apz_set_leaf_symmetry", "apz_get_leaf_symmetry", "apz_leaf_symmetry_keys"):
        assert sym in _native.HIP_SYMBOLS and hasattr(_native.hip(), sym)


# ---- the pipeline's configuration keys
class SymNet(TiltNet):
    """... that records what it is told about symmetry"""

    def __init__(self, hw):
        TiltNet.__init__(self, hw)
        self.leaf_symmetry, self.calls = "none", []

    def set_leaf_symmetry(self, mode, seed=None):
        self.calls.append((mode, seed))
        self.leaf_symmetry = mode


def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 4, "c_puct": 5, "buffer_size": 301, "batch_size": 16, "epochs": 1, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 1, "play_batch_size": 1, "pure_mcts_playout_num": 4, "eval_games": 1,
         "async_update": False, "concurrent_games": 2, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


class _Trainer(TiltTrainer):
    def state(self):
        return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

    def load_state(self, state):
        self._p = {"w": np.array(state["p/w"], np.float32), "b": np.array(state["p/b"], np.float32)}
        self.t = int(state["meta"]["t"])


def _pipe(conf, net=None, eval_net=None, resume=None, seed=77):
    net = net or SymNet(64)
    return TrainPipeline(conf, policy_value_net=net, seed=seed, trainer=_Trainer(net), eval_net=eval_net, distributed=False,
                         resume=resume), net


def test_conf_keys_reach_the_evaluators(tmp_path):
    pipe, net = _pipe(_conf(tmp_path))
    assert (pipe.leaf_symmetry, pipe.arena_symmetry, pipe.symmetry_seed) == ("none", "none", 77) and net.calls == []
    pipe.policy_evaluate(1)
    assert net.calls == []                                  # nothing is on: the evaluator is never told anything
    pipe.engine.close()
    # the self-play evaluator gets leaf_symmetry and the run's seed; the arena on the same evaluator holds arena_symmetry for its
    # duration and gives the evaluator back as it found it
    pipe, net = _pipe(_conf(tmp_path, leaf_symmetry="keyed", arena_symmetry="mean8"))
    assert net.calls == [("keyed", 77)]
    pipe.policy_evaluate(1)
    assert net.calls == [("keyed", 77), ("mean8", 77), ("keyed", 77)] and net.leaf_symmetry == "keyed"
    pipe.engine.close()
    # an arena evaluator of its own; an explicit seed
    arena_net = SymNet(64)
    pipe, net = _pipe(_conf(tmp_path, leaf_symmetry="keyed", arena_symmetry="mean8", symmetry_seed=2 ** 40 + 3), eval_net=arena_net)
    assert net.calls == [("keyed", 2 ** 40 + 3)] and arena_net.calls == []
    pipe.policy_evaluate(1, net=arena_net)
    assert arena_net.calls == [("mean8", 2 ** 40 + 3), ("none", 2 ** 40 + 3)] and len(net.calls) == 1
    pipe.engine.close()
    # equal modes on one evaluator: no switching around the arena
    pipe, net = _pipe(_conf(tmp_path, leaf_symmetry="keyed", arena_symmetry="keyed"))
    pipe.policy_evaluate(1)
    assert net.calls == [("keyed", 77)]
    pipe.engine.close()


def test_bad_keys_and_evaluators_without_the_method_raise(tmp_path):
    for key in ("leaf_symmetry", "arena_symmetry"):
        with pytest.raises(ValueError, match=key):
            _pipe(_conf(tmp_path, **{key: "mean9"}))
        with pytest.raises(ValueError, match="set_leaf_symmetry"):
            _pipe(_conf(tmp_path, **{key: "keyed"}), net=TiltNet(64))
    with pytest.raises(ValueError, match="set_leaf_symmetry"):
        _pipe(_conf(tmp_path, arena_symmetry="mean8"), eval_net=TiltNet(64))
    pipe, _ = _pipe(_conf(tmp_path), net=TiltNet(64))       # mode "none" asks nothing of the evaluator
    pipe.engine.close()
    with pytest.raises(ValueError, match="eval_net"):       # one evaluator cannot hold two modes at once
        _pipe(_conf(tmp_path, async_update=True, leaf_symmetry="keyed"))


def test_checkpoints_carry_the_keys_only_when_a_mode_is_on(tmp_path):
    import os
    plain = _conf(tmp_path / "plain", checkpoint_every=1)
    pipe, _ = _pipe(plain)
    pipe.run()
    pipe.engine.close()
    p_plain = os.path.join(plain["model_dir"], "checkpoints", "ckpt_%08d" % 1)
    state = checkpoint.read_state(p_plain)
    assert not any(k in state for k in ("leaf_symmetry", "arena_symmetry", "symmetry_seed"))
    keyed = _conf(tmp_path / "keyed", checkpoint_every=1, leaf_symmetry="keyed")
    pipe, _ = _pipe(keyed)
    pipe.run()
    pipe.engine.close()
    p_keyed = os.path.join(keyed["model_dir"], "checkpoints", "ckpt_%08d" % 1)
    state = checkpoint.read_state(p_keyed)
    assert (state["leaf_symmetry"], state["arena_symmetry"], state["symmetry_seed"]) == ("keyed", "none", 77)
    # resume: the keys must match; a checkpoint without them is one written with "none"
    again, net = _pipe(keyed, resume=p_keyed)
    assert net.calls == [("keyed", 77)]
    again.engine.close()
    again, _ = _pipe(plain, resume=p_plain)
    again.engine.close()
    with pytest.raises(ValueError, match="leaf_symmetry"):
        _pipe(plain, resume=p_keyed)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        _pipe(keyed, resume=p_plain)
    with pytest.raises(ValueError, match="arena_symmetry"):
        _pipe(dict(keyed, arena_symmetry="mean8"), resume=p_keyed)
    with pytest.raises(ValueError, match="symmetry_seed"):
        _pipe(dict(keyed, symmetry_seed=78), resume=p_keyed)
