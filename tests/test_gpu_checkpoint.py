"""Checkpoints on the GPU: HipTrainer.state / load_state (weights, BatchNorm statistics, Adam moments, step and dropout
counters), DeviceReplayBuffer.state / load_state, the lock-step TrainPipeline stopped and resumed, and a calibrated
f16x2 evaluator through a checkpoint.  Everything is compared bit for bit."""
import random

import numpy as np
import pytest

from _replay_games import random_game_tuples
from alphapig_amd import checkpoint, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NETS = [("resnet", 15, 1, "f32"), ("resnet", 15, 1, "f16x2"), ("simple", 8, 0, "f32")]


def _problem(kind, side, n, blocks, seed):
    rs = np.random.RandomState(seed)
    prm = weights.init_params(kind, side, side, 9, blocks, 128, seed=seed + 1, style="bench")
    states = (rs.rand(n, 9, side, side) > 0.6).astype(np.float32)
    pis = rs.dirichlet(np.ones(side * side), size=n).astype(np.float32)
    zs = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    return prm, states, pis, zs


def _host(group):
    return {k: v.cpu().numpy() for k, v in group.items()}


def _same(a, b, what):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("kind,side,blocks,arith", NETS)
def test_a_reloaded_trainer_takes_the_steps_of_the_one_that_went_on(tmp_path, kind, side, blocks, arith):
    from alphapig_amd.train import HipTrainer
    prm, states, pis, zs = _problem(kind, side, 16, blocks, seed=3)
    make = lambda p, **kw: HipTrainer(p, kind, n_blocks=blocks, batch_size=16, dropout=0.5, seed=5, trunk_arith=arith, **kw)
    a = make(prm)
    for _ in range(3):
        a.train_step(states, pis, zs, 2e-3)
    checkpoint.write_part(str(tmp_path), "trainer", a.state())
    state = checkpoint.read_part(str(tmp_path), "trainer")
    assert state["meta"]["t"] == 3 and state["meta"]["seed"] == 5 and state["meta"]["dropout_step0"] == 0
    other = weights.init_params(kind, side, side, 9, blocks, 128, seed=99, style="bench")
    b = make(other, dropout_step0=7)                        # everything of it is replaced
    views = {k: b.p[k].data_ptr() for k in b.p}
    b.load_state(state)
    assert views == {k: b.p[k].data_ptr() for k in b.p} and (b.t, b.dropout_step0, b._eval_t) == (3, 0, -1)
    c = make(a.get_params(), dropout_step0=3)               # the control: the weights alone, Adam starts over
    out = {}
    for name, tr in (("a", a), ("b", b), ("c", c)):
        out[name] = [tr.train_step(states, pis, zs, 2e-3) for _ in range(2)]
    assert out["a"] == out["b"]
    for group in ("p", "m", "v"):
        _same(_host(getattr(a, group)), _host(getattr(b, group)), group)
    assert (a.t, a.trunk_overflows) == (b.t, b.trunk_overflows) and a.t == 5
    ma, mc = _host(a.m), _host(c.m)
    assert any(ma[k].tobytes() != mc[k].tobytes() for k in ma)
    pa, va = a.policy_value(states)
    pb, vb = b.policy_value(states)
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    with pytest.raises(ValueError):
        b.load_state({k: v for k, v in state.items() if k != "m/fc_3_1_1_weight"})
    for tr in (a, b, c):
        tr.close()


@pytest.mark.parametrize("maxlen,n_tuples", [(301, 90), (8, 5), (100000, 37)])
def test_device_buffer_round_trip(tmp_path, maxlen, n_tuples):
    from alphapig_amd.replay import CompactReplayBuffer, DeviceReplayBuffer
    from test_replay_checkpoint import SIDE, check_round_trip
    check_round_trip(lambda m: DeviceReplayBuffer(m, SIDE, SIDE, 9), maxlen, n_tuples,
                     other=lambda m: CompactReplayBuffer(m, SIDE, SIDE, 9))
    # ... and through the files of a checkpoint
    a = DeviceReplayBuffer(maxlen, SIDE, SIDE, 9)
    codes, pis, zs = random_game_tuples(SIDE, 4, n_tuples, seed=2)
    a.extend_codes(codes, pis, zs)
    checkpoint.write_part(str(tmp_path), "buffer", a.state())
    b = DeviceReplayBuffer(maxlen, SIDE, SIDE, 9)
    b.load_state(checkpoint.read_part(str(tmp_path), "buffer"))
    k = min(16, len(a))
    for x, y in zip(a.sample(random.Random(3), k), b.sample(random.Random(3), k)):
        assert x.is_cuda and y.is_cuda and torch.equal(x, y)


def _conf(tmp_path, replay, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 301, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 6, "play_batch_size": 2, "pure_mcts_playout_num": 10,
         "async_update": False, "concurrent_games": 8, "n_blocks": 1, "n_filter": 64,
         "model_dir": str(tmp_path / "models"), "replay": replay}
    c.update(kw)
    return c


@pytest.mark.parametrize("replay", ["device", "tuples"])
def test_lock_step_pipeline_resumed_is_the_pipeline_that_went_on(tmp_path, replay):
    """(two plain runs of this configuration are bit-equal: profiles/r13_device_replay.md)"""
    from alphapig_amd.pipeline import TrainPipeline
    key = lambda hist: [(r["buffer"], r.get("loss"), r.get("entropy"), r.get("kl")) for r in hist]
    whole = TrainPipeline(_conf(tmp_path / "whole", replay), device=0, seed=5, distributed=False)
    want = (key(whole.run()), whole.lr_multiplier, whole._trainer().get_params())
    whole.close()
    conf = _conf(tmp_path / "cut", replay, checkpoint_every=3, checkpoint_buffer=True)
    first = TrainPipeline(dict(conf, game_batch_num=3), device=0, seed=5, distributed=False)
    first.run()
    first.close()
    path = checkpoint.complete_checkpoints(first.checkpoint_dir)[-1]
    assert path.endswith("ckpt_00000003") and checkpoint.has_part(path, "trainer") and checkpoint.has_part(path, "buffer")
    second = TrainPipeline(conf, device=0, seed=5, distributed=False, resume=path)
    got = (key(second.run()), second.lr_multiplier, second._trainer().get_params())
    second.close()
    assert got[0] == want[0] and len(got[0]) == 6 and sum(r[1] is not None for r in got[0][3:]) >= 2
    assert got[1] == want[1]
    for k, v in want[2].items():
        np.testing.assert_array_equal(v, got[2][k], err_msg=k)


def test_a_calibrated_evaluator_comes_back_with_its_exponents(tmp_path):
    """15x15, f16x2: the self-play evaluator's activation exponents travel in state.json, and the evaluator of the resumed
    pipeline answers 33 boards (the batched kernel's side of the 32-board threshold) with the same bits.  No update has
    run, so the weights travel as the evaluator's own (part `weights`)."""
    from alphapig_amd.pipeline import TrainPipeline
    conf = _conf(tmp_path, "device", board_width=15, board_height=15, n_in_row=5, n_filter=128, concurrent_games=66,
                 n_playout=4)
    codes, _, _ = random_game_tuples(15, 5, 33, seed=8)
    a = TrainPipeline(conf, device=0, seed=5, distributed=False)
    net = a.policy_value_net
    assert net.trunk_arith == "f16x2"
    net.set_params(weights.init_params("resnet", 15, 15, 9, 1, 128, seed=31, style="bench"))    # not what seed 5 starts from
    net.calibrate_trunk(codes=codes)
    exps = net.trunk_act_exponents()
    assert len(exps) == 2 and any(exps)
    a.engine.run_steps(3)
    want = net.evaluate_codes(codes)
    path = a.save_checkpoint(str(tmp_path / "ckpt"))
    a.close()
    assert checkpoint.read_state(path)["act_exponents"] == exps and checkpoint.has_part(path, "weights")
    b = TrainPipeline(conf, device=0, seed=5, distributed=False, resume=path)
    assert b.policy_value_net.trunk_act_exponents() == exps
    got = b.policy_value_net.evaluate_codes(codes)
    assert b.policy_value_net.trunk_overflows() == 0
    b.close()
    for x, y in zip(want, got):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
