"""TrainPipeline's `replay` key: the host code buffer delivers the mini-batches, losses and learning-rate multiplier of the
default tuple buffer.  Stand-in evaluator and trainer (tests/_pipeline_worker.py), lock step, no GPU."""
import random

import numpy as np
import pytest

from _pipeline_worker import TiltNet, TiltTrainer
from alphapig_amd.pipeline import ReplayBuffer, TrainPipeline
from alphapig_amd.replay import CompactReplayBuffer


class RecordingTrainer(TiltTrainer):
    def __init__(self, net):
        TiltTrainer.__init__(self, net)
        self.seen = []

    def train_step(self, states, pis, zs, lr):
        self.seen.append((np.array(states), np.array(pis), np.array(zs), lr))
        return TiltTrainer.train_step(self, states, pis, zs, lr)


def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 100000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 3, "play_batch_size": 2, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


def _run(tmp_path, **kw):
    net = TiltNet(64)
    trainer = RecordingTrainer(net)
    pipe = TrainPipeline(_conf(tmp_path, **kw), policy_value_net=net, seed=77, trainer=trainer, distributed=False)
    hist = pipe.run()
    pipe.engine.close()
    return pipe, trainer, hist


@pytest.mark.parametrize("buffer_size", [100000, 301])           # 301: the ring wraps, inside a tuple
def test_compact_replay_trains_on_the_tuple_buffers_mini_batches(tmp_path, buffer_size):
    pa, ta, ha = _run(tmp_path, buffer_size=buffer_size)
    pb, tb, hb = _run(tmp_path, buffer_size=buffer_size, replay="compact")
    assert isinstance(pa.data_buffer, ReplayBuffer) and isinstance(pb.data_buffer, CompactReplayBuffer)
    assert len(ta.seen) == len(tb.seen) >= 4
    for a, b in zip(ta.seen, tb.seen):
        assert a[0].dtype == b[0].dtype == np.float32 and a[0].shape == (16, 9, 8, 8)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    key = lambda h: [(r["buffer"], r.get("loss"), r.get("entropy"), r.get("kl")) for r in h]
    assert key(ha) == key(hb) and sum("loss" in r for r in ha) >= 2
    assert pa.lr_multiplier == pb.lr_multiplier
    assert len(pa.data_buffer) == len(pb.data_buffer) == min(ha[-1]["buffer"], buffer_size)
    if buffer_size == 301:
        assert pa.data_buffer.maxlen == len(pa.data_buffer)
    for k in ("w", "b"):
        np.testing.assert_array_equal(ta.get_params()[k], tb.get_params()[k])


def test_default_replay_is_the_tuple_buffer_and_a_bad_value_raises(tmp_path):
    net = TiltNet(64)
    pipe = TrainPipeline(_conf(tmp_path), policy_value_net=net, seed=1, trainer=TiltTrainer(net), distributed=False)
    assert pipe.replay == "tuples" and type(pipe.data_buffer) is ReplayBuffer
    pipe.engine.close()
    with pytest.raises(ValueError, match="replay"):
        TrainPipeline(_conf(tmp_path, replay="gpu"), policy_value_net=net, seed=1, trainer=TiltTrainer(net), distributed=False)


def test_device_replay_needs_a_trainer_that_takes_device_batches(tmp_path):
    """(without a GPU the same construction fails for want of one: either way before anything is built)"""
    net = TiltNet(64)
    with pytest.raises(RuntimeError, match="replay='device'"):
        TrainPipeline(_conf(tmp_path, replay="device"), policy_value_net=net, seed=1, trainer=TiltTrainer(net), distributed=False)


def test_sgf_bootstrap_fills_the_code_buffer_with_the_same_entries(golden_dir, tmp_path):
    """Game records yield planes (train_mxnet.py:137-154): the code buffer stores the codes that reproduce them, and the
    bootstrap updates of the asynchronous schedule see the tuple buffer's mini-batches."""
    from test_pipeline_async import _sgf_dir
    sgf_home, good = _sgf_dir(golden_dir, tmp_path)
    recs = []
    for replay in ("tuples", "compact"):
        net = TiltNet(225)
        conf = _conf(tmp_path, board_width=15, board_height=15, n_in_row=5, n_playout=6, epochs=1, kl_targ=1e9,
                     game_batch_num=5, play_batch_size=1, async_update=True, round_steps=8, sgf_batches=4, sgf_dir=sgf_home,
                     replay=replay)
        trainer = RecordingTrainer(net)
        random.seed(9)                          # (the pipeline shuffles its game records with the global generator)
        pipe = TrainPipeline(conf, policy_value_net=net, seed=3, trainer=trainer, eval_net=TiltNet(225), distributed=False)
        pipe.run()
        sgf_recs = [r for r in pipe.trainer_history if r.get("sgf")]
        assert [r["batch"] for r in sgf_recs] == [1, 2, 3, 4] and sum("loss" in r for r in sgf_recs) >= 2
        n_sgf_steps = sum("loss" in r for r in sgf_recs)
        recs.append((sgf_recs, trainer.seen[:n_sgf_steps]))
        pipe.engine.close()
    assert recs[0][0] == recs[1][0]
    for a, b in zip(recs[0][1], recs[1][1]):
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
