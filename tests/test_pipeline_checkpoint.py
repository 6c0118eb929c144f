"""TrainPipeline checkpoints: in lock step a run that is stopped after a checkpoint and resumed from it is the run that
was never stopped -- history, learning-rate multiplier, every mini-batch the trainer saw, the final buffer.  Stand-in
evaluator and trainer (tests/_pipeline_worker.py), no GPU."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from _pipeline_worker import TiltNet, TiltTrainer
from alphapig_amd import checkpoint
from alphapig_amd.pipeline import TrainPipeline

HERE = os.path.dirname(os.path.abspath(__file__))


class RecordingTrainer(TiltTrainer):
    """... that records its mini-batches and can be checkpointed"""

    def __init__(self, net):
        TiltTrainer.__init__(self, net)
        self.seen = []

    def train_step(self, states, pis, zs, lr):
        self.seen.append((np.array(states), np.array(pis), np.array(zs), lr))
        return TiltTrainer.train_step(self, states, pis, zs, lr)

    def state(self):
        return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

    def load_state(self, state):
        self._p = {"w": np.array(state["p/w"], np.float32), "b": np.array(state["p/b"], np.float32)}
        self.t = int(state["meta"]["t"])


def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 301, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 6, "play_batch_size": 2, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


def _pipe(conf, resume=None, seed=77):
    net = TiltNet(64)
    trainer = RecordingTrainer(net)
    pipe = TrainPipeline(conf, policy_value_net=net, seed=seed, trainer=trainer, eval_net=TiltNet(64), distributed=False,
                         resume=resume)
    return pipe, trainer


def _entries(buf):
    if hasattr(buf, "entry"):
        return [buf.entry(i) for i in range(len(buf))]
    return list(buf)


def _same_entries(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(x, y))


def _ckpt(conf, n):
    return os.path.join(conf["model_dir"], "checkpoints", "ckpt_%08d" % n)


@pytest.mark.parametrize("replay,extra", [("tuples", {"checkpoint_buffer": True}), ("compact", {})])
def test_lock_step_resume_is_the_uninterrupted_run(tmp_path, replay, extra):
    whole, t_whole = _pipe(_conf(tmp_path / "a", replay=replay))
    h_whole = whole.run()
    assert not os.path.exists(os.path.join(whole.model_dir, "checkpoints"))
    conf = _conf(tmp_path / "b", replay=replay, checkpoint_every=3, **extra)
    first, t_first = _pipe(dict(conf, game_batch_num=3))
    first.run()
    first.engine.close()
    path = _ckpt(conf, 3)
    assert os.path.exists(os.path.join(path, "COMPLETE")) and not os.path.exists(path + ".tmp")
    names = sorted(os.listdir(path))
    assert "state.json" in names and "selfplay_rank0.json" in names and "buffer.json" in names and "trainer.json" in names
    assert all(n.endswith((".json", ".npy")) or n == "COMPLETE" for n in names)
    second, t_second = _pipe(conf, resume=path)
    assert second.history == h_whole[:3] and second._batches_done == 3
    h = second.run()
    key = lambda hist: [(r["batch"], r["episode_len"], r["buffer"], r.get("loss"), r.get("entropy"), r.get("kl")) for r in hist]
    assert key(h) == key(h_whole) and len(h) == 6 and sum("loss" in r for r in h[3:]) >= 2
    assert second.lr_multiplier == whole.lr_multiplier and second._train_steps == whole._train_steps
    seen = t_first.seen + t_second.seen
    assert len(seen) == len(t_whole.seen) and len(t_second.seen) >= 2
    for a, b in zip(seen, t_whole.seen):
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    _same_entries(_entries(second.data_buffer), _entries(whole.data_buffer))
    for k in ("w", "b"):
        np.testing.assert_array_equal(t_second.get_params()[k], t_whole.get_params()[k])
        np.testing.assert_array_equal(second.policy_value_net.params()[k], whole.policy_value_net.params()[k])
    assert second.engine.next_index == whole.engine.next_index and second._taken == whole._taken
    assert os.path.exists(os.path.join(_ckpt(conf, 6), "COMPLETE"))
    whole.engine.close()
    second.engine.close()


def test_without_the_games_in_flight_no_game_reaches_the_trainer_twice(tmp_path):
    conf = _conf(tmp_path, replay="compact", checkpoint_every=3, checkpoint_selfplay="none", buffer_size=100000)
    first, _ = _pipe(dict(conf, game_batch_num=3))
    taken = []

    def spy(pipe, log):
        """the game indices a pipeline hands to its buffer, read off the engine's finished list as it is drained"""
        inner = pipe.collect_selfplay_data_ai

        def collect(n):
            while len(pipe.engine.finished) < n:
                pipe.engine.run_steps(16)
            log.extend(e.index for e in pipe.engine.finished[:n])
            return inner(n)
        pipe.collect_selfplay_data_ai = collect
    spy(first, taken)
    first.run()
    waiting = [e.index for e in first.engine.finished]
    next_index = first.engine.next_index
    first.engine.close()
    second, _ = _pipe(conf, resume=_ckpt(conf, 3))
    assert second.engine.next_index == next_index and [e.index for e in second.engine.finished] == waiting
    assert not any(s.active for s in second.engine.slots)
    spy(second, taken)
    second.run()
    assert len(taken) == 12 == len(set(taken))
    assert all(i in taken[6:6 + len(waiting)] for i in waiting[:6])
    second.engine.close()


def test_an_unfinished_or_foreign_checkpoint_is_refused(tmp_path):
    conf = _conf(tmp_path, replay="compact", checkpoint_every=3, game_batch_num=3)
    first, _ = _pipe(conf)
    first.run()
    first.engine.close()
    path = _ckpt(conf, 3)
    with pytest.raises(ValueError, match="batch_size"):
        _pipe(dict(conf, batch_size=8), resume=path)
    with pytest.raises(ValueError, match="replay"):
        _pipe(dict(conf, replay="tuples"), resume=path)
    os.remove(os.path.join(path, "COMPLETE"))
    with pytest.raises(ValueError, match="COMPLETE"):
        _pipe(conf, resume=path)
    with pytest.raises(ValueError, match="COMPLETE"):
        _pipe(conf, resume=str(tmp_path / "nowhere"))


def test_only_the_newest_checkpoints_stay_and_the_tuple_buffer_stays_home_by_default(tmp_path, caplog):
    conf = _conf(tmp_path, checkpoint_every=1, checkpoint_keep=2, game_batch_num=4)
    pipe, _ = _pipe(conf)
    pipe.run()
    pipe.engine.close()
    root = os.path.join(conf["model_dir"], "checkpoints")
    assert sorted(os.listdir(root)) == ["ckpt_00000003", "ckpt_00000004"]
    assert not checkpoint.has_part(_ckpt(conf, 4), "buffer")
    import logging
    with caplog.at_level(logging.INFO, logger="alphapig_amd.pipeline"):
        again, _ = _pipe(conf, resume=_ckpt(conf, 4))
    assert len(again.data_buffer) == 0 and sum("empty buffer" in r.getMessage() for r in caplog.records) == 1
    assert again.run() == pipe.history              # nothing left to do
    again.engine.close()


def test_asynchronous_resume_continues_the_buffer_and_the_update_count(tmp_path):
    conf = _conf(tmp_path, replay="compact", async_update=True, round_steps=24, kl_targ=1e9, play_batch_size=1,
                 checkpoint_every=4, checkpoint_keep=100, buffer_size=100000)
    first, _ = _pipe(dict(conf, game_batch_num=9))
    first.run()
    first.engine.close()
    done = checkpoint.complete_checkpoints(os.path.join(conf["model_dir"], "checkpoints"))
    assert done and all(os.path.basename(d) in ("ckpt_00000004", "ckpt_00000008", "ckpt_00000012") for d in done)
    path = done[0]
    state = checkpoint.read_state(path)
    # the cut: all games handed over up to the round that crossed the multiple are in the buffer, none twice
    rounds = [r for r in first.history if r["round"] <= state["round"]]
    assert state["games_collected"] == sum(r["games"] for r in rounds) == state["games_recv"] >= 4
    buf = checkpoint.read_part(path, "buffer")
    second, t_second = _pipe(dict(conf, game_batch_num=14), resume=path)
    assert second.data_buffer.ring.appended == buf["meta"]["appended"] == 8 * len(buf["codes"])
    assert len(second.data_buffer) == 8 * len(buf["codes"])
    sp = checkpoint.read_part(path, "selfplay_rank0")
    assert len(sp["fin_index"]) == 0                   # every finished game went to the trainer before the cut
    assert second.updates_done == state["updates_done"] and second._games_collected == state["games_collected"]
    saved_updates, saved_hist = state["updates_done"], len(state["trainer_history"])
    second.run()
    assert second.updates_done > saved_updates and second._games_collected >= 14
    assert second.trainer_history[:saved_hist] == state["trainer_history"]
    batches = [r["batch"] for r in second.trainer_history]
    assert batches == sorted(set(batches)) and second.history[len(state["history"])]["round"] == state["round"] + 1
    assert t_second.t == second._train_steps
    second.engine.close()


def test_two_ranks_in_lock_step_resume_to_the_uninterrupted_history(tmp_path):
    """gloo, world size 2: both ranks write their self-play parts, and the resumed pair reproduces rank 0's history"""
    def launch(out, *args):
        os.makedirs(out, exist_ok=True)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(27500 + random.randint(0, 2000)),
               os.path.join(HERE, "_checkpoint_worker.py"), out] + list(args)
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-4000:]
        return [json.load(open(os.path.join(out, "pipe%d.json" % k))) for k in range(2)]

    whole = launch(str(tmp_path / "whole"), "6", "0")
    launch(str(tmp_path / "cut"), "3", "3")
    path = os.path.join(str(tmp_path / "cut"), "checkpoints", "ckpt_00000003")
    assert all(checkpoint.has_part(path, "selfplay_rank%d" % r) for r in range(2)) and os.path.exists(os.path.join(path, "COMPLETE"))
    resumed = launch(str(tmp_path / "cut"), "6", "3", path)
    assert resumed[0]["history"] == whole[0]["history"] and len(whole[0]["history"]) == 6
    assert sum("loss" in r for r in whole[0]["history"][3:]) >= 2
    assert resumed[0]["lr_multiplier"] == whole[0]["lr_multiplier"] and resumed[0]["trainer_w"] == whole[0]["trainer_w"]
    for r in range(2):
        assert resumed[r]["w"] == whole[r]["w"] and resumed[r]["next_index"] == whole[r]["next_index"]
