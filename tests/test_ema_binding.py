"""CPU-side checks of the averaged weights' interface (HipTrainer(ema_decay=, ema_warmup=); csrc/ema.h): the entry point in the
header, the library and the binding; the coefficient's schedule; what ema_decay admits, before anything looks for a GPU; and
TrainPipeline's side -- who gets the average (the self-play evaluator) and who the raw weights (the KL monitor's evaluator).
Stand-in evaluator and trainer (tests/_pipeline_worker.py), no GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from alphapig_amd import _native, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.is_available() -> False: a refusal that comes after the GPU check shows as a RuntimeError, on every machine"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_entry_point_in_header_library_and_binding():
    L = _native.hip()
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    assert re.search(r"\bint\s+apz_ema_update\s*\(\s*apz_engine\s*\*", hdr)
    assert "apz_ema_update" in _native.HIP_SYMBOLS and hasattr(L, "apz_ema_update")
    # engine, table, ntensors, c, skip_a, skip_b, stream
    assert len(L.apz_ema_update.argtypes) == 7
    assert "csrc/ema.h" in hdr
    from alphapig_amd import hipconv
    assert list(inspect.signature(hipconv.ema_update).parameters) == ["entries", "c", "device", "skip", "skip2"]


# ---- the coefficient ---------------------------------------------------------------------------------------------------
def test_coefficient_schedule():
    from alphapig_amd.train import ema_coefficient
    c0 = ema_coefficient(0.999, 0, True)
    assert isinstance(c0, np.float32) and c0 == np.float32(0.9)
    assert ema_coefficient(0.999, 0, False) == np.float32(1 - 0.999)
    for decay in (0.5, 0.9, 0.999, 0.9999):
        cs = [ema_coefficient(decay, n, True) for n in range(0, 120000, 7)]
        assert all(isinstance(c, np.float32) for c in cs)
        assert all(a >= b for a, b in zip(cs, cs[1:])), decay                   # non-increasing in n
        first = next(n for n in range(200000) if (1 + n) / (10 + n) >= decay)
        for n in (first, first + 1, first + 1000):
            assert ema_coefficient(decay, n, True) == np.float32(1 - decay)
        if first > 0:
            assert ema_coefficient(decay, first - 1, True) > np.float32(1 - decay)
        assert all(ema_coefficient(decay, n, False) == np.float32(1 - decay) for n in (0, 1, 5, first))


@pytest.mark.parametrize("d", [0, 1, 1.5, -0.1, float("nan"), float("inf")])
def test_ema_decay_must_lie_strictly_between_0_and_1(d, no_gpu):
    from alphapig_amd.train import HipTrainer
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=1, style="bench")
    with pytest.raises(ValueError, match="ema_decay"):               # (a RuntimeError here would be the GPU check coming first)
        HipTrainer(prm, "resnet", 1, batch_size=8, ema_decay=d)


def test_good_settings_reach_the_gpu_check(no_gpu):
    from alphapig_amd.train import HipTrainer
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=1, style="bench")
    for kw in ({"ema_decay": 0.999}, {"ema_decay": 0.5, "ema_warmup": False}, {"ema_decay": None}):
        with pytest.raises(RuntimeError, match="needs a GPU"):
            HipTrainer(prm, "resnet", 1, batch_size=8, **kw)


def test_net_takes_the_two_keywords():
    """(that train_step hands them to its HipTrainer: tests/test_gpu_ema.py)"""
    from alphapig_amd.policy_value_net import PolicyValueNet
    sig = inspect.signature(PolicyValueNet.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is True
    assert callable(PolicyValueNet.ema_params)


# ---- TrainPipeline -----------------------------------------------------------------------------------------------------
def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 1000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 3, "play_batch_size": 2, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


def _classes():
    from _pipeline_worker import TiltNet, TiltTrainer

    class LogNet(TiltNet):
        """TiltNet that remembers every w it was given"""

        def __init__(self, hw):
            TiltNet.__init__(self, hw)
            self.given, self.seen = [], []

        def set_params(self, prm, _keep_trainer=False):
            TiltNet.set_params(self, prm, _keep_trainer)
            self.given.append(self._p["w"].copy())

        def policy_value(self, states):
            self.seen.append(self._p["w"].copy())              # the weights this forward ran on
            return TiltNet.policy_value(self, states)

    class EmaTilt(TiltTrainer):
        """TiltTrainer with HipTrainer's averaged weights (decay 0.5, no warm-up: the average is never the raw weights once
        they have moved) and an evaluator of its own for the KL monitor"""

        def __init__(self, net):
            TiltTrainer.__init__(self, net)
            self.ema_p = {k: v.copy() for k, v in self._p.items()}
            self.ema_updates = 0
            self.own = LogNet(len(self._p["w"]))
            self.raw_log = []

        def train_step(self, states, pis, zs, lr):
            out = TiltTrainer.train_step(self, states, pis, zs, lr)
            for k in self.ema_p:
                self.ema_p[k] = (self.ema_p[k] + np.float32(0.5) * (self._p[k] - self.ema_p[k])).astype(np.float32)
            self.ema_updates += 1
            self.raw_log.append(self._p["w"].copy())
            return out

        def ema_params(self):
            return {k: v.copy() for k, v in self.ema_p.items()}

        def policy_value(self, states):
            self.own.set_params(self._p)
            return self.own.policy_value(states)

        def state(self):
            out = {"meta": {"t": self.t, "ema_updates": self.ema_updates}}
            for k in ("w", "b"):
                out["p/" + k], out["e/" + k] = self._p[k].copy(), self.ema_p[k].copy()
            return out

        def load_state(self, state):
            self._p = {k: np.array(state["p/" + k], np.float32) for k in ("w", "b")}
            self.ema_p = {k: np.array(state["e/" + k], np.float32) for k in ("w", "b")}
            self.t, self.ema_updates = int(state["meta"]["t"]), int(state["meta"]["ema_updates"])

    return LogNet, EmaTilt, TiltTrainer


def _pipeline(tmp_path, trainer_cls=None, **kw):
    from alphapig_amd.pipeline import TrainPipeline
    LogNet, EmaTilt, _ = _classes()
    net = LogNet(64)
    trainer = (trainer_cls or EmaTilt)(net)
    return TrainPipeline(_conf(tmp_path, **kw), policy_value_net=net, seed=1, trainer=trainer, distributed=False), net, trainer


def test_lock_step_plays_on_the_average_and_monitors_on_the_raw_weights(tmp_path):
    pipe, net, tr = _pipeline(tmp_path, ema_decay=0.5)
    hist = pipe.run()
    pipe.engine.close()
    upd = [r for r in hist if "loss" in r]
    assert upd and tr.ema_updates == tr.t > 0
    assert upd[-1]["ema_updates"] == tr.ema_updates and all(r["ema_updates"] > 0 for r in upd)
    # the self-play evaluator: the averaged values, installed once per update -- and never a raw weight vector
    assert np.array_equal(net.params()["w"], tr.ema_params()["w"]) and np.array_equal(net.params()["b"], tr.ema_params()["b"])
    assert not np.array_equal(net.params()["w"], tr.get_params()["w"])
    assert len(net.given) == len(upd)
    assert not any(np.array_equal(g, raw) for g in net.given for raw in tr.raw_log)
    # the evaluator that served the KL forwards: the raw ones, old and new forward of every update
    assert np.array_equal(tr.own.params()["w"], tr.get_params()["w"])
    assert len(tr.own.given) == len(upd) + tr.t
    assert all(np.array_equal(g, raw) for g, raw in zip(tr.own.given[-1:], tr.raw_log[-1:]))


def test_pipeline_takes_and_matches_the_keys(tmp_path):
    for kw, decay, warm in (({}, None, True), ({"ema_decay": 0.999}, 0.999, True), ({"ema_decay": 0.9, "ema_warmup": False}, 0.9, False)):
        pipe, _, _ = _pipeline(tmp_path, **kw)
        assert pipe.ema_decay == decay and pipe.ema_warmup is warm
        assert pipe._conf_match["ema_decay"] == decay and pipe._conf_match["ema_warmup"] is warm
        pipe.engine.close()
    for bad in (0, 1, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            _pipeline(tmp_path, ema_decay=bad)


def test_a_trainer_without_the_average_is_refused(tmp_path):
    _, _, TiltTrainer = _classes()
    with pytest.raises(ValueError, match="ema_decay"):
        _pipeline(tmp_path, trainer_cls=TiltTrainer, ema_decay=0.999)
    pipe, _, _ = _pipeline(tmp_path, trainer_cls=TiltTrainer)             # without the key it is welcome, as always
    pipe.engine.close()


def test_a_trainer_built_without_the_average_is_refused(tmp_path):
    """HipTrainer(ema_decay=None) has the names -- ema_p is None, ema_params() raises: refused at construction all the same"""
    _, EmaTilt, _ = _classes()

    class Off(EmaTilt):
        def __init__(self, net):
            EmaTilt.__init__(self, net)
            self.ema_p, self.ema_decay = None, None

        def ema_params(self):
            raise ValueError("this trainer keeps no averaged weights (ema_decay=None)")

    with pytest.raises(ValueError, match="ema_decay"):
        _pipeline(tmp_path, trainer_cls=Off, ema_decay=0.999)


def test_the_first_forward_after_an_asynchronous_resume_sees_the_raw_weights(tmp_path):
    """The asynchronous schedule with an evaluator of the trainer thread's own: every forward of the KL monitor runs on the
    raw weights -- also the first one after a resume, when that evaluator holds something else (built from the self-play
    evaluator it would hold the average; this fresh stand-in holds zeros)."""
    from alphapig_amd import checkpoint
    from alphapig_amd.pipeline import TrainPipeline
    LogNet, EmaTilt, _ = _classes()
    conf = _conf(tmp_path, replay="compact", async_update=True, round_steps=24, kl_targ=1e9, play_batch_size=1,
                 checkpoint_every=4, checkpoint_keep=100, buffer_size=100000, ema_decay=0.5)

    def build(n, resume=None):
        net, kl_net = LogNet(64), LogNet(64)
        tr = EmaTilt(net)
        pipe = TrainPipeline(dict(conf, game_batch_num=n), policy_value_net=net, seed=77, trainer=tr, eval_net=kl_net,
                             distributed=False, resume=resume)
        return pipe, net, kl_net, tr

    first, net, kl_net, tr = build(9)
    first.run()
    first.engine.close()
    # the uninterrupted run: each update's old forward ran on the raw weights the update before left, the first on the initial ones
    assert tr.t > 0 and len(kl_net.seen) > 0 and not tr.own.seen
    assert np.array_equal(kl_net.seen[0], np.zeros(64, np.float32))
    assert all(any(np.array_equal(w, raw) for raw in tr.raw_log) for w in kl_net.seen[1:])
    done = checkpoint.complete_checkpoints(os.path.join(conf["model_dir"], "checkpoints"))
    assert done
    path = done[0]
    tstate = checkpoint.read_part(path, "trainer")
    raw, avg = np.asarray(tstate["p/w"], np.float32), np.asarray(tstate["e/w"], np.float32)
    assert int(tstate["meta"]["t"]) > 0 and not np.array_equal(raw, avg)
    second, net2, kl_net2, tr2 = build(14, resume=path)
    assert np.array_equal(net2.params()["w"], avg)             # what plays after the resume is the average
    assert np.array_equal(tr2.get_params()["w"], raw) and not kl_net2.seen
    second.run()
    second.engine.close()
    assert tr2.t > int(tstate["meta"]["t"]) and kl_net2.seen
    assert np.array_equal(kl_net2.seen[0], raw)                # the first old forward: the raw weights of the checkpoint
    assert not any(np.array_equal(w, avg) for w in kl_net2.seen)


def test_ema_update_refuses_a_foreign_table():
    from alphapig_amd import hipconv
    for tab in (np.zeros(3, np.float32), np.zeros((2, 3), np.uint64), np.zeros(2, [("s", "u8"), ("w", "u8")])):
        with pytest.raises(ValueError, match="ema_table"):
            hipconv.ema_update(tab, 0.5, None)


def test_without_the_key_the_history_is_todays(tmp_path):
    """Same seed, the key absent / None, a trainer with or without the average: one history, the raw weights in the self-play
    evaluator (what the KL monitor left there), no ema_updates in any record"""
    _, EmaTilt, TiltTrainer = _classes()
    runs = []
    for name, cls, kw in (("a", TiltTrainer, {}), ("b", EmaTilt, {}), ("c", EmaTilt, {"ema_decay": None})):
        pipe, net, tr = _pipeline(tmp_path / name, trainer_cls=cls, **kw)
        hist = pipe.run()
        pipe.engine.close()
        assert any("loss" in r for r in hist) and all("ema_updates" not in r for r in hist)
        assert np.array_equal(net.params()["w"], tr.get_params()["w"])
        runs.append((hist, net.params()["w"], len(net.given)))
    for hist, w, given in runs[1:]:
        assert hist == runs[0][0] and np.array_equal(w, runs[0][1]) and given == runs[0][2]
