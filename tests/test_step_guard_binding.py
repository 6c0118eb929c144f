"""CPU-side checks of the guarded optimiser step's interface (HipTrainer(step_guard=, clip_norm=); csrc/grad_guard.h): the two
entry points in the header, the library and the binding; what clip_norm admits, before anything looks for a GPU; TrainPipeline's
two conf keys, a checkpoint from before them, and policy_update's learning-rate multiplier when every step was skipped.
Stand-in evaluator and trainer (tests/_pipeline_worker.py), no GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from alphapig_amd import _native, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_SYMBOLS = ["apz_grad_norm", "apz_adam_step_guarded"]


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.is_available() -> False: a refusal that comes after the GPU check shows as a RuntimeError, on every machine"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_entry_points_in_header_library_and_binding():
    L = _native.hip()
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    for s in GUARD_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*apz_engine\s*\*" % s, hdr), s
        assert s in _native.HIP_SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    # apz_adam_step's arguments + clip, loss3, skip_in, record; the norm alone: without lr_t, b1, b2, eps
    assert len(L.apz_adam_step_guarded.argtypes) == len(L.apz_adam_step.argtypes) + 4
    assert len(L.apz_grad_norm.argtypes) == len(L.apz_adam_step_guarded.argtypes) - 4
    assert "csrc/grad_guard.h" in hdr and "rescale_eff" in hdr
    from alphapig_amd import hipconv
    for f in ("grad_norm", "adam_step_guarded"):
        assert callable(getattr(hipconv, f))


@pytest.mark.parametrize("clip", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_clip_norm_must_be_a_finite_positive_number(clip, no_gpu):
    from alphapig_amd.train import HipTrainer
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=1, style="bench")
    with pytest.raises(ValueError, match="clip_norm"):               # (a RuntimeError here would be the GPU check coming first)
        HipTrainer(prm, "resnet", 1, batch_size=8, clip_norm=clip)


def test_good_settings_reach_the_gpu_check(no_gpu):
    from alphapig_amd.train import HipTrainer
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=1, style="bench")
    for kw in ({"step_guard": True}, {"clip_norm": 2.5}, {"step_guard": True, "clip_norm": 1e-3}, {"step_guard": False, "clip_norm": None}):
        with pytest.raises(RuntimeError, match="needs a GPU"):
            HipTrainer(prm, "resnet", 1, batch_size=8, **kw)


def test_net_takes_the_two_keywords():
    """(that train_step hands them to its HipTrainer: tests/test_gpu_step_guard.py)"""
    from alphapig_amd.policy_value_net import PolicyValueNet
    sig = inspect.signature(PolicyValueNet.__init__).parameters
    assert sig["train_step_guard"].default is False and sig["train_clip_norm"].default is None


# ---- TrainPipeline ---------------------------------------------------------------------------------------------------
def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 1000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 2, "play_batch_size": 2, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


def _trainer_class():
    from _pipeline_worker import TiltTrainer

    class GuardedTilt(TiltTrainer):
        """TiltTrainer with HipTrainer's guard attributes: skips (changes nothing, keeps t) the steps whose index is in `bad`"""

        def __init__(self, net, bad=()):
            TiltTrainer.__init__(self, net)
            self.bad, self.asked = set(bad), 0
            self.skipped_steps = self.clipped_steps = 0
            self.last_grad_norm = self.last_skip_reason = None

        def train_step(self, states, pis, zs, lr):
            i, self.asked = self.asked, self.asked + 1
            if i in self.bad or "all" in self.bad:
                self.skipped_steps += 1
                self.last_grad_norm, self.last_skip_reason = float("nan"), "non-finite gradient"
                return float("nan"), float("nan")
            self.last_grad_norm, self.last_skip_reason = 0.25, None
            return TiltTrainer.train_step(self, states, pis, zs, lr)

        def state(self):
            return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

        def load_state(self, state):
            self._p = {"w": np.array(state["p/w"], np.float32), "b": np.array(state["p/b"], np.float32)}
            self.t = int(state["meta"]["t"])
    return GuardedTilt


def _pipeline(tmp_path, bad=(), resume=None, **kw):
    from _pipeline_worker import TiltNet
    from alphapig_amd.pipeline import TrainPipeline
    net = TiltNet(64)
    trainer = _trainer_class()(net, bad)
    return TrainPipeline(_conf(tmp_path, **kw), policy_value_net=net, seed=1, trainer=trainer, eval_net=TiltNet(64),
                         distributed=False, resume=resume), trainer


def test_pipeline_takes_and_matches_the_two_keys(tmp_path):
    for kw, guard, clip in (({}, False, None), ({"step_guard": True}, True, None), ({"clip_norm": 3}, True, 3.0),
                            ({"step_guard": False, "clip_norm": 0.5}, True, 0.5)):
        pipe, _ = _pipeline(tmp_path, **kw)
        assert pipe.step_guard is guard and pipe.clip_norm == clip
        assert pipe._conf_match["step_guard"] is guard and pipe._conf_match["clip_norm"] == clip
        pipe.engine.close()
    for bad in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_norm"):
            _pipeline(tmp_path, clip_norm=bad)


def test_pipeline_resumes_a_checkpoint_from_before_the_keys(tmp_path):
    conf = dict(checkpoint_every=2)
    first, _ = _pipeline(tmp_path, **conf)
    first.run()
    first.engine.close()
    path = os.path.join(first.model_dir, "checkpoints", "ckpt_%08d" % 2)
    sj = os.path.join(path, "state.json")
    state = json.load(open(sj))
    assert state["conf"]["step_guard"] is False and state["conf"]["clip_norm"] is None
    del state["conf"]["step_guard"], state["conf"]["clip_norm"]                    # as a run from before the keys wrote it
    json.dump(state, open(sj, "w"))
    second, _ = _pipeline(tmp_path, resume=path, **conf)                           # off matches "no such key"
    assert second._batches_done == 2 and second.lr_multiplier == first.lr_multiplier
    second.engine.close()
    for kw, key in (({"step_guard": True}, "step_guard"), ({"clip_norm": 1.0}, "step_guard")):
        with pytest.raises(ValueError, match=key):
            _pipeline(tmp_path, resume=path, **dict(conf, **kw))
    # ... and one written WITH the keys asks for the same ones
    third, _ = _pipeline(tmp_path / "c", step_guard=True, clip_norm=2.0, **conf)
    third.run()
    third.engine.close()
    path3 = os.path.join(third.model_dir, "checkpoints", "ckpt_%08d" % 2)
    with pytest.raises(ValueError, match="clip_norm"):
        _pipeline(tmp_path / "c", resume=path3, step_guard=True, clip_norm=4.0, **conf)
    again, _ = _pipeline(tmp_path / "c", resume=path3, clip_norm=2.0, **conf)
    again.engine.close()


def _mini(rs, n=16):
    return [((rs.rand(4, 8, 8) > 0.5).astype(np.float32), rs.dirichlet(np.ones(64)).astype(np.float32), float(rs.choice([-1, 1])))
            for _ in range(n)]


def test_policy_update_keeps_the_multiplier_when_every_step_was_skipped():
    from _pipeline_worker import TiltNet, TiltTrainer
    from alphapig_amd.train import policy_update
    mini = _mini(np.random.RandomState(3))
    # every step skipped: nothing changed, KL = 0 < kl_targ / 2 would raise the multiplier -- it stays
    net = TiltNet(64)
    tr = _trainer_class()(net, bad=("all",))
    mon = {}
    loss, ent, kl, mult = policy_update(tr, mini, 2e-3, 1.0, epochs=3, kl_targ=0.02, evaluator=net, monitors=mon)
    assert mult == 1.0 and kl == 0.0 and np.isnan(loss)
    assert mon["skipped_steps"] == 3 and mon["clipped_steps"] == 0 and np.isnan(mon["grad_norm"])
    assert tr.t == 0 and tr.asked == 3
    # none skipped: the multiplier moves exactly as with a trainer that has no counters
    results = []
    for make in (lambda n: _trainer_class()(n), TiltTrainer):
        net = TiltNet(64)
        tr = make(net)
        mon = {}
        results.append(policy_update(tr, mini, 2e-3, 1.0, epochs=3, kl_targ=0.02, evaluator=net, monitors=mon) + (mon,))
    assert results[0][:4] == results[1][:4] and results[0][3] != 1.0
    assert results[0][4]["skipped_steps"] == 0 and results[0][4]["grad_norm"] == 0.25
    assert "skipped_steps" not in results[1][4] and "grad_norm" not in results[1][4]           # the test doubles: as before
    # a trainer that has the counters and says its guard is off (HipTrainer's default): as before as well
    net = TiltNet(64)
    tr = _trainer_class()(net)
    tr.step_guard = False
    mon = {}
    assert policy_update(tr, mini, 2e-3, 1.0, epochs=3, kl_targ=0.02, evaluator=net, monitors=mon) == results[1][:4]
    assert mon == results[1][4]
    # one of three skipped: the update changed the net, the KL decides as always
    net = TiltNet(64)
    tr = _trainer_class()(net, bad=(1,))
    mon = {}
    out = policy_update(tr, mini, 2e-3, 1.0, epochs=3, kl_targ=0.02, evaluator=net, monitors=mon)
    assert mon["skipped_steps"] == 1 and tr.t == 2 and out[3] != 1.0


def test_pipeline_records_and_warns_about_skipped_steps(tmp_path, caplog):
    import logging
    pipe, trainer = _pipeline(tmp_path, bad=("all",), step_guard=True, game_batch_num=3)
    with caplog.at_level(logging.WARNING, logger="alphapig_amd.pipeline"):
        hist = pipe.run()
    pipe.engine.close()
    upd = [r for r in hist if "loss" in r]
    assert upd and all(r["skipped_steps"] > 0 and r["clipped_steps"] == 0 for r in upd)
    assert all(r["grad_norm"] is None for r in upd)            # the NaN norm of a skipped step: None, which strict JSON can carry
    json.loads(json.dumps([{k: v for k, v in r.items() if k == "grad_norm"} for r in hist], allow_nan=False))
    assert upd[-1]["skipped_steps"] == trainer.skipped_steps == trainer.asked
    assert pipe.lr_multiplier == 1.0
    assert any("skipped" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    # with the keys off the record is what it was
    pipe, _ = _pipeline(tmp_path / "off", game_batch_num=3)
    hist = pipe.run()
    pipe.engine.close()
    assert all("skipped_steps" not in r and "grad_norm" not in r for r in hist)
