"""CPU-side checks of the legal-move policy's interface (apz_set_legal_policy): the four entry points
in the header, the library and the binding; the keyword on HipTrainer and PolicyValueNet, as far as the GPU check; the net
handing the switch to its trainer; TrainPipeline's conf key on its way to every net and trainer it builds, into the
checkpoint's conf keys and through a resume."""
import inspect
import os
import re

import numpy as np
import pytest

from _pipeline_worker import TiltNet, TiltTrainer
from alphapig_amd import _native, checkpoint, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGAL_SYMBOLS = ["apz_set_legal_policy", "apz_get_legal_policy", "apz_occupancy_planes", "apz_pv_loss_legal"]


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.is_available() -> False: a refusal that comes after the GPU check shows as a RuntimeError, on every machine"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_header_library_and_binding_agree_on_the_four_symbols():
    L = _native.hip()
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    for s in LEGAL_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*apz_engine\s*\*" % s, hdr), s
        assert s in _native.HIP_SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    # apz_pv_loss's arguments plus the occupancy; apz_pv_loss itself as it was
    assert len(L.apz_pv_loss_legal.argtypes) == len(L.apz_pv_loss.argtypes) + 1 == 13
    assert len(L.apz_occupancy_planes.argtypes) == 8 and len(L.apz_set_legal_policy.argtypes) == 2
    for text in ("csrc/heads.h", "csrc/conv8_small.h", "csrc/heads_train.h"):
        assert text in hdr
    # no engine without a GPU: the calls refuse a null engine instead of touching it
    assert L.apz_set_legal_policy(None, 1) < 0 and L.apz_get_legal_policy(None) < 0
    assert L.apz_occupancy_planes(None, None, 1, 9, 15, 15, None, None) < 0
    assert L.apz_pv_loss_legal(*([None] * 6 + [1] + [None] * 6)) < 0


@pytest.mark.parametrize("side,kind", [(15, "resnet"), (9, "resnet"), (8, "simple")])
@pytest.mark.parametrize("on", [False, True])
def test_trainer_takes_the_keyword_as_far_as_the_gpu_check(side, kind, on, no_gpu):
    from alphapig_amd.train import HipTrainer
    blocks = 1 if kind == "resnet" else 0
    prm = weights.init_params(kind, side, side, 9, blocks, 128, seed=1, style="bench")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        HipTrainer(prm, kind, blocks, batch_size=8, framed=side == 9, legal_policy=on)
    assert inspect.signature(HipTrainer.__init__).parameters["legal_policy"].default is False


def test_net_takes_the_keyword_and_carries_the_switch_to_its_trainer(monkeypatch):
    from alphapig_amd import policy_value_net as pvn
    from alphapig_amd import train
    sig = inspect.signature(pvn.PolicyValueNet.__init__).parameters
    assert sig["legal_policy"].default is False
    assert callable(pvn.PolicyValueNet.set_legal_policy) and callable(pvn.LanedEvaluator.set_legal_policy)
    L = _native.hip()
    if L.apz_device_count() == 0:                     # as far as the engine: "no CPU fallback"
        with pytest.raises(pvn.EvaluatorError, match="no CPU fallback"):
            pvn.PolicyValueNet(15, 15, batch_size=4, n_blocks=1, legal_policy=True)
    # train_step hands the net's switch to the trainer it builds, beside train_framed
    seen = {}

    class Recorder(object):
        def __init__(self, params, *a, **kw):
            seen.update(kw)

        def train_step(self, *a):
            return 0.0, 0.0

        def sync_evaluator(self, net):
            pass

    monkeypatch.setattr(train, "HipTrainer", Recorder)
    for on in (False, True):
        net = object.__new__(pvn.PolicyValueNet)        # no engine: only what train_step reads
        net.__dict__.update(_h=None, _trainer=None, net_kind="resnet", _n_blocks=1, batchsize=8, _device=0, train_framed=False,
                            train_step_guard=False, train_clip_norm=None, ema_decay=None, ema_warmup=True, legal_policy=on,
                            params=lambda: {})
        net.train_step(None, None, None, 1e-3)
        assert seen["legal_policy"] is on and seen["framed"] is False


# ---- TrainPipeline
class FakeNet(TiltNet):
    """tests/fakenet.py's closed-form net behind PolicyValueNet's constructor: records what TrainPipeline passes"""
    built = []

    def __init__(self, width, height, batch_size=512, **kw):
        TiltNet.__init__(self, width * height)
        self.kw, self.legal_policy = kw, bool(kw.get("legal_policy", False))
        self.net_kind, self._n_blocks, self._n_filter, self._device, self._trainer = "resnet", 1, 128, 0, None
        FakeNet.built.append(self)

    def set_legal_policy(self, on):
        self.legal_policy = bool(on)


def _conf(tmp_path, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 301, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 2, "play_batch_size": 1, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


class StatefulTrainer(TiltTrainer):
    def state(self):
        return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

    def load_state(self, state):
        self._p = {"w": np.array(state["p/w"], np.float32), "b": np.array(state["p/b"], np.float32)}
        self.t = int(state["meta"]["t"])


@pytest.mark.parametrize("kw,want", [({}, False), ({"legal_policy": False}, False), ({"legal_policy": True}, True)])
def test_pipeline_passes_the_key_to_every_net_and_trainer_it_builds(tmp_path, monkeypatch, kw, want):
    from alphapig_amd import pipeline, train
    FakeNet.built = []
    monkeypatch.setattr(pipeline, "PolicyValueNet", FakeNet)
    pipe = pipeline.TrainPipeline(_conf(tmp_path, **kw), seed=3, distributed=False)
    try:
        assert pipe.legal_policy is want and pipe._conf_match["legal_policy"] is want
        assert len(FakeNet.built) == 1 and FakeNet.built[0].kw["legal_policy"] is want and pipe.policy_value_net.legal_policy is want
        # the trainer the pipeline builds for that net
        seen = {}
        monkeypatch.setattr(train, "HipTrainer", lambda params, *a, **k: seen.update(k) or TiltTrainer(pipe.policy_value_net))
        pipe._trainer()
        assert seen["legal_policy"] is want and seen["framed"] is False
    finally:
        pipe.engine.close()


def test_pipeline_switches_the_evaluators_it_is_handed_and_refuses_those_that_cannot(tmp_path):
    from alphapig_amd.pipeline import TrainPipeline
    net, ev = FakeNet(8, 8), FakeNet(8, 8)
    pipe = TrainPipeline(_conf(tmp_path, legal_policy=True), policy_value_net=net, eval_net=ev, seed=3, trainer=TiltTrainer(net),
                         distributed=False)
    assert net.legal_policy and ev.legal_policy
    pipe.engine.close()
    net, ev = FakeNet(8, 8), FakeNet(8, 8)
    pipe = TrainPipeline(_conf(tmp_path), policy_value_net=net, eval_net=ev, seed=3, trainer=TiltTrainer(net), distributed=False)
    assert not net.legal_policy and not ev.legal_policy          # key absent: nothing is called
    pipe.engine.close()
    plain = TiltNet(64)                                          # no set_legal_policy
    with pytest.raises(ValueError, match="set_legal_policy"):
        TrainPipeline(_conf(tmp_path, legal_policy=True), policy_value_net=plain, seed=3, trainer=TiltTrainer(plain), distributed=False)
    net = FakeNet(8, 8)
    off = TiltTrainer(net)
    off.legal_policy = False
    with pytest.raises(ValueError, match="legal_policy=False"):
        TrainPipeline(_conf(tmp_path, legal_policy=True), policy_value_net=net, seed=3, trainer=off, distributed=False)


def test_checkpoint_carries_the_key_and_a_resume_with_the_other_value_is_refused(tmp_path):
    from alphapig_amd.pipeline import TrainPipeline

    def pipe(conf, resume=None):
        net = FakeNet(8, 8)
        return TrainPipeline(conf, policy_value_net=net, seed=5, trainer=StatefulTrainer(net), eval_net=FakeNet(8, 8),
                             distributed=False, resume=resume)
    paths = {}
    for on in (False, True):
        conf = _conf(tmp_path / str(on), legal_policy=on, checkpoint_every=2)
        p = pipe(conf)
        p.run()
        p.engine.close()
        paths[on] = os.path.join(conf["model_dir"], "checkpoints", "ckpt_%08d" % 2)
        assert checkpoint.read_state(paths[on])["conf"]["legal_policy"] is on
    for on in (False, True):
        conf = _conf(tmp_path / str(on), legal_policy=on, checkpoint_every=2)
        again = pipe(conf, resume=paths[on])                     # the same value: goes on
        assert again._batches_done == 2
        again.engine.close()
        with pytest.raises(ValueError, match="legal_policy=%r, this pipeline has legal_policy=%r" % (not on, on)):
            pipe(conf, resume=paths[not on])
    # a checkpoint from before the key counts as off
    import json
    state_file = os.path.join(paths[False], "state.json")
    state = json.load(open(state_file))
    del state["conf"]["legal_policy"]
    json.dump(state, open(state_file, "w"))
    conf = _conf(tmp_path / "False", checkpoint_every=2)
    old = pipe(conf, resume=paths[False])
    assert old._batches_done == 2
    old.engine.close()
    with pytest.raises(ValueError, match="legal_policy=False, this pipeline has legal_policy=True"):
        pipe(dict(conf, legal_policy=True), resume=paths[False])
