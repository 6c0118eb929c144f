"""The static activation exponents of the f16x2 trunk kernel, host side (no GPU): the exponent rule at its edges,
LanedEvaluator's delegation, and what TrainPipeline's act_scale key does to the evaluators and the round records.
Stand-in evaluator and trainer: tests/_pipeline_worker.py."""
import numpy as np
import pytest

from _pipeline_worker import TiltNet, TiltTrainer
from alphapig_amd.pipeline import TrainPipeline
from alphapig_amd.policy_value_net import ACT_EXP_MAX, ACT_WINDOW_LOG2, LanedEvaluator, act_exponent_for


def test_exponent_rule_at_its_edges():
    assert (ACT_WINDOW_LOG2, ACT_EXP_MAX) == (4, 100)
    # m 2^a in [2^4, 2^5): an exact power of two is the LOWER edge of its binade, the float below it belongs to the one before
    for e in (-20, -3, 0, 1, 4, 5, 9, 10):
        m = np.float32(2.0) ** e
        assert act_exponent_for(m) == 4 - e
        assert act_exponent_for(np.nextafter(m, np.float32(0))) == 4 - (e - 1)
        assert act_exponent_for(np.nextafter(m, np.float32(np.inf))) == 4 - e
        for v in (m, np.nextafter(m, np.float32(0)), np.nextafter(np.float32(2) * m, np.float32(0))):
            assert 16.0 <= float(v) * 2.0 ** act_exponent_for(v) < 32.0
    # the issue's outlier net: maxima 1.0 / 1.6e3 / 285 / 259 -> 4 / -6 / -4 / -4
    assert [act_exponent_for(m) for m in (1.0, 1.6e3, 285.0, 259.0)] == [4, -6, -4, -4]
    assert act_exponent_for(0.0) == 0
    # a subnormal float (2^-149 .. 2^-127) would want a > 100: clamped; so is a huge maximum
    assert act_exponent_for(np.float32(1e-45)) == 100 and act_exponent_for(np.float32(2.0) ** -127) == 100
    assert act_exponent_for(np.float32(2.0) ** -96) == 100 and act_exponent_for(np.float32(2.0) ** -95) == 99
    assert act_exponent_for(np.float32(3e38)) == -100
    assert act_exponent_for(np.float32(2.0) ** 104) == -100 and act_exponent_for(np.float32(2.0) ** 103) == -99
    # the weight-scale clamp: 2^-(a + k) must stay a normal float, -126 <= a + k <= 126 for every channel's k
    assert act_exponent_for(2.0 ** -90, k_min=18, k_max=18) == 94
    assert act_exponent_for(2.0 ** -90, k_min=18, k_max=40) == 86
    assert act_exponent_for(2.0 ** 90, k_min=-60, k_max=18) == -66
    assert act_exponent_for(0.0, k_min=-100, k_max=100) == 0
    for bad in (np.inf, -np.inf, np.nan, -1.0):
        with pytest.raises(ValueError):
            act_exponent_for(bad)


class _Lane(object):
    n_slots, batchsize, hw, code_stride = 3, 32, 64, 80

    def __init__(self, exps):
        self.exps, self.auto, self.calibrated = list(exps), None, []

    def calibrate_trunk(self, planes=None, codes=None):
        self.calibrated.append(("planes" if planes is not None else "codes", len(planes if planes is not None else codes)))
        self.exps = [4, -6]
        return np.array([1.0, 1600.0], np.float32)

    def trunk_act_exponents(self):
        return list(self.exps)

    def set_trunk_act_exponents(self, seq):
        self.exps = [int(a) for a in seq]

    def set_act_scale_auto(self, on):
        self.auto = bool(on)

    def trunk_overflows(self):
        return 2


def test_laned_evaluator_calibrates_lane_0_and_fans_the_exponents_out():
    a, b, c = _Lane([0, 0]), _Lane([0, 0]), _Lane([1, 1])
    ev = LanedEvaluator([a, b, c])
    m = ev.calibrate_trunk(codes=np.zeros((5, 80), np.uint8))
    np.testing.assert_array_equal(m, np.array([1.0, 1600.0], np.float32))
    assert a.calibrated == [("codes", 5)] and b.calibrated == [] and c.calibrated == []      # one measuring forward
    assert a.exps == b.exps == c.exps == [4, -6] and ev.trunk_act_exponents() == [4, -6]
    ev.calibrate_trunk(planes=np.zeros((3, 9, 8, 8), np.float32))
    assert a.calibrated[-1] == ("planes", 3)
    ev.set_trunk_act_exponents((2, -1))
    assert a.exps == b.exps == c.exps == [2, -1]
    ev.set_act_scale_auto(True)
    assert (a.auto, b.auto, c.auto) == (True, True, True)
    ev.set_act_scale_auto(False)
    assert (a.auto, b.auto, c.auto) == (False, False, False)
    assert ev.trunk_overflows() == 6


class _ScaledTiltNet(TiltNet):
    """TiltNet with the activation-scale interface of PolicyValueNet: counts what the pipeline asks of it."""

    def __init__(self, hw):
        TiltNet.__init__(self, hw)
        self.auto, self.calibrations, self.exps, self.batchsize, self.sets_at_calibration = None, [], [0, 0], 4, []

    def trunk_overflows(self):
        return 7

    def set_act_scale_auto(self, on):
        self.auto = bool(on)

    def trunk_act_exponents(self):
        return list(self.exps)

    def calibrate_trunk(self, planes=None, codes=None):
        assert planes is None and codes.dtype == np.uint8 and codes.ndim == 2
        self.calibrations.append(len(codes))
        self.sets_at_calibration.append(self.sets)
        self.exps = [3, -len(self.calibrations)]
        return np.ones(2, np.float32)


def _conf(tmp_path, **kw):
    c = {"board_width": 15, "board_height": 15, "n_in_row": 5, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 6, "c_puct": 5, "buffer_size": 100000, "batch_size": 16, "epochs": 1, "kl_targ": 1e9,
         "check_freq": 1000, "eval_games": 2, "game_batch_num": 4, "play_batch_size": 1, "pure_mcts_playout_num": 10,
         "async_update": True, "round_steps": 8, "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


@pytest.mark.parametrize("value", ["on", "AUTO", "", None, True])
def test_unknown_act_scale_is_rejected(value):
    with pytest.raises(ValueError, match="act_scale"):
        TrainPipeline({"act_scale": value}, policy_value_net=object(), trainer=object())


@pytest.mark.parametrize("async_update", [True, False])
def test_round_records_carry_the_evaluators_overflow_count_with_act_scale_off(tmp_path, async_update):
    net, kl = _ScaledTiltNet(225), _ScaledTiltNet(225)
    pipe = TrainPipeline(_conf(tmp_path, async_update=async_update), policy_value_net=net, seed=3, trainer=TiltTrainer(net),
                         eval_net=kl, distributed=False)
    assert pipe.act_scale == "off"
    hist = pipe.run()
    assert hist and all(r["eval_trunk_overflows"] == 7 for r in hist)
    assert not any("act_exponents" in r for r in hist)
    assert net.auto is None and kl.auto is None and net.calibrations == []          # "off" touches nothing
    pipe.engine.close()


def test_an_evaluator_without_an_overflow_count_is_left_out_of_the_record(tmp_path):
    net = TiltNet(225)
    pipe = TrainPipeline(_conf(tmp_path, game_batch_num=2), policy_value_net=net, seed=3, trainer=TiltTrainer(net),
                         eval_net=TiltNet(225), distributed=False)
    hist = pipe.run()
    assert hist and not any("eval_trunk_overflows" in r or "act_exponents" in r for r in hist)
    pipe.engine.close()


@pytest.mark.parametrize("async_update", [True, False])
def test_act_scale_auto_arms_the_evaluators_and_calibrates_after_every_installation(tmp_path, async_update):
    net, kl = _ScaledTiltNet(225), _ScaledTiltNet(225)
    pipe = TrainPipeline(_conf(tmp_path, act_scale="auto", async_update=async_update), policy_value_net=net, seed=3,
                         trainer=TiltTrainer(net), eval_net=kl, distributed=False)
    assert net.auto is True and kl.auto is True and net.calibrations == []         # nothing played yet: no calibration
    hist = pipe.run()
    installs = pipe.weight_broadcasts if async_update else sum(1 for r in hist if "loss" in r)
    assert installs >= 1 and len(net.calibrations) == installs and kl.calibrations == []
    # on the engine's most recent code batch, cut to the evaluator's batch size, and with the NEW weights in place
    assert all(1 <= n <= net.batchsize for n in net.calibrations)
    if async_update:
        assert net.sets_at_calibration == list(range(1, installs + 1))
    assert all(r["eval_trunk_overflows"] == 7 for r in hist)
    assert hist[-1]["act_exponents"] == [3, -installs] and all(isinstance(a, int) for a in hist[-1]["act_exponents"])
    assert hist[0]["act_exponents"] in ([0, 0], [3, -1])
    pipe.engine.close()


def test_calibration_is_skipped_while_no_code_batch_exists(tmp_path):
    net = _ScaledTiltNet(225)
    pipe = TrainPipeline(_conf(tmp_path, act_scale="auto"), policy_value_net=net, seed=3, trainer=TiltTrainer(net),
                         eval_net=_ScaledTiltNet(225), distributed=False)
    assert pipe.engine.last_codes is None
    pipe._calibrate_after_install()
    assert net.calibrations == []
    pipe.engine.run_steps(2)
    assert pipe.engine.last_codes is not None and pipe.engine.last_codes.shape[1] == pipe.engine.pool.code_stride
    pipe._calibrate_after_install()
    assert net.calibrations == [min(len(pipe.engine.last_codes), net.batchsize)]
    pipe.engine.close()
