"""CPU-side checks of the framed training step's interface (HipTrainer(framed=True): the boards of 6x6 .. 14x14 other than
8x8 and 10x10 on the 15x15 trunk kernels, csrc/bn_frame.h): what the switch admits and refuses, before anything looks for a
GPU; the new entry points in the header, the library and the binding; TrainPipeline's refusals at construction."""
import os
import re

import pytest

from alphapig_amd import _native, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SYMBOLS = ["apz_bn_fwd_frame", "apz_bn_bwd_frame", "apz_frame_planes_dev", "apz_conv1x1_fwd_frame",
                 "apz_conv1x1_bwd2_frame"]


def _prm(side, kind="resnet", nf=128):
    return weights.init_params(kind, side, side, 9, 1 if kind == "resnet" else 0, nf, seed=1, style="bench")


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.is_available() -> False: a refusal that comes after the GPU check shows as a RuntimeError, on every machine"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.mark.parametrize("side", [6, 7, 9, 11, 12, 13, 14])
def test_framed_switch_admits_the_framed_sides(side, no_gpu):
    from alphapig_amd.train import HipTrainer, check_trainable_board
    prm = _prm(side)
    check_trainable_board(prm, framed=True)
    with pytest.raises(RuntimeError, match="needs a GPU"):           # past every shape check: the next thing is the GPU
        HipTrainer(prm, "resnet", 1, batch_size=8, framed=True)


def _refused(prm, match, kind="resnet", **kw):
    from alphapig_amd.train import HipTrainer, check_trainable_board
    with pytest.raises(ValueError, match=match):
        check_trainable_board(prm, framed=True, net_kind=kind, **kw)
    with pytest.raises(ValueError, match=match):                     # (a RuntimeError here would be the GPU check coming first)
        HipTrainer(prm, kind, 1 if kind == "resnet" else 0, batch_size=8, framed=True, **kw)


def test_framed_switch_refuses_10x10(no_gpu):
    _refused(_prm(10), "10x10")


def test_framed_switch_refuses_the_simple_net_and_64_filters(no_gpu):
    _refused(_prm(9, "simple"), "residual net", kind="simple")
    _refused(_prm(9, nf=64), "128 filters")
    _refused(_prm(9, nf=256), "128 filters")


def test_framed_switch_refuses_the_f16x2_trunk(no_gpu):
    _refused(_prm(9), "f16x2", trunk_arith="f16x2")


@pytest.mark.parametrize("side", [9, 13])
def test_default_call_is_unchanged(side, no_gpu):
    from alphapig_amd.train import HipTrainer, check_trainable_board
    prm = _prm(side)
    for call in (lambda: check_trainable_board(prm), lambda: check_trainable_board(prm, framed=False),
                 lambda: HipTrainer(prm, "resnet", 1, batch_size=8), lambda: HipTrainer(prm, "resnet", 1, batch_size=8, framed=False)):
        with pytest.raises(ValueError, match="15x15 and 8x8") as ei:
            call()
        assert "%dx%d" % (side, side) in str(ei.value)


@pytest.mark.parametrize("side", [8, 15])
@pytest.mark.parametrize("framed", [False, True])
def test_15x15_and_8x8_pass_whatever_the_switch_says(side, framed, no_gpu):
    from alphapig_amd.train import HipTrainer, check_trainable_board
    check_trainable_board(_prm(side), framed=framed)
    check_trainable_board(_prm(8, "simple"), framed=framed, net_kind="simple")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        HipTrainer(_prm(side), "resnet", 1, batch_size=8, framed=framed)


def test_new_entry_points_in_header_library_and_binding():
    L = _native.hip()
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    for s in FRAME_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*apz_engine\s*\*" % s, hdr), s
        assert s in _native.HIP_SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.apz_bn_fwd_frame.argtypes) == len(L.apz_bn_fwd_stats.argtypes)          # - stats + side
    assert len(L.apz_bn_bwd_frame.argtypes) == len(L.apz_bn_bwd_max.argtypes) + 1        # + side
    assert "csrc/bn_frame.h" in hdr


def _conf(tmp_path, side, **kw):
    c = {"board_width": side, "board_height": side, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 1000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 1, "play_batch_size": 1, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": str(tmp_path / "models")}
    c.update(kw)
    return c


def _pipeline(tmp_path, side, **kw):
    from _pipeline_worker import TiltNet, TiltTrainer
    from alphapig_amd.pipeline import TrainPipeline
    net = TiltNet(side * side)
    return TrainPipeline(_conf(tmp_path, side, **kw), policy_value_net=net, seed=1, trainer=TiltTrainer(net), distributed=False)


@pytest.mark.parametrize("bad,match", [({"replay": "compact"}, "replay='tuples'"), ({"replay": "device"}, "replay='tuples'"),
                                       ({"train_arith": "f16x2"}, "train_arith='f32'")])
def test_pipeline_refuses_at_construction(tmp_path, bad, match, no_gpu):
    with pytest.raises(ValueError, match=match):
        _pipeline(tmp_path, 9, train_framed=True, **bad)


def test_pipeline_key_defaults_off_and_reaches_the_checkpoint_keys(tmp_path):
    for kw, want in (({}, False), ({"train_framed": True}, True)):
        pipe = _pipeline(tmp_path, 9, **kw)
        assert pipe.train_framed is want and pipe._conf_match["train_framed"] is want
        pipe.engine.close()
    # 15x15 and 8x8: the key changes nothing, so the combinations stay open
    pipe = _pipeline(tmp_path, 8, train_framed=True, replay="compact", train_arith="f16x2")
    assert pipe.train_framed and pipe.replay == "compact"
    pipe.engine.close()


def test_net_carries_the_switch_to_its_trainer():
    import inspect
    from alphapig_amd.policy_value_net import PolicyValueNet
    assert inspect.signature(PolicyValueNet.__init__).parameters["train_framed"].default is False
