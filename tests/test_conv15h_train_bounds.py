"""The data-gradient bar of tests/test_gpu_generic_train_f16x2.py, tried on the CPU, and the binding of the dense f16x2
training route (HipTrainer(trunk_arith="f16x2") on the 15x15 nets without the padded-row trunk; csrc/conv15_split.h).

The float64 emulation of tests/test_conv15h_bounds.py in the data gradient's orientation: W'[ci][co][ky][kx] =
W[co][ci][2-ky][2-kx], the per-channel scale S over W's INPUT channel, dy times 2^a in front of the split with a from
wino3h16_dgrad_exponent restated (max |dy| 2^a in [2^7, 2^8)), 2^-a undone with S.  What is left is the representation
error.  The GPU bar is twice the larger of the kernel's scale-1 error and the fp32 kernel's error on the same input, relative
to max |dx64|; its second term alone -- float32 accumulation of the unsplit operands, here PyTorch's CPU convolution -- is a
lower bound of it that needs no GPU, and the representation must stay within a quarter of THAT: half the float32 error.
Without the input scale the 1e-6 row misses it: the lo terms are subnormal fp16."""
import os
import re

import numpy as np
import pytest

from alphapig_amd import weights
from test_conv15h_bounds import emulate_split

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGNITUDES = [1.0, 1e-3, 1e-6, 1e-9, 3e4]
SHAPES = [(1, 64, 64), (2, 256, 128)]             # (n, C of dy, C of dx)
NEW_SYMBOLS = ["apz_conv15h_packed_size", "apz_conv15h_pack_many", "apz_conv15h_fwd_packed", "apz_conv15h_dgrad"]


def dgrad_exponent(m):
    """wino3h16_dgrad_exponent (csrc/trunk15_wino3h16.h): a with m 2^a in [2^7, 2^8); 0 for m == 0; clamped to [-64, 110]"""
    if not m > 0:
        return 0
    return int(np.clip(7 - int(np.floor(np.log2(float(m)))), -64, 110))


def dgrad_case(n, c_dy, c_dx, seed=0):
    """dy with max |dy| = 1 (float32), weights [C of dy][C of dx][3][3] = randn / sqrt(9 C of dy)"""
    rs = np.random.RandomState(7000 + 10 * c_dy + c_dx + n + seed)
    dy = rs.randn(n, c_dy, 15, 15)
    dy = (dy / np.abs(dy).max()).astype(np.float32)
    w = (rs.randn(c_dy, c_dx, 3, 3) / np.sqrt(9.0 * c_dy)).astype(np.float32)
    return dy, w


def flipped(w):
    """W [co][ci][ky][kx] -> W' [ci][co][2-ky][2-kx]: the forward weights of the data-gradient convolution"""
    return np.ascontiguousarray(np.asarray(w, np.float64).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def dgrad64(dy, w):
    import torch
    return torch.nn.functional.conv_transpose2d(torch.tensor(np.asarray(dy, np.float64)), torch.tensor(np.asarray(w, np.float64)),
                                                padding=1).numpy()


def emulate_dgrad(dy, w, a):
    """The float64 value of the f16x2 data gradient of float32 dy with the input scale 2^a"""
    scaled = (np.asarray(dy, np.float32) * np.float32(2.0 ** a)).astype(np.float32)          # exact: a power of two
    wf = flipped(w)
    return emulate_split(scaled, wf, np.zeros(len(wf))) / 2.0 ** a


def _errors(dy, w, a):
    import torch
    want = dgrad64(dy, w)
    scale = float(np.abs(want).max())
    rep = float(np.abs(emulate_dgrad(dy, w, a) - want).max()) / scale
    f32 = torch.nn.functional.conv_transpose2d(torch.tensor(dy), torch.tensor(w), padding=1).numpy()
    e32 = float(np.abs(f32.astype(np.float64) - want).max()) / scale
    return rep, e32


def test_flipped_weights_are_the_data_gradient():
    """conv2d with W' is conv_transpose2d with W: the orientation the emulation (and the packer) uses"""
    import torch
    dy, w = dgrad_case(1, 64, 64)
    got = torch.nn.functional.conv2d(torch.tensor(dy.astype(np.float64)), torch.tensor(flipped(w)), padding=1).numpy()
    np.testing.assert_allclose(got, dgrad64(dy, w), rtol=0, atol=1e-13)


def test_exponent_window():
    for m in (1.0, 1e-3, 1e-6, 1e-9, 3e4, 127.9, 128.0, 255.9, 256.0):
        assert 128.0 <= np.float32(m) * 2.0 ** dgrad_exponent(np.float32(m)) < 256.0, m
    assert dgrad_exponent(0.0) == 0 and dgrad_exponent(1e-38) == 110 and dgrad_exponent(3e38) == -64


@pytest.mark.parametrize("magnitude", MAGNITUDES, ids=["1", "1e-3", "1e-6", "1e-9", "3e4"])
@pytest.mark.parametrize("n,c_dy,c_dx", SHAPES, ids=["%dx%dto%d" % s for s in SHAPES])
def test_scaled_representation_meets_a_quarter_of_the_data_gradient_bar(n, c_dy, c_dx, magnitude):
    dy, w = dgrad_case(n, c_dy, c_dx)
    dy = (dy * np.float32(magnitude)).astype(np.float32)
    a = dgrad_exponent(np.abs(dy).max())
    rep, e32 = _errors(dy, w, a)
    print("a = %d: representation %.3e, float32 accumulation %.3e, ratio to a quarter of the bar %.4f" % (a, rep, e32, rep / (0.5 * e32)))
    assert rep <= 0.25 * 2 * e32, (rep, e32)


@pytest.mark.parametrize("n,c_dy,c_dx", SHAPES, ids=["%dx%dto%d" % s for s in SHAPES])
def test_without_the_scale_the_1e_6_row_misses_the_bar(n, c_dy, c_dx):
    dy, w = dgrad_case(n, c_dy, c_dx)
    dy = (dy * np.float32(1e-6)).astype(np.float32)
    rep, e32 = _errors(dy, w, 0)
    print("a = 0: representation %.3e, float32 accumulation %.3e" % (rep, e32))
    assert rep > 0.25 * 2 * e32, (rep, e32)


# ---- binding -----------------------------------------------------------------------------------------------------------
def _prm(side, kind="resnet", nf=64, blocks=1):
    return weights.init_params(kind, side, side, 9, blocks if kind == "resnet" else 0, nf, seed=1, style="bench")


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.is_available() -> False: a refusal that comes after the GPU check shows as a RuntimeError, on every machine"""
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.mark.parametrize("kind,nf,route,layers", [("simple", 128, "dense", ["conv2", "conv3", "conv4", "conv5", "conv_final"]),
                                                  ("resnet", 64, "dense", ["convA1", "convB1"]),
                                                  ("resnet", 256, "dense", ["convA1", "convB1"]),
                                                  ("resnet", 128, "rows16", None)])
def test_f16x2_admits_every_15x15_net(kind, nf, route, layers, no_gpu):
    from alphapig_amd.train import HipTrainer, f16x2_dense_layers, f16x2_route
    prm = _prm(15, kind, nf)
    blocks = 1 if kind == "resnet" else 0
    assert f16x2_route(prm, kind, blocks) == route
    if layers is not None:
        assert f16x2_dense_layers(prm, kind, blocks) == layers         # the first layer (C_in = 9) is never among them
    with pytest.raises(RuntimeError, match="needs a GPU"):             # past every shape check: the next thing is the GPU
        HipTrainer(prm, kind, blocks, batch_size=8, trunk_arith="f16x2")


@pytest.mark.parametrize("kind", ["resnet", "simple"])
def test_f16x2_refuses_8x8_with_the_words_it_had(kind, no_gpu):
    from alphapig_amd.train import HipTrainer
    with pytest.raises(ValueError, match=r"trunk_arith='f16x2' needs the 15x15 residual trunk of 128 filters \(net_kind '%s', 8x8\)" % kind):
        HipTrainer(_prm(8, kind, 128), kind, 1 if kind == "resnet" else 0, batch_size=8, trunk_arith="f16x2")


def test_f16x2_refuses_framed_boards_unknown_values_and_nets_without_a_layer(no_gpu):
    from alphapig_amd.train import HipTrainer
    with pytest.raises(ValueError, match="framed training has no trunk_arith='f16x2' form"):
        HipTrainer(_prm(9, nf=128), "resnet", 1, batch_size=8, framed=True, trunk_arith="f16x2")
    with pytest.raises(ValueError, match="must be 'f32' or 'f16x2'"):
        HipTrainer(_prm(15), "resnet", 1, batch_size=8, trunk_arith="bf16")
    with pytest.raises(ValueError, match="multiples of 64"):
        HipTrainer(_prm(15, nf=32), "resnet", 1, batch_size=8, trunk_arith="f16x2")
    with pytest.raises(RuntimeError, match="needs a GPU"):             # the default is untouched
        HipTrainer(_prm(15, nf=32), "resnet", 1, batch_size=8)


def test_new_entry_points_are_declared_and_bound():
    from alphapig_amd import _native
    header = open(os.path.join(REPO, "include", "alphapig_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % s, header), s
        assert s in _native.HIP_SYMBOLS, s
    assert "apz_conv15h_pack_entry" in header


def test_pipeline_hands_the_switch_to_the_trainer_and_records_overflows(tmp_path, monkeypatch):
    """train_arith="f16x2" with a generic 15x15 net: the pipeline's trainer is built with trunk_arith="f16x2", and the update
    record carries its trunk_overflows"""
    from _pipeline_worker import TiltNet, TiltTrainer
    from alphapig_amd import train
    from alphapig_amd.pipeline import TrainPipeline
    from test_frame_train_binding import _conf
    net = TiltNet(15 * 15)
    pipe = TrainPipeline(_conf(tmp_path, 15, train_arith="f16x2"), policy_value_net=net, seed=1, trainer=TiltTrainer(net),
                         distributed=False)
    seen = {}

    class Recorder(object):
        trunk_overflows = 2

        def __init__(self, params, net_kind, n_blocks, **kw):
            seen.update(kw, net_kind=net_kind, n_blocks=n_blocks)

    class Net(object):
        net_kind, _n_blocks, _device = "resnet", 1, 0

        def params(self):
            return _prm(15, "resnet", 256)

    monkeypatch.setattr(train, "HipTrainer", Recorder)
    trainer = pipe._new_trainer(Net())
    assert seen["trunk_arith"] == "f16x2" and seen["net_kind"] == "resnet" and seen["framed"] is False
    rec = {}
    pipe._note_overflows(rec, trainer)
    assert rec["trunk_overflows"] == 2
    pipe.engine.close()
