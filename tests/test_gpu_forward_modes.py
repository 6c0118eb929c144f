"""The mode of a forward leaves nothing behind (csrc/apz_engine.hip, FwdMode / trunk_route): whichever entry point ran last --
a warm-up, the layer bench, a layer read-back, a refused call, a failed or a successful calibration, the exact repeat of an
overflowed forward, a slot submission in flight, profiling on or off, a graph replay -- the next synchronous forward of an
engine returns the bits of a fresh twin's FIRST forward, and the engine counts exactly the overflows that were provoked.

Engines: the 15x15 / 128-filter net (2 blocks) in every arithmetic, the 8x8 simple net and a framed 9x9 net, batch_size 64.
Batches: 5 and 40 boards, the two sides of the 32 / 33 boundary between the small-batch and the batched trunk kernels (8x8 boards
have one kernel family: 5 only).  Every step below runs with a batch in flight on slot 1; `graphs` turns apz_set_forward_graphs
on for the 5-board batches, where the third submission captures and later ones replay.  Everything is compared bit for bit
(assert_array_equal): nothing here is a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphapig_amd import weights
from alphapig_amd._native import as_ptr
from alphapig_amd.policy_value_net import KERNEL_CLASSES, EvaluatorError, PolicyValueNet

from test_gpu_net import random_positions

pytestmark = pytest.mark.gpu

# name -> (board side, net kind, residual blocks, trunk_arith, uniform_trunk)
ENGINES = {
    "f32": (15, "resnet", 2, "f32", False),
    "f16x2": (15, "resnet", 2, "f16x2", False),
    "f16x2-uniform": (15, "resnet", 2, "f16x2", True),
    "bf16x3": (15, "resnet", 2, "bf16x3", False),
    "simple8": (8, "simple", 0, "f16x2", False),
    "framed9": (9, "resnet", 1, "f16x2", False),
}
CASES = [(name, n, False) for name in ENGINES for n in (5, 40) if not (name == "simple8" and n == 40)]
CASES += [(name, 5, True) for name in ENGINES]
SLOT = 1


@functools.lru_cache(maxsize=None)
def _params(side, kind, blocks):
    return weights.init_params(kind, side, side, 9, blocks, 128, seed=41, style="bench")


@functools.lru_cache(maxsize=None)
def _big():
    """tests/test_gpu_act_scale.py's `big`: stem outputs in the tens of thousands, the f16x2 trunk kernels overflow"""
    prm = dict(_params(15, "resnet", 2))
    prm["res_conv1_weight"] = np.asarray(prm["res_conv1_weight"], np.float32) * 3.0e4
    return prm


@functools.lru_cache(maxsize=None)
def _broken():
    """... and its net whose first block is not finite in exact fp32 either: a calibration on it fails (match="finite")"""
    prm = dict(_big())
    prm["bnA1_gamma"] = np.full_like(np.asarray(prm["bnA1_gamma"], np.float32), 3e38)
    return prm


@functools.lru_cache(maxsize=None)
def _positions(side):
    codes, planes = random_positions(65, side, seed=77)
    codes.setflags(write=False)
    planes.setflags(write=False)
    return codes, planes


def _make(name):
    side, kind, blocks, arith, uniform = ENGINES[name]
    return PolicyValueNet(side, side, batch_size=64, n_blocks=blocks, n_filter=128, model_params=_params(side, kind, blocks),
                          net_kind=kind, trunk_arith=arith, uniform_trunk=uniform)


def _layers(net):
    """(first and last conv layer, whether the engine has rows16 activations)"""
    last = 2 * net._n_blocks if net.net_kind == "resnet" else 5
    ring = net.net_kind == "resnet" and net._n_filter == 128 and net.board_width != 8
    return (0, last), ring


def _read_backs(net, n):
    (first, last), ring = _layers(net)
    out = [net.layer_output(first, n), net.layer_output(last, n)]
    if ring:
        out += [net.layer_frame(first, n), net.layer_frame(last, n)]
    return out


def _counts(net):
    return {k: net.kernel_time_ms(k)[1] for k in KERNEL_CLASSES}


@pytest.mark.parametrize("name,n,graphs", CASES)
def test_every_entry_point_leaves_the_next_forward_alone(name, n, graphs):
    side = ENGINES[name][0]
    codes_all, planes_all = _positions(side)
    codes, planes = codes_all[:n], planes_all[:n]
    f16_15 = name in ("f16x2", "f16x2-uniform")
    twin, net = _make(name), _make(name)
    try:
        ref = twin.forward_with_logits(planes)                      # the reference: a fresh engine's first forward
        twin.forward_planes(planes)
        ref_layers = _read_backs(twin, n)
        net._ck(net.L.apz_set_forward_graphs(net._h, int(graphs)))
        overflows = 0

        def check(what):
            got = net.forward_with_logits(planes)
            for a, b, part in zip(got, ref, ("logits", "probs", "value logits", "values")):
                np.testing.assert_array_equal(a, b, err_msg="%s after %s" % (part, what))
            assert net.trunk_overflows() == overflows, what

        def step(what, fn):
            """fn() with a batch in flight on SLOT, then that batch's results, then a synchronous forward"""
            k = net.submit_codes_slot(SLOT, codes)
            fn()
            p, v = net.wait_slot(SLOT, k)
            np.testing.assert_array_equal(p, ref[1], err_msg="slot probs across " + what)
            np.testing.assert_array_equal(v, ref[3], err_msg="slot values across " + what)
            check(what)

        def prewarm():
            net.prewarm(n, 2)

        def bench():
            assert net.conv_bench(1, n, iters=1, warmup=0) >= 0.0

        def read_backs():
            for got, want in zip(_read_backs(net, n), ref_layers):
                np.testing.assert_array_equal(got, want)

        def refused():
            with pytest.raises(EvaluatorError, match="max_batch"):
                net.forward_with_logits(planes_all)                 # 65 boards
            with pytest.raises(EvaluatorError):
                net.prewarm(65, 1)
            with pytest.raises(EvaluatorError, match="bad layer"):
                net.conv_bench(99, n, iters=1, warmup=0)
            with pytest.raises(EvaluatorError, match="bad layer"):
                net._ck(net.L.apz_layer_io(net._h, 99, as_ptr(np.zeros(1, np.float32), C.c_float), 1))

        check("nothing")
        net.forward_planes(planes)                                  # the bench and the read-backs run on the resident planes
        step("prewarm", prewarm)
        step("conv_bench", bench)
        step("layer read-backs", read_backs)
        step("refused calls", refused)

        # the same with profiling on: the bench and the read-backs time nothing, a forward is still counted
        def profiled():
            net.set_profiling(1)
            bench()
            read_backs()
            refused()
            net.sync()
            assert not any(_counts(net).values()), _counts(net)     # (the slot's batch went out before profiling came on)
            prewarm()
            net.sync()
            assert _counts(net)["forward"] == 2
        step("profiled bench, read-backs and prewarm", profiled)
        timed = _counts(net)
        net.set_profiling(0)
        (_, last), _ = _layers(net)
        assert timed["forward"] == 3                                 # ... + the synchronous forward of the check
        assert timed["trunk"] == 3 * last                            # nothing from the bench or a read-back

        if f16_15:
            exps = net.trunk_act_exponents()

            def failed_calibration():
                net.set_params(_broken())
                net.set_trunk_act_exponents([1, -2, 3, -4])
                with pytest.raises(EvaluatorError, match="finite"):
                    net.calibrate_trunk(planes)
                assert net.trunk_act_exponents() == [1, -2, 3, -4]
                net.set_trunk_act_exponents(exps)
                net.set_params(_params(15, "resnet", 2))
            step("a calibration that fails", failed_calibration)

            def calibration():
                net.calibrate_trunk(planes_all[:5])
                net.set_trunk_act_exponents([0] * 4)
            step("a calibration that succeeds", calibration)

            def overflow():
                # (without uniform_trunk a batch of <= 32 boards runs exact fp32 and cannot overflow: 40 boards there)
                boards = planes if (ENGINES[name][4] or n > 32) else planes_all[:40]
                net.set_params(_big())
                net.forward_with_logits(boards)
                net.set_params(_params(15, "resnet", 2))
            overflows += 1
            step("an overflowing forward", overflow)

        # a last round without anything in between: with graphs on, submissions 3 and 4 of the shape are the capture and a replay
        for i in range(4):
            step("submission %d" % (i + 1), lambda: None)
    finally:
        twin.close()
        net.close()
