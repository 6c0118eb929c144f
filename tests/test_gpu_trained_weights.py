"""The inference kernels against float64 on weights the project's own training step produced (tests/trained_nets.py: HipTrainer
steps from the Xavier start on the committed self-play episodes, inside the test; nothing synthetic).  Every other inference
test runs on weights.init_params statistics drawn from fixed ranges; a trained net has stem variances of 1e-2, trunk variances
from 0.05 to tens and a residual stream of 20 to 30, and the Winograd transforms, the f16x2 hi / lo split with its per-channel
weight scale, the per-layer activation exponent and the BatchNorm fold of csrc/weights_pack.h see those operands here for the
first time.

Unlike the logit-only tests of the deep nets, every convolution layer is compared (apz_layer_io), per layer and per output
channel, so that a fault in one channel of a middle layer is not diluted by what follows it.

Bars (tests/trained_nets.py, all from rules the suite already uses; tests/test_trained_bounds.py shows that plain float32
arithmetic sits at about a hundredth of them):
  probabilities, values      2e-5
  logits, value logit        (1e-4 / 3) * max(1, max |float64|)              (tests/test_gpu_winograd_numerics.py)
  a layer                    (1e-4 / 3) * max(1, max |float64 layer|)
  an output channel c        (1e-4 / 3) * max(1, A_c), A_c = max over boards and cells of conv(|x|, |folded w|) + |shift|
  a dead channel             float64 pre-activation below minus its bar everywhere -> exactly 0
  the split kernels          additionally, per layer: error <= max(2 x the direct kernel's, 1.25 x the fp32 Winograd kernel's,
                             1e-6 x the layer scale), the three measured in the same run on the same inputs
The measured table, r12_trained_weights.json, goes to the directory APZ_TABLE_DIR names (the run committed as
profiles/r12_trained_weights.json set it); without the variable it goes to a pytest temporary directory and the tree stays clean."""
import json
import os
import time

import numpy as np
import pytest

import trained_nets as tn
from test_gpu_net import _net_with_trunk_kernel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_BOUND_F16X2 = 655.0                      # |V| = |B^T d B| <= 100 |x| must stay inside the fp16 range (trunk15_wino3h16.h)
SPLIT_ROUTES = ("wino3b", "wino3h", "wino3hs")
RECORD = {"tolerance": tn.TOL, "head_atol": tn.HEAD_ATOL, "f16x2_activation_bound": ACT_BOUND_F16X2,
          "training": {"batch": tn.BATCH, "lr": tn.LR, "dropout": tn.DROPOUT}, "fixtures": {}, "rows": [], "test_seconds": {}}


_OUT = {}


@pytest.fixture(scope="module", autouse=True)
def _table_dir(tmp_path_factory):
    _OUT["dir"] = os.environ.get("APZ_TABLE_DIR") or str(tmp_path_factory.mktemp("trained_weights"))


def _save():
    out = os.path.join(REPO, _OUT["dir"])          # (an absolute APZ_TABLE_DIR stays as it is)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "r12_trained_weights.json"), "w") as f:
        json.dump(RECORD, f, indent=1)


class _Timer(object):
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.time()

    def __exit__(self, *exc):
        RECORD["test_seconds"][self.name] = round(time.time() - self.t0, 3)
        _save()


def _fixture(name, kind, side, n_blocks, steps, detail=None):
    t = tn.trained(kind, side, n_blocks, steps)
    planes = tn.eval_positions(side)
    t0 = time.time()
    ref = tn.Reference(t.params, planes, kind, n_blocks, detail)
    RECORD["fixtures"][name] = {
        "net": "%s %dx%d, %d blocks" % (kind, side, side, n_blocks), "steps": steps, "train_seconds": round(t.seconds, 3),
        "float64_reference_seconds": round(time.time() - t0, 3), "sha256": t.sha256, "loss_first": t.losses[0],
        "loss_last20_mean": float(np.mean(t.losses[-20:])), "loss_history": [round(x, 4) for x in t.losses],
        "stem_var": [float(np.min(t.params["res_conv1_var" if kind == "resnet" else "conv1_var"])),
                     float(np.max(t.params["res_conv1_var" if kind == "resnet" else "conv1_var"]))],
        "trunk_var": {k: [float(np.min(t.params[k])), float(np.max(t.params[k]))] for k in tn.trunk_var_names(kind, n_blocks)},
        "float64_activation_max": [float(np.abs(a).max()) for a in ref.layers],
        "logit_scale": ref.logit_scale, "value_logit_scale": ref.vlogit_scale}
    return t, planes, ref


@pytest.fixture(scope="module")
def net3():
    return _fixture("resnet15_3", "resnet", 15, 3, 300)


@pytest.fixture(scope="module")
def net10():
    return _fixture("resnet15_10", "resnet", 15, 10, 500, detail=(0, 1, 10, 20))


@pytest.fixture(scope="module")
def simple8():
    return _fixture("simple8", "simple", 8, 0, 300)


def _net15(prm, n_blocks, batch=64, **kw):
    from alphapig_amd.policy_value_net import PolicyValueNet
    return PolicyValueNet(15, 15, batch_size=batch, n_blocks=n_blocks, n_filter=128, model_params=prm, **kw)


def _measure(net, ref, planes, rows, layers, row):
    """One forward of `planes` (= boards `rows` of the reference): heads and the given layers against float64.  A forward the
    f16x2 kernel had to repeat on the exact kernel is counted in row["overflow_repeats"]; its heads are the exact kernel's and
    are held to the bars all the same, but apz_layer_io would show the overflowed layers, so the exponents are then taken from
    these boards (calibrate_trunk) and the forward is run once more without a repeat.  -> failures."""
    n = len(planes)
    before = net.trunk_overflows()
    heads = net.forward_with_logits(planes)
    rec, bad = ref.check_heads(heads, rows)
    row["overflow_repeats"] = net.trunk_overflows() - before
    if row["overflow_repeats"]:
        row["act_max_at_calibration"] = [float(v) for v in net.calibrate_trunk(planes=planes)]
        before = net.trunk_overflows()
        heads = net.forward_with_logits(planes)
        rec2, bad2 = ref.check_heads(heads, rows)
        bad += bad2
        rec = {k: max(v, rec2[k]) for k, v in rec.items()}
        assert net.trunk_overflows() == before, "a calibrated forward of the calibration boards repeated"
    row["exponents"] = net.trunk_act_exponents() if net.trunk_arith == "f16x2" and net.board_width == 15 else None
    row.update(rec)
    p2, v2 = net.forward_planes(planes)
    np.testing.assert_array_equal(p2, heads[1])
    np.testing.assert_array_equal(v2, heads[3])
    row["layers"] = []
    for l in layers:
        r, b = ref.check_layer(l, net.layer_output(l, n), rows)
        row["layers"].append(r)
        bad += b
    return ["%s n=%d: %s" % (row.get("route"), n, b) for b in bad]


def _gate(rows_by_route, split, direct, wino):
    """The comparator gate on every layer of route `split`; the ratio error / allowance goes into the record."""
    bad = []
    for s, d, w in zip(rows_by_route[split]["layers"], rows_by_route[direct]["layers"], rows_by_route[wino]["layers"]):
        allow = max(2.0 * d["err"], 1.25 * w["err"], 1e-6 * s["scale"])
        s["gate_err_over_allowance"] = s["err"] / allow
        if not tn.comparator_gate(s["err"], d["err"], w["err"], s["scale"]):
            bad.append("%s layer %d: error %.3g, direct %.3g, fp32 Winograd %.3g (comparator gate)" %
                       (split, s["layer"], s["err"], d["err"], w["err"]))
    return bad


@pytest.mark.parametrize("install", ["host", "device"])
@pytest.mark.parametrize("n", [7, 33])
def test_every_layer_on_every_trunk_route(net3, n, install):
    """3 blocks, 300 steps.  trunk15_ring_kernel (direct), trunk15_wino3s_kernel, trunk15_wino3_kernel, trunk15_wino3b_kernel,
    trunk15_wino3h16_kernel forced onto the batch, and for n <= 32 trunk15_wino3hs_kernel (uniform_trunk): layers 0 .. 6, logits,
    value logit, probabilities and values against float64, and the split kernels against the comparator gate.  The weights
    arrive as apz_load_weights brings them (fold and pack on the host) or as trainer.sync_evaluator does (the kernels of
    csrc/weights_pack.h)."""
    t, positions, ref = net3
    rows = slice(0, 7) if n == 7 else slice(7, 40)
    planes = positions[rows]
    start = tn._start("resnet", 15, 3)
    routes = ["ring", "wino3", "wino3-batched", "wino3b", "wino3h"] + (["wino3hs"] if n <= 32 else [])
    with _Timer("every_layer[%d-%s]" % (n, install)):
        by_route, bad = {}, []
        for route in routes:
            first = t.params if install == "host" else start
            net = _net15(first, 3, uniform_trunk=True) if route == "wino3hs" else _net_with_trunk_kernel(route, first, 3, 64)
            try:
                if install == "device":
                    t.trainer.sync_evaluator(net)
                row = {"test": "every_layer", "fixture": "resnet15_3", "route": route, "n": n, "install": install}
                bad += _measure(net, ref, planes, rows, range(7), row)
                by_route[route] = row
                RECORD["rows"].append(row)
            finally:
                net.close()
        for route in routes:
            if route in SPLIT_ROUTES:
                bad += _gate(by_route, route, "ring", "wino3-batched")
        # the two fp32 Winograd forms are the same arithmetic in the same order
        for a, b in zip(by_route["wino3"]["layers"], by_route["wino3-batched"]["layers"]):
            assert a["err"] == b["err"]
    assert not bad, bad


@pytest.mark.parametrize("arith", ["auto", "f32"])
def test_ten_blocks_at_24_and_40_boards(net10, arith):
    """10 blocks, 500 steps, as PolicyValueNet comes by default (f16x2 above 32 boards, the exact kernel below) and with
    trunk_arith="f32": heads and layers 0, 1, 10 and 20.  Uncalibrated repeats are counted, not forbidden (a repeat is exact,
    so the bars hold whatever the count); after calibrate_trunk on one half of the positions the other half runs on the f16x2
    kernel (forced onto its 20 boards) without a single repeat, inside the bars."""
    t, positions, ref = net10
    layers = (0, 1, 10, 20)
    with _Timer("ten_blocks[%s]" % arith):
        net = _net15(t.params, 10, trunk_arith=arith)
        bad = []
        try:
            assert net.trunk_arith == ("f16x2" if arith == "auto" else "f32")
            for n in (24, 40):
                # n == 40 on an engine of its own: the 24-board forward must not have left exponents behind
                cur = _net15(t.params, 10, trunk_arith=arith) if arith == "auto" and n == 40 else net
                try:
                    row = {"test": "ten_blocks", "fixture": "resnet15_10", "route": arith, "n": n, "install": "host"}
                    bad += _measure(cur, ref, positions[:n], slice(0, n), layers, row)
                    RECORD["rows"].append(row)
                finally:
                    if cur is not net:
                        cur.close()
            if arith == "auto":
                idx = np.arange(40)
                half_a, half_b = idx[idx % 4 < 2], idx[idx % 4 >= 2]
                maxima = net.calibrate_trunk(planes=positions[half_a])
                assert maxima.shape == (20,) and np.isfinite(maxima).all() and maxima.max() < ACT_BOUND_F16X2
                net._ck(net.L.apz_test_select_trunk(net._h, 4))          # the f16x2 kernel for every batch size
                before = net.trunk_overflows()
                row = {"test": "ten_blocks_calibrated_other_half", "fixture": "resnet15_10", "route": "wino3h", "n": len(half_b),
                       "install": "host", "calibration_act_max": [float(v) for v in maxima]}
                bad += _measure(net, ref, positions[half_b], half_b, layers, row)
                RECORD["rows"].append(row)
                assert row["overflow_repeats"] == 0 and net.trunk_overflows() == before
                assert any(row["exponents"]), "calibration left every exponent at 0: nothing of the scaled form ran"
        finally:
            net.close()
    assert not bad, bad


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
def test_a_boards_bits_do_not_depend_on_the_batch(net3, arith):
    """The same board alone, at row 5 of 7 and at row 35 of 40: the same bits in every head output and in every layer -- f16x2
    with uniform_trunk (trunk15_wino3hs_kernel at 1 and 7 boards, trunk15_wino3h16_kernel at 40) and the f32 route
    (trunk15_wino3s_kernel / trunk15_wino3_kernel)."""
    t, positions, _ = net3
    board = positions[12]
    seven, forty = positions[:7].copy(), positions.copy()
    seven[5], forty[35] = board, board
    with _Timer("batch_independence[%s]" % arith):
        net = _net15(t.params, 3, trunk_arith=arith, uniform_trunk=(arith == "f16x2"))
        try:
            net.forward_with_logits(forty)
            if net.trunk_overflows():                # bits are uniform among forwards that do not repeat
                net.calibrate_trunk(planes=forty)
            before = net.trunk_overflows()
            got = []
            for planes, r in ((board[None], 0), (seven, 5), (forty, 35)):
                heads = [np.array(a[r], copy=True) for a in net.forward_with_logits(planes)]
                net.forward_planes(planes)
                got.append(heads + [net.layer_output(l, len(planes))[r] for l in range(7)])
            assert net.trunk_overflows() == before
            for other in got[1:]:
                for a, b in zip(got[0], other):
                    np.testing.assert_array_equal(a, b)
        finally:
            net.close()


@pytest.mark.parametrize("side,arith", [(15, "f32"), (15, "f16x2"), (15, "bf16x3"), (8, "f32"), (8, "f16x2")])
def test_device_install_gives_the_host_installs_bits(net3, simple8, side, arith):
    """trainer.sync_evaluator(net): BatchNorm fold and weight pack as kernels (csrc/weights_pack.h).  set_params(trainer.
    get_params()): the same maps on the host.  On trained statistics (variances of 1e-2 to tens) both evaluators give the
    same bits, at 7 boards and at all of them."""
    from alphapig_amd.policy_value_net import PolicyValueNet
    t, positions, _ = net3 if side == 15 else simple8
    kind, blocks = ("resnet", 3) if side == 15 else ("simple", 0)
    with _Timer("install[%d-%s]" % (side, arith)):
        kw = dict(batch_size=64, n_blocks=blocks, n_filter=128, net_kind=kind, trunk_arith=arith)
        dev = PolicyValueNet(side, side, model_params=tn._start(kind, side, blocks), **kw)
        host = PolicyValueNet(side, side, model_params=tn._start(kind, side, blocks), **kw)
        try:
            t.trainer.sync_evaluator(dev)
            host.set_params(t.trainer.get_params())
            assert tn.params_sha256(t.trainer.get_params()) == t.sha256
            for planes in (positions[:7], positions):
                a, b = dev.forward_with_logits(planes), host.forward_with_logits(planes)
                for x, y in zip(a, b):
                    np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
                dev.forward_planes(planes)
                host.forward_planes(planes)
                for l in range(2 * blocks + 1 if kind == "resnet" else 6):
                    np.testing.assert_array_equal(dev.layer_output(l, len(planes)), host.layer_output(l, len(planes)))
            assert dev.trunk_overflows() == host.trunk_overflows()
        finally:
            dev.close()
            host.close()


@pytest.mark.parametrize("n", [3, 33])
def test_simple_net_8x8_every_layer(simple8, n):
    """The 8x8 plain net, 300 steps: conv8_kernel (csrc/conv8_small.h, "f32") and conv8h_kernel (csrc/conv8_split.h, "f16x2") on
    all six layers and head8_kernel's four outputs against float64.  The 8x8 path has one exact kernel, which is both the
    direct and the fp32 comparator of the split kernel's gate: error <= max(2 x conv8_kernel's, 1e-6 x the layer scale)."""
    from alphapig_amd.policy_value_net import PolicyValueNet
    t, positions, ref = simple8
    rows = slice(0, 3) if n == 3 else slice(3, 36)
    with _Timer("simple8[%d]" % n):
        by_route, bad = {}, []
        for arith in ("f32", "f16x2"):
            net = PolicyValueNet(8, 8, batch_size=64, model_params=t.params, net_kind="simple", trunk_arith=arith)
            try:
                row = {"test": "simple8", "fixture": "simple8", "route": "conv8" if arith == "f32" else "conv8h", "n": n,
                       "install": "host"}
                bad += _measure(net, ref, positions[rows], rows, range(6), row)
                by_route[arith] = row
                RECORD["rows"].append(row)
            finally:
                net.close()
        bad += _gate(by_route, "f16x2", "f32", "f32")
    assert not bad, bad
