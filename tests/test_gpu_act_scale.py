"""Static per-layer activation exponents of the f16x2 trunk kernel (csrc/trunk15_wino3h16.h, WINO3H16_PLAIN_SCALED;
include/alphapig_hip.h, apz_set_trunk_act_exponents): the input of trunk convolution l is multiplied by 2^a_l in front of
the two-term fp16 split and 2^-a_l is folded into the bias FMA, so a layer whose activations lie above ~655 (overflow:
the forward is repeated on the exact kernel, every time) or below 2^-3 (subnormal lo term: ~9 bits) is evaluated at full
accuracy without a repeat.  The exponents come from a calibration forward (csrc/act_max.h measures the maxima), from the
caller, or -- opt-in -- from the exact repeat of an overflowed forward.  The reference computes these convolutions in
fp32 with no such range (policy_value_net_mxnet.py:77-83); the oracle is its float64 restatement.

Shapes: 6-board batches forced onto the batched kernel (apz_test_select_trunk), and n in {33, 40, 100} on the default
routing (an odd count, more than one item per workgroup, plain and residual instantiations).  Tolerances: LOGIT_ATOL (1e-4)
on logits and 2e-5 on probabilities / values where the logit scale is <= 1, else the stress test's rule
(1e-4 / 3) * max(1, max |oracle logit|) (tests/test_gpu_winograd_numerics.py).

The error table (r10_act_scale_numerics.json, written where tests/test_gpu_winograd_numerics.py writes its tables and
committed under profiles/) and the timings: profiles/r10_act_scale.md."""
import os

import numpy as np
import pytest

from alphapig_amd import weights
from alphapig_amd.policy_value_net import EvaluatorError, PolicyValueNet, act_exponent_for
from oracle import net_ref

from test_gpu_net import LOGIT_ATOL, _net_with_trunk_kernel, random_positions
from test_gpu_winograd_numerics import TOL, _boards, _variant
from test_gpu_winograd_numerics import _write_table as _write_stress_table

pytestmark = pytest.mark.gpu

_ROWS = []                       # what the tests measured, in the stress tables' row format ("wino3h" = the calibrated engine)


def _write_table():
    _write_stress_table("r10_act_scale_numerics.json", ("wino3h",), _ROWS)


def _net(prm, n_blocks=2, batch=128, arith="f16x2", k8=False, **kw):
    old = os.environ.pop("APZ_F16X2_K8", None)
    if k8:
        os.environ["APZ_F16X2_K8"] = "1"
    try:
        return PolicyValueNet(15, 15, batch_size=batch, n_blocks=n_blocks, n_filter=128, model_params=prm, trunk_arith=arith, **kw)
    finally:
        os.environ.pop("APZ_F16X2_K8", None)
        if old is not None:
            os.environ["APZ_F16X2_K8"] = old


def _rel_bound(o_logits):
    return TOL * max(1.0, float(np.abs(o_logits).max()))


@pytest.fixture(scope="module")
def base():
    return weights.init_params("resnet", 15, 15, 9, 2, 128, seed=41, style="bench")


@pytest.fixture(scope="module")
def big(base):
    """the existing overflow tests' net: stem outputs in the tens of thousands"""
    prm = dict(base)
    prm["res_conv1_weight"] = np.asarray(base["res_conv1_weight"], np.float32) * 3.0e4
    return prm


@pytest.fixture(scope="module")
def outlier(base):
    """one hot BatchNorm gamma: channel 3 of the first block's inner activation is ~1.6e3"""
    prm = dict(base)
    g = np.array(base["bnA1_gamma"], np.float32)
    g[3] = 5e3
    prm["bnA1_gamma"] = g
    return prm


@pytest.fixture(scope="module")
def pos100():
    return random_positions(100, 15, seed=77)          # (codes, planes)


@pytest.fixture(scope="module")
def outlier_oracle(outlier, pos100):
    rows = [0, 1, 32, 39, 50, 98, 99]
    return rows, net_ref.forward(outlier, pos100[1][rows], "resnet", 2, np.float64)


def test_exponents_of_zero_are_todays_engine(base, big, pos100):
    planes = pos100[1][:40]
    fresh, zeroed = _net(base), _net(base)
    exact, split = _net(big, arith="f32"), _net(big)
    try:
        assert fresh.trunk_act_exponents() == [0, 0, 0, 0]
        zeroed.set_trunk_act_exponents([0] * 4)
        a, b = fresh.forward_with_logits(planes), zeroed.forward_with_logits(planes)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert fresh.trunk_overflows() == 0 and zeroed.trunk_overflows() == 0
        # auto off (the default): an overflow still repeats, nothing learns from it
        for _ in range(2):
            before = split.trunk_overflows()
            x, y = exact.forward_with_logits(planes), split.forward_with_logits(planes)
            assert split.trunk_overflows() == before + 1
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u, v)
        assert split.trunk_overflows() == 2 and split.trunk_act_exponents() == [0, 0, 0, 0]
    finally:
        for n in (fresh, zeroed, exact, split):
            n.close()


def test_outlier_channel_runs_without_a_repeat_once_calibrated(outlier):
    """One hot BatchNorm gamma (bnA1_gamma[3] = 5e3): the inner activation of block 1 reaches ~2e3.  Whether the UNSCALED
    kernel overflows on that is a property of the boards: the proven bound |V| <= 100 max |x| is not reached by every
    position.  A float64 restatement of V = B^T d B gives max |V| = 59 544 (below fp16's 65 520) for the sparse leaves of
    random_positions(40, 15, seed=8) -- and on an MI355X such a batch (seed 77) indeed ran without a repeat -- but 72 342 for
    the 40 boards of _boards("random", n=40, seed=5) (10 to 120 stones each), which are therefore the boards of this test."""
    planes = _boards("random", n=40, seed=5)
    rows = [0, 1, 17, 38, 39]
    o = net_ref.forward(outlier, planes[rows], "resnet", 2, np.float64)
    net = _net(outlier)
    try:
        net.forward_with_logits(planes)
        assert net.trunk_overflows() == 1                          # uncalibrated: every such forward repeats
        m = net.calibrate_trunk(planes)
        exps = net.trunk_act_exponents()
        print("outlier net: layer maxima", m.tolist(), "exponents", exps)
        assert net.trunk_overflows() == 1                          # a calibration is no overflow
        assert exps[1] < 0
        logits, _, vlog, _ = net.forward_with_logits(planes)
        assert net.trunk_overflows() == 1                          # ... and the same forward no longer repeats
        bound = _rel_bound(o[0])
        err_l = float(np.abs(logits[rows] - o[0]).max())
        err_v = float(np.abs(vlog[rows] - o[2][:, 0]).max())
        print("outlier net: logit err %.3g value-logit err %.3g bound %.3g" % (err_l, err_v, bound))
        assert err_l <= bound and err_v <= bound
    finally:
        net.close()


def test_lower_end_small_activations_keep_full_accuracy(base, pos100):
    planes = pos100[1][:40]
    prm = dict(base)
    for k in ("res_conv1_weight", "res_conv1_bias", "res_conv1_mean", "res_conv1_beta"):
        prm[k] = (np.asarray(base[k], np.float32) * np.float32(2.0 ** -20)).astype(np.float32)
    prm["convA1_weight"] = (np.asarray(base["convA1_weight"], np.float32) * np.float32(2.0 ** 20)).astype(np.float32)
    rows = [0, 1, 17, 38, 39]
    o = net_ref.forward(prm, planes[rows], "resnet", 2, np.float64)
    exact, plain, cal = _net(prm, arith="f32"), _net(prm), _net(prm)
    try:
        # the condition on the input: the exact-fp32 engine itself is within LOGIT_ATOL of the oracle
        e = exact.forward_with_logits(planes)
        np.testing.assert_allclose(e[0][rows], o[0], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(e[2][rows], o[2][:, 0], rtol=0, atol=LOGIT_ATOL)
        cal.calibrate_trunk(planes)
        exps = cal.trunk_act_exponents()
        assert exps[0] >= 20
        c, u = cal.forward_with_logits(planes), plain.forward_with_logits(planes)
        assert cal.trunk_overflows() == 0 and plain.trunk_overflows() == 0
        errs = {"exponents": exps,
                "calibrated_logit_err": float(np.abs(c[0][rows] - o[0]).max()),
                "calibrated_value_err": float(np.abs(c[3][rows] - o[3][:, 0]).max()),
                "uncalibrated_logit_err": float(np.abs(u[0][rows] - o[0]).max()),
                "uncalibrated_value_err": float(np.abs(u[3][rows] - o[3][:, 0]).max()),
                "exact_f32_logit_err": float(np.abs(e[0][rows] - o[0]).max())}
        print("lower end:", errs)
        # (logit scale <= 1 here: the absolute errors are the relative ones)
        _ROWS[:] = [r for r in _ROWS if r["weights"] != "lower_end_2_blocks"]
        _ROWS.append(dict(errs, weights="lower_end_2_blocks", boards="sparse", logit_scale=1.0, value_logit_scale=1.0,
                          wino3h_logit_err_rel=errs["calibrated_logit_err"], wino3h_value_err_rel=errs["calibrated_value_err"]))
        _write_table()
        np.testing.assert_allclose(c[0][rows], o[0], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(c[2][rows], o[2][:, 0], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(c[1][rows], o[1], rtol=0, atol=2e-5)
        np.testing.assert_allclose(c[3][rows], o[3][:, 0], rtol=0, atol=2e-5)
        assert errs["uncalibrated_logit_err"] > errs["calibrated_logit_err"]
    finally:
        for n in (exact, plain, cal):
            n.close()


def test_layer_maxima_are_exact_and_exponents_follow_the_rule(outlier, big, pos100):
    planes = pos100[1][:40]
    exact, net = _net(outlier, arith="f32"), _net(outlier)
    try:
        exact.forward_planes(planes)
        want = np.array([np.abs(exact.layer_output(l, 40)).max() for l in range(4)], np.float32)
        got = net.calibrate_trunk(planes)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)                   # a maximum is exact in any order
        assert net.trunk_act_exponents() == [act_exponent_for(m) for m in want]
        # ... the same through the codes entry point (the stem decodes the codes itself: the same planes, the same bits)
        net.set_trunk_act_exponents([0] * 4)
        np.testing.assert_array_equal(net.calibrate_trunk(codes=pos100[0][:40]), want)
        assert net.trunk_act_exponents() == [act_exponent_for(m) for m in want]
        # a batch of at most 32 boards (the exact path's small-batch kernel) calibrates too
        exact.forward_planes(planes[:7])
        want7 = np.array([np.abs(exact.layer_output(l, 7)).max() for l in range(4)], np.float32)
        np.testing.assert_array_equal(net.calibrate_trunk(planes[:7]), want7)
        with pytest.raises(EvaluatorError):
            net.set_trunk_act_exponents([0, 0, 0])                  # count must be 2 * n_blocks
        with pytest.raises(EvaluatorError):
            net.set_trunk_act_exponents([0, 101, 0, 0])
    finally:
        exact.close()
        net.close()
    # a layer that overflows in exact fp32: the call fails and the previous exponents stay
    broken = dict(big)
    broken["bnA1_gamma"] = np.full_like(np.asarray(big["bnA1_gamma"], np.float32), 3e38)
    net = _net(broken)
    try:
        net.set_trunk_act_exponents([1, -2, 3, -4])
        with pytest.raises(EvaluatorError, match="finite"):
            net.calibrate_trunk(planes)
        assert net.trunk_act_exponents() == [1, -2, 3, -4]
        assert net.trunk_overflows() == 0
    finally:
        net.close()


def test_stress_rows_run_without_a_repeat_once_calibrated():
    """The rows of tests/test_gpu_winograd_numerics.py whose activations explode or vanish through the 10-block net, 6 boards
    forced onto the batched f16x2 kernel, calibrated on the same boards: no repeat in any row, every error within
    (1e-4 / 3) * max(1, scale), rows with logit scale > 1e3 within max(that, 4 x the direct kernel's own error)."""
    rows = []
    planes = _boards("random")
    for vname in ("base", "w4_raw", "w025_raw", "var_1e-3"):
        prm = _variant(vname)
        o_logits, _, o_vlog, _ = net_ref.forward(prm, planes, "resnet", 10, np.float64)
        scale = max(1.0, float(np.abs(o_logits).max()))
        vscale = max(1.0, float(np.abs(o_vlog).max()))
        row = {"weights": vname, "boards": "random", "logit_scale": scale, "value_logit_scale": vscale}
        ring = _net_with_trunk_kernel("ring", prm, 10, 16)
        try:
            logits, _, vlog, _ = ring.forward_with_logits(planes)
        finally:
            ring.close()
        row["ring_logit_err_rel"] = float(np.abs(logits - o_logits).max()) / scale
        row["ring_value_err_rel"] = float(np.abs(vlog - o_vlog[:, 0]).max()) / vscale
        net = _net_with_trunk_kernel("wino3h", prm, 10, 16)
        try:
            net.forward_with_logits(planes)
            row["uncalibrated_repeats"] = net.trunk_overflows()
            row["layer_max"] = [float(m) for m in net.calibrate_trunk(planes)]
            row["exponents"] = net.trunk_act_exponents()
            logits, _, vlog, _ = net.forward_with_logits(planes)
            row["calibrated_repeats"] = net.trunk_overflows() - row["uncalibrated_repeats"]
        finally:
            net.close()
        assert np.isfinite(logits).all() and np.isfinite(vlog).all(), vname
        row["wino3h_logit_err_rel"] = float(np.abs(logits - o_logits).max()) / scale
        row["wino3h_value_err_rel"] = float(np.abs(vlog - o_vlog[:, 0]).max()) / vscale
        print("%-9s scale %9.3g  repeats %d -> %d  exponents %d .. %d  scaled %.2e / %.2e  ring %.2e / %.2e" % (
            vname, scale, row["uncalibrated_repeats"], row["calibrated_repeats"], max(row["exponents"]), min(row["exponents"]),
            row["wino3h_logit_err_rel"], row["wino3h_value_err_rel"], row["ring_logit_err_rel"], row["ring_value_err_rel"]))
        rows.append(row)
    _ROWS[:] = [r for r in _ROWS if r["weights"] == "lower_end_2_blocks"] + rows
    _write_table()

    def bound(r, key):
        return max(TOL, 4.0 * r["ring_" + key]) if r["logit_scale"] > 1e3 else TOL
    assert all(r["calibrated_repeats"] == 0 for r in rows), rows
    bad = [r for r in rows if r["wino3h_logit_err_rel"] > bound(r, "logit_err_rel") or
           r["wino3h_value_err_rel"] > bound(r, "value_err_rel")]
    assert not bad, bad


@pytest.mark.parametrize("n", [33, 100])
def test_bits_do_not_depend_on_place_or_launch_shape_with_exponents(outlier, pos100, outlier_oracle, n):
    planes = pos100[1][:n]
    rows, o = outlier_oracle
    keep = [i for i, r in enumerate(rows) if r < n]
    net = _net(outlier)
    try:
        net.calibrate_trunk(planes)
        exps = net.trunk_act_exponents()
        assert any(a != 0 for a in exps)
        logits, probs, vlog, vals = net.forward_with_logits(planes)
        bound = _rel_bound(o[0][keep])
        sel = [rows[i] for i in keep]
        assert float(np.abs(logits[sel] - o[0][keep]).max()) <= bound
        assert float(np.abs(vlog[sel] - o[2][keep, 0]).max()) <= bound
        perm = np.random.RandomState(1).permutation(n)
        p2 = net.forward_with_logits(planes[perm])
        np.testing.assert_array_equal(p2[0], logits[perm])
        np.testing.assert_array_equal(p2[2], vlog[perm])
        sub = net.forward_with_logits(planes[n - 33:])             # the last 33 boards: same kernel, other launch shape
        np.testing.assert_array_equal(sub[0], logits[n - 33:])
        np.testing.assert_array_equal(sub[2], vlog[n - 33:])
        assert net.trunk_overflows() == 0 and net.trunk_act_exponents() == exps
    finally:
        net.close()


def test_auto_response_lowers_the_exponents_from_the_exact_repeat(big, pos100):
    codes, planes = pos100[0][:40], pos100[1][:40]
    rows = [0, 1, 20, 39]
    o = net_ref.forward(big, planes[rows], "resnet", 2, np.float64)
    bound = _rel_bound(o[0])
    exact, net = _net(big, arith="f32"), _net(big)
    others = []
    try:
        net.set_act_scale_auto(True)
        a, b = exact.forward_with_logits(planes), net.forward_with_logits(planes)     # apz_forward
        assert net.trunk_overflows() == 1
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)                    # the repeat's results: the exact kernel's bits
        exps = net.trunk_act_exponents()
        assert all(e < 0 for e in exps), exps
        c = net.forward_with_logits(planes)
        assert net.trunk_overflows() == 1 and net.trunk_act_exponents() == exps        # no repeat, nothing more to learn
        assert float(np.abs(c[0][rows] - o[0]).max()) <= bound
        assert float(np.abs(c[2][rows] - o[2][:, 0]).max()) <= bound
        # prewarm / the layer bench / the layer hook arm the word without collecting it: they never adjust exponents
        lazy = _net(big)
        others.append(lazy)
        lazy.forward_planes(planes)                                 # (auto still off: a plain repeat; the planes stay resident)
        lazy.set_act_scale_auto(True)
        lazy.conv_bench(1, 40, iters=1, warmup=0)
        lazy.layer_output(2, 40)
        lazy.prewarm(40, 1)
        lazy.sync()
        assert lazy.trunk_act_exponents() == [0, 0, 0, 0] and lazy.trunk_overflows() == 1
        # the other collecting entry points, a fresh engine each; the exponents they learn and the bits they then give are
        # those of the engine above (same batch, same kernels)
        ex_planes, ex_codes = exact.forward_planes(planes), exact.evaluate_codes(codes)
        calls = [("apz_wait", lambda n_: n_.evaluate_codes_slot(1, codes), ex_codes),
                 ("apz_forward_host", lambda n_: n_.forward_planes(planes), ex_planes),
                 ("apz_forward_codes_host", lambda n_: n_.evaluate_codes(codes), ex_codes)]
        for name, call, want in calls:
            eng = _net(big)
            others.append(eng)
            eng.set_act_scale_auto(True)
            first = call(eng)
            assert eng.trunk_overflows() == 1, name
            np.testing.assert_array_equal(first[0], want[0], err_msg=name)
            np.testing.assert_array_equal(first[1], want[1], err_msg=name)
            assert eng.trunk_act_exponents() == exps, name
            second = call(eng)
            assert eng.trunk_overflows() == 1, name
            np.testing.assert_array_equal(second[0], c[1], err_msg=name)
            np.testing.assert_array_equal(second[1], c[3], err_msg=name)
    finally:
        for n in [exact, net] + others:
            n.close()


def test_engines_without_a_scaled_form_refuse_and_go_on_working(base, pos100):
    planes = pos100[1][:40]
    o = net_ref.forward(base, planes[:3], "resnet", 2, np.float64)
    for kw, what in ((dict(arith="f32"), "APZ_ARITH_F16X2"), (dict(k8=True), "APZ_F16X2_K8")):
        net = _net(base, **kw)
        try:
            for call in (lambda: net.set_trunk_act_exponents([1, 1, 1, 1]), lambda: net.calibrate_trunk(planes),
                         lambda: net.calibrate_trunk(codes=pos100[0][:40]), lambda: net.set_act_scale_auto(True),
                         lambda: net.trunk_act_exponents()):
                with pytest.raises(EvaluatorError, match=what) as ei:
                    call()
                assert "code -4" in str(ei.value)                   # APZ_E_UNSUPPORTED
            logits = net.forward_with_logits(planes)[0]
            np.testing.assert_allclose(logits[:3], o[0], rtol=0, atol=LOGIT_ATOL)
            assert net.trunk_overflows() == 0
        finally:
            net.close()
    prm8 = weights.init_params("resnet", 8, 8, 9, 2, 128, seed=2, style="bench")
    net8 = PolicyValueNet(8, 8, batch_size=32, n_blocks=2, n_filter=128, model_params=prm8)
    try:
        assert net8.trunk_arith == "f16x2"
        codes8, planes8 = random_positions(19, 8, seed=9)
        for call in (lambda: net8.set_trunk_act_exponents([1, 1, 1, 1]), lambda: net8.calibrate_trunk(planes8),
                     lambda: net8.calibrate_trunk(codes=codes8), lambda: net8.set_act_scale_auto(True)):
            with pytest.raises(EvaluatorError, match="8x8") as ei:
                call()
            assert "code -4" in str(ei.value)
        logits = net8.forward_with_logits(planes8)[0]
        np.testing.assert_allclose(logits, net_ref.forward(prm8, planes8, "resnet", 2)[0], rtol=0, atol=LOGIT_ATOL)
    finally:
        net8.close()
