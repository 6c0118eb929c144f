"""conv15h_kernel (csrc/conv15_split.h): the two-term fp16 convolution of every 15x15 net that has no Winograd trunk -- the
simple net and the residual nets of 64 and 256 filters -- through the operator entry (hipconv.conv3x3_fwd_f16x2_dense,
apz_conv15h_fwd) and through the evaluator with trunk_arith="f16x2".

Operator: against float64 at the suite's forward bar 2e-5 * max |float64| + 1e-6 (tests/test_gpu_train.py; tests/
test_conv15h_bounds.py shows on the CPU that the split's representation sits at 0.003 of it), on the shapes at which the
kernel takes another path: one, two, three (odd: the double buffer ends on its first half) and four sub-chunks per wave,
and more items than workgroups.  The zero border of the LDS tile is probed with integer-valued cases that have no tolerance.

Evaluator: the nets and positions of tests/generic_nets.py against tests/trained_nets.Reference, bits that do not depend on
the batch, the comparator gate against the fp32 generic kernel, every collecting entry point, both weight loaders, the
overflow repeat, large activations, and an "auto" engine that launches what it launched before."""
import numpy as np
import pytest

import generic_nets as gn
import trained_nets as tn
from test_conv15h_bounds import conv64, op_case, op_tol

pytestmark = pytest.mark.gpu

MAX_BATCH = 80
CASES = [(1, 64, 16), (3, 128, 48), (2, 192, 16), (3, 256, 48)]
VARIANTS = {"plain": (False, False, False), "bias_relu": (True, False, True), "resid": (False, True, False),
            "bias_resid_relu": (True, True, True)}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def conv15h_grid(n, cout, num_cu):
    """launch_conv15h_t / Conv15H::grid_for, restated: items = (board, 16 output channels), persistent over two workgroups per CU"""
    return min(n * (cout // 16), 2 * num_cu)


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda", dtype=dtype)


def _run(x, w, b=None, r=None, relu=False):
    """-> (y as a NumPy array, the flag word)"""
    import torch
    from alphapig_amd import hipconv
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
    y = hipconv.conv3x3_fwd_f16x2_dense(_dev(x), _dev(w), None if b is None else _dev(b), None if r is None else _dev(r),
                                        relu=relu, flag=flag)
    torch.cuda.synchronize()
    return y.cpu().numpy(), int(flag.item())


_refs = {}


def _case(n, cin, cout):
    """(x, w, b, resid, float64 conv without bias): computed once per shape, read-only"""
    key = (n, cin, cout)
    if key not in _refs:
        x, w, b = op_case(n, cin, cout)
        r = np.random.RandomState(77 + n + cin).randn(n, cout, 15, 15).astype(np.float32)
        c = conv64(x, w, np.zeros(cout))
        for a in (x, w, b, r, c):
            a.setflags(write=False)
        _refs[key] = (x, w, b, r, c)
    return _refs[key]


def _want(c, b, r, variant):
    use_b, use_r, relu = VARIANTS[variant]
    want = c + (np.asarray(b, np.float64)[None, :, None, None] if use_b else 0.0) + (np.asarray(r, np.float64) if use_r else 0.0)
    return np.maximum(want, 0) if relu else want


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n,cin,cout", CASES, ids=["%dx%dto%d" % s for s in CASES])
def test_operator_against_float64(n, cin, cout, variant):
    assert conv15h_grid(n, cout, _cus()) == n * (cout // 16)         # one item per workgroup
    assert (cin // 16) // 4 == {64: 1, 128: 2, 192: 3, 256: 4}[cin]    # sub-chunks per wave
    x, w, b, r, c = _case(n, cin, cout)
    use_b, use_r, relu = VARIANTS[variant]
    got, flag = _run(x, w, b if use_b else None, r if use_r else None, relu)
    want = _want(c, b, r, variant)
    err, tol = float(np.abs(got - want).max()), op_tol(want)
    print("%s %s: error %.3g = %.4f of tol" % ((n, cin, cout), variant, err, err / tol))
    assert np.isfinite(got).all() and err <= tol, (err, tol)
    assert flag == 0


@pytest.mark.parametrize("variant", ["plain", "bias_resid_relu"])
def test_operator_with_more_items_than_workgroups(variant):
    """64 -> 256 at the smallest batch whose 16 n items exceed the grid of two workgroups per CU: some workgroups take a
    second item.  Against float64, and every board carries the bits of the same board launched alone."""
    cus = _cus()
    cin, cout = 64, 256
    n = 2 * cus // 16 + 1
    grid = conv15h_grid(n, cout, cus)
    assert grid == 2 * cus and 16 * (n - 1) <= grid < 16 * n, (cus, n, grid)
    x, w, b, r, c = _case(n, cin, cout)
    use_b, use_r, relu = VARIANTS[variant]
    got, flag = _run(x, w, b if use_b else None, r if use_r else None, relu)
    want = _want(c, b, r, variant)
    err, tol = float(np.abs(got - want).max()), op_tol(want)
    print("%s %s: error %.3g = %.4f of tol" % ((n, cin, cout), variant, err, err / tol))
    assert np.isfinite(got).all() and err <= tol, (err, tol)
    assert flag == 0
    differ = []
    for i in range(n):
        alone, f1 = _run(x[i:i + 1], w, b if use_b else None, r[i:i + 1] if use_r else None, relu)
        assert f1 == 0
        if not np.array_equal(alone[0], got[i]):
            differ.append(i)
    assert not differ, differ


# ---- the zero border of the LDS tile: integer-valued, no tolerance
PROBE_CELLS = [(0, 0), (0, 14), (14, 0), (14, 14), (0, 7), (14, 7), (7, 0), (7, 14)]
PROBE_CI, PROBE_CO = 37, 5


def _probe_board(cin):
    x = np.zeros((cin, 15, 15), np.float32)
    for y, c in PROBE_CELLS:
        x[PROBE_CI, y, c] = 1.0
    return x


def _probe_counts():
    """float64: the number of probe cells in every cell's 3x3 neighbourhood"""
    p = np.zeros((17, 17))
    for y, c in PROBE_CELLS:
        p[y + 1, c + 1] = 1.0
    return sum(p[ky:ky + 15, kx:kx + 15] for ky in range(3) for kx in range(3))


def _probe_weight(cin, cout, cos):
    w = np.zeros((cout, cin, 3, 3), np.float32)
    for co in cos:
        w[co, PROBE_CI] = 1.0
    return w


def test_border_probe_one_board():
    """Zero except the four corners and the middles of the four edges, an all-ones 3x3 weight in one channel: every output
    cell is the count of its neighbours, exactly -- a wrong halo or a padding column that is read shows as an integer."""
    x = _probe_board(64)[None]
    got, flag = _run(x, _probe_weight(64, 16, [PROBE_CO]))
    want = np.zeros((1, 16, 15, 15))
    want[0, PROBE_CO] = _probe_counts()
    assert want[0, PROBE_CO].max() == 1 and want[0, PROBE_CO].sum() == 4 * 4 + 4 * 6
    np.testing.assert_array_equal(got.astype(np.float64), want)
    assert flag == 0


def test_border_probe_behind_a_dense_board():
    """The same board as item 2 of the launch, after a dense first board."""
    dense = np.random.RandomState(5).randn(64, 15, 15).astype(np.float32)
    x = np.stack([dense, _probe_board(64)])
    got, flag = _run(x, _probe_weight(64, 16, [PROBE_CO]))
    want = np.zeros((16, 15, 15))
    want[PROBE_CO] = _probe_counts()
    np.testing.assert_array_equal(got[1].astype(np.float64), want)
    assert flag == 0


def test_border_probe_restaged_in_a_workgroup_that_held_a_dense_board():
    """... and as the LAST board of the launch with more items than workgroups: its sixteen items are the second items of
    workgroups 0 .. 15, whose tiles held the dense board 0 and then their partial sums.  The halo survives the restage."""
    cus = _cus()
    n = 2 * cus // 16 + 1
    assert conv15h_grid(n, 256, cus) == 16 * (n - 1)
    x = np.random.RandomState(6).randn(n, 64, 15, 15).astype(np.float32) * 3.0
    x[n - 1] = _probe_board(64)
    cos = [PROBE_CO + 16 * t for t in range(16)]
    got, flag = _run(x, _probe_weight(64, 256, cos))
    want = np.zeros((256, 15, 15))
    want[cos] = _probe_counts()
    np.testing.assert_array_equal(got[n - 1].astype(np.float64), want)
    assert flag == 0


def test_operator_raises_the_word_beyond_the_fp16_range():
    x, w, b, r, c = _case(1, 64, 16)
    big = np.array(x)
    big[0, 11, 7, 7] = 1.0e5
    _, flag = _run(big, w)
    assert flag == 1
    _, flag = _run(x, w)
    assert flag == 0


def test_operator_refuses_other_shapes():
    import torch
    from alphapig_amd import hipconv
    z = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(ValueError, match="multiple of 64"):
        hipconv.conv3x3_fwd_f16x2_dense(z(1, 9, 15, 15), z(64, 9, 3, 3))
    with pytest.raises(ValueError, match="multiple of 64"):
        hipconv.conv3x3_fwd_f16x2_dense(z(1, 64, 15, 15), z(24, 64, 3, 3))
    with pytest.raises(ValueError, match="15"):
        hipconv.conv3x3_fwd_f16x2_dense(z(1, 64, 8, 8), z(64, 64, 3, 3))


# ---- the evaluator
def _engine(cfg, prm, arith="f16x2", batch=MAX_BATCH):
    from alphapig_amd.policy_value_net import PolicyValueNet
    kind, side, blocks, nf = cfg
    return PolicyValueNet(side, side, batch_size=batch, n_blocks=blocks, n_filter=nf, model_params=prm, net_kind=kind,
                          trunk_arith=arith)


@pytest.fixture(scope="module", params=gn.GEN, ids=gn.GEN_IDS)
def gen(request):
    """(configuration, parameters, the f16x2 evaluator, the f32 evaluator): built once per net for the whole file."""
    cfg = request.param
    prm = gn.params(*cfg)
    split, exact = _engine(cfg, prm), _engine(cfg, prm, "f32")
    assert split.trunk_arith == "f16x2" and exact.trunk_arith == "f32"
    yield cfg, prm, split, exact
    split.close()
    exact.close()


_ref5 = {}


def _reference5(cfg, prm):
    if cfg not in _ref5:
        _ref5[cfg] = tn.Reference(prm, gn.positions(5, cfg[1])[1], cfg[0], cfg[2])
    return _ref5[cfg]


def _layer_records(net, ref, planes, n_layers):
    net.forward_planes(planes)
    recs, bad = [], []
    for l in range(n_layers):
        r, b = ref.check_layer(l, net.layer_output(l, len(planes)))
        recs.append(r)
        bad += b
    return recs, bad


def test_heads_and_every_layer_at_5_boards(gen):
    cfg, prm, split, _ = gen
    kind, side, blocks, nf = cfg
    chans = gn.layer_channels(kind, blocks, nf)
    assert all(ci % 64 == 0 and co % 16 == 0 for ci, co, _ in chans[1:])      # every layer behind the first is conv15h_kernel's
    _, planes = gn.positions(5, side)
    ref = _reference5(cfg, prm)
    before = split.trunk_overflows()
    rec, bad = ref.check_heads(split.forward_with_logits(planes))
    recs, bad2 = _layer_records(split, ref, planes, len(chans))
    print(gn.gen_id(*cfg), {k: "%.4f" % v for k, v in rec.items() if k.endswith("_over_bar")},
          [(r["layer"], "%.4f" % r["err_over_bar"], "%.4f" % r["chan_err_over_bar"]) for r in recs])
    assert not bad + bad2, bad + bad2
    probs, vals = split.forward_planes(planes)
    np.testing.assert_allclose(probs, ref.probs, rtol=0, atol=tn.HEAD_ATOL)
    np.testing.assert_allclose(vals, ref.value, rtol=0, atol=tn.HEAD_ATOL)
    assert split.trunk_overflows() == before == 0


def test_comparator_gate_against_the_fp32_generic_kernel(gen):
    cfg, prm, split, exact = gen
    kind, side, blocks, nf = cfg
    n_layers = len(gn.layer_channels(kind, blocks, nf))
    _, planes = gn.positions(5, side)
    ref = _reference5(cfg, prm)
    s, _ = _layer_records(split, ref, planes, n_layers)
    d, _ = _layer_records(exact, ref, planes, n_layers)
    print(gn.gen_id(*cfg), [(a["layer"], "%.3g" % a["err"], "%.3g" % b["err"]) for a, b in zip(s, d)])
    bad = [(a["layer"], a["err"], b["err"]) for a, b in zip(s, d) if not tn.comparator_gate(a["err"], b["err"], b["err"], a["scale"])]
    assert not bad, bad
    np.testing.assert_array_equal(split.layer_output(0, 5), exact.layer_output(0, 5))     # the first layer: the same kernel


def test_bits_do_not_depend_on_the_batch(gen):
    """Each of 70 positions alone, inside a launch of 33 and inside the launch of 70: the same bits, heads and logits."""
    cfg, prm, split, _ = gen
    _, planes = gn.positions(70, cfg[1])
    h70 = [np.asarray(a) for a in split.forward_with_logits(planes)]
    for lo in (0, 33, 37):
        for a, b in zip(split.forward_with_logits(planes[lo:lo + 33]), h70):
            np.testing.assert_array_equal(np.asarray(a), b[lo:lo + 33])
    differ = [i for i in range(70)
              if any(not np.array_equal(np.asarray(a)[0], b[i]) for a, b in zip(split.forward_with_logits(planes[i:i + 1]), h70))]
    assert not differ, differ
    assert split.trunk_overflows() == 0


def test_entry_points_and_loaders(gen):
    torch = pytest.importorskip("torch")
    cfg, prm, split, _ = gen
    codes, planes = gn.positions(33, cfg[1])
    pp, vp = split.forward_planes(planes)
    pc, vc = split.evaluate_codes(codes)
    np.testing.assert_array_equal(pc, pp)
    np.testing.assert_array_equal(vc, vp)
    pd, vd = split.policy_value_dev(torch.tensor(planes, device="cuda"))
    np.testing.assert_array_equal(pd, pp)
    np.testing.assert_array_equal(vd[:, 0], vp)
    for rep in range(4):                                     # (the third use of a slot replays a graph)
        ps, vs = split.evaluate_codes_slot(1, codes)
        np.testing.assert_array_equal(ps, pp, err_msg="slot, use %d" % rep)
        np.testing.assert_array_equal(vs, vp)
    dev = _engine(cfg, gn.params(*cfg, seed=gn.PARAM_SEED[gn.gen_id(*cfg)] + 100), batch=40)
    try:
        assert not np.array_equal(dev.forward_planes(planes)[0], pp)
        dev.load_device_params({k: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda") for k, v in prm.items()},
                               torch.cuda.current_stream().cuda_stream)
        p2, v2 = dev.forward_planes(planes)
        np.testing.assert_array_equal(p2, pp)
        np.testing.assert_array_equal(v2, vp)
        split.forward_planes(planes[:5])
        dev.forward_planes(planes[:5])
        for l in range(len(gn.layer_channels(cfg[0], cfg[2], cfg[3]))):
            np.testing.assert_array_equal(dev.layer_output(l, 5), split.layer_output(l, 5), err_msg="layer %d" % l)
    finally:
        dev.close()
    assert split.trunk_overflows() == 0


def _first_weight(kind):
    return "res_conv1_weight" if kind == "resnet" else "conv1_weight"


@pytest.mark.parametrize("cfg", [gn.GEN[0], gn.GEN[2]], ids=[gn.GEN_IDS[0], gn.GEN_IDS[2]])
def test_overflow_repeats_the_forward_on_the_fp32_generic_kernel(cfg):
    """The first layer's weights times 1e6: its outputs leave the fp16 range, the layer that reads them raises the forward's
    word and every collecting entry point answers with the bits of a trunk_arith="f32" engine."""
    torch = pytest.importorskip("torch")
    prm = gn.params(*cfg)
    big = dict(prm)
    big[_first_weight(cfg[0])] = np.asarray(prm[_first_weight(cfg[0])], np.float32) * 1.0e6
    codes, planes = gn.positions(33, cfg[1])
    exact, split = _engine(cfg, big, "f32", 40), _engine(cfg, big, "f16x2", 40)
    try:
        assert split.trunk_overflows() == 0
        a, b = exact.forward_with_logits(planes), split.forward_with_logits(planes)          # apz_forward
        assert split.trunk_overflows() == 1
        for x, y in zip(a, b):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        pa, pb = exact.forward_planes(planes), split.forward_planes(planes)                 # apz_forward_host
        assert split.trunk_overflows() == 2
        np.testing.assert_array_equal(pa[0], pb[0])
        np.testing.assert_array_equal(pa[1], pb[1])
        ca, cb = exact.evaluate_codes(codes), split.evaluate_codes(codes)                   # apz_forward_codes_host
        assert split.trunk_overflows() == 3
        np.testing.assert_array_equal(ca[0], cb[0])
        np.testing.assert_array_equal(ca[1], cb[1])
        t = torch.tensor(planes, device="cuda")
        da, db = exact.policy_value_dev(t), split.policy_value_dev(t)                       # apz_forward_dev_host
        assert split.trunk_overflows() == 4
        np.testing.assert_array_equal(da[0], db[0])
        np.testing.assert_array_equal(da[1], db[1])
        for rep in range(4):                                                                # apz_submit_codes / apz_wait, a graph replayed
            sa, sb = exact.evaluate_codes_slot(1, codes[:32]), split.evaluate_codes_slot(1, codes[:32])
            assert split.trunk_overflows() == 5 + rep
            np.testing.assert_array_equal(sa[0], sb[0])
            np.testing.assert_array_equal(sa[1], sb[1])
        split.set_params(prm)                       # ordinary weights afterwards: no repeat, the split kernel's own results
        q = split.forward_with_logits(planes[:5])
        assert split.trunk_overflows() == 8
        rec, bad = _reference5(cfg, prm).check_heads(q)
        assert not bad, bad
    finally:
        exact.close()
        split.close()


def test_large_activations_keep_the_relative_error():
    """The first layer's weights times 300 on the simple net: activations in the hundreds and thousands, the relative error of
    the last layer against float64 at the fp32 kernel's level (the figures of tests/test_gpu_conv8.py), no forward repeated."""
    from oracle import net_ref
    cfg = gn.GEN[0]
    prm = dict(gn.params(*cfg))
    prm["conv1_weight"] = np.asarray(prm["conv1_weight"], np.float32) * 300.0
    _, planes = gn.positions(12, cfg[1])
    layers = net_ref.forward(prm, planes, "simple", dtype=np.float64, return_layers=True)[4]
    want = layers[5]
    scale = np.abs(want).max()
    maxima = [float(np.abs(a).max()) for a in layers]
    print("float64 layer maxima", ["%.1f" % m for m in maxima])
    assert maxima[0] > 50.0 and scale > 10.0, maxima     # what conv15h_kernel reads is far above the order 1 of the other tests
    errs = {}
    for arith in ("f32", "f16x2"):
        net = _engine(cfg, prm, arith, 16)
        try:
            net.forward_planes(planes)
            errs[arith] = float(np.abs(net.layer_output(5, 12) - want).max() / scale)
            assert net.trunk_overflows() == 0
        finally:
            net.close()
    print(errs)
    assert errs["f32"] < 2e-6 and errs["f16x2"] < 2e-6, errs
    assert errs["f16x2"] < 3 * errs["f32"] + 2e-7, errs


def test_auto_is_still_f32_and_launches_what_it_launched(gen):
    cfg, prm, _, exact = gen
    from alphapig_amd.policy_value_net import PolicyValueNet
    kind, side, blocks, nf = cfg
    auto = PolicyValueNet(side, side, batch_size=8, n_blocks=blocks, n_filter=nf, model_params=prm, net_kind=kind)
    try:
        assert auto.trunk_arith == "f32"
        _, planes = gn.positions(5, side)
        for a, b in zip(auto.forward_with_logits(planes), exact.forward_with_logits(planes)):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        auto.forward_planes(planes)
        exact.forward_planes(planes)
        for l in range(len(gn.layer_channels(kind, blocks, nf))):
            np.testing.assert_array_equal(auto.layer_output(l, 5), exact.layer_output(l, 5))
        assert auto.trunk_overflows() == 0
    finally:
        auto.close()
