"""The evaluator on the generic convolution route: every 15x15 net that is not the 128-filter residual net runs all its 3x3 layers
on conv3x3_mfma_kernel (csrc/conv3x3_mfma.h through launch_conv_generic / launch_conv_t / launch_conv_r), expands position codes
with encode_planes_kernel and takes the dense head path (head_conv1x1_kernel, head_fc_kernel<1, true>).  The three nets of
tests/generic_nets.py -- the simple net, and the one-block residual net with 64 and with 256 filters -- against
tests/trained_nets.Reference (float64; tests/test_generic_bounds.py shows on the CPU that plain float32 sits at a hundredth of
these bars), per layer and per output channel, at the three batch sizes where the launch rule changes form:

  n = 5             layers of 128 / 256 output channels split over 2 / 4 workgroups of one 64-channel tile per board
  n = CUs / 2 + 1   256-channel layers unsplit with CT = 4 tiles per workgroup, 128-channel layers still split
  n = CUs + 1       nothing split (CT = 2 for 128 channels); every layer of >= 128 input channels has one workgroup per CU, so
                    exactly one workgroup takes a second board (the 256-channel ones restage two LDS chunks for it)

Every case asserts the form of every layer of its net from the device's CU count (the rule restated in tests/generic_nets.py).
The measured ratios go to <APZ_TABLE_DIR>/r25_generic_route.json when that variable is set (profiles/r25_generic_route.md)."""
import time

import numpy as np
import pytest

import generic_nets as gn
import trained_nets as tn

pytestmark = pytest.mark.gpu

MAX_BATCH = 300
TABLE = gn.Table("r25_generic_route")
_nets = {}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(cfg, prm, batch=MAX_BATCH):
    from alphapig_amd.policy_value_net import PolicyValueNet
    kind, side, blocks, nf = cfg
    return PolicyValueNet(side, side, batch_size=batch, n_blocks=blocks, n_filter=nf, model_params=prm, net_kind=kind)


@pytest.fixture(scope="module", params=gn.GEN, ids=gn.GEN_IDS)
def gen(request):
    """(configuration, parameters, one evaluator of up to 300 boards): built once per net for the whole file."""
    cfg = request.param
    prm = gn.params(*cfg)
    net = _engine(cfg, prm)
    assert net.trunk_arith == "f32"
    yield cfg, prm, net
    net.close()


def _forms(cfg, n):
    kind, side, blocks, nf = cfg
    return [gn.evaluator_form(n, ci, co, side, _cus()) for ci, co, _ in gn.layer_channels(kind, blocks, nf)]


def _small_launch_heads(net, planes):
    """forward_with_logits of every board in launches of 5 (the last launch takes the batch's last five boards)"""
    n = len(planes)
    out = None
    for lo in list(range(0, n - 4, 5)) + [n - 5]:
        part = [np.asarray(a) for a in net.forward_with_logits(planes[lo:lo + 5])]
        if out is None:
            out = [np.empty((n,) + a.shape[1:], np.float32) for a in part]
        for o, a in zip(out, part):
            o[lo:lo + 5] = a
    return out


def test_heads_and_every_layer_at_5_boards(gen):
    """Logits, probabilities, value logit and values, then every convolution layer (apz_layer_io) per layer and per output
    channel, against float64: 6 layers of the simple net, 3 of the one-block residual nets, all in the split form."""
    cfg, prm, net = gen
    kind, side, blocks, nf = cfg
    t0 = time.time()
    chans = gn.layer_channels(kind, blocks, nf)
    forms = _forms(cfg, 5)
    for (ci, co, _), f in zip(chans, forms):          # 128 / 256 output channels: split; 64: one tile, never split
        assert (f.ct, f.groups, f.second_board) == (1, co // 64, False), (ci, co, f)
    assert len(chans) == (6 if kind == "simple" else 3)
    _, planes = gn.positions(5, side)
    ref = tn.Reference(prm, planes, kind, blocks)
    rec, bad = ref.check_heads(net.forward_with_logits(planes))
    probs, vals = net.forward_planes(planes)
    layers = []
    for l in range(len(chans)):
        r, b = ref.check_layer(l, net.layer_output(l, 5))
        bad += b
        layers.append({"layer": l, "form": gn.form_name(forms[l]), "residual": chans[l][2], "err_over_bar": r["err_over_bar"],
                       "chan_err_over_bar": r["chan_err_over_bar"], "dead_channels": r["dead_channels"]})
    print(gn.gen_id(*cfg), {k: "%.4f" % v for k, v in rec.items() if k.endswith("_over_bar")},
          [(x["layer"], "%.4f" % x["err_over_bar"], "%.4f" % x["chan_err_over_bar"]) for x in layers])
    TABLE.add(test="heads_and_every_layer_at_5_boards", net=gn.gen_id(*cfg), n=5,
              heads={k: v for k, v in rec.items() if k.endswith("_over_bar")}, layers=layers, seconds=round(time.time() - t0, 3))
    assert not bad, bad
    np.testing.assert_allclose(probs, ref.probs, rtol=0, atol=tn.HEAD_ATOL)
    np.testing.assert_allclose(vals, ref.value, rtol=0, atol=tn.HEAD_ATOL)


@pytest.mark.parametrize("batch", ["four_tiles_unsplit", "second_board"])
def test_large_batches_oracle_rows_and_the_small_launchs_bits(gen, batch):
    """Rows 0, 1, CUs - 1, CUs, n - 1 (those the batch has) and 20 seeded random rows against float64: heads, and every layer
    per channel.  EVERY row must carry the bits of the same board evaluated in a launch of 5 -- launch_conv_t documents the
    same arithmetic in the same order for the split and the unsplit form, and the test above holds the launch of 5 to the
    oracle on all its layers."""
    cfg, prm, net = gen
    kind, side, blocks, nf = cfg
    t0 = time.time()
    cus = _cus()
    n = cus // 2 + 1 if batch == "four_tiles_unsplit" else cus + 1
    assert n <= MAX_BATCH, (n, cus)
    chans = gn.layer_channels(kind, blocks, nf)
    forms = _forms(cfg, n)
    for (ci, co, _), f in zip(chans, forms):
        if batch == "four_tiles_unsplit":              # 256 channels: CT = 4 unsplit; 128: still two workgroups per board
            assert (f.ct, f.groups) == {64: (1, 1), 128: (1, 2), 256: (4, 1)}[co], (ci, co, f)
            assert not f.second_board
        else:                                          # nothing split; >= 128 input channels: one workgroup per CU, one board more
            assert (f.ct, f.groups) == (co // 64, 1), (ci, co, f)
            assert f.second_board == (ci >= 128) and (ci < 128 or (f.per_cu == 1 and f.grid == n - 1)), (ci, co, f)
            assert f.chunks == (2 if ci == 256 else 1)
    _, planes = gn.positions(n, side)
    rows = sorted(set(r for r in (0, 1, cus - 1, cus, n - 1) if r < n) |
                  set(np.random.RandomState(25).permutation(n)[:20].tolist()))
    ref = tn.Reference(prm, planes[rows], kind, blocks)
    heads = net.forward_with_logits(planes)
    rec, bad = ref.check_heads([np.asarray(a)[rows] for a in heads])
    net.forward_planes(planes)
    layers = []
    for l in range(len(chans)):
        r, b = ref.check_layer(l, net.layer_output(l, n)[rows])
        bad += b
        layers.append({"layer": l, "form": gn.form_name(forms[l]), "residual": chans[l][2], "err_over_bar": r["err_over_bar"],
                       "chan_err_over_bar": r["chan_err_over_bar"]})
    small = _small_launch_heads(net, planes)
    differ = {name: np.flatnonzero((np.asarray(a).reshape(n, -1) != b.reshape(n, -1)).any(axis=1)).tolist()
              for name, a, b in zip(("logits", "probs", "value_logit", "values"), heads, small)}
    print(gn.gen_id(*cfg), batch, n, {k: "%.4f" % v for k, v in rec.items() if k.endswith("_over_bar")},
          [(x["layer"], "%.4f" % x["err_over_bar"], "%.4f" % x["chan_err_over_bar"]) for x in layers], differ)
    TABLE.add(test="large_batches_oracle_rows_and_the_small_launchs_bits", net=gn.gen_id(*cfg), batch=batch, n=n, oracle_rows=rows,
              heads={k: v for k, v in rec.items() if k.endswith("_over_bar")}, layers=layers,
              rows_whose_bits_differ_from_a_launch_of_5={k: len(v) for k, v in differ.items()}, seconds=round(time.time() - t0, 3))
    assert not bad, bad
    assert not any(differ.values()), {k: v[:10] for k, v in differ.items()}


@pytest.mark.parametrize("batch", ["5", "second_board"])
def test_codes_path_gives_the_planes_paths_bits(gen, batch):
    """These nets have no stem that reads position codes: evaluate_codes expands them with encode_planes_kernel first."""
    cfg, prm, net = gen
    t0 = time.time()
    n = 5 if batch == "5" else _cus() + 1
    assert n <= MAX_BATCH
    codes, planes = gn.positions(n, cfg[1])
    pc, vc = net.evaluate_codes(codes)
    pp, vp = net.forward_planes(planes)
    np.testing.assert_array_equal(pc, pp)
    np.testing.assert_array_equal(vc, vp)
    assert np.abs(pp.sum(axis=1) - 1).max() < 1e-5
    TABLE.add(test="codes_path_gives_the_planes_paths_bits", net=gn.gen_id(*cfg), n=n, seconds=round(time.time() - t0, 3))


def test_device_weight_install_gives_the_host_installs_bits(gen):
    """apz_load_weights_dev on these nets: pack_direct_kernel for every 3x3 layer, the dense 15x15 forms of
    pack_head_conv_kernel and pack_fc_kernel.  An engine built on other weights and refreshed from device tensors answers with
    the bits of the engine that was given the weights from the host -- heads and every layer."""
    torch = pytest.importorskip("torch")
    cfg, prm, host = gen
    kind, side, blocks, nf = cfg
    t0 = time.time()
    _, planes = gn.positions(5, side)
    dev = _engine(cfg, gn.params(*cfg, seed=gn.PARAM_SEED[gn.gen_id(*cfg)] + 100), batch=8)
    try:
        before = dev.forward_with_logits(planes)
        tensors = {k: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda") for k, v in prm.items()}
        dev.load_device_params(tensors, torch.cuda.current_stream().cuda_stream)
        want, got = host.forward_with_logits(planes), dev.forward_with_logits(planes)
        assert np.abs(before[0] - want[0]).max() > 1e-3          # the refresh changed something
        for name, a, b in zip(("logits", "probs", "value_logit", "values"), got, want):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=name)
        host.forward_planes(planes)
        dev.forward_planes(planes)
        for l in range(len(gn.layer_channels(kind, blocks, nf))):
            np.testing.assert_array_equal(dev.layer_output(l, 5), host.layer_output(l, 5), err_msg="layer %d" % l)
    finally:
        dev.close()
    TABLE.add(test="device_weight_install_gives_the_host_installs_bits", net=gn.gen_id(*cfg), n=5, seconds=round(time.time() - t0, 3))
