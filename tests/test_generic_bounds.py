"""The bars of tests/test_gpu_generic_nets.py, tried on the CPU: a bar that plain float32 arithmetic cannot meet is a wrong bar.
The three nets of the generic convolution route (tests/generic_nets.py: the simple net and the one-block residual nets of 64 and
256 filters, all 15x15, weights.init_params(style="bench")) on 12 boards: the inference graph with PyTorch's float32 library
operators against tests/trained_nets.Reference (float64): every layer, every output channel (against (1e-4 / 3) * max(1, A_c)),
logits, value logit, probabilities and values stay within a QUARTER of their bar, and channels the oracle calls dead are
exactly 0.  Also: the launch rule of tests/generic_nets.py on the 256 CUs the GPU cases are written for."""
import numpy as np
import pytest

import generic_nets as gn
import trained_nets as tn

TABLE = gn.Table("r25_generic_bounds")


@pytest.mark.parametrize("kind,side,blocks,nf", gn.GEN, ids=gn.GEN_IDS)
def test_float32_meets_a_quarter_of_every_bar_on_the_generic_nets(kind, side, blocks, nf):
    import torch
    prm = gn.params(kind, side, blocks, nf)
    _, planes = gn.positions(12, side)
    ref = tn.Reference(prm, planes, kind, blocks)
    chans = gn.layer_channels(kind, blocks, nf)
    assert [a.shape[1] for a in ref.layers] == [co for _, co, _ in chans]
    got = tn.torch_forward_layers(prm, planes, kind, blocks, torch.float32)
    rec, bad = ref.check_heads(got[:4])
    worst = {k: v for k, v in rec.items() if k.endswith("_over_bar")}
    for l, a in enumerate(got[4]):
        r, b = ref.check_layer(l, a)
        bad += b
        worst["layer%d" % l] = r["err_over_bar"]
        worst["layer%d_chan" % l] = r["chan_err_over_bar"]
    print(gn.gen_id(kind, side, blocks, nf), {k: "%.4f" % v for k, v in worst.items()})
    TABLE.add(net=gn.gen_id(kind, side, blocks, nf), n=len(planes), float32_err_over_bar=worst)
    assert not bad, bad
    assert max(worst.values()) <= 0.25, worst


def test_reference_bars_do_not_depend_on_the_filter_count():
    """Reference takes its shapes from the parameters: the bars are TOL * max(1, scale) for every width, 128 included."""
    assert tn.TOL == 1e-4 / 3.0 and tn.HEAD_ATOL == 2e-5
    for (kind, side, blocks, nf) in gn.GEN + (("resnet", 15, 1, 128),):
        prm = gn.params(kind, side, blocks, nf, seed=7)
        _, planes = gn.positions(2, side)
        ref = tn.Reference(prm, planes, kind, blocks)
        for l in range(len(ref.layers)):
            assert ref.layer_bar(l) == tn.TOL * max(1.0, float(np.abs(ref.layers[l]).max()))
            np.testing.assert_array_equal(ref.chan_bar(l), tn.TOL * np.maximum(1.0, ref.A[l]))
            assert ref.A[l].shape == (ref.layers[l].shape[1],)


def test_launch_rule_on_256_compute_units():
    """The forms the GPU cases name, from the restated rule at the MI355X's 256 CUs."""
    cu = 256
    # LDS of a board's tile: 9 -> 12 channels, 64, 128 and 256 (two chunks of 128) at 15x15; one chunk of 256 at 8x8
    assert [gn.conv_lds_bytes(c, 15) for c in (9, 64, 128, 256)] == [13312, 69888, 139520, 139520]
    assert gn.conv_chunk(256, 15) == 128 and gn.conv_chunk(256, 8) == 256 and gn.conv_lds_bytes(256, 8) == 114944
    f = gn.evaluator_form
    assert f(5, 128, 256, 15, cu)[:3] == (1, 4, True) and f(5, 64, 64, 15, cu)[:3] == (1, 1, False)
    assert f(129, 256, 256, 15, cu)[:3] == (4, 1, False) and f(129, 64, 128, 15, cu)[:3] == (1, 2, True)
    assert f(257, 128, 128, 15, cu)[:3] == (2, 1, False)
    assert f(257, 128, 128, 15, cu).second_board and f(257, 256, 256, 15, cu).chunks == 2
    assert not f(257, 64, 128, 15, cu).second_board and f(257, 64, 128, 15, cu).per_cu == 2
    g = gn.operator_form
    assert [g(257, 256, co, 8, cu).ct for co in (64, 128, 256)] == [1, 2, 4]
    assert all(g(257, 256, co, 8, cu).second_board and g(257, 256, co, 8, cu).per_cu == 1 for co in (64, 128, 256))
    assert g(257, 256, 64, 15, cu).chunks == 2 and g(257, 128, 64, 15, cu).chunks == 1
    stem = g(4 * cu + 1, 9, 64, 8, cu)
    assert stem.per_cu == 4 and stem.grid == 4 * cu and stem.second_board
    assert g(4 * cu + 1, 9, 64, 15, cu) == stem          # the same at 15x15: 12 channels of 272 floats fit four times
    # every direct case of test_conv3x3_fwd_dgrad_wgrad_bias's first list: one tile per workgroup, no second board
    for n, ci, co, hw in [(5, 128, 128, 15), (3, 9, 128, 15), (130, 128, 128, 15), (7, 64, 64, 8), (4, 64, 128, 8), (2, 256, 256, 8),
                          (3, 256, 256, 15), (6, 128, 64, 15)]:
        for a, b in ((ci, co), (co, ci))[:2 if ci >= 64 else 1]:       # forward, data gradient (none into the 9 planes)
            assert g(n, a, b, hw, cu).ct == 1 and not g(n, a, b, hw, cu).second_board
