"""trunk15_wino3hs_kernel (csrc/trunk15_wino3hs.h): the small-batch form of the f16x2 trunk kernel, selected by
PolicyValueNet(uniform_trunk=True) / apz_set_trunk_uniform for batches of <= 32 boards.  Its contract is BIT equality with
trunk15_wino3h16_kernel (plain and scaled forms) for every output element of every board, so that a position's bits do not
depend on how many boards share its forward.  The reference is a second f16x2 net with the batched kernel forced onto the
small batch through the test hook apz_test_select_trunk(..., 4).

Nets: 15x15 / 128 filters / 3 blocks (six trunk launches, plain and residual), style="bench" weights."""
import os

import numpy as np
import pytest

from alphapig_amd import weights
from oracle import net_ref

from test_gpu_net import LOGIT_ATOL, random_positions

pytestmark = pytest.mark.gpu

EXPONENTS = [2, -1, 3, 0, -2, 1]            # the 0 mixes the plain form in


def _net(prm, batch=64, arith="f16x2", uniform=False, batched=False, n_blocks=3, k8=False, **kw):
    from alphapig_amd.policy_value_net import PolicyValueNet
    old = os.environ.pop("APZ_F16X2_K8", None)
    if k8:
        os.environ["APZ_F16X2_K8"] = "1"
    try:
        net = PolicyValueNet(15, 15, batch_size=batch, n_blocks=n_blocks, n_filter=128, model_params=prm, trunk_arith=arith,
                             uniform_trunk=uniform, **kw)
    finally:
        os.environ.pop("APZ_F16X2_K8", None)
        if old is not None:
            os.environ["APZ_F16X2_K8"] = old
    if batched:
        net._ck(net.L.apz_test_select_trunk(net._h, 4))
    return net


@pytest.fixture(scope="module")
def prm3():
    return weights.init_params("resnet", 15, 15, 9, 3, 128, seed=15, style="bench")


@pytest.fixture(scope="module")
def nets(prm3):
    """(uniform net, forced-batched net) on the same weights."""
    small, batched = _net(prm3, uniform=True), _net(prm3, batched=True)
    yield small, batched
    small.close()
    batched.close()


def _assert_same_bits(small, batched, planes, layers=(1, 2, 6)):
    n = len(planes)
    a = small.forward_with_logits(planes)
    b = batched.forward_with_logits(planes)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    small.forward_planes(planes)
    batched.forward_planes(planes)
    for layer in layers:
        np.testing.assert_array_equal(small.layer_output(layer, n), batched.layer_output(layer, n))
    return a


@pytest.mark.parametrize("n", [1, 2, 3, 7, 32])
def test_small_batch_f16x2_kernel_gives_the_batched_kernels_bits(nets, prm3, n):
    """A lone board, a full pair, a pair plus a lone board, an odd middle and the limit: logits, probabilities, value
    logits, values and the outputs of trunk layers 1, 2 and 6 carry the batched kernel's bits; logits within LOGIT_ATOL
    of the float64 oracle; no overflow."""
    small, batched = nets
    assert small.uniform_trunk and not batched.uniform_trunk
    _, planes = random_positions(n, 15, seed=500 + n)
    a = _assert_same_bits(small, batched, planes)
    o = net_ref.forward(prm3, planes, "resnet", 3, np.float64)
    np.testing.assert_allclose(a[0], o[0], rtol=0, atol=LOGIT_ATOL)
    assert small.trunk_overflows() == 0 and batched.trunk_overflows() == 0


def test_bits_across_the_32_33_boundary_on_one_engine(nets):
    """40 boards in one forward run the batched kernel; slices of 1, 7 and 32 of them on the SAME uniform engine run the
    small-batch kernel: every row equals its row of the 40-board forward."""
    small, _ = nets
    _, planes = random_positions(40, 15, seed=77)
    whole = [np.array(x, copy=True) for x in small.forward_with_logits(planes)]
    for lo, hi in ((0, 1), (5, 12), (8, 40)):
        part = small.forward_with_logits(planes[lo:hi])
        for x, y in zip(part, whole):
            np.testing.assert_array_equal(np.asarray(x), y[lo:hi])
    assert small.trunk_overflows() == 0


@pytest.mark.parametrize("n", [1, 7])
def test_scaled_form_gives_the_batched_scaled_kernels_bits(prm3, n):
    small, batched = _net(prm3, uniform=True), _net(prm3, batched=True)
    try:
        small.set_trunk_act_exponents(EXPONENTS)
        batched.set_trunk_act_exponents(EXPONENTS)
        assert list(small.trunk_act_exponents()) == EXPONENTS
        _, planes = random_positions(n, 15, seed=600 + n)
        _assert_same_bits(small, batched, planes)
        assert list(small.trunk_act_exponents()) == EXPONENTS
        assert list(batched.trunk_act_exponents()) == EXPONENTS
        assert small.trunk_overflows() == 0
        # (the exponents do change low-order bits: the scaled form really ran)
        plain = _net(prm3, uniform=True)
        try:
            assert not np.array_equal(_layer6(plain, planes), _layer6(small, planes))
        finally:
            plain.close()
    finally:
        small.close()
        batched.close()


def _layer6(net, planes):
    net.forward_planes(planes)
    return net.layer_output(6, len(planes))


def test_reduction_words_over_mixed_launches(prm3):
    """300 forwards (x 6 trunk launches) of changing sizes at random offsets on ONE uniform engine -- different subsets of
    the ticket words in use, plain and scaled forms, the exponents changed half way: every result equals the forced-
    batched reference for those boards."""
    _, planes = random_positions(32, 15, seed=901)
    batched = _net(prm3, batch=32, batched=True)
    refs = [batched.forward_planes(planes)]
    batched.set_trunk_act_exponents(EXPONENTS)
    refs.append(batched.forward_planes(planes))
    refs = [(np.array(p, copy=True), np.array(v, copy=True)) for p, v in refs]
    batched.close()
    assert not np.array_equal(refs[0][0], refs[1][0])
    small = _net(prm3, batch=32, uniform=True)
    try:
        sizes = [1, 32, 2, 7, 31, 3, 16, 1, 24, 5]
        rs = np.random.RandomState(4)
        for it in range(300):
            if it == 150:
                small.set_trunk_act_exponents(EXPONENTS)
            ref_p, ref_v = refs[it >= 150]
            n = sizes[it % len(sizes)]
            lo = int(rs.randint(0, 32 - n + 1))
            p, v = small.forward_planes(planes[lo:lo + n])
            assert np.array_equal(p, ref_p[lo:lo + n]) and np.array_equal(v, ref_v[lo:lo + n]), (it, n, lo)
        assert small.trunk_overflows() == 0
    finally:
        small.close()


def test_overflow_repeats_the_small_forward_on_the_exact_kernel():
    """Stem outputs far beyond the fp16 range in a 5-board batch on the uniform route: the small-batch kernel raises the
    word, the forward is repeated on the exact-fp32 kernel and carries its bits; ordinary weights: no repeat."""
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=41, style="bench")
    big = dict(prm)
    big["res_conv1_weight"] = np.asarray(prm["res_conv1_weight"], np.float32) * 3.0e4
    _, planes = random_positions(5, 15, seed=18)
    exact = _net(big, n_blocks=2, arith="f32")
    split = _net(big, n_blocks=2, uniform=True)
    ok = _net(prm, n_blocks=2, uniform=True)
    try:
        assert split.trunk_overflows() == 0
        a, b = exact.forward_with_logits(planes), split.forward_with_logits(planes)
        assert split.trunk_overflows() == 1
        for x, y in zip(a, b):
            assert np.isfinite(np.asarray(y)).all()
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        ok.forward_with_logits(planes)
        assert ok.trunk_overflows() == 0
    finally:
        exact.close()
        split.close()
        ok.close()


def test_forward_graphs_replay_the_small_batch_kernel(prm3):
    """apz_set_forward_graphs on a uniform net: the third submission of (slot, 4 boards) captures the launch sequence with
    trunk15_wino3hs_kernel in it (every launch of the capture carries its own epoch) and later ones replay it: the bits of
    the plain launches, also for new positions in the slot."""
    codes, _ = random_positions(8, 15, seed=31)
    net = _net(prm3, uniform=True)
    try:
        def run(lo):
            k = net.submit_codes_slot(0, codes[lo:lo + 4])
            p, v = net.wait_slot(0, k)
            return np.array(p, copy=True), np.array(v, copy=True)

        net._ck(net.L.apz_set_forward_graphs(net._h, 0))
        plain, plain_b = run(0), run(4)
        assert not np.array_equal(plain[0], plain_b[0])
        net._ck(net.L.apz_set_forward_graphs(net._h, 1))
        for rep in range(5):                                    # 1, 2: plain; 3: captured + launched; 4, 5: replayed
            p, v = run(0)
            np.testing.assert_array_equal(p, plain[0])
            np.testing.assert_array_equal(v, plain[1])
        p, v = run(4)
        np.testing.assert_array_equal(p, plain_b[0])
        np.testing.assert_array_equal(v, plain_b[1])
        assert net.trunk_overflows() == 0
    finally:
        net.close()


def test_default_route_is_untouched(prm3):
    """Without the switch trunk_arith="f16x2" still runs 7 boards on the exact-fp32 small-batch kernel."""
    _, planes = random_positions(7, 15, seed=507)
    split, exact = _net(prm3), _net(prm3, arith="f32")
    try:
        assert split.uniform_trunk is False
        for x, y in zip(split.forward_with_logits(planes), exact.forward_with_logits(planes)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    finally:
        split.close()
        exact.close()


def test_unsupported_and_no_op_cases(prm3):
    from alphapig_amd.policy_value_net import PolicyValueNet
    UNSUPPORTED = -4                                            # APZ_E_UNSUPPORTED
    for kw in (dict(arith="bf16x3"), dict(k8=True)):
        net = _net(prm3, **kw)
        try:
            assert net.L.apz_set_trunk_uniform(net._h, 1) == UNSUPPORTED
            assert len(net.L.apz_last_error()) > 0
        finally:
            net.close()
    net = _net(prm3, arith="f32")
    try:
        assert net.L.apz_set_trunk_uniform(net._h, 1) == 0
    finally:
        net.close()
    p8 = weights.init_params("resnet", 8, 8, 9, 2, 64, seed=4, style="bench")
    net8 = PolicyValueNet(8, 8, batch_size=16, n_blocks=2, n_filter=64, model_params=p8, uniform_trunk=True)
    try:
        assert net8.L.apz_set_trunk_uniform(net8._h, 1) == 0
        assert net8.L.apz_set_trunk_uniform(net8._h, 0) == 0
    finally:
        net8.close()
