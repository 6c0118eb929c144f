"""trunk15_wino3h16_kernel (csrc/trunk15_wino3h16.h): the f16x2 trunk kernel for batches of more than 32 boards, with
16-channel chunks and three term products (H.Vlo + L.Vhi + H.Vhi) -- against the float64 oracle, against its predecessor
trunk15_wino3h_kernel (selected by APZ_F16X2_K8=1 at engine creation), for launch-shape- and position-independent bits, and
with the overflow word that repeats a forward on the exact kernel."""
import os

import numpy as np
import pytest

from alphapig_amd import weights
from oracle import net_ref

from test_gpu_net import LOGIT_ATOL, random_positions

pytestmark = pytest.mark.gpu


def _net(prm, n_blocks, batch, arith="f16x2", k8=False):
    from alphapig_amd.policy_value_net import PolicyValueNet
    old = os.environ.pop("APZ_F16X2_K8", None)
    if k8:
        os.environ["APZ_F16X2_K8"] = "1"
    try:
        return PolicyValueNet(15, 15, batch_size=batch, n_blocks=n_blocks, n_filter=128, model_params=prm, trunk_arith=arith)
    finally:
        os.environ.pop("APZ_F16X2_K8", None)
        if old is not None:
            os.environ["APZ_F16X2_K8"] = old


@pytest.fixture(scope="module")
def prm10():
    return weights.init_params("resnet", 15, 15, 9, 10, 128, seed=0, style="bench")


@pytest.mark.parametrize("n", [33, 100, 511, 600])
def test_k16_kernel_against_oracle_and_bits_independent_of_place(prm10, n):
    net = _net(prm10, 10, 600)
    try:
        _, planes = random_positions(n, 15, seed=900 + n)
        logits, probs, vlog, vals = net.forward_with_logits(planes)
        rows = sorted(set([0, 1, n // 2, n - 2, n - 1]) | set(np.random.RandomState(n).permutation(n)[:11].tolist()))
        o_logits, o_probs, o_vlog, o_vals = net_ref.forward(prm10, planes[rows], "resnet", 10, np.float64)
        np.testing.assert_allclose(logits[rows], o_logits, rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(vlog[rows], o_vlog[:, 0], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(probs[rows], o_probs, rtol=0, atol=2e-5)
        np.testing.assert_allclose(vals[rows], o_vals[:, 0], rtol=0, atol=2e-5)
        perm = np.random.RandomState(1).permutation(n)
        p2 = net.forward_with_logits(planes[perm])
        np.testing.assert_array_equal(p2[0], logits[perm])
        np.testing.assert_array_equal(p2[2], vlog[perm])
        sub = net.forward_with_logits(planes[n - 33:])             # the last 33 boards: same kernel, other launch shape
        np.testing.assert_array_equal(sub[0], logits[n - 33:])
        assert net.trunk_overflows() == 0
    finally:
        net.close()


def test_k16_kernel_10_blocks_512_boards_agrees_with_the_k8_kernel(prm10):
    """The bench's launch shape on both f16x2 kernels: the same leaf probabilities and values to 2e-5, logits to 1e-4 (the
    two differ in low-order bits only: the new one drops the lo.lo product and sums in another order)."""
    _, planes = random_positions(512, 15, seed=4242)
    new, old = _net(prm10, 10, 512), _net(prm10, 10, 512, k8=True)
    try:
        a, b = new.forward_with_logits(planes), old.forward_with_logits(planes)
        np.testing.assert_allclose(a[0], b[0], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(a[1], b[1], rtol=0, atol=2e-5)
        np.testing.assert_allclose(a[2], b[2], rtol=0, atol=LOGIT_ATOL)
        np.testing.assert_allclose(a[3], b[3], rtol=0, atol=2e-5)
        rows = [0, 1, 255, 256, 510, 511]
        o = net_ref.forward(prm10, planes[rows], "resnet", 10, np.float64)
        np.testing.assert_allclose(a[0][rows], o[0], rtol=0, atol=LOGIT_ATOL)
    finally:
        new.close()
        old.close()


def test_k16_overflow_repeats_the_forward_on_the_exact_kernel():
    """Stem outputs far beyond the fp16 range in a 100-board batch: the non-finite trunk output raises the word, the forward
    is repeated on the exact-fp32 kernel, and the results carry that kernel's bits."""
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=41, style="bench")
    big = dict(prm)
    big["res_conv1_weight"] = np.asarray(prm["res_conv1_weight"], np.float32) * 3.0e4
    _, planes = random_positions(100, 15, seed=18)
    exact = _net(big, 2, 128, arith="f32")
    split = _net(big, 2, 128)
    try:
        assert split.trunk_overflows() == 0
        a, b = exact.forward_with_logits(planes), split.forward_with_logits(planes)
        assert split.trunk_overflows() == 1
        for x, y in zip(a, b):
            assert np.isfinite(np.asarray(y)).all()
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        ok = _net(prm, 2, 128)                                  # ordinary weights: no repeat
        try:
            ok.forward_with_logits(planes)
            assert ok.trunk_overflows() == 0
        finally:
            ok.close()
    finally:
        exact.close()
        split.close()
