"""The arithmetic behind the framed engines (csrc/frame15.h), in numpy float64, without a GPU.

A square board of side S < 15 is embedded in the top-left S x S window of a 15x15 frame of zeros.  The residual net of
oracle/net_ref.py is run on the frame, layer by layer, with the off-board cells of every layer's output set to zero
before the next layer reads them, and the heads read the S x S crop: that is net_ref.forward on the S x S planes, to
rounding (1e-12; the two forms add the same products, the frame's adds more zeros).  Without the clearing the
bias-and-neighbour values a layer leaves outside the window flow back over the board's edge: the edge cells of the trunk
output then differ by more than 1e-3, which is why the engine pays for a clear after every layer."""
import numpy as np
import pytest

from alphapig_amd import weights
from oracle import net_ref

N_BLOCKS = 2
FRAME = 15


def planes_for(side, n, seed):
    """binary planes with the colour plane all ones on even boards, all zeros on odd ones"""
    rs = np.random.RandomState(seed)
    x = (rs.rand(n, 9, side, side) < 0.3).astype(np.float64)
    x[:, 8] = (np.arange(n) % 2 == 0)[:, None, None]
    return x


def framed_forward(prm, planes, n_blocks, clear):
    """-> (logits, probs, value logit, value, [every layer's S x S crop])"""
    n, c, side, _ = planes.shape
    dt = np.float64

    def mask(a):
        if clear:
            a = a.copy()
            a[:, :, side:, :] = 0.0
            a[:, :, :side, side:] = 0.0
        return a

    x = np.zeros((n, c, FRAME, FRAME), dtype=dt)
    x[:, :, :side, :side] = planes
    x = mask(net_ref._conv_act(x, prm, "res_conv1"))
    layers = [x[:, :, :side, :side]]
    for i in range(1, n_blocks + 1):
        skip = x
        y = net_ref._conv(x, prm["convA%d_weight" % i].astype(dt), prm["convA%d_bias" % i].astype(dt))
        y = mask(np.maximum(net_ref._bn(y, prm, "bnA%d" % i, False, ("_moving_mean", "_moving_var")), 0))
        layers.append(y[:, :, :side, :side])
        y = net_ref._conv(y, prm["convB%d_weight" % i].astype(dt), prm["convB%d_bias" % i].astype(dt))
        y = net_ref._bn(y, prm, "bnB%d" % i, False, ("_moving_mean", "_moving_var"))
        x = np.maximum(y + skip, 0)
        if i < n_blocks:                    # the last layer's off-board cells are never read: the heads take the crop
            x = mask(x)
        layers.append(x[:, :, :side, :side])
    return net_ref._heads(np.ascontiguousarray(x[:, :, :side, :side]), prm) + (layers,)


@pytest.mark.parametrize("side", [6, 9, 14])
def test_cleared_frame_equals_the_small_board_and_the_clear_is_needed(side):
    prm = weights.init_params("resnet", side, side, 9, N_BLOCKS, 128, seed=20 + side, style="bench")
    planes = planes_for(side, 3, seed=side)
    ref = net_ref.forward(prm, planes, "resnet", N_BLOCKS, np.float64, return_layers=True)
    got = framed_forward(prm, planes, N_BLOCKS, clear=True)
    for a, b in zip(got[:4], ref[:4]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    assert len(got[4]) == len(ref[4]) == 2 * N_BLOCKS + 1
    for a, b in zip(got[4], ref[4]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    # the same without the clear: wrong at the board's last row and last column
    dirty = framed_forward(prm, planes, N_BLOCKS, clear=False)
    edge = np.zeros((side, side), dtype=bool)
    edge[side - 1, :] = True
    edge[:, side - 1] = True
    d = np.abs(dirty[4][-1] - ref[4][-1])
    print("side %d: without the clear the trunk output differs by %.3g at edge cells, %.3g elsewhere; logits by %.3g"
          % (side, d[:, :, edge].max(), d[:, :, ~edge].max(), np.abs(dirty[0] - ref[0]).max()))
    assert d[:, :, edge].max() > 1e-3
    # ... and the stem, which reads the zero-embedded planes, is still right: the error enters with the second layer
    np.testing.assert_allclose(dirty[4][0], ref[4][0], rtol=0, atol=1e-12)
