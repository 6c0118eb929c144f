"""CPU-side checks of the framed-board interface (square boards of 6x6 .. 14x14 on the 15x15 trunk kernels,
csrc/frame15.h): the built library exports the new test hook and the header declares it, the Python binding knows it, and
the trainer refuses such a net at construction, before it looks for a GPU."""
import os
import re

import pytest

from alphapig_amd import _native, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_layer_frame():
    L = _native.hip()
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    assert re.search(r"\bint\s+apz_layer_frame\s*\(\s*apz_engine\s*\*", hdr)
    assert "apz_layer_frame" in _native.HIP_SYMBOLS
    assert hasattr(L, "apz_layer_frame")
    assert L.apz_layer_frame.argtypes is not None and len(L.apz_layer_frame.argtypes) == 4


def test_header_says_which_boards_are_supported():
    hdr = open(os.path.join(ROOT, "include", "alphapig_hip.h")).read()
    assert "csrc/frame15.h" in hdr and "framed" in hdr


@pytest.mark.parametrize("side", [9, 13])
def test_trainer_refuses_a_framed_net_without_looking_for_a_gpu(side):
    from alphapig_amd.train import HipTrainer, check_trainable_board
    prm = weights.init_params("resnet", side, side, 9, 1, 128, seed=1, style="bench")
    with pytest.raises(ValueError, match="15x15 and 8x8") as ei:
        check_trainable_board(prm)
    assert "%dx%d" % (side, side) in str(ei.value)
    with pytest.raises(ValueError, match="15x15 and 8x8"):          # (a RuntimeError here would be the GPU check coming first)
        HipTrainer(prm, "resnet", 1, batch_size=8)


@pytest.mark.parametrize("side", [8, 15])
def test_trainable_boards_pass_the_shape_check(side):
    from alphapig_amd.train import check_trainable_board
    check_trainable_board(weights.init_params("resnet", side, side, 9, 1, 128, seed=1, style="bench"))
