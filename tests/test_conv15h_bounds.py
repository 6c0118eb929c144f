"""The bars of tests/test_gpu_conv15h.py, tried on the CPU: what conv15h_kernel (csrc/conv15_split.h) can and cannot represent.

A float64 emulation of the two-term split -- every activation as hi = fp16(x), lo = fp16(x - hi); every weight times the
per-output-channel power of two S[co] of f16x2_scale_for, split the same way; all four term products, summed in float64, S
undone in the bias step -- against the float64 convolution of the unsplit operands.  What is left is the error of the
REPRESENTATION, the part no accumulation order can remove.  It must stay under a quarter of every bar the GPU tests use:

  operator shapes   2e-5 * max |float64| + 1e-6 (the forward bar of tests/test_gpu_train.py), at inputs of order 1, of order
                    300 and of order 1e-3 (the low end: the lo terms reach the fp16 subnormals; documented, not guarded)
  layer 1 of the three nets of tests/generic_nets.py   trained_nets.Reference's layer bar and per-channel bars

Plain float32 accumulation of the unsplit operands (PyTorch's CPU convolution) is held to the same quarter at orders 1 and
300.  Also here: the C header declares apz_conv15h_fwd and _native.HIP_SYMBOLS lists it."""
import os
import re

import numpy as np
import pytest

import generic_nets as gn
import trained_nets as tn

# (n, C_in, C_out) of the operator cases of tests/test_gpu_conv15h.py (the case with more items than the grid: 64 -> 256)
OP_SHAPES = [(1, 64, 16), (3, 128, 48), (2, 192, 16), (3, 256, 48), (2, 64, 256)]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def op_tol(want):
    return 2e-5 * float(np.abs(want).max()) + 1e-6


def op_case(n, cin, cout, magnitude=1.0, seed=0):
    """Inputs of tests/test_gpu_conv15h.py: randn with about half the values passed through ReLU; weights randn / sqrt(9 C_in)."""
    rs = np.random.RandomState(1000 * cin + cout + n + seed)
    x = rs.randn(n, cin, 15, 15)
    relu = rs.rand(n, cin, 15, 15) < 0.5
    x = np.where(relu, np.maximum(x, 0), x) * magnitude
    w = rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)
    b = rs.randn(cout)
    return x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)


def conv64(x, w, b):
    import torch
    y = torch.nn.functional.conv2d(torch.tensor(np.asarray(x, np.float64)), torch.tensor(np.asarray(w, np.float64)),
                                   torch.tensor(np.asarray(b, np.float64)), padding=1)
    return y.numpy()


def split16(v):
    """float64 array (float32 values for activations) -> (hi, lo) as float64: fp16 roundings to nearest even, the remainder
    formed exactly (csrc/wino_f16x2.h f16x2_split: in double on the host, by v_fma_mix on the device)"""
    with np.errstate(over="ignore"):
        hi = np.asarray(v, np.float32).astype(np.float16).astype(np.float64)
        lo = (np.asarray(v, np.float64) - hi).astype(np.float32).astype(np.float16).astype(np.float64)
    return hi, lo


def channel_scale(w):
    """f16x2_scale_for: the power of two that puts max |w| of an output channel into [2^13, 2^14) (a zero channel: 1)"""
    m = np.abs(w).reshape(len(w), -1).max(axis=1)
    _, e = np.frexp(m)
    return np.where(m > 0, np.ldexp(1.0, np.clip(14 - e, -100, 100)), 1.0)


def emulate_split(x, w, shift):
    """x float32 activations, w float64 folded weights [C_out][C_in][3][3], shift float64 [C_out] -> the float64 value of
    sum over the four term products / S + shift"""
    S = channel_scale(w)
    whi, wlo = split16(np.asarray(w, np.float64) * S[:, None, None, None])
    xhi, xlo = split16(np.asarray(x, np.float32))
    zero = np.zeros(len(w))
    acc = conv64(xlo, wlo, zero) + conv64(xlo, whi, zero)
    acc = acc + conv64(xhi, wlo, zero) + conv64(xhi, whi, zero)
    return acc / S[None, :, None, None] + np.asarray(shift, np.float64)[None, :, None, None]


@pytest.mark.parametrize("magnitude", [1.0, 300.0, 1e-3], ids=["order_1", "order_300", "order_1e-3"])
@pytest.mark.parametrize("n,cin,cout", OP_SHAPES, ids=["%dx%dto%d" % s for s in OP_SHAPES])
def test_split_representation_meets_a_quarter_of_the_operator_bar(n, cin, cout, magnitude):
    import torch
    x, w, b = op_case(n, cin, cout, magnitude)
    want = conv64(x, w, b)
    tol = op_tol(want)
    rep = float(np.abs(emulate_split(x, w.astype(np.float64), b.astype(np.float64)) - want).max()) / tol
    print("split representation: %.4f of tol" % rep)
    assert rep <= 0.25, rep
    if magnitude >= 1.0:
        f32 = torch.nn.functional.conv2d(torch.tensor(x), torch.tensor(w), torch.tensor(b), padding=1).numpy()
        acc = float(np.abs(f32.astype(np.float64) - want).max()) / tol
        print("plain float32 accumulation: %.4f of tol" % acc)
        assert acc <= 0.25, acc


def test_split_range_ends_where_the_header_says():
    """65 504 is the largest finite fp16: an input beyond it has no split (hi = inf, lo = -inf -> NaN sums, the kernel's word)."""
    hi, lo = split16(np.array([65504.0, 1.0e5], np.float32))
    assert np.isfinite(hi[0]) and np.isfinite(lo[0]) and hi[0] + lo[0] == 65504.0
    assert not np.isfinite(hi[1])


@pytest.mark.parametrize("kind,side,blocks,nf", gn.GEN, ids=gn.GEN_IDS)
def test_split_representation_meets_a_quarter_of_the_layer_bars(kind, side, blocks, nf):
    """Layer 1 (the first layer conv15h_kernel takes: 64 -> 64, 64 -> 64 and 256 -> 256) of the three nets on 5 boards, its input
    the float32 rounding of the oracle's layer 0."""
    prm = gn.params(kind, side, blocks, nf)
    _, planes = gn.positions(5, side)
    ref = tn.Reference(prm, planes, kind, blocks, detail=[1])
    ci, co, resid = gn.layer_channels(kind, blocks, nf)[1]
    assert ci % 64 == 0 and co % 16 == 0 and not resid
    conv, bn, fix = tn.layer_names(kind, blocks)[1]
    w, shift = tn.folded(prm, conv, bn, fix)
    x = ref.layers[0].astype(np.float32)
    got = np.maximum(emulate_split(x, w, shift), 0)
    rec, bad = ref.check_layer(1, got)
    print(gn.gen_id(kind, side, blocks, nf), "%.4f of the layer bar, %.4f of the channel bars" % (rec["err_over_bar"], rec["chan_err_over_bar"]))
    assert not bad, bad
    assert rec["err_over_bar"] <= 0.25 and rec["chan_err_over_bar"] <= 0.25, rec


def test_operator_entry_is_declared_and_bound():
    from alphapig_amd import _native
    header = open(os.path.join(REPO, "include", "alphapig_hip.h")).read()
    assert re.search(r"\bint\s+apz_conv15h_fwd\s*\(", header)
    assert "apz_conv15h_fwd" in _native.HIP_SYMBOLS
