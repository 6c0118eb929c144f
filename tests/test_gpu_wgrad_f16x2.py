"""The trunk's weight gradient on the fp16 matrix pipe (csrc/wgrad_wino3h.h, apz_wgrad_wino_f16x2,
hipconv.conv3x3_wgrad_f16x2): the operator against float64 autograd and against the exact kernel's own error across
gradient magnitudes, the device-chosen scale, the overflow word, bits.  (The kernel is slower than the exact one --
profiles/r08_wgrad_f16x2.md -- so no trainer option uses it and there is no trainer test.)"""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional


def _rows16(t):
    return F.pad(t, (0, 1)).contiguous()


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _dymax(dy):
    return dy.abs().amax(dim=(0, 2, 3)).reshape(1, 128).contiguous()      # what bn_bwd's dxmax holds: partial maxima


def _dw64(x, dy):
    """float64 autograd dw of conv2d(x, w, padding=1) for the output gradient dy (dense CPU tensors)"""
    w64 = torch.zeros(128, 128, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, padding=1).backward(dy.double())
    return w64.grad


def _inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, 128, 15, 15, generator=g))
    base = torch.randn(n, 128, 15, 15, generator=g)
    return x, base


SCALES = (1.0, 1e-5, 1e-9, 3e4)


@pytest.mark.parametrize("n", [1, 6, 64, 131, 513])
def test_weight_gradient_against_float64(n):
    """x = relu(randn), dy = randn * s for s in 1, 1e-5, 1e-9, 3e4: the project's bar for this tensor (1e-4 of max |dw64|),
    and within a few times the exact kernel's own error on the same data (the f16x2 class: 22 bits per operand instead of
    24); the overflow word stays clear in every row."""
    from alphapig_amd import hipconv
    x, base = _inputs(n, 7000 + n)
    xc = _rows16(x).cuda()
    for s in SCALES:
        dy = (base * s).float()
        dyc = _rows16(dy).cuda()
        flag = _flag()
        dw = hipconv.conv3x3_wgrad_f16x2(xc, dyc, _dymax(dyc), flag)
        dw32 = hipconv.conv3x3_wgrad(xc, dyc, hipconv.ROWS16)
        torch.cuda.synchronize()
        ref = _dw64(x, dy)
        scale = float(ref.abs().max())
        e16 = float((dw.double().cpu() - ref).abs().max())
        e32 = float((dw32.double().cpu() - ref).abs().max())
        print("n=%d s=%g: f16x2 %.3g, f32 %.3g of max |dw64|; flag %d" % (n, s, e16 / scale, e32 / scale, int(flag.item())))
        assert int(flag.item()) == 0, (n, s)
        assert e16 < 1e-4 * scale, (n, s, e16 / scale)
        assert e16 <= max(4 * e32, 1e-5 * scale), (n, s, e16 / scale, e32 / scale)


def test_the_scale_matters():
    """The s = 1e-5 row with a dymax that claims the maximum already sits in the window [2^6, 2^7), which forces a = 0:
    the lo terms of the transformed gradient are subnormal fp16 or lost, and the error is beyond ten times the bar."""
    from alphapig_amd import hipconv
    n = 64
    x, base = _inputs(n, 7000 + n)
    dy = (base * 1e-5).float()
    xc, dyc = _rows16(x).cuda(), _rows16(dy).cuda()
    flag = _flag()
    good = hipconv.conv3x3_wgrad_f16x2(xc, dyc, _dymax(dyc), flag)
    wrong = hipconv.conv3x3_wgrad_f16x2(xc, dyc, torch.full((1, 128), 100.0, device="cuda"), flag)
    torch.cuda.synchronize()
    ref = _dw64(x, dy)
    scale = float(ref.abs().max())
    e_good = float((good.double().cpu() - ref).abs().max()) / scale
    e_wrong = float((wrong.double().cpu() - ref).abs().max()) / scale
    print("scaled %.3g, unscaled %.3g of max |dw64|" % (e_good, e_wrong))
    assert e_good < 1e-4
    assert e_wrong > 10 * 1e-4, e_wrong


def test_overflow_word():
    from alphapig_amd import hipconv
    n = 6
    x, base = _inputs(n, 7100)
    xc, dyc = _rows16(x).cuda(), _rows16(base).cuda()
    # one activation of 2e3: the transformed input leaves the range the fp16 terms are guaranteed for
    hot = xc.clone()
    hot[3, 17, 6, 6] = 2e3
    flag = _flag()
    hipconv.conv3x3_wgrad_f16x2(hot, dyc, _dymax(dyc), flag)
    torch.cuda.synchronize()
    assert int(flag.item()) != 0
    # an all-zero gradient with zero maxima: a = 0, an exact zero result, no flag
    flag = _flag()
    zero = torch.zeros_like(dyc)
    dw = hipconv.conv3x3_wgrad_f16x2(xc, zero, torch.zeros((1, 128), device="cuda"), flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert float(dw.abs().max()) == 0.0
    # a large gradient: the scale keeps the transformed gradient inside fp16
    flag = _flag()
    big = (dyc * 3e4).contiguous()
    dw = hipconv.conv3x3_wgrad_f16x2(xc, big, _dymax(big), flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert bool(torch.isfinite(dw).all())


@pytest.mark.parametrize("n", [6, 513])
def test_same_bits_on_every_run(n):
    from alphapig_amd import hipconv
    x, base = _inputs(n, 7200 + n)
    xc, dyc = _rows16(x).cuda(), _rows16((base * 1e-4).float()).cuda()
    flag = _flag()
    a = hipconv.conv3x3_wgrad_f16x2(xc, dyc, _dymax(dyc), flag)
    b = hipconv.conv3x3_wgrad_f16x2(xc, dyc, _dymax(dyc), flag)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert int(flag.item()) == 0


def test_operator_validation():
    from alphapig_amd import hipconv
    flag = _flag()
    dm = torch.ones((1, 128), device="cuda")
    dense = torch.zeros(2, 128, 15, 15, device="cuda")
    with pytest.raises(ValueError):
        hipconv.conv3x3_wgrad_f16x2(dense, dense, dm, flag)
    x = torch.zeros(2, 128, 15, 16, device="cuda")
    with pytest.raises(ValueError):
        hipconv.conv3x3_wgrad_f16x2(x, torch.zeros(2, 64, 15, 16, device="cuda"), dm, flag)


def test_evaluator_engine_serves_the_weight_gradient_in_both_orders():
    """One engine runs the scaled f16x2 trunk kernels (a 33-board forward with activation exponents: the batched route) and
    apz_wgrad_wino_f16x2, in both orders: each kernel gets its own dynamic-LDS attribute whichever came first.  dw carries
    the bits of hipconv's engine (the decomposition depends on n and the CU count only), the forward those of a net that
    never ran a training operator.  The attribute is process-wide, so the case discriminates only where it is the first in
    its process to touch these kernels."""
    import ctypes as C
    import numpy as np
    from alphapig_amd import hipconv, weights
    from alphapig_amd.policy_value_net import PolicyValueNet
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=3, style="bench")
    planes = (np.random.RandomState(5).rand(33, 9, 15, 15) < 0.3).astype(np.float32)
    x, base = _inputs(6, 7300)
    xc, dyc = _rows16(x).cuda(), _rows16(base).cuda()
    dymax = _dymax(dyc)

    def make():
        net = PolicyValueNet(15, 15, batch_size=64, n_blocks=1, n_filter=128, model_params=prm, trunk_arith="f16x2")
        net.set_trunk_act_exponents([1, 1])
        return net

    def wgrad_on(net):
        dw, flag = torch.empty(128, 128, 3, 3, device="cuda"), _flag()
        rc = net.L.apz_wgrad_wino_f16x2(net._h, xc.data_ptr(), dyc.data_ptr(), dw.data_ptr(), 6, dymax.data_ptr(),
                                        int(dymax.numel()), flag.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, net.L.apz_last_error().decode()
        assert int(flag.item()) == 0
        return dw

    a, b, plain = make(), make(), make()
    fwd_a = a.forward_planes(planes)
    dw_a = wgrad_on(a)
    dw_b = wgrad_on(b)
    fwd_b = b.forward_planes(planes)
    fwd = plain.forward_planes(planes)
    flag = _flag()
    dw = hipconv.conv3x3_wgrad_f16x2(xc, dyc, dymax, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    for net, got_dw, got_fwd in ((a, dw_a, fwd_a), (b, dw_b, fwd_b)):
        assert torch.equal(got_dw, dw)
        assert np.array_equal(got_fwd[0], fwd[0]) and np.array_equal(got_fwd[1], fwd[1])
        assert net.trunk_overflows() == 0
    assert plain.trunk_overflows() == 0
    for net in (a, b, plain):
        net.close()
