"""HipTrainer(trunk_arith="f16x2"): the training step's trunk forward (with the BatchNorm statistics in the epilogue) and
data gradient (with a power-of-two input scale chosen on the device) on trunk15_wino3h16_kernel -- the operators against
float64, the trainer against float64 autograd and against the exact "f32" trainer, and the step that an overflow repeats
on the exact kernels."""
import numpy as np
import pytest

from test_gpu_train import _compare_grads, _hip_masks, _problem

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional


def _rows16(t):
    return F.pad(t, (0, 1)).contiguous()


def _layer(seed, scale_w=1 / 34):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(128, 128, 3, 3, generator=g) * scale_w).cuda()
    b = torch.randn(128, generator=g).cuda()
    return g, w, b


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _pack(w, b=None):
    from alphapig_amd import hipconv
    u, bb = hipconv.wino3h_pack_many(w[None].contiguous(), None if b is None else b[None].contiguous())
    return u, bb


@pytest.mark.parametrize("n", [13, 70, 512])
def test_forward_with_statistics(n):
    """apz_wino3h_conv_stats: y against float64 at the f16x2 accuracy class, the per-(channel, board) sums against float64
    sums of the kernel's own y, bn_fwd(stats=...) against bn_fwd's own statistics pass, and bits independent of the board's
    place in the batch and of the launch shape."""
    from alphapig_amd import hipconv
    g, w, b = _layer(300 + n)
    x = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
    be = (torch.randn(128, generator=g) * 0.2).cuda()
    u, bb = _pack(w, b)
    flag = _flag()
    y, st = hipconv.conv3x3_fwd_stats_f16x2(x, u[0, 0], bb[0, 0], flag)
    y32 = hipconv.conv3x3_fwd(x, w, b, hipconv.ROWS16)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert float(y[..., 15].abs().max()) == 0.0                       # the pad column
    y64 = F.conv2d(x[..., :15].double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
    scale = float(y64.abs().max())
    e16 = float((y[..., :15].double().cpu() - y64).abs().max()) / scale
    e32 = float((y32[..., :15].double().cpu() - y64).abs().max()) / scale
    # the f16x2 class: 22 bits per operand instead of 24 -- within a few times the exact kernel's own error
    assert e16 < max(4 * e32, 1e-5), (e16, e32)
    yy = y[..., :15].double()
    s1, s2 = yy.sum(dim=(2, 3)).t(), (yy * yy).sum(dim=(2, 3)).t()
    assert float((st[..., 0] - s1).abs().max()) < 1e-5 * float(yy.abs().sum(dim=(2, 3)).max())
    assert float((st[..., 1] - s2).abs().max()) < 1e-5 * float(s2.max())
    a0, m0, i0 = hipconv.bn_fwd(y, None, be, None, None, None, True, hipconv.ROWS16, 0.1, 1e-3)
    a1, m1, i1 = hipconv.bn_fwd(y, None, be, None, None, None, True, hipconv.ROWS16, 0.1, 1e-3, stats=st)
    torch.cuda.synchronize()
    assert float((m0 - m1).abs().max()) < 1e-6 * float(m0.abs().max()) + 1e-7
    assert float(((i0 - i1) / i0).abs().max()) < 1e-5
    assert float((a0 - a1).abs().max()) < 1e-4 * float(a0.abs().max())
    # bits: a permuted batch, the last 13 boards alone (another launch shape), a second run
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    yp, stp = hipconv.conv3x3_fwd_stats_f16x2(x[perm].contiguous(), u[0, 0], bb[0, 0], flag)
    ys, sts = hipconv.conv3x3_fwd_stats_f16x2(x[n - 13:].contiguous(), u[0, 0], bb[0, 0], flag)
    y2, st2 = hipconv.conv3x3_fwd_stats_f16x2(x, u[0, 0], bb[0, 0], flag)
    torch.cuda.synchronize()
    assert torch.equal(yp, y[perm]) and torch.equal(stp, st[:, perm])
    assert torch.equal(ys, y[n - 13:]) and torch.equal(sts, st[:, n - 13:])
    assert torch.equal(y2, y) and torch.equal(st2, st)
    assert int(flag.item()) == 0


def _dgrad_errors(dy, w, add=None, dymax=None):
    """-> (f16x2 error, exact-kernel error, flag) of dx = conv_input(dy, w) (+ add), relative to max |dx64|"""
    from alphapig_amd import hipconv
    u, bb = _pack(w)
    flag = _flag()
    if dymax is None:
        dymax = dy.abs().amax(dim=(0, 2, 3)).reshape(1, 128).contiguous()   # what bn_bwd's dxmax holds: partial maxima
    dx = hipconv.conv3x3_dgrad_f16x2(dy, u[0, 1], bb[0, 1], dymax, flag, add=add)
    dx32 = hipconv.conv3x3_dgrad(dy, w, hipconv.ROWS16, add=add)
    torch.cuda.synchronize()
    dx64 = F.conv_transpose2d(dy[..., :15].double().cpu(), w.double().cpu(), padding=1)
    if add is not None:
        dx64 = dx64 + add[..., :15].double().cpu()
    scale = float(dx64.abs().max())
    assert float(dx[..., 15].abs().max()) == 0.0
    e16 = float((dx[..., :15].double().cpu() - dx64).abs().max()) / scale
    e32 = float((dx32[..., :15].double().cpu() - dx64).abs().max()) / scale
    return e16, e32, int(flag.item())


def test_data_gradient_across_magnitudes():
    """One dy pattern at max |dy| of 1, 1e-3, 1e-6, 1e-9 and 3e4: the error relative to the largest float64 result stays
    at the level of the scale-1 row and of the exact kernel's own error on the same input (bound: twice the larger of the
    two), with no overflow.  Without the scale (a maximum that gives a = 0) the 1e-6 row is off by orders of magnitude:
    its lo terms are subnormal fp16."""
    g, w, _ = _layer(41)
    base = _rows16(torch.randn(64, 128, 15, 15, generator=g)).cuda()
    base = base / float(base.abs().max())
    e1, e32_1, f1 = _dgrad_errors(base, w)
    assert f1 == 0
    for s in (1e-3, 1e-6, 1e-9, 3e4):
        e16, e32, f = _dgrad_errors((base * s).contiguous(), w)
        assert f == 0, s
        assert e16 <= 2 * max(e1, e32), (s, e16, e1, e32)
    # a = 0 (max |dy| claimed in [2^7, 2^8)): the unscaled kernel on the 1e-6 row
    dy = (base * 1e-6).contiguous()
    wrong = torch.full((1, 128), 200.0, device="cuda")
    e_unscaled, _, _ = _dgrad_errors(dy, w, dymax=wrong)
    assert e_unscaled > 20 * 2 * max(e1, e32_1), e_unscaled


@pytest.mark.parametrize("n", [13, 70])
def test_data_gradient_with_the_skip_gradient(n):
    """add (the skip gradient) lands on the result, odd batches included; small gradients as a mean loss hands back."""
    g, w, _ = _layer(50 + n)
    dy = (_rows16(torch.randn(n, 128, 15, 15, generator=g)) * 3e-6).cuda()
    add = (_rows16(torch.randn(n, 128, 15, 15, generator=g)) * 1e-5).cuda()
    e16, e32, f = _dgrad_errors(dy, w, add=add)
    e16n, e32n, _ = _dgrad_errors(dy, w)
    assert f == 0
    assert e16 <= 2 * max(e16n, e32), (e16, e16n, e32)
    assert e16n <= 2 * max(e32n, 4e-6), (e16n, e32n)


def test_bn_bwd_leaves_the_maxima():
    """apz_bn_bwd_max: the same dx as apz_bn_bwd, and per (split, channel) a max |dx| whose maximum is max |dx|."""
    from alphapig_amd import hipconv
    n = 70
    g = torch.Generator().manual_seed(7)
    x = _rows16(torch.randn(n, 128, 15, 15, generator=g)).cuda()
    dy = (_rows16(torch.randn(n, 128, 15, 15, generator=g)) * 1e-4).cuda()
    ga = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
    be = torch.zeros(128).cuda()
    y, m, i, k = hipconv.bn_fwd(x, ga, be, None, None, None, True, hipconv.ROWS16, 0.1, 1e-3, want_mask=True)
    dmax = torch.empty((hipconv.bn_bwd_splits(x, hipconv.ROWS16), 128), device="cuda")
    d0 = hipconv.bn_bwd(dy, x, None, ga, m, i, True, False, hipconv.ROWS16, mask=k)
    d1 = hipconv.bn_bwd(dy, x, None, ga, m, i, True, False, hipconv.ROWS16, mask=k, dxmax=dmax)
    torch.cuda.synchronize()
    assert torch.equal(d0[0], d1[0])
    per_channel = d1[0].abs().amax(dim=(0, 2, 3))
    assert torch.equal(dmax.amax(dim=0), per_channel)


@pytest.mark.parametrize("n,blocks", [(24, 2), (70, 1), (256, 1)])
def test_f16x2_trainer_gradients_match_float64_autograd(n, blocks):
    """test_gpu_train.py's float64 autograd check with the trunk on the f16x2 kernel: the same bars (loss / entropy 2e-5,
    gradients 1e-4 of each tensor's scale, moving statistics, ReLU flips); 256 boards: the small gradients of a mean loss."""
    from alphapig_amd.train import HipTrainer
    from torch_trainer import TorchTrainer
    prm, states, pis, zs = _problem("resnet", 15, n, blocks, seed=15 + n)
    tr = HipTrainer(prm, "resnet", n_blocks=blocks, batch_size=n, dropout=0.5, seed=5, trunk_arith="f16x2")
    loss3 = tr.loss_and_grads(states, pis, zs, keep_tape=True).cpu().numpy().astype(np.float64)
    assert tr.trunk_overflows == 0
    got = tr.get_grads()
    masks = {k: v.cpu() for k, v in tr.relu_masks().items()}
    ref = TorchTrainer(prm, "resnet", n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
                       mask_fn=_hip_masks(5), relu_masks=masks)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    loss, ent = ref.loss(t64(states), t64(pis), t64(zs), train=True)
    loss.backward()
    assert abs(loss3[0] + loss3[1] - float(loss)) < 2e-5 * (1 + abs(float(loss)))
    assert abs(loss3[2] - float(ent)) < 2e-5 * (1 + abs(float(ent)))
    assert set(got) == set(ref.train_names)
    _compare_grads(got, ref.grads(), 1e-4)
    plain = TorchTrainer(prm, "resnet", n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
                         mask_fn=_hip_masks(5))
    seen = {}
    plain._relu = lambda x, name: seen.setdefault(name, torch.relu(x))
    plain.loss(t64(states), t64(pis), t64(zs), train=True)
    for name, m in masks.items():
        flips = int(((seen[name] > 0) != m).sum())
        assert flips <= 2e-5 * m.numel() + 3, (name, flips)
    new, new_ref = tr.get_params(), ref.get_params()
    for k in tr.stat_names:
        np.testing.assert_allclose(new[k], new_ref[k], rtol=2e-4, atol=2e-5, err_msg=k)
    tr.close()


def test_f16x2_steps_match_the_comparator_and_the_f32_trainer():
    """Three optimiser steps on the f16x2 trunk against the PyTorch comparator (float32 on the GPU, the same dropout masks
    and, per step, the ReLU decisions of the f16x2 forward): test_trainer_steps_match_the_comparator's bars, losses and
    parameters.  Against the f32 HipTrainer from the same state: the same loss bar and Adam's step bound (2 lr per step)
    -- the element count bar needs shared ReLU decisions: a handful of activations within rounding distance of zero land
    on different sides in the two arithmetics and move whole gradient rows, which Adam's first, sign-like steps turn
    into full-size differences."""
    from alphapig_amd.train import HipTrainer
    from torch_trainer import TorchTrainer
    prm, states, pis, zs = _problem("resnet", 15, 24, 2, seed=1)
    fast = HipTrainer(prm, "resnet", n_blocks=2, batch_size=24, dropout=0.5, seed=3, trunk_arith="f16x2")
    cmp_ = TorchTrainer(prm, "resnet", n_blocks=2, batch_size=24, device="cuda", dropout=0.5, mask_fn=_hip_masks(3))
    got_l, cmp_l = [], []
    for _ in range(3):
        got_l.append(fast.train_step(states, pis, zs, 1e-3, keep_tape=True))
        cmp_.relu_masks = fast.relu_masks()
        cmp_l.append(cmp_.train_step(states, pis, zs, 1e-3))
    np.testing.assert_allclose(got_l, cmp_l, rtol=3e-4)
    assert fast.trunk_overflows == 0
    keys = ("convA1_weight", "convB2_weight", "bnA1_gamma", "bnB2_beta", "res_conv1_weight", "bnA1_moving_var",
            "bnB2_moving_mean", "fc_3_1_1_weight", "fc_3_2_1_weight", "conv3_1_1_weight", "conv3_2_1_beta")
    a, b = fast.get_params(), cmp_.get_params()
    for k in keys:
        d = np.abs(a[k] - b[k])
        assert int((d > 2e-4).sum()) <= max(8, 0.01 * d.size), k
        assert float(d.max()) < 2 * 1e-3 * 3 + 2e-4, k
    ref = HipTrainer(prm, "resnet", n_blocks=2, batch_size=24, dropout=0.5, seed=3)
    ref_l = [ref.train_step(states, pis, zs, 1e-3) for _ in range(3)]
    np.testing.assert_allclose(got_l, ref_l, rtol=3e-4)
    r = ref.get_params()
    for k in keys:
        assert float(np.abs(a[k] - r[k]).max()) < 2 * 1e-3 * 3 + 2e-4, k
    fast.close()
    ref.close()


@pytest.mark.parametrize("n,blocks", [(13, 2), (70, 3)])
def test_f16x2_steps_are_the_same_bits_on_every_run(n, blocks):
    from alphapig_amd.train import HipTrainer
    prm, states, pis, zs = _problem("resnet", 15, n, blocks, seed=9)
    runs = []
    for _ in range(2):
        tr = HipTrainer(prm, "resnet", n_blocks=blocks, batch_size=n, dropout=0.5, seed=5, trunk_arith="f16x2")
        losses = [tr.train_step(states, pis, zs, 2e-3) for _ in range(3)]
        runs.append((losses, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()},
                     {k: v.cpu().numpy() for k, v in tr.v.items()}))
        tr.close()
    assert runs[0][0] == runs[1][0]
    for i in (1, 2, 3):
        for k in runs[0][i]:
            np.testing.assert_array_equal(runs[0][i][k], runs[1][i][k], err_msg=k)


def _state(tr):
    return (tr.t, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()}, {k: v.cpu().numpy() for k, v in tr.v.items()})


def _assert_same_state(a, b):
    assert a[0] == b[0]
    for i in (1, 2, 3):
        assert set(a[i]) == set(b[i])
        for k in a[i]:
            np.testing.assert_array_equal(a[i][k], b[i][k], err_msg=k)


def test_an_overflowed_step_is_the_f32_step():
    """bnA1_gamma of one channel at 5e3: the next convolution's transformed input leaves the fp16 range, the step is taken
    again on the exact kernels -- and ends with the f32 trainer's parameters, moments, t, moving statistics, loss and
    entropy, bit for bit.  Without the outlier no step repeats, and the parameters differ from the f32 trainer's."""
    from alphapig_amd.train import HipTrainer
    prm, states, pis, zs = _problem("resnet", 15, 40, 2, seed=21)
    hot = dict(prm)
    hot["bnA1_gamma"] = np.array(prm["bnA1_gamma"], dtype=np.float32).copy()
    hot["bnA1_gamma"][3] = 5e3
    fast = HipTrainer(hot, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2, trunk_arith="f16x2")
    ref = HipTrainer(hot, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2)
    lf = fast.train_step(states, pis, zs, 1e-3)
    lr = ref.train_step(states, pis, zs, 1e-3)
    assert fast.trunk_overflows == 1
    assert lf == lr
    _assert_same_state(_state(fast), _state(ref))
    fast.close()
    ref.close()
    fast = HipTrainer(prm, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2, trunk_arith="f16x2")
    ref = HipTrainer(prm, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2)
    fast.train_step(states, pis, zs, 1e-3)
    ref.train_step(states, pis, zs, 1e-3)
    assert fast.trunk_overflows == 0
    a, b = fast.get_params(), ref.get_params()
    assert any(not np.array_equal(a[k], b[k]) for k in ("convA1_weight", "convB2_weight", "bnA1_moving_mean"))
    fast.close()
    ref.close()


def test_trunk_arith_validation():
    from alphapig_amd.train import HipTrainer
    for kind, side, blocks in (("resnet", 8, 2), ("simple", 8, 0)):
        prm, _, _, _ = _problem(kind, side, 4, blocks, seed=3)
        with pytest.raises(ValueError):
            HipTrainer(prm, kind, n_blocks=blocks, batch_size=4, trunk_arith="f16x2")
    prm, states, pis, zs = _problem("resnet", 15, 13, 1, seed=3)
    with pytest.raises(ValueError):
        HipTrainer(prm, "resnet", n_blocks=1, batch_size=13, trunk_arith="bf16")
    a = HipTrainer(prm, "resnet", n_blocks=1, batch_size=13, seed=4)
    b = HipTrainer(prm, "resnet", n_blocks=1, batch_size=13, seed=4, trunk_arith="f32")
    for _ in range(2):
        assert a.train_step(states, pis, zs, 1e-3) == b.train_step(states, pis, zs, 1e-3)
    _assert_same_state(_state(a), _state(b))
    a.close()
    b.close()


def test_policy_update_on_the_f16x2_trainer():
    from alphapig_amd.train import HipTrainer, policy_update
    prm, states, pis, zs = _problem("resnet", 15, 64, 1, seed=4)
    tr = HipTrainer(prm, "resnet", n_blocks=1, batch_size=64, dropout=0.5, seed=1, trunk_arith="f16x2")
    batch = [(states[i], pis[i], zs[i]) for i in range(64)]
    mult, first = 1.0, None
    for _ in range(4):
        loss, ent, kl, mult = policy_update(tr, batch, learn_rate=5e-3, lr_multiplier=mult, epochs=3, kl_targ=0.02)
        first = loss if first is None else first
        assert np.isfinite(loss) and np.isfinite(ent) and np.isfinite(kl) and kl >= -1e-6
    assert loss < first
    assert 0.05 / 1.5 <= mult <= 20 * 1.5
    assert tr.trunk_overflows == 0
    tr.close()
