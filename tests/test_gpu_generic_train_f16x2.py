"""HipTrainer(trunk_arith="f16x2") on the generic 15x15 nets (rows16 False: the simple net, the residual nets of 64 and 256
filters): every 3x3 layer with C_in a multiple of 64 runs its forward and its data gradient on conv15h_kernel
(csrc/conv15_split.h) -- the operators against float64, the packed forward against the per-call operator, the dense bn_bwd
with its maxima, the trainer against float64 autograd and against the exact "f32" trainer, the step that an overflow repeats
on the exact kernels, and the switches that must go on working with it.  On the parent of this file's commit the constructor
refuses every one of these nets, so the trainer tests fail there."""
import time

import numpy as np
import pytest

import generic_nets as gn
from test_gpu_generic_train import GRAD_BATCH, _problem

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

TABLE = gn.Table("r32_generic_train_f16x2")
# (n, C of dy, C of dx): one sub-chunk per wave; ...; four sub-chunks and both weight buffers; 528 items for a grid of 2 x 256
DGRAD_SHAPES = [(1, 64, 64), (3, 128, 64), (2, 256, 128), (3, 256, 256), (33, 64, 256)]
MAGNITUDES = (1e-3, 1e-6, 1e-9, 3e4)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _layer(c_out, c_in, seed):
    """-> (generator, weight [c_out][c_in][3][3], bias [c_out]) on the device"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(c_out, c_in, 3, 3, generator=g) / (9.0 * c_out) ** 0.5).cuda()
    b = torch.randn(c_out, generator=g).cuda()
    return g, w, b


def _pack(w, b=None, flag=None):
    from alphapig_amd import hipconv
    return hipconv.conv15h_pack_many([(w, b)], flag=flag)[0]


def _dgrad_errors(dy, w, packed, add=None, dymax=None):
    """-> (f16x2 error, exact-kernel error, flag, dx) of dx = conv_input(dy, w) (+ add), errors relative to max |dx64|"""
    from alphapig_amd import hipconv
    flag = _flag()
    if dymax is None:
        dymax = dy.abs().amax(dim=(0, 2, 3)).reshape(1, -1).contiguous()   # what bn_bwd's dxmax holds: partial maxima
    dx = hipconv.conv3x3_dgrad_f16x2_dense(dy, packed[1], dymax, flag, add=add)
    dx32 = hipconv.conv3x3_dgrad(dy, w, hipconv.DENSE, add=add)
    torch.cuda.synchronize()
    dx64 = F.conv_transpose2d(dy.double().cpu(), w.double().cpu(), padding=1)
    if add is not None:
        dx64 = dx64 + add.double().cpu()
    scale = float(dx64.abs().max())
    e16 = float((dx.double().cpu() - dx64).abs().max()) / scale
    e32 = float((dx32.double().cpu() - dx64).abs().max()) / scale
    return e16, e32, int(flag.item()), dx


@pytest.mark.parametrize("n,c_dy,c_dx", DGRAD_SHAPES, ids=["%dx%dto%d" % s for s in DGRAD_SHAPES])
def test_data_gradient_against_float64_across_magnitudes(n, c_dy, c_dx):
    """The bar of test_gpu_train_f16x2.py::test_data_gradient_across_magnitudes: one dy pattern at max |dy| of 1, 1e-3, 1e-6,
    1e-9 and 3e4 -- the error relative to max |dx64| is at most twice the larger of the scale-1 row and the fp32 kernel's
    error on the same input, flag 0.  A wrong dymax (200: a = 0) on the 1e-6 row is more than 20 times worse; `add` lands on
    the result; zero dy gives exactly `add`; a +inf dymax sets the flag."""
    from alphapig_amd import hipconv
    g, w, _ = _layer(c_dy, c_dx, 4100 + c_dy + c_dx + n)
    packed = _pack(w)
    base = torch.randn(n, c_dy, 15, 15, generator=g).cuda()
    base = (base / float(base.abs().max())).contiguous()
    e1, e32_1, f1, _ = _dgrad_errors(base, w, packed)
    print("scale 1: f16x2 %.3e, fp32 %.3e" % (e1, e32_1))
    assert f1 == 0
    row = {"1": e1 / (2 * max(e1, e32_1))}
    for s in MAGNITUDES:
        e16, e32, f, _ = _dgrad_errors((base * s).contiguous(), w, packed)
        print("scale %g: f16x2 %.3e, fp32 %.3e, over the bar %.4f" % (s, e16, e32, e16 / (2 * max(e1, e32))))
        row["%g" % s] = e16 / (2 * max(e1, e32))
        assert f == 0, s
        assert e16 <= 2 * max(e1, e32), (s, e16, e1, e32)
    dy = (base * 1e-6).contiguous()
    wrong = torch.full((1, c_dy), 200.0, device="cuda")
    e_unscaled, _, _, _ = _dgrad_errors(dy, w, packed, dymax=wrong)
    print("1e-6 with a = 0: %.3e" % e_unscaled)
    assert e_unscaled > 20 * 2 * max(e1, e32_1), e_unscaled
    # add, small gradients as a mean loss hands back
    add = (torch.randn(n, c_dx, 15, 15, generator=g) * 1e-5).cuda()
    dy = (base * 3e-6).contiguous()
    ea, e32a, fa, _ = _dgrad_errors(dy, w, packed, add=add)
    en, e32n, _, _ = _dgrad_errors(dy, w, packed)
    assert fa == 0
    assert ea <= 2 * max(en, e32a), (ea, en, e32a)
    # zero dy: exactly add, or +0
    zero = torch.zeros_like(base)
    zmax = torch.zeros((3, c_dy), device="cuda")
    flag = _flag()
    dx_add = hipconv.conv3x3_dgrad_f16x2_dense(zero, packed[1], zmax, flag, add=add)
    dx_0 = hipconv.conv3x3_dgrad_f16x2_dense(zero, packed[1], zmax, flag)
    torch.cuda.synchronize()
    assert torch.equal(dx_add, add)
    assert int(dx_0.view(torch.int32).abs().max()) == 0             # +0 everywhere, by its bits
    assert int(flag.item()) == 0
    # +inf among the maxima: no scale fits, the flag says so; a NaN entry is ignored
    nanmax = base.abs().amax(dim=(0, 2, 3)).reshape(1, -1).repeat(2, 1).contiguous()
    nanmax[1, 0] = float("nan")
    dx_nan = hipconv.conv3x3_dgrad_f16x2_dense(base, packed[1], nanmax, flag)
    dx_ref = hipconv.conv3x3_dgrad_f16x2_dense(base, packed[1], nanmax[:1].contiguous(), flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and torch.equal(dx_nan, dx_ref)
    nanmax[1, 0] = float("inf")
    hipconv.conv3x3_dgrad_f16x2_dense(base, packed[1], nanmax, flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    TABLE.add(test="data_gradient_against_float64", shape=[n, c_dy, c_dx], err_over_bar=row, e16_scale1=e1, e32_scale1=e32_1,
              unscaled_1e6=e_unscaled)


CELLS = [(0, 0), (0, 14), (14, 0), (14, 14), (0, 7), (14, 7), (7, 0), (7, 14)]      # corners, edge centres


def test_one_hot_probes_pin_the_flip_the_transposition_and_the_borders():
    """One nonzero dy cell per board (each corner, each edge centre), one nonzero weight tap: dx is nonzero exactly where
    float64 says, and equal to it there (one product: exact up to the split of a 22-bit operand)."""
    from alphapig_amd import hipconv
    co, ci = 37, 21                                # dy channel, dx channel
    dy = torch.zeros(len(CELLS), 64, 15, 15)
    for b, (y, x) in enumerate(CELLS):
        dy[b, co, y, x] = 1.5
    dy = dy.cuda()
    dymax = dy.abs().amax(dim=(0, 2, 3)).reshape(1, -1).contiguous()
    for tap in range(9):
        w = torch.zeros(64, 128, 3, 3)
        w[co, ci, tap // 3, tap % 3] = 0.3125
        w = w.cuda()
        flag = _flag()
        dx = hipconv.conv3x3_dgrad_f16x2_dense(dy, _pack(w)[1], dymax, flag)
        torch.cuda.synchronize()
        dx64 = F.conv_transpose2d(dy.double().cpu(), w.double().cpu(), padding=1)
        assert int(flag.item()) == 0
        assert torch.equal(dx.cpu() != 0, dx64 != 0), tap
        assert int((dx64 != 0).sum()) >= 3, tap                      # (a diagonal tap leaves the board from five of the eight cells)
        assert torch.equal(dx.cpu().double(), dx64), tap


@pytest.mark.parametrize("n,cin,cout", [(3, 128, 64), (2, 64, 256), (5, 256, 256)])
def test_packed_forward_is_the_per_call_operator_bit_for_bit(n, cin, cout):
    from alphapig_amd import hipconv
    g, w, b = _layer(cout, cin, 4300 + cin + cout)
    x = torch.randn(n, cin, 15, 15, generator=g).cuda()
    resid = torch.randn(n, cout, 15, 15, generator=g).cuda()
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    packed = _pack(w, b, flag=word)
    assert int(word.item()) == 0                                      # the pack launch zeroes the step's overflow word
    flag = _flag()
    for r in (None, resid):
        want = hipconv.conv3x3_fwd_f16x2_dense(x, w, b, resid=r, relu=False, flag=flag)
        got = hipconv.conv3x3_fwd_f16x2_dense_packed(x, packed[0], resid=r, flag=flag)
        torch.cuda.synchronize()
        assert torch.equal(got, want), r is None
    nob = hipconv.conv3x3_fwd_f16x2_dense_packed(x, _pack(w)[0], flag=flag)
    assert torch.equal(nob, hipconv.conv3x3_fwd_f16x2_dense(x, w, None, flag=flag))
    x[1, 5, 3, 3] = 1e5                                                # beyond 65 504: the word
    hipconv.conv3x3_fwd_f16x2_dense_packed(x, packed[0], flag=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1


def test_pack_many_packs_layers_of_different_shapes_in_one_launch():
    """Three layers of three shapes in one table: each equals its own single-layer pack, both orientations"""
    from alphapig_amd import hipconv
    layers = [_layer(64, 64, 1)[1:], _layer(256, 128, 2)[1:], _layer(128, 256, 3)[1:]]
    many = hipconv.conv15h_pack_many(layers)
    again = hipconv.conv15h_pack_many(layers, out=many)
    assert again[1][1][0].data_ptr() == many[1][1][0].data_ptr()
    for (w, b), got in zip(layers, many):
        one = _pack(w, b)
        for o in (0, 1):
            assert torch.equal(got[o][0].view(torch.int32), one[o][0].view(torch.int32))
            assert torch.equal(got[o][1], one[o][1])
        assert float(got[1][1][0].abs().max()) == 0.0               # the data gradient has no bias
    with pytest.raises(ValueError):
        hipconv.conv15h_pack_many([(torch.zeros(64, 9, 3, 3, device="cuda"), None)])


@pytest.mark.parametrize("n,c,relu", [(7, 64, True), (70, 256, False)])
def test_dense_bn_bwd_leaves_the_maxima(n, c, relu):
    """apz_bn_bwd_max on dense tensors: dx, dres, dgamma and dbeta of the call without dxmax, bit for bit, and per (split,
    channel) a max |dx| whose maximum over the splits is max |dx| of the channel."""
    from alphapig_amd import hipconv
    g = torch.Generator().manual_seed(7 + n)
    x = torch.randn(n, c, 15, 15, generator=g).cuda()
    dy = (torch.randn(n, c, 15, 15, generator=g) * 1e-4).cuda()
    ga = (1 + 0.1 * torch.randn(c, generator=g)).cuda()
    be = torch.zeros(c).cuda()
    y, m, i = hipconv.bn_fwd(x, ga, be, None, None, None, relu, hipconv.DENSE, 0.1, 1e-3)
    dmax = torch.full((hipconv.bn_bwd_splits(x, hipconv.DENSE), c), -1.0, device="cuda")
    d0 = hipconv.bn_bwd(dy, x, y, ga, m, i, relu, True, hipconv.DENSE)
    d1 = hipconv.bn_bwd(dy, x, y, ga, m, i, relu, True, hipconv.DENSE, dxmax=dmax)
    torch.cuda.synchronize()
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    assert torch.equal(dmax.amax(dim=0), d1[0].abs().amax(dim=(0, 2, 3)))
    assert float(dmax.min()) >= 0.0


# ---- the trainer ---------------------------------------------------------------------------------------------------------
def _trainer(cfg, prm, n, **kw):
    from alphapig_amd.train import HipTrainer
    kind, side, blocks, nf = cfg
    kw.setdefault("dropout", 0.5)
    tr = HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, **kw)
    assert tr.rows16 is False
    return tr


@pytest.mark.parametrize("cfg", gn.GEN, ids=gn.GEN_IDS)
def test_f16x2_trainer_gradients_match_float64_autograd_on_the_generic_nets(cfg):
    """tests/test_gpu_generic_train.py's float64 autograd check with the eligible layers on the f16x2 kernel, the same bars: loss
    and entropy 2e-5, gradients 1e-4 of each tensor's scale, at most 2e-5 * numel + 3 ReLU flips, statistics 2e-4 / 2e-5.  No
    overflow, and a trunk weight gradient whose bits differ from the f32 trainer's: the fast path ran."""
    from alphapig_amd.train import f16x2_dense_layers
    from torch_trainer import TorchTrainer
    from test_gpu_train import _compare_grads, _hip_masks
    kind, side, blocks, nf = cfg
    name = gn.gen_id(*cfg)
    n = GRAD_BATCH[name]
    t0 = time.time()
    prm, states, pis, zs = _problem(cfg, n, seed=side + n)
    tr = _trainer(cfg, prm, n, seed=5, trunk_arith="f16x2")
    loss3 = tr.loss_and_grads(states, pis, zs, keep_tape=True).cpu().numpy().astype(np.float64)
    assert tr.trunk_overflows == 0
    got = tr.get_grads()
    masks = {k: v.cpu() for k, v in tr.relu_masks().items()}
    ref = TorchTrainer(prm, kind, n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
                       mask_fn=_hip_masks(5), relu_masks=masks)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    loss, ent = ref.loss(t64(states), t64(pis), t64(zs), train=True)
    loss.backward()
    g64 = ref.grads()
    worst = {}
    for k, g in g64.items():                           # _compare_grads' figure, for the table
        scale = np.abs(g64[k[:-5] + "_weight"]).max() if k.endswith("_bias") and not k.startswith("fc_") else np.abs(g).max()
        worst[k] = float(np.abs(got[k].astype(np.float64) - g).max() / (scale + 1e-12) / 1e-4)
    loss64, ent64 = float(loss.detach()), float(ent.detach())
    loss_ratio = abs(loss3[0] + loss3[1] - loss64) / (2e-5 * (1 + abs(loss64)))
    print(name, "loss %.4f" % loss_ratio, "worst gradient %s %.4f" % max(worst.items(), key=lambda kv: kv[1]))
    assert abs(loss3[0] + loss3[1] - loss64) < 2e-5 * (1 + abs(loss64))
    assert abs(loss3[2] - ent64) < 2e-5 * (1 + abs(ent64))
    assert set(got) == set(ref.train_names)
    _compare_grads(got, g64, 1e-4)
    plain = TorchTrainer(prm, kind, n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
                         mask_fn=_hip_masks(5))
    seen = {}
    plain._relu = lambda x, name: seen.setdefault(name, torch.relu(x))
    plain.loss(t64(states), t64(pis), t64(zs), train=True)
    flips = {}
    for k, m in masks.items():
        flips[k] = int(((seen[k] > 0) != m).sum())
        assert flips[k] <= 2e-5 * m.numel() + 3, (k, flips[k])
    new, new_ref = tr.get_params(), ref.get_params()
    for k in tr.stat_names:
        np.testing.assert_allclose(new[k], new_ref[k], rtol=2e-4, atol=2e-5, err_msg=k)
    for k in tr.fixed_gamma_names:
        assert np.all(new[k] == 1.0), k
    tr.close()
    exact = _trainer(cfg, prm, n, seed=5)
    exact.loss_and_grads(states, pis, zs)
    g32 = exact.get_grads()
    exact.close()
    layers = f16x2_dense_layers(prm, kind, blocks)
    assert layers
    assert any(not np.array_equal(got[k + "_weight"], g32[k + "_weight"]) for k in layers)
    TABLE.add(test="trainer_gradients_match_float64_autograd", net=name, n=n, loss_err_over_bar=loss_ratio,
              grad_err_over_bar=worst, relu_flips=flips, seconds=round(time.time() - t0, 3))


def _state(tr):
    return (tr.t, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()}, {k: v.cpu().numpy() for k, v in tr.v.items()})


def _assert_same_state(a, b):
    assert a[0] == b[0]
    for i in (1, 2, 3):
        assert set(a[i]) == set(b[i])
        for k in a[i]:
            np.testing.assert_array_equal(a[i][k], b[i][k], err_msg=k)


def test_f16x2_steps_on_the_256_filter_net_are_the_same_bits_on_every_run():
    cfg = ("resnet", 15, 1, 256)
    prm, states, pis, zs = _problem(cfg, 13, seed=9)
    runs = []
    for _ in range(2):
        tr = _trainer(cfg, prm, 13, seed=5, trunk_arith="f16x2")
        losses = [tr.train_step(states, pis, zs, 2e-3) for _ in range(3)]
        assert tr.trunk_overflows == 0
        runs.append((losses,) + _state(tr))
        tr.close()
    assert np.isfinite(np.asarray(runs[0][0], np.float64)).all()
    assert runs[0][0] == runs[1][0]
    _assert_same_state(runs[0][1:], runs[1][1:])


@pytest.mark.parametrize("cfg", gn.GEN, ids=gn.GEN_IDS)
def test_an_overflowed_step_is_the_f32_step(cfg):
    """An outlier of 1e6 in bnA1_gamma[3] (the residual nets) or conv2_beta[3] (the simple net): the next layer's input leaves
    65 504, the step is taken again on the exact kernels and ends with the f32 trainer's losses, parameters, moments, t and
    moving statistics, bit for bit.  Without the outlier no step repeats."""
    kind, side, blocks, nf = cfg
    n = 8
    prm, states, pis, zs = _problem(cfg, n, seed=21)
    key = "bnA1_gamma" if kind == "resnet" else "conv2_beta"
    hot = dict(prm)
    hot[key] = np.array(prm[key], dtype=np.float32).copy()
    hot[key][3] = 1e6
    fast = _trainer(cfg, hot, n, seed=2, trunk_arith="f16x2")
    ref = _trainer(cfg, hot, n, seed=2)
    lf = fast.train_step(states, pis, zs, 1e-3)
    lr = ref.train_step(states, pis, zs, 1e-3)
    assert fast.trunk_overflows == 1
    assert lf == lr
    _assert_same_state(_state(fast), _state(ref))
    fast.close()
    ref.close()
    fast = _trainer(cfg, prm, n, seed=2, trunk_arith="f16x2")
    fast.train_step(states, pis, zs, 1e-3)
    assert fast.trunk_overflows == 0
    fast.close()


# ---- combinations, on resnet15x64 at n = 8 ---------------------------------------------------------------------------------
CFG64 = ("resnet", 15, 1, 64)


def test_guarded_and_averaged_steps():
    """step_guard=True: a step that stands has the unguarded step's bits; ema_decay=0.99: the raw weights are those of the
    trainer without it and the average moved"""
    prm, states, pis, zs = _problem(CFG64, 8, seed=31)
    plain = _trainer(CFG64, prm, 8, seed=4, trunk_arith="f16x2")
    want = plain.train_step(states, pis, zs, 1e-3)
    for kw in ({"step_guard": True}, {"ema_decay": 0.99}):
        tr = _trainer(CFG64, prm, 8, seed=4, trunk_arith="f16x2", **kw)
        assert tr.train_step(states, pis, zs, 1e-3) == want
        assert tr.trunk_overflows == 0
        _assert_same_state(_state(tr), _state(plain))
        if "step_guard" in kw:
            assert tr.skipped_steps == 0 and np.isfinite(tr.last_grad_norm) and tr.last_grad_norm > 0
        else:
            assert tr.ema_updates == 1
            ema, raw = tr.ema_params(), tr.get_params()
            assert any(not np.array_equal(ema[k], raw[k]) for k in ("convA1_weight", "convB1_weight"))
        tr.close()
    plain.close()


def test_legal_policy_step_follows_the_f32_trainer():
    """legal_policy=True: the loss over the empty cells, on both arithmetics -- the same loss to the bar the two trainers are
    held to elsewhere (rtol 3e-4), no overflow"""
    prm, states, pis, zs = _problem(CFG64, 8, seed=34)
    fast = _trainer(CFG64, prm, 8, seed=4, trunk_arith="f16x2", legal_policy=True)
    ref = _trainer(CFG64, prm, 8, seed=4, legal_policy=True)
    lf, lr = fast.train_step(states, pis, zs, 1e-3), ref.train_step(states, pis, zs, 1e-3)
    assert np.isfinite(np.asarray(lf, np.float64)).all()
    np.testing.assert_allclose(lf, lr, rtol=3e-4)
    assert fast.trunk_overflows == 0
    fast.close()
    ref.close()


def test_state_round_trip_and_an_identical_next_step():
    prm, states, pis, zs = _problem(CFG64, 8, seed=32)
    a = _trainer(CFG64, prm, 8, seed=4, trunk_arith="f16x2")
    a.train_step(states, pis, zs, 1e-3)
    st = a.state()
    assert st["meta"]["trunk_arith"] == "f16x2"
    b = _trainer(CFG64, prm, 8, seed=4, trunk_arith="f16x2")
    b.load_state(st)
    _assert_same_state(_state(a), _state(b))
    assert a.train_step(states, pis, zs, 1e-3) == b.train_step(states, pis, zs, 1e-3)
    _assert_same_state(_state(a), _state(b))
    a.close()
    b.close()


def test_sync_evaluator_equals_a_fresh_evaluator():
    from alphapig_amd.policy_value_net import PolicyValueNet
    kind, side, blocks, nf = CFG64
    prm, states, pis, zs = _problem(CFG64, 8, seed=33)
    _, planes = gn.positions(5, side)
    kw = dict(batch_size=8, n_blocks=blocks, n_filter=nf, net_kind=kind)
    net = PolicyValueNet(side, side, model_params=prm, **kw)
    tr = _trainer(CFG64, prm, 8, seed=3, trunk_arith="f16x2")
    assert np.isfinite(np.asarray(tr.train_step(states, pis, zs, 2e-3), np.float64)).all()
    tr.sync_evaluator(net)
    got = net.forward_with_logits(planes)
    fresh = PolicyValueNet(side, side, model_params=tr.get_params(), **kw)
    want = fresh.forward_with_logits(planes)
    for name, a, b in zip(("logits", "probs", "value_logit", "values"), got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=name)
    for x in (net, fresh):
        x.close()
    tr.close()


def test_policy_update_lowers_the_loss():
    """As test_gpu_train_f16x2.py::test_policy_update_on_the_f16x2_trainer"""
    from alphapig_amd.train import policy_update
    prm, states, pis, zs = _problem(CFG64, 8, seed=4)
    tr = _trainer(CFG64, prm, 8, seed=1, trunk_arith="f16x2")
    batch = [(states[i], pis[i], zs[i]) for i in range(8)]
    mult, first = 1.0, None
    for _ in range(4):
        loss, ent, kl, mult = policy_update(tr, batch, learn_rate=5e-3, lr_multiplier=mult, epochs=3, kl_targ=0.02)
        first = loss if first is None else first
        assert np.isfinite(loss) and np.isfinite(ent) and np.isfinite(kl) and kl >= -1e-6
    assert loss < first
    assert 0.05 / 1.5 <= mult <= 20 * 1.5
    assert tr.trunk_overflows == 0
    tr.close()
