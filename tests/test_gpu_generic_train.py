"""The trainer on the generic convolution route: the three nets of tests/generic_nets.py (the simple net and the one-block residual
nets of 64 and 256 filters, 15x15) train on dense tensors with the direct kernels (HipTrainer.rows16 False: conv3x3_mfma_kernel
forward and data gradient, the direct weight-gradient kernel, dense BatchNorm and heads).  Procedures and bars are those of
tests/test_gpu_train.py, which runs them on the 128-filter residual net at 15x15 and on the 8x8 nets."""
import time

import numpy as np
import pytest

import generic_nets as gn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TABLE = gn.Table("r25_generic_train")
GRAD_BATCH = {"simple15": 8, "resnet15x64": 10, "resnet15x256": 6}


def _problem(cfg, n, seed):
    kind, side, blocks, nf = cfg
    rs = np.random.RandomState(seed)
    prm = gn.params(*cfg, seed=seed + 1)
    states = (rs.rand(n, 9, side, side) > 0.6).astype(np.float32)
    pis = rs.dirichlet(np.ones(side * side), size=n).astype(np.float32)
    zs = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    return prm, states, pis, zs


@pytest.mark.parametrize("cfg", gn.GEN, ids=gn.GEN_IDS)
def test_trainer_gradients_match_float64_autograd_on_the_generic_nets(cfg):
    """test_gpu_train.py::test_trainer_gradients_match_float64_autograd on these nets: loss to 2e-5, every gradient to 1e-4 of
    its tensor's scale, at most 2e-5 * numel + 3 ReLU decisions away from the plain float64 graph, statistics to 2e-4 / 2e-5."""
    from alphapig_amd.train import HipTrainer
    from torch_trainer import TorchTrainer
    from test_gpu_train import _compare_grads, _hip_masks
    kind, side, blocks, nf = cfg
    name = gn.gen_id(*cfg)
    n = GRAD_BATCH[name]
    t0 = time.time()
    prm, states, pis, zs = _problem(cfg, n, seed=side + n)
    tr = HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, dropout=0.5, seed=5)
    assert tr.rows16 is False
    loss3 = tr.loss_and_grads(states, pis, zs, keep_tape=True).cpu().numpy().astype(np.float64)
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
    TABLE.add(test="trainer_gradients_match_float64_autograd", net=name, n=n, loss_err_over_bar=loss_ratio,
              grad_err_over_bar=worst, relu_flips=flips, seconds=round(time.time() - t0, 3))


def test_training_steps_on_the_256_filter_net_are_the_same_bits_on_every_run():
    """test_gpu_train.py::test_training_steps_are_the_same_bits_on_every_run on the widest generic net: 256 -> 256 layers stage two
    LDS chunks per board in the forward and the data gradient, and the direct weight-gradient kernel adds per-slice partial sums."""
    from alphapig_amd.train import HipTrainer
    cfg = ("resnet", 15, 1, 256)
    t0 = time.time()
    prm, states, pis, zs = _problem(cfg, 13, seed=9)
    runs = []
    for _ in range(2):
        tr = HipTrainer(prm, "resnet", n_blocks=1, batch_size=13, dropout=0.5, seed=5)
        assert tr.rows16 is False
        losses = [tr.train_step(states, pis, zs, 2e-3) for _ in range(3)]
        runs.append((losses, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()}))
        tr.close()
    assert np.isfinite(np.asarray(runs[0][0], np.float64)).all()
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k], err_msg=k)
    for k in runs[0][2]:
        np.testing.assert_array_equal(runs[0][2][k], runs[1][2][k], err_msg=k)
    assert any(np.abs(runs[0][1][k] - np.asarray(prm[k], np.float32)).max() > 0 for k in ("convA1_weight", "convB1_weight"))
    TABLE.add(test="training_steps_are_the_same_bits_on_every_run", net=gn.gen_id(*cfg), n=13, seconds=round(time.time() - t0, 3))


@pytest.mark.parametrize("cfg", gn.GEN, ids=gn.GEN_IDS)
def test_evaluator_after_a_step_equals_a_fresh_evaluator(cfg):
    """After one optimiser step, sync_evaluator (apz_load_weights_dev from the trainer's tensors, behind the step on its stream)
    leaves the evaluator with the bits of a PolicyValueNet constructed from trainer.get_params()."""
    from alphapig_amd.policy_value_net import PolicyValueNet
    from alphapig_amd.train import HipTrainer
    kind, side, blocks, nf = cfg
    t0 = time.time()
    prm, states, pis, zs = _problem(cfg, 8, seed=21)
    _, planes = gn.positions(5, side)
    kw = dict(batch_size=8, n_blocks=blocks, n_filter=nf, net_kind=kind)
    net = PolicyValueNet(side, side, model_params=prm, **kw)
    tr = HipTrainer(prm, kind, n_blocks=blocks, batch_size=8, dropout=0.5, seed=3)
    assert tr.rows16 is False
    before = net.forward_with_logits(planes)
    loss = tr.train_step(states, pis, zs, 2e-3)
    assert np.isfinite(np.asarray(loss, np.float64)).all()
    tr.sync_evaluator(net)
    got = net.forward_with_logits(planes)
    fresh = PolicyValueNet(side, side, model_params=tr.get_params(), **kw)
    want = fresh.forward_with_logits(planes)
    assert np.abs(np.asarray(before[0]) - np.asarray(want[0])).max() > 1e-4        # the step moved the answer
    for name, a, b in zip(("logits", "probs", "value_logit", "values"), got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=name)
    for x in (net, fresh):
        x.close()
    tr.close()
    TABLE.add(test="evaluator_after_a_step_equals_a_fresh_evaluator", net=gn.gen_id(*cfg), n=5, seconds=round(time.time() - t0, 3))
