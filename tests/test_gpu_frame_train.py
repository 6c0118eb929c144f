"""The training step on framed boards (HipTrainer(framed=True): 6x6 .. 14x14 other than 8x8 and 10x10 on the 15x15 trunk
kernels, the board mask in the BatchNorm passes -- csrc/bn_frame.h) against the PyTorch comparator tests/torch_trainer.py
at the plain S x S shapes, with the procedures and bars of tests/test_gpu_train.py; and the public interface above it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_train import _compare_grads, _hip_masks, _problem  # noqa: E402


def _off_board_words(t, S):
    """how many off-board cells of a padded-row tensor [n][C][15][16] are not exactly +0"""
    on = torch.zeros(15, 16, dtype=torch.bool, device=t.device)
    on[:S, :S] = True
    return int((t.contiguous().view(torch.int32)[..., ~on] != 0).sum())


@pytest.mark.parametrize("side,n,blocks", [(9, 24, 2), (13, 10, 1), (6, 5, 1), (14, 7, 1)])
def test_framed_trainer_gradients_match_float64_autograd(side, n, blocks):
    """test_gpu_train.py::test_trainer_gradients_match_float64_autograd, its procedure and bars, for the framed trainer
    against float64 autograd on the plain S x S board; and the invariant of the tape: every off-board cell of the
    activations a trunk convolution reads is exactly +0."""
    from alphapig_amd.train import HipTrainer
    from torch_trainer import TorchTrainer
    kind = "resnet"
    prm, states, pis, zs = _problem(kind, side, n, blocks, seed=side + n)
    tr = HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, dropout=0.5, seed=5, framed=True)
    assert tr.rows16 and tr.frame_side == side
    loss3 = tr.loss_and_grads(states, pis, zs, keep_tape=True).cpu().numpy().astype(np.float64)
    got = tr.get_grads()
    for i, blk in enumerate(tr.tape["blocks"]):
        for name in ("x", "ha", "out"):
            assert _off_board_words(getattr(blk, name), side) == 0, (i, name)
    masks = {k: v.cpu() for k, v in tr.relu_masks().items()}
    assert all(tuple(m.shape[2:]) == (side, side) for m in masks.values())
    ref = TorchTrainer(prm, kind, n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
                       mask_fn=_hip_masks(5), relu_masks=masks)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    loss, ent = ref.loss(t64(states), t64(pis), t64(zs), train=True)
    loss.backward()
    assert abs(loss3[0] + loss3[1] - float(loss)) < 2e-5 * (1 + abs(float(loss)))
    assert abs(loss3[2] - float(ent)) < 2e-5 * (1 + abs(float(ent)))
    assert set(got) == set(ref.train_names)
    _compare_grads(got, ref.grads(), 1e-4)
    plain = TorchTrainer(prm, kind, n_blocks=blocks, batch_size=n, device="cpu", dtype=torch.float64, dropout=0.5,
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
    for k in tr.fixed_gamma_names:
        assert np.all(new[k] == 1.0), k
    tr.close()


def test_framed_trainer_steps_match_the_comparator():
    """test_gpu_train.py::test_trainer_steps_match_the_comparator at 9x9"""
    from alphapig_amd.train import HipTrainer
    from torch_trainer import TorchTrainer
    prm, states, pis, zs = _problem("resnet", 9, 24, 2, seed=1)
    tr = HipTrainer(prm, "resnet", n_blocks=2, batch_size=24, dropout=0.5, seed=3, framed=True)
    ref = TorchTrainer(prm, "resnet", n_blocks=2, batch_size=24, device="cuda", dropout=0.5, mask_fn=_hip_masks(3))
    got_l, ref_l = [], []
    for _ in range(3):
        got_l.append(tr.train_step(states, pis, zs, 1e-3, keep_tape=True))
        ref.relu_masks = tr.relu_masks()
        ref_l.append(ref.train_step(states, pis, zs, 1e-3))
    np.testing.assert_allclose(got_l, ref_l, rtol=3e-4)
    a, b = tr.get_params(), ref.get_params()
    for k in ("convA1_weight", "convB2_weight", "bnA1_gamma", "bnB2_beta", "res_conv1_weight", "bnA1_moving_var",
              "bnB2_moving_mean", "fc_3_1_1_weight", "fc_3_2_1_weight", "conv3_1_1_weight", "conv3_2_1_beta"):
        d = np.abs(a[k] - b[k])
        assert int((d > 2e-4).sum()) <= max(8, 0.01 * d.size), k
        assert float(d.max()) < 2 * 1e-3 * 3 + 2e-4, k
    tr.close()


def test_framed_training_steps_are_the_same_bits_on_every_run():
    from alphapig_amd.train import HipTrainer
    prm, states, pis, zs = _problem("resnet", 13, 13, 2, seed=9)
    runs = []
    for _ in range(2):
        tr = HipTrainer(prm, "resnet", n_blocks=2, batch_size=13, dropout=0.5, seed=5, framed=True)
        losses = [tr.train_step(states, pis, zs, 2e-3) for _ in range(3)]
        runs.append((losses, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()}))
        tr.close()
    assert runs[0][0] == runs[1][0] and all(np.isfinite(l).all() for l in runs[0][0])
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k], err_msg=k)
    for k in runs[0][2]:
        np.testing.assert_array_equal(runs[0][2][k], runs[1][2][k], err_msg=k)


def test_net_train_step_on_a_framed_board():
    """PolicyValueNet(9, 9, train_framed=True).train_step: the loss falls on a fixed batch and the (framed) evaluator holds
    exactly the trainer's weights; without the switch the call is refused as it always was."""
    from alphapig_amd.policy_value_net import PolicyValueNet
    prm, states, pis, zs = _problem("resnet", 9, 32, 2, seed=9)
    plain = PolicyValueNet(9, 9, batch_size=32, n_blocks=2, n_filter=128, model_params=prm)
    with pytest.raises(ValueError, match="15x15 and 8x8"):
        plain.train_step(states, pis, zs, 2e-3)
    plain.close()
    net = PolicyValueNet(9, 9, batch_size=32, n_blocks=2, n_filter=128, model_params=prm, train_framed=True)
    p0, _ = net.policy_value(states)
    losses = []
    for _ in range(8):
        loss, ent = net.train_step(states, pis, zs, 2e-3)
        assert loss.shape == (1,) and ent.shape == (1,) and np.isfinite(loss[0]) and np.isfinite(ent[0])
        losses.append(float(loss[0]))
    p1, _ = net.policy_value(states)
    assert np.abs(p1 - p0).max() > 1e-4
    assert min(losses[-3:]) < losses[0]
    for k, v in net._trainer.get_params().items():
        np.testing.assert_array_equal(net.params()[k], v, err_msg=k)
    net.close()


def test_policy_update_on_a_framed_board():
    """train_mxnet.py:194-240 at 13x13: the KL monitor goes through the trainer's own (framed) evaluator"""
    from alphapig_amd.train import HipTrainer, policy_update
    prm, states, pis, zs = _problem("resnet", 13, 32, 1, seed=4)
    tr = HipTrainer(prm, "resnet", n_blocks=1, batch_size=32, dropout=0.5, seed=1, framed=True)
    batch = [(states[i], pis[i], zs[i]) for i in range(32)]
    mult, first = 1.0, None
    for _ in range(4):
        loss, ent, kl, mult = policy_update(tr, batch, learn_rate=5e-3, lr_multiplier=mult, epochs=3, kl_targ=0.02)
        first = loss if first is None else first
        assert np.isfinite(loss) and np.isfinite(ent) and kl >= -1e-6
    assert loss < first
    assert 0.05 / 1.5 <= mult <= 20 * 1.5
    assert (tr._evaluator().board_width, tr._evaluator().board_height) == (13, 13)
    tr.close()


def test_framed_trainer_state_round_trip():
    """state() -> load_state() into a fresh trainer: the next step has the same bits; the state carries the switch"""
    from alphapig_amd.train import HipTrainer
    prm, states, pis, zs = _problem("resnet", 9, 12, 1, seed=2)
    a = HipTrainer(prm, "resnet", n_blocks=1, batch_size=12, dropout=0.5, seed=7, framed=True)
    for _ in range(2):
        a.train_step(states, pis, zs, 1e-3)
    st = a.state()
    assert st["meta"]["framed"] is True
    b = HipTrainer(prm, "resnet", n_blocks=1, batch_size=12, dropout=0.5, seed=7, framed=True)
    b.load_state(st)
    assert a.train_step(states, pis, zs, 1e-3) == b.train_step(states, pis, zs, 1e-3)
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    # a state loaded into a trainer built the other way is refused
    prm15 = _problem("resnet", 15, 4, 1, seed=2)[0]
    on, off = (HipTrainer(prm15, "resnet", n_blocks=1, batch_size=4, framed=f) for f in (True, False))
    with pytest.raises(ValueError, match="framed"):
        off.load_state(on.state())
    with pytest.raises(ValueError, match="framed"):
        on.load_state(off.state())
    for t in (a, b, on, off):
        t.close()


def test_train_pipeline_on_a_framed_board(tmp_path):
    """One lock-step game batch of self-play on 9x9 and its update on the framed trainer"""
    from alphapig_amd.pipeline import TrainPipeline
    conf = {"board_width": 9, "board_height": 9, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
            "n_playout": 8, "c_puct": 5, "buffer_size": 5000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
            "check_freq": 1000, "game_batch_num": 1, "play_batch_size": 2, "pure_mcts_playout_num": 10,
            "async_update": False, "concurrent_games": 8, "n_blocks": 1, "n_filter": 128,
            "model_dir": str(tmp_path / "models"), "train_framed": True}
    pipe = TrainPipeline(conf, device=0, seed=5, distributed=False)
    hist = pipe.run()
    assert len(hist) == 1 and np.isfinite(hist[0]["loss"]) and np.isfinite(hist[0]["entropy"]) and np.isfinite(hist[0]["kl"])
    assert pipe._trainer().frame_side == 9 and pipe._trainer().t >= 1
    pipe.close()
