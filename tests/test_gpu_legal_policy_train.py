"""The legal-move policy in the training step (HipTrainer(legal_policy=True): hipconv.pv_loss(occ=...), the occupancy made on
the device from the batch's planes) on the three trainer routes: the 15x15 padded-row trunk, a framed
9x9 board and the dense 8x8 simple net.  The planes are those of tests/test_gpu_train.py (independent 0 / 1 cells at density
0.4: the inputs its bars were set on), so about two cells in three carry a stone; pi lives on the empty cells, as visit
counts do."""
import numpy as np
import pytest

from alphapig_amd import weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 8
ROUTES = {"r15": ("resnet", 15, 1, False), "f9": ("resnet", 9, 1, True), "s8": ("simple", 8, 0, False)}


def problem(name, empty=False):
    """-> (params, states [N][9][S][S], pis [N][S*S], zs [N], occ bool [N][S*S]); empty: N boards without a stone"""
    kind, side, blocks, _ = ROUTES[name]
    rs = np.random.RandomState(100 + side)
    prm = weights.init_params(kind, side, side, 9, blocks, 128, seed=side + 1, style="bench")
    states = (rs.rand(N, 9, side, side) > 0.6).astype(np.float32)
    if empty:
        states[:, 6:8] = 0
    # move m = h * W + w counts rows from the bottom, the planes from the top
    occ = ((states[:, 6] != 0) | (states[:, 7] != 0))[:, ::-1].reshape(N, side * side)
    pis = rs.dirichlet(np.ones(side * side), size=N) * ~occ
    pis = (pis / pis.sum(axis=1, keepdims=True)).astype(np.float32)
    zs = rs.choice([-1.0, 1.0], size=N).astype(np.float32)
    return prm, states, pis, zs, occ


def trainer(name, prm, legal=True, **kw):
    from alphapig_amd.train import HipTrainer
    kind, side, blocks, framed = ROUTES[name]
    return HipTrainer(prm, kind, n_blocks=blocks, batch_size=N, dropout=0.5, seed=5, framed=framed, legal_policy=legal, **kw)


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg=k)


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_gradients_match_float64_autograd_with_the_stones_masked(name):
    """Every gradient of one forward + backward against float64 autograd of the same graph (tests/torch_trainer.py, the HIP
    dropout masks and ReLU decisions) with -inf on the occupied logits in front of log_softmax, at the bars
    tests/test_gpu_train.py holds the unmasked step to: 2e-5 (1 + |loss|) on loss and entropy, 1e-4 of each gradient's scale"""
    from test_gpu_train import _compare_grads, _hip_masks
    from torch_trainer import TorchTrainer
    kind, side, blocks, _ = ROUTES[name]
    prm, states, pis, zs, occ = problem(name)
    mask = torch.as_tensor(occ)

    class Masked(TorchTrainer):
        def forward(self, states, train=True):
            F = self.torch.nn.functional
            plain = F.log_softmax
            F.log_softmax = lambda logits, dim: plain(logits.masked_fill(mask, float("-inf")), dim=dim)
            try:
                return TorchTrainer.forward(self, states, train)
            finally:
                F.log_softmax = plain

        def loss(self, states, mcts_probs, winners, train=True):
            logp, v = self.forward(states, train)
            assert bool(torch.isinf(logp[mask]).all())
            logp = logp.masked_fill(mask, 0.0)                     # the sums run over the empty cells
            p = logp.exp().masked_fill(mask, 0.0)
            value_loss = ((winners.reshape(-1, 1) - v) ** 2).mean()
            return value_loss + (-(logp * mcts_probs).sum(dim=1)).mean(), (-(p * logp).sum(dim=1)).mean()

    tr = trainer(name, prm)
    loss3 = tr.loss_and_grads(states, pis, zs, keep_tape=True).cpu().numpy().astype(np.float64)
    got = tr.get_grads()
    masks = {k: v.cpu() for k, v in tr.relu_masks().items()}
    ref = Masked(prm, kind, n_blocks=blocks, batch_size=N, device="cpu", dtype=torch.float64, dropout=0.5,
                 mask_fn=_hip_masks(5), relu_masks=masks)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    loss, ent = ref.loss(t64(states), t64(pis), t64(zs), train=True)
    loss.backward()
    print("%s: loss %.6f (float64 %.6f)  entropy %.6f (float64 %.6f)" % (name, loss3[0] + loss3[1], float(loss), loss3[2], float(ent)))
    assert abs(loss3[0] + loss3[1] - float(loss)) < 2e-5 * (1 + abs(float(loss)))
    assert abs(loss3[2] - float(ent)) < 2e-5 * (1 + abs(float(ent)))
    assert set(got) == set(ref.train_names)
    _compare_grads(got, ref.grads(), 1e-4)
    # ... and it is another step than the unmasked one: the entropy is that of fewer cells
    off = trainer(name, prm, legal=False)
    plain3 = off.loss_and_grads(states, pis, zs).cpu().numpy()
    assert plain3[2] > loss3[2] + 1e-3 and plain3[0] == np.float32(loss3[0])
    off.close()
    tr.close()


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_two_runs_device_batches_and_a_reloaded_state_give_the_same_bits(name):
    prm, states, pis, zs, occ = problem(name)
    runs = []
    for upload in (False, False, True):
        tr = trainer(name, prm)
        batch = tr.upload(states, pis, zs) if upload else None
        losses = [tr.train_step(batch if upload else states, pis, zs, 2e-3) for _ in range(3)]
        runs.append((losses, tr.get_params(), {k: v.cpu().numpy() for k, v in tr.m.items()}, tr))
    for other in runs[1:]:                                       # a second run; a DeviceBatch uploaded once
        assert runs[0][0] == other[0]
        same(runs[0][1], other[1])
        same(runs[0][2], other[2])
    # state() / load_state(): the switch travels in meta, the step after a reload is the step that was never interrupted
    a, b = runs[0][3], runs[1][3]
    state = a.state()
    assert state["meta"]["legal_policy"] is True
    c = trainer(name, prm)
    c.load_state(state)
    assert c.legal_policy and c.state()["meta"]["legal_policy"] is True
    assert c.train_step(states, pis, zs, 2e-3) == b.train_step(states, pis, zs, 2e-3)
    same(c.get_params(), b.get_params())
    off = trainer(name, prm, legal=False)
    assert "legal_policy" not in off.state()["meta"]             # a trainer without the switch writes what it always wrote
    with pytest.raises(ValueError, match="legal_policy=True"):
        off.load_state(state)
    with pytest.raises(ValueError, match="legal_policy=False"):
        c.load_state(off.state())
    off.load_state(off.state())
    for tr in (a, b, c, off, runs[2][3]):
        tr.close()


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_a_batch_of_empty_boards_takes_the_switch_off_step(name):
    prm, states, pis, zs, occ = problem(name, empty=True)
    assert not occ.any()
    on, off = trainer(name, prm), trainer(name, prm, legal=False)
    for _ in range(2):
        assert on.train_step(states, pis, zs, 2e-3) == off.train_step(states, pis, zs, 2e-3)
    same(on.get_params(), off.get_params())
    same({k: v.cpu().numpy() for k, v in on.m.items()}, {k: v.cpu().numpy() for k, v in off.m.items()})
    on.close()
    off.close()


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_policy_update_monitors_masked_rows(name):
    from alphapig_amd.train import policy_update
    prm, states, pis, zs, occ = problem(name)
    tr = trainer(name, prm)
    rows = []
    inner = tr.policy_value

    def recording(batch):
        out = inner(batch)
        rows.append(np.array(out[0], copy=True))
        return out
    tr.policy_value = recording
    loss, ent, kl, mult = policy_update(tr, [(states[i], pis[i], zs[i]) for i in range(N)], learn_rate=5e-3, epochs=2, kl_targ=0.02)
    assert tr._eval is not None and tr._eval.legal_policy            # the trainer's own evaluator, created with the switch
    assert np.isfinite([loss, ent, kl]).all() and kl >= -1e-6
    assert len(rows) >= 2
    for p in (rows[0], rows[-1]):                                    # the monitor's old and new rows
        assert not p[occ].view(np.uint32).any() and (p[~occ] > 0).all()
        assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 2e-5
    assert np.abs(rows[0] - rows[-1]).max() > 0
    tr.close()
