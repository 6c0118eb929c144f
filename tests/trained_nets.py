"""Weights the project's own training step produces, and the float64 yardstick the inference kernels are held to on them
-- TEST HELPER ONLY (tests/test_gpu_trained_weights.py on the GPU, tests/test_trained_bounds.py on the CPU).

Every other inference test builds its net with weights.init_params(style="bench" / "reference"): BatchNorm statistics drawn
from fixed ranges that do not depend on what the layers compute.  A net that has taken optimiser steps holds the statistics
of its own activations (stem variances of 1e-2, trunk variances from 0.05 to tens, residual streams of 20 to 30), and the
kernels whose accuracy depends on operand magnitude -- the Winograd transforms, the f16x2 hi / lo split with its per-channel
weight scale, the per-layer activation exponent, the BatchNorm fold of csrc/weights_pack.h -- see other operands there.

  fixture_tuples(side)      the committed self-play episodes (tests/golden/selfplay_episodes.npz) after get_equi_data
  trained_params(...)       HipTrainer steps from the Xavier "reference" start on those tuples; cached per process; asserts
                            that the trained regime was reached, so that no test on its weights passes vacuously
  trained_params_cpu(...)   the same loop on tests/torch_trainer.py (float32, CPU)
  eval_positions(side)      about 40 boards: fixture positions no training batch drew, test_gpu_net.random_positions, an
                            empty and a full board
  Reference                 float64 layer outputs, pre-activations and the bars (all from rules the suite
                            already uses: 2e-5 on probabilities / values, (1e-4 / 3) * max(1, scale) on logits and layers)
"""
import collections
import hashlib
import os
import time

import numpy as np

from alphapig_amd import weights
from alphapig_amd.augment import get_equi_data
from oracle import net_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPISODES = {15: ("ep15_400", "ep15_a", "ep15_forced"), 8: ("ep8_a",)}
HELD_OUT_POSITIONS = {15: 18, 8: 4}          # whole positions (all eight images) kept out of every training batch
N_RANDOM = {15: 20, 8: 30}
N_EVAL = {15: 40, 8: 36}
BATCH, LR, DROPOUT, INIT_SEED, DRAW_SEED = 64, 2e-3, 0.5, 12, 1212

TOL = 1e-4 / 3.0                             # tests/test_gpu_winograd_numerics.py: 1e-4 with a 3x margin, relative above 1
HEAD_ATOL = 2e-5                             # probabilities and values, as everywhere in the suite
BN_EPS = net_ref.BN_EPS


# ---- data -------------------------------------------------------------------------------------------------------------
_tuples = {}


def fixture_tuples(side):
    """-> (states float32 [T, 9, side, side], pis float32 [T, side^2], zs float32 [T], position int [T]): the committed
    episodes of that board size after get_equi_data (eight images per position, reference order); position[t] numbers the
    position tuple t is an image of."""
    if side not in _tuples:
        g = np.load(os.path.join(GOLDEN, "selfplay_episodes.npz"))
        play = []
        for ep in EPISODES[side]:
            play += list(zip(g[ep + "/states"], g[ep + "/pis"], g[ep + "/zs"]))
        ext = get_equi_data(play, side, side)
        assert len(ext) == 8 * len(play)
        _tuples[side] = (np.stack([s for s, _, _ in ext]).astype(np.float32),
                         np.stack([p for _, p, _ in ext]).astype(np.float32),
                         np.asarray([z for _, _, z in ext], np.float32), np.repeat(np.arange(len(play)), 8))
    return _tuples[side]


def held_out(side):
    """Position numbers that no training batch draws (a fixed choice)."""
    n_pos = len(fixture_tuples(side)[0]) // 8
    return np.sort(np.random.RandomState(77).permutation(n_pos)[:HELD_OUT_POSITIONS[side]])


def _train(trainer, side, steps):
    states, pis, zs, pos = fixture_tuples(side)
    pool = np.flatnonzero(~np.isin(pos, held_out(side)))
    rs = np.random.RandomState(DRAW_SEED)
    losses = []
    for _ in range(steps):
        idx = rs.choice(pool, BATCH, replace=False)
        loss, _ = trainer.train_step(states[idx], pis[idx], zs[idx], LR)
        losses.append(float(loss))
    return losses


def _start(kind, side, n_blocks):
    return weights.init_params(kind, side, side, 9, n_blocks, 128, seed=INIT_SEED, style="reference")


def trunk_var_names(kind, n_blocks):
    if kind == "resnet":
        return ["bn%s%d_moving_var" % (ab, i) for i in range(1, n_blocks + 1) for ab in "AB"]
    return [name + "_var" for name, _ in net_ref.SIMPLE_LAYERS[1:]]


def assert_trained_regime(prm, losses, kind, n_blocks):
    """The three marks of the trained corner (measured with room to spare on the CPU trainer before any kernel ran here)."""
    assert np.isfinite(losses).all()
    assert np.mean(losses[-20:]) < losses[0], (losses[0], losses[-20:])
    stem_var = np.asarray(prm["res_conv1_var" if kind == "resnet" else "conv1_var"])
    assert stem_var.max() < 0.25, stem_var.max()
    for name in trunk_var_names(kind, n_blocks):
        v = np.asarray(prm[name])
        assert v.min() < 0.25 or v.max() > 3.0, (name, v.min(), v.max())


Trained = collections.namedtuple("Trained", "params losses trainer seconds sha256")
_trained = {}


def params_sha256(prm):
    h = hashlib.sha256()
    for k in sorted(prm):
        h.update(k.encode())
        h.update(np.ascontiguousarray(prm[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def trained(kind, side, n_blocks, steps, arith="f32"):
    """The cached training run with its live trainer (for sync_evaluator), wall time and parameter digest."""
    key = (kind, side, n_blocks, steps, arith)
    if key not in _trained:
        from alphapig_amd.train import HipTrainer
        t0 = time.time()
        tr = HipTrainer(_start(kind, side, n_blocks), net_kind=kind, n_blocks=n_blocks, batch_size=BATCH, dropout=DROPOUT,
                        seed=INIT_SEED, trunk_arith=arith)
        losses = _train(tr, side, steps)
        prm = tr.get_params()
        assert_trained_regime(prm, losses, kind, n_blocks)
        _trained[key] = Trained(prm, losses, tr, time.time() - t0, params_sha256(prm))
    return _trained[key]


def trained_params(kind, side, n_blocks, steps, arith="f32"):
    """-> (parameters {name: float32 array}, loss history): `steps` HipTrainer steps (batch 64, lr 2e-3, dropout 0.5,
    batches drawn with a fixed RandomState) from init_params(style="reference", seed fixed); cached per process."""
    t = trained(kind, side, n_blocks, steps, arith)
    return t.params, t.losses


_trained_cpu = {}


def trained_params_cpu(kind, side, n_blocks, steps):
    """The same loop on tests/torch_trainer.py (float32 autograd on the CPU) -> (parameters, loss history)."""
    key = (kind, side, n_blocks, steps)
    if key not in _trained_cpu:
        from torch_trainer import TorchTrainer
        tr = TorchTrainer(_start(kind, side, n_blocks), net_kind=kind, n_blocks=n_blocks, batch_size=BATCH, dropout=DROPOUT,
                          seed=INIT_SEED)
        losses = _train(tr, side, steps)
        _trained_cpu[key] = (tr.get_params(), losses)
    return _trained_cpu[key]


_positions = {}


def eval_positions(side):
    """float32 [n, 9, side, side]: an empty board, a full board, then held-out fixture positions (one image each on 15x15,
    two on 8x8) and random positions by turns.  Any leading slice holds some of each."""
    if side not in _positions:
        from test_gpu_net import random_positions
        from alphapig_amd.treepool import TreePool
        states, _, _, pos = fixture_tuples(side)
        per = 1 if side == 15 else 2
        held = [states[8 * p + (3 * j + p) % 8] for p in held_out(side) for j in range(per)]
        _, rnd = random_positions(N_RANDOM[side], side, seed=4000 + side)
        pool = TreePool(side, side, 4 if side < 15 else 5, n_games=1, n_playout=1)
        edge = []
        for k in (0, side * side):
            cells = np.random.RandomState(5).permutation(side * side)[:k]
            pool.set_position(0, cells, [1 + (i % 2) for i in range(k)], 1 + (k % 2))
            edge.append(pool.codes_to_planes(pool.codes(0)[None], 9)[0])
        assert edge[0][:8].sum() == 0 and edge[1][6:8].sum() == side * side
        out = list(edge)
        for i in range(max(len(held), len(rnd))):
            out += [held[i]] if i < len(held) else []
            out += [rnd[i]] if i < len(rnd) else []
        seen, uniq = set(), []
        for p in out:                         # (a random position of no stones is the empty board again)
            key = np.asarray(p, np.float32).tobytes()
            if key not in seen:
                seen.add(key)
                uniq.append(p)
        assert len(uniq) >= N_EVAL[side]
        _positions[side] = np.ascontiguousarray(np.stack(uniq[:N_EVAL[side]]), dtype=np.float32)
    return _positions[side]


# ---- the float64 side -------------------------------------------------------------------------------------------------
def layer_names(kind, n_blocks):
    """Per engine layer: (conv name, BatchNorm name, fix_gamma)."""
    if kind == "resnet":
        out = [("res_conv1", "res_conv1", True)]
        for i in range(1, n_blocks + 1):
            out += [("convA%d" % i, "bnA%d" % i, False), ("convB%d" % i, "bnB%d" % i, False)]
        return out
    return [(name, name, True) for name, _ in net_ref.SIMPLE_LAYERS]


def folded(prm, conv, bn, fix_gamma):
    """float64 (w * scale[co], shift[co]): scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta."""
    mean_n, var_n = ("_mean", "_var") if fix_gamma else ("_moving_mean", "_moving_var")
    f = lambda k: np.asarray(prm[k], np.float64)
    gamma = 1.0 if fix_gamma else f(bn + "_gamma")
    scale = gamma / np.sqrt(f(bn + var_n) + BN_EPS)
    return f(conv + "_weight") * scale[:, None, None, None], (f(conv + "_bias") - f(bn + mean_n)) * scale + f(bn + "_beta")


class Reference(object):
    """float64 results of `planes` on `prm` with the bars of every quantity:
      layers[l]   output of conv layer l in apz_layer_io order;   layer_bar[l] = TOL * max(1, max |layers[l]|)
      pre[l]      its pre-activation (before ReLU; the skip added), and chan_bar[l][c] = TOL * max(1, A_c), A_c = the maximum
                  over boards and cells of conv(|x|, |folded w|)[c] + |shift[c]|: the magnitude the fp32 rounding error of
                  channel c scales with, whatever cancels in the sum and however large the other channels are
                  (computed for the layers in `detail`; default all)
      logits, probs, vlogit, value and their bars."""

    def __init__(self, prm, planes, kind, n_blocks=0, detail=None):
        self.kind, self.n_blocks, self.n = kind, n_blocks, len(planes)
        o = net_ref.forward(prm, planes, kind, n_blocks, np.float64, return_layers=True)
        self.logits, self.probs, self.vlogit, self.value = o[0], o[1], o[2][:, 0], o[3][:, 0]
        self.layers = o[4]
        names = layer_names(kind, n_blocks)
        assert len(names) == len(self.layers)
        self.detail = list(range(len(names))) if detail is None else list(detail)
        self.pre, self.A = {}, {}
        x64 = np.asarray(planes, np.float64)
        for l in self.detail:
            conv, bn, fix = names[l]
            w, shift = folded(prm, conv, bn, fix)
            x = x64 if l == 0 else self.layers[l - 1]
            pre = net_ref._conv(x, w, shift)
            if kind == "resnet" and l >= 2 and l % 2 == 0:
                pre = pre + self.layers[l - 2]
            # the folded form is the same function as the oracle's unfolded BatchNorm
            assert np.abs(np.maximum(pre, 0) - self.layers[l]).max() <= 1e-10 * max(1.0, np.abs(self.layers[l]).max())
            self.pre[l] = pre
            self.A[l] = net_ref._conv(np.abs(x), np.abs(w), np.abs(shift)).max(axis=(0, 2, 3))
        self.layer_scale = [max(1.0, float(np.abs(a).max())) for a in self.layers]
        self.logit_scale = max(1.0, float(np.abs(self.logits).max()))
        self.vlogit_scale = max(1.0, float(np.abs(self.vlogit).max()))

    def layer_bar(self, l):
        return TOL * self.layer_scale[l]

    def chan_bar(self, l):
        return TOL * np.maximum(1.0, self.A[l])

    def check_layer(self, l, got, rows=slice(None)):
        """-> (record, failures) of one layer's output for the boards `rows` of the reference."""
        want = self.layers[l][rows]
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        rec = {"layer": l, "scale": self.layer_scale[l], "act_max": float(np.abs(want).max())}
        bad = []
        if not np.isfinite(got).all():
            return dict(rec, err=float("inf"), err_over_bar=float("inf")), ["layer %d: non-finite output" % l]
        diff = np.abs(got - want)
        rec["err"] = float(diff.max())
        rec["err_over_bar"] = rec["err"] / self.layer_bar(l)
        if rec["err_over_bar"] >= 1.0:
            bad.append("layer %d: error %.3g over the layer bar %.3g" % (l, rec["err"], self.layer_bar(l)))
        if l in self.A:
            cbar = self.chan_bar(l)
            ratio = diff.max(axis=(0, 2, 3)) / cbar
            rec["chan_err_over_bar"] = float(ratio.max())
            if rec["chan_err_over_bar"] >= 1.0:
                c = int(ratio.argmax())
                bad.append("layer %d channel %d: error %.3g over its bar %.3g" % (l, c, ratio[c] * cbar[c], cbar[c]))
            dead = (self.pre[l][rows] < -cbar[None, :, None, None]).all(axis=(0, 2, 3))
            rec["dead_channels"] = int(dead.sum())
            alive = np.flatnonzero(dead & (got != 0).any(axis=(0, 2, 3)))
            if len(alive):
                bad.append("layer %d: dead channels %s are not exactly 0" % (l, alive[:8].tolist()))
        return rec, bad

    def check_heads(self, heads, rows=slice(None)):
        """heads = (logits, probs, value logits, values) as forward_with_logits returns them."""
        logits, probs, vlog, vals = [np.asarray(a, np.float64) for a in heads]
        rec, bad = {}, []
        for name, got, want, bar in (("logits", logits, self.logits[rows], TOL * self.logit_scale),
                                     ("value_logit", vlog, self.vlogit[rows], TOL * self.vlogit_scale),
                                     ("probs", probs, self.probs[rows], HEAD_ATOL), ("values", vals, self.value[rows], HEAD_ATOL)):
            assert got.shape == want.shape, (name, got.shape, want.shape)
            err = float(np.abs(got - want).max()) if np.isfinite(got).all() else float("inf")
            rec[name + "_err"] = err
            rec[name + "_err_over_bar"] = err / bar
            if err >= bar:
                bad.append("%s: error %.3g over the bar %.3g" % (name, err, bar))
        rec["logit_scale"], rec["value_logit_scale"] = self.logit_scale, self.vlogit_scale
        return rec, bad


def comparator_gate(split, direct, wino, scale):
    """The split kernels' gate of tests/test_gpu_winograd_numerics.py, per layer: error <= max(2 x the direct kernel's error,
    1.25 x the fp32 Winograd kernel's error, 1e-6 x the layer scale), all three measured on the same inputs."""
    return split <= max(2.0 * direct, 1.25 * wino, 1e-6 * scale)


def torch_forward_layers(prm, planes, kind, n_blocks, dtype):
    """The inference graph with PyTorch's library operators on the CPU in `dtype` -> (logits, probs, value logits, values,
    [layer outputs]) as NumPy arrays: the independent second source of the oracle's per-layer outputs (float64) and the
    'plain float32 forward' the bars are tried on (float32)."""
    import torch
    F = torch.nn.functional
    t = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in prm.items()}

    def bn(x, name, fix_gamma, mean_n, var_n):
        gamma = torch.ones_like(t[name + "_beta"]) if fix_gamma else t[name + "_gamma"]
        return F.batch_norm(x, t[name + mean_n], t[name + var_n], gamma, t[name + "_beta"], training=False, eps=BN_EPS)

    def conv_act(x, name):
        k = t[name + "_weight"].shape[-1]
        return F.relu(bn(F.conv2d(x, t[name + "_weight"], t[name + "_bias"], padding=k // 2), name, True, "_mean", "_var"))

    x = torch.tensor(np.asarray(planes), dtype=dtype)
    layers = []
    if kind == "resnet":
        x = conv_act(x, "res_conv1")
        layers.append(x)
        for i in range(1, n_blocks + 1):
            y = F.conv2d(x, t["convA%d_weight" % i], t["convA%d_bias" % i], padding=1)
            y = F.relu(bn(y, "bnA%d" % i, False, "_moving_mean", "_moving_var"))
            layers.append(y)
            y = F.conv2d(y, t["convB%d_weight" % i], t["convB%d_bias" % i], padding=1)
            x = F.relu(bn(y, "bnB%d" % i, False, "_moving_mean", "_moving_var") + x)
            layers.append(x)
    else:
        for name, _ in net_ref.SIMPLE_LAYERS:
            x = conv_act(x, name)
            layers.append(x)
    logits = F.linear(conv_act(x, "conv3_1_1").flatten(1), t["fc_3_1_1_weight"], t["fc_3_1_1_bias"])
    vlogit = F.linear(conv_act(x, "conv3_2_1").flatten(1), t["fc_3_2_1_weight"], t["fc_3_2_1_bias"])[:, 0]
    return (logits.numpy(), torch.softmax(logits, dim=1).numpy(), vlogit.numpy(), torch.tanh(vlogit).numpy(),
            [a.numpy() for a in layers])
