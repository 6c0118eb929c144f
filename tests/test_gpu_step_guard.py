"""HipTrainer(step_guard=True, clip_norm=...) on the GPU (csrc/grad_guard.h), batch 4: the one-block 128-filter net at 15x15
on "f32" and on "f16x2", the same net framed at 9x9, the simple net at 8x8.  Everything is compared bit for bit.
  (a) the guard on and nothing to refuse: the plain trainer's steps;
  (b) a bad mini-batch (a NaN z; a +inf in a state plane) is skipped cleanly -- and poisons a trainer without the guard;
  (c) clipping: the step is the existing adam_step with the recorded rescale_eff;
  (d) the counters through state() / load_state, and the resumed trainer's next step;
  (e) "f16x2": a pass that is SURE to overflow (a BatchNorm gamma of 5e3, two blocks, batch 40) -- the guarded exact repeat;
  (f) the settings from PolicyValueNet and from TrainPipeline's conf reach the HipTrainer they build."""
import numpy as np
import pytest

from alphapig_amd import checkpoint, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 4
NETS = [("resnet", 15, 1, "f32", False), ("resnet", 15, 1, "f16x2", False), ("resnet", 9, 1, "f32", True),
        ("simple", 8, 0, "f32", False)]
IDS = ["resnet15-f32", "resnet15-f16x2", "framed9", "simple8"]


def _batch(side, seed):
    rs = np.random.RandomState(seed)
    return ((rs.rand(N, 9, side, side) > 0.6).astype(np.float32), rs.dirichlet(np.ones(side * side), size=N).astype(np.float32),
            rs.choice([-1.0, 1.0], size=N).astype(np.float32))


def _bad(batch, how):
    states, pis, zs = (a.copy() for a in batch)
    if how == "nan_z":
        zs[1] = np.nan
    else:
        states[2, 3, 1, 2] = np.inf
    return states, pis, zs


def _make(net, **kw):
    from alphapig_amd.train import HipTrainer
    kind, side, blocks, arith, framed = net
    prm = weights.init_params(kind, side, side, 9, blocks, 128, seed=4, style="bench")
    return HipTrainer(prm, kind, n_blocks=blocks, batch_size=N, dropout=0.5, seed=5, trunk_arith=arith, framed=framed, **kw)


def _snap(tr):
    """every parameter and statistic, both moments: host copies"""
    return {g + "/" + k: v.cpu().numpy() for g in ("p", "m", "v") for k, v in getattr(tr, g).items()}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_a_guard_with_nothing_to_refuse_changes_no_bit(net):
    plain, guarded = _make(net), _make(net, step_guard=True)
    assert guarded.step_guard and guarded.clip_norm is None and not plain.step_guard
    batches = [_batch(net[1], s) for s in (1, 2)]
    for i in range(6):
        out_p = plain.train_step(*batches[i % 2], 2e-3)
        out_g = guarded.train_step(*batches[i % 2], 2e-3)
        assert out_p == out_g
        assert guarded.last_skip_reason is None and np.isfinite(guarded.last_grad_norm) and guarded.last_grad_norm > 0
        assert guarded.last_rescale_eff == np.float32(1.0 / N)
    _same(_snap(plain), _snap(guarded))
    assert (guarded.t, guarded.skipped_steps, guarded.clipped_steps) == (6, 0, 0) and plain.t == 6
    assert guarded.trunk_overflows == plain.trunk_overflows
    assert plain.skipped_steps == 0 and plain.last_grad_norm is None
    for tr in (plain, guarded):
        tr.close()


@pytest.mark.parametrize("how", ["nan_z", "inf_plane"])
@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_a_bad_batch_is_skipped_cleanly(net, how):
    good, good2 = _batch(net[1], 1), _batch(net[1], 2)
    bad = _bad(good, how)
    a, b = _make(net, step_guard=True), _make(net, step_guard=True)
    a.train_step(*good, 2e-3)
    b.train_step(*good, 2e-3)
    before = _snap(b)
    loss, entropy = b.train_step(*bad, 2e-3)
    _same(_snap(b), before)                                    # weights, moments AND moving statistics
    assert (b.t, b.skipped_steps, b.clipped_steps) == (1, 1, 0)
    print(net, how, "reason:", b.last_skip_reason, "loss", loss, "norm", b.last_grad_norm, "overflows", b.trunk_overflows)
    assert "non-finite gradient" in b.last_skip_reason and not np.isfinite(b.last_grad_norm)
    if how == "nan_z":
        assert "non-finite loss" in b.last_skip_reason and not np.isfinite(loss)      # the step's own loss is what it returns
    # (the inf plane: the stem's BatchNorm turns its channels into NaN, which the ReLU behind it reads as 0 -- the loss may
    # well be finite, the stem's gradients and its moving statistics are not; on "f16x2" an overflowed pass is repeated on
    # the exact kernels first and the repeat is guarded in turn)
    assert b.trunk_overflows in (0, 1)
    out_a, out_b = a.train_step(*good2, 2e-3), b.train_step(*good2, 2e-3)
    assert out_a == out_b and b.last_skip_reason is None
    _same(_snap(a), _snap(b))                                  # (the dropout masks of step 2 included: t went back)
    assert (a.t, b.t, a.skipped_steps, b.skipped_steps) == (2, 2, 0, 1)
    # the defect this closes: the same mini-batch on a trainer without the guard
    c = _make(net)
    c.train_step(*good, 2e-3)
    c.train_step(*bad, 2e-3)
    assert any(bool(torch.isnan(c.p[k]).any()) for k in c.train_names)
    assert all(bool(torch.isfinite(v).all()) for v in b.p.values())
    for tr in (a, b, c):
        tr.close()


def _entries(tr):
    return [(tr.p[k], tr.grad[k], tr.m[k], tr.v[k], tr.wd if k.endswith(("_weight", "_gamma")) else 0.0) for k in tr.train_names]


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_a_clipped_step_is_adam_step_with_the_recorded_rescale(net):
    from alphapig_amd import hipconv
    batch = _batch(net[1], 1)
    ref = _make(net)
    ref.loss_and_grads(*batch)
    norm = ref.grad_norm()
    assert np.isfinite(norm) and norm > 0
    # (the same number from NumPy: grad / batch_size over all trainable tensors, to float32 rounding)
    total = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in ref.get_grads().values())
    assert abs(norm - np.sqrt(total) / N) <= 2.0 ** -23 * norm
    tr = _make(net, clip_norm=norm / 2)
    assert tr.step_guard
    tr.train_step(*batch, 2e-3)
    assert (tr.t, tr.clipped_steps, tr.skipped_steps) == (1, 1, 0) and tr.last_grad_norm == norm
    eff = tr.last_rescale_eff
    assert eff != np.float32(1.0 / N) and abs(float(eff) * N - 0.5) < 1e-6
    b1, b2 = 0.9, 0.999
    lr_t = 2e-3 * (1.0 - b2) ** 0.5 / (1.0 - b1)
    hipconv.adam_step(_entries(ref), lr_t, b1, b2, 1e-8, float(eff), ref.device)
    _same(_snap(ref), _snap(tr))
    # a clip above the norm: the plain step
    plain, loose = _make(net), _make(net, clip_norm=norm * 2)
    assert plain.train_step(*batch, 2e-3) == loose.train_step(*batch, 2e-3)
    _same(_snap(plain), _snap(loose))
    assert loose.clipped_steps == 0 and loose.last_grad_norm == norm
    for t in (ref, tr, plain, loose):
        t.close()


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_counters_travel_with_the_state(tmp_path, net):
    good, good2 = _batch(net[1], 1), _batch(net[1], 2)
    a = _make(net, clip_norm=1e-3)                             # (far below the norm: every step that is taken is clipped)
    a.train_step(*good, 2e-3)
    a.train_step(*_bad(good, "nan_z"), 2e-3)
    a.train_step(*good2, 2e-3)
    assert (a.t, a.skipped_steps, a.clipped_steps) == (2, 1, 2)
    checkpoint.write_part(str(tmp_path), "trainer", a.state())
    state = checkpoint.read_part(str(tmp_path), "trainer")
    meta = state["meta"]
    assert (meta["step_guard"], meta["clip_norm"], meta["skipped_steps"], meta["clipped_steps"]) == (True, 1e-3, 1, 2)
    kind, side, blocks, arith, framed = net
    from alphapig_amd.train import HipTrainer
    other = weights.init_params(kind, side, side, 9, blocks, 128, seed=99, style="bench")
    b = HipTrainer(other, kind, n_blocks=blocks, batch_size=N, dropout=0.5, seed=5, trunk_arith=arith, framed=framed,
                   clip_norm=1e-3)
    views = {k: b.p[k].data_ptr() for k in b.p}
    b.load_state(state)
    assert views == {k: b.p[k].data_ptr() for k in b.p}        # written INTO the one-buffer statistics and the packed weights
    assert (b.t, b.skipped_steps, b.clipped_steps) == (2, 1, 2)
    assert a.train_step(*good, 2e-3) == b.train_step(*good, 2e-3)
    _same(_snap(a), _snap(b))
    assert (a.t, a.skipped_steps, a.clipped_steps) == (b.t, b.skipped_steps, b.clipped_steps) == (3, 1, 3)
    # a state from before the guard: zeros, and the trainer's own settings stand
    old = dict(state, meta={k: v for k, v in meta.items() if k not in ("step_guard", "clip_norm", "skipped_steps", "clipped_steps")})
    b.load_state(old)
    assert (b.t, b.skipped_steps, b.clipped_steps, b.step_guard, b.clip_norm) == (2, 0, 0, True, 1e-3)
    for tr in (a, b):
        tr.close()


# ---- (e) the guarded exact repeat of an overflowed f16x2 pass ---------------------------------------------------------
def _hot_problem():
    """tests/test_gpu_train_f16x2.py's overflow: bnA1_gamma of one channel at 5e3, so the next convolution's transformed
    input leaves the fp16 range in EVERY forward pass of this net"""
    rs = np.random.RandomState(21)
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=22, style="bench")
    hot = dict(prm)
    hot["bnA1_gamma"] = np.array(prm["bnA1_gamma"], dtype=np.float32).copy()
    hot["bnA1_gamma"][3] = 5e3
    n = 40
    return hot, ((rs.rand(n, 9, 15, 15) > 0.6).astype(np.float32), rs.dirichlet(np.ones(225), size=n).astype(np.float32),
                 rs.choice([-1.0, 1.0], size=n).astype(np.float32))


def _hot_trainer(prm, arith, **kw):
    from alphapig_amd.train import HipTrainer
    return HipTrainer(prm, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2, trunk_arith=arith, **kw)


def test_an_overflowed_guarded_step_is_the_f32_step():
    """The overflow word skips the first guarded Adam, the pass is repeated on the exact kernels and the repeat's own record
    decides: taken -- the plain f32 trainer's and the unguarded f16x2 trainer's loss, state and t, bit for bit.  The first
    step is the one tests/test_gpu_train_f16x2.py shows to overflow; a second one follows the unguarded f16x2 trainer in
    whatever it does, and the f32 trainer if it overflowed again."""
    hot, batch = _hot_problem()
    g, u, r = _hot_trainer(hot, "f16x2", step_guard=True), _hot_trainer(hot, "f16x2"), _hot_trainer(hot, "f32")
    for step in (1, 2):
        out = [tr.train_step(*batch, 1e-3) for tr in (g, u, r)]
        assert g.trunk_overflows == u.trunk_overflows and g.trunk_overflows >= 1
        if step == 1:
            assert g.trunk_overflows == 1                                      # the repeat did run
        assert out[0] == out[1] and np.isfinite(out[0][0])
        assert (g.t, u.t, r.t) == (step, step, step)
        assert g.skipped_steps == 0 and g.clipped_steps == 0 and g.last_skip_reason is None
        assert np.isfinite(g.last_grad_norm) and g.last_rescale_eff == np.float32(1.0 / 40)
        _same(_snap(g), _snap(u))
        if g.trunk_overflows == step:                                          # every step so far ended on the exact kernels
            assert out[0] == out[2]
            _same(_snap(g), _snap(r))
    for tr in (g, u, r):
        tr.close()


def test_an_overflowed_guarded_step_with_a_nan_z_is_skipped_after_its_repeat():
    """The same net with a NaN z: overflow, exact repeat, and the REPEAT's record says skip -- everything as before the step,
    the overflow counted once; the good batch afterwards is a fresh f32 trainer's first step."""
    hot, batch = _hot_problem()
    bad = _bad(batch, "nan_z")
    g, r = _hot_trainer(hot, "f16x2", step_guard=True), _hot_trainer(hot, "f32")
    before = _snap(g)
    loss, _ = g.train_step(*bad, 1e-3)
    _same(_snap(g), before)
    assert (g.t, g.trunk_overflows, g.skipped_steps, g.clipped_steps) == (0, 1, 1, 0) and not np.isfinite(loss)
    # the repeat's verdict, not the first pass's: no overflow among the reasons
    assert g.last_skip_reason == "non-finite gradient, non-finite loss"
    assert g.train_step(*batch, 1e-3) == r.train_step(*batch, 1e-3)
    _same(_snap(g), _snap(r))
    assert (g.t, g.trunk_overflows, g.skipped_steps, g.last_skip_reason) == (1, 2, 1, None)
    for tr in (g, r):
        tr.close()


# ---- (f) the settings reach the trainer ------------------------------------------------------------------------------
def test_net_hands_the_settings_to_its_trainer():
    from alphapig_amd.policy_value_net import PolicyValueNet
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=4, style="bench")
    good = _batch(15, 1)
    for kw, want in (({}, (False, None)), ({"train_step_guard": True}, (True, None)), ({"train_clip_norm": 1e-6}, (True, 1e-6))):
        net = PolicyValueNet(15, 15, batch_size=N, n_blocks=1, n_filter=128, model_params=prm, **kw)
        loss, _ = net.train_step(*good, 2e-3)
        tr = net._trainer
        assert (tr.step_guard, tr.clip_norm) == want and np.isfinite(loss[0])
        assert tr.clipped_steps == (1 if want[1] else 0)
        if want[0]:
            net.train_step(*_bad(good, "nan_z"), 2e-3)
            assert tr.skipped_steps == 1 and tr.t == 1
            for k, v in tr.get_params().items():               # the evaluator still holds the (finite) weights of step 1
                assert np.isfinite(v).all() and np.array_equal(net.params()[k], v), k
        net.close()


def test_pipeline_hands_the_keys_to_its_trainer(tmp_path):
    """One lock-step game batch on 15x15 with the real HipTrainer: conf keys -> trainer, counters -> history record"""
    from alphapig_amd.pipeline import TrainPipeline
    conf = {"board_width": 15, "board_height": 15, "n_in_row": 5, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
            "n_playout": 8, "c_puct": 5, "buffer_size": 5000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
            "check_freq": 1000, "game_batch_num": 1, "play_batch_size": 2, "pure_mcts_playout_num": 10,
            "async_update": False, "concurrent_games": 8, "n_blocks": 1, "n_filter": 128,
            "model_dir": str(tmp_path / "models"), "clip_norm": 1e-6}
    pipe = TrainPipeline(conf, device=0, seed=5, distributed=False)
    hist = pipe.run()
    tr = pipe._trainer()
    assert (tr.step_guard, tr.clip_norm) == (True, 1e-6) and tr.t >= 1
    rec = hist[0]
    assert np.isfinite(rec["loss"]) and rec["skipped_steps"] == 0 and rec["clipped_steps"] == tr.t == tr.clipped_steps
    assert rec["grad_norm"] == tr.last_grad_norm and rec["grad_norm"] > 1e-6
    pipe.close()
