"""The averaged weights on the GPU (csrc/ema.h; HipTrainer(ema_decay=...)).  Everything is compared bit for bit.
  (1) ema_update_kernel against the NumPy float32 expression s + c * (w - s): tensors of 1 .. 32 * 256 + 7 elements that start
      0 .. 3 floats past a 16-byte boundary inside guarded parent buffers; w and the guards untouched; an empty table;
      NaN / inf weights by class;
  (2) the two skip words;
  (3) the trainer: ema_params() is the NumPy recurrence over get_params(), and weights, moments, statistics and losses are
      those of a trainer without the average;
  (4) a refused step (guard) moves neither ema_p nor ema_updates;
  (5) an overflowed f16x2 step moves the average once, to the f32 trainer's bits;
  (6) state() / load_state;
  (7) sync_evaluator(net, ema=True) against set_params(ema_params()); PolicyValueNet and TrainPipeline hand the settings on."""
import numpy as np
import pytest

from alphapig_amd import checkpoint, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [1, 3, 4, 5, 255, 256, 257, 8191, 8192, 8193, 32 * 256 + 7]
GUARD = 8
CS = [np.float32(0.9), np.float32(1e-3), np.float32(2.0 ** -24)]


def _values(rs, n):
    """normal floats of mixed magnitude (1e-20 .. 1e20), both signs, and a few +-0; no subnormals"""
    x = (rs.choice([-1.0, 1.0], size=n) * 10.0 ** rs.uniform(-20, 20, size=n)).astype(np.float32)
    zero = rs.rand(n) < 0.05
    x[zero] = rs.choice(np.array([0.0, -0.0], np.float32), size=int(zero.sum()))
    return x


def _problem(seed, special=False):
    """-> [(s parent, w parent, s offset, w offset, n)] as host arrays: the tensor sits GUARD + offset floats into its parent,
    GUARD floats behind it"""
    rs = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(SIZES):
        so, wo = i % 4, (i + i // 4 + 1) % 4
        sp, wp = _values(rs, GUARD + so + n + GUARD), _values(rs, GUARD + wo + n + GUARD)
        if i % 3 == 0:                                    # some tensors hold w == s throughout
            wp[GUARD + wo:GUARD + wo + n] = sp[GUARD + so:GUARD + so + n]
        if special:
            idx = rs.randint(0, n, size=min(n, 6))
            wp[GUARD + wo + idx] = np.array([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf], np.float32)[:len(idx)]
        out.append((sp, wp, so, wo, n))
    return out


def _expected(problem, c):
    with np.errstate(all="ignore"):
        res = []
        for sp, wp, so, wo, n in problem:
            s, w = sp[GUARD + so:GUARD + so + n], wp[GUARD + wo:GUARD + wo + n]
            e = s + c * (w - s)                           # three float32 operations, each rounded on its own
            assert e.dtype == np.float32
            res.append(e)
        return res


def _launch(problem, c, skip=None, skip2=None):
    """-> [(s parent after, w parent after)] host arrays"""
    from alphapig_amd import hipconv
    dev = torch.device("cuda", 0)
    parents, entries = [], []
    for sp, wp, so, wo, n in problem:
        ds, dw = torch.from_numpy(sp).to(dev), torch.from_numpy(wp).to(dev)
        parents.append((ds, dw))
        s, w = ds[GUARD + so:GUARD + so + n], dw[GUARD + wo:GUARD + wo + n]
        assert (s.data_ptr() // 4) % 4 == so and (w.data_ptr() // 4) % 4 == wo      # (allocations start on 16 bytes and more)
        entries.append((s, w))
    hipconv.ema_update(entries, c, dev, skip=skip, skip2=skip2)
    torch.cuda.synchronize()
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in parents]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_outside(problem, after):
    for (sp, wp, so, wo, n), (s_after, w_after) in zip(problem, after):
        assert np.array_equal(_bits(w_after), _bits(wp)), n                                     # w: read only
        lo, hi = GUARD + so, GUARD + so + n
        assert np.array_equal(_bits(s_after[:lo]), _bits(sp[:lo])) and np.array_equal(_bits(s_after[hi:]), _bits(sp[hi:])), n


@pytest.fixture(scope="module")
def problem():
    return _problem(11)


@pytest.mark.parametrize("c", CS, ids=["0.9", "1e-3", "2^-24"])
def test_1_kernel_is_the_numpy_float32_expression(problem, c):
    after = _launch(problem, c)
    _check_outside(problem, after)
    for (sp, wp, so, wo, n), (s_after, _), want in zip(problem, after, _expected(problem, c)):
        got = s_after[GUARD + so:GUARD + so + n]
        assert np.array_equal(_bits(got), _bits(want)), (n, so, wo)
        if np.array_equal(wp[GUARD + wo:GUARD + wo + n], sp[GUARD + so:GUARD + so + n]):
            assert np.array_equal(got, sp[GUARD + so:GUARD + so + n])                           # w == s stays s
    # ones stay exactly one (the pinned gammas)
    one = [(np.ones(GUARD + 300 + GUARD, np.float32), np.ones(GUARD + 300 + GUARD, np.float32), 0, 0, 300)]
    assert np.array_equal(_bits(_launch(one, c)[0][0]), _bits(one[0][0]))


def test_1_empty_table_and_bad_arguments():
    from alphapig_amd import hipconv
    dev = torch.device("cuda", 0)
    hipconv.ema_update([], 0.5, dev)                                                            # APZ_OK: nothing raised
    L, hnd, stream = hipconv._ctx(dev)
    assert L.apz_ema_update(hnd, None, 0, 0.5, None, None, stream) == 0
    assert L.apz_ema_update(hnd, None, 1, 0.5, None, None, stream) < 0                          # as apz_adam_step: no table
    assert L.apz_ema_update(None, None, 0, 0.5, None, None, stream) < 0
    a, b = torch.zeros(4, device=dev), torch.zeros(5, device=dev)
    with pytest.raises(ValueError):
        hipconv.ema_update([(a, b)], 0.5, dev)
    with pytest.raises(ValueError):
        hipconv.ema_update([(torch.zeros(4, 4, device=dev)[:, :2], torch.zeros(4, 2, device=dev))], 0.5, dev)
    torch.cuda.synchronize()


def test_1_non_finite_weights_by_class():
    prob = _problem(12, special=True)
    c = CS[0]
    after = _launch(prob, c)
    _check_outside(prob, after)
    seen = set()
    for (sp, wp, so, wo, n), (s_after, _), want in zip(prob, after, _expected(prob, c)):
        got = s_after[GUARD + so:GUARD + so + n]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), n
        assert np.array_equal(np.signbit(got[np.isinf(got)]), np.signbit(want[np.isinf(want)])), n
        fin = np.isfinite(want)
        assert np.array_equal(_bits(got[fin]), _bits(want[fin])), n
        seen |= {"nan"} if np.isnan(got).any() else set()
        seen |= {"inf"} if np.isinf(got).any() else set()
    assert seen == {"nan", "inf"}


@pytest.mark.parametrize("words", [(None, None), (0, None), (1, None), (0, 1), (None, 1)],
                         ids=["none-none", "0-none", "1-none", "0-1", "none-1"])
def test_2_skip_words(problem, words):
    dev = torch.device("cuda", 0)
    a, b = (None if v is None else torch.tensor([v], dtype=torch.int32, device=dev) for v in words)
    c = CS[0]
    after = _launch(problem, c, skip=a, skip2=b)
    _check_outside(problem, after)
    skipped = any(v for v in words)
    for (sp, wp, so, wo, n), (s_after, _), want in zip(problem, after, _expected(problem, c)):
        got = s_after[GUARD + so:GUARD + so + n]
        assert np.array_equal(_bits(got), _bits(sp[GUARD + so:GUARD + so + n] if skipped else want)), n
    for t, v in zip((a, b), words):
        if t is not None:
            assert int(t.item()) == v                                                           # the words are only read


# ---- the trainer -------------------------------------------------------------------------------------------------------
NETS = [("resnet", 15, 1, 8), ("simple", 8, 0, 4)]
IDS = ["resnet15", "simple8"]


def _batch(side, n, seed):
    rs = np.random.RandomState(seed)
    return ((rs.rand(n, 9, side, side) > 0.6).astype(np.float32), rs.dirichlet(np.ones(side * side), size=n).astype(np.float32),
            rs.choice([-1.0, 1.0], size=n).astype(np.float32))


def _bad(batch, how):
    """the bad batches of tests/test_gpu_step_guard.py"""
    states, pis, zs = (a.copy() for a in batch)
    if how == "nan_z":
        zs[1] = np.nan
    else:
        states[2, 3, 1, 2] = np.inf
    return states, pis, zs


def _make(net, arith="f32", seed=4, **kw):
    from alphapig_amd.train import HipTrainer
    kind, side, blocks, n = net
    prm = weights.init_params(kind, side, side, 9, blocks, 128, seed=seed, style="bench")
    return HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, dropout=0.5, seed=5, trunk_arith=arith, **kw)


def _snap(tr, groups=("p", "m", "v")):
    return {g + "/" + k: v.cpu().numpy() for g in groups for k, v in getattr(tr, g).items()}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_3_trainer_follows_the_numpy_recurrence(net):
    from alphapig_amd.train import ema_coefficient
    tr, plain = _make(net, ema_decay=0.9), _make(net)
    assert plain.ema_p is None and plain.ema_updates == 0 and not any(k.startswith("e/") for k in plain.state())
    assert not hasattr(plain, "_ema_buf")                      # nothing allocated
    assert list(tr.ema_p) == list(tr.p) and tr.ema_updates == 0
    base = tr._ema_buf.data_ptr()
    off = 0
    for k, v in tr.ema_p.items():                              # views of ONE flat buffer, in p's order
        assert v.data_ptr() == base + 4 * off and v.shape == tr.p[k].shape
        off += v.numel()
    assert off == tr._ema_buf.numel()
    e = tr.get_params()
    _same(tr.ema_params(), e)                                  # starts as a copy of p (pinned gammas at 1)
    batches = [_batch(net[1], net[3], s) for s in (1, 2)]
    for step in range(5):
        out = tr.train_step(*batches[step % 2], 2e-3)
        assert out == plain.train_step(*batches[step % 2], 2e-3)
        c = ema_coefficient(0.9, step, True)
        p = tr.get_params()
        e = {k: e[k] + c * (p[k] - e[k]) for k in e}
        assert all(v.dtype == np.float32 for v in e.values())
        _same(tr.ema_params(), e)                              # statistics included
        assert tr.ema_updates == step + 1
        _same(_snap(tr), _snap(plain))
    for k in tr.fixed_gamma_names:
        assert np.array_equal(tr.ema_params()[k], np.ones_like(e[k]))
    assert any(not np.array_equal(e[k], p[k]) for k in tr.train_names)
    with pytest.raises(ValueError):
        plain.ema_params()
    for t in (tr, plain):
        t.close()


@pytest.mark.parametrize("how", ["nan_z", "inf_plane"])
@pytest.mark.parametrize("net,arith", [(NETS[0], "f32"), (NETS[0], "f16x2"), (NETS[1], "f32")],
                         ids=["resnet15-f32", "resnet15-f16x2", "simple8"])
def test_4_a_refused_step_moves_nothing(net, arith, how):
    good, good2 = _batch(net[1], net[3], 1), _batch(net[1], net[3], 2)
    a, b = (_make(net, arith, step_guard=True, ema_decay=0.9) for _ in range(2))
    a.train_step(*good, 2e-3)
    b.train_step(*good, 2e-3)
    before, n0 = _snap(b, ("p", "m", "v", "ema_p")), b.ema_updates
    assert n0 == 1
    b.train_step(*_bad(good, how), 2e-3)
    assert b.skipped_steps == 1 and b.t == 1
    _same(_snap(b, ("p", "m", "v", "ema_p")), before)
    assert b.ema_updates == n0
    assert a.train_step(*good2, 2e-3) == b.train_step(*good2, 2e-3)             # a good step afterwards advances them once
    assert (a.ema_updates, b.ema_updates) == (2, 2)
    _same(_snap(a, ("p", "m", "v", "ema_p")), _snap(b, ("p", "m", "v", "ema_p")))
    assert any(before["ema_p/" + k].tobytes() != v.cpu().numpy().tobytes() for k, v in b.ema_p.items())
    for t in (a, b):
        t.close()


def _hot_problem():
    """the overflow of tests/test_gpu_step_guard.py / test_gpu_train_f16x2.py: bnA1_gamma of one channel at 5e3, so the next
    convolution's transformed input leaves the fp16 range in every forward pass of this net"""
    rs = np.random.RandomState(21)
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=22, style="bench")
    hot = dict(prm)
    hot["bnA1_gamma"] = np.array(prm["bnA1_gamma"], dtype=np.float32).copy()
    hot["bnA1_gamma"][3] = 5e3
    n = 40
    return hot, ((rs.rand(n, 9, 15, 15) > 0.6).astype(np.float32), rs.dirichlet(np.ones(225), size=n).astype(np.float32),
                 rs.choice([-1.0, 1.0], size=n).astype(np.float32))


@pytest.mark.parametrize("guard", [False, True], ids=["unguarded", "guarded"])
def test_5_an_overflowed_f16x2_step_moves_the_average_once(guard):
    from alphapig_amd.train import HipTrainer
    hot, batch = _hot_problem()
    h, r = (HipTrainer(hot, "resnet", n_blocks=2, batch_size=40, dropout=0.5, seed=2, trunk_arith=arith, step_guard=guard,
                       ema_decay=0.9) for arith in ("f16x2", "f32"))
    assert h.train_step(*batch, 1e-3) == r.train_step(*batch, 1e-3)
    assert h.trunk_overflows == 1 and r.trunk_overflows == 0                    # the step did overflow and was repeated
    assert (h.ema_updates, r.ema_updates) == (1, 1)
    _same(_snap(h, ("ema_p", "p")), _snap(r, ("ema_p", "p")))
    assert any(not np.array_equal(v.cpu().numpy(), h.p[k].cpu().numpy()) for k, v in h.ema_p.items())
    for t in (h, r):
        t.close()


def test_6_state_round_trip(tmp_path):
    net = NETS[0]
    good, good2 = _batch(net[1], net[3], 1), _batch(net[1], net[3], 2)
    a = _make(net, ema_decay=0.9)
    a.train_step(*good, 2e-3)
    a.train_step(*good2, 2e-3)
    checkpoint.write_part(str(tmp_path), "trainer", a.state())
    state = checkpoint.read_part(str(tmp_path), "trainer")
    meta = state["meta"]
    assert (meta["ema_decay"], meta["ema_warmup"], meta["ema_updates"]) == (0.9, True, 2)
    assert sorted(k[2:] for k in state if k.startswith("e/")) == sorted(a.p)
    b = _make(net, seed=99, ema_decay=0.9)
    views = {k: v.data_ptr() for k, v in b.ema_p.items()}
    b.load_state(state)
    assert views == {k: v.data_ptr() for k, v in b.ema_p.items()} and b.ema_updates == 2
    for batch in (good, good2):
        assert a.train_step(*batch, 2e-3) == b.train_step(*batch, 2e-3)
    assert (a.ema_updates, b.ema_updates) == (4, 4)
    _same(_snap(a, ("p", "m", "v", "ema_p")), _snap(b, ("p", "m", "v", "ema_p")))
    # a wrong shape among the e/ arrays: refused before anything is written
    before = _snap(b, ("p", "ema_p"))
    broken = dict(state)
    broken["e/fc_3_1_1_bias"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        b.load_state(broken)
    _same(_snap(b, ("p", "ema_p")), before)
    # a state without the average into an averaging trainer: the average starts at the loaded weights
    plain = _make(net)
    plain.train_step(*good, 2e-3)
    pstate = plain.state()
    assert not any(k.startswith("e/") for k in pstate) and "ema_decay" not in pstate["meta"]
    b.load_state(pstate)
    assert b.ema_updates == 0 and b.t == 1
    _same(b.ema_params(), b.get_params())
    _same(b.get_params(), plain.get_params())
    # a state with the average into a trainer without: ignored
    plain.load_state(state)
    assert plain.ema_p is None and plain.ema_updates == 0 and plain.t == 2
    for t in (a, b, plain):
        t.close()


def test_7_sync_evaluator_installs_the_average():
    from alphapig_amd.policy_value_net import PolicyValueNet
    net = NETS[0]
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=4, style="bench")
    tr = _make(net, ema_decay=0.9)
    for s in (1, 2, 3):
        tr.train_step(*_batch(15, 8, s), 2e-3)
    boards = _batch(15, 8, 7)[0]
    a = PolicyValueNet(15, 15, batch_size=8, n_blocks=1, n_filter=128, model_params=prm)
    b = PolicyValueNet(15, 15, batch_size=8, n_blocks=1, n_filter=128, model_params=prm)
    tr.sync_evaluator(a, ema=True)
    b.set_params(tr.ema_params())
    pa, va = a.policy_value(boards)
    pb, vb = b.policy_value(boards)
    assert pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
    tr.sync_evaluator(a)                                       # and the raw weights give another answer
    assert a.policy_value(boards)[0].tobytes() != pa.tobytes()
    plain = _make(net)
    with pytest.raises(ValueError):
        plain.sync_evaluator(a, ema=True)
    for t in (tr, plain, a, b):
        t.close()


def test_7_net_hands_the_settings_to_its_trainer():
    from alphapig_amd.policy_value_net import PolicyValueNet
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=4, style="bench")
    net = PolicyValueNet(15, 15, batch_size=8, n_blocks=1, n_filter=128, model_params=prm, ema_decay=0.9, ema_warmup=False)
    assert net.ema_params() is None
    for s in (1, 2):
        net.train_step(*_batch(15, 8, s), 2e-3)
    tr = net._trainer
    assert (tr.ema_decay, tr.ema_warmup, tr.ema_updates) == (0.9, False, 2)
    raw, avg = tr.get_params(), net.ema_params()
    _same(avg, tr.ema_params())
    for k, v in net.params().items():                          # the net's own evaluator keeps the RAW weights
        assert np.array_equal(v, raw[k]), k
    assert any(not np.array_equal(avg[k], raw[k]) for k in raw)
    net.close()


def test_7_pipeline_plays_on_the_average(tmp_path):
    """One lock-step game batch on 15x15 with the real HipTrainer: conf key -> trainer, the self-play evaluator holds the
    average behind the update, the record carries ema_updates"""
    from alphapig_amd.pipeline import TrainPipeline
    conf = {"board_width": 15, "board_height": 15, "n_in_row": 5, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
            "n_playout": 8, "c_puct": 5, "buffer_size": 5000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
            "check_freq": 1000, "game_batch_num": 1, "play_batch_size": 2, "pure_mcts_playout_num": 10,
            "async_update": False, "concurrent_games": 8, "n_blocks": 1, "n_filter": 128,
            "model_dir": str(tmp_path / "models"), "ema_decay": 0.9}
    pipe = TrainPipeline(conf, device=0, seed=5, distributed=False)
    hist = pipe.run()
    tr = pipe._trainer()
    assert tr.ema_decay == 0.9 and tr.t >= 1 and hist[0]["ema_updates"] == tr.ema_updates == tr.t
    avg, raw = tr.ema_params(), tr.get_params()
    held = pipe.policy_value_net.params()
    for k in avg:
        assert np.array_equal(held[k], avg[k]), k
    assert any(not np.array_equal(avg[k], raw[k]) for k in raw)
    pipe.close()
