"""HipTrainer.train_step in every form it takes: (trunk_arith f32 / f16x2) x (guard off / on) x (average off / on), on clean
steps, on an f16x2 step that overflows and is repeated, on a step the guard refuses, and on one that does both; and
loss_and_grads on f16x2.  The 15x15 resnet with 1 block of 128 filters, n = 4, dropout 0.5.  Everything is compared bit for
bit.
  (a) clean steps: guard and average, alone or together, change no bit of the plain trainer's step;
  (b) one overflowing f16x2 step is the f32 trainer's step under the same settings, and moves the average once;
  (c) a refused step (NaN z) leaves everything as it was, the dropout masks' step included;
  (d) overflow and NaN z in one step: repeated, then skipped;
  (e) loss_and_grads on f16x2: train_step's first-attempt / repeat gradients, and no optimiser state moves."""
import numpy as np
import pytest

from alphapig_amd import weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 4
ARITHS = ["f32", "f16x2"]
GROUPS = ("p", "m", "v")                                       # (the moving statistics are tensors of p)


def _params(hot=False):
    """hot: the overflow of tests/test_gpu_train_f16x2.py::test_an_overflowed_step_is_the_f32_step -- bnA1_gamma of one
    channel at 5e3, so the next convolution's transformed input leaves the fp16 range"""
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=4, style="bench")
    if hot:
        prm = dict(prm)
        prm["bnA1_gamma"] = np.array(prm["bnA1_gamma"], dtype=np.float32).copy()
        prm["bnA1_gamma"][3] = 5e3
    return prm


def _batch(seed, nan_z=False):
    rs = np.random.RandomState(seed)
    states, pis, zs = ((rs.rand(N, 9, 15, 15) > 0.6).astype(np.float32), rs.dirichlet(np.ones(225), size=N).astype(np.float32),
                       rs.choice([-1.0, 1.0], size=N).astype(np.float32))
    if nan_z:
        zs[1] = np.nan
    return states, pis, zs


def _make(arith, guard=False, ema=False, hot=False):
    from alphapig_amd.train import HipTrainer
    return HipTrainer(_params(hot), "resnet", n_blocks=1, batch_size=N, dropout=0.5, seed=5, trunk_arith=arith,
                      step_guard=guard, ema_decay=0.9 if ema else None)


def _snap(tr, groups=GROUPS):
    return {g + "/" + k: v.cpu().numpy() for g in groups for k, v in getattr(tr, g).items()}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _all(tr):
    return _snap(tr, GROUPS + (("ema_p",) if tr.ema_p is not None else ()))


def _close(*trs):
    for tr in trs:
        tr.close()


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_a_clean_steps_are_the_plain_trainers(arith):
    forms = {(g, e): _make(arith, g, e) for g in (False, True) for e in (False, True)}
    batches = [_batch(s) for s in (1, 2, 3)]
    outs = {k: [tr.train_step(*b, 2e-3) for b in batches] for k, tr in forms.items()}
    plain = forms[False, False]
    for k, tr in forms.items():
        assert outs[k] == outs[False, False], k
        _same(_snap(tr), _snap(plain))
        assert (tr.t, tr.trunk_overflows, tr.skipped_steps, tr.clipped_steps) == (3, 0, 0, 0), k
        assert tr.ema_updates == (3 if k[1] else 0), k
    _same(_snap(forms[False, True], ("ema_p",)), _snap(forms[True, True], ("ema_p",)))
    assert any(not np.array_equal(v.cpu().numpy(), plain.p[k].cpu().numpy()) for k, v in forms[True, True].ema_p.items())
    _close(*forms.values())


# ---- (b) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [False, True], ids=["noavg", "avg"])
@pytest.mark.parametrize("guard", [False, True], ids=["unguarded", "guarded"])
def test_b_an_overflowed_step_is_the_f32_step(guard, ema):
    h, r = _make("f16x2", guard, ema, hot=True), _make("f32", guard, ema, hot=True)
    batch = _batch(1)
    assert h.train_step(*batch, 2e-3) == r.train_step(*batch, 2e-3)
    assert h.trunk_overflows == 1 and r.trunk_overflows == 0   # the step did overflow and was repeated
    _same(_all(h), _all(r))
    assert (h.t, r.t) == (1, 1) and (h.skipped_steps, h.clipped_steps) == (0, 0)
    assert h.ema_updates == r.ema_updates == (1 if ema else 0)
    assert (h.last_grad_norm, h.last_rescale_eff, h.last_skip_reason) == (r.last_grad_norm, r.last_rescale_eff, r.last_skip_reason)
    assert (h.last_grad_norm is not None) == guard
    if ema:
        assert any(not np.array_equal(v.cpu().numpy(), h.p[k].cpu().numpy()) for k, v in h.ema_p.items())
    _close(h, r)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [False, True], ids=["noavg", "avg"])
@pytest.mark.parametrize("arith", ARITHS)
def test_c_a_refused_step_leaves_everything_as_it_was(arith, ema):
    twin, tr = _make(arith, True, ema), _make(arith, True, ema)
    good, good2 = _batch(1), _batch(2)
    assert twin.train_step(*good, 2e-3) == tr.train_step(*good, 2e-3)
    before, counts = _all(tr), (tr.t, tr.ema_updates)
    loss, _ = tr.train_step(*_batch(1, nan_z=True), 2e-3)
    _same(_all(tr), before)
    assert (tr.t, tr.ema_updates) == counts == (1, 1 if ema else 0)
    assert tr.skipped_steps == 1 and not np.isfinite(loss) and "non-finite loss" in tr.last_skip_reason
    # the twin never saw the bad batch: the same next step shows that t, and with it the dropout masks, went back
    assert twin.train_step(*good2, 2e-3) == tr.train_step(*good2, 2e-3)
    _same(_all(tr), _all(twin))
    assert (tr.t, twin.t, tr.ema_updates, twin.ema_updates) == (2, 2) + ((2, 2) if ema else (0, 0))
    assert tr.last_skip_reason is None and (tr.skipped_steps, twin.skipped_steps) == (1, 0)
    _close(twin, tr)


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_d_overflow_and_a_nan_z_in_one_step():
    tr = _make("f16x2", True, True, hot=True)
    before = _all(tr)
    loss, _ = tr.train_step(*_batch(1, nan_z=True), 2e-3)
    assert (tr.trunk_overflows, tr.skipped_steps) == (1, 1)    # repeated on the exact kernels, and the repeat refused
    assert (tr.t, tr.ema_updates, tr.clipped_steps) == (0, 0, 0) and not np.isfinite(loss)
    _same(_all(tr), before)                                    # the average included
    tr.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hot", [False, True], ids=["clean", "overflowing"])
def test_e_loss_and_grads_on_f16x2(hot):
    """The gradients train_step leaves behind are those of its last pass: the first attempt's on a clean batch, the exact
    repeat's on an overflowing one.  loss_and_grads runs in training mode and so moves the moving statistics, as documented
    and as train_step's pass does; every other tensor of p, and m and v, stay."""
    a, b = _make("f16x2", hot=hot), _make("f16x2", hot=hot)
    batch = _batch(1)
    before = _snap(a)
    a.loss_and_grads(*batch)
    b.train_step(*batch, 2e-3)
    assert a.trunk_overflows == b.trunk_overflows == (1 if hot else 0)
    ga, gb = a.get_grads(), b.get_grads()
    _same(ga, gb)
    assert (a.t, b.t) == (0, 1)
    after = _snap(a)
    moved = [k for k in before if before[k].tobytes() != after[k].tobytes()]
    assert moved and all(k[2:] in a.stat_names for k in moved), moved
    _same({k: after[k] for k in after if k[2:] in a.stat_names}, {k: v for k, v in _snap(b).items() if k[2:] in a.stat_names})
    _close(a, b)
