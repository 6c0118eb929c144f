"""The legal-move policy on the GPU (apz_set_legal_policy, apz_pv_loss_legal, apz_occupancy_planes):
the operators against float64 over the empty cells and their exact requirements, then the evaluator through every entry
point, HIP graphs, the overflow repeat, the leaf symmetries and self-play.  Bars, restatements and input families:
tests/test_legal_policy_bounds.py."""
import numpy as np
import pytest

import test_head_loss_bounds as hb
import test_legal_policy_bounds as lb
from alphapig_amd import weights
from alphapig_amd.augment import leaf_symmetry_keys
from test_gpu_leaf_symmetry import evaluate_async, fold, images, planes_of, positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x1E6A1


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def run_loss(args, occ=True, grads=True):
    """hipconv.pv_loss on host arrays (logits, u, pi, z, occ) -> dict of host arrays"""
    from alphapig_amd import hipconv
    t = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in args]
    kw = {"occ": t[4]} if occ else {}
    if grads:
        out = hipconv.pv_loss(t[0], t[1], t[2], t[3], grads=True, outputs=True, **kw)
    else:
        out = hipconv.pv_loss(t[0], t[1], outputs=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. operators
@pytest.mark.parametrize("side", [15, 9, 8])
@pytest.mark.parametrize("c_in", [9, 4])
def test_occupancy_planes_equals_the_numpy_definition(side, c_in):
    from alphapig_amd import hipconv
    rs = np.random.RandomState(side + c_in)
    own = 6 if c_in == 9 else 0
    for n in lb.NS:
        planes = (rs.rand(n, c_in, side, side) < 0.3).astype(np.float32)
        planes[:, own:own + 2] *= rs.choice([1.0, -2.5, 1e-30, 7.0], size=(n, 2, side, side)).astype(np.float32)
        planes[0, own] = 0
        planes[0, own + 1] = 0                                   # a board with no stone, other planes set
        want = ((planes[:, own] != 0) | (planes[:, own + 1] != 0))[:, ::-1, :].reshape(n, side * side).astype(np.uint8)
        got = hipconv.occupancy_planes(torch.as_tensor(planes).cuda())
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, side * side)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert not want[0].any() and (n == 1 or want.any())
    # real positions: the occupancy of the planes is the code bytes' (bottom row first in both)
    codes = positions(side)[:12]
    got = hipconv.occupancy_planes(torch.as_tensor(planes_of(codes, side, c_in)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, (codes[:, :side * side] != 0).astype(np.uint8))


@pytest.mark.parametrize("hw", lb.HWS)
@pytest.mark.parametrize("n", lb.NS)
def test_masked_loss_against_float64_and_the_exact_requirements(n, hw):
    worst = {}
    for combo, lf, tf in hb.loss_combos()[::3]:
        for j, of in enumerate(lb.OCC_FAMILIES):
            args = lb.legal_loss_batch(lf, tf, of, n, hw, combo + j)
            if (combo + j) % 2:
                args = (lb.max_on_a_stone(args[0], args[4], combo),) + args[1:]
            occ = args[4] != 0
            bars, ref = lb.legal_pv_loss_bars(*args)
            got = run_loss(args)
            for k in bars:
                assert np.isfinite(got[k]).all(), (lf, tf, of, k)
                q = hb.ratio(got[k], ref[k], bars[k])
                worst[k] = max(worst.get(k, 0.0), q)
                assert q <= 1.0, (lf, tf, of, k, q)
            # the bars of the DESIGN table, spelled out (the bars above are cut at them)
            assert np.abs(got["probs"] - ref["probs"]).max() <= 1e-6
            assert (np.abs(got["loss3"] - ref["loss3"]) <= 1e-5 * (1 + np.abs(ref["loss3"]))).all()
            for k in ("dlogits", "dvlogit"):
                assert np.abs(got[k] - ref[k]).max() <= 1e-4 * np.abs(ref[k]).max() + 1e-6
            assert lb.positive_zero(got["probs"][occ]) and lb.positive_zero(got["dlogits"][occ])
            free = ~occ.all(axis=1)
            # the outputs-only unmasked call on logits whose occupied cells are -inf: the same probs, bit for bit
            if free.any():
                neg = np.where(occ, np.float32(-np.inf), args[0]).astype(np.float32)[free]
                plain = run_loss((neg, args[1][free]), occ=False, grads=False)
                same_bits(got["probs"][free], plain["probs"], "probs against -inf logits")
            # whatever the occupied logits hold changes no output bit
            for junk in (np.nan, np.inf, -np.inf, 1e30):
                other = run_loss((np.where(occ, np.float32(junk), args[0]).astype(np.float32),) + args[1:])
                for k in got:
                    same_bits(got[k], other[k], "%s with %r on the stones" % (k, junk))
    print("n %d hw %d masked loss kernel error / bar: %s" % (n, hw, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("hw", lb.HWS)
@pytest.mark.parametrize("n", lb.NS)
def test_masked_loss_on_degenerate_boards(n, hw):
    logits, u, pi, z = hb.loss_batch("randn30", "dirichlet", n, hw, 5)
    # no stone: the unmasked call's bits in every output
    none = np.zeros((n, hw), np.uint8)
    a, b = run_loss((logits, u, pi, z, none)), run_loss((logits, u, pi, z), occ=False)
    assert set(a) == set(b) == {"loss3", "dlogits", "dvlogit", "probs", "values"}
    for k in a:
        same_bits(a[k], b[k], "no stone: " + k)
    same_bits(run_loss((logits, u, pi, z, none), grads=False)["probs"], b["probs"])
    # a single empty cell: p == 1, ce == 0, ent == 0
    one = np.stack([lb.occupancy_row(np.random.RandomState(hw + i), "all_but_one", hw) for i in range(n)])
    pi1 = (one == 0).astype(np.float32)
    got = run_loss((logits, u, pi1, z, one))
    assert (got["probs"][one == 0] == 1).all() and lb.positive_zero(got["probs"][one != 0])
    assert got["loss3"][1] == 0 and got["loss3"][2] == 0 and not got["dlogits"].any() and lb.positive_zero(got["dlogits"][one != 0])
    # no empty cell: all zeros, finite
    got = run_loss((logits, u, pi, z, np.ones((n, hw), np.uint8)))
    assert all(np.isfinite(v).all() for v in got.values())
    assert lb.positive_zero(got["probs"]) and lb.positive_zero(got["dlogits"]) and got["loss3"][1] == 0 and got["loss3"][2] == 0
    same_bits(got["values"], b["values"])
    same_bits(got["dvlogit"], b["dvlogit"])
    same_bits(got["loss3"][:1], b["loss3"][:1])


# ---- 2. the evaluator
ENGINES = {"r15": dict(side=15, kind="resnet", blocks=1), "f9": dict(side=9, kind="resnet", blocks=1),
           "s8": dict(side=8, kind="simple", blocks=0)}
NMAX = 33


def make(name, batch=64, prm=None, **kw):
    from alphapig_amd.policy_value_net import PolicyValueNet
    cfg = ENGINES[name]
    kw.setdefault("trunk_arith", "f32")         # one kernel family for every batch size: a row's bits do not depend on n
    prm = prm or weights.init_params(cfg["kind"], cfg["side"], cfg["side"], 9, cfg["blocks"], 128, seed=5, style="bench")
    return PolicyValueNet(cfg["side"], cfg["side"], batch_size=batch, n_blocks=cfg["blocks"], n_filter=128, model_params=prm,
                          net_kind=cfg["kind"], **kw)


@pytest.fixture(scope="module")
def labs():
    """name -> (net with the switch ON, codes and planes of NMAX positions, the switch-off forward of all of them, the
    switch-on forward of all of them): one engine per net, every reference computed once"""
    made = {}

    def get(name):
        if name not in made:
            side = ENGINES[name]["side"]
            codes = positions(side)[:NMAX]
            planes = planes_of(codes, side, 9)
            net = make(name)
            off = net.forward_with_logits(planes)
            assert net.L.apz_get_legal_policy(net._h) == 0
            net.set_legal_policy(True)
            assert net.L.apz_get_legal_policy(net._h) == 1 and net.legal_policy
            made[name] = (net, codes, planes, off, net.forward_with_logits(planes))
        return made[name]
    yield get
    for lab in made.values():
        lab[0].close()


@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_every_entry_point_gives_the_masked_rows(labs, name, n):
    net, codes, planes, off, on = labs(name)
    codes, planes = codes[:n], planes[:n]
    hw = net.hw
    occ = codes[:, :hw] != 0
    logits, probs, vlog, vals = net.forward_with_logits(planes)                     # apz_forward
    # against the float64 softmax over the empty cells of the engine's own logits, at the inference bar (cut at 2e-5)
    bar, sum_bar = lb.legal_softmax_bar(logits, occ)
    q = hb.ratio(probs, lb.legal_softmax64(logits, occ)[0], bar)
    qs = hb.ratio(probs.astype(np.float64).sum(axis=1), 1.0, sum_bar)
    print("%s n %d: masked probs error / bar %.3f, row sum %.3f; stones per board %d .. %d" % (
        name, n, q, qs, occ.sum(axis=1).min(), occ.sum(axis=1).max()))
    assert q <= 1.0 and qs <= 1.0 and (bar <= hb.CAP_INFER).all()
    assert lb.positive_zero(probs[occ]) and (probs[~occ] > 0).all()
    # the rows do not depend on n; logits and values are the switch-off forward's
    same_bits(probs, on[1][:n], "rows of a forward of %d against a forward of %d" % (n, NMAX))
    same_bits(logits, off[0][:n])
    same_bits(vlog, off[2][:n])
    same_bits(vals, off[3][:n], "values")
    assert (off[1][:n][occ] > 0).all()                             # where the switch-off policy puts mass on the stones
    same_bits(probs[0], off[1][0], "the empty board")              # positions()[0]: no stone, the switch-off bits
    # every other entry point: the same bits
    p, v = net.forward_planes(planes)                                               # apz_forward_host
    same_bits(p, probs, "forward_planes")
    same_bits(v, vals)
    p, v = net.policy_value_dev(torch.as_tensor(planes).cuda())                     # apz_forward_dev_host
    same_bits(p, probs, "policy_value_dev")
    p, v = net.evaluate_codes(codes)                                                # apz_forward_codes_host
    same_bits(p, probs, "evaluate_codes")
    same_bits(v, vals)
    p, v = evaluate_async(net, codes)                                               # apz_forward_codes_async
    same_bits(p, probs, "async")
    for slot in (0, 2):                                                             # apz_submit_codes / apz_wait
        p, v = net.wait_slot(slot, net.submit_codes_slot(slot, codes))
        same_bits(p, probs, "slot %d" % slot)
        same_bits(v, vals)


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_switch_off_after_on_restores_the_old_bits(labs, name):
    net, codes, planes, off, on = labs(name)
    try:
        net.set_legal_policy(False)
        for got, want in zip(net.forward_with_logits(planes), off):
            same_bits(got, want)
        same_bits(net.evaluate_codes(codes)[0], off[1])
        same_bits(net.wait_slot(1, net.submit_codes_slot(1, codes))[0], off[1])
    finally:
        net.set_legal_policy(True)
    same_bits(net.evaluate_codes(codes)[0], on[1])


def test_the_switch_survives_weight_loads(labs):
    net, codes, planes, off, on = labs("r15")
    prm = net.params()
    net.set_params(prm)
    assert net.L.apz_get_legal_policy(net._h) == 1
    same_bits(net.evaluate_codes(codes)[0], on[1])
    dev = {k: torch.as_tensor(v).cuda() for k, v in prm.items()}
    torch.cuda.synchronize()
    net.load_device_params(dev)
    net.sync()
    same_bits(net.wait_slot(0, net.submit_codes_slot(0, codes))[0], on[1])


def test_graph_replay_gives_the_plain_bits(labs):
    net, codes, planes, off, on = labs("r15")
    shapes = [(0, 0, 1), (1, 3, 7), (2, 0, 33)]

    def run(slot, lo, n):
        p, v = net.wait_slot(slot, net.submit_codes_slot(slot, codes[lo:lo + n]))
        return np.array(p, copy=True), np.array(v, copy=True)
    try:
        net._ck(net.L.apz_set_forward_graphs(net._h, 1))
        for rep in range(5):                                    # submissions 1, 2: plain; 3: captured + launched; 4 ..: replayed
            for s in shapes:
                p, v = run(*s)
                same_bits(p, on[1][s[1]:s[1] + s[2]], "graphs on, submission %d of %s" % (rep + 1, s))
                same_bits(v, on[3][s[1]:s[1] + s[2]])
        p, _ = run(1, 10, 7)                                    # the replayed graph reads the slot's codes: other stones, other mask
        same_bits(p, on[1][10:17])
        net.set_legal_policy(False)                             # drops the graphs: the next submissions run the other heads
        for rep in range(4):
            same_bits(run(1, 3, 7)[0], off[1][3:10], "switch off under graphs")
        net.set_legal_policy(True)
        for rep in range(4):
            same_bits(run(1, 3, 7)[0], on[1][3:10], "switch on again under graphs")
    finally:
        net._ck(net.L.apz_set_forward_graphs(net._h, 0))
        net.set_legal_policy(True)


def test_the_exact_repeat_of_an_overflowed_batch_returns_masked_rows():
    """The FullyConnected parameters scaled as tests/test_gpu_head_edges.py scales them (f = 30: a peaked policy) and a stem
    whose outputs leave the fp16 range (tests/test_gpu_net.py: res_conv1_weight x 3e4): the f16x2 forward of 33 boards
    overflows, the entry point repeats it on the exact kernel, and the repeat goes through the masked head"""
    from test_gpu_head_edges import scaled
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=41, style="bench")
    big = scaled(prm, 30)
    big["res_conv1_weight"] = np.asarray(prm["res_conv1_weight"], np.float32) * 3.0e4
    codes = positions(15)[:NMAX]
    occ = codes[:, :225] != 0
    exact, split = make("r15", prm=big, legal_policy=True), make("r15", prm=big, trunk_arith="f16x2", legal_policy=True)
    try:
        want = exact.evaluate_codes(codes)
        assert lb.positive_zero(want[0][occ]) and np.abs(want[0].astype(np.float64).sum(axis=1) - 1).max() <= 2e-5
        count = 0
        for entry in ("slot", "host", "planes"):
            if entry == "slot":
                got = split.wait_slot(1, split.submit_codes_slot(1, codes))
            elif entry == "host":
                got = split.evaluate_codes(codes)
            else:
                got = split.forward_planes(planes_of(codes, 15, 9))
            count += 1
            assert split.trunk_overflows() == count, entry
            assert np.isfinite(got[0]).all() and lb.positive_zero(got[0][occ])
            same_bits(got[0], want[0], entry)
            same_bits(got[1], want[1], entry)
    finally:
        exact.close()
        split.close()


# ---- 3. leaf symmetry
def test_keyed_is_the_masked_answer_on_the_image_folded_back(labs):
    net, codes, planes, off, on = labs("r15")
    occ = codes[:, :225] != 0
    ks = leaf_symmetry_keys(codes, SEED)
    assert len(set(ks.tolist())) >= 4
    img = images(codes, 15, ks)
    q, w = net.evaluate_codes(img)                               # symmetry off, switch on: masked by the images' own stones
    try:
        net.set_leaf_symmetry("keyed", SEED)
        for entry in ("host", "slot"):
            p, v = net.evaluate_codes(codes) if entry == "host" else net.wait_slot(0, net.submit_codes_slot(0, codes))
            same_bits(p, fold(q, 15, ks), "keyed, " + entry)
            same_bits(v, w)
            assert lb.positive_zero(p[occ]) and (p[~occ] > 0).all()
    finally:
        net.set_leaf_symmetry("none", SEED)


def test_mean8_rows_are_zero_on_the_positions_stones_and_sum_to_one():
    net = make("r15", batch=8, leaf_symmetry="mean8", legal_policy=True)
    try:
        codes = positions(15)[:8]
        occ = codes[:, :225] != 0
        for entry in ("host", "slot"):
            p, v = net.evaluate_codes(codes) if entry == "host" else net.wait_slot(0, net.submit_codes_slot(0, codes))
            assert np.isfinite(p).all() and lb.positive_zero(p[occ]) and (p[~occ] > 0).all()
            assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 8 * 2e-5
    finally:
        net.close()


# ---- 4. self-play
def test_selfplay_does_not_depend_on_the_games_in_flight_and_every_evaluated_row_is_masked():
    from alphapig_amd.selfplay import SelfPlayEngine
    net = make("r15", batch=16, legal_policy=True)
    seen = {"rows": 0, "stones": 0}

    def tap(ids, codes, p, v):
        occ = codes[:, :225] != 0
        assert lb.positive_zero(p[occ]) and np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 2e-5
        seen["rows"] += len(ids)
        seen["stones"] += int(occ.sum())

    def play(concurrent, tap=None):
        eng = SelfPlayEngine(net, 15, 15, 5, n_games=concurrent, n_playout=16, c_puct=5, temp=1.0, base_seed=77, n_threads=4,
                             forced_opening=True)
        eng.tap = tap
        try:
            return {e.index: e for e in eng.play_games(8)}
        finally:
            eng.close()
    try:
        eight, three = play(8, tap), play(3)
        assert sorted(eight) == sorted(three) == list(range(8))
        for k in range(8):
            np.testing.assert_array_equal(eight[k].moves, three[k].moves)
            np.testing.assert_array_equal(eight[k].pis, three[k].pis)
            assert eight[k].winner == three[k].winner
        print("self-play, legal policy: %d evaluated rows, %d stones under them; games of %s plies"
              % (seen["rows"], seen["stones"], [len(eight[k].moves) for k in range(8)]))
        assert seen["rows"] > 200 and seen["stones"] > seen["rows"]
    finally:
        net.close()
