"""Dihedral leaf symmetry of the evaluator on the GPU (apz_set_leaf_symmetry, csrc/leaf_sym.h): "keyed" and "mean8" against
what a mode-none engine answers on host-built images (bit for bit), against the float64 oracle evaluated on the images and
folded in float64 (the bars tests/test_gpu_net.py holds probabilities and values to: 2e-5), and through the entry points,
HIP graphs, the overflow repeat, a weight refresh, the refusals and self-play.

Image k of a code row and folding back are restated here from the tables of alphapig_amd.augment; nothing below reads
what the kernels computed to decide what they should have computed."""
import ctypes as C
import functools

import numpy as np
import pytest

from alphapig_amd import weights
from alphapig_amd.augment import dihedral_tables, leaf_symmetry_keys
from alphapig_amd.policy_value_net import EvaluatorError, PolicyValueNet
from oracle import net_ref

pytestmark = pytest.mark.gpu

BAR = 2e-5              # tests/test_gpu_net.py: probabilities and values against the float64 oracle
SEED = 0x5EED0F1EAF
BATCH = 96              # max_batch of the shared engines: 65 boards keyed, 12 positions (96 boards) under mean8
N_ORACLE = 12           # positions held against the oracle: the empty board, a lone corner stone, ten random ones

# name -> (board side, net kind, residual blocks, filters, c_in, trunk_arith, uniform_trunk)
ENGINES = {
    "r15-f32": (15, "resnet", 2, 128, 9, "f32", False),
    "r15-auto": (15, "resnet", 2, 128, 9, "auto", False),
    "r15-uniform": (15, "resnet", 2, 128, 9, "auto", True),
    "r15-64": (15, "resnet", 1, 64, 9, "auto", False),        # its first layer does not take codes: apz_encode_planes
    "s8": (8, "simple", 0, 64, 9, "auto", False),
    "r8-128": (8, "resnet", 1, 128, 9, "auto", False),
    "f9": (9, "resnet", 1, 128, 9, "auto", False),
    "f6": (6, "resnet", 1, 128, 9, "auto", False),
    "r15-c4": (15, "resnet", 1, 128, 4, "auto", False),
}
ALL = [n for n in ENGINES if n != "r15-uniform"]


@functools.lru_cache(maxsize=None)
def params(name):
    """With init_params weights the policy hardly depends on the position: its shape is the head's, and how far the eight
    folded policies lie apart is a property of the seed (from 7e-4 to 3e-2 on the 15x15 net).  Seed 5 keeps them more
    than 1e-3 apart on every position used, for every net here (asserted on the float64 oracle: oracle_folded)."""
    side, kind, blocks, filt, c_in, _, _ = ENGINES[name]
    return weights.init_params(kind, side, side, c_in, blocks, filt, seed=5, style="bench")


def make(name, batch=BATCH, prm=None, **kw):
    side, kind, blocks, filt, c_in, arith, uniform = ENGINES[name]
    return PolicyValueNet(side, side, batch_size=batch, n_blocks=blocks, n_filter=filt, model_params=prm or params(name),
                          net_kind=kind, c_in=c_in, trunk_arith=arith, uniform_trunk=uniform, **kw)


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(name):
        if name not in made:
            made[name] = make(name)
        made[name].set_leaf_symmetry("none", SEED)
        return made[name]
    yield get
    for net in made.values():
        net.close()


@functools.lru_cache(maxsize=None)
def positions(side):
    """-> codes uint8 [65, stride]: the empty board, a lone corner stone, then random positions of 0 .. 40 plies"""
    from alphapig_amd.treepool import TreePool
    hw = side * side
    pool = TreePool(side, side, 4 if side < 9 else 5, n_games=1, n_playout=1)
    rs = np.random.RandomState(500 + side)
    cells = [[], [0]] + [list(rs.permutation(hw)[:int(rs.randint(0, min(41, hw)))]) for _ in range(63)]
    codes = []
    for c in cells:
        k = len(c)
        pool.set_position(0, c, [1 + (i % 2) for i in range(k)], 1 + (k % 2))
        codes.append(pool.codes(0))
    pool.close()
    codes = np.stack(codes)
    codes.setflags(write=False)
    return codes


def planes_of(codes, side, c_in):
    from alphapig_amd.treepool import TreePool
    pool = TreePool(side, side, 4 if side < 9 else 5, n_games=1, n_playout=1)
    try:
        return pool.codes_to_planes(codes, c_in)
    finally:
        pool.close()


def images(codes, side, ks):
    """row b -> its image ks[b]: codes_k[p] = codes[perm_p[k][p]], the colour byte copied, pad bytes 0"""
    hw = side * side
    pp = dihedral_tables(side)[1]
    out = np.zeros_like(codes)
    for b, k in enumerate(ks):
        out[b, :hw] = codes[b, pp[k]]
    out[:, hw] = codes[:, hw]
    return out


def images8(codes, side):
    """board b -> rows 8b .. 8b + 7, image k in row 8b + k"""
    return images(np.repeat(codes, 8, axis=0), side, np.tile(np.arange(8), len(codes)))


def fold(q, side, ks):
    """the net answered q[b] on image ks[b]: probs[perm_p[k][p]] = q[p]"""
    pp = dihedral_tables(side)[1]
    out = np.empty_like(q)
    for b, k in enumerate(ks):
        out[b, pp[k]] = q[b]
    return out


def mean8_restated(q, v, side):
    """fp32: 0.125f * (((((((u_0 + u_1) + u_2) + u_3) + u_4) + u_5) + u_6) + u_7), the value from the eight values likewise"""
    n = len(q) // 8
    assert q.dtype == np.float32 and v.dtype == np.float32
    u = fold(q, side, np.tile(np.arange(8), n)).reshape(n, 8, -1)
    w = v.reshape(n, 8)
    s, t = u[:, 0].copy(), w[:, 0].copy()
    for k in range(1, 8):
        s = s + u[:, k]
        t = t + w[:, k]
    assert s.dtype == np.float32 and t.dtype == np.float32
    return np.float32(0.125) * s, np.float32(0.125) * t


def evaluate(net, entry, codes):
    if entry == "host":
        p, v = net.evaluate_codes(codes)
    else:
        slot = int(entry[4:])
        p, v = net.wait_slot(slot, net.submit_codes_slot(slot, codes))
    return np.array(p, copy=True), np.array(v, copy=True)


def evaluate_async(net, codes):
    """apz_forward_codes_async on pinned buffers, then apz_sync"""
    L, n = net.L, len(codes)
    sizes = (codes.nbytes, n * net.hw * 4, n * 4)
    bufs = [L.apz_host_alloc(s) for s in sizes]
    assert all(bufs)
    try:
        C.memmove(bufs[0], np.ascontiguousarray(codes).ctypes.data, sizes[0])
        net._ck(L.apz_forward_codes_async(net._h, bufs[0], n, bufs[1], bufs[2]))
        net.sync()
        p = np.frombuffer((C.c_float * (n * net.hw)).from_address(bufs[1]), np.float32).reshape(n, net.hw).copy()
        v = np.frombuffer((C.c_float * n).from_address(bufs[2]), np.float32).copy()
        return p, v
    finally:
        for b in bufs:
            L.apz_host_free(b)


@functools.lru_cache(maxsize=None)
def oracle_folded(name):
    """float64 oracle on the eight images of the first N_ORACLE positions, folded in float64 -> (F [n, 8, hw], V [n, 8])"""
    side, kind, blocks, _, c_in, _, _ = ENGINES[name]
    codes = positions(side)[:N_ORACLE]
    o = net_ref.forward(params(name), planes_of(images8(codes, side), side, c_in), kind, blocks, np.float64)
    F = fold(np.asarray(o[1], np.float64), side, np.tile(np.arange(8), N_ORACLE)).reshape(N_ORACLE, 8, -1)
    V = np.asarray(o[3], np.float64)[:, 0].reshape(N_ORACLE, 8)
    # the precondition of every oracle comparison below: on EVERY position used the eight folded policies differ pairwise by
    # more than 1e-3 somewhere -- otherwise a wrong k, or perm_s in place of perm_p, could hide under the bar
    gaps = np.array([[[np.abs(F[b, j] - F[b, k]).max() for k in range(8)] for j in range(8)] for b in range(N_ORACLE)])
    smallest = gaps[:, ~np.eye(8, dtype=bool)].min()
    print("%s: smallest pairwise gap of the folded oracle policies on any position %.3e" % (name, smallest))
    assert smallest > 1e-3, gaps.min(axis=0)
    return F, V


# ---- 1. bits, keyed
@pytest.mark.parametrize("name", ALL)
def test_keyed_carries_the_bits_of_a_plain_forward_on_the_images(nets, name):
    net, side = nets(name), ENGINES[name][0]
    codes = positions(side)
    seen = set()
    for n in (1, 3, 33, 65):
        ks = leaf_symmetry_keys(codes[:n], SEED)
        seen |= set(ks.tolist())
        img = images(codes[:n], side, ks)
        for entry in ("host", "slot0", "slot3"):
            net.set_leaf_symmetry("none")
            p0, v0 = evaluate(net, entry, img)              # the same n, the same row order: the forward's input bytes
            net.set_leaf_symmetry("keyed", SEED)
            assert (net.leaf_symmetry, net.symmetry_seed) == ("keyed", SEED)
            p1, v1 = evaluate(net, entry, codes[:n])
            np.testing.assert_array_equal(p1, fold(p0, side, ks), err_msg="%s n %d %s" % (name, n, entry))
            np.testing.assert_array_equal(v1, v0)
            assert np.isfinite(p1).all() and np.abs(p1.sum(axis=1) - 1).max() < 1e-5
    assert seen == set(range(8))                            # every image was used, the identity among them
    net.set_leaf_symmetry("none")
    p0, v0 = evaluate_async(net, img)
    net.set_leaf_symmetry("keyed", SEED)
    p1, v1 = evaluate_async(net, codes[:65])
    np.testing.assert_array_equal(p1, fold(p0, side, ks))
    np.testing.assert_array_equal(v1, v0)
    # another seed, other images: the engine follows leaf_symmetry_keys there too
    net.set_leaf_symmetry("keyed", SEED + 1)
    ks2 = leaf_symmetry_keys(codes[:33], SEED + 1)
    assert (ks2 != ks[:33]).any()
    p2, _ = evaluate(net, "host", codes[:33])
    net.set_leaf_symmetry("none")
    np.testing.assert_array_equal(p2, fold(evaluate(net, "host", images(codes[:33], side, ks2))[0], side, ks2))
    mode, seed = C.c_int32(-1), C.c_uint64(0)
    net._ck(net.L.apz_get_leaf_symmetry(net._h, C.byref(mode), C.byref(seed)))
    assert (mode.value, seed.value) == (0, SEED + 1)


# ---- 2. bits, mean8
@pytest.mark.parametrize("name", ALL)
def test_mean8_is_the_fp32_fold_of_a_plain_forward_on_the_eight_images(nets, name):
    net, side = nets(name), ENGINES[name][0]
    codes = positions(side)
    for n in (1, 4, 5):                                     # 8, 32 and 40 boards: both routes under "auto"
        img = images8(codes[2:2 + n], side)
        for entry in ("host", "slot1"):
            net.set_leaf_symmetry("none")
            q, v = evaluate(net, entry, img)
            net.set_leaf_symmetry("mean8")
            p1, v1 = evaluate(net, entry, codes[2:2 + n])
            want_p, want_v = mean8_restated(q, v, side)
            np.testing.assert_array_equal(p1, want_p, err_msg="%s n %d %s" % (name, n, entry))
            np.testing.assert_array_equal(v1, want_v)
    net.set_leaf_symmetry("none")
    q, v = evaluate_async(net, img)
    net.set_leaf_symmetry("mean8")
    p1, v1 = evaluate_async(net, codes[2:7])
    np.testing.assert_array_equal(p1, mean8_restated(q, v, side)[0])
    np.testing.assert_array_equal(v1, mean8_restated(q, v, side)[1])


# ---- 3. oracle
@pytest.mark.parametrize("name", ALL)
def test_keyed_and_mean8_against_the_float64_oracle(nets, name):
    net, side = nets(name), ENGINES[name][0]
    codes = positions(side)[:N_ORACLE]
    F, V = oracle_folded(name)
    ks = leaf_symmetry_keys(codes, SEED)
    rows = np.arange(N_ORACLE)
    for entry in ("host", "slot2"):
        net.set_leaf_symmetry("keyed", SEED)
        p, v = evaluate(net, entry, codes)
        ep, ev = np.abs(p - F[rows, ks]).max(), np.abs(v - V[rows, ks]).max()
        net.set_leaf_symmetry("mean8")
        pm, vm = evaluate(net, entry, codes)
        em, evm = np.abs(pm - F.mean(axis=1)).max(), np.abs(vm - V.mean(axis=1)).max()
        print("%s %s: keyed probs %.2e values %.2e; mean8 probs %.2e values %.2e" % (name, entry, ep, ev, em, evm))
        assert ep <= BAR and ev <= BAR and em <= BAR and evm <= BAR
    # what the precondition is for: the identity's answer is far outside the bar
    moved = ks != 6
    assert moved.any() and np.abs(F[rows, 6] - F[rows, ks])[moved].max() > 1e-3


# ---- 4. equivariance of mean8
@pytest.mark.parametrize("name", ["r15-auto", "r15-64", "s8", "f9", "f6"])
def test_mean8_is_equivariant(nets, name):
    net, side = nets(name), ENGINES[name][0]
    n = 6
    codes = positions(side)[:n]
    F, V = oracle_folded(name)
    M, W = F[:n].mean(axis=1), V[:n].mean(axis=1)           # the oracle's mean: exactly equivariant
    pp = dihedral_tables(side)[1]
    net.set_leaf_symmetry("mean8")
    p, v = evaluate(net, "host", codes)
    assert np.abs(p - M).max() <= BAR and np.abs(v - W).max() <= BAR
    worst = 0.0
    for j in range(8):
        pj, vj = evaluate(net, "slot0" if j % 2 else "host", images(codes, side, [j] * n))
        # the image's policy is the position's, permuted like its pi: P_j[q] = P[perm_p[j][q]]
        worst = max(worst, np.abs(pj - p[:, pp[j]]).max(), np.abs(vj - v).max())
        assert np.abs(pj - p[:, pp[j]]).max() <= 2 * BAR and np.abs(vj - v).max() <= 2 * BAR, j
        assert np.abs(pj - M[:, pp[j]]).max() <= BAR and np.abs(vj - W).max() <= BAR, j
    print("%s: mean8 on the eight images against the permuted mean8 answer: %.2e" % (name, worst))


# ---- 5. a keyed answer depends on the position only
@pytest.mark.parametrize("name", ["r15-f32", "r15-uniform"])
def test_a_keyed_answer_does_not_depend_on_row_batch_or_slot(nets, name):
    net, side = nets(name), 15
    codes = positions(side)
    x = codes[7:8]
    net.set_leaf_symmetry("keyed", SEED)
    first3 = np.concatenate([x, codes[20:22]])
    last3 = np.concatenate([codes[20:22], x])
    last7 = np.concatenate([codes[30:36], x])
    first7 = np.concatenate([x, codes[30:36]])
    last40 = np.concatenate([codes[10:49], x])              # beyond the small-batch kernels
    ref_p, ref_v = evaluate(net, "slot0", first3)
    ref_p, ref_v = ref_p[0], ref_v[0]
    for entry in ("slot0", "slot1", "slot2", "slot3", "host"):
        for batch, row in ((first3, 0), (last3, 2), (last7, 6), (first7, 0), (x, 0), (last40, 39)):
            p, v = evaluate(net, entry, batch)
            np.testing.assert_array_equal(p[row], ref_p, err_msg="%s, %d boards, row %d" % (entry, len(batch), row))
            np.testing.assert_array_equal(v[row], ref_v)
    assert net.trunk_overflows() == 0


# ---- 6. HIP graphs
@pytest.mark.parametrize("name", ["r15-auto", "f9", "s8"])
def test_graph_replay_gives_the_plain_bits(nets, name):
    net, side = nets(name), ENGINES[name][0]
    codes = positions(side)
    for mode in ("keyed", "mean8"):
        net._ck(net.L.apz_set_forward_graphs(net._h, 0))
        net.set_leaf_symmetry(mode, SEED)
        plain = evaluate(net, "slot1", codes[3:6])
        other = evaluate(net, "slot1", codes[40:43])
        net._ck(net.L.apz_set_forward_graphs(net._h, 1))
        try:
            for rep in range(5):                            # submissions 1, 2: plain; 3: captured and launched; then replayed
                p, v = evaluate(net, "slot1", codes[3:6])
                np.testing.assert_array_equal(p, plain[0], err_msg="%s submission %d" % (mode, rep + 1))
                np.testing.assert_array_equal(v, plain[1])
            p, v = evaluate(net, "slot1", codes[40:43])     # the replayed graph reads the slot's buffer: other positions
            np.testing.assert_array_equal(p, other[0])
            np.testing.assert_array_equal(v, other[1])
            net.set_leaf_symmetry(mode, SEED + 9)           # the setter drops the graphs: a capture never outlives its seed
            moved = evaluate(net, "slot1", codes[3:6])
            net.set_leaf_symmetry(mode, SEED)
            for rep in range(5):
                p, v = evaluate(net, "slot1", codes[3:6])
                np.testing.assert_array_equal(p, plain[0], err_msg="%s submission %d after the seed came back" % (mode, rep + 1))
                np.testing.assert_array_equal(v, plain[1])
            if mode == "keyed":
                k0, k9 = leaf_symmetry_keys(codes[3:6], SEED), leaf_symmetry_keys(codes[3:6], SEED + 9)
                assert (k0 != k9).any() == (not np.array_equal(moved[0], plain[0]))
        finally:
            net._ck(net.L.apz_set_forward_graphs(net._h, 0))


# ---- 7. the overflow repeat
def test_mean8_overflow_is_repeated_on_the_exact_kernel():
    """the recipe of tests/test_gpu_net.py::test_f16x2_overflow_repeats_the_forward_on_the_exact_kernel: stem outputs in the
    tens of thousands.  Five positions under mean8 are a 40-board forward: the f16x2 kernel, which overflows."""
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=41, style="bench")
    big = dict(prm)
    big["res_conv1_weight"] = np.asarray(prm["res_conv1_weight"], np.float32) * 3.0e4
    mk = lambda arith: PolicyValueNet(15, 15, batch_size=8, n_blocks=2, n_filter=128, model_params=big, trunk_arith=arith,
                                      leaf_symmetry="mean8", symmetry_seed=SEED)
    exact, split = mk("f32"), mk("f16x2")
    try:
        assert split.batchsize == 8 and split.trunk_overflows() == 0
        codes = positions(15)[2:7]
        for i, entry in enumerate(("host", "slot0", "slot0", "slot0", "slot3")):
            a, b = evaluate(exact, entry, codes), evaluate(split, entry, codes)
            assert split.trunk_overflows() == i + 1 and exact.trunk_overflows() == 0
            assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all()
            np.testing.assert_array_equal(a[0], b[0], err_msg=entry)
            np.testing.assert_array_equal(a[1], b[1])
        # four positions are 32 boards: the exact small-batch kernel, nothing to repeat
        a, b = evaluate(exact, "host", codes[:4]), evaluate(split, "host", codes[:4])
        assert split.trunk_overflows() == 5
        np.testing.assert_array_equal(a[0], b[0])
    finally:
        exact.close()
        split.close()


# ---- 8. one weight version per answer
@pytest.mark.parametrize("mode", ["keyed", "mean8"])
def test_a_submitted_batch_is_answered_with_the_weights_it_was_submitted_under(mode):
    old = params("r15-auto")
    new = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=99, style="bench")
    net = make("r15-auto", batch=40)
    try:
        net.set_leaf_symmetry(mode, SEED)
        codes = positions(15)[:5]
        want_old = evaluate(net, "slot0", codes)
        n = net.submit_codes_slot(0, codes)
        net.set_params(new)
        got = net.wait_slot(0, n)
        np.testing.assert_array_equal(got[0], want_old[0])
        np.testing.assert_array_equal(got[1], want_old[1])
        fresh = evaluate(net, "slot0", codes)
        assert np.abs(fresh[0] - want_old[0]).max() > 1e-3   # ... and the next one with the new ones
        twin = make("r15-auto", batch=40, prm=new, leaf_symmetry=mode, symmetry_seed=SEED)
        try:
            np.testing.assert_array_equal(evaluate(twin, "slot0", codes)[0], fresh[0])
        finally:
            twin.close()
    finally:
        net.close()


# ---- 9. refusals
def test_refusals_carry_a_message(nets):
    net = make("f9", batch=16)
    codes = positions(9)
    try:
        assert net.L.apz_set_leaf_symmetry(net._h, 3, 0) == -1           # APZ_E_ARG
        assert b"mode" in net.L.apz_last_error() and b"3" in net.L.apz_last_error()
        assert net.L.apz_set_leaf_symmetry(net._h, -1, 0) == -1
        net.set_leaf_symmetry("mean8")                      # created without it: max_batch stays 16, two positions per forward
        with pytest.raises(EvaluatorError, match="max_batch"):
            net.submit_codes_slot(0, codes[:3])             # 24 boards
        p = np.empty((3, net.hw), np.float32)
        v = np.empty(3, np.float32)
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        three = np.ascontiguousarray(codes[:3])
        rc = net.L.apz_forward_codes_host(net._h, three.ctypes.data_as(u8), 3, p.ctypes.data_as(fp), v.ctypes.data_as(fp))
        assert rc == -1 and b"mean8" in net.L.apz_last_error() and b"max_batch" in net.L.apz_last_error()
        with pytest.raises(EvaluatorError, match="nothing submitted"):
            net.wait_slot(0, 3)                             # the refused submission left the slot free
        pa, va = net.evaluate_codes(codes[:5])              # the Python mirror splits: 2 + 2 + 1 positions
        pb, vb = evaluate(net, "slot0", codes[:2])
        np.testing.assert_array_equal(pa[:2], pb)
        # the setter while a slot is in flight
        n = net.submit_codes_slot(1, codes[:2])
        with pytest.raises(EvaluatorError, match="in flight"):
            net.set_leaf_symmetry("keyed", 5)
        assert net.leaf_symmetry == "mean8"
        p1, _ = net.wait_slot(1, n)
        np.testing.assert_array_equal(p1, pb)
        net.set_leaf_symmetry("keyed", 5)
        with pytest.raises(ValueError):
            net.set_leaf_symmetry("keyed9")
        assert net.leaf_symmetry == "keyed"
    finally:
        net.close()
    # at construction: max_batch = 8 * batch_size, batchsize stays the caller's
    net = make("f9", batch=4, leaf_symmetry="mean8")
    try:
        assert net.batchsize == 4 and net._max_batch == 32
        p, v = evaluate(net, "slot0", codes[:4])
        with pytest.raises(EvaluatorError):
            net.submit_codes_slot(0, codes[:5])
        plain = nets("f9")
        q, w = evaluate(plain, "host", images8(codes[:4], 9))
        np.testing.assert_array_equal(p, mean8_restated(q, w, 9)[0])
    finally:
        net.close()


# ---- 10. self-play and a one-board player
def test_selfplay_keyed_depends_on_the_seed_only_and_a_mean8_player_finishes_a_game():
    from alphapig_amd.game import Board
    from alphapig_amd.mcts_alphaZero import MCTSPlayer
    from alphapig_amd.selfplay import SelfPlayEngine
    prm = weights.init_params("resnet", 15, 15, 9, 2, 128, seed=17, style="bench")
    net = PolicyValueNet(15, 15, batch_size=16, n_blocks=2, n_filter=128, model_params=prm, trunk_arith="f32",
                         leaf_symmetry="keyed", symmetry_seed=SEED)
    table = {}

    def play(concurrent, tap=None):
        eng = SelfPlayEngine(net, 15, 15, 5, n_games=concurrent, n_playout=24, c_puct=5, temp=1.0, base_seed=321, n_threads=4)
        eng.tap = tap
        try:
            return {e.index: e for e in eng.play_games(6)}
        finally:
            eng.close()

    def tap(ids, codes, p, v):
        for i in range(len(ids)):
            if len(table) < 48:
                table.setdefault(codes[i].tobytes(), (p[i].copy(), np.float32(v[i])))
    try:
        six, three = play(6, tap), play(3)
        assert sorted(six) == sorted(three) == list(range(6))
        for k in range(6):
            np.testing.assert_array_equal(six[k].moves, three[k].moves)
            np.testing.assert_array_equal(six[k].pis, three[k].pis)
            assert six[k].winner == three[k].winner
        # the tapped rows are folded answers: the float64 oracle on each position's keyed image, folded back
        rows = np.stack([np.frombuffer(k, np.uint8) for k in table])
        ks = leaf_symmetry_keys(rows, SEED)
        assert len(set(ks.tolist())) >= 4
        o = net_ref.forward(prm, planes_of(images(rows, 15, ks), 15, 9), "resnet", 2, np.float64)
        ep = np.abs(np.stack([t[0] for t in table.values()]) - fold(np.asarray(o[1]), 15, ks)).max()
        ev = np.abs(np.array([t[1] for t in table.values()]) - np.asarray(o[3])[:, 0]).max()
        print("self-play, keyed: %d tapped rows, probs %.2e values %.2e; games of %s plies"
              % (len(table), ep, ev, [len(six[k].moves) for k in range(6)]))
        assert ep <= BAR and ev <= BAR
        # a one-board player under mean8 (created keyed with batch_size 16: two positions per forward)
        net.set_leaf_symmetry("mean8")
        board = Board(width=15, height=15, n_in_row=5)
        board.init_board(0)
        player = MCTSPlayer(net.policy_value_fn, c_puct=5, n_playout=6, rng=np.random.RandomState(4))
        plies = 0
        while True:
            move = player.get_action(board)
            assert move in board.availables
            board.do_move(move)
            plies += 1
            end, winner = board.game_end()
            if end:
                break
        assert winner in (-1, board.players[0], board.players[1]) and 9 <= plies <= 225
        print("mean8 player: a game of %d plies, winner %s" % (plies, winner))
    finally:
        net.close()
