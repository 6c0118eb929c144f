"""Square boards of 6x6 .. 14x14 (other than 8x8 and 10x10) on the 15x15 trunk kernels: the "framed" engines of csrc/frame15.h,
through the C ABI and PolicyValueNet, against the float64 oracle (oracle/net_ref.py) on the S x S planes.

The board sits in the top-left S x S window of a 15x15 frame; frame_clear_kernel zeroes the off-board cells of every layer
but the last, so the frame's convolutions are the small board's (tests/test_frame_theory.py has the arithmetic).  Bars:
those of tests/test_gpu_net.py -- LOGIT_ATOL = 1e-4 on logits and value logits, 2e-5 on probabilities and values, 1e-4 /
2e-4 on the stem / last trunk layer -- and exact equality wherever two runs must carry the same bits.

Positions come from the host pool at size S: the empty board, the full board, the four corners, the whole last row and
last column, a single stone (so both colours are to move among them), then random legal positions.  The five special
boards lead the batch: a 5-board batch holds all of them."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import test_head_loss_bounds as hb
from alphapig_amd import weights
from alphapig_amd.selfplay import SelfPlayEngine
from oracle import net_ref, selfplay_ref
from oracle.board_ref import RefBoard
from oracle.mcts_ref import RefMCTSPlayer
from test_gpu_net import LOGIT_ATOL, random_positions
from test_gpu_selfplay import Never, Recorder, replay_fn

pytestmark = pytest.mark.gpu

NMAX = 70
N_BLOCKS = 3


def _pvn(side, prm, n_blocks=N_BLOCKS, batch=NMAX, c_in=9, **kw):
    from alphapig_amd.policy_value_net import PolicyValueNet
    return PolicyValueNet(side, side, batch_size=batch, n_blocks=n_blocks, n_filter=128, model_params=prm, c_in=c_in, **kw)


@functools.lru_cache(maxsize=None)
def positions(side, c_in=9):
    """-> (codes uint8 [70, stride], planes float32 [70, c_in, S, S]); read-only for the tests that share them"""
    from alphapig_amd.treepool import TreePool
    pool = TreePool(side, side, 4 if side < 9 else 5, n_games=1, n_playout=1)
    hw = side * side
    rs = np.random.RandomState(side)
    full = rs.permutation(hw)
    edge = sorted(set(range(hw - side, hw)) | set(range(side - 1, hw, side)))
    special = [[], list(full), [0, side - 1, hw - side, hw - 1], edge, [hw // 2]]
    codes = []
    for cells in special:
        k = len(cells)
        pool.set_position(0, cells, [1 + (i % 2) for i in range(k)], 1 + (k % 2))
        codes.append(pool.codes(0))
    codes = np.concatenate([np.stack(codes), random_positions(NMAX - len(special), side, c_in, seed=900 + side)[0]])
    planes = pool.codes_to_planes(codes, c_in)
    assert sorted(set(codes[:5, hw].tolist())) == [0, 1]            # both colours to move among the special boards
    stones = [6, 7] if c_in == 9 else [0, 1]                        # every own / every opposing stone
    assert planes[1, stones].sum() == hw and planes[0, :c_in - 1].sum() == 0   # the full and the empty board
    pool.close()
    codes.setflags(write=False)
    planes.setflags(write=False)
    return codes, planes


@functools.lru_cache(maxsize=None)
def params(side, c_in=9, n_blocks=N_BLOCKS):
    return weights.init_params("resnet", side, side, c_in, n_blocks, 128, seed=40 + side, style="bench")


@functools.lru_cache(maxsize=None)
def oracle(side, c_in=9):
    """float64 outputs of the 3-block net on all 70 boards: (logits, probs, value logit, value, (stem, trunk))"""
    return net_ref.forward(params(side, c_in), positions(side, c_in)[1], "resnet", N_BLOCKS, np.float64, True)


def check_heads(out, ref, n, tag=""):
    logits, probs, vlog, vals = out
    e = (np.abs(logits - ref[0][:n]).max(), np.abs(vlog - ref[2][:n, 0]).max(), np.abs(probs - ref[1][:n]).max(),
         np.abs(vals - ref[3][:n, 0]).max())
    print("%s n %d: logits %.2e value logit %.2e probs %.2e values %.2e" % ((tag, n) + e))
    assert e[0] <= LOGIT_ATOL and e[1] <= LOGIT_ATOL and e[2] <= 2e-5 and e[3] <= 2e-5


@pytest.fixture(scope="module")
def nets():
    """-> get(side, c_in=9, **kw): one engine per configuration for the whole module"""
    made = {}

    def get(side, c_in=9, **kw):
        key = (side, c_in) + tuple(sorted(kw.items()))
        if key not in made:
            select = kw.pop("select", None)
            made[key] = _pvn(side, params(side, c_in), c_in=c_in, **kw)
            if select is not None:
                made[key]._ck(made[key].L.apz_test_select_trunk(made[key]._h, select))
        return made[key]

    yield get
    for net in made.values():
        net.close()


# ---- 1. oracle parity
@pytest.mark.parametrize("n", [1, 5, 33, 70])
@pytest.mark.parametrize("side,c_in", [(6, 9), (7, 9), (9, 9), (13, 9), (14, 9), (9, 4)])
def test_framed_net_against_the_oracle(nets, side, c_in, n):
    net = nets(side, c_in, trunk_arith="f32")
    planes = positions(side, c_in)[1][:n]
    ref = oracle(side, c_in)
    out = net.forward_with_logits(planes)
    check_heads(out, ref, n, "%dx%d c_in %d" % (side, side, c_in))
    assert np.abs(out[1].sum(axis=1) - 1).max() < 1e-5
    p2, v2 = net.forward_planes(planes)
    np.testing.assert_array_equal(p2, out[1])
    np.testing.assert_array_equal(v2, out[3])
    stem, trunk = ref[4]
    np.testing.assert_allclose(net.layer_output(0, n), stem[:n], rtol=0, atol=1e-4)
    np.testing.assert_allclose(net.layer_output(2 * N_BLOCKS, n), trunk[:n], rtol=0, atol=2e-4)


def test_framed_net_of_10_blocks_13x13():
    prm = params(13, 9, 10)
    planes = positions(13)[1]
    rows = [0, 1, 2, 3, 4, 31, 32, 33, 68, 69]            # the oracle's 21 layers on ten boards; the GPU runs all 70
    ref = net_ref.forward(prm, planes[rows], "resnet", 10, np.float64)
    net = _pvn(13, prm, n_blocks=10, trunk_arith="f32")
    try:
        out = net.forward_with_logits(planes)
        check_heads([a[rows] for a in out], ref, len(rows), "13x13, 10 blocks")
    finally:
        net.close()


# ---- 2. every trunk route
ROUTES = {"f32-small": (dict(trunk_arith="f32"), 5), "f32-batched": (dict(trunk_arith="f32"), 70),
          "f32-batched-forced": (dict(trunk_arith="f32", select=4), 5), "direct": (dict(trunk_arith="f32", select=0), 33),
          "f16x2": (dict(trunk_arith="f16x2"), 70), "f16x2-uniform": (dict(trunk_arith="f16x2", uniform_trunk=True), 5),
          "bf16x3": (dict(trunk_arith="bf16x3"), 70)}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("side", [9, 13])
def test_every_trunk_route(nets, side, route):
    kw, n = ROUTES[route]
    net = nets(side, **kw)
    planes = positions(side)[1]
    out = net.forward_with_logits(planes[:n])
    check_heads(out, oracle(side), n, "%dx%d %s" % (side, side, route))
    assert net.trunk_overflows() == 0
    if route == "f16x2-uniform":                          # the small-batch form carries the batched kernel's bits
        big = nets(side, trunk_arith="f16x2").forward_with_logits(planes)
        for a, b in zip(out, big):
            np.testing.assert_array_equal(a, b[:n])


# ---- 3. the invariant
@pytest.mark.parametrize("arith", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("side", [7, 12, 13])
def test_off_board_cells_are_zero_after_every_layer_but_the_last(nets, side, n, arith):
    net = nets(side, trunk_arith=arith)
    planes = positions(side)[1][:n]
    net.forward_planes(planes)
    off = np.ones((15, 16), dtype=bool)
    off[:side, :side] = False
    last = 2 * N_BLOCKS
    for layer in range(last + 1):
        frame = net.layer_frame(layer, n)
        assert frame.shape == (n, 128, 15, 16)
        np.testing.assert_array_equal(frame[:, :, :side, :side], net.layer_output(layer, n))
        if layer < last:
            assert not frame.view(np.uint32)[:, :, off].any(), "layer %d" % layer          # +0, bit for bit
        else:
            # the hook shows the raw buffer: what the last convolution left outside the board is still there
            assert frame[:, :, off].any()
        assert frame[:, :, :side, :side].any()


# ---- 4. independence of buffer history, of the row in the batch and of the batch size; codes against planes
@pytest.mark.parametrize("arith", ["f32", "f16x2"])
@pytest.mark.parametrize("side", [9, 13])
def test_bits_depend_on_the_board_alone(nets, side, arith):
    codes, planes = positions(side)
    used = nets(side, trunk_arith=arith)
    fresh = _pvn(side, params(side), trunk_arith=arith)
    try:
        # a different batch first: 70 full boards, the colour plane all ones -- then 33 boards of the shared set
        dirt = np.repeat(planes[1:2], NMAX, axis=0).copy()
        dirt[:, 8] = 1.0
        used.forward_with_logits(dirt)
        a, b = used.forward_with_logits(planes[:33]), fresh.forward_with_logits(planes[:33])
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        # 33 boards against the same boards inside the batch of 70 (one route: both are batches of more than 32)
        whole = used.forward_with_logits(planes)
        for x, y in zip(a, whole):
            np.testing.assert_array_equal(x, y[:33])
        # ... and in other rows of it
        perm = np.random.RandomState(side).permutation(NMAX)
        shuffled = used.forward_with_logits(planes[perm])
        for x, y in zip(shuffled, whole):
            np.testing.assert_array_equal(x, y[perm])
    finally:
        fresh.close()
    # the codes path (frame_encode_kernel) against the planes path (frame_planes_kernel), both batch classes
    for n in (5, NMAX):
        pc, vc = used.evaluate_codes(codes[:n])
        pp, vp = used.forward_planes(planes[:n])
        np.testing.assert_array_equal(pc, pp)
        np.testing.assert_array_equal(vc, vp)
        ps, vs = used.evaluate_codes_slot(0, codes[:n])
        np.testing.assert_array_equal(np.asarray(ps), pp)
        np.testing.assert_array_equal(np.asarray(vs), vp)


def test_policy_value_fn_on_a_framed_board(nets):
    from alphapig_amd.game import Board
    net = nets(9, trunk_arith="f32")
    b = Board(width=9, height=9, n_in_row=5)
    b.init_board(0)
    for m in (40, 80, 8, 72, 0):
        b.do_move(m)
    pairs, value = net.policy_value_fn(b)
    acts, pr = zip(*pairs)
    state = np.ascontiguousarray(b.current_state(), dtype=np.float32)[None]
    o = net_ref.forward(params(9), state, "resnet", N_BLOCKS, np.float64)
    assert list(acts) == list(b.availables)
    np.testing.assert_allclose(np.array(pr), o[1][0][list(acts)], rtol=0, atol=2e-5)
    np.testing.assert_allclose(value, o[3][0], rtol=0, atol=2e-5)


# ---- 5. the dense planes encoder at these sizes
@pytest.mark.parametrize("c_in", [9, 4])
@pytest.mark.parametrize("side", [6, 13])
def test_encode_planes_on_device_equals_the_host_encoder(nets, side, c_in):
    net = nets(side, trunk_arith="f32")
    codes, planes = positions(side, c_in)
    n = len(codes)
    got = np.full(planes.shape, np.nan, dtype=np.float32)
    dc = net.L.apz_device_alloc(net._h, codes.nbytes)
    dp = net.L.apz_device_alloc(net._h, got.nbytes)
    assert dc and dp
    try:
        host = np.ascontiguousarray(codes)
        net._ck(net.L.apz_memcpy_h2d(net._h, dc, host.ctypes.data, host.nbytes))
        net._ck(net.L.apz_encode_planes(net._h, dc, n, c_in, dp))
        net._ck(net.L.apz_sync(net._h))
        net._ck(net.L.apz_memcpy_d2h(net._h, got.ctypes.data, dp, got.nbytes))
    finally:
        net.L.apz_device_free(net._h, dc)
        net.L.apz_device_free(net._h, dp)
    np.testing.assert_array_equal(got.view(np.uint32), np.asarray(planes).view(np.uint32))


@pytest.mark.parametrize("side", [6, 13])
def test_augment8_on_device_equals_the_host_tables(nets, side):
    from alphapig_amd.augment import augment8_gpu, get_equi_data
    net = nets(side, trunk_arith="f32")
    rs = np.random.RandomState(side)
    planes = (rs.rand(7, 9, side, side) > 0.5).astype(np.float32)
    pis = rs.rand(7, side * side).astype(np.float32)
    xo, po = augment8_gpu(net, planes, pis)
    ext = get_equi_data([(planes[i], pis[i], 0.0) for i in range(7)], side, side)
    np.testing.assert_array_equal(xo, np.stack([e[0] for e in ext]))
    np.testing.assert_array_equal(po, np.stack([e[1] for e in ext]))


@pytest.mark.parametrize("side,n_in_row,c_in", [(9, 5, 9), (13, 5, 4)])
def test_device_replay_buffer_samples_what_the_host_code_buffer_samples(side, n_in_row, c_in):
    """apz_replay_gather works on dense S x S data; the mini-batch then goes through the framed forward from device planes"""
    from _replay_games import episodes
    from alphapig_amd.replay import CompactReplayBuffer, DeviceReplayBuffer
    cb, db = CompactReplayBuffer(301, side, side, c_in), DeviceReplayBuffer(301, side, side, c_in)
    for codes, pis, zs in episodes(side, n_in_row, 12, seed=side, lo=13):
        cb.extend_codes(codes, pis, zs)
        db.extend_codes(codes, pis, zs)
    got, want = db.sample(random.Random(7), 40), cb.sample(random.Random(7), 40)
    assert got.states.is_cuda and tuple(got.states.shape) == (40, c_in, side, side)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x), np.asarray(y))
    if c_in == 9:
        net = _pvn(side, params(side), trunk_arith="f32")
        try:
            pd, vd = net.policy_value_dev(got.states)
            ph, vh = net.policy_value(np.asarray(want[0]))
            np.testing.assert_array_equal(pd, ph)
            np.testing.assert_array_equal(vd, vh)
        finally:
            net.close()


# ---- 6. the heads at hw <= 64 (6x6, 7x7), peaked and saturated
HEAD_PARAMS = ("fc_3_1_1_weight", "fc_3_1_1_bias", "fc_3_2_1_weight", "fc_3_2_1_bias")
HEAD_NMAX = 37


@pytest.fixture(scope="module")
def small_heads():
    made, cache = {}, {}

    def get(side, f):
        prm = dict(params(side, 9, 1))
        for k in HEAD_PARAMS:
            prm[k] = np.asarray(prm[k], dtype=np.float32) * np.float32(f)
        planes = positions(side)[1][:HEAD_NMAX]
        if side not in made:
            made[side] = [_pvn(side, prm, n_blocks=1, batch=64), f]
        elif made[side][1] != f:
            made[side][0].set_params(prm)
            made[side][1] = f
        if (side, f) not in cache:
            cache[(side, f)] = net_ref.forward(prm, planes, "resnet", 1, np.float64)
        return made[side][0], planes, cache[(side, f)]

    yield get
    for net, _ in made.values():
        net.close()


@pytest.mark.parametrize("n", [1, 5, 17, 37])
@pytest.mark.parametrize("f", [1, 30, 1000])
@pytest.mark.parametrize("side", [6, 7])
def test_small_board_heads_scaled(small_heads, side, f, n):
    """fc_3_1_1 / fc_3_2_1 scaled by f scale the logits and the value logit by f (tests/test_gpu_head_edges.py): the
    linear layers against the float64 oracle to LOGIT_ATOL * f, softmax and tanh against float64 of the kernel's own
    logits at the bars of tests/test_head_loss_bounds.py"""
    net, planes, ref = small_heads(side, f)
    planes = planes[:n]
    o_logits, o_vlog = ref[0][:n], ref[2][:n, 0]
    logits, probs, vlog, vals = net.forward_with_logits(planes)
    for a in (logits, probs, vlog, vals):
        assert np.isfinite(a).all()
    bar = LOGIT_ATOL * f
    e_l, e_v = np.abs(logits - o_logits).max(), np.abs(vlog - o_vlog).max()
    p_bar, sum_bar = hb.softmax_bar(logits)
    q_p = hb.ratio(probs, hb.softmax64(logits)[0], p_bar)
    q_s = hb.ratio(probs.astype(np.float64).sum(axis=1), 1.0, sum_bar)
    q_v = hb.ratio(vals, np.tanh(vlog.astype(np.float64)), hb.tanh_bar(vlog))
    print("%dx%d f %g n %d: logits %.2e value logit %.2e (bar %.0e)  error / bar: probs %.3f row sum %.3f values %.3f  "
          "max p %.6f  max |value logit| %.1f" % (side, side, f, n, e_l, e_v, bar, q_p, q_s, q_v, probs.max(), np.abs(vlog).max()))
    assert e_l <= bar and e_v <= bar
    assert q_p <= 1.0 and q_s <= 1.0 and q_v <= 1.0
    assert (np.abs(vals) <= 1).all()
    top = np.sort(o_logits, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * bar
    np.testing.assert_array_equal(probs.argmax(axis=1)[clear], o_logits.argmax(axis=1)[clear])
    gap = np.sort(logits.astype(np.float64), axis=1)
    hot = gap[:, -1] - gap[:, -2] > hb.ONE_HOT_GAP          # one-hot wherever the kernel's own logits say so
    assert (probs[hot].max(axis=1) == 1).all() and ((probs[hot] == 0).sum(axis=1) == probs.shape[1] - 1).all()
    p2, v2 = net.forward_planes(planes)
    np.testing.assert_array_equal(p2, probs)
    np.testing.assert_array_equal(v2, vals)


# ---- 7. range handling
HOT_CHANNEL, HOT_GAMMA, HOT_SHRINK = 3, 5e4, 2.0 ** -13


@functools.lru_cache(maxsize=None)
def hot_params():
    """One hot BatchNorm gamma: channel 3 of block 1's inner activation reaches 1.0e4 on the 40 boards of the test, far past
    the ~655 from which the unscaled two-term fp16 split of the transformed input can overflow (|V| <= 100 max |x|); a
    float64 restatement of V = B^T d B on these boards gives max |V| = 2.3e5, beyond fp16's 65 504: the forward overflows.
    The next convolution's weights for that input channel are shrunk by 2^-13, so the logits keep their scale (max 2.9,
    as without the hot channel) and LOGIT_ATOL keeps its meaning."""
    prm = dict(params(13))
    g = np.array(prm["bnA1_gamma"], np.float32)
    g[HOT_CHANNEL] = HOT_GAMMA
    prm["bnA1_gamma"] = g
    w = np.array(prm["convB1_weight"], np.float32)
    w[:, HOT_CHANNEL] *= np.float32(HOT_SHRINK)
    prm["convB1_weight"] = w
    return prm


def test_range_overflow_repeats_and_calibration_ends_the_repeats():
    prm = hot_params()
    codes, planes = positions(13)
    n = 40
    ref = net_ref.forward(prm, planes[:n], "resnet", N_BLOCKS, np.float64, return_layers=True)
    hot = float(ref[-1][1].max())
    print("13x13 hot net: max inner activation of block 1 = %.4g, max |oracle logit| = %.3g" % (hot, np.abs(ref[0]).max()))
    assert hot > 655
    net = _pvn(13, prm, trunk_arith="f16x2")
    try:
        out = net.forward_with_logits(planes[:n])
        assert net.trunk_overflows() == 1                     # repeated on the exact kernel ...
        check_heads(out, ref, n, "13x13 hot, repeated")
        out = net.forward_with_logits(planes[:n])
        assert net.trunk_overflows() == 2                     # ... every time, until calibrated
        m = net.calibrate_trunk(codes=codes[:n])
        exps = net.trunk_act_exponents()
        print("13x13 hot net: layer maxima", m.tolist(), "exponents", exps)
        assert net.trunk_overflows() == 2 and exps[1] < 0
        np.testing.assert_allclose(m[1], hot, rtol=1e-4)      # the maximum is an on-board one
        pc, vc = net.evaluate_codes(codes[:n])
        out = net.forward_with_logits(planes[:n])
        assert net.trunk_overflows() == 2
        check_heads(out, ref, n, "13x13 hot, calibrated")
        np.testing.assert_array_equal(pc, out[1])
    finally:
        net.close()


# ---- 8. HIP-graph replay
def test_graph_replay_of_a_framed_forward_gives_the_plain_bits(nets):
    net = nets(9, trunk_arith="f16x2", uniform_trunk=True)
    codes = positions(9)[0]

    def run(lo):
        k = net.submit_codes_slot(1, codes[lo:lo + 5])
        p, v = net.wait_slot(1, k)
        return np.array(p, copy=True), np.array(v, copy=True)

    net._ck(net.L.apz_set_forward_graphs(net._h, 0))
    plain, plain_b = run(0), run(20)
    net._ck(net.L.apz_set_forward_graphs(net._h, 1))
    try:
        for rep in range(5):                                  # submissions 1, 2: plain; 3: captured and launched; then replayed
            p, v = run(0)
            np.testing.assert_array_equal(p, plain[0])
            np.testing.assert_array_equal(v, plain[1])
        p, v = run(20)                                        # the replayed graph reads the slot's buffer: other positions
        np.testing.assert_array_equal(p, plain_b[0])
        np.testing.assert_array_equal(v, plain_b[1])
    finally:
        net._ck(net.L.apz_set_forward_graphs(net._h, 0))
    check = net_ref.forward(params(9), positions(9)[1][:5], "resnet", N_BLOCKS, np.float64)
    np.testing.assert_allclose(plain[0], check[1], rtol=0, atol=2e-5)


# ---- 9. self-play
def test_selfplay_9x9_equals_the_sequential_oracle_on_recorded_outputs():
    """9x9, five in a row, 40 concurrent games in ONE group: the batches start at 40 boards and shrink below 33 as games
    finish, so both batch classes of the "f32" route serve the same games.  The evaluations two games consumed are
    recorded (engine tap) and replayed into the sequential oracle: moves, winner and z exact, pi to 1e-12."""
    side, nrow, npl, G, base = 9, 5, 48, 40, 777
    prm = params(side)
    net = _pvn(side, prm, batch=64, trunk_arith="f32")
    eng = SelfPlayEngine(net, side, side, nrow, n_games=G, n_playout=npl, c_puct=5, temp=1.0, base_seed=base, n_threads=4,
                         pipeline=1, forced_opening=False)
    chosen, table, batch_sizes = (0, 1), {}, set()

    def tap(ids, codes, p, v):
        batch_sizes.add(len(ids))
        for i, s in enumerate(ids):
            if eng.slots[int(s)].index in chosen:
                table[codes[i].tobytes()] = (p[i].copy(), np.float32(v[i]))
    eng.tap = tap
    try:
        eps = {e.index: e for e in eng.play_games(G)}
        assert len(eps) == G
        assert max(batch_sizes) > 32 and min(batch_sizes) <= 32, sorted(batch_sizes)
        fn = replay_fn(table, eng.pool.code_stride)
        for k in chosen:
            e = eps[k]
            b = RefBoard(side, side, nrow)
            pl = RefMCTSPlayer(fn, c_puct=5, n_playout=npl, is_selfplay=1, rng=np.random.RandomState(base + k))
            winner, data = selfplay_ref.start_self_play(b, pl, temp=1.0, pyrandom=Never())
            assert winner == e.winner
            np.testing.assert_array_equal(np.array(b.move_list), e.moves)
            np.testing.assert_allclose(np.stack([d[1] for d in data]), e.pis, rtol=0, atol=1e-12)
            np.testing.assert_array_equal(np.array([d[2] for d in data]), e.zs)
        keys = list(table.keys())[:32]
        kc = np.stack([np.frombuffer(k, dtype=np.uint8) for k in keys])
        o = net_ref.forward(prm, eng.pool.codes_to_planes(kc, 9), "resnet", N_BLOCKS, np.float64)
        np.testing.assert_allclose(np.stack([table[k][0] for k in keys]), o[1], rtol=0, atol=2e-5)
        np.testing.assert_allclose(np.array([table[k][1] for k in keys]), o[3][:, 0], rtol=0, atol=2e-5)
        print("9x9 self-play: games 0 / 1 = %d / %d plies, %d recorded evaluations, batch sizes %d .. %d"
              % (len(eps[0].moves), len(eps[1].moves), len(table), min(batch_sizes), max(batch_sizes)))
    finally:
        eng.close()
        net.close()


# ---- 10. arena
def test_arena_6x6_equals_the_sequential_oracle_on_recorded_outputs():
    from alphapig_amd.arena import Arena, win_ratio
    from oracle.mcts_ref import RefPureMCTSPlayer
    side, nrow, npl, pure_n, base, n = 6, 4, 24, 20, 4242, 2
    prm = params(side, 9, 2)
    net = _pvn(side, prm, n_blocks=2, batch=16)
    try:
        rec = Recorder(net)
        res = Arena(rec, side, side, nrow, n_playout=npl, pure_mcts_playout_num=pure_n, base_seed=base, n_threads=2,
                    max_concurrent=2).play(n)
        assert [r.index for r in res] == list(range(n)) and len(rec.table) > 0
        fn = replay_fn(rec.table, (side * side + 1 + 15) // 16 * 16)
        for r in res:
            b = RefBoard(side, side, nrow)
            b.init_board(r.index % 2)
            rs = np.random.RandomState(base + r.index)
            players = {1: RefMCTSPlayer(fn, 5, npl, 0, rng=rs), 2: RefPureMCTSPlayer(5, pure_n, rng=rs)}
            while True:
                b.do_move(int(players[b.get_current_player()].get_action(b)))
                end, winner = b.game_end()
                if end:
                    break
            assert list(r.moves) == list(b.move_list), r.index
            assert r.winner == winner
        assert 0.0 <= win_ratio(res) <= 1.0
    finally:
        net.close()


# ---- 11. refusals
@pytest.mark.parametrize("h,w,filters,kind", [(5, 5, 128, 0), (16, 16, 128, 0), (9, 11, 128, 0), (9, 9, 128, 1), (9, 9, 64, 0), (10, 10, 128, 0)])
def test_unsupported_configurations_are_refused_with_a_message(h, w, filters, kind):
    from alphapig_amd import _native
    L = _native.hip()
    cfg = _native.ApzConfig(h, w, 9, filters, 2, kind, 8, 0)
    assert not L.apz_create(C.byref(cfg))
    msg = L.apz_last_error().decode()
    print(msg)
    assert msg and "15x15" in msg
    # the same through the evaluator class
    from alphapig_amd.policy_value_net import EvaluatorError, PolicyValueNet
    with pytest.raises(EvaluatorError):
        PolicyValueNet(w, h, batch_size=8, n_blocks=2, n_filter=filters, net_kind="resnet" if kind == 0 else "simple")


@pytest.mark.parametrize("side,filters,kind", [(8, 128, 0), (8, 64, 1), (15, 128, 0), (15, 64, 0), (15, 256, 1)])
def test_8x8_and_15x15_engines_are_created_as_before(side, filters, kind):
    from alphapig_amd import _native
    L = _native.hip()
    cfg = _native.ApzConfig(side, side, 9, filters, 1, kind, 8, 0)
    h = L.apz_create(C.byref(cfg))
    assert h, L.apz_last_error().decode()
    L.apz_destroy(h)
