"""The device replay buffer (alphapig_amd/replay.py: DeviceReplayBuffer, csrc/replay.h) on the GPU: the gathered mini-batch
against the host code buffer and against the reference's own tables, the KL monitor's forward on device planes, and
policy_update / TrainPipeline fed from it against the tuple path.  Everything is compared bit for bit."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from _replay_games import episodes, random_game_tuples
from alphapig_amd import weights
from alphapig_amd.augment import get_equi_data
from alphapig_amd.game import Board

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _host(batch):
    return tuple(np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in batch)


def _same(a, b):
    a, b = _host(a), _host(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.float32 and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


def _pair(M, width, c_in):
    from alphapig_amd.replay import CompactReplayBuffer, DeviceReplayBuffer
    return CompactReplayBuffer(M, width, width, c_in), DeviceReplayBuffer(M, width, width, c_in)


@pytest.mark.parametrize("width,n_in_row,c_in", [(15, 5, 9), (8, 4, 4)])
def test_device_buffer_samples_what_the_host_code_buffer_samples(width, n_in_row, c_in):
    M = 1001                                    # not a multiple of 8: the wrap falls inside a tuple
    cb, db = _pair(M, width, c_in)
    assert db.codes.shape == (126 + 1, cb.code_stride) and db.nbytes() == 127 * (cb.code_stride + 4 * width * width + 4)
    for i, (codes, pis, zs) in enumerate(episodes(width, n_in_row, 32, seed=width, lo=13)):
        cb.extend_codes(codes, pis, zs)
        db.extend_codes(codes, pis, zs)
        assert len(db) == len(cb)
        if i in (0, 5, 31):                     # before the first wrap, after it, at the end
            for k in (1, 7, 64):
                got = db.sample(random.Random(100 * i + k), k)
                assert got.states.is_cuda and tuple(got.states.shape) == (k, c_in, width, width)
                _same(got, cb.sample(random.Random(100 * i + k), k))
    assert cb.ring.appended >= 3 * M + 8
    for i in (0, 7, 8, M - 1):
        for x, y in zip(db.entry(i), cb.entry(i)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("tag,width,n_in_row", [("e2", 15, 5), ("e1", 8, 4)])
def test_gather_applies_the_reference_tables(golden_dir, tag, width, n_in_row):
    from alphapig_amd import hipconv
    g = np.load(os.path.join(golden_dir, "equi.npz"))
    assert int(g[tag + "_w"]) == width
    codes, pis, zs = random_game_tuples(width, n_in_row, 12, seed=2)
    cb, db = _pair(5, width, 9)                 # a ring of capacity 2: the tuple below lands in its LAST slot
    assert db.ring.capacity == 2
    db.extend_codes(codes[:2], pis[:2], zs[:2])
    cb.extend_codes(codes[:2], pis[:2], zs[:2])
    words = np.arange(8, 16, dtype=np.int32)   # slot 1, all eight symmetries
    states, p, z = _host(hipconv.replay_gather(db.codes, db.pi, db.z, words, width, width, 9))
    planes = cb._dec.codes_to_planes(codes[1:2], 9)[0]
    np.testing.assert_array_equal(states, planes.reshape(-1)[g[tag + "_state_perm"]])
    np.testing.assert_array_equal(p, pis[1][g[tag + "_pi_perm"]])
    np.testing.assert_array_equal(z, np.full(8, zs[1], np.float32))


def test_identity_image_is_the_reference_boards_planes(golden_dir):
    from alphapig_amd import hipconv
    g = np.load(os.path.join(golden_dir, "planes.npz"))
    by_width = {}
    for k in range(int(g["n_cases"])):
        w, n, sp, _ = [int(x) for x in g["c%d_meta" % k]]
        if w not in (8, 15):                    # (the HIP engine exists for these two boards)
            continue
        b = Board(width=w, height=w, n_in_row=n)
        b.init_board(sp)
        for m in g["c%d_moves" % k]:
            b.do_move(int(m))
        by_width.setdefault(w, []).append((b.position_codes(), g["c%d_planes" % k], g["c%d_planes4" % k]))
    assert set(by_width) == {8, 15}
    for w, cases in by_width.items():
        t = len(cases)
        codes = torch.tensor(np.stack([c[0] for c in cases]), device="cuda")
        pi = torch.zeros((t, w * w), device="cuda")
        z = torch.zeros((t,), device="cuda")
        words = np.arange(t, dtype=np.int32) * 8 + 6
        for c_in, col in ((9, 1), (4, 2)):
            states = hipconv.replay_gather(codes, pi, z, words, w, w, c_in)[0].cpu().numpy()
            np.testing.assert_array_equal(states, np.stack([c[col] for c in cases]).astype(np.float32))


@pytest.mark.parametrize("width,n_in_row,c_in", [(15, 5, 9), (8, 4, 4)])
def test_smallest_shapes(width, n_in_row, c_in):
    cb, db = _pair(5, width, c_in)              # capacity 2; blocks of up to 6 tuples: some are dead on arrival
    for codes, pis, zs in episodes(width, n_in_row, 9, seed=7, lo=1, hi=6):
        cb.extend_codes(codes, pis, zs)
        db.extend_codes(codes, pis, zs)
        _same(db.sample(random.Random(3), 1), cb.sample(random.Random(3), 1))               # n = 1
        _same(db.sample(random.Random(4), 5), cb.sample(random.Random(4), 5))               # every live entry
    for words in ([8] * 5 + [9, 15, 8], [15], [0, 15, 7, 8], list(range(16)) * 40):         # one slot; the last word; > 1 block
        words = np.array(words, dtype=np.int32)
        _same(db._gather(words), cb._gather(words))


def test_refusals_happen_before_the_library_is_called(monkeypatch):
    from alphapig_amd import _native, hipconv
    cap, stride = 2, 240
    codes = torch.zeros((cap, stride), dtype=torch.uint8, device="cuda")
    pi = torch.zeros((cap, 225), device="cuda")
    z = torch.zeros((cap,), device="cuda")
    L = _native.hip()
    hnd = hipconv._engine(15, 15, 0)
    out = [torch.zeros((1, 9, 15, 15), device="cuda"), torch.zeros((1, 225), device="cuda"), torch.zeros((1,), device="cuda")]
    call = lambda ent, n_planes: L.apz_replay_gather(hnd, codes.data_ptr(), pi.data_ptr(), z.data_ptr(), cap,
                                                     (C.c_int32 * 1)(ent), 1, n_planes, out[0].data_ptr(), out[1].data_ptr(),
                                                     out[2].data_ptr(), None)
    # the library itself refuses, before it copies or launches anything
    assert call(8 * cap, 9) < 0 and b"outside" in L.apz_last_error()
    assert call(-1, 9) < 0 and call(0, 5) < 0
    assert L.apz_replay_gather(hnd, None, None, None, cap, None, 0, 9, None, None, None, None) == 0      # n == 0

    def unreachable(*a, **kw):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hipconv._native, "hip", unreachable)
    monkeypatch.setattr(hipconv, "_engine", unreachable)
    for bad in ([8 * cap], [-1], [0, 3, 16], [1.5]):
        with pytest.raises(ValueError):
            hipconv.replay_gather(codes, pi, z, bad, 15, 15, 9)
    with pytest.raises(ValueError):
        hipconv.replay_gather(codes, pi, z, [0], 15, 15, 5)
    with pytest.raises(ValueError):
        hipconv.replay_gather(codes, pi[:, :64], z, [0], 15, 15, 9)
    states, p, zz = hipconv.replay_gather(codes, pi, z, [], 15, 15, 9)                                   # n == 0
    assert tuple(states.shape) == (0, 9, 15, 15) and tuple(p.shape) == (0, 225) and tuple(zz.shape) == (0,)


@pytest.mark.parametrize("width,kind,ns", [(15, "resnet", (1, 33)), (8, "simple", (5,))])
def test_policy_value_dev_carries_policy_values_bits(width, kind, ns):
    from alphapig_amd.policy_value_net import PolicyValueNet
    prm = weights.init_params(kind, width, width, 9, 1, 128, seed=4, style="bench")
    net = PolicyValueNet(width, width, batch_size=16 if width == 8 else 64, n_blocks=1, n_filter=128, model_params=prm,
                         net_kind=kind)
    cb, db = _pair(1001, width, 9)
    codes, pis, zs = random_game_tuples(width, 5 if width == 15 else 4, 40, seed=6)
    db.extend_codes(codes, pis, zs)
    for n in ns + (40,):                        # 40 on the 8x8 net: more than batch_size, chunked
        t = db.sample(random.Random(n), n).states
        p_dev, v_dev = net.policy_value_dev(t)
        p, v = net.policy_value(t.cpu().numpy())
        assert p_dev.shape == (n, width * width) and v_dev.shape == (n, 1)
        np.testing.assert_array_equal(p_dev, p)
        np.testing.assert_array_equal(v_dev, v)
    with pytest.raises(ValueError):
        net.policy_value_dev(t.cpu())
    net.close()


def test_policy_update_from_the_device_buffer_is_the_list_paths_update():
    from alphapig_amd.pipeline import ReplayBuffer
    from alphapig_amd.replay import DeviceReplayBuffer
    from alphapig_amd.train import HipTrainer, policy_update
    from alphapig_amd.treepool import TreePool
    prm = weights.init_params("resnet", 15, 15, 9, 1, 128, seed=8, style="bench")
    pool = TreePool(15, 15, 5, n_games=1, n_playout=1)
    rb, db = ReplayBuffer(1001), DeviceReplayBuffer(1001, 15, 15, 9)
    for codes, pis, zs in episodes(15, 5, 8, seed=9, lo=13, hi=30):
        rb.extend(get_equi_data(list(zip(pool.codes_to_planes(codes, 9), pis, zs)), 15, 15))
        db.extend_codes(codes, pis, zs)
    pool.close()
    res = []
    for buf in (rb, db):
        tr = HipTrainer(prm, "resnet", n_blocks=1, batch_size=16, seed=2)
        rng, mult, outs = random.Random(12), 1.0, []
        for _ in range(2):
            mon = {}
            loss, ent, kl, mult = policy_update(tr, buf.sample(rng, 16), 2e-3, mult, epochs=2, kl_targ=0.02, monitors=mon)
            outs.append((loss, ent, kl, mult, mon["explained_var_old"], mon["explained_var_new"]))
        res.append((outs, tr.get_params()))
        tr.close()
    assert res[0][0] == res[1][0]
    for k, v in res[0][1].items():
        np.testing.assert_array_equal(v, res[1][1][k], err_msg=k)


def test_pipeline_with_the_device_buffer_is_the_tuple_pipeline(tmp_path):
    from alphapig_amd.pipeline import TrainPipeline
    from alphapig_amd.replay import DeviceReplayBuffer
    runs = []
    for replay in ("tuples", "device"):
        conf = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
                "n_playout": 8, "c_puct": 5, "buffer_size": 301, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
                "check_freq": 1000, "game_batch_num": 3, "play_batch_size": 2, "pure_mcts_playout_num": 10,
                "async_update": False, "concurrent_games": 8, "n_blocks": 1, "n_filter": 64,
                "model_dir": str(tmp_path / replay), "replay": replay}
        pipe = TrainPipeline(conf, device=0, seed=5, distributed=False)
        hist = pipe.run()
        assert isinstance(pipe.data_buffer, DeviceReplayBuffer) == (replay == "device")
        runs.append(([(r["buffer"], r.get("loss"), r.get("entropy"), r.get("kl")) for r in hist], pipe.lr_multiplier,
                     pipe._trainer().get_params()))
        pipe.close()
    assert runs[0][0] == runs[1][0] and sum(r[1] is not None for r in runs[0][0]) >= 2
    assert runs[0][1] == runs[1][1]
    for k, v in runs[0][2].items():
        np.testing.assert_array_equal(v, runs[1][2][k], err_msg=k)
