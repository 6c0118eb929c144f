"""state() / load_state() of the replay buffers: a fresh buffer loaded with the state of a used one holds the same
entries, draws the same mini-batches and goes on the same way -- wrapped ring, tiny ring and a ring not yet full."""
import random

import numpy as np
import pytest

from alphapig_amd.pipeline import ReplayBuffer
from alphapig_amd.replay import CompactReplayBuffer

SIDE = 8
HW = SIDE * SIDE
SHAPES = [(301, 90), (8, 5), (100000, 37)]      # maxlen, tuples: capacity 39 wrapped twice, capacity 2, not yet full


def tuples(n, seed):
    """n tuples as the self-play exchange delivers them: position codes, pi, z"""
    rs = np.random.RandomState(seed)
    stride = (HW + 1 + 15) // 16 * 16
    codes = np.zeros((n, stride), dtype=np.uint8)
    codes[:, :HW] = rs.randint(0, 9, size=(n, HW))
    codes[:, HW] = rs.randint(0, 2, size=n)
    pis = rs.rand(n, HW).astype(np.float32)
    zs = rs.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32)
    return codes, pis, zs


def same_entries(a, b):
    assert len(a) == len(b) and a.ring.appended == b.ring.appended
    for i in range(len(a)):
        for x, y in zip(a.entry(i), b.entry(i)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def same_sample(a, b, k):
    x, y = a.sample(random.Random(3), k), b.sample(random.Random(3), k)
    for u, v in zip(x, y):
        u, v = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in (u, v))
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()


def check_round_trip(make, maxlen, n_tuples, other=None):
    """other: a second constructor whose buffer must agree with the restored one as well (device against host)"""
    a = make(maxlen)
    done = 0
    for chunk in (n_tuples // 3, n_tuples - n_tuples // 3):         # (two extends: the second one wraps)
        a.extend_codes(*[x[done:done + chunk] for x in tuples(n_tuples, 1)])
        done += chunk
    state = a.state()
    A, n = a.ring.appended, len(a)
    assert len(state["codes"]) == len(state["pi"]) == len(state["z"]) == (A + 7) // 8 - (A - n) // 8 <= a.ring.capacity
    assert state["codes"].dtype == np.uint8 and state["pi"].dtype == np.float32 and state["z"].dtype == np.float32
    b = make(maxlen)
    b.load_state(state)
    bufs = [a, b]
    if other is not None:
        c = other(maxlen)
        c.load_state(state)
        bufs.append(c)
    k = min(16, len(a))
    for x in bufs[1:]:
        same_entries(a, x)
        same_sample(a, x, k)
    for x in bufs:
        x.extend_codes(*tuples(50, 2))
    for x in bufs[1:]:
        same_entries(a, x)
        same_sample(a, x, min(16, len(a)))


@pytest.mark.parametrize("maxlen,n_tuples", SHAPES)
def test_compact_buffer_round_trip(maxlen, n_tuples):
    check_round_trip(lambda m: CompactReplayBuffer(m, SIDE, SIDE, 9), maxlen, n_tuples)


def test_an_empty_buffer_round_trips():
    a, b = CompactReplayBuffer(301, SIDE, SIDE, 9), CompactReplayBuffer(301, SIDE, SIDE, 9)
    b.extend_codes(*tuples(3, 5))
    state = a.state()
    assert len(state["codes"]) == 0
    b2 = CompactReplayBuffer(301, SIDE, SIDE, 9)
    b2.load_state(state)
    assert len(b2) == 0


@pytest.mark.parametrize("field,make", [("maxlen", lambda: CompactReplayBuffer(300, SIDE, SIDE, 9)),
                                        ("height", lambda: CompactReplayBuffer(301, 15, 15, 9)),
                                        ("c_in", lambda: CompactReplayBuffer(301, SIDE, SIDE, 4))])
def test_a_state_of_another_buffer_is_refused(field, make):
    a = CompactReplayBuffer(301, SIDE, SIDE, 9)
    a.extend_codes(*tuples(60, 1))
    b = make()
    with pytest.raises(ValueError, match=field):
        b.load_state(a.state())
    assert len(b) == 0
    state = a.state()
    state["codes"] = state["codes"][:-1]
    c = CompactReplayBuffer(301, SIDE, SIDE, 9)
    with pytest.raises(ValueError):
        c.load_state(state)
    assert len(c) == 0


@pytest.mark.parametrize("maxlen,n", [(301, 700), (8, 20), (1000, 90)])
def test_tuple_buffer_round_trip(maxlen, n):
    rs = np.random.RandomState(4)
    items = [(rs.rand(9, SIDE, SIDE).astype(np.float32), rs.rand(HW), np.float64(rs.choice([-1.0, 1.0]))) for _ in range(n + 50)]
    a, b = ReplayBuffer(maxlen), ReplayBuffer(maxlen)
    a.extend(items[:n])
    b.load_state(a.state())
    for step in range(2):
        assert len(a) == len(b) == min(maxlen, n + 50 * step)
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert np.asarray(u).dtype == np.asarray(v).dtype and np.array_equal(u, v)
        for x, y in zip(a.sample(random.Random(3), min(8, len(a))), b.sample(random.Random(3), min(8, len(b)))):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        a.extend(items[n:])
        b.extend(items[n:])
    with pytest.raises(ValueError, match="maxlen"):
        ReplayBuffer(maxlen + 1).load_state(a.state())
