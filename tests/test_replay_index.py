"""The ring arithmetic of the code replay buffers (alphapig_amd/replay.py) against the reference's own container,
`collections.deque(maxlen=M)` of 8x augmented entries, and the host code buffer against pipeline.ReplayBuffer."""
import collections
import random

import numpy as np
import pytest

from _replay_games import episodes
from alphapig_amd.augment import get_equi_data
from alphapig_amd.pipeline import ReplayBuffer
from alphapig_amd.replay import CompactReplayBuffer, RingIndex
from alphapig_amd.treepool import TreePool


@pytest.mark.parametrize("M", [5, 8, 13, 64, 1001])
def test_ring_rule_against_deque(M):
    rs = random.Random(M)
    dq = collections.deque(maxlen=M)
    ring = RingIndex(M)
    assert ring.capacity == (M + 7) // 8 + 1
    phys = [None] * ring.capacity          # which tuple every ring slot holds, written the way a backend writes its rows
    t_next = 0
    for _ in range(300):
        t = rs.randint(1, 40)
        dq.extend((T, k) for T in range(t_next, t_next + t) for k in range(8))
        skip, segs = ring.extend(t)
        at = t_next + skip
        assert len(segs) <= 2 or ring.capacity < 3
        for slot, cnt in segs:
            assert 0 <= slot and slot + cnt <= ring.capacity
            phys[slot:slot + cnt] = range(at, at + cnt)
            at += cnt
        t_next += t
        assert at == t_next and len(ring) == len(dq)
        live = {T for T, _ in dq}
        assert len(live) <= ring.capacity and len({T % ring.capacity for T in live}) == len(live)
        n = len(dq)
        for i in [0, n - 1, -1] + [rs.randrange(n) for _ in range(10)]:
            assert ring.locate(i) == dq[i]
            w = ring.word(i)
            assert 0 <= w < 8 * ring.capacity and (phys[w >> 3], w & 7) == dq[i]
        k = min(n, 7)
        words = ring.sample(random.Random(11), k)
        assert words.dtype == np.int32 and words.shape == (k,)
        drawn = random.Random(11).sample(range(n), k)          # the same draws as ReplayBuffer.sample makes
        assert [(phys[w >> 3], w & 7) for w in words] == [dq[i] for i in drawn]
    with pytest.raises(IndexError):
        ring.locate(len(dq))


@pytest.mark.parametrize("width,n_in_row,c_in", [(15, 5, 9), (8, 4, 4)])
def test_compact_buffer_samples_what_the_tuple_buffer_samples(width, n_in_row, c_in):
    M = 1001
    pool = TreePool(width, width, n_in_row, n_games=1, n_playout=1)
    rb, cb = ReplayBuffer(M), CompactReplayBuffer(M, width, width, c_in)
    appended = 0
    for codes, pis, zs in episodes(width, n_in_row, 32, seed=width, lo=13):
        states = pool.codes_to_planes(codes, c_in)
        rb.extend(get_equi_data(list(zip(states, pis, zs)), width, width))
        cb.extend_codes(codes, pis, zs)
        appended += 8 * len(codes)
        assert len(cb) == len(rb)
    assert appended >= 3 * M + 8 and len(cb) == M          # the ring has wrapped at least three times
    for k in (1, 7, 64):
        mini = rb.sample(random.Random(5 + k), k)
        got = cb.sample(random.Random(5 + k), k)
        assert got.states.dtype == np.float32 and got.states.shape == (k, c_in, width, width)
        assert got.pis.dtype == np.float32 and got.zs.dtype == np.float32
        assert np.array_equal(got.states, np.stack([d[0] for d in mini]).astype(np.float32))
        assert np.array_equal(got.pis, np.stack([d[1] for d in mini]).astype(np.float32))
        assert np.array_equal(got.zs, np.array([d[2] for d in mini], dtype=np.float32))
    for i in (0, 1, 7, 8, M // 2, M - 1):
        s, p, z = cb.entry(i)
        assert np.array_equal(s, rb[i][0]) and np.array_equal(p, rb[i][1]) and z == rb[i][2]
    pool.close()
