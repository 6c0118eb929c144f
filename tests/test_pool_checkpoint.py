"""TreePool.save_game / load_game: a game taken out of one pool mid-search and put into another goes on exactly as
the game that stayed -- root visit counts, emitted code rows, moves and winners, to the end of the games -- and a damaged
blob is refused as a whole.  Stand-in evaluator (tests/fakenet.py), no GPU."""
import struct

import numpy as np
import pytest

from alphapig_amd.treepool import MOVE_READY, NEED_EVAL, TreePool, TreePoolError
from fakenet import fake_policy_value_batch

BOARDS = [(8, 4, 16), (15, 5, 24)]          # side, n_in_row, n_playout
HEADER = 88                                 # bytes; the counts sit at 52 (history), 56 (path), 60 (nodes)


def _pool(side, n_in_row, n_playout, n_games=8):
    pool = TreePool(side, side, n_in_row, n_games=n_games, n_playout=n_playout, n_threads=1)
    for g in range(n_games):
        pool.reset(g, 0)
    return pool


def _answers(pool, codes):
    return fake_policy_value_batch(pool.codes_to_planes(codes, 9))


def _round(pools, ids, log):
    """One scheduler round of the games `ids` on every pool of `pools`, which must agree in everything they emit; the
    evaluator is asked once and its answers go to all of them.  A ready game plays its most visited move (first maximum).
    -> the games still running"""
    outs = [p.advance(ids) for p in pools]
    st, codes = outs[0]
    for o in outs[1:]:
        np.testing.assert_array_equal(o[0], st)
        np.testing.assert_array_equal(o[1][st == NEED_EVAL], codes[st == NEED_EVAL])
    need = ids[st == NEED_EVAL]
    if len(need):
        probs, values = _answers(pools[0], codes[st == NEED_EVAL])
        for p in pools:
            p.feed(need, probs, values)
        log.append(("leaf", need.tolist(), codes[st == NEED_EVAL].tobytes()))
    ready = ids[st == MOVE_READY]
    alive = set(int(g) for g in ids)
    if len(ready):
        visits = [p.root_visits_dense(ready) for p in pools]
        for v in visits[1:]:
            np.testing.assert_array_equal(v[0], visits[0][0])
            np.testing.assert_array_equal(v[1], visits[0][1])
        moves = visits[0][0].argmax(axis=1).astype(np.int32)
        played = [p.play_moves(ready, moves) for p in pools]
        for q in played[1:]:
            for a, b in zip(q, played[0]):
                np.testing.assert_array_equal(a, b)
        codes_b, movers_b, ended, winner = played[0]
        log.append(("move", ready.tolist(), visits[0][0].tobytes(), moves.tolist(), codes_b.tobytes(), movers_b.tolist(),
                    ended.tolist(), winner.tolist()))
        alive -= set(int(g) for g in ready[ended])
    return np.array(sorted(alive), dtype=np.int32)


def _to_the_end(pools, ids, log, limit=100000):
    for _ in range(limit):
        if not len(ids):
            return
        ids = _round(pools, ids, log)
    raise AssertionError("the games did not end")


def _mid_search(side, n_in_row, n_playout):
    """A pool of 8 games: 0 .. 5 inside the search of their third move with a leaf pending, 6 right after its first
    play_move, 7 empty.  -> (pool, the code rows of the pending leaves of games 0 .. 5)"""
    pool = _pool(side, n_in_row, n_playout)
    log = []
    ids = np.arange(6, dtype=np.int32)
    for _ in range(2 * (n_playout + 1) + n_playout // 2):
        ids = _round([pool], ids, log)
    assert len(ids) == 6 and sum(1 for e in log if e[0] == "move") >= 2
    st, codes = pool.advance(ids)
    assert (st == NEED_EVAL).all()
    six = np.array([6], dtype=np.int32)
    while not any(e[0] == "move" and e[1] == [6] for e in log):
        _round([pool], six, log)
    assert pool.playouts_done(6) == 0 and pool.status(6)[1] == 1 and pool.status(7)[1] == 0
    return pool, codes


@pytest.mark.parametrize("side,n_in_row,n_playout", BOARDS)
def test_saved_games_go_on_in_a_fresh_pool_as_in_the_old_one(side, n_in_row, n_playout):
    a, codes = _mid_search(side, n_in_row, n_playout)
    blobs = [a.save_game(g) for g in range(8)]
    assert all(isinstance(b, bytes) and len(b) > HEADER for b in blobs)
    assert struct.unpack_from("<i", blobs[0], 40)[0] == 1 and struct.unpack_from("<i", blobs[6], 40)[0] == 0   # pending
    assert struct.unpack_from("<i", blobs[7], 60)[0] == 1 < struct.unpack_from("<i", blobs[6], 60)[0]          # nodes
    b = _pool(side, n_in_row, n_playout)
    for g in range(8):
        b.load_game(g, blobs[g])
        assert b.save_game(g) == blobs[g]
        assert b.stats(g) == a.stats(g) and b.playouts_done(g) == a.playouts_done(g)
    for g in range(6):
        np.testing.assert_array_equal(b.pending_path(g), a.pending_path(g))
    # the pending leaves get the answers to the code rows the old pool emitted for them
    probs, values = _answers(a, codes)
    for p in (a, b):
        p.feed(np.arange(6, dtype=np.int32), probs, values)
    log = []
    _to_the_end([a, b], np.arange(8, dtype=np.int32), log)
    assert sum(len(e[1]) for e in log if e[0] == "move") > 8 * n_in_row
    for g in range(8):
        assert a.status(g) == b.status(g) and a.status(g)[2]
        np.testing.assert_array_equal(a.history(g)[0], b.history(g)[0])
    a.close()
    b.close()


def _patched(blob, offset, fmt, value):
    out = bytearray(blob)
    struct.pack_into(fmt, out, offset, value)
    return bytes(out)


def _damaged(blob, hw):
    n_hist, n_path, n_nodes = struct.unpack_from("<iii", blob, 52)
    arena = HEADER + 3 * hw + 3 * n_hist + 2 * n_path           # parent, first_child, n (i32), n_child, action (i16) ...
    first_child, action = arena + 4 * n_nodes, arena + 14 * n_nodes
    assert n_nodes > 4
    return {"one byte short": blob[:-1], "half": blob[:len(blob) // 2], "empty": b"",
            "magic": _patched(blob, 0, "<I", struct.unpack_from("<I", blob, 0)[0] + 1),
            "board": _patched(blob, 8, "<i", struct.unpack_from("<i", blob, 8)[0] + 1),
            "first_child past the arena": _patched(blob, first_child + 4 * 0, "<i", n_nodes),
            "action off the board": _patched(blob, action + 2 * 3, "<h", hw)}


@pytest.mark.parametrize("side,n_in_row,n_playout", BOARDS)
def test_a_damaged_blob_is_refused_and_the_slot_plays_on(side, n_in_row, n_playout):
    a, codes = _mid_search(side, n_in_row, n_playout)
    b = _pool(side, n_in_row, n_playout)
    for g in range(8):
        b.load_game(g, a.save_game(g))
    blob = a.save_game(2)
    other = _pool(*[x for x in BOARDS if x[0] != side][0], n_games=1)
    cases = _damaged(blob, side * side)
    cases["a game of another board"] = other.save_game(0)
    for name, bad in cases.items():
        for g in (2, 6, 7):                     # a slot with a pending leaf, one between moves, an empty one
            before = b.save_game(g)
            with pytest.raises(TreePoolError, match=r"code -\d"):
                b.load_game(g, bad)
            assert b.save_game(g) == before, name
    with pytest.raises(TreePoolError):
        other.load_game(0, blob)
    probs, values = _answers(a, codes)
    for p in (a, b):
        p.feed(np.arange(6, dtype=np.int32), probs, values)
    _to_the_end([a, b], np.arange(8, dtype=np.int32), [])
    for g in range(8):
        assert a.status(g) == b.status(g) and a.status(g)[2]
    for p in (a, b, other):
        p.close()
