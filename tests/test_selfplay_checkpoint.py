"""SelfPlayEngine.state / load_state: an engine stopped between two run_steps calls and rebuilt from its state plays the
episodes of the engine that was never stopped, bit for bit -- trees, NumPy legacy streams and half-recorded games
included.  Stand-in evaluator (tests/fakenet.py), no GPU."""
import io
import json

import numpy as np
import pytest

from alphapig_amd.selfplay import SelfPlayEngine
from fakenet import fake_policy_value_batch


def _engine(sampler="host", pipeline=2, side=8, **kw):
    args = dict(n_games=8, n_playout=8 if side == 8 else 4, temp=1.0, base_seed=1000, n_threads=1, pipeline=pipeline,
                forced_opening=(side == 15), sampler=sampler)
    args.update(kw)
    return SelfPlayEngine(fake_policy_value_batch, side, side, 4 if side == 8 else 5, **args)


def _through_files(state):
    """what a checkpoint does with a state: JSON for the plain values, .npy without pickling for the arrays"""
    meta = json.loads(json.dumps(state["meta"]))
    buf = io.BytesIO()
    np.savez(buf, **{k: v for k, v in state.items() if k != "meta"})
    buf.seek(0)
    with np.load(buf, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    out["meta"] = meta
    return out


def _same_episodes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.index == y.index and x.winner == y.winner
        for f in ("moves", "movers", "codes", "pis", "zs"):
            u, v = getattr(x, f), getattr(y, f)
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (x.index, f)


@pytest.mark.parametrize("sampler,pipeline,side", [("host", 1, 8), ("host", 2, 8), ("numpy", 1, 8), ("numpy", 2, 8),
                                                   ("host", 2, 15)])
def test_a_reloaded_engine_plays_the_episodes_of_the_one_that_went_on(sampler, pipeline, side):
    a = _engine(sampler, pipeline, side)
    a.run_steps(40)
    assert a.stats["moves"] > 8 and any(len(s.movers) for s in a.slots)
    state = _through_files(a.state())
    b = _engine(sampler, pipeline, side)
    b.load_state(state)
    c = _engine(sampler, pipeline, side)            # the control: told only where the game sequence stands
    c.next_index = a.next_index
    a.run_steps(300)
    b.run_steps(300)
    c.run_steps(300)
    assert len(a.finished) >= (8 if side == 8 else 2)       # (15x15 games are long: the ones in flight at the cut)
    _same_episodes(a.finished, b.finished)
    assert a.next_index == b.next_index
    assert {k: a.stats[k] for k in a._STATE_STATS} == {k: b.stats[k] for k in a._STATE_STATS}
    np.testing.assert_array_equal(a.slot_games, b.slot_games)
    # ... and a second state of both is the same state
    sa, sb = a.state(), b.state()
    assert sa["meta"] == sb["meta"] and sorted(sa) == sorted(sb)
    for k in sa:
        if k != "meta":
            assert sa[k].dtype == sb[k].dtype and sa[k].tobytes() == sb[k].tobytes(), k
    key = lambda eps: [(e.index, e.moves.tolist()) for e in eps]
    assert key(c.finished) != key(a.finished)
    for e in (a, b, c):
        e.close()


def test_finished_episodes_nobody_took_travel_with_the_state():
    a = _engine()
    a.run_steps(250)
    assert len(a.finished) >= 3
    del a.finished[:1]
    b = _engine()
    b.load_state(_through_files(a.state()))
    _same_episodes(a.finished, b.finished)
    a.close()
    b.close()


def test_a_state_without_games_keeps_the_sequence_and_the_finished_episodes():
    a = _engine()
    a.run_steps(250)
    state = _through_files(a.state(games=False))
    assert "blobs" not in state
    b = _engine()
    b.load_state(state)
    _same_episodes(a.finished, b.finished)
    assert b.next_index == a.next_index and not any(s.active for s in b.slots)
    done = set(e.index for e in b.finished)
    b.run_steps(250)
    fresh = [e.index for e in b.finished if e.index not in done]
    assert fresh and min(fresh) >= a.next_index and len(set(e.index for e in b.finished)) == len(b.finished)
    a.close()
    b.close()


@pytest.mark.parametrize("field,other", [("board_width", dict(side=15)), ("n_games", dict(n_games=4)),
                                         ("n_playout", dict(n_playout=9)), ("sampler", dict(sampler="numpy")),
                                         ("index_offset", dict(index_offset=1, index_stride=2)),
                                         ("index_stride", dict(index_stride=2))])
def test_a_state_of_another_engine_is_refused_by_name(field, other):
    a = _engine()
    a.run_steps(10)
    state = a.state()
    b = _engine(**other)
    with pytest.raises(ValueError, match=field):
        b.load_state(state)
    assert b.next_index == 0 and not any(s.active for s in b.slots)
    a.close()
    b.close()
