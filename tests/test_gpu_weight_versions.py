"""Every evaluator answer carries ONE weight version across a device-side refresh.

apz_load_weights_dev (PolicyValueNet.load_device_params, HipTrainer.sync_evaluator, TrainPipeline._install_weights) folds
BatchNorm and repacks every layer with kernels on a caller-chosen stream while batches submitted earlier are still queued
or running on the engine's own non-blocking stream.  The contract, for weight versions V0, V1, ... installed in that order:

  1. a batch submitted before an install call was entered is answered with the bits of the previous version;
  2. a batch submitted after the install call has returned is answered with the bits of the new version;
  3. no answer mixes versions;
  4. on every route, whichever stream the refresh runs on, with or without a replayed graph;
  5. with submitters and a refresher in different host threads, answers in submission order carry non-decreasing versions.

"The bits of version k": the answer of a reference evaluator of the same configuration that only ever held version k
behind a stand-in host load -- refreshed through the same device path, then sync(), nothing in flight -- to the same codes
through the same entry point (apz_submit_codes / apz_wait) at the same batch size: the same route, the same arithmetic, so
every comparison is assert_array_equal.  Host pack against device pack is settled elsewhere (tests/test_gpu_net.py,
tests/test_gpu_train.py, tests/test_gpu_trained_weights.py).  So that the references are not a mirror of a shared mistake,
each is held once to oracle/net_ref.py in float64 on its first boards with the bars of tests/test_gpu_net.py: LOGIT_ATOL
on the logits and the value logit, 2e-5 on probabilities and values.

An overflowed f16x2 batch is the one documented exception to (1) -- apz_wait repeats it on the weights installed at the
time of the wait -- and has a test of its own at the end; it takes no part in the ordering tests.
"""
import collections
import threading

import numpy as np
import pytest

from alphapig_amd import weights
from oracle import net_ref
from test_gpu_net import LOGIT_ATOL, random_positions

pytestmark = pytest.mark.gpu

K = 4                       # weight sets per configuration
SEEDS = (71, 72, 73, 74)    # ... their seeds; STANDIN_SEED: the host load every evaluator starts from
STANDIN_SEED = 70
N_ORACLE = 5                # boards of X that every reference version is held to float64 on (the smallest batch of any route)
POOL = 128                  # X = the first n boards of a side's pool, Y = n boards from POOL on

Route = collections.namedtuple("Route", "kind side blocks arith uniform n")
Answers = collections.namedtuple("Answers", "px vx py vy")


def _init(kind, side, blocks, seed):
    return weights.init_params(kind, side, side, 9, blocks, 128, seed=seed, style="bench")


def _net(route, prm=None, batch=None):
    from alphapig_amd.policy_value_net import PolicyValueNet
    if prm is None:
        prm = _init(route.kind, route.side, route.blocks, STANDIN_SEED)
    return PolicyValueNet(route.side, route.side, batch_size=batch or max(route.n, 8), n_blocks=route.blocks, n_filter=128,
                          model_params=prm, net_kind=route.kind, trunk_arith=route.arith, uniform_trunk=route.uniform)


def _graphs(net, on):
    net._ck(net.L.apz_set_forward_graphs(net._h, int(on)))


@pytest.fixture(scope="module")
def lab():
    """Shared, read-only: weight sets on the host and as CUDA tensors, position pools, float64 oracles, reference answers."""
    torch = pytest.importorskip("torch")
    host, dev, pools, oracles, refs = {}, {}, {}, {}, {}

    class Lab(object):
        def host_sets(self, kind, side, blocks):
            key = (kind, side, blocks)
            if key not in host:
                host[key] = tuple(_init(kind, side, blocks, s) for s in SEEDS)
            return host[key]

        def dev_sets(self, kind, side, blocks):
            key = (kind, side, blocks)
            if key not in dev:
                dev[key] = tuple({k: torch.tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
                                  for k, v in prm.items()} for prm in self.host_sets(*key))
                torch.cuda.synchronize()
            return dev[key]

        def pool(self, side):
            """-> (codes, planes) of 2 * POOL boards (15x15, 8x8) or of the 70 boards of tests/test_gpu_frame_boards.py"""
            if side not in pools:
                if side in (15, 8):
                    pools[side] = random_positions(2 * POOL, side, seed=500 + side)
                else:
                    from test_gpu_frame_boards import positions
                    pools[side] = positions(side)
            return pools[side]

        def batches(self, side, n):
            codes = self.pool(side)[0]
            half = POOL if side in (15, 8) else len(codes) - n
            return codes[:n], codes[half:half + n]

        def oracle(self, kind, side, blocks, k):
            key = (kind, side, blocks, k)
            if key not in oracles:
                oracles[key] = net_ref.forward(self.host_sets(kind, side, blocks)[k], self.pool(side)[1][:N_ORACLE], kind,
                                               blocks, np.float64)
            return oracles[key]

        def refs(self, route):
            """-> K Answers, one per weight set: what a single-version evaluator says to X and Y of this route"""
            if route not in refs:
                X, Y = self.batches(route.side, route.n)
                out = []
                for k, tensors in enumerate(self.dev_sets(route.kind, route.side, route.blocks)):
                    ref = _net(route)
                    _graphs(ref, 0)
                    ref.load_device_params(tensors)
                    ref.sync()
                    ref.submit_codes_slot(0, X)
                    px, vx = ref.wait_slot(0, route.n)
                    ref.submit_codes_slot(1, Y)
                    py, vy = ref.wait_slot(1, route.n)
                    assert ref.trunk_overflows() == 0
                    # the reference itself against float64: its answer's first boards, and the logits behind them
                    o = self.oracle(route.kind, route.side, route.blocks, k)
                    m = N_ORACLE
                    lg, pr, vl, vv = ref.forward_with_logits(np.array(self.pool(route.side)[1][:m]))
                    e = (np.abs(lg - o[0]).max(), np.abs(vl - o[2][:, 0]).max(), np.abs(px[:m] - o[1]).max(),
                         np.abs(vx[:m] - o[3][:, 0]).max(), np.abs(pr - o[1]).max(), np.abs(vv - o[3][:, 0]).max())
                    print("%s set %d: logits %.2e value logit %.2e probs %.2e values %.2e (slot answer), %.2e %.2e" %
                          ((tuple(route), k) + e))
                    assert e[0] <= LOGIT_ATOL and e[1] <= LOGIT_ATOL and max(e[2:]) <= 2e-5
                    ref.close()
                    out.append(Answers(px, vx, py, vy))
                for a in range(K):                       # the sets are told apart by the bytes of either answer
                    for b in range(a + 1, K):
                        assert float(np.abs(out[a].px - out[b].px).max()) > 0 and float(np.abs(out[a].py - out[b].py).max()) > 0
                refs[route] = tuple(out)
            return refs[route]

        def loaded(self, route, k=0, batch=None):
            """an evaluator of this route holding set k: stand-in host load, device refresh, drained"""
            net = _net(route, batch=batch)
            net.load_device_params(self.dev_sets(route.kind, route.side, route.blocks)[k])
            net.sync()
            return net

    yield Lab()
    dev.clear()


def _same(got, p, v, what):
    np.testing.assert_array_equal(got[0], p, err_msg=what + ": probabilities")
    np.testing.assert_array_equal(got[1], v, err_msg=what + ": values")


class Refresher(object):
    """The three ways a caller hands apz_load_weights_dev its stream.  "fresh": a non-default torch stream on which the
    source tensors are cloned immediately before the call, with no host synchronisation -- the packing kernels are ordered
    behind the clone only by running on that stream.  Every source dict stays alive until drop(), after net.sync()."""

    def __init__(self, mode):
        import torch
        self.torch, self.mode, self.keep = torch, mode, []
        self.side = torch.cuda.Stream() if mode == "fresh" else None

    def __call__(self, net, tensors):
        torch = self.torch
        if self.mode == "default":
            net.load_device_params(tensors)
        elif self.mode == "current":
            net.load_device_params(tensors, torch.cuda.current_stream().cuda_stream)
        else:
            with torch.cuda.stream(self.side):
                clone = {k: v.clone() for k, v in tensors.items()}
            self.keep.append(clone)
            net.load_device_params(clone, self.side.cuda_stream)

    def drop(self, net):
        net.sync()
        if self.side is not None:
            self.side.synchronize()
        del self.keep[:]


# ---- 1. queued forwards keep their weights
ROUTES = [Route("resnet", 15, 3, "f32", False, 5),          # small-batch kernel
          Route("resnet", 15, 3, "f32", False, 40),         # batched
          Route("resnet", 15, 3, "f16x2", False, 40),
          Route("resnet", 15, 3, "f16x2", True, 5),         # uniform_trunk: the small-batch form of the f16x2 kernel
          Route("resnet", 15, 3, "bf16x3", False, 40),
          Route("simple", 8, 0, "f32", False, 20),
          Route("simple", 8, 0, "f16x2", False, 40),        # conv8h
          Route("resnet", 13, 3, "f16x2", False, 40),       # framed
          Route("resnet", 9, 3, "f32", False, 5),           # framed
          # ~1 ms of queued forwards in front of packing kernels of tens of microseconds (README, per-layer times)
          Route("resnet", 15, 10, "f16x2", False, 128)]
CYCLES = 12


def _route_id(r):
    return "%s%d-b%d-%s%s-n%d" % (r.kind, r.side, r.blocks, r.arith, "-uniform" if r.uniform else "", r.n)


@pytest.mark.parametrize("mode", ["default", "current", "fresh"])
@pytest.mark.parametrize("route", ROUTES, ids=_route_id)
def test_queued_forwards_keep_their_weights(lab, route, mode):
    """Slots 0 and 1 are submitted, the refresh to the next version is called, slots 2 and 3 are submitted, then all four
    are collected: the first two carry the previous version's bits, the last two the new version's -- 12 times over,
    the versions cycling through the K sets."""
    refs = lab.refs(route)
    tensors = lab.dev_sets(route.kind, route.side, route.blocks)
    X, Y = lab.batches(route.side, route.n)
    net = lab.loaded(route, 0)
    refresh = Refresher(mode)
    cur = 0
    for cycle in range(CYCLES):
        nxt = (cur + 1) % K
        net.submit_codes_slot(0, X)
        net.submit_codes_slot(1, Y)
        refresh(net, tensors[nxt])
        net.submit_codes_slot(2, X)
        net.submit_codes_slot(3, Y)
        got = [net.wait_slot(s, route.n) for s in range(4)]
        tag = "cycle %d, set %d -> %d, " % (cycle, cur, nxt)
        _same(got[0], refs[cur].px, refs[cur].vx, tag + "slot 0 (before the refresh)")
        _same(got[1], refs[cur].py, refs[cur].vy, tag + "slot 1 (before the refresh)")
        _same(got[2], refs[nxt].px, refs[nxt].vx, tag + "slot 2 (after the refresh)")
        _same(got[3], refs[nxt].py, refs[nxt].vy, tag + "slot 3 (after the refresh)")
        assert float(np.abs(refs[nxt].px - refs[cur].px).max()) > 0          # the refresh changed something
        cur = nxt
    assert net.trunk_overflows() == 0
    refresh.drop(net)
    net.close()


# ---- 2. the same with replayed graphs
@pytest.mark.parametrize("n", [7, 32])
@pytest.mark.parametrize("kind,side,blocks", [("resnet", 15, 3), ("simple", 8, 0)])
def test_replayed_graphs_keep_their_weights(lab, kind, side, blocks, n):
    """apz_set_forward_graphs on: the third submission of a (slot, n) pair captures, later ones replay.  The refresh drops
    graph executables whose last replay may still be running; that replay answers with the old version, and the graphs
    captured afterwards hold the new weights.  References: plain launches (graphs off)."""
    import torch
    route = Route(kind, side, blocks, "auto", False, n)
    refs = lab.refs(route)
    tensors = lab.dev_sets(kind, side, blocks)
    X, Y = lab.batches(side, n)
    net = lab.loaded(route, 0)
    _graphs(net, 1)
    side_stream = torch.cuda.Stream()

    def expect(got, k, slot, tag):
        r = refs[k]
        _same(got, *((r.px, r.vx) if slot % 2 == 0 else (r.py, r.vy)), what="%s, slot %d, set %d" % (tag, slot, k))

    for rep in range(5):                         # 1, 2: plain; 3: captured and launched; 4, 5: replayed
        for slot in range(4):
            net.submit_codes_slot(slot, X if slot % 2 == 0 else Y)
            expect(net.wait_slot(slot, n), 0, slot, "submission %d" % (rep + 1))
    net.submit_codes_slot(0, X)                  # the sixth: replays queued in front of the refresh ...
    net.submit_codes_slot(1, Y)
    net.load_device_params(tensors[1], side_stream.cuda_stream)
    net.submit_codes_slot(2, X)                  # ... and plain launches behind it
    net.submit_codes_slot(3, Y)
    got = [net.wait_slot(s, n) for s in range(4)]
    for slot in range(4):
        expect(got[slot], 0 if slot < 2 else 1, slot, "across the refresh")
    assert float(np.abs(refs[1].px - refs[0].px).max()) > 0
    for rep in range(5):                         # captured again, on the new weights
        for slot in range(4):
            net.submit_codes_slot(slot, X if slot % 2 == 0 else Y)
            expect(net.wait_slot(slot, n), 1, slot, "submission %d after the refresh" % (rep + 1))
    net.sync()
    side_stream.synchronize()
    net.close()


# ---- 3. two host threads
N_VERSIONS = 9              # versions 0 .. 8, version v holds set v % K
PER_VERSION = 5             # completed submissions between two refreshes


def test_submitter_and_refresher_threads_see_versions_in_order(lab):
    """The main thread keeps two submissions in flight on alternating slots; a second thread installs versions 1 .. 8 on
    its own torch stream, each after the main thread has completed five more submissions (a handshake on a condition
    variable, no sleeping), while the main thread goes on submitting.  Every answer is one set's reference, looked up by
    its bytes; consecutive answers hold the same set or the next one, so the versions (version v holds set v % 4) never
    go backwards and none is missing; the first answer is version 0, the last two -- submitted after the join -- are 8."""
    import torch
    route = Route("resnet", 15, 3, "f16x2", False, 40)
    refs = lab.refs(route)
    tensors = lab.dev_sets(route.kind, route.side, route.blocks)
    X, Y = lab.batches(route.side, route.n)
    by_bytes = {}
    for k, r in enumerate(refs):
        by_bytes[(0, r.px.tobytes(), r.vx.tobytes())] = k
        by_bytes[(1, r.py.tobytes(), r.vy.tobytes())] = k
    assert len(by_bytes) == 2 * K
    net = lab.loaded(route, 0)
    cond = threading.Condition()
    state = {"done": 0, "finished": False, "abort": False, "error": None, "installed_at": []}

    def refresher():
        try:
            stream = torch.cuda.Stream()
            last = 0
            for v in range(1, N_VERSIONS):
                with cond:
                    cond.wait_for(lambda: state["done"] >= last + PER_VERSION or state["abort"])
                    if state["abort"]:
                        return
                net.load_device_params(tensors[v % K], stream.cuda_stream)
                with cond:
                    last = state["done"]
                    state["installed_at"].append(last)
            stream.synchronize()
        except Exception as exc:                 # reported by the main thread
            state["error"] = exc
        finally:
            with cond:
                state["finished"] = True

    seen = []                                    # set index per submission, in submission order

    def collect(i):
        got = net.wait_slot(i % 2, route.n)
        key = (i % 2, got[0].tobytes(), got[1].tobytes())
        assert key in by_bytes, "submission %d is no single version's answer" % i
        seen.append(by_bytes[key])
        with cond:
            state["done"] += 1
            cond.notify_all()

    th = threading.Thread(target=refresher)
    th.start()
    try:
        i = 0
        while True:
            with cond:
                if state["finished"]:
                    break
            assert i < 100000, "the refresher thread never finished"
            if i >= 2:
                collect(i - 2)
            net.submit_codes_slot(i % 2, X if i % 2 == 0 else Y)
            i += 1
        for j in range(max(i - 2, 0), i):
            collect(j)
    finally:
        with cond:
            state["abort"] = True
            cond.notify_all()
        th.join()
    assert state["error"] is None, state["error"]
    for j in range(i, i + 2):                    # after the join: version 8
        net.submit_codes_slot(j % 2, X if j % 2 == 0 else Y)
        collect(j)
    versions, v = [], 0
    for j, k in enumerate(seen):
        if k != v % K:
            assert k == (v + 1) % K, "submission %d answers with set %d after version %d: %s" % (j, k, v, seen)
            v += 1
        versions.append(v)
    print("installed after completed submission", state["installed_at"])
    print("versions per submission", "".join(str(x) for x in versions))
    assert seen[0] == 0
    assert versions[-2:] == [N_VERSIONS - 1] * 2, versions
    assert sorted(set(versions)) == list(range(N_VERSIONS)), versions
    assert net.trunk_overflows() == 0
    net.sync()
    net.close()


# ---- 4. lanes
@pytest.mark.parametrize("kind,side,blocks,n", [("simple", 8, 0, 32), ("resnet", 15, 3, 40)])
def test_lanes_are_refreshed_between_submissions(lab, kind, side, blocks, n):
    """TrainPipeline._install_weights on a LanedEvaluator of two lanes, from the submitting thread: four slots in flight
    before the refresh come back with the old version, four submitted after it with the new one -- X and Y on both lanes
    (slot s runs on lane s % 2)."""
    import torch
    from alphapig_amd.policy_value_net import LanedEvaluator
    route = Route(kind, side, blocks, "auto", False, n)
    refs = lab.refs(route)
    tensors = lab.dev_sets(kind, side, blocks)
    X, Y = lab.batches(side, n)
    laned = LanedEvaluator([lab.loaded(route, 0), lab.loaded(route, 0)])
    codes = [X, Y, Y, X]

    def expect(got, k, tag):
        r = refs[k]
        for slot in range(4):
            _same(got[slot], *((r.px, r.vx) if codes[slot] is X else (r.py, r.vy)), what="%s, slot %d, set %d" % (tag, slot, k))

    cur = 0
    for cycle in range(K):
        nxt = (cur + 1) % K
        for slot in range(4):
            laned.submit_codes_slot(slot, codes[slot])
        laned.load_device_params(tensors[nxt], torch.cuda.current_stream().cuda_stream)
        expect([laned.wait_slot(s, n) for s in range(4)], cur, "cycle %d, in flight before the refresh" % cycle)
        for slot in range(4):
            laned.submit_codes_slot(slot, codes[slot])
        expect([laned.wait_slot(s, n) for s in range(4)], nxt, "cycle %d, submitted after the refresh" % cycle)
        cur = nxt
    laned.sync()
    laned.close()


# ---- 5. the trainer's hand-off
def test_trainer_hand_off_without_a_host_synchronisation():
    """HipTrainer.train_step, at once sync_evaluator(net), at once one evaluation by net: the bits of a reference evaluator
    refreshed from the same trainer after torch.cuda.synchronize().  The packing kernels run behind Adam on the trainer's
    stream and the engine's stream behind them.  (train_step reads the loss back behind Adam, so Adam has finished when
    it returns; what is left to order here is the packing against the evaluation.  tests/test_gpu_train.py::
    test_net_train_step_updates_the_selfplay_evaluator compares the parameter tables after such a hand-off, not an
    evaluation against a single-version evaluator.)"""
    import torch
    from alphapig_amd.policy_value_net import PolicyValueNet
    from alphapig_amd.train import HipTrainer
    n, blocks = 8, 2
    rs = np.random.RandomState(17)
    prm = _init("resnet", 15, blocks, SEEDS[0])
    codes, planes = random_positions(n, 15, seed=515)
    pis = rs.dirichlet(np.ones(225), size=n).astype(np.float32)
    zs = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    tr = HipTrainer(prm, "resnet", n_blocks=blocks, batch_size=n, dropout=0.5, seed=3)
    net = PolicyValueNet(15, 15, batch_size=n, n_blocks=blocks, n_filter=128, model_params=prm)
    ref = PolicyValueNet(15, 15, batch_size=n, n_blocks=blocks, n_filter=128, model_params=prm)
    net.submit_codes_slot(0, codes)
    before = net.wait_slot(0, n)
    tr.train_step(planes, pis, zs, 2e-3)
    tr.sync_evaluator(net)
    net.submit_codes_slot(0, codes)
    got = net.wait_slot(0, n)
    torch.cuda.synchronize()
    tr.sync_evaluator(ref)
    ref.sync()
    ref.submit_codes_slot(0, codes)
    want = ref.wait_slot(0, n)
    _same(got, want[0], want[1], "after train_step + sync_evaluator")
    assert float(np.abs(got[0] - before[0]).max()) > 0
    o = net_ref.forward(tr.get_params(), planes, "resnet", blocks, np.float64)
    assert np.abs(want[0] - o[1]).max() <= 2e-5 and np.abs(want[1] - o[3][:, 0]).max() <= 2e-5
    tr.close()
    net.close()
    ref.close()


# ---- 6. an overflowed batch across a refresh
def test_overflowed_batch_is_repeated_on_the_weights_installed_at_the_wait(lab):
    """apz_wait repeats an overflowed f16x2 batch on the exact kernel when it is collected (csrc/apz_engine.hip: the repeat
    is queued on the engine's stream by apz_wait, behind everything apz_load_weights_dev ordered in front of it): submitted
    under the old version (conv1_weight x 1e6, tests/test_gpu_conv8.py), refreshed, then waited for, the batch comes back
    finite with the bits of a trunk_arith="f32" evaluator of the NEW version, and trunk_overflows() advances by one --
    include/alphapig_hip.h says so at apz_wait."""
    import torch
    n = 40
    route = Route("simple", 8, 0, "f16x2", False, n)
    exact = lab.refs(route._replace(arith="f32"))
    tensors = lab.dev_sets("simple", 8, 0)
    X, _ = lab.batches(8, n)
    big = dict(tensors[0])
    big["conv1_weight"] = tensors[0]["conv1_weight"] * 1.0e6
    torch.cuda.synchronize()
    net = _net(route)
    net.load_device_params(big)
    net.sync()
    side_stream = torch.cuda.Stream()
    count = net.trunk_overflows()
    net.submit_codes_slot(0, X)
    net.load_device_params(tensors[1], side_stream.cuda_stream)
    p, v = net.wait_slot(0, n)
    assert net.trunk_overflows() == count + 1
    assert np.isfinite(p).all() and np.isfinite(v).all()
    _same((p, v), exact[1].px, exact[1].vx, "the repeat of the overflowed batch")
    # the old version's exact answer is another one, so the comparison above tells the two apart
    old = _net(route._replace(arith="f32"))
    old.load_device_params(big)
    old.sync()
    old.submit_codes_slot(0, X)
    po, _ = old.wait_slot(0, n)
    assert np.isfinite(po).all() and float(np.abs(po - p).max()) > 0
    # and ordinary batches afterwards: the new version's f16x2 bits, no repeat
    split = lab.refs(route)
    net.submit_codes_slot(1, X)
    _same(net.wait_slot(1, n), split[1].px, split[1].vx, "the next batch")
    assert net.trunk_overflows() == count + 1
    net.sync()
    side_stream.synchronize()
    old.close()
    net.close()
